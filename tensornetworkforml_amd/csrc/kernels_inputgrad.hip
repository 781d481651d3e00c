// Input gradients (tnml_input_grad / tnml_input_grad_indices):
//   g[s][i][d] = sum_l' cot[l'][s] d f[l'][s] / d x[s][i][d]     for every sample s, site i and feature d
// f is linear in every x[s][i][:] separately, so with P_i[a] the contraction of sites 0 .. i-1 and Q_i[c] that of sites
// i+1 .. N-1 (the open label axis contracted with cot[:, s] at the label site l, P_0 = Q_{N-1} = 1):
//   pass A, i = 0 .. N-2:   P_{i+1}[c] = sum_{a,d} P_i[a] x_i[d] A_i[a][d][c]                 (at i = l: ... cot[l'] A_l[a][d][c][l'])
//   pass B, i = N-1 .. 0:   T[a][d]    = sum_c A_i[a][d][c] Q_i[c]                            (at i = l: ... A_l[a][d][c][l'] cot[l'])
//                           g[i][d]    = sum_a P_i[a] T[a][d]
//                           Q_{i-1}[a] = sum_d x_i[d] T[a][d]
//   after i = 0:            cf = Q_{-1} = sum_l' cot[l'] f[l']
// One kernel runs both passes.  A workgroup of four waves owns 64 samples, each wave 16 of them as the rows of its
// v_mfma_f32_16x16x4_f32 tiles (the form of anyd_chain_kernel); samples never meet, so there is no communication between
// workgroups.  The site's core is staged in LDS as the plain matrix [(a, d)][c]: pass A reads it as the B operand of
// (P (x) x) . A, pass B reads the same image transposed as the B operand of Q . A^T.  Pass A stores P_1 .. P_{N-1} to an HBM
// stack [N][cap][b_pad] (the library's [m][b_pad] environment layout); pass B reads it back in reverse, keeps Q in LDS and
// writes g straight into [b][N][D].  The label core is taken one label slice at a time (at bond 50 and ten labels it is 200 KB),
// the slices accumulate in the LDS tile that receives the product.
//
// LDS (floats; mb = largest bond of the chain):  core image mb D x (mb | 1);  two environment tiles mb x 81;  x 64 x D;
// cot L x 64;  T 64 x (mb D | 1);  the bond table, N + 1 ints.  ds_read_b32 / ds_write_b32 bank over 32 dwords per 32-lane half (lanes 0-31 = k-quarters 0 and
// 1 of an MFMA operand fetch):
//   environment tiles, row stride 81: the operand fetch reads 16 consecutive samples of rows k and k + 1 (17 banks apart: one
//     2-way collision; at a row stride of 64 every fetch of pass B would be 2-way); the accumulator store walks 16 rows at one
//     sample: 17 o mod 32 is distinct for the 16 rows, 2-way against the second k-quarter;
//   core image, odd row stride: row-wise (pass A) 16 consecutive banks per k-quarter, transposed (pass B) r * stride mod 32 is
//     distinct for the 16 rows; at most 2-way between the two k-quarters;
//   T, odd row stride: the store puts 16 consecutive columns of rows 4 q + r, the two reads walk 16 rows at one column;
//     at most 2-way.
#include "tnml_internal.h"

namespace tnml {

typedef float ig_f4 __attribute__((ext_vector_type(4)));

constexpr int kIgTS = 64;          // samples per workgroup
constexpr int kIgLd = 81;          // row stride of the environment tiles in LDS

// Two 16 x 16 output tiles that share their A operand, K in steps of 4 (operand and accumulator layout: anyd_mfma_tile of
// kernels_anyd.hip): A[i][k] = fa(k) of row i = lane & 15, B[k][j] = fb0(k) / fb1(k) of column j = lane & 15; fa receives k as
// (k / D, k % D), kept by increments.  acc[r] holds row 4 * (lane >> 4) + r, column lane & 15 (v_mfma_f32_16x16x4_f32).
template <class FA, class FB0, class FB1>
__device__ inline void ig_mfma_pair(int K, int D, FA fa, FB0 fb0, FB1 fb1, ig_f4 &acc0, ig_f4 &acc1) {
  const int kq = (threadIdx.x & 63) >> 4;
  int a = 0, d = kq;
  while (d >= D) { d -= D; ++a; }
  acc0 = {0.f, 0.f, 0.f, 0.f};
  acc1 = {0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < K; k0 += 4) {
    const int k = k0 + kq;
    float av = 0.f, b0 = 0.f, b1 = 0.f;
    if (k < K) { av = fa(k, a, d); b0 = fb0(k); b1 = fb1(k); }
    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b0, acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b1, acc1, 0, 0, 0);
    d += 4;
    while (d >= D) { d -= D; ++a; }
  }
}

size_t input_grad_lds_bytes(int mb, int D, int L, int N) {
  const size_t ldA = (size_t)mb | 1, ldT = ((size_t)mb * D) | 1;
  return ((size_t)mb * D * ldA + 2 * (size_t)mb * kIgLd + (size_t)kIgTS * D + (size_t)L * kIgTS + (size_t)kIgTS * ldT) * sizeof(float) +
         (size_t)(N + 1) * sizeof(int);
}

__global__ __launch_bounds__(256) void input_grad_kernel(InputGradParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int D = p.D, L = p.L, N = p.N, mb = p.mb, lp = p.l_pos;
  const int ldA = mb | 1, ldT = (mb * D) | 1;
  float *sA = (float *)smem_raw;                           // [ml D][ldA]  core of the site (one label slice of the label core)
  float *sE0 = sA + (size_t)mb * D * ldA;                  // [mb][kIgLd]
  float *sE1 = sE0 + (size_t)mb * kIgLd;                   // [mb][kIgLd]
  float *sX = sE1 + (size_t)mb * kIgLd;                    // [64][D]
  float *sCot = sX + (size_t)kIgTS * D;                    // [L][64]
  float *sT = sCot + (size_t)L * kIgTS;                    // [64][ldT]
  int *sBond = (int *)(sT + (size_t)kIgTS * ldT);          // [N + 1]: 1, bond[0 .. N-2], 1 (a site's two bonds without a trip to memory)
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r16 = lane & 15, part = lane >> 4;
  const int s0 = blockIdx.x * kIgTS, sw = wave * 16;       // sw: this wave's samples
  for (int e = tid; e <= N; e += 256) sBond[e] = (e == 0 || e == N) ? 1 : p.bond[e - 1];
  auto bond_l = [&](int i) { return sBond[i]; };
  auto bond_r = [&](int i) { return sBond[i + 1]; };
  auto stage = [&](int i, int sl, int ml, int mr) {
    const int n = ml * D * mr, qk = 256 / mr, qc = 256 % mr;
    int k = tid / mr, c = tid % mr;                          // (row, column) of element e, kept by increments
    const float *src = i == lp ? p.labcore + sl : p.cores + (size_t)i * p.core_stride;
    const size_t step = i == lp ? (size_t)L : 1;
    for (int e = tid; e < n; e += 256) {
      sA[k * ldA + c] = src[(size_t)e * step];
      k += qk; c += qc;
      if (c >= mr) { c -= mr; ++k; }
    }
  };
  auto load_x = [&](int i) {
    for (int e = tid; e < kIgTS * D; e += 256) sX[e] = p.X[((size_t)i * p.x_bpad + s0) * D + e];
  };
  for (int e = tid; e < L * kIgTS; e += 256) sCot[e] = p.cot[(size_t)(e / kIgTS) * p.b_pad + s0 + e % kIgTS];
  if (tid < kIgTS) sE0[tid] = 1.f;
  __syncthreads();

  // ---- pass A: P_1 .. P_{N-1} to the stack ------------------------------------------------------
  float *ein = sE0, *eout = sE1;
  for (int i = 0; i < N - 1; ++i) {
    const int ml = bond_l(i), mr = bond_r(i), K = ml * D, nsl = i == lp ? L : 1;
    for (int sl = 0; sl < nsl; ++sl) {
      __syncthreads();                                       // the core image and x of the previous product are free
      stage(i, sl, ml, mr);
      if (sl == 0) load_x(i);
      __syncthreads();
      const float crv = i == lp ? sCot[sl * kIgTS + sw + r16] : 1.f, *xs = sX + (sw + r16) * D, *es = ein + sw + r16;
      for (int ot = 0; ot < (mr + 15) / 16; ot += 2) {
        const int o0 = ot * 16 + r16, o1 = o0 + 16;
        ig_f4 acc0, acc1;
        ig_mfma_pair(
            K, D, [&](int, int a, int d) { return es[a * kIgLd] * xs[d] * crv; },
            [&](int k) { return o0 < mr ? sA[k * ldA + o0] : 0.f; }, [&](int k) { return o1 < mr ? sA[k * ldA + o1] : 0.f; }, acc0, acc1);
        for (int r = 0; r < 4; ++r) {
          const int col = sw + 4 * part + r;
          if (o0 < mr) eout[o0 * kIgLd + col] = sl ? eout[o0 * kIgLd + col] + acc0[r] : acc0[r];
          if (o1 < mr) eout[o1 * kIgLd + col] = sl ? eout[o1 * kIgLd + col] + acc1[r] : acc1[r];
        }
      }
    }
    __syncthreads();
    float *dst = p.stack + (size_t)(i + 1) * p.cap * p.b_pad + s0;
    for (int e = tid; e < mr * kIgTS; e += 256) dst[(size_t)(e / kIgTS) * p.b_pad + e % kIgTS] = eout[(e / kIgTS) * kIgLd + e % kIgTS];
    float *t = ein; ein = eout; eout = t;
  }

  // ---- pass B: T = Q . A^T, g, Q of the next site to the left -----------------------------------
  __syncthreads();
  float *sP = sE0, *sQ = sE1;
  if (tid < kIgTS) sQ[tid] = 1.f;
  for (int i = N - 1; i >= 0; --i) {
    const int ml = bond_l(i), mr = bond_r(i), J = ml * D, nsl = i == lp ? L : 1;
    for (int sl = 0; sl < nsl; ++sl) {
      __syncthreads();                                       // Q of this site is complete; core image, x, P and T are free
      stage(i, sl, ml, mr);
      if (sl == 0) {
        load_x(i);
        if (i == 0) {
          if (tid < kIgTS) sP[tid] = 1.f;
        } else {
          const float *src = p.stack + (size_t)i * p.cap * p.b_pad + s0;
          for (int e = tid; e < ml * kIgTS; e += 256) sP[(e / kIgTS) * kIgLd + e % kIgTS] = src[(size_t)(e / kIgTS) * p.b_pad + e % kIgTS];
        }
      }
      __syncthreads();
      const float crv = i == lp ? sCot[sl * kIgTS + sw + r16] : 1.f, *qs = sQ + sw + r16;
      for (int jt = 0; jt < (J + 15) / 16; jt += 2) {
        const int j0 = jt * 16 + r16, j1 = j0 + 16;
        ig_f4 acc0, acc1;
        ig_mfma_pair(
            mr, D, [&](int k, int, int) { return qs[k * kIgLd] * crv; },
            [&](int k) { return j0 < J ? sA[j0 * ldA + k] : 0.f; }, [&](int k) { return j1 < J ? sA[j1 * ldA + k] : 0.f; }, acc0, acc1);
        for (int r = 0; r < 4; ++r) {
          float *row = sT + (sw + 4 * part + r) * ldT;
          if (j0 < J) row[j0] = sl ? row[j0] + acc0[r] : acc0[r];
          if (j1 < J) row[j1] = sl ? row[j1] + acc1[r] : acc1[r];
        }
      }
    }
    __syncthreads();
    // the two small contractions of this wave's 16 samples: lane = (sample r16, quarter `part` of the bond index a)
    const int s = sw + r16;
    const float *Ts = sT + (size_t)s * ldT;
    for (int d = 0; d < D; ++d) {
      float v = 0.f;
      for (int a = part; a < ml; a += 4) v = fmaf(sP[a * kIgLd + s], Ts[a * D + d], v);
      v += __shfl_xor(v, 16);
      v += __shfl_xor(v, 32);
      if (part == 0 && s0 + s < p.b) p.g[((size_t)(s0 + s) * N + i) * D + d] = v;
    }
    // (a wave reads and writes only its own samples of Q, and its products with Q are behind it)
    for (int a = part; a < ml; a += 4) {
      float v = 0.f;
      for (int d = 0; d < D; ++d) v = fmaf(sX[s * D + d], Ts[a * D + d], v);
      sQ[a * kIgLd + s] = v;
    }
  }
  __syncthreads();
  if (p.cf && tid < kIgTS && s0 + tid < p.b) p.cf[s0 + tid] = sQ[tid];
}

bool launch_input_grad(const InputGradParams &p, hipStream_t st) {
  if (p.b < 1 || p.b > p.b_pad || p.b_pad % kIgTS || p.x_bpad < p.b_pad || p.mb < 1 || p.mb > p.cap || p.D < 2 || p.D > kMaxD ||
      p.l_pos < 0 || p.l_pos >= p.N)
    return false;
  const size_t lds = input_grad_lds_bytes(p.mb, p.D, p.L, p.N);
  if (lds > 160 * 1024) return false;
  hipLaunchKernelGGL(input_grad_kernel, dim3((p.b + kIgTS - 1) / kIgTS), dim3(256), lds, st, p);
  return true;
}

// ------------------------------------------------------------------------------------------
// cot[l'][s] = (l' == first maximum of f[:, s]) for s < b, 0 beyond: the rule of act_and_lossder (act_device.h)
// ------------------------------------------------------------------------------------------
__global__ void input_grad_onehot_kernel(const float *__restrict__ f, int f_bpad, int L, int b, float *__restrict__ cot, int b_pad) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= b_pad) return;
  int am = -1;
  if (s < b) {
    am = 0;
    float best = f[s];
    for (int l = 0; l < L; ++l) {
      const float fv = f[(size_t)l * f_bpad + s];
      if (fv > best) { best = fv; am = l; }
    }
  }
  for (int l = 0; l < L; ++l) cot[(size_t)l * b_pad + s] = l == am ? 1.f : 0.f;
}

bool launch_input_grad_onehot(const float *f, int f_bpad, int L, int b, float *cot, int b_pad, hipStream_t st) {
  if (b < 1 || b > b_pad || b_pad > f_bpad || L < 1) return false;
  hipLaunchKernelGGL(input_grad_onehot_kernel, dim3((b_pad + 255) / 256), dim3(256), 0, st, f, f_bpad, L, b, cot, b_pad);
  return true;
}

// ------------------------------------------------------------------------------------------
// chain rule through the pixel feature map (kernels_dataset.hip): out[s][i] = sum_k g[s][i][k] dpsi_k / dp at the pixel of
// sample idx[s], site i;  psi_k(p) = coef_k sin^(D-1-k)(pi p / 2) cos^k(pi p / 2),
//   dpsi_k / dp = (pi / 2) coef_k [(D-1-k) sin^(D-2-k) cos^(k+1) - k sin^(D-k) cos^(k-1)]
// in float64 with one rounding of the sum; a term whose integer factor is 0 is dropped, not evaluated
// ------------------------------------------------------------------------------------------
__device__ inline double ig_powi(double v, int k) {
  double r = 1.0;
  for (int i = 0; i < k; ++i) r *= v;
  return r;
}

__global__ void input_grad_pixels_kernel(InputGradPixels p) {
  const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (size_t)p.b * p.N) return;
  const int s = (int)(e / p.N), i = (int)(e - (size_t)s * p.N), D = p.D;
  const double a = 3.141592653589793 * (double)p.data[(size_t)p.idx[s] * p.N + i] / 2;
  const double sn = sin(a), cs = cos(a);
  double acc = 0.0;
  for (int k = 0; k < D; ++k) {
    double t = 0.0;
    if (D - 1 - k > 0) t += (double)(D - 1 - k) * ig_powi(sn, D - 2 - k) * ig_powi(cs, k + 1);
    if (k > 0) t -= (double)k * ig_powi(sn, D - k) * ig_powi(cs, k - 1);
    acc += (double)p.g[e * D + k] * (1.5707963267948966 * p.coef[k] * t);
  }
  p.out[e] = (float)acc;
}

bool launch_input_grad_pixels(const InputGradPixels &p, hipStream_t st) {
  if (p.b < 1 || p.N < 1 || p.D < 2 || p.D > kMaxD) return false;
  const size_t n = (size_t)p.b * p.N;
  hipLaunchKernelGGL(input_grad_pixels_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, p);
  return true;
}

}  // namespace tnml
