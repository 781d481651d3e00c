// Core gradients (tnml_core_grad / tnml_core_grad_indices): the derivative of sum_s cf[s],
// cf[s] = sum_l' cot[l'][s] f[l'][s], with respect to every core at once.  With P_i[s][a] the contraction of sites 0 .. i-1 and
// Q_i[s][c] that of sites i+1 .. N-1 of sample s (P_0 = Q_{N-1} = 1; the chain that has passed the label site l carries cot):
//   G_i[a][d][c]     = sum_s P_i[s][a] x_i[s][d] Q_i[s][c]                    i != l
//   G_l[a][d][c][l'] = sum_s cot[l'][s] P_l[s][a] x_l[s][d] Q_l[s][c]         (P_l and Q_l are free of cot)
// Two kernels per chunk of samples:
//   core_grad_chain_kernel   the two passes of input_grad_kernel (kernels_inputgrad.hip: same tiles, same LDS image, same bank
//                            argument) without g and without the re-read of P: pass A stores P_1 .. P_{N-1} to one HBM stack
//                            [N][cap][b_pad], pass B stores Q_{N-2} .. Q_0 to a second one and leaves cf.
//   core_grad_reduce_kernel  the sum over samples, parallel over sites: for a site one GEMM with K = samples,
//                            (P_i (x) x_i)^T [ml D x samples] . Q_i^T [samples x mr], at the label site one per label slice with
//                            cot[l'][s] folded into x.  Grid (site, block of output tiles, label slice).  A wave owns two
//                            16 x 16 output tiles side by side (one A operand, two B operands, v_mfma_f32_16x16x4_f32) and walks
//                            ALL samples of the chunk in ascending order, 64 at a time through LDS; the accumulators of a chunk
//                            after the first start from G, so that every element is one fixed left-to-right sum whatever the
//                            chunk size.  No atomics, no split of the sample axis.
//
// LDS of the reduction (floats): P tile mb x 65, Q tile mb x 65, x tile 64 x D.  The stacks are sample-contiguous, so the tiles are
// filled by coalesced loads (a thread's element e -> row e / 64, sample e % 64: 64 consecutive banks per row, conflict-free
// writes).  ds_read_b32 banks over 32 dwords per 32-lane half (lanes 0-31 = k-quarters 0 and 1 of an operand fetch):
//   P tile, row stride 65: a lane reads row a = (row of the output tile) / D at sample k: bank (a + k) mod 32.  The 16 lanes of a
//     k-quarter touch at most 16 consecutive a (lanes with the same a read one address: broadcast), the second quarter the same
//     rows one sample on: at most 2-way.  At a row stride of 64 all rows of a quarter would share one bank.
//   Q tile, row stride 65: 16 consecutive rows c at sample k, bank (c + k) mod 32: the same argument, at most 2-way.
//   x tile: a half reads two samples x D features, at most 2 D <= 16 distinct addresses with 2 D consecutive banks: conflict-free.
#include "tnml_internal.h"

namespace tnml {

typedef float cg_f4 __attribute__((ext_vector_type(4)));

constexpr int kCgTS = 64;          // samples per workgroup of the chain kernel, and per LDS tile of the reduction
constexpr int kCgLd = 81;          // chain kernel: row stride of the environment tiles in LDS (input_grad_kernel's)
constexpr int kCgLdR = 65;         // reduction: row stride of the P and Q tiles

// Two 16 x 16 output tiles that share their A operand, K in steps of 4: ig_mfma_pair of kernels_inputgrad.hip.
template <class FA, class FB0, class FB1>
__device__ inline void cg_mfma_pair(int K, int D, FA fa, FB0 fb0, FB1 fb1, cg_f4 &acc0, cg_f4 &acc1) {
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

size_t core_grad_chain_lds_bytes(int mb, int D, int L, int N) {
  const size_t ldA = (size_t)mb | 1, ldT = ((size_t)mb * D) | 1;
  return ((size_t)mb * D * ldA + 2 * (size_t)mb * kCgLd + (size_t)kCgTS * D + (size_t)L * kCgTS + (size_t)kCgTS * ldT) * sizeof(float) +
         (size_t)(N + 1) * sizeof(int);
}

// ------------------------------------------------------------------------------------------
// chain kernel: four waves own 64 samples, each wave 16 of them as the rows of its MFMA tiles
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void core_grad_chain_kernel(CoreGradParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int D = p.D, L = p.L, N = p.N, mb = p.mb, lp = p.l_pos;
  const int ldA = mb | 1, ldT = (mb * D) | 1;
  float *sA = (float *)smem_raw;                           // [ml D][ldA]  core of the site (one label slice of the label core)
  float *sE0 = sA + (size_t)mb * D * ldA;                  // [mb][kCgLd]
  float *sE1 = sE0 + (size_t)mb * kCgLd;                   // [mb][kCgLd]
  float *sX = sE1 + (size_t)mb * kCgLd;                    // [64][D]
  float *sCot = sX + (size_t)kCgTS * D;                    // [L][64]
  float *sT = sCot + (size_t)L * kCgTS;                    // [64][ldT]
  int *sBond = (int *)(sT + (size_t)kCgTS * ldT);          // [N + 1]: 1, bond[0 .. N-2], 1
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r16 = lane & 15, part = lane >> 4;
  const int s0 = blockIdx.x * kCgTS, sw = wave * 16;       // sw: this wave's samples
  for (int e = tid; e <= N; e += 256) sBond[e] = (e == 0 || e == N) ? 1 : p.tab[e - 1];
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
    for (int e = tid; e < kCgTS * D; e += 256) sX[e] = p.X[((size_t)i * p.x_bpad + s0) * D + e];
  };
  for (int e = tid; e < L * kCgTS; e += 256) sCot[e] = p.cot[(size_t)(e / kCgTS) * p.b_pad + s0 + e % kCgTS];
  if (tid < kCgTS) sE0[tid] = 1.f;
  __syncthreads();

  // ---- pass A: P_1 .. P_{N-1} to the first stack ------------------------------------------------
  float *ein = sE0, *eout = sE1;
  for (int i = 0; i < N - 1; ++i) {
    const int ml = sBond[i], mr = sBond[i + 1], K = ml * D, nsl = i == lp ? L : 1;
    for (int sl = 0; sl < nsl; ++sl) {
      __syncthreads();                                       // the core image and x of the previous product are free
      stage(i, sl, ml, mr);
      if (sl == 0) load_x(i);
      __syncthreads();
      const float crv = i == lp ? sCot[sl * kCgTS + sw + r16] : 1.f, *xs = sX + (sw + r16) * D, *es = ein + sw + r16;
      for (int ot = 0; ot < (mr + 15) / 16; ot += 2) {
        const int o0 = ot * 16 + r16, o1 = o0 + 16;
        cg_f4 acc0, acc1;
        cg_mfma_pair(
            K, D, [&](int, int a, int d) { return es[a * kCgLd] * xs[d] * crv; },
            [&](int k) { return o0 < mr ? sA[k * ldA + o0] : 0.f; }, [&](int k) { return o1 < mr ? sA[k * ldA + o1] : 0.f; }, acc0, acc1);
        for (int r = 0; r < 4; ++r) {
          const int col = sw + 4 * part + r;
          if (o0 < mr) eout[o0 * kCgLd + col] = sl ? eout[o0 * kCgLd + col] + acc0[r] : acc0[r];
          if (o1 < mr) eout[o1 * kCgLd + col] = sl ? eout[o1 * kCgLd + col] + acc1[r] : acc1[r];
        }
      }
    }
    __syncthreads();
    float *dst = p.stackP + (size_t)(i + 1) * p.cap * p.b_pad + s0;
    for (int e = tid; e < mr * kCgTS; e += 256) dst[(size_t)(e / kCgTS) * p.b_pad + e % kCgTS] = eout[(e / kCgTS) * kCgLd + e % kCgTS];
    float *t = ein; ein = eout; eout = t;
  }

  // ---- pass B: Q_{N-2} .. Q_0 to the second stack; T = Q . A^T, Q of the next site to the left ---
  __syncthreads();
  float *sQ = sE1;
  if (tid < kCgTS) sQ[tid] = 1.f;
  for (int i = N - 1; i >= 0; --i) {
    const int ml = sBond[i], mr = sBond[i + 1], J = ml * D, nsl = i == lp ? L : 1;
    for (int sl = 0; sl < nsl; ++sl) {
      __syncthreads();                                       // Q of this site is complete; core image, x and T are free
      stage(i, sl, ml, mr);
      if (sl == 0) {
        load_x(i);
        if (i < N - 1) {
          float *dst = p.stackQ + (size_t)i * p.cap * p.b_pad + s0;
          for (int e = tid; e < mr * kCgTS; e += 256) dst[(size_t)(e / kCgTS) * p.b_pad + e % kCgTS] = sQ[(e / kCgTS) * kCgLd + e % kCgTS];
        }
      }
      __syncthreads();
      const float crv = i == lp ? sCot[sl * kCgTS + sw + r16] : 1.f, *qs = sQ + sw + r16;
      for (int jt = 0; jt < (J + 15) / 16; jt += 2) {
        const int j0 = jt * 16 + r16, j1 = j0 + 16;
        cg_f4 acc0, acc1;
        cg_mfma_pair(
            mr, D, [&](int k, int, int) { return qs[k * kCgLd] * crv; },
            [&](int k) { return j0 < J ? sA[j0 * ldA + k] : 0.f; }, [&](int k) { return j1 < J ? sA[j1 * ldA + k] : 0.f; }, acc0, acc1);
        for (int r = 0; r < 4; ++r) {
          float *row = sT + (sw + 4 * part + r) * ldT;
          if (j0 < J) row[j0] = sl ? row[j0] + acc0[r] : acc0[r];
          if (j1 < J) row[j1] = sl ? row[j1] + acc1[r] : acc1[r];
        }
      }
    }
    __syncthreads();
    // Q of the next site to the left for this wave's 16 samples: lane = (sample r16, quarter `part` of the bond index a)
    // (a wave reads and writes only its own samples of Q, and its products with Q are behind it)
    const int s = sw + r16;
    const float *Ts = sT + (size_t)s * ldT;
    for (int a = part; a < ml; a += 4) {
      float v = 0.f;
      for (int d = 0; d < D; ++d) v = fmaf(sX[s * D + d], Ts[a * D + d], v);
      sQ[a * kCgLd + s] = v;
    }
  }
  __syncthreads();
  if (p.cf && tid < kCgTS && s0 + tid < p.b) p.cf[s0 + tid] = sQ[tid];
}

static bool core_grad_geometry_ok(const CoreGradParams &p) {
  return p.b >= 1 && p.b <= p.b_pad && p.b_pad % kCgTS == 0 && p.x_bpad >= p.b_pad && p.mb >= 1 && p.mb <= p.cap && p.D >= 2 && p.D <= kMaxD &&
         p.N >= 2 && p.L >= 1 && p.l_pos >= 0 && p.l_pos < p.N;
}

bool launch_core_grad_chain(const CoreGradParams &p, hipStream_t st) {
  if (!core_grad_geometry_ok(p)) return false;
  const size_t lds = core_grad_chain_lds_bytes(p.mb, p.D, p.L, p.N);
  if (lds > 160 * 1024) return false;
  hipLaunchKernelGGL(core_grad_chain_kernel, dim3((p.b + kCgTS - 1) / kCgTS), dim3(256), lds, st, p);
  return true;
}

// ------------------------------------------------------------------------------------------
// reduction kernel: G_i (+)= (P_i (x) x_i [cot])^T . Q_i^T over the samples of the chunk
// ------------------------------------------------------------------------------------------
size_t core_grad_reduce_lds_bytes(int mb, int D) { return (2 * (size_t)mb * kCgLdR + (size_t)kCgTS * D) * sizeof(float); }

int core_grad_reduce_blocks(int mb, int D) {
  const int pairs = ((mb * D + 15) / 16) * (((mb + 15) / 16 + 1) / 2);
  return (pairs + 3) / 4;
}

__global__ __launch_bounds__(256) void core_grad_reduce_kernel(CoreGradParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int i = blockIdx.x, sl = blockIdx.z, D = p.D, N = p.N;
  const bool label = i == p.l_pos;
  if (sl > 0 && !label) return;                              // only the label site has more than one slice
  const int ml = i == 0 ? 1 : p.tab[i - 1], mr = i == N - 1 ? 1 : p.tab[i];
  const int J = ml * D, CP = ((mr + 15) / 16 + 1) / 2, npairs = ((J + 15) / 16) * CP;
  if ((int)blockIdx.y * 4 >= npairs) return;                 // (the grid is sized for the largest bond)
  float *sP = (float *)smem_raw;                             // [ml][kCgLdR]
  float *sQ = sP + (size_t)p.mb * kCgLdR;                    // [mr][kCgLdR]
  float *sX = sQ + (size_t)p.mb * kCgLdR;                    // [64][D]: x, at the label site x cot[sl]
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r16 = lane & 15, part = lane >> 4;
  const int q = blockIdx.y * 4 + wave;                       // this wave's pair of tiles: row tile q / CP, column tiles 2 (q % CP) + {0, 1}
  const bool active = q < npairs;
  const int row0 = (q / CP) * 16, c0 = (q % CP) * 32 + r16, c1 = c0 + 16;
  const int j = row0 + r16, ja = j / D, jd = j - ja * D;     // the row of the A operand this lane supplies: (a, d)
  const int nL = label ? p.L : 1;
  float *Gi = p.G + (size_t)p.tab[N + i] + sl;
  cg_f4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};   // acc[r]: row row0 + 4 part + r, column c0 / c1
  if (active && !p.first) {
    for (int r = 0; r < 4; ++r) {
      const int row = row0 + 4 * part + r;
      if (row < J && c0 < mr) acc0[r] = Gi[((size_t)row * mr + c0) * nL];
      if (row < J && c1 < mr) acc1[r] = Gi[((size_t)row * mr + c1) * nL];
    }
  }
  const float *srcP = p.stackP + (size_t)i * p.cap * p.b_pad, *srcQ = p.stackQ + (size_t)i * p.cap * p.b_pad;
  const float *srcX = p.X + (size_t)i * p.x_bpad * D, *cot = p.cot + (size_t)sl * p.b_pad;
  for (int s0 = 0; s0 < p.b; s0 += kCgTS) {
    __syncthreads();                                         // the tiles of the previous 64 samples are free
    if (i == 0) { if (tid < kCgTS) sP[tid] = 1.f; }
    else for (int e = tid; e < ml * kCgTS; e += 256) sP[(e / kCgTS) * kCgLdR + e % kCgTS] = srcP[(size_t)(e / kCgTS) * p.b_pad + s0 + e % kCgTS];
    if (i == N - 1) { if (tid < kCgTS) sQ[tid] = 1.f; }
    else for (int e = tid; e < mr * kCgTS; e += 256) sQ[(e / kCgTS) * kCgLdR + e % kCgTS] = srcQ[(size_t)(e / kCgTS) * p.b_pad + s0 + e % kCgTS];
    for (int e = tid; e < kCgTS * D; e += 256) {
      const float xv = srcX[(size_t)s0 * D + e];
      sX[e] = label ? xv * cot[s0 + e / D] : xv;
    }
    __syncthreads();
    if (!active) continue;
    for (int k = part; k < kCgTS; k += 4) {
      const float av = j < J ? sP[ja * kCgLdR + k] * sX[k * D + jd] : 0.f;
      const float b0 = c0 < mr ? sQ[c0 * kCgLdR + k] : 0.f, b1 = c1 < mr ? sQ[c1 * kCgLdR + k] : 0.f;
      acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b0, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b1, acc1, 0, 0, 0);
    }
  }
  if (!active) return;
  for (int r = 0; r < 4; ++r) {
    const int row = row0 + 4 * part + r;
    if (row < J && c0 < mr) Gi[((size_t)row * mr + c0) * nL] = acc0[r];
    if (row < J && c1 < mr) Gi[((size_t)row * mr + c1) * nL] = acc1[r];
  }
}

bool launch_core_grad_reduce(const CoreGradParams &p, hipStream_t st) {
  if (!core_grad_geometry_ok(p)) return false;
  const size_t lds = core_grad_reduce_lds_bytes(p.mb, p.D);
  if (lds > 160 * 1024) return false;
  hipLaunchKernelGGL(core_grad_reduce_kernel, dim3(p.N, core_grad_reduce_blocks(p.mb, p.D), p.L), dim3(256), lds, st, p);
  return true;
}

}  // namespace tnml
