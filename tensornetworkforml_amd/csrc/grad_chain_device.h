// The two-pass chain of the gradient calls: the one device body of input_grad_kernel (kernels_inputgrad.hip) and
// core_grad_chain_kernel (kernels_coregrad.hip), DESIGN.md sections 15, 16 and 19.
// With P_i[a] the contraction of sites 0 .. i-1 and Q_i[c] that of sites i+1 .. N-1 of a sample (the open label axis contracted
// with cot[:, s] at the label site l, P_0 = Q_{N-1} = 1):
//   pass A, i = 0 .. N-2:   P_{i+1}[c] = sum_{a,d} P_i[a] x_i[d] A_i[a][d][c]                 (at i = l: ... cot[l'] A_l[a][d][c][l'])
//   pass B, i = N-1 .. 0:   T[a][d]    = sum_c A_i[a][d][c] Q_i[c]                            (at i = l: ... A_l[a][d][c][l'] cot[l'])
//                           Q_{i-1}[a] = sum_d x_i[d] T[a][d]
//   after i = 0:            cf = Q_{-1} = sum_l' cot[l'] f[l']
// A workgroup of four waves owns 64 samples, each wave 16 of them as the rows of its v_mfma_f32_16x16x4_f32 tiles (the form of
// anyd_chain_kernel); samples never meet, so there is no communication between workgroups.  The site's core is staged in LDS as
// the plain matrix [(a, d)][c]: pass A reads it as the B operand of (P (x) x) . A, pass B reads the same image transposed as the B
// operand of Q . A^T.  Pass A stores P_1 .. P_{N-1} to an HBM stack [N][cap][b_pad] (the library's [m][b_pad] environment
// layout); pass B keeps Q in LDS.  The label core is taken one label slice at a time (at bond 50 and ten labels it is 200 KB), the
// slices accumulate in the LDS tile that receives the product.  What a kernel does with P, Q and T of a site is its two hooks.
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
#pragma once
#include "tnml_internal.h"

namespace tnml {

typedef float gc_f4 __attribute__((ext_vector_type(4)));

constexpr int kGcTS = 64;          // samples per workgroup
constexpr int kGcLd = 81;          // row stride of the environment tiles in LDS

// What the body reads: the fields InputGradParams and CoreGradParams share, filled by either kernel from its own block.
struct GradChainView {
  const int *bond;         // [N-1] bond dimensions of the chain
  const float *cores, *labcore, *X, *cot;
  float *stack;            // [N][cap][b_pad]: slot i receives P_i, i = 1 .. N-1
  float *cf;               // [b] or nullptr
  size_t core_stride;
  int b, b_pad, x_bpad, N, D, L, l_pos, cap, mb;
};

// scaled: the two exponent rows of the range-safe form (below) behind the bond table
inline size_t grad_chain_lds_bytes(int mb, int D, int L, int N, bool scaled = false) {
  const size_t ldA = (size_t)mb | 1, ldT = ((size_t)mb * D) | 1;
  return ((size_t)mb * D * ldA + 2 * (size_t)mb * kGcLd + (size_t)kGcTS * D + (size_t)L * kGcTS + (size_t)kGcTS * ldT) * sizeof(float) +
         (size_t)(N + 1) * sizeof(int) + (scaled ? 2 * (size_t)kGcTS * sizeof(int) : 0);
}

// Two 16 x 16 output tiles that share their A operand, K in steps of 4 (operand and accumulator layout: anyd_mfma_tile of
// kernels_anyd.hip): A[i][k] = fa(k) of row i = lane & 15, B[k][j] = fb0(k) / fb1(k) of column j = lane & 15; fa receives k as
// (k / D, k % D), kept by increments.  acc[r] holds row 4 * (lane >> 4) + r, column lane & 15 (v_mfma_f32_16x16x4_f32).
template <class FA, class FB0, class FB1>
__device__ inline void gc_mfma_pair(int K, int D, FA fa, FB0 fb0, FB1 fb1, gc_f4 &acc0, gc_f4 &acc1) {
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

// The range-safe form: the column of sample s (the thread's, of the workgroup's 64; lane = (sample, quarter
// `part` of the bond index)) of the tile E [m][kGcLd] is multiplied by exactly 2^-k, k = ilogb(max_a |E[a][s]|) + 1, and k is added
// to the sample's exponent ex[s]; k = 0 where that maximum is 0 or not finite.  frexpf gives the same k (mx = v 2^k, 0.5 <= v < 1),
// ldexpf is exact short of the subnormal range.  The four lanes of a sample are lanes r16, r16 + 16, r16 + 32, r16 + 48 of one wave.
__device__ inline void gc_rescale(float *E, int m, int s, int part, int *ex) {
  float mx = 0.f;
  bool bad = false;
  for (int a = part; a < m; a += 4) {
    const float av = fabsf(E[a * kGcLd + s]);
    bad |= !(av < INFINITY);
    mx = fmaxf(mx, av);
  }
  if (bad) mx = INFINITY;
  mx = fmaxf(mx, __shfl_xor(mx, 16));
  mx = fmaxf(mx, __shfl_xor(mx, 32));
  int k = 0;
  if (mx > 0.f && mx < INFINITY) (void)frexpf(mx, &k);
  if (k != 0) for (int a = part; a < m; a += 4) E[a * kGcLd + s] = ldexpf(E[a * kGcLd + s], -k);
  if (part == 0) ex[s] += k;
}

// Both passes for the 64 samples of workgroup blockIdx.x, 256 threads.  The two places where the kernels differ:
//   site_hook(i, ml, mr, sP, sQ, s0)   all 256 threads, pass B at the first label slice of site i, between the barrier that ends the
//                                      products of site i + 1 and the one before those of site i: sQ [mr][kGcLd] holds Q_i, sP
//                                      [mb][kGcLd] is free (P_i is not kept from pass A)
//   t_hook(i, ml, s, Ts, sP, s0)       once T of site i is complete, before Q of site i - 1 replaces Q_i: the thread's sample s
//                                      (of the workgroup's 64; lane = (sample, quarter of the bond index a)), its row Ts of T [ml D]
// SCALED: every P_{i+1} and every Q_{i-1} is rescaled per sample (gc_rescale) as soon as it is complete.  Pass A writes the cumulative
// exponent eP_{i+1}[s] to estack [N][b_pad] beside the stack; pass B keeps eQ[s] in LDS.  Both hooks receive sEQ (the exponents of
// the Q they see) as one more argument, and cf = ldexpf(Q_{-1}, eQ).  No expression of the unscaled form changes.
template <bool SCALED = false, class SiteHook, class THook>
__device__ inline void grad_chain_body(const GradChainView &p, SiteHook site_hook, THook t_hook, int *estack = nullptr) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int D = p.D, L = p.L, N = p.N, mb = p.mb, lp = p.l_pos;
  const int ldA = mb | 1, ldT = (mb * D) | 1;
  float *sA = (float *)smem_raw;                           // [ml D][ldA]  core of the site (one label slice of the label core)
  float *sE0 = sA + (size_t)mb * D * ldA;                  // [mb][kGcLd]
  float *sE1 = sE0 + (size_t)mb * kGcLd;                   // [mb][kGcLd]
  float *sX = sE1 + (size_t)mb * kGcLd;                    // [64][D]
  float *sCot = sX + (size_t)kGcTS * D;                    // [L][64]
  float *sT = sCot + (size_t)L * kGcTS;                    // [64][ldT]
  int *sBond = (int *)(sT + (size_t)kGcTS * ldT);          // [N + 1]: 1, bond[0 .. N-2], 1 (a site's two bonds without a trip to memory)
  int *sEP = sBond + (N + 1), *sEQ = sEP + kGcTS;          // SCALED: [64] exponents of P (pass A) and of Q (pass B)
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r16 = lane & 15, part = lane >> 4;
  const int s0 = blockIdx.x * kGcTS, sw = wave * 16;       // sw: this wave's samples
  if constexpr (SCALED) { if (tid < 2 * kGcTS) sEP[tid] = 0; }
  for (int e = tid; e <= N; e += 256) sBond[e] = (e == 0 || e == N) ? 1 : p.bond[e - 1];
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
    for (int e = tid; e < kGcTS * D; e += 256) sX[e] = p.X[((size_t)i * p.x_bpad + s0) * D + e];
  };
  for (int e = tid; e < L * kGcTS; e += 256) sCot[e] = p.cot[(size_t)(e / kGcTS) * p.b_pad + s0 + e % kGcTS];
  if (tid < kGcTS) sE0[tid] = 1.f;
  __syncthreads();

  // ---- pass A: P_1 .. P_{N-1} to the stack ------------------------------------------------------
  float *ein = sE0, *eout = sE1;
  for (int i = 0; i < N - 1; ++i) {
    const int ml = sBond[i], mr = sBond[i + 1], K = ml * D, nsl = i == lp ? L : 1;
    for (int sl = 0; sl < nsl; ++sl) {
      __syncthreads();                                       // the core image and x of the previous product are free
      stage(i, sl, ml, mr);
      if (sl == 0) load_x(i);
      __syncthreads();
      const float crv = i == lp ? sCot[sl * kGcTS + sw + r16] : 1.f, *xs = sX + (sw + r16) * D, *es = ein + sw + r16;
      for (int ot = 0; ot < (mr + 15) / 16; ot += 2) {
        const int o0 = ot * 16 + r16, o1 = o0 + 16;
        gc_f4 acc0, acc1;
        gc_mfma_pair(
            K, D, [&](int, int a, int d) { return es[a * kGcLd] * xs[d] * crv; },
            [&](int k) { return o0 < mr ? sA[k * ldA + o0] : 0.f; }, [&](int k) { return o1 < mr ? sA[k * ldA + o1] : 0.f; }, acc0, acc1);
        for (int r = 0; r < 4; ++r) {
          const int col = sw + 4 * part + r;
          if (o0 < mr) eout[o0 * kGcLd + col] = sl ? eout[o0 * kGcLd + col] + acc0[r] : acc0[r];
          if (o1 < mr) eout[o1 * kGcLd + col] = sl ? eout[o1 * kGcLd + col] + acc1[r] : acc1[r];
        }
      }
    }
    __syncthreads();
    if constexpr (SCALED) {
      gc_rescale(eout, mr, sw + r16, part, sEP);
      __syncthreads();
      if (tid < kGcTS) estack[(size_t)(i + 1) * p.b_pad + s0 + tid] = sEP[tid];
    }
    float *dst = p.stack + (size_t)(i + 1) * p.cap * p.b_pad + s0;
    for (int e = tid; e < mr * kGcTS; e += 256) dst[(size_t)(e / kGcTS) * p.b_pad + e % kGcTS] = eout[(e / kGcTS) * kGcLd + e % kGcTS];
    float *t = ein; ein = eout; eout = t;
  }

  // ---- pass B: T = Q . A^T, the hooks, Q of the next site to the left ---------------------------
  __syncthreads();
  float *sP = sE0, *sQ = sE1;
  if (tid < kGcTS) sQ[tid] = 1.f;
  for (int i = N - 1; i >= 0; --i) {
    const int ml = sBond[i], mr = sBond[i + 1], J = ml * D, nsl = i == lp ? L : 1;
    for (int sl = 0; sl < nsl; ++sl) {
      __syncthreads();                                       // Q of this site is complete; core image, x, P and T are free
      stage(i, sl, ml, mr);
      if (sl == 0) {
        load_x(i);
        if constexpr (SCALED) site_hook(i, ml, mr, sP, sQ, s0, sEQ);
        else site_hook(i, ml, mr, sP, sQ, s0);
      }
      __syncthreads();
      const float crv = i == lp ? sCot[sl * kGcTS + sw + r16] : 1.f, *qs = sQ + sw + r16;
      for (int jt = 0; jt < (J + 15) / 16; jt += 2) {
        const int j0 = jt * 16 + r16, j1 = j0 + 16;
        gc_f4 acc0, acc1;
        gc_mfma_pair(
            mr, D, [&](int k, int, int) { return qs[k * kGcLd] * crv; },
            [&](int k) { return j0 < J ? sA[j0 * ldA + k] : 0.f; }, [&](int k) { return j1 < J ? sA[j1 * ldA + k] : 0.f; }, acc0, acc1);
        for (int r = 0; r < 4; ++r) {
          float *row = sT + (sw + 4 * part + r) * ldT;
          if (j0 < J) row[j0] = sl ? row[j0] + acc0[r] : acc0[r];
          if (j1 < J) row[j1] = sl ? row[j1] + acc1[r] : acc1[r];
        }
      }
    }
    __syncthreads();
    // the small contractions of this wave's 16 samples: lane = (sample r16, quarter `part` of the bond index a)
    const int s = sw + r16;
    const float *Ts = sT + (size_t)s * ldT;
    if constexpr (SCALED) t_hook(i, ml, s, Ts, sP, s0, sEQ);
    else t_hook(i, ml, s, Ts, sP, s0);
    // (a wave reads and writes only its own samples of Q, and its products with Q are behind it)
    for (int a = part; a < ml; a += 4) {
      float v = 0.f;
      for (int d = 0; d < D; ++d) v = fmaf(sX[s * D + d], Ts[a * D + d], v);
      sQ[a * kGcLd + s] = v;
    }
    if constexpr (SCALED) gc_rescale(sQ, ml, s, part, sEQ);
  }
  __syncthreads();
  if constexpr (SCALED) {
    if (p.cf && tid < kGcTS && s0 + tid < p.b) p.cf[s0 + tid] = ldexpf(sQ[tid], sEQ[tid]);
  } else {
    if (p.cf && tid < kGcTS && s0 + tid < p.b) p.cf[s0 + tid] = sQ[tid];
  }
}

}  // namespace tnml
