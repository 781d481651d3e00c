// Prediction with a power-of-two exponent per sample (tnml_predict_scaled, and every prediction while tnml_set_chain_scaling is
// on).  One kernel, 64 samples per workgroup, 256 threads, the tiles, LDS image and bank argument of
// grad_chain_device.h:
//   left half-chain   i = 0 .. l-1     P_{i+1}[c] = sum_{a,d} P_i[a] x_i[d] A_i[a][d][c]          (the form of pass A)
//   right half-chain  i = N-1 .. l+1   T[a][d] = sum_c A_i[a][d][c] Q_i[c],  Q_{i-1}[a] = sum_d x_i[d] T[a][d]   (pass B)
//   label site        per label l'     T[a][d] = sum_c A_l[a][d][c][l'] Q_l[c],  f[l'] = sum_a P_l[a] sum_d x_l[d] T[a][d]
// After every site the sample's column is rescaled by gc_rescale, so P_l and Q_l are mantissas with the exponents eP and eQ, and
// f[l'][s] 2^(eP + eQ) is the network's output.  The last step normalises over the labels: 0.5 <= max_l' |mant[l'][s]| < 1.
// No environment is stored: the only traffic besides the cores and x is mant, expo and f.
//
// LDS: that of the two-pass body in its scaled form (grad_chain_lds_bytes(.., true)), used as: core image; two environment tiles
// (the left chain alternates between them, the right chain then keeps Q in the one that does not hold P_l); x; f [L][64] in the
// place of cot; T; the bond table; the two exponent rows.
#include "tnml_internal.h"
#include "grad_chain_device.h"

namespace tnml {

__global__ __launch_bounds__(256) void scaled_pred_kernel(ScaledPredParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int D = p.D, L = p.L, N = p.N, mb = p.mb, lp = p.l_pos;
  const int ldA = mb | 1, ldT = (mb * D) | 1;
  float *sA = (float *)smem_raw;                           // [ml D][ldA]  core of the site (one label slice of the label core)
  float *sE0 = sA + (size_t)mb * D * ldA;                  // [mb][kGcLd]
  float *sE1 = sE0 + (size_t)mb * kGcLd;                   // [mb][kGcLd]
  float *sX = sE1 + (size_t)mb * kGcLd;                    // [64][D]
  float *sF = sX + (size_t)kGcTS * D;                      // [L][64]
  float *sT = sF + (size_t)L * kGcTS;                      // [64][ldT]
  int *sBond = (int *)(sT + (size_t)kGcTS * ldT);          // [N + 1]: 1, bond[0 .. N-2], 1
  int *sEP = sBond + (N + 1), *sEQ = sEP + kGcTS;          // [64] exponents of P and of Q
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r16 = lane & 15, part = lane >> 4;
  const int s0 = blockIdx.x * kGcTS, sw = wave * 16;       // sw: this wave's samples
  if (tid < 2 * kGcTS) sEP[tid] = 0;
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
    for (int e = tid; e < kGcTS * D; e += 256) sX[e] = p.X[((size_t)i * p.b_pad + s0) * D + e];
  };
  // T [64][ml D] = Q . A^T over the staged image (the product of pass B)
  auto product_T = [&](int ml, int mr, const float *sQ) {
    const int J = ml * D;
    const float *qs = sQ + sw + r16;
    for (int jt = 0; jt < (J + 15) / 16; jt += 2) {
      const int j0 = jt * 16 + r16, j1 = j0 + 16;
      gc_f4 acc0, acc1;
      gc_mfma_pair(
          mr, D, [&](int k, int, int) { return qs[k * kGcLd]; },
          [&](int k) { return j0 < J ? sA[j0 * ldA + k] : 0.f; }, [&](int k) { return j1 < J ? sA[j1 * ldA + k] : 0.f; }, acc0, acc1);
      for (int r = 0; r < 4; ++r) {
        float *row = sT + (sw + 4 * part + r) * ldT;
        if (j0 < J) row[j0] = acc0[r];
        if (j1 < J) row[j1] = acc1[r];
      }
    }
  };
  if (tid < kGcTS) { sE0[tid] = 1.f; sE1[tid] = 1.f; }
  __syncthreads();

  // ---- left half-chain: P_l with its exponents ---------------------------------------------------
  float *ein = sE0, *eout = sE1;
  for (int i = 0; i < lp; ++i) {
    const int ml = sBond[i], mr = sBond[i + 1], K = ml * D;
    __syncthreads();                                         // the core image and x of the previous product are free
    stage(i, 0, ml, mr);
    load_x(i);
    __syncthreads();
    const float *xs = sX + (sw + r16) * D, *es = ein + sw + r16;
    for (int ot = 0; ot < (mr + 15) / 16; ot += 2) {
      const int o0 = ot * 16 + r16, o1 = o0 + 16;
      gc_f4 acc0, acc1;
      gc_mfma_pair(
          K, D, [&](int, int a, int d) { return es[a * kGcLd] * xs[d]; },
          [&](int k) { return o0 < mr ? sA[k * ldA + o0] : 0.f; }, [&](int k) { return o1 < mr ? sA[k * ldA + o1] : 0.f; }, acc0, acc1);
      for (int r = 0; r < 4; ++r) {
        const int col = sw + 4 * part + r;
        if (o0 < mr) eout[o0 * kGcLd + col] = acc0[r];
        if (o1 < mr) eout[o1 * kGcLd + col] = acc1[r];
      }
    }
    __syncthreads();
    gc_rescale(eout, mr, sw + r16, part, sEP);
    float *t = ein; ein = eout; eout = t;
  }
  float *sP = ein, *sQ = eout;                               // P_l; the other tile is free for Q

  // ---- right half-chain: Q_l with its exponents, in place ----------------------------------------
  __syncthreads();
  if (tid < kGcTS) sQ[tid] = 1.f;
  for (int i = N - 1; i > lp; --i) {
    const int ml = sBond[i], mr = sBond[i + 1];
    __syncthreads();                                         // Q of this site is complete; core image, x and T are free
    stage(i, 0, ml, mr);
    load_x(i);
    __syncthreads();
    product_T(ml, mr, sQ);
    __syncthreads();
    // (a wave reads and writes only its own samples of Q, and its products with Q are behind it)
    const int s = sw + r16;
    const float *Ts = sT + (size_t)s * ldT;
    for (int a = part; a < ml; a += 4) {
      float v = 0.f;
      for (int d = 0; d < D; ++d) v = fmaf(sX[s * D + d], Ts[a * D + d], v);
      sQ[a * kGcLd + s] = v;
    }
    gc_rescale(sQ, ml, s, part, sEQ);
  }

  // ---- label site, one label slice at a time -----------------------------------------------------
  {
    const int ml = sBond[lp], mr = sBond[lp + 1], s = sw + r16;
    const float *Ts = sT + (size_t)s * ldT;
    for (int sl = 0; sl < L; ++sl) {
      __syncthreads();                                       // Q_l is complete; the core image and T of the previous slice are free
      stage(lp, sl, ml, mr);
      if (sl == 0) load_x(lp);
      __syncthreads();
      product_T(ml, mr, sQ);
      __syncthreads();
      float v = 0.f;
      for (int a = part; a < ml; a += 4) {
        float u = 0.f;
        for (int d = 0; d < D; ++d) u = fmaf(sX[s * D + d], Ts[a * D + d], u);
        v = fmaf(sP[a * kGcLd + s], u, v);
      }
      v += __shfl_xor(v, 16);
      v += __shfl_xor(v, 32);
      if (part == 0) sF[sl * kGcTS + s] = v;
    }
  }
  __syncthreads();

  // ---- normalisation over the labels and the three stores ----------------------------------------
  if (tid < kGcTS) {
    const int s = tid, ex = sEP[s] + sEQ[s];
    float mx = 0.f;
    bool bad = false;
    for (int l = 0; l < L; ++l) {
      const float av = fabsf(sF[l * kGcTS + s]);
      bad |= !(av < INFINITY);
      mx = fmaxf(mx, av);
    }
    int k = 0;
    const bool norm = !bad && mx > 0.f;
    if (norm) (void)frexpf(mx, &k);
    const int eo = norm ? ex + k : 0;
    p.expo[s0 + s] = eo;
    for (int l = 0; l < L; ++l) {
      const float m = ldexpf(sF[l * kGcTS + s], norm ? -k : ex);
      p.mant[(size_t)l * p.b_pad + s0 + s] = m;
      p.f[(size_t)l * p.b_pad + s0 + s] = ldexpf(m, eo);
    }
  }
}

size_t scaled_pred_lds_bytes(int mb, int D, int L, int N) { return grad_chain_lds_bytes(mb, D, L, N, true); }

bool launch_scaled_pred(const ScaledPredParams &p, hipStream_t st) {
  if (p.b < 1 || p.b > p.b_pad || p.b_pad % kGcTS || p.mb < 1 || p.D < 2 || p.D > kMaxD || p.N < 2 || p.L < 1 || p.l_pos < 0 || p.l_pos >= p.N)
    return false;
  const size_t lds = scaled_pred_lds_bytes(p.mb, p.D, p.L, p.N);
  if (lds > 160 * 1024) return false;
  hipLaunchKernelGGL(scaled_pred_kernel, dim3((p.b + kGcTS - 1) / kGcTS), dim3(256), lds, st, p);
  return true;
}

}  // namespace tnml
