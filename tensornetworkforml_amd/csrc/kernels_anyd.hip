// Generic feature dimension (3 <= D <= 8): every kernel of the per-step sweep, the forward chain and the input re-tiling with D
// as a run-time value.  The D == 2 kernels (kernels_wide.hip, kernels_narrow.hip, kernels_big.hip) stay the specialisations they
// are; tnml_api.hip sends a context with D != 2 here ("Generic feature dimension").
//
// Every operand at general D is a row-wise Kronecker product of a per-sample environment with that sample's D-vector; the
// kernels form those operands on the fly from LDS, so D only appears in how an operand index splits into (bond, feature).
// Layouts are the library's: x [site][b_pad][D], environments [m][b_pad], f [L][b_pad], merged tensors in the sweep-relative
// frame (h, dk, dk1, g, l).
#include "tnml_internal.h"
#include "jacobi_device.h"
#include "act_device.h"

namespace tnml {

typedef float anyd_f4 __attribute__((ext_vector_type(4)));

// one 16 x 16 output tile, K in steps of 4: A[i][k] = fa(i, k) (row i = lane & 15), B[k][j] = fb(k, j) (column j = lane & 15)
// acc[r] holds row 4 * (lane >> 4) + r, column lane & 15 (v_mfma_f32_16x16x4_f32)
template <class FA, class FB>
__device__ inline anyd_f4 anyd_mfma_tile(int K, FA fa, FB fb) {
  const int lane = threadIdx.x & 63, r = lane & 15, kq = lane >> 4;
  anyd_f4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < K; k0 += 4) {
    const int k = k0 + kq;
    const float a = k < K ? fa(r, k) : 0.f;
    const float b = k < K ? fb(k, r) : 0.f;
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0);
  }
  return acc;
}

// ------------------------------------------------------------------------------------------
// X [b][N][D] -> x [N][b_pad][D]; samples b .. b_pad-1 are zero
// ------------------------------------------------------------------------------------------
__global__ void anyd_transpose_input_kernel(const float *__restrict__ in, float *__restrict__ out, int b, int b_pad, int N, int D) {
  const int n = blockIdx.y;
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < b_pad * D; e += gridDim.x * blockDim.x) {
    const int s = e / D, d = e - s * D;
    out[((size_t)n * b_pad + s) * D + d] = s < b ? in[((size_t)s * N + n) * D + d] : 0.f;
  }
}

void launch_transpose_input_anyd(const float *X_bnd, float *X_nbd, int b, int b_pad, int N, int D, hipStream_t st) {
  const dim3 grid((b_pad * D + 255) / 256, N);
  hipLaunchKernelGGL(anyd_transpose_input_kernel, grid, dim3(256), 0, st, X_bnd, X_nbd, b, b_pad, N, D);
}

// ------------------------------------------------------------------------------------------
// Forward environment chain (Network.forward, Network_class.py:227-255) on the matrix cores: a workgroup of four waves holds
// 64 samples, each wave 16 of them as the rows of its MFMA tiles.  Per site, env_out = (env_in (x) x_site) . A_site:
//   A[s][k = in*D + d] = env_in[in][s] * x[s][d],  B[k][o] = core(in, d, o)   (the site's core, staged in LDS)
// LOGMODE (calibration): every environment is renormalised per sample by its max |.|, the log of the factor accumulates, and
// the workgroup writes log max |f| of each 16-sample group; nothing else is stored.
// ------------------------------------------------------------------------------------------
constexpr int kAnydChainTS = 64;

size_t anyd_chain_lds_bytes(int Mmax, int D, int L) {
  const int mo = Mmax > L ? Mmax : L;
  const int mo16 = (mo + 15) & ~15;
  return kAnydChainTS * sizeof(double) + ((size_t)Mmax * D * mo16 + 2 * (size_t)mo16 * kAnydChainTS + (size_t)kAnydChainTS * D) * sizeof(float);
}

template <bool LOGMODE>
__global__ __launch_bounds__(256) void anyd_chain_kernel(const ChainSite *__restrict__ sites, int n_sites, const float *__restrict__ cores,
                                                         const float *__restrict__ labcore, const float *__restrict__ X,
                                                         float *__restrict__ env_base, float *__restrict__ f, int b, int b_pad, int L,
                                                         int Mmax, int D, float *__restrict__ logmax_out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int mo = Mmax > L ? Mmax : L, mo16 = (mo + 15) & ~15;
  double *sScale = (double *)smem_raw;                             // [64] accumulated log scale (LOGMODE)
  float *sA = (float *)(sScale + kAnydChainTS);                    // [n_in * D][mo16]
  float *sE0 = sA + (size_t)Mmax * D * mo16;                        // [mo16][64]
  float *sE1 = sE0 + (size_t)mo16 * kAnydChainTS;                   // [mo16][64]
  float *sX = sE1 + (size_t)mo16 * kAnydChainTS;                    // [64][D]
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int s0 = blockIdx.x * kAnydChainTS;
  if (tid < kAnydChainTS) { sE0[tid] = 1.f; sScale[tid] = 0.0; }
  float *ein = sE0, *eout = sE1;
  for (int i = 0; i < n_sites; ++i) {
    const ChainSite cs = sites[i];
    const float *src = (cs.is_label ? labcore : cores) + cs.core_off;
    const int K = cs.n_in * D, no = cs.n_out;
    for (int e = tid; e < K * no; e += 256) {
      const int o = e % no, k = e / no;
      sA[k * mo16 + o] = src[(k / D) * cs.s_in + (k % D) * cs.s_d + o * cs.s_out];
    }
    for (int e = tid; e < kAnydChainTS * D; e += 256) sX[e] = X[((size_t)cs.x_site * b_pad + s0) * D + e];
    __syncthreads();
    const int sw = wave * 16;                                        // this wave's samples
    for (int ot = 0; ot < (no + 15) / 16; ++ot) {
      const anyd_f4 acc = anyd_mfma_tile(
          K, [&](int r, int k) { return ein[(k / D) * kAnydChainTS + sw + r] * sX[(sw + r) * D + (k % D)]; },
          [&](int k, int c) { const int o = ot * 16 + c; return o < no ? sA[k * mo16 + o] : 0.f; });
      const int o = ot * 16 + (lane & 15);
      if (o < no)
        for (int r = 0; r < 4; ++r) eout[o * kAnydChainTS + sw + 4 * (lane >> 4) + r] = acc[r];
    }
    __syncthreads();
    if (LOGMODE) {
      if (tid < kAnydChainTS) {
        float mx = 0.f;
        for (int o = 0; o < no; ++o) mx = fmaxf(mx, fabsf(eout[o * kAnydChainTS + tid]));
        if (mx > 0.f && isfinite(mx)) {
          const float inv = 1.f / mx;
          for (int o = 0; o < no; ++o) eout[o * kAnydChainTS + tid] *= inv;
          sScale[tid] += log((double)mx);
        }
      }
      __syncthreads();
    } else if (cs.env_out_off >= 0 && env_base) {
      for (int e = tid; e < no * kAnydChainTS; e += 256) {
        const int o = e / kAnydChainTS, s = e % kAnydChainTS;
        env_base[cs.env_out_off + (size_t)o * b_pad + s0 + s] = eout[e];
      }
    } else if (cs.env_out_off < 0) {
      for (int e = tid; e < no * kAnydChainTS; e += 256) {
        const int o = e / kAnydChainTS, s = e % kAnydChainTS;
        f[(size_t)o * b_pad + s0 + s] = eout[e];
      }
    }
    float *t = ein; ein = eout; eout = t;
  }
  if (LOGMODE && tid < kAnydChainTS) {
    // ein holds f (L values per sample, renormalised): log max |f_s| + accumulated scale, then the max over 16 samples
    const int no = L;
    float mx = 0.f;
    for (int o = 0; o < no; ++o) mx = fmaxf(mx, fabsf(ein[o * kAnydChainTS + tid]));
    float v = (s0 + tid < b && mx > 0.f) ? (float)(log((double)mx) + sScale[tid]) : -INFINITY;
    for (int off = 8; off >= 1; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 16));
    if ((tid & 15) == 0) logmax_out[(s0 + tid) / 16] = v;
  }
}

bool launch_env_chain_anyd(const ChainSite *sites_dev, int n_sites, const float *cores, const float *labcore, const float *X,
                           float *env_base, float *f, int b, int b_pad, int L, int Mmax, int D, float *logmax_out, hipStream_t st) {
  const size_t lds = anyd_chain_lds_bytes(Mmax, D, L);
  if (lds > 160 * 1024 || b_pad % kAnydChainTS) return false;
  if (logmax_out)
    hipLaunchKernelGGL(anyd_chain_kernel<true>, dim3(b_pad / kAnydChainTS), dim3(256), lds, st, sites_dev, n_sites, cores, labcore, X,
                       env_base, f, b, b_pad, L, Mmax, D, logmax_out);
  else
    hipLaunchKernelGGL(anyd_chain_kernel<false>, dim3(b_pad / kAnydChainTS), dim3(256), lds, st, sites_dev, n_sites, cores, labcore, X,
                       env_base, f, b, b_pad, L, Mmax, D, logmax_out);
  return true;
}

// ------------------------------------------------------------------------------------------
// Norm-environment chain at general D (one workgroup, float64):  env_out[o][o'] = sum_{in,in',d} A(in,d,o) env_in[in][in'] A(in',d,o')
// T[in][d][o'] lives in HBM scratch (Mmax * D * Mmax doubles), env in LDS.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void anyd_norm_chain_kernel(const NormChainSite *__restrict__ sites, int n_sites,
                                                              const float *__restrict__ cores, double *__restrict__ env_base,
                                                              double *__restrict__ T, int D) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  double *env = (double *)smem_raw;
  const int tid = threadIdx.x;
  if (tid == 0) env[0] = 1.0;
  __syncthreads();
  for (int i = 0; i < n_sites; ++i) {
    const NormChainSite cs = sites[i];
    const int ni = cs.n_in, no = cs.n_out;
    const float *A = cores + cs.core_off;
    auto a_at = [&](int in, int d, int o) { return (double)A[in * cs.s_in + d * cs.s_d + o * cs.s_out]; };
    for (int e = tid; e < ni * D * no; e += 256) {
      const int o = e % no, q = e / no, d = q % D, in = q / D;
      double acc = 0.0;
      for (int j = 0; j < ni; ++j) acc += env[in * ni + j] * a_at(j, d, o);
      T[e] = acc;
    }
    __syncthreads();
    for (int e = tid; e < no * no; e += 256) {
      const int o2 = e % no, o1 = e / no;
      double acc = 0.0;
      for (int q = 0; q < ni * D; ++q) acc += a_at(q / D, q % D, o1) * T[q * no + o2];
      env_base[cs.env_out_off + e] = acc;
    }
    __syncthreads();
    for (int e = tid; e < no * no; e += 256) env[e] = env_base[cs.env_out_off + e];
    __syncthreads();
  }
}

bool launch_norm_chain_anyd(const NormChainSite *sites_dev, int n_sites, const float *cores, double *env_base, double *T_scratch,
                            int Mmax, int D, hipStream_t st) {
  const size_t lds = (size_t)Mmax * Mmax * sizeof(double);
  if (lds > 160 * 1024) return false;
  hipLaunchKernelGGL(anyd_norm_chain_kernel, dim3(1), dim3(256), lds, st, sites_dev, n_sites, cores, env_base, T_scratch, D);
  return true;
}

// ------------------------------------------------------------------------------------------
// Batch side of a step (classic sequence, one workgroup of four waves per 64 samples):
//   1. f of the previous step from its updated merged tensor (do_f):  f[l][s] = sum_{i,j} P[s][i] Bprev[i][j][l] Q[s][j],
//      P[s][(h', d)] = Hprev[h'][s] x_{k-1}[s][d],  Q[s][(d', g')] = x_k[s][d'] Gprev[g'][s]; T = P . Bprev on the matrix cores,
//      column chunk by column chunk through LDS, then the sum over j with Q in a fixed order;
//   2. activation, loss derivative, metrics (act_device.h);
//   3. extension of the behind environment:  Hcur[h][s] = sum_{h', d} Hprev[h'][s] x_{k-1}[s][d] A(h', d, h);
//   4. gradient partial of the 64 samples:  dB[(h, dk)][(dk1, g, l)] = sum_s U[s][(h, dk)] V[s][(dk1, g, l)],
//      U = Hcur (x) x_k, V = x_{k+1} (x) Gcur (x) g_l, on the matrix cores; one slab per workgroup (+ the metric tail).
// ------------------------------------------------------------------------------------------
constexpr int kAnydTS = 64;
constexpr int kAnydCW = 128;        // columns of the f product per LDS chunk

struct AnydBatchLds {
  float *sXm, *sXk, *sXp, *sHp, *sGp, *sGc, *sE, *sF, *sGL, *sT, *sRed;
};
// (offsets in floats, so that the host can size the request without a base pointer)
__host__ __device__ inline size_t anyd_batch_layout(AnydBatchLds *w, unsigned char *base, int D, int hp, int gp, int h, int g, int L) {
  size_t q = 0;
  size_t o[11];
  int k = 0;
  auto take = [&](size_t n) { o[k++] = q; q += (n + 3) & ~(size_t)3; };
  take((size_t)kAnydTS * D); take((size_t)kAnydTS * D); take((size_t)kAnydTS * D);
  take((size_t)hp * kAnydTS); take((size_t)gp * kAnydTS); take((size_t)g * kAnydTS);
  take((size_t)h * kAnydTS); take((size_t)L * kAnydTS); take((size_t)L * kAnydTS);
  take((size_t)kAnydTS * kAnydCW); take(4 * 256);
  if (w) {
    float *f = (float *)base;
    w->sXm = f + o[0]; w->sXk = f + o[1]; w->sXp = f + o[2]; w->sHp = f + o[3]; w->sGp = f + o[4]; w->sGc = f + o[5];
    w->sE = f + o[6]; w->sF = f + o[7]; w->sGL = f + o[8]; w->sT = f + o[9]; w->sRed = f + o[10];
  }
  return q * sizeof(float);
}

size_t anyd_batch_lds_bytes(int D, int hp, int gp, int h, int g, int L) {
  return anyd_batch_layout(nullptr, nullptr, D, hp, gp, h, g, L);
}

__global__ __launch_bounds__(256) void anyd_batch_kernel(WideParams p, int D, int do_grad) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int s0 = blockIdx.x * kAnydTS, b_pad = p.b_pad, L = p.L;
  const int hp = p.hp, gp = p.gp, h = p.h, g = p.g;
  AnydBatchLds w;
  anyd_batch_layout(&w, smem_raw, D, hp, gp, h, g, L);
  const bool need_prev = p.do_f || p.do_ext;
  for (int e = tid; e < kAnydTS * D; e += 256) {
    w.sXm[e] = (need_prev && p.x_km1) ? p.x_km1[(size_t)s0 * D + e] : 0.f;
    w.sXk[e] = p.x_k ? p.x_k[(size_t)s0 * D + e] : 0.f;
    w.sXp[e] = (do_grad && p.x_kp1) ? p.x_kp1[(size_t)s0 * D + e] : 0.f;
  }
  if (need_prev)
    for (int e = tid; e < hp * kAnydTS; e += 256) w.sHp[e] = p.Hprev ? p.Hprev[(size_t)(e / kAnydTS) * b_pad + s0 + e % kAnydTS] : 1.f;
  if (p.do_f)
    for (int e = tid; e < gp * kAnydTS; e += 256) w.sGp[e] = p.Gprev ? p.Gprev[(size_t)(e / kAnydTS) * b_pad + s0 + e % kAnydTS] : 1.f;
  if (do_grad)
    for (int e = tid; e < g * kAnydTS; e += 256) w.sGc[e] = p.Gcur ? p.Gcur[(size_t)(e / kAnydTS) * b_pad + s0 + e % kAnydTS] : 1.f;
  __syncthreads();

  // ---- 1. f of the previous step ----------------------------------------------------------------
  if (p.do_f) {
    const int KP = hp * D, NC = D * gp * L;
    float facc2[4] = {0.f, 0.f, 0.f, 0.f};
    for (int c0 = 0; c0 < NC; c0 += kAnydCW) {
      const int cw = min(kAnydCW, NC - c0);
      const int ntile = (kAnydTS / 16) * ((cw + 15) / 16);
      for (int t = wave; t < ntile; t += 4) {
        const int st = t % (kAnydTS / 16), ct = t / (kAnydTS / 16);
        const anyd_f4 acc = anyd_mfma_tile(
            KP, [&](int r, int k) { const int s = st * 16 + r; return w.sHp[(k / D) * kAnydTS + s] * w.sXm[s * D + (k % D)]; },
            [&](int k, int cc) { const int c = c0 + ct * 16 + cc; return c < NC ? p.Bprev[(size_t)k * NC + c] : 0.f; });
        const int cl = ct * 16 + (lane & 15), c = c0 + cl;
        if (cl < cw) {
          const int j = c / L, dq = j / gp, gq = j % gp;
          for (int r = 0; r < 4; ++r) {
            const int s = st * 16 + 4 * (lane >> 4) + r;
            w.sT[s * kAnydCW + cl] = acc[r] * w.sXk[s * D + dq] * w.sGp[gq * kAnydTS + s];
          }
        }
      }
      __syncthreads();
      for (int q = 0; q < 4; ++q) {
        const int s = tid % kAnydTS, l = tid / kAnydTS + 4 * q;
        if (l < L) {
          float a = facc2[q];
          for (int cl = ((l - c0 % L) + L) % L; cl < cw; cl += L) a += w.sT[s * kAnydCW + cl];
          facc2[q] = a;
        }
      }
      __syncthreads();
    }
    for (int q = 0; q < 4; ++q) {
      const int s = tid % kAnydTS, l = tid / kAnydTS + 4 * q;
      if (l < L) w.sF[l * kAnydTS + s] = facc2[q];
    }
    for (int l = tid / kAnydTS + 16; l < L; l += 4) {   // L > 16: the rest in plain FMAs
      const int s = tid % kAnydTS;
      float a = 0.f;
      for (int i = 0; i < KP; ++i) {
        const float pv = w.sHp[(i / D) * kAnydTS + s] * w.sXm[s * D + (i % D)];
        for (int j = 0; j < D * gp; ++j)
          a = fmaf(pv * p.Bprev[((size_t)i * D * gp + j) * L + l], w.sXk[s * D + j / gp] * w.sGp[(j % gp) * kAnydTS + s], a);
      }
      w.sF[l * kAnydTS + s] = a;
    }
    __syncthreads();
    for (int e = tid; e < L * kAnydTS; e += 256) {
      const int l = e / kAnydTS, s = e % kAnydTS;
      if (s0 + s < p.b) p.f[(size_t)l * b_pad + s0 + s] = w.sF[e];
    }
  } else if (do_grad) {
    for (int e = tid; e < L * kAnydTS; e += 256) {
      const int l = e / kAnydTS, s = e % kAnydTS;
      w.sF[e] = p.f[(size_t)l * b_pad + s0 + s];
    }
  }
  if (!do_grad) return;
  __syncthreads();

  // ---- 2. activation, loss derivative, metrics --------------------------------------------------
  float m_abs = 0.f;
  int m_cor = 0, m_nf = 0, m_cnt = 0;
  if (tid < kAnydTS) {
    const int s = tid;
    if (s0 + s < p.b) {
      float sa = 0.f;
      int cor = 0, nf = 0;
      act_and_lossder(w.sF + s, kAnydTS, w.sT + s, w.sGL + s, kAnydTS, L, p.y[s0 + s], p.act_fn, p.loss_fn, p.T, sa, cor, nf);
      m_abs = sa; m_cor = cor; m_nf = nf; m_cnt = 1;
    } else {
      for (int l = 0; l < L; ++l) w.sGL[l * kAnydTS + s] = 0.f;
    }
  }

  // ---- 3. extension of the behind environment ---------------------------------------------------
  if (p.do_ext) {
    const CoreView A = p.ext_core;
    for (int e = tid; e < h * kAnydTS; e += 256) {
      const int o = e / kAnydTS, s = e % kAnydTS;
      float a = 0.f;
      for (int in = 0; in < hp; ++in) {
        const float ev = w.sHp[in * kAnydTS + s];
        for (int d = 0; d < D; ++d) a = fmaf(ev * w.sXm[s * D + d], A.base[in * A.s_in + d * A.s_d + o * A.s_out], a);
      }
      w.sE[e] = a;
      p.Hcur[(size_t)o * b_pad + s0 + s] = a;
    }
  } else {
    for (int e = tid; e < h * kAnydTS; e += 256) {
      const int o = e / kAnydTS, s = e % kAnydTS;
      w.sE[e] = p.Hcur ? p.Hcur[(size_t)o * b_pad + s0 + s] : 1.f;
    }
  }
  // metric tail: one value per wave, then wave 0 sums
  float *red = w.sRed;
  if (tid < kAnydTS) {
    float v0 = (float)m_cor, v1 = m_abs, v2 = (float)m_nf, v3 = (float)m_cnt;
    for (int off = 32; off >= 1; off >>= 1) {
      v0 += __shfl_xor(v0, off); v1 += __shfl_xor(v1, off); v2 += __shfl_xor(v2, off); v3 += __shfl_xor(v3, off);
    }
    if (tid == 0) { red[0] = v0; red[1] = v1; red[2] = v2; red[3] = v3; }
  }
  __syncthreads();

  // ---- 4. gradient partial ----------------------------------------------------------------------
  const int R = h * D, C = D * g * L, gL = g * L;
  float *slab = p.slabs + (size_t)blockIdx.x * p.slab_stride;
  const int IT = (R + 15) / 16, JT = (C + 15) / 16;
  for (int t = wave; t < IT * JT; t += 4) {
    const int it = t / JT, jt = t % JT;
    const anyd_f4 acc = anyd_mfma_tile(
        kAnydTS,
        [&](int r, int s) { const int i = it * 16 + r; return i < R ? w.sE[(i / D) * kAnydTS + s] * w.sXk[s * D + (i % D)] : 0.f; },
        [&](int s, int cc) {
          const int j = jt * 16 + cc;
          if (j >= C) return 0.f;
          const int dk1 = j / gL, rem = j % gL, gq = rem / L, l = rem % L;
          return w.sXp[s * D + dk1] * w.sGc[gq * kAnydTS + s] * w.sGL[l * kAnydTS + s];
        });
    const int j = jt * 16 + (lane & 15);
    if (j < C)
      for (int r = 0; r < 4; ++r) {
        const int i = it * 16 + 4 * (lane >> 4) + r;
        if (i < R) slab[(size_t)i * C + j] = acc[r];
      }
  }
  if (tid < kMetricSlots) slab[(size_t)R * C + tid] = red[tid];
}

bool launch_batch_anyd(const WideParams &p, int D, int nblk, bool do_grad, hipStream_t st) {
  const size_t lds = anyd_batch_lds_bytes(D, p.hp, p.gp, p.h, p.g, p.L);
  if (lds > 160 * 1024) return false;
  if (do_grad && (size_t)p.h * D * D * p.g * p.L + kMetricSlots > (size_t)p.slab_stride) return false;
  hipLaunchKernelGGL(anyd_batch_kernel, dim3(nblk), dim3(256), lds, st, p, D, do_grad ? 1 : 0);
  return true;
}

// ------------------------------------------------------------------------------------------
// Update side of a step (one workgroup, float64): merged tensor (or the given one), L2 term 2 wd Nh^T.B.Ng, clipping, B += lr dB,
// Gram matrix of the short side of the matricised B_new, two-sided Jacobi eigen-decomposition of it (jacobi_device.h), kept rank
// (fixed / reference from the host, adaptive here), the two new cores with sqrt(S) on both, the next behind norm environment.
// The capture block (B, dB_raw, B_new, L2_grad, sigma, scalars; layout of tnml_get_step_debug) is the workspace.
// The matricised tensor in the relative frame: row i = (h, dk) = h D + dk, column j = (dk1, g, l); an odd short side is padded
// with one zero row / column, whose zero eigenvalue sorts last and is never kept (m <= the true short side).
// ------------------------------------------------------------------------------------------
constexpr int kAnydUT = 512;

size_t anyd_update_lds_bytes(int n_pad, bool w_in_lds) {
  const size_t nn = (size_t)n_pad * n_pad;
  return (nn * (w_in_lds ? 2 : 1) + 3 * (size_t)n_pad + 64) * sizeof(double) + (2 * (size_t)n_pad + 8) * sizeof(int);
}

__global__ __launch_bounds__(kAnydUT) void anyd_update_kernel(NarrowParams p, double *__restrict__ Wg, double *__restrict__ T2, int w_in_lds) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int tid = threadIdx.x, NT = kAnydUT;
  const int D = p.D, h = p.h, g = p.g, s = p.s, L = p.L, Bs = p.bsize;
  const int R = h * D, C = D * g * L;
  const bool short_rows = R <= C;
  const int n = short_rows ? R : C, len = short_rows ? C : R;
  const int n_pad = n + (n & 1), np = n_pad / 2;
  double *ws = p.dbg;
  double *wB = ws, *wDB = ws + Bs, *wBN = ws + 2 * (size_t)Bs, *wG2 = ws + 3 * (size_t)Bs;
  double *sig = ws + 4 * (size_t)Bs, *sc = sig + kDbgSigma;
  double *G = (double *)smem_raw;
  double *W = w_in_lds ? G + (size_t)n_pad * n_pad : Wg;
  double *alpha = G + (size_t)n_pad * n_pad * (w_in_lds ? 2 : 1);
  double *beta = alpha + n_pad, *lam = beta + n_pad, *red = lam + n_pad;
  int *partner = (int *)(red + 64), *ord = partner + n_pad, *flags = ord + n_pad;
  const int DgL = D * g * L, gL = g * L;
  // cycle stamps of the phases (capture on): [0] before the Jacobi loop, [1] in it, [2] after it, [3] 100 MHz ticks of the
  // whole kernel, [4] the Gram matrix alone (part of [0])
  const long long c_start = clock64(), w_start = wall_clock64();
  long long c_gram = 0, c_jac0 = 0, c_jac1 = 0;
  auto stamp_end = [&]() {
    if (p.stamps && tid == 0) {
      p.stamps[0] = (double)(c_jac0 - c_start); p.stamps[1] = (double)(c_jac1 - c_jac0); p.stamps[2] = (double)(clock64() - c_jac1);
      p.stamps[3] = (double)(wall_clock64() - w_start); p.stamps[4] = (double)c_gram;
    }
  };

  // ---- merged tensor ----
  for (int e = tid; e < Bs; e += NT) {
    double v;
    if (p.Bdirect) v = (double)p.Bdirect[e];
    else {
      const int l = e % L, gq = (e / L) % g, dk1 = (e / gL) % D, dk = (e / DgL) % D, hq = e / (D * DgL);
      double a = 0.0;
      for (int q = 0; q < s; ++q)
        a += (double)p.lab.base[hq * p.lab.s_in + dk * p.lab.s_d + q * p.lab.s_out + l] *
             (double)p.pl.base[q * p.pl.s_in + dk1 * p.pl.s_d + gq * p.pl.s_out];
      v = a;
    }
    wB[e] = v;
  }
  __syncthreads();
  // ---- L2 term ----
  double l2 = 0.0;
  if (p.l2_flag) {
    for (int e = tid; e < Bs; e += NT) {                // T = Nh^T . B over h  (into the B_new block)
      const int rest = e % (D * DgL), he = e / (D * DgL);
      double a = 0.0;
      if (p.Nh) for (int q = 0; q < h; ++q) a += p.Nh[q * h + he] * wB[(size_t)q * D * DgL + rest];
      else a = wB[e];
      wBN[e] = a;
    }
    __syncthreads();
    for (int e = tid; e < Bs; e += NT) {                // G = T . Ng over g
      const int l = e % L, f_ = (e / L) % g, pre = e / gL;
      double a = 0.0;
      if (p.Ng) for (int q = 0; q < g; ++q) a += wBN[(size_t)pre * gL + q * L + l] * p.Ng[q * g + f_];
      else a = wBN[e];
      wG2[e] = 2.0 * (double)p.wd * a;
      l2 += wB[e] * a;
    }
  } else {
    for (int e = tid; e < Bs; e += NT) wG2[e] = (double)p.wd * wB[e];
  }
  // ---- raw gradient, the two sums of the clipping rule ----
  double sB = 0.0, sD = 0.0;
  for (int e = tid; e < Bs; e += NT) {
    const double dr = (double)p.red[e];
    wDB[e] = dr;
    sB += fabs(wB[e]);
    sD += fabs(dr - wG2[e]);
  }
  auto block_sum = [&](double v) -> double {
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    double t = 0.0;
    for (int i = 0; i < NT / 64; ++i) t += red[i];
    __syncthreads();
    return t;
  };
  const double sumB = block_sum(sB), sumD = block_sum(sD), l2s = block_sum(l2);
  const double fac = sumD > sumB ? sumB / sumD : 1.0;
  int nonfinite = 0;
  for (int e = tid; e < Bs; e += NT) {
    const double bn = wB[e] + (double)p.lr * ((wDB[e] - wG2[e]) * fac);
    wBN[e] = bn;
    const float bf = (float)bn;
    if (!isfinite(bf)) nonfinite = 1;
    p.Bnew[e] = bf;
  }
  if (nonfinite) atomicOr(p.status, 1);
  if (tid == 0) {
    sc[0] = (double)p.wd * l2s; sc[1] = sumB; sc[2] = sumD;
    if (p.metrics) {
      const double cnt = (double)p.red[Bs + 3];
      const double inv = cnt > 0 ? 1.0 / cnt : 0.0;
      p.metrics[0] = (float)((double)p.red[Bs] * inv);
      p.metrics[1] = (float)((double)p.red[Bs + 1] * inv / (double)L);
      if (p.red[Bs + 2] != 0.f) atomicOr(p.status, 1);
    }
  }
  if (p.stop_after_update) return;
  __syncthreads();

  // ---- Gram matrix of the short side (float64 of the float32 B_new), trace-normalised ----
  const long long c_gram0 = clock64();
  auto M_at = [&](int i, int j) -> double { return (double)p.Bnew[(size_t)i * C + j]; };
  for (int e = tid; e < n_pad * n_pad; e += NT) {
    const int a = e / n_pad, b2 = e % n_pad;
    double acc = 0.0;
    if (a < n && b2 < n && a <= b2) {
      if (short_rows) for (int x = 0; x < len; ++x) acc += M_at(a, x) * M_at(b2, x);
      else for (int x = 0; x < len; ++x) acc += M_at(x, a) * M_at(x, b2);
    }
    if (a <= b2) { G[a * n_pad + b2] = acc; G[b2 * n_pad + a] = acc; }
    W[e] = a == b2 ? 1.0 : 0.0;
  }
  __syncthreads();
  double tr = 0.0;
  for (int i = tid; i < n; i += NT) tr += G[i * n_pad + i];
  tr = block_sum(tr);
  const double inv_tr = tr > 0.0 && isfinite(tr) ? 1.0 / tr : 1.0;
  for (int e = tid; e < n_pad * n_pad; e += NT) G[e] *= inv_tr;
  __syncthreads();
  c_jac0 = clock64();
  c_gram = c_jac0 - c_gram0;

  // ---- two-sided Jacobi, round-robin pairing over n_pad positions ----
  const double abs2 = kJacobiAbs * kJacobiAbs, big2 = p.svd_stop2 > 0 ? p.svd_stop2 : kSvdStop2Default;
  int sweeps = 0, rounds = 0;
  bool converged = !isfinite(tr) ? false : (n_pad < 2);
  // kept2: diagonal entries far below the m-th largest are treated as if they were at kKeptFrac of it (jacobi_device.h), as
  // the D = 2 kernels do -- the discarded cluster only has to be separated from the kept subspace, not resolved
  for (int sw = 0; sw < kJacobiMaxSweeps && !converged && isfinite(tr); ++sw) {
    if (tid == 0) flags[0] = 0;
    if (tid < n_pad) {
      const double di = G[tid * n_pad + tid];
      int rk = 0;
      for (int j = 0; j < n_pad; ++j) { const double dj = G[j * n_pad + j]; rk += (dj > di) || (dj == di && j < tid); }
      if (rk == p.m - 1) red[32] = di;
    }
    __syncthreads();
    const double kept2 = (kKeptFrac * red[32]) * (kKeptFrac * red[32]);
    for (int r = 0; r < n_pad - 1; ++r) {
      if (tid < np) {
        auto idx = [&](int pos) { return pos == 0 ? 0 : 1 + (pos - 1 + r) % (n_pad - 1); };
        const int pp = idx(tid), qq = idx(n_pad - 1 - tid);
        const Rot rt = jacobi_rot(G[pp * n_pad + pp], G[qq * n_pad + qq], G[pp * n_pad + qq], kept2, abs2, big2);
        alpha[pp] = rt.c; beta[pp] = -rt.s; partner[pp] = qq;
        alpha[qq] = rt.c; beta[qq] = rt.s; partner[qq] = pp;
        if (rt.level == 2) flags[0] = 1;
      }
      __syncthreads();
      for (int e = tid; e < np * np; e += NT) {         // 2 x 2 block (pair P, pair Q): R_P^T . G . R_Q, in place
        auto idx = [&](int pos) { return pos == 0 ? 0 : 1 + (pos - 1 + r) % (n_pad - 1); };
        const int P = e / np, Q = e % np;
        const int i0 = idx(P), i1 = idx(n_pad - 1 - P), j0 = idx(Q), j1 = idx(n_pad - 1 - Q);
        const double g00 = G[i0 * n_pad + j0], g01 = G[i0 * n_pad + j1], g10 = G[i1 * n_pad + j0], g11 = G[i1 * n_pad + j1];
        const double ai0 = alpha[i0], bi0 = beta[i0], ai1 = alpha[i1], bi1 = beta[i1];
        const double aj0 = alpha[j0], bj0 = beta[j0], aj1 = alpha[j1], bj1 = beta[j1];
        // column j0 of R: R[j0][j0] = aj0, R[j1][j0] = bj0; column j1: R[j1][j1] = aj1, R[j0][j1] = bj1
        const double t00 = g00 * aj0 + g01 * bj0, t01 = g01 * aj1 + g00 * bj1;    // (G R) rows i0
        const double t10 = g10 * aj0 + g11 * bj0, t11 = g11 * aj1 + g10 * bj1;    // (G R) rows i1
        G[i0 * n_pad + j0] = ai0 * t00 + bi0 * t10;
        G[i0 * n_pad + j1] = ai0 * t01 + bi0 * t11;
        G[i1 * n_pad + j0] = ai1 * t10 + bi1 * t00;
        G[i1 * n_pad + j1] = ai1 * t11 + bi1 * t01;
      }
      for (int e = tid; e < n_pad * np; e += NT) {      // W . R: row k, pair P
        auto idx = [&](int pos) { return pos == 0 ? 0 : 1 + (pos - 1 + r) % (n_pad - 1); };
        const int k = e / np, P = e % np;
        const int i0 = idx(P), i1 = idx(n_pad - 1 - P);
        const double w0 = W[k * n_pad + i0], w1 = W[k * n_pad + i1];
        W[k * n_pad + i0] = alpha[i0] * w0 + beta[i0] * w1;
        W[k * n_pad + i1] = alpha[i1] * w1 + beta[i1] * w0;
      }
      __syncthreads();
      ++rounds;
    }
    ++sweeps;
    converged = flags[0] == 0;
    __syncthreads();
  }
  if (!converged && tid == 0) atomicOr(p.status, isfinite(tr) ? 2 : 1);
  c_jac1 = clock64();

  // ---- eigenvalues, descending order; the padding position n sorts last whatever the sign of a rounding-level eigenvalue ----
  for (int i = tid; i < n_pad; i += NT) lam[i] = G[i * n_pad + i] * tr;
  __syncthreads();
  for (int i = tid; i < n_pad; i += NT) {
    const double li = i < n ? lam[i] : -INFINITY;
    int rk = 0;
    for (int j = 0; j < n_pad; ++j) { const double lj = j < n ? lam[j] : -INFINITY; rk += (lj > li) || (lj == li && j < i); }
    ord[rk] = i;
  }
  __syncthreads();
  for (int i = tid; i < n; i += NT) sig[i] = sqrt(fmax(lam[ord[i]], 0.0));
  if (tid == 0) {
    int me = p.m;
    if (p.trunc_thr > 0.0) {
      double tot = 0.0;
      for (int j = 0; j < n; ++j) tot += sqrt(fmax(lam[ord[j]], 0.0));
      double cum = 0.0;
      int idx = 0;
      for (int j = 0; j < n; ++j) {
        cum += sqrt(fmax(lam[ord[j]], 0.0));
        if (cum / tot > p.trunc_thr) { idx = j; break; }
      }
      me = min(p.m, idx + 1);
      if (p.m_out) *p.m_out = me;
    }
    flags[1] = me;
    sc[3] = (double)sweeps; sc[4] = (double)n;
    if (p.counters) {
      atomicAdd(p.counters + 0, (unsigned long long)sweeps);
      atomicAdd(p.counters + 1, 1ull);
      atomicAdd(p.counters + 2, (unsigned long long)rounds);
    }
  }
  __syncthreads();
  const int m = flags[1];
  const double lam_max = lam[ord[0]];
  for (int r = tid; r < m; r += NT) {
    const double l_ = lam[ord[r]];
    const bool ok = l_ > 1e-300 && l_ > 1e-30 * lam_max;
    const double q4 = ok ? sqrt(sqrt(l_)) : 0.0;
    alpha[r] = q4; beta[r] = ok ? 1.0 / q4 : 0.0;
  }
  __syncthreads();

  // ---- the two new cores: behind [(h, dk)][r] = U sqrt(S), ahead [r][(dk1, g, l)] = sqrt(S) V^T ----
  for (int e = tid; e < R * m; e += NT) {
    const int i = e / m, r = e % m, col = ord[r];
    double v;
    if (short_rows) v = W[i * n_pad + col] * alpha[r];
    else { double a = 0.0; for (int j = 0; j < C; ++j) a += M_at(i, j) * W[j * n_pad + col]; v = a * beta[r]; }
    const int hq = i / D, dk = i % D;
    p.out_behind[hq * p.ob_s_h + dk * p.ob_s_d + r * p.ob_s_m] = (float)v;
    if (T2) T2[e] = (double)(float)v;
  }
  for (int e = tid; e < m * C; e += NT) {
    const int r = e / C, j = e % C, col = ord[r];
    double v;
    if (!short_rows) v = W[j * n_pad + col] * alpha[r];
    else { double a = 0.0; for (int i = 0; i < R; ++i) a += W[i * n_pad + col] * M_at(i, j); v = a * beta[r]; }
    const int dk1 = j / gL, rem = j % gL, gq = rem / L, l = rem % L;
    p.out_ahead[r * p.oa_s_m + dk1 * p.oa_s_d + gq * p.oa_s_g + l] = (float)v;
  }
  if (!p.Nh_new || !T2) { stamp_end(); return; }
  __syncthreads();
  // ---- next behind norm environment: Nh_new[r][r'] = sum_{h, h', dk} A(h, dk, r) Nh[h][h'] A(h', dk, r') ----
  double *U2 = T2 + (size_t)R * m;                      // [(h', dk)][r'] = sum_h Nh[h][h'] A(h, dk, r')
  for (int e = tid; e < R * m; e += NT) {
    const int i = e / m, r = e % m, hq = i / D, dk = i % D;
    double a = 0.0;
    if (p.Nh) for (int q = 0; q < h; ++q) a += p.Nh[q * h + hq] * T2[(size_t)(q * D + dk) * m + r];
    else a = T2[e];
    U2[e] = a;
  }
  __syncthreads();
  for (int e = tid; e < m * m; e += NT) {
    const int r = e / m, r2 = e % m;
    double a = 0.0;
    for (int i = 0; i < R; ++i) a += T2[(size_t)i * m + r] * U2[(size_t)i * m + r2];
    p.Nh_new[e] = a;
  }
  stamp_end();
}

bool launch_update_anyd(const NarrowParams &p, double *W_scratch, double *T2_scratch, hipStream_t st) {
  const int R = p.h * p.D, C = p.D * p.g * p.L, n = R < C ? R : C, n_pad = n + (n & 1);
  if (n < 1 || n > kBigMaxN || p.m < 1 || p.m > n) return false;
  const bool w_lds = anyd_update_lds_bytes(n_pad, true) <= 160 * 1024;
  const size_t lds = anyd_update_lds_bytes(n_pad, w_lds);
  if (lds > 160 * 1024) return false;
  hipLaunchKernelGGL(anyd_update_kernel, dim3(1), dim3(kAnydUT), lds, st, p, W_scratch, T2_scratch, w_lds ? 1 : 0);
  return true;
}

}  // namespace tnml
