// Two-site likelihood sweep: the kernels of one step of tnml_nll_sweep, in the sweep-relative frame.
// No float atomic, every sum in a fixed order, no waiting between workgroups: every hand-over is a launch boundary.
//   nll_sweep_chain_kernel   one workgroup per tile of 64 samples walks a list of plain sites, out[o][s] = sum_{i, d} (in[i][s] x[s][d])
//                            A(i, d, o) in float32, and stores the environments the list asks for: the ahead stack of a call (every
//                            site in front of the first pair) and the behind chain at the start site.
//   nll_sweep_merge_kernel   B[h][dk][dk1][g][l] = sum_s lab(h, dk, s, l) pl(s, dk1, g) in float64 from the float32 cores; stored as
//                            float64 (the update) and rounded to float32 (the batch kernel).
//   nll_sweep_batch_kernel   one workgroup per tile: extends the behind chain by the core the step before left (the expression of the
//                            chain kernel, so that a call that starts here finds the same bits), forms U[(a, d)][s] = H[a][s] x_k[s][d]
//                            and V[(e, c)][s] = x_{k+1}[s][e] G[c][s], f[l][s] = sum U B V, the cotangent (nll_cot_kernel's forms), the
//                            per-sample term and flag, and its partial Gd[(a, d)][(e, c)][l] = sum_s U (cot_l V) on
//                            v_mfma_f32_16x16x4_f32: 16 k-steps of four samples, even and odd steps in two accumulators.
//   nll_sweep_reduce_kernel  Gd[e] = the partials of the tiles added in ascending order.
//   nll_sweep_update_kernel  one workgroup, float64 on v_mfma_f64_16x16x4_f64 (mm_lds): T = Nh . (S (x) S) B . Ng, Z = <B, T>,
//                            log Z = log|Z| + ln2 (eH + eG), Gz = 2 T / Z, B' = B + lr (Gd - Gz), the renormalisation of section 25,
//                            the guard and the record; B' leaves as float32 for the split (B itself behind the guard).
//   nll_sweep_extend_kernel  one workgroup after the split: the behind metric environment through the core the step left, with
//                            lognorm_env_kernel's products, order and power of two (a call that starts at the next site walks to the
//                            same bits); thread 0 adds the kept rank and the discarded weight to the step's record.
#include "small_gemm_device.h"
#include "lognorm_device.h"

#include <algorithm>
#include <cmath>

namespace tnml {

constexpr int kNllsLd = kNllsTile + 1;     // row length of the MFMA operands in LDS
constexpr int kNllsUpdWaves = kNllsUpdThreads / 64;

size_t nll_sweep_chain_lds_bytes(int cap, int D) { return ((size_t)2 * cap * kNllsTile + (size_t)kNllsTile * D) * sizeof(float); }
size_t nll_sweep_batch_lds_bytes(int h, int g, int hp, int D, int L) {
  const size_t rows = (size_t)hp + h + g, ops = (size_t)D * h + (size_t)D * g;
  return (rows * kNllsTile + ops * kNllsLd + (size_t)3 * kNllsTile * D + (size_t)6 * L * kNllsTile) * sizeof(float);
}
size_t nll_sweep_update_lds_bytes() { return (size_t)3 * kNllsUpdThreads * sizeof(double); }
size_t nll_sweep_extend_lds_bytes(int mb, int D) { return lognorm_env_lds_bytes(mb, D); }

// one output of one site for one sample; E: [n_in][kNllsTile] and x: [kNllsTile][D] in LDS.  The chain kernel and the extension of
// the batch kernel both call this and nothing else: the order of its sums is part of their results.
__device__ __forceinline__ float nlls_site_out(const float *E, const float *x, const float *A, int n_in, int D, int s_in, int s_d, int s) {
  float acc = 0.f;
  for (int i = 0; i < n_in; ++i) {
    const float e = E[i * kNllsTile + s];
    for (int d = 0; d < D; ++d) acc = fmaf(e * x[s * D + d], A[(size_t)i * s_in + (size_t)d * s_d], acc);
  }
  return acc;
}

__global__ __launch_bounds__(kNllsThreads) void nll_sweep_chain_kernel(NllSweepChainParams p) {
  extern __shared__ __attribute__((aligned(16))) float nlls_sh[];
  const int tid = threadIdx.x, s = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6), D = p.D;
  const size_t s0 = (size_t)blockIdx.x * kNllsTile;
  float *E0 = nlls_sh, *E1 = E0 + (size_t)p.cap * kNllsTile, *sx = E1 + (size_t)p.cap * kNllsTile;
  if (w == 0) {
    E0[s] = 1.f;
    if (p.init_off >= 0) p.stack[p.init_off + s0 + s] = 1.f;
  }
  int n_last = 1;
  __syncthreads();
  for (int j = 0; j < p.n_sites; ++j) {
    const NllSweepSite q = p.sites[j];
    for (int e = tid; e < kNllsTile * D; e += kNllsThreads) sx[e] = p.X[((size_t)q.x_site * p.x_bpad + s0) * D + e];
    __syncthreads();
    const float *A = p.cores + q.core_off;
    for (int o = w; o < q.n_out; o += kNllsThreads / 64) {
      const float v = nlls_site_out(E0, sx, A + (size_t)o * q.s_out, q.n_in, D, q.s_in, q.s_d, s);
      E1[o * kNllsTile + s] = v;
      if (q.out_off >= 0) p.stack[q.out_off + (size_t)o * p.b_pad + s0 + s] = v;
    }
    __syncthreads();
    float *t = E0; E0 = E1; E1 = t;
    n_last = q.n_out;
  }
  if (p.last_out)
    for (int o = w; o < n_last; o += kNllsThreads / 64) p.last_out[(size_t)o * p.b_pad + s0 + s] = E0[o * kNllsTile + s];
}

__global__ __launch_bounds__(256) void nll_sweep_merge_kernel(NllSweepMergeParams p) {
  const int D = p.D, L = p.L, g = p.g, sb = p.s;
  const int n = p.h * D * D * g * L;
  for (int e = blockIdx.x * 256 + threadIdx.x; e < n; e += gridDim.x * 256) {
    int r = e;
    const int l = r % L; r /= L;
    const int c = r % g; r /= g;
    const int d1 = r % D; r /= D;
    const int d0 = r % D, a = r / D;
    const float *lab = p.lab.base + (size_t)a * p.lab.s_in + (size_t)d0 * p.lab.s_d + l;
    const float *pl = p.pl.base + (size_t)d1 * p.pl.s_d + (size_t)c * p.pl.s_out;
    double v = 0.0;
    for (int k = 0; k < sb; ++k) v = fma((double)lab[(size_t)k * p.lab.s_out], (double)pl[(size_t)k * p.pl.s_in], v);
    p.B64[e] = v;
    p.B32[e] = (float)v;
  }
}

__global__ __launch_bounds__(kNllsThreads) void nll_sweep_batch_kernel(NllSweepBatchParams p) {
  extern __shared__ __attribute__((aligned(16))) float nlls_sh[];
  const int tid = threadIdx.x, s = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int D = p.D, L = p.L, h = p.h, g = p.g, hp = p.do_ext ? p.hp : 0;
  const int R = h * D, Q = D * g;
  const size_t s0 = (size_t)blockIdx.x * kNllsTile;
  float *sHp = nlls_sh, *sH = sHp + (size_t)hp * kNllsTile, *sG = sH + (size_t)h * kNllsTile;
  float *sU = sG + (size_t)g * kNllsTile, *sV = sU + (size_t)R * kNllsLd;
  float *sX = sV + (size_t)Q * kNllsLd;                  // [3][tile][D]: sites k - 1, k, k + 1
  float *sCot = sX + (size_t)3 * kNllsTile * D, *sF = sCot + (size_t)L * kNllsTile;   // [L][tile], [4][L][tile]
  const bool live = (int)(s0 + s) < p.b;                 // (the columns behind the batch hold whatever the buffers held)
  for (int e = tid; e < kNllsTile * D; e += kNllsThreads) {
    const bool in = (int)(s0 + e / D) < p.b;
    sX[e] = p.do_ext && in ? p.x_km1[s0 * D + e] : 0.f;
    sX[kNllsTile * D + e] = in ? p.x_k[s0 * D + e] : 0.f;
    sX[2 * kNllsTile * D + e] = in ? p.x_kp1[s0 * D + e] : 0.f;
  }
  for (int a = w; a < hp; a += 4) sHp[a * kNllsTile + s] = p.Hprev[(size_t)a * p.b_pad + s0 + s];
  if (!p.do_ext)
    for (int a = w; a < h; a += 4) sH[a * kNllsTile + s] = p.Hcur[(size_t)a * p.b_pad + s0 + s];
  for (int c = w; c < g; c += 4) sG[c * kNllsTile + s] = live ? p.G[(size_t)c * p.b_pad + s0 + s] : 0.f;
  __syncthreads();
  if (p.do_ext) {
    // (the features of the columns behind the batch are zero here and whatever X holds in the chain kernel: those columns are
    // never read as samples)
    for (int o = w; o < h; o += 4) {
      const float v = nlls_site_out(sHp, sX, p.ext_core.base + (size_t)o * p.ext_core.s_out, hp, D, p.ext_core.s_in, p.ext_core.s_d, s);
      sH[o * kNllsTile + s] = v;
      p.Hcur[(size_t)o * p.b_pad + s0 + s] = v;
    }
    __syncthreads();
  }
  const float *xk = sX + kNllsTile * D, *xk1 = sX + 2 * kNllsTile * D;
  for (int r = w; r < R; r += 4) sU[r * kNllsLd + s] = live ? sH[(r / D) * kNllsTile + s] * xk[s * D + r % D] : 0.f;
  for (int q = w; q < Q; q += 4) sV[q * kNllsLd + s] = xk1[s * D + q / g] * sG[(q % g) * kNllsTile + s];
  __syncthreads();
  // f[l][s] = sum_r U[r][s] (sum_q B[r][q][l] V[q][s]): the rows dealt to the four waves, their partial sums added in wave order
  for (int l = 0; l < L; ++l) {
    float acc = 0.f;
    for (int r = w; r < R; r += 4) {
      const float *Br = p.B32 + (size_t)r * Q * L + l;
      float t = 0.f;
      for (int q = 0; q < Q; ++q) t = fmaf(Br[(size_t)q * L], sV[q * kNllsLd + s], t);
      acc = fmaf(sU[r * kNllsLd + s], t, acc);
    }
    sF[(w * L + l) * kNllsTile + s] = acc;
  }
  __syncthreads();
  if (w == 0) {
    float *f = sF + (size_t)4 * L * kNllsTile;             // (the fifth block: f itself)
    for (int l = 0; l < L; ++l)
      f[l * kNllsTile + s] = ((sF[l * kNllsTile + s] + sF[(L + l) * kNllsTile + s]) + sF[(2 * L + l) * kNllsTile + s]) + sF[(3 * L + l) * kNllsTile + s];
    if (!live) {
      for (int l = 0; l < L; ++l) sCot[l * kNllsTile + s] = 0.f;
    } else {
      bool bad = false;
      double term;
      if (p.y) {
        const int y = p.y[s0 + s];
        const float fy = f[y * kNllsTile + s];
        const float c = 2.f / ((float)p.batch * fy);
        bad = !(fabsf(c) <= 3.4028234e38f);
        term = log((double)fy * (double)fy);
        for (int l = 0; l < L; ++l) sCot[l * kNllsTile + s] = l == y ? c : 0.f;
      } else {
        double den = 0.0;
        for (int l = 0; l < L; ++l) {
          const double v = (double)f[l * kNllsTile + s];
          den = fma(v, v, den);
        }
        const double k = 2.0 / ((double)p.batch * den);
        for (int l = 0; l < L; ++l) {
          const float c = (float)(k * (double)f[l * kNllsTile + s]);
          bad = bad || !(fabsf(c) <= 3.4028234e38f);
          sCot[l * kNllsTile + s] = c;
        }
        term = log(den);
      }
      bad = bad || !(fabs(term) <= kLnzDblMax);
      // (a bad sample adds nothing to Gd: the step is not applied, and a NaN would hide the gradient of the others in the capture)
      if (bad) for (int l = 0; l < L; ++l) sCot[l * kNllsTile + s] = 0.f;
      p.terms[s0 + s] = term;
      p.bad[s0 + s] = bad ? 1 : 0;
    }
  }
  __syncthreads();
  // partial Gd[r][q][l] = sum_s U[r][s] (cot[l][s] V[q][s]): 16 x 16 tiles of (r, q) per label, dealt round-robin to the waves
  const int tr = (R + 15) >> 4, tq = (Q + 15) >> 4, ntiles = tr * tq * L;
  const int r15 = lane & 15, k4 = lane >> 4;
  float *slab = p.slabs + (size_t)blockIdx.x * ((size_t)R * Q * L);
  for (int t = w; t < ntiles; t += 4) {
    const int l = t % L, tt = t / L, ti = tt / tq, tj = tt - ti * tq;
    const int ra = ti * 16 + r15, qb = tj * 16 + r15;
    const float *ua = sU + (size_t)min(ra, R - 1) * kNllsLd, *vb = sV + (size_t)min(qb, Q - 1) * kNllsLd, *cl = sCot + l * kNllsTile;
    fvec4_t acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < kNllsTile / 4; ks += 2) {
      const int ka = 4 * ks + k4, kb = ka + 4;
      const float a0 = ra < R ? ua[ka] : 0.f, a1 = ra < R ? ua[kb] : 0.f;
      const float b0 = qb < Q ? vb[ka] * cl[ka] : 0.f, b1 = qb < Q ? vb[kb] * cl[kb] : 0.f;
      acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b0, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b1, acc1, 0, 0, 0);
    }
    const fvec4_t acc = acc0 + acc1;
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int r = ti * 16 + 4 * k4 + reg;
      if (r < R && qb < Q) slab[((size_t)r * Q + qb) * L + l] = acc[reg];
    }
  }
}

__global__ __launch_bounds__(256) void nll_sweep_reduce_kernel(const float *__restrict__ slabs, int tiles, int bsize, float *__restrict__ Gd) {
  for (int e = blockIdx.x * 256 + threadIdx.x; e < bsize; e += gridDim.x * 256) {
    float v = slabs[e];
    for (int t = 1; t < tiles; ++t) v += slabs[(size_t)t * bsize + e];
    Gd[e] = v;
  }
}

// three sums over the workgroup in a fixed order: a thread's own partial sums through a tree in LDS
__device__ inline void nlls_block_sum3(double &a, double &b, double &c, double *red) {
  const int tid = threadIdx.x;
  red[tid] = a; red[kNllsUpdThreads + tid] = b; red[2 * kNllsUpdThreads + tid] = c;
  __syncthreads();
  for (int w = kNllsUpdThreads / 2; w > 0; w >>= 1) {
    if (tid < w) {
      red[tid] += red[tid + w];
      red[kNllsUpdThreads + tid] += red[kNllsUpdThreads + tid + w];
      red[2 * kNllsUpdThreads + tid] += red[2 * kNllsUpdThreads + tid + w];
    }
    __syncthreads();
  }
  a = red[0]; b = red[kNllsUpdThreads]; c = red[2 * kNllsUpdThreads];
  __syncthreads();
}

__global__ __launch_bounds__(kNllsUpdThreads) void nll_sweep_update_kernel(NllSweepUpdateParams p) {
  extern __shared__ __attribute__((aligned(16))) double nlls_shd[];
  const int tid = threadIdx.x, D = p.D, L = p.L, h = p.h, g = p.g, Bs = p.bsize;
  const int RW = D * D * g * L;
  // T1[a][x] = sum_a' Nh[a][a'] B[a'][x]
  mm_lds(1, h, RW, h, p.Nh, 0, h, 1, p.B64, 0, RW, 1, [&](int, int i, int j, double v) { p.T1[(size_t)i * RW + j] = v; });
  __syncthreads();
  if (p.S) {
    // the metric on both feature axes in place: the thread of (a, c, l) owns its D x D elements
    const int gl = g * L;
    for (int e = tid; e < h * gl; e += kNllsUpdThreads) {
      double *t = p.T1 + (size_t)(e / gl) * RW + e % gl;
      double in[kD * kD];                                  // (D == kD: the launch function sees to it; registers, no scratch)
#pragma unroll
      for (int d = 0; d < kD * kD; ++d) in[d] = t[(size_t)d * gl];
#pragma unroll
      for (int d0 = 0; d0 < kD; ++d0)
#pragma unroll
        for (int d1 = 0; d1 < kD; ++d1) {
          double v = 0.0;
#pragma unroll
          for (int e0 = 0; e0 < kD; ++e0)
#pragma unroll
            for (int e1 = 0; e1 < kD; ++e1) v = fma(p.S[d0 * kD + e0] * p.S[d1 * kD + e1], in[e0 * kD + e1], v);
          t[(size_t)(d0 * kD + d1) * gl] = v;
        }
    }
    __syncthreads();
  }
  // T2[i][c][l] = sum_c' T1[i][c'][l] Ng[c'][c], i = (a, dk, dk1), the label as the batch
  mm_lds(L, h * D * D, g, g, p.T1, 1, g * L, L, p.Ng, 0, g, 1, [&](int l, int i, int j, double v) { p.T2[((size_t)i * g + j) * L + l] = v; });
  __syncthreads();
  double z = 0.0, q0 = 0.0, q1 = 0.0;
  for (int e = tid; e < Bs; e += kNllsUpdThreads) {
    const double b = p.B64[e];
    z = fma(b, p.T2[e], z);
    q0 = fma(b, b, q0);
  }
  double dummy = 0.0;
  nlls_block_sum3(z, q0, dummy, nlls_shd);
  const double two_over_z = 2.0 / z, lr = (double)p.lr;
  for (int e = tid; e < Bs; e += kNllsUpdThreads) {
    const double gz = two_over_z * p.T2[e], gd = (double)p.Gd[e];
    const double bn = fma(lr, gd - gz, p.B64[e]);
    p.T1[e] = bn;                                           // (T1 is dead: the unrounded B' waits there for its factor)
    q1 = fma(bn, bn, q1);
    p.dbg[e] = p.B64[e];
    p.dbg[(size_t)Bs + e] = gd;
    p.dbg[2 * (size_t)Bs + e] = gz;
  }
  {
    double d1 = 0.0, d2 = 0.0;
    nlls_block_sum3(q1, d1, d2, nlls_shd);
  }
  const double nbad = p.acc[1];
  int bits = p.env_status[0] & 3;
  if (!(fabs(z) <= kLnzDblMax)) bits |= 1;
  else if (z == 0.0) bits |= 2;
  if (!(nbad == 0.0)) bits |= kNllStepBadBatch;
  const double rs = p.renorm && q1 > 0.0 && q1 <= kLnzDblMax ? sqrt(q0 / q1) : 1.0;
  // an element beyond float32 (or a NaN that the sums let through) keeps the step from being applied, as bit 4 of section 24 does
  int over = 0;
  for (int e = tid; e < Bs; e += kNllsUpdThreads) over |= !(fabs(p.T1[e] * rs) <= 3.4028234e38) ? 1 : 0;
  over = __syncthreads_or(over);
  if (over && !bits) bits |= 4;
  int sk = *p.skip;
  __syncthreads();
  if (bits) sk = 1;
  if (sk) bits |= kNllStepNotApplied;
  for (int e = tid; e < Bs; e += kNllsUpdThreads) {
    const float v = sk ? (float)p.B64[e] : (float)(p.T1[e] * rs);
    p.Bout[e] = v;
    p.dbg[3 * (size_t)Bs + e] = (double)v;
  }
  if (tid == 0) {
    if (sk) *p.skip = 1;
    const double logz = log(fabs(z)) + 0.6931471805599453094 * (double)(p.expH[0] + p.expG[0]);
    p.rec[0] = -(p.acc[0] / (double)p.batch - logz);
    p.rec[1] = logz;
    p.rec[2] = nbad;
    p.rec[3] = (double)bits;
  }
}

__device__ inline double nlls_block_max(double x, double *red) {
  for (int o = 32; o > 0; o >>= 1) x = fmax(x, __shfl_xor(x, o, 64));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
  __syncthreads();
  double r = red[0];
  for (int w = 1; w < kNllsUpdWaves; ++w) r = fmax(r, red[w]);
  return r;
}

__global__ __launch_bounds__(kNllsUpdThreads) void nll_sweep_extend_kernel(NllSweepExtendParams p) {
  extern __shared__ __attribute__((aligned(16))) double nlls_shd[];
  const int tid = threadIdx.x, D = p.D;
  const bool right = p.right_walk != 0;
  const int m_kept = p.m_dev ? *p.m_dev : p.m_fixed;
  const int ml = right ? m_kept : p.ml, mr = right ? p.mr : m_kept, Dm = D * mr;
  const int nin = right ? mr : ml, nout = right ? ml : mr;
  const size_t m = (size_t)p.lds_m;
  double *E = nlls_shd, *En = E + m * m, *T = En + m * m, *red = T + m * D * m;
  const float *Al = p.core;
  if (tid == 0) {
    // the record of the split: kept rank, discarded weight sum_{j >= m} sigma_j^2 / sum sigma_j^2
    double tot = 0.0, tail = 0.0;
    for (int j = 0; j < p.n_sigma; ++j) {
      const double v = p.sigma[j] * p.sigma[j];
      tot += v;
      if (j >= m_kept) tail += v;
      p.sigma_out[j] = p.sigma[j];
    }
    p.rec[4] = (double)m_kept;
    p.rec[5] = tot > 0.0 ? tail / tot : 0.0;
  }
  for (int e = tid; e < nin * nin; e += kNllsUpdThreads) E[e] = p.Ein[e];
  for (int e = tid; e < nout * nout; e += kNllsUpdThreads) En[e] = 0.0;
  __syncthreads();
  if (right)   // T[(a, d)][c'] = sum_c A[a][d][c] E[c][c']
    mm_lds(1, ml * D, mr, mr, Al, 0, mr, 1, E, 0, mr, 1, [&](int, int r, int j, double v) { T[r * mr + j] = v; });
  else         // T[a'][(d, c)] = sum_a E[a][a'] A[a][d][c]
    mm_lds(1, ml, Dm, ml, E, 0, 1, ml, Al, 0, Dm, 1, [&](int, int r, int j, double v) { T[r * Dm + j] = v; });
  __syncthreads();
  if (p.S) {
    lnz_fold_metric(T, p.S, ml, mr, D, kNllsUpdThreads);
    __syncthreads();
  }
  if (right)   // E'[a][a'] += sum_x T[a][x] A[a'][x], x = (d, c')
    mm_lds(1, ml, ml, Dm, T, 0, Dm, 1, Al, 0, 1, Dm, [&](int, int r, int j, double v) { En[r * ml + j] += v; });
  else         // E'[c'][c] += sum_k A[k][c'] T[k][c], k = (a', d)
    mm_lds(1, mr, mr, ml * D, Al, 0, 1, mr, T, 0, mr, 1, [&](int, int r, int j, double v) { En[r * mr + j] += v; });
  __syncthreads();
  double mx = 0.0;
  for (int e = tid; e < nout * nout; e += kNllsUpdThreads) {
    const double a = fabs(En[e]);
    mx = fmax(mx, a <= kLnzDblMax ? a : INFINITY);
  }
  mx = nlls_block_max(mx, red);
  if (!(mx <= kLnzDblMax)) {
    if (tid == 0) atomicOr(p.status, 1);
    return;
  }
  const int kexp = mx > 0.0 ? ilogb(mx) + 1 : 0;
  for (int e = tid; e < nout * nout; e += kNllsUpdThreads) p.Eout[e] = ldexp(En[e], -kexp);
  if (tid == 0) p.exp_out[0] = p.exp_in[0] + kexp;
}

bool launch_nll_sweep_chain(const NllSweepChainParams &p, int tiles, hipStream_t st) {
  if (tiles < 1 || p.b_pad < tiles * kNllsTile || p.b_pad % kNllsTile || p.x_bpad < tiles * kNllsTile || p.cap < 1 || p.D < 2 || p.D > kMaxD || p.n_sites < 0) return false;
  const size_t lds = nll_sweep_chain_lds_bytes(p.cap, p.D);
  if (lds > 160 * 1024) return false;
  hipLaunchKernelGGL(nll_sweep_chain_kernel, dim3(tiles), dim3(kNllsThreads), lds, st, p);
  return true;
}

bool launch_nll_sweep_merge(const NllSweepMergeParams &p, hipStream_t st) {
  if (p.h < 1 || p.g < 1 || p.s < 1 || p.D < 2 || p.D > kMaxD || p.L < 1) return false;
  const int n = p.h * p.D * p.D * p.g * p.L;
  hipLaunchKernelGGL(nll_sweep_merge_kernel, dim3(std::min((n + 255) / 256, 1024)), dim3(256), 0, st, p);
  return true;
}

bool launch_nll_sweep_batch(const NllSweepBatchParams &p, int tiles, hipStream_t st) {
  if (tiles < 1 || p.b < 1 || p.b > tiles * kNllsTile || p.b_pad < tiles * kNllsTile || p.b_pad % kNllsTile || p.x_bpad < tiles * kNllsTile || p.h < 1 || p.g < 1 || p.L < 1 || p.D < 2 ||
      p.D > kMaxD || p.batch < 1 || (p.do_ext && p.hp < 1))
    return false;
  const size_t lds = nll_sweep_batch_lds_bytes(p.h, p.g, p.do_ext ? p.hp : 0, p.D, p.L);
  if (lds > 160 * 1024) return false;
  hipLaunchKernelGGL(nll_sweep_batch_kernel, dim3(tiles), dim3(kNllsThreads), lds, st, p);
  return true;
}

bool launch_nll_sweep_reduce(const float *slabs, int tiles, int bsize, float *Gd, hipStream_t st) {
  if (tiles < 1 || bsize < 1) return false;
  hipLaunchKernelGGL(nll_sweep_reduce_kernel, dim3(std::min((bsize + 255) / 256, 1024)), dim3(256), 0, st, slabs, tiles, bsize, Gd);
  return true;
}

bool launch_nll_sweep_update(const NllSweepUpdateParams &p, hipStream_t st) {
  if (p.h < 1 || p.g < 1 || p.L < 1 || p.D != kD || p.bsize != p.h * p.D * p.D * p.g * p.L || p.batch < 1 ||
      (p.renorm != 0 && p.renorm != 1) || (size_t)p.bsize >= ((size_t)1 << 23))
    return false;
  hipLaunchKernelGGL(nll_sweep_update_kernel, dim3(1), dim3(kNllsUpdThreads), nll_sweep_update_lds_bytes(), st, p);
  return true;
}

bool launch_nll_sweep_extend(const NllSweepExtendParams &p, int mb, hipStream_t st) {
  if (p.ml < 1 || p.mr < 1 || p.ml > mb || p.mr > mb || p.m_fixed < 1 || p.m_fixed > mb || mb > kLnzMaxBond || p.D < 2 || p.D > kMaxD ||
      p.n_sigma < 0 || p.n_sigma > kBigMaxN)
    return false;
  const size_t lds = nll_sweep_extend_lds_bytes(mb, p.D);
  if (lds > 160 * 1024) return false;
  NllSweepExtendParams q = p;
  q.lds_m = mb;
  hipLaunchKernelGGL(nll_sweep_extend_kernel, dim3(1), dim3(kNllsUpdThreads), lds, st, q);
  return true;
}

}  // namespace tnml
