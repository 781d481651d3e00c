// Exact samples and log-likelihoods of the Born distribution |f|^2 of the chain over a pixel grid (tnml_sample).
// float64 throughout, no float atomic, every sum in a fixed order, no waiting between workgroups: the hand-overs are launch boundaries.
//   sample_env_kernel   the metric environments R_i[a][a'] = sum S[d][d'] A_i[a][d][c] R_{i+1}[c][c'] A_i[a'][d'][c'], R_N = 1, stored
//                       for EVERY site and multiplied by an exact power of two after each (the exponent is dropped: the walk needs R_i
//                       up to a factor).  phase 1: one workgroup walks N-1 .. l_pos+1, the part all class slots share.  phase 2: one
//                       workgroup per class slot a call needs (-1: the label summed, c: its slice c) walks l_pos .. 1 from phase 1's
//                       result.  Per site and label slice:
//                         1  AS[a][d'][c] = sum_d S[d'][d] A[a][d][c] as doubles into the workgroup's staging area of global memory;
//                         2  T = AS . R into LDS;  3  R'[a][a'] += sum_{d,c'} T[a][d][c'] A[a'][d][c'] in registers.
//   sample_walk_kernel  one workgroup per tile of 16 samples of one class slot, eight waves with two samples each.  Per site: A_i (float32) and
//                       R_{i+1} into LDS, U = V . A_i and T = U . R_{i+1} on the f64 matrix cores (mm_lds), then per sample
//                       Q = T U^T, the K densities w_k phi_k^T Q phi_k (four consecutive levels per lane), an inclusive scan over
//                       the wave, the search, the new v = phi_k^T U and its power-of-two rescale.  On the label site the classes
//                       are streamed one slice at a time: P(l) for every l, the draw, then the slices that were chosen.
// Status word: bit 1 a non-finite environment or density, bit 2 a sample whose densities sum to nothing (a clamped class or
// prefix of zero weight); status[1] is the smallest such sample.
#include "small_gemm_device.h"

#include <cmath>

namespace tnml {

constexpr int kSmpThreads = 1024;
constexpr int kSmpWaves = kSmpThreads / 64;
constexpr int kSmpWalkThreads = 512;         // the walk: eight waves, two samples of the tile each (256 registers a lane: no scratch)
constexpr int kSmpWalkWaves = kSmpWalkThreads / 64;
constexpr int kSmpPerWave = kSmpTile / kSmpWalkWaves;
constexpr int kSmpAcc = 4;                  // elements of R' a thread owns at the most: bonds up to 64
constexpr double kSmpDblMax = 1.7976931348623157e308;

static size_t smp_even(size_t x) { return (x + 1) & ~(size_t)1; }

size_t sample_env_lds_bytes(int mb, int D) {
  const size_t m = (size_t)mb;
  return (m * m + m * D * m + 2 * kSmpWaves) * sizeof(double);
}
size_t sample_walk_lds_bytes(int mb, int D, int L, int K) {
  const size_t m = (size_t)mb;
  return (m * m + 2 * kSmpTile * D * m + kSmpTile * m + (size_t)K * D + K + kSmpTile * D * D + (size_t)D * D + (size_t)kSmpTile * L) * sizeof(double) +
         smp_even(m * D * m) * sizeof(float) + (size_t)kSmpTile * sizeof(int);
}

__device__ inline int smp_ml(const SampleParams &p, int i) { return i == 0 ? 1 : p.bond[i - 1]; }
__device__ inline int smp_mr(const SampleParams &p, int i) { return i == p.N - 1 ? 1 : p.bond[i]; }
// R_i of compact slot `slot`: the shared stack beyond the label site, the slot's own up to it
__device__ inline double *smp_env(const SampleParams &p, int slot, int i) {
  return i > p.l_pos ? p.env_shared + (size_t)i * p.env_stride : p.env_slots + ((size_t)slot * (p.l_pos + 1) + i) * p.env_stride;
}

__device__ double smp_block_max(double x, double *red) {
  for (int o = 32; o > 0; o >>= 1) x = fmax(x, __shfl_xor(x, o, 64));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
  __syncthreads();
  double r = red[0];
  for (int w = 1; w < kSmpWaves; ++w) r = fmax(r, red[w]);
  return r;
}

__global__ __launch_bounds__(kSmpThreads) void sample_env_kernel(SampleParams p) {
  extern __shared__ __attribute__((aligned(16))) double smp_sh[];
  const int tid = threadIdx.x, N = p.N, D = p.D, l = p.l_pos, wg = blockIdx.x;
  const size_t m = (size_t)p.lds_m;
  double *R = smp_sh, *T = R + m * m, *red = T + m * D * m;
  double *AS = p.stage + (size_t)wg * p.stage_stride;
  const int q = p.phase == 2 ? p.slot_class[wg] : -1;
  const int first = p.phase == 1 ? N - 1 : l, last = p.phase == 1 ? l + 1 : 1;
  if (p.phase == 1) {
    if (tid == 0) { R[0] = 1.0; p.env_shared[(size_t)N * p.env_stride] = 1.0; }
  } else {
    const int nr = smp_mr(p, l);                                 // R starts as R_{l+1}, nr x nr
    const double *src = p.env_shared + (size_t)(l + 1) * p.env_stride;
    for (int e = tid; e < nr * nr; e += kSmpThreads) R[e] = src[e];
  }
  int bad = 0, it = 0;
  __syncthreads();
  for (int i = first; i >= last; --i, ++it) {
    const int ml = smp_ml(p, i), mr = smp_mr(p, i), Dm = D * mr;
    const bool lab = i == l;
    const int Lx = lab ? p.L : 1, l0 = lab && q >= 0 ? q : 0, l1 = lab && q < 0 ? p.L : l0 + 1;
    const float *A = lab ? p.lab : p.cores + (size_t)i * p.core_stride;
    double acc[kSmpAcc];
#pragma unroll
    for (int k = 0; k < kSmpAcc; ++k) acc[k] = 0.0;
    for (int lp = l0; lp < l1; ++lp) {
      // 1  the metric folded into the core
      for (int e = tid; e < ml * Dm; e += kSmpThreads) {
        const int c = e % mr, d = (e / mr) % D, a = e / Dm;
        double v = 0.0;
        for (int dd = 0; dd < D; ++dd) v = fma(p.S[d * D + dd], (double)A[(((size_t)a * D + dd) * mr + c) * Lx + lp], v);
        AS[e] = v;
      }
      __syncthreads();
      // 2  T[(a, d)][c'] = sum_c AS[(a, d)][c] R[c][c']
      for (int e = tid; e < ml * Dm; e += kSmpThreads) {
        const int cp = e % mr, ad = e / mr;
        const double *as = AS + (size_t)ad * mr;
        double v = 0.0;
        for (int c = 0; c < mr; ++c) v = fma(as[c], R[c * mr + cp], v);
        T[e] = v;
      }
      __syncthreads();
      // 3  R'[a][a'] += sum_x T[a][x] A[a'][x],  x = (d, c')
#pragma unroll
      for (int k = 0; k < kSmpAcc; ++k) {
        const int e = tid + k * kSmpThreads;
        if (e < ml * ml) {
          const int a = e / ml, ap = e % ml;
          const double *t = T + (size_t)a * Dm;
          const float *b = A + ((size_t)ap * Dm) * Lx + lp;
          double v = acc[k];
          for (int x = 0; x < Dm; ++x) v = fma(t[x], (double)b[(size_t)x * Lx], v);
          acc[k] = v;
        }
      }
      __syncthreads();
    }
    double mx = 0.0;
#pragma unroll
    for (int k = 0; k < kSmpAcc; ++k) {
      const double a = fabs(acc[k]);
      mx = fmax(mx, a <= kSmpDblMax ? a : INFINITY);              // (a NaN fails the comparison)
    }
    mx = smp_block_max(mx, red + (it & 1) * kSmpWaves);
    if (!(mx <= kSmpDblMax)) { bad = 1; break; }
    const int kexp = mx > 0.0 ? ilogb(mx) + 1 : 0;
    double *out = smp_env(p, wg, i);
#pragma unroll
    for (int k = 0; k < kSmpAcc; ++k) {
      const int e = tid + k * kSmpThreads;
      if (e < ml * ml) {
        const double v = ldexp(acc[k], -kexp);
        R[e] = v;
        out[e] = v;
      }
    }
    __syncthreads();
  }
  if (bad && tid == 0) atomicOr(p.status, 1);
}

__device__ inline double smp_uniform(unsigned long long seed, long long s, int j, int N) {
  unsigned long long z = seed + ((unsigned long long)s * (unsigned long long)(N + 1) + (unsigned long long)j + 1ull) * 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z = z ^ (z >> 31);
  return (double)(z >> 11) * 1.1102230246251565e-16;             // 2^-53
}

// the LDS areas of the walk kernel
struct SmpLds {
  double *R, *U, *T, *V, *phi, *w, *Q, *S, *P;
  float *A;
  int *lab;
};

// one core slice (ml, D, mr) into LDS as it is stored; stride Lx, slice lp on the label site
__device__ inline void smp_stage_core(const float *A, int n, int Lx, int lp, float *dst) {
  for (int e = threadIdx.x; e < n; e += kSmpWalkThreads) dst[e] = A[(size_t)e * Lx + lp];
}

// U = V . A (16 x D mr) and T = U . R (16 D x mr) on the matrix cores; both end behind a barrier
__device__ inline void smp_products(const SmpLds &s, int m, int ml, int mr, int D) {
  const int Dm = D * mr;
  double *U = s.U, *T = s.T;
  mm_lds(1, kSmpTile, Dm, ml, s.V, 0, m, 1, s.A, 0, Dm, 1, [&](int, int i, int j, double v) { U[i * Dm + j] = v; });
  __syncthreads();
  mm_lds(1, kSmpTile * D, mr, mr, s.U, 0, mr, 1, s.R, 0, mr, 1, [&](int, int i, int j, double v) { T[i * mr + j] = v; });
  __syncthreads();
}

// Q[d][d'] = sum_c T[d][c] U[d'][c] of one sample of the wave into LDS
__device__ inline void smp_form_Q(const SmpLds &s, int smp, int lane, int mr, int D) {
  if (lane < D * D) {
    const double *t = s.T + (size_t)(smp * D + lane / D) * mr, *u = s.U + (size_t)(smp * D + lane % D) * mr;
    double v = 0.0;
    for (int c = 0; c < mr; ++c) v = fma(t[c], u[c], v);
    s.Q[smp * D * D + lane] = v;
  }
}

// what a wave carries for each of its two samples from site to site (the same in every lane)
struct SmpState {
  int sample, label, dead;
  double logp0, logp1;
};

// The draw of one site for the wave's sample, from Q in LDS: densities, scan, search (or the clamped level), logp, the new v.
// active: the sample takes part (its label is the staged slice); otherwise nothing is written.
__device__ inline void smp_draw_pixel(const SampleParams &p, const SmpLds &s, SmpState &st, int smp, int lane, int i, int m, int mr, bool active) {
  const int D = p.D, K = p.K, N = p.N;
  const double *Q = s.Q + smp * D * D;
  double pl[4];
  bool nonfinite = false;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int k = 4 * lane + j;
    double v = 0.0;
    if (k < K) {
      const double *ph = s.phi + (size_t)k * D;
      double a = 0.0;
      for (int d = 0; d < D; ++d) {
        double t = 0.0;
        for (int dd = 0; dd < D; ++dd) t = fma(Q[d * D + dd], ph[dd], t);
        a = fma(ph[d], t, a);
      }
      v = s.w[k] * a;
      if (!(fabs(v) <= kSmpDblMax)) { nonfinite = true; v = 0.0; }
      v = v > 0.0 ? v : 0.0;
    }
    pl[j] = v;
  }
  const double c0 = pl[0], c1 = c0 + pl[1], c2 = c1 + pl[2], c3 = c2 + pl[3];
  double x = c3;
  for (int o = 1; o < 64; o <<= 1) {
    const double y = __shfl_up(x, o, 64);
    if (lane >= o) x += y;
  }
  double excl = __shfl_up(x, 1, 64);
  if (lane == 0) excl = 0.0;
  const double total = __shfl(x, 63, 64);
  const double u = st.sample >= 0 ? (p.u ? p.u[(size_t)st.sample * (N + 1) + i] : smp_uniform(p.seed, st.sample, i, N)) : 0.5;
  const double t = u * total;
  const double cl[4] = {excl + c0, excl + c1, excl + c2, excl + c3};
  int cand = 1 << 20, lastpos = -1;
#pragma unroll
  for (int j = 3; j >= 0; --j) {
    const int k = 4 * lane + j;
    if (k < K && cl[j] > t) cand = k;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (pl[j] > 0.0) lastpos = 4 * lane + j;
  for (int o = 32; o > 0; o >>= 1) {
    cand = min(cand, __shfl_xor(cand, o, 64));
    lastpos = max(lastpos, __shfl_xor(lastpos, o, 64));
    nonfinite = nonfinite || __shfl_xor((int)nonfinite, o, 64);
  }
  int k = cand < K ? cand : (lastpos >= 0 ? lastpos : 0);
  const bool clamped = i < p.n_given && st.sample >= 0;
  if (clamped) k = p.given[(size_t)st.sample * p.n_given + i];
  const int j = k & 3;
  const double mine = j == 0 ? pl[0] : j == 1 ? pl[1] : j == 2 ? pl[2] : pl[3];
  const double psel = __shfl(mine, k >> 2, 64);
  // the new v and its rescale
  double v = 0.0;
  if (lane < mr) {
    const double *ph = s.phi + (size_t)k * D;
    for (int d = 0; d < D; ++d) v = fma(ph[d], s.U[(size_t)(smp * D + d) * mr + lane], v);
  }
  double mx = fabs(v);
  for (int o = 32; o > 0; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o, 64));
  if (mx > 0.0 && mx <= kSmpDblMax) v = ldexp(v, -(ilogb(mx) + 1));
  if (active && st.sample >= 0) {
    if (!st.dead) {
      if (nonfinite) { st.dead = 1; if (lane == 0) atomicOr(p.status, 1); }
      else if (!(total > 0.0)) { st.dead = 1; if (lane == 0) { atomicOr(p.status, 2); atomicMin(p.status + 1, st.sample); } }
    }
    const double term = log(psel / total);
    st.logp0 += term;
    if (clamped) st.logp1 += term;
    if (lane < mr) s.V[(size_t)smp * m + lane] = v;
    if (lane == 0) p.levels[(size_t)st.sample * N + i] = k;
  }
}

// The label of the wave's sample from P(l') in LDS, by u[N] and the rule of the pixels (every lane computes the same)
__device__ inline void smp_draw_label(const SampleParams &p, const SmpLds &s, SmpState &st, int smp, int lane) {
  const int L = p.L, N = p.N;
  double total = 0.0;
  bool nonfinite = false;
  for (int lp = 0; lp < L; ++lp) {
    const double a = s.P[smp * L + lp];
    if (!(fabs(a) <= kSmpDblMax)) nonfinite = true;
    else total += a > 0.0 ? a : 0.0;
  }
  const double u = st.sample >= 0 ? (p.u ? p.u[(size_t)st.sample * (N + 1) + N] : smp_uniform(p.seed, st.sample, N, N)) : 0.5;
  const double t = u * total;
  int pick = -1, lastpos = 0;
  double c = 0.0, psel = 0.0, plast = 0.0;
  for (int lp = 0; lp < L; ++lp) {
    const double a0 = s.P[smp * L + lp], a = a0 > 0.0 && a0 <= kSmpDblMax ? a0 : 0.0;
    c += a;
    if (pick < 0 && c > t) { pick = lp; psel = a; }
    if (a > 0.0) { lastpos = lp; plast = a; }
  }
  if (pick < 0) { pick = lastpos; psel = plast; }
  st.label = pick;
  if (st.sample >= 0) {
    if (nonfinite) { st.dead = 1; if (lane == 0) atomicOr(p.status, 1); }
    else if (!(total > 0.0)) { st.dead = 1; if (lane == 0) { atomicOr(p.status, 2); atomicMin(p.status + 1, st.sample); } }
    st.logp0 += log(psel / total);
  }
  if (lane == 0) s.lab[smp] = st.sample >= 0 ? pick : -1;
}

__global__ __launch_bounds__(kSmpWalkThreads) void sample_walk_kernel(SampleParams p) {
  extern __shared__ __attribute__((aligned(16))) double smp_sh[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, tile = blockIdx.x;
  const int N = p.N, D = p.D, L = p.L, K = p.K, l = p.l_pos, m = p.lds_m;
  SmpLds s;
  s.R = smp_sh;
  s.U = s.R + (size_t)m * m;
  s.T = s.U + (size_t)kSmpTile * D * m;
  s.V = s.T + (size_t)kSmpTile * D * m;
  s.phi = s.V + (size_t)kSmpTile * m;
  s.w = s.phi + (size_t)K * D;
  s.Q = s.w + K;
  s.S = s.Q + kSmpTile * D * D;
  s.P = s.S + D * D;
  s.A = (float *)(s.P + (size_t)kSmpTile * L);
  s.lab = (int *)(s.A + (((size_t)m * D * m + 1) & ~(size_t)1));
  const int slot = p.tile_slot[tile], q = p.slot_class[slot];
  SmpState st[kSmpPerWave];
#pragma unroll
  for (int h = 0; h < kSmpPerWave; ++h) {
    st[h].sample = p.tile_samples[tile * kSmpTile + wave + h * kSmpWalkWaves];
    st[h].label = st[h].sample >= 0 ? p.classes[st[h].sample] : q;
    st[h].dead = 0;
    st[h].logp0 = st[h].logp1 = 0.0;
  }
  for (int e = tid; e < K * D; e += kSmpWalkThreads) s.phi[e] = p.phi[e];
  for (int e = tid; e < K; e += kSmpWalkThreads) s.w[e] = p.w[e];
  for (int e = tid; e < D * D; e += kSmpWalkThreads) s.S[e] = p.S[e];
  for (int e = tid; e < kSmpTile * m; e += kSmpWalkThreads) s.V[e] = (e % m) == 0 ? 1.0 : 0.0;
  __syncthreads();
  for (int i = 0; i < N; ++i) {
    const int ml = smp_ml(p, i), mr = smp_mr(p, i), nA = ml * D * mr;
    const double *Rg = smp_env(p, slot, i + 1);
    for (int e = tid; e < mr * mr; e += kSmpWalkThreads) s.R[e] = Rg[e];
    // One pass per staged core slice.  A plain site and a label site with a given class have one; a label site whose label is
    // drawn has L passes that only form P(l') = tr(S Q^(l')), the draw, and L more for the slices that were chosen.
    const bool lab = i == l, joint = lab && q < 0;
    const int npass = joint ? 2 * L : 1, Lx = lab ? L : 1;
    const float *Ag = lab ? p.lab : p.cores + (size_t)i * p.core_stride;
    for (int pass = 0; pass < npass; ++pass) {
      const int lp = joint ? (pass < L ? pass : pass - L) : (lab ? q : 0);
      if (joint && pass == L) {
#pragma unroll
        for (int h = 0; h < kSmpPerWave; ++h) smp_draw_label(p, s, st[h], wave + h * kSmpWalkWaves, lane);
        __syncthreads();
      }
      if (joint && pass >= L) {
        bool any = false;
        for (int k = 0; k < kSmpTile; ++k) any = any || s.lab[k] == lp;
        if (!any) continue;                                      // (the same in every thread)
      }
      smp_stage_core(Ag, nA, Lx, lp, s.A);
      __syncthreads();
      smp_products(s, m, ml, mr, D);
#pragma unroll
      for (int h = 0; h < kSmpPerWave; ++h) smp_form_Q(s, wave + h * kSmpWalkWaves, lane, mr, D);
      __syncthreads();
#pragma unroll
      for (int h = 0; h < kSmpPerWave; ++h) {
        const int smp = wave + h * kSmpWalkWaves;
        if (joint && pass < L) {
          if (lane == 0) {
            double a = 0.0;
            for (int e = 0; e < D * D; ++e) a = fma(s.S[e], s.Q[smp * D * D + e], a);
            s.P[smp * L + lp] = a;
          }
        } else {
          smp_draw_pixel(p, s, st[h], smp, lane, i, m, mr, !joint || st[h].label == lp);
        }
      }
      __syncthreads();
    }
  }
#pragma unroll
  for (int h = 0; h < kSmpPerWave; ++h)
    if (st[h].sample >= 0 && lane == 0) {
      p.labels[st[h].sample] = st[h].label;
      p.logp[2 * (size_t)st[h].sample] = st[h].logp0;
      p.logp[2 * (size_t)st[h].sample + 1] = st[h].logp1;
    }
}

static bool smp_geometry(const SampleParams &p) {
  return p.N >= 2 && p.D >= 2 && p.D <= kMaxD && p.L >= 1 && p.l_pos >= 0 && p.l_pos < p.N && p.K >= 2 && p.K <= kSmpMaxK && p.n >= 1 &&
         p.n_given >= 0 && p.n_given <= p.N && p.n_slots >= 1 && p.n_tiles >= 1;
}

bool launch_sample(const SampleParams &p, int mb, hipStream_t st) {
  if (!smp_geometry(p) || mb < 1 || mb > kSmpMaxBond) return false;
  const size_t m = (size_t)mb, le = sample_env_lds_bytes(mb, p.D), lw = sample_walk_lds_bytes(mb, p.D, p.L, p.K);
  if (le > 160 * 1024 || lw > 160 * 1024 || m * m > (size_t)kSmpAcc * kSmpThreads) return false;
  if (p.env_stride < m * m || p.stage_stride < m * p.D * m) return false;
  SampleParams q = p;
  q.lds_m = mb;
  q.phase = 1;
  hipLaunchKernelGGL(sample_env_kernel, dim3(1), dim3(kSmpThreads), le, st, q);
  if (q.l_pos >= 1) {
    q.phase = 2;
    hipLaunchKernelGGL(sample_env_kernel, dim3(q.n_slots), dim3(kSmpThreads), le, st, q);
  }
  q.phase = 0;
  hipLaunchKernelGGL(sample_walk_kernel, dim3(q.n_tiles), dim3(kSmpWalkThreads), lw, st, q);
  return true;
}

}  // namespace tnml
