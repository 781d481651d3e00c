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
//                       are streamed one slice at a time: P(l) for every l, the draw, then the slices that were chosen.  The draw
//                       itself is sample_device.h's, shared with kernels_sample_masked.hip.
// Status word: bit 1 a non-finite environment or density, bit 2 a sample whose densities sum to nothing (a clamped class or
// prefix of zero weight); status[1] is the smallest such sample.
#include "small_gemm_device.h"
#include "sample_device.h"

#include <cmath>

namespace tnml {

constexpr int kSmpThreads = 1024;
constexpr int kSmpWaves = kSmpThreads / 64;
constexpr int kSmpWalkThreads = 512;         // the walk: eight waves, two samples of the tile each (256 registers a lane: no scratch)
constexpr int kSmpWalkWaves = kSmpWalkThreads / 64;
constexpr int kSmpPerWave = kSmpTile / kSmpWalkWaves;
constexpr int kSmpAcc = 4;                  // elements of R' a thread owns at the most: bonds up to 64

size_t sample_env_lds_bytes(int mb, int D) {
  const size_t m = (size_t)mb;
  return (m * m + m * D * m + 2 * kSmpWaves) * sizeof(double);
}
size_t sample_walk_lds_bytes(int mb, int D, int L, int K) {
  const size_t m = (size_t)mb;
  return (m * m + 2 * kSmpTile * D * m + kSmpTile * m + (size_t)K * D + K + kSmpTile * D * D + (size_t)D * D + (size_t)kSmpTile * L) * sizeof(double) +
         smp_even(m * D * m) * sizeof(float) + (size_t)kSmpTile * sizeof(int);
}

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
    const int nr = smp_mr(p.bond, N, l);                         // R starts as R_{l+1}, nr x nr
    const double *src = p.env_shared + (size_t)(l + 1) * p.env_stride;
    for (int e = tid; e < nr * nr; e += kSmpThreads) R[e] = src[e];
  }
  int bad = 0, it = 0;
  __syncthreads();
  for (int i = first; i >= last; --i, ++it) {
    const int ml = smp_ml(p.bond, i), mr = smp_mr(p.bond, N, i), Dm = D * mr;
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

// what a wave carries for each of its two samples from site to site (the same in every lane)
struct SmpState {
  int sample, label, dead;
  double logp0, logp1;
};

// u[j] of the wave's sample, j the site or N for the label; a padding row draws with 0.5 and writes nothing
__device__ inline double smp_u(const SampleParams &p, const SmpState &st, int j) {
  return st.sample >= 0 ? (p.u ? p.u[(size_t)st.sample * (p.N + 1) + j] : smp_uniform(p.seed, st.sample, j, p.N)) : 0.5;
}

// The draw of one site for the wave's sample, from Q in LDS: the level (the clamped one inside the prefix), logp, the new v.
// active: the sample takes part (its label is the staged slice); otherwise nothing is written.
__device__ inline void smp_draw_pixel(const SampleParams &p, const SmpLds &s, SmpState &st, int smp, int lane, int i, int m, int mr, bool active) {
  const int D = p.D;
  const bool clamped = i < p.n_given && st.sample >= 0;
  const SmpPick pk = smp_pick_level(s.Q + smp * D * D, s.phi, s.w, p.K, D, lane, smp_u(p, st, i), clamped ? p.given[(size_t)st.sample * p.n_given + i] : -1);
  const double v = smp_next_v(s.phi + (size_t)pk.k * D, s.U + (size_t)smp * D * mr, D, mr, lane);
  if (active && st.sample >= 0) {
    smp_mark_dead(p.status, st.sample, st.dead, lane, pk.nonfinite, pk.total);
    const double term = log(pk.psel / pk.total);
    st.logp0 += term;
    if (clamped) st.logp1 += term;
    if (lane < mr) s.V[(size_t)smp * m + lane] = v;
    if (lane == 0) p.levels[(size_t)st.sample * p.N + i] = pk.k;
  }
}

// The label of the wave's sample from P(l') in LDS, by u[N]
__device__ inline void smp_draw_label(const SampleParams &p, const SmpLds &s, SmpState &st, int smp, int lane) {
  const SmpPick pk = smp_pick_label(s.P + smp * p.L, p.L, smp_u(p, st, p.N));
  st.label = pk.k;
  if (st.sample >= 0) {
    // (smp_mark_dead leaves a sample alone that a pixel before the label has marked already: its bit and its number are in the
    // status word, and sums that are not finite at the label without having been so before it come from an environment or a metric
    // that is not finite, for which sample_env_kernel has set bit 1 itself)
    smp_mark_dead(p.status, st.sample, st.dead, lane, pk.nonfinite, pk.total);
    st.logp0 += log(pk.psel / pk.total);
  }
  if (lane == 0) s.lab[smp] = st.sample >= 0 ? pk.k : -1;
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
  s.lab = (int *)(s.A + smp_even((size_t)m * D * m));
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
    const int ml = smp_ml(p.bond, i), mr = smp_mr(p.bond, N, i), nA = ml * D * mr;
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
      for (int h = 0; h < kSmpPerWave; ++h) {
        const int smp = wave + h * kSmpWalkWaves;
        smp_form_Q(s.T + (size_t)smp * D * mr, s.U + (size_t)smp * D * mr, s.Q + smp * D * D, D, mr, lane);
      }
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
