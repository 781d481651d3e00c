// Samples and log-likelihoods given ANY set of known pixels (tnml_sample_masked).  float64 throughout, no float
// atomic, every sum in a fixed order, no waiting between workgroups: two launches, environment then walk.  A ROW is a sample of the
// call, or the empty mask of a class slot (its normaliser, or the padding behind the last sample of a slot); a tile holds T rows of
// ONE class slot (-1: the label summed, c: its slice c).  Each row's arithmetic touches only its own rows of every operand, so a
// result depends neither on T nor on the rows that share the tile.
//   sample_env_masked_kernel   one workgroup per tile walks N-1 .. 0 once.  Per site it stages A_i (float32 as stored) into LDS once
//                              for the tile, then on the f64 matrix cores (mm_lds)
//                                1  T0[(a,d)][s,c'] = sum_c A[a,d,c] R_s[c,c']               rows as columns: (ml D x mr)(mr x T mr)
//                                2  T0_s[a][d][c'] <- sum_d' S_{s,i}[d][d'] T0_s[a][d'][c']   the row's own metric, elementwise
//                                3  R'_s[a][a'] (+)= sum_{d,c'} T0_s[a][d,c'] A[a'][d,c']     rows as rows:    (T ml x D mr)(D mr x ml)
//                              into the row's stack slot of site i (the label site adds its slices there, one after the other), then
//                              per row the largest magnitude, the power of two, the exponent sum and R_{s,i} back into LDS.  S_{s,i} is
//                              w_k phi_k phi_k^T on a known site and S on a free one: the only place a mask is looked at.
//                              E[row] = log R_{s,0} + ln2 sum k (-inf where R_{s,0} <= 0).
//   sample_walk_masked_kernel  the walk of kernels_sample.hip with T_s = U_s . R_{s,i+1} as a product batched per row; on a known site
//                              nothing is drawn and no density is formed, v' = phi_k^T U only; the label is drawn with the row's own
//                              metric of the label site.  The draw itself is sample_device.h's, as in kernels_sample.hip.
// Status word: bit 1 a non-finite environment or density, bit 2 a sample whose densities sum to nothing; status[1] the smallest such.
#include "small_gemm_device.h"
#include "sample_device.h"

#include <cmath>

namespace tnml {

constexpr int kSmkThreads = 512;
constexpr int kSmkWaves = kSmkThreads / 64;
constexpr int kSmkPerWave = kSmkMaxTile / kSmkWaves;        // rows of a tile a wave of the walk owns at the most
constexpr double kSmkLn2 = 0.6931471805599453;

size_t sample_masked_env_lds_bytes(int mb, int D, int T) {
  const size_t m = (size_t)mb, t = (size_t)T;
  return (t * m * m + t * m * D * m + t * D * D) * sizeof(double) + 2 * t * sizeof(int) + smp_even(m * D * m) * sizeof(float);
}
size_t sample_masked_walk_lds_bytes(int mb, int D, int L, int K, int T) {
  const size_t m = (size_t)mb, t = (size_t)T;
  return (t * m * m + 2 * t * D * m + t * m + (size_t)K * D + K + 2 * t * D * D + t * L) * sizeof(double) + smp_even(m * D * m) * sizeof(float) +
         2 * t * sizeof(int);
}

// R_{s,i} of row `row` of the launch
__device__ inline double *smk_env(const SampleMaskedParams &p, int row, int i) {
  return p.stack + ((size_t)row * (p.N + 1) + i) * p.env_stride;
}
// the known level of sample smp on site i, -1 where the site is free (rows without a sample have the empty mask)
__device__ inline int smk_known(const SampleMaskedParams &p, int smp, int i) {
  if (smp < 0 || !p.mask[(size_t)(p.mask_rows == 1 ? 0 : smp) * p.N + i]) return -1;
  return p.known[(size_t)smp * p.N + i];
}
// S_{s,i}[e] into dst for the T rows of a tile
__device__ inline void smk_metric(const SampleMaskedParams &p, const int *srow, int i, double *dst) {
  const int D = p.D, DD = D * D;
  for (int e = threadIdx.x; e < p.T * DD; e += kSmkThreads) {
    const int s = e / DD, r = e - s * DD, d = r / D, dd = r - d * D;
    const int k = smk_known(p, srow[s], i);
    dst[e] = k < 0 ? p.S[r] : p.w[k] * (p.phi[(size_t)k * D + d] * p.phi[(size_t)k * D + dd]);
  }
}

__global__ __launch_bounds__(kSmkThreads) void sample_env_masked_kernel(SampleMaskedParams p) {
  extern __shared__ __attribute__((aligned(16))) double smk_sh[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, tile = blockIdx.x;
  const int N = p.N, D = p.D, T = p.T, l = p.l_pos, m = p.lds_m;
  double *Rl = smk_sh;                                            // [mr][T mr]: the rows' R_{i+1} side by side
  double *T0 = Rl + (size_t)T * m * m;                            // [T ml][D mr]
  double *Ss = T0 + (size_t)T * m * D * m;                        // [T][D][D]
  int *esum = (int *)(Ss + T * D * D);                            // [T]
  int *srow = esum + T;                                           // [T]
  float *A = (float *)(srow + T);                                 // [ml][D][mr]
  const int q = p.tile_class[tile];
  for (int s = tid; s < T; s += kSmkThreads) {
    Rl[s] = 1.0;
    esum[s] = 0;
    srow[s] = p.tile_rows[tile * T + s];
    smk_env(p, tile * T + s, N)[0] = 1.0;
  }
  __syncthreads();
  for (int i = N - 1; i >= 0; --i) {
    const int ml = smp_ml(p.bond, i), mr = smp_mr(p.bond, N, i), Dm = D * mr, Tm = T * mr;
    const bool lab = i == l;
    const int Lx = lab ? p.L : 1, l0 = lab && q >= 0 ? q : 0, l1 = lab && q < 0 ? p.L : l0 + 1;
    const float *Ag = lab ? p.lab : p.cores + (size_t)i * p.core_stride;
    smk_metric(p, srow, i, Ss);
    for (int lp = l0; lp < l1; ++lp) {
      for (int e = tid; e < ml * Dm; e += kSmkThreads) A[e] = Ag[(size_t)e * Lx + lp];
      __syncthreads();
      // 1  T0[(s, a)][(d, c')] = sum_c A[(a, d)][c] Rl[c][(s, c')]
      mm_lds(1, ml * D, Tm, mr, A, 0, mr, 1, Rl, 0, Tm, 1, [&](int, int ad, int j, double v) {
        const int s = j / mr, cp = j - s * mr, a = ad / D, d = ad - a * D;
        T0[((size_t)(s * ml + a) * D + d) * mr + cp] = v;
      });
      __syncthreads();
      // 2  the row's metric over d, in place: one thread per (s, a, c')
      for (int e = tid; e < T * ml * mr; e += kSmkThreads) {
        const int cp = e % mr, sa = e / mr, s = sa / ml;
        double *t = T0 + (size_t)sa * Dm + cp;
        const double *sm = Ss + s * D * D;
        double in[kMaxD], out[kMaxD];
#pragma unroll
        for (int d = 0; d < kMaxD; ++d)
          if (d < D) in[d] = t[d * mr];
#pragma unroll
        for (int d = 0; d < kMaxD; ++d)
          if (d < D) {
            double v = 0.0;
#pragma unroll
            for (int dd = 0; dd < kMaxD; ++dd)
              if (dd < D) v = fma(sm[d * D + dd], in[dd], v);
            out[d] = v;
          }
#pragma unroll
        for (int d = 0; d < kMaxD; ++d)
          if (d < D) t[d * mr] = out[d];
      }
      __syncthreads();
      // 3  R'[(s, a)][a'] (+)= sum_x T0[(s, a)][x] A[a'][x],  x = (d, c'), into the row's stack slot of this site
      const bool first = lp == l0;
      mm_lds(1, T * ml, ml, Dm, T0, 0, Dm, 1, A, 0, 1, Dm, [&](int, int sa, int ap, double v) {
        const int s = sa / ml, a = sa - s * ml;
        double *out = smk_env(p, tile * T + s, i) + a * ml + ap;
        *out = first ? v : *out + v;
      });
      __syncthreads();
    }
    // per row: the largest magnitude, the power of two, the exponent sum; R_{s,i} to its slot and into LDS for the next site
    for (int s = wave; s < T; s += kSmkWaves) {
      double *out = smk_env(p, tile * T + s, i);
      double mx = 0.0;
      for (int e = lane; e < ml * ml; e += 64) {
        const double a = fabs(out[e]);
        mx = fmax(mx, a <= kSmpDblMax ? a : INFINITY);          // (a NaN fails the comparison)
      }
      for (int o = 32; o > 0; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o, 64));
      int kexp = 0;
      if (!(mx <= kSmpDblMax)) { if (lane == 0) atomicOr(p.status, 1); }
      else if (mx > 0.0) kexp = ilogb(mx) + 1;
      for (int e = lane; e < ml * ml; e += 64) {
        const double v = ldexp(out[e], -kexp);
        const int c = e / ml, cp = e - c * ml;
        out[e] = v;
        Rl[(size_t)c * (T * ml) + s * ml + cp] = v;
      }
      if (lane == 0) esum[s] += kexp;
    }
    __syncthreads();
  }
  for (int s = tid; s < T; s += kSmkThreads) {
    const double r0 = Rl[s];                                      // R_{s,0} is 1 x 1
    p.E[tile * T + s] = r0 > 0.0 ? log(r0) + kSmkLn2 * (double)esum[s] : (r0 == r0 ? -INFINITY : r0);
  }
}

// the LDS areas of the walk kernel
struct SmkLds {
  double *R, *U, *T, *V, *phi, *w, *Q, *S, *P;
  float *A;
  int *lab, *srow;
};

// what a wave carries for each of its rows from site to site (the same in every lane)
struct SmkState {
  int sample, label, dead;
  double logp0;
};

// u[j] of the row's sample, j the site or N for the label
__device__ inline double smk_u(const SampleMaskedParams &p, const SmkState &st, int j) {
  return p.u ? p.u[(size_t)st.sample * (p.N + 1) + j] : smp_uniform(p.seed, st.sample, j, p.N);
}

// One site of the wave's row smp (a sample): on a free site Q, the draw of the level and the log share; on a known one the given
// level; then the new v.
__device__ inline void smk_pixel(const SampleMaskedParams &p, const SmkLds &s, SmkState &st, int smp, int lane, int i, int m, int mr) {
  const int D = p.D;
  const double *U = s.U + (size_t)smp * D * mr;
  int k = smk_known(p, st.sample, i);
  if (k < 0) {
    double *Q = s.Q + smp * D * D;
    smp_form_Q(s.T + (size_t)smp * D * mr, U, Q, D, mr, lane);
    __builtin_amdgcn_wave_barrier();
    const SmpPick pk = smp_pick_level(Q, s.phi, s.w, p.K, D, lane, smk_u(p, st, i), -1);
    k = pk.k;
    smp_mark_dead(p.status, st.sample, st.dead, lane, pk.nonfinite, pk.total);
    st.logp0 += log(pk.psel / pk.total);
  }
  const double v = smp_next_v(s.phi + (size_t)k * D, U, D, mr, lane);
  if (lane < mr) s.V[(size_t)smp * m + lane] = v;
  if (lane == 0) p.levels[(size_t)st.sample * p.N + i] = k;
}

// The label of the wave's row from P(l') in LDS, by u[N]
__device__ inline void smk_label(const SampleMaskedParams &p, const SmkLds &s, SmkState &st, int smp, int lane) {
  const SmpPick pk = smp_pick_label(s.P + smp * p.L, p.L, smk_u(p, st, p.N));
  st.label = pk.k;
  smp_mark_dead(p.status, st.sample, st.dead, lane, pk.nonfinite, pk.total);
  st.logp0 += log(pk.psel / pk.total);
  if (lane == 0) s.lab[smp] = pk.k;
}

__global__ __launch_bounds__(kSmkThreads) void sample_walk_masked_kernel(SampleMaskedParams p) {
  extern __shared__ __attribute__((aligned(16))) double smk_sh[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, tile = blockIdx.x;
  const int N = p.N, D = p.D, L = p.L, K = p.K, T = p.T, l = p.l_pos, m = p.lds_m;
  SmkLds s;
  s.R = smk_sh;                                                   // [T][mr][mr]
  s.U = s.R + (size_t)T * m * m;                                  // [T][D][mr]
  s.T = s.U + (size_t)T * D * m;
  s.V = s.T + (size_t)T * D * m;                                  // [T][m]
  s.phi = s.V + (size_t)T * m;
  s.w = s.phi + (size_t)K * D;
  s.Q = s.w + K;                                                  // [T][D][D]
  s.S = s.Q + T * D * D;                                          // [T][D][D]: the rows' metric of the label site
  s.P = s.S + T * D * D;                                          // [T][L]
  s.A = (float *)(s.P + (size_t)T * L);
  s.lab = (int *)(s.A + smp_even((size_t)m * D * m));
  s.srow = s.lab + T;
  const int q = p.tile_class[tile];
  SmkState st[kSmkPerWave];
#pragma unroll
  for (int h = 0; h < kSmkPerWave; ++h) {
    const int smp = wave + h * kSmkWaves;
    st[h].sample = smp < T ? p.tile_rows[tile * T + smp] : -1;
    st[h].label = q;
    st[h].dead = 0;
    st[h].logp0 = 0.0;
  }
  for (int e = tid; e < K * D; e += kSmkThreads) s.phi[e] = p.phi[e];
  for (int e = tid; e < K; e += kSmkThreads) s.w[e] = p.w[e];
  for (int e = tid; e < T * m; e += kSmkThreads) s.V[e] = (e % m) == 0 ? 1.0 : 0.0;
  for (int e = tid; e < T; e += kSmkThreads) { s.srow[e] = p.tile_rows[tile * T + e]; s.lab[e] = -1; }
  __syncthreads();
  smk_metric(p, s.srow, l, s.S);
  for (int i = 0; i < N; ++i) {
    const int ml = smp_ml(p.bond, i), mr = smp_mr(p.bond, N, i), nA = ml * D * mr, Dm = D * mr, m2 = mr * mr;
    for (int e = tid; e < T * m2; e += kSmkThreads) {
      const int r = e / m2;
      s.R[e] = smk_env(p, tile * T + r, i + 1)[e - r * m2];
    }
    // One pass per staged core slice.  A plain site and a label site with a given class have one; a label site whose label is
    // drawn has L passes that only form P(l') = tr(S_s Q^(l')), the draw, and L more for the slices that were chosen.
    const bool lab = i == l, joint = lab && q < 0;
    const int npass = joint ? 2 * L : 1, Lx = lab ? L : 1;
    const float *Ag = lab ? p.lab : p.cores + (size_t)i * p.core_stride;
    for (int pass = 0; pass < npass; ++pass) {
      const int lp = joint ? (pass < L ? pass : pass - L) : (lab ? q : 0);
      if (joint && pass == L) {
#pragma unroll
        for (int h = 0; h < kSmkPerWave; ++h)
          if (st[h].sample >= 0) smk_label(p, s, st[h], wave + h * kSmkWaves, lane);
        __syncthreads();
      }
      if (joint && pass >= L) {
        bool any = false;
        for (int k = 0; k < T; ++k) any = any || s.lab[k] == lp;
        if (!any) continue;                                      // (the same in every thread)
      }
      for (int e = tid; e < nA; e += kSmkThreads) s.A[e] = Ag[(size_t)e * Lx + lp];
      __syncthreads();
      // U = V . A (T x D mr), then T_s = U_s . R_s (D x mr) per row
      {
        double *U = s.U, *Tt = s.T;
        mm_lds(1, T, Dm, ml, s.V, 0, m, 1, s.A, 0, Dm, 1, [&](int, int r, int j, double v) { U[r * Dm + j] = v; });
        __syncthreads();
        mm_lds(T, D, mr, mr, s.U, Dm, mr, 1, s.R, m2, mr, 1, [&](int r, int d, int j, double v) { Tt[r * Dm + d * mr + j] = v; });
        __syncthreads();
      }
#pragma unroll
      for (int h = 0; h < kSmkPerWave; ++h) {
        const int smp = wave + h * kSmkWaves;
        if (st[h].sample < 0) continue;                          // (the same in every lane of the wave)
        if (joint && pass < L) {
          // P(l') = sum_{d,d'} S_s[d][d'] Q[d][d'],  Q[d][d'] = sum_c T[d][c] U[d'][c]
          if (lane == 0) {
            double a = 0.0;
            for (int e = 0; e < D * D; ++e) {
              const double *t = s.T + (size_t)(smp * D + e / D) * mr, *u = s.U + (size_t)(smp * D + e % D) * mr;
              double v = 0.0;
              for (int c = 0; c < mr; ++c) v = fma(t[c], u[c], v);
              a = fma(s.S[smp * D * D + e], v, a);
            }
            s.P[smp * L + lp] = a;
          }
        } else if (!joint || st[h].label == lp) {
          smk_pixel(p, s, st[h], smp, lane, i, m, mr);
        }
      }
      __syncthreads();
    }
  }
#pragma unroll
  for (int h = 0; h < kSmkPerWave; ++h)
    if (st[h].sample >= 0 && lane == 0) {
      p.labels[st[h].sample] = st[h].label;
      p.logp0[st[h].sample] = st[h].logp0;
    }
}

static bool smk_geometry(const SampleMaskedParams &p) {
  return p.N >= 2 && p.D >= 2 && p.D <= kMaxD && p.L >= 1 && p.l_pos >= 0 && p.l_pos < p.N && p.K >= 2 && p.K <= kSmpMaxK && p.n >= 1 &&
         p.n_tiles >= 1 && (p.mask_rows == 1 || p.mask_rows == p.n) &&
         (p.T == 1 || p.T == 2 || p.T == 4 || p.T == 8 || p.T == kSmkMaxTile);
}

int sample_masked_tile(int mb, int D, int L, int K) {
  for (int T = kSmkMaxTile; T >= 1; T >>= 1)
    if (sample_masked_env_lds_bytes(mb, D, T) <= 160 * 1024 && sample_masked_walk_lds_bytes(mb, D, L, K, T) <= 160 * 1024) return T;
  return 0;
}

bool launch_sample_masked(const SampleMaskedParams &p, int mb, bool walk, hipStream_t st) {
  if (!smk_geometry(p) || mb < 1 || mb > kSmpMaxBond) return false;
  const size_t le = sample_masked_env_lds_bytes(mb, p.D, p.T), lw = sample_masked_walk_lds_bytes(mb, p.D, p.L, p.K, p.T);
  if (le > 160 * 1024 || lw > 160 * 1024 || p.env_stride < (size_t)mb * mb) return false;
  SampleMaskedParams q = p;
  q.lds_m = mb;
  hipLaunchKernelGGL(sample_env_masked_kernel, dim3(q.n_tiles), dim3(kSmkThreads), le, st, q);
  if (walk) hipLaunchKernelGGL(sample_walk_masked_kernel, dim3(q.n_tiles), dim3(kSmkThreads), lw, st, q);
  return true;
}

}  // namespace tnml
