// Per-pixel conditionals given any set of known pixels (tnml_site_conditionals).  float64 throughout, no float
// atomic, every sum in a fixed order, no waiting between workgroups: two launches a chunk.  Rows, tiles, class slots, the mask and the
// per-row stack of right environments R_{s,i} are those of kernels_sample_masked.hip, whose sample_env_masked_kernel is the first
// launch, exactly as it is.  The second is
//   site_cond_kernel   one workgroup per tile walks 0 .. N-1 once with the rows' LEFT environments Lf_s in LDS (Lf_{s,0} = 1).  Per
//                      site it stages the rows' R_{s,i+1} from the stack and, per label slice, A_i (float32 as stored) once for the
//                      tile; then, kSccRows rows a' of the core at a time, on the f64 matrix cores (mm_lds, batched over the rows s)
//                        1  T2_s[a'][d][c]  = sum_a Lf_s[a'][a] A[a][d][c]                      (ra x ml)(ml x D mr)
//                        2  T1_s[a'][d][c'] = sum_c A[a'][d][c] R_s[c][c']                      (ra D x mr)(mr x mr)
//                        3  Q_s[d][d']     += sum_{a',c} T2_s[a'][d][c] T1_s[a'][d'][c]         one wave per row, lanes over c
//                        4  T2_s[a'][d][c] <- sum_d' S_{s,i}[d][d'] T2_s[a'][d'][c]             the row's own metric, elementwise
//                        5  Lf'_s[c][c']  (+)= sum_{a',d} T2_s[a'][d][c] A[a'][d][c']            (mr x ra D)(ra D x mr)
//                      so that T1 and T2 are never whole in LDS; Lf' accumulates in the row's slot of lf_next (chunks and label
//                      slices one after the other, as the environment kernel adds its slices).  Then one wave per row: Lf' times
//                      its power of two back into LDS (the exponent is discarded: everything below is normalised per site), and
//                      from Q_s the K densities max(0, w_k phi_k^T Q phi_k) / tr(S Q), four consecutive levels a lane, reduced to
//                      mean, variance, entropy, the log density of the known level and the first level of largest density.
// Each row's arithmetic touches only its own rows of every operand and the chunk of kSccRows does not depend on T, so a result
// depends neither on T nor on the rows that share the tile.  Status word: bit 1 a non-finite environment or density.
#include "small_gemm_device.h"
#include "sample_device.h"

#include <cmath>

namespace tnml {

constexpr int kSccThreads = 512;
constexpr int kSccWaves = kSccThreads / 64;

static inline size_t scc_ra(int mb) { return (size_t)(mb < kSccRows ? mb : kSccRows); }

size_t site_cond_lds_bytes(int mb, int D, int K, int T) {
  const size_t m = (size_t)mb, t = (size_t)T, d = (size_t)D;
  return (2 * t * m * m + 2 * t * scc_ra(mb) * d * m + 2 * t * d * d + d * d + (size_t)K * (d + 2)) * sizeof(double) + smp_even(t) * sizeof(int) +
         smp_even(m * d * m) * sizeof(float);
}

// R_{s,i} of row `row` of the launch (the environment kernel's slot)
__device__ inline const double *scc_env(const SampleMaskedParams &p, int row, int i) {
  return p.stack + ((size_t)row * (p.N + 1) + i) * p.env_stride;
}
// the known level of sample smp on site i, -1 where the site is free (rows without a sample have the empty mask)
__device__ inline int scc_known(const SampleMaskedParams &p, int smp, int i) {
  if (smp < 0 || !p.mask[(size_t)(p.mask_rows == 1 ? 0 : smp) * p.N + i]) return -1;
  return p.known[(size_t)smp * p.N + i];
}

__device__ inline double scc_wave_sum(double v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// The statistics of site i of sample smp from the row's Q [D][D]; called by one whole wave.  phi, w, val, Sg: the tables in LDS.
__device__ inline void scc_statistics(const SiteCondParams &sp, const double *Q, const double *phi, const double *w, const double *val,
                                      const double *Sg, int smp, int i, int lane) {
  const SampleMaskedParams &p = sp.m;
  const int D = p.D, DD = D * D, K = p.K;
  double tr = 0.0;
  for (int e = 0; e < DD; ++e) tr = fma(Sg[e], Q[e], tr);
  const size_t at = (size_t)smp * p.N + i;
  if (sp.q && lane < DD) sp.q[at * DD + lane] = Q[lane] / tr;
  if (!sp.stats && !sp.mode) return;
  double pl[4], vl[4];
  bool nonfinite = !(fabs(tr) <= kSmpDblMax);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int k = 4 * lane + j;
    double v = 0.0;
    vl[j] = 0.0;
    if (k < K) {
      const double *ph = phi + (size_t)k * D;
      double a = 0.0;
      for (int d = 0; d < D; ++d) {
        double t = 0.0;
        for (int dd = 0; dd < D; ++dd) t = fma(Q[d * D + dd], ph[dd], t);
        a = fma(ph[d], t, a);
      }
      v = w[k] * a;
      if (!(fabs(v) <= kSmpDblMax)) { nonfinite = true; v = 0.0; }
      v = v > 0.0 ? v / tr : 0.0;
      vl[j] = val[k];
    }
    pl[j] = v;
  }
  if (nonfinite && lane == 0) atomicOr(p.status, 1);
  const double mean = scc_wave_sum(((pl[0] * vl[0] + pl[1] * vl[1]) + pl[2] * vl[2]) + pl[3] * vl[3]);
  double var = 0.0, ent = 0.0;
  int best = 4 * lane;
  double pbest = pl[0];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const double dv = vl[j] - mean;
    var += pl[j] * (dv * dv);
    if (pl[j] > 0.0) ent -= pl[j] * log(pl[j]);
    if (pl[j] > pbest) { pbest = pl[j]; best = 4 * lane + j; }
  }
  var = scc_wave_sum(var);
  ent = scc_wave_sum(ent);
  for (int o = 32; o > 0; o >>= 1) {                             // the first level of largest density
    const double po = __shfl_xor(pbest, o, 64);
    const int bo = __shfl_xor(best, o, 64);
    if (po > pbest || (po == pbest && bo < best)) { pbest = po; best = bo; }
  }
  const int kn = scc_known(p, smp, i);
  double lk = 0.0;
  if (kn >= 0) {
    const int j = kn & 3;
    const double mine = j == 0 ? pl[0] : j == 1 ? pl[1] : j == 2 ? pl[2] : pl[3];
    lk = log(__shfl(mine, kn >> 2, 64));
  }
  if (lane == 0) {
    if (sp.stats) {
      double *o = sp.stats + at * 4;
      o[0] = mean; o[1] = var; o[2] = ent; o[3] = lk;
    }
    if (sp.mode) sp.mode[at] = best;
  }
}

__global__ __launch_bounds__(kSccThreads) void site_cond_kernel(SiteCondParams sp) {
  extern __shared__ __attribute__((aligned(16))) double scc_sh[];
  const SampleMaskedParams &p = sp.m;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, tile = blockIdx.x;
  const int N = p.N, D = p.D, DD = D * D, K = p.K, T = p.T, l = p.l_pos, m = p.lds_m;
  const int rmax = m < kSccRows ? m : kSccRows;
  double *Lf = scc_sh;                                            // [T][ml][ml]
  double *Rr = Lf + (size_t)T * m * m;                            // [T][mr][mr]: the rows' R_{i+1}
  double *T2 = Rr + (size_t)T * m * m;                            // [T][rmax][D][mr]
  double *T1 = T2 + (size_t)T * rmax * D * m;                     // [T][rmax][D][mr]
  double *Qs = T1 + (size_t)T * rmax * D * m;                     // [T][D][D]
  double *Ss = Qs + T * DD;                                       // [T][D][D]: the rows' metric of the site
  double *Sg = Ss + T * DD;                                       // [D][D]
  double *phi = Sg + DD;                                          // [K][D]
  double *w = phi + (size_t)K * D;                                // [K]
  double *val = w + K;                                            // [K]
  int *srow = (int *)(val + K);                                   // [T]
  float *A = (float *)(srow + smp_even((size_t)T));               // [ml][D][mr]
  const int q = p.tile_class[tile];
  for (int e = tid; e < K * D; e += kSccThreads) phi[e] = p.phi[e];
  for (int e = tid; e < K; e += kSccThreads) { w[e] = p.w[e]; val[e] = sp.values[e]; }
  for (int e = tid; e < DD; e += kSccThreads) Sg[e] = p.S[e];
  for (int s = tid; s < T; s += kSccThreads) {
    Lf[s] = 1.0;                                                  // Lf_{s,0} is 1 x 1
    srow[s] = p.tile_rows[tile * T + s];
  }
  __syncthreads();
  for (int i = 0; i < N; ++i) {
    const int ml = smp_ml(p.bond, i), mr = smp_mr(p.bond, N, i), Dm = D * mr, m2r = mr * mr;
    const bool lab = i == l;
    const int Lx = lab ? p.L : 1, l0 = lab && q >= 0 ? q : 0, l1 = lab && q < 0 ? p.L : l0 + 1;
    const float *Ag = lab ? p.lab : p.cores + (size_t)i * p.core_stride;
    for (int e = tid; e < T * m2r; e += kSccThreads) {
      const int r = e / m2r;
      Rr[e] = scc_env(p, tile * T + r, i + 1)[e - r * m2r];
    }
    for (int e = tid; e < T * DD; e += kSccThreads) {
      const int s = e / DD, r = e - s * DD, d = r / D, dd = r - d * D;
      const int k = scc_known(p, srow[s], i);
      Ss[e] = k < 0 ? Sg[r] : w[k] * (phi[(size_t)k * D + d] * phi[(size_t)k * D + dd]);
      Qs[e] = 0.0;
    }
    bool first = true;
    for (int lp = l0; lp < l1; ++lp) {
      __syncthreads();                                            // (the previous slice's last product has read A)
      for (int e = tid; e < ml * Dm; e += kSccThreads) A[e] = Ag[(size_t)e * Lx + lp];
      __syncthreads();
      for (int a0 = 0; a0 < ml; a0 += rmax) {
        const int ra = min(rmax, ml - a0);
        const float *Ac = A + (size_t)a0 * Dm;
        // 1, 2  T2_s = Lf_s[a0 ..] . A and T1_s = A[a0 ..] . R_s: independent, back to back
        const int slot = mm_lds(T, ra, Dm, ml, Lf + (size_t)a0 * ml, ml * ml, ml, 1, A, 0, Dm, 1,
                                [&](int s, int ar, int j, double v) { T2[(size_t)(s * rmax + ar) * Dm + j] = v; });
        mm_lds(T, ra * D, mr, mr, Ac, 0, mr, 1, Rr, m2r, mr, 1,
               [&](int s, int ad, int cp, double v) { T1[(size_t)(s * rmax * D + ad) * mr + cp] = v; }, false, slot);
        __syncthreads();
        // 3  Q_s += T2_s . T1_s^T over (a', c): one wave per row, lane c, a' in turn, then the lanes in a fixed tree
        for (int s = wave; s < T; s += kSccWaves)
          for (int e = 0; e < DD; ++e) {
            const int d = e / D, dd = e - d * D;
            double v = 0.0;
            if (lane < mr)
              for (int ar = 0; ar < ra; ++ar)
                v = fma(T2[(size_t)((s * rmax + ar) * D + d) * mr + lane], T1[(size_t)((s * rmax + ar) * D + dd) * mr + lane], v);
            v = scc_wave_sum(v);
            if (lane == 0) Qs[s * DD + e] += v;
          }
        __syncthreads();
        // 4  the row's metric over d, in place: one thread per (s, a', c)
        for (int e = tid; e < T * ra * mr; e += kSccThreads) {
          const int c = e % mr, sa = e / mr, s = sa / ra, ar = sa - s * ra;
          double *t = T2 + (size_t)(s * rmax + ar) * Dm + c;
          const double *sm = Ss + s * DD;
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
        // 5  Lf'_s[c][c'] (+)= sum_x T2_s[x][c] A[a0 ..][x][c'],  x = (a', d), into the row's slot of lf_next
        const bool fresh = first;
        mm_lds(T, mr, mr, ra * D, T2, rmax * Dm, 1, mr, Ac, 0, mr, 1, [&](int s, int c, int cp, double v) {
          double *out = sp.lf_next + (size_t)(tile * T + s) * p.env_stride + c * mr + cp;
          *out = fresh ? v : *out + v;
        });
        first = false;
        __syncthreads();
      }
    }
    // per row: Lf' times its power of two into LDS for the next site; the statistics of this one
    for (int s = wave; s < T; s += kSccWaves) {
      const double *nx = sp.lf_next + (size_t)(tile * T + s) * p.env_stride;
      double mx = 0.0;
      for (int e = lane; e < m2r; e += 64) {
        const double a = fabs(nx[e]);
        mx = fmax(mx, a <= kSmpDblMax ? a : INFINITY);            // (a NaN fails the comparison)
      }
      for (int o = 32; o > 0; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o, 64));
      int kexp = 0;
      if (!(mx <= kSmpDblMax)) { if (lane == 0) atomicOr(p.status, 1); }
      else if (mx > 0.0) kexp = ilogb(mx) + 1;
      for (int e = lane; e < m2r; e += 64) Lf[(size_t)s * m2r + e] = ldexp(nx[e], -kexp);
      if (srow[s] >= 0) scc_statistics(sp, Qs + s * DD, phi, w, val, Sg, srow[s], i, lane);
    }
    __syncthreads();
  }
}

static bool scc_geometry(const SiteCondParams &p) {
  return p.values && p.lf_next && (p.q || p.stats || p.mode) && p.m.T >= 1 && p.m.T <= kSmkMaxTile;
}

int site_cond_tile(int mb, int D, int L, int K) {
  if (mb < 1 || mb > kSccMaxBond) return 0;
  for (int T = sample_masked_tile(mb, D, L, K); T >= 1; T >>= 1)
    if (site_cond_lds_bytes(mb, D, K, T) <= 160 * 1024) return T;
  return 0;
}

bool launch_site_cond(const SiteCondParams &p, int mb, hipStream_t st) {
  if (!scc_geometry(p) || mb < 1 || mb > kSccMaxBond) return false;
  const size_t lds = site_cond_lds_bytes(mb, p.m.D, p.m.K, p.m.T);
  if (lds > 160 * 1024 || p.m.env_stride < (size_t)mb * mb) return false;
  if (!launch_sample_masked(p.m, mb, false, st)) return false;
  SiteCondParams q = p;
  q.m.lds_m = mb;
  hipLaunchKernelGGL(site_cond_kernel, dim3(q.m.n_tiles), dim3(kSccThreads), lds, st, q);
  return true;
}

}  // namespace tnml
