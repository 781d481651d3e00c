// The gradient of log p(known pixels [, class]) over all cores, every sample with its own mask and its own optional label
// (tnml_nll_masked_grad / tnml_nll_masked_step).  float64 throughout, no float atomic, every sum in a fixed
// order, no waiting between workgroups: two launches a chunk and one reduction.  Rows, tiles, class slots, the mask and the per-row
// stack of right environments R_{s,i} are those of kernels_sample_masked.hip, whose sample_env_masked_kernel is the first launch,
// exactly as it is.  Then
//   masked_grad_kernel         one workgroup per tile walks 0 .. N-1 once with the rows' LEFT environments Lf_s in LDS (Lf_{s,0} = 1),
//                              in the mould of site_cond_kernel.  Per site it stages the rows' R_{s,i+1} from the stack and makes two
//                              passes over the label slices and, per slice (A_i staged once for the tile, float32 as stored), over
//                              the core kNmgRows rows a at a time, on the f64 matrix cores (mm_lds):
//                                pass 1   1  X_s[a][d][c']  = sum_a' Lf_s[a][a'] A[a'][d][c']                  (ra x ml)(ml x D mr)
//                                         2  X_s[a][d][c'] <- sum_d' S_{s,i}[d][d'] X_s[a][d'][c']            the row's own metric
//                                         3  Lf'_s[c][c'] (+)= sum_{a,d} X_s[a][d][c] A[a][d][c']              (mr x ra D)(ra D x mr)
//                                then one wave per row: n_s = sum Lf'_s[c][c'] R_s[c][c'], the per-site normaliser, which carries the
//                                same powers of two as the products below, so that no exponent is needed;
//                                pass 2   1, 2 again, X_s times w_s / n_s (w_s the row's weight: 2 / n, -2, or exactly 0)
//                                         4  P[(a,d)][c] = sum_{s,c'} X_s[(a,d)][c'] R_s[c'][c]                (ra D x T mr)(T mr x mr)
//                                the rows stacked along k, so that the sum over the samples of a tile runs inside the MFMA k-loop;
//                                P goes to the tile's slot of the partial buffer.  Then Lf' times its power of two back into LDS.
//   masked_grad_reduce_kernel  one thread per core element adds the chunk's partials to a float64 accumulator in ascending tile
//                              order; after the last chunk the one cast to float32.
// The second pass is the price of forming n_s here: the environment kernel keeps the sum of its exponents, not one per site, and is
// not touched.  A result depends on T (which rows share a k-loop) and on nothing else of the launch geometry.
// Status word: bit 1 a non-finite left environment, bit 2 a normaliser that is not positive and finite, bit 4 an element beyond float32.
#include "small_gemm_device.h"
#include "sample_device.h"

#include <cfloat>
#include <cmath>

namespace tnml {

constexpr int kNmgThreads = 512;
constexpr int kNmgWaves = kNmgThreads / 64;
constexpr int kNmgReduceThreads = 256;

static inline size_t nmg_ra(int mb) { return (size_t)(mb < kNmgRows ? mb : kNmgRows); }

size_t masked_grad_lds_bytes(int mb, int D, int K, int T) {
  const size_t m = (size_t)mb, t = (size_t)T, d = (size_t)D;
  return (2 * t * m * m + nmg_ra(mb) * d * t * m + t * d * d + d * d + (size_t)K * (d + 1) + 2 * t) * sizeof(double) + smp_even(t) * sizeof(int) +
         smp_even(m * d * m) * sizeof(float);
}

// R_{s,i} of row `row` of the launch (the environment kernel's slot)
__device__ inline const double *nmg_env(const SampleMaskedParams &p, int row, int i) {
  return p.stack + ((size_t)row * (p.N + 1) + i) * p.env_stride;
}
// the known level of sample smp on site i, -1 where the site is free (rows without a sample have the empty mask)
__device__ inline int nmg_known(const SampleMaskedParams &p, int smp, int i) {
  if (smp < 0 || !p.mask[(size_t)(p.mask_rows == 1 ? 0 : smp) * p.N + i]) return -1;
  return p.known[(size_t)smp * p.N + i];
}

__device__ inline double nmg_wave_sum(double v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ __launch_bounds__(kNmgThreads) void masked_grad_kernel(MaskedGradParams gp) {
  extern __shared__ __attribute__((aligned(16))) double nmg_sh[];
  const SampleMaskedParams &p = gp.m;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, tile = blockIdx.x;
  const int N = p.N, D = p.D, DD = D * D, K = p.K, T = p.T, l = p.l_pos, m = p.lds_m;
  const int rmax = m < kNmgRows ? m : kNmgRows;
  double *Lf = nmg_sh;                                            // [T][ml][ml]
  double *Rr = Lf + (size_t)T * m * m;                            // [T][mr][mr]: the rows' R_{i+1}, [(s, c')][c] for product 4
  double *X = Rr + (size_t)T * m * m;                             // [rmax][D][T][mr]
  double *Ss = X + (size_t)rmax * D * T * m;                      // [T][D][D]: the rows' metric of the site
  double *Sg = Ss + T * DD;                                       // [D][D]
  double *phi = Sg + DD;                                          // [K][D]
  double *w = phi + (size_t)K * D;                                // [K]
  double *wr = w + K;                                             // [T] the rows' weights
  double *scl = wr + T;                                           // [T] w_s / n_s of the site
  int *srow = (int *)(scl + T);                                   // [T]
  float *A = (float *)(srow + smp_even((size_t)T));               // [ml][D][mr]
  double *part = gp.part + (size_t)tile * gp.total;
  const int q = p.tile_class[tile];
  for (int e = tid; e < K * D; e += kNmgThreads) phi[e] = p.phi[e];
  for (int e = tid; e < K; e += kNmgThreads) w[e] = p.w[e];
  for (int e = tid; e < DD; e += kNmgThreads) Sg[e] = p.S[e];
  for (int s = tid; s < T; s += kNmgThreads) {
    Lf[s] = 1.0;                                                  // Lf_{s,0} is 1 x 1
    srow[s] = p.tile_rows[tile * T + s];
    wr[s] = gp.wrow[tile * T + s];
    scl[s] = 0.0;
  }
  __syncthreads();
  for (int i = 0; i < N; ++i) {
    const int ml = smp_ml(p.bond, i), mr = smp_mr(p.bond, N, i), Dm = D * mr, m2r = mr * mr, Tm = T * mr;
    const bool lab = i == l;
    const int Lx = lab ? p.L : 1, l0 = lab && q >= 0 ? q : 0, l1 = lab && q < 0 ? p.L : l0 + 1;
    const float *Ag = lab ? p.lab : p.cores + (size_t)i * p.core_stride;
    double *Pi = part + gp.off[i];                                // the site's part of the tile's partial gradient
    for (int e = tid; e < T * m2r; e += kNmgThreads) {
      const int r = e / m2r;
      Rr[e] = nmg_env(p, tile * T + r, i + 1)[e - r * m2r];
    }
    for (int e = tid; e < T * DD; e += kNmgThreads) {
      const int s = e / DD, r = e - s * DD, d = r / D, dd = r - d * D;
      const int k = nmg_known(p, srow[s], i);
      Ss[e] = k < 0 ? Sg[r] : w[k] * (phi[(size_t)k * D + d] * phi[(size_t)k * D + dd]);
    }
    if (lab && q >= 0)                                            // (a given class touches its own slice of the label core alone)
      for (int e = tid; e < ml * Dm * Lx; e += kNmgThreads)
        if (e % Lx != q) Pi[e] = 0.0;
    bool first = true;
    for (int pass = 0; pass < 2; ++pass) {
      for (int lp = l0; lp < l1; ++lp) {
        __syncthreads();                                          // (the previous slice's last product has read A)
        for (int e = tid; e < ml * Dm; e += kNmgThreads) A[e] = Ag[(size_t)e * Lx + lp];
        __syncthreads();
        for (int a0 = 0; a0 < ml; a0 += rmax) {
          const int ra = min(rmax, ml - a0);
          const float *Ac = A + (size_t)a0 * Dm;
          // 1  X_s = Lf_s[a0 ..] . A
          mm_lds(T, ra, Dm, ml, Lf + (size_t)a0 * ml, ml * ml, ml, 1, A, 0, Dm, 1, [&](int s, int ar, int j, double v) {
            const int d = j / mr;
            X[((size_t)(ar * D + d) * T + s) * mr + (j - d * mr)] = v;
          });
          __syncthreads();
          // 2  the row's metric over d, in place, and in pass 2 the row's weight over its normaliser: one thread per (s, a, c')
          for (int e = tid; e < T * ra * mr; e += kNmgThreads) {
            const int c = e % mr, sa = e / mr, s = sa / ra, ar = sa - s * ra;
            double *t = X + ((size_t)ar * D * T + s) * mr + c;
            const double *sm = Ss + s * DD;
            const double sc = scl[s];
            double in[kMaxD], out[kMaxD];
#pragma unroll
            for (int d = 0; d < kMaxD; ++d)
              if (d < D) in[d] = t[(size_t)d * Tm];
#pragma unroll
            for (int d = 0; d < kMaxD; ++d)
              if (d < D) {
                double v = 0.0;
#pragma unroll
                for (int dd = 0; dd < kMaxD; ++dd)
                  if (dd < D) v = fma(sm[d * D + dd], in[dd], v);
                out[d] = pass == 0 ? v : (sc == 0.0 ? 0.0 : v * sc);
              }
#pragma unroll
            for (int d = 0; d < kMaxD; ++d)
              if (d < D) t[(size_t)d * Tm] = out[d];
          }
          __syncthreads();
          if (pass == 0) {
            // 3  Lf'_s[c][c'] (+)= sum_x X_s[x][c] A[a0 ..][x][c'],  x = (a, d), into the row's slot of lf_next
            const bool fresh = first;
            mm_lds(T, mr, mr, ra * D, X, mr, 1, Tm, Ac, 0, mr, 1, [&](int s, int c, int cp, double v) {
              double *out = gp.lf_next + (size_t)(tile * T + s) * p.env_stride + c * mr + cp;
              *out = fresh ? v : *out + v;
            });
            first = false;
          } else {
            // 4  P[x][c] = sum_{(s, c')} X[x][(s, c')] Rr[(s, c')][c] into the tile's partial gradient
            mm_lds(1, ra * D, mr, Tm, X, 0, Tm, 1, Rr, 0, mr, 1,
                   [&](int, int x, int c, double v) { Pi[((size_t)(a0 * D + x) * mr + c) * Lx + lp] = v; });
          }
          __syncthreads();
        }
      }
      if (pass == 0) {
        // per row: n_s = <Lf'_s, R_s>, lanes over the elements in turn, then the lanes in a fixed tree
        for (int s = wave; s < T; s += kNmgWaves) {
          const double *nx = gp.lf_next + (size_t)(tile * T + s) * p.env_stride;
          double v = 0.0;
          for (int e = lane; e < m2r; e += 64) v = fma(nx[e], Rr[(size_t)s * m2r + e], v);
          v = nmg_wave_sum(v);
          if (lane == 0) {
            const double ws = wr[s];
            const bool ok = v > 0.0 && v <= kSmpDblMax;
            scl[s] = ws != 0.0 && ok ? ws / v : 0.0;
            if (ws != 0.0 && !ok) atomicOr(gp.status, 2);
          }
        }
      }
    }
    // per row: Lf' times its power of two into LDS for the next site (the exponent is discarded: n_s is formed per site)
    for (int s = wave; s < T; s += kNmgWaves) {
      const double *nx = gp.lf_next + (size_t)(tile * T + s) * p.env_stride;
      double mx = 0.0;
      for (int e = lane; e < m2r; e += 64) {
        const double a = fabs(nx[e]);
        mx = fmax(mx, a <= kSmpDblMax ? a : INFINITY);            // (a NaN fails the comparison)
      }
      for (int o = 32; o > 0; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o, 64));
      int kexp = 0;
      if (!(mx <= kSmpDblMax)) { if (lane == 0) atomicOr(gp.status, 1); }
      else if (mx > 0.0) kexp = ilogb(mx) + 1;
      for (int e = lane; e < m2r; e += 64) Lf[(size_t)s * m2r + e] = ldexp(nx[e], -kexp);
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(kNmgReduceThreads) void masked_grad_reduce_kernel(MaskedGradReduceParams p) {
  const size_t e = (size_t)blockIdx.x * kNmgReduceThreads + threadIdx.x;
  if (e >= p.total) return;
  double a = p.first ? 0.0 : p.acc[e];
  for (int t = 0; t < p.n_tiles; ++t) a += p.part[(size_t)t * p.total + e];
  p.acc[e] = a;
  if (p.last) {
    if (!(fabs(a) <= (double)FLT_MAX)) atomicOr(p.status, 4);
    p.G[e] = (float)a;
  }
}

static bool nmg_geometry(const MaskedGradParams &p) {
  return p.off && p.wrow && p.lf_next && p.part && p.status && p.total >= 1 && p.m.T >= 1 && p.m.T <= kSmkMaxTile;
}

int masked_grad_tile(int mb, int D, int L, int K) {
  if (mb < 1 || mb > kNmgMaxBond) return 0;
  for (int T = sample_masked_tile(mb, D, L, K); T >= 1; T >>= 1)
    if (masked_grad_lds_bytes(mb, D, K, T) <= 160 * 1024) return T;
  return 0;
}

bool launch_masked_grad(const MaskedGradParams &p, int mb, hipStream_t st) {
  if (!nmg_geometry(p) || mb < 1 || mb > kNmgMaxBond) return false;
  const size_t lds = masked_grad_lds_bytes(mb, p.m.D, p.m.K, p.m.T);
  if (lds > 160 * 1024 || p.m.env_stride < (size_t)mb * mb) return false;
  if (!launch_sample_masked(p.m, mb, false, st)) return false;
  MaskedGradParams q = p;
  q.m.lds_m = mb;
  hipLaunchKernelGGL(masked_grad_kernel, dim3(q.m.n_tiles), dim3(kNmgThreads), lds, st, q);
  return true;
}

bool launch_masked_grad_reduce(const MaskedGradReduceParams &p, hipStream_t st) {
  if (!p.part || !p.acc || !p.G || !p.status || p.total < 1 || p.n_tiles < 1) return false;
  const size_t blocks = (p.total + kNmgReduceThreads - 1) / kNmgReduceThreads;
  if (blocks > (size_t)INT_MAX) return false;
  hipLaunchKernelGGL(masked_grad_reduce_kernel, dim3((unsigned)blocks), dim3(kNmgReduceThreads), 0, st, p);
  return true;
}

}  // namespace tnml
