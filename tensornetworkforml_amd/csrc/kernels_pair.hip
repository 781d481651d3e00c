// Pixel-pair marginals (tnml_pair_marginals).  float64 throughout, float32 cores read as stored, no float
// atomic, every sum in a fixed order, no waiting between workgroups: the hand-overs are launch boundaries.  The shared metric
// environments L_i, R_i come from lognorm_env_kernel (kernels_nll.hip) with the grid's metric S and the call's class slot.  Then
//   pair_close_kernel   one workgroup per site j.  R_{j+1} in LDS; per label slice T[(a,e)][c'] = sum_c A[a][e][c] R[c][c'] and
//                       B[(a,e)][(a',e')] (+)= sum_c' T[(a,e)][c'] A[a'][e'][c'] on the f64 matrix cores, B stored as [e,e'][a,a'].
//                       Then q1raw[e,e'] = sum L_j[a,a'] B[e,e'][a,a'] (one wave per (e,e'), lanes over (a,a'), a fixed tree), and by
//                       wave 0 q1 = q1raw / tr(S q1raw) and the mean, variance and entropy of max(0, w_k phi_k^T q1 phi_k).
//   pair_walk_kernel    grid (rows of a chunk, D^2).  Workgroup (r, (d,d')) starts from E = L_i, i = rows[r], and walks j = i .. N-2
//                       with the body of lognorm_env_kernel's left walk, E kept in the order [c][c'] of the formula:
//                         1  T[a][(e',c')] = sum_a' E[a][a'] A_j[a'][e'][c']
//                         2  T[a][e][c']  <- sum_e' M[e][e'] T[a][e'][c'],   M = the unit matrix of (d,d') on site i, S behind it
//                         3  E'[c][c']   += sum_(a,e) A_j[a][e][c] T[a][e][c']
//                       so that after site i E is C_i,i+1[d,d'].  E' times an exact 2^-k into E, k added to the running exponent; then
//                       the D^2 products sum_x E[x] B_{j+1}[e,e'][x] (one wave per (e,e'), B streamed from memory) into
//                       Q[r][j+1][(d,d')][(e,e')] unnormalised, the running exponent into qexp[r][j+1][(d,d')].
//   pair_stats_kernel   grid (N, rows of a chunk), one workgroup per pair (i, j).  j <= i: zeros.  Otherwise the D^2 blocks of Q to
//                       the largest exponent of a block that is not zero, q = Q / sum S (x) S Q in place, G[k][(e,e')] = sum
//                       phi_k[d] phi_k[d'] q[(d,d')][(e,e')] in LDS, and thread k forms p(k,k') = max(0, w_k w_k' sum G[k][(e,e')]
//                       phi_k'[e] phi_k'[e']) for k' = 0 .. K-1 in turn: the row sums p_i(k), sum p val_k', sum p log p stay with
//                       the thread, the column sums p_j(k') go through the wave's shuffles into one LDS word per wave.  Covariance,
//                       correlation and I = sum p log p - sum p_i log p_i - sum p_j log p_j from fixed trees.
// A workgroup of the walk touches only its own row and (d,d'), and the deal of tiles to waves does not change any sum: a result depends
// neither on the other rows, nor on the chunk, nor on the number of threads of the walk.
#include "small_gemm_device.h"
#include "lognorm_device.h"

#include <climits>
#include <cmath>

namespace tnml {

constexpr int kPairWalkMaxThreads = 1024;
constexpr int kPairMaxWaves = kPairWalkMaxThreads / 64;

static inline size_t pr_even(size_t x) { return (x + 1) & ~(size_t)1; }

size_t pair_close_lds_bytes(int mb, int D, int K) {
  const size_t m = (size_t)mb, d = (size_t)D;
  return (m * m + m * d * m + 2 * d * d + (size_t)K * (d + 2)) * sizeof(double);
}
size_t pair_walk_lds_bytes(int mb, int D) {
  const size_t m = (size_t)mb, d = (size_t)D;
  return (2 * m * m + m * d * m + 2 * d * d + 2 * kPairMaxWaves) * sizeof(double);
}
size_t pair_stats_lds_bytes(int D, int K) {
  const size_t d = (size_t)D, k = (size_t)K, nw = kPairStatThreads / 64;
  return (k * d * d + k * (d + 2) + nw * k + 2 * d * d + nw * 8) * sizeof(double) + pr_even(d * d) * sizeof(int);
}
int pair_walk_threads(int mb) { return mb <= 32 ? 256 : kPairWalkMaxThreads; }

__device__ inline double pr_wave_sum(double v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// sum_x a[x] b[x], x = lane, lane + 64, ... in turn, then the lanes in a fixed tree: every lane gets the result
__device__ inline double pr_wave_dot(const double *a, const double *b, int n, int lane) {
  double v = 0.0;
  for (int x = lane; x < n; x += 64) v = fma(a[x], b[x], v);
  return pr_wave_sum(v);
}

// w_k phi_k^T Q phi_k for the D x D matrix Q
__device__ inline double pr_form(const double *Q, const double *ph, int D) {
  double a = 0.0;
  for (int d = 0; d < D; ++d) {
    double t = 0.0;
    for (int dd = 0; dd < D; ++dd) t = fma(Q[d * D + dd], ph[dd], t);
    a = fma(ph[d], t, a);
  }
  return a;
}

__global__ __launch_bounds__(kPairCloseThreads) void pair_close_kernel(PairParams pp) {
  extern __shared__ __attribute__((aligned(16))) double pr_sh[];
  const LogNormParams &p = pp.e;
  if (p.status[0]) return;                                         // (the environment launch's word: nothing here is worth forming)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = blockIdx.x;
  const int D = p.D, DD = D * D, K = pp.K;
  const size_t m = (size_t)p.lds_m;
  const int ml = lnz_ml(p, j), mr = lnz_mr(p, j), mlD = ml * D, m2l = ml * ml;
  double *R = pr_sh;                                               // [mr][mr]
  double *T = R + m * m;                                           // [ml][D][mr]
  double *q1s = T + m * D * m;                                     // [D][D]
  double *Sg = q1s + DD;                                           // [D][D]
  double *phi = Sg + DD;                                           // [K][D]
  double *w = phi + (size_t)K * D;                                 // [K]
  double *val = w + K;                                             // [K]
  const double *Rg = p.envR + (size_t)(j + 1) * p.env_stride;
  for (int e = tid; e < mr * mr; e += kPairCloseThreads) R[e] = Rg[e];
  for (int e = tid; e < K * D; e += kPairCloseThreads) phi[e] = pp.phi[e];
  for (int e = tid; e < K; e += kPairCloseThreads) { w[e] = pp.w[e]; val[e] = pp.values[e]; }
  for (int e = tid; e < DD; e += kPairCloseThreads) Sg[e] = p.metric[e];
  __syncthreads();
  const bool lab = j == p.l_pos;
  const int Lx = lab ? p.L : 1;
  const int l0 = lab && p.class_plus1 > 0 ? p.class_plus1 - 1 : 0, l1 = lab && p.class_plus1 > 0 ? l0 + 1 : Lx;
  const float *A = lab ? p.lab : p.cores + (size_t)j * p.core_stride;
  double *Bj = pp.B + (size_t)j * DD * p.env_stride;
  bool first = true;
  for (int lp = l0; lp < l1; ++lp) {
    const float *Al = A + lp;
    mm_lds(1, mlD, mr, mr, Al, 0, mr * Lx, Lx, R, 0, mr, 1, [&](int, int r, int c, double v) { T[r * mr + c] = v; });
    __syncthreads();
    const bool fresh = first;
    mm_lds(1, mlD, mlD, mr, T, 0, mr, 1, Al, 0, Lx, mr * Lx, [&](int, int r, int c, double v) {
      const int a = r / D, e = r - a * D, ap = c / D, ep = c - ap * D;
      double *out = Bj + (size_t)(e * D + ep) * p.env_stride + a * ml + ap;
      *out = fresh ? v : *out + v;
    });
    first = false;
    __syncthreads();
  }
  const double *Lj = p.envL + (size_t)j * p.env_stride;
  for (int ee = wave; ee < DD; ee += kPairCloseThreads / 64) {
    const double v = pr_wave_dot(Lj, Bj + (size_t)ee * p.env_stride, m2l, lane);
    if (lane == 0) q1s[ee] = v;
  }
  __syncthreads();
  if (wave != 0) return;
  double tr = 0.0;
  for (int e = 0; e < DD; ++e) tr = fma(Sg[e], q1s[e], tr);
  bool bad = !(fabs(tr) <= kLnzDblMax) || tr == 0.0;
  if (lane < DD) pp.q1[(size_t)j * DD + lane] = q1s[lane] / tr;
  double pl[4], vl[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int k = 4 * lane + u;
    double v = 0.0;
    vl[u] = 0.0;
    if (k < K) {
      v = w[k] * pr_form(q1s, phi + (size_t)k * D, D);
      if (!(fabs(v) <= kLnzDblMax)) { bad = true; v = 0.0; }
      v = v > 0.0 ? v / tr : 0.0;
      vl[u] = val[k];
    }
    pl[u] = v;
  }
  if (bad && lane == 0) atomicOr(p.status + 1, 1);
  const double mean = pr_wave_sum(((pl[0] * vl[0] + pl[1] * vl[1]) + pl[2] * vl[2]) + pl[3] * vl[3]);
  double var = 0.0, ent = 0.0;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const double dv = vl[u] - mean;
    var += pl[u] * (dv * dv);
    if (pl[u] > 0.0) ent -= pl[u] * log(pl[u]);
  }
  var = pr_wave_sum(var);
  ent = pr_wave_sum(ent);
  if (lane == 0) {
    double *o = pp.stats1 + (size_t)j * 3;
    o[0] = mean; o[1] = var; o[2] = ent;
  }
}

__device__ inline double pr_block_max(double x, double *red, int nw) {
  for (int o = 32; o > 0; o >>= 1) x = fmax(x, __shfl_xor(x, o, 64));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
  __syncthreads();
  double r = red[0];
  for (int w = 1; w < nw; ++w) r = fmax(r, red[w]);
  return r;
}

__global__ __launch_bounds__(kPairWalkMaxThreads) void pair_walk_kernel(PairParams pp) {
  extern __shared__ __attribute__((aligned(16))) double pr_sh[];
  const LogNormParams &p = pp.e;
  if (p.status[0]) return;
  const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63, wave = tid >> 6, nw = nt >> 6;
  const int N = p.N, D = p.D, DD = D * D;
  const int r = blockIdx.x, i = pp.rows[r], dd = blockIdx.y;
  if (i >= N - 1) return;                                          // (the last site has no pair to its right)
  const size_t m = (size_t)p.lds_m;
  double *E = pr_sh, *En = E + m * m, *T = En + m * m;             // [m][m], [m][m], [m][D][m]
  double *M0 = T + m * D * m, *Sg = M0 + DD, *red = Sg + DD;       // the metric of site i, the grid's, 2 x the waves' maxima
  {
    const int ml = lnz_ml(p, i);
    const double *Lg = p.envL + (size_t)i * p.env_stride;
    for (int e = tid; e < ml * ml; e += nt) E[e] = Lg[e];
    for (int e = tid; e < DD; e += nt) { M0[e] = e == dd ? 1.0 : 0.0; Sg[e] = p.metric[e]; }
  }
  int expo = 0;
  __syncthreads();
  for (int j = i; j < N - 1; ++j) {
    const int ml = lnz_ml(p, j), mr = lnz_mr(p, j), Dm = D * mr, m2r = mr * mr;
    const bool lab = j == p.l_pos;
    const int Lx = lab ? p.L : 1;
    const int l0 = lab && p.class_plus1 > 0 ? p.class_plus1 - 1 : 0, l1 = lab && p.class_plus1 > 0 ? l0 + 1 : Lx;
    const float *A = lab ? p.lab : p.cores + (size_t)j * p.core_stride;
    const double *Mj = j == i ? M0 : Sg;
    for (int e = tid; e < m2r; e += nt) En[e] = 0.0;               // (product 3 is behind two barriers)
    for (int lp = l0; lp < l1; ++lp) {
      const float *Al = A + lp;
      mm_lds(1, ml, Dm, ml, E, 0, ml, 1, Al, 0, Dm * Lx, Lx, [&](int, int a, int x, double v) { T[a * Dm + x] = v; });
      __syncthreads();
      lnz_fold_metric(T, Mj, ml, mr, D, nt);
      __syncthreads();
      mm_lds(1, mr, mr, ml * D, Al, 0, Lx, mr * Lx, T, 0, mr, 1, [&](int, int c, int cp, double v) { En[c * mr + cp] += v; });
      __syncthreads();
    }
    double mx = 0.0;
    for (int e = tid; e < m2r; e += nt) {
      const double a = fabs(En[e]);
      mx = fmax(mx, a <= kLnzDblMax ? a : INFINITY);               // (a NaN fails the comparison)
    }
    mx = pr_block_max(mx, red + ((j - i) & 1) * kPairMaxWaves, nw);
    if (!(mx <= kLnzDblMax)) {
      if (tid == 0) atomicOr(p.status + 1, 1);
      return;
    }
    const int kexp = mx > 0.0 ? ilogb(mx) + 1 : 0;
    expo += kexp;
    for (int e = tid; e < m2r; e += nt) E[e] = ldexp(En[e], -kexp);
    __syncthreads();
    const size_t at = (size_t)r * N + (j + 1);
    const double *Bn = pp.B + (size_t)(j + 1) * DD * p.env_stride;
    for (int ee = wave; ee < DD; ee += nw) {
      const double v = pr_wave_dot(E, Bn + (size_t)ee * p.env_stride, m2r, lane);
      if (lane == 0) pp.Q[(at * DD + dd) * DD + ee] = v;
    }
    if (tid == 0) pp.qexp[at * DD + dd] = expo;
  }
}

// the sums of n values per thread over the workgroup: the lanes in a fixed tree, then the waves in turn; every thread gets them
template <int n>
__device__ inline void pr_block_sums(double (&v)[n], double *red) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = kPairStatThreads / 64;
#pragma unroll
  for (int t = 0; t < n; ++t) v[t] = pr_wave_sum(v[t]);
  __syncthreads();                                                 // (red may still be read from the call before)
  if (lane == 0)
#pragma unroll
    for (int t = 0; t < n; ++t) red[wave * n + t] = v[t];
  __syncthreads();
#pragma unroll
  for (int t = 0; t < n; ++t) {
    double s = red[t];
    for (int u = 1; u < nw; ++u) s += red[u * n + t];
    v[t] = s;
  }
}

__global__ __launch_bounds__(kPairStatThreads) void pair_stats_kernel(PairParams pp) {
  extern __shared__ __attribute__((aligned(16))) double pr_sh[];
  const LogNormParams &p = pp.e;
  if (p.status[0]) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = kPairStatThreads / 64;
  const int N = p.N, D = p.D, DD = D * D, K = pp.K;
  const int j = blockIdx.x, r = blockIdx.y, i = pp.rows[r];
  const size_t at = (size_t)r * N + j;
  double *Q = pp.Q + at * DD * DD;
  double *so = pp.stats + at * 3;
  if (j <= i) {
    for (int e = tid; e < DD * DD; e += kPairStatThreads) Q[e] = 0.0;
    if (tid < 3) so[tid] = 0.0;
    return;
  }
  double *G = pr_sh;                                               // [D^2][K]
  double *phi = G + (size_t)K * DD;                                // [K][D]
  double *w = phi + (size_t)K * D;                                 // [K]
  double *val = w + K;                                             // [K]
  double *col = val + K;                                           // [waves][K]: the waves' parts of the column sums
  double *Sg = col + (size_t)nw * K;                               // [D][D]
  double *part = Sg + DD;                                          // [D^2]
  double *red = part + DD;                                         // [waves][8]
  int *bx = (int *)(red + nw * 8);                                 // [D^2]: a block's exponent, INT_MIN where it is zero
  for (int e = tid; e < K * D; e += kPairStatThreads) phi[e] = pp.phi[e];
  for (int e = tid; e < K; e += kPairStatThreads) { w[e] = pp.w[e]; val[e] = pp.values[e]; }
  for (int e = tid; e < DD; e += kPairStatThreads) Sg[e] = p.metric[e];
  if (tid < DD) {
    bool nz = false;
    for (int e = 0; e < DD; ++e) nz = nz || Q[tid * DD + e] != 0.0;
    bx[tid] = nz ? pp.qexp[at * DD + tid] : INT_MIN;
  }
  __syncthreads();
  int emax = INT_MIN;
  for (int e = 0; e < DD; ++e) emax = max(emax, bx[e]);
  if (tid < DD) {
    const int sh = bx[tid] == INT_MIN ? 0 : bx[tid] - emax;
    double s = 0.0;
    for (int e = 0; e < DD; ++e) s = fma(Sg[e], ldexp(Q[tid * DD + e], sh), s);
    part[tid] = s;
  }
  __syncthreads();
  double norm = 0.0;
  for (int e = 0; e < DD; ++e) norm = fma(Sg[e], part[e], norm);
  bool bad = !(fabs(norm) <= kLnzDblMax) || norm == 0.0;
  for (int e = tid; e < DD * DD; e += kPairStatThreads) {
    const int b = e / DD;
    Q[e] = ldexp(Q[e], bx[b] == INT_MIN ? 0 : bx[b] - emax) / norm;
  }
  __syncthreads();
  // G[(e,e')][k] = sum_(d,d') phi_k[d] phi_k[d'] q[(d,d')][(e,e')]
  if (tid < K) {
    const double *ph = phi + (size_t)tid * D;
    for (int ee = 0; ee < DD; ++ee) {
      double a = 0.0;
      for (int d = 0; d < D; ++d) {
        double t = 0.0;
        for (int dp = 0; dp < D; ++dp) t = fma(Q[(size_t)(d * D + dp) * DD + ee], ph[dp], t);
        a = fma(ph[d], t, a);
      }
      G[(size_t)ee * K + tid] = a;
    }
  }
  __syncthreads();
  const bool live = tid < K;
  const double wk = live ? w[tid] : 0.0;
  double pi = 0.0, rowv = 0.0, plp = 0.0;
  for (int kp = 0; kp < K; ++kp) {
    const double *ph = phi + (size_t)kp * D;
    double v = 0.0;
    if (live) {
      double a = 0.0;
      for (int e = 0; e < D; ++e) {
        double t = 0.0;
        for (int ep = 0; ep < D; ++ep) t = fma(G[(size_t)(e * D + ep) * K + tid], ph[ep], t);
        a = fma(ph[e], t, a);
      }
      v = (wk * w[kp]) * a;
      if (!(fabs(v) <= kLnzDblMax)) { bad = true; v = 0.0; }
      v = v > 0.0 ? v : 0.0;
    }
    pi += v;
    rowv = fma(v, val[kp], rowv);
    if (v > 0.0) plp = fma(v, log(v), plp);
    const double cs = pr_wave_sum(v);
    if (lane == 0) col[(size_t)wave * K + kp] = cs;
  }
  __syncthreads();
  double pj = 0.0;
  if (live)
    for (int u = 0; u < nw; ++u) pj += col[(size_t)u * K + tid];
  const double vk = live ? val[tid] : 0.0;
  double s[6] = {pi * vk, pj * vk, vk * rowv, plp, pi > 0.0 ? pi * log(pi) : 0.0, pj > 0.0 ? pj * log(pj) : 0.0};
  pr_block_sums(s, red);
  const double mi = s[0], mj = s[1];
  double v2[2] = {pi * ((vk - mi) * (vk - mi)), pj * ((vk - mj) * (vk - mj))};
  pr_block_sums(v2, red);
  if (bad) atomicOr(p.status + 1, 1);
  if (tid == 0) {
    const double cov = s[2] - mi * mj;
    so[0] = cov;
    so[1] = v2[0] > 0.0 && v2[1] > 0.0 ? cov / (sqrt(v2[0]) * sqrt(v2[1])) : 0.0;
    so[2] = (s[3] - s[4]) - s[5];
  }
}

static bool pr_geometry(const PairParams &p, int mb) {
  const LogNormParams &e = p.e;
  return e.N >= 2 && e.D >= 2 && e.D <= kMaxD && e.L >= 1 && e.l_pos >= 0 && e.l_pos < e.N && e.class_plus1 >= 0 && e.class_plus1 <= e.L &&
         e.metric_sites == 1 && e.metric && mb >= 1 && mb <= kPairMaxBond && e.env_stride >= (size_t)mb * mb && p.K >= 2 && p.K <= kSmpMaxK &&
         p.phi && p.w && p.values && p.B && p.q1 && p.stats1;
}

bool launch_pair_close(const PairParams &p, int mb, hipStream_t st) {
  if (!pr_geometry(p, mb)) return false;
  const size_t lds = pair_close_lds_bytes(mb, p.e.D, p.K);
  if (lds > 160 * 1024) return false;
  PairParams q = p;
  q.e.lds_m = mb;
  hipLaunchKernelGGL(pair_close_kernel, dim3(q.e.N), dim3(kPairCloseThreads), lds, st, q);
  return true;
}

bool launch_pair_rows(const PairParams &p, int mb, hipStream_t st) {
  if (!pr_geometry(p, mb) || p.n_rows < 1 || !p.rows || !p.Q || !p.qexp || !p.stats) return false;
  const size_t lds_w = pair_walk_lds_bytes(mb, p.e.D), lds_s = pair_stats_lds_bytes(p.e.D, p.K);
  if (lds_w > 160 * 1024 || lds_s > 160 * 1024) return false;
  PairParams q = p;
  q.e.lds_m = mb;
  const int DD = q.e.D * q.e.D;
  hipLaunchKernelGGL(pair_walk_kernel, dim3(q.n_rows, DD), dim3(pair_walk_threads(mb)), lds_w, st, q);
  hipLaunchKernelGGL(pair_stats_kernel, dim3(q.e.N, q.n_rows), dim3(kPairStatThreads), lds_s, st, q);
  return true;
}

}  // namespace tnml
