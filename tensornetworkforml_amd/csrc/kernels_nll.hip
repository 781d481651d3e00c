// Likelihood gradients: the gradient of the log-norm, d log|<W|W>_S| / d A_i for every core of the chain
// (tnml_log_norm_grad), and the cotangent and per-sample terms of the negative log-likelihood of a batch (tnml_nll_grad).
// float64 throughout, no float atomic, every sum in a fixed order, no waiting between workgroups: the hand-over between the two
// kernels is a launch boundary.
//   lognorm_env_kernel   two workgroups.  Workgroup 0 walks L_1 .. L_{N-1}, L_{i+1}[c][c'] = sum S[d][d'] A_i[a][d][c] L_i[a][a'] A_i[a'][d'][c'],
//                        L_0 = 1; workgroup 1 walks R_{N-1} .. R_0, R_i[a][a'] = sum S[d][d'] A_i[a][d][c] R_{i+1}[c][c'] A_i[a'][d'][c'], R_N = 1;
//                        the label is summed on the label site (class_plus1 0) or slice class_plus1 - 1 alone is taken.  Every matrix is multiplied by an exact 2^-k, k = ilogb(max|.|) + 1,
//                        and stored with the RUNNING exponent of its side: L_i 2^eL_i and R_i 2^eR_i are the true environments, and
//                        <W|W>_S = R_0 2^eR_0.  Per site and label slice, with E the environment the walk comes from:
//                          1  T = A . E (right walk, rows (a, d)) or E^T . A (left walk, columns (d, c)) on the f64 matrix cores, the
//                             float32 core read as it is stored;
//                          2  the metric folded into T in place: T[a][d][c] <- sum_d' S[d][d'] T[a][d'][c], one thread per (a, c);
//                          3  E' += T . A^T (right) or A^T . T (left) on the matrix cores, one owner per element.
//   lognorm_grad_kernel  grid (N, L); the slices above 0 exist on the label site only.  Per site and slice: L_i and R_{i+1} into LDS,
//                        X = L_i . A_i, the metric folded into X in place, Gz = X . R_{i+1}, every element times
//                        2 / R_0 in float64, then the power of two 2^(eL_i + eR_{i+1} - eR_0) by ldexp, then the cast to float32.
//                        mode 0 stores Gz in the flat layout of tnml_get_cores, mode 1 replaces G[e] by G[e] - Gz[e] there.
//   nll_cot_kernel       one thread per sample of a chunk, in the mould of loss_cot_kernel: from f [L][f_bpad] the cotangent of the data
//                        term of -log p, cot[l'][s] = 2 delta(l', y_s) / (b f_y[s]) with labels (float32, as the emulation of
//                        tests/nll_reference.py forms it) or 2 f_l'[s] / (b sum_l f_l[s]^2) without (formed in float64, rounded once),
//                        zero in the columns behind the chunk; the sample's term log f_y^2 or log sum_l f_l^2 in float64 into
//                        terms[off + s], and bad[off + s] = 1 where a cotangent or the term is not finite (f_y == 0, a non-finite f).
//   nll_sum_kernel       one workgroup: acc[0] = sum of terms[0 .. n), acc[1] = sum of bad[0 .. n).  A thread sums its elements in
//                        ascending order, a fixed tree combines the 256 partial sums: the result depends on n alone, not on the chunks.
//   nll_record_kernel    one workgroup, after nll_sum_kernel and the norm launches of a likelihood step (section 25): the step's four
//                        values into its slot and the sticky skip word that optim_step_kernel reads first.  Plain stores.
// Status words: status[0], written by the environment launch alone, bit 1 a non-finite environment, bit 2 <W|W>_S == 0; status[1],
// written by the gradient launch alone, bit 4 a gradient element beyond float32.  The gradient kernel returns at once where
// status[0] is set: it reads nothing that a workgroup of its own launch writes.
#include "small_gemm_device.h"
#include "lognorm_device.h"

#include <cmath>

namespace tnml {

constexpr int kLnzEnvThreads = 1024;
constexpr int kLnzEnvWaves = kLnzEnvThreads / 64;
constexpr int kLnzGradThreads = 512;

size_t lognorm_env_lds_bytes(int mb, int D) {
  const size_t m = (size_t)mb;
  return (2 * m * m + m * D * m + 2 * kLnzEnvWaves) * sizeof(double);
}
size_t lognorm_grad_lds_bytes(int mb, int D) {
  const size_t m = (size_t)mb;
  return (2 * m * m + m * D * m) * sizeof(double);
}

__device__ double lnz_block_max(double x, double *red) {
  for (int o = 32; o > 0; o >>= 1) x = fmax(x, __shfl_xor(x, o, 64));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
  __syncthreads();
  double r = red[0];
  for (int w = 1; w < kLnzEnvWaves; ++w) r = fmax(r, red[w]);
  return r;
}

__global__ __launch_bounds__(kLnzEnvThreads) void lognorm_env_kernel(LogNormParams p) {
  extern __shared__ __attribute__((aligned(16))) double lnz_sh[];
  const int tid = threadIdx.x, N = p.N, D = p.D, l = p.l_pos;
  const bool right = blockIdx.x == 1;
  const size_t m = (size_t)p.lds_m;
  double *E = lnz_sh, *En = E + m * m, *T = En + m * m, *red = T + m * D * m;
  double *stack = right ? p.envR : p.envL;
  int *ex = right ? p.expR : p.expL;
  const int n_sites = right ? N : N - 1;
  if (tid == 0) {
    const int start = right ? N : 0;
    E[0] = 1.0;
    stack[(size_t)start * p.env_stride] = 1.0;
    ex[start] = 0;
  }
  int expo = 0, bad = 0;
  __syncthreads();
  for (int s = 0; s < n_sites; ++s) {
    const int i = right ? N - 1 - s : s;
    const int ml = lnz_ml(p, i), mr = lnz_mr(p, i), Dm = D * mr;
    const int nout = right ? ml : mr;
    const bool lab = i == l;
    const int Lx = lab ? p.L : 1;
    const float *A = lab ? p.lab : p.cores + (size_t)i * p.core_stride;
    const double *S = lnz_metric(p, i);
    for (int e = tid; e < nout * nout; e += kLnzEnvThreads) En[e] = 0.0;     // (product 3 is behind two barriers)
    const int l0 = lab && p.class_plus1 > 0 ? p.class_plus1 - 1 : 0, l1 = lab && p.class_plus1 > 0 ? l0 + 1 : Lx;   // (a class: its slice alone)
    for (int lp = l0; lp < l1; ++lp) {
      const float *Al = A + lp;
      if (right)   // T[(a, d)][c'] = sum_c A[a][d][c] E[c][c']
        mm_lds(1, ml * D, mr, mr, Al, 0, mr * Lx, Lx, E, 0, mr, 1, [&](int, int r, int j, double v) { T[r * mr + j] = v; });
      else         // T[a'][(d, c)] = sum_a E[a][a'] A[a][d][c]
        mm_lds(1, ml, Dm, ml, E, 0, 1, ml, Al, 0, Dm * Lx, Lx, [&](int, int r, int j, double v) { T[r * Dm + j] = v; });
      __syncthreads();
      if (S) {
        lnz_fold_metric(T, S, ml, mr, D, kLnzEnvThreads);
        __syncthreads();
      }
      if (right)   // E'[a][a'] += sum_x T[a][x] A[a'][x], x = (d, c')
        mm_lds(1, ml, ml, Dm, T, 0, Dm, 1, Al, 0, Lx, Dm * Lx, [&](int, int r, int j, double v) { En[r * ml + j] += v; });
      else         // E'[c'][c] += sum_k A[k][c'] T[k][c], k = (a', d)
        mm_lds(1, mr, mr, ml * D, Al, 0, Lx, mr * Lx, T, 0, mr, 1, [&](int, int r, int j, double v) { En[r * mr + j] += v; });
      __syncthreads();
    }
    double mx = 0.0;
    for (int e = tid; e < nout * nout; e += kLnzEnvThreads) {
      const double a = fabs(En[e]);
      mx = fmax(mx, a <= kLnzDblMax ? a : INFINITY);               // (a NaN fails the comparison)
    }
    mx = lnz_block_max(mx, red + (s & 1) * kLnzEnvWaves);
    if (!(mx <= kLnzDblMax)) { bad = 1; break; }
    const int kexp = mx > 0.0 ? ilogb(mx) + 1 : 0;
    expo += kexp;
    const int slot = right ? i : i + 1;
    double *out = stack + (size_t)slot * p.env_stride;
    for (int e = tid; e < nout * nout; e += kLnzEnvThreads) {
      const double v = ldexp(En[e], -kexp);
      E[e] = v;
      out[e] = v;
    }
    if (tid == 0) ex[slot] = expo;
    __syncthreads();
  }
  if (tid == 0) {
    if (bad) atomicOr(p.status, 1);
    else if (right) {
      const double v = E[0];
      if (v == 0.0) atomicOr(p.status, 2);
      p.out[0] = v > 0.0 ? 1.0 : (v < 0.0 ? -1.0 : 0.0);
      p.out[1] = v != 0.0 ? log(fabs(v)) + (double)expo * 0.6931471805599453094 : -INFINITY;
    }
  }
}

__global__ __launch_bounds__(kLnzGradThreads) void lognorm_grad_kernel(LogNormParams p) {
  extern __shared__ __attribute__((aligned(16))) double lnz_sh[];
  const int tid = threadIdx.x, i = blockIdx.x, lp = blockIdx.y, N = p.N, D = p.D;
  const bool lab = i == p.l_pos;
  if (lp > 0 && !lab) return;
  if (p.status[0] & 3) return;
  const size_t m = (size_t)p.lds_m;
  double *Lm = lnz_sh, *Rm = Lm + m * m, *X = Rm + m * m;
  const int ml = lnz_ml(p, i), mr = lnz_mr(p, i), Dm = D * mr, Lx = lab ? p.L : 1;
  const float *Al = (lab ? p.lab : p.cores + (size_t)i * p.core_stride) + lp;
  const double *S = lnz_metric(p, i);
  const double *Lg = p.envL + (size_t)i * p.env_stride, *Rg = p.envR + (size_t)(i + 1) * p.env_stride;
  for (int e = tid; e < ml * ml; e += kLnzGradThreads) Lm[e] = Lg[e];
  for (int e = tid; e < mr * mr; e += kLnzGradThreads) Rm[e] = Rg[e];
  const double two_over_R0 = 2.0 / p.envR[0];
  const int ex = p.expL[i] + p.expR[i + 1] - p.expR[0];
  __syncthreads();
  // X[a][(d, c')] = sum_a' L_i[a][a'] A[a'][d][c']
  mm_lds(1, ml, Dm, ml, Lm, 0, ml, 1, Al, 0, Dm * Lx, Lx, [&](int, int r, int j, double v) { X[r * Dm + j] = v; });
  __syncthreads();
  if (S) {
    lnz_fold_metric(X, S, ml, mr, D, kLnzGradThreads);
    __syncthreads();
  }
  // Gz[(a, d)][c] = sum_c' X[(a, d)][c'] R_{i+1}[c'][c]
  float *G = p.G + p.tab[N + i] + lp;
  const int mode = p.mode;
  bool bad = false;
  mm_lds(1, ml * D, mr, mr, X, 0, mr, 1, Rm, 0, mr, 1, [&](int, int r, int j, double v) {
    const float g = (float)ldexp(v * two_over_R0, ex);
    if (!(fabsf(g) <= 3.4028234e38f)) bad = true;
    float *dst = G + (size_t)(r * mr + j) * Lx;
    *dst = mode ? *dst - g : g;
  });
  if (bad) atomicOr(p.status + 1, 4);                            // (its own word: status[0] is only read in this launch)
}

constexpr int kNllThreads = 256;

__global__ __launch_bounds__(kNllThreads) void nll_cot_kernel(NllCotParams p) {
  const int s = blockIdx.x * kNllThreads + threadIdx.x, L = p.L;
  if (s >= p.b_pad) return;
  if (s >= p.b) {
    if (p.cot)
      for (int l = 0; l < L; ++l) p.cot[(size_t)l * p.b_pad + s] = 0.f;
    return;
  }
  const float *f = p.f + s;
  bool bad = false;
  double term;
  if (p.y) {
    const int y = p.y[s];
    const float fy = f[(size_t)y * p.f_bpad];
    const float c = 2.f / ((float)p.batch * fy);
    bad = !(fabsf(c) <= 3.4028234e38f);
    term = log((double)fy * (double)fy);
    if (p.cot)
      for (int l = 0; l < L; ++l) p.cot[(size_t)l * p.b_pad + s] = l == y ? c : 0.f;
  } else {
    double den = 0.0;
    for (int l = 0; l < L; ++l) {
      const double v = (double)f[(size_t)l * p.f_bpad];
      den = fma(v, v, den);
    }
    const double k = 2.0 / ((double)p.batch * den);
    for (int l = 0; l < L; ++l) {
      const float c = (float)(k * (double)f[(size_t)l * p.f_bpad]);
      bad = bad || !(fabsf(c) <= 3.4028234e38f);
      if (p.cot) p.cot[(size_t)l * p.b_pad + s] = c;
    }
    term = log(den);
  }
  bad = bad || !(fabs(term) <= kLnzDblMax);
  p.terms[p.off + s] = term;
  p.bad[p.off + s] = bad ? 1 : 0;
}

__global__ __launch_bounds__(kNllThreads) void nll_sum_kernel(const double *__restrict__ terms, const int *__restrict__ bad, int n, double *__restrict__ acc) {
  __shared__ double red[2][kNllThreads];
  const int tid = threadIdx.x;
  double t = 0.0, nb = 0.0;
  for (int e = tid; e < n; e += kNllThreads) { t += terms[e]; nb += (double)bad[e]; }
  red[0][tid] = t;
  red[1][tid] = nb;
  __syncthreads();
  for (int w = kNllThreads / 2; w > 0; w >>= 1) {
    if (tid < w) { red[0][tid] += red[0][tid + w]; red[1][tid] += red[1][tid + w]; }
    __syncthreads();
  }
  if (tid == 0) { acc[0] = red[0][0]; acc[1] = red[1][0]; }
}

__global__ __launch_bounds__(64) void nll_record_kernel(const double *__restrict__ acc, const double *__restrict__ out, const int *__restrict__ status,
                                                        double *__restrict__ rec, int *__restrict__ skip) {
  if (threadIdx.x != 0) return;
  const double nbad = acc[1];
  int bits = status[0] | status[1];
  if (!(nbad == 0.0)) bits |= kNllStepBadBatch;                   // (a NaN count is a bad batch too)
  int sk = *skip;
  if (bits) { sk = 1; *skip = 1; }
  if (sk) bits |= kNllStepNotApplied;
  rec[0] = acc[0];
  rec[1] = out[1];
  rec[2] = nbad;
  rec[3] = (double)bits;
}

bool launch_nll_record(const double *acc, const double *out, const int *status, double *rec, int *skip, hipStream_t st) {
  if (!acc || !out || !status || !rec || !skip) return false;
  hipLaunchKernelGGL(nll_record_kernel, dim3(1), dim3(64), 0, st, acc, out, status, rec, skip);
  return true;
}

bool launch_nll_cot(const NllCotParams &p, hipStream_t st) {
  if (p.b < 1 || p.b > p.b_pad || p.b_pad % 64 || p.f_bpad < p.b_pad || p.L < 1 || p.off < 0 || p.batch < 1) return false;
  hipLaunchKernelGGL(nll_cot_kernel, dim3((p.b_pad + kNllThreads - 1) / kNllThreads), dim3(kNllThreads), 0, st, p);
  return true;
}

bool launch_nll_sum(const double *terms, const int *bad, int n, double *acc, hipStream_t st) {
  if (n < 1) return false;
  hipLaunchKernelGGL(nll_sum_kernel, dim3(1), dim3(kNllThreads), 0, st, terms, bad, n, acc);
  return true;
}

static bool lnz_geometry(const LogNormParams &p) {
  return p.N >= 2 && p.D >= 2 && p.D <= kMaxD && p.L >= 1 && p.l_pos >= 0 && p.l_pos < p.N &&
         (p.metric_sites == 0 || p.metric_sites == 1 || p.metric_sites == p.N) && (p.mode == 0 || p.mode == 1) && p.class_plus1 >= 0 &&
         p.class_plus1 <= p.L;
}

bool launch_lognorm_env(const LogNormParams &p, int mb, hipStream_t st) {
  if (!lnz_geometry(p) || mb < 1 || mb > kLnzMaxBond) return false;
  const size_t m = (size_t)mb, lds = lognorm_env_lds_bytes(mb, p.D);
  if (lds > 160 * 1024 || p.env_stride < m * m) return false;
  LogNormParams q = p;
  q.lds_m = mb;
  hipLaunchKernelGGL(lognorm_env_kernel, dim3(2), dim3(kLnzEnvThreads), lds, st, q);
  return true;
}

bool launch_lognorm_grad(const LogNormParams &p, int mb, hipStream_t st) {
  if (!lnz_geometry(p) || p.class_plus1 != 0 || mb < 1 || mb > kLnzMaxBond) return false;
  const size_t m = (size_t)mb, lds = lognorm_grad_lds_bytes(mb, p.D);
  if (lds > 160 * 1024 || p.env_stride < m * m) return false;
  LogNormParams q = p;
  q.lds_m = mb;
  hipLaunchKernelGGL(lognorm_grad_kernel, dim3(q.N, q.L), dim3(kLnzGradThreads), lds, st, q);
  return true;
}

}  // namespace tnml
