// Inner products and linear combinations of two MPS (tnml_inner / tnml_axpby).  W is the context's chain (plain
// cores in their slots, the label core in its buffer), V a second chain with the same N, D, L and label position in the flat layout of
// tnml_get_cores.  Three kernels, float64 throughout, no atomic, every sum in a fixed order, and no waiting between workgroups: the
// hand-overs are launch boundaries.
//   inner_chain_kernel  grid (products, 2 halves), one workgroup per half-chain.  It walks its sites towards the label:
//                         1  both cores -> float64 in the workgroup's staging area of global memory, as (in, d, out) with `in` the bond
//                            towards the chain end; the metric S_i is folded into the second chain's core on the way;
//                         2  per d:  T_d = A_d^T E  into LDS (one barrier), E' += T_d B_d  in registers (one barrier);
//                         3  E <- 2^-k E', k = ilogb(max |E'|) + 1 (0 where the maximum is 0), k joins the half's exponent.
//                       E and T_d live in LDS (two areas of max-bond^2 doubles); the half's E and exponent go to global memory.
//                       A non-finite float reaches E' as a NaN or an infinity whatever the other factor is: the maximum sees it
//                       and the status word is set.
//   inner_meet_kernel   one workgroup per product: per (d, l') X = E_L^T A_l into LDS, Y = X E_R in registers, the product with the
//                       (metric-folded) label core of the second chain summed per thread and then over the workgroup in a fixed tree.
//   sum_place_kernel    one workgroup per site: the whole float32 scratch slot of alpha W + beta V as the direct sum -- zeros, then
//                       the two blocks; alpha and beta multiply the label-site blocks in float64, one rounding per element.
// The three products <W|W>, <V|V>, <W|V> run the same instructions on different pointers: a V that is bit-equal to W gives three
// bit-equal results.
#include "tnml_internal.h"

#include <algorithm>
#include <cmath>

namespace tnml {

constexpr int kAlgThreads = 1024;
constexpr int kAlgPlaceThreads = 256;
constexpr int kAlgAcc = 10;                 // elements of E' a thread owns at the most: kAlgAcc * kAlgThreads >= max-bond^2 wherever the LDS fits
constexpr int kAlgWaves = kAlgThreads / 64;

size_t algebra_chain_lds_bytes(int mb_w, int mb_v) {
  const size_t m = (size_t)std::max(mb_w, mb_v);
  return (2 * m * m + 2 * kAlgWaves) * sizeof(double);
}
size_t algebra_meet_lds_bytes(int mb_w, int mb_v) {
  const size_t m = (size_t)std::max(mb_w, mb_v);
  return (m * m + kAlgThreads) * sizeof(double);
}

// one chain as the kernels address it: core i at plain + off[i] (ml, D, mr), the label core at lab (ml, D, mr, L)
struct AlgChain { const float *plain, *lab; const long long *off; const int *bond; };
__device__ inline AlgChain alg_chain(const AlgebraParams &p, int which) {
  AlgChain c;
  c.plain = which ? p.v_plain : p.w_plain;
  c.lab = which ? p.v_lab : p.w_lab;
  c.off = p.off + (size_t)which * p.N;
  c.bond = p.bond + (size_t)which * (p.N - 1);
  return c;
}
__device__ inline int alg_ml(const AlgChain &c, int i) { return i == 0 ? 1 : c.bond[i - 1]; }
__device__ inline int alg_mr(const AlgChain &c, int i, int N) { return i == N - 1 ? 1 : c.bond[i]; }
__device__ inline const double *alg_metric(const AlgebraParams &p, int site) {
  return p.metric_sites == 0 ? nullptr : p.metric + (p.metric_sites == 1 ? 0 : (size_t)site * p.D * p.D);
}
// products: 0 <W|W>, 1 <V|V>, 2 <W|V>
__device__ inline int alg_first(int prod) { return prod == 1 ? 1 : 0; }
__device__ inline int alg_second(int prod) { return prod == 0 ? 0 : 1; }

// dst[(in * D + d) * nout + out] = sum_d' S[d][d'] core(in, d', out), or the core itself where S is null.  right: `in` is the right bond
__device__ void alg_stage(const float *src, int ml, int mr, int D, bool right, const double *S, double *dst) {
  const int nin = right ? mr : ml, nout = right ? ml : mr, n = nin * D * nout;
  for (int e = threadIdx.x; e < n; e += kAlgThreads) {
    const int out = e % nout, d = (e / nout) % D, in = e / (nout * D);
    const int a = right ? out : in, c = right ? in : out;
    double v;
    if (S) {
      v = 0.0;
      for (int dd = 0; dd < D; ++dd) v = fma(S[d * D + dd], (double)src[((size_t)a * D + dd) * mr + c], v);
    } else {
      v = (double)src[((size_t)a * D + d) * mr + c];
    }
    dst[e] = v;
  }
}

// the maximum of one value per thread; every thread receives it (red: 2 * kAlgWaves doubles, alternating halves)
__device__ double alg_block_max(double x, double *red) {
  for (int o = 32; o > 0; o >>= 1) x = fmax(x, __shfl_xor(x, o, 64));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
  __syncthreads();
  double r = red[0];
  for (int w = 1; w < kAlgWaves; ++w) r = fmax(r, red[w]);
  return r;
}

__global__ __launch_bounds__(kAlgThreads) void inner_chain_kernel(AlgebraParams p) {
  extern __shared__ __attribute__((aligned(16))) double alg_sh[];
  const int tid = threadIdx.x, prod = blockIdx.x, half = blockIdx.y, N = p.N, D = p.D, l = p.l_pos;
  const int wg = prod * 2 + half;
  double *E = alg_sh, *T = E + p.lds_m2, *red = T + p.lds_m2;
  const AlgChain ca = alg_chain(p, alg_first(prod)), cb = alg_chain(p, alg_second(prod));
  double *As = p.stage + (size_t)wg * 2 * p.stage_stride, *Bs = As + p.stage_stride;
  const bool right = half == 1;
  const int n_sites = right ? N - 1 - l : l;

  if (tid == 0) E[0] = 1.0;
  int nia = 1, nib = 1, expo = 0, bad = 0;
  __syncthreads();
  for (int s = 0; s < n_sites; ++s) {
    const int i = right ? N - 1 - s : s;
    const int mla = alg_ml(ca, i), mra = alg_mr(ca, i, N), mlb = alg_ml(cb, i), mrb = alg_mr(cb, i, N);
    const int noa = right ? mla : mra, nob = right ? mlb : mrb;
    // 1  both cores as (in, d, out) doubles
    alg_stage(ca.plain + ca.off[i], mla, mra, D, right, nullptr, As);
    alg_stage(cb.plain + cb.off[i], mlb, mrb, D, right, alg_metric(p, i), Bs);
    __syncthreads();
    // 2  E'[oa][ob] = sum_d sum_ib (sum_ia A(ia, d, oa) E[ia][ib]) B(ib, d, ob)
    double acc[kAlgAcc];
#pragma unroll
    for (int k = 0; k < kAlgAcc; ++k) acc[k] = 0.0;
    const int nT = noa * nib, nE = noa * nob;
    for (int d = 0; d < D; ++d) {
      for (int e = tid; e < nT; e += kAlgThreads) {
        const int oa = e % noa, ib = e / noa;
        const double *a = As + (size_t)d * noa + oa;
        double v = 0.0;
        for (int ia = 0; ia < nia; ++ia) v = fma(a[(size_t)ia * D * noa], E[ia * nib + ib], v);
        T[oa * nib + ib] = v;
      }
      __syncthreads();
#pragma unroll
      for (int k = 0; k < kAlgAcc; ++k) {
        const int e = tid + k * kAlgThreads;
        if (e < nE) {
          const int oa = e / nob, ob = e % nob;
          const double *b = Bs + (size_t)d * nob + ob, *t = T + oa * nib;
          double v = acc[k];
          for (int ib = 0; ib < nib; ++ib) v = fma(t[ib], b[(size_t)ib * D * nob], v);
          acc[k] = v;
        }
      }
      __syncthreads();
    }
    // 3  rescale by an exact power of two
    double mx = 0.0;
#pragma unroll
    for (int k = 0; k < kAlgAcc; ++k) {
      const double a = fabs(acc[k]);
      mx = fmax(mx, a <= 1.7976931348623157e308 ? a : INFINITY);      // (a NaN fails the comparison)
    }
    mx = alg_block_max(mx, red + (s & 1) * kAlgWaves);
    if (!(mx <= 1.7976931348623157e308)) { bad = 1; break; }
    const int kexp = mx > 0.0 ? ilogb(mx) + 1 : 0;
#pragma unroll
    for (int k = 0; k < kAlgAcc; ++k) {
      const int e = tid + k * kAlgThreads;
      if (e < nE) E[e] = ldexp(acc[k], -kexp);
    }
    expo += kexp;
    nia = noa; nib = nob;
    __syncthreads();
  }
  double *out = p.half_E + (size_t)wg * p.half_stride;
  for (int e = tid; e < nia * nib; e += kAlgThreads) out[e] = bad ? 0.0 : E[e];
  if (tid == 0) {
    p.half_expo[wg] = expo;
    if (bad) p.status[0] = 1;                                    // (every writer stores the same word)
  }
}

__global__ __launch_bounds__(kAlgThreads) void inner_meet_kernel(AlgebraParams p) {
  extern __shared__ __attribute__((aligned(16))) double alg_sh[];
  const int tid = threadIdx.x, prod = blockIdx.x, N = p.N, D = p.D, L = p.L, l = p.l_pos;
  double *X = alg_sh, *red = X + p.lds_m2;
  const AlgChain ca = alg_chain(p, alg_first(prod)), cb = alg_chain(p, alg_second(prod));
  const int mla = alg_ml(ca, l), mra = alg_mr(ca, l, N), mlb = alg_ml(cb, l), mrb = alg_mr(cb, l, N);
  const double *EL = p.half_E + (size_t)(prod * 2) * p.half_stride, *ER = EL + p.half_stride;
  const double *S = alg_metric(p, l);
  const float *A = ca.lab, *B = cb.lab;
  double acc = 0.0;
  for (int d = 0; d < D; ++d)
    for (int lp = 0; lp < L; ++lp) {
      // X[a'][c] = sum_a E_L[a][a'] A[a][d][c][l']
      for (int e = tid; e < mlb * mra; e += kAlgThreads) {
        const int c = e % mra, ap = e / mra;
        double v = 0.0;
        for (int a = 0; a < mla; ++a) v = fma(EL[a * mlb + ap], (double)A[(((size_t)a * D + d) * mra + c) * L + lp], v);
        X[e] = v;
      }
      __syncthreads();
      // Y[a'][c'] = sum_c X[a'][c] E_R[c][c'], times the second chain's label core (metric folded)
      for (int e = tid; e < mlb * mrb; e += kAlgThreads) {
        const int cp = e % mrb, ap = e / mrb;
        double y = 0.0;
        for (int c = 0; c < mra; ++c) y = fma(X[ap * mra + c], ER[c * mrb + cp], y);
        double b;
        if (S) {
          b = 0.0;
          for (int dd = 0; dd < D; ++dd) b = fma(S[d * D + dd], (double)B[(((size_t)ap * D + dd) * mrb + cp) * L + lp], b);
        } else {
          b = (double)B[(((size_t)ap * D + d) * mrb + cp) * L + lp];
        }
        acc = fma(y, b, acc);
      }
      __syncthreads();
    }
  red[tid] = acc;
  __syncthreads();
  for (int w = kAlgThreads / 2; w > 0; w >>= 1) {
    if (tid < w) red[tid] += red[tid + w];
    __syncthreads();
  }
  if (tid == 0) {
    const double v = red[0];
    const int ex = p.half_expo[prod * 2] + p.half_expo[prod * 2 + 1];
    if (!(fabs(v) <= 1.7976931348623157e308)) p.status[0] = 1;
    p.out[2 * prod] = v > 0.0 ? 1.0 : (v < 0.0 ? -1.0 : 0.0);
    p.out[2 * prod + 1] = v != 0.0 ? log(fabs(v)) + (double)ex * 0.6931471805599453094 : -INFINITY;
  }
}

__global__ __launch_bounds__(kAlgPlaceThreads) void sum_place_kernel(AlgebraParams p) {
  const int i = blockIdx.x, tid = threadIdx.x, N = p.N, D = p.D;
  const AlgChain cw = alg_chain(p, 0), cv = alg_chain(p, 1);
  const bool lab = i == p.l_pos;
  const int Lx = lab ? p.L : 1;
  const int wl = alg_ml(cw, i), wr = alg_mr(cw, i, N), vl = alg_ml(cv, i), vr = alg_mr(cv, i, N);
  const int nl = i == 0 ? 1 : wl + vl, nr = i == N - 1 ? 1 : wr + vr;
  const size_t n = (size_t)nl * D * nr * Lx, cap = lab ? p.lab_elems : p.core_stride;
  const float *W = lab ? cw.lab : cw.plain + cw.off[i], *V = lab ? cv.lab : cv.plain + cv.off[i];
  float *dst = lab ? p.out_lab : p.out_cores + (size_t)i * p.core_stride;
  bool bad = false;
  for (size_t e = tid; e < cap; e += kAlgPlaceThreads) {
    float r = 0.f;
    if (e < n) {
      const int lp = (int)(e % Lx), c = (int)((e / Lx) % nr), d = (int)((e / ((size_t)Lx * nr)) % D), a = (int)(e / ((size_t)Lx * nr * D));
      const bool in_w = (i == 0 || a < wl) && (i == N - 1 || c < wr), in_v = (i == 0 || a >= wl) && (i == N - 1 || c >= wr);
      if (in_w) {
        const float x = W[(((size_t)a * D + d) * wr + c) * Lx + lp];
        r = lab ? (float)(p.alpha * (double)x) : x;
      } else if (in_v) {
        const int av = i == 0 ? a : a - wl, cvv = i == N - 1 ? c : c - wr;
        const float x = V[(((size_t)av * D + d) * vr + cvv) * Lx + lp];
        r = lab ? (float)(p.beta * (double)x) : x;
      }
      if (!(fabsf(r) <= 3.4028234e38f)) bad = true;
    }
    dst[e] = r;
  }
  if (lab)                                                       // the label site's plain slot holds nothing
    for (size_t e = tid; e < p.core_stride; e += kAlgPlaceThreads) p.out_cores[(size_t)i * p.core_stride + e] = 0.f;
  if (bad) p.status[0] = 1;
}

static bool alg_geometry(const AlgebraParams &p) {
  return p.N >= 2 && p.D >= 2 && p.D <= kMaxD && p.L >= 1 && p.l_pos >= 0 && p.l_pos < p.N;
}

bool launch_inner(const AlgebraParams &p, int mb_w, int mb_v, hipStream_t st) {
  if (!alg_geometry(p) || (p.n_prod != 1 && p.n_prod != 3) || mb_w < 1 || mb_v < 1) return false;
  if (p.metric_sites != 0 && p.metric_sites != 1 && p.metric_sites != p.N) return false;
  const size_t m = (size_t)std::max(mb_w, mb_v), lds = algebra_chain_lds_bytes(mb_w, mb_v), lds2 = algebra_meet_lds_bytes(mb_w, mb_v);
  if (lds > 160 * 1024 || lds2 > 160 * 1024 || m * m > (size_t)kAlgAcc * kAlgThreads) return false;
  if (p.half_stride < m * m || p.stage_stride < m * m * p.D) return false;
  AlgebraParams q = p;
  q.lds_m2 = (int)(m * m);
  hipLaunchKernelGGL(inner_chain_kernel, dim3(q.n_prod, 2), dim3(kAlgThreads), lds, st, q);
  hipLaunchKernelGGL(inner_meet_kernel, dim3(q.n_prod), dim3(kAlgThreads), lds2, st, q);
  return true;
}

bool launch_sum_place(const AlgebraParams &p, hipStream_t st) {
  if (!alg_geometry(p)) return false;
  hipLaunchKernelGGL(sum_place_kernel, dim3(p.N), dim3(kAlgPlaceThreads), 0, st, p);
  return true;
}

}  // namespace tnml
