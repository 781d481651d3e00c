// What the two samplers do alike on the device: tnml_sample's walk (kernels_sample.hip) and tnml_sample_masked's
// (kernels_sample_masked.hip, section 23).  The helpers take plain pointers and scalars -- the two kernels keep their own parameter
// blocks, LDS maps and barriers -- and each is called by one whole wave for one sample of its tile: every lane gets the same result.
// Both kernels are compiled with contraction on and their results are tested bit for bit (tests/test_sample_bits_gpu.py): the form
// and the operand order of every floating-point expression here are part of the result.
#pragma once
#include "tnml_internal.h"

#include <cmath>

namespace tnml {

constexpr double kSmpDblMax = 1.7976931348623157e308;

__host__ __device__ inline size_t smp_even(size_t x) { return (x + 1) & ~(size_t)1; }

// the bonds to the left and to the right of site i; bond[] is the chain's table
__device__ inline int smp_ml(const int *bond, int i) { return i == 0 ? 1 : bond[i - 1]; }
__device__ inline int smp_mr(const int *bond, int N, int i) { return i == N - 1 ? 1 : bond[i]; }

// the counter hash: SplitMix64 of seed + (s (N + 1) + j + 1) GOLDEN, s the CALL's sample number, j the site (N: the label)
__device__ inline double smp_uniform(unsigned long long seed, long long s, int j, int N) {
  unsigned long long z = seed + ((unsigned long long)s * (unsigned long long)(N + 1) + (unsigned long long)j + 1ull) * 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z = z ^ (z >> 31);
  return (double)(z >> 11) * 1.1102230246251565e-16;             // 2^-53
}

// Q[d][d'] = sum_c T[d][c] U[d'][c] of one sample, one lane per entry; T and U are the sample's D rows of mr.  It only writes: the
// barrier between this and the first read of Q is the caller's.
__device__ inline void smp_form_Q(const double *T, const double *U, double *Q, int D, int mr, int lane) {
  if (lane < D * D) {
    const double *t = T + (size_t)(lane / D) * mr, *u = U + (size_t)(lane % D) * mr;
    double v = 0.0;
    for (int c = 0; c < mr; ++c) v = fma(t[c], u[c], v);
    Q[lane] = v;
  }
}

// one draw: the level or label, its density, the sum of all densities, and whether one of them was not finite
struct SmpPick {
  int k;
  double psel, total;
  bool nonfinite;
};

// The level of one site from the sample's Q: the K densities w_k phi_k^T Q phi_k (four consecutive levels per lane; negative and
// non-finite ones count as zero), an inclusive scan over the wave, the first level whose cumulative sum exceeds u total (the last
// level of positive density where rounding leaves none).  forced >= 0: that level instead, psel its density.
__device__ inline SmpPick smp_pick_level(const double *Q, const double *phi, const double *w, int K, int D, int lane, double u, int forced) {
  double pl[4];
  bool nonfinite = false;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int k = 4 * lane + j;
    double v = 0.0;
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
  if (forced >= 0) k = forced;
  const int j = k & 3;
  const double mine = j == 0 ? pl[0] : j == 1 ? pl[1] : j == 2 ? pl[2] : pl[3];
  return {k, __shfl(mine, k >> 2, 64), total, nonfinite};
}

// The label from the sample's P(l'), l' < L, by the rule of the pixels (every lane computes the same)
__device__ inline SmpPick smp_pick_label(const double *P, int L, double u) {
  double total = 0.0;
  bool nonfinite = false;
  for (int lp = 0; lp < L; ++lp) {
    const double a = P[lp];
    if (!(fabs(a) <= kSmpDblMax)) nonfinite = true;
    else total += a > 0.0 ? a : 0.0;
  }
  const double t = u * total;
  int pick = -1, lastpos = 0;
  double c = 0.0, psel = 0.0, plast = 0.0;
  for (int lp = 0; lp < L; ++lp) {
    const double a0 = P[lp], a = a0 > 0.0 && a0 <= kSmpDblMax ? a0 : 0.0;
    c += a;
    if (pick < 0 && c > t) { pick = lp; psel = a; }
    if (a > 0.0) { lastpos = lp; plast = a; }
  }
  if (pick < 0) { pick = lastpos; psel = plast; }
  return {pick, psel, total, nonfinite};
}

// The new v[lane] = sum_d phi_k[d] U[d][lane], lane < mr, times the power of two that brings the wave's largest magnitude below 1
__device__ inline double smp_next_v(const double *phi_k, const double *U, int D, int mr, int lane) {
  double v = 0.0;
  if (lane < mr)
    for (int d = 0; d < D; ++d) v = fma(phi_k[d], U[(size_t)d * mr + lane], v);
  double mx = fabs(v);
  for (int o = 32; o > 0; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o, 64));
  if (mx > 0.0 && mx <= kSmpDblMax) v = ldexp(v, -(ilogb(mx) + 1));
  return v;
}

// A draw that cannot be used marks its sample dead, once: status bit 1 for a non-finite density, bit 2 and the smallest sample
// number in status[1] for densities that sum to nothing
__device__ inline void smp_mark_dead(int *status, int sample, int &dead, int lane, bool nonfinite, double total) {
  if (dead) return;
  if (nonfinite) { dead = 1; if (lane == 0) atomicOr(status, 1); }
  else if (!(total > 0.0)) { dead = 1; if (lane == 0) { atomicOr(status, 2); atomicMin(status + 1, sample); } }
}

}  // namespace tnml
