// What the walks over the metric environments do alike on the device: lognorm_env_kernel and lognorm_grad_kernel (kernels_nll.hip,
// DESIGN.md section 24) and the pair kernels (kernels_pair.hip, section 28).  The form and the operand order of every expression
// here are part of those kernels' results.
#pragma once
#include "tnml_internal.h"

namespace tnml {

constexpr double kLnzDblMax = 1.7976931348623157e308;

__device__ inline int lnz_ml(const LogNormParams &p, int i) { return i == 0 ? 1 : p.tab[i - 1]; }
__device__ inline int lnz_mr(const LogNormParams &p, int i) { return i == p.N - 1 ? 1 : p.tab[i]; }
__device__ inline const double *lnz_metric(const LogNormParams &p, int i) {
  return p.metric_sites == 0 ? nullptr : p.metric + (p.metric_sites == 1 ? 0 : (size_t)i * p.D * p.D);
}

// T[a][d][c] <- sum_d' S[d][d'] T[a][d'][c] in place: the thread of (a, c) owns its D elements
__device__ inline void lnz_fold_metric(double *T, const double *S, int ml, int mr, int D, int nthreads) {
  for (int e = threadIdx.x; e < ml * mr; e += nthreads) {
    const int a = e / mr, c = e % mr;
    double *t = T + (size_t)a * D * mr + c;
    double in[kMaxD];
#pragma unroll
    for (int d = 0; d < kMaxD; ++d) in[d] = d < D ? t[(size_t)d * mr] : 0.0;
#pragma unroll
    for (int d = 0; d < kMaxD; ++d)
      if (d < D) {
        double v = 0.0;
#pragma unroll
        for (int dd = 0; dd < kMaxD; ++dd)
          if (dd < D) v = fma(S[d * D + dd], in[dd], v);
        t[(size_t)d * mr] = v;
      }
  }
}

}  // namespace tnml
