// Gradient training over all cores (tnml_gd_train_indices / tnml_gd_step): the two kernels that turn the core
// gradients of section 16 into an optimiser step without the host.
//   loss_cot_kernel     one thread per sample: act_and_lossder (act_device.h, the function the sweep's batch kernels call) on the
//                       f [L][f_bpad] of a chunk and its gathered labels -> the loss derivative cot [L][b_pad], zero in the columns
//                       behind the chunk's samples.  For a fixed label a wave reads and writes 64 consecutive floats.
//   optim_step_kernel   one workgroup per site.  G is read through the offset half of the table, the core in its slot
//                       (cores + i * core_stride, or the label core), optimiser state in the flat layout of G.  Two passes over the
//                       first core_elems floats, element e by thread e % 256 (consecutive lanes, consecutive floats):
//                         pass 1  s_A = sum |A_e|, s_d = sum |G_e - wd A_e| in float64: a thread sums its elements in ascending order,
//                                 a fixed tree through LDS combines the 256 partial sums -- the sums depend on the core alone;
//                         pass 2  the update rule (SGD with the per-core clip and momentum, or Adam with decoupled decay), in float64,
//                                 rounded once on the store;
//                         renorm  (likelihood training, section 25) between the two: q0 = sum A_e^2, q1 = sum A'_e^2 of the unrounded
//                                 new elements, summed like pass 1; pass 2 then stores A'_e sqrt(q0 / q1), still one rounding.  The
//                                 factor is 1 where q1 is 0 or not finite.  The state is not rescaled.
//                       With a skip word (section 25) the launch returns at once where the word is set.
//                       No atomics; nothing behind core_elems is touched.
#include "tnml_internal.h"
#include "act_device.h"

namespace tnml {

constexpr int kOptThreads = 256;

size_t loss_cot_lds_bytes(int L) { return (size_t)2 * L * kOptThreads * sizeof(float); }

__global__ __launch_bounds__(kOptThreads) void loss_cot_kernel(LossCotParams p) {
  extern __shared__ float sh[];                     // [2][L][kOptThreads]: activated f, loss derivative
  const int tid = threadIdx.x, s = blockIdx.x * kOptThreads + tid, L = p.L;
  if (s >= p.b_pad) return;
  float *g = sh + (size_t)L * kOptThreads + tid;
  if (s < p.b) {
    float sa;
    int correct, nf = 0;
    act_and_lossder(p.f + s, p.f_bpad, sh + tid, g, kOptThreads, L, p.y[s], p.act_fn, p.loss_fn, p.T, sa, correct, nf);
    for (int l = 0; l < L; ++l) p.cot[(size_t)l * p.b_pad + s] = g[l * kOptThreads];
  } else {
    for (int l = 0; l < L; ++l) p.cot[(size_t)l * p.b_pad + s] = 0.f;
  }
}

bool launch_loss_cot(const LossCotParams &p, hipStream_t st) {
  const size_t lds = loss_cot_lds_bytes(p.L);
  if (p.b < 1 || p.b > p.b_pad || p.b_pad % 64 || p.f_bpad < p.b_pad || p.L < 1 || lds > 64 * 1024) return false;
  if (p.act_fn < 0 || p.act_fn > 2 || p.loss_fn < 0 || p.loss_fn > 2) return false;
  hipLaunchKernelGGL(loss_cot_kernel, dim3((p.b_pad + kOptThreads - 1) / kOptThreads), dim3(kOptThreads), lds, st, p);
  return true;
}

// the 256-entry tree of pass 1 over two sums at once; every thread returns with both totals
__device__ inline void optim_tree2(double (*red)[kOptThreads], int tid, double &a, double &b) {
  red[0][tid] = a;
  red[1][tid] = b;
  __syncthreads();
  for (int w = kOptThreads / 2; w > 0; w >>= 1) {
    if (tid < w) { red[0][tid] += red[0][tid + w]; red[1][tid] += red[1][tid + w]; }
    __syncthreads();
  }
  a = red[0][0];
  b = red[1][0];
  __syncthreads();                                               // (the tree is used again)
}

// The update rule of one element in float64: the change of A[e] (0: the element stays as it is), the new state in st0 / st1.
struct OptimRule {
  int kind;
  bool has_vel;
  double wd, lr, scale, mu, b1, b2, eps, c1, c2;
  __device__ double delta(double a, double g, double s0, double s1, double &st0, double &st1) const {
    if (kind == TNML_OPT_SGD) {
      double d = (g - wd * a) * scale;
      if (has_vel) { d = mu * s0 + d; st0 = d; }
      return lr * d;
    }
    const double mn = b1 * s0 + (1.0 - b1) * g, vn = b2 * s1 + (1.0 - b2) * g * g;
    st0 = mn;
    st1 = vn;
    return lr * ((mn / c1) / (sqrt(vn / c2) + eps) - wd * a);
  }
};

__global__ __launch_bounds__(kOptThreads) void optim_step_kernel(OptimStepParams p) {
  __shared__ double red[2][kOptThreads];
  if (p.skip && *p.skip) return;                                  // (uniform over the launch: the word is written by an earlier launch)
  const int i = blockIdx.x, tid = threadIdx.x, N = p.N;
  const int ml = i == 0 ? 1 : p.tab[i - 1], mr = i == N - 1 ? 1 : p.tab[i];
  const int n = ml * p.D * mr * (i == p.l_pos ? p.L : 1);
  float *A = i == p.l_pos ? p.labcore : p.cores + (size_t)i * p.core_stride;
  const size_t off = (size_t)p.tab[N + i];
  const float *G = p.G + off;
  const double wd = (double)p.wd, lr = (double)p.lr;

  double scale = 1.0;
  if (p.kind == TNML_OPT_SGD && p.clip) {
    double sA = 0.0, sd = 0.0;
    for (int e = tid; e < n; e += kOptThreads) {
      const double a = (double)A[e];
      sA += fabs(a);
      sd += fabs((double)G[e] - wd * a);
    }
    optim_tree2(red, tid, sA, sd);
    if (sd > sA) scale = sA / sd;
  }

  float *s0 = p.s0 ? p.s0 + off : nullptr, *s1 = p.s1 ? p.s1 + off : nullptr;
  const OptimRule rule{p.kind, s0 != nullptr, wd, lr, scale, p.mu, p.beta1, p.beta2, p.eps, p.corr1, p.corr2};

  // renormalisation: the sums of A^2 and of the unrounded A'^2 from the state as it is, before anything is stored; the pass below
  // repeats the rule on the same operands and multiplies by the one factor before its one rounding
  double rs = 1.0;
  if (p.renorm) {
    double q0 = 0.0, q1 = 0.0;
    for (int e = tid; e < n; e += kOptThreads) {
      const double a = (double)A[e];
      double t0 = 0.0, t1 = 0.0;
      const double an = a + rule.delta(a, (double)G[e], s0 ? (double)s0[e] : 0.0, s1 ? (double)s1[e] : 0.0, t0, t1);
      q0 += a * a;
      q1 += an * an;
    }
    optim_tree2(red, tid, q0, q1);
    if (q1 > 0.0 && q1 <= 1.7976931348623157e308) rs = sqrt(q0 / q1);
  }

  for (int e = tid; e < n; e += kOptThreads) {
    const double a = (double)A[e];
    double t0 = 0.0, t1 = 0.0;
    const double delta = rule.delta(a, (double)G[e], s0 ? (double)s0[e] : 0.0, s1 ? (double)s1[e] : 0.0, t0, t1);
    if (s0) s0[e] = (float)t0;
    if (s1) s1[e] = (float)t1;
    if (delta != 0.0 || rs != 1.0) A[e] = (float)((a + delta) * rs);   // (lr = 0 leaves the core bit for bit, a -0 included)
  }
}

bool launch_optim_step(const OptimStepParams &p, hipStream_t st) {
  if (p.N < 2 || p.D < 2 || p.D > kMaxD || p.L < 1 || p.l_pos < 0 || p.l_pos >= p.N) return false;
  if (p.kind != TNML_OPT_SGD && p.kind != TNML_OPT_ADAM) return false;
  if (p.kind == TNML_OPT_ADAM && (!p.s0 || !p.s1 || p.clip)) return false;
  if (p.renorm != 0 && p.renorm != 1) return false;
  hipLaunchKernelGGL(optim_step_kernel, dim3(p.N), dim3(kOptThreads), 0, st, p);
  return true;
}

}  // namespace tnml
