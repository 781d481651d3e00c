// The generic feature-dimension path (D != 2: sweep_anyd / standalone_anyd of tnml_api.hip and the launch wrappers of
// kernels_anyd.hip) planned by the real host code, built --cuda-host-only with AddressSanitizer and UBSan, against the stand-in
// runtime of hip_stub.cpp (every copy checked against its allocation registry).  The stand-in decodes the argument blocks of the
// D == 2 kernels only; the launches of this path pass through check_anyd_launch below first (the binary is linked with
// -Wl,--wrap=hipLaunchKernel), which checks every pointer of their argument blocks together with the extent the kernel touches at
// the context's D -- by a device -> host copy of exactly that range, which the stand-in refuses outside one live allocation.
// `make san-anyd` builds and runs it; tests/test_feature_dim_host.py runs `make san-anyd`.
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../tnml_internal.h"
#include "fail_each.h"

using namespace tnml;

namespace tnml {
__global__ void anyd_transpose_input_kernel(const float *, float *, int, int, int, int);
template <bool LOGMODE>
__global__ void anyd_chain_kernel(const ChainSite *, int, const float *, const float *, const float *, float *, float *, int, int, int, int,
                                  int, float *);
__global__ void anyd_norm_chain_kernel(const NormChainSite *, int, const float *, double *, double *, int);
__global__ void anyd_batch_kernel(WideParams, int, int);
__global__ void anyd_update_kernel(NarrowParams, double *, double *, int);
}  // namespace tnml

extern "C" void san_stub_report(void);
extern "C" long san_stub_launches(const char *substr);
extern "C" hipError_t __real_hipLaunchKernel(const void *fn, dim3 g, dim3 b, void **args, size_t shm, hipStream_t st);

static long g_anyd_checks = 0;
static const char *g_what = "";

[[noreturn]] static void die(const char *fmt, ...) __attribute__((format(printf, 1, 2)));
static void die(const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  fprintf(stderr, "plan_anyd VIOLATION [%s]: ", g_what);
  vfprintf(stderr, fmt, ap);
  fprintf(stderr, "\n");
  va_end(ap);
  abort();
}
// [p, p + bytes) inside one live allocation: the stand-in's copy check aborts otherwise
static void need(const void *p, size_t bytes, const char *what) {
  ++g_anyd_checks;
  if (!p) die("%s: null pointer (%zu bytes wanted)", what, bytes);
  if (!bytes) return;
  std::vector<char> tmp(bytes);
  g_what = what;
  if (hipMemcpy(tmp.data(), p, bytes, hipMemcpyDeviceToHost) != hipSuccess) die("%s: copy refused", what);
}
static void opt(const void *p, size_t bytes, const char *what) { if (p) need(p, bytes, what); }
static size_t view_extent(const CoreView &v, int D, int tail) {
  return (size_t)(v.n_in - 1) * v.s_in + (size_t)(D - 1) * v.s_d + (size_t)(v.n_out - 1) * v.s_out + tail;
}

static void check_batch(const WideParams &p, int D, int do_grad, int nblk) {
  const size_t bp = p.b_pad;
  if (p.b < 1 || p.b > p.b_pad || p.b_pad % 64 || (size_t)nblk * 64 != bp) die("batch: b %d b_pad %d grid %d", p.b, p.b_pad, nblk);
  const bool need_prev = p.do_f || p.do_ext;
  need(p.x_k, bp * D * 4, "batch x_k");
  if (need_prev) need(p.x_km1, bp * D * 4, "batch x_km1");
  opt(p.Hprev, (size_t)p.hp * bp * 4, "batch Hprev");
  need(p.f, (size_t)p.L * bp * 4, "batch f");
  if (p.do_f) { opt(p.Gprev, (size_t)p.gp * bp * 4, "batch Gprev"); need(p.Bprev, (size_t)p.hp * D * D * p.gp * p.L * 4, "batch Bprev"); }
  if (p.do_ext) {
    if (p.ext_core.n_in != p.hp || p.ext_core.n_out != p.h) die("batch: extension core %d x %d for hp %d h %d", p.ext_core.n_in, p.ext_core.n_out, p.hp, p.h);
    need(p.ext_core.base, view_extent(p.ext_core, D, 1) * 4, "batch ext_core");
    need(p.Hcur, (size_t)p.h * bp * 4, "batch Hcur");
  }
  if (!do_grad) return;
  need(p.x_kp1, bp * D * 4, "batch x_kp1");
  opt(p.Hcur, (size_t)p.h * bp * 4, "batch Hcur");
  opt(p.Gcur, (size_t)p.g * bp * 4, "batch Gcur");
  need(p.y, bp * 4, "batch y");
  const size_t RC = (size_t)p.h * D * D * p.g * p.L;
  if ((size_t)p.bsize != RC) die("batch: bsize %d != h D D g L = %zu", p.bsize, RC);
  if ((size_t)p.slab_stride < RC + kMetricSlots) die("batch: slab stride %d < %zu", p.slab_stride, RC + kMetricSlots);
  need(p.slabs, ((size_t)(nblk - 1) * p.slab_stride + RC + kMetricSlots) * 4, "batch slabs");
}

static void check_update(const NarrowParams &p, double *W, double *T2, int w_in_lds) {
  const int D = p.D;
  if (D < 3 || D > kMaxD) die("update: D %d", D);
  const size_t Bs = (size_t)p.h * D * D * p.g * p.L;
  if ((size_t)p.bsize != Bs) die("update: bsize %d != h D D g L = %zu", p.bsize, Bs);
  const int R = p.h * D, C = D * p.g * p.L, n = R < C ? R : C, n_pad = n + (n & 1);
  if (p.m < 1 || p.m > n) die("update: kept rank %d outside [1, %d]", p.m, n);
  need(p.dbg, (4 * Bs + kDbgSigma + 5) * 8, "update capture block");
  need(p.red, (Bs + kMetricSlots) * 4, "update red");
  if (p.Bdirect) need(p.Bdirect, Bs * 4, "update Bdirect");
  else { need(p.lab.base, view_extent(p.lab, D, p.L) * 4, "update label core"); need(p.pl.base, view_extent(p.pl, D, 1) * 4, "update plain core"); }
  if (p.l2_flag) { opt(p.Nh, (size_t)p.h * p.h * 8, "update Nh"); opt(p.Ng, (size_t)p.g * p.g * 8, "update Ng"); }
  need(p.Bnew, Bs * 4, "update Bnew");
  opt(p.metrics, 2 * 4, "update metrics");
  opt(p.counters, 3 * 8, "update counters");
  need(p.status, 4, "update status");
  if (p.stop_after_update) return;
  if (!w_in_lds) need(W, (size_t)n_pad * n_pad * 8, "update eigenvectors (HBM)");
  need(p.out_behind, ((size_t)(p.h - 1) * p.ob_s_h + (size_t)(D - 1) * p.ob_s_d + (size_t)(p.m - 1) * p.ob_s_m + 1) * 4, "update behind core");
  need(p.out_ahead, ((size_t)(p.m - 1) * p.oa_s_m + (size_t)(D - 1) * p.oa_s_d + (size_t)(p.g - 1) * p.oa_s_g + p.L) * 4, "update ahead core");
  if (p.Nh_new && T2) { need(T2, 2 * (size_t)R * p.m * 8, "update T2"); need(p.Nh_new, (size_t)p.m * p.m * 8, "update Nh_new"); }
  if (p.m_out) {        // the adaptive rank the kernel would decide: the cap (what the host then reads back)
    need(p.m_out, 4, "update m_out");
    memcpy(p.m_out, &p.m, 4);
  }
}

static void check_chain(const ChainSite *sites, int n, const float *cores, const float *lab, const float *X, float *env, float *f, int b, int b_pad,
                        int L, int Mmax, int D, float *logmax, int grid) {
  if ((size_t)grid * 64 != (size_t)b_pad || b < 1 || b > b_pad) die("chain: grid %d, b %d, b_pad %d", grid, b, b_pad);
  need(sites, (size_t)n * sizeof(ChainSite), "chain table");
  for (int i = 0; i < n; ++i) {
    const ChainSite &c = sites[i];
    if (c.n_in > Mmax || c.n_out > (Mmax > L ? Mmax : L)) die("chain: site %d is %d -> %d beyond M %d", i, c.n_in, c.n_out, Mmax);
    const size_t ext = (size_t)(c.n_in - 1) * c.s_in + (size_t)(D - 1) * c.s_d + (size_t)(c.n_out - 1) * c.s_out + 1;
    need((c.is_label ? lab : cores) + c.core_off, ext * 4, "chain core");
    need(X + (size_t)c.x_site * b_pad * D, (size_t)b_pad * D * 4, "chain features");
    if (c.env_out_off >= 0) { if (env && !logmax) need(env + c.env_out_off, (size_t)c.n_out * b_pad * 4, "chain environment slot"); }
    else if (!logmax) need(f, (size_t)L * b_pad * 4, "chain f");
    if (i + 1 < n && sites[i + 1].n_in != c.n_out) die("chain: site %d produces %d, site %d takes %d", i, c.n_out, i + 1, sites[i + 1].n_in);
  }
  if (logmax) need(logmax, (size_t)b_pad / 16 * 4, "chain log max partials");
}

static void check_norm(const NormChainSite *sites, int n, const float *cores, double *env, double *T, int D) {
  need(sites, (size_t)n * sizeof(NormChainSite), "norm table");
  for (int i = 0; i < n; ++i) {
    const NormChainSite &c = sites[i];
    need(cores + c.core_off, ((size_t)(c.n_in - 1) * c.s_in + (size_t)(D - 1) * c.s_d + (size_t)(c.n_out - 1) * c.s_out + 1) * 4, "norm core");
    need(env + c.env_out_off, (size_t)c.n_out * c.n_out * 8, "norm environment slot");
    need(T, (size_t)c.n_in * D * c.n_out * 8, "norm scratch");
    if (i + 1 < n && sites[i + 1].n_in != c.n_out) die("norm chain: site %d produces %d, site %d takes %d", i, c.n_out, i + 1, sites[i + 1].n_in);
  }
}

extern "C" hipError_t __wrap_hipLaunchKernel(const void *fn, dim3 g, dim3 b, void **args, size_t shm, hipStream_t st) {
  if (fn == (const void *)&anyd_batch_kernel) {
    g_what = "anyd_batch_kernel";
    check_batch(*(const WideParams *)args[0], *(int *)args[1], *(int *)args[2], (int)g.x);
  } else if (fn == (const void *)&anyd_update_kernel) {
    g_what = "anyd_update_kernel";
    if (g.x != 1) die("update: grid %u", g.x);
    check_update(*(const NarrowParams *)args[0], *(double **)args[1], *(double **)args[2], *(int *)args[3]);
  } else if (fn == (const void *)&anyd_chain_kernel<true> || fn == (const void *)&anyd_chain_kernel<false>) {
    g_what = "anyd_chain_kernel";
    check_chain(*(const ChainSite **)args[0], *(int *)args[1], *(const float **)args[2], *(const float **)args[3], *(const float **)args[4],
                *(float **)args[5], *(float **)args[6], *(int *)args[7], *(int *)args[8], *(int *)args[9], *(int *)args[10], *(int *)args[11],
                *(float **)args[12], (int)g.x);
  } else if (fn == (const void *)&anyd_norm_chain_kernel) {
    g_what = "anyd_norm_chain_kernel";
    check_norm(*(const NormChainSite **)args[0], *(int *)args[1], *(const float **)args[2], *(double **)args[3], *(double **)args[4], *(int *)args[5]);
  } else if (fn == (const void *)&anyd_transpose_input_kernel) {
    g_what = "anyd_transpose_input_kernel";
    const int bb = *(int *)args[2], bp = *(int *)args[3], N = *(int *)args[4], D = *(int *)args[5];
    need(*(const float **)args[0], (size_t)bb * N * D * 4, "transpose input");
    need(*(float **)args[1], (size_t)N * bp * D * 4, "transpose output");
  }
  g_what = "";
  return __real_hipLaunchKernel(fn, g, b, args, shm, st);
}

#define OK(call)                                                                              \
  do {                                                                                        \
    int rc_ = (call);                                                                         \
    if (rc_ != TNML_OK) { fprintf(stderr, "%s:%d %s -> %d: %s\n", __FILE__, __LINE__, #call, rc_, tnml_last_error()); exit(1); } \
  } while (0)
#define FAILS_WITH(code, call)                                                                \
  do {                                                                                        \
    int rc_ = (call);                                                                         \
    if (rc_ != (code)) { fprintf(stderr, "%s:%d %s -> %d, expected %d\n", __FILE__, __LINE__, #call, rc_, (code)); exit(1); } \
  } while (0)

static tnml_ctx *make(int N, int D, int L, int M, int b, std::vector<float> &X, std::vector<int> &y) {
  tnml_ctx *ctx = nullptr;
  OK(tnml_create(&ctx, N, D, L, M, b, 0));
  std::vector<int> bond(N - 1, M);
  size_t total = 0;
  for (int i = 0; i < N; ++i) total += (size_t)(i == 0 ? 1 : M) * D * (i == N - 1 ? 1 : M) * (i == 0 ? L : 1);
  std::vector<float> cores(total);
  for (size_t e = 0; e < total; ++e) cores[e] = 0.1f + 1e-3f * (float)(e % 97);
  OK(tnml_set_cores(ctx, cores.data(), total, bond.data(), 0));
  X.assign((size_t)b * N * D, 0.5f);
  y.resize(b);
  for (int s = 0; s < b; ++s) y[s] = s % L;
  OK(tnml_set_input(ctx, X.data(), y.data(), b));
  return ctx;
}

// whole sweeps, both directions, one policy; forward, calibration, staged batches, prediction on another batch size
static void run_sweeps(int N, int D, int L, int M, int b, int policy, int sweeps) {
  std::vector<float> X;
  std::vector<int> y;
  tnml_ctx *ctx = make(N, D, L, M, b, X, y);
  double lm = 0;
  OK(tnml_forward_logabsmax(ctx, &lm));
  OK(tnml_scale_cores(ctx, 0.9));
  OK(tnml_stage_batch(ctx, 0, X.data(), y.data(), b));
  OK(tnml_stage_batch(ctx, 1, X.data(), y.data(), b > 3 ? b - 3 : b));       // ragged
  std::vector<float> f((size_t)L * b), met((size_t)2 * (N - 1));
  for (int sw = 0; sw < sweeps; ++sw) {
    OK(tnml_select_batch(ctx, sw & 1));
    OK(tnml_forward(ctx, f.data()));
    const int left = tnml_l_pos(ctx) == N - 1;
    const int n1 = (sw & 1) ? N - 1 : ((N - 1) / 3 > 0 ? (N - 1) / 3 : 1), n2 = N - 1 - n1;     // a sweep in one call or in two
    OK(tnml_sweep(ctx, left, n1, 1, 1e-3f, 1e-3f, 1, TNML_ACT_SOFTMAX, TNML_LOSS_FULL_CROSS_ENT, 0.1f, policy, met.data(), n2 ? nullptr : f.data()));
    if (n2) OK(tnml_sweep(ctx, left, n2, 0, 1e-3f, 1e-3f, 1, TNML_ACT_SOFTMAX, TNML_LOSS_FULL_CROSS_ENT, 0.1f, policy, met.data() + 2 * n1, f.data()));
    if (tnml_l_pos(ctx) != (left ? 0 : N - 1)) { fprintf(stderr, "label at %d after a %s sweep\n", tnml_l_pos(ctx), left ? "left" : "right"); exit(1); }
  }
  // a sweep without the L2 term, the switches that have no effect at D != 2
  OK(tnml_set_persistent(ctx, 1)); OK(tnml_set_step_pipeline(ctx, 1)); OK(tnml_set_chain_path(ctx, 1)); OK(tnml_set_narrow_path(ctx, 1));
  OK(tnml_forward(ctx, nullptr));
  OK(tnml_sweep(ctx, tnml_l_pos(ctx) == N - 1, N - 1, 1, 1e-3f, 1e-3f, 0, TNML_ACT_LINEAR, TNML_LOSS_MSE, 1.f, policy, nullptr, f.data()));
  size_t need_ = 0;
  OK(tnml_cores_size(ctx, &need_));
  std::vector<float> back(need_);
  std::vector<int> bond2(N - 1);
  int lp = -1;
  OK(tnml_get_cores(ctx, back.data(), need_, bond2.data(), &lp));
  std::vector<float> Xp((size_t)(b / 2 + 3) * N * D, 0.25f), fp((size_t)L * (b / 2 + 3));
  OK(tnml_predict(ctx, Xp.data(), b / 2 + 3, fp.data()));
  OK(tnml_destroy(ctx));
  printf("planned D %d N %d bond %d L %d b %d policy %d: %d sweeps ok\n", D, N, M, L, b, policy, sweeps);
  fflush(stdout);
}

// the standalone sub-steps and the refusals of this path
static void run_entry_points(int N, int D, int L, int M, int b) {
  std::vector<float> X;
  std::vector<int> y;
  tnml_ctx *ctx = make(N, D, L, M, b, X, y);
  std::vector<float> f((size_t)L * b);
  OK(tnml_forward(ctx, f.data()));
  const size_t nB = (size_t)1 * D * D * M * L;           // sites (0, 1): ml = 1
  std::vector<float> B(nB, 0.01f);
  std::vector<double> Bn(nB), grad(nB);
  float met2[2];
  double loss = 0;
  OK(tnml_update_B(ctx, nullptr, 0, 1e-3f, 1e-3f, 1, TNML_ACT_SOFTMAX, TNML_LOSS_FULL_CROSS_ENT, 1.f, Bn.data(), nB, met2));
  OK(tnml_update_B(ctx, B.data(), 0, 1e-3f, 0.f, 0, TNML_ACT_LINEAR, TNML_LOSS_MSE, 1.f, Bn.data(), nB, nullptr));
  OK(tnml_l2_term(ctx, B.data(), 0, 1e-3f, &loss, grad.data(), nB));
  {
    const int shapes[][3] = {{D, D * 5, 2}, {3 * D, 7 * D, 3 * D}, {7 * D, 3 * D, 5}, {D * M, D * M * L, M}};
    for (auto &sh : shapes) {
      std::vector<float> mat((size_t)sh[0] * sh[1], 0.1f), US((size_t)sh[0] * sh[2]), SV((size_t)sh[2] * sh[1]);
      std::vector<double> sig(sh[0] < sh[1] ? sh[0] : sh[1]);
      OK(tnml_svd_split(ctx, mat.data(), sh[0], sh[1], sh[2], US.data(), SV.data(), sig.data()));
    }
    std::vector<float> mat((size_t)D * 43 * D * 43, 0.1f), US((size_t)D * 43 * 4), SV((size_t)4 * D * 43);
    FAILS_WITH(TNML_ERR_ARG, tnml_svd_split(ctx, mat.data(), D * 43, D * 43, 4, US.data(), SV.data(), nullptr));   // beyond 128 (or the buffers)
    FAILS_WITH(TNML_ERR_ARG, tnml_svd_split(ctx, mat.data(), D + 1, D, 1, US.data(), SV.data(), nullptr));         // not a multiple of D
  }
  OK(tnml_debug_enable(ctx, 1));
  OK(tnml_forward(ctx, nullptr));
  OK(tnml_sweep(ctx, 0, 1, 1, 1e-3f, 1e-3f, 1, TNML_ACT_SOFTMAX, TNML_LOSS_FULL_CROSS_ENT, 0.1f, TNML_TRUNC_FIXED, met2, f.data()));
  std::vector<double> cap((size_t)4 * M * M * L * D * D + 4096);
  size_t got = 0;
  for (int what = TNML_DBG_B; what <= TNML_DBG_L2_GRAD; ++what) OK(tnml_get_step_debug(ctx, what, cap.data(), cap.size(), &got));
  std::vector<float> env((size_t)(M > D * L ? M : D * L) * b);
  int m = 0;
  OK(tnml_get_env(ctx, TNML_SIDE_LEFT, 0, env.data(), env.size(), &m));
  unsigned char uid[128];
  OK(tnml_comm_unique_id(uid));
  FAILS_WITH(TNML_ERR_STATE, tnml_comm_init(ctx, 0, 1, uid));                      // multi-GPU is D = 2 only
  OK(tnml_destroy(ctx));
  printf("entry points D %d N %d bond %d L %d b %d: ok\n", D, N, M, L, b);
  fflush(stdout);
}

// one shape at the 128 limit (D = 4, bond 32 runs a full sweep), one beyond it (bond 33: TNML_ERR_ARG at the first step over it)
static void run_limits() {
  run_sweeps(6, 4, 2, 32, 64, TNML_TRUNC_FIXED, 2);
  std::vector<float> X;
  std::vector<int> y;
  const int N = 6, D = 4, L = 2, M = 33, b = 64;
  tnml_ctx *ctx = make(N, D, L, M, b, X, y);
  OK(tnml_forward(ctx, nullptr));
  int failed_at = -1;
  for (int j = 0; j < N - 1 && failed_at < 0; ++j) {
    const int rc = tnml_sweep(ctx, 0, 1, j == 0, 1e-3f, 1e-3f, 1, TNML_ACT_SOFTMAX, TNML_LOSS_FULL_CROSS_ENT, 0.1f, TNML_TRUNC_FIXED, nullptr, nullptr);
    if (rc == TNML_ERR_ARG) failed_at = j;
    else if (rc != TNML_OK) { fprintf(stderr, "bond 33: step %d -> %d: %s\n", j, rc, tnml_last_error()); exit(1); }
  }
  // bonds after the fixed policy: 4, 16, 33, 33 -> the step on sites (3, 4) has a short side of 4 * 33 = 132
  if (failed_at != 3) { fprintf(stderr, "bond 33 at D = 4: expected TNML_ERR_ARG at step 3, got %d\n", failed_at); exit(1); }
  OK(tnml_destroy(ctx));
  printf("limits D 4: bond 32 ok, bond 33 refused at step %d (%s)\n", failed_at, "short side 132 > 128");
  fflush(stdout);
}

// Failed allocations (injected by the stand-in, see fail_each.h): the scratch of the update kernel is two buffers allocated on first
// use, from a sweep or from a standalone sub-step -- a failure of either leaves none, and the call repeated plans its launches with
// both; then the batch group grows under failure and a sweep is planned over the new buffers
static void run_alloc_failures() {
  const int N = 6, D = 3, L = 2, M = 6, b = 64, b2 = 300;
  std::vector<float> X, f((size_t)L * b2), met((size_t)2 * (N - 1));
  std::vector<int> y;
  auto sweep = [&](tnml_ctx *ctx) {
    return tnml_sweep(ctx, tnml_l_pos(ctx) == N - 1, N - 1, 1, 1e-3f, 1e-3f, 1, TNML_ACT_SOFTMAX, TNML_LOSS_FULL_CROSS_ENT, 0.1f, TNML_TRUNC_FIXED, met.data(), f.data());
  };
  tnml_ctx *ctx = make(N, D, L, M, b, X, y);
  OK(tnml_forward(ctx, f.data()));
  fail_each_alloc("first generic-D sweep", [&] { return sweep(ctx); });
  std::vector<float> X2((size_t)b2 * N * D, 0.5f);
  std::vector<int> y2(b2, 0);
  fail_each_alloc("tnml_set_input, b 64 -> 300 (D = 3)", [&] { return tnml_set_input(ctx, X2.data(), y2.data(), b2); });
  OK(tnml_forward(ctx, f.data()));
  OK(sweep(ctx));
  OK(tnml_destroy(ctx));
  ctx = make(N, D, L, M, b, X, y);
  OK(tnml_forward(ctx, f.data()));
  const size_t nB = (size_t)1 * D * D * M * L;
  std::vector<float> B(nB, 0.01f);
  std::vector<double> grad(nB);
  double loss = 0;
  fail_each_alloc("first standalone sub-step (tnml_l2_term)", [&] { return tnml_l2_term(ctx, B.data(), 0, 1e-3f, &loss, grad.data(), nB); });
  OK(sweep(ctx));
  OK(tnml_destroy(ctx));
}

int main() {
  FAILS_WITH(TNML_ERR_ARG, tnml_create(nullptr, 8, 3, 2, 4, 16, 0));
  tnml_ctx *bad = nullptr;
  FAILS_WITH(TNML_ERR_ARG, tnml_create(&bad, 8, 1, 2, 4, 16, 0));
  FAILS_WITH(TNML_ERR_ARG, tnml_create(&bad, 8, 9, 2, 4, 16, 0));
  const int policies[] = {TNML_TRUNC_FIXED, TNML_TRUNC_REFERENCE, TNML_TRUNC_ADAPTIVE};
  for (int D : {3, 4})
    for (int pol : policies) {
      run_sweeps(12, D, 2, 6, 77, pol, 2);
      run_sweeps(9, D, 3, 5, 130, pol, 2);              // odd bond, three labels
    }
  run_sweeps(60, 3, 2, 20, 300, TNML_TRUNC_FIXED, 2);    // the bench's D = 3 bond (short side 60) on a shorter chain
  run_sweeps(7, 8, 2, 4, 64, TNML_TRUNC_REFERENCE, 2);
  run_entry_points(8, 3, 2, 6, 50);
  run_entry_points(7, 4, 3, 5, 40);
  run_limits();
  run_alloc_failures();
  san_stub_report();
  const char *paths[] = {"anyd_batch_kernel", "anyd_update_kernel", "anyd_chain_kernel", "anyd_norm_chain_kernel", "anyd_transpose_input_kernel",
                         "reduce_slabs_kernel"};
  for (const char *k : paths)
    if (san_stub_launches(k) < 1) { fprintf(stderr, "launch path %s was never taken\n", k); return 1; }
  printf("generic-D launches: %ld argument extents checked\n", g_anyd_checks);
  printf("generic-D host planning under ASan + UBSan: ok\n");
  return 0;
}
