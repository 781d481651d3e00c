// The gradient of the log-norm and the likelihood of a batch (tnml_log_norm_grad, tnml_nll_grad(_indices), tnml_nll_eval(_indices) of
// tnml_api.hip and the launch wrappers of kernels_nll.hip) planned by the real
// host code, built --cuda-host-only with AddressSanitizer and UBSan, against the stand-in runtime of hip_stub.cpp, which reads the
// table of every launch as the kernels do and checks every core, both environment stacks, both exponent arrays and every core's
// part of G with its extent.  Nothing computes there: the outputs come back as the memory holds them.  `make san-nll` builds and
// runs it; tests/test_nll_host.py runs `make san-nll`.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../tnml_internal.h"
#include "fail_each.h"

extern "C" void san_stub_report(void);
extern "C" long san_stub_launches(const char *substr);

static int g_refusals = 0;

#define OK(call)                                                                              \
  do {                                                                                        \
    int rc_ = (call);                                                                         \
    if (rc_ != TNML_OK) { fprintf(stderr, "%s:%d %s -> %d: %s\n", __FILE__, __LINE__, #call, rc_, tnml_last_error()); exit(1); } \
  } while (0)
// the call is refused with `code` before anything is launched
#define FAILS_WITH(code, call)                                                                \
  do {                                                                                        \
    const long before_ = san_stub_launches("");                                               \
    int rc_ = (call);                                                                         \
    if (rc_ != (code)) { fprintf(stderr, "%s:%d %s -> %d, expected %d\n", __FILE__, __LINE__, #call, rc_, (code)); exit(1); } \
    if (san_stub_launches("") != before_) { fprintf(stderr, "%s:%d %s launched before it failed\n", __FILE__, __LINE__, #call); exit(1); } \
    ++g_refusals;                                                                             \
  } while (0)
#define CHECK(cond, ...) do { if (!(cond)) { fprintf(stderr, "%s:%d ", __FILE__, __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } } while (0)

struct Chain {
  std::vector<int32_t> bond;
  std::vector<float> flat;
  Chain(int N, int D, int L, const std::vector<int> &b, int l_pos, float v = 0.1f) : bond(b.begin(), b.end()) {
    size_t total = 0;
    for (int i = 0; i < N; ++i) total += (size_t)(i == 0 ? 1 : b[i - 1]) * D * (i == N - 1 ? 1 : b[i]) * (i == l_pos ? L : 1);
    flat.assign(total, v);
  }
};

static void set_cores(tnml_ctx *ctx, const Chain &w, int l_pos) { OK(tnml_set_cores(ctx, w.flat.data(), w.flat.size(), w.bond.data(), l_pos)); }

// the call without a metric and with both metric forms: each is one launch of either kernel, and writes nothing behind the gradient
static void grad_calls(tnml_ctx *ctx, int N, int D, const Chain &w) {
  std::vector<double> S((size_t)N * D * D, 0.5);
  std::vector<float> G(w.flat.size() + 1, -7.f);
  double sl[2];
  const long a = san_stub_launches("lognorm_env_kernel"), b = san_stub_launches("lognorm_grad_kernel");
  OK(tnml_log_norm_grad(ctx, nullptr, 0, G.data(), w.flat.size(), sl));
  OK(tnml_log_norm_grad(ctx, nullptr, 1, G.data(), w.flat.size() + 1, sl));
  OK(tnml_log_norm_grad(ctx, S.data(), 0, G.data(), w.flat.size(), sl));
  OK(tnml_log_norm_grad(ctx, S.data(), 1, G.data(), w.flat.size(), sl));
  CHECK(G.back() == -7.f, "the float behind the gradient was written");
  CHECK(san_stub_launches("lognorm_env_kernel") - a == 4 && san_stub_launches("lognorm_grad_kernel") - b == 4, "four calls did not make four launches of each kernel");
}

// the likelihood of a batch: both objectives, X and index forms, the default chunk and chunks of 64, gradient and value alone
static void nll_calls(tnml_ctx *ctx, int N, int D, int L, const Chain &w, int b) {
  std::vector<float> X((size_t)b * N * D, 0.5f), G(w.flat.size() + 1, -7.f);
  std::vector<int32_t> y(b), idx(b);
  for (int s = 0; s < b; ++s) { y[s] = s % L; idx[s] = (s * 7) % b; }
  std::vector<double> S((size_t)D * D, 0.5);
  double out3[3];
  OK(tnml_dataset_attach(ctx, X.data(), y.data(), b, N, D, TNML_DATASET_FEATURES));
  for (int chunk : {0, 64}) {
    OK(tnml_set_core_grad_chunk(ctx, chunk));
    const long e = san_stub_launches("lognorm_env_kernel"), g = san_stub_launches("lognorm_grad_kernel"), t = san_stub_launches("nll_sum_kernel");
    const long q = san_stub_launches("nll_cot_kernel"), r = san_stub_launches("core_grad_reduce_kernel");
    OK(tnml_nll_grad(ctx, X.data(), y.data(), b, S.data(), G.data(), w.flat.size(), out3));
    OK(tnml_nll_grad(ctx, X.data(), nullptr, b, nullptr, G.data(), w.flat.size(), out3));
    OK(tnml_nll_grad_indices(ctx, idx.data(), b, 1, S.data(), G.data(), w.flat.size(), out3));
    OK(tnml_nll_grad_indices(ctx, idx.data(), b, 0, nullptr, G.data(), w.flat.size(), out3));
    CHECK(san_stub_launches("lognorm_grad_kernel") - g == 4 && san_stub_launches("core_grad_reduce_kernel") - r == san_stub_launches("nll_cot_kernel") - q,
          "four gradients: one subtraction each, one reduction per cotangent");
    const long r2 = san_stub_launches("core_grad_reduce_kernel");
    OK(tnml_nll_eval(ctx, X.data(), y.data(), b, S.data(), out3));
    OK(tnml_nll_eval(ctx, X.data(), nullptr, b, nullptr, out3));
    OK(tnml_nll_eval_indices(ctx, idx.data(), b, 1, S.data(), out3));
    OK(tnml_nll_eval_indices(ctx, idx.data(), b, 0, nullptr, out3));
    CHECK(san_stub_launches("lognorm_env_kernel") - e == 8 && san_stub_launches("lognorm_grad_kernel") - g == 4 && san_stub_launches("nll_sum_kernel") - t == 8 &&
          san_stub_launches("core_grad_reduce_kernel") == r2, "the value alone launched a gradient kernel");
    if (chunk == 64) CHECK(san_stub_launches("nll_cot_kernel") - q == 8 * ((b + 63) / 64), "chunks of 64: %ld cotangent launches for b %d", san_stub_launches("nll_cot_kernel") - q, b);
  }
  OK(tnml_set_core_grad_chunk(ctx, 0));
  CHECK(G.back() == -7.f, "the float behind the gradient was written");
  OK(tnml_dataset_detach(ctx));
}

static void run_true_size(const char *name, int N, int D, int L, int M, int l_pos) {
  tnml_ctx *ctx = nullptr;
  OK(tnml_create(&ctx, N, D, L, M, 64, 0));
  OK(tnml_set_any_position(ctx, 1));
  Chain w(N, D, L, std::vector<int>(N - 1, M), l_pos);
  set_cores(ctx, w, l_pos);
  grad_calls(ctx, N, D, w);
  nll_calls(ctx, N, D, L, w, 200);
  OK(tnml_destroy(ctx));
  printf("planned the log-norm gradient %s bond %d L %d, label on %d\n", name, M, L, l_pos);
  fflush(stdout);
}

// a ragged chain at every label position (and N = 2); the group grows when a label position brings a larger bond
static void run_ragged(int N, int D, int L, int M) {
  tnml_ctx *ctx = nullptr;
  OK(tnml_create(&ctx, N, D, L, M, 64, 0));
  OK(tnml_set_any_position(ctx, 1));
  for (int l = 0; l < N; ++l) {
    std::vector<int> bw(N - 1);
    for (int i = 0; i < N - 1; ++i) bw[i] = 1 + (i * 7 + l * 3) % (M - 1);
    if (l >= N / 2) bw[(l * 5) % (N - 1)] = M;
    Chain w(N, D, L, bw, l);
    set_cores(ctx, w, l);
    grad_calls(ctx, N, D, w);
    nll_calls(ctx, N, D, L, w, l % 2 ? 70 : 17);
  }
  OK(tnml_destroy(ctx));
  printf("planned the log-norm gradient ragged N %d D %d L %d bonds <= %d at every label position\n", N, D, L, M);
  fflush(stdout);
}

static void run_refusals() {
  const int N = 6, D = 2, L = 3, M = 4;
  tnml_ctx *ctx = nullptr;
  OK(tnml_create(&ctx, N, D, L, M, 64, 0));
  Chain w(N, D, L, std::vector<int>(N - 1, M), 2);
  std::vector<float> G(w.flat.size());
  const size_t n = G.size();
  double sl[2];
  std::vector<double> S((size_t)N * D * D, 0.5);
  FAILS_WITH(TNML_ERR_STATE, tnml_log_norm_grad(ctx, nullptr, 0, G.data(), n, sl));                  // cores never set
  set_cores(ctx, w, 2);
  FAILS_WITH(TNML_ERR_ARG, tnml_log_norm_grad(nullptr, nullptr, 0, G.data(), n, sl));
  FAILS_WITH(TNML_ERR_ARG, tnml_log_norm_grad(ctx, nullptr, 0, nullptr, n, sl));
  FAILS_WITH(TNML_ERR_ARG, tnml_log_norm_grad(ctx, nullptr, 0, G.data(), n, nullptr));
  FAILS_WITH(TNML_ERR_ARG, tnml_log_norm_grad(ctx, nullptr, 2, G.data(), n, sl));
  FAILS_WITH(TNML_ERR_ARG, tnml_log_norm_grad(ctx, S.data(), -1, G.data(), n, sl));
  FAILS_WITH(TNML_ERR_ARG, tnml_log_norm_grad(ctx, nullptr, 0, G.data(), n - 1, sl));
  {
    std::vector<double> T(S);
    T[1] = 0.25;                                                                                      // S[0][1] != S[1][0]
    FAILS_WITH(TNML_ERR_ARG, tnml_log_norm_grad(ctx, T.data(), 0, G.data(), n, sl));
    CHECK(strstr(tnml_last_error(), "symmetric"), "the refusal does not say symmetric: %s", tnml_last_error());
    T = S;
    T[(size_t)3 * D * D + 3] = NAN;                                                                   // site 3 of a per-site metric
    OK(tnml_log_norm_grad(ctx, T.data(), 0, G.data(), n, sl));                                        // (a shared metric ends after D D entries)
    FAILS_WITH(TNML_ERR_ARG, tnml_log_norm_grad(ctx, T.data(), 1, G.data(), n, sl));
    CHECK(strstr(tnml_last_error(), "site 3"), "the refusal does not name the site: %s", tnml_last_error());
    T[(size_t)3 * D * D + 3] = INFINITY;
    FAILS_WITH(TNML_ERR_ARG, tnml_log_norm_grad(ctx, T.data(), 1, G.data(), n, sl));
  }
  OK(tnml_log_norm_grad(ctx, S.data(), 1, G.data(), n, sl));                                          // usable afterwards
  {
    const int b = 5;
    std::vector<float> X((size_t)b * N * D, 0.5f);
    std::vector<int32_t> y(b, 1), idx(b, 0);
    double out3[3];
    FAILS_WITH(TNML_ERR_ARG, tnml_nll_grad(nullptr, X.data(), y.data(), b, nullptr, G.data(), n, out3));
    FAILS_WITH(TNML_ERR_ARG, tnml_nll_grad(ctx, nullptr, y.data(), b, nullptr, G.data(), n, out3));
    FAILS_WITH(TNML_ERR_ARG, tnml_nll_grad(ctx, X.data(), y.data(), b, nullptr, nullptr, n, out3));
    FAILS_WITH(TNML_ERR_ARG, tnml_nll_grad(ctx, X.data(), y.data(), b, nullptr, G.data(), n, nullptr));
    FAILS_WITH(TNML_ERR_ARG, tnml_nll_grad(ctx, X.data(), y.data(), 0, nullptr, G.data(), n, out3));
    FAILS_WITH(TNML_ERR_ARG, tnml_nll_grad(ctx, X.data(), y.data(), b, nullptr, G.data(), n - 1, out3));
    y[3] = L;
    FAILS_WITH(TNML_ERR_ARG, tnml_nll_grad(ctx, X.data(), y.data(), b, nullptr, G.data(), n, out3));
    FAILS_WITH(TNML_ERR_ARG, tnml_nll_eval(ctx, X.data(), y.data(), b, nullptr, out3));
    y[3] = 0;
    std::vector<double> T(S);
    T[2] = 0.75;
    FAILS_WITH(TNML_ERR_ARG, tnml_nll_grad(ctx, X.data(), y.data(), b, T.data(), G.data(), n, out3));
    FAILS_WITH(TNML_ERR_STATE, tnml_nll_grad_indices(ctx, idx.data(), b, 1, nullptr, G.data(), n, out3));   // no dataset
    FAILS_WITH(TNML_ERR_STATE, tnml_nll_eval_indices(ctx, idx.data(), b, 1, nullptr, out3));
    OK(tnml_dataset_attach(ctx, X.data(), y.data(), b, N, D, TNML_DATASET_FEATURES));
    idx[2] = b;
    FAILS_WITH(TNML_ERR_ARG, tnml_nll_grad_indices(ctx, idx.data(), b, 1, nullptr, G.data(), n, out3));
    FAILS_WITH(TNML_ERR_ARG, tnml_nll_eval_indices(ctx, idx.data(), b, 0, nullptr, out3));
    idx[2] = 0;
    FAILS_WITH(TNML_ERR_ARG, tnml_nll_grad_indices(ctx, nullptr, b, 1, nullptr, G.data(), n, out3));
    FAILS_WITH(TNML_ERR_ARG, tnml_nll_eval_indices(ctx, idx.data(), 0, 1, nullptr, out3));
    OK(tnml_nll_grad_indices(ctx, idx.data(), b, 1, nullptr, G.data(), n, out3));
    OK(tnml_nll_grad(ctx, X.data(), y.data(), b, S.data(), G.data(), n, out3));
  }
  OK(tnml_destroy(ctx));
  // bond 64 is taken, bond 65 refused with the bytes in the message
  OK(tnml_create(&ctx, 4, 2, 2, 65, 64, 0));
  Chain fits(4, 2, 2, std::vector<int>{2, 64, 2}, 1), big(4, 2, 2, std::vector<int>{2, 65, 2}, 1);
  std::vector<float> Gb(big.flat.size());
  set_cores(ctx, big, 1);
  FAILS_WITH(TNML_ERR_ARG, tnml_log_norm_grad(ctx, nullptr, 0, Gb.data(), Gb.size(), sl));
  CHECK(strstr(tnml_last_error(), "bytes of LDS") && strstr(tnml_last_error(), "bond 65"), "the bond refusal names neither: %s", tnml_last_error());
  {
    std::vector<float> X((size_t)3 * 4 * 2, 0.5f);
    double out3[3];
    FAILS_WITH(TNML_ERR_ARG, tnml_nll_grad(ctx, X.data(), nullptr, 3, nullptr, Gb.data(), Gb.size(), out3));
    FAILS_WITH(TNML_ERR_ARG, tnml_nll_eval(ctx, X.data(), nullptr, 3, nullptr, out3));
  }
  set_cores(ctx, fits, 1);
  OK(tnml_log_norm_grad(ctx, nullptr, 0, Gb.data(), Gb.size(), sl));
  OK(tnml_destroy(ctx));
  // D = 8: the environments and their product at bond 64 are beyond the LDS
  OK(tnml_create(&ctx, 4, 8, 2, 64, 64, 0));
  Chain wide(4, 8, 2, std::vector<int>{2, 64, 2}, 1), narrow(4, 8, 2, std::vector<int>{2, 40, 2}, 1);
  std::vector<float> Gw(wide.flat.size());
  set_cores(ctx, wide, 1);
  FAILS_WITH(TNML_ERR_ARG, tnml_log_norm_grad(ctx, nullptr, 0, Gw.data(), Gw.size(), sl));
  CHECK(strstr(tnml_last_error(), "bytes of LDS"), "the LDS refusal does not name the bytes: %s", tnml_last_error());
  set_cores(ctx, narrow, 1);
  OK(tnml_log_norm_grad(ctx, nullptr, 0, Gw.data(), Gw.size(), sl));
  OK(tnml_destroy(ctx));
  // with a communicator the call is refused
  setenv("TNML_FORCE_COMM", "1", 1);
  OK(tnml_create(&ctx, N, D, L, M, 64, 0));
  unsigned char uid[128];
  OK(tnml_comm_unique_id(uid));
  OK(tnml_comm_init(ctx, 0, 1, uid));
  Chain w0(N, D, L, std::vector<int>(N - 1, M), 0);
  set_cores(ctx, w0, 0);
  FAILS_WITH(TNML_ERR_STATE, tnml_log_norm_grad(ctx, nullptr, 0, G.data(), n, sl));
  OK(tnml_destroy(ctx));
  unsetenv("TNML_FORCE_COMM");
  printf("log-norm gradient refusals: ok\n");
}

// the call leaves everything as it was: no new forward before a sweep, and the optimiser state stays bound
static void run_state_rule() {
  const int N = 8, D = 2, L = 2, M = 6, b = 40;
  const int kAct = TNML_ACT_SOFTMAX, kLoss = TNML_LOSS_FULL_CROSS_ENT;
  tnml_ctx *ctx = nullptr;
  OK(tnml_create(&ctx, N, D, L, M, 64, 0));
  std::vector<float> X((size_t)b * N * D, 0.5f), f((size_t)L * b);
  std::vector<int> lab(b, 1);
  Chain w(N, D, L, std::vector<int>(N - 1, 2), 0);
  std::vector<float> G(w.flat.size()), back(w.flat.size());
  double met[3], sl[2];
  set_cores(ctx, w, 0);
  OK(tnml_optim_config(ctx, TNML_OPT_SGD, 0.9, 0.9, 0.999, 1e-8, 0));
  OK(tnml_gd_step(ctx, X.data(), lab.data(), b, 0.1f, 0.f, kAct, kLoss, 0.1f, met));
  OK(tnml_set_input(ctx, X.data(), lab.data(), b));
  OK(tnml_forward(ctx, f.data()));
  OK(tnml_log_norm_grad(ctx, nullptr, 0, G.data(), G.size(), sl));
  OK(tnml_gd_step(ctx, X.data(), lab.data(), b, 0.1f, 0.f, kAct, kLoss, 0.1f, met));                  // the state is still bound
  OK(tnml_forward(ctx, f.data()));
  OK(tnml_log_norm_grad(ctx, nullptr, 0, G.data(), G.size(), sl));
  OK(tnml_sweep(ctx, 0, 2, 1, 1e-3f, 1e-3f, 1, kAct, kLoss, 0.1f, TNML_TRUNC_FIXED, nullptr, nullptr));   // no new forward needed
  OK(tnml_destroy(ctx));
  printf("state rule of the log-norm gradient: ok\n");
}

// every allocation of the new group fails in turn, fresh and when a larger bond makes it grow
static void run_alloc_failures(int D) {
  const int N = 6, L = 2, M = 12;
  tnml_ctx *ctx = nullptr;
  OK(tnml_create(&ctx, N, D, L, M, 64, 0));
  Chain w(N, D, L, std::vector<int>(N - 1, 3), 3), w5(N, D, L, std::vector<int>(N - 1, 5), 3);
  std::vector<float> G(w5.flat.size());
  double sl[2];
  set_cores(ctx, w, 3);
  int k = fail_each_alloc("tnml_log_norm_grad, fresh context", [&] { return tnml_log_norm_grad(ctx, nullptr, 0, G.data(), G.size(), sl); });
  if (k != 9) { fprintf(stderr, "%d allocations failed in turn, the group has 9\n", k); exit(1); }
  k = fail_each_alloc("tnml_log_norm_grad, the group exists", [&] { return tnml_log_norm_grad(ctx, nullptr, 0, G.data(), G.size(), sl); });
  if (k != 0) { fprintf(stderr, "%d allocations in a second call\n", k); exit(1); }
  set_cores(ctx, w5, 3);
  k = fail_each_alloc("tnml_log_norm_grad, a larger bond", [&] { return tnml_log_norm_grad(ctx, nullptr, 0, G.data(), G.size(), sl); });
  if (k != 9) { fprintf(stderr, "%d allocations failed in turn when the group grew, it has 9\n", k); exit(1); }
  OK(tnml_destroy(ctx));
  // the likelihood calls on a fresh context: the prediction, core-gradient, log-norm and per-sample groups, then growth of the last
  OK(tnml_create(&ctx, N, D, L, M, 64, 0));
  OK(tnml_set_any_position(ctx, 1));
  set_cores(ctx, w, 3);
  const int b = 70, b2 = 1500;
  std::vector<float> X((size_t)b2 * N * D, 0.5f);
  std::vector<int32_t> y(b2, 1);
  double out3[3];
  k = fail_each_alloc("tnml_nll_grad, fresh context", [&] { return tnml_nll_grad(ctx, X.data(), y.data(), b, nullptr, G.data(), G.size(), out3); });
  if (k < 3) { fprintf(stderr, "%d allocations failed in turn, the per-sample group alone has 3\n", k); exit(1); }      // (groups made by an earlier round stay)
  k = fail_each_alloc("tnml_nll_eval, more samples", [&] { return tnml_nll_eval(ctx, X.data(), y.data(), b2, nullptr, out3); });
  if (k < 3) { fprintf(stderr, "%d allocations failed in turn when the per-sample group grew, it has 3\n", k); exit(1); }
  k = fail_each_alloc("tnml_nll_grad, the groups exist", [&] { return tnml_nll_grad(ctx, X.data(), nullptr, b, nullptr, G.data(), G.size(), out3); });
  if (k != 0) { fprintf(stderr, "%d allocations in a later call\n", k); exit(1); }
  OK(tnml_destroy(ctx));
}

int main() {
  run_true_size("c3", 784, 2, 2, 20, 0);
  run_true_size("c3 last", 784, 2, 2, 20, 783);
  run_true_size("c3 inner label", 784, 2, 2, 20, 391);
  run_true_size("c5", 784, 2, 10, 50, 783);
  run_true_size("c5 first", 784, 2, 10, 50, 0);
  run_true_size("c5 inner label", 784, 2, 10, 50, 400);
  run_ragged(17, 2, 3, 5);
  run_ragged(17, 3, 3, 7);
  run_ragged(17, 8, 17, 6);
  run_ragged(2, 2, 2, 5);
  run_ragged(2, 8, 10, 3);
  run_refusals();
  run_state_rule();
  run_alloc_failures(2);
  run_alloc_failures(3);
  san_stub_report();
  const char *paths[] = {"lognorm_env_kernel", "lognorm_grad_kernel", "nll_cot_kernel", "nll_sum_kernel"};
  for (const char *k : paths)
    if (san_stub_launches(k) < 1) { fprintf(stderr, "launch path %s was never taken\n", k); return 1; }
  printf("nll: %ld lognorm_env_kernel and %ld lognorm_grad_kernel launches checked, %d refusals\n", san_stub_launches("lognorm_env_kernel"),
         san_stub_launches("lognorm_grad_kernel"), g_refusals);
  printf("log-norm gradient host planning under ASan + UBSan: ok\n");
  return 0;
}
