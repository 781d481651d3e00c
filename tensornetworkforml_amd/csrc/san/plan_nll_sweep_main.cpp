// The two-site likelihood sweep (tnml_nll_sweep, tnml_nll_sweep_indices, tnml_nll_sweep_debug of nll_sweep_host.hip and the launch
// wrappers of kernels_nll_sweep.hip) planned by the real host code, built --cuda-host-only with AddressSanitizer and UBSan, against the
// stand-in runtime of hip_stub.cpp, which checks every copy and every launch argument block against its allocation registry.
// Nothing computes there: the records come back as the memory holds them (zeros), so the kept rank of a step is the planned one and
// the adaptive rank (which the host reads back from the device) cannot be planned here.  `make san-nll-sweep` builds and runs it;
// tests/test_nll_sweep_host.py runs `make san-nll-sweep`.
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

// n steps: one merge, batch, reduction, sum, update, split and environment launch each, and the call's two walks and its norm walk
static void sweep_counted(tnml_ctx *ctx, const float *X, const int32_t *y, const int32_t *idx, int b, const double *S, int left, int n, int renorm,
                          int max_bond, double *vals) {
  const long m0 = san_stub_launches("nll_sweep_merge_kernel"), b0 = san_stub_launches("nll_sweep_batch_kernel"),
             u0 = san_stub_launches("nll_sweep_update_kernel"), e0 = san_stub_launches("nll_sweep_extend_kernel"),
             c0 = san_stub_launches("nll_sweep_chain_kernel"), w0 = san_stub_launches("lognorm_env_kernel");
  if (idx) OK(tnml_nll_sweep_indices(ctx, idx, b, y != nullptr, S, left, n, 1e-2f, renorm, max_bond, 1.0, vals));
  else OK(tnml_nll_sweep(ctx, X, y, b, S, left, n, 1e-2f, renorm, max_bond, 1.0, vals));
  CHECK(san_stub_launches("nll_sweep_merge_kernel") - m0 == n && san_stub_launches("nll_sweep_batch_kernel") - b0 == n &&
        san_stub_launches("nll_sweep_update_kernel") - u0 == n && san_stub_launches("nll_sweep_extend_kernel") - e0 == n,
        "%d steps, other launch counts", n);
  CHECK(san_stub_launches("nll_sweep_chain_kernel") - c0 == 2 && san_stub_launches("lognorm_env_kernel") - w0 == 1, "walks of one call");
}

// a right pass to the end and a left pass over the whole chain, from label position l, in X and index form
static void passes(tnml_ctx *ctx, int N, int D, int L, int l, int b, int max_bond) {
  std::vector<float> X((size_t)b * N * D, 0.5f);
  std::vector<int32_t> y(b), idx(b);
  for (int s = 0; s < b; ++s) { y[s] = s % L; idx[s] = (s * 7) % b; }
  std::vector<double> S((size_t)D * D, 0.5), vals((size_t)N * 6);
  OK(tnml_dataset_attach(ctx, X.data(), y.data(), b, N, D, TNML_DATASET_FEATURES));
  if (l < N - 1) sweep_counted(ctx, X.data(), y.data(), nullptr, b, S.data(), 0, N - 1 - l, 1, max_bond, vals.data());
  sweep_counted(ctx, X.data(), nullptr, nullptr, b, nullptr, 1, N - 1, 0, max_bond, vals.data());
  sweep_counted(ctx, nullptr, y.data(), idx.data(), b, S.data(), 0, 2, 1, max_bond, vals.data());
  sweep_counted(ctx, nullptr, nullptr, idx.data(), b, nullptr, 0, N - 3, 1, max_bond, vals.data());          // a second call goes on
  int32_t bond[1024], lp = -1;
  OK(tnml_get_bonds(ctx, bond, &lp));
  CHECK(lp == N - 1, "l_pos %d after the passes", lp);
  for (int i = 0; i < N - 1; ++i) CHECK(bond[i] >= 1 && bond[i] <= max_bond, "bond %d is %d", i, bond[i]);
  size_t n = 0;
  std::vector<double> out((size_t)4 * max_bond * max_bond * D * D * L + 128);
  for (int what = TNML_NLL_SWEEP_B; what <= TNML_NLL_SWEEP_SIGMA; ++what) OK(tnml_nll_sweep_debug(ctx, what, out.data(), out.size(), &n));
  OK(tnml_dataset_detach(ctx));
}

static void run_test_shapes() {
  for (int N : {6, 9})
    for (int L : {2, 3})
      for (int l : {0, N / 2, N - 1})
        for (int b : {1, 17, 70}) {
          tnml_ctx *ctx = nullptr;
          OK(tnml_create(&ctx, N, 2, L, 16, 64, 0));
          std::vector<int> bw(N - 1);
          for (int i = 0; i < N - 1; ++i) bw[i] = 1 + (i * 7 + l * 3) % 4;
          Chain w(N, 2, L, bw, l);
          set_cores(ctx, w, l);
          passes(ctx, N, 2, L, l, b, 16);
          OK(tnml_destroy(ctx));
        }
  printf("planned likelihood sweeps at the test shapes: N 6 and 9, L 2 and 3, the label at both ends and inside, b 1 / 17 / 70\n");
  // the large-tensor path: N = 4, bond 40, short side 80
  tnml_ctx *ctx = nullptr;
  OK(tnml_create(&ctx, 4, 2, 2, 40, 64, 0));
  Chain w(4, 2, 2, std::vector<int>(3, 40), 1);
  set_cores(ctx, w, 1);
  std::vector<float> X((size_t)70 * 4 * 2, 0.5f);
  std::vector<int32_t> y(70, 1);
  double vals[12];
  const long big0 = san_stub_launches("big");
  OK(tnml_nll_sweep(ctx, X.data(), y.data(), 70, nullptr, 0, 2, 1e-2f, 1, 40, 1.0, vals));
  CHECK(san_stub_launches("big") > big0, "the 80 x 160 step did not take the large-tensor path");
  OK(tnml_destroy(ctx));
  printf("planned likelihood sweep on the large-tensor path: N 4, bond 40, short side 80\n");
  fflush(stdout);
}

static void run_true_size(const char *name, int L, int M) {
  const int N = 784, D = 2, b = 200;
  tnml_ctx *ctx = nullptr;
  OK(tnml_create(&ctx, N, D, L, M, 64, 0));
  Chain w(N, D, L, std::vector<int>(N - 1, M), 0);
  set_cores(ctx, w, 0);
  std::vector<float> X((size_t)b * N * D, 0.5f);
  std::vector<int32_t> y(b, 1);
  std::vector<double> vals((size_t)N * 6), S((size_t)D * D, 0.5);
  sweep_counted(ctx, X.data(), y.data(), nullptr, b, S.data(), 0, N - 1, 1, M, vals.data());
  sweep_counted(ctx, X.data(), nullptr, nullptr, b, S.data(), 1, N - 1, 1, M, vals.data());
  OK(tnml_destroy(ctx));
  printf("planned likelihood sweeps %s: N 784, bond %d, L %d, right and left\n", name, M, L);
  fflush(stdout);
}

static void run_refusals() {
  const int N = 6, D = 2, L = 3, M = 8, b = 5;
  tnml_ctx *ctx = nullptr;
  OK(tnml_create(&ctx, N, D, L, M, 64, 0));
  Chain w(N, D, L, std::vector<int>(N - 1, 4), 2);
  std::vector<float> X((size_t)b * N * D, 0.5f);
  std::vector<int32_t> y(b, 1), idx(b, 0);
  std::vector<double> S((size_t)D * D, 0.5);
  double v[6 * 8];
  size_t n = 0;
  FAILS_WITH(TNML_ERR_STATE, tnml_nll_sweep(ctx, X.data(), y.data(), b, nullptr, 0, 1, 1e-2f, 1, M, 1.0, v));          // cores never set
  set_cores(ctx, w, 2);
  FAILS_WITH(TNML_ERR_ARG, tnml_nll_sweep(nullptr, X.data(), y.data(), b, nullptr, 0, 1, 1e-2f, 1, M, 1.0, v));
  FAILS_WITH(TNML_ERR_ARG, tnml_nll_sweep(ctx, nullptr, y.data(), b, nullptr, 0, 1, 1e-2f, 1, M, 1.0, v));
  FAILS_WITH(TNML_ERR_ARG, tnml_nll_sweep(ctx, X.data(), y.data(), b, nullptr, 0, 1, 1e-2f, 1, M, 1.0, nullptr));
  FAILS_WITH(TNML_ERR_ARG, tnml_nll_sweep(ctx, X.data(), y.data(), 0, nullptr, 0, 1, 1e-2f, 1, M, 1.0, v));
  FAILS_WITH(TNML_ERR_ARG, tnml_nll_sweep(ctx, X.data(), y.data(), b, nullptr, 0, 1, 1e-2f, 2, M, 1.0, v));
  CHECK(strstr(tnml_last_error(), "renorm"), "the refusal does not say renorm: %s", tnml_last_error());
  FAILS_WITH(TNML_ERR_ARG, tnml_nll_sweep(ctx, X.data(), y.data(), b, nullptr, 0, 0, 1e-2f, 1, M, 1.0, v));
  FAILS_WITH(TNML_ERR_ARG, tnml_nll_sweep(ctx, X.data(), y.data(), b, nullptr, 0, 1, 1e-2f, 1, 0, 1.0, v));
  FAILS_WITH(TNML_ERR_ARG, tnml_nll_sweep(ctx, X.data(), y.data(), b, nullptr, 0, 1, 1e-2f, 1, M + 1, 1.0, v));
  CHECK(strstr(tnml_last_error(), "max_bond"), "the refusal does not say max_bond: %s", tnml_last_error());
  FAILS_WITH(TNML_ERR_ARG, tnml_nll_sweep(ctx, X.data(), y.data(), b, nullptr, 0, 1, 1e-2f, 1, M, 0.0, v));
  FAILS_WITH(TNML_ERR_ARG, tnml_nll_sweep(ctx, X.data(), y.data(), b, nullptr, 0, 1, 1e-2f, 1, M, 1.5, v));
  FAILS_WITH(TNML_ERR_ARG, tnml_nll_sweep(ctx, X.data(), y.data(), b, nullptr, 0, 1, 1e-2f, 1, M, NAN, v));
  FAILS_WITH(TNML_ERR_STATE, tnml_nll_sweep(ctx, X.data(), y.data(), b, nullptr, 0, 4, 1e-2f, 1, M, 1.0, v));          // three steps to the right end
  FAILS_WITH(TNML_ERR_STATE, tnml_nll_sweep(ctx, X.data(), y.data(), b, nullptr, 1, 3, 1e-2f, 1, M, 1.0, v));          // two to the left end
  y[3] = L;
  FAILS_WITH(TNML_ERR_ARG, tnml_nll_sweep(ctx, X.data(), y.data(), b, nullptr, 0, 1, 1e-2f, 1, M, 1.0, v));
  y[3] = 0;
  {
    std::vector<double> T(S);
    T[2] = 0.75;
    FAILS_WITH(TNML_ERR_ARG, tnml_nll_sweep(ctx, X.data(), y.data(), b, T.data(), 0, 1, 1e-2f, 1, M, 1.0, v));
    CHECK(strstr(tnml_last_error(), "symmetric"), "the refusal does not say symmetric: %s", tnml_last_error());
  }
  FAILS_WITH(TNML_ERR_STATE, tnml_nll_sweep_debug(ctx, TNML_NLL_SWEEP_B, v, 48, &n));                                   // no step has run
  FAILS_WITH(TNML_ERR_STATE, tnml_nll_sweep_indices(ctx, idx.data(), b, 1, nullptr, 0, 1, 1e-2f, 1, M, 1.0, v));       // no dataset
  OK(tnml_dataset_attach(ctx, X.data(), y.data(), b, N, D, TNML_DATASET_FEATURES));
  FAILS_WITH(TNML_ERR_ARG, tnml_nll_sweep_indices(ctx, nullptr, b, 1, nullptr, 0, 1, 1e-2f, 1, M, 1.0, v));
  FAILS_WITH(TNML_ERR_ARG, tnml_nll_sweep_indices(ctx, idx.data(), 0, 1, nullptr, 0, 1, 1e-2f, 1, M, 1.0, v));
  idx[2] = b;
  FAILS_WITH(TNML_ERR_ARG, tnml_nll_sweep_indices(ctx, idx.data(), b, 1, nullptr, 0, 1, 1e-2f, 1, M, 1.0, v));
  idx[2] = 0;
  OK(tnml_nll_sweep_indices(ctx, idx.data(), b, 1, S.data(), 0, 3, 1e-2f, 1, M, 1.0, v));                              // usable afterwards
  FAILS_WITH(TNML_ERR_ARG, tnml_nll_sweep_debug(ctx, 5, v, 48, &n));
  FAILS_WITH(TNML_ERR_ARG, tnml_nll_sweep_debug(ctx, TNML_NLL_SWEEP_B, v, 1, &n));
  OK(tnml_destroy(ctx));
  // D = 3 is refused
  OK(tnml_create(&ctx, 4, 3, 2, 4, 64, 0));
  Chain w3(4, 3, 2, std::vector<int>(3, 3), 0);
  set_cores(ctx, w3, 0);
  std::vector<float> X3((size_t)2 * 4 * 3, 0.5f);
  FAILS_WITH(TNML_ERR_ARG, tnml_nll_sweep(ctx, X3.data(), nullptr, 2, nullptr, 0, 1, 1e-2f, 1, 4, 1.0, v));
  OK(tnml_destroy(ctx));
  // bond 70 at L = 2 gives a merged matrix of 140 x 280: refused, and first of all as tnml_nll_grad refuses a bond above the norm walk's
  // 64 (with bonds up to 64 a short side cannot pass 128, so the call's own check of the short side is never the first to speak)
  OK(tnml_create(&ctx, 4, 2, 2, 70, 64, 0));
  Chain w70(4, 2, 2, std::vector<int>(3, 70), 1);
  set_cores(ctx, w70, 1);
  std::vector<float> X4((size_t)3 * 4 * 2, 0.5f);
  FAILS_WITH(TNML_ERR_ARG, tnml_nll_sweep(ctx, X4.data(), nullptr, 3, nullptr, 0, 1, 1e-2f, 1, 70, 1.0, v));
  OK(tnml_destroy(ctx));
  // with a communicator the call is refused
  setenv("TNML_FORCE_COMM", "1", 1);
  OK(tnml_create(&ctx, N, D, L, M, 64, 0));
  unsigned char uid[128];
  OK(tnml_comm_unique_id(uid));
  OK(tnml_comm_init(ctx, 0, 1, uid));
  Chain w0(N, D, L, std::vector<int>(N - 1, 4), 0);
  set_cores(ctx, w0, 0);
  FAILS_WITH(TNML_ERR_STATE, tnml_nll_sweep(ctx, X.data(), y.data(), b, nullptr, 0, 1, 1e-2f, 1, M, 1.0, v));
  FAILS_WITH(TNML_ERR_STATE, tnml_nll_sweep_indices(ctx, idx.data(), b, 1, nullptr, 0, 1, 1e-2f, 1, M, 1.0, v));
  OK(tnml_destroy(ctx));
  unsetenv("TNML_FORCE_COMM");
  printf("likelihood sweep refusals: ok (%d)\n", g_refusals);
}

// after a call: a sweep needs a forward, a stateful step needs tnml_optim_reset
static void run_state_rule() {
  const int N = 8, D = 2, L = 2, M = 8, b = 40;
  const int kAct = TNML_ACT_SOFTMAX, kLoss = TNML_LOSS_FULL_CROSS_ENT;
  tnml_ctx *ctx = nullptr;
  OK(tnml_create(&ctx, N, D, L, M, 64, 0));
  std::vector<float> X((size_t)b * N * D, 0.5f), f((size_t)L * b);
  std::vector<int> lab(b, 1);
  Chain w(N, D, L, std::vector<int>(N - 1, 2), 0);
  double v[6 * 8], met[3];
  set_cores(ctx, w, 0);
  OK(tnml_optim_config(ctx, TNML_OPT_SGD, 0.9, 0.9, 0.999, 1e-8, 0));
  OK(tnml_set_input(ctx, X.data(), lab.data(), b));
  OK(tnml_forward(ctx, f.data()));
  OK(tnml_gd_step(ctx, X.data(), lab.data(), b, 0.1f, 0.f, kAct, kLoss, 0.1f, met));
  OK(tnml_forward(ctx, f.data()));
  OK(tnml_nll_sweep(ctx, X.data(), lab.data(), b, nullptr, 0, N - 1, 1e-2f, 1, M, 1.0, v));
  FAILS_WITH(TNML_ERR_STATE, tnml_sweep(ctx, 1, 2, 1, 1e-3f, 1e-3f, 1, kAct, kLoss, 0.1f, TNML_TRUNC_FIXED, nullptr, nullptr));
  FAILS_WITH(TNML_ERR_STATE, tnml_gd_step(ctx, X.data(), lab.data(), b, 0.1f, 0.f, kAct, kLoss, 0.1f, met));
  CHECK(strstr(tnml_last_error(), "tnml_optim_reset"), "the refusal does not name the remedy: %s", tnml_last_error());
  OK(tnml_forward(ctx, f.data()));                               // (the resident batch is still there)
  OK(tnml_sweep(ctx, 1, 2, 1, 1e-3f, 1e-3f, 1, kAct, kLoss, 0.1f, TNML_TRUNC_FIXED, nullptr, nullptr));
  OK(tnml_optim_reset(ctx));
  OK(tnml_destroy(ctx));
  printf("state rules of the likelihood sweep: ok\n");
}

// every allocation of a call fails in turn, at the first site and with the label at every other site, and when the group grows
static void run_alloc_failures() {
  const int N = 6, D = 2, L = 2, M = 12, b = 70;
  std::vector<float> X((size_t)200 * N * D, 0.5f);
  std::vector<int32_t> y(200, 1);
  std::vector<double> vals((size_t)N * 6);
  for (int l = 0; l < N - 1; ++l) {
    tnml_ctx *ctx = nullptr;
    OK(tnml_create(&ctx, N, D, L, M, 64, 0));
    Chain w(N, D, L, std::vector<int>(N - 1, 3), l);
    set_cores(ctx, w, l);
    char what[64];
    snprintf(what, sizeof what, "tnml_nll_sweep, fresh, label on %d", l);
    int k = fail_each_alloc(what, [&] { return tnml_nll_sweep(ctx, X.data(), y.data(), b, nullptr, 0, 1, 1e-2f, 1, M, 1.0, vals.data()); });
    if (k < 16) { fprintf(stderr, "%d allocations failed in turn, the sweep's group alone has 16\n", k); exit(1); }
    int32_t bond[8], lp = -1;
    OK(tnml_get_bonds(ctx, bond, &lp));
    CHECK(lp == l + 1, "the failed calls moved the label: l_pos %d", lp);
    if (l + 1 < N - 1) {
      k = fail_each_alloc("tnml_nll_sweep, a larger batch", [&] { return tnml_nll_sweep(ctx, X.data(), y.data(), 200, nullptr, 0, 1, 1e-2f, 1, M, 1.0, vals.data()); });
      if (k < 16) { fprintf(stderr, "%d allocations failed in turn when the group grew\n", k); exit(1); }
    }
    OK(tnml_destroy(ctx));
  }
}

int main() {
  run_test_shapes();
  run_true_size("c3", 2, 20);
  run_true_size("c5", 10, 50);
  run_refusals();
  run_state_rule();
  run_alloc_failures();
  san_stub_report();
  printf("likelihood sweep host planning under ASan + UBSan: ok\n");
  return 0;
}
