// Samples and log-likelihoods (tnml_sample of tnml_api.hip and the launch wrapper of kernels_sample.hip) planned by the real host
// code, built --cuda-host-only with AddressSanitizer and UBSan, against the stand-in runtime of hip_stub.cpp, which reads the bond,
// slot and tile tables, the classes and the given levels of every launch as the kernels do and checks every core, environment,
// staging area, the grid, the uniforms and the outputs with their extents.  Nothing computes there: the outputs come back as the
// memory holds them.  `make san-sample` builds and runs it; tests/test_sample_host.py runs `make san-sample`.
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

struct Grid {
  std::vector<double> phi, w;
  Grid(int K, int D) : phi((size_t)K * D, 0.5), w((size_t)K, 1.0 / K) {}
};

// the arguments of one call and its outputs
struct Call {
  int n, N, n_given;
  std::vector<int32_t> classes, given, levels, labels;
  std::vector<double> u, logp;
  Call(int n_, int N_, int L, int K, int n_given_, int mix) : n(n_), N(N_), n_given(n_given_), classes((size_t)n_), given((size_t)n_ * n_given_ + 1),
      levels((size_t)n_ * N_), labels((size_t)n_), u((size_t)n_ * (N_ + 1), 0.25), logp((size_t)2 * n_) {
    // mix 0: all -1; 1: every class and -1 in turn; 2: one class only
    for (int s = 0; s < n; ++s) classes[s] = mix == 0 ? -1 : mix == 1 ? s % (L + 1) - 1 : L - 1;
    for (size_t e = 0; e < given.size(); ++e) given[e] = (int32_t)(e % K);
  }
  int run(tnml_ctx *ctx, const Grid &g, int K, bool with_u, bool null_classes = false) {
    return tnml_sample(ctx, n, K, g.phi.data(), g.w.data(), null_classes ? nullptr : classes.data(), n_given ? given.data() : nullptr, n_given,
                       with_u ? u.data() : nullptr, 7, levels.data(), labels.data(), logp.data());
  }
};

static void set_cores(tnml_ctx *ctx, const Chain &w, int l_pos) { OK(tnml_set_cores(ctx, w.flat.data(), w.flat.size(), w.bond.data(), l_pos)); }

// drawn and given classes, with and without a prefix, hashed and explicit uniforms, growing n: each call is one walk launch, one
// environment launch for the shared part and one for the slots unless the label sits on site 0
static void sample_calls(tnml_ctx *ctx, int N, int D, int L, int l_pos, int K) {
  Grid g(K, D);
  const long e0 = san_stub_launches("sample_env_kernel"), w0 = san_stub_launches("sample_walk_kernel");
  int calls = 0;
  for (int mix = 0; mix < 3; ++mix)
    for (int n_given : {0, N / 2, N}) {
      Call c(mix == 1 ? 40 : 16 + 17 * mix, N, L, K, n_given, mix);
      OK(c.run(ctx, g, K, (mix + n_given) % 2 == 0, mix == 0 && n_given == 0));
      ++calls;
    }
  Call one(1, N, L, K, 0, 2);
  OK(one.run(ctx, g, K, false));
  ++calls;
  CHECK(san_stub_launches("sample_walk_kernel") - w0 == calls, "%d calls did not make %d walk launches", calls, calls);
  CHECK(san_stub_launches("sample_env_kernel") - e0 == calls * (l_pos >= 1 ? 2 : 1), "%d calls made %ld environment launches", calls, san_stub_launches("sample_env_kernel") - e0);
}

static void run_true_size(const char *name, int N, int D, int L, int M, int l_pos) {
  tnml_ctx *ctx = nullptr;
  OK(tnml_create(&ctx, N, D, L, M, 64, 0));
  Chain w(N, D, L, std::vector<int>(N - 1, M), l_pos);
  set_cores(ctx, w, l_pos);
  sample_calls(ctx, N, D, L, l_pos, 256);
  OK(tnml_destroy(ctx));
  printf("planned samples %s bond %d L %d, label on %d\n", name, M, L, l_pos);
  fflush(stdout);
}

// a ragged chain at every label position (and N = 2), K = 2, 7 and 256 in turn
static void run_ragged(int N, int D, int L, int M) {
  tnml_ctx *ctx = nullptr;
  OK(tnml_create(&ctx, N, D, L, M, 64, 0));
  const int Ks[3] = {2, 7, 256};
  for (int l = 0; l < N; ++l) {
    std::vector<int> b(N - 1);
    for (int i = 0; i < N - 1; ++i) b[i] = 1 + (i * 7 + l * 3) % M;
    b[(l * 5) % (N - 1)] = M;
    Chain w(N, D, L, b, l);
    set_cores(ctx, w, l);
    sample_calls(ctx, N, D, L, l, Ks[l % 3]);
  }
  OK(tnml_destroy(ctx));
  printf("planned samples ragged N %d D %d L %d bonds <= %d at every label position\n", N, D, L, M);
  fflush(stdout);
}

static void run_refusals() {
  const int N = 6, D = 2, L = 3, M = 4, K = 5, n = 20;
  tnml_ctx *ctx = nullptr;
  OK(tnml_create(&ctx, N, D, L, M, 64, 0));
  Chain w(N, D, L, std::vector<int>(N - 1, M), 2);
  Grid g(K, D);
  Call c(n, N, L, K, 3, 1);
  const double *ph = g.phi.data(), *wt = g.w.data(), *u = c.u.data();
  const int32_t *cl = c.classes.data(), *gv = c.given.data();
  int32_t *lv = c.levels.data(), *lb = c.labels.data();
  double *lp = c.logp.data();
  FAILS_WITH(TNML_ERR_STATE, tnml_sample(ctx, n, K, ph, wt, cl, gv, 3, u, 0, lv, lb, lp));                    // cores never set
  set_cores(ctx, w, 2);
  auto unchanged = [&] {
    std::vector<float> back(w.flat.size());
    std::vector<int32_t> bg(N - 1);
    int lpos = -1;
    OK(tnml_get_cores(ctx, back.data(), back.size(), bg.data(), &lpos));
    CHECK(lpos == 2 && bg == w.bond && back == w.flat, "a refused call changed the chain");
  };
  FAILS_WITH(TNML_ERR_ARG, tnml_sample(nullptr, n, K, ph, wt, cl, gv, 3, u, 0, lv, lb, lp));
  FAILS_WITH(TNML_ERR_ARG, tnml_sample(ctx, 0, K, ph, wt, cl, gv, 3, u, 0, lv, lb, lp));
  FAILS_WITH(TNML_ERR_ARG, tnml_sample(ctx, -3, K, ph, wt, cl, gv, 3, u, 0, lv, lb, lp));
  FAILS_WITH(TNML_ERR_ARG, tnml_sample(ctx, n, 1, ph, wt, cl, gv, 3, u, 0, lv, lb, lp));
  FAILS_WITH(TNML_ERR_ARG, tnml_sample(ctx, n, 257, ph, wt, cl, gv, 3, u, 0, lv, lb, lp));
  FAILS_WITH(TNML_ERR_ARG, tnml_sample(ctx, n, K, nullptr, wt, cl, gv, 3, u, 0, lv, lb, lp));
  FAILS_WITH(TNML_ERR_ARG, tnml_sample(ctx, n, K, ph, nullptr, cl, gv, 3, u, 0, lv, lb, lp));
  FAILS_WITH(TNML_ERR_ARG, tnml_sample(ctx, n, K, ph, wt, cl, gv, -1, u, 0, lv, lb, lp));
  FAILS_WITH(TNML_ERR_ARG, tnml_sample(ctx, n, K, ph, wt, cl, gv, N + 1, u, 0, lv, lb, lp));
  FAILS_WITH(TNML_ERR_ARG, tnml_sample(ctx, n, K, ph, wt, cl, nullptr, 3, u, 0, lv, lb, lp));
  FAILS_WITH(TNML_ERR_ARG, tnml_sample(ctx, n, K, ph, wt, cl, gv, 3, u, 0, nullptr, lb, lp));
  FAILS_WITH(TNML_ERR_ARG, tnml_sample(ctx, n, K, ph, wt, cl, gv, 3, u, 0, lv, nullptr, lp));
  FAILS_WITH(TNML_ERR_ARG, tnml_sample(ctx, n, K, ph, wt, cl, gv, 3, u, 0, lv, lb, nullptr));
  {
    std::vector<int32_t> bad(c.classes);
    bad[n - 1] = L;
    FAILS_WITH(TNML_ERR_ARG, tnml_sample(ctx, n, K, ph, wt, bad.data(), gv, 3, u, 0, lv, lb, lp));
    bad[n - 1] = -2;
    FAILS_WITH(TNML_ERR_ARG, tnml_sample(ctx, n, K, ph, wt, bad.data(), gv, 3, u, 0, lv, lb, lp));
    std::vector<int32_t> bg(c.given);
    bg[3 * n - 1] = K;
    FAILS_WITH(TNML_ERR_ARG, tnml_sample(ctx, n, K, ph, wt, cl, bg.data(), 3, u, 0, lv, lb, lp));
    bg[3 * n - 1] = -1;
    FAILS_WITH(TNML_ERR_ARG, tnml_sample(ctx, n, K, ph, wt, cl, bg.data(), 3, u, 0, lv, lb, lp));
    for (double v : {0.0, -1.0, (double)NAN, (double)INFINITY}) {
      std::vector<double> bw(g.w);
      bw[K - 1] = v;
      FAILS_WITH(TNML_ERR_ARG, tnml_sample(ctx, n, K, ph, bw.data(), cl, gv, 3, u, 0, lv, lb, lp));
    }
    std::vector<double> bp(g.phi);
    bp[K * D - 1] = NAN;
    FAILS_WITH(TNML_ERR_ARG, tnml_sample(ctx, n, K, bp.data(), wt, cl, gv, 3, u, 0, lv, lb, lp));
    for (double v : {1.0, -0.5, (double)NAN}) {
      std::vector<double> bu(c.u);
      bu[(size_t)n * (N + 1) - 1] = v;
      FAILS_WITH(TNML_ERR_ARG, tnml_sample(ctx, n, K, ph, wt, cl, gv, 3, bu.data(), 0, lv, lb, lp));
    }
  }
  unchanged();
  OK(tnml_sample(ctx, n, K, ph, wt, cl, gv, 3, u, 0, lv, lb, lp));                                            // usable afterwards
  OK(tnml_destroy(ctx));
  // a bond the kernels have no room for: refused with the bytes in the message; bond 64 is the largest they take
  OK(tnml_create(&ctx, 4, 2, 2, 128, 64, 0));
  Chain big(4, 2, 2, std::vector<int>{2, 65, 2}, 0), fits(4, 2, 2, std::vector<int>{2, 64, 2}, 0);
  Grid g2(256, 2);
  Call c2(n, 4, 2, 256, 0, 1);
  set_cores(ctx, big, 0);
  FAILS_WITH(TNML_ERR_SHAPE, c2.run(ctx, g2, 256, true));
  if (!strstr(tnml_last_error(), "bytes of LDS")) { fprintf(stderr, "LDS refusal does not name the bytes: %s\n", tnml_last_error()); exit(1); }
  set_cores(ctx, fits, 0);
  OK(c2.run(ctx, g2, 256, true));
  OK(tnml_destroy(ctx));
  // D = 8 at bond 16 with L = 10 and K = 256 fits
  OK(tnml_create(&ctx, 5, 8, 10, 16, 64, 0));
  Chain d8(5, 8, 10, std::vector<int>(4, 16), 2);
  Grid g3(256, 8);
  Call c3(n, 5, 10, 256, 2, 1);
  set_cores(ctx, d8, 2);
  OK(c3.run(ctx, g3, 256, false));
  OK(tnml_destroy(ctx));
  // with a communicator the call is refused
  setenv("TNML_FORCE_COMM", "1", 1);
  OK(tnml_create(&ctx, N, D, L, M, 64, 0));
  unsigned char uid[128];
  OK(tnml_comm_unique_id(uid));
  OK(tnml_comm_init(ctx, 0, 1, uid));
  Chain w0(N, D, L, std::vector<int>(N - 1, M), 0);
  set_cores(ctx, w0, 0);
  FAILS_WITH(TNML_ERR_STATE, tnml_sample(ctx, n, K, ph, wt, cl, gv, 3, u, 0, lv, lb, lp));
  OK(tnml_destroy(ctx));
  unsetenv("TNML_FORCE_COMM");
  printf("sample refusals: ok\n");
}

// tnml_sample leaves everything as it was: no new forward before a sweep, the optimiser state stays bound
static void run_state_rule() {
  const int N = 8, D = 2, L = 2, M = 6, b = 40, K = 7;
  tnml_ctx *ctx = nullptr;
  OK(tnml_create(&ctx, N, D, L, M, 64, 0));
  std::vector<float> X((size_t)b * N * D, 0.5f), f((size_t)L * b);
  std::vector<int> lab(b, 1);
  Chain w(N, D, L, std::vector<int>(N - 1, 2), 0);
  Grid g(K, D);
  Call c(24, N, L, K, 0, 1);
  double met[3];
  set_cores(ctx, w, 0);
  OK(tnml_optim_config(ctx, TNML_OPT_SGD, 0.9, 0.9, 0.999, 1e-8, 0));
  OK(tnml_gd_step(ctx, X.data(), lab.data(), b, 0.1f, 0.f, TNML_ACT_SOFTMAX, TNML_LOSS_FULL_CROSS_ENT, 0.1f, met));
  OK(tnml_set_input(ctx, X.data(), lab.data(), b));
  OK(tnml_forward(ctx, f.data()));
  OK(c.run(ctx, g, K, false));
  OK(tnml_gd_step(ctx, X.data(), lab.data(), b, 0.1f, 0.f, TNML_ACT_SOFTMAX, TNML_LOSS_FULL_CROSS_ENT, 0.1f, met));   // the state is still bound
  OK(tnml_forward(ctx, f.data()));
  OK(c.run(ctx, g, K, true));
  OK(tnml_sweep(ctx, 0, 2, 1, 1e-3f, 1e-3f, 1, TNML_ACT_SOFTMAX, TNML_LOSS_FULL_CROSS_ENT, 0.1f, TNML_TRUNC_FIXED, nullptr, nullptr));
  OK(tnml_destroy(ctx));
  printf("state rule after tnml_sample: ok\n");
}

// every allocation of the new group fails in turn, on first use and whenever a call makes it grow
static void run_alloc_failures(int D) {
  const int N = 6, L = 3, M = 12, K = 7;
  tnml_ctx *ctx = nullptr;
  OK(tnml_create(&ctx, N, D, L, M, 64, 0));
  Chain w(N, D, L, std::vector<int>(N - 1, 3), 3), w5(N, D, L, std::vector<int>(N - 1, 5), 3);
  Grid g(K, D);
  set_cores(ctx, w, 3);
  Call small(10, N, L, K, 0, 2), more(100, N, L, K, 2, 1);
  int k = fail_each_alloc("tnml_sample, fresh context", [&] { return small.run(ctx, g, K, false); });
  if (k != 17) { fprintf(stderr, "%d allocations failed in turn, the group has 17\n", k); exit(1); }
  k = fail_each_alloc("tnml_sample, the group exists", [&] { return small.run(ctx, g, K, false); });
  if (k != 0) { fprintf(stderr, "%d allocations in a second call\n", k); exit(1); }
  k = fail_each_alloc("tnml_sample, more samples, slots, a prefix and uniforms", [&] { return more.run(ctx, g, K, true); });
  if (k != 17) { fprintf(stderr, "%d allocations failed in turn when the group grew, it has 17\n", k); exit(1); }
  set_cores(ctx, w5, 3);
  k = fail_each_alloc("tnml_sample, a larger bond", [&] { return small.run(ctx, g, K, false); });
  if (k != 17) { fprintf(stderr, "%d allocations failed in turn when the bond grew, the group has 17\n", k); exit(1); }
  OK(more.run(ctx, g, K, true));
  OK(tnml_destroy(ctx));
}

int main() {
  run_true_size("c3", 784, 2, 2, 20, 0);
  run_true_size("c3 last", 784, 2, 2, 20, 783);
  run_true_size("c3 inner label", 784, 2, 2, 20, 391);
  run_true_size("c5", 784, 2, 10, 50, 783);
  run_true_size("c5 first", 784, 2, 10, 50, 0);
  run_true_size("c5 inner label", 784, 2, 10, 50, 400);
  run_ragged(17, 2, 3, 7);
  run_ragged(17, 3, 3, 7);
  run_ragged(17, 8, 17, 6);
  run_ragged(2, 2, 2, 5);
  run_ragged(2, 8, 10, 3);
  run_refusals();
  run_state_rule();
  run_alloc_failures(2);
  run_alloc_failures(3);
  san_stub_report();
  const char *paths[] = {"sample_env_kernel", "sample_walk_kernel"};
  for (const char *k : paths)
    if (san_stub_launches(k) < 1) { fprintf(stderr, "launch path %s was never taken\n", k); return 1; }
  printf("sample: %ld sample_env_kernel and %ld sample_walk_kernel launches checked, %d refusals\n", san_stub_launches("sample_env_kernel"),
         san_stub_launches("sample_walk_kernel"), g_refusals);
  printf("sample host planning under ASan + UBSan: ok\n");
  return 0;
}
