// Per-pixel conditionals (tnml_site_conditionals of tnml_api.hip, the front it shares with tnml_sample_masked, and the launch wrapper
// of kernels_site_cond.hip) planned by the real host code, built --cuda-host-only with AddressSanitizer and UBSan, against the
// stand-in runtime of hip_stub.cpp, which checks the environment launch as it does for the sampler -- held to THIS call's tile --
// and the site_cond_kernel launch behind it: the same block, the values, the left environments and the outputs with their extents,
// grid, block and LDS.  Nothing computes there: the outputs come back as the memory holds them.  `make san-site-cond` builds and
// runs it; tests/test_site_cond_host.py runs `make san-site-cond`.
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
extern "C" void san_stub_masked_reset(void);
extern "C" void san_stub_masked_check(int walk, int n, const int32_t *classes);
extern "C" void san_stub_site_cond_call(int on);

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
  std::vector<double> phi, w, values;
  Grid(int K, int D) : phi((size_t)K * D, 0.5), w((size_t)K, 1.0 / K), values((size_t)K, 0.25) {}
};

enum Out { kQ = 1, kStats = 2, kMode = 4, kLogp = 8, kAll = 15 };

// the arguments of one call and its outputs; per-sample masks shift their kind (empty, full, prefix, suffix, alternating) from row to row
struct Call {
  int n, N, L, mask_rows;
  std::vector<int32_t> classes, known, mode;
  std::vector<uint8_t> mask;
  std::vector<double> q, stats, logp;
  Call(int n_, int N_, int D, int L_, int K, int mix, int kind, bool per_sample) : n(n_), N(N_), L(L_), mask_rows(per_sample ? n_ : 1), classes((size_t)n_),
      known((size_t)n_ * N_), mode((size_t)n_ * N_), mask((size_t)(per_sample ? n_ : 1) * N_), q((size_t)n_ * N_ * D * D), stats((size_t)n_ * N_ * 4),
      logp((size_t)n_) {
    for (int s = 0; s < n; ++s) classes[s] = mix == 0 ? -1 : mix == 1 ? s % (L + 1) - 1 : L - 1;
    for (int r = 0; r < mask_rows; ++r)
      for (int i = 0; i < N; ++i) {
        const int k = (kind + r) % 5;
        mask[(size_t)r * N + i] = k == 0 ? 0 : k == 1 ? 1 : k == 2 ? i < N / 2 : k == 3 ? i >= N / 2 : i % 2;
      }
    for (int s = 0; s < n; ++s)
      for (int i = 0; i < N; ++i) known[(size_t)s * N + i] = mask[(size_t)(per_sample ? s : 0) * N + i] ? (int32_t)((s + i) % K) : -7;
  }
  int run(tnml_ctx *ctx, const Grid &g, int K, int outs = kAll, bool with_values = true, bool null_classes = false) {
    san_stub_masked_reset();
    san_stub_site_cond_call(1);
    const int rc = tnml_site_conditionals(ctx, n, K, g.phi.data(), g.w.data(), with_values ? g.values.data() : nullptr, null_classes ? nullptr : classes.data(),
                                          mask.data(), mask_rows, known.data(), outs & kQ ? q.data() : nullptr, outs & kStats ? stats.data() : nullptr,
                                          outs & kMode ? mode.data() : nullptr, outs & kLogp ? logp.data() : nullptr);
    san_stub_site_cond_call(0);
    if (rc == TNML_OK) san_stub_masked_check(0, n, null_classes ? nullptr : classes.data());
    return rc;
  }
};

static void set_cores(tnml_ctx *ctx, const Chain &w, int l_pos) { OK(tnml_set_cores(ctx, w.flat.data(), w.flat.size(), w.bond.data(), l_pos)); }

// shared and per-sample masks of every kind, summed and given classes, every output NULL in turn and alone: every chunk is one
// environment launch and, unless logp_out is the only output, one site_cond_kernel launch behind it; never a walk of the sampler
static void calls(tnml_ctx *ctx, int N, int D, int L, int K, size_t budget) {
  Grid g(K, D);
  OK(tnml_set_sample_stack_bytes(ctx, budget));
  const int outs[9] = {kAll, kAll & ~kQ, kAll & ~kStats, kAll & ~kMode, kAll & ~kLogp, kQ, kStats, kMode, kLogp};
  int idx = 0;
  for (int mix = 0; mix < 3; ++mix)
    for (int kind = 0; kind < 5; ++kind, ++idx) {
      const long e0 = san_stub_launches("sample_env_masked_kernel"), s0 = san_stub_launches("site_cond_kernel"), w0 = san_stub_launches("sample_walk_masked_kernel");
      Call c(mix == 1 ? 40 : 16 + 17 * mix, N, D, L, K, mix, kind, idx % 2 == 1);
      const int o = outs[idx % 9];
      OK(c.run(ctx, g, K, o, idx % 3 != 0, mix == 0 && kind == 0));
      const long e = san_stub_launches("sample_env_masked_kernel") - e0, s = san_stub_launches("site_cond_kernel") - s0;
      CHECK(e >= 1 && s == (o == kLogp ? 0 : e) && san_stub_launches("sample_walk_masked_kernel") == w0,
            "a call with outputs %d made %ld environment and %ld site_cond launches", o, e, s);
    }
  Call one(1, N, D, L, K, 2, 4, false);
  OK(one.run(ctx, g, K));
  OK(tnml_set_sample_stack_bytes(ctx, (size_t)1 << 30));
}

static void run_true_size(const char *name, int N, int D, int L, int M, int l_pos) {
  tnml_ctx *ctx = nullptr;
  OK(tnml_create(&ctx, N, D, L, M, 64, 0));
  Chain w(N, D, L, std::vector<int>(N - 1, M), l_pos);
  set_cores(ctx, w, l_pos);
  calls(ctx, N, D, L, 256, (size_t)1 << 30);
  // a budget of one tile of this call: one chunk a tile
  const int T = tnml::site_cond_tile(M, D, L, 256);
  CHECK(T >= 1, "no tile at bond %d", M);
  const long e0 = san_stub_launches("sample_env_masked_kernel");
  calls(ctx, N, D, L, 256, (size_t)T * (N + 1) * M * M * sizeof(double));
  CHECK(san_stub_launches("sample_env_masked_kernel") - e0 > 16, "a budget of one tile did not split the calls into chunks");
  OK(tnml_destroy(ctx));
  printf("planned site conditionals %s bond %d L %d, label on %d, tiles of %d\n", name, M, L, l_pos, T);
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
    calls(ctx, N, D, L, Ks[l % 3], l % 2 ? (size_t)1 << 30 : (size_t)2 * 16 * (N + 1) * M * M * sizeof(double));
  }
  OK(tnml_destroy(ctx));
  printf("planned site conditionals ragged N %d D %d L %d bonds <= %d at every label position\n", N, D, L, M);
  fflush(stdout);
}

static void run_refusals() {
  const int N = 6, D = 2, L = 3, M = 4, K = 5, n = 20;
  tnml_ctx *ctx = nullptr;
  OK(tnml_create(&ctx, N, D, L, M, 64, 0));
  Chain w(N, D, L, std::vector<int>(N - 1, M), 2);
  Grid g(K, D);
  Call c(n, N, D, L, K, 1, 4, true);
  const double *ph = g.phi.data(), *wt = g.w.data(), *va = g.values.data();
  const int32_t *cl = c.classes.data(), *kn = c.known.data();
  const uint8_t *mk = c.mask.data();
  double *q = c.q.data(), *st = c.stats.data(), *lp = c.logp.data();
  int32_t *mo = c.mode.data();
  FAILS_WITH(TNML_ERR_STATE, tnml_site_conditionals(ctx, n, K, ph, wt, va, cl, mk, n, kn, q, st, mo, lp));                 // cores never set
  set_cores(ctx, w, 2);
  FAILS_WITH(TNML_ERR_ARG, tnml_site_conditionals(nullptr, n, K, ph, wt, va, cl, mk, n, kn, q, st, mo, lp));
  FAILS_WITH(TNML_ERR_ARG, tnml_site_conditionals(ctx, n, K, ph, wt, va, cl, mk, n, kn, nullptr, nullptr, nullptr, nullptr)); // every output NULL
  FAILS_WITH(TNML_ERR_ARG, tnml_site_conditionals(ctx, 0, K, ph, wt, va, cl, mk, n, kn, q, st, mo, lp));
  FAILS_WITH(TNML_ERR_ARG, tnml_site_conditionals(ctx, n, 1, ph, wt, va, cl, mk, n, kn, q, st, mo, lp));
  FAILS_WITH(TNML_ERR_ARG, tnml_site_conditionals(ctx, n, 257, ph, wt, va, cl, mk, n, kn, q, st, mo, lp));
  FAILS_WITH(TNML_ERR_ARG, tnml_site_conditionals(ctx, n, K, nullptr, wt, va, cl, mk, n, kn, q, st, mo, lp));
  FAILS_WITH(TNML_ERR_ARG, tnml_site_conditionals(ctx, n, K, ph, nullptr, va, cl, mk, n, kn, q, st, mo, lp));
  FAILS_WITH(TNML_ERR_ARG, tnml_site_conditionals(ctx, n, K, ph, wt, va, cl, mk, 2, kn, q, st, mo, lp));                   // mask_rows
  FAILS_WITH(TNML_ERR_ARG, tnml_site_conditionals(ctx, n, K, ph, wt, va, cl, nullptr, n, kn, q, st, mo, lp));              // NULL mask
  FAILS_WITH(TNML_ERR_ARG, tnml_site_conditionals(ctx, n, K, ph, wt, va, cl, mk, n, nullptr, q, st, mo, lp));              // NULL known, bits set
  {
    std::vector<int32_t> bad(c.classes);
    bad[n - 1] = L;
    FAILS_WITH(TNML_ERR_ARG, tnml_site_conditionals(ctx, n, K, ph, wt, va, bad.data(), mk, n, kn, q, st, mo, lp));
    size_t at = 0;
    for (size_t e = 0; e < c.mask.size(); ++e)
      if (c.mask[e]) at = e;
    std::vector<int32_t> bk(c.known);
    bk[at] = K;
    FAILS_WITH(TNML_ERR_ARG, tnml_site_conditionals(ctx, n, K, ph, wt, va, cl, mk, n, bk.data(), q, st, mo, lp));
    std::vector<double> bw(g.w), bp(g.phi);
    bw[K - 1] = 0.0;
    bp[K * D - 1] = NAN;
    FAILS_WITH(TNML_ERR_ARG, tnml_site_conditionals(ctx, n, K, ph, bw.data(), va, cl, mk, n, kn, q, st, mo, lp));
    FAILS_WITH(TNML_ERR_ARG, tnml_site_conditionals(ctx, n, K, bp.data(), wt, va, cl, mk, n, kn, q, st, mo, lp));
    for (double v : {(double)NAN, (double)INFINITY, -(double)INFINITY}) {                                                   // a value that is not finite
      std::vector<double> bv(g.values);
      bv[K - 1] = v;
      FAILS_WITH(TNML_ERR_ARG, tnml_site_conditionals(ctx, n, K, ph, wt, bv.data(), cl, mk, n, kn, q, st, mo, lp));
    }
  }
  OK(tnml_set_sample_stack_bytes(ctx, 64));                                                                                // a budget below one tile's need
  FAILS_WITH(TNML_ERR_ARG, tnml_site_conditionals(ctx, n, K, ph, wt, va, cl, mk, n, kn, q, st, mo, lp));
  OK(tnml_set_sample_stack_bytes(ctx, (size_t)1 << 30));
  OK(c.run(ctx, g, K));                                                                                                    // usable afterwards
  OK(tnml_destroy(ctx));
  // the bond limit: kSccMaxBond is taken, one more is refused with the bytes in the message
  OK(tnml_create(&ctx, 4, 2, 2, 128, 64, 0));
  Chain big(4, 2, 2, std::vector<int>{2, tnml::kSccMaxBond + 1, 2}, 0), fits(4, 2, 2, std::vector<int>{2, tnml::kSccMaxBond, 2}, 0);
  Grid g2(256, 2);
  Call c2(n, 4, 2, 2, 256, 1, 3, true);
  set_cores(ctx, big, 0);
  FAILS_WITH(TNML_ERR_SHAPE, c2.run(ctx, g2, 256));
  if (!strstr(tnml_last_error(), "bytes of LDS")) { fprintf(stderr, "LDS refusal does not name the bytes: %s\n", tnml_last_error()); exit(1); }
  set_cores(ctx, fits, 0);
  OK(c2.run(ctx, g2, 256));
  OK(tnml_destroy(ctx));
  // D = 8 at bond 16 with L = 10 and K = 256 fits
  OK(tnml_create(&ctx, 5, 8, 10, 16, 64, 0));
  Chain d8(5, 8, 10, std::vector<int>(4, 16), 2);
  Grid g3(256, 8);
  Call c3(n, 5, 8, 10, 256, 1, 2, true);
  set_cores(ctx, d8, 2);
  OK(c3.run(ctx, g3, 256));
  OK(tnml_destroy(ctx));
  // with a communicator the call is refused
  setenv("TNML_FORCE_COMM", "1", 1);
  OK(tnml_create(&ctx, N, D, L, M, 64, 0));
  unsigned char uid[128];
  OK(tnml_comm_unique_id(uid));
  OK(tnml_comm_init(ctx, 0, 1, uid));
  Chain w0(N, D, L, std::vector<int>(N - 1, M), 0);
  set_cores(ctx, w0, 0);
  FAILS_WITH(TNML_ERR_STATE, tnml_site_conditionals(ctx, n, K, ph, wt, va, cl, mk, n, kn, q, st, mo, lp));
  OK(tnml_destroy(ctx));
  unsetenv("TNML_FORCE_COMM");
  printf("site conditionals refusals: ok\n");
}

// every allocation of the new group fails in turn, fresh and at growth; the masked group, which the sampler creates first here, is
// the sampler's own and is failed in turn by san/plan_masked
static void run_alloc_failures(int D) {
  const int N = 6, L = 3, M = 12, K = 7, members = 5;
  tnml_ctx *ctx = nullptr;
  OK(tnml_create(&ctx, N, D, L, M, 64, 0));
  Chain w(N, D, L, std::vector<int>(N - 1, 3), 3);
  Grid g(K, D);
  set_cores(ctx, w, 3);
  Call small(10, N, D, L, K, 2, 2, false), more(100, N, D, L, K, 1, 4, true);
  {
    std::vector<int32_t> lv((size_t)more.n * N), lb((size_t)more.n);
    std::vector<double> lp((size_t)2 * more.n);
    OK(tnml_sample_masked(ctx, more.n, K, g.phi.data(), g.w.data(), more.classes.data(), more.mask.data(), more.mask_rows, more.known.data(), nullptr, 1, 1,
                          lv.data(), lb.data(), lp.data(), nullptr));
  }
  auto grows = [&](const char *what, Call &c, int want) {
    const int k = fail_each_alloc(what, [&] { return c.run(ctx, g, K); });
    if (k != want) { fprintf(stderr, "%s: %d allocations failed in turn, expected %d\n", what, k, want); exit(1); }
  };
  grows("tnml_site_conditionals, its group is new", small, members);
  grows("tnml_site_conditionals, the group exists", small, 0);
  grows("tnml_site_conditionals, more samples and tiles", more, members);
  OK(tnml_destroy(ctx));
  // both groups new: the masked group's fifteen, then the first of the new group
  OK(tnml_create(&ctx, N, D, L, M, 64, 0));
  set_cores(ctx, w, 3);
  grows("tnml_site_conditionals, fresh context", small, 16);
  OK(tnml_destroy(ctx));
}

int main() {
  run_true_size("c3", 784, 2, 2, 20, 0);
  run_true_size("c3 inner label", 784, 2, 2, 20, 391);
  run_true_size("c5", 784, 2, 10, 50, 783);
  run_true_size("c5 inner label", 784, 2, 10, 50, 400);
  run_ragged(17, 2, 3, 7);
  run_ragged(17, 3, 3, 7);
  run_ragged(17, 8, 17, 6);
  run_ragged(2, 2, 2, 5);
  run_refusals();
  run_alloc_failures(2);
  run_alloc_failures(3);
  san_stub_report();
  if (san_stub_launches("site_cond_kernel") < 1) { fprintf(stderr, "launch path site_cond_kernel was never taken\n"); return 1; }
  printf("site conditionals: %ld sample_env_masked_kernel and %ld site_cond_kernel launches checked, %d refusals\n",
         san_stub_launches("sample_env_masked_kernel"), san_stub_launches("site_cond_kernel"), g_refusals);
  printf("site conditionals host planning under ASan + UBSan: ok\n");
  return 0;
}
