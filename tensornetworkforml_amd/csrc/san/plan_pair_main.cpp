// Pixel-pair marginals (tnml_pair_marginals of tnml_api.hip and the launch wrappers of kernels_pair.hip) planned by the real host
// code, built --cuda-host-only with AddressSanitizer and UBSan, against the stand-in runtime of hip_stub.cpp, which checks the
// environment launch with its class slot and the three launches behind it: the same block, the grid, B, the chunk's rows (distinct,
// ascending) and every output with its extent, grid, block and LDS.  Nothing computes there: the outputs come back as the memory
// holds them.  `make san-pair` builds and runs it; tests/test_pair_host.py runs `make san-pair`.
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
  std::vector<double> phi, w, values;
  Grid(int K, int D) : phi((size_t)K * D, 0.5), w((size_t)K, 1.0 / K), values((size_t)K, 0.25) {}
};

enum Out { kQ1 = 1, kStats1 = 2, kQ = 4, kStats = 8, kAll = 15 };

static size_t row_bytes(int N, int D) { return (size_t)N * ((size_t)D * D * D * D * 8 + (size_t)D * D * 4 + 3 * 8); }

// the rows of one call (kind 0: all sites in descending order, 1: every third, 2: the last site alone, 3: none) and its outputs
struct Call {
  int N, D;
  std::vector<int32_t> rows;
  std::vector<double> q1, stats1, q, stats;
  Call(int N_, int D_, int kind) : N(N_), D(D_), q1((size_t)N_ * D_ * D_), stats1((size_t)N_ * 3) {
    if (kind == 0) for (int i = N - 1; i >= 0; --i) rows.push_back(i);
    if (kind == 1) for (int i = 1; i < N; i += 3) rows.push_back(i);
    if (kind == 2) rows.push_back(N - 1);
    q.resize(rows.size() * N * D * D * D * D);
    stats.resize(rows.size() * N * 3);
  }
  int run(tnml_ctx *ctx, const Grid &g, int K, int slot, int outs = kAll, bool with_values = true) {
    return tnml_pair_marginals(ctx, K, g.phi.data(), g.w.data(), with_values ? g.values.data() : nullptr, slot, rows.empty() ? nullptr : rows.data(),
                               (int)rows.size(), outs & kQ1 ? q1.data() : nullptr, outs & kStats1 ? stats1.data() : nullptr,
                               outs & kQ && !rows.empty() ? q.data() : nullptr, outs & kStats && !rows.empty() ? stats.data() : nullptr);
  }
};

static void set_cores(tnml_ctx *ctx, const Chain &w, int l_pos) { OK(tnml_set_cores(ctx, w.flat.data(), w.flat.size(), w.bond.data(), l_pos)); }

// every kind of rows, the label summed and every class in turn, every output NULL in turn and alone: a call is one environment and one
// per-site launch, and a walk and a statistics launch per chunk where a pair output is asked for
static void calls(tnml_ctx *ctx, int N, int D, int L, int K, size_t budget) {
  Grid g(K, D);
  OK(tnml_set_sample_stack_bytes(ctx, budget));
  const int outs[9] = {kAll, kAll & ~kQ1, kAll & ~kStats1, kAll & ~kQ, kAll & ~kStats, kQ1, kStats1, kQ, kStats};
  int idx = 0;
  for (int kind = 0; kind < 4; ++kind)
    for (int o = 0; o < 9; ++o, ++idx) {
      Call c(N, D, kind);
      const bool pairs = !c.rows.empty() && (outs[o] & (kQ | kStats));
      if (!pairs && !(outs[o] & (kQ1 | kStats1))) continue;        // (refused: run_refusals)
      const long e0 = san_stub_launches("lognorm_env_kernel"), c0 = san_stub_launches("pair_close_kernel"), w0 = san_stub_launches("pair_walk_kernel"),
                 s0 = san_stub_launches("pair_stats_kernel");
      OK(c.run(ctx, g, K, idx % (L + 1) - 1, outs[o], idx % 3 != 0));
      const long e = san_stub_launches("lognorm_env_kernel") - e0, cl = san_stub_launches("pair_close_kernel") - c0,
                 wk = san_stub_launches("pair_walk_kernel") - w0, st = san_stub_launches("pair_stats_kernel") - s0;
      const size_t per = budget / row_bytes(N, D) < c.rows.size() ? budget / row_bytes(N, D) : c.rows.size();
      const long chunks = pairs ? (long)((c.rows.size() + per - 1) / per) : 0;
      CHECK(e == 1 && cl == 1 && wk == chunks && st == chunks, "a call with outputs %d and %zu rows made %ld, %ld, %ld, %ld launches (%ld chunks)", outs[o],
            c.rows.size(), e, cl, wk, st, chunks);
    }
  OK(tnml_set_sample_stack_bytes(ctx, (size_t)1 << 30));
}

static void run_true_size(const char *name, int N, int D, int L, int M, int l_pos) {
  tnml_ctx *ctx = nullptr;
  OK(tnml_create(&ctx, N, D, L, M, 64, 0));
  Chain w(N, D, L, std::vector<int>(N - 1, M), l_pos);
  set_cores(ctx, w, l_pos);
  calls(ctx, N, D, L, 256, (size_t)1 << 30);
  const long w0 = san_stub_launches("pair_walk_kernel");
  calls(ctx, N, D, L, 256, row_bytes(N, D));                     // a budget of one row: one chunk a row
  CHECK(san_stub_launches("pair_walk_kernel") - w0 > N, "a budget of one row did not split the calls into chunks");
  OK(tnml_destroy(ctx));
  printf("planned pair marginals %s bond %d L %d, label on %d\n", name, M, L, l_pos);
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
    calls(ctx, N, D, L, Ks[l % 3], l % 2 ? (size_t)1 << 30 : 3 * row_bytes(N, D) + 5);
  }
  OK(tnml_destroy(ctx));
  printf("planned pair marginals ragged N %d D %d L %d bonds <= %d at every label position\n", N, D, L, M);
  fflush(stdout);
}

static void run_refusals() {
  const int N = 6, D = 2, L = 3, M = 4, K = 5;
  tnml_ctx *ctx = nullptr;
  OK(tnml_create(&ctx, N, D, L, M, 64, 0));
  Chain w(N, D, L, std::vector<int>(N - 1, M), 2);
  Grid g(K, D);
  Call c(N, D, 0);
  const double *ph = g.phi.data(), *wt = g.w.data(), *va = g.values.data();
  const int32_t *ro = c.rows.data();
  double *q1 = c.q1.data(), *s1 = c.stats1.data(), *q = c.q.data(), *st = c.stats.data();
  FAILS_WITH(TNML_ERR_STATE, tnml_pair_marginals(ctx, K, ph, wt, va, -1, ro, N, q1, s1, q, st));                           // cores never set
  set_cores(ctx, w, 2);
  FAILS_WITH(TNML_ERR_ARG, tnml_pair_marginals(nullptr, K, ph, wt, va, -1, ro, N, q1, s1, q, st));
  FAILS_WITH(TNML_ERR_ARG, tnml_pair_marginals(ctx, K, ph, wt, va, -1, ro, N, nullptr, nullptr, nullptr, nullptr));      // every output NULL
  FAILS_WITH(TNML_ERR_ARG, tnml_pair_marginals(ctx, K, ph, wt, va, -1, nullptr, 0, nullptr, nullptr, q, st));            // ... or without a row
  FAILS_WITH(TNML_ERR_ARG, tnml_pair_marginals(ctx, 1, ph, wt, va, -1, ro, N, q1, s1, q, st));
  FAILS_WITH(TNML_ERR_ARG, tnml_pair_marginals(ctx, 257, ph, wt, va, -1, ro, N, q1, s1, q, st));
  FAILS_WITH(TNML_ERR_ARG, tnml_pair_marginals(ctx, K, nullptr, wt, va, -1, ro, N, q1, s1, q, st));
  FAILS_WITH(TNML_ERR_ARG, tnml_pair_marginals(ctx, K, ph, nullptr, va, -1, ro, N, q1, s1, q, st));
  FAILS_WITH(TNML_ERR_ARG, tnml_pair_marginals(ctx, K, ph, wt, va, -2, ro, N, q1, s1, q, st));                             // the class slot
  FAILS_WITH(TNML_ERR_ARG, tnml_pair_marginals(ctx, K, ph, wt, va, L, ro, N, q1, s1, q, st));
  FAILS_WITH(TNML_ERR_ARG, tnml_pair_marginals(ctx, K, ph, wt, va, -1, ro, -1, q1, s1, q, st));                            // the rows
  FAILS_WITH(TNML_ERR_ARG, tnml_pair_marginals(ctx, K, ph, wt, va, -1, nullptr, N, q1, s1, q, st));
  {
    std::vector<int32_t> bad(c.rows);
    bad[N - 1] = N;
    FAILS_WITH(TNML_ERR_ARG, tnml_pair_marginals(ctx, K, ph, wt, va, -1, bad.data(), N, q1, s1, q, st));
    bad[N - 1] = -1;
    FAILS_WITH(TNML_ERR_ARG, tnml_pair_marginals(ctx, K, ph, wt, va, -1, bad.data(), N, q1, s1, q, st));
    bad[N - 1] = bad[0];
    FAILS_WITH(TNML_ERR_ARG, tnml_pair_marginals(ctx, K, ph, wt, va, -1, bad.data(), N, q1, s1, q, st));
    std::vector<double> bw(g.w), bp(g.phi);
    bw[K - 1] = 0.0;
    bp[K * D - 1] = NAN;
    FAILS_WITH(TNML_ERR_ARG, tnml_pair_marginals(ctx, K, ph, bw.data(), va, -1, ro, N, q1, s1, q, st));
    FAILS_WITH(TNML_ERR_ARG, tnml_pair_marginals(ctx, K, bp.data(), wt, va, -1, ro, N, q1, s1, q, st));
    for (double v : {(double)NAN, (double)INFINITY, -(double)INFINITY}) {                                                   // a value that is not finite
      std::vector<double> bv(g.values);
      bv[K - 1] = v;
      FAILS_WITH(TNML_ERR_ARG, tnml_pair_marginals(ctx, K, ph, wt, bv.data(), -1, ro, N, q1, s1, q, st));
    }
  }
  OK(tnml_set_sample_stack_bytes(ctx, row_bytes(N, D) - 1));                                                               // a budget below one row's need
  FAILS_WITH(TNML_ERR_ARG, tnml_pair_marginals(ctx, K, ph, wt, va, -1, ro, N, q1, s1, q, st));
  OK(tnml_pair_marginals(ctx, K, ph, wt, va, -1, ro, N, q1, s1, nullptr, nullptr));                                        // (the per-site part needs none)
  OK(tnml_set_sample_stack_bytes(ctx, (size_t)1 << 30));
  OK(c.run(ctx, g, K, 1));                                                                                                 // usable afterwards
  OK(tnml_destroy(ctx));
  // the bond limit: kPairMaxBond is taken, one more is refused with the bytes in the message
  OK(tnml_create(&ctx, 4, 2, 2, 128, 64, 0));
  Chain big(4, 2, 2, std::vector<int>{2, tnml::kPairMaxBond + 1, 2}, 0), fits(4, 2, 2, std::vector<int>{2, tnml::kPairMaxBond, 2}, 0);
  Grid g2(256, 2);
  Call c2(4, 2, 0);
  set_cores(ctx, big, 0);
  FAILS_WITH(TNML_ERR_SHAPE, c2.run(ctx, g2, 256, -1));
  if (!strstr(tnml_last_error(), "bytes of LDS")) { fprintf(stderr, "LDS refusal does not name the bytes: %s\n", tnml_last_error()); exit(1); }
  set_cores(ctx, fits, 0);
  OK(c2.run(ctx, g2, 256, -1));
  OK(tnml_destroy(ctx));
  // D = 8 at bond 16 with L = 10 and K = 256 fits; at bond 64 the environments and their product do not
  OK(tnml_create(&ctx, 5, 8, 10, 64, 64, 0));
  Chain d8(5, 8, 10, std::vector<int>(4, 16), 2), d8big(5, 8, 10, std::vector<int>(4, 64), 2);
  Grid g3(256, 8);
  Call c3(5, 8, 0);
  set_cores(ctx, d8, 2);
  OK(c3.run(ctx, g3, 256, 9));
  set_cores(ctx, d8big, 2);
  FAILS_WITH(TNML_ERR_SHAPE, c3.run(ctx, g3, 256, 9));
  OK(tnml_destroy(ctx));
  // with a communicator the call is refused
  setenv("TNML_FORCE_COMM", "1", 1);
  OK(tnml_create(&ctx, N, D, L, M, 64, 0));
  unsigned char uid[128];
  OK(tnml_comm_unique_id(uid));
  OK(tnml_comm_init(ctx, 0, 1, uid));
  Chain w0(N, D, L, std::vector<int>(N - 1, M), 0);
  set_cores(ctx, w0, 0);
  FAILS_WITH(TNML_ERR_STATE, tnml_pair_marginals(ctx, K, ph, wt, va, -1, ro, N, q1, s1, q, st));
  OK(tnml_destroy(ctx));
  unsetenv("TNML_FORCE_COMM");
  printf("pair marginals refusals: ok\n");
}

// every allocation of the new group fails in turn, fresh and at growth (a larger bond; more rows in a chunk)
static void run_alloc_failures(int D) {
  const int N = 6, L = 3, M = 12, K = 7, members = 18;
  tnml_ctx *ctx = nullptr;
  OK(tnml_create(&ctx, N, D, L, M, 64, 0));
  Chain w(N, D, L, std::vector<int>(N - 1, 3), 3), wider(N, D, L, std::vector<int>(N - 1, 5), 3);
  Grid g(K, D);
  set_cores(ctx, w, 3);
  Call none(N, D, 3), few(N, D, 1), all(N, D, 0);
  auto grows = [&](const char *what, Call &c, int want) {
    const int k = fail_each_alloc(what, [&] { return c.run(ctx, g, K, -1); });
    if (k != want) { fprintf(stderr, "%s: %d allocations failed in turn, expected %d\n", what, k, want); exit(1); }
  };
  grows("tnml_pair_marginals, its group is new", none, members);
  grows("tnml_pair_marginals, the group exists", none, 0);
  grows("tnml_pair_marginals, rows", few, members);
  grows("tnml_pair_marginals, more rows", all, members);
  grows("tnml_pair_marginals, fewer rows", few, 0);
  set_cores(ctx, wider, 3);
  grows("tnml_pair_marginals, a larger bond", few, members);
  OK(tnml_destroy(ctx));
}

int main() {
  run_true_size("c3", 784, 2, 2, 20, 0);
  run_true_size("c5 inner label", 784, 2, 10, 50, 400);
  run_ragged(17, 2, 3, 7);
  run_ragged(17, 3, 3, 7);
  run_ragged(17, 8, 17, 6);
  run_ragged(2, 2, 2, 5);
  run_refusals();
  run_alloc_failures(2);
  run_alloc_failures(3);
  san_stub_report();
  for (const char *k : {"pair_close_kernel", "pair_walk_kernel", "pair_stats_kernel"})
    if (san_stub_launches(k) < 1) { fprintf(stderr, "launch path %s was never taken\n", k); return 1; }
  printf("pair marginals: %ld lognorm_env_kernel, %ld pair_close_kernel, %ld pair_walk_kernel and %ld pair_stats_kernel launches checked, %d refusals\n",
         san_stub_launches("lognorm_env_kernel"), san_stub_launches("pair_close_kernel"), san_stub_launches("pair_walk_kernel"),
         san_stub_launches("pair_stats_kernel"), g_refusals);
  printf("pair marginals host planning under ASan + UBSan: ok\n");
  return 0;
}
