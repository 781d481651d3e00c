// Samples and log-likelihoods given any set of known pixels (tnml_sample_masked of tnml_api.hip and the launch wrapper of
// kernels_sample_masked.hip) planned by the real host code, built --cuda-host-only with AddressSanitizer and UBSan, against the
// stand-in runtime of hip_stub.cpp, which reads the bond, tile and row tables, the mask and the known levels of every launch as the
// kernels do and checks every core, stack slot, the grid, the uniforms and the outputs with their extents, and keeps the rows of a
// call's launches so that this program can ask: every sample in exactly one tile of its class.  Nothing computes there: the outputs
// come back as the memory holds them.  `make san-masked` builds and runs it; tests/test_sample_masked_host.py runs `make san-masked`.
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

enum MaskKind { kEmpty, kFull, kPrefix, kSuffix, kAlternating, kMaskKinds };

// the arguments of one call and its outputs
struct Call {
  int n, N, L, mask_rows;
  std::vector<int32_t> classes, known, levels, labels;
  std::vector<uint8_t> mask;
  std::vector<double> u, logp, clw;
  // mix 0: all -1; 1: every class and -1 in turn; 2: one class only.  Per-sample masks shift the kind from row to row.
  Call(int n_, int N_, int L_, int K, int mix, MaskKind kind, bool per_sample) : n(n_), N(N_), L(L_), mask_rows(per_sample ? n_ : 1), classes((size_t)n_),
      known((size_t)n_ * N_), levels((size_t)n_ * N_), labels((size_t)n_), mask((size_t)(per_sample ? n_ : 1) * N_), u((size_t)n_ * (N_ + 1), 0.25),
      logp((size_t)2 * n_), clw((size_t)L_) {
    for (int s = 0; s < n; ++s) classes[s] = mix == 0 ? -1 : mix == 1 ? s % (L + 1) - 1 : L - 1;
    for (int r = 0; r < mask_rows; ++r)
      for (int i = 0; i < N; ++i) {
        const int k = (kind + r) % kMaskKinds;
        mask[(size_t)r * N + i] = k == kEmpty ? 0 : k == kFull ? 1 : k == kPrefix ? i < N / 2 : k == kSuffix ? i >= N / 2 : i % 2;
      }
    // levels outside the grid where the mask is not set: they are ignored
    for (int s = 0; s < n; ++s)
      for (int i = 0; i < N; ++i) known[(size_t)s * N + i] = mask[(size_t)(per_sample ? s : 0) * N + i] ? (int32_t)((s + i) % K) : -7;
  }
  int run(tnml_ctx *ctx, const Grid &g, int K, bool with_u, int draw, bool with_clw, bool null_classes = false) {
    san_stub_masked_reset();
    const int rc = tnml_sample_masked(ctx, n, K, g.phi.data(), g.w.data(), null_classes ? nullptr : classes.data(), mask.data(), mask_rows, known.data(),
                                      with_u ? u.data() : nullptr, 7, draw, draw ? levels.data() : nullptr, draw ? labels.data() : nullptr, logp.data(),
                                      with_clw ? clw.data() : nullptr);
    if (rc == TNML_OK) {
      san_stub_masked_check(0, n, null_classes ? nullptr : classes.data());
      if (draw) san_stub_masked_check(1, n, null_classes ? nullptr : classes.data());
    }
    return rc;
  }
};

static void set_cores(tnml_ctx *ctx, const Chain &w, int l_pos) { OK(tnml_set_cores(ctx, w.flat.data(), w.flat.size(), w.bond.data(), l_pos)); }

// shared and per-sample masks of every kind, drawn and given classes, draw 0 and 1, with and without class_logw_out, hashed and
// explicit uniforms: a call without the walk launches no walk kernel, and every chunk is one environment launch
static void masked_calls(tnml_ctx *ctx, int N, int D, int L, int K, size_t budget) {
  Grid g(K, D);
  OK(tnml_set_sample_stack_bytes(ctx, budget));
  int idx = 0;
  for (int mix = 0; mix < 3; ++mix)
    for (int kind = 0; kind < kMaskKinds; ++kind, ++idx) {
      const bool per_sample = idx % 2 == 1;
      const int draw = idx % 3 != 0;
      const long e0 = san_stub_launches("sample_env_masked_kernel"), w0 = san_stub_launches("sample_walk_masked_kernel");
      Call c(mix == 1 ? 40 : 16 + 17 * mix, N, L, K, mix, (MaskKind)kind, per_sample);
      OK(c.run(ctx, g, K, idx % 2 == 0, draw, idx % 4 < 2, mix == 0 && kind == 0));
      const long e = san_stub_launches("sample_env_masked_kernel") - e0, w = san_stub_launches("sample_walk_masked_kernel") - w0;
      CHECK(e >= 1 && w == (draw ? e : 0), "a call with draw = %d made %ld environment and %ld walk launches", draw, e, w);
    }
  Call one(1, N, L, K, 2, kAlternating, false);
  OK(one.run(ctx, g, K, false, 1, false));
  OK(tnml_set_sample_stack_bytes(ctx, (size_t)1 << 30));
}

static void run_true_size(const char *name, int N, int D, int L, int M, int l_pos) {
  tnml_ctx *ctx = nullptr;
  OK(tnml_create(&ctx, N, D, L, M, 64, 0));
  Chain w(N, D, L, std::vector<int>(N - 1, M), l_pos);
  set_cores(ctx, w, l_pos);
  masked_calls(ctx, N, D, L, 256, (size_t)1 << 30);
  // a budget of one tile (of 16, 8, 4, 2 or 1 rows, whichever the call takes: 16 rows fit the budget in every case): many chunks
  const long e0 = san_stub_launches("sample_env_masked_kernel");
  masked_calls(ctx, N, D, L, 256, (size_t)16 * (N + 1) * M * M * sizeof(double));
  CHECK(san_stub_launches("sample_env_masked_kernel") - e0 > 16, "a small stack budget did not split the calls into chunks");
  OK(tnml_destroy(ctx));
  printf("planned masked samples %s bond %d L %d, label on %d\n", name, M, L, l_pos);
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
    masked_calls(ctx, N, D, L, Ks[l % 3], l % 2 ? (size_t)1 << 30 : (size_t)2 * 16 * (N + 1) * M * M * sizeof(double));
  }
  OK(tnml_destroy(ctx));
  printf("planned masked samples ragged N %d D %d L %d bonds <= %d at every label position\n", N, D, L, M);
  fflush(stdout);
}

static void run_refusals() {
  const int N = 6, D = 2, L = 3, M = 4, K = 5, n = 20;
  tnml_ctx *ctx = nullptr;
  OK(tnml_create(&ctx, N, D, L, M, 64, 0));
  Chain w(N, D, L, std::vector<int>(N - 1, M), 2);
  Grid g(K, D);
  Call c(n, N, L, K, 1, kAlternating, true);
  const double *ph = g.phi.data(), *wt = g.w.data(), *u = c.u.data();
  const int32_t *cl = c.classes.data(), *kn = c.known.data();
  const uint8_t *mk = c.mask.data();
  int32_t *lv = c.levels.data(), *lb = c.labels.data();
  double *lp = c.logp.data(), *cw = c.clw.data();
  FAILS_WITH(TNML_ERR_STATE, tnml_sample_masked(ctx, n, K, ph, wt, cl, mk, n, kn, u, 0, 1, lv, lb, lp, cw));             // cores never set
  set_cores(ctx, w, 2);
  auto unchanged = [&] {
    std::vector<float> back(w.flat.size());
    std::vector<int32_t> bg(N - 1);
    int lpos = -1;
    OK(tnml_get_cores(ctx, back.data(), back.size(), bg.data(), &lpos));
    CHECK(lpos == 2 && bg == w.bond && back == w.flat, "a refused call changed the chain");
  };
  FAILS_WITH(TNML_ERR_ARG, tnml_sample_masked(nullptr, n, K, ph, wt, cl, mk, n, kn, u, 0, 1, lv, lb, lp, cw));
  FAILS_WITH(TNML_ERR_ARG, tnml_sample_masked(ctx, 0, K, ph, wt, cl, mk, n, kn, u, 0, 1, lv, lb, lp, cw));
  FAILS_WITH(TNML_ERR_ARG, tnml_sample_masked(ctx, -3, K, ph, wt, cl, mk, 1, kn, u, 0, 1, lv, lb, lp, cw));
  FAILS_WITH(TNML_ERR_ARG, tnml_sample_masked(ctx, n, 1, ph, wt, cl, mk, n, kn, u, 0, 1, lv, lb, lp, cw));
  FAILS_WITH(TNML_ERR_ARG, tnml_sample_masked(ctx, n, 257, ph, wt, cl, mk, n, kn, u, 0, 1, lv, lb, lp, cw));
  FAILS_WITH(TNML_ERR_ARG, tnml_sample_masked(ctx, n, K, nullptr, wt, cl, mk, n, kn, u, 0, 1, lv, lb, lp, cw));
  FAILS_WITH(TNML_ERR_ARG, tnml_sample_masked(ctx, n, K, ph, nullptr, cl, mk, n, kn, u, 0, 1, lv, lb, lp, cw));
  FAILS_WITH(TNML_ERR_ARG, tnml_sample_masked(ctx, n, K, ph, wt, cl, mk, 0, kn, u, 0, 1, lv, lb, lp, cw));                // mask_rows
  FAILS_WITH(TNML_ERR_ARG, tnml_sample_masked(ctx, n, K, ph, wt, cl, mk, 2, kn, u, 0, 1, lv, lb, lp, cw));
  FAILS_WITH(TNML_ERR_ARG, tnml_sample_masked(ctx, n, K, ph, wt, cl, mk, n + 1, kn, u, 0, 1, lv, lb, lp, cw));
  FAILS_WITH(TNML_ERR_ARG, tnml_sample_masked(ctx, n, K, ph, wt, cl, nullptr, n, kn, u, 0, 1, lv, lb, lp, cw));           // NULL mask
  FAILS_WITH(TNML_ERR_ARG, tnml_sample_masked(ctx, n, K, ph, wt, cl, mk, n, nullptr, u, 0, 1, lv, lb, lp, cw));           // NULL known, bits set
  FAILS_WITH(TNML_ERR_ARG, tnml_sample_masked(ctx, n, K, ph, wt, cl, mk, n, kn, u, 0, 1, nullptr, lb, lp, cw));           // draw without outputs
  FAILS_WITH(TNML_ERR_ARG, tnml_sample_masked(ctx, n, K, ph, wt, cl, mk, n, kn, u, 0, 1, lv, nullptr, lp, cw));
  FAILS_WITH(TNML_ERR_ARG, tnml_sample_masked(ctx, n, K, ph, wt, cl, mk, n, kn, u, 0, 1, lv, lb, nullptr, cw));
  FAILS_WITH(TNML_ERR_ARG, tnml_sample_masked(ctx, n, K, ph, wt, cl, mk, n, kn, u, 0, 0, nullptr, nullptr, nullptr, cw));
  FAILS_WITH(TNML_ERR_ARG, tnml_set_sample_stack_bytes(nullptr, 1 << 20));
  FAILS_WITH(TNML_ERR_ARG, tnml_set_sample_stack_bytes(ctx, 0));
  {
    std::vector<int32_t> bad(c.classes);
    bad[n - 1] = L;
    FAILS_WITH(TNML_ERR_ARG, tnml_sample_masked(ctx, n, K, ph, wt, bad.data(), mk, n, kn, u, 0, 1, lv, lb, lp, cw));
    bad[n - 1] = -2;
    FAILS_WITH(TNML_ERR_ARG, tnml_sample_masked(ctx, n, K, ph, wt, bad.data(), mk, n, kn, u, 0, 1, lv, lb, lp, cw));
    // a known level outside the grid at a masked site (the last site of the last row of the alternating kind is one)
    size_t at = 0;
    for (size_t e = 0; e < c.mask.size(); ++e)
      if (c.mask[e]) at = e;
    std::vector<int32_t> bk(c.known);
    bk[at] = K;
    FAILS_WITH(TNML_ERR_ARG, tnml_sample_masked(ctx, n, K, ph, wt, cl, mk, n, bk.data(), u, 0, 1, lv, lb, lp, cw));
    bk[at] = -1;
    FAILS_WITH(TNML_ERR_ARG, tnml_sample_masked(ctx, n, K, ph, wt, cl, mk, n, bk.data(), u, 0, 1, lv, lb, lp, cw));
    for (double v : {0.0, -1.0, (double)NAN, (double)INFINITY}) {
      std::vector<double> bw(g.w);
      bw[K - 1] = v;
      FAILS_WITH(TNML_ERR_ARG, tnml_sample_masked(ctx, n, K, ph, bw.data(), cl, mk, n, kn, u, 0, 1, lv, lb, lp, cw));
    }
    std::vector<double> bp(g.phi);
    bp[K * D - 1] = NAN;
    FAILS_WITH(TNML_ERR_ARG, tnml_sample_masked(ctx, n, K, bp.data(), wt, cl, mk, n, kn, u, 0, 1, lv, lb, lp, cw));
    for (double v : {1.0, -0.5, (double)NAN}) {
      std::vector<double> bu(c.u);
      bu[(size_t)n * (N + 1) - 1] = v;
      FAILS_WITH(TNML_ERR_ARG, tnml_sample_masked(ctx, n, K, ph, wt, cl, mk, n, kn, bu.data(), 0, 1, lv, lb, lp, cw));
    }
  }
  // a stack budget below one tile's need
  OK(tnml_set_sample_stack_bytes(ctx, 64));
  FAILS_WITH(TNML_ERR_ARG, tnml_sample_masked(ctx, n, K, ph, wt, cl, mk, n, kn, u, 0, 1, lv, lb, lp, cw));
  OK(tnml_set_sample_stack_bytes(ctx, (size_t)1 << 30));
  unchanged();
  OK(tnml_sample_masked(ctx, n, K, ph, wt, cl, mk, n, kn, u, 0, 1, lv, lb, lp, cw));                                       // usable afterwards
  // an empty mask takes a NULL known; draw = 0 takes NULL levels and labels
  std::vector<uint8_t> none((size_t)N, 0);
  OK(tnml_sample_masked(ctx, n, K, ph, wt, cl, none.data(), 1, nullptr, u, 0, 0, nullptr, nullptr, lp, nullptr));
  OK(tnml_destroy(ctx));
  // a bond the kernels have no room for: refused with the bytes in the message; bond 64 is the largest they take
  OK(tnml_create(&ctx, 4, 2, 2, 128, 64, 0));
  Chain big(4, 2, 2, std::vector<int>{2, 65, 2}, 0), fits(4, 2, 2, std::vector<int>{2, 64, 2}, 0);
  Grid g2(256, 2);
  Call c2(n, 4, 2, 256, 1, kSuffix, true);
  set_cores(ctx, big, 0);
  FAILS_WITH(TNML_ERR_SHAPE, c2.run(ctx, g2, 256, true, 1, true));
  if (!strstr(tnml_last_error(), "bytes of LDS")) { fprintf(stderr, "LDS refusal does not name the bytes: %s\n", tnml_last_error()); exit(1); }
  set_cores(ctx, fits, 0);
  OK(c2.run(ctx, g2, 256, true, 1, true));
  OK(tnml_destroy(ctx));
  // D = 8 at bond 16 with L = 10 and K = 256 fits
  OK(tnml_create(&ctx, 5, 8, 10, 16, 64, 0));
  Chain d8(5, 8, 10, std::vector<int>(4, 16), 2);
  Grid g3(256, 8);
  Call c3(n, 5, 10, 256, 1, kPrefix, true);
  set_cores(ctx, d8, 2);
  OK(c3.run(ctx, g3, 256, false, 1, true));
  OK(tnml_destroy(ctx));
  // with a communicator the call is refused
  setenv("TNML_FORCE_COMM", "1", 1);
  OK(tnml_create(&ctx, N, D, L, M, 64, 0));
  unsigned char uid[128];
  OK(tnml_comm_unique_id(uid));
  OK(tnml_comm_init(ctx, 0, 1, uid));
  Chain w0(N, D, L, std::vector<int>(N - 1, M), 0);
  set_cores(ctx, w0, 0);
  FAILS_WITH(TNML_ERR_STATE, tnml_sample_masked(ctx, n, K, ph, wt, cl, mk, n, kn, u, 0, 1, lv, lb, lp, cw));
  OK(tnml_destroy(ctx));
  unsetenv("TNML_FORCE_COMM");
  printf("masked sample refusals: ok\n");
}

// tnml_sample_masked leaves everything as it was: no new forward before a sweep, the optimiser state stays bound, tnml_sample's own
// group is untouched
static void run_state_rule() {
  const int N = 8, D = 2, L = 2, M = 6, b = 40, K = 7;
  tnml_ctx *ctx = nullptr;
  OK(tnml_create(&ctx, N, D, L, M, 64, 0));
  std::vector<float> X((size_t)b * N * D, 0.5f), f((size_t)L * b);
  std::vector<int> lab(b, 1);
  Chain w(N, D, L, std::vector<int>(N - 1, 2), 0);
  Grid g(K, D);
  Call c(24, N, L, K, 1, kAlternating, true);
  double met[3];
  set_cores(ctx, w, 0);
  OK(tnml_optim_config(ctx, TNML_OPT_SGD, 0.9, 0.9, 0.999, 1e-8, 0));
  OK(tnml_gd_step(ctx, X.data(), lab.data(), b, 0.1f, 0.f, TNML_ACT_SOFTMAX, TNML_LOSS_FULL_CROSS_ENT, 0.1f, met));
  OK(tnml_set_input(ctx, X.data(), lab.data(), b));
  OK(tnml_forward(ctx, f.data()));
  OK(c.run(ctx, g, K, false, 1, true));
  OK(tnml_gd_step(ctx, X.data(), lab.data(), b, 0.1f, 0.f, TNML_ACT_SOFTMAX, TNML_LOSS_FULL_CROSS_ENT, 0.1f, met));   // the state is still bound
  OK(tnml_forward(ctx, f.data()));
  OK(tnml_sample(ctx, c.n, K, g.phi.data(), g.w.data(), c.classes.data(), nullptr, 0, nullptr, 3, c.levels.data(), c.labels.data(), c.logp.data()));
  OK(c.run(ctx, g, K, true, 0, false));
  OK(tnml_sample(ctx, c.n, K, g.phi.data(), g.w.data(), c.classes.data(), nullptr, 0, nullptr, 3, c.levels.data(), c.labels.data(), c.logp.data()));
  OK(tnml_sweep(ctx, 0, 2, 1, 1e-3f, 1e-3f, 1, TNML_ACT_SOFTMAX, TNML_LOSS_FULL_CROSS_ENT, 0.1f, TNML_TRUNC_FIXED, nullptr, nullptr));
  OK(tnml_destroy(ctx));
  printf("state rule after tnml_sample_masked: ok\n");
}

// every allocation of the new group fails in turn, on first use and on every kind of growth
static void run_alloc_failures(int D) {
  const int N = 6, L = 3, M = 12, K = 7, members = 15;
  tnml_ctx *ctx = nullptr;
  OK(tnml_create(&ctx, N, D, L, M, 64, 0));
  Chain w(N, D, L, std::vector<int>(N - 1, 3), 3), w5(N, D, L, std::vector<int>(N - 1, 5), 3);
  Grid g(K, D);
  set_cores(ctx, w, 3);
  Call small(10, N, L, K, 2, kPrefix, false), more(100, N, L, K, 1, kAlternating, false), rows(100, N, L, K, 1, kAlternating, true);
  auto grows = [&](const char *what, Call &c, bool with_u, bool with_clw, int want) {
    const int k = fail_each_alloc(what, [&] { return c.run(ctx, g, K, with_u, 1, with_clw); });
    if (k != want) { fprintf(stderr, "%s: %d allocations failed in turn, expected %d\n", what, k, want); exit(1); }
  };
  grows("tnml_sample_masked, fresh context", small, false, false, members);
  grows("tnml_sample_masked, the group exists", small, false, false, 0);
  grows("tnml_sample_masked, more samples and tiles", more, false, false, members);
  grows("tnml_sample_masked, explicit uniforms", more, true, false, members);
  grows("tnml_sample_masked, a mask per sample", rows, true, false, members);
  grows("tnml_sample_masked, every class slot", small, false, true, 0);
  set_cores(ctx, w5, 3);
  grows("tnml_sample_masked, a larger bond", rows, true, true, members);
  OK(rows.run(ctx, g, K, true, 1, true));
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
  const char *paths[] = {"sample_env_masked_kernel", "sample_walk_masked_kernel"};
  for (const char *k : paths)
    if (san_stub_launches(k) < 1) { fprintf(stderr, "launch path %s was never taken\n", k); return 1; }
  printf("masked sample: %ld sample_env_masked_kernel and %ld sample_walk_masked_kernel launches checked, %d refusals\n",
         san_stub_launches("sample_env_masked_kernel"), san_stub_launches("sample_walk_masked_kernel"), g_refusals);
  printf("masked sample host planning under ASan + UBSan: ok\n");
  return 0;
}
