// Likelihood gradients from incomplete data (tnml_nll_masked_grad / tnml_nll_masked_step of nll_masked_host.hip and the launch
// wrappers of kernels_nll_masked.hip) planned by the real host code, built --cuda-host-only with AddressSanitizer and UBSan, against
// the stand-in runtime of hip_stub.cpp, which checks the environment launch as it does for the sampler -- held to THIS call's tile --
// and the masked_grad_kernel and masked_grad_reduce_kernel launches behind it: the same block, the offsets, the row weights (2 / n a
// sample, -2 the one normaliser row, 0 padding), the left environments, the partial gradients and the accumulator with their extents,
// grid, block and LDS; and the update launch of the step.  Nothing computes there: the outputs come back as the memory holds them.
// `make san-nll-masked` builds and runs it; tests/test_nll_masked_host.py runs `make san-nll-masked`.
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
extern "C" long san_stub_nmg_normalisers(void);

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
    san_stub_site_cond_call(2);                                                               \
    int rc_ = (call);                                                                         \
    san_stub_site_cond_call(0);                                                               \
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

// the arguments of one call and its outputs; per-sample masks shift their kind (empty, full, prefix, suffix, alternating) from row to row
struct Call {
  int n, N, L, mask_rows;
  std::vector<int32_t> classes, known;
  std::vector<uint8_t> mask;
  std::vector<double> logp;
  std::vector<float> grad;
  double out4[4];
  Call(int n_, int N_, int L_, int K, int mix, int kind, bool per_sample, size_t total) : n(n_), N(N_), L(L_), mask_rows(per_sample ? n_ : 1),
      classes((size_t)n_), known((size_t)n_ * N_), mask((size_t)(per_sample ? n_ : 1) * N_), logp((size_t)n_), grad(total) {
    for (int s = 0; s < n; ++s) classes[s] = mix == 0 ? -1 : mix == 1 ? s % (L + 1) - 1 : L - 1;
    for (int r = 0; r < mask_rows; ++r)
      for (int i = 0; i < N; ++i) {
        const int k = (kind + r) % 5;
        mask[(size_t)r * N + i] = k == 0 ? 0 : k == 1 ? 1 : k == 2 ? i < N / 2 : k == 3 ? i >= N / 2 : i % 2;
      }
    for (int s = 0; s < n; ++s)
      for (int i = 0; i < N; ++i) known[(size_t)s * N + i] = mask[(size_t)(per_sample ? s : 0) * N + i] ? (int32_t)((s + i) % K) : -7;
  }
  // what: 0 the gradient, 1 the value alone, 2 the step
  int run(tnml_ctx *ctx, const Grid &g, int K, int what = 0, bool null_classes = false, bool with_logp = true) {
    san_stub_masked_reset();
    (void)san_stub_nmg_normalisers();
    san_stub_site_cond_call(2);
    const int32_t *cl = null_classes ? nullptr : classes.data();
    int rc;
    if (what == 2) rc = tnml_nll_masked_step(ctx, n, K, g.phi.data(), g.w.data(), cl, mask.data(), mask_rows, known.data(), 0.01f, 0.f, 1, out4);
    else rc = tnml_nll_masked_grad(ctx, n, K, g.phi.data(), g.w.data(), cl, mask.data(), mask_rows, known.data(), what == 0 ? grad.data() : nullptr, grad.size(),
                                   with_logp ? logp.data() : nullptr, out4);
    san_stub_site_cond_call(0);
    if (rc == TNML_OK) {
      san_stub_masked_check(0, n, cl);                           // every sample in exactly one tile, and that tile of its class
      const long nz = san_stub_nmg_normalisers();
      if (nz != (what == 1 ? 0 : 1)) { fprintf(stderr, "a call (what %d) carried %ld normaliser rows of weight -2\n", what, nz); exit(1); }
    }
    return rc;
  }
};

static void set_cores(tnml_ctx *ctx, const Chain &w, int l_pos) { OK(tnml_set_cores(ctx, w.flat.data(), w.flat.size(), w.bond.data(), l_pos)); }

// shared and per-sample masks of every kind, summed, mixed and given classes; the gradient, the value alone and the step in turn:
// every chunk is one environment launch and, unless the value alone is asked for, one masked_grad_kernel and one reduction behind
// it; a step adds one update launch; never a walk of the sampler
static void calls(tnml_ctx *ctx, int N, int L, int K, size_t total, size_t budget, const Grid &g) {
  OK(tnml_set_sample_stack_bytes(ctx, budget));
  int idx = 0;
  for (int mix = 0; mix < 3; ++mix)
    for (int kind = 0; kind < 5; ++kind, ++idx) {
      const long e0 = san_stub_launches("sample_env_masked_kernel"), g0 = san_stub_launches("masked_grad_kernel"), r0 = san_stub_launches("masked_grad_reduce_kernel"),
                 w0 = san_stub_launches("sample_walk_masked_kernel"), o0 = san_stub_launches("optim_step_kernel");
      Call c(mix == 1 ? 40 : 16 + 17 * mix, N, L, K, mix, kind, idx % 2 == 1, total);
      const int what = idx % 3;
      OK(c.run(ctx, g, K, what, mix == 0 && kind == 0, idx % 4 != 0));
      const long e = san_stub_launches("sample_env_masked_kernel") - e0, k = san_stub_launches("masked_grad_kernel") - g0,
                 r = san_stub_launches("masked_grad_reduce_kernel") - r0, o = san_stub_launches("optim_step_kernel") - o0;
      CHECK(e >= 1 && k == (what == 1 ? 0 : e) && r == k && o == (what == 2 ? 1 : 0) && san_stub_launches("sample_walk_masked_kernel") == w0,
            "a call (what %d) made %ld environment, %ld gradient, %ld reduction and %ld update launches", what, e, k, r, o);
    }
  Call one(1, N, L, K, 2, 4, false, total);
  OK(one.run(ctx, g, K));
  OK(tnml_set_sample_stack_bytes(ctx, (size_t)1 << 30));
}

static void run_true_size(const char *name, int N, int D, int L, int M, int l_pos) {
  tnml_ctx *ctx = nullptr;
  OK(tnml_create(&ctx, N, D, L, M, 64, 0));
  Chain w(N, D, L, std::vector<int>(N - 1, M), l_pos);
  set_cores(ctx, w, l_pos);
  Grid g(256, D);
  calls(ctx, N, L, 256, w.flat.size(), (size_t)1 << 30, g);
  // a budget of one tile of this call (its stack and its partial gradient): one chunk a tile
  const int T = tnml::masked_grad_tile(M, D, L, 256);
  CHECK(T >= 1, "no tile at bond %d", M);
  const long e0 = san_stub_launches("sample_env_masked_kernel");
  calls(ctx, N, L, 256, w.flat.size(), ((size_t)T * (N + 1) * M * M + w.flat.size()) * sizeof(double), g);
  CHECK(san_stub_launches("sample_env_masked_kernel") - e0 > 16, "a budget of one tile did not split the calls into chunks");
  OK(tnml_destroy(ctx));
  printf("planned masked likelihood gradients %s bond %d L %d, label on %d, tiles of %d\n", name, M, L, l_pos, T);
  fflush(stdout);
}

// a ragged chain at every label position, K = 2, 7 and 256 in turn, the three optimisers in turn
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
    OK(tnml_optim_config(ctx, l % 3 == 2 ? TNML_OPT_ADAM : TNML_OPT_SGD, l % 3 == 1 ? 0.9 : 0.0, 0.9, 0.999, 1e-8, l % 3 == 1));
    Grid g(Ks[l % 3], D);
    calls(ctx, N, L, Ks[l % 3], w.flat.size(), l % 2 ? (size_t)1 << 30 : ((size_t)2 * 16 * (N + 1) * M * M + 2 * w.flat.size()) * sizeof(double), g);
  }
  OK(tnml_destroy(ctx));
  printf("planned masked likelihood gradients ragged N %d D %d L %d bonds <= %d at every label position\n", N, D, L, M);
  fflush(stdout);
}

static void run_refusals() {
  const int N = 6, D = 2, L = 3, M = 4, K = 5, n = 20;
  tnml_ctx *ctx = nullptr;
  OK(tnml_create(&ctx, N, D, L, M, 64, 0));
  Chain w(N, D, L, std::vector<int>(N - 1, M), 2);
  Grid g(K, D);
  Call c(n, N, L, K, 1, 4, true, w.flat.size());
  const double *ph = g.phi.data(), *wt = g.w.data();
  const int32_t *cl = c.classes.data(), *kn = c.known.data();
  const uint8_t *mk = c.mask.data();
  double *lp = c.logp.data(), *o4 = c.out4;
  float *gr = c.grad.data();
  const size_t cap = c.grad.size();
  FAILS_WITH(TNML_ERR_STATE, tnml_nll_masked_grad(ctx, n, K, ph, wt, cl, mk, n, kn, gr, cap, lp, o4));                       // cores never set
  FAILS_WITH(TNML_ERR_STATE, tnml_nll_masked_step(ctx, n, K, ph, wt, cl, mk, n, kn, 0.1f, 0.f, 1, o4));
  set_cores(ctx, w, 2);
  FAILS_WITH(TNML_ERR_ARG, tnml_nll_masked_grad(nullptr, n, K, ph, wt, cl, mk, n, kn, gr, cap, lp, o4));
  FAILS_WITH(TNML_ERR_ARG, tnml_nll_masked_grad(ctx, n, K, ph, wt, cl, mk, n, kn, gr, cap, lp, nullptr));                    // NULL out4
  FAILS_WITH(TNML_ERR_ARG, tnml_nll_masked_grad(ctx, n, K, ph, wt, cl, mk, n, kn, gr, cap - 1, lp, o4));                     // capacity
  FAILS_WITH(TNML_ERR_ARG, tnml_nll_masked_grad(ctx, 0, K, ph, wt, cl, mk, n, kn, gr, cap, lp, o4));
  FAILS_WITH(TNML_ERR_ARG, tnml_nll_masked_grad(ctx, n, 1, ph, wt, cl, mk, n, kn, gr, cap, lp, o4));
  FAILS_WITH(TNML_ERR_ARG, tnml_nll_masked_grad(ctx, n, 257, ph, wt, cl, mk, n, kn, gr, cap, lp, o4));
  FAILS_WITH(TNML_ERR_ARG, tnml_nll_masked_grad(ctx, n, K, nullptr, wt, cl, mk, n, kn, gr, cap, lp, o4));
  FAILS_WITH(TNML_ERR_ARG, tnml_nll_masked_grad(ctx, n, K, ph, nullptr, cl, mk, n, kn, gr, cap, lp, o4));
  FAILS_WITH(TNML_ERR_ARG, tnml_nll_masked_grad(ctx, n, K, ph, wt, cl, mk, 2, kn, gr, cap, lp, o4));                         // mask_rows
  FAILS_WITH(TNML_ERR_ARG, tnml_nll_masked_grad(ctx, n, K, ph, wt, cl, nullptr, n, kn, gr, cap, lp, o4));                    // NULL mask
  FAILS_WITH(TNML_ERR_ARG, tnml_nll_masked_grad(ctx, n, K, ph, wt, cl, mk, n, nullptr, gr, cap, lp, o4));                    // NULL known, bits set
  {
    std::vector<int32_t> bad(c.classes);
    bad[n - 1] = L;
    FAILS_WITH(TNML_ERR_ARG, tnml_nll_masked_grad(ctx, n, K, ph, wt, bad.data(), mk, n, kn, gr, cap, lp, o4));
    size_t at = 0;
    for (size_t e = 0; e < c.mask.size(); ++e)
      if (c.mask[e]) at = e;
    std::vector<int32_t> bk(c.known);
    bk[at] = K;
    FAILS_WITH(TNML_ERR_ARG, tnml_nll_masked_grad(ctx, n, K, ph, wt, cl, mk, n, bk.data(), gr, cap, lp, o4));
    std::vector<double> bw(g.w), bp(g.phi);
    bw[K - 1] = 0.0;
    bp[K * D - 1] = NAN;
    FAILS_WITH(TNML_ERR_ARG, tnml_nll_masked_grad(ctx, n, K, ph, bw.data(), cl, mk, n, kn, gr, cap, lp, o4));
    FAILS_WITH(TNML_ERR_ARG, tnml_nll_masked_grad(ctx, n, K, bp.data(), wt, cl, mk, n, kn, gr, cap, lp, o4));
  }
  FAILS_WITH(TNML_ERR_ARG, tnml_nll_masked_step(nullptr, n, K, ph, wt, cl, mk, n, kn, 0.1f, 0.f, 1, o4));
  FAILS_WITH(TNML_ERR_ARG, tnml_nll_masked_step(ctx, n, K, ph, wt, cl, mk, n, kn, 0.1f, 0.f, 1, nullptr));
  FAILS_WITH(TNML_ERR_ARG, tnml_nll_masked_step(ctx, n, K, ph, wt, cl, mk, n, kn, 0.1f, 0.f, 2, o4));                        // renorm
  FAILS_WITH(TNML_ERR_ARG, tnml_nll_masked_step(ctx, n, K, ph, wt, cl, mk, 2, kn, 0.1f, 0.f, 1, o4));
  OK(tnml_set_sample_stack_bytes(ctx, 64));                                                                                  // a budget below one tile's need
  FAILS_WITH(TNML_ERR_ARG, tnml_nll_masked_grad(ctx, n, K, ph, wt, cl, mk, n, kn, gr, cap, lp, o4));
  // (the stack of one tile alone holds the value-only call, not the gradient with its partial buffer)
  OK(tnml_set_sample_stack_bytes(ctx, (size_t)tnml::masked_grad_tile(M, D, L, K) * (N + 1) * M * M * sizeof(double)));
  FAILS_WITH(TNML_ERR_ARG, tnml_nll_masked_grad(ctx, n, K, ph, wt, cl, mk, n, kn, gr, cap, lp, o4));
  OK(c.run(ctx, g, K, 1));
  OK(tnml_set_sample_stack_bytes(ctx, (size_t)1 << 30));
  OK(c.run(ctx, g, K));                                                                                                      // usable afterwards
  // the optimiser state belongs to the bonds and the label position of its first step
  OK(tnml_optim_config(ctx, TNML_OPT_ADAM, 0.0, 0.9, 0.999, 1e-8, 0));
  OK(c.run(ctx, g, K, 2));
  Chain moved(N, D, L, std::vector<int>(N - 1, M), 3);
  set_cores(ctx, moved, 3);
  FAILS_WITH(TNML_ERR_STATE, tnml_nll_masked_step(ctx, n, K, ph, wt, cl, mk, n, kn, 0.1f, 0.f, 1, o4));
  OK(tnml_optim_reset(ctx));
  OK(c.run(ctx, g, K, 2));
  OK(tnml_destroy(ctx));
  // the bond limit: kNmgMaxBond is taken, one more is refused with the bytes in the message
  OK(tnml_create(&ctx, 4, 2, 2, 128, 64, 0));
  Chain big(4, 2, 2, std::vector<int>{2, tnml::kNmgMaxBond + 1, 2}, 0), fits(4, 2, 2, std::vector<int>{2, tnml::kNmgMaxBond, 2}, 0);
  Grid g2(256, 2);
  Call c2(n, 4, 2, 256, 1, 3, true, big.flat.size());
  set_cores(ctx, big, 0);
  FAILS_WITH(TNML_ERR_SHAPE, tnml_nll_masked_grad(ctx, n, 256, g2.phi.data(), g2.w.data(), c2.classes.data(), c2.mask.data(), n, c2.known.data(), c2.grad.data(),
                                                  c2.grad.size(), c2.logp.data(), c2.out4));
  if (!strstr(tnml_last_error(), "bytes of LDS")) { fprintf(stderr, "LDS refusal does not name the bytes: %s\n", tnml_last_error()); exit(1); }
  set_cores(ctx, fits, 0);
  OK(c2.run(ctx, g2, 256));
  OK(tnml_destroy(ctx));
  // with a communicator the calls are refused
  setenv("TNML_FORCE_COMM", "1", 1);
  OK(tnml_create(&ctx, N, D, L, M, 64, 0));
  unsigned char uid[128];
  OK(tnml_comm_unique_id(uid));
  OK(tnml_comm_init(ctx, 0, 1, uid));
  Chain w0(N, D, L, std::vector<int>(N - 1, M), 0);
  set_cores(ctx, w0, 0);
  FAILS_WITH(TNML_ERR_STATE, tnml_nll_masked_grad(ctx, n, K, ph, wt, cl, mk, n, kn, gr, cap, lp, o4));
  FAILS_WITH(TNML_ERR_STATE, tnml_nll_masked_step(ctx, n, K, ph, wt, cl, mk, n, kn, 0.1f, 0.f, 1, o4));
  OK(tnml_destroy(ctx));
  unsetenv("TNML_FORCE_COMM");
  printf("masked likelihood gradient refusals: ok\n");
}

// every allocation of the new group fails in turn, fresh and at growth; the masked group, which the sampler creates first here, is
// the sampler's own and is failed in turn by san/plan_masked
static void run_alloc_failures(int D) {
  const int N = 6, L = 3, M = 12, K = 7, members = 7;
  tnml_ctx *ctx = nullptr;
  OK(tnml_create(&ctx, N, D, L, M, 64, 0));
  Chain w(N, D, L, std::vector<int>(N - 1, 3), 3);
  Grid g(K, D);
  set_cores(ctx, w, 3);
  Call small(10, N, L, K, 2, 2, false, w.flat.size()), more(100, N, L, K, 1, 4, true, w.flat.size());
  {
    std::vector<int32_t> lv((size_t)more.n * N), lb((size_t)more.n);
    std::vector<double> lp((size_t)2 * more.n);
    OK(tnml_sample_masked(ctx, more.n, K, g.phi.data(), g.w.data(), more.classes.data(), more.mask.data(), more.mask_rows, more.known.data(), nullptr, 1, 1,
                          lv.data(), lb.data(), lp.data(), nullptr));
  }
  auto grows = [&](const char *what, Call &c, int mode, int want) {
    const int k = fail_each_alloc(what, [&] { return c.run(ctx, g, K, mode); });
    if (k != want) { fprintf(stderr, "%s: %d allocations failed in turn, expected %d\n", what, k, want); exit(1); }
  };
  grows("tnml_nll_masked_grad, the value alone needs no group", small, 1, 0);
  grows("tnml_nll_masked_grad, its group is new", small, 0, members);
  grows("tnml_nll_masked_grad, the group exists", small, 0, 0);
  grows("tnml_nll_masked_grad, more samples and tiles", more, 0, members);
  OK(tnml_optim_config(ctx, TNML_OPT_ADAM, 0.0, 0.9, 0.999, 1e-8, 0));
  grows("tnml_nll_masked_step, the optimiser state is new", small, 2, 2);
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
  run_refusals();
  run_alloc_failures(2);
  run_alloc_failures(3);
  san_stub_report();
  if (san_stub_launches("masked_grad_kernel") < 1) { fprintf(stderr, "launch path masked_grad_kernel was never taken\n"); return 1; }
  printf("masked likelihood gradients: %ld sample_env_masked_kernel, %ld masked_grad_kernel and %ld optim_step_kernel launches checked, %d refusals\n",
         san_stub_launches("sample_env_masked_kernel"), san_stub_launches("masked_grad_kernel"), san_stub_launches("optim_step_kernel"), g_refusals);
  printf("masked likelihood gradient host planning under ASan + UBSan: ok\n");
  return 0;
}
