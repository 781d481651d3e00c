// Inner products and linear combinations of two MPS (tnml_inner / tnml_axpby of api_mps.hip and the launch wrappers of
// kernels_algebra.hip) planned by the real host code, built --cuda-host-only with AddressSanitizer and UBSan, against the stand-in
// runtime of hip_stub.cpp, which reads both bond and offset tables of every launch as the kernels do and checks every core of
// either chain, the staging areas, the half results, the outputs and the float32 result with its extent.  Nothing computes there:
// the six outputs come back as the memory holds them.  `make san-algebra` builds and runs it; tests/test_mps_algebra_host.py runs
// `make san-algebra`.
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

static const int kAct = TNML_ACT_SOFTMAX, kLoss = TNML_LOSS_FULL_CROSS_ENT;

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

// tnml_inner with a second chain, without one, with both metric forms: each is one chain and one meet launch
static void inner_calls(tnml_ctx *ctx, int N, int D, const Chain &v, int l_pos) {
  double out[6];
  std::vector<double> S((size_t)N * D * D, 0.5);
  const long a = san_stub_launches("inner_chain_kernel"), b = san_stub_launches("inner_meet_kernel");
  OK(tnml_inner(ctx, v.flat.data(), v.flat.size(), v.bond.data(), l_pos, nullptr, 0, out));
  OK(tnml_inner(ctx, nullptr, 0, nullptr, 0, nullptr, 0, out));
  CHECK(out[2] == 0.0 && out[3] == -INFINITY && out[4] == 0.0 && out[5] == -INFINITY, "<W|W> alone: the other four entries are %g %g %g %g", out[2], out[3], out[4], out[5]);
  OK(tnml_inner(ctx, v.flat.data(), v.flat.size(), v.bond.data(), l_pos, S.data(), 1, out));
  OK(tnml_inner(ctx, v.flat.data(), v.flat.size(), v.bond.data(), l_pos, S.data(), N, out));
  CHECK(san_stub_launches("inner_chain_kernel") - a == 4 && san_stub_launches("inner_meet_kernel") - b == 4, "four calls did not make four launches of each kernel");
}

static void run_true_size(const char *name, int N, int D, int L, int M, int l_pos) {
  tnml_ctx *ctx = nullptr;
  OK(tnml_create(&ctx, N, D, L, 2 * M, 64, 0));                 // room for the sum of two bond-M chains
  Chain w(N, D, L, std::vector<int>(N - 1, M), l_pos), v(N, D, L, std::vector<int>(N - 1, M), l_pos);
  set_cores(ctx, w, l_pos);
  inner_calls(ctx, N, D, v, l_pos);
  std::vector<int32_t> bo(N - 1);
  OK(tnml_axpby(ctx, 0.5, 0.5, v.flat.data(), v.flat.size(), v.bond.data(), l_pos, bo.data()));
  for (int i = 0; i < N - 1; ++i) CHECK(bo[i] == 2 * M, "bond %d after the sum is %d", i, bo[i]);
  inner_calls(ctx, N, D, v, l_pos);                             // the summed chain against V: bonds 2 M and M
  OK(tnml_destroy(ctx));
  printf("planned inner products and the sum %s bond %d L %d, label on %d\n", name, M, L, l_pos);
  fflush(stdout);
}

// a ragged 17-site chain with different bonds for W and V at every label position (and N = 2)
static void run_ragged(int N, int D, int L, int MW, int MV) {
  tnml_ctx *ctx = nullptr;
  OK(tnml_create(&ctx, N, D, L, MW + MV, 64, 0));
  for (int l = 0; l < N; ++l) {
    std::vector<int> bw(N - 1), bv(N - 1);
    for (int i = 0; i < N - 1; ++i) { bw[i] = 1 + (i * 7 + l * 3) % MW; bv[i] = 1 + (i * 5 + l) % MV; }
    bw[(l * 5) % (N - 1)] = MW;
    bv[(l * 3 + 1) % (N - 1)] = MV;
    Chain w(N, D, L, bw, l), v(N, D, L, bv, l);
    set_cores(ctx, w, l);
    inner_calls(ctx, N, D, v, l);
    std::vector<int32_t> bo(N - 1);
    OK(tnml_axpby(ctx, 1.0, -1.0, v.flat.data(), v.flat.size(), v.bond.data(), l, bo.data()));
    for (int i = 0; i < N - 1; ++i) CHECK(bo[i] == bw[i] + bv[i], "bond %d after the sum is %d", i, bo[i]);
    std::vector<int32_t> bg(N - 1);
    size_t n = 0;
    int lp = -1;
    OK(tnml_cores_size(ctx, &n));
    std::vector<float> back(n);
    OK(tnml_get_cores(ctx, back.data(), n, bg.data(), &lp));
    CHECK(lp == l && bg == bo, "the committed chain has l_pos %d", lp);
    inner_calls(ctx, N, D, v, l);
  }
  OK(tnml_destroy(ctx));
  printf("planned inner products and sums ragged N %d D %d L %d bonds <= %d and <= %d at every label position\n", N, D, L, MW, MV);
  fflush(stdout);
}

static void run_refusals() {
  const int N = 6, D = 2, L = 3, M = 4;
  tnml_ctx *ctx = nullptr;
  OK(tnml_create(&ctx, N, D, L, M, 64, 0));                     // capacity max(4, 2 * 3) = 6
  Chain w(N, D, L, std::vector<int>(N - 1, M), 2), v(N, D, L, std::vector<int>(N - 1, 2), 2), v3(N, D, L, std::vector<int>(N - 1, 3), 2);
  double out[6], S[N * D * D] = {0};
  int32_t bo[N - 1];
  const float *vf = v.flat.data();
  const size_t vn = v.flat.size();
  const int32_t *vb = v.bond.data();
  FAILS_WITH(TNML_ERR_STATE, tnml_inner(ctx, nullptr, 0, nullptr, 0, nullptr, 0, out));               // cores never set
  {
    Chain u(N, D, L, std::vector<int>(N - 1, 2), 0);                                                  // (a fresh context has its label on site 0)
    FAILS_WITH(TNML_ERR_STATE, tnml_inner(ctx, u.flat.data(), u.flat.size(), u.bond.data(), 0, nullptr, 0, out));
    FAILS_WITH(TNML_ERR_STATE, tnml_axpby(ctx, 1.0, 1.0, u.flat.data(), u.flat.size(), u.bond.data(), 0, bo));
  }
  set_cores(ctx, w, 2);
  auto unchanged = [&] {
    std::vector<float> back(w.flat.size());
    std::vector<int32_t> bg(N - 1);
    int lp = -1;
    OK(tnml_get_cores(ctx, back.data(), back.size(), bg.data(), &lp));
    CHECK(lp == 2 && bg == w.bond && back == w.flat, "a refused call changed the chain");
  };
  FAILS_WITH(TNML_ERR_ARG, tnml_inner(nullptr, vf, vn, vb, 2, nullptr, 0, out));
  FAILS_WITH(TNML_ERR_ARG, tnml_inner(ctx, vf, vn, vb, 2, nullptr, 0, nullptr));
  FAILS_WITH(TNML_ERR_ARG, tnml_inner(ctx, vf, vn - 1, vb, 2, nullptr, 0, out));
  FAILS_WITH(TNML_ERR_ARG, tnml_inner(ctx, vf, vn, nullptr, 2, nullptr, 0, out));
  FAILS_WITH(TNML_ERR_ARG, tnml_inner(ctx, vf, vn, vb, 3, nullptr, 0, out));                          // another label position
  FAILS_WITH(TNML_ERR_ARG, tnml_inner(ctx, vf, vn, vb, 2, S, 0, out));
  FAILS_WITH(TNML_ERR_ARG, tnml_inner(ctx, vf, vn, vb, 2, S, 2, out));
  FAILS_WITH(TNML_ERR_ARG, tnml_inner(ctx, vf, vn, vb, 2, S, N + 1, out));
  {
    std::vector<int32_t> zb(v.bond);
    zb[1] = 0;
    FAILS_WITH(TNML_ERR_ARG, tnml_inner(ctx, vf, vn, zb.data(), 2, nullptr, 0, out));
    FAILS_WITH(TNML_ERR_ARG, tnml_axpby(ctx, 1.0, 1.0, vf, vn, zb.data(), 2, bo));
  }
  FAILS_WITH(TNML_ERR_ARG, tnml_axpby(nullptr, 1.0, 1.0, vf, vn, vb, 2, bo));
  FAILS_WITH(TNML_ERR_ARG, tnml_axpby(ctx, 1.0, 1.0, vf, vn, vb, 2, nullptr));
  FAILS_WITH(TNML_ERR_ARG, tnml_axpby(ctx, 1.0, 1.0, nullptr, 0, nullptr, 2, bo));
  FAILS_WITH(TNML_ERR_ARG, tnml_axpby(ctx, NAN, 1.0, vf, vn, vb, 2, bo));
  FAILS_WITH(TNML_ERR_ARG, tnml_axpby(ctx, 1.0, INFINITY, vf, vn, vb, 2, bo));
  FAILS_WITH(TNML_ERR_ARG, tnml_axpby(ctx, 1.0, 1.0, vf, vn + 3, vb, 2, bo));
  FAILS_WITH(TNML_ERR_ARG, tnml_axpby(ctx, 1.0, 1.0, vf, vn, vb, 1, bo));
  FAILS_WITH(TNML_ERR_ARG, tnml_axpby(ctx, 1.0, 1.0, v3.flat.data(), v3.flat.size(), v3.bond.data(), 2, bo));   // 4 + 3 > 6
  if (!strstr(tnml_last_error(), "capacity 6") || !strstr(tnml_last_error(), "bond 0")) { fprintf(stderr, "the capacity refusal names neither: %s\n", tnml_last_error()); exit(1); }
  unchanged();
  OK(tnml_inner(ctx, vf, vn, vb, 2, nullptr, 0, out));                                                // usable afterwards
  OK(tnml_axpby(ctx, 1.0, 1.0, vf, vn, vb, 2, bo));
  OK(tnml_destroy(ctx));
  // bonds the chain kernel's LDS has no room for: refused with the bytes in the message; V's bond counts as W's does
  OK(tnml_create(&ctx, 4, 2, 2, 128, 64, 0));
  Chain big(4, 2, 2, std::vector<int>{2, 128, 2}, 0), fits(4, 2, 2, std::vector<int>{2, 100, 2}, 0), small(4, 2, 2, std::vector<int>{2, 3, 2}, 0);
  set_cores(ctx, big, 0);
  FAILS_WITH(TNML_ERR_SHAPE, tnml_inner(ctx, nullptr, 0, nullptr, 0, nullptr, 0, out));
  if (!strstr(tnml_last_error(), "bytes of LDS")) { fprintf(stderr, "LDS refusal does not name the bytes: %s\n", tnml_last_error()); exit(1); }
  set_cores(ctx, small, 0);
  FAILS_WITH(TNML_ERR_SHAPE, tnml_inner(ctx, big.flat.data(), big.flat.size(), big.bond.data(), 0, nullptr, 0, out));
  OK(tnml_inner(ctx, fits.flat.data(), fits.flat.size(), fits.bond.data(), 0, nullptr, 0, out));      // the largest bond it takes
  set_cores(ctx, fits, 0);
  OK(tnml_inner(ctx, fits.flat.data(), fits.flat.size(), fits.bond.data(), 0, nullptr, 0, out));
  OK(tnml_destroy(ctx));
  // with a communicator every call is refused
  setenv("TNML_FORCE_COMM", "1", 1);
  OK(tnml_create(&ctx, N, D, L, M, 64, 0));
  unsigned char uid[128];
  OK(tnml_comm_unique_id(uid));
  OK(tnml_comm_init(ctx, 0, 1, uid));
  Chain w0(N, D, L, std::vector<int>(N - 1, M), 0), v0(N, D, L, std::vector<int>(N - 1, 2), 0);
  set_cores(ctx, w0, 0);
  FAILS_WITH(TNML_ERR_STATE, tnml_inner(ctx, v0.flat.data(), v0.flat.size(), v0.bond.data(), 0, nullptr, 0, out));
  FAILS_WITH(TNML_ERR_STATE, tnml_axpby(ctx, 1.0, 1.0, v0.flat.data(), v0.flat.size(), v0.bond.data(), 0, bo));
  OK(tnml_destroy(ctx));
  unsetenv("TNML_FORCE_COMM");
  printf("algebra refusals: ok\n");
}

// tnml_inner leaves everything as it was (no new forward before a sweep, the optimiser state stays bound); a committed tnml_axpby
// leaves the context as tnml_scale_cores does and unbinds a bound optimiser state
static void run_state_rule() {
  const int N = 8, D = 2, L = 2, M = 6, b = 40;
  tnml_ctx *ctx = nullptr;
  OK(tnml_create(&ctx, N, D, L, M, 64, 0));
  std::vector<float> X((size_t)b * N * D, 0.5f), f((size_t)L * b);
  std::vector<int> lab(b, 1);
  Chain w(N, D, L, std::vector<int>(N - 1, 2), 0), v(N, D, L, std::vector<int>(N - 1, 3), 0);
  double met[3], out[6];
  int32_t bo[N - 1];
  for (int which = 1; which < 3; ++which) {
    set_cores(ctx, w, 0);
    if (which == 1) OK(tnml_optim_config(ctx, TNML_OPT_SGD, 0.9, 0.9, 0.999, 1e-8, 0));
    else OK(tnml_optim_config(ctx, TNML_OPT_ADAM, 0.0, 0.9, 0.999, 1e-3, 0));
    OK(tnml_gd_step(ctx, X.data(), lab.data(), b, 0.1f, 0.f, kAct, kLoss, 0.1f, met));
    OK(tnml_set_input(ctx, X.data(), lab.data(), b));
    OK(tnml_forward(ctx, f.data()));
    OK(tnml_inner(ctx, v.flat.data(), v.flat.size(), v.bond.data(), 0, nullptr, 0, out));
    OK(tnml_gd_step(ctx, X.data(), lab.data(), b, 0.1f, 0.f, kAct, kLoss, 0.1f, met));               // the state is still bound
    OK(tnml_forward(ctx, f.data()));
    OK(tnml_inner(ctx, v.flat.data(), v.flat.size(), v.bond.data(), 0, nullptr, 0, out));
    OK(tnml_sweep(ctx, 0, 2, 1, 1e-3f, 1e-3f, 1, kAct, kLoss, 0.1f, TNML_TRUNC_FIXED, nullptr, nullptr));   // inner: no new forward needed
    set_cores(ctx, w, 0);
    OK(tnml_optim_reset(ctx));
    OK(tnml_gd_step(ctx, X.data(), lab.data(), b, 0.1f, 0.f, kAct, kLoss, 0.1f, met));
    OK(tnml_forward(ctx, f.data()));
    OK(tnml_axpby(ctx, 1.0, 1.0, v.flat.data(), v.flat.size(), v.bond.data(), 0, bo));
    FAILS_WITH(TNML_ERR_STATE, tnml_sweep(ctx, 0, N - 1, 1, 1e-3f, 1e-3f, 1, kAct, kLoss, 0.1f, TNML_TRUNC_FIXED, nullptr, nullptr));
    FAILS_WITH(TNML_ERR_STATE, tnml_gd_step(ctx, X.data(), lab.data(), b, 0.1f, 0.f, kAct, kLoss, 0.1f, met));
    if (!strstr(tnml_last_error(), "tnml_optim_reset")) { fprintf(stderr, "the refusal does not name tnml_optim_reset: %s\n", tnml_last_error()); exit(1); }
    OK(tnml_optim_reset(ctx));
    OK(tnml_gd_step(ctx, X.data(), lab.data(), b, 0.1f, 0.f, kAct, kLoss, 0.1f, met));
    OK(tnml_forward(ctx, f.data()));
    OK(tnml_sweep(ctx, 0, N - 1, 1, 1e-3f, 1e-3f, 1, kAct, kLoss, 0.1f, TNML_TRUNC_FIXED, nullptr, nullptr));
  }
  OK(tnml_destroy(ctx));
  printf("commit rule and optimiser state rule after tnml_axpby: ok\n");
}

// every allocation of the new group fails in turn, whichever call creates it, and when a larger second chain makes it grow
static void run_alloc_failures(int D) {
  const int N = 6, L = 2, M = 12;
  for (int first = 0; first < 2; ++first) {
    tnml_ctx *ctx = nullptr;
    OK(tnml_create(&ctx, N, D, L, M, 64, 0));
    Chain w(N, D, L, std::vector<int>(N - 1, 3), 3), v(N, D, L, std::vector<int>(N - 1, 2), 3), v5(N, D, L, std::vector<int>(N - 1, 5), 3);
    set_cores(ctx, w, 3);
    double out[6];
    int32_t bo[N - 1];
    int k;
    if (first == 0) k = fail_each_alloc("tnml_inner, fresh context", [&] { return tnml_inner(ctx, v.flat.data(), v.flat.size(), v.bond.data(), 3, nullptr, 0, out); });
    else k = fail_each_alloc("tnml_axpby, fresh context", [&] { return tnml_axpby(ctx, 1.0, 1.0, v.flat.data(), v.flat.size(), v.bond.data(), 3, bo); });
    if (k != 11) { fprintf(stderr, "%d allocations failed in turn, the group has 11\n", k); exit(1); }
    k = fail_each_alloc("tnml_inner, the group exists", [&] { return tnml_inner(ctx, v.flat.data(), v.flat.size(), v.bond.data(), 3, nullptr, 0, out); });
    if (k != 0) { fprintf(stderr, "%d allocations in a second call\n", k); exit(1); }
    k = fail_each_alloc("tnml_inner, a larger second chain", [&] { return tnml_inner(ctx, v5.flat.data(), v5.flat.size(), v5.bond.data(), 3, nullptr, 0, out); });
    if (k != 11) { fprintf(stderr, "%d allocations failed in turn when the group grew, it has 11\n", k); exit(1); }
    OK(tnml_destroy(ctx));
  }
}

int main() {
  run_true_size("c3", 784, 2, 2, 20, 0);
  run_true_size("c3 last", 784, 2, 2, 20, 783);
  run_true_size("c3 inner label", 784, 2, 2, 20, 391);
  run_true_size("c5", 784, 2, 10, 50, 783);
  run_true_size("c5 first", 784, 2, 10, 50, 0);
  run_true_size("c5 inner label", 784, 2, 10, 50, 400);
  run_ragged(17, 2, 3, 5, 7);
  run_ragged(17, 3, 3, 7, 4);
  run_ragged(17, 8, 17, 6, 3);
  run_ragged(2, 2, 2, 5, 7);
  run_ragged(2, 8, 10, 3, 4);
  run_refusals();
  run_state_rule();
  run_alloc_failures(2);
  run_alloc_failures(3);
  san_stub_report();
  const char *paths[] = {"inner_chain_kernel", "inner_meet_kernel", "sum_place_kernel"};
  for (const char *k : paths)
    if (san_stub_launches(k) < 1) { fprintf(stderr, "launch path %s was never taken\n", k); return 1; }
  printf("algebra: %ld inner_chain_kernel and %ld sum_place_kernel launches checked, %d refusals\n", san_stub_launches("inner_chain_kernel"),
         san_stub_launches("sum_place_kernel"), g_refusals);
  printf("algebra host planning under ASan + UBSan: ok\n");
  return 0;
}
