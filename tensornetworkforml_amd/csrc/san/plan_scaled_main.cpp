// Range-safe chains (tnml_set_chain_scaling / tnml_predict_scaled of tnml_api.hip and the launch wrappers of kernels_scaled.hip,
// kernels_inputgrad.hip and kernels_coregrad.hip) planned by the real host code, built --cuda-host-only with AddressSanitizer and
// UBSan, against the stand-in runtime of hip_stub.cpp, which checks every pointer of the three new kernels' parameter blocks with
// the extent the kernel touches: the wrapped plain blocks, the exponent stacks [N][b_pad], mant, expo and f, every core through the
// uploaded bond table.  `make san-scaled` builds and runs it; tests/test_scaled_chain_host.py runs `make san-scaled`.
#include <hip/hip_runtime.h>

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

static const char *kScaled[] = {"scaled_pred_kernel", "input_grad_scaled_kernel", "core_grad_chain_scaled_kernel"};
static const char *kPlain[] = {"env_chain", "label_meet_kernel", "input_grad_kernel", "core_grad_chain_kernel"};
struct Counts { long scaled[3], plain[4]; };
static Counts counts() {
  Counts c;
  for (int i = 0; i < 3; ++i) c.scaled[i] = san_stub_launches(kScaled[i]);
  for (int i = 0; i < 4; ++i) c.plain[i] = san_stub_launches(kPlain[i]);
  return c;
}
// since `from`: the scaled kernels were launched pred / ig / cg times and no plain chain at all
static void expect_scaled(const char *what, const Counts &from, long pred, long ig, long cg) {
  const Counts now = counts();
  const long want[3] = {pred, ig, cg};
  for (int i = 0; i < 3; ++i)
    if (now.scaled[i] - from.scaled[i] != want[i]) { fprintf(stderr, "%s: %ld launches of %s, expected %ld\n", what, now.scaled[i] - from.scaled[i], kScaled[i], want[i]); exit(1); }
  for (int i = 0; i < 4; ++i)
    if (now.plain[i] != from.plain[i]) { fprintf(stderr, "%s: %ld launches of the plain %s with the switch on\n", what, now.plain[i] - from.plain[i], kPlain[i]); exit(1); }
}

static size_t set_cores(tnml_ctx *ctx, int N, int D, int L, const std::vector<int> &bond, int l_pos) {
  size_t total = 0;
  for (int i = 0; i < N; ++i) total += (size_t)(i == 0 ? 1 : bond[i - 1]) * D * (i == N - 1 ? 1 : bond[i]) * (i == l_pos ? L : 1);
  std::vector<float> cores(total, 0.1f);
  OK(tnml_set_cores(ctx, cores.data(), total, bond.data(), l_pos));
  return total;
}

// C3 / C5 at true size with the switch on: b samples in the default chunk and in chunks of 64
static void run_true_size(const char *name, int N, int D, int L, int M, int b, int l_pos) {
  tnml_ctx *ctx = nullptr;
  OK(tnml_create(&ctx, N, D, L, M, 64, 0));
  OK(tnml_set_any_position(ctx, 1));
  OK(tnml_set_chain_scaling(ctx, 1));
  const size_t total = set_cores(ctx, N, D, L, std::vector<int>(N - 1, M), l_pos);
  std::vector<float> X((size_t)b * N * D, 0.5f), cot((size_t)L * b, 1.f), G(total), cf(b), g((size_t)b * N * D), f((size_t)L * b), mant((size_t)L * b);
  std::vector<int> y(b, 0), expo(b);
  const int def = (int)(((size_t)256 << 20) / ((size_t)N * M * 4) / 64 * 64), nd = (b + def - 1) / def, n64 = (b + 63) / 64;
  double met[3];
  for (int pass = 0; pass < 2; ++pass) {
    const long nc = pass ? n64 : nd;
    OK(tnml_set_core_grad_chunk(ctx, pass ? 64 : 0));
    OK(tnml_set_input_grad_chunk(ctx, pass ? 64 : 0));
    Counts c0 = counts();
    OK(tnml_predict(ctx, X.data(), b, f.data()));
    OK(tnml_predict_scaled(ctx, X.data(), b, mant.data(), expo.data()));
    expect_scaled("predict, predict_scaled", c0, 2, 0, 0);
    c0 = counts();
    OK(tnml_input_grad(ctx, X.data(), b, cot.data(), g.data(), cf.data()));
    expect_scaled("input_grad, dense cot", c0, 0, nc, 0);
    c0 = counts();
    OK(tnml_input_grad(ctx, X.data(), b, nullptr, g.data(), nullptr));
    expect_scaled("input_grad, predicted class", c0, nc, nc, 0);
    c0 = counts();
    OK(tnml_core_grad(ctx, X.data(), b, cot.data(), G.data(), total, cf.data()));
    expect_scaled("core_grad, dense cot", c0, 0, 0, nc);
    c0 = counts();
    OK(tnml_core_grad(ctx, X.data(), b, nullptr, G.data(), total, nullptr));
    expect_scaled("core_grad, predicted class", c0, nc, 0, nc);
    c0 = counts();
    OK(tnml_gd_step(ctx, X.data(), y.data(), b, 1e-3f, 0.f, 0, 0, 1.f, met));
    expect_scaled("gd_step", c0, nc, 0, nc);
  }
  // the switch off again: the plain kernels, none of the scaled ones
  OK(tnml_set_chain_scaling(ctx, 0));
  const Counts c0 = counts();
  OK(tnml_predict(ctx, X.data(), 70, f.data()));
  OK(tnml_input_grad(ctx, X.data(), 70, cot.data(), g.data(), cf.data()));
  OK(tnml_core_grad(ctx, X.data(), 70, cot.data(), G.data(), total, cf.data()));
  const Counts c1 = counts();
  for (int i = 0; i < 3; ++i)
    if (c1.scaled[i] != c0.scaled[i]) { fprintf(stderr, "%s launched with the switch off\n", kScaled[i]); exit(1); }
  // (70 samples in chunks of 64)
  if (c1.plain[2] - c0.plain[2] != 2 || c1.plain[3] - c0.plain[3] != 2) { fprintf(stderr, "the plain gradient kernels did not run with the switch off\n"); exit(1); }
  OK(tnml_destroy(ctx));
  printf("planned scaled chains %s bond %d L %d b %d (default chunk %d)\n", name, M, L, b, def);
  fflush(stdout);
}

// a ragged 17-site chain at every label position: predict, predict_scaled, eval, both gradients and gd_step, b = 70 and b = 1
static void run_ragged(int D, int L, int M) {
  const int N = 17, n = 90;
  tnml_ctx *ctx = nullptr;
  OK(tnml_create(&ctx, N, D, L, M, 64, 0));
  OK(tnml_set_any_position(ctx, 1));
  std::vector<float> X((size_t)200 * N * D, 0.5f), cot((size_t)L * 200, 1.f), cf(200), G((size_t)N * D * M * M * L), g((size_t)200 * N * D), f((size_t)L * 200), mant((size_t)L * 200);
  std::vector<int> lab(n, 0), idx(200), y(200, L - 1), expo(200);
  for (int i = 0; i < 200; ++i) idx[i] = (i * 37) % n;                       // repeats included
  OK(tnml_dataset_attach(ctx, X.data(), lab.data(), n, N, D, TNML_DATASET_FEATURES));
  double met[3], acc3[3];
  for (int l = 0; l < N; ++l) {
    std::vector<int> bond(N - 1);
    for (int i = 0; i < N - 1; ++i) bond[i] = 1 + (i * 7 + l * 3) % M;
    bond[(l * 5) % (N - 1)] = M;
    const size_t total = set_cores(ctx, N, D, L, bond, l);
    OK(tnml_predict_scaled(ctx, X.data(), 70, mant.data(), expo.data()));     // (the switch is off for l = 0's first call)
    OK(tnml_set_chain_scaling(ctx, 1));
    const Counts c0 = counts();
    OK(tnml_predict(ctx, X.data(), 70, f.data()));
    OK(tnml_predict(ctx, X.data(), 1, f.data()));
    OK(tnml_predict_scaled(ctx, X.data(), 1, mant.data(), expo.data()));
    OK(tnml_predict_indices(ctx, idx.data(), 200, f.data()));
    OK(tnml_eval_indices(ctx, idx.data(), 200, 0, 1.f, acc3));
    OK(tnml_input_grad(ctx, X.data(), 70, cot.data(), g.data(), cf.data()));
    OK(tnml_input_grad(ctx, X.data(), 1, nullptr, g.data(), nullptr));
    OK(tnml_input_grad_indices(ctx, idx.data(), 200, nullptr, TNML_WRT_FEATURES, g.data(), cf.data()));
    OK(tnml_core_grad(ctx, X.data(), 70, cot.data(), G.data(), total, cf.data()));
    OK(tnml_core_grad(ctx, X.data(), 1, nullptr, G.data(), total, nullptr));
    OK(tnml_core_grad_indices(ctx, idx.data(), 200, nullptr, G.data(), total, cf.data()));
    OK(tnml_gd_step(ctx, X.data(), y.data(), 70, 1e-3f, 0.f, 0, 0, 1.f, met));
    OK(tnml_gd_train_indices(ctx, idx.data(), 200, 70, 1e-3f, 0.f, 2, 2, 1.f, nullptr));
    const Counts c1 = counts();
    for (int i = 0; i < 4; ++i)
      if (c1.plain[i] != c0.plain[i]) { fprintf(stderr, "label site %d: the plain %s ran with the switch on\n", l, kPlain[i]); exit(1); }
    if (l % 2) OK(tnml_set_chain_scaling(ctx, 0));
  }
  OK(tnml_destroy(ctx));
  printf("planned scaled chains ragged N %d D %d L %d bond <= %d\n", N, D, L, M);
  fflush(stdout);
}

static void run_refusals() {
  const int N = 6, D = 2, L = 3, M = 4;
  tnml_ctx *ctx = nullptr;
  OK(tnml_create(&ctx, N, D, L, M, 64, 0));
  std::vector<float> X((size_t)70 * N * D, 0.5f), mant((size_t)L * 70), f((size_t)L * 70);
  std::vector<int> expo(70);
  FAILS_WITH(TNML_ERR_ARG, tnml_set_chain_scaling(nullptr, 1));
  FAILS_WITH(TNML_ERR_ARG, tnml_set_chain_scaling(ctx, 2));
  FAILS_WITH(TNML_ERR_ARG, tnml_set_chain_scaling(ctx, -1));
  FAILS_WITH(TNML_ERR_STATE, tnml_predict_scaled(ctx, X.data(), 70, mant.data(), expo.data()));        // cores never set
  set_cores(ctx, N, D, L, std::vector<int>(N - 1, M), 2);
  FAILS_WITH(TNML_ERR_STATE, tnml_predict_scaled(ctx, X.data(), 70, mant.data(), expo.data()));        // inner label, any_position off
  OK(tnml_set_chain_scaling(ctx, 1));
  FAILS_WITH(TNML_ERR_STATE, tnml_predict(ctx, X.data(), 70, f.data()));                               // the same rule with the switch on
  OK(tnml_set_any_position(ctx, 1));
  FAILS_WITH(TNML_ERR_ARG, tnml_predict_scaled(nullptr, X.data(), 70, mant.data(), expo.data()));
  FAILS_WITH(TNML_ERR_ARG, tnml_predict_scaled(ctx, nullptr, 70, mant.data(), expo.data()));
  FAILS_WITH(TNML_ERR_ARG, tnml_predict_scaled(ctx, X.data(), 70, nullptr, expo.data()));
  FAILS_WITH(TNML_ERR_ARG, tnml_predict_scaled(ctx, X.data(), 70, mant.data(), nullptr));
  FAILS_WITH(TNML_ERR_ARG, tnml_predict_scaled(ctx, X.data(), 0, mant.data(), expo.data()));
  OK(tnml_predict_scaled(ctx, X.data(), 70, mant.data(), expo.data()));                                // usable afterwards
  OK(tnml_predict(ctx, X.data(), 70, f.data()));
  OK(tnml_destroy(ctx));
  // a shape whose LDS tiles exceed 160 KB: refused with the bytes in the message, by the prediction and by both gradients
  OK(tnml_create(&ctx, 4, 2, 2, 100, 64, 0));
  const size_t t4 = set_cores(ctx, 4, 2, 2, std::vector<int>(3, 100), 0);
  std::vector<float> X4((size_t)4 * 4 * 2, 0.5f), G4(t4), m4(2 * 4), g4(4 * 4 * 2), cot4(2 * 4, 1.f);
  std::vector<int> e4(4);
  FAILS_WITH(TNML_ERR_ARG, tnml_predict_scaled(ctx, X4.data(), 4, m4.data(), e4.data()));
  if (!strstr(tnml_last_error(), "bytes of LDS")) { fprintf(stderr, "LDS refusal does not name the bytes: %s\n", tnml_last_error()); exit(1); }
  OK(tnml_set_chain_scaling(ctx, 1));
  FAILS_WITH(TNML_ERR_ARG, tnml_predict(ctx, X4.data(), 4, m4.data()));
  if (!strstr(tnml_last_error(), "bytes of LDS")) { fprintf(stderr, "LDS refusal does not name the bytes: %s\n", tnml_last_error()); exit(1); }
  FAILS_WITH(TNML_ERR_ARG, tnml_input_grad(ctx, X4.data(), 4, cot4.data(), g4.data(), nullptr));
  FAILS_WITH(TNML_ERR_ARG, tnml_core_grad(ctx, X4.data(), 4, cot4.data(), G4.data(), t4, nullptr));
  OK(tnml_destroy(ctx));
  // with a communicator the gradient calls are refused as before, whatever the switch says
  setenv("TNML_FORCE_COMM", "1", 1);
  OK(tnml_create(&ctx, N, D, L, M, 64, 0));
  unsigned char uid[128];
  OK(tnml_comm_unique_id(uid));
  OK(tnml_comm_init(ctx, 0, 1, uid));
  const size_t total = set_cores(ctx, N, D, L, std::vector<int>(N - 1, M), 0);
  OK(tnml_set_chain_scaling(ctx, 1));
  std::vector<float> G(total), g((size_t)70 * N * D), cot((size_t)L * 70, 1.f);
  std::vector<int> y(70, 0);
  FAILS_WITH(TNML_ERR_STATE, tnml_input_grad(ctx, X.data(), 70, cot.data(), g.data(), nullptr));
  FAILS_WITH(TNML_ERR_STATE, tnml_core_grad(ctx, X.data(), 70, cot.data(), G.data(), total, nullptr));
  FAILS_WITH(TNML_ERR_STATE, tnml_gd_step(ctx, X.data(), y.data(), 70, 1e-3f, 0.f, 0, 0, 1.f, nullptr));
  OK(tnml_destroy(ctx));
  unsetenv("TNML_FORCE_COMM");
  printf("scaled-chain refusals: ok\n");
}

// every allocation of the groups the switch enlarges fails in turn: the prediction group with its three scaled members (first
// use with the switch off, through tnml_predict_scaled; regrowth of a plain group once the switch is on; growth), and the two
// gradient groups with their exponent stacks
static void run_alloc_failures(int D) {
  const int N = 6, L = 2, M = 6;
  std::vector<float> X((size_t)300 * N * D, 0.5f), cot((size_t)L * 300, 1.f), g((size_t)300 * N * D), cf(300), f((size_t)L * 300), mant((size_t)L * 300);
  std::vector<int> expo(300);
  tnml_ctx *ctx = nullptr;
  OK(tnml_create(&ctx, N, D, L, M, 64, 0));
  OK(tnml_set_any_position(ctx, 1));
  const size_t total = set_cores(ctx, N, D, L, std::vector<int>(N - 1, M), 3);
  std::vector<float> G(total);
  int k = fail_each_alloc("tnml_predict_scaled, first use, b 70", [&] { return tnml_predict_scaled(ctx, X.data(), 70, mant.data(), expo.data()); });
  if (k != 8) { fprintf(stderr, "%d allocations failed in turn, the prediction group has 8 with its scaled members\n", k); exit(1); }
  OK(tnml_destroy(ctx));
  OK(tnml_create(&ctx, N, D, L, M, 64, 0));
  OK(tnml_set_any_position(ctx, 1));
  set_cores(ctx, N, D, L, std::vector<int>(N - 1, M), 3);
  // plain groups first, then the switch: every group is made again with its scaled members at the capacity it had
  OK(tnml_predict(ctx, X.data(), 70, f.data()));
  OK(tnml_input_grad(ctx, X.data(), 70, cot.data(), g.data(), cf.data()));
  OK(tnml_core_grad(ctx, X.data(), 70, cot.data(), G.data(), total, cf.data()));
  OK(tnml_set_chain_scaling(ctx, 1));
  k = fail_each_alloc("tnml_predict, switch on over a plain group", [&] { return tnml_predict(ctx, X.data(), 70, f.data()); });
  if (k != 8) { fprintf(stderr, "%d allocations failed in turn, the prediction group has 8 with its scaled members\n", k); exit(1); }
  k = fail_each_alloc("tnml_input_grad, switch on over a plain group", [&] { return tnml_input_grad(ctx, X.data(), 70, cot.data(), g.data(), cf.data()); });
  if (k != 7) { fprintf(stderr, "%d allocations failed in turn, the input-gradient group has 7 with its exponent stack\n", k); exit(1); }
  k = fail_each_alloc("tnml_core_grad, switch on over a plain group", [&] { return tnml_core_grad(ctx, X.data(), 70, cot.data(), G.data(), total, cf.data()); });
  if (k != 7) { fprintf(stderr, "%d allocations failed in turn, the core-gradient group has 7 with its exponent stack\n", k); exit(1); }
  fail_each_alloc("tnml_predict_scaled, b 70 -> 300", [&] { return tnml_predict_scaled(ctx, X.data(), 300, mant.data(), expo.data()); });
  fail_each_alloc("tnml_input_grad, b 70 -> 300", [&] { return tnml_input_grad(ctx, X.data(), 300, nullptr, g.data(), cf.data()); });
  fail_each_alloc("tnml_core_grad, b 70 -> 300", [&] { return tnml_core_grad(ctx, X.data(), 300, nullptr, G.data(), total, cf.data()); });
  OK(tnml_destroy(ctx));
}

int main() {
  run_true_size("c3", 784, 2, 2, 20, 5000, 0);
  run_true_size("c5", 784, 2, 10, 50, 5000, 783);
  run_true_size("c5 inner label", 784, 2, 10, 50, 200, 400);
  run_ragged(2, 3, 5);
  run_ragged(3, 3, 7);
  run_ragged(8, 17, 6);
  run_refusals();
  run_alloc_failures(2);
  run_alloc_failures(3);
  san_stub_report();
  for (const char *k : kScaled)
    if (san_stub_launches(k) < 1) { fprintf(stderr, "launch path %s was never taken\n", k); return 1; }
  printf("scaled chains: %ld scaled_pred_kernel, %ld input_grad_scaled_kernel and %ld core_grad_chain_scaled_kernel launches checked, %d refusals\n",
         san_stub_launches(kScaled[0]), san_stub_launches(kScaled[1]), san_stub_launches(kScaled[2]), g_refusals);
  printf("scaled-chain host planning under ASan + UBSan: ok\n");
  return 0;
}
