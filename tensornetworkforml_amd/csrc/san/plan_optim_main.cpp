// Gradient training (tnml_optim_config / tnml_optim_reset / tnml_gd_train_indices / tnml_gd_step of tnml_api.hip and the launch
// wrappers of kernels_optim.hip) planned by the real host code, built --cuda-host-only with AddressSanitizer and UBSan, against the
// stand-in runtime of hip_stub.cpp, which checks both new parameter blocks: f and cot at their own strides, the labels, every core's
// slot and its part of G, vel, m and v through the uploaded table, and the grid against N.  `make san-optim` builds and runs it;
// tests/test_gradient_step_host.py runs `make san-optim`.
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

static const int kAct = TNML_ACT_SOFTMAX, kLoss = TNML_LOSS_FULL_CROSS_ENT;

struct Counts { long chain, reduce, cot, step, metrics; };
static Counts counts() {
  return {san_stub_launches("core_grad_chain_kernel"), san_stub_launches("core_grad_reduce_kernel"), san_stub_launches("loss_cot_kernel"),
          san_stub_launches("optim_step_kernel"), san_stub_launches("dataset_metrics_kernel")};
}
// one chain, reduction, loss-derivative and metrics launch per chunk, one optimiser launch per step
static void expect_launches(const char *what, const Counts &a, long chunks, long steps) {
  const Counts b = counts();
  if (b.chain - a.chain != chunks || b.reduce - a.reduce != chunks || b.cot - a.cot != chunks || b.metrics - a.metrics != chunks || b.step - a.step != steps) {
    fprintf(stderr, "%s: %ld chain, %ld reduction, %ld loss-derivative, %ld metrics launches (expected %ld each), %ld optimiser launches (expected %ld)\n",
            what, b.chain - a.chain, b.reduce - a.reduce, b.cot - a.cot, b.metrics - a.metrics, chunks, b.step - a.step, steps);
    exit(1);
  }
}

static size_t set_cores(tnml_ctx *ctx, int N, int D, int L, const std::vector<int> &bond, int l_pos) {
  size_t total = 0;
  for (int i = 0; i < N; ++i) total += (size_t)(i == 0 ? 1 : bond[i - 1]) * D * (i == N - 1 ? 1 : bond[i]) * (i == l_pos ? L : 1);
  std::vector<float> cores(total, 0.1f);
  OK(tnml_set_cores(ctx, cores.data(), total, bond.data(), l_pos));
  return total;
}

static void config(tnml_ctx *ctx, int which) {       // 0 plain SGD with the clip, 1 SGD with momentum, 2 Adam
  if (which == 0) OK(tnml_optim_config(ctx, TNML_OPT_SGD, 0.0, 0.9, 0.999, 1e-8, 1));
  else if (which == 1) OK(tnml_optim_config(ctx, TNML_OPT_SGD, 0.9, 0.9, 0.999, 1e-8, 0));
  else OK(tnml_optim_config(ctx, TNML_OPT_ADAM, 0.0, 0.9, 0.999, 1e-3, 0));
}

// C3 / C5 at true size: a batch of b in the default chunk and in chunks of 64, an epoch of several batches with a ragged last one
static void run_true_size(const char *name, int N, int D, int L, int M, int b, int l_pos) {
  const int n = 300;
  tnml_ctx *ctx = nullptr;
  OK(tnml_create(&ctx, N, D, L, M, 64, 0));
  set_cores(ctx, N, D, L, std::vector<int>(N - 1, M), l_pos);
  std::vector<float> X((size_t)n * N * D, 0.5f);
  std::vector<int> lab(n), idx(2 * b + 17);
  for (int i = 0; i < n; ++i) lab[i] = i % L;
  for (size_t i = 0; i < idx.size(); ++i) idx[i] = (int)((i * 37) % n);
  OK(tnml_dataset_attach(ctx, X.data(), lab.data(), n, N, D, TNML_DATASET_FEATURES));
  const int def = (int)(((size_t)256 << 20) / ((size_t)N * M * 4) / 64 * 64);
  std::vector<double> met(3 * 3);
  for (int which = 0; which < 3; ++which) {
    config(ctx, which);
    Counts a = counts();
    OK(tnml_gd_train_indices(ctx, idx.data(), b, b, 0.5f, 1e-3f, kAct, kLoss, 0.1f, met.data()));
    expect_launches("default chunk", a, (b + def - 1) / def, 1);
  }
  // three steps, the last ragged (17 samples)
  Counts a = counts();
  OK(tnml_gd_train_indices(ctx, idx.data(), 2 * b + 17, b, 0.5f, 0.f, kAct, kLoss, 0.1f, met.data()));
  expect_launches("epoch of three batches", a, 2 * ((b + def - 1) / def) + 1, 3);
  OK(tnml_set_core_grad_chunk(ctx, 1));                // rounded up to 64
  a = counts();
  OK(tnml_gd_train_indices(ctx, idx.data(), b, b, 0.5f, 1e-3f, kAct, kLoss, 0.1f, nullptr));
  expect_launches("chunk 64", a, (b + 63) / 64, 1);
  OK(tnml_set_core_grad_chunk(ctx, 0));
  OK(tnml_gd_train_indices(ctx, idx.data(), 1, 1, 0.5f, 1e-3f, kAct, kLoss, 0.1f, met.data()));
  OK(tnml_destroy(ctx));
  printf("planned gradient training %s bond %d L %d b %d (default chunk %d)\n", name, M, L, b, def);
  fflush(stdout);
}

// a ragged 17-site chain at every label position: the three optimisers, dataset batches with repeats, a host batch, b = 70 and 1,
// several steps with a ragged last batch, chunks of 64
static void run_ragged(int D, int L, int M) {
  const int N = 17, n = 90;
  tnml_ctx *ctx = nullptr;
  OK(tnml_create(&ctx, N, D, L, M, 64, 0));
  std::vector<float> X((size_t)200 * N * D, 0.5f);
  std::vector<int> lab(200), idx(250);
  for (int i = 0; i < 200; ++i) lab[i] = i % L;
  for (int i = 0; i < 250; ++i) idx[i] = (i * 37) % n;                       // repeats included
  std::vector<double> met(3 * 4);
  OK(tnml_dataset_attach(ctx, X.data(), lab.data(), n, N, D, TNML_DATASET_FEATURES));
  for (int l = 0; l < N; ++l) {
    std::vector<int> bond(N - 1);
    for (int i = 0; i < N - 1; ++i) bond[i] = 1 + (i * 7 + l * 3) % M;
    bond[(l * 5) % (N - 1)] = M;
    set_cores(ctx, N, D, L, bond, l);
    for (int which = 0; which < 3; ++which) {
      config(ctx, which);
      const Counts a = counts();
      OK(tnml_gd_train_indices(ctx, idx.data(), 250, 70, 0.5f, 1e-3f, which, which, 0.5f, met.data()));     // 70, 70, 70, 40
      expect_launches("ragged epoch", a, 4, 4);
      OK(tnml_gd_step(ctx, X.data(), lab.data(), 70, 0.5f, 0.f, kAct, kLoss, 0.1f, met.data()));
      OK(tnml_gd_step(ctx, X.data(), lab.data(), 1, 0.5f, 0.f, kAct, kLoss, 0.1f, nullptr));
      OK(tnml_gd_train_indices(ctx, idx.data(), 1, 70, 0.5f, 0.f, kAct, kLoss, 0.1f, met.data()));
    }
  }
  // a smaller chunk than the buffers hold, then the default again
  OK(tnml_set_core_grad_chunk(ctx, 64));
  OK(tnml_gd_step(ctx, X.data(), lab.data(), 200, 0.5f, 0.f, kAct, kLoss, 0.1f, met.data()));
  OK(tnml_set_core_grad_chunk(ctx, 0));
  OK(tnml_gd_step(ctx, X.data(), lab.data(), 200, 0.5f, 0.f, kAct, kLoss, 0.1f, met.data()));
  OK(tnml_destroy(ctx));
  printf("planned gradient training ragged N %d D %d L %d bond <= %d\n", N, D, L, M);
  fflush(stdout);
}

static void run_refusals() {
  const int N = 6, D = 2, L = 3, M = 4;
  tnml_ctx *ctx = nullptr;
  OK(tnml_create(&ctx, N, D, L, M, 64, 0));
  std::vector<float> X((size_t)70 * N * D, 0.5f);
  std::vector<int> lab(70, 1), idx = {0, 3, 9, 3};
  double met[12];
  // tnml_optim_config
  FAILS_WITH(TNML_ERR_ARG, tnml_optim_config(nullptr, TNML_OPT_SGD, 0.0, 0.9, 0.999, 1e-8, 1));
  FAILS_WITH(TNML_ERR_ARG, tnml_optim_config(ctx, 2, 0.0, 0.9, 0.999, 1e-8, 1));
  FAILS_WITH(TNML_ERR_ARG, tnml_optim_config(ctx, -1, 0.0, 0.9, 0.999, 1e-8, 0));
  FAILS_WITH(TNML_ERR_ARG, tnml_optim_config(ctx, TNML_OPT_SGD, -0.1, 0.9, 0.999, 1e-8, 1));
  FAILS_WITH(TNML_ERR_ARG, tnml_optim_config(ctx, TNML_OPT_SGD, 1.0, 0.9, 0.999, 1e-8, 1));
  FAILS_WITH(TNML_ERR_ARG, tnml_optim_config(ctx, TNML_OPT_ADAM, 0.0, 1.0, 0.999, 1e-8, 0));
  FAILS_WITH(TNML_ERR_ARG, tnml_optim_config(ctx, TNML_OPT_ADAM, 0.0, 0.9, -0.5, 1e-8, 0));
  FAILS_WITH(TNML_ERR_ARG, tnml_optim_config(ctx, TNML_OPT_ADAM, 0.0, 0.9, 0.999, 0.0, 0));
  FAILS_WITH(TNML_ERR_ARG, tnml_optim_config(ctx, TNML_OPT_ADAM, 0.0, 0.9, 0.999, -1e-8, 0));
  FAILS_WITH(TNML_ERR_ARG, tnml_optim_config(ctx, TNML_OPT_ADAM, 0.0, 0.9, 0.999, 1e-8, 1));       // Adam has no clip
  FAILS_WITH(TNML_ERR_ARG, tnml_optim_config(ctx, TNML_OPT_SGD, 0.0, 0.9, 0.999, 1e-8, 2));
  FAILS_WITH(TNML_ERR_ARG, tnml_optim_reset(nullptr));
  // the steps
  FAILS_WITH(TNML_ERR_STATE, tnml_gd_train_indices(ctx, idx.data(), 4, 2, 0.1f, 0.f, kAct, kLoss, 0.1f, met));          // no dataset
  FAILS_WITH(TNML_ERR_STATE, tnml_gd_step(ctx, X.data(), lab.data(), 70, 0.1f, 0.f, kAct, kLoss, 0.1f, met));           // cores never set
  OK(tnml_dataset_attach(ctx, X.data(), lab.data(), 10, N, D, TNML_DATASET_FEATURES));
  FAILS_WITH(TNML_ERR_STATE, tnml_gd_train_indices(ctx, idx.data(), 4, 2, 0.1f, 0.f, kAct, kLoss, 0.1f, met));          // cores never set
  set_cores(ctx, N, D, L, std::vector<int>(N - 1, M), 2);
  FAILS_WITH(TNML_ERR_ARG, tnml_gd_train_indices(nullptr, idx.data(), 4, 2, 0.1f, 0.f, kAct, kLoss, 0.1f, met));
  FAILS_WITH(TNML_ERR_ARG, tnml_gd_train_indices(ctx, nullptr, 4, 2, 0.1f, 0.f, kAct, kLoss, 0.1f, met));
  FAILS_WITH(TNML_ERR_ARG, tnml_gd_train_indices(ctx, idx.data(), 0, 2, 0.1f, 0.f, kAct, kLoss, 0.1f, met));
  FAILS_WITH(TNML_ERR_ARG, tnml_gd_train_indices(ctx, idx.data(), -4, 2, 0.1f, 0.f, kAct, kLoss, 0.1f, met));
  FAILS_WITH(TNML_ERR_ARG, tnml_gd_train_indices(ctx, idx.data(), 4, 0, 0.1f, 0.f, kAct, kLoss, 0.1f, met));
  FAILS_WITH(TNML_ERR_ARG, tnml_gd_train_indices(ctx, idx.data(), 4, -1, 0.1f, 0.f, kAct, kLoss, 0.1f, met));
  FAILS_WITH(TNML_ERR_ARG, tnml_gd_train_indices(ctx, idx.data(), 4, 2, 0.1f, 0.f, 3, kLoss, 0.1f, met));
  FAILS_WITH(TNML_ERR_ARG, tnml_gd_train_indices(ctx, idx.data(), 4, 2, 0.1f, 0.f, kAct, -1, 0.1f, met));
  FAILS_WITH(TNML_ERR_ARG, tnml_gd_train_indices(ctx, idx.data(), 4, 2, 0.1f, 0.f, kAct, 3, 0.1f, met));
  idx[2] = 10;
  FAILS_WITH(TNML_ERR_ARG, tnml_gd_train_indices(ctx, idx.data(), 4, 2, 0.1f, 0.f, kAct, kLoss, 0.1f, met));
  idx[2] = -1;
  FAILS_WITH(TNML_ERR_ARG, tnml_gd_train_indices(ctx, idx.data(), 4, 2, 0.1f, 0.f, kAct, kLoss, 0.1f, nullptr));
  idx[2] = 9;
  FAILS_WITH(TNML_ERR_ARG, tnml_gd_step(nullptr, X.data(), lab.data(), 70, 0.1f, 0.f, kAct, kLoss, 0.1f, met));
  FAILS_WITH(TNML_ERR_ARG, tnml_gd_step(ctx, nullptr, lab.data(), 70, 0.1f, 0.f, kAct, kLoss, 0.1f, met));
  FAILS_WITH(TNML_ERR_ARG, tnml_gd_step(ctx, X.data(), nullptr, 70, 0.1f, 0.f, kAct, kLoss, 0.1f, met));
  FAILS_WITH(TNML_ERR_ARG, tnml_gd_step(ctx, X.data(), lab.data(), 0, 0.1f, 0.f, kAct, kLoss, 0.1f, met));
  FAILS_WITH(TNML_ERR_ARG, tnml_gd_step(ctx, X.data(), lab.data(), 70, 0.1f, 0.f, 7, kLoss, 0.1f, met));
  lab[5] = L;
  FAILS_WITH(TNML_ERR_ARG, tnml_gd_step(ctx, X.data(), lab.data(), 70, 0.1f, 0.f, kAct, kLoss, 0.1f, met));
  lab[5] = -1;
  FAILS_WITH(TNML_ERR_ARG, tnml_gd_step(ctx, X.data(), lab.data(), 70, 0.1f, 0.f, kAct, kLoss, 0.1f, met));
  lab[5] = 1;
  // the context is usable afterwards
  OK(tnml_gd_train_indices(ctx, idx.data(), 4, 3, 0.1f, 0.f, kAct, kLoss, 0.1f, met));
  OK(tnml_gd_step(ctx, X.data(), lab.data(), 70, 0.1f, 0.f, kAct, kLoss, 0.1f, met));
  OK(tnml_destroy(ctx));
  // a shape whose LDS tiles exceed 160 KB: refused with the bytes in the message
  OK(tnml_create(&ctx, 4, 2, 2, 100, 64, 0));
  set_cores(ctx, 4, 2, 2, std::vector<int>(3, 100), 0);
  std::vector<float> X4((size_t)4 * 4 * 2, 0.5f);
  std::vector<int> y4(4, 0);
  FAILS_WITH(TNML_ERR_ARG, tnml_gd_step(ctx, X4.data(), y4.data(), 4, 0.1f, 0.f, kAct, kLoss, 0.1f, met));
  if (!strstr(tnml_last_error(), "bytes of LDS")) { fprintf(stderr, "LDS refusal does not name the bytes: %s\n", tnml_last_error()); exit(1); }
  OK(tnml_destroy(ctx));
  // with a communicator both calls are refused
  setenv("TNML_FORCE_COMM", "1", 1);
  OK(tnml_create(&ctx, N, D, L, M, 64, 0));
  unsigned char uid[128];
  OK(tnml_comm_unique_id(uid));
  OK(tnml_comm_init(ctx, 0, 1, uid));
  set_cores(ctx, N, D, L, std::vector<int>(N - 1, M), 0);
  FAILS_WITH(TNML_ERR_STATE, tnml_gd_step(ctx, X.data(), lab.data(), 70, 0.1f, 0.f, kAct, kLoss, 0.1f, met));
  FAILS_WITH(TNML_ERR_STATE, tnml_gd_train_indices(ctx, idx.data(), 4, 2, 0.1f, 0.f, kAct, kLoss, 0.1f, met));
  OK(tnml_destroy(ctx));
  unsetenv("TNML_FORCE_COMM");
  printf("gradient-training refusals: ok\n");
}

// the state is bound to the bonds and l_pos of its first step: after a planned sweep (l_pos moves, bonds change) a stateful step is
// refused until tnml_optim_reset, plain SGD is accepted; a step leaves the context as tnml_scale_cores does (no sweep without a forward)
static void run_state_rule() {
  const int N = 8, D = 2, L = 2, M = 4, b = 40;
  tnml_ctx *ctx = nullptr;
  OK(tnml_create(&ctx, N, D, L, M, 64, 0));
  std::vector<float> X((size_t)b * N * D, 0.5f), f((size_t)L * b);
  std::vector<int> lab(b, 1);
  double met[3];
  for (int which = 1; which < 3; ++which) {
    set_cores(ctx, N, D, L, std::vector<int>(N - 1, 2), 0);
    config(ctx, which);
    OK(tnml_gd_step(ctx, X.data(), lab.data(), b, 0.1f, 0.f, kAct, kLoss, 0.1f, met));
    OK(tnml_set_input(ctx, X.data(), lab.data(), b));
    FAILS_WITH(TNML_ERR_STATE, tnml_sweep(ctx, 0, N - 1, 1, 1e-3f, 1e-3f, 1, kAct, kLoss, 0.1f, TNML_TRUNC_FIXED, nullptr, nullptr));
    OK(tnml_forward(ctx, f.data()));
    OK(tnml_gd_step(ctx, X.data(), lab.data(), b, 0.1f, 0.f, kAct, kLoss, 0.1f, met));
    FAILS_WITH(TNML_ERR_STATE, tnml_sweep(ctx, 0, N - 1, 1, 1e-3f, 1e-3f, 1, kAct, kLoss, 0.1f, TNML_TRUNC_FIXED, nullptr, nullptr));
    OK(tnml_forward(ctx, f.data()));
    OK(tnml_sweep(ctx, 0, N - 1, 1, 1e-3f, 1e-3f, 1, kAct, kLoss, 0.1f, TNML_TRUNC_FIXED, nullptr, nullptr));
    if (tnml_l_pos(ctx) != N - 1) { fprintf(stderr, "the planned sweep left l_pos at %d\n", tnml_l_pos(ctx)); exit(1); }
    FAILS_WITH(TNML_ERR_STATE, tnml_gd_step(ctx, X.data(), lab.data(), b, 0.1f, 0.f, kAct, kLoss, 0.1f, met));
    if (!strstr(tnml_last_error(), "tnml_optim_reset")) { fprintf(stderr, "the refusal does not name tnml_optim_reset: %s\n", tnml_last_error()); exit(1); }
    OK(tnml_optim_reset(ctx));
    OK(tnml_gd_step(ctx, X.data(), lab.data(), b, 0.1f, 0.f, kAct, kLoss, 0.1f, met));
    // plain SGD has no state: accepted where the stateful optimiser was refused
    OK(tnml_forward(ctx, f.data()));
    OK(tnml_sweep(ctx, 1, N - 1, 1, 1e-3f, 1e-3f, 1, kAct, kLoss, 0.1f, TNML_TRUNC_FIXED, nullptr, nullptr));
    FAILS_WITH(TNML_ERR_STATE, tnml_gd_step(ctx, X.data(), lab.data(), b, 0.1f, 0.f, kAct, kLoss, 0.1f, met));
    config(ctx, 0);
    OK(tnml_gd_step(ctx, X.data(), lab.data(), b, 0.1f, 0.f, kAct, kLoss, 0.1f, met));
  }
  OK(tnml_destroy(ctx));
  printf("optimiser state rule after a planned sweep: ok\n");
}

// every allocation of the call's groups fails in turn.  The prediction, core-gradient and metrics groups are grown by the plain-SGD
// step first, so that every allocation counted for the stateful step is one of the state group's two.
static void run_alloc_failures(int D) {
  const int N = 6, L = 2, M = 6, n = 50;
  tnml_ctx *ctx = nullptr;
  OK(tnml_create(&ctx, N, D, L, M, 64, 0));
  set_cores(ctx, N, D, L, std::vector<int>(N - 1, M), 3);
  std::vector<float> X((size_t)300 * N * D, 0.5f);
  std::vector<int> lab(300, 1), idx(300);
  for (int i = 0; i < 300; ++i) idx[i] = (i * 7) % n;
  double met[3 * 8];
  fail_each_alloc("tnml_gd_step, plain SGD, b 70", [&] { return tnml_gd_step(ctx, X.data(), lab.data(), 70, 0.1f, 0.f, kAct, kLoss, 0.1f, met); });
  config(ctx, 1);
  int k = fail_each_alloc("tnml_gd_step, momentum, b 70", [&] { return tnml_gd_step(ctx, X.data(), lab.data(), 70, 0.1f, 0.f, kAct, kLoss, 0.1f, met); });
  if (k != 2) { fprintf(stderr, "%d allocations failed in turn, the state group has 2\n", k); exit(1); }
  config(ctx, 2);
  k = fail_each_alloc("tnml_gd_step, Adam after momentum", [&] { return tnml_gd_step(ctx, X.data(), lab.data(), 70, 0.1f, 0.f, kAct, kLoss, 0.1f, met); });
  if (k != 0) { fprintf(stderr, "%d allocations for Adam after momentum: the state group exists\n", k); exit(1); }
  fail_each_alloc("tnml_gd_step, b 70 -> 300", [&] { return tnml_gd_step(ctx, X.data(), lab.data(), 300, 0.1f, 0.f, kAct, kLoss, 0.1f, met); });
  OK(tnml_dataset_attach(ctx, X.data(), lab.data(), n, N, D, TNML_DATASET_FEATURES));
  fail_each_alloc("tnml_gd_train_indices, 8 steps", [&] { return tnml_gd_train_indices(ctx, idx.data(), 300, 40, 0.1f, 0.f, kAct, kLoss, 0.1f, met); });
  OK(tnml_destroy(ctx));
  // a fresh context whose first step is Adam's: every group of the call at first use
  OK(tnml_create(&ctx, N, D, L, M, 64, 0));
  set_cores(ctx, N, D, L, std::vector<int>(N - 1, M), 0);
  config(ctx, 2);
  fail_each_alloc("tnml_gd_step, Adam, fresh context", [&] { return tnml_gd_step(ctx, X.data(), lab.data(), 70, 0.1f, 0.f, kAct, kLoss, 0.1f, met); });
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
  run_state_rule();
  run_alloc_failures(2);
  run_alloc_failures(3);
  san_stub_report();
  const char *paths[] = {"loss_cot_kernel", "optim_step_kernel", "core_grad_chain_kernel", "core_grad_reduce_kernel", "dataset_metrics_kernel"};
  for (const char *k : paths)
    if (san_stub_launches(k) < 1) { fprintf(stderr, "launch path %s was never taken\n", k); return 1; }
  printf("gradient training: %ld loss_cot_kernel and %ld optim_step_kernel launches checked, %d refusals\n", san_stub_launches("loss_cot_kernel"),
         san_stub_launches("optim_step_kernel"), g_refusals);
  printf("gradient-training host planning under ASan + UBSan: ok\n");
  return 0;
}
