// Core gradients (tnml_core_grad / tnml_core_grad_indices / tnml_set_core_grad_chunk of tnml_api.hip and the launch wrappers of
// kernels_coregrad.hip) planned by the real host code, built --cuda-host-only with AddressSanitizer and UBSan, against the stand-in
// runtime of hip_stub.cpp, which checks every pointer of the two new kernels' parameter block together with the extent the kernel
// touches: both stacks, site-major X, cot, cf, every core through the uploaded table, the label core, and every core's part of G at
// the offset the flat layout gives it.  `make san-coregrad` builds and runs it; tests/test_core_grad_host.py runs `make san-coregrad`.
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

// one chain launch and one reduction launch per chunk
static void expect_launches(const char *what, long before_chain, long before_reduce, long want) {
  const long chain = san_stub_launches("core_grad_chain_kernel") - before_chain, red = san_stub_launches("core_grad_reduce_kernel") - before_reduce;
  if (chain != want || red != want) { fprintf(stderr, "%s: %ld chain and %ld reduction launches, expected %ld each\n", what, chain, red, want); exit(1); }
}

static size_t set_cores(tnml_ctx *ctx, int N, int D, int L, const std::vector<int> &bond, int l_pos) {
  size_t total = 0;
  for (int i = 0; i < N; ++i) total += (size_t)(i == 0 ? 1 : bond[i - 1]) * D * (i == N - 1 ? 1 : bond[i]) * (i == l_pos ? L : 1);
  std::vector<float> cores(total, 0.1f);
  OK(tnml_set_cores(ctx, cores.data(), total, bond.data(), l_pos));
  return total;
}

// C3 / C5 at true size: b = 5000 in the default chunk and in chunks of 64, dense cotangent and predicted class
static void run_true_size(const char *name, int N, int D, int L, int M, int b, int l_pos) {
  tnml_ctx *ctx = nullptr;
  OK(tnml_create(&ctx, N, D, L, M, 64, 0));
  const size_t total = set_cores(ctx, N, D, L, std::vector<int>(N - 1, M), l_pos);
  std::vector<float> X((size_t)b * N * D, 0.5f), cot((size_t)L * b, 1.f), G(total + 7), cf(b);
  const int def = (int)(((size_t)256 << 20) / ((size_t)N * M * 4) / 64 * 64);
  long bc = san_stub_launches("core_grad_chain_kernel"), br = san_stub_launches("core_grad_reduce_kernel");
  OK(tnml_core_grad(ctx, X.data(), b, cot.data(), G.data(), total, cf.data()));
  expect_launches("default chunk", bc, br, (b + def - 1) / def);
  bc = san_stub_launches("core_grad_chain_kernel"); br = san_stub_launches("core_grad_reduce_kernel");
  OK(tnml_core_grad(ctx, X.data(), b, nullptr, G.data(), total + 7, nullptr));
  expect_launches("default chunk, predicted class", bc, br, (b + def - 1) / def);
  OK(tnml_set_core_grad_chunk(ctx, 1));                // rounded up to 64
  bc = san_stub_launches("core_grad_chain_kernel"); br = san_stub_launches("core_grad_reduce_kernel");
  OK(tnml_core_grad(ctx, X.data(), b, cot.data(), G.data(), total, cf.data()));
  expect_launches("chunk 64", bc, br, (b + 63) / 64);
  OK(tnml_set_core_grad_chunk(ctx, 0));
  OK(tnml_core_grad(ctx, X.data(), 1, cot.data(), G.data(), total, cf.data()));
  OK(tnml_destroy(ctx));
  printf("planned core gradients %s bond %d L %d b %d (default chunk %d)\n", name, M, L, b, def);
  fflush(stdout);
}

// a ragged 17-site chain at every label position; b = 70 and b = 1, dense cotangent and predicted class (an inner label with
// tnml_set_any_position off), dataset samples with repeats
static void run_ragged(int D, int L, int M) {
  const int N = 17, n = 90;
  tnml_ctx *ctx = nullptr;
  OK(tnml_create(&ctx, N, D, L, M, 64, 0));
  std::vector<float> X((size_t)200 * N * D, 0.5f), cot((size_t)L * 200, 1.f), cf(200), G((size_t)N * D * M * M * L);
  std::vector<int> lab(n, 0), idx(200);
  for (int i = 0; i < 200; ++i) idx[i] = (i * 37) % n;                       // repeats included
  OK(tnml_dataset_attach(ctx, X.data(), lab.data(), n, N, D, TNML_DATASET_FEATURES));
  for (int l = 0; l < N; ++l) {
    std::vector<int> bond(N - 1);
    for (int i = 0; i < N - 1; ++i) bond[i] = 1 + (i * 7 + l * 3) % M;
    bond[(l * 5) % (N - 1)] = M;
    const size_t total = set_cores(ctx, N, D, L, bond, l);
    OK(tnml_core_grad(ctx, X.data(), 70, cot.data(), G.data(), total, cf.data()));
    OK(tnml_core_grad(ctx, X.data(), 70, nullptr, G.data(), total, cf.data()));
    OK(tnml_core_grad(ctx, X.data(), 1, cot.data(), G.data(), G.size(), nullptr));
    OK(tnml_core_grad_indices(ctx, idx.data(), 200, cot.data(), G.data(), total, cf.data()));
    OK(tnml_core_grad_indices(ctx, idx.data(), 1, nullptr, G.data(), total, cf.data()));
    FAILS_WITH(TNML_ERR_ARG, tnml_core_grad(ctx, X.data(), 70, cot.data(), G.data(), total - 1, cf.data()));
  }
  // a smaller chunk than the buffers hold, then the default again
  OK(tnml_set_core_grad_chunk(ctx, 64));
  OK(tnml_core_grad(ctx, X.data(), 200, cot.data(), G.data(), G.size(), cf.data()));
  OK(tnml_set_core_grad_chunk(ctx, 0));
  OK(tnml_core_grad(ctx, X.data(), 200, cot.data(), G.data(), G.size(), cf.data()));
  OK(tnml_destroy(ctx));
  printf("planned core gradients ragged N %d D %d L %d bond <= %d\n", N, D, L, M);
  fflush(stdout);
}

static void run_refusals() {
  const int N = 6, D = 2, L = 3, M = 4;
  tnml_ctx *ctx = nullptr;
  OK(tnml_create(&ctx, N, D, L, M, 64, 0));
  std::vector<float> X((size_t)70 * N * D, 0.5f), cot((size_t)L * 70, 1.f), G((size_t)N * D * M * M * L), cf(70);
  std::vector<int> lab(10, 0), idx = {0, 3, 9, 3};
  const size_t cap = G.size();
  FAILS_WITH(TNML_ERR_STATE, tnml_core_grad(ctx, X.data(), 70, cot.data(), G.data(), cap, cf.data()));             // cores never set
  const size_t total = set_cores(ctx, N, D, L, std::vector<int>(N - 1, M), 2);
  FAILS_WITH(TNML_ERR_ARG, tnml_core_grad(nullptr, X.data(), 70, cot.data(), G.data(), cap, cf.data()));
  FAILS_WITH(TNML_ERR_ARG, tnml_core_grad(ctx, nullptr, 70, cot.data(), G.data(), cap, cf.data()));
  FAILS_WITH(TNML_ERR_ARG, tnml_core_grad(ctx, X.data(), 70, cot.data(), nullptr, cap, cf.data()));
  FAILS_WITH(TNML_ERR_ARG, tnml_core_grad(ctx, X.data(), 0, cot.data(), G.data(), cap, cf.data()));
  FAILS_WITH(TNML_ERR_ARG, tnml_core_grad(ctx, X.data(), -3, cot.data(), G.data(), cap, cf.data()));
  FAILS_WITH(TNML_ERR_ARG, tnml_core_grad(ctx, X.data(), 70, cot.data(), G.data(), total - 1, cf.data()));         // capacity
  FAILS_WITH(TNML_ERR_ARG, tnml_core_grad(ctx, X.data(), 70, cot.data(), G.data(), 0, cf.data()));
  FAILS_WITH(TNML_ERR_ARG, tnml_set_core_grad_chunk(ctx, -1));
  FAILS_WITH(TNML_ERR_ARG, tnml_set_core_grad_chunk(nullptr, 64));
  FAILS_WITH(TNML_ERR_STATE, tnml_core_grad_indices(ctx, idx.data(), 4, cot.data(), G.data(), cap, cf.data()));    // no dataset
  OK(tnml_dataset_attach(ctx, X.data(), lab.data(), 10, N, D, TNML_DATASET_FEATURES));
  FAILS_WITH(TNML_ERR_ARG, tnml_core_grad_indices(nullptr, idx.data(), 4, cot.data(), G.data(), cap, cf.data()));
  FAILS_WITH(TNML_ERR_ARG, tnml_core_grad_indices(ctx, nullptr, 4, cot.data(), G.data(), cap, cf.data()));
  FAILS_WITH(TNML_ERR_ARG, tnml_core_grad_indices(ctx, idx.data(), 4, cot.data(), nullptr, cap, cf.data()));
  FAILS_WITH(TNML_ERR_ARG, tnml_core_grad_indices(ctx, idx.data(), 0, cot.data(), G.data(), cap, cf.data()));
  FAILS_WITH(TNML_ERR_ARG, tnml_core_grad_indices(ctx, idx.data(), 4, cot.data(), G.data(), total - 1, cf.data()));
  idx[2] = 10;
  FAILS_WITH(TNML_ERR_ARG, tnml_core_grad_indices(ctx, idx.data(), 4, cot.data(), G.data(), cap, cf.data()));
  idx[2] = -1;
  FAILS_WITH(TNML_ERR_ARG, tnml_core_grad_indices(ctx, idx.data(), 4, nullptr, G.data(), cap, cf.data()));
  idx[2] = 9;
  // the context is usable afterwards
  OK(tnml_core_grad_indices(ctx, idx.data(), 4, nullptr, G.data(), cap, cf.data()));
  OK(tnml_core_grad(ctx, X.data(), 70, cot.data(), G.data(), total, cf.data()));
  OK(tnml_destroy(ctx));
  // a shape whose LDS tiles exceed 160 KB: refused with the bytes in the message
  OK(tnml_create(&ctx, 4, 2, 2, 100, 64, 0));
  const size_t t4 = set_cores(ctx, 4, 2, 2, std::vector<int>(3, 100), 0);
  std::vector<float> X4((size_t)4 * 4 * 2, 0.5f), G4(t4);
  FAILS_WITH(TNML_ERR_ARG, tnml_core_grad(ctx, X4.data(), 4, nullptr, G4.data(), t4, nullptr));
  if (!strstr(tnml_last_error(), "bytes of LDS")) { fprintf(stderr, "LDS refusal does not name the bytes: %s\n", tnml_last_error()); exit(1); }
  OK(tnml_destroy(ctx));
  // with a communicator both calls are refused
  setenv("TNML_FORCE_COMM", "1", 1);
  OK(tnml_create(&ctx, N, D, L, M, 64, 0));
  unsigned char uid[128];
  OK(tnml_comm_unique_id(uid));
  OK(tnml_comm_init(ctx, 0, 1, uid));
  set_cores(ctx, N, D, L, std::vector<int>(N - 1, M), 0);
  FAILS_WITH(TNML_ERR_STATE, tnml_core_grad(ctx, X.data(), 70, cot.data(), G.data(), cap, cf.data()));
  FAILS_WITH(TNML_ERR_STATE, tnml_core_grad_indices(ctx, idx.data(), 4, cot.data(), G.data(), cap, cf.data()));
  OK(tnml_destroy(ctx));
  unsetenv("TNML_FORCE_COMM");
  printf("core-gradient refusals: ok\n");
}

// every allocation of the calls' groups (prediction group, core-gradient group, index list) fails in turn, at first use and at
// growth.  The prediction group is grown by tnml_predict first, so that every allocation counted below is one of the
// core-gradient group's six.  The input-gradient call in between shows the two groups do not share a member.
static void run_alloc_failures(int D) {
  const int N = 6, L = 2, M = 6, n = 50;
  tnml_ctx *ctx = nullptr;
  OK(tnml_create(&ctx, N, D, L, M, 64, 0));
  OK(tnml_set_any_position(ctx, 1));
  const size_t total = set_cores(ctx, N, D, L, std::vector<int>(N - 1, M), 3);
  std::vector<float> X((size_t)300 * N * D, 0.5f), cot((size_t)L * 300, 1.f), G(total), g((size_t)300 * N * D), cf(300), f((size_t)L * 300);
  std::vector<int> lab(n, 1), idx(300);
  for (int i = 0; i < 300; ++i) idx[i] = (i * 7) % n;
  fail_each_alloc("tnml_predict, b 70", [&] { return tnml_predict(ctx, X.data(), 70, f.data()); });
  int k = fail_each_alloc("tnml_core_grad, b 70", [&] { return tnml_core_grad(ctx, X.data(), 70, cot.data(), G.data(), total, cf.data()); });
  if (k != 6) { fprintf(stderr, "%d allocations failed in turn, the core-gradient group has 6\n", k); exit(1); }
  OK(tnml_input_grad(ctx, X.data(), 70, cot.data(), g.data(), cf.data()));
  fail_each_alloc("tnml_predict, b 70 -> 300", [&] { return tnml_predict(ctx, X.data(), 300, f.data()); });
  k = fail_each_alloc("tnml_core_grad, b 70 -> 300", [&] { return tnml_core_grad(ctx, X.data(), 300, nullptr, G.data(), total, cf.data()); });
  if (k != 6) { fprintf(stderr, "%d allocations failed in turn, the core-gradient group has 6\n", k); exit(1); }
  OK(tnml_dataset_attach(ctx, X.data(), lab.data(), n, N, D, TNML_DATASET_FEATURES));
  fail_each_alloc("tnml_core_grad_indices, first index list", [&] { return tnml_core_grad_indices(ctx, idx.data(), 300, nullptr, G.data(), total, cf.data()); });
  OK(tnml_set_core_grad_chunk(ctx, 640));
  fail_each_alloc("tnml_core_grad_indices, b 300", [&] { return tnml_core_grad_indices(ctx, idx.data(), 300, cot.data(), G.data(), total, cf.data()); });
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
  const char *paths[] = {"core_grad_chain_kernel", "core_grad_reduce_kernel", "input_grad_onehot_kernel"};
  for (const char *k : paths)
    if (san_stub_launches(k) < 1) { fprintf(stderr, "launch path %s was never taken\n", k); return 1; }
  printf("core gradients: %ld core_grad_chain_kernel and %ld core_grad_reduce_kernel launches checked, %d refusals\n",
         san_stub_launches("core_grad_chain_kernel"), san_stub_launches("core_grad_reduce_kernel"), g_refusals);
  printf("core-gradient host planning under ASan + UBSan: ok\n");
  return 0;
}
