// Input gradients (tnml_input_grad / tnml_input_grad_indices / tnml_set_input_grad_chunk of tnml_api.hip and the launch wrappers of
// kernels_inputgrad.hip) planned by the real host code, built --cuda-host-only with AddressSanitizer and UBSan, against the stand-in
// runtime of hip_stub.cpp, which checks every pointer of the new kernels' parameter blocks together with the extent the kernel
// touches: stack, site-major X, cot, g, cf, every core through the uploaded bond table, the label core.  `make san-inputgrad`
// builds and runs it; tests/test_input_grad_host.py runs `make san-inputgrad`.
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

static void expect_launches(const char *what, long before, long want) {
  const long got = san_stub_launches("input_grad_kernel") - before;
  if (got != want) { fprintf(stderr, "%s: %ld input_grad_kernel launches, expected %ld\n", what, got, want); exit(1); }
}

static void set_cores(tnml_ctx *ctx, int N, int D, int L, const std::vector<int> &bond, int l_pos) {
  size_t total = 0;
  for (int i = 0; i < N; ++i) total += (size_t)(i == 0 ? 1 : bond[i - 1]) * D * (i == N - 1 ? 1 : bond[i]) * (i == l_pos ? L : 1);
  std::vector<float> cores(total, 0.1f);
  OK(tnml_set_cores(ctx, cores.data(), total, bond.data(), l_pos));
}

// C3 / C5 at true size: b = 5000 with the default chunk and with chunk 64, dense cotangent and predicted class
static void run_true_size(const char *name, int N, int D, int L, int M, int b, int l_pos) {
  tnml_ctx *ctx = nullptr;
  OK(tnml_create(&ctx, N, D, L, M, 64, 0));
  set_cores(ctx, N, D, L, std::vector<int>(N - 1, M), l_pos);
  std::vector<float> X((size_t)b * N * D, 0.5f), cot((size_t)L * b, 1.f), g((size_t)b * N * D), cf(b);
  const int def = (int)(((size_t)256 << 20) / ((size_t)N * M * 4) / 64 * 64);
  long before = san_stub_launches("input_grad_kernel");
  OK(tnml_input_grad(ctx, X.data(), b, cot.data(), g.data(), cf.data()));
  expect_launches("default chunk", before, (b + def - 1) / def);
  before = san_stub_launches("input_grad_kernel");
  OK(tnml_input_grad(ctx, X.data(), b, nullptr, g.data(), nullptr));
  expect_launches("default chunk, predicted class", before, (b + def - 1) / def);
  OK(tnml_set_input_grad_chunk(ctx, 1));               // rounded up to 64
  before = san_stub_launches("input_grad_kernel");
  OK(tnml_input_grad(ctx, X.data(), b, cot.data(), g.data(), cf.data()));
  expect_launches("chunk 64", before, (b + 63) / 64);
  OK(tnml_set_input_grad_chunk(ctx, 0));
  OK(tnml_input_grad(ctx, X.data(), 1, cot.data(), g.data(), cf.data()));
  OK(tnml_destroy(ctx));
  printf("planned input gradients %s bond %d L %d b %d (default chunk %d)\n", name, M, L, b, def);
  fflush(stdout);
}

// a ragged 17-site chain at every label position; b = 70 and b = 1, dense cotangent and predicted class (an inner label with
// tnml_set_any_position off), both dataset forms
static void run_ragged(int D, int L, int M) {
  const int N = 17, n = 90;
  tnml_ctx *ctx = nullptr;
  OK(tnml_create(&ctx, N, D, L, M, 64, 0));
  std::vector<float> X((size_t)200 * N * D, 0.5f), cot((size_t)L * 200, 1.f), g((size_t)200 * N * D), cf(200), pix((size_t)n * N, 0.25f);
  std::vector<int> lab(n, 0), idx(200);
  for (int i = 0; i < 200; ++i) idx[i] = (i * 37) % n;                       // repeats included
  for (int form : {TNML_DATASET_FEATURES, TNML_DATASET_PIXELS}) {
    OK(tnml_dataset_attach(ctx, form == TNML_DATASET_PIXELS ? pix.data() : X.data(), lab.data(), n, N, D, form));
    for (int l = 0; l < N; ++l) {
      std::vector<int> bond(N - 1);
      for (int i = 0; i < N - 1; ++i) bond[i] = 1 + (i * 7 + l * 3) % M;
      bond[(l * 5) % (N - 1)] = M;
      set_cores(ctx, N, D, L, bond, l);
      OK(tnml_input_grad(ctx, X.data(), 70, cot.data(), g.data(), cf.data()));
      OK(tnml_input_grad(ctx, X.data(), 70, nullptr, g.data(), cf.data()));
      OK(tnml_input_grad(ctx, X.data(), 1, cot.data(), g.data(), nullptr));
      OK(tnml_input_grad_indices(ctx, idx.data(), 200, cot.data(), TNML_WRT_FEATURES, g.data(), cf.data()));
      OK(tnml_input_grad_indices(ctx, idx.data(), 1, nullptr, TNML_WRT_FEATURES, g.data(), cf.data()));
      if (form == TNML_DATASET_PIXELS) OK(tnml_input_grad_indices(ctx, idx.data(), 200, nullptr, TNML_WRT_PIXELS, g.data(), cf.data()));
      else FAILS_WITH(TNML_ERR_STATE, tnml_input_grad_indices(ctx, idx.data(), 200, cot.data(), TNML_WRT_PIXELS, g.data(), cf.data()));
    }
  }
  // a smaller chunk than the buffers hold, then the default again
  OK(tnml_set_input_grad_chunk(ctx, 64));
  OK(tnml_input_grad(ctx, X.data(), 200, cot.data(), g.data(), cf.data()));
  OK(tnml_set_input_grad_chunk(ctx, 0));
  OK(tnml_input_grad(ctx, X.data(), 200, cot.data(), g.data(), cf.data()));
  OK(tnml_destroy(ctx));
  printf("planned input gradients ragged N %d D %d L %d bond <= %d\n", N, D, L, M);
  fflush(stdout);
}

static void run_refusals() {
  const int N = 6, D = 2, L = 3, M = 4;
  tnml_ctx *ctx = nullptr;
  OK(tnml_create(&ctx, N, D, L, M, 64, 0));
  std::vector<float> X((size_t)70 * N * D, 0.5f), cot((size_t)L * 70, 1.f), g((size_t)70 * N * D), cf(70);
  std::vector<int> lab(10, 0), idx = {0, 3, 9, 3};
  FAILS_WITH(TNML_ERR_STATE, tnml_input_grad(ctx, X.data(), 70, cot.data(), g.data(), cf.data()));            // cores never set
  set_cores(ctx, N, D, L, std::vector<int>(N - 1, M), 2);
  FAILS_WITH(TNML_ERR_ARG, tnml_input_grad(nullptr, X.data(), 70, cot.data(), g.data(), cf.data()));
  FAILS_WITH(TNML_ERR_ARG, tnml_input_grad(ctx, nullptr, 70, cot.data(), g.data(), cf.data()));
  FAILS_WITH(TNML_ERR_ARG, tnml_input_grad(ctx, X.data(), 70, cot.data(), nullptr, cf.data()));
  FAILS_WITH(TNML_ERR_ARG, tnml_input_grad(ctx, X.data(), 0, cot.data(), g.data(), cf.data()));
  FAILS_WITH(TNML_ERR_ARG, tnml_input_grad(ctx, X.data(), -3, cot.data(), g.data(), cf.data()));
  FAILS_WITH(TNML_ERR_ARG, tnml_set_input_grad_chunk(ctx, -1));
  FAILS_WITH(TNML_ERR_STATE, tnml_input_grad_indices(ctx, idx.data(), 4, cot.data(), TNML_WRT_FEATURES, g.data(), cf.data()));   // no dataset
  OK(tnml_dataset_attach(ctx, X.data(), lab.data(), 10, N, D, TNML_DATASET_FEATURES));
  FAILS_WITH(TNML_ERR_STATE, tnml_input_grad_indices(ctx, idx.data(), 4, cot.data(), TNML_WRT_PIXELS, g.data(), cf.data()));
  FAILS_WITH(TNML_ERR_ARG, tnml_input_grad_indices(ctx, idx.data(), 4, cot.data(), 2, g.data(), cf.data()));
  FAILS_WITH(TNML_ERR_ARG, tnml_input_grad_indices(ctx, nullptr, 4, cot.data(), TNML_WRT_FEATURES, g.data(), cf.data()));
  FAILS_WITH(TNML_ERR_ARG, tnml_input_grad_indices(ctx, idx.data(), 4, cot.data(), TNML_WRT_FEATURES, nullptr, cf.data()));
  FAILS_WITH(TNML_ERR_ARG, tnml_input_grad_indices(ctx, idx.data(), 0, cot.data(), TNML_WRT_FEATURES, g.data(), cf.data()));
  idx[2] = 10;
  FAILS_WITH(TNML_ERR_ARG, tnml_input_grad_indices(ctx, idx.data(), 4, cot.data(), TNML_WRT_FEATURES, g.data(), cf.data()));
  idx[2] = -1;
  FAILS_WITH(TNML_ERR_ARG, tnml_input_grad_indices(ctx, idx.data(), 4, nullptr, TNML_WRT_FEATURES, g.data(), cf.data()));
  idx[2] = 9;
  // the context is usable afterwards
  OK(tnml_input_grad_indices(ctx, idx.data(), 4, nullptr, TNML_WRT_FEATURES, g.data(), cf.data()));
  OK(tnml_input_grad(ctx, X.data(), 70, cot.data(), g.data(), cf.data()));
  OK(tnml_destroy(ctx));
  // a shape whose LDS tiles exceed 160 KB: refused with the bytes in the message
  OK(tnml_create(&ctx, 4, 2, 2, 100, 64, 0));
  set_cores(ctx, 4, 2, 2, std::vector<int>(3, 100), 0);
  std::vector<float> X4((size_t)4 * 4 * 2, 0.5f), g4(X4.size());
  FAILS_WITH(TNML_ERR_ARG, tnml_input_grad(ctx, X4.data(), 4, nullptr, g4.data(), nullptr));
  if (!strstr(tnml_last_error(), "bytes of LDS")) { fprintf(stderr, "LDS refusal does not name the bytes: %s\n", tnml_last_error()); exit(1); }
  OK(tnml_destroy(ctx));
  // with a communicator both calls are refused
  setenv("TNML_FORCE_COMM", "1", 1);
  OK(tnml_create(&ctx, N, D, L, M, 64, 0));
  unsigned char uid[128];
  OK(tnml_comm_unique_id(uid));
  OK(tnml_comm_init(ctx, 0, 1, uid));
  set_cores(ctx, N, D, L, std::vector<int>(N - 1, M), 0);
  FAILS_WITH(TNML_ERR_STATE, tnml_input_grad(ctx, X.data(), 70, cot.data(), g.data(), cf.data()));
  FAILS_WITH(TNML_ERR_STATE, tnml_input_grad_indices(ctx, idx.data(), 4, cot.data(), TNML_WRT_FEATURES, g.data(), cf.data()));
  OK(tnml_destroy(ctx));
  unsetenv("TNML_FORCE_COMM");
  printf("input-gradient refusals: ok\n");
}

// every allocation of the calls' groups (prediction group, input-gradient group, index list) fails in turn; a larger b grows them.
// tnml_predict at an inner label needs the switch; the input-gradient calls do not
static void run_alloc_failures(int D) {
  const int N = 6, L = 2, M = 6, n = 50;
  tnml_ctx *ctx = nullptr;
  OK(tnml_create(&ctx, N, D, L, M, 64, 0));
  OK(tnml_set_any_position(ctx, 1));
  set_cores(ctx, N, D, L, std::vector<int>(N - 1, M), 3);
  std::vector<float> X((size_t)300 * N * D, 0.5f), cot((size_t)L * 300, 1.f), g((size_t)300 * N * D), cf(300), pix((size_t)n * N, 0.5f);
  std::vector<int> lab(n, 1), idx(300);
  for (int i = 0; i < 300; ++i) idx[i] = (i * 7) % n;
  // (a group that was created stays: the prediction group is grown by tnml_predict first, so that every allocation counted below is
  // one of the input-gradient group's six)
  std::vector<float> f((size_t)L * 300);
  fail_each_alloc("tnml_predict, b 70", [&] { return tnml_predict(ctx, X.data(), 70, f.data()); });
  int k = fail_each_alloc("tnml_input_grad, b 70", [&] { return tnml_input_grad(ctx, X.data(), 70, cot.data(), g.data(), cf.data()); });
  if (k != 6) { fprintf(stderr, "%d allocations failed in turn, the input-gradient group has 6\n", k); exit(1); }
  fail_each_alloc("tnml_predict, b 70 -> 300", [&] { return tnml_predict(ctx, X.data(), 300, f.data()); });
  k = fail_each_alloc("tnml_input_grad, b 70 -> 300", [&] { return tnml_input_grad(ctx, X.data(), 300, nullptr, g.data(), cf.data()); });
  if (k != 6) { fprintf(stderr, "%d allocations failed in turn, the input-gradient group has 6\n", k); exit(1); }
  OK(tnml_dataset_attach(ctx, pix.data(), lab.data(), n, N, D, TNML_DATASET_PIXELS));
  fail_each_alloc("tnml_input_grad_indices, first index list", [&] { return tnml_input_grad_indices(ctx, idx.data(), 300, nullptr, TNML_WRT_PIXELS, g.data(), cf.data()); });
  OK(tnml_set_input_grad_chunk(ctx, 640));
  fail_each_alloc("tnml_input_grad_indices, b 300", [&] { return tnml_input_grad_indices(ctx, idx.data(), 300, cot.data(), TNML_WRT_FEATURES, g.data(), cf.data()); });
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
  const char *paths[] = {"input_grad_kernel", "input_grad_onehot_kernel", "input_grad_pixels_kernel"};
  for (const char *k : paths)
    if (san_stub_launches(k) < 1) { fprintf(stderr, "launch path %s was never taken\n", k); return 1; }
  printf("input gradients: %ld input_grad_kernel launches checked, %d refusals\n", san_stub_launches("input_grad_kernel"), g_refusals);
  printf("input-gradient host planning under ASan + UBSan: ok\n");
  return 0;
}
