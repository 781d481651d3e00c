// The device-resident dataset (tnml_dataset_attach / tnml_select_indices / tnml_predict_indices / tnml_eval_indices /
// tnml_resident_metrics / tnml_dataset_read of api_dataset.hip and the launch wrappers of kernels_dataset.hip) planned by the real host
// code, built --cuda-host-only with AddressSanitizer and UBSan, against the stand-in runtime of hip_stub.cpp.  The binary is linked
// with -Wl,--wrap=hipLaunchKernel: every launch of kernels_dataset.hip passes through check_* below first, which checks the grid and
// every pointer of the argument block together with the extent the kernel touches -- for the gather THROUGH the index list the host
// uploaded (the stand-in's device memory is host memory, so the list can be read back): every row it names must lie inside the
// dataset allocation.  `make san-dataset` builds and runs it; tests/test_dataset_host.py runs `make san-dataset`.
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../tnml_internal.h"
#include "fail_each.h"

using namespace tnml;

namespace tnml {
template <bool PIXELS>
__global__ void dataset_gather_d2_kernel(DatasetGather);
template <bool PIXELS>
__global__ void dataset_gather_anyd_kernel(DatasetGather);
__global__ void dataset_metrics_kernel(const float *, const int *, int, int, int, int, float, double *);
__global__ void dataset_metrics_sum_kernel(const double *, int, int, double *);
}  // namespace tnml

extern "C" void san_stub_report(void);
extern "C" long san_stub_launches(const char *substr);
extern "C" hipError_t __real_hipLaunchKernel(const void *fn, dim3 g, dim3 b, void **args, size_t shm, hipStream_t st);

static long g_checks = 0, g_gathers = 0, g_rows = 0;
static const char *g_what = "";
static int g_n = 0, g_L = 0;        // samples of the dataset attached right now, labels of the context

[[noreturn]] static void die(const char *fmt, ...) __attribute__((format(printf, 1, 2)));
static void die(const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  fprintf(stderr, "plan_dataset VIOLATION [%s]: ", g_what);
  vfprintf(stderr, fmt, ap);
  fprintf(stderr, "\n");
  va_end(ap);
  abort();
}
// [p, p + bytes) inside one live allocation: the stand-in's copy check aborts otherwise
static void need(const void *p, size_t bytes, const char *what, void *keep = nullptr) {
  ++g_checks;
  if (!p) die("%s: null pointer (%zu bytes wanted)", what, bytes);
  if (!bytes) return;
  std::vector<char> tmp(keep ? 0 : bytes);
  g_what = what;
  if (hipMemcpy(keep ? keep : (void *)tmp.data(), p, bytes, hipMemcpyDeviceToHost) != hipSuccess) die("%s: copy refused", what);
}

static void check_gather(const DatasetGather &p, dim3 g, dim3 blk, bool d2) {
  ++g_gathers;
  if (p.b < 1 || p.b > p.b_pad || p.b_pad % 64) die("gather: b %d b_pad %d", p.b, p.b_pad);
  if (p.D < 2 || p.D > kMaxD || d2 != (p.D == kD)) die("gather: D %d in the %s kernel", p.D, d2 ? "D = 2" : "general-D");
  if ((int)g.x * 32 != p.b_pad || (int)g.y * 32 < p.N || g.z != 1 || blk.x != 256) die("gather: grid (%u, %u) block %u for b_pad %d, N %d", g.x, g.y, blk.x, p.b_pad, p.N);
  if (g_n < 1) die("gather launched without a dataset");
  const size_t per = (size_t)p.N * (p.pixels ? 1 : p.D);
  need(p.data, (size_t)g_n * per * 4, "gather dataset");
  std::vector<int> idx(p.b);
  need(p.idx, (size_t)p.b * 4, "gather index list", idx.data());
  for (int i = 0; i < p.b; ++i) {
    if (idx[i] < 0 || idx[i] >= g_n) die("gather: index %d at position %d outside [0, %d) reached a launch", idx[i], i, g_n);
    ++g_rows;
  }
  need(p.out, (size_t)p.N * p.b_pad * p.D * 4, "gather output");
  if (p.y_out) {
    need(p.labels, (size_t)g_n * 4, "gather labels");
    need(p.y_out, (size_t)p.b_pad * 4, "gather label output");
  }
  if (p.pixels)
    for (int s = 0; s < p.D; ++s)
      if (!(p.coef[s] >= 1.0)) die("gather: feature-map factor %d is %g", s, p.coef[s]);
}

static void check_metrics(const float *f, const int *y, int L, int b, int b_pad, int act_fn, double *part, dim3 g, dim3 blk, size_t shm) {
  if (b < 1 || b > b_pad || b_pad % 64 || L != g_L || act_fn < 0 || act_fn > 2) die("metrics: b %d b_pad %d L %d act %d", b, b_pad, L, act_fn);
  if ((int)g.x != (b + kDsMetricThreads - 1) / kDsMetricThreads || blk.x != (unsigned)kDsMetricThreads) die("metrics: grid %u block %u for b %d", g.x, blk.x, b);
  if (shm != (size_t)2 * L * kDsMetricThreads * 4 || shm > 64 * 1024) die("metrics: %zu bytes of LDS for L %d", shm, L);
  need(f, (size_t)L * b_pad * 4, "metrics f");
  need(y, (size_t)b_pad * 4, "metrics labels");
  need(part, (size_t)g.x * 4 * 8, "metrics block partials");
}

extern "C" hipError_t __wrap_hipLaunchKernel(const void *fn, dim3 g, dim3 b, void **args, size_t shm, hipStream_t st) {
  if (fn == (const void *)&dataset_gather_d2_kernel<true> || fn == (const void *)&dataset_gather_d2_kernel<false>) {
    g_what = "dataset_gather_d2_kernel";
    const DatasetGather &p = *(const DatasetGather *)args[0];
    if (p.pixels != (fn == (const void *)&dataset_gather_d2_kernel<true>)) die("gather: form %d in the wrong instantiation", p.pixels);
    check_gather(p, g, b, true);
  } else if (fn == (const void *)&dataset_gather_anyd_kernel<true> || fn == (const void *)&dataset_gather_anyd_kernel<false>) {
    g_what = "dataset_gather_anyd_kernel";
    const DatasetGather &p = *(const DatasetGather *)args[0];
    if (p.pixels != (fn == (const void *)&dataset_gather_anyd_kernel<true>)) die("gather: form %d in the wrong instantiation", p.pixels);
    check_gather(p, g, b, false);
  } else if (fn == (const void *)&dataset_metrics_kernel) {
    g_what = "dataset_metrics_kernel";
    check_metrics(*(const float **)args[0], *(const int **)args[1], *(int *)args[2], *(int *)args[3], *(int *)args[4], *(int *)args[5],
                  *(double **)args[7], g, b, shm);
  } else if (fn == (const void *)&dataset_metrics_sum_kernel) {
    g_what = "dataset_metrics_sum_kernel";
    const int nblk = *(int *)args[1];
    if (nblk < 1 || g.x != 1 || b.x < 4) die("metrics sum: %d partials, grid %u block %u", nblk, g.x, b.x);
    need(*(const double **)args[0], (size_t)nblk * 4 * 8, "metrics sum partials");
    need(*(double **)args[3], 4 * 8, "metrics sum accumulators");
  }
  g_what = "";
  return __real_hipLaunchKernel(fn, g, b, args, shm, st);
}

#define OK(call)                                                                              \
  do {                                                                                        \
    int rc_ = (call);                                                                         \
    if (rc_ != TNML_OK) { fprintf(stderr, "%s:%d %s -> %d: %s\n", __FILE__, __LINE__, #call, rc_, tnml_last_error()); exit(1); } \
  } while (0)
#define FAILS_WITH(code, call)                                                                \
  do {                                                                                        \
    const long before_ = g_gathers;                                                           \
    int rc_ = (call);                                                                         \
    if (rc_ != (code)) { fprintf(stderr, "%s:%d %s -> %d, expected %d\n", __FILE__, __LINE__, #call, rc_, (code)); exit(1); } \
    if (g_gathers != before_) { fprintf(stderr, "%s:%d %s launched a gather before it failed\n", __FILE__, __LINE__, #call); exit(1); } \
  } while (0)

static void attach(tnml_ctx *ctx, int n, int N, int D, int L, int form) {
  std::vector<float> data((size_t)n * N * (form == TNML_DATASET_PIXELS ? 1 : D));
  for (size_t e = 0; e < data.size(); ++e) data[e] = (float)(e % 101) / 100.f;
  std::vector<int> lab(n);
  for (int i = 0; i < n; ++i) lab[i] = i % L;
  OK(tnml_dataset_attach(ctx, data.data(), lab.data(), n, N, D, form));
  g_n = n;
  if (tnml_dataset_size(ctx) != n) { fprintf(stderr, "dataset size %d, attached %d\n", tnml_dataset_size(ctx), n); exit(1); }
}

static std::vector<int> indices(int b, int n, int salt) {
  std::vector<int> v(b);
  for (int i = 0; i < b; ++i) v[i] = (int)(((long long)i * 7919 + salt) % n);      // repeats included once b > n
  return v;
}

static void run(int N, int D, int L, int M, int b_cap) {
  tnml_ctx *ctx = nullptr;
  OK(tnml_create(&ctx, N, D, L, M, b_cap, 0));
  g_L = L; g_n = 0;
  std::vector<int> bond(N - 1, M);
  size_t total = 0;
  for (int i = 0; i < N; ++i) total += (size_t)(i == 0 ? 1 : M) * D * (i == N - 1 ? 1 : M) * (i == 0 ? L : 1);
  std::vector<float> cores(total, 0.1f);
  OK(tnml_set_cores(ctx, cores.data(), total, bond.data(), 0));
  std::vector<int> one = {0};
  double out3[3];
  std::vector<float> f((size_t)L * 4 * b_cap + 64 * L), X((size_t)(4 * b_cap + 64) * N * D);
  // nothing attached yet
  FAILS_WITH(TNML_ERR_STATE, tnml_select_indices(ctx, one.data(), 1));
  FAILS_WITH(TNML_ERR_STATE, tnml_predict_indices(ctx, one.data(), 1, f.data()));
  FAILS_WITH(TNML_ERR_STATE, tnml_eval_indices(ctx, one.data(), 1, TNML_ACT_SOFTMAX, 0.1f, out3));
  FAILS_WITH(TNML_ERR_STATE, tnml_dataset_read(ctx, one.data(), 1, X.data()));
  FAILS_WITH(TNML_ERR_STATE, tnml_resident_metrics(ctx, TNML_ACT_SOFTMAX, 0.1f, out3));
  {
    std::vector<float> d((size_t)4 * N * D, 0.5f);
    std::vector<int> l = {0, 1 % L, L, 0};
    FAILS_WITH(TNML_ERR_ARG, tnml_dataset_attach(ctx, d.data(), l.data(), 4, N, D, TNML_DATASET_FEATURES));      // label == L
    l[2] = -1;
    FAILS_WITH(TNML_ERR_ARG, tnml_dataset_attach(ctx, d.data(), l.data(), 4, N, D, TNML_DATASET_PIXELS));
    l[2] = 0;
    FAILS_WITH(TNML_ERR_ARG, tnml_dataset_attach(ctx, d.data(), l.data(), 4, N + 1, D, TNML_DATASET_FEATURES));
    FAILS_WITH(TNML_ERR_ARG, tnml_dataset_attach(ctx, d.data(), l.data(), 4, N, D == 2 ? 3 : 2, TNML_DATASET_FEATURES));
    FAILS_WITH(TNML_ERR_ARG, tnml_dataset_attach(ctx, d.data(), l.data(), 0, N, D, TNML_DATASET_FEATURES));
    FAILS_WITH(TNML_ERR_ARG, tnml_dataset_attach(ctx, d.data(), l.data(), 4, N, D, 2));
  }
  const int ns[2] = {3 * b_cap + 29, b_cap / 2 + 3};            // re-attach with another n
  for (int form : {TNML_DATASET_FEATURES, TNML_DATASET_PIXELS})
    for (int n : ns) {
      attach(ctx, n, N, D, L, form);
      // ragged, one sample, a full batch, larger than the capacity the context was created with (the buffers grow)
      for (int b : {b_cap - 3, 1, b_cap, b_cap + 70, 2 * b_cap + 5}) {
        std::vector<int> idx = indices(b, n, b);
        OK(tnml_select_indices(ctx, idx.data(), b));
        if (tnml_batch(ctx) != b) { fprintf(stderr, "resident batch %d after selecting %d\n", tnml_batch(ctx), b); exit(1); }
        OK(tnml_forward(ctx, f.data()));
        OK(tnml_resident_metrics(ctx, TNML_ACT_SOFTMAX, 0.1f, out3));
        std::vector<float> met((size_t)2 * (N - 1));
        OK(tnml_sweep(ctx, 0, N - 1, 1, 1e-3f, 1e-3f, 1, TNML_ACT_SOFTMAX, TNML_LOSS_FULL_CROSS_ENT, 0.1f, TNML_TRUNC_FIXED, met.data(), nullptr));
        OK(tnml_resident_metrics(ctx, TNML_ACT_LINEAR, 1.f, out3));
        // evaluation and prediction at the far end of the chain, then the sweep back
        OK(tnml_predict_indices(ctx, idx.data(), b, f.data()));
        OK(tnml_eval_indices(ctx, idx.data(), b, TNML_ACT_SIGMOID, 0.5f, out3));
        OK(tnml_select_indices(ctx, idx.data(), b));
        OK(tnml_forward(ctx, nullptr));
        OK(tnml_sweep(ctx, 1, N - 1, 1, 1e-3f, 1e-3f, 1, TNML_ACT_SOFTMAX, TNML_LOSS_FULL_CROSS_ENT, 0.1f, TNML_TRUNC_FIXED, nullptr, nullptr));
        OK(tnml_dataset_read(ctx, idx.data(), b, X.data()));
      }
      // more samples than any buffer holds, repeats included
      const int big = 3 * tnml_batch(ctx) + 4 * b_cap + 17;
      std::vector<int> all = indices(big, n, 1);
      OK(tnml_eval_indices(ctx, all.data(), big, TNML_ACT_SOFTMAX, 0.1f, out3));
      // refusals: nothing is launched, the resident batch stays
      const int b_before = tnml_batch(ctx);
      std::vector<int> bad = indices(b_cap, n, 2);
      bad[b_cap / 2] = n;
      FAILS_WITH(TNML_ERR_ARG, tnml_select_indices(ctx, bad.data(), b_cap));
      FAILS_WITH(TNML_ERR_ARG, tnml_predict_indices(ctx, bad.data(), b_cap, f.data()));
      FAILS_WITH(TNML_ERR_ARG, tnml_eval_indices(ctx, bad.data(), b_cap, TNML_ACT_SOFTMAX, 0.1f, out3));
      FAILS_WITH(TNML_ERR_ARG, tnml_dataset_read(ctx, bad.data(), b_cap, X.data()));
      bad[b_cap / 2] = -1;
      FAILS_WITH(TNML_ERR_ARG, tnml_select_indices(ctx, bad.data(), b_cap));
      bad[b_cap / 2] = INT32_MIN;
      FAILS_WITH(TNML_ERR_ARG, tnml_eval_indices(ctx, bad.data(), b_cap, TNML_ACT_SOFTMAX, 0.1f, out3));
      FAILS_WITH(TNML_ERR_ARG, tnml_select_indices(ctx, one.data(), 0));
      FAILS_WITH(TNML_ERR_ARG, tnml_select_indices(ctx, one.data(), -5));
      FAILS_WITH(TNML_ERR_ARG, tnml_eval_indices(ctx, one.data(), 0, TNML_ACT_SOFTMAX, 0.1f, out3));
      FAILS_WITH(TNML_ERR_ARG, tnml_eval_indices(ctx, one.data(), 1, 3, 0.1f, out3));
      FAILS_WITH(TNML_ERR_ARG, tnml_select_indices(ctx, nullptr, 1));
      if (tnml_batch(ctx) != b_before) { fprintf(stderr, "a refused call changed the resident batch\n"); exit(1); }
      OK(tnml_forward(ctx, nullptr));
      // an intermediate label position: prediction and evaluation are refused, selecting is not
      OK(tnml_sweep(ctx, 0, 1, 1, 1e-3f, 1e-3f, 1, TNML_ACT_SOFTMAX, TNML_LOSS_FULL_CROSS_ENT, 0.1f, TNML_TRUNC_FIXED, nullptr, nullptr));
      FAILS_WITH(TNML_ERR_STATE, tnml_predict_indices(ctx, one.data(), 1, f.data()));
      FAILS_WITH(TNML_ERR_STATE, tnml_eval_indices(ctx, one.data(), 1, TNML_ACT_SOFTMAX, 0.1f, out3));
      OK(tnml_set_cores(ctx, cores.data(), total, bond.data(), 0));
      OK(tnml_dataset_detach(ctx));
      g_n = 0;
      FAILS_WITH(TNML_ERR_STATE, tnml_select_indices(ctx, one.data(), 1));
    }
  // destroy frees a dataset that is still attached
  attach(ctx, 5, N, D, L, TNML_DATASET_PIXELS);
  OK(tnml_destroy(ctx));
  printf("planned dataset calls D %d N %d bond %d L %d capacity %d: ok\n", D, N, M, L, b_cap);
  fflush(stdout);
}

// with a communicator the dataset calls are refused (D = 2 only: the generic path has no communicator)
static void run_comm() {
  setenv("TNML_FORCE_COMM", "1", 1);
  tnml_ctx *ctx = nullptr;
  OK(tnml_create(&ctx, 8, 2, 2, 4, 64, 0));
  unsigned char uid[128];
  OK(tnml_comm_unique_id(uid));
  OK(tnml_comm_init(ctx, 0, 1, uid));
  std::vector<float> d((size_t)4 * 8 * 2, 0.5f);
  std::vector<int> l = {0, 1, 0, 1}, one = {0};
  double out3[3];
  FAILS_WITH(TNML_ERR_STATE, tnml_dataset_attach(ctx, d.data(), l.data(), 4, 8, 2, TNML_DATASET_FEATURES));
  FAILS_WITH(TNML_ERR_STATE, tnml_select_indices(ctx, one.data(), 1));
  FAILS_WITH(TNML_ERR_STATE, tnml_eval_indices(ctx, one.data(), 1, TNML_ACT_SOFTMAX, 0.1f, out3));
  FAILS_WITH(TNML_ERR_STATE, tnml_resident_metrics(ctx, TNML_ACT_SOFTMAX, 0.1f, out3));
  OK(tnml_destroy(ctx));
  unsetenv("TNML_FORCE_COMM");
  printf("communicator attached: dataset calls refused\n");
}

// Failed allocations (injected by the stand-in, see fail_each.h) in every group the dataset calls size: the dataset itself, the index
// list, the batch group a larger selection grows, the metrics partials, the prediction group, the temporary of tnml_dataset_read.
// Each call fails once per allocation, then succeeds; a forward and a full sweep over the grown buffers close the sequence.
static void run_alloc_failures(int D) {
  const int N = 6, L = 2, M = 6, b_cap = 64, n = 500;
  tnml_ctx *ctx = nullptr;
  OK(tnml_create(&ctx, N, D, L, M, b_cap, 0));
  g_L = L;
  std::vector<int> bond(N - 1, M);
  size_t total = 0;
  for (int i = 0; i < N; ++i) total += (size_t)(i == 0 ? 1 : M) * D * (i == N - 1 ? 1 : M) * (i == 0 ? L : 1);
  std::vector<float> cores(total, 0.1f), data((size_t)n * N * D, 0.5f), f((size_t)L * 2500), X((size_t)300 * N * D), met((size_t)2 * (N - 1));
  OK(tnml_set_cores(ctx, cores.data(), total, bond.data(), 0));
  std::vector<int> lab(n, 1), few = indices(40, n, 1), more = indices(300, n, 2), many = indices(2500, n, 3);
  double out3[3];
  g_n = n;
  fail_each_alloc("tnml_dataset_attach", [&] { return tnml_dataset_attach(ctx, data.data(), lab.data(), n, N, D, TNML_DATASET_FEATURES); });
  fail_each_alloc("tnml_select_indices, first index list", [&] { return tnml_select_indices(ctx, few.data(), 40); });
  fail_each_alloc("tnml_select_indices, b 40 -> 300", [&] { return tnml_select_indices(ctx, more.data(), 300); });
  OK(tnml_forward(ctx, f.data()));
  fail_each_alloc("tnml_resident_metrics", [&] { return tnml_resident_metrics(ctx, TNML_ACT_SOFTMAX, 0.1f, out3); });
  fail_each_alloc("tnml_predict_indices, b 300", [&] { return tnml_predict_indices(ctx, more.data(), 300, f.data()); });
  fail_each_alloc("tnml_eval_indices, longer index list", [&] { return tnml_eval_indices(ctx, many.data(), 2500, TNML_ACT_SOFTMAX, 0.1f, out3); });
  fail_each_alloc("tnml_dataset_read", [&] { return tnml_dataset_read(ctx, more.data(), 300, X.data()); });
  OK(tnml_sweep(ctx, 0, N - 1, 1, 1e-3f, 1e-3f, 1, TNML_ACT_SOFTMAX, TNML_LOSS_FULL_CROSS_ENT, 0.1f, TNML_TRUNC_FIXED, met.data(), nullptr));
  OK(tnml_destroy(ctx));
  g_n = 0;
}

int main() {
  run(12, 2, 2, 6, 100);
  run(37, 2, 3, 5, 64);            // more than one site tile, odd bond, three labels
  run(12, 3, 2, 6, 100);
  run(33, 3, 10, 4, 70);           // ten labels: the metrics kernel's LDS tile
  run(9, 8, 2, 4, 64);
  run_comm();
  run_alloc_failures(2);
  run_alloc_failures(3);
  san_stub_report();
  const char *paths[] = {"dataset_gather_d2_kernel<true>", "dataset_gather_d2_kernel<false>", "dataset_gather_anyd_kernel<true>",
                         "dataset_gather_anyd_kernel<false>", "dataset_metrics_kernel", "dataset_metrics_sum_kernel"};
  for (const char *k : paths)
    if (san_stub_launches(k) < 1) { fprintf(stderr, "launch path %s was never taken\n", k); return 1; }
  printf("dataset launches: %ld argument extents checked, %ld gathers through %ld indices\n", g_checks, g_gathers, g_rows);
  printf("dataset host planning under ASan + UBSan: ok\n");
  return 0;
}
