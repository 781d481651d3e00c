// The slice reduction of the persistent sweep (tnml_set_persist_reduce / tnml_slice_reduce_steps of tnml_api.hip, the reducer loop of
// wide_pipe_block in wide_pipe_device.h) planned by the real host code, built --cuda-host-only with AddressSanitizer and UBSan,
// against the stand-in runtime of hip_stub.cpp.  `make san-slices` builds and runs it; tests/test_slice_reduce_host.py runs
// `make san-slices`.
// Whole sweeps (right, left, right) through the C ABI, in both persistent modes, with the switch at 1 and at 0: bond 20 at two labels
// on 16 sites at the batch sizes whose workgroup counts sit on the edges of the reduction groups (33, 512, 513, 1000, 5000), bond 5 at
// three labels (no compiled shape: the generic bodies), and the headline chain at true size.  After every sweep the records the
// "device" received are read back and checked:
//   * switch 1: exactly the records that form a pre-gradient beyond one level reduce in slices; switch 0: none, and every field of
//     the hand-off is the last-arriver form's;
//   * the runs the reducers walk (the kernel's own loop, repeated here) cover the 16-byte elements [0, n4) once each, a run is whole
//     128-byte lines, there are no more reducers than workgroups, and the group sums of a run fit the workgroup's LDS;
//   * the arrival and the done word lie in the step's own counter block and are no word another role of that step uses;
//   * the helpers of step k wait on the done word of the record that forms Z_k (the prologue at k = 0) for its reducer count, or,
//     where that record has a single writer, for the value that writer stores;
//   * tnml_slice_reduce_steps says the number of such records.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../tnml_internal.h"
#include "../wide_pipe_device.h"

using namespace tnml;

extern "C" void san_stub_report(void);
extern "C" long san_stub_launches(const char *substr);
extern "C" const void *san_stub_last_persist(int *n_steps);

#define OK(call)                                                                              \
  do {                                                                                        \
    int rc_ = (call);                                                                         \
    if (rc_ != TNML_OK) { fprintf(stderr, "%s:%d %s -> %d: %s\n", __FILE__, __LINE__, #call, rc_, tnml_last_error()); exit(1); } \
  } while (0)
#define CHECK(cond, ...)                                                                      \
  do {                                                                                        \
    if (!(cond)) { fprintf(stderr, "%s:%d %s: ", __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } \
  } while (0)

static long g_sliced = 0, g_records = 0;

// one batch-side record of a sweep; blk: the counter block sweep_persist gave it; -> 1 if it reduces in slices
static int check_batch_record(const WidePipeParams &w, const unsigned *blk, int mode_reduce, const char *what, int k) {
  CHECK(w.persist == 1, "%s %d: not a persistent record", what, k);
  CHECK(w.gcnt == blk && w.tcnt == blk + 16, "%s %d: tickets outside the step's block", what, k);
  const bool beyond_one_level = w.do_z && !w.one_level;
  CHECK(w.slice_red == (mode_reduce == 1 && beyond_one_level ? 1 : 0), "%s %d: slice_red %d with switch %d, do_z %d, one_level %d", what, k,
        w.slice_red, mode_reduce, w.do_z, w.one_level);
  if (!w.slice_red) {
    CHECK(w.slice_S == 0 && w.slice_R == 0 && !w.sarrive && !w.sdone, "%s %d: slice fields set on a record of another form", what, k);
    return 0;
  }
  const int n4 = (w.zsize + kMetricSlots + 3) / 4, S = w.slice_S, R = w.slice_R;
  CHECK(S >= 8 && S % 8 == 0, "%s %d: run of %d elements", what, k, S);
  CHECK(R >= 1 && R <= w.nwide, "%s %d: %d reducers, %d workgroups", what, k, R, w.nwide);
  CHECK(R == std::min((n4 + S - 1) / S, w.nwide), "%s %d: %d reducers for %d elements in runs of %d", what, k, R, n4, S);
  CHECK(w.ngroups == (w.nwide + kPipeGroupMax - 1) / kPipeGroupMax && w.gsz == kPipeGroupMax, "%s %d: groups %d x %d", what, k, w.ngroups, w.gsz);
  CHECK((size_t)w.ngroups * S * 16 <= wide_pipe_lds_bytes(w) - 16, "%s %d: group sums beyond LDS", what, k);
  // the kernel's loop: reducer wg takes the runs wg, wg + R, ...
  std::vector<int> seen(n4, 0);
  for (int wg = 0; wg < R; ++wg)
    for (int run = wg; run * S < n4; run += R)
      for (int el = 0; el < std::min(S, n4 - run * S); ++el) ++seen[run * S + el];
  for (int e = 0; e < n4; ++e) CHECK(seen[e] == 1, "%s %d: element %d of %d summed %d times", what, k, e, n4, seen[e]);
  CHECK((size_t)n4 * 4 <= (size_t)w.slab_stride, "%s %d: %d elements beyond the slab stride", what, k, n4);
  // the two words: inside the block, apart from each other, from the tickets of either form and from the helpers' two counters
  const long a = w.sarrive - blk, d = w.sdone - blk;
  CHECK(a >= 0 && a < 32 && d >= 0 && d < 32 && a != d, "%s %d: words %ld, %ld of the block", what, k, a, d);
  for (long word : {a, d}) CHECK(word > 16 && word != 20 && word != 21, "%s %d: word %ld of the block is in use", what, k, word);
  return 1;
}

// three whole sweeps; -> records that reduced in slices over the three
static int plan_chain(int N, int M, int L, int b, int mode_reduce, int mode) {
  const int D = kD;
  tnml_ctx *ctx = nullptr;
  OK(tnml_create(&ctx, N, D, L, M, b, 0));
  std::vector<int> bond(N - 1, M);
  size_t total = 0;
  for (int i = 0; i < N; ++i) total += (size_t)(i == 0 ? 1 : M) * D * (i == N - 1 ? 1 : M) * (i == 0 ? L : 1);
  std::vector<float> cores(total);
  for (size_t e = 0; e < total; ++e) cores[e] = 0.1f + 1e-3f * (float)(e % 97);
  OK(tnml_set_cores(ctx, cores.data(), total, bond.data(), 0));
  std::vector<float> X((size_t)b * N * D, 0.5f), f((size_t)L * b), met((size_t)2 * (N - 1));
  std::vector<int> y(b);
  for (int s = 0; s < b; ++s) y[s] = s % L;
  OK(tnml_set_input(ctx, X.data(), y.data(), b));
  OK(tnml_set_persistent(ctx, mode));
  OK(tnml_set_persist_reduce(ctx, mode_reduce));
  CHECK(tnml_set_persist_reduce(ctx, 2) == TNML_ERR_ARG && tnml_set_persist_reduce(ctx, -1) == TNML_ERR_ARG, "a mode outside 0 | 1 is taken");
  int per_sweep[3] = {0, 0, 0}, uniform_sliced = 0, uniform = 0, nwide = 0;
  const char *kernel = mode == 1 ? "sweep_persist_kernel" : "persist_update_kernel";
  for (int sw = 0; sw < 3; ++sw) {
    OK(tnml_forward(ctx, f.data()));
    const int left = tnml_l_pos(ctx) == N - 1;
    const long before = san_stub_launches(kernel);
    OK(tnml_sweep(ctx, left, N - 1, 1, 1e-3f, 1e-3f, sw != 1, TNML_ACT_SOFTMAX, TNML_LOSS_FULL_CROSS_ENT, 0.1f, TNML_TRUNC_FIXED, met.data(), f.data()));
    CHECK(san_stub_launches(kernel) == before + 1, "N %d bond %d b %d sweep %d took another path", N, M, b, sw);
    int n = 0;
    const PersistStep *st = (const PersistStep *)san_stub_last_persist(&n);
    CHECK(st && n == N - 1, "records of %d steps", n);
    // the counter blocks: record k has block k, the prologue (record n) block n
    const unsigned *base = st[0].w.gcnt;
    int sliced = check_batch_record(st[n].w, base + (size_t)n * 32, mode_reduce, "prologue", n);
    for (int k = 0; k < n; ++k) {
      const unsigned *blk = base + (size_t)k * 32;
      sliced += check_batch_record(st[k].w, blk, mode_reduce, "step", k);
      const PersistHelperParams &t = st[k].t;
      const NarrowParams &u = st[k].n;
      CHECK(t.tcnt == blk + 20 && t.pcnt == blk + 21 && u.pready == blk + 21, "step %d: helper counters moved", k);
      const WidePipeParams &src = k == 0 ? st[n].w : st[k - 1].w;           // the record whose iteration forms Z_k
      CHECK(src.do_z, "step %d: nothing forms its pre-gradient", k);
      if (src.slice_red) CHECK(t.zready == src.sdone && t.zwant == (unsigned)src.slice_R, "step %d: helpers wait for %u, %d reducers count", k, t.zwant, src.slice_R);
      else CHECK(t.zready == src.zready && t.zwant == src.zpublish, "step %d: helpers wait for %u, the single writer stores %u", k, t.zwant, src.zpublish);
      CHECK(t.Z == src.zred && u.zred == src.zred, "step %d: Z read where it was not written", k);
      if (mode_reduce == 0) CHECK(t.zready == st[0].t.zready && t.zwant == (unsigned)k + 1, "step %d: switch 0 is not the last-arriver hand-off", k);
      const WidePipeParams &w = st[k].w;
      if (w.do_z && w.hj == M && w.gn == M && w.gj == M) { ++uniform; uniform_sliced += w.slice_red; }
      nwide = w.nwide;
    }
    int said = -1;
    OK(tnml_slice_reduce_steps(ctx, &said));
    CHECK(said == sliced, "tnml_slice_reduce_steps says %d, %d records reduce in slices", said, sliced);
    per_sweep[sw] = sliced;
    g_records += n + 1;
  }
  OK(tnml_destroy(ctx));
  const int all = per_sweep[0] + per_sweep[1] + per_sweep[2];
  g_sliced += all;
  if (mode_reduce == 1 && M == 20) CHECK(uniform > 0 && uniform_sliced == uniform, "%d of %d uniform steps reduce in slices", uniform_sliced, uniform);
  printf("planned slices N %d bond %d L %d b %d workgroups %d switch %d mode %d: %d %d %d records in slices, %d of %d uniform steps\n", N, M, L, b, nwide,
         mode_reduce, mode, per_sweep[0], per_sweep[1], per_sweep[2], uniform_sliced, uniform);
  fflush(stdout);
  return all;
}

int main() {
  const int batches[5] = {33, 512, 513, 1000, 5000};
  for (int mode_reduce = 1; mode_reduce >= 0; --mode_reduce)
    for (int mode = 1; mode <= 2; ++mode) {
      for (int b : batches) {
        const int got = plan_chain(16, 20, 2, b, mode_reduce, mode);
        CHECK((got > 0) == (mode_reduce == 1), "bond 20, batch %d, switch %d: %d records in slices", b, mode_reduce, got);
      }
      // (bond 5 at three labels: the 1200-float pre-gradients of its uniform steps are beyond one level too, on the generic bodies)
      const int got5 = plan_chain(10, 5, 3, 513, mode_reduce, mode);
      CHECK((got5 > 0) == (mode_reduce == 1), "bond 5, switch %d: %d records in slices", mode_reduce, got5);
    }
  CHECK(plan_chain(784, 20, 2, 5000, 1, 1) > 3 * 760, "the headline chain reduces in slices in its uniform middle");
  CHECK(plan_chain(784, 20, 2, 5000, 0, 1) == 0, "switch 0");
  printf("slice plans: %ld of %ld records reduce in slices\n", g_sliced, g_records);
  san_stub_report();
  printf("slice-reduction host planning under ASan + UBSan: ok\n");
  return 0;
}
