// The marks of the shape-compiled persistent sweep (tnml_set_shape_kernels / tnml_fixed_shape_steps of tnml_api.hip, the table
// kPersistShapes of wide_pipe_device.h) planned by the real host code, built --cuda-host-only with AddressSanitizer and UBSan,
// against the stand-in runtime of hip_stub.cpp.  `make san-shape` builds and runs it; tests/test_shape_kernels_host.py runs
// `make san-shape`.
//   plan_shape on | off        whole sweeps (right, left, right) at bond 5, 10 and 20 through the C ABI with the switch on / off.  After
//                              every sweep the records the "device" received are read back: a record is marked exactly where the
//                              main itself finds the uniform shape of a table entry, the count is what tnml_fixed_shape_steps says,
//                              and nothing is marked with the switch off, at a bond outside the table, or in mode 2.
//   plan_shape compare A B     two call traces (TNML_SAN_TRACE) of the runs above: apart from the shape field of the records and the
//                              instantiation named in the launch they must be the same text, i.e. marking changes nothing else of
//                              the plan.
// Every run also checks that no constant of a table entry can disagree with a record that is marked with it (persist_step_shape).
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
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

// the table entry whose uniform shape the two role records of a step show, found without persist_step_shape: 1 + index, or 0
static int uniform_entry(const PersistStep &ps) {
  const NarrowParams &n = ps.n;
  const PersistHelperParams &t = ps.t;
  for (int i = 0; i < kNumPersistShapes; ++i) {
    const int H = kPersistShapes[i].H, L = kPersistShapes[i].L;
    const bool update = n.D == kD && n.h == H && n.g == H && n.s == H && n.m == H && n.L == L && n.z_rows == kD * H && n.bsize == H * kD * kD * H * L;
    const bool helper = t.h == H && t.g == H && t.s == H && t.L == L && t.zr == kD * H;
    if (update && helper) return i + 1;
  }
  return 0;
}

static long g_marked = 0, g_records = 0;

// three whole sweeps of an N-site chain at bond M; -> steps marked over the three
static int plan_chain(int N, int M, int L, int b, bool on, int mode) {
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
  OK(tnml_set_shape_kernels(ctx, on ? 1 : 0));
  int marked_all = 0;
  for (int sw = 0; sw < 3; ++sw) {
    OK(tnml_forward(ctx, f.data()));
    const int left = tnml_l_pos(ctx) == N - 1;
    const long before = san_stub_launches(mode == 1 ? "sweep_persist_kernel" : "persist_update_kernel");
    OK(tnml_sweep(ctx, left, N - 1, 1, 1e-3f, 1e-3f, 1, TNML_ACT_SOFTMAX, TNML_LOSS_FULL_CROSS_ENT, 0.1f, TNML_TRUNC_FIXED, met.data(), f.data()));
    CHECK(san_stub_launches(mode == 1 ? "sweep_persist_kernel" : "persist_update_kernel") == before + 1, "N %d bond %d sweep %d took another path", N, M, sw);
    int n_steps = 0;
    const PersistStep *st = (const PersistStep *)san_stub_last_persist(&n_steps);
    CHECK(st && n_steps == N - 1, "records of %d steps", n_steps);
    int marked = 0, launch_shape = 0;
    for (int k = 0; k < n_steps; ++k) {
      const int want = (on && mode == 1) ? uniform_entry(st[k]) : 0;
      CHECK(st[k].shape == want, "N %d bond %d sweep %d step %d: shape %d, the record shows %d (h %d g %d s %d m %d L %d z_rows %d)", N, M, sw, k,
            st[k].shape, want, st[k].n.h, st[k].n.g, st[k].n.s, st[k].n.m, st[k].n.L, st[k].n.z_rows);
      if (st[k].shape) { ++marked; CHECK(!launch_shape || launch_shape == st[k].shape, "two shapes in one launch"); launch_shape = st[k].shape; }
    }
    CHECK(st[n_steps].shape == 0, "the prologue record is marked");
    int said = -1;
    OK(tnml_fixed_shape_steps(ctx, &said));
    CHECK(said == marked, "tnml_fixed_shape_steps says %d, %d records are marked", said, marked);
    marked_all += marked;
    g_records += n_steps;
  }
  OK(tnml_destroy(ctx));
  g_marked += marked_all;
  printf("planned shapes N %d bond %d L %d switch %s mode %d: %d of %d steps marked\n", N, M, L, on ? "on" : "off", mode, marked_all, 3 * (N - 1));
  fflush(stdout);
  return marked_all;
}

// a constant of a table entry that disagrees with the step cannot be marked with that entry
static void constants_cannot_disagree() {
  int tried = 0;
  for (int i = 0; i < kNumPersistShapes; ++i) {
    const int H = kPersistShapes[i].H, L = kPersistShapes[i].L;
    int v[8] = {H, H, H, H, L, kD * H, H * kD * kD * H * L, kPersistHelpers};      // h, g, s, m, L, z_rows, bsize, helpers
    CHECK(persist_step_shape(v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7]) == i + 1, "entry %d does not fit its own shape", i);
    for (int j = 0; j < 8; ++j)
      for (int d = -1; d <= 1; d += 2) {
        int w[8];
        memcpy(w, v, sizeof w);
        w[j] += d;
        CHECK(persist_step_shape(w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7]) != i + 1, "entry %d marks a step whose value %d is off by %d", i, j, d);
        ++tried;
      }
  }
  CHECK(persist_step_shape(1, 20, 20, 2, 2, 1, 160, kPersistHelpers) == 0 && persist_step_shape(5, 5, 5, 5, 3, 10, 300, kPersistHelpers) == 0, "a ramp step is marked");
  printf("shape constants: %d disagreeing values refused\n", tried);
}

// the text of a trace without what marking may change
static std::vector<std::string> normalised(const char *path) {
  std::ifstream in(path);
  CHECK(in.good(), "cannot read %s", path);
  std::vector<std::string> out;
  for (std::string line; std::getline(in, line);) {
    for (size_t at; (at = line.find(" shape=")) != std::string::npos;) {
      size_t end = at + 7;
      while (end < line.size() && line[end] >= '0' && line[end] <= '9') ++end;
      line.erase(at, end - at);
    }
    const size_t k = line.find("sweep_persist_kernel<");
    if (k != std::string::npos) {                       // the instantiation: up to the launch geometry
      const size_t open = k + 20, geo = line.find(" grid=", open);
      if (geo != std::string::npos) line.erase(open, geo - open);
    }
    out.push_back(line);
  }
  return out;
}

int main(int argc, char **argv) {
  const std::string what = argc > 1 ? argv[1] : "on";
  if (what == "compare") {
    CHECK(argc == 4, "compare needs two traces");
    const auto a = normalised(argv[2]), b = normalised(argv[3]);
    CHECK(a.size() == b.size() && a.size() > 100, "%zu and %zu lines", a.size(), b.size());
    for (size_t i = 0; i < a.size(); ++i) CHECK(a[i] == b[i], "line %zu differs beyond the shape field:\n%.400s\n%.400s", i + 1, a[i].c_str(), b[i].c_str());
    printf("shape traces: %zu lines equal apart from the shape field\n", a.size());
    return 0;
  }
  const bool on = what == "on";
  constants_cannot_disagree();
  const int bonds[3] = {5, 10, 20};
  for (int M : bonds) {
    const int marked = plan_chain(24, M, 2, 64, on, 1);
    CHECK((marked > 0) == (on && M != 5), "bond %d: %d steps marked", M, marked);
  }
  CHECK(plan_chain(24, 10, 3, 64, on, 1) == 0, "three labels are not in the table");
  CHECK(plan_chain(24, 20, 2, 64, on, 2) == 0, "mode 2 has the generic kernels only");
  plan_chain(784, 20, 2, 5000, on, 1);                   // the headline chain at true size
  printf("shape plans, switch %s: %ld of %ld records marked\n", on ? "on" : "off", g_marked, g_records);
  san_stub_report();
  printf("shape-kernel host planning under ASan + UBSan: ok\n");
  return 0;
}
