// Likelihood training (tnml_nll_step, tnml_nll_train_indices, tnml_set_nll_overlap of tnml_api.hip and the launch wrappers of
// kernels_nll.hip / kernels_optim.hip) planned by the real host code, built --cuda-host-only with AddressSanitizer and UBSan, against
// the stand-in runtime of hip_stub.cpp, which checks every extent of every launch of a step: the chunks' chains, the cotangent at the
// chunk's offset, the norm term's stacks, the record's slot, the skip word and every core's part of G and of the optimiser state.
// Nothing computes there: the records come back as the memory holds them (zeros: every step "applied").  Run as
// `plan_nll_step trace` with TNML_SAN_TRACE set, it plans the ragged chain alone, reads its own call trace and checks the event fork
// and join of every overlapped step.  `make san-nll-step`
// builds and runs it; tests/test_nll_step_host.py runs `make san-nll-step`.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "../tnml_internal.h"
#include "fail_each.h"

extern "C" void san_stub_report(void);
extern "C" long san_stub_launches(const char *substr);

static int g_refusals = 0;
static long g_overlapped_steps = 0;

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

static void set_cores(tnml_ctx *ctx, const Chain &w, int l_pos) { OK(tnml_set_cores(ctx, w.flat.data(), w.flat.size(), w.bond.data(), l_pos)); }

struct Counts {
  long env, grad, sum, rec, opt, cot, red;
  static Counts now() {
    return {san_stub_launches("lognorm_env_kernel"), san_stub_launches("lognorm_grad_kernel"), san_stub_launches("nll_sum_kernel"), san_stub_launches("nll_record_kernel"),
            san_stub_launches("optim_step_kernel"), san_stub_launches("nll_cot_kernel"), san_stub_launches("core_grad_reduce_kernel")};
  }
};

// both objectives, X and index forms, the default chunk and chunks of 64, overlap on and off, renorm on and off, the three optimisers;
// a multi-step call with a ragged last batch
static void step_calls(tnml_ctx *ctx, int N, int D, int L, int b) {
  std::vector<float> X((size_t)b * N * D, 0.5f);
  std::vector<int32_t> y(b), idx(b);
  for (int s = 0; s < b; ++s) { y[s] = s % L; idx[s] = (s * 7) % b; }
  std::vector<double> S((size_t)D * D, 0.5);
  const int batch = (b + 2) / 3 + 1, n_steps = (b + batch - 1) / batch;
  std::vector<double> v4(4), vals((size_t)n_steps * 4);
  OK(tnml_dataset_attach(ctx, X.data(), y.data(), b, N, D, TNML_DATASET_FEATURES));
  const int optim[3][2] = {{TNML_OPT_SGD, 0}, {TNML_OPT_SGD, 1}, {TNML_OPT_ADAM, 0}};
  for (int o = 0; o < 3; ++o) {
    OK(tnml_optim_config(ctx, optim[o][0], o == 1 ? 0.9 : 0.0, 0.9, 0.999, 1e-8, optim[o][1]));
    for (int chunk : {0, 64})
      for (int overlap : {0, 1})
        for (int renorm : {0, 1}) {
          OK(tnml_set_core_grad_chunk(ctx, chunk));
          OK(tnml_set_nll_overlap(ctx, overlap));
          const Counts a = Counts::now();
          OK(tnml_nll_step(ctx, X.data(), y.data(), b, S.data(), 1e-3f, 0.f, renorm, v4.data()));
          OK(tnml_nll_step(ctx, X.data(), nullptr, b, nullptr, 1e-3f, 1e-2f, renorm, v4.data()));
          OK(tnml_nll_train_indices(ctx, idx.data(), b, batch, 1, S.data(), 1e-3f, 0.f, renorm, vals.data()));
          OK(tnml_nll_train_indices(ctx, idx.data(), b, batch, 0, nullptr, 1e-3f, 0.f, renorm, vals.data()));
          const Counts z = Counts::now();
          const long steps = 2 + 2 * n_steps;
          CHECK(z.env - a.env == steps && z.grad - a.grad == steps && z.sum - a.sum == steps && z.rec - a.rec == steps && z.opt - a.opt == steps,
                "%ld steps: %ld env %ld grad %ld sum %ld record %ld update launches", steps, z.env - a.env, z.grad - a.grad, z.sum - a.sum, z.rec - a.rec, z.opt - a.opt);
          CHECK(z.cot - a.cot == z.red - a.red, "one reduction per cotangent");
          if (chunk == 64) CHECK(z.cot - a.cot >= 2 * ((b + 63) / 64), "chunks of 64: %ld cotangent launches for b %d", z.cot - a.cot, b);
          for (int k = 0; k < n_steps; ++k) CHECK(vals[(size_t)k * 4 + 3] == 0.0, "step %d is marked %g on a runtime that computes nothing", k, vals[(size_t)k * 4 + 3]);
          if (overlap) g_overlapped_steps += steps;
        }
  }
  OK(tnml_set_core_grad_chunk(ctx, 0));
  OK(tnml_set_nll_overlap(ctx, 0));
  OK(tnml_optim_config(ctx, TNML_OPT_SGD, 0.0, 0.9, 0.999, 1e-8, 1));
  OK(tnml_dataset_detach(ctx));
}

static void run_true_size(const char *name, int N, int D, int L, int M, int l_pos) {
  tnml_ctx *ctx = nullptr;
  OK(tnml_create(&ctx, N, D, L, M, 64, 0));
  OK(tnml_set_any_position(ctx, 1));
  Chain w(N, D, L, std::vector<int>(N - 1, M), l_pos);
  set_cores(ctx, w, l_pos);
  step_calls(ctx, N, D, L, 200);
  OK(tnml_set_chain_scaling(ctx, 1));                            // the scaled kernels of the same step
  step_calls(ctx, N, D, L, 70);
  OK(tnml_destroy(ctx));
  printf("planned likelihood steps %s bond %d L %d, label on %d\n", name, M, L, l_pos);
  fflush(stdout);
}

static void run_ragged(int N, int D, int L, int M) {
  tnml_ctx *ctx = nullptr;
  OK(tnml_create(&ctx, N, D, L, M, 64, 0));
  OK(tnml_set_any_position(ctx, 1));
  for (int l = 0; l < N; ++l) {
    std::vector<int> bw(N - 1);
    for (int i = 0; i < N - 1; ++i) bw[i] = 1 + (i * 7 + l * 3) % (M - 1);
    if (l >= N / 2) bw[(l * 5) % (N - 1)] = M;
    Chain w(N, D, L, bw, l);
    set_cores(ctx, w, l);
    OK(tnml_optim_reset(ctx));                                   // (other bonds, another l_pos)
    step_calls(ctx, N, D, L, l % 2 ? 70 : 17);
  }
  OK(tnml_destroy(ctx));
  printf("planned likelihood steps ragged N %d D %d L %d bonds <= %d at every label position\n", N, D, L, M);
  fflush(stdout);
}

static void run_refusals() {
  const int N = 6, D = 2, L = 3, M = 4, b = 5;
  tnml_ctx *ctx = nullptr;
  OK(tnml_create(&ctx, N, D, L, M, 64, 0));
  Chain w(N, D, L, std::vector<int>(N - 1, M), 2);
  std::vector<float> X((size_t)b * N * D, 0.5f);
  std::vector<int32_t> y(b, 1), idx(b, 0);
  std::vector<double> S((size_t)D * D, 0.5);
  double v[4 * b];
  FAILS_WITH(TNML_ERR_STATE, tnml_nll_step(ctx, X.data(), y.data(), b, nullptr, 1e-3f, 0.f, 1, v));            // cores never set
  set_cores(ctx, w, 2);
  FAILS_WITH(TNML_ERR_ARG, tnml_nll_step(nullptr, X.data(), y.data(), b, nullptr, 1e-3f, 0.f, 1, v));
  FAILS_WITH(TNML_ERR_ARG, tnml_nll_step(ctx, nullptr, y.data(), b, nullptr, 1e-3f, 0.f, 1, v));
  FAILS_WITH(TNML_ERR_ARG, tnml_nll_step(ctx, X.data(), y.data(), b, nullptr, 1e-3f, 0.f, 1, nullptr));
  FAILS_WITH(TNML_ERR_ARG, tnml_nll_step(ctx, X.data(), y.data(), 0, nullptr, 1e-3f, 0.f, 1, v));
  FAILS_WITH(TNML_ERR_ARG, tnml_nll_step(ctx, X.data(), y.data(), b, nullptr, 1e-3f, 0.f, 2, v));
  FAILS_WITH(TNML_ERR_ARG, tnml_nll_step(ctx, X.data(), y.data(), b, nullptr, 1e-3f, 0.f, -1, v));
  CHECK(strstr(tnml_last_error(), "renorm"), "the refusal does not say renorm: %s", tnml_last_error());
  y[3] = L;
  FAILS_WITH(TNML_ERR_ARG, tnml_nll_step(ctx, X.data(), y.data(), b, nullptr, 1e-3f, 0.f, 1, v));
  y[3] = 0;
  {
    std::vector<double> T(S);
    T[2] = 0.75;
    FAILS_WITH(TNML_ERR_ARG, tnml_nll_step(ctx, X.data(), y.data(), b, T.data(), 1e-3f, 0.f, 1, v));
    CHECK(strstr(tnml_last_error(), "symmetric"), "the refusal does not say symmetric: %s", tnml_last_error());
    T[2] = NAN;
    FAILS_WITH(TNML_ERR_ARG, tnml_nll_step(ctx, X.data(), y.data(), b, T.data(), 1e-3f, 0.f, 1, v));
  }
  FAILS_WITH(TNML_ERR_STATE, tnml_nll_train_indices(ctx, idx.data(), b, 2, 1, nullptr, 1e-3f, 0.f, 1, v));      // no dataset
  OK(tnml_dataset_attach(ctx, X.data(), y.data(), b, N, D, TNML_DATASET_FEATURES));
  FAILS_WITH(TNML_ERR_ARG, tnml_nll_train_indices(ctx, nullptr, b, 2, 1, nullptr, 1e-3f, 0.f, 1, v));
  FAILS_WITH(TNML_ERR_ARG, tnml_nll_train_indices(ctx, idx.data(), b, 2, 1, nullptr, 1e-3f, 0.f, 1, nullptr));
  FAILS_WITH(TNML_ERR_ARG, tnml_nll_train_indices(ctx, idx.data(), 0, 2, 1, nullptr, 1e-3f, 0.f, 1, v));
  FAILS_WITH(TNML_ERR_ARG, tnml_nll_train_indices(ctx, idx.data(), b, 0, 1, nullptr, 1e-3f, 0.f, 1, v));
  FAILS_WITH(TNML_ERR_ARG, tnml_nll_train_indices(ctx, idx.data(), b, 2, 1, nullptr, 1e-3f, 0.f, 2, v));
  idx[2] = b;
  FAILS_WITH(TNML_ERR_ARG, tnml_nll_train_indices(ctx, idx.data(), b, 2, 1, nullptr, 1e-3f, 0.f, 1, v));
  idx[2] = -1;
  FAILS_WITH(TNML_ERR_ARG, tnml_nll_train_indices(ctx, idx.data(), b, 2, 0, nullptr, 1e-3f, 0.f, 1, v));
  idx[2] = 0;
  FAILS_WITH(TNML_ERR_ARG, tnml_set_nll_overlap(ctx, 2));
  FAILS_WITH(TNML_ERR_ARG, tnml_set_nll_overlap(nullptr, 1));
  OK(tnml_nll_train_indices(ctx, idx.data(), b, 2, 1, S.data(), 1e-3f, 0.f, 1, v));                             // usable afterwards
  OK(tnml_nll_step(ctx, X.data(), nullptr, b, S.data(), 1e-3f, 0.f, 0, v));
  OK(tnml_destroy(ctx));
  // bond 64 is taken, bond 65 refused
  OK(tnml_create(&ctx, 4, 2, 2, 65, 64, 0));
  OK(tnml_set_any_position(ctx, 1));
  Chain fits(4, 2, 2, std::vector<int>{2, 64, 2}, 1), big(4, 2, 2, std::vector<int>{2, 65, 2}, 1);
  std::vector<float> X4((size_t)3 * 4 * 2, 0.5f);
  set_cores(ctx, big, 1);
  FAILS_WITH(TNML_ERR_ARG, tnml_nll_step(ctx, X4.data(), nullptr, 3, nullptr, 1e-3f, 0.f, 1, v));
  set_cores(ctx, fits, 1);
  OK(tnml_nll_step(ctx, X4.data(), nullptr, 3, nullptr, 1e-3f, 0.f, 1, v));
  OK(tnml_destroy(ctx));
  // with a communicator the call is refused
  setenv("TNML_FORCE_COMM", "1", 1);
  OK(tnml_create(&ctx, N, D, L, M, 64, 0));
  unsigned char uid[128];
  OK(tnml_comm_unique_id(uid));
  OK(tnml_comm_init(ctx, 0, 1, uid));
  Chain w0(N, D, L, std::vector<int>(N - 1, M), 0);
  set_cores(ctx, w0, 0);
  FAILS_WITH(TNML_ERR_STATE, tnml_nll_step(ctx, X.data(), y.data(), b, nullptr, 1e-3f, 0.f, 1, v));
  FAILS_WITH(TNML_ERR_STATE, tnml_nll_train_indices(ctx, idx.data(), b, 2, 1, nullptr, 1e-3f, 0.f, 1, v));
  OK(tnml_destroy(ctx));
  unsetenv("TNML_FORCE_COMM");
  printf("likelihood step refusals: ok\n");
}

// after a step: a sweep needs a forward, the resident batch stays, the state is bound as section 17 binds it
static void run_state_rule() {
  const int N = 8, D = 2, L = 2, M = 6, b = 40;
  const int kAct = TNML_ACT_SOFTMAX, kLoss = TNML_LOSS_FULL_CROSS_ENT;
  tnml_ctx *ctx = nullptr;
  OK(tnml_create(&ctx, N, D, L, M, 64, 0));
  std::vector<float> X((size_t)b * N * D, 0.5f), f((size_t)L * b);
  std::vector<int> lab(b, 1);
  Chain w(N, D, L, std::vector<int>(N - 1, 2), 0);
  double v[4], met[3];
  set_cores(ctx, w, 0);
  OK(tnml_optim_config(ctx, TNML_OPT_SGD, 0.9, 0.9, 0.999, 1e-8, 0));
  OK(tnml_set_input(ctx, X.data(), lab.data(), b));
  OK(tnml_forward(ctx, f.data()));
  OK(tnml_nll_step(ctx, X.data(), lab.data(), b, nullptr, 1e-3f, 0.f, 1, v));
  FAILS_WITH(TNML_ERR_STATE, tnml_sweep(ctx, 0, 2, 1, 1e-3f, 1e-3f, 1, kAct, kLoss, 0.1f, TNML_TRUNC_FIXED, nullptr, nullptr));
  OK(tnml_forward(ctx, f.data()));                               // (the resident batch is still there)
  OK(tnml_gd_step(ctx, X.data(), lab.data(), b, 0.1f, 0.f, kAct, kLoss, 0.1f, met));   // one state for both objectives
  OK(tnml_forward(ctx, f.data()));
  OK(tnml_sweep(ctx, 0, 2, 1, 1e-3f, 1e-3f, 1, kAct, kLoss, 0.1f, TNML_TRUNC_FIXED, nullptr, nullptr));
  FAILS_WITH(TNML_ERR_STATE, tnml_nll_step(ctx, X.data(), lab.data(), b, nullptr, 1e-3f, 0.f, 1, v));           // the sweep moved the label
  CHECK(strstr(tnml_last_error(), "tnml_optim_reset"), "the refusal does not name the remedy: %s", tnml_last_error());
  OK(tnml_optim_reset(ctx));
  OK(tnml_set_any_position(ctx, 1));
  OK(tnml_nll_step(ctx, X.data(), lab.data(), b, nullptr, 1e-3f, 0.f, 1, v));
  OK(tnml_destroy(ctx));
  printf("state rules of the likelihood step: ok\n");
}

// every allocation of the new group fails in turn, fresh and when a call of more steps makes it grow
static void run_alloc_failures(int D) {
  const int N = 6, L = 2, M = 12, b = 70;
  tnml_ctx *ctx = nullptr;
  OK(tnml_create(&ctx, N, D, L, M, 64, 0));
  OK(tnml_set_any_position(ctx, 1));
  Chain w(N, D, L, std::vector<int>(N - 1, 3), 3);
  set_cores(ctx, w, 3);
  std::vector<float> X((size_t)b * N * D, 0.5f);
  std::vector<int32_t> y(b, 1), idx(b, 0);
  std::vector<double> vals((size_t)b * 4);
  OK(tnml_optim_config(ctx, TNML_OPT_ADAM, 0.0, 0.9, 0.999, 1e-8, 0));
  int k = fail_each_alloc("tnml_nll_step, fresh context", [&] { return tnml_nll_step(ctx, X.data(), y.data(), b, nullptr, 1e-3f, 0.f, 1, vals.data()); });
  if (k < 4) { fprintf(stderr, "%d allocations failed in turn, the state and record groups alone have 4\n", k); exit(1); }
  k = fail_each_alloc("tnml_nll_step, the groups exist", [&] { return tnml_nll_step(ctx, X.data(), y.data(), b, nullptr, 1e-3f, 0.f, 1, vals.data()); });
  if (k != 0) { fprintf(stderr, "%d allocations in a second call\n", k); exit(1); }
  OK(tnml_dataset_attach(ctx, X.data(), y.data(), b, N, D, TNML_DATASET_FEATURES));
  k = fail_each_alloc("tnml_nll_train_indices, more steps", [&] { return tnml_nll_train_indices(ctx, idx.data(), b, 9, 1, nullptr, 1e-3f, 0.f, 1, vals.data()); });
  if (k < 2) { fprintf(stderr, "%d allocations failed in turn when the record group grew, it has 2\n", k); exit(1); }
  OK(tnml_destroy(ctx));
}

// Every launch of the environment kernel on a stream other than the one of the gradient kernel behind it must be forked and joined:
//   event_record eF sY; stream_wait sX eF; ... launch lognorm_env_kernel stream=sX; event_record eJ sX; ... stream_wait sY eJ; ... launch lognorm_grad_kernel stream=sY
static long check_trace(const char *path) {
  std::ifstream in(path);
  std::vector<std::string> ln;
  for (std::string s; std::getline(in, s);) ln.push_back(s);
  auto stream_of = [](const std::string &s) { const size_t at = s.find(" stream=s"); return at == std::string::npos ? std::string() : s.substr(at + 9, s.find(' ', at + 9) - at - 9); };
  long found = 0;
  for (size_t i = 0; i < ln.size(); ++i) {
    if (ln[i].rfind("launch ", 0) != 0 || ln[i].find("lognorm_env_kernel") == std::string::npos) continue;
    const std::string sx = stream_of(ln[i]);
    size_t g = i + 1;
    while (g < ln.size() && !(ln[g].rfind("launch ", 0) == 0 && ln[g].find("lognorm_grad_kernel") != std::string::npos) &&
           !(ln[g].rfind("launch ", 0) == 0 && ln[g].find("lognorm_env_kernel") != std::string::npos)) ++g;
    if (g == ln.size() || ln[g].find("lognorm_grad_kernel") == std::string::npos) continue;      // (a value alone: no gradient launch)
    const std::string sy = stream_of(ln[g]);
    if (sx == sy) continue;
    // backwards: the wait of sX on an event recorded on sY
    std::string ef;
    size_t w = i;
    while (w-- > 0) if (ln[w].rfind("stream_wait s" + sx + " e", 0) == 0) { ef = ln[w].substr(ln[w].rfind('e')); break; }
    CHECK(!ef.empty(), "line %zu: the environment kernel on s%s waits for nothing", i + 1, sx.c_str());
    bool rec = false;
    for (size_t r = w; r-- > 0 && !rec;) if (ln[r] == "event_record " + ef + " s" + sy) rec = true;
    CHECK(rec, "line %zu: %s was never recorded on s%s", w + 1, ef.c_str(), sy.c_str());
    // forwards: the join before the gradient kernel
    std::string ej;
    size_t j = i + 1;
    for (; j < g; ++j) if (ln[j].rfind("event_record e", 0) == 0 && ln[j].size() > sx.size() + 2 && ln[j].substr(ln[j].size() - sx.size() - 2) == " s" + sx) { ej = ln[j].substr(13, ln[j].find(' ', 13) - 13); break; }
    CHECK(!ej.empty(), "line %zu: nothing recorded on s%s behind the environment kernel", i + 1, sx.c_str());
    bool joined = false;
    for (size_t q = j + 1; q < g; ++q) if (ln[q] == "stream_wait s" + sy + " " + ej) joined = true;
    CHECK(joined, "line %zu: s%s does not wait for %s before the gradient kernel", g + 1, sy.c_str(), ej.c_str());
    ++found;
  }
  return found;
}

int main(int argc, char **argv) {
  if (argc > 1 && !strcmp(argv[1], "trace")) {                   // a short chain alone keeps the trace small
    const char *tr = getenv("TNML_SAN_TRACE");
    CHECK(tr && *tr, "the trace mode needs TNML_SAN_TRACE");
    run_ragged(17, 2, 3, 5);
    san_stub_report();
    const long found = check_trace(tr);
    CHECK(found == g_overlapped_steps && found > 0, "%ld steps ran with the overlap on, the trace shows %ld forks and joins", g_overlapped_steps, found);
    printf("nll-step: %ld overlapped steps, each forked and joined by an event in the trace\n", found);
    return 0;
  }
  run_true_size("c3", 784, 2, 2, 20, 0);
  run_true_size("c3 inner label", 784, 2, 2, 20, 391);
  run_true_size("c5", 784, 2, 10, 50, 783);
  run_true_size("c5 inner label", 784, 2, 10, 50, 400);
  run_ragged(17, 2, 3, 5);
  run_ragged(17, 3, 3, 7);
  run_ragged(17, 8, 17, 6);
  run_ragged(2, 2, 2, 5);
  run_refusals();
  run_state_rule();
  run_alloc_failures(2);
  run_alloc_failures(3);
  san_stub_report();
  const char *paths[] = {"lognorm_env_kernel", "lognorm_grad_kernel", "nll_cot_kernel", "nll_sum_kernel", "nll_record_kernel", "optim_step_kernel",
                         "core_grad_chain_scaled_kernel", "core_grad_chain_kernel"};
  for (const char *k : paths)
    if (san_stub_launches(k) < 1) { fprintf(stderr, "launch path %s was never taken\n", k); return 1; }
  printf("nll-step: %ld nll_record_kernel and %ld optim_step_kernel launches checked, %d refusals\n", san_stub_launches("nll_record_kernel"),
         san_stub_launches("optim_step_kernel"), g_refusals);
  printf("likelihood step host planning under ASan + UBSan: ok\n");
  return 0;
}
