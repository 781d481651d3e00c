// One context through every state change and every call behind it (tests/context_lifecycle_cases.py: the mutators, readers and
// consumers of tests/test_context_lifecycle_gpu.py), planned by the real host code, built --cuda-host-only with AddressSanitizer and
// UBSan, against the stand-in runtime of hip_stub.cpp.  The stand-in's extent checks are the assertion: every pointer of every launch
// must lie inside a live allocation of sufficient size, which is what a capacity group sized for the bonds or the batch of before a
// mutator would miss.  Per shape: warm-up (every call once at the start state), then mutator after mutator on the SAME context, each
// followed by every call.  Nothing computes there: a compress keeps the bonds it started from (plan_orth_main.cpp), so the shrink is
// a tnml_set_cores of the cut bonds behind it, and a sum that would pass the capacity starts from halved bonds.  Shapes A, B and C of
// the tables, and C3 / C5 at true size.  `make san-lifecycle` builds and runs it; tests/test_context_lifecycle_host.py runs
// `make san-lifecycle`.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../tnml_internal.h"

extern "C" void san_stub_report(void);
extern "C" long san_stub_launches(const char *substr);
extern "C" void san_stub_site_cond_call(int on);

static int g_refusals = 0;
static long g_calls = 0;

#define OK(call)                                                                              \
  do {                                                                                        \
    int rc_ = (call);                                                                         \
    ++g_calls;                                                                                \
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
static const float kLr = 1e-2f, kWd = 1e-3f, kT = 0.1f;

struct Chain {
  std::vector<int32_t> bond;
  std::vector<float> flat;
  Chain(int N, int D, int L, const std::vector<int> &b, int l_pos, float v = 0.1f) : bond(b.begin(), b.end()) {
    size_t total = 0;
    for (int i = 0; i < N; ++i) total += (size_t)(i == 0 ? 1 : b[i - 1]) * D * (i == N - 1 ? 1 : b[i]) * (i == l_pos ? L : 1);
    flat.assign(total, v);
  }
};

struct Shape {
  const char *name;
  int N, D, L, M;
  int narrow;                     // tnml_set_narrow_path
  std::vector<int> bond;          // the start bonds
  int b[3];                       // the capacity and first batch, the batch that grows the group, the one that shrinks
  int cap() const { return std::max(M, D * std::min(L, M)); }
};

struct Run {
  const Shape &s;
  tnml_ctx *ctx = nullptr;
  int b_now;
  static const int kDs = 96, kK = 8, kDraw = 19, kPred = 45;
  std::vector<float> pixels, Xp, Xg;
  std::vector<int32_t> ds_y, yp, yg, idx, idx_sel, known;
  std::vector<double> phi, w, S;
  std::vector<uint8_t> mask;

  explicit Run(const Shape &sh) : s(sh), b_now(sh.b[0]) {
    const int N = s.N, D = s.D, L = s.L;
    pixels.assign((size_t)kDs * N, 0.25f);
    ds_y.resize(kDs); idx.resize(41); idx_sel.resize(53);
    for (int i = 0; i < kDs; ++i) ds_y[i] = i % L;
    for (int i = 0; i < 41; ++i) idx[i] = (i * 7) % kDs;
    for (int i = 0; i < 53; ++i) idx_sel[i] = (i * 11 + 3) % kDs;
    Xp.assign((size_t)kPred * N * D, 0.5f); yp.resize(kPred);
    for (int i = 0; i < kPred; ++i) yp[i] = i % L;
    Xg.assign((size_t)kDraw * N * D, 0.5f); yg.resize(kDraw);
    for (int i = 0; i < kDraw; ++i) yg[i] = (i + 1) % L;
    phi.assign((size_t)kK * D, 0.5); w.assign(kK, 1.0 / kK); S.assign((size_t)D * D, 0.25);
    for (int d = 0; d < D; ++d) S[(size_t)d * D + d] = 0.5;
    known.assign((size_t)kDraw * N, 0);
    for (size_t i = 0; i < known.size(); ++i) known[i] = (int)(i % kK);
    mask.resize(N);
    for (int i = 0; i < N; ++i) mask[i] = i % 2 == 0;
  }

  std::vector<int> bonds(int *l_pos = nullptr) const {
    std::vector<int32_t> b32(s.N - 1);
    int lp = -1;
    OK(tnml_get_bonds(ctx, b32.data(), &lp));
    if (l_pos) *l_pos = lp;
    return std::vector<int>(b32.begin(), b32.end());
  }
  void set_cores(const std::vector<int> &b, int l_pos) {
    Chain c(s.N, s.D, s.L, b, l_pos);
    OK(tnml_set_cores(ctx, c.flat.data(), c.flat.size(), c.bond.data(), l_pos));
  }
  void set_input(int b) {
    std::vector<float> X((size_t)b * s.N * s.D, 0.5f);
    std::vector<int32_t> y(b);
    for (int i = 0; i < b; ++i) y[i] = i % s.L;
    OK(tnml_set_input(ctx, X.data(), y.data(), b));
    b_now = b;
  }
  void start() { set_cores(s.bond, 0); set_input(s.b[0]); }
  bool left() const { return tnml_l_pos(ctx) == s.N - 1; }
  size_t merged(int *pml = nullptr, int *pmr = nullptr) const {
    int l;
    const std::vector<int> b = bonds(&l);
    const int p = left() ? l - 1 : l;
    const int ml = p == 0 ? 1 : b[p - 1], mr = p == s.N - 2 ? 1 : b[p + 1];
    if (pml) *pml = ml;
    if (pmr) *pmr = mr;
    return (size_t)ml * s.D * s.D * mr * s.L;
  }

  // ---- the readers ---------------------------------------------------------------------------------------------------------------
  void forward() { std::vector<float> f((size_t)s.L * b_now); OK(tnml_forward(ctx, f.data())); }
  void readers(bool refused_before_forward) {
    const int N = s.N, D = s.D, L = s.L, cap = s.cap();
    double m3[3];
    const size_t bs = merged();
    std::vector<double> Bnew(bs), l2g(bs);
    std::vector<float> Bin(bs, 0.1f);
    float met2[2];
    double l2 = 0;
    if (refused_before_forward) {                                  // no f, no environments: TNML_ERR_STATE until a forward
      FAILS_WITH(TNML_ERR_STATE, tnml_resident_metrics(ctx, kAct, kT, m3));
      // (not FAILS_WITH: the norm environments of the L2 term, which hang on the cores alone, are built before the refusal)
      int rc = tnml_update_B(ctx, nullptr, left(), kLr, kWd, 1, kAct, kLoss, kT, Bnew.data(), bs, met2);
      if (rc != TNML_ERR_STATE) { fprintf(stderr, "tnml_update_B without a forward -> %d\n", rc); exit(1); }
      ++g_refusals;
    }
    forward();
    OK(tnml_resident_metrics(ctx, kAct, kT, m3));
    std::vector<float> env((size_t)b_now * cap * 2);
    int m = 0;
    const int l = tnml_l_pos(ctx);
    for (int i = 0; i < l; ++i) OK(tnml_get_env(ctx, TNML_SIDE_LEFT, i, env.data(), env.size(), &m));
    for (int i = l + 1; i < N; ++i) OK(tnml_get_env(ctx, TNML_SIDE_RIGHT, i, env.data(), env.size(), &m));
    OK(tnml_update_B(ctx, nullptr, left(), kLr, kWd, 1, kAct, kLoss, kT, Bnew.data(), bs, met2));
    OK(tnml_l2_term(ctx, Bin.data(), left(), kWd, &l2, l2g.data(), bs));
    std::vector<float> f((size_t)L * kPred), mant((size_t)L * kPred), g((size_t)kPred * N * D), cf(kPred);
    std::vector<int32_t> expo(kPred);
    OK(tnml_predict(ctx, Xp.data(), kPred, f.data()));
    OK(tnml_predict_scaled(ctx, Xp.data(), kPred, mant.data(), expo.data()));
    OK(tnml_predict_indices(ctx, idx.data(), (int)idx.size(), f.data()));
    OK(tnml_eval_indices(ctx, idx.data(), (int)idx.size(), kAct, kT, m3));
    OK(tnml_input_grad(ctx, Xp.data(), kPred, nullptr, g.data(), cf.data()));
    size_t nc = 0;
    OK(tnml_cores_size(ctx, &nc));
    std::vector<float> G(nc);
    OK(tnml_core_grad(ctx, Xp.data(), kPred, nullptr, G.data(), nc, cf.data()));
    OK(tnml_core_grad_indices(ctx, idx.data(), (int)idx.size(), nullptr, G.data(), nc, cf.data()));
    double sl[2], o3[3];
    OK(tnml_log_norm_grad(ctx, S.data(), 0, G.data(), nc, sl));
    OK(tnml_nll_grad(ctx, Xg.data(), yg.data(), kDraw, S.data(), G.data(), nc, o3));
    OK(tnml_nll_eval(ctx, Xg.data(), yg.data(), kDraw, S.data(), o3));
    std::vector<int32_t> rank(N - 1);
    std::vector<double> sigma((size_t)(N - 1) * cap);
    double logn = 0;
    OK(tnml_bond_spectra(ctx, 1e-6, rank.data(), sigma.data(), &logn));
    Chain v(N, D, L, std::vector<int>(N - 1, std::min(3, cap)), l);
    double o6[6];
    OK(tnml_inner(ctx, v.flat.data(), v.flat.size(), v.bond.data(), l, nullptr, 0, o6));
    OK(tnml_inner(ctx, nullptr, 0, nullptr, 0, nullptr, 0, o6));
    {
      const std::vector<int> b = bonds();
      if (*std::max_element(b.begin(), b.end()) <= 64) {           // the samplers and the conditionals take bonds up to 64
        std::vector<int32_t> lev((size_t)kDraw * N), lab(kDraw), mode((size_t)kDraw * N);
        std::vector<double> lp((size_t)kDraw * 2), clw(L), q((size_t)kDraw * N * D * D), st((size_t)kDraw * N * 4), lp1(kDraw);
        OK(tnml_sample(ctx, kDraw, kK, phi.data(), w.data(), nullptr, nullptr, 0, nullptr, 7, lev.data(), lab.data(), lp.data()));
        OK(tnml_sample_masked(ctx, kDraw, kK, phi.data(), w.data(), nullptr, mask.data(), 1, known.data(), nullptr, 7, 1, lev.data(), lab.data(),
                              lp.data(), clw.data()));
        san_stub_site_cond_call(1);                                // (which tile rule the stand-in holds the environment launches to)
        OK(tnml_site_conditionals(ctx, kDraw, kK, phi.data(), w.data(), nullptr, nullptr, mask.data(), 1, known.data(), q.data(), st.data(),
                                  mode.data(), lp1.data()));
        san_stub_site_cond_call(0);
      }
    }
  }

  // ---- the consumers, each from the state (bond, l_pos) ----------------------------------------------------------------------------
  void sweep_to_the_end(int policy = TNML_TRUNC_FIXED) {
    forward();
    const int l = tnml_l_pos(ctx), N = s.N;
    std::vector<float> met((size_t)N * 2), f((size_t)s.L * b_now);
    if (l == N - 1) OK(tnml_sweep(ctx, 1, N - 1, 1, kLr, kWd, 1, kAct, kLoss, kT, policy, met.data(), f.data()));
    else OK(tnml_sweep(ctx, 0, N - 1 - l, l == 0, kLr, kWd, 1, kAct, kLoss, kT, policy, met.data(), f.data()));
  }
  void gd_step() { double m3[3]; OK(tnml_gd_step(ctx, Xp.data(), yp.data(), kPred, kLr, kWd, kAct, kLoss, kT, m3)); }
  void nll_step() { double v4[4]; OK(tnml_nll_step(ctx, Xg.data(), yg.data(), kDraw, S.data(), 1e-3f, kWd, 1, v4)); }
  void compress(int m_max) {
    const int N = s.N;
    std::vector<int32_t> bo(N - 1);
    std::vector<double> sigma((size_t)(N - 1) * s.cap()), disc(N - 1);
    double logn = 0;
    OK(tnml_compress(ctx, m_max, 1.0, 1e-6, bo.data(), sigma.data(), disc.data(), &logn));
    int l;
    std::vector<int> b = bonds(&l);                               // what the device would have committed
    for (int &v : b) v = std::min(v, m_max);
    set_cores(b, l);
  }
  void consumers(bool rebound) {
    int l;
    const std::vector<int> b = bonds(&l);
    double m3[3];
    sweep_to_the_end();
    set_cores(b, l);
    if (rebound) {                                                 // vel / m / v belong to other bonds or another l_pos
      FAILS_WITH(TNML_ERR_STATE, tnml_gd_step(ctx, Xp.data(), yp.data(), kPred, kLr, kWd, kAct, kLoss, kT, m3));
      OK(tnml_optim_reset(ctx));
    }
    gd_step();
    set_cores(b, l);
    nll_step();
    set_cores(b, l);
    compress(3);
    set_cores(b, l);
  }
  void every_call(bool refused_before_forward, bool rebound) { readers(refused_before_forward); consumers(rebound); }

  // ---- the mutators ----------------------------------------------------------------------------------------------------------------
  int reference_steps() const {                                    // steps of a right sweep the reference's rule allows from the bonds of now
    std::vector<int> b = bonds();
    const int N = s.N;
    for (int p = 0; p < N - 1; ++p) {
      const int m = tnml_trunc_rank(TNML_TRUNC_REFERENCE, 0, p, N, p == 0 ? 1 : b[p - 1], s.D, p == N - 2 ? 1 : b[p + 1], s.L, s.M);
      if (m < 1) return p;
      b[p] = m;
    }
    return N - 1;
  }
  // -> (the f and the environments are gone: refusals until a forward, the optimiser state is unbound)
  void mutate(int which, bool &no_f, bool &rebound) {
    const int N = s.N, cap = s.cap();
    no_f = true; rebound = false;
    int l;
    std::vector<int> b = bonds(&l);
    switch (which) {
      case 0: set_cores(b, l); break;                                                       // set_cores
      case 1: {                                                                             // set_cores_bonds
        for (int i = 0; i < N - 1; ++i) b[i] = 1 + (i * 7 + 2) % std::min(cap, 5);
        set_cores(b, N - 1); rebound = true; break;
      }
      case 2: OK(tnml_scale_cores(ctx, 0.9)); break;
      case 3: start(); forward(); {                                                         // sweep_right
        OK(tnml_sweep(ctx, 0, N - 1, 1, kLr, kWd, 1, kAct, kLoss, kT, TNML_TRUNC_FIXED, nullptr, nullptr));
        no_f = false; rebound = true; break;
      }
      case 4: start(); {                                                                    // sweep_reference
        const int n = reference_steps();
        if (n < N - 1) OK(tnml_set_any_position(ctx, 1));
        forward();
        OK(tnml_sweep(ctx, 0, n, 1, kLr, kWd, 1, kAct, kLoss, kT, TNML_TRUNC_REFERENCE, nullptr, nullptr));
        no_f = false; rebound = true; break;
      }
      case 5: start(); OK(tnml_set_any_position(ctx, 1)); forward();                        // segment
        OK(tnml_sweep(ctx, 0, 3, 1, kLr, kWd, 1, kAct, kLoss, kT, TNML_TRUNC_FIXED, nullptr, nullptr));
        no_f = false; rebound = true; break;
      case 6: OK(tnml_optim_config(ctx, TNML_OPT_SGD, 0.9, 0.9, 0.999, 1e-8, 1)); gd_step(); break;
      case 7: OK(tnml_optim_config(ctx, TNML_OPT_ADAM, 0.0, 0.9, 0.999, 1e-8, 0)); gd_step(); break;
      case 8: nll_step(); break;
      case 9: {                                                                             // orthogonalize
        std::vector<int32_t> bo(N - 1);
        double logn = 0;
        OK(tnml_orthogonalize(ctx, 1e-6, bo.data(), &logn));
        rebound = true; break;
      }
      case 10: compress(3); rebound = true; break;
      case 11: {                                                                            // axpby
        if (*std::max_element(b.begin(), b.end()) >= cap) {
          for (int &v : b) v = std::max(1, v / 2);
          set_cores(b, l);
        }
        std::vector<int> add(N - 1);
        for (int i = 0; i < N - 1; ++i) add[i] = std::min(b[i], cap - b[i]);
        Chain v(N, s.D, s.L, add, l);
        std::vector<int32_t> bo(N - 1);
        OK(tnml_axpby(ctx, 0.7, 0.4, v.flat.data(), v.flat.size(), v.bond.data(), l, bo.data()));
        for (int i = 0; i < N - 1; ++i)
          if (bo[i] != b[i] + add[i]) { fprintf(stderr, "bond %d after the sum is %d\n", i, bo[i]); exit(1); }
        rebound = true; break;
      }
      case 12: set_input(s.b[1]); break;
      case 13: set_input(s.b[2]); break;
      case 14: OK(tnml_select_indices(ctx, idx_sel.data(), (int)idx_sel.size())); b_now = (int)idx_sel.size(); break;
      case 15: {                                                                            // stage_batch + select_batch
        const int bb = s.b[1];
        std::vector<float> X((size_t)bb * N * s.D, 0.5f);
        std::vector<int32_t> y(bb, 0);
        OK(tnml_stage_batch(ctx, 3, X.data(), y.data(), bb));
        OK(tnml_select_batch(ctx, 3));
        b_now = bb; break;
      }
      case 16: { std::vector<int32_t> y(b_now, 1); OK(tnml_set_labels(ctx, y.data(), b_now)); break; }
      case 17: OK(tnml_set_chain_scaling(ctx, 1)); break;
      case 18: OK(tnml_set_chain_scaling(ctx, 0)); break;
    }
  }

  void run() {
    OK(tnml_create(&ctx, s.N, s.D, s.L, s.M, s.b[0], 0));
    if (s.narrow) OK(tnml_set_narrow_path(ctx, 1));
    OK(tnml_optim_config(ctx, TNML_OPT_ADAM, 0.0, 0.9, 0.999, 1e-8, 0));
    OK(tnml_dataset_attach(ctx, pixels.data(), ds_y.data(), kDs, s.N, s.D, TNML_DATASET_PIXELS));
    start();
    every_call(true, false);                                       // the warm-up: every group exists
    OK(tnml_optim_reset(ctx));
    for (int which = 0; which < 19; ++which) {
      bool no_f, rebound;                                          // (every_call ends with a tnml_set_cores: only a sweep leaves an f)
      mutate(which, no_f, rebound);
      every_call(no_f, rebound);
      OK(tnml_optim_reset(ctx));
    }
    OK(tnml_destroy(ctx));
    printf("planned the life cycle of shape %s: N %d D %d L %d M %d, batches %d / %d / %d\n", s.name, s.N, s.D, s.L, s.M, s.b[0], s.b[1], s.b[2]);
    fflush(stdout);
  }
};

int main() {
  const std::vector<int> ragged{2, 4, 4, 3, 4, 4, 2};
  const Shape shapes[] = {
      {"A", 8, 2, 3, 12, 0, ragged, {37, 70, 5}},
      {"B", 8, 3, 3, 12, 0, ragged, {37, 70, 5}},
      {"C", 8, 2, 3, 12, 1, ragged, {37, 70, 5}},
      {"C3", 784, 2, 2, 20, 0, std::vector<int>(783, 20), {200, 333, 5}},
      {"C5", 784, 2, 10, 50, 0, std::vector<int>(783, 50), {200, 333, 5}},
  };
  for (const Shape &s : shapes) Run(s).run();
  san_stub_report();
  printf("life cycle: %ld calls planned, %d refusals\n", g_calls, g_refusals);
  printf("plan_lifecycle: OK\n");
  return 0;
}
