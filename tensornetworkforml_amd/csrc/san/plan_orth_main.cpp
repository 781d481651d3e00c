// Orthogonal form, compression and bond spectra (tnml_orthogonalize / tnml_compress / tnml_bond_spectra of api_mps.hip and the launch
// wrapper of kernels_orth.hip) planned by the real host code, built --cuda-host-only with AddressSanitizer and UBSan, against the
// stand-in runtime of hip_stub.cpp, which walks the operation list of every call and checks every slot, scratch and output pointer
// of the parameter block with its extent.  Nothing computes there: the scratch bond table comes back as it was uploaded, so every
// planned call commits the bonds it started from.  `make san-orth` builds and runs it; tests/test_orthogonalize_host.py runs
// `make san-orth`.
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

static void set_cores(tnml_ctx *ctx, int N, int D, int L, const std::vector<int> &bond, int l_pos) {
  size_t total = 0;
  for (int i = 0; i < N; ++i) total += (size_t)(i == 0 ? 1 : bond[i - 1]) * D * (i == N - 1 ? 1 : bond[i]) * (i == l_pos ? L : 1);
  std::vector<float> cores(total, 0.1f);
  OK(tnml_set_cores(ctx, cores.data(), total, bond.data(), l_pos));
}

struct Out {
  std::vector<int32_t> bond;
  std::vector<double> sigma, disc;
  double logn = 0;
  Out(int N, int cap) : bond(N - 1), sigma((size_t)(N - 1) * cap), disc(N - 1) {}
};

// the three calls; each is one load, one chain and one store launch
static void three_calls(tnml_ctx *ctx, int N, int cap, int m_max) {
  Out o(N, cap);
  const long a = san_stub_launches("orth_chain_kernel"), b = san_stub_launches("orth_load_kernel"), c = san_stub_launches("orth_store_kernel");
  OK(tnml_bond_spectra(ctx, 1e-6, o.bond.data(), o.sigma.data(), &o.logn));
  OK(tnml_orthogonalize(ctx, 1e-6, o.bond.data(), &o.logn));
  OK(tnml_compress(ctx, m_max, 1.0, 0.0, o.bond.data(), o.sigma.data(), o.disc.data(), &o.logn));
  OK(tnml_compress(ctx, cap, 0.9, 1e-6, o.bond.data(), o.sigma.data(), o.disc.data(), &o.logn));
  if (san_stub_launches("orth_chain_kernel") - a != 4 || san_stub_launches("orth_load_kernel") - b != 4 || san_stub_launches("orth_store_kernel") - c != 4) {
    fprintf(stderr, "four calls did not make four launches of each kernel\n");
    exit(1);
  }
}

static void run_true_size(const char *name, int N, int D, int L, int M, int l_pos) {
  tnml_ctx *ctx = nullptr;
  OK(tnml_create(&ctx, N, D, L, M, 64, 0));
  set_cores(ctx, N, D, L, std::vector<int>(N - 1, M), l_pos);
  three_calls(ctx, N, M > D * (L < M ? L : M) ? M : D * (L < M ? L : M), M / 2);
  OK(tnml_destroy(ctx));
  printf("planned orthogonal form %s bond %d L %d, label on %d\n", name, M, L, l_pos);
  fflush(stdout);
}

// a ragged 17-site chain at every label position
static void run_ragged(int D, int L, int M) {
  const int N = 17;
  tnml_ctx *ctx = nullptr;
  OK(tnml_create(&ctx, N, D, L, M, 64, 0));
  const int cap = M > D * (L < M ? L : M) ? M : D * (L < M ? L : M);
  for (int l = 0; l < N; ++l) {
    std::vector<int> bond(N - 1);
    for (int i = 0; i < N - 1; ++i) bond[i] = 1 + (i * 7 + l * 3) % M;
    bond[(l * 5) % (N - 1)] = M;
    set_cores(ctx, N, D, L, bond, l);
    three_calls(ctx, N, cap, 2);
  }
  OK(tnml_destroy(ctx));
  printf("planned orthogonal form ragged N %d D %d L %d bond <= %d at every label position\n", N, D, L, M);
  fflush(stdout);
}

static void run_refusals() {
  const int N = 6, D = 2, L = 3, M = 4, cap = 6;
  tnml_ctx *ctx = nullptr;
  OK(tnml_create(&ctx, N, D, L, M, 64, 0));
  Out o(N, cap);
  int32_t *bo = o.bond.data();
  double *sg = o.sigma.data(), *dc = o.disc.data(), *ln = &o.logn;
  FAILS_WITH(TNML_ERR_STATE, tnml_orthogonalize(ctx, 1e-6, bo, ln));                                  // cores never set
  FAILS_WITH(TNML_ERR_STATE, tnml_compress(ctx, 2, 1.0, 1e-6, bo, sg, dc, ln));
  FAILS_WITH(TNML_ERR_STATE, tnml_bond_spectra(ctx, 1e-6, bo, sg, ln));
  set_cores(ctx, N, D, L, std::vector<int>(N - 1, M), 2);
  FAILS_WITH(TNML_ERR_ARG, tnml_orthogonalize(nullptr, 1e-6, bo, ln));
  FAILS_WITH(TNML_ERR_ARG, tnml_orthogonalize(ctx, 1e-6, nullptr, ln));
  FAILS_WITH(TNML_ERR_ARG, tnml_orthogonalize(ctx, 1e-6, bo, nullptr));
  FAILS_WITH(TNML_ERR_ARG, tnml_orthogonalize(ctx, -1e-6, bo, ln));
  FAILS_WITH(TNML_ERR_ARG, tnml_orthogonalize(ctx, 1.0, bo, ln));
  FAILS_WITH(TNML_ERR_ARG, tnml_compress(nullptr, 2, 1.0, 1e-6, bo, sg, dc, ln));
  FAILS_WITH(TNML_ERR_ARG, tnml_compress(ctx, 0, 1.0, 1e-6, bo, sg, dc, ln));
  FAILS_WITH(TNML_ERR_ARG, tnml_compress(ctx, -3, 1.0, 1e-6, bo, sg, dc, ln));
  FAILS_WITH(TNML_ERR_ARG, tnml_compress(ctx, 2, 0.0, 1e-6, bo, sg, dc, ln));
  FAILS_WITH(TNML_ERR_ARG, tnml_compress(ctx, 2, 1.0001, 1e-6, bo, sg, dc, ln));
  FAILS_WITH(TNML_ERR_ARG, tnml_compress(ctx, 2, 1.0, 1.0, bo, sg, dc, ln));
  FAILS_WITH(TNML_ERR_ARG, tnml_compress(ctx, 2, 1.0, 1e-6, nullptr, sg, dc, ln));
  FAILS_WITH(TNML_ERR_ARG, tnml_compress(ctx, 2, 1.0, 1e-6, bo, nullptr, dc, ln));
  FAILS_WITH(TNML_ERR_ARG, tnml_compress(ctx, 2, 1.0, 1e-6, bo, sg, nullptr, ln));
  FAILS_WITH(TNML_ERR_ARG, tnml_compress(ctx, 2, 1.0, 1e-6, bo, sg, dc, nullptr));
  FAILS_WITH(TNML_ERR_ARG, tnml_bond_spectra(nullptr, 1e-6, bo, sg, ln));
  FAILS_WITH(TNML_ERR_ARG, tnml_bond_spectra(ctx, 1e-6, nullptr, sg, ln));
  FAILS_WITH(TNML_ERR_ARG, tnml_bond_spectra(ctx, 1e-6, bo, nullptr, ln));
  FAILS_WITH(TNML_ERR_ARG, tnml_bond_spectra(ctx, 1e-6, bo, sg, nullptr));
  FAILS_WITH(TNML_ERR_ARG, tnml_bond_spectra(ctx, 3.0, bo, sg, ln));
  three_calls(ctx, N, cap, 2);                                                                        // usable afterwards
  OK(tnml_destroy(ctx));
  // a bond the kernel's LDS has no room for: refused with the bytes in the message
  OK(tnml_create(&ctx, 4, 2, 2, 128, 64, 0));
  set_cores(ctx, 4, 2, 2, std::vector<int>{2, 128, 2}, 0);
  Out big(4, 128);
  FAILS_WITH(TNML_ERR_SHAPE, tnml_orthogonalize(ctx, 1e-6, big.bond.data(), &big.logn));
  if (!strstr(tnml_last_error(), "bytes of LDS")) { fprintf(stderr, "LDS refusal does not name the bytes: %s\n", tnml_last_error()); exit(1); }
  FAILS_WITH(TNML_ERR_SHAPE, tnml_bond_spectra(ctx, 1e-6, big.bond.data(), big.sigma.data(), &big.logn));
  set_cores(ctx, 4, 2, 2, std::vector<int>{2, 96, 2}, 0);                                            // the largest bond it takes
  OK(tnml_orthogonalize(ctx, 1e-6, big.bond.data(), &big.logn));
  OK(tnml_destroy(ctx));
  // with a communicator every call is refused
  setenv("TNML_FORCE_COMM", "1", 1);
  OK(tnml_create(&ctx, N, D, L, M, 64, 0));
  unsigned char uid[128];
  OK(tnml_comm_unique_id(uid));
  OK(tnml_comm_init(ctx, 0, 1, uid));
  set_cores(ctx, N, D, L, std::vector<int>(N - 1, M), 0);
  FAILS_WITH(TNML_ERR_STATE, tnml_orthogonalize(ctx, 1e-6, bo, ln));
  FAILS_WITH(TNML_ERR_STATE, tnml_compress(ctx, 2, 1.0, 1e-6, bo, sg, dc, ln));
  FAILS_WITH(TNML_ERR_STATE, tnml_bond_spectra(ctx, 1e-6, bo, sg, ln));
  OK(tnml_destroy(ctx));
  unsetenv("TNML_FORCE_COMM");
  printf("orthogonal-form refusals: ok\n");
}

// a committed call leaves the context as tnml_scale_cores does (no sweep without a forward) and unbinds a bound optimiser state even
// where no bond changed; tnml_bond_spectra leaves everything as it was
static void run_state_rule() {
  const int N = 8, D = 2, L = 2, M = 4, b = 40;
  tnml_ctx *ctx = nullptr;
  OK(tnml_create(&ctx, N, D, L, M, 64, 0));
  std::vector<float> X((size_t)b * N * D, 0.5f), f((size_t)L * b);
  std::vector<int> lab(b, 1);
  Out o(N, M);
  double met[3];
  for (int which = 1; which < 3; ++which) {
    set_cores(ctx, N, D, L, std::vector<int>(N - 1, 2), 0);
    if (which == 1) OK(tnml_optim_config(ctx, TNML_OPT_SGD, 0.9, 0.9, 0.999, 1e-8, 0));
    else OK(tnml_optim_config(ctx, TNML_OPT_ADAM, 0.0, 0.9, 0.999, 1e-3, 0));
    OK(tnml_gd_step(ctx, X.data(), lab.data(), b, 0.1f, 0.f, kAct, kLoss, 0.1f, met));
    OK(tnml_set_input(ctx, X.data(), lab.data(), b));
    OK(tnml_forward(ctx, f.data()));
    OK(tnml_bond_spectra(ctx, 1e-6, o.bond.data(), o.sigma.data(), &o.logn));
    OK(tnml_gd_step(ctx, X.data(), lab.data(), b, 0.1f, 0.f, kAct, kLoss, 0.1f, met));               // the state is still bound
    OK(tnml_forward(ctx, f.data()));
    OK(tnml_bond_spectra(ctx, 1e-6, o.bond.data(), o.sigma.data(), &o.logn));
    OK(tnml_sweep(ctx, 0, 2, 1, 1e-3f, 1e-3f, 1, kAct, kLoss, 0.1f, TNML_TRUNC_FIXED, nullptr, nullptr));   // spectra: no new forward needed
    set_cores(ctx, N, D, L, std::vector<int>(N - 1, 2), 0);
    OK(tnml_optim_reset(ctx));
    OK(tnml_gd_step(ctx, X.data(), lab.data(), b, 0.1f, 0.f, kAct, kLoss, 0.1f, met));
    OK(tnml_forward(ctx, f.data()));
    OK(tnml_orthogonalize(ctx, 1e-6, o.bond.data(), &o.logn));                                        // (the planned call keeps every bond)
    FAILS_WITH(TNML_ERR_STATE, tnml_sweep(ctx, 0, N - 1, 1, 1e-3f, 1e-3f, 1, kAct, kLoss, 0.1f, TNML_TRUNC_FIXED, nullptr, nullptr));
    FAILS_WITH(TNML_ERR_STATE, tnml_gd_step(ctx, X.data(), lab.data(), b, 0.1f, 0.f, kAct, kLoss, 0.1f, met));
    if (!strstr(tnml_last_error(), "tnml_optim_reset")) { fprintf(stderr, "the refusal does not name tnml_optim_reset: %s\n", tnml_last_error()); exit(1); }
    OK(tnml_optim_reset(ctx));
    OK(tnml_gd_step(ctx, X.data(), lab.data(), b, 0.1f, 0.f, kAct, kLoss, 0.1f, met));
    OK(tnml_compress(ctx, 2, 1.0, 1e-6, o.bond.data(), o.sigma.data(), o.disc.data(), &o.logn));
    FAILS_WITH(TNML_ERR_STATE, tnml_gd_step(ctx, X.data(), lab.data(), b, 0.1f, 0.f, kAct, kLoss, 0.1f, met));
    OK(tnml_optim_config(ctx, TNML_OPT_SGD, 0.0, 0.9, 0.999, 1e-8, 1));                               // plain SGD has no state
    OK(tnml_gd_step(ctx, X.data(), lab.data(), b, 0.1f, 0.f, kAct, kLoss, 0.1f, met));
    OK(tnml_orthogonalize(ctx, 1e-6, o.bond.data(), &o.logn));
    OK(tnml_gd_step(ctx, X.data(), lab.data(), b, 0.1f, 0.f, kAct, kLoss, 0.1f, met));
    OK(tnml_forward(ctx, f.data()));
    OK(tnml_sweep(ctx, 0, N - 1, 1, 1e-3f, 1e-3f, 1, kAct, kLoss, 0.1f, TNML_TRUNC_FIXED, nullptr, nullptr));
  }
  OK(tnml_destroy(ctx));
  printf("optimiser state rule after a committed call: ok\n");
}

// every allocation of the scratch group fails in turn; the group is created by the first call, whichever it is
static void run_alloc_failures(int D) {
  const int N = 6, L = 2, M = 6;
  for (int first = 0; first < 3; ++first) {
    tnml_ctx *ctx = nullptr;
    OK(tnml_create(&ctx, N, D, L, M, 64, 0));
    set_cores(ctx, N, D, L, std::vector<int>(N - 1, M), 3);
    Out o(N, M > D * 2 ? M : D * 2);
    int k;
    if (first == 0) k = fail_each_alloc("tnml_orthogonalize, fresh context", [&] { return tnml_orthogonalize(ctx, 1e-6, o.bond.data(), &o.logn); });
    else if (first == 1) k = fail_each_alloc("tnml_compress, fresh context", [&] { return tnml_compress(ctx, 2, 1.0, 1e-6, o.bond.data(), o.sigma.data(), o.disc.data(), &o.logn); });
    else k = fail_each_alloc("tnml_bond_spectra, fresh context", [&] { return tnml_bond_spectra(ctx, 1e-6, o.bond.data(), o.sigma.data(), &o.logn); });
    if (k != 12) { fprintf(stderr, "%d allocations failed in turn, the scratch group has 12\n", k); exit(1); }
    k = fail_each_alloc("tnml_compress, the group exists", [&] { return tnml_compress(ctx, 2, 1.0, 1e-6, o.bond.data(), o.sigma.data(), o.disc.data(), &o.logn); });
    if (k != 0) { fprintf(stderr, "%d allocations in a second call\n", k); exit(1); }
    OK(tnml_destroy(ctx));
  }
}

int main() {
  run_true_size("c3", 784, 2, 2, 20, 0);
  run_true_size("c5", 784, 2, 10, 50, 783);
  run_true_size("c5 inner label", 784, 2, 10, 50, 400);
  run_ragged(2, 3, 5);
  run_ragged(3, 3, 7);
  run_ragged(8, 17, 6);
  run_refusals();
  run_state_rule();
  run_alloc_failures(2);
  run_alloc_failures(3);
  san_stub_report();
  const char *paths[] = {"orth_load_kernel", "orth_chain_kernel", "orth_store_kernel"};
  for (const char *k : paths)
    if (san_stub_launches(k) < 1) { fprintf(stderr, "launch path %s was never taken\n", k); return 1; }
  printf("orthogonal form: %ld orth_chain_kernel launches checked, %d refusals\n", san_stub_launches("orth_chain_kernel"), g_refusals);
  printf("orthogonal-form host planning under ASan + UBSan: ok\n");
  return 0;
}
