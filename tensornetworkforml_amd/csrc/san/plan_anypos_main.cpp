// Label at an intermediate site (tnml_set_any_position) planned by the real host code of the library, built --cuda-host-only with
// AddressSanitizer and UBSan, against the stand-in runtime of hip_stub.cpp: forward, predict, predict_indices, eval_indices and
// segment starts at every position of a ragged chain and at C3 / C5 sizes, on the four step paths (single-launch step, classic
// sequence, large-tensor path, generic feature dimension), in both directions, with buffer growth in between.  The stand-in checks
// every pointer of the new launches (label_meet_kernel, the half-chains) together with the extent touched.
// `make san-anypos` builds and runs it; tests/test_any_position_host.py runs `make san-anypos`.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../../include/tnml.h"

extern "C" void san_stub_report(void);
extern "C" long san_stub_launches(const char *substr);

#define OK(call)                                                                              \
  do {                                                                                        \
    int rc_ = (call);                                                                         \
    if (rc_ != TNML_OK) { fprintf(stderr, "%s:%d %s -> %d: %s\n", __FILE__, __LINE__, #call, rc_, tnml_last_error()); exit(1); } \
  } while (0)
#define FAILS_WITH(code, call)                                                                \
  do {                                                                                        \
    int rc_ = (call);                                                                         \
    if (rc_ != (code)) { fprintf(stderr, "%s:%d %s -> %d, expected %d\n", __FILE__, __LINE__, #call, rc_, (code)); exit(1); } \
  } while (0)

static long g_segments = 0, g_forwards = 0;

// cores with the label axis on site l for the given bonds
static void set_cores_at(tnml_ctx *ctx, int N, int D, int L, const std::vector<int> &bond, int l) {
  size_t total = 0;
  for (int i = 0; i < N; ++i) total += (size_t)(i == 0 ? 1 : bond[i - 1]) * D * (i == N - 1 ? 1 : bond[i]) * (i == l ? L : 1);
  std::vector<float> cores(total);
  for (size_t e = 0; e < total; ++e) cores[e] = 0.1f + 1e-3f * (float)(e % 97);
  OK(tnml_set_cores(ctx, cores.data(), total, bond.data(), l));
}

#define SWEEP(ctx, left, n, first, pol) tnml_sweep(ctx, left, n, first, 1e-3f, 1e-3f, 1, TNML_ACT_SOFTMAX, TNML_LOSS_FULL_CROSS_ENT, 0.1f, pol, met.data(), f.data())

// mode: 0 single-launch step, 1 classic sequence, 2 large-tensor path (ignored at D != 2: the generic path)
static void run(const char *name, int N, int D, int L, int M, const std::vector<int> &bond, int b, int mode, int policy, bool every_position) {
  tnml_ctx *ctx = nullptr;
  OK(tnml_create(&ctx, N, D, L, M, b, 0));
  if (mode == 1) OK(tnml_set_step_pipeline(ctx, 0));
  if (mode == 2) OK(tnml_set_narrow_path(ctx, 1));
  const int nds = b + 70;
  std::vector<float> X((size_t)nds * N * D, 0.5f), f((size_t)L * nds), met((size_t)2 * N);
  std::vector<int> y(nds), idx(nds);
  for (int s = 0; s < nds; ++s) { y[s] = s % L; idx[s] = (s * 7) % nds; }
  OK(tnml_dataset_attach(ctx, X.data(), y.data(), nds, N, D, TNML_DATASET_FEATURES));
  std::vector<int> pos;
  if (every_position) for (int l = 0; l < N; ++l) pos.push_back(l);
  else pos = {1, N / 2, N - 2};
  double out3[3];
  for (int l : pos) {
    const bool inside = l != 0 && l != N - 1;
    set_cores_at(ctx, N, D, L, bond, l);
    OK(tnml_set_input(ctx, X.data(), y.data(), b));
    // switch off: the four calls refuse an intermediate position
    OK(tnml_set_any_position(ctx, 0));
    if (inside) {
      FAILS_WITH(TNML_ERR_STATE, tnml_forward(ctx, f.data()));
      FAILS_WITH(TNML_ERR_STATE, tnml_predict(ctx, X.data(), b, f.data()));
      FAILS_WITH(TNML_ERR_STATE, tnml_predict_indices(ctx, idx.data(), b, f.data()));
      FAILS_WITH(TNML_ERR_STATE, tnml_eval_indices(ctx, idx.data(), b, TNML_ACT_SOFTMAX, 0.1f, out3));
    }
    OK(tnml_set_any_position(ctx, 1));
    for (int left = 0; left < 2; ++left) {
      if (left ? l < 1 : l > N - 2) continue;
      set_cores_at(ctx, N, D, L, bond, l);
      // a batch of the context's capacity, then (second direction) a larger one: the batch buffers grow between two segments
      const int bb = left ? b + 37 : b;
      OK(tnml_select_indices(ctx, idx.data(), bb));
      if (inside) FAILS_WITH(TNML_ERR_STATE, SWEEP(ctx, left, 1, 0, policy));          // a new batch without a forward
      OK(tnml_forward(ctx, f.data()));
      ++g_forwards;
      OK(tnml_resident_metrics(ctx, TNML_ACT_SOFTMAX, 0.1f, out3));
      std::vector<float> env((size_t)(M > D * L ? M : D * L) * 2 * bb);
      int m = 0;
      if (l > 0) OK(tnml_get_env(ctx, TNML_SIDE_LEFT, l - 1, env.data(), env.size(), &m));
      if (l < N - 1) OK(tnml_get_env(ctx, TNML_SIDE_RIGHT, l + 1, env.data(), env.size(), &m));
      // predictions leave the resident batch alone; more samples than any buffer holds
      OK(tnml_predict(ctx, X.data(), bb / 2 + 3, f.data()));
      OK(tnml_predict_indices(ctx, idx.data(), bb + 5, f.data()));
      OK(tnml_eval_indices(ctx, idx.data(), nds, TNML_ACT_SOFTMAX, 0.1f, out3));
      if (inside) {
        FAILS_WITH(TNML_ERR_STATE, SWEEP(ctx, left, 1, 1, policy));                    // first_of_sweep stays ends-only
        // the standalone sub-steps after an intermediate forward
        const int p = left ? l - 1 : l;
        const size_t nB = (size_t)(p == 0 ? 1 : bond[p - 1]) * D * D * (p + 1 == N - 1 ? 1 : bond[p + 1]) * L;
        std::vector<double> Bn(nB), grad(nB);
        std::vector<float> B(nB, 0.01f);
        float met2[2];
        double loss = 0;
        OK(tnml_update_B(ctx, nullptr, left, 1e-3f, 1e-3f, 1, TNML_ACT_SOFTMAX, TNML_LOSS_FULL_CROSS_ENT, 0.1f, Bn.data(), nB, met2));
        OK(tnml_l2_term(ctx, B.data(), left, 1e-3f, &loss, grad.data(), nB));
      }
      // the segment: its first call, a continuation, and the refusal of the other direction
      const int room = left ? l : N - 1 - l;
      const int n1 = room >= 3 ? 2 : 1;
      OK(SWEEP(ctx, left, n1, inside ? 0 : 1, policy));
      ++g_segments;
      if (room > n1) OK(SWEEP(ctx, left, room - n1 > 2 ? 2 : 1, 0, policy));
      const int lp = tnml_l_pos(ctx);
      if (lp != 0 && lp != N - 1) FAILS_WITH(TNML_ERR_STATE, SWEEP(ctx, !left, 1, 0, policy));
      if (lp != 0 && lp != N - 1) {                                                    // a forward where the segment stopped, and on
        OK(tnml_forward(ctx, f.data()));
        ++g_forwards;
        OK(SWEEP(ctx, left, 1, 0, policy));
        ++g_segments;
      }
    }
  }
  // with a communicator the switch is refused
  if (D == 2) {
    OK(tnml_set_any_position(ctx, 0));
    unsigned char uid[128];
    setenv("TNML_FORCE_COMM", "1", 1);
    OK(tnml_comm_unique_id(uid));
    OK(tnml_comm_init(ctx, 0, 1, uid));
    FAILS_WITH(TNML_ERR_STATE, tnml_set_any_position(ctx, 1));
  }
  OK(tnml_destroy(ctx));
  printf("planned any-position %-26s D %d mode %d policy %d: ok\n", name, D, mode, policy);
  fflush(stdout);
}

int main() {
  const std::vector<int> ragged = {2, 4, 3, 4, 2};
  for (int mode = 0; mode < 3; ++mode) {
    run("ragged N 6 L 3", 6, 2, 3, 4, ragged, 70, mode, TNML_TRUNC_FIXED, true);
    run("ragged N 6 L 2", 6, 2, 2, 4, ragged, 5, mode, TNML_TRUNC_REFERENCE, true);
    run("N 8 bond 4 L 3", 8, 2, 3, 4, std::vector<int>(7, 4), 37, mode, TNML_TRUNC_ADAPTIVE, true);
  }
  run("D 3 N 5 bond 3", 5, 3, 3, 3, std::vector<int>(4, 3), 70, 0, TNML_TRUNC_FIXED, true);
  run("D 8 N 5 bond 2", 5, 8, 2, 2, std::vector<int>(4, 2), 20, 0, TNML_TRUNC_FIXED, true);
  run("bond 50 L 10 (chunked core)", 5, 2, 10, 50, std::vector<int>(4, 50), 70, 0, TNML_TRUNC_FIXED, true);
  // the BASELINE shapes at their true chain length
  run("c3 bond 20 b 5000", 784, 2, 2, 20, std::vector<int>(783, 20), 5000, 0, TNML_TRUNC_FIXED, false);
  run("c3 bond 20 b 5000", 784, 2, 2, 20, std::vector<int>(783, 20), 5000, 1, TNML_TRUNC_FIXED, false);
  run("c5 bond 50 L 10 b 5000", 784, 2, 10, 50, std::vector<int>(783, 50), 5000, 0, TNML_TRUNC_FIXED, false);
  san_stub_report();
  const char *paths[] = {"label_meet_kernel", "env_chain_roles_kernel", "env_chain_kernel", "anyd_chain_kernel", "step_pipe_kernel",
                         "narrow_step_kernel", "big_jacobi", "anyd_update_kernel"};
  for (const char *k : paths)
    if (san_stub_launches(k) < 1) { fprintf(stderr, "launch path %s was never taken\n", k); return 1; }
  printf("any-position: %ld forwards, %ld segment starts, %ld label_meet launches checked\n", g_forwards, g_segments, san_stub_launches("label_meet_kernel"));
  printf("any-position host planning under ASan + UBSan: ok\n");
  return 0;
}
