// Private to the host side of libtnml_hip.so (tnml_api.hip and the api_*.hip files): what more than one of them needs -- the error macros, the
// context with its buffer Owner, the state invalidators, and the helpers one call family lends another.
#pragma once
#include <rccl/rccl.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <initializer_list>
#include <memory>
#include <utility>

#include "tnml_internal.h"
#include "wide_pipe_device.h"      // PersistStep and kPipeGroupMax: the context holds the records of the persistent sweep

using namespace tnml;

// Nothing declared here is part of the C ABI: the library is loaded into processes that hold other libraries, and a visible
// symbol called `fail` or `make_group` could be interposed.
#pragma GCC visibility push(hidden)

namespace tnml {
int fail(int code, const char *fmt, ...);      // defined beside tnml_last_error, whose message it sets for the thread
}

#define HIP_TRY(expr)                                                                          \
  do {                                                                                         \
    hipError_t e_ = (expr);                                                                    \
    if (e_ != hipSuccess) return fail(TNML_ERR_HIP, "%s failed: %s (%s:%d)", #expr,           \
                                      hipGetErrorString(e_), __FILE__, __LINE__);              \
  } while (0)

#define NCCL_TRY(expr)                                                                         \
  do {                                                                                         \
    ncclResult_t r_ = (expr);                                                                  \
    if (r_ != ncclSuccess) return fail(TNML_ERR_COMM, "%s failed: %s (%s:%d)", #expr,         \
                                       ncclGetErrorString(r_), __FILE__, __LINE__);            \
  } while (0)

static constexpr size_t kLdsMax = 160 * 1024;      // LDS of a workgroup on gfx950: what a launch may ask for

// What one tnml_sweep call fixes for all its steps: the arguments of the call (mode 1: standalone update_B, Bdirect_dev: merged tensor
// to use instead of the product of the two cores), whether it starts a segment, its sample tiles, its closing timing event.
struct SweepCall {
  int left_dir, n_steps;
  float lr, weight_dec;
  int l2_flag, act_fn, loss_fn;
  float T;
  int trunc_policy;
  float *metrics_out, *f_out;
  int mode;
  const float *Bdirect_dev;
  hipEvent_t sw_ev1;
  bool seg_start;
  int nblk;
};

// A reduced pre-gradient left in zred for the next step: the step (relative index k) of a sweep call with these arguments may start
// from it.  rows / cols: its shape as a matrix, where the taker checks it (large-tensor pipeline).
struct ZTicket {
  bool valid = false;
  int k = -1, left = 0, act = 0, loss = 0, rows = 0, cols = 0;
  float T = 0.f;
  bool matches(const SweepCall &s, int k_) const {
    return valid && k == k_ && left == s.left_dir && act == s.act_fn && loss == s.loss_fn && T == s.T;
  }
  void leave(const SweepCall &s, int k_, bool valid_, int rows_ = 0, int cols_ = 0) {
    valid = valid_; k = k_; left = s.left_dir; act = s.act_fn; loss = s.loss_fn; T = s.T; rows = rows_; cols = cols_;
  }
};

// Who owns what ("Who owns what").  Everything a context creates in the runtime -- device memory, pinned host memory,
// events, streams -- is created by Owner::make and recorded there; the members of tnml_ctx stay the raw handles the argument blocks
// of the kernels copy by value.  ~Owner releases what is still recorded, newest first, so `delete ctx` is the whole teardown and a
// tnml_create that fails half-way leaks nothing.  No other host code calls the runtime's create / destroy functions.
//
// Capacity groups.  Buffers sized from the same quantity are (re)sized by ONE function, which writes each member's size once and
// hands the list to make().  make() frees every member first and creates them afterwards (the batch group's two environment stacks
// are ~0.8 GB each at C5: old and new together would double the peak), and frees them all again when one creation fails.  The rule
// for every group: after a failed (re)size the group is completely empty, its capacity field is 0 and every flag that depends on it
// (have_input, have_labels, envs_valid_*, f_current, big_ready, ...) is cleared -- the group's function does that BEFORE it calls
// make(); the call returns TNML_ERR_HIP; the same call repeated later succeeds; and no call in between launches with a null or
// undersized member, because every reader goes through that capacity field or one of those flags.
struct Owner {
  enum Kind { kDev, kPinned, kEvent, kStream };
  struct Member { void **slot; size_t arg; Kind kind; bool wanted = true; };   // arg: bytes (memory) or creation flags (event); !wanted: released, not created
  std::vector<std::pair<void *, Kind>> held;                   // by value: the slots may be locals or move (sweep_ev)

  Owner() = default;
  Owner(const Owner &) = delete;
  Owner &operator=(const Owner &) = delete;
  ~Owner() { for (; !held.empty(); held.pop_back()) destroy(held.back().first, held.back().second); }

  static void destroy(void *h, Kind k) {
    switch (k) {
      case kDev: (void)hipFree(h); break;
      case kPinned: (void)hipHostFree(h); break;
      case kEvent: (void)hipEventDestroy((hipEvent_t)h); break;
      case kStream: (void)hipStreamDestroy((hipStream_t)h); break;
    }
  }
  template <class T> void release(T *&p) {                     // free, un-record, null
    for (size_t i = held.size(); p && i-- > 0;)
      if (held[i].first == (void *)p) { destroy(held[i].first, held[i].second); held.erase(held.begin() + i); break; }
    p = nullptr;
  }
  // all of the list or none of it: whatever the slots hold is released first
  hipError_t make(std::initializer_list<Member> group) {
    for (const Member &m : group) release(*m.slot);
    for (const Member &m : group) {
      if (!m.wanted) continue;
      void *h = nullptr;
      hipError_t e = hipSuccess;
      switch (m.kind) {
        case kDev: e = hipMalloc(&h, m.arg); break;
        case kPinned: e = hipHostMalloc(&h, m.arg); break;
        case kEvent: e = hipEventCreateWithFlags((hipEvent_t *)&h, (unsigned)m.arg); break;
        case kStream: e = hipStreamCreateWithFlags((hipStream_t *)&h, hipStreamNonBlocking); break;
      }
      if (e != hipSuccess) {
        for (const Member &u : group) release(*u.slot);
        return e;
      }
      held.emplace_back(h, m.kind);
      *m.slot = h;
    }
    return hipSuccess;
  }
};
template <class T> inline Owner::Member own_dev(T *&p, size_t count) { return {(void **)&p, count * sizeof(T), Owner::kDev}; }
template <class T> inline Owner::Member own_dev_if(bool wanted, T *&p, size_t count) { return {(void **)&p, count * sizeof(T), Owner::kDev, wanted}; }
template <class T> inline Owner::Member own_pinned(T *&p, size_t count) { return {(void **)&p, count * sizeof(T), Owner::kPinned}; }
inline Owner::Member own_event(hipEvent_t &e, unsigned flags) { return {(void **)&e, flags, Owner::kEvent}; }
inline Owner::Member own_stream(hipStream_t &s) { return {(void **)&s, 0, Owner::kStream}; }

struct tnml_ctx {
  Owner own;                            // (first member: destroyed last)
  int N = 0, D = 0, L = 0, Mmax = 0;   // Mmax = buffer capacity per bond
  int Mpol = 0;                         // the M of Network(N, M, ...): fixed-policy rank
  int b = 0, b_pad = 0, b_cap = 0;
  int device = 0;
  hipStream_t stream = nullptr;
  hipStream_t stream2 = nullptr;             // large-tensor steps: merged tensor and Nh^T.B beside the batch kernel; persistent sweep: helper grid
  hipStream_t stream3 = nullptr;             // persistent sweep in three launches: batch-side grid
  hipEvent_t ev_p0 = nullptr, ev_p2 = nullptr, ev_p3 = nullptr;
  int persist_mode = 1;                      // tnml_set_persistent: 0 per-step launches, 1 one kernel per sweep (default), 2 one kernel per role
  hipEvent_t ev_main = nullptr, ev_prep = nullptr;
  // communicator path of the pipelined step: update side on `stream`, batch side + all-reduce of the pre-gradient on `stream2`
  struct {
    // (ev_upd[i]: an update launch has ended; ev_bat[i]: a batch-side launch and the exchange behind it have ended)
    hipEvent_t ev_upd[2] = {nullptr, nullptr}, ev_bat[2] = {nullptr, nullptr};
    int upd = 0, bat = 0;                    // index of the event recorded last
    bool pending = false;                    // stream2 holds batch-side work `stream` has not waited for yet
    bool enabled = true;                     // tnml_set_comm_overlap
    // hand-offs without events, as in the large-tensor pipeline below: [0] "Z (all-reduced) is ready", [1] "update launch done"
    unsigned *flags = nullptr;
    unsigned zseq = 0, dseq = 0;
    bool flags_enabled = true, done_valid = false, zsig_valid = false;
  } split;
  // pipelined large-tensor step (kernels_big.hip): the batch kernel of step k+1 runs on stream2 beside the SVD of step k and leaves
  // the reduced pre-gradient Z_{k+1} in zred; the step then starts with the contraction A_k^T . Z instead of the batch kernel
  struct {
    bool enabled = true;                     // tnml_set_step_pipeline(ctx, 0) turns it off together with the in-LDS pipeline
    ZTicket Z;
    float *Pk = nullptr;                     // [D * Mmax][b_pad]  E_k (x) x_k, the row operand of Z_{k+1}
    hipEvent_t ev_upd = nullptr, ev_z = nullptr;
    bool pending = false;                    // stream2 holds batch work of the pipelined large-tensor step the context's stream has not joined
    // hand-offs of that pipeline without events (kernels_big.hip, big_signal_kernel): [0] "Z of the next step is ready" (side stream ->
    // context's stream), [1] "B_new is ready" (context's stream -> side stream); sequence numbers
    unsigned *flags = nullptr;
    unsigned zsig_seq = 0, bsig_seq = 0;
    bool flags_enabled = true;
    bool ext_on_side = false;                // the last environment extension of the pipeline ran on the side stream
  } bigpipe;
  hipEvent_t ev0 = nullptr, ev1 = nullptr, pev0 = nullptr, pev1 = nullptr;
  // host bookkeeping
  std::vector<int> bond;
  int l_pos = 0;
  bool cores_set = false;
  bool have_input = false, have_labels = false;
  bool envs_valid_L = false, envs_valid_R = false;  // forward built the stack this side
  bool Ln_valid = false, Rn_valid = false;
  bool f_current = false;     // ctx->f holds the f the next step must start from
  bool Bnew_valid = false;    // ctx->Bnew holds the updated B of the previous step
  int prev_h = 0, prev_g = 0; // dims of Bnew (relative frame)
  int prev_left_dir = 0;
  int last_bsize = 0, last_n = 0, last_h = 0, last_g = 0, last_left_dir = 0;
  bool debug = false, profile = false, stamps = false;
  bool check_launches = false;               // tnml_debug_enable bit 2: read the launch status back after every kernel launch
  int sync_interval = 256;                   // tnml_set_sync_interval: drain the stream every so many steps (0 = never)
  double svd_stop2 = kSvdStop2Default;
  double chol_thr = kCholThrDefault;         // off(G) / trace(G) above which the pivoted-Cholesky step runs (0 disables it)
  double trunc_thr = 0.999;                  // adaptive truncation threshold (tensor_svd's default argument)
  double prof_ms[4] = {0, 0, 0, 0};
  long long prof_n[4] = {0, 0, 0, 0};
  // whole-sweep timing without any synchronisation inside the timed region (tnml_profile_enable(ctx, 2)): one event pair per
  // tnml_sweep call, read back by tnml_profile_get(which = 4)
  bool sweep_timing = false;
  std::vector<hipEvent_t> sweep_ev;          // pairs
  size_t sweep_ev_used = 0;
  double sweep_ms = 0;
  long long sweep_launches = 0, step_launches = 0;
  // tnml_get_counters: work since the last tnml_profile_reset, from the dimensions of every step actually run
  double cnt_steps = 0, cnt_bytes = 0, cnt_flops = 0, cnt_fwd_bytes = 0, cnt_fwd = 0;
  // staged batches (tnml_stage_batch / tnml_select_batch): device-resident [b][N][D] inputs + labels
  static constexpr int kStageSlots = 8;
  float *stageX[kStageSlots] = {nullptr};
  int *stageY[kStageSlots] = {nullptr};
  int stageB[kStageSlots] = {0};
  // device buffers
  size_t core_stride = 0, lab_elems = 0, bmax = 0;
  float *X = nullptr, *Xstage = nullptr;
  int *y = nullptr;
  float *f = nullptr, *ftmp = nullptr, *ftmp2 = nullptr;
  float *Lenv = nullptr, *Renv = nullptr;
  float *cores = nullptr, *lab[2] = {nullptr, nullptr};
  int lab_cur = 0;
  double *Ln = nullptr, *Rn = nullptr;
  float *Bnew = nullptr, *slabs = nullptr, *red = nullptr, *metrics = nullptr, *scal = nullptr;
  float *Bscr = nullptr, *Bscr2 = nullptr;   // scratch merged tensors of the standalone entry points
  BigScratch big{};                          // HBM scratch of the large-tensor path, allocated on first use
  bool big_ready = false;
  bool force_big = false;                    // tnml_set_narrow_path
  bool chain_plain = false;                  // tnml_set_chain_path
  bool any_pos = false;                      // tnml_set_any_position
  bool seg_starting = false;                 // the sweep call in flight starts a segment and has not planned its first step yet
  float *predEnv = nullptr;                  // prediction at an intermediate label site: [2][Mmax][pred_cap], the two environments next to it
  float *prepB = nullptr;                    // fused narrow launch: merged tensor / L2 term from the helper workgroups
  double *prepG = nullptr;
  unsigned *sync = nullptr;
  // pipelined step (wide_pipe_device.h): partial / group / reduced pre-gradients, arrival counters, B_new flag
  float *zslabs = nullptr, *gslabs = nullptr, *zred = nullptr;
  int zstride = 0;
  struct {
    bool enabled = true;                     // tnml_set_step_pipeline
    int tiles = 2;                           // sample tiles per batch-side workgroup where the SVD is long enough to hide them
    unsigned *cnt = nullptr;                 // [0..15] group counters, [16] top counter, [17] flag
    int nwide = 0, tpw = 1, ngroups = 0;
    ZTicket Z;                               // zred holds the pre-gradient of relative step Z.k of a sweep in direction Z.left
    unsigned token = 0;
  } pipe;
  // persistent sweep (sweep_persist_kernel): per-step records (device + two pinned host staging buffers), second buffers of the
  // reduced pre-gradient, T_k buffers, per-step arrival counters, the flag words of the launch
  bool persist_enabled = true;               // tnml_set_persistent
  bool shape_kernels = true;                 // tnml_set_shape_kernels: persistent sweeps may run the bodies compiled for a step shape
  int fixed_steps = 0;                       // steps of the last persistent sweep that did (tnml_fixed_shape_steps)
  bool persist_slices = true;                // tnml_set_persist_reduce: pre-gradients beyond one level are reduced in slices by many workgroups
  int slice_steps = 0;                       // records of the last persistent sweep that were (tnml_slice_reduce_steps)
  PersistStep *pst_dev = nullptr, *pst_host[2] = {nullptr, nullptr};
  hipEvent_t pst_ev[2] = {nullptr, nullptr};
  int pst_cur = 0;
  float *zred2 = nullptr, *prepRaw = nullptr;
  double *Tbuf[2] = {nullptr, nullptr}, *TNbuf[2] = {nullptr, nullptr}, *Apub = nullptr;
  unsigned *pst_cnt = nullptr, *pst_flags = nullptr;
  long long persist_sweeps = 0;
  int num_cus = 256;
  float *Xpred_stage = nullptr, *Xpred = nullptr, *fpred = nullptr;   // tnml_predict's own batch (the resident one is untouched)
  int pred_cap = 0;
  // range-safe chains (tnml_set_chain_scaling).  Members of the prediction group once a scaled prediction has
  // been asked for: mantissas [L][pred_cap], exponents [pred_cap], the bond table [N] of scaled_pred_kernel.  The exponent stacks
  // [N][cap] of pass A are members of the two gradient groups while the switch is on.
  bool scaled = false;
  float *pred_mant = nullptr;
  int *pred_expo = nullptr, *pred_bond = nullptr, *ig_estack = nullptr, *cg_estack = nullptr;
  int slab_stride = 0, nblk_cap = 0, metrics_cap = 0;
  double *dbg = nullptr;
  size_t dbg_elems = 0;
  int *status = nullptr;
  unsigned long long *counters = nullptr;
  char *tables = nullptr;      // device scratch for ChainSite / NormChainSite tables
  size_t tables_bytes = 0;
  double *anyd_W = nullptr, *anyd_T2 = nullptr;   // generic-D update kernel: Jacobi vectors beyond LDS, behind core + its norm product
  // device-resident dataset (tnml_dataset_attach): features [n][N][D] or pixels [n][N], labels [n]; the index list of the call in
  // flight lives in ds_idx (device), filled through one of two pinned host buffers so that the caller's list is free on return
  float *ds_data = nullptr;
  int *ds_labels = nullptr;
  int ds_n = 0, ds_form = 0;
  double ds_coef[kMaxD] = {0};
  int *ds_idx = nullptr, *ds_idx_host[2] = {nullptr, nullptr};
  hipEvent_t ds_idx_ev[2] = {nullptr, nullptr};
  bool ds_idx_busy[2] = {false, false};
  int ds_idx_cap = 0, ds_idx_cur = 0;
  int *ds_ypred = nullptr;                   // [pred_cap] labels of the chunk tnml_eval_indices is evaluating, beside Xpred / fpred
  double *ds_part = nullptr, *ds_acc = nullptr;   // block partials and the four accumulators of the metrics kernels
  int ds_part_cap = 0;
  // input gradients (tnml_input_grad): one group sized from ig_cap samples -- the stack of pass A
  // [N][Mmax][ig_cap], cot [L][ig_cap], g [ig_cap][N][D], its pixel form [ig_cap][N], cf [ig_cap] -- and the bond table [N]
  float *ig_stack = nullptr, *ig_cot = nullptr, *ig_g = nullptr, *ig_gpix = nullptr, *ig_cf = nullptr;
  int *ig_bond = nullptr;
  int ig_cap = 0, ig_chunk = 0;              // ig_chunk: tnml_set_input_grad_chunk (0 = default)
  // core gradients (tnml_core_grad): one group sized from cg_cap samples -- the stacks of both passes
  // [N][Mmax][cg_cap], cot [L][cg_cap], cf [cg_cap] -- with the table [2N] (bonds, then every core's offset in the flat layout) and
  // G, the gradient in the layout of tnml_get_cores, sized for every bond at its capacity
  float *cg_stackP = nullptr, *cg_stackQ = nullptr, *cg_cot = nullptr, *cg_cf = nullptr, *cg_G = nullptr;
  int *cg_tab = nullptr;
  int cg_cap = 0, cg_chunk = 0;              // cg_chunk: tnml_set_core_grad_chunk (0 = default)
  // gradient training (tnml_gd_train_indices).  State group: opt_s0 / opt_s1 (SGD vel / Adam m, v) in the
  // layout and of the size of cg_G, created by the first step of a stateful optimiser and bound to that step's bonds and l_pos.
  // Metrics group: [opt_met_cap][4] doubles, one row per step of the call in flight.
  struct {
    int kind = TNML_OPT_SGD, clip = 1;
    double momentum = 0.0, beta1 = 0.9, beta2 = 0.999, eps = 1e-8;
    long long t = 0;                         // Adam steps taken since the last reset
    std::vector<int> bond;                   // what the state is bound to (meaningful while opt_s0 exists)
    int l_pos = -1;
  } opt;
  float *opt_s0 = nullptr, *opt_s1 = nullptr;
  double *opt_met = nullptr;
  int opt_met_cap = 0;
  std::vector<int> opt_tab;                  // host copy of cg_tab for the call in flight (outlives the asynchronous upload)
  // orthogonal form / compression / bond spectra.  One group, created by the first call: the float64 work copy
  // of the slots and the label buffer, the absorbed site, the carried factors, the float32 result the commit copies from, the
  // operation list, the scratch bond table and the outputs of the call.
  struct {
    double *W = nullptr, *Mbuf = nullptr, *aux = nullptr, *sigma = nullptr, *disc = nullptr, *result = nullptr;
    float *out_cores = nullptr, *out_lab = nullptr;
    OrthOp *ops = nullptr;
    int *bond = nullptr, *rank = nullptr, *status = nullptr;
    bool ready = false;
  } orth;
  // inner products and linear combinations.  One group, sized from the second chain: its cores (flat layout,
  // v_cap floats), the bond and offset tables of both chains, the metric, the staging areas and half results of the six workgroups
  // (sized from m_cap, the largest bond of either chain), the six outputs, the float32 result tnml_axpby commits from, the status.
  struct {
    float *V = nullptr, *out_cores = nullptr, *out_lab = nullptr;
    int *bond = nullptr, *half_expo = nullptr, *status = nullptr;
    long long *off = nullptr;
    double *metric = nullptr, *stage = nullptr, *half_E = nullptr, *out = nullptr;
    size_t v_cap = 0;
    int m_cap = 0;
    std::vector<int> bond_host;              // host copies of the two tables for the call in flight (they outlive the asynchronous upload)
    std::vector<long long> off_host;
  } alg;
  // samples and log-likelihoods.  One group, regrown when a call needs more of any member: the tables of the
  // call (bonds, slots, tiles, classes, given levels), the grid and its metric, the uniforms (u_cap doubles, 1 when they are hashed),
  // the environment stacks (shared part and env_slots per-slot parts of lpos_cap sites each, env_stride doubles a site), the
  // staging areas of the environment workgroups, the outputs and the status words.
  struct {
    int *bond = nullptr, *slot_class = nullptr, *tile_slot = nullptr, *tile_samples = nullptr, *classes = nullptr, *given = nullptr;
    int *levels = nullptr, *labels = nullptr, *status = nullptr;
    double *S = nullptr, *phi = nullptr, *w = nullptr, *u = nullptr, *env_shared = nullptr, *env_slots = nullptr, *stage = nullptr, *logp = nullptr;
    size_t n_cap = 0, given_cap = 0, u_cap = 0, tiles_cap = 0, slots_cap = 0, slot_sites_cap = 0;
    int m_cap = 0;
    std::vector<int> host;                   // host copies of the tables for the call in flight (they outlive the asynchronous upload)
    std::vector<double> hostd;
  } smp;
  // the same given any set of known pixels.  One group of its own, regrown when a call needs more of any
  // member: the tables of the call (bonds, tiles, rows, mask, known levels), the grid and its metric, the uniforms, the per-row
  // environment stack of one chunk (stack_cap doubles, at most stack_bytes), E per row, the outputs and the status words.
  struct {
    int *bond = nullptr, *tile_class = nullptr, *tile_rows = nullptr, *known = nullptr, *levels = nullptr, *labels = nullptr, *status = nullptr;
    unsigned char *mask = nullptr;
    double *S = nullptr, *phi = nullptr, *w = nullptr, *u = nullptr, *stack = nullptr, *E = nullptr, *logp0 = nullptr;
    size_t tiles_cap = 0, rows_cap = 0, n_cap = 0, mask_cap = 0, u_cap = 0, stack_cap = 0;
    size_t stack_bytes = (size_t)1 << 30;    // tnml_set_sample_stack_bytes
    std::vector<int> host;                   // host copies of the tables for the call in flight (they outlive the asynchronous upload)
    std::vector<double> hostd, hostE, hostp;
  } smk;
  // the gradient of the log-norm.  One group, sized from m_cap, the largest bond of a call: the table of
  // grad_table, the metric, both environment stacks with their exponents, the gradient (of cg_G's size), the two outputs, the status.
  struct {
    int *tab = nullptr, *expL = nullptr, *expR = nullptr, *status = nullptr;
    double *metric = nullptr, *envL = nullptr, *envR = nullptr, *out = nullptr;
    float *G = nullptr;
    int m_cap = 0;
    std::vector<int> tab_host;               // host copy of the table for the call in flight (it outlives the asynchronous upload)
  } lnz;
  // the likelihood of a batch: per-sample terms and flags of the call in flight, and their two sums
  struct {
    double *terms = nullptr, *acc = nullptr;
    int *bad = nullptr;
    int n_cap = 0;
  } nll;
  // likelihood training.  One group, created by the first step and regrown with the steps of a call: the
  // per-step records [cap][4], the sticky skip word of the guard, and the two events that carry the norm walk to stream2 and back.
  struct {
    double *rec = nullptr;
    int *skip = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    int cap = 0;
    int overlap = 0;                         // tnml_set_nll_overlap: the norm walk on stream2 beside the chunks of the step
    std::vector<double> metric_host;         // host copy of the metric for the call in flight (it outlives the asynchronous upload)
  } nst;
  // per-pixel conditionals.  One group of its own, regrown when a call needs more of any member: the values
  // of the levels, the left environments behind the site a row of one chunk is on (lf_cap doubles), and the three outputs of n_cap
  // samples.  The tables, the grid, the stack and E are the masked group's (smk), through smk_ensure.
  struct {
    double *values = nullptr, *lf_next = nullptr, *q = nullptr, *stats = nullptr;
    int *mode = nullptr;
    size_t n_cap = 0, lf_cap = 0;
    std::vector<double> values_host;         // host copy of the values for the call in flight (it outlives the asynchronous upload)
  } scc;
  // pixel-pair marginals.  One group of its own, regrown when a bond or a chunk outgrows it: the table of
  // grad_table, the grid with its metric and values, both environment stacks of the call's class slot with their exponents, B_j
  // of every site, the per-site outputs, and for rows_cap rows of one chunk the sites, Q, its exponents and the pair statistics.
  struct {
    int *tab = nullptr, *expL = nullptr, *expR = nullptr, *status = nullptr, *rows = nullptr, *qexp = nullptr;
    double *S = nullptr, *phi = nullptr, *w = nullptr, *values = nullptr, *envL = nullptr, *envR = nullptr, *out = nullptr;
    double *B = nullptr, *q1 = nullptr, *stats1 = nullptr, *Q = nullptr, *stats = nullptr;
    int m_cap = 0;
    size_t rows_cap = 0;
    std::vector<int> tab_host, rows_host, sites_host;   // host copies for the call in flight (they outlive the asynchronous uploads)
    std::vector<double> hostd;               // S, the values, phi, w
  } pair;
  // two-site likelihood sweep.  One group of its own, regrown when a call needs more samples, a larger bond
  // or more steps: the ahead stack [N][m_cap][b_cap] and the behind pair of the per-sample chains, the partial and reduced data
  // gradient, the merged tensor (float64, float32, and what the split receives), the update's scratch and capture block, the
  // records, the site tables, the metric and the sticky guard word.
  struct {
    float *stack = nullptr, *behind[2] = {nullptr, nullptr}, *slabs = nullptr, *Gd = nullptr, *B32 = nullptr, *Bout = nullptr;
    double *B64 = nullptr, *T1 = nullptr, *T2 = nullptr, *dbg = nullptr, *rec = nullptr, *metric = nullptr, *sigma = nullptr;
    NllSweepSite *sites = nullptr;
    int *skip = nullptr;
    int b_cap = 0, m_cap = 0, steps_cap = 0;
    int last_h = 0, last_g = 0, last_nn = 0, last_left = 0;   // the last step of the last call (tnml_nll_sweep_debug); 0: none
    std::vector<NllSweepSite> sites_host;    // host copies for the call in flight (they outlive the asynchronous uploads)
    std::vector<double> metric_host;
  } nsw;
  // likelihood gradients from incomplete data.  One group of its own, regrown when a call needs more of any
  // member: the table of grad_table, the weight of every row of the call, the left environments behind the site a row of one chunk is
  // on (lf_cap doubles), the partial gradients of one chunk's tiles (part_cap doubles), the float64 accumulator and the float32
  // gradient (total_cap each), the status word.  The tables, the grid, the stack and E are the masked group's (smk), through smk_ensure.
  struct {
    int *tab = nullptr, *status = nullptr;
    double *wrow = nullptr, *lf_next = nullptr, *part = nullptr, *acc = nullptr;
    float *G = nullptr;
    size_t rows_cap = 0, lf_cap = 0, part_cap = 0, total_cap = 0;
    std::vector<int> tab_host;               // host copies for the call in flight (they outlive the asynchronous uploads)
    std::vector<double> wrow_host;
  } nmg;
  // multi-GPU
  ncclComm_t comm = nullptr;
  int rank = 0, nranks = 1;

  int ml(int i) const { return i == 0 ? 1 : bond[i - 1]; }
  int mr(int i) const { return i == N - 1 ? 1 : bond[i]; }
  float *env_slot(float *base, int site) const { return base + (size_t)site * Mmax * b_pad; }
  long long env_off(int site) const { return (long long)site * Mmax * b_pad; }
  float *core_slot(int site) const { return cores + (size_t)site * core_stride; }
  double *norm_slot(double *base, int site) const { return base + (size_t)site * Mmax * Mmax; }
};

// no step may start from a pre-gradient left earlier (cores, batch, labels or the launch form changed)
inline void drop_pregradients(tnml_ctx *c) { c->pipe.Z.valid = false; c->bigpipe.Z.valid = false; }

// The resident batch changed (tnml_set_input, tnml_select_batch, tnml_select_indices, a regrown batch group): what was computed from
// its samples is gone -- the environment stacks, f, the updated merged tensor of a previous step, the pre-gradients.  The norm
// environments (Ln_valid / Rn_valid) are contractions of the cores alone and stay, as does the optimiser binding.  tnml_set_labels
// drops the pre-gradients only: the stacks and f do not see the labels.
inline void batch_changed(tnml_ctx *c) {
  c->envs_valid_L = c->envs_valid_R = false;
  c->f_current = false;
  c->Bnew_valid = false;
  drop_pregradients(c);
}

// The model changed (tnml_set_cores, tnml_scale_cores, a training step, a committed orthogonalisation / compression / sum): nothing
// computed from the cores is current any more.  The ONE place that says which state hangs on the cores:
//   envs_valid_L/R, f_current   the environment stacks and f of the resident batch are products of the old cores
//   Ln_valid / Rn_valid         the norm environments of the L2 term are contractions of the old cores
//   Bnew_valid                  the updated merged tensor of a previous step belongs to the old chain: no mid-sweep continuation
//   the pre-gradient tickets    a pre-gradient a step left for its successor was formed with the old cores' environments
// What does NOT hang on the cores stays: the resident batch and its labels, the staged batches, the dataset, every capacity group.
inline void cores_changed(tnml_ctx *c) {
  c->envs_valid_L = c->envs_valid_R = false;
  c->Ln_valid = c->Rn_valid = false;
  c->f_current = false;
  c->Bnew_valid = false;
  drop_pregradients(c);
}

// vel / m / v describe the cores element by element: a commit that changes the gauge, the bonds or the meaning of an element leaves
// them unbound (tnml_gd_step / tnml_nll_step refuse until tnml_optim_reset).  tnml_set_cores and a sweep need no call: the binding is
// the pair (bonds, l_pos), which the step compares.
inline void unbind_optimiser(tnml_ctx *c) {
  if (c->opt_s0) c->opt.l_pos = -1;
}

// Helpers defined in one host file and called from another (a helper of one file alone is static there)
namespace tnml {
// groups and cores
int make_group(tnml_ctx *c, const char *what, std::initializer_list<Owner::Member> group);
int size_batch_group(tnml_ctx *c, int b_cap);
size_t core_elems(const tnml_ctx *c, const std::vector<int> &bond, int i, int l_pos);
// the prediction group and its chain: every chunked call runs on them
int pred_ensure_buffers(tnml_ctx *c, int bp, bool scaled_out = false);
int pred_allowed(tnml_ctx *c);
int pred_table(tnml_ctx *c, bool scaled = false);
int pred_chain(tnml_ctx *c, int b);
// the dataset's index lists and metrics, and the chunk loader
int ds_usable(tnml_ctx *c);
int ds_upload_indices(tnml_ctx *c, const int32_t *idx, int b);
int ds_ensure_metrics(tnml_ctx *c, int b_pad);
int load_chunk(tnml_ctx *c, const float *X, const int *idx_dev, const int32_t *y, int off, int bc, int *y_out);
// what the two-site likelihood sweep (nll_sweep_host.hip) borrows: the sticky status word, the table of the gradient calls, the norm
// term's checks, group, upload and environment launch, the per-sample terms, and the launch wrappers of the update / SVD kernels
int check_status(tnml_ctx *c);
int grad_table(const tnml_ctx *c, const char *what, std::vector<int> &tab, size_t &total, int &mb);
int lnz_check(const tnml_ctx *c, const char *what, const double *S, int n_metric, int mb);
int lnz_ensure(tnml_ctx *c, int mb, bool want_G);
int lnz_upload(tnml_ctx *c, const std::vector<int> &tab_host, const double *S, int n_metric, bool wait);
int lnz_launch_env(tnml_ctx *c, int n_metric, int mb, hipStream_t st);
int nll_ensure(tnml_ctx *c, int n);
// what the masked likelihood gradient (nll_masked_host.hip) borrows: the refusals and tables of the samplers' front, the masked
// group, and the state rules of the optimiser
int largest_bond(const tnml_ctx *c);
int smp_check_sizes(const char *what, const double *phi, const double *w, int n, int K);
int smp_check_grid(const char *what, int K, int D, const double *phi, const double *w);
int smp_check_classes(const char *what, const int32_t *classes, int n, int L);
int smp_check_state(const tnml_ctx *c, const char *what);
void smp_bond_table(const tnml_ctx *c, std::vector<int> &host);
void smp_grid_metric(std::vector<double> &S, int K, int D, const double *phi, const double *w);
int smk_ensure(tnml_ctx *c, size_t tiles, size_t rows, size_t n, size_t mask, size_t u, size_t stack);
bool opt_stateful(const tnml_ctx *c);
int opt_ensure_state(tnml_ctx *c);
int narrow_path(const tnml_ctx *c, int h, int g, int s, int L, int m);
int run_narrow(tnml_ctx *c, NarrowParams &n, int path, bool skip_prep = false, hipEvent_t after_update = nullptr,
               const BigFront *front = nullptr, unsigned *sig_flag = nullptr, unsigned sig_val = 0);
}  // namespace tnml

#pragma GCC visibility pop
