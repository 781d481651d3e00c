// Internal declarations shared by the translation units of libtnml_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/tnml.h"

namespace tnml {

constexpr int kD = 2;           // feature dimension the kernels are specialised for (kernels_anyd.hip: 3 <= D <= kMaxD)
constexpr int kMaxD = 8;
constexpr int kTS = 32;         // samples per workgroup in the wide step kernel (v1)
constexpr int kWideThreads = 1024; // 4 waves per SIMD: the v1 formulation is latency-bound
constexpr int kNarrowThreads = 1024;
constexpr int kMetricSlots = 4;    // per-slab tail: correct count, sum|y-fa|, non-finite count, pad
constexpr int kDbgScalars = 120 + 16 * 12;   // 5 scalars + 115 stamps + (experiment builds) 12 probe points x 16 waves
constexpr int kDbgSigma = 128;     // capture block: 4 tensors, then this many singular values, then scalars
constexpr double kCholThrSmall = 0.35;     // the same for matrices with n < 32
constexpr double kCholThrDefault = 0.22;   // off(G)/trace(G) above which the Cholesky step pays off (kernels_narrow.hip phase 6b)
constexpr double kSvdStop2Default = 1e-6;   // see jacobi_rot (jacobi_device.h) and tnml_set_svd_stop
constexpr int kCounterSlots = 16;   // device counters: [0..3] Jacobi statistics, [4..7] fused-launch timing diagnostics, [8..] spare

// A plain (label-free) core or the label core addressed in the sweep-relative frame.
//   plain:  A(in, d, out)      = base[in*s_in + d*s_d + out*s_out]
//   label:  A(h, d, s, l)      = base[h*s_in + d*s_d + s*s_out + l]   (label stride is 1)
struct CoreView {
  const float *base;
  int n_in, n_out;
  int s_in, s_d, s_out;
};

// One site of the forward environment chain (see env_chain_kernel).
struct ChainSite {
  int core_off;     // float offset of the core (into cores[] or the label core when is_label)
  int is_label;
  int n_in, n_out;  // n_in = dimension of the incoming environment, n_out of the produced one
  int s_in, s_d, s_out;
  int x_site;       // absolute site whose features are contracted
  long long env_out_off;  // float offset of the produced environment slot, -1 for the label site
};

// Everything the wide step kernel needs, in the sweep-relative frame.
struct WideParams {
  int b, b_pad, L;
  int h, g;            // behind / ahead bond of the merged tensor of THIS step
  int hp, gp;          // the same for the previous step (f part); gp == shared bond of this step
  int do_f;            // recompute f from the previous step's updated B
  int do_ext;          // behind environment has to be extended (k >= 1)
  int first_ext;       // extension starts from the scalar 1 (k == 1)
  int act_fn, loss_fn;
  float T;
  const float *x_km1, *x_k, *x_kp1;   // [b_pad][D]
  const float *Hprev;  // behind env of the previous step  [hp][b_pad]
  float *Hcur;         // behind env of this step          [h][b_pad]  (written when do_ext)
  const float *Gprev;  // ahead env of the previous step   [gp][b_pad]
  const float *Gcur;   // ahead env of this step           [g][b_pad]
  const float *Bprev;  // updated merged tensor of the previous step, relative layout
  CoreView ext_core;   // core of site t=k-1: A(hp, d, h)
  const int *y;        // [b_pad]
  float *f;            // [L][b_pad]   read (do_f == 0) or written (do_f == 1)
  float *slabs;        // [nblk][slab_stride]
  int slab_stride;
  int bsize;           // h*D*D*g*L
  double *stamps;      // diagnostic cycle stamps of workgroup 0 (nullptr normally)
};

struct NarrowParams {
  int L, D;
  int h, g, s, m;          // behind, ahead, shared bond before the step; kept rank m
  int bsize;               // h*D*D*g*L
  int l2_flag;
  float lr, wd;
  double inv_b_global;     // 1 / global batch
  const float *red;        // reduced slab: dB_raw (relative layout) + metric tail
  CoreView lab;            // label core of site t=k:   A(h, d, s, l)
  CoreView pl;             // plain core of site t=k+1: A(s, d, g)
  const double *Nh;        // behind norm env (h x h) or nullptr (== [[1]])
  const double *Ng;        // ahead  norm env (g x g) or nullptr
  float *Bnew;             // out: updated merged tensor, relative layout
  float *out_behind;       // out: new plain core of site t=k
  int ob_s_h, ob_s_d, ob_s_m;          // strides of (h, d, s') in out_behind
  float *out_ahead;        // out: new label core of site t=k+1
  int oa_s_m, oa_s_d, oa_s_g;          // strides of (s', d, g) in out_ahead (label stride 1)
  double *Nh_new;          // out: behind norm env of the next step (m x m)
  float *metrics;          // out: (accuracy, MAE) of this step
  double *dbg;             // debug block (see narrow kernel), may be nullptr
  double *stamps;          // cycle stamps (diagnostic), may be nullptr
  unsigned long long *counters;  // [0] += jacobi sweeps, [1] += SVDs, [2] += jacobi rounds, [3] Cholesky steps (always on)
  const float *Bdirect;    // if set: the merged tensor (relative layout) is given, the two cores are not read
  int stop_after_update;   // 1: return after B_new (standalone update_B / compute_L2_reg; needs dbg)
  // fused launch (single GPU, in-LDS path): workgroups 1.. of the same launch reduce the gradient slabs and
  // compute the merged tensor and the L2 term slice by slice; workgroup 0 waits for them on `sync`
  int fused;               // 1: gridDim.x = 1 + nred (+ D*D slice workgroups unless prep_ready)
  int prep_ready;          // prepB / prepG were produced by the preceding wide launch
  const float *slabs;      // [nslabs][slab_stride]
  int nslabs, slab_stride, nred;
  float *red_out;          // == red
  float *prepB;            // [bsize] merged tensor (float), written by the slice workgroups
  double *prepG;           // [bsize] Ln.B.Rn
  unsigned *sync;          // arrival counter, zero between launches
  double trunc_thr;        // > 0: adaptive truncation threshold on cumsum(S) / sum(S); m is then the cap
  int left_dir;            // direction (only read when trunc_thr > 0: the output strides follow the kept rank)
  int *m_out;              // device int receiving the kept rank (adaptive truncation), may be nullptr
  double chol_thr;         // > 0: one pivoted-Cholesky step before the Jacobi iteration when off(G) / trace(G) exceeds it
  double svd_stop2;        // Jacobi stops after a sweep whose rotations all had g^2 / scale^2 <= svd_stop2 (tnml_set_svd_stop)
  int *status;             // device status word: bit0 non-finite, bit1 jacobi not converged, bit2 helpers late, bit3 flag never seen
  int wait_count;          // fused / pipelined launch: helper arrivals workgroup 0 waits for on `sync`
  // pipelined step (wide_pipe_device.h): the raw gradient is A_{k-1}^T . Z_k, Z_k reduced by the previous launch
  int pipe;                // 1: `zred` replaces `red`
  int z_first;             // first step of a sweep: Z_0 is the gradient itself
  int z_rows;              // h_{k-1} * D
  int zsize;               // elements of Z_k (the metric tail follows)
  const float *zred;
  CoreView zcore;          // A_{k-1}(h_{k-1}, d, h_k)
  unsigned *flag;          // if set: B_new is stored with agent-scope stores and `token` is written here afterwards
  unsigned token;
  // persistent sweep (sweep_persist_kernel, kernels_narrow.hip): the workgroup loops over the steps of a sweep; merged tensor, L2 term
  // and raw gradient of step k come from the helper workgroups of the launch (projections with the behind core of step k-1)
  int persist;             // 1: called from sweep_persist_kernel (pipe == 1 as well)
  int write_ahead;         // the new label core is wanted (last step of the launch); otherwise its product is skipped
  int persist_off;         // byte offset of the persistent LDS region (PersistLds), Mcap its capacity per bond
  int Mcap;
  const float *prepRaw;    // raw gradient of this step [h][RW] (beside prepB / prepG), written by the helper workgroups
  const unsigned *pready;  // >= pwant: every helper workgroup has stored its slice of the three
  unsigned pwant;
  double *Apub;            // out: behind core before rounding [D h][m], 1 / sigma [m], next behind norm environment [m][m]
  unsigned *aflag;         // set to coretoken once the behind core before rounding and 1 / sigma are stored (in phase 9, as soon as both are complete): the
                           // helpers start the projections that do not need the norm environment
  unsigned *coreflag;      // set to coretoken at the end of the step: the norm environment in Apub and the float32 behind core are stored
                           // (helpers: the L2 projection; batch side: extends)
  unsigned coretoken;
  // two-stream communicator path without events (tnml_api.hip, split branch): the update workgroup waits for zpoll_flag to reach
  // zpoll_want before it touches zred (the side stream's all-reduce is followed by a one-thread kernel that stores it), and stores
  // done_val to done_flag behind an agent-scope release when everything it writes is out (the side stream's next batch launch sits
  // behind a one-wave kernel that waits for it)
  const unsigned *zpoll_flag; unsigned zpoll_want;
  unsigned *done_flag; unsigned done_val;
  unsigned *abort_flag;    // set by any workgroup whose wait timed out; every wait of the launch gives up once it is set
};

// LDS that survives from one step of a persistent sweep to the next (update workgroup only)
struct PersistLds { double *Nh, *Ad; };
__host__ __device__ inline PersistLds persist_lds(unsigned char *base, int Mcap) {
  PersistLds q;
  q.Nh = (double *)base;                       // [m][m]   behind norm environment of the next step
  q.Ad = q.Nh + (size_t)Mcap * Mcap;           // [D h][m] behind core of the step just finished (U sqrt(S)) before its rounding to float32
  return q;
}
inline size_t persist_lds_bytes(int Mcap) {
  return ((size_t)Mcap * Mcap + (size_t)kD * Mcap * Mcap) * sizeof(double) + 16;
}

struct NormChainSite {
  int core_off;
  int n_in, n_out, s_in, s_d, s_out;   // A(in, d, out): env over `in` -> env over `out`
  long long env_out_off;               // double offset of the produced norm environment
};

void launch_transpose_input(const float *X_bnd, float *X_nbd, int b, int b_pad, int N, hipStream_t st);
void launch_env_chain(const ChainSite *sites_dev, int n_sites, const float *cores, const float *labcore,
                      const float *X, float *env_base, float *f, int b, int b_pad, int L, int Mmax,
                      float *logmax_out, hipStream_t st, bool force_plain = false);
constexpr int kChainSamplesPerBlock = 16;
// The label site between two environments (kernels_meet.hip): f[l][s] = sum_{a,d,c} Lenv[a][s] x[s][d] core[a][d][c][l] Renv[c][s]
struct MeetParams {
  const float *Lenv, *Renv;   // [ml][b_pad], [mr][b_pad]
  const float *x;             // [b_pad][D] features of the label site
  const float *core;          // [ml][D][mr][L]
  float *f;                   // [L][b_pad]; samples b .. b_pad-1 receive 0
  int b, b_pad, ml, mr, D, L;
  int rows_per_chunk;         // a-rows of the core staged in LDS at a time; <= 0: as many as fit (label_meet_chunk_rows)
};
int label_meet_chunk_rows(int ml, int mr, int D, int L);
size_t label_meet_lds_bytes(int rows_per_chunk, int mr, int D, int L);
// false: refused (geometry, or not even one a-row of the core fits in LDS)
bool launch_label_meet(MeetParams p, hipStream_t st);
// slice-wise pre-computation of the merged tensor and its L2 term (small_gemm_device.h: prep_slice_block)
struct PrepParams {
  CoreView lab, pl;        // as NarrowParams
  const double *Nh, *Ng;
  int h, g, s, L, l2_flag;
  float *prepB;
  double *prepG;
  int nparts;              // row parts per slice (0 == 1): workgroup index = part * D * D + slice
};

// false: no kernel of this build fits the tile's operands into LDS.  *prep_done: the launch carried the D*D slice workgroups
// that fill prep.prepB / prep.prepG
bool launch_wide(const WideParams &p, int nblk, const PrepParams *prep, hipStream_t st, bool *prep_done);
void launch_f_only(const WideParams &p, int nblk, hipStream_t st);
void launch_reduce(const float *slabs, int nblk, int slab_stride, int n, float *red, hipStream_t st);
void launch_narrow(const NarrowParams &p, size_t lds_bytes, hipStream_t st);   // grid = p.fused ? 1 + p.wait_count : 1
// Large-tensor path of the same step (kernels_big.hip): HBM scratch, n = min(rows, cols) <= 128.
struct BigScratch {
  float *Bf;          // [bmax]   merged tensor
  double *T;          // [bmax]   Nh^T . B, or (factored form) NL = Nh^T . lab followed by PR = pl . Ng
  double *part;       // [kBigParts][3] block-partial sums, then {step factor, sum|B|, sum|dv|, L2 sum}
  double *gram;       // [8][128][128] partial Gram matrices
  double2 *rotlog;    // [(kJacobiMaxSweeps * 127 + 2)][64] rotations (c, s) in application order
  double *lam;        // [3][128] eigenvalues by position, sigma^(1/2), sigma^(-1/2) of the kept columns
  int *info;          // rounds applied, sweeps, converged, kept rank, then the eigenvalue order [128]
  double *VW;         // [(rows + cols)][n]  V, then W^T V
  float *Cb;          // [rows][m]  new behind core, contiguous
  double *T2;         // [rows][m]
  unsigned *prog;     // [0..6] progress / final word / time-out notes of the replay that rides in the Jacobi launch, [7] arrival
                      //        counter of the weight-decay kernel's blocks (kernels_big.hip)
};
constexpr int kBigMaxN = 128;
constexpr int kBigParts = 2048;
size_t big_jacobi_lds_bytes(int n);
// false: a launch of the path was illegal or (check) failed; big_launch_error() names it
// `front`: the raw gradient of a pipelined large-tensor step, red = A^T . Z, formed in the SAME launch as the merged tensor
// (neither needs the other); without a merged tensor to form it is launched alone, in front of the chain
struct BigFront {
  const float *Z; CoreView A; int ncols; float *red;
  // optional: the behind environment E_k and P'_k = E_k (x) x_k of the NEXT step's batch kernel in the same launch (big_ext_kernel's work)
  const float *ext_Eprev = nullptr, *ext_x_km1 = nullptr, *ext_x_k = nullptr; CoreView ext_A{}; int b_pad = 0;
  float *ext_Ecur = nullptr, *ext_Pk = nullptr;
  // optional: Z (and what the extension rewrites) belongs to the side stream until poll_flag has reached poll_want (big_signal_kernel);
  // wait_ev: the event to fall back on where the contraction is launched alone
  unsigned *poll_flag = nullptr; unsigned poll_want = 0; hipEvent_t wait_ev = nullptr;
  bool ext_acquire = false;      // the extension's inputs were written on the side stream too (behind the first pipelined step)
};
bool launch_narrow_big(const NarrowParams &p, const BigScratch &s, hipStream_t st, bool check, bool prep_only = false,
                       bool skip_prep = false, hipEvent_t after_update = nullptr, const BigFront *front = nullptr,
                       unsigned *sig_flag = nullptr, unsigned sig_val = 0);      // sig_flag: the Gram kernel stores sig_val there (instead of the event)
bool launch_big_signal(unsigned *flag, unsigned value, hipStream_t st);
bool launch_big_gate(const unsigned *flag, unsigned want, int *status, hipStream_t st);
// pipelined large-tensor step: behind environment + (h, d) operand of the pre-gradient; raw gradient = A^T . Z (kernels_big.hip)
bool launch_big_ext(const float *Eprev, const float *x_km1, const float *x_k, const CoreView &A, int b_pad, float *Ecur, float *Pk,
                    hipStream_t st);
bool launch_big_contract(const float *Zred, const CoreView &A, int ncols, float *red, hipStream_t st);
// LDS the tiled batch kernel asks for at these dimensions (0: the shape is beyond it)
size_t wide_tiled_lds_bytes(int L, int h, int hp, int gp, int g, bool ext);
void launch_wide_tiled(const WideParams &p, int nblk, size_t lds_bytes, hipStream_t st);
const char *big_launch_error();
size_t narrow_lds_bytes(int h, int g, int s, int L, int m);
void launch_norm_chain(const NormChainSite *sites_dev, int n_sites, const float *cores, double *env_base,
                       int Mmax, hipStream_t st);
void launch_scale(float *p, size_t n, float factor, hipStream_t st);
void launch_absmax(const float *f, int L, int b, int b_pad, float *out, hipStream_t st);
void launch_activation(const float *f, const int *y, int L, int b, int b_pad, int act_fn, int loss_fn,
                       float T, float *act_out, float *der_out, hipStream_t st);

// Generic feature dimension (kernels_anyd.hip): per-step launches only.  false: the launch was refused (geometry / LDS).
void launch_transpose_input_anyd(const float *X_bnd, float *X_nbd, int b, int b_pad, int N, int D, hipStream_t st);
size_t anyd_chain_lds_bytes(int Mmax, int D, int L);
bool launch_env_chain_anyd(const ChainSite *sites_dev, int n_sites, const float *cores, const float *labcore, const float *X,
                           float *env_base, float *f, int b, int b_pad, int L, int Mmax, int D, float *logmax_out, hipStream_t st);
bool launch_norm_chain_anyd(const NormChainSite *sites_dev, int n_sites, const float *cores, double *env_base, double *T_scratch,
                            int Mmax, int D, hipStream_t st);
size_t anyd_batch_lds_bytes(int D, int hp, int gp, int h, int g, int L);
// batch side of a step (WideParams as for the classic wide kernel; do_grad = false: f of the previous step only, f_only_kernel's role)
bool launch_batch_anyd(const WideParams &p, int D, int nblk, bool do_grad, hipStream_t st);
size_t anyd_update_lds_bytes(int n_pad, bool w_in_lds);
// update side: p.dbg is required (the capture block is the workspace); W_scratch [128 x 128], T2_scratch [2 * D * Mmax * Mmax] doubles
bool launch_update_anyd(const NarrowParams &p, double *W_scratch, double *T2_scratch, hipStream_t st);

// Device-resident dataset (kernels_dataset.hip): gather / embed / re-tile of the samples idx[0..b) and metrics over f.
struct DatasetGather {
  const float *data;       // features [n][N][D], or pixels [n][N] when `pixels`
  const int *labels;       // [n]; read only when y_out is set
  const int *idx;          // [b] sample rows, every one inside [0, n) (checked on the host before the launch)
  float *out;              // [N][b_pad][D]; samples b .. b_pad-1 are zeroed
  int *y_out;              // [b_pad] or nullptr
  int b, b_pad, N, D, pixels;
  double coef[kMaxD];      // pixels form: sqrt(C(D-1, s)), the constant factors of the feature map
};
constexpr int kDsMetricThreads = 256;
// false: refused (geometry / LDS)
bool launch_dataset_gather(const DatasetGather &p, hipStream_t st);
size_t dataset_metrics_lds_bytes(int L);
// part [ceil(b / kDsMetricThreads)][4] block partials; acc[4] = {correct, sum |onehot - act(f)|, non-finite samples, samples},
// restarted from zero when reset != 0 and continued otherwise
bool launch_dataset_metrics(const float *f, const int *y, int L, int b, int b_pad, int act_fn, float T, double *part, int reset, double *acc,
                            hipStream_t st);

// Input gradients (kernels_inputgrad.hip): both chains of 64 samples per workgroup, the body of grad_chain_device.h (which also
// has grad_chain_lds_bytes, the LDS of this kernel and of core_grad_chain_kernel).
struct InputGradParams {
  const int *bond;         // [N-1] bond dimensions of the chain
  const float *cores;      // plain cores, core i at i * core_stride, [ml][D][mr]
  const float *labcore;    // [ml][D][mr][L] of site l_pos
  const float *X;          // [N][x_bpad][D]; samples b .. b_pad-1 are zero
  const float *cot;        // [L][b_pad]
  float *stack;            // [N][cap][b_pad]: slot i receives P_i, i = 1 .. N-1
  float *g;                // [b][N][D]
  float *cf;               // [b] or nullptr
  size_t core_stride;
  int b, b_pad, x_bpad, N, D, L, l_pos;
  int cap;                 // rows of a stack slot: the context's bond capacity
  int mb;                  // largest bond of the chain: what the LDS tiles are sized for
};
// false: refused (geometry / LDS)
bool launch_input_grad(const InputGradParams &p, hipStream_t st);
// cot [L][b_pad] = one-hot of the first maximum of f [L][f_bpad] per sample, zero for samples b .. b_pad-1
bool launch_input_grad_onehot(const float *f, int f_bpad, int L, int b, float *cot, int b_pad, hipStream_t st);
struct InputGradPixels {
  const float *g;          // [b][N][D]
  const float *data;       // pixels [n][N] of the dataset
  const int *idx;          // [b] sample rows
  float *out;              // [b][N]
  int b, N, D;
  double coef[kMaxD];      // sqrt(C(D-1, k))
};
bool launch_input_grad_pixels(const InputGradPixels &p, hipStream_t st);

// Core gradients (kernels_coregrad.hip): one parameter block for the chain kernel (both stacks, cf) and the reduction kernel (G).
struct CoreGradParams {
  const int *tab;          // [2N]: tab[0 .. N-2] bond dimensions of the chain; tab[N + i] offset of core i in the flat layout of G
  const float *cores;      // plain cores, core i at i * core_stride, [ml][D][mr]
  const float *labcore;    // [ml][D][mr][L] of site l_pos
  const float *X;          // [N][x_bpad][D]; samples b .. b_pad-1 are zero
  const float *cot;        // [L][b_pad]
  float *stackP;           // [N][cap][b_pad]: slot i receives P_i, i = 1 .. N-1
  float *stackQ;           // [N][cap][b_pad]: slot i receives Q_i, i = 0 .. N-2
  float *G;                // the layout of tnml_get_cores: core after core, (ml, D, mr), on l_pos (ml, D, mr, L)
  float *cf;               // [b] or nullptr
  size_t core_stride;
  int b, b_pad, x_bpad, N, D, L, l_pos;
  int cap;                 // rows of a stack slot: the context's bond capacity
  int mb;                  // largest bond of the chain: what the LDS tiles are sized for
  int first;               // reduction: 1 = the accumulators start at zero, 0 = they start from G (a chunk after the first)
};
size_t core_grad_reduce_lds_bytes(int mb, int D);
// workgroups of the reduction along y: four waves, each with two 16 x 16 output tiles side by side, cover a site of bonds <= mb
int core_grad_reduce_blocks(int mb, int D);
// false: refused (geometry / LDS)
bool launch_core_grad_chain(const CoreGradParams &p, hipStream_t st);
bool launch_core_grad_reduce(const CoreGradParams &p, hipStream_t st);

// Range-safe chains: the gradient kernels with a power-of-two exponent per sample carried along both passes.
// The blocks wrap the plain ones, whose fields and order stay what the stand-in runtime and the traces read.
struct InputGradScaledParams {
  InputGradParams base;
  int *estack;             // [N][b_pad]: row i receives the exponent of P_i in base.stack, i = 1 .. N-1
};
struct CoreGradScaledParams {
  CoreGradParams base;     // stackQ receives ldexpf(Q_i, eP_i + eQ_i): the reduction kernel runs on it as it is
  int *estack;             // [N][b_pad]: row i receives the exponent of P_i in base.stackP, i = 1 .. N-1
};
bool launch_input_grad_scaled(const InputGradScaledParams &p, hipStream_t st);
bool launch_core_grad_chain_scaled(const CoreGradScaledParams &p, hipStream_t st);
// Prediction with per-sample exponents (kernels_scaled.hip): both half-chains towards the label site and the label site itself in
// one kernel, 64 samples per workgroup, no environment stored.  f[l][s] = mant[l][s] 2^expo[s], 0.5 <= max_l |mant[l][s]| < 1
// (expo = 0 and the plain values where every f[:, s] is 0 or one is not finite); f receives ldexpf(mant, expo).
struct ScaledPredParams {
  const int *bond;         // [N-1] bond dimensions of the chain
  const float *cores;      // plain cores, core i at i * core_stride, [ml][D][mr]
  const float *labcore;    // [ml][D][mr][L] of site l_pos
  const float *X;          // [N][b_pad][D]; samples b .. b_pad-1 are zero
  float *mant;             // [L][b_pad]
  int *expo;               // [b_pad]
  float *f;                // [L][b_pad]
  size_t core_stride;
  int b, b_pad, N, D, L, l_pos;
  int mb;                  // largest bond of the chain: what the LDS tiles are sized for
};
size_t scaled_pred_lds_bytes(int mb, int D, int L, int N);
// false: refused (geometry / LDS)
bool launch_scaled_pred(const ScaledPredParams &p, hipStream_t st);

// Gradient training (kernels_optim.hip): the loss derivative of a chunk as the cotangent of the core gradients, and one optimiser
// step over all cores.
struct LossCotParams {
  const float *f;          // [L][f_bpad]: the prediction chain's output for the chunk
  const int *y;            // [b] labels of the chunk's samples
  float *cot;              // [L][b_pad]: loss derivative of samples 0 .. b-1, zero for b .. b_pad-1
  int L, b, b_pad, f_bpad, act_fn, loss_fn;
  float T;
};
struct OptimStepParams {
  const int *tab;          // the table of CoreGradParams: bonds, then every core's offset in the flat layout
  float *cores;            // plain cores, core i at i * core_stride; only the first ml D mr floats of a slot are touched
  float *labcore;          // [ml][D][mr][L] of site l_pos
  const float *G;          // gradient, flat layout
  float *s0, *s1;          // optimiser state, flat layout: SGD vel (nullptr without momentum) / Adam m and v
  size_t core_stride;
  int N, D, L, l_pos;
  int kind, clip;          // TNML_OPT_SGD / TNML_OPT_ADAM; SGD: the per-core clip
  float lr, wd;
  double mu, beta1, beta2, eps;
  double corr1, corr2;     // Adam: 1 - beta1^t and 1 - beta2^t of this step
  // likelihood training; both off for the discriminative path
  int renorm;              // 1: a third pass gives every core the Frobenius norm it had before the step
  const int *skip;         // nullptr, or the sticky word of nll_record_kernel: non-zero, the launch touches neither cores nor state
};
size_t loss_cot_lds_bytes(int L);
// false: refused (geometry / LDS)
bool launch_loss_cot(const LossCotParams &p, hipStream_t st);
bool launch_optim_step(const OptimStepParams &p, hipStream_t st);

// Orthogonal form, compression, bond spectra (kernels_orth.hip): the operations of a call in the order the one
// workgroup performs them, and the parameter block shared by the three kernels of the call.
constexpr int kOrthRight = 0;    // decompose the site towards the right: it becomes a left isometry, the bond on its right is cut
constexpr int kOrthLeft = 1;     // towards the left: right isometry, the bond on its left is cut
constexpr int kOrthCentre = 2;   // absorb, normalise to Frobenius norm 1 (its log joins the log-norm) and store
struct OrthOp {
  int site, kind;
  int cut;                 // decompositions: 0 rank rule only, 1 and the bond's spectrum is recorded, 2 and the bond is cut (m_max / threshold)
  int pad;
};
struct OrthParams {
  const OrthOp *ops;       // [n_ops]
  int n_ops;
  int N, D, L, l_pos;
  int *bond;               // [N-1] scratch copy of the bond table: the chain kernel rewrites it as it goes
  const float *cores;      // the context's slots (read by the load kernel only), core i at i * core_stride
  const float *labcore;
  double *W;               // float64 work copy: N slots of core_stride doubles, then the label site's lab_elems
  double *Mbuf;            // [lab_elems] the site with its carried factor absorbed
  double *aux;             // [4][aux_stride]: two carried factors (r x n), P and its inverse of the re-orthogonalisation (r x r)
  size_t core_stride, lab_elems, aux_stride;
  int ld, npad;            // LDS geometry (launch_orth fills them from the largest bond)
  int m_max;
  double threshold, rank_tol;
  double *sigma_out;       // [N-1][sigma_ld] normalised spectrum of every bond whose decomposition has cut >= 1
  int sigma_ld;
  double *discarded_out;   // [N-1]
  int *rank_out;           // [N-1] rank by the rank rule, before a cut
  double *result;          // [0] log-norm, [1] g = exp(log-norm / N)
  int *status;             // [0]: 1 non-finite (or zero) input / result, 2 the Jacobi iteration or the re-orthogonalisation did not converge
  float *out_cores;        // float32 scratch copy of the slots: g . W, zero behind core_elems
  float *out_lab;
};
size_t orth_chain_lds_bytes(int mb);
// load, chain and store kernel of one call; mb: largest bond of the chain.  false: refused (geometry / LDS)
bool launch_orth(const OrthParams &p, int mb, hipStream_t st);

// Inner products and linear combinations of two MPS (kernels_algebra.hip): one parameter block for the three
// kernels.  Chain 0 is W, the context's (plain cores in their slots, the label core in its buffer), chain 1 is V in the flat layout of
// tnml_get_cores; products 0, 1, 2 are <W|W>, <V|V>, <W|V>, and workgroup (product, half) of the chain kernel has the number
// 2 * product + half (half 0: sites 0 .. l_pos-1, half 1: sites N-1 .. l_pos+1).
struct AlgebraParams {
  int N, D, L, l_pos;
  int n_prod;              // 1: <W|W> alone (chain 1 is not read), 3: all three
  int metric_sites;        // 0: identity, 1: one [D][D] for all sites, N: [N][D][D]
  int lds_m2;              // LDS geometry: the square of the largest bond of either chain (launch_inner fills it)
  const int *bond;         // [2][N-1] bond dimensions of W, then of V
  const long long *off;    // [2][N] float offset of core i from w_plain / v_plain (not read for the label site)
  const float *w_plain, *w_lab, *v_plain, *v_lab;
  const double *metric;
  double *stage;           // [6][2][stage_stride] the two cores of the site a workgroup is on, as doubles
  size_t stage_stride;
  double *half_E;          // [6][half_stride] what each half-chain hands to the meet kernel, with half_expo [6]: E 2^expo is the half's product
  size_t half_stride;
  int *half_expo;
  double *out;             // [6] {sign, log|.|} per product
  int *status;             // [0]: 1 a non-finite input or result
  // sum_place_kernel: the float32 scratch copy of the slots of alpha W + beta V, zero behind each core
  double alpha, beta;
  float *out_cores, *out_lab;
  size_t core_stride, lab_elems;
};
size_t algebra_chain_lds_bytes(int mb_w, int mb_v);
size_t algebra_meet_lds_bytes(int mb_w, int mb_v);
// chain and meet kernel of one tnml_inner call; mb_w, mb_v: largest bond of either chain.  false: refused (geometry / LDS)
bool launch_inner(const AlgebraParams &p, int mb_w, int mb_v, hipStream_t st);
bool launch_sum_place(const AlgebraParams &p, hipStream_t st);

// Samples and log-likelihoods of the Born distribution (kernels_sample.hip): one parameter block for the
// environment kernel (phase 1: the sites all class slots share, phase 2: one workgroup per slot) and the walk kernel (one workgroup
// per tile of kSmpTile samples of ONE slot).  A slot is a class the call conditions on, or -1 for the label summed; the call's slots
// are numbered 0 .. n_slots-1 in slot_class.
constexpr int kSmpTile = 16;
constexpr int kSmpMaxK = 256;
constexpr int kSmpMaxBond = 64;
struct SampleParams {
  int N, D, L, l_pos, K;
  int n, n_given, n_tiles, n_slots;
  int phase;               // environment kernel: 1 or 2 (launch_sample fills it)
  int lds_m;               // LDS geometry: the largest bond (launch_sample fills it)
  const int *bond;         // [N-1]
  const float *cores, *lab;
  size_t core_stride;
  const double *S;         // [D][D] sum_k w_k phi_k phi_k^T
  const double *phi, *w;   // [K][D], [K]
  const int *slot_class;   // [n_slots]
  double *env_shared;      // [N+1][env_stride]: R_i for i > l_pos (R_N = 1)
  double *env_slots;       // [n_slots][l_pos+1][env_stride]: R_i for 1 <= i <= l_pos
  size_t env_stride;
  double *stage;           // [n_slots][stage_stride] the metric-folded core of the site a workgroup is on
  size_t stage_stride;
  const int *tile_slot;    // [n_tiles]
  const int *tile_samples; // [n_tiles][kSmpTile] sample numbers, -1 behind the last of a slot
  const int *classes;      // [n]
  const int *given;        // [n][n_given] (not read when n_given is 0)
  const double *u;         // [n][N+1], or null: the counter hash of (seed, sample, site)
  unsigned long long seed;
  int *levels;             // [n][N]
  int *labels;             // [n]
  double *logp;            // [n][2]
  int *status;             // [0] bit 1 non-finite, bit 2 a sample of zero weight; [1] the smallest such sample
};
size_t sample_env_lds_bytes(int mb, int D);
size_t sample_walk_lds_bytes(int mb, int D, int L, int K);
// the two environment launches and the walk of one tnml_sample call; mb: largest bond.  false: refused (geometry / LDS)
bool launch_sample(const SampleParams &p, int mb, hipStream_t st);

// The same given any set of known pixels (kernels_sample_masked.hip): one parameter block for the environment
// kernel and the walk kernel of one chunk of tiles.  A row is a sample of the call or an empty mask (tile_rows -1: the normaliser of
// its class slot, or padding); a tile holds T rows of one class slot, and row r of the launch owns stack slots [r][0 .. N].
constexpr int kSmkMaxTile = 16;
struct SampleMaskedParams {
  int N, D, L, l_pos, K;
  int n;                   // samples of the CALL (the extent of mask, known, u and the outputs)
  int T, n_tiles;          // rows per tile (16, 8, 4, 2 or 1), tiles of this launch
  int lds_m;               // LDS geometry: the largest bond (launch_sample_masked fills it)
  int mask_rows;           // 1 or n
  const int *bond;         // [N-1]
  const float *cores, *lab;
  size_t core_stride;
  const double *S;         // [D][D] sum_k w_k phi_k phi_k^T
  const double *phi, *w;   // [K][D], [K]
  const int *tile_class;   // [n_tiles]
  const int *tile_rows;    // [n_tiles][T] sample numbers of the call, -1: the empty mask
  const unsigned char *mask;   // [mask_rows][N]
  const int *known;        // [n][N], read where the mask is set
  double *stack;           // [n_tiles T][N+1][env_stride]: R_{s,i}, R_{s,N} = 1
  size_t env_stride;
  double *E;               // [n_tiles T] log R_{s,0} + ln2 sum of the exponents
  const double *u;         // [n][N+1], or null: the counter hash of (seed, sample, site)
  unsigned long long seed;
  int *levels;             // [n][N]
  int *labels;             // [n]
  double *logp0;           // [n]
  int *status;             // [0] bit 1 non-finite, bit 2 a sample whose densities sum to nothing; [1] the smallest such sample
};
size_t sample_masked_env_lds_bytes(int mb, int D, int T);
size_t sample_masked_walk_lds_bytes(int mb, int D, int L, int K, int T);
// the largest T of 16, 8, 4, 2, 1 at which both kernels fit 160 KB of LDS; 0: none does
int sample_masked_tile(int mb, int D, int L, int K);
// the environment launch and (walk) the walk launch of one chunk; mb: largest bond.  false: refused (geometry / LDS)
bool launch_sample_masked(const SampleMaskedParams &p, int mb, bool walk, hipStream_t st);

// Per-pixel conditionals (kernels_site_cond.hip): the environment launch above with the tile of this call, then
// site_cond_kernel on the same tiles, rows and stack.  The left environment is formed kSccRows rows at a time, so that its two
// products with the core are never whole in LDS together; that number is part of every result (it fixes the order of the sums).
constexpr int kSccMaxBond = TNML_SITE_COND_MAX_BOND;   // the one bond limit of tnml_site_conditionals
constexpr int kSccRows = 16;
struct SiteCondParams {
  SampleMaskedParams m;    // the block of the environment launch: tables, grid, stack, E, status (u, levels, labels, logp0 unused)
  const double *values;    // [K] the number each level stands for
  double *lf_next;         // [n_tiles T][env_stride] the left environment behind the site a row is on, before its power of two
  double *q;               // [n][N][D][D]  Q / tr(S Q)
  double *stats;           // [n][N][4]     mean, variance, entropy, log p(known level) (0 on a free site)
  int *mode;               // [n][N]
};
size_t site_cond_lds_bytes(int mb, int D, int K, int T);
// the largest T of 16, 8, 4, 2, 1 at which the environment kernel and site_cond_kernel both fit 160 KB of LDS (and which
// sample_masked_tile allows, whose launch function is used); 0: none does
int site_cond_tile(int mb, int D, int L, int K);
// the environment launch and site_cond_kernel of one chunk; mb: largest bond.  false: refused (geometry / LDS)
bool launch_site_cond(const SiteCondParams &p, int mb, hipStream_t st);

// Likelihood gradients from incomplete data (kernels_nll_masked.hip): the environment launch above with the tile
// of this call, then masked_grad_kernel on the same tiles, rows and stack, which leaves one partial gradient per tile, and per chunk
// masked_grad_reduce_kernel, which adds the partials in ascending tile order.  The core is worked kNmgRows rows at a time; that
// number and T fix the order of every sum.
constexpr int kNmgMaxBond = kSmpMaxBond;
constexpr int kNmgRows = 16;
struct MaskedGradParams {
  SampleMaskedParams m;    // the block of the environment launch: tables, grid, stack, E, status (u, levels, labels, logp0 unused)
  const int *off;          // [N] the offset of core i in the flat layout of tnml_get_cores
  const double *wrow;      // [n_tiles T] the weight of every row of the launch: 2 / n a sample, -2 the normaliser, 0 padding
  double *lf_next;         // [n_tiles T][env_stride] the left environment behind the site a row is on, before its power of two
  double *part;            // [n_tiles][total] the partial gradient of every tile of the launch
  size_t total;            // floats of the flat layout
  int *status;             // [0] bit 1 a non-finite left environment, bit 2 a per-site normaliser that is not positive and finite
};
struct MaskedGradReduceParams {
  const double *part;      // [n_tiles][total]
  double *acc;             // [total] the running sum over the tiles of the chunks so far
  float *G;                // [total] written by the last chunk
  size_t total;
  int n_tiles, first, last;
  int *status;             // [0] bit 4 an element beyond float32
};
size_t masked_grad_lds_bytes(int mb, int D, int K, int T);
// the largest T of 16, 8, 4, 2, 1 at which the environment kernel and masked_grad_kernel both fit 160 KB of LDS (and which
// sample_masked_tile allows, whose launch function is used); 0: none does
int masked_grad_tile(int mb, int D, int L, int K);
// the environment launch and masked_grad_kernel of one chunk; mb: largest bond.  false: refused (geometry / LDS)
bool launch_masked_grad(const MaskedGradParams &p, int mb, hipStream_t st);
bool launch_masked_grad_reduce(const MaskedGradReduceParams &p, hipStream_t st);

// The gradient of the log-norm (kernels_nll.hip): one parameter block for the environment kernel (two
// workgroups, one per direction) and the gradient kernel (grid (N, L)).  L_i 2^expL[i] and R_i 2^expR[i] are the environments.
constexpr int kLnzMaxBond = 64;
struct LogNormParams {
  int N, D, L, l_pos;
  int metric_sites;        // 0: identity, 1: one [D][D] for all sites, N: [N][D][D]
  int lds_m;               // LDS geometry: the largest bond (the launch functions fill it)
  int mode;                // gradient kernel: 0 stores Gz, 1 replaces G[e] by G[e] - Gz[e]
  int class_plus1;         // environment kernel: 0 the label is summed (what a zeroed block means), q + 1 slice q of the label site alone (the gradient kernel needs 0)
  const int *tab;          // the table of CoreGradParams: bonds, then every core's offset in the flat layout
  const float *cores, *lab;
  size_t core_stride;
  const double *metric;
  double *envL, *envR;     // [N+1][env_stride] each: L_i for i = 0 .. N-1 (L_0 = 1), R_i for i = 0 .. N (R_N = 1)
  int *expL, *expR;        // [N+1] each: the running exponents
  size_t env_stride;
  float *G;                // the layout of tnml_get_cores
  double *out;             // [2] {sign of <W|W>_S, log|<W|W>_S|}
  int *status;             // [0] (environment launch): bit 1 a non-finite environment, bit 2 <W|W>_S == 0; [1] (gradient launch): bit 4 a gradient element beyond float32
};
size_t lognorm_env_lds_bytes(int mb, int D);
size_t lognorm_grad_lds_bytes(int mb, int D);
// mb: largest bond.  false: refused (geometry / LDS)
bool launch_lognorm_env(const LogNormParams &p, int mb, hipStream_t st);
bool launch_lognorm_grad(const LogNormParams &p, int mb, hipStream_t st);
// The likelihood of a batch (kernels_nll.hip): the cotangent of the data term of a chunk, its per-sample terms, and their sum.
struct NllCotParams {
  const float *f;          // [L][f_bpad]: the prediction chain's output for the chunk
  const int *y;            // [b] labels of the chunk's samples, or nullptr: the label is summed
  float *cot;              // [L][b_pad]: zero for samples b .. b_pad-1; nullptr: the value alone is wanted
  double *terms;           // [n] of the call: terms[off + s] = log f_y^2 or log sum_l f_l^2
  int *bad;                // [n] of the call: bad[off + s] = 1 where a cotangent or the term is not finite
  int L, b, b_pad, f_bpad;
  int off;                 // the chunk's first sample within the batch
  int batch;               // samples of the batch the mean runs over
};
// false: refused (geometry)
bool launch_nll_cot(const NllCotParams &p, hipStream_t st);
// acc[0] = sum terms[0 .. n), acc[1] = sum bad[0 .. n), in an order that depends on n alone
bool launch_nll_sum(const double *terms, const int *bad, int n, double *acc, hipStream_t st);
// The record and guard of one likelihood step: one workgroup after nll_sum_kernel and the norm launches.
// rec[0 .. 4) = {acc[0] (the sum of the batch's terms), out[1] (log|Z|), acc[1] (samples with a non-finite cotangent), status bits};
// the bits are status[0] | status[1] of the norm launches, kNllStepBadBatch where acc[1] > 0, kNllStepNotApplied where *skip is set
// on leaving.  *skip is set, never cleared, when any of the other bits is.
constexpr int kNllStepBadBatch = 8, kNllStepNotApplied = 16;
bool launch_nll_record(const double *acc, const double *out, const int *status, double *rec, int *skip, hipStream_t st);

// Pixel-pair marginals (kernels_pair.hip): the environment launch above with the grid's metric and the call's
// class slot into the group's own stacks, then pair_close_kernel (one workgroup per site), and per chunk of rows pair_walk_kernel
// (grid (rows, D^2)) and pair_stats_kernel (grid (N, rows)).  Status word e.status[1]: bit 1 a non-finite or vanishing normaliser.
constexpr int kPairMaxBond = kLnzMaxBond;
constexpr int kPairCloseThreads = 1024;
constexpr int kPairStatThreads = 256;
struct PairParams {
  LogNormParams e;         // the block of the environment launch: table, cores, metric (the grid's S), stacks, exponents, status
  int K;
  int n_rows;              // rows of this chunk
  const double *phi, *w;   // [K][D], [K]
  const double *values;    // [K] the number each level stands for
  const int *rows;         // [n_rows] the sites the chunk's rows start from
  double *B;               // [N][D^2][env_stride]: B_j[e,e'][a,a'], site j closed from the right
  double *q1;              // [N][D][D]
  double *stats1;          // [N][3] mean, variance, entropy
  double *Q;               // [n_rows][N][D^2][D^2]: the walk stores Q_ij unnormalised, the statistics kernel normalises in place
  int *qexp;               // [n_rows][N][D^2]: the running exponent of the walk (row, d, d') at site j
  double *stats;           // [n_rows][N][3] covariance, correlation, mutual information
};
size_t pair_close_lds_bytes(int mb, int D, int K);
size_t pair_walk_lds_bytes(int mb, int D);
size_t pair_stats_lds_bytes(int D, int K);
// threads of a walk workgroup at largest bond mb (the result does not depend on it)
int pair_walk_threads(int mb);
// mb: largest bond.  false: refused (geometry / LDS)
bool launch_pair_close(const PairParams &p, int mb, hipStream_t st);
bool launch_pair_rows(const PairParams &p, int mb, hipStream_t st);

// Two-site likelihood sweep (kernels_nll_sweep.hip).  Everything is in the sweep-relative frame of section 4:
// the step merges relative sites (k, k + 1), `behind` is the chain over the sites the sweep has left, `ahead` the chain over the
// sites in front of the pair; the merged tensor is B[h][dk][dk1][g][l] (the relative layout of NarrowParams::Bdirect).
constexpr int kNllsTile = 64;            // samples per workgroup of the chain and batch kernels
constexpr int kNllsThreads = 256;
constexpr int kNllsUpdThreads = 1024;
constexpr int kNllsRec = 6;              // values per step: the record of tnml_nll_sweep
// one site of a per-sample walk: out[o][s] = sum_{i, d} (in[i][s] x[s][d]) A(i, d, o)
struct NllSweepSite {
  long long core_off;      // float offset of the plain core from `cores`
  long long out_off;       // float offset of the produced environment from `stack`, -1: not stored
  int n_in, n_out, s_in, s_d, s_out;
  int x_site;              // absolute site whose features are contracted
};
struct NllSweepChainParams {
  const NllSweepSite *sites;   // [n_sites] in walk order
  int n_sites;
  const float *cores;
  const float *X;          // [N][x_bpad][D]
  float *stack;
  long long init_off;      // float offset of the slot that receives the walk's start (ones), -1: not stored
  float *last_out;         // [n_out of the last site][b_pad] the walk's end (ones for an empty walk), or nullptr
  int b_pad, x_bpad, D, cap;   // cap: the largest environment of the walk (LDS geometry)
};
struct NllSweepMergeParams {
  CoreView lab, pl;        // as NarrowParams: A(h, d, s, l) of the label site, A(s, d, g) of the site ahead
  int h, g, s, D, L;
  double *B64;             // [h][D][D][g][L]
  float *B32;
};
struct NllSweepBatchParams {
  int b, b_pad, x_bpad, D, L, batch;
  int h, g, hp;            // behind / ahead bond of this step, behind bond of the step before (do_ext)
  int do_ext;              // the behind chain is extended by the core the step before left: Hcur = (Hprev x_km1) . ext_core
  const float *x_km1, *x_k, *x_kp1;   // [x_bpad][D]
  const float *Hprev;      // [hp][b_pad]
  float *Hcur;             // [h][b_pad]: read (do_ext == 0) or written
  CoreView ext_core;       // A(hp, d, h)
  const float *G;          // [g][b_pad] ahead chain
  const float *B32;        // merged tensor, relative layout
  const int *y;            // [b] labels, or nullptr: the label is summed
  float *slabs;            // [tiles][bsize] partial Gd of every workgroup
  double *terms;           // [b] log f_y^2 or log sum_l f_l^2
  int *bad;                // [b] 1 where a cotangent or the term is not finite
};
struct NllSweepUpdateParams {
  int D, L, h, g, bsize, batch, renorm;
  float lr;
  const double *B64;
  const float *Gd;         // [bsize] reduced data gradient
  const double *Nh, *Ng;   // behind (h x h) and ahead (g x g) metric environments with their running exponents
  const int *expH, *expG;
  const double *S;         // [D][D] or nullptr
  const double *acc;       // {sum of the batch's terms, samples with a bad cotangent}
  const int *env_status;   // status word of the environment launch
  double *T1, *T2;         // [bsize] scratch
  float *Bout;             // [bsize] what the split receives as Bdirect
  double *dbg;             // [4][bsize] B, Gd, Gz, B_new
  double *rec;             // [kNllsRec] of this step
  int *skip;               // sticky guard word of the call
};
struct NllSweepExtendParams {
  int right_walk;          // 1: R_i from R_{i+1} (a left step), 0: L_{i+1} from L_i (a right step)
  int ml, mr, D, lds_m;    // the plain core [ml][D][mr] the step left behind; lds_m: LDS geometry (the launch function fills it)
  const int *m_dev;        // the kept rank on the device (adaptive truncation) or nullptr: it replaces mr (right step) / ml (left step)
  const float *core;
  const double *S;         // [D][D] or nullptr
  const double *Ein; double *Eout;   // dense square environments
  const int *exp_in; int *exp_out;
  const double *sigma;     // [n_sigma] singular values of the split, descending
  int n_sigma, m_fixed;
  double *sigma_out;       // [n_sigma] a copy that outlives the capture block of the SVD kernels
  double *rec;             // the step's record: [4] kept rank, [5] discarded weight
  int *status;             // bit 1: a non-finite environment
};
size_t nll_sweep_chain_lds_bytes(int cap, int D);
size_t nll_sweep_batch_lds_bytes(int h, int g, int hp, int D, int L);
size_t nll_sweep_update_lds_bytes();
size_t nll_sweep_extend_lds_bytes(int mb, int D);
// false: refused (geometry / LDS)
bool launch_nll_sweep_chain(const NllSweepChainParams &p, int tiles, hipStream_t st);
bool launch_nll_sweep_merge(const NllSweepMergeParams &p, hipStream_t st);
bool launch_nll_sweep_batch(const NllSweepBatchParams &p, int tiles, hipStream_t st);
bool launch_nll_sweep_reduce(const float *slabs, int tiles, int bsize, float *Gd, hipStream_t st);
bool launch_nll_sweep_update(const NllSweepUpdateParams &p, hipStream_t st);
bool launch_nll_sweep_extend(const NllSweepExtendParams &p, int mb, hipStream_t st);

}  // namespace tnml
