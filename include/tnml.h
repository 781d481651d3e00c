/*
 * tnml.h -- C ABI of libtnml_hip.so: the MI355X (gfx950) backend of the MPS two-site sweep
 * optimiser.
 *
 * The reference (francescovidaich964/TensorNetworkForML) is pure Python/NumPy and has no FFI:
 * its boundary for this path is the Python API of TensorNetwork/Network_class.py.  Each entry
 * point below names the reference method (file:line under /root/reference/TensorNetwork) whose
 * arithmetic it replaces; INTEGRATION.md shows the ctypes stub a maintainer of the reference
 * would add to Network_class.py to call it.
 *
 * Conventions
 *   - every function returns 0 on success and a negative tnml_status on failure;
 *     tnml_last_error() returns a thread-local, human readable message for the last failure;
 *   - plain pointers and sizes only; host pointers unless a name ends in _dev;
 *   - a tnml_ctx owns all device memory, one HIP stream and (optionally) one RCCL communicator;
 *     one host thread per context; calls are stream-ordered and return after enqueueing unless
 *     they hand data back to the host (those synchronise the stream);
 *   - all tensors are float32 on the device; batch-independent norm environments and the
 *     merged-tensor update/SVD run in float64 inside the kernels;
 *   - canonical layouts (identical to oracle/mps_oracle.py):
 *       bond[i]      dimension of the bond between site i and i+1, i = 0..N-2
 *       core i       [ml][D][mr]      ml = bond[i-1] (1 at i = 0), mr = bond[i] (1 at i = N-1)
 *       core l_pos   [ml][D][mr][L]   the label axis is last on the site that carries it
 *       cores_flat   the N cores above concatenated in site order
 *       X            [b][N][D]        as Network.forward receives it (Network_class.py:195)
 *       f, g         [L][b]
 *       env          [b][m]           on the host side of tnml_get_env
 *       B            [ml][D][D][mr][L]  merged two-site tensor (a, d, d', c, l)
 */
#ifndef TNML_H
#define TNML_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct tnml_ctx tnml_ctx;

typedef enum {
  TNML_OK = 0,
  TNML_ERR_ARG = -1,       /* bad argument / shape mismatch (the reference's AssertionError)   */
  TNML_ERR_STATE = -2,     /* call not allowed in this state (the reference's Exception)       */
  TNML_ERR_HIP = -3,       /* HIP runtime failure                                               */
  TNML_ERR_NOGPU = -4,     /* no usable gfx950 device                                           */
  TNML_ERR_COMM = -5,      /* RCCL failure                                                      */
  TNML_ERR_SHAPE = -6,     /* reference truncation policy hits the reference's own ValueError   */
  TNML_ERR_NONFINITE = -7  /* non-finite values reached the SVD (reference: LinAlgError)        */
} tnml_status;

/* activation / loss / truncation selectors (Network_class.py:127-133, :894-945) */
enum { TNML_ACT_LINEAR = 0, TNML_ACT_SIGMOID = 1, TNML_ACT_SOFTMAX = 2 };
enum { TNML_LOSS_MSE = 0, TNML_LOSS_CROSS_ENTROPY = 1, TNML_LOSS_FULL_CROSS_ENT = 2 };
enum { TNML_TRUNC_REFERENCE = 0, TNML_TRUNC_FIXED = 1, TNML_TRUNC_ADAPTIVE = 2 };
enum { TNML_SIDE_LEFT = 0, TNML_SIDE_RIGHT = 1 };

/* what tnml_get_step_debug can hand back about the most recent sweep step */
enum {
  TNML_DBG_B = 0,        /* merged tensor before the update        [ml][D][D][mr][L]            */
  TNML_DBG_DB_RAW = 1,   /* bond gradient before weight decay      same shape                    */
  TNML_DBG_B_NEW = 2,    /* updated, un-truncated merged tensor    same shape                    */
  TNML_DBG_SIGMA = 3,    /* all singular values, descending        [min(rows, cols)]             */
  TNML_DBG_L2 = 4,       /* {L2 loss term, sum|B|, sum|dB|, jacobi sweeps, n, cycles before /
                            in / after the Jacobi loop, 100 MHz ticks of the whole kernel}  [9]  */
  TNML_DBG_L2_GRAD = 5   /* 2*wd*Ln.B.Rn (or wd*B)                 same shape as B               */
};

const char *tnml_last_error(void);
const char *tnml_version(void);
/* number of visible HIP devices (0 without a GPU; never fails) */
int tnml_device_count(void);

/* ---- life cycle ------------------------------------------------------------------------- */
/* Network.__init__ (Network_class.py:84-191) minus the random init, which stays on the host.
 * b_capacity: largest batch a later tnml_set_input may bring (buffers grow if exceeded).
 * D: local feature dimension, 2 <= D <= 8 (TNML_ERR_ARG otherwise).  D = 2 runs every specialised path this header
 * describes.  3 <= D <= 8 runs a generic path of per-step launches (batch kernel -> slab reduction -> update / SVD kernel)
 * with the same layouts ([b][N][D] inputs, [ml][D][mr] cores, [ml][D][D][mr][L] merged tensors), the same capture block
 * and the same limit (short side of the matricised merged tensor <= 128: bond <= 42 at D = 3, <= 32 at D = 4, <= 16 at
 * D = 8).  On a D != 2 context tnml_set_persistent, tnml_set_step_pipeline, tnml_set_chain_path and tnml_set_narrow_path
 * accept their arguments and have no effect, and tnml_comm_init returns TNML_ERR_STATE (multi-GPU is D = 2 only). */
/* A call that fails with TNML_ERR_HIP because an allocation failed leaves the context usable: it holds no half-sized buffer, and the
 * call may be made again (a sweep that stopped inside the chain: from tnml_set_cores on).  A failed tnml_create leaves *out NULL and
 * nothing allocated. */
int tnml_create(tnml_ctx **out, int N, int D, int L, int Mmax, int b_capacity, int device);
int tnml_destroy(tnml_ctx *ctx);
int tnml_synchronize(tnml_ctx *ctx);

/* ---- multi-GPU: batch shards, one RCCL all-reduce of the bond gradient per step ---------- */
/* 128-byte RCCL unique id, created on rank 0 and handed to every rank by the caller. */
int tnml_comm_unique_id(void *uid128);
int tnml_comm_init(tnml_ctx *ctx, int rank, int nranks, const void *uid128);
/* With a communicator the pipelined step is launched in two parts -- update side on the context's stream, batch side on a second
 * stream followed by the all-reduce of the pre-gradient -- so that the exchange travels beside the SVD of the step instead of
 * behind it (on = 1, default).  on = 0: one fused launch per step with the all-reduce between launches (round 2). */
int tnml_set_comm_overlap(tnml_ctx *ctx, int on);
/* measurement: mean device time (us) of one all-reduce of n_floats floats on the exchange stream over `reps` back-to-back calls
 * (collective: every rank calls it; 0 without a communicator; needs one sweep before it) */
int tnml_comm_probe(tnml_ctx *ctx, int n_floats, int reps, double *us_per_allreduce);

/* ---- parameters ------------------------------------------------------------------------- */
/* replaces assignments to Network.As / Network.l_pos
 * cores_flat: the N cores one after another, (ml, D, mr) row-major, the one on site l_pos (ml, D, mr, L); bond[i] joins sites i
 * and i + 1.  Every bond must lie in [1, capacity], where capacity = max(M, D * min(L, M)) for the M given to tnml_create (the
 * reference truncation policy legitimately reaches D * min(L, M) next to a chain end).  A bond above the capacity is refused
 * with TNML_ERR_ARG even where both cores next to it fit their slots -- the environment slots, and the tiles of the chain
 * kernels, hold `capacity` rows.  A refused call leaves the context's cores, bonds and label position as they were. */
int tnml_set_cores(tnml_ctx *ctx, const float *cores_flat, size_t n_floats, const int32_t *bond,
                   int l_pos);
int tnml_cores_size(tnml_ctx *ctx, size_t *n_floats);
int tnml_get_cores(tnml_ctx *ctx, float *cores_flat, size_t capacity, int32_t *bond, int *l_pos);
/* bond [N-1] and l_pos (or NULL) alone: host bookkeeping, nothing is copied from the device */
int tnml_get_bonds(tnml_ctx *ctx, int32_t *bond, int *l_pos);
/* every core *= factor: the calibration loop of Network.__init__ (Network_class.py:175-176) */
int tnml_scale_cores(tnml_ctx *ctx, double factor);
/* Tests and diagnostics: the core slots as the device holds them, padding included -- slots [N][core_stride] with
 * core_stride = Mcap D Mcap floats (Mcap: the bond capacity, max(M, D min(L, M))) and the label buffer [Mcap D Mcap L]; the
 * capacities are in floats (TNML_ERR_ARG when too small). */
int tnml_get_core_slots(tnml_ctx *ctx, float *slots, size_t slots_capacity, float *label_buffer, size_t label_capacity);

/* ---- batch ------------------------------------------------------------------------------ */
/* X [b][N][D] float32, y [b] int32 (may be NULL when only forward is wanted) */
int tnml_set_input(tnml_ctx *ctx, const float *X, const int32_t *y, int b);
/* A data loader that keeps several batches on the device: tnml_stage_batch copies X [b][N][D] and y [b] into device slot
 * `slot` (0..7, synchronous host -> device copy); tnml_select_batch makes a staged batch the resident one with device-side
 * work only (re-tiling to the site-major layout, label copy) and without waiting -- the counterpart of tnml_set_input for
 * inputs that are already in HBM.  No reference analogue (the reference's loaders hand NumPy arrays to forward,
 * Network_class.py:324-327). */
int tnml_stage_batch(tnml_ctx *ctx, int slot, const float *X, const int32_t *y, int b);
int tnml_select_batch(tnml_ctx *ctx, int slot);
/* labels of the resident batch alone (Network.sweep receives y after forward saw X,
 * Network_class.py:327-333) */
int tnml_set_labels(tnml_ctx *ctx, const int32_t *y, int b);

/* ---- hot path --------------------------------------------------------------------------- */
/* Network.forward (Network_class.py:195-258): builds the environment stack for the current
 * l_pos (0 -> right environments, N-1 -> left environments) and f.  f_out [L][b] may be NULL. */
int tnml_forward(tnml_ctx *ctx, float *f_out);
/* max |f| over the (global) batch after a forward: Network_class.py:169 */
int tnml_f_absmax(tnml_ctx *ctx, double *out);
/* log(max |f|) over the (global) batch with per-site renormalisation: the calibration of
 * Network.__init__ (Network_class.py:168-170) needs max|f| of the un-calibrated chain, which is
 * ~1e-66 at N = 784 and underflows float32; this variant is exact in any range and leaves the
 * environment stacks untouched. */
int tnml_forward_logabsmax(tnml_ctx *ctx, double *out);
/* the f the next sweep step starts from (Network.sweep's argument f, Network_class.py:384) */
int tnml_set_f(tnml_ctx *ctx, const float *f);
int tnml_get_f(tnml_ctx *ctx, float *f_out);

/* Network.sweep / sweep_step / update_B / tensor_svd / compute_L2_reg
 * (Network_class.py:384-436, 440-573, 577-763, 839-962, 966-1179): n_steps two-site steps in
 * the given direction, starting at the current l_pos.  A full sweep is n_steps = N-1 right
 * after tnml_forward.
 *   first_of_sweep  non-zero: reset the environment list grown by this direction (:426-429)
 *   metrics_out     [n_steps][2] = (accuracy, MAE) per step (var_hist, :739-750), or NULL
 *   f_out           [L][b] output recomputed from the last updated, un-truncated B (:494-523) */
int tnml_sweep(tnml_ctx *ctx, int left_dir, int n_steps, int first_of_sweep, float lr,
               float weight_dec, int l2_flag, int act_fn, int loss_fn, float T, int trunc_policy,
               float *metrics_out, float *f_out);

/* The three sub-steps the reference also exposes as methods, as standalone device calls (the same
 * kernels as tnml_sweep, run in "stop after the update" / "given merged tensor" modes).
 *   tnml_update_B   Network.update_B (Network_class.py:577-763): extends the behind environment,
 *                   returns the updated merged tensor of sites (p, p+1), p = l_pos (- 1 when left_dir);
 *                   B_canon [ml][D][D][mr][L] or NULL (= product of the two cores); cores, bonds and
 *                   l_pos are left untouched; metrics2 = (accuracy, MAE) or NULL.
 *   tnml_l2_term    Network.compute_L2_reg (:966-1179): loss = wd <B, Ln.B.Rn>, grad = 2 wd Ln.B.Rn.
 *   tnml_svd_split  Network.tensor_svd (:839-962): U sqrt(S) [rows][m] and sqrt(S) Vh [m][cols] of a
 *                   rows x cols matrix (both multiples of D, min <= 128), sigma[min(rows, cols)] or NULL. */
int tnml_update_B(tnml_ctx *ctx, const float *B_canon, int left_dir, float lr, float weight_dec, int l2_flag,
                  int act_fn, int loss_fn, float T, double *Bnew_canon, size_t capacity, float *metrics2);
int tnml_l2_term(tnml_ctx *ctx, const float *B_canon, int left_dir, float weight_dec, double *loss,
                 double *grad_canon, size_t capacity);
int tnml_svd_split(tnml_ctx *ctx, const float *mat, int rows, int cols, int m, float *US, float *SVh,
                   double *sigma);

/* Network.forward's return value for a batch that is NOT made resident (the validation loop of
 * Network.train, Network_class.py:339-346): X [b][N][D] -> f_out [L][b].  One chain towards the label
 * site, no environment is stored; the training batch, its environments and f stay as they are.  Same
 * l_pos restriction as tnml_forward. */
int tnml_predict(tnml_ctx *ctx, const float *X, int b, float *f_out);

/* on = 1: tnml_forward, tnml_predict, tnml_predict_indices and tnml_eval_indices also run with the label at an
 * intermediate site, and a forward there lets tnml_sweep start a segment (below).  Default 0: every call behaves
 * as before.  With a communicator: TNML_ERR_STATE.
 *   tnml_forward at 0 < l < N-1 builds Lenv[0..l-1] and Renv[l+1..N-1] into their usual slots (two half-chains, neither with a
 *   label site) and f[l'][s] = sum_{a,d,c} Lenv[l-1][a][s] x_l[s][d] A_l[a][d][c][l'] Renv[l+1][c][s] (label_meet_kernel,
 *   csrc/kernels_meet.hip); tnml_get_env then answers for both sides.  The three prediction calls run the same kernels and keep
 *   nothing but the two environments next to the label site, in buffers of their own; their f is bit-equal to tnml_forward's.
 *   At l = 0 and l = N-1 every call takes the path it takes with the switch off.  tnml_forward_logabsmax stays ends-only.
 *   Segment start: after such a forward ONE tnml_sweep(first_of_sweep = 0) in either direction is accepted wherever the
 *   position allows the step; it starts from the f of the forward (or of tnml_set_f), and the calls after it continue as any
 *   mid-sweep call does.  Its first step takes the classic launch sequence on every path (the pipelined step resumes with the
 *   second).  The stack behind the segment counts as rewritten once its first step is planned; a call refused or failed before
 *   that leaves both stacks valid.  first_of_sweep = 1 stays ends-only; a direction change, or a sweep after a new batch, still needs a forward first.
 *   tnml_update_B and tnml_l2_term run after an intermediate forward too.   */
int tnml_set_any_position(tnml_ctx *ctx, int on);

/* ---- device-resident dataset --------------------------------------------------------------- */
/* A context can hold ONE dataset of n samples with labels in HBM; batches and evaluations are then formed on the device from
 * index lists, and only the lists and a few scalars cross the bus.  No reference analogue: the reference's
 * loaders hand NumPy arrays to forward (Network_class.py:324-327), its evaluation scripts loop over such batches.
 *   form TNML_DATASET_FEATURES  data [n][N][D] float32, already embedded: what tnml_set_input takes
 *   form TNML_DATASET_PIXELS    data [n][N] float32 in [0, 1]; the feature map of data_generator.psi (D = 2: [sin(pi x / 2),
 *                               cos(pi x / 2)]; D > 2: sqrt(C(D-1, s)) sin^(D-1-s) cos^s) is applied on the device whenever a
 *                               batch is formed, in float64 with one rounding to float32: 1 / D of the memory and of the upload
 * With a communicator attached every call of this block returns TNML_ERR_STATE (a resident dataset is not sharded over ranks). */
enum { TNML_DATASET_FEATURES = 0, TNML_DATASET_PIXELS = 1 };
/* Uploads data and labels [n] int32 (synchronous) and replaces an earlier dataset.  N and D describe `data` and must be the
 * context's (TNML_ERR_ARG otherwise, as for labels outside [0, L)); a refused call leaves an earlier dataset in place.
 * tnml_dataset_detach frees the dataset (tnml_destroy does too); tnml_dataset_size returns n, 0 without a dataset. */
int tnml_dataset_attach(tnml_ctx *ctx, const float *data, const int32_t *labels, int n, int N, int D, int form);
int tnml_dataset_detach(tnml_ctx *ctx);
int tnml_dataset_size(tnml_ctx *ctx);
/* The samples idx[0..b) become the resident batch, labels included: the counterpart of tnml_set_input / tnml_select_batch (same
 * state resets, same growth of the batch buffers).  The list is copied to a buffer of the context and the call returns after
 * enqueueing.  Indices outside [0, n) are refused (TNML_ERR_ARG) before anything is launched and with the resident batch left as it
 * was; repeated indices are allowed. */
int tnml_select_indices(tnml_ctx *ctx, const int32_t *idx, int b);
/* tnml_predict for dataset samples: f_out [L][b]; the resident batch, its environments and f stay as they are. */
int tnml_predict_indices(tnml_ctx *ctx, const int32_t *idx, int b, float *f_out);
/* The evaluation loop of Network.train (Network_class.py:339-346) and of the reference's evaluation scripts, reduced on the device:
 * forward chain over the listed samples in chunks that fit the prediction buffers (b may exceed every batch capacity), then
 *   out3 = {samples whose argmax over labels equals their label (first maximum, taken on f itself: csrc/act_device.h),
 *           sum over samples and labels of |onehot(y) - act(f)| (per sample in float32 as the sweep's metrics, across samples in float64),
 *           samples with a non-finite activated output}
 * Accuracy = out3[0] / b, mean absolute error = out3[1] / (b L).  Same l_pos restriction as tnml_forward. */
int tnml_eval_indices(tnml_ctx *ctx, const int32_t *idx, int b, int act_fn, float T, double *out3);
/* The same three numbers for the resident batch, from the f that tnml_forward or tnml_sweep left on the device (the per-batch
 * training accuracy of Network.train, Network_class.py:327, without copying f back).  Needs no dataset. */
int tnml_resident_metrics(tnml_ctx *ctx, int act_fn, float T, double *out3);
/* The embedded samples idx[0..b) as the device forms them, X_out [b][N][D]: for tests and inspection, not a hot path. */
int tnml_dataset_read(tnml_ctx *ctx, const int32_t *idx, int b, float *X_out);

/* ---- input gradients ------------------------------------------------------------------------- */
/* Which inputs a decision rests on: the gradient of the network output with respect to the embedded inputs (saliency maps, the
 * direction of an adversarial step, the cotangent for a layer in front of the MPS).  No reference analogue.  Two chains per sample on
 * the matrix cores -- one from the left that stores its environments, one from the right that meets them site by site -- in one
 * kernel (csrc/kernels_inputgrad.hip).
 * RANGE: the stored environments are float32 without renormalisation, as tnml_forward's are: the call is meant for calibrated
 * networks (max |f| of order 1); an un-calibrated chain at N = 784 underflows here as it does there.
 * LIMITS: single GPU (TNML_ERR_STATE with a communicator, the rule of the dataset block); the kernel's LDS tiles are sized from the
 * largest bond of the chain, and a shape that needs more than 160 KB is refused with TNML_ERR_ARG and a message naming the bytes
 * (D = 2, two labels, N = 784: bonds up to 85).  Every refusal happens before anything is launched. */
enum { TNML_WRT_FEATURES = 0, TNML_WRT_PIXELS = 1 };
/* g[s][i][d] = sum_l' cot[l'][s] d f[l'][s] / d X[s][i][d] for a batch that is NOT made resident.
 * X [b][N][D], cot [L][b] or NULL (= one-hot of the first maximum of f per sample), grad_out [b][N][D],
 * cf_out [b] or NULL (= sum_l' cot f).  Any l_pos, with or without tnml_set_any_position.
 * b may exceed every batch capacity: the call works in chunks (tnml_set_input_grad_chunk).  Like tnml_predict it leaves the
 * resident batch, its environments, f, the cores and l_pos exactly as they were, and it synchronises before returning. */
int tnml_input_grad(tnml_ctx *ctx, const float *X, int b, const float *cot, float *grad_out, float *cf_out);
/* the same for samples of the attached dataset; wrt = TNML_WRT_FEATURES -> grad_out [b][N][D];
 * wrt = TNML_WRT_PIXELS (dataset in TNML_DATASET_PIXELS form only, TNML_ERR_STATE otherwise) -> grad_out [b][N],
 * the chain rule through the feature map psi, its derivative evaluated in float64 on the device */
int tnml_input_grad_indices(tnml_ctx *ctx, const int32_t *idx, int b, const float *cot, int wrt, float *grad_out, float *cf_out);
/* samples per pass (rounded up to a multiple of 64); 0 = default: the largest multiple of 64 whose stack of stored environments
 * (N x bond capacity x samples floats) stays within 256 MiB, at least 64.  Tests and diagnostics. */
int tnml_set_input_grad_chunk(tnml_ctx *ctx, int samples);

/* ---- core gradients -------------------------------------------------------------------------- */
/* The gradient with respect to the parameters themselves, all N cores in one call: what gradient descent over all cores, Adam in a
 * host framework, one-site updates, a fine-tuning pass after sweeping or a sensitivity analysis need.  No reference analogue.
 *   G_i[a][d][c]     = sum_s P_i[s][a] x_i[s][d] Q_i[s][c]                      (i != l_pos)
 *   G_l[a][d][c][l'] = sum_s cot[l'][s] P_l[s][a] x_l[s][d] Q_l[s][c]           (i == l_pos)
 * the derivative of sum_s cf[s], cf[s] = sum_l' cot[l'][s] f[l'][s], with P and Q the two per-sample chains of the input
 * gradients.  A chain kernel stores both chains to HBM, a reduction kernel sums over the samples on the matrix cores, one fixed
 * left-to-right sum per element: the result does not depend on the chunk size (csrc/kernels_coregrad.hip).
 * RANGE and LIMITS: those of the input gradients above (calibrated networks; single GPU; a shape whose LDS tiles need more than
 * 160 KB is refused with TNML_ERR_ARG and a message naming the bytes).  Every refusal happens before anything is launched.
 * X [b][N][D], cot [L][b] or NULL (= one-hot of the first maximum of f per sample), grad_flat in the layout of tnml_get_cores (the
 * cores follow one another, each (ml, D, mr) row-major, the core on l_pos (ml, D, mr, L)), capacity in floats, at least
 * tnml_cores_size (TNML_ERR_ARG otherwise; floats behind the gradient are left alone), cf_out [b] or NULL.  Any l_pos, with or
 * without tnml_set_any_position.  b may exceed every batch capacity: the call works in chunks (tnml_set_core_grad_chunk).  It
 * leaves the resident batch, its environments, f, the cores, l_pos and the input-gradient buffers exactly as they were, and it
 * synchronises before returning. */
int tnml_core_grad(tnml_ctx *ctx, const float *X, int b, const float *cot, float *grad_flat, size_t capacity, float *cf_out);
/* the same for samples of the attached dataset */
int tnml_core_grad_indices(tnml_ctx *ctx, const int32_t *idx, int b, const float *cot, float *grad_flat, size_t capacity, float *cf_out);
/* samples per pass (rounded up to a multiple of 64); 0 = default: the largest multiple of 64 for which each of the two stacks of
 * stored environments (N x bond capacity x samples floats) stays within 256 MiB, at least 64.  Tests and diagnostics. */
int tnml_set_core_grad_chunk(tnml_ctx *ctx, int samples);

/* ---- gradient training over all cores --------------------------------------------------------- */
/* Optimiser steps on the device from the core gradients above (csrc/kernels_optim.hip): whole-chain gradient
 * descent at fixed bonds, at any l_pos, without an SVD -- the companion of the two-site sweep (sweep to find the bonds, then
 * fine-tune).  No reference analogue.  Per batch: the prediction chain, the metrics of the batch BEFORE the step, the library's own
 * loss derivative (compute_loss_derivate of apply_act_func, all nine activation / loss pairs) as the cotangent, the core gradients
 * G, then one update of every core in its slot.  The loss derivative is the descent direction, so the update ADDS:
 *   TNML_OPT_SGD   d = G - wd A;  clip: per core, if sum|d| > sum|A| then d *= sum|A| / sum|d| (the reference's rule for the merged
 *                  tensor, applied to each core);  momentum mu > 0: vel = mu vel + d, A += lr vel;  mu == 0: A += lr d (no state)
 *   TNML_OPT_ADAM  t += 1; m = b1 m + (1 - b1) G; v = b2 v + (1 - b2) G G;
 *                  A += lr ((m / (1 - b1^t)) / (sqrt(v / (1 - b2^t)) + eps) - wd A)          (decoupled decay; no clip)
 * in float64 from the float32 G, rounded once on the store; sum|.| in float64 in a fixed order.
 * tnml_optim_config: momentum in [0, 1), betas in [0, 1), eps > 0, clip 0 / 1 (TNML_ERR_ARG otherwise, and for ADAM with clip != 0).
 * Default: SGD, momentum 0, betas 0.9 / 0.999, eps 1e-8, clip 1.  It also does what tnml_optim_reset does.
 * STATE: vel / m / v are device buffers in the layout of tnml_get_cores, allocated on the first step of a stateful optimiser and
 * bound to the bonds and l_pos of that step (or of the last tnml_optim_reset / tnml_optim_config).  A step at other bonds or another
 * l_pos -- after a sweep, say -- returns TNML_ERR_STATE until tnml_optim_reset, which zeroes the state, sets t = 0 and binds it to
 * the current bonds and l_pos.  SGD without momentum has no state and is never refused for this reason. */
enum { TNML_OPT_SGD = 0, TNML_OPT_ADAM = 1 };
int tnml_optim_config(tnml_ctx *ctx, int kind, double momentum, double beta1, double beta2, double eps, int clip);
int tnml_optim_reset(tnml_ctx *ctx);
/* n_steps = ceil(n / batch) optimiser steps from the attached dataset: step k uses the samples idx[k * batch .. min((k + 1) * batch, n)).
 * metrics_out [n_steps][3] = (correct, sum |onehot - act(f)|, non-finite samples) of each batch BEFORE its step, or NULL.
 * The index list and the tables are uploaded once, every step is enqueued without waiting, and the call synchronises once at the
 * end.  A batch may exceed every buffer: it is worked in the chunks of tnml_set_core_grad_chunk, and the updated cores do not
 * depend on the chunk size.  If a step saw a non-finite activated output the call returns TNML_ERR_NONFINITE after all steps ran:
 * the cores are then what they became (as after a diverged sweep: set them again); metrics_out is filled all the same.
 * AFTER a call the context is as after tnml_scale_cores: the cores changed, so the environments, f and the norm environments of
 * the resident batch are stale -- tnml_sweep returns TNML_ERR_STATE until a tnml_forward; the resident batch and its labels stay.
 * REFUSALS, all before anything is launched: NULL pointers, n < 1, batch < 1, an index outside the dataset, unknown act_fn /
 * loss_fn, a shape beyond the LDS limit of the core gradients or more labels than the metrics kernel's tile holds -> TNML_ERR_ARG;
 * no dataset, cores never set, a communicator attached, state bound to other bonds -> TNML_ERR_STATE. */
int tnml_gd_train_indices(tnml_ctx *ctx, const int32_t *idx, int n, int batch, float lr, float weight_dec, int act_fn, int loss_fn,
                          float T, double *metrics_out);
/* one step on a host batch X [b][N][D], y [b] (labels outside [0, L): TNML_ERR_ARG); metrics3 [3] or NULL */
int tnml_gd_step(tnml_ctx *ctx, const float *X, const int32_t *y, int b, float lr, float weight_dec, int act_fn, int loss_fn, float T,
                 double *metrics3);

/* ---- range-safe chains ------------------------------------------------------------------------- */
/* The chains of the prediction and gradient calls are float32 products over all sites.  A network whose f is of order 1 may still
 * have partial products over a few hundred sites that leave float32 (after Adam, weight decay or a change of gauge moved the size
 * of single cores); the calls then return inf, nan or a silent 0.  With this switch on every sample carries a power-of-two exponent
 * along its chains: after the product of every site the sample's column is multiplied by exactly 2^-k, k = ilogb(max |.|) + 1
 * (k = 0 where that maximum is 0 or not finite), and k joins the sample's int32 exponent.  The scaling is exact, so wherever the
 * plain chain stays in range the results agree with it to rounding-order effects of the compiler only.
 * on = 1: tnml_predict, tnml_predict_indices, tnml_eval_indices, tnml_input_grad(_indices), tnml_core_grad(_indices), tnml_gd_step
 * and tnml_gd_train_indices (and the prediction behind a NULL cot) run scaled chains; their plain outputs receive
 * ldexpf(mantissa, exponent) with IEEE saturation and flush, so an f that itself lies outside float32 still reads inf or 0 there:
 * read such an f with tnml_predict_scaled.  The resident batch, its environments, the sweep, tnml_forward,
 * tnml_forward_logabsmax and the orthogonalisation calls are untouched.  Default 0: every launch and buffer is what it was.
 * on outside {0, 1}: TNML_ERR_ARG.  The refusals of the calls themselves (communicator, LDS limit) are unchanged. */
int tnml_set_chain_scaling(tnml_ctx *ctx, int on);
/* f of a batch that is NOT made resident, as mantissa and exponent: X [b][N][D] -> mant_out [L][b], expo_out [b] with
 * f[l][s] = mant[l][s] * 2^expo[s] and 0.5 <= max_l |mant[l][s]| < 1 per sample.  Where every f[:, s] is 0 or one of them is not
 * finite, expo[s] = 0 and mant holds the values as they are.  Works with the switch above on or off, at any label position
 * tnml_predict accepts, and refuses what tnml_predict refuses (plus a shape beyond the 160 KB LDS limit of the kernel:
 * TNML_ERR_ARG with the bytes).  This is how the output of an un-calibrated network (about 1e-66 at N = 784) is read and its
 * argmax taken. */
int tnml_predict_scaled(tnml_ctx *ctx, const float *X, int b, float *mant_out, int32_t *expo_out);

/* Accuracy / speed of the in-kernel Jacobi SVD (no reference analogue: the reference calls LAPACK,
 * Network_class.py:887).  The iteration ends after a sweep in which every rotation had
 * g^2 <= stop2 * scale^2; the off-diagonals left behind are of relative size ~stop2.  Default 1e-6
 * (truncated product within ~6e-6 max|B| of LAPACK's); 1e-4 saves about one sweep in five and leaves ~2e-4;
 * 1e-8 costs one more and reaches ~1e-6.  Allowed range [1e-12, 1e-2]. */
int tnml_set_svd_stop(tnml_ctx *ctx, double stop2);

/* A sweep step is ONE launch by default: workgroup 0 updates and splits the merged tensor of step k while the other
 * workgroups of the same launch form f of step k and the batch-summed pre-gradient of step k+1.
 * on = 0 restores the classic sequence (batch kernel -> [reduction] -> update/SVD kernel), which is also what steps
 * whose merged tensor does not fit one workgroup's LDS take.  Results agree to float32 rounding.
 * on >= 2: number of 32-sample tiles a batch-side workgroup accumulates before it writes its partial pre-gradient on steps
 * whose SVD is long enough to hide that (short side >= 32); on = 1 means the default, 2. */
int tnml_set_step_pipeline(tnml_ctx *ctx, int on);

/* A FULL sweep (n_steps = N-1 right after tnml_forward) on a single GPU under the fixed or the reference truncation is ONE launch by
 * default: a persistent kernel whose update workgroup, helper workgroup and batch-side workgroups each loop over the N-1 steps and
 * hand their results to each other through flags in memory.  Sweeps it does not cover (partial sweeps, a
 * communicator, adaptive truncation, per-step capture, merged tensors beyond one workgroup's LDS) take one launch per step as
 * before.
 *   on = 1 (default)  the three roles in ONE launch
 *   on = 2            the three roles as three launches on three streams of the context, resident together (each role with its own
 *                     register allocation; measured equal to on = 1 within 2 %); a tool that SERIALISES launches (rocprofv3 --pmc)
 *                     keeps them from meeting: the bounded waits then time out and tnml_sweep fails with TNML_ERR_STATE
 *   on = 0            one launch per step everywhere */
int tnml_set_persistent(tnml_ctx *ctx, int on);
/* The one-launch persistent sweep (tnml_set_persistent 1) is also compiled for the step shapes of its table (bond 10 and 20 at two
 * labels, D = 2): a step whose behind, ahead, shared and kept bond all equal that bond runs a body with the shape as compile-time
 * constants, every other step (the bond ramps at the chain ends, any other bond or label count) the generic body.  Same results, bit
 * for bit.  on = 1 (default) / 0: mark such steps or run the generic body everywhere. */
int tnml_set_shape_kernels(tnml_ctx *ctx, int on);
/* *n_steps = steps of the last persistent sweep that ran a body compiled for their shape (0: none, switch off, or mode 2) */
int tnml_fixed_shape_steps(tnml_ctx *ctx, int *n_steps);
/* How the batch-side workgroups of a persistent sweep (both modes) sum their partial pre-gradients where one workgroup's LDS does not
 * hold sixteen of them (bond 20 at two labels: 6400 floats per partial):
 *   mode = 1 (default)  in slices: every workgroup counts its arrival, the first R workgroups each sum runs of 16 16-byte elements
 *                       over all partials and count themselves done, the helper workgroups wait for R
 *   mode = 0            by last arrivers: the last of each group of sixteen sums its group, the last group sums the group sums
 * Same summation tree, same results bit for bit.  Smaller pre-gradients take one level through one workgroup's LDS either way, and
 * per-step launches always reduce by last arrivers. */
int tnml_set_persist_reduce(tnml_ctx *ctx, int mode);
/* *n_steps = batch-side iterations of the last persistent sweep that reduced in slices (0: none, or mode 0) */
int tnml_slice_reduce_steps(tnml_ctx *ctx, int *n_steps);

/* tnml_sweep enqueues every launch of its n_steps steps without waiting (2 - 14 launches per step).  A profiler that
 * intercepts dispatches (rocprofv3 --pmc serialises them and keeps per-dispatch state) can be overrun by tens of
 * thousands of queued launches; n_steps > 0 drains the stream every n_steps steps, 0 never.  Default 256: at most ~3600
 * dispatches outstanding on the large-tensor path, one host round trip per 14 ms of a C3 sweep (the persistent sweep is one
 * launch and never drains). */
int tnml_set_sync_interval(tnml_ctx *ctx, int n_steps);

/* The batch-independent part of a step (update_B's tail, compute_L2_reg, tensor_svd) runs in one
 * workgroup's LDS when the merged tensor fits (min(rows, cols) <= 64 and <= 160 KB of LDS: bond <= 32 at
 * two labels) and through HBM-resident kernels otherwise (min(rows, cols) <= 128: bond 50 with ten labels).
 * LIMIT: the Jacobi kernels take a short side of at most 128, i.e. bond dimension M <= 64 at D = 2 (128 / D in general); tnml_sweep
 * returns TNML_ERR_ARG at the first step beyond it (the reference itself has no such limit; its largest published
 * bond is 50).
 * force_large = 1 sends every step down the second path (tests, diagnostics); 0 restores the automatic
 * choice. */
int tnml_set_narrow_path(tnml_ctx *ctx, int force_large);

/* The hand-offs between the context's two streams (pipelined large-tensor step; update side / batch side + all-reduce of the communicator
 * path) are sequence numbers in memory by default: the consuming kernel, or a one-wave gate kernel in front of it, polls the word a
 * one-thread signal kernel (or the producing workgroup itself) stores -- an event dependency costs the stream that records or waits
 * 6-7 us even when it is satisfied.  Every waiting kernel is enqueued after the kernels it waits for and its wait is bounded
 * (TNML_ERR_STATE on a time-out), but a tool that lets only ONE kernel run at a time (rocprofv3 --pmc serialises dispatches) keeps the
 * producer from ever starting: on = 0 (or the environment variable TNML_EVENT_HANDOFFS=1 at tnml_create) uses events everywhere. */
int tnml_set_flag_handoffs(tnml_ctx *ctx, int on);

/* The forward environment chain (Network.forward, Network_class.py:227-255) runs on the matrix cores for bond dimensions
 * <= 32 (one wave per 16 samples) and as plain FMAs otherwise and in the renormalising calibration pass.  force_plain = 1
 * sends every chain down the plain-FMA kernel (tests, diagnostics); 0 restores the automatic choice. */
int tnml_set_chain_path(tnml_ctx *ctx, int force_plain);

/* TNML_TRUNC_ADAPTIVE (not reference behaviour): tensor_svd computes the cumulative share of the singular
 * values and the first index where it exceeds `threshold` (Network_class.py:889-891, default argument
 * 0.999) but never uses it.  Under this policy the kept rank is min(M, index + 1), decided on the device
 * from the full spectrum; tnml_sweep then synchronises once per step to learn the new bond dimension. */
int tnml_set_trunc_threshold(tnml_ctx *ctx, double threshold);

/* Network.apply_act_func / compute_loss_derivate on the device-resident f (:767-835);
 * act_out, lossder_out [L][b], either may be NULL.  input_is_activated != 0: f already went
 * through the activation (what compute_loss_derivate receives, :800), only the derivative runs. */
int tnml_activation(tnml_ctx *ctx, int act_fn, int loss_fn, float T, int input_is_activated,
                    float *act_out, float *lossder_out);

/* ---- inspection (API parity: Network.r_cum_contraction / l_cum_contraction) -------------- */
int tnml_get_env(tnml_ctx *ctx, int side, int site, float *out, size_t capacity, int *m);
/* bit 0: capture B, dB, B_new, sigma of every step into a debug block (tests only; off by default);
 * bit 1: in-kernel cycle stamps only; bit 2: read the launch status back after every kernel launch of a step
 * (a failed launch then names its kernel; launch geometry is validated before every launch regardless) */
int tnml_debug_enable(tnml_ctx *ctx, int on);
int tnml_get_step_debug(tnml_ctx *ctx, int what, double *out, size_t capacity, size_t *n);
int tnml_l_pos(tnml_ctx *ctx);
int tnml_batch(tnml_ctx *ctx);

/* ---- measurement ------------------------------------------------------------------------ */
/* HIP-event timing on the context's own stream (torch.cuda.Event would not see it) */
int tnml_timer_start(tnml_ctx *ctx);
/* phase boundary visible to a profiler: an empty kernel `tnml_phase_marker_kernel` of `id` workgroups of 64 threads (1 <= id <=
 * 1024) on the context's stream; bench.py brackets its warm-up / timed / resident / cold passes with it and
 * tools/rocprof_summary.py cuts kernel traces and counter passes to the window between two markers */
int tnml_marker(tnml_ctx *ctx, int id);
int tnml_timer_stop(tnml_ctx *ctx, double *elapsed_ms);
/* tnml_profile_enable(ctx, 1): accumulated per-kernel device time (ms) and launch counts since the last reset, measured
 * with HIP events around each launch (synchronises after every launch: slows the sweep; break-downs only)
 *   which: 0 forward chain, 1 batch-side kernel (classic wide kernel / prologue of the pipelined step), 2 reduce kernel,
 *          3 update+SVD kernel (classic narrow kernel / the single launch of a pipelined step)
 * tnml_profile_enable(ctx, 2): one HIP event pair per tnml_sweep call, nothing waits inside the timed region
 *   which: 4 -> ms between first and last launch of all sweeps since the reset, launches = kernel launches they made
 *          5 -> the same ms, launches = number of pipelined steps among them (single-launch steps and large-tensor steps that
 *               took their gradient from the pre-gradient the previous step's side stream left) */
int tnml_profile_enable(tnml_ctx *ctx, int on);
int tnml_profile_get(tnml_ctx *ctx, int which, double *ms, long long *launches);
int tnml_profile_reset(tnml_ctx *ctx);
/* Work done since the last tnml_profile_reset, computed from the dimensions of every step that ran:
 *   out8 = {sweep steps, algorithmic bytes of those steps (4 b (2h + g + 3D + 2L + 1) each: environments, features, f, labels),
 *           algorithmic flops (4 b D^2 h g L + 2 b D h^2 each), forward calls, algorithmic bytes of those forwards,
 *           kernel launches of the sweeps, pipelined steps among them (single-launch steps + large-tensor steps fed by Z),
 *           device ms inside the sweeps (0 unless tnml_profile_enable(ctx, 2) was on; read it through tnml_profile_get(4) first)} */
int tnml_get_counters(tnml_ctx *ctx, double *out8);
/* always-on counters of the SVD since the last reset: out3 = {Jacobi sweeps, number of SVDs, Jacobi rounds (one barrier each)} */
int tnml_svd_stats(tnml_ctx *ctx, int reset, double *out3);
/* the same with a capacity: out[0..capacity) of {sweeps, SVDs, rounds, SVDs that took the pivoted-Cholesky step}; entries beyond
 * the fourth are left untouched */
int tnml_svd_stats_ex(tnml_ctx *ctx, int reset, double *out, int capacity);

/* ---- orthogonal form about the label, compression, bond spectra ------ */
/* ("canonical" names the array layout (ml, D, mr[, L]) in this library; the gauge is called orthogonal form.)
 * Float64 inside, float32 cores in and out, the label site l = l_pos stays where it is.  tnml_orthogonalize rewrites the cores so that
 * every core left of l, as a (ml D) x mr matrix, is g Q with Q^T Q = 1, every core right of l, as ml x (D mr), is g Q with Q Q^T = 1,
 * and the label core is g C with |C|_F = 1; g = exp(log|W| / N) is shared by all N cores, f(x) is unchanged, log|W| (natural log of
 * the chain's norm) goes to *log_norm_out.  Every bond is decomposed with the orthogonality centre on it and shrinks to its Schmidt
 * rank: directions with sigma_j <= rank_tol * sigma_1 are dropped (the arithmetic resolves no direction below 3e-8 sigma_1: a
 * smaller rank_tol acts as that), so a second call keeps every bond.
 * tnml_compress additionally cuts every bond to min(m_max, adaptive rank at `threshold`) -- the rule of TNML_TRUNC_ADAPTIVE on the
 * bond's Schmidt spectrum, threshold = 1 disables it -- with the orthogonality centre on the bond at the moment it is cut and earlier
 * cuts applied.  sigma_out [N-1][Mcap] (Mcap = the context's bond capacity, max(M, D min(L, M))) receives every bond's normalised
 * spectrum before the cut (sum sigma^2 = 1, zero-padded), discarded_out [N-1] the weight sum_{j > m} sigma_j^2 that was cut,
 * log_norm_out the log-norm of the compressed chain.  tnml_bond_spectra computes the same spectra, ranks and log-norm on a scratch
 * copy: cores, bonds and every piece of state stay bit for bit.
 * bond_out / rank_out [N-1].  A committed call leaves the context in the state tnml_scale_cores leaves (the resident batch and its
 * labels stay, a tnml_forward is needed before a sweep) with every slot float behind the new core zero, and unbinds the optimiser
 * state (tnml_optim_reset before the next stateful step).  A call that fails -- TNML_ERR_ARG (NULL output, m_max < 1, threshold
 * outside (0, 1], rank_tol outside [0, 1)), TNML_ERR_STATE (cores never set, communicator attached), TNML_ERR_SHAPE (a bond the
 * kernel's LDS has no room for), TNML_ERR_NONFINITE (a core element that is not finite or beyond 1.8e19 in magnitude, a zero chain,
 * a result beyond float32), TNML_ERR_HIP -- leaves cores, bonds and l_pos as they were. */
int tnml_orthogonalize(tnml_ctx *ctx, double rank_tol, int32_t *bond_out, double *log_norm_out);
int tnml_compress(tnml_ctx *ctx, int m_max, double threshold, double rank_tol, int32_t *bond_out, double *sigma_out,
                  double *discarded_out, double *log_norm_out);
int tnml_bond_spectra(tnml_ctx *ctx, double rank_tol, int32_t *rank_out, double *sigma_out, double *log_norm_out);

/* ---- inner products and linear combinations of two MPS --------------- */
/* W is the context's chain, V a second chain with the same N, D, L and the same label position, handed in as other_flat / other_bond
 * in the layout of tnml_get_cores; its bonds are free.  With a symmetric float64 metric S_i per site (metric NULL: the identity;
 * metric_sites 1: one [D][D] for all sites; metric_sites N: [N][D][D]; the label axis is always contracted with the identity)
 *   <W|V>_S = sum W[d_0 .. d_{N-1}, l'] V[d'_0 .. d'_{N-1}, l'] prod_i S_i[d_i, d'_i],
 * computed in float64 from the float32 cores by two transfer half-chains that meet on the label site.  After every site the transfer
 * matrix is multiplied by an exact power of two that joins an integer exponent, so nothing leaves the range at N = 784 whatever the
 * cores' scale.  out6 = {sign, log|.|} of <W|W>, <V|V>, <W|V>; a zero product gives (0, -inf).  other_flat NULL: only <W|W> (the
 * other four entries 0 and -inf).  The three products run the same instructions in the same order: a V bit-equal to W gives three
 * bit-equal pairs, and two calls on the same cores are bit-equal.  tnml_inner changes nothing on the device (bit for bit, as
 * tnml_bond_spectra); no forward is needed afterwards.
 * tnml_axpby: W <- alpha W + beta V as the direct sum: every bond becomes mW_i + mV_i (bond_out [N-1]), interior cores are
 * block-diagonal per d (and per l' on the label site), site 0 is a row concatenation, site N-1 a column stack; alpha and beta multiply
 * the label-site blocks only, in float64 with one rounding per element.  It commits as tnml_compress does: the state
 * tnml_scale_cores leaves, every slot float behind the new core zero, the optimiser state unbound.
 * A call that fails leaves cores, bonds and l_pos as they were; all of these happen before anything is launched:
 * TNML_ERR_ARG (NULL output; n_floats not what the bonds imply; a bond < 1; other_l_pos != l_pos; metric_sites not 1 or N; a
 * non-finite alpha or beta; for tnml_axpby a NULL other_flat or a summed bond above the context's bond capacity), TNML_ERR_STATE
 * (cores never set; a communicator attached), TNML_ERR_SHAPE (the transfer matrix of the two largest bonds does not fit the
 * kernel's LDS; the message names the bytes).  TNML_ERR_NONFINITE: a core element that is not finite (tnml_inner), a result element
 * that is not a finite float32 (tnml_axpby). */
int tnml_inner(tnml_ctx *ctx, const float *other_flat, size_t n_floats, const int32_t *other_bond, int other_l_pos,
               const double *metric, int metric_sites, double *out6);
int tnml_axpby(tnml_ctx *ctx, double alpha, double beta, const float *other_flat, size_t n_floats,
               const int32_t *other_bond, int other_l_pos, int32_t *bond_out);

/* ---- samples and log-likelihoods of the Born distribution ------------- */
/* Over a pixel grid of K levels (2 <= K <= 256) with feature vectors phi [K][D] and positive weights w [K] the chain defines
 *   p(k_0 .. k_{N-1}, l) = prod_i w[k_i] f_l(phi[k_0], .., phi[k_{N-1}])^2 / Z,     Z = <W|W>_S,  S = sum_k w_k phi_k phi_k^T.
 * tnml_sample draws n exact samples from it in one pass over the chain, without rejection, in float64 from the float32 cores:
 * metric environments R_i from the right (one stack per class a call conditions on, one with the label summed; each multiplied
 * by an exact power of two per site), then per sample and site the K densities w_k phi_k^T Q phi_k, their running sums c_k and
 * the smallest k with c_k > u_i c_{K-1} (the last k of positive density if there is none).
 * classes [n]: -1 draws the label on the label site from P(l | levels before it), by u[N] and the same rule, and its log joins
 * logp; a class c conditions on it: the sample comes from p(. | c) and no label term enters logp.  classes NULL: all -1.
 * given [n][n_given]: the first n_given sites are clamped to these levels instead of drawn.  u [n][N+1] in [0, 1): the uniforms
 * (column N for the label); u NULL: the device generates u[s][j] as SplitMix64 of seed + (s (N+1) + j + 1) 0x9E3779B97F4A7C15,
 * top 53 bits times 2^-53, so that a seeded call can be repeated anywhere.
 * levels_out [n][N], labels_out [n] (the given class where there is one), logp_out [n][2]: [0] the log-probability of all levels
 * [and the drawn label] [given the class], [1] the sum of the terms of the clamped sites alone -- with the label site outside
 * the prefix, or a given class, [0] - [1] is the log-density of the completion given the prefix.  n_given = N is a likelihood
 * call: nothing but a label is drawn.  For known sites other than a prefix see tnml_sample_masked below.
 * Every sum runs in a fixed order: two calls with the same arguments are bit-equal.  Nothing else on the device changes (cores,
 * bonds, l_pos, the resident batch, f, the environments and the optimiser binding stay bit for bit); no forward is needed afterwards.
 * Refused before anything is launched: TNML_ERR_ARG (n < 1; K outside [2, 256]; a class outside [-1, L); a given level outside
 * [0, K); n_given outside [0, N]; a weight that is not positive and finite, a non-finite phi, a u outside [0, 1); a NULL phi, w or
 * output, a NULL given with n_given > 0), TNML_ERR_STATE (cores never set; a communicator attached), TNML_ERR_SHAPE (a bond above
 * 64, or LDS: the message names the bytes).  After the run: TNML_ERR_NONFINITE (a core element that is not finite), TNML_ERR_ARG
 * naming the sample and its class when a sample is conditioned on a class or a prefix of zero weight. */
int tnml_sample(tnml_ctx *ctx, int n, int K, const double *phi, const double *w, const int32_t *classes, const int32_t *given,
                int n_given, const double *u, uint64_t seed, int32_t *levels_out, int32_t *labels_out, double *logp_out);

/* ---- the same given ANY set of known pixels ---------------------------- */
/* mask [mask_rows][N] (mask_rows 1: shared by all samples, or n): site i of sample s is KNOWN where it is non-zero, and its level is
 * known [n][N] there (entries at other sites are ignored, whatever they hold; known may be NULL when no mask bit is set).  Every
 * sample has metric environments of its own from the right, with w_k phi_k phi_k^T in place of S on its known sites, each multiplied
 * by a power of two per site whose exponents are summed: E_s = log R_{s,0} + ln2 sum.  The same kernel computes, as one more row
 * with the empty mask, the normaliser of every class slot the call needs.
 * draw = 1: the walk of tnml_sample with the sample's own environments; nothing is drawn on a known site.  levels_out [n][N] holds
 * the known levels as given and the drawn ones elsewhere, labels_out [n] the given class or the drawn label, logp_out [n][2]:
 *   [0] log p(drawn levels [, drawn label] | known levels [, class]),
 *   [1] log p(known levels [| class])   (class -1: the marginal over the label; exactly 0 for an empty mask).
 * draw = 0: only the environments run; [1] as above, [0] = 0, labels_out (if not NULL) the given classes, levels_out may be NULL.
 * class_logw_out [L] or NULL: log P(c), -inf for a class of zero weight.  u, seed: as tnml_sample (the hash takes the call's sample
 * number).  The stack of environments, (N + 1) m^2 doubles a sample at largest bond m, is filled in chunks of whole tiles that stay
 * within tnml_set_sample_stack_bytes (default 1 GiB); no result depends on the chunking, on the tile size or on the other samples
 * of the call.  Every sum runs in a fixed order.  Nothing else on the device changes, as for tnml_sample.
 * Refused before anything is launched: the list of tnml_sample, and TNML_ERR_ARG for mask_rows neither 1 nor n, a NULL mask, a NULL
 * known with a mask bit set, a known level outside [0, K) at a masked site, draw with a NULL levels_out or labels_out, a NULL
 * logp_out, a stack budget below one tile's need; TNML_ERR_STATE (cores never set; a communicator attached); TNML_ERR_SHAPE (a bond
 * above 64, or LDS: the message names the bytes).  After the run: TNML_ERR_NONFINITE as tnml_sample; TNML_ERR_ARG naming the smallest
 * sample, and its class, whose known pixels (or class) have zero weight. */
int tnml_sample_masked(tnml_ctx *ctx, int n, int K, const double *phi, const double *w, const int32_t *classes, const uint8_t *mask,
                       int mask_rows, const int32_t *known, const double *u, uint64_t seed, int draw, int32_t *levels_out,
                       int32_t *labels_out, double *logp_out, double *class_logw_out);
/* bytes of the environment stack a chunk of tnml_sample_masked may take (0: TNML_ERR_ARG) */
int tnml_set_sample_stack_bytes(tnml_ctx *ctx, size_t bytes);

/* ---- per-pixel conditionals ------------------------------------------- */
/* What the model believes about every single pixel given the pixels it was shown.  n, K, phi, w, classes, mask, mask_rows and known
 * are tnml_sample_masked's, and so are the per-sample environments R_{s,i} from the right.  A second walk carries the matching
 * environment from the left, Lf_{s,0} = 1,
 *   Lf_{s,i+1}[c,c'] = sum_{a,a',d,d'} Lf_{s,i}[a,a'] S_{s,i}[d,d'] A_i[a,d,c] A_i[a',d',c']
 * (label slices as on the right, an exact power of two per site whose exponent is discarded), and meets R_{s,i+1} at every site in
 * the one-site matrix that leaves out the site's own metric:
 *   Q_{s,i}[d,d'] = sum_{a,a',c,c'} Lf_{s,i}[a,a'] A_i[a,d,c] R_{s,i+1}[c,c'] A_i[a',d',c']
 *   p_{s,i}(k)    = max(0, w_k phi_k^T Q_{s,i} phi_k) / tr(S Q_{s,i})
 * = p(x_i = k | the known pixels other than i [, class]): the posterior marginal of a free site, the leave-one-out conditional of a
 * known one, by one code path.
 * values [K] or NULL: the number each level stands for in the mean and the variance (NULL: the level index).
 * q_out [n][N][D][D]: Q / tr(S Q).  stats_out [n][N][4]: the mean sum_k p(k) values[k]; the variance sum_k p(k) (values[k] - mean)^2;
 * the entropy -sum_k p(k) log p(k) (a zero density adds nothing); log p(k_s[i]) on a known site and 0 on a free one.
 * mode_out [n][N]: the first k of largest density.  logp_out [n]: log p(known levels [| class]), column 1 of tnml_sample_masked with
 * draw = 0, bit for bit.  Each output may be NULL, not all of them.
 * Chunks, the stack budget and the class-slot tiles are tnml_sample_masked's; the tile is the largest of 16, 8, 4, 2, 1 at which both
 * kernels of this call fit 160 KB of LDS, and no result depends on it, on the chunking or on the other samples.  Every sum runs in a
 * fixed order.  Nothing else on the device changes, and no forward is needed afterwards.
 * Refused before anything is launched: the list of tnml_sample_masked (without its output and uniform rules), and TNML_ERR_ARG when
 * every output is NULL or a value is not finite; TNML_ERR_SHAPE for a bond above 64 (TNML_SITE_COND_MAX_BOND), or LDS: the message
 * names the bytes.  After the run: the errors of tnml_sample_masked. */
#define TNML_SITE_COND_MAX_BOND 64
int tnml_site_conditionals(tnml_ctx *ctx, int n, int K, const double *phi, const double *w, const double *values,
                           const int32_t *classes, const uint8_t *mask, int mask_rows, const int32_t *known,
                           double *q_out, double *stats_out, int32_t *mode_out, double *logp_out);

/* ---- pixel-pair marginals --------------------------------------------- */
/* The joint marginal of every pair of pixels, exactly and without sampling.  K, phi, w and values are tnml_site_conditionals';
 * S = sum_k w_k phi_k phi_k^T.  class_slot -1: the label is summed; q >= 0: slice q of the label site alone, and everything is
 * conditional on that class.  With L_i, R_i the metric environments of tnml_log_norm_grad for S (and the class slot):
 *   B_j[e,e'][a,a']      = sum_{c,c'} A_j[a,e,c] R_{j+1}[c,c'] A_j[a',e',c']
 *   q1_j[e,e']           = sum_{a,a'} L_j[a,a'] B_j[e,e'][a,a'] / tr(S q1_j)
 *   C_i,i+1[d,d'][c,c']  = sum_{a,a'} L_i[a,a'] A_i[a,d,c] A_i[a',d',c']
 *   C_i,j+1[d,d'][c,c']  = sum S[e,e'] A_j[a,e,c] C_i,j[d,d'][a,a'] A_j[a',e',c']             (j > i)
 *   Q_ij[d,d'][e,e']     = sum_{a,a'} C_i,j[d,d'][a,a'] B_j[e,e'][a,a'],   q_ij = Q_ij / sum S[d,d'] S[e,e'] Q_ij[d,d'][e,e']
 *   p_ij(k,k')           = max(0, w_k w_k' sum phi_k[d] phi_k[d'] q_ij[d,d'][e,e'] phi_k'[e] phi_k'[e'])
 * = p(x_i = k, x_j = k' [| class]).  Every C matrix is multiplied by an exact power of two after every site; the exponents of the
 * D^2 matrices of a row are brought together before q_ij is normalised and none survives.
 * rows [n_rows]: distinct sites.  Row r covers the pairs (rows[r], j), j > rows[r]; entries with j <= rows[r] are written as 0.
 * q1_out [N][D][D].  stats1_out [N][3]: mean, variance and entropy of p_i(k) = max(0, w_k phi_k^T q1_i phi_k) over values.
 * q_out [n_rows][N][D^2][D^2]: q_ij, indexed [(d,d')][(e,e')].  stats_out [n_rows][N][3]: with p_i, p_j the marginals summed from
 * the clamped table p_ij and their means and variances over values, the covariance sum p_ij(k,k') values[k] values[k'] -
 * mean_i mean_j; the correlation, covariance over the two standard deviations, 0 where a variance is 0; the mutual information
 * sum p_ij log(p_ij / (p_i p_j)) in nats, formed as sum p_ij log p_ij - sum p_i log p_i - sum p_j log p_j (a zero density adds
 * nothing).  Each output may be NULL, not all of them; with n_rows = 0 only the per-site part runs.
 * Rows run in ascending site order in chunks whose buffers stay within tnml_set_sample_stack_bytes; a row's result depends neither
 * on the other rows nor on the chunking.  Every sum runs in a fixed order: two calls are bit-equal.  Nothing else on the device
 * changes, and no forward is needed afterwards.
 * Refused before anything is launched: TNML_ERR_ARG (a NULL ctx, phi or w; K outside [2, 256]; a weight not positive and finite; a
 * grid point or a value not finite; class_slot outside [-1, L); n_rows < 0; rows NULL with n_rows > 0; a row outside [0, N) or
 * repeated; every output NULL, or only pair outputs with n_rows = 0; a budget below one row's need); TNML_ERR_STATE (cores never
 * set; a communicator attached); TNML_ERR_SHAPE for a bond above 64 (TNML_PAIR_MAX_BOND), or LDS: the message names the bytes.
 * After the run: TNML_ERR_NONFINITE for a non-finite environment, Z == 0, or a marginal whose normaliser is zero or not finite. */
#define TNML_PAIR_MAX_BOND 64
int tnml_pair_marginals(tnml_ctx *ctx, int K, const double *phi, const double *w, const double *values, int class_slot,
                        const int32_t *rows, int n_rows, double *q1_out, double *stats1_out, double *q_out, double *stats_out);

/* ---- the gradient of the log-norm ------------------------------------ */
/* grad_flat receives Gz_i = d log|<W|W>_S| / d A_i for every core, in the layout of tnml_get_cores (capacity in floats, at least
 * tnml_cores_size; floats behind the gradient are left alone), and sign_log2 [2] = {sign of <W|W>_S, log|<W|W>_S|}, the pair
 * tnml_inner returns (for an indefinite metric the sign may be -1; the gradient is that of log|.| either way).  S: NULL for the
 * Euclidean product, else a symmetric float64 metric, [D][D] for every site (per_site 0) or [N][D][D] (per_site 1); the label axis
 * is contracted with the identity.  With S = sum_k w_k phi_k phi_k^T of a pixel grid <W|W>_S is the normaliser Z of tnml_sample,
 * and Gz is the model term of every likelihood gradient.
 * Computed in float64 from the float32 cores: both metric environments of every site, each multiplied by an exact power of two
 * after every site and stored with its running exponent, then per site L_i . (S A_i) . R_{i+1} scaled by 2 / <W|W>_S, the power of two
 * applied by ldexp, one rounding to float32 per element.  sum(Gz_i A_i) = 2 at every site, and Gz is of order 1 / |A_i|: it is a
 * float32 for the un-calibrated 784-site chain whose <W|W> is about 1e-132.  No float atomic, every sum in a fixed order: two calls
 * on the same cores are bit-equal.  Nothing on the device changes but the call's own buffers; no forward is needed afterwards.
 * Refused before anything is launched: TNML_ERR_ARG (a NULL output; per_site neither 0 nor 1; capacity too small; a metric entry
 * that is not finite, or S[d][e] and S[e][d] further apart than 1e-12 of their size; a bond above 64 or environments beyond 160 KB of LDS: the message names the bytes),
 * TNML_ERR_STATE (cores never set; a communicator attached).  After the run: TNML_ERR_NONFINITE (a core element or an environment
 * that is not finite; <W|W>_S == 0, sign_log2 then holds (0, -inf); a gradient element beyond float32): grad_flat is not written. */
int tnml_log_norm_grad(tnml_ctx *ctx, const double *S, int per_site, float *grad_flat, size_t capacity, double *sign_log2);

/* The negative log-likelihood of a batch under p(x, l) = prod_i w(x_i) f_l(x)^2 / Z, Z = <W|W>_S, and its gradient over all cores.
 * X [b][N][D] are the features phi[level] of the pixels on the grid whose Gram matrix is S [D][D] (NULL: the identity); y [b], or
 * NULL for -log p(x) with the label summed.  out3 = { -mean_s(log f_y^2 [or log sum_l f_l^2] - log Z), log Z, samples whose
 * cotangent is not finite }; the term -mean_s sum_i log w(x_{s,i}) does not depend on the model and is the caller's to add.
 * grad_flat (layout and capacity of tnml_core_grad) receives the DESCENT direction G = Gd - Gz: cores + lr G lowers the value.  Gd
 * is tnml_core_grad's gradient with the cotangent 2 delta(l', y_s) / (b f_y[s]) (or 2 f_l'[s] / (b sum_l f_l[s]^2)), in the chunks
 * and with the kernels of that call (tnml_set_core_grad_chunk, tnml_set_chain_scaling apply); Gz is tnml_log_norm_grad's, subtracted
 * on the device.  sum(G_i A_i) = 0 at every site.  The gradient does not depend on the chunk size, nor does the value.
 * The cotangent is a float32, so f itself must be representable: a calibrated network.  Samples with f_y == 0 or a non-finite f are
 * counted; if there are any the call returns TNML_ERR_NONFINITE naming the count, with out3 written and grad_flat not.
 * _indices: the rows idx of the attached dataset (its features must lie on the grid), with the dataset's labels (use_labels != 0) or
 * without.  tnml_nll_eval / tnml_nll_eval_indices: the value alone, without a gradient launch.
 * Refusals: those of tnml_core_grad(_indices) and of tnml_log_norm_grad (per_site 0), and TNML_ERR_ARG for a label outside [0, L).
 * Nothing on the device changes but the calls' own buffers. */
int tnml_nll_grad(tnml_ctx *ctx, const float *X, const int32_t *y, int b, const double *S, float *grad_flat, size_t capacity, double *out3);
int tnml_nll_grad_indices(tnml_ctx *ctx, const int32_t *idx, int b, int use_labels, const double *S, float *grad_flat, size_t capacity,
                          double *out3);
int tnml_nll_eval(tnml_ctx *ctx, const float *X, const int32_t *y, int b, const double *S, double *out3);
int tnml_nll_eval_indices(tnml_ctx *ctx, const int32_t *idx, int n, int use_labels, const double *S, double *out3);

/* ---- likelihood training ----------------------------------------------- */
/* Optimiser steps on G = Gd - Gz of the calls above, with the optimiser of tnml_optim_config and its state rules: the cores stay on
 * the device, nothing of G reaches the host.  Per step: the chunks and kernels of tnml_nll_grad (tnml_set_core_grad_chunk,
 * tnml_set_chain_scaling apply), the sum of the batch's terms, the norm term subtracted on the device, a one-workgroup record, then
 * the update kernel of tnml_gd_step on G.
 * renorm (0 / 1, TNML_ERR_ARG otherwise).  sum(G_i A_i) = 0 at every site, so a plain step only ever grows a core,
 * |A + lr G|^2 = |A|^2 + lr^2 |G|^2, and over an epoch f leaves float32 although the loss does not see a core's scale.  renorm = 1:
 * the update ends with A' <- A' sqrt(sum A^2 / sum A'^2) per core -- both sums in float64 in the fixed order of the clip's sums, A'
 * unrounded, the factor applied in float64 before the one rounding of the store; no factor where sum A'^2 is 0 or not finite; with
 * lr = 0 the core is unchanged bit for bit.  The optimiser state is not rescaled.  renorm = 0 is the plain rule.
 * values4 / values_out [n_steps][4], n_steps = ceil(n / batch): { the value of tnml_nll_eval on batch k BEFORE its step, log Z before
 * the step, samples of the batch whose cotangent is not finite, status bits }.  Bits: 1 / 2 / 4 the status of the norm term (a
 * non-finite environment; Z == 0; a gradient element beyond float32), 8 a batch with a non-finite cotangent, 16 the step was NOT
 * applied.
 * THE GUARD.  A step whose batch or norm term is bad sets a sticky word on the device; the update of that step and of every later
 * step of the call returns without touching cores or state, so after the first bad step k the cores and the state are those after
 * step k - 1.  The call then returns TNML_ERR_NONFINITE naming k and the count, with values_out filled and Adam's t advanced by the
 * applied steps only.  The word is cleared at the start of every call.
 * tnml_nll_train_indices keeps the form of tnml_gd_train_indices: index list, tables and the metric uploaded once, every step
 * enqueued without a wait, one synchronisation at the end.  AFTER a call the context is as after tnml_gd_train_indices.
 * REFUSALS, all before anything is launched: those of tnml_nll_grad(_indices) and of tnml_gd_step / tnml_gd_train_indices. */
int tnml_nll_step(tnml_ctx *ctx, const float *X, const int32_t *y, int b, const double *S, float lr, float weight_dec, int renorm,
                  double *values4);
int tnml_nll_train_indices(tnml_ctx *ctx, const int32_t *idx, int n, int batch, int use_labels, const double *S, float lr,
                           float weight_dec, int renorm, double *values_out);
/* on = 1: the environment walk of the norm term (two workgroups, cores only) runs on a second stream beside the chunks of its step,
 * forked by an event behind the previous update and joined by one before the norm gradient.  Same kernels, inputs and orders: the
 * results are bit-equal.  Default 0 (DESIGN.md section 25 has the measurement).  on outside {0, 1}: TNML_ERR_ARG. */
int tnml_set_nll_overlap(tnml_ctx *ctx, int on);

/* ---- two-site likelihood sweep ------------------------------------------ */
/* DMRG-style steps on the negative log-likelihood: the label sits on site l; a right step (left_dir 0) works on sites (p, p+1) with
 * p = l, a left step on p = l - 1.  With B[a,d,e,c,l'] the product of the two cores, P / Q the per-sample chains behind / ahead of
 * the pair and Lm = L_p, Rm = R_{p+2} the metric environments of tnml_log_norm_grad:
 *   f[l',s] = sum P x_p x_{p+1} Q B,   cot as tnml_nll_grad,   Gd = sum_s cot P x_p x_{p+1} Q   (float32, matrix cores, fixed order)
 *   T = Lm (S (x) S) B Rm,  Z_step = <B, T>,  Gz = 2 T / Z_step,  log Z = log|Z_step| + ln2 (expo_L[p] + expo_R[p+2])   (float64)
 *   B' = B + lr (Gd - Gz);  renorm = 1: B' <- B' sqrt(sum B^2 / sum B'^2), no factor where sum B'^2 is 0 or not finite
 *   split = tensor_svd's (U sqrt(S) behind, sqrt(S) Vh ahead with the label), B' rounded to float32 once where the SVD kernel takes
 *   it; kept rank m = min(max_bond, short side of the merged matrix), and with threshold < 1 the fewest singular values whose
 *   cumulative share sum_j<m sigma_j / sum sigma_j exceeds threshold (TNML_TRUNC_ADAPTIVE's rule), capped by that m.
 * X, y (or NULL: the label is summed) and S ([D][D] or NULL) are tnml_nll_step's.  The call starts at the current l_pos -- any
 * position, no tnml_set_any_position -- takes n_steps steps in the given direction and moves l_pos with them; a second call goes
 * on where the first stopped.  It builds its own chains (the whole batch stays resident: one ahead stack of N x b_pad x capacity
 * floats and the behind pair, no chunks) and stores nothing in the resident batch's stacks.
 * values_out [n_steps][6]: { the value of tnml_nll_eval on the cores BEFORE the step, log Z before the step, samples whose cotangent
 * is not finite, status bits (those of tnml_nll_step), the kept rank, the discarded weight sum_{j>=m} sigma_j^2 / sum sigma_j^2 }.
 * With threshold < 1 the host learns the bond once per step (one wait per step); otherwise every step is enqueued without a wait and
 * the call synchronises once.
 * TRUNCATION WHEN THE LABEL MOVES.  The merged matrix has rank up to min(ml D, mr L) (right step), so with max_bond equal to the
 * existing bond the split truncates even at lr = 0 and the value may RISE (by up to 1.9 nats on random chains of bond 4): this is
 * the reference's sweep geometry.  A sweep meant to descend needs a max_bond that holds the full rank; threshold brings bonds back down.
 * THE GUARD.  A step with a sample of f_y == 0, a non-finite cotangent or a bad norm term sets the sticky word of section 25; that
 * step and every later step of the call hand B itself to the split (the rest of the call re-gauges and does not update), and the
 * call returns TNML_ERR_NONFINITE naming the first bad step, with values_out filled.
 * AFTER a call the context is as after tnml_compress: bonds and l_pos moved, the optimiser state unbound (tnml_optim_reset), the
 * stacks and f of the resident batch stale (tnml_sweep / tnml_update_B return TNML_ERR_STATE until a tnml_forward).  Two calls with
 * equal arguments on equal cores are bit-equal, and so is one call of n steps against two of k and n - k.
 * REFUSALS, all before anything is launched: those of tnml_nll_grad(_indices); D != 2 (TNML_ERR_ARG: the generic-D update is not
 * wired to this call); max_bond < 1 or above the context's bond capacity; threshold outside (0, 1]; renorm outside {0, 1};
 * n_steps < 1; a step whose merged matrix has a short side above 128; a kernel that needs more than 160 KB of LDS (the message
 * names the bytes); TNML_ERR_STATE for more steps than the chain has left in that direction and for a communicator. */
int tnml_nll_sweep(tnml_ctx *ctx, const float *X, const int32_t *y, int b, const double *S, int left_dir, int n_steps, float lr,
                   int renorm, int max_bond, double threshold, double *values_out);
int tnml_nll_sweep_indices(tnml_ctx *ctx, const int32_t *idx, int b, int use_labels, const double *S, int left_dir, int n_steps,
                           float lr, int renorm, int max_bond, double threshold, double *values_out);
/* the last step of the last call, for tests: what = 0 B, 1 Gd, 2 Gz, 3 B_new as the split received it (canonical
 * [ml][D][D][mr][L], float64), 4 sigma (descending, the short side's count).  TNML_ERR_STATE when no step has run. */
enum { TNML_NLL_SWEEP_B = 0, TNML_NLL_SWEEP_GD = 1, TNML_NLL_SWEEP_GZ = 2, TNML_NLL_SWEEP_B_NEW = 3, TNML_NLL_SWEEP_SIGMA = 4 };
int tnml_nll_sweep_debug(tnml_ctx *ctx, int what, double *out, size_t capacity, size_t *n);

/* ---- likelihood training from incomplete data --------------------------- */
/* The gradient of log p(x_G [, c]) over all cores, x_G the known pixels of a sample: every sample has its own mask and its own
 * optional label.  n, K, phi, w, mask, mask_rows and known are tnml_sample_masked's; classes [n] (or NULL: all -1) holds the label of
 * a sample, or -1 where it is unknown and summed -- the JOINT probability p(x_G, c), not the conditional.  With S_{s,i} = w_k phi_k
 * phi_k^T on a known site and S = sum_k w_k phi_k phi_k^T on a free one, R_{s,i} / Lf_{s,i} the per-sample environments of
 * tnml_sample_masked / tnml_site_conditionals (all label slices for class -1, slice c alone otherwise), E_s = log R_{s,0} + ln2 (sum
 * of the exponents), and log Z = E of the empty mask with class -1:
 *   value   = -mean_s (E_s - log Z) = -mean_s log p(x_G,s [, c_s])        (it carries the w_k of the known sites)
 *   g_s,i[a,d,c(,l')] = 2 / n_s,i  sum Lf_s,i[a,a'] S_s,i[d,d'] A_i[a',d',c'(,l')] R_s,i+1[c,c'],    n_s,i = <that contraction, A_i>
 *   G_i     = (1/n) sum_s g_s,i - g_empty,i                                (the DESCENT direction: cores + lr G lowers the value)
 * n_s,i is formed per site from the same rescaled environments, so that no exponent enters the gradient.  sum(G_i A_i) = 0 at every
 * site.  Float64 throughout from the float32 cores, the sum over the samples of a tile inside the matrix cores' k-loop, the tiles
 * added in ascending order, ONE rounding to float32 per element: two equal calls are bit-equal, and the result does not depend on
 * the stack budget or the number of chunks (it may depend on the tile T, which the shape fixes: the largest of 16, 8, 4, 2, 1 at
 * which both kernels fit 160 KB of LDS).  Per tile of a chunk the call needs T (N + 1) m^2 doubles of stack and one partial gradient
 * of tnml_cores_size doubles; both count against tnml_set_sample_stack_bytes.
 * grad_flat (layout of tnml_get_cores, capacity in floats) or NULL: the value alone, only the environments run.  logp_out [n] or
 * NULL: E_s - log Z.  out4 = { value, log Z, samples with E_s = -inf or not finite, status bits }; bits: 1 a non-finite environment,
 * 2 a per-site normaliser that is not positive and finite, 4 a gradient element beyond float32.
 * The cost is O(n N m^3 D) float64 and (N + 1) m^2 doubles of stack a sample: fully observed, uniformly labelled batches should keep
 * using tnml_nll_grad.  Nothing on the device changes but the call's own buffers and the scratch of tnml_sample_masked.
 * Refused before anything is launched: the list of tnml_sample_masked (without its output and uniform rules), TNML_ERR_ARG for a NULL
 * out4, a capacity below tnml_cores_size, a budget below one tile's need; TNML_ERR_SHAPE for a bond above 64, or LDS: the message
 * names the bytes.  After the run: TNML_ERR_NONFINITE naming the count of bad samples (or log Z, or the status bits), with out4
 * written and grad_flat not. */
int tnml_nll_masked_grad(tnml_ctx *ctx, int n, int K, const double *phi, const double *w, const int32_t *classes, const uint8_t *mask,
                         int mask_rows, const int32_t *known, float *grad_flat, size_t capacity, double *logp_out, double *out4);
/* One optimiser step on that gradient: the optimiser of tnml_optim_config, its state rules and renorm as tnml_nll_step, the update
 * kernel of tnml_gd_step.  values4 = out4 of the gradient BEFORE the step, its bits joined by 8 (a batch with a bad sample) and 16
 * (the step was NOT applied).  THE GUARD: the call waits for the gradient once; a bad batch (a sample of zero weight, a status bit)
 * returns TNML_ERR_NONFINITE before the update is enqueued, with cores, state and Adam's t untouched.  AFTER an applied step the
 * context is as after tnml_gd_step: the stacks and f of the resident batch are stale until a tnml_forward.
 * REFUSALS, all before anything is launched: those of tnml_nll_masked_grad; renorm outside {0, 1}; TNML_ERR_STATE for an optimiser
 * state bound to other bonds or another l_pos. */
int tnml_nll_masked_step(tnml_ctx *ctx, int n, int K, const double *phi, const double *w, const int32_t *classes, const uint8_t *mask,
                         int mask_rows, const int32_t *known, float lr, float weight_dec, int renorm, double *values4);

/* Host-side planning helper, exported so that CPU tests can check the bond bookkeeping without a
 * GPU: truncation rank kept by tensor_svd (Network_class.py:894-945) for a step on sites
 * (p, p+1).  Returns m >= 1, or TNML_ERR_SHAPE where the reference itself raises. */
int tnml_trunc_rank(int policy, int left_dir, int p, int N, int ml, int D, int mr, int L, int M);

#ifdef __cplusplus
}
#endif
#endif /* TNML_H */
