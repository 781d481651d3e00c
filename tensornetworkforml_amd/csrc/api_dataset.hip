// Host API, the device-resident dataset: tnml_dataset_attach ... tnml_dataset_read, the index batches (tnml_select_indices,
// tnml_predict_indices, tnml_eval_indices, tnml_resident_metrics), and load_chunk, which every chunked call takes its samples from.
#include "tnml_host.h"

// ---------------------------------------------------------------------------------------------
// device-resident dataset: upload once, then batches and evaluations by index list
// ---------------------------------------------------------------------------------------------
int tnml::ds_usable(tnml_ctx *c) {
  if (!c) return fail(TNML_ERR_ARG, "ctx is NULL");
  if (c->comm) return fail(TNML_ERR_STATE, "a resident dataset is not sharded over ranks: the dataset calls are single-GPU only");
  if (!c->ds_data) return fail(TNML_ERR_STATE, "no dataset attached: call tnml_dataset_attach first");
  return TNML_OK;
}

static void ds_drop(tnml_ctx *c) { c->own.release(c->ds_data); c->own.release(c->ds_labels); c->ds_n = 0; }

extern "C" int tnml_dataset_attach(tnml_ctx *c, const float *data, const int32_t *labels, int n, int N, int D, int form) {
  if (!c || !data || !labels) return fail(TNML_ERR_ARG, "NULL argument");
  if (c->comm) return fail(TNML_ERR_STATE, "a resident dataset is not sharded over ranks: the dataset calls are single-GPU only");
  if (n < 1) return fail(TNML_ERR_ARG, "empty dataset");
  if (N != c->N || D != c->D) return fail(TNML_ERR_ARG, "dataset for N = %d, D = %d attached to a context with N = %d, D = %d", N, D, c->N, c->D);
  if (form != TNML_DATASET_FEATURES && form != TNML_DATASET_PIXELS) return fail(TNML_ERR_ARG, "unknown dataset form %d", form);
  for (int i = 0; i < n; ++i)
    if (labels[i] < 0 || labels[i] >= c->L) return fail(TNML_ERR_ARG, "label %d of sample %d outside [0, %d)", labels[i], i, c->L);
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipStreamSynchronize(c->stream));          // an earlier dataset may still be read
  // Dataset group (sized from n): both arrays or none (ds_usable asks for ds_data)
  const size_t per = (size_t)c->N * (form == TNML_DATASET_PIXELS ? 1 : c->D);
  c->ds_n = 0;
  hipError_t e = c->own.make({own_dev(c->ds_data, (size_t)n * per), own_dev(c->ds_labels, (size_t)n)});
  if (e == hipSuccess) e = hipMemcpy(c->ds_data, data, (size_t)n * per * sizeof(float), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(c->ds_labels, labels, (size_t)n * sizeof(int), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    ds_drop(c);
    return fail(TNML_ERR_HIP, "uploading a dataset of %d samples failed: %s", n, hipGetErrorString(e));
  }
  c->ds_n = n; c->ds_form = form;
  double binom = 1.0;                                 // C(D-1, s), exact in float64 for D <= kMaxD
  for (int s = 0; s < c->D; ++s) {
    c->ds_coef[s] = std::sqrt(binom);
    binom = binom * (double)(c->D - 1 - s) / (double)(s + 1);
  }
  return TNML_OK;
}

extern "C" int tnml_dataset_detach(tnml_ctx *c) {
  if (!c) return fail(TNML_ERR_ARG, "ctx is NULL");
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipStreamSynchronize(c->stream));
  ds_drop(c);
  return TNML_OK;
}

extern "C" int tnml_dataset_size(tnml_ctx *c) { return c ? c->ds_n : TNML_ERR_ARG; }

// idx[0..b) validated against [0, n) and copied to ds_idx; the caller's list is free when this returns and nothing waits for the
// device except for a pinned buffer whose previous copy (two calls back) has not been consumed yet
int tnml::ds_upload_indices(tnml_ctx *c, const int32_t *idx, int b) {
  for (int i = 0; i < b; ++i)
    if (idx[i] < 0 || idx[i] >= c->ds_n) return fail(TNML_ERR_ARG, "index %d at position %d outside [0, %d)", idx[i], i, c->ds_n);
  if (b > c->ds_idx_cap) {                   // Index-list group: the device list, its two pinned buffers and their events
    HIP_TRY(hipStreamSynchronize(c->stream));
    const size_t cap = ((size_t)b + 1023) / 1024 * 1024;
    c->ds_idx_cap = 0;
    c->ds_idx_busy[0] = c->ds_idx_busy[1] = false;
    int rc = make_group(c, "the index list", {
        own_dev(c->ds_idx, cap), own_pinned(c->ds_idx_host[0], cap), own_pinned(c->ds_idx_host[1], cap),
        own_event(c->ds_idx_ev[0], hipEventDisableTiming), own_event(c->ds_idx_ev[1], hipEventDisableTiming)});
    if (rc) return rc;
    c->ds_idx_cap = (int)cap;
  }
  const int slot = (c->ds_idx_cur ^= 1);
  if (c->ds_idx_busy[slot]) HIP_TRY(hipEventSynchronize(c->ds_idx_ev[slot]));
  memcpy(c->ds_idx_host[slot], idx, (size_t)b * sizeof(int));
  HIP_TRY(hipMemcpyAsync(c->ds_idx, c->ds_idx_host[slot], (size_t)b * sizeof(int), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipEventRecord(c->ds_idx_ev[slot], c->stream));
  c->ds_idx_busy[slot] = true;
  return TNML_OK;
}

static int ds_gather(tnml_ctx *c, const int *idx_dev, int b, int b_pad, float *X_out, int *y_out) {
  DatasetGather g{};
  g.data = c->ds_data; g.labels = c->ds_labels; g.idx = idx_dev; g.out = X_out; g.y_out = y_out;
  g.b = b; g.b_pad = b_pad; g.N = c->N; g.D = c->D; g.pixels = (c->ds_form == TNML_DATASET_PIXELS);
  for (int s = 0; s < kMaxD; ++s) g.coef[s] = c->ds_coef[s];
  if (!launch_dataset_gather(g, c->stream)) return fail(TNML_ERR_ARG, "internal: dataset gather refused (b %d, b_pad %d)", b, b_pad);
  HIP_TRY(hipGetLastError());
  return TNML_OK;
}

extern "C" int tnml_select_indices(tnml_ctx *c, const int32_t *idx, int b) {
  int rc = ds_usable(c);
  if (rc) return rc;
  if (!idx) return fail(TNML_ERR_ARG, "NULL argument");
  if (b < 1) return fail(TNML_ERR_ARG, "empty batch");
  HIP_TRY(hipSetDevice(c->device));
  rc = ds_upload_indices(c, idx, b);                  // refuses a bad index before anything of the resident batch is touched
  if (rc) return rc;
  if (b > c->b_cap) {
    HIP_TRY(hipStreamSynchronize(c->stream));
    rc = size_batch_group(c, b);
    if (rc != TNML_OK) return rc;
  }
  c->b = b;
  // what tnml_set_input does after its host -> device copy, with the rows picked by index, on the device and without waiting
  rc = ds_gather(c, c->ds_idx, b, c->b_pad, c->X, c->y);
  if (rc) return rc;
  c->have_input = true;
  c->have_labels = true;
  batch_changed(c);
  return TNML_OK;
}

// Metrics group: the block partials of b_pad samples and the four accumulators (restarted by every call that uses them)
int tnml::ds_ensure_metrics(tnml_ctx *c, int b_pad) {
  const int nblk = (b_pad + kDsMetricThreads - 1) / kDsMetricThreads;
  if (nblk <= c->ds_part_cap) return TNML_OK;
  HIP_TRY(hipStreamSynchronize(c->stream));
  c->ds_part_cap = 0;
  int rc = make_group(c, "the metrics partials", {own_dev(c->ds_part, (size_t)nblk * 4), own_dev(c->ds_acc, 4)});
  if (rc) return rc;
  c->ds_part_cap = nblk;
  return TNML_OK;
}

static int ds_forward_allowed(tnml_ctx *c) { return pred_allowed(c); }

extern "C" int tnml_predict_indices(tnml_ctx *c, const int32_t *idx, int b, float *f_out) {
  int rc = ds_usable(c);
  if (rc) return rc;
  if (!idx || !f_out) return fail(TNML_ERR_ARG, "NULL argument");
  if (b < 1) return fail(TNML_ERR_ARG, "empty batch");
  if ((rc = ds_forward_allowed(c))) return rc;
  HIP_TRY(hipSetDevice(c->device));
  if ((rc = ds_upload_indices(c, idx, b))) return rc;
  if ((rc = pred_ensure_buffers(c, (b + 63) / 64 * 64))) return rc;
  if ((rc = load_chunk(c, nullptr, c->ds_idx, nullptr, 0, b, nullptr))) return rc;
  if ((rc = pred_table(c))) return rc;
  if ((rc = pred_chain(c, b))) return rc;
  HIP_TRY(hipMemcpy2DAsync(f_out, (size_t)b * sizeof(float), c->fpred, (size_t)c->pred_cap * sizeof(float), (size_t)b * sizeof(float),
                           c->L, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return TNML_OK;
}

static int ds_read_acc(tnml_ctx *c, double *out3) {
  double acc[4] = {0, 0, 0, 0};
  HIP_TRY(hipMemcpyAsync(acc, c->ds_acc, sizeof acc, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  out3[0] = acc[0]; out3[1] = acc[1]; out3[2] = acc[2];
  return TNML_OK;
}

extern "C" int tnml_eval_indices(tnml_ctx *c, const int32_t *idx, int b, int act_fn, float T, double *out3) {
  int rc = ds_usable(c);
  if (rc) return rc;
  if (!idx || !out3) return fail(TNML_ERR_ARG, "NULL argument");
  if (b < 1) return fail(TNML_ERR_ARG, "empty index list");
  if (act_fn < 0 || act_fn > 2) return fail(TNML_ERR_ARG, "unknown activation");
  if (dataset_metrics_lds_bytes(c->L) > 64 * 1024) return fail(TNML_ERR_ARG, "metrics kernel: %d labels exceed its LDS tile", c->L);
  if ((rc = ds_forward_allowed(c))) return rc;
  HIP_TRY(hipSetDevice(c->device));
  if ((rc = ds_upload_indices(c, idx, b))) return rc;
  // chunks as wide as the prediction buffers (at least the resident batch's capacity); whole 256-sample blocks of the metrics
  // kernel where they are wide enough, so that a sample's block does not depend on the chunking
  if ((rc = pred_ensure_buffers(c, std::max({c->pred_cap, c->b_pad, 64})))) return rc;     // (64: both groups may be empty after a failed growth)
  const int bpad = c->pred_cap;
  const int chunk = bpad >= kDsMetricThreads ? bpad / kDsMetricThreads * kDsMetricThreads : bpad;
  if ((rc = ds_ensure_metrics(c, bpad))) return rc;
  if ((rc = pred_table(c))) return rc;
  for (int off = 0; off < b; off += chunk) {
    const int bc = std::min(chunk, b - off);
    if ((rc = load_chunk(c, nullptr, c->ds_idx, nullptr, off, bc, c->ds_ypred))) return rc;
    if ((rc = pred_chain(c, bc))) return rc;
    if (!launch_dataset_metrics(c->fpred, c->ds_ypred, c->L, bc, bpad, act_fn, T, c->ds_part, off == 0, c->ds_acc, c->stream))
      return fail(TNML_ERR_ARG, "internal: metrics launch refused");
    HIP_TRY(hipGetLastError());
  }
  return ds_read_acc(c, out3);
}

extern "C" int tnml_resident_metrics(tnml_ctx *c, int act_fn, float T, double *out3) {
  if (!c || !out3) return fail(TNML_ERR_ARG, "NULL argument");
  if (c->comm) return fail(TNML_ERR_STATE, "the metrics of a sharded batch are not reduced over ranks: single-GPU only");
  if (act_fn < 0 || act_fn > 2) return fail(TNML_ERR_ARG, "unknown activation");
  if (!c->have_input || !c->have_labels) return fail(TNML_ERR_STATE, "no resident batch with labels");
  if (!c->f_current) return fail(TNML_ERR_STATE, "no f on the device: call tnml_forward or tnml_sweep first");
  if (dataset_metrics_lds_bytes(c->L) > 64 * 1024) return fail(TNML_ERR_ARG, "metrics kernel: %d labels exceed its LDS tile", c->L);
  HIP_TRY(hipSetDevice(c->device));
  int rc = ds_ensure_metrics(c, c->b_pad);
  if (rc) return rc;
  if (!launch_dataset_metrics(c->f, c->y, c->L, c->b, c->b_pad, act_fn, T, c->ds_part, 1, c->ds_acc, c->stream))
    return fail(TNML_ERR_ARG, "internal: metrics launch refused");
  HIP_TRY(hipGetLastError());
  return ds_read_acc(c, out3);
}

extern "C" int tnml_dataset_read(tnml_ctx *c, const int32_t *idx, int b, float *X_out) {
  int rc = ds_usable(c);
  if (rc) return rc;
  if (!idx || !X_out) return fail(TNML_ERR_ARG, "NULL argument");
  if (b < 1) return fail(TNML_ERR_ARG, "empty index list");
  HIP_TRY(hipSetDevice(c->device));
  if ((rc = ds_upload_indices(c, idx, b))) return rc;
  const int N = c->N, D = c->D, bp = (b + 63) / 64 * 64;
  float *tmp = nullptr;                    // owned for the length of this call
  if ((rc = make_group(c, "the gathered samples", {own_dev(tmp, (size_t)N * bp * D)}))) return rc;
  rc = ds_gather(c, c->ds_idx, b, bp, tmp, nullptr);
  std::vector<float> host;
  if (!rc) {
    host.resize((size_t)N * bp * D);
    hipError_t e = hipMemcpyAsync(host.data(), tmp, host.size() * sizeof(float), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) rc = fail(TNML_ERR_HIP, "reading the gathered samples back failed: %s", hipGetErrorString(e));
  } else {
    (void)hipStreamSynchronize(c->stream);
  }
  c->own.release(tmp);
  if (rc) return rc;
  for (int s = 0; s < b; ++s)              // [N][bp][D] as the device forms it -> [b][N][D]
    for (int n = 0; n < N; ++n)
      memcpy(X_out + ((size_t)s * N + n) * D, host.data() + ((size_t)n * bp + s) * D, (size_t)D * sizeof(float));
  return TNML_OK;
}

// Samples off .. off + bc of a call into the prediction group, site-major in Xpred [N][pred_cap][D]: the dataset rows idx_dev[off ..)
// with their labels to y_out (or nullptr), or, idx_dev == nullptr, X [..][N][D] of the host through Xpred_stage with y (or nullptr) to
// ds_ypred
int tnml::load_chunk(tnml_ctx *c, const float *X, const int *idx_dev, const int32_t *y, int off, int bc, int *y_out) {
  const int N = c->N, D = c->D;
  if (idx_dev) return ds_gather(c, idx_dev + off, bc, c->pred_cap, c->Xpred, y_out);
  HIP_TRY(hipMemcpyAsync(c->Xpred_stage, X + (size_t)off * N * D, (size_t)bc * N * D * sizeof(float), hipMemcpyHostToDevice, c->stream));
  if (y) HIP_TRY(hipMemcpyAsync(c->ds_ypred, y + off, (size_t)bc * sizeof(int), hipMemcpyHostToDevice, c->stream));
  if (D != kD) launch_transpose_input_anyd(c->Xpred_stage, c->Xpred, bc, c->pred_cap, N, D, c->stream);
  else launch_transpose_input(c->Xpred_stage, c->Xpred, bc, c->pred_cap, N, c->stream);
  HIP_TRY(hipGetLastError());
  return TNML_OK;
}
