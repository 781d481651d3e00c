// Host side of libtnml_hip.so: context, device buffers, per-step planning in the sweep-relative
// frame, the sweep driver (wide -> reduce -> [RCCL all-reduce] -> narrow per step, all enqueued on
// one stream without host synchronisation) and the C ABI of include/tnml.h.
#include "tnml_host.h"
#include "small_gemm_device.h"
#include "grad_chain_device.h"

static thread_local std::string g_err;

int tnml::fail(int code, const char *fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

// ---------------------------------------------------------------------------------------------
extern "C" const char *tnml_last_error(void) { return g_err.c_str(); }
extern "C" const char *tnml_version(void) { return "tnml-hip 0.1 (gfx950)"; }

extern "C" int tnml_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

#include "host_plan.inc"      // tnml_trunc_rank, canon_to_rel: pure host arithmetic, also built with sanitizers (make san)

// one (re)size of a group: the message names the group
int tnml::make_group(tnml_ctx *c, const char *what, std::initializer_list<Owner::Member> group) {
  const hipError_t e = c->own.make(group);
  return e == hipSuccess ? TNML_OK : fail(TNML_ERR_HIP, "allocating %s failed: %s", what, hipGetErrorString(e));
}

// Batch group: everything sized from b_pad (bigpipe.Pk too: batch_Pk below creates it on first use, this releases it)
int tnml::size_batch_group(tnml_ctx *c, int b_cap) {
  const int b_pad = (b_cap + 63) / 64 * 64, ntiles = b_pad / kTS;
  c->b = c->b_cap = c->b_pad = c->nblk_cap = 0;
  c->have_input = c->have_labels = false;
  batch_changed(c);
  c->own.release(c->bigpipe.Pk);
  // batch-side workgroups of the pipelined step: at most kPipeMaxWide (from the device's CU count), each looping over pipe_tpw sample tiles
  const int kPipeMaxWide = std::max(16, c->num_cus - 16);      // + update workgroup and its helpers: all resident, one per CU
  c->pipe.tpw = (ntiles + kPipeMaxWide - 1) / kPipeMaxWide;
  c->pipe.nwide = (ntiles + c->pipe.tpw - 1) / c->pipe.tpw;
  c->pipe.ngroups = (c->pipe.nwide + kPipeGroupMax - 1) / kPipeGroupMax;
  const size_t x_elems = (size_t)c->N * b_pad * c->D, f_elems = (size_t)c->L * b_pad, env_elems = (size_t)c->N * c->Mmax * b_pad;
  int rc = make_group(c, "the batch buffers", {
      own_dev(c->X, x_elems), own_dev(c->Xstage, x_elems), own_dev(c->y, (size_t)b_pad),
      own_dev(c->f, f_elems), own_dev(c->ftmp, f_elems), own_dev(c->ftmp2, f_elems),
      own_dev(c->Lenv, env_elems), own_dev(c->Renv, env_elems),
      own_dev(c->slabs, (size_t)ntiles * c->slab_stride), own_dev(c->zslabs, (size_t)c->pipe.nwide * c->zstride)});
  if (rc) return rc;
  c->b_cap = b_cap;
  c->b_pad = b_pad;
  c->nblk_cap = ntiles;
  HIP_TRY(hipMemsetAsync(c->y, 0, (size_t)b_pad * sizeof(int), c->stream));
  HIP_TRY(hipMemsetAsync(c->f, 0, f_elems * sizeof(float), c->stream));
  return TNML_OK;
}

// [D * Mmax][b_pad]  E_k (x) x_k of the pipelined large-tensor step, on its first use after a (re)size of the batch group
static int batch_Pk(tnml_ctx *c) {
  return c->bigpipe.Pk ? TNML_OK : make_group(c, "the row operand of the pipelined large-tensor step", {own_dev(c->bigpipe.Pk, (size_t)c->D * c->Mmax * c->b_pad)});
}

// a call that reads the batch group without asking for an input batch: refused while the group is empty
static int batch_group_there(const tnml_ctx *c) {
  return c->b_pad ? TNML_OK : fail(TNML_ERR_STATE, "the batch buffers are empty (an earlier growth failed): call tnml_set_input again");
}

extern "C" int tnml_create(tnml_ctx **out, int N, int D, int L, int Mmax, int b_capacity, int device) {
  if (!out) return fail(TNML_ERR_ARG, "out is NULL");
  *out = nullptr;
  if (N < 2 || L < 1 || Mmax < 1 || b_capacity < 1) return fail(TNML_ERR_ARG, "bad sizes N=%d L=%d M=%d b=%d", N, L, Mmax, b_capacity);
  if (D < 2 || D > kMaxD) return fail(TNML_ERR_ARG, "feature dimension D = %d outside the supported range [2, %d]", D, kMaxD);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(TNML_ERR_NOGPU, "no HIP device visible: the HIP path has no CPU fallback");
  if (device < 0 || device >= ndev) return fail(TNML_ERR_ARG, "device %d out of range (%d visible)", device, ndev);
  HIP_TRY(hipSetDevice(device));
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, device));
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(TNML_ERR_NOGPU, "device %d is %s; this library carries gfx950 code only", device, prop.gcnArchName);
  std::unique_ptr<tnml_ctx> c(new tnml_ctx());                 // every early return below releases what exists so far
  if (getenv("TNML_EVENT_HANDOFFS") && atoi(getenv("TNML_EVENT_HANDOFFS"))) { c->bigpipe.flags_enabled = false; c->split.flags_enabled = false; }   // see tnml_set_flag_handoffs
  // Under the reference truncation policy the bond next to a chain end becomes len(S) =
  // min(D*left, D*L) (Network_class.py:907-910), which exceeds M when M < D*L (the MNIST script
  // runs M = 3, L = 2): size every buffer for that.
  c->Mpol = Mmax;
  Mmax = std::max(Mmax, D * std::min(L, Mmax));
  c->N = N; c->D = D; c->L = L; c->Mmax = Mmax; c->device = device;
  c->num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  c->bond.assign(N - 1, 1);
  c->core_stride = (size_t)Mmax * D * Mmax;
  c->lab_elems = (size_t)Mmax * D * Mmax * L;
  c->bmax = (size_t)Mmax * D * D * Mmax * L;
  c->slab_stride = (int)((c->bmax + kMetricSlots + 63) / 64 * 64);
  c->zstride = (int)((2 * c->bmax + kMetricSlots + 63) / 64 * 64);       // Z has up to D times the elements of the gradient
  c->metrics_cap = N;
  c->dbg_elems = 4 * c->bmax + kDbgSigma + kDbgScalars + 8;   // 4 tensors, sigma[kDbgSigma], 5 scalars, stamps
  c->tables_bytes = (size_t)N * std::max(sizeof(ChainSite), sizeof(NormChainSite));
  // Fixed group: streams, events and everything sized from N, D, L and the bond capacity alone; it lives as long as the context
  const unsigned notime = hipEventDisableTiming;
  const size_t bmax = c->bmax, zstride = (size_t)c->zstride, norm_elems = (size_t)N * Mmax * Mmax, nrec = (size_t)N + 1;
  int rc = make_group(c.get(), "the context's streams, events and fixed buffers", {
      own_stream(c->stream), own_stream(c->stream2), own_stream(c->stream3),
      own_event(c->ev_p0, notime), own_event(c->ev_p2, notime), own_event(c->ev_p3, notime),
      own_event(c->ev_main, notime), own_event(c->ev_prep, notime), own_event(c->bigpipe.ev_upd, notime), own_event(c->bigpipe.ev_z, notime),
      own_event(c->split.ev_upd[0], notime), own_event(c->split.ev_bat[0], notime),
      own_event(c->split.ev_upd[1], notime), own_event(c->split.ev_bat[1], notime),
      own_event(c->ev0, hipEventDefault), own_event(c->ev1, hipEventDefault), own_event(c->pev0, hipEventDefault), own_event(c->pev1, hipEventDefault),
      own_dev(c->cores, (size_t)N * c->core_stride), own_dev(c->lab[0], c->lab_elems), own_dev(c->lab[1], c->lab_elems),
      own_dev(c->Ln, norm_elems), own_dev(c->Rn, norm_elems),
      own_dev(c->Bnew, bmax), own_dev(c->Bscr, bmax), own_dev(c->prepB, bmax), own_dev(c->prepG, bmax), own_dev(c->sync, 1),
      own_dev(c->gslabs, (size_t)kPipeGroupMax * zstride), own_dev(c->zred, zstride), own_dev(c->pipe.cnt, 32), own_dev(c->zred2, zstride),
      own_dev(c->Tbuf[0], zstride), own_dev(c->Tbuf[1], zstride), own_dev(c->TNbuf[0], zstride), own_dev(c->TNbuf[1], zstride),
      own_dev(c->prepRaw, bmax), own_dev(c->Apub, persist_pub_doubles(D * Mmax * Mmax, Mmax)),
      own_dev(c->pst_dev, nrec), own_pinned(c->pst_host[0], nrec), own_event(c->pst_ev[0], notime),
      own_pinned(c->pst_host[1], nrec), own_event(c->pst_ev[1], notime),
      own_dev(c->pst_cnt, nrec * 32), own_dev(c->pst_flags, 8), own_dev(c->Bscr2, bmax), own_dev(c->red, (size_t)c->slab_stride),
      own_dev(c->metrics, (size_t)c->metrics_cap * 2), own_dev(c->scal, 64), own_dev(c->dbg, c->dbg_elems),
      own_dev(c->status, 2),                                   // [0] status word, [1] kept rank of the last adaptive step
      own_dev(c->counters, (size_t)kCounterSlots),             // see kCounterSlots (tnml_internal.h)
      own_dev(c->tables, c->tables_bytes)});
  if (rc) return rc;
  HIP_TRY(hipMemset(c->sync, 0, sizeof(unsigned)));
  HIP_TRY(hipMemset(c->pipe.cnt, 0, 32 * sizeof(unsigned)));
  HIP_TRY(hipMemsetAsync(c->status, 0, 2 * sizeof(int), c->stream));
  HIP_TRY(hipMemsetAsync(c->counters, 0, kCounterSlots * sizeof(unsigned long long), c->stream));
  // both label buffers start zeroed: a sweep step writes the elements of its label core alone into the buffer it switches to, and
  // tnml_get_core_slots hands out the whole buffer -- the padding must not be what the allocation happened to hold
  HIP_TRY(hipMemsetAsync(c->lab[0], 0, c->lab_elems * sizeof(float), c->stream));
  HIP_TRY(hipMemsetAsync(c->lab[1], 0, c->lab_elems * sizeof(float), c->stream));
  rc = size_batch_group(c.get(), b_capacity);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(c->stream));
  *out = c.release();
  return TNML_OK;
}

extern "C" int tnml_destroy(tnml_ctx *c) {
  if (!c) return TNML_OK;
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  if (c->comm) ncclCommDestroy(c->comm);
  delete c;                                                    // ~Owner releases every buffer, event and stream
  return TNML_OK;
}

// the device status word is sticky: read and clear it (the stream must be idle)
int tnml::check_status(tnml_ctx *c) {
  int st = 0;
  HIP_TRY(hipMemcpy(&st, c->status, sizeof(int), hipMemcpyDeviceToHost));
  if (!st) return TNML_OK;
  HIP_TRY(hipMemset(c->status, 0, sizeof(int)));
  if (st & 124) {       // 4: helpers late, 8: B_new flag never seen, 16: the replay workgroups never saw the rotation log grow,
                        // 32 / 64: the side stream / the context's stream of the large-tensor pipeline never saw the other's sequence number
    HIP_TRY(hipMemset(c->sync, 0, sizeof(unsigned)));          // a late helper may have left the arrival counter mid-count
    HIP_TRY(hipMemset(c->pipe.cnt, 0, 17 * sizeof(unsigned)));
    drop_pregradients(c);
    if ((st & 16) && c->big_ready) {
      unsigned pw[8] = {0};
      (void)hipMemcpy(pw, c->big.prog, sizeof pw, hipMemcpyDeviceToHost);
      return fail(TNML_ERR_STATE, "internal: a replay workgroup never saw the rotation log grow (status %d; its token %u, progress word %u:%u, final word %u:%u, "
                  "rounds applied %u, vector %u; host token %u)", st, pw[2], pw[3] >> 12, pw[3] & 4095u, pw[4] >> 12, pw[4] & 4095u, pw[5], pw[6], c->pipe.token & 0xfffffu);
    }
    return fail(TNML_ERR_STATE, "internal: a workgroup of a sweep-step launch never saw its hand-off (status %d)", st);
  }
  if (st & 1) return fail(TNML_ERR_NONFINITE, "non-finite values reached the bond update / SVD (status %d)", st);
  return fail(TNML_ERR_NONFINITE, "Jacobi SVD did not converge (status %d)", st);
}

extern "C" int tnml_synchronize(tnml_ctx *c) {
  if (!c) return fail(TNML_ERR_ARG, "ctx is NULL");
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return check_status(c);       // failures inside sweeps that handed nothing back surface here
}

// ---------------------------------------------------------------------------------------------
// multi-GPU
// ---------------------------------------------------------------------------------------------
extern "C" int tnml_comm_unique_id(void *uid128) {
  if (!uid128) return fail(TNML_ERR_ARG, "uid buffer is NULL");
  static_assert(sizeof(ncclUniqueId) == 128, "RCCL unique id is expected to be 128 bytes");
  ncclUniqueId id;
  NCCL_TRY(ncclGetUniqueId(&id));
  memcpy(uid128, &id, sizeof id);
  return TNML_OK;
}

extern "C" int tnml_comm_init(tnml_ctx *c, int rank, int nranks, const void *uid128) {
  if (!c || !uid128) return fail(TNML_ERR_ARG, "NULL argument");
  if (nranks < 1 || rank < 0 || rank >= nranks) return fail(TNML_ERR_ARG, "bad rank %d / %d", rank, nranks);
  if (c->D != kD) return fail(TNML_ERR_STATE, "multi-GPU runs are D == %d only (this context has D = %d)", kD, c->D);
  if (c->any_pos) return fail(TNML_ERR_STATE, "sharded batches with the label at an intermediate site are not supported: tnml_set_any_position(ctx, 0) first");
  HIP_TRY(hipSetDevice(c->device));
  c->rank = rank;
  c->nranks = nranks;
  // a 1-rank communicator is pointless in production; TNML_FORCE_COMM=1 creates it anyway so that the
  // RCCL code path (init + per-step all-reduce on the context's stream) can be exercised on one GPU
  if (nranks == 1 && !(getenv("TNML_FORCE_COMM") && atoi(getenv("TNML_FORCE_COMM")))) return TNML_OK;
  ncclUniqueId id;
  memcpy(&id, uid128, sizeof id);
  NCCL_TRY(ncclCommInitRank(&c->comm, nranks, id, rank));
  return TNML_OK;
}

// ---------------------------------------------------------------------------------------------
// parameters
// ---------------------------------------------------------------------------------------------
size_t tnml::core_elems(const tnml_ctx *c, const std::vector<int> &bond, int i, int l_pos) {
  const int ml = i == 0 ? 1 : bond[i - 1], mr = i == c->N - 1 ? 1 : bond[i];
  return (size_t)ml * c->D * mr * (i == l_pos ? c->L : 1);
}

extern "C" int tnml_set_cores(tnml_ctx *c, const float *flat, size_t n_floats, const int32_t *bond, int l_pos) {
  if (!c || !flat || !bond) return fail(TNML_ERR_ARG, "NULL argument");
  if (l_pos < 0 || l_pos >= c->N) return fail(TNML_ERR_ARG, "l_pos %d out of range", l_pos);
  HIP_TRY(hipSetDevice(c->device));
  std::vector<int> nb(bond, bond + c->N - 1);
  // every buffer indexed by a bond (environment slots of Mmax rows, the LDS tiles and operand layouts of the chain kernels, the
  // norm environments) is sized by the capacity; a core that is narrow on its other side would pass the size check below
  for (int i = 0; i < c->N - 1; ++i)
    if (nb[i] > c->Mmax)
      return fail(TNML_ERR_ARG, "bond %d between sites %d and %d exceeds the capacity %d of this context (created with M = %d)",
                  nb[i], i, i + 1, c->Mmax, c->Mpol);
  size_t total = 0;
  for (int i = 0; i < c->N; ++i) {
    const int ml = i == 0 ? 1 : nb[i - 1], mr = i == c->N - 1 ? 1 : nb[i];
    if (ml < 1 || mr < 1) return fail(TNML_ERR_ARG, "bond dimension < 1 at site %d", i);
    const size_t ne = core_elems(c, nb, i, l_pos);
    if (i == l_pos ? ne > c->lab_elems : ne > c->core_stride)
      return fail(TNML_ERR_ARG, "core %d (%d x %d x %d) exceeds the capacity for M = %d", i, ml, c->D, mr, c->Mmax);
    total += ne;
  }
  if (total != n_floats) return fail(TNML_ERR_ARG, "cores_flat holds %zu floats, bonds imply %zu", n_floats, total);
  std::vector<float> stage((size_t)c->N * c->core_stride, 0.f);
  size_t off = 0;
  const float *labsrc = nullptr;
  size_t labn = 0;
  for (int i = 0; i < c->N; ++i) {
    const size_t ne = core_elems(c, nb, i, l_pos);
    if (i == l_pos) { labsrc = flat + off; labn = ne; }
    else memcpy(stage.data() + (size_t)i * c->core_stride, flat + off, ne * sizeof(float));
    off += ne;
  }
  HIP_TRY(hipMemcpyAsync(c->cores, stage.data(), stage.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(c->lab[c->lab_cur], labsrc, labn * sizeof(float), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  c->bond = nb;
  c->l_pos = l_pos;
  c->cores_set = true;
  cores_changed(c);
  return TNML_OK;
}

extern "C" int tnml_cores_size(tnml_ctx *c, size_t *n_floats) {
  if (!c || !n_floats) return fail(TNML_ERR_ARG, "NULL argument");
  size_t total = 0;
  for (int i = 0; i < c->N; ++i) total += core_elems(c, c->bond, i, c->l_pos);
  *n_floats = total;
  return TNML_OK;
}

extern "C" int tnml_get_cores(tnml_ctx *c, float *flat, size_t capacity, int32_t *bond, int *l_pos) {
  if (!c || !flat) return fail(TNML_ERR_ARG, "NULL argument");
  if (!c->cores_set) return fail(TNML_ERR_STATE, "cores were never set");
  HIP_TRY(hipSetDevice(c->device));
  size_t total = 0;
  tnml_cores_size(c, &total);
  if (capacity < total) return fail(TNML_ERR_ARG, "capacity %zu < %zu floats", capacity, total);
  std::vector<float> stage((size_t)c->N * c->core_stride);
  std::vector<float> labh(c->lab_elems);
  HIP_TRY(hipMemcpyAsync(stage.data(), c->cores, stage.size() * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(labh.data(), c->lab[c->lab_cur], labh.size() * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  size_t off = 0;
  for (int i = 0; i < c->N; ++i) {
    const size_t ne = core_elems(c, c->bond, i, c->l_pos);
    memcpy(flat + off, i == c->l_pos ? labh.data() : stage.data() + (size_t)i * c->core_stride, ne * sizeof(float));
    off += ne;
  }
  if (bond) for (int i = 0; i < c->N - 1; ++i) bond[i] = c->bond[i];
  if (l_pos) *l_pos = c->l_pos;
  return TNML_OK;
}

// the bonds and the label position alone: host bookkeeping, nothing is copied from the device
extern "C" int tnml_get_bonds(tnml_ctx *c, int32_t *bond, int *l_pos) {
  if (!c || !bond) return fail(TNML_ERR_ARG, "NULL argument");
  if (!c->cores_set) return fail(TNML_ERR_STATE, "cores were never set");
  for (int i = 0; i < c->N - 1; ++i) bond[i] = c->bond[i];
  if (l_pos) *l_pos = c->l_pos;
  return TNML_OK;
}

extern "C" int tnml_get_core_slots(tnml_ctx *c, float *slots, size_t slots_capacity, float *label_buffer, size_t label_capacity) {
  if (!c || !slots || !label_buffer) return fail(TNML_ERR_ARG, "NULL argument");
  const size_t ns = (size_t)c->N * c->core_stride;
  if (slots_capacity < ns || label_capacity < c->lab_elems)
    return fail(TNML_ERR_ARG, "capacities %zu and %zu < %zu and %zu floats", slots_capacity, label_capacity, ns, c->lab_elems);
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipMemcpyAsync(slots, c->cores, ns * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(label_buffer, c->lab[c->lab_cur], c->lab_elems * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return TNML_OK;
}

extern "C" int tnml_scale_cores(tnml_ctx *c, double factor) {
  if (!c) return fail(TNML_ERR_ARG, "ctx is NULL");
  if (!c->cores_set) return fail(TNML_ERR_STATE, "cores were never set");
  HIP_TRY(hipSetDevice(c->device));
  launch_scale(c->cores, (size_t)c->N * c->core_stride, (float)factor, c->stream);
  launch_scale(c->lab[c->lab_cur], c->lab_elems, (float)factor, c->stream);
  HIP_TRY(hipGetLastError());
  cores_changed(c);
  return TNML_OK;
}

// ---------------------------------------------------------------------------------------------
// batch
// ---------------------------------------------------------------------------------------------
extern "C" int tnml_set_input(tnml_ctx *c, const float *X, const int32_t *y, int b) {
  if (!c || !X) return fail(TNML_ERR_ARG, "NULL argument");
  if (b < 1) return fail(TNML_ERR_ARG, "empty batch");
  if (y)
    for (int i = 0; i < b; ++i)
      if (y[i] < 0 || y[i] >= c->L) return fail(TNML_ERR_ARG, "label %d of sample %d outside [0, %d)", y[i], i, c->L);
  HIP_TRY(hipSetDevice(c->device));
  if (b > c->b_cap) {
    HIP_TRY(hipStreamSynchronize(c->stream));
    int rc = size_batch_group(c, b);
    if (rc != TNML_OK) return rc;
  }
  // keep the padding of a previous, larger batch from leaking: b_pad is per-capacity, the live
  // batch is [0, b); kernels mask samples >= b.
  c->b = b;
  HIP_TRY(hipMemcpyAsync(c->Xstage, X, (size_t)b * c->N * c->D * sizeof(float), hipMemcpyHostToDevice, c->stream));
  if (c->D != kD) launch_transpose_input_anyd(c->Xstage, c->X, b, c->b_pad, c->N, c->D, c->stream);
  else launch_transpose_input(c->Xstage, c->X, b, c->b_pad, c->N, c->stream);
  HIP_TRY(hipGetLastError());
  if (y) {
    HIP_TRY(hipMemsetAsync(c->y, 0, (size_t)c->b_pad * sizeof(int), c->stream));
    HIP_TRY(hipMemcpyAsync(c->y, y, (size_t)b * sizeof(int), hipMemcpyHostToDevice, c->stream));
  }
  HIP_TRY(hipStreamSynchronize(c->stream));   // X / y host buffers may be released by the caller
  c->have_input = true;
  c->have_labels = (y != nullptr);
  batch_changed(c);
  return TNML_OK;
}

extern "C" int tnml_stage_batch(tnml_ctx *c, int slot, const float *X, const int32_t *y, int b) {
  if (!c || !X || !y) return fail(TNML_ERR_ARG, "NULL argument");
  if (slot < 0 || slot >= tnml_ctx::kStageSlots) return fail(TNML_ERR_ARG, "slot %d outside [0, %d)", slot, tnml_ctx::kStageSlots);
  if (b < 1) return fail(TNML_ERR_ARG, "empty batch");
  for (int i = 0; i < b; ++i)
    if (y[i] < 0 || y[i] >= c->L) return fail(TNML_ERR_ARG, "label %d of sample %d outside [0, %d)", y[i], i, c->L);
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipStreamSynchronize(c->stream));
  // Stage-slot group (one per slot, sized from its batch): complete (both arrays, its size) or empty
  float *&sx = c->stageX[slot];
  int *&sy = c->stageY[slot];
  c->stageB[slot] = 0;
  hipError_t e = c->own.make({own_dev(sx, (size_t)b * c->N * c->D), own_dev(sy, (size_t)b)});
  if (e == hipSuccess) e = hipMemcpy(sx, X, (size_t)b * c->N * c->D * sizeof(float), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(sy, y, (size_t)b * sizeof(int), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    c->own.release(sx); c->own.release(sy);
    return fail(TNML_ERR_HIP, "staging a batch of %d samples failed: %s", b, hipGetErrorString(e));
  }
  c->stageB[slot] = b;
  return TNML_OK;
}

extern "C" int tnml_select_batch(tnml_ctx *c, int slot) {
  if (!c) return fail(TNML_ERR_ARG, "ctx is NULL");
  if (slot < 0 || slot >= tnml_ctx::kStageSlots || !c->stageX[slot] || !c->stageY[slot] || c->stageB[slot] < 1)
    return fail(TNML_ERR_ARG, "slot %d holds no staged batch", slot);
  HIP_TRY(hipSetDevice(c->device));
  const int b = c->stageB[slot];
  if (b > c->b_cap) {
    HIP_TRY(hipStreamSynchronize(c->stream));
    int rc = size_batch_group(c, b);
    if (rc != TNML_OK) return rc;
  }
  c->b = b;
  // what tnml_set_input does after its host -> device copy, entirely on the device and without waiting
  if (c->D != kD) launch_transpose_input_anyd(c->stageX[slot], c->X, b, c->b_pad, c->N, c->D, c->stream);
  else launch_transpose_input(c->stageX[slot], c->X, b, c->b_pad, c->N, c->stream);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemsetAsync(c->y, 0, (size_t)c->b_pad * sizeof(int), c->stream));
  HIP_TRY(hipMemcpyAsync(c->y, c->stageY[slot], (size_t)b * sizeof(int), hipMemcpyDeviceToDevice, c->stream));
  c->have_input = true;
  c->have_labels = true;
  batch_changed(c);
  return TNML_OK;
}

extern "C" int tnml_set_labels(tnml_ctx *c, const int32_t *y, int b) {
  if (!c || !y) return fail(TNML_ERR_ARG, "NULL argument");
  if (!c->have_input) return fail(TNML_ERR_STATE, "no input batch: call tnml_set_input first");
  if (b != c->b) return fail(TNML_ERR_ARG, "labels (%d) and resident batch (%d) differ in length", b, c->b);
  for (int i = 0; i < b; ++i)
    if (y[i] < 0 || y[i] >= c->L) return fail(TNML_ERR_ARG, "label %d of sample %d outside [0, %d)", y[i], i, c->L);
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipMemsetAsync(c->y, 0, (size_t)c->b_pad * sizeof(int), c->stream));
  HIP_TRY(hipMemcpyAsync(c->y, y, (size_t)b * sizeof(int), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  c->have_labels = true;
  drop_pregradients(c);             // the pre-gradient carries the loss derivative of the old labels
  return TNML_OK;
}

static int copy_f_out(tnml_ctx *c, const float *src_dev, float *f_out) {
  // [L][b_pad] on the device -> [L][b] on the host
  HIP_TRY(hipMemcpy2DAsync(f_out, (size_t)c->b * sizeof(float), src_dev, (size_t)c->b_pad * sizeof(float),
                           (size_t)c->b * sizeof(float), c->L, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return TNML_OK;
}

// ---------------------------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------------------------
// chain order and strides of every site for the environment chain that ends at the label site
static int upload_chain_table(tnml_ctx *c) {
  const int N = c->N, D = c->D, L = c->L;
  std::vector<ChainSite> tab(N);
  const bool right_envs = (c->l_pos == 0);
  for (int k = 0; k < N; ++k) {
    ChainSite cs{};
    const int i = right_envs ? N - 1 - k : k;       // chain order
    const int ml = c->ml(i), mr = c->mr(i);
    cs.x_site = i;
    const bool lab = (k == N - 1);
    cs.is_label = lab;
    cs.core_off = lab ? 0 : (int)((size_t)i * c->core_stride);
    if (right_envs) {
      cs.n_in = mr;
      if (!lab) { cs.n_out = ml; cs.s_in = 1; cs.s_d = mr; cs.s_out = D * mr; cs.env_out_off = c->env_off(i); }
      else { cs.n_out = L; cs.s_in = L; cs.s_d = mr * L; cs.s_out = 1; cs.env_out_off = -1; }
    } else {
      cs.n_in = ml;
      if (!lab) { cs.n_out = mr; cs.s_in = D * mr; cs.s_d = mr; cs.s_out = 1; cs.env_out_off = c->env_off(i); }
      else { cs.n_out = L; cs.s_in = D * L; cs.s_d = L; cs.s_out = 1; cs.env_out_off = -1; }
    }
    tab[k] = cs;
  }
  HIP_TRY(hipMemcpyAsync(c->tables, tab.data(), tab.size() * sizeof(ChainSite), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));   // tab is a stack object
  return TNML_OK;
}

// ---------------------------------------------------------------------------------------------
// Label at an intermediate site (tnml_set_any_position): two half-chains that start at the chain ends and
// stop next to the label site -- the chain kernels with a table that has no label entry -- and the contraction of the label core
// with the environment on either side of it (kernels_meet.hip).
// ---------------------------------------------------------------------------------------------
static bool label_inside(const tnml_ctx *c) { return c->l_pos != 0 && c->l_pos != c->N - 1; }

// sites 0 .. l-1 (left environments) followed by sites N-1 .. l+1 (right environments) in the context's table scratch.  keep:
// every environment goes to its slot of the stack the launch is given; otherwise only the last one of either half is stored, as
// the named output of its chain (the slot of the table entry that would carry the label site: env_out_off = -1)
static int upload_half_tables(tnml_ctx *c, bool keep) {
  const int N = c->N, D = c->D, l = c->l_pos;
  std::vector<ChainSite> tab;
  tab.reserve(N - 1);
  for (int i = 0; i < l; ++i) {
    ChainSite cs{};
    const int ml = c->ml(i), mr = c->mr(i);
    cs.x_site = i; cs.core_off = (int)((size_t)i * c->core_stride);
    cs.n_in = ml; cs.n_out = mr; cs.s_in = D * mr; cs.s_d = mr; cs.s_out = 1;
    cs.env_out_off = keep ? c->env_off(i) : (i == l - 1 ? -1 : 0);
    tab.push_back(cs);
  }
  for (int i = N - 1; i > l; --i) {
    ChainSite cs{};
    const int ml = c->ml(i), mr = c->mr(i);
    cs.x_site = i; cs.core_off = (int)((size_t)i * c->core_stride);
    cs.n_in = mr; cs.n_out = ml; cs.s_in = 1; cs.s_d = mr; cs.s_out = D * mr;
    cs.env_out_off = keep ? c->env_off(i) : (i == l + 1 ? -1 : 0);
    tab.push_back(cs);
  }
  HIP_TRY(hipMemcpyAsync(c->tables, tab.data(), tab.size() * sizeof(ChainSite), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));   // tab is a stack object
  return TNML_OK;
}

// one half-chain of the uploaded pair: `env` the stack it fills (keep) or nullptr, `last` the buffer of its last environment otherwise
static int half_chain(tnml_ctx *c, bool right_half, const float *X, float *env, float *last, int b, int b_pad) {
  const int l = c->l_pos, n = right_half ? c->N - 1 - l : l;
  const ChainSite *tab = (const ChainSite *)c->tables + (right_half ? l : 0);
  if (c->D != kD) {
    if (!launch_env_chain_anyd(tab, n, c->cores, c->lab[c->lab_cur], X, env, last, b, b_pad, c->L, c->Mmax, c->D, nullptr, c->stream))
      return fail(TNML_ERR_ARG, "forward chain at D = %d, M = %d: %zu bytes of LDS exceed 160 KB", c->D, c->Mmax, anyd_chain_lds_bytes(c->Mmax, c->D, c->L));
  } else
  launch_env_chain(tab, n, c->cores, c->lab[c->lab_cur], X, env, last, b, b_pad, c->L, c->Mmax, nullptr, c->stream, c->chain_plain);
  HIP_TRY(hipGetLastError());
  return TNML_OK;
}

static int label_meet(tnml_ctx *c, const float *Lenv, const float *Renv, const float *X, float *f, int b, int b_pad) {
  MeetParams m{};
  const int l = c->l_pos;
  m.Lenv = Lenv; m.Renv = Renv; m.x = X + (size_t)l * b_pad * c->D; m.core = c->lab[c->lab_cur]; m.f = f;
  m.b = b; m.b_pad = b_pad; m.ml = c->ml(l); m.mr = c->mr(l); m.D = c->D; m.L = c->L;
  if (!launch_label_meet(m, c->stream))
    return fail(TNML_ERR_ARG, "label site %d: one row of its core (%d x %d x %d floats) and the environment tile do not fit 160 KB of LDS", l, c->D, m.mr, c->L);
  HIP_TRY(hipGetLastError());
  return TNML_OK;
}

// tnml_forward with the label inside the chain: both stacks up to the label site, f from their meeting
static int run_chain_inside(tnml_ctx *c) {
  HIP_TRY(hipSetDevice(c->device));
  const int N = c->N, l = c->l_pos;
  int rc = upload_half_tables(c, true);
  if (rc) return rc;
  if (c->profile) HIP_TRY(hipEventRecord(c->pev0, c->stream));
  if ((rc = half_chain(c, false, c->X, c->Lenv, c->f, c->b, c->b_pad))) return rc;
  if ((rc = half_chain(c, true, c->X, c->Renv, c->f, c->b, c->b_pad))) return rc;
  if ((rc = label_meet(c, c->env_slot(c->Lenv, l - 1), c->env_slot(c->Renv, l + 1), c->X, c->f, c->b, c->b_pad))) return rc;
  if (c->profile) {
    HIP_TRY(hipEventRecord(c->pev1, c->stream));
    HIP_TRY(hipEventSynchronize(c->pev1));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, c->pev0, c->pev1));
    c->prof_ms[0] += ms; c->prof_n[0]++;
  }
  c->cnt_fwd += 1;
  for (int i = 0; i < N - 1; ++i) c->cnt_fwd_bytes += 4.0 * c->b * (2.0 * c->bond[i] + c->D);
  c->envs_valid_L = c->envs_valid_R = true;
  c->f_current = true;
  c->Bnew_valid = false;
  drop_pregradients(c);
  return TNML_OK;
}

static int run_chain(tnml_ctx *c, bool logmode) {
  if (!c->cores_set) return fail(TNML_ERR_STATE, "cores were never set");
  if (!c->have_input) return fail(TNML_ERR_STATE, "no input batch: call tnml_set_input first");
  if (label_inside(c)) {
    if (!c->any_pos || logmode)
      return fail(TNML_ERR_STATE, "forward should not be called if l has an intermediate position (l_pos = %d)", c->l_pos);
    return run_chain_inside(c);
  }
  HIP_TRY(hipSetDevice(c->device));
  const int N = c->N, D = c->D, L = c->L;
  const bool right_envs = (c->l_pos == 0);
  int rc0 = upload_chain_table(c);
  if (rc0) return rc0;
  if (c->profile) HIP_TRY(hipEventRecord(c->pev0, c->stream));
  if (D != kD) {
    if (!launch_env_chain_anyd((const ChainSite *)c->tables, N, c->cores, c->lab[c->lab_cur], c->X, right_envs ? c->Renv : c->Lenv, c->f,
                               c->b, c->b_pad, L, c->Mmax, D, logmode ? c->slabs : nullptr, c->stream))
      return fail(TNML_ERR_ARG, "forward chain at D = %d, M = %d: %zu bytes of LDS exceed 160 KB", D, c->Mmax, anyd_chain_lds_bytes(c->Mmax, D, L));
  } else
  launch_env_chain((const ChainSite *)c->tables, N, c->cores, c->lab[c->lab_cur], c->X,
                   right_envs ? c->Renv : c->Lenv, c->f, c->b, c->b_pad, L, c->Mmax,
                   logmode ? c->slabs : nullptr, c->stream, c->chain_plain);
  HIP_TRY(hipGetLastError());
  if (c->profile) {
    HIP_TRY(hipEventRecord(c->pev1, c->stream));
    HIP_TRY(hipEventSynchronize(c->pev1));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, c->pev0, c->pev1));
    c->prof_ms[0] += ms; c->prof_n[0]++;
  }
  if (!logmode) {
    c->cnt_fwd += 1;
    for (int i = 0; i < N - 1; ++i) c->cnt_fwd_bytes += 4.0 * c->b * (2.0 * c->bond[i] + D);      // environment in + out, features
    c->envs_valid_R = right_envs;
    c->envs_valid_L = !right_envs;
    c->f_current = true;
    c->Bnew_valid = false;
    drop_pregradients(c);
  }
  return TNML_OK;
}

extern "C" int tnml_forward(tnml_ctx *c, float *f_out) {
  if (!c) return fail(TNML_ERR_ARG, "ctx is NULL");
  int rc = run_chain(c, false);
  if (rc) return rc;
  if (f_out) return copy_f_out(c, c->f, f_out);
  return TNML_OK;
}

// Prediction group, grown to bp samples: tnml_predict's own batch -- Xpred_stage [b][N][D] as uploaded, Xpred [N][pred_cap][D],
// fpred [L][pred_cap] -- with the two environments next to an intermediate label site (predEnv) and the labels of the chunk
// tnml_eval_indices is evaluating (ds_ypred)
int tnml::pred_ensure_buffers(tnml_ctx *c, int bp, bool scaled_out) {
  const bool sc = c->scaled || scaled_out || c->pred_mant;     // (once there, the scaled members stay members)
  if (bp <= c->pred_cap && (!sc || c->pred_mant)) return TNML_OK;
  bp = std::max(bp, c->pred_cap);                              // (the gradient groups were sized against this capacity)
  const int N = c->N, D = c->D, L = c->L;
  HIP_TRY(hipStreamSynchronize(c->stream));
  c->pred_cap = 0;
  int rc = make_group(c, "the prediction buffers", {
      own_dev(c->Xpred_stage, (size_t)bp * N * D), own_dev(c->Xpred, (size_t)bp * N * D), own_dev(c->fpred, (size_t)bp * L),
      own_dev(c->predEnv, (size_t)2 * c->Mmax * bp), own_dev(c->ds_ypred, (size_t)bp),
      own_dev_if(sc, c->pred_mant, (size_t)bp * L), own_dev_if(sc, c->pred_expo, (size_t)bp), own_dev_if(sc, c->pred_bond, (size_t)N)});
  if (rc) return rc;
  // on the context's stream: a memset on the null stream is not ordered against this (non-blocking) stream and could land behind
  // the re-tiling kernel that follows
  HIP_TRY(hipMemsetAsync(c->Xpred, 0, (size_t)bp * N * D * sizeof(float), c->stream));
  c->pred_cap = bp;
  return TNML_OK;
}

// scaled_pred_kernel stages a whole core and three tiles of the largest bond in LDS, as the two-pass gradient chain does
static int scaled_pred_fits(const tnml_ctx *c) {
  const int mb = *std::max_element(c->bond.begin(), c->bond.end());
  const size_t lds = scaled_pred_lds_bytes(mb, c->D, c->L, c->N);
  if (lds > kLdsMax) return fail(TNML_ERR_ARG, "scaled prediction at D = %d, bond %d, L = %d: %zu bytes of LDS exceed 160 KB", c->D, mb, c->L, lds);
  return TNML_OK;
}

// may a prediction run at this label position (and, with scaled chains, at these bonds)?
int tnml::pred_allowed(tnml_ctx *c) {
  if (!c->cores_set) return fail(TNML_ERR_STATE, "cores were never set");
  if (label_inside(c) && !c->any_pos)
    return fail(TNML_ERR_STATE, "forward should not be called if l has an intermediate position (l_pos = %d)", c->l_pos);
  return c->scaled ? scaled_pred_fits(c) : TNML_OK;
}

// the chain table of a prediction: towards the label site, or the two half-chains
// (scaled chains: the bond table of scaled_pred_kernel; c->bond is not written while a call is in flight)
int tnml::pred_table(tnml_ctx *c, bool scaled) {
  if (c->scaled || scaled) {
    HIP_TRY(hipMemcpyAsync(c->pred_bond, c->bond.data(), (size_t)(c->N - 1) * sizeof(int), hipMemcpyHostToDevice, c->stream));
    return TNML_OK;
  }
  return label_inside(c) ? upload_half_tables(c, false) : upload_chain_table(c);
}

// scaled chains: both half-chains and the label site in one kernel over Xpred -> pred_mant, pred_expo, fpred
static int pred_chain_scaled(tnml_ctx *c, int b) {
  if (int rc = scaled_pred_fits(c)) return rc;
  const int mb = *std::max_element(c->bond.begin(), c->bond.end());
  ScaledPredParams p{};
  p.bond = c->pred_bond; p.cores = c->cores; p.labcore = c->lab[c->lab_cur]; p.X = c->Xpred;
  p.mant = c->pred_mant; p.expo = c->pred_expo; p.f = c->fpred; p.core_stride = c->core_stride;
  p.b = b; p.b_pad = c->pred_cap; p.N = c->N; p.D = c->D; p.L = c->L; p.l_pos = c->l_pos; p.mb = mb;
  if (!launch_scaled_pred(p, c->stream)) return fail(TNML_ERR_ARG, "internal: scaled prediction launch refused (b %d, b_pad %d)", b, c->pred_cap);
  HIP_TRY(hipGetLastError());
  return TNML_OK;
}

// one chain towards the label site over Xpred -> fpred, no environment stored (the chain table must be uploaded)
int tnml::pred_chain(tnml_ctx *c, int b) {
  if (c->scaled) return pred_chain_scaled(c, b);
  const int N = c->N, D = c->D, L = c->L, bpad = c->pred_cap;
  if (label_inside(c)) {
    float *EL = c->predEnv, *ER = c->predEnv + (size_t)c->Mmax * c->pred_cap;
    int rc = half_chain(c, false, c->Xpred, nullptr, EL, b, bpad);
    if (!rc) rc = half_chain(c, true, c->Xpred, nullptr, ER, b, bpad);
    if (!rc) rc = label_meet(c, EL, ER, c->Xpred, c->fpred, b, bpad);
    return rc;
  }
  if (D != kD) {
    if (!launch_env_chain_anyd((const ChainSite *)c->tables, N, c->cores, c->lab[c->lab_cur], c->Xpred, nullptr, c->fpred, b, bpad, L,
                               c->Mmax, D, nullptr, c->stream))
      return fail(TNML_ERR_ARG, "forward chain at D = %d, M = %d: %zu bytes of LDS exceed 160 KB", D, c->Mmax, anyd_chain_lds_bytes(c->Mmax, D, L));
  } else
  launch_env_chain((const ChainSite *)c->tables, N, c->cores, c->lab[c->lab_cur], c->Xpred, nullptr, c->fpred, b, bpad, L,
                   c->Mmax, nullptr, c->stream, c->chain_plain);
  HIP_TRY(hipGetLastError());
  return TNML_OK;
}

extern "C" int tnml_predict(tnml_ctx *c, const float *X, int b, float *f_out) {
  // Network.forward's output for a batch that is NOT made resident (validation, Network_class.py:339-346):
  // one chain towards the label site, no environment is stored, the training batch and its environments
  // stay as they are.
  if (!c || !X || !f_out) return fail(TNML_ERR_ARG, "NULL argument");
  if (b < 1) return fail(TNML_ERR_ARG, "empty batch");
  int rc = pred_allowed(c);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(c->device));
  rc = pred_ensure_buffers(c, (b + 63) / 64 * 64);
  if (rc) return rc;
  if ((rc = load_chunk(c, X, nullptr, nullptr, 0, b, nullptr))) return rc;
  rc = pred_table(c);
  if (rc) return rc;
  if ((rc = pred_chain(c, b))) return rc;
  HIP_TRY(hipMemcpy2DAsync(f_out, (size_t)b * sizeof(float), c->fpred, (size_t)c->pred_cap * sizeof(float), (size_t)b * sizeof(float),
                           c->L, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return TNML_OK;
}

extern "C" int tnml_predict_scaled(tnml_ctx *c, const float *X, int b, float *mant_out, int32_t *expo_out) {
  if (!c || !X || !mant_out || !expo_out) return fail(TNML_ERR_ARG, "NULL argument");
  if (b < 1) return fail(TNML_ERR_ARG, "empty batch");
  int rc = pred_allowed(c);
  if (!rc) rc = scaled_pred_fits(c);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(c->device));
  rc = pred_ensure_buffers(c, (b + 63) / 64 * 64, true);
  if (rc) return rc;
  if ((rc = load_chunk(c, X, nullptr, nullptr, 0, b, nullptr))) return rc;
  if ((rc = pred_table(c, true))) return rc;
  if ((rc = pred_chain_scaled(c, b))) return rc;
  HIP_TRY(hipMemcpy2DAsync(mant_out, (size_t)b * sizeof(float), c->pred_mant, (size_t)c->pred_cap * sizeof(float), (size_t)b * sizeof(float),
                           c->L, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(expo_out, c->pred_expo, (size_t)b * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return TNML_OK;
}

extern "C" int tnml_set_chain_scaling(tnml_ctx *c, int on) {
  if (!c) return fail(TNML_ERR_ARG, "ctx is NULL");
  if (on != 0 && on != 1) return fail(TNML_ERR_ARG, "chain scaling %d is neither 0 nor 1", on);
  c->scaled = on != 0;
  return TNML_OK;
}

extern "C" int tnml_forward_logabsmax(tnml_ctx *c, double *out) {
  if (!c || !out) return fail(TNML_ERR_ARG, "NULL argument");
  int rc = run_chain(c, true);
  if (rc) return rc;
  const int nb = c->b_pad / kChainSamplesPerBlock;
  std::vector<float> part(nb);
  HIP_TRY(hipMemcpyAsync(part.data(), c->slabs, nb * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  float best = -INFINITY;
  for (float v : part) best = std::max(best, v);
  if (c->comm) {
    HIP_TRY(hipMemcpyAsync(c->scal, &best, sizeof(float), hipMemcpyHostToDevice, c->stream));
    NCCL_TRY(ncclAllReduce(c->scal, c->scal, 1, ncclFloat, ncclMax, c->comm, c->stream));
    HIP_TRY(hipMemcpyAsync(&best, c->scal, sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
  }
  *out = best;
  return TNML_OK;
}

extern "C" int tnml_f_absmax(tnml_ctx *c, double *out) {
  if (!c || !out) return fail(TNML_ERR_ARG, "NULL argument");
  if (int rc = batch_group_there(c)) return rc;
  HIP_TRY(hipSetDevice(c->device));
  launch_absmax(c->f, c->L, c->b, c->b_pad, c->scal, c->stream);
  HIP_TRY(hipGetLastError());
  if (c->comm) NCCL_TRY(ncclAllReduce(c->scal, c->scal, 1, ncclFloat, ncclMax, c->comm, c->stream));
  float v = 0;
  HIP_TRY(hipMemcpyAsync(&v, c->scal, sizeof(float), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  *out = v;
  return TNML_OK;
}

extern "C" int tnml_set_f(tnml_ctx *c, const float *f) {
  if (!c || !f) return fail(TNML_ERR_ARG, "NULL argument");
  if (!c->have_input) return fail(TNML_ERR_STATE, "no input batch");
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipMemcpy2DAsync(c->f, (size_t)c->b_pad * sizeof(float), f, (size_t)c->b * sizeof(float),
                           (size_t)c->b * sizeof(float), c->L, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  c->f_current = true;
  drop_pregradients(c);             // a pre-gradient computed from the device's own f no longer applies
  return TNML_OK;
}

extern "C" int tnml_get_f(tnml_ctx *c, float *f_out) {
  if (!c || !f_out) return fail(TNML_ERR_ARG, "NULL argument");
  if (int rc = batch_group_there(c)) return rc;
  HIP_TRY(hipSetDevice(c->device));
  return copy_f_out(c, c->f, f_out);
}

extern "C" int tnml_activation(tnml_ctx *c, int act_fn, int loss_fn, float T, int input_is_activated, float *act_out,
                               float *lossder_out) {
  if (!c) return fail(TNML_ERR_ARG, "ctx is NULL");
  if (!c->have_input) return fail(TNML_ERR_STATE, "no resident batch");
  if (lossder_out && !c->have_labels) return fail(TNML_ERR_STATE, "the loss derivative needs labels");
  if (act_fn < 0 || act_fn > 2 || loss_fn < 0 || loss_fn > 2) return fail(TNML_ERR_ARG, "unknown activation / loss");
  HIP_TRY(hipSetDevice(c->device));
  launch_activation(c->f, c->have_labels ? c->y : nullptr, c->L, c->b, c->b_pad,
                    act_fn | (input_is_activated ? 0x100 : 0), loss_fn, T, c->ftmp, c->ftmp2, c->stream);
  HIP_TRY(hipGetLastError());
  if (act_out) { int rc = copy_f_out(c, c->ftmp, act_out); if (rc) return rc; }
  if (lossder_out) { int rc = copy_f_out(c, c->ftmp2, lossder_out); if (rc) return rc; }
  return TNML_OK;
}

// ---------------------------------------------------------------------------------------------
// input gradients: g[s][i][d] = sum_l' cot[l'][s] d f[l'][s] / d X[s][i][d] (kernels_inputgrad.hip)
// ---------------------------------------------------------------------------------------------
static constexpr size_t kIgStackBytes = (size_t)256 << 20;     // the default chunk keeps the stack of pass A within this

// What the three gradient calls (input gradients, core gradients, gradient training) share: the chunk rule, the chain's LDS refusal,
// the cotangent of a chunk; the chunk itself comes from load_chunk.
// samples per pass: the caller's setting (ig_chunk or cg_chunk, rounded up to 64) or the largest multiple of 64 for which a stack
// [N][Mmax][samples] stays within kIgStackBytes, at least 64
static int grad_chunk_samples(const tnml_ctx *c, int setting) {
  if (setting > 0) return (setting + 63) / 64 * 64;
  const size_t per_sample = (size_t)c->N * c->Mmax * sizeof(float);
  return (int)std::max<size_t>(64, kIgStackBytes / per_sample / 64 * 64);
}

int tnml::largest_bond(const tnml_ctx *c) {
  int mb = 1;
  for (int v : c->bond) mb = std::max(mb, v);
  return mb;
}

// the two-pass chain kernel stages a whole core and three tiles of the largest bond in LDS; `what` names the call in the refusal
static int grad_chain_fits(const tnml_ctx *c, const char *what, int mb) {
  const size_t lds = grad_chain_lds_bytes(mb, c->D, c->L, c->N, c->scaled);
  if (lds > kLdsMax) return fail(TNML_ERR_ARG, "%s at D = %d, bond %d, L = %d: %zu bytes of LDS exceed 160 KB", what, c->D, mb, c->L, lds);
  return TNML_OK;
}

// The cotangent of the loaded chunk in cot_dev [L][bp]: columns off .. off + bc of the caller's cot [L][b], or, cot == nullptr, the
// predicted class: the prediction chain as it is, then the one-hot of its first maximum
static int chunk_cotangent(tnml_ctx *c, const float *cot, int off, int b, int bc, float *cot_dev, int bp) {
  if (cot) {
    HIP_TRY(hipMemcpy2DAsync(cot_dev, (size_t)bp * sizeof(float), cot + off, (size_t)b * sizeof(float), (size_t)bc * sizeof(float), c->L,
                             hipMemcpyHostToDevice, c->stream));
    return TNML_OK;
  }
  int rc = pred_chain(c, bc);
  if (rc) return rc;
  if (!launch_input_grad_onehot(c->fpred, c->pred_cap, c->L, bc, cot_dev, bp, c->stream)) return fail(TNML_ERR_ARG, "internal: one-hot launch refused");
  HIP_TRY(hipGetLastError());
  return TNML_OK;
}

// Input-gradient group, grown to bp samples (a multiple of 64): everything the call sizes from its chunk, and the bond table.  The
// chunk's site-major X, its staging buffer and (cot == NULL) its f are the prediction group's.
static int ig_ensure_buffers(tnml_ctx *c, int bp) {
  if (bp <= c->ig_cap && (!c->scaled || c->ig_estack)) return TNML_OK;
  bp = std::max(bp, c->ig_cap);
  const size_t N = c->N, D = c->D, L = c->L;
  HIP_TRY(hipStreamSynchronize(c->stream));
  c->ig_cap = 0;
  int rc = make_group(c, "the input-gradient buffers", {
      own_dev(c->ig_stack, N * c->Mmax * bp), own_dev(c->ig_cot, L * bp), own_dev(c->ig_g, (size_t)bp * N * D),
      own_dev(c->ig_gpix, (size_t)bp * N), own_dev(c->ig_cf, (size_t)bp), own_dev(c->ig_bond, N),
      own_dev_if(c->scaled || c->ig_estack, c->ig_estack, N * bp)});
  if (rc) return rc;
  HIP_TRY(hipMemsetAsync(c->ig_cot, 0, L * bp * sizeof(float), c->stream));     // the columns behind a chunk's samples stay finite
  c->ig_cap = bp;
  return TNML_OK;
}

// X [b][N][D] on the host, or the dataset rows idx[0..b) when X is NULL
static int input_grad_impl(tnml_ctx *c, const float *X, const int32_t *idx, int b, const float *cot, int wrt, float *grad_out, float *cf_out) {
  const int N = c->N, D = c->D, L = c->L;
  if (!c->cores_set) return fail(TNML_ERR_STATE, "cores were never set");
  const int mb = largest_bond(c);
  int rc = grad_chain_fits(c, "input gradient", mb);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(c->device));
  if (idx && (rc = ds_upload_indices(c, idx, b))) return rc;    // refuses a bad index before anything is launched
  const int chunk = std::min(grad_chunk_samples(c, c->ig_chunk), (b + 63) / 64 * 64);
  if ((rc = pred_ensure_buffers(c, chunk))) return rc;
  if ((rc = ig_ensure_buffers(c, chunk))) return rc;
  const int bp = c->ig_cap, xbp = c->pred_cap;
  HIP_TRY(hipMemcpyAsync(c->ig_bond, c->bond.data(), (size_t)(N - 1) * sizeof(int), hipMemcpyHostToDevice, c->stream));
  if (!cot && (rc = pred_table(c))) return rc;
  const bool pixels = idx && wrt == TNML_WRT_PIXELS;
  for (int off = 0; off < b; off += chunk) {
    const int bc = std::min(chunk, b - off);
    if ((rc = load_chunk(c, X, idx ? c->ds_idx : nullptr, nullptr, off, bc, nullptr))) return rc;
    if ((rc = chunk_cotangent(c, cot, off, b, bc, c->ig_cot, bp))) return rc;
    InputGradParams p{};
    p.bond = c->ig_bond; p.cores = c->cores; p.labcore = c->lab[c->lab_cur]; p.X = c->Xpred; p.cot = c->ig_cot;
    p.stack = c->ig_stack; p.g = c->ig_g; p.cf = c->ig_cf; p.core_stride = c->core_stride;
    p.b = bc; p.b_pad = bp; p.x_bpad = xbp; p.N = N; p.D = D; p.L = L; p.l_pos = c->l_pos; p.cap = c->Mmax; p.mb = mb;
    if (c->scaled) {
      const InputGradScaledParams ps{p, c->ig_estack};
      if (!launch_input_grad_scaled(ps, c->stream)) return fail(TNML_ERR_ARG, "internal: scaled input-gradient launch refused (b %d, b_pad %d)", bc, bp);
    } else
    if (!launch_input_grad(p, c->stream)) return fail(TNML_ERR_ARG, "internal: input-gradient launch refused (b %d, b_pad %d)", bc, bp);
    HIP_TRY(hipGetLastError());
    if (pixels) {
      InputGradPixels q{};
      q.g = c->ig_g; q.data = c->ds_data; q.idx = c->ds_idx + off; q.out = c->ig_gpix; q.b = bc; q.N = N; q.D = D;
      for (int s = 0; s < kMaxD; ++s) q.coef[s] = c->ds_coef[s];
      if (!launch_input_grad_pixels(q, c->stream)) return fail(TNML_ERR_ARG, "internal: pixel chain-rule launch refused");
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipMemcpyAsync(grad_out + (size_t)off * N, c->ig_gpix, (size_t)bc * N * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    } else {
      HIP_TRY(hipMemcpyAsync(grad_out + (size_t)off * N * D, c->ig_g, (size_t)bc * N * D * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    }
    if (cf_out) HIP_TRY(hipMemcpyAsync(cf_out + off, c->ig_cf, (size_t)bc * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  }
  HIP_TRY(hipStreamSynchronize(c->stream));
  return TNML_OK;
}

extern "C" int tnml_input_grad(tnml_ctx *c, const float *X, int b, const float *cot, float *grad_out, float *cf_out) {
  if (!c || !X || !grad_out) return fail(TNML_ERR_ARG, "NULL argument");
  if (c->comm) return fail(TNML_ERR_STATE, "input gradients are single-GPU only: a communicator is attached");
  if (b < 1) return fail(TNML_ERR_ARG, "empty batch");
  return input_grad_impl(c, X, nullptr, b, cot, TNML_WRT_FEATURES, grad_out, cf_out);
}

extern "C" int tnml_input_grad_indices(tnml_ctx *c, const int32_t *idx, int b, const float *cot, int wrt, float *grad_out, float *cf_out) {
  int rc = ds_usable(c);
  if (rc) return rc;
  if (!idx || !grad_out) return fail(TNML_ERR_ARG, "NULL argument");
  if (b < 1) return fail(TNML_ERR_ARG, "empty index list");
  if (wrt != TNML_WRT_FEATURES && wrt != TNML_WRT_PIXELS) return fail(TNML_ERR_ARG, "unknown wrt %d", wrt);
  if (wrt == TNML_WRT_PIXELS && c->ds_form != TNML_DATASET_PIXELS)
    return fail(TNML_ERR_STATE, "gradients with respect to pixels need a dataset in TNML_DATASET_PIXELS form");
  return input_grad_impl(c, nullptr, idx, b, cot, wrt, grad_out, cf_out);
}

extern "C" int tnml_set_input_grad_chunk(tnml_ctx *c, int samples) {
  if (!c) return fail(TNML_ERR_ARG, "ctx is NULL");
  if (samples < 0) return fail(TNML_ERR_ARG, "samples per pass %d < 0", samples);
  c->ig_chunk = samples;
  return TNML_OK;
}

// ---------------------------------------------------------------------------------------------
// core gradients: G_i = d sum_s cf[s] / d A_i for every site (kernels_coregrad.hip)
// ---------------------------------------------------------------------------------------------
// The table of CoreGradParams for the current cores: tab[0 .. N-2] the bonds, tab[N + i] the offset of core i in the flat layout of
// tnml_get_cores; total: the floats of that layout, mb: the largest bond.  `what` names the call in the refusal.
int tnml::grad_table(const tnml_ctx *c, const char *what, std::vector<int> &tab, size_t &total, int &mb) {
  const int N = c->N;
  tab.assign(2 * (size_t)N, 0);
  total = 0;
  mb = largest_bond(c);
  for (int i = 0; i < N; ++i) {
    if (i < N - 1) tab[i] = c->bond[i];
    if (total > (size_t)INT_MAX) return fail(TNML_ERR_ARG, "%s: %zu floats of cores are beyond the offset table", what, total);
    tab[N + i] = (int)total;
    total += core_elems(c, c->bond, i, c->l_pos);
  }
  return TNML_OK;
}

// Core-gradient group, grown to bp samples (a multiple of 64).  G and the table do not depend on bp; they are members all the same,
// so that a failed growth leaves nothing behind.  The chunk's site-major X, its staging buffer and (cot == NULL) its f are the
// prediction group's.
static int cg_ensure_buffers(tnml_ctx *c, int bp) {
  if (bp <= c->cg_cap && (!c->scaled || c->cg_estack)) return TNML_OK;
  bp = std::max(bp, c->cg_cap);
  const size_t N = c->N, L = c->L;
  HIP_TRY(hipStreamSynchronize(c->stream));
  c->cg_cap = 0;
  int rc = make_group(c, "the core-gradient buffers", {
      own_dev(c->cg_stackP, N * c->Mmax * bp), own_dev(c->cg_stackQ, N * c->Mmax * bp), own_dev(c->cg_cot, L * bp),
      own_dev(c->cg_cf, (size_t)bp), own_dev(c->cg_tab, 2 * N), own_dev(c->cg_G, N * c->core_stride + c->lab_elems),
      own_dev_if(c->scaled || c->cg_estack, c->cg_estack, N * bp)});
  if (rc) return rc;
  HIP_TRY(hipMemsetAsync(c->cg_cot, 0, L * bp * sizeof(float), c->stream));     // the columns behind a chunk's samples stay finite
  c->cg_cap = bp;
  return TNML_OK;
}

// The chain and the reduction over the loaded chunk of bc samples with the cotangent in cg_cot: both stacks, cf, and G (first: the
// accumulators start at zero, otherwise from G).  cg_tab holds the table of grad_table, mb is its largest bond.
static int run_core_grad_chunk(tnml_ctx *c, int bc, bool first, int mb) {
  const int bp = c->cg_cap;
  CoreGradParams p{};
  p.tab = c->cg_tab; p.cores = c->cores; p.labcore = c->lab[c->lab_cur]; p.X = c->Xpred; p.cot = c->cg_cot;
  p.stackP = c->cg_stackP; p.stackQ = c->cg_stackQ; p.G = c->cg_G; p.cf = c->cg_cf; p.core_stride = c->core_stride;
  p.b = bc; p.b_pad = bp; p.x_bpad = c->pred_cap; p.N = c->N; p.D = c->D; p.L = c->L; p.l_pos = c->l_pos; p.cap = c->Mmax; p.mb = mb;
  p.first = first;
  if (c->scaled) {
    const CoreGradScaledParams ps{p, c->cg_estack};
    if (!launch_core_grad_chain_scaled(ps, c->stream)) return fail(TNML_ERR_ARG, "internal: scaled core-gradient chain launch refused (b %d, b_pad %d)", bc, bp);
  } else
  if (!launch_core_grad_chain(p, c->stream)) return fail(TNML_ERR_ARG, "internal: core-gradient chain launch refused (b %d, b_pad %d)", bc, bp);
  HIP_TRY(hipGetLastError());
  if (!launch_core_grad_reduce(p, c->stream)) return fail(TNML_ERR_ARG, "internal: core-gradient reduction launch refused (b %d, b_pad %d)", bc, bp);
  HIP_TRY(hipGetLastError());
  return TNML_OK;
}

// X [b][N][D] on the host, or the dataset rows idx[0..b) when X is NULL
static int core_grad_impl(tnml_ctx *c, const float *X, const int32_t *idx, int b, const float *cot, float *grad_flat, size_t capacity, float *cf_out) {
  if (!c->cores_set) return fail(TNML_ERR_STATE, "cores were never set");
  size_t total;
  std::vector<int> tab;
  int mb, rc = grad_table(c, "core gradient", tab, total, mb);
  if (rc) return rc;
  if (capacity < total) return fail(TNML_ERR_ARG, "capacity %zu < %zu floats", capacity, total);
  if ((rc = grad_chain_fits(c, "core gradient", mb))) return rc;
  HIP_TRY(hipSetDevice(c->device));
  if (idx && (rc = ds_upload_indices(c, idx, b))) return rc;    // refuses a bad index before anything is launched
  const int chunk = std::min(grad_chunk_samples(c, c->cg_chunk), (b + 63) / 64 * 64);
  if ((rc = pred_ensure_buffers(c, chunk))) return rc;
  if ((rc = cg_ensure_buffers(c, chunk))) return rc;
  HIP_TRY(hipMemcpyAsync(c->cg_tab, tab.data(), tab.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));                     // (`tab` is a local: no return below leaves the copy reading it)
  if (!cot && (rc = pred_table(c))) return rc;
  for (int off = 0; off < b; off += chunk) {
    const int bc = std::min(chunk, b - off);
    if ((rc = load_chunk(c, X, idx ? c->ds_idx : nullptr, nullptr, off, bc, nullptr))) return rc;
    if ((rc = chunk_cotangent(c, cot, off, b, bc, c->cg_cot, c->cg_cap))) return rc;
    if ((rc = run_core_grad_chunk(c, bc, off == 0, mb))) return rc;
    if (cf_out) HIP_TRY(hipMemcpyAsync(cf_out + off, c->cg_cf, (size_t)bc * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  }
  HIP_TRY(hipMemcpyAsync(grad_flat, c->cg_G, total * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return TNML_OK;
}

extern "C" int tnml_core_grad(tnml_ctx *c, const float *X, int b, const float *cot, float *grad_flat, size_t capacity, float *cf_out) {
  if (!c || !X || !grad_flat) return fail(TNML_ERR_ARG, "NULL argument");
  if (c->comm) return fail(TNML_ERR_STATE, "core gradients are single-GPU only: a communicator is attached");
  if (b < 1) return fail(TNML_ERR_ARG, "empty batch");
  return core_grad_impl(c, X, nullptr, b, cot, grad_flat, capacity, cf_out);
}

extern "C" int tnml_core_grad_indices(tnml_ctx *c, const int32_t *idx, int b, const float *cot, float *grad_flat, size_t capacity, float *cf_out) {
  int rc = ds_usable(c);
  if (rc) return rc;
  if (!idx || !grad_flat) return fail(TNML_ERR_ARG, "NULL argument");
  if (b < 1) return fail(TNML_ERR_ARG, "empty index list");
  return core_grad_impl(c, nullptr, idx, b, cot, grad_flat, capacity, cf_out);
}

extern "C" int tnml_set_core_grad_chunk(tnml_ctx *c, int samples) {
  if (!c) return fail(TNML_ERR_ARG, "ctx is NULL");
  if (samples < 0) return fail(TNML_ERR_ARG, "samples per pass %d < 0", samples);
  c->cg_chunk = samples;
  return TNML_OK;
}

// ---------------------------------------------------------------------------------------------
// gradient training: optimiser steps over all cores from the core gradients (kernels_optim.hip)
// ---------------------------------------------------------------------------------------------
bool tnml::opt_stateful(const tnml_ctx *c) { return c->opt.kind == TNML_OPT_ADAM || c->opt.momentum > 0.0; }
static size_t opt_state_elems(const tnml_ctx *c) { return (size_t)c->N * c->core_stride + c->lab_elems; }     // cg_G's

// zero vel / m / v (when they exist), t = 0, bound to the current bonds and l_pos
static int opt_reset(tnml_ctx *c) {
  c->opt.t = 0;
  c->opt.bond = c->bond;
  c->opt.l_pos = c->l_pos;
  if (!c->opt_s0) return TNML_OK;
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipMemsetAsync(c->opt_s0, 0, opt_state_elems(c) * sizeof(float), c->stream));
  HIP_TRY(hipMemsetAsync(c->opt_s1, 0, opt_state_elems(c) * sizeof(float), c->stream));
  return TNML_OK;
}

extern "C" int tnml_optim_config(tnml_ctx *c, int kind, double momentum, double beta1, double beta2, double eps, int clip) {
  if (!c) return fail(TNML_ERR_ARG, "ctx is NULL");
  if (kind != TNML_OPT_SGD && kind != TNML_OPT_ADAM) return fail(TNML_ERR_ARG, "unknown optimiser %d", kind);
  if (!(momentum >= 0.0 && momentum < 1.0)) return fail(TNML_ERR_ARG, "momentum %g outside [0, 1)", momentum);
  if (!(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0)) return fail(TNML_ERR_ARG, "betas (%g, %g) outside [0, 1)", beta1, beta2);
  if (!(eps > 0.0) || !std::isfinite(eps)) return fail(TNML_ERR_ARG, "eps %g is not a positive number", eps);
  if (clip != 0 && clip != 1) return fail(TNML_ERR_ARG, "clip %d is neither 0 nor 1", clip);
  if (kind == TNML_OPT_ADAM && clip) return fail(TNML_ERR_ARG, "the clip belongs to TNML_OPT_SGD: configure TNML_OPT_ADAM with clip = 0");
  c->opt.kind = kind; c->opt.clip = clip;
  c->opt.momentum = momentum; c->opt.beta1 = beta1; c->opt.beta2 = beta2; c->opt.eps = eps;
  return opt_reset(c);
}

extern "C" int tnml_optim_reset(tnml_ctx *c) {
  if (!c) return fail(TNML_ERR_ARG, "ctx is NULL");
  return opt_reset(c);
}

// State group, on the first step of a stateful optimiser: a failed allocation leaves it empty and the call repeatable
int tnml::opt_ensure_state(tnml_ctx *c) {
  if (!opt_stateful(c) || c->opt_s0) return TNML_OK;
  HIP_TRY(hipStreamSynchronize(c->stream));
  int rc = make_group(c, "the optimiser state", {own_dev(c->opt_s0, opt_state_elems(c)), own_dev(c->opt_s1, opt_state_elems(c))});
  if (rc) return rc;
  return opt_reset(c);
}

static int opt_ensure_metrics(tnml_ctx *c, int n_steps) {
  if (n_steps <= c->opt_met_cap) return TNML_OK;
  HIP_TRY(hipStreamSynchronize(c->stream));
  c->opt_met_cap = 0;
  int rc = make_group(c, "the per-step metrics", {own_dev(c->opt_met, (size_t)n_steps * 4)});
  if (rc) return rc;
  c->opt_met_cap = n_steps;
  return TNML_OK;
}

// What a training call runs between the prediction chain of a chunk and the optimiser step: the discriminative loss of section 17
// or the negative log-likelihood of section 25.  Everything else of the call -- chunks, core gradients, optimiser tail -- is shared.
struct TrainObjective {
  bool nll;                  // false: metrics + loss derivative per chunk; true: likelihood cotangent per chunk, norm term per step
  const char *what;          // names the call in a refusal
  int act_fn, loss_fn;       // discriminative
  float T;
  bool labelled;             // likelihood: joint (labels) or marginal (the label summed)
  const double *S;           // likelihood: metric [D][D] or NULL
  int renorm;                // likelihood: the third pass of the update kernel
};

static int lnz_launch_grad(tnml_ctx *c, int n_metric, int mb, int mode, float *G);      // (with the norm term, below)

static int nst_ensure(tnml_ctx *c, int n_steps) {
  if (n_steps <= c->nst.cap) return TNML_OK;
  HIP_TRY(hipStreamSynchronize(c->stream));
  c->nst.cap = 0;
  int rc = make_group(c, "the records of the likelihood steps", {
      own_dev(c->nst.rec, (size_t)n_steps * 4), own_dev(c->nst.skip, 1),
      own_event(c->nst.ev_fork, hipEventDisableTiming), own_event(c->nst.ev_join, hipEventDisableTiming)});
  if (rc) return rc;
  c->nst.cap = n_steps;
  return TNML_OK;
}

// n_steps = ceil(n / batch) steps over X [n][N][D], y [n] on the host, or over the dataset rows idx[0..n) when X is NULL.  The
// per-chunk body is core_grad_impl's with the objective's cotangent.  out: [n_steps][3] metrics (discriminative, or NULL) or
// [n_steps][4] values (likelihood).
static int train_impl(tnml_ctx *c, const TrainObjective &obj, const float *X, const int32_t *y, const int32_t *idx, int n, int batch, float lr,
                      float wd, double *out) {
  const int N = c->N, D = c->D, L = c->L;
  const int act_fn = obj.act_fn, loss_fn = obj.loss_fn;
  const float T = obj.T;
  if (!obj.nll && (act_fn < 0 || act_fn > 2 || loss_fn < 0 || loss_fn > 2)) return fail(TNML_ERR_ARG, "unknown activation / loss");
  if (obj.nll && obj.renorm != 0 && obj.renorm != 1) return fail(TNML_ERR_ARG, "%s: renorm %d is neither 0 nor 1", obj.what, obj.renorm);
  if (!c->cores_set) return fail(TNML_ERR_STATE, "cores were never set");
  if (y)
    for (int i = 0; i < n; ++i)
      if (y[i] < 0 || y[i] >= L) return fail(TNML_ERR_ARG, "label %d of sample %d outside [0, %d)", y[i], i, L);
  size_t total;
  std::vector<int> &tab = c->opt_tab;                           // (a member: the upload below is not waited for)
  int mb, rc = grad_table(c, obj.what, tab, total, mb);
  if (rc) return rc;
  if ((rc = grad_chain_fits(c, obj.what, mb))) return rc;
  if (!obj.nll && (dataset_metrics_lds_bytes(L) > 64 * 1024 || loss_cot_lds_bytes(L) > 64 * 1024))
    return fail(TNML_ERR_ARG, "metrics / loss-derivative kernel: %d labels exceed its LDS tile", L);
  const int n_metric = obj.nll && obj.S ? 1 : 0;
  if (obj.nll && (rc = lnz_check(c, obj.what, obj.S, n_metric, mb))) return rc;
  const bool stateful = opt_stateful(c);
  if (stateful && c->opt_s0 && (c->opt.bond != c->bond || c->opt.l_pos != c->l_pos))
    return fail(TNML_ERR_STATE, "the optimiser state belongs to other bonds or another l_pos (l_pos %d then, %d now): call tnml_optim_reset",
                c->opt.l_pos, c->l_pos);
  HIP_TRY(hipSetDevice(c->device));
  if (idx && (rc = ds_upload_indices(c, idx, n))) return rc;    // refuses a bad index before anything is launched
  const int n_steps = (n + batch - 1) / batch;
  const int chunk = std::min(grad_chunk_samples(c, c->cg_chunk), (std::min(batch, n) + 63) / 64 * 64);
  if ((rc = pred_ensure_buffers(c, chunk))) return rc;
  if ((rc = cg_ensure_buffers(c, chunk))) return rc;
  if (!obj.nll && (rc = ds_ensure_metrics(c, c->pred_cap))) return rc;
  if ((rc = opt_ensure_state(c))) return rc;
  if (!obj.nll && (rc = opt_ensure_metrics(c, n_steps))) return rc;
  if (obj.nll) {
    if ((rc = lnz_ensure(c, mb, false))) return rc;
    if ((rc = nll_ensure(c, std::min(batch, n)))) return rc;
    if ((rc = nst_ensure(c, n_steps))) return rc;
  }
  const int bp = c->cg_cap, xbp = c->pred_cap;
  HIP_TRY(hipMemcpyAsync(c->cg_tab, tab.data(), tab.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
  if ((rc = pred_table(c))) return rc;
  const bool overlap = obj.nll && c->nst.overlap;
  const bool labelled = obj.nll ? obj.labelled : true;
  const long long t_start = c->opt.t;
  if (obj.nll) {                                                // once per call: the table and the metric of the norm term, the guard cleared
    if (n_metric) c->nst.metric_host.assign(obj.S, obj.S + (size_t)D * D);
    if ((rc = lnz_upload(c, tab, n_metric ? c->nst.metric_host.data() : nullptr, n_metric, false))) return rc;
    HIP_TRY(hipMemsetAsync(c->nst.skip, 0, sizeof(int), c->stream));
  }
  cores_changed(c);                                             // from here on
  for (int k = 0; k < n_steps; ++k) {
    const int s0 = k * batch, bk = std::min(batch, n - s0);
    if (overlap) {                                              // the norm walk reads the cores alone: beside the chunks, on stream2
      HIP_TRY(hipEventRecord(c->nst.ev_fork, c->stream));       // (behind the update of step k - 1 and its record)
      HIP_TRY(hipStreamWaitEvent(c->stream2, c->nst.ev_fork, 0));
      if ((rc = lnz_launch_env(c, n_metric, mb, c->stream2))) return rc;
      HIP_TRY(hipEventRecord(c->nst.ev_join, c->stream2));
    }
    for (int off = 0; off < bk; off += chunk) {
      const int bc = std::min(chunk, bk - off);
      if ((rc = load_chunk(c, X, idx ? c->ds_idx : nullptr, y, s0 + off, bc, labelled ? c->ds_ypred : nullptr))) return rc;
      if ((rc = pred_chain(c, bc))) return rc;
      if (obj.nll) {
        NllCotParams q{};
        q.f = c->fpred; q.y = labelled ? c->ds_ypred : nullptr; q.cot = c->cg_cot;
        q.terms = c->nll.terms; q.bad = c->nll.bad; q.L = L; q.b = bc; q.b_pad = bp; q.f_bpad = xbp; q.off = off; q.batch = bk;
        if (!launch_nll_cot(q, c->stream)) return fail(TNML_ERR_ARG, "internal: likelihood cotangent launch refused (b %d, b_pad %d)", bc, bp);
        HIP_TRY(hipGetLastError());
      } else {
        if (!launch_dataset_metrics(c->fpred, c->ds_ypred, L, bc, xbp, act_fn, T, c->ds_part, off == 0, c->ds_acc, c->stream))
          return fail(TNML_ERR_ARG, "internal: metrics launch refused");
        HIP_TRY(hipGetLastError());
        LossCotParams q{};
        q.f = c->fpred; q.y = c->ds_ypred; q.cot = c->cg_cot; q.L = L; q.b = bc; q.b_pad = bp; q.f_bpad = xbp;
        q.act_fn = act_fn; q.loss_fn = loss_fn; q.T = T;
        if (!launch_loss_cot(q, c->stream)) return fail(TNML_ERR_ARG, "internal: loss-derivative launch refused (b %d, b_pad %d)", bc, bp);
        HIP_TRY(hipGetLastError());
      }
      if ((rc = run_core_grad_chunk(c, bc, off == 0, mb))) return rc;
    }
    if (obj.nll) {                                              // G = Gd - Gz, the step's record, the guard
      if (!launch_nll_sum(c->nll.terms, c->nll.bad, bk, c->nll.acc, c->stream)) return fail(TNML_ERR_ARG, "internal: likelihood sum launch refused");
      HIP_TRY(hipGetLastError());
      if (overlap) HIP_TRY(hipStreamWaitEvent(c->stream, c->nst.ev_join, 0));
      else if ((rc = lnz_launch_env(c, n_metric, mb, c->stream))) return rc;
      if ((rc = lnz_launch_grad(c, n_metric, mb, 1, c->cg_G))) return rc;
      if (!launch_nll_record(c->nll.acc, c->lnz.out, c->lnz.status, c->nst.rec + (size_t)k * 4, c->nst.skip, c->stream))
        return fail(TNML_ERR_ARG, "internal: likelihood record launch refused");
      HIP_TRY(hipGetLastError());
    }
    OptimStepParams o{};
    o.tab = c->cg_tab; o.cores = c->cores; o.labcore = c->lab[c->lab_cur]; o.G = c->cg_G;
    o.s0 = stateful ? c->opt_s0 : nullptr; o.s1 = c->opt.kind == TNML_OPT_ADAM ? c->opt_s1 : nullptr;
    o.core_stride = c->core_stride; o.N = N; o.D = D; o.L = L; o.l_pos = c->l_pos;
    o.kind = c->opt.kind; o.clip = c->opt.clip; o.lr = lr; o.wd = wd;
    o.mu = c->opt.momentum; o.beta1 = c->opt.beta1; o.beta2 = c->opt.beta2; o.eps = c->opt.eps;
    o.corr1 = o.corr2 = 1.0;
    if (c->opt.kind == TNML_OPT_ADAM) {
      const double t = (double)++c->opt.t;
      o.corr1 = 1.0 - std::pow(c->opt.beta1, t);
      o.corr2 = 1.0 - std::pow(c->opt.beta2, t);
    }
    if (obj.nll) { o.renorm = obj.renorm; o.skip = c->nst.skip; }
    if (!launch_optim_step(o, c->stream)) return fail(TNML_ERR_ARG, "internal: optimiser step launch refused");
    HIP_TRY(hipGetLastError());
    if (!obj.nll) HIP_TRY(hipMemcpyAsync(c->opt_met + (size_t)k * 4, c->ds_acc, 4 * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
  }
  std::vector<double> met((size_t)n_steps * 4);
  HIP_TRY(hipMemcpyAsync(met.data(), obj.nll ? c->nst.rec : c->opt_met, met.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  int bad = -1;
  if (obj.nll) {
    int applied = 0;
    for (int k = 0; k < n_steps; ++k) {
      const double *r = &met[(size_t)k * 4];
      const int bk = std::min(batch, n - k * batch), bits = (int)r[3];
      out[(size_t)k * 4 + 0] = -(r[0] / (double)bk - r[1]);
      out[(size_t)k * 4 + 1] = r[1];
      out[(size_t)k * 4 + 2] = r[2];
      out[(size_t)k * 4 + 3] = r[3];
      if (!(bits & kNllStepNotApplied)) ++applied;
      else if (bad < 0) bad = k;
    }
    if (c->opt.kind == TNML_OPT_ADAM) c->opt.t = t_start + applied;     // (the steps behind the guard took no step)
    if (bad >= 0) {
      const int bits = (int)met[(size_t)bad * 4 + 3];
      return fail(TNML_ERR_NONFINITE, "%s: step %d of %d saw %g samples with a cotangent that is not finite (f_y == 0, or an f beyond float32: calibrate the "
                  "network), norm status %d; %d steps were applied, the cores and the optimiser state are what they left",
                  obj.what, bad, n_steps, met[(size_t)bad * 4 + 2], bits & 7, applied);
    }
    return TNML_OK;
  }
  for (int k = 0; k < n_steps; ++k) {
    if (out) for (int j = 0; j < 3; ++j) out[(size_t)k * 3 + j] = met[(size_t)k * 4 + j];
    if (met[(size_t)k * 4 + 2] > 0 && bad < 0) bad = k;
  }
  if (bad >= 0)
    return fail(TNML_ERR_NONFINITE, "step %d of %d saw %g samples with a non-finite activated output; every step ran and the cores are what they became",
                bad, n_steps, met[(size_t)bad * 4 + 2]);
  return TNML_OK;
}

static int gd_impl(tnml_ctx *c, const float *X, const int32_t *y, const int32_t *idx, int n, int batch, float lr, float wd, int act_fn,
                   int loss_fn, float T, double *metrics_out) {
  const TrainObjective obj{false, "gradient step", act_fn, loss_fn, T, true, nullptr, 0};
  return train_impl(c, obj, X, y, idx, n, batch, lr, wd, metrics_out);
}

extern "C" int tnml_gd_train_indices(tnml_ctx *c, const int32_t *idx, int n, int batch, float lr, float weight_dec, int act_fn, int loss_fn,
                                     float T, double *metrics_out) {
  int rc = ds_usable(c);
  if (rc) return rc;
  if (!idx) return fail(TNML_ERR_ARG, "NULL argument");
  if (n < 1) return fail(TNML_ERR_ARG, "empty index list");
  if (batch < 1) return fail(TNML_ERR_ARG, "batch %d < 1", batch);
  return gd_impl(c, nullptr, nullptr, idx, n, batch, lr, weight_dec, act_fn, loss_fn, T, metrics_out);
}

extern "C" int tnml_gd_step(tnml_ctx *c, const float *X, const int32_t *y, int b, float lr, float weight_dec, int act_fn, int loss_fn, float T,
                            double *metrics3) {
  if (!c || !X || !y) return fail(TNML_ERR_ARG, "NULL argument");
  if (c->comm) return fail(TNML_ERR_STATE, "gradient training is single-GPU only: a communicator is attached");
  if (b < 1) return fail(TNML_ERR_ARG, "empty batch");
  return gd_impl(c, X, y, nullptr, b, b, lr, weight_dec, act_fn, loss_fn, T, metrics3);
}

// ---------------------------------------------------------------------------------------------
// norm environments of the side a sweep runs towards (only when not inherited from the last sweep)
// ---------------------------------------------------------------------------------------------
// ---------------------------------------------------------------------------------------------
// samples and log-likelihoods of the Born distribution (kernels_sample.hip)
// ---------------------------------------------------------------------------------------------
// The group of the call, (re)sized when any member is too small: all of it or none
static int smp_ensure(tnml_ctx *c, size_t n, size_t given, size_t u, size_t tiles, size_t slots, size_t slot_sites, int mb) {
  auto &g = c->smp;
  if (g.m_cap > 0 && g.n_cap >= n && g.given_cap >= given && g.u_cap >= u && g.tiles_cap >= tiles && g.slots_cap >= slots &&
      g.slot_sites_cap >= slot_sites && g.m_cap >= mb)
    return TNML_OK;
  const size_t N = (size_t)c->N, D = (size_t)c->D;
  const size_t n_cap = std::max(g.n_cap, n), given_cap = std::max(std::max(g.given_cap, given), (size_t)1), u_cap = std::max(std::max(g.u_cap, u), (size_t)1);
  const size_t tiles_cap = std::max(g.tiles_cap, tiles), slots_cap = std::max(g.slots_cap, slots);
  const size_t slot_sites_cap = std::max(std::max(g.slot_sites_cap, slot_sites), (size_t)1);
  const int m_cap = std::max(g.m_cap, mb);
  g.n_cap = g.given_cap = g.u_cap = g.tiles_cap = g.slots_cap = g.slot_sites_cap = 0;
  g.m_cap = 0;
  HIP_TRY(hipStreamSynchronize(c->stream));
  const size_t m2 = (size_t)m_cap * m_cap;
  int rc = make_group(c, "the scratch of the sampler", {
      own_dev(g.bond, N), own_dev(g.slot_class, slots_cap), own_dev(g.tile_slot, tiles_cap), own_dev(g.tile_samples, tiles_cap * kSmpTile),
      own_dev(g.classes, n_cap), own_dev(g.given, given_cap), own_dev(g.S, D * D), own_dev(g.phi, (size_t)kSmpMaxK * D),
      own_dev(g.w, (size_t)kSmpMaxK), own_dev(g.u, u_cap), own_dev(g.env_shared, (N + 1) * m2), own_dev(g.env_slots, slot_sites_cap * m2),
      own_dev(g.stage, slots_cap * m2 * D), own_dev(g.levels, n_cap * N), own_dev(g.labels, n_cap), own_dev(g.logp, 2 * n_cap),
      own_dev(g.status, 2)});
  if (rc) return rc;
  g.n_cap = n_cap; g.given_cap = given_cap; g.u_cap = u_cap; g.tiles_cap = tiles_cap; g.slots_cap = slots_cap;
  g.slot_sites_cap = slot_sites_cap; g.m_cap = m_cap;
  return TNML_OK;
}

// The host front that tnml_sample and tnml_sample_masked (below) share: the refusals that read the same in both, each in the place
// it has in the call's own order (`what` names the call), and what both upload alike.
int tnml::smp_check_sizes(const char *what, const double *phi, const double *w, int n, int K) {
  if (!phi || !w) return fail(TNML_ERR_ARG, "%s: %s is NULL", what, phi ? "w" : "phi");
  if (n < 1) return fail(TNML_ERR_ARG, "%s: n = %d < 1", what, n);
  if (K < 2 || K > kSmpMaxK) return fail(TNML_ERR_ARG, "%s: K = %d outside [2, %d]", what, K, kSmpMaxK);
  return TNML_OK;
}

int tnml::smp_check_grid(const char *what, int K, int D, const double *phi, const double *w) {
  for (int k = 0; k < K; ++k) {
    if (!(w[k] > 0.0) || !std::isfinite(w[k])) return fail(TNML_ERR_ARG, "%s: weight %d is %g (weights are positive and finite)", what, k, w[k]);
    for (int d = 0; d < D; ++d)
      if (!std::isfinite(phi[(size_t)k * D + d])) return fail(TNML_ERR_ARG, "%s: phi[%d][%d] is not finite", what, k, d);
  }
  return TNML_OK;
}

int tnml::smp_check_classes(const char *what, const int32_t *classes, int n, int L) {
  if (classes)
    for (int s = 0; s < n; ++s)
      if (classes[s] < -1 || classes[s] >= L) return fail(TNML_ERR_ARG, "%s: class %d of sample %d outside [-1, %d)", what, (int)classes[s], s, L);
  return TNML_OK;
}

static int smp_check_uniforms(const char *what, const double *u, int n, int N) {
  if (u)
    for (size_t e = 0; e < (size_t)n * (N + 1); ++e)
      if (!(u[e] >= 0.0 && u[e] < 1.0)) return fail(TNML_ERR_ARG, "%s: u[%zu][%zu] = %g outside [0, 1)", what, e / (N + 1), e % (N + 1), u[e]);
  return TNML_OK;
}

int tnml::smp_check_state(const tnml_ctx *c, const char *what) {
  if (!c->cores_set) return fail(TNML_ERR_STATE, "cores were never set");
  if (c->comm) return fail(TNML_ERR_STATE, "%s runs on one GPU: this context has a communicator attached", what);
  return TNML_OK;
}

// the first N entries of a call's host tables: the bond to the right of every site, 1 behind the last
void tnml::smp_bond_table(const tnml_ctx *c, std::vector<int> &host) {
  for (int i = 0; i < c->N - 1; ++i) host[i] = c->bond[i];
  host[c->N - 1] = 1;
}

// the grid's metric S = sum_k w_k phi_k phi_k^T, in this order
void tnml::smp_grid_metric(std::vector<double> &S, int K, int D, const double *phi, const double *w) {
  S.assign((size_t)D * D, 0.0);
  for (int k = 0; k < K; ++k)
    for (int d = 0; d < D; ++d)
      for (int e = 0; e < D; ++e) S[(size_t)d * D + e] += w[k] * phi[(size_t)k * D + d] * phi[(size_t)k * D + e];
}

// S (from g.hostd), phi, w and the initial status words into the group g of the call (c->smp or c->smk), in this order
template <class Group>
static int smp_upload_grid(tnml_ctx *c, Group &g, int K, const double *phi, const double *w) {
  static const int init_status[2] = {0, INT_MAX};
  const size_t D = (size_t)c->D;
  HIP_TRY(hipMemcpyAsync(g.S, g.hostd.data(), D * D * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(g.phi, phi, (size_t)K * D * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(g.w, w, (size_t)K * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(g.status, init_status, sizeof init_status, hipMemcpyHostToDevice, c->stream));
  return TNML_OK;
}

extern "C" int tnml_sample(tnml_ctx *c, int n, int K, const double *phi, const double *w, const int32_t *classes, const int32_t *given,
                           int n_given, const double *u, uint64_t seed, int32_t *levels_out, int32_t *labels_out, double *logp_out) {
  const char *what = "tnml_sample";
  if (!c) return fail(TNML_ERR_ARG, "ctx is NULL");
  if (!levels_out || !labels_out || !logp_out) return fail(TNML_ERR_ARG, "tnml_sample: an output is NULL");
  int rc = smp_check_sizes(what, phi, w, n, K);
  if (rc) return rc;
  const int N = c->N, D = c->D, L = c->L;
  if (n_given < 0 || n_given > N) return fail(TNML_ERR_ARG, "tnml_sample: n_given = %d outside [0, %d]", n_given, N);
  if (n_given > 0 && !given) return fail(TNML_ERR_ARG, "tnml_sample: given is NULL with n_given = %d", n_given);
  if ((rc = smp_check_grid(what, K, D, phi, w)) || (rc = smp_check_classes(what, classes, n, L))) return rc;
  for (size_t e = 0; e < (size_t)n * n_given; ++e)
    if (given[e] < 0 || given[e] >= K)
      return fail(TNML_ERR_ARG, "tnml_sample: given level %d of sample %zu, site %zu outside [0, %d)", (int)given[e], e / n_given, e % n_given, K);
  if ((rc = smp_check_uniforms(what, u, n, N)) || (rc = smp_check_state(c, what))) return rc;
  const int mb = largest_bond(c);
  const size_t lds = std::max(sample_env_lds_bytes(mb, D), sample_walk_lds_bytes(mb, D, L, K));
  if (lds > kLdsMax || mb > kSmpMaxBond)
    return fail(TNML_ERR_SHAPE, "tnml_sample at bond %d, D = %d, L = %d, K = %d: the core, the environment and the tile of %d samples take %zu bytes of LDS "
                "(160 KB and bonds up to %d fit)", mb, D, L, K, kSmpTile, lds, kSmpMaxBond);
  // slots in the order -1, 0 .. L-1 of those the call uses; tiles of one slot each
  auto &g = c->smp;
  std::vector<int> slot_of((size_t)L + 1, -1), count((size_t)L + 1, 0);
  for (int s = 0; s < n; ++s) count[(classes ? classes[s] : -1) + 1]++;
  int n_slots = 0, n_tiles = 0;
  for (int q = 0; q <= L; ++q)
    if (count[q]) { slot_of[q] = n_slots++; n_tiles += (count[q] + kSmpTile - 1) / kSmpTile; }
  // host tables: bond [N] | slot_class [n_slots] | tile_slot [n_tiles] | tile_samples [n_tiles][16] | classes [n]
  const size_t o_slot = (size_t)N, o_tslot = o_slot + n_slots, o_tsmp = o_tslot + n_tiles, o_cls = o_tsmp + (size_t)n_tiles * kSmpTile;
  g.host.assign(o_cls + n, -1);
  smp_bond_table(c, g.host);
  {
    std::vector<int> next((size_t)L + 1, 0);
    int t = 0;
    for (int q = 0; q <= L; ++q)
      if (count[q]) {
        g.host[o_slot + slot_of[q]] = q - 1;
        next[q] = t * kSmpTile;
        const int nt = (count[q] + kSmpTile - 1) / kSmpTile;
        for (int k = 0; k < nt; ++k) g.host[o_tslot + t + k] = slot_of[q];
        t += nt;
      }
    for (int s = 0; s < n; ++s) {
      const int q = (classes ? classes[s] : -1) + 1;
      g.host[o_tsmp + next[q]++] = s;
      g.host[o_cls + s] = q - 1;
    }
  }
  smp_grid_metric(g.hostd, K, D, phi, w);
  HIP_TRY(hipSetDevice(c->device));
  rc = smp_ensure(c, (size_t)n, (size_t)n * n_given, u ? (size_t)n * (N + 1) : 0, (size_t)n_tiles, (size_t)n_slots,
                      (size_t)n_slots * (c->l_pos + 1), mb);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(g.bond, g.host.data(), (size_t)N * sizeof(int), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(g.slot_class, g.host.data() + o_slot, (size_t)n_slots * sizeof(int), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(g.tile_slot, g.host.data() + o_tslot, (size_t)n_tiles * sizeof(int), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(g.tile_samples, g.host.data() + o_tsmp, (size_t)n_tiles * kSmpTile * sizeof(int), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(g.classes, g.host.data() + o_cls, (size_t)n * sizeof(int), hipMemcpyHostToDevice, c->stream));
  if ((rc = smp_upload_grid(c, g, K, phi, w))) return rc;
  if (n_given) HIP_TRY(hipMemcpyAsync(g.given, given, (size_t)n * n_given * sizeof(int), hipMemcpyHostToDevice, c->stream));
  if (u) HIP_TRY(hipMemcpyAsync(g.u, u, (size_t)n * (N + 1) * sizeof(double), hipMemcpyHostToDevice, c->stream));
  SampleParams p{};
  p.N = N; p.D = D; p.L = L; p.l_pos = c->l_pos; p.K = K;
  p.n = n; p.n_given = n_given; p.n_tiles = n_tiles; p.n_slots = n_slots;
  p.bond = g.bond; p.cores = c->cores; p.lab = c->lab[c->lab_cur]; p.core_stride = c->core_stride;
  p.S = g.S; p.phi = g.phi; p.w = g.w; p.slot_class = g.slot_class;
  const size_t m2 = (size_t)g.m_cap * g.m_cap;
  p.env_shared = g.env_shared; p.env_slots = g.env_slots; p.env_stride = m2;
  p.stage = g.stage; p.stage_stride = m2 * D;
  p.tile_slot = g.tile_slot; p.tile_samples = g.tile_samples; p.classes = g.classes; p.given = n_given ? g.given : nullptr;
  p.u = u ? g.u : nullptr; p.seed = seed;
  p.levels = g.levels; p.labels = g.labels; p.logp = g.logp; p.status = g.status;
  if (!launch_sample(p, mb, c->stream)) {
    (void)hipStreamSynchronize(c->stream);                       // (the uploads read the caller's memory)
    return fail(TNML_ERR_SHAPE, "tnml_sample: the launch was refused (bond %d)", mb);
  }
  HIP_TRY(hipGetLastError());
  int st[2] = {0, 0};
  HIP_TRY(hipMemcpyAsync(st, g.status, sizeof st, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (st[0] & 1) return fail(TNML_ERR_NONFINITE, "tnml_sample: a core element is not finite");
  if (st[0] & 2) {
    const int s = st[1] >= 0 && st[1] < n ? st[1] : 0, cls = classes ? classes[s] : -1;
    if (cls >= 0)
      return fail(TNML_ERR_ARG, "tnml_sample: sample %d is conditioned on class %d%s, which the model gives zero weight", s, cls,
                  n_given ? " and on its given levels" : "");
    return fail(TNML_ERR_ARG, "tnml_sample: sample %d (class -1) is conditioned on given levels of zero weight, or the model is zero", s);
  }
  HIP_TRY(hipMemcpyAsync(levels_out, g.levels, (size_t)n * N * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(labels_out, g.labels, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(logp_out, g.logp, (size_t)2 * n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return TNML_OK;
}

// ---------------------------------------------------------------------------------------------
// the same given any set of known pixels (kernels_sample_masked.hip)
// ---------------------------------------------------------------------------------------------
// The group of the call, (re)sized when any member is too small: all of it or none
int tnml::smk_ensure(tnml_ctx *c, size_t tiles, size_t rows, size_t n, size_t mask, size_t u, size_t stack) {
  auto &g = c->smk;
  if (g.stack_cap > 0 && g.tiles_cap >= tiles && g.rows_cap >= rows && g.n_cap >= n && g.mask_cap >= mask && g.u_cap >= u && g.stack_cap >= stack)
    return TNML_OK;
  const size_t N = (size_t)c->N, D = (size_t)c->D;
  const size_t tiles_cap = std::max(g.tiles_cap, tiles), rows_cap = std::max(g.rows_cap, rows), n_cap = std::max(g.n_cap, n);
  const size_t mask_cap = std::max(g.mask_cap, mask), u_cap = std::max(std::max(g.u_cap, u), (size_t)1), stack_cap = std::max(g.stack_cap, stack);
  g.tiles_cap = g.rows_cap = g.n_cap = g.mask_cap = g.u_cap = g.stack_cap = 0;
  HIP_TRY(hipStreamSynchronize(c->stream));
  int rc = make_group(c, "the scratch of the masked sampler", {
      own_dev(g.bond, N), own_dev(g.tile_class, tiles_cap), own_dev(g.tile_rows, rows_cap), own_dev(g.mask, mask_cap * N),
      own_dev(g.known, n_cap * N), own_dev(g.S, D * D), own_dev(g.phi, (size_t)kSmpMaxK * D), own_dev(g.w, (size_t)kSmpMaxK),
      own_dev(g.u, u_cap), own_dev(g.stack, stack_cap), own_dev(g.E, rows_cap), own_dev(g.levels, n_cap * N), own_dev(g.labels, n_cap),
      own_dev(g.logp0, n_cap), own_dev(g.status, 2)});
  if (rc) return rc;
  g.tiles_cap = tiles_cap; g.rows_cap = rows_cap; g.n_cap = n_cap; g.mask_cap = mask_cap; g.u_cap = u_cap; g.stack_cap = stack_cap;
  return TNML_OK;
}

extern "C" int tnml_set_sample_stack_bytes(tnml_ctx *c, size_t bytes) {
  if (!c) return fail(TNML_ERR_ARG, "ctx is NULL");
  if (bytes < 1) return fail(TNML_ERR_ARG, "tnml_set_sample_stack_bytes: a budget of 0 bytes holds no tile");
  c->smk.stack_bytes = bytes;
  return TNML_OK;
}

// The group of tnml_site_conditionals (section 26), (re)sized when a member is too small: all of it or none
static int scc_ensure(tnml_ctx *c, size_t n, size_t lf) {
  auto &g = c->scc;
  if (g.lf_cap > 0 && g.n_cap >= n && g.lf_cap >= lf) return TNML_OK;
  const size_t N = (size_t)c->N, D = (size_t)c->D;
  const size_t n_cap = std::max(g.n_cap, n), lf_cap = std::max(g.lf_cap, lf);
  g.n_cap = g.lf_cap = 0;
  HIP_TRY(hipStreamSynchronize(c->stream));
  int rc = make_group(c, "the buffers of the per-pixel conditionals", {
      own_dev(g.values, (size_t)kSmpMaxK), own_dev(g.lf_next, lf_cap), own_dev(g.q, n_cap * N * D * D), own_dev(g.stats, n_cap * N * 4),
      own_dev(g.mode, n_cap * N)});
  if (rc) return rc;
  g.n_cap = n_cap; g.lf_cap = lf_cap;
  return TNML_OK;
}

// The front of tnml_sample_masked and of tnml_site_conditionals (section 26; sc: what that call adds, NULL for the sampler): the
// refusals, the class-slot tiles, the chunks under the stack budget, the launches and the errors after the run.  `what` names the call.
struct SiteCondCall {
  const double *values;
  double *q_out, *stats_out;
  int32_t *mode_out;
};

static int smk_run(tnml_ctx *c, const char *what, const SiteCondCall *sc, int n, int K, const double *phi, const double *w,
                   const int32_t *classes, const uint8_t *mask, int mask_rows, const int32_t *known, const double *u, uint64_t seed, int draw,
                   int32_t *levels_out, int32_t *labels_out, double *logp_out, double *class_logw_out) {
  int rc = smp_check_sizes(what, phi, w, n, K);
  if (rc) return rc;
  const int N = c->N, D = c->D, L = c->L;
  if (mask_rows != 1 && mask_rows != n) return fail(TNML_ERR_ARG, "%s: mask_rows = %d, neither 1 nor n = %d", what, mask_rows, n);
  if (!mask) return fail(TNML_ERR_ARG, "%s: mask is NULL", what);
  if ((rc = smp_check_grid(what, K, D, phi, w)) || (rc = smp_check_classes(what, classes, n, L))) return rc;
  for (int s = 0; s < n; ++s) {
    const uint8_t *ms = mask + (size_t)(mask_rows == 1 ? 0 : s) * N;
    for (int i = 0; i < N; ++i) {
      if (!ms[i]) continue;
      if (!known) return fail(TNML_ERR_ARG, "%s: known is NULL and the mask of sample %d has site %d set", what, s, i);
      const int32_t k = known[(size_t)s * N + i];
      if (k < 0 || k >= K) return fail(TNML_ERR_ARG, "%s: known level %d of sample %d, site %d outside [0, %d)", what, (int)k, s, i, K);
    }
  }
  if (sc && sc->values)
    for (int k = 0; k < K; ++k)
      if (!std::isfinite(sc->values[k])) return fail(TNML_ERR_ARG, "%s: values[%d] is not finite", what, k);
  if ((rc = smp_check_uniforms(what, u, n, N)) || (rc = smp_check_state(c, what))) return rc;
  const int mb = largest_bond(c);
  const int T = sc ? site_cond_tile(mb, D, L, K) : mb > kSmpMaxBond ? 0 : sample_masked_tile(mb, D, L, K);
  if (T < 1 && sc)
    return fail(TNML_ERR_SHAPE, "%s at bond %d, D = %d, L = %d, K = %d: the core, both environments and the products of one sample take "
                "%zu bytes of LDS (160 KB and bonds up to %d fit)", what, mb, D, L, K,
                std::max(sample_masked_env_lds_bytes(mb, D, 1), site_cond_lds_bytes(mb, D, K, 1)), kSccMaxBond);
  if (T < 1)
    return fail(TNML_ERR_SHAPE, "%s at bond %d, D = %d, L = %d, K = %d: the core, the environment and the products of one sample take "
                "%zu bytes of LDS (160 KB and bonds up to %d fit)", what, mb, D, L, K,
                std::max(sample_masked_env_lds_bytes(mb, D, 1), sample_masked_walk_lds_bytes(mb, D, L, K, 1)), kSmpMaxBond);
  const size_t m2 = (size_t)mb * mb, tile_stack = (size_t)T * (N + 1) * m2;
  auto &g = c->smk;
  if (g.stack_bytes / sizeof(double) < tile_stack)
    return fail(TNML_ERR_ARG, "%s: one tile of %d samples needs a stack of %zu bytes, the budget of tnml_set_sample_stack_bytes is %zu",
                what, T, tile_stack * sizeof(double), g.stack_bytes);
  // rows of a class slot: its normaliser (the empty mask), then its samples; slots in the order -1, 0 .. L-1 of those the call
  // uses (all of them for class_logw_out); tiles of T rows of one slot each, padded with empty masks
  std::vector<int> count((size_t)L + 1, 0), first_tile((size_t)L + 1, -1), next((size_t)L + 1, 0);
  for (int s = 0; s < n; ++s) count[(classes ? classes[s] : -1) + 1]++;
  int n_tiles = 0;
  for (int q = 0; q <= L; ++q)
    if (count[q] || class_logw_out) { first_tile[q] = n_tiles; next[q] = n_tiles * T + 1; n_tiles += (count[q] + 1 + T - 1) / T; }
  const size_t rows = (size_t)n_tiles * T;
  // host tables: bond [N] | tile_class [n_tiles] | tile_rows [rows] | row of sample [n]
  const size_t o_tcls = (size_t)N, o_rows = o_tcls + n_tiles, o_rof = o_rows + rows;
  g.host.assign(o_rof + n, -1);
  smp_bond_table(c, g.host);
  for (int q = 0; q <= L; ++q)
    if (first_tile[q] >= 0)
      for (int t = first_tile[q]; t < first_tile[q] + (count[q] + T) / T; ++t) g.host[o_tcls + t] = q - 1;
  for (int s = 0; s < n; ++s) {
    const int q = (classes ? classes[s] : -1) + 1;
    g.host[o_rof + s] = next[q];
    g.host[o_rows + next[q]++] = s;
  }
  smp_grid_metric(g.hostd, K, D, phi, w);
  const size_t chunk_tiles = std::min((size_t)n_tiles, g.stack_bytes / sizeof(double) / tile_stack);
  HIP_TRY(hipSetDevice(c->device));
  rc = smk_ensure(c, (size_t)n_tiles, rows, (size_t)n, (size_t)mask_rows, u ? (size_t)n * (N + 1) : 0, chunk_tiles * tile_stack);
  if (rc) return rc;
  const bool left = sc && (sc->q_out || sc->stats_out || sc->mode_out);   // (logp_out alone: the environments only)
  if (left && (rc = scc_ensure(c, (size_t)n, chunk_tiles * T * m2))) return rc;
  HIP_TRY(hipMemcpyAsync(g.bond, g.host.data(), (size_t)N * sizeof(int), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(g.tile_class, g.host.data() + o_tcls, (size_t)n_tiles * sizeof(int), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(g.tile_rows, g.host.data() + o_rows, rows * sizeof(int), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(g.mask, mask, (size_t)mask_rows * N, hipMemcpyHostToDevice, c->stream));
  if (known) HIP_TRY(hipMemcpyAsync(g.known, known, (size_t)n * N * sizeof(int), hipMemcpyHostToDevice, c->stream));
  if ((rc = smp_upload_grid(c, g, K, phi, w))) return rc;
  if (u) HIP_TRY(hipMemcpyAsync(g.u, u, (size_t)n * (N + 1) * sizeof(double), hipMemcpyHostToDevice, c->stream));
  SampleMaskedParams p{};
  p.N = N; p.D = D; p.L = L; p.l_pos = c->l_pos; p.K = K; p.n = n; p.T = T; p.mask_rows = mask_rows;
  p.bond = g.bond; p.cores = c->cores; p.lab = c->lab[c->lab_cur]; p.core_stride = c->core_stride;
  p.S = g.S; p.phi = g.phi; p.w = g.w; p.mask = g.mask; p.known = g.known;
  p.stack = g.stack; p.env_stride = m2;
  p.u = u ? g.u : nullptr; p.seed = seed;
  p.levels = g.levels; p.labels = g.labels; p.logp0 = g.logp0; p.status = g.status;
  SiteCondParams sp{};
  if (left) {
    auto &h = c->scc;
    h.values_host.resize((size_t)K);
    for (int k = 0; k < K; ++k) h.values_host[k] = sc->values ? sc->values[k] : (double)k;
    HIP_TRY(hipMemcpyAsync(h.values, h.values_host.data(), (size_t)K * sizeof(double), hipMemcpyHostToDevice, c->stream));
    sp.values = h.values; sp.lf_next = h.lf_next;
    sp.q = sc->q_out ? h.q : nullptr; sp.stats = sc->stats_out ? h.stats : nullptr; sp.mode = sc->mode_out ? h.mode : nullptr;
  }
  // chunks of whole tiles: every chunk reuses the stack, the launches of one stream follow each other
  for (size_t t0 = 0; t0 < (size_t)n_tiles; t0 += chunk_tiles) {
    p.n_tiles = (int)std::min(chunk_tiles, (size_t)n_tiles - t0);
    p.tile_class = g.tile_class + t0; p.tile_rows = g.tile_rows + t0 * T; p.E = g.E + t0 * T;
    sp.m = p;
    if (!(left ? launch_site_cond(sp, mb, c->stream) : launch_sample_masked(p, mb, draw != 0, c->stream))) {
      (void)hipStreamSynchronize(c->stream);                     // (the uploads read the caller's memory)
      return fail(TNML_ERR_SHAPE, "%s: the launch was refused (bond %d)", what, mb);
    }
  }
  HIP_TRY(hipGetLastError());
  int st[2] = {0, 0};
  g.hostE.resize(rows);
  HIP_TRY(hipMemcpyAsync(st, g.status, sizeof st, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(g.hostE.data(), g.E, rows * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  const double *E = g.hostE.data();
  auto norm_of = [&](int cls) { return E[(size_t)first_tile[cls + 1] * T]; };
  bool nonfinite = (st[0] & 1) != 0;
  for (int q = 0; q <= L; ++q)
    if (first_tile[q] >= 0 && std::isnan(norm_of(q - 1))) nonfinite = true;
  for (int s = 0; s < n; ++s)
    if (std::isnan(E[g.host[o_rof + s]])) nonfinite = true;
  if (nonfinite) return fail(TNML_ERR_NONFINITE, "%s: a core element is not finite", what);
  for (int s = 0; s < n; ++s) {
    const int cls = classes ? classes[s] : -1;
    if (std::isinf(norm_of(cls))) {
      if (cls >= 0) return fail(TNML_ERR_ARG, "%s: sample %d is conditioned on class %d, which the model gives zero weight", what, s, cls);
      return fail(TNML_ERR_ARG, "%s: the model is zero (sample %d, class -1)", what, s);
    }
    if (std::isinf(E[g.host[o_rof + s]]))
      return fail(TNML_ERR_ARG, "%s: the known pixels of sample %d (class %d) have zero weight", what, s, cls);
  }
  if (st[0] & 2) {
    const int s = st[1] >= 0 && st[1] < n ? st[1] : 0;
    return fail(TNML_ERR_ARG, "%s: the densities of sample %d (class %d) sum to nothing behind its known pixels", what, s, classes ? classes[s] : -1);
  }
  if (sc) {
    auto &h = c->scc;
    const size_t sites = (size_t)n * N;
    if (sc->q_out) HIP_TRY(hipMemcpyAsync(sc->q_out, h.q, sites * D * D * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (sc->stats_out) HIP_TRY(hipMemcpyAsync(sc->stats_out, h.stats, sites * 4 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (sc->mode_out) HIP_TRY(hipMemcpyAsync(sc->mode_out, h.mode, sites * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    if (left) HIP_TRY(hipStreamSynchronize(c->stream));
    if (logp_out)
      for (int s = 0; s < n; ++s) logp_out[s] = E[g.host[o_rof + s]] - norm_of(classes ? classes[s] : -1);
    return TNML_OK;
  }
  if (draw) {
    g.hostp.resize((size_t)n);
    HIP_TRY(hipMemcpyAsync(levels_out, g.levels, (size_t)n * N * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(labels_out, g.labels, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(g.hostp.data(), g.logp0, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
  }
  for (int s = 0; s < n; ++s) {
    const int cls = classes ? classes[s] : -1;
    logp_out[2 * (size_t)s] = draw ? g.hostp[s] : 0.0;
    logp_out[2 * (size_t)s + 1] = E[g.host[o_rof + s]] - norm_of(cls);
    if (!draw && labels_out) labels_out[s] = cls;
  }
  if (class_logw_out)
    for (int cl = 0; cl < L; ++cl) class_logw_out[cl] = std::isinf(norm_of(cl)) ? -INFINITY : norm_of(cl) - norm_of(-1);
  return TNML_OK;
}

extern "C" int tnml_sample_masked(tnml_ctx *c, int n, int K, const double *phi, const double *w, const int32_t *classes, const uint8_t *mask,
                                  int mask_rows, const int32_t *known, const double *u, uint64_t seed, int draw, int32_t *levels_out,
                                  int32_t *labels_out, double *logp_out, double *class_logw_out) {
  if (!c) return fail(TNML_ERR_ARG, "ctx is NULL");
  if (!logp_out) return fail(TNML_ERR_ARG, "tnml_sample_masked: logp_out is NULL");
  if (draw && (!levels_out || !labels_out)) return fail(TNML_ERR_ARG, "tnml_sample_masked: draw with a NULL %s", levels_out ? "labels_out" : "levels_out");
  return smk_run(c, "tnml_sample_masked", nullptr, n, K, phi, w, classes, mask, mask_rows, known, u, seed, draw, levels_out, labels_out, logp_out,
                 class_logw_out);
}

// ---------------------------------------------------------------------------------------------
// per-pixel conditionals (kernels_site_cond.hip)
// ---------------------------------------------------------------------------------------------
extern "C" int tnml_site_conditionals(tnml_ctx *c, int n, int K, const double *phi, const double *w, const double *values,
                                      const int32_t *classes, const uint8_t *mask, int mask_rows, const int32_t *known, double *q_out,
                                      double *stats_out, int32_t *mode_out, double *logp_out) {
  if (!c) return fail(TNML_ERR_ARG, "ctx is NULL");
  if (!q_out && !stats_out && !mode_out && !logp_out) return fail(TNML_ERR_ARG, "tnml_site_conditionals: every output is NULL");
  const SiteCondCall sc{values, q_out, stats_out, mode_out};
  return smk_run(c, "tnml_site_conditionals", &sc, n, K, phi, w, classes, mask, mask_rows, known, nullptr, 0, 0, nullptr, nullptr, logp_out, nullptr);
}

// ---------------------------------------------------------------------------------------------
// the gradient of the log-norm (kernels_nll.hip)
// ---------------------------------------------------------------------------------------------
// The group of the call, (re)sized when a bond outgrows it: all of it or none
// (want_G: the gradient of its own that tnml_log_norm_grad stores to; the likelihood calls subtract into cg_G and do without)
int tnml::lnz_ensure(tnml_ctx *c, int mb, bool want_G) {
  if (c->lnz.m_cap >= mb && c->lnz.m_cap > 0 && (!want_G || c->lnz.G)) return TNML_OK;
  mb = std::max(mb, c->lnz.m_cap);
  want_G = want_G || c->lnz.G;                                  // (once there, it stays a member)
  const size_t N = (size_t)c->N, D = (size_t)c->D, m2 = (size_t)mb * mb;
  c->lnz.m_cap = 0;
  HIP_TRY(hipStreamSynchronize(c->stream));
  int rc = make_group(c, "the buffers of the log-norm gradient", {
      own_dev(c->lnz.tab, 2 * N), own_dev(c->lnz.metric, N * D * D), own_dev(c->lnz.envL, (N + 1) * m2), own_dev(c->lnz.envR, (N + 1) * m2),
      own_dev(c->lnz.expL, N + 1), own_dev(c->lnz.expR, N + 1), own_dev_if(want_G, c->lnz.G, N * c->core_stride + c->lab_elems),
      own_dev(c->lnz.out, 2), own_dev(c->lnz.status, 2)});
  if (rc) return rc;
  c->lnz.m_cap = mb;
  return TNML_OK;
}

// what the calls refuse of a metric ([D][D] per site, n_metric of them) and of the bonds, before anything is launched
int tnml::lnz_check(const tnml_ctx *c, const char *what, const double *S, int n_metric, int mb) {
  const int D = c->D;
  for (int i = 0; i < n_metric; ++i)
    for (int d = 0; d < D; ++d)
      for (int e = 0; e < D; ++e) {
        const double v = S[((size_t)i * D + d) * D + e], w = S[((size_t)i * D + e) * D + d];
        if (!std::isfinite(v)) return fail(TNML_ERR_ARG, "%s: the metric of site %d is not finite at (%d, %d)", what, i, d, e);
        if (!(std::fabs(v - w) <= 1e-12 * (std::fabs(v) + std::fabs(w))))                                 // (a Gram matrix summed in two orders)
          return fail(TNML_ERR_ARG, "%s: the metric of site %d is not symmetric at (%d, %d): %.17g and %.17g", what, i, d, e, v, w);
      }
  const size_t lds = std::max(lognorm_env_lds_bytes(mb, D), lognorm_grad_lds_bytes(mb, D));
  if (mb > kLnzMaxBond || lds > kLdsMax)
    return fail(TNML_ERR_ARG, "%s at D = %d, bond %d: beyond bond %d, or %zu bytes of LDS for the two environments and their product beyond 160 KB",
                what, D, mb, kLnzMaxBond, lds);
  return TNML_OK;
}

// The norm term after lnz_check and lnz_ensure, in three parts so that a call of many steps uploads once.  lnz_upload: the table
// (tab_host outlives the upload), the status words cleared, the metric; wait: S is the caller's memory, the upload is waited for --
// otherwise S outlives it as well.  lnz_launch_env: the environment kernel on `st`, behind a clearing of the status words of its own
// when `st` is not where lnz_upload cleared them or a step was there since.  lnz_launch_grad -- mode 0: Gz stored to G, mode 1:
// G -= Gz -- the gradient kernel on the context's stream.  The status words and {sign, log|Z|} stay in the group for the reader.
static LogNormParams lnz_params(const tnml_ctx *c, int n_metric, int mode, float *G) {
  const auto &g = c->lnz;
  LogNormParams p{};
  p.N = c->N; p.D = c->D; p.L = c->L; p.l_pos = c->l_pos;
  p.metric_sites = n_metric; p.mode = mode < 0 ? 0 : mode;
  p.tab = g.tab; p.cores = c->cores; p.lab = c->lab[c->lab_cur]; p.core_stride = c->core_stride;
  p.metric = n_metric ? g.metric : nullptr;
  p.envL = g.envL; p.envR = g.envR; p.expL = g.expL; p.expR = g.expR; p.env_stride = (size_t)g.m_cap * g.m_cap;
  p.G = G; p.out = g.out; p.status = g.status;
  return p;
}

int tnml::lnz_upload(tnml_ctx *c, const std::vector<int> &tab_host, const double *S, int n_metric, bool wait) {
  auto &g = c->lnz;
  const int D = c->D;
  HIP_TRY(hipMemcpyAsync(g.tab, tab_host.data(), tab_host.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemsetAsync(g.status, 0, 2 * sizeof(int), c->stream));
  if (n_metric) {
    HIP_TRY(hipMemcpyAsync(g.metric, S, (size_t)n_metric * D * D * sizeof(double), hipMemcpyHostToDevice, c->stream));
    if (wait) HIP_TRY(hipStreamSynchronize(c->stream));         // (the upload reads the caller's memory)
  }
  return TNML_OK;
}

// (the steps of a training call: every step clears the words the one before it left, on the stream of its environment kernel)
int tnml::lnz_launch_env(tnml_ctx *c, int n_metric, int mb, hipStream_t st) {
  HIP_TRY(hipMemsetAsync(c->lnz.status, 0, 2 * sizeof(int), st));
  if (!launch_lognorm_env(lnz_params(c, n_metric, 0, nullptr), mb, st)) return fail(TNML_ERR_ARG, "internal: log-norm environment launch refused (bond %d)", mb);
  HIP_TRY(hipGetLastError());
  return TNML_OK;
}

static int lnz_launch_grad(tnml_ctx *c, int n_metric, int mb, int mode, float *G) {
  if (!launch_lognorm_grad(lnz_params(c, n_metric, mode, G), mb, c->stream)) return fail(TNML_ERR_ARG, "internal: log-norm gradient launch refused (bond %d)", mb);
  HIP_TRY(hipGetLastError());
  return TNML_OK;
}

// one call, one norm term: upload and launches on the context's stream (mode -1: no gradient launch)
static int lnz_enqueue(tnml_ctx *c, const std::vector<int> &tab_host, const double *S, int n_metric, int mb, int mode, float *G) {
  int rc = lnz_upload(c, tab_host, S, n_metric, true);
  if (rc) return rc;
  if (!launch_lognorm_env(lnz_params(c, n_metric, mode, G), mb, c->stream)) return fail(TNML_ERR_ARG, "internal: log-norm environment launch refused (bond %d)", mb);
  HIP_TRY(hipGetLastError());
  return mode >= 0 ? lnz_launch_grad(c, n_metric, mb, mode, G) : TNML_OK;
}

// the status word and {sign, log|Z|} of the launches above, after a synchronisation; `what` names the call in the refusal
static int lnz_result(tnml_ctx *c, const char *what, double *sign_log2) {
  int st2[2] = {0, 0};
  double res[2] = {0.0, 0.0};
  HIP_TRY(hipStreamSynchronize(c->stream));
  HIP_TRY(hipMemcpy(st2, c->lnz.status, 2 * sizeof(int), hipMemcpyDeviceToHost));     // (blocking copies: `st2` and `res` are locals)
  const int st = st2[0] | st2[1];
  HIP_TRY(hipMemcpy(res, c->lnz.out, 2 * sizeof(double), hipMemcpyDeviceToHost));
  if (st & 1) return fail(TNML_ERR_NONFINITE, "%s: a core element or an environment is not finite", what);
  sign_log2[0] = res[0]; sign_log2[1] = res[1];
  if (st & 2) return fail(TNML_ERR_NONFINITE, "%s: <W|W> is zero, its logarithm has no gradient", what);
  if (st & 4) return fail(TNML_ERR_NONFINITE, "%s: an element of the norm term's gradient is beyond float32", what);
  return TNML_OK;
}

extern "C" int tnml_log_norm_grad(tnml_ctx *c, const double *S, int per_site, float *grad_flat, size_t capacity, double *sign_log2) {
  if (!c) return fail(TNML_ERR_ARG, "ctx is NULL");
  if (!grad_flat || !sign_log2) return fail(TNML_ERR_ARG, "tnml_log_norm_grad: %s is NULL", grad_flat ? "sign_log2" : "grad_flat");
  if (per_site != 0 && per_site != 1) return fail(TNML_ERR_ARG, "tnml_log_norm_grad: per_site %d is neither 0 nor 1", per_site);
  if (!c->cores_set) return fail(TNML_ERR_STATE, "cores were never set");
  if (c->comm) return fail(TNML_ERR_STATE, "tnml_log_norm_grad runs on one GPU: this context has a communicator attached");
  size_t total;
  int mb, rc = grad_table(c, "tnml_log_norm_grad", c->lnz.tab_host, total, mb);
  if (rc) return rc;
  if (capacity < total) return fail(TNML_ERR_ARG, "tnml_log_norm_grad: capacity %zu < %zu floats", capacity, total);
  const int n_metric = S ? (per_site ? c->N : 1) : 0;
  if ((rc = lnz_check(c, "tnml_log_norm_grad", S, n_metric, mb))) return rc;
  HIP_TRY(hipSetDevice(c->device));
  if ((rc = lnz_ensure(c, mb, true))) return rc;
  if ((rc = lnz_enqueue(c, c->lnz.tab_host, S, n_metric, mb, 0, c->lnz.G))) return rc;
  if ((rc = lnz_result(c, "tnml_log_norm_grad", sign_log2))) return rc;
  HIP_TRY(hipMemcpyAsync(grad_flat, c->lnz.G, total * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return TNML_OK;
}

// ---------------------------------------------------------------------------------------------
// pixel-pair marginals (kernels_pair.hip)
// ---------------------------------------------------------------------------------------------
// The group of the call, (re)sized when the largest bond or the rows of a chunk outgrow it: all of it or none
static int pair_ensure(tnml_ctx *c, int mb, size_t rows) {
  auto &g = c->pair;
  if (g.m_cap >= mb && g.m_cap > 0 && g.rows_cap >= rows) return TNML_OK;
  mb = std::max(mb, g.m_cap);
  const size_t rows_cap = std::max(std::max(g.rows_cap, rows), (size_t)1);
  const size_t N = (size_t)c->N, D = (size_t)c->D, DD = D * D, m2 = (size_t)mb * mb;
  g.m_cap = 0;
  g.rows_cap = 0;
  HIP_TRY(hipStreamSynchronize(c->stream));
  int rc = make_group(c, "the buffers of the pair marginals", {
      own_dev(g.tab, 2 * N), own_dev(g.S, DD), own_dev(g.phi, (size_t)kSmpMaxK * D), own_dev(g.w, (size_t)kSmpMaxK),
      own_dev(g.values, (size_t)kSmpMaxK), own_dev(g.envL, (N + 1) * m2), own_dev(g.envR, (N + 1) * m2), own_dev(g.expL, N + 1),
      own_dev(g.expR, N + 1), own_dev(g.out, 2), own_dev(g.status, 2), own_dev(g.B, N * DD * m2), own_dev(g.q1, N * DD),
      own_dev(g.stats1, N * 3), own_dev(g.rows, N), own_dev(g.Q, rows_cap * N * DD * DD), own_dev(g.qexp, rows_cap * N * DD),
      own_dev(g.stats, rows_cap * N * 3)});
  if (rc) return rc;
  g.m_cap = mb;
  g.rows_cap = rows_cap;
  return TNML_OK;
}

extern "C" int tnml_pair_marginals(tnml_ctx *c, int K, const double *phi, const double *w, const double *values, int class_slot,
                                   const int32_t *rows, int n_rows, double *q1_out, double *stats1_out, double *q_out, double *stats_out) {
  const char *what = "tnml_pair_marginals";
  if (!c) return fail(TNML_ERR_ARG, "ctx is NULL");
  if (n_rows < 0) return fail(TNML_ERR_ARG, "%s: n_rows = %d < 0", what, n_rows);
  const bool pairs = n_rows > 0 && (q_out || stats_out);
  if (!q1_out && !stats1_out && !pairs) return fail(TNML_ERR_ARG, "%s: every output is NULL%s", what, n_rows == 0 && (q_out || stats_out) ? " or has no row" : "");
  int rc = smp_check_sizes(what, phi, w, 1, K);
  if (rc) return rc;
  const int N = c->N, D = c->D, L = c->L, DD = D * D;
  if ((rc = smp_check_grid(what, K, D, phi, w))) return rc;
  if (values)
    for (int k = 0; k < K; ++k)
      if (!std::isfinite(values[k])) return fail(TNML_ERR_ARG, "%s: values[%d] is not finite", what, k);
  if (class_slot < -1 || class_slot >= L) return fail(TNML_ERR_ARG, "%s: class slot %d outside [-1, %d)", what, class_slot, L);
  if (n_rows > 0 && !rows) return fail(TNML_ERR_ARG, "%s: rows is NULL with n_rows = %d", what, n_rows);
  auto &g = c->pair;
  {
    std::vector<char> seen((size_t)N, 0);
    for (int r = 0; r < n_rows; ++r) {
      if (rows[r] < 0 || rows[r] >= N) return fail(TNML_ERR_ARG, "%s: rows[%d] = %d outside [0, %d)", what, r, (int)rows[r], N);
      if (seen[rows[r]]) return fail(TNML_ERR_ARG, "%s: rows[%d] = %d is repeated", what, r, (int)rows[r]);
      seen[rows[r]] = 1;
    }
  }
  if ((rc = smp_check_state(c, what))) return rc;
  size_t total;
  int mb;
  if ((rc = grad_table(c, what, g.tab_host, total, mb))) return rc;
  const size_t lds = std::max(std::max(lognorm_env_lds_bytes(mb, D), pair_close_lds_bytes(mb, D, K)),
                              std::max(pair_walk_lds_bytes(mb, D), pair_stats_lds_bytes(D, K)));
  if (mb > kPairMaxBond || lds > kLdsMax)
    return fail(TNML_ERR_SHAPE, "%s at bond %d, D = %d, K = %d: two environments and their product with a core, or the table of one pair, take %zu "
                "bytes of LDS (160 KB and bonds up to %d fit)", what, mb, D, K, lds, kPairMaxBond);
  // rows in ascending site order (the longest walks start first), in chunks whose Q, exponents and statistics stay under the budget
  const size_t row_bytes = (size_t)N * ((size_t)DD * DD * sizeof(double) + (size_t)DD * sizeof(int) + 3 * sizeof(double));
  size_t chunk = 0;
  if (pairs) {
    chunk = std::min((size_t)n_rows, c->smk.stack_bytes / row_bytes);
    if (chunk < 1)
      return fail(TNML_ERR_ARG, "%s: one row needs %zu bytes, the budget of tnml_set_sample_stack_bytes is %zu", what, row_bytes, c->smk.stack_bytes);
    g.rows_host.resize((size_t)n_rows);                             // positions in the caller's list, by ascending site
    for (int r = 0; r < n_rows; ++r) g.rows_host[r] = r;
    std::sort(g.rows_host.begin(), g.rows_host.end(), [&](int x, int y) { return rows[x] < rows[y]; });
  }
  smp_grid_metric(g.hostd, K, D, phi, w);
  // S | values | phi | w: the uploads below read the group's copy, never the caller's memory
  const size_t o_val = (size_t)DD, o_phi = o_val + K, o_w = o_phi + (size_t)K * D;
  g.hostd.resize(o_w + K);
  for (int k = 0; k < K; ++k) g.hostd[o_val + k] = values ? values[k] : (double)k;
  std::copy(phi, phi + (size_t)K * D, g.hostd.begin() + o_phi);
  std::copy(w, w + K, g.hostd.begin() + o_w);
  HIP_TRY(hipSetDevice(c->device));
  if ((rc = pair_ensure(c, mb, chunk))) return rc;
  HIP_TRY(hipMemcpyAsync(g.tab, g.tab_host.data(), g.tab_host.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemsetAsync(g.status, 0, 2 * sizeof(int), c->stream));
  HIP_TRY(hipMemcpyAsync(g.S, g.hostd.data(), (size_t)DD * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(g.values, g.hostd.data() + o_val, (size_t)K * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(g.phi, g.hostd.data() + o_phi, (size_t)K * D * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(g.w, g.hostd.data() + o_w, (size_t)K * sizeof(double), hipMemcpyHostToDevice, c->stream));
  PairParams p{};
  LogNormParams &e = p.e;
  e.N = N; e.D = D; e.L = L; e.l_pos = c->l_pos; e.metric_sites = 1; e.mode = 0; e.class_plus1 = class_slot + 1;
  e.tab = g.tab; e.cores = c->cores; e.lab = c->lab[c->lab_cur]; e.core_stride = c->core_stride; e.metric = g.S;
  e.envL = g.envL; e.envR = g.envR; e.expL = g.expL; e.expR = g.expR; e.env_stride = (size_t)g.m_cap * g.m_cap;
  e.out = g.out; e.status = g.status;
  p.K = K; p.phi = g.phi; p.w = g.w; p.values = g.values; p.B = g.B; p.q1 = g.q1; p.stats1 = g.stats1;
  p.rows = g.rows; p.Q = g.Q; p.qexp = g.qexp; p.stats = g.stats;
  auto refused = [&](const char *which) {
    return fail(TNML_ERR_SHAPE, "%s: the %s launch was refused (bond %d)", what, which, mb);
  };
  if (!launch_lognorm_env(e, mb, c->stream)) return refused("environment");
  if (!launch_pair_close(p, mb, c->stream)) return refused("per-site");
  HIP_TRY(hipGetLastError());
  if (pairs) {
    std::vector<int> &sites = g.sites_host;                        // (a member: it outlives the asynchronous uploads)
    sites.resize((size_t)n_rows);
    for (int r = 0; r < n_rows; ++r) sites[r] = rows[g.rows_host[r]];
    for (size_t r0 = 0; r0 < (size_t)n_rows; r0 += chunk) {
      const size_t nr = std::min(chunk, (size_t)n_rows - r0);
      // (the chunk before this one has been copied out and waited for)
      HIP_TRY(hipMemcpyAsync(g.rows, sites.data() + r0, nr * sizeof(int), hipMemcpyHostToDevice, c->stream));
      p.n_rows = (int)nr;
      if (!launch_pair_rows(p, mb, c->stream)) return refused("row");
      HIP_TRY(hipGetLastError());
      for (size_t r = 0; r < nr; ++r) {
        const size_t to = (size_t)g.rows_host[r0 + r];
        if (q_out) HIP_TRY(hipMemcpyAsync(q_out + to * N * DD * DD, g.Q + r * N * DD * DD, (size_t)N * DD * DD * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        if (stats_out) HIP_TRY(hipMemcpyAsync(stats_out + to * N * 3, g.stats + r * N * 3, (size_t)N * 3 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
      }
      HIP_TRY(hipStreamSynchronize(c->stream));
    }
  }
  int st[2] = {0, 0};
  HIP_TRY(hipStreamSynchronize(c->stream));
  HIP_TRY(hipMemcpy(st, g.status, sizeof st, hipMemcpyDeviceToHost));      // (a blocking copy: `st` is a local)
  if (st[0] & 1) return fail(TNML_ERR_NONFINITE, "%s: a core element or an environment is not finite", what);
  if (st[0] & 2) return fail(TNML_ERR_NONFINITE, "%s: the model's norm Z is zero%s", what, class_slot >= 0 ? " for this class" : "");
  if (st[1] & 1) return fail(TNML_ERR_NONFINITE, "%s: a marginal's normaliser is zero or not finite", what);
  if (q1_out) HIP_TRY(hipMemcpyAsync(q1_out, g.q1, (size_t)N * DD * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (stats1_out) HIP_TRY(hipMemcpyAsync(stats1_out, g.stats1, (size_t)N * 3 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return TNML_OK;
}

// ---------------------------------------------------------------------------------------------
// the negative log-likelihood of a batch and its gradient over all cores (layer 2)
// ---------------------------------------------------------------------------------------------
// per-sample terms and flags of a call, and the two sums: one group sized from the samples of a call
int tnml::nll_ensure(tnml_ctx *c, int n) {
  if (n <= c->nll.n_cap) return TNML_OK;
  HIP_TRY(hipStreamSynchronize(c->stream));
  c->nll.n_cap = 0;
  const size_t cap = ((size_t)n + 1023) / 1024 * 1024;
  int rc = make_group(c, "the per-sample terms of the likelihood", {own_dev(c->nll.terms, cap), own_dev(c->nll.bad, cap), own_dev(c->nll.acc, 2)});
  if (rc) return rc;
  c->nll.n_cap = (int)cap;
  return TNML_OK;
}

// X [b][N][D] and y [b] (or NULL: the label is summed) on the host, or the dataset rows idx[0..b) with their labels (use_labels) when
// X is NULL.  grad_flat NULL: the value alone, no gradient launch.
static int nll_grad_impl(tnml_ctx *c, const char *what, const float *X, const int32_t *y, const int32_t *idx, int b, bool use_labels,
                         const double *S, float *grad_flat, size_t capacity, double *out3) {
  const int L = c->L;
  if (!c->cores_set) return fail(TNML_ERR_STATE, "cores were never set");
  if (y)
    for (int i = 0; i < b; ++i)
      if (y[i] < 0 || y[i] >= L) return fail(TNML_ERR_ARG, "label %d of sample %d outside [0, %d)", y[i], i, L);
  size_t total;
  std::vector<int> &tab = c->lnz.tab_host;                      // (a member: the uploads below are not waited for)
  int mb, rc = grad_table(c, what, tab, total, mb);
  if (rc) return rc;
  const bool grad = grad_flat != nullptr;
  if (grad && capacity < total) return fail(TNML_ERR_ARG, "%s: capacity %zu < %zu floats", what, capacity, total);
  if (grad && (rc = grad_chain_fits(c, what, mb))) return rc;
  if (!grad && c->scaled && (rc = scaled_pred_fits(c))) return rc;
  if ((rc = lnz_check(c, what, S, S ? 1 : 0, mb))) return rc;
  HIP_TRY(hipSetDevice(c->device));
  if (idx && (rc = ds_upload_indices(c, idx, b))) return rc;    // refuses a bad index before anything is launched
  const int chunk = std::min(grad_chunk_samples(c, c->cg_chunk), (b + 63) / 64 * 64);
  if ((rc = pred_ensure_buffers(c, chunk))) return rc;
  if (grad && (rc = cg_ensure_buffers(c, chunk))) return rc;
  if ((rc = lnz_ensure(c, mb, false))) return rc;
  if ((rc = nll_ensure(c, b))) return rc;
  const int xbp = c->pred_cap;
  if (grad) HIP_TRY(hipMemcpyAsync(c->cg_tab, tab.data(), tab.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
  if ((rc = pred_table(c))) return rc;
  const bool labelled = idx ? use_labels : y != nullptr;
  for (int off = 0; off < b; off += chunk) {
    const int bc = std::min(chunk, b - off);
    if ((rc = load_chunk(c, X, idx ? c->ds_idx : nullptr, y, off, bc, labelled ? c->ds_ypred : nullptr))) return rc;
    if ((rc = pred_chain(c, bc))) return rc;
    NllCotParams q{};
    q.f = c->fpred; q.y = labelled ? c->ds_ypred : nullptr; q.cot = grad ? c->cg_cot : nullptr;
    q.terms = c->nll.terms; q.bad = c->nll.bad; q.L = L; q.b = bc; q.b_pad = grad ? c->cg_cap : xbp; q.f_bpad = xbp; q.off = off; q.batch = b;
    if (!launch_nll_cot(q, c->stream)) return fail(TNML_ERR_ARG, "internal: likelihood cotangent launch refused (b %d, b_pad %d)", bc, q.b_pad);
    HIP_TRY(hipGetLastError());
    if (grad && (rc = run_core_grad_chunk(c, bc, off == 0, mb))) return rc;
  }
  if (!launch_nll_sum(c->nll.terms, c->nll.bad, b, c->nll.acc, c->stream)) return fail(TNML_ERR_ARG, "internal: likelihood sum launch refused");
  HIP_TRY(hipGetLastError());
  if ((rc = lnz_enqueue(c, tab, S, S ? 1 : 0, mb, grad ? 1 : -1, grad ? c->cg_G : nullptr))) return rc;
  double acc[2] = {0.0, 0.0}, sl[2] = {0.0, 0.0};
  if ((rc = lnz_result(c, what, sl))) return rc;               // (synchronises; `acc` is a local: its copy is not left in flight)
  HIP_TRY(hipMemcpy(acc, c->nll.acc, 2 * sizeof(double), hipMemcpyDeviceToHost));
  out3[0] = -(acc[0] / (double)b - sl[1]);
  out3[1] = sl[1];
  out3[2] = acc[1];
  if (acc[1] > 0)
    return fail(TNML_ERR_NONFINITE, "%s: %g of %d samples have a cotangent that is not finite (f_y == 0, or an f beyond float32: calibrate the network)",
                what, acc[1], b);
  if (grad) {
    HIP_TRY(hipMemcpyAsync(grad_flat, c->cg_G, total * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
  }
  return TNML_OK;
}

extern "C" int tnml_nll_grad(tnml_ctx *c, const float *X, const int32_t *y, int b, const double *S, float *grad_flat, size_t capacity, double *out3) {
  if (!c || !X || !grad_flat || !out3) return fail(TNML_ERR_ARG, "NULL argument");
  if (c->comm) return fail(TNML_ERR_STATE, "likelihood gradients are single-GPU only: a communicator is attached");
  if (b < 1) return fail(TNML_ERR_ARG, "empty batch");
  return nll_grad_impl(c, "tnml_nll_grad", X, y, nullptr, b, y != nullptr, S, grad_flat, capacity, out3);
}

extern "C" int tnml_nll_grad_indices(tnml_ctx *c, const int32_t *idx, int b, int use_labels, const double *S, float *grad_flat, size_t capacity,
                                     double *out3) {
  int rc = ds_usable(c);
  if (rc) return rc;
  if (!idx || !grad_flat || !out3) return fail(TNML_ERR_ARG, "NULL argument");
  if (b < 1) return fail(TNML_ERR_ARG, "empty index list");
  return nll_grad_impl(c, "tnml_nll_grad_indices", nullptr, nullptr, idx, b, use_labels != 0, S, grad_flat, capacity, out3);
}

extern "C" int tnml_nll_eval_indices(tnml_ctx *c, const int32_t *idx, int n, int use_labels, const double *S, double *out3) {
  int rc = ds_usable(c);
  if (rc) return rc;
  if (!idx || !out3) return fail(TNML_ERR_ARG, "NULL argument");
  if (n < 1) return fail(TNML_ERR_ARG, "empty index list");
  return nll_grad_impl(c, "tnml_nll_eval_indices", nullptr, nullptr, idx, n, use_labels != 0, S, nullptr, 0, out3);
}

extern "C" int tnml_nll_eval(tnml_ctx *c, const float *X, const int32_t *y, int b, const double *S, double *out3) {
  if (!c || !X || !out3) return fail(TNML_ERR_ARG, "NULL argument");
  if (c->comm) return fail(TNML_ERR_STATE, "likelihoods are single-GPU only: a communicator is attached");
  if (b < 1) return fail(TNML_ERR_ARG, "empty batch");
  return nll_grad_impl(c, "tnml_nll_eval", X, y, nullptr, b, y != nullptr, S, nullptr, 0, out3);
}

// ---------------------------------------------------------------------------------------------
// likelihood training: optimiser steps on the gradient of the negative log-likelihood
// ---------------------------------------------------------------------------------------------
extern "C" int tnml_nll_step(tnml_ctx *c, const float *X, const int32_t *y, int b, const double *S, float lr, float weight_dec, int renorm,
                             double *values4) {
  if (!c || !X || !values4) return fail(TNML_ERR_ARG, "NULL argument");
  if (c->comm) return fail(TNML_ERR_STATE, "likelihood training is single-GPU only: a communicator is attached");
  if (b < 1) return fail(TNML_ERR_ARG, "empty batch");
  const TrainObjective obj{true, "tnml_nll_step", 0, 0, 1.f, y != nullptr, S, renorm};
  return train_impl(c, obj, X, y, nullptr, b, b, lr, weight_dec, values4);
}

extern "C" int tnml_nll_train_indices(tnml_ctx *c, const int32_t *idx, int n, int batch, int use_labels, const double *S, float lr,
                                      float weight_dec, int renorm, double *values_out) {
  int rc = ds_usable(c);
  if (rc) return rc;
  if (!idx || !values_out) return fail(TNML_ERR_ARG, "NULL argument");
  if (n < 1) return fail(TNML_ERR_ARG, "empty index list");
  if (batch < 1) return fail(TNML_ERR_ARG, "batch %d < 1", batch);
  const TrainObjective obj{true, "tnml_nll_train_indices", 0, 0, 1.f, use_labels != 0, S, renorm};
  return train_impl(c, obj, nullptr, nullptr, idx, n, batch, lr, weight_dec, values_out);
}

extern "C" int tnml_set_nll_overlap(tnml_ctx *c, int on) {
  if (!c) return fail(TNML_ERR_ARG, "ctx is NULL");
  if (on != 0 && on != 1) return fail(TNML_ERR_ARG, "tnml_set_nll_overlap: on %d is neither 0 nor 1", on);
  c->nst.overlap = on;
  return TNML_OK;
}

// ---------------------------------------------------------------------------------------------
// narrow step: in-LDS kernel, or the large-tensor path when the merged tensor does not fit
// ---------------------------------------------------------------------------------------------
// Large-tensor group: the HBM scratch of the path and the flag words of its pipeline, sized from the bond capacity on first use
static int ensure_big(tnml_ctx *c) {
  if (c->big_ready) return TNML_OK;
  const size_t rows_cols = (size_t)c->D * c->Mmax * (1 + c->L);
  BigScratch &g = c->big;
  int rc = make_group(c, "the large-tensor scratch", {
      own_dev(g.Bf, c->bmax), own_dev(g.T, c->bmax),
      own_dev(g.part, 3 * kBigParts + 8),                      // block partials, then {step factor, the three sums}
      own_dev(g.gram, (size_t)8 * kBigMaxN * kBigMaxN), own_dev(g.rotlog, ((size_t)30 * (kBigMaxN - 1) + 2) * (kBigMaxN / 2)),
      own_dev(g.lam, 3 * kBigMaxN), own_dev(g.info, 4 + kBigMaxN), own_dev(g.VW, rows_cols * kBigMaxN),
      own_dev(g.Cb, rows_cols * c->Mmax), own_dev(g.T2, rows_cols * c->Mmax), own_dev(g.prog, 8), own_dev(c->bigpipe.flags, 4)});
  if (rc) return rc;
  HIP_TRY(hipMemset(g.prog, 0, 8 * sizeof(unsigned)));
  HIP_TRY(hipMemset(c->bigpipe.flags, 0, 4 * sizeof(unsigned)));
  c->big_ready = true;
  return TNML_OK;
}

// which path a step of these dimensions takes: 0 in-LDS, 1 large-tensor, <0 error already reported
int tnml::narrow_path(const tnml_ctx *c, int h, int g, int s, int L, int m) {
  const bool force_big = c->force_big;
  const int r = kD * h, cc = kD * g * L, nn = std::min(r, cc);
  const size_t lds = narrow_lds_bytes(h, g, s, L, m);
  if (!force_big && nn <= 64 && lds <= kLdsMax) return 0;
  if (nn > kBigMaxN)
    return fail(TNML_ERR_ARG, "min(rows, cols) = %d > %d: the Jacobi kernels handle n <= %d", nn, kBigMaxN, kBigMaxN);
  if (nn % 2) return fail(TNML_ERR_ARG, "odd matrix side %d", nn);
  return 1;
}

int tnml::run_narrow(tnml_ctx *c, NarrowParams &n, int path, bool skip_prep, hipEvent_t after_update, const BigFront *front,
                     unsigned *sig_flag, unsigned sig_val) {
  if (path == 0) {
    size_t lds = narrow_lds_bytes(n.h, n.g, n.s, n.L, n.m);
    if (n.fused && !n.prep_ready) lds = std::max(lds, prep_slice_lds_bytes(n.h, n.g, n.s, n.L));   // slice workgroups ride along
    if (lds > kLdsMax) return fail(TNML_ERR_ARG, "internal: update launch needs %zu bytes of LDS", lds);
    launch_narrow(n, lds, c->stream);
    return TNML_OK;
  }
  int rc = ensure_big(c);
  if (rc) return rc;
  n.dbg = c->dbg;                       // the capture block is this path's workspace
  n.token = ++c->pipe.token;                 // (tags the progress words of the replay that rides in the Jacobi launch)
  if (!launch_narrow_big(n, c->big, c->stream, c->check_launches, false, skip_prep, after_update, front, sig_flag, sig_val)) return fail(TNML_ERR_HIP, "%s", big_launch_error());
  return TNML_OK;
}

static int build_norm_chain(tnml_ctx *c, bool right_side) {
  // right_side: Rn[i] for i = N-1 .. 1 (sites i..N-1);  else Ln[i] for i = 0 .. N-2 (sites 0..i)
  const int N = c->N, D = c->D;
  std::vector<NormChainSite> tab;
  for (int k = 0; k < N - 1; ++k) {
    const int i = right_side ? N - 1 - k : k;
    if (i == c->l_pos) break;                       // never crosses the label site
    NormChainSite ns{};
    const int ml = c->ml(i), mr = c->mr(i);
    ns.core_off = (int)((size_t)i * c->core_stride);
    if (right_side) { ns.n_in = mr; ns.n_out = ml; ns.s_in = 1; ns.s_d = mr; ns.s_out = D * mr; }
    else { ns.n_in = ml; ns.n_out = mr; ns.s_in = D * mr; ns.s_d = mr; ns.s_out = 1; }
    ns.env_out_off = (long long)i * c->Mmax * c->Mmax;
    tab.push_back(ns);
  }
  if (tab.empty()) return TNML_OK;
  HIP_TRY(hipMemcpyAsync(c->tables, tab.data(), tab.size() * sizeof(NormChainSite), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (D != kD) {
    if (!launch_norm_chain_anyd((const NormChainSite *)c->tables, (int)tab.size(), c->cores, right_side ? c->Rn : c->Ln, c->prepG, c->Mmax, D,
                                c->stream))
      return fail(TNML_ERR_ARG, "norm environments at M = %d: %zu bytes of LDS exceed 160 KB", c->Mmax, (size_t)c->Mmax * c->Mmax * sizeof(double));
  } else
  launch_norm_chain((const NormChainSite *)c->tables, (int)tab.size(), c->cores, right_side ? c->Rn : c->Ln, c->Mmax,
                    c->stream);
  HIP_TRY(hipGetLastError());
  return TNML_OK;
}

// ---------------------------------------------------------------------------------------------
// the sweep
// ---------------------------------------------------------------------------------------------

static void prof_begin(tnml_ctx *c) { if (c->profile) (void)hipEventRecord(c->pev0, c->stream); }
static void prof_end(tnml_ctx *c, int which) {
  if (!c->profile) return;
  (void)hipEventRecord(c->pev1, c->stream);
  (void)hipEventSynchronize(c->pev1);
  float ms = 0;
  (void)hipEventElapsedTime(&ms, c->pev0, c->pev1);
  c->prof_ms[which] += ms;
  c->prof_n[which]++;
}

// ---------------------------------------------------------------------------------------------
// The sweep-relative frame, in ONE place: sweep_impl (one launch per step at D = 2), sweep_persist (one launch
// per sweep) and sweep_anyd (D = 3..8) all turn "the step at the label site, in direction d" into sites, bonds, strides and
// environment / core slots through the functions of this section, and advance the host state through them.  Relative site t is
// absolute site t (right sweep) or N-1-t (left sweep); the label core sits on relative site k, the step merges relative sites
// (k, k+1); rel_site / rel_bond / x_rel / env_rel / norm_rel address the chain by the offset dt from the label site.
// ---------------------------------------------------------------------------------------------
static int rel_site(const tnml_ctx *c, int left_dir, int dt) { return left_dir ? c->l_pos - dt : c->l_pos + dt; }
// bond between relative sites (k + dt, k + dt + 1); 1 beyond a chain end
static int rel_bond(const tnml_ctx *c, int left_dir, int dt) {
  const int i = left_dir ? c->l_pos - dt - 1 : c->l_pos + dt;
  return (i < 0 || i > c->N - 2) ? 1 : c->bond[i];
}
// features of relative site k + dt; nullptr beyond a chain end
static const float *x_rel(const tnml_ctx *c, int left_dir, int dt) {
  const int i = rel_site(c, left_dir, dt);
  return (i < 0 || i > c->N - 1) ? nullptr : c->X + (size_t)i * c->b_pad * c->D;
}
// environment over the sites behind (dt < 0: the stack the sweep grows) or ahead (dt > 0: the stack forward built) of relative
// site k + dt, kept in that site's slot; nullptr beyond a chain end (== the scalar 1)
static float *env_rel(const tnml_ctx *c, int left_dir, int dt) {
  const int i = rel_site(c, left_dir, dt);
  return (i < 0 || i > c->N - 1) ? nullptr : c->env_slot((dt > 0) != (left_dir != 0) ? c->Renv : c->Lenv, i);
}
// the same for the norm environments; dt == 0: the slot the step writes (behind norm environment of the next step)
static double *norm_rel(const tnml_ctx *c, int left_dir, int dt) {
  const int i = rel_site(c, left_dir, dt);
  return (i < 0 || i > c->N - 1) ? nullptr : c->norm_slot((dt > 0) != (left_dir != 0) ? c->Rn : c->Ln, i);
}

// pipelined step (wide_pipe_device.h): operands of the batch-side workgroups for base step j (relative index; -1 = start of a sweep),
// i.e. f from B_new(j) and the pre-gradient Z of step j+1; j is the step at the label site or the one before it.  E_t (behind
// environment of step t) lives in the behind stack's slot of relative site t-1, the ahead environment of step t in the ahead stack's
// slot of relative site t+2.
static void fill_wide_pipe(const tnml_ctx *c, WidePipeParams &w, const SweepCall &sc, int j) {
  const int N = c->N, D = c->D, left_dir = sc.left_dir;
  const int o = j - (left_dir ? N - 1 - c->l_pos : c->l_pos);      // relative site j as an offset from the label site (0 or -1)
  w = WidePipeParams{};
  w.b = c->b; w.b_pad = c->b_pad; w.L = c->L;
  w.first = j < 0;
  w.hj = rel_bond(c, left_dir, o - 1);
  w.gj = j >= 0 ? rel_bond(c, left_dir, o + 1) : 1;
  w.gn = rel_bond(c, left_dir, o + 2);
  w.hprev = rel_bond(c, left_dir, o - 2);
  w.first_ext = (j == 1);
  w.act_fn = sc.act_fn; w.loss_fn = sc.loss_fn; w.T = sc.T;
  w.x_jm1 = x_rel(c, left_dir, o - 1); w.x_j = x_rel(c, left_dir, o); w.x_jp1 = x_rel(c, left_dir, o + 1); w.x_jp2 = x_rel(c, left_dir, o + 2);
  w.Eprev = env_rel(c, left_dir, o - 2);
  w.Ecur = env_rel(c, left_dir, o - 1);
  if (j >= 1) {
    w.ext_core.base = c->core_slot(rel_site(c, left_dir, o - 1));
    w.ext_core.n_in = w.hprev; w.ext_core.n_out = w.hj;
    if (!left_dir) { w.ext_core.s_in = D * w.hj; w.ext_core.s_d = w.hj; w.ext_core.s_out = 1; }
    else { w.ext_core.s_in = 1; w.ext_core.s_d = w.hprev; w.ext_core.s_out = D * w.hprev; }
  }
  w.Gj = j >= 0 ? env_rel(c, left_dir, o + 2) : nullptr;
  w.Gn = env_rel(c, left_dir, o + 3);
  w.Bnew = c->Bnew;
  w.y = c->y; w.f = c->f;
  w.zsize = (w.first ? 1 : w.hj * D) * D * D * w.gn * c->L;
  w.slab_stride = c->zstride;
  w.slabs = c->zslabs; w.gslabs = c->gslabs; w.zred = c->zred;
  w.gcnt = c->pipe.cnt; w.tcnt = c->pipe.cnt + 16;
  w.nwide = c->pipe.nwide; w.gsz = kPipeGroupMax; w.ngroups = c->pipe.ngroups;
  w.tiles_per_wg = c->pipe.tpw; w.ntiles = c->b_pad / kTS;
  w.flag = c->pipe.cnt + 17;
  w.status = c->status;
}

static bool wide_pipe_fits(const tnml_ctx *c, const WidePipeParams &w) {
  if (wide_pipe_lds_bytes(w) > kLdsMax) return false;
  if (w.do_z && (wide_pipe_ztiles(w) > 16 * kPipeMaxZT || w.zsize + kMetricSlots > c->zstride)) return false;
  return true;
}

// a small pre-gradient (bonds of a few): one reduction level, the sixteen chunk sums through the last arriver's LDS
static void pipe_try_one_level(WidePipeParams &w) {
  if (w.do_z && w.nwide <= 256 && (size_t)16 * (w.zsize + kMetricSlots) * sizeof(float) <= wide_pipe_lds_bytes(w) - 16) {
    w.gsz = w.nwide; w.ngroups = 1; w.one_level = 1;
  }
}

// Persistent sweep, a record that would take two levels (`blk`: the step's own 32-word counter block, zeroed before the launch): the
// first R batch-side workgroups reduce runs of S 16-byte elements straight from the partials (wide_pipe_block).  R = ceil(n4 / S),
// capped at the workgroups there are (a reducer then loops over runs `R` apart).  Left as it is where the group sums of a run do not
// fit the workgroup's LDS.
static void pipe_plan_slices(WidePipeParams &w, unsigned *blk) {
  if (!w.persist || !w.do_z || w.one_level) return;
  const int S = kPipeSliceLen, n4 = (w.zsize + kMetricSlots + 3) / 4;
  if ((size_t)w.ngroups * S * 4 * sizeof(float) > wide_pipe_lds_bytes(w) - 16 || w.ngroups > kPipeGroupMax) return;
  if ((size_t)w.nwide * w.slab_stride * sizeof(float) >= ((size_t)1 << 31)) return;      // the reducers address all partials from one base
  w.slice_red = 1; w.slice_S = S; w.slice_R = std::min((n4 + S - 1) / S, w.nwide);
  w.sarrive = blk + kPstArriveWord; w.sdone = blk + kPstDoneWord;
}

// `tpw` sample tiles per batch-side workgroup: the workgroups and reduction groups of the launch
static void set_pipe_tiles(WidePipeParams &w, int tpw) {
  w.tiles_per_wg = tpw; w.nwide = (w.ntiles + tpw - 1) / tpw;
  w.ngroups = (w.nwide + kPipeGroupMax - 1) / kPipeGroupMax; w.gsz = kPipeGroupMax;
}

// Communicator path: whatever the batch-side stream still holds (f, environments, the exchanged pre-gradient) has to be complete
// before the context's stream touches it outside a split step.
static int split_join(tnml_ctx *c, bool leave_zbig = false) {
  if (c->bigpipe.pending && !leave_zbig) {
    HIP_TRY(hipStreamWaitEvent(c->stream, c->bigpipe.ev_z, 0));
    c->bigpipe.pending = false;
  }
  if (c->split.pending) {
    HIP_TRY(hipStreamWaitEvent(c->stream, c->split.ev_bat[c->split.bat], 0));
    c->split.pending = false;
  }
  c->split.done_valid = false; c->split.zsig_valid = false;
  return TNML_OK;
}

// Two-stream communicator path of the pipelined step.  Hand-offs between the two streams: sequence numbers in memory where both
// sides are kernels of this library (the update workgroup polls / stores them itself, the side stream runs a one-wave gate kernel and a
// one-thread signal kernel) -- an event costs the stream that records or waits 6-7 us even when satisfied (tools/c5_gaps.py); events
// stay for the first step of a run and for joining the side stream afterwards.
// the side stream goes on once the last update launch has ended: gate kernel on its sequence number, or its event
static int split_wait_update(tnml_ctx *c) {
  if (c->split.flags_enabled && c->split.done_valid) {
    if (!launch_big_gate(c->split.flags + 1, c->split.dseq, c->status, c->stream2)) return fail(TNML_ERR_HIP, "%s", big_launch_error());
  } else HIP_TRY(hipStreamWaitEvent(c->stream2, c->split.ev_upd[c->split.upd], 0));
  return TNML_OK;
}
// behind a batch-side launch: the pre-gradient summed over the ranks (zsize < 0: none), the sequence number and event the next update waits for
static int split_exchange(tnml_ctx *c, int zsize) {
  if (zsize >= 0) NCCL_TRY(ncclAllReduce(c->zred, c->zred, zsize + kMetricSlots, ncclFloat, ncclSum, c->comm, c->stream2));
  if (c->split.flags_enabled) {
    ++c->split.zseq;
    if (!launch_big_signal(c->split.flags, c->split.zseq, c->stream2)) return fail(TNML_ERR_HIP, "%s", big_launch_error());
    c->split.zsig_valid = true;
  }
  c->split.bat ^= 1;
  HIP_TRY(hipEventRecord(c->split.ev_bat[c->split.bat], c->stream2));
  c->split.pending = true;
  return TNML_OK;
}

// Geometry of the step at the label site.  fail: 0, or 1 the reference's un-truncated factor does not fit, 2 merged tensor / 3 new cores over the buffers
struct StepGeom {
  int left_dir, p, k;      // the step merges absolute sites (p, p + 1); k: its index counted from the chain end the sweep left
  int sb, sa;              // absolute site that keeps the behind (plain) core / that receives the label core
  int h, g, s, m;          // behind, ahead, shared bond; kept rank (the cap under the adaptive policy)
  int nn;                  // short side of the merged tensor as a matrix
  size_t bsize;            // h D D g L
  int fail;
};
static StepGeom step_geom(const tnml_ctx *c, int left_dir, int trunc_policy) {
  const int N = c->N, D = c->D, L = c->L;
  StepGeom q{};
  q.left_dir = left_dir;
  q.sb = c->l_pos; q.sa = rel_site(c, left_dir, 1);
  q.p = std::min(q.sb, q.sa);
  q.k = left_dir ? N - 1 - q.sb : q.sb;
  q.h = rel_bond(c, left_dir, -1); q.s = rel_bond(c, left_dir, 0); q.g = rel_bond(c, left_dir, 1);
  q.m = tnml_trunc_rank(trunc_policy, left_dir, q.p, N, c->ml(q.p), D, c->mr(q.p + 1), L, c->Mpol);
  q.nn = std::min(D * q.h, D * q.g * L);
  q.bsize = (size_t)q.h * D * D * q.g * L;
  if (q.m < 0) q.fail = 1;
  else if (q.bsize > c->bmax || q.m > c->Mmax) q.fail = 2;
  else if ((size_t)q.h * D * q.m > c->core_stride || (size_t)q.m * D * q.g * L > c->lab_elems) q.fail = 3;
  return q;
}
static int step_geom_error(const tnml_ctx *c, const StepGeom &q) {
  if (q.fail == 1) return fail(TNML_ERR_SHAPE, "shapes not aligned: the reference's un-truncated SVD factor does not fit "
                                               "at sites (%d, %d) (Network_class.py:914 / :949)", q.p, q.p + 1);
  if (q.fail == 2) return fail(TNML_ERR_ARG, "step at sites (%d,%d) exceeds the buffers sized for M = %d", q.p, q.p + 1, c->Mmax);
  return fail(TNML_ERR_ARG, "new cores at sites (%d,%d) exceed the buffers sized for M = %d", q.p, q.p + 1, c->Mmax);
}

// Update side of the step: what every planner passes the same way.  The per-step planners go on with fill_step_update; the
// persistent sweep adds its own red, out_ahead, metrics, stamps and hand-off fields.
static void fill_update(const tnml_ctx *c, NarrowParams &n, const StepGeom &q, int l2_flag, float lr, float wd) {
  const int D = c->D, L = c->L, h = q.h, g = q.g, s = q.s, m = q.m;
  n.L = L; n.D = D; n.h = h; n.g = g; n.s = s; n.m = m; n.bsize = (int)q.bsize;
  n.l2_flag = l2_flag ? 1 : 0; n.lr = lr; n.wd = wd;
  n.lab.base = c->lab[c->lab_cur]; n.lab.n_in = h; n.lab.n_out = s;
  n.pl.base = c->core_slot(q.sa); n.pl.n_in = s; n.pl.n_out = g;
  if (!q.left_dir) {
    n.lab.s_in = D * s * L; n.lab.s_d = s * L; n.lab.s_out = L;
    n.pl.s_in = D * g; n.pl.s_d = g; n.pl.s_out = 1;
    n.ob_s_h = D * m; n.ob_s_d = m; n.ob_s_m = 1;
    n.oa_s_m = D * g * L; n.oa_s_d = g * L; n.oa_s_g = L;
  } else {
    n.lab.s_in = L; n.lab.s_d = h * L; n.lab.s_out = D * h * L;
    n.pl.s_in = 1; n.pl.s_d = s; n.pl.s_out = D * s;
    n.ob_s_h = 1; n.ob_s_d = h; n.ob_s_m = D * h;
    n.oa_s_m = L; n.oa_s_d = m * L; n.oa_s_g = D * m * L;
  }
  if (l2_flag) {
    n.Nh = norm_rel(c, q.left_dir, -1);     // sites t < k
    n.Ng = norm_rel(c, q.left_dir, 2);      // sites t > k + 1
    n.Nh_new = norm_rel(c, q.left_dir, 0);
  }
  n.Bnew = c->Bnew;
  n.out_behind = c->core_slot(q.sb);
  n.svd_stop2 = c->svd_stop2;
  n.status = c->status; n.counters = c->counters;
}

// The update record of a per-step launch (sweep_impl at D = 2, sweep_anyd): fill_update plus where the step reads its gradient and
// writes its label core and metrics, the capture block (`dbg`: the caller's), the adaptive-rank triple, and mode 1's redirect of
// B_new away from the chain.  The caller adds chol_thr and the fused / pipelined fields.
static void fill_step_update(const tnml_ctx *c, NarrowParams &n, const StepGeom &q, const SweepCall &sc, int step, double *dbg) {
  fill_update(c, n, q, sc.l2_flag, sc.lr, sc.weight_dec);
  n.red = c->red;
  n.out_ahead = c->lab[c->lab_cur ^ 1];
  n.metrics = c->metrics + 2 * (size_t)step;
  n.dbg = dbg;
  n.stamps = (c->debug || c->stamps) ? c->dbg + 4 * c->bmax + kDbgSigma + 5 : nullptr;
  n.Bdirect = sc.Bdirect_dev;
  n.stop_after_update = sc.mode == 1;
  if (sc.trunc_policy == TNML_TRUNC_ADAPTIVE && sc.mode == 0) { n.trunc_thr = c->trunc_thr; n.left_dir = sc.left_dir; n.m_out = c->status + 1; }
  if (sc.mode == 1) { n.Bnew = c->Bscr2; n.Nh_new = nullptr; }
}

// Batch side of a classic step (wide kernel, generic-D batch kernel): gradient slabs of this step, the behind environment extended
// by the core of relative site k - 1 and, where f is not current, f of the previous step from its updated B.  `stamps` is the caller's.
static int fill_wide(const tnml_ctx *c, WideParams &w, const StepGeom &q, const SweepCall &sc) {
  const int D = c->D, ld = q.left_dir;
  w = WideParams{};
  w.b = c->b; w.b_pad = c->b_pad; w.L = c->L;
  w.h = q.h; w.g = q.g;
  w.act_fn = sc.act_fn; w.loss_fn = sc.loss_fn; w.T = sc.T;
  w.y = c->y; w.f = c->f;
  w.slabs = c->slabs; w.slab_stride = c->slab_stride; w.bsize = (int)q.bsize;
  w.x_k = x_rel(c, ld, 0);
  w.x_kp1 = x_rel(c, ld, 1);
  w.hp = 1; w.gp = 1;
  w.do_ext = (q.k >= 1);
  w.first_ext = (q.k == 1);
  if (q.k >= 1) {                                    // relative site k - 1, plain since the previous step
    const int hp = w.hp = rel_bond(c, ld, -2);
    w.x_km1 = x_rel(c, ld, -1);
    w.ext_core.base = c->core_slot(rel_site(c, ld, -1));
    w.ext_core.n_in = hp; w.ext_core.n_out = q.h;
    if (!ld) { w.ext_core.s_in = D * q.h; w.ext_core.s_d = q.h; w.ext_core.s_out = 1; }
    else { w.ext_core.s_in = 1; w.ext_core.s_d = hp; w.ext_core.s_out = D * hp; }
    w.Hprev = env_rel(c, ld, -2);
    w.Hcur = env_rel(c, ld, -1);
  }
  if (c->Bnew_valid && !c->f_current) {
    // f of the previous step from its updated B: that step acted on relative sites k - 1, k
    if (q.k < 1 || c->prev_h != w.hp || c->prev_g != q.s)
      return fail(TNML_ERR_STATE, "internal: previous-step dims (%d,%d) do not match (%d,%d)", c->prev_h, c->prev_g, w.hp, q.s);
    w.do_f = 1;
    w.gp = q.s;
    w.Gprev = env_rel(c, ld, 1);                     // sites t > k
    w.Bprev = c->Bnew;
  }
  w.Gcur = env_rel(c, ld, 2);
  return TNML_OK;
}

// algorithmic work of a step: environments, features of three sites, f, labels; gradient + f products and the extension
static void add_step_work(const tnml_ctx *c, const StepGeom &q, double &bytes, double &flops) {
  const double bb = (double)c->b, D = c->D, L = c->L, h = q.h, g = q.g;
  bytes += 4.0 * bb * (2.0 * h + g + 3.0 * D + 2.0 * L + 1.0);
  flops += 4.0 * bb * D * D * h * g * L + 2.0 * bb * D * h * h;
}

// the step is planned: the label moves on to site sa, the bond between the two sites is the kept rank, the other label buffer is current
static void advance_frame(tnml_ctx *c, const StepGeom &q, int m_kept) {
  c->bond[q.p] = m_kept;
  c->l_pos = q.sa;
  c->lab_cur ^= 1;
  c->prev_h = q.h; c->prev_g = q.g; c->prev_left_dir = q.left_dir;
}

// the capture block (tnml_get_step_debug) describes this step
static void note_last_step(tnml_ctx *c, const StepGeom &q) {
  c->last_bsize = (int)q.bsize; c->last_n = q.nn; c->last_h = q.h; c->last_g = q.g; c->last_left_dir = q.left_dir;
}

// after the launches of a step of the per-step planners; f_stored: the batch-side work of the step stored its f already
static int finish_step(tnml_ctx *c, const StepGeom &q, const SweepCall &sc, int step, bool f_stored) {
  int m_kept = q.m;
  note_last_step(c, q);
  if (sc.trunc_policy == TNML_TRUNC_ADAPTIVE) {       // the kept rank is decided on the device: one sync per step
    HIP_TRY(hipMemcpyAsync(&m_kept, c->status + 1, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (m_kept < 1 || m_kept > q.m) return fail(TNML_ERR_NONFINITE, "adaptive truncation returned rank %d (cap %d)", m_kept, q.m);
  }
  advance_frame(c, q, m_kept);
  if (c->seg_starting) {                           // first step of a segment (tnml_set_any_position): the behind stack is no longer forward's
    (q.left_dir ? c->envs_valid_R : c->envs_valid_L) = false;
    c->seg_starting = false;
  }
  c->cnt_steps += 1;
  add_step_work(c, q, c->cnt_bytes, c->cnt_flops);
  c->Bnew_valid = true;
  c->f_current = f_stored;
  if (c->check_launches) HIP_TRY(hipGetLastError());
  if (c->sync_interval > 0 && (step + 1) % c->sync_interval == 0) HIP_TRY(hipStreamSynchronize(c->stream));
  return TNML_OK;
}

// mode 1 (standalone update_B) ends here: the behind environment list grew (as update_B does, Network_class.py:637-652), nothing else changes
static int finish_update_only(tnml_ctx *c, const StepGeom &q, float *metrics_out) {
  note_last_step(c, q);
  HIP_TRY(hipGetLastError());
  if (metrics_out) {
    HIP_TRY(hipMemcpyAsync(metrics_out, c->metrics, 2 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
  }
  return TNML_OK;
}

// after the last step of a call: valid norm stacks, f from the last updated B (what sweep_step returns, Network_class.py:573), copies out
static int finish_sweep(tnml_ctx *c, const SweepCall &sc) {
  const int left_dir = sc.left_dir, l2_flag = sc.l2_flag, nblk = sc.nblk;
  float *const metrics_out = sc.metrics_out, *const f_out = sc.f_out;
  // the behind norm stack is whole (the one valid for the opposite direction) once the sweep is complete; mid-sweep the ahead one stays usable
  bool &behind = left_dir ? c->Rn_valid : c->Ln_valid, &ahead = left_dir ? c->Ln_valid : c->Rn_valid;
  const bool complete = c->l_pos == (left_dir ? 0 : c->N - 1);
  behind = l2_flag && complete;
  if (!l2_flag || complete) ahead = false;
  if (!c->f_current) {
    // the step that just ended acted on relative sites (k - 1, k) seen from the label site
    WideParams w{};
    w.b = c->b; w.b_pad = c->b_pad; w.L = c->L;
    w.hp = c->prev_h; w.gp = c->prev_g;
    w.Hprev = env_rel(c, left_dir, -2);
    w.Gprev = env_rel(c, left_dir, 1);
    w.x_km1 = x_rel(c, left_dir, -1);
    w.x_k = x_rel(c, left_dir, 0);
    w.Bprev = c->Bnew;
    w.f = c->f;
    prof_begin(c);
    if (c->D == kD) launch_f_only(w, nblk, c->stream);
    else {
      w.do_f = 1;
      if (!launch_batch_anyd(w, c->D, nblk, false, c->stream))
        return fail(TNML_ERR_ARG, "f of the last step at D = %d needs %zu bytes of LDS", c->D, anyd_batch_lds_bytes(c->D, w.hp, w.gp, 1, 1, c->L));
      c->sweep_launches += 1;
    }
    prof_end(c, 1);
    HIP_TRY(hipGetLastError());
    c->f_current = true;
  }
  if (sc.sw_ev1) HIP_TRY(hipEventRecord(sc.sw_ev1, c->stream));
  if (metrics_out) HIP_TRY(hipMemcpyAsync(metrics_out, c->metrics, (size_t)sc.n_steps * 2 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  if (f_out) { int rc = copy_f_out(c, c->f, f_out); if (rc) return rc; }
  if (metrics_out || f_out) {
    HIP_TRY(hipStreamSynchronize(c->stream));
    return check_status(c);
  }
  return TNML_OK;
}

// ---------------------------------------------------------------------------------------------
// Persistent sweep: the whole sweep as ONE launch of sweep_persist_kernel (kernels_narrow.hip).  Applies to a full sweep that
// starts right after tnml_forward on a single GPU, fixed or reference truncation (all bond dimensions are known before the
// launch), every step in the in-LDS regime, no per-step capture.  Every step is planned through the shared frame functions above (the
// records ARE the per-step path's NarrowParams / WidePipeParams, plus the hand-off fields), and the host bookkeeping -- bonds, label
// position, label-core buffer -- advances through advance_frame.  Returns 1 if the sweep was enqueued, 0 if this sweep has to take
// the per-step path (state untouched), < 0 on error.
// ---------------------------------------------------------------------------------------------
// What the update role of the persistent kernels takes as compile-time constants (PersistArgs, kernels_narrow.hip) must be what the
// record says: a mode planned here later and not taught to the kernel would otherwise be ignored silently.
static bool persist_record_ok(const NarrowParams &n) {
  return n.pipe == 1 && n.persist == 1 && n.flag && !n.fused && !n.prep_ready && !n.Bdirect && !n.dbg && !n.stop_after_update &&
         !(n.trunc_thr > 0.0) && !n.m_out && !n.zpoll_flag && !n.done_flag && !n.sync && n.wait_count == 0;
}

static int sweep_persist(tnml_ctx *c, const SweepCall &sc) {
  const int N = c->N, D = c->D, L = c->L, left_dir = sc.left_dir, n_steps = sc.n_steps, trunc_policy = sc.trunc_policy;
  // (cycle stamps alone -- tnml_debug_enable(ctx, 2) -- are allowed: they are taken at the middle step of the sweep)
  if (!c->persist_enabled || !c->pipe.enabled || c->comm || c->debug || c->profile || c->check_launches) return 0;
  if (trunc_policy == TNML_TRUNC_ADAPTIVE || n_steps != N - 1 || c->force_big) return 0;
  if (!c->f_current || c->Bnew_valid) return 0;
  // state the planning loop advances; restored if some step does not fit
  const std::vector<int> bond0 = c->bond;
  const int l_pos0 = c->l_pos, lab_cur0 = c->lab_cur;
  auto give_up = [&]() { c->bond = bond0; c->l_pos = l_pos0; c->lab_cur = lab_cur0; return 0; };
  const int buf = c->pst_cur;
  HIP_TRY(hipEventSynchronize(c->pst_ev[buf]));              // the copy that last read this staging buffer is done
  PersistStep *st = c->pst_host[buf];
  st[n_steps] = PersistStep{};
  WidePipeParams &pro = st[n_steps].w;                       // the batch side's prologue rides in the record after the last step
  const int ntiles = c->b_pad / kTS;
  // one sample tile per batch-side workgroup while the device has the CUs (the reduced pre-gradient of step k+1 has to be there
  // when step k ends: with two tiles per workgroup it arrived ~2 us late behind a 40-round SVD); fixed for the whole launch --
  // a workgroup keeps its samples from step to step
  int tpw = c->pipe.tpw;
  while ((ntiles + tpw - 1) / tpw + 1 + kPersistHelpers > c->num_cus) ++tpw;
  const int nwide = (ntiles + tpw - 1) / tpw;
  const int nH = kPersistHelpers;
  if (1 + nH + nwide > c->num_cus) return 0;                 // every workgroup of the launch must be resident
  const int Mcap = c->Mmax;
  const size_t pbytes = persist_lds_bytes(Mcap);
  unsigned *fl = c->pst_flags;                               // [0] B_new token, [2] Z ready, [3] end of step: behind core stored, [4] abort, [5] A' / 1 / sigma stored
  float *zr2[2] = {c->zred, c->zred2};
  size_t lds_narrow = 0, lds_wide = 0, lds_help = 0;
  // prologue: Z_0 from forward's f
  fill_wide_pipe(c, pro, sc, -1);
  pro.do_ext = 0; pro.wait_flag = 0; pro.do_z = 1; pro.do_f = 0;
  set_pipe_tiles(pro, tpw);
  pro.wg0 = 1 + nH; pro.persist = 1; pro.zred = zr2[0]; pro.zready = fl + 2; pro.zpublish = 1; pro.abort_flag = fl + 4;
  pro.gcnt = c->pst_cnt + (size_t)n_steps * 32; pro.tcnt = pro.gcnt + 16;
  if (!wide_pipe_fits(c, pro)) return give_up();
  pipe_try_one_level(pro);
  if (c->persist_slices) pipe_plan_slices(pro, pro.gcnt);
  int n_slice = pro.slice_red;
  lds_wide = wide_pipe_lds_bytes(pro);
  double bytes = 0, flops = 0;
  for (int k = 0; k < n_steps; ++k) {
    const StepGeom q = step_geom(c, left_dir, trunc_policy);
    if (q.fail) return give_up();                            // the per-step path reports it (the reference's ValueError, the buffers)
    const int h = q.h, g = q.g, s = q.s, m = q.m;
    const size_t nlds = narrow_lds_bytes(h, g, s, L, m);
    if (q.nn > 64 || (q.nn & 1) || nlds + pbytes > kLdsMax || h > Mcap || m > Mcap || q.bsize > 8192) return give_up();
    PersistStep &ps = st[k];
    ps = PersistStep{};
    // ---- update + SVD workgroup (Nh / Ng: only "is there one", the values are in LDS)
    NarrowParams &n = ps.n;
    fill_update(c, n, q, sc.l2_flag, sc.lr, sc.weight_dec);
    // the label core is written once, by the last step: into the buffer the per-step sequence would have ended on
    n.out_ahead = c->lab[(c->lab_cur + (n_steps - k)) & 1];
    n.write_ahead = (k == n_steps - 1);
    n.metrics = c->metrics + 2 * (size_t)k;
    n.chol_thr = c->chol_thr;
    n.stamps = (c->stamps && k == n_steps / 2) ? c->dbg + 4 * c->bmax + kDbgSigma + 5 : nullptr;
    n.pipe = 1; n.persist = 1; n.z_first = (k == 0);
    fill_wide_pipe(c, ps.w, sc, k);
    WidePipeParams &wp = ps.w;
    const int zr = k == 0 ? 1 : wp.hprev * D;
    if (zr > 64) return give_up();
    n.z_rows = zr; n.zsize = zr * D * D * g * L;
    n.zred = zr2[k & 1]; n.red = n.zred;
    n.prepB = c->prepB; n.prepG = c->prepG; n.prepRaw = c->prepRaw;
    n.pready = c->pst_cnt + (size_t)k * 32 + 21; n.pwant = (unsigned)nH;
    n.flag = fl + 0; n.token = (unsigned)k + 1;
    n.Apub = c->Apub;
    n.aflag = fl + 5; n.coreflag = fl + 3; n.coretoken = (unsigned)k + 1; n.abort_flag = fl + 4;
    n.Mcap = Mcap;
    if (!persist_record_ok(n)) return give_up();             // (a plan the persistent kernels do not know: the per-step path runs it)
    lds_narrow = std::max(lds_narrow, nlds);
    // ---- batch-side workgroups: f from B_new(k), pre-gradient of step k+1
    wp.do_ext = k >= 1; wp.do_f = 1; wp.wait_flag = 1;
    wp.do_z = (k + 1 <= N - 2);
    set_pipe_tiles(wp, tpw);
    wp.wg0 = 1 + nH; wp.persist = 1; wp.flag = fl + 0; wp.token = (unsigned)k + 1;
    wp.coreflag = fl + 3; wp.corewant = (unsigned)k; wp.zready = fl + 2; wp.zpublish = (unsigned)k + 2; wp.abort_flag = fl + 4;
    wp.zred = zr2[(k + 1) & 1];
    wp.gcnt = c->pst_cnt + (size_t)k * 32; wp.tcnt = wp.gcnt + 16;
    wp.stamps = n.stamps;
    if (!wide_pipe_fits(c, wp)) return give_up();
    pipe_try_one_level(wp);
    if (c->persist_slices) pipe_plan_slices(wp, wp.gcnt);
    n_slice += wp.slice_red;
    lds_wide = std::max(lds_wide, wide_pipe_lds_bytes(wp));
    // ---- helper workgroups: T_k, T_k . Ng beside the SVD of step k-1; the three projections once its behind core is published
    PersistHelperParams &t = ps.t;
    t.zr = zr; t.s = s; t.g = g; t.L = L; t.h = h; t.l2_flag = n.l2_flag;
    t.W = k == 0 ? nullptr : c->Bnew;
    t.lab = n.lab; t.pl = n.pl; t.Ng = n.Ng;
    t.T = c->Tbuf[k & 1]; t.TN = c->TNbuf[k & 1]; t.Z = zr2[k & 1];
    t.prepRaw = c->prepRaw; t.prepB = c->prepB; t.prepG = c->prepG; t.Apub = c->Apub;
    t.flag = fl + 0; t.want = (unsigned)k; t.aflag = fl + 5; t.awant = (unsigned)k; t.zready = fl + 2; t.zwant = (unsigned)k + 1;
    t.tcnt = c->pst_cnt + (size_t)k * 32 + 20; t.pcnt = c->pst_cnt + (size_t)k * 32 + 21;
    t.abort_flag = fl + 4; t.status = c->status; t.stamps = n.stamps;
    // Z_k reduced in slices: its reducers count themselves done in their step's block, and all of them is what the helpers wait for
    // (no last finisher, no flag hop); otherwise the single writer stores k + 1 into the launch's Z word
    const WidePipeParams &zsrc = k == 0 ? pro : st[k - 1].w;
    if (zsrc.slice_red) { t.zready = zsrc.sdone; t.zwant = (unsigned)zsrc.slice_R; }
    lds_help = std::max(lds_help, persist_helper_lds_bytes(zr, s, g, L, h, nH));
    if ((size_t)zr * D * D * g * L + kMetricSlots > (size_t)c->zstride) return give_up();
    // ---- the bookkeeping of the per-step path (the capture block belongs to the stamped step, if there is one)
    advance_frame(c, q, m);
    if (!c->stamps || k <= n_steps / 2) note_last_step(c, q);
    add_step_work(c, q, bytes, flops);
  }
  const size_t lds = c->persist_mode >= 2 ? lds_narrow + pbytes : std::max(std::max(lds_narrow + pbytes, lds_wide), lds_help);
  if (lds > kLdsMax || lds_wide > kLdsMax || lds_help > kLdsMax) return give_up();
  const int persist_off = (int)((lds - pbytes) & ~(size_t)15);
  for (int k = 0; k < n_steps; ++k) st[k].n.persist_off = persist_off;
  // ---- the steps a compiled shape fits (kPersistShapes): every constant of the shape against the update AND the helper record.  One
  // launch has the bodies of one shape: the first one met (a chain has one uniform bond); mode 2 has the generic kernels only.
  int shape = 0, n_fixed = 0;
  if (c->shape_kernels && c->persist_mode < 2)
    for (int k = 0; k < n_steps; ++k) {
      const NarrowParams &n = st[k].n;
      const PersistHelperParams &t = st[k].t;
      const int id = persist_step_shape(n.h, n.g, n.s, n.m, n.L, n.z_rows, n.bsize, nH);
      if (!id || (shape && id != shape) || n.D != kD) continue;
      if (persist_step_shape(t.h, t.g, t.s, n.m, t.L, t.zr, n.bsize, nH) != id) continue;
      shape = id; st[k].shape = id; ++n_fixed;
    }
  // ---- enqueue: records, zeroed flags and counters, one launch
  HIP_TRY(hipMemcpyAsync(c->pst_dev, st, (size_t)(n_steps + 1) * sizeof(PersistStep), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipEventRecord(c->pst_ev[buf], c->stream));
  c->pst_cur ^= 1;
  HIP_TRY(hipMemsetAsync(c->pst_flags, 0, 8 * sizeof(unsigned), c->stream));
  HIP_TRY(hipMemsetAsync(c->pst_cnt, 0, (size_t)(n_steps + 1) * 32 * sizeof(unsigned), c->stream));
  if (c->persist_mode >= 2) {
    // one launch per role: the helper and batch-side grids start once the records and zeroed flags are in place, and the
    // context's stream continues only after all three have ended
    HIP_TRY(hipEventRecord(c->ev_p0, c->stream));
    HIP_TRY(hipStreamWaitEvent(c->stream2, c->ev_p0, 0));
    HIP_TRY(hipStreamWaitEvent(c->stream3, c->ev_p0, 0));
    launch_sweep_persist_split(c->pst_dev, n_steps, nH, nwide, lds, lds_help, lds_wide, c->stream, c->stream2, c->stream3);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c->ev_p2, c->stream2));
    HIP_TRY(hipEventRecord(c->ev_p3, c->stream3));
    HIP_TRY(hipStreamWaitEvent(c->stream, c->ev_p2, 0));
    HIP_TRY(hipStreamWaitEvent(c->stream, c->ev_p3, 0));
  } else {
    if (!launch_sweep_persist(c->pst_dev, n_steps, nH, 1 + nH + nwide, lds, c->stream, shape))
      return fail(TNML_ERR_STATE, "no persistent sweep kernel for step shape %d", shape);
    HIP_TRY(hipGetLastError());
  }
  c->fixed_steps = n_fixed; c->slice_steps = n_slice;
  c->cnt_steps += n_steps; c->cnt_bytes += bytes; c->cnt_flops += flops;
  c->sweep_launches += 1; c->step_launches += n_steps; c->persist_sweeps += 1;
  c->Bnew_valid = true; c->f_current = true; drop_pregradients(c);
  return 1;
}

// mode 0: n_steps full steps.  mode 1 (standalone update_B): ONE step up to and including the update of
// the merged tensor -- the behind environment is extended and B_new lands in the debug block, but no
// SVD runs and cores, bonds and l_pos stay as they are.  Bdirect_dev: merged tensor to use instead of
// the product of the two cores (relative layout), or nullptr.
static int sweep_anyd(tnml_ctx *c, const SweepCall &sc);
static int standalone_anyd(tnml_ctx *c, NarrowParams &n);

static int norm_envs_for_label_site(tnml_ctx *c);

// ---------------------------------------------------------------------------------------------
// The per-step planner at D = 2 (every sweep step the persistent launch does not take).  The loop of sweep_impl plans the geometry
// and the update record of a step and hands them to ONE of four launch paths:
//   plan_pipe_step -> launch_pipe_step_fused    the single-launch in-LDS step on one stream
//                  -> launch_pipe_step_split    the same step on two streams (communicator), both with launch_pipe_prologue
//   step_classic_lds                            wide -> [reduce] -> [all-reduce] -> narrow, in LDS
//   step_big                                    the chain through HBM and its pipeline (plan_next_z, launch_next_z)
// Every path counts its own launches where it makes them.  The order of the runtime calls inside a path is part of its behaviour
// (san/hip_stub.cpp writes it as a trace that is compared across changes of this file).
// ---------------------------------------------------------------------------------------------
// merge / L2 slices ride in the batch-side launch: an in-LDS step of a full sweep on the product of the two cores
static bool slices_ride(const SweepCall &sc, int npath) { return npath == 0 && sc.mode == 0 && !sc.Bdirect_dev; }

struct PipePlan {
  WidePipeParams wp, wpro;     // batch side of the step; the prologue that forms Z of this step where none is waiting
  bool need_prologue;
};

// Pipelined step: ONE launch (update + SVD of step k next to the batch-side work of step k+1).  Pure decision -- 1: the step is
// pipelined and pp is filled, 0: it takes the classic sequence, < 0: an internal check failed; nothing is launched, no state changes.
// (the first step of a segment takes the classic sequence: its behind environment is extended again from the stack forward
//  built, its f is forward's; the pipelined step resumes with the second step, from its own prologue)
static int plan_pipe_step(const tnml_ctx *c, const SweepCall &sc, const StepGeom &q, int step, int npath, PipePlan &pp) {
  const int N = c->N, L = c->L, k = q.k;
  if (!c->pipe.enabled || !slices_ride(sc, npath) || (sc.seg_start && step == 0)) return 0;
  if (prep_slice_lds_bytes(q.h, q.g, q.s, L) > kLdsMax) return 0;      // the slice workgroups of the launch must fit too
  WidePipeParams &wp = pp.wp, &wpro = pp.wpro;
  fill_wide_pipe(c, wp, sc, k);
  wp.do_ext = k >= 1; wp.do_f = 1; wp.wait_flag = 1;
  wp.do_z = (k + 1 <= N - 2);
  if (wp.do_z && !wide_pipe_fits(c, wp)) wp.do_z = 0;            // the next step will start from its own prologue
  pipe_try_one_level(wp);
  if (wp.do_z && c->pipe.tiles > wp.tiles_per_wg && q.nn >= 32) {
    // the SVD of this step is long (short side >= 32): a batch-side workgroup accumulates several sample tiles in
    // registers before it writes its partial pre-gradient -- proportionally fewer partial tensors to write and re-read
    // (gsz / one_level stay as pipe_try_one_level left them: not set_pipe_tiles)
    wp.tiles_per_wg = c->pipe.tiles;
    wp.nwide = (wp.ntiles + wp.tiles_per_wg - 1) / wp.tiles_per_wg;
    wp.ngroups = (wp.nwide + kPipeGroupMax - 1) / kPipeGroupMax;
  }
  if (!wide_pipe_fits(c, wp)) return 0;
  pp.need_prologue = !c->pipe.Z.matches(sc, k);
  if (pp.need_prologue) {
    fill_wide_pipe(c, wpro, sc, k - 1);
    wpro.do_ext = 0; wpro.wait_flag = 0; wpro.do_z = 1;
    wpro.do_f = (k >= 1 && c->Bnew_valid && !c->f_current) ? 1 : 0;
    if (wpro.do_f && (c->prev_h != wpro.hj || c->prev_g != wpro.gj))
      return fail(TNML_ERR_STATE, "internal: previous-step dims (%d,%d) do not match (%d,%d)", c->prev_h, c->prev_g, wpro.hj, wpro.gj);
    if (!wide_pipe_fits(c, wpro)) return 0;
  }
  return 1;
}

// Z of this step where no launch left it: the batch-side workgroups alone, on the stream the batch side of the step runs on
static int launch_pipe_prologue(tnml_ctx *c, WidePipeParams &wpro, bool split) {
  NarrowParams none{};
  wpro.wg0 = 0;
  if (split) { int rc = split_wait_update(c); if (rc) return rc; }
  prof_begin(c);
  launch_step_pipe(none, wpro, wide_pipe_lds_bytes(wpro), split ? c->stream2 : c->stream);
  prof_end(c, 1);
  c->sweep_launches++; c->step_launches++;
  if (split) { int rc = split_exchange(c, wpro.zsize); if (rc) return rc; }
  else if (c->comm) NCCL_TRY(ncclAllReduce(c->zred, c->zred, wpro.zsize + kMetricSlots, ncclFloat, ncclSum, c->comm, c->stream));
  if (wpro.do_f) c->f_current = true;
  return TNML_OK;
}

// What a pipelined launch adds to the update record and its batch side: the hand-off between the two and where the workgroups start.
// merged tensor / L2 term of this step: from the slice workgroups this launch carries (a slice of more than 8 rows is
// cut into two row parts: twice the workgroups, half the dependent tiles in each).  (Measured, round 2: preparing them
// at the end of the PREVIOUS launch inside workgroup 0 cost it 23 k cycles and saved 16 k of waiting -- removed.)
static void fill_pipe_update(tnml_ctx *c, NarrowParams &n, WidePipeParams &wp, const StepGeom &q) {
  const int D = c->D, L = c->L;
  n.fused = 1; n.nred = 0; n.sync = c->sync; n.red_out = nullptr;
  n.prep_ready = 0;
  n.wait_count = kD * kD * (q.h > 8 ? 2 : 1);
  n.pipe = 1; n.z_first = (q.k == 0); n.z_rows = wp.hprev * D;
  n.zsize = (q.k == 0 ? 1 : n.z_rows) * D * D * q.g * L;
  n.zred = c->zred; n.red = c->zred; n.zcore = wp.ext_core;
  n.flag = c->pipe.cnt + 17; n.token = ++c->pipe.token;
  wp.token = n.token;
  wp.wg0 = 1 + n.wait_count;
}
// LDS of the update side of a pipelined launch: the update workgroup and its slice helpers
static size_t pipe_update_lds(const tnml_ctx *c, const StepGeom &q) {
  return std::max(narrow_lds_bytes(q.h, q.g, q.s, c->L, q.m), prep_slice_lds_bytes(q.h, q.g, q.s, c->L));
}

static int launch_pipe_step_fused(tnml_ctx *c, const SweepCall &sc, const StepGeom &q, NarrowParams &n, PipePlan &pp) {
  WidePipeParams &wp = pp.wp;
  { int rc = split_join(c); if (rc) return rc; }
  if (pp.need_prologue) { int rc = launch_pipe_prologue(c, pp.wpro, false); if (rc) return rc; }
  fill_pipe_update(c, n, wp, q);
  const size_t lds = std::max(pipe_update_lds(c, q), wide_pipe_lds_bytes(wp));
  if (lds > kLdsMax) return fail(TNML_ERR_ARG, "internal: pipelined step needs %zu bytes of LDS", lds);
  prof_begin(c);
  launch_step_pipe(n, wp, lds, c->stream);
  prof_end(c, 3);
  c->sweep_launches++; c->step_launches++;
  if (c->comm && wp.do_z) NCCL_TRY(ncclAllReduce(c->zred, c->zred, wp.zsize + kMetricSlots, ncclFloat, ncclSum, c->comm, c->stream));
  c->bigpipe.Z.valid = false;
  c->pipe.Z.leave(sc, q.k + 1, wp.do_z != 0);
  return TNML_OK;
}

// Communicator path (batch shards over the ranks): the pre-gradient Z_{k+1} is final ~25 us into a ~57 us step, but behind
// a fused launch its all-reduce could only start when the SVD of step k has ended -- on the critical path of every step.
// So the step is launched in two parts: the update side (workgroup 0 + slice helpers) on the context's stream, the
// batch side on stream2 followed by the all-reduce, which then travels beside the SVD; the next update launch waits
// for its event.  Same kernels, same arithmetic as the fused launch (the B_new hand-off is a flag in memory either way).
static int launch_pipe_step_split(tnml_ctx *c, const SweepCall &sc, const StepGeom &q, NarrowParams &n, PipePlan &pp) {
  WidePipeParams &wp = pp.wp;
  if (c->split.flags_enabled && !c->split.flags) {
    { int rc = make_group(c, "the hand-off words of the two-stream step", {own_dev(c->split.flags, 4)}); if (rc) return rc; }
    HIP_TRY(hipMemsetAsync(c->split.flags, 0, 4 * sizeof(unsigned), c->stream));
  }
  if (!c->split.pending) {                 // first split step after anything else: stream2 starts behind the context's stream
    c->split.upd ^= 1;
    HIP_TRY(hipEventRecord(c->split.ev_upd[c->split.upd], c->stream));
    c->split.done_valid = false; c->split.zsig_valid = false;
  }
  if (pp.need_prologue) { int rc = launch_pipe_prologue(c, pp.wpro, true); if (rc) return rc; }
  fill_pipe_update(c, n, wp, q);
  const size_t lds_u = pipe_update_lds(c, q), lds_b = wide_pipe_lds_bytes(wp);
  if (lds_u > kLdsMax || lds_b > kLdsMax) return fail(TNML_ERR_ARG, "internal: pipelined step needs %zu / %zu bytes of LDS", lds_u, lds_b);
  const bool sflags = c->split.flags_enabled;
  // batch side of step k: needs the behind core the update launch of step k-1 left, then B_new(k) (flag in memory)
  { int rc = split_wait_update(c); if (rc) return rc; }
  {
    NarrowParams none{};
    WidePipeParams wb = wp;
    wb.wg0 = 0;
    launch_step_pipe(none, wb, lds_b, c->stream2);
  }
  // update side of step k: needs Z_k summed over the ranks (the exchange enqueued behind the previous batch-side launch)
  if (c->split.pending) {
    if (sflags && c->split.zsig_valid) { n.zpoll_flag = c->split.flags; n.zpoll_want = c->split.zseq; }
    else HIP_TRY(hipStreamWaitEvent(c->stream, c->split.ev_bat[c->split.bat], 0));
  }
  if (sflags) { n.done_flag = c->split.flags + 1; n.done_val = ++c->split.dseq; }
  launch_step_pipe_update(n, wp, lds_u, c->stream);
  if (sflags) c->split.done_valid = true;
  else {
    c->split.upd ^= 1;
    HIP_TRY(hipEventRecord(c->split.ev_upd[c->split.upd], c->stream));
  }
  { int rc = split_exchange(c, wp.do_z ? wp.zsize : -1); if (rc) return rc; }
  c->sweep_launches += 2; c->step_launches++;
  c->bigpipe.Z.valid = false;
  c->pipe.Z.leave(sc, q.k + 1, wp.do_z != 0);
  return TNML_OK;
}

// Classic in-LDS sequence: wide kernel (gradient slabs, with the merge / L2 slice workgroups where they ride) -> [slab reduction]
// -> [all-reduce over the batch shards] -> narrow kernel.
// single GPU: the slab reduction rides in the narrow launch as helper workgroups (no separate reduce kernel, no boundary) and the
// merge / L2 products ride in the wide launch (or, with the plain-FMA wide kernel, in the narrow launch as well)
static int step_classic_lds(tnml_ctx *c, const SweepCall &sc, const StepGeom &q, NarrowParams &n) {
  const int L = c->L;
  { int rc = split_join(c); if (rc) return rc; }
  drop_pregradients(c);
  WideParams w{};
  { int rc = fill_wide(c, w, q, sc); if (rc) return rc; }
  w.stamps = c->stamps ? c->dbg + 4 * c->bmax + kDbgSigma + 5 + 17 : nullptr;
  PrepParams prep{};
  prep.lab = n.lab; prep.pl = n.pl; prep.Nh = n.Nh; prep.Ng = n.Ng; prep.h = q.h; prep.g = q.g; prep.s = q.s; prep.L = L;
  prep.l2_flag = n.l2_flag; prep.prepB = c->prepB; prep.prepG = c->prepG;
  prof_begin(c);
  bool prep_done = false;
  if (!launch_wide(w, sc.nblk, slices_ride(sc, 0) ? &prep : nullptr, c->stream, &prep_done))
    return fail(TNML_ERR_ARG, "step at sites (%d,%d): a 32-sample tile of this bond dimension does not fit the batch kernels' LDS", q.p, q.p + 1);
  c->sweep_launches++;
  n.prep_ready = prep_done ? 1 : 0;
  // slices the batch launch could not host would ride in the update launch -- unless they do not fit a workgroup's LDS
  // either (bond 64 next to a chain end at three labels): then the update workgroup forms B and Ln.B.Rn itself, which
  // the launch does only un-fused (separate reduction)
  if (n.fused && !prep_done && prep_slice_lds_bytes(q.h, q.g, q.s, L) > kLdsMax) { n.fused = 0; n.nred = 0; }
  if (n.fused) n.wait_count = n.nred + (n.prep_ready ? 0 : kD * kD);
  prof_end(c, 1);
  // ---- reduce (+ all-reduce over the batch shards)
  if (!n.fused) {
    prof_begin(c);
    launch_reduce(c->slabs, sc.nblk, c->slab_stride, (int)q.bsize + kMetricSlots, c->red, c->stream);
    prof_end(c, 2);
    c->sweep_launches++;
  }
  if (c->comm) NCCL_TRY(ncclAllReduce(c->red, c->red, q.bsize + kMetricSlots, ncclFloat, ncclSum, c->comm, c->stream));
  prof_begin(c);
  { int rc = run_narrow(c, n, 0); if (rc) return rc; }
  prof_end(c, 3);
  c->sweep_launches++;
  return TNML_OK;
}

// Pipelined large-tensor step: may the batch kernel of step k+1 run beside the SVD of this one?  Pure decision.
// Needs: the next step is a large-tensor step too, both environments exist as arrays (k >= 2, an ahead environment two sites
// on), the tiled batch kernel takes the doubled row operand (h -> D h), the slabs of Z fit the pre-gradient scratch.
struct NextZ {
  bool on;
  int gnext;         // ahead bond of step k+1
  size_t lds_z;      // LDS of its batch kernel
};
static NextZ plan_next_z(const tnml_ctx *c, const SweepCall &sc, const StepGeom &q) {
  const int N = c->N, D = c->D, L = c->L, left_dir = sc.left_dir, h = q.h, g = q.g, m = q.m;
  NextZ z{false, 0, 0};
  if (!(c->bigpipe.enabled && c->pipe.enabled && sc.mode == 0 && !sc.Bdirect_dev && !c->debug && !c->profile && sc.trunc_policy != TNML_TRUNC_ADAPTIVE &&
        q.k >= 2 && q.k + 1 <= N - 2 && sc.nblk <= c->pipe.nwide))
    return z;
  const int pn = std::min(q.sa, rel_site(c, left_dir, 2));   // sites (pn, pn + 1) of step k+1; g is the bond the two steps share
  z.gnext = rel_bond(c, left_dir, 2);
  const int mnext = tnml_trunc_rank(sc.trunc_policy, left_dir, pn, N, left_dir ? z.gnext : m, D, left_dir ? m : z.gnext, L, c->Mpol);
  const size_t zs = (size_t)D * h * D * D * z.gnext * L;
  z.lds_z = wide_tiled_lds_bytes(L, D * h, h, g, z.gnext, false);      // (its launch extends no environment and hands Hcur in)
  z.on = mnext > 0 && narrow_path(c, m, z.gnext, g, L, mnext) == 1 && zs + kMetricSlots <= (size_t)c->zstride &&
         z.lds_z > 0 && z.lds_z <= kLdsMax && D * h <= 2 * c->Mmax && (size_t)D * h * c->b_pad <= (size_t)2 * c->Mmax * c->b_pad;
  return z;
}

// The side-stream chain of the large-tensor pipeline, behind B_new(k): E_k and P'_k = E_k (x) x_k (unless the step's first launch
// formed them: ext_in_front); then the tiled batch kernel "of step k+1" with P'_k in the place of its behind environment (D h
// rows): f of step k from B_new(k) and the slabs of Z_{k+1}; their sum; the exchange.  w: the batch side of step k (fill_wide).
static int launch_next_z(tnml_ctx *c, const SweepCall &sc, const StepGeom &q, const WideParams &w, const NextZ &nz, bool ext_in_front, bool bsig) {
  const int D = c->D, L = c->L, h = q.h, g = q.g;
  if (bsig) { if (!launch_big_gate(c->bigpipe.flags + 1, c->bigpipe.bsig_seq, c->status, c->stream2)) return fail(TNML_ERR_HIP, "%s", big_launch_error()); }
  else HIP_TRY(hipStreamWaitEvent(c->stream2, c->bigpipe.ev_upd, 0));
  c->bigpipe.ext_on_side = !ext_in_front;
  if (!ext_in_front && !launch_big_ext(w.Hprev, w.x_km1, w.x_k, w.ext_core, c->b_pad, w.Hcur, c->bigpipe.Pk, c->stream2)) return fail(TNML_ERR_HIP, "%s", big_launch_error());
  WideParams z{};
  z.b = c->b; z.b_pad = c->b_pad; z.L = L;
  z.h = D * h; z.g = nz.gnext; z.hp = h; z.gp = g;
  z.do_f = 1; z.do_ext = 0; z.first_ext = 0;
  z.act_fn = sc.act_fn; z.loss_fn = sc.loss_fn; z.T = sc.T;
  z.x_km1 = w.x_k; z.x_k = w.x_kp1;
  z.x_kp1 = x_rel(c, sc.left_dir, 2);
  z.Hprev = w.Hcur; z.Hcur = c->bigpipe.Pk;
  z.Gprev = w.Gcur;
  z.Gcur = env_rel(c, sc.left_dir, 3);
  z.Bprev = c->Bnew;
  z.y = c->y; z.f = c->f;
  z.slabs = c->zslabs; z.slab_stride = c->zstride; z.bsize = (int)((size_t)D * h * D * D * nz.gnext * L);
  launch_wide_tiled(z, sc.nblk, nz.lds_z, c->stream2);
  launch_reduce(c->zslabs, sc.nblk, c->zstride, z.bsize + kMetricSlots, c->zred, c->stream2);
  if (c->comm) NCCL_TRY(ncclAllReduce(c->zred, c->zred, z.bsize + kMetricSlots, ncclFloat, ncclSum, c->comm, c->stream2));
  if (c->bigpipe.flags_enabled) { ++c->bigpipe.zsig_seq; if (!launch_big_signal(c->bigpipe.flags, c->bigpipe.zsig_seq, c->stream2)) return fail(TNML_ERR_HIP, "%s", big_launch_error()); }
  HIP_TRY(hipEventRecord(c->bigpipe.ev_z, c->stream2));
  c->bigpipe.pending = true;
  c->bigpipe.Z.leave(sc, q.k + 1, true, D * h, D * D * nz.gnext * L);
  c->sweep_launches += ext_in_front ? 2 : 3;
  return TNML_OK;
}

// Large-tensor step, the chain through HBM: batch kernel + reduction (a step fed by Z has neither: its contraction rides in the
// chain's first launch), then the update: seven launches in the factored form (front products [+ contraction, + next environment],
// merged tensor + weight decay, update, Gram, Jacobi + replay + order, cores + T2, norm environment), eight with T = Nh^T . B.
// f_stored: f of this step is stored by the batch kernel of the next one (launch_next_z).
// (Kept apart from step_classic_lds: the two share fill_wide and the reduce / all-reduce lines only, and every line of the pipeline
//  here would be a condition there.)
static int step_big(tnml_ctx *c, const SweepCall &sc, const StepGeom &q, NarrowParams &n, bool &f_stored) {
  const int D = c->D, L = c->L, k = q.k, g = q.g;
  const bool whole = sc.mode == 0 && !sc.Bdirect_dev;         // a full sweep step on the product of the two cores
  // is the reduced pre-gradient of THIS step waiting in zred (left there by the batch kernel that ran on stream2 beside the
  // previous step's SVD)?
  const bool zbig = whole && k >= 3 && c->bigpipe.Z.matches(sc, k) &&
                    c->bigpipe.Z.cols == D * D * g * L && c->bigpipe.Z.rows == D * rel_bond(c, sc.left_dir, -2);
  // (a step fed by Z does not wait for the side stream with an event: the workgroups of its first launch that need Z poll the
  //  sequence number the side stream leaves behind its chain -- see big_signal_kernel; everything else of that launch starts at once)
  const bool zpoll = zbig && c->bigpipe.flags_enabled && c->bigpipe.pending;
  { int rc = split_join(c, zpoll); if (rc) return rc; }
  drop_pregradients(c);
  WideParams w{};
  { int rc = fill_wide(c, w, q, sc); if (rc) return rc; }
  w.stamps = c->stamps ? c->dbg + 4 * c->bmax + kDbgSigma + 5 + 17 : nullptr;
  // The merged tensor and T = Nh^T . B need nothing this step's batch kernel produces -- they run on a second stream beside it
  // (two of the chain's fourteen launches, 30 us of a 380 us C5 step), joined by an event before the weight-decay kernel reads them.
  // (a step that takes its gradient from Z has no batch kernel to hide them behind: they stay on the context's stream, in front of
  // the chain, and the two cross-queue hops -- 10 us each -- are saved)
  const bool prep_ahead = whole && !zbig;
  if (prep_ahead) {
    { int rc = ensure_big(c); if (rc) return rc; }
    HIP_TRY(hipEventRecord(c->ev_main, c->stream));                  // everything the previous step wrote
    HIP_TRY(hipStreamWaitEvent(c->stream2, c->ev_main, 0));
    if (!launch_narrow_big(n, c->big, c->stream2, c->check_launches, true, false)) return fail(TNML_ERR_HIP, "%s", big_launch_error());
    HIP_TRY(hipEventRecord(c->ev_prep, c->stream2));
  }
  prof_begin(c);
  BigFront front{};
  if (zbig) {
    // raw gradient = A_{k-1}^T . Z_k (+ the metric tail): no batch kernel, no slab reduction, no exchange on this stream; it rides
    // in the launch that forms the merged tensor (run_narrow below)
    front.Z = c->zred; front.A = w.ext_core; front.ncols = D * D * g * L; front.red = c->red;
    if (zpoll) { front.poll_flag = c->bigpipe.flags; front.poll_want = c->bigpipe.zsig_seq; front.wait_ev = c->bigpipe.ev_z; }
    prof_end(c, 1);
    c->step_launches++;           // (counted with the single-launch steps: a step that took its gradient from Z)
  } else {
    bool prep_done = false;
    if (!launch_wide(w, sc.nblk, nullptr, c->stream, &prep_done))
      return fail(TNML_ERR_ARG, "step at sites (%d,%d): a 32-sample tile of this bond dimension does not fit the batch kernels' LDS", q.p, q.p + 1);
    prof_end(c, 1);
    prof_begin(c);
    launch_reduce(c->slabs, sc.nblk, c->slab_stride, (int)q.bsize + kMetricSlots, c->red, c->stream);
    prof_end(c, 2);
    if (c->comm) NCCL_TRY(ncclAllReduce(c->red, c->red, q.bsize + kMetricSlots, ncclFloat, ncclSum, c->comm, c->stream));
    c->sweep_launches += 2;
  }
  prof_begin(c);
  if (prep_ahead) HIP_TRY(hipStreamWaitEvent(c->stream, c->ev_prep, 0));
  const NextZ nz = plan_next_z(c, sc, q);
  if (nz.on) { int rc = ensure_big(c); if (rc) return rc; }          // (the flag words of the hand-offs live with its scratch)
  if (nz.on) { int rc = batch_Pk(c); if (rc) return rc; }
  // (a step fed by Z launches no batch kernel of its own: the environment work for the NEXT step's batch kernel rides in this
  //  step's first launch on this stream, and the side stream's chain starts with the batch kernel itself)
  const bool ext_in_front = nz.on && zbig;
  if (ext_in_front) {
    front.ext_Eprev = w.Hprev; front.ext_x_km1 = w.x_km1; front.ext_x_k = w.x_k; front.ext_A = w.ext_core; front.b_pad = c->b_pad;
    front.ext_Ecur = w.Hcur; front.ext_Pk = c->bigpipe.Pk;
    front.ext_acquire = c->bigpipe.ext_on_side;
  }
  const bool bsig = nz.on && c->bigpipe.flags_enabled;
  if (bsig) ++c->bigpipe.bsig_seq;
  { int rc = run_narrow(c, n, 1, prep_ahead, nz.on ? c->bigpipe.ev_upd : nullptr, zbig ? &front : nullptr, bsig ? c->bigpipe.flags + 1 : nullptr, c->bigpipe.bsig_seq);
    if (rc) return rc; }
  prof_end(c, 3);
  c->sweep_launches += (sc.Bdirect_dev || prep_ahead) ? 8 : 7;
  if (zbig && !nz.on) {
    // a step that took its gradient from Z launched no batch kernel, and none for the next step either: the behind environment
    // E_k the next (classic) step extends has to be formed here
    if (!launch_big_ext(w.Hprev, w.x_km1, w.x_k, w.ext_core, c->b_pad, w.Hcur, c->bigpipe.Pk, c->stream)) return fail(TNML_ERR_HIP, "%s", big_launch_error());
    c->sweep_launches += 1;
  }
  if (nz.on) { int rc = launch_next_z(c, sc, q, w, nz, ext_in_front, bsig); if (rc) return rc; }
  f_stored = nz.on;
  return TNML_OK;
}

static int sweep_impl(tnml_ctx *c, int left_dir, int n_steps, int first_of_sweep, float lr, float weight_dec,
                      int l2_flag, int act_fn, int loss_fn, float T, int trunc_policy, float *metrics_out,
                      float *f_out, int mode, const float *Bdirect_dev) {
  if (!c) return fail(TNML_ERR_ARG, "ctx is NULL");
  if (!c->cores_set) return fail(TNML_ERR_STATE, "cores were never set");
  if (!c->have_input || !c->have_labels) return fail(TNML_ERR_STATE, "a sweep needs inputs and labels (tnml_set_input)");
  if (n_steps < 1) return fail(TNML_ERR_ARG, "n_steps < 1");
  if (act_fn < 0 || act_fn > 2 || loss_fn < 0 || loss_fn > 2) return fail(TNML_ERR_ARG, "unknown activation / loss");
  if (trunc_policy != TNML_TRUNC_REFERENCE && trunc_policy != TNML_TRUNC_FIXED && trunc_policy != TNML_TRUNC_ADAPTIVE)
    return fail(TNML_ERR_ARG, "unknown truncation policy");
  left_dir = left_dir ? 1 : 0;
  const int N = c->N, D = c->D, L = c->L;
  HIP_TRY(hipSetDevice(c->device));
  if (left_dir ? !(c->l_pos >= 1 && c->l_pos - n_steps >= 0) : !(c->l_pos + n_steps <= N - 1))
    return fail(TNML_ERR_STATE, "position not allowed for %s sweep step (l_pos = %d, n_steps = %d)",
                left_dir ? "left" : "right", c->l_pos, n_steps);
  if (!(left_dir ? c->envs_valid_L : c->envs_valid_R))
    return fail(TNML_ERR_STATE, "the %s environments are not built for this batch: call tnml_forward at l_pos = %d first",
                left_dir ? "left" : "right", left_dir ? N - 1 : 0);
  // segment start (tnml_set_any_position): a forward with the label inside the chain built BOTH stacks and left f; nothing of a
  // previous step (B_new, a pre-gradient) is valid, and either direction may follow
  const bool seg_start = !first_of_sweep && c->any_pos && label_inside(c) && c->envs_valid_L && c->envs_valid_R && !c->Bnew_valid;
  if (first_of_sweep) {
    if ((left_dir && c->l_pos != N - 1) || (!left_dir && c->l_pos != 0))
      return fail(TNML_ERR_STATE, "first_of_sweep set but l_pos = %d", c->l_pos);
    c->Bnew_valid = false;
  } else if (!seg_start && (!c->Bnew_valid || c->prev_left_dir != left_dir)) {
    return fail(TNML_ERR_STATE, "mid-sweep continuation without a preceding step in the same direction");
  }
  if (!c->f_current && !c->Bnew_valid) return fail(TNML_ERR_STATE, "no f to start from: call tnml_forward or tnml_set_f");
  if (n_steps > c->metrics_cap) return fail(TNML_ERR_ARG, "n_steps > N");
  // norm environments towards which the sweep runs (a segment start has no previous step that left the one behind it either: both
  // stacks are built up to the label site, and finish_sweep marks the one behind invalid again when the segment stops mid-chain)
  if (l2_flag) {
    if (seg_start) { int rc = norm_envs_for_label_site(c); if (rc) return rc; }
    if (!left_dir && !c->Rn_valid) { int rc = build_norm_chain(c, true); if (rc) return rc; c->Rn_valid = true; }
    if (left_dir && !c->Ln_valid) { int rc = build_norm_chain(c, false); if (rc) return rc; c->Ln_valid = true; }
  }
  // the stack behind a segment is rewritten from its first step on: finish_step marks it invalid once that step is planned (the
  // opposite direction then needs a forward again); a call that fails before it leaves both stacks as forward built them
  c->seg_starting = seg_start && mode == 0;
  hipEvent_t sw_ev1 = nullptr;
  if (c->sweep_timing && mode == 0) {
    if (c->sweep_ev_used + 2 > c->sweep_ev.size()) {
      hipEvent_t a = nullptr, b2 = nullptr;
      { int rc = make_group(c, "a pair of timing events", {own_event(a, hipEventDefault), own_event(b2, hipEventDefault)}); if (rc) return rc; }
      c->sweep_ev.push_back(a); c->sweep_ev.push_back(b2);
    }
    HIP_TRY(hipEventRecord(c->sweep_ev[c->sweep_ev_used], c->stream));
    sw_ev1 = c->sweep_ev[c->sweep_ev_used + 1];
    c->sweep_ev_used += 2;
  }
  // (the generic-D batch kernel takes 64 samples per workgroup)
  const SweepCall sc{left_dir, n_steps, lr, weight_dec, l2_flag, act_fn, loss_fn, T, trunc_policy, metrics_out, f_out, mode, Bdirect_dev,
                     sw_ev1, seg_start, D != kD ? c->b_pad / kTS / 2 : c->b_pad / kTS};
  if (D != kD) return sweep_anyd(c, sc);

  int done_persist = 0;
  if (mode == 0 && !Bdirect_dev && first_of_sweep) {
    done_persist = sweep_persist(c, sc);
    if (done_persist < 0) return done_persist;
  }
  const bool split = c->comm && c->split.enabled && !c->profile;      // a pipelined step goes out in two parts (launch_pipe_step_split)
  for (int step = 0; step < (done_persist ? 0 : n_steps); ++step) {
    const StepGeom q = step_geom(c, left_dir, trunc_policy);
    if (q.fail) return step_geom_error(c, q);
    const int npath = narrow_path(c, q.h, q.g, q.s, L, q.m);
    if (npath < 0) return npath;
    // ---- the update record (built first: the wide launch carries its slice workgroups)
    NarrowParams n{};
    fill_step_update(c, n, q, sc, step, (c->debug || mode == 1) ? c->dbg : nullptr);
    n.chol_thr = c->chol_thr;
    n.prepB = c->prepB; n.prepG = c->prepG;
    if (slices_ride(sc, npath) && !c->comm) {        // + slab reduction in the narrow launch (a pipelined launch keeps the slab fields as they are)
      n.fused = 1; n.slabs = c->slabs; n.nslabs = sc.nblk; n.slab_stride = c->slab_stride;
      n.nred = ((int)q.bsize + kMetricSlots + 63) / 64; n.red_out = c->red; n.sync = c->sync;
    }
    // ---- one of the four paths
    PipePlan pp{};
    const int piped = plan_pipe_step(c, sc, q, step, npath, pp);
    if (piped < 0) return piped;
    bool f_stored = piped != 0;      // (the batch-side work of a pipelined step stored f of this step already)
    int rc;
    if (piped) rc = split ? launch_pipe_step_split(c, sc, q, n, pp) : launch_pipe_step_fused(c, sc, q, n, pp);
    else if (npath == 0) rc = step_classic_lds(c, sc, q, n);
    else rc = step_big(c, sc, q, n, f_stored);
    if (rc) return rc;
    if (mode == 1) return finish_update_only(c, q, metrics_out);
    if ((rc = finish_step(c, q, sc, step, f_stored))) return rc;
  }
  HIP_TRY(hipGetLastError());
  { int rc = split_join(c); if (rc) return rc; }
  return finish_sweep(c, sc);
}

extern "C" int tnml_sweep(tnml_ctx *c, int left_dir, int n_steps, int first_of_sweep, float lr, float weight_dec,
                          int l2_flag, int act_fn, int loss_fn, float T, int trunc_policy, float *metrics_out,
                          float *f_out) {
  return sweep_impl(c, left_dir, n_steps, first_of_sweep, lr, weight_dec, l2_flag, act_fn, loss_fn, T, trunc_policy,
                    metrics_out, f_out, 0, nullptr);
}

static int norm_envs_for_label_site(tnml_ctx *c) {
  if (!c->Ln_valid) { int rc = build_norm_chain(c, false); if (rc) return rc; c->Ln_valid = true; }
  if (!c->Rn_valid) { int rc = build_norm_chain(c, true); if (rc) return rc; c->Rn_valid = true; }
  return TNML_OK;
}

extern "C" int tnml_update_B(tnml_ctx *c, const float *B_canon, int left_dir, float lr, float weight_dec, int l2_flag,
                             int act_fn, int loss_fn, float T, double *Bnew_canon, size_t capacity, float *metrics2) {
  if (!c || !Bnew_canon) return fail(TNML_ERR_ARG, "NULL argument");
  left_dir = left_dir ? 1 : 0;
  const int l = c->l_pos, p = left_dir ? l - 1 : l;
  if (p < 0 || p > c->N - 2) return fail(TNML_ERR_STATE, "position not allowed for %s sweep step (l_pos = %d)", left_dir ? "left" : "right", l);
  HIP_TRY(hipSetDevice(c->device));
  const int ml = c->ml(p), mr = c->mr(p + 1);
  const size_t bsize = (size_t)ml * c->D * c->D * mr * c->L;
  if (capacity < bsize) return fail(TNML_ERR_ARG, "capacity too small");
  const float *Bd = nullptr;
  if (B_canon) {
    std::vector<float> rel(bsize);
    canon_to_rel(B_canon, rel.data(), left_dir, ml, mr, c->D, c->L);
    HIP_TRY(hipMemcpyAsync(c->Bscr, rel.data(), bsize * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    Bd = c->Bscr;
  }
  if (l2_flag) { int rc = norm_envs_for_label_site(c); if (rc) return rc; }
  const bool first = c->l_pos == (left_dir ? c->N - 1 : 0);
  int rc = sweep_impl(c, left_dir, 1, first, lr, weight_dec, l2_flag, act_fn, loss_fn, T, TNML_TRUNC_FIXED, metrics2, nullptr,
                      1, Bd);
  if (rc) return rc;
  size_t n = 0;
  const bool dbg_was = c->debug;
  c->debug = true;
  rc = tnml_get_step_debug(c, TNML_DBG_B_NEW, Bnew_canon, capacity, &n);
  c->debug = dbg_was;
  return rc;
}

extern "C" int tnml_l2_term(tnml_ctx *c, const float *B_canon, int left_dir, float weight_dec, double *loss,
                            double *grad_canon, size_t capacity) {
  if (!c || !B_canon || !loss || !grad_canon) return fail(TNML_ERR_ARG, "NULL argument");
  left_dir = left_dir ? 1 : 0;
  const int l = c->l_pos, p = left_dir ? l - 1 : l;
  if (p < 0 || p > c->N - 2) return fail(TNML_ERR_STATE, "no merged tensor at l_pos = %d for a %s step", l, left_dir ? "left" : "right");
  if (!c->cores_set) return fail(TNML_ERR_STATE, "cores were never set");
  HIP_TRY(hipSetDevice(c->device));
  const int D = c->D, L = c->L;
  const int ml = c->ml(p), mr = c->mr(p + 1);
  const int h = left_dir ? mr : ml, g = left_dir ? ml : mr;
  const size_t bsize = (size_t)ml * D * D * mr * L;
  if (capacity < bsize) return fail(TNML_ERR_ARG, "capacity too small");
  if (bsize > c->bmax) return fail(TNML_ERR_ARG, "merged tensor exceeds the buffers sized for M = %d", c->Mmax);
  const int npath = D != kD ? 0 : narrow_path(c, h, g, 1, L, 1);
  if (npath < 0) return npath;
  int rc = norm_envs_for_label_site(c);
  if (rc) return rc;
  std::vector<float> rel(bsize);
  canon_to_rel(B_canon, rel.data(), left_dir, ml, mr, D, L);
  HIP_TRY(hipMemcpyAsync(c->Bscr, rel.data(), bsize * sizeof(float), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemsetAsync(c->red, 0, (size_t)c->slab_stride * sizeof(float), c->stream));
  NarrowParams n{};
  n.L = L; n.D = D; n.h = h; n.g = g; n.s = 1; n.m = 1; n.bsize = (int)bsize;
  n.l2_flag = 1; n.lr = 0.f; n.wd = weight_dec;
  n.red = c->red;
  n.Nh = norm_rel(c, left_dir, -1);
  n.Ng = norm_rel(c, left_dir, 2);
  n.Bnew = c->Bscr2;
  n.dbg = c->dbg; n.status = c->status; n.counters = nullptr;
  n.Bdirect = c->Bscr; n.stop_after_update = 1;
  n.svd_stop2 = c->svd_stop2;
  rc = D != kD ? standalone_anyd(c, n) : run_narrow(c, n, npath);
  if (rc) return rc;
  HIP_TRY(hipGetLastError());
  c->last_bsize = (int)bsize; c->last_n = 1; c->last_h = h; c->last_g = g; c->last_left_dir = left_dir;
  const bool dbg_was = c->debug;
  c->debug = true;
  size_t nn = 0;
  double sc[kDbgScalars];
  rc = tnml_get_step_debug(c, TNML_DBG_L2_GRAD, grad_canon, capacity, &nn);
  if (!rc) rc = tnml_get_step_debug(c, TNML_DBG_L2, sc, kDbgScalars, &nn);
  c->debug = dbg_was;
  if (rc) return rc;
  *loss = sc[0];
  return TNML_OK;
}

extern "C" int tnml_svd_split(tnml_ctx *c, const float *mat, int rows, int cols, int m, float *US, float *SVh, double *sigma) {
  // tensor_svd (Network_class.py:839-962) of an arbitrary rows x cols matrix: U sqrt(S) [rows][m], sqrt(S) Vh [m][cols]
  if (!c || !mat || !US || !SVh) return fail(TNML_ERR_ARG, "NULL argument");
  const int D = c->D;
  if (rows < D || cols < D || rows % D || cols % D) return fail(TNML_ERR_ARG, "rows and cols must be multiples of D = %d", D);
  const int h = rows / D, g = cols / D, nn = std::min(rows, cols);
  if (m < 1 || m > nn) return fail(TNML_ERR_ARG, "kept rank %d outside [1, %d]", m, nn);
  const size_t bsize = (size_t)rows * cols;
  if (bsize > c->bmax || (size_t)rows * m > c->bmax || (size_t)m * cols > c->bmax)
    return fail(TNML_ERR_ARG, "matrix exceeds the buffers sized for M = %d", c->Mmax);
  const int npath = D != kD ? 0 : narrow_path(c, h, g, 1, 1, m);
  if (npath < 0) return npath;
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipMemcpyAsync(c->Bscr, mat, bsize * sizeof(float), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemsetAsync(c->red, 0, (size_t)c->slab_stride * sizeof(float), c->stream));
  float *us_dev = c->slabs, *svh_dev = c->slabs + c->bmax;       // the slab area is idle outside a step
  if ((size_t)c->nblk_cap * c->slab_stride < 2 * c->bmax) return fail(TNML_ERR_ARG, "slab scratch too small");
  NarrowParams n{};
  n.L = 1; n.D = D; n.h = h; n.g = g; n.s = 1; n.m = m; n.bsize = (int)bsize;
  n.l2_flag = 0; n.lr = 0.f; n.wd = 0.f;
  n.red = c->red;
  n.Bnew = c->Bscr2;
  n.out_behind = us_dev; n.ob_s_h = D * m; n.ob_s_d = m; n.ob_s_m = 1;
  n.out_ahead = svh_dev; n.oa_s_m = cols; n.oa_s_d = g; n.oa_s_g = 1;
  n.dbg = c->dbg; n.status = c->status; n.counters = c->counters;
  n.stamps = (c->debug || c->stamps) ? c->dbg + 4 * c->bmax + kDbgSigma + 5 : nullptr;
  n.Bdirect = c->Bscr;
  n.svd_stop2 = c->svd_stop2;
  n.chol_thr = c->chol_thr;
  { int rc = D != kD ? standalone_anyd(c, n) : run_narrow(c, n, npath); if (rc) return rc; }
  HIP_TRY(hipGetLastError());
  c->last_bsize = (int)bsize; c->last_n = nn; c->last_h = h; c->last_g = g; c->last_left_dir = 0;
  HIP_TRY(hipMemcpyAsync(US, us_dev, (size_t)rows * m * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(SVh, svh_dev, (size_t)m * cols * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (sigma) {
    std::vector<double> sg(kBigMaxN);
    HIP_TRY(hipMemcpy(sg.data(), c->dbg + 4 * bsize, nn * sizeof(double), hipMemcpyDeviceToHost));
    for (int i = 0; i < nn; ++i) sigma[i] = sg[i];
  }
  return check_status(c);
}

// ---------------------------------------------------------------------------------------------
// Generic feature dimension (3 <= D <= 8, kernels_anyd.hip): the classic per-step sequence only -- batch kernel -> slab reduction
// -> update kernel -- with no persistent sweep, pipelined step, large-tensor pipeline or communicator.  Planning and bookkeeping
// go through the shared frame functions (step_geom, fill_wide, fill_update, finish_step, finish_sweep), the capture block is laid
// out as on the D == 2 path; the update kernel takes any short side up to kBigMaxN (odd sides padded to even inside it).
// ---------------------------------------------------------------------------------------------
static int anyd_scratch(tnml_ctx *c) {           // Generic-D group, on first use: both or none
  return c->anyd_W ? TNML_OK : make_group(c, "the scratch of the generic-D update", {
      own_dev(c->anyd_W, (size_t)kBigMaxN * kBigMaxN), own_dev(c->anyd_T2, 2 * (size_t)c->D * c->Mmax * c->Mmax)});
}

// update kernel in "stop after the update" / "given matrix" mode (tnml_l2_term, tnml_svd_split)
static int standalone_anyd(tnml_ctx *c, NarrowParams &n) {
  const int r = c->D * n.h, cc = c->D * n.g * n.L, nn = std::min(r, cc);
  if (nn > kBigMaxN) return fail(TNML_ERR_ARG, "min(rows, cols) = %d > %d: the Jacobi kernels handle n <= %d", nn, kBigMaxN, kBigMaxN);
  int rc = anyd_scratch(c);
  if (rc) return rc;
  n.D = c->D;
  if (!launch_update_anyd(n, c->anyd_W, nullptr, c->stream))
    return fail(TNML_ERR_ARG, "update kernel at D = %d refused a %d x %d matrix (kept rank %d)", c->D, r, cc, n.m);
  return TNML_OK;
}

static int sweep_anyd(tnml_ctx *c, const SweepCall &sc) {
  const int D = c->D, L = c->L, nblk = sc.nblk;              // (64 samples per batch-side workgroup)
  { int rc = anyd_scratch(c); if (rc) return rc; }
  for (int step = 0; step < sc.n_steps; ++step) {
    const StepGeom q = step_geom(c, sc.left_dir, sc.trunc_policy);
    if (q.fail) return step_geom_error(c, q);
    const int p = q.p, h = q.h, g = q.g;
    if (q.nn > kBigMaxN)
      return fail(TNML_ERR_ARG, "step at sites (%d,%d): min(rows, cols) = %d > %d: the Jacobi kernels handle n <= %d", p, p + 1, q.nn,
                  kBigMaxN, kBigMaxN);
    // ---- batch side: f of the previous step, activation / metrics, behind environment, gradient slabs ----
    WideParams w{};
    { int rc = fill_wide(c, w, q, sc); if (rc) return rc; }
    prof_begin(c);
    if (!launch_batch_anyd(w, D, nblk, true, c->stream))
      return fail(TNML_ERR_ARG, "step at sites (%d,%d): the batch kernel at D = %d needs %zu bytes of LDS", p, p + 1, D,
                  anyd_batch_lds_bytes(D, w.hp, w.gp, h, g, L));
    prof_end(c, 1);
    prof_begin(c);
    launch_reduce(c->slabs, nblk, c->slab_stride, (int)q.bsize + kMetricSlots, c->red, c->stream);
    prof_end(c, 2);
    // ---- update side (chol_thr stays 0: the generic-D update kernel has no Cholesky step; the capture block is its workspace) ----
    NarrowParams n{};
    fill_step_update(c, n, q, sc, step, c->dbg);
    prof_begin(c);
    if (!launch_update_anyd(n, c->anyd_W, c->anyd_T2, c->stream))
      return fail(TNML_ERR_ARG, "step at sites (%d,%d): update kernel at D = %d refused a %d x %d matrix", p, p + 1, D, D * h, D * g * L);
    prof_end(c, 3);
    c->sweep_launches += 3;
    if (sc.mode == 1) return finish_update_only(c, q, sc.metrics_out);
    { int rc = finish_step(c, q, sc, step, false); if (rc) return rc; }
    drop_pregradients(c);
  }
  HIP_TRY(hipGetLastError());
  return finish_sweep(c, sc);
}

// ---------------------------------------------------------------------------------------------
// inspection
// ---------------------------------------------------------------------------------------------
extern "C" int tnml_l_pos(tnml_ctx *c) { return c ? c->l_pos : TNML_ERR_ARG; }
extern "C" int tnml_batch(tnml_ctx *c) { return c ? c->b : TNML_ERR_ARG; }

extern "C" int tnml_get_env(tnml_ctx *c, int side, int site, float *out, size_t capacity, int *m_out) {
  if (!c || !out) return fail(TNML_ERR_ARG, "NULL argument");
  if (site < 0 || site >= c->N) return fail(TNML_ERR_ARG, "site out of range");
  if (int rc = batch_group_there(c)) return rc;
  HIP_TRY(hipSetDevice(c->device));
  const int m = side == TNML_SIDE_LEFT ? c->mr(site) : c->ml(site);
  if (capacity < (size_t)m * c->b) return fail(TNML_ERR_ARG, "capacity too small");
  std::vector<float> tmp((size_t)m * c->b_pad);
  const float *src = c->env_slot(side == TNML_SIDE_LEFT ? c->Lenv : c->Renv, site);
  HIP_TRY(hipMemcpyAsync(tmp.data(), src, tmp.size() * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  for (int s = 0; s < c->b; ++s)
    for (int a = 0; a < m; ++a) out[(size_t)s * m + a] = tmp[(size_t)a * c->b_pad + s];
  if (m_out) *m_out = m;
  return TNML_OK;
}

extern "C" int tnml_set_trunc_threshold(tnml_ctx *c, double threshold) {
  if (!c) return fail(TNML_ERR_ARG, "ctx is NULL");
  if (!(threshold > 0.0 && threshold < 1.0)) return fail(TNML_ERR_ARG, "threshold %g outside (0, 1)", threshold);
  c->trunc_thr = threshold;
  return TNML_OK;
}

extern "C" int tnml_set_narrow_path(tnml_ctx *c, int force_large) {
  if (!c) return fail(TNML_ERR_ARG, "ctx is NULL");
  c->force_big = force_large != 0;
  return TNML_OK;
}

// mean device time of one all-reduce of `n_floats` floats on the exchange stream, `reps` of them back to back (the message of a C3
// step is 6404 floats); 0 without a communicator
extern "C" int tnml_comm_probe(tnml_ctx *c, int n_floats, int reps, double *us_per_allreduce) {
  if (!c || !us_per_allreduce || n_floats < 1 || reps < 1) return fail(TNML_ERR_ARG, "bad argument");
  *us_per_allreduce = 0.0;
  if (!c->comm) return TNML_OK;
  if ((size_t)n_floats > (size_t)c->zstride) return fail(TNML_ERR_ARG, "probe message of %d floats exceeds the pre-gradient buffer (%d)", n_floats, c->zstride);
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipStreamSynchronize(c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream2));
  // (gslabs: scratch of the same size class, not live between sweeps)
  float *buf = c->gslabs ? c->gslabs : c->zslabs;
  if (!buf) return fail(TNML_ERR_STATE, "no pipelined-step buffers yet: run a sweep first");
  for (int w = 0; w < 3; ++w) NCCL_TRY(ncclAllReduce(buf, buf, n_floats, ncclFloat, ncclSum, c->comm, c->stream2));
  HIP_TRY(hipEventRecord(c->ev0, c->stream2));
  for (int r = 0; r < reps; ++r) NCCL_TRY(ncclAllReduce(buf, buf, n_floats, ncclFloat, ncclSum, c->comm, c->stream2));
  HIP_TRY(hipEventRecord(c->ev1, c->stream2));
  HIP_TRY(hipEventSynchronize(c->ev1));
  float ms = 0;
  HIP_TRY(hipEventElapsedTime(&ms, c->ev0, c->ev1));
  *us_per_allreduce = 1e3 * ms / reps;
  return TNML_OK;
}

extern "C" int tnml_set_comm_overlap(tnml_ctx *c, int on) {
  if (!c) return fail(TNML_ERR_ARG, "ctx is NULL");
  c->split.enabled = on != 0;
  return TNML_OK;
}

extern "C" int tnml_set_flag_handoffs(tnml_ctx *c, int on) {
  if (!c) return fail(TNML_ERR_ARG, "ctx is NULL");
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipStreamSynchronize(c->stream));          // nothing of either form in flight while the form changes
  if (c->stream2) HIP_TRY(hipStreamSynchronize(c->stream2));
  c->bigpipe.flags_enabled = on != 0; c->split.flags_enabled = on != 0;
  c->split.done_valid = false; c->split.zsig_valid = false;
  return TNML_OK;
}

extern "C" int tnml_set_any_position(tnml_ctx *c, int on) {
  if (!c) return fail(TNML_ERR_ARG, "ctx is NULL");
  if (c->comm) return fail(TNML_ERR_STATE, "sharded batches with the label at an intermediate site are not supported");
  c->any_pos = on != 0;
  return TNML_OK;
}

extern "C" int tnml_set_chain_path(tnml_ctx *c, int force_plain) {
  if (!c) return fail(TNML_ERR_ARG, "ctx is NULL");
  c->chain_plain = force_plain != 0;
  return TNML_OK;
}

extern "C" int tnml_set_step_pipeline(tnml_ctx *c, int on) {
  if (!c) return fail(TNML_ERR_ARG, "ctx is NULL");
  c->pipe.enabled = on != 0;
  c->bigpipe.enabled = on != 0;
  c->pipe.tiles = on >= 2 ? on : (on == 1 ? 2 : 1);
  drop_pregradients(c);
  return TNML_OK;
}

extern "C" int tnml_set_shape_kernels(tnml_ctx *c, int on) {
  if (!c) return TNML_ERR_ARG;
  c->shape_kernels = on != 0;
  return TNML_OK;
}

extern "C" int tnml_fixed_shape_steps(tnml_ctx *c, int *n_steps) {
  if (!c || !n_steps) return TNML_ERR_ARG;
  *n_steps = c->fixed_steps;
  return TNML_OK;
}

extern "C" int tnml_set_persist_reduce(tnml_ctx *c, int mode) {
  if (!c) return fail(TNML_ERR_ARG, "ctx is NULL");
  if (mode < 0 || mode > 1) return fail(TNML_ERR_ARG, "mode %d outside [0, 1]", mode);
  c->persist_slices = mode == 1;
  return TNML_OK;
}

extern "C" int tnml_slice_reduce_steps(tnml_ctx *c, int *n_steps) {
  if (!c || !n_steps) return TNML_ERR_ARG;
  *n_steps = c->slice_steps;
  return TNML_OK;
}

extern "C" int tnml_set_persistent(tnml_ctx *c, int on) {
  if (!c) return fail(TNML_ERR_ARG, "ctx is NULL");
  if (on < 0 || on > 2) return fail(TNML_ERR_ARG, "mode %d outside [0, 2]", on);
  c->persist_enabled = on != 0;
  if (on) c->persist_mode = on;
  return TNML_OK;
}

extern "C" int tnml_set_sync_interval(tnml_ctx *c, int n_steps) {
  if (!c) return fail(TNML_ERR_ARG, "ctx is NULL");
  if (n_steps < 0) return fail(TNML_ERR_ARG, "negative interval");
  c->sync_interval = n_steps;
  return TNML_OK;
}

extern "C" int tnml_set_svd_stop(tnml_ctx *c, double stop2) {
  if (!c) return fail(TNML_ERR_ARG, "ctx is NULL");
  if (!(stop2 >= 1e-12 && stop2 <= 1e-2)) return fail(TNML_ERR_ARG, "svd stop threshold %g outside [1e-12, 1e-2]", stop2);
  c->svd_stop2 = stop2;
  return TNML_OK;
}

extern "C" int tnml_debug_enable(tnml_ctx *c, int on) {
  if (!c) return fail(TNML_ERR_ARG, "ctx is NULL");
  c->debug = (on & 1) != 0;    // 1: full capture of every step
  c->stamps = (on & 2) != 0;   // 2: cycle stamps only (timing runs)
  c->check_launches = (on & 4) != 0;   // 4: launch status read back after every launch of a step
  return TNML_OK;
}

extern "C" int tnml_get_step_debug(tnml_ctx *c, int what, double *out, size_t capacity, size_t *n_out) {
  if (!c || !out) return fail(TNML_ERR_ARG, "NULL argument");
  if (!c->debug && !(c->stamps && what == TNML_DBG_L2)) return fail(TNML_ERR_STATE, "debug capture is off (tnml_debug_enable)");
  if (c->last_bsize <= 0) return fail(TNML_ERR_STATE, "no step has run yet");
  HIP_TRY(hipSetDevice(c->device));
  const size_t Bs = c->last_bsize;
  std::vector<double> hbuf(4 * Bs + kDbgSigma + kDbgScalars + 8);   // tensors, sigma, 5 scalars, stamps
  HIP_TRY(hipMemcpyAsync(hbuf.data(), c->dbg, (4 * Bs + kDbgSigma + 5) * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(hbuf.data() + 4 * Bs + kDbgSigma + 5, c->dbg + 4 * c->bmax + kDbgSigma + 5, (kDbgScalars - 5) * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  auto tensor_out = [&](size_t block) -> int {
    if (capacity < Bs) return fail(TNML_ERR_ARG, "capacity too small");
    const int D = c->D, L = c->L, h = c->last_h, g = c->last_g;
    const double *src = hbuf.data() + block * Bs;
    if (!c->last_left_dir) {
      memcpy(out, src, Bs * sizeof(double));           // relative == canonical for a right sweep
    } else {
      // relative (h, dk, dk1, g, l) -> canonical (a = g, d = dk1, d' = dk, c = h, l)
      for (int h_ = 0; h_ < h; ++h_) for (int dk = 0; dk < D; ++dk) for (int dk1 = 0; dk1 < D; ++dk1)
        for (int g_ = 0; g_ < g; ++g_) for (int l = 0; l < L; ++l)
          out[((((size_t)g_ * D + dk1) * D + dk) * h + h_) * L + l] = src[((((size_t)h_ * D + dk) * D + dk1) * g + g_) * L + l];
    }
    if (n_out) *n_out = Bs;
    return TNML_OK;
  };
  switch (what) {
    case TNML_DBG_B: return tensor_out(0);
    case TNML_DBG_DB_RAW: return tensor_out(1);
    case TNML_DBG_B_NEW: return tensor_out(2);
    case TNML_DBG_L2_GRAD: return tensor_out(3);
    case TNML_DBG_SIGMA:
      if (capacity < (size_t)c->last_n) return fail(TNML_ERR_ARG, "capacity too small");
      memcpy(out, hbuf.data() + 4 * Bs, c->last_n * sizeof(double));
      if (n_out) *n_out = c->last_n;
      return TNML_OK;
    case TNML_DBG_L2:
      if (capacity < (size_t)kDbgScalars) return fail(TNML_ERR_ARG, "capacity too small");
      memcpy(out, hbuf.data() + 4 * Bs + kDbgSigma, kDbgScalars * sizeof(double));
      if (n_out) *n_out = kDbgScalars;
      return TNML_OK;
  }
  return fail(TNML_ERR_ARG, "unknown debug selector %d", what);
}

// ---------------------------------------------------------------------------------------------
// measurement
// ---------------------------------------------------------------------------------------------
// A phase boundary a profiler can see: an empty kernel of `id` workgroups on the context's stream.  In a rocprofv3 kernel trace (and
// in a --pmc pass, which lists dispatches in the same order) it appears as `tnml_phase_marker_kernel` with Grid_Size = 64 * id, so a
// trace can be cut to the launches between two markers (tools/rocprof_summary.py) -- no clock domain to reconcile, no marker API.
__global__ void tnml_phase_marker_kernel() {}
extern "C" int tnml_marker(tnml_ctx *c, int id) {
  if (!c || id < 1 || id > 1024) return fail(TNML_ERR_ARG, "marker id outside [1, 1024]");
  HIP_TRY(hipSetDevice(c->device));
  hipLaunchKernelGGL(tnml_phase_marker_kernel, dim3(id), dim3(64), 0, c->stream);
  HIP_TRY(hipGetLastError());
  return TNML_OK;
}
extern "C" int tnml_timer_start(tnml_ctx *c) {
  if (!c) return fail(TNML_ERR_ARG, "ctx is NULL");
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipEventRecord(c->ev0, c->stream));
  return TNML_OK;
}
extern "C" int tnml_timer_stop(tnml_ctx *c, double *elapsed_ms) {
  if (!c || !elapsed_ms) return fail(TNML_ERR_ARG, "NULL argument");
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipEventRecord(c->ev1, c->stream));
  HIP_TRY(hipEventSynchronize(c->ev1));
  float ms = 0;
  HIP_TRY(hipEventElapsedTime(&ms, c->ev0, c->ev1));
  *elapsed_ms = ms;
  return TNML_OK;
}
extern "C" int tnml_profile_enable(tnml_ctx *c, int on) {
  if (!c) return fail(TNML_ERR_ARG, "ctx is NULL");
  c->profile = on == 1;            // 1: HIP events around every launch (synchronises after each)
  c->sweep_timing = on == 2;       // 2: one event pair per tnml_sweep call, nothing waits inside the timed region
  return TNML_OK;
}
extern "C" int tnml_profile_get(tnml_ctx *c, int which, double *ms, long long *launches) {
  if (c && (which == 4 || which == 5)) {
    // 4: device time between the first and the last launch of every tnml_sweep call since the last reset, and the number
    //    of kernel launches those calls made; 5: the same time, and the number of single-launch (pipelined) steps
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (size_t i = 0; i + 1 < c->sweep_ev_used; i += 2) {
      float t = 0;
      HIP_TRY(hipEventElapsedTime(&t, c->sweep_ev[i], c->sweep_ev[i + 1]));
      c->sweep_ms += t;
    }
    c->sweep_ev_used = 0;
    if (ms) *ms = c->sweep_ms;
    if (launches) *launches = which == 4 ? c->sweep_launches : c->step_launches;
    return TNML_OK;
  }
  if (!c || which < 0 || which > 3) return fail(TNML_ERR_ARG, "bad argument");
  if (ms) *ms = c->prof_ms[which];
  if (launches) *launches = c->prof_n[which];
  return TNML_OK;
}
extern "C" int tnml_get_counters(tnml_ctx *c, double *out8) {
  if (!c || !out8) return fail(TNML_ERR_ARG, "NULL argument");
  out8[0] = c->cnt_steps; out8[1] = c->cnt_bytes; out8[2] = c->cnt_flops;
  out8[3] = c->cnt_fwd; out8[4] = c->cnt_fwd_bytes;
  out8[5] = (double)c->sweep_launches; out8[6] = (double)c->step_launches; out8[7] = c->sweep_ms;
  return TNML_OK;
}

static int read_counters(tnml_ctx *c, int reset, unsigned long long *h) {
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipMemcpyAsync(h, c->counters, kCounterSlots * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (reset) {        // the Jacobi statistics only: [4..7] belong to the in-kernel timing diagnostics
    HIP_TRY(hipMemsetAsync(c->counters, 0, 4 * sizeof(unsigned long long), c->stream));
    HIP_TRY(hipMemsetAsync(c->counters + 8, 0, (kCounterSlots - 8) * sizeof(unsigned long long), c->stream));
  }
  return TNML_OK;
}

extern "C" int tnml_svd_stats(tnml_ctx *c, int reset, double *out3) {
  if (!c || !out3) return fail(TNML_ERR_ARG, "NULL argument");
  unsigned long long h[kCounterSlots];
  int rc = read_counters(c, reset, h);
  if (rc) return rc;
  out3[0] = (double)h[0]; out3[1] = (double)h[1]; out3[2] = (double)h[2];
  return TNML_OK;
}

extern "C" int tnml_svd_stats_ex(tnml_ctx *c, int reset, double *out, int capacity) {
  if (!c || !out || capacity < 1) return fail(TNML_ERR_ARG, "NULL argument / empty buffer");
  unsigned long long h[kCounterSlots];
  int rc = read_counters(c, reset, h);
  if (rc) return rc;
  for (int i = 0; i < capacity && i < 4; ++i) out[i] = (double)h[i];
  return TNML_OK;
}

extern "C" int tnml_profile_reset(tnml_ctx *c) {
  if (!c) return fail(TNML_ERR_ARG, "ctx is NULL");
  for (int i = 0; i < 4; ++i) { c->prof_ms[i] = 0; c->prof_n[i] = 0; }
  c->sweep_ms = 0; c->sweep_launches = 0; c->step_launches = 0; c->sweep_ev_used = 0;
  c->cnt_steps = c->cnt_bytes = c->cnt_flops = c->cnt_fwd_bytes = c->cnt_fwd = 0;
  return TNML_OK;
}
