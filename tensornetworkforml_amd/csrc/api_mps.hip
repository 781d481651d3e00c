// Host API, algebra on the whole MPS: tnml_orthogonalize / tnml_compress / tnml_bond_spectra, and tnml_inner / tnml_axpby with a
// second chain.
#include "tnml_host.h"

// ---------------------------------------------------------------------------------------------
// orthogonal form about the label, compression, bond spectra (kernels_orth.hip)
// ---------------------------------------------------------------------------------------------
// Scratch group, on the first call: all of it or none (a failed allocation leaves it empty and the call repeatable)
static int orth_ensure(tnml_ctx *c) {
  if (c->orth.ready) return TNML_OK;
  const size_t N = (size_t)c->N, cap = (size_t)c->Mmax;
  HIP_TRY(hipStreamSynchronize(c->stream));
  int rc = make_group(c, "the scratch of the orthogonal form", {
      own_dev(c->orth.W, N * c->core_stride + c->lab_elems), own_dev(c->orth.Mbuf, c->lab_elems), own_dev(c->orth.aux, 4 * cap * cap),
      own_dev(c->orth.sigma, N * cap), own_dev(c->orth.disc, N), own_dev(c->orth.result, 2),
      own_dev(c->orth.out_cores, N * c->core_stride), own_dev(c->orth.out_lab, c->lab_elems),
      own_dev(c->orth.ops, 3 * N + 2), own_dev(c->orth.bond, N), own_dev(c->orth.rank, N), own_dev(c->orth.status, 1)});
  if (rc) return rc;
  c->orth.ready = true;
  return TNML_OK;
}

// mode 0: orthogonal form, 1: compression, 2: spectra only (nothing is committed)
static int orth_impl(tnml_ctx *c, int mode, int m_max, double threshold, double rank_tol, int32_t *bond_out, double *sigma_out,
                     double *discarded_out, double *log_norm_out) {
  const char *what = mode == 0 ? "tnml_orthogonalize" : mode == 1 ? "tnml_compress" : "tnml_bond_spectra";
  if (!c) return fail(TNML_ERR_ARG, "ctx is NULL");
  if (!bond_out || !log_norm_out || (mode != 0 && !sigma_out) || (mode == 1 && !discarded_out))
    return fail(TNML_ERR_ARG, "%s: an output pointer is NULL", what);
  if (mode == 1 && m_max < 1) return fail(TNML_ERR_ARG, "%s: m_max %d < 1", what, m_max);
  if (mode == 1 && !(threshold > 0.0 && threshold <= 1.0)) return fail(TNML_ERR_ARG, "%s: threshold %g outside (0, 1]", what, threshold);
  if (!(rank_tol >= 0.0 && rank_tol < 1.0)) return fail(TNML_ERR_ARG, "%s: rank_tol %g outside [0, 1)", what, rank_tol);
  if (!c->cores_set) return fail(TNML_ERR_STATE, "cores were never set");
  if (c->comm) return fail(TNML_ERR_STATE, "%s runs on one GPU: this context has a communicator attached", what);
  const int N = c->N, l = c->l_pos;
  int mb = 1;
  for (int i = 0; i < N - 1; ++i) mb = std::max(mb, c->bond[i]);
  const size_t lds = orth_chain_lds_bytes(mb);
  if (lds > kLdsMax)
    return fail(TNML_ERR_SHAPE, "%s at bond %d: the Gram matrix and its eigenvectors take %zu bytes of LDS, beyond 160 KB", what, mb, lds);
  HIP_TRY(hipSetDevice(c->device));
  int rc = orth_ensure(c);
  if (rc) return rc;
  // the operations: every decomposition hands its carried factor to the next operation's site
  std::vector<OrthOp> ops;
  // (all three calls walk the same way -- centre to site 0, to site N-1 with the centre on every bond in turn, back to the label:
  // a bond then ends at its Schmidt rank, not at the rank one side shows, and a second call keeps every bond)
  const int cut = mode == 0 ? 0 : mode == 1 ? 2 : 1;
  for (int i = N - 1; i > 0; --i) ops.push_back({i, kOrthLeft, 0, 0});      // rank rule only
  for (int i = 0; i < N - 1; ++i) ops.push_back({i, kOrthRight, cut, 0});   // every bond with the centre on it
  for (int i = N - 1; i > l; --i) ops.push_back({i, kOrthLeft, 0, 0});      // back to the label
  ops.push_back({l, kOrthCentre, 0, 0});
  OrthParams p{};
  p.ops = c->orth.ops; p.n_ops = (int)ops.size();
  p.N = N; p.D = c->D; p.L = c->L; p.l_pos = l;
  p.bond = c->orth.bond; p.cores = c->cores; p.labcore = c->lab[c->lab_cur];
  p.W = c->orth.W; p.Mbuf = c->orth.Mbuf; p.aux = c->orth.aux;
  p.core_stride = c->core_stride; p.lab_elems = c->lab_elems; p.aux_stride = (size_t)c->Mmax * c->Mmax;
  p.m_max = mode == 1 ? m_max : INT_MAX; p.threshold = mode == 1 ? threshold : 1.0; p.rank_tol = rank_tol;
  p.sigma_out = c->orth.sigma; p.sigma_ld = c->Mmax; p.discarded_out = c->orth.disc; p.rank_out = c->orth.rank;
  p.result = c->orth.result; p.status = c->orth.status;
  p.out_cores = c->orth.out_cores; p.out_lab = c->orth.out_lab;
  HIP_TRY(hipMemcpyAsync(c->orth.ops, ops.data(), ops.size() * sizeof(OrthOp), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(c->orth.bond, c->bond.data(), (size_t)(N - 1) * sizeof(int), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemsetAsync(c->orth.status, 0, sizeof(int), c->stream));
  if (!launch_orth(p, mb, c->stream)) {
    (void)hipStreamSynchronize(c->stream);                     // (the uploads read locals of this call)
    return fail(TNML_ERR_SHAPE, "%s: the launch was refused (bond %d)", what, mb);
  }
  HIP_TRY(hipGetLastError());
  int st = 0;
  double res[2] = {0, 0};
  std::vector<int> nb((size_t)N - 1), rk((size_t)N - 1);
  HIP_TRY(hipMemcpyAsync(&st, c->orth.status, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(res, c->orth.result, sizeof res, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(nb.data(), c->orth.bond, nb.size() * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(rk.data(), c->orth.rank, rk.size() * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));                    // (ops is a local: the upload has completed as well)
  if (st == 1 || (st == 0 && !std::isfinite(res[0])))
    return fail(TNML_ERR_NONFINITE, "%s: a core is not finite, beyond 1.8e19 in magnitude or zero, or the result does not fit float32", what);
  if (st) return fail(TNML_ERR_NONFINITE, "%s: the Jacobi iteration or the re-orthogonalisation did not converge (status %d)", what, st);
  for (int i = 0; i < N - 1; ++i)
    if (nb[i] < 1 || nb[i] > c->bond[i]) return fail(TNML_ERR_STATE, "internal: %s produced bond %d at %d (was %d)", what, nb[i], i, c->bond[i]);
  if (mode != 0) {
    HIP_TRY(hipMemcpyAsync(sigma_out, c->orth.sigma, (size_t)(N - 1) * c->Mmax * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (mode == 1) HIP_TRY(hipMemcpyAsync(discarded_out, c->orth.disc, (size_t)(N - 1) * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
  }
  *log_norm_out = res[0];
  if (mode == 2) {
    for (int i = 0; i < N - 1; ++i) bond_out[i] = rk[i];
    return TNML_OK;
  }
  // commit: device-to-device copy, then the bond table
  HIP_TRY(hipMemcpyAsync(c->cores, c->orth.out_cores, (size_t)N * c->core_stride * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(c->lab[c->lab_cur], c->orth.out_lab, c->lab_elems * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
  c->bond = nb;
  for (int i = 0; i < N - 1; ++i) bond_out[i] = nb[i];
  cores_changed(c);
  unbind_optimiser(c);                                          // vel / m / v refer to the old gauge
  return TNML_OK;
}

extern "C" int tnml_orthogonalize(tnml_ctx *c, double rank_tol, int32_t *bond_out, double *log_norm_out) {
  return orth_impl(c, 0, 0, 1.0, rank_tol, bond_out, nullptr, nullptr, log_norm_out);
}

extern "C" int tnml_compress(tnml_ctx *c, int m_max, double threshold, double rank_tol, int32_t *bond_out, double *sigma_out,
                             double *discarded_out, double *log_norm_out) {
  return orth_impl(c, 1, m_max, threshold, rank_tol, bond_out, sigma_out, discarded_out, log_norm_out);
}

extern "C" int tnml_bond_spectra(tnml_ctx *c, double rank_tol, int32_t *rank_out, double *sigma_out, double *log_norm_out) {
  return orth_impl(c, 2, 0, 1.0, rank_tol, rank_out, sigma_out, nullptr, log_norm_out);
}

// ---------------------------------------------------------------------------------------------
// inner products and linear combinations of two MPS (kernels_algebra.hip)
// ---------------------------------------------------------------------------------------------
// The group of the two calls, (re)sized when the second chain or a bond outgrows it: all of it or none
static int alg_ensure(tnml_ctx *c, size_t v_floats, int mb) {
  if (c->alg.v_cap >= v_floats && c->alg.m_cap >= mb && c->alg.m_cap > 0) return TNML_OK;
  const size_t N = (size_t)c->N, D = (size_t)c->D;
  const size_t v_cap = std::max(std::max(c->alg.v_cap, v_floats), (size_t)1);
  const int m_cap = std::max(c->alg.m_cap, mb);
  c->alg.v_cap = 0;
  c->alg.m_cap = 0;
  HIP_TRY(hipStreamSynchronize(c->stream));
  const size_t m2 = (size_t)m_cap * m_cap;
  int rc = make_group(c, "the scratch of the inner products and linear combinations", {
      own_dev(c->alg.V, v_cap), own_dev(c->alg.bond, 2 * N), own_dev(c->alg.off, 2 * N), own_dev(c->alg.metric, N * D * D),
      own_dev(c->alg.stage, 12 * m2 * D), own_dev(c->alg.half_E, 6 * m2), own_dev(c->alg.half_expo, 8), own_dev(c->alg.out, 6),
      own_dev(c->alg.out_cores, N * c->core_stride), own_dev(c->alg.out_lab, c->lab_elems), own_dev(c->alg.status, 1)});
  if (rc) return rc;
  c->alg.v_cap = v_cap;
  c->alg.m_cap = m_cap;
  return TNML_OK;
}

// what both calls check of the second chain; *mb_v: its largest bond
static int alg_check_other(tnml_ctx *c, const char *what, size_t n_floats, const int32_t *other_bond, int other_l_pos, int *mb_v) {
  if (!other_bond) return fail(TNML_ERR_ARG, "%s: other_bond is NULL", what);
  if (other_l_pos != c->l_pos)
    return fail(TNML_ERR_ARG, "%s: the second chain has its label on site %d, this context on site %d", what, other_l_pos, c->l_pos);
  *mb_v = 1;
  for (int i = 0; i < c->N - 1; ++i) {
    if (other_bond[i] < 1) return fail(TNML_ERR_ARG, "%s: bond %d of the second chain is %d", what, i, other_bond[i]);
    *mb_v = std::max(*mb_v, (int)other_bond[i]);
  }
  std::vector<int> nb(other_bond, other_bond + c->N - 1);
  size_t total = 0;
  for (int i = 0; i < c->N; ++i) total += core_elems(c, nb, i, c->l_pos);
  if (total != n_floats) return fail(TNML_ERR_ARG, "%s: other_flat holds %zu floats, its bonds imply %zu", what, n_floats, total);
  return TNML_OK;
}

// the tables of both chains and the second chain's cores to the device; the parameter block without the fields of one call
static int alg_upload(tnml_ctx *c, const float *other_flat, size_t n_floats, const int32_t *other_bond, AlgebraParams *p) {
  const int N = c->N;
  c->alg.bond_host.assign(2 * (size_t)N, 1);
  c->alg.off_host.assign(2 * (size_t)N, 0);
  for (int i = 0; i < N - 1; ++i) c->alg.bond_host[i] = c->bond[i];
  for (int i = 0; i < N; ++i) c->alg.off_host[i] = (long long)((size_t)i * c->core_stride);
  size_t v_lab_off = 0;
  if (other_flat) {
    std::vector<int> nb(other_bond, other_bond + N - 1);
    size_t off = 0;
    for (int i = 0; i < N; ++i) {
      if (i < N - 1) c->alg.bond_host[N - 1 + i] = nb[i];
      c->alg.off_host[N + i] = (long long)off;
      if (i == c->l_pos) v_lab_off = off;
      off += core_elems(c, nb, i, c->l_pos);
    }
    HIP_TRY(hipMemcpyAsync(c->alg.V, other_flat, n_floats * sizeof(float), hipMemcpyHostToDevice, c->stream));
  }
  HIP_TRY(hipMemcpyAsync(c->alg.bond, c->alg.bond_host.data(), 2 * (size_t)N * sizeof(int), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(c->alg.off, c->alg.off_host.data(), 2 * (size_t)N * sizeof(long long), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemsetAsync(c->alg.status, 0, sizeof(int), c->stream));
  *p = AlgebraParams{};
  p->N = N; p->D = c->D; p->L = c->L; p->l_pos = c->l_pos;
  p->n_prod = other_flat ? 3 : 1;
  p->bond = c->alg.bond; p->off = c->alg.off;
  p->w_plain = c->cores; p->w_lab = c->lab[c->lab_cur];
  p->v_plain = other_flat ? c->alg.V : nullptr; p->v_lab = other_flat ? c->alg.V + v_lab_off : nullptr;
  const size_t m2 = (size_t)c->alg.m_cap * c->alg.m_cap;
  p->stage = c->alg.stage; p->stage_stride = m2 * c->D;
  p->half_E = c->alg.half_E; p->half_stride = m2; p->half_expo = c->alg.half_expo;
  p->out = c->alg.out; p->status = c->alg.status;
  p->alpha = 1.0; p->beta = 1.0;
  p->out_cores = c->alg.out_cores; p->out_lab = c->alg.out_lab;
  p->core_stride = c->core_stride; p->lab_elems = c->lab_elems;
  return TNML_OK;
}

extern "C" int tnml_inner(tnml_ctx *c, const float *other_flat, size_t n_floats, const int32_t *other_bond, int other_l_pos,
                          const double *metric, int metric_sites, double *out6) {
  if (!c) return fail(TNML_ERR_ARG, "ctx is NULL");
  if (!out6) return fail(TNML_ERR_ARG, "tnml_inner: out6 is NULL");
  if (metric && metric_sites != 1 && metric_sites != c->N)
    return fail(TNML_ERR_ARG, "tnml_inner: metric_sites %d is neither 1 nor N = %d", metric_sites, c->N);
  int mb_v = 1;
  if (other_flat) {
    int rc = alg_check_other(c, "tnml_inner", n_floats, other_bond, other_l_pos, &mb_v);
    if (rc) return rc;
  }
  if (!c->cores_set) return fail(TNML_ERR_STATE, "cores were never set");
  if (c->comm) return fail(TNML_ERR_STATE, "tnml_inner runs on one GPU: this context has a communicator attached");
  int mb_w = 1;
  for (int i = 0; i < c->N - 1; ++i) mb_w = std::max(mb_w, c->bond[i]);
  if (!other_flat) mb_v = mb_w;
  const size_t lds = algebra_chain_lds_bytes(mb_w, mb_v);
  if (lds > kLdsMax)
    return fail(TNML_ERR_SHAPE, "tnml_inner at bonds %d and %d: the transfer matrix and its product take %zu bytes of LDS, beyond 160 KB",
                mb_w, mb_v, lds);
  HIP_TRY(hipSetDevice(c->device));
  int rc = alg_ensure(c, other_flat ? n_floats : 0, std::max(mb_w, mb_v));
  if (rc) return rc;
  AlgebraParams p;
  rc = alg_upload(c, other_flat, n_floats, other_bond, &p);
  if (rc) { (void)hipStreamSynchronize(c->stream); return rc; }
  if (metric) {
    p.metric = c->alg.metric; p.metric_sites = metric_sites;
    HIP_TRY(hipMemcpyAsync(c->alg.metric, metric, (size_t)metric_sites * c->D * c->D * sizeof(double), hipMemcpyHostToDevice, c->stream));
  }
  if (!launch_inner(p, mb_w, mb_v, c->stream)) {
    (void)hipStreamSynchronize(c->stream);                     // (the uploads read the caller's memory)
    return fail(TNML_ERR_SHAPE, "tnml_inner: the launch was refused (bonds %d and %d)", mb_w, mb_v);
  }
  HIP_TRY(hipGetLastError());
  int st = 0;
  double res[6] = {0, 0, 0, 0, 0, 0};
  HIP_TRY(hipMemcpyAsync(&st, c->alg.status, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(res, c->alg.out, (size_t)2 * p.n_prod * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (st) return fail(TNML_ERR_NONFINITE, "tnml_inner: a core element is not finite");
  for (int k = 0; k < 6; ++k) out6[k] = k < 2 * p.n_prod ? res[k] : (k % 2 ? -INFINITY : 0.0);
  return TNML_OK;
}

extern "C" int tnml_axpby(tnml_ctx *c, double alpha, double beta, const float *other_flat, size_t n_floats,
                          const int32_t *other_bond, int other_l_pos, int32_t *bond_out) {
  if (!c) return fail(TNML_ERR_ARG, "ctx is NULL");
  if (!bond_out || !other_flat) return fail(TNML_ERR_ARG, "tnml_axpby: %s is NULL", bond_out ? "other_flat" : "bond_out");
  if (!std::isfinite(alpha) || !std::isfinite(beta)) return fail(TNML_ERR_ARG, "tnml_axpby: alpha %g or beta %g is not finite", alpha, beta);
  int mb_v = 1;
  int rc = alg_check_other(c, "tnml_axpby", n_floats, other_bond, other_l_pos, &mb_v);
  if (rc) return rc;
  if (!c->cores_set) return fail(TNML_ERR_STATE, "cores were never set");
  if (c->comm) return fail(TNML_ERR_STATE, "tnml_axpby runs on one GPU: this context has a communicator attached");
  const int N = c->N;
  std::vector<int> nb((size_t)N - 1);
  int mb = 1;
  for (int i = 0; i < N - 1; ++i) {
    nb[i] = c->bond[i] + other_bond[i];
    if (nb[i] > c->Mmax)
      return fail(TNML_ERR_ARG, "tnml_axpby: bond %d would become %d + %d = %d, beyond the capacity %d of this context (created with M = %d)",
                  i, c->bond[i], (int)other_bond[i], nb[i], c->Mmax, c->Mpol);
    mb = std::max(mb, nb[i]);
  }
  HIP_TRY(hipSetDevice(c->device));
  rc = alg_ensure(c, n_floats, mb);
  if (rc) return rc;
  AlgebraParams p;
  rc = alg_upload(c, other_flat, n_floats, other_bond, &p);
  if (rc) { (void)hipStreamSynchronize(c->stream); return rc; }
  p.alpha = alpha; p.beta = beta;
  if (!launch_sum_place(p, c->stream)) {
    (void)hipStreamSynchronize(c->stream);
    return fail(TNML_ERR_SHAPE, "tnml_axpby: the launch was refused");
  }
  HIP_TRY(hipGetLastError());
  int st = 0;
  HIP_TRY(hipMemcpyAsync(&st, c->alg.status, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (st) return fail(TNML_ERR_NONFINITE, "tnml_axpby: an element of alpha W + beta V is not a finite float32");
  // commit: device-to-device copy, then the bond table
  HIP_TRY(hipMemcpyAsync(c->cores, c->alg.out_cores, (size_t)N * c->core_stride * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(c->lab[c->lab_cur], c->alg.out_lab, c->lab_elems * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
  c->bond = nb;
  for (int i = 0; i < N - 1; ++i) bond_out[i] = nb[i];
  cores_changed(c);
  unbind_optimiser(c);                                          // vel / m / v refer to the old cores
  return TNML_OK;
}
