// Host API, likelihood training from incomplete data: tnml_nll_masked_grad / tnml_nll_masked_step.  The
// environments are walked by sample_env_masked_kernel as it is, on the tables, the stack and the chunks of tnml_sample_masked; the
// gradient kernels are kernels_nll_masked.hip's, and the step is the update kernel of tnml_gd_step on their gradient.
#include "tnml_host.h"

namespace {

// the group of section 31, regrown when a call needs more of any member: all of it or none
int nmg_ensure(tnml_ctx *c, size_t rows, size_t lf, size_t part, size_t total) {
  auto &g = c->nmg;
  if (g.total_cap > 0 && g.rows_cap >= rows && g.lf_cap >= lf && g.part_cap >= part && g.total_cap >= total) return TNML_OK;
  const size_t rows_cap = std::max(g.rows_cap, rows), lf_cap = std::max(g.lf_cap, lf), part_cap = std::max(g.part_cap, part);
  const size_t total_cap = std::max(g.total_cap, total);
  g.rows_cap = g.lf_cap = g.part_cap = g.total_cap = 0;
  HIP_TRY(hipStreamSynchronize(c->stream));
  int rc = make_group(c, "the buffers of the masked likelihood gradient", {
      own_dev(g.tab, 2 * (size_t)c->N), own_dev(g.wrow, rows_cap), own_dev(g.lf_next, lf_cap), own_dev(g.part, part_cap),
      own_dev(g.acc, total_cap), own_dev(g.G, total_cap), own_dev(g.status, 2)});
  if (rc) return rc;
  g.rows_cap = rows_cap; g.lf_cap = lf_cap; g.part_cap = part_cap; g.total_cap = total_cap;
  return TNML_OK;
}

// What both calls share: the refusals, the class-slot tiles, the chunks under the stack budget, the launches, and out4 =
// {value, log Z, samples with E_s = -inf or not finite, status bits}.  grad: the gradient is left in c->nmg.G (total floats).
// TNML_ERR_NONFINITE (a bad sample, a bad normaliser, a status bit) comes back with out4 written.
int nmg_run(tnml_ctx *c, const char *what, int n, int K, const double *phi, const double *w, const int32_t *classes, const uint8_t *mask,
            int mask_rows, const int32_t *known, bool grad, size_t capacity, double *logp_out, double *out4, size_t *total_out) {
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
  if ((rc = smp_check_state(c, what))) return rc;
  auto &g = c->smk;
  auto &h = c->nmg;
  size_t total;
  int mb;
  if ((rc = grad_table(c, what, h.tab_host, total, mb))) return rc;
  if (total_out) *total_out = total;
  if (grad && capacity < total) return fail(TNML_ERR_ARG, "%s: capacity %zu < %zu floats", what, capacity, total);
  const int T = masked_grad_tile(mb, D, L, K);
  if (T < 1)
    return fail(TNML_ERR_SHAPE, "%s at bond %d, D = %d, L = %d, K = %d: the core, both environments and the products of one sample take "
                "%zu bytes of LDS (160 KB and bonds up to %d fit)", what, mb, D, L, K,
                std::max(sample_masked_env_lds_bytes(mb, D, 1), masked_grad_lds_bytes(mb, D, K, 1)), kNmgMaxBond);
  const size_t m2 = (size_t)mb * mb, tile_stack = (size_t)T * (N + 1) * m2, tile_need = tile_stack + (grad ? total : 0);
  if (g.stack_bytes / sizeof(double) < tile_need)
    return fail(TNML_ERR_ARG, "%s: one tile of %d samples needs %zu bytes of stack%s, the budget of tnml_set_sample_stack_bytes is %zu",
                what, T, tile_need * sizeof(double), grad ? " and partial gradient" : "", g.stack_bytes);
  // rows of class slot -1: the normaliser (the empty mask), then its samples; rows of a slot c >= 0: its samples; slots in the order
  // -1, 0 .. L-1 of those the call uses; tiles of T rows of one slot each, padded with empty masks of weight 0
  std::vector<int> count((size_t)L + 1, 0), next((size_t)L + 1, 0);
  for (int s = 0; s < n; ++s) count[(classes ? classes[s] : -1) + 1]++;
  int n_tiles = 0;
  const size_t o_tcls = (size_t)N;
  std::vector<int> first_tile((size_t)L + 1, -1);
  for (int q = 0; q <= L; ++q) {
    const int nrows = count[q] + (q == 0 ? 1 : 0);
    if (!nrows) continue;
    first_tile[q] = n_tiles;
    next[q] = n_tiles * T + (q == 0 ? 1 : 0);
    n_tiles += (nrows + T - 1) / T;
  }
  const size_t rows = (size_t)n_tiles * T;
  // host tables: bond [N] | tile_class [n_tiles] | tile_rows [rows] | row of sample [n]
  const size_t o_rows = o_tcls + n_tiles, o_rof = o_rows + rows;
  g.host.assign(o_rof + n, -1);
  smp_bond_table(c, g.host);
  for (int q = 0, t = 0; q <= L; ++q)
    if (first_tile[q] >= 0) {
      const int nt = (count[q] + (q == 0 ? 1 : 0) + T - 1) / T;
      for (int k = 0; k < nt; ++k) g.host[o_tcls + t++] = q - 1;
    }
  h.wrow_host.assign(rows, 0.0);
  h.wrow_host[0] = -2.0;                                         // (slot -1 comes first and its first row is the normaliser)
  for (int s = 0; s < n; ++s) {
    const int q = (classes ? classes[s] : -1) + 1;
    g.host[o_rof + s] = next[q];
    h.wrow_host[next[q]] = 2.0 / (double)n;
    g.host[o_rows + next[q]++] = s;
  }
  smp_grid_metric(g.hostd, K, D, phi, w);
  const size_t chunk_tiles = std::min((size_t)n_tiles, g.stack_bytes / sizeof(double) / tile_need);
  HIP_TRY(hipSetDevice(c->device));
  if ((rc = smk_ensure(c, (size_t)n_tiles, rows, (size_t)n, (size_t)mask_rows, 0, chunk_tiles * tile_stack))) return rc;
  if (grad && (rc = nmg_ensure(c, rows, chunk_tiles * T * m2, chunk_tiles * total, total))) return rc;
  static const int init_status[2] = {0, INT_MAX};
  HIP_TRY(hipMemcpyAsync(g.bond, g.host.data(), (size_t)N * sizeof(int), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(g.tile_class, g.host.data() + o_tcls, (size_t)n_tiles * sizeof(int), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(g.tile_rows, g.host.data() + o_rows, rows * sizeof(int), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(g.mask, mask, (size_t)mask_rows * N, hipMemcpyHostToDevice, c->stream));
  if (known) HIP_TRY(hipMemcpyAsync(g.known, known, (size_t)n * N * sizeof(int), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(g.S, g.hostd.data(), (size_t)D * D * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(g.phi, phi, (size_t)K * D * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(g.w, w, (size_t)K * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(g.status, init_status, sizeof init_status, hipMemcpyHostToDevice, c->stream));
  if (grad) {
    HIP_TRY(hipMemcpyAsync(h.tab, h.tab_host.data(), h.tab_host.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(h.wrow, h.wrow_host.data(), rows * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemsetAsync(h.status, 0, 2 * sizeof(int), c->stream));
  }
  MaskedGradParams gp{};
  SampleMaskedParams &p = gp.m;
  p.N = N; p.D = D; p.L = L; p.l_pos = c->l_pos; p.K = K; p.n = n; p.T = T; p.mask_rows = mask_rows;
  p.bond = g.bond; p.cores = c->cores; p.lab = c->lab[c->lab_cur]; p.core_stride = c->core_stride;
  p.S = g.S; p.phi = g.phi; p.w = g.w; p.mask = g.mask; p.known = g.known;
  p.stack = g.stack; p.env_stride = m2;
  p.levels = g.levels; p.labels = g.labels; p.logp0 = g.logp0; p.status = g.status;
  if (grad) { gp.off = h.tab + N; gp.lf_next = h.lf_next; gp.part = h.part; gp.total = total; gp.status = h.status; }
  // chunks of whole tiles: every chunk reuses the stack and the partial buffer, the launches of one stream follow each other
  for (size_t t0 = 0; t0 < (size_t)n_tiles; t0 += chunk_tiles) {
    p.n_tiles = (int)std::min(chunk_tiles, (size_t)n_tiles - t0);
    p.tile_class = g.tile_class + t0; p.tile_rows = g.tile_rows + t0 * T; p.E = g.E + t0 * T;
    if (grad) gp.wrow = h.wrow + t0 * T;
    if (!(grad ? launch_masked_grad(gp, mb, c->stream) : launch_sample_masked(p, mb, false, c->stream))) {
      (void)hipStreamSynchronize(c->stream);                     // (the uploads read the caller's memory)
      return fail(TNML_ERR_SHAPE, "%s: the launch was refused (bond %d)", what, mb);
    }
    HIP_TRY(hipGetLastError());
    if (grad) {
      MaskedGradReduceParams r{};
      r.part = h.part; r.acc = h.acc; r.G = h.G; r.total = total; r.n_tiles = p.n_tiles;
      r.first = t0 == 0; r.last = t0 + chunk_tiles >= (size_t)n_tiles; r.status = h.status;
      if (!launch_masked_grad_reduce(r, c->stream)) {
        (void)hipStreamSynchronize(c->stream);
        return fail(TNML_ERR_ARG, "internal: masked gradient reduction launch refused");
      }
      HIP_TRY(hipGetLastError());
    }
  }
  int st[2] = {0, 0}, sg[2] = {0, 0};
  g.hostE.resize(rows);
  HIP_TRY(hipMemcpyAsync(st, g.status, sizeof st, hipMemcpyDeviceToHost, c->stream));
  if (grad) HIP_TRY(hipMemcpyAsync(sg, h.status, sizeof sg, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(g.hostE.data(), g.E, rows * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  const double *E = g.hostE.data();
  const double logz = E[0];
  int bits = (st[0] & 1) | sg[0], bad = 0;
  double sum = 0.0;
  for (int s = 0; s < n; ++s) {
    const double e = E[g.host[o_rof + s]];
    if (!std::isfinite(e)) ++bad;
    sum += e - logz;
    if (logp_out) logp_out[s] = e - logz;
  }
  out4[0] = -(sum / (double)n);
  out4[1] = logz;
  out4[2] = (double)bad;
  out4[3] = (double)bits;
  if (!std::isfinite(logz))
    return fail(TNML_ERR_NONFINITE, "%s: the normaliser log Z is %g (the model is zero, or a core element is not finite)", what, logz);
  if (bad > 0)
    return fail(TNML_ERR_NONFINITE, "%s: %d of %d samples have known pixels (or a class) of zero weight, or a likelihood that is not finite", what,
                bad, n);
  if (bits)
    return fail(TNML_ERR_NONFINITE, "%s: status %d (1 a non-finite environment, 2 a per-site normaliser that is not positive, 4 a gradient "
                "element beyond float32)", what, bits);
  return TNML_OK;
}

}  // namespace

extern "C" int tnml_nll_masked_grad(tnml_ctx *c, int n, int K, const double *phi, const double *w, const int32_t *classes, const uint8_t *mask,
                                    int mask_rows, const int32_t *known, float *grad_flat, size_t capacity, double *logp_out, double *out4) {
  if (!c) return fail(TNML_ERR_ARG, "ctx is NULL");
  if (!out4) return fail(TNML_ERR_ARG, "tnml_nll_masked_grad: out4 is NULL");
  size_t total = 0;
  int rc = nmg_run(c, "tnml_nll_masked_grad", n, K, phi, w, classes, mask, mask_rows, known, grad_flat != nullptr, capacity, logp_out, out4, &total);
  if (rc || !grad_flat) return rc;
  HIP_TRY(hipMemcpyAsync(grad_flat, c->nmg.G, total * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return TNML_OK;
}

extern "C" int tnml_nll_masked_step(tnml_ctx *c, int n, int K, const double *phi, const double *w, const int32_t *classes, const uint8_t *mask,
                                    int mask_rows, const int32_t *known, float lr, float weight_dec, int renorm, double *values4) {
  const char *what = "tnml_nll_masked_step";
  if (!c) return fail(TNML_ERR_ARG, "ctx is NULL");
  if (!values4) return fail(TNML_ERR_ARG, "%s: values4 is NULL", what);
  if (renorm != 0 && renorm != 1) return fail(TNML_ERR_ARG, "%s: renorm %d is neither 0 nor 1", what, renorm);
  const bool stateful = opt_stateful(c);
  if (stateful && c->opt_s0 && (c->opt.bond != c->bond || c->opt.l_pos != c->l_pos))
    return fail(TNML_ERR_STATE, "the optimiser state belongs to other bonds or another l_pos (l_pos %d then, %d now): call tnml_optim_reset",
                c->opt.l_pos, c->l_pos);
  // the gradient first, with its one wait: a bad batch is known on the host before the update is enqueued (THE GUARD)
  int rc = nmg_run(c, what, n, K, phi, w, classes, mask, mask_rows, known, true, (size_t)-1, nullptr, values4, nullptr);
  if (rc) {
    if (rc == TNML_ERR_NONFINITE) values4[3] = (double)((int)values4[3] | (values4[2] > 0 ? kNllStepBadBatch : 0) | kNllStepNotApplied);
    return rc;
  }
  if ((rc = opt_ensure_state(c))) return rc;
  cores_changed(c);                                             // from here on
  OptimStepParams o{};
  o.tab = c->nmg.tab; o.cores = c->cores; o.labcore = c->lab[c->lab_cur]; o.G = c->nmg.G;
  o.s0 = stateful ? c->opt_s0 : nullptr; o.s1 = c->opt.kind == TNML_OPT_ADAM ? c->opt_s1 : nullptr;
  o.core_stride = c->core_stride; o.N = c->N; o.D = c->D; o.L = c->L; o.l_pos = c->l_pos;
  o.kind = c->opt.kind; o.clip = c->opt.clip; o.lr = lr; o.wd = weight_dec;
  o.mu = c->opt.momentum; o.beta1 = c->opt.beta1; o.beta2 = c->opt.beta2; o.eps = c->opt.eps;
  o.corr1 = o.corr2 = 1.0;
  if (c->opt.kind == TNML_OPT_ADAM) {
    const double t = (double)++c->opt.t;
    o.corr1 = 1.0 - std::pow(c->opt.beta1, t);
    o.corr2 = 1.0 - std::pow(c->opt.beta2, t);
  }
  o.renorm = renorm; o.skip = nullptr;
  if (!launch_optim_step(o, c->stream)) return fail(TNML_ERR_ARG, "internal: optimiser step launch refused");
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(c->stream));
  return TNML_OK;
}
