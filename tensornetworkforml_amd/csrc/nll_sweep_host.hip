// Host API, two-site likelihood sweep: tnml_nll_sweep / tnml_nll_sweep_indices / tnml_nll_sweep_debug.  The
// kernels of the step are kernels_nll_sweep.hip's; the metric environments are walked once per call by lognorm_env_kernel as it is,
// and the split is reached through run_narrow in the "given merged tensor" mode of tnml_svd_split.
#include "tnml_host.h"

namespace {

// one planned step in the sweep-relative frame: the pair (p, p + 1), the site that keeps the plain core (sb, where the label sits) and
// the one that receives the label (sa); behind / shared / ahead bond, short side, kept rank (the cap under a threshold), launch path
struct SweepStep {
  int p, sb, sa, h, s, g, nn, m, path;
  size_t bsize;
};

// the group of section 30, regrown when a call needs more samples, a larger bond or more steps: all of it or none
int nsw_ensure(tnml_ctx *c, int b_pad, int mcap, int n_steps) {
  auto &g = c->nsw;
  if (b_pad <= g.b_cap && mcap <= g.m_cap && n_steps <= g.steps_cap) return TNML_OK;
  b_pad = std::max(b_pad, g.b_cap); mcap = std::max(mcap, g.m_cap); n_steps = std::max(n_steps, g.steps_cap);
  const size_t N = (size_t)c->N, D = (size_t)c->D, bs = (size_t)mcap * D * D * mcap * c->L, env = (size_t)mcap * b_pad;
  const size_t tiles = (size_t)b_pad / kNllsTile;
  HIP_TRY(hipStreamSynchronize(c->stream));
  g.b_cap = g.m_cap = g.steps_cap = 0;
  g.last_nn = 0;
  int rc = make_group(c, "the buffers of the likelihood sweep", {
      own_dev(g.stack, N * env), own_dev(g.behind[0], env), own_dev(g.behind[1], env), own_dev(g.slabs, tiles * bs), own_dev(g.Gd, bs),
      own_dev(g.B32, bs), own_dev(g.Bout, bs), own_dev(g.B64, bs), own_dev(g.T1, bs), own_dev(g.T2, bs), own_dev(g.dbg, 4 * bs),
      own_dev(g.rec, (size_t)n_steps * kNllsRec), own_dev(g.metric, D * D), own_dev(g.sigma, (size_t)kBigMaxN),
      own_dev(g.sites, 2 * N), own_dev(g.skip, 1)});
  if (rc) return rc;
  g.b_cap = b_pad; g.m_cap = mcap; g.steps_cap = n_steps;
  return TNML_OK;
}

// the site records of a per-sample walk over the plain sites first, first + dir, ... (count of them); every produced environment goes
// to the slot of the next site when `store`
void walk_sites(const tnml_ctx *c, std::vector<NllSweepSite> &out, int first, int count, int dir, bool store, size_t slot_floats) {
  for (int k = 0; k < count; ++k) {
    const int j = first + k * dir, ml = c->ml(j), mr = c->mr(j);
    NllSweepSite q{};
    q.core_off = (long long)((size_t)j * c->core_stride);
    q.x_site = j;
    if (dir > 0) { q.n_in = ml; q.n_out = mr; q.s_in = c->D * mr; q.s_d = mr; q.s_out = 1; }
    else { q.n_in = mr; q.n_out = ml; q.s_in = 1; q.s_d = mr; q.s_out = c->D * mr; }
    q.out_off = store ? (long long)((size_t)(j + dir) * slot_floats) : -1;
    out.push_back(q);
  }
}

int sweep_impl_nll(tnml_ctx *c, const char *what, const float *X, const int32_t *y, const int32_t *idx, int b, bool labelled, const double *S,
                   int left_dir, int n_steps, float lr, int renorm, int max_bond, double threshold, double *values_out) {
  const int N = c->N, D = c->D, L = c->L;
  left_dir = left_dir ? 1 : 0;
  // ---- refusals: nothing is launched before the last of them ----
  if (!c->cores_set) return fail(TNML_ERR_STATE, "cores were never set");
  if (D != kD) return fail(TNML_ERR_ARG, "%s: D = %d (the two-site likelihood sweep runs at D = 2)", what, D);
  if (renorm != 0 && renorm != 1) return fail(TNML_ERR_ARG, "%s: renorm %d is neither 0 nor 1", what, renorm);
  if (n_steps < 1) return fail(TNML_ERR_ARG, "%s: n_steps %d < 1", what, n_steps);
  if (max_bond < 1 || max_bond > c->Mmax) return fail(TNML_ERR_ARG, "%s: max_bond %d outside [1, %d] (the context's bond capacity)", what, max_bond, c->Mmax);
  if (!(threshold > 0.0 && threshold <= 1.0)) return fail(TNML_ERR_ARG, "%s: threshold %g outside (0, 1]", what, threshold);
  if (y)
    for (int i = 0; i < b; ++i)
      if (y[i] < 0 || y[i] >= L) return fail(TNML_ERR_ARG, "label %d of sample %d outside [0, %d)", y[i], i, L);
  const int l0 = c->l_pos, avail = left_dir ? l0 : N - 1 - l0;
  if (n_steps > avail)
    return fail(TNML_ERR_STATE, "%s: %d %s steps asked for, the chain has %d left from l_pos = %d", what, n_steps, left_dir ? "left" : "right", avail, l0);
  size_t total;
  std::vector<int> &tab = c->lnz.tab_host;                      // (a member: the upload below is not waited for)
  int mb, rc = grad_table(c, what, tab, total, mb);
  if (rc) return rc;
  const int mcap = std::max(mb, max_bond), n_metric = S ? 1 : 0;
  if ((rc = lnz_check(c, what, S, n_metric, mcap))) return rc;
  // the plan: with a threshold the bonds can only be smaller than these, and so is every size below
  const bool adaptive = threshold < 1.0;
  std::vector<SweepStep> plan((size_t)n_steps);
  {
    std::vector<int> bond = c->bond;
    auto bl = [&](int i) { return i == 0 ? 1 : bond[i - 1]; };
    auto br = [&](int i) { return i == N - 1 ? 1 : bond[i]; };
    int l = l0;
    for (int k = 0; k < n_steps; ++k) {
      SweepStep &q = plan[k];
      q.sb = l; q.sa = left_dir ? l - 1 : l + 1; q.p = std::min(q.sb, q.sa);
      q.h = left_dir ? br(l) : bl(l); q.s = bond[q.p]; q.g = left_dir ? bl(q.sa) : br(q.sa);
      q.nn = std::min(D * q.h, D * q.g * L);
      q.m = std::min(max_bond, q.nn);
      q.bsize = (size_t)q.h * D * D * q.g * L;
      if (q.nn > kBigMaxN)
        return fail(TNML_ERR_ARG, "%s: the merged matrix of sites (%d, %d) has a short side of %d > %d", what, q.p, q.p + 1, q.nn, kBigMaxN);
      if (q.bsize > c->bmax) return fail(TNML_ERR_ARG, "%s: step at sites (%d, %d) exceeds the buffers sized for M = %d", what, q.p, q.p + 1, c->Mmax);
      if ((q.path = narrow_path(c, q.h, q.g, 1, L, q.m)) < 0) return q.path;
      const int hp = k ? plan[k - 1].h : 0;
      const size_t lds = nll_sweep_batch_lds_bytes(q.h, q.g, hp, D, L);
      if (lds > kLdsMax)
        return fail(TNML_ERR_ARG, "%s: the batch kernel of the step at sites (%d, %d) needs %zu bytes of LDS (bonds %d, %d, %d), beyond 160 KB", what,
                    q.p, q.p + 1, lds, hp, q.h, q.g);
      bond[q.p] = q.m;
      l = q.sa;
    }
  }
  if (nll_sweep_chain_lds_bytes(mcap, D) > kLdsMax)
    return fail(TNML_ERR_ARG, "%s: the chain kernel needs %zu bytes of LDS at bond %d, beyond 160 KB", what, nll_sweep_chain_lds_bytes(mcap, D), mcap);
  // ---- buffers ----
  HIP_TRY(hipSetDevice(c->device));
  if (idx && (rc = ds_upload_indices(c, idx, b))) return rc;    // refuses a bad index before anything is launched
  const int b_pad = (b + kNllsTile - 1) / kNllsTile * kNllsTile, tiles = b_pad / kNllsTile;
  if ((rc = pred_ensure_buffers(c, b_pad))) return rc;
  if ((rc = lnz_ensure(c, mcap, false))) return rc;
  if ((rc = nll_ensure(c, b))) return rc;
  if ((rc = nsw_ensure(c, b_pad, mcap, n_steps))) return rc;
  auto &g = c->nsw;
  const int xbp = c->pred_cap, bp = g.b_cap;             // (row strides; the launches cover this call's tiles)

  const size_t slot = (size_t)g.m_cap * bp, env_stride = (size_t)c->lnz.m_cap * c->lnz.m_cap;
  // ---- once per call: the batch, the norm term's table, metric and walk, both per-sample walks, the guard cleared ----
  if (n_metric) g.metric_host.assign(S, S + (size_t)D * D);
  if ((rc = lnz_upload(c, tab, n_metric ? g.metric_host.data() : nullptr, n_metric, false))) return rc;
  if ((rc = load_chunk(c, X, idx ? c->ds_idx : nullptr, y, 0, b, labelled ? c->ds_ypred : nullptr))) return rc;
  if ((rc = lnz_launch_env(c, n_metric, mb, c->stream))) return rc;
  g.sites_host.clear();
  const SweepStep &q0 = plan[0];
  int n_behind, n_ahead;
  if (!left_dir) {
    walk_sites(c, g.sites_host, 0, q0.sb, +1, false, slot);
    n_behind = (int)g.sites_host.size();
    walk_sites(c, g.sites_host, N - 1, N - 1 - q0.sa, -1, true, slot);
  } else {
    walk_sites(c, g.sites_host, N - 1, N - 1 - q0.sb, -1, false, slot);
    n_behind = (int)g.sites_host.size();
    walk_sites(c, g.sites_host, 0, q0.sa, +1, true, slot);
  }
  n_ahead = (int)g.sites_host.size() - n_behind;
  if (!g.sites_host.empty())
    HIP_TRY(hipMemcpyAsync(g.sites, g.sites_host.data(), g.sites_host.size() * sizeof(NllSweepSite), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemsetAsync(g.skip, 0, sizeof(int), c->stream));
  HIP_TRY(hipMemsetAsync(c->red, 0, (size_t)c->slab_stride * sizeof(float), c->stream));   // (the split's raw gradient: none)
  {
    NllSweepChainParams p{};
    p.cores = c->cores; p.X = c->Xpred; p.stack = g.stack; p.b_pad = bp; p.x_bpad = xbp; p.D = D; p.cap = g.m_cap;
    p.sites = g.sites; p.n_sites = n_behind; p.init_off = -1; p.last_out = g.behind[0];
    if (!launch_nll_sweep_chain(p, tiles, c->stream)) return fail(TNML_ERR_ARG, "internal: chain launch of the likelihood sweep refused");
    p.sites = g.sites + n_behind; p.n_sites = n_ahead; p.init_off = (long long)((size_t)(left_dir ? 0 : N - 1) * slot); p.last_out = nullptr;
    if (!launch_nll_sweep_chain(p, tiles, c->stream)) return fail(TNML_ERR_ARG, "internal: chain launch of the likelihood sweep refused");
    HIP_TRY(hipGetLastError());
  }
  cores_changed(c);                                             // from here on
  unbind_optimiser(c);
  const double *Sdev = n_metric ? c->lnz.metric : nullptr;
  for (int k = 0; k < n_steps; ++k) {
    SweepStep q = plan[k];
    // (with a threshold the bonds are what the steps before kept)
    q.h = left_dir ? c->mr(q.sb) : c->ml(q.sb); q.s = c->bond[q.p]; q.g = left_dir ? c->ml(q.sa) : c->mr(q.sa);
    q.nn = std::min(D * q.h, D * q.g * L); q.m = std::min(max_bond, q.nn); q.bsize = (size_t)q.h * D * D * q.g * L;
    if (adaptive && (q.path = narrow_path(c, q.h, q.g, 1, L, q.m)) < 0) return q.path;
    const int h = q.h, s = q.s, gg = q.g, m = q.m;
    NarrowParams n{};
    n.L = L; n.D = D; n.h = h; n.g = gg; n.s = 1; n.m = m; n.bsize = (int)q.bsize;
    NllSweepMergeParams mp{};
    mp.h = h; mp.g = gg; mp.s = s; mp.D = D; mp.L = L; mp.B64 = g.B64; mp.B32 = g.B32;
    mp.lab.base = c->lab[c->lab_cur]; mp.lab.n_in = h; mp.lab.n_out = s;
    mp.pl.base = c->core_slot(q.sa); mp.pl.n_in = s; mp.pl.n_out = gg;
    if (!left_dir) {
      mp.lab.s_in = D * s * L; mp.lab.s_d = s * L; mp.lab.s_out = L;
      mp.pl.s_in = D * gg; mp.pl.s_d = gg; mp.pl.s_out = 1;
      n.ob_s_h = D * m; n.ob_s_d = m; n.ob_s_m = 1;
      n.oa_s_m = D * gg * L; n.oa_s_d = gg * L; n.oa_s_g = L;
    } else {
      mp.lab.s_in = L; mp.lab.s_d = h * L; mp.lab.s_out = D * h * L;
      mp.pl.s_in = 1; mp.pl.s_d = s; mp.pl.s_out = D * s;
      n.ob_s_h = 1; n.ob_s_d = h; n.ob_s_m = D * h;
      n.oa_s_m = L; n.oa_s_d = m * L; n.oa_s_g = D * m * L;
    }
    if (!launch_nll_sweep_merge(mp, c->stream)) return fail(TNML_ERR_ARG, "internal: merge launch of the likelihood sweep refused");
    // ---- batch side ----
    NllSweepBatchParams bp_{};
    bp_.b = b; bp_.b_pad = bp; bp_.x_bpad = xbp; bp_.D = D; bp_.L = L; bp_.batch = b;
    bp_.h = h; bp_.g = gg;
    bp_.x_k = c->Xpred + (size_t)q.sb * xbp * D; bp_.x_kp1 = c->Xpred + (size_t)q.sa * xbp * D;
    bp_.Hcur = g.behind[k & 1];
    if (k) {
      const int prev = left_dir ? q.sb + 1 : q.sb - 1, hp = left_dir ? c->mr(prev) : c->ml(prev);
      bp_.do_ext = 1; bp_.hp = hp;
      bp_.x_km1 = c->Xpred + (size_t)prev * xbp * D;
      bp_.Hprev = g.behind[(k - 1) & 1];
      bp_.ext_core.base = c->core_slot(prev); bp_.ext_core.n_in = hp; bp_.ext_core.n_out = h;
      if (!left_dir) { bp_.ext_core.s_in = D * h; bp_.ext_core.s_d = h; bp_.ext_core.s_out = 1; }
      else { bp_.ext_core.s_in = 1; bp_.ext_core.s_d = hp; bp_.ext_core.s_out = D * hp; }
    }
    bp_.G = g.stack + (size_t)q.sa * slot;
    bp_.B32 = g.B32; bp_.y = labelled ? c->ds_ypred : nullptr;
    bp_.slabs = g.slabs; bp_.terms = c->nll.terms; bp_.bad = c->nll.bad;
    if (!launch_nll_sweep_batch(bp_, tiles, c->stream))
      return fail(TNML_ERR_ARG, "internal: batch launch of the likelihood sweep refused (bonds %d, %d)", h, gg);
    if (!launch_nll_sweep_reduce(g.slabs, tiles, (int)q.bsize, g.Gd, c->stream)) return fail(TNML_ERR_ARG, "internal: reduction launch refused");
    if (!launch_nll_sum(c->nll.terms, c->nll.bad, b, c->nll.acc, c->stream)) return fail(TNML_ERR_ARG, "internal: likelihood sum launch refused");
    // ---- norm term, update, guard, record ----
    const int ih = left_dir ? q.p + 2 : q.p, ig = left_dir ? q.p : q.p + 2;
    double *envH = left_dir ? c->lnz.envR : c->lnz.envL, *envG = left_dir ? c->lnz.envL : c->lnz.envR;
    int *expH = left_dir ? c->lnz.expR : c->lnz.expL, *expG = left_dir ? c->lnz.expL : c->lnz.expR;
    NllSweepUpdateParams up{};
    up.D = D; up.L = L; up.h = h; up.g = gg; up.bsize = (int)q.bsize; up.batch = b; up.renorm = renorm; up.lr = lr;
    up.B64 = g.B64; up.Gd = g.Gd;
    up.Nh = envH + (size_t)ih * env_stride; up.Ng = envG + (size_t)ig * env_stride; up.expH = expH + ih; up.expG = expG + ig;
    up.S = Sdev; up.acc = c->nll.acc; up.env_status = c->lnz.status;
    up.T1 = g.T1; up.T2 = g.T2; up.Bout = g.Bout; up.dbg = g.dbg; up.rec = g.rec + (size_t)k * kNllsRec; up.skip = g.skip;
    if (!launch_nll_sweep_update(up, c->stream)) return fail(TNML_ERR_ARG, "internal: update launch of the likelihood sweep refused");
    HIP_TRY(hipGetLastError());
    // ---- the split: tensor_svd of the given merged tensor (tnml_svd_split's launch), new cores into their slots ----
    n.red = c->red;
    n.Bnew = c->Bscr2;
    n.out_behind = c->core_slot(q.sb);
    n.out_ahead = c->lab[c->lab_cur ^ 1];
    n.dbg = c->dbg; n.status = c->status; n.counters = c->counters;
    n.Bdirect = g.Bout;
    n.svd_stop2 = c->svd_stop2;
    n.chol_thr = c->chol_thr;
    if (adaptive) { n.trunc_thr = threshold; n.left_dir = left_dir; n.m_out = c->status + 1; }
    if ((rc = run_narrow(c, n, q.path))) return rc;
    HIP_TRY(hipGetLastError());
    // ---- behind metric environment through the new plain core, the record of the split ----
    NllSweepExtendParams ep{};
    ep.right_walk = left_dir; ep.D = D;
    ep.ml = left_dir ? m : h; ep.mr = left_dir ? h : m;
    ep.m_dev = adaptive ? c->status + 1 : nullptr; ep.m_fixed = m;
    ep.core = c->core_slot(q.sb); ep.S = Sdev;
    const int io = q.p + 1;                                      // L_{p+1} (right step) or R_{p+1} (left step)
    ep.Ein = up.Nh; ep.Eout = envH + (size_t)io * env_stride; ep.exp_in = up.expH; ep.exp_out = expH + io;
    ep.sigma = c->dbg + 4 * q.bsize; ep.n_sigma = q.nn; ep.sigma_out = g.sigma;
    ep.rec = up.rec; ep.status = c->lnz.status;
    if (!launch_nll_sweep_extend(ep, c->lnz.m_cap, c->stream)) return fail(TNML_ERR_ARG, "internal: environment launch of the likelihood sweep refused");
    HIP_TRY(hipGetLastError());
    int m_kept = m;
    if (adaptive) {                                              // the kept rank is decided on the device: one wait per step
      HIP_TRY(hipMemcpyAsync(&m_kept, c->status + 1, sizeof(int), hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(hipStreamSynchronize(c->stream));
      if (m_kept < 1 || m_kept > m) return fail(TNML_ERR_NONFINITE, "%s: adaptive truncation returned rank %d (cap %d)", what, m_kept, m);
    }
    c->bond[q.p] = m_kept;
    c->l_pos = q.sa;
    c->lab_cur ^= 1;
    g.last_h = h; g.last_g = gg; g.last_nn = q.nn; g.last_left = left_dir;
  }
  std::vector<double> rec((size_t)n_steps * kNllsRec);
  HIP_TRY(hipMemcpyAsync(rec.data(), g.rec, rec.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  int bad = -1;
  for (int k = 0; k < n_steps; ++k) {
    for (int j = 0; j < kNllsRec; ++j) values_out[(size_t)k * kNllsRec + j] = rec[(size_t)k * kNllsRec + j];
    if (((int)rec[(size_t)k * kNllsRec + 3] & kNllStepNotApplied) && bad < 0) bad = k;
  }
  if ((rc = check_status(c))) return rc;
  if (bad >= 0)
    return fail(TNML_ERR_NONFINITE, "%s: step %d of %d saw %g samples with a cotangent that is not finite (f_y == 0, or an f beyond float32: calibrate "
                "the network), norm status %d; from that step on the call re-gauged without updating", what, bad, n_steps,
                rec[(size_t)bad * kNllsRec + 2], (int)rec[(size_t)bad * kNllsRec + 3] & 7);
  return TNML_OK;
}

}  // namespace

extern "C" int tnml_nll_sweep(tnml_ctx *c, const float *X, const int32_t *y, int b, const double *S, int left_dir, int n_steps, float lr,
                              int renorm, int max_bond, double threshold, double *values_out) {
  if (!c || !X || !values_out) return fail(TNML_ERR_ARG, "NULL argument");
  if (c->comm) return fail(TNML_ERR_STATE, "the likelihood sweep is single-GPU only: a communicator is attached");
  if (b < 1) return fail(TNML_ERR_ARG, "empty batch");
  return sweep_impl_nll(c, "tnml_nll_sweep", X, y, nullptr, b, y != nullptr, S, left_dir, n_steps, lr, renorm, max_bond, threshold, values_out);
}

extern "C" int tnml_nll_sweep_indices(tnml_ctx *c, const int32_t *idx, int b, int use_labels, const double *S, int left_dir, int n_steps,
                                      float lr, int renorm, int max_bond, double threshold, double *values_out) {
  int rc = ds_usable(c);
  if (rc) return rc;
  if (!idx || !values_out) return fail(TNML_ERR_ARG, "NULL argument");
  if (b < 1) return fail(TNML_ERR_ARG, "empty index list");
  return sweep_impl_nll(c, "tnml_nll_sweep_indices", nullptr, nullptr, idx, b, use_labels != 0, S, left_dir, n_steps, lr, renorm, max_bond,
                        threshold, values_out);
}

extern "C" int tnml_nll_sweep_debug(tnml_ctx *c, int what, double *out, size_t capacity, size_t *n_out) {
  if (!c || !out || !n_out) return fail(TNML_ERR_ARG, "NULL argument");
  if (what < TNML_NLL_SWEEP_B || what > TNML_NLL_SWEEP_SIGMA) return fail(TNML_ERR_ARG, "tnml_nll_sweep_debug: unknown selector %d", what);
  const auto &g = c->nsw;
  if (!g.last_nn || !g.b_cap) return fail(TNML_ERR_STATE, "tnml_nll_sweep_debug: no step of a likelihood sweep has run");
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipStreamSynchronize(c->stream));
  const int D = c->D, L = c->L, h = g.last_h, gg = g.last_g;
  if (what == TNML_NLL_SWEEP_SIGMA) {
    if (capacity < (size_t)g.last_nn) return fail(TNML_ERR_ARG, "capacity too small");
    HIP_TRY(hipMemcpy(out, g.sigma, (size_t)g.last_nn * sizeof(double), hipMemcpyDeviceToHost));
    *n_out = (size_t)g.last_nn;
    return TNML_OK;
  }
  const size_t bs = (size_t)h * D * D * gg * L;
  if (capacity < bs) return fail(TNML_ERR_ARG, "capacity too small");
  std::vector<double> rel(bs);
  HIP_TRY(hipMemcpy(rel.data(), g.dbg + (size_t)what * bs, bs * sizeof(double), hipMemcpyDeviceToHost));
  if (!g.last_left) std::copy(rel.begin(), rel.end(), out);
  else {
    // relative [h = mr][e][d][g = ml][l] -> canonical [ml][d][e][mr][l]
    const int ml = gg, mr = h;
    for (int a = 0; a < ml; ++a)
      for (int d = 0; d < D; ++d)
        for (int e = 0; e < D; ++e)
          for (int cc = 0; cc < mr; ++cc)
            for (int l = 0; l < L; ++l)
              out[((((size_t)a * D + d) * D + e) * mr + cc) * L + l] = rel[((((size_t)cc * D + e) * D + d) * ml + a) * L + l];
  }
  *n_out = bs;
  return TNML_OK;
}
