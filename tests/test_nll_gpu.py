"""tnml_log_norm_grad on the device against the float64 reference of tests/nll_reference.py.  Every comparison
is with the reference; the bounds are derived, not measured:
    Gz, per site      2^-22 max|Gz_i|: one float32 rounding of the output is 2^-24 relative, and the float64 sums of at most
                      N m^2 D^2 terms stay far below that
    log|Z|            N m^2 D^2 2^-52 absolute, against the reference and against the device's own tnml_inner
    sum(Gz_i A_i)     2 within 2^-22 sum|Gz_i A_i|, on the device's output
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p_ in (ROOT, HERE):
    if p_ not in sys.path:
        sys.path.insert(0, p_)

import mps_algebra_reference as A                                  # noqa: E402
import nll_reference as R                                          # noqa: E402
from tensornetworkforml_amd import _hip                            # noqa: E402

pytestmark = pytest.mark.gpu

ARG, STATE, NONFINITE = -1, -2, -7
G_TOL = 2.0 ** -22


def _code(call):
    with pytest.raises(_hip.TnmlError) as ei:
        call()
    return ei.value.code


def context_M(D, cap, L):
    """the smallest M whose bond capacity max(M, D min(L, M)) holds `cap`"""
    return next(M for M in range(1, cap + 1) if max(M, D * min(L, M)) >= cap)


def new_ctx(cores, l, D, L, b=64):
    cap = max(c.shape[2] for c in cores)
    ctx = _hip.Context(len(cores), D, L, context_M(D, cap, L), b)
    ctx.set_any_position(True)
    ctx.set_cores(A.as32(cores), l)
    return ctx


def log_tol(cores, D):
    m = max(c.shape[2] for c in cores)
    return len(cores) * m * m * D * D * 2.0 ** -52


def check_against_reference(ctx, cores, l, D, metric, what):
    """the device's Gz and log|Z| against the reference and against tnml_inner, and the identity on the device's output"""
    G, (sign, logz) = ctx.log_norm_grad(metric)
    Gr, (sr, lr) = R.log_norm_gradient(cores, l, metric)
    tol = log_tol(cores, D)
    assert sign == sr and abs(logz - lr) <= tol, (what, sign, sr, logz, lr, tol)
    own = ctx.inner(None, 0, metric)[0]
    assert own[0] == sign and abs(own[1] - logz) <= tol, (what, own, logz, tol)
    for i, (g, gr) in enumerate(zip(G, Gr)):
        assert g.dtype == np.float32 and g.shape == gr.shape and np.isfinite(g).all(), (what, i)
        err, scale = float(np.abs(g - gr).max()), float(np.abs(gr).max())
        assert err <= G_TOL * scale, (what, i, err, scale)
        prod = g.astype(np.float64) * cores[i]
        assert abs(float(prod.sum()) - 2.0) <= G_TOL * float(np.abs(prod).sum()), (what, i, float(prod.sum()))
    return G, (sign, logz)


def bits(ctx):
    cores, bond, lp = ctx.get_cores()
    slots, lab = ctx.core_slots()
    return [c.tobytes() for c in cores], bond.tobytes(), lp, slots.tobytes(), lab.tobytes()


# ---------------------------------------------------------------------------------------------------------------
# 1. every shared chain at every metric form
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', R.chain_cases(), ids=R.case_id)
def test_log_norm_grad_against_reference(case):
    D, cap, L, N, l = case
    cores = R.build_chain(case)
    ctx = new_ctx(cores, l, D, L)
    before = bits(ctx)
    for name, metric in R.metrics_of(case):
        G, out = check_against_reference(ctx, cores, l, D, metric, name)
        G2, out2 = ctx.log_norm_grad(metric)                       # the same call twice: bit-equal
        assert out2 == out and all(a.tobytes() == b.tobytes() for a, b in zip(G, G2)), name
    assert bits(ctx) == before                                     # nothing on the device changed
    ctx.close()


@pytest.mark.parametrize('case', R.chain_cases(), ids=R.case_id)
def test_network_log_norm_gradient_uniform_metric(case):
    """the fifth metric, 'uniform' (data_generator.psi_gram), on every shared chain through Network.log_norm_gradient, and no
    metric through the same method: the bounds of check_against_reference, the canonical shapes, the identity"""
    import tensornetworkforml_amd as pkg
    D, cap, L, N, l = case
    cores = R.build_chain(case)
    net = pkg.Network_class.Network(N, context_M(D, cap, L), D=D, L=L, trunc='fixed')
    net._host_cores = A.as64(cores)
    net._l_pos = l
    net._host_newer = True
    S = pkg.data_generator.psi_gram(D)
    for metric, ref_metric in (('uniform', S), (None, None)):
        G, (sign, logz) = net.log_norm_gradient(metric)
        Gr, (sr, lr) = R.log_norm_gradient(cores, l, ref_metric)
        assert sign == sr and abs(logz - lr) <= log_tol(cores, D)
        own = net.inner(None, metric)[0]
        assert own[0] == sign and abs(own[1] - logz) <= log_tol(cores, D)
        for i, (g, gr) in enumerate(zip(G, Gr)):
            assert g.dtype == np.float32 and g.shape == cores[i].shape
            assert float(np.abs(g - gr).max()) <= G_TOL * float(np.abs(gr).max()), i
            prod = g.astype(np.float64) * cores[i]
            assert abs(float(prod.sum()) - 2.0) <= G_TOL * float(np.abs(prod).sum()), i


# ---------------------------------------------------------------------------------------------------------------
# 2. long un-calibrated chains: the exponent bookkeeping
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('L', [2, 10])
@pytest.mark.parametrize('l', [0, 391, 783])
def test_log_norm_grad_long_raw_chain(L, l):
    """N = 784, bond 20, un-calibrated random cores (f about 1e-66): the status is clean, every Gz finite and within the bounds,
    under the Euclidean metric (Z far above the float32 range) and, with every core times 0.6, under the grid's (Z below the
    float64 range)"""
    (N, D, _, _), cores = R.raw_long_chain(L, l)
    ctx = new_ctx(cores, l, D, L)
    _, (sign, logz) = check_against_reference(ctx, cores, l, D, None, 'euclidean')
    assert sign == 1.0 and logz > 100.0
    _, cores = R.raw_long_chain(L, l, 0.6)
    ctx.set_cores(A.as32(cores), l)
    _, phi, w = R.grid(R.K, D)
    _, (sign, logz) = check_against_reference(ctx, cores, l, D, R.gram(phi, w), 'grid')
    assert sign == 1.0 and logz < -745.0
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------
# 3. the sign under an indefinite metric; refusals on the device; what the status word reports
# ---------------------------------------------------------------------------------------------------------------
def test_log_norm_grad_indefinite_metric():
    case = (2, 5, 3, 3, 1)
    cores = R.build_chain(case)
    metric = np.stack([A.spd_metric(np.random.default_rng(4), 2), -A.spd_metric(np.random.default_rng(3), 2),
                       A.spd_metric(np.random.default_rng(5), 2)])
    ctx = new_ctx(cores, 1, 2, 3)
    _, (sign, _) = check_against_reference(ctx, cores, 1, 2, metric, 'indefinite')
    assert sign == -1.0
    ctx.close()


def test_log_norm_grad_refusals_and_status():
    D, L, N, l = 2, 2, 4, 1
    rng = np.random.default_rng(7)
    shapes = R.shapes_of(N, D, L, [2, 65, 2], l)
    ctx = _hip.Context(N, D, L, 65, 64)
    ctx.set_any_position(True)
    assert _code(lambda: ctx.log_norm_grad()) == STATE             # cores never set
    ctx.set_cores([rng.random(s).astype(np.float32) for s in shapes], l)
    assert _code(lambda: ctx.log_norm_grad()) == ARG               # bond 65
    assert 'bond 65' in str(_hip.lib().tnml_last_error())
    cores = [rng.random(s).astype(np.float32) for s in R.shapes_of(N, D, L, [2, 64, 2], l)]
    ctx.set_cores(cores, l)
    ctx.log_norm_grad()                                            # bond 64 is taken
    assert _code(lambda: ctx.log_norm_grad(np.array([[1.0, 0.5], [0.25, 1.0]]))) == ARG
    assert _code(lambda: ctx.log_norm_grad(np.array([[1.0, np.nan], [np.nan, 1.0]]))) == ARG
    assert _code(lambda: ctx.log_norm_grad(np.eye(3))) == ARG
    bad = [c.copy() for c in cores]
    bad[2][1, 0, 1] = np.inf
    ctx.set_cores(bad, l)
    assert _code(lambda: ctx.log_norm_grad()) == NONFINITE
    bad[2][1, 0, 1] = np.nan
    ctx.set_cores(bad, l)
    assert _code(lambda: ctx.log_norm_grad()) == NONFINITE
    zero = [c.copy() for c in cores]
    zero[3][:] = 0.0
    ctx.set_cores(zero, l)
    assert _code(lambda: ctx.log_norm_grad()) == NONFINITE         # <W|W> == 0
    assert 'zero' in str(_hip.lib().tnml_last_error())
    ctx.set_cores(cores, l)
    G, _ = ctx.log_norm_grad()                                     # usable afterwards
    assert all(np.isfinite(g).all() for g in G)
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------
# 4. layer 2: the negative log-likelihood of a batch and its gradient, against the float64 reference
#    bounds: ten times the float32 emulation's worst figure of the row (nll_reference.EMULATION), rounded up to one digit
# ---------------------------------------------------------------------------------------------------------------
def network_of(cores, l, D, L):
    import tensornetworkforml_amd as pkg
    cap = max(c.shape[2] for c in cores)
    net = pkg.Network_class.Network(len(cores), context_M(D, cap, L), D=D, L=L, trunc='fixed')
    net._host_cores = A.as64(cores)
    net._l_pos = l
    net._host_newer = True
    return net


def check_likelihood(ctx, cores, l, X, lab, S, row, what):
    """both objectives against the float64 reference -> {objective: (G, out3)}; the figures are printed before they are asserted"""
    res = {}
    for name, y in (('joint', lab), ('marginal', None)):
        G, out = ctx.nll_grad(X, y, S)
        Gr, vr, lzr = R.nll_gradient(cores, l, X, y, S)
        gb, vb = R.gpu_bounds(row, name)
        gerr = R.deviation([g.astype(np.float64) for g in G], Gr)
        verr = abs(out[0] - vr) / max(1.0, abs(vr))
        print('%s %s: G %.2e (bound %.0e)  value %.2e (bound %.0e)' % (what, name, gerr, gb, verr, vb))
        assert out[2] == 0 and abs(out[1] - lzr) <= log_tol(cores, cores[0].shape[1])
        assert gerr <= gb and verr <= vb, (what, name, gerr, gb, verr, vb)
        ev = ctx.nll_eval(X, y, S)
        assert ev[0] == out[0] and ev[1] == out[1] and ev[2] == 0                     # the value alone: the same sums
        res[name] = (G, out)
    return res


@pytest.mark.parametrize('lc', R.likelihood_cases(), ids=R.likelihood_id)
def test_nll_gradient_against_reference(lc):
    case, b = lc
    D, cap, L, N, l = case
    cores, l, lev, lab, X, S = R.build_likelihood_case(lc)
    ctx = new_ctx(cores, l, D, L)
    before = bits(ctx)
    check_likelihood(ctx, cores, l, X, lab, S, case[:3], R.likelihood_id(lc))
    assert bits(ctx) == before
    ctx.close()


def test_nll_gradient_long_calibrated_chain():
    """N = 784, bond 10, L = 2, b = 64, images drawn from the chain itself: the same rule for the bound, with its own emulation row"""
    D, cap, L, N, l = R.LONG_CASE
    cores, l, lev, lab, X, S = R.build_long_case()
    ctx = new_ctx(cores, l, D, L)
    check_likelihood(ctx, cores, l, X, lab, S, 'long', 'long')
    ctx.close()


@pytest.mark.parametrize('lc', R.likelihood_cases(), ids=R.likelihood_id)
def test_nll_value_against_log_prob(lc):
    """Network.nll_gradient's value (the sum log w term included) against -mean(log_prob(X, y, joint=True)) of the device's float64
    sampler on every shared case, within the row's value bound; Network.nll gives the same value without a gradient launch"""
    D, cap, L, N, l = lc[0]
    row = lc[0][:3]
    cores, l, lev, lab, X, S = R.build_likelihood_case(lc)
    net = network_of(cores, l, D, L)
    G, value = net.nll_gradient(lev, lab, levels=R.K)
    ref = -float(np.mean(net.log_prob(lev, lab, levels=R.K, joint=True)[0]))
    err = abs(value - ref) / max(1.0, abs(ref))
    print('%s: nll %.6f against log_prob %.6f, %.2e (bound %.0e)' % (R.likelihood_id(lc), value, ref, err, R.gpu_bounds(row, 'joint')[1]))
    assert err <= R.gpu_bounds(row, 'joint')[1]
    assert net.nll(lev, lab, levels=R.K) == value
    Gm, vm = net.nll_gradient(lev, None, levels=R.K)
    assert vm <= value and net.nll(lev, levels=R.K) == vm         # p(x) >= p(x, y)
    assert all(g.shape == c.shape for g, c in zip(G, cores))


@pytest.mark.parametrize('row', R.ROWS, ids=lambda r: 'D%d_M%d_L%d' % tuple(r))
def test_nll_gradient_identity(row):
    """sum(G_i A_i) = 0 per site on the device's output, both objectives, every case of the row, Gd from the float64 reference.
    Per site against the site's own sum|Gd_i A_i|, 2^-22 = 2.4e-7 is out of float32's reach: the float32 emulation of
    tests/nll_reference.py leaves 2.3e-7 to 7.2e-7 per row (IDENTITY_EMULATION, asserted by the host test), an MI355X 2.4e-7 to
    5.2e-7 -- Gd carries the rounding of two float32 chains of up to N sites and of a sum over the batch, not one rounding of its
    output.  Asserted: the per-site residual within ten times the emulation's figure of the row, rounded up to one digit, and each
    site's residual within 2^-22 of sum|Gd_i A_i| summed over every site."""
    worst_site, worst_all = 0.0, 0.0
    for lc in [c for c in R.likelihood_cases() if c[0][:3] == tuple(row)]:
        D, cap, L, N, l = lc[0]
        cores, l, lev, lab, X, S = R.build_likelihood_case(lc)
        ctx = new_ctx(cores, l, D, L)
        for y in (lab, None):
            G, _ = ctx.nll_grad(X, y, S)
            site, every = R.identity_residuals(cores, l, X, y, G)
            worst_site, worst_all = max(worst_site, site), max(worst_all, every)
        ctx.close()
    print('row %s: worst |sum(G_i A_i)| / sum|Gd_i A_i| of the site = %.2e (bound %.0e); over the sum of every site %.2e (bound %.2e)'
          % (tuple(row), worst_site, R.identity_bound(row), worst_all, G_TOL))
    assert worst_site <= R.identity_bound(row), (row, worst_site)
    assert worst_all <= G_TOL, (row, worst_all)


# ---------------------------------------------------------------------------------------------------------------
# 5. bit-equality: chunks, repetition, the index form
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('b', [70, 200])
def test_nll_gradient_bit_equality(b):
    case = (2, 33, 2, 17, 8)
    D, cap, L, N, l = case
    cores = R.build_chain(case)
    lev, lab, X = R.draw_batch(case, cores, b, 1)
    _, phi, w = R.grid(R.K, D)
    S = R.gram(phi, w)
    ctx = new_ctx(cores, l, D, L)
    ctx.dataset_attach(X, lab)
    idx = np.arange(b, dtype=np.int32)
    for y, labels in ((lab, True), (None, False)):
        G0, o0 = ctx.nll_grad(X, y, S)
        G1, o1 = ctx.nll_grad(X, y, S)                             # the same call twice
        Gi, oi = ctx.nll_grad_indices(idx, labels, S)              # the index form
        ei = ctx.nll_eval_indices(idx, labels, S)
        ctx.set_core_grad_chunk(64)
        Gc, oc = ctx.nll_grad(X, y, S)                             # chunks of 64 against the default chunk
        ctx.set_core_grad_chunk(0)
        for G, o in ((G1, o1), (Gi, oi), (Gc, oc)):
            assert o.tobytes() == o0.tobytes() and all(a.tobytes() == c.tobytes() for a, c in zip(G, G0))
        assert ei.tobytes() == o0.tobytes()
    ctx.close()


def test_nll_refusals_and_bad_samples():
    case = (2, 5, 3, 3, 1)
    D, cap, L, N, l = case
    cores = R.build_chain(case)
    lev, lab, X = R.draw_batch(case, cores, 17)
    ctx = new_ctx(cores, l, D, L)
    assert _code(lambda: ctx.nll_grad(X, np.full(17, L))) == ARG                    # a label outside [0, L)
    assert _code(lambda: ctx.nll_grad(X, lab, np.array([[1.0, 0.5], [0.25, 1.0]]))) == ARG
    assert _code(lambda: ctx.nll_grad_indices(np.arange(3))) == STATE               # no dataset
    zero = [c.copy() for c in cores]
    zero[l][..., 1] = 0.0                                                           # f_1 == 0 for every sample
    ctx.set_cores(A.as32(zero), l)
    y1 = np.ones(17, dtype=np.int32)
    assert _code(lambda: ctx.nll_grad(X, y1)) == NONFINITE
    assert '17 of 17 samples' in str(_hip.lib().tnml_last_error())
    G, out = ctx.nll_grad(X, None)                                                  # the marginal does not see the empty slice
    assert out[2] == 0 and all(np.isfinite(g).all() for g in G)
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------
# 6. range-safe chains, and what an un-calibrated network gets
# ---------------------------------------------------------------------------------------------------------------
def test_nll_gradient_with_chain_scaling():
    """with tnml_set_chain_scaling on the data term takes the scaled kernels, as gradient_step does: the same bounds hold, and a
    chain whose cores alternate between 2^40 and 2^-40 times the calibrated ones (f unchanged, every partial product of the plain
    kernels beyond float32) is within them too"""
    lc = next(c for c in R.likelihood_cases() if c[0] == (2, 33, 2, 17, 8))
    D, cap, L, N, l = lc[0]
    cores, l, lev, lab, X, S = R.build_likelihood_case(lc)
    ctx = new_ctx(cores, l, D, L)
    ctx.set_chain_scaling(True)
    check_likelihood(ctx, cores, l, X, lab, S, lc[0][:3], 'scaled')
    wild = [c * (2.0 ** 40 if i % 2 == 0 else 2.0 ** -40) for i, c in enumerate(cores[:16])] + [cores[16]]
    ctx.set_cores(A.as32(wild), l)
    for name, y in (('joint', lab), ('marginal', None)):
        G, out = ctx.nll_grad(X, y, S)
        Gr, vr, _ = R.nll_gradient(wild, l, X, y, S)
        gb, vb = R.gpu_bounds(lc[0][:3], name)
        errs = [float(np.abs(g - gr).max()) / float(np.abs(gr).max()) for g, gr in zip(G, Gr)]      # per core: their scales differ by 2^80
        print('scaled, alternating cores, %s: G %.2e (bound %.0e) value %.2e' % (name, max(errs), gb, abs(out[0] - vr) / max(1.0, abs(vr))))
        assert out[2] == 0 and abs(out[0] - vr) <= vb * max(1.0, abs(vr)) and max(errs) <= gb
    ctx.close()


def test_uncalibrated_network_gets_the_norm_term_and_a_count():
    """N = 784, un-calibrated and every core times 0.6 (f far below float32: it is stored as 0): layer 1 returns Gz, layer 2
    TNML_ERR_NONFINITE naming the count of samples"""
    (N, D, L, l), cores = R.raw_long_chain(2, 0, 0.6)
    ctx = new_ctx(cores, l, D, L)
    _, phi, w = R.grid(R.K, D)
    S = R.gram(phi, w)
    G, (sign, logz) = ctx.log_norm_grad(S)
    assert sign == 1.0 and all(np.isfinite(g).all() for g in G)
    rng = np.random.default_rng(5)
    X = phi[rng.integers(0, R.K, (8, N))].astype(np.float32)
    assert _code(lambda: ctx.nll_grad(X, np.zeros(8, dtype=np.int32), S)) == NONFINITE
    assert '8 of 8 samples' in str(_hip.lib().tnml_last_error())
    ctx.close()
