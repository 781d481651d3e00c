"""The reference of tests/nll_reference.py checked on the CPU: against central differences of the log-norm of
tests/mps_algebra_reference.py, against the dense table of tests/sample_reference.py, on the two identities, and on the conditions
the shared cases must meet; the host side of tnml_log_norm_grad under sanitizers; the argument checks of the Python layer.
"""
import math
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
import sample_reference as sref                                    # noqa: E402

H = 1e-6
FD_TOL = 1e-7                                    # of max|G|; the differences reach about 1e-9
IDENTITY_TOL = 1e-12
FD_CASES = [c for c in R.chain_cases() if c[:3] in ((2, 5, 3), (3, 7, 3), (8, 16, 17))]


def _fd(fn, cores, i, idx, h=H):
    """central difference of fn(cores) in element idx of core i"""
    up = [c.copy() for c in cores]
    dn = [c.copy() for c in cores]
    up[i][idx] += h
    dn[i][idx] -= h
    return (fn(up) - fn(dn)) / (2 * h)


@pytest.mark.parametrize('case', FD_CASES, ids=R.case_id)
def test_log_norm_gradient_against_central_differences(case):
    """d log<W|W>_S / d A against (log<W + h e|W + h e> - log<W - h e|W - h e>) / 2h of mps_algebra_reference.inner, three random
    elements per site, at every metric form"""
    D, cap, L, N, l = case
    cores = R.build_chain(case)
    rng = np.random.default_rng([1, D, cap, L, N, l])
    for name, metric in R.metrics_of(case):
        G, (sign, logz) = R.log_norm_gradient(cores, l, metric)
        s_ref, l_ref = A.inner(cores, cores, l, metric)
        assert sign == s_ref == 1.0 and abs(logz - l_ref) < 1e-12 * max(1.0, abs(l_ref)), (name, logz, l_ref)
        gmax = max(np.abs(g).max() for g in G)
        for i in range(N):
            for _ in range(3):
                idx = tuple(int(rng.integers(0, n)) for n in cores[i].shape)
                fd = _fd(lambda cs: A.inner(cs, cs, l, metric)[1], cores, i, idx)
                assert abs(fd - G[i][idx]) <= FD_TOL * gmax, (name, i, idx, fd, G[i][idx], gmax)


def test_log_norm_gradient_with_an_indefinite_metric():
    """the sign of <W|W>_S is reported and the gradient is that of log|<W|W>_S|"""
    case = (2, 5, 3, 3, 1)
    cores = R.build_chain(case)
    metric = -A.spd_metric(np.random.default_rng(3), 2)            # one site of three with a negative definite metric: Z < 0
    metric = np.stack([A.spd_metric(np.random.default_rng(4), 2), metric, A.spd_metric(np.random.default_rng(5), 2)])
    G, (sign, logz) = R.log_norm_gradient(cores, 1, metric)
    assert sign == -1.0 and (sign, logz) == pytest.approx(A.inner(cores, cores, 1, metric), abs=1e-12)
    gmax = max(np.abs(g).max() for g in G)
    for i in range(3):
        idx = (0,) * cores[i].ndim
        fd = _fd(lambda cs: A.inner(cs, cs, 1, metric)[1], cores, i, idx)
        assert abs(fd - G[i][idx]) <= FD_TOL * gmax


@pytest.mark.parametrize('case', R.chain_cases(), ids=R.case_id)
def test_log_norm_identity(case):
    """sum(Gz_i A_i) = 2 at every site: <W|W> is of degree two in every core"""
    D, cap, L, N, l = case
    cores = R.build_chain(case)
    assert max(c.shape[2] for c in cores) == cap and (N == 2 or min(c.shape[2] for c in cores[:-1]) == 1)
    for name, metric in R.metrics_of(case):
        G, _ = R.log_norm_gradient(cores, l, metric)
        for i in range(N):
            assert abs(float((G[i] * cores[i]).sum()) - 2.0) <= IDENTITY_TOL, (name, i)


def test_log_norm_gradient_of_the_raw_long_chain_is_a_float32():
    """N = 784, bond 20, un-calibrated and every core times 0.6: Z is below float64 itself under the grid's metric (and the
    unscaled chain's far above float32 under the Euclidean one, which sums 2^784 terms); every Gz element is of order 1 / |A_i|"""
    (N, D, L, l), cores = R.raw_long_chain(2, 391)
    _, phi, w = R.grid(R.K, D)
    assert R.log_norm(cores, l)[1] > 100.0
    (N, D, L, l), cores = R.raw_long_chain(2, 391, 0.6)
    G, (sign, logz) = R.log_norm_gradient(cores, l, R.gram(phi, w))
    assert sign == 1.0 and logz < -745.0
    gmax = max(np.abs(g).max() for g in G)
    assert np.isfinite(np.float32(gmax)) and 1e-3 < gmax < 1e3
    for i in (0, 1, 390, 391, 392, 783):
        assert abs(float((G[i] * cores[i]).sum()) - 2.0) <= 1e-10


def test_log_norm_grad_host_side_under_sanitizers():
    """csrc/Makefile target `san-nll`: tnml_log_norm_grad of tnml_api.hip and the launch wrappers of kernels_nll.hip, built
    --cuda-host-only with -fsanitize=address,undefined, against the stand-in runtime of csrc/san/hip_stub.cpp
    (csrc/san/plan_nll_main.cpp, a stand-alone program): C3 and C5 at true size with the label at both ends and inside, a ragged
    17-site chain at every label position at D = 2, 3 and 8, N = 2, the three metric forms, both objectives of the likelihood in X
    and index form with the default chunk and chunks of 64, gradient and value alone, bond 64 taken and 65 refused, every refusal
    (none launches), the state rule, and every allocation of the new groups failing in turn, fresh and at growth."""
    import shutil
    import subprocess
    if shutil.which('g++') is None or not os.path.exists('/opt/rocm/bin/hipcc'):
        pytest.skip('no g++ / hipcc')
    csrc = os.path.join(ROOT, 'tensornetworkforml_amd', 'csrc')
    out = subprocess.run(['make', '-C', csrc, '-j4', 'san-nll'], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert 'log-norm gradient host planning under ASan + UBSan: ok' in out.stdout
    for name in ('c3 bond 20 L 2, label on 0', 'c3 last bond 20', 'c3 inner label', 'c5 bond 50 L 10', 'c5 first', 'c5 inner label',
                 'ragged N 17 D 2', 'ragged N 17 D 3', 'ragged N 17 D 8', 'ragged N 2 D 2', 'log-norm gradient refusals: ok',
                 'state rule of the log-norm gradient: ok', '0 live allocations'):
        assert name in out.stdout, name
    assert out.stdout.count(' 9 failed in turn') >= 4              # the log-norm group has nine members: fresh and at growth, D = 2 and 3
    for name in ('tnml_nll_grad, fresh context', 'tnml_nll_eval, more samples', 'tnml_nll_grad, the groups exist'):
        assert out.stdout.count(name) == 2, name
    assert 'nll_cot_kernel' in out.stdout and 'nll_sum_kernel' in out.stdout


def test_python_layer_without_a_device():
    """the symbol is declared, and Network.log_norm_gradient refuses a bad metric before it touches the device"""
    from tensornetworkforml_amd import _hip
    import tensornetworkforml_amd as pkg
    assert 'tnml_log_norm_grad' in _hip.SYMBOLS and hasattr(_hip.lib(), 'tnml_log_norm_grad')
    assert len(_hip.lib().tnml_log_norm_grad.argtypes) == 6
    assert callable(_hip.Context.log_norm_grad)
    Network = pkg.Network_class.Network
    assert callable(Network.log_norm_gradient)
    net = Network.__new__(Network)                                 # the checks read N and D alone
    net.N, net.D = 5, 2
    assert net._checked_metric(None) is None
    assert net._checked_metric('uniform').shape == (2, 2)
    assert net._checked_metric(np.eye(2)).dtype == np.float64 and net._checked_metric(np.ones((5, 2, 2))).shape == (5, 2, 2)
    for bad in ('euclid', np.eye(3), np.ones((4, 2, 2)), np.array([[1.0, 0.5], [0.25, 1.0]]), np.array([[1.0, math.nan], [math.nan, 1.0]]),
                np.array([[math.inf, 0.0], [0.0, 1.0]])):
        with pytest.raises(ValueError):
            net._checked_metric(bad)


# ---------------------------------------------------------------------------------------------------------------
# layer 2: the negative log-likelihood of a batch and its gradient
# ---------------------------------------------------------------------------------------------------------------
def _dense_nll(cores, l, phi, w, lev, lab):
    """-mean log p(x, y), or -mean log p(x) with lab None, read off the dense table"""
    P = sref.dense_joint(cores, l, phi, w)
    rows = tuple(lev[:, i] for i in range(lev.shape[1]))
    p = P[rows + (lab,)] if lab is not None else P[rows].sum(axis=-1)
    return float(-np.log(p).mean())


@pytest.mark.parametrize('shape', [(4, 3, 2, 2, 2), (3, 2, 3, 3, 1)], ids=['N4_K3_D2_L2', 'N3_K2_D3_L3'])
def test_nll_and_gradient_against_the_dense_table(shape):
    """value and central differences of the exact NLL by sample_reference.dense_joint, both objectives"""
    N, K, D, L, l = shape
    cores, phi, w = sref.dense_case(D, L, N, K, l)
    rng = np.random.default_rng([2, N, K, D, L])
    lev = rng.integers(0, K, (9, N)).astype(np.int32)
    lab_all = rng.integers(0, L, 9).astype(np.int32)
    S, X = R.gram(phi, w), phi[lev]
    logw = -float(np.log(w)[lev].sum(axis=1).mean())
    for lab in (lab_all, None):
        G, value, _ = R.nll_gradient(cores, l, X, lab, S)
        exact = _dense_nll(cores, l, phi, w, lev, lab)
        assert abs(value + logw - exact) <= 1e-12 * max(1.0, abs(exact)), (value + logw, exact)
        assert abs(R.nll_value(cores, l, X, lab, S) - value) <= 1e-13
        gmax = max(np.abs(g).max() for g in G)
        for i in range(N):
            for _ in range(3):
                idx = tuple(int(rng.integers(0, n)) for n in cores[i].shape)
                fd = -_fd(lambda cs: _dense_nll(cs, l, phi, w, lev, lab), cores, i, idx)       # G descends
                assert abs(fd - G[i][idx]) <= FD_TOL * gmax, (i, idx, fd, G[i][idx], gmax)


@pytest.mark.parametrize('lc', R.likelihood_cases(), ids=R.likelihood_id)
def test_nll_identity_and_conditioning(lc):
    """sum(G_i A_i) = 0 at every site for both objectives (the likelihood does not see the scale of a core), and the condition the
    shared cases must meet: min_s |f_y| / max|f| >= 1e-3 on images and labels drawn from the case's own chain, no sample dropped"""
    cores, l, lev, lab, X, S = R.build_likelihood_case(lc)
    assert lev.shape == (lc[1], len(cores)) and X.dtype == np.float32
    assert R.label_ratio(cores, l, X, lab) >= R.MIN_RATIO
    for y in (lab, None):
        G, value, logz = R.nll_gradient(cores, l, X, y, S)
        assert np.isfinite(value)
        for i in range(len(cores)):
            assert abs(float((G[i] * cores[i]).sum())) <= IDENTITY_TOL, i


def test_emulation_table_is_what_the_code_gives():
    """the float32 emulation against float64 on every shared case: the worst relative deviation per row and objective is the one
    in nll_reference.EMULATION (within a quarter: the summation order of einsum follows the host's vector width)"""
    worst = {}
    for lc in R.likelihood_cases():
        for name, (g, v) in R.emulation_figures(lc).items():
            w = worst.setdefault((lc[0][:3], name), [0.0, 0.0])
            w[0], w[1] = max(w[0], g), max(w[1], v)
    assert set(worst) == {(tuple(r), o) for r in R.ROWS for o in ('joint', 'marginal')}
    for (row, name), (g, v) in worst.items():
        tg, tv = R.EMULATION[row][name]
        assert abs(g - tg) <= 0.25 * tg and abs(v - tv) <= 0.25 * tv, (row, name, g, tg, v, tv)
        bg, bv = R.gpu_bounds(row, name)
        assert 10 * tg <= bg < 20 * tg and 10 * tv <= bv < 20 * tv
    for name, (g, v) in R.long_emulation_figures().items():        # the long calibrated chain has a row of its own
        tg, tv = R.EMULATION['long'][name]
        assert abs(g - tg) <= 0.25 * tg and abs(v - tv) <= 0.25 * tv, ('long', name, g, tg, v, tv)


def test_identity_emulation_table_is_what_the_code_gives():
    """sum(G_i A_i) = 0 against the one site's own sum|Gd_i A_i|: the float32 emulation's worst residual per row is the one in
    nll_reference.IDENTITY_EMULATION (within a quarter), and it is above 2^-22 on four of the six rows -- the bound the device is held
    to is ten times the emulation's figure, not 2^-22"""
    worst = {}
    for lc in R.likelihood_cases():
        worst[lc[0][:3]] = max(worst.get(lc[0][:3], 0.0), R.identity_emulation_figure(lc))
    assert set(worst) == {tuple(r) for r in R.ROWS}
    for row, v in worst.items():
        t = R.IDENTITY_EMULATION[row]
        assert abs(v - t) <= 0.25 * t, (row, v, t)
        assert 10 * t <= R.identity_bound(row) < 20 * t
    assert sum(v > 2.0 ** -22 for v in R.IDENTITY_EMULATION.values()) >= 4


def test_likelihood_python_layer_without_a_device():
    from tensornetworkforml_amd import _hip
    import tensornetworkforml_amd as pkg
    assert 'tnml_get_bonds' in _hip.SYMBOLS and len(_hip.lib().tnml_get_bonds.argtypes) == 3
    for s_, n_ in (('tnml_nll_grad', 8), ('tnml_nll_grad_indices', 8), ('tnml_nll_eval', 6), ('tnml_nll_eval_indices', 6)):
        assert s_ in _hip.SYMBOLS and len(getattr(_hip.lib(), s_).argtypes) == n_
    Network = pkg.Network_class.Network
    for m in ('nll_gradient', 'nll_gradient_indices', 'nll'):
        assert callable(getattr(Network, m))
    net = Network.__new__(Network)
    net.N, net.D, net.L = 3, 2, 2
    X = np.array([[0.0, 0.5, 1.0], [1.0, 0.0, 0.5]])
    feats, y, S, logw = net._likelihood_batch(X, [1, 0], 3, None, None)
    assert feats.shape == (2, 3, 2) and feats.dtype == np.float32 and y.dtype == np.int32 and S.shape == (2, 2)
    assert logw == pytest.approx(3 * math.log(3.0))
    for bad in (lambda: net._likelihood_batch(X + 0.1, None, 3, None, None),            # off the grid
                lambda: net._likelihood_batch(X[:, :2], None, 3, None, None),           # two sites
                lambda: net._likelihood_batch(X, [0, 2], 3, None, None),                # a label outside [0, L)
                lambda: net._likelihood_batch(X, [0], 3, None, None),                   # one label for two images
                lambda: net._likelihood_batch(np.array([[0, 1, 3]]), None, 3, None, None)):   # a level outside the grid
        with pytest.raises(ValueError):
            bad()
