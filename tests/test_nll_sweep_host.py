"""The two-site likelihood sweep without a device: the statement of tests/nll_sweep_reference.py against
nll_reference.py, finite differences and the dense table, and the conditions the cases of tests/test_nll_sweep_gpu.py rest on.

  1  the two-site gradient contracted with either core is nll_gradient's core gradient
  2  central finite differences of the value in B
  3  <G, B> = 0
  4  log Z of the step against the dense enumeration at N = 4
  5  the conditions of the GPU cases: the ratio, the descent in float64 and in the emulation, the lr = 0 identity, the tables
  6  the refusals that need no device, the Python layer
"""
import ctypes as C
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

import nll_reference as NR                                         # noqa: E402
import nll_sweep_reference as R                                    # noqa: E402
import sample_reference as sref                                    # noqa: E402


@pytest.fixture(scope='module')
def built():
    return {R.case_id(c): R.build_case(c) for c in R.CASES}


@pytest.fixture(scope='module')
def passes(built):
    out = {}
    for c in R.CASES:
        cores, l, X, lab, y, S = built[R.case_id(c)]
        out[R.case_id(c)] = (R.there_and_back(cores, l, X, y, S, R.LR, c[5], R.MAX_BOND),
                             R.there_and_back(cores, l, X, y, S, R.LR, c[5], R.MAX_BOND, emulate=True))
    return out


def rel(a, ref):
    return float(np.abs(a - ref).max() / np.abs(ref).max())


# ---------------------------------------------------------------------------------------------------------------
# 1 - 3  the gradient
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', R.CASES, ids=R.case_id)
@pytest.mark.parametrize('left', [False, True], ids=['right', 'left'])
def test_two_site_gradient_is_the_core_gradient_contracted(case, left, built):
    cores, l, X, lab, y, S = built[R.case_id(case)]
    N = case[0]
    if (left and l == 0) or (not left and l == N - 1):
        left = not left
    g = R.step_gradient(cores, l, X, y, S, left)
    G2 = g['Gd'] - g['Gz']
    G, value, logz = NR.nll_gradient(cores, l, X.astype(np.float64), y, S)
    p = g['p']
    if left:        # the label is on p + 1
        Gp = np.einsum('adecl,kecl->adk', G2, cores[p + 1])
        Gq = np.einsum('adecl,adk->kecl', G2, cores[p])
    else:
        Gp = np.einsum('adecl,kec->adkl', G2, cores[p + 1])
        Gq = np.einsum('adecl,adkl->kec', G2, cores[p])
    assert rel(Gp, G[p]) <= 1e-12 and rel(Gq, G[p + 1]) <= 1e-12
    assert abs(g['value'] - value) <= 1e-12 * max(1.0, abs(value)) and abs(g['logz'] - logz) <= 1e-12 * max(1.0, abs(logz))
    # 3: the likelihood does not see the scale of B
    assert abs(float((G2 * g['B']).sum())) <= 1e-12 * float(np.abs(g['Gd'] * g['B']).sum())


def _value_of(B, cores, l, X, y, S, left):
    """the value of the batch with the merged tensor replaced by B"""
    p = l - 1 if left else l
    Xd = X.astype(np.float64)
    P, Q = R.chains(cores, p, Xd, np.float64)
    f = np.einsum('sa,sd,se,sc,adecl->ls', P, Xd[:, p], Xd[:, p + 1], Q, B)
    _, terms = NR.cotangent(f, y)
    Ls, lgL, Rs, lgR = NR.environments(cores, l, S)
    T = np.einsum('ab,dD,eE,bDECl,Cc->adecl', Ls[p], S, S, B, Rs[p + 2], optimize=True)
    return float(-(terms.mean() - (math.log(abs(float((B * T).sum()))) + lgL[p] + lgR[p + 2])))


@pytest.mark.parametrize('case', [R.CASES[0], R.CASES[2], R.CASES[6]], ids=R.case_id)
def test_central_differences_of_the_value_in_B(case, built):
    cores, l, X, lab, y, S = built[R.case_id(case)]
    left = R.plan(case[0], l)[0][0]
    g = R.step_gradient(cores, l, X, y, S, left)
    G2, B = g['Gd'] - g['Gz'], g['B']
    assert abs(_value_of(B, cores, l, X, y, S, left) - g['value']) <= 1e-12
    rng = np.random.default_rng(3)
    h = 1e-6 * np.abs(B).max()
    for _ in range(12):
        idx = tuple(int(rng.integers(0, n)) for n in B.shape)
        Bp, Bm = B.copy(), B.copy()
        Bp[idx] += h
        Bm[idx] -= h
        fd = (_value_of(Bp, cores, l, X, y, S, left) - _value_of(Bm, cores, l, X, y, S, left)) / (2 * h)
        assert abs(-fd - G2[idx]) <= 1e-6 * np.abs(G2).max(), (idx, fd, G2[idx])       # G descends: -d value / d B


def test_log_z_against_the_dense_table():
    """N = 4: Z by enumeration of every image and label, at both label positions a step can start from"""
    N, K, D, L, l = 4, 3, 2, 2, 1
    cores, phi, w = sref.dense_case(D, L, N, K, l)
    S = sref.gram(phi, w)
    T = NR.A.dense(cores, l)
    wt = np.ones(())
    for i in range(N):
        T = np.moveaxis(np.tensordot(phi, T, (1, i)), 0, i)
        wt = np.multiply.outer(wt, w)
    logz = math.log(float((T ** 2 * wt[..., None]).sum()))
    X = phi[np.zeros((3, N), dtype=int)]
    for left in (False, True):
        g = R.step_gradient(cores, l, X, None, S, left)
        assert abs(g['logz'] - logz) <= 1e-12 * max(1.0, abs(logz))


# ---------------------------------------------------------------------------------------------------------------
# 5  the conditions the GPU cases rest on
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', R.CASES, ids=R.case_id)
def test_ratio(case, built):
    cores, l, X, lab, y, S = built[R.case_id(case)]
    assert R.label_ratio(cores, l, X, y) >= R.MIN_RATIO


@pytest.mark.parametrize('case', R.DESCENT, ids=R.case_id)
def test_every_step_lowers_the_value(case, passes):
    (c64, l64, v64), (c32, l32, v32) = passes[R.case_id(case)]
    assert len(R.DESCENT) >= 4
    assert (np.diff(v64[:, 0]) < 0).all() and (np.diff(v32[:, 0]) < 0).all()
    assert (v64[:, 5] <= 1e-9).all()                   # MAX_BOND holds the rank: what a split of a descent case drops is an update's trace


@pytest.mark.parametrize('case', R.CASES, ids=R.case_id)
def test_the_pass_lowers_the_batch_value(case, built, passes):
    cores, l, X, lab, y, S = built[R.case_id(case)]
    (c64, l64, v64), _ = passes[R.case_id(case)]
    assert NR.nll_value(c64, l64, X, y, S) < v64[0, 0]
    assert l64 == (case[0] - 1 if case[2] == case[0] - 1 else 0)


@pytest.mark.parametrize('case', R.LR0, ids=R.case_id)
def test_lr_zero_identity(case, built):
    cores, l, X, lab, y, S = built[R.case_id(case)]
    c0, l0, v0 = R.there_and_back(cores, l, X, y, S, 0.0, case[5], R.MAX_BOND)
    assert (v0[:, 5] == 0).all()
    f0, f1 = NR.forward(cores, l, X.astype(np.float64)), NR.forward(c0, l0, X.astype(np.float64))
    assert rel(f1, f0) <= 1e-13 if l0 == l else True
    # (the label may end on another site than it started from: compare the values, which do not depend on it)
    assert abs(NR.nll_value(c0, l0, X, y, S) - v0[0, 0]) <= 1e-13 * max(1.0, abs(v0[0, 0]))


def test_truncation_at_the_existing_bond_can_raise_the_value(built):
    """what the docstrings warn of: with max_bond = 4, the bond the chain has, a pass at lr = 0 changes the function"""
    worst = 0.0
    for case in R.CASES:
        cores, l, X, lab, y, S = built[R.case_id(case)]
        c0, l0, v0 = R.there_and_back(cores, l, X, y, S, 0.0, case[5], R.CAP)
        worst = max(worst, NR.nll_value(c0, l0, X, y, S) - v0[0, 0])
    assert worst > 1e-3


def test_emulation_table_is_what_the_code_gives(passes, built):
    worst = dict.fromkeys(R.EMULATION, 0.0)
    for case in R.CASES:
        figs = R.emulation_figures(case) + R.single_step_figures(case)
        for k, v in zip(('value', 'logz', 'f', 'discarded', 'Gd', None, 'B_new'), figs):
            if k:
                worst[k] = max(worst[k], v)
    for k, v in worst.items():
        assert 0.25 * R.EMULATION[k] <= v <= 1.25 * R.EMULATION[k], (k, v)
        assert 10 * R.EMULATION[k] <= R.gpu_bound(k) < 20 * R.EMULATION[k]


def test_adaptive_rank_rule():
    S = np.array([4.0, 2.0, 1.0, 0.5, 0.25])
    assert R.kept_rank(S, 5, 1.0) == 5 and R.kept_rank(S, 3, 1.0) == 3
    assert R.kept_rank(S, 5, 0.9) == 3 and R.kept_rank(S, 5, 0.95) == 4 and R.kept_rank(S, 5, 0.5) == 1 and R.kept_rank(S, 2, 0.9) == 2
    assert R.discarded_weight(S, 5) == 0.0 and R.discarded_weight(S, 4) == pytest.approx(0.0625 / (S ** 2).sum())


# ---------------------------------------------------------------------------------------------------------------
# 6  no device
# ---------------------------------------------------------------------------------------------------------------
def test_refusals_without_a_device():
    from tensornetworkforml_amd import _hip
    lib = _hip.lib()
    vals = np.zeros(6)
    X = np.zeros((1, 2, 2), dtype=np.float32)
    n = C.c_size_t()
    assert lib.tnml_nll_sweep(None, _hip._ptr(X, C.c_float), None, 1, None, 0, 1, 0.01, 1, 4, 1.0, _hip._ptr(vals, C.c_double)) == -1
    idx = np.zeros(1, dtype=np.int32)
    assert lib.tnml_nll_sweep_indices(None, _hip._ptr(idx, C.c_int32), 1, 1, None, 0, 1, 0.01, 1, 4, 1.0, _hip._ptr(vals, C.c_double)) == -1
    assert lib.tnml_nll_sweep_debug(None, 0, _hip._ptr(vals, C.c_double), 6, C.byref(n)) == -1
    assert b'NULL' in lib.tnml_last_error()


def test_nll_sweep_host_side_under_sanitizers():
    """csrc/Makefile target `san-nll-sweep`: nll_sweep_host.hip and the launch wrappers it reaches, built --cuda-host-only with
    -fsanitize=address,undefined, against the stand-in runtime of csrc/san/hip_stub.cpp (csrc/san/plan_nll_sweep_main.cpp, a
    stand-alone program): whole passes at the shapes of the GPU tests, the large-tensor step, N = 784 at bond 20 and 50, every refusal
    (none launches), the state rules, every allocation of a call failing in turn with the label at every site."""
    import shutil
    import subprocess
    if shutil.which('g++') is None or not os.path.exists('/opt/rocm/bin/hipcc'):
        pytest.skip('no g++ / hipcc')
    csrc = os.path.join(ROOT, 'tensornetworkforml_amd', 'csrc')
    out = subprocess.run(['make', '-C', csrc, '-j4', 'san-nll-sweep'], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert 'likelihood sweep host planning under ASan + UBSan: ok' in out.stdout
    for name in ('at the test shapes', 'on the large-tensor path', 'c3: N 784, bond 20', 'c5: N 784, bond 50', 'likelihood sweep refusals: ok',
                 'state rules of the likelihood sweep: ok', 'tnml_nll_sweep, fresh, label on 4', 'a larger batch'):
        assert name in out.stdout, name
    assert '0 live allocations' in out.stdout
    assert 'ERROR' not in out.stderr and 'runtime error' not in out.stderr


def test_python_layer_without_a_device():
    from tensornetworkforml_amd import _hip
    import tensornetworkforml_amd as pkg
    for s_, n_ in (('tnml_nll_sweep', 12), ('tnml_nll_sweep_indices', 12), ('tnml_nll_sweep_debug', 5)):
        assert s_ in _hip.SYMBOLS and len(getattr(_hip.lib(), s_).argtypes) == n_
    for m in ('nll_sweep', 'nll_sweep_indices', 'nll_sweep_debug', 'bonds'):
        assert callable(getattr(_hip.Context, m))
    Network = pkg.Network_class.Network
    assert callable(Network.nll_sweep)
    import inspect
    sig = inspect.signature(Network.train_generative)
    assert sig.parameters['method'].default == 'gradient' and sig.parameters['threshold'].default == 1.0
    assert 'rise' in Network.nll_sweep.__doc__.lower() and 'full rank' in Network.nll_sweep.__doc__
    from tensornetworkforml_amd import training_diagonals, training_binary_MNIST
    for script in (training_diagonals, training_binary_MNIST):
        with pytest.raises(SystemExit):
            script.main(['--resident', '--method', 'sweep'])                      # needs --objective nll
        with pytest.raises(SystemExit):
            script.main(['--resident', '--objective', 'nll', '--max-bond', '8'])  # needs --method sweep
