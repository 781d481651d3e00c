"""Label at an intermediate site (include/tnml.h, tnml_set_any_position) without a GPU: the float64 expectation
the GPU tests use (`label_inside_forward`, plain NumPy on the oracle's `site_matrix`), checked against the oracle itself; the new entry
point in header / library / `_hip.SYMBOLS`; `Network.any_position` and the schedule of `train_resident(steps_per_batch=k)`; the host
side of the new calls under AddressSanitizer + UBSan (csrc/Makefile target `san-anypos`)."""
import os
import pickle
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tensornetworkforml_amd import _hip                    # noqa: E402
from oracle import mps_oracle as mo                        # noqa: E402


# ---------------------------------------------------------------------------------------------------------------
# the expectation: both environment stacks up to the label site, and f from their meeting
# ---------------------------------------------------------------------------------------------------------------
def random_cores_at(N, D, L, bond, l_pos, rng, scale=1.0):
    """U[0,1)/scale cores in the canonical layout (ml, D, mr[, L]) with the label axis on site l_pos."""
    cores = []
    for i in range(N):
        ml = 1 if i == 0 else int(bond[i - 1])
        mr = 1 if i == N - 1 else int(bond[i])
        cores.append(rng.random((ml, D, mr, L) if i == l_pos else (ml, D, mr)) / scale)
    return cores


def label_inside_forward(cores, l, X):
    """(Lenv {i: (b, mr_i)} for i < l, Renv {i: (b, ml_i)} for i > l, f (L, b)) for cores that carry the label on site l, built
    site by site as mo.forward builds them; at l = 0 and l = N-1 the same expressions as mo.forward."""
    N = len(cores)
    Lenv, Renv = {}, {}
    env = None
    for i in range(l):
        T = mo.site_matrix(cores[i], X[:, i])                                   # (b, ml, mr)
        env = T[:, 0] if i == 0 else np.einsum('ba,bac->bc', env, T)
        Lenv[i] = env
    E = env
    env = None
    for i in range(N - 1, l, -1):
        T = mo.site_matrix(cores[i], X[:, i])
        env = T[:, :, 0] if i == N - 1 else np.einsum('bac,bc->ba', T, env)
        Renv[i] = env
    R = env
    T = mo.site_matrix(cores[l], X[:, l])                                       # (b, ml, mr, L)
    if l == 0:
        f = np.einsum('bcl,bc->lb', T[:, 0], R)
    elif l == N - 1:
        f = np.einsum('ba,bal->lb', E, T[:, :, 0])
    else:
        f = np.einsum('ba,bacl,bc->lb', E, T, R)
    return Lenv, Renv, f


def place(st, X, Lenv, Renv):
    """Hand the oracle's sweep_step a batch and both environment stacks."""
    st.X, st.Lenv, st.Renv = X, dict(Lenv), dict(Renv)


KW = dict(lr=1e-2, weight_dec=1e-3, L2_flag=True, act_fn='softmax', loss_fn='full_cross_ent', T=0.1, trunc='fixed')


@pytest.mark.parametrize('N,D', [(7, 2), (8, 2), (10, 2), (7, 3), (8, 3)])
def test_expectation_against_the_oracle(N, D):
    rng = np.random.default_rng(N * 10 + D)
    M, L, b = 4, 3, 9
    X = rng.random((b, N, D))
    y1h = mo.one_hot(rng.integers(0, L, b), L)
    # at the ends: mo.forward exactly
    for l in (0, N - 1):
        cores = random_cores_at(N, D, L, [M] * (N - 1), l, rng, scale=M * 0.5)
        st = mo.MPSState(N, D, L, M, cores, l_pos=l)
        f_o = mo.forward(st, X)
        Lenv, Renv, f = label_inside_forward(st.cores, l, X)
        assert np.array_equal(f, f_o)
        for i, e in (st.Renv if l == 0 else st.Lenv).items():
            assert np.array_equal(e, (Renv if l == 0 else Lenv)[i])
    # after three oracle steps the rebuilt environments are the sweep's own, and sweep_step runs from them in both directions
    st = mo.MPSState(N, D, L, M, random_cores_at(N, D, L, [M] * (N - 1), 0, rng, scale=M * 0.5), l_pos=0)
    f = mo.forward(st, X)
    for _ in range(3):
        f = mo.sweep_step(st, f, y1h, left_dir=False, **KW)
    assert st.l_pos == 3
    Lenv, Renv, f_in = label_inside_forward(st.cores, 3, X)
    for i in range(0, 2):                                   # the sweep has grown Lenv[0], Lenv[1]; Lenv[2] comes with the next step
        assert np.array_equal(Lenv[i], st.Lenv[i]), i
    for i in range(4, N):
        assert np.array_equal(Renv[i], st.Renv[i]), i
    for left in (False, True):
        s2 = st.copy()
        place(s2, X, Lenv, Renv)
        f2 = mo.sweep_step(s2, f_in, y1h, left_dir=left, **KW)
        f2 = mo.sweep_step(s2, f2, y1h, left_dir=left, **KW)
        assert s2.l_pos == (1 if left else 5) and np.isfinite(f2).all()
    # the sweep's own continuation and the one from the rebuilt environments agree (f_in is f of the truncated cores, f is not)
    s2 = st.copy()
    place(s2, X, Lenv, Renv)
    a = mo.sweep_step(s2, f_in, y1h, left_dir=False, **KW)
    b_ = mo.sweep_step(st, f_in, y1h, left_dir=False, **KW)
    np.testing.assert_allclose(a, b_, rtol=1e-12, atol=1e-300)


# ---------------------------------------------------------------------------------------------------------------
# the public surface
# ---------------------------------------------------------------------------------------------------------------
def test_switch_is_declared_exported_and_bound():
    header = open(os.path.join(ROOT, 'include', 'tnml.h')).read()
    assert re.search(r'int tnml_set_any_position\(tnml_ctx \*ctx, int on\);', header)
    assert 'tnml_set_any_position' in _hip.SYMBOLS and hasattr(_hip.lib(), 'tnml_set_any_position')
    assert callable(_hip.Context.set_any_position)


def _net(N=9, M=3):
    import tensornetworkforml_amd as pkg
    np.random.seed(1)
    return pkg.Network(N=N, M=M, L=2, act_fn='softmax', loss_fn='full_cross_ent', trunc='fixed')


def test_any_position_attribute_is_not_pickled_and_guards_the_calls():
    net = _net()
    assert net.any_position is False
    net._host_cores, net._l_pos, net._host_newer = random_cores_at(9, 2, 2, [3] * 8, 4, np.random.default_rng(0)), 4, True    # label on site 4
    X = np.zeros((3, 9, 2))
    for call in (lambda: net.forward(X), lambda: net.predict(X)):
        with pytest.raises(Exception, match='intermediate position'):
            call()
    net.any_position = True
    assert net.any_position is True
    net2 = pickle.loads(pickle.dumps(net))
    assert net2.any_position is False and net2.l_pos == 4 and net2._seg_left is False
    net._seg_left = True                                      # the direction of the last segment travels with the model
    assert pickle.loads(pickle.dumps(net))._seg_left is True and net.__getstate__()['seg_left'] is True
    net._seg_left = False
    assert 'any_position' not in net.__getstate__() and '_any_position' not in net.__getstate__()
    with pytest.raises(ValueError, match='steps_per_batch'):
        net.train_resident([], [], 0.1, steps_per_batch=0)


def schedule(N, k, l0, left0, n_batches):
    """(l_pos, left_dir, n_steps) per batch of train_resident(steps_per_batch=k) starting at l0 with previous direction left0."""
    out, l, left = [], l0, left0
    for _ in range(n_batches):
        if l == 0:
            left = False
        elif l == N - 1:
            left = True
        n = min(k, l if left else N - 1 - l)
        out.append((l, left, n))
        l += -n if left else n
    return out


def test_segment_schedule():
    net = _net(N=25)
    got, l = [], 0
    for _ in range(12):
        net._l_pos, net._host_newer = l, True
        left, n, first = net._next_segment(7)
        got.append((l, left, n))
        assert first == (l == (24 if left else 0)) and n >= 1
        l += -n if left else n
    assert got == schedule(25, 7, 0, False, 12)
    # 24 = 7 + 7 + 7 + 3: the segment that reaches an end is short, the next one turns round
    assert [g[2] for g in got[:8]] == [7, 7, 7, 3, 7, 7, 7, 3] and [g[1] for g in got[:8]] == [False] * 4 + [True] * 4
    # k = N - 1 from an end is the default schedule
    assert schedule(25, 24, 0, False, 3) == [(0, False, 24), (24, True, 24), (0, False, 24)]


@pytest.mark.parametrize('script', ['training_diagonals', 'training_binary_MNIST'])
def test_steps_per_batch_flag_needs_resident(script, capsys):
    import importlib
    mod = importlib.import_module('tensornetworkforml_amd.' + script)
    with pytest.raises(SystemExit):
        mod.main(['--steps-per-batch', '5'])
    assert '--steps-per-batch needs --resident' in capsys.readouterr().err


def test_any_position_host_side_under_sanitizers():
    """csrc/Makefile target `san-anypos`: tnml_api.hip's forward / predict / evaluate / sweep with the label at an intermediate site and
    the launch wrapper of kernels_meet.hip, built --cuda-host-only with -fsanitize=address,undefined, against the stand-in runtime of
    csrc/san/hip_stub.cpp (csrc/san/plan_anypos_main.cpp, a stand-alone program): every position of a ragged chain and C3 / C5 sizes,
    the four step paths, both directions, buffer growth in between, the refusals; every launch of label_meet_kernel and of the
    half-chains has its pointers and extents checked."""
    import shutil
    import subprocess
    if shutil.which('g++') is None or not os.path.exists('/opt/rocm/bin/hipcc'):
        pytest.skip('no g++ / hipcc')
    csrc = os.path.join(ROOT, 'tensornetworkforml_amd', 'csrc')
    out = subprocess.run(['make', '-C', csrc, '-j4', 'san-anypos'], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert 'any-position host planning under ASan + UBSan: ok' in out.stdout
    for name in ('ragged N 6 L 3', 'D 3 N 5 bond 3', 'bond 50 L 10 (chunked core)', 'c3 bond 20 b 5000', 'c5 bond 50 L 10 b 5000'):
        assert 'planned any-position ' + name in out.stdout, name
    m = re.search(r'any-position: (\d+) forwards, (\d+) segment starts, (\d+) label_meet launches checked', out.stdout)
    assert m and int(m.group(1)) > 100 and int(m.group(2)) > 100 and int(m.group(3)) > 300, out.stdout[-2000:]
    assert re.search(r'san-stub: \d+ launches checked \(\d+ kernels\), \d+ pointer extents checked, 0 live allocations', out.stdout)
