"""Label at an intermediate site on the GPU (include/tnml.h, tnml_set_any_position).

  1  forward at every position        f and every environment of both stacks against plain NumPy in float64
                                      (test_any_position_host.label_inside_forward); bit-equal at the ends with the switch on or off
  2  predict / evaluate               bit-equal to forward's f; counts over a list longer than the prediction buffers; resident state untouched
  3  segment start, stepwise          three right steps on batch A, a new batch, forward, two steps right -- and, from the same state, two
                                      steps left -- beside the float64 oracle (tnml_debug_enable), on every step path
  4  state machine                    the refusals, switch off and on; a refused call changes nothing
  5  Python                           Network.forward / evaluate / sweep_step mid-chain, train_resident(steps_per_batch), the scripts

Tolerances: the header of tests/test_hip_parity.py -- forward f and environments 2e-5 of max|.|; B, dB_raw, L2_grad, B_new after gauge
alignment 5e-3; sigma 2e-3; f_new 5e-3; accuracy exact; MAE 2e-3.  Every test prints the worst values it observed.
"""
import contextlib
import io
import os
import pickle
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import golden_util as gu                                         # noqa: E402
from test_any_position_host import label_inside_forward, place, random_cores_at, schedule    # noqa: E402
from tensornetworkforml_amd import _hip                          # noqa: E402
from tensornetworkforml_amd import data_generator as gen         # noqa: E402
from tensornetworkforml_amd import Network_class as tn           # noqa: E402
from oracle import mps_oracle as mo                              # noqa: E402

pytestmark = pytest.mark.gpu

STATE = -2
S_L, S_R = _hip.SIDE_LEFT, _hip.SIDE_RIGHT


def quiet():
    return contextlib.redirect_stdout(io.StringIO())


def relerr(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def _code(call):
    with pytest.raises(_hip.TnmlError) as ei:
        call()
    return ei.value.code


def features(rng, b, N, D):
    p = rng.random((b, N)) * (rng.random((b, N)) > 0.5)
    return gen.psi(p, D).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------
# 1. forward at every position
# ---------------------------------------------------------------------------------------------------------------
RAGGED = [2, 4, 3, 4, 2]
FORWARD_CASES = {
    'ragged b 5': dict(N=6, D=2, L=3, M=4, bond=RAGGED, b=5, plain=False, sites=None),
    'ragged b 70': dict(N=6, D=2, L=3, M=4, bond=RAGGED, b=70, plain=False, sites=None),
    'ragged b 5, plain chain': dict(N=6, D=2, L=3, M=4, bond=RAGGED, b=5, plain=True, sites=None),
    'ragged b 70, plain chain': dict(N=6, D=2, L=3, M=4, bond=RAGGED, b=70, plain=True, sites=None),
    'D 3': dict(N=5, D=3, L=3, M=3, bond=[3] * 4, b=70, plain=False, sites=None),
    'bond 50, ten labels (chunked label core)': dict(N=5, D=2, L=10, M=50, bond=[50] * 4, b=70, plain=False, sites=[2]),
}


@pytest.mark.parametrize('case', list(FORWARD_CASES))
def test_forward_at_every_position(case):
    c = FORWARD_CASES[case]
    N, D, L, M, b = c['N'], c['D'], c['L'], c['M'], c['b']
    rng = np.random.default_rng(7)
    X = features(rng, b, N, D)
    y = rng.integers(0, L, b)
    X64 = X.astype(np.float64)
    ctx = _hip.Context(N, D, L, M, b)
    ctx.set_chain_path(c['plain'])
    ctx.set_input(X, y)
    worst = dict(f=0.0, env=0.0)
    for l in (c['sites'] if c['sites'] is not None else range(N)):      # l = 1 and l = N-2: one side is a single site
        cores32 = [a.astype(np.float32) for a in random_cores_at(N, D, L, c['bond'], l, rng, scale=0.5 * max(c['bond']))]
        Lenv, Renv, f_o = label_inside_forward([a.astype(np.float64) for a in cores32], l, X64)
        inside = 0 < l < N - 1
        ctx.set_any_position(False)
        ctx.set_cores(cores32, l)
        if inside:
            assert _code(ctx.forward) == STATE
            f_off = None
        else:
            f_off = ctx.forward()
            env_off = {i: ctx.get_env(S_R if l == 0 else S_L, i) for i in (range(1, N) if l == 0 else range(N - 1))}
        ctx.set_any_position(True)
        ctx.set_cores(cores32, l)
        f_d = ctx.forward()
        worst['f'] = max(worst['f'], relerr(f_d, f_o))
        for i in range(l):
            e = ctx.get_env(S_L, i)
            worst['env'] = max(worst['env'], relerr(e, Lenv[i]))
            if f_off is not None:
                assert np.array_equal(e, env_off[i])
        for i in range(l + 1, N):
            e = ctx.get_env(S_R, i)
            worst['env'] = max(worst['env'], relerr(e, Renv[i]))
            if f_off is not None:
                assert np.array_equal(e, env_off[i])
        if f_off is not None:
            assert np.array_equal(f_d, f_off)                            # the ends take the path they always took
        # the metrics of the resident f
        correct, abs_sum, nonfinite = ctx.resident_metrics('linear', 1.0)
        assert correct == int((np.argmax(f_d, axis=0) == y).sum()) and nonfinite == 0
    ctx.close()
    print('forward at every position,', case, {k: '%.2e' % v for k, v in worst.items()})
    assert worst['f'] < 2e-5 and worst['env'] < 2e-5


# ---------------------------------------------------------------------------------------------------------------
# 2. predict and evaluate
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('D,l', [(2, 2), (2, 4), (3, 1)])
def test_predict_and_evaluate_inside_the_chain(D, l):
    N, L, M, b, n = 6, 3, 4, 70, 300
    rng = np.random.default_rng(3 + D)
    Xall = features(rng, n, N, D)
    yall = rng.integers(0, L, n)
    cores32 = [a.astype(np.float32) for a in random_cores_at(N, D, L, RAGGED if D == 2 else [3] * 5, l, rng, scale=1.5)]
    ctx = _hip.Context(N, D, L, M, b)
    ctx.set_any_position(True)
    ctx.set_cores(cores32, l)
    ctx.dataset_attach(Xall, yall)
    resident = np.arange(b) * 3
    ctx.select_indices(resident)
    f_res = ctx.forward()
    envs = [ctx.get_env(S_L, i) for i in range(l)] + [ctx.get_env(S_R, i) for i in range(l + 1, N)]
    # the same samples through the three prediction calls
    assert np.array_equal(ctx.predict(Xall[resident]), f_res)
    assert np.array_equal(ctx.predict_indices(resident), f_res)
    idx = rng.integers(0, n, 2 * 128 + 41)                               # longer than the prediction buffers (128 samples): three chunks
    T = 0.1
    results = {act: ctx.eval_indices(idx, act, T) for act in ('linear', 'softmax')}
    f_all = ctx.predict_indices(idx)                                     # (this grows the prediction buffers)
    assert np.array_equal(f_all[:, :7], ctx.predict(Xall[idx[:7]]))
    for act, res in results.items():                                     # ... and the chunking does not matter (float64 sums of the same terms)
        again = ctx.eval_indices(idx, act, T)
        assert again[0] == res[0] and again[2] == res[2] and abs(again[1] - res[1]) <= 1e-9 * abs(res[1])
    worst = 0.0
    for act, (correct, abs_sum, nonfinite) in results.items():
        fa = mo.apply_act_func(f_all.astype(np.float64), act, T)
        assert correct == int((np.argmax(f_all, axis=0) == yall[idx]).sum()) and nonfinite == 0
        mae = np.abs(mo.one_hot(yall[idx], L) - fa).mean()
        worst = max(worst, abs(abs_sum / (len(idx) * L) - mae))
    # the resident batch, its f and its environments are untouched
    assert np.array_equal(ctx.get_f(), f_res)
    for e0, e1 in zip(envs, [ctx.get_env(S_L, i) for i in range(l)] + [ctx.get_env(S_R, i) for i in range(l + 1, N)]):
        assert np.array_equal(e0, e1)
    assert ctx.resident_metrics('linear', 1.0)[0] == int((np.argmax(f_res, axis=0) == yall[resident]).sum())
    ctx.close()
    print('evaluate inside the chain D %d l %d: MAE difference %.2e' % (D, l, worst))
    assert worst < 2e-3


# ---------------------------------------------------------------------------------------------------------------
# 3. segment start, stepwise
# ---------------------------------------------------------------------------------------------------------------
def _compare_step(ctx, st, rec, met, f_d, f_o, worst, b):
    def upd(key, v):
        worst[key] = max(worst.get(key, 0.0), float(v))
    shp = rec['B'].shape
    B_d = ctx.step_debug('B').reshape(shp)
    sa, tc = gu.gauge_signs(B_d, rec['B'])
    upd('B', relerr(B_d, gu.regauge(rec['B'], sa, tc)))
    for key in ('dB_raw', 'L2_grad', 'B_new'):
        upd(key, relerr(ctx.step_debug(key).reshape(shp), gu.regauge(rec[key], sa, tc)))
    sig = ctx.step_debug('sigma')
    upd('sigma', np.abs(sig - rec['S']).max() / rec['S'].max())
    upd('f_new', relerr(f_d, f_o))
    upd('acc', abs(float(met[0, 0]) - rec['accuracy']) * b)
    upd('MAE', abs(float(met[0, 1]) - rec['MAE']))
    _, bond_d, lp = ctx.get_cores()
    assert lp == ctx.l_pos == st.l_pos and list(bond_d) == list(st.bond)


SEGMENT_PATHS = ['single launch', 'classic sequence', 'large tensor', 'D 3', 'reference policy', 'adaptive policy']


@pytest.mark.parametrize('path', SEGMENT_PATHS)
def test_segment_start_step_by_step(path):
    N, M, bA, bB = 8, 4, 37, 42
    D = 3 if path == 'D 3' else 2
    trunc = {'reference policy': 'reference', 'adaptive policy': 'adaptive'}.get(path, 'fixed')
    L = 3
    rng = np.random.default_rng(17)
    XA, XB = features(rng, bA, N, D), features(rng, bB, N, D)
    yA, yB = rng.integers(0, L, bA), rng.integers(0, L, bB)
    st = mo.MPSState(N, D, L, M, mo.random_cores(N, M, D, L, rng=rng, scale=M * 0.5 * 0.64 * D))
    mo.calibrate(st, XA.astype(np.float64))
    cores32 = [c.astype(np.float32) for c in st.cores]
    st = mo.MPSState(N, D, L, M, [c.astype(np.float64) for c in cores32])
    kw = dict(lr=1e-2, weight_dec=1e-3, L2_flag=True, act_fn='softmax', loss_fn='full_cross_ent', T=0.1, trunc=trunc)
    hp = (kw['lr'], kw['weight_dec'], True, kw['act_fn'], kw['loss_fn'], kw['T'], trunc)
    ctx = _hip.Context(N, D, L, M, bA)
    if path == 'classic sequence':
        ctx.set_step_pipeline(0)
    if path == 'large tensor':
        ctx.set_narrow_path(1)
    ctx.set_any_position(True)
    ctx.debug_enable(True)
    ctx.set_cores(cores32, 0)
    ctx.set_input(XA, yA)
    worst = {}
    # three right steps on batch A
    XA64, XB64 = XA.astype(np.float64), XB.astype(np.float64)
    y1hA, y1hB = mo.one_hot(yA, L), mo.one_hot(yB, L)
    f_o = mo.forward(st, XA64)
    f_d = ctx.forward()
    assert relerr(f_d, f_o) < 2e-5
    for j in range(3):
        rec = {}
        f_o = mo.sweep_step(st, f_o, y1hA, left_dir=False, record=rec, **kw)
        met, f_d = ctx.sweep(False, 1, j == 0, *hp)
        _compare_step(ctx, st, rec, met, f_d, f_o, worst, bA)
    assert ctx.l_pos == 3
    cores_mid, bond_mid, _ = ctx.get_cores()
    st_mid = mo.MPSState(N, D, L, M, [c.astype(np.float64) for c in cores_mid], l_pos=3)
    # batch B (larger: the batch buffers grow), forward inside the chain, two steps to the right on the SAME context
    for left, own_state in ((False, True), (True, False)):
        if not own_state:                            # the same state again (the device's cores after the three steps), then to the left
            ctx.set_cores(cores_mid, 3)
            st = st_mid.copy()
        ctx.set_input(XB, yB)
        assert _code(lambda: ctx.sweep(left, 1, False, *hp)) == STATE     # a new batch needs its forward
        f_d = ctx.forward()
        # (forward against the expectation from the device's own cores; the steps beside the oracle's own state)
        worst['f_forward'] = max(worst.get('f_forward', 0.0), relerr(f_d, label_inside_forward(st_mid.cores, 3, XB64)[2]))
        Lenv, Renv, f_o = label_inside_forward(st.cores, 3, XB64)
        place(st, XB64, Lenv, Renv)
        if left and path == 'single launch':
            # update_B after an intermediate forward: the oracle's B_new of the step that follows
            s2 = st.copy()
            place(s2, XB64, Lenv, Renv)
            rec = {}
            mo.sweep_step(s2, f_o, y1hB, left_dir=True, record=rec, **kw)
            Bn, met2 = ctx.update_B(None, True, *hp[:6])
            Bn = Bn[:rec['B_new'].size].reshape(rec['B_new'].shape)
            worst['update_B'] = relerr(Bn, rec['B_new'])
            assert ctx.l_pos == 3 and abs(float(met2[0]) - rec['accuracy']) * bB < 0.5
        for j in range(2):
            rec = {}
            f_o = mo.sweep_step(st, f_o, y1hB, left_dir=left, record=rec, **kw)
            met, f_d = ctx.sweep(left, 1, False, *hp)
            _compare_step(ctx, st, rec, met, f_d, f_o, worst, bB)
        assert ctx.l_pos == (1 if left else 5)
    ctx.close()
    print('segment start,', path, {k: '%.2e' % v for k, v in worst.items()})
    assert worst['f_forward'] < 2e-5
    assert worst['B'] < 5e-3 and worst['dB_raw'] < 5e-3 and worst['L2_grad'] < 5e-3 and worst['B_new'] < 5e-3
    assert worst.get('update_B', 0.0) < 5e-3
    assert worst['sigma'] < 2e-3 and worst['f_new'] < 5e-3
    assert worst['acc'] < 0.5 and worst['MAE'] < 2e-3


@pytest.mark.parametrize('calls', [(3,), (1, 2), (1, 1, 1)])
def test_segment_of_several_steps_per_call(calls):
    """A segment of three steps as one call, as 1 + 2 and as three calls, in both directions, against the oracle: within a call the
    first step of the segment takes the classic sequence and the single-launch step resumes with the second."""
    N, M, L, D, b = 10, 6, 2, 2, 90
    rng = np.random.default_rng(5)
    X, y = features(rng, b, N, D), rng.integers(0, L, b)
    X64, y1h = X.astype(np.float64), mo.one_hot(y, L)
    cores32 = [a.astype(np.float32) for a in random_cores_at(N, D, L, [M] * (N - 1), 4, rng, scale=0.5 * M * 0.64 * D)]
    kw = dict(lr=1e-2, weight_dec=1e-3, L2_flag=True, act_fn='softmax', loss_fn='full_cross_ent', T=0.1, trunc='fixed')
    hp = (1e-2, 1e-3, True, 'softmax', 'full_cross_ent', 0.1, 'fixed')
    worst = dict(f=0.0, acc=0.0, MAE=0.0)
    for left in (False, True):
        st = mo.MPSState(N, D, L, M, [c.astype(np.float64) for c in cores32], l_pos=4)
        Lenv, Renv, f_o = label_inside_forward(st.cores, 4, X64)
        place(st, X64, Lenv, Renv)
        acc_o, mae_o = [], []
        for _ in range(3):
            rec = {}
            f_o = mo.sweep_step(st, f_o, y1h, left_dir=left, record=rec, **kw)
            acc_o.append(rec['accuracy']); mae_o.append(rec['MAE'])
        ctx = _hip.Context(N, D, L, M, b)
        ctx.set_any_position(True)
        ctx.set_cores(cores32, 4)
        ctx.set_input(X, y)
        ctx.forward(want_f=False)
        outs = [ctx.sweep(left, n, False, *hp) for n in calls]
        met, f_d = np.concatenate([m for m, _ in outs]), outs[-1][1]
        _, bond_d, lp = ctx.get_cores()
        ctx.close()
        assert lp == st.l_pos == (1 if left else 7) and list(bond_d) == list(st.bond)
        worst['f'] = max(worst['f'], relerr(f_d, f_o))
        worst['acc'] = max(worst['acc'], float(np.abs(met[:, 0] - np.array(acc_o)).max() * b))
        worst['MAE'] = max(worst['MAE'], float(np.abs(met[:, 1] - np.array(mae_o)).max()))
    print('segment of three steps as', calls, {k: '%.2e' % v for k, v in worst.items()})
    assert worst['f'] < 5e-3 and worst['acc'] < 0.5 and worst['MAE'] < 2e-3


# ---------------------------------------------------------------------------------------------------------------
# 4. state machine
# ---------------------------------------------------------------------------------------------------------------
def test_state_machine(monkeypatch):
    N, M, L, D, b = 6, 4, 3, 2, 20
    rng = np.random.default_rng(9)
    X, y = features(rng, 60, N, D), rng.integers(0, L, 60)
    cores32 = [a.astype(np.float32) for a in random_cores_at(N, D, L, RAGGED, 3, rng, scale=1.5)]
    hp = (1e-2, 1e-3, True, 'softmax', 'full_cross_ent', 0.1, 'fixed')
    ctx = _hip.Context(N, D, L, M, b)
    ctx.set_cores(cores32, 3)
    ctx.dataset_attach(X, y)
    ctx.select_indices(np.arange(b))

    def snapshot():
        cores, bond, lp = ctx.get_cores()
        return [c.copy() for c in cores], list(bond), lp

    def same(a, b_):
        return a[1] == b_[1] and a[2] == b_[2] and all(np.array_equal(x, z) for x, z in zip(a[0], b_[0]))

    s0 = snapshot()
    # switch off: the four calls refuse an intermediate position, and the switch exists
    assert hasattr(_hip.lib(), 'tnml_set_any_position')
    ctx.set_any_position(False)
    idx = np.arange(30)
    for call in (ctx.forward, lambda: ctx.predict(X[:5]), lambda: ctx.predict_indices(idx), lambda: ctx.eval_indices(idx, 'softmax', 0.1)):
        assert _code(call) == STATE
    assert same(s0, snapshot())
    # switch on
    ctx.set_any_position(True)
    f0 = ctx.forward()
    assert _code(lambda: ctx.sweep(False, 1, True, *hp)) == STATE         # first_of_sweep stays ends-only
    assert _code(lambda: ctx.sweep(True, 1, True, *hp)) == STATE
    assert _code(ctx.forward_logabsmax) == STATE                          # calibration stays ends-only
    assert same(s0, snapshot()) and np.array_equal(ctx.get_f(), f0)
    ctx.sweep(False, 1, False, *hp)                                       # the segment starts; the other direction now needs a forward
    s1, f1 = snapshot(), ctx.get_f()
    assert s1[2] == 4
    assert _code(lambda: ctx.sweep(True, 1, False, *hp)) == STATE
    assert same(s1, snapshot()) and np.array_equal(ctx.get_f(), f1)
    ctx.forward()
    ctx.sweep(True, 1, False, *hp)                                        # ... and after one it runs
    assert ctx.l_pos == 3
    ctx.forward()
    f2 = ctx.get_f()
    ctx.select_indices(np.arange(b) + 7)
    s2 = snapshot()
    assert _code(lambda: ctx.sweep(False, 1, False, *hp)) == STATE        # a new batch without a forward
    assert _code(lambda: ctx.sweep(True, 1, False, *hp)) == STATE
    assert same(s2, snapshot()) and np.array_equal(ctx.get_f(), f2)
    ctx.forward()
    ctx.sweep(True, 2, False, *hp)
    assert ctx.l_pos == 1
    # a segment that reached the end: the opposite sweep needs its forward as ever
    ctx.forward()
    ctx.sweep(True, 1, False, *hp)
    assert ctx.l_pos == 0
    assert _code(lambda: ctx.sweep(False, N - 1, True, *hp)) == STATE
    ctx.forward()
    ctx.sweep(False, N - 1, True, *hp)
    assert ctx.l_pos == N - 1
    ctx.close()
    # with a one-rank communicator the switch itself is refused
    from tensornetworkforml_amd import dist as tdist
    monkeypatch.setenv('TNML_FORCE_COMM', '1')
    ctx = _hip.Context(N, D, L, M, b)
    tdist.attach_comm(ctx, 0, 1)
    assert _code(lambda: ctx.set_any_position(True)) == STATE
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------
# 5. Python
# ---------------------------------------------------------------------------------------------------------------
def _golden_net_mid_chain(steps=5):
    from test_network_gpu import net_from_golden
    d = gu.load('traj_fixed_N16_script')
    net = net_from_golden(d)
    X, y = d['X'], d['y']
    lr, wd = float(d['lr']), float(d['wd'])
    y1h = mo.one_hot(y, int(d['L']))
    f = net.forward(X)
    for _ in range(steps):
        f = net.sweep_step(f, y1h, lr, X.shape[0], wd)
    assert net.l_pos == steps
    return d, net, lr, wd


def test_network_forward_evaluate_and_sweep_step_inside_the_chain():
    d, net, lr, wd = _golden_net_mid_chain()
    N, L, D, M = int(d['N']), int(d['L']), int(d['D']), int(d['M'])
    l = net.l_pos
    rng = np.random.default_rng(2)
    X = features(rng, 53, N, D).astype(np.float64)
    y = rng.integers(0, L, 53)
    with pytest.raises(Exception, match='intermediate position'):
        net.forward(X)
    blob = pickle.dumps(net)
    worst = {}
    for left in (False, True):
        net = pickle.loads(blob)
        assert net.any_position is False and net.l_pos == l
        net.any_position = True
        f = net.forward(X)
        cores64 = [c.astype(np.float64) for c in net._ctx.get_cores()[0]]
        Lenv, Renv, f_o = label_inside_forward(cores64, l, X.astype(np.float32).astype(np.float64))
        worst['f'] = max(worst.get('f', 0.0), relerr(f.elem, f_o))
        lc, rc = net.l_cum_contraction, net.r_cum_contraction
        assert len(lc) == l and len(rc) == N - 1 - l
        env = max([relerr(lc[i].elem.T, Lenv[i]) for i in range(l)] + [relerr(rc[k].elem.T, Renv[l + 1 + k]) for k in range(N - 1 - l)])
        worst['env'] = max(worst.get('env', 0.0), env)
        assert relerr(net.predict(X).elem, f_o) < 2e-5
        # evaluate on an attached dataset
        net.attach_dataset(X, y)
        acc, mae = net.evaluate(np.arange(53))
        fa = mo.apply_act_func(f_o, net.act_fn, net.T)
        assert acc == float((np.argmax(f.elem, axis=0) == y).mean()) and abs(mae - np.abs(mo.one_hot(y, L) - fa).mean()) < 2e-3
        # one step from there, beside the oracle
        st = mo.MPSState(N, D, L, M, cores64, l_pos=l)
        place(st, X.astype(np.float32).astype(np.float64), Lenv, Renv)
        kw = dict(lr=lr, weight_dec=wd, L2_flag=bool(d['L2_flag']), act_fn=net.act_fn, loss_fn=net.loss_fn, T=net.T, trunc=net.trunc)
        f_new_o = mo.sweep_step(st, f_o, mo.one_hot(y, L), left_dir=left, **kw)
        f_new = net.sweep_step(f, mo.one_hot(y, L), lr, 53, wd, L2_flag=bool(d['L2_flag']), left_dir=left)
        worst['f_new'] = max(worst.get('f_new', 0.0), relerr(f_new.elem, f_new_o))
        lp = net.l_pos
        assert lp == st.l_pos == (l - 1 if left else l + 1)
        # the lists hold exactly what is valid on the device: the environments beyond the label site on both sides
        lc, rc = net.l_cum_contraction, net.r_cum_contraction
        want_l = list(range(lp)) if left else list(range(lp - 1))
        want_r = list(range(N - 1, lp + 1, -1)) if left else list(range(lp + 1, N))
        assert len(lc) == len(want_l) and len(rc) == len(want_r)
        still = max([relerr(lc[k].elem.T, Lenv[i]) for k, i in enumerate(want_l) if i in Lenv and i < min(l, lp)] +
                    [relerr(rc[k].elem.T, Renv[i]) for k, i in enumerate(want_r) if i in Renv and i > max(l, lp)])
        worst['env_after'] = max(worst.get('env_after', 0.0), still)
    print('Network inside the chain', {k: '%.2e' % v for k, v in worst.items()})
    assert worst['f'] < 2e-5 and worst['env'] < 2e-5 and worst['env_after'] < 2e-5 and worst['f_new'] < 5e-3


def _resident_runs(steps_list, n_epochs=2, linear_dim=5, M=6, seed=31):
    np.random.seed(seed)
    data, label = gen.create_dataset(600, linear_dim, 0.6)
    sizes = dict(train_batch_size=120, val_batch_size=50, test_batch_size=64)
    x_cal = gen.psi(data.reshape(len(data), -1)[:120], 2)
    with quiet():
        net0 = tn.Network(N=linear_dim ** 2, M=M, D=2, L=2, calibration_X=x_cal, normalize=True, act_fn='softmax', loss_fn='full_cross_ent',
                          trunc='fixed')
    blob = pickle.dumps(net0)
    runs = []
    for k in steps_list:
        net = pickle.loads(blob)
        np.random.seed(seed + 1)
        with quiet():
            _, tr_idx, va_idx, _ = gen.prepare_device_dataset(net, data, label, 1, 0.2, D=2, pixels=False, **sizes)
            val_acc, var_hist = net.train_resident(tr_idx, va_idx, lr=0.01, n_epochs=n_epochs, weight_dec=1e-3, **({} if k is None else dict(steps_per_batch=k)))
        cores, bond, lp = net._ctx.get_cores()
        runs.append(dict(net=net, val_acc=list(val_acc), var_hist=var_hist, cores=cores, bond=list(bond), l_pos=lp))
    return blob, data, label, sizes, runs


def _same_cores(a, b):
    return a['bond'] == b['bond'] and a['l_pos'] == b['l_pos'] and all(
        x.shape == z.shape and np.array_equal(x.view(np.uint32), z.view(np.uint32)) for x, z in zip(a['cores'], b['cores']))


def test_steps_per_batch_of_a_whole_sweep_is_the_default_training():
    N = 25
    _, _, _, _, (default, whole) = _resident_runs([None, N - 1])
    assert _same_cores(default, whole) and default['val_acc'] == whole['val_acc']
    assert isinstance(whole['var_hist'], list) and len(whole['var_hist']) == 2
    assert default['var_hist'].shape == (2, 2, 4 * (N - 1)) and np.array_equal(np.array(whole['var_hist']), default['var_hist'])
    assert whole['net'].segment_log == schedule(N, N - 1, 0, False, 8) and whole['net'].any_position is False
    na, nb = pickle.loads(pickle.dumps(default['net'])), pickle.loads(pickle.dumps(whole['net']))
    assert na.l_pos == nb.l_pos
    for ta, tb in zip(na.As, nb.As):
        assert list(ta.axes_names) == list(tb.axes_names) and np.array_equal(ta.elem, tb.elem)


def test_steps_per_batch_schedule_and_the_same_schedule_by_hand():
    N, k, seed = 25, 7, 31
    blob, data, label, sizes, (run,) = _resident_runs([k])
    net = run['net']
    want = schedule(N, k, 0, False, 8)
    assert net.segment_log == want and [s[2] for s in want] == [7, 7, 7, 3, 7, 7, 7, 3]
    assert len(run['var_hist']) == 2 and [v.shape for v in run['var_hist']] == [(2, 24), (2, 24)]
    assert all(np.isfinite(v).all() for v in run['var_hist']) and np.isfinite(run['val_acc']).all()
    assert all(np.isfinite(c).all() for c in run['cores']) and run['l_pos'] == net.l_pos == 0
    # the same schedule through the C ABI calls
    net0 = pickle.loads(blob)
    cores0 = [np.asarray(c, dtype=np.float32) for c in net0._host_cores]
    ctx = _hip.Context(N, 2, 2, net0.M, sizes['train_batch_size'])
    ctx.set_any_position(True)
    ctx.set_cores(cores0, 0)
    ctx.dataset_attach(gen.psi(data.reshape(len(data), -1), 2), label)
    tr, va, _ = gen.split_indices(len(data), 1, 0.2)
    tr_idx = gen.IndexLoader(tr, sizes['train_batch_size'], shuffle=True, drop_last=True)
    va_idx = gen.IndexLoader(va, sizes['val_batch_size'], shuffle=True, drop_last=True)
    np.random.seed(seed + 1)
    seg = iter(want)
    hist, vals = [], []
    for epoch in range(2):
        vh = [[], []]
        for idx in tr_idx:
            ctx.select_indices(idx)
            ctx.forward(want_f=False)
            ctx.resident_metrics('softmax', net0.T)
            l, left, n = next(seg)
            assert ctx.l_pos == l
            met, _ = ctx.sweep(left, n, l in (0, N - 1), 0.01, 1e-3, True, 'softmax', 'full_cross_ent', net0.T, 'fixed', want_f=False)
            vh[0].extend(float(v) for v in met[:, 0])
            vh[1].extend(float(v) for v in met[:, 1])
        hist.append(np.array(vh))
        vals.append(np.mean([ctx.eval_indices(idx, 'softmax', net0.T)[0] / len(idx) for idx in va_idx]))
    cores, bond, lp = ctx.get_cores()
    ctx.close()
    assert _same_cores(run, dict(cores=cores, bond=list(bond), l_pos=lp))
    assert vals == run['val_acc'] and all(np.array_equal(a, b) for a, b in zip(hist, run['var_hist']))


def _printed_figures(text):
    acc = [ln for ln in text.splitlines() if 'Accuracy:' in ln]
    mae = [ln for ln in text.splitlines() if 'Mean Absolute Error:' in ln]
    assert len(acc) == 1 and len(mae) == 1, text
    return float(acc[0].split(':')[1]), float(mae[0].split(':')[1])


def test_diagonals_scripts_with_steps_per_batch_and_a_model_saved_mid_sweep(tmp_path, monkeypatch):
    from tensornetworkforml_amd import training_diagonals as train_script
    from tensornetworkforml_amd import evaluate_diagonals as eval_script
    monkeypatch.chdir(tmp_path)
    out = str(tmp_path / 'diag.dat')
    np.random.seed(3)
    with quiet():
        val_acc, var_hist = train_script.main(['--n_samples', '2000', '--n_train_batch', '2', '--n_epochs', '3', '--resident',
                                               '--steps-per-batch', '5', '--out', out])
    # six batches of five steps from site 0 of 64: the label stands on site 30
    assert len(var_hist) == 3 and all(v.shape == (2, 10) and np.isfinite(v).all() for v in var_hist) and len(val_acc) == 3
    with open(out, 'rb') as fh:
        net = pickle.load(fh)
    assert net.l_pos == 30 and net.any_position is False and net._seg_left is False
    buf = io.StringIO()
    np.random.seed(8)
    with contextlib.redirect_stdout(buf):
        acc, mae = eval_script.main(['--filename', out, '--n_samples', '500', '--batch_size', '128'])
    assert _printed_figures(buf.getvalue()) == (float(repr(acc)), float(repr(mae)))
    assert 0.0 <= acc <= 1.0 and 0.0 <= mae <= 1.0
    # the same figures from Network.evaluate on the same data; without the switch the model refuses
    np.random.seed(8)
    data, label = gen.create_dataset(500, 8, 0.6)
    with quiet():
        _, _, _, test_loader = gen.prepare_device_dataset(net, data, label, 0, 0, 1, 1, 128, D=net.D, pixels=True)
    with pytest.raises(Exception, match='intermediate position'):
        net.evaluate(test_loader)
    net.any_position = True
    assert net.evaluate(test_loader) == (acc, mae)


def test_binary_mnist_script_with_steps_per_batch(tmp_path, monkeypatch):
    from tensornetworkforml_amd import training_binary_MNIST as train_script
    from test_network_gpu import _synthetic_mnist
    root = str(tmp_path / 'datasets')
    _synthetic_mnist(root, 2000, 500, 5)
    monkeypatch.chdir(tmp_path)
    out = str(tmp_path / 'mnist.dat')
    np.random.seed(4)
    with quiet():
        val_acc, var_hist = train_script.main(['--data_dir', root, '--n_epochs', '2', '--n_train_batch', '4', '--normalise', '--lr', '0.01',
                                               '--L2_decay', '1e-3', '--resident', '--steps-per-batch', '5', '--out', out])
    assert len(var_hist) == 2 and all(v.shape == (2, 20) and np.isfinite(v).all() for v in var_hist)
    assert all(0.0 <= v <= 1.0 for v in val_acc)
    with open(out, 'rb') as fh:
        net = pickle.load(fh)
    assert net.N == 196 and net.l_pos == 40
