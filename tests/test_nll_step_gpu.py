"""Likelihood training on the device (tnml_nll_step, tnml_nll_train_indices, tnml_set_nll_overlap) against the
float64 reference of tests/nll_step_reference.py.  The bounds are read from that module's emulation tables (ten times the float32
emulation's figure, rounded up to one digit; tests/test_nll_step_host.py asserts the tables); everything else is bit-equality.
The optimiser state has no read-back: where a test says "and the state", both contexts take one more identical step and their cores
are compared again.

  1  one step against the reference      every row of nll_reference.likelihood_cases(), joint and marginal, SGD plain / SGD clip +
                                         momentum / Adam, renorm on and off
  2  three steps with state              momentum and Adam on nll_step_reference.three_step_cases()
  3  bit-equalities                      chunks, index form, repetition, overlap, one call of four steps, lr = 0, the values
  4  renormalisation                     norms kept within 2^-22; without it no norm shrinks
  5  the short run                       20 steps against the reference trajectory
  6  the guard                           f_c == 0 in the middle batch of three; an un-calibrated chain
  7  refusals and state
  8  Network.nll_step, train_generative, the script option
"""
import ctypes as C
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
import nll_reference as N                                          # noqa: E402
import nll_step_reference as R                                     # noqa: E402
from tensornetworkforml_amd import _hip                            # noqa: E402
from tensornetworkforml_amd import data_generator as gen           # noqa: E402

pytestmark = pytest.mark.gpu

ARG, STATE, NONFINITE = -1, -2, -7
BAD_BATCH, NOT_APPLIED = 8, 16


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


def configure(ctx, name):
    o = R.OPTIMS[name]
    ctx.optim_config(o['kind'], momentum=o['momentum'], eps=o.get('eps', 1e-8), clip=o['clip'])


def dev_cores(ctx):
    return [c.astype(np.float64) for c in ctx.get_cores()[0]]


def same(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def grid_metric(D):
    _, phi, w = N.grid(N.K, D)
    return N.gram(phi, w)


# ---------------------------------------------------------------------------------------------------------------
# 1. one step against the reference
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('lc', N.likelihood_cases(), ids=N.likelihood_id)
def test_one_step_against_the_reference(lc):
    D, cap, L, _, l = lc[0]
    row = lc[0][:3]
    case = R.StepCase(lc)
    ctx = new_ctx(case.cores, l, D, L)
    for cfg in R.configs():
        objective, name, renorm = cfg
        ref, lr = case.reference(cfg)
        ctx.set_cores(A.as32(case.cores), l)
        configure(ctx, name)
        v = ctx.nll_step(case.X, case.y(objective), case.S, lr, R.WD, renorm)
        err, bound = R.step_deviation(dev_cores(ctx), ref.cores, case.cores), R.step_bound(row, cfg)
        verr = abs(v[0] - case.value[objective]) / max(1.0, abs(case.value[objective]))
        print('%s %s: step %.2e of max|dA| (bound %.0e)  value %.2e' % (N.likelihood_id(lc), R.config_id(cfg), err, bound, verr))
        assert v[2] == 0 and v[3] == 0
        assert verr <= N.gpu_bounds(row, objective)[1]
        assert err <= bound, (R.config_id(cfg), err, bound)
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------
# 2. three steps with state
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('lc', R.three_step_cases(), ids=N.likelihood_id)
def test_three_steps_with_state(lc):
    D, cap, L, _, l = lc[0]
    case = R.StepCase(lc)
    ctx = new_ctx(case.cores, l, D, L)
    for name in R.STATE_OPTIMS:
        ref, lr = R.three_steps(case, name)
        ctx.set_cores(A.as32(case.cores), l)
        configure(ctx, name)
        for _ in range(3):
            v = ctx.nll_step(case.X, case.lab, case.S, lr, R.WD, True)
            assert v[2] == 0 and v[3] == 0
        err, bound = R.step_deviation(dev_cores(ctx), ref.cores, case.cores), R.three_step_bound(lc[0][:3], name)
        print('%s three steps, %s: %.2e of max|dA| (bound %.0e)' % (N.likelihood_id(lc), name, err, bound))
        assert err <= bound, (name, err, bound)
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------
# 3. bit-equalities
# ---------------------------------------------------------------------------------------------------------------
BIT_CASE = (2, 33, 2, 17, 8)
HYPER = dict(lr=0.02, weight_dec=1e-2)


def bit_setup(b):
    D, cap, L, _, l = BIT_CASE
    cores = N.build_chain(BIT_CASE)
    lev, lab, X = N.draw_batch(BIT_CASE, cores, b, 1)
    return cores, l, D, L, lab.astype(np.int32), X, grid_metric(D)


def fresh(setup, name='sgd_clip_mom'):
    cores, l, D, L, lab, X, S = setup
    ctx = new_ctx(cores, l, D, L)
    ctx.dataset_attach(X, lab)
    configure(ctx, name)
    return ctx


@pytest.mark.parametrize('b', [70, 200])
@pytest.mark.parametrize('name', ['sgd_clip_mom', 'adam'])
def test_bit_equalities(b, name):
    setup = bit_setup(b)
    cores, l, D, L, lab, X, S = setup
    idx = np.arange(b, dtype=np.int32)
    a = fresh(setup, name)
    for labels in (True, False):
        y = lab if labels else None
        # chunks of 64, the index form, overlap on: each against the X form in the default chunk, two steps so that the state takes part
        others = {'chunk': fresh(setup, name), 'index': fresh(setup, name), 'overlap': fresh(setup, name)}
        others['chunk'].set_core_grad_chunk(64)
        others['overlap'].set_nll_overlap(True)
        a.set_cores(A.as32(cores), l)
        a.optim_reset()
        for _ in range(2):
            va = a.nll_step(X, y, S, renorm=True, **HYPER)
            for what, c in others.items():
                vc = c.nll_train_indices(idx, b, labels, S, renorm=True, **HYPER)[0] if what == 'index' else c.nll_step(X, y, S, renorm=True, **HYPER)
                assert vc.tobytes() == va.tobytes(), (what, vc, va)
        ca = a.get_cores()[0]
        for what, c in others.items():
            assert same(c.get_cores()[0], ca), what
            c.close()
        # the same call twice from the same cores and a reset state
        a.set_cores(A.as32(cores), l)
        a.optim_reset()
        for _ in range(2):
            vb = a.nll_step(X, y, S, renorm=True, **HYPER)
        assert vb.tobytes() == va.tobytes() and same(a.get_cores()[0], ca)
    a.close()


@pytest.mark.parametrize('overlap', [False, True])
def test_one_call_of_four_steps_and_the_values(overlap):
    """nll_train_indices over n = 200 and batch 50 against four nll_step calls; values[k][0:2] against nll_eval on the cores
    before step k"""
    setup = bit_setup(200)
    cores, l, D, L, lab, X, S = setup
    idx = np.random.default_rng(3).permutation(200).astype(np.int32)
    a, c = fresh(setup), fresh(setup)
    a.set_nll_overlap(overlap)
    vals = a.nll_train_indices(idx, 50, True, S, renorm=True, **HYPER)
    assert vals.shape == (4, 4) and (vals[:, 2:] == 0).all()
    for k in range(4):
        sel = idx[50 * k:50 * (k + 1)]
        ev = c.nll_eval_indices(sel, True, S)
        v = c.nll_step(X[sel], lab[sel], S, renorm=True, **HYPER)
        assert v.tobytes() == vals[k].tobytes(), (k, v, vals[k])
        assert ev[0] == v[0] and ev[1] == v[1]
    assert same(a.get_cores()[0], c.get_cores()[0])
    # and the state: a ragged call of three steps (70, 70, 60) against three calls
    v1 = a.nll_train_indices(idx, 70, False, S, renorm=False, **HYPER)
    v2 = np.concatenate([c.nll_train_indices(idx[k:k + 70], 70, False, S, renorm=False, **HYPER) for k in range(0, 200, 70)])
    assert v1.shape == (3, 4) and v1.tobytes() == v2.tobytes()
    assert same(a.get_cores()[0], c.get_cores()[0])
    a.close()
    c.close()


@pytest.mark.parametrize('name', ['sgd', 'sgd_clip_mom', 'adam'])
def test_lr_zero_leaves_the_cores(name):
    setup = bit_setup(70)
    cores, l, D, L, lab, X, S = setup
    ctx = fresh(setup, name)
    before = ctx.get_cores()[0]
    slots0, lab0 = ctx.core_slots()
    for renorm in (True, False):
        ctx.nll_step(X, lab, S, 0.0, 0.0, renorm)
        ctx.nll_train_indices(np.arange(70), 30, False, S, 0.0, 0.0, renorm)
    assert same(ctx.get_cores()[0], before)
    slots1, lab1 = ctx.core_slots()
    assert slots0.tobytes() == slots1.tobytes() and lab0.tobytes() == lab1.tobytes()
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------
# 4. renormalisation
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('lc', R.three_step_cases(), ids=N.likelihood_id)
def test_renormalisation(lc):
    """with renorm every core's Frobenius norm after the step is within 2^-22 relative of before (one float32 rounding per element,
    2^-24, and sums in float64); without it and with plain unclipped SGD no core's norm has shrunk (|A + lr G|^2 = |A|^2 + lr^2 |G|^2)"""
    D, cap, L, _, l = lc[0]
    case = R.StepCase(lc)
    ctx = new_ctx(case.cores, l, D, L)
    n0 = [float(np.sqrt((c * c).sum())) for c in case.cores]
    for objective in R.OBJECTIVES:
        for name in R.STEP_OPTIMS:
            ctx.set_cores(A.as32(case.cores), l)
            configure(ctx, name)
            ctx.nll_step(case.X, case.y(objective), case.S, case.lr((objective, name, True)), R.WD, True)
            n1 = [float(np.sqrt((c * c).sum())) for c in dev_cores(ctx)]
            worst = max(abs(a / b - 1.0) for a, b in zip(n1, n0))
            print('%s %s %s: norms within %.2e' % (N.likelihood_id(lc), objective, name, worst))
            assert worst <= 2.0 ** -22, (objective, name, worst)
        ctx.set_cores(A.as32(case.cores), l)
        configure(ctx, 'sgd')
        ctx.nll_step(case.X, case.y(objective), case.S, case.lr((objective, 'sgd', False)), 0.0, False)
        n1 = [float(np.sqrt((c * c).sum())) for c in dev_cores(ctx)]
        assert all(a >= b * (1.0 - 2.0 ** -22) for a, b in zip(n1, n0)) and max(a / b for a, b in zip(n1, n0)) > 1.0 + 1e-6
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------
# 5. the short run
# ---------------------------------------------------------------------------------------------------------------
def test_short_run():
    setup = R.training_run_setup()
    lev, lab, X, cores, S, idx = setup
    ref_vals, _, ref = R.training_run(False, setup)
    run = R.RUN
    ctx = new_ctx(cores, run['l'], run['D'], run['L'])
    ctx.dataset_attach(X, lab)
    configure(ctx, 'sgd')
    vals = ctx.nll_train_indices(idx, run['batch'], True, S, run['lr'], run['wd'], True)
    err, bound = R.trajectory_deviation(vals[:, 0], ref_vals), R.trajectory_bound()
    step = R.step_deviation(dev_cores(ctx), ref.cores, cores)
    ctx.close()
    print('short run: values %s\n  against the float64 trajectory %.2e (bound %.0e); cores after 20 steps %.2e of the move'
          % (np.round(vals[:, 0], 4), err, bound, step))
    assert vals.shape == (run['steps'], 4) and (vals[:, 2:] == 0).all()
    assert vals[-1, 0] < vals[0, 0]
    assert err <= bound, (err, bound)


# ---------------------------------------------------------------------------------------------------------------
# 6. the guard
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['sgd_clip_mom', 'adam'])
def test_guard_stops_at_the_first_bad_step(name):
    """the label core's slice of class 1 is zero, so f_1 == 0 exactly; three batches of 17, only the middle one holds a sample
    labelled 1.  This provokes a non-finite value on purpose, not a fault: every kernel runs to its end."""
    case = (2, 5, 3, 17, 5)
    D, cap, L, _, l = case
    cores = N.build_chain(case)
    cores[l][..., 1] = 0.0
    lev, lab, X = N.draw_batch(case, N.build_chain(case), 51)
    lab = np.where(lab == 1, 0, lab).astype(np.int32)
    lab[17 + 4] = 1
    S = grid_metric(D)
    a, c = new_ctx(cores, l, D, L), new_ctx(cores, l, D, L)
    for ctx in (a, c):
        ctx.dataset_attach(X, lab)
        configure(ctx, name)
    idx = np.arange(51, dtype=np.int32)
    with pytest.raises(_hip.TnmlError, match='step 1 of 3 saw 1 samples') as ei:
        a.nll_train_indices(idx, 17, True, S, renorm=True, **HYPER)
    assert ei.value.code == NONFINITE
    vals = ei.value.values
    v0 = c.nll_step(X[:17], lab[:17], S, renorm=True, **HYPER)
    assert vals.shape == (3, 4) and vals[0].tobytes() == v0.tobytes() and v0[3] == 0
    assert vals[1, 2] == 1 and int(vals[1, 3]) == BAD_BATCH | NOT_APPLIED and np.isfinite(vals[1, 1])
    assert int(vals[2, 3]) & NOT_APPLIED and vals[2, 2] == 0 and np.isfinite(vals[2, 0])      # a good batch, and still not applied
    assert same(a.get_cores()[0], c.get_cores()[0])
    # a following call on good batches works, from the same state (Adam's t counts the applied step alone)
    good = np.concatenate([idx[:17], idx[34:]])
    va = a.nll_train_indices(good, 17, True, S, renorm=True, **HYPER)
    vc = c.nll_train_indices(good, 17, True, S, renorm=True, **HYPER)
    assert va.tobytes() == vc.tobytes() and (va[:, 3] == 0).all()
    assert same(a.get_cores()[0], c.get_cores()[0])
    a.close()
    c.close()


def test_guard_on_an_uncalibrated_chain():
    """N = 784 as Network() draws it before the calibration, every core times 0.6: f is far below float32, every cotangent is
    infinite -- the cores are untouched bit for bit, whatever the steps of the call"""
    (Nn, D, L, l), cores = N.raw_long_chain(2, 0, 0.6)
    ctx = new_ctx(cores, l, D, L)
    configure(ctx, 'sgd_clip_mom')
    _, phi, w = N.grid(N.K, D)
    rng = np.random.default_rng(5)
    X = phi[rng.integers(0, N.K, (16, Nn))].astype(np.float32)
    y = np.zeros(16, dtype=np.int32)
    ctx.dataset_attach(X, y)
    before = ctx.get_cores()[0]
    slots0, lab0 = ctx.core_slots()
    with pytest.raises(_hip.TnmlError, match='step 0 of 2 saw 8 samples') as ei:
        ctx.nll_train_indices(np.arange(16), 8, True, N.gram(phi, w), 1e-2, 0.0, True)
    assert ei.value.code == NONFINITE and (ei.value.values[:, 3].astype(int) & NOT_APPLIED).all()
    assert _code(lambda: ctx.nll_step(X, y, N.gram(phi, w), 1e-2, 0.0, False)) == NONFINITE
    assert same(ctx.get_cores()[0], before)
    slots1, lab1 = ctx.core_slots()
    assert slots0.tobytes() == slots1.tobytes() and lab0.tobytes() == lab1.tobytes()
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------
# 7. refusals and state
# ---------------------------------------------------------------------------------------------------------------
SWEEP = (1e-2, 1e-3, True, 'softmax', 'full_cross_ent', 0.1, 'fixed')


def test_refusals(monkeypatch):
    Nn, D, L, M = 6, 2, 3, 4
    case_rng = np.random.default_rng(68)
    shapes = N.shapes_of(Nn, D, L, [M] * (Nn - 1), 2)
    cores = [case_rng.random(s).astype(np.float32) + 0.1 for s in shapes]
    _, phi, w = N.grid(N.K, D)
    X = phi[case_rng.integers(0, N.K, (10, Nn))].astype(np.float32)
    y = case_rng.integers(0, L, 10).astype(np.int32)
    S = N.gram(phi, w)
    ctx = _hip.Context(Nn, D, L, M, 64)
    ctx.set_any_position(True)
    lib, f32p, i32p, f64p = _hip.lib(), C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_double)
    Xp, yp, Sp = X.ctypes.data_as(f32p), y.ctypes.data_as(i32p), S.ctypes.data_as(f64p)
    idx = np.array([0, 1, 9, 1], dtype=np.int32)
    ip = idx.ctypes.data_as(i32p)
    out = np.zeros(16)
    op = out.ctypes.data_as(f64p)
    assert lib.tnml_nll_step(ctx._h, Xp, yp, 10, Sp, 0.1, 0.0, 1, op) == STATE                     # cores never set
    assert lib.tnml_nll_train_indices(ctx._h, ip, 4, 2, 1, Sp, 0.1, 0.0, 1, op) == STATE           # no dataset
    ctx.set_cores(cores, 2)
    ctx.dataset_attach(X, y)
    counters = ctx.counters()
    assert lib.tnml_nll_step(None, Xp, yp, 10, Sp, 0.1, 0.0, 1, op) == ARG
    assert lib.tnml_nll_step(ctx._h, None, yp, 10, Sp, 0.1, 0.0, 1, op) == ARG
    assert lib.tnml_nll_step(ctx._h, Xp, yp, 10, Sp, 0.1, 0.0, 1, None) == ARG
    assert lib.tnml_nll_step(ctx._h, Xp, yp, 0, Sp, 0.1, 0.0, 1, op) == ARG                        # an empty batch
    assert lib.tnml_nll_step(ctx._h, Xp, yp, 10, Sp, 0.1, 0.0, 2, op) == ARG                       # renorm 2
    assert 'renorm' in lib.tnml_last_error().decode()
    assert lib.tnml_nll_train_indices(ctx._h, None, 4, 2, 1, Sp, 0.1, 0.0, 1, op) == ARG
    assert lib.tnml_nll_train_indices(ctx._h, ip, 4, 2, 1, Sp, 0.1, 0.0, 1, None) == ARG
    assert lib.tnml_nll_train_indices(ctx._h, ip, 0, 2, 1, Sp, 0.1, 0.0, 1, op) == ARG
    assert lib.tnml_nll_train_indices(ctx._h, ip, 4, 0, 1, Sp, 0.1, 0.0, 1, op) == ARG             # batch < 1
    assert lib.tnml_nll_train_indices(ctx._h, ip, 4, 2, 1, Sp, 0.1, 0.0, -1, op) == ARG
    assert _code(lambda: ctx.nll_train_indices([0, 10], 2, True, S)) == ARG                       # a bad index
    assert _code(lambda: ctx.nll_train_indices([-1], 1, True, S)) == ARG
    assert _code(lambda: ctx.nll_step(X, np.full(10, L), S)) == ARG                               # a label outside [0, L)
    assert _code(lambda: ctx.nll_step(X, y, np.array([[1.0, 0.5], [0.25, 1.0]]))) == ARG          # a non-symmetric metric
    assert _code(lambda: ctx.nll_train_indices(idx, 2, True, np.array([[1.0, np.nan], [np.nan, 1.0]]))) == ARG
    assert _code(lambda: ctx.set_nll_overlap(2)) == ARG
    assert (out == 0).all() and same(ctx.get_cores()[0], cores)                                   # nothing was written
    assert ctx.counters() == counters                                               # nothing was launched
    # usable afterwards, index form against X form
    v1 = ctx.nll_train_indices([0, 1, 9], 3, True, S, 0.01, 0.0, True)[0]
    after = ctx.get_cores()[0]
    ctx.set_cores(cores, 2)
    v2 = ctx.nll_step(X[[0, 1, 9]], y[[0, 1, 9]], S, 0.01, 0.0, True)
    assert v1.tobytes() == v2.tobytes() and same(after, ctx.get_cores()[0])
    ctx.close()
    # bond 65 refused, bond 64 taken
    rng = np.random.default_rng(7)
    ctx = _hip.Context(4, 2, 2, 65, 64)
    ctx.set_any_position(True)
    X4 = phi[rng.integers(0, N.K, (3, 4))].astype(np.float32)
    ctx.set_cores([rng.random(s).astype(np.float32) + 0.1 for s in N.shapes_of(4, 2, 2, [2, 65, 2], 1)], 1)
    with pytest.raises(_hip.TnmlError, match='bond 65') as ei:
        ctx.nll_step(X4, None, S)
    assert ei.value.code == ARG
    ctx.set_cores([(rng.random(s).astype(np.float32) + 0.1) / 8 for s in N.shapes_of(4, 2, 2, [2, 64, 2], 1)], 1)
    v = ctx.nll_step(X4, np.zeros(3, dtype=np.int32), S, 1e-3, 0.0, True)
    assert v[3] == 0 and np.isfinite(v[:2]).all()
    ctx.close()
    # a communicator attached
    from tensornetworkforml_amd import dist as tdist
    monkeypatch.setenv('TNML_FORCE_COMM', '1')
    ctx = _hip.Context(Nn, D, L, M, 64)
    ctx.set_cores([case_rng.random(s).astype(np.float32) for s in N.shapes_of(Nn, D, L, [M] * (Nn - 1), 0)], 0)
    tdist.attach_comm(ctx, 0, 1)
    assert _code(lambda: ctx.nll_step(X, y, S)) == STATE
    assert _code(lambda: ctx.nll_train_indices([0], 1, True, S)) == STATE
    ctx.close()


def test_context_state_after_a_step():
    """a sweep returns TNML_ERR_STATE after a step until a forward; the resident batch stays; a stale optimiser binding after
    compress is refused until optim_reset"""
    Nn, D, L, M, b = 12, 2, 2, 6, 100
    rng = np.random.default_rng(65)
    _, phi, w = N.grid(N.K, D)
    S = N.gram(phi, w)
    X = phi[rng.integers(0, N.K, (b, Nn))].astype(np.float32)
    y = rng.integers(0, L, b).astype(np.int32)
    shapes = N.shapes_of(Nn, D, L, [M] * (Nn - 1), 0)
    cores = [((rng.random(s) + 0.1) / (0.5 * s[0] * D + 0.8)).astype(np.float32) for s in shapes]
    ctx = _hip.Context(Nn, D, L, M, b)
    ctx.set_cores(cores, 0)
    ctx.set_input(X, y)
    ctx.forward()
    configure(ctx, 'sgd_clip_mom')
    v = ctx.nll_step(X[:70], y[:70], S, 1e-2, 0.0, True)
    assert v[3] == 0
    assert _code(lambda: ctx.sweep(False, Nn - 1, True, *SWEEP)) == STATE
    f = ctx.forward()
    assert np.array_equal(f, ctx.predict(X))                       # the resident batch is still there
    ctx.nll_step(X[:70], y[:70], S, 1e-2, 0.0, True)               # the state is still bound
    ctx.compress(3)
    assert _code(lambda: ctx.nll_step(X[:70], y[:70], S, 1e-2, 0.0, True)) == STATE
    assert 'tnml_optim_reset' in _hip.lib().tnml_last_error().decode()
    ctx.optim_reset()
    ctx.nll_step(X[:70], y[:70], S, 1e-2, 0.0, True)
    ctx.forward(want_f=False)
    ctx.sweep(False, Nn - 1, True, *SWEEP)
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------
# 8. Network level and the script
# ---------------------------------------------------------------------------------------------------------------
def test_network_methods(capsys):
    import tensornetworkforml_amd as pkg
    Nn, D, L, M, n = 16, 2, 2, 4, 230
    np.random.seed(3)
    data, label = gen.create_dataset(n, 4, 0.3)
    lev = np.round(np.clip(data.reshape(n, -1), 0.0, 1.0) * 255).astype(np.int32)                 # on the grid of 256 levels
    pix = (lev / 255.0).astype(np.float32)
    X = gen.psi(lev / 255.0, D)
    net = pkg.Network(N=Nn, M=M, D=D, L=L, normalize=True, calibration_X=X[:16], act_fn='softmax', loss_fn='full_cross_ent', T=1.0, trunc='fixed')
    net.attach_dataset(pix, label, pixels=True)
    start, _, lp = net._ctx.get_cores()
    S = grid_metric(D)
    twin = _hip.Context(Nn, D, L, M, 64)
    twin.set_cores(start, lp)
    twin.dataset_attach(pix, label, 'pixels')
    # nll_step: dataset indices, then images with the sum log w term
    nll, logz = net.nll_step(np.arange(50), lr=0.01)
    t = twin.nll_train_indices(np.arange(50), 50, True, S, 0.01, 0.0, True)[0]
    assert (nll, logz) == (t[0], t[1])
    nll, logz = net.nll_step(lev[50:90], label[50:90], lr=0.01, weight_dec=1e-3, renorm=False)
    t = twin.nll_step(X[50:90].astype(np.float32), label[50:90], S, 0.01, 1e-3, False)
    assert logz == t[1] and nll == pytest.approx(t[0] + Nn * np.log(256.0), rel=1e-12)
    assert same(net._ctx.get_cores()[0], twin.get_cores()[0])
    assert all(np.array_equal(h.astype(np.float32), c) for h, c in zip(net.As and net._host_cores, twin.get_cores()[0]))
    # train_generative over two epochs against the `_hip`-level calls: 180 training samples in batches of 50 -> 50, 50, 50, 30
    tr = gen.IndexLoader(np.arange(180), 50, shuffle=False)
    va = gen.IndexLoader(np.arange(180, n), 25, shuffle=False)
    val_nll, hist = net.train_generative(tr, va, lr=0.01, n_epochs=2, weight_dec=1e-3, optimizer='sgd', momentum=0.9)
    out = capsys.readouterr().out
    assert '--- TRAINING PROCEDURE ---' in out and 'Epoch 1/2 - train NLL' in out and 'val NLL' in out and 'val accuracy' in out
    assert hist.shape == (2, 4) and len(val_nll) == 2 and np.isfinite(hist).all()
    twin.optim_config('sgd', momentum=0.9, clip=True)
    for epoch in range(2):
        v = twin.nll_train_indices(np.arange(180), 50, True, S, 0.01, 1e-3, True)
        assert np.array_equal(hist[epoch], v[:, 0])
        ev = np.array([twin.nll_eval_indices(idx, True, S)[0] for idx in va])
        assert val_nll[epoch] == pytest.approx(float(ev.mean()), rel=1e-12)
    assert same(net._ctx.get_cores()[0], twin.get_cores()[0])
    assert hist[1].mean() < hist[0].mean()
    # a forward makes sweeping possible again
    f = net.forward(X[:64])
    net.sweep(X[:64], label[:64], f, 1e-2, 1e-3)
    twin.close()


def test_script_option(tmp_path, capsys):
    from tensornetworkforml_amd import training_diagonals
    np.random.seed(11)
    val_nll, hist = training_diagonals.main(['--resident', '--objective', 'nll', '--n_samples', '1000', '--linear_dim', '4', '--M', '4', '--n_epochs', '2',
                                             '--n_train_batch', '4', '--lr', '0.01', '--L2_decay', '0', '--out', str(tmp_path / 'model.dat')])
    out = capsys.readouterr().out
    assert 'Epoch 1/2 - train NLL' in out and 'validation NLL per epoch' in out
    assert len(val_nll) == 2 and np.isfinite(val_nll).all() and hist.shape == (2, 4) and np.isfinite(hist).all() and (tmp_path / 'model.dat').exists()
