"""Gradient training on the GPU (include/tnml.h, tnml_optim_config / tnml_gd_train_indices / tnml_gd_step),
through `_hip.Context` and `Network`.

  1  one step against the reference   SGD with the clip on the shared cases of tests/gradient_step_reference.py (N in {2, 3, 17},
                                      the label at both ends and inside, uniform and ragged bonds, b in {1, 70}) for the rows
                                      below; at (2, 20, 2) all nine activation / loss pairs
  2  several steps with state         three consecutive steps, SGD with momentum 0.9 and Adam, at (2, 20, 2) and (3, 7, 3)
  3  bit-equalities                   chunk 64 against the default chunk; one call of four steps against four calls; the same call
                                      on two contexts; gd_step on dataset_read against gd_train_indices; lr = 0; slot padding
  4  state                            sweep refused until a forward; forward = predict; the state rule after a sweep; optim_config
                                      alone moves nothing
  5  a short training run             per-step correct counts against the float64 trajectory
  6  Network level                    gradient_step, train_gradient against the `_hip`-level calls, pickling
  7  refusals                         each of include/tnml.h, the context usable afterwards; TNML_ERR_NONFINITE
  8  reuse                            a larger and a smaller batch, other cores and bonds, the other optimiser on one context

The measure of 1, 2 and 8 is max |dA_dev - dA_ref| over all cores relative to max |dA_ref|, dA = A_after - A_before, with lr chosen
per case so that max |dA_ref| >= 0.1 max |A| (tests/test_gradient_step_host.py asserts this and every other condition on the inputs
with the reference alone).  Tolerances: the rule of tests/test_core_grad_gpu.py, ten times the worst value observed on an MI355X
against the float64 reference, rounded up to one digit.  Worst observed:
    (D, cap, L)     SGD, one step      bound       three steps    momentum 0.9   bound     Adam        bound
    (2, 5, 3)       3.80e-07           4e-6        (2, 20, 2)     1.06e-06       2e-5      9.40e-07    1e-5
    (2, 20, 2)      6.55e-06           7e-5        (3, 7, 3)      1.29e-06       2e-5      9.47e-07    1e-5
    (2, 33, 2)      1.11e-06           2e-5
    (2, 50, 10)     7.16e-07           8e-6        reuse (test 8) 5.14e-07       6e-6
    (3, 7, 3)       7.73e-07           8e-6
    (8, 16, 17)     7.28e-07           8e-6
One bound for SGD exceeds 2e-5: (2, 20, 2), the row of the nine activation / loss pairs.  Per pair the worst values are
linear/MSE 1.39e-06, linear/cross_entropy 5.50e-07, linear/full_cross_ent 4.55e-06, sigmoid/MSE 5.10e-07, sigmoid/cross_entropy
3.22e-07, sigmoid/full_cross_ent 5.85e-07, softmax/MSE 4.00e-06, softmax/cross_entropy 6.14e-07, softmax/full_cross_ent 6.55e-06:
the responsible terms are in the loss derivative, not in the chains or the update.  1 / (z + 1e-4) of full_cross_ent passes the
error of the activated output on divided by |z| (the cases admit |z| down to 0.05: a gain of up to 20 on the few 1e-7 of a float32
f), and the device's softmax uses the fast exponential (__expf) against the float64 exp of the reference; softmax/MSE was not
separated further.  Every other row, and the pairs of this row without softmax and full_cross_ent, stay below 2e-6.
Adam was expected to be looser than SGD by up to max|G| / eps = 100, the gain of m / (sqrt(v) + eps) on an error of G at an element
of size eps.  It is not: that gain needs an ABSOLUTE error of the order of 1e-6 max|G| on an element a hundred times smaller than
max|G|, and a float32 element of G is wrong relative to its own terms sum_s |P x Q cot|, which are small where the element is
small.  Every test prints the worst values it observed.
"""
import ctypes as C
import os
import pickle
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import gradient_step_reference as R                                # noqa: E402
from input_grad_reference import ragged_bonds, scaled_cores       # noqa: E402
from tensornetworkforml_amd import _hip                           # noqa: E402
from tensornetworkforml_amd import data_generator as gen          # noqa: E402

pytestmark = pytest.mark.gpu

ARG, STATE, NONFINITE = -1, -2, -7
# ten times the observed value, rounded up to one digit (see the head of the file)
SGD_TOL = {(2, 5, 3): 4e-6, (2, 20, 2): 7e-5, (2, 33, 2): 2e-5, (2, 50, 10): 8e-6, (3, 7, 3): 8e-6, (8, 16, 17): 8e-6}
MOMENTUM_TOL = {(2, 20, 2): 2e-5, (3, 7, 3): 2e-5}
ADAM_TOL = {(2, 20, 2): 1e-5, (3, 7, 3): 1e-5}
REUSE_TOL = 6e-6


def _code(call):
    with pytest.raises(_hip.TnmlError) as ei:
        call()
    return ei.value.code


def features(rng, b, N, D):
    return R._features(rng, b, N, D)


def cores_for(N, D, L, cap, l, rng, ragged, X=None):
    """scaled_cores in float32, calibrated on X (f of order 1) when X is given"""
    bond = ragged_bonds(N, cap, rng) if ragged else [cap] * (N - 1)
    base = scaled_cores(N, D, L, bond, l, rng)
    if X is not None:
        med = np.median(np.abs(R.forward64(base, l, X.astype(np.float64))))
        base = [c * med ** (-1.0 / N) for c in base]
    return [c.astype(np.float32) for c in base]


def context_M(row):
    """The smallest M whose bond capacity max(M, D min(L, M)) holds the bonds of a row.  (At (8, 16, 17) M = 16 itself would have
    the capacity 128, for which the prediction chain has no LDS tile; M = 2 has the capacity 16.  The slots are then wider than
    the cores wherever the capacity exceeds the row's largest bond.)"""
    D, cap, L = row
    return next(M for M in range(1, cap + 1) if max(M, D * min(L, M)) >= cap)


def as64(a):
    return [c.astype(np.float64) for c in a]


def step_error(after, before, ref_after):
    """max |dA_dev - dA_ref| over all cores relative to max |dA_ref|"""
    scale = max(np.abs(r - b.astype(np.float64)).max() for r, b in zip(ref_after, before))
    err = max(np.abs((a.astype(np.float64) - b.astype(np.float64)) - (r - b.astype(np.float64))).max() for a, b, r in zip(after, before, ref_after))
    return err / scale


def same_cores(G0, G1):
    return len(G0) == len(G1) and all(np.array_equal(a, c) for a, c in zip(G0, G1))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------
# 1. one step against the reference
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('row', R.ROWS, ids=lambda r: 'D%d-cap%d-L%d' % r)
def test_one_step_against_the_reference(row):
    D, cap, L = row
    worst, ctxs, by_pair = 0.0, {}, {}
    for case in R.row_cases(row):
        N = case['N']
        if N not in ctxs:
            ctxs[N] = _hip.Context(N, D, L, context_M(row), 70)
            ctxs[N].optim_config('sgd', clip=True)
        ctx = ctxs[N]
        for act, loss in R.pairs_of(row):
            lr = R.case_lr(case, act, loss)
            ref = R.GradientStepReference(as64(case['cores']), case['l'])
            info = ref.step(case['X'], case['y'], lr, R.WD, act, loss, R.T_CASES)
            ctx.set_cores(case['cores'], case['l'])
            correct, abs_sum, nonfinite = ctx.gd_step(case['X'], case['y'], lr, R.WD, act, loss, R.T_CASES)
            after, bond, lp = ctx.get_cores()
            assert lp == case['l'] and [a.shape for a in after] == [c.shape for c in case['cores']]
            assert nonfinite == 0 and correct == info['correct'] and abs(abs_sum - info['abs_sum']) <= 1e-4 * max(info['abs_sum'], 1.0)
            err = step_error(after, case['cores'], ref.cores)
            worst, by_pair[act, loss] = max(worst, err), max(by_pair.get((act, loss), 0.0), err)
    for ctx in ctxs.values():
        ctx.close()
    print('gradient step D %d cap %d L %d: %.2e of max|dA|' % (D, cap, L, worst))
    if len(by_pair) > 1:
        print('    per pair: ' + ', '.join('%s/%s %.2e' % (a, lo, v) for (a, lo), v in by_pair.items()))
    assert worst <= SGD_TOL[row], worst


# ---------------------------------------------------------------------------------------------------------------
# 2. several steps with state
# ---------------------------------------------------------------------------------------------------------------
def three_step_lr(case, opt, unit, act, loss):
    """The learning rate of a three-step case, from the reference alone: the first rung of unit * 0.01 * 1.15^k whose float64
    trajectory moves the cores by between a tenth of max|A| and max|A| (a larger one may leave the basin of the multilinear
    model, where any error is amplified without bound).  -> (lr, the reference after its three steps)"""
    c64 = as64(case['cores'])
    amax = max(np.abs(c).max() for c in c64)
    for k in range(40):
        lr = R.f32(unit * 0.01 * 1.15 ** k)
        ref = R.GradientStepReference(c64, case['l'], **opt)
        for _ in range(3):
            ref.step(case['X'], case['y'], lr, R.WD, act, loss, R.T_CASES)
        move = max(np.abs(r - c).max() for r, c in zip(ref.cores, c64))
        if np.isfinite(move) and 0.1 * amax <= move <= amax:
            return lr, ref
    raise AssertionError('no learning rate moves the cores by 0.1 .. 1 max|A|')


@pytest.mark.parametrize('kind', ['momentum', 'adam'])
@pytest.mark.parametrize('row', [(2, 20, 2), (3, 7, 3)], ids=lambda r: 'D%d-cap%d-L%d' % r)
def test_three_steps_with_state(row, kind):
    """Three steps on one batch of 70, linear / MSE, weight decay on.  Momentum 0.9 runs without the clip (its decision at the
    later steps is not covered by the conditions on the inputs), in units of max|A| over the largest |d| of the first step; Adam,
    whose step per element is at most lr, in units of max|A|, with eps = 1e-2 max|G_ref| of the first step."""
    D, cap, L = row
    worst, ctxs = 0.0, {}
    act, loss = 'linear', 'MSE'
    for case in R.row_cases(row):
        if case['b'] != 70:
            continue
        N = case['N']
        c64 = as64(case['cores'])
        amax = max(np.abs(c).max() for c in c64)
        probe = R.GradientStepReference(c64, case['l'], clip=False)
        info = probe.step(case['X'], case['y'], 1.0, R.WD, act, loss, R.T_CASES)
        if kind == 'momentum':
            opt = dict(kind='sgd', momentum=0.9, clip=False)
            unit = amax / max(np.abs(a - c).max() for a, c in zip(probe.cores, c64))
        else:
            opt = dict(kind='adam', eps=1e-2 * max(np.abs(g).max() for g in info['G']), clip=False)
            unit = amax
        lr, ref = three_step_lr(case, opt, unit, act, loss)
        if N not in ctxs:
            ctxs[N] = _hip.Context(N, D, L, context_M(row), 70)
        ctx = ctxs[N]
        ctx.set_cores(case['cores'], case['l'])
        ctx.optim_config(opt['kind'], momentum=opt.get('momentum', 0.0), eps=opt.get('eps', 1e-8), clip=False)
        for _ in range(3):
            ctx.gd_step(case['X'], case['y'], lr, R.WD, act, loss, R.T_CASES)
        worst = max(worst, step_error(ctx.get_cores()[0], case['cores'], ref.cores))
    for ctx in ctxs.values():
        ctx.close()
    print('three steps, %s, D %d cap %d L %d: %.2e of max|dA|' % (kind, D, cap, L, worst))
    assert worst <= (MOMENTUM_TOL if kind == 'momentum' else ADAM_TOL)[row], worst


# ---------------------------------------------------------------------------------------------------------------
# 3. bit-equalities
# ---------------------------------------------------------------------------------------------------------------
HYPER = (0.05, 1e-2, 'softmax', 'full_cross_ent', 1.0)          # lr, weight_dec, act_fn, loss_fn, T


@pytest.mark.parametrize('D,cap,L,l,kind', [(2, 20, 2, 0, 'momentum'), (2, 5, 3, 4, 'adam'), (3, 7, 3, 8, 'sgd')])
def test_bit_equalities(D, cap, L, l, kind):
    N, n = 9, 120
    rng = np.random.default_rng(31 + D)
    data = features(rng, n, N, D)
    labels = rng.integers(0, L, n).astype(np.int32)
    cores = cores_for(N, D, L, cap, l, rng, True, data)
    opt = dict(momentum=dict(kind='sgd', momentum=0.9, clip=True), adam=dict(kind='adam', eps=1e-3, clip=False), sgd=dict(kind='sgd', clip=True))[kind]

    def fresh():
        ctx = _hip.Context(N, D, L, cap, 64)
        ctx.set_cores(cores, l)
        ctx.dataset_attach(data, labels, 'features')
        ctx.optim_config(**opt)
        return ctx

    a, c = fresh(), fresh()
    # chunk 64 against the default chunk, two steps each so that the state takes part
    c.set_core_grad_chunk(64)
    for b in (70, 200):
        idx = rng.integers(0, n, b)
        for _ in range(2):
            ma = a.gd_train_indices(idx, b, *HYPER)
            mc = c.gd_train_indices(idx, b, *HYPER)
            assert ma[0, 0] == mc[0, 0] and ma[0, 2] == mc[0, 2] == 0 and abs(ma[0, 1] - mc[0, 1]) <= 1e-9 * ma[0, 1]
        assert same_cores(a.get_cores()[0], c.get_cores()[0]), b
    c.set_core_grad_chunk(0)
    # one call of four steps with a ragged last batch against four calls; the same call from the same state on two contexts
    idx = rng.integers(0, n, 250)
    m1 = a.gd_train_indices(idx, 70, *HYPER)
    m2 = np.concatenate([c.gd_train_indices(idx[k:k + 70], 70, *HYPER) for k in range(0, 250, 70)])
    assert m1.shape == (4, 3) and np.array_equal(m1, m2)
    assert same_cores(a.get_cores()[0], c.get_cores()[0])
    assert np.array_equal(a.gd_train_indices(idx, 70, *HYPER), c.gd_train_indices(idx, 70, *HYPER))
    assert same_cores(a.get_cores()[0], c.get_cores()[0])
    # a host batch read from the dataset against the index call
    idx = np.concatenate([rng.integers(0, n, 90), [3, 3, 3, n - 1, 0]])
    mi = a.gd_train_indices(idx, idx.size, *HYPER)[0]
    mx = c.gd_step(c.dataset_read(idx), labels[idx], *HYPER)
    assert tuple(mi) == tuple(float(v) for v in mx)
    assert same_cores(a.get_cores()[0], c.get_cores()[0])
    # lr = 0 leaves every core as it is, bit for bit
    before = a.get_cores()[0]
    a.gd_train_indices(idx, 50, 0.0, 0.0, *HYPER[2:])
    assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(before, a.get_cores()[0]))
    # the floats of every slot behind its core, and of the label buffer behind the label core, are untouched
    slots0, lab0 = a.core_slots()
    a.gd_train_indices(idx, 50, *HYPER)
    slots1, lab1 = a.core_slots()
    moved = 0
    for i, core in enumerate(before):
        if i == l:
            assert np.array_equal(bits(lab0[core.size:]), bits(lab1[core.size:]))
            moved += int((bits(lab0[:core.size]) != bits(lab1[:core.size])).sum())
        else:
            assert np.array_equal(bits(slots0[i, core.size:]), bits(slots1[i, core.size:])), i
            moved += int((bits(slots0[i, :core.size]) != bits(slots1[i, :core.size])).sum())
    assert np.array_equal(bits(slots0[l]), bits(slots1[l]))                  # (the slot of the label site is not in use)
    assert moved > 0.9 * sum(c_.size for c_ in before)
    a.close()
    c.close()


# ---------------------------------------------------------------------------------------------------------------
# 4. state
# ---------------------------------------------------------------------------------------------------------------
SWEEP = (1e-2, 1e-3, True, 'softmax', 'full_cross_ent', 0.1, 'fixed')


def test_context_state_after_a_step():
    N, D, L, M, b = 12, 2, 2, 6, 100
    rng = np.random.default_rng(65)
    X, y = features(rng, b, N, D), rng.integers(0, L, b)
    cores = cores_for(N, D, L, M, 0, rng, False, X)
    ctx = _hip.Context(N, D, L, M, b)
    ctx.set_cores(cores, 0)
    ctx.set_input(X, y)
    ctx.forward()
    # optim_config alone moves nothing
    other = features(rng, 150, N, D)
    cot = rng.standard_normal((L, 150)).astype(np.float32)
    ig0, cg0 = ctx.input_grad(other, cot), ctx.core_grad(other, cot)
    ctx.optim_config('adam', eps=1e-3, clip=False)
    ctx.optim_config('sgd', momentum=0.9, clip=True)
    ig1, cg1 = ctx.input_grad(other, cot), ctx.core_grad(other, cot)
    assert np.array_equal(ig0[0], ig1[0]) and np.array_equal(ig0[1], ig1[1]) and same_cores(cg0[0], cg1[0]) and np.array_equal(cg0[1], cg1[1])
    assert same_cores(ctx.get_cores()[0], cores)
    # a step: the resident batch stays, its f and environments are stale
    ctx.gd_step(other, rng.integers(0, L, 150), *HYPER)
    assert _code(lambda: ctx.sweep(False, N - 1, True, *SWEEP)) == STATE
    assert not same_cores(ctx.get_cores()[0], cores)
    f = ctx.forward()
    assert np.array_equal(f, ctx.predict(X))
    ctx.sweep(False, N - 1, True, *SWEEP)
    assert ctx.l_pos == N - 1
    # the state belongs to l_pos = 0: refused until optim_reset; plain SGD has none
    for opt in (dict(kind='sgd', momentum=0.9), dict(kind='adam', eps=1e-3, clip=False)):
        ctx.set_cores(cores, 0)
        ctx.set_input(X, y)
        ctx.optim_config(**opt)
        ctx.gd_step(other, np.zeros(150, dtype=np.int32), *HYPER)
        ctx.forward(want_f=False)
        ctx.sweep(False, N - 1, True, *SWEEP)
        with pytest.raises(_hip.TnmlError, match='tnml_optim_reset') as ei:
            ctx.gd_step(other, np.zeros(150, dtype=np.int32), *HYPER)
        assert ei.value.code == STATE
        ctx.optim_reset()
        ctx.gd_step(other, np.zeros(150, dtype=np.int32), *HYPER)
        ctx.forward(want_f=False)
        ctx.sweep(True, N - 1, True, *SWEEP)
        assert _code(lambda: ctx.gd_step(other, np.zeros(150, dtype=np.int32), *HYPER)) == STATE
        ctx.optim_config('sgd', momentum=0.0, clip=True)
        ctx.gd_step(other, np.zeros(150, dtype=np.int32), *HYPER)
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------
# 5. a short training run
# ---------------------------------------------------------------------------------------------------------------
def test_short_training_run():
    X, y, cores, idx = R.training_run_setup()
    correct_ref, acc0, acc1, _ = R.training_run_reference()
    run = R.RUN
    ctx = _hip.Context(run['N'], run['D'], run['L'], run['M'], 64)
    ctx.set_cores(cores, 0)
    ctx.dataset_attach(X, y, 'features')
    ctx.optim_config('sgd', clip=True)
    met = ctx.gd_train_indices(idx, run['batch'], run['lr'], run['wd'], run['act_fn'], run['loss_fn'], run['T'])
    acc_dev = ctx.eval_indices(np.arange(run['n']), run['act_fn'], run['T'])[0] / run['n']
    ctx.close()
    print('training run: correct per step, device %s, float64 %s; accuracy %.3f -> %.3f (float64 %.3f)'
          % ([int(v) for v in met[:, 0]], correct_ref, acc0, acc_dev, acc1))
    assert met.shape == (run['steps'], 3) and (met[:, 2] == 0).all()
    assert np.abs(met[:, 0] - np.array(correct_ref)).max() <= 2


# ---------------------------------------------------------------------------------------------------------------
# 6. Network level
# ---------------------------------------------------------------------------------------------------------------
def test_network_methods(capsys):
    import tensornetworkforml_amd as pkg
    N, D, L, M, n = 16, 2, 2, 4, 230
    np.random.seed(3)
    rng = np.random.default_rng(70)
    data, label = gen.create_dataset(n, 4, 0.3)
    pix = np.clip(data.reshape(n, -1), 0.0, 1.0).astype(np.float32)
    X = gen.psi(pix.astype(np.float64), D)
    net = pkg.Network(N=N, M=M, D=D, L=L, normalize=True, calibration_X=X[:16], act_fn='softmax', loss_fn='full_cross_ent', T=1.0, trunc='fixed')
    net.attach_dataset(pix, label, pixels=True)
    start, _, lp = net._ctx.get_cores()
    twin = _hip.Context(N, D, L, M, 64)
    twin.set_cores(start, lp)
    twin.dataset_attach(pix, label, 'pixels')
    # gradient_step: dataset indices, then a host batch
    acc, mae = net.gradient_step(np.arange(50), lr=0.05)
    m = twin.gd_train_indices(np.arange(50), 50, 0.05, 0.0, 'softmax', 'full_cross_ent', 1.0)[0]
    assert (acc, mae) == (m[0] / 50, m[1] / (50 * L)) and 0.0 <= acc <= 1.0
    acc, mae = net.gradient_step(X[50:90].astype(np.float32), label[50:90], lr=0.05, weight_dec=1e-3)
    m = twin.gd_step(X[50:90].astype(np.float32), label[50:90], 0.05, 1e-3, 'softmax', 'full_cross_ent', 1.0)
    assert (acc, mae) == (m[0] / 40, m[1] / (40 * L))
    assert same_cores(net._ctx.get_cores()[0], twin.get_cores()[0])
    # As follows the device
    As = net.As
    dev = net._ctx.get_cores()[0]
    assert len(As) == N and all(np.array_equal(h.astype(np.float32), c) for h, c in zip(net._host_cores, dev))
    # train_gradient over two epochs against the `_hip`-level calls: 180 training samples in batches of 50 -> 50, 50, 50, 30
    tr = gen.IndexLoader(np.arange(180), 50, shuffle=False)
    va = gen.IndexLoader(np.arange(180, n), 25, shuffle=False)
    val_acc, hist = net.train_gradient(tr, va, lr=0.05, n_epochs=2, weight_dec=1e-3, optimizer='sgd', momentum=0.9)
    out = capsys.readouterr().out
    assert '--- TRAINING PROCEDURE ---' in out and 'Epoch 1/2 - train accuracy' in out and 'val accuracy' in out
    assert hist.shape == (2, 2, 4) and len(val_acc) == 2
    twin.optim_config('sgd', momentum=0.9, clip=True)
    for epoch in range(2):
        m = np.concatenate([twin.gd_train_indices(np.arange(150), 50, 0.05, 1e-3, 'softmax', 'full_cross_ent', 1.0),
                            twin.gd_train_indices(np.arange(150, 180), 30, 0.05, 1e-3, 'softmax', 'full_cross_ent', 1.0)])
        sizes = np.array([50, 50, 50, 30])
        assert np.array_equal(hist[epoch, 0], m[:, 0] / sizes) and np.array_equal(hist[epoch, 1], m[:, 1] / (sizes * L))
        v = [twin.eval_indices(idx, 'softmax', 1.0)[0] / len(idx) for idx in va]
        assert val_acc[epoch] == np.mean(v)
    final = twin.get_cores()[0]
    assert same_cores(net._ctx.get_cores()[0], final)
    # a pickled and restored network holds the updated cores
    back = pickle.loads(pickle.dumps(net))
    f0 = np.asarray(back.predict(X[:20]).elem)
    assert np.array_equal(f0.astype(np.float32), twin.predict(X[:20].astype(np.float32)))
    assert same_cores(back._ctx.get_cores()[0], final)
    # a forward makes sweeping possible again
    f = net.forward(X[:64])
    net.sweep(X[:64], label[:64], f, 1e-2, 1e-3)
    twin.close()


# ---------------------------------------------------------------------------------------------------------------
# 7. refusals
# ---------------------------------------------------------------------------------------------------------------
def test_refusals(monkeypatch):
    N, D, L, M = 6, 2, 3, 4
    rng = np.random.default_rng(68)
    ctx = _hip.Context(N, D, L, M, 64)
    X = features(rng, 10, N, D)
    y = rng.integers(0, L, 10).astype(np.int32)
    lib, f32p, i32p = _hip.lib(), C.POINTER(C.c_float), C.POINTER(C.c_int32)
    Xp, yp = X.ctypes.data_as(f32p), y.ctypes.data_as(i32p)
    idx = np.array([0, 1, 9, 1], dtype=np.int32)
    ip = idx.ctypes.data_as(i32p)
    assert lib.tnml_gd_step(ctx._h, Xp, yp, 10, 0.1, 0.0, 2, 2, 1.0, None) == STATE              # cores never set
    assert lib.tnml_gd_train_indices(ctx._h, ip, 4, 2, 0.1, 0.0, 2, 2, 1.0, None) == STATE       # no dataset
    cores = cores_for(N, D, L, M, 2, rng, False, X)
    ctx.set_cores(cores, 2)
    ctx.dataset_attach(X, y, 'features')
    assert lib.tnml_gd_step(ctx._h, None, yp, 10, 0.1, 0.0, 2, 2, 1.0, None) == ARG
    assert lib.tnml_gd_step(ctx._h, Xp, None, 10, 0.1, 0.0, 2, 2, 1.0, None) == ARG
    assert lib.tnml_gd_step(ctx._h, Xp, yp, 0, 0.1, 0.0, 2, 2, 1.0, None) == ARG
    assert lib.tnml_gd_step(ctx._h, Xp, yp, 10, 0.1, 0.0, 3, 2, 1.0, None) == ARG
    assert lib.tnml_gd_step(ctx._h, Xp, yp, 10, 0.1, 0.0, 2, -1, 1.0, None) == ARG
    assert _code(lambda: ctx.gd_step(X, np.full(10, L), 0.1, 0.0, 'linear', 'MSE', 1.0)) == ARG  # a label out of range
    assert lib.tnml_gd_train_indices(ctx._h, None, 4, 2, 0.1, 0.0, 2, 2, 1.0, None) == ARG
    assert lib.tnml_gd_train_indices(ctx._h, ip, 0, 2, 0.1, 0.0, 2, 2, 1.0, None) == ARG
    assert lib.tnml_gd_train_indices(ctx._h, ip, 4, 0, 0.1, 0.0, 2, 2, 1.0, None) == ARG
    assert lib.tnml_gd_train_indices(ctx._h, ip, 4, 2, 0.1, 0.0, 2, 3, 1.0, None) == ARG
    assert _code(lambda: ctx.gd_train_indices([0, 10], 2, 0.1, 0.0, 'linear', 'MSE', 1.0)) == ARG
    assert _code(lambda: ctx.gd_train_indices([-1], 1, 0.1, 0.0, 'linear', 'MSE', 1.0)) == ARG
    assert lib.tnml_optim_config(ctx._h, 2, 0.0, 0.9, 0.999, 1e-8, 0) == ARG
    assert lib.tnml_optim_config(ctx._h, 0, 1.0, 0.9, 0.999, 1e-8, 1) == ARG
    assert lib.tnml_optim_config(ctx._h, 0, -0.1, 0.9, 0.999, 1e-8, 1) == ARG
    assert lib.tnml_optim_config(ctx._h, 1, 0.0, 1.0, 0.999, 1e-8, 0) == ARG
    assert lib.tnml_optim_config(ctx._h, 1, 0.0, 0.9, -0.1, 1e-8, 0) == ARG
    assert lib.tnml_optim_config(ctx._h, 1, 0.0, 0.9, 0.999, 0.0, 0) == ARG
    assert lib.tnml_optim_config(ctx._h, 1, 0.0, 0.9, 0.999, 1e-8, 1) == ARG                     # Adam has no clip
    assert lib.tnml_optim_config(None, 0, 0.0, 0.9, 0.999, 1e-8, 1) == ARG and lib.tnml_optim_reset(None) == ARG
    assert same_cores(ctx.get_cores()[0], cores)                                                 # nothing was launched
    # usable afterwards, with the default optimiser
    m1 = ctx.gd_train_indices([0, 1, 9], 3, 0.1, 0.0, 'linear', 'MSE', 1.0)
    after = ctx.get_cores()[0]
    ctx.set_cores(cores, 2)
    m2 = ctx.gd_step(X[[0, 1, 9]], y[[0, 1, 9]], 0.1, 0.0, 'linear', 'MSE', 1.0)
    assert tuple(m1[0]) == tuple(float(v) for v in m2) and same_cores(after, ctx.get_cores()[0])
    # a network scaled by 1e30: every step runs, the call reports it
    ctx.scale_cores(1e30)
    assert _code(lambda: ctx.gd_train_indices([0, 1, 9, 2], 2, 0.1, 0.0, 'linear', 'MSE', 1.0)) == NONFINITE
    ctx.set_cores(cores, 2)
    ctx.gd_train_indices([0, 1, 9, 2], 2, 0.1, 0.0, 'linear', 'MSE', 1.0)
    ctx.close()
    # LDS: the message names the bytes
    ctx = _hip.Context(4, 2, 2, 100, 64)
    ctx.set_cores(cores_for(4, 2, 2, 100, 0, rng, False), 0)
    with pytest.raises(_hip.TnmlError, match='bytes of LDS') as ei:
        ctx.gd_step(features(rng, 4, 4, 2), np.zeros(4, dtype=np.int32), 0.1, 0.0, 'linear', 'MSE', 1.0)
    assert ei.value.code == ARG
    ctx.close()
    # a communicator attached: the rule of the dataset block
    from tensornetworkforml_amd import dist as tdist
    monkeypatch.setenv('TNML_FORCE_COMM', '1')
    ctx = _hip.Context(N, D, L, M, 64)
    ctx.set_cores(cores_for(N, D, L, M, 0, rng, False), 0)
    tdist.attach_comm(ctx, 0, 1)
    assert _code(lambda: ctx.gd_step(X, y, 0.1, 0.0, 'linear', 'MSE', 1.0)) == STATE
    assert _code(lambda: ctx.gd_train_indices([0], 1, 0.1, 0.0, 'linear', 'MSE', 1.0)) == STATE
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------
# 8. reuse of one context
# ---------------------------------------------------------------------------------------------------------------
def test_reuse_larger_smaller_other_cores_other_optimiser():
    N, D, L, M = 17, 2, 3, 8
    rng = np.random.default_rng(69)
    ctx = _hip.Context(N, D, L, M, 64)
    worst = 0.0
    for b, l, ragged, kind in ((300, 3, True, 'sgd'), (17, 3, True, 'momentum'), (130, 16, False, 'sgd'), (5, 0, True, 'momentum'), (300, 9, True, 'sgd')):
        X, y = features(rng, b, N, D), rng.integers(0, L, b)
        cores = cores_for(N, D, L, M, l, rng, ragged, X)
        opt = dict(kind='sgd', momentum=0.9 if kind == 'momentum' else 0.0, clip=False)
        c64 = as64(cores)
        amax = max(np.abs(c).max() for c in c64)
        probe = R.GradientStepReference(c64, l, clip=False)
        probe.step(X, y, 1.0, R.WD, 'linear', 'MSE', 1.0)
        lr = 0.1001 * amax / max(np.abs(a - c).max() for a, c in zip(probe.cores, c64))
        ref = R.GradientStepReference(c64, l, **opt)
        ref.step(X, y, lr, R.WD, 'linear', 'MSE', 1.0)
        ctx.set_cores(cores, l)
        ctx.optim_config(**opt)
        ctx.gd_step(X, y, lr, R.WD, 'linear', 'MSE', 1.0)
        worst = max(worst, step_error(ctx.get_cores()[0], cores, ref.cores))
    ctx.close()
    print('reuse: worst %.2e of max|dA|' % worst)
    assert worst <= REUSE_TOL
