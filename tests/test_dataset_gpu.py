"""Device-resident dataset on the GPU (include/tnml.h "device-resident dataset").

  features form     dataset_read / select_indices + forward / predict_indices against X[idx] through set_input / predict: bit equality
  training          train_resident against train on the loader path: bit-identical cores, bonds, l_pos, val_acc, var_hist, pickles
  pixels form       the device's psi against the host's float64 psi rounded to float32: <= 1 unit in the last place of float32;
                    forward against the float64 oracle under the bound of the existing forward comparisons (relative 2e-5)
  evaluation        eval_indices: correct count == Network.accuracy's count (integer), mean |onehot - act(f)| within 4e-6 of a
                    float64 host evaluation of the device's own f (the bound of the per-step MAE comparison of
                    tests/test_true_shapes_gpu.py); resident_metrics; the non-finite flag
  state and errors  every documented refusal leaves the resident batch usable
  scripts           --resident training, evaluate_*.py
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

from tensornetworkforml_amd import _hip                       # noqa: E402
from tensornetworkforml_amd import data_generator as gen      # noqa: E402
from tensornetworkforml_amd import Network_class as tn        # noqa: E402
from oracle import mps_oracle as mo                            # noqa: E402

pytestmark = pytest.mark.gpu


def quiet():
    return contextlib.redirect_stdout(io.StringIO())


def relerr(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def calibrated_cores(N, M, D, L, X64, seed):
    """float32 cores whose f is O(1) on X64 (the oracle's calibration), and the float64 oracle state holding the same numbers."""
    rng = np.random.default_rng(seed)
    st = mo.MPSState(N, D, L, M, mo.random_cores(N, M, D, L, rng=rng, scale=M * 0.5 * 0.64 * D))
    mo.calibrate(st, X64)
    cores32 = [c.astype(np.float32) for c in st.cores]
    return cores32, mo.MPSState(N, D, L, M, [c.astype(np.float64) for c in cores32])


def make_dataset(n, N, D, L, seed):
    rng = np.random.default_rng(seed)
    pix = rng.random((n, N)).astype(np.float32)
    X64 = gen.psi(pix.astype(np.float64), D)
    y = rng.integers(0, L, n)
    return pix, X64, X64.astype(np.float32), y


def index_lists(n, cap, seed):
    rng = np.random.default_rng(seed)
    return {'ragged': rng.permutation(n)[:cap - 23], 'one': np.array([n - 1]), 'repeats': np.array([3, 3, 7, 3, n - 1, 7, 0, 0, 3] * 5),
            'beyond_capacity': rng.integers(0, n, 2 * cap + 37)}


# ---------------------------------------------------------------------------------------------------------------
# 4. features form: exact
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('D', [2, 3])
def test_features_form_is_exact(D):
    N, M, L, cap, n = 37, 6, 2, 100, 400            # N spans two 32-site tiles, the second one partial
    pix, X64, X32, y = make_dataset(n, N, D, L, 1)
    cores32, _ = calibrated_cores(N, M, D, L, X64[:32], 2)
    for name, idx in index_lists(n, cap, 3).items():
        assert (len(idx) % 64 != 0) and (name != 'beyond_capacity' or len(idx) > cap)
        ctx = _hip.Context(N, D, L, M, cap)          # a fresh context: the long list makes select_indices grow the buffers
        ctx.set_cores(cores32, 0)
        ctx.dataset_attach(X32, y, 'features')
        assert ctx.dataset_size == n
        got = ctx.dataset_read(idx)
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), X32[idx].view(np.uint32)), name
        ctx.select_indices(idx)
        assert ctx.b == len(idx)
        f_sel = ctx.forward()
        correct, abs_sum, nonfinite = ctx.resident_metrics('linear', 1.0)
        envs_sel = [ctx.get_env(_hip.SIDE_RIGHT, s) for s in (1, N // 2, N - 1)]
        fp_sel = ctx.predict_indices(idx)
        ctx.set_input(X32[idx], y[idx])
        f_set = ctx.forward()
        envs_set = [ctx.get_env(_hip.SIDE_RIGHT, s) for s in (1, N // 2, N - 1)]
        fp_set = ctx.predict(X32[idx])
        assert np.array_equal(f_sel.view(np.uint32), f_set.view(np.uint32)), name
        assert np.array_equal(fp_sel.view(np.uint32), fp_set.view(np.uint32)), name
        for a, b in zip(envs_sel, envs_set):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), name
        # the labels travelled with the samples
        assert (f_set[0] != f_set[1]).all()
        assert correct == int((np.argmax(f_set, axis=0) == y[idx]).sum()) and nonfinite == 0, name
        ref_sum = np.abs(np.eye(L)[:, y[idx]] - f_set.astype(np.float64)).sum()
        assert abs(abs_sum - ref_sum) <= 4e-6 * len(idx) * L, name
        ctx.close()


# ---------------------------------------------------------------------------------------------------------------
# 5. training is the same training
# ---------------------------------------------------------------------------------------------------------------
def _train_three_ways(linear_dim, M, D, trunc, n_samples, n_epochs, train_batch, val_batch, seed):
    """(loader run, loader run again, resident run) from the same initial network, seeds and batch order."""
    np.random.seed(seed)
    data, label = gen.create_dataset(n_samples, linear_dim, 0.6)
    sizes = dict(train_batch_size=train_batch, val_batch_size=val_batch, test_batch_size=64)
    train_loader, val_loader, _ = gen.prepare_dataset(data, label, 1, 0.2, D=D, **sizes)
    x_cal = next(iter(train_loader)).X
    with quiet():
        net0 = tn.Network(N=linear_dim ** 2, M=M, D=D, L=2, calibration_X=x_cal, normalize=True, act_fn='softmax',
                          loss_fn='full_cross_ent', trunc=trunc)
    blob = pickle.dumps(net0)
    runs = []
    for mode in ('loader', 'loader', 'resident'):
        net = pickle.loads(blob)
        np.random.seed(seed + 1)
        with quiet():
            if mode == 'loader':
                val_acc, var_hist = net.train(train_loader, val_loader, lr=0.01, n_epochs=n_epochs, weight_dec=1e-3)
            else:
                ds, tr_idx, va_idx, _ = gen.prepare_device_dataset(net, data, label, 1, 0.2, D=D, pixels=False, **sizes)
                assert len(ds) == n_samples and not ds.pixels
                val_acc, var_hist = net.train_resident(tr_idx, va_idx, lr=0.01, n_epochs=n_epochs, weight_dec=1e-3)
        cores, bond, lp = net._ctx.get_cores()
        runs.append(dict(net=net, val_acc=list(val_acc), var_hist=var_hist, cores=cores, bond=list(bond), l_pos=lp))
    return runs


def _assert_same_training(a, b, what):
    assert a['bond'] == b['bond'] and a['l_pos'] == b['l_pos'] == a['net'].l_pos == b['net'].l_pos, what
    for i, (ca, cb) in enumerate(zip(a['cores'], b['cores'])):
        assert ca.shape == cb.shape and np.array_equal(ca.view(np.uint32), cb.view(np.uint32)), (what, 'core', i)
    assert a['val_acc'] == b['val_acc'], (what, a['val_acc'], b['val_acc'])
    assert a['var_hist'].shape == b['var_hist'].shape and np.array_equal(a['var_hist'], b['var_hist']), what


@pytest.mark.parametrize('linear_dim,M,D,trunc,n_epochs', [(5, 6, 2, 'fixed', 3), (5, 6, 2, 'reference', 3), (14, 10, 2, 'fixed', 2),
                                                           (14, 10, 2, 'reference', 2), (5, 4, 3, 'fixed', 1)])
def test_train_resident_is_the_same_training(linear_dim, M, D, trunc, n_epochs):
    n_samples = 600 if linear_dim == 5 else 400
    train_batch, val_batch = (240, 50) if linear_dim == 5 else (160, 40)         # neither a multiple of 64
    first, second, resident = _train_three_ways(linear_dim, M, D, trunc, n_samples, n_epochs, train_batch, val_batch, 20 + linear_dim + D)
    N = linear_dim ** 2
    assert first['var_hist'].shape == (n_epochs, 2, 2 * (N - 1)) and np.isfinite(first['var_hist']).all()
    # the premise: the loader path repeats itself bit for bit
    _assert_same_training(first, second, 'loader path, run twice')
    _assert_same_training(first, resident, 'loader path against resident path')
    # the pickled state of both loads into equal models; the dataset is not pickled
    na, nb = pickle.loads(pickle.dumps(first['net'])), pickle.loads(pickle.dumps(resident['net']))
    assert na.l_pos == nb.l_pos and len(na.As) == len(nb.As) == N and nb._dataset is None
    for ta, tb in zip(na.As, nb.As):
        assert list(ta.axes_names) == list(tb.axes_names) and np.array_equal(ta.elem, tb.elem)
    with pytest.raises(RuntimeError, match='attach_dataset'):
        nb.evaluate(np.arange(4))
    # environment lists and TX after the last sweep, as train leaves them
    la, lb = first['net'], resident['net']
    for which in ('r_cum_contraction', 'l_cum_contraction'):
        ea, eb = getattr(la, which), getattr(lb, which)
        assert (ea is None) == (eb is None)
        if ea is not None:
            assert len(ea) == len(eb)
            if len(ea):
                assert np.array_equal(ea[len(ea) // 2].elem, eb[len(eb) // 2].elem)
    assert len(lb.TX) == N and np.array_equal(lb.TX[3].elem, la.TX[3].elem.astype(np.float32).astype(np.float64))


# ---------------------------------------------------------------------------------------------------------------
# 6. pixels form
# ---------------------------------------------------------------------------------------------------------------
def _ordered(a):
    i = np.ascontiguousarray(a, dtype=np.float32).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7fffffff), i)


@pytest.mark.parametrize('D', [2, 3, 5, 8])
def test_pixels_form_matches_host_psi_within_one_ulp(D):
    """One unit in the last place is what two correctly working float64 evaluations allow after a single rounding to float32."""
    N, L, M = 50, 2, 2
    rng = np.random.default_rng(40 + D)
    one, zero = np.float32(1), np.float32(0)
    special = np.array([0, 1, np.nextafter(zero, one), np.nextafter(one, zero), np.nextafter(np.nextafter(one, zero), zero), 0.5,
                        np.float32(1e-3), np.float32(1) - np.float32(1e-3)], dtype=np.float32)
    vals = np.concatenate([special, rng.random(100000).astype(np.float32)])
    n = -(-len(vals) // N)
    pix = np.concatenate([vals, rng.random(n * N - len(vals)).astype(np.float32)]).reshape(n, N)
    want = gen.psi(pix.astype(np.float64), D).astype(np.float32)          # float64 psi, then _hip._f32's conversion
    ctx = _hip.Context(N, D, L, M, 64)
    ctx.dataset_attach(pix, np.zeros(n, dtype=np.int64), 'pixels')
    got = np.concatenate([ctx.dataset_read(np.arange(k, min(k + 500, n))) for k in range(0, n, 500)])
    ctx.close()
    assert got.shape == want.shape == (n, N, D)
    diff = np.abs(_ordered(got) - _ordered(want))
    print('D = %d: %d of %d elements differ from the host, largest distance %d ulp' % (D, int((diff > 0).sum()), diff.size, int(diff.max())))
    assert diff.max() <= 1
    assert np.array_equal(got[0, :2], want[0, :2])                         # psi(0), psi(1): exact ends


@pytest.mark.parametrize('D', [2, 3])
def test_pixels_forward_against_the_float64_oracle(D):
    """forward from a pixels batch and from the host-embedded batch, each against the float64 oracle on the host's float64 psi,
    under the bound of the existing forward comparisons (tests/test_hip_parity.py, tests/test_feature_dim_gpu.py): relative 2e-5."""
    N, M, L, n, b = 40, 8, 2, 300, 150
    pix, X64, X32, y = make_dataset(n, N, D, L, 50 + D)
    cores32, st = calibrated_cores(N, M, D, L, X64[:32], 51)
    idx = np.random.default_rng(52).permutation(n)[:b]
    f_o = mo.forward(st, X64[idx])
    ctx = _hip.Context(N, D, L, M, b)
    ctx.set_cores(cores32, 0)
    ctx.dataset_attach(pix, y, 'pixels')
    ctx.select_indices(idx)
    f_pix = ctx.forward()
    ctx.set_input(X32[idx], y[idx])
    f_host = ctx.forward()
    ctx.close()
    print('D = %d: pixels batch %.2e, host-embedded batch %.2e (relative to max|f| of the oracle)' % (D, relerr(f_pix, f_o), relerr(f_host, f_o)))
    assert relerr(f_pix, f_o) < 2e-5
    assert relerr(f_host, f_o) < 2e-5


# ---------------------------------------------------------------------------------------------------------------
# 7. evaluation
# ---------------------------------------------------------------------------------------------------------------
def _host_metrics(f32, y, act_fn, T, L):
    fa = mo.apply_act_func(f32.astype(np.float64), act_fn, T)
    return int((np.argmax(f32, axis=0) == y).sum()), np.abs(np.eye(L)[:, y] - fa).mean()


def _eval_net(D, L=2, cap=64, trained=True):
    N, M, n = 25, 6, 700
    np.random.seed(60 + D + L)
    if L == 2:
        data, label = gen.create_dataset(n, 5, 0.6)
    else:
        data, label = np.random.random((n, 5, 5)), np.random.randint(0, L, n)
    X = gen.psi(data.reshape(n, -1), D)
    with quiet():
        net = tn.Network(N=N, M=M, D=D, L=L, calibration_X=X[:cap], normalize=True, act_fn='softmax', loss_fn='full_cross_ent', trunc='fixed')
        net.attach_dataset(X, label, pixels=False)
        if trained:
            net.train_resident(gen.IndexLoader(np.arange(cap), cap, drop_last=True), gen.IndexLoader(np.arange(cap, 2 * cap), cap), lr=0.01,
                               n_epochs=2, weight_dec=1e-3)
    return net, X, label


@pytest.mark.parametrize('D,L', [(2, 2), (3, 2), (2, 3)])
def test_eval_indices_counts_and_errors(D, L):
    cap = 64
    net, X, label = _eval_net(D, L, cap, trained=(L == 2))
    ctx = net._ctx
    b = 3 * cap + 17
    assert b > ctx.b and net.l_pos in (0, net.N - 1)
    idx = np.random.default_rng(61).permutation(len(X))[:b]
    # what the validation loop of Network.train counts, in chunks (this leaves the prediction buffers one capacity wide, so that the
    # evaluation below really runs in four chunks)
    want_correct = 0
    for k in range(0, b, cap):
        ch = idx[k:k + cap]
        want_correct += int(round(net.accuracy(X[ch], label[ch], net.predict(X[ch])) * len(ch)))
    results = {act: ctx.eval_indices(idx, act, net.T) for act in ('linear', 'sigmoid', 'softmax')}
    f_all = ctx.predict_indices(idx)                 # the device's own f of these samples
    srt = np.sort(f_all, axis=0)
    assert (srt[-1] > srt[-2]).all(), 'a tie between labels would make the integer comparison meaningless'
    for act, (correct, abs_sum, nonfinite) in results.items():
        host_correct, host_mae = _host_metrics(f_all, label[idx], act, net.T, L)
        print('D %d L %d %s: correct %d / %d, MAE device %.9f host %.9f (difference %.2e)' % (D, L, act, correct, b, abs_sum / (b * L), host_mae,
                                                                                               abs(abs_sum / (b * L) - host_mae)))
        assert isinstance(correct, int) and correct == want_correct == host_correct
        assert nonfinite == 0
        assert abs(abs_sum / (b * L) - host_mae) < 4e-6
    # Network.evaluate: overall figures for an index array, mean over batches for a loader (differs with a ragged last batch)
    acc, mae = net.evaluate(idx)
    assert acc == want_correct / b and abs(mae - _host_metrics(f_all, label[idx], 'softmax', net.T, L)[1]) < 4e-6
    acc_raw, mae_raw = net.evaluate(idx, activated=False)
    assert acc_raw == acc and abs(mae_raw - _host_metrics(f_all, label[idx], 'linear', net.T, L)[1]) < 4e-6
    loader = gen.IndexLoader(idx, 50, shuffle=False)
    per = [_host_metrics(f_all[:, k:k + 50], label[idx[k:k + 50]], 'softmax', net.T, L) for k in range(0, b, 50)]
    acc_l, mae_l = net.evaluate(loader)
    assert len(per) == 5 and b % 50
    assert abs(acc_l - np.mean([c / len(idx[k:k + 50]) for (c, _), k in zip(per, range(0, b, 50))])) < 1e-12
    assert abs(mae_l - np.mean([m for _, m in per])) < 4e-6


def test_resident_metrics_against_eval_and_the_non_finite_flag():
    net, X, label = _eval_net(2, 2, 64)
    ctx, N, L, T = net._ctx, net.N, net.L, net.T
    idx = np.random.default_rng(62).permutation(len(X))[:300]
    # after a forward: the same f as the evaluation's chain, the same 256-sample blocks -> the same numbers
    with quiet():
        net._forward_indices(idx)
    res = ctx.resident_metrics('softmax', T)
    ev = ctx.eval_indices(idx, 'softmax', T)
    f_fwd = ctx.get_f()
    assert np.array_equal(f_fwd, ctx.predict_indices(idx))
    assert res[0] == ev[0] == _host_metrics(f_fwd, label[idx], 'softmax', T, L)[0] and res[2] == ev[2] == 0
    assert abs(res[1] - ev[1]) <= 1e-12 * abs(ev[1])
    # after a sweep the device holds the f of the last updated, UN-truncated merged tensor, the evaluation runs the chain over the
    # truncated cores: resident_metrics is exact on the f it was given (count) and within the MAE bound of it, and differs from the
    # evaluation by no more than the two f differ (triangle inequality: per element ||a - x| - |a - y|| <= |x - y|)
    left = net.l_pos == N - 1
    ctx.sweep(left, N - 1, True, 0.01, 1e-3, True, 'softmax', 'full_cross_ent', T, 'fixed', want_metrics=False, want_f=False)
    res = ctx.resident_metrics('softmax', T)
    f_swp = ctx.get_f()
    ev = ctx.eval_indices(idx, 'softmax', T)
    f_ev = ctx.predict_indices(idx)
    assert (f_swp[0] != f_swp[1]).all()
    host_c, host_mae = _host_metrics(f_swp, label[idx], 'softmax', T, L)
    b = len(idx)
    assert res[0] == host_c and abs(res[1] / (b * L) - host_mae) < 4e-6 and res[2] == 0
    moved = int((np.argmax(f_swp, axis=0) != np.argmax(f_ev, axis=0)).sum())
    gap = np.abs(mo.apply_act_func(f_swp.astype(np.float64), 'softmax', T) - mo.apply_act_func(f_ev.astype(np.float64), 'softmax', T)).mean()
    print('after a sweep: correct %d (resident) / %d (evaluation), %d samples changed side; MAE %.9f / %.9f, mean |act(f) - act(f)| %.2e'
          % (res[0], ev[0], moved, res[1] / (b * L), ev[1] / (b * L), gap))
    assert abs(res[0] - ev[0]) <= moved
    assert abs(res[1] - ev[1]) / (b * L) <= gap + 2 * 4e-6
    # a NaN core raises the flag
    cores, _, lp = ctx.get_cores()
    cores[N // 2][0, 0, 0] = np.nan
    ctx.set_cores(cores, lp)
    correct, abs_sum, nonfinite = ctx.eval_indices(idx, 'softmax', T)
    assert nonfinite == b
    ctx.select_indices(idx)
    ctx.forward(want_f=False)
    assert ctx.resident_metrics('sigmoid', T)[2] == b
    acc, mae = net.evaluate(idx)
    assert np.isnan(mae)


# ---------------------------------------------------------------------------------------------------------------
# 8. state and errors
# ---------------------------------------------------------------------------------------------------------------
def _code(fn):
    with pytest.raises(_hip.TnmlError) as ei:
        fn()
    return ei.value.code


@pytest.mark.parametrize('D', [2, 3])
def test_refusals_leave_the_resident_batch_usable(D, monkeypatch):
    ARG, STATE = -1, -2
    N, M, L, cap, n = 20, 5, 3, 70, 200
    pix, X64, X32, y = make_dataset(n, N, D, L, 70 + D)
    cores32, _ = calibrated_cores(N, M, D, L, X64[:32], 71)
    ctx = _hip.Context(N, D, L, M, cap)
    ctx.set_cores(cores32, 0)
    good = np.arange(10, 10 + cap)
    # nothing attached
    assert _code(lambda: ctx.select_indices(good)) == STATE
    assert _code(lambda: ctx.predict_indices(good)) == STATE
    assert _code(lambda: ctx.eval_indices(good, 'softmax', 0.1)) == STATE
    assert _code(lambda: ctx.dataset_read(good)) == STATE
    assert _code(lambda: ctx.resident_metrics('softmax', 0.1)) == STATE          # no resident batch either
    # a dataset of another N or D, labels outside [0, L)
    assert _code(lambda: ctx.dataset_attach(np.zeros((5, N + 1, D), np.float32), np.zeros(5, int), 'features')) == ARG
    assert _code(lambda: ctx.dataset_attach(np.zeros((5, N, D + 1), np.float32), np.zeros(5, int), 'features')) == ARG
    assert _code(lambda: ctx.dataset_attach(np.zeros((5, N + 1), np.float32), np.zeros(5, int), 'pixels')) == ARG
    assert _code(lambda: ctx.dataset_attach(X32[:5], np.array([0, 1, L, 0, 0]), 'features')) == ARG
    assert _code(lambda: ctx.dataset_attach(X32[:5], np.array([0, -1, 0, 0, 0]), 'features')) == ARG
    assert ctx.dataset_size == 0
    ctx.dataset_attach(X32, y, 'features')
    ctx.select_indices(good)
    f0 = ctx.forward()
    envs0 = [ctx.get_env(_hip.SIDE_RIGHT, s) for s in (1, N - 1)]

    def still_usable():
        assert ctx.b == cap
        assert np.array_equal(ctx.get_f(), f0)
        for s, e in zip((1, N - 1), envs0):
            assert np.array_equal(ctx.get_env(_hip.SIDE_RIGHT, s), e)
        assert np.array_equal(ctx.forward(), f0)

    for bad_value in (n, n + 1000, -1, -2 ** 31, 2 ** 31 - 1):
        bad = good.copy()
        bad[cap // 2] = bad_value
        assert _code(lambda: ctx.select_indices(bad)) == ARG
        assert _code(lambda: ctx.predict_indices(bad)) == ARG
        assert _code(lambda: ctx.eval_indices(bad, 'softmax', 0.1)) == ARG
        assert _code(lambda: ctx.dataset_read(bad)) == ARG
        still_usable()
    assert _code(lambda: ctx.select_indices(np.array([2 ** 31]))) == ARG                  # beyond int32: refused by the binding
    empty = np.zeros(0, dtype=np.int64)
    assert _code(lambda: ctx.select_indices(empty)) == ARG
    assert _code(lambda: ctx.predict_indices(empty)) == ARG
    assert _code(lambda: ctx.eval_indices(empty, 'softmax', 0.1)) == ARG
    with pytest.raises(TypeError):
        ctx.select_indices(np.array([0.5, 1.0]))
    still_usable()
    # predict_indices / eval_indices leave f and the environments bit-identical (the check made for predict)
    other = np.arange(n - 2 * cap - 9, n)
    fp = ctx.predict_indices(other)
    assert np.array_equal(fp, ctx.predict(X32[other]))
    ctx.eval_indices(other, 'sigmoid', 0.3)
    assert np.array_equal(ctx.get_f(), f0)
    for s, e in zip((1, N - 1), envs0):
        assert np.array_equal(ctx.get_env(_hip.SIDE_RIGHT, s), e)
    # ... and the sweep that follows is the sweep without them
    args = (False, N - 1, True, 0.01, 1e-3, True, 'softmax', 'full_cross_ent', 0.1, 'fixed')
    met_a, f_a = ctx.sweep(*args)
    ctx.set_cores(cores32, 0)
    ctx.select_indices(good)
    ctx.forward()
    met_b, f_b = ctx.sweep(*args)
    assert np.array_equal(met_a, met_b) and np.array_equal(f_a, f_b)
    # an intermediate label position
    ctx.set_cores(cores32, 0)
    ctx.select_indices(good)
    ctx.forward()
    ctx.sweep(False, 2, True, 0.01, 1e-3, True, 'softmax', 'full_cross_ent', 0.1, 'fixed')
    assert ctx.l_pos == 2
    assert _code(lambda: ctx.predict_indices(good)) == STATE
    assert _code(lambda: ctx.eval_indices(good, 'softmax', 0.1)) == STATE
    # re-attach replaces, detach frees, select then fails cleanly
    ctx.set_cores(cores32, 0)
    ctx.dataset_attach(pix[:50], y[:50], 'pixels')
    assert ctx.dataset_size == 50
    assert _code(lambda: ctx.select_indices(good)) == ARG                                 # 79 >= 50 now
    ctx.select_indices(np.arange(50))
    assert np.isfinite(ctx.forward()).all()
    ctx.dataset_detach()
    assert ctx.dataset_size == 0
    assert _code(lambda: ctx.select_indices(np.arange(5))) == STATE
    assert np.isfinite(ctx.forward()).all()                                               # the resident batch outlives its dataset
    ctx.close()
    if D == 2:
        # a communicator attached (one rank, forced): the dataset calls are refused
        from tensornetworkforml_amd import dist as tdist
        monkeypatch.setenv('TNML_FORCE_COMM', '1')
        ctx = _hip.Context(N, D, L, M, cap)
        ctx.set_cores(cores32, 0)
        tdist.attach_comm(ctx, 0, 1)
        assert _code(lambda: ctx.dataset_attach(X32, y, 'features')) == STATE
        assert _code(lambda: ctx.select_indices(good)) == STATE
        assert _code(lambda: ctx.eval_indices(good, 'softmax', 0.1)) == STATE
        ctx.set_input(X32[good], y[good])
        assert np.array_equal(ctx.forward(), f0)
        assert _code(lambda: ctx.resident_metrics('softmax', 0.1)) == STATE
        ctx.close()


# ---------------------------------------------------------------------------------------------------------------
# 9. the four scripts
# ---------------------------------------------------------------------------------------------------------------
def _printed_figures(text):
    acc = [ln for ln in text.splitlines() if 'Accuracy:' in ln]
    mae = [ln for ln in text.splitlines() if 'Mean Absolute Error:' in ln]
    assert len(acc) == 1 and len(mae) == 1, text
    return float(acc[0].split(':')[1]), float(mae[0].split(':')[1])


def test_diagonals_scripts_resident_training_then_evaluation(tmp_path, monkeypatch):
    from tensornetworkforml_amd import training_diagonals as train_script
    from tensornetworkforml_amd import evaluate_diagonals as eval_script
    monkeypatch.chdir(tmp_path)
    out = str(tmp_path / 'diag.dat')
    np.random.seed(3)
    with quiet():
        val_acc, var_hist = train_script.main(['--n_samples', '2000', '--n_train_batch', '2', '--n_epochs', '3', '--resident', '--out', out])
    assert var_hist.shape == (3, 2, 2 * 63) and np.isfinite(var_hist).all() and len(val_acc) == 3 and val_acc[-1] >= 0.95
    buf = io.StringIO()
    np.random.seed(8)
    with contextlib.redirect_stdout(buf):
        acc, mae = eval_script.main(['--filename', out, '--n_samples', '1000', '--batch_size', '128'])
    assert _printed_figures(buf.getvalue()) == (float(repr(acc)), float(repr(mae)))
    assert acc >= 0.9 and 0.0 <= mae <= 1.0
    # the same figures from Network.evaluate on the same data
    with open(out, 'rb') as fh:
        net = pickle.load(fh)
    np.random.seed(8)
    data, label = gen.create_dataset(1000, 8, 0.6)
    with quiet():
        _, _, _, test_loader = gen.prepare_device_dataset(net, data, label, 0, 0, 1, 1, 128, D=net.D, pixels=True)
    assert [len(i) for i in test_loader] == [128] * 7 + [104]
    assert net.evaluate(test_loader) == (acc, mae)
    # the features form holds the float32 numbers the loader path uploads: the same accuracy as predict + host argmax, batch by batch
    with quiet():
        _, _, _, feat_loader = gen.prepare_device_dataset(net, data, label, 0, 0, 1, 1, 128, D=net.D, pixels=False)
    _, _, ref_loader = gen.prepare_dataset(data, label, 0, 0, 1, 1, 128, D=net.D)
    ref_acc = float(np.mean([net.accuracy(b.X, b.y, net.predict(b.X)) for b in ref_loader]))
    assert net.evaluate(feat_loader)[0] == ref_acc
    assert (data.shape, net.N) == ((1000, 8, 8), 64)


def test_binary_mnist_scripts_resident_training_then_evaluation(tmp_path, monkeypatch):
    from tensornetworkforml_amd import training_binary_MNIST as train_script
    from tensornetworkforml_amd import evaluate_binary_MNIST as eval_script
    from test_network_gpu import _synthetic_mnist
    root = str(tmp_path / 'datasets')
    n01 = _synthetic_mnist(root, 2000, 500, 5)
    monkeypatch.chdir(tmp_path)
    out = str(tmp_path / 'mnist.dat')
    np.random.seed(4)
    with quiet():
        val_acc, var_hist = train_script.main(['--data_dir', root, '--n_epochs', '2', '--n_train_batch', '4', '--normalise', '--lr', '0.01',
                                               '--L2_decay', '1e-3', '--resident', '--out', out])
    assert n01 > 500 and var_hist.shape == (2, 2, 4 * 195) and np.isfinite(var_hist).all() and all(0.0 <= v <= 1.0 for v in val_acc)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        acc, mae = eval_script.main(['--filename', out, '--data_dir', root, '--normalise', '--batch_size', '100'])
    assert _printed_figures(buf.getvalue()) == (float(repr(acc)), float(repr(mae)))
    with open(out, 'rb') as fh:
        net = pickle.load(fh)
    assert net.N == 196
    _, _, te, tel = gen.get_MNIST_dataset(root)
    mask = tel < 2
    data01 = eval_script.pooling(te)[mask] / 255.0
    with quiet():
        _, _, _, test_loader = gen.prepare_device_dataset(net, data01, tel[mask], 0, 0, 1, 1, 100, D=2, pixels=True)
    assert net.evaluate(test_loader) == (acc, mae) and 0.0 <= acc <= 1.0 and 0.0 <= mae <= 1.0
