"""The two-site likelihood sweep on the device (tnml_nll_sweep, tnml_nll_sweep_indices, tnml_nll_sweep_debug)
against the float64 reference of tests/nll_sweep_reference.py.  The float32 bounds are read from that module's emulation table (ten
times the emulation's figure, rounded up to one digit; tests/test_nll_sweep_host.py asserts the table); what is float64 on the device
and in the reference alike (B, Gz) is held to F64; everything else is bit-equality.

  1  single steps from equal cores     B, Gd, Gz, B_new, sigma of the capture and the six values, every case
  2  whole right + left passes         values, log Z, bonds, l_pos, predict; the batch's NLL falls
  3  lr = 0 at full-rank max_bond      predict unchanged
  4  truncation                        threshold 0.99 on the device's own sigma, the discarded weight, max_bond as the cap
  5  bit equality                      repetition, n steps against k and n - k, the index form
  6  the guard                         one sample of f_y == 0
  7  state behind the call, refusals
  8  Network.nll_sweep, train_generative(method='sweep'), the script option
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
import nll_reference as NR                                         # noqa: E402
import nll_sweep_reference as R                                    # noqa: E402
from tensornetworkforml_amd import _hip                            # noqa: E402

pytestmark = pytest.mark.gpu

ARG, STATE, NONFINITE = -1, -2, -7
# float64 on both sides, sums of at most a few thousand terms in another order: 2^-53 times the terms, with a decade to spare
F64 = 1e-12


def _code(call):
    with pytest.raises(_hip.TnmlError) as ei:
        call()
    return ei.value.code


def new_ctx(cores, l, L, M=R.MAX_BOND, b=64):
    ctx = _hip.Context(len(cores), R.D, L, M, b)
    ctx.set_any_position(True)
    ctx.set_cores(A.as32(cores), l)
    return ctx


def dev_cores(ctx):
    return [c.astype(np.float64) for c in ctx.get_cores()[0]]


def same(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def rel(a, ref):
    return float(np.abs(np.asarray(a) - np.asarray(ref)).max() / np.abs(ref).max())


def close_values(dev, ref):
    """the six values of every step: value, log Z and the discarded weight within the table's bounds, no bad sample, no bit, the
    reference's rank"""
    dev, ref = np.atleast_2d(dev), np.atleast_2d(ref)
    dv = np.abs(dev[:, 0] - ref[:, 0]) / np.maximum(1.0, np.abs(ref[:, 0]))
    dz = np.abs(dev[:, 1] - ref[:, 1]) / np.maximum(1.0, np.abs(ref[:, 1]))
    print('values: value %.3e (bound %.0e)  log Z %.3e (bound %.0e)' % (dv.max(), R.gpu_bound('value'), dz.max(), R.gpu_bound('logz')))
    assert dv.max() <= R.gpu_bound('value'), dv
    assert dz.max() <= R.gpu_bound('logz'), dz
    assert (dev[:, 2] == 0).all() and (dev[:, 3] == 0).all(), dev[:, 2:4]
    assert (dev[:, 4] == ref[:, 4]).all(), (dev[:, 4], ref[:, 4])
    dw = np.abs(dev[:, 5] - ref[:, 5]).max()
    print('discarded weight: %.3e (bound %.0e)' % (dw, R.gpu_bound('discarded')))
    assert dw <= R.gpu_bound('discarded'), (dev[:, 5], ref[:, 5])


@pytest.fixture(scope='module')
def built():
    return {R.case_id(c): R.build_case(c) for c in R.CASES}


@pytest.fixture(scope='module')
def passes(built):
    """the float64 pass of every case, computed once"""
    return {R.case_id(c): R.there_and_back(*built[R.case_id(c)][:3], built[R.case_id(c)][4], built[R.case_id(c)][5], R.LR, c[5], R.MAX_BOND)
            for c in R.CASES}


# ---------------------------------------------------------------------------------------------------------------
# 1  single steps
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', R.CASES, ids=R.case_id)
def test_single_step_against_the_reference(case, built):
    cores, l, X, lab, y, S = built[R.case_id(case)]
    left = R.plan(case[0], l)[0][0]
    _, l_ref, rec = R.step(cores, l, X, y, S, left, R.LR, case[5], R.MAX_BOND)
    ctx = new_ctx(cores, l, case[1])
    vals = ctx.nll_sweep(X, y, S, left_dir=left, n_steps=1, lr=R.LR, renorm=case[5], max_bond=R.MAX_BOND)
    shape = rec['B'].shape
    figs = {}
    for name, bound in (('B', F64), ('Gd', R.gpu_bound('Gd')), ('Gz', F64), ('B_new', R.gpu_bound('B_new'))):
        figs[name] = rel(ctx.nll_sweep_debug(name).reshape(shape), rec[name])
        print('%s: %.3e (bound %.0e)' % (name, figs[name], bound))
    sig = ctx.nll_sweep_debug('sigma')
    # |sigma_j - sigma_j'| <= |dB|_2 <= |dB|_F <= sqrt(size) max|dB|
    sig_bound = R.gpu_bound('B_new') * np.abs(rec['B_new']).max() * np.sqrt(rec['B'].size)
    print('sigma: %.3e (bound %.3e)' % (np.abs(sig - rec['sigma']).max(), sig_bound))
    assert figs['B'] <= F64 and figs['Gz'] <= F64, figs
    assert figs['Gd'] <= R.gpu_bound('Gd') and figs['B_new'] <= R.gpu_bound('B_new'), figs
    assert sig.shape == rec['sigma'].shape and np.abs(sig - rec['sigma']).max() <= sig_bound
    close_values(vals, rec['values'])
    assert ctx.l_pos == l_ref
    ctx.close()


def test_single_step_on_the_large_tensor_path():
    """N = 4, bond 40, L = 2, b = 70: the merged matrix is 80 x 160, beyond the in-LDS kernel"""
    cores, l, X, lab, S = R.big_case()
    new, l_ref, rec = R.step(cores, l, X, lab, S, False, R.LR, True, 40)
    ctx = new_ctx(cores, l, 2, M=40)
    vals = ctx.nll_sweep(X, lab, S, left_dir=False, n_steps=1, lr=R.LR, renorm=True, max_bond=40)
    shape = rec['B'].shape
    assert shape == (40, 2, 2, 40, 2)
    for name, bound in (('B', F64), ('Gd', R.gpu_bound('Gd')), ('Gz', F64), ('B_new', R.gpu_bound('B_new'))):
        fig = rel(ctx.nll_sweep_debug(name).reshape(shape), rec[name])
        print('%s: %.3e (bound %.0e)' % (name, fig, bound))
        assert fig <= bound, (name, fig)
    close_values(vals, rec['values'])
    f_dev, f_ref = ctx.predict(X), NR.forward(new, l_ref, X.astype(np.float64))
    print('f: %.3e (bound %.0e)' % (rel(f_dev, f_ref), R.gpu_bound('f')))
    assert rel(f_dev, f_ref) <= R.gpu_bound('f')
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------
# 2 / 3  whole passes
# ---------------------------------------------------------------------------------------------------------------
def run_pass(ctx, N, l, X, y, S, lr, renorm, **kw):
    out = []
    for left, n in R.plan(N, l):
        out.append(ctx.nll_sweep(X, y, S, left_dir=left, n_steps=n, lr=lr, renorm=renorm, max_bond=R.MAX_BOND, **kw))
    return np.concatenate(out)


@pytest.mark.parametrize('case', R.CASES, ids=R.case_id)
def test_whole_pass_against_the_reference(case, built, passes):
    cores, l, X, lab, y, S = built[R.case_id(case)]
    c_ref, l_ref, v_ref = passes[R.case_id(case)]
    ctx = new_ctx(cores, l, case[1])
    before = ctx.nll_eval(X, y, S)[0]
    vals = run_pass(ctx, case[0], l, X, y, S, R.LR, case[5])
    close_values(vals, v_ref)
    bonds, lp = ctx.bonds()
    assert lp == l_ref == ctx.l_pos
    assert bonds.tolist() == [c.shape[2] for c in c_ref[:-1]]
    f_dev, f_ref = ctx.predict(X), NR.forward(c_ref, l_ref, X.astype(np.float64))
    print('f: %.3e (bound %.0e)' % (rel(f_dev, f_ref), R.gpu_bound('f')))
    assert rel(f_dev, f_ref) <= R.gpu_bound('f')
    after = ctx.nll_eval(X, y, S)[0]
    print('nll %.6f -> %.6f' % (before, after))
    assert after < before
    ctx.close()


@pytest.mark.parametrize('case', R.LR0, ids=R.case_id)
def test_lr_zero_leaves_the_function(case, built):
    cores, l, X, lab, y, S = built[R.case_id(case)]
    ctx = new_ctx(cores, l, case[1])
    f0 = NR.forward(cores, l, X.astype(np.float64))
    vals = run_pass(ctx, case[0], l, X, y, S, 0.0, case[5])
    assert (vals[:, 3] == 0).all()
    cs, lp = dev_cores(ctx), ctx.l_pos
    f1 = NR.forward(cs, lp, X.astype(np.float64))
    print('f: %.3e (bound %.0e)' % (rel(f1, f0), R.gpu_bound('f')))
    assert rel(f1, f0) <= R.gpu_bound('f')
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------
# 4  truncation
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', [R.CASES[1], R.CASES[4]], ids=R.case_id)
def test_truncation(case, built):
    cores, l, X, lab, y, S = built[R.case_id(case)]
    N = case[0]
    ctx = new_ctx(cores, l, case[1])
    for left, n in R.plan(N, l):
        for _ in range(n):
            v = ctx.nll_sweep(X, y, S, left_dir=left, n_steps=1, lr=R.LR, renorm=case[5], max_bond=R.MAX_BOND, threshold=0.99)[0]
            sig = ctx.nll_sweep_debug('sigma')
            m = R.kept_rank(sig, min(R.MAX_BOND, len(sig)), 0.99)
            assert v[4] == m, (v, sig)
            assert abs(v[5] - R.discarded_weight(sig, m)) <= F64
            p = ctx.l_pos if left else ctx.l_pos - 1
            assert ctx.bonds()[0][p] == m
    ctx.close()
    ctx = new_ctx(cores, l, case[1])
    for left, n in R.plan(N, l)[:1]:
        vals = ctx.nll_sweep(X, y, S, left_dir=left, n_steps=n, lr=R.LR, renorm=case[5], max_bond=3)
        assert (vals[:, 4] <= 3).all() and (ctx.bonds()[0] <= 4).all()
        assert vals[:, 4].max() == 3
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------
# 5  bit equality
# ---------------------------------------------------------------------------------------------------------------
def test_bit_equalities(built):
    case = R.CASES[4]
    cores, l, X, lab, y, S = built[R.case_id(case)]
    N, L = case[0], case[1]
    n = N - 1 - l
    a, b, c, d = (new_ctx(cores, l, L) for _ in range(4))
    va = a.nll_sweep(X, y, S, n_steps=n, lr=R.LR, max_bond=R.MAX_BOND)
    vb = b.nll_sweep(X, y, S, n_steps=n, lr=R.LR, max_bond=R.MAX_BOND)
    assert va.tobytes() == vb.tobytes() and same(a.get_cores()[0], b.get_cores()[0])
    vc = np.concatenate([c.nll_sweep(X, y, S, n_steps=1, lr=R.LR, max_bond=R.MAX_BOND),
                         c.nll_sweep(X, y, S, n_steps=n - 1, lr=R.LR, max_bond=R.MAX_BOND)])
    assert va.tobytes() == vc.tobytes() and same(a.get_cores()[0], c.get_cores()[0])
    d.dataset_attach(X, lab)
    vd = d.nll_sweep_indices(np.arange(len(lab)), labels=True, S=S, n_steps=n, lr=R.LR, max_bond=R.MAX_BOND)
    assert va.tobytes() == vd.tobytes() and same(a.get_cores()[0], d.get_cores()[0])
    # and back, continuing on each context
    wa = a.nll_sweep(X, y, S, left_dir=True, n_steps=N - 1, lr=R.LR, max_bond=R.MAX_BOND)
    wc = np.concatenate([c.nll_sweep(X, y, S, left_dir=True, n_steps=3, lr=R.LR, max_bond=R.MAX_BOND),
                         c.nll_sweep(X, y, S, left_dir=True, n_steps=N - 4, lr=R.LR, max_bond=R.MAX_BOND)])
    assert wa.tobytes() == wc.tobytes() and same(a.get_cores()[0], c.get_cores()[0])
    for ctx in (a, b, c, d):
        ctx.close()


# ---------------------------------------------------------------------------------------------------------------
# 6  the guard
# ---------------------------------------------------------------------------------------------------------------
def test_guard_hands_B_itself_to_the_split(built):
    """the label core's slice of class 1 is zero, so f_1 == 0 exactly, and one sample is labelled 1.  This provokes a non-finite value
    on purpose, not a fault: every kernel runs to its end."""
    case = R.CASES[0]
    cores, l, X, lab, y, S = built[R.case_id(case)]
    cores = [c.copy() for c in cores]
    cores[l][..., 1] = 0.0
    lab = np.zeros_like(lab)
    lab[4] = 1
    ctx = new_ctx(cores, l, case[1])
    f0 = NR.forward(cores, l, X.astype(np.float64))
    with pytest.raises(_hip.TnmlError) as ei:
        ctx.nll_sweep(X, lab, S, n_steps=3, lr=R.LR, max_bond=R.MAX_BOND)
    assert ei.value.code == NONFINITE and 'step 0 of 3' in str(ei.value)
    vals = ei.value.values
    assert vals[0, 2] == 1 and (vals[:, 3].astype(int) & R.NOT_APPLIED).all() and int(vals[0, 3]) & R.BAD_BATCH
    assert ctx.l_pos == l + 3
    f1 = NR.forward(dev_cores(ctx), ctx.l_pos, X.astype(np.float64))
    print('f: %.3e (bound %.0e)' % (rel(f1, f0), R.gpu_bound('f')))
    assert rel(f1, f0) <= R.gpu_bound('f')
    # the word is cleared at the start of every call
    lab[4] = 0
    vals = ctx.nll_sweep(X, lab, S, n_steps=1, lr=R.LR, max_bond=R.MAX_BOND)
    assert vals[0, 3] == 0
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------
# 7  state behind the call, refusals
# ---------------------------------------------------------------------------------------------------------------
def test_state_behind_the_call(built):
    case = R.CASES[0]
    cores, l, X, lab, y, S = built[R.case_id(case)]
    N, L = case[0], case[1]
    phi, w, _ = R.grid_metric()
    ctx = new_ctx(cores, l, L, b=len(lab))
    ctx.set_input(X, lab)
    ctx.forward()
    ctx.optim_config('sgd', momentum=0.9, clip=True)
    ctx.gd_step(X, lab, 1e-3, 0.0, 'softmax', 'full_cross_ent', 1.0)
    ctx.forward()
    ctx.nll_sweep(X, y, S, n_steps=N - 1, lr=R.LR, max_bond=R.MAX_BOND)
    assert _code(lambda: ctx.sweep(True, 1, True, 1e-3, 0.0, False, 'softmax', 'full_cross_ent', 1.0, 'fixed')) == STATE
    assert _code(lambda: ctx.update_B(None, True, 1e-3, 0.0, False, 'softmax', 'full_cross_ent', 1.0)) == STATE
    assert _code(lambda: ctx.gd_step(X, lab, 1e-3, 0.0, 'softmax', 'full_cross_ent', 1.0)) == STATE
    cs, _, lp = ctx.get_cores()
    fresh = _hip.Context(N, R.D, L, R.MAX_BOND, len(lab))
    fresh.set_any_position(True)
    fresh.set_cores(cs, lp)
    cot = np.random.default_rng(7).standard_normal((L, len(lab))).astype(np.float32)
    for name, call in (('predict', lambda c: [c.predict(X)]), ('core_grad', lambda c: c.core_grad(X, cot)[0]),
                       ('inner', lambda c: [c.inner(metric=S)]), ('log_norm_grad', lambda c: c.log_norm_grad(S)[0]),
                       ('sample', lambda c: list(c.sample(40, phi, w, seed=11)))):
        assert same(call(ctx), call(fresh)), name
    ctx.forward()
    ctx.sweep(True, 1, True, 1e-3, 0.0, False, 'softmax', 'full_cross_ent', 1.0, 'fixed')
    ctx.optim_reset()
    ctx.gd_step(X, lab, 1e-3, 0.0, 'softmax', 'full_cross_ent', 1.0)
    ctx.close()
    fresh.close()


def test_refusals(built):
    case = R.CASES[0]
    cores, l, X, lab, y, S = built[R.case_id(case)]
    N, L = case[0], case[1]
    ctx = new_ctx(cores, l, L)
    kw = dict(n_steps=1, lr=R.LR, max_bond=R.MAX_BOND)
    assert _code(lambda: ctx.nll_sweep(X, y, S, **dict(kw, max_bond=0))) == ARG
    assert _code(lambda: ctx.nll_sweep(X, y, S, **dict(kw, max_bond=R.MAX_BOND + 1))) == ARG
    assert _code(lambda: ctx.nll_sweep(X, y, S, threshold=0.0, **kw)) == ARG
    assert _code(lambda: ctx.nll_sweep(X, y, S, threshold=1.5, **kw)) == ARG
    assert _code(lambda: ctx.nll_sweep(X, y, S, renorm=2, **kw)) == ARG
    assert _code(lambda: ctx.nll_sweep(X, y, S, **dict(kw, n_steps=0))) == ARG
    assert _code(lambda: ctx.nll_sweep(X, y, S, **dict(kw, n_steps=N))) == STATE
    assert _code(lambda: ctx.nll_sweep(X, y, S, left_dir=True, **kw)) == STATE          # the label is on site 0
    assert _code(lambda: ctx.nll_sweep(X, np.full_like(lab, L), S, **kw)) == ARG
    assert _code(lambda: ctx.nll_sweep(X, y, np.array([[1.0, 0.5], [0.0, 1.0]]), **kw)) == ARG
    assert _code(lambda: ctx.nll_sweep_indices(np.arange(3), S=S, **kw)) == STATE        # no dataset
    assert _code(lambda: ctx.nll_sweep_debug('B')) == STATE                             # no step has run
    assert same(ctx.get_cores()[0], A.as32(cores)) and ctx.l_pos == l
    ctx.close()
    ctx3 = _hip.Context(4, 3, 2, 4, 64)
    rng = np.random.default_rng(0)
    ctx3.set_cores([rng.random(s).astype(np.float32) for s in NR.shapes_of(4, 3, 2, [3, 3, 3], 0)], 0)
    lib = _hip.lib()
    vals = np.zeros(6)
    X3 = np.ones((2, 4, 3), dtype=np.float32)
    rc = lib.tnml_nll_sweep(ctx3._h, _hip._ptr(X3, _hip.C.c_float), None, 2, None, 0, 1, 0.01, 1, 4, 1.0, _hip._ptr(vals, _hip.C.c_double))
    assert rc == ARG                                                                    # D = 3
    ctx3.close()


# ---------------------------------------------------------------------------------------------------------------
# 8  the Python layer
# ---------------------------------------------------------------------------------------------------------------
def test_network_methods(capsys):
    import tensornetworkforml_amd as pkg
    from tensornetworkforml_amd import data_generator as gen
    Nn, D, L, M, n = 16, 2, 2, 8, 230
    np.random.seed(3)
    data, label = gen.create_dataset(n, 4, 0.3)
    lev = np.round(np.clip(data.reshape(n, -1), 0.0, 1.0) * 255).astype(np.int32)                 # on the grid of 256 levels
    pix = (lev / 255.0).astype(np.float32)
    X = gen.psi(lev / 255.0, D)
    net = pkg.Network(N=Nn, M=M, D=D, L=L, normalize=True, calibration_X=X[:16], act_fn='softmax', loss_fn='full_cross_ent', T=1.0, trunc='fixed')
    net.attach_dataset(pix, label, pixels=True)
    start, _, lp = net._ctx.get_cores()
    _, phi, w = NR.grid(256, D)
    S = NR.gram(phi, w)
    twin = _hip.Context(Nn, D, L, M, 64)
    twin.set_cores(start, lp)
    twin.dataset_attach(pix, label, 'pixels')
    # nll_sweep: dataset indices to the end of the chain, then images with the sum log w term, three steps back
    left = lp == Nn - 1
    vals, bonds = net.nll_sweep(np.arange(50), lr=0.01)
    t = twin.nll_sweep_indices(np.arange(50), True, S, left, Nn - 1, 0.01, True, M)
    assert vals.tobytes() == t.tobytes() and bonds == twin.bonds()[0].tolist() and net.l_pos == (0 if left else Nn - 1)
    vals, bonds = net.nll_sweep(lev[50:90], label[50:90], lr=0.01, n_steps=3, renorm=False)
    t = twin.nll_sweep(X[50:90].astype(np.float32), label[50:90], S, not left, 3, 0.01, False, M)
    assert np.array_equal(vals[:, 1:], t[:, 1:]) and vals[:, 0] == pytest.approx(t[:, 0] + Nn * np.log(256.0), rel=1e-12)
    assert same(net._ctx.get_cores()[0], twin.get_cores()[0])
    with pytest.raises(ValueError):
        net.nll_sweep(np.arange(50))                                   # the label is inside the chain and no direction is given
    net.nll_sweep(np.arange(50), left_dir=left, lr=0.01)               # back to the end it came from
    assert all(np.array_equal(h.astype(np.float32), c) for h, c in zip(net.As and net._host_cores, net._ctx.get_cores()[0]))
    # train_generative(method='sweep') over two epochs: 180 training samples in batches of 50 -> 50, 50, 50, 30
    tr = gen.IndexLoader(np.arange(180), 50, shuffle=False)
    va = gen.IndexLoader(np.arange(180, n), 25, shuffle=False)
    before = net.nll(np.arange(180, n))
    val_nll, hist = net.train_generative(tr, va, lr=0.01, n_epochs=2, method='sweep')
    out = capsys.readouterr().out
    assert '--- TRAINING PROCEDURE ---' in out and 'Epoch 1/2 - train NLL' in out and 'val NLL' in out and 'largest bond' in out
    assert hist.shape == (2, 4) and len(val_nll) == 2 and np.isfinite(hist).all()
    # (M = 8 truncates in the middle of 16 sites, so single sweeps may rise; over two epochs the validation NLL falls)
    print('validation NLL before %.4f, per epoch' % before, val_nll)
    assert val_nll[-1] < before
    with pytest.raises(ValueError):
        net.train_generative(tr, va, lr=0.01, n_epochs=1, method='dmrg')


def test_script_option(tmp_path, capsys):
    from tensornetworkforml_amd import training_diagonals
    np.random.seed(11)
    val_nll, hist = training_diagonals.main(['--resident', '--objective', 'nll', '--method', 'sweep', '--max-bond', '8', '--n_samples', '1000',
                                             '--linear_dim', '4', '--M', '8', '--n_epochs', '2', '--n_train_batch', '2', '--lr', '0.01',
                                             '--L2_decay', '0', '--out', str(tmp_path / 'model.dat')])
    out = capsys.readouterr().out
    assert 'Epoch 1/2 - train NLL' in out and 'largest bond' in out and 'validation NLL per epoch' in out
    print('validation NLL per epoch', val_nll)
    assert len(val_nll) == 2 and np.isfinite(val_nll).all() and hist.shape == (2, 2) and (tmp_path / 'model.dat').exists()
    assert val_nll[1] < val_nll[0]
