"""Local feature dimensions D = 3 .. 8 on the device (the generic-D path, kernels_anyd.hip) against the float64 oracle.

Bounds as in test_hip_parity.py's stepwise test: B / dB_raw / L2_grad / B_new 5e-3 of max|.| after the +-1 gauge of the SVD,
sigma 2e-3 of sigma_max, f 5e-3, accuracy exact, MAE 2e-3.  Forward environments 2e-5.
"""
import os
import pickle
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import golden_util as gu
from oracle import mps_oracle as mo

pytestmark = pytest.mark.gpu

L2_TERM_TOL = 1e-5      # tnml_l2_term against mo.compute_L2_reg (also the bound of tests/test_context_lifecycle_gpu.py's carried pairs)


def hip():
    from tensornetworkforml_amd import _hip
    return _hip


def relerr(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def embed(u, D):
    from tensornetworkforml_amd import data_generator as gen
    return gen.psi(u, D)


def problem(N, M, D, L, b, seed=0, calibrate=True):
    """Sparse-ish pixels embedded at D, U[0,1) cores scaled as Network(normalize=True), calibrated in float64; the float32 cores
    are the common start of device and oracle."""
    rng = np.random.default_rng(seed)
    u = rng.random((b, N)) * (rng.random((b, N)) > 0.5)
    X = embed(u, D).astype(np.float32)
    y = rng.integers(0, L, b)
    cores = mo.random_cores(N, M, D, L, rng=rng, scale=M * 0.5 * 0.64 * D)
    if calibrate:
        st = mo.MPSState(N, D, L, M, cores)
        mo.calibrate(st, X.astype(np.float64))
        cores = st.cores
    cores32 = [c.astype(np.float32) for c in cores]
    return X, y, cores32


def make(N, M, D, L, X, y, cores32, l_pos=0):
    ctx = hip().Context(N, D, L, M, X.shape[0])
    ctx.set_cores(cores32, l_pos)
    ctx.set_input(X, y)
    st = mo.MPSState(N, D, L, M, [c.astype(np.float64) for c in cores32], l_pos)
    return ctx, st


# ---- forward / predict ------------------------------------------------------------------------------------
@pytest.mark.parametrize('D,M,N,L', [(3, 6, 10, 2), (4, 5, 9, 3), (8, 4, 7, 2), (3, 20, 16, 10)])
def test_forward_envs_predict(D, M, N, L):
    X, y, c32 = problem(N, M, D, L, 100)
    ctx, st = make(N, M, D, L, X, y, c32)
    for left in (False, True):
        if left:
            c32b = [np.ascontiguousarray(c) for c in c32]
            # label on the last site: move it there on both sides with a fresh random network of that layout
            rng = np.random.default_rng(1)
            cores = [rng.random(c.shape if i not in (0, N - 1) else ((1, D, M) if i == 0 else (M, D, 1, L))) / (M * 0.64 * D)
                     for i, c in enumerate(c32b)]
            cores = [c.astype(np.float32) for c in cores]
            ctx.set_cores(cores, N - 1)
            st = mo.MPSState(N, D, L, M, [c.astype(np.float64) for c in cores], N - 1)
        f_o = mo.forward(st, X.astype(np.float64))
        f_d = ctx.forward()
        assert relerr(f_d, f_o) < 2e-5
        envs = st.Lenv if left else st.Renv
        side = hip().SIDE_LEFT if left else hip().SIDE_RIGHT
        for site, e in envs.items():
            assert relerr(ctx.get_env(side, site), e) < 2e-5, site
        assert np.array_equal(ctx.predict(X), f_d)


def test_calibration_logabsmax_N784():
    D, M, N, L, b = 3, 10, 784, 2, 64
    rng = np.random.default_rng(3)
    u = rng.random((b, N))
    X = embed(u, D).astype(np.float32)
    cores = [c.astype(np.float32) for c in mo.random_cores(N, M, D, L, rng=rng, scale=M * 0.5 * 0.64 * D)]
    ctx, st = make(N, M, D, L, X, np.zeros(b, np.int64), cores)
    lm = ctx.forward_logabsmax()
    # the value itself: log max|f| of the un-calibrated float64 chain (~1e-60 here, far inside float64's range)
    f_raw = mo.forward(st, X.astype(np.float64))
    lm_o = float(np.log(np.abs(f_raw).max()))
    assert np.isfinite(lm_o) and abs(lm - lm_o) < 1e-4 * max(1.0, abs(lm_o)), (lm, lm_o)
    # float64 oracle with the same per-site renormalisation is not needed: scale the cores by the device's factor and compare f
    F2 = float(np.exp(lm / N))
    ctx.scale_cores(1.0 / F2)
    st.cores = [c / F2 for c in st.cores]
    f_o = mo.forward(st, X.astype(np.float64))
    assert 0.1 < np.abs(f_o).max() < 10.0
    assert relerr(ctx.forward(), f_o) < 1e-4


# ---- step by step vs the oracle ------------------------------------------------------------------------------
def stepwise(D, M, N, L, b, act, loss, trunc, n_sweeps=2, lr=1e-2, wd=1e-3):
    X, y, c32 = problem(N, M, D, L, b)
    ctx, st = make(N, M, D, L, X, y, c32)
    ctx.debug_enable(True)
    kw = dict(lr=lr, weight_dec=wd, L2_flag=True, act_fn=act, loss_fn=loss, T=0.1, trunc=trunc)
    y1h = mo.one_hot(y, L)
    worst = {}
    degenerate = False

    def upd(k, v):
        worst[k] = max(worst.get(k, 0.0), v)

    Xd = X.astype(np.float64)
    for sw in range(n_sweeps):
        f_o = mo.forward(st, Xd)
        upd('f_forward', relerr(ctx.forward(), f_o))
        left = st.l_pos == N - 1
        if left:
            st.Renv = {}
        else:
            st.Lenv = {}
        for j in range(N - 1):
            rec = {}
            f_o = mo.sweep_step(st, f_o, y1h, left_dir=left, record=rec, **kw)
            met, f_d = ctx.sweep(left, 1, j == 0, lr, wd, True, act, loss, 0.1, trunc)
            shp = rec['B'].shape
            if not degenerate:
                B_d = ctx.step_debug('B').reshape(shp)
                sa, tc = gu.gauge_signs(B_d, rec['B'])
                for key in ('B', 'dB_raw', 'L2_grad', 'B_new'):
                    upd(key, relerr(ctx.step_debug(key).reshape(shp), gu.regauge(rec[key], sa, tc)))
            Sk = rec['S'][:rec['m'] + 1]
            if len(Sk) > 1 and np.min(-np.diff(Sk)) < 2e-3 * rec['S'][0]:
                degenerate = True
            upd('sigma', np.abs(ctx.step_debug('sigma') - rec['S']).max() / rec['S'].max())
            upd('f_new', relerr(f_d, f_o))
            upd('acc', abs(float(met[0, 0]) - rec['accuracy']))
            upd('MAE', abs(float(met[0, 1]) - rec['MAE']))
            assert ctx.l_pos == st.l_pos
        _, bond_d, _ = ctx.get_cores()
        assert list(bond_d) == list(st.bond)
    print(D, M, N, act, loss, trunc, {k: '%.2e' % v for k, v in worst.items()})
    for key in ('B', 'dB_raw', 'L2_grad', 'B_new'):
        assert worst.get(key, 0.0) < 5e-3, (key, worst)
    assert worst['sigma'] < 2e-3, worst
    assert worst['f_new'] < 5e-3 and worst['f_forward'] < 5e-3, worst
    assert worst['acc'] < 1e-6, worst          # the same count (float32 rounding of the fraction)
    assert worst['MAE'] < 2e-3, worst
    return ctx, st


@pytest.mark.parametrize('D,M,N,L,act,loss,trunc', [
    (3, 6, 10, 2, 'softmax', 'full_cross_ent', 'fixed'),
    (3, 5, 9, 2, 'linear', 'MSE', 'fixed'),                 # odd bond: odd matrix sides everywhere
    (3, 6, 8, 2, 'softmax', 'full_cross_ent', 'reference'),  # chain ends: rows = 3 at l_pos = 0
    (3, 6, 10, 3, 'linear', 'MSE', 'adaptive'),
    (4, 5, 9, 2, 'softmax', 'full_cross_ent', 'fixed'),
    (4, 4, 8, 2, 'linear', 'MSE', 'reference'),
    (4, 6, 8, 2, 'softmax', 'full_cross_ent', 'adaptive'),
])
def test_stepwise_vs_oracle(D, M, N, L, act, loss, trunc):
    stepwise(D, M, N, L, 200, act, loss, trunc)


def test_whole_sweeps_ragged_batch():
    D, M, N, L, b = 3, 8, 14, 2, 333
    X, y, c32 = problem(N, M, D, L, b, seed=5)
    ctx, st = make(N, M, D, L, X, y, c32)
    Xd = X.astype(np.float64)
    for sw in range(3):
        f_o = mo.forward(st, Xd)
        ctx.forward()
        left = st.l_pos == N - 1
        vh = ([], [])
        f_o = mo.sweep(st, Xd, y, f_o, 1e-2, 1e-3, L2_flag=True, left_dir=left, var_hist=vh, act_fn='softmax',
                       loss_fn='full_cross_ent', T=0.1, trunc='fixed')
        met, f_d = ctx.sweep(left, N - 1, True, 1e-2, 1e-3, True, 'softmax', 'full_cross_ent', 0.1, 'fixed')
        assert relerr(f_d, f_o) < 5e-3, sw
        assert np.abs(met[:, 0] - np.array(vh[0])).max() < 1e-6
        assert np.abs(met[:, 1] - np.array(vh[1])).max() < 2e-3
        assert list(ctx.get_cores()[1]) == list(st.bond)
    X2 = embed(np.random.default_rng(9).random((50, N)), D).astype(np.float32)
    assert relerr(ctx.predict(X2), mo.forward(st, X2.astype(np.float64))) < 5e-3


# ---- standalone calls ------------------------------------------------------------------------------------------
def test_standalone_update_l2_svd():
    D, M, N, L, b = 3, 6, 8, 2, 150
    X, y, c32 = problem(N, M, D, L, b, seed=7)
    ctx, st = make(N, M, D, L, X, y, c32)
    f = ctx.forward()
    f_o = mo.forward(st, X.astype(np.float64))
    # update_B on sites (0, 1)
    Bnew, met = ctx.update_B(None, False, 1e-2, 1e-3, True, 'softmax', 'full_cross_ent', 0.1)
    rec = {}
    st2 = st.copy()
    st2.Lenv = {}
    mo.sweep_step(st2, f_o, mo.one_hot(y, L), lr=1e-2, weight_dec=1e-3, L2_flag=True, left_dir=False, act_fn='softmax',
                  loss_fn='full_cross_ent', T=0.1, trunc='fixed', record=rec)
    Bn = Bnew[:rec['B_new'].size].reshape(rec['B_new'].shape)
    assert relerr(Bn, rec['B_new']) < 5e-3
    assert abs(float(met[0]) - rec['accuracy']) < 1e-6
    # l2 term of the merged tensor at l_pos = 0
    B = rec['B'].astype(np.float32)
    loss, grad = ctx.l2_term(B, False, 1e-3)
    loss_o, grad_o = mo.compute_L2_reg(st.copy(), B.astype(np.float64), 0, 1e-3)
    assert relerr(grad, grad_o) < L2_TERM_TOL and abs(loss - loss_o) <= L2_TERM_TOL * abs(loss_o)
    # svd split, odd and even sides (a context whose buffers hold the larger matrices)
    rng = np.random.default_rng(11)
    big = hip().Context(N, D, L, 32, 64)
    # (short sides 105 / 108 / 126: padded size above 100 keeps the Jacobi eigenvectors in HBM instead of LDS)
    for rows, cols, m in ((9, 15, 5), (12, 30, 12), (21, 9, 7), (27, 27, 20), (3, 96, 3), (108, 120, 50), (105, 120, 105),
                          (129, 126, 40)):
        A = rng.standard_normal((rows, cols)).astype(np.float32)
        US, SVh, sig = big.svd_split(A, m)
        S = np.linalg.svd(A.astype(np.float64), compute_uv=False)
        assert np.abs(sig[:m] - S[:m]).max() < 1e-5 * S[0], (rows, cols, m)          # kept singular values
        assert np.abs(sig - S).max() < 2e-3 * S[0], (rows, cols, m)                 # the discarded ones are only separated
        U, S2, Vh = np.linalg.svd(A.astype(np.float64), full_matrices=False)
        best = (U[:, :m] * S2[:m]) @ Vh[:m]
        assert relerr(US.astype(np.float64) @ SVh, best) < 1e-4


# ---- limits ----------------------------------------------------------------------------------------------------
def test_size_limit_and_multi_gpu_refused():
    """D = 4: bond 32 reaches a short side of 128 and runs; bond 33 fails with TNML_ERR_ARG at the first step whose short side
    exceeds 128 (the steps before it run)."""
    D, N, L, b = 4, 6, 2, 64
    for M, ok in ((32, True), (33, False)):
        X, y, c32 = problem(N, M, D, L, b, seed=2)
        ctx, st = make(N, M, D, L, X, y, c32)
        ctx.forward()
        n_max, raised = 0, False
        for j in range(N - 1):
            _, bond, lp = ctx.get_cores()
            h = 1 if lp == 0 else int(bond[lp - 1])
            g = 1 if lp + 1 == N - 1 else int(bond[lp + 1])
            n = min(D * h, D * g * L)
            if n > 128:
                with pytest.raises(hip().TnmlError) as ei:
                    ctx.sweep(False, 1, j == 0, 1e-2, 1e-3, True, 'softmax', 'full_cross_ent', 0.1, 'fixed')
                assert ei.value.code == -1 and '128' in str(ei.value)
                raised = True
                break
            ctx.sweep(False, 1, j == 0, 1e-2, 1e-3, True, 'softmax', 'full_cross_ent', 0.1, 'fixed')
            n_max = max(n_max, n)
        assert raised == (not ok)
        if ok:
            assert n_max == 128 and ctx.l_pos == N - 1
        ctx.close()
    X, y, c32 = problem(6, 4, 3, 2, 32)
    ctx, _ = make(6, 4, 3, 2, X, y, c32)
    with pytest.raises(hip().TnmlError) as ei:
        ctx.comm_init(0, 2, hip().comm_unique_id())
    assert ei.value.code == -2


# ---- Network API -----------------------------------------------------------------------------------------------
def test_network_diagonals_D3_matches_oracle(tmp_path):
    """lr = 1e-3: at lr = 1e-2 the float32 and float64 trajectories of this problem part after a few sweeps (the D = 2 path
    parts from the oracle there too, by one validation sample in the third epoch)."""
    import tensornetworkforml_amd as tn
    from tensornetworkforml_amd import data_generator as gen
    D = 3
    np.random.seed(0)
    data, label = gen.create_dataset(1500, 5, 0.5)
    train_loader, val_loader, _ = gen.prepare_dataset(data, label, 1, 0.2, 400, 150, 150, D=D)   # 300 validation samples
    np.random.seed(1)
    net = tn.Network(N=25, M=6, D=D, L=2, normalize=True, act_fn='softmax', loss_fn='full_cross_ent', trunc='fixed')
    cores0 = [c.astype(np.float64) for c in net._context(1).get_cores()[0]]
    st = mo.MPSState(25, D, 2, 6, cores0, 0)
    # the same batches for both: fix the loader orders by recording them
    batches = [[(b.X, b.y) for b in train_loader] for _ in range(3)]
    vals = [(b.X, b.y) for b in val_loader]
    acc0 = sum(int((np.argmax(mo.forward(st, X), 0) == y).sum()) for X, y in vals) / sum(len(y) for _, y in vals)
    f0 = np.asarray(net.forward(vals[0][0]).elem).copy()

    class Fixed:
        def __init__(self, bs):
            self.bs = bs

        def __len__(self):
            return len(self.bs)

        def __iter__(self):
            for X, y in self.bs:
                out = gen.Batch((X[i], y[i]) for i in range(len(y)))
                out.X, out.y = X, y
                yield out

    acc_d, acc_o = [], []
    for ep in range(3):
        acc_d.append(net.train(Fixed(batches[ep]), Fixed(vals), lr=1e-3, n_epochs=1, weight_dec=1e-3)[0][-1])
        for X, y in batches[ep]:
            f = mo.forward(st, X)
            mo.sweep(st, X, y, f, 1e-3, 1e-3, L2_flag=True, left_dir=st.l_pos == 24, act_fn='softmax',
                     loss_fn='full_cross_ent', T=0.1, trunc='fixed')
        correct = sum(int((np.argmax(mo.forward(st, X), 0) == y).sum()) for X, y in vals)
        acc_o.append(correct / sum(len(y) for _, y in vals))
    assert np.abs(np.array(acc_d) - np.array(acc_o)).max() <= 0.005, (acc_d, acc_o)      # one sample of 300 at the most
    # and training did something: the accuracy moved and the network function changed
    assert abs(acc_d[-1] - acc0) >= 0.05, (acc0, acc_d)
    assert relerr(np.asarray(net.forward(vals[0][0]).elem), f0) > 0.05
    p = tmp_path / 'net.dat'
    with open(p, 'wb') as fh:
        pickle.dump(net, fh)
    with open(p, 'rb') as fh:
        net2 = pickle.load(fh)
    Xv = vals[0][0]
    assert np.array_equal(np.asarray(net2.forward(Xv).elem), np.asarray(net.forward(Xv).elem))
