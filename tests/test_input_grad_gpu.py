"""Input gradients on the GPU (include/tnml.h, tnml_input_grad / tnml_input_grad_indices), through
`_hip.Context` and `Network`.

  1  against the reference      g and cf against tests/input_grad_reference.py in float64: N in {2, 3, 17}, the label at both ends, at every
                                inner site of N = 3 and at two inner sites of N = 17, uniform and ragged bonds, b in {1, 17, 70}, a dense
                                random cotangent, for the (D, cap, L) rows below
  2  Euler identity             |sum_d g x - cf| for every site, on the device's own output
  3  bit-equalities             chunk 64 against the default chunk; cot=None against the one-hot of predict's argmax;
                                input_grad_indices(.., 'features') against input_grad on dataset_read; repeated indices
  4  pixels                     wrt='pixels' against the reference gradient times the analytic dpsi/dp, D = 2 and 3
  5  nothing else moved         f, every environment, cores, l_pos; a sweep after the call; an inner label with any_position off
  6  refusals                   each of include/tnml.h, the context usable afterwards
  7  reuse                      a larger b, a smaller b, other cores on one context

Tolerance of 1, 2 and 4: relative to max|g| of the case (max|cf| for cf and the Euler identity).  It starts from 2e-5, the bound
tests/test_forward_chain_gpu.py holds the same float32 chain arithmetic to; the bounds below are ten times the worst value
observed on an MI355X, rounded up to one digit and never above 2e-5.  Worst observed (the float32 emulation on the CPU gave
1e-7 .. 1e-6):
    (D, cap, L)     g          cf                      (D, cap, L)     g          cf
    (2, 1, 2)       3.44e-07   3.23e-07                (2, 64, 2)      1.97e-06   4.30e-07
    (2, 5, 3)       2.46e-07   4.10e-07                (2, 50, 10)     4.65e-07   5.00e-07
    (2, 20, 2)      2.07e-07   1.60e-07                (3, 7, 3)       3.00e-07   2.32e-07
    (2, 33, 2)      5.82e-07   5.87e-07                (8, 16, 17)     1.23e-06   2.78e-07
    Euler identity  3.78e-07 (2, 20, 2), 3.05e-07 (2, 50, 10), 3.70e-07 (3, 7, 3), 4.48e-07 (8, 16, 17)
    pixels          6.88e-08 (D = 2), 2.17e-07 (D = 3)
Every test prints the worst values it observed.
"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from input_grad_reference import dpsi, input_grad_reference, ragged_bonds, scaled_cores    # noqa: E402
from tensornetworkforml_amd import _hip                          # noqa: E402
from tensornetworkforml_amd import data_generator as gen         # noqa: E402

pytestmark = pytest.mark.gpu

ARG, STATE = -1, -2
TOL = 2e-5

# (D, cap, L): bonds that are no multiple of 4 or 16, the largest bond, a label core larger than LDS (50, ten labels), L > 16;
# with each row its bound for g and cf: ten times the worse of the two observed values, rounded up to one digit, at most TOL
ROWS = [(2, 1, 2), (2, 5, 3), (2, 20, 2), (2, 33, 2), (2, 64, 2), (2, 50, 10), (3, 7, 3), (8, 16, 17)]
ROW_TOL = {(2, 1, 2): 4e-6, (2, 5, 3): 5e-6, (2, 20, 2): 3e-6, (2, 33, 2): 6e-6, (2, 64, 2): 2e-5, (2, 50, 10): 6e-6, (3, 7, 3): 4e-6,
           (8, 16, 17): 2e-5}
EULER_TOL = 5e-6
PIXEL_TOL = 3e-6


def _code(call):
    with pytest.raises(_hip.TnmlError) as ei:
        call()
    return ei.value.code


def pixels(rng, b, N):
    return (rng.random((b, N)) * (rng.random((b, N)) > 0.3)).astype(np.float32)


def features(rng, b, N, D):
    return gen.psi(pixels(rng, b, N).astype(np.float64), D).astype(np.float32)


def labels_of(N):
    return {2: [0, 1], 3: [0, 1, 2], 17: [0, 5, 11, 16]}[N]


def cores_for(N, D, L, cap, l, rng, ragged):
    bond = ragged_bonds(N, cap, rng) if ragged else [cap] * (N - 1)
    return [c.astype(np.float32) for c in scaled_cores(N, D, L, bond, l, rng)]


def as64(cores):
    return [c.astype(np.float64) for c in cores]


def rel(a, ref, scale=None):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    assert a.shape == ref.shape, (a.shape, ref.shape)
    return np.abs(a - ref).max() / max(np.abs(ref).max() if scale is None else scale, 1e-300)


# ---------------------------------------------------------------------------------------------------------------
# 1. against the reference
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('row', ROWS, ids=lambda r: 'D%d-cap%d-L%d' % r)
def test_against_the_reference(row):
    D, cap, L = row
    rng = np.random.default_rng(100 * D + cap + L)
    worst = dict(g=0.0, cf=0.0)
    for N in (2, 3, 17):
        ctx = _hip.Context(N, D, L, cap, 70)
        Xall = features(rng, 70, N, D)
        for l in labels_of(N):
            for ragged in (False, True):
                cores = cores_for(N, D, L, cap, l, rng, ragged)
                ctx.set_cores(cores, l)
                for b in (1, 17, 70):
                    X = Xall[:b]
                    cot = rng.standard_normal((L, b)).astype(np.float32)
                    g, cf = ctx.input_grad(X, cot)
                    g_o, cf_o = input_grad_reference(as64(cores), l, X.astype(np.float64), cot.astype(np.float64))
                    worst['g'] = max(worst['g'], rel(g, g_o))
                    worst['cf'] = max(worst['cf'], rel(cf, cf_o))
        ctx.close()
    print('input gradient D %d cap %d L %d: g %.2e of max|g|, cf %.2e of max|cf|' % (D, cap, L, worst['g'], worst['cf']))
    assert worst['g'] <= ROW_TOL[row] and worst['cf'] <= ROW_TOL[row], worst


# ---------------------------------------------------------------------------------------------------------------
# 2. Euler identity: f is homogeneous of degree 1 in every site's vector
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('row', [(2, 20, 2), (2, 50, 10), (3, 7, 3), (8, 16, 17)], ids=lambda r: 'D%d-cap%d-L%d' % r)
def test_euler_identity(row):
    D, cap, L = row
    N, b = 17, 70
    rng = np.random.default_rng(7 + cap)
    ctx = _hip.Context(N, D, L, cap, b)
    X = features(rng, b, N, D)
    worst = 0.0
    for l in labels_of(N):
        ctx.set_cores(cores_for(N, D, L, cap, l, rng, True), l)
        g, cf = ctx.input_grad(X, rng.standard_normal((L, b)).astype(np.float32))
        per_site = np.einsum('bnd,bnd->bn', g.astype(np.float64), X.astype(np.float64))
        worst = max(worst, np.abs(per_site - cf[:, None].astype(np.float64)).max() / np.abs(cf).max())
    ctx.close()
    print('Euler identity D %d cap %d L %d: %.2e of max|cf|' % (D, cap, L, worst))
    assert worst <= EULER_TOL


# ---------------------------------------------------------------------------------------------------------------
# 3. bit-equalities
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('D,cap,L,l', [(2, 20, 2, 0), (2, 5, 3, 4), (3, 7, 3, 8)])
def test_bit_equalities(D, cap, L, l):
    N, n = 9, 60
    rng = np.random.default_rng(11 + D)
    ctx = _hip.Context(N, D, L, cap, 64)
    ctx.set_any_position(True)                                 # (for predict at an inner label; the gradient calls do not need it)
    ctx.set_cores(cores_for(N, D, L, cap, l, rng, True), l)
    for b in (70, 200):
        X = features(rng, b, N, D)
        cot = rng.standard_normal((L, b)).astype(np.float32)
        g0, cf0 = ctx.input_grad(X, cot)
        ctx.set_input_grad_chunk(64)
        g1, cf1 = ctx.input_grad(X, cot)
        ctx.set_input_grad_chunk(0)
        assert np.array_equal(g0, g1) and np.array_equal(cf0, cf1), b
        # the predicted class: first maximum of predict's f
        f = ctx.predict(X)
        onehot = np.zeros((L, b), dtype=np.float32)
        onehot[np.argmax(f, axis=0), np.arange(b)] = 1.0
        gn, cfn = ctx.input_grad(X)
        ge, cfe = ctx.input_grad(X, onehot)
        assert np.array_equal(gn, ge) and np.array_equal(cfn, cfe), b
        assert rel(cfn, f.max(axis=0)) <= TOL                  # (another order of the same contraction: equal to rounding)
    # dataset samples, repeats included
    for form in ('features', 'pixels'):
        pix = pixels(rng, n, N)
        data = pix if form == 'pixels' else gen.psi(pix.astype(np.float64), D).astype(np.float32)
        ctx.dataset_attach(data, rng.integers(0, L, n), form)
        idx = np.concatenate([rng.integers(0, n, 90), [3, 3, 3, n - 1, 0]])
        cot = rng.standard_normal((L, idx.size)).astype(np.float32)
        gi, cfi = ctx.input_grad_indices(idx, cot, 'features')
        gx, cfx = ctx.input_grad(ctx.dataset_read(idx), cot)
        assert np.array_equal(gi, gx) and np.array_equal(cfi, cfx), form
        same = np.concatenate([[7] * 70, [8] * 5])
        gs, cfs = ctx.input_grad_indices(same, None, 'features')
        assert (gs[:70] == gs[0]).all() and (cfs[:70] == cfs[0]).all() and (gs[70:] == gs[70]).all()
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------
# 4. pixels
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('D', [2, 3])
def test_gradient_with_respect_to_pixels(D):
    N, L, cap, n, l = 17, 3, 6, 80, 6
    rng = np.random.default_rng(40 + D)
    ctx = _hip.Context(N, D, L, cap, 64)
    cores = cores_for(N, D, L, cap, l, rng, True)
    ctx.set_cores(cores, l)
    pix = pixels(rng, n, N)
    pix[0, :3] = [0.0, 1.0, 0.5]
    ctx.dataset_attach(pix, rng.integers(0, L, n), 'pixels')
    idx = np.concatenate([[0], rng.integers(0, n, 74)])
    cot = rng.standard_normal((L, idx.size)).astype(np.float32)
    gp, cf = ctx.input_grad_indices(idx, cot, 'pixels')
    assert gp.shape == (idx.size, N)
    X = ctx.dataset_read(idx).astype(np.float64)
    g_o, cf_o = input_grad_reference(as64(cores), l, X, cot.astype(np.float64))
    gp_o = np.einsum('bnd,bnd->bn', g_o, dpsi(pix[idx].astype(np.float64), D))
    err = rel(gp, gp_o)
    print('pixel gradient D %d: %.2e of max|g|, cf %.2e' % (D, err, rel(cf, cf_o)))
    assert err <= PIXEL_TOL and rel(cf, cf_o) <= PIXEL_TOL
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------
# 5. nothing else moved
# ---------------------------------------------------------------------------------------------------------------
SWEEP = (1e-2, 1e-3, True, 'softmax', 'full_cross_ent', 0.1, 'fixed')


def test_resident_state_is_untouched():
    N, D, L, M, b = 12, 2, 2, 6, 100
    rng = np.random.default_rng(5)
    X, y = features(rng, b, N, D), rng.integers(0, L, b)
    other = features(rng, 300, N, D)
    cores = cores_for(N, D, L, M, 0, rng, False)
    outs = []
    for with_call in (False, True):
        ctx = _hip.Context(N, D, L, M, b)
        ctx.set_cores(cores, 0)
        ctx.set_input(X, y)
        ctx.forward()
        if with_call:
            ctx.dataset_attach(other[:50], rng.integers(0, L, 50), 'features')
            before = (ctx.get_f(), [ctx.get_env(_hip.SIDE_RIGHT, i) for i in range(1, N)], ctx.get_cores(), ctx.l_pos)
            ctx.input_grad(other)
            ctx.input_grad(other, rng.standard_normal((L, 300)).astype(np.float32))
            ctx.input_grad_indices(np.arange(50), None, 'features')
            after = (ctx.get_f(), [ctx.get_env(_hip.SIDE_RIGHT, i) for i in range(1, N)], ctx.get_cores(), ctx.l_pos)
            assert np.array_equal(before[0], after[0]) and before[3] == after[3]
            assert all(np.array_equal(a, c) for a, c in zip(before[1], after[1]))
            assert all(np.array_equal(a, c) for a, c in zip(before[2][0], after[2][0])) and np.array_equal(before[2][1], after[2][1])
        met, f = ctx.sweep(False, N - 1, True, *SWEEP)
        outs.append((met, f, ctx.get_cores()[0]))
        ctx.close()
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
    assert all(np.array_equal(a, c) for a, c in zip(outs[0][2], outs[1][2]))


def test_inner_label_without_any_position():
    N, D, L, M, l = 9, 2, 3, 5, 4
    rng = np.random.default_rng(6)
    ctx = _hip.Context(N, D, L, M, 64)
    cores = cores_for(N, D, L, M, l, rng, True)
    ctx.set_cores(cores, l)
    X = features(rng, 40, N, D)
    ctx.dataset_attach(X, rng.integers(0, L, 40), 'features')
    idx = np.arange(40)
    assert _code(lambda: ctx.predict(X)) == STATE and _code(lambda: ctx.predict_indices(idx)) == STATE
    g, cf = ctx.input_grad_indices(idx, None, 'features')
    assert _code(lambda: ctx.predict(X)) == STATE
    # the same numbers as with the switch on, where predict gives the class
    ctx.set_any_position(True)
    f = ctx.predict(X)
    g2, cf2 = ctx.input_grad(X)
    assert np.array_equal(g, g2) and np.array_equal(cf, cf2) and rel(cf, f.max(axis=0)) <= TOL
    onehot = np.zeros((L, 40))
    onehot[np.argmax(f, axis=0), np.arange(40)] = 1.0
    g_o, _ = input_grad_reference(as64(cores), l, X.astype(np.float64), onehot)
    assert rel(g, g_o) <= TOL
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------
# 6. refusals
# ---------------------------------------------------------------------------------------------------------------
def test_refusals(monkeypatch):
    import ctypes as C
    N, D, L, M = 6, 2, 3, 4
    rng = np.random.default_rng(8)
    ctx = _hip.Context(N, D, L, M, 64)
    X = features(rng, 10, N, D)
    assert _code(lambda: ctx.input_grad(X)) == STATE                                     # cores never set
    cores = cores_for(N, D, L, M, 2, rng, False)
    ctx.set_cores(cores, 2)
    lib, f32p = _hip.lib(), C.POINTER(C.c_float)
    g = np.empty((10, N, D), dtype=np.float32)
    assert lib.tnml_input_grad(ctx._h, None, 10, None, g.ctypes.data_as(f32p), None) == ARG
    assert lib.tnml_input_grad(ctx._h, X.ctypes.data_as(f32p), 10, None, None, None) == ARG
    assert lib.tnml_input_grad(ctx._h, X.ctypes.data_as(f32p), 0, None, g.ctypes.data_as(f32p), None) == ARG
    assert _code(lambda: ctx.input_grad(X[:0])) == ARG
    assert _code(lambda: ctx.input_grad_indices([0, 1])) == STATE                        # no dataset
    ctx.dataset_attach(X, rng.integers(0, L, 10), 'features')
    assert _code(lambda: ctx.input_grad_indices([0, 10])) == ARG and _code(lambda: ctx.input_grad_indices([-1])) == ARG
    assert _code(lambda: ctx.input_grad_indices([0, 1], None, 'pixels')) == STATE       # a features dataset
    assert _code(lambda: ctx.set_input_grad_chunk(-1)) == ARG
    # usable afterwards
    g1, cf1 = ctx.input_grad_indices([0, 1, 9])
    g2, cf2 = ctx.input_grad(X[[0, 1, 9]])
    assert np.array_equal(g1, g2) and np.array_equal(cf1, cf2)
    ctx.close()
    # LDS: the message names the bytes
    ctx = _hip.Context(4, 2, 2, 100, 64)
    ctx.set_cores(cores_for(4, 2, 2, 100, 0, rng, False), 0)
    with pytest.raises(_hip.TnmlError, match='bytes of LDS') as ei:
        ctx.input_grad(features(rng, 4, 4, 2))
    assert ei.value.code == ARG
    ctx.close()
    # a communicator attached: the rule of the dataset block
    from tensornetworkforml_amd import dist as tdist
    monkeypatch.setenv('TNML_FORCE_COMM', '1')
    ctx = _hip.Context(N, D, L, M, 64)
    ctx.set_cores(cores_for(N, D, L, M, 0, rng, False), 0)
    tdist.attach_comm(ctx, 0, 1)
    assert _code(lambda: ctx.input_grad(X)) == STATE and _code(lambda: ctx.input_grad_indices([0])) == STATE
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------
# 7. reuse of one context, and the Network methods
# ---------------------------------------------------------------------------------------------------------------
def test_reuse_larger_smaller_other_cores():
    N, D, L, M = 17, 2, 3, 8
    rng = np.random.default_rng(9)
    ctx = _hip.Context(N, D, L, M, 64)
    worst = 0.0
    for b, l in ((300, 3), (17, 3), (130, 16), (5, 0), (300, 9)):
        cores = cores_for(N, D, L, M, l, rng, True)
        ctx.set_cores(cores, l)
        X = features(rng, b, N, D)
        cot = rng.standard_normal((L, b)).astype(np.float32)
        g, cf = ctx.input_grad(X, cot)
        g_o, cf_o = input_grad_reference(as64(cores), l, X.astype(np.float64), cot.astype(np.float64))
        worst = max(worst, rel(g, g_o), rel(cf, cf_o))
    ctx.close()
    print('reuse: worst %.2e' % worst)
    assert worst <= TOL


def test_network_methods():
    import tensornetworkforml_amd as pkg
    N, D, L, M, b = 16, 2, 3, 4, 30
    np.random.seed(3)
    rng = np.random.default_rng(10)
    pix = pixels(rng, 50, N)
    X = gen.psi(pix.astype(np.float64), D)
    net = pkg.Network(N=N, M=M, D=D, L=L, normalize=True, calibration_X=X[:16], act_fn='softmax', loss_fn='full_cross_ent', trunc='fixed')
    f = np.asarray(net.predict(X[:b]).elem)
    cores = as64(net._ctx.get_cores()[0])                      # the calibrated cores as the device holds them
    g, cf = net.input_gradient(X[:b], return_cf=True)
    assert g.shape == (b, N, D) and rel(cf, f.max(axis=0)) <= TOL
    cls = rng.integers(0, L, b)
    g_c = net.input_gradient(X[:b], cls)
    onehot = np.zeros((L, b))
    onehot[cls, np.arange(b)] = 1.0
    g_o, _ = input_grad_reference(cores, net.l_pos, X[:b].astype(np.float32).astype(np.float64), onehot)
    assert rel(g_c, g_o) <= TOL
    dense = rng.standard_normal((L, b))
    assert np.array_equal(net.input_gradient(X[:b], onehot.astype(np.float32)), g_c)
    assert net.input_gradient(X[:b], dense).shape == (b, N, D)
    # a user edit of As reaches the device first, as in predict
    As = net.As
    As[3].elem *= 2.0
    g2 = net.input_gradient(X[:b], cls)
    assert rel(g2, 2.0 * g_o) <= 2 * TOL
    net.attach_dataset(pix, rng.integers(0, L, 50), pixels=True)
    sal = net.input_gradient_indices(np.arange(b), cls)
    assert sal.shape == (b, N)
    gf = net.input_gradient_indices(np.arange(b), cls, wrt='features')
    Xd = net._ctx.dataset_read(np.arange(b)).astype(np.float64)
    g_o2, _ = input_grad_reference(cores, net.l_pos, Xd, onehot)
    assert rel(gf, 2.0 * g_o2) <= 2 * TOL
    assert rel(sal, 2.0 * np.einsum('bnd,bnd->bn', g_o2, dpsi(pix[:b].astype(np.float64), D))) <= 2 * TOL


def test_evaluation_script_writes_saliency_maps(tmp_path, monkeypatch):
    """evaluate_binary_MNIST.py --saliency OUT.npy: the maps of the script are Network.input_gradient_indices over the test digits."""
    import contextlib
    import io
    import pickle
    from tensornetworkforml_amd import training_binary_MNIST as train_script
    from tensornetworkforml_amd import evaluate_binary_MNIST as eval_script
    from test_network_gpu import _synthetic_mnist
    root = str(tmp_path / 'datasets')
    _synthetic_mnist(root, 600, 200, 5)
    monkeypatch.chdir(tmp_path)
    out, sal_file = str(tmp_path / 'mnist.dat'), str(tmp_path / 'saliency.npy')
    np.random.seed(4)
    with contextlib.redirect_stdout(io.StringIO()):
        train_script.main(['--data_dir', root, '--n_epochs', '1', '--n_train_batch', '2', '--normalise', '--lr', '0.01', '--L2_decay', '1e-3',
                           '--resident', '--out', out])
        acc, mae = eval_script.main(['--filename', out, '--data_dir', root, '--normalise', '--batch_size', '100', '--saliency', sal_file])
        acc2, mae2 = eval_script.main(['--filename', out, '--data_dir', root, '--normalise', '--batch_size', '100'])
    assert (acc, mae) == (acc2, mae2)
    sal = np.load(sal_file)
    _, _, te, tel = gen.get_MNIST_dataset(root)
    mask = tel < 2
    assert sal.shape == (int(mask.sum()), 14, 14) and sal.dtype == np.float32 and np.isfinite(sal).all() and np.abs(sal).max() > 0
    with open(out, 'rb') as fh:
        net = pickle.load(fh)
    net.attach_dataset(eval_script.pooling(te)[mask] / 255.0, tel[mask], pixels=True)
    assert np.array_equal(net.input_gradient_indices(np.arange(int(mask.sum()))), sal.reshape(len(sal), -1))
