"""Core gradients on the GPU (include/tnml.h, tnml_core_grad / tnml_core_grad_indices), through
`_hip.Context` and `Network`.

  1  against the reference      G per core and cf against tests/core_grad_reference.py in float64: N in {2, 3, 17}, the label at both
                                ends, at the inner site of N = 3 and at two inner sites of N = 17, uniform and ragged bonds,
                                b in {1, 17, 70}, a dense random cotangent, for the (D, cap, L) rows below
  2  Euler identity             |sum(G_i A_i) - sum_s cf| for every site, on the device's own output, four rows
  3  tie to the input gradient  sum_{a,c} G_i[a][d][c] A_i[a][d][c] = sum_s x[s][i][d] g[s][i][d] for every site and d, G from
                                core_grad and g from input_grad on the same X and cot; cf of the two calls bit-equal (one device
                                body runs both chains)
  4  bit-equalities             chunk 64 against the default chunk (b = 70, 200); the same call twice; cot=None against the one-hot
                                of predict's first maximum; core_grad_indices against core_grad on dataset_read; a capacity larger
                                than needed leaves the floats behind the gradient alone
  5  three plain updates        A_i += lr G_i three times against the same in float64 NumPy
  6  nothing else moved         f, every environment, cores, l_pos; a sweep after the call; input_grad before and after
  7  refusals                   each of include/tnml.h, the context usable afterwards
  8  reuse                      a larger b, a smaller b, other cores and bonds on one context

Tolerances.  G is measured relative to max|G| over all cores of a case, cf relative to max|cf|; the Euler identity relative to
sum_s |cf[s]|, the tie relative to the largest sum_s |x g| over (site, d): the natural scale of a sum's rounding error.  The bounds
start from 2e-5, what tests/test_forward_chain_gpu.py holds the same float32 chain arithmetic to; each bound below is ten times the
worst value observed on an MI355X against the float64 reference, rounded up to one digit (the factor covers other seeds and other
summation lengths: the rule of tests/test_input_grad_gpu.py).  Every bound for G stays within 2e-5.  Three bounds for cf do not:
(2, 1, 2), (2, 33, 2) and (2, 50, 10).  The responsible term is the sum over the labels in cf[s] = sum_l' cot[l'][s] f[l'][s] at
b = 1, where max|cf| is the one |cf| there is: with a mixed-sign cotangent the terms cancel, and sum_l' |cot f| / |cf| is 254, 77
and 7017 in the worst case of those rows (N = 2 or 3, computed in float64), so a rounding error of 3e-8, 3e-8 and 3e-9 of the terms
shows as 7e-6, 2e-6 and 2e-5 of the result.  Worst observed:
    (D, cap, L)     G          cf                      (D, cap, L)     G          cf
    (2, 1, 2)       5.49e-07   7.17e-06                (2, 64, 2)      1.03e-06   2.51e-07
    (2, 5, 3)       3.73e-07   6.87e-07                (2, 50, 10)     7.12e-07   1.89e-05
    (2, 20, 2)      7.36e-07   3.61e-07                (3, 7, 3)       5.59e-07   4.26e-07
    (2, 33, 2)      1.03e-06   2.19e-06                (8, 16, 17)     7.18e-07   3.59e-07
    Euler identity  3.65e-08 (2, 20, 2), 7.48e-08 (2, 50, 10), 8.12e-08 (3, 7, 3), 1.18e-07 (8, 16, 17)
    tie             3.20e-08 (2, 20, 2), 4.01e-08 (2, 50, 10), 3.48e-08 (3, 7, 3), 5.13e-08 (8, 16, 17)
    three updates   5.40e-08 of max|A|
Every test prints the worst values it observed.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from core_grad_reference import core_grad_reference               # noqa: E402
from input_grad_reference import ragged_bonds, scaled_cores       # noqa: E402
from tensornetworkforml_amd import _hip                           # noqa: E402
from tensornetworkforml_amd import data_generator as gen          # noqa: E402

pytestmark = pytest.mark.gpu

ARG, STATE = -1, -2
TOL = 2e-5

# (D, cap, L): one tile, bonds that are no multiple of 16, a partial second column tile (20), an odd number of tiles (33: 66 rows make
# five row tiles), the largest bond, a label core larger than LDS (50, ten labels), D = 3, and D = 8 with 128 output rows and L > 16;
# with each row its bounds for G and cf: ten times the observed value, rounded up to one digit (see the head of the file)
ROWS = [(2, 1, 2), (2, 5, 3), (2, 20, 2), (2, 33, 2), (2, 64, 2), (2, 50, 10), (3, 7, 3), (8, 16, 17)]
ROW_TOL_G = {(2, 1, 2): 6e-6, (2, 5, 3): 4e-6, (2, 20, 2): 8e-6, (2, 33, 2): 2e-5, (2, 64, 2): 2e-5, (2, 50, 10): 8e-6, (3, 7, 3): 6e-6,
             (8, 16, 17): 8e-6}
ROW_TOL_CF = {(2, 1, 2): 8e-5, (2, 5, 3): 7e-6, (2, 20, 2): 4e-6, (2, 33, 2): 3e-5, (2, 64, 2): 3e-6, (2, 50, 10): 2e-4, (3, 7, 3): 5e-6,
              (8, 16, 17): 4e-6}
EULER_TOL = 2e-6
TIE_TOL = 6e-7
UPDATE_TOL = 6e-7


def _code(call):
    with pytest.raises(_hip.TnmlError) as ei:
        call()
    return ei.value.code


def pixels(rng, b, N):
    return (rng.random((b, N)) * (rng.random((b, N)) > 0.3)).astype(np.float32)


def features(rng, b, N, D):
    return np.ascontiguousarray(gen.psi(pixels(rng, b, N).astype(np.float64), D), dtype=np.float32)    # (raw ctypes calls below)


def labels_of(N):
    return {2: [0, 1], 3: [0, 1, 2], 17: [0, 5, 11, 16]}[N]


def cores_for(N, D, L, cap, l, rng, ragged):
    bond = ragged_bonds(N, cap, rng) if ragged else [cap] * (N - 1)
    return [c.astype(np.float32) for c in scaled_cores(N, D, L, bond, l, rng)]


def as64(a):
    return [c.astype(np.float64) for c in a]


def rel(a, ref, scale=None):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    assert a.shape == ref.shape, (a.shape, ref.shape)
    return np.abs(a - ref).max() / max(np.abs(ref).max() if scale is None else scale, 1e-300)


def rel_cores(G, G_ref):
    """the worst element of any core, relative to max|G_ref| over all cores"""
    scale = max(np.abs(g).max() for g in G_ref)
    assert len(G) == len(G_ref)
    return max(rel(g, r, scale) for g, r in zip(G, G_ref))


def same_cores(G0, G1):
    return len(G0) == len(G1) and all(np.array_equal(a, c) for a, c in zip(G0, G1))


# ---------------------------------------------------------------------------------------------------------------
# 1. against the reference
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('row', ROWS, ids=lambda r: 'D%d-cap%d-L%d' % r)
def test_against_the_reference(row):
    D, cap, L = row
    rng = np.random.default_rng(200 * D + cap + L)
    worst = dict(G=0.0, cf=0.0)
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
                    G, cf = ctx.core_grad(X, cot)
                    G_o, cf_o = core_grad_reference(as64(cores), l, X.astype(np.float64), cot.astype(np.float64))
                    assert [g.shape for g in G] == [c.shape for c in cores] and all(g.dtype == np.float32 for g in G)
                    worst['G'] = max(worst['G'], rel_cores(G, G_o))
                    worst['cf'] = max(worst['cf'], rel(cf, cf_o))
        ctx.close()
    print('core gradient D %d cap %d L %d: G %.2e of max|G|, cf %.2e of max|cf|' % (D, cap, L, worst['G'], worst['cf']))
    assert worst['G'] <= ROW_TOL_G[row] and worst['cf'] <= ROW_TOL_CF[row], worst


# ---------------------------------------------------------------------------------------------------------------
# 2. Euler identity: f is homogeneous of degree 1 in every core
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('row', [(2, 20, 2), (2, 50, 10), (3, 7, 3), (8, 16, 17)], ids=lambda r: 'D%d-cap%d-L%d' % r)
def test_euler_identity(row):
    D, cap, L = row
    N, b = 17, 70
    rng = np.random.default_rng(17 + cap)
    ctx = _hip.Context(N, D, L, cap, b)
    X = features(rng, b, N, D)
    worst = 0.0
    for l in labels_of(N):
        cores = cores_for(N, D, L, cap, l, rng, True)
        ctx.set_cores(cores, l)
        G, cf = ctx.core_grad(X, rng.standard_normal((L, b)).astype(np.float32))
        cf = cf.astype(np.float64)
        per_site = np.array([(g.astype(np.float64) * a.astype(np.float64)).sum() for g, a in zip(G, cores)])
        worst = max(worst, np.abs(per_site - cf.sum()).max() / np.abs(cf).sum())
    ctx.close()
    print('Euler identity D %d cap %d L %d: %.2e of sum|cf|' % (D, cap, L, worst))
    assert worst <= EULER_TOL


# ---------------------------------------------------------------------------------------------------------------
# 3. tie to the input gradient, both from the device
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('row', [(2, 20, 2), (2, 50, 10), (3, 7, 3), (8, 16, 17)], ids=lambda r: 'D%d-cap%d-L%d' % r)
def test_tie_to_the_input_gradient(row):
    D, cap, L = row
    N, b = 17, 70
    rng = np.random.default_rng(23 + cap)
    ctx = _hip.Context(N, D, L, cap, b)
    X = features(rng, b, N, D)
    worst = 0.0
    for l in labels_of(N):
        cores = cores_for(N, D, L, cap, l, rng, True)
        ctx.set_cores(cores, l)
        cot = rng.standard_normal((L, b)).astype(np.float32)
        G, cf_core = ctx.core_grad(X, cot)
        g, cf_input = ctx.input_grad(X, cot)
        assert np.array_equal(cf_core, cf_input)                   # one device body computes both (csrc/grad_chain_device.h)
        terms = X.astype(np.float64) * g.astype(np.float64)                                      # (b, N, D)
        lhs = np.array([(G[i].astype(np.float64) * cores[i].astype(np.float64)).sum(axis=(0, 2, 3) if i == l else (0, 2)) for i in range(N)])
        worst = max(worst, np.abs(lhs - terms.sum(0)).max() / np.abs(terms).sum(0).max())
    ctx.close()
    print('tie to the input gradient D %d cap %d L %d: %.2e of max sum|x g|' % (D, cap, L, worst))
    assert worst <= TIE_TOL


# ---------------------------------------------------------------------------------------------------------------
# 4. bit-equalities
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('D,cap,L,l', [(2, 20, 2, 0), (2, 5, 3, 4), (3, 7, 3, 8)])
def test_bit_equalities(D, cap, L, l):
    N, n = 9, 60
    rng = np.random.default_rng(31 + D)
    ctx = _hip.Context(N, D, L, cap, 64)
    ctx.set_any_position(True)                                 # (for predict at an inner label; the gradient calls do not need it)
    cores = cores_for(N, D, L, cap, l, rng, True)
    ctx.set_cores(cores, l)
    total = sum(c.size for c in cores)
    f32p = C.POINTER(C.c_float)
    for b in (70, 200):
        X = features(rng, b, N, D)
        cot = rng.standard_normal((L, b)).astype(np.float32)
        G0, cf0 = ctx.core_grad(X, cot)
        ctx.set_core_grad_chunk(64)                            # two and four chunks: the accumulators are handed over through G
        G1, cf1 = ctx.core_grad(X, cot)
        ctx.set_core_grad_chunk(0)
        assert same_cores(G0, G1) and np.array_equal(cf0, cf1), b
        G2, cf2 = ctx.core_grad(X, cot)                        # the same call twice
        assert same_cores(G0, G2) and np.array_equal(cf0, cf2), b
        # the predicted class: first maximum of predict's f
        f = ctx.predict(X)
        onehot = np.zeros((L, b), dtype=np.float32)
        onehot[np.argmax(f, axis=0), np.arange(b)] = 1.0
        Gn, cfn = ctx.core_grad(X)
        Ge, cfe = ctx.core_grad(X, onehot)
        assert same_cores(Gn, Ge) and np.array_equal(cfn, cfe), b
        assert rel(cfn, f.max(axis=0)) <= TOL                  # (another order of the same contraction: equal to rounding)
        # a capacity larger than needed: the floats behind the gradient are untouched
        flat = np.full(total + 37, -7.5, dtype=np.float32)
        rc = _hip.lib().tnml_core_grad(ctx._h, X.ctypes.data_as(f32p), b, cot.ctypes.data_as(f32p), flat.ctypes.data_as(f32p), flat.size, None)
        assert rc == 0 and (flat[total:] == -7.5).all()
        assert np.array_equal(flat[:total], np.concatenate([g.ravel() for g in G0]))
    # dataset samples, repeats included
    X = features(rng, n, N, D)
    ctx.dataset_attach(X, rng.integers(0, L, n), 'features')
    idx = np.concatenate([rng.integers(0, n, 90), [3, 3, 3, n - 1, 0]])
    cot = rng.standard_normal((L, idx.size)).astype(np.float32)
    Gi, cfi = ctx.core_grad_indices(idx, cot)
    Gx, cfx = ctx.core_grad(ctx.dataset_read(idx), cot)
    assert same_cores(Gi, Gx) and np.array_equal(cfi, cfx)
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------
# 5. three plain updates
# ---------------------------------------------------------------------------------------------------------------
def test_three_plain_updates():
    """A_i += lr G_i with cot = onehot(y) - f, which is what compute_loss_derivate gives for the MSE loss of a linear output (the
    library's derivative is the descent direction).  lr = 3e-5 was chosen on the CPU (max|G| is about 600 at the start, the cores are
    of order 1): the float64 run's mean squared error falls 20.3 -> 8.3 -> 5.4 -> 4.0, and the test asserts that it falls at each
    step.  The cores are compared relative to max|A| over all cores."""
    N, D, L, M, b, lr = 8, 2, 2, 4, 70, 3e-5
    rng = np.random.default_rng(55)
    X = features(rng, b, N, D)
    y1h = np.zeros((L, b))
    y1h[rng.integers(0, L, b), np.arange(b)] = 1.0
    start = [c.astype(np.float32) for c in scaled_cores(N, D, L, [M] * (N - 1), 0, rng)]

    def forward64(cores):
        return np.stack([core_grad_reference(cores, 0, X.astype(np.float64), np.eye(L)[:, k:k + 1].repeat(b, 1))[1] for k in range(L)])

    ref, mse = as64(start), []
    for _ in range(3):
        f = forward64(ref)
        mse.append(((y1h - f) ** 2).mean())
        G_o, _ = core_grad_reference(ref, 0, X.astype(np.float64), y1h - f)
        ref = [a + lr * g for a, g in zip(ref, G_o)]
    mse.append(((y1h - forward64(ref)) ** 2).mean())
    print('float64 mean squared error over three updates: ' + ' '.join('%.6f' % v for v in mse))
    assert mse[1] < mse[0] and mse[2] < mse[1] and mse[3] < mse[2], mse

    ctx = _hip.Context(N, D, L, M, b)
    dev = start
    for _ in range(3):
        ctx.set_cores(dev, 0)
        cot = (y1h - ctx.predict(X).astype(np.float64)).astype(np.float32)
        G, _ = ctx.core_grad(X, cot)
        dev = [(a + np.float32(lr) * g).astype(np.float32) for a, g in zip(dev, G)]
    ctx.close()
    worst = rel_cores(dev, ref)
    print('three plain updates: cores %.2e of max|A|' % worst)
    assert worst <= UPDATE_TOL


# ---------------------------------------------------------------------------------------------------------------
# 6. nothing else moved
# ---------------------------------------------------------------------------------------------------------------
SWEEP = (1e-2, 1e-3, True, 'softmax', 'full_cross_ent', 0.1, 'fixed')


def test_resident_state_is_untouched():
    N, D, L, M, b = 12, 2, 2, 6, 100
    rng = np.random.default_rng(65)
    X, y = features(rng, b, N, D), rng.integers(0, L, b)
    other = features(rng, 300, N, D)
    cot = rng.standard_normal((L, 300)).astype(np.float32)
    cores = cores_for(N, D, L, M, 0, rng, False)
    outs = []
    for with_call in (False, True):
        ctx = _hip.Context(N, D, L, M, b)
        ctx.set_cores(cores, 0)
        ctx.set_input(X, y)
        ctx.forward()
        if with_call:
            ctx.dataset_attach(other[:50], rng.integers(0, L, 50), 'features')
            ig_before = ctx.input_grad(other, cot)
            before = (ctx.get_f(), [ctx.get_env(_hip.SIDE_RIGHT, i) for i in range(1, N)], ctx.get_cores(), ctx.l_pos)
            ctx.core_grad(other)
            ctx.core_grad(other, cot)
            ctx.core_grad_indices(np.arange(50))
            after = (ctx.get_f(), [ctx.get_env(_hip.SIDE_RIGHT, i) for i in range(1, N)], ctx.get_cores(), ctx.l_pos)
            assert np.array_equal(before[0], after[0]) and before[3] == after[3]
            assert all(np.array_equal(a, c) for a, c in zip(before[1], after[1]))
            assert same_cores(before[2][0], after[2][0]) and np.array_equal(before[2][1], after[2][1])
            ig_after = ctx.input_grad(other, cot)
            assert np.array_equal(ig_before[0], ig_after[0]) and np.array_equal(ig_before[1], ig_after[1])
        met, f = ctx.sweep(False, N - 1, True, *SWEEP)
        outs.append((met, f, ctx.get_cores()[0]))
        ctx.close()
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
    assert same_cores(outs[0][2], outs[1][2])


def test_inner_label_without_any_position():
    N, D, L, M, l = 9, 2, 3, 5, 4
    rng = np.random.default_rng(66)
    ctx = _hip.Context(N, D, L, M, 64)
    cores = cores_for(N, D, L, M, l, rng, True)
    ctx.set_cores(cores, l)
    X = features(rng, 40, N, D)
    assert _code(lambda: ctx.predict(X)) == STATE
    G, cf = ctx.core_grad(X)
    assert _code(lambda: ctx.predict(X)) == STATE
    # the same numbers as with the switch on, where predict gives the class
    ctx.set_any_position(True)
    f = ctx.predict(X)
    G2, cf2 = ctx.core_grad(X)
    assert same_cores(G, G2) and np.array_equal(cf, cf2) and rel(cf, f.max(axis=0)) <= TOL
    onehot = np.zeros((L, 40))
    onehot[np.argmax(f, axis=0), np.arange(40)] = 1.0
    G_o, _ = core_grad_reference(as64(cores), l, X.astype(np.float64), onehot)
    assert rel_cores(G, G_o) <= TOL
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------
# 7. refusals
# ---------------------------------------------------------------------------------------------------------------
def test_refusals(monkeypatch):
    N, D, L, M = 6, 2, 3, 4
    rng = np.random.default_rng(68)
    ctx = _hip.Context(N, D, L, M, 64)
    X = features(rng, 10, N, D)
    lib, f32p, i32p = _hip.lib(), C.POINTER(C.c_float), C.POINTER(C.c_int32)
    flat = np.empty(N * D * M * M * L, dtype=np.float32)
    Xp, Gp = X.ctypes.data_as(f32p), flat.ctypes.data_as(f32p)
    assert lib.tnml_core_grad(ctx._h, Xp, 10, None, Gp, flat.size, None) == STATE                # cores never set
    cores = cores_for(N, D, L, M, 2, rng, False)
    ctx.set_cores(cores, 2)
    total = sum(c.size for c in cores)
    assert lib.tnml_core_grad(ctx._h, None, 10, None, Gp, flat.size, None) == ARG
    assert lib.tnml_core_grad(ctx._h, Xp, 10, None, None, flat.size, None) == ARG
    assert lib.tnml_core_grad(ctx._h, Xp, 0, None, Gp, flat.size, None) == ARG
    assert lib.tnml_core_grad(ctx._h, Xp, 10, None, Gp, total - 1, None) == ARG                  # capacity below tnml_cores_size
    assert _code(lambda: ctx.core_grad(X[:0])) == ARG
    assert _code(lambda: ctx.core_grad_indices([0, 1])) == STATE                                 # no dataset
    ctx.dataset_attach(X, rng.integers(0, L, 10), 'features')
    assert _code(lambda: ctx.core_grad_indices([0, 10])) == ARG and _code(lambda: ctx.core_grad_indices([-1])) == ARG
    idx = np.array([0, 1], dtype=np.int32)
    assert lib.tnml_core_grad_indices(ctx._h, None, 2, None, Gp, flat.size, None) == ARG
    assert lib.tnml_core_grad_indices(ctx._h, idx.ctypes.data_as(i32p), 2, None, None, flat.size, None) == ARG
    assert lib.tnml_core_grad_indices(ctx._h, idx.ctypes.data_as(i32p), 0, None, Gp, flat.size, None) == ARG
    assert lib.tnml_core_grad_indices(ctx._h, idx.ctypes.data_as(i32p), 2, None, Gp, total - 1, None) == ARG
    assert _code(lambda: ctx.set_core_grad_chunk(-1)) == ARG
    # usable afterwards
    G1, cf1 = ctx.core_grad_indices([0, 1, 9])
    G2, cf2 = ctx.core_grad(X[[0, 1, 9]])
    assert same_cores(G1, G2) and np.array_equal(cf1, cf2)
    ctx.close()
    # LDS: the message names the bytes
    ctx = _hip.Context(4, 2, 2, 100, 64)
    ctx.set_cores(cores_for(4, 2, 2, 100, 0, rng, False), 0)
    with pytest.raises(_hip.TnmlError, match='bytes of LDS') as ei:
        ctx.core_grad(features(rng, 4, 4, 2))
    assert ei.value.code == ARG
    ctx.close()
    # a communicator attached: the rule of the dataset block
    from tensornetworkforml_amd import dist as tdist
    monkeypatch.setenv('TNML_FORCE_COMM', '1')
    ctx = _hip.Context(N, D, L, M, 64)
    ctx.set_cores(cores_for(N, D, L, M, 0, rng, False), 0)
    tdist.attach_comm(ctx, 0, 1)
    assert _code(lambda: ctx.core_grad(X)) == STATE and _code(lambda: ctx.core_grad_indices([0])) == STATE
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------
# 8. reuse of one context, and the Network methods
# ---------------------------------------------------------------------------------------------------------------
def test_reuse_larger_smaller_other_cores():
    N, D, L, M = 17, 2, 3, 8
    rng = np.random.default_rng(69)
    ctx = _hip.Context(N, D, L, M, 64)
    worst = 0.0
    for b, l, ragged in ((300, 3, True), (17, 3, True), (130, 16, False), (5, 0, True), (300, 9, True)):
        cores = cores_for(N, D, L, M, l, rng, ragged)
        ctx.set_cores(cores, l)
        X = features(rng, b, N, D)
        cot = rng.standard_normal((L, b)).astype(np.float32)
        G, cf = ctx.core_grad(X, cot)
        G_o, cf_o = core_grad_reference(as64(cores), l, X.astype(np.float64), cot.astype(np.float64))
        worst = max(worst, rel_cores(G, G_o), rel(cf, cf_o))
    ctx.close()
    print('reuse: worst %.2e' % worst)
    assert worst <= TOL


def test_network_methods():
    import tensornetworkforml_amd as pkg
    N, D, L, M, b = 16, 2, 3, 4, 30
    np.random.seed(3)
    rng = np.random.default_rng(70)
    pix = pixels(rng, 50, N)
    X = gen.psi(pix.astype(np.float64), D)
    net = pkg.Network(N=N, M=M, D=D, L=L, normalize=True, calibration_X=X[:16], act_fn='linear', loss_fn='MSE', trunc='fixed')
    f = net.predict(X[:b])
    cores = as64(net._ctx.get_cores()[0])                      # the calibrated cores as the device holds them
    G, cf = net.core_gradient(X[:b], return_cf=True)
    assert [g.shape for g in G] == [c.shape for c in cores] and rel(cf, np.asarray(f.elem).max(axis=0)) <= TOL
    # the recipe of the README: the gradient of the loss
    y = np.zeros((L, b))
    y[rng.integers(0, L, b), np.arange(b)] = 1.0
    cot = net.compute_loss_derivate(net.apply_act_func(f), y)
    G_l = net.core_gradient(X[:b], cot)
    X32 = X[:b].astype(np.float32).astype(np.float64)
    G_o, _ = core_grad_reference(cores, net.l_pos, X32, np.asarray(cot.elem).astype(np.float32).astype(np.float64))
    assert rel_cores(G_l, G_o) <= TOL
    cls = rng.integers(0, L, b)
    onehot = np.zeros((L, b))
    onehot[cls, np.arange(b)] = 1.0
    assert same_cores(net.core_gradient(X[:b], cls), net.core_gradient(X[:b], onehot.astype(np.float32)))
    # a user edit of As reaches the device first, as in predict
    As = net.As
    As[3].elem *= 2.0
    G2 = net.core_gradient(X[:b], cls)
    G_c, _ = core_grad_reference(cores, net.l_pos, X32, onehot)
    G_c = [g * (1.0 if i == 3 else 2.0) for i, g in enumerate(G_c)]        # linear in every other core
    assert rel_cores(G2, G_c) <= 2 * TOL
    net.attach_dataset(X.astype(np.float32), rng.integers(0, L, 50))
    Gd = net.core_gradient_indices(np.arange(b), cls)
    assert same_cores(Gd, G2)
