"""tnml_nll_masked_grad / tnml_nll_masked_step on the device against the NumPy statement of tests/nll_masked_reference.py (DESIGN.md
section 31).  Every comparison is with the reference, never with the device's own output, except where bit-equality between two
device calls is the claim, and in the two tests that hold the new call against the device's own nll_gradient and log_prob_masked.
The bounds are derived, none of them comes from the device (nll_masked_reference.Case.bounds, per site):

    |G - G_ref64| <= 2^-22 max|G_i| + N m^2 D^2 2^-52 max|Gz_i| + 10 d_LD
    value, logp within N m^2 D^2 2^-52 max(1, |v|) + 10 d_LD

the one float32 rounding, section 24's float64 accumulation form, and section 24's margin of ten on the reference's own
float64-against-long-double difference d_LD.  Every test prints its figures before it asserts."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p_ in (ROOT, HERE):
    if p_ not in sys.path:
        sys.path.insert(0, p_)

import mps_algebra_reference as A                                  # noqa: E402
import nll_masked_reference as M                                   # noqa: E402
import nll_reference as N                                          # noqa: E402
import nll_step_reference as SR                                    # noqa: E402
import test_sample_gpu as G                                        # noqa: E402  (its helpers: new_ctx, network_of, bits, _code)
from tensornetworkforml_amd import _hip                            # noqa: E402

pytestmark = pytest.mark.gpu

ARG, STATE, SHAPE, NONFINITE = -1, -2, -6, -7
BAD_BATCH, NOT_APPLIED = 8, 16
SWEEP = (1e-2, 1e-3, True, 'softmax', 'full_cross_ent', 0.1, 'fixed')


def ctx_of(c, cores=None):
    ctx = G.new_ctx(c.N, c.D, c.L, c.mb)
    ctx.set_cores(A.as32(c.cores if cores is None else cores), c.l)
    return ctx


def device(ctx, c, want=('G', 'logp')):
    return ctx.nll_masked_grad(c.n, c.phi, c.w, c.mask, c.known, c.classes, want=want)


def step(ctx, c, lr, wd=0.0, renorm=True):
    return ctx.nll_masked_step(c.n, c.phi, c.w, c.mask, c.known, c.classes, lr, wd, renorm)


def site_errors(Gd, Gref):
    return np.array([float(np.abs(g.astype(np.float64) - r).max()) for g, r in zip(Gd, Gref)])


def same(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def configure(ctx, name):
    o = SR.OPTIMS[name]
    ctx.optim_config(o['kind'], momentum=o['momentum'], eps=o.get('eps', 1e-8), clip=o['clip'])


def dev_cores(ctx):
    return [x.astype(np.float64) for x in ctx.get_cores()[0]]


def tile_bytes(ctx, c):
    """what one tile of the call needs under tnml_set_sample_stack_bytes, from the refusal's own message"""
    ctx.set_sample_stack_bytes(8)
    assert G._code(lambda: device(ctx, c)) == ARG
    return int(re.search(r'needs (\d+) bytes', _hip.lib().tnml_last_error().decode()).group(1))


# ---------------------------------------------------------------------------------------------------------------
# 1. the gradient, the value and logp against the reference
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', M.GRAD_CASES)
def test_gradient_against_reference(name):
    """dense N = 4 (all 16 masks, classes -1 / 0 / 1, the label on 0, 2, 3); ragged N = 17 at the three rows with the label at both
    ends and inside, n = 1 / 17 / 70; bond 20 (two 16-row chunks, the second ragged); bonds 50 and 64 (T = 2 and 1)"""
    c = M.case(name)
    ref = c.ref
    gb, vb, lb = c.bounds()
    ctx = ctx_of(c)
    Gd, logp, out = device(ctx, c)
    ctx.close()
    err = site_errors(Gd, ref['G'])
    ev, el = abs(out[0] - float(ref['value'])), float(np.abs(logp - ref['logp']).max())
    sums = np.abs(M.site_sums(Gd, c.cores) - M.site_sums(ref['G'], c.cores))
    sb = gb * np.array([float(np.abs(x).sum()) for x in c.cores])
    print('%s n %d bonds %s: G worst err/bound %.3f (err %.2e, max|G| %.2e)  value %.2e (%.1e)  logp %.2e (%.1e)  sum(G A) worst/bound %.3f'
          % (name, c.n, c.bond, (err / gb).max(), err.max(), M.gmax(ref['G']), ev, vb, el, lb, (sums / sb).max()))
    assert out[2] == 0 and out[3] == 0
    assert abs(out[1] - float(ref['logz'])) <= vb
    assert ev <= vb and el <= lb
    assert (err <= gb).all(), (name, np.argmax(err / gb), (err / gb).max())
    assert (sums <= sb).all()


# ---------------------------------------------------------------------------------------------------------------
# 2. the full mask against the device's own nll_gradient; empty masks; logp against log_prob_masked
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,objective', [('full_mask', 'joint'), ('full_mask_marginal', 'marginal')])
def test_full_mask_against_nll_gradient(name, objective):
    c = M.case(name)
    row = (c.D, c.mb, c.L)
    ctx = ctx_of(c)
    Gm, _, out = device(ctx, c)
    X = c.phi[c.known].astype(np.float32)
    Gn, out3 = ctx.nll_grad(X, c.classes if objective == 'joint' else None, N.gram(c.phi, c.w))
    ctx.close()
    value_n = out3[0] - float(np.log(c.w)[c.known].sum(axis=1).mean())
    gbound, vbound = N.gpu_bounds(row, objective)
    dev = N.deviation([g.astype(np.float64) for g in Gm], [g.astype(np.float64) for g in Gn])
    dv = abs(out[0] - value_n) / max(1.0, abs(value_n))
    print('%s: masked against nll_gradient %.2e (%.0e)  value %.2e (%.0e)' % (name, dev, gbound, dv, vbound))
    assert dev <= gbound and dv <= vbound


def test_empty_masks_give_nothing():
    c = M.case('empty')
    gb, _, _ = c.bounds()
    ctx = ctx_of(c)
    Gd, logp, out = device(ctx, c)
    ctx.close()
    err = site_errors(Gd, [np.zeros_like(x) for x in c.cores])
    print('empty masks: value %r  max|G| / bound %.3f' % (out[0], (err / gb).max()))
    assert out[0] == 0.0 and (logp == 0.0).all()
    assert (err <= gb).all()


@pytest.mark.parametrize('name', ['ragged_D2_L2_M5_l8', 'ragged_D8_L10_M16_l16'])
def test_logp_against_log_prob_masked(name):
    c = M.case(name)
    _, _, lb = c.bounds()
    ctx = ctx_of(c)
    _, logp, _ = device(ctx, c, want=('logp',))
    ctx.close()
    net = G.network_of(c.cores, c.l, G.context_M(c.D, c.mb, c.L), c.D, c.L)
    lab, unl = np.where(c.classes >= 0)[0], np.where(c.classes < 0)[0]
    other = np.zeros(c.n)
    if len(lab):
        other[lab] = net.log_prob_masked(c.known[lab], c.mask[lab], classes=c.classes[lab], levels=c.K, weights=c.w, joint=True)
    if len(unl):
        other[unl] = net.log_prob_masked(c.known[unl], c.mask[unl], levels=c.K, weights=c.w)
    d = float(np.abs(logp - other).max())
    print('%s: logp against log_prob_masked %.2e (%.1e)' % (name, d, lb))
    assert d <= lb


# ---------------------------------------------------------------------------------------------------------------
# 3. determinism: a repeated call, a stack budget of one tile
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['ragged_D3_L3_M7_l8', 'bond20_N5'])
def test_budget_and_repeat_are_bit_equal(name):
    c = M.case(name)
    ctx = ctx_of(c)
    G1, l1, o1 = device(ctx, c)
    G2, l2, o2 = device(ctx, c)
    need = tile_bytes(ctx, c)
    ctx.set_sample_stack_bytes(need - 1)
    assert G._code(lambda: device(ctx, c)) == ARG
    ctx.set_sample_stack_bytes(need)
    G3, l3, o3 = device(ctx, c)
    ctx.set_sample_stack_bytes(2 * need + 7)
    G4, l4, o4 = device(ctx, c)
    ctx.close()
    print('%s: one tile needs %d bytes' % (name, need))
    for Gx, lx, ox in ((G2, l2, o2), (G3, l3, o3), (G4, l4, o4)):
        assert same(G1, Gx) and l1.tobytes() == lx.tobytes() and o1.tobytes() == ox.tobytes()


# ---------------------------------------------------------------------------------------------------------------
# 4. the step
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', M.STEP_CASES)
def test_one_step_against_the_reference(name):
    """one step per optimiser against nll_step_reference's update applied to the reference G; lr = 0 leaves the cores bit-equal"""
    c = M.case(name)
    _, vb, _ = c.bounds()
    ctx = ctx_of(c)
    for opt in M.STEP_OPTIMS:
        lr, want = M.step_lr(c, opt), M.step_reference(c, opt)
        bound = M.step_bound(c, opt)
        ctx.set_cores(A.as32(c.cores), c.l)
        configure(ctx, opt)
        v = step(ctx, c, lr, M.WD)
        err = site_errors(dev_cores(ctx), want)
        print('%s %s: lr %.3g  step worst err/bound %.3f (err %.2e)  value %.2e (%.1e)' % (name, opt, lr, (err / bound).max(), err.max(),
                                                                                         abs(v[0] - float(c.ref['value'])), vb))
        assert v[2] == 0 and v[3] == 0
        assert abs(v[0] - float(c.ref['value'])) <= vb
        assert (err <= bound).all(), (opt, (err / bound).max())
        ctx.set_cores(A.as32(c.cores), c.l)
        configure(ctx, opt)
        before = G.bits(ctx)
        step(ctx, c, 0.0)
        assert G.bits(ctx) == before
    ctx.close()


def test_a_sample_of_zero_weight_changes_nothing():
    c = M.case('descent')
    cores = [x.copy() for x in c.cores]
    cores[c.l][..., 1] = 0.0                                       # class 1 has zero weight
    cls = c.classes.copy()
    cls[:] = 0
    cls[3] = 1
    ctx = ctx_of(c, cores)
    configure(ctx, 'sgd_clip_mom')
    ctx.nll_masked_step(c.n, c.phi, c.w, c.mask, c.known, np.zeros(c.n, dtype=np.int32), 1e-2)      # (the state exists)
    before = G.bits(ctx)
    with pytest.raises(_hip.TnmlError) as ei:
        ctx.nll_masked_step(c.n, c.phi, c.w, c.mask, c.known, cls, 1e-2)
    v = ei.value.values
    print('zero weight: code %d values %s' % (ei.value.code, v))
    assert ei.value.code == NONFINITE and v[2] == 1 and int(v[3]) & NOT_APPLIED and int(v[3]) & BAD_BATCH
    assert G.bits(ctx) == before
    with pytest.raises(_hip.TnmlError) as ei:
        ctx.nll_masked_grad(c.n, c.phi, c.w, c.mask, c.known, cls)
    assert ei.value.code == NONFINITE and ei.value.values[2] == 1
    # the state is untouched too: the next good step equals that of a context that never saw the bad batch
    twin = ctx_of(c, cores)
    configure(twin, 'sgd_clip_mom')
    good = np.zeros(c.n, dtype=np.int32)
    twin.nll_masked_step(c.n, c.phi, c.w, c.mask, c.known, good, 1e-2)
    twin.nll_masked_step(c.n, c.phi, c.w, c.mask, c.known, good, 1e-2)
    ctx.nll_masked_step(c.n, c.phi, c.w, c.mask, c.known, good, 1e-2)
    assert G.bits(ctx) == G.bits(twin)
    ctx.close()
    twin.close()


def test_ten_steps_lower_the_value():
    c = M.case('descent')
    ctx = ctx_of(c)
    configure(ctx, 'sgd')
    vals = [step(ctx, c, M.DESCENT_LR)[0] for _ in range(10)]
    vals.append(device(ctx, c, want=())[2][0])
    ctx.close()
    print('ten steps: %s' % ' '.join('%.4f' % v for v in vals))
    assert vals[-1] < vals[0]
    assert abs(vals[0] - float(c.ref['value'])) <= c.bounds()[1]


# ---------------------------------------------------------------------------------------------------------------
# 5. the state of the context
# ---------------------------------------------------------------------------------------------------------------
def _resident(c, b=40):
    rng = np.random.default_rng(5)
    X = c.phi[rng.integers(0, c.K, (b, c.N))].astype(np.float32)
    return X, rng.integers(0, c.L, b).astype(np.int32)


def test_a_gradient_call_changes_nothing():
    """get_cores, bonds, l_pos, the resident batch's forward and a following sweep are bit-equal to a context that never made the call"""
    c = M.case('descent_l0')
    X, y = _resident(c)
    out = []
    for call in (False, True):
        ctx = _hip.Context(c.N, c.D, c.L, 4, 64)
        ctx.set_cores(A.as32(c.cores), c.l)
        ctx.set_input(X, y)
        f0 = ctx.forward()
        if call:
            device(ctx, c)
            device(ctx, c, want=())
        bond, lp = ctx.bonds()
        state = (G.bits(ctx), bond.tobytes(), lp, ctx.forward().tobytes())
        met, f = ctx.sweep(False, c.N - 1, True, *SWEEP)
        out.append((f0.tobytes(), state, met.tobytes(), f.tobytes(), G.bits(ctx)))
        ctx.close()
    assert out[0] == out[1]


def test_context_state_after_a_step():
    """a sweep is refused after a step until a forward, as after gd_step; the resident batch stays"""
    c = M.case('descent_l0')
    X, y = _resident(c)
    ctx = _hip.Context(c.N, c.D, c.L, 4, 64)
    ctx.set_cores(A.as32(c.cores), c.l)
    ctx.set_input(X, y)
    ctx.forward()
    configure(ctx, 'sgd_clip_mom')
    step(ctx, c, 1e-2)
    assert G._code(lambda: ctx.sweep(False, c.N - 1, True, *SWEEP)) == STATE
    f = ctx.forward()
    assert np.array_equal(f, ctx.predict(X))
    ctx.sweep(False, c.N - 1, True, *SWEEP)
    ctx.forward(want_f=False)
    assert G._code(lambda: step(ctx, c, 1e-2)) == STATE             # the state belongs to the label position before the sweep
    ctx.optim_reset()
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------
# 6. refusals, and the Network level
# ---------------------------------------------------------------------------------------------------------------
def test_refusals():
    c = M.case('descent')
    lib, f32p, i32p, f64p, u8p = _hip.lib(), C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_uint8)
    phi, w = np.ascontiguousarray(c.phi), np.ascontiguousarray(c.w)
    mask, known, cls = np.ascontiguousarray(c.mask, dtype=np.uint8), np.ascontiguousarray(c.known), np.ascontiguousarray(c.classes)
    flat, out, logp = np.zeros(4096, dtype=np.float32), np.zeros(4), np.zeros(c.n)
    pp, wp, mp, kp, cp = phi.ctypes.data_as(f64p), w.ctypes.data_as(f64p), mask.ctypes.data_as(u8p), known.ctypes.data_as(i32p), cls.ctypes.data_as(i32p)
    fp, op, lp = flat.ctypes.data_as(f32p), out.ctypes.data_as(f64p), logp.ctypes.data_as(f64p)
    ctx = G.new_ctx(c.N, c.D, c.L, c.mb)
    grad = lambda *a: lib.tnml_nll_masked_grad(*a)
    assert grad(ctx._h, c.n, c.K, pp, wp, cp, mp, c.n, kp, fp, flat.size, lp, op) == STATE          # cores never set
    ctx.set_cores(A.as32(c.cores), c.l)
    before = G.bits(ctx)
    assert grad(None, c.n, c.K, pp, wp, cp, mp, c.n, kp, fp, flat.size, lp, op) == ARG
    assert grad(ctx._h, c.n, c.K, pp, wp, cp, mp, c.n, kp, fp, flat.size, lp, None) == ARG
    assert grad(ctx._h, 0, c.K, pp, wp, cp, mp, c.n, kp, fp, flat.size, lp, op) == ARG
    assert grad(ctx._h, c.n, 1, pp, wp, cp, mp, c.n, kp, fp, flat.size, lp, op) == ARG
    assert grad(ctx._h, c.n, 257, pp, wp, cp, mp, c.n, kp, fp, flat.size, lp, op) == ARG
    assert grad(ctx._h, c.n, c.K, None, wp, cp, mp, c.n, kp, fp, flat.size, lp, op) == ARG
    assert grad(ctx._h, c.n, c.K, pp, None, cp, mp, c.n, kp, fp, flat.size, lp, op) == ARG
    assert grad(ctx._h, c.n, c.K, pp, wp, cp, mp, 2, kp, fp, flat.size, lp, op) == ARG               # mask_rows
    assert grad(ctx._h, c.n, c.K, pp, wp, cp, None, c.n, kp, fp, flat.size, lp, op) == ARG
    assert grad(ctx._h, c.n, c.K, pp, wp, cp, mp, c.n, None, fp, flat.size, lp, op) == ARG           # NULL known, bits set
    assert grad(ctx._h, c.n, c.K, pp, wp, cp, mp, c.n, kp, fp, 10, lp, op) == ARG                    # capacity
    bad = cls.copy()
    bad[2] = c.L
    assert grad(ctx._h, c.n, c.K, pp, wp, bad.ctypes.data_as(i32p), mp, c.n, kp, fp, flat.size, lp, op) == ARG
    bk = known.copy()
    bk[np.where(c.mask)[0][0], np.where(c.mask)[1][0]] = c.K
    assert grad(ctx._h, c.n, c.K, pp, wp, cp, mp, c.n, bk.ctypes.data_as(i32p), fp, flat.size, lp, op) == ARG
    bw = w.copy()
    bw[1] = 0.0
    assert grad(ctx._h, c.n, c.K, pp, bw.ctypes.data_as(f64p), cp, mp, c.n, kp, fp, flat.size, lp, op) == ARG
    assert lib.tnml_nll_masked_step(ctx._h, c.n, c.K, pp, wp, cp, mp, c.n, kp, 0.1, 0.0, 2, op) == ARG       # renorm
    assert lib.tnml_nll_masked_step(ctx._h, c.n, c.K, pp, wp, cp, mp, c.n, kp, 0.1, 0.0, 1, None) == ARG
    assert G.bits(ctx) == before
    # value alone: a NULL gradient needs no capacity; every output but out4 may be NULL
    assert grad(ctx._h, c.n, c.K, pp, wp, cp, mp, c.n, kp, None, 0, None, op) == 0
    assert abs(out[0] - float(c.ref['value'])) <= c.bounds()[1]
    ctx.close()
    # the bond limit: 64 is taken (the cases above), 65 is refused with the bytes in the message
    rng = np.random.default_rng(3)
    big = [rng.standard_normal(s) * 0.1 for s in N.shapes_of(4, 2, 2, [2, 65, 2], 0)]
    ctx = G.new_ctx(4, 2, 2, 65)
    ctx.set_cores(A.as32(big), 0)
    _, phi7, w7 = M.SR.grid(7, 2)
    assert G._code(lambda: ctx.nll_masked_grad(2, phi7, w7, np.zeros(4, dtype=bool), None)) == SHAPE
    assert 'bytes of LDS' in lib.tnml_last_error().decode()
    ctx.close()


def test_network_level():
    """Network.nll_gradient_masked / nll_masked / nll_step_masked: the context's calls on the grid of `levels` and `weights`"""
    c = M.case('descent')
    net = G.network_of(c.cores, c.l, 4, c.D, c.L)
    Gn, v = net.nll_gradient_masked(c.known, c.mask, y=c.classes, levels=c.K, weights=c.w)
    ctx = ctx_of(c)
    Gc, _, out = device(ctx, c)
    assert same(Gn, Gc) and v == out[0]
    assert net.nll_masked(c.known, c.mask, y=c.classes, levels=c.K, weights=c.w) == v
    x = np.arange(c.K) / (c.K - 1)
    assert net.nll_masked(x[c.known], c.mask, y=c.classes, levels=c.K, weights=c.w) == v             # pixel values on the grid
    v_all = net.nll_masked(c.known, None, y=int(0), levels=c.K, weights=c.w)                      # None: every pixel known; an int
    assert v_all == ctx.nll_masked_grad(c.n, c.phi, c.w, np.ones(c.N, dtype=bool), c.known, np.zeros(c.n, dtype=np.int32), want=())[2][0]
    net.configure_optimizer('sgd', clip=False)
    v0, logz = net.nll_step_masked(c.known, c.mask, y=c.classes, lr=M.DESCENT_LR, levels=c.K, weights=c.w)
    configure(ctx, 'sgd')
    o = step(ctx, c, M.DESCENT_LR)
    assert (v0, logz) == (o[0], o[1])
    assert same(net._ctx.get_cores()[0], ctx.get_cores()[0])
    assert net.nll_masked(c.known, c.mask, y=c.classes, levels=c.K, weights=c.w) < v0
    ctx.close()


def test_script_option(tmp_path, capsys):
    """training_diagonals.py --objective nll --missing F --unlabelled F2: masked steps in a host loop, accuracy under occlusion"""
    from tensornetworkforml_amd import training_diagonals
    np.random.seed(11)
    val_acc, hist = training_diagonals.main(['--resident', '--objective', 'nll', '--missing', '0.3', '--unlabelled', '0.25', '--n_samples', '400',
                                             '--linear_dim', '4', '--M', '4', '--n_epochs', '2', '--n_train_batch', '4', '--lr', '0.01',
                                             '--L2_decay', '0', '--out', str(tmp_path / 'model.dat')])
    out = capsys.readouterr().out
    assert 'Epoch 1/2 - masked NLL' in out and 'masked NLL per epoch' in out and 'validation accuracy of classify_masked' in out
    assert len(val_acc) == 2 and hist.shape == (2, 4) and np.isfinite(hist).all() and (tmp_path / 'model.dat').exists()
