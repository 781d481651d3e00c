"""Range-safe chains on the GPU (include/tnml.h, tnml_set_chain_scaling / tnml_predict_scaled), through
`_hip.Context` and `Network`.

  1  calibrated networks, switch on   predict, predict_scaled (recombined with np.ldexp in float64), input_grad and core_grad against
                                      the float64 references: N in {2, 3, 17}, the label sites of labels_of, uniform and ragged
                                      bonds, b in {1, 17, 70}, for the (D, cap, L) rows below.  The bounds are the existing tests'
                                      own (imported): ROW_TOL of tests/test_input_grad_gpu.py, ROW_TOL_G / ROW_TOL_CF of
                                      tests/test_core_grad_gpu.py, TOL = 2e-5 of max|f| for the predictions.  Prints whether the
                                      gradient results are bit-equal to the same calls with the switch off (not asserted: the
                                      compiler may contract the two instantiations differently).
  2  balanced decalibration           tests/scaled_chain_reference.py: N = 17, label sites 0, 5, 8, 16, b = 70.  Switch on: predict,
                                      input_grad and core_grad (per core, relative to that core's own max|G_i|) within the same
                                      bounds of the float64 reference on the decalibrated cores.  Switch off: predict is non-finite
                                      or off by more than 1e-2 of max|f| in at least one sample at every one of these sites.
  3  f out of range                   all 17 cores times 2^-12 (f times 2^-204) and times 2^+12: 0.5 <= max_l |mant| < 1 for every
                                      sample, np.ldexp(mant, expo) within TOL of the float64 reference per sample, relative to that
                                      sample's max_l |f|; at 2^+204 the plain output of predict is inf.
  4  chunking                         chunk 64 against the default at b = 70 with the switch on: g, cf and every G_i bit-equal
  5  one SGD step                     gd_step with the switch on over the balanced pattern, linear / MSE, no clip: accuracy equal,
                                      MAE within TOL, per core |after - ref_after| <= SGD_TOL[row] max|ref change of that core| +
                                      2^-23 max|A_i| (one float32 ulp of the stored core, which the 2^+-20 sizes make visible)
  6  state and refusals               the switch and the scaled calls leave f, the environments, the cores and l_pos of a resident
                                      batch alone; a sweep afterwards matches one without them; a bad `on`, NULL outputs of
                                      predict_scaled, an inner label with any_position off; the Network attribute and method

Worst observed on an MI355X (every test prints its own):
    1  (D, cap, L)     predict    predict_scaled  g          cf (input)  G          cf (core)   gradients bit-equal to switch off
       (2, 5, 3)       3.32e-07   3.32e-07        2.46e-07   4.10e-07    3.73e-07   6.87e-07    yes
       (2, 33, 2)      2.91e-07   2.91e-07        5.82e-07   5.87e-07    1.03e-06   2.19e-06    yes
       (2, 50, 10)     2.98e-07   2.98e-07        4.65e-07   5.00e-07    7.12e-07   1.89e-05    yes
       (3, 7, 3)       2.79e-07   2.79e-07        3.00e-07   2.32e-07    5.59e-07   4.26e-07    yes
       (8, 16, 17)     4.83e-07   4.83e-07        1.23e-06   2.78e-07    7.18e-07   3.59e-07    yes
    2  (2, 5, 3)       predict 1.40e-07, g 2.06e-07, cf 1.39e-07, G (per core) 1.24e-06; switch off: 70 of 70 samples broken at every site
       (3, 7, 3)       predict 2.03e-07, g 2.10e-07, cf 2.37e-07, G (per core) 1.49e-06; switch off: 70 of 70 samples broken at every site
    3  2^-204: 3.40e-07 (2, 5, 3), 3.32e-07 (3, 7, 3);  2^+204: 3.40e-07, 3.32e-07
    5  accuracy equal (22 and 27 of 70), MAE differs by 1.2e-08 and 2.2e-09, cores 0.39 of the bound at worst
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import gradient_step_reference as R                                                          # noqa: E402
from core_grad_reference import core_grad_reference                                          # noqa: E402
from input_grad_reference import input_grad_reference                                        # noqa: E402
from scaled_chain_reference import BALANCED_N, balanced_pattern, decalibrate                 # noqa: E402
from test_any_position_host import label_inside_forward                                      # noqa: E402
from test_core_grad_gpu import ROW_TOL_CF, ROW_TOL_G                                         # noqa: E402
from test_gradient_step_gpu import SGD_TOL, context_M                                        # noqa: E402
from test_input_grad_gpu import ROW_TOL, cores_for, features, labels_of                      # noqa: E402
from test_scaled_chain_host import BALANCED_LABELS, BALANCED_ROWS, balanced_case             # noqa: E402
from tensornetworkforml_amd import _hip                                                      # noqa: E402

pytestmark = pytest.mark.gpu

ARG, STATE = -1, -2
TOL = 2e-5
ROWS = [(2, 5, 3), (2, 33, 2), (2, 50, 10), (3, 7, 3), (8, 16, 17)]


def _code(call):
    with pytest.raises(_hip.TnmlError) as ei:
        call()
    return ei.value.code


def as64(cores):
    return [c.astype(np.float64) for c in cores]


def rel(a, ref, scale=None):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    assert a.shape == ref.shape, (a.shape, ref.shape)
    return np.abs(a - ref).max() / max(np.abs(ref).max() if scale is None else scale, 1e-300)


def rel_cores(G, G_ref):
    """the worst element of any core, relative to max|G_ref| over all cores (tests/test_core_grad_gpu.py)"""
    scale = max(np.abs(g).max() for g in G_ref)
    return max(rel(g, r, scale) for g, r in zip(G, G_ref))


def recombine(mant, expo):
    return np.ldexp(mant.astype(np.float64), expo.astype(np.int64)[None, :])


def same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def check_normalised(mant, expo):
    """0.5 <= max_l |mant| < 1 per sample (every f of these tests is finite and not all zero)"""
    mx = np.abs(mant).max(axis=0)
    assert mant.dtype == np.float32 and expo.dtype == np.int32 and expo.shape == (mant.shape[1],)
    assert (mx >= 0.5).all() and (mx < 1.0).all(), (mx.min(), mx.max())


# ---------------------------------------------------------------------------------------------------------------
# 1. calibrated networks with the switch on
# ---------------------------------------------------------------------------------------------------------------
# The bounds of the two existing tests are ten times what those tests observed on their own draws, and cf at b = 1 is a sum over the
# labels with cancellation (up to 7000-fold, head of tests/test_core_grad_gpu.py): another draw of the cotangent can pass a bound with
# no difference in the code (a first version of this test drew its own cases and saw cf 5.4e-06 against 4e-06 at (8, 16, 17), with the
# switch on and, bit for bit, with it off).  So each gradient call is checked on the cases its bound was taken on: the generator of
# tests/test_input_grad_gpu.py (seed 100 D + cap + L) for input_grad, that of tests/test_core_grad_gpu.py (200 D + cap + L) for
# core_grad, drawn in those tests' order (features per N; cores per label site and bond pattern; the cotangent per b).  The two
# predictions are checked on both.
@pytest.mark.parametrize('row', ROWS, ids=lambda r: 'D%d-cap%d-L%d' % r)
def test_calibrated_networks_with_the_switch_on(row):
    D, cap, L = row
    worst = dict(f=0.0, fs=0.0, g=0.0, cf_in=0.0, G=0.0, cf_core=0.0)
    bit_equal = True
    for which, seed in (('input', 100 * D + cap + L), ('core', 200 * D + cap + L)):
        rng = np.random.default_rng(seed)
        for N in (2, 3, 17):
            ctx = _hip.Context(N, D, L, context_M(row), 70)
            ctx.set_any_position(True)
            Xall = features(rng, 70, N, D)
            for l in labels_of(N):
                for ragged in (False, True):
                    cores = cores_for(N, D, L, cap, l, rng, ragged)
                    ctx.set_cores(cores, l)
                    c64 = as64(cores)
                    for b in (1, 17, 70):
                        X = Xall[:b]
                        X64 = X.astype(np.float64)
                        cot = rng.standard_normal((L, b)).astype(np.float32)
                        call = ctx.input_grad if which == 'input' else ctx.core_grad
                        ctx.set_chain_scaling(False)
                        off = call(X, cot)
                        ctx.set_chain_scaling(True)
                        f = ctx.predict(X)
                        mant, expo = ctx.predict_scaled(X)
                        on = call(X, cot)
                        f_o = label_inside_forward(c64, l, X64)[2]
                        check_normalised(mant, expo)
                        assert same(f, recombine(mant, expo).astype(np.float32))          # fpred = ldexpf(mant, expo)
                        worst['f'] = max(worst['f'], rel(f, f_o))
                        worst['fs'] = max(worst['fs'], rel(recombine(mant, expo), f_o))
                        if which == 'input':
                            g_o, cf_o = input_grad_reference(c64, l, X64, cot.astype(np.float64))
                            worst['g'] = max(worst['g'], rel(on[0], g_o))
                            worst['cf_in'] = max(worst['cf_in'], rel(on[1], cf_o))
                            bit_equal &= same(on[0], off[0]) and same(on[1], off[1])
                        else:
                            G_o, cf_o = core_grad_reference(c64, l, X64, cot.astype(np.float64))
                            assert [g.shape for g in on[0]] == [c.shape for c in cores]
                            worst['G'] = max(worst['G'], rel_cores(on[0], G_o))
                            worst['cf_core'] = max(worst['cf_core'], rel(on[1], cf_o))
                            bit_equal &= same(on[1], off[1]) and all(same(a, c) for a, c in zip(on[0], off[0]))
            ctx.close()
    print('scaled chains D %d cap %d L %d: predict %.2e, predict_scaled %.2e of max|f|; g %.2e, cf %.2e; G %.2e, cf %.2e; '
          'gradients bit-equal to the switch off: %s' % (D, cap, L, worst['f'], worst['fs'], worst['g'], worst['cf_in'], worst['G'],
                                                         worst['cf_core'], 'yes' if bit_equal else 'no'))
    assert worst['f'] <= TOL and worst['fs'] <= TOL, worst
    assert worst['g'] <= ROW_TOL[row] and worst['cf_in'] <= ROW_TOL[row], worst
    assert worst['G'] <= ROW_TOL_G[row] and worst['cf_core'] <= ROW_TOL_CF[row], worst


# ---------------------------------------------------------------------------------------------------------------
# 2. balanced decalibration: f of order 1, partial products at 2^+-160
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('row', BALANCED_ROWS, ids=lambda r: 'D%d-cap%d-L%d' % r)
def test_balanced_decalibration(row):
    D, cap, L = row
    N, b = BALANCED_N, 70
    ctx = _hip.Context(N, D, L, context_M(row), b)
    ctx.set_any_position(True)
    worst = dict(f=0.0, g=0.0, cf_in=0.0, G=0.0, cf_core=0.0)
    broken_min = b
    for l in BALANCED_LABELS:
        _, dec, X = balanced_case(row, l, b)
        d64, X64 = as64(dec), X.astype(np.float64)
        cot = np.random.default_rng(l).standard_normal((L, b)).astype(np.float32)
        ctx.set_cores(dec, l)
        f_o = label_inside_forward(d64, l, X64)[2]
        g_o, cf_o = input_grad_reference(d64, l, X64, cot.astype(np.float64))
        G_o, cfG_o = core_grad_reference(d64, l, X64, cot.astype(np.float64))
        ctx.set_chain_scaling(True)
        f = ctx.predict(X)
        g, cfi = ctx.input_grad(X, cot)
        G, cfc = ctx.core_grad(X, cot)
        worst['f'] = max(worst['f'], rel(f, f_o))
        worst['g'] = max(worst['g'], rel(g, g_o))
        worst['cf_in'] = max(worst['cf_in'], rel(cfi, cf_o))
        worst['G'] = max(worst['G'], max(rel(a, r) for a, r in zip(G, G_o)))         # per core, relative to its own max|G_i|
        worst['cf_core'] = max(worst['cf_core'], rel(cfc, cfG_o))
        ctx.set_chain_scaling(False)
        with np.errstate(invalid='ignore'):
            f_plain = ctx.predict(X).astype(np.float64)
            broken = ~np.isfinite(f_plain).all(axis=0) | (np.abs(np.nan_to_num(f_plain) - f_o).max(axis=0) > 1e-2 * np.abs(f_o).max())
        broken_min = min(broken_min, int(broken.sum()))
        assert broken.any(), 'the plain chain survived the balanced pattern at label site %d' % l
    ctx.close()
    print('balanced decalibration D %d cap %d L %d: predict %.2e, g %.2e, cf %.2e, G (per core) %.2e, cf %.2e; switch off: at least %d of %d '
          'samples broken per label site' % (D, cap, L, worst['f'], worst['g'], worst['cf_in'], worst['G'], worst['cf_core'], broken_min, b))
    assert worst['f'] <= TOL, worst
    assert worst['g'] <= ROW_TOL[row] and worst['cf_in'] <= ROW_TOL[row], worst
    assert worst['G'] <= ROW_TOL_G[row] and worst['cf_core'] <= ROW_TOL_CF[row], worst


# ---------------------------------------------------------------------------------------------------------------
# 3. f itself outside float32
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('row', BALANCED_ROWS, ids=lambda r: 'D%d-cap%d-L%d' % r)
@pytest.mark.parametrize('k', [-12, 12])
def test_f_out_of_range(row, k):
    D, cap, L = row
    N, b = BALANCED_N, 70
    ctx = _hip.Context(N, D, L, context_M(row), b)
    ctx.set_any_position(True)
    worst = 0.0
    for on in (False, True):                                   # predict_scaled works whether or not the switch is on
        ctx.set_chain_scaling(on)
        for l in BALANCED_LABELS:
            cores, _, X = balanced_case(row, l, b)
            dec = decalibrate(cores, [k] * N)
            ctx.set_cores(dec, l)
            f_o = label_inside_forward(as64(dec), l, X.astype(np.float64))[2]
            assert np.isfinite(f_o).all() and abs(np.log2(np.abs(f_o).max()) - k * N) < 12
            mant, expo = ctx.predict_scaled(X)
            check_normalised(mant, expo)
            per_sample = np.abs(recombine(mant, expo) - f_o).max(axis=0) / np.abs(f_o).max(axis=0)
            worst = max(worst, per_sample.max())
            top = np.sort(f_o, axis=0)
            clear = (top[-1] - top[-2]) > 2 * TOL * np.abs(f_o).max(axis=0)
            assert np.array_equal(mant.argmax(axis=0)[clear], f_o.argmax(axis=0)[clear])                 # the argmax is readable
            if on:
                f = ctx.predict(X)
                with np.errstate(over='ignore', under='ignore'):
                    expect = recombine(mant, expo).astype(np.float32)                  # IEEE saturation / flush of ldexpf
                assert same(f, expect)
                assert np.isinf(f).any() if k > 0 else (f == 0).all()
    ctx.close()
    print('f times 2^%d, D %d cap %d L %d: predict_scaled %.2e of max_l|f| per sample' % (k * N, D, cap, L, worst))
    assert worst <= TOL


# ---------------------------------------------------------------------------------------------------------------
# 4. the results do not depend on the chunking
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('row', BALANCED_ROWS, ids=lambda r: 'D%d-cap%d-L%d' % r)
def test_chunking_with_the_switch_on(row):
    D, cap, L = row
    N, b = BALANCED_N, 70
    ctx = _hip.Context(N, D, L, context_M(row), 64)
    ctx.set_any_position(True)
    ctx.set_chain_scaling(True)
    for l in (0, 8):
        _, dec, X = balanced_case(row, l, b)
        ctx.set_cores(dec, l)
        for cot in (np.random.default_rng(l).standard_normal((L, b)).astype(np.float32), None):
            g0, cfi0 = ctx.input_grad(X, cot)
            G0, cfc0 = ctx.core_grad(X, cot)
            ctx.set_input_grad_chunk(64)
            ctx.set_core_grad_chunk(64)
            g1, cfi1 = ctx.input_grad(X, cot)
            G1, cfc1 = ctx.core_grad(X, cot)
            ctx.set_input_grad_chunk(0)
            ctx.set_core_grad_chunk(0)
            assert np.isfinite(g0).all() and all(np.isfinite(a).all() for a in G0)
            assert same(g0, g1) and same(cfi0, cfi1) and same(cfc0, cfc1) and all(same(a, c) for a, c in zip(G0, G1)), l
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------
# 5. one SGD step over the balanced pattern
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('l', [0, 8])
def test_one_sgd_step_over_the_balanced_pattern(l):
    row = (2, 5, 3)
    D, cap, L = row
    N, b, lr = BALANCED_N, 70, 0.05
    _, dec, X = balanced_case(row, l, b)
    y = np.random.default_rng(50 + l).integers(0, L, b).astype(np.int32)
    ref = R.GradientStepReference(as64(dec), l, clip=False)
    info = ref.step(X, y, lr, R.WD, 'linear', 'MSE', R.T_CASES)
    ctx = _hip.Context(N, D, L, context_M(row), b)
    ctx.optim_config('sgd', clip=False)
    ctx.set_chain_scaling(True)
    ctx.set_cores(dec, l)
    correct, abs_sum, nonfinite = ctx.gd_step(X, y, lr, R.WD, 'linear', 'MSE', R.T_CASES)
    after, _, lp = ctx.get_cores()
    ctx.close()
    mae, mae_ref = abs_sum / (b * L), info['abs_sum'] / (b * L)
    print('SGD step over the balanced pattern, label site %d: correct %d (reference %d), MAE %.6f (reference %.6f, difference %.1e)'
          % (l, correct, info['correct'], mae, mae_ref, abs(mae - mae_ref)))
    assert lp == l and nonfinite == 0 and correct == info['correct']
    assert abs(mae - mae_ref) <= TOL * max(np.abs(info['f']).max(), 1.0)
    worst = 0.0
    for i, (a, before, r) in enumerate(zip(after, dec, ref.cores)):
        b64 = before.astype(np.float64)
        bound = SGD_TOL[row] * np.abs(r - b64).max() + 2.0 ** -23 * max(np.abs(b64).max(), np.abs(r).max())
        err = np.abs(a.astype(np.float64) - r).max()
        worst = max(worst, err / bound)
        assert err <= bound, (i, err, bound)
    print('    cores: %.2f of the bound at worst' % worst)


# ---------------------------------------------------------------------------------------------------------------
# 6. state and refusals
# ---------------------------------------------------------------------------------------------------------------
SWEEP = (1e-2, 1e-3, True, 'softmax', 'full_cross_ent', 0.1, 'fixed')


def test_resident_state_is_untouched():
    N, D, L, M, b = 12, 2, 2, 6, 100
    rng = np.random.default_rng(5)
    X, y = features(rng, b, N, D), rng.integers(0, L, b)
    other = features(rng, 300, N, D)
    cores = cores_for(N, D, L, M, 0, rng, False)
    outs = []
    for with_calls in (False, True):
        ctx = _hip.Context(N, D, L, M, b)
        ctx.set_cores(cores, 0)
        ctx.set_input(X, y)
        ctx.forward()
        if with_calls:
            snap = lambda: (ctx.get_f(), [ctx.get_env(_hip.SIDE_RIGHT, i) for i in range(1, N)], ctx.get_cores(), ctx.l_pos)    # noqa: E731
            before = snap()
            ctx.set_chain_scaling(True)
            ctx.predict(other)
            ctx.predict_scaled(other)
            ctx.input_grad(other)
            ctx.core_grad(other, rng.standard_normal((L, 300)).astype(np.float32))
            ctx.set_chain_scaling(False)
            ctx.predict_scaled(other[:7])
            after = snap()
            assert np.array_equal(before[0], after[0]) and before[3] == after[3]
            assert all(np.array_equal(a, c) for a, c in zip(before[1], after[1]))
            assert all(np.array_equal(a, c) for a, c in zip(before[2][0], after[2][0])) and np.array_equal(before[2][1], after[2][1])
        met, f = ctx.sweep(False, N - 1, True, *SWEEP)
        outs.append((met, f, ctx.get_cores()[0]))
        ctx.close()
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
    assert all(np.array_equal(a, c) for a, c in zip(outs[0][2], outs[1][2]))


def test_refusals():
    N, D, L, M, l = 9, 2, 3, 5, 4
    rng = np.random.default_rng(6)
    ctx = _hip.Context(N, D, L, M, 64)
    X = features(rng, 10, N, D)
    assert _code(lambda: ctx.predict_scaled(X)) == STATE                                 # cores never set
    ctx.set_cores(cores_for(N, D, L, M, l, rng, True), l)
    for bad in (2, -1, 7):
        assert _code(lambda: ctx.set_chain_scaling(bad)) == ARG
    lib, f32p, i32p = _hip.lib(), C.POINTER(C.c_float), C.POINTER(C.c_int32)
    assert lib.tnml_set_chain_scaling(None, 1) == ARG
    mant, expo = np.empty((L, 10), dtype=np.float32), np.empty(10, dtype=np.int32)
    Xp, mp, ep = X.ctypes.data_as(f32p), mant.ctypes.data_as(f32p), expo.ctypes.data_as(i32p)
    assert lib.tnml_predict_scaled(ctx._h, Xp, 10, None, ep) == ARG
    assert lib.tnml_predict_scaled(ctx._h, Xp, 10, mp, None) == ARG
    assert lib.tnml_predict_scaled(ctx._h, None, 10, mp, ep) == ARG
    assert lib.tnml_predict_scaled(ctx._h, Xp, 0, mp, ep) == ARG
    # an inner label with any_position off: the rule of predict, with the switch off and on
    assert _code(lambda: ctx.predict_scaled(X)) == STATE
    ctx.set_chain_scaling(True)
    assert _code(lambda: ctx.predict_scaled(X)) == STATE and _code(lambda: ctx.predict(X)) == STATE
    g, cf = ctx.input_grad(X)                                                             # (the gradient calls never needed it)
    ctx.set_any_position(True)
    mant, expo = ctx.predict_scaled(X)
    check_normalised(mant, expo)
    assert rel(cf, recombine(mant, expo).max(axis=0)) <= TOL
    ctx.close()
    # LDS: the message names the bytes
    ctx = _hip.Context(4, 2, 2, 100, 64)
    ctx.set_cores(cores_for(4, 2, 2, 100, 0, rng, False), 0)
    with pytest.raises(_hip.TnmlError, match='bytes of LDS') as ei:
        ctx.predict_scaled(features(rng, 4, 4, 2))
    assert ei.value.code == ARG
    ctx.close()


def test_network_attribute_and_method():
    import tensornetworkforml_amd as pkg
    from tensornetworkforml_amd import data_generator as gen
    N, D, L, M, b = BALANCED_N, 2, 3, 4, 40
    np.random.seed(4)
    rng = np.random.default_rng(12)
    X = gen.psi((rng.random((b, N)) * (rng.random((b, N)) > 0.3)).astype(np.float64), D)
    net = pkg.Network(N=N, M=M, D=D, L=L, normalize=True, calibration_X=X[:16], act_fn='linear', loss_fn='MSE', trunc='fixed')
    assert net.scaled_chains is False
    # the balanced pattern as a user edit of As: f stays what it was, the suffix products drop to 2^-160
    As = net.As
    for i, k in enumerate(balanced_pattern()):
        As[i].elem *= 2.0 ** int(k)
    mant, expo = net.predict_scaled(X)                          # with the attribute off
    cores = as64(net._ctx.get_cores()[0])                      # the decalibrated cores as the device holds them
    f_o = R.forward64(cores, net.l_pos, X.astype(np.float32).astype(np.float64))
    check_normalised(mant, expo)
    assert 0.01 < np.abs(f_o).max() < 100 and rel(recombine(mant, expo), f_o) <= TOL

    def plain_is_broken():
        with np.errstate(invalid='ignore'):
            f = np.asarray(net.predict(X).elem)
            return not np.isfinite(f).all() or rel(np.nan_to_num(f), f_o) > 1e-2

    assert plain_is_broken()
    net.scaled_chains = True
    assert rel(net.predict(X).elem, f_o) <= TOL
    g, cf = net.input_gradient(X, return_cf=True)
    assert np.isfinite(np.asarray(g)).all() and rel(cf, f_o.max(axis=0)) <= TOL
    net.scaled_chains = False
    assert plain_is_broken()
