"""tnml_inner / tnml_axpby on the device against the float64 reference of tests/mps_algebra_reference.py.
Every comparison is with the reference, never with the device's own output; every bound is ten times the worst value observed on an
MI355X in its class, rounded up to one digit (the table is in DESIGN.md section 21 and repeated at the bounds below).  Distance and cosine are
compared only on pairs whose reference relative distance is >= 1e-3 (tests/test_mps_algebra_host.py asserts that on the reference).
"""
import ctypes as C
import math
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
import orthogonalize_reference as R                                # noqa: E402
from gradient_step_reference import forward64                      # noqa: E402
from tensornetworkforml_amd import _hip                            # noqa: E402

pytestmark = pytest.mark.gpu

ARG, STATE, SHAPE, NONFINITE = -1, -2, -6, -7
# Observed on an MI355X (worst over the cases of each class) -> bound = 10 x the worst value, rounded up to one digit:
#   |dlog| of any output on the short chains (N = 2, 3, 17 at three metrics: 1.15e-13, 3.42e-14, 7.46e-14 per row; bonds 64 and
#     33: 3.55e-15; log|aW + bV|^2: 7.11e-15)                                                    1.15e-13 -> 2e-12
#   |dlog| at N = 784 (pair 5.68e-13; raw chain and chain scaled by 1e15 per core, log<W|W> = 54307: 5.82e-11)   5.82e-11 -> 6e-10
#   cosine, relative distance and distance^2, all pairs (short 7.82e-14, bonds 64 and 33 2.00e-15, N = 784 4.87e-13,
#     compression certificate 1.78e-14)                                                        4.87e-13 -> 5e-12
#   0.5 log<W|W> against tnml_bond_spectra's log|W| at N = 784                                 1.65e-12 -> 2e-11
#   tnml_predict after tnml_axpby / compress / combine against a f_W + b f_V, of max|f| (6.87e-07, 1.30e-06, 1.11e-06 per row;
#     W + W compressed back 2.55e-07, combine 1.36e-07 and 4.36e-07)                           1.30e-06 -> 2e-05
LOG_TOL_SHORT = 2e-12
LOG_TOL_LONG = 6e-10
COS_TOL = 5e-12
SPECTRA_TOL = 2e-11
F_TOL = 2e-05
SWEEP = (1e-2, 1e-3, True, 'softmax', 'full_cross_ent', 0.1, 'fixed')
HYPER = (0.05, 0.0, 'softmax', 'full_cross_ent', 0.1)


def _code(call):
    with pytest.raises(_hip.TnmlError) as ei:
        call()
    return ei.value.code


def context_M(D, cap, L):
    """the smallest M whose bond capacity max(M, D min(L, M)) holds `cap`"""
    return next(M for M in range(1, cap + 1) if max(M, D * min(L, M)) >= cap)


def new_ctx(N, D, L, cap, b=A.B):
    ctx = _hip.Context(N, D, L, context_M(D, cap, L), b)
    ctx.set_any_position(True)
    return ctx


def log_err(dev, ref):
    """worst |dlog| of the pairs of two (3, 2) results; the signs must agree"""
    dev, ref = np.asarray(dev), np.asarray(ref)
    assert np.array_equal(dev[:, 0], ref[:, 0]), (dev, ref)
    return float(np.abs(dev[:, 1] - ref[:, 1]).max())


def cos_dist_err(dev, ref):
    d_dev, d_ref = math.sqrt(max(0.0, A.distance2(dev))), math.sqrt(max(0.0, A.distance2(ref)))
    assert d_ref >= A.MIN_DISTANCE
    return max(abs(A.cosine(dev) - A.cosine(ref)), abs(d_dev - d_ref))


def bits(ctx):
    cores, bond, lp = ctx.get_cores()
    slots, lab = ctx.core_slots()
    return [c.tobytes() for c in cores], bond.tobytes(), lp, slots.tobytes(), lab.tobytes()


def network_of(cores, l, M, D, L):
    import tensornetworkforml_amd as pkg
    net = pkg.Network_class.Network(len(cores), M, D=D, L=L, trunc='fixed')
    net._host_cores = A.as64(cores)
    net._l_pos = l
    net._host_newer = True
    return net


# ---------------------------------------------------------------------------------------------------------------
# 1. the six outputs against the reference: N = 2, 3, 17 ragged at every label position, three metrics; tile edges
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('row', A.ROWS, ids=lambda r: 'D%d_L%d' % r)
def test_inner_products_small_chains(row):
    D, L = row
    worst_log, worst_cos, n = 0.0, 0.0, 0
    for N in (2, 3, 17):
        ctx = new_ctx(N, D, L, A.MW)
        for l in range(N):
            W, V, X, metrics = A.build_small((N, D, L, l))
            ctx.set_cores(A.as32(W), l)
            for name, S in metrics:
                ref = A.inner3(W, V, l, S)
                dev = ctx.inner(A.as32(V), l, S)
                worst_log = max(worst_log, log_err(dev, ref))
                worst_cos = max(worst_cos, cos_dist_err(dev, ref))
                n += 1
            alone = ctx.inner()
            assert np.array_equal(alone[0], ctx.inner(A.as32(V), l)[0]) and alone[1:].tolist() == [[0.0, -math.inf]] * 2
        ctx.close()
    print('D %d L %d: %d calls, |dlog| %.2e, cosine / distance %.2e' % (D, L, n, worst_log, worst_cos))
    assert n == 22 * 3
    assert worst_log <= LOG_TOL_SHORT and worst_cos <= COS_TOL


def test_inner_products_bonds_64_and_33():
    (N, D, L, l), W, V, X, metrics = A.tile_pair()
    ctx = new_ctx(N, D, L, 64)
    ctx.set_cores(A.as32(W), l)
    worst_log, worst_cos = 0.0, 0.0
    for name, S in metrics:
        ref, dev = A.inner3(W, V, l, S), ctx.inner(A.as32(V), l, S)
        worst_log, worst_cos = max(worst_log, log_err(dev, ref)), max(worst_cos, cos_dist_err(dev, ref))
    ctx.close()
    print('bonds 64 and 33: |dlog| %.2e, cosine / distance %.2e' % (worst_log, worst_cos))
    assert worst_log <= LOG_TOL_SHORT and worst_cos <= COS_TOL


# ---------------------------------------------------------------------------------------------------------------
# 2. N = 784: the exponent bookkeeping, the cross-check with tnml_bond_spectra, chains outside every float range
# ---------------------------------------------------------------------------------------------------------------
def test_long_chains_and_the_norm_of_bond_spectra():
    (N, D, L, l), W, V = A.long_pair()
    ctx = new_ctx(N, D, L, 20, 8)
    ctx.set_cores(A.as32(W), l)
    ref, dev = A.inner3(W, V, l), ctx.inner(A.as32(V), l)
    e_pair, e_cos = log_err(dev, ref), cos_dist_err(dev, ref)
    logn = ctx.bond_spectra()[2]
    e_spec = abs(0.5 * dev[0, 1] - logn)
    print('N = 784 pair: |dlog| %.2e, cosine / distance %.2e (distance %.3e); 0.5 log<W|W> - log|W| of bond_spectra %.2e'
          % (e_pair, e_cos, math.sqrt(A.distance2(ref)), e_spec))
    # an un-calibrated network (f about 1e-66) and the same cores times 1e15 each: finite logs, equal to the reference's
    _, raw = A.raw_long_chain()
    big = A.as64(A.as32([c * 1e15 for c in raw]))
    e_raw = 0.0
    for cores in (raw, big):
        ctx.set_cores(A.as32(cores), l)
        dev = ctx.inner(A.as32(W), l)
        assert np.isfinite(dev[:, 1]).all()
        e_raw = max(e_raw, log_err(dev, A.inner3(cores, W, l)))
    print('N = 784 raw chain and chain scaled by 1e15 per core: |dlog| %.2e (log<W|W> %.1f and %.1f)' % (e_raw, A.inner(raw, raw, l)[1], A.inner(big, big, l)[1]))
    # a NaN anywhere is reported
    before = bits(ctx)
    for site in (5, N - 3):
        bad = A.as32(W)
        bad[site][0, 1, 0] = np.nan
        assert _code(lambda: ctx.inner(bad, l)) == NONFINITE
    bad = A.as32(W)
    bad[l][0, 0, 0, 1] = np.inf
    assert _code(lambda: ctx.inner(bad, l)) == NONFINITE
    assert bits(ctx) == before
    ctx.close()
    assert e_pair <= LOG_TOL_LONG and e_raw <= LOG_TOL_LONG and e_cos <= COS_TOL and e_spec <= SPECTRA_TOL


# ---------------------------------------------------------------------------------------------------------------
# 3. bit-equality; tnml_inner leaves the context bit for bit
# ---------------------------------------------------------------------------------------------------------------
def test_equal_chains_give_cosine_one_and_the_context_stays_bit_for_bit():
    N, D, L, l = 17, 2, 2, 0
    W, V, X, metrics = A.build_small((N, D, L, l))
    y = (np.arange(A.B) % L).astype(np.int32)
    ctx = new_ctx(N, D, L, A.MW)
    ctx.set_cores(A.as32(W), l)
    ctx.set_input(X, y)
    f = ctx.forward()
    envs = [ctx.get_env(_hip.SIDE_RIGHT, i).tobytes() for i in range(1, N)]
    before = bits(ctx)
    for name, S in metrics:
        t = ctx.inner(A.as32(W), l, S)
        assert t[0].tobytes() == t[1].tobytes() == t[2].tobytes(), (name, t)
        assert np.array_equal(t, ctx.inner(A.as32(W), l, S))                                       # two calls are bit-equal
        u = ctx.inner(A.as32(V), l, S)
        assert np.array_equal(u, ctx.inner(A.as32(V), l, S))
    assert bits(ctx) == before and ctx.get_f().tobytes() == f.tobytes()
    assert [ctx.get_env(_hip.SIDE_RIGHT, i).tobytes() for i in range(1, N)] == envs
    ctx.sweep(False, 2, True, *SWEEP)                                                              # no new forward needed
    ctx.close()
    a, b, c = network_of(W, l, 12, D, L), network_of(W, l, 12, D, L), network_of(V, l, 12, D, L)
    for metric in (None, 'uniform', metrics[2][1]):
        assert a.cosine(b, metric) == 1.0 and a.distance(b, metric) == 0.0 and a.distance(b, metric, relative=False) == 0.0
    ref = A.inner3(W, V, l, A.psi_gram(D))
    assert abs(a.cosine(c, 'uniform') - A.cosine(ref)) <= COS_TOL
    assert abs(a.distance(c, 'uniform') - math.sqrt(A.distance2(ref))) <= COS_TOL
    assert abs(a.distance(c, relative=False) / math.exp(0.5 * A.inner(W, W, l)[1]) - math.sqrt(A.distance2(A.inner3(W, V, l)))) <= COS_TOL
    alone = a.inner()
    assert alone[0][0] == 1.0 and abs(alone[0][1] - A.inner(W, W, l)[1]) <= LOG_TOL_SHORT and alone[1] == alone[2] == (0.0, -math.inf)
    c.l_pos = 3
    with pytest.raises(ValueError, match='label'):
        a.inner(c)


# ---------------------------------------------------------------------------------------------------------------
# 4. tnml_axpby: slots bit for bit, predictions, the norm of the sum, compress, combine
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('row', A.ROWS, ids=lambda r: 'D%d_L%d' % r)
def test_linear_combination_small_chains(row):
    D, L = row
    worst_f, worst_sum, n = 0.0, 0.0, 0
    for N in (2, 3, 17):
        ctx = new_ctx(N, D, L, A.MW + A.MV)
        cap = ctx.bond_capacity
        for l in range(N):
            W, V, X, _ = A.build_small((N, D, L, l))
            X64 = X.astype(np.float64)
            fw, fv = forward64(W, l, X64), forward64(V, l, X64)
            t = [s * math.exp(lg) for s, lg in A.inner3(W, V, l)]
            for a, b in ((1.0, 1.0), (1.0, -1.0), (0.5, 0.5), (-1.0, 0.5)):
                ctx.set_cores(A.as32(W), l)
                bond = ctx.axpby(a, b, A.as32(V), l)
                want = A.direct_sum(W, V, l, a, b, np.float32)
                assert [int(v) for v in bond] == R.bonds_of(want) and ctx.l_pos == l
                slots, lab = ctx.core_slots()
                ws, wl = A.slots_of(want, l, cap, D, L)
                assert slots.tobytes() == ws.tobytes() and lab.tobytes() == wl.tobytes(), (N, l, a, b)
                f_ref = a * fw + b * fv
                worst_f = max(worst_f, float(np.abs(ctx.predict(X) - f_ref).max() / max(abs(a) * np.abs(fw).max(), abs(b) * np.abs(fv).max())))
                s, lg = ctx.inner()[0]
                ref2 = a * a * t[0] + b * b * t[1] + 2 * a * b * t[2]
                assert s == 1.0 and ref2 > 0
                worst_sum = max(worst_sum, abs(lg - math.log(ref2)))
                n += 1
        ctx.close()
    print('D %d L %d: %d sums bit for bit, predict %.2e of max|f|, log|aW + bV|^2 %.2e' % (D, L, n, worst_f, worst_sum))
    assert n == 22 * 4
    assert worst_f <= F_TOL and worst_sum <= LOG_TOL_SHORT


def test_sum_at_the_tile_edges_and_compress_back():
    (N, D, L, l), W, V, X, _ = A.tile_pair()
    ctx = new_ctx(N, D, L, 97)
    ctx.set_cores(A.as32(W), l)
    ctx.axpby(0.5, 0.5, A.as32(V), l)
    slots, lab = ctx.core_slots()
    ws, wl = A.slots_of(A.direct_sum(W, V, l, 0.5, 0.5, np.float32), l, ctx.bond_capacity, D, L)
    assert slots.tobytes() == ws.tobytes() and lab.tobytes() == wl.tobytes()
    ctx.close()
    # W + W compressed to the original bond is 2 W; combine of two copies of one network returns that network's function
    N, D, L, l = 17, 3, 3, 8
    W, V, X, _ = A.build_small((N, D, L, l))
    X64 = X.astype(np.float64)
    fw = forward64(W, l, X64)
    ctx = new_ctx(N, D, L, 2 * A.MW)
    ctx.set_cores(A.as32(W), l)
    ctx.axpby(1.0, 1.0, A.as32(W), l)
    bond, _, disc, _ = ctx.compress(A.MW)
    assert all(int(x) <= y for x, y in zip(bond, R.bonds_of(W)))
    e_comp = float(np.abs(ctx.predict(X) - 2 * fw).max() / np.abs(2 * fw).max())
    ctx.close()
    import tensornetworkforml_amd as pkg
    a, b = network_of(W, l, A.MW, D, L), network_of(W, l, A.MW, D, L)
    net = pkg.Network_class.combine([a, b], max_bond=A.MW)
    assert net.M == A.MW and net.l_pos == l
    net.any_position = True
    e_comb = float(np.abs(net.predict(X).elem - fw).max() / np.abs(fw).max())
    mixed = pkg.Network_class.combine([a, network_of(V, l, A.MV, D, L)], coeffs=[0.25, -2.0], max_bond=A.MW + A.MV)
    mixed.any_position = True
    f_ref = 0.25 * fw - 2.0 * forward64(V, l, X64)
    e_mix = float(np.abs(mixed.predict(X).elem - f_ref).max() / np.abs(f_ref).max())
    print('W + W compressed back: predict %.2e; combine of two copies %.2e; combine 0.25 W - 2 V %.2e of max|f|' % (e_comp, e_comb, e_mix))
    assert max(e_comp, e_comb, e_mix) <= F_TOL
    # Network.add in place, and the ValueError that names the M needed
    big = network_of(W, l, A.MW + A.MV, D, L)
    assert big.add(network_of(V, l, A.MV, D, L), 0.25, -2.0) == [x + y for x, y in zip(R.bonds_of(W), R.bonds_of(V))]
    big.any_position = True
    assert float(np.abs(big.predict(X).elem - f_ref).max() / np.abs(f_ref).max()) <= F_TOL
    with pytest.raises(ValueError, match='M >= %d' % (2 * A.MW)):                                 # capacity max(5, 3 * 3) = 9
        a.add(b)


# ---------------------------------------------------------------------------------------------------------------
# 5. the compression certificate
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', A.CERT_CASES, ids=lambda c: c[0])
def test_compression_certificate(case):
    name, (D, cap, L), N, l, m_max, thr = case
    W, X, Wc_ref, d2_ref, disc_ref = A.certificate_reference(case)
    ctx = new_ctx(N, D, L, cap, R.B)
    ctx.set_cores(A.as32(W), l)
    _, _, disc, _ = ctx.compress(m_max, thr)
    d2 = A.distance2(ctx.inner(A.as32(W), l)[[1, 0, 2]])                                           # relative to |W|: W is the second chain here
    ctx.close()
    print('%s: relative distance^2 %.6e (reference %.6e, |d| %.2e), discarded %.6e' % (name, d2, d2_ref, abs(d2 - d2_ref), disc.sum()))
    assert abs(d2 - d2_ref) <= COS_TOL
    assert d2 <= 2.0 * disc.sum()


# ---------------------------------------------------------------------------------------------------------------
# 6. refusals; the state after a committed tnml_axpby
# ---------------------------------------------------------------------------------------------------------------
def test_refusals_leave_everything_as_it_was(monkeypatch):
    N, D, L, l = 17, 2, 2, 3
    W, V, X, _ = A.build_small((N, D, L, l))
    lib = _hip.lib()
    f32p, i32p, f64p = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_double)
    ctx = new_ctx(N, D, L, A.MW + 3)                                                               # W + W (bond 10) does not fit
    flat = np.concatenate([c.ravel() for c in A.as32(V)])
    vb = np.array(R.bonds_of(V), dtype=np.int32)
    out, bo, S = np.zeros(6), np.zeros(N - 1, dtype=np.int32), np.zeros((N, D, D))
    fp, bp, op, bop, sp = flat.ctypes.data_as(f32p), vb.ctypes.data_as(i32p), out.ctypes.data_as(f64p), bo.ctypes.data_as(i32p), S.ctypes.data_as(f64p)
    assert lib.tnml_inner(ctx._h, None, 0, None, 0, None, 0, op) == STATE                          # cores never set
    ctx.set_cores(A.as32(W), l)
    before = bits(ctx)
    zb = vb.copy()
    zb[4] = 0
    zbp = zb.ctypes.data_as(i32p)
    n = 0
    for rc in (lib.tnml_inner(None, fp, flat.size, bp, l, None, 0, op), lib.tnml_inner(ctx._h, fp, flat.size, bp, l, None, 0, None),
               lib.tnml_inner(ctx._h, fp, flat.size - 1, bp, l, None, 0, op), lib.tnml_inner(ctx._h, fp, flat.size, None, l, None, 0, op),
               lib.tnml_inner(ctx._h, fp, flat.size, zbp, l, None, 0, op), lib.tnml_inner(ctx._h, fp, flat.size, bp, l + 1, None, 0, op),
               lib.tnml_inner(ctx._h, fp, flat.size, bp, l, sp, 0, op), lib.tnml_inner(ctx._h, fp, flat.size, bp, l, sp, 2, op),
               lib.tnml_axpby(None, 1.0, 1.0, fp, flat.size, bp, l, bop), lib.tnml_axpby(ctx._h, 1.0, 1.0, fp, flat.size, bp, l, None),
               lib.tnml_axpby(ctx._h, 1.0, 1.0, None, 0, None, l, bop), lib.tnml_axpby(ctx._h, float('nan'), 1.0, fp, flat.size, bp, l, bop),
               lib.tnml_axpby(ctx._h, 1.0, float('inf'), fp, flat.size, bp, l, bop), lib.tnml_axpby(ctx._h, 1.0, 1.0, fp, flat.size + 2, bp, l, bop),
               lib.tnml_axpby(ctx._h, 1.0, 1.0, fp, flat.size, zbp, l, bop), lib.tnml_axpby(ctx._h, 1.0, 1.0, fp, flat.size, bp, l - 1, bop)):
        assert rc == ARG
        n += 1
    assert n == 16
    with pytest.raises(_hip.TnmlError, match=r'beyond the capacity %d' % ctx.bond_capacity) as ei:
        ctx.axpby(1.0, 1.0, A.as32(W), l)
    assert ei.value.code == ARG and bits(ctx) == before
    # a result beyond float32 is reported and nothing is committed
    thin = [np.full(shp, 0.5, dtype=np.float32) for shp in R.shapes_of(N, D, L, [1] * (N - 1), l)]
    assert _code(lambda: ctx.axpby(1.0, 1e39, thin, l)) == NONFINITE
    assert bits(ctx) == before
    ctx.axpby(1.0, 1.0, thin, l)                                                                   # usable afterwards
    ctx.close()
    # bonds beyond the chain kernel's LDS: refused with the bytes in the message
    ctx = _hip.Context(4, 2, 2, 128, 64)
    rng = np.random.default_rng(3)
    Xs = R.features(rng, 8, 4, 2)
    big, small = R.make_cores(4, 2, 2, [2, 128, 2], 0, rng, Xs), R.make_cores(4, 2, 2, [2, 3, 2], 0, rng, Xs)
    ctx.set_cores(A.as32(small), 0)
    before = bits(ctx)
    with pytest.raises(_hip.TnmlError, match='bytes of LDS') as ei:
        ctx.inner(A.as32(big), 0)
    assert ei.value.code == SHAPE and bits(ctx) == before
    ctx.close()
    # a communicator attached
    from tensornetworkforml_amd import dist as tdist
    monkeypatch.setenv('TNML_FORCE_COMM', '1')
    W, V, X, _ = A.build_small((N, D, L, 0))                                                       # (a communicator wants the label on a chain end)
    ctx = _hip.Context(N, D, L, A.MW + A.MV, A.B)
    ctx.set_cores(A.as32(W), 0)
    tdist.attach_comm(ctx, 0, 1)
    before = bits(ctx)
    assert _code(lambda: ctx.inner(A.as32(V), 0)) == STATE and _code(lambda: ctx.axpby(1.0, 1.0, A.as32(V), 0)) == STATE
    assert bits(ctx) == before
    ctx.close()


def test_context_state_after_a_sum():
    N, D, L, l = 17, 2, 2, 0
    W, V, X, _ = A.build_small((N, D, L, l))
    y = (np.arange(A.B) % L).astype(np.int32)
    ctx = new_ctx(N, D, L, A.MW + A.MV)
    for opt in (dict(kind='sgd', momentum=0.9), dict(kind='adam', eps=1e-3, clip=False)):
        ctx.set_cores(A.as32(W), l)
        ctx.optim_config(**opt)
        ctx.gd_step(X, y, *HYPER)
        ctx.inner(A.as32(V), l)
        ctx.gd_step(X, y, *HYPER)                                                                  # tnml_inner leaves the state bound
        ctx.set_input(X, y)
        ctx.forward()
        ctx.axpby(1.0, 1.0, A.as32(V), l)
        assert _code(lambda: ctx.sweep(False, N - 1, True, *SWEEP)) == STATE                       # the resident f is stale
        with pytest.raises(_hip.TnmlError, match='tnml_optim_reset') as ei:
            ctx.gd_step(X, y, *HYPER)
        assert ei.value.code == STATE
        ctx.optim_reset()
        ctx.gd_step(X, y, *HYPER)
        f = ctx.forward()                                                                          # the resident batch stayed
        assert np.array_equal(f, ctx.predict(X))
        ctx.sweep(False, 2, True, *SWEEP)
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------
# 7. the scripts
# ---------------------------------------------------------------------------------------------------------------
def test_scripts_print_distance_and_compare(tmp_path, monkeypatch, capsys):
    import pickle
    from tensornetworkforml_amd import evaluate_diagonals as eval_script
    from tensornetworkforml_amd import training_diagonals as train_script
    monkeypatch.chdir(tmp_path)
    out = str(tmp_path / 'diag.dat')
    np.random.seed(4)
    train_script.main(['--n_samples', '400', '--linear_dim', '4', '--M', '4', '--n_epochs', '1', '--trunc', 'fixed', '--resident', '--compress', '2',
                       '--out', out])
    line = [ln for ln in capsys.readouterr().out.splitlines() if 'relative distance |W - W_c| / |W|' in ln]
    assert len(line) == 1
    d = float(line[0].rsplit(':', 1)[1])
    assert 0.0 <= d < 1.0 and math.isfinite(d)
    np.random.seed(5)
    eval_script.main(['--filename', out, '--n_samples', '200', '--compare', out])
    line = [ln for ln in capsys.readouterr().out.splitlines() if 'cosine' in ln]
    assert len(line) == 1 and 'cosine 1.000000000, relative distance |W - V| / |W| 0' in line[0], line
    with open(out, 'rb') as fh:
        net = pickle.load(fh)
    assert max(int(c.shape[2]) for c in net._host_cores[:-1]) <= 2
