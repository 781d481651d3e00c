"""tnml_orthogonalize / tnml_compress / tnml_bond_spectra on the device against the float64 reference of
tests/orthogonalize_reference.py, through gauge-free quantities: f after the call (tnml_predict), the
normalised spectra, the log-norm, the discarded weights, bonds and ranks (equal), and the isometry defect of the returned float32
cores divided by g next to the defect of the reference's cores rounded to float32.

The cases are those of the reference module; tests/test_orthogonalize_host.py checks, with the reference alone, that no singular
value of any decomposed matrix comes near rank_tol, that every cut falls into a gap and that every compression moves f visibly.

Bounds: ten times the worst value observed on an MI355X, rounded up to one digit (WORST below; every test prints what it
observed).  Two conditions hold whatever was measured: the isometry defect may not exceed ten times the defect of the rounded
reference in the same case, and the f error after tnml_orthogonalize may not exceed ten times what the reference's
float32-rounded orthogonal cores give through the float64 chain.
    (D, bond, L)    |dlog|     spectra    f, tnml_predict   (before the call)   f, float64 chain   rounded reference   defect     rounded ref.   f bound
    (2, 5, 3)       1.15e-14   2.72e-15   4.32e-07          3.05e-07            2.34e-07           2.34e-07            9.41e-08   9.41e-08       5e-06
    (2, 33, 2)      1.23e-13   5.91e-15   1.92e-06          1.09e-06            2.08e-07           2.08e-07            8.31e-08   8.31e-08       2e-05
    (2, 64, 2)      2.67e-13   3.96e-15   2.89e-06          2.31e-06            1.55e-07           1.55e-07            9.14e-08   9.14e-08       3e-05
    (2, 50, 10)     1.95e-13   2.68e-14   2.86e-06          2.05e-06            1.87e-07           1.87e-07            9.33e-08   9.33e-08       3e-05
    (3, 7, 3)       1.33e-14   1.39e-15   3.31e-07          4.57e-07            1.42e-07           1.42e-07            8.67e-08   8.67e-08       4e-06
    (8, 16, 17)     5.68e-14   1.67e-15   1.51e-06          1.57e-06            1.28e-07           1.28e-07            7.37e-08   7.37e-08       2e-05
    compression     |dlog|     spectra    discarded  f, tnml_predict   f, float64 chain   rounded reference   defect     rounded ref.
    half_l0         4.00e-15   7.20e-16   1.00e-16   1.40e-07          5.52e-08           5.52e-08            7.34e-08   7.34e-08
    half_l8         2.10e-14   1.80e-15   3.80e-17   6.51e-07          1.26e-07           1.26e-07            8.29e-08   8.29e-08
    half_l16        4.40e-14   2.40e-15   1.10e-16   2.32e-07          1.19e-07           1.19e-07            7.25e-08   7.25e-08
    half_L10        4.10e-14   1.10e-15   7.80e-18   1.59e-06          1.22e-07           1.22e-07            7.35e-08   7.35e-08
    half_D3         3.60e-15   7.80e-16   8.70e-18   1.99e-07          2.19e-07           2.19e-07            6.10e-08   6.10e-08
    half_D8         7.10e-15   1.40e-15   5.90e-17   1.59e-06          3.29e-07           3.29e-07            3.47e-08   3.47e-08
    adaptive        2.50e-14   1.90e-15   4.00e-16   3.45e-07          6.66e-08           6.66e-08            7.40e-08   7.40e-08
    adaptive_capped 2.30e-14   1.70e-15   1.90e-16   3.67e-07          1.96e-07           1.96e-07            7.38e-08   7.38e-08
    three_sites     3.10e-15   3.90e-16   2.10e-16   1.45e-07          4.07e-08           4.07e-08            3.29e-08   3.29e-08
    two_sites       4.00e-15   6.70e-16   3.90e-16   2.44e-07          3.25e-08           3.25e-08            3.10e-08   3.10e-08
    N = 200, bond 4: g 1.466, |dlog| 0.0e+00, f 5.00e-06 through tnml_predict (1.47e-06 before the call), 1.65e-06 through the float64 chain (rounded
    reference 1.65e-06), defect 7.91e-08 (rounded reference 7.91e-08).
    bond 96, N = 14: |dlog| 3.3e-13, f 7.96e-07 through tnml_predict, 1.02e-07 through the float64 chain (rounded reference 1.02e-07),
    defect 6.70e-08 (rounded reference 6.70e-08).
Bounds: |dlog| 3e-12, spectra 3e-13, discarded 4e-15, f per row as listed (the compression cases of a row included), N = 200: 5e-05.
"""
import ctypes as C
import os
import pickle
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p_ in (ROOT, HERE):
    if p_ not in sys.path:
        sys.path.insert(0, p_)

import orthogonalize_reference as R                                # noqa: E402
from gradient_step_reference import forward64                      # noqa: E402
from tensornetworkforml_amd import _hip                            # noqa: E402
from tensornetworkforml_amd import data_generator as gen           # noqa: E402

pytestmark = pytest.mark.gpu

ARG, STATE, SHAPE, NONFINITE = -1, -2, -6, -7
# ten times the observed value, rounded up to one digit (see the head of the file)
LOG_TOL = 3e-12
F_TOL = {(2, 5, 3): 5e-06, (2, 33, 2): 2e-05, (2, 64, 2): 3e-05, (2, 50, 10): 3e-05, (3, 7, 3): 4e-06, (8, 16, 17): 2e-05}
SIGMA_TOL = 3e-13
DISC_TOL = 4e-15
LONG_F_TOL = 5e-05


def _code(call):
    with pytest.raises(_hip.TnmlError) as ei:
        call()
    return ei.value.code


def context_M(D, cap, L):
    """the smallest M whose bond capacity max(M, D min(L, M)) holds `cap` (tests/test_gradient_step_gpu.py: at (8, 16, 17) M = 16
    itself would have the capacity 128, for which the prediction chain has no LDS tile)"""
    return next(M for M in range(1, cap + 1) if max(M, D * min(L, M)) >= cap)


def new_ctx(N, D, L, cap, cores, l, b=R.B):
    ctx = _hip.Context(N, D, L, context_M(D, cap, L), b)
    ctx.set_any_position(True)
    ctx.set_cores(cores, l)
    return ctx


def as64(cores):
    return [np.asarray(c, dtype=np.float64) for c in cores]


def relerr(a, ref):
    return float(np.abs(np.asarray(a, dtype=np.float64) - ref).max() / np.abs(ref).max())


def check_form(ctx, unit_ref, logn_ref, l, X, f_ref):
    """the figures of one committed call against the reference's unit cores: f error of the device through tnml_predict, f error
    of the device's cores and of the rounded reference's through the float64 chain, the two isometry defects"""
    dev, bond, lp = ctx.get_cores()
    assert lp == l and [int(v) for v in bond] == R.bonds_of(unit_ref)
    g = np.exp(logn_ref / len(dev))
    ref32 = [c.astype(np.float32).astype(np.float64) for c in R.with_gauge(unit_ref, logn_ref)[0]]
    f_dev = relerr(ctx.predict(X), f_ref)
    f_d64 = relerr(forward64(as64(dev), l, X.astype(np.float64)), f_ref)
    f_r32 = relerr(forward64(ref32, l, X.astype(np.float64)), f_ref)
    d_dev = R.isometry_defect([c / g for c in as64(dev)], l)
    d_r32 = R.isometry_defect([c / g for c in ref32], l)
    return f_dev, f_d64, f_r32, d_dev, d_r32


# ---------------------------------------------------------------------------------------------------------------
# 1. orthogonal form, spectra and the compression without a cut on every shape
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('row', R.ROWS, ids=lambda r: 'D%d_M%d_L%d' % r)
def test_orthogonal_form_and_spectra(row):
    D, cap, L = row
    worst = dict(log=0.0, f=0.0, f_before=0.0, f_d64=0.0, f_r32=0.0, sig=0.0, defect=0.0, defect_r32=0.0)
    for case in R.orth_cases():
        name, N, D_, L_, cap_, l, kind = case
        if (D_, cap_, L_) != row:
            continue
        cores, X = R.build_case(case)
        f_ref = forward64(cores, l, X.astype(np.float64))
        unit, logn_ref = R.orthogonalize(cores, l)
        ranks_ref, spectra_ref, _ = R.bond_spectra(cores, l)
        ctx = new_ctx(N, D, L, cap, cores, l)
        # spectra first: nothing may move
        slots0, lab0 = ctx.core_slots()
        ranks, sigma, logn_s = ctx.bond_spectra()
        slots1, lab1 = ctx.core_slots()
        assert np.array_equal(slots0.view(np.uint32), slots1.view(np.uint32)) and np.array_equal(lab0.view(np.uint32), lab1.view(np.uint32)), name
        assert [int(v) for v in ctx.get_cores()[1]] == R.bonds_of(cores) and ctx.l_pos == l, name
        assert [int(v) for v in ranks] == ranks_ref, (name, ranks, ranks_ref)
        worst['sig'] = max(worst['sig'], float(np.abs(sigma - R.pad_spectra(spectra_ref, sigma.shape[1])).max()))
        worst['log'] = max(worst['log'], abs(logn_s - logn_ref))
        # the orthogonal form
        f_before = relerr(ctx.predict(X), f_ref)
        bond, logn = ctx.orthogonalize()
        assert [int(v) for v in bond] == R.bonds_of(unit), (name, bond, R.bonds_of(unit))
        worst['log'] = max(worst['log'], abs(logn - logn_ref))
        f_dev, f_d64, f_r32, d_dev, d_r32 = check_form(ctx, unit, logn_ref, l, X, f_ref)
        print('%s: |dlog| %.1e, f %.2e through tnml_predict (%.2e before the call), %.2e through the float64 chain (rounded reference %.2e), '
              'defect %.2e (rounded reference %.2e)' % (name, abs(logn - logn_ref), f_dev, f_before, f_d64, f_r32, d_dev, d_r32))
        assert d_dev <= 10 * d_r32, (name, d_dev, d_r32)
        assert f_d64 <= 10 * f_r32, (name, f_d64, f_r32)
        for k, v in (('f', f_dev), ('f_before', f_before), ('f_d64', f_d64), ('f_r32', f_r32), ('defect', d_dev), ('defect_r32', d_r32)):
            worst[k] = max(worst[k], v)
        # slot floats behind the new cores are zero
        slots, lab = ctx.core_slots()
        dev = ctx.get_cores()[0]
        for i, c in enumerate(dev):
            tail = lab[c.size:] if i == l else slots[i, c.size:]
            assert not tail.any(), (name, i)
        # a second call keeps every bond; the compression without a cut gives the same bonds from the original cores
        bond2, logn2 = ctx.orthogonalize()
        assert np.array_equal(bond2, bond) and abs(logn2 - logn) <= 1e-6, name
        ctx.set_cores(cores, l)
        bond3, _, disc3, logn3 = ctx.compress(ctx.bond_capacity, 1.0)
        assert np.array_equal(bond3, bond) and not disc3.any() and abs(logn3 - logn) <= LOG_TOL, name
        ctx.close()
    print('row %s worst: %s' % (row, ', '.join('%s %.2e' % kv for kv in worst.items())))
    assert worst['log'] <= LOG_TOL and worst['sig'] <= SIGMA_TOL and worst['f'] <= F_TOL[row]


# ---------------------------------------------------------------------------------------------------------------
# 2. compression
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', R.COMPRESS_CASES, ids=lambda c: c[0])
def test_compression(case):
    name, (D, cap, L), N, l, m_max, thr = case
    cores, X = R.build_compress_case(case)
    unit, spectra_ref, disc_ref, logn_ref = R.compress(cores, l, m_max, thr)
    f_ref = forward64(R.with_gauge(unit, logn_ref)[0], l, X.astype(np.float64))
    ctx = new_ctx(N, D, L, max(R.bonds_of(cores)), cores, l)
    bond, sigma, disc, logn = ctx.compress(m_max, thr)
    assert [int(v) for v in bond] == R.bonds_of(unit), (bond, R.bonds_of(unit))
    f_dev, f_d64, f_r32, d_dev, d_r32 = check_form(ctx, unit, logn_ref, l, X, f_ref)
    dsig = float(np.abs(sigma - R.pad_spectra(spectra_ref, sigma.shape[1])).max())
    ddisc = float(np.abs(disc - disc_ref).max())
    print('%s: bonds %s, |dlog| %.1e, spectra %.1e, discarded %.1e, f %.2e through tnml_predict, %.2e through the float64 chain (rounded '
          'reference %.2e), defect %.2e (rounded reference %.2e)' % (name, [int(v) for v in bond], abs(logn - logn_ref), dsig, ddisc, f_dev, f_d64, f_r32, d_dev, d_r32))
    assert abs(logn - logn_ref) <= LOG_TOL and dsig <= SIGMA_TOL and ddisc <= DISC_TOL
    assert f_dev <= F_TOL[(D, cap, L)] and f_d64 <= 10 * f_r32 and d_dev <= 10 * d_r32
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------
# 3. a rank-deficient interior bond; a longer chain
# ---------------------------------------------------------------------------------------------------------------
def test_duplicated_column_drops_the_bond_by_exactly_one():
    cores, X, l, k = R.duplicated_column_case()
    N, D, L = len(cores), cores[0].shape[1], cores[l].shape[3]
    ctx = new_ctx(N, D, L, 5, cores, l)
    ranks, _, _ = ctx.bond_spectra()
    bond, logn = ctx.orthogonalize()
    want = R.bonds_of(cores)
    want[k] -= 1
    assert [int(v) for v in bond][3:13] == want[3:13] and int(ranks[k]) == want[k]
    assert [int(v) for v in bond] == R.bonds_of(R.orthogonalize(cores, l)[0])
    assert relerr(ctx.predict(X), forward64(cores, l, X.astype(np.float64))) <= F_TOL[(2, 5, 3)]
    ctx.close()


def test_largest_bond_the_kernel_takes():
    """bond 96: the largest dynamic LDS the chain kernel asks for (157 KB); N = 14 so that the middle bonds can be filled"""
    N, D, L, cap, l = 14, 2, 2, 96, 0
    rng = np.random.default_rng(96)
    X = R.features(rng, R.B, N, D)
    cores = R.make_cores(N, D, L, [cap] * (N - 1), l, rng, X)
    f_ref = forward64(cores, l, X.astype(np.float64))
    unit, logn_ref = R.orthogonalize(cores, l)
    assert max(R.bonds_of(unit)) == cap
    ctx = new_ctx(N, D, L, cap, cores, l)
    bond, logn = ctx.orthogonalize()
    f_dev, f_d64, f_r32, d_dev, d_r32 = check_form(ctx, unit, logn_ref, l, X, f_ref)
    print('bond 96: bonds %s, |dlog| %.1e, f %.2e through tnml_predict, %.2e through the float64 chain (rounded reference %.2e), defect %.2e '
          '(rounded reference %.2e)' % ([int(v) for v in bond], abs(logn - logn_ref), f_dev, f_d64, f_r32, d_dev, d_r32))
    assert abs(logn - logn_ref) <= LOG_TOL and f_d64 <= 10 * f_r32 and d_dev <= 10 * d_r32 and np.isfinite(ctx.predict(X)).all()
    ctx.close()


def test_long_chain_stays_inside_float32():
    cores, X, l = R.long_chain_case()
    N, D, L = len(cores), cores[0].shape[1], cores[l].shape[3]
    f_ref = forward64(cores, l, X.astype(np.float64))
    unit, logn_ref = R.orthogonalize(cores, l)
    ctx = new_ctx(N, D, L, 4, cores, l)
    f_before = relerr(ctx.predict(X), f_ref)
    bond, logn = ctx.orthogonalize()
    f_dev, f_d64, f_r32, d_dev, d_r32 = check_form(ctx, unit, logn_ref, l, X, f_ref)
    print('N = %d: g %.4g, |dlog| %.1e, f %.2e through tnml_predict (%.2e before the call), %.2e through the float64 chain (rounded reference '
          '%.2e), defect %.2e (rounded reference %.2e)' % (N, np.exp(logn / N), abs(logn - logn_ref), f_dev, f_before, f_d64, f_r32, d_dev, d_r32))
    assert np.isfinite(ctx.predict(X)).all() and abs(logn - logn_ref) <= 10 * LOG_TOL
    assert f_dev <= LONG_F_TOL and f_d64 <= 10 * f_r32 and d_dev <= 10 * d_r32
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------
# 4. exact checks: determinism, refusals, the state of the context
# ---------------------------------------------------------------------------------------------------------------
SWEEP = (1e-2, 1e-3, True, 'softmax', 'full_cross_ent', 0.1, 'fixed')
HYPER = (0.05, 1e-2, 'softmax', 'full_cross_ent', 1.0)


def small_problem(l=0, seed=11):
    N, D, L, cap = 12, 2, 2, 6
    rng = np.random.default_rng(seed)
    X = R.features(rng, 100, N, D)
    cores = R.make_cores(N, D, L, [cap] * (N - 1), l, rng, X)
    return N, D, L, cap, cores, X, rng.integers(0, L, 100).astype(np.int32)


def bits(ctx):
    slots, lab = ctx.core_slots()
    return slots.view(np.uint32).copy(), lab.view(np.uint32).copy(), [int(v) for v in ctx.get_cores()[1]], ctx.l_pos


def same_bits(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2] and a[3] == b[3]


def test_two_contexts_are_bit_equal():
    case = next(c for c in R.COMPRESS_CASES if c[0] == 'half_l8')
    name, (D, cap, L), N, l, m_max, thr = case
    cores, X = R.build_compress_case(case)
    out = []
    for _ in range(2):
        ctx = new_ctx(N, D, L, cap, cores, l)
        spec = ctx.bond_spectra()
        comp = ctx.compress(m_max, thr)
        state = bits(ctx)
        orth = ctx.orthogonalize()
        out.append((spec, comp, state, orth, bits(ctx)))
        ctx.close()
    a, b = out
    for k in (0, 1, 3):
        assert all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(a[k], b[k])), k
    assert same_bits(a[2], b[2]) and same_bits(a[4], b[4])


def test_refusals_leave_everything_as_it_was(monkeypatch):
    N, D, L, cap, cores, X, y = small_problem(l=3)
    lib, i32p, f64p = _hip.lib(), C.POINTER(C.c_int32), C.POINTER(C.c_double)
    ctx = _hip.Context(N, D, L, cap, 100)
    bond = np.zeros(N - 1, dtype=np.int32)
    sig = np.zeros((N - 1, ctx.bond_capacity))
    disc = np.zeros(N - 1)
    logn = C.c_double()
    bp, sp, dp, lp = bond.ctypes.data_as(i32p), sig.ctypes.data_as(f64p), disc.ctypes.data_as(f64p), C.byref(logn)
    assert lib.tnml_orthogonalize(ctx._h, 1e-6, bp, lp) == STATE                                  # cores never set
    assert lib.tnml_compress(ctx._h, 2, 1.0, 1e-6, bp, sp, dp, lp) == STATE
    assert lib.tnml_bond_spectra(ctx._h, 1e-6, bp, sp, lp) == STATE
    ctx.set_any_position(True)
    ctx.set_cores(cores, 3)
    before = bits(ctx)
    n = 0
    for rc in (lib.tnml_orthogonalize(None, 1e-6, bp, lp), lib.tnml_orthogonalize(ctx._h, 1e-6, None, lp),
               lib.tnml_orthogonalize(ctx._h, 1e-6, bp, None), lib.tnml_orthogonalize(ctx._h, -1e-6, bp, lp),
               lib.tnml_orthogonalize(ctx._h, 1.0, bp, lp), lib.tnml_orthogonalize(ctx._h, float('nan'), bp, lp),
               lib.tnml_compress(ctx._h, 0, 1.0, 1e-6, bp, sp, dp, lp), lib.tnml_compress(ctx._h, 2, 0.0, 1e-6, bp, sp, dp, lp),
               lib.tnml_compress(ctx._h, 2, 1.5, 1e-6, bp, sp, dp, lp), lib.tnml_compress(ctx._h, 2, float('nan'), 1e-6, bp, sp, dp, lp),
               lib.tnml_compress(ctx._h, 2, 1.0, 1e-6, None, sp, dp, lp), lib.tnml_compress(ctx._h, 2, 1.0, 1e-6, bp, None, dp, lp),
               lib.tnml_compress(ctx._h, 2, 1.0, 1e-6, bp, sp, None, lp), lib.tnml_compress(ctx._h, 2, 1.0, 1e-6, bp, sp, dp, None),
               lib.tnml_compress(ctx._h, 2, 1.0, 1.0, bp, sp, dp, lp), lib.tnml_bond_spectra(ctx._h, 1e-6, None, sp, lp),
               lib.tnml_bond_spectra(ctx._h, 1e-6, bp, None, lp), lib.tnml_bond_spectra(ctx._h, 1e-6, bp, sp, None),
               lib.tnml_bond_spectra(ctx._h, 2.0, bp, sp, lp)):
        assert rc == ARG
        n += 1
    assert n == 19 and same_bits(before, bits(ctx))
    # a network scaled by 1e30: reported, untouched
    ctx.scale_cores(1e30)
    scaled = bits(ctx)
    assert _code(lambda: ctx.orthogonalize()) == NONFINITE
    assert _code(lambda: ctx.compress(2)) == NONFINITE
    assert _code(lambda: ctx.bond_spectra()) == NONFINITE
    assert same_bits(scaled, bits(ctx))
    ctx.set_cores(cores, 3)
    ctx.orthogonalize()                                                                           # usable afterwards
    ctx.close()
    # a bond beyond the kernel's LDS: refused with the bytes in the message
    ctx = _hip.Context(4, 2, 2, 128, 64)
    rng = np.random.default_rng(3)
    big = R.make_cores(4, 2, 2, [2, 128, 2], 0, rng, R.features(rng, 8, 4, 2))
    ctx.set_cores(big, 0)
    before = bits(ctx)
    with pytest.raises(_hip.TnmlError, match='bytes of LDS') as ei:
        ctx.orthogonalize()
    assert ei.value.code == SHAPE and same_bits(before, bits(ctx))
    ctx.close()
    # a communicator attached
    from tensornetworkforml_amd import dist as tdist
    monkeypatch.setenv('TNML_FORCE_COMM', '1')
    N, D, L, cap, cores, X, y = small_problem(l=0)
    ctx = _hip.Context(N, D, L, cap, 100)
    ctx.set_cores(cores, 0)
    tdist.attach_comm(ctx, 0, 1)
    before = bits(ctx)
    for call in (ctx.orthogonalize, lambda: ctx.compress(2), ctx.bond_spectra):
        assert _code(call) == STATE
    assert same_bits(before, bits(ctx))
    ctx.close()


def test_context_state_after_a_call():
    N, D, L, cap, cores, X, y = small_problem(l=0)
    other = X[:64]
    yo = np.zeros(64, dtype=np.int32)
    ctx = _hip.Context(N, D, L, cap, 100)
    ctx.set_cores(cores, 0)
    ctx.set_input(X, y)
    ctx.forward()
    # spectra only: a sweep is still possible without a new forward
    ctx.bond_spectra()
    ctx.sweep(False, 2, True, *SWEEP)
    ctx.set_cores(cores, 0)
    ctx.set_input(X, y)
    ctx.forward()
    for call in (ctx.orthogonalize, lambda: ctx.compress(3)):
        call()
        assert _code(lambda: ctx.sweep(False, N - 1, True, *SWEEP)) == STATE                      # the resident f is stale
        f = ctx.forward()                                                                         # the resident batch stayed
        assert np.array_equal(f, ctx.predict(X))
    ctx.sweep(False, N - 1, True, *SWEEP)
    assert ctx.l_pos == N - 1
    # a bound optimiser state is unbound by a committed call, even where no bond changes; plain SGD has none
    for opt in (dict(kind='sgd', momentum=0.9), dict(kind='adam', eps=1e-3, clip=False)):
        ctx.set_cores(cores, 0)
        ctx.orthogonalize()                                                                       # (the bonds are at their ranks from here on)
        ctx.optim_config(**opt)
        ctx.gd_step(other, yo, *HYPER)
        ctx.bond_spectra()
        ctx.gd_step(other, yo, *HYPER)                                                            # spectra leave the state bound
        bond0 = ctx.get_cores()[1]
        bond, _ = ctx.orthogonalize()
        assert np.array_equal(bond, bond0)
        with pytest.raises(_hip.TnmlError, match='tnml_optim_reset') as ei:
            ctx.gd_step(other, yo, *HYPER)
        assert ei.value.code == STATE
        ctx.optim_reset()
        ctx.gd_step(other, yo, *HYPER)
        ctx.compress(3)
        assert _code(lambda: ctx.gd_step(other, yo, *HYPER)) == STATE
        ctx.optim_config('sgd', momentum=0.0, clip=True)
        ctx.gd_step(other, yo, *HYPER)
        ctx.orthogonalize()
        ctx.gd_step(other, yo, *HYPER)
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------
# 5. Network level; end to end
# ---------------------------------------------------------------------------------------------------------------
def _diagonals(n, D, seed):
    np.random.seed(seed)
    data, label = gen.create_dataset(n, 4, 0.3)
    pix = np.clip(data.reshape(n, -1), 0.0, 1.0).astype(np.float32)
    return pix, label, gen.psi(pix.astype(np.float64), D)


def test_network_methods_equal_the_context_calls():
    import tensornetworkforml_amd as pkg
    N, D, L, M, n = 16, 2, 2, 4, 200
    pix, label, X = _diagonals(n, D, 3)
    net = pkg.Network(N=N, M=M, D=D, L=L, normalize=True, calibration_X=X[:16], act_fn='softmax', loss_fn='full_cross_ent', T=1.0, trunc='fixed')
    net.attach_dataset(pix, label, pixels=True)
    net.gradient_step(np.arange(50), lr=0.05)
    start, _, lp = net._ctx.get_cores()
    twin = _hip.Context(N, D, L, M, 64)
    twin.set_cores(start, lp)
    with pytest.raises(ValueError):
        net.compress()
    spectra, logn = net.bond_spectra()
    rk, sg, ln = twin.bond_spectra()
    assert logn == ln and len(spectra) == N - 1 and all(np.array_equal(s, sg[i, :int(rk[i])]) for i, s in enumerate(spectra))
    assert net.orthogonalize() == twin.orthogonalize()[1]
    assert all(np.array_equal(a, c) for a, c in zip(net._ctx.get_cores()[0], twin.get_cores()[0]))
    bonds, disc = net.compress(max_bond=2)
    tb, _, td, _ = twin.compress(2)
    assert bonds == [int(v) for v in tb] and np.array_equal(disc, td) and max(bonds) == 2
    bonds, disc = net.compress(threshold=0.9)
    tb, _, td, _ = twin.compress(twin.bond_capacity, 0.9)
    assert bonds == [int(v) for v in tb] and np.array_equal(disc, td)
    final = twin.get_cores()[0]
    # the host copy follows the device; a pickled and restored network holds the new cores and bonds
    As = net.As
    assert len(As) == N and all(np.array_equal(h.astype(np.float32), c) for h, c in zip(net._host_cores, final))
    back = pickle.loads(pickle.dumps(net))
    assert np.array_equal(np.asarray(back.predict(X[:20]).elem).astype(np.float32), twin.predict(X[:20].astype(np.float32)))
    assert all(np.array_equal(a, c) for a, c in zip(back._ctx.get_cores()[0], final))
    # a forward makes sweeping possible again
    f = net.forward(X[:64])
    net.sweep(X[:64], label[:64], f, 1e-2, 1e-3)
    twin.close()


def test_end_to_end_fine_tune_compress_sweep():
    """Diagonals, N = 16, bond 4, 200 samples: a few gradient steps, compress(max_bond = 2), forward and one sweep; the accuracy
    after the compression against the reference's on the same cores (count difference as in the training run of
    tests/test_gradient_step_gpu.py: 2)."""
    N, D, L, M, n = 16, 2, 2, 4, 200
    pix, label, X = _diagonals(n, D, 5)
    X32 = X.astype(np.float32)
    rng = np.random.default_rng(21)
    cores = R.make_cores(N, D, L, [M] * (N - 1), 0, rng, X32, delta=0.5)
    ctx = _hip.Context(N, D, L, M, n)
    ctx.set_cores(cores, 0)
    ctx.dataset_attach(pix, label, 'pixels')
    ctx.optim_config('sgd', clip=True)
    for k in range(4):
        ctx.gd_train_indices(np.arange(n), 50, 0.05, 0.0, 'softmax', 'full_cross_ent', 1.0)
    tuned = as64(ctx.get_cores()[0])
    correct0 = ctx.eval_indices(np.arange(n), 'softmax', 1.0)[0]
    bond, _, disc, logn = ctx.compress(2)
    unit, _, disc_ref, logn_ref = R.compress(tuned, 0, 2, 1.0)
    assert [int(v) for v in bond] == R.bonds_of(unit) and max(bond) == 2
    correct1 = ctx.eval_indices(np.arange(n), 'softmax', 1.0)[0]
    f_ref = forward64(R.with_gauge(unit, logn_ref)[0], 0, X)
    correct_ref = int((np.argmax(f_ref, axis=0) == label).sum())
    print('accuracy %.3f before, %.3f after the compression (reference %.3f); discarded %.2e' % (correct0 / n, correct1 / n, correct_ref / n, disc.sum()))
    assert abs(correct1 - correct_ref) <= 2
    ctx.select_indices(np.arange(n))
    f = ctx.forward()
    assert np.isfinite(f).all()
    met, f = ctx.sweep(False, N - 1, True, *SWEEP)
    assert np.isfinite(met).all() and np.isfinite(f).all() and all(np.isfinite(c).all() for c in ctx.get_cores()[0])
    ctx.close()
