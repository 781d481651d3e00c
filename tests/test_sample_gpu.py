"""tnml_sample on the device against the float64 reference of tests/sample_reference.py.  Every comparison is
with the reference or with a dense enumeration, never with the device's own output.  Draws are compared on the samples the reference
calls decidable (every cumulative sum at least 1e-9, relative, away from its threshold: tests/test_sample_host.py asserts that these
are at least 95 % of every case); their levels and labels must be equal, their logp within the bounds below, each ten times the worst
value observed on an MI355X in its class, rounded up to one digit (the table is in DESIGN.md section 22)."""
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
import sample_reference as S                                       # noqa: E402
from tensornetworkforml_amd import _hip                            # noqa: E402
from tensornetworkforml_amd import data_generator as gen           # noqa: E402

pytestmark = pytest.mark.gpu

ARG, STATE, SHAPE, NONFINITE = -1, -2, -6, -7
# Observed on an MI355X (worst |dlogp| over the decidable samples of each class) -> bound = 10 x the worst, rounded up to one digit:
#   draws, N = 17 ragged, 51 cases (2.84e-14, 2.84e-14, 4.26e-14 per row), bonds 50 and 64 (2.13e-14, 7.11e-15)   4.26e-14 -> 5e-13
#   log_prob against the dense table, N = 4, 162 rows (conditional 3.24e-12, joint 3.24e-12: the smallest
#     probability of the table is 6.5e-7 of the largest, the rest of a cancellation)                         3.24e-12 -> 4e-11
#   prefix, both columns, and the likelihood call on the same samples                                         1.42e-13 -> 2e-12
#   N = 784 (calibrated 9.09e-13, raw 9.09e-13; log p about -4330)                                            9.09e-13 -> 1e-11
#   log p(x, l) - log p(x, l') against 2 log|f_l / f_l'| of tnml_predict, 43 pairs: the float32 forward
#     chain's error, not this code's                                                                          1.91e-06 -> 2e-05
LOGP_TOL_DRAWS = 5e-13
LOGP_TOL_DENSE = 4e-11
LOGP_TOL_PREFIX = 2e-12
LOGP_TOL_LONG = 1e-11
LOGP_TOL_PREDICT = 2e-05
SWEEP = (1e-2, 1e-3, True, 'softmax', 'full_cross_ent', 0.1, 'fixed')


def _code(call):
    with pytest.raises(_hip.TnmlError) as ei:
        call()
    return ei.value.code


def context_M(D, cap, L):
    return next(M for M in range(1, cap + 1) if max(M, D * min(L, M)) >= cap)


def new_ctx(N, D, L, cap, b=8):
    ctx = _hip.Context(N, D, L, context_M(D, cap, L), b)
    ctx.set_any_position(True)
    return ctx


def network_of(cores, l, M, D, L):
    import tensornetworkforml_amd as pkg
    net = pkg.Network_class.Network(len(cores), M, D=D, L=L, trunc='fixed')
    net._host_cores = A.as64(cores)
    net._l_pos = l
    net._host_newer = True
    net.any_position = True
    return net


def bits(ctx):
    cores, bond, lp = ctx.get_cores()
    slots, lab = ctx.core_slots()
    return [c.tobytes() for c in cores], bond.tobytes(), lp, slots.tobytes(), lab.tobytes()


def compare(dev, ref):
    """(decidable samples, worst |dlogp| over them); their levels and labels must be equal"""
    (lv, lb, lp), (rlv, rlb, rlp, mg) = dev, ref
    ok = S.decidable(mg)
    assert np.array_equal(lv[ok], rlv[ok]) and np.array_equal(lb[ok], rlb[ok]), 'a decidable sample differs'
    assert np.all(np.isfinite(lp[ok]))
    return int(ok.sum()), float(np.abs(lp[ok] - rlp[ok]).max()) if ok.any() else 0.0


# ---------------------------------------------------------------------------------------------------------------
# 1. draws equal the reference's
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('row', S.ROWS, ids=lambda r: 'D%d_L%d' % r)
def test_draws_equal_the_reference(row):
    D, L = row
    ctx = new_ctx(17, D, L, 7)
    worst, n_ok, n_all = 0.0, 0, 0
    for case in [c for c in S.draw_cases() if (c[1], c[2]) == row]:
        N, _, _, l, K = case
        cores, phi, w, classes, u = S.build_draw_case(case)
        ctx.set_cores(A.as32(cores), l)
        k, err = compare(ctx.sample(S.N_DRAWS, phi, w, classes, None, u), S.walk(cores, l, phi, w, classes, u))
        assert k >= 0.95 * S.N_DRAWS, case
        worst, n_ok, n_all = max(worst, err), n_ok + k, n_all + S.N_DRAWS
    ctx.close()
    print('D %d L %d: %d of %d samples decidable and equal, |dlogp| %.2e' % (D, L, n_ok, n_all, worst))
    assert n_all == 17 * S.N_DRAWS and worst <= LOGP_TOL_DRAWS


@pytest.mark.parametrize('case', S.wide_cases(), ids=lambda c: 'bond%d' % c[4])
def test_draws_at_bonds_50_and_64(case):
    N, D, L, l, M, K = case
    cores, phi, w, classes, u = S.build_wide_case(case)
    ctx = new_ctx(N, D, L, M)
    ctx.set_cores(A.as32(cores), l)
    k, err = compare(ctx.sample(S.N_DRAWS, phi, w, classes, None, u), S.walk(cores, l, phi, w, classes, u))
    ctx.close()
    print('bond %d: %d of %d samples decidable and equal, |dlogp| %.2e' % (M, k, S.N_DRAWS, err))
    assert k >= 0.95 * S.N_DRAWS and err <= LOGP_TOL_DRAWS


# ---------------------------------------------------------------------------------------------------------------
# 2. log_prob against dense enumeration
# ---------------------------------------------------------------------------------------------------------------
def test_log_prob_against_dense_enumeration():
    D, L, N, K, l = 2, 2, 4, 3, 2
    cores, phi, w = S.dense_case(D, L, N, K, l)
    P = S.dense_joint(cores, l, phi, w)
    lev, lab = S.dense_rows(N, K, L)
    assert len(lab) == 162
    net = network_of(cores, l, 4, D, L)
    cond, labels = net.log_prob(lev, classes=lab, levels=K, weights=w)
    assert np.array_equal(labels, lab)
    Pc = P / P.reshape(-1, L).sum(axis=0)
    e_cond = float(np.abs(cond - np.log(Pc.ravel())).max())
    joint, _ = net.log_prob(lev, classes=lab, levels=K, weights=w, joint=True)
    e_joint = float(np.abs(joint - np.log(P.ravel())).max())
    print('162 rows: conditional |dlogp| %.2e, joint %.2e, sums %.15f %.15f' % (e_cond, e_joint, np.exp(joint).sum(), np.exp(cond).sum() / L))
    assert e_cond <= LOGP_TOL_DENSE and e_joint <= LOGP_TOL_DENSE
    assert abs(np.exp(joint).sum() - 1.0) <= 162 * LOGP_TOL_DENSE and abs(np.exp(cond).sum() - L) <= 162 * LOGP_TOL_DENSE
    # pixel values on the grid are levels; values off the grid are refused
    x = np.arange(K) / (K - 1)
    again, _ = net.log_prob(x[lev], classes=lab, levels=K, weights=w)
    assert np.array_equal(again, cond)
    with pytest.raises(ValueError, match='not on the grid'):
        net.log_prob(x[lev] + 0.01, classes=lab, levels=K, weights=w)
    # the label drawn from P(l | x): log p(x, l) of the dense table at that label
    drawn, labels = net.log_prob(lev[::L], levels=K, weights=w, seed=5)
    ref = np.log(P.reshape(-1, L)[np.arange(81), labels])
    assert float(np.abs(drawn - ref).max()) <= LOGP_TOL_DENSE


# ---------------------------------------------------------------------------------------------------------------
# 3. seeded calls
# ---------------------------------------------------------------------------------------------------------------
def test_seeded_calls_equal_the_hash_and_repeat_bit_for_bit():
    case = (17, 3, 3, 8, 7)
    N, D, L, l, K = case
    cores, phi, w, classes, _ = S.build_draw_case(case)
    ctx = new_ctx(N, D, L, 7)
    ctx.set_cores(A.as32(cores), l)
    for seed in (0, 12345, 2 ** 64 - 1):
        a = ctx.sample(S.N_DRAWS, phi, w, classes, None, None, seed)
        b = ctx.sample(S.N_DRAWS, phi, w, classes, None, S.hash_uniforms(seed, S.N_DRAWS, N))
        c = ctx.sample(S.N_DRAWS, phi, w, classes, None, None, seed)
        for x, y, z in zip(a, b, c):
            assert x.tobytes() == y.tobytes() == z.tobytes(), seed
    d = ctx.sample(S.N_DRAWS, phi, w, classes, None, None, 1)
    assert not np.array_equal(a[0], d[0])
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------
# 4. frequencies
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', S.FREQ_CASES, ids=lambda c: 'N%d_K%d_D%d_L%d_l%d' % c)
def test_frequencies_against_the_dense_probabilities(case):
    N, K, D, L, l = case
    cores, phi, w = S.dense_case(D, L, N, K, l)
    P = S.dense_joint(cores, l, phi, w).ravel()
    ctx = new_ctx(N, D, L, 3)
    ctx.set_cores(A.as32(cores), l)
    lev, lab, _ = ctx.sample(S.FREQ_N, phi, w, None, None, None, S.FREQ_SEED)
    ctx.close()
    chi2, dof = S.chi_square(S.outcome_counts(lev, lab, K, L), P, S.FREQ_N)
    print('N %d K %d D %d L %d label on %d: chi2 %.1f at dof %d (bound %.1f)' % (N, K, D, L, l, chi2, dof, S.chi_bound(dof)))
    assert dof >= 1 and chi2 <= S.chi_bound(dof)


# ---------------------------------------------------------------------------------------------------------------
# 5. prefix
# ---------------------------------------------------------------------------------------------------------------
def test_prefix_and_likelihood_calls():
    worst = 0.0
    for case in [(17, 2, 2, 12, 7), (17, 3, 3, 3, 256), (17, 8, 10, 8, 2)]:
        N, D, L, l, K = case
        cores, phi, w, classes, u = S.build_draw_case(case)
        rng = np.random.default_rng(5)
        ctx = new_ctx(N, D, L, 7)
        ctx.set_cores(A.as32(cores), l)
        given = rng.integers(0, K, (S.N_DRAWS, N // 2)).astype(np.int32)
        dev, ref = ctx.sample(S.N_DRAWS, phi, w, classes, given, u), S.walk(cores, l, phi, w, classes, u, given)
        assert np.array_equal(dev[0][:, :N // 2], given)
        k, err = compare(dev, ref)
        assert k >= 0.95 * S.N_DRAWS
        worst = max(worst, err)
        # n_given = N: nothing but a label is drawn, and both columns agree where the class is given
        full = ctx.sample(S.N_DRAWS, phi, w, classes, dev[0], u)
        rfull = S.walk(cores, l, phi, w, classes, u, dev[0])
        k, err = compare(full, rfull)
        worst = max(worst, err)
        fixed = classes >= 0
        assert np.array_equal(full[0], dev[0]) and np.array_equal(full[2][fixed, 0], full[2][fixed, 1])
        ok = S.decidable(ref[3]) & S.decidable(rfull[3]) & (full[1] == dev[1])
        assert float(np.abs(full[2][ok, 0] - dev[2][ok, 0]).max()) <= LOGP_TOL_PREFIX                 # the same sample, the same log p
        net = network_of(cores, l, 7, D, L)
        lp, _ = net.log_prob(dev[0][fixed], classes=classes[fixed], levels=K, weights=w)
        assert float(np.abs(lp - full[2][fixed, 0]).max()) <= LOGP_TOL_PREFIX                         # (Network normalises the weights again)
        ctx.close()
    print('prefix: |dlogp| %.2e' % worst)
    assert worst <= LOGP_TOL_PREFIX


# ---------------------------------------------------------------------------------------------------------------
# 6. long chain
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('which', [0, 1], ids=['calibrated', 'raw'])
def test_long_chain(which):
    name, W, l = S.long_cases()[which]
    N, D, L, K = 784, 2, 2, 256
    _, phi, w = S.grid(K, D)
    classes = np.array([-1, 0, 1, -1] * (S.LONG_N // 4), dtype=np.int32)
    u = S.hash_uniforms(784, S.LONG_N, N)
    ctx = new_ctx(N, D, L, 20)
    ctx.set_cores(A.as32(W), l)
    dev = ctx.sample(S.LONG_N, phi, w, classes, None, u)
    ctx.close()
    k, err = compare(dev, S.walk(W, l, phi, w, classes, u))
    print('N 784 %s: %d of %d samples decidable and equal, |dlogp| %.2e, logp about %.1f' % (name, k, S.LONG_N, err, dev[2][:, 0].mean()))
    assert k >= 0.95 * S.LONG_N and err <= LOGP_TOL_LONG and np.all(np.isfinite(dev[2]))


# ---------------------------------------------------------------------------------------------------------------
# 7. against predict
# ---------------------------------------------------------------------------------------------------------------
def test_log_prob_differences_against_predict():
    """log p(x, l) - log p(x, l') = 2 log|f_l(x) / f_l'(x)|: the new path against the float32 forward chain, which limits it"""
    case = (17, 2, 3, 8, 256)
    N, D, L, l, K = case
    cores, phi, w, _, _ = S.build_draw_case(case)
    net = network_of(cores, l, 7, D, L)
    X, labels, _, lev = net.sample(24, levels=K, seed=3)
    f = net._sync_to_device(1).predict(gen.psi(X, D)).astype(np.float64)                              # (L, n)
    lp = np.stack([net.log_prob(lev, classes=c, levels=K, joint=True)[0] for c in range(L)])
    worst, n = 0.0, 0
    for s in range(24):
        use = [c for c in range(L) if abs(f[c, s]) >= 0.1 * np.abs(f[:, s]).max()]
        for c in use[1:]:
            worst = max(worst, abs((lp[c, s] - lp[use[0], s]) - 2.0 * math.log(abs(f[c, s] / f[use[0], s]))))
            n += 1
    print('against predict: %d pairs, worst %.2e' % (n, worst))
    assert n >= 12 and worst <= LOGP_TOL_PREDICT


# ---------------------------------------------------------------------------------------------------------------
# 8. state and refusals
# ---------------------------------------------------------------------------------------------------------------
def test_state_and_refusals(monkeypatch):
    case = (17, 2, 2, 0, 256)
    N, D, L, l, K = case
    cores, phi, w, classes, u = S.build_draw_case(case)
    n = S.N_DRAWS
    lib = _hip.lib()
    i32p, f64p = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    lev, lab, lp = np.zeros((n, N), dtype=np.int32), np.zeros(n, dtype=np.int32), np.zeros((n, 2))
    pp, wp, cp, up = phi.ctypes.data_as(f64p), w.ctypes.data_as(f64p), classes.ctypes.data_as(i32p), u.ctypes.data_as(f64p)
    lvp, lbp, lpp = lev.ctypes.data_as(i32p), lab.ctypes.data_as(i32p), lp.ctypes.data_as(f64p)
    ctx = new_ctx(N, D, L, 7, R.B)
    assert lib.tnml_sample(ctx._h, n, K, pp, wp, cp, None, 0, up, 0, lvp, lbp, lpp) == STATE                      # cores never set
    ctx.set_cores(A.as32(cores), l)
    X = R.features(np.random.default_rng(1), R.B, N, D)
    ctx.set_input(X, (np.arange(R.B) % L).astype(np.int32))
    f = ctx.forward()
    side = _hip.SIDE_RIGHT
    envs = [ctx.get_env(side, i).tobytes() for i in range(l + 1, N)]
    before = bits(ctx)
    ctx.sample(n, phi, w, classes, None, u)
    bad_cls, bad_given, bad_w, bad_phi, bad_u = classes.copy(), np.zeros((n, 2), dtype=np.int32), w.copy(), phi.copy(), u.copy()
    bad_cls[5], bad_given[3, 1], bad_w[2], bad_phi[1, 0], bad_u[0, 0] = L, K, 0.0, np.inf, 1.0
    neg_cls, nan_w = classes.copy(), w.copy()
    neg_cls[0], nan_w[0] = -2, np.nan
    gp = bad_given.ctypes.data_as(i32p)
    codes = [lib.tnml_sample(None, n, K, pp, wp, cp, None, 0, up, 0, lvp, lbp, lpp),
             lib.tnml_sample(ctx._h, 0, K, pp, wp, cp, None, 0, up, 0, lvp, lbp, lpp),
             lib.tnml_sample(ctx._h, n, 1, pp, wp, cp, None, 0, up, 0, lvp, lbp, lpp),
             lib.tnml_sample(ctx._h, n, 257, pp, wp, cp, None, 0, up, 0, lvp, lbp, lpp),
             lib.tnml_sample(ctx._h, n, K, pp, wp, bad_cls.ctypes.data_as(i32p), None, 0, up, 0, lvp, lbp, lpp),
             lib.tnml_sample(ctx._h, n, K, pp, wp, neg_cls.ctypes.data_as(i32p), None, 0, up, 0, lvp, lbp, lpp),
             lib.tnml_sample(ctx._h, n, K, pp, wp, cp, gp, 2, up, 0, lvp, lbp, lpp),
             lib.tnml_sample(ctx._h, n, K, pp, wp, cp, gp, -1, up, 0, lvp, lbp, lpp),
             lib.tnml_sample(ctx._h, n, K, pp, wp, cp, gp, N + 1, up, 0, lvp, lbp, lpp),
             lib.tnml_sample(ctx._h, n, K, pp, wp, cp, None, 2, up, 0, lvp, lbp, lpp),
             lib.tnml_sample(ctx._h, n, K, pp, bad_w.ctypes.data_as(f64p), cp, None, 0, up, 0, lvp, lbp, lpp),
             lib.tnml_sample(ctx._h, n, K, pp, nan_w.ctypes.data_as(f64p), cp, None, 0, up, 0, lvp, lbp, lpp),
             lib.tnml_sample(ctx._h, n, K, bad_phi.ctypes.data_as(f64p), wp, cp, None, 0, up, 0, lvp, lbp, lpp),
             lib.tnml_sample(ctx._h, n, K, pp, wp, cp, None, 0, bad_u.ctypes.data_as(f64p), 0, lvp, lbp, lpp),
             lib.tnml_sample(ctx._h, n, K, None, wp, cp, None, 0, up, 0, lvp, lbp, lpp),
             lib.tnml_sample(ctx._h, n, K, pp, wp, cp, None, 0, up, 0, None, lbp, lpp),
             lib.tnml_sample(ctx._h, n, K, pp, wp, cp, None, 0, up, 0, lvp, None, lpp),
             lib.tnml_sample(ctx._h, n, K, pp, wp, cp, None, 0, up, 0, lvp, lbp, None)]
    assert codes == [ARG] * 18, codes
    assert bits(ctx) == before and ctx.get_f().tobytes() == f.tobytes()
    assert [ctx.get_env(side, i).tobytes() for i in range(l + 1, N)] == envs
    ctx.sweep(False, 2, True, *SWEEP)                                                                  # no new forward needed
    # a class whose label slice is zero: the error names the sample and the class
    zero = [c.copy() for c in cores]
    zero[l][..., 1] = 0.0
    ctx.set_cores(A.as32(zero), l)
    before = bits(ctx)
    only = np.full(n, -1, dtype=np.int32)
    only[7] = 1
    with pytest.raises(_hip.TnmlError, match=r'sample 7 is conditioned on class 1') as ei:
        ctx.sample(n, phi, w, only, None, u)
    assert ei.value.code == ARG and bits(ctx) == before
    lv0, lb0, _ = ctx.sample(n, phi, w, None, None, u)                                                # drawn labels avoid the empty class
    assert np.all(lb0 == 0)
    # a NaN core
    nan = [c.copy() for c in cores]
    nan[9][0, 0, 0] = np.nan
    ctx.set_cores(A.as32(nan), l)
    assert _code(lambda: ctx.sample(n, phi, w, classes, None, u)) == NONFINITE
    nan = [c.copy() for c in cores]
    nan[0][0, 1, 0] = np.nan
    ctx.set_cores(A.as32(nan), l)
    assert _code(lambda: ctx.sample(n, phi, w, classes, None, u)) == NONFINITE
    ctx.set_cores(A.as32(cores), l)
    k, err = compare(ctx.sample(n, phi, w, classes, None, u), S.walk(cores, l, phi, w, classes, u))   # usable afterwards
    assert k >= 0.95 * n and err <= LOGP_TOL_DRAWS
    ctx.close()
    # a bond the kernels have no room for
    ctx = _hip.Context(4, 2, 2, 128, 8)
    rng = np.random.default_rng(3)
    big = R.make_cores(4, 2, 2, [2, 128, 2], 0, rng, R.features(rng, 8, 4, 2))
    ctx.set_cores(A.as32(big), 0)
    before = bits(ctx)
    with pytest.raises(_hip.TnmlError, match='bytes of LDS') as ei:
        ctx.sample(4, phi, w)
    assert ei.value.code == SHAPE and bits(ctx) == before
    ctx.close()
    # a communicator attached
    from tensornetworkforml_amd import dist as tdist
    monkeypatch.setenv('TNML_FORCE_COMM', '1')
    ctx = _hip.Context(N, D, L, 7, 8)
    c0 = S.chain(N, D, L, [3] * (N - 1), 0, np.random.default_rng(2))
    ctx.set_cores(A.as32(c0), 0)
    tdist.attach_comm(ctx, 0, 1)
    assert _code(lambda: ctx.sample(4, phi, w)) == STATE
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------
# 9. the scripts
# ---------------------------------------------------------------------------------------------------------------
def test_scripts_write_samples_and_print_log_prob(tmp_path, monkeypatch, capsys):
    from tensornetworkforml_amd import evaluate_diagonals as eval_script
    from tensornetworkforml_amd import training_diagonals as train_script
    monkeypatch.chdir(tmp_path)
    out, img = str(tmp_path / 'diag.dat'), str(tmp_path / 'img.npy')
    np.random.seed(4)
    train_script.main(['--n_samples', '400', '--linear_dim', '4', '--M', '4', '--n_epochs', '1', '--trunc', 'fixed', '--resident', '--out', out])
    capsys.readouterr()
    np.random.seed(5)
    eval_script.main(['--filename', out, '--n_samples', '200', '--sample', img, '--sample-n', '48', '--sample-class', '1', '--seed', '9', '--log-prob'])
    lines = capsys.readouterr().out.splitlines()
    X = np.load(img)
    assert X.shape == (48, 4, 4) and np.all((X >= 0.0) & (X <= 1.0)) and np.array_equal(np.rint(X * 255) / 255, X)
    cls = [ln for ln in lines if 'Samples of class' in ln]
    assert len(cls) == 1 and 'class 1: 48, mean log p(x | l)' in cls[0] and math.isfinite(float(cls[0].rsplit(' ', 1)[1]))
    lp = [ln for ln in lines if 'Mean log p(x, y)' in ln]
    assert len(lp) == 1 and 'over 200 samples' in lp[0]
    mean = float(lp[0].split(':')[1].split()[0])
    assert math.isfinite(mean) and mean < 0.0
    eval_script.main(['--filename', out, '--n_samples', '50', '--sample', img, '--sample-n', '20'])
    cls = [ln for ln in capsys.readouterr().out.splitlines() if 'Samples of class' in ln]
    assert 1 <= len(cls) <= 2 and all('mean log p(x, l)' in ln for ln in cls) and np.load(img).shape == (20, 4, 4)
