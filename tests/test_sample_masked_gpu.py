"""tnml_sample_masked on the device against the float64 reference of tests/sample_masked_reference.py.  Every
comparison is with the reference or with a dense enumeration, never with the device's own output, except where bit-equality between
two device calls is the claim.  Draws are compared on the samples the reference calls decidable (tests/test_sample_masked_host.py
asserts that these are at least 95 % of every case); their levels and labels must be equal, their logp within the bounds below, each
ten times the worst value observed on an MI355X in its class, rounded up to one digit (the table is in DESIGN.md section 23)."""
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
import sample_masked_reference as M                                # noqa: E402
import sample_reference as S                                       # noqa: E402
import test_sample_gpu as G                                        # noqa: E402  (its helpers: new_ctx, network_of, bits)
from tensornetworkforml_amd import _hip                            # noqa: E402
from tensornetworkforml_amd import data_generator as gen           # noqa: E402

pytestmark = pytest.mark.gpu

ARG, STATE, SHAPE, NONFINITE = -1, -2, -6, -7
# Observed on an MI355X (worst |dlogp| over the decidable samples of each class, both columns) -> bound = 10 x the worst, rounded up
# to one digit:
#   dense tables, N = 4, 192 rows a label position: marginal 3.55e-14, completion 1.07e-14, class weights 6.66e-16,
#     posterior 1.40e-11 (what a cancellation leaves, as in tests/test_sample_gpu.py), log_prob_masked 3.55e-14           1.40e-11 -> 2e-10
#   draws, N = 17 ragged, 51 cases, per-sample and shared masks, all 4080 samples equal, per row (D, L):
#     (2, 2) 3.29e-11 -> 4e-10      (3, 3) 4.53e-10 -> 5e-9      (8, 10) 2.23e-08 -> 3e-7
#     These are 1e3 to 5e5 times the 4.26e-14 of tnml_sample's draws, and all of it is in logp[:, 1] = log p(known levels): the known
#     levels of these cases are RANDOM, an image the model gives log p = -30 .. -110, and f of such an image is what a cancellation
#     between the chain's terms leaves, so the relative error of f^2 in float64 is eps times a condition number of 1e5 .. 1e8 in
#     ANY summation order.  The float64 NumPy reference itself differs from the same recursion in long double by 5.24e-11, 4.42e-09
#     and 1.62e-08 on the three rows (the worst sample of each: a full or nearly full mask) -- the device is as close to the
#     reference as the reference is to the truth.  tnml_sample's own draws never meet this: a DRAWN image is a probable one.
#   bonds 50 and 64 (tiles of 2 and 1), suffix and random masks: 1.42e-14, 2.97e-12, 5.33e-15, 2.49e-14                  2.97e-12 -> 3e-11
#   logp0 + logp1 against the likelihood call of tnml_sample on the completed image (random known levels again)           2.53e-12 -> 3e-11
#   N = 784, both chains, four masks (log p about -2170 a column; -4330 with the empty mask): 4.55e-13 .. 9.09e-13        9.09e-13 -> 1e-11
#   classify_masked with a full mask against 2 log|f_c / f_c'| of tnml_predict, 43 pairs: the float32 forward chain's
#     error, the bound of tests/test_sample_gpu.py                                                                         1.91e-06 -> 2e-05
LOGP_TOL_DENSE = 2e-10
LOGP_TOL_DRAWS = {(2, 2): 4e-10, (3, 3): 5e-9, (8, 10): 3e-7}
LOGP_TOL_WIDE = 3e-11
LOGP_TOL_IDENT = 3e-11
LOGP_TOL_LONG = 1e-11
LOGP_TOL_PREDICT = G.LOGP_TOL_PREDICT


def compare(dev, ref, mask=None, known=None):
    """(decidable samples, worst |dlogp| over them, both columns); their levels and labels must be equal, known sites as given"""
    (lv, lb, lp), (rlv, rlb, rlp, mg) = dev[:3], ref
    ok = S.decidable(mg)
    assert np.array_equal(lv[ok], rlv[ok]) and np.array_equal(lb[ok], rlb[ok]), 'a decidable sample differs'
    if mask is not None:
        mm = np.broadcast_to(mask, lv.shape)
        assert np.array_equal(lv[mm], known[mm]), 'a known site came back changed'
    assert np.all(np.isfinite(lp[ok]))
    return int(ok.sum()), float(np.abs(lp[ok] - rlp[ok]).max()) if ok.any() else 0.0


# ---------------------------------------------------------------------------------------------------------------
# 1. dense tables
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('l', [0, 2, 3])
def test_dense_marginals_conditionals_and_posteriors(l):
    D, L, N, K = 2, 2, 4, 3
    cores, phi, w = S.dense_case(D, L, N, K, l)
    P = S.dense_joint(cores, l, phi, w)
    masks = M.all_masks(N)
    per = 12
    n = per * len(masks)
    rng = np.random.default_rng([41, l])
    mask = np.repeat(np.array(masks), per, axis=0)
    classes = np.tile(np.array([-1, 0, 1] * 4, dtype=np.int32), len(masks))
    known = rng.integers(0, K, (n, N)).astype(np.int32)
    u = rng.random((n, N + 1))
    ctx = G.new_ctx(N, D, L, 3)
    ctx.set_cores(A.as32(cores), l)
    lev, lab, lp, clw = ctx.sample_masked(n, phi, w, mask, known, classes, u, class_logw=True)
    _, lab0, lp0 = ctx.sample_masked(n, phi, w, mask, known, classes, draw=False)
    ctx.close()
    assert np.array_equal(lev[mask], known[mask]) and np.array_equal(lab[classes >= 0], classes[classes >= 0])
    assert np.array_equal(lab0, classes) and np.array_equal(lp0[:, 1], lp[:, 1]) and np.all(lp0[:, 0] == 0.0)
    e1 = max(abs(lp[s, 1] - math.log(M.dense_marginal(P, mask[s], known[s], classes[s]))) for s in range(n))
    e0 = max(abs(lp[s, 0] - math.log(M.dense_completion(P, mask[s], known[s], classes[s], lev[s], lab[s]))) for s in range(n))
    ec = float(np.abs(clw - np.log(P.reshape(-1, L).sum(axis=0))).max())
    # the posterior over the class, hidden pixels summed out
    net = G.network_of(cores, l, 4, D, L)
    pred, log_post = net.classify_masked(known, mask, levels=K, weights=w)
    post = np.array([M.dense_posterior(P, mask[s], known[s]) for s in range(n)])
    ep = float(np.abs(log_post - np.log(post)).max())
    clear = np.abs(post[:, 0] - post[:, 1]) > 1e-9
    assert np.array_equal(pred[clear], post.argmax(axis=1)[clear])
    lpm = net.log_prob_masked(known, mask, levels=K, weights=w)
    ej = max(abs(lpm[s] - math.log(M.dense_marginal(P, mask[s], known[s], -1))) for s in range(n))
    print('dense l %d, %d rows: marginal %.2e completion %.2e class weights %.2e posterior %.2e log_prob_masked %.2e' % (l, n, e1, e0, ec, ep, ej))
    assert max(e1, e0, ec, ep, ej) <= LOGP_TOL_DENSE


# ---------------------------------------------------------------------------------------------------------------
# 2. ragged chains
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('row', S.ROWS, ids=lambda r: 'D%d_L%d' % r)
def test_ragged_chains_equal_the_reference(row):
    D, L = row
    ctx = G.new_ctx(17, D, L, 7)
    worst, n_ok, n_all = 0.0, 0, 0
    for ci, case in enumerate(S.draw_cases()):
        if (case[1], case[2]) != row:
            continue
        N, _, _, l, K = case
        cores, phi, w, classes, u = S.build_draw_case(case)
        mask, shared, known = M.ragged_inputs(ci, case)
        ctx.set_cores(A.as32(cores), l)
        for m in (mask, shared):
            k, err = compare(ctx.sample_masked(S.N_DRAWS, phi, w, m, known, classes, u), M.masked_walk(cores, l, phi, w, classes, u, m, known), m, known)
            assert k >= 0.95 * S.N_DRAWS, case
            worst, n_ok, n_all = max(worst, err), n_ok + k, n_all + S.N_DRAWS
    ctx.close()
    print('D %d L %d: %d of %d samples decidable and equal, |dlogp| %.2e' % (D, L, n_ok, n_all, worst))
    assert n_all == 2 * 17 * S.N_DRAWS and worst <= LOGP_TOL_DRAWS[row]


# ---------------------------------------------------------------------------------------------------------------
# 3. bonds 50 and 64: tiles of 2 and of 1
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', S.wide_cases(), ids=lambda c: 'bond%d' % c[4])
def test_bonds_50_and_64(case):
    N, D, L, l, Mb, K = case
    cores, phi, w, classes, u = S.build_wide_case(case)
    suffix, rnd, known = M.wide_inputs(case)
    ctx = G.new_ctx(N, D, L, Mb)
    ctx.set_cores(A.as32(cores), l)
    for m in (suffix, rnd):
        k, err = compare(ctx.sample_masked(S.N_DRAWS, phi, w, m, known, classes, u), M.masked_walk(cores, l, phi, w, classes, u, m, known), m, known)
        print('bond %d: %d of %d samples decidable and equal, |dlogp| %.2e' % (Mb, k, S.N_DRAWS, err))
        assert k >= 0.95 * S.N_DRAWS and err <= LOGP_TOL_WIDE
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------
# 4. against the existing sampler on the device
# ---------------------------------------------------------------------------------------------------------------
def test_prefix_and_empty_masks_against_the_existing_sampler():
    for ci, case in [(12, (17, 2, 2, 12, 7)), (20, (17, 3, 3, 3, 256)), (42, (17, 8, 10, 8, 2))]:
        N, D, L, l, K = case
        cores, phi, w, classes, u = S.build_draw_case(case)
        _, _, known = M.ragged_inputs(ci, case)
        ctx = G.new_ctx(N, D, L, 7)
        ctx.set_cores(A.as32(cores), l)
        prefix = np.arange(N) < N // 2
        given = np.ascontiguousarray(known[:, :N // 2])
        new = ctx.sample_masked(S.N_DRAWS, phi, w, prefix, known, classes, u)
        old = ctx.sample(S.N_DRAWS, phi, w, classes, given, u)
        ok = S.decidable(M.masked_walk(cores, l, phi, w, classes, u, prefix, known)[3]) & S.decidable(S.walk(cores, l, phi, w, classes, u, given)[3])
        assert ok.sum() >= 0.95 * S.N_DRAWS
        if l < N // 2:
            # a label drawn INSIDE the prefix: tnml_sample draws it given the levels before it only, the new call given every known
            # pixel -- two different distributions; the samples with a given class are the same in both
            ok &= classes >= 0
        assert np.array_equal(new[0][ok], old[0][ok]) and np.array_equal(new[1][ok], old[1][ok])
        empty = np.zeros(N, dtype=bool)
        new = ctx.sample_masked(S.N_DRAWS, phi, w, empty, None, classes, u)
        old = ctx.sample(S.N_DRAWS, phi, w, classes, None, u)
        ok = S.decidable(M.masked_walk(cores, l, phi, w, classes, u, empty, None)[3]) & S.decidable(S.walk(cores, l, phi, w, classes, u)[3])
        assert ok.sum() >= 0.95 * S.N_DRAWS
        assert np.array_equal(new[0][ok], old[0][ok]) and np.array_equal(new[1][ok], old[1][ok])
        assert np.all(new[2][:, 1] == 0.0)                                                             # exactly
        ctx.close()


# ---------------------------------------------------------------------------------------------------------------
# 5. the identity  logp0 + logp1 = log p(completed image)
# ---------------------------------------------------------------------------------------------------------------
def test_columns_add_up_to_the_likelihood_of_the_completed_image():
    worst = 0.0
    for ci, case in [(12, (17, 2, 2, 12, 7)), (20, (17, 3, 3, 3, 256)), (42, (17, 8, 10, 8, 2))]:
        N, D, L, l, K = case
        cores, phi, w, classes, u = S.build_draw_case(case)
        mask, _, known = M.ragged_inputs(ci, case)
        ctx = G.new_ctx(N, D, L, 7)
        ctx.set_cores(A.as32(cores), l)
        lev, lab, lp = ctx.sample_masked(S.N_DRAWS, phi, w, mask, known, classes, u)
        fixed = classes >= 0
        full = ctx.sample(S.N_DRAWS, phi, w, lab, lev, u)                                               # n_given = N, every class given
        ctx.close()
        worst = max(worst, float(np.abs((lp[fixed, 0] + lp[fixed, 1]) - full[2][fixed, 0]).max()))
        net = G.network_of(cores, l, 7, D, L)
        joint, _ = net.log_prob(lev[~fixed], classes=lab[~fixed], levels=K, weights=w, joint=True)
        worst = max(worst, float(np.abs((lp[~fixed, 0] + lp[~fixed, 1]) - joint).max()))
    print('identity: |logp0 + logp1 - log p| %.2e' % worst)
    assert worst <= LOGP_TOL_IDENT


# ---------------------------------------------------------------------------------------------------------------
# 6. independence of chunks, tiles, neighbours
# ---------------------------------------------------------------------------------------------------------------
def test_results_do_not_depend_on_chunks_order_or_neighbours():
    ci = 25
    case = S.draw_cases()[ci]
    N, D, L, l, K = case
    assert (D, L, l) == (3, 3, 8)
    cores, phi, w, classes, u = S.build_draw_case(case)
    mask, _, known = M.ragged_inputs(ci, case)
    n = S.N_DRAWS
    ctx = G.new_ctx(N, D, L, 7)
    ctx.set_cores(A.as32(cores), l)
    same = lambda a, b: all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    base = ctx.sample_masked(n, phi, w, mask, known, classes, u, class_logw=True)
    assert same(base, ctx.sample_masked(n, phi, w, mask, known, classes, u, class_logw=True))          # two identical calls
    # a stack budget of two tiles: 40 samples and the normalisers in tiles of 16 rows are at least 4 tiles, so at least 2 chunks of
    # 2; a budget of one tile: at least 4 chunks
    mb = max(c.shape[2] for c in cores)
    tile = 16 * (N + 1) * mb * mb * 8
    for budget in (2 * tile, tile):
        ctx.set_sample_stack_bytes(budget)
        assert same(base, ctx.sample_masked(n, phi, w, mask, known, classes, u, class_logw=True)), budget
    assert G._code(lambda: (ctx.set_sample_stack_bytes(tile - 8), ctx.sample_masked(n, phi, w, mask, known, classes, u))) == ARG
    ctx.set_sample_stack_bytes(1 << 30)
    # rows permuted
    perm = np.random.default_rng(6).permutation(n)
    got = ctx.sample_masked(n, phi, w, mask[perm], known[perm], classes[perm], u[perm])
    assert same([x[perm] for x in base[:3]], got)
    # one sample alone
    one = ctx.sample_masked(1, phi, w, mask[:1], known[:1], classes[:1], u[:1])
    assert same([x[:1] for x in base[:3]], one)
    # seeded
    for seed in (0, 12345, 2 ** 64 - 1):
        a = ctx.sample_masked(n, phi, w, mask, known, classes, None, seed)
        b = ctx.sample_masked(n, phi, w, mask, known, classes, S.hash_uniforms(seed, n, N))
        assert same(a, b), seed
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------
# 7. frequencies
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', M.FREQ_MASKED, ids=lambda c: 'N%d_K%d_l%d_known%s' % (c[0], c[1], c[4], ''.join(map(str, c[5]))))
def test_frequencies_against_the_dense_conditional(case):
    N, K, D, L, l, sites = case
    cores, phi, w = S.dense_case(D, L, N, K, l)
    P = S.dense_joint(cores, l, phi, w)
    mask = np.zeros(N, dtype=bool)
    mask[list(sites)] = True
    known = np.zeros((S.FREQ_N, N), dtype=np.int32)
    known[:, list(sites)] = [(1 + j) % K for j in range(len(sites))]
    cond = P * 0.0
    idx = tuple(int(known[0, i]) if mask[i] else slice(None) for i in range(N))
    cond[idx] = P[idx]
    cond = (cond / cond.sum()).ravel()
    ctx = G.new_ctx(N, D, L, 3)
    ctx.set_cores(A.as32(cores), l)
    lev, lab, _ = ctx.sample_masked(S.FREQ_N, phi, w, mask, known, None, None, S.FREQ_SEED)
    ctx.close()
    assert np.array_equal(lev[:, mask], known[:, mask])
    counts = S.outcome_counts(lev, lab, K, L)
    assert counts[cond == 0.0].sum() == 0
    keep = cond > 0.0
    chi2, dof = S.chi_square(counts[keep], cond[keep], S.FREQ_N)
    print('N %d K %d label on %d, sites %s known: chi2 %.1f at dof %d (bound %.1f)' % (N, K, l, sites, chi2, dof, S.chi_bound(dof)))
    assert dof >= 1 and chi2 <= S.chi_bound(dof)


# ---------------------------------------------------------------------------------------------------------------
# 8. long chain
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('which', [0, 1], ids=['calibrated', 'raw'])
@pytest.mark.parametrize('name', ['bottom', 'checker', 'random', 'empty'])
def test_long_chain(which, name):
    _, W, l = S.long_cases()[which]
    N, D, L, K = 784, 2, 2, 256
    _, phi, w = S.grid(K, D)
    masks, known = M.long_inputs()
    u = S.hash_uniforms(784, M.LONG_N, N)
    ctx = G.new_ctx(N, D, L, 20)
    ctx.set_cores(A.as32(W), l)
    dev = ctx.sample_masked(M.LONG_N, phi, w, masks[name], known, M.LONG_CLASSES, u)
    ctx.close()
    k, err = compare(dev, M.masked_walk(W, l, phi, w, M.LONG_CLASSES, u, masks[name], known), masks[name], known)
    print('N 784 %d %s: %d of %d samples decidable and equal, |dlogp| %.2e, logp about %.1f %.1f' % (which, name, k, M.LONG_N, err, dev[2][:, 0].mean(), dev[2][:, 1].mean()))
    assert k >= 0.95 * M.LONG_N and err <= LOGP_TOL_LONG and np.all(np.isfinite(dev[2]))


# ---------------------------------------------------------------------------------------------------------------
# 9. against the classifier
# ---------------------------------------------------------------------------------------------------------------
def test_classify_masked_with_a_full_mask_against_predict():
    """log P(c | x) - log P(c' | x) = 2 log|f_c(x) / f_c'(x)|: the new path against the float32 forward chain, which limits it"""
    case = (17, 2, 3, 8, 256)
    N, D, L, l, K = case
    cores, phi, w, _, _ = S.build_draw_case(case)
    net = G.network_of(cores, l, 7, D, L)
    X, _, _, lev = net.sample(24, levels=K, seed=3)
    f = net._sync_to_device(1).predict(gen.psi(X, D)).astype(np.float64)                              # (L, n)
    pred, log_post = net.classify_masked(lev, np.ones(N, dtype=bool), levels=K)
    worst, n, checked = 0.0, 0, 0
    for s in range(24):
        a = np.abs(f[:, s])
        use = [c for c in range(L) if a[c] >= 0.1 * a.max()]
        for c in use[1:]:
            worst = max(worst, abs((log_post[s, c] - log_post[s, use[0]]) - 2.0 * math.log(abs(f[c, s] / f[use[0], s]))))
            n += 1
        # the prediction wherever the two largest |f| are further apart than ten times the bound on the log difference (which
        # includes every sample whose second |f| fails the 0.1 filter)
        top = np.sort(a)[::-1]
        if 2.0 * math.log(top[0] / top[1]) > 10.0 * LOGP_TOL_PREDICT:
            assert pred[s] == a.argmax()
            checked += 1
    print('against predict: %d pairs, worst %.2e, %d predictions' % (n, worst, checked))
    assert n >= 12 and checked >= 12 and worst <= LOGP_TOL_PREDICT
    assert float(np.abs(np.exp(log_post).sum(axis=1) - 1.0).max()) <= 1e-12


# ---------------------------------------------------------------------------------------------------------------
# 10. state and refusals
# ---------------------------------------------------------------------------------------------------------------
def test_state_and_refusals(monkeypatch):
    ci, case = 0, (17, 2, 2, 0, 256)
    N, D, L, l, K = case
    assert S.draw_cases()[ci] == case
    cores, phi, w, classes, u = S.build_draw_case(case)
    mask, _, known = M.ragged_inputs(ci, case)
    n = S.N_DRAWS
    call = lambda c, **kw: c.sample_masked(n, kw.get('phi', phi), kw.get('w', w), kw.get('mask', mask), kw.get('known', known),
                                           kw.get('classes', classes), kw.get('u', u))
    ctx = G.new_ctx(N, D, L, 7, R.B)
    assert G._code(lambda: call(ctx)) == STATE                                                         # cores never set
    ctx.set_cores(A.as32(cores), l)
    X = R.features(np.random.default_rng(1), R.B, N, D)
    ctx.set_input(X, (np.arange(R.B) % L).astype(np.int32))
    f = ctx.forward()
    side = _hip.SIDE_RIGHT
    envs = [ctx.get_env(side, i).tobytes() for i in range(l + 1, N)]
    before = G.bits(ctx)
    old = ctx.sample(n, phi, w, classes, None, u)
    ref = M.masked_walk(cores, l, phi, w, classes, u, mask, known)
    k, err = compare(call(ctx), ref, mask, known)
    assert k >= 0.95 * n and err <= LOGP_TOL_DRAWS[(D, L)]
    # refusals, one code each
    import ctypes as C
    lib = _hip.lib()
    i32p, f64p, u8p = C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_uint8)
    m8 = np.ascontiguousarray(mask, dtype=np.uint8)
    lev, lab, lp = np.zeros((n, N), dtype=np.int32), np.zeros(n, dtype=np.int32), np.zeros((n, 2))
    pp, wp, cp, up, mp, kp = (phi.ctypes.data_as(f64p), w.ctypes.data_as(f64p), classes.ctypes.data_as(i32p), u.ctypes.data_as(f64p),
                              m8.ctypes.data_as(u8p), known.ctypes.data_as(i32p))
    lvp, lbp, lpp = lev.ctypes.data_as(i32p), lab.ctypes.data_as(i32p), lp.ctypes.data_as(f64p)
    bad_known, off_mask_known = known.copy(), known.copy()
    s_on, i_on = np.argwhere(mask)[0]
    s_off, i_off = np.argwhere(~mask)[0]
    bad_known[s_on, i_on], off_mask_known[s_off, i_off] = K, K + 5
    bad_cls, bad_w, bad_phi, bad_u = classes.copy(), w.copy(), phi.copy(), u.copy()
    bad_cls[5], bad_w[2], bad_phi[1, 0], bad_u[0, 0] = L, 0.0, np.inf, 1.0
    sm = lib.tnml_sample_masked
    codes = [sm(None, n, K, pp, wp, cp, mp, n, kp, up, 0, 1, lvp, lbp, lpp, None),
             sm(ctx._h, 0, K, pp, wp, cp, mp, n, kp, up, 0, 1, lvp, lbp, lpp, None),
             sm(ctx._h, n, 1, pp, wp, cp, mp, n, kp, up, 0, 1, lvp, lbp, lpp, None),
             sm(ctx._h, n, 257, pp, wp, cp, mp, n, kp, up, 0, 1, lvp, lbp, lpp, None),
             sm(ctx._h, n, K, pp, wp, cp, mp, 2, kp, up, 0, 1, lvp, lbp, lpp, None),                    # mask_rows neither 1 nor n
             sm(ctx._h, n, K, pp, wp, cp, None, n, kp, up, 0, 1, lvp, lbp, lpp, None),                  # NULL mask
             sm(ctx._h, n, K, pp, wp, cp, mp, n, None, up, 0, 1, lvp, lbp, lpp, None),                  # NULL known, bits set
             sm(ctx._h, n, K, pp, wp, cp, mp, n, bad_known.ctypes.data_as(i32p), up, 0, 1, lvp, lbp, lpp, None),
             sm(ctx._h, n, K, pp, wp, cp, mp, n, kp, up, 0, 1, None, lbp, lpp, None),                   # draw without levels_out
             sm(ctx._h, n, K, pp, wp, cp, mp, n, kp, up, 0, 1, lvp, None, lpp, None),
             sm(ctx._h, n, K, pp, wp, cp, mp, n, kp, up, 0, 0, None, None, None, None),
             sm(ctx._h, n, K, pp, wp, bad_cls.ctypes.data_as(i32p), mp, n, kp, up, 0, 1, lvp, lbp, lpp, None),
             sm(ctx._h, n, K, pp, bad_w.ctypes.data_as(f64p), cp, mp, n, kp, up, 0, 1, lvp, lbp, lpp, None),
             sm(ctx._h, n, K, bad_phi.ctypes.data_as(f64p), wp, cp, mp, n, kp, up, 0, 1, lvp, lbp, lpp, None),
             sm(ctx._h, n, K, pp, wp, cp, mp, n, kp, bad_u.ctypes.data_as(f64p), 0, 1, lvp, lbp, lpp, None),
             sm(ctx._h, n, K, None, wp, cp, mp, n, kp, up, 0, 1, lvp, lbp, lpp, None),
             lib.tnml_set_sample_stack_bytes(ctx._h, 0)]
    assert codes == [ARG] * 17, codes
    # a level outside the grid where the mask is NOT set is ignored; draw = 0 takes NULL levels and labels
    assert sm(ctx._h, n, K, pp, wp, cp, mp, n, off_mask_known.ctypes.data_as(i32p), up, 0, 1, lvp, lbp, lpp, None) == 0
    assert lev.tobytes() == call(ctx)[0].tobytes()
    assert sm(ctx._h, n, K, pp, wp, cp, mp, n, kp, up, 0, 0, None, None, lpp, None) == 0
    assert G.bits(ctx) == before and ctx.get_f().tobytes() == f.tobytes()
    assert [ctx.get_env(side, i).tobytes() for i in range(l + 1, N)] == envs
    again = ctx.sample(n, phi, w, classes, None, u)                                                   # the existing group still serves
    assert all(x.tobytes() == y.tobytes() for x, y in zip(old, again))
    ctx.sweep(False, 2, True, *G.SWEEP)                                                                # no new forward needed
    # known pixels of zero weight: phi_k = 0 at one level
    ctx.set_cores(A.as32(cores), l)
    zphi = phi.copy()
    zphi[3] = 0.0
    zk = known.copy()
    full = np.zeros((n, N), dtype=bool)
    full[7, 4], zk[7, 4] = True, 3
    full[9, 4], zk[9, 4] = True, 3
    with pytest.raises(_hip.TnmlError, match=r'sample 7 \(class %d\)' % classes[7]) as ei:
        ctx.sample_masked(n, zphi, w, full, zk, classes, u)
    assert ei.value.code == ARG
    # a NaN core
    nan = [c.copy() for c in cores]
    nan[9][0, 0, 0] = np.nan
    ctx.set_cores(A.as32(nan), l)
    assert G._code(lambda: call(ctx)) == NONFINITE
    ctx.set_cores(A.as32(cores), l)
    k, err = compare(call(ctx), ref, mask, known)                                                     # usable afterwards
    assert k >= 0.95 * n and err <= LOGP_TOL_DRAWS[(D, L)]
    ctx.close()
    # a bond the kernels have no room for
    ctx = _hip.Context(4, 2, 2, 128, 8)
    rng = np.random.default_rng(3)
    big = R.make_cores(4, 2, 2, [2, 128, 2], 0, rng, R.features(rng, 8, 4, 2))
    ctx.set_cores(A.as32(big), 0)
    before = G.bits(ctx)
    with pytest.raises(_hip.TnmlError, match='bytes of LDS') as ei:
        ctx.sample_masked(4, phi, w, np.zeros(4, dtype=bool), None)
    assert ei.value.code == SHAPE and G.bits(ctx) == before
    ctx.close()
    # a communicator attached
    from tensornetworkforml_amd import dist as tdist
    monkeypatch.setenv('TNML_FORCE_COMM', '1')
    ctx = _hip.Context(N, D, L, 7, 8)
    c0 = S.chain(N, D, L, [3] * (N - 1), 0, np.random.default_rng(2))
    ctx.set_cores(A.as32(c0), 0)
    tdist.attach_comm(ctx, 0, 1)
    assert G._code(lambda: ctx.sample_masked(4, phi, w, np.zeros(N, dtype=bool), None)) == STATE
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------
# 11. the scripts
# ---------------------------------------------------------------------------------------------------------------
def test_scripts_inpaint_and_classify_occluded_images(tmp_path, monkeypatch, capsys):
    from tensornetworkforml_amd import evaluate_diagonals as eval_script
    from tensornetworkforml_amd import training_diagonals as train_script
    monkeypatch.chdir(tmp_path)
    out, img = str(tmp_path / 'diag.dat'), str(tmp_path / 'img.npy')
    np.random.seed(4)
    train_script.main(['--n_samples', '400', '--linear_dim', '4', '--M', '4', '--n_epochs', '1', '--trunc', 'fixed', '--resident', '--out', out])
    capsys.readouterr()
    for which in ('bottom', 'checker'):
        np.random.seed(5)
        data, _ = gen.create_dataset(200, 4, 0.6)                                                     # the images the script draws
        np.random.seed(5)
        eval_script.main(['--filename', out, '--n_samples', '200', '--inpaint', img, '--inpaint-known', which, '--sample-n', '24', '--seed', '9'])
        lines = capsys.readouterr().out.splitlines()
        X = np.load(img)
        assert X.shape == (24, 4, 4) and np.all((X >= 0.0) & (X <= 1.0)) and np.array_equal(np.rint(X * 255) / 255, X)
        keep = eval_script.known_half(which, 4).reshape(4, 4)
        want = np.rint(np.clip(data[:24].reshape(24, 4, 4), 0.0, 1.0) * 255.0) / 255.0
        assert np.array_equal(X[:, keep], want[:, keep]) and keep.sum() == 8
        ln = [x for x in lines if 'Inpainted 24 images, %s known' % which in x]
        assert len(ln) == 1
        mean, share = float(ln[0].split('known) ')[1].split(',')[0]), float(ln[0].rsplit(' ', 1)[1])
        assert math.isfinite(mean) and mean < 0.0 and 0.0 <= share <= 1.0
    eval_script.main(['--filename', out, '--n_samples', '200', '--occluded', '0.3', '--seed', '2'])
    ln = [x for x in capsys.readouterr().out.splitlines() if 'Occluded 0.30 of the pixels of 200 images' in x]
    assert len(ln) == 1
    a, b = float(ln[0].split('summed out ')[1].split(',')[0]), float(ln[0].rsplit(' ', 1)[1])
    assert 0.0 <= a <= 1.0 and 0.0 <= b <= 1.0
