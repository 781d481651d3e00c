"""tnml_pair_marginals on the device against the NumPy statement of tests/pair_reference.py and against dense enumeration
(DESIGN.md section 28).  Every comparison is with the reference or the enumeration, never with the device's own output, except
where bit-equality between two device calls is the claim.  The bounds are pair_reference.BOUNDS: per class of case and per measure
ten times the larger of the reference's own float64-against-long-double difference and 2^-53 N m^2 D -- none of them comes from
the device.  The one-site outputs are held to the same bounds (q1 with q; mean and variance with the covariance; the entropy with
the mutual information).  Every test prints its figures before it asserts."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p_ in (ROOT, HERE):
    if p_ not in sys.path:
        sys.path.insert(0, p_)

import context_lifecycle_cases as lc                               # noqa: E402
import mps_algebra_reference as A                                  # noqa: E402
import orthogonalize_reference as R                                # noqa: E402
import pair_reference as P                                         # noqa: E402
import sample_reference as S                                       # noqa: E402
import test_sample_gpu as G                                        # noqa: E402  (its helpers: new_ctx, network_of, bits, _code)
from tensornetworkforml_amd import _hip                            # noqa: E402

pytestmark = pytest.mark.gpu

ARG, STATE, SHAPE = -1, -2, -6
OUTPUTS = ('q1', 'stats1', 'q', 'stats')


def device(ctx, args, **kw):
    """one device call on the arguments of pair_reference.pair_marginals -> the reference's dict"""
    cores, l, phi, w, values, q, rows = args
    rows = np.arange(len(cores)) if rows is None else np.asarray(rows)
    return dict(zip(OUTPUTS, ctx.pair_marginals(phi, w, rows, q, values, **kw)))


def rows_of(args):
    return list(range(len(args[0]))) if args[6] is None else list(args[6])


def check(dev, ref, args, cls, tag):
    """the device against the reference in the measures of the bounds; zeros where a row covers no pair; -> the figures"""
    rows = rows_of(args)
    d = P.differences(dev, ref, rows, args[4])
    print('%s: %s' % (tag, ' '.join('%s %.2e (%.0e)' % (k, d[k], P.BOUNDS[cls][k]) for k in P.MEASURES)))
    out = ~P.pairs_of(rows, len(args[0]))
    assert not dev['q'][out].any() and not dev['stats'][out].any()
    assert np.all(np.isfinite(dev['q'])) and np.all(np.isfinite(dev['stats'])) and np.all(np.isfinite(dev['stats1']))
    for k in P.MEASURES:
        assert d[k] <= P.BOUNDS[cls][k], (tag, k, d[k])
    return d


def same(a, b, keys=OUTPUTS):
    return all(a[k].tobytes() == b[k].tobytes() for k in keys)


# ---------------------------------------------------------------------------------------------------------------
# 1. dense enumeration: the label on both ends and inside, summed and every class, 4 and 256 levels
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K', P.DENSE_K)
@pytest.mark.parametrize('l', P.DENSE_L)
def test_dense_enumeration(l, K):
    """every output against the whole tensor closed with S (pair_reference.dense_features) and against the reference"""
    N, D, L = 4, 2, 3
    ctx = G.new_ctx(N, D, L, 3)
    calls = [(i, c) for i, c in enumerate(P.class_calls('dense')) if c[0][1] == l and len(c[0][3]) == K]
    assert len(calls) == 4
    for index, (args, _) in calls:
        cores, _, phi, w, values, q, _ = args
        ctx.set_cores(A.as32(cores), l)
        dev = device(ctx, args)
        check(dev, P.reference('dense', index), args, 'dense', 'dense l %d K %d class %d' % (l, K, q))
        check(dev, P.dense_features(cores, l, phi, w, values, q), args, 'dense', '  against the enumeration')
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------
# 2. ragged 17-site chains at every label position: the label site as i, as j and in between; -1 and the classes in turn
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('row', S.ROWS, ids=lambda r: 'D%d_L%d' % r)
def test_ragged_chains(row):
    D, L = row
    cls = ('ragged', row)
    ctx = G.new_ctx(17, D, L, 7)
    worst = {}
    calls = P.class_calls(cls)
    assert sorted(c[0][1] for c in calls) == list(range(17)) and {c[0][5] for c in calls} == set(range(-1, L))
    for index, (args, _) in enumerate(calls):
        ctx.set_cores(A.as32(args[0]), args[1])
        worst = P.worse(worst, check(device(ctx, args), P.reference(cls, index), args, cls, 'D %d label on %d class %d K %d' % (
            D, args[1], args[5], len(args[3]))))
    ctx.close()
    print('D %d L %d, %d calls: %s' % (D, L, len(calls), worst))


# ---------------------------------------------------------------------------------------------------------------
# 3. bonds 50 (L = 10) and 64: the LDS edge
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('wi', [0, 1], ids=['bond50', 'bond64'])
def test_wide_bonds(wi):
    N, D, L, l, Mb, K = S.wide_cases()[wi]
    ctx = G.new_ctx(N, D, L, Mb)
    for index in (2 * wi, 2 * wi + 1):
        args, _ = P.class_calls('wide')[index]
        ctx.set_cores(A.as32(args[0]), l)
        check(device(ctx, args), P.reference('wide', index), args, 'wide', 'bond %d class %d' % (Mb, args[5]))
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------
# 4. N = 784, not calibrated: the exponents run through their whole range
# ---------------------------------------------------------------------------------------------------------------
def test_long_chain():
    args, _ = P.class_calls('long')[0]
    assert set(args[6]) == {0, 391, args[1], 782}
    ctx = G.new_ctx(784, 2, 2, 20)
    ctx.set_cores(A.as32(args[0]), args[1])
    dev = device(ctx, args)
    ctx.close()
    check(dev, P.reference('long', 0), args, 'long', 'N 784 rows %s' % (args[6],))


# ---------------------------------------------------------------------------------------------------------------
# 5. bit-equality: repetition, order, neighbours, chunks, outputs, and the maps of Network
# ---------------------------------------------------------------------------------------------------------------
def test_results_do_not_depend_on_repetition_order_neighbours_chunks_or_outputs():
    ci = 25
    N, D, L, l, K = S.draw_cases()[ci]
    assert (D, L, l) == (3, 3, 8)
    args = P.ragged_inputs(ci) + (1, None)
    ctx = G.new_ctx(N, D, L, 7)
    ctx.set_cores(A.as32(args[0]), l)
    base = device(ctx, args)
    assert same(base, device(ctx, args))                                                              # a repeated call
    perm = np.random.default_rng(6).permutation(N)                                                    # rows permuted
    got = device(ctx, args[:6] + (perm,))
    assert same(base, dict(got, q=got['q'][np.argsort(perm)], stats=got['stats'][np.argsort(perm)]))
    for i in (0, l, N - 2, N - 1):                                                                    # one row alone
        one = device(ctx, args[:6] + ([i],))
        assert same(base, dict(one, q=np.concatenate([base['q'][:i], one['q'], base['q'][i + 1:]]),
                               stats=np.concatenate([base['stats'][:i], one['stats'], base['stats'][i + 1:]]))), i
    none = device(ctx, args[:6] + ([],))                                                              # n_rows = 0: the per-site part alone
    assert same(base, none, ('q1', 'stats1')) and none['q'].shape == (0, N, D * D, D * D)
    row_bytes = N * (D ** 4 * 8 + D * D * 4 + 3 * 8)                                                  # a budget of one row and of three
    for budget in (row_bytes, 3 * row_bytes + 7):
        ctx.set_sample_stack_bytes(budget)
        assert same(base, device(ctx, args)), budget
    assert G._code(lambda: (ctx.set_sample_stack_bytes(row_bytes - 1), device(ctx, args))) == ARG
    ctx.set_sample_stack_bytes(1 << 30)
    for k in range(1, 16):                                                                            # every subset of the outputs
        want = tuple(name for b, name in enumerate(OUTPUTS) if k >> b & 1)
        got = device(ctx, args, want=want)
        assert all((got[name] is None) != (name in want) for name in OUTPUTS) and same(base, got, want), want
    ctx.close()
    # the maps of Network are assembled from stats_out and stats1_out as they are
    net = G.network_of(args[0], l, 7, D, L)
    x, w = args[4], args[3]
    mi = net.mutual_information(classes=1, levels=K, weights=w)
    cov, corr, mean, std = net.pixel_correlations(classes=1, levels=K, weights=w)
    iu = np.triu_indices(N, 1)
    assert np.array_equal(mi, mi.T) and np.array_equal(cov, cov.T) and np.array_equal(corr, corr.T)
    assert mi[iu].tobytes() == base['stats'][..., 2][iu].tobytes() and np.diag(mi).tobytes() == base['stats1'][:, 2].tobytes()
    assert cov[iu].tobytes() == base['stats'][..., 0][iu].tobytes() and np.diag(cov).tobytes() == base['stats1'][:, 1].tobytes()
    assert corr[iu].tobytes() == base['stats'][..., 1][iu].tobytes() and np.all(np.diag(corr) == 1.0)
    assert mean.tobytes() == base['stats1'][:, 0].tobytes() and np.array_equal(std, np.sqrt(base['stats1'][:, 1]))
    q6, q1 = net.pixel_pair_marginals(rows=[3, 0], classes=1, levels=K, weights=w)
    assert q6.shape == (2, N, D, D, D, D) and q6.tobytes() == base['q'][[3, 0]].tobytes() and q1.tobytes() == base['q1'].tobytes()
    ref = P.pair_marginals(*args)
    tab = net.pair_probs(q6[0, 5], levels=K, weights=w)
    assert float(np.abs(tab - P.pair_table(ref['q'][3, 5], args[2], w)).max()) <= D * D * P.BOUNDS[('ragged', (D, L))]['q'] * float(np.abs(ref['q'][3, 5]).max())
    # I(x_i; l) against the reference's
    info = net.pixel_label_information(levels=K, weights=w)
    want = P.label_information(args[0], l, args[2], w)
    print('pixel_label_information: worst difference %.2e' % float(np.abs(info - want).max()))
    assert info.shape == (N,) and float(np.abs(info - want).max()) <= 2 * P.BOUNDS[('ragged', (D, L))]['mi']


# ---------------------------------------------------------------------------------------------------------------
# 6. nothing else moves, and nothing that moved before matters
# ---------------------------------------------------------------------------------------------------------------
def test_after_every_state_change_the_call_equals_a_fresh_context_and_changes_nothing():
    pr = lc.problem('A')
    live = lc.Live(_hip.Context(pr['N'], pr['D'], pr['L'], pr['M'], pr['capacity']), pr)
    lc.start(live)
    rng = np.random.default_rng(11)
    x = np.arange(len(pr['w']), dtype=np.float64)
    call = lambda ctx, q: dict(zip(OUTPUTS, ctx.pair_marginals(pr['phi'], pr['w'], np.arange(pr['N']), q, x)))
    for name in ('sweep_right', 'gd_step_adam', 'compress_to_3', 'axpby'):
        if name == 'gd_step_adam':
            live.ctx.optim_reset()                                                                    # (the sweep moved the label)
        lc.MUTATORS[name][0](live, rng)
        cores, _, lp = live.ctx.get_cores()
        before = G.bits(live.ctx)
        fresh = _hip.Context(pr['N'], pr['D'], pr['L'], pr['M'], pr['capacity'])
        fresh.set_any_position(True)
        fresh.set_cores(cores, lp)
        for q in (-1, 1):
            assert same(call(live.ctx, q), call(fresh, q)), (name, q)
        fresh.close()
        assert G.bits(live.ctx) == before, name
    # forward's f is what it was, with no forward in between needed for the next call
    f0 = live.ctx.forward(want_f=True)
    call(live.ctx, -1)
    f1 = live.ctx.forward(want_f=True)
    assert np.asarray(f0).tobytes() == np.asarray(f1).tobytes()
    live.ctx.close()


# ---------------------------------------------------------------------------------------------------------------
# 7. the refusals on the device
# ---------------------------------------------------------------------------------------------------------------
def test_refusals(monkeypatch):
    ci = 0
    N, D, L, l, K = S.draw_cases()[ci]
    cls = ('ragged', (D, L))
    args = P.ragged_inputs(ci) + (P.ragged_slot(ci), None)
    cores, _, phi, w, x, q, _ = args
    ctx = G.new_ctx(N, D, L, 7, R.B)
    assert G._code(lambda: device(ctx, args)) == STATE                                                # cores never set
    ctx.set_cores(A.as32(cores), l)
    before = G.bits(ctx)
    check(device(ctx, args), P.reference(cls, 0), args, cls, 'before the refusals')
    bad = x.copy()
    bad[1] = np.inf
    assert G._code(lambda: device(ctx, args[:4] + (bad,) + args[5:])) == ARG                          # a value that is not finite
    badphi = phi.copy()
    badphi[0, 0] = np.nan
    assert G._code(lambda: device(ctx, args[:2] + (badphi,) + args[3:])) == ARG                       # the grid
    assert G._code(lambda: device(ctx, args[:3] + (-w,) + args[4:])) == ARG                           # the weights
    for bad_q in (-2, L):
        assert G._code(lambda: device(ctx, args[:5] + (bad_q, None))) == ARG                          # the class slot
    for rows in ([0, N], [-1], [3, 5, 3]):
        assert G._code(lambda: device(ctx, args[:6] + (rows,))) == ARG                                # a row out of range or repeated
    assert G._code(lambda: device(ctx, args, want=())) == ARG                                         # every output NULL
    assert G._code(lambda: device(ctx, args[:6] + ([],), want=('q', 'stats'))) == ARG                 # ... or without a row
    assert G.bits(ctx) == before
    check(device(ctx, args), P.reference(cls, 0), args, cls, 'after the refusals')
    ctx.close()
    # a bond above the limit
    lim = _hip.PAIR_MAX_BOND
    ctx = _hip.Context(4, 2, 2, 128, 8)
    rng = np.random.default_rng(3)
    big = R.make_cores(4, 2, 2, [2, lim + 1, 2], 0, rng, R.features(rng, 8, 4, 2))
    ctx.set_cores(A.as32(big), 0)
    with pytest.raises(_hip.TnmlError, match='bytes of LDS') as ei:
        ctx.pair_marginals(phi, w, [0])
    assert ei.value.code == SHAPE
    ctx.close()
    # a communicator attached
    from tensornetworkforml_amd import dist as tdist
    monkeypatch.setenv('TNML_FORCE_COMM', '1')
    ctx = _hip.Context(N, D, L, 7, 8)
    ctx.set_cores(A.as32(S.chain(N, D, L, [3] * (N - 1), 0, np.random.default_rng(2))), 0)
    tdist.attach_comm(ctx, 0, 1)
    assert G._code(lambda: ctx.pair_marginals(phi, w, [0])) == STATE
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------
# 8. the script
# ---------------------------------------------------------------------------------------------------------------
def test_script_writes_the_mutual_information_map(tmp_path, monkeypatch, capsys):
    from tensornetworkforml_amd import evaluate_diagonals as eval_script
    from tensornetworkforml_amd import training_diagonals as train_script
    monkeypatch.chdir(tmp_path)
    out, path = str(tmp_path / 'diag.dat'), str(tmp_path / 'mi.npy')
    np.random.seed(4)
    train_script.main(['--n_samples', '400', '--linear_dim', '4', '--M', '4', '--n_epochs', '1', '--trunc', 'fixed', '--resident', '--out', out])
    capsys.readouterr()
    np.random.seed(5)
    eval_script.main(['--filename', out, '--n_samples', '200', '--mutual-info', path])
    lines = capsys.readouterr().out.splitlines()
    mi = np.load(path)
    assert mi.shape == (16, 16) and np.array_equal(mi, mi.T) and np.all(np.isfinite(mi)) and np.all(mi > -1e-12) and np.all(np.diag(mi) > 0.0)
    by_dist = [x for x in lines if 'Mutual information at distance' in x]
    assert [int(x.split('distance')[1].split(':')[0]) for x in by_dist] == [1, 2, 4, 8]
    for x in by_dist:
        dist = int(x.split('distance')[1].split(':')[0])
        assert abs(float(x.split('mean ')[1].split(' ')[0]) - float(np.diagonal(mi, dist).mean())) <= 1e-3 * abs(float(np.diagonal(mi, dist).mean())) + 1e-12
    top = [x for x in lines if 'Sites of largest I(x_i; l)' in x]
    assert len(top) == 1 and top[0].count('(') == 11
