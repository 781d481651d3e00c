"""tnml_site_conditionals on the device against the NumPy statement of tests/site_cond_reference.py and against dense enumeration
(DESIGN.md section 26).  Every comparison is with the reference or the enumeration, never with the device's own output, except
where bit-equality between two device calls is the claim.  The bounds are site_cond_reference.BOUNDS: per class of case and per
measure ten times the larger of the reference's own float64-against-long-double difference and 2^-53 N m^2 D -- none of them comes
from the device.  Modes are compared on the (sample, site) pairs the reference calls decidable (tests/test_site_cond_host.py
asserts that these are at least 95 % of every case).  Every test prints its figures before it asserts."""
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
import site_cond_reference as C                                    # noqa: E402
import test_sample_gpu as G                                        # noqa: E402  (its helpers: new_ctx, network_of, bits, _code)
from tensornetworkforml_amd import _hip                            # noqa: E402

pytestmark = pytest.mark.gpu

ARG, STATE, SHAPE = -1, -2, -6


def device(ctx, args, **kw):
    """one device call on the arguments of site_cond_reference.conditionals -> the reference's dict"""
    cores, l, phi, w, values, classes, mask, known = args
    q, stats, mode, logp = ctx.site_conditionals(len(classes), phi, w, mask, known, classes, values, **kw)
    return {'q': q, 'stats': stats, 'mode': mode, 'logp': logp}


def check(dev, ref, values, cls, tag):
    """the device against the reference in the measures of the bounds; modes equal on every decidable pair; -> the figures"""
    d = C.differences(dev, ref, values)
    ok = C.decidable_modes(ref['p'])
    print('%s: %s | %d of %d modes decidable' % (tag, ' '.join('%s %.2e (%.0e)' % (k, d[k], C.BOUNDS[cls][k]) for k in C.MEASURES), ok.sum(), ok.size))
    assert np.array_equal(dev['mode'][ok], ref['mode'][ok]), 'a decidable mode differs'
    assert ok.sum() >= 0.95 * ok.size
    inf = ~np.isfinite(ref['stats'][..., 3])
    assert np.array_equal(dev['stats'][..., 3][inf], ref['stats'][..., 3][inf])
    for k in C.MEASURES:
        assert d[k] <= C.BOUNDS[cls][k], (tag, k, d[k])
    return d


def same(a, b):
    return all(a[k].tobytes() == b[k].tobytes() for k in ('q', 'stats', 'mode', 'logp'))


# ---------------------------------------------------------------------------------------------------------------
# 1. dense enumeration: known and free label sites, both chain ends, the empty and the full mask
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('l', C.DENSE_L)
def test_dense_enumeration(l):
    """The table through Network.pixel_probs and the four statistics against the enumeration of sample_reference.dense_joint.  A
    density is w_k phi_k^T q phi_k with |phi_k| = 1 and w_k <= 1, so its error is at most D max|dq|: the table's bound is D times
    the bound of q times max|q| of the site."""
    args = C.dense_inputs(l)
    cores, _, phi, w, values, classes, mask, known = args
    N, D, L, K = 4, 2, 2, 3
    P = S.dense_joint(cores, l, phi, w)
    ctx = G.new_ctx(N, D, L, 3)
    ctx.set_cores(A.as32(cores), l)
    dev = device(ctx, args)
    ctx.close()
    check(dev, C.reference('dense', l, None), values, 'dense', 'dense l %d' % l)
    n = len(classes)
    table = np.array([[C.dense_conditional(P, mask[s], known[s], classes[s], i) for i in range(N)] for s in range(n)])
    net = G.network_of(cores, l, 4, D, L)
    p = net.pixel_probs(dev['q'], levels=K, weights=w)
    scale = np.abs(dev['q']).max(axis=(-1, -2))
    ep = float((np.abs(p - table).max(-1) / scale).max())
    enum = dict(C.statistics(table, values, mask, known), q=dev['q'])
    d = C.differences(dev, enum, values)
    print('dense l %d against the enumeration: table %.2e (%.0e) %s' % (l, ep, D * C.BOUNDS['dense']['q'], d))
    assert ep <= D * C.BOUNDS['dense']['q']
    assert np.array_equal(dev['mode'][C.decidable_modes(table)], enum['mode'][C.decidable_modes(table)])
    for k in ('mean', 'var', 'entropy', 'logp_known'):
        assert d[k] <= C.BOUNDS['dense'][k], (k, d[k])


# ---------------------------------------------------------------------------------------------------------------
# 2. ragged chains, 40 samples (not a multiple of a tile), known levels drawn from the model and random
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', C.LEVEL_KINDS)
@pytest.mark.parametrize('row', S.ROWS, ids=lambda r: 'D%d_L%d' % r)
def test_ragged_chains(row, kind):
    D, L = row
    cls = ('ragged', row, kind)
    ctx = G.new_ctx(17, D, L, 7)
    worst, calls = {}, 0
    for ci, case in C.ragged_cases(row):
        a = C.ragged_inputs(ci, kind)
        ctx.set_cores(A.as32(a[0]), a[1])
        for which, m in (('own', a[6]), ('shared', a[7])):
            dev = device(ctx, a[:6] + (m, a[8]))
            worst = C.worse(worst, check(dev, C.reference('ragged', (ci, kind), which), a[4], cls, 'case %d %s %s' % (ci, kind, which)))
            calls += 1
    ctx.close()
    print('D %d L %d %s levels, %d calls: %s' % (D, L, kind, calls, worst))
    assert calls == 2 * len(C.RAGGED_POSITIONS[row])


# ---------------------------------------------------------------------------------------------------------------
# 3. bonds 50 (L = 10) and 64: small tiles, the core taken sixteen rows at a time
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('wi', [0, 1], ids=['bond50', 'bond64'])
def test_wide_bonds(wi):
    N, D, L, l, Mb, K = S.wide_cases()[wi]
    a = C.wide_inputs(wi)
    ctx = G.new_ctx(N, D, L, Mb)
    ctx.set_cores(A.as32(a[0]), l)
    for which, m in (('suffix', a[6]), ('random', a[7])):
        check(device(ctx, a[:6] + (m, a[8])), C.reference('wide', wi, which), a[4], 'wide', 'bond %d %s' % (Mb, which))
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------
# 4. N = 784
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('which', [0, 1], ids=['calibrated', 'raw'])
@pytest.mark.parametrize('name', ['bottom', 'checker', 'random', 'empty', 'full'])
def test_long_chain(which, name):
    a = C.long_inputs(which)
    ctx = G.new_ctx(784, 2, 2, 20)
    ctx.set_cores(A.as32(a[0]), a[1])
    dev = device(ctx, a[:6] + (a[6][name], a[7]))
    if name == 'bottom':
        # logp_out is column 1 of the sampler's draw = 0 call, bit for bit, although that call's tile is 16 rows at bond 20 and this one's 8
        _, _, lp = ctx.sample_masked(len(a[5]), a[2], a[3], a[6][name], a[7], a[5], draw=False)
        assert dev['logp'].tobytes() == np.ascontiguousarray(lp[:, 1]).tobytes()
    ctx.close()
    check(dev, C.reference('long', which, name), a[4], 'long', 'N 784 %d %s' % (which, name))
    assert np.all(np.isfinite(dev['q'])) and np.all(np.isfinite(dev['logp']))


# ---------------------------------------------------------------------------------------------------------------
# 5. logp_out, NULL outputs, independence of chunks, tiles, order and neighbours
# ---------------------------------------------------------------------------------------------------------------
def test_logp_equals_the_sampler_and_results_do_not_depend_on_chunks_order_or_neighbours():
    ci = 25
    case = S.draw_cases()[ci]
    N, D, L, l, K = case
    assert (D, L, l) == (3, 3, 8)
    a = C.ragged_inputs(ci, 'drawn')
    cores, _, phi, w, values, classes, mask, shared, known = a
    n = S.N_DRAWS
    args = a[:6] + (mask, known)
    ctx = G.new_ctx(N, D, L, 7)
    ctx.set_cores(A.as32(cores), l)
    base = device(ctx, args)
    assert same(base, device(ctx, args))                                                              # a repeated call
    # logp_out is column 1 of the sampler's draw = 0 call, bit for bit (test_long_chain repeats this where the two tiles differ)
    _, _, lp = ctx.sample_masked(n, phi, w, mask, known, classes, draw=False)
    assert base['logp'].tobytes() == np.ascontiguousarray(lp[:, 1]).tobytes()
    # every output NULL in turn, and alone
    for k in ('q', 'stats', 'mode', 'logp'):
        rest = device(ctx, args, want=tuple(x for x in ('q', 'stats', 'mode', 'logp') if x != k))
        assert rest[k] is None and all(rest[x].tobytes() == base[x].tobytes() for x in rest if x != k), k
        alone = device(ctx, args, want=(k,))
        assert alone[k].tobytes() == base[k].tobytes() and all(alone[x] is None for x in alone if x != k), k
    # a stack budget of two tiles and of one: 40 samples and the normalisers are at least 4 tiles of at most 16 rows
    T = 16
    while T > 1 and not _fits(7, D, L, K, T):
        T //= 2
    tile = T * (N + 1) * 7 * 7 * 8
    for budget in (2 * tile, tile):
        ctx.set_sample_stack_bytes(budget)
        assert same(base, device(ctx, args)), budget
    assert G._code(lambda: (ctx.set_sample_stack_bytes(tile - 8), device(ctx, args))) == ARG
    ctx.set_sample_stack_bytes(1 << 30)
    # rows permuted
    perm = np.random.default_rng(6).permutation(n)
    got = device(ctx, a[:5] + (classes[perm], mask[perm], known[perm]))
    assert same({k: v[perm] for k, v in base.items()}, got)
    # one sample alone
    one = device(ctx, a[:5] + (classes[:1], mask[:1], known[:1]))
    assert same({k: v[:1] for k, v in base.items()}, one)
    # mask_rows 1 against the same mask repeated n times
    assert same(device(ctx, a[:6] + (shared, known)), device(ctx, a[:6] + (np.tile(shared, (n, 1)), known)))
    ctx.close()


def _fits(m, D, L, K, T):
    """the tile rule of DESIGN.md section 26 in bytes: both kernels of the call within 160 KB of LDS"""
    ev = lambda x: (x + 1) // 2 * 2
    env = (T * m * m + T * m * D * m + T * D * D) * 8 + 2 * T * 4 + ev(m * D * m) * 4
    ra = min(m, 16)
    new = (2 * T * m * m + 2 * T * ra * D * m + 2 * T * D * D + D * D + K * (D + 2)) * 8 + ev(T) * 4 + ev(m * D * m) * 4
    return max(env, new) <= 160 * 1024


# ---------------------------------------------------------------------------------------------------------------
# 6. through Network
# ---------------------------------------------------------------------------------------------------------------
def test_through_network():
    ci = 25
    case = S.draw_cases()[ci]
    N, D, L, l, K = case
    assert (D, L, l, K) == (3, 3, 8, 256)
    a = C.ragged_inputs(ci, 'drawn')
    cores, _, phi, w, x, classes, mask, shared, known = a
    net = G.network_of(cores, l, 7, D, L)
    cls = ('ragged', (D, L), 'drawn')
    # pixel_conditionals at D = 3, in pixel values
    ref = C.reference('ragged', (ci, 'drawn'), 'own')
    mean, std, mode, ent, lk, Q = net.pixel_conditionals(x[known], mask, classes, levels=K, weights=w)
    dev = {'q': Q, 'stats': np.stack([mean, std ** 2, ent, lk], -1)}
    d = C.differences(dev, ref, x)
    print('pixel_conditionals: %s' % d)
    ok = C.decidable_modes(ref['p'])
    assert np.array_equal(mode[ok], x[ref['mode']][ok])
    # (std ** 2 squares a square root: two more roundings of a number below range^2 / 4)
    assert all(d[k] <= C.BOUNDS[cls][k] + (4 * 2.0 ** -53 if k == 'var' else 0.0) for k in C.MEASURES), d
    p = net.pixel_probs(Q, levels=K, weights=w)
    assert float(np.abs(p - ref['p']).max()) <= D * C.BOUNDS[cls]['q'] * float(np.abs(ref['q']).max())
    # expected_image: known pixels unchanged with std 0, hidden ones the posterior mean
    img, sd = net.expected_image(x[known], mask, classes, levels=K, weights=w)
    assert np.array_equal(img[mask], x[known][mask]) and np.all(sd[mask] == 0.0)
    assert np.array_equal(img[~mask], mean[~mask]) and np.array_equal(sd[~mask], std[~mask]) and np.all(sd[~mask] > 0.0)
    # pixel_surprise sums to minus the log pseudo-likelihood of the reference
    full = C.conditionals(cores, l, phi, w, x, classes, np.ones(N, dtype=bool), known)
    sur = net.pixel_surprise(known, classes, levels=K, weights=w)
    err = float(np.abs(sur.sum(1) + full['stats'][..., 3].sum(1)).max())
    print('pixel_surprise: |sum + log pseudo-likelihood| %.2e' % err)
    assert sur.shape == (S.N_DRAWS, N) and np.all(sur > 0.0) and err <= N * C.BOUNDS[cls]['logp_known']


# ---------------------------------------------------------------------------------------------------------------
# 7. the refusals on the device
# ---------------------------------------------------------------------------------------------------------------
def test_refusals(monkeypatch):
    ci, case = 0, (17, 2, 2, 0, 256)
    N, D, L, l, K = case
    a = C.ragged_inputs(ci, 'drawn')
    cores, _, phi, w, x, classes, mask, shared, known = a
    args = a[:6] + (mask, known)
    ctx = G.new_ctx(N, D, L, 7, R.B)
    assert G._code(lambda: device(ctx, args)) == STATE                                                # cores never set
    ctx.set_cores(A.as32(cores), l)
    before = G.bits(ctx)
    check(device(ctx, args), C.reference('ragged', (ci, 'drawn'), 'own'), x, ('ragged', (D, L), 'drawn'), 'before the refusals')
    bad = x.copy()
    bad[3] = np.inf
    assert G._code(lambda: device(ctx, a[:4] + (bad,) + a[5:6] + (mask, known))) == ARG               # a value that is not finite
    assert G._code(lambda: device(ctx, args, want=())) == ARG                                         # every output NULL
    bad_known = known.copy()
    bad_known[tuple(np.argwhere(mask)[0])] = K
    assert G._code(lambda: device(ctx, a[:6] + (mask, bad_known))) == ARG                             # the sampler's own refusals
    assert G.bits(ctx) == before
    ctx.close()
    # a bond above the limit
    lim = _hip.SITE_COND_MAX_BOND
    ctx = _hip.Context(4, 2, 2, 128, 8)
    rng = np.random.default_rng(3)
    big = R.make_cores(4, 2, 2, [2, lim + 1, 2], 0, rng, R.features(rng, 8, 4, 2))
    ctx.set_cores(A.as32(big), 0)
    with pytest.raises(_hip.TnmlError, match='bytes of LDS') as ei:
        ctx.site_conditionals(4, phi, w, np.zeros(4, dtype=bool), None)
    assert ei.value.code == SHAPE
    ctx.close()
    # a communicator attached
    from tensornetworkforml_amd import dist as tdist
    monkeypatch.setenv('TNML_FORCE_COMM', '1')
    ctx = _hip.Context(N, D, L, 7, 8)
    ctx.set_cores(A.as32(S.chain(N, D, L, [3] * (N - 1), 0, np.random.default_rng(2))), 0)
    tdist.attach_comm(ctx, 0, 1)
    assert G._code(lambda: ctx.site_conditionals(4, phi, w, np.zeros(N, dtype=bool), None)) == STATE
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------
# 8. the scripts
# ---------------------------------------------------------------------------------------------------------------
def _check_script_output(lines, mean_file, sur_file, lev, keep, n, side):
    img, sur = np.load(mean_file), np.load(sur_file)
    want = lev[:n].reshape(n, side, side) / 255.0
    assert img.shape == (n, side, side) and np.array_equal(img[:, keep], want[:, keep]) and np.all((img >= 0.0) & (img <= 1.0))
    assert sur.shape == (n, side, side) and np.all(np.isfinite(sur)) and np.all(sur >= 0.0)
    ln = [x for x in lines if 'Posterior mean of %d images' % n in x]
    assert len(ln) == 1
    e_mean, e_draw = float(ln[0].split('hidden pixels ')[1].split(',')[0]), float(ln[0].split('drawn completion ')[1].split(',')[0])
    assert abs(e_mean - float(np.abs(img[:, ~keep] - want[:, ~keep]).mean())) <= 1e-4 and 0.0 <= e_draw <= 1.0
    ln = [x for x in lines if 'Surprise maps of %d images' % n in x]
    assert len(ln) == 1 and abs(float(ln[0].split('likelihood ')[1].split(' ')[0]) - float(sur.reshape(n, -1).sum(1).mean())) <= 1e-3


def test_scripts_write_posterior_means_and_surprise_maps(tmp_path, monkeypatch, capsys):
    from tensornetworkforml_amd import data_generator as gen
    from tensornetworkforml_amd import evaluate_binary_MNIST as eval_mnist
    from tensornetworkforml_amd import evaluate_diagonals as eval_script
    from tensornetworkforml_amd import training_binary_MNIST as train_mnist
    from tensornetworkforml_amd import training_diagonals as train_script
    from test_network_gpu import _synthetic_mnist
    monkeypatch.chdir(tmp_path)
    out, img, sur = str(tmp_path / 'diag.dat'), str(tmp_path / 'mean.npy'), str(tmp_path / 'surprise.npy')
    np.random.seed(4)
    train_script.main(['--n_samples', '400', '--linear_dim', '4', '--M', '4', '--n_epochs', '1', '--trunc', 'fixed', '--resident', '--out', out])
    capsys.readouterr()
    np.random.seed(5)
    data, _ = gen.create_dataset(200, 4, 0.6)                                                         # the images the script draws
    np.random.seed(5)
    eval_script.main(['--filename', out, '--n_samples', '200', '--inpaint-mean', img, '--inpaint-known', 'checker', '--surprise', sur,
                      '--sample-n', '24', '--seed', '9'])
    _check_script_output(capsys.readouterr().out.splitlines(), img, sur, eval_script._levels8(data), eval_script.known_half('checker', 4).reshape(4, 4), 24, 4)
    # the MNIST script on synthetic IDX files
    root = str(tmp_path / 'datasets')
    _synthetic_mnist(root, 600, 200, 5)
    out = str(tmp_path / 'mnist.dat')
    np.random.seed(4)
    train_mnist.main(['--data_dir', root, '--n_epochs', '1', '--n_train_batch', '2', '--normalise', '--lr', '0.01', '--L2_decay', '1e-3', '--resident',
                      '--out', out])
    capsys.readouterr()
    eval_mnist.main(['--filename', out, '--data_dir', root, '--normalise', '--batch_size', '100', '--inpaint-mean', img, '--inpaint-known', 'bottom',
                     '--surprise', sur, '--sample-n', '8'])
    _, _, te, tel = gen.get_MNIST_dataset(root)
    lev = eval_script._levels8(eval_mnist.pooling(te)[tel < 2] / 255.0)
    _check_script_output(capsys.readouterr().out.splitlines(), img, sur, lev, eval_script.known_half('bottom', 14).reshape(14, 14), 8, 14)
