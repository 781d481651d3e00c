"""Per-pixel conditionals given any set of known pixels in NumPy (test infrastructure): the statement of
tnml_site_conditionals in include/tnml.h, on top of tests/sample_reference.py and tests/sample_masked_reference.py.  Per sample the
metric environments from the right of section 23, the matching environment from the left, the one-site matrix Q that leaves out
the site's own metric, and from it the K densities of the site and their statistics; vectorised over the samples of a class slot.
The same statement runs in float64 and in np.longdouble (80-bit here, eps 1.08e-19): their difference is the reference's own
error, from which the bounds of tests/test_site_cond_gpu.py come (BOUNDS below, with the function that produced them).  Also a dense
enumeration of the one-site conditionals for short chains, and the shared cases of tests/test_site_cond_host.py and
tests/test_site_cond_gpu.py.

mask (n, N) or (N,) bool, known (n, N) levels (read where the mask is set), classes (n,) with -1 = the label summed.
p[s, i, k] = p(x_i = k | the known pixels of s other than i [, class]): the posterior marginal on a free site, the leave-one-out
conditional on a known one."""
import functools
import math

import numpy as np

import sample_masked_reference as M
import sample_reference as S

MEASURES = ('q', 'mean', 'var', 'entropy', 'logp_known')


def _rescale(E):
    """(E 2^-e per sample, e): e the exponent of frexp of the largest magnitude (0 where that is 0)"""
    mx = np.abs(E).reshape(len(E), -1).max(axis=1)
    _, e = np.frexp(mx.astype(np.float64))
    e = np.where(mx > 0, e, 0)
    return E * np.ldexp(np.ones(len(E), dtype=E.dtype), -e)[:, None, None], e


def _slices(core, is_label, q):
    """the (ml, D, mr) slices a class slot sums over on this site"""
    if not is_label:
        return [core]
    return [core[..., c] for c in (range(core.shape[3]) if q < 0 else [q])]


def conditionals(cores, l, phi, w, values, classes, mask, known, dtype=np.float64):
    """-> {'q': (n, N, D, D) Q / tr(S Q), 'p': (n, N, K), 'stats': (n, N, 4) mean, variance, entropy, log p(known level) (0 on a free
    site), 'mode': (n, N) the first level of largest density, 'logp': (n,) log p(known [| class])}, all in `dtype`"""
    cores = [np.asarray(c, dtype=dtype) for c in cores]
    phi, w = np.asarray(phi, dtype=dtype), np.asarray(w, dtype=dtype)
    classes = np.asarray(classes, dtype=np.int64)
    n, N, K, D = len(classes), len(cores), len(w), phi.shape[1]
    values = np.arange(K, dtype=dtype) if values is None else np.asarray(values, dtype=dtype)
    mask = np.broadcast_to(np.asarray(mask, dtype=bool), (n, N))
    known = np.zeros((n, N), dtype=np.int64) if known is None else np.asarray(known, dtype=np.int64)
    Sg = np.einsum('k,kd,ke->de', w, phi, phi)
    kk = np.where(mask, known, 0)
    Sm = np.where(mask[:, :, None, None], w[kk][:, :, None, None] * phi[kk][:, :, :, None] * phi[kk][:, :, None, :], Sg)     # (n, N, D, D)
    out = {'q': np.zeros((n, N, D, D), dtype=dtype), 'p': np.zeros((n, N, K), dtype=dtype), 'logp': np.zeros(n, dtype=dtype)}
    ln2 = np.log(dtype(2))
    for q in sorted(set(int(c) for c in classes)):
        idx = np.where(classes == q)[0]
        # rows: the samples of the slot, then the empty mask (the slot's normaliser)
        Sr = np.concatenate([Sm[idx], np.broadcast_to(Sg, (1, N, D, D))])
        m = len(Sr)
        R = [None] * (N + 1)
        R[N] = np.ones((m, 1, 1), dtype=dtype)
        ex = np.zeros(m, dtype=np.int64)
        for i in range(N - 1, -1, -1):
            E = 0
            for C in _slices(cores[i], i == l, q):
                T0 = np.einsum('adc,ncf->nadf', C, R[i + 1])
                E = E + np.einsum('nadf,bdf->nab', np.einsum('nde,naef->nadf', Sr[:, i], T0), C)
            R[i], e = _rescale(E)
            ex += e
        with np.errstate(divide='ignore'):
            Etot = np.log(R[0][:, 0, 0]) + ln2 * ex.astype(dtype)
        out['logp'][idx] = Etot[:-1] - Etot[-1]
        Lf = np.ones((m - 1, 1, 1), dtype=dtype)
        for i in range(N):
            Q, nxt = 0, 0
            for C in _slices(cores[i], i == l, q):
                T2 = np.einsum('nab,adc->nbdc', Lf, C)
                T1 = np.einsum('bef,ncf->nbec', C, R[i + 1][:-1])
                Q = Q + np.einsum('nbdc,nbec->nde', T2, T1)
                nxt = nxt + np.einsum('nbec,bef->ncf', np.einsum('nde,nbdc->nbec', Sr[:-1, i], T2), C)
            Lf, _ = _rescale(nxt)
            tr = np.einsum('de,nde->n', Sg, Q)
            out['q'][idx, i] = Q / tr[:, None, None]
            out['p'][idx, i] = np.maximum(0, w * np.einsum('kd,nde,ke->nk', phi, Q, phi)) / tr[:, None]
    out.update(statistics(out['p'], values, mask, known))
    return out


def statistics(p, values, mask, known):
    """{'stats': (.., 4), 'mode': (..)} of a table p (n, N, K): mean, variance, entropy (a zero density adds nothing), log p(known level)
    on a known site and 0 on a free one; the first level of largest density"""
    values = np.asarray(values, dtype=p.dtype)
    mean = (p * values).sum(-1)
    var = (p * (values - mean[..., None]) ** 2).sum(-1)
    with np.errstate(divide='ignore', invalid='ignore'):
        ent = -np.where(p > 0, p * np.log(p), 0).sum(-1)
        pk = np.take_along_axis(p, np.where(mask, known, 0)[..., None].astype(np.int64), -1)[..., 0]
        lk = np.where(mask, np.log(pk), 0)
    return {'stats': np.stack([mean, var, ent, lk], -1), 'mode': p.argmax(-1).astype(np.int32)}


def decidable_modes(p):
    """(n, N) bool: the two largest densities of the site differ by more than sample_reference.MARGIN, relative"""
    top = np.sort(np.asarray(p, dtype=np.float64), axis=-1)[..., -2:]
    return top[..., 1] - top[..., 0] > S.MARGIN * top[..., 1]


def dense_conditional(P, mask, known, q, i):
    """p(x_i = . | the known levels other than site i [, class q]), (K,), from the joint table P[k_0 .. k_{N-1}, l] of
    sample_reference.dense_joint"""
    N = P.ndim - 1
    Pq = P.sum(-1) if q < 0 else P[..., q]
    sub = Pq[tuple(int(known[j]) if (mask[j] and j != i) else slice(None) for j in range(N))]
    free = [j for j in range(N) if not mask[j] or j == i]
    v = sub.sum(axis=tuple(a for a, j in enumerate(free) if j != i))
    return v / v.sum()


# ---------------------------------------------------------------------------------------------------------------
# differences between two results in the measures of the bounds
# ---------------------------------------------------------------------------------------------------------------
def differences(a, b, values):
    """{measure: worst difference} of result a against result b (the reference): max|dQ| / max|Q| per (sample, site); |d mean| / range,
    |d variance| / range^2, |d entropy|, |d log p(known)| (where the reference's is finite)"""
    rng = float(np.max(values) - np.min(values))
    qa, qb = np.asarray(a['q'], dtype=np.longdouble), np.asarray(b['q'], dtype=np.longdouble)
    sa, sb = np.asarray(a['stats'], dtype=np.longdouble), np.asarray(b['stats'], dtype=np.longdouble)
    dq = np.abs(qa - qb).max(axis=(-1, -2)) / np.abs(qb).max(axis=(-1, -2))
    fin = np.isfinite(sb[..., 3])
    d = np.abs(sa - sb)
    return {'q': float(dq.max()), 'mean': float(d[..., 0].max()) / rng, 'var': float(d[..., 1].max()) / rng ** 2,
            'entropy': float(d[..., 2].max()), 'logp_known': float(d[..., 3][fin].max()) if fin.any() else 0.0}


def worse(x, y):
    return {k: max(x.get(k, 0.0), y[k]) for k in MEASURES}


# ---------------------------------------------------------------------------------------------------------------
# shared cases
# ---------------------------------------------------------------------------------------------------------------
DENSE_L = (0, 2, 3)
RAGGED_POSITIONS = {(2, 2): tuple(range(17)), (3, 3): (0, 5, 8, 11, 16), (8, 10): (0, 5, 8, 11, 16)}
LEVEL_KINDS = ('drawn', 'random')
CLASSES = ['dense'] + [('ragged', row, kind) for row in S.ROWS for kind in LEVEL_KINDS] + ['wide', 'long']


def dense_inputs(l):
    """the N = 4, K = 3, D = 2, L = 2 chain with the label on l: all 16 masks, classes -1 / 0 / 1, random known levels, 12 rows a mask"""
    D, L, N, K = 2, 2, 4, 3
    cores, phi, w = S.dense_case(D, L, N, K, l)
    masks = M.all_masks(N)
    per = 12
    rng = np.random.default_rng([61, l])
    mask = np.repeat(np.array(masks), per, axis=0)
    classes = np.tile(np.array([-1, 0, 1] * 4, dtype=np.int32), len(masks))
    known = rng.integers(0, K, (len(mask), N)).astype(np.int32)
    values = np.array([0.0, 0.25, 1.0])
    return cores, l, phi, w, values, classes, mask, known


def ragged_cases(row):
    """(index in sample_reference.draw_cases(), case) of the ragged 17-site cases of row (D, L) that the device tests run"""
    return [(ci, c) for ci, c in enumerate(S.draw_cases()) if (c[1], c[2]) == row and c[3] in RAGGED_POSITIONS[row]]


@functools.lru_cache(maxsize=None)
def ragged_inputs(ci, kind):
    """(cores, l, phi, w, values, classes, per-sample masks, shared mask, known) of a ragged case: known levels drawn from the model
    by sample_reference.walk (given the sample's class), or random"""
    case = S.draw_cases()[ci]
    N, D, L, l, K = case
    cores, phi, w, classes, u = S.build_draw_case(case)
    mask, shared, known = M.ragged_inputs(ci, case)
    if kind == 'drawn':
        known = S.walk(cores, l, phi, w, classes, u)[0]
    x, _, _ = S.grid(K, D)
    return cores, l, phi, w, x, classes, mask, shared, np.ascontiguousarray(known, dtype=np.int32)


@functools.lru_cache(maxsize=None)
def wide_inputs(wi):
    """bond 50 (L = 10) and bond 64 of sample_reference.wide_cases(): (cores, l, phi, w, values, classes, suffix mask, random masks, known)"""
    case = S.wide_cases()[wi]
    N, D, L, l, Mb, K = case
    cores, phi, w, classes, u = S.build_wide_case(case)
    suffix, rnd, _ = M.wide_inputs(case)
    known = S.walk(cores, l, phi, w, classes, u)[0]
    x, _, _ = S.grid(K, D)
    return cores, l, phi, w, x, classes, suffix, rnd, np.ascontiguousarray(known, dtype=np.int32)


@functools.lru_cache(maxsize=None)
def long_inputs(which):
    """N = 784, bond 20: (cores, l, phi, w, values, classes, {name: mask}, known) with the masks of sample_masked_reference.long_inputs()
    and the full one"""
    _, W, l = S.long_cases()[which]
    x, phi, w = S.grid(256, 2)
    masks, known = M.long_inputs()
    masks = dict(masks, full=np.ones(784, dtype=bool))
    return W, l, phi, w, x, M.LONG_CLASSES, masks, known


@functools.lru_cache(maxsize=None)
def reference(cls, key, which):
    """the float64 result of one call of a class of cases, computed once: key is l (dense), (ci, kind) (ragged), wi (wide), which
    chain (long); `which` names the mask of the call"""
    if cls == 'dense':
        a = dense_inputs(key)
        return conditionals(*a)
    if cls == 'ragged':
        a = ragged_inputs(*key)
        return conditionals(*a[:6], a[6] if which == 'own' else a[7], a[8])
    if cls == 'wide':
        a = wide_inputs(key)
        return conditionals(*a[:6], a[6] if which == 'suffix' else a[7], a[8])
    a = long_inputs(key)
    return conditionals(*a[:6], a[6][which], a[7])


# ---------------------------------------------------------------------------------------------------------------
# bounds
# ---------------------------------------------------------------------------------------------------------------
def accumulation(N, m, D):
    """figure (b): the first-order accumulation of one site's sums times the sites, 2^-53 N m^2 D"""
    return 2.0 ** -53 * N * m * m * D


def round_up(x):
    """x rounded up to one digit"""
    e = math.floor(math.log10(x))
    return math.ceil(x / 10.0 ** e - 1e-9) * 10.0 ** e


def own_error(args, n=None):
    """figure (a) of one call: the float64 statement against the long-double one, in every measure (n: the first n samples only)"""
    cores, l, phi, w, values, classes, mask, known = args
    if n is not None:
        classes, known = classes[:n], known[:n]
        mask = mask if np.ndim(mask) == 1 else mask[:n]
    return differences(conditionals(cores, l, phi, w, values, classes, mask, known),
                       conditionals(cores, l, phi, w, values, classes, mask, known, dtype=np.longdouble), values)


def class_calls(cls, sample=False):
    """[(args of conditionals, (N, m, D))] of a class of cases; sample: one call of the class (what the host test recomputes)"""
    out = []
    if cls == 'dense':
        out = [(dense_inputs(l), (4, 3, 2)) for l in DENSE_L]
    elif cls == 'wide':
        for wi, case in enumerate(S.wide_cases()):
            a = wide_inputs(wi)
            out += [(a[:6] + (m, a[8]), (case[0], case[4], case[1])) for m in (a[6], a[7])]
    elif cls == 'long':
        for which in (0, 1):
            a = long_inputs(which)
            out += [(a[:6] + (m, a[7]), (784, 20, 2)) for m in a[6].values()]
    else:
        _, row, kind = cls
        for ci, case in ragged_cases(row):
            a = ragged_inputs(ci, kind)
            out += [(a[:6] + (m, a[8]), (17, 7, row[0])) for m in (a[6], a[7])]
    return out[:1] if sample else out


def figures(cls, sample=False):
    """(figure (a) per measure, figure (b)) of a class of cases"""
    a, b = {}, 0.0
    for args, (N, m, D) in class_calls(cls, sample):
        a = worse(a, own_error(args))
        b = max(b, accumulation(N, m, D))
    return a, b


def bounds_of(cls):
    """the bound of every measure of a class: ten times the larger of (a) and (b), rounded up to one digit"""
    a, b = figures(cls)
    return {k: round_up(10.0 * max(a[k], b)) for k in MEASURES}


# BOUNDS = {cls: bounds_of(cls) for cls in CLASSES}, as committed (tests/test_site_cond_host.py recomputes the dense class whole and
# one call of every other class).  Figure (b) decides wherever a row holds one number five times: the drawn levels, the wide and
# the long chains.  With random known levels figure (a) decides, most of all in log p(known level): the reference's own error on an
# image the model finds improbable, as section 23 found it (1.0e-10, 1.0e-11 and 1.6e-8 on the three rows).
BOUNDS = {
    'dense': {'q': 2e-12, 'mean': 8e-13, 'var': 5e-13, 'entropy': 2e-12, 'logp_known': 2e-12},
    ('ragged', (2, 2), 'drawn'): {'q': 2e-12, 'mean': 2e-12, 'var': 2e-12, 'entropy': 2e-12, 'logp_known': 2e-12},
    ('ragged', (2, 2), 'random'): {'q': 5e-11, 'mean': 8e-12, 'var': 4e-12, 'entropy': 3e-11, 'logp_known': 2e-9},
    ('ragged', (3, 3), 'drawn'): {'q': 3e-12, 'mean': 3e-12, 'var': 3e-12, 'entropy': 3e-12, 'logp_known': 3e-12},
    ('ragged', (3, 3), 'random'): {'q': 4e-12, 'mean': 3e-12, 'var': 3e-12, 'entropy': 6e-12, 'logp_known': 2e-10},
    ('ragged', (8, 10), 'drawn'): {'q': 8e-12, 'mean': 8e-12, 'var': 8e-12, 'entropy': 8e-12, 'logp_known': 8e-12},
    ('ragged', (8, 10), 'random'): {'q': 4e-10, 'mean': 2e-9, 'var': 2e-9, 'entropy': 6e-9, 'logp_known': 2e-7},
    'wide': {'q': 9e-11, 'mean': 9e-11, 'var': 9e-11, 'entropy': 9e-11, 'logp_known': 9e-11},
    'long': {'q': 7e-10, 'mean': 7e-10, 'var': 7e-10, 'entropy': 7e-10, 'logp_known': 7e-10},
}
