"""Pixel-pair marginals in NumPy (test infrastructure): the statement of tnml_pair_marginals in
include/tnml.h.  The shared metric environments L_i, R_i of the grid's S (label summed, or one class), B_j (site j closed from the
right, its pixel open), the one-site marginals, the walk of the D^2 matrices C_i,j[d,d'] from site i to the right and their
products with B_j; from q_ij the K x K table of the pair and covariance, correlation and mutual information.  The same statement
runs in float64 and in np.longdouble (80-bit here, eps 1.08e-19): their difference is the reference's own error, from which the
bounds of tests/test_pair_gpu.py come (BOUNDS below, with the function that produced them).  Also dense enumeration for short
chains, in the levels (K^N L numbers) and in the features (the whole tensor, any K), and the shared cases of
tests/test_pair_host.py and tests/test_pair_gpu.py.

Powers of two are taken out of every environment and of the D^2 walk matrices together; that is exact, and the normalisation of
q1_j and q_ij removes them."""
import functools
import math

import numpy as np

import mps_algebra_reference as A
import sample_reference as S

MEASURES = ('q', 'cov', 'corr', 'mi')
CORR_MIN_STD = 1e-6                              # |d corr| is measured where both reference standard deviations exceed this times the range


def _rescale(E):
    mx = float(np.abs(E).max())
    if not mx > 0 or not np.isfinite(mx):
        return E
    return E * np.ldexp(E.dtype.type(1), -int(np.frexp(mx)[1]))


def _slices(core, is_label, q):
    if not is_label:
        return [core]
    return [core[..., c] for c in (range(core.shape[3]) if q < 0 else [q])]


def pair_table(q, phi, w):
    """p(k,k') = max(0, w_k w_k' sum phi_k[d] phi_k[d'] q[..., (d,d'), (e,e')] phi_k'[e] phi_k'[e']): (..., D^2, D^2) -> (..., K, K)"""
    q = np.asarray(q)
    phi, w = np.asarray(phi, dtype=q.dtype), np.asarray(w, dtype=q.dtype)
    K, D = phi.shape
    pp = (phi[:, :, None] * phi[:, None, :]).reshape(K, D * D)
    G = np.einsum('kx,...xy->...ky', pp, q.reshape(q.shape[:-2] + (D * D, D * D)))
    return np.maximum(0, (w[:, None] * w[None, :]) * np.einsum('...ky,jy->...kj', G, pp))


def site_statistics(p, values):
    """(.., 3) mean, variance, entropy of a table p (.., K); a zero density adds nothing"""
    values = np.asarray(values, dtype=p.dtype)
    mean = (p * values).sum(-1)
    var = (p * (values - mean[..., None]) ** 2).sum(-1)
    with np.errstate(divide='ignore', invalid='ignore'):
        ent = -np.where(p > 0, p * np.log(p), 0).sum(-1)
    return np.stack([mean, var, ent], -1)


def pair_statistics(P, values):
    """(.., 3) covariance, correlation (0 where a variance is 0), mutual information in nats of a table P (.., K, K), with the
    marginals summed from the table"""
    values = np.asarray(values, dtype=P.dtype)
    pi, pj = P.sum(-1), P.sum(-2)
    mi, mj = (pi * values).sum(-1), (pj * values).sum(-1)
    cov = np.einsum('...kj,k,j->...', P, values, values) - mi * mj
    vi = (pi * (values - mi[..., None]) ** 2).sum(-1)
    vj = (pj * (values - mj[..., None]) ** 2).sum(-1)
    with np.errstate(divide='ignore', invalid='ignore'):
        corr = np.where((vi > 0) & (vj > 0), cov / (np.sqrt(vi) * np.sqrt(vj)), 0)
        info = np.where(P > 0, P * np.log(P / (pi[..., :, None] * pj[..., None, :])), 0).sum((-1, -2))
    return np.stack([cov, corr, info], -1)


def pair_marginals(cores, l, phi, w, values=None, q=-1, rows=None, dtype=np.float64):
    """-> {'q1': (N, D, D), 'p1': (N, K), 'stats1': (N, 3), 'q': (R, N, D^2, D^2), 'stats': (R, N, 3), 'std': (N,)} in `dtype`;
    rows None: all sites.  Entries (r, j) with j <= rows[r] are zero."""
    cores = [np.asarray(c, dtype=dtype) for c in cores]
    phi, w = np.asarray(phi, dtype=dtype), np.asarray(w, dtype=dtype)
    N, K, D = len(cores), len(w), phi.shape[1]
    DD = D * D
    values = np.arange(K, dtype=dtype) if values is None else np.asarray(values, dtype=dtype)
    rows = list(range(N)) if rows is None else [int(r) for r in rows]
    Sg = np.einsum('k,kd,ke->de', w, phi, phi)
    sl = [_slices(cores[i], i == l, q) for i in range(N)]
    R = [None] * (N + 1)
    R[N] = np.ones((1, 1), dtype=dtype)
    for i in range(N - 1, 0, -1):
        R[i] = _rescale(sum(np.einsum('adc,de,cf,bef->ab', C, Sg, R[i + 1], C, optimize=True) for C in sl[i]))
    Lf = [np.ones((1, 1), dtype=dtype)]
    for i in range(N - 1):
        Lf.append(_rescale(sum(np.einsum('ab,adc,de,bef->cf', Lf[i], C, Sg, C, optimize=True) for C in sl[i])))
    B = [sum(np.einsum('aec,cf,bgf->egab', C, R[j + 1], C, optimize=True) for C in sl[j]) for j in range(N)]
    out = {'q1': np.zeros((N, D, D), dtype=dtype), 'q': np.zeros((len(rows), N, DD, DD), dtype=dtype),
           'stats': np.zeros((len(rows), N, 3), dtype=dtype)}
    for j in range(N):
        q1 = np.einsum('ab,egab->eg', Lf[j], B[j])
        out['q1'][j] = q1 / (Sg * q1).sum()
    out['p1'] = np.maximum(0, w * np.einsum('kd,nde,ke->nk', phi, out['q1'], phi))
    out['stats1'] = site_statistics(out['p1'], values)
    out['std'] = np.sqrt(out['stats1'][:, 1])
    for r, i in enumerate(rows):
        if i >= N - 1:
            continue
        Cm = _rescale(sum(np.einsum('ab,adc,bxf->dxcf', Lf[i], C, C, optimize=True) for C in sl[i]))
        for j in range(i + 1, N):
            Q = np.einsum('dxab,egab->dxeg', Cm, B[j])
            Q = Q / np.einsum('dx,eg,dxeg->', Sg, Sg, Q)
            out['q'][r, j] = Q.reshape(DD, DD)
            if j < N - 1:
                Cm = _rescale(sum(np.einsum('eg,aec,dxab,bgf->dxcf', Sg, C, Cm, C, optimize=True) for C in sl[j]))
        out['stats'][r, i + 1:] = pair_statistics(pair_table(out['q'][r, i + 1:], phi, w), values)
    return out


def label_information(cores, l, phi, w, dtype=np.float64):
    """I(x_i; l) = sum_c P(c) KL(p(x_i | c) || p(x_i)), (N,), from the one-site marginals of every class and the summed label"""
    L = np.asarray(cores[l]).shape[3]
    pc = np.exp(S.class_log_weights(cores, l, phi, w)).astype(dtype)
    p = pair_marginals(cores, l, phi, w, None, -1, [], dtype)['p1']
    out = np.zeros(len(cores), dtype=dtype)
    for c in range(L):
        if pc[c] > 0:
            out += pc[c] * kl(pair_marginals(cores, l, phi, w, None, c, [], dtype)['p1'], p)
    return out


def kl(p, r):
    """sum_k p log(p / r) over the last axis; a zero p adds nothing"""
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where(p > 0, p * np.log(p / r), 0).sum(-1)


# ---------------------------------------------------------------------------------------------------------------
# dense enumeration
# ---------------------------------------------------------------------------------------------------------------
def dense_levels(cores, l, phi, w, values, q):
    """from the joint table P[k_0 .. k_{N-1}, l] of sample_reference.dense_joint (K^N L numbers): {'p1': (N, K), 'P': (N, N, K, K)
    (zero for j <= i), 'stats1', 'stats' (N, N, 3), 'label_info': (N,) (q = -1 only)}"""
    P = S.dense_joint(cores, l, phi, w)
    N, K = P.ndim - 1, P.shape[0]
    Pq = P.sum(-1) if q < 0 else P[..., q] / P[..., q].sum()
    out = {'p1': np.stack([Pq.sum(tuple(a for a in range(N) if a != i)) for i in range(N)]), 'P': np.zeros((N, N, K, K))}
    for i in range(N):
        for j in range(i + 1, N):
            out['P'][i, j] = Pq.sum(tuple(a for a in range(N) if a not in (i, j)))
    out['stats1'] = site_statistics(out['p1'], values)
    out['stats'] = pair_statistics(out['P'], values) * (np.arange(N)[:, None] < np.arange(N)[None, :])[..., None]
    if q < 0:
        Pl = P.sum(tuple(range(N)))
        out['label_info'] = np.array([
            kl_joint(P.sum(tuple(a for a in range(N) if a != i)), out['p1'][i], Pl) for i in range(N)])
    return out


def kl_joint(Pkc, pk, pc):
    with np.errstate(divide='ignore', invalid='ignore'):
        return float(np.where(Pkc > 0, Pkc * np.log(Pkc / (pk[:, None] * pc[None, :])), 0).sum())


def dense_features(cores, l, phi, w, values, q):
    """the result of pair_marginals(rows = all) from the whole tensor W[d_0 .. d_{N-1}, l'] (any K): every site but the open ones
    closed with S, no environment and no walk"""
    W = A.dense(cores, l)
    N, D = W.ndim - 1, W.shape[0]
    DD = D * D
    phi, w = np.asarray(phi, dtype=np.float64), np.asarray(w, dtype=np.float64)
    values = np.arange(len(w), dtype=np.float64) if values is None else np.asarray(values, dtype=np.float64)
    Sg = np.einsum('k,kd,ke->de', w, phi, phi)
    Wq = W if q < 0 else W[..., q:q + 1]
    out = {'q1': np.zeros((N, D, D)), 'q': np.zeros((N, N, DD, DD))}

    def closed(keep):
        """rho[(d_i, d_i') for i in keep]: W W with S on every other site and the label summed"""
        V = Wq
        for a in range(N):
            if a not in keep:
                V = np.moveaxis(np.tensordot(Sg, V, (1, a)), 0, a)
        ax = [a for a in range(N + 1) if a not in keep]
        T = np.tensordot(Wq, V, (ax, ax))                                     # (d_keep ..., d'_keep ...)
        return T

    for i in range(N):
        q1 = closed((i,))
        out['q1'][i] = q1 / (Sg * q1).sum()
        for j in range(i + 1, N):
            T = closed((i, j)).transpose(0, 2, 1, 3)                           # (d, d', e, e')
            out['q'][i, j] = (T / np.einsum('dx,eg,dxeg->', Sg, Sg, T)).reshape(DD, DD)
    out['p1'] = np.maximum(0, w * np.einsum('kd,nde,ke->nk', phi, out['q1'], phi))
    out['stats1'] = site_statistics(out['p1'], values)
    out['std'] = np.sqrt(out['stats1'][:, 1])
    out['stats'] = pair_statistics(pair_table(out['q'], phi, w), values) * (np.arange(N)[:, None] < np.arange(N)[None, :])[..., None]
    return out


# ---------------------------------------------------------------------------------------------------------------
# differences between two results in the measures of the bounds
# ---------------------------------------------------------------------------------------------------------------
def pairs_of(rows, N):
    """(R, N) bool: the entries a row covers"""
    return np.asarray(rows)[:, None] < np.arange(N)[None, :]


def corr_condition(ref, rows, values):
    """(R, N) bool: both reference standard deviations of the pair exceed CORR_MIN_STD times the range"""
    rng = float(np.max(values) - np.min(values))
    ok = np.asarray(ref['std'], dtype=np.float64) > CORR_MIN_STD * rng
    return ok[np.asarray(rows)][:, None] & ok[None, :]


def differences(a, b, rows, values):
    """{measure: worst difference} of result a against result b (the reference) over the pairs of `rows`: max|dq| / max|q| per pair
    (and per site for q1); |d cov| / range^2 (and the one-site mean / range, variance / range^2); |d corr| where corr_condition
    holds; |d MI| in nats (and the one-site entropy)"""
    rng = float(np.max(values) - np.min(values))
    N = np.asarray(b['q1']).shape[0]
    ld = lambda x: np.asarray(x, dtype=np.longdouble)
    out = {k: 0.0 for k in MEASURES}
    if a.get('q1') is not None:
        out['q'] = float((np.abs(ld(a['q1']) - ld(b['q1'])).max((-1, -2)) / np.abs(ld(b['q1'])).max((-1, -2))).max())
    if a.get('stats1') is not None:
        d = np.abs(ld(a['stats1']) - ld(b['stats1']))
        out['cov'] = max(float(d[:, 0].max()) / rng, float(d[:, 1].max()) / rng ** 2)
        out['mi'] = float(d[:, 2].max())
    cover = pairs_of(rows, N)
    if not cover.any():
        return out
    if a.get('q') is not None:
        qa, qb = ld(a['q'])[cover], ld(b['q'])[cover]
        out['q'] = max(out['q'], float((np.abs(qa - qb).max((-1, -2)) / np.abs(qb).max((-1, -2))).max()))
    if a.get('stats') is not None:
        d = np.abs(ld(a['stats']) - ld(b['stats']))
        out['cov'] = max(out['cov'], float(d[..., 0][cover].max()) / rng ** 2)
        cc = cover & corr_condition(b, rows, values)
        out['corr'] = float(d[..., 1][cc].max()) if cc.any() else 0.0
        out['mi'] = max(out['mi'], float(d[..., 2][cover].max()))
    return out


def worse(x, y):
    return {k: max(x.get(k, 0.0), y[k]) for k in MEASURES}


# ---------------------------------------------------------------------------------------------------------------
# shared cases: (cores, l, phi, w, values, class slot, rows) per call
# ---------------------------------------------------------------------------------------------------------------
DENSE_L = (0, 2, 3)
DENSE_K = (4, 256)
LONG_K = 16
CLASSES = ['dense'] + [('ragged', row) for row in S.ROWS] + ['wide', 'long']


def dense_inputs(l, K, N=4):
    """the N = 4 (or 5), D = 2, L = 3 chain with the label on l and K levels"""
    cores, phi, w = S.dense_case(2, 3, N, K, l)
    x, _, _ = S.grid(K, 2)
    return cores, l, phi, w, x


def ragged_cases(row):
    """(index in sample_reference.draw_cases(), case) of the ragged 17-site cases of row (D, L): every label position"""
    return [(ci, c) for ci, c in enumerate(S.draw_cases()) if (c[1], c[2]) == row]


@functools.lru_cache(maxsize=None)
def ragged_inputs(ci):
    case = S.draw_cases()[ci]
    N, D, L, l, K = case
    cores, phi, w, _, _ = S.build_draw_case(case)
    x, _, _ = S.grid(K, D)
    return cores, l, phi, w, x


def ragged_slot(ci):
    """the class slot a ragged case runs with: -1 and the classes in turn over the label positions"""
    N, D, L, l, K = S.draw_cases()[ci]
    return (l % (L + 1)) - 1


@functools.lru_cache(maxsize=None)
def wide_inputs(wi):
    case = S.wide_cases()[wi]
    N, D, L, l, Mb, K = case
    cores, phi, w, _, _ = S.build_wide_case(case)
    x, _, _ = S.grid(K, D)
    return cores, l, phi, w, x


WIDE_SLOTS = (-1, 3)                             # (the class of the second wide case is taken modulo its L)


@functools.lru_cache(maxsize=None)
def long_inputs():
    """the un-calibrated N = 784 chain at bond 20 with LONG_K levels, and its rows {0, 391, label site, 782} in ascending order"""
    _, W, l = S.long_cases()[1]
    x, phi, w = S.grid(LONG_K, 2)
    return W, l, phi, w, x, tuple(sorted({0, 391, l, 782}))


def class_calls(cls, sample=False):
    """[(cores, l, phi, w, values, class slot, rows), (N, m, D)] of a class of cases; sample: one call of the class (what the host
    test recomputes)"""
    out = []
    if cls == 'dense':
        out = [(dense_inputs(l, K) + (q, None), (4, 3, 2)) for l in DENSE_L for K in DENSE_K for q in (-1, 0, 1, 2)]
    elif cls == 'wide':
        for wi, case in enumerate(S.wide_cases()):
            out += [(wide_inputs(wi) + (q % case[2] if q >= 0 else q, None), (case[0], case[4], case[1])) for q in WIDE_SLOTS]
    elif cls == 'long':
        a = long_inputs()
        out = [(a[:5] + (-1, a[5]), (784, 20, 2))]
    else:
        _, row = cls
        out = [(ragged_inputs(ci) + (ragged_slot(ci), None), (17, 7, row[0])) for ci, _ in ragged_cases(row)]
    return out[:1] if sample else out


@functools.lru_cache(maxsize=None)
def reference(cls, index):
    """the float64 result of call `index` of class_calls(cls), computed once"""
    args, _ = class_calls(cls)[index]
    return pair_marginals(*args)


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


def own_error(args):
    """figure (a) of one call: the float64 statement against the long-double one, in every measure"""
    N = len(args[0])
    rows = list(range(N)) if args[6] is None else args[6]
    return differences(pair_marginals(*args), pair_marginals(*args, dtype=np.longdouble), rows, args[4])


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


# BOUNDS = {cls: bounds_of(cls) for cls in CLASSES}, as committed (tests/test_pair_host.py recomputes the dense class whole and one
# call of every other class).
BOUNDS = {
    'dense': {'q': 8e-14, 'cov': 8e-14, 'corr': 9e-14, 'mi': 8e-14},
    ('ragged', (2, 2)): {'q': 2e-12, 'cov': 2e-12, 'corr': 2e-12, 'mi': 2e-12},
    ('ragged', (3, 3)): {'q': 3e-12, 'cov': 3e-12, 'corr': 3e-12, 'mi': 3e-12},
    ('ragged', (8, 10)): {'q': 8e-12, 'cov': 8e-12, 'corr': 8e-12, 'mi': 8e-12},
    'wide': {'q': 9e-11, 'cov': 9e-11, 'corr': 9e-11, 'mi': 9e-11},
    'long': {'q': 7e-10, 'cov': 7e-10, 'corr': 7e-10, 'mi': 7e-10},
}
