"""Inner products, distances and linear combinations of two MPS in float64 NumPy (test infrastructure): the
statement of tnml_inner / tnml_axpby in include/tnml.h.  Also the shared cases of tests/test_mps_algebra_host.py (which checks the
conditions on them with this reference alone) and tests/test_mps_algebra_gpu.py (which runs them on the device).

Cores are arrays (ml, D, mr[, L]) with the label on site l; W and V share N, D, L and l, their bonds are free.
"""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from gradient_step_reference import forward64                                                # noqa: E402,F401
import orthogonalize_reference as oref                                                       # noqa: E402


def site_metric(metric, i, D):
    """S_i of metric None / (D, D) / (N, D, D)"""
    if metric is None:
        return np.eye(D)
    metric = np.asarray(metric, dtype=np.float64)
    return metric if metric.ndim == 2 else metric[i]


def _rescale(E, expo):
    """E / |E|_max with the logarithm of the factor added to expo (this reference's own rescaling: any positive factor will do)"""
    m = np.abs(E).max()
    if m == 0.0:
        return E, expo
    return E / m, expo + math.log(m)


def inner(W, V, l, metric=None):
    """(sign, log|<W|V>_S|) by the two transfer half-chains that meet on the label site; a zero product gives (0, -inf)"""
    W = [np.asarray(c, dtype=np.float64) for c in W]
    V = [np.asarray(c, dtype=np.float64) for c in V]
    N, D = len(W), W[0].shape[1]
    EL, lg = np.ones((1, 1)), 0.0
    for i in range(l):
        EL = np.einsum('de,adc,ab,bef->cf', site_metric(metric, i, D), W[i], EL, V[i], optimize=True)
        EL, lg = _rescale(EL, lg)
    ER = np.ones((1, 1))
    for i in range(N - 1, l, -1):
        ER = np.einsum('de,adc,cf,bef->ab', site_metric(metric, i, D), W[i], ER, V[i], optimize=True)
        ER, lg = _rescale(ER, lg)
    v = float(np.einsum('ab,de,adcl,befl,cf->', EL, site_metric(metric, l, D), W[l], V[l], ER, optimize=True))
    if v == 0.0:
        return 0.0, -math.inf
    return math.copysign(1.0, v), math.log(abs(v)) + lg


def inner3(W, V, l, metric=None):
    """the six outputs of tnml_inner as (3, 2): <W|W>, <V|V>, <W|V>"""
    return np.array([inner(W, W, l, metric), inner(V, V, l, metric), inner(W, V, l, metric)])


def dense(cores, l):
    """the whole tensor W[d_0 .. d_{N-1}, l'] (N <= 6)"""
    assert len(cores) <= 6
    T = np.ones((1,))                                            # (..., bond)
    lab = None
    for i, c in enumerate(cores):
        c = np.asarray(c, dtype=np.float64)
        if i == l:
            T = np.tensordot(T, c, (-1, 0))                      # (..., D, mr, L)
            T = np.moveaxis(T, -1, 0)                            # (L, ..., D, mr)
            lab = True
        else:
            T = np.tensordot(T, c, (-1, 0))
    assert lab
    T = T[..., 0]                                                # right bond of the last site is 1
    return np.moveaxis(T, 0, -1)                                 # (d_0 .. d_{N-1}, L)


def inner_dense(W, V, l, metric=None):
    """<W|V>_S as a plain number from the dense tensors"""
    A, B = dense(W, l), dense(V, l)
    N, D = len(W), A.shape[0]
    for i in range(N):
        B = np.moveaxis(np.tensordot(site_metric(metric, i, D), B, (1, i)), 0, i)
    return float((A * B).sum())


def direct_sum(W, V, l, alpha=1.0, beta=1.0, dtype=np.float64):
    """alpha W + beta V as one chain: bonds add, interior cores block-diagonal, site 0 a row concatenation, site N-1 a column stack;
    alpha and beta multiply the label-site blocks in float64.  dtype float32: W and V are taken as float32 values and the label-site
    products are rounded once, everything else is copied -- what tnml_axpby stores."""
    N = len(W)
    out = []
    for i in range(N):
        a, b = np.asarray(W[i], dtype=np.float64), np.asarray(V[i], dtype=np.float64)
        if i == l:
            a, b = alpha * a, beta * b
        nl = 1 if i == 0 else a.shape[0] + b.shape[0]
        nr = 1 if i == N - 1 else a.shape[2] + b.shape[2]
        c = np.zeros((nl, a.shape[1], nr) + a.shape[3:])
        c[:a.shape[0], :, :a.shape[2]] = a                       # (the two blocks share the one row of site 0, the one column of site N-1)
        c[nl - b.shape[0]:, :, nr - b.shape[2]:] = b
        out.append(c.astype(dtype))
    return out


def psi_gram(D, points=48):
    """int_0^1 psi(x) psi(x)^T dx by Gauss-Legendre quadrature, with the feature map written out here"""
    t, w = np.polynomial.legendre.leggauss(points)
    x = 0.5 * (t + 1.0)
    sn, cs = np.sin(np.pi * x / 2), np.cos(np.pi * x / 2)
    p = np.stack([math.sqrt(math.comb(D - 1, s)) * sn ** (D - 1 - s) * cs ** s for s in range(D)], axis=-1)
    return np.einsum('q,qa,qb->ab', 0.5 * w, p, p)


def cosine(t):
    (_, lww), (_, lvv), (s, lwv) = t
    return s * math.exp(lwv - 0.5 * (lww + lvv)) if s != 0 else 0.0


def distance2(t):
    """relative distance squared |W - V|^2 / |W|^2 from the three pairs"""
    (_, lww), (_, lvv), (s, lwv) = t
    return 1.0 + math.exp(lvv - lww) - 2.0 * s * (math.exp(lwv - lww) if s != 0 else 0.0)


def as32(cores):
    return [np.asarray(c, dtype=np.float32) for c in cores]


def as64(cores):
    return [np.asarray(c, dtype=np.float64) for c in cores]


def slots_of(cores, l, cap, D, L):
    """(slots (N, cap D cap), label buffer (cap D cap L,)) float32 with zeros behind every core: what Context.core_slots returns"""
    N = len(cores)
    slots = np.zeros((N, cap * D * cap), dtype=np.float32)
    lab = np.zeros(cap * D * cap * L, dtype=np.float32)
    for i, c in enumerate(cores):
        flat = np.asarray(c, dtype=np.float32).ravel()
        if i == l:
            lab[:flat.size] = flat
        else:
            slots[i, :flat.size] = flat
    return slots, lab


# ---------------------------------------------------------------------------------------------------------------
# shared cases
# ---------------------------------------------------------------------------------------------------------------
ROWS = [(2, 2), (3, 3), (8, 10)]                 # (D, L)
MW, MV = 5, 7                                    # largest bond of W and of V in the ragged chains
B = 24                                           # samples of the calibration / prediction batch
MIN_DISTANCE = 1e-3                              # distance and cosine comparisons use pairs at least this far apart (relative)


def spd_metric(rng, D, sites=None):
    """a symmetric positive definite metric, (D, D) or (sites, D, D), of entries about 1"""
    shape = (D, D) if sites is None else (sites, D, D)
    G = rng.standard_normal(shape)
    return np.einsum('...ab,...cb->...ac', G, G) / D + 0.25 * np.eye(D)


def metrics_of(rng, N, D):
    return [('none', None), ('shared', spd_metric(rng, D)), ('per_site', spd_metric(rng, D, N))]


def make_pair(N, D, L, l, rng, mw=MW, mv=MV, ragged=True):
    """(W, V, X): two independent chains (float32 values as float64), calibrated to max|f| = 1 on X (B, N, D)"""
    X = oref.features(rng, B, N, D)
    bw = oref.ragged_bonds(N, mw, rng) if ragged and N > 2 else [mw] * (N - 1)
    bv = oref.ragged_bonds(N, mv, rng) if ragged and N > 2 else [mv] * (N - 1)
    return oref.make_cores(N, D, L, bw, l, rng, X), oref.make_cores(N, D, L, bv, l, rng, X), X


def small_cases():
    """(N, D, L, l) of every small pair: N = 2, 3 uniform and N = 17 ragged, at every label position, for the three rows"""
    return [(N, D, L, l) for (D, L) in ROWS for N in (2, 3, 17) for l in range(N)]


def build_small(case):
    N, D, L, l = case
    rng = np.random.default_rng([21, N, D, L, l])
    W, V, X = make_pair(N, D, L, l, rng)
    return W, V, X, metrics_of(rng, N, D)


def tile_pair():
    """bonds 64 and 33 on a 17-site chain, label inside: the edges of the kernels' thread tiles (64 x 33 > 1024 elements per E)"""
    rng = np.random.default_rng(64033)
    N, D, L, l = 17, 2, 2, 8
    W, V, X = make_pair(N, D, L, l, rng, 64, 33, ragged=False)
    return (N, D, L, l), W, V, X, metrics_of(rng, N, D)


def long_pair(l=0):
    """N = 784, bond 20, L = 2 (C3): the exponent bookkeeping.  V is W with every element moved by up to 5 %"""
    rng = np.random.default_rng(784)
    N, D, L = 784, 2, 2
    X = oref.features(rng, 8, N, D)
    W = oref.make_cores(N, D, L, [20] * (N - 1), l, rng, X)
    V = as64(as32([c * (1.0 + 0.05 * rng.uniform(-1, 1, c.shape)) for c in W]))
    return (N, D, L, l), W, V


def raw_long_chain(l=0):
    """N = 784, bond 20 as Network() draws it with normalize=True before the calibration: U[0, 1) / (M 0.5 0.64 D), f about 1e-66"""
    rng = np.random.default_rng(66)
    N, D, L, M = 784, 2, 2, 20
    scale = M * 0.5 * 0.64 * D
    shapes = oref.shapes_of(N, D, L, [M] * (N - 1), l)
    return (N, D, L, l), as64(as32([rng.random(s) / scale for s in shapes]))


# compression certificate: the planted cases of the orthogonal-form tests that cut into the gap
CERT_CASES = [c for c in oref.COMPRESS_CASES if c[0] in ('half_l0', 'half_l8', 'half_D3')]


def certificate_reference(case):
    """(W, X, m_max, l, relative distance^2 between W and its compression, sum of the discarded weights) in float64"""
    name, (D, cap, L), N, l, m_max, thr = case
    W, X = oref.build_compress_case(case)
    unit, _, disc, logn = oref.compress(W, l, m_max, thr)
    Wc, _ = oref.with_gauge(unit, logn)
    return W, X, Wc, distance2(inner3(W, Wc, l)), float(np.sum(disc))
