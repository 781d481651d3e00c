"""Likelihood gradients of the Born distribution of an MPS in float64 NumPy (test infrastructure): the statement
of tnml_log_norm_grad in include/tnml.h, and of the negative log-likelihood of a batch and its gradient built on it.  Also the shared
cases of tests/test_nll_host.py (which checks the conditions on them with this reference alone) and tests/test_nll_gpu.py (which
runs them on the device).

Cores are arrays (ml, D, mr[, L]) with the label on site l.  S is a symmetric (D, D) metric, or (N, D, D) per site, or None.

    L_0 = 1, L_{i+1}[c,c'] = sum S[d,d'] A_i[a,d,c] L_i[a,a'] A_i[a',d',c']          (the label summed on the label site)
    R_N = 1, R_i[a,a']     = sum S[d,d'] A_i[a,d,c] R_{i+1}[c,c'] A_i[a',d',c']
    Z = R_0,   Gz_i[a,d,c(,l')] = 2 / Z  sum L_i[a,a'] S[d,d'] A_i[a',d',c'(,l')] R_{i+1}[c,c'] = d log|Z| / d A_i
    nll = -mean_s (log f_y[s]^2 - log Z)   or, without labels,   -mean_s (log sum_l f_l[s]^2 - log Z)
    G = Gd - Gz,  Gd = core_grad(cot),  cot[l',s] = 2 delta(l', y_s) / (b f_y[s])   or   2 f_l'[s] / (b sum_l f_l[s]^2)
A += lr G descends the nll.  sum(Gz_i A_i) = 2 and sum(G_i A_i) = 0 at every site.

dtype float32 runs the per-sample chains and their sums in float32 and leaves the metric environments in float64, as the device does.
"""
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p_ in (ROOT, HERE):
    if p_ not in sys.path:
        sys.path.insert(0, p_)

import mps_algebra_reference as A                                                           # noqa: E402
import orthogonalize_reference as oref                                                      # noqa: E402
from core_grad_reference import core_grad_reference                                         # noqa: E402
from orthogonalize_reference import ROWS, labels_of, make_cores, shapes_of                  # noqa: E402,F401
from sample_reference import grid, gram, walk, dense_joint, dense_rows                      # noqa: E402,F401


# ---------------------------------------------------------------------------------------------------------------
# layer 1: the gradient of the log-norm
# ---------------------------------------------------------------------------------------------------------------
def _scaled(E, lg):
    m = np.abs(E).max()
    if m == 0.0:
        return E, lg
    return E / m, lg + math.log(m)


def environments(cores, l, metric=None):
    """(Ls, lgL, Rs, lgR): L_i exp(lgL[i]) for i = 0 .. N-1 and R_i exp(lgR[i]) for i = 0 .. N are the metric environments"""
    cores = [np.asarray(c, dtype=np.float64) for c in cores]
    N, D = len(cores), cores[0].shape[1]
    Ls, lgL = [np.ones((1, 1))], [0.0]
    for i in range(N - 1):
        S = A.site_metric(metric, i, D)
        if i == l:
            E = np.einsum('de,adcl,ab,befl->cf', S, cores[i], Ls[i], cores[i], optimize=True)
        else:
            E = np.einsum('de,adc,ab,bef->cf', S, cores[i], Ls[i], cores[i], optimize=True)
        E, lg = _scaled(E, lgL[i])
        Ls.append(E)
        lgL.append(lg)
    Rs, lgR = [None] * (N + 1), [0.0] * (N + 1)
    Rs[N] = np.ones((1, 1))
    for i in range(N - 1, -1, -1):
        S = A.site_metric(metric, i, D)
        if i == l:
            E = np.einsum('de,adcl,cf,befl->ab', S, cores[i], Rs[i + 1], cores[i], optimize=True)
        else:
            E = np.einsum('de,adc,cf,bef->ab', S, cores[i], Rs[i + 1], cores[i], optimize=True)
        Rs[i], lgR[i] = _scaled(E, lgR[i + 1])
    return Ls, lgL, Rs, lgR


def log_norm_gradient(cores, l, metric=None):
    """(Gz list of float64 arrays shaped like the cores, (sign, log|Z|))"""
    cores = [np.asarray(c, dtype=np.float64) for c in cores]
    N, D = len(cores), cores[0].shape[1]
    Ls, lgL, Rs, lgR = environments(cores, l, metric)
    z = float(Rs[0][0, 0])
    if z == 0.0:
        raise ZeroDivisionError('<W|W> is zero')
    sign, logz = math.copysign(1.0, z), math.log(abs(z)) + lgR[0]
    G = []
    for i in range(N):
        S = A.site_metric(metric, i, D)
        sub = 'ab,de,becl,cf->adfl' if i == l else 'ab,de,bec,cf->adf'
        X = np.einsum(sub, Ls[i], S, cores[i], Rs[i + 1], optimize=True)
        G.append(2.0 * sign * math.exp(lgL[i] + lgR[i + 1] - logz) * X)
    return G, (sign, logz)


def log_norm(cores, l, metric=None):
    """(sign, log|<W|W>_S|) by this module's right walk"""
    _, _, Rs, lgR = environments(cores, l, metric)
    z = float(Rs[0][0, 0])
    return (0.0, -math.inf) if z == 0.0 else (math.copysign(1.0, z), math.log(abs(z)) + lgR[0])


# ---------------------------------------------------------------------------------------------------------------
# layer 2: the negative log-likelihood of a batch and its gradient
# ---------------------------------------------------------------------------------------------------------------
def forward(cores, l, X):
    """f (L, b) in the dtype of the arguments: both half-chains towards the label site"""
    N, b = len(cores), X.shape[0]
    dt = np.result_type(X.dtype, *[c.dtype for c in cores])
    P = np.ones((b, 1), dtype=dt)
    for i in range(l):
        P = np.einsum('ba,bd,adc->bc', P, X[:, i], cores[i])
    Q = np.ones((b, 1), dtype=dt)
    for i in range(N - 1, l, -1):
        Q = np.einsum('adc,bd,bc->ba', cores[i], X[:, i], Q)
    return np.einsum('ba,bd,adcl,bc->lb', P, X[:, l], cores[l], Q)


def cotangent(f, y):
    """(cot (L, b), terms (b,)): the cotangent of the data term and log f_y^2 (y given) or log sum_l f_l^2 (y None) per sample,
    in the dtype of f; the terms are formed in float64 from the values of f"""
    L, b = f.shape
    f64 = f.astype(np.float64)
    cot = np.zeros_like(f)
    two = f.dtype.type(2.0)
    if y is not None:
        fy = f[y, np.arange(b)]
        cot[y, np.arange(b)] = two / (f.dtype.type(b) * fy)
        terms = np.log(f64[y, np.arange(b)] ** 2)
    else:
        den = (f64 ** 2).sum(axis=0)
        cot = (two * f64 / (b * den)).astype(f.dtype)
        terms = np.log(den)
    return cot, terms


def nll_gradient(cores, l, X, y, metric, dtype=np.float64):
    """(G list, value, log Z): G = Gd - Gz in float64 arrays, value = -mean(terms - log Z); X (b, N, D) features, y (b,) or None.
    dtype float32: the chains, f, the cotangent and Gd in float32 (Gd - Gz rounded to float32 as well), Gz and log Z in float64."""
    c64 = [np.asarray(c, dtype=np.float64) for c in cores]
    cd = [c.astype(dtype) for c in c64]
    Xd = np.asarray(X, dtype=dtype)
    f = forward(cd, l, Xd)
    cot, terms = cotangent(f, y)
    Gd, _ = core_grad_reference(cd, l, Xd, cot)
    Gz, (sign, logz) = log_norm_gradient(c64, l, metric)
    if dtype == np.float32:
        G = [(g - z.astype(np.float32)).astype(np.float64) for g, z in zip(Gd, Gz)]
    else:
        G = [g - z for g, z in zip(Gd, Gz)]
    return G, float(-(terms.mean() - logz)), logz


def nll_value(cores, l, X, y, metric):
    c64 = [np.asarray(c, dtype=np.float64) for c in cores]
    _, terms = cotangent(forward(c64, l, np.asarray(X, dtype=np.float64)), y)
    return float(-(terms.mean() - log_norm(c64, l, metric)[1]))


# ---------------------------------------------------------------------------------------------------------------
# shared cases
# ---------------------------------------------------------------------------------------------------------------
K = 256
BATCHES = (1, 17, 70)                            # on either side of the 64-sample tile


def chain_bonds(N, cap, rng):
    """N-1 bonds in [1, cap]: cap among them, and a bond of 1 wherever the chain has a second bond"""
    bond = [int(v) for v in rng.integers(1, cap + 1, N - 1)]
    where = [int(v) for v in rng.permutation(N - 1)]
    bond[where[0]] = cap
    if N > 2:
        bond[where[1]] = 1
    return bond


def chain_cases():
    """(D, cap, L, N, l) of every shared chain: the six rows, N = 2, 3, 17, the label at both ends and inside"""
    return [(D, cap, L, N, l) for (D, cap, L) in ROWS for N in (2, 3, 17) for l in labels_of(N)]


def case_id(case):
    return 'D%d_M%d_L%d_N%d_l%d' % case


def build_chain(case):
    """the float32-rounded cores (as float64) of a shared chain, calibrated to max|f| = 1 on a batch of its own"""
    D, cap, L, N, l = case
    rng = np.random.default_rng([24, D, cap, L, N, l])
    bond = chain_bonds(N, cap, rng)
    X = oref.features(rng, oref.B, N, D)
    return make_cores(N, D, L, bond, l, rng, X)


def metrics_of(case):
    """[(name, metric)] of a shared chain: none, a random SPD (D, D), a per-site (N, D, D), the grid's S"""
    D, cap, L, N, l = case
    rng = np.random.default_rng([25, D, cap, L, N, l])
    _, phi, w = grid(K, D)
    return [('none', None), ('shared', A.spd_metric(rng, D)), ('per_site', A.spd_metric(rng, D, N)), ('grid', gram(phi, w))]


def raw_long_chain(L, l, factor=1.0):
    """N = 784, bond 20 as Network() draws it before the calibration: U[0, 1) / (M 0.5 0.64 D), f about 1e-66; factor: every
    core times it (0.6: <W|W> under the grid's metric falls to about 1e-350, below float64 itself)"""
    rng = np.random.default_rng([66, L, l])
    N, D, M = 784, 2, 20
    scale = M * 0.5 * 0.64 * D
    return (N, D, L, l), A.as64(A.as32([factor * rng.random(s) / scale for s in shapes_of(N, D, L, [M] * (N - 1), l)]))


def draw_batch(case, cores, b, seed=0):
    """(levels (b, N), labels (b,), features (b, N, D) float32) drawn by `walk` from the case's own chain, classes -1"""
    D, cap, L, N, l = case
    rng = np.random.default_rng([26, D, cap, L, N, l, b, seed])
    _, phi, w = grid(K, D)
    lev, lab, _, _ = walk(cores, l, phi, w, np.full(b, -1), rng.random((b, N + 1)))
    return lev, lab, phi[lev].astype(np.float32)


def likelihood_cases():
    """(chain case, b) of layers 2 and 3: every shared chain with one of the batch sizes, each row seeing all three"""
    out = []
    for k, case in enumerate(chain_cases()):
        out.append((case, BATCHES[k % len(BATCHES)]))
    return out


def likelihood_id(lc):
    return case_id(lc[0]) + '_b%d' % lc[1]


# seeds of draw_batch, chosen on the CPU so that min_s |f_y| / max|f| >= MIN_RATIO holds (tests/test_nll_host.py asserts it)
MIN_RATIO = 1e-3
BATCH_SEED = {}


def build_likelihood_case(lc):
    """(cores, l, levels, labels, X float32 (b, N, D), S): images and labels drawn from the case's own chain"""
    case, b = lc
    D, cap, L, N, l = case
    cores = build_chain(case)
    lev, lab, X = draw_batch(case, cores, b, BATCH_SEED.get(likelihood_id(lc), 0))
    _, phi, w = grid(K, D)
    return cores, l, lev, lab, X, gram(phi, w)


def label_ratio(cores, l, X, y):
    """min_s |f_y[s]| / max |f|: what the cotangent 1 / f_y amplifies"""
    f = forward([np.asarray(c, dtype=np.float64) for c in cores], l, X.astype(np.float64))
    return float(np.abs(f[y, np.arange(len(y))]).min() / np.abs(f).max())


def deviation(G, Gref):
    """max |G - Gref| over all cores, relative to max |Gref| over all cores"""
    return max(float(np.abs(g - r).max()) for g, r in zip(G, Gref)) / max(float(np.abs(r).max()) for r in Gref)


def emulation_figures(lc):
    """{objective: (gradient deviation, value deviation)} of the float32 emulation against float64 on one case"""
    cores, l, lev, lab, X, S = build_likelihood_case(lc)
    out = {}
    for name, y in (('joint', lab), ('marginal', None)):
        G64, v64, _ = nll_gradient(cores, l, X, y, S)
        G32, v32, _ = nll_gradient(cores, l, X, y, S, dtype=np.float32)
        out[name] = (deviation(G32, G64), abs(v32 - v64) / max(1.0, abs(v64)))
    return out


# The worst deviation of the float32 emulation from float64 per row (D, cap, L) and objective over the cases of likelihood_cases():
# (gradient, of max|G| over the case; value, of max(1, |nll|)).  tests/test_nll_host.py asserts that the code still gives these figures
# (within a quarter: einsum's summation order follows the host's vector width); the bounds of tests/test_nll_gpu.py are read from here.
EMULATION = {
    (2, 5, 3): {'joint': (1.049e-06, 7.503e-08), 'marginal': (1.106e-06, 8.041e-08)},
    (2, 33, 2): {'joint': (1.810e-06, 5.216e-07), 'marginal': (2.526e-06, 5.215e-07)},
    (2, 64, 2): {'joint': (2.238e-06, 1.341e-07), 'marginal': (2.297e-06, 1.515e-07)},
    (2, 50, 10): {'joint': (2.892e-06, 2.300e-07), 'marginal': (5.286e-06, 4.234e-07)},
    (3, 7, 3): {'joint': (1.611e-06, 1.029e-07), 'marginal': (4.204e-06, 1.554e-07)},
    (8, 16, 17): {'joint': (1.051e-06, 5.755e-07), 'marginal': (1.090e-06, 8.131e-07)},
    'long': {'joint': (6.941e-06, 3.707e-08), 'marginal': (6.403e-06, 3.748e-08)},      # build_long_case, its own row
}


def round_up_one_digit(v):
    e = math.floor(math.log10(v))
    return math.ceil(v / 10.0 ** e - 1e-9) * 10.0 ** e


def gpu_bounds(row, objective):
    """(gradient bound, value bound) of a row on the device: ten times the emulation's worst figure, rounded up to one digit.  The
    factor ten is for the summation order (MFMA k-steps of four on the device, einsum in the emulation), the one thing the emulation
    does not share with the kernels."""
    g, v = EMULATION[row if isinstance(row, str) else tuple(row)][objective]
    return round_up_one_digit(10.0 * g), round_up_one_digit(10.0 * v)


LONG_CASE = (2, 10, 2, 784, 391)                 # (D, bond, L, N, l): one long calibrated chain, b = 64


def build_long_case():
    """(cores, l, levels, labels, X, S): N = 784, bond 10, L = 2, calibrated, 64 images drawn from the chain itself"""
    D, cap, L, N, l = LONG_CASE
    rng = np.random.default_rng([27, N, cap])
    Xc = oref.features(rng, 16, N, D)
    cores = make_cores(N, D, L, [cap] * (N - 1), l, rng, Xc)
    _, phi, w = grid(K, D)
    lev, lab, _, _ = walk(cores, l, phi, w, np.full(64, -1), rng.random((64, N + 1)))
    return cores, l, lev, lab, phi[lev].astype(np.float32), gram(phi, w)


def long_emulation_figures():
    cores, l, lev, lab, X, S = build_long_case()
    out = {}
    for name, y in (('joint', lab), ('marginal', None)):
        G64, v64, _ = nll_gradient(cores, l, X, y, S)
        G32, v32, _ = nll_gradient(cores, l, X, y, S, dtype=np.float32)
        out[name] = (deviation(G32, G64), abs(v32 - v64) / max(1.0, abs(v64)))
    return out


def identity_residuals(cores, l, X, y, G):
    """(per site, of all sites): max_i |sum(G_i A_i)| / sum|Gd_i A_i| over the site's own elements, and max_i |sum(G_i A_i)| over
    the sum of sum|Gd_i A_i| over every site; Gd in float64"""
    Xd = np.asarray(X, dtype=np.float64)
    cot, _ = cotangent(forward(cores, l, Xd), y)
    Gd, _ = core_grad_reference(cores, l, Xd, cot)
    scales = [float(np.abs(gd * c).sum()) for gd, c in zip(Gd, cores)]
    res = [abs(float((np.asarray(g, dtype=np.float64) * c).sum())) for g, c in zip(G, cores)]
    return max(r / s for r, s in zip(res, scales)), max(res) / sum(scales)


def identity_emulation_figure(lc):
    """the worst per-site residual of sum(G_i A_i) = 0 of the float32 emulation on one case, over both objectives"""
    cores, l, lev, lab, X, S = build_likelihood_case(lc)
    return max(identity_residuals(cores, l, X, y, nll_gradient(cores, l, X, y, S, dtype=np.float32)[0])[0] for y in (lab, None))


# sum(G_i A_i) = 0 per site.  G = Gd - Gz is a float32 difference of two gradients whose products with A_i both sum to 2, and Gd
# carries the float32 rounding of two chains of up to N sites and of a sum over b samples, not one rounding of its output: against the
# elements of the one site, sum|Gd_i A_i|, a bound of 2^-22 = 2.4e-7 is out of float32's reach -- the emulation itself leaves the
# residuals below, the worst per row (D, cap, L) over the cases of likelihood_cases() and both objectives.  tests/test_nll_host.py
# asserts that the code still gives them (within a quarter); tests/test_nll_gpu.py asserts ten times the figure, rounded up to one digit.
IDENTITY_EMULATION = {
    (2, 5, 3): 3.620e-07,
    (2, 33, 2): 3.216e-07,
    (2, 64, 2): 2.297e-07,
    (2, 50, 10): 2.347e-07,
    (3, 7, 3): 4.227e-07,
    (8, 16, 17): 7.221e-07,
}


def identity_bound(row):
    return round_up_one_digit(10.0 * IDENTITY_EMULATION[tuple(row)])
