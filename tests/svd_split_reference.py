"""Constructed matrices, error metrics and plain numpy references for the SVD split (tnml_svd_split: U sqrt(S), sqrt(S) Vh, all
singular values).  Shared by test_svd_split_host.py and test_svd_split_gpu.py.

A family is a function of (rows, cols, rng) that returns a float32 matrix; n = min(rows, cols) throughout.  Every metric is
relative to S0, the largest singular value float64 LAPACK finds for the float32 input, and every metric is well defined where the
best rank-m product is not unique (equal singular values across the cut).
"""
import numpy as np

# off(G) / trace(G) above which kernels_narrow.hip takes the pivoted-Cholesky step (tnml_internal.h: kCholThrDefault for n >= 32,
# kCholThrSmall below); never at n <= 4
CHOL_THR_DEFAULT = 0.22
CHOL_THR_SMALL = 0.35

# rows x cols per kernel (the in-LDS and HBM-resident kernels at D = 2, the generic-D kernel at D = 3).  n = 2: the pair meets
# itself; n = 4: no Cholesky step; n = 40 / 42: one / two eigenvector blocks per lane; 80 x 40: short side on the columns.
# 64 x 128 does not fit the in-LDS kernel (narrow_carve: four 64 x 64 float64 buffers and two float32 copies of the matrix alone
# are 192 KB of the 160 KB a workgroup has), so the automatic choice hands it -- and every other n = 64 matrix, 64 x 64 too -- to
# the HBM-resident kernel; the Cholesky counter of test_svd_split_gpu.py shows which kernel ran.
SHAPES_LDS = [(2, 2), (4, 40), (6, 6), (20, 40), (40, 80), (42, 84), (80, 40)]
SHAPES_BIG_FORCED = [(20, 40), (40, 80)]          # under set_narrow_path(1)
SHAPES_BIG_AUTO = [(64, 128), (100, 200), (128, 128)]
SHAPES_ANYD = [(9, 15), (27, 27), (21, 9), (105, 120)]
ALL_SHAPES = sorted(set(SHAPES_LDS + SHAPES_BIG_FORCED + SHAPES_BIG_AUTO + SHAPES_ANYD))

CLUSTER_LEVELS = (4.0, 2.0, 1.0, 0.5)


def chol_threshold(n):
    return CHOL_THR_DEFAULT if n >= 32 else CHOL_THR_SMALL


# ---- families -------------------------------------------------------------------------------------------------------
def _orthonormal(k, n, rng):
    """k x n with orthonormal columns (k >= n), float64."""
    q, r = np.linalg.qr(rng.standard_normal((k, n)))
    return q * np.sign(np.diag(r))


def with_spectrum(rows, cols, s, rng):
    """orthonormal x diag(s) x orthonormal, rounded to float32."""
    n = min(rows, cols)
    s = np.asarray(s, np.float64)
    assert s.shape == (n,)
    return ((_orthonormal(rows, n, rng) * s) @ _orthonormal(cols, n, rng).T).astype(np.float32)


def gauss(rows, cols, rng):
    return rng.standard_normal((rows, cols)).astype(np.float32)


def graded1e6(rows, cols, rng):
    return with_spectrum(rows, cols, np.logspace(0, -6, min(rows, cols)), rng)


def flat_then_drop(rows, cols, rng):
    n = min(rows, cols)
    return with_spectrum(rows, cols, np.where(np.arange(n) < (n + 1) // 2, 1.0, 1e-3), rng)


def cluster_spectrum(n):
    return np.array([CLUSTER_LEVELS[(4 * k) // n] for k in range(n)])


def clusters(rows, cols, rng):
    return with_spectrum(rows, cols, cluster_spectrum(min(rows, cols)), rng)


def cluster_cuts(n):
    """(m at the first plateau edge, m one inside a plateau or None where no plateau has two members)."""
    s = cluster_spectrum(n)
    edge = next(m for m in range(1, n + 1) if m == n or s[m - 1] != s[m])
    inside = next((m for m in range(1, n) if s[m - 1] == s[m]), None)
    return edge, inside


def near_equal(rows, cols, rng):
    n = min(rows, cols)
    return with_spectrum(rows, cols, (1.0 + 1e-6 * np.arange(n))[::-1], rng)


def perm_diag(rows, cols, rng):
    """One entry +-2^-(k mod 7) per index k of the short side, at a random permutation of the long side: both Gram matrices are
    exactly diagonal, and for n > 7 the singular values repeat exactly."""
    n, long_ = min(rows, cols), max(rows, cols)
    at = rng.permutation(long_)[:n]
    val = np.ldexp(1.0, -(np.arange(n) % 7)) * rng.choice([-1.0, 1.0], n)
    A = np.zeros((rows, cols), np.float32)
    if rows <= cols:
        A[np.arange(n), at] = val
    else:
        A[at, np.arange(n)] = val
    return A


def dup_rank(n):
    return max(1, n // 3)


def dup_rows(rows, cols, rng):
    """k = dup_rank(n) Gaussian rows, every other row an exact copy of one of them: rank exactly k, G not diagonal."""
    k = dup_rank(min(rows, cols))
    base = rng.standard_normal((k, cols)).astype(np.float32)
    src = np.concatenate([np.arange(k), rng.integers(0, k, rows - k)])
    return np.ascontiguousarray(base[src])


def rank1_plus_noise(rows, cols, rng):
    u, v = rng.standard_normal(rows), rng.standard_normal(cols)
    return (np.outer(u, v) + 1e-3 * rng.standard_normal((rows, cols))).astype(np.float32)


def scaled_up(rows, cols, rng):
    return np.ldexp(gauss(rows, cols, rng), 40)


def scaled_down(rows, cols, rng):
    return np.ldexp(gauss(rows, cols, rng), -40)


FAMILIES = {f.__name__: f for f in (gauss, graded1e6, flat_then_drop, clusters, near_equal, perm_diag, dup_rows,
                                    rank1_plus_noise, scaled_up, scaled_down)}


def make(family, rows, cols, seed=0):
    """The matrix of a family at a shape: the generator is seeded by (seed, rows, cols) alone, so that scaled_up / scaled_down are
    exact power-of-two multiples of gauss at the same seed and shape."""
    return FAMILIES[family](rows, cols, np.random.default_rng([seed, rows, cols]))


def kept_ranks(family, n):
    """The cuts m every test takes for a family at short side n: 1, n // 2, n, and the family's own edges."""
    ms = {1, max(1, n // 2), n}
    if family == 'clusters':
        ms.update(m for m in cluster_cuts(n) if m is not None)
    if family == 'dup_rows':
        ms.update(m for m in (dup_rank(n), dup_rank(n) + 1) if m <= n)
    return sorted(ms)


# ---- the quantity the Cholesky decision compares with its threshold --------------------------------------------------------
def chol_ratio(A):
    """sqrt(sum_{i != j} G_ij^2) / trace(G) of the float64 Gram matrix of the short side (both triangles)."""
    A = np.asarray(A, np.float64)
    G = A @ A.T if A.shape[0] <= A.shape[1] else A.T @ A
    off = G - np.diag(np.diag(G))
    return float(np.sqrt((off * off).sum()) / np.trace(G))


# ---- metrics -----------------------------------------------------------------------------------------------------------
GAP_MIN = 1e-2            # e_best is asserted only where (S[m-1] - S[m]) / S0 is at least this


def lapack64(A):
    return np.linalg.svd(np.asarray(A, np.float64), full_matrices=False)


def metrics(A, US, SVh, sig, m, svd64=None):
    """dict of e_sig, e_all, e_opt, e_gram, e_best (all over S0), `gapped` (whether e_best is to be asserted), `finite` and
    `sorted`.  svd64: lapack64(A) where the caller has it already."""
    A = np.asarray(A, np.float64)
    U, S, Vh = svd64 if svd64 is not None else lapack64(A)
    n, S0 = S.size, S[0]
    US, SVh, sig = np.asarray(US, np.float64), np.asarray(SVh, np.float64), np.asarray(sig, np.float64)
    assert US.shape == (A.shape[0], m) and SVh.shape == (m, A.shape[1]) and sig.shape == (n,)
    out = {'finite': bool(np.isfinite(US).all() and np.isfinite(SVh).all() and np.isfinite(sig).all()),
           'sorted': bool((np.diff(sig) <= 0).all())}
    if not out['finite']:
        out.update(e_sig=np.inf, e_all=np.inf, e_opt=np.inf, e_gram=np.inf, e_best=np.inf, gapped=True)
        return out
    prod = US @ SVh
    out['e_sig'] = float(np.abs(sig[:m] - S[:m]).max() / S0)
    out['e_all'] = float(np.abs(sig - S).max() / S0)
    out['e_opt'] = float((np.linalg.norm(A - prod) - np.sqrt((S[m:] ** 2).sum())) / S0)
    d = np.diag(sig[:m])
    out['e_gram'] = float(max(np.abs(US.T @ US - d).max(), np.abs(SVh @ SVh.T - d).max()) / S0)
    out['e_best'] = float(np.abs(prod - (U[:, :m] * S[:m]) @ Vh[:m]).max() / S0)
    out['gapped'] = bool((S[m - 1] - (S[m] if m < n else 0.0)) / S0 >= GAP_MIN)
    return out


def failures(mt, cap, cap_all=None):
    """Names of the checks a metrics dict misses under `cap` (e_all under cap_all, default cap)."""
    bad = [k for k in ('finite', 'sorted') if not mt[k]]
    bad += [k for k in ('e_sig', 'e_opt', 'e_gram') if not abs(mt[k]) < cap]
    if not mt['e_all'] < (cap if cap_all is None else cap_all):
        bad.append('e_all')
    if mt['gapped'] and not mt['e_best'] < cap:
        bad.append('e_best')
    return bad


# ---- references ----------------------------------------------------------------------------------------------------------
def ref64(A, m):
    """(U sqrt(S), sqrt(S) Vh, S) from float64 LAPACK."""
    U, S, Vh = lapack64(A)
    r = np.sqrt(S[:m])
    return U[:, :m] * r, r[:, None] * Vh[:m], S


def ref32(A, m):
    """The same from np.linalg.svd on the float32 array, split in float32."""
    U, S, Vh = np.linalg.svd(np.asarray(A, np.float32), full_matrices=False)
    assert U.dtype == np.float32
    r = np.sqrt(S[:m])
    return U[:, :m] * r, r[:, None] * Vh[:m], S
