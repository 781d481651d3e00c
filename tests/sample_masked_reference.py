"""Sampling and scoring given ANY set of known pixels in float64 NumPy (test infrastructure): the statement of
tnml_sample_masked in include/tnml.h, on top of tests/sample_reference.py.  Per sample the metric environments from the right with
w_k phi_k phi_k^T in place of S on the known sites and the exponents of the power-of-two rescales summed, then the walk of
sample_reference with the sample's own environments; a dense enumeration of marginals and conditionals for short chains; the mask
generators and the shared cases of tests/test_sample_masked_host.py and tests/test_sample_masked_gpu.py.

mask (n, N) bool, known (n, N) levels (read where the mask is set), classes (n,) with -1 = the label summed / drawn."""
import itertools
import math

import numpy as np

import sample_reference as S

LN2 = math.log(2.0)


def site_metric(phi, w, Sg, known):
    """S_{s,i}: w_k phi_k phi_k^T on a known site (known >= 0), S on a free one"""
    return Sg if known < 0 else w[known] * np.outer(phi[known], phi[known])


def environments(cores, l, phi, w, Sg, q, mask, known):
    """(R[0 .. N], E) of one sample: R[i] rescaled by 2^-k per site, E = log R[0] + ln2 sum k (-inf where R[0] <= 0)"""
    N = len(cores)
    R = [None] * (N + 1)
    R[N] = np.ones((1, 1))
    ex = 0
    for i in range(N - 1, -1, -1):
        Sm = site_metric(phi, w, Sg, int(known[i]) if mask[i] else -1)
        C = cores[i]
        if i == l:
            C = C if q < 0 else C[..., q:q + 1]
            E = np.einsum('de,adcl,cf,befl->ab', Sm, C, R[i + 1], C, optimize=True)
        else:
            E = np.einsum('de,adc,cf,bef->ab', Sm, C, R[i + 1], C, optimize=True)
        m = np.abs(E).max()
        if m > 0:
            _, e = np.frexp(m)
            E = np.ldexp(E, -int(e))
            ex += int(e)
        R[i] = E
    r0 = R[0][0, 0]
    return R, (math.log(r0) + ex * LN2) if r0 > 0 else -math.inf


def normalisers(cores, l, phi, w, classes_needed):
    """{q: E of the empty mask of class slot q}"""
    cores = [np.asarray(c, dtype=np.float64) for c in cores]
    N = len(cores)
    Sg = S.gram(phi, w)
    none = np.zeros(N, dtype=bool)
    return {int(q): environments(cores, l, phi, w, Sg, int(q), none, none.astype(int))[1] for q in classes_needed}


def class_log_weights(cores, l, phi, w):
    """log P(c) = E_{empty,c} - E_{empty,-1}"""
    L = cores[l].shape[3]
    nz = normalisers(cores, l, phi, w, range(-1, L))
    return np.array([nz[c] - nz[-1] for c in range(L)])


def masked_walk(cores, l, phi, w, classes, u, mask, known, draw=True):
    """-> (levels (n, N) int32, labels (n,) int32, logp (n, 2), margins (n, N + 1)).  logp[:, 0] = log p(drawn | known [, class]),
    logp[:, 1] = log p(known [| class]); margins inf where nothing was drawn.  draw=False: the environments only."""
    cores = [np.asarray(c, dtype=np.float64) for c in cores]
    classes = np.asarray(classes, dtype=np.int64)
    n, N = len(classes), len(cores)
    mask = np.broadcast_to(np.asarray(mask, dtype=bool), (n, N))
    known = np.zeros((n, N), dtype=np.int64) if known is None else np.asarray(known, dtype=np.int64)
    Sg = S.gram(phi, w)
    levels = np.where(mask, known, 0).astype(np.int32)
    labels = classes.astype(np.int32).copy()
    logp = np.zeros((n, 2))
    margins = np.full((n, N + 1), np.inf)
    norm = normalisers(cores, l, phi, w, sorted(set(int(c) for c in classes)))
    for s in range(n):
        q = int(classes[s])
        R, E = environments(cores, l, phi, w, Sg, q, mask[s], known[s])
        logp[s, 1] = E - norm[q]
        if not draw:
            continue
        v = np.ones(1)
        lab = q
        for i in range(N):
            if i == l:
                U4 = np.einsum('a,adcl->dcl', v, cores[i])
                if q < 0:
                    Sm = site_metric(phi, w, Sg, int(known[s, i]) if mask[s, i] else -1)
                    Ql = np.einsum('dcl,ce,fel->ldf', U4, R[i + 1], U4, optimize=True)
                    P = np.maximum(0.0, np.einsum('df,ldf->l', Sm, Ql))
                    k, tot, mg = S._draw(P[None], u[s:s + 1, N])
                    lab = int(k[0])
                    margins[s, N] = mg[0]
                    logp[s, 0] += math.log(P[lab] / tot[0])
                    labels[s] = lab
                U = U4[:, :, lab]
            else:
                U = np.einsum('a,adc->dc', v, cores[i])
            if mask[s, i]:
                k = int(known[s, i])
            else:
                Q = U @ R[i + 1] @ U.T
                p = np.maximum(0.0, w * np.einsum('kd,df,kf->k', phi, Q, phi))
                kk, tot, mg = S._draw(p[None], u[s:s + 1, i])
                k = int(kk[0])
                margins[s, i] = mg[0]
                logp[s, 0] += math.log(p[k] / tot[0])
            levels[s, i] = k
            v = phi[k] @ U
            mx = np.abs(v).max()
            if mx > 0:
                _, e = np.frexp(mx)
                v = np.ldexp(v, -int(e))
    return levels, labels, logp, margins


# ---------------------------------------------------------------------------------------------------------------
# dense enumeration (N <= 6)
# ---------------------------------------------------------------------------------------------------------------
def dense_marginal(P, mask, known, q):
    """p(known levels [| class q]) from the joint table P[k_0 .. k_{N-1}, l] of sample_reference.dense_joint"""
    N = P.ndim - 1
    Pq = P.sum(-1) if q < 0 else P[..., q] / P[..., q].sum()
    return Pq[tuple(int(known[i]) if mask[i] else slice(None) for i in range(N))].sum()


def dense_completion(P, mask, known, q, levels, label):
    """p(levels [, label] | known levels [, class q]) of a completed sample"""
    full = P[tuple(int(k) for k in levels)][int(label)] if q < 0 else (P[..., q] / P[..., q].sum())[tuple(int(k) for k in levels)]
    return full / dense_marginal(P, mask, known, q)


def dense_posterior(P, mask, known):
    """P(c | known levels), (L,)"""
    N = P.ndim - 1
    j = P[tuple(int(known[i]) if mask[i] else slice(None) for i in range(N))]
    j = j.reshape(-1, P.shape[-1]).sum(axis=0)
    return j / j.sum()


def all_masks(N):
    return [np.array(b, dtype=bool) for b in itertools.product([0, 1], repeat=N)]


# ---------------------------------------------------------------------------------------------------------------
# mask generators and shared cases
# ---------------------------------------------------------------------------------------------------------------
DENSITIES = (0.0, 0.3, 0.7, 1.0)


def random_masks(rng, n, N):
    """per-sample masks of density DENSITIES[s % 4]"""
    dens = np.array(DENSITIES)[np.arange(n) % 4]
    return rng.random((n, N)) < dens[:, None]


def ragged_inputs(ci, case):
    """(per-sample masks (n, N), one shared mask (N,), known (n, N)) of the ci-th case of sample_reference.draw_cases()"""
    N, D, L, l, K = case
    rng = np.random.default_rng([31, ci])
    mask = random_masks(rng, S.N_DRAWS, N)
    known = rng.integers(0, K, (S.N_DRAWS, N))
    shared = rng.random(N) < 0.5
    return mask, shared, known.astype(np.int32)


def wide_inputs(case):
    """(suffix mask (N,), random masks (n, N), known (n, N)) of a case of sample_reference.wide_cases()"""
    N, D, L, l, M, K = case
    rng = np.random.default_rng([32, M])
    suffix = np.arange(N) >= N // 2
    return suffix, random_masks(rng, S.N_DRAWS, N), rng.integers(0, K, (S.N_DRAWS, N)).astype(np.int32)


LONG_N = 8
LONG_CLASSES = np.array([-1, 0, 1, -1] * 2, dtype=np.int32)


def long_inputs():
    """{name: mask (784,)} and known (8, 784) for the N = 784 chains: levels in the middle of the grid"""
    rng = np.random.default_rng(7)
    N = 784
    site = np.arange(N)
    masks = {'bottom': site >= N // 2, 'checker': site % 2 == 0, 'random': rng.random(N) < 0.5, 'empty': np.zeros(N, dtype=bool)}
    return masks, rng.integers(100, 156, (LONG_N, N)).astype(np.int32)


# frequencies: (N, K, D, L, l, known sites)
FREQ_MASKED = [(4, 3, 2, 2, 2, (1, 3)), (4, 2, 2, 2, 3, (3,))]
