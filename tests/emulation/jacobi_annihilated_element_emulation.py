"""CPU emulation (development aid) of the SVD split of the D = 2 kernels on the constructed spectra of tests/svd_split_reference.py:
float64 Gram matrix scaled by a power of two, optional pivoted-Cholesky step, two-sided Jacobi in position space with float32
rotation parameters, the sliding-window stop, factors q sqrt(sigma) and W q / sqrt(sigma) rounded to float32.  It is no bit-level
model: rotation parameters come from the current matrix, not from the kernels' float32 look-ahead, and hardware rcp / rsq / sqrt are
exact here.  It shows the same misses of the same size as the device at n >= 6 (tests/test_svd_split_gpu.py: e.g. e_gram 9.3e-5
at 6x6 flat_then_drop, e_sig 1.4e-4 for exact zeros, e_opt 5.8e-5 at 128x128 near_equal) and differs from it at n <= 4.  Kept
honest by tests/test_svd_split_host.py::test_emulation_shows_both_defects.  It shows what two details of the kernels cost:

  zero=True     the annihilated element of a diagonal block is written as an exact 0 (both kernels did; the in-LDS one still does).
                The tangent is a float32 number, so the rotation leaves ~1e-7 of the element; discarding it is no similarity
                transform, and every small eigenvalue moves by ~2e-8 lambda_max: singular values below 1e-4 sigma_max come out
                wrong, exact zeros as 1.5e-4.
  vfloor=1e-300 the Cholesky step goes on factorising once the remaining diagonal is rounding noise, and the back-transform divides
                L u by the square root of ANY positive eigenvalue (as the kernel did): for an eigenvalue made of that noise the result
                is a unit vector in no particular direction.  The kernel now zeroes such columns (eigenvalue <= 1e-15 trace).

What remains with zero=False, vfloor=1e-15 is listed in DESIGN.md 5.3, "Constructed spectra".

    python tests/emulation/jacobi_annihilated_element_emulation.py            (about half a minute)
"""
import os as _os, sys as _sys
_HERE = _os.path.dirname(_os.path.abspath(__file__))
_sys.path.insert(0, _os.path.dirname(_HERE))

import numpy as np
import svd_split_reference as sr
from jacobi_emulation import pi_perm

f32 = np.float32
KEPT_FRAC, TOL2, ABS2 = 0.2, 1e-14, 1e-30


def pchol(G, pivmin=1e-26):
    """The kernel's pivoted Cholesky: column k of L against the ORIGINAL row index, pivot = largest remaining diagonal entry (float32
    key), stop once it is <= pivmin."""
    n = G.shape[0]; A = G.copy(); L = np.zeros((n, n)); left = np.ones(n, bool); d = np.diag(A).copy()
    for k in range(n):
        key = np.where(left, d.astype(f32), f32(-1)); jp = int(np.argmax(key))
        if not key[jp] > pivmin: break
        inv = 1.0 / np.sqrt(d[jp])
        l = np.where(left, A[jp] * inv, 0.0)
        L[:, k] = l
        A = A - np.outer(A[jp] * inv, A[jp] * inv)
        d = np.where(left, d - l * l, d); left[jp] = False
    return L


def jacobi(G, m, stop2=1e-6, zero=False, maxsweeps=30):
    n = G.shape[0]; G = G.copy(); V = np.eye(n)
    inv = np.argsort(pi_perm(n)); ev = np.arange(0, n, 2); od = ev + 1
    kept2_of = lambda G: max((KEPT_FRAC * max(np.sort(np.diag(G))[::-1][m - 1], 0.0)) ** 2, 1e-36)
    rounds = last_big = 0; kept2 = kept2_of(G)
    while rounds < maxsweeps * (n - 1):
        a, b, g = G[ev, ev].astype(f32), G[od, od].astype(f32), G[ev, od].astype(f32)
        with np.errstate(all='ignore'):
            g2 = g * g; sc = np.maximum(np.abs(a * b), f32(kept2))
            act = g2 > np.maximum(f32(TOL2) * sc, f32(ABS2))
            d = b - a; den = d + np.copysign(np.sqrt(d * d + f32(4) * g2), d)
            t = np.where(act, f32(2) * g / np.where(den == 0, f32(1), den), f32(0)).astype(np.float64)
            big = act & (g2 > f32(stop2) * sc)
        c = 1.0 / np.sqrt(1.0 + t * t); s = c * t
        J = np.eye(n); J[ev, ev] = c; J[od, od] = c; J[ev, od] = s; J[od, ev] = -s
        Gn = J.T @ G @ J
        if zero:
            rot = t != 0; Gn[ev[rot], od[rot]] = 0; Gn[od[rot], ev[rot]] = 0
        Gn = (Gn + Gn.T) * 0.5
        G = Gn[np.ix_(inv, inv)]; V = (V @ J)[:, inv]
        rounds += 1
        if big.any(): last_big = rounds
        if rounds - last_big >= n - 1: break
        if rounds % (n - 1) == 0: kept2 = kept2_of(G)
    return rounds, G, V


def split(A, m, chol=None, vfloor=1e-15, **kw):
    """(US, SVh, sigma, rounds, Cholesky step taken) as tnml_svd_split forms them; chol: None = the kernel's decision."""
    A = np.asarray(A, np.float64)
    short_rows = A.shape[0] <= A.shape[1]
    W = A if short_rows else A.T
    n = W.shape[0]
    G = W @ W.T; e = np.frexp(np.trace(G))[1]; G = np.ldexp(G, -e)
    off2 = (G ** 2).sum() - (np.diag(G) ** 2).sum()
    use_chol = (n > 4 and off2 > (sr.chol_threshold(n) * np.trace(G)) ** 2) if chol is None else chol
    if use_chol:
        L = pchol(G)
        rounds, Gd, V = jacobi(L.T @ L, m, **kw)
        ls = np.diag(Gd); good = ls > vfloor
        V = (L @ V) * np.where(good, 1.0 / np.sqrt(np.where(good, ls, 1.0)), 0.0)
    else:
        rounds, Gd, V = jacobi(G, m, **kw)
    lam = np.ldexp(np.maximum(np.diag(Gd), 0.0), e)
    o = np.argsort(-lam, kind='stable'); lk = lam[o[:m]]
    ok = (lk > 1e-300) & (lk > 1e-30 * lam[o[0]])
    sq = np.where(ok, np.sqrt(np.sqrt(np.where(ok, lk, 1.0))), 0.0); isq = np.where(ok, 1.0 / np.where(ok, sq, 1.0), 0.0)
    Q = V[:, o[:m]]
    shortf, longf = (Q * sq).astype(f32), (W.T @ (Q * isq)).astype(f32)
    return (shortf, longf.T, np.sqrt(lam[o]), rounds, use_chol) if short_rows else (longf, shortf.T, np.sqrt(lam[o]), rounds, use_chol)


def table(name, shapes, families, **kw):
    print('==', name)
    for fam in families:
        worst, where = {}, {}
        for rows, cols in shapes:
            A = sr.make(fam, rows, cols); s64 = sr.lapack64(A)
            for m in sr.kept_ranks(fam, min(rows, cols)):
                US, SVh, sig, rounds, uc = split(A, m, **kw)
                mt = sr.metrics(A, US, SVh, sig, m, s64)
                for k in ('e_sig', 'e_all', 'e_opt', 'e_gram', 'e_best'):
                    if (k != 'e_best' or mt['gapped']) and abs(mt[k]) > worst.get(k, 0.0):
                        worst[k] = abs(mt[k]); where[k] = '%dx%d m=%d%s' % (rows, cols, m, ' chol' if uc else '')
        print('%-16s' % fam, ' '.join('%s %.1e' % (k, worst.get(k, 0.0)) for k in ('e_sig', 'e_all', 'e_opt', 'e_gram', 'e_best')),
              '| e_gram at', where.get('e_gram'), '| e_sig at', where.get('e_sig'))


if __name__ == '__main__':
    fams = [f for f in sr.FAMILIES if not f.startswith('scaled')]
    big = sr.SHAPES_BIG_FORCED + sr.SHAPES_BIG_AUTO[:1]
    table('in-LDS as it was', sr.SHAPES_LDS, fams, zero=True, vfloor=1e-300)
    table('in-LDS as it is (noise eigenvectors zeroed)', sr.SHAPES_LDS, fams, zero=True)
    table('in-LDS without the exact zero', sr.SHAPES_LDS, fams)
    table('HBM-resident (no Cholesky step) as it was', big, fams, chol=False, zero=True)
    table('HBM-resident as it is (no exact zero)', big, fams, chol=False)
    for st in (1e-4, 1e-8):
        table('in-LDS without the exact zero, svd_stop %g' % st, sr.SHAPES_BIG_FORCED, ['gauss', 'clusters', 'graded1e6'], stop2=st)
