"""The yardstick of test_svd_split_gpu.py, checked without a device: both numpy references pass every metric of
svd_split_reference.py on every family, shape and cut under the tightest cap the device tests use; every mutant of a correct split
misses at least one metric under the loosest cap; and the quantity the in-LDS kernel compares with its Cholesky threshold lies well
away from that threshold for the families whose counter the device tests assert."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import svd_split_reference as sr

TIGHT, LOOSE = 5e-6, 1e-3         # set_svd_stop(1e-8) and set_svd_stop(1e-4) in test_svd_split_gpu.py


def test_thresholds_match_the_kernel_constants():
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'tensornetworkforml_amd', 'csrc',
                            'tnml_internal.h')).read()
    val = {k: float(v) for k, v in re.findall(r'constexpr double (kCholThr\w+) = ([0-9.eE+-]+);', src)}
    assert val == {'kCholThrDefault': sr.CHOL_THR_DEFAULT, 'kCholThrSmall': sr.CHOL_THR_SMALL}


def test_families_are_what_they_claim():
    for rows, cols in sr.ALL_SHAPES:
        n = min(rows, cols)
        for name in sr.FAMILIES:
            A = sr.make(name, rows, cols)
            assert A.dtype == np.float32 and A.shape == (rows, cols) and np.isfinite(A).all(), (name, rows, cols)
        # perm_diag: both Gram matrices exactly diagonal, singular values = the sorted absolute entries
        A = sr.make('perm_diag', rows, cols).astype(np.float64)
        for G in (A @ A.T, A.T @ A):
            assert np.count_nonzero(G - np.diag(np.diag(G))) == 0
        assert sr.chol_ratio(A) == 0.0
        assert np.array_equal(np.sort(np.abs(A[A != 0]))[::-1], np.sort(np.ldexp(1.0, -(np.arange(n) % 7)))[::-1])
        # dup_rows: exactly dup_rank(n) distinct rows
        A = sr.make('dup_rows', rows, cols)
        assert len({r.tobytes() for r in A}) == sr.dup_rank(n)
        assert np.linalg.matrix_rank(A.astype(np.float64)) == sr.dup_rank(n)
        # the scaled families are exact power-of-two multiples of gauss at the same seed
        g = sr.make('gauss', rows, cols)
        assert np.array_equal(sr.make('scaled_up', rows, cols), np.ldexp(g, 40))
        assert np.array_equal(sr.make('scaled_down', rows, cols), np.ldexp(g, -40))
        # the cuts of clusters: one at a plateau edge, one inside a plateau
        s = sr.cluster_spectrum(n)
        edge, inside = sr.cluster_cuts(n)
        assert edge == n or s[edge - 1] > s[edge]
        assert (inside is None) == (n <= 4) and (inside is None or s[inside - 1] == s[inside])


@pytest.mark.parametrize('ref', [sr.ref64, sr.ref32], ids=['ref64', 'ref32'])
def test_references_pass_every_metric(ref):
    worst = {}
    for rows, cols in sr.ALL_SHAPES:
        n = min(rows, cols)
        for name in sr.FAMILIES:
            A = sr.make(name, rows, cols)
            s64 = sr.lapack64(A)
            for m in sr.kept_ranks(name, n):
                US, SVh, sig = ref(A, m)
                mt = sr.metrics(A, US, SVh, sig, m, s64)
                for k in ('e_sig', 'e_all', 'e_opt', 'e_gram'):
                    worst[k] = max(worst.get(k, 0.0), abs(mt[k]))
                if mt['gapped']:
                    worst['e_best'] = max(worst.get('e_best', 0.0), mt['e_best'])
                assert not sr.failures(mt, TIGHT), (name, rows, cols, m, mt)
    print(ref.__name__, {k: '%.1e' % v for k, v in worst.items()})
    assert set(worst) == {'e_sig', 'e_all', 'e_opt', 'e_gram', 'e_best'}


# ---- mutants -------------------------------------------------------------------------------------------------------------
def _balance_lost(US, SVh, sig, S0, m):
    r = np.sqrt(sig[:m])
    return US * r, SVh / r[:, None], sig


def _last_column_zeroed(US, SVh, sig, S0, m):
    US = US.copy()
    US[:, m - 1] = 0.0
    return US, SVh, sig


def _columns_swapped_in_one_factor(US, SVh, sig, S0, m):
    US = US.copy()
    US[:, [0, m - 1]] = US[:, [m - 1, 0]]
    return US, SVh, sig


def _sign_flipped_in_one_factor(US, SVh, sig, S0, m):
    SVh = SVh.copy()
    SVh[m - 1] *= -1.0
    return US, SVh, sig


def _sigma_exchanged(US, SVh, sig, S0, m):
    sig = sig.copy()
    sig[[0, m - 1]] = sig[[m - 1, 0]]
    return US, SVh, sig


def _sigma_shifted(US, SVh, sig, S0, m):
    return US, SVh, sig + 2e-3 * S0


def _one_nan(US, SVh, sig, S0, m):
    SVh = SVh.copy()
    SVh[0, 0] = np.nan
    return US, SVh, sig


MUTANTS = [_balance_lost, _last_column_zeroed, _columns_swapped_in_one_factor, _sign_flipped_in_one_factor, _sigma_exchanged,
           _sigma_shifted, _one_nan]

# (family, rows, cols, m): each with S[m-1] > 1e-2 S0, m >= 2 and, but for the plateau of `clusters`, S[0] > S[m-1]
MUTANT_CASES = [('gauss', 20, 40, 10), ('gauss', 80, 40, 40), ('clusters', 40, 80, 10), ('clusters', 40, 80, 15),
                ('graded1e6', 6, 6, 2), ('dup_rows', 64, 128, 21), ('scaled_up', 27, 27, 13), ('scaled_down', 9, 15, 4),
                ('perm_diag', 42, 84, 21)]


@pytest.mark.parametrize('mutant', MUTANTS, ids=[f.__name__.lstrip('_') for f in MUTANTS])
def test_mutants_fail(mutant):
    for name, rows, cols, m in MUTANT_CASES:
        A = sr.make(name, rows, cols)
        s64 = sr.lapack64(A)
        S = s64[1]
        assert S[m - 1] > 1e-2 * S[0]
        US, SVh, sig = sr.ref64(A, m)
        assert not sr.failures(sr.metrics(A, US, SVh, sig, m, s64), TIGHT)
        if mutant is _sigma_exchanged and S[0] == pytest.approx(S[m - 1], rel=1e-3):
            continue                               # inside one plateau there is nothing to exchange
        mt = sr.metrics(A, *mutant(US, SVh, sig, S[0], m), m, s64)
        assert sr.failures(mt, LOOSE), (mutant.__name__, name, rows, cols, m, mt)


def test_balance_mutant_needs_a_scale_other_than_one():
    """(U S, Vh) is caught through e_gram unless every kept value is 1: the families hold values away from 1 on purpose."""
    A = sr.make('gauss', 20, 40)
    US, SVh, sig = sr.ref64(A, 5)
    assert 'e_gram' in sr.failures(sr.metrics(A, *_balance_lost(US, SVh, sig, sig[0], 5), 5), LOOSE)


# ---- the Cholesky decision is not on its threshold ----------------------------------------------------------------------------
def test_cholesky_ratio_separates_the_families():
    lo, hi = {}, {}
    for rows, cols in sr.SHAPES_LDS:
        n = min(rows, cols)
        thr = sr.chol_threshold(n)
        for name in ('graded1e6', 'rank1_plus_noise'):
            if n > 4:
                q = sr.chol_ratio(sr.make(name, rows, cols)) / thr
                hi[name] = min(hi.get(name, np.inf), q)
                assert q >= 1.5, (name, rows, cols, q)
        for name in ('perm_diag', 'near_equal', 'gauss'):
            if name == 'gauss' and n < 20:
                continue
            q = sr.chol_ratio(sr.make(name, rows, cols)) / thr
            lo[name] = max(lo.get(name, 0.0), q)
            assert q <= 0.6, (name, rows, cols, q)
    print('ratio / threshold: at least', {k: round(v, 2) for k, v in hi.items()}, 'at most', {k: round(v, 2) for k, v in lo.items()})


# ---- the CPU emulation of the D = 2 kernels still shows the two defects it was written for -------------------------------------
def test_emulation_shows_both_defects():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'emulation'))
    import jacobi_annihilated_element_emulation as em

    def run(name, rows, cols, m, **kw):
        A = sr.make(name, rows, cols)
        US, SVh, sig, _, chol = em.split(A, m, **kw)
        return sr.metrics(A, US, SVh, sig, m), chol

    # exact zero written for the annihilated element: an exactly zero singular value comes out near 1e-4 S0, without it near 1e-8
    assert run('dup_rows', 20, 40, 7, chol=False, zero=True)[0]['e_sig'] > 5e-5
    assert run('dup_rows', 20, 40, 7, chol=False, zero=False)[0]['e_sig'] < 1e-6
    # eigenvectors made of rounding noise, normalised by the Cholesky back-transform: e_gram far above the cap, zeroed: under it
    mt, chol = run('dup_rows', 40, 80, 40, zero=True, vfloor=1e-300)
    assert chol and mt['e_gram'] > 1e-3
    mt, chol = run('dup_rows', 40, 80, 40, zero=True)
    assert chol and mt['e_gram'] < 5e-5
