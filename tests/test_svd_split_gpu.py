"""The SVD split (Context.svd_split = tnml_svd_split, the code every sweep step runs) on constructed spectra, on all three Jacobi
kernels: the in-LDS workgroup (kernels_narrow.hip), the HBM-resident big_jacobi_kernel with its rotation-log replay, and the
generic-D update kernel (kernels_anyd.hip).  Families, metrics and references: svd_split_reference.py, whose own check is
test_svd_split_host.py.

Caps.  None is derived from what the device returns: with the default stop setting every metric is held to 5e-5, the bound
test_hip_parity.py::test_svd_accuracy_late_in_training holds the same quantities to (1e-3 at set_svd_stop(1e-4), 5e-6 at 1e-8); the
error over ALL singular values keeps the 2e-3 of test_feature_dim_gpu.py (discarded values are only separated from the kept ones).
A float32 LAPACK stays under 1.2e-6 on every case (test_svd_split_host.py).

KNOWN_MISSES lists single checks (one metric at one cut) that miss a cap for a cause written down in DESIGN.md 5.3 ("Constructed
spectra").  Such a case is reported as an expected failure only if exactly those checks miss: any other miss of the case fails it,
and so does a listed check that passes.  The module prints the worst value seen per kernel, family and metric when
it is done; DESIGN.md carries that table.
"""
import contextlib
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import svd_split_reference as sr

pytestmark = pytest.mark.gpu

CAP = {None: 5e-5, 1e-4: 1e-3, 1e-8: 5e-6}       # per set_svd_stop setting (None: the default, 1e-6)
CAP_ALL = 2e-3
STOP_DEFAULT = 1e-6                               # kSvdStop2Default (tnml_internal.h)
METRICS = ('e_sig', 'e_all', 'e_opt', 'e_gram', 'e_best')

# kernel -> (feature dimension, shapes, set_narrow_path)
KERNELS = {
    'lds': (2, sr.SHAPES_LDS, False),
    'big_forced': (2, sr.SHAPES_BIG_FORCED, True),
    'big_auto': (2, sr.SHAPES_BIG_AUTO, False),
    'anyd': (3, sr.SHAPES_ANYD, False),
}

# Known misses, each ONE check at ONE cut: (kernel, (rows, cols), family, stop setting) -> (cause, {(m, check): value observed on the
# MI355X}); causes in DESIGN.md 5.3.  A case listed here must miss exactly these checks and no other -- every other cut, metric and
# counter of the case is asserted as everywhere else, and a listed check that passes is a failure too -- and is then reported as an
# expected failure.
_ZERO = ('the in-LDS kernel writes the annihilated element as an exact 0 although its float32 tangent leaves ~1e-7 of it: no similarity '
         'transform, small eigenvalues move by ~2e-8 lambda_max (fixed in the HBM-resident kernel, where these cases pass): ')
_CHOL = ('after the Cholesky step the back-transform v = L u / sqrt(lambda) multiplies what the iteration leaves of the coupling between '
         'a large and a small eigenvalue by sigma_large / sigma_small: ')
_CLUSTER = ('inside a cluster whose spread is below sqrt(svd_stop2) no rotation counts as big, the window ends after one tournament of '
            'small rotations, and there convergence is only linear: ')
_N2 = ('rank 1 at n = 2: the float32 tangent (v_rcp_f32, v_sqrt_f32) leaves 1e-7 of the annihilated element; the scale that remainder '
       'is compared with is the kept diagonal entry measured BEFORE the first rotation (lambda_1 / 2 where the true lambda_2 is 0), so '
       'it counts as small and the window of ne - 1 = 1 round ends the iteration; over sqrt(sigma_1 sigma_2): ')
KNOWN_MISSES = {
    ('lds', (2, 2), 'dup_rows', None): (_N2, {(2, 'e_gram'): '1.10e-4'}),
    ('lds', (4, 40), 'dup_rows', None): (_ZERO, {(2, 'e_sig'): '8.90e-5', (2, 'e_gram'): '8.90e-5', (4, 'e_sig'): '8.90e-5',
                                                 (4, 'e_gram'): '8.90e-5'}),
    ('lds', (4, 40), 'dup_rows_tail', None): (_ZERO, {(2, 'tail'): '8.05e-3 sqrt(S0)', (4, 'tail'): '8.05e-3 sqrt(S0)'}),
    ('lds', (6, 6), 'flat_then_drop', None): (_CHOL, {(6, 'e_gram'): '8.96e-5'}),
    ('lds', (40, 80), 'graded1e6', None): (_ZERO, {(40, 'e_gram'): '5.53e-5'}),
    ('lds', (40, 80), 'flat_then_drop', None): (_ZERO, {(40, 'e_gram'): '5.82e-5'}),
    ('lds', (40, 80), 'clusters', None): (_ZERO, {(40, 'e_gram'): '6.07e-5'}),
    ('lds', (42, 84), 'graded1e6', None): (_CHOL, {(42, 'e_gram'): '1.03e-4 (5.5e-5 without the exact zero)'}),
    ('lds', (42, 84), 'flat_then_drop', None): (_ZERO, {(42, 'e_gram'): '5.79e-5'}),
    ('lds', (80, 40), 'graded1e6', None): (_ZERO, {(40, 'e_gram'): '5.99e-5'}),
    ('big_auto', (128, 128), 'near_equal', None): (_CLUSTER, {(64, 'e_opt'): '5.83e-5'}),
    ('lds', (20, 40), 'graded1e6', 1e-8): (_CHOL, {(20, 'e_gram'): '1.62e-5'}),
    ('lds', (40, 80), 'graded1e6', 1e-8): (_CHOL, {(40, 'e_gram'): '5.53e-5 (3.5e-5 without the exact zero)'}),
    ('lds', (40, 80), 'clusters', 1e-4): (_CLUSTER, {(40, 'e_gram'): '1.78e-3'}),
    ('big_forced', (40, 80), 'clusters', 1e-4): (_CLUSTER, {(40, 'e_gram'): '1.68e-3'}),
}


def hip():
    from tensornetworkforml_amd import _hip
    return _hip


@pytest.fixture(scope='module')
def contexts():
    """One context per feature dimension, its buffers sized for the largest matrix (D = 2: 32768 elements, D = 3: 18432)."""
    ctxs = {2: hip().Context(4, 2, 2, 64, 64), 3: hip().Context(4, 3, 2, 32, 64)}
    yield ctxs
    for c in ctxs.values():
        c.close()


@pytest.fixture(scope='module')
def table():
    """(kernel, family, stop setting) -> worst value per metric, printed once the module is done."""
    worst = {}
    yield worst
    print('\nworst observed / S0  | ' + ' | '.join('%-7s' % k for k in METRICS))
    for (kernel, family, stop2), w in worst.items():
        print('worst | %-10s | %-16s | stop %-7s | %s' % (kernel, family, stop2 or 'default',
                                                        ' | '.join('%.1e' % w.get(k, 0.0) for k in METRICS)))


@contextlib.contextmanager
def on_kernel(contexts, kernel, stop2=None):
    D, _, force = KERNELS[kernel]
    ctx = contexts[D]
    ctx.set_narrow_path(force)
    if stop2 is not None:
        ctx.set_svd_stop(stop2)
    try:
        yield ctx
    finally:
        ctx.set_narrow_path(False)
        ctx.set_svd_stop(STOP_DEFAULT)


@functools.lru_cache(maxsize=None)
def case(family, rows, cols):
    """(matrix, its float64 LAPACK SVD): computed once, shared by every test, never written to."""
    A = sr.make(family, rows, cols)
    A.setflags(write=False)
    return A, sr.lapack64(A)


def counts(ctx):
    """(SVDs, Cholesky steps) since the context was made."""
    _, svds, _ = ctx.svd_stats(False)
    return int(svds), int(ctx.cholesky_steps)


def expected_cholesky(kernel, family, n):
    """1 / 0 where the decision is far from its threshold (test_svd_split_host.py), None where it is left open."""
    if kernel != 'lds' or n <= 4:
        return 0                                   # only the in-LDS kernel has the step, and never at n <= 4
    if family in ('graded1e6', 'rank1_plus_noise'):
        return 1
    if family in ('perm_diag', 'near_equal') or (family == 'gauss' and n >= 20):
        return 0
    return None


def settle(key, cap_text, missed):
    """missed: {(m, check): text}.  Fails unless it is exactly what KNOWN_MISSES lists for the case (nothing, for most); returns the
    reason of the expected failure, or None."""
    cause, known = KNOWN_MISSES.get(key, ('', {}))
    kernel, (rows, cols), family, _ = key
    where = '%s %dx%d %s (%s): ' % (kernel, rows, cols, family, cap_text)
    new = ['m = %d: %s' % (m, missed[(m, c)]) for (m, c) in sorted(missed) if (m, c) not in known]
    assert not new, where + '; '.join(new)
    gone = ['m = %d: %s (was %s)' % (m, c, known[(m, c)]) for (m, c) in sorted(known) if (m, c) not in missed]
    assert not gone, where + 'listed in KNOWN_MISSES but passing now, take it out: ' + '; '.join(gone)
    return cause + '; '.join('m = %d: %s %s' % (m, c, known[(m, c)]) for (m, c) in sorted(known)) + ' (%s)' % cap_text if known else None


def run_case(contexts, table, kernel, shape, family, stop2=None):
    """Every cut of one family at one shape on one kernel: metrics under the cap of the stop setting, the two counters per call.
    Returns the reason of an expected failure (see KNOWN_MISSES) or None."""
    cap = CAP[stop2]
    rows, cols = shape
    n = min(rows, cols)
    A, s64 = case(family, rows, cols)
    worst = table.setdefault((kernel, family, stop2), {})
    missed = {}
    with on_kernel(contexts, kernel, stop2) as ctx:
        for m in sr.kept_ranks(family, n):
            svd0, chol0 = counts(ctx)
            US, SVh, sig = ctx.svd_split(A, m)
            svd1, chol1 = counts(ctx)
            mt = sr.metrics(A, US, SVh, sig, m, s64)
            for k in METRICS:
                if k != 'e_best' or mt['gapped']:
                    worst[k] = max(worst.get(k, 0.0), abs(mt[k]))
            for k in sr.failures(mt, cap, CAP_ALL):
                missed[(m, k)] = '%s %.2e' % (k, mt[k]) if k.startswith('e_') else k
            if svd1 - svd0 != 1:
                missed[(m, 'svd count')] = 'svd count +%d' % (svd1 - svd0)
            want = expected_cholesky(kernel, family, n)
            if want is not None and chol1 - chol0 != want:
                missed[(m, 'cholesky count')] = 'cholesky count +%d, expected +%d' % (chol1 - chol0, want)
    return settle((kernel, shape, family, stop2), 'cap %g' % cap, missed)


def cases(kernels, families, stops=(None,), shapes=None):
    out = []
    for kernel in kernels:
        for shape in KERNELS[kernel][1]:
            if shapes is not None and shape not in shapes:
                continue
            for family in families:
                for stop2 in stops:
                    ident = '%s-%dx%d-%s' % (kernel, shape[0], shape[1], family) + ('-stop%g' % stop2 if stop2 else '')
                    out.append(pytest.param(kernel, shape, family, stop2, id=ident))
    return out


def test_every_known_miss_belongs_to_a_case():
    keys = {tuple(p.values) for f in (('default', cases(KERNELS, sr.FAMILIES)), ('tail', cases(KERNELS, ['dup_rows_tail'])),
                                      ('stop', cases(('lds', 'big_forced'), ('gauss', 'clusters', 'graded1e6'), (1e-4, 1e-8),
                                                     sr.SHAPES_BIG_FORCED))) for p in f[1]}
    assert set(KNOWN_MISSES) <= keys


# ---- accuracy and counters, default stop setting: one test per kernel, shape and family ---------------------------------
@pytest.mark.parametrize('kernel,shape,family,stop2', cases(KERNELS, sr.FAMILIES))
def test_split_default_stop(contexts, table, kernel, shape, family, stop2):
    known = run_case(contexts, table, kernel, shape, family)
    if known:
        pytest.xfail(known)


# ---- the other stop settings, both D = 2 paths ------------------------------------------------------------------------------
@pytest.mark.parametrize('kernel,shape,family,stop2', cases(('lds', 'big_forced'), ('gauss', 'clusters', 'graded1e6'), (1e-4, 1e-8),
                                                            sr.SHAPES_BIG_FORCED))
def test_split_other_stop_settings(contexts, table, kernel, shape, family, stop2):
    A, _ = case(family, *shape)
    m = min(shape) // 2
    with on_kernel(contexts, kernel) as ctx:
        before = ctx.svd_split(A, m)
    try:
        known = run_case(contexts, table, kernel, shape, family, stop2)
    finally:
        with on_kernel(contexts, kernel) as ctx:       # the default is back: the same bits as before the setting changed
            assert_same_bits(before, ctx.svd_split(A, m))
    if known:
        pytest.xfail(known)


# ---- replicas agree ------------------------------------------------------------------------------------------------------------
def assert_same_bits(a, b):
    for x, y, what in zip(a, b, ('US', 'SVh', 'sig')):
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), what


@pytest.mark.parametrize('kernel', list(KERNELS))
def test_same_call_twice_same_bits(contexts, kernel):
    with on_kernel(contexts, kernel) as ctx:
        for rows, cols in KERNELS[kernel][1]:
            n = min(rows, cols)
            for family in ('gauss', 'clusters', 'dup_rows', 'graded1e6'):
                A, _ = case(family, rows, cols)
                m = max(1, n // 2)
                assert_same_bits(ctx.svd_split(A, m), ctx.svd_split(A, m))


def test_same_bits_after_calls_of_other_shapes_and_paths(contexts):
    """Stale scratch (rotation log, progress words, Gram buffers, the reduction buffer) would show here."""
    c2, c3 = contexts[2], contexts[3]
    big, _ = case('clusters', 128, 128)
    small, _ = case('gauss', 6, 6)
    mid, _ = case('graded1e6', 40, 80)
    first = c2.svd_split(big, 64)                      # HBM-resident
    c2.svd_split(small, 3)                             # in-LDS
    assert_same_bits(first, c2.svd_split(big, 64))
    lds = c2.svd_split(mid, 20)                        # in-LDS, with the Cholesky step
    try:
        c2.set_narrow_path(True)
        forced = c2.svd_split(mid, 20)                 # the same matrix on the HBM-resident kernel
        c2.svd_split(small, 6)
        assert_same_bits(forced, c2.svd_split(mid, 20))
    finally:
        c2.set_narrow_path(False)
    assert_same_bits(lds, c2.svd_split(mid, 20))
    assert_same_bits(first, c2.svd_split(big, 64))
    odd, _ = case('clusters', 105, 120)
    tiny, _ = case('dup_rows', 9, 15)
    first = c3.svd_split(odd, 52)
    c3.svd_split(tiny, 4)
    assert_same_bits(first, c3.svd_split(odd, 52))


# ---- exact edges -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kernel', list(KERNELS))
def test_diagonal_gram_gives_the_entries(contexts, kernel):
    """perm_diag: every rotation has t = 0 from the first round on; sigma is the sorted absolute entries."""
    with on_kernel(contexts, kernel) as ctx:
        for rows, cols in KERNELS[kernel][1]:
            A, _ = case('perm_diag', rows, cols)
            want = np.sort(np.abs(A[A != 0]).astype(np.float64))[::-1]
            for m in sr.kept_ranks('perm_diag', min(rows, cols)):
                sig = ctx.svd_split(A, m)[2]
                assert np.abs(sig - want).max() <= 1e-12 * want[0], (rows, cols, m)


@pytest.mark.parametrize('kernel', list(KERNELS))
def test_power_of_two_scaling_is_exact(contexts, kernel):
    """scaled_up / scaled_down are gauss times 2^+-40: sigma scales by 2^+-40 and both factors by 2^+-20, bit for bit."""
    with on_kernel(contexts, kernel) as ctx:
        for rows, cols in KERNELS[kernel][1]:
            n = min(rows, cols)
            for m in sr.kept_ranks('gauss', n):
                base = ctx.svd_split(case('gauss', rows, cols)[0], m)
                for family, e in (('scaled_up', 40), ('scaled_down', -40)):
                    US, SVh, sig = ctx.svd_split(case(family, rows, cols)[0], m)
                    back = (np.ldexp(US, -e // 2), np.ldexp(SVh, -e // 2), np.ldexp(sig, -e))
                    assert_same_bits(base, back)


@pytest.mark.parametrize('kernel,shape,family,stop2', cases(KERNELS, ['dup_rows_tail']))
def test_rank_deficient_columns_beyond_the_rank_are_small(contexts, kernel, shape, family, stop2):
    """dup_rows with m above the exact rank k: the columns beyond k of both factors are finite and below 1e-3 sqrt(S0)."""
    rows, cols = shape
    n = min(rows, cols)
    k = sr.dup_rank(n)
    A, (_, S, _) = case('dup_rows', rows, cols)
    missed = {}
    with on_kernel(contexts, kernel) as ctx:
        for m in sorted({min(k + 1, n), n}):
            if m <= k:
                continue
            US, SVh, _ = ctx.svd_split(A, m)
            tail = max(np.abs(US[:, k:]).max(), np.abs(SVh[k:]).max())
            if not (np.isfinite(US).all() and np.isfinite(SVh).all() and tail < 1e-3 * np.sqrt(S[0])):
                missed[(m, 'tail')] = 'columns beyond the rank %.2e sqrt(S0)' % (tail / np.sqrt(S[0]))
    known = settle((kernel, shape, family, stop2), 'cap 1e-3 sqrt(S0)', missed)
    if known:
        pytest.xfail(known)


# ---- refusals leave the context usable -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('kernel', list(KERNELS))
def test_refusals_leave_the_context_usable(contexts, kernel):
    D, shapes, _ = KERNELS[kernel]
    rows, cols = shapes[-1]
    n = min(rows, cols)
    A, _ = case('clusters', rows, cols)
    rng = np.random.default_rng(5)
    refused = [(A, 0), (A, n + 1),
               (rng.standard_normal((rows + 1, cols)).astype(np.float32), 1),          # rows not a multiple of D
               (rng.standard_normal((65 * D, 65 * D)).astype(np.float32), 4)]           # short side 130 (D = 2) / 195 (D = 3) > 128
    with on_kernel(contexts, kernel) as ctx:
        if D == 2:
            assert refused[-1][0].shape == (130, 130) and refused[-1][0].size <= 32768  # the buffers would hold it
        before = ctx.svd_split(A, n // 2)
        for mat, m in refused:
            with pytest.raises(hip().TnmlError) as ei:
                ctx.svd_split(mat, m)
            assert ei.value.code == -1, (mat.shape, m, str(ei.value))
            assert_same_bits(before, ctx.svd_split(A, n // 2))
