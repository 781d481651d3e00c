"""The Jacobi rounds of the in-LDS SVD (kernels_narrow.hip, phase 7) run as one loop per wave role, unrolled by two.  That is a change
of control flow and addressing alone: no operand, operation or rounding may move, so everything here is equality of bits.

1. Context.svd_split against bits recorded from the build BEFORE the round loop was restructured
   (tests/golden/svd_split_bits_in_lds_jacobi.npz, written by tools/record_svd_split_bits.py).  Short sides 2 (a pair that meets
   itself), 4 and 6 (the first sizes with separate V and G waves), 20 and 40 (the two benchmark sizes; 40 is the largest size at one
   V block per lane), 42 (two V blocks per lane), 48, 62 (a second G item per thread); matrices n x 2n; cuts 1, n / 2, n.  Families of
   svd_split_reference.py: gauss and near_equal (nearly orthonormal rows) at every size -- neither takes the Cholesky step: an n x 2n
   Gaussian matrix has off(G) / trace(G) ~ 1 / sqrt(2n), under the threshold -- and graded1e6, which takes it wherever the kernel has
   it (n > 4), at n = 4, 6, 20, 40, 42.  US, SVh, sigma and the sweeps / rounds / Cholesky counters of svd_stats are asserted equal.
   The file holds the input matrices too (two of the families go through LAPACK on the host).
   A later, DELIBERATE change of the SVD's numerics re-records the file with that script; nothing else may.
2. The same call twice returns the same bits.
3. Persistent sweeps at the two compiled shapes (bond 20 and bond 10, two labels; N = 16, 64 samples): bodies compiled for the shape
   against the generic bodies and mode 1 against mode 2 bit for bit, and against one launch per step (set_persistent(0), another
   association order of the same sums) under the path-against-path bounds of
   test_hip_parity.py::test_persistent_sweep_matches_per_step_launches_and_oracle, which test_shape_kernels_gpu.py relies on for its
   generic path.
"""
import os

import numpy as np
import pytest

from test_timed_paths_gpu import HP_SOFT, assert_same, device_sweep, new_ctx, path_of, prepare, relerr

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'svd_split_bits_in_lds_jacobi.npz')
SIZES = (2, 4, 6, 20, 40, 42, 48, 62)
FAMILIES = {'gauss': SIZES, 'near_equal': SIZES, 'graded1e6': (4, 6, 20, 40, 42)}
GROUPS = [(f, n) for f, sizes in FAMILIES.items() for n in sizes]


def hip():
    from tensornetworkforml_amd import _hip
    return _hip


def cuts(n):
    return sorted({1, max(1, n // 2), n})


@pytest.fixture(scope='module')
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope='module')
def ctx():
    c = hip().Context(4, 2, 2, 64, 64)
    yield c
    c.close()


def stats(ctx):
    sweeps, svds, rounds = ctx.svd_stats(False)
    return np.array([sweeps, svds, rounds, ctx.cholesky_steps])


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_the_file_holds_exactly_the_cases(golden):
    want = {'A_%s_%d' % g for g in GROUPS}
    want |= {'%s_%s_%d_%d' % (w, f, n, m) for f, n in GROUPS for m in cuts(n) for w in ('US', 'SVh', 'sigma', 'counters')}
    assert set(golden) == want


@pytest.mark.parametrize('family,n', GROUPS)
def test_svd_split_bits_are_those_of_the_parent_build(ctx, golden, family, n):
    A = golden['A_%s_%d' % (family, n)]
    assert A.shape == (n, 2 * n) and A.dtype == np.float32
    for m in cuts(n):
        key = '%s_%d_%d' % (family, n, m)
        s0 = stats(ctx)
        US, SVh, sig = ctx.svd_split(A, m)
        d = (stats(ctx) - s0).astype(np.int64)
        want = golden['counters_' + key]                      # sweeps, rounds, Cholesky steps
        print(key, 'sweeps', d[0], 'rounds', d[2], 'cholesky', d[3], 'recorded', list(want))
        assert d[1] == 1
        # the Cholesky decision of each family, by its own rule and as recorded
        assert d[3] == (1 if family == 'graded1e6' and n > 4 else 0)
        assert [d[0], d[2], d[3]] == list(want), key
        assert same_bits(sig, golden['sigma_' + key]), key
        assert same_bits(US, golden['US_' + key]), key
        assert same_bits(SVh, golden['SVh_' + key]), key


def test_same_call_twice_same_bits(ctx, golden):
    for family, n in GROUPS:
        A = golden['A_%s_%d' % (family, n)]
        m = max(1, n // 2)
        s0 = stats(ctx)
        a = ctx.svd_split(A, m)
        s1 = stats(ctx)
        b = ctx.svd_split(A, m)
        s2 = stats(ctx)
        assert all(same_bits(x, y) for x, y in zip(a, b)), (family, n)
        assert list(s1 - s0) == list(s2 - s1), (family, n)


# ---- persistent sweeps at the two compiled shapes ------------------------------------------------------------------------------------
N, B, L = 16, 64, 2


@pytest.mark.parametrize('M', [20, 10])
def test_persistent_sweeps_at_the_compiled_shapes(M):
    X, y, cores32 = prepare(N, M, L, B, 11)
    forms = (('on', 1, True), ('off', 1, False), ('mode2', 2, True), ('per_step', 0, True))
    ctxs = {}
    for name, mode, shape in forms:
        c = new_ctx(N, L, M, X, y, cores32, 0, mode)
        c.set_shape_kernels(shape)
        ctxs[name] = c
    try:
        for sw in range(2):
            left = sw == 1
            if sw == 1:                                       # sweep 2: every form from the cores the first one left
                cores_d, _, lp = ctxs['on'].get_cores()
                for name in ('off', 'mode2', 'per_step'):
                    ctxs[name].set_cores(cores_d, lp)
            res, fixed = {}, {}
            for name, c in ctxs.items():
                met, f, cnt = device_sweep(c, left, HP_SOFT)
                res[name] = (met, f, c.get_cores())
                fixed[name] = c.fixed_shape_steps()
                assert path_of(cnt, N) == ('per-step' if name == 'per_step' else 'persistent'), (name, sw)
            assert fixed['on'] > 0 and fixed['off'] == 0 and fixed['mode2'] == 0, fixed
            assert_same(res['on'], res['off'])                # compiled for the shape = generic body
            assert_same(res['on'], res['mode2'])              # one kernel = one kernel per role
            (m1, f1, (_, bond1, lp1)), (m0, f0, (_, bond0, lp0)) = res['on'], res['per_step']
            fp = relerr(f1, f0)
            acc, mae = np.abs(m1[:, 0] - m0[:, 0]).max(), np.abs(m1[:, 1] - m0[:, 1]).max()
            print('bond', M, 'sweep', sw + 1, 'fixed steps', fixed['on'], 'persistent vs per-step: f %.2e accuracy %.2e MAE %.2e' % (fp, acc, mae))
            assert list(bond1) == list(bond0) and lp1 == lp0
            assert fp < (1e-5 if sw == 0 else 1.4e-2)
            assert acc <= 1.0 / B + 1e-6 and mae < 2e-4
    finally:
        for c in ctxs.values():
            c.close()
