"""The NumPy statement of the per-pixel conditionals (tests/site_cond_reference.py) against a dense
enumeration, its statistics against the full table, the committed bounds of tests/test_site_cond_gpu.py against the function that
produced them, the condition that makes the device's modes comparable, the host side of tnml_site_conditionals under the
sanitizers, and what of the Python wrappers needs no device."""
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p_ in (ROOT, HERE):
    if p_ not in sys.path:
        sys.path.insert(0, p_)

import sample_masked_reference as M                                # noqa: E402
import sample_reference as S                                       # noqa: E402
import site_cond_reference as C                                    # noqa: E402
from tensornetworkforml_amd import _hip                            # noqa: E402

# the reference against a dense table: both are float64 sums over the same few terms in different orders (the bound of
# tests/test_sample_masked_host.py for the same chains; 5.8e-14 to 8.1e-14 is what the cases below give)
P_TOL_DENSE = 4e-11


@pytest.mark.parametrize('l', C.DENSE_L)
def test_reference_against_dense_enumeration(l):
    """N = 4, K = 3, D = 2, L = 2: all 16 masks, every assignment of known levels, classes -1, 0 and 1"""
    D, L, N, K = 2, 2, 4, 3
    cores, phi, w = S.dense_case(D, L, N, K, l)
    P = S.dense_joint(cores, l, phi, w)
    lev, _ = S.dense_rows(N, K, 1)
    worst, rows = 0.0, 0
    for mask in M.all_masks(N):
        known = np.unique(np.where(mask, lev, 0), axis=0)
        for q in (-1, 0, 1):
            r = C.conditionals(cores, l, phi, w, None, np.full(len(known), q), mask, known)
            for s in range(len(known)):
                for i in range(N):
                    worst = max(worst, float(np.abs(r['p'][s, i] - C.dense_conditional(P, mask, known[s], q, i)).max()))
            assert float(np.abs(r['logp'] - np.log([M.dense_marginal(P, mask, k, q) for k in known])).max()) <= P_TOL_DENSE
            rows += len(known)
    print('label on %d, %d rows: worst difference of a probability %.2e' % (l, rows, worst))
    assert rows == 3 * 4 ** 4 and worst <= P_TOL_DENSE


def test_statistics_against_the_full_table():
    a = C.ragged_inputs(25, 'drawn')
    cores, l, phi, w, x, classes, mask, shared, known = a
    r = C.reference('ragged', (25, 'drawn'), 'own')
    p, st = r['p'], r['stats']
    assert float(np.abs(p.sum(-1) - 1.0).max()) <= 1e-12                                             # Q is normalised by tr(S Q)
    assert float(np.abs(w * np.einsum('kd,nide,ke->nik', phi, r['q'], phi) - p).max()) <= 1e-15      # the table is a function of q alone
    n, N, K = p.shape
    for s in range(0, n, 7):
        for i in range(N):
            mean = sum(p[s, i, k] * x[k] for k in range(K))
            var = sum(p[s, i, k] * (x[k] - mean) ** 2 for k in range(K))
            ent = -sum(p[s, i, k] * np.log(p[s, i, k]) for k in range(K) if p[s, i, k] > 0)
            lk = np.log(p[s, i, known[s, i]]) if mask[s, i] else 0.0
            assert np.allclose([mean, var, ent, lk], st[s, i], rtol=1e-12, atol=1e-15)
            assert r['mode'][s, i] == max(range(K), key=lambda k: (p[s, i, k], -k))
    # a zero density adds nothing to the entropy; the first of two equal largest densities is the mode
    t = C.statistics(np.array([[[0.5, 0.0, 0.5]]]), [0.0, 1.0, 2.0], np.array([[True]]), np.array([[1]]))
    assert np.array_equal(t['mode'], [[0]]) and np.allclose(t['stats'][0, 0, :3], [1.0, 1.0, np.log(2.0)]) and t['stats'][0, 0, 3] == -np.inf


@pytest.mark.parametrize('cls', C.CLASSES, ids=str)
def test_bounds_are_what_their_function_gives(cls):
    """The committed table: ten times the larger of the reference's own float64-against-long-double difference (a) and
    2^-53 N m^2 D (b), rounded up to one digit.  The dense class is recomputed whole; of every other class one call, whose (a)
    cannot exceed the class's."""
    assert np.finfo(np.longdouble).eps < 2e-19
    assert set(C.BOUNDS) == set(C.CLASSES) and all(set(C.BOUNDS[c]) == set(C.MEASURES) for c in C.CLASSES)
    if cls == 'dense':
        assert C.bounds_of(cls) == pytest.approx(C.BOUNDS[cls], rel=1e-9)
        return
    a, b = C.figures(cls, sample=True)
    print(cls, a, b)
    for k in C.MEASURES:
        assert C.round_up(10.0 * max(a[k], b)) <= C.BOUNDS[cls][k] * (1 + 1e-9), k
        assert C.BOUNDS[cls][k] >= C.round_up(10.0 * b) * (1 - 1e-9)
    calls = C.class_calls(cls)
    assert C.BOUNDS[cls]['var'] >= 10.0 * max(C.accumulation(*dims) for _, dims in calls)


def test_device_cases_have_decidable_modes():
    """in every device case at least 95 % of the (sample, site) pairs have two largest densities further apart than MARGIN, relative"""
    total, und, gap = 0, 0, np.inf
    refs = [C.reference('dense', l, None) for l in C.DENSE_L]
    for row in S.ROWS:
        for ci, _ in C.ragged_cases(row):
            refs += [C.reference('ragged', (ci, kind), which) for kind in C.LEVEL_KINDS for which in ('own', 'shared')]
    refs += [C.reference('wide', wi, which) for wi in (0, 1) for which in ('suffix', 'random')]
    for r in refs:
        ok = C.decidable_modes(r['p'])
        assert ok.sum() >= 0.95 * ok.size
        top = np.sort(r['p'].astype(np.float64), axis=-1)[..., -2:]
        total, und, gap = total + ok.size, und + int((~ok).sum()), min(gap, float(((top[..., 1] - top[..., 0]) / top[..., 1])[ok].min()))
    print('%d sites, %d undecidable, smallest decidable gap %.2e' % (total, und, gap))


@pytest.mark.parametrize('which', [0, 1], ids=['calibrated', 'raw'])
def test_long_chains_have_decidable_modes(which):
    for name in ('bottom', 'full'):
        ok = C.decidable_modes(C.reference('long', which, name)['p'])
        assert ok.sum() >= 0.95 * ok.size


def test_call_is_declared_exported_and_bound():
    header = open(os.path.join(ROOT, 'include', 'tnml.h')).read()
    assert re.search(r'int tnml_site_conditionals\(tnml_ctx \*ctx, int n, int K, const double \*phi, const double \*w, const double \*values,\s*'
                     r'const int32_t \*classes, const uint8_t \*mask, int mask_rows, const int32_t \*known,\s*'
                     r'double \*q_out, double \*stats_out, int32_t \*mode_out, double \*logp_out\);', header)
    # the bond limit is one constant, stated in the header, the README and the wrapper
    lim = int(re.search(r'#define TNML_SITE_COND_MAX_BOND (\d+)', header).group(1))
    assert lim == _hip.SITE_COND_MAX_BOND
    internal = open(os.path.join(ROOT, 'tensornetworkforml_amd', 'csrc', 'tnml_internal.h')).read()
    assert 'kSccMaxBond = TNML_SITE_COND_MAX_BOND' in internal
    assert re.search(r'bonds up to %d \(`TNML_SITE_COND_MAX_BOND`\)' % lim, open(os.path.join(ROOT, 'README.md')).read())
    name = 'tnml_site_conditionals'
    assert name in _hip.SYMBOLS and hasattr(_hip.lib(), name) and len(getattr(_hip.lib(), name).argtypes) == 14
    assert callable(_hip.Context.site_conditionals)
    import tensornetworkforml_amd as pkg
    for m in ('pixel_conditionals', 'expected_image', 'pixel_surprise', 'pixel_probs'):
        assert callable(getattr(pkg.Network_class.Network, m))


def test_pixel_probs_is_the_table_of_the_reference():
    import tensornetworkforml_amd as pkg
    r = C.reference('ragged', (25, 'drawn'), 'own')
    a = C.ragged_inputs(25, 'drawn')
    net = pkg.Network_class.Network.__new__(pkg.Network_class.Network)
    net.N, net.D = 17, 3
    p = net.pixel_probs(r['q'], levels=256, weights=a[3])
    assert p.shape == r['p'].shape and float(np.abs(p - r['p']).max()) <= 1e-15


def test_site_conditionals_host_side_under_sanitizers():
    """csrc/Makefile target `san-site-cond`: tnml_site_conditionals of tnml_api.hip and the launch wrapper of kernels_site_cond.hip,
    built --cuda-host-only with -fsanitize=address,undefined, against the stand-in runtime of csrc/san/hip_stub.cpp
    (csrc/san/plan_site_cond_main.cpp, a stand-alone program): C3 and C5 at true size under the default budget and under one tile's,
    a ragged 17-site chain at D = 2, 3 and 8, N = 2, every output NULL in turn, every refusal (none launches), the bond limit taken
    and refused, and every allocation of the new group failing in turn."""
    import shutil
    import subprocess
    if shutil.which('g++') is None or not os.path.exists('/opt/rocm/bin/hipcc'):
        pytest.skip('no g++ / hipcc')
    csrc = os.path.join(ROOT, 'tensornetworkforml_amd', 'csrc')
    out = subprocess.run(['make', '-C', csrc, '-j4', 'san-site-cond'], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert 'site conditionals host planning under ASan + UBSan: ok' in out.stdout
    for name in ('c3 bond 20 L 2, label on 0, tiles of 8', 'c3 inner label', 'c5 bond 50 L 10, label on 783, tiles of 2', 'c5 inner label',
                 'ragged N 17 D 2', 'ragged N 17 D 3', 'ragged N 17 D 8', 'ragged N 2 D 2', 'site conditionals refusals: ok', '0 live allocations'):
        assert name in out.stdout, name
    assert out.stdout.count(' 5 failed in turn') == 4 and out.stdout.count(' 0 failed in turn') == 2 and out.stdout.count('16 failed in turn') == 2
