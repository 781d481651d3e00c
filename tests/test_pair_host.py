"""The NumPy statement of the pixel-pair marginals (tests/pair_reference.py) against dense enumeration, its
identities, the committed bounds of tests/test_pair_gpu.py against the function that produced them, the condition under which a
correlation is compared, the host side of tnml_pair_marginals under the sanitizers, and what of the Python wrappers needs no
device."""
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

import pair_reference as P                                         # noqa: E402
import sample_reference as S                                       # noqa: E402
from tensornetworkforml_amd import _hip                            # noqa: E402

# the reference against a dense table: both are float64 sums over the same few terms in different orders (the bound of
# tests/test_site_cond_host.py for chains of this kind; 5e-15 is what the cases below give)
P_TOL_DENSE = 4e-11


@pytest.mark.parametrize('N', [4, 5])
def test_reference_against_dense_enumeration(N):
    """D = 2, L = 3, K = 4, the label on the first, a middle and the last site, summed and every class: the table of every pair, the
    one-site tables, every statistic and I(x_i; l) against the K^N L numbers of sample_reference.dense_joint; q itself against the
    whole tensor closed with S"""
    worst = 0.0
    for l in (0, 2, N - 1):
        cores, _, phi, w, x = P.dense_inputs(l, 4, N)
        for q in (-1, 0, 1, 2):
            r = P.pair_marginals(cores, l, phi, w, x, q)
            lev, fea = P.dense_levels(cores, l, phi, w, x, q), P.dense_features(cores, l, phi, w, x, q)
            d = [np.abs(P.pair_table(r['q'], phi, w) - lev['P']).max(), np.abs(r['p1'] - lev['p1']).max(), np.abs(r['stats'] - lev['stats']).max(),
                 np.abs(r['stats1'] - lev['stats1']).max(), np.abs(r['q'] - fea['q']).max(), np.abs(r['q1'] - fea['q1']).max(),
                 np.abs(fea['stats'] - lev['stats']).max()]
            worst = max(worst, float(max(d)))
        info = P.label_information(cores, l, phi, w)
        worst = max(worst, float(np.abs(info - P.dense_levels(cores, l, phi, w, x, -1)['label_info']).max()))
        assert np.all(info >= -1e-15)
    print('N %d: worst difference %.2e' % (N, worst))
    assert worst <= P_TOL_DENSE


def test_identities():
    ci = 25
    N, D, L, l, K = S.draw_cases()[ci]
    cores, _, phi, w, x = P.ragged_inputs(ci)
    Sg = S.gram(phi, w).reshape(-1)
    for q in (-1, 1):
        r = P.pair_marginals(cores, l, phi, w, x, q)
        cover = P.pairs_of(range(N), N)
        Q = r['q'].reshape(N, N, D, D, D, D)
        assert float(np.abs(np.einsum('x,ijxy,y->ij', Sg, r['q'], Sg)[cover] - 1.0).max()) <= 1e-13           # sum S (x) S q_ij = 1
        for i in range(N - 1):                                                                                  # S on j leaves q1_i, S on i q1_j
            assert float(np.abs(np.einsum('jxy,y->jx', r['q'][i, i + 1:], Sg) - r['q1'][i].reshape(-1)).max()) <= 1e-13
            assert float(np.abs(np.einsum('x,jxy->jy', Sg, r['q'][i, i + 1:]) - r['q1'][i + 1:].reshape(N - 1 - i, -1)).max()) <= 1e-13
        # (d,d') <-> (d',d) together with (e,e') <-> (e',e): the same sums in another order
        assert float(np.abs(Q - Q.transpose(0, 1, 3, 2, 5, 4)).max()) <= 1e-13 * float(np.abs(Q).max())
        assert not r['q'][~cover].any() and not r['stats'][~cover].any()
        # MI >= 0 up to the rounding of its K^2 terms, whose magnitudes sum to less than 2 log K + I; |corr| <= 1
        assert np.all(r['stats'][..., 2] >= -2.0 ** -53 * K * K) and np.all(np.abs(r['stats'][..., 1]) <= 1 + 1e-12)
        tab = P.pair_table(r['q'][3, 9], phi, w)
        assert abs(tab.sum() - 1.0) <= 1e-13 and float(np.abs(tab.sum(1) - r['p1'][3]).max()) <= 1e-14
    # a chain of bond 1 is a product: no information, no covariance
    rng = np.random.default_rng(8)
    prod = S.chain(6, 2, 3, [1] * 5, 2, rng)
    x, phi, w = S.grid(7, 2)
    r = P.pair_marginals(prod, 2, phi, w, x, -1)
    assert float(np.abs(r['stats'][..., [0, 2]]).max()) <= 1e-15
    # a zero density adds nothing; a variance of zero gives correlation 0
    t = P.pair_statistics(np.array([[0.5, 0.0], [0.0, 0.5]]), [0.0, 1.0])
    assert np.allclose(t, [0.25, 1.0, np.log(2.0)])
    assert P.pair_statistics(np.array([[0.5, 0.5], [0.0, 0.0]]), [0.0, 1.0])[1] == 0.0


@pytest.mark.parametrize('cls', P.CLASSES, ids=str)
def test_every_device_case_keeps_its_correlations_comparable(cls):
    """both reference standard deviations of every pair of every case exceed CORR_MIN_STD times the range"""
    smallest = np.inf
    for index, (args, _) in enumerate(P.class_calls(cls)):
        ref = P.reference(cls, index)
        rows = list(range(len(args[0]))) if args[6] is None else args[6]
        assert P.corr_condition(ref, rows, args[4]).all(), (cls, index)
        smallest = min(smallest, float(ref['std'].min() / (np.max(args[4]) - np.min(args[4]))))
    print('%s: smallest standard deviation %.2e of the range' % (cls, smallest))


@pytest.mark.parametrize('cls', P.CLASSES, ids=str)
def test_bounds_are_what_their_function_gives(cls):
    """The committed table: ten times the larger of the reference's own float64-against-long-double difference (a) and
    2^-53 N m^2 D (b), rounded up to one digit.  The dense class is recomputed whole; of every other class one call, whose (a)
    cannot exceed the class's."""
    assert np.finfo(np.longdouble).eps < 2e-19
    assert set(P.BOUNDS) == set(P.CLASSES) and all(set(P.BOUNDS[c]) == set(P.MEASURES) for c in P.CLASSES)
    if cls == 'dense':
        assert P.bounds_of(cls) == pytest.approx(P.BOUNDS[cls], rel=1e-9)
        return
    a, b = P.figures(cls, sample=True)
    print(cls, a, b)
    calls = P.class_calls(cls)
    bmax = max(P.accumulation(*dims) for _, dims in calls)
    for k in P.MEASURES:
        assert P.round_up(10.0 * max(a[k], b)) <= P.BOUNDS[cls][k] * (1 + 1e-9), k
        assert P.BOUNDS[cls][k] >= P.round_up(10.0 * bmax) * (1 - 1e-9)


def test_call_is_declared_exported_and_bound():
    header = open(os.path.join(ROOT, 'include', 'tnml.h')).read()
    assert re.search(r'int tnml_pair_marginals\(tnml_ctx \*ctx, int K, const double \*phi, const double \*w, const double \*values, int class_slot,\s*'
                     r'const int32_t \*rows, int n_rows, double \*q1_out, double \*stats1_out, double \*q_out, double \*stats_out\);', header)
    lim = int(re.search(r'#define TNML_PAIR_MAX_BOND (\d+)', header).group(1))
    assert lim == _hip.PAIR_MAX_BOND
    internal = open(os.path.join(ROOT, 'tensornetworkforml_amd', 'csrc', 'tnml_internal.h')).read()
    assert 'kPairMaxBond = kLnzMaxBond' in internal and 'kLnzMaxBond = %d' % lim in internal
    assert re.search(r'bonds up to %d \(`TNML_PAIR_MAX_BOND`\)' % lim, open(os.path.join(ROOT, 'README.md')).read())
    name = 'tnml_pair_marginals'
    assert name in _hip.SYMBOLS and hasattr(_hip.lib(), name) and len(getattr(_hip.lib(), name).argtypes) == 12
    assert callable(_hip.Context.pair_marginals)
    import tensornetworkforml_amd as pkg
    for m in ('pixel_pair_marginals', 'mutual_information', 'pixel_correlations', 'pair_probs', 'pixel_label_information'):
        assert callable(getattr(pkg.Network_class.Network, m))


def test_pair_probs_is_the_table_of_the_reference():
    import tensornetworkforml_amd as pkg
    ci = 25
    N, D, L, l, K = S.draw_cases()[ci]
    cores, _, phi, w, x = P.ragged_inputs(ci)
    r = P.pair_marginals(cores, l, phi, w, x, -1, [2, 7])
    net = pkg.Network_class.Network.__new__(pkg.Network_class.Network)
    net.N, net.D = N, D
    p = net.pair_probs(r['q'].reshape(2, N, D, D, D, D), levels=K, weights=w)
    assert p.shape == (2, N, K, K) and float(np.abs(p - P.pair_table(r['q'], phi, w)).max()) <= 1e-15
    sym = net._symmetric(np.arange(9.0).reshape(3, 3), [7.0, 8.0, 9.0])
    assert np.array_equal(sym, [[7, 1, 2], [1, 8, 5], [2, 5, 9]])


def test_pair_marginals_host_side_under_sanitizers():
    """csrc/Makefile target `san-pair`: tnml_pair_marginals of tnml_api.hip and the launch wrappers of kernels_pair.hip, built
    --cuda-host-only with -fsanitize=address,undefined, against the stand-in runtime of csrc/san/hip_stub.cpp
    (csrc/san/plan_pair_main.cpp, a stand-alone program): C3 and C5 at true size under the default budget and under one row's, a
    ragged 17-site chain at D = 2, 3 and 8, N = 2, every output NULL in turn, every refusal (none launches), the bond limit taken
    and refused, and every allocation of the new group failing in turn, fresh and at growth."""
    import shutil
    import subprocess
    if shutil.which('g++') is None or not os.path.exists('/opt/rocm/bin/hipcc'):
        pytest.skip('no g++ / hipcc')
    csrc = os.path.join(ROOT, 'tensornetworkforml_amd', 'csrc')
    out = subprocess.run(['make', '-C', csrc, '-j4', 'san-pair'], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert 'pair marginals host planning under ASan + UBSan: ok' in out.stdout
    for name in ('c3 bond 20 L 2, label on 0', 'c5 inner label bond 50 L 10, label on 400', 'ragged N 17 D 2', 'ragged N 17 D 3', 'ragged N 17 D 8',
                 'ragged N 2 D 2', 'pair marginals refusals: ok', '0 live allocations'):
        assert name in out.stdout, name
    assert out.stdout.count('18 failed in turn') == 8 and out.stdout.count(' 0 failed in turn') == 4
