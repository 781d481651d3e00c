"""Inner products, distances and linear combinations of two MPS without a GPU: the float64 reference of
tests/mps_algebra_reference.py against a dense contraction, against quadrature and against forward64, the conditions that make the
device comparisons of tests/test_mps_algebra_gpu.py decidable, the declarations, and the host side of the new calls under sanitizers."""
import math
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

import mps_algebra_reference as A                                                             # noqa: E402
import orthogonalize_reference as R                                                           # noqa: E402
from gradient_step_reference import forward64                                                 # noqa: E402
from tensornetworkforml_amd import _hip                                                       # noqa: E402


def random_chain(rng, N, D, L, bond, l):
    return [rng.standard_normal(s) for s in R.shapes_of(N, D, L, bond, l)]


@pytest.mark.parametrize('N', [2, 3, 6])
def test_transfer_chain_against_dense_contraction(N):
    """<W|W>, <V|V>, <W|V> of the transfer reference are the sums over the dense tensors: D = 2, 3, L = 2, 3, every label position,
    Euclidean and with a metric per site.  Both are float64 sums of at most D^6 L products of O(1) numbers: 1e-11 relative to the
    norms covers their rounding a thousand times."""
    n = 0
    for D in (2, 3):
        for L in (2, 3):
            for l in range(N):
                rng = np.random.default_rng([5, N, D, L, l])
                W = random_chain(rng, N, D, L, [3] * (N - 1), l)
                V = random_chain(rng, N, D, L, [2 + (i % 3) for i in range(N - 1)], l)
                for metric in (None, A.spd_metric(rng, D, N)):
                    t = A.inner3(W, V, l, metric)
                    want = [A.inner_dense(W, W, l, metric), A.inner_dense(V, V, l, metric), A.inner_dense(W, V, l, metric)]
                    scale = math.sqrt(want[0] * want[1])
                    for (s, lg), w, sc in zip(t, want, (want[0], want[1], scale)):
                        assert abs(s * math.exp(lg) - w) <= 1e-11 * sc, (N, D, L, l, s * math.exp(lg), w)
                    n += 1
    assert n == 2 * 2 * N * 2


def test_zero_product_and_signs():
    rng = np.random.default_rng(3)
    W = random_chain(rng, 3, 2, 2, [2, 2], 1)
    Z = [c.copy() for c in W]
    Z[0][:] = 0.0
    assert A.inner(W, Z, 1) == (0.0, -math.inf)
    M = [c.copy() for c in W]
    M[1] = -M[1]
    s, lg = A.inner(W, M, 1)
    assert s == -1.0 and abs(lg - A.inner(W, W, 1)[1]) < 1e-12


@pytest.mark.parametrize('D', [2, 3, 8])
def test_uniform_metric_is_the_l2_inner_product(D):
    """With psi_gram(D) on every site <W|V> is int f_W . f_V over uniform pixels: against a 16-point Gauss-Legendre grid per site of
    forward64 outputs at N = 3 (the integrand is a polynomial of degree 2 (D - 1) in sin and cos of pi x / 2 per site; 16 points
    integrate it to 1e-13 at D = 8, checked below on the Gram matrix itself)."""
    from tensornetworkforml_amd import data_generator as gen
    G = gen.psi_gram(D)
    assert np.abs(G - A.psi_gram(D)).max() < 1e-14 and np.abs(G - A.psi_gram(D, 16)).max() < 1e-12
    assert np.array_equal(G, G.T)
    if D == 2:
        assert np.abs(G - np.array([[0.5, 1 / math.pi], [1 / math.pi, 0.5]])).max() < 1e-15
    N, L = 3, 2
    t, w = np.polynomial.legendre.leggauss(16)
    x, w = 0.5 * (t + 1.0), 0.5 * w
    grid = np.stack(np.meshgrid(x, x, x, indexing='ij'), -1).reshape(-1, N)
    wt = np.einsum('i,j,k->ijk', w, w, w).ravel()
    X = gen.psi(grid, D)
    for l in range(N):
        rng = np.random.default_rng([8, D, l])
        W = random_chain(rng, N, D, L, [3, 2], l)
        V = random_chain(rng, N, D, L, [2, 3], l)
        fw, fv = forward64(W, l, X), forward64(V, l, X)
        want = float((fw * fv * wt[None, :]).sum())
        s, lg = A.inner(W, V, l, G)
        assert abs(s * math.exp(lg) - want) <= 1e-10 * math.sqrt(float((fw * fw * wt).sum()) * float((fv * fv * wt).sum())), (D, l)


def test_direct_sum_adds_the_functions():
    """forward64(aW + bV) = a f_W + b f_V for every small case, and the float32 form rounds the label-site blocks only"""
    for case in A.small_cases():
        N, D, L, l = case
        W, V, X, _ = A.build_small(case)
        X64 = X.astype(np.float64)
        fw, fv = forward64(W, l, X64), forward64(V, l, X64)
        for a, b in ((1.0, 1.0), (1.0, -1.0), (0.5, 0.5), (0.3, -1.7)):
            S = A.direct_sum(W, V, l, a, b)
            assert R.bonds_of(S) == [x + y for x, y in zip(R.bonds_of(W), R.bonds_of(V))]
            f = forward64(S, l, X64)
            assert np.abs(f - (a * fw + b * fv)).max() <= 1e-12 * (abs(a) * np.abs(fw).max() + abs(b) * np.abs(fv).max()), case
        S32 = A.direct_sum(W, V, l, 0.5, -1.0, np.float32)
        S64 = A.direct_sum(W, V, l, 0.5, -1.0)
        assert all(c.dtype == np.float32 and np.array_equal(c.astype(np.float64), d) for c, d in zip(S32, S64)), case   # powers of two: exact


def test_norm_of_the_sum_from_the_three_products():
    for case in A.small_cases()[::5]:
        N, D, L, l = case
        W, V, X, _ = A.build_small(case)
        t = A.inner3(W, V, l)
        ww, vv, wv = (s * math.exp(lg) for s, lg in t)
        for a, b in ((1.0, 1.0), (1.0, -1.0), (0.5, 0.5)):
            S = A.direct_sum(W, V, l, a, b)
            s, lg = A.inner(S, S, l)
            assert abs(s * math.exp(lg) - (a * a * ww + b * b * vv + 2 * a * b * wv)) <= 1e-12 * (a * a * ww + b * b * vv), case


def test_pairs_are_far_enough_apart_for_distance_comparisons():
    """Distance and cosine are compared on the device only for pairs whose reference relative distance is >= 1e-3: the three terms of
    the distance cancel in float64, and below that the cancellation, not the kernels, would decide."""
    pairs = [(c, A.build_small(c)[:2]) for c in A.small_cases()]
    case, W, V, _, _ = A.tile_pair()
    pairs.append((case, (W, V)))
    case, W, V = A.long_pair()
    pairs.append((case, (W, V)))
    for case, (W, V) in pairs:
        d = math.sqrt(max(0.0, A.distance2(A.inner3(W, V, case[3]))))
        assert d >= A.MIN_DISTANCE and math.isfinite(d), (case, d)


def test_compression_certificate_holds_on_the_reference():
    """|W - W_c|^2 / |W|^2 <= sum of the discarded weights: the cuts of one sweep with the centre on the bond are nested orthogonal
    projections, so the squared errors add up and each is its discarded weight times a squared norm that is at most |W|^2.  The
    device test asserts the bound with the usual factor 2 (d^2 <= 2 sum); here the float64 reference must keep that factor to spare,
    up to 1e-6 relative for its own rounding (the cancellation in d^2 >= 1e-6 costs 1e-9 at the most)."""
    for case in A.CERT_CASES:
        W, X, Wc, d2, disc = A.certificate_reference(case)
        assert d2 >= A.MIN_DISTANCE ** 2, (case[0], d2)
        assert d2 <= disc * (1 + 1e-6), (case[0], d2, disc)


def test_calls_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, 'include', 'tnml.h')).read()
    assert re.search(r'int tnml_inner\(tnml_ctx \*ctx, const float \*other_flat, size_t n_floats, const int32_t \*other_bond, int other_l_pos,\s*'
                     r'const double \*metric, int metric_sites, double \*out6\);', header)
    assert re.search(r'int tnml_axpby\(tnml_ctx \*ctx, double alpha, double beta, const float \*other_flat, size_t n_floats,\s*'
                     r'const int32_t \*other_bond, int other_l_pos, int32_t \*bond_out\);', header)
    for s in ('tnml_inner', 'tnml_axpby'):
        assert s in _hip.SYMBOLS and hasattr(_hip.lib(), s)
    assert len(_hip.lib().tnml_inner.argtypes) == 8 and len(_hip.lib().tnml_axpby.argtypes) == 8
    for m in ('inner', 'axpby'):
        assert callable(getattr(_hip.Context, m))
    import tensornetworkforml_amd as pkg
    for m in ('inner', 'cosine', 'distance', 'add'):
        assert callable(getattr(pkg.Network_class.Network, m))
    assert callable(pkg.Network_class.combine) and callable(pkg.data_generator.psi_gram)


def test_algebra_host_side_under_sanitizers():
    """csrc/Makefile target `san-algebra`: tnml_inner / tnml_axpby of api_mps.hip and the launch wrappers of kernels_algebra.hip,
    built --cuda-host-only with -fsanitize=address,undefined, against the stand-in runtime of csrc/san/hip_stub.cpp
    (csrc/san/plan_algebra_main.cpp, a stand-alone program): C3 and C5 at true size with the label at both ends and inside, a ragged
    17-site chain with different bonds for W and V at every label position at D = 2, 3 and 8, N = 2, every refusal (none launches),
    the commit and optimiser-state rules after tnml_axpby, and every allocation of the new group failing in turn."""
    import shutil
    import subprocess
    if shutil.which('g++') is None or not os.path.exists('/opt/rocm/bin/hipcc'):
        pytest.skip('no g++ / hipcc')
    csrc = os.path.join(ROOT, 'tensornetworkforml_amd', 'csrc')
    out = subprocess.run(['make', '-C', csrc, '-j4', 'san-algebra'], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert 'algebra host planning under ASan + UBSan: ok' in out.stdout
    for name in ('c3 bond 20 L 2, label on 0', 'c3 last bond 20', 'c3 inner label', 'c5 bond 50 L 10', 'c5 first', 'c5 inner label',
                 'ragged N 17 D 2', 'ragged N 17 D 3', 'ragged N 17 D 8', 'ragged N 2 D 2', 'algebra refusals: ok',
                 'commit rule and optimiser state rule after tnml_axpby: ok', '0 live allocations'):
        assert name in out.stdout, name
    assert out.stdout.count('11 failed in turn') == 8
