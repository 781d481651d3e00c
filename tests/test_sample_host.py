"""Sampling from the Born distribution of an MPS without a GPU: the float64 walk of tests/sample_reference.py
against a dense enumeration, the counter hash, the conditions that make the device comparisons of tests/test_sample_gpu.py decidable,
the declarations, and the host side of the new call under sanitizers."""
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

import sample_reference as S                                                                  # noqa: E402
from tensornetworkforml_amd import _hip                                                       # noqa: E402

# Both sides are float64 sums of a few hundred products; their rounding is a few hundred eps of the LARGEST probability of the table,
# not of each entry (an entry 1e-7 of the largest is what is left of a cancellation, and its logarithm carries 1e7 eps).  So
# probabilities are compared, relative to the largest of the table: 1e-13 is about 500 eps.
DENSE_TOL = 1e-13


def perr(logp, ref):
    return float(np.abs(np.exp(logp) - ref).max() / ref.max())


def dense_configs():
    return [(D, L, N, K, l) for D in (2, 3) for L in (2, 3) for N in (2, 3, 4) for K in (2, 3) for l in range(N) if (D + L + N + K + l) % 2 == 0 or N == 4]


def test_walk_against_dense_enumeration():
    """log p(x | c), log p(x, l) and the prefix split of the reference walk are those of the dense table: N <= 4, D in {2, 3},
    L in {2, 3}, K in {2, 3}, every label position, non-uniform weights; the probabilities sum to 1."""
    n_cases = 0
    for (D, L, N, K, l) in dense_configs():
        cores, phi, w = S.dense_case(D, L, N, K, l)
        P = S.dense_joint(cores, l, phi, w)
        lev, lab = S.dense_rows(N, K, L)
        n = len(lab)
        u = np.random.default_rng([N, K, l]).random((n, N + 1))
        flat = P.reshape(-1, L)
        # conditional on the class
        _, labels, logp, _ = S.walk(cores, l, phi, w, lab, u, given=lev)
        Pc = P / flat.sum(axis=0)
        assert np.array_equal(labels, lab)
        assert perr(logp[:, 0], Pc.ravel()) <= DENSE_TOL and np.array_equal(logp[:, 0], logp[:, 1])
        assert abs(np.exp(logp[:, 0]).sum() - L) <= 100 * DENSE_TOL
        # joint: the label drawn from P(l | x) with every pixel clamped
        _, labels, logp, _ = S.walk(cores, l, phi, w, np.full(n, -1), u, given=lev)
        assert perr(logp[:, 0], flat[np.arange(n) // L, labels]) <= DENSE_TOL
        # joint through the class weights
        clw = S.class_log_weights(cores, l, phi, w)
        assert np.abs(np.exp(clw) - flat.sum(axis=0)).max() <= 100 * DENSE_TOL
        # prefix split: column 1 is the log-probability of the prefix (given the class, or with the label outside the prefix)
        for g in range(1, N):
            levels, labels, logp, _ = S.walk(cores, l, phi, w, lab, u, given=lev[:, :g])
            marg = Pc.sum(axis=tuple(range(g, N)))                                   # (K,)*g + (L,)
            assert perr(logp[:, 1], marg[tuple(lev[:, i] for i in range(g)) + (lab,)]) <= DENSE_TOL
            assert perr(logp[:, 0], Pc[tuple(levels[:, i] for i in range(N)) + (lab,)]) <= DENSE_TOL
            if l >= g:
                _, _, logp, _ = S.walk(cores, l, phi, w, np.full(n, -1), u, given=lev[:, :g])
                marg = P.sum(axis=tuple(range(g, N + 1)))
                assert perr(logp[:, 1], marg[tuple(lev[:, i] for i in range(g))]) <= DENSE_TOL
        n_cases += 1
    assert n_cases >= 4 * 4 * 2 and {c[4] for c in dense_configs() if c[2] == 4} == {0, 1, 2, 3}


def test_hash_gives_reproducible_uniforms():
    u = S.hash_uniforms(7, 40, 17)
    assert u.shape == (40, 18) and u.dtype == np.float64 and np.all(u >= 0.0) and np.all(u < 1.0)
    assert np.array_equal(u, S.hash_uniforms(7, 40, 17)) and not np.array_equal(u, S.hash_uniforms(8, 40, 17))
    for seed, s, j, N in ((0, 0, 0, 1), (7, 39, 17, 17), (2 ** 64 - 1, 3, 784, 784), (12345, 4095, 2, 784)):
        assert S.hash_uniforms(seed, s + 1, N)[s, j] == S.hash_uniform_scalar(seed, s, j, N)
    big = S.hash_uniforms(1, 4096, 15)
    assert abs(big.mean() - 0.5) < 0.01 and len(np.unique(big)) == big.size


def test_gpu_cases_are_decidable_on_the_reference():
    """At least 95 % of the samples of every device case have every draw's margin >= 1e-9 (float64 differences between two
    summation orders are of order 1e-13): the draw cases, the wide bonds, the prefix cases."""
    worst, n = np.inf, 0
    cases = [(c, S.build_draw_case(c)) for c in S.draw_cases()] + [(c, S.build_wide_case(c)) for c in S.wide_cases()]
    for case, (cores, phi, w, classes, u) in cases:
        _, _, logp, mg = S.walk(cores, case[3], phi, w, classes, u)
        assert S.decidable(mg).mean() >= 0.95 and np.all(np.isfinite(logp)), case
        worst, n = min(worst, mg.min()), n + 1
    print('%d cases, smallest margin %.2e' % (n, worst))
    assert n == 53


def test_long_chains_are_decidable_on_the_reference():
    _, phi, w = S.grid(256, 2)
    classes = np.array([-1, 0, 1, -1] * (S.LONG_N // 4), dtype=np.int32)
    u = S.hash_uniforms(784, S.LONG_N, 784)
    for name, W, l in S.long_cases():
        _, _, logp, mg = S.walk(W, l, phi, w, classes, u)
        print('%s: smallest margin %.2e' % (name, mg.min()))
        assert S.decidable(mg).mean() >= 0.95 and np.all(np.isfinite(logp)), name


@pytest.mark.parametrize('case', S.FREQ_CASES, ids=lambda c: 'N%d_K%d_D%d_L%d_l%d' % c)
def test_frequencies_of_the_reference_stay_under_the_bound(case):
    """the chi-square of the device test, on the reference walk fed the same hashed uniforms"""
    N, K, D, L, l = case
    cores, phi, w = S.dense_case(D, L, N, K, l)
    P = S.dense_joint(cores, l, phi, w).ravel()
    lev, lab, _, _ = S.walk(cores, l, phi, w, np.full(S.FREQ_N, -1), S.hash_uniforms(S.FREQ_SEED, S.FREQ_N, N))
    chi2, dof = S.chi_square(S.outcome_counts(lev, lab, K, L), P, S.FREQ_N)
    print('chi2 %.1f at dof %d (bound %.1f)' % (chi2, dof, S.chi_bound(dof)))
    assert dof >= 1 and chi2 <= S.chi_bound(dof)


def test_call_is_declared_exported_and_bound():
    header = open(os.path.join(ROOT, 'include', 'tnml.h')).read()
    assert re.search(r'int tnml_sample\(tnml_ctx \*ctx, int n, int K, const double \*phi, const double \*w, const int32_t \*classes, '
                     r'const int32_t \*given,\s*int n_given, const double \*u, uint64_t seed, int32_t \*levels_out, int32_t \*labels_out, '
                     r'double \*logp_out\);', header)
    assert 'tnml_sample' in _hip.SYMBOLS and hasattr(_hip.lib(), 'tnml_sample') and len(_hip.lib().tnml_sample.argtypes) == 13
    assert callable(_hip.Context.sample)
    import tensornetworkforml_amd as pkg
    for m in ('sample', 'log_prob', 'class_log_weights'):
        assert callable(getattr(pkg.Network_class.Network, m))


def test_given_pixel_values_must_lie_on_the_grid():
    import tensornetworkforml_amd as pkg
    lv = pkg.Network_class.Network._levels_of
    x = np.arange(256) / 255.0
    k = np.array([[0, 255, 17], [3, 128, 254]])
    assert np.array_equal(lv(x[k], x, 'given'), k) and np.array_equal(lv(k, x, 'given'), k)
    assert np.array_equal(lv(x[k], x[::-1].copy(), 'given'), 255 - k)
    with pytest.raises(ValueError, match='not on the grid'):
        lv(x[k] + 1e-3, x, 'given')
    with pytest.raises(ValueError, match='shape'):
        lv(x[:3], x, 'given')


def test_sample_host_side_under_sanitizers():
    """csrc/Makefile target `san-sample`: tnml_sample of tnml_api.hip and the launch wrapper of kernels_sample.hip, built
    --cuda-host-only with -fsanitize=address,undefined, against the stand-in runtime of csrc/san/hip_stub.cpp
    (csrc/san/plan_sample_main.cpp, a stand-alone program): C3 and C5 at true size with the label at both ends and inside, a ragged
    17-site chain at every label position at D = 2, 3 and 8, N = 2, every refusal (none launches), and every allocation of the new
    group failing in turn."""
    import shutil
    import subprocess
    if shutil.which('g++') is None or not os.path.exists('/opt/rocm/bin/hipcc'):
        pytest.skip('no g++ / hipcc')
    csrc = os.path.join(ROOT, 'tensornetworkforml_amd', 'csrc')
    out = subprocess.run(['make', '-C', csrc, '-j4', 'san-sample'], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert 'sample host planning under ASan + UBSan: ok' in out.stdout
    for name in ('c3 bond 20 L 2, label on 0', 'c3 last bond 20', 'c3 inner label', 'c5 bond 50 L 10', 'c5 first', 'c5 inner label',
                 'ragged N 17 D 2', 'ragged N 17 D 3', 'ragged N 17 D 8', 'ragged N 2 D 2', 'sample refusals: ok', 'state rule after tnml_sample: ok', '0 live allocations'):
        assert name in out.stdout, name
    assert out.stdout.count('17 failed in turn') == 6
