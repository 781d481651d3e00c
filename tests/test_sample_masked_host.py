"""The float64 reference of sampling given any set of known pixels (tests/sample_masked_reference.py) against a
dense enumeration and against the prefix walk of tests/sample_reference.py, the conditions that make the device comparisons of
tests/test_sample_masked_gpu.py decidable, the host side of tnml_sample_masked under the sanitizers, and the argument checks of the
Python wrappers that need no device."""
import itertools
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

import sample_masked_reference as M                                # noqa: E402
import sample_reference as S                                       # noqa: E402
from tensornetworkforml_amd import _hip                            # noqa: E402

# the reference against a dense table: both are float64 sums over the same few terms in different orders; the bound of the device
# tests against dense tables (tests/test_sample_gpu.py: the smallest probability of a table is ~1e-6 of the largest, the rest of a
# cancellation)
LOGP_TOL_DENSE = 4e-11


@pytest.mark.parametrize('N', [3, 4])
def test_reference_against_dense_enumeration(N):
    worst = [0.0, 0.0, 0.0]
    rows = 0
    for K, D, L in itertools.product([2, 3], [2, 3], [2, 3]):
        for l in range(N):
            cores, phi, w = S.dense_case(D, L, N, K, l)
            P = S.dense_joint(cores, l, phi, w)
            masks = M.all_masks(N)
            cls = list(range(-1, L))
            n = len(masks) * len(cls)
            rng = np.random.default_rng([51, N, K, D, L, l])
            mask = np.repeat(np.array(masks), len(cls), axis=0)
            classes = np.tile(np.array(cls), len(masks))
            known = rng.integers(0, K, (n, N))
            u = rng.random((n, N + 1))
            lev, lab, lp, _ = M.masked_walk(cores, l, phi, w, classes, u, mask, known)
            assert np.array_equal(lev[mask], known[mask]) and np.array_equal(lab[classes >= 0], classes[classes >= 0])
            for s in range(n):
                worst[0] = max(worst[0], abs(lp[s, 1] - math.log(M.dense_marginal(P, mask[s], known[s], classes[s]))))
                worst[1] = max(worst[1], abs(lp[s, 0] - math.log(M.dense_completion(P, mask[s], known[s], classes[s], lev[s], lab[s]))))
            empty = ~mask.any(axis=1)
            assert np.all(lp[empty, 1] == 0.0)                                                       # exactly
            clw = M.class_log_weights(cores, l, phi, w)
            worst[2] = max(worst[2], float(np.abs(clw - S.class_log_weights(cores, l, phi, w)).max()),
                           float(np.abs(clw - np.log(P.reshape(-1, L).sum(axis=0))).max()))
            rows += n
    print('N %d, %d rows: marginal %.2e completion %.2e class weights %.2e' % (N, rows, *worst))
    assert max(worst) <= LOGP_TOL_DENSE


def test_prefix_mask_against_the_prefix_walk():
    """equal levels and labels on the samples decidable in both; logp0_masked = logp0 - logp1 of the prefix walk where the class is
    given (with a drawn label inside the prefix the two condition the label differently: see the device test)"""
    worst = 0.0
    for ci in (3, 12, 25, 42):
        case = S.draw_cases()[ci]
        N, D, L, l, K = case
        cores, phi, w, classes, u = S.build_draw_case(case)
        _, _, known = M.ragged_inputs(ci, case)
        prefix = np.arange(N) < N // 2
        given = known[:, :N // 2]
        a = M.masked_walk(cores, l, phi, w, classes, u, prefix, known)
        b = S.walk(cores, l, phi, w, classes, u, given)
        ok = S.decidable(a[3]) & S.decidable(b[3])
        fixed = classes >= 0
        same = ok & (fixed | (l >= N // 2))
        assert same.sum() >= 0.4 * S.N_DRAWS
        assert np.array_equal(a[0][same], b[0][same]) and np.array_equal(a[1][same], b[1][same])
        sel = ok & fixed
        worst = max(worst, float(np.abs(a[2][sel, 0] - (b[2][sel, 0] - b[2][sel, 1])).max()))
    print('prefix: |logp0_masked - (logp0 - logp1)| %.2e' % worst)
    assert worst <= 2e-12                                                                             # LOGP_TOL_PREFIX of tests/test_sample_gpu.py


def test_gpu_cases_are_decidable_on_the_reference():
    """At least 95 % of the samples of every device case have every draw's margin >= 1e-9: the ragged cases with per-sample masks of
    density (0, 0.3, 0.7, 1)[s % 4] and with one shared mask, the wide bonds with a suffix and a random mask; all logs finite."""
    worst, n = np.inf, 0
    for ci, case in enumerate(S.draw_cases()):
        N, D, L, l, K = case
        cores, phi, w, classes, u = S.build_draw_case(case)
        mask, shared, known = M.ragged_inputs(ci, case)
        for m in (mask, shared):
            _, _, lp, mg = M.masked_walk(cores, l, phi, w, classes, u, m, known)
            assert S.decidable(mg).mean() >= 0.95 and np.all(np.isfinite(lp)), case
            worst, n = min(worst, mg.min()), n + 1
    for case in S.wide_cases():
        cores, phi, w, classes, u = S.build_wide_case(case)
        suffix, rnd, known = M.wide_inputs(case)
        for m in (suffix, rnd):
            _, _, lp, mg = M.masked_walk(cores, case[3], phi, w, classes, u, m, known)
            assert S.decidable(mg).mean() >= 0.95 and np.all(np.isfinite(lp)), case
            worst, n = min(worst, mg.min()), n + 1
    print('%d cases, smallest margin %.2e' % (n, worst))
    assert n == 106


@pytest.mark.parametrize('which', [0, 1], ids=['calibrated', 'raw'])
def test_long_chains_are_decidable_on_the_reference(which):
    _, phi, w = S.grid(256, 2)
    masks, known = M.long_inputs()
    u = S.hash_uniforms(784, M.LONG_N, 784)
    name, W, l = S.long_cases()[which]
    for mname, m in masks.items():
        _, _, lp, mg = M.masked_walk(W, l, phi, w, M.LONG_CLASSES, u, m, known)
        print('%s %s: smallest margin %.2e, logp about %.1f %.1f' % (name, mname, mg.min(), lp[:, 0].mean(), lp[:, 1].mean()))
        assert S.decidable(mg).mean() >= 0.95 and np.all(np.isfinite(lp)), (name, mname)
        if mname == 'empty':
            assert np.all(lp[:, 1] == 0.0)


@pytest.mark.parametrize('case', M.FREQ_MASKED, ids=lambda c: 'N%d_K%d_l%d' % (c[0], c[1], c[4]))
def test_frequencies_of_the_reference_stay_under_the_bound(case):
    """the chi-square of the device test, on the reference walk fed the same hashed uniforms"""
    N, K, D, L, l, sites = case
    cores, phi, w = S.dense_case(D, L, N, K, l)
    P = S.dense_joint(cores, l, phi, w)
    mask = np.zeros(N, dtype=bool)
    mask[list(sites)] = True
    known = np.zeros((S.FREQ_N, N), dtype=np.int32)
    known[:, list(sites)] = [(1 + j) % K for j in range(len(sites))]
    cond = P * 0.0
    idx = tuple(int(known[0, i]) if mask[i] else slice(None) for i in range(N))
    cond[idx] = P[idx]
    cond = (cond / cond.sum()).ravel()
    lev, lab, _, _ = M.masked_walk(cores, l, phi, w, np.full(S.FREQ_N, -1), S.hash_uniforms(S.FREQ_SEED, S.FREQ_N, N), mask, known)
    keep = cond > 0.0
    counts = S.outcome_counts(lev, lab, K, L)
    assert counts[~keep].sum() == 0
    chi2, dof = S.chi_square(counts[keep], cond[keep], S.FREQ_N)
    print('chi2 %.1f at dof %d (bound %.1f)' % (chi2, dof, S.chi_bound(dof)))
    assert dof >= 1 and chi2 <= S.chi_bound(dof)


def test_calls_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, 'include', 'tnml.h')).read()
    assert re.search(r'int tnml_sample_masked\(tnml_ctx \*ctx, int n, int K, const double \*phi, const double \*w, const int32_t \*classes, '
                     r'const uint8_t \*mask,\s*int mask_rows, const int32_t \*known, const double \*u, uint64_t seed, int draw, '
                     r'int32_t \*levels_out,\s*int32_t \*labels_out, double \*logp_out, double \*class_logw_out\);', header)
    assert re.search(r'int tnml_set_sample_stack_bytes\(tnml_ctx \*ctx, size_t bytes\);', header)
    assert 'are not supported' not in header[header.index('samples and log-likelihoods of the Born distribution'):]
    for name, nargs in (('tnml_sample_masked', 16), ('tnml_set_sample_stack_bytes', 2)):
        assert name in _hip.SYMBOLS and hasattr(_hip.lib(), name) and len(getattr(_hip.lib(), name).argtypes) == nargs
    assert callable(_hip.Context.sample_masked) and callable(_hip.Context.set_sample_stack_bytes)
    import tensornetworkforml_amd as pkg
    for m in ('sample', 'log_prob_masked', 'classify_masked'):
        assert callable(getattr(pkg.Network_class.Network, m))


def test_masked_levels_of_the_wrappers():
    """pixel values are read where the mask is set only; shapes are checked before any device call"""
    import tensornetworkforml_amd as pkg
    net = pkg.Network_class.Network.__new__(pkg.Network_class.Network)
    net.N = 3
    x = np.arange(256) / 255.0
    k = np.array([[0, 255, 17], [3, 128, 254]])
    mask = np.array([[True, False, True], [False, True, True]])
    X = x[k].copy()
    X[~mask] = 0.123456                                                                               # off the grid, but hidden
    m, lev = net._masked_levels(X, mask, x, 2)
    assert np.array_equal(m, mask) and np.array_equal(lev[mask], k[mask]) and lev.dtype == np.int32
    m, lev = net._masked_levels(k + 1000 * ~mask, mask, x, 2)                                         # integer levels
    assert np.array_equal(lev[mask], k[mask])
    m, lev = net._masked_levels(x[k], mask[0], x, 2)                                                  # one mask for all
    assert m.shape == (3,) and np.array_equal(lev[:, mask[0]], k[:, mask[0]])
    with pytest.raises(ValueError, match='not on the grid'):
        net._masked_levels(X, ~mask, x, 2)
    with pytest.raises(ValueError, match='mask has shape'):
        net._masked_levels(X, mask[:, :2], x, 2)
    with pytest.raises(ValueError, match='known values have shape'):
        net._masked_levels(X[:1], mask, x, 2)
    with pytest.raises(ValueError, match='needs their values'):
        net._masked_levels(None, mask, x, 2)
    assert net._masked_levels(None, np.zeros(3, dtype=bool), x, 2)[1] is None


def test_masked_sample_host_side_under_sanitizers():
    """csrc/Makefile target `san-masked`: tnml_sample_masked of tnml_api.hip and the launch wrapper of kernels_sample_masked.hip, built
    --cuda-host-only with -fsanitize=address,undefined, against the stand-in runtime of csrc/san/hip_stub.cpp
    (csrc/san/plan_masked_main.cpp, a stand-alone program): C3 and C5 at true size with the label at both ends and inside, a ragged
    17-site chain at every label position at D = 2, 3 and 8, N = 2, shared and per-sample masks of five kinds, draw 0 and 1, several
    chunks, every refusal (none launches), the state rule, and every allocation of the new group failing in turn."""
    import shutil
    import subprocess
    if shutil.which('g++') is None or not os.path.exists('/opt/rocm/bin/hipcc'):
        pytest.skip('no g++ / hipcc')
    csrc = os.path.join(ROOT, 'tensornetworkforml_amd', 'csrc')
    out = subprocess.run(['make', '-C', csrc, '-j4', 'san-masked'], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert 'masked sample host planning under ASan + UBSan: ok' in out.stdout
    for name in ('c3 bond 20 L 2, label on 0', 'c3 last bond 20', 'c3 inner label', 'c5 bond 50 L 10', 'c5 first', 'c5 inner label',
                 'ragged N 17 D 2', 'ragged N 17 D 3', 'ragged N 17 D 8', 'ragged N 2 D 2', 'masked sample refusals: ok',
                 'state rule after tnml_sample_masked: ok', '0 live allocations'):
        assert name in out.stdout, name
    assert out.stdout.count('15 failed in turn') == 10 and out.stdout.count(' 0 failed in turn') == 4
