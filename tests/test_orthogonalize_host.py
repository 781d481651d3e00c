"""Orthogonal form, compression and bond spectra without a GPU: the float64 reference of
tests/orthogonalize_reference.py against itself on every input of tests/test_orthogonalize_gpu.py, the conditions that make the
device comparisons decidable, the declarations, and the host side of the new calls under sanitizers."""
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

import orthogonalize_reference as R                                                           # noqa: E402
from gradient_step_reference import forward64                                                 # noqa: E402
from tensornetworkforml_amd import _hip                                                       # noqa: E402


def all_inputs():
    """(name, cores, X, l) of every chain the GPU tests decompose without a cut"""
    for case in R.orth_cases():
        cores, X = R.build_case(case)
        yield case[0], cores, X, case[5]
    cores, X, l, _ = R.duplicated_column_case()
    yield 'duplicated_column', cores, X, l
    cores, X, l = R.long_chain_case()
    yield 'long_chain', cores, X, l


def no_sigma_near_rank_tol(log, name):
    for S, r0, m in log:
        rel = S / S[0]
        assert not ((rel > 1e-8) & (rel < 1e-4)).any(), (name, rel[(rel > 1e-8) & (rel < 1e-4)])


def test_reference_orthogonal_form_of_every_input():
    n = 0
    for name, cores, X, l in all_inputs():
        X64 = X.astype(np.float64)
        f0 = forward64(cores, l, X64)
        assert 0.5 <= np.abs(f0).max() <= 2.0, name              # calibrated to f of order 1
        log = []
        u, logn = R.orthogonalize(cores, l, log=log)
        no_sigma_near_rank_tol(log, name)
        assert R.isometry_defect(u, l) <= 1e-13, name
        f1 = forward64(R.with_gauge(u, logn)[0], l, X64)
        assert np.abs(f1 - f0).max() <= 1e-12 * len(cores), name
        # the compression without a cut is the orthogonal form: same bonds, same function, same log-norm
        log2 = []
        u2, spectra, disc, logn2 = R.compress(cores, l, 10 ** 6, 1.0, log=log2)
        no_sigma_near_rank_tol(log2, name)
        assert R.bonds_of(u2) == R.bonds_of(u) and abs(logn2 - logn) <= 1e-12 * len(cores) and not disc.any(), name
        assert np.abs(forward64(R.with_gauge(u2, logn2)[0], l, X64) - f0).max() <= 1e-12 * len(cores), name
        assert all(abs((s ** 2).sum() - 1.0) <= 1e-13 for s in spectra), name
        ranks, _, logn3 = R.bond_spectra(cores, l)
        assert ranks == R.bonds_of(u) and logn3 == logn2, name
        # a bond never stays larger than the rows or columns of the matrix it cuts
        D = cores[0].shape[1]
        for i, b in enumerate(R.bonds_of(u)):
            Ll = cores[l].shape[3] if l <= i else 1
            Lr = cores[l].shape[3] if l > i else 1
            assert b <= min(D ** (i + 1) * Ll, D ** (len(cores) - 1 - i) * Lr), (name, i, b)
        n += 1
    assert n == len(R.orth_cases()) + 2


def test_duplicated_column_drops_the_bond_by_one():
    cores, X, l, k = R.duplicated_column_case()
    u, _ = R.orthogonalize(cores, l)
    want = R.bonds_of(cores)
    want[k] -= 1
    assert R.bonds_of(u)[3:13] == want[3:13]
    assert R.bond_spectra(cores, l)[0][k] == want[k]


def test_compression_cases_meet_their_conditions():
    for case in R.COMPRESS_CASES:
        name, (D, cap, L), N, l, m_max, thr = case
        cores, X = R.build_compress_case(case)
        X64 = X.astype(np.float64)
        f0 = forward64(cores, l, X64)
        log, cuts = [], []
        u, spectra, disc, logn = R.compress(cores, l, m_max, thr, log=log, cuts=cuts)
        no_sigma_near_rank_tol(log, name)
        n_cut = 0
        for (S, m), d in zip(cuts, disc):
            if m < len(S):
                assert S[m - 1] / S[m] >= 1.05, (name, S[m - 1] / S[m])
                n_cut += 1
            if thr < 1.0:
                cum = np.cumsum(S) / S.sum()
                ma = int(np.argmax(cum > thr)) + 1
                if ma <= min(m_max, len(S)):                    # the adaptive rule decides (or ties with) this bond
                    assert cum[ma - 1] - thr >= 1e-3 and (ma < 2 or thr - cum[ma - 2] >= 1e-3), (name, cum[ma - 1], thr)
            assert abs(d - (S[m:] ** 2).sum()) <= 1e-15
        assert n_cut >= 1 and max(R.bonds_of(u)) <= m_max, name
        # `discarded` is the lost norm: the chain's squared norm falls by the discarded share at every cut
        _, logn0 = R.orthogonalize(cores, l)
        assert abs(2 * (logn - logn0) - np.log1p(-disc).sum()) <= 1e-10, name
        f1 = forward64(R.with_gauge(u, logn)[0], l, X64)
        move = np.abs(f1 - f0).max() / np.abs(f0).max()
        print('%s: bonds %s, f moves by %.3g of max|f|' % (name, R.bonds_of(u), move))
        assert 1e-3 <= move <= 0.5, (name, move)
        assert R.isometry_defect(u, l) <= 1e-13, name


def test_calls_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, 'include', 'tnml.h')).read()
    assert re.search(r'int tnml_orthogonalize\(tnml_ctx \*ctx, double rank_tol, int32_t \*bond_out, double \*log_norm_out\);', header)
    assert re.search(r'int tnml_compress\(tnml_ctx \*ctx, int m_max, double threshold, double rank_tol, int32_t \*bond_out, double \*sigma_out,'
                     r'\s+double \*discarded_out, double \*log_norm_out\);', header)
    assert re.search(r'int tnml_bond_spectra\(tnml_ctx \*ctx, double rank_tol, int32_t \*rank_out, double \*sigma_out, double \*log_norm_out\);', header)
    for s in ('tnml_orthogonalize', 'tnml_compress', 'tnml_bond_spectra'):
        assert s in _hip.SYMBOLS and hasattr(_hip.lib(), s)
    for m in ('orthogonalize', 'compress', 'bond_spectra'):
        assert callable(getattr(_hip.Context, m))
    import tensornetworkforml_amd as pkg
    for m in ('orthogonalize', 'compress', 'bond_spectra'):
        assert callable(getattr(pkg.Network, m))
    with pytest.raises(ValueError):
        pkg.Network.compress(object.__new__(pkg.Network))       # neither bound given: refused before anything is touched


def test_orthogonal_form_host_side_under_sanitizers():
    """csrc/Makefile target `san-orth`: the calls of api_mps.hip and the launch wrapper of kernels_orth.hip, built
    --cuda-host-only with -fsanitize=address,undefined, against the stand-in runtime of csrc/san/hip_stub.cpp
    (csrc/san/plan_orth_main.cpp, a stand-alone program): C3 and C5 at true size, a ragged chain at every label position at
    D = 2, 3 and 8, all three calls, every refusal, the optimiser-state rule after a committed call, every allocation of the scratch
    group failing in turn; every launch of the three new kernels has its pointers and extents checked."""
    import shutil
    import subprocess
    if shutil.which('g++') is None or not os.path.exists('/opt/rocm/bin/hipcc'):
        pytest.skip('no g++ / hipcc')
    csrc = os.path.join(ROOT, 'tensornetworkforml_amd', 'csrc')
    out = subprocess.run(['make', '-C', csrc, '-j4', 'san-orth'], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert 'orthogonal-form host planning under ASan + UBSan: ok' in out.stdout
    for name in ('c3 bond 20 L 2', 'c5 bond 50 L 10', 'ragged N 17 D 2', 'ragged N 17 D 3', 'ragged N 17 D 8'):
        assert 'planned orthogonal form ' + name in out.stdout, name
    assert 'orthogonal-form refusals: ok' in out.stdout and 'optimiser state rule after a committed call: ok' in out.stdout
    m = re.search(r'orthogonal form: (\d+) orth_chain_kernel launches checked, (\d+) refusals', out.stdout)
    assert m and int(m.group(1)) > 100 and int(m.group(2)) >= 12, out.stdout[-2000:]
    assert re.search(r'san-stub: \d+ launches checked \(\d+ kernels\), \d+ pointer extents checked, 0 live allocations', out.stdout)
