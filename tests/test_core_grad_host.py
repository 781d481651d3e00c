"""Core gradients without a GPU (include/tnml.h, tnml_core_grad): the float64 reference of the GPU tests
(tests/core_grad_reference.py) against the unit-step identity and the Euler identity on an independent forward, the public
surface, and the host side of the new calls under AddressSanitizer + UBSan (csrc/Makefile target `san-coregrad`)."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from core_grad_reference import core_grad_reference                                          # noqa: E402
from input_grad_reference import ragged_bonds, scaled_cores                                  # noqa: E402
from test_any_position_host import label_inside_forward                                      # noqa: E402
from tensornetworkforml_amd import _hip                                                      # noqa: E402


def label_sites(N):
    return sorted({0, N // 2, N - 1} | ({1, N - 2} if N > 3 else set()))


@pytest.mark.parametrize('L', [1, 3, 10])
@pytest.mark.parametrize('D', [2, 3, 8])
@pytest.mark.parametrize('N', [2, 3, 17])
def test_reference_meets_the_unit_step_and_euler_identities(N, D, L):
    """f is linear in every core, so sum(cot f(A + e)) - sum(cot f(A)) = G[e] for a unit step e on one element, with no truncation
    error: one random element of every core against an independent forward (label_inside_forward), within 1e-10 of max|G|.
    f is homogeneous of degree 1 in every core: sum(G_i A_i) = sum_s cf[s] for every site, within 1e-10 of sum_s |cf[s]| (float64
    rounding of sums of a few thousand terms is below 1e-12; a wrong formula misses by O(1)).  Ragged bonds, the label at both
    ends and inside."""
    rng = np.random.default_rng(2000 * N + 10 * D + L)
    b, worst_step, worst_euler = 5, 0.0, 0.0
    for l in label_sites(N):
        bond = ragged_bonds(N, 5, rng)
        cores = scaled_cores(N, D, L, bond, l, rng)
        X = rng.random((b, N, D))
        cot = rng.standard_normal((L, b))
        G, cf = core_grad_reference(cores, l, X, cot)
        assert [g.shape for g in G] == [c.shape for c in cores]
        f0 = label_inside_forward(cores, l, X)[2]
        total0 = (cot * f0).sum()
        assert np.abs(cf - (cot * f0).sum(0)).max() <= 1e-12 * np.abs(cf).max()
        scale = max(np.abs(g).max() for g in G)
        assert scale > 0
        for i in range(N):
            e = tuple(int(rng.integers(0, n)) for n in cores[i].shape)
            stepped = [c.copy() for c in cores]
            stepped[i][e] += 1.0
            diff = (cot * label_inside_forward(stepped, l, X)[2]).sum() - total0
            worst_step = max(worst_step, abs(diff - G[i][e]) / scale)
            worst_euler = max(worst_euler, abs((G[i] * cores[i]).sum() - cf.sum()) / np.abs(cf).sum())
    print('N %d D %d L %d: unit step %.2e of max|G|, Euler %.2e of sum|cf|' % (N, D, L, worst_step, worst_euler))
    assert worst_step <= 1e-10 and worst_euler <= 1e-10


def test_calls_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, 'include', 'tnml.h')).read()
    assert re.search(r'int tnml_core_grad\(tnml_ctx \*ctx, const float \*X, int b, const float \*cot, float \*grad_flat, size_t capacity, '
                     r'float \*cf_out\);', header)
    assert re.search(r'int tnml_core_grad_indices\(tnml_ctx \*ctx, const int32_t \*idx, int b, const float \*cot, float \*grad_flat, '
                     r'size_t capacity, float \*cf_out\);', header)
    assert re.search(r'int tnml_set_core_grad_chunk\(tnml_ctx \*ctx, int samples\);', header)
    for s in ('tnml_core_grad', 'tnml_core_grad_indices', 'tnml_set_core_grad_chunk'):
        assert s in _hip.SYMBOLS and hasattr(_hip.lib(), s)
    for m in ('core_grad', 'core_grad_indices', 'set_core_grad_chunk'):
        assert callable(getattr(_hip.Context, m))
    import tensornetworkforml_amd as pkg
    assert callable(pkg.Network.core_gradient) and callable(pkg.Network.core_gradient_indices)


def test_core_grad_host_side_under_sanitizers():
    """csrc/Makefile target `san-coregrad`: tnml_core_grad / tnml_core_grad_indices of tnml_api.hip and the launch wrappers of
    kernels_coregrad.hip, built --cuda-host-only with -fsanitize=address,undefined, against the stand-in runtime of
    csrc/san/hip_stub.cpp (csrc/san/plan_coregrad_main.cpp, a stand-alone program): C3 and C5 at true size in the default chunk and
    in chunks of 64, a ragged chain at every label position at D = 2, 3 and 8, one sample, dataset samples, every refusal, every
    allocation of the new group failing in turn at first use and at growth; every launch of the two new kernels has its pointers
    and extents checked."""
    import shutil
    import subprocess
    if shutil.which('g++') is None or not os.path.exists('/opt/rocm/bin/hipcc'):
        pytest.skip('no g++ / hipcc')
    csrc = os.path.join(ROOT, 'tensornetworkforml_amd', 'csrc')
    out = subprocess.run(['make', '-C', csrc, '-j4', 'san-coregrad'], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert 'core-gradient host planning under ASan + UBSan: ok' in out.stdout
    for name in ('c3 bond 20 L 2 b 5000', 'c5 bond 50 L 10 b 5000', 'ragged N 17 D 2', 'ragged N 17 D 3', 'ragged N 17 D 8'):
        assert 'planned core gradients ' + name in out.stdout, name
    assert out.stdout.count('tnml_core_grad, b 70  ') == 2 and out.stdout.count('tnml_core_grad, b 70 -> 300') == 2
    m = re.search(r'core gradients: (\d+) core_grad_chain_kernel and (\d+) core_grad_reduce_kernel launches checked, (\d+) refusals', out.stdout)
    assert m and int(m.group(1)) > 200 and m.group(1) == m.group(2) and int(m.group(3)) >= 20, out.stdout[-2000:]
    assert re.search(r'san-stub: \d+ launches checked \(\d+ kernels\), \d+ pointer extents checked, 0 live allocations', out.stdout)
