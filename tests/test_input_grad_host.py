"""Input gradients without a GPU (include/tnml.h, tnml_input_grad): the float64 reference of the GPU tests
(tests/input_grad_reference.py) against the unit-step identity and an independent forward, the analytic derivative of the pixel
feature map against central differences, the public surface, and the host side of the new calls under AddressSanitizer + UBSan
(csrc/Makefile target `san-inputgrad`)."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from input_grad_reference import dpsi, input_grad_reference, ragged_bonds, scaled_cores    # noqa: E402
from test_any_position_host import label_inside_forward                                      # noqa: E402
from tensornetworkforml_amd import _hip                                                      # noqa: E402
from tensornetworkforml_amd import data_generator as gen                                     # noqa: E402


def label_sites(N):
    return sorted({0, N // 2, N - 1} | ({1, N - 2} if N > 3 else set()))


@pytest.mark.parametrize('L', [1, 3, 10])
@pytest.mark.parametrize('D', [2, 3, 8])
@pytest.mark.parametrize('N', [2, 3, 17])
def test_reference_meets_the_unit_step_identity(N, D, L):
    """f is linear in every x[s][i][:], so f(x + e_{i,d}) - f(x) = g[i][d] with no truncation error: the reference's g against
    differences of an independent forward (label_inside_forward), within 1e-12 of max|g| (float64 reached 3e-15), and its cf
    against sum_l cot f of the same forward.  Ragged bonds, the label at both ends and inside."""
    rng = np.random.default_rng(1000 * N + 10 * D + L)
    b, worst = 3, 0.0
    for l in label_sites(N):
        bond = ragged_bonds(N, 5, rng)
        cores = scaled_cores(N, D, L, bond, l, rng)
        X = rng.random((b, N, D))
        cot = rng.standard_normal((L, b))
        g, cf = input_grad_reference(cores, l, X, cot)
        f0 = label_inside_forward(cores, l, X)[2]
        cf0 = (cot * f0).sum(0)
        scale = np.abs(g).max()
        assert scale > 0
        assert np.abs(cf - cf0).max() <= 1e-12 * np.abs(cf0).max()
        # one batch of b N D perturbed copies: sample s, site i, feature d
        Xp = np.repeat(X[:, None, None], N, 1).repeat(D, 2)
        for i in range(N):
            for d in range(D):
                Xp[:, i, d, i, d] += 1.0
        fp = label_inside_forward(cores, l, Xp.reshape(b * N * D, N, D))[2].reshape(L, b, N, D)
        diff = np.einsum('lb,lbnd->bnd', cot, fp) - cf0[:, None, None]
        worst = max(worst, np.abs(diff - g).max() / scale)
        # f is homogeneous of degree 1 in every site's vector
        assert np.abs(np.einsum('bnd,bnd->bn', g, X) - cf[:, None]).max() <= 1e-12 * scale
    print('unit-step identity N %d D %d L %d: worst %.2e of max|g|' % (N, D, L, worst))
    assert worst <= 1e-12


@pytest.mark.parametrize('D', range(2, 9))
def test_dpsi_against_central_differences(D):
    p = np.array([[0.0, 0.3, 1.0]])
    h = 1e-6
    fd = (gen.psi(p + h, D) - gen.psi(p - h, D)) / (2 * h)
    err = np.abs(dpsi(p, D) - fd).max()
    print('dpsi D %d: %.2e' % (D, err))
    assert dpsi(p, D).shape == (1, 3, D)
    assert err <= 1e-8


def test_calls_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, 'include', 'tnml.h')).read()
    assert re.search(r'int tnml_input_grad\(tnml_ctx \*ctx, const float \*X, int b, const float \*cot, float \*grad_out, float \*cf_out\);', header)
    assert re.search(r'int tnml_input_grad_indices\(tnml_ctx \*ctx, const int32_t \*idx, int b, const float \*cot, int wrt, float \*grad_out, '
                     r'float \*cf_out\);', header)
    assert re.search(r'int tnml_set_input_grad_chunk\(tnml_ctx \*ctx, int samples\);', header)
    for s in ('tnml_input_grad', 'tnml_input_grad_indices', 'tnml_set_input_grad_chunk'):
        assert s in _hip.SYMBOLS and hasattr(_hip.lib(), s)
    for m in ('input_grad', 'input_grad_indices', 'set_input_grad_chunk'):
        assert callable(getattr(_hip.Context, m))
    import tensornetworkforml_amd as pkg
    assert callable(pkg.Network.input_gradient) and callable(pkg.Network.input_gradient_indices)


def test_cotangent_forms():
    import tensornetworkforml_amd as pkg
    np.random.seed(1)
    net = pkg.Network(N=5, M=3, L=3, act_fn='softmax', loss_fn='full_cross_ent', trunc='fixed')
    assert net._cotangent(None, 4) is None
    oh = net._cotangent(np.array([2, 0, 1, 2]), 4)
    assert oh.dtype == np.float32 and np.array_equal(oh, np.eye(3, dtype=np.float32)[:, [2, 0, 1, 2]])
    dense = np.arange(12.0).reshape(3, 4)
    assert np.array_equal(net._cotangent(dense, 4), dense.astype(np.float32))
    with pytest.raises(AssertionError):
        net._cotangent(np.array([0, 3, 0, 0]), 4)
    with pytest.raises(AssertionError):
        net._cotangent(np.zeros((4, 3)), 4)


def test_input_grad_host_side_under_sanitizers():
    """csrc/Makefile target `san-inputgrad`: tnml_input_grad / tnml_input_grad_indices of tnml_api.hip and the launch wrappers of
    kernels_inputgrad.hip, built --cuda-host-only with -fsanitize=address,undefined, against the stand-in runtime of
    csrc/san/hip_stub.cpp (csrc/san/plan_inputgrad_main.cpp, a stand-alone program): C3 and C5 at true size in one and in many
    chunks, a ragged chain at every label position at D = 2, 3 and 8, one sample, both dataset forms, every refusal, every
    allocation of the new group failing in turn; every launch of the new kernels has its pointers and extents checked."""
    import shutil
    import subprocess
    if shutil.which('g++') is None or not os.path.exists('/opt/rocm/bin/hipcc'):
        pytest.skip('no g++ / hipcc')
    csrc = os.path.join(ROOT, 'tensornetworkforml_amd', 'csrc')
    out = subprocess.run(['make', '-C', csrc, '-j4', 'san-inputgrad'], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert 'input-gradient host planning under ASan + UBSan: ok' in out.stdout
    for name in ('c3 bond 20 L 2 b 5000', 'c5 bond 50 L 10 b 5000', 'ragged N 17 D 2', 'ragged N 17 D 3', 'ragged N 17 D 8'):
        assert 'planned input gradients ' + name in out.stdout, name
    m = re.search(r'input gradients: (\d+) input_grad_kernel launches checked, (\d+) refusals', out.stdout)
    assert m and int(m.group(1)) > 200 and int(m.group(2)) >= 10, out.stdout[-2000:]
    assert re.search(r'san-stub: \d+ launches checked \(\d+ kernels\), \d+ pointer extents checked, 0 live allocations', out.stdout)
