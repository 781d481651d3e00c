"""Local feature dimension D != 2 without a GPU: the context accepts 3 <= D <= 8 up to the device check, the generalised
feature map, and the D = 2 map unchanged."""
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def hip():
    from tensornetworkforml_amd import _hip
    return _hip


def _no_gpu():
    try:
        return hip().device_count() == 0
    except Exception:
        return True


@pytest.mark.skipif(not _no_gpu(), reason="the device check only fails where there is no GPU")
@pytest.mark.parametrize('D', [3, 4, 8])
def test_supported_D_reaches_the_device_check(D):
    with pytest.raises(hip().TnmlError) as ei:
        hip().Context(8, D, 2, 4, 16)
    assert ei.value.code == -4


@pytest.mark.parametrize('D', [1, 9])
def test_unsupported_D_is_an_argument_error(D):
    with pytest.raises(hip().TnmlError) as ei:
        hip().Context(8, D, 2, 4, 16)
    assert ei.value.code == -1
    assert '[2, 8]' in str(ei.value)


def test_psi_known_values_D3_D4():
    from tensornetworkforml_amd import data_generator as gen
    x = np.array([[0.0, 0.5, 1.0]])
    s, c = np.sin(np.pi * x / 2), np.cos(np.pi * x / 2)
    p3 = gen.psi(x, 3)
    assert p3.shape == (1, 3, 3)
    np.testing.assert_allclose(p3[..., 0], s ** 2, atol=1e-15)
    np.testing.assert_allclose(p3[..., 1], math.sqrt(2) * s * c, atol=1e-15)
    np.testing.assert_allclose(p3[..., 2], c ** 2, atol=1e-15)
    np.testing.assert_allclose(p3[0, 1], [0.5, math.sqrt(2) * 0.5, 0.5], atol=1e-15)      # x = 0.5: sin = cos = 1/sqrt(2)
    p4 = gen.psi(x, 4)
    np.testing.assert_allclose(p4[0, 0], [0.0, 0.0, 0.0, 1.0], atol=1e-15)                  # x = 0: sin = 0, cos = 1
    np.testing.assert_allclose(p4[0, 2], [1.0, 0.0, 0.0, 0.0], atol=1e-15)                  # x = 1
    np.testing.assert_allclose(p4[0, 1], np.sqrt([1, 3, 3, 1]) / 2 ** 1.5, atol=1e-15)


@pytest.mark.parametrize('D', [2, 3, 4, 5, 8])
def test_psi_components_square_sum_to_one(D):
    from tensornetworkforml_amd import data_generator as gen
    u = np.random.default_rng(0).random((7, 11))
    p = gen.psi(u, D)
    assert p.shape == (7, 11, D)
    np.testing.assert_allclose((p ** 2).sum(-1), 1.0, atol=1e-13)


def test_psi_D2_bit_identical():
    from tensornetworkforml_amd import data_generator as gen
    u = np.random.default_rng(1).random((5, 9))
    assert np.array_equal(gen.psi(u, 2), gen.psi(u))
    ref = np.transpose(np.array((np.sin(np.pi * u / 2), np.cos(np.pi * u / 2))), [1, 2, 0])
    assert np.array_equal(gen.psi(u), ref)


def test_prepare_dataset_takes_D():
    from tensornetworkforml_amd import data_generator as gen
    np.random.seed(0)
    data, label = gen.create_dataset(40, 4, 0.5)
    tl, vl, _ = gen.prepare_dataset(data, label, 1, 0.25, 10, 10, 10, D=3)
    assert next(iter(tl)).X.shape == (10, 16, 3)
    tl2, _, _ = gen.prepare_dataset(data, label, 1, 0.25, 10, 10, 10)
    assert next(iter(tl2)).X.shape == (10, 16, 2)


def test_trunc_rank_takes_D():
    # the planning arithmetic the generic-D path shares with D = 2 (host_plan.inc)
    assert hip().trunc_rank('fixed', 0, 0, 10, 1, 3, 20, 2, 20) == 3          # rows = 3 at the chain end
    assert hip().trunc_rank('fixed', 0, 3, 10, 20, 3, 20, 2, 20) == 20
    assert hip().trunc_rank('reference', 0, 0, 10, 1, 3, 20, 2, 20) == 3


def test_generic_D_host_side_under_sanitizers():
    """csrc/Makefile target `san-anyd`: the host side of the generic-D path (sweep_anyd / standalone_anyd of tnml_api.hip and the
    launch wrappers of kernels_anyd.hip, built --cuda-host-only with -fsanitize=address,undefined) against the stand-in runtime of
    csrc/san/hip_stub.cpp, with every kernels_anyd.hip launch's argument extents checked at its D (csrc/san/plan_anyd_main.cpp):
    whole sweeps at D = 3 / 4 / 8 under the fixed, reference and adaptive policies, forward, predict, calibration, update_B,
    l2_term, svd_split, one shape at the 128 limit and one beyond it."""
    import re
    import shutil
    import subprocess
    if shutil.which('g++') is None or not os.path.exists('/opt/rocm/bin/hipcc'):
        pytest.skip('no g++ / hipcc')
    csrc = os.path.join(ROOT, 'tensornetworkforml_amd', 'csrc')
    out = subprocess.run(['make', '-C', csrc, '-j4', 'san-anyd'], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert 'generic-D host planning under ASan + UBSan: ok' in out.stdout
    assert 'bond 33 refused at step 3' in out.stdout
    m = re.search(r'generic-D launches: (\d+) argument extents checked', out.stdout)
    assert m and int(m.group(1)) > 5000, out.stdout[-2000:]
    assert re.search(r'san-stub: \d+ launches checked \(\d+ kernels\), \d+ pointer extents checked, 0 live allocations', out.stdout)
