"""Range-safe chains (include/tnml.h, tnml_set_chain_scaling / tnml_predict_scaled) without a GPU: the new
entry points in header / library / `_hip.SYMBOLS` / `Network`; the fixture of tests/scaled_chain_reference.py -- exactness of
`decalibrate`, and a float32 transcription of the plain chain that leaves float32 on the balanced pattern at every label site the
GPU test uses; the host side of the new calls under AddressSanitizer + UBSan (csrc/Makefile target `san-scaled`)."""
import os
import pickle
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import gradient_step_reference as R                                                          # noqa: E402
from core_grad_reference import core_grad_reference                                          # noqa: E402
from input_grad_reference import input_grad_reference, scaled_cores                          # noqa: E402
from scaled_chain_reference import BALANCED_N, balanced_pattern, decalibrate, plain_chain_float32    # noqa: E402
from test_any_position_host import label_inside_forward                                      # noqa: E402
from tensornetworkforml_amd import _hip                                                      # noqa: E402

BALANCED_ROWS = [(2, 5, 3), (3, 7, 3)]
BALANCED_LABELS = [0, 5, 8, 16]


def balanced_case(row, l, b=70):
    """(calibrated cores float32, decalibrated cores float32, X float32) of the balanced pattern for a row and a label site"""
    D, cap, L = row
    rng = np.random.default_rng([D, cap, L, l])
    X = R._features(rng, b, BALANCED_N, D)
    base = scaled_cores(BALANCED_N, D, L, [cap] * (BALANCED_N - 1), l, rng)
    med = np.median(np.abs(R.forward64(base, l, X.astype(np.float64))))
    cores = [(c * med ** (-1.0 / BALANCED_N)).astype(np.float32) for c in base]
    return cores, decalibrate(cores, balanced_pattern()), X


def as64(cores):
    return [c.astype(np.float64) for c in cores]


def test_calls_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, 'include', 'tnml.h')).read()
    assert re.search(r'int tnml_set_chain_scaling\(tnml_ctx \*ctx, int on\);', header)
    assert re.search(r'int tnml_predict_scaled\(tnml_ctx \*ctx, const float \*X, int b, float \*mant_out, int32_t \*expo_out\);', header)
    for s in ('tnml_set_chain_scaling', 'tnml_predict_scaled'):
        assert s in _hip.SYMBOLS and hasattr(_hip.lib(), s)
    for m in ('set_chain_scaling', 'predict_scaled'):
        assert callable(getattr(_hip.Context, m))
    import tensornetworkforml_amd as pkg
    assert callable(pkg.Network.predict_scaled) and isinstance(pkg.Network.scaled_chains, property)


def test_network_attribute_is_runtime_state():
    import tensornetworkforml_amd as pkg
    net = pkg.Network(N=6, M=3, D=2, L=2)
    assert net.scaled_chains is False
    net.scaled_chains = 1
    assert net.scaled_chains is True
    twin = pickle.loads(pickle.dumps(net))
    assert twin.scaled_chains is False                  # not pickled, like any_position
    assert 'scaled' not in ' '.join(net.__getstate__())


def test_scripts_take_the_flag():
    from tensornetworkforml_amd import evaluate_binary_MNIST, evaluate_diagonals, training_diagonals
    with pytest.raises(SystemExit):
        training_diagonals.main(['--scaled-chains'])                # only valid with --resident --optimizer
    with pytest.raises(SystemExit):
        training_diagonals.main(['--resident', '--scaled-chains'])
    for mod in (evaluate_diagonals, evaluate_binary_MNIST):
        with pytest.raises(FileNotFoundError):                      # the flag parses; the model file does not exist
            mod.main(['--scaled-chains', '--filename', os.path.join(ROOT, 'no_such_model.dat')])


@pytest.mark.parametrize('row', BALANCED_ROWS, ids=lambda r: 'D%d-cap%d-L%d' % r)
def test_decalibrate_is_exact_and_balanced(row):
    k = balanced_pattern()
    assert k.sum() == 0 and k[:8].sum() == 160 and k[9:].sum() == -160
    for l in BALANCED_LABELS:
        cores, dec, X = balanced_case(row, l)
        X64 = X.astype(np.float64)
        assert all(d.dtype == np.float32 for d in dec)
        for i, (c, d) in enumerate(zip(cores, dec)):
            assert np.array_equal(d.astype(np.float64), c.astype(np.float64) * 2.0 ** int(k[i]))
        # powers of two commute with every rounding of the float64 chain: f is bit-equal, by both references
        f_cal, f_dec = R.forward64(as64(cores), l, X64), R.forward64(as64(dec), l, X64)
        assert np.array_equal(f_cal, f_dec) and np.isfinite(f_cal).all() and 0.01 < np.median(np.abs(f_cal)) < 100
        assert np.array_equal(label_inside_forward(as64(cores), l, X64)[2], label_inside_forward(as64(dec), l, X64)[2])
        # g is the calibrated network's, G_i differs by 2^-k[i]
        cot = np.random.default_rng(l).standard_normal(f_cal.shape)
        g_cal, cf_cal = input_grad_reference(as64(cores), l, X64, cot)
        g_dec, cf_dec = input_grad_reference(as64(dec), l, X64, cot)
        assert np.array_equal(g_cal, g_dec) and np.array_equal(cf_cal, cf_dec)
        G_cal, _ = core_grad_reference(as64(cores), l, X64, cot)
        G_dec, _ = core_grad_reference(as64(dec), l, X64, cot)
        for i in range(BALANCED_N):
            assert np.array_equal(G_dec[i], G_cal[i] * 2.0 ** -int(k[i])), i


@pytest.mark.parametrize('row', BALANCED_ROWS, ids=lambda r: 'D%d-cap%d-L%d' % r)
def test_plain_float32_chain_leaves_the_range_on_the_balanced_pattern(row):
    """The fixture really is out of range: the float32 chain without renormalisation gives a non-finite or zero f for at least one
    sample at every label site of the GPU test, while on the calibrated cores it agrees with float64."""
    for l in BALANCED_LABELS:
        cores, dec, X = balanced_case(row, l)
        f64 = R.forward64(as64(cores), l, X.astype(np.float64))
        f_cal = plain_chain_float32(cores, l, X)
        assert np.abs(f_cal - f64).max() <= 2e-5 * np.abs(f64).max()
        f_dec = plain_chain_float32(dec, l, X)
        broken = ~np.isfinite(f_dec).all(axis=0) | (f_dec == 0).all(axis=0)
        print('plain float32 chain, D %d cap %d L %d, label site %2d: %d of %d samples non-finite or zero' % (*row, l, broken.sum(), broken.size))
        assert broken.any(), l


def test_scaled_chain_host_side_under_sanitizers():
    """csrc/Makefile target `san-scaled`: the new calls of tnml_api.hip and the launch wrappers of the three new kernels, built
    --cuda-host-only with -fsanitize=address,undefined, against the stand-in runtime of csrc/san/hip_stub.cpp
    (csrc/san/plan_scaled_main.cpp, a stand-alone program): C3 and C5 at true size in the default chunk and in chunks of 64 with the
    switch on, a ragged 17-site chain at every label position at D = 2, 3 and 8 through predict, predict_scaled, eval, both
    gradients and gd_step, every refusal, every allocation of the grown groups failing in turn; every launch of the new kernels
    has its pointers and extents checked, the exponent stacks and expo among them."""
    import shutil
    import subprocess
    if shutil.which('g++') is None or not os.path.exists('/opt/rocm/bin/hipcc'):
        pytest.skip('no g++ / hipcc')
    csrc = os.path.join(ROOT, 'tensornetworkforml_amd', 'csrc')
    out = subprocess.run(['make', '-C', csrc, '-j4', 'san-scaled'], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert 'scaled-chain host planning under ASan + UBSan: ok' in out.stdout
    for name in ('c3 bond 20 L 2 b 5000', 'c5 bond 50 L 10 b 5000', 'c5 inner label bond 50 L 10 b 200', 'ragged N 17 D 2', 'ragged N 17 D 3',
                 'ragged N 17 D 8'):
        assert 'planned scaled chains ' + name in out.stdout, name
    assert 'scaled-chain refusals: ok' in out.stdout
    assert out.stdout.count('tnml_predict_scaled, first use, b 70') == 2 and out.stdout.count('switch on over a plain group') == 6
    m = re.search(r'scaled chains: (\d+) scaled_pred_kernel, (\d+) input_grad_scaled_kernel and (\d+) core_grad_chain_scaled_kernel launches checked, '
                  r'(\d+) refusals', out.stdout)
    assert m and min(int(m.group(i)) for i in (1, 2, 3)) > 200 and int(m.group(4)) >= 18, out.stdout[-2000:]
    assert re.search(r'san-stub: \d+ launches checked \(\d+ kernels\), \d+ pointer extents checked, 0 live allocations', out.stdout)
