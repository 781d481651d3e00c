"""Gradient training without a GPU (include/tnml.h, tnml_gd_train_indices): the float64 reference of the GPU
tests (tests/gradient_step_reference.py) against the plain update, the clip's bound and Adam's first step; the conditions on the
inputs of tests/test_gradient_step_gpu.py, asserted with the reference alone; the public surface; and the host side of the new calls
under AddressSanitizer + UBSan (csrc/Makefile target `san-optim`)."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import gradient_step_reference as R                                                          # noqa: E402
from core_grad_reference import core_grad_reference                                          # noqa: E402
from input_grad_reference import ragged_bonds, scaled_cores                                  # noqa: E402
from tensornetworkforml_amd import _hip                                                      # noqa: E402


def small_case(rng, N=6, D=2, L=3, cap=4, l=2, b=9):
    cores = scaled_cores(N, D, L, ragged_bonds(N, cap, rng), l, rng)
    return cores, l, rng.random((b, N, D)), rng.integers(0, L, b)


def test_forward_of_the_reference_is_the_core_gradient_chain():
    """forward64 against cf of core_grad_reference with a one-hot cotangent per label"""
    rng = np.random.default_rng(1)
    for l in (0, 2, 5):
        cores, _, X, _ = small_case(rng, l=l)
        f = R.forward64(cores, l, X)
        for k in range(3):
            cot = np.zeros((3, X.shape[0]))
            cot[k] = 1.0
            assert np.abs(core_grad_reference(cores, l, X, cot)[1] - f[k]).max() <= 1e-12 * np.abs(f).max()


@pytest.mark.parametrize('pair', [(a, lo) for a in R.ACTS for lo in R.LOSSES], ids=lambda p: '%s-%s' % p)
def test_plain_step_is_the_core_gradient(pair):
    """wd = 0, clip off, no momentum: the step equals A + lr * core_grad_reference(cores, l, X, loss derivative) exactly"""
    act, loss = pair
    rng = np.random.default_rng(2)
    cores, l, X, y = small_case(rng)
    ref = R.GradientStepReference(cores, l, clip=False)
    lr = 0.37
    info = ref.step(X, y, lr, 0.0, act, loss, 0.7)
    G, _ = core_grad_reference([c.copy() for c in cores], l, X, info['cot'])
    for a_new, a, g in zip(ref.cores, cores, G):
        assert np.array_equal(a_new, a + R.f32(lr) * g)


def test_clip_bounds_the_step_per_core():
    rng = np.random.default_rng(3)
    for wd in (0.0, 0.3):
        cores, l, X, y = small_case(rng, b=40)
        ref = R.GradientStepReference(cores, l)
        lr = 0.5
        info = ref.step(X, y, lr, wd, 'linear', 'MSE', 1.0)
        assert (info['ratio'] > 1).any()
        for a_new, a in zip(ref.cores, cores):
            assert np.abs(a_new - a).sum() <= lr * np.abs(a).sum() * (1 + 1e-12)


def test_adam_first_step_is_bounded_by_lr():
    rng = np.random.default_rng(4)
    cores, l, X, y = small_case(rng, b=40)
    ref = R.GradientStepReference(cores, l, kind='adam', clip=False)
    lr = 0.01
    ref.step(X, y, lr, 0.0, 'softmax', 'full_cross_ent', 0.5)
    assert max(np.abs(a_new - a).max() for a_new, a in zip(ref.cores, cores)) <= R.f32(lr) * (1 + 1e-12)
    # momentum: the second step of the same batch moves further than the first
    ref = R.GradientStepReference(cores, l, momentum=0.9, clip=False)
    ref.step(X, y, 1e-4, 0.0, 'linear', 'MSE', 1.0)
    first = [a.copy() for a in ref.cores]
    ref.step(X, y, 1e-4, 0.0, 'linear', 'MSE', 1.0)
    assert np.abs(ref.cores[0] - first[0]).sum() > np.abs(first[0] - cores[0]).sum()


@pytest.mark.parametrize('row', R.ROWS, ids=lambda r: 'D%d-cap%d-L%d' % r)
def test_input_conditions_of_the_gpu_cases(row):
    """What tests/test_gradient_step_gpu.py relies on, for every case and activation / loss pair of a row: the reference is finite;
    no core sits within CLIP_MARGIN of the clip's threshold; both outcomes of the clip occur in the row; the cross-entropy
    denominators stay SAFE away from zero; the step moves the cores by at least a tenth of max|A|."""
    clipped = unclipped = n = 0
    for case in R.row_cases(row):
        c64 = [c.astype(np.float64) for c in case['cores']]
        amax = max(np.abs(c).max() for c in c64)
        for act, loss in R.pairs_of(row):
            lr = R.case_lr(case, act, loss)
            ref = R.GradientStepReference(c64, case['l'])
            info = ref.step(case['X'], case['y'], lr, R.WD, act, loss, R.T_CASES)
            assert all(np.isfinite(c).all() for c in ref.cores) and np.isfinite(info['cot']).all()
            assert np.abs(info['ratio'] - 1).min() >= R.CLIP_MARGIN, (case['N'], case['l'], case['b'], act, loss)
            clipped += int((info['ratio'] > 1).sum())
            unclipped += int((info['ratio'] < 1).sum())
            fa, y = info['fa'], case['y']
            if loss == 'cross_entropy' and act != 'softmax':
                assert np.abs(fa[y, np.arange(y.size)]).min() >= R.SAFE
            if loss == 'full_cross_ent':
                z = fa - (np.arange(fa.shape[0])[:, None] != y[None, :])
                assert np.abs(z + 1e-4).min() >= R.SAFE
            assert max(np.abs(a - c).max() for a, c in zip(ref.cores, c64)) >= 0.1 * amax
            n += 1
    assert n == 36 * len(R.pairs_of(row)) and clipped > 0 and unclipped > 0, (n, clipped, unclipped)


def test_reference_training_run_learns():
    correct, acc0, acc1, _ = R.training_run_reference()
    print('float64 training run: correct per step %s, accuracy %.3f -> %.3f' % (correct, acc0, acc1))
    assert len(correct) == R.RUN['steps'] and acc1 > acc0


def test_calls_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, 'include', 'tnml.h')).read()
    assert re.search(r'enum \{ TNML_OPT_SGD = 0, TNML_OPT_ADAM = 1 \};', header)
    assert re.search(r'int tnml_optim_config\(tnml_ctx \*ctx, int kind, double momentum, double beta1, double beta2, double eps, int clip\);', header)
    assert re.search(r'int tnml_optim_reset\(tnml_ctx \*ctx\);', header)
    assert re.search(r'int tnml_gd_train_indices\(tnml_ctx \*ctx, const int32_t \*idx, int n, int batch, float lr, float weight_dec, int act_fn, '
                     r'int loss_fn,\s+float T, double \*metrics_out\);', header)
    assert re.search(r'int tnml_gd_step\(tnml_ctx \*ctx, const float \*X, const int32_t \*y, int b, float lr, float weight_dec, int act_fn, '
                     r'int loss_fn, float T,\s+double \*metrics3\);', header)
    for s in ('tnml_optim_config', 'tnml_optim_reset', 'tnml_gd_train_indices', 'tnml_gd_step'):
        assert s in _hip.SYMBOLS and hasattr(_hip.lib(), s)
    for m in ('optim_config', 'optim_reset', 'gd_train_indices', 'gd_step'):
        assert callable(getattr(_hip.Context, m))
    import tensornetworkforml_amd as pkg
    assert callable(pkg.Network.gradient_step) and callable(pkg.Network.train_gradient)
    from tensornetworkforml_amd import training_diagonals
    with pytest.raises(SystemExit):
        training_diagonals.main(['--optimizer', 'sgd'])           # only valid with --resident


def test_gradient_step_host_side_under_sanitizers():
    """csrc/Makefile target `san-optim`: the new calls of tnml_api.hip and the launch wrappers of kernels_optim.hip, built
    --cuda-host-only with -fsanitize=address,undefined, against the stand-in runtime of csrc/san/hip_stub.cpp
    (csrc/san/plan_optim_main.cpp, a stand-alone program): C3 and C5 at true size in the default chunk and in chunks of 64, a
    ragged chain at every label position at D = 2, 3 and 8, multi-step calls with a ragged last batch, every refusal, the
    tnml_optim_reset rule after a planned sweep, every allocation of the state group failing in turn; every launch of the two new
    kernels has its pointers and extents checked."""
    import shutil
    import subprocess
    if shutil.which('g++') is None or not os.path.exists('/opt/rocm/bin/hipcc'):
        pytest.skip('no g++ / hipcc')
    csrc = os.path.join(ROOT, 'tensornetworkforml_amd', 'csrc')
    out = subprocess.run(['make', '-C', csrc, '-j4', 'san-optim'], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert 'gradient-training host planning under ASan + UBSan: ok' in out.stdout
    for name in ('c3 bond 20 L 2 b 5000', 'c5 bond 50 L 10 b 5000', 'ragged N 17 D 2', 'ragged N 17 D 3', 'ragged N 17 D 8'):
        assert 'planned gradient training ' + name in out.stdout, name
    assert 'gradient-training refusals: ok' in out.stdout and 'optimiser state rule after a planned sweep: ok' in out.stdout
    assert out.stdout.count('tnml_gd_step, momentum, b 70') == 2
    m = re.search(r'gradient training: (\d+) loss_cot_kernel and (\d+) optim_step_kernel launches checked, (\d+) refusals', out.stdout)
    assert m and int(m.group(1)) > 200 and int(m.group(2)) > 200 and int(m.group(3)) >= 40, out.stdout[-2000:]
    assert re.search(r'san-stub: \d+ launches checked \(\d+ kernels\), \d+ pointer extents checked, 0 live allocations', out.stdout)
