"""The reference of tests/nll_step_reference.py checked on the CPU: descent of the short run, the growth of
the cores without renormalisation, the emulation tables the GPU bounds are read from, the conditions the shared cases must meet
(clip margin, label ratio, size of the move), the host side of the likelihood steps under sanitizers, the Python layer.
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p_ in (ROOT, HERE):
    if p_ not in sys.path:
        sys.path.insert(0, p_)

import nll_reference as N                                          # noqa: E402
import nll_step_reference as R                                     # noqa: E402


@pytest.fixture(scope='module')
def run():
    """the short run in float64 and in the emulation, computed once"""
    setup = R.training_run_setup()
    v64, ratios, ref64 = R.training_run(False, setup)
    v32, _, _ = R.training_run(True, setup)
    return setup, v64, ratios, ref64, v32


def test_descent(run):
    """N = 16, D = 2, L = 2, bond 4, 200 images with labels drawn from a teacher chain, batch 50, 20 SGD steps with renorm: the
    reference run goes down from first to last value, and on every batch from one epoch to the next"""
    setup, v64, ratios, ref64, _ = run
    assert len(v64) == R.RUN['steps'] == 20 and np.isfinite(v64).all()
    assert v64[-1] < v64[0]
    per_epoch = v64.reshape(5, 4)
    assert (np.diff(per_epoch, axis=0) < 0).all(), per_epoch
    # renorm: every core keeps its norm over the whole run (float64: to rounding)
    for a, c in zip(ref64.cores, setup[3]):
        assert abs((a * a).sum() / (c * c).sum() - 1.0) <= 1e-12


def test_ratio(run):
    """min_s |f_y| / max|f| >= nll_reference.MIN_RATIO for every batch used: the batch of every step of the run at the cores it
    meets, and (as tests/test_nll_host.py asserts them) the shared cases"""
    _, _, ratios, _, _ = run
    assert ratios.min() >= N.MIN_RATIO, ratios
    for lc in R.three_step_cases():
        cores, l, lev, lab, X, S = N.build_likelihood_case(lc)
        assert N.label_ratio(cores, l, X, lab) >= N.MIN_RATIO


def test_growth_without_renorm():
    """sum(G_i A_i) = 0 at every site, so with renorm off and plain SGD (no decay) every core's squared norm grows by lr^2 |G_i|^2"""
    for lc in R.three_step_cases()[:4]:
        case = R.StepCase(lc)
        for objective in R.OBJECTIVES:
            G = case.G[objective]
            lr = R.case_lr(case.cores, case.l, case.S, G, 'sgd')
            ref = R.NllStepReference(case.cores, case.l, case.S, renorm=False, **R.OPTIMS['sgd'])
            ref.apply(G, lr, 0.0)
            for a, c, g in zip(ref.cores, case.cores, G):
                grow, want = float((a * a).sum() - (c * c).sum()), R.f32(lr) ** 2 * float((g * g).sum())
                assert want > 0 and abs(grow - want) <= 1e-9 * max(want, float((c * c).sum())), (lc, grow, want)
            on = R.NllStepReference(case.cores, case.l, case.S, renorm=True, **R.OPTIMS['sgd'])
            on.apply(G, lr, 0.0)
            for a, c, p in zip(on.cores, case.cores, ref.cores):
                assert abs((a * a).sum() / (c * c).sum() - 1.0) <= 1e-13
                assert np.allclose(a, p * np.sqrt((c * c).sum() / (p * p).sum()), rtol=1e-13, atol=0)
    # lr = 0 leaves every core as it is, with and without renorm
    for renorm in (True, False):
        ref = R.NllStepReference(case.cores, case.l, case.S, renorm=renorm, emulate=True, **R.OPTIMS['sgd_clip_mom'])
        ref.apply(case.G['joint'], 0.0, R.WD)
        assert all(np.array_equal(a, c) for a, c in zip(ref.cores, case.cores))


@pytest.fixture(scope='module')
def step_figures():
    """per likelihood case: the emulation's figures, the clip ratios and the moves of test 1, computed once"""
    out = []
    for lc in N.likelihood_cases():
        case = R.StepCase(lc, emulation=True)
        amax = max(float(np.abs(c).max()) for c in case.cores)
        for cfg in R.configs():
            ref, lr = case.reference(cfg)
            emu, _ = case.reference(cfg, emulate=True)
            out.append((lc, cfg, R.step_deviation(emu.cores, ref.cores, case.cores), R.moved(ref.cores, case.cores) / amax,
                        ref.ratio if R.OPTIMS[cfg[1]]['clip'] else None, lr))
    return out


def test_step_emulation_table_is_what_the_code_gives(step_figures):
    worst = {}
    for lc, cfg, dev, _, _, _ in step_figures:
        key = (lc[0][:3], R.config_id(cfg))
        worst[key] = max(worst.get(key, 0.0), dev)
    assert set(worst) == {(tuple(r), R.config_id(c)) for r in N.ROWS for c in R.configs()}
    for (row, cid), v in worst.items():
        t = R.STEP_EMULATION[row][cid]
        assert abs(v - t) <= 0.25 * t, (row, cid, v, t)
    for row in N.ROWS:
        for cfg in R.configs():
            t = R.STEP_EMULATION[tuple(row)][R.config_id(cfg)]
            assert 10 * t <= R.step_bound(row, cfg) < 20 * t


def test_clip_and_move_conditions(step_figures):
    """conditions on the inputs: |s_d / s_A - 1| >= CLIP_MARGIN for every core of every clipped case, so that float32 cannot decide
    the clip differently; the largest change of every case at least MIN_MOVE of max|A|, so that the store's own rounding stays
    below the bound; lr a float32"""
    for lc, cfg, _, move, ratio, lr in step_figures:
        assert move >= R.MIN_MOVE, (lc, cfg, move)
        assert lr == R.f32(lr) and lr > 0
        if ratio is not None:
            assert np.abs(ratio - 1.0).min() >= R.CLIP_MARGIN, (lc, cfg, ratio)


def test_three_step_emulation_table_is_what_the_code_gives():
    worst = {}
    for lc in R.three_step_cases():
        for name, v in R.three_step_emulation_figures(lc).items():
            worst[(lc[0][:3], name)] = max(worst.get((lc[0][:3], name), 0.0), v)
    assert set(worst) == {(tuple(r), o) for r in N.ROWS for o in R.STATE_OPTIMS}
    for (row, name), v in worst.items():
        t = R.THREE_STEP_EMULATION[row][name]
        assert abs(v - t) <= 0.25 * t, (row, name, v, t)
        assert 10 * t <= R.three_step_bound(row, name) < 20 * t


def test_trajectory_emulation_is_what_the_code_gives(run):
    _, v64, _, _, v32 = run
    v = R.trajectory_deviation(v32, v64)
    assert abs(v - R.TRAJECTORY_EMULATION) <= 0.25 * R.TRAJECTORY_EMULATION, v
    assert 10 * R.TRAJECTORY_EMULATION <= R.trajectory_bound() < 20 * R.TRAJECTORY_EMULATION


def test_nll_step_host_side_under_sanitizers():
    """csrc/Makefile target `san-nll-step`: tnml_nll_step / tnml_nll_train_indices / tnml_set_nll_overlap of tnml_api.hip and the launch
    wrappers they reach, built --cuda-host-only with -fsanitize=address,undefined, against the stand-in runtime of
    csrc/san/hip_stub.cpp (csrc/san/plan_nll_step_main.cpp, a stand-alone program): C3 and C5 at true size, plain and with scaled
    chains, a ragged 17-site chain at every label position at D = 2, 3 and 8, both objectives in X and index form, chunks of 64,
    overlap and renorm on and off, every refusal (none launches), the state rules, every allocation of the new group failing in
    turn; and, in its own call trace, the event fork and join of every overlapped step."""
    import shutil
    import subprocess
    if shutil.which('g++') is None or not os.path.exists('/opt/rocm/bin/hipcc'):
        pytest.skip('no g++ / hipcc')
    csrc = os.path.join(ROOT, 'tensornetworkforml_amd', 'csrc')
    out = subprocess.run(['make', '-C', csrc, '-j4', 'san-nll-step'], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert 'likelihood step host planning under ASan + UBSan: ok' in out.stdout
    for name in ('c3 bond 20 L 2, label on 0', 'c3 inner label', 'c5 bond 50 L 10', 'c5 inner label', 'ragged N 17 D 2', 'ragged N 17 D 3',
                 'ragged N 17 D 8', 'likelihood step refusals: ok', 'state rules of the likelihood step: ok',
                 'each forked and joined by an event in the trace'):
        assert name in out.stdout, name
    assert out.stdout.count('0 live allocations') == 2
    assert 'ERROR' not in out.stderr and 'runtime error' not in out.stderr


def test_python_layer_without_a_device():
    from tensornetworkforml_amd import _hip
    import tensornetworkforml_amd as pkg
    for s_, n_ in (('tnml_nll_step', 9), ('tnml_nll_train_indices', 10), ('tnml_set_nll_overlap', 2)):
        assert s_ in _hip.SYMBOLS and len(getattr(_hip.lib(), s_).argtypes) == n_
    for m in ('nll_step', 'nll_train_indices', 'set_nll_overlap'):
        assert callable(getattr(_hip.Context, m))
    Network = pkg.Network_class.Network
    for m in ('nll_step', 'train_generative'):
        assert callable(getattr(Network, m))
    from tensornetworkforml_amd import training_diagonals
    with pytest.raises(SystemExit):
        training_diagonals.main(['--objective', 'nll'])             # needs --resident
    with pytest.raises(SystemExit):
        training_diagonals.main(['--resident', '--no-renorm'])      # needs --objective nll
