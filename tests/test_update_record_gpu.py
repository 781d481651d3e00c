"""The update workgroup reads its step record field by field (kernels_narrow.hip: StepArgs / PersistArgs): every path
through narrow_body on a chain whose consecutive steps differ in every field of the record.

What such a change can break is a field taken from another step's record or from a stale copy, so the shape is a ramp:
N = 10, bond 5, three labels, 33 samples.  From the all-5 start the behind bond of a sweep runs 1, 2, 4, 5, ..., the far end
4, 2, 1 in the next direction, 5 is odd, and 33 samples are one full tile and one sample.  Three CONSECUTIVE sweeps
(right, left, right) rewrite the ring of record buffers between launches.

Bounds are those of the existing tests of the same paths (helpers of test_timed_paths_gpu.py):
  persistent sweep, L2 term on       test_persistent_sweep_step_by_step: its sweep-1 bounds for the sweep from the calibrated
                                     start, its sweep-2 bounds for every later sweep -- like its sweep 2, sweeps 2 and 3 here
                                     continue on the device and restart the oracle from the device's cores, so each is ONE
                                     sweep of rounding from a common, uncalibrated state
  persistent sweep, L2 term off      test_persistent_sweep_activations_and_losses (the existing test of that switch), same rule
  mode 0 (one launch per step)       the same bounds as mode 1: the same quantities, float32 sums in another order
  classic sequence, adaptive rank    test_hip_parity.py: sigma 5e-4 of sigma_max, f 5e-3, accuracy within 2 samples, MAE 2e-3
  standalone update_B                test_hip_parity.py: captured tensors 5e-3 of max|.|, accuracy exact
Each test prints what it observed before it asserts.  Observed on MI355X (worst over modes 1 and 0, L2 on and off):
  three sweeps   sweep 1 sigma 7.5e-8, off-diagonal 3.5e-7, environments 3.0e-7, f 4.1e-7, MAE 8.5e-8; sweeps 2 and 3 sigma 6.5e-7,
                 off-diagonal 3.1e-7, environments 5.8e-7, f 5.6e-7, MAE 1.0e-7; accuracy exact in all (modes 1 and 2 bit-equal)
  classic        sigma 3.9e-7, f 4.7e-7, MAE 5.3e-8;  adaptive: sigma 3.9e-6, f 2.5e-6, MAE 1.8e-7, kept ranks 2, 3, 4, 5, ...
  update_B       every captured tensor within 2.9e-7, accuracy and MAE exact to float32
"""
import numpy as np
import pytest

import golden_util as gu
import sweep_invariants as si
from oracle import mps_oracle as mo
from test_timed_paths_gpu import (D, assert_same, compare, device_sweep, fmt, new_ctx, path_of, prepare, relerr,
                                  state_of)

pytestmark = pytest.mark.gpu

N, M, L, B = 10, 5, 3, 33
SEED = 11                                   # test_persistent_sweep_step_by_step


def hp_of(l2, policy='fixed'):
    return (1e-2, 1e-3, l2, 'softmax', 'full_cross_ent', 0.1, policy)


def oracle_kw(hp, **extra):
    return dict(L2_flag=hp[2], act_fn=hp[3], loss_fn=hp[4], T=hp[5], trunc=hp[6], **extra)


_problem = {}


def problem():
    if not _problem:
        X, y, cores32 = prepare(N, M, L, B, SEED)
        _problem.update(X=X, y=y, cores32=cores32, X64=X.astype(np.float64))
    return _problem


def consecutive_sweeps(ctx, hp, n_sweeps, **okw):
    """`n_sweeps` whole sweeps on `ctx`, alternating direction, the device continuing from its own cores.  The oracle
    runs each sweep from the cores the device started it with.  Returns per sweep (observations, counters, result)."""
    pr = problem()
    out = []
    for sw in range(n_sweeps):
        cores_d, bond_d, lp = ctx.get_cores()
        left = lp == N - 1
        assert lp == (0 if sw % 2 == 0 else N - 1)
        st = state_of(cores_d, lp, M, L)
        f_o = mo.forward(st, pr['X64'])
        o = si.oracle_sweep(st, pr['X64'], pr['y'], f_o, hp[0], hp[1], left_dir=left, **oracle_kw(hp, **okw))
        met, f_d, cnt = device_sweep(ctx, left, hp)
        assert list(ctx.get_cores()[1]) == list(st.bond), (sw, list(ctx.get_cores()[1]), list(st.bond))
        out.append((compare(ctx, met, f_d, o, left, B), cnt, (met, f_d, ctx.get_cores()), [len(s) for s in o['S']]))
    return out


_three = {}


def three_sweeps(l2):
    """Modes 1, 2 and 0 from the calibrated start, three consecutive sweeps each; run once per L2 switch."""
    if l2 not in _three:
        pr = problem()
        res = {}
        for mode in (1, 2, 0):
            ctx = new_ctx(N, L, M, pr['X'], pr['y'], pr['cores32'], 0, mode)
            res[mode] = consecutive_sweeps(ctx, hp_of(l2), 3)
            ctx.close()
        _three[l2] = res
    return _three[l2]


# bounds per sweep (first, later) of the tests named in the module docstring
BOUNDS = {
    True: (dict(sigma=5e-6, off=5e-6, env=1e-5, f=1e-5, acc=0.5, mae=1e-6),
           dict(sigma=1e-2, off=1e-4, env=1e-2, f=1e-1, acc=1.0 + 1e-3, mae=2e-5)),
    False: (dict(sigma=1.5e-4, off=5e-6, env=3e-4, f=3e-4, acc=0.5, mae=5e-6),
            dict(sigma=4e-3, off=3e-6, env=2e-4, f=3e-4, acc=0.5, mae=5e-6)),
}


def check(obs, bound, what):
    bad = {k: (v, bound[k]) for k, v in obs.items() if not v <= bound[k]}
    assert not bad, (what, bad)


def test_the_shape_ramps():
    """Consecutive steps of the three sweeps really differ: kept ranks 2, 4, 5 behind, and an odd bond."""
    ranks = [sw[3] for sw in three_sweeps(True)[1]]
    print('kept ranks per sweep', ranks)
    for r in ranks:
        assert r[:3] == [2, 4, 5] and set(r[3:]) == {5}


@pytest.mark.parametrize('l2', [True, False])
def test_three_sweeps_modes_1_and_2_are_bit_equal(l2):
    res = three_sweeps(l2)
    for sw in range(3):
        assert path_of(res[1][sw][1], N) == 'persistent' and path_of(res[2][sw][1], N) == 'persistent'
        assert_same(res[1][sw][2], res[2][sw][2])


@pytest.mark.parametrize('mode', [1, 0])
@pytest.mark.parametrize('l2', [True, False])
def test_three_sweeps_step_by_step_vs_oracle(l2, mode):
    """sigma of every step, behind environments, every step's own metrics row and f, sweep by sweep."""
    res = three_sweeps(l2)[mode]
    print('mode', mode, 'L2' if l2 else 'no L2', [fmt(sw[0]) for sw in res])
    for sw in range(3):
        assert path_of(res[sw][1], N) == ('persistent' if mode else 'per-step')
    for sw in range(3):
        check(res[sw][0], BOUNDS[l2][min(sw, 1)], (mode, l2, sw))


# the per-step paths of narrow_body the persistent kernel does not cover
PER_STEP = dict(sigma=5e-4, f=5e-3, acc=2.0 + 1e-6 * B, mae=2e-3)


def check_per_step(obs, what):
    bad = {k: (obs[k], v) for k, v in PER_STEP.items() if not obs[k] <= v}
    assert not bad, (what, bad)


def test_classic_sequence_vs_oracle():
    """tnml_set_step_pipeline(0): narrow_step_kernel with its reduce and slice helpers, both directions."""
    pr = problem()
    ctx = new_ctx(N, L, M, pr['X'], pr['y'], pr['cores32'], 0, 0)
    ctx.set_step_pipeline(False)
    res = consecutive_sweeps(ctx, hp_of(True), 2)
    ctx.close()
    print('classic', [fmt(sw[0]) for sw in res])
    for sw in range(2):
        assert res[sw][1]['pipelined_steps'] == 0 and res[sw][1]['sweep_steps'] == N - 1
        check_per_step(res[sw][0], ('classic', sw))


def test_adaptive_truncation_vs_oracle():
    """The kept rank and m_out come per step from the device's singular values; both directions."""
    pr = problem()
    thr = 0.97                               # test_hip_parity.py::test_adaptive_truncation_vs_oracle
    ctx = new_ctx(N, L, M, pr['X'], pr['y'], pr['cores32'], 0, 1)
    ctx.set_trunc_threshold(thr)
    res = consecutive_sweeps(ctx, hp_of(True, 'adaptive'), 2, threshold=thr)
    ctx.close()
    print('adaptive', [fmt(sw[0]) for sw in res], 'kept ranks', [sw[3] for sw in res])
    for sw in range(2):
        assert path_of(res[sw][1], N) == 'per-step'
        check_per_step(res[sw][0], ('adaptive', sw))
    # (consecutive_sweeps asserted the device's bonds equal to the oracle's) the rank adapts: below the fixed policy's 2, 4, 5
    assert res[0][3][:3] != [2, 4, 5] and len(set(res[0][3])) > 2


@pytest.mark.parametrize('given', [False, True])
def test_standalone_update_B_with_capture(given):
    """update_B alone at a mid-chain site (stop_after_update, the debug block): B from the two cores, or handed in.  Device and
    oracle step side by side to that site, as test_hip_parity.py::test_stepwise_vs_oracle_and_golden does; the two outer bonds
    of the merged tensor carry a sign each between them (golden_util.gauge_signs)."""
    pr = problem()
    hp = hp_of(True)
    ctx = new_ctx(N, L, M, pr['X'], pr['y'], pr['cores32'], 0, 1)
    ctx.debug_enable(True)
    ctx.forward(want_f=False)
    st = state_of(pr['cores32'], 0, M, L)
    f_o = mo.forward(st, pr['X64'])
    y1h = mo.one_hot(pr['y'], L)
    st.Lenv = {}
    for k in range(2):                       # behind bonds 1, 2: the label then stands at site 2, behind bond 4
        ctx.sweep(False, 1, k == 0, *hp)
        f_o = mo.sweep_step(st, f_o, y1h, hp[0], hp[1], left_dir=False, **oracle_kw(hp))
    cores_d, _, lp = ctx.get_cores()
    assert lp == 2 and st.l_pos == 2
    rec = {}
    mo.sweep_step(st, f_o, y1h, hp[0], hp[1], left_dir=False, record=rec, **oracle_kw(hp))
    shp = rec['B'].shape
    assert shp == (4, D, D, 5, L)
    # the merged tensor of the device's own two cores (its gauge), float32: what update_B forms itself when none is given
    B_own = np.einsum('adkl,kec->adecl', cores_d[2].astype(np.float64), cores_d[3].astype(np.float64)).astype(np.float32)
    sa, tc = gu.gauge_signs(B_own.astype(np.float64), rec['B'])
    Bnew, met = ctx.update_B(B_own if given else None, False, *hp[:6])
    obs = dict(B_new=relerr(Bnew[:rec['B_new'].size].reshape(shp), gu.regauge(rec['B_new'], sa, tc)),
               acc=abs(float(met[0]) - rec['accuracy']), mae=abs(float(met[1]) - rec['MAE']))
    for name in ('B', 'dB_raw', 'L2_grad', 'B_new'):
        obs['dbg_' + name] = relerr(ctx.step_debug(name).reshape(shp), gu.regauge(rec[name], sa, tc))
    assert ctx.l_pos == 2                    # update_B moves nothing
    ctx.close()
    print('update_B', 'given' if given else 'from the cores', fmt(obs))
    assert obs['acc'] < 1e-6 and obs['mae'] < 2e-3
    assert max(obs[k] for k in obs if k not in ('acc', 'mae')) < 5e-3
