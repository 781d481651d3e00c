"""The conditions on the float64 oracle that make tests/test_update_rule_gpu.py mean something (no GPU).

For every case of update_rule_reference.CASES, over its two sweeps: every value finite; no step within 5 % of the clip switch; every
mutant of the update rule moves the increment of every step where it is a different rule by at least FLOOR; the cases meant to run
the unclipped branch do so in at least three steps, with at least three clipped beside them.  FLOOR is at least 20 times the GPU
test's increment bound, and the persistent cases' sigma bound is a twentieth of what dropping the decay term does to sigma.

One test records why the cases exist: at the suite's older setting (weight_dec = 1e-3, L2_flag off) dropping the decay term moves
B_new by less than the 5e-3 the step-wise tests allow.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sweep_invariants as si
import update_rule_reference as ur
from oracle import mps_oracle as mo

IDS = [c['id'] for c in ur.CASES]


def test_rule_is_the_oracles_update():
    rng = np.random.default_rng(0)
    B, raw, G = (rng.standard_normal((2, 3, 3, 4, 2)) for _ in range(3))
    for scale, clipped in ((10.0, True), (0.01, False)):
        sumB, sumD, fac, Bn = ur.rule(B, scale * raw, scale * G, 0.01)
        dB = scale * raw - scale * G
        assert sumB == np.abs(B).sum() and sumD == np.abs(dB).sum() and (sumD > sumB) == clipped
        assert fac == (sumB / sumD if clipped else 1.0)
        assert np.array_equal(Bn, B + 0.01 * (dB / (sumD / sumB) if clipped else dB))


@pytest.mark.parametrize('c', ur.CASES, ids=IDS)
def test_case_shows_every_term(c):
    X, y, c32, recs = ur.record(c)
    assert len(recs) == 2 * (c['N'] - 1)
    for r in recs:
        for key in ('B', 'dB_raw', 'L2_grad', 'B_new', 'f_new', 'S'):
            assert np.isfinite(r[key]).all(), (key, r['sweep'], r['step'])
    ms = ur.mutants(recs, c['lr'], c['wd'], c['L2_flag'])          # (asserts that rule() reproduces every recorded B_new)
    for m, r in zip(ms, recs):
        assert abs(m['ratio'] - 1.0) >= ur.CLIP_MARGIN, (r['sweep'], r['step'], m['ratio'])
    n_clip = sum(m['clipped'] for m in ms)
    se = ur.smallest_effects(ms)
    print(c['id'], 'clipped %d of %d' % (n_clip, len(ms)), {k: '%.1e in %d' % v for k, v in se.items()})
    want = set(ur.MUTANTS_ANY) | (set(ur.MUTANTS_L2) if c['L2_flag'] else set())
    if n_clip == len(ms):
        want.discard('fac_always')
    assert set(se) == want, (sorted(se), sorted(want))
    for k, (v, n) in se.items():
        assert v >= ur.FLOOR, (k, v)
    if c['tag'] == 'unclipped':
        assert n_clip >= 3 and len(ms) - n_clip >= 3, n_clip
        assert se['fac_always'][1] >= 3 and se['fac_one'][1] >= 3
    elif c['wd'] >= 1.0:
        assert n_clip == len(ms)                                    # every step is clipped at weight_dec = 1
    # the f product of anyd_batch_kernel: a case tagged for a branch has the shape that takes it
    if c['tag'] == 'L20':
        assert c['L'] > 16
    if c['tag'] == 'chunks':
        cols = max(c['D'] * r['B'].shape[0 if r['left_dir'] else 3] * c['L'] for r in recs)
        assert cols > 128 and 128 % c['L'] != 0, cols
    if c['tag'] == 'ragged':
        assert c['b'] > 64 and c['b'] % 64 not in (0, 1)
    if c['tag'] == 'odd':
        assert any(b % 2 for r in recs for b in r['bond'])
    if c['kernel'] == 'anyd':
        assert c['N'] <= 10
        for r in recs:
            a, D, _, cc, L = r['B'].shape
            assert (min(D * a * L, D * cc) if r['left_dir'] else min(D * a, D * cc * L)) <= 64      # the short side
    else:
        assert c['N'] <= 16


def test_table_covers_the_issue():
    by = lambda **kw: [c for c in ur.CASES if all(c[k] == v for k, v in kw.items())]
    for kernel in ('lds', 'large', 'anyd'):
        for act, loss in ur.PAIRS3:
            for l2 in (True, False):
                assert by(kernel=kernel, act=act, loss=loss, L2_flag=l2, wd=1.0, tag='decay'), (kernel, act, loss, l2)     # i
        assert by(kernel=kernel, tag='unclipped')                                                                     # ii
    assert {c['D'] for c in by(kernel='anyd')} >= {3, 5, 8}                                                           # iii
    for act, loss in ur.PAIRS9:                                                                                       # iv
        assert [c for c in by(kernel='anyd', D=3, M=6, N=8, L=3, b=100, act=act, loss=loss, L2_flag=True)], (act, loss)
    for tag in ('L20', 'chunks', 'ragged', 'odd'):                                                                    # v - viii
        assert by(kernel='anyd', tag=tag), tag


def test_floor_is_twenty_increment_bounds():
    for kernel, bound in ur.INC_BOUND.items():
        assert 20 * bound <= ur.FLOOR, (kernel, bound)
    for kernel, sb in ur.STANDALONE_BOUNDS.items():
        assert 20 * sb['inc'] <= ur.FLOOR, (kernel, sb)


def test_old_setting_does_not_see_the_decay_term():
    """weight_dec = 1e-3, L2_flag off, the D = 3 shape of (i): B_new without the term differs from B_new by less than 5e-3 of max|B_new|
    (the bound of the step-wise tests), in every step of the three pairs -- and by more than it at weight_dec = 1."""
    worst = {1e-3: 0.0, 1.0: 0.0}
    for c in [c for c in ur.CASES if c['kernel'] == 'anyd' and c['tag'] == 'decay' and not c['L2_flag']]:
        X, y, c32 = ur.inputs(c)
        for wd in worst:
            for _, _, r in ur.oracle_steps(X, y, c32, c, wd=wd):
                _, _, _, Bn_drop = ur.rule(r['B'], r['dB_raw'], 0.0 * r['L2_grad'], c['lr'])
                worst[wd] = max(worst[wd], np.abs(Bn_drop - r['B_new']).max() / np.abs(r['B_new']).max())
    print({k: '%.1e' % v for k, v in worst.items()})
    assert worst[1e-3] < 5e-3
    assert worst[1.0] > 5e-3


@pytest.mark.parametrize('l2', [True, False])
@pytest.mark.parametrize('act,loss', ur.PAIRS3)
def test_persistent_cases_see_the_decay_term(act, loss, l2):
    """Sweep 1 of the persistent cases with the decay term dropped (weight_dec = 0) against the true oracle: the kept singular values
    differ, relative to each step's sigma_max, by at least 20 times the bound the GPU test puts on them."""
    import test_timed_paths_gpu as tp
    P = ur.PERSIST
    X, y, c32 = tp.prepare(P['N'], P['M'], P['L'], P['b'], P['seed'])
    X64 = X.astype(np.float64)
    S = []
    for wd in (P['wd'], 0.0):
        st = tp.state_of(c32, 0, P['M'], P['L'])
        o = si.oracle_sweep(st, X64, y, mo.forward(st, X64), P['lr'], wd, left_dir=False, L2_flag=l2, act_fn=act, loss_fn=loss,
                            T=ur.T, trunc='fixed')
        assert np.isfinite(o['f']).all()
        S.append(o['S'])
    diff = float(si.sigma_errors(S[1], S[0]).max())
    print(act, loss, l2, 'sigma moves by %.2e' % diff)
    assert diff >= 20 * ur.PERSIST_BOUNDS['sigma'], diff
