"""The helpers of the persistent sweep wait once: the L2 term's last factor is applied by the update workgroup.

Part 2 of a helper workgroup (persist_helper_block, kernels_narrow.hip) stores P2 = diag(1 / sigma) A'^T (T . Ng) in the slot of
prepG and arrives; the update workgroup forms Ln.B.Rn = Nh^T . P2 from the Nh it kept in LDS one step earlier.  The sums are the
helper's former third product, element for element, so nothing may move: modes 1 (one kernel) and 2 (one kernel per role) stay
equal bit for bit, and both stay within the bounds of test_hip_parity.py::test_persistent_sweep_matches_per_step_launches_and_
oracle against the per-step path (which forms the L2 term from the cores) and the float64 oracle.

Shapes (33 samples: one full sample tile and one sample; two sweeps, one per direction):
  N = 16, bond 20, L = 2    the fixed body of the table's second entry, bond ramps at both ends, the k == 0 identity step
  N = 14, bond 10, L = 2    the other table entry
  N = 10, bond 5,  L = 3    generic body, odd bond (1 / sigma ends in a padded double in the published block), three labels.  Its
                            steps with ahead bond 1 have RW = D D g L = 12 columns for 8 helpers: slices of 2, helpers 6 and 7 have
                            no column and still have to pass the single wait and arrive.
A wait that gave up sets the launch's status word, which the sweep call reads back and raises on: a sweep that returns is a sweep
whose status word was 0.
"""
import numpy as np
import pytest

import sweep_invariants as si
from oracle import mps_oracle as mo
from test_shape_kernels_gpu import uniform_steps
from test_timed_paths_gpu import D, assert_same, device_sweep, new_ctx, path_of, prepare, relerr, state_of

pytestmark = pytest.mark.gpu

B = 33
SEED = 11
N_HELPERS = 8                               # kPersistHelpers (wide_pipe_device.h)
CASES = [(16, 20, 2), (14, 10, 2), (10, 5, 3)]
TABLE = ((10, 2), (20, 2))                  # kPersistShapes: (bond, labels)


def hp_of(l2):
    # test_persistent_sweep_matches_per_step_launches_and_oracle: lr, weight decay, L2, activation, loss, T, truncation
    return (1e-2, 1e-3, l2, 'softmax', 'full_cross_ent', 0.1, 'fixed')


_runs = {}


def runs(N, M, L, l2, modes):
    """Sweep 1 (right, calibrated start) and sweep 2 (left, every context and the oracle from the first context's cores) on one
    context per mode; run once per key.  Per sweep: results per mode, fixed / expected step counts of the first context, the
    oracle's record."""
    key = (N, M, L, l2, modes)
    if key in _runs:
        return _runs[key]
    X, y, cores32 = prepare(N, M, L, B, SEED)
    X64 = X.astype(np.float64)
    hp = hp_of(l2)
    ctxs = [new_ctx(N, L, M, X, y, cores32, 0, mode) for mode in modes]
    st = state_of(cores32, 0, M, L)
    out = []
    for sw in range(2):
        left = sw == 1
        if sw == 1:
            cores_d, _, lp = ctxs[0].get_cores()
            st = state_of(cores_d, lp, M, L)
            for ctx in ctxs[1:]:
                ctx.set_cores(cores_d, int(lp))
        bond_before = list(ctxs[0].get_cores()[1])
        f_o = mo.forward(st, X64)
        o = si.oracle_sweep(st, X64, y, f_o, hp[0], hp[1], left_dir=left, L2_flag=l2, act_fn=hp[3], loss_fn=hp[4], T=hp[5], trunc=hp[6])
        res = {}
        fixed = None
        for mode, ctx in zip(modes, ctxs):
            met, f_d, cnt = device_sweep(ctx, left, hp)          # raises if a wait gave up (status word != 0)
            ctx.synchronize()
            after = ctx.get_cores()
            assert path_of(cnt, N) == ('per-step' if mode == 0 else 'persistent'), (mode, sw)
            if fixed is None:
                fixed = (ctx.fixed_shape_steps(), uniform_steps(bond_before, after[1], left, M, L))
            diag, _ = si.step_sigmas(after[0], after[1], left)
            res[mode] = dict(arrays=(met, f_d, after), sigma=float(si.sigma_errors(diag, o['S']).max()))
        out.append(dict(res=res, fixed=fixed, o=o, bond_before=bond_before))
    for ctx in ctxs:
        ctx.close()
    _runs[key] = out
    return out


@pytest.mark.parametrize('N,M,L', CASES)
def test_modes_1_and_2_agree_bit_for_bit_with_l2(N, M, L):
    for sw in runs(N, M, L, True, (1, 0, 2)):
        assert_same(sw['res'][1]['arrays'], sw['res'][2]['arrays'])      # metrics, f, cores, bonds, label position


@pytest.mark.parametrize('N,M,L', CASES)
def test_single_wait_sweep_matches_per_step_path_and_oracle(N, M, L):
    """The bounds of test_persistent_sweep_matches_per_step_launches_and_oracle, unchanged."""
    out = runs(N, M, L, True, (1, 0, 2))
    worst = {}
    for i, sw in enumerate(out):
        o = sw['o']
        for mode in (1, 0, 2):
            met, f_d, (cores_d, bond_d, lp) = sw['res'][mode]['arrays']
            assert [len(s) for s in o['S']] == [int(bond_d[si.behind_site(N, k, i == 1)[0]]) for k in range(N - 1)]
            assert lp == (0 if i == 1 else N - 1)
            worst['f_vs_oracle%d' % i] = max(worst.get('f_vs_oracle%d' % i, 0), relerr(f_d, o['f']))
            worst['acc'] = max(worst.get('acc', 0), np.abs(met[:, 0] - np.array(o['accuracy'])).max() * B)
            worst['mae'] = max(worst.get('mae', 0), np.abs(met[:, 1] - np.array(o['MAE'])).max())
            worst['sigma%d' % i] = max(worst.get('sigma%d' % i, 0), sw['res'][mode]['sigma'])
        (m1, f1, _), (m0, f0, _) = sw['res'][1]['arrays'], sw['res'][0]['arrays']
        worst['f_paths%d' % i] = relerr(f1, f0)
        assert np.abs(m1[:, 0] - m0[:, 0]).max() <= 1.0 / B + 1e-6
        assert np.abs(m1[:, 1] - m0[:, 1]).max() < 2e-4
    print('single wait', N, M, L, {k: '%.2e' % v for k, v in worst.items()})
    assert worst['f_vs_oracle0'] < 1e-5 and worst['f_paths0'] < 1e-5
    assert worst['f_vs_oracle1'] < 4.5e-2 and worst['f_paths1'] < 1.4e-2
    assert worst['sigma0'] < 5e-6 and worst['sigma1'] < 1e-2
    assert worst['acc'] <= 1.0 + 1e-3       # samples
    assert worst['mae'] < 3e-5


def test_fixed_steps_are_marked_with_l2():
    """The two table shapes run their compiled bodies through the new front (the marks sit where test_marked_steps_are_the_uniform_
    ones expects them), the third shape runs the generic one."""
    for N, M, L in CASES:
        for sw in runs(N, M, L, True, (1, 0, 2)):
            got, uniform = sw['fixed']
            assert 0 < uniform < N - 1                           # every launch mixes uniform steps and bond ramps
            want = uniform if (M, L) in TABLE else 0             # a uniform step outside the table has no compiled body
            assert got == want, (N, M, got, want)


def test_without_l2_modes_agree_and_marks_stay():
    """The path without the L2 term (no P2, nothing added on the update workgroup) at the bond-20 shape."""
    N, M, L = CASES[0]
    for sw in runs(N, M, L, False, (1, 2)):
        assert_same(sw['res'][1]['arrays'], sw['res'][2]['arrays'])
        got, want = sw['fixed']
        assert 0 < want < N - 1 and got == want, (got, want)


def test_helpers_without_columns_pass_the_single_wait():
    """N = 10, bond 5, L = 3: a step with ahead bond 1 has fewer column slices than helpers.  Both sweeps of both persistent modes
    returned (status word 0) and left finite, agreeing results."""
    N, M, L = CASES[2]
    out = runs(N, M, L, True, (1, 0, 2))
    idle = 0
    for sw in out:
        for g in set(sw['bond_before']) | {1}:           # ahead bonds met in the sweep; 1 at its last step
            RW = D * D * g * L
            cw = (RW + N_HELPERS - 1) // N_HELPERS
            idle += (N_HELPERS - 1) * cw >= RW           # the last helper's slice starts at or past the end
        for mode in (1, 2):
            met, f_d, (cores_d, _, _) = sw['res'][mode]['arrays']
            assert np.isfinite(f_d).all() and np.isfinite(met).all() and all(np.isfinite(c).all() for c in cores_d)
    assert idle > 0
