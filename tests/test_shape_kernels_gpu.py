"""The persistent sweep kernel compiled for a step shape (kernels_narrow.hip: PersistArgs<FixedShape>, HelperArgs<FixedShape>;
the table kPersistShapes of wide_pipe_device.h holds bond 10 and bond 20 at two labels).

A marked step runs a body whose dimensions are compile-time constants; it has to compute what the generic body computes, bit
for bit, and the marks have to sit on the uniform steps and nowhere else.  So the chains are short: N = 14 at bond 10 and
N = 16 at bond 20, two labels, 33 samples (one full sample tile and one sample).  With D = 2 the bond ramps 2, 4, 8, (16,) M at
both ends, so every launch mixes generic and fixed steps and only a handful of mid-chain steps have the uniform shape.  Three
CONSECUTIVE sweeps (right, left, right) from the calibrated start, L2 term on and off.

The criterion is equality of every array with the generic path (switch off) and with mode 2 (one kernel per role, generic
bodies only), which the existing tests pin to the oracle; the comparison with the oracle is printed for the record.
"""
import numpy as np
import pytest

import sweep_invariants as si
from oracle import mps_oracle as mo
from test_timed_paths_gpu import (D, assert_same, compare, device_sweep, fmt, new_ctx, path_of, prepare, state_of)

pytestmark = pytest.mark.gpu

L, B = 2, 33
SEED = 11
CASES = [(14, 10), (16, 20)]                # (N, bond): the two shapes of the table


def hp_of(l2):
    return (1e-2, 1e-3, l2, 'softmax', 'full_cross_ent', 0.1, 'fixed')


_problem = {}


def problem(N, M, L_=L):
    key = (N, M, L_)
    if key not in _problem:
        X, y, cores32 = prepare(N, M, L_, B, SEED)
        _problem[key] = dict(X=X, y=y, cores32=cores32, X64=X.astype(np.float64))
    return _problem[key]


def uniform_steps(bond_before, bond_after, left, M, L_):
    """Steps of a sweep whose behind, shared, ahead and kept bond all equal M and whose pre-gradient has D * M rows (the
    behind bond of the step before was M too), from the chain's bond lists before and after the sweep."""
    bb = list(bond_before)[::-1] if left else list(bond_before)
    nb = list(bond_after)[::-1] if left else list(bond_after)
    n_steps = len(bb)
    h = [1 if k == 0 else nb[k - 1] for k in range(n_steps)]          # behind bond of step k = kept bond of step k - 1
    count = 0
    for k in range(n_steps):
        s, g, m = bb[k], (bb[k + 1] if k + 1 < n_steps else 1), nb[k]
        z_rows = 1 if k == 0 else D * h[k - 1]
        count += (h[k], g, s, m, z_rows) == (M, M, M, M, D * M)
    return count


def three_sweeps_on(ctx, N, M, hp, with_oracle):
    """Three consecutive whole sweeps; per sweep (result arrays, counters, fixed-step count, expected count, oracle comparison)."""
    pr = problem(N, M)
    out = []
    for sw in range(3):
        cores_d, bond_d, lp = ctx.get_cores()
        left = lp == N - 1
        assert lp == (0 if sw % 2 == 0 else N - 1)
        obs = None
        if with_oracle:
            st = state_of(cores_d, lp, M, L)
            f_o = mo.forward(st, pr['X64'])
            o = si.oracle_sweep(st, pr['X64'], pr['y'], f_o, hp[0], hp[1], left_dir=left, L2_flag=hp[2], act_fn=hp[3],
                                loss_fn=hp[4], T=hp[5], trunc=hp[6])
        met, f_d, cnt = device_sweep(ctx, left, hp)
        after = ctx.get_cores()
        if with_oracle:
            obs = compare(ctx, met, f_d, o, left, B)
        out.append(((met, f_d, after), cnt, ctx.fixed_shape_steps(), uniform_steps(bond_d, after[1], left, M, L), obs))
    return out


_runs = {}


def runs(N, M, l2):
    """mode 1 with the switch on, mode 1 with it off, mode 2; run once per case and L2 switch."""
    key = (N, M, l2)
    if key not in _runs:
        pr = problem(N, M)
        res = {}
        for name, mode, on in (('on', 1, True), ('off', 1, False), ('mode2', 2, True)):
            ctx = new_ctx(N, L, M, pr['X'], pr['y'], pr['cores32'], 0, mode)
            ctx.set_shape_kernels(on)
            res[name] = three_sweeps_on(ctx, N, M, hp_of(l2), name == 'on')
            ctx.close()
        _runs[key] = res
    return _runs[key]


@pytest.mark.parametrize('l2', [True, False])
@pytest.mark.parametrize('N,M', CASES)
def test_fixed_bodies_equal_generic_bodies_and_mode_2(N, M, l2):
    res = runs(N, M, l2)
    print('N', N, 'bond', M, 'L2' if l2 else 'no L2', 'fixed steps per sweep', [sw[2] for sw in res['on']],
          'vs oracle', [fmt(sw[4]) for sw in res['on']])
    for sw in range(3):
        for name in ('on', 'off', 'mode2'):
            assert path_of(res[name][sw][1], N) == 'persistent', (name, sw)
        assert_same(res['on'][sw][0], res['off'][sw][0])
        assert_same(res['on'][sw][0], res['mode2'][sw][0])


@pytest.mark.parametrize('l2', [True, False])
@pytest.mark.parametrize('N,M', CASES)
def test_marked_steps_are_the_uniform_ones(N, M, l2):
    res = runs(N, M, l2)
    print('N', N, 'bond', M, 'fixed / expected per sweep', [(sw[2], sw[3]) for sw in res['on']])
    for sw in range(3):
        got, want = res['on'][sw][2], res['on'][sw][3]
        assert 0 < want < N - 1                          # every launch mixes generic and fixed steps
        assert got == want, (sw, got, want)
        assert res['off'][sw][2] == 0 and res['mode2'][sw][2] == 0


def test_a_shape_outside_the_table_runs_the_generic_kernel():
    """N = 10, bond 5, three labels (the chain of test_update_record_gpu.py): no mark, still one launch per sweep."""
    N, M, L3 = 10, 5, 3
    pr = problem(N, M, L3)
    ctx = new_ctx(N, L3, M, pr['X'], pr['y'], pr['cores32'], 0, 1)
    for sw in range(2):
        left = ctx.get_cores()[2] == N - 1
        _, _, cnt = device_sweep(ctx, left, hp_of(True))
        assert path_of(cnt, N) == 'persistent'
        assert ctx.fixed_shape_steps() == 0
    ctx.close()
