"""The hand-over between the update workgroup and the helper workgroups of the persistent sweep (kernels_narrow.hip:
narrow_body phases 9-11, persist_helper_block part 2), at the smallest shapes where its transport can go wrong.

The update workgroup publishes A' = U sqrt(S) and 1 / sigma under one token right after its cores and the behind norm
environment Nh under the end-of-step token; the helpers start their first product level on the first token and wait for the
second only in front of the L2 product.  The published block and the helpers' three result slices travel as 16-byte
agent-scope stores and loads with explicit heads and tails.  What the cases pin down (RW = D D g L columns over 8 helpers,
cw = ceil(RW / 8) columns each):

  ('fixed', 6, 12, 40, 3)      mid-chain RW = 72, cw = 9: no slice width is a multiple of 4 floats or 2 doubles, and the row
                               starts i RW + 9 hid fall on every offset of the 16-byte grid
  ('fixed', 5, 10, 33, 3)      odd bond: RW = 60, cw = 8 with a last slice of 4; odd h, odd h h: 1 / sigma and Nh end in a
                               padded double
  l2 = False                   the second token is never waited for: the sweep has to finish with status OK
  ('reference', 2, 14, 9, 2)   RW = 8 / 16: one or two columns per helper
  every case                   first and last steps have h = 1 or zr = 1 (a one-double block); with three labels the chain ends
                               have RW = 12, cw = 2: helpers 6 and 7 have no column at all (nc = 0)

Every case runs two sweeps (right, then left from one common state: both directions, inherited norm environments) in modes 1
(one kernel), 2 (one kernel per role) and 0 (one launch per step).  Modes 1 and 2 must agree bit for bit.  Modes 1 and 0 are
each held to the float64 oracle step by step (every step's singular values through the Gram matrix of the core it left, the
behind environments, the per-step metrics, f) with the constants of test_persistent_sweep_step_by_step, and to each other with
the same constants.
"""
import numpy as np
import pytest

import sweep_invariants as si
from oracle import mps_oracle as mo
from test_timed_paths_gpu import (assert_same, compare, device_sweep, fmt, new_ctx, path_of, prepare, relerr, state_of)

pytestmark = pytest.mark.gpu

CASES = [
    ('fixed', 6, 12, 40, 3, True),
    ('fixed', 5, 10, 33, 3, True),
    ('fixed', 6, 12, 40, 3, False),
    ('fixed', 5, 10, 33, 3, False),
    ('reference', 2, 14, 9, 2, True),
]


def slice_widths(g, L, nH=8):
    RW = 2 * 2 * g * L
    cw = (RW + nH - 1) // nH
    return RW, cw, [max(0, min(RW, (i + 1) * cw) - min(RW, i * cw)) for i in range(nH)]


def test_the_cases_reach_the_shapes_they_are_meant_to():
    RW, cw, nc = slice_widths(6, 3)
    assert (RW, cw) == (72, 9) and {(i * RW + hid * cw) % 4 for i in range(6) for hid in range(8)} == {0, 1, 2, 3}
    RW, cw, nc = slice_widths(5, 3)
    assert (RW, cw, nc[-1]) == (60, 8, 4)
    RW, cw, nc = slice_widths(1, 3)          # the chain ends with three labels
    assert (RW, cw) == (12, 2) and nc[6:] == [0, 0]


@pytest.mark.parametrize('policy,M,N,b,L,l2', CASES)
def test_handoff_step_by_step(policy, M, N, b, L, l2):
    hp = (1e-2, 1e-3, l2, 'softmax', 'full_cross_ent', 0.1, policy)
    X, y, cores32 = prepare(N, M, L, b, 11)
    X64 = X.astype(np.float64)
    modes = (1, 2, 0)
    ctxs = [new_ctx(N, L, M, X, y, cores32, 0, mode) for mode in modes]
    okw = dict(L2_flag=l2, act_fn=hp[3], loss_fn=hp[4], T=hp[5], trunc=policy)
    st = state_of(cores32, 0, M, L)
    obs, paths, res = [], [], []
    for sw in range(2):
        left = sw == 1
        if sw == 1:
            cores_d, _, lp = ctxs[0].get_cores()
            st = state_of(cores_d, lp, M, L)
            for ctx in ctxs[1:]:
                ctx.set_cores(cores_d, lp)
        f_o = mo.forward(st, X64)
        o = si.oracle_sweep(st, X64, y, f_o, hp[0], hp[1], left_dir=left, **okw)
        out, ob, pa = [], [], []
        for ctx in ctxs:
            met, f_d, cnt = device_sweep(ctx, left, hp)     # (a sweep that gave up raises: status OK is part of every call)
            out.append((met, f_d, ctx.get_cores()))
            ob.append(compare(ctx, met, f_d, o, left, b))
            pa.append(path_of(cnt, N))
        res.append(out); obs.append(ob); paths.append(pa)
    for ctx in ctxs:
        ctx.close()
    for sw in range(2):
        assert paths[sw] == ['persistent', 'persistent', 'per-step']
        assert_same(res[sw][0], res[sw][1])                 # one kernel or three: the same bits
    # modes 1 and 0 against each other: per-step metrics and f
    between = []
    for sw in range(2):
        (m1, f1, _), (m0, f0, _) = res[sw][0], res[sw][2]
        between.append(dict(f=float(relerr(f1, f0)), acc=float(np.abs(m1[:, 0] - m0[:, 0]).max() * b),
                            mae=float(np.abs(m1[:, 1] - m0[:, 1]).max())))
    print('hand-off', policy, M, N, b, L, 'L2' if l2 else 'no L2')
    for sw in range(2):
        print('  sweep %d: mode 1 vs oracle' % (sw + 1), fmt(obs[sw][0]), '| mode 0 vs oracle', fmt(obs[sw][2]),
              '| mode 1 vs mode 0', fmt(between[sw]))
    # the constants of test_persistent_sweep_step_by_step
    for i in (0, 2):
        o1, o2 = obs[0][i], obs[1][i]
        assert o1['sigma'] < 5e-6 and o1['off'] < 5e-6 and o1['env'] < 1e-5
        assert o1['f'] < 1e-5 and o1['acc'] < 0.5 and o1['mae'] < 1e-6
        assert o2['sigma'] < 1e-2 and o2['off'] < 1e-4 and o2['env'] < 1e-2
        assert o2['f'] < 1e-1 and o2['acc'] <= 1.0 + 1e-3 and o2['mae'] < 2e-5
    b1, b2 = between
    assert b1['f'] < 1e-5 and b1['acc'] < 0.5 and b1['mae'] < 1e-6
    assert b2['f'] < 1e-1 and b2['acc'] <= 1.0 + 1e-3 and b2['mae'] < 2e-5
