"""The core token of the persistent sweep goes out in front of T2 on the steps whose short side is the behind core.

On those steps (every uniform step, and the ramp steps with r <= c) the update workgroup publishes A' = U sqrt(S) and 1 / sigma
for the helper workgroups right after the pass that forms them, and only then runs T2 = Nh . Cb, the first product of the next
norm environment (narrow_body, phase 9, kernels_narrow.hip).  On the other steps (the far end of the chain, where the behind core
comes out of the long-side product) the token keeps its place behind that product.  Nothing of the arithmetic moves, so every
result must stay what it was, bit for bit between the forms of the persistent sweep and to float32 rounding against the per-step
path, which does not publish anything.

Shapes (33 samples: one full sample tile and one sample; three consecutive sweeps right, left, right; L2 term on and off -- with
it off there is no T2 and no norm environment, and the token still has to be raised or the helpers' bounded wait gives up and
the sweep call raises):
  N = 14, bond 10, L = 2    first entry of the shape table
  N = 16, bond 20, L = 2    second entry
  N = 10, bond 5,  L = 3    outside the table (generic body), odd kept bond: 1 / sigma ends in the padded double of the block
Every launch mixes ramp steps (matrix sides 2, 4, 8, 16, 32; those at the far end are the unmoved branch) with uniform steps
(the moved branch).

The persistent-vs-per-step bounds are those of test_hip_parity.py::test_persistent_sweep_matches_per_step_launches_and_oracle,
read from that test's own asserts (they are literals there, not names): its first-sweep bound for the sweep from the calibrated
start, its second-sweep bound for the two sweeps after it, which like its second sweep start both paths from one state (the
persistent context's cores) and run in the regime where these untrained chains amplify float32 rounding.
"""
import inspect
import re

import numpy as np
import pytest

import test_hip_parity
from test_shape_kernels_gpu import uniform_steps
from test_timed_paths_gpu import assert_same, device_sweep, new_ctx, path_of, prepare, relerr

pytestmark = pytest.mark.gpu

B = 33
SEED = 11
CASES = [(14, 10, 2), (16, 20, 2), (10, 5, 3)]
TABLE = ((10, 2), (20, 2))                  # kPersistShapes: (bond, labels)


def parity_bounds():
    """(f first sweep, f later sweeps, MAE per step) between the persistent and the per-step path, from the asserts of the
    parity test; the accuracy bound there is one sample (1 / b + 1e-6), which is a count and not a tolerance."""
    src = inspect.getsource(test_hip_parity.test_persistent_sweep_matches_per_step_launches_and_oracle)
    pats = (r"worst\['f_paths0'\] < ([0-9.e-]+)", r"worst\['f_paths1'\] < ([0-9.e-]+)",
            r"res\[0\]\[0\]\[:, 1\] - res\[1\]\[0\]\[:, 1\]\)\.max\(\) < ([0-9.e-]+)")
    found = [re.search(p, src) for p in pats]
    assert all(found), 'the parity test no longer states its bounds in the form this test reads'
    return tuple(float(m.group(1)) for m in found)


def hp_of(l2):
    # the hyper-parameters of the parity test: lr, weight decay, L2, activation, loss, T, truncation
    return (1e-2, 1e-3, l2, 'softmax', 'full_cross_ent', 0.1, 'fixed')


_problem = {}


def problem(N, M, L):
    key = (N, M, L)
    if key not in _problem:
        _problem[key] = prepare(N, M, L, B, SEED)
    return _problem[key]


def three_sweeps(ctx, N, M, L, hp, starts=None):
    """Three whole sweeps (right, left, right).  starts: per sweep the (cores, label position) to start from (the per-step
    context follows the persistent one); None: free running.  Per sweep: result arrays, the cores it started from, counters,
    fixed-step count, expected uniform-step count."""
    out = []
    for sw in range(3):
        if starts is not None:
            ctx.set_cores(starts[sw][0], int(starts[sw][1]))
        cores_b, bond_b, lp = ctx.get_cores()
        assert lp == (0 if sw % 2 == 0 else N - 1)
        left = lp == N - 1
        met, f_d, cnt = device_sweep(ctx, left, hp)          # raises if a bounded wait gave up (status word != 0)
        after = ctx.get_cores()
        out.append(dict(arrays=(met, f_d, after), start=(cores_b, lp), cnt=cnt, fixed=ctx.fixed_shape_steps(),
                        uniform=uniform_steps(bond_b, after[1], left, M, L)))
    return out


_runs = {}


def runs(N, M, L, l2):
    """One context per form, each from the same calibrated start, run once per case and L2 switch:
       on / off      mode 1 with the shape switch on / off
       mode2         one kernel per role
       again         mode 1 once more on a fresh context, created after the first one is closed
       reset         the first context after its three sweeps and set_cores back to the start: one more sweep
       perstep       one launch per step, started before every sweep from the cores the 'on' context started it from"""
    key = (N, M, L, l2)
    if key in _runs:
        return _runs[key]
    X, y, cores32 = problem(N, M, L)
    hp = hp_of(l2)
    res = {}
    for name, mode, on in (('on', 1, True), ('off', 1, False), ('mode2', 2, True), ('again', 1, True)):
        ctx = new_ctx(N, L, M, X, y, cores32, 0, mode)
        ctx.set_shape_kernels(on)
        res[name] = three_sweeps(ctx, N, M, L, hp)
        if name == 'on':
            ctx.set_cores(cores32, 0)
            met, f_d, cnt = device_sweep(ctx, False, hp)
            res['reset'] = dict(arrays=(met, f_d, ctx.get_cores()), cnt=cnt)
        ctx.close()
    ctx = new_ctx(N, L, M, X, y, cores32, 0, 0)
    res['perstep'] = three_sweeps(ctx, N, M, L, hp, starts=[sw['start'] for sw in res['on']])
    ctx.close()
    _runs[key] = res
    return res


@pytest.mark.parametrize('l2', [True, False])
@pytest.mark.parametrize('N,M,L', CASES)
def test_forms_of_the_persistent_sweep_agree_bit_for_bit(N, M, L, l2):
    """Mode 1 == mode 2, shape switch on == off, and the same three sweeps once more on a fresh context: identical arrays."""
    res = runs(N, M, L, l2)
    for sw in range(3):
        for name in ('on', 'off', 'mode2', 'again'):
            assert path_of(res[name][sw]['cnt'], N) == 'persistent', (name, sw)
        assert_same(res['on'][sw]['arrays'], res['mode2'][sw]['arrays'])
        assert_same(res['on'][sw]['arrays'], res['off'][sw]['arrays'])
        assert_same(res['on'][sw]['arrays'], res['again'][sw]['arrays'])


@pytest.mark.parametrize('l2', [True, False])
@pytest.mark.parametrize('N,M,L', CASES)
def test_both_token_places_run_in_every_launch(N, M, L, l2):
    """Every launch mixes uniform steps (token in front of T2) with bond ramps, the far end's among them (token behind the
    long-side product); the compiled bodies run exactly on the uniform steps of a table shape."""
    res = runs(N, M, L, l2)
    for sw in range(3):
        uniform = res['on'][sw]['uniform']
        assert 0 < uniform < N - 1
        assert res['on'][sw]['fixed'] == (uniform if (M, L) in TABLE else 0)
        assert res['off'][sw]['fixed'] == 0 and res['mode2'][sw]['fixed'] == 0


@pytest.mark.parametrize('l2', [True, False])
@pytest.mark.parametrize('N,M,L', CASES)
def test_persistent_sweep_matches_the_per_step_path(N, M, L, l2):
    f_first, f_later, mae = parity_bounds()
    res = runs(N, M, L, l2)
    seen = []
    for sw in range(3):
        assert path_of(res['perstep'][sw]['cnt'], N) == 'per-step'
        (m1, f1, (c1, b1, lp1)), (m0, f0, (c0, b0, lp0)) = res['on'][sw]['arrays'], res['perstep'][sw]['arrays']
        assert list(b1) == list(b0) and lp1 == lp0
        seen.append((float(relerr(f1, f0)), float(np.abs(m1[:, 0] - m0[:, 0]).max() * B), float(np.abs(m1[:, 1] - m0[:, 1]).max())))
    print('token order', N, M, L, 'L2' if l2 else 'no L2', 'f / accuracy in samples / MAE per sweep', ['%.2e %.2f %.2e' % s for s in seen])
    for sw, (df, dacc, dmae) in enumerate(seen):
        assert df < (f_first if sw == 0 else f_later), (sw, df)
        assert dacc <= 1.0 + 1e-6 * B, (sw, dacc)               # one sample
        assert dmae < mae, (sw, dmae)


@pytest.mark.parametrize('l2', [True, False])
@pytest.mark.parametrize('N,M,L', CASES)
def test_sweep_after_set_cores_on_a_used_context(N, M, L, l2):
    """Three sweeps, then set_cores back to the start: the next sweep is the first one again (tokens, published block and
    records carry nothing over)."""
    res = runs(N, M, L, l2)
    assert path_of(res['reset']['cnt'], N) == 'persistent'
    assert_same(res['reset']['arrays'], res['on'][0]['arrays'])


def test_two_shapes_in_one_process_follow_their_tables():
    """A bond-10 and a bond-20 context alive together, their sweeps interleaved: two instantiations of the kernel in one process,
    each step with the constants of its own shape; the arrays are those of the contexts that ran alone."""
    hp = hp_of(True)
    shapes = CASES[:2]
    ctxs = []
    for N, M, L in shapes:
        X, y, cores32 = problem(N, M, L)
        ctx = new_ctx(N, L, M, X, y, cores32, 0, 1)
        ctx.set_shape_kernels(True)
        ctxs.append(ctx)
    for sw in range(3):
        for (N, M, L), ctx in zip(shapes, ctxs):
            bond_b, lp = ctx.get_cores()[1:]
            left = lp == N - 1
            met, f_d, cnt = device_sweep(ctx, left, hp)
            after = ctx.get_cores()
            want = runs(N, M, L, True)['on'][sw]
            assert path_of(cnt, N) == 'persistent'
            assert ctx.fixed_shape_steps() == uniform_steps(bond_b, after[1], left, M, L) == want['fixed'] > 0
            assert_same((met, f_d, after), want['arrays'])
    for ctx in ctxs:
        ctx.close()
