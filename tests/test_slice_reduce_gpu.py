"""The slice reduction of the persistent sweep (tnml_set_persist_reduce, wide_pipe_device.h) against the last-arriver form.

Where sixteen partial pre-gradients do not fit one workgroup's LDS (bond 20 at two labels: 6400 floats each), the batch-side
workgroups of a persistent sweep count their arrivals and the first R of them each sum runs of 16-byte elements over all partials,
instead of the last arriver of each group of sixteen and then the last group.  The summation tree is the same, so every number the
sweep leaves must be the same, bit for bit.  Batch sizes sit on the edges of the groups (workgroups = 32-sample tiles of the batch
padded to 64):

  33     2 workgroups: fewer workgroups than runs, the reducers loop
  512    16 workgroups: exactly one full group
  513    18 workgroups: a second group begins
  1000   32 workgroups
  5000   158 workgroups: ten groups, the last one short, fewer reducers (101) than workgroups

N = 16 at bond 20 has ramp steps with one-level pre-gradients at both ends and the 6400-float pre-gradient in between; N = 10 at
bond 5 and three labels has no compiled shape (the generic bodies) and 1200-float pre-gradients beyond one level in its middle.
"""
import numpy as np
import pytest

from test_timed_paths_gpu import assert_same, device_sweep, new_ctx, path_of, prepare

pytestmark = pytest.mark.gpu

D, TS = 2, 32


def upm(x, m):
    return (x + m - 1) // m * m


def batch_lds_floats(L, hj, gj, gn, hprev, first, do_ext, do_f, do_z):
    """LDS floats of one batch-side workgroup: wide_pipe_dims and wide_pipe_carve of wide_pipe_device.h."""
    P = TS + 1
    nI = 1 if first else hj * D
    IP, JP, KA, EH = upm(nI, 16), upm(D * gj, 4), upm(hprev * D, 4), upm(hj, 16)
    RS, HS, I3, J3 = (JP * L) | 1, EH + 1, upm(nI * D, 16), upm(D * gn, 16)
    q = 4 * TS * D + 2 * L * TS
    q += (KA * P + KA * HS) if do_ext else 0
    q += EH * P + IP * P
    q += (JP * P + IP * RS) if do_f else 0
    q += (L * I3 * P + J3 * P) if do_z else 0
    q += (IP // 16) * L * TS if do_f else 0
    return q + 4 * TS


def records_beyond_one_level(bond, left, N, M, L):
    """Batch-side iterations of a whole sweep under the fixed truncation whose pre-gradient is beyond one level (sweep_persist and
    pipe_try_one_level of tnml_api.hip), and the bonds the sweep leaves.  bond: the N - 1 bonds in site order."""
    rb = list(bond[::-1] if left else bond)                      # bonds in the sweep's own frame
    at = lambda i: rb[i] if 0 <= i < N - 1 else 1
    # the prologue: Z_0 has the rows of d_0 alone
    gn = at(1)
    count = int(16 * (D * D * gn * L + 4) > batch_lds_floats(L, 1, 1, gn, 1, True, False, False, True))
    for k in range(N - 1):
        hj, gj, gn, hprev = at(k - 1), at(k + 1), at(k + 2), at(k - 2)
        do_z = k + 1 <= N - 2
        if do_z:
            zsize = hj * D * D * D * gn * L
            count += int(16 * (zsize + 4) > batch_lds_floats(L, hj, gj, gn, hprev, False, k >= 1, True, True))
        rb[k] = min(M, D * hj, D * gj * L)
    return count, (rb[::-1] if left else rb)


HP = {True: (1e-2, 1e-3, True, 'softmax', 'full_cross_ent', 0.1, 'fixed'),
      False: (1e-2, 1e-3, False, 'softmax', 'full_cross_ent', 0.1, 'fixed')}

CASES = [(16, 20, 2, 33), (16, 20, 2, 512), (16, 20, 2, 513), (16, 20, 2, 1000), (16, 20, 2, 5000), (10, 5, 3, 513)]


def three_sweeps(N, M, L, X, y, cores32, mode, reduce, l2):
    """right, left, right from the calibrated start; -> per sweep: (results for bit comparison, slice steps, path, bonds before)"""
    ctx = new_ctx(N, L, M, X, y, cores32, 0, mode)
    ctx.set_persist_reduce(reduce)
    out = []
    for sw in range(3):
        left = sw == 1
        bond_before = [int(v) for v in ctx.get_cores()[1]]
        met, f, cnt = device_sweep(ctx, left, HP[l2])
        out.append(((met, f, ctx.get_cores()), ctx.slice_reduce_steps(), path_of(cnt, N), bond_before))
    ctx.close()
    return out


@pytest.mark.parametrize('l2', [True, False])
@pytest.mark.parametrize('N,M,L,b', CASES)
def test_slices_equal_last_arrivers_bit_for_bit(N, M, L, b, l2):
    X, y, cores32 = prepare(N, M, L, b, 31)
    new = three_sweeps(N, M, L, X, y, cores32, 1, 1, l2)
    old = three_sweeps(N, M, L, X, y, cores32, 1, 0, l2)
    roles = three_sweeps(N, M, L, X, y, cores32, 2, 1, l2)
    again = three_sweeps(N, M, L, X, y, cores32, 1, 1, l2)
    counts = []
    for sw in range(3):
        left = sw == 1
        want, _ = records_beyond_one_level(new[sw][3], left, N, M, L)
        counts.append((new[sw][1], want))
        print('N', N, 'bond', M, 'L', L, 'b', b, 'L2', l2, 'sweep', sw, 'slice steps', new[sw][1], 'records beyond one level', want,
              'switch 0:', old[sw][1], 'mode 2:', roles[sw][1])
        assert [r[sw][2] for r in (new, old, roles, again)] == ['persistent'] * 4
        assert_same(new[sw][0], old[sw][0])              # slices == last arrivers
        assert_same(new[sw][0], roles[sw][0])            # one kernel == one kernel per role
        assert_same(new[sw][0], again[sw][0])            # a fresh context repeats the bits
        assert new[sw][1] == want and roles[sw][1] == want and again[sw][1] == want
        assert old[sw][1] == 0
        if M == 20:
            assert new[sw][1] > 0                         # the new form ran
    assert sum(c for c, _ in counts) > 0
