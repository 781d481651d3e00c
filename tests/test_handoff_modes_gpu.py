"""The two forms of the hand-offs between a context's two streams (tnml_set_flag_handoffs): sequence numbers in memory (default) and
events.  Both forms run the same kernels with the same reduction order, so whole sweeps must agree bit for bit: cores, bonds, f and
the per-step metrics.  Two launch paths have such hand-offs:
  (a) the large-tensor pipeline (batch kernel of step k+1 on the side stream beside the SVD of step k): N = 8, bond 6, two labels,
      batch 96; steps 2 to 5 satisfy k >= 2 && k + 1 <= N - 2, so steps fed by Z, steps that feed Z and classic steps all occur;
  (b) the two-stream communicator step (update side / batch side + all-reduce): N = 6, bond 4, batch 40, with a one-rank
      communicator (TNML_FORCE_COMM=1) in a fresh child process per form, each under its own time limit.
One forward + full right sweep and one forward + full left sweep per run, fixed truncation, L2 term on.
Observed on the build before the per-step planner was split into one function per path: both cases bit-equal."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

HP = (1e-3, 1e-3, True, 'softmax', 'full_cross_ent', 0.1, 'fixed')


def problem(N, M, b, L=2, D=2, seed=17):
    from oracle import mps_oracle as mo
    rng = np.random.default_rng(seed)
    p = rng.random((b, N)) * (rng.random((b, N)) > 0.5)
    X = np.stack([np.sin(np.pi * p / 2), np.cos(np.pi * p / 2)], -1).astype(np.float32)
    y = rng.integers(0, L, b)
    cores = mo.random_cores(N, M, D, L, rng=rng, scale=M * 0.5 * 0.64 * D)
    st = mo.MPSState(N, D, L, M, cores)
    mo.calibrate(st, X.astype(np.float64))
    return X, y, [c.astype(np.float32) for c in st.cores]


def run_sweeps(N, M, b, flags, large, comm):
    """-> dict of arrays: f and metrics of both sweeps, bonds and cores at the end"""
    from tensornetworkforml_amd import _hip
    from tensornetworkforml_amd import dist as tdist
    L, D = 2, 2
    X, y, cores = problem(N, M, b, L, D)
    ctx = _hip.Context(N, D, L, M, b)
    ctx.set_cores(cores, 0)
    ctx.set_input(X, y)
    ctx.set_persistent(0)
    if large:
        ctx.set_narrow_path(1)
    if comm:
        tdist.attach_comm(ctx, 0, 1)
    ctx.set_flag_handoffs(flags)
    out = two_sweeps(ctx, N)
    ctx.close()
    return out


def two_sweeps(ctx, N):
    """forward + right sweep, forward + left sweep -> dict of arrays: f and metrics of both, bonds and cores at the end"""
    out = {}
    for sw in range(2):
        ctx.forward()
        met, f = ctx.sweep(ctx.l_pos == N - 1, N - 1, True, *HP)
        out['met%d' % sw], out['f%d' % sw] = met, f
    cs, bond, lp = ctx.get_cores()
    out['bond'] = bond
    out['l_pos'] = np.array([lp])
    for i, c in enumerate(cs):
        out['core%d' % i] = c
    return out


def assert_same(a, b):
    assert sorted(a) == sorted(b)
    for k in sorted(a):
        assert np.all(np.isfinite(a[k])), k
        np.testing.assert_array_equal(np.asarray(a[k]), np.asarray(b[k]), err_msg=k)


def test_large_tensor_pipeline_flags_equal_events():
    N = 8
    res = [run_sweeps(N, 6, 96, flags, large=True, comm=False) for flags in (True, False)]
    assert res[0]['met0'].shape == (N - 1, 2) and int(res[0]['l_pos'][0]) == 0
    assert_same(res[0], res[1])


def test_large_tensor_pipeline_after_batch_growth():
    """The pipelined large-tensor step keeps one buffer of the batch's padded width of its own (E_k (x) x_k, allocated at its first
    use).  A context that has run such sweeps at 96 samples (padded width 128) and then takes 200 (256) must hand the kernels a
    buffer of the new width: its sweeps on the 200 samples agree bit for bit with those of a context created at 200 that starts
    from the same cores.  (Before the buffer was sized with the rest of the batch's buffers the first context wrote past its end.)"""
    from tensornetworkforml_amd import _hip
    N, M, L, D = 8, 6, 2, 2
    X1, y1, cores = problem(N, M, 96)
    X2, y2, _ = problem(N, M, 200)

    def context(cap, cores, l_pos):
        ctx = _hip.Context(N, D, L, M, cap)
        ctx.set_cores(cores, l_pos)
        ctx.set_persistent(0)
        ctx.set_narrow_path(1)
        return ctx
    a = context(96, cores, 0)
    a.set_input(X1, y1)
    two_sweeps(a, N)
    cores1, _, l_pos1 = a.get_cores()
    a.set_input(X2, y2)
    grown = two_sweeps(a, N)
    a.close()
    b = context(200, cores1, l_pos1)
    b.set_input(X2, y2)
    fresh = two_sweeps(b, N)
    b.close()
    assert grown['met0'].shape == (N - 1, 2) and grown['f0'].shape == (L, 200) and l_pos1 == 0
    assert_same(grown, fresh)


def test_two_stream_communicator_step_flags_equal_events(tmp_path):
    N = 6
    res = []
    for flags in (1, 0):
        out = str(tmp_path / ('flags%d.npz' % flags))
        env = dict(os.environ, TNML_FORCE_COMM='1')
        r = subprocess.run([sys.executable, os.path.abspath(__file__), str(flags), out], cwd=ROOT, env=env, capture_output=True,
                           text=True, timeout=120)
        assert r.returncode == 0, (flags, r.returncode, r.stdout[-2000:], r.stderr[-2000:])     # (nothing more runs after a failure)
        with np.load(out) as d:
            res.append({k: d[k] for k in d.files})
    assert res[0]['met0'].shape == (N - 1, 2) and int(res[0]['l_pos'][0]) == 0
    assert_same(res[0], res[1])


if __name__ == '__main__':
    np.savez(sys.argv[2], **run_sweeps(6, 4, 40, bool(int(sys.argv[1])), large=False, comm=True))
