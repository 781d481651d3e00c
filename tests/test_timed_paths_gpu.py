"""The two paths bench.py times, held to the float64 oracle step by step.

  * the persistent sweep (sweep_persist_kernel, kernels_narrow.hip: one launch per sweep; C2, C3, C4), modes 1 (one
    kernel) and 2 (one kernel per role);
  * the pipelined large-tensor step (the `bigpipe` branch of tnml_api.hip: wide_step_mfma_tiled_kernel, big_front_kernel,
    big_jacobi_kernel; C5).

Both are switched off by per-step capture (tnml_debug_enable) and by single-step calls, so the step-level tests of
test_hip_parity.py never run them.  Here a whole sweep runs as the benchmark runs it and every step is read back from
what the sweep leaves (tests/sweep_invariants.py): the Gram diagonal of each behind core is that step's kept singular
values, its off-diagonal the orthogonality of the kept singular vectors, and the behind environments are the batch side's
output (compared after an orthogonal Procrustes alignment).  Every case asserts the path that ran through the
context's counters.

Bounds (float32 device vs float64 oracle) are at most 10x the value observed on MI355X, which each assert states:
  sigma of every step        relative to that step's sigma_max; sweep 1 5e-6 .. 1.5e-4 (the per-step path's bound is 5e-4)
  Gram off-diagonal          relative to sigma_max
  behind environments        Procrustes-aligned, relative to max|E|
  f after the sweep, per-step accuracy (exact in sweep 1) and MAE
Sweep 2 starts every context and the oracle from one state (the first context's cores) and is bounded looser: these untrained
chains amplify float32 rounding in their second sweep (test_hip_parity.py::test_persistent_sweep_matches_per_step_launches_and_oracle).
"""
import numpy as np
import pytest

import sweep_invariants as si
from oracle import mps_oracle as mo

pytestmark = pytest.mark.gpu

D = 2


def hip():
    from tensornetworkforml_amd import _hip
    return _hip


def relerr(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def tiles_per_wg(b, num_cus=256):
    """Sample tiles each batch-side workgroup of the persistent sweep loops over (sweep_persist in tnml_api.hip) on the
    MI355X's 256 CUs."""
    ntiles = (b + 31) // 32
    tpw = (ntiles + max(16, num_cus - 16) - 1) // max(16, num_cus - 16)
    while (ntiles + tpw - 1) // tpw + 1 + 8 > num_cus:
        tpw += 1
    return tpw


def prepare(N, M, L, b, seed, zero_frac=0.6):
    """Inputs and a calibrated random start, float32-rounded on both sides."""
    rng = np.random.default_rng(seed)
    p = rng.random((b, N)) * (rng.random((b, N)) > zero_frac)
    X = np.stack([np.sin(np.pi * p / 2), np.cos(np.pi * p / 2)], -1).astype(np.float32)
    y = rng.integers(0, L, b).astype(np.int32)
    st = mo.MPSState(N, D, L, M, mo.random_cores(N, M, D, L, rng=rng, scale=M * 0.5 * 0.64 * D))
    mo.calibrate(st, X.astype(np.float64))
    cores32 = [c.astype(np.float32) for c in st.cores]
    return X, y, cores32


def new_ctx(N, L, M, X, y, cores32, l_pos=0, persistent=1):
    ctx = hip().Context(N, D, L, M, X.shape[0])
    ctx.set_persistent(persistent)
    ctx.set_cores(cores32, l_pos)
    ctx.set_input(X, y)
    return ctx


def state_of(cores, l_pos, M, L):
    N = len(cores)
    return mo.MPSState(N, D, L, M, [c.astype(np.float64) for c in cores], l_pos=int(l_pos))


def device_sweep(ctx, left, hp):
    """forward + one whole sweep as the benchmark runs it; returns (metrics, f, counters of that sweep)."""
    ctx.profile_reset()
    ctx.forward(want_f=False)
    met, f = ctx.sweep(left, ctx.N - 1, True, *hp)
    return met, f, ctx.counters()


def compare(ctx, met, f_d, o, left, b):
    """The sweep the device just ran against the oracle's record `o` (si.oracle_sweep)."""
    cores_d, bond_d, lp = ctx.get_cores()
    N = ctx.N
    assert [len(s) for s in o['S']] == [int(bond_d[si.behind_site(N, k, left)[0]]) for k in range(N - 1)]
    assert lp == (0 if left else N - 1)
    diag, off = si.step_sigmas(cores_d, bond_d, left)
    side = hip().SIDE_RIGHT if left else hip().SIDE_LEFT
    env = max([si.env_residual(ctx.get_env(side, s), E) for s, E in o['env'].items()] or [0.0])
    return dict(sigma=float(si.sigma_errors(diag, o['S']).max()), off=float(off.max()), env=float(env),
                f=float(relerr(f_d, o['f'])), acc=float(np.abs(met[:, 0] - o['accuracy']).max() * b),
                mae=float(np.abs(met[:, 1] - o['MAE']).max()))


def path_of(cnt, N):
    if cnt['launches'] == 1 and cnt['sweep_steps'] == N - 1 and cnt['pipelined_steps'] == N - 1:
        return 'persistent'
    assert cnt['sweep_steps'] == N - 1 and cnt['launches'] >= N - 1, cnt
    return 'per-step'


def two_sweeps(N, M, L, b, seed, hp, modes=(1, 2), zero_frac=0.6):
    """Sweep 1 (right, from the calibrated start) and sweep 2 (left, every context and the oracle from the cores the
    first context left) on contexts of the given persistence modes.  Returns (per-sweep observations of the first
    context, per-sweep paths, results of every context for bit comparisons)."""
    X, y, cores32 = prepare(N, M, L, b, seed, zero_frac)
    X64 = X.astype(np.float64)
    ctxs = [new_ctx(N, L, M, X, y, cores32, 0, mode) for mode in modes]
    okw = dict(L2_flag=hp[2], act_fn=hp[3], loss_fn=hp[4], T=hp[5], trunc=hp[6])
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
        out = []
        for i, ctx in enumerate(ctxs):
            met, f_d, cnt = device_sweep(ctx, left, hp)
            out.append((met, f_d, ctx.get_cores()))
            if i == 0:
                obs.append(compare(ctx, met, f_d, o, left, b))
                paths.append(path_of(cnt, N))
        res.append(out)
    for ctx in ctxs:
        ctx.close()
    return obs, paths, res


def assert_same(a, b):
    (ma, fa, (ca, bonda, lpa)), (mb, fb, (cb, bondb, lpb)) = a, b
    np.testing.assert_array_equal(ma, mb)
    np.testing.assert_array_equal(fa, fb)
    assert list(bonda) == list(bondb) and lpa == lpb
    for x, y_ in zip(ca, cb):
        np.testing.assert_array_equal(x, y_)


HP_SOFT = (1e-2, 1e-3, True, 'softmax', 'full_cross_ent', 0.1, 'fixed')


def fmt(d):
    return {k: '%.2e' % v for k, v in d.items()}


# ---------------------------------------------------------------------------------------------------------------
# a. the extraction itself, on the per-step path where the device's singular values can be captured
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('large', [False, True])
def test_gram_of_behind_core_equals_captured_sigma(large):
    N, M, L, b = 12, 10, 3, 100
    X, y, cores32 = prepare(N, M, L, b, 4)
    ctx = new_ctx(N, L, M, X, y, cores32)
    ctx.set_narrow_path(large)
    ctx.debug_enable(True)
    worst = dict(diag=0.0, off=0.0)
    for left in (False, True):
        ctx.forward(want_f=False)
        for k in range(N - 1):
            ctx.sweep(left, 1, k == 0, *HP_SOFT)
            sig = ctx.step_debug('sigma')
            cores_d, bond_d, _ = ctx.get_cores()
            p, site = si.behind_site(N, k, left)
            A = cores_d[site].astype(np.float64)
            G = np.einsum('kdc,jdc->kj', A, A) if left else np.einsum('adk,adj->kj', A, A)
            m = int(bond_d[p])
            assert G.shape == (m, m)
            worst['diag'] = max(worst['diag'], np.abs(np.diag(G) - sig[:m]).max() / sig[0])
            worst['off'] = max(worst['off'], np.abs(G - np.diag(np.diag(G))).max() / sig[0])
    ctx.close()
    print('extraction', 'large' if large else 'lds', fmt(worst))
    assert worst['diag'] < 3e-6 and worst['off'] < 3e-6      # observed 3.7e-7 / 3.5e-7 (float32 rounding of the cores)


# ---------------------------------------------------------------------------------------------------------------
# b, c. the persistent sweep: sweep 1 from the calibrated start, sweep 2 from one common start
# ---------------------------------------------------------------------------------------------------------------
PERSIST_CASES = [
    # the five shapes of test_persistent_sweep_matches_per_step_launches_and_oracle
    ('fixed', 20, 48, 300, 2), ('reference', 10, 40, 130, 2), ('fixed', 12, 25, 77, 3), ('fixed', 8, 33, 64, 2),
    ('reference', 3, 14, 9, 2),
    ('fixed', 6, 12, 300, 10),          # ten labels at a small bond
    ('fixed', 8, 16, 1, 2),             # one sample: one padded tile
    ('fixed', 12, 20, 7713, 2),         # two tiles per batch-side workgroup, the last tile holds one sample
    ('fixed', 20, 32, 20000, 2),        # the C4 single-GPU batch: three tiles per batch-side workgroup
]


@pytest.mark.parametrize('policy,M,N,b,L', PERSIST_CASES)
def test_persistent_sweep_step_by_step(policy, M, N, b, L):
    hp = (1e-2, 1e-3, True, 'softmax', 'full_cross_ent', 0.1, policy)
    obs, paths, res = two_sweeps(N, M, L, b, 11, hp)
    for sw in range(2):
        assert_same(res[sw][0], res[sw][1])            # modes 1 and 2: the same arithmetic in one kernel or three
    print('persistent', policy, M, N, b, L, 'tpw', tiles_per_wg(b), paths, 'sweep 1', fmt(obs[0]), 'sweep 2', fmt(obs[1]))
    assert paths == ['persistent', 'persistent']
    if b > 7680:
        assert tiles_per_wg(b) >= 2
    o1, o2 = obs
    # observed over the nine cases, sweep 1: sigma 7.8e-7, off-diagonal 7.8e-7, environments 1.8e-6, f 1.3e-6, MAE 9.9e-8,
    # accuracy exact; sweep 2 (amplifies rounding, worst at bond 20, N = 48): sigma 2.2e-3, off-diagonal 1.6e-5, environments
    # 1.0e-3, f 1.1e-2, MAE 2.0e-6, accuracy within one sample
    assert o1['sigma'] < 5e-6 and o1['off'] < 5e-6 and o1['env'] < 1e-5
    assert o1['f'] < 1e-5 and o1['acc'] < 0.5 and o1['mae'] < 1e-6
    assert o2['sigma'] < 1e-2 and o2['off'] < 1e-4 and o2['env'] < 1e-2
    assert o2['f'] < 1e-1 and o2['acc'] <= 1.0 + 1e-3 and o2['mae'] < 2e-5


@pytest.mark.parametrize('act', mo.ACTS)
@pytest.mark.parametrize('loss', mo.LOSSES)
@pytest.mark.parametrize('l2', [True, False])
def test_persistent_sweep_activations_and_losses(act, loss, l2):
    N, M, L, b = 12, 6, 3, 40
    hp = (1e-2, 1e-3, l2, act, loss, 0.1, 'fixed')
    obs, paths, res = two_sweeps(N, M, L, b, 5, hp)
    for sw in range(2):
        assert_same(res[sw][0], res[sw][1])
    print('persistent', act, loss, 'L2' if l2 else 'no L2', paths, 'sweep 1', fmt(obs[0]), 'sweep 2', fmt(obs[1]))
    assert paths == ['persistent', 'persistent']
    o1, o2 = obs
    # observed over the 18 cases, sweep 1: sigma 1.6e-5, off-diagonal 8.6e-7, environments 3.4e-5, f 3.9e-5 (all worst at sigmoid +
    # full_cross_ent), MAE 5.3e-7, accuracy exact; sweep 2: sigma 4.1e-4, off-diagonal 3.1e-7, environments 2.2e-5, f 3.2e-5,
    # MAE 6.0e-7, accuracy exact
    assert o1['sigma'] < 1.5e-4 and o1['off'] < 5e-6 and o1['env'] < 3e-4
    assert o1['f'] < 3e-4 and o1['acc'] < 0.5 and o1['mae'] < 5e-6
    assert o2['sigma'] < 4e-3 and o2['off'] < 3e-6 and o2['env'] < 2e-4
    assert o2['f'] < 3e-4 and o2['acc'] < 0.5 and o2['mae'] < 5e-6


@pytest.mark.parametrize('M', [32, 33])
def test_persistent_plan_at_the_edge_of_the_lds_regime(M):
    """Two labels, bond 32: from the sixth step on the merged tensor is 64 x 128 with 8192 elements, the largest
    sweep_persist's shape checks admit (nn == 64, bsize == 8192) -- but the plan as a whole does not fit at this bond, so
    the per-step launches run (measured on MI355X; asserted, so a change shows).  Bond 33 crosses the shape limit at
    the seventh step, after six steps were planned: sweep_persist gives up, restores bonds, label position and label
    buffer, and the per-step launches run -- bit for bit what a context with the persistent sweep turned off computes."""
    N, L, b = 16, 2, 200
    obs, paths, res = two_sweeps(N, M, L, b, 13, HP_SOFT, modes=(1, 0))
    for sw in range(2):
        if M == 33:
            assert_same(res[sw][0], res[sw][1])
    print('edge M =', M, paths, 'sweep 1', fmt(obs[0]), 'sweep 2', fmt(obs[1]))
    # (bond 32 does not fit the persistent plan either: sweep_persist declines it and the per-step launches run)
    assert paths == ['per-step', 'per-step']
    o1, o2 = obs
    # observed (M = 32 / 33), sweep 1: sigma 9.1e-7 / 1.5e-7, off-diagonal 3.0e-7 / 3.4e-7, environments 2.0e-6 / 1.8e-6, f 1.2e-6 /
    # 1.1e-6, MAE 8.2e-8 / 7.0e-8; sweep 2: sigma 2.1e-6 / 1.2e-5, off-diagonal 2.9e-6 / 2.6e-6, environments 5.8e-6 / 8.0e-6,
    # f 2.2e-6 / 2.0e-6, MAE 2.7e-7 / 1.9e-7; accuracy exact
    assert o1['sigma'] < 9e-6 and o1['off'] < 3e-6 and o1['env'] < 2e-5
    assert o1['f'] < 1e-5 and o1['acc'] < 0.5 and o1['mae'] < 8e-7
    assert o2['sigma'] < 1.2e-4 and o2['off'] < 2.8e-5 and o2['env'] < 8e-5
    assert o2['f'] < 2e-5 and o2['acc'] < 0.5 and o2['mae'] < 2.7e-6


# ---------------------------------------------------------------------------------------------------------------
# d. the pipelined large-tensor step (C5's path) against the oracle
# ---------------------------------------------------------------------------------------------------------------
def small_steps(N, M, L):
    """Steps of a right sweep from the random start (all bonds M) whose matrix side is <= 64: an upper bound on the
    steps the in-LDS path takes."""
    bond = [M] * (N - 1)
    n = 0
    for p in range(N - 1):
        h = 1 if p == 0 else bond[p - 1]
        g = 1 if p + 1 == N - 1 else bond[p + 1]
        n += min(D * h, D * g * L) <= 64
        bond[p] = min(M, min(D * h, D * g * L))
    return n


@pytest.mark.parametrize('N,b', [(16, 2000), (12, 8200)])
def test_large_tensor_sweep_vs_oracle(N, b):
    """Bond 50, ten labels.  At b = 2000 the mid-chain steps are pipelined (the batch kernel of step k+1 beside the SVD
    of step k; tnml_get_counters counts them with the single-launch steps); beyond 7680 samples (more than one sample
    tile per batch workgroup) no step is pipelined: the classic large-tensor sequence runs (`nblk <= pipe_nwide` in
    tnml_api.hip)."""
    M, L = 50, 10
    hp = (1e-3, 1e-3, True, 'softmax', 'full_cross_ent', 0.1, 'fixed')
    X, y, cores32 = prepare(N, M, L, b, 21)
    X64 = X.astype(np.float64)
    ctx = new_ctx(N, L, M, X, y, cores32)
    st = state_of(cores32, 0, M, L)
    f_o = mo.forward(st, X64)
    o = si.oracle_sweep(st, X64, y, f_o, hp[0], hp[1], left_dir=False, L2_flag=True, act_fn=hp[3], loss_fn=hp[4],
                        T=hp[5], trunc='fixed')
    met, f_d, cnt = device_sweep(ctx, False, hp)
    obs = compare(ctx, met, f_d, o, False, b)
    ctx.close()
    n_small = small_steps(N, M, L)
    piped_big = cnt['pipelined_steps'] - (n_small + 1)
    print('large-tensor sweep N', N, 'b', b, fmt(obs), 'pipelined steps', cnt['pipelined_steps'], 'of which large >=', piped_big)
    if b <= 7680:
        assert piped_big >= N - 1 - n_small - 4, cnt                # observed 4 of the 8 large steps (a lower bound)
    else:
        assert cnt['pipelined_steps'] == 0, cnt
    # observed (b = 2000 / 8200): sigma 1.8e-6 / 3.7e-6, off-diagonal 1.5e-6 / 1.5e-6, environments 1.2e-6 / 9.1e-7, f 1.2e-6 /
    # 1.2e-6, MAE 2.0e-8 / 2.3e-8, accuracy exact
    assert obs['sigma'] < 3e-5 and obs['off'] < 1.5e-5 and obs['env'] < 1.2e-5
    assert obs['f'] < 1.2e-5 and obs['acc'] < 0.5 and obs['mae'] < 2e-7
