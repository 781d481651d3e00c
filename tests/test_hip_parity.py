"""GPU parity tests: the HIP path (through the C ABI of include/tnml.h) against the golden vectors
of the reference and against the float64 oracle on the same seeded inputs.

Tolerances (the device computes in float32, the reference in float64):
  forward f / environments        rtol 2e-5 of max|.|
  per-step B, B_new, L2 term      rtol 5e-3 of max|.|   after aligning the +-1 gauge of the SVD
                                                        (observed 1e-6 .. 1e-5; 8e-4 with near-degenerate
                                                        singular values, where B is gauge dependent)
  per-step dB_raw                 rtol 5e-3 of max|.|   (1/(f-1+1e-4) amplifies float32 noise; observed <= 6e-4)
  singular values                 rtol 5e-4 of sigma_max (observed <= 1.3e-4)
  persistent sweep (one launch)   sigma of every step from the Gram diagonal of its behind core (tests/sweep_invariants.py):
                                  5e-6 of sigma_max in sweep 1 (observed 7.8e-7), 1e-2 in sweep 2 (2.2e-3); f 1e-5 in sweep 1,
                                  4.5e-2 in sweep 2 (1.5e-2; the two device forms 1.4e-2 apart, observed 4.9e-3)
  f after every step              rtol 5e-3 of max|f|   (observed <= 1e-5)
  accuracy per step               exact;  MAE 2e-3 (observed <= 6e-7)
"""
import numpy as np
import pytest

import golden_util as gu
import sweep_invariants as si
from oracle import mps_oracle as mo

pytestmark = pytest.mark.gpu


def hip():
    from tensornetworkforml_amd import _hip
    return _hip


def relerr(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def make_ctx(N, D, L, M, cores, l_pos, X, y=None):
    ctx = hip().Context(N, D, L, M, X.shape[0])
    ctx.set_cores(cores, l_pos)
    ctx.set_input(X, y)
    return ctx


@pytest.mark.parametrize('name', gu.names('forward_'))
def test_forward_golden(name):
    d = gu.load(name)
    N, M, L, D = int(d['N']), int(d['M']), int(d['L']), int(d['D'])
    for tag, X, l_pos in (('a_', d['X'], 0), ('b_', d['X2'], N - 1)):
        ctx = make_ctx(N, D, L, M, gu.indexed(d, tag + 'core', N), l_pos, X)
        f = ctx.forward()
        assert relerr(f, d[tag + 'f']) < 2e-5
        side = hip().SIDE_RIGHT if l_pos == 0 else hip().SIDE_LEFT
        nm = 'Renv' if l_pos == 0 else 'Lenv'
        sites = range(1, N) if l_pos == 0 else range(0, N - 1)
        for i in sites:
            e = ctx.get_env(side, i)
            assert relerr(e, d['%s%s%d' % (tag, nm, i)]) < 2e-5, (tag, i)
        ctx.close()


def _kw(d):
    return dict(lr=float(d['lr']), weight_dec=float(d['wd']), L2_flag=bool(d['L2_flag']),
                act_fn=str(d['act_fn']), loss_fn=str(d['loss_fn']), T=float(d['T']), trunc=str(d['policy']))


def canon_to(d_arr, shape):
    return np.asarray(d_arr).reshape(shape)


gauge_signs, regauge = gu.gauge_signs, gu.regauge


BIG_PATH_CASES = ['traj_fixed_N16_script', 'traj_reference_N16_script', 'traj_fixed_L3', 'traj_fixed_L10',
                  'traj_fixed_softmax_full_cross_ent_L21', 'traj_reference_sigmoid_MSE_L20']


@pytest.mark.parametrize('name,large', [(n, False) for n in gu.names('traj_')] + [(n, True) for n in BIG_PATH_CASES])
def test_stepwise_vs_oracle_and_golden(name, large):
    """(`large`: the same through the large-tensor path.)
    Device and float64 oracle run the same sweeps side by side, one step per call; every step's
    merged tensor, raw gradient, weight-decay term, updated tensor, singular values, f and metrics
    are compared.  The oracle itself is pinned to the reference by tests/test_oracle_golden.py; the
    golden f_new / accuracy are checked directly too."""
    d = gu.load(name)
    N, M, L, D = int(d['N']), int(d['M']), int(d['L']), int(d['D'])
    kw = _kw(d)
    X, y = d['X'], d['y']
    cores0 = gu.indexed(d, 'init_core', N)
    st = mo.MPSState(N, D, L, M, cores0, 0)
    ctx = make_ctx(N, D, L, M, cores0, 0, X, y)
    ctx.set_narrow_path(large)       # True: the HBM-resident kernels (kernels_big.hip) instead of the in-LDS one
    ctx.debug_enable(True)
    y1h = mo.one_hot(y, L)
    k = 0
    worst = {'B': 0.0, 'dB_raw': 0.0, 'L2_grad': 0.0, 'B_new': 0.0}
    degenerate_seen = False

    def upd(key, v):
        worst[key] = max(worst.get(key, 0.0), v)

    for sw in range(int(d['n_sweeps'])):
        f_o = mo.forward(st, X)
        f_d = ctx.forward()
        upd('f_forward', relerr(f_d, f_o))
        assert relerr(f_d, d['sw%d_f_forward' % sw]) < 2e-3
        left_dir = st.l_pos == N - 1
        if left_dir:
            st.Renv = {}
        else:
            st.Lenv = {}
        for j in range(N - 1):
            rec = {}
            f_o = mo.sweep_step(st, f_o, y1h, left_dir=left_dir, record=rec, **kw)
            met, f_d = ctx.sweep(left_dir, 1, j == 0, kw['lr'], kw['weight_dec'], kw['L2_flag'], kw['act_fn'],
                                 kw['loss_fn'], kw['T'], kw['trunc'])
            shp = rec['B'].shape
            if not degenerate_seen:
                B_d = canon_to(ctx.step_debug('B'), shp)
                sa, tc = gauge_signs(B_d, rec['B'])
                upd('B', relerr(B_d, regauge(rec['B'], sa, tc)))
                upd('dB_raw', relerr(canon_to(ctx.step_debug('dB_raw'), shp), regauge(rec['dB_raw'], sa, tc)))
                upd('L2_grad', relerr(canon_to(ctx.step_debug('L2_grad'), shp), regauge(rec['L2_grad'], sa, tc)))
                upd('B_new', relerr(canon_to(ctx.step_debug('B_new'), shp), regauge(rec['B_new'], sa, tc)))
            # Once two kept singular values (nearly) coincide, the singular vectors -- hence every
            # later merged tensor -- are defined only up to a rotation inside that subspace: the
            # tensors stop being comparable element-wise, sigma / f / metrics still are.
            Sk = rec['S'][:rec['m'] + 1]
            if len(Sk) > 1 and np.min(-np.diff(Sk)) < 2e-3 * rec['S'][0]:
                degenerate_seen = True
            sig = ctx.step_debug('sigma')
            upd('sigma', np.abs(sig - rec['S']).max() / rec['S'].max())
            upd('f_new', relerr(f_d, f_o))
            upd('acc', abs(float(met[0, 0]) - rec['accuracy']))
            upd('MAE', abs(float(met[0, 1]) - rec['MAE']))
            assert ctx.l_pos == st.l_pos
            # golden (reference) values of the same step
            pre = 'st%d_' % k
            upd('f_new_vs_ref', relerr(f_d, d[pre + 'f_new']))
            k += 1
        cores_d, bond_d, lp = ctx.get_cores()
        assert list(bond_d) == list(st.bond)
    print(name, {kk: '%.2e' % v for kk, v in worst.items()})
    assert worst['f_forward'] < 2e-3
    # B is gauge dependent beyond signs when singular values are (nearly) degenerate: loose bound,
    # the tight ones are on sigma, f and the metrics
    assert worst['B'] < 5e-3 and worst['B_new'] < 5e-3
    assert worst['dB_raw'] < 5e-3
    assert worst['L2_grad'] < 5e-3
    assert worst['sigma'] < 2e-3   # 7e-4 on the near-degenerate N16 case (gauge-dependent L1 clipping)
    assert worst['f_new'] < 5e-3 and worst['f_new_vs_ref'] < 5e-3
    assert worst['acc'] < 1e-6
    assert worst['MAE'] < 2e-3
    # final forward against the reference
    assert relerr(ctx.forward(), d['final_f']) < 5e-3
    ctx.close()


@pytest.mark.parametrize('policy,M,N,b,L', [('fixed', 20, 48, 300, 2), ('reference', 10, 40, 130, 2),
                                            ('fixed', 12, 24, 77, 3),
                                            # C5-shaped (10 labels, bond 40): merged tensor 80 x 800, the large-tensor path
                                            ('fixed', 40, 10, 70, 10)])
def test_full_sweeps_vs_oracle(policy, M, N, b, L):
    """Whole sweeps in one call (n_steps = N-1): ragged batch sizes (padding lanes), headline-like
    bond, both directions."""
    rng = np.random.default_rng(5)
    D = 2
    p = rng.random((b, N)) * (rng.random((b, N)) > 0.6)
    X = np.stack([np.sin(np.pi * p / 2), np.cos(np.pi * p / 2)], -1)
    y = rng.integers(0, L, b)
    cores = mo.random_cores(N, M, D, L, rng=rng, scale=M * 0.5 * 0.64 * D)
    st = mo.MPSState(N, D, L, M, cores)
    mo.calibrate(st, X)
    # float32-rounded cores on both sides so that both start from the same numbers
    cores32 = [c.astype(np.float32) for c in st.cores]
    st = mo.MPSState(N, D, L, M, [c.astype(np.float64) for c in cores32])
    ctx = make_ctx(N, D, L, M, cores32, 0, X.astype(np.float32), y)
    kw = dict(lr=1e-2, weight_dec=1e-3, L2_flag=True, act_fn='softmax', loss_fn='full_cross_ent', T=0.1, trunc=policy)
    X64 = X.astype(np.float32).astype(np.float64)
    for sw in range(2):
        f_o = mo.forward(st, X64)
        f_d = ctx.forward()
        assert relerr(f_d, f_o) < 1e-3, sw
        left_dir = st.l_pos == N - 1
        vh = [[], []]
        f_o = mo.sweep(st, X64, y, f_o, kw['lr'], kw['weight_dec'], L2_flag=True, left_dir=left_dir, var_hist=vh,
                       act_fn=kw['act_fn'], loss_fn=kw['loss_fn'], T=kw['T'], trunc=policy)
        met, f_d = ctx.sweep(left_dir, N - 1, True, kw['lr'], kw['weight_dec'], True, kw['act_fn'], kw['loss_fn'],
                             kw['T'], policy)
        assert relerr(f_d, f_o) < 5e-3, sw
        assert np.abs(met[:, 0] - np.array(vh[0])).max() <= 2.0 / b + 1e-6
        assert np.abs(met[:, 1] - np.array(vh[1])).max() < 2e-3
        _, bond_d, lp = ctx.get_cores()
        assert list(bond_d) == list(st.bond) and lp == st.l_pos
    # the network function on fresh inputs agrees (the only gauge-invariant view of the cores)
    p2 = rng.random((b, N))
    X2 = np.stack([np.sin(np.pi * p2 / 2), np.cos(np.pi * p2 / 2)], -1).astype(np.float32)
    ctx.set_input(X2, y)
    assert relerr(ctx.forward(), mo.forward(st, X2.astype(np.float64))) < 5e-3
    ctx.close()


def test_errors_mirror_reference():
    h = hip()
    rng = np.random.default_rng(0)
    N, M, L, D, b = 6, 3, 3, 2, 5
    cores = mo.random_cores(N, M, D, L, rng=rng, scale=M * 0.64)
    X = rng.random((b, N, D)).astype(np.float32)
    y = rng.integers(0, L, b)
    ctx = make_ctx(N, D, L, M, cores, 0, X, y)
    ctx.forward()
    # the reference raises ValueError at the last right step for L = 3 (Network_class.py:914)
    with pytest.raises(h.TnmlError) as ei:
        ctx.sweep(False, N - 1, True, 1e-3, 1e-3, True, 'softmax', 'full_cross_ent', 0.1, 'reference')
    assert ei.value.code == -6
    ctx.close()
    # forward at an intermediate label position raises (Network_class.py:258)
    ctx = make_ctx(N, D, L, M, cores, 0, X, y)
    ctx.forward()
    ctx.sweep(False, 2, True, 1e-3, 1e-3, True, 'softmax', 'full_cross_ent', 0.1, 'fixed')
    with pytest.raises(h.TnmlError) as ei:
        ctx.forward()
    assert ei.value.code == -2
    ctx.close()


def test_rccl_path_single_rank(monkeypatch):
    """The per-step all-reduce is an RCCL call issued by the library between the reduce and the
    update kernels.  With one GPU only a 1-rank communicator can be built (TNML_FORCE_COMM=1), which
    still exercises ncclCommInitRank, the max all-reduce of the calibration and 2(N-1) sum
    all-reduces on the context's stream; the result must equal the communicator-free run."""
    from tensornetworkforml_amd import dist as tdist
    d = gu.load('traj_fixed_N16_script')
    N, M, L, D = int(d['N']), int(d['M']), int(d['L']), int(d['D'])
    kw = _kw(d)
    outs = []
    for force in ('0', '1'):
        monkeypatch.setenv('TNML_FORCE_COMM', force)
        ctx = make_ctx(N, D, L, M, gu.indexed(d, 'init_core', N), 0, d['X'], d['y'])
        ctx.set_persistent(0)        # a communicator takes one launch per step: the same launches on the other side, bit for bit
        tdist.attach_comm(ctx, 0, 1)
        lmax = ctx.forward_logabsmax()
        ctx.forward()
        met, f = ctx.sweep(False, N - 1, True, kw['lr'], kw['weight_dec'], kw['L2_flag'], kw['act_fn'], kw['loss_fn'],
                           kw['T'], kw['trunc'])
        ctx.forward()
        met2, f2 = ctx.sweep(True, N - 1, True, kw['lr'], kw['weight_dec'], kw['L2_flag'], kw['act_fn'], kw['loss_fn'],
                             kw['T'], kw['trunc'])
        outs.append((lmax, met, f, met2, f2))
        ctx.close()
    for a, b in zip(outs[0], outs[1]):
        np.testing.assert_array_equal(np.asarray(a), np.asarray(b))


def test_large_tensor_pipeline_matches_classic_sequence():
    """Large-tensor steps (merged tensor beyond one workgroup's LDS: bond 50 with ten labels) are pipelined too (round 3): the batch
    kernel of step k+1 runs on a second stream beside the SVD of step k and leaves the reduced pre-gradient Z_{k+1}; the step then
    starts with the contraction A_k^T . Z (big_front_kernel, kernels_big.hip; the hand-offs between the two streams are sequence numbers
    in memory or -- third run below -- events: bit-equal).  Same sums in another association order: whole sweeps against the classic launch sequence (tnml_set_step_pipeline(0)), which the stepwise and
    true-shape tests hold against the oracle."""
    N, M, b, L, D = 24, 50, 2000, 10, 2
    rng = np.random.default_rng(21)
    p = rng.random((b, N)) * (rng.random((b, N)) > 0.6)
    X = np.stack([np.sin(np.pi * p / 2), np.cos(np.pi * p / 2)], -1).astype(np.float32)
    y = rng.integers(0, L, b)
    from tensornetworkforml_amd.Network_class import random_canonical_cores
    cores = random_canonical_cores(N, M, D, L, scale=M * 0.5 * 0.64 * D, rng=rng)
    hp = (1e-3, 1e-3, True, 'softmax', 'full_cross_ent', 0.1, 'fixed')
    res, piped = [], []
    for pipe, flags in ((0, True), (1, True), (1, False)):
        ctx = make_ctx(N, D, L, M, cores, 0, X, y)
        ctx.set_step_pipeline(pipe)
        ctx.set_flag_handoffs(flags)       # hand-offs between the two streams: sequence numbers in memory (default) / events
        ctx.scale_cores(1.0 / float(np.exp(ctx.forward_logabsmax() / N)))
        ctx.profile_reset()
        outs = []
        for sw in range(2):
            ctx.forward(want_f=False)
            outs.append(ctx.sweep(ctx.l_pos == N - 1, N - 1, True, *hp))
        piped.append(ctx.counters()['pipelined_steps'])
        res.append(outs)
        ctx.close()
    assert piped[0] == 0 and piped[1] >= 2 * (N - 1) - 16, piped       # the pipelined sequence really ran on the mid-chain steps
    for (ma, fa), (mb, fb) in zip(res[1], res[2]):                        # the same kernels, the same arithmetic: bit for bit
        np.testing.assert_array_equal(np.asarray(ma), np.asarray(mb))
        np.testing.assert_array_equal(np.asarray(fa), np.asarray(fb))
    obs = []
    for sw in range(2):
        (m0, f0), (m1, f1) = res[0][sw], res[1][sw]
        obs.append((relerr(f1, f0), float(np.abs(m0[:, 0] - m1[:, 0]).max()) * b, float(np.abs(m0[:, 1] - m1[:, 1]).max())))
    print('large-tensor pipeline vs classic sequence (f, accuracy in samples, MAE) per sweep:', obs)
    assert obs[0][0] < 3e-5 and obs[0][1] <= 1.0 + 1e-3 and obs[0][2] < 1e-6        # observed 2e-6, 0, 3e-8
    assert obs[1][0] < 5e-3 and obs[1][1] <= 3.0 + 1e-3 and obs[1][2] < 1e-5        # observed 2e-4, 1, 1e-7 (the second sweep of a fresh network amplifies)


def test_rccl_exchange_beside_the_svd(monkeypatch):
    """With a communicator the pipelined step is launched in two parts -- update side on the context's stream, batch side +
    all-reduce of the pre-gradient on a second stream (tnml_set_comm_overlap, default on) -- so that the exchange starts when
    Z is final (~25 us into a ~57 us step) instead of after the SVD.  On one GPU (TNML_FORCE_COMM=1: a one-rank communicator):
      * bit-equal f, metrics and cores to the fused launch with the all-reduce between launches and to the communicator-free
        per-step launches (the same kernels and the same arithmetic; the one-rank sum is the identity);
      * the device time of a C3-shaped sweep against the communicator-free per-step launches: within 3 us per step (observed
        +1.4: 65.0 -> 66.4 us).  The two hand-offs of a split step (update launch waits for the exchange, batch-side launch waits for
        the previous update launch) are sequence numbers in memory: the update workgroup polls / stores them itself, the side
        stream runs a one-wave gate kernel and a one-thread signal kernel.  As two cross-queue EVENT dependencies they cost 10 us
        per step (65.2 -> 75.1 us: an event costs the stream that records or waits 6-7 us even when it is already satisfied)."""
    from tensornetworkforml_amd import dist as tdist
    N, M, b, L, D = 96, 20, 5000, 2, 2
    rng = np.random.default_rng(5)
    p = rng.random((b, N)) * (rng.random((b, N)) > 0.8)
    X = np.stack([np.sin(np.pi * p / 2), np.cos(np.pi * p / 2)], -1).astype(np.float32)
    y = rng.integers(0, L, b)
    cores = mo.random_cores(N, M, D, L, rng=rng, scale=M * 0.5 * 0.64 * D)
    st = mo.MPSState(N, D, L, M, cores)
    mo.calibrate(st, X[:500].astype(np.float64))
    cores32 = [c.astype(np.float32) for c in st.cores]
    hp = (1e-3, 1e-3, True, 'softmax', 'full_cross_ent', 0.1, 'fixed')
    res, us = {}, {}
    for name, force, overlap, flags in (('no communicator', '0', True, True), ('fused + all-reduce between launches', '1', False, True),
                                        ('two streams', '1', True, True), ('two streams, event hand-offs', '1', True, False)):
        monkeypatch.setenv('TNML_FORCE_COMM', force)
        ctx = make_ctx(N, D, L, M, cores32, 0, X, y)
        ctx.set_persistent(0)
        tdist.attach_comm(ctx, 0, 1)
        ctx.set_comm_overlap(overlap)
        ctx.set_flag_handoffs(flags)
        outs = []
        for sw in range(4):
            ctx.forward(want_f=False)
            met, f = ctx.sweep(ctx.l_pos == N - 1, N - 1, True, *hp)
            outs.append((met, f))
        outs.append(tuple(ctx.get_cores()[0]))
        # device time of two more sweeps (HIP events on the context's stream around each tnml_sweep call; nothing waits inside)
        ctx.profile_reset()
        ctx.profile_enable(2)
        for sw in range(4):
            ctx.forward(want_f=False)
            ctx.sweep(ctx.l_pos == N - 1, N - 1, True, *hp, want_metrics=False, want_f=False)
        ms, _ = ctx.profile_get(4)
        us[name] = 1e3 * ms / (4 * (N - 1))
        res[name] = outs
        ctx.close()
    print('device time per step (us):', {k: round(v, 2) for k, v in us.items()})
    for other in ('fused + all-reduce between launches', 'two streams', 'two streams, event hand-offs'):
        for a, b_ in zip(res['no communicator'], res[other]):
            for x, y_ in zip(a, b_):
                np.testing.assert_array_equal(np.asarray(x), np.asarray(y_))
    assert us['two streams'] - us['no communicator'] < 3.0, us         # observed 1.4 (9.9 with events)
    assert us['two streams, event hand-offs'] > us['two streams'] + 3.0, us     # (the events are what the sequence numbers replaced: observed +8.5)
    assert abs(us['fused + all-reduce between launches'] - us['no communicator']) < 3.0, us


# default threshold: worst product error observed between 2.6e-6 and 2.6e-5 over builds that differ only in the rounding
# order of float64 sums (the worst step of two late sweeps is a tail statistic of a chaotic trajectory)
# (median, 90th percentile) bounds at <= 10 x the observed 9.9e-8 / 2.0e-6 (default), 1.8e-6 / 3.3e-5 (1e-4), 6.9e-8 / 1.1e-7 (1e-8)
MED_TOL = {None: (1e-6, 2e-5), 1e-4: (1.8e-5, 3.3e-4), 1e-8: (7e-7, 1.1e-6)}


@pytest.mark.parametrize('stop2,tol', [(None, 5e-5), (1e-4, 1e-3), (1e-8, 5e-6)])
def test_svd_accuracy_late_in_training(stop2, tol):
    """The Jacobi iteration stops early once its rotations are small (tnml_set_svd_stop); late in training
    that happens after few sweeps.  Every step of the 7th and 8th pass: the product of the two new cores
    against LAPACK's best rank-m approximation of the device's own updated merged tensor, and the kept
    singular values."""
    N, M, b, L, D = 20, 12, 600, 2, 2
    rng = np.random.default_rng(3)
    p = rng.random((b, N)) * (rng.random((b, N)) > 0.81)
    X = np.stack([np.sin(np.pi * p / 2), np.cos(np.pi * p / 2)], -1).astype(np.float32)
    y = rng.integers(0, L, b)
    st = mo.MPSState(N, D, L, M, mo.random_cores(N, M, D, L, rng=rng, scale=M * 0.5 * 0.64 * D))
    mo.calibrate(st, X.astype(np.float64))
    ctx = make_ctx(N, D, L, M, [c.astype(np.float32) for c in st.cores], 0, X, y)
    if stop2 is not None:
        ctx.set_svd_stop(stop2)
    hp = (1e-3, 1e-3, True, 'softmax', 'full_cross_ent', 0.1, 'fixed')

    def matricize(B, left):
        ml, _, _, mr, _ = B.shape
        return B.reshape(ml * D, D * mr * L) if not left else np.transpose(B, (0, 1, 4, 2, 3)).reshape(ml * D * L, D * mr)

    worst_prod = worst_sig = 0.0
    prods = []
    for ps in range(8):
        ctx.forward(want_f=False)
        left = ctx.l_pos == N - 1
        if ps < 6:
            ctx.sweep(left, N - 1, True, *hp, want_metrics=False, want_f=False)
            continue
        ctx.debug_enable(True)
        for k in range(N - 1):
            _, bond0, lp0 = ctx.get_cores()
            ctx.sweep(left, 1, k == 0, *hp)
            pp = lp0 - 1 if left else lp0
            ml = 1 if pp == 0 else int(bond0[pp - 1])
            mr = 1 if pp == N - 2 else int(bond0[pp + 1])
            Bm = matricize(ctx.step_debug('B_new').reshape(ml, D, D, mr, L), left)
            sig = ctx.step_debug('sigma')
            cores1, bond1, _ = ctx.get_cores()
            m = int(bond1[pp])
            A, C = cores1[pp].astype(np.float64), cores1[pp + 1].astype(np.float64)
            prod = np.einsum('adkl,kec->adecl', A, C) if A.ndim == 4 else np.einsum('adk,kecl->adecl', A, C)
            U, S, Vh = np.linalg.svd(Bm, full_matrices=False)
            best = (U[:, :m] * S[:m]) @ Vh[:m]
            prods.append(np.abs(matricize(prod, left) - best).max() / np.abs(Bm).max())
            worst_prod = max(worst_prod, prods[-1])
            worst_sig = max(worst_sig, (np.abs(sig[:m] - S[:m]) / S[0]).max())
        ctx.debug_enable(False)
    med, p90 = float(np.median(prods)), float(np.percentile(prods, 90))
    print('svd_stop2', stop2, 'product error: worst %.2e, median %.2e, 90th percentile %.2e; worst kept sigma error %.2e' % (worst_prod, med, p90, worst_sig))
    assert worst_prod < tol
    assert worst_sig < tol
    # the worst step is a tail statistic of a chaotic trajectory (it moved between 2.6e-6 and 2.6e-5 over builds that differ only
    # in the rounding order of float64 sums); the bulk of the distribution does not move and is held much tighter
    assert med < MED_TOL[stop2][0] and p90 < MED_TOL[stop2][1]
    ctx.close()


@pytest.mark.parametrize('large', [False, True])
def test_adaptive_truncation_vs_oracle(large):
    """trunc='adaptive' (labelled non-reference: the reference computes the index and never uses it,
    Network_class.py:889-891): the kept rank comes from the device's singular values; bond dimensions, f and
    metrics follow the oracle's over two sweeps."""
    N, M, b, L, D = 14, 12, 90, 2, 2
    rng = np.random.default_rng(21)
    p = rng.random((b, N)) * (rng.random((b, N)) > 0.6)
    X = np.stack([np.sin(np.pi * p / 2), np.cos(np.pi * p / 2)], -1).astype(np.float32)
    y = rng.integers(0, L, b)
    st = mo.MPSState(N, D, L, M, mo.random_cores(N, M, D, L, rng=rng, scale=M * 0.5 * 0.64 * D))
    mo.calibrate(st, X.astype(np.float64))
    cores32 = [c.astype(np.float32) for c in st.cores]
    st = mo.MPSState(N, D, L, M, [c.astype(np.float64) for c in cores32])
    ctx = make_ctx(N, D, L, M, cores32, 0, X, y)
    ctx.set_narrow_path(large)
    thr = 0.97
    ctx.set_trunc_threshold(thr)
    X64 = X.astype(np.float64)
    bonds_seen = set()
    for sw in range(2):
        f_o = mo.forward(st, X64)
        f_d = ctx.forward()
        assert relerr(f_d, f_o) < 1e-3
        left_dir = st.l_pos == N - 1
        vh = [[], []]
        f_o = mo.sweep(st, X64, y, f_o, 1e-2, 1e-3, L2_flag=True, left_dir=left_dir, var_hist=vh, act_fn='softmax',
                       loss_fn='full_cross_ent', T=0.1, trunc='adaptive', threshold=thr)
        met, f_d = ctx.sweep(left_dir, N - 1, True, 1e-2, 1e-3, True, 'softmax', 'full_cross_ent', 0.1, 'adaptive')
        _, bond_d, lp = ctx.get_cores()
        assert list(bond_d) == list(st.bond), (list(bond_d), list(st.bond))
        bonds_seen.update(int(v) for v in bond_d)
        assert relerr(f_d, f_o) < 5e-3
        assert np.abs(met[:, 0] - np.array(vh[0])).max() <= 2.0 / b + 1e-6
    assert len(bonds_seen) > 2 and min(bonds_seen) < M      # the rank really adapts
    ctx.close()


@pytest.mark.parametrize('N,M,b,L,policy', [(2, 2, 5, 2, 'fixed'), (2, 2, 5, 2, 'reference'), (3, 3, 1, 2, 'fixed'),
                                            (4, 1, 3, 2, 'fixed'), (5, 2, 33, 3, 'fixed'), (3, 2, 7, 2, 'reference'),
                                            (6, 4, 64, 2, 'adaptive')])
def test_tiny_chains_and_batches(N, M, b, L, policy):
    """Edge sizes: a two-site chain (the only step is first and last at once), one sample, bond 1, a batch that is
    exactly / not a multiple of the 32-sample tile: two sweeps against the oracle."""
    rng = np.random.default_rng(1)
    D = 2
    p = rng.random((b, N))
    X = np.stack([np.sin(np.pi * p / 2), np.cos(np.pi * p / 2)], -1).astype(np.float32)
    y = rng.integers(0, L, b)
    cores = [c.astype(np.float32) for c in mo.random_cores(N, M, D, L, rng=rng, scale=M * 0.64)]
    st = mo.MPSState(N, D, L, M, [c.astype(np.float64) for c in cores])
    ctx = make_ctx(N, D, L, M, cores, 0, X, y)
    X64 = X.astype(np.float64)
    for sw in range(2):
        f_o = mo.forward(st, X64)
        assert relerr(ctx.forward(), f_o) < 1e-4
        left = st.l_pos == N - 1
        vh = [[], []]
        f_o = mo.sweep(st, X64, y, f_o, 1e-2, 1e-3, L2_flag=True, left_dir=left, var_hist=vh, act_fn='softmax',
                       loss_fn='full_cross_ent', T=0.1, trunc=policy)
        met, f_d = ctx.sweep(left, N - 1, True, 1e-2, 1e-3, True, 'softmax', 'full_cross_ent', 0.1, policy)
        assert relerr(f_d, f_o) < 1e-3
        assert np.abs(met[:, 0] - np.array(vh[0])).max() < 1e-6
        _, bond, lp = ctx.get_cores()
        assert list(bond) == list(st.bond) and lp == st.l_pos
    ctx.close()


def test_batch_larger_than_the_capacity_given_at_creation():
    """tnml_create's b_capacity is a hint: a larger batch re-allocates the batch-sized buffers (and a smaller one
    afterwards must not see the old padding)."""
    N, M, L, D = 10, 4, 2, 2
    rng = np.random.default_rng(2)
    cores = [c.astype(np.float32) for c in mo.random_cores(N, M, D, L, rng=rng, scale=M * 0.64)]
    ctx = hip().Context(N, D, L, M, 16)
    ctx.set_cores(cores, 0)
    for b in (16, 300, 7):
        p = rng.random((b, N))
        X = np.stack([np.sin(np.pi * p / 2), np.cos(np.pi * p / 2)], -1).astype(np.float32)
        y = rng.integers(0, L, b)
        ctx.set_input(X, y)
        st = mo.MPSState(N, D, L, M, [c.astype(np.float64) for c in ctx.get_cores()[0]], ctx.l_pos)
        f_o = mo.forward(st, X.astype(np.float64))
        assert relerr(ctx.forward(), f_o) < 1e-4
        left = st.l_pos == N - 1
        f_o = mo.sweep(st, X.astype(np.float64), y, f_o, 1e-2, 1e-3, L2_flag=True, left_dir=left, act_fn='softmax',
                       loss_fn='full_cross_ent', T=0.1, trunc='fixed')
        _, f_d = ctx.sweep(left, N - 1, True, 1e-2, 1e-3, True, 'softmax', 'full_cross_ent', 0.1, 'fixed')
        assert relerr(f_d, f_o) < 1e-3, b
    ctx.close()


def test_counters_and_classic_sequence_agree_with_the_pipelined_step():
    """tnml_get_counters accounts for the steps that ran; the classic launch sequence (tnml_set_step_pipeline(0)) and the
    default single-launch step give the same sweep to float32 rounding."""
    d = gu.load('traj_fixed_N16_script')
    N, M, L, D = int(d['N']), int(d['M']), int(d['L']), int(d['D'])
    kw = _kw(d)
    outs = []
    for pipe in (True, False):
        ctx = make_ctx(N, D, L, M, gu.indexed(d, 'init_core', N), 0, d['X'], d['y'])
        ctx.set_persistent(False)            # one launch per step (the persistent sweep has its own test below)
        ctx.set_step_pipeline(pipe)
        ctx.profile_reset()
        ctx.forward()
        met, f = ctx.sweep(False, N - 1, True, kw['lr'], kw['weight_dec'], kw['L2_flag'], kw['act_fn'], kw['loss_fn'], kw['T'], kw['trunc'])
        cnt = ctx.counters()
        assert cnt['sweep_steps'] == N - 1 and cnt['forwards'] == 1
        assert cnt['algorithmic_bytes'] > 0 and cnt['algorithmic_flops'] > 0 and cnt['forward_bytes'] > 0
        assert cnt['pipelined_steps'] == (N if pipe else 0)          # N - 1 steps + the launch that starts the sweep
        assert cnt['launches'] >= N - 1
        outs.append((met, f))
        ctx.close()
    assert relerr(outs[0][1], outs[1][1]) < 1e-4
    assert np.abs(outs[0][0] - outs[1][0]).max() < 1e-5


@pytest.mark.parametrize('policy,M,N,b,L', [('fixed', 20, 48, 300, 2), ('reference', 10, 40, 130, 2), ('fixed', 12, 25, 77, 3),
                                            ('fixed', 8, 33, 64, 2), ('reference', 3, 14, 9, 2)])
def test_persistent_sweep_matches_per_step_launches_and_oracle(policy, M, N, b, L):
    """A full sweep as ONE persistent launch (default) against the same sweep as one launch per step and against the float64
    oracle: f, per-step metrics, bonds, and the network function afterwards; two sweeps (both directions; a third one of these
    untrained chains already amplifies float32 rounding past any useful bound on either path), ragged batches, chains of odd and
    even length (the label core ends in either of its two buffers)."""
    rng = np.random.default_rng(11)
    D = 2
    p = rng.random((b, N)) * (rng.random((b, N)) > 0.6)
    X = np.stack([np.sin(np.pi * p / 2), np.cos(np.pi * p / 2)], -1).astype(np.float32)
    y = rng.integers(0, L, b)
    cores = mo.random_cores(N, M, D, L, rng=rng, scale=M * 0.5 * 0.64 * D)
    st = mo.MPSState(N, D, L, M, cores)
    mo.calibrate(st, X.astype(np.float64))
    cores32 = [c.astype(np.float32) for c in st.cores]
    st = mo.MPSState(N, D, L, M, [c.astype(np.float64) for c in cores32])
    kw = dict(lr=1e-2, weight_dec=1e-3, L2_flag=True, act_fn='softmax', loss_fn='full_cross_ent', T=0.1, trunc=policy)
    ctxs = []
    for persistent in (1, 0, 2):             # one kernel per sweep (default), one launch per step, one kernel per role
        ctx = make_ctx(N, D, L, M, cores32, 0, X, y)
        ctx.set_persistent(persistent)
        ctx.profile_reset()
        ctxs.append(ctx)
    X64 = X.astype(np.float64)
    worst = {}
    for sw in range(2):
        if sw == 1:
            # Sweep 2 starts from ONE state everywhere (the persistent context's cores after sweep 1, float32 -> float64 for
            # the oracle): these untrained chains amplify float32 rounding -- free-running second sweeps of the three device
            # forms differed from the oracle by 2e-3 .. 8e-3 depending on nothing but the association order of the forward
            # chain -- so each sweep is compared on its own.
            cores_d, bond_d, lp = ctxs[0].get_cores()
            st = mo.MPSState(N, D, L, M, [c.astype(np.float64) for c in cores_d], l_pos=int(lp))
            assert list(st.bond) == [int(v) for v in bond_d]
            for ctx in ctxs[1:]:
                ctx.set_cores(cores_d, int(lp))
        f_o = mo.forward(st, X64)
        left_dir = st.l_pos == N - 1
        o = si.oracle_sweep(st, X64, y, f_o, kw['lr'], kw['weight_dec'], L2_flag=True, left_dir=left_dir,
                            act_fn=kw['act_fn'], loss_fn=kw['loss_fn'], T=kw['T'], trunc=policy)
        f_o, vh = o['f'], (o['accuracy'], o['MAE'])
        res = []
        for ctx in ctxs:
            ctx.forward()
            met, f_d = ctx.sweep(left_dir, N - 1, True, kw['lr'], kw['weight_dec'], True, kw['act_fn'], kw['loss_fn'], kw['T'], policy)
            res.append((met, f_d))
            worst['f_vs_oracle%d' % sw] = max(worst.get('f_vs_oracle%d' % sw, 0), relerr(f_d, f_o))
            worst['acc'] = max(worst.get('acc', 0), np.abs(met[:, 0] - np.array(vh[0])).max() * b)
            worst['mae'] = max(worst.get('mae', 0), np.abs(met[:, 1] - np.array(vh[1])).max())
            cores_d, bond_d, lp = ctx.get_cores()
            assert list(bond_d) == list(st.bond) and lp == st.l_pos
            # every step's kept singular values: the Gram diagonal of the core it left behind (tests/sweep_invariants.py)
            diag, _ = si.step_sigmas(cores_d, bond_d, left_dir)
            worst['sigma%d' % sw] = max(worst.get('sigma%d' % sw, 0), si.sigma_errors(diag, o['S']).max())
        # the two device paths: the same sums in another association order
        worst['f_paths%d' % sw] = relerr(res[0][1], res[1][1])
        assert np.abs(res[0][0][:, 0] - res[1][0][:, 0]).max() <= 1.0 / b + 1e-6
        assert np.abs(res[0][0][:, 1] - res[1][0][:, 1]).max() < 2e-4
        np.testing.assert_array_equal(res[0][1], res[2][1])       # the same arithmetic in one kernel or three
        np.testing.assert_array_equal(res[0][0], res[2][0])
    print('persistent sweep', policy, M, N, b, L, {k: '%.2e' % v for k, v in worst.items()})
    # The first sweep of a fresh network does not amplify rounding; the second does even from a common start (bond 20, N = 48:
    # device vs oracle 1.5e-2, the two device forms 4.9e-3 apart after its 47 steps -- test_float32_rounding_is_amplified_by_
    # the_sweep_dynamics measures the same on the oracle alone), so there f is only bounded and the per-step metrics carry the
    # comparison: accuracy of every step within one sample, MAE within 2.5e-6.
    assert worst['f_vs_oracle0'] < 1e-5 and worst['f_paths0'] < 1e-5      # observed <= 1e-6 / 9e-7 over the five cases
    assert worst['f_vs_oracle1'] < 4.5e-2 and worst['f_paths1'] < 1.4e-2     # observed 1.54e-2 / 4.89e-3 (bond 20, N = 48)
    # every step's kept singular values (Gram diagonal of its behind core): observed <= 7.8e-7 of sigma_max in sweep 1, 2.2e-3
    # in sweep 2 (bond 20, N = 48; 1.2e-3 at bond 8, N = 33)
    assert worst['sigma0'] < 5e-6 and worst['sigma1'] < 1e-2
    assert worst['acc'] <= 1.0 + 1e-3       # samples
    assert worst['mae'] < 3e-5
    # the persistent context made one launch per sweep, the other one N - 1 (+ the launch that starts a sweep)
    assert ctxs[0].counters()['launches'] == 2 and ctxs[0].counters()['sweep_steps'] == 2 * (N - 1) and ctxs[2].counters()['launches'] == 2
    assert ctxs[1].counters()['launches'] >= 2 * (N - 1)
    p2 = rng.random((b, N))
    X2 = np.stack([np.sin(np.pi * p2 / 2), np.cos(np.pi * p2 / 2)], -1).astype(np.float32)
    for ctx in ctxs:                                  # the network function on fresh input, each context against its own cores
        cores_d, _, lp = ctx.get_cores()
        f2 = mo.forward(mo.MPSState(N, D, L, M, [c.astype(np.float64) for c in cores_d], l_pos=int(lp)), X2.astype(np.float64))
        ctx.set_input(X2, y)
        assert relerr(ctx.forward(), f2) < 2e-5       # observed <= 2e-6
        ctx.close()
