"""The step-level views of tests/sweep_invariants.py on float64 oracle trajectories (no GPU).

The GPU tests of the timed paths (tests/test_timed_paths_gpu.py) read every step's singular values and behind
environments out of what one launch leaves behind.  These tests hold the helpers themselves: the identity
Gram(behind core) = diag(S[:m]) holds on the oracle, the helpers do not see the freedom an SVD leaves, and they do see
a wrong core -- at the site where it is wrong.
"""
import numpy as np
import pytest

import sweep_invariants as si
from oracle import mps_oracle as mo

# (policy, N, M, L): both policies, L in {2, 3, 10}; the reference policy keeps m = nS at the first and last steps and
# raises at the last right step for L > 2 (Network_class.py:914), so it runs with two labels
CASES = [('fixed', 9, 6, 2), ('fixed', 8, 5, 3), ('fixed', 7, 12, 10), ('reference', 9, 6, 2), ('reference', 6, 3, 2)]


def trajectory(policy, N, M, L, seed=0, b=40):
    """A calibrated random start, then one right and one left sweep of the oracle, each recorded."""
    rng = np.random.default_rng(seed)
    D = 2
    p = rng.random((b, N)) * (rng.random((b, N)) > 0.6)
    X = np.stack([np.sin(np.pi * p / 2), np.cos(np.pi * p / 2)], -1)
    y = rng.integers(0, L, b)
    st = mo.MPSState(N, D, L, M, mo.random_cores(N, M, D, L, rng=rng, scale=M * 0.5 * 0.64 * D))
    mo.calibrate(st, X)
    kw = dict(L2_flag=True, act_fn='softmax', loss_fn='full_cross_ent', T=0.1, trunc=policy)
    out = []
    for left in (False, True):
        f = mo.forward(st, X)
        rec = si.oracle_sweep(st, X, y, f, 1e-2, 1e-3, left_dir=left, **kw)
        out.append((left, [c.copy() for c in st.cores], list(st.bond), rec))
    return X, out


@pytest.fixture(scope='module', params=CASES, ids=['%s-N%d-M%d-L%d' % c for c in CASES])
def traj(request):
    return request.param, trajectory(*request.param)


def test_gram_of_behind_cores_is_diag_S(traj):
    (policy, N, M, L), (X, sweeps) = traj
    edge = 0
    for left, cores, bond, rec in sweeps:
        diag, off = si.step_sigmas(cores, bond, left)
        err = si.sigma_errors(diag, rec['S'])
        assert err.max() <= 1e-12, (left, err.max())
        assert off.max() <= 1e-12, (left, off.max())
        # the first and last steps are where m = nS (the whole spectrum is kept)
        for k in (0, N - 2):
            p, _ = si.behind_site(N, k, left)
            ml, mr = (1 if p == 0 else bond[p - 1]), (1 if p + 1 == N - 1 else bond[p + 1])
            nS = min(2 * ml, 2 * mr * L) if not left else min(2 * ml * L, 2 * mr)
            edge += len(diag[k]) == nS
        # the environments the sweep grew are the contraction of the cores it left
        fresh = si.behind_envs(cores, X, left)
        assert sorted(fresh) == sorted(rec['env'])
        for site, E in rec['env'].items():
            assert si.env_residual(fresh[site], E) <= 1e-12
            assert np.abs(fresh[site] - E).max() <= 1e-12 * np.abs(E).max()
    assert edge >= 2


def gauge(cores, Qs):
    """cores[i] . Q_i and Q_i^T . cores[i + 1] on every bond i: the same network function."""
    out = [np.array(c) for c in cores]
    for i, Q in enumerate(Qs):
        out[i] = np.einsum('adk...,kj->adj...', out[i], Q)
        out[i + 1] = np.einsum('kj,k...->j...', Q, out[i + 1])
    return out


def random_orthogonal(m, rng):
    Q, R = np.linalg.qr(rng.standard_normal((m, m)))
    return Q * np.sign(np.diag(R))[None, :]


def test_helpers_do_not_see_the_gauge(traj):
    (policy, N, M, L), (X, sweeps) = traj
    rng = np.random.default_rng(7)
    for left, cores, bond, rec in sweeps:
        f0 = mo.forward(mo.MPSState(N, 2, L, M, cores, l_pos=0 if left else N - 1), X)
        # a sign per singular pair on every bond: the freedom of the SVD itself
        signs = [np.diag(rng.choice([-1.0, 1.0], size=m)) for m in bond]
        gc = gauge(cores, signs)
        assert np.abs(mo.forward(mo.MPSState(N, 2, L, M, gc, l_pos=0 if left else N - 1), X) - f0).max() <= 1e-12 * np.abs(f0).max()
        diag, off = si.step_sigmas(gc, bond, left)
        assert si.sigma_errors(diag, rec['S']).max() <= 1e-12 and off.max() <= 1e-12
        envs = si.behind_envs(gc, X, left)
        assert max(si.env_residual(envs[s], rec['env'][s]) for s in rec['env']) <= 1e-12
        # an arbitrary orthogonal gauge on every bond: the environments still align; the Gram matrices are no longer
        # diagonal, and the off-diagonal check says so on every step whose bond has more than one column
        Qs = [random_orthogonal(m, rng) for m in bond]
        gc = gauge(cores, Qs)
        envs = si.behind_envs(gc, X, left)
        assert max(si.env_residual(envs[s], rec['env'][s]) for s in rec['env']) <= 1e-12
        _, off = si.step_sigmas(gc, bond, left)
        for k in range(N - 1):
            p, _ = si.behind_site(N, k, left)
            if bond[p] > 1:
                assert off[k] > 1e-6, (k, off[k])


def test_rotation_inside_a_degenerate_cluster_is_invisible():
    """A rotation that mixes singular vectors of equal singular values is the other freedom of an SVD: the Gram matrix
    of a core U . diag(sqrt(S)) with S = (4, 2, 2, 1) does not change under it."""
    rng = np.random.default_rng(3)
    S = np.array([4.0, 2.0, 2.0, 1.0])
    U = random_orthogonal(6, rng)[:, :4]                      # (D * ml, m) with D = 2, ml = 3
    A = (U * np.sqrt(S)[None, :]).reshape(2, 3, 4).transpose(1, 0, 2)
    B = rng.standard_normal((4, 2, 1))
    R = np.eye(4)
    R[1:3, 1:3] = random_orthogonal(2, rng)
    for cores in ([A, B], gauge([A, B], [R])):
        diag, off = si.step_sigmas(cores, [4], False)
        assert np.abs(diag[0] - S).max() <= 1e-12 * S[0] and off[0] <= 1e-12


@pytest.mark.parametrize('left', [False, True])
def test_a_perturbed_core_is_named(traj, left):
    """A 1e-4 relative perturbation of one behind core shows up at that step alone (singular values, off-diagonal), and
    the first environment it reaches is the one of its site."""
    (policy, N, M, L), (X, sweeps) = traj
    _, cores, bond, rec = sweeps[int(left)]
    rng = np.random.default_rng(11)
    for k in range(N - 1):
        p, site = si.behind_site(N, k, left)
        bad = [c.copy() for c in cores]
        bad[site] = bad[site] * (1 + 1e-4 * rng.standard_normal(bad[site].shape))
        diag, off = si.step_sigmas(bad, bond, left)
        err = si.sigma_errors(diag, rec['S'])
        flagged = set(np.nonzero(np.maximum(err, off) > 1e-8)[0])
        assert flagged == {k}, (k, err, off)
        envs = si.behind_envs(bad, X, left)
        res = {s: si.env_residual(envs[s], rec['env'][s]) for s in rec['env']}
        wrong = [s for s in res if res[s] > 1e-8]
        if site in rec['env']:
            # sweep order: the right sweep grows Lenv upwards, the left sweep Renv downwards
            first = min(wrong) if not left else max(wrong)
            assert first == site, (site, res)
        else:
            assert not wrong, (site, res)


@pytest.mark.parametrize('left', [False, True])
def test_swapped_column_scales_are_detected(traj, left):
    """The behind core of a step with the scales of its largest and smallest kept singular pair swapped is still
    orthogonal with the right set of singular values: only the diagonal in step order, and the environments, see it."""
    (policy, N, M, L), (X, sweeps) = traj
    _, cores, bond, rec = sweeps[int(left)]
    seen = 0
    for k in range(N - 1):
        p, site = si.behind_site(N, k, left)
        S = rec['S'][k]
        if len(S) < 2 or S[0] - S[-1] < 1e-3 * S[0]:
            continue
        bad = [c.copy() for c in cores]
        j0, j1 = 0, len(S) - 1
        r = np.sqrt(S[j1] / S[j0])
        if not left:
            bad[site][:, :, j0] *= r
            bad[site][:, :, j1] /= r
        else:
            bad[site][j0] *= r
            bad[site][j1] /= r
        diag, off = si.step_sigmas(bad, bond, left)
        err = si.sigma_errors(diag, rec['S'])
        assert off[k] <= 1e-12 and np.sort(diag[k])[::-1] == pytest.approx(S, rel=1e-12)
        assert err[k] > 0.5 * (S[0] - S[-1]) / S[0]
        if site in rec['env']:
            envs = si.behind_envs(bad, X, left)
            assert si.env_residual(envs[site], rec['env'][site]) > 1e-6
        seen += 1
    assert seen >= 1
