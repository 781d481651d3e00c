"""The forward environment chain at D = 2, kernel variant by kernel variant (csrc/kernels_wide.hip, launch_env_chain), and the bond
capacity rule of tnml_set_cores (include/tnml.h).

launch_env_chain picks its kernel from the context's CAPACITY, not from the bonds in use:
    cap = max(M, D * min(L, M))          (the enlargement tnml_create applies to the M it is given)
    mo  = max(cap, L)
    cap even and mo <= 32:   env_chain_roles_kernel<NV4, NT, NKS>   mo <= 10 (1,1,5) | <= 16 (2,1,8) | <= 20 (4,2,10) | <= 24 (5,2,12) | else (8,2,16)
    otherwise, or tnml_set_chain_path(1):   env_chain_kernel<false>   ("plain")
    calibration (tnml_forward_logabsmax):   env_chain_kernel<true>
`variant()` below restates that ladder; every case asserts the variant it means to enter, so a changed ladder fails an expectation
instead of silently moving a test to another kernel.

  1  every variant, every environment   13 (M, L) rows at both edges of every rung x chain lengths 2, 3, 4, 5, 9, 17 (below, at and
                                        above the loader count 3, the ring 4 and one / two / three warming blocks of 8; both parities
                                        of the two-site unrolled loop); label at both ends, and -- any_position on -- at 1, N // 2,
                                        N - 2; uniform bonds at the capacity and a ragged set (one bond at the capacity, one odd bond
                                        just below it, a bond of 1 inside the chain); b = 1, 17, 70 on a context of capacity 70; through
                                        the variant and through the plain kernel.  Every environment get_env returns and f against
                                        float64; predict(X) bit-equal to forward's f and the resident f / environments bit-unchanged
  2  a reused context                   bonds 20 at b = 70, then ragged smaller bonds at b = 17, then back: nothing stale is read
  3  label_meet_kernel, two label passes   L = 17 inside the chain (rows M 4 L 17 of 1, and M 20 L 17 here)
  4  calibration and f_absmax           f_absmax() is max|f| of the returned f exactly; forward_logabsmax() against the float64 log max|f|
                                        of a chain whose f (1e-60) lies below float32's range
  5  bonds above the capacity           tnml_set_cores refuses them and the context keeps what it had

The float64 expectation is test_any_position_host.label_inside_forward (plain NumPy on the oracle's site_matrix) on the cores
rounded to float32, which both sides receive.

Tolerance: forward f and environments 2e-5 of max|.|, the forward tolerance in the header of tests/test_hip_parity.py.  Behind it:
a float32 NumPy run of label_inside_forward against its float64 run, on exactly the cases of this file (core scale
0.5 * max(bond)), stays below 3.5e-7 on every environment and below 1.5e-6 on f; 2e-5 leaves the device more than an order of
magnitude for its summation order and still fails on one wrong operand.  log max|f|: 1e-4 * max(1, |value|), as
test_feature_dim_gpu.py::test_calibration_logabsmax_N784 -- at a value of -138 that is 1.4e-2, i.e. 1.4 % of f: the calibration test
pins the renormalisation, the padding samples and the range, and would NOT catch a small arithmetic error in env_chain_kernel<true>.
Every test prints the worst values it observed.

Environments compared per (M, L) row and kernel (the variant, and again the plain kernel): 12, 36, 72, 120, 240, 480 at
N = 2, 3, 4, 5, 9, 17 -- 960 per row and kernel; 240 on the reused context, 24 with two label passes.  Each case prints, behind its
own figures, the worst errors and the count of its kernel over the run so far: the last such line per kernel is the table below.
Observed on MI355X (worst environment / worst f / environments compared):
  (1,1,5)    M 10 L 3                             2.4e-07 / 5.1e-07 /   960
  (2,1,8)    M 12, 16 L 2                         2.4e-07 / 8.0e-07 /  1920
  (4,2,10)   M 18, 20 L 2; M 12 L 10; M 4 L 17    4.0e-07 / 1.2e-06 /  3840
  (5,2,12)   M 22 L 2; M 24 L 10                  4.1e-07 / 1.4e-06 /  1920
  (8,2,16)   M 26 L 2; M 32 L 10                  5.5e-07 / 2.2e-06 /  1920
  plain      M 9, 34 L 2, and all rows forced     3.8e-07 / 2.2e-06 / 14400
  reused context 3.4e-07 / 1.1e-06;  two label passes 1.8e-07 / 9.6e-07;  f_absmax exact beside f 1.7e-07;  log max|f| off by 2.3e-05
  at -138.5.
"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from test_any_position_host import label_inside_forward, random_cores_at    # noqa: E402
from tensornetworkforml_amd import _hip                          # noqa: E402
from tensornetworkforml_amd import data_generator as gen         # noqa: E402

pytestmark = pytest.mark.gpu

D = 2
TOL = 2e-5
B_CAP = 70
BATCHES = (1, 17, 70)      # one live lane; a second 16-sample workgroup with one live sample; across the 64 samples of a meet workgroup
S_L, S_R = _hip.SIDE_LEFT, _hip.SIDE_RIGHT


def relerr(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def features(rng, b, N):
    p = rng.random((b, N)) * (rng.random((b, N)) > 0.5)
    return gen.psi(p, D).astype(np.float32)


def capacity(M, L):
    return max(M, D * min(L, M))


def variant(cap, mo, force_plain=False):
    """launch_env_chain's ladder (csrc/kernels_wide.hip)."""
    if force_plain or mo > 32 or cap % 2:
        return 'plain'
    for top, name in ((10, (1, 1, 5)), (16, (2, 1, 8)), (20, (4, 2, 10)), (24, (5, 2, 12))):
        if mo <= top:
            return name
    return (8, 2, 16)


def ragged_bonds(N, cap, rng):
    """Bonds in [1, cap]: one at the capacity, one odd bond just below it (a last column tile of one column at cap 18), a bond of 1
    inside the chain -- as many of the three as the chain has room for."""
    nb = N - 1
    odd = cap - 1 if cap % 2 == 0 else cap - 2
    bond = rng.integers(1, cap + 1, nb)
    if nb == 1:
        bond[0] = odd
    elif nb == 2:
        bond[:] = rng.permutation([cap, odd])
    else:
        one = int(rng.integers(1, nb - 1))
        rest = rng.permutation([i for i in range(nb) if i != one])
        bond[one], bond[rest[0]], bond[rest[1]] = 1, cap, odd
    return [int(m) for m in bond]


def positions(N):
    """(l, any_position): both ends with the switch off; 1, N // 2, N - 2 with it on, where the chain has such sites."""
    inside = sorted({l for l in (1, N // 2, N - 2) if 0 < l < N - 1})
    return [(0, False), (N - 1, False)] + [(l, True) for l in inside]


def env_sites(N, l):
    return [(S_L, i) for i in range(l)] + [(S_R, i) for i in range(l + 1, N)]


def problem(N, L, bond, l, rng):
    cores32 = [a.astype(np.float32) for a in random_cores_at(N, D, L, bond, l, rng, scale=0.5 * max(bond))]
    return cores32, [a.astype(np.float64) for a in cores32]


def check_forward(ctx, N, l, X, b, expect, worst):
    """One forward of the resident cores on X[:b] against the float64 expectation of the whole X; then predict.  Returns the number
    of environments compared."""
    Lenv, Renv, f_o = expect
    ctx.set_input(X[:b])
    f_d = ctx.forward()
    worst['f'] = max(worst['f'], relerr(f_d, f_o[:, :b]))
    envs = []
    for side, i in env_sites(N, l):
        e = ctx.get_env(side, i)
        worst['env'] = max(worst['env'], relerr(e, (Lenv if side == S_L else Renv)[i][:b]))
        envs.append(e)
    # include/tnml.h: predict gives forward's f for the same samples and leaves the resident batch, f and environments alone
    f_p = ctx.predict(X[:b])
    assert np.array_equal(f_p.view(np.uint32), f_d.view(np.uint32)), ('predict', l, b)
    assert np.array_equal(ctx.get_f().view(np.uint32), f_d.view(np.uint32)), ('resident f', l, b)
    for (side, i), e in zip(env_sites(N, l), envs):
        assert np.array_equal(ctx.get_env(side, i).view(np.uint32), e.view(np.uint32)), ('resident environment', l, b, side, i)
    return len(envs)


# ---------------------------------------------------------------------------------------------------------------
# 1. every variant, every environment
# ---------------------------------------------------------------------------------------------------------------
#        M   L  cap  mo  kernel
ROWS = [(10, 3, 10, 10, (1, 1, 5)),       # all five k-steps used
        (12, 2, 12, 12, (2, 1, 8)),       # lower edge of its range
        (16, 2, 16, 16, (2, 1, 8)),       # full 16-column tile, eight k-steps
        (18, 2, 18, 18, (4, 2, 10)),      # bond 17 or 18: the second tile holds one or two columns
        (20, 2, 20, 20, (4, 2, 10)),      # headline bond
        (12, 10, 20, 20, (4, 2, 10)),     # capacity raised by L, not by M
        (4, 17, 8, 17, (4, 2, 10)),       # mo set by L; the label site has n_out = 17
        (22, 2, 22, 22, (5, 2, 12)),      # lower edge of its range
        (24, 10, 24, 24, (5, 2, 12)),     # upper edge of its range
        (26, 2, 26, 26, (8, 2, 16)),      # lower edge of its range
        (32, 10, 32, 32, (8, 2, 16)),     # every tile and k-step full
        (9, 2, 9, 9, 'plain'),            # odd capacity
        (34, 2, 34, 34, 'plain')]         # above 32
LENGTHS = (2, 3, 4, 5, 9, 17)
PER_VARIANT = {}                          # kernel name -> worst errors and environments compared over the cases run so far (printed)


@pytest.mark.parametrize('N', LENGTHS)
@pytest.mark.parametrize('M,L,cap,mo,kernel', ROWS, ids=['M%d-L%d' % r[:2] for r in ROWS])
def test_every_variant_every_environment(M, L, cap, mo, kernel, N):
    assert (capacity(M, L), max(capacity(M, L), L)) == (cap, mo)
    assert variant(cap, mo) == kernel and variant(cap, mo, True) == 'plain'
    rng = np.random.default_rng(1000 * M + 10 * L + N)
    X = features(rng, B_CAP, N)
    X64 = X.astype(np.float64)
    bond_sets = [[cap] * (N - 1), ragged_bonds(N, cap, rng)]
    rag = bond_sets[1]
    assert all(1 <= m <= cap for m in rag) and any(m % 2 and m > 1 for m in rag)
    assert N < 3 or cap in rag
    assert N < 4 or 1 in rag[1:-1]
    pos = positions(N)
    assert len(pos) == {2: 2, 3: 3, 4: 4}.get(N, 5)
    ctx = _hip.Context(N, D, L, M, B_CAP)
    worst = {False: dict(f=0.0, env=0.0), True: dict(f=0.0, env=0.0)}
    compared = {False: 0, True: 0}
    for l, anypos in pos:
        ctx.set_any_position(anypos)
        for bond in bond_sets:
            cores32, cores64 = problem(N, L, bond, l, rng)
            expect = label_inside_forward(cores64, l, X64)              # once, for all 70 samples
            ctx.set_cores(cores32, l)
            for plain in (False, True):
                ctx.set_chain_path(plain)
                for b in BATCHES:
                    compared[plain] += check_forward(ctx, N, l, X, b, expect, worst[plain])
    ctx.close()
    for plain in (False, True):
        name = ('%s' % (variant(cap, mo, plain),)).replace(' ', '')
        tot = PER_VARIANT.setdefault(name, dict(env=0.0, f=0.0, n=0))
        tot.update(env=max(tot['env'], worst[plain]['env']), f=max(tot['f'], worst[plain]['f']), n=tot['n'] + compared[plain])
        # (the last line a run prints for a variant is its worst error and its count over the whole run)
        print('forward chain %s M %d L %d N %d: env %.2e f %.2e, %d environments; %s so far: env %.2e f %.2e, %d environments' % (
            name, M, L, N, worst[plain]['env'], worst[plain]['f'], compared[plain], name, tot['env'], tot['f'], tot['n']))
    # nothing was skipped inside the loops: N - 1 environments per forward
    assert compared[False] == compared[True] == len(pos) * len(bond_sets) * len(BATCHES) * (N - 1)
    for plain in (False, True):
        assert worst[plain]['f'] < TOL and worst[plain]['env'] < TOL, (plain, worst[plain])


# ---------------------------------------------------------------------------------------------------------------
# 2. state left behind on a reused context
# ---------------------------------------------------------------------------------------------------------------
def test_reused_context_reads_nothing_stale():
    """Wide bonds and a full batch, then narrower ragged bonds and a short batch on the same context, then back: rows of the ring
    slots, of the LDS tile and of the environment slots beyond the bonds in use, and the samples beyond b, hold the previous
    forward's values and must not be read."""
    M, L, N = 20, 2, 9
    cap = capacity(M, L)
    assert variant(cap, max(cap, L)) == (4, 2, 10)
    rng = np.random.default_rng(29)
    X = features(rng, B_CAP, N)
    X64 = X.astype(np.float64)
    wide, narrow = [cap] * (N - 1), [7, 20, 3, 1, 12, 5, 19, 2]
    ctx = _hip.Context(N, D, L, M, B_CAP)
    worst = dict(f=0.0, env=0.0)
    compared = 0
    for l, anypos in positions(N):
        ctx.set_any_position(anypos)
        for plain in (False, True):
            ctx.set_chain_path(plain)
            first = problem(N, L, wide, l, rng)
            for (cores32, cores64), b in ((first, 70), (problem(N, L, narrow, l, rng), 17), (first, 70)):
                ctx.set_cores(cores32, l)
                compared += check_forward(ctx, N, l, X, b, label_inside_forward(cores64, l, X64), worst)
    ctx.close()
    print('reused context', {k: '%.2e' % v for k, v in worst.items()}, '%d environments' % compared)
    assert compared == 5 * 2 * 3 * (N - 1)
    assert worst['f'] < TOL and worst['env'] < TOL


# ---------------------------------------------------------------------------------------------------------------
# 3. two label passes in label_meet_kernel
# ---------------------------------------------------------------------------------------------------------------
def test_label_meet_takes_two_label_passes():
    """label_meet_kernel takes labels 16 at a time: L = 17 is one full pass and a pass of one label."""
    M, L, N, l = 20, 17, 5, 2
    cap = capacity(M, L)
    assert cap == 34 and variant(cap, max(cap, L)) == 'plain'
    rng = np.random.default_rng(31)
    X = features(rng, B_CAP, N)
    X64 = X.astype(np.float64)
    ctx = _hip.Context(N, D, L, M, B_CAP)
    ctx.set_any_position(True)
    worst = dict(f=0.0, env=0.0)
    compared = 0
    for bond in ([M] * (N - 1), [17, cap, 9, 20]):
        cores32, cores64 = problem(N, L, bond, l, rng)
        expect = label_inside_forward(cores64, l, X64)
        assert expect[2].shape == (L, B_CAP)
        ctx.set_cores(cores32, l)
        for b in BATCHES:
            compared += check_forward(ctx, N, l, X, b, expect, worst)
    ctx.close()
    print('two label passes', {k: '%.2e' % v for k, v in worst.items()})
    assert compared == 2 * len(BATCHES) * (N - 1)
    assert worst['f'] < TOL and worst['env'] < TOL


# ---------------------------------------------------------------------------------------------------------------
# 4. calibration and f_absmax
# ---------------------------------------------------------------------------------------------------------------
def test_f_absmax_is_the_maximum_of_the_resident_f():
    M, L, N, b = 20, 3, 9, 17
    rng = np.random.default_rng(37)
    X = features(rng, b, N)
    ctx = _hip.Context(N, D, L, M, B_CAP)
    worst = 0.0
    for l in (0, N - 1):
        cores32, cores64 = problem(N, L, ragged_bonds(N, capacity(M, L), rng), l, rng)
        ctx.set_cores(cores32, l)
        ctx.set_input(X)
        f_d = ctx.forward()
        worst = max(worst, relerr(f_d, label_inside_forward(cores64, l, X.astype(np.float64))[2]))
        amax = ctx.f_absmax()
        assert amax == float(np.abs(f_d).max()), (l, amax, float(np.abs(f_d).max()))     # a maximum is exact in float32
    ctx.close()
    print('f_absmax: exact; f %.2e' % worst)
    assert worst < TOL


def test_calibration_logabsmax_below_float32_range():
    """forward_logabsmax renormalises every sample after every site (env_chain_kernel<true>): log max|f| of a chain whose f, 1e-60,
    float32 cannot hold; padding samples must not win the maximum."""
    M, L, N = 20, 2, 17
    rng = np.random.default_rng(41)
    X = features(rng, B_CAP, N)
    X64 = X.astype(np.float64)
    ctx = _hip.Context(N, D, L, M, B_CAP)
    worst = 0.0
    for l in (0, N - 1):
        cores = random_cores_at(N, D, L, [M] * (N - 1), l, rng, scale=0.5 * M)
        f0 = np.abs(label_inside_forward(cores, l, X64)[2]).max()
        g = (1e-60 / f0) ** (1.0 / N)                                    # the same factor on every core: f -> 1e-60
        cores32 = [(a * g).astype(np.float32) for a in cores]
        cores64 = [a.astype(np.float64) for a in cores32]
        ctx.set_cores(cores32, l)
        for b in (70, 17):
            f_o = label_inside_forward(cores64, l, X64[:b])[2]
            lm_o = float(np.log(np.abs(f_o).max()))
            assert np.isfinite(lm_o) and 0.0 < np.abs(f_o).max() < 1e-55        # far below float32's smallest subnormal (1.4e-45)
            ctx.set_input(X[:b])
            lm = ctx.forward_logabsmax()
            worst = max(worst, abs(lm - lm_o))
            assert abs(lm - lm_o) < 1e-4 * max(1.0, abs(lm_o)), (l, b, lm, lm_o)
    ctx.close()
    print('log max|f| of a 1e-60 chain: worst difference %.2e at %.1f' % (worst, lm_o))


# ---------------------------------------------------------------------------------------------------------------
# 5. bonds above the capacity
# ---------------------------------------------------------------------------------------------------------------
REFUSED = [(4, [16, 4, 4, 4], 0),       # the example: cores of 32 and 128 floats in slots of 128, away from the label site
           (0, [16, 4, 4, 4], 0),       # the wide bond next to the label site
           (0, [4, 16, 4, 4], 1),       # further along the chain: the message names other sites
           (4, [4, 4, 4, 16], 3)]       # next to the label site at the other end


@pytest.mark.parametrize('l_pos,wide,at', REFUSED, ids=['label %d bonds %s' % (r[0], '-'.join(map(str, r[1]))) for r in REFUSED])
def test_set_cores_refuses_a_bond_above_capacity(l_pos, wide, at):
    """Capacity 8 and one bond of 16: the cores on either side of the wide bond fit their slots (128 floats, 256 with the label axis),
    but the environment slots hold 8 rows.  The call itself is what is tested: no chain ever runs on the refused bonds."""
    N, L, M, b = 5, 2, 8, 17
    cap = capacity(M, L)
    assert cap == 8 and wide[at] == 16
    rng = np.random.default_rng(43)
    X = features(rng, b, N)
    good32, good64 = problem(N, L, [8, 3, 8, 5], l_pos, rng)
    wide32, _ = problem(N, L, wide, l_pos, rng)
    assert all(a.size <= cap * D * cap * (L if i == l_pos else 1) for i, a in enumerate(wide32))     # every core fits its slot
    ctx = _hip.Context(N, D, L, M, b)
    ctx.set_cores(good32, l_pos)
    ctx.set_input(X)
    _, _, f_o = label_inside_forward(good64, l_pos, X.astype(np.float64))
    f_before = ctx.forward()
    assert relerr(f_before, f_o) < TOL

    def kept():
        # the context keeps its previous cores, bonds and label position
        cores, bond, lp = ctx.get_cores()
        assert list(bond) == [8, 3, 8, 5] and lp == ctx.l_pos == l_pos
        assert all(np.array_equal(a.view(np.uint32), g.view(np.uint32)) for a, g in zip(cores, good32))

    with pytest.raises(_hip.TnmlError) as ei:
        ctx.set_cores(wide32, l_pos)
    assert ei.value.code == -1                                            # TNML_ERR_ARG
    msg = str(ei.value)
    assert 'bond 16' in msg and 'sites %d and %d' % (at, at + 1) in msg and 'capacity 8' in msg, msg
    kept()
    # the lower end of the rule: a bond of 0
    none = list(wide)
    none[at] = 0
    with pytest.raises(_hip.TnmlError) as ei:
        ctx.set_cores([np.zeros(shp, np.float32) for shp in _hip.core_shapes(none, l_pos, D, L)], l_pos)
    assert ei.value.code == -1
    kept()
    f_after = ctx.forward()
    ctx.close()
    assert relerr(f_after, f_o) < TOL and np.array_equal(f_after.view(np.uint32), f_before.view(np.uint32))
