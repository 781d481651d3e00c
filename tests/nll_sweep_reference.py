"""The two-site likelihood sweep in float64 NumPy (test infrastructure): the statement of tnml_nll_sweep in
include/tnml.h on top of nll_reference.py, with the shared cases of tests/test_nll_sweep_host.py (which checks the conditions on them
with this reference alone) and tests/test_nll_sweep_gpu.py (which runs them on the device), and the tables the GPU bounds are read from.

The label sits on site l; a right step works on sites (p, p+1) with p = l, a left step on p = l - 1.  B[a,d,e,c,l'] is the product of
the two cores, P[s,a] / Q[s,c] the per-sample chains over the sites < p / > p+1, Lm = L_p and Rm = R_{p+2} the metric environments.

    f[l',s] = sum P x_p x_{p+1} Q B            cot as nll_reference.cotangent            Gd = sum_s cot P x_p x_{p+1} Q
    T = Lm (S (x) S) B Rm,  Z = <B, T>,  Gz = 2 T / Z,  log Z = log|Z| + the environments' logs
    B' = B + lr (Gd - Gz);  renorm: B' <- B' sqrt(sum B^2 / sum B'^2)
    split: U sqrt(S) behind, sqrt(S) Vh ahead with the label; m = min(max_bond, short side), under threshold < 1 also the fewest
    singular values whose share of sum(S) exceeds it

emulate=True follows the device's roundings: float32 chains, f, cotangent and Gd, the merged tensor rounded to float32 for f, B' rounded
to float32 where the split takes it, the new cores stored as float32; T, Z, Gz, the update and the SVD in float64.
"""
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p_ in (ROOT, HERE):
    if p_ not in sys.path:
        sys.path.insert(0, p_)

import nll_reference as NR                                                                  # noqa: E402
from nll_reference import round_up_one_digit                                                # noqa: E402,F401
from sample_reference import grid, gram                                                     # noqa: E402

BAD_BATCH, NOT_APPLIED = 8, 16


def merged(cores, l, left):
    """(p, B (ml, D, D, mr, L) float64) of the step at label site l"""
    p = l - 1 if left else l
    a, b = np.asarray(cores[p], dtype=np.float64), np.asarray(cores[p + 1], dtype=np.float64)
    B = np.einsum('adk,kecl->adecl', a, b) if left else np.einsum('adkl,kec->adecl', a, b)
    return p, B


def chains(cores, p, X, dt):
    """(P (b, ml), Q (b, mr)) over the sites < p and > p + 1 in dtype dt"""
    N, b = len(cores), X.shape[0]
    P = np.ones((b, 1), dtype=dt)
    for i in range(p):
        P = np.einsum('ba,bd,adc->bc', P, X[:, i], cores[i].astype(dt))
    Q = np.ones((b, 1), dtype=dt)
    for i in range(N - 1, p + 1, -1):
        Q = np.einsum('adc,bd,bc->ba', cores[i].astype(dt), X[:, i], Q)
    return P, Q


def step_gradient(cores, l, X, y, S, left, emulate=False):
    """dict(p, B, Gd, Gz, value, logz, nbad, f): the two-site gradient and the value of the batch before the step"""
    dt = np.float32 if emulate else np.float64
    c64 = [np.asarray(c, dtype=np.float64) for c in cores]
    D = c64[0].shape[1]
    p, B = merged(c64, l, left)
    Xd = np.asarray(X, dtype=dt)
    P, Q = chains(c64, p, Xd, dt)
    f = np.einsum('sa,sd,se,sc,adecl->ls', P, Xd[:, p], Xd[:, p + 1], Q, B.astype(dt))
    with np.errstate(divide='ignore', invalid='ignore'):
        cot, terms = NR.cotangent(f, y)
    badcol = ~(np.isfinite(cot).all(axis=0) & np.isfinite(terms))
    cot = np.where(badcol[None, :], 0, cot).astype(dt)
    Gd = np.einsum('ls,sa,sd,se,sc->adecl', cot, P, Xd[:, p], Xd[:, p + 1], Q).astype(np.float64)
    Ls, lgL, Rs, lgR = NR.environments(c64, l, S)
    Sm = np.eye(D) if S is None else np.asarray(S, dtype=np.float64)
    T = np.einsum('ab,dD,eE,bDECl,Cc->adecl', Ls[p], Sm, Sm, B, Rs[p + 2], optimize=True)
    Z = float((B * T).sum())
    logz = math.log(abs(Z)) + lgL[p] + lgR[p + 2]
    return dict(p=p, B=B, Gd=Gd, Gz=2.0 * T / Z, value=float(-(terms.mean() - logz)), logz=logz, nbad=int(badcol.sum()), f=f)


def kept_rank(S, cap, threshold):
    m = min(cap, len(S))
    if threshold < 1.0:
        m = min(m, int(np.argmax(np.cumsum(S) / S.sum() > threshold)) + 1)
    return m


def split(Bn, left, max_bond, threshold=1.0, sigma=None):
    """(core of site p, core of site p + 1, S, m): tensor_svd's split of the merged tensor with the label on the core ahead;
    sigma: decide the rank on these singular values (the device's own) instead of the split's"""
    ml, D, _, mr, L = Bn.shape
    M = np.transpose(Bn, (2, 3, 0, 1, 4)).reshape(D * mr, ml * D * L) if left else Bn.reshape(ml * D, D * mr * L)
    U, Sv, Vh = np.linalg.svd(M, full_matrices=False)
    m = kept_rank(Sv if sigma is None else np.asarray(sigma), min(max_bond, len(Sv)), threshold)
    r = np.sqrt(Sv[:m])
    US, SV = U[:, :m] * r, r[:, None] * Vh[:m]
    if left:
        return np.transpose(SV.reshape(m, ml, D, L), (1, 2, 0, 3)), US.T.reshape(m, D, mr), Sv, m
    return US.reshape(ml, D, m), SV.reshape(m, D, mr, L), Sv, m


def discarded_weight(S, m):
    return float((S[m:] ** 2).sum() / (S ** 2).sum())


def step(cores, l, X, y, S, left, lr, renorm=True, max_bond=16, threshold=1.0, emulate=False, skip=False):
    """one step: (new cores, new l, record) with record = dict(values (6,), B, Gd, Gz, B_new, sigma, f, skip)"""
    g = step_gradient(cores, l, X, y, S, left, emulate)
    lr = float(np.float32(lr))
    B = g['B']
    Bn = B + lr * (g['Gd'] - g['Gz'])
    if renorm:
        q1 = float((Bn ** 2).sum())
        if q1 > 0 and math.isfinite(q1):
            Bn = Bn * math.sqrt(float((B ** 2).sum()) / q1)
    bits = BAD_BATCH if g['nbad'] else 0
    skip = skip or bits != 0
    if skip:
        bits |= NOT_APPLIED
        Bn = B
    if emulate:
        Bn = Bn.astype(np.float32).astype(np.float64)
    a, b, Sv, m = split(Bn, left, max_bond, threshold)
    if emulate:
        a, b = a.astype(np.float32).astype(np.float64), b.astype(np.float32).astype(np.float64)
    new = [np.asarray(c, dtype=np.float64) for c in cores]
    p = g['p']
    new[p], new[p + 1] = a, b
    vals = np.array([g['value'], g['logz'], g['nbad'], bits, m, discarded_weight(Sv, m)])
    return new, (l - 1 if left else l + 1), dict(values=vals, B=B, Gd=g['Gd'], Gz=g['Gz'], B_new=Bn, sigma=Sv, f=g['f'], skip=skip)


def sweep(cores, l, X, y, S, left, n_steps, lr, renorm=True, max_bond=16, threshold=1.0, emulate=False):
    """n_steps steps: (cores, l, values (n_steps, 6))"""
    vals, skip = [], False
    for _ in range(n_steps):
        cores, l, rec = step(cores, l, X, y, S, left, lr, renorm, max_bond, threshold, emulate, skip)
        skip = rec['skip']
        vals.append(rec['values'])
    return cores, l, np.array(vals)


def plan(N, l):
    """[(left, n_steps)] of a whole right + left pass from l: to the far end first, then back over the whole chain"""
    if l == N - 1:
        return [(True, N - 1), (False, N - 1)]
    return [(False, N - 1 - l), (True, N - 1)]


def there_and_back(cores, l, X, y, S, lr, renorm=True, max_bond=16, threshold=1.0, emulate=False):
    """(cores, l, values of every step in order) of plan(N, l)"""
    out = []
    for left, n in plan(len(cores), l):
        cores, l, v = sweep(cores, l, X, y, S, left, n, lr, renorm, max_bond, threshold, emulate)
        out.append(v)
    return cores, l, np.concatenate(out)


# ---------------------------------------------------------------------------------------------------------------
# shared cases
# ---------------------------------------------------------------------------------------------------------------
D, CAP, MAX_BOND, K, LR = 2, 4, 16, 16, 0.01
# (N, L, l, b, labelled, renorm): N = 6 and 9, L = 2 and 3, the label at both ends and inside, b on either side of the 64-sample tile
CASES = [
    (6, 2, 0, 70, True, True), (6, 2, 5, 70, False, True), (6, 3, 2, 17, True, False), (6, 3, 0, 1, False, True),
    (9, 2, 4, 70, True, True), (9, 2, 0, 70, False, True), (9, 3, 8, 17, True, True), (9, 2, 8, 70, True, False),
]
# the descent cases: those of the prototype (L = 2, b = 70, renorm), where every step of the pass lowers the value
DESCENT = [c for c in CASES if c[1] == 2 and c[3] == 70 and c[5]]
# the lr = 0 cases: those whose pass never truncates at MAX_BOND (tests/test_nll_sweep_host.py asserts a discarded weight of 0 and the
# identity in float64); N9_L3_l8 is not one of them, two of its splits discard weight
LR0 = [CASES[0], CASES[2], CASES[4]]
MIN_RATIO = NR.MIN_RATIO
SEED = {}


def case_id(case):
    return 'N%d_L%d_l%d_b%d_%s_%s' % (case[0], case[1], case[2], case[3], 'joint' if case[4] else 'marginal', 'renorm' if case[5] else 'plain')


def grid_metric():
    _, phi, w = grid(K, D)
    return phi, w, gram(phi, w)


def build_case(case):
    """(cores float32-rounded float64, l, X float32 (b, N, D), labels int32 (b,), y (labels or None), S)"""
    N, L, l, b, labelled, renorm = case
    rng = np.random.default_rng([30, N, L, l, b, SEED.get(case_id(case), 0)])
    bond = NR.chain_bonds(N, CAP, rng)
    phi, w, S = grid_metric()
    Xc = NR.oref.features(rng, NR.oref.B, N, D)
    cores = NR.make_cores(N, D, L, bond, l, rng, Xc)
    lev, lab, _, _ = NR.walk(cores, l, phi, w, np.full(b, -1), rng.random((b, N + 1)))
    lab = lab.astype(np.int32)
    return cores, l, phi[lev].astype(np.float32), lab, (lab if labelled else None), S


def label_ratio(cores, l, X, y):
    f = NR.forward([np.asarray(c, dtype=np.float64) for c in cores], l, X.astype(np.float64))
    num = np.abs(f[y, np.arange(len(y))]).min() if y is not None else np.sqrt((f ** 2).sum(axis=0)).min()
    return float(num / np.abs(f).max())


def big_case():
    """the large-tensor SVD path: N = 4, bond 40, L = 2, b = 70, label at 1: the merged matrix of the first right step is 80 x 160"""
    N, L, l, b = 4, 2, 1, 70
    rng = np.random.default_rng([30, 40])
    phi, w, S = grid_metric()
    Xc = NR.oref.features(rng, NR.oref.B, N, D)
    cores = NR.make_cores(N, D, L, [40, 40, 40], l, rng, Xc)
    lev, lab, _, _ = NR.walk(cores, l, phi, w, np.full(b, -1), rng.random((b, N + 1)))
    return cores, l, phi[lev].astype(np.float32), lab.astype(np.int32), S


def emulation_figures(case):
    """(value, log Z, max|f|, discarded weight) deviations of the emulation from float64 over the pass of plan(): values and log Z of
    max(1, |.|), f after the pass of max|f|, the discarded weight (a share of 1) as it is"""
    cores, l, X, lab, y, S = build_case(case)
    c64, l64, v64 = there_and_back(cores, l, X, y, S, LR, case[5], MAX_BOND)
    c32, l32, v32 = there_and_back(cores, l, X, y, S, LR, case[5], MAX_BOND, emulate=True)
    f64, f32 = NR.forward(c64, l64, X.astype(np.float64)), NR.forward(c32, l32, X.astype(np.float64))
    dv = float((np.abs(v32[:, 0] - v64[:, 0]) / np.maximum(1.0, np.abs(v64[:, 0]))).max())
    dz = float((np.abs(v32[:, 1] - v64[:, 1]) / np.maximum(1.0, np.abs(v64[:, 1]))).max())
    return dv, dz, float(np.abs(f32 - f64).max() / np.abs(f64).max()), float(np.abs(v32[:, 5] - v64[:, 5]).max())


def single_step_figures(case):
    """(Gd, Gz, B_new) deviations of the emulation's first step from float64, each of max|.| of the float64 array"""
    cores, l, X, lab, y, S = build_case(case)
    left = plan(case[0], l)[0][0]
    _, _, r64 = step(cores, l, X, y, S, left, LR, case[5], MAX_BOND)
    _, _, r32 = step(cores, l, X, y, S, left, LR, case[5], MAX_BOND, emulate=True)
    return tuple(float(np.abs(r32[k] - r64[k]).max() / np.abs(r64[k]).max()) for k in ('Gd', 'Gz', 'B_new'))


# The worst deviation of the float32 emulation from float64 over CASES: (value, log Z, f after the pass) and (Gd, Gz, B_new) of the
# first step.  tests/test_nll_sweep_host.py asserts that the code still gives figures no larger than these (and no smaller than a
# quarter: einsum's summation order follows the host's vector width); the bounds of tests/test_nll_sweep_gpu.py are read from here.
EMULATION = dict(value=4.570e-07, logz=2.094e-07, f=2.761e-06, discarded=3.506e-07, Gd=1.549e-07, B_new=4.355e-08)


def gpu_bound(name):
    """ten times the emulation's worst figure, rounded up to one digit: the margin of nll_reference.gpu_bounds, for the summation
    order (MFMA k-steps of four on the device, einsum in the emulation) and, for f, the Jacobi SVD against LAPACK"""
    return round_up_one_digit(10.0 * EMULATION[name])
