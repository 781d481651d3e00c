"""The update rule that ends every sweep step, restated in float64, its mutants, and the cases at which each of its terms shows
(test helper, not a conftest; no GPU).

    L2_grad = 2 wd Nh^T.B.Ng   (L2_flag)    |    wd B   (L2_flag off)
    dB      = dB_raw - L2_grad
    dB_clip = dB / (sum|dB| / sum|B|)   if sum|dB| > sum|B|   else dB
    B_new   = B + lr dB_clip                                          (oracle/mps_oracle.py `sweep_step`, "clip + update")

`rule` is that text.  `mutants` gives, per recorded oracle step, the increment B_new - B a wrong rule would give, and how far it
lies from the true increment: `effect = max|inc_mutant - inc| / max|inc|`.  A GPU test that bounds the device's increment to a
twentieth of the smallest effect cannot pass a kernel that carries one of these mutants.

A mutant is evaluated in the steps where it is a different rule.  `fac_one` (no clipping) is the true rule in a step that is
not clipped, `fac_always` (the quotient applied whether or not sum|dB| > sum|B|) is the true rule in a clipped one, and
`nh_identity` is the true rule where the behind norm environment is the 1 x 1 matrix [[1]] (the first step of a sweep): there
the effect is None, not zero, and the minimum runs over the other steps -- all of them, none left out.
"""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import mps_oracle as mo

FLOOR = 2e-3            # smallest mutant effect every case must reach (tests/test_update_rule_host.py)
CLIP_MARGIN = 0.05      # no step has sum|dB| / sum|B| within this of 1

# Bounds of tests/test_update_rule_gpu.py.  Unless said otherwise each is 10 x the worst value observed on MI355X over all cases of the
# kernel (the observed value beside it; DESIGN.md, "The update rule under test").  They live here because
# tests/test_update_rule_host.py holds FLOOR and the persistent cases against them.
# Comparison 1, the increment B_new - B against rule() on the captured operands, relative to max|increment|.  The lds and large captures
# hold B_new as the float32 the kernel stores (half an ulp of B_new is ~5e-6 of an increment that is 1e-2 of B); anyd's holds the
# float64 value, and what is left there is lr = 0.01 passed as a float32 (2.2e-8).
INC_BOUND = dict(lds=5.1e-5,          # observed 5.10e-6
                 large=8.8e-5,        # observed 8.71e-6
                 anyd=2.3e-7)         # observed 2.24e-8 in every case
# Reasoned, not measured: the captured weight_dec B against wd B.  weight_dec reaches the kernel as a float32 (relative rounding at most
# 2^-24 = 6.0e-8), the product is one float64 multiplication.  Observed 3.97e-8 (wd = 0.3), 1.49e-8 (0.1), 0 (1).
WD_B_TOL = 1e-7
# Comparison 2, sweep 1 against the oracle's record after the sign gauge: relative to max|.| (tensors) or to the value (scalars)
OPERAND_BOUNDS = {
    'lds': dict(dB_raw=7.8e-5, L2_grad=8.8e-5, L2_loss=2.5e-6, B_measure=2.4e-5, dB_measure=2.4e-5, wdB=WD_B_TOL),
    #          observed 7.71e-6       8.79e-6         2.49e-7          2.33e-6            2.40e-6
    'large': dict(dB_raw=3.0e-5, L2_grad=2.0e-5, L2_loss=2.2e-6, B_measure=6.6e-6, dB_measure=1.6e-5, wdB=WD_B_TOL),
    #          observed 2.98e-6       1.95e-6         2.20e-7          6.53e-7            1.51e-6
    'anyd': dict(dB_raw=4.1e-5, L2_grad=4.1e-5, L2_loss=1.2e-6, B_measure=1.6e-6, dB_measure=3.0e-5, wdB=WD_B_TOL),
    #          observed 4.08e-6       4.05e-6         1.14e-7          1.58e-7            2.97e-6
    # sigmoid + full_cross_ent at T = 0.1 saturates: 1 / (fa - [y = 0] + 1e-4) with fa within 1e-4 of 0 or 1 turns the float32 rounding of
    # fa (6e-8) into 1e-3 of the derivative.  Its own row, so that it does not loosen the other anyd cases a hundredfold.
    'anyd-saturated': dict(dB_raw=6.8e-3, L2_grad=2.6e-4, L2_loss=2.3e-4, B_measure=2.2e-5, dB_measure=4.4e-3, wdB=WD_B_TOL),
    #          observed 6.79e-4       2.53e-5         2.29e-5          2.18e-6            4.31e-4
}
# Comparison 3, Context.update_B at the first step against rule() on the oracle's record (increment, relative to max|increment|; here the
# float32 rounding of B itself enters too) and Context.l2_term against the oracle on the same float32 tensor.  The l2_term bounds are
# reasoned: both sides sum float64 products of the same numbers, at most 8192 terms for the loss (n eps = 9e-13); observed 3.3e-16.
L2_TERM_TOL = 1e-12
STANDALONE_BOUNDS = {'lds': dict(inc=9.4e-5, l2_grad=L2_TERM_TOL, l2_loss=L2_TERM_TOL),        # observed 9.36e-6
                     'large': dict(inc=7.5e-5, l2_grad=L2_TERM_TOL, l2_loss=L2_TERM_TOL),      # observed 7.47e-6
                     'anyd': dict(inc=2.9e-6, l2_grad=L2_TERM_TOL, l2_loss=L2_TERM_TOL)}       # observed 2.82e-7
# The persistent sweep at weight_dec = 1, sweep 1 (figures of tests/test_timed_paths_gpu.compare)
PERSIST_BOUNDS = dict(sigma=3.7e-6, env=6.0e-6, f=6.5e-6, off=6.2e-6, mae=1.0e-6)
#                 observed 3.61e-7      5.90e-7    6.47e-7    6.12e-7      9.24e-8
T = 0.1
PAIRS3 = (('linear', 'MSE'), ('softmax', 'full_cross_ent'), ('sigmoid', 'cross_entropy'))
PAIRS9 = tuple((a, l) for a in mo.ACTS for l in mo.LOSSES)


def rule(B, dB_raw, L2_grad, lr):
    """(sumB, sumD, fac, B_new) in float64."""
    B, dB_raw, L2_grad = (np.asarray(a, np.float64) for a in (B, dB_raw, L2_grad))
    dB = dB_raw - L2_grad
    sumB = np.abs(B).sum()
    sumD = np.abs(dB).sum()
    clipped = sumD > sumB
    dB_clip = dB / (sumD / sumB) if clipped else dB
    fac = float(sumB / sumD) if clipped else 1.0
    return float(sumB), float(sumD), fac, B + lr * dB_clip


def _inc(B, dB_raw, L2_grad, lr, fac_mode=None):
    dB = dB_raw - L2_grad
    sumB, sumD = np.abs(B).sum(), np.abs(dB).sum()
    if fac_mode == 'one':
        return lr * dB
    if fac_mode == 'always':
        return lr * (dB / (sumD / sumB))
    return lr * (dB / (sumD / sumB) if sumD > sumB else dB)


MUTANTS_ANY = ('drop', 'double', 'flip', 'fac_one', 'fac_always')
MUTANTS_L2 = ('no_factor_2', 'nh_identity')


def mutants(recs, lr, wd, L2_flag):
    """Per recorded step: dict(clipped, ratio = sum|dB| / sum|B|, inc, mut = {name: increment}, effect = {name: float or None})."""
    out = []
    for rec in recs:
        B, raw, G = rec['B'], rec['dB_raw'], rec['L2_grad']
        sumB, sumD, fac, B_new = rule(B, raw, G, lr)
        assert np.array_equal(B_new, rec['B_new']), 'rule() is not the oracle\'s update'
        inc = B_new - B
        clipped = sumD > sumB
        mut = dict(drop=_inc(B, raw, 0.0 * G, lr), double=_inc(B, raw, 2.0 * G, lr), flip=_inc(B, raw, -G, lr),
                   fac_one=_inc(B, raw, G, lr, 'one') if clipped else None,
                   fac_always=None if clipped else _inc(B, raw, G, lr, 'always'))
        if L2_flag:
            mut['no_factor_2'] = _inc(B, raw, 0.5 * G, lr)
            left = rec['left_dir']
            Nh = rec['Rn'] if left else rec['Ln']
            if Nh.shape == (1, 1):
                mut['nh_identity'] = None
            else:       # the ahead environment alone
                G1 = np.einsum('axycl,cf->axyfl', B, rec['Rn']) if not left else np.einsum('ae,axycl->exycl', rec['Ln'], B)
                mut['nh_identity'] = _inc(B, raw, 2.0 * wd * G1, lr)
        scale = np.abs(inc).max()
        effect = {k: (None if v is None else float(np.abs(v - inc).max() / scale)) for k, v in mut.items()}
        out.append(dict(clipped=bool(clipped), ratio=float(sumD / sumB), inc=inc, mut=mut, effect=effect))
    return out


def smallest_effects(ms):
    """{mutant: (smallest effect over the steps where it is a different rule, number of such steps)}."""
    names = sorted({k for m in ms for k in m['effect']})
    res = {}
    for k in names:
        v = [m['effect'][k] for m in ms if m['effect'].get(k) is not None]
        if v:
            res[k] = (min(v), len(v))
    return res


# ---------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------
def case(kernel, D, M, N, L, b, act, loss, L2_flag, wd=1.0, lr=1e-2, seed=0, trunc='fixed', tag='', standalone=False):
    """kernel: 'lds' (D = 2, the per-step path capture selects), 'large' (D = 2, set_narrow_path(True)) or 'anyd' (D != 2).
    standalone: also checked through Context.update_B / Context.l2_term at its first step."""
    assert (kernel == 'anyd') == (D != 2)
    name = '%s-D%d-M%d-N%d-L%d-b%d-%s-%s-%s-wd%g%s' % (kernel, D, M, N, L, b, act, loss, 'L2' if L2_flag else 'noL2', wd,
                                                     '-' + tag if tag else '')
    return dict(id=name, kernel=kernel, D=D, M=M, N=N, L=L, b=b, act=act, loss=loss, L2_flag=bool(L2_flag), wd=float(wd),
                lr=float(lr), seed=seed, trunc=trunc, tag=tag, standalone=standalone)


def _cases():
    cs = []
    # i. the decay term at the training scripts' weight_dec = 1, both forms, on each kernel
    for kernel, D, M, N, L, b in (('lds', 2, 6, 12, 3, 40), ('large', 2, 10, 12, 3, 100), ('anyd', 3, 6, 8, 3, 100)):
        for act, loss in PAIRS3:
            for l2 in (True, False):
                cs.append(case(kernel, D, M, N, L, b, act, loss, l2, tag='decay', standalone=True))
    # ii. steps that are not clipped, with a decay term that still shows: linear + MSE at a small batch (found by a search over wd
    #     in 1e-2 .. 3e-1, b in 4 .. 16 and four to eight seeds on the oracle; clipped / not clipped steps beside each)
    cs.append(case('lds', 2, 6, 12, 3, 4, 'linear', 'MSE', True, wd=0.01, seed=0, tag='unclipped'))          # 6 / 16
    cs.append(case('lds', 2, 6, 12, 3, 4, 'linear', 'MSE', False, wd=0.3, seed=0, tag='unclipped'))          # 5 / 17
    cs.append(case('large', 2, 10, 12, 3, 4, 'linear', 'MSE', True, wd=0.03, seed=2, tag='unclipped'))       # 10 / 12
    cs.append(case('large', 2, 10, 12, 3, 4, 'linear', 'MSE', False, wd=0.1, seed=2, tag='unclipped'))       # 4 / 18
    cs.append(case('anyd', 3, 6, 8, 3, 8, 'linear', 'MSE', True, wd=0.1, seed=2, tag='unclipped'))           # 8 / 6
    cs.append(case('anyd', 3, 6, 8, 3, 8, 'linear', 'MSE', False, wd=0.3, seed=6, tag='unclipped'))          # 4 / 10
    # iii. D = 5 and D = 8
    cs.append(case('anyd', 5, 4, 7, 2, 100, 'softmax', 'full_cross_ent', True, tag='D5'))
    cs.append(case('anyd', 8, 4, 6, 2, 100, 'linear', 'MSE', False, tag='D8'))
    # iv. the six pairs (i) leaves out, L2 on, at its D = 3 shape.  sigmoid + full_cross_ent saturates at T = 0.1 (sum|dB| / sum|B| above
    #     1e3 in every step): at wd = 1 no seed or batch reached the floor (no_factor_2 at most 1.2e-3), at wd = 30 every mutant does
    for act, loss in PAIRS9:
        if (act, loss) == ('sigmoid', 'full_cross_ent'):
            cs.append(case('anyd', 3, 6, 8, 3, 100, act, loss, True, wd=30.0, seed=0, tag='pairs'))
        elif (act, loss) not in PAIRS3:
            cs.append(case('anyd', 3, 6, 8, 3, 100, act, loss, True, seed=2, tag='pairs'))
    # v. twenty labels: labels 16 .. 19 of f come from the plain-FMA tail
    cs.append(case('anyd', 3, 6, 7, 20, 70, 'softmax', 'full_cross_ent', True, tag='L20'))
    # vi. D g L = 144 columns of the f product: two 128-column chunks, the second starting at label phase 128 % 6 = 2
    cs.append(case('anyd', 3, 8, 7, 6, 100, 'softmax', 'full_cross_ent', False, tag='chunks'))
    # vii. three 64-sample tiles, the last holding 22 samples
    cs.append(case('anyd', 3, 6, 8, 3, 150, 'sigmoid', 'cross_entropy', True, tag='ragged'))
    # viii. an odd bond: odd matrix sides, padded by one inside the kernel
    cs.append(case('anyd', 3, 5, 8, 2, 100, 'linear', 'MSE', True, tag='odd', trunc='reference'))
    ids = [c['id'] for c in cs]
    assert len(set(ids)) == len(ids)
    return cs


PERSIST = dict(N=12, M=6, L=3, b=40, seed=5, lr=1e-2, wd=1.0)     # shape of tests/test_timed_paths_gpu.py's activation cases


# ---------------------------------------------------------------------------------------------------------------
# the oracle's record of a case: two sweeps (right, then left) from the float32-rounded calibrated start
# ---------------------------------------------------------------------------------------------------------------
def inputs(c):
    from test_feature_dim_gpu import problem
    return problem(c['N'], c['M'], c['D'], c['L'], c['b'], seed=c['seed'])


def oracle_steps(X, y, cores32, c, wd=None, n_sweeps=2):
    """Generator over the oracle's steps: yields (sweep, step, record) after each step; the record also holds the two norm
    environments of the step (Ln, Rn), its direction and f before / after.  The caller may run a device beside it."""
    N, D, L, M = c['N'], c['D'], c['L'], c['M']
    wd = c['wd'] if wd is None else wd
    st = mo.MPSState(N, D, L, M, [np.asarray(a, np.float64) for a in cores32], 0)
    Xd = np.asarray(X, np.float64)
    y1h = mo.one_hot(y, L)
    for sw in range(n_sweeps):
        f = mo.forward(st, Xd)
        left = st.l_pos == N - 1
        if left:
            st.Renv = {}
        else:
            st.Lenv = {}
        for j in range(N - 1):
            p = st.l_pos - 1 if left else st.l_pos
            rec = dict(Ln=mo.norm_env_left(st, p - 1).copy(), Rn=mo.norm_env_right(st, p + 2).copy(), left_dir=left, sweep=sw,
                       step=j, f_prev=f)
            f = mo.sweep_step(st, f, y1h, c['lr'], wd, L2_flag=c['L2_flag'], left_dir=left, act_fn=c['act'], loss_fn=c['loss'],
                              T=T, trunc=c['trunc'], record=rec)
            rec['bond'] = list(st.bond)
            rec['l_pos'] = st.l_pos
            yield sw, j, rec


@functools.lru_cache(maxsize=None)
def _record(cid):
    c = BY_ID[cid]
    X, y, c32 = inputs(c)
    return X, y, c32, [rec for _, _, rec in oracle_steps(X, y, c32, c)]


def record(c):
    """(X, y, cores32, records of the 2 (N - 1) steps), computed once per case and shared; treat as read-only."""
    return _record(c['id'])


CASES = _cases()
BY_ID = {c['id']: c for c in CASES}
