"""Likelihood training in float64 NumPy (test infrastructure): one optimiser step on the gradient of the
negative log-likelihood and a run of such steps, stated with nll_reference.nll_gradient (the gradient G = Gd - Gz and the value),
the update rules of gradient_step_reference.GradientStepReference (SGD with the per-core clip and momentum, Adam with decoupled
decay) and the renormalisation of include/tnml.h:

    A'_i = A_i + lr (...)                                         the rule of section 17 on G_i
    A'_i <- A'_i sqrt(sum A_i^2 / sum A'_i^2)                     renorm; no factor where sum A'_i^2 is 0 or not finite

Also the shared cases of tests/test_nll_step_host.py (which checks the conditions on them with this reference alone) and
tests/test_nll_step_gpu.py (which runs them on the device), and the tables the bounds of the GPU tests are read from.

emulate=True is the float32 emulation of nll_reference.py carried through the step: chains and gradient in float32, the update in
float64 from the float32 gradient and the float32 state, one rounding to float32 on every store (cores and state).

lr and weight_dec cross the C ABI as float32: the reference rounds them the same way before it computes in float64.
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

import nll_reference as nref                                                                 # noqa: E402
import orthogonalize_reference as oref                                                       # noqa: E402
from gradient_step_reference import CLIP_MARGIN, f32                                         # noqa: E402,F401
from sample_reference import gram, grid, walk                                                # noqa: E402

WD = 1e-2
# (Adam's eps as tests/test_gradient_step_gpu.py sets it: at 1e-8 an element whose gradient is rounding noise moves by lr times its sign)
OPTIMS = {'sgd': dict(kind='sgd', momentum=0.0, clip=False), 'sgd_clip_mom': dict(kind='sgd', momentum=0.9, clip=True),
          'adam': dict(kind='adam', momentum=0.0, clip=False, eps=1e-3), 'momentum': dict(kind='sgd', momentum=0.9, clip=False)}
STEP_OPTIMS = ('sgd', 'sgd_clip_mom', 'adam')
OBJECTIVES = ('joint', 'marginal')


def _r32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


class NllStepReference:
    """cores: list of arrays (ml, D, mr[, L]) (taken as float64 copies), label on site l, S the metric.  step() changes self.cores in
    place of the list and returns (nll, log Z) of the batch before the step."""

    def __init__(self, cores, l, S, kind='sgd', momentum=0.0, betas=(0.9, 0.999), eps=1e-8, clip=True, renorm=True, emulate=False):
        assert kind in ('sgd', 'adam') and not (kind == 'adam' and clip)
        self.cores = [np.array(c, dtype=np.float64) for c in cores]
        self.l, self.S, self.kind, self.mu, self.b1, self.b2, self.eps = l, S, kind, float(momentum), betas[0], betas[1], float(eps)
        self.clip, self.renorm, self.emulate = bool(clip), bool(renorm), bool(emulate)
        self.t = 0
        self.vel = [np.zeros_like(c) for c in self.cores]
        self.m = [np.zeros_like(c) for c in self.cores]
        self.v = [np.zeros_like(c) for c in self.cores]
        self.ratio = None                                       # s_d / s_A per core of the last SGD step

    def gradient(self, X, y):
        return nref.nll_gradient(self.cores, self.l, X, y, self.S, dtype=np.float32 if self.emulate else np.float64)

    def apply(self, G, lr, wd):
        """the optimiser tail on a gradient G (list of float64 arrays)"""
        lr, wd = f32(lr), f32(wd)
        store = _r32 if self.emulate else (lambda a: a)
        self.ratio = np.zeros(len(self.cores))
        if self.kind == 'adam':
            self.t += 1
        for i, (A, g) in enumerate(zip(self.cores, G)):
            if self.kind == 'sgd':
                d = g - wd * A
                s_A, s_d = np.abs(A).sum(), np.abs(d).sum()
                self.ratio[i] = s_d / s_A if s_A > 0 else np.inf
                if self.clip and s_d > s_A:
                    d = d * (s_A / s_d)
                if self.mu > 0:
                    d = self.mu * self.vel[i] + d
                    self.vel[i] = store(d)
                new = A + lr * d
            else:
                mn = self.b1 * self.m[i] + (1 - self.b1) * g
                vn = self.b2 * self.v[i] + (1 - self.b2) * g * g
                self.m[i], self.v[i] = store(mn), store(vn)
                new = A + lr * ((mn / (1 - self.b1 ** self.t)) / (np.sqrt(vn / (1 - self.b2 ** self.t)) + self.eps) - wd * A)
            if self.renorm:
                q0, q1 = float((A * A).sum()), float((new * new).sum())
                if q1 > 0.0 and math.isfinite(q1):
                    new = new * math.sqrt(q0 / q1)
            self.cores[i] = store(new)

    def step(self, X, y, lr, wd):
        G, value, logz = self.gradient(X, y)
        self.apply(G, lr, wd)
        return value, logz


# ---------------------------------------------------------------------------------------------------------------
# test 1: one step on every row of nll_reference.likelihood_cases()
# ---------------------------------------------------------------------------------------------------------------
MIN_MOVE = 1e-2             # the largest change of a core element, of max|A|: the store's own rounding (2^-24 of |A|) stays far below


def configs():
    """(objective, optimiser name, renorm) of test 1"""
    return [(o, k, r) for o in OBJECTIVES for k in STEP_OPTIMS for r in (True, False)]


def config_id(cfg):
    return '%s-%s-%s' % (cfg[0], cfg[1], 'renorm' if cfg[2] else 'plain')


def moved(new, old):
    return max(float(np.abs(a - c).max()) for a, c in zip(new, old))


def case_lr(cores, l, S, G, name):
    """the float32 lr at which the plain rule of optimiser `name` moves the cores by 2 MIN_MOVE max|A| (the rules are linear in lr;
    the renormalised step then still moves them by more than MIN_MOVE, which tests/test_nll_step_host.py asserts)"""
    ref = NllStepReference(cores, l, S, renorm=False, **OPTIMS[name])
    ref.apply(G, 1.0, WD)
    amax = max(float(np.abs(c).max()) for c in cores)
    return float(np.float32(2.0 * MIN_MOVE * amax / moved(ref.cores, cores)))


def step_deviation(new, ref_new, old):
    """max|A' - A'_ref| over all cores, of max|A'_ref - A| over all cores"""
    return moved(new, ref_new) / moved(ref_new, old)


class StepCase:
    """One row of likelihood_cases() with both gradients computed once: .cores, .l, .X, .lab, .S, .G[objective] (float64) and
    .G32[objective] (the emulation's)."""

    def __init__(self, lc, emulation=False):
        self.lc = lc
        self.cores, self.l, self.lev, self.lab, self.X, self.S = nref.build_likelihood_case(lc)
        self.G, self.G32, self.value = {}, {}, {}
        for name, y in (('joint', self.lab), ('marginal', None)):
            self.G[name], self.value[name], self.logz = nref.nll_gradient(self.cores, self.l, self.X, y, self.S)
            if emulation:
                self.G32[name] = nref.nll_gradient(self.cores, self.l, self.X, y, self.S, dtype=np.float32)[0]

    def y(self, objective):
        return self.lab if objective == 'joint' else None

    def lr(self, cfg):
        return case_lr(self.cores, self.l, self.S, self.G[cfg[0]], cfg[1])

    def reference(self, cfg, emulate=False):
        """the reference after one step of the configuration from the case's cores, and the lr used"""
        lr = self.lr(cfg)
        ref = NllStepReference(self.cores, self.l, self.S, renorm=cfg[2], emulate=emulate, **OPTIMS[cfg[1]])
        ref.apply((self.G32 if emulate else self.G)[cfg[0]], lr, WD)
        return ref, lr


def step_emulation_figures(lc):
    """{config id: deviation of the float32 emulation's step from the float64 step} on one case"""
    case = StepCase(lc, emulation=True)
    out = {}
    for cfg in configs():
        ref, _ = case.reference(cfg)
        emu, _ = case.reference(cfg, emulate=True)
        out[config_id(cfg)] = step_deviation(emu.cores, ref.cores, case.cores)
    return out


# ---------------------------------------------------------------------------------------------------------------
# test 2: three steps with state, on the case's own batch
# ---------------------------------------------------------------------------------------------------------------
# (momentum without the clip: CLIP_MARGIN is a condition on the first step's inputs, and float32 may decide a later clip differently)
STATE_OPTIMS = ('momentum', 'adam')


def three_step_cases():
    """the rows of likelihood_cases() with N > 2 and b = 17, the batch that is no multiple of the tile: two per row.  b = 1 leaves
    nothing to sum; among the b = 70 rows are trajectories on which min |f_y| / max|f| falls below MIN_RATIO within the three steps
    (the cotangent 1 / f_y then amplifies any rounding: float32 and float64 part ways by up to 0.16 of the move)."""
    return [lc for lc in nref.likelihood_cases() if lc[0][3] > 2 and lc[1] == 17]


def three_steps(case, name, emulate=False):
    """the reference after three joint, renormalised steps of optimiser `name` on the case's batch, at the lr of test 1"""
    lr = case.lr(('joint', name, True))
    ref = NllStepReference(case.cores, case.l, case.S, renorm=True, emulate=emulate, **OPTIMS[name])
    for _ in range(3):
        ref.step(case.X, case.lab, lr, WD)
    return ref, lr


def three_step_emulation_figures(lc):
    case = StepCase(lc)
    return {name: step_deviation(three_steps(case, name, True)[0].cores, three_steps(case, name)[0].cores, case.cores) for name in STATE_OPTIMS}


# ---------------------------------------------------------------------------------------------------------------
# test 5: the short run
# ---------------------------------------------------------------------------------------------------------------
RUN = dict(N=16, D=2, L=2, M=4, l=0, n=200, batch=50, steps=20, lr=0.03, wd=0.0)


def _positive_chain(rng, Xc):
    """cores drawn as Network() draws them, U[0, 1) + 0.1, calibrated to max|f| = 1 on Xc and rounded to float32: f > 0 on the whole
    grid (the features of [0, 1] are not negative), so no sample sits next to a zero of f_y, where -log f_y^2 has a pole"""
    N, D, L, M, l = RUN['N'], RUN['D'], RUN['L'], RUN['M'], RUN['l']
    cores = [rng.random(s) + 0.1 for s in oref.shapes_of(N, D, L, [M] * (N - 1), l)]
    k = np.abs(nref.forward(cores, l, Xc.astype(np.float64))).max() ** (-1.0 / N)
    return [_r32(c * k) for c in cores]


def training_run_setup():
    """(levels (200, 16), labels, X float32 (200, 16, 2), start cores (float32 values), S, index list of the 20 steps): images and
    labels drawn by sample_reference.walk from a teacher chain, the batches of 50 taken in order, round and round; plain SGD with
    renorm from a student chain drawn like the teacher."""
    N, D = RUN['N'], RUN['D']
    rng = np.random.default_rng([25, N, RUN['M'], 0])
    Xc = oref.features(rng, 16, N, D)
    teacher, student = _positive_chain(rng, Xc), _positive_chain(rng, Xc)
    _, phi, w = grid(nref.K, D)
    lev, lab, _, _ = walk(teacher, RUN['l'], phi, w, np.full(RUN['n'], -1), rng.random((RUN['n'], N + 1)))
    idx = np.concatenate([np.arange(RUN['n'])] * (RUN['steps'] * RUN['batch'] // RUN['n'] + 1))[:RUN['batch'] * RUN['steps']]
    return lev, np.asarray(lab, dtype=np.int32), phi[lev].astype(np.float32), student, gram(phi, w), idx


def training_run(emulate=False, setup=None):
    """(values per step, min_s |f_y| / max|f| of every step's batch at the cores it meets, reference) of the trajectory"""
    lev, lab, X, cores, S, idx = setup or training_run_setup()
    ref = NllStepReference(cores, RUN['l'], S, kind='sgd', momentum=0.0, clip=False, renorm=True, emulate=emulate)
    vals, ratios = [], []
    for k in range(RUN['steps']):
        sel = idx[k * RUN['batch']:(k + 1) * RUN['batch']]
        ratios.append(nref.label_ratio(ref.cores, RUN['l'], X[sel], lab[sel]))
        vals.append(ref.step(X[sel], lab[sel], RUN['lr'], RUN['wd'])[0])
    return np.array(vals), np.array(ratios), ref


def trajectory_deviation(vals, ref_vals):
    return float((np.abs(vals - ref_vals) / np.maximum(1.0, np.abs(ref_vals))).max())


# ---------------------------------------------------------------------------------------------------------------
# the tables the GPU bounds are read from
# ---------------------------------------------------------------------------------------------------------------
# The worst deviation of the float32 emulation's step from the float64 step per row (D, cap, L) and configuration over the cases of
# nll_reference.likelihood_cases(), of the largest change of a core element.  tests/test_nll_step_host.py asserts that the code still
# gives these figures (within a quarter: einsum's summation order follows the host's vector width).
STEP_EMULATION = {
    (2, 5, 3): {
        'joint-sgd-renorm': 2.382e-06, 'joint-sgd-plain': 2.893e-06, 'joint-sgd_clip_mom-renorm': 2.364e-06, 'joint-sgd_clip_mom-plain': 2.893e-06,
        'joint-adam-renorm': 2.394e-05, 'joint-adam-plain': 4.644e-05, 'marginal-sgd-renorm': 2.630e-06, 'marginal-sgd-plain': 2.397e-06,
        'marginal-sgd_clip_mom-renorm': 2.630e-06, 'marginal-sgd_clip_mom-plain': 2.397e-06, 'marginal-adam-renorm': 2.325e-05, 'marginal-adam-plain': 4.077e-05,
    },
    (2, 33, 2): {
        'joint-sgd-renorm': 2.388e-06, 'joint-sgd-plain': 2.268e-06, 'joint-sgd_clip_mom-renorm': 2.345e-06, 'joint-sgd_clip_mom-plain': 2.983e-06,
        'joint-adam-renorm': 4.279e-05, 'joint-adam-plain': 5.708e-05, 'marginal-sgd-renorm': 2.590e-06, 'marginal-sgd-plain': 2.481e-06,
        'marginal-sgd_clip_mom-renorm': 2.590e-06, 'marginal-sgd_clip_mom-plain': 2.481e-06, 'marginal-adam-renorm': 4.297e-05, 'marginal-adam-plain': 5.504e-05,
    },
    (2, 64, 2): {
        'joint-sgd-renorm': 2.528e-06, 'joint-sgd-plain': 2.594e-06, 'joint-sgd_clip_mom-renorm': 2.528e-06, 'joint-sgd_clip_mom-plain': 2.594e-06,
        'joint-adam-renorm': 9.022e-05, 'joint-adam-plain': 1.138e-04, 'marginal-sgd-renorm': 2.363e-06, 'marginal-sgd-plain': 2.444e-06,
        'marginal-sgd_clip_mom-renorm': 2.363e-06, 'marginal-sgd_clip_mom-plain': 2.444e-06, 'marginal-adam-renorm': 1.089e-04, 'marginal-adam-plain': 1.406e-04,
    },
    (2, 50, 10): {
        'joint-sgd-renorm': 2.854e-06, 'joint-sgd-plain': 3.005e-06, 'joint-sgd_clip_mom-renorm': 2.854e-06, 'joint-sgd_clip_mom-plain': 3.005e-06,
        'joint-adam-renorm': 9.790e-05, 'joint-adam-plain': 1.287e-04, 'marginal-sgd-renorm': 5.319e-06, 'marginal-sgd-plain': 5.280e-06,
        'marginal-sgd_clip_mom-renorm': 5.319e-06, 'marginal-sgd_clip_mom-plain': 5.280e-06, 'marginal-adam-renorm': 2.148e-04, 'marginal-adam-plain': 2.772e-04,
    },
    (3, 7, 3): {
        'joint-sgd-renorm': 2.991e-06, 'joint-sgd-plain': 2.591e-06, 'joint-sgd_clip_mom-renorm': 2.991e-06, 'joint-sgd_clip_mom-plain': 2.591e-06,
        'joint-adam-renorm': 2.334e-05, 'joint-adam-plain': 3.146e-05, 'marginal-sgd-renorm': 2.741e-06, 'marginal-sgd-plain': 3.148e-06,
        'marginal-sgd_clip_mom-renorm': 2.741e-06, 'marginal-sgd_clip_mom-plain': 3.148e-06, 'marginal-adam-renorm': 3.187e-05, 'marginal-adam-plain': 4.277e-05,
    },
    (8, 16, 17): {
        'joint-sgd-renorm': 2.500e-06, 'joint-sgd-plain': 2.542e-06, 'joint-sgd_clip_mom-renorm': 2.500e-06, 'joint-sgd_clip_mom-plain': 2.542e-06,
        'joint-adam-renorm': 7.057e-05, 'joint-adam-plain': 9.615e-05, 'marginal-sgd-renorm': 2.444e-06, 'marginal-sgd-plain': 2.498e-06,
        'marginal-sgd_clip_mom-renorm': 2.444e-06, 'marginal-sgd_clip_mom-plain': 2.498e-06, 'marginal-adam-renorm': 4.043e-05, 'marginal-adam-plain': 6.761e-05,
    },
}
# the same after three steps with state (joint, renorm), per row and optimiser
THREE_STEP_EMULATION = {
    (2, 5, 3): {'momentum': 9.15e-07, 'adam': 7.88e-06},
    (2, 33, 2): {'momentum': 2.35e-06, 'adam': 1.74e-05},
    (2, 64, 2): {'momentum': 3.55e-06, 'adam': 4.57e-04},
    (2, 50, 10): {'momentum': 1.34e-06, 'adam': 2.29e-05},
    (3, 7, 3): {'momentum': 9.20e-07, 'adam': 6.40e-06},
    (8, 16, 17): {'momentum': 1.33e-06, 'adam': 2.82e-05},
}
# the short run: max_k |value_k - reference value_k| / max(1, |reference value_k|) of the emulation
TRAJECTORY_EMULATION = 8.865e-08


def step_bound(row, cfg):
    """ten times the emulation's figure, rounded up to one digit: the project's rule for G (section 24), with the same reason for
    the factor ten -- the summation order is the one thing the emulation does not share with the kernels"""
    return nref.round_up_one_digit(10.0 * STEP_EMULATION[tuple(row)][config_id(cfg)])


def three_step_bound(row, name):
    return nref.round_up_one_digit(10.0 * THREE_STEP_EMULATION[tuple(row)][name])


def trajectory_bound():
    return nref.round_up_one_digit(10.0 * TRAJECTORY_EMULATION)
