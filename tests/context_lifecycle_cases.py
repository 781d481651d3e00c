"""Tables of the context life-cycle tests: shapes, mutators, readers, consumers and the verdict of every (mutator, call) pair.

tests/test_context_lifecycle_gpu.py drives one long-lived context through a mutator and asks of every call whether it returns what
the same call returns on a fresh context that was handed the same cores and the same batch; tests/test_context_lifecycle_host.py checks
these tables for completeness and computes the one factor they hold.  Nothing here needs a GPU: the functions take a `Live` (a context
with the book-keeping a twin needs) and are only called by the GPU tests.

SHAPES are the smallest at which padding, growth and shrinking all occur: N = 8, L = 3, ragged bonds (2, 4, 4, 3, 4, 4, 2), a context
created for M = 12 and 37 samples, batches of 37, 70 (grows the batch group; no multiple of 16, 32 or 64) and 5, a pixel dataset of 96
samples, K = 8 grid levels.  A: D = 2, the default persistent sweep; B: D = 3 (the generic-D path); C: A on the large-tensor path; D / E:
A under set_persistent(0) / (2).

A MUTATOR is a function (live, rng) -> None.  A READER is a function (ctx, pr) -> tuple of arrays that changes neither cores nor batch;
a CONSUMER also moves the model, runs last on a state of its own, and returns get_cores() with its results.

verdict(mutator, call) is one of
  'equal'    bit for bit against the fresh context (the default);
  'refused'  the API documents TNML_ERR_STATE until a remedy (REMEDY: 'forward' or 'optim_reset'); the refusal is asserted with its
             code and the first words of its message, the remedy applied on both sides, the pair compared as 'equal';
  'carried'  the design hands a float64 quantity from the mutator to the call along another route than a fresh context takes; every
             such pair cites the line that carries it (CARRIED).
sensitive(mutator, call): the mutator must change the call's result (the control against a call that ignores its inputs).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p_ in (ROOT, HERE):
    if p_ not in sys.path:
        sys.path.insert(0, p_)

import batch_handover_cases as bc                                  # noqa: E402
import sample_reference as sr                                      # noqa: E402
from oracle import mps_oracle as mo                                # noqa: E402
from test_any_position_host import label_inside_forward, place, random_cores_at    # noqa: E402

N, L, M, CAPACITY = 8, 3, 12, 37
BONDS = (2, 4, 4, 3, 4, 4, 2)
OTHER_BONDS = (3, 4, 2, 4, 3, 4, 3)              # set_cores_bonds
ADD_BONDS = (2, 4, 4, 4, 4, 4, 2)                # the second chain of axpby: the bonds grow to 4 + 4 = 8
SIZES = (37, 70, 5)
DATASET_N, K, N_DRAW, N_PRED = 96, 8, 19, 45
SEED = 20260
# the hyper-parameters of tests/test_update_record_gpu.py (hp_of(True)), in the order of Context.sweep behind first_of_sweep
HP = (1e-2, 1e-3, True, 'softmax', 'full_cross_ent', 0.1, 'fixed')
HP_REFERENCE = HP[:6] + ('reference',)
GD = (1e-2, 1e-3, 'softmax', 'full_cross_ent', 0.1)               # lr, weight_dec, act_fn, loss_fn, T of gd_step
OPTIM_START = dict(kind='adam', clip=False)

SHAPES = {
    'A': dict(D=2, calls=()),
    'B': dict(D=3, calls=()),
    'C': dict(D=2, calls=(('set_narrow_path', 1),)),
    'D': dict(D=2, calls=(('set_persistent', 0),)),
    'E': dict(D=2, calls=(('set_persistent', 2),)),
}
# calls a shape refuses at the start state itself are left out of its table (none: the generic-D path takes every call of the table)
LEFT_OUT = {name: () for name in SHAPES}

ARG, STATE = -1, -2
S_L, S_R = 0, 1


# ---------------------------------------------------------------------------------------------------------------
# the problem of a shape: built once, never written to
# ---------------------------------------------------------------------------------------------------------------
_problems = {}


def cores_at(D, bond, l_pos, seed):
    rng = np.random.default_rng(seed)
    return [a.astype(np.float32) for a in random_cores_at(N, D, L, bond, l_pos, rng, scale=0.5 * max(bond))]


def problem(shape):
    if shape not in _problems:
        D = SHAPES[shape]['D']
        rng = np.random.default_rng(SEED + D)
        pr = dict(shape=shape, N=N, D=D, L=L, M=M, capacity=CAPACITY, calls=SHAPES[shape]['calls'])
        pr['cores'] = cores_at(D, BONDS, 0, SEED + 10 * D)
        pr['batches'] = {b: bc.make_batch(N, D, L, b, SEED + 100 * D + b) for b in SIZES}
        pr['pixels'] = rng.random((DATASET_N, N)).astype(np.float32)
        pr['ds_labels'] = rng.integers(0, L, DATASET_N).astype(np.int32)
        pr['idx'] = rng.permutation(DATASET_N)[:41].astype(np.int32)               # the *_indices readers
        pr['idx_select'] = rng.permutation(DATASET_N)[:53].astype(np.int32)        # the select_indices mutator
        pr['Xp'], pr['yp'] = bc.make_batch(N, D, L, N_PRED, SEED + 100 * D + 1)     # predict, gradients, gd_step: not resident
        _, phi, w = sr.grid(K, D)
        pr['phi'], pr['w'], pr['S'] = phi, w, sr.gram(phi, w)
        lev = rng.integers(0, K, (N_DRAW, N))
        pr['Xg'], pr['yg'] = phi[lev].astype(np.float32), rng.integers(0, L, N_DRAW).astype(np.int32)   # on the grid: the likelihood calls
        pr['known'] = lev.astype(np.int32)
        pr['mask'] = (np.arange(N) % 2 == 0)                                       # checker
        pr['y_other'] = ((pr['batches'][37][1] + 1) % L).astype(np.int32)          # set_labels
        _problems[shape] = pr
    return _problems[shape]


def other_chain(pr, l_pos, bond=(3,) * (N - 1), seed=5):
    """the fixed second chain of `inner` and `axpby`, with its label where the context's is"""
    return cores_at(pr['D'], bond, l_pos, SEED + 1000 * seed + 10 * pr['D'] + l_pos)


# ---------------------------------------------------------------------------------------------------------------
# a context and what a twin needs to know about it
# ---------------------------------------------------------------------------------------------------------------
class Live:
    """A context, the switches and the optimiser it was given, and how its resident batch is loaded."""

    def __init__(self, ctx, pr):
        self.ctx, self.pr = ctx, pr
        self.switches = list(pr['calls'])
        self.optim = dict(OPTIM_START)
        self.batch = None
        for method, arg in self.switches:
            getattr(ctx, method)(arg)
        ctx.optim_config(**self.optim)
        ctx.dataset_attach(pr['pixels'], pr['ds_labels'], form='pixels')

    def switch(self, method, arg):
        getattr(self.ctx, method)(arg)
        self.switches = [s for s in self.switches if s[0] != method] + [(method, arg)]

    def configure(self, **optim):
        self.optim = optim
        self.ctx.optim_config(**optim)

    def load(self, how, *args):
        """('input', b) | ('labels', b) | ('indices',) | ('staged', b): the resident batch, by the call of that name"""
        c, pr = self.ctx, self.pr
        if how == 'input':
            c.set_input(*pr['batches'][args[0]])
        elif how == 'labels':
            c.set_labels(pr['y_other'])
        elif how == 'indices':
            c.select_indices(pr['idx_select'])
        elif how == 'staged':
            c.stage_batch(3, *pr['batches'][args[0]])
            c.select_batch(3)
        self.batch = (how,) + args

    def mirror_batch(self, other):
        """the same batch on a twin: a staged batch by set_input, new labels with their inputs, a selection by the same indices"""
        c, pr, how = other.ctx, self.pr, self.batch[0]
        if how in ('input', 'staged'):
            c.set_input(*pr['batches'][self.batch[1]])
        elif how == 'labels':
            c.set_input(pr['batches'][37][0], pr['y_other'])
        else:
            c.select_indices(pr['idx_select'])
        other.batch = self.batch

    def batch_arrays(self):
        """(X float64, y) of the resident batch as the device holds it"""
        c, pr, how = self.ctx, self.pr, self.batch[0]
        if how in ('input', 'staged'):
            X, y = pr['batches'][self.batch[1]]
        elif how == 'labels':
            X, y = pr['batches'][37][0], pr['y_other']
        else:
            X, y = c.dataset_read(pr['idx_select']), pr['ds_labels'][pr['idx_select']]
        return np.asarray(X, np.float64), y


def start(live):
    """the start state: the shape's cores with the label on site 0, the batch of 37"""
    live.ctx.set_cores(live.pr['cores'], 0)
    live.load('input', 37)


# ---------------------------------------------------------------------------------------------------------------
# mutators
# ---------------------------------------------------------------------------------------------------------------
def reference_steps(D):
    """steps of a right sweep from the start bonds that the reference truncation rule allows (its last step raises the reference's own
    ValueError where D ml < D L with ml the collapsed bond: D = 2, L = 3)"""
    bond = list(BONDS)
    for p in range(N - 1):
        ml = 1 if p == 0 else bond[p - 1]
        mr = 1 if p == N - 2 else bond[p + 1]
        m, ok = mo.trunc_rank('reference', False, p, N, ml, D, mr, L, M)
        if not ok:
            return p
        bond[p] = m
    return N - 1


def m_set_cores(live, rng):
    cores = [(a * (0.75 + 0.5 * rng.random(a.shape))).astype(np.float32) for a in live.pr['cores']]
    live.ctx.set_cores(cores, 0)


def m_set_cores_bonds(live, rng):
    live.ctx.set_cores(cores_at(live.pr['D'], OTHER_BONDS, N - 1, int(rng.integers(1 << 30))), N - 1)


def m_scale_cores(live, rng):
    live.ctx.scale_cores(0.9)


def m_sweep_right(live, rng):
    live.ctx.forward(want_f=False)
    live.ctx.sweep(False, N - 1, True, *HP, want_metrics=False, want_f=False)


def m_sweep_reference(live, rng):
    n = reference_steps(live.pr['D'])
    if n < N - 1:                                                   # the sweep stops in front of the step the reference itself refuses
        live.switch('set_any_position', True)
    live.ctx.forward(want_f=False)
    live.ctx.sweep(False, n, True, *HP_REFERENCE, want_metrics=False, want_f=False)


def m_segment(live, rng):
    live.switch('set_any_position', True)
    live.ctx.forward(want_f=False)
    live.ctx.sweep(False, 3, True, *HP, want_metrics=False, want_f=False)


def m_gd_step_sgd_momentum(live, rng):
    live.configure(kind='sgd', momentum=0.9, clip=True)
    live.ctx.gd_step(live.pr['Xp'], live.pr['yp'], *GD)


def m_gd_step_adam(live, rng):
    live.configure(kind='adam', clip=False)
    live.ctx.gd_step(live.pr['Xp'], live.pr['yp'], 1e-3, *GD[1:])


def m_nll_step(live, rng):
    live.ctx.nll_step(live.pr['Xg'], live.pr['yg'], live.pr['S'], lr=1e-3, weight_dec=0.0, renorm=True)


def m_orthogonalize(live, rng):
    live.ctx.orthogonalize()


def m_compress_to_3(live, rng):
    live.ctx.compress(3)


def m_axpby(live, rng):
    c = live.ctx
    c.axpby(0.7, 0.4, other_chain(live.pr, c.l_pos, ADD_BONDS, seed=6), c.l_pos)


def m_set_input_70(live, rng):
    live.load('input', 70)


def m_set_input_5(live, rng):
    live.load('input', 5)


def m_select_indices(live, rng):
    live.load('indices')


def m_stage_select(live, rng):
    live.load('staged', 70)


def m_set_labels(live, rng):
    live.load('labels', 37)


def m_chain_scaling_on(live, rng):
    live.switch('set_chain_scaling', 1)


def m_chain_scaling_off(live, rng):
    live.switch('set_chain_scaling', 1)
    live.switch('set_chain_scaling', 0)


# name: (function, what it changes, changes bonds or l_pos or unbinds the optimiser, leaves an optimiser state behind)
MUTATORS = {
    'set_cores': (m_set_cores, 'model', False, False),
    'set_cores_bonds': (m_set_cores_bonds, 'model', True, False),
    'scale_cores': (m_scale_cores, 'model', False, False),
    'sweep_right': (m_sweep_right, 'model', True, False),
    'sweep_reference': (m_sweep_reference, 'model', True, False),
    'segment': (m_segment, 'model', True, False),
    'gd_step_sgd_momentum': (m_gd_step_sgd_momentum, 'model', False, True),
    'gd_step_adam': (m_gd_step_adam, 'model', False, True),
    'nll_step': (m_nll_step, 'model', False, True),
    'orthogonalize': (m_orthogonalize, 'model', True, False),
    'compress_to_3': (m_compress_to_3, 'model', True, False),
    'axpby': (m_axpby, 'model', True, False),
    'set_input_70': (m_set_input_70, 'batch', False, False),
    'set_input_5': (m_set_input_5, 'batch', False, False),
    'select_indices': (m_select_indices, 'batch', False, False),
    'stage_batch+select_batch': (m_stage_select, 'batch', False, False),
    'set_labels': (m_set_labels, 'labels', False, False),
    'chain_scaling_on': (m_chain_scaling_on, 'switch', False, False),
    'chain_scaling_off': (m_chain_scaling_off, 'switch', False, False),
}
SWEEPS = ('sweep_right', 'sweep_reference', 'segment')


def changes(mutator):
    return MUTATORS[mutator][1]


def rebinds(mutator):
    return MUTATORS[mutator][2]


def stateful(mutator):
    return MUTATORS[mutator][3]


# ---------------------------------------------------------------------------------------------------------------
# readers
# ---------------------------------------------------------------------------------------------------------------
def flat(*parts):
    """a tuple of arrays from arrays, lists of arrays, tuples and scalars"""
    out = []
    for p in parts:
        if p is None:
            continue
        if isinstance(p, (list, tuple)):
            out.extend(flat(*p))
        else:
            out.append(np.asarray(p))
    return tuple(out)


def model_of(ctx):
    cores, bond, l_pos = ctx.get_cores()
    return flat(cores, bond, l_pos)


def left_step(ctx):
    return ctx.l_pos == ctx.N - 1


def merged_shape(ctx):
    _, bond, l = ctx.get_cores()
    p = l - 1 if left_step(ctx) else l
    return (1 if p == 0 else int(bond[p - 1]), ctx.D, ctx.D, 1 if p == ctx.N - 2 else int(bond[p + 1]), ctx.L)


def r_forward(ctx, pr):
    f, l = ctx.forward(), ctx.l_pos
    return flat(f, [ctx.get_env(S_L, i) for i in range(l)], [ctx.get_env(S_R, i) for i in range(l + 1, ctx.N)])


def r_predict(ctx, pr):
    return flat(ctx.predict(pr['Xp']))


def r_predict_scaled(ctx, pr):
    return flat(ctx.predict_scaled(pr['Xp']))


def r_predict_indices(ctx, pr):
    return flat(ctx.predict_indices(pr['idx']))


def r_eval_indices(ctx, pr):
    return flat(ctx.eval_indices(pr['idx'], 'softmax', 0.1))


def r_resident_metrics(ctx, pr):
    return flat(ctx.resident_metrics('softmax', 0.1))


def r_input_grad(ctx, pr):
    return flat(ctx.input_grad(pr['Xp']))


def r_core_grad(ctx, pr):
    return flat(ctx.core_grad(pr['Xp']))


def r_core_grad_indices(ctx, pr):
    return flat(ctx.core_grad_indices(pr['idx']))


def r_log_norm_grad(ctx, pr):
    return flat(ctx.log_norm_grad(pr['S']))


def r_nll_grad(ctx, pr):
    return flat(ctx.nll_grad(pr['Xg'], pr['yg'], pr['S']))


def r_nll_eval(ctx, pr):
    return flat(ctx.nll_eval(pr['Xg'], pr['yg'], pr['S']))


def r_bond_spectra(ctx, pr):
    return flat(ctx.bond_spectra())


def r_inner(ctx, pr):
    return flat(ctx.inner(other_chain(pr, ctx.l_pos), ctx.l_pos), ctx.inner())


def r_sample(ctx, pr):
    return flat(ctx.sample(N_DRAW, pr['phi'], pr['w'], seed=7))


def r_sample_masked(ctx, pr):
    return flat(ctx.sample_masked(N_DRAW, pr['phi'], pr['w'], pr['mask'], pr['known'], seed=7, class_logw=True))


def r_site_conditionals(ctx, pr):
    return flat(ctx.site_conditionals(N_DRAW, pr['phi'], pr['w'], pr['mask'], pr['known']))


def r_update_B(ctx, pr):
    out, met = ctx.update_B(None, left_step(ctx), *HP[:6])
    return flat(out[:int(np.prod(merged_shape(ctx)))], met)


def l2_input(shape):
    """the merged tensor r_l2_term hands in, from its shape alone"""
    return np.random.default_rng(SEED + sum(shape)).random(shape).astype(np.float32)


def r_l2_term(ctx, pr):
    return flat(ctx.l2_term(l2_input(merged_shape(ctx)), left_step(ctx), HP[1]))


# name: (function, needs the f and the environments of a forward)
READERS = {
    'forward': (r_forward, False),
    'predict': (r_predict, False),
    'predict_scaled': (r_predict_scaled, False),
    'predict_indices': (r_predict_indices, False),
    'eval_indices': (r_eval_indices, False),
    'resident_metrics': (r_resident_metrics, True),
    'input_grad': (r_input_grad, False),
    'core_grad': (r_core_grad, False),
    'core_grad_indices': (r_core_grad_indices, False),
    'log_norm_grad': (r_log_norm_grad, False),
    'nll_grad': (r_nll_grad, False),
    'nll_eval': (r_nll_eval, False),
    'bond_spectra': (r_bond_spectra, False),
    'inner': (r_inner, False),
    'sample': (r_sample, False),
    'sample_masked': (r_sample_masked, False),
    'site_conditionals': (r_site_conditionals, False),
    'update_B': (r_update_B, True),
    'l2_term': (r_l2_term, False),
}
AFTER_FORWARD = tuple(k for k, v in READERS.items() if v[1])


# ---------------------------------------------------------------------------------------------------------------
# consumers
# ---------------------------------------------------------------------------------------------------------------
def sweep_plan(ctx):
    """(left_dir, n_steps, first_of_sweep) of the sweep to the end of the chain that l_pos allows"""
    l = ctx.l_pos
    if l == ctx.N - 1:
        return True, ctx.N - 1, True
    return False, ctx.N - 1 - l, l == 0


def c_sweep(ctx, pr):
    f0 = ctx.forward()
    met, f = ctx.sweep(*sweep_plan(ctx), *HP)
    return flat(f0, met, f, model_of(ctx))


def c_gd_step(ctx, pr):
    return flat(ctx.gd_step(pr['Xp'], pr['yp'], *GD), model_of(ctx))


def c_nll_step(ctx, pr):
    return flat(ctx.nll_step(pr['Xg'], pr['yg'], pr['S'], lr=1e-3, weight_dec=1e-3, renorm=True), model_of(ctx))


def c_compress(ctx, pr):
    return flat(ctx.compress(3), model_of(ctx))


CONSUMERS = {'sweep': c_sweep, 'gd_step': c_gd_step, 'nll_step': c_nll_step, 'compress': c_compress}
OPTIMISER_CALLS = ('gd_step', 'nll_step')
CALLS = tuple(READERS) + tuple(CONSUMERS)


def calls_of(shape):
    return tuple(c for c in CALLS if c not in LEFT_OUT[shape])


# ---------------------------------------------------------------------------------------------------------------
# verdicts
# ---------------------------------------------------------------------------------------------------------------
# (mutator, call): (the lines that carry the quantity, what it is).  A COMPLETE sweep with the L2 term leaves the norm environments
# behind it valid: every step formed the next one from the core it had just written, Nh_new = Cb^T (Nh x 1_d) Cb in the update
# kernel.  A fresh context contracts them from the cores in norm_chain_kernel: the same float64 numbers from the same float32 cores,
# summed in another order.  tnml_l2_term hands its float64 results out as they are, so the last bits show (observed: the loss one unit
# in the last place apart, 21 of 81 gradient elements at D = 3).  tnml_update_B and the sweep consumer read the same environments, but
# what they hand out cannot show it: the term enters B_new as 2 lr wd G, 2e-5 of a last-place change of G, and f as float32.
_COMPLETE_SWEEP_L2 = (
    'tnml_api.hip, finish_sweep: `behind = l2_flag && complete` keeps the norm stack behind a complete sweep valid; '
    'tnml_api.hip, norm_envs_for_label_site: builds only the stack that is not valid',
    'the float64 norm environments Ln (after a right sweep) the steps of the sweep formed one from the other')
CARRIED = {('sweep_right', 'l2_term'): _COMPLETE_SWEEP_L2, ('sweep_reference', 'l2_term'): _COMPLETE_SWEEP_L2}

# How much larger the error of the inherited route may be than that of the rebuilt one: both routes on the oracle itself, in float64
# against long double, shape A, the state a right sweep from the start state leaves, CARRIED_FACTOR_CASES merged tensors
# (tests/test_context_lifecycle_host.py computes it: the largest ratio either way, rounded up to one digit).
CARRIED_FACTOR, CARRIED_FACTOR_SEED, CARRIED_FACTOR_CASES = 4.0, SEED, 16

REMEDY = {'forward': 'forward', 'optimiser': 'optim_reset'}
REFUSAL_WORDS = {
    'resident_metrics': 'no f on the device',
    'update_B': 'the %s environments are not built for this batch',
    'gd_step': 'the optimiser state belongs to other bonds or another l_pos',
    'nll_step': 'the optimiser state belongs to other bonds or another l_pos',
}


def complete_sweep(mutator, D):
    """the mutator ends with a sweep that reached the other end of the chain (a sweep that stops inside leaves the stack behind it
    invalid, and the next call builds it as a fresh context does)"""
    return mutator == 'sweep_right' or (mutator == 'sweep_reference' and reference_steps(D) == N - 1)


def verdict(mutator, call, D=2):
    """-> (verdict, remedy or None, citation or None) on a shape of feature dimension D"""
    if (mutator, call) in CARRIED and complete_sweep(mutator, D):
        return 'carried', None, CARRIED[(mutator, call)]
    # A changed model or batch leaves no f and no environments (include/tnml.h, tnml_scale_cores / tnml_gd_train_indices "AFTER a
    # call ..." / tnml_select_indices).  A sweep leaves its f, and the stack ahead of it: resident_metrics runs on that f, update_B
    # continues behind a sweep that stopped inside the chain, but behind a complete one the step turns round and the stack of the
    # other direction was never built.  New labels and the switches leave the forward of before.
    if call in AFTER_FORWARD:
        if changes(mutator) in ('model', 'batch') and mutator not in SWEEPS:
            return 'refused', REMEDY['forward'], None
        if call == 'update_B' and complete_sweep(mutator, D):
            return 'refused', REMEDY['forward'], None
    # vel / m / v are bound to the bonds and l_pos of the last reset (include/tnml.h, STATE of tnml_optim_config)
    if call in OPTIMISER_CALLS and rebinds(mutator):
        return 'refused', REMEDY['optimiser'], None
    return 'equal', None, None


SCALE_INVARIANT = ('sample', 'sample_masked', 'site_conditionals', 'nll_eval')
GAUGE_DEPENDENT = ('core_grad', 'core_grad_indices', 'log_norm_grad', 'nll_grad') + tuple(CONSUMERS)
RESIDENT = ('forward', 'resident_metrics', 'update_B', 'sweep')


def sensitive(mutator, call):
    """the mutator must change what the call returns"""
    what = changes(mutator)
    if what == 'model':
        if mutator == 'scale_cores':
            return call not in SCALE_INVARIANT                     # the Born distribution does not see a common factor
        if mutator == 'orthogonalize':
            return call in GAUGE_DEPENDENT                         # f and every gauge-invariant number change in rounding at most
        return True
    if what == 'batch':
        return call in RESIDENT
    if what == 'labels':
        return call in RESIDENT and call != 'forward'
    return False                                                   # the scaled chains agree with the plain ones to rounding


# ---------------------------------------------------------------------------------------------------------------
# the float64 oracle of the sweep consumer (for carried pairs, and the factor)
# ---------------------------------------------------------------------------------------------------------------
def oracle_sweep_from(pr, cores, l_pos, X, y, inherit=None):
    """f after the sweep of c_sweep from (cores, l_pos) on (X, y) by mo.sweep_step; inherit: norm environments (Ln, Rn) to start with"""
    st = mo.MPSState(N, pr['D'], L, M, [np.asarray(a, np.float64) for a in cores], l_pos)
    if inherit is not None:
        st.Ln, st.Rn = dict(inherit[0]), dict(inherit[1])
    Lenv, Renv, f = label_inside_forward(st.cores, l_pos, X)
    place(st, X, Lenv, Renv)
    left = l_pos == N - 1
    y1h = mo.one_hot(y, L)
    for _ in range(N - 1 if left else N - 1 - l_pos):
        f = mo.sweep_step(st, f, y1h, HP[0], HP[1], L2_flag=HP[2], left_dir=left, act_fn=HP[3], loss_fn=HP[4], T=HP[5], trunc=HP[6])
    return f, st


# ---------------------------------------------------------------------------------------------------------------
# the oracle of tnml_l2_term in long double, and the two float64 routes to its norm environments
# ---------------------------------------------------------------------------------------------------------------
def norm_env(cores, sites, dtype, route='rebuilt'):
    """the norm environment over `sites` (in contraction order; cores without a label axis), left to right or right to left.
    route 'rebuilt': mo.norm_env_left / norm_env_right's expression; 'inherited': the two products of the update kernel,
    T2 = (Nh x 1_d) Cb, then Cb^T T2"""
    env = np.ones((1, 1), dtype=dtype)
    if not sites:
        return env
    rightwards = sites[0] < sites[-1] or len(sites) == 1 and sites[0] == 0
    for k in sites:
        c = np.asarray(cores[k], dtype=dtype)
        if not rightwards:
            c = c.transpose(2, 1, 0)                                # (mr, D, ml): the same expression from the other end
        if route == 'rebuilt':
            env = np.einsum('adc,ae,edf->cf', c, env, c)
        else:
            env = np.einsum('adc,adf->cf', c, np.einsum('ae,edf->adf', env, c))
    return env


def l2_oracle(cores, l_pos, B, weight_dec, dtype=np.longdouble, route='rebuilt'):
    """(loss, grad) of mo.compute_L2_reg for the merged tensor at the label site, in `dtype`; the weight decay is the float32 the
    call receives"""
    weight_dec = dtype(np.float32(weight_dec))
    left = l_pos == N - 1
    p = l_pos - 1 if left else l_pos
    Ln = norm_env(cores, list(range(p)), dtype, route)
    Rn = norm_env(cores, list(range(N - 1, p + 1, -1)), dtype, route)
    G = np.einsum('ae,axycl,cf->exyfl', Ln, np.asarray(B, dtype=dtype), Rn)
    return weight_dec * np.sum(np.asarray(B, dtype=dtype) * G), 2 * weight_dec * G


def l2_error(got, ref):
    """the larger of the loss's relative error and the gradient's, relative to max|gradient|"""
    (loss, grad), (loss_o, grad_o) = got, ref
    e_loss = abs(np.longdouble(loss) - loss_o) / abs(loss_o)
    e_grad = np.abs(np.asarray(grad, np.longdouble).reshape(grad_o.shape) - grad_o).max() / np.abs(grad_o).max()
    return float(max(e_loss, e_grad))
