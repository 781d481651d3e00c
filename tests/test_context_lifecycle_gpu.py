"""Every call after every state change against a fresh context, bit for bit.

A tnml_ctx holds a dozen validity flags and tickets (envs_valid_L/R, Ln/Rn_valid, f_current, Bnew_valid, the pre-gradient tickets, the
hand-off sequence numbers, the optimiser binding) and about fifteen capacity groups that grow on demand; a dozen entry points change
the model or the batch under them, each with its own list of what it invalidates.  The oracle here needs no tolerance: the same call
on a fresh context that was handed the same cores (get_cores -> set_cores) and the same batch must return the same bits.

One case = one (shape, mutator) of tests/context_lifecycle_cases.py:
  (a) a long-lived context at the start state runs every reader and every consumer once (every capacity group exists; the results
      must already equal those of a fresh context), the start state restored after each consumer.  Then its caches are FILLED at
      the start state: forward, update_B and l2_term with the L2 term (both norm stacks valid), forward again (environment stack
      and resident f current) -- every flag a mutator has to clear is set when the mutator runs;
  (b) the mutator; get_cores() and the batch are noted;
  (c) every reader on the long-lived context and on ONE fresh context with the same constructor arguments, switches, optimiser,
      dataset, cores and batch: np.array_equal on every output, shapes and dtypes included.  resident_metrics and update_B come
      first, on exactly what the mutator left.  Where the table says 'refused' (a changed model or batch; update_B behind a
      complete sweep, whose step turns round) BOTH refusals are asserted with code and words before the one forward that is their
      remedy; where it says 'equal' (a sweep leaves its f and the stack ahead, new labels and the switches leave the forward of
      before) they run without a forward on the long-lived side, the fresh context given a forward and the same f by set_f.  After
      the whole battery get_cores() and the resident f of the long-lived context are what they were;
  (d) every consumer, the first directly on the mutated state (which one comes first rotates with the mutator), the others after a
      set_cores of the noted cores, each against a fresh context of its own.  The optimiser state is part of a step's definition:
      behind a stateful mutator (gd_step with momentum, gd_step with Adam, nll_step) BOTH gd_step and nll_step run on the state
      that step left -- where they are not first, the long-lived context takes the mutator's step again from the start state --
      and the fresh side replays both steps.  Behind a mutator that changed bonds or l_pos both refusals are asserted before the
      optim_reset;
  (e) for pairs marked sensitive the result must differ from the one at the start state (a fresh context per shape, computed once);
  (f) both contexts are closed and the case prints how many pairs were equal, refused and carried: they add up to every call.
'carried' pairs (tnml_l2_term behind a complete sweep: the norm environments
the sweep's steps formed one from the other, against the ones a fresh context contracts from the cores) hold both sides to the oracle
of the call (mo.compute_L2_reg's expression, in long double) within the bound tests/test_feature_dim_gpu.py asserts for the call, and
the long-lived error to CARRIED_FACTOR times the fresh one.

test_the_readme_workflow_on_one_context runs sweep right, sweep left, two Adam steps, orthogonalize, compress(3), axpby, compress(4),
two likelihood steps, a batch of 70, forward + sweep, a segment and every reader on ONE context per shape, and compares forward's f
and core_grad with a fresh context after every stage.

Shapes: N = 8, L = 3, bonds (2, 4, 4, 3, 4, 4, 2), M = 12, capacity 37, batches of 37 / 70 / 5 -- the smallest at which padding, growth
and shrinking occur; D = 2 on the persistent (1 and 2), per-step and large-tensor paths, D = 3 on the generic path.

Observed on an MI355X: of the 95 x 23 = 2185 pairs 1973 are bit-equal, 206 are refused as documented and bit-equal behind the
remedy, every sensitive pair changed.  Six pairs differ, all of them tnml_l2_term behind a COMPLETE sweep (sweep_right on every
shape, sweep_reference at D = 3), in the last place of its float64 results (the loss 6.9e-18 of 0.042 apart, 21 of 81 gradient
elements at D = 3): the norm environments such a sweep leaves valid were formed step by step in the update kernel, a fresh context
contracts them in norm_chain_kernel.  A tnml_scale_cores(1.0) in between makes those pairs bit-equal; they
are the 'carried' list (errors against the long-double oracle 1.4e-16 to 1.5e-15 on both sides, ratios 0.75 to 1.5).  A sweep that
stops inside the chain leaves that stack invalid and is bit-equal, update_B continues behind it bit-equal to a fresh segment start
from the same f, and so is a sweep behind a sweep on every path.  In the workflow the segment starts behind a whole left sweep and
inherits ITS stack: l2_term is compared only behind stages that leave no such stack (L2_INHERITED).  A case takes 0.12 to 0.22 s
(the first of a shape 0.5 s), the file 12 to 16 s.

What the tests notice, tried once each with a build that leaves one invalidation out: cores_changed without Ln_valid / Rn_valid --
all nine model mutators that go through it (set_cores, set_cores_bonds, scale_cores, both gd_steps, nll_step, orthogonalize,
compress_to_3, axpby) fail on all five shapes, and the five workflow tests; batch_changed without f_current -- the four batch
mutators fail on all five shapes (resident_metrics is not refused); tnml_scale_cores without its cores_changed -- scale_cores
fails on all five shapes.  Not populated: the pre-gradient tickets (only a sweep step sets them, and it moves the model).
"""
import os
import sys
import time

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p_ in (ROOT, HERE):
    if p_ not in sys.path:
        sys.path.insert(0, p_)

import context_lifecycle_cases as lc                               # noqa: E402
from tensornetworkforml_amd import _hip                            # noqa: E402
from test_feature_dim_gpu import L2_TERM_TOL                      # noqa: E402

pytestmark = pytest.mark.gpu

MUTATOR_NAMES = list(lc.MUTATORS)


def same(a, b):
    """two tuples of arrays: lengths, dtypes, shapes and values (a NaN equals nothing)"""
    return len(a) == len(b) and all(x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y, equal_nan=False)
                                    for x, y in zip(a, b))


def first_difference(a, b):
    if len(a) != len(b):
        return 'outputs %d / %d' % (len(a), len(b))
    for k, (x, y) in enumerate(zip(a, b)):
        if x.dtype != y.dtype or x.shape != y.shape:
            return 'output %d: %s %s / %s %s' % (k, x.dtype, x.shape, y.dtype, y.shape)
        if not np.array_equal(x, y, equal_nan=False):
            d = np.abs(x.astype(np.float64) - y.astype(np.float64))
            return 'output %d: %d of %d elements differ, max |.| %.3g of %.3g' % (k, int((x != y).sum()), x.size, np.nanmax(d),
                                                                                  np.nanmax(np.abs(y.astype(np.float64))))
    return None


def new_live(pr):
    return lc.Live(_hip.Context(pr['N'], pr['D'], pr['L'], pr['M'], pr['capacity']), pr)


def twin_of(live, cores, l_pos):
    """a fresh context with the constructor arguments, switches, optimiser and dataset of `live`, given its cores and its batch"""
    t = new_live(live.pr)
    for method, arg in live.switches:
        if (method, arg) not in live.pr['calls']:
            t.switch(method, arg)
    if t.optim != live.optim:
        t.configure(**live.optim)
    t.ctx.set_cores(cores, l_pos)
    live.mirror_batch(t)
    return t


def refusal(call):
    with pytest.raises(_hip.TnmlError) as ei:
        call()
    return ei.value.code, str(ei.value).split(': ', 1)[1]


def expect_refusal(live, name, fn):
    code, msg = refusal(lambda: fn(live.ctx, live.pr))
    words = lc.REFUSAL_WORDS[name]
    if '%s' in words:
        words = words % ('left' if lc.left_step(live.ctx) else 'right')
    assert code == lc.STATE and msg.startswith(words), (name, code, msg)


_start = {}


def start_results(shape):
    """every call of the shape at the start state, each on a context that saw nothing else of the battery before it but readers"""
    if shape not in _start:
        pr, out = lc.problem(shape), {}
        t = new_live(pr)
        lc.start(t)
        for name in lc.calls_of(shape):
            if name in lc.READERS:
                fn, after_forward = lc.READERS[name]
                if after_forward:
                    t.ctx.forward(want_f=False)
                out[name] = fn(t.ctx, pr)
        t.ctx.close()
        for name in lc.calls_of(shape):
            if name in lc.CONSUMERS:
                t = new_live(pr)
                lc.start(t)
                out[name] = lc.CONSUMERS[name](t.ctx, pr)
                t.ctx.close()
        _start[shape] = out
    return _start[shape]


def populate(live):
    """the caches of the start state filled: both norm stacks valid (update_B and l2_term with the L2 term), the environment stack
    and the resident f of a forward.  What a mutator must clear is set when it runs."""
    live.ctx.forward(want_f=False)
    lc.r_update_B(live.ctx, live.pr)
    lc.r_l2_term(live.ctx, live.pr)
    live.ctx.forward(want_f=False)


def warm(live, shape, bad):
    """(a): every reader and consumer once on the long-lived context at the start state, then the start state with its caches filled"""
    pr, ref = live.pr, start_results(shape)
    lc.start(live)
    for name in lc.calls_of(shape):
        if name in lc.READERS:
            fn, after_forward = lc.READERS[name]
            if after_forward:
                live.ctx.forward(want_f=False)
            got = fn(live.ctx, pr)
        else:
            live.ctx.optim_reset()
            got = lc.CONSUMERS[name](live.ctx, pr)
            lc.start(live)
        if not same(got, ref[name]):
            bad.append(('warm-up', name, first_difference(got, ref[name])))
    live.configure(**lc.OPTIM_START)                                 # zero state, bound to the start bonds
    lc.start(live)
    populate(live)


def carried_l2_term(live, got, want, cores, l_pos, what, bad):
    """both results of r_l2_term against the long-double oracle from the same cores"""
    ref = lc.l2_oracle(cores, l_pos, lc.l2_input(lc.merged_shape(live.ctx)), lc.HP[1])
    e_long, e_fresh = lc.l2_error(got, ref), lc.l2_error(want, ref)
    print('    carried %s: loss and gradient against the oracle: long-lived %.3e, fresh %.3e' % (what, e_long, e_fresh))
    if not (e_long < L2_TERM_TOL and e_fresh < L2_TERM_TOL and e_long <= lc.CARRIED_FACTOR * e_fresh):
        bad.append((what, 'carried', e_long, e_fresh))


def mutate(live, mutator, index):
    lc.MUTATORS[mutator][0](live, np.random.default_rng(lc.SEED + index))


@pytest.mark.parametrize('mutator', MUTATOR_NAMES)
@pytest.mark.parametrize('shape', list(lc.SHAPES))
def test_every_call_after_a_mutator_equals_a_fresh_context(shape, mutator):
    t0 = time.perf_counter()
    pr = lc.problem(shape)
    index = MUTATOR_NAMES.index(mutator)
    calls = lc.calls_of(shape)
    before = start_results(shape)
    bad, count, n_sensitive = [], dict(equal=0, refused=0, carried=0), 0
    live = new_live(pr)
    warm(live, shape, bad)                                            # (a)
    mutate(live, mutator, index)                                      # (b)
    cores, bond, l_pos = live.ctx.get_cores()
    model = lc.model_of(live.ctx)

    def judge(name, got, want, where=''):
        nonlocal n_sensitive
        kind = lc.verdict(mutator, name, pr['D'])[0]
        if kind == 'carried':
            assert name == 'l2_term', 'the one carried call'
            carried_l2_term(live, got, want, cores, l_pos, (mutator, name), bad)
        elif not same(got, want):
            bad.append((name, where, 'long-lived / fresh', first_difference(got, want)))
        count[kind] += 1
        if lc.sensitive(mutator, name):
            n_sensitive += 1
            if same(got, before[name]):
                bad.append((name, 'the mutator did not change the result'))

    # (c) readers.  First the two that read the f and the environments of the resident batch, on what the mutator left: refused,
    # both of them, before the one forward that is their remedy -- or, where the table says 'equal' (a sweep leaves its f, a switch
    # or new labels leave the forward of before), run on that very state, the fresh context given a forward and the same f
    fresh = twin_of(live, cores, l_pos)
    lead = [r for r in lc.AFTER_FORWARD if r in calls]
    pending = []
    fresh_ready = False
    for name in lead:
        fn = lc.READERS[name][0]
        if lc.verdict(mutator, name, pr['D'])[0] == 'refused':
            expect_refusal(live, name, fn)
            pending.append(name)
        else:
            if not fresh_ready:
                fresh.ctx.forward(want_f=False)
                fresh.ctx.set_f(live.ctx.get_f())
                fresh_ready = True
            judge(name, fn(live.ctx, pr), fn(fresh.ctx, pr), 'on the state the mutator left')
    f_resident = None
    for name in ['forward'] + pending + [r for r in calls if r in lc.READERS and r not in lead and r != 'forward']:
        fn = lc.READERS[name][0]
        judge(name, fn(live.ctx, pr), fn(fresh.ctx, pr))
        if name == 'forward':
            f_resident = live.ctx.get_f()
    fresh.ctx.close()
    if not same((f_resident,), (live.ctx.get_f(),)):                  # after the whole battery
        bad.append(('get_f', 'the readers moved the resident f'))
    if not same(model, lc.model_of(live.ctx)):
        bad.append(('get_cores', 'the readers moved the model', first_difference(model, lc.model_of(live.ctx))))

    # (d) consumers
    names = [c for c in calls if c in lc.CONSUMERS]
    names = names[index % len(names):] + names[:index % len(names)]
    for name in names:                                                # vel / m / v bound to other bonds: both calls, before the reset
        if name in lc.OPTIMISER_CALLS and lc.verdict(mutator, name, pr['D'])[0] == 'refused':
            expect_refusal(live, name, lc.CONSUMERS[name])
    for k, name in enumerate(names):
        fn = lc.CONSUMERS[name]
        assert lc.verdict(mutator, name, pr['D'])[0] != 'carried', 'no consumer is carried'
        replay = lc.stateful(mutator) and name in lc.OPTIMISER_CALLS
        if replay and k:                                              # the state the mutator's step left, again: the step itself, again
            lc.start(live)
            live.ctx.optim_reset()
            mutate(live, mutator, index)
            if not same(model, lc.model_of(live.ctx)):
                bad.append((name, 'the mutator, repeated from the start state, gave other cores'))
        elif k:
            live.ctx.set_cores(cores, l_pos)
        if name in lc.OPTIMISER_CALLS and not replay:
            live.ctx.optim_reset()
        got = fn(live.ctx, pr)
        if replay:                                                    # the fresh side takes the mutator's step too, from the start state
            fresh = new_live(pr)
            lc.start(fresh)
            mutate(fresh, mutator, index)
        else:
            fresh = twin_of(live, cores, l_pos)
        judge(name, got, fn(fresh.ctx, pr), 'first' if k == 0 else ('replayed' if replay else 'restored'))
        fresh.ctx.close()
    live.ctx.close()                                                  # (f)
    print('%s %-24s %d pairs equal, %d refused, %d carried, %d sensitive; bonds %s l_pos %d; %.2f s'
          % (shape, mutator, count['equal'], count['refused'], count['carried'], n_sensitive, list(map(int, bond)), l_pos,
             time.perf_counter() - t0))
    assert not bad, bad
    assert sum(count.values()) == len(calls)
    assert count['refused'] == sum(lc.verdict(mutator, c, pr['D'])[0] == 'refused' for c in calls)


# ---------------------------------------------------------------------------------------------------------------
# the workflow of the README on one context
# ---------------------------------------------------------------------------------------------------------------
def whole_sweep(live):
    live.ctx.forward(want_f=False)
    live.ctx.sweep(*lc.sweep_plan(live.ctx), *lc.HP, want_metrics=False, want_f=False)


def adam_steps(live):
    live.configure(kind='adam', clip=False)
    for _ in range(2):
        live.ctx.gd_step(live.pr['Xp'], live.pr['yp'], 1e-3, *lc.GD[1:])


def nll_steps(live):
    live.ctx.optim_reset()
    for _ in range(2):
        live.ctx.nll_step(live.pr['Xg'], live.pr['yg'], live.pr['S'], lr=1e-3, weight_dec=0.0, renorm=True)


def segment(live):
    """back to site 0 by a left sweep, then three steps right with the label allowed inside"""
    whole_sweep(live)
    lc.m_segment(live, None)


def all_readers(live):
    for name, (fn, after_forward) in lc.READERS.items():
        if name in lc.calls_of(live.pr['shape']):
            if after_forward:
                live.ctx.forward(want_f=False)
            fn(live.ctx, live.pr)


STAGES = [
    ('sweep right', whole_sweep), ('sweep left', whole_sweep), ('gd_step x 2', adam_steps),
    ('orthogonalize', lambda v: v.ctx.orthogonalize()), ('compress(3)', lambda v: v.ctx.compress(3)),
    ('axpby', lambda v: lc.m_axpby(v, None)), ('compress(4)', lambda v: v.ctx.compress(4)), ('nll_step x 2', nll_steps),
    ('batch 70', lambda v: v.load('input', 70)), ('forward + sweep right', whole_sweep), ('segment', segment),
    ('every reader', all_readers),
]


# stages behind which a norm stack is the one a complete sweep left (the segment starts behind a whole left sweep and builds only the
# stack that is not valid; reading changes nothing)
L2_INHERITED = ('sweep right', 'sweep left', 'forward + sweep right', 'segment', 'every reader')


@pytest.mark.parametrize('shape', list(lc.SHAPES))
def test_the_readme_workflow_on_one_context(shape):
    t0 = time.perf_counter()
    pr = lc.problem(shape)
    live = new_live(pr)
    lc.start(live)
    bad = []
    for stage, fn in STAGES:
        fn(live)
        cores, bond, l_pos = live.ctx.get_cores()
        fresh = twin_of(live, cores, l_pos)
        # forward and core_grad, and behind the forward the two calls that read the norm stacks (l2_term where no complete sweep
        # left one of them valid: those pairs are the carried ones)
        names = ['forward', 'core_grad', 'update_B'] + ([] if stage in L2_INHERITED else ['l2_term'])
        for name in names:
            got, want = lc.READERS[name][0](live.ctx, pr), lc.READERS[name][0](fresh.ctx, pr)
            if not same(got, want):
                bad.append((stage, name, first_difference(got, want)))
            assert all(np.isfinite(x).all() for x in got), (stage, name)
        fresh.ctx.close()
        print('%s %-22s bonds %s l_pos %d' % (shape, stage, list(map(int, bond)), l_pos))
    live.ctx.close()
    print('%s workflow: %.2f s' % (shape, time.perf_counter() - t0))
    assert not bad, bad
