"""The staged-batch hand-over (tnml_stage_batch / tnml_select_batch) and batch-size histories, bit for bit.

bench.py puts select_batch in front of every timed pass: four staged batches in rotation, no host wait between the sweep before and
the forward behind.  select_batch(slot) and set_input(X, y) with the same arrays run the same re-tiling kernel into the same
buffers, so everything downstream must be EQUAL, bit for bit: every comparison between two contexts below is an equality of uint32
views (bits / same_bits of tests/test_orthogonalize_gpu.py).  The only inequalities are the two bounds tests/test_hip_parity.py uses
for the same calls against the float64 oracle (forward 1e-4, f after a sweep 1e-3 of max|f|), applied to the first pass of every
configuration: a hand-over wrong in both contexts alike would otherwise go unseen.

  1  rotation          8 passes over the slots (70, 300, 7, 130), capacity 70 (slot 1 grows the batch group through select_batch),
                       against a twin that calls set_input; f, metrics, core slots, bonds, l_pos after every pass, the environment
                       stack of the first round; all eight configurations of tests/batch_handover_cases.py
  2  no host wait      the benchmark's timed loop (nothing handed back, no synchronising call) against the same loop with a
                       synchronisation after every call: persistent sweep in one and in three launches, the two-stream large-tensor
                       step, the one-rank communicator
  3  size histories    16 -> 300 -> 7 samples through a context created for 16 against contexts created for 300 that see one batch
  4  slots             re-staging, staging a resident slot, two slots alike, all eight slots, labels, a dataset in between
  5  state, refusals   TNML_ERR_STATE / TNML_ERR_ARG leave the resident batch, f, the cores and the slot as they were

tests/test_batch_handover_host.py shows with the oracle alone that the batches differ by what is compared here.
Measured on an MI355X: the 42 tests of this file take 12 s, 7 s of them the first RCCL communicator of the process.

What the tests found when they first ran: the twins of the persistent-sweep configurations differed in the padding of the label
buffer that tnml_get_core_slots hands out (test 1 at its first pass, and the tests of 4 and 5 that compare core slots).  The two label
buffers were never initialised and a sweep step writes the elements of its label core alone; tnml_create zeroes them now.  f,
metrics, bonds and the cores proper were equal throughout; tests 2 and 3 passed as they stood.

What the tests notice, tried once each with a build that leaves one piece of the hand-over out: a re-tiling kernel that does not
zero-fill [b, b_pad) fails test 1 on 'shape' (non-finite values), test 2 on 'comm' and the resident-slot test of 4 -- those sweeps
do not mask the samples behind b, the zero-fill is what they rely on.  Two pieces are not needed by whole sweeps and go unnoticed
here: clearing the labels behind b (the kernels mask them) and dropping the pre-gradient tickets in select_batch (a whole sweep
ends without one that the next could take, and the segment start behind a select in the middle of a sweep takes none either:
test_select_in_the_middle_of_a_sweep passes with and without the drop).
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p_ in (ROOT, HERE):
    if p_ not in sys.path:
        sys.path.insert(0, p_)

import batch_handover_cases as bc                                  # noqa: E402
from test_any_position_host import random_cores_at                 # noqa: E402
from tensornetworkforml_amd import _hip                            # noqa: E402
from tensornetworkforml_amd import dist as tdist                   # noqa: E402

pytestmark = pytest.mark.gpu

ARG, STATE = -1, -2
S_L, S_R = _hip.SIDE_LEFT, _hip.SIDE_RIGHT
FWD_TOL, SWEEP_TOL = 1e-4, 1e-3                                     # tests/test_hip_parity.py, against the float64 oracle


def _code(call):
    with pytest.raises(_hip.TnmlError) as ei:
        call()
    return ei.value.code


def relerr(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    assert a.shape == ref.shape, (a.shape, ref.shape)
    return float(np.abs(a - ref).max() / max(np.abs(ref).max(), 1e-300))


def u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same(a, b):
    """two float32 arrays, bit for bit"""
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype == np.float32 and a.shape == b.shape and np.array_equal(u32(a), u32(b))


def bits(ctx):
    slots, lab = ctx.core_slots()
    return slots.view(np.uint32).copy(), lab.view(np.uint32).copy(), [int(v) for v in ctx.get_cores()[1]], ctx.l_pos


def same_bits(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2] and a[3] == b[3]


def new_ctx(c, capacity, monkeypatch, cores=None, l_pos=0):
    """a context of configuration c on its launch path, with the configuration's cores (or the ones given)"""
    monkeypatch.setenv('TNML_FORCE_COMM', '1' if c['comm'] else '0')
    ctx = _hip.Context(c['N'], c['D'], c['L'], c['M'], capacity)
    for method, arg in c['calls']:
        getattr(ctx, method)(arg)
    ctx.set_cores(c['cores'] if cores is None else cores, l_pos)
    if c['comm']:
        tdist.attach_comm(ctx, 0, 1)
    return ctx


def envs(ctx):
    """the stack forward built, site by site"""
    N = ctx.N
    return [ctx.get_env(S_R, i) for i in range(1, N)] if ctx.l_pos == 0 else [ctx.get_env(S_L, i) for i in range(N - 1)]


def one_pass(ctx, load, want_env=False):
    """bench.py's one_pass with everything handed back: (f of forward, metrics, f of the sweep, state bits[, environments])"""
    load()
    f0 = ctx.forward()
    env = envs(ctx) if want_env else None
    left = ctx.l_pos == ctx.N - 1
    met, f1 = ctx.sweep(left, ctx.N - 1, True, *bc.HP)
    return dict(b=ctx.b, f0=f0, met=met, f1=f1, state=bits(ctx), env=env)


def assert_same_pass(a, b, what):
    assert a['b'] == b['b'], what
    assert same(a['f0'], b['f0']), (what, 'f of forward')
    assert same(a['met'], b['met']), (what, 'metrics')
    assert same(a['f1'], b['f1']), (what, 'f of the sweep')
    assert same_bits(a['state'], b['state']), (what, 'cores, bonds, l_pos')
    assert (a['env'] is None) == (b['env'] is None)
    if a['env'] is not None:
        assert len(a['env']) == len(b['env']) and all(same(x, y) for x, y in zip(a['env'], b['env'])), (what, 'environments')
    assert np.isfinite(a['f0']).all() and np.isfinite(a['f1']).all() and np.isfinite(a['met']).all(), what


def loader(ctx, how, k, X, y):
    return (lambda: ctx.select_batch(k)) if how == 'select' else (lambda: ctx.set_input(X, y))


def stage_all(ctx, batches):
    for k, (X, y) in enumerate(batches):
        ctx.stage_batch(k, X, y)


# ---------------------------------------------------------------------------------------------------------------
# 1. rotation equals set_input, pass by pass
# ---------------------------------------------------------------------------------------------------------------
N_PASSES = 8


def rotation(c, how, monkeypatch):
    """8 passes over the four batches in a context created for 70 samples; the results of every pass"""
    ctx = new_ctx(c, bc.SIZES[0], monkeypatch)
    if how == 'select':
        stage_all(ctx, c['batches'])
    out = []
    for p in range(N_PASSES):
        k = p % len(c['batches'])
        X, y = c['batches'][k]
        ctx.profile_reset()
        out.append(one_pass(ctx, loader(ctx, how, k, X, y), want_env=p < len(c['batches'])))
        cnt = ctx.counters()                                        # the library's account of the sweep: which path it took
        assert cnt['sweep_steps'] == ctx.N - 1, cnt
        out[-1]['persistent'] = cnt['launches'] == 1 and cnt['pipelined_steps'] == ctx.N - 1
        assert out[-1]['persistent'] or cnt['launches'] >= ctx.N - 1, cnt
        if c['name'] == 'shape':
            out[-1]['fixed'] = ctx.fixed_shape_steps()
    ctx.close()
    return out


@pytest.mark.parametrize('name', list(bc.CONFIGS))
def test_rotation_equals_set_input_pass_by_pass(name, monkeypatch):
    c = bc.case(name)
    got = rotation(c, 'select', monkeypatch)
    twin = rotation(c, 'set_input', monkeypatch)
    # the first pass of the configuration against the float64 oracle
    f0_o, f1_o, _ = bc.oracle_first_pass(name, 0)
    e0, e1 = relerr(got[0]['f0'], f0_o), relerr(got[0]['f1'], f1_o)
    print('%s: first pass against the oracle: forward %.2e, f after the sweep %.2e' % (name, e0, e1))
    assert e0 < FWD_TOL and e1 < SWEEP_TOL
    for p in range(N_PASSES):
        assert got[p]['b'] == bc.SIZES[p % 4]
        assert_same_pass(got[p], twin[p], (name, 'pass', p))
        if c['D'] == 2:                                             # one launch per sweep where the configuration says so, and only there
            assert got[p]['persistent'] == twin[p]['persistent'] == (name in ('persist', 'persist3', 'shape')), (name, p)
        if name == 'shape':                                         # the compiled-shape body really ran behind a selected batch
            assert got[p]['fixed'] > 0 and got[p]['fixed'] == twin[p]['fixed'], (p, got[p]['fixed'])


# ---------------------------------------------------------------------------------------------------------------
# 2. no host wait between passes
# ---------------------------------------------------------------------------------------------------------------
def timed_loop(c, sync, capacity, monkeypatch):
    """bench.py's timed loop at a small shape"""
    ctx = new_ctx(c, capacity, monkeypatch)
    stage_all(ctx, c['batches'])
    wait = ctx.synchronize if sync else (lambda: None)
    wait()
    for p in range(N_PASSES):
        ctx.select_batch(p % len(c['batches']))
        wait()
        ctx.forward(want_f=False)
        wait()
        left = ctx.l_pos == ctx.N - 1                               # host bookkeeping: nothing waits
        ctx.sweep(left, ctx.N - 1, True, *bc.HP, want_metrics=False, want_f=False)
        wait()
    ctx.synchronize()                                               # (reads the status word too: a failed SVD raises here)
    state = bits(ctx)
    f = ctx.forward()
    ctx.close()
    return state, f


@pytest.mark.parametrize('capacity', [300, 70])
@pytest.mark.parametrize('name', ['persist', 'persist3', 'large', 'comm'])
def test_no_host_wait_between_passes(name, capacity, monkeypatch):
    """Shows whether a select overtakes a reader of X or y on another stream of the context.  Capacity 300: no select has to grow
    the batch group, so nothing waits at all between the first select and the end; capacity 70: the passes of test 1, where the
    second select grows the group (and waits once) and seven hand-overs follow without a wait."""
    c = bc.case(name)
    free, f_free = timed_loop(c, False, capacity, monkeypatch)
    held, f_held = timed_loop(c, True, capacity, monkeypatch)
    assert same_bits(free, held), name
    assert same(f_free, f_held) and np.isfinite(f_free).all(), name


# ---------------------------------------------------------------------------------------------------------------
# 3. history leaves nothing behind
# ---------------------------------------------------------------------------------------------------------------
HISTORY = (16, 300, 7)


def single_pass(c, how, X, y, cores, l_pos, monkeypatch):
    ctx = new_ctx(c, max(HISTORY), monkeypatch, cores, l_pos)
    if how == 'select':
        ctx.stage_batch(0, X, y)
    r = one_pass(ctx, loader(ctx, how, 0, X, y))
    r['cores'] = ctx.get_cores()
    r['resident'] = ctx.resident_metrics('softmax', 0.1)
    ctx.close()
    return r


@pytest.mark.parametrize('how', ['set_input', 'select'])
@pytest.mark.parametrize('name', ['persist', 'per_step', 'large', 'anyd', 'shape'])
def test_history_leaves_nothing_behind(name, how, monkeypatch):
    """Context A is created for 16 samples and sees 16, 300 and 7; its 300 pass (the growth) and its 7 pass (under the grown
    capacity, behind the padding of 300) must equal, bit for bit, the pass of a context B created for 300 that is given A's cores
    of that moment (get_cores / set_cores) and this one batch.

    Why B may be compared: nothing but b and sizes derived from the capacity enters the launch plan.  size_batch_group
    (tnml_api.hip) sets b_pad, nblk_cap and pipe.tpw / nwide / ngroups from the capacity alone, and A's capacity after its growth is
    B's; the planners read the sample tiles as b_pad / kTS (SweepCall.nblk in sweep_impl, w.ntiles in fill_wide_pipe, ntiles and tpw
    in sweep_persist) and the samples as c->b.  What differs between A and B is what the buffers held before, which is what this
    test is about; the cores are compared as get_cores returns them, since the padding of A's slots holds earlier bonds.
    Both ways of loading run for every configuration.  'shape' is here because its sweep does not mask the samples behind b: with a
    re-tiling kernel that left [b, b_pad) as it was, that configuration ran into non-finite values (tried once with such a build)."""
    c = bc.case(name, HISTORY)
    A = new_ctx(c, HISTORY[0], monkeypatch)
    if how == 'select':
        stage_all(A, c['batches'])
    for k, (X, y) in enumerate(c['batches']):
        start, _, lp = A.get_cores()
        a = one_pass(A, loader(A, how, k, X, y))
        a['cores'] = A.get_cores()
        a['resident'] = A.resident_metrics('softmax', 0.1)
        if k == 0:
            continue
        b = single_pass(c, how, X, y, start, lp, monkeypatch)
        what = (name, how, 'b', HISTORY[k])
        assert a['b'] == b['b'] == HISTORY[k]
        assert same(a['f0'], b['f0']), (what, 'f of forward')
        assert same(a['met'], b['met']), (what, 'metrics')
        assert same(a['f1'], b['f1']), (what, 'f of the sweep')
        assert a['cores'][2] == b['cores'][2] and np.array_equal(a['cores'][1], b['cores'][1]), what
        assert all(same(x, y_) for x, y_ in zip(a['cores'][0], b['cores'][0])), (what, 'cores')
        assert a['resident'] == b['resident'], (what, 'resident_metrics')
        assert np.isfinite(a['f1']).all()
    A.close()


# ---------------------------------------------------------------------------------------------------------------
# 4. slots
# ---------------------------------------------------------------------------------------------------------------
def test_restaging_a_slot_replaces_it(monkeypatch):
    c = bc.case('persist')
    (X0, y0), (X1, y1) = c['batches'][0], c['batches'][1]
    ctx, twin = new_ctx(c, 70, monkeypatch), new_ctx(c, 70, monkeypatch)
    ctx.stage_batch(0, X0, y0)
    ctx.stage_batch(0, X1, y1)                                      # larger than the first: the slot is sized again
    assert_same_pass(one_pass(ctx, lambda: ctx.select_batch(0)), one_pass(twin, lambda: twin.set_input(X1, y1)), 'larger')
    ctx.stage_batch(0, X0, y0)                                      # and smaller again
    assert_same_pass(one_pass(ctx, lambda: ctx.select_batch(0)), one_pass(twin, lambda: twin.set_input(X0, y0)), 'smaller')
    ctx.close()
    twin.close()


def test_staging_a_slot_while_it_is_resident(monkeypatch):
    """stage_batch waits for the stream and select_batch had copied already: the resident batch is the old one"""
    c = bc.case('persist')
    (X0, y0), (X3, y3) = c['batches'][0], c['batches'][3]
    ctx, twin = new_ctx(c, 300, monkeypatch), new_ctx(c, 300, monkeypatch)
    ctx.stage_batch(0, X0, y0)
    ctx.select_batch(0)
    ctx.stage_batch(0, X3, y3)
    assert ctx.b == len(y0)
    assert_same_pass(one_pass(ctx, lambda: None), one_pass(twin, lambda: twin.set_input(X0, y0)), 'the old batch')
    assert_same_pass(one_pass(ctx, lambda: ctx.select_batch(0)), one_pass(twin, lambda: twin.set_input(X3, y3)), 'the new batch')
    ctx.close()
    twin.close()


def test_two_slots_staged_alike_give_equal_passes(monkeypatch):
    c = bc.case('persist')
    X, y = c['batches'][3]
    out = []
    for slot in (0, 5):
        ctx = new_ctx(c, 70, monkeypatch)
        ctx.stage_batch(0, X, y)
        ctx.stage_batch(5, X, y)
        out.append([one_pass(ctx, lambda: ctx.select_batch(slot)) for _ in range(2)])
        ctx.close()
    for p in range(2):
        assert_same_pass(out[0][p], out[1][p], p)


EIGHT = (70, 300, 7, 130, 1, 64, 65, 33)       # + a single sample, one sample tile exactly, one sample more, one tile row of the transpose + 1


@pytest.mark.parametrize('name', ['persist', 'anyd'])
def test_eight_slots_each_selected_once(name, monkeypatch):
    c = bc.case(name, EIGHT)
    ctx, twin = new_ctx(c, 70, monkeypatch), new_ctx(c, 70, monkeypatch)
    stage_all(ctx, c['batches'])
    for k in (3, 1, 4, 7, 0, 6, 2, 5):
        X, y = c['batches'][k]
        ctx.select_batch(k)
        twin.set_input(X, y)
        assert ctx.b == twin.b == EIGHT[k]
        f, ft = ctx.forward(), twin.forward()
        assert same(f, ft) and np.isfinite(f).all(), k
        assert all(same(a, b) for a, b in zip(envs(ctx), envs(twin))), k
    ctx.close()
    twin.close()


def test_select_brings_the_labels_set_input_left_out(monkeypatch):
    c = bc.case('persist')
    (X0, y0), (X3, y3) = c['batches'][0], c['batches'][3]
    ctx, twin = new_ctx(c, 70, monkeypatch), new_ctx(c, 70, monkeypatch)
    ctx.stage_batch(2, X3, y3)
    ctx.set_input(X0, None)
    ctx.forward()
    assert _code(lambda: ctx.sweep(False, ctx.N - 1, True, *bc.HP)) == STATE          # no labels yet
    assert_same_pass(one_pass(ctx, lambda: ctx.select_batch(2)), one_pass(twin, lambda: twin.set_input(X3, y3)), 'labels')
    ctx.close()
    twin.close()


def test_set_labels_after_a_select_equals_staging_them(monkeypatch):
    c = bc.case('persist')
    X, y = c['batches'][3]
    y2 = np.resize(c['batches'][1][1], y.shape)
    assert not np.array_equal(y, y2)
    a, b = new_ctx(c, 70, monkeypatch), new_ctx(c, 70, monkeypatch)
    a.stage_batch(0, X, y)
    b.stage_batch(0, X, y2)

    def relabelled():
        a.select_batch(0)
        a.set_labels(y2)
    assert_same_pass(one_pass(a, relabelled), one_pass(b, lambda: b.select_batch(0)), 'set_labels')
    a.close()
    b.close()


def test_select_batch_between_two_selections_from_a_dataset(monkeypatch):
    c = bc.case('persist')
    (X0, y0), (X1, y1), _, (X3, y3) = c['batches']
    idx1, idx2 = np.arange(5, 290, 3), np.arange(40)[::-1].copy()
    ctx, twin = new_ctx(c, 70, monkeypatch), new_ctx(c, 70, monkeypatch)
    for t in (ctx, twin):
        t.dataset_attach(X1, y1)
    ctx.stage_batch(0, X3, y3)
    for step, (la, lb) in enumerate(((lambda: ctx.select_indices(idx1), lambda: twin.select_indices(idx1)),
                                     (lambda: ctx.select_batch(0), lambda: twin.set_input(X3, y3)),
                                     (lambda: ctx.select_indices(idx2), lambda: twin.select_indices(idx2)))):
        assert_same_pass(one_pass(ctx, la), one_pass(twin, lb), step)
    assert ctx.b == len(idx2)
    ctx.close()
    twin.close()


# ---------------------------------------------------------------------------------------------------------------
# 5. state and refusals
# ---------------------------------------------------------------------------------------------------------------
def test_a_sweep_behind_a_select_needs_a_forward(monkeypatch):
    c = bc.case('persist')
    ctx = new_ctx(c, 70, monkeypatch)
    stage_all(ctx, c['batches'])
    ctx.select_batch(0)
    ctx.forward()
    for k in (1, 2, 3, 0):
        ctx.select_batch(k)
        assert ctx.b == bc.SIZES[k] == int(_hip.lib().tnml_batch(ctx._h))                     # Context.b follows the slot
        left = ctx.l_pos == ctx.N - 1
        assert _code(lambda: ctx.sweep(left, ctx.N - 1, True, *bc.HP)) == STATE               # the f and the stack of the batch before
        assert ctx.forward().shape == (c['L'], bc.SIZES[k])
        met, f = ctx.sweep(left, ctx.N - 1, True, *bc.HP)
        assert f.shape == (c['L'], bc.SIZES[k]) and np.isfinite(f).all() and np.isfinite(met).all()
    ctx.close()


def test_refusals_leave_everything_as_it_was(monkeypatch):
    c = bc.case('persist')
    (X0, y0), (X3, y3) = c['batches'][0], c['batches'][3]
    N, D, L = c['N'], c['D'], c['L']
    lib, f32p, i32p = _hip.lib(), C.POINTER(C.c_float), C.POINTER(C.c_int32)
    ctx, twin = new_ctx(c, 70, monkeypatch), new_ctx(c, 70, monkeypatch)
    ctx.stage_batch(0, X0, y0)
    ctx.stage_batch(1, X3, y3)
    ctx.select_batch(0)
    twin.set_input(X0, y0)
    f = ctx.forward()
    assert same(f, twin.forward())
    before = bits(ctx)
    other = np.ascontiguousarray(c['batches'][1][0][:40])
    yo = np.ascontiguousarray(c['batches'][1][1][:40])
    xp, yp = other.ctypes.data_as(f32p), yo.ctypes.data_as(i32p)
    bad = yo.copy()
    n = 0
    for call in (lambda: ctx.select_batch(4), lambda: ctx.select_batch(-1), lambda: ctx.select_batch(8)):      # empty, outside
        assert _code(call) == ARG
        n += 1
    for v in (L, -1):                                                                                          # a label outside [0, L)
        bad[:] = yo
        bad[17] = v
        assert _code(lambda: ctx.stage_batch(1, other, bad)) == ARG
        n += 1
    assert _code(lambda: ctx.stage_batch(1, np.zeros((0, N, D), np.float32), np.zeros(0, np.int32))) == ARG    # b = 0
    n += 1
    for rc in (lib.tnml_stage_batch(ctx._h, 1, xp, None, 40), lib.tnml_stage_batch(ctx._h, 1, None, yp, 40),   # y = NULL, X = NULL
               lib.tnml_stage_batch(ctx._h, 1, xp, yp, 0), lib.tnml_stage_batch(ctx._h, 1, xp, yp, -3),
               lib.tnml_stage_batch(ctx._h, -1, xp, yp, 40), lib.tnml_stage_batch(ctx._h, 8, xp, yp, 40),
               lib.tnml_select_batch(None, 0), lib.tnml_stage_batch(None, 1, xp, yp, 40)):
        assert rc == ARG
        n += 1
    assert n == 14
    # the resident batch, its f and the cores are as they were, and a sweep still runs without a new forward
    assert ctx.b == len(y0) == int(lib.tnml_batch(ctx._h))
    assert same(ctx.get_f(), f) and same_bits(before, bits(ctx))
    met, f1 = ctx.sweep(False, N - 1, True, *bc.HP)
    met_t, f1_t = twin.sweep(False, N - 1, True, *bc.HP)
    assert same(met, met_t) and same(f1, f1_t) and same_bits(bits(ctx), bits(twin))
    # the slot the refused calls named holds what it held
    assert_same_pass(one_pass(ctx, lambda: ctx.select_batch(1)), one_pass(twin, lambda: twin.set_input(X3, y3)), 'slot 1')
    ctx.close()
    twin.close()


@pytest.mark.parametrize('name', ['persist', 'large'])
def test_select_in_the_middle_of_a_sweep(name, monkeypatch):
    """any_position on: three steps on one batch, another batch by select_batch, forward with the label at site 3, two more steps.
    The steps before leave a pre-gradient for step 3 of that sweep behind, which the steps after the hand-over must not use."""
    c = bc.case(name)
    (X0, y0), (X3, y3) = c['batches'][0], c['batches'][3]
    out = []
    for how in ('select', 'set_input'):
        ctx = new_ctx(c, max(bc.SIZES), monkeypatch)
        ctx.set_any_position(True)
        if how == 'select':
            ctx.stage_batch(0, X0, y0)
            ctx.stage_batch(1, X3, y3)
        loader(ctx, how, 0, X0, y0)()
        f0 = ctx.forward()
        m1, f1 = ctx.sweep(False, 3, True, *bc.HP)
        loader(ctx, how, 1, X3, y3)()
        assert ctx.l_pos == 3 and ctx.b == len(y3)
        f2 = ctx.forward()
        m2, f3 = ctx.sweep(False, 2, False, *bc.HP)
        out.append(((f0, m1, f1, f2, m2, f3), bits(ctx)))
        ctx.close()
    assert all(same(a, b) and np.isfinite(a).all() for a, b in zip(out[0][0], out[1][0]))
    assert same_bits(out[0][1], out[1][1]) and out[0][1][3] == 5


@pytest.mark.parametrize('l', [0, 2, 3, 5])
def test_select_with_the_label_inside_the_chain(l):
    """any_position on, ragged bonds as in tests/test_any_position_gpu.py: select_batch + forward equals set_input + forward"""
    N, D, L, M, bond = 6, 2, 3, 4, [2, 4, 3, 4, 2]
    rng = np.random.default_rng(40 + l)
    cores = [a.astype(np.float32) for a in random_cores_at(N, D, L, bond, l, rng, scale=0.5 * max(bond))]
    out = []
    for how in ('select', 'set_input'):
        ctx = _hip.Context(N, D, L, M, 7)
        ctx.set_any_position(True)
        ctx.set_cores(cores, l)
        res = []
        for k, b in enumerate((7, 70)):
            X, y = bc.make_batch(N, D, L, b, 4000 + k)
            if how == 'select':
                ctx.stage_batch(k, X, y)
                ctx.select_batch(k)
            else:
                ctx.set_input(X, y)
            f = ctx.forward()
            env = [ctx.get_env(S_L, i) for i in range(l)] + [ctx.get_env(S_R, i) for i in range(l + 1, N)]
            res.append((f, env, ctx.resident_metrics('linear', 1.0)))
        out.append(res)
        ctx.close()
    for (f, env, rm), (ft, envt, rmt) in zip(*out):
        assert same(f, ft) and np.isfinite(f).all() and rm == rmt
        assert len(env) == N - 1 and all(same(a, b) for a, b in zip(env, envt))
