"""Cases of the staged-batch hand-over tests (tnml_stage_batch / tnml_select_batch), plain NumPy.

tests/test_batch_handover_host.py checks with the float64 oracle alone that the four staged batches of every configuration can be
told apart by what tests/test_batch_handover_gpu.py compares; the seeds below were picked so that they can.

A configuration is a chain shape and the launch path a context is put on: `calls` are Context methods applied after creation, `comm`
asks for the one-rank communicator (TNML_FORCE_COMM=1 + dist.attach_comm).
"""
import numpy as np

from oracle import mps_oracle as mo
from tensornetworkforml_amd import data_generator as gen

# one partial sample tile, several tiles, fewer samples than one tile row of the 32 x 32 transpose, b_pad 128 against 192
SIZES = (70, 300, 7, 130)
# bench.py's hyper-parameters, in the order of Context.sweep behind (left_dir, n_steps, first_of_sweep)
HP = (1e-3, 1e-3, True, 'softmax', 'full_cross_ent', 0.1, 'fixed')
HP_KW = dict(lr=1e-3, weight_dec=1e-3, L2_flag=True, act_fn='softmax', loss_fn='full_cross_ent', T=0.1, trunc='fixed')

CONFIGS = {
    # id: chain shape, launch path, seed of the cores (batch k of a configuration: seed + 97 (k + 1))
    'persist': dict(N=12, D=2, L=2, M=6, calls=(), comm=False, seed=1100),                                   # one persistent launch
    'persist3': dict(N=12, D=2, L=2, M=6, calls=(('set_persistent', 2),), comm=False, seed=1200),            # three launches, three streams
    'per_step': dict(N=12, D=2, L=2, M=6, calls=(('set_persistent', 0),), comm=False, seed=1300),
    'classic': dict(N=12, D=2, L=2, M=6, calls=(('set_persistent', 0), ('set_step_pipeline', False)), comm=False, seed=1400),
    'large': dict(N=12, D=2, L=3, M=6, calls=(('set_narrow_path', 1),), comm=False, seed=1500),              # two-stream large-tensor step
    'shape': dict(N=14, D=2, L=2, M=10, calls=(), comm=False, seed=1600),                                    # the body compiled for bond 10
    'anyd': dict(N=9, D=3, L=3, M=5, calls=(), comm=False, seed=1700),                                       # generic-D path
    'comm': dict(N=12, D=2, L=2, M=6, calls=(), comm=True, seed=1800),
}


def features(rng, b, N, D):
    """sin / cos features of uniform pixels; data_generator.psi beyond D = 2"""
    p = rng.random((b, N))
    if D == 2:
        return np.stack([np.sin(np.pi * p / 2), np.cos(np.pi * p / 2)], -1).astype(np.float32)
    return gen.psi(p, D).astype(np.float32)


def make_batch(N, D, L, b, seed):
    rng = np.random.default_rng(seed)
    X = features(rng, b, N, D)
    return X, rng.integers(0, L, b).astype(np.int32)


def make_cores(N, D, L, M, seed):
    """mo.random_cores scaled as in test_batch_larger_than_the_capacity_given_at_creation (M * 0.64 at D = 2), as float32"""
    rng = np.random.default_rng(seed)
    return [c.astype(np.float32) for c in mo.random_cores(N, M, D, L, rng=rng, scale=M * 0.5 * 0.64 * D)]


_cases = {}


def case(name, sizes=SIZES):
    """dict(N, D, L, M, calls, comm, cores (float32), batches [(X float32, y int32)]) of a configuration; built once, never
    written to."""
    key = (name, tuple(sizes))
    if key not in _cases:
        c = dict(CONFIGS[name])
        c['name'] = name
        c['cores'] = make_cores(c['N'], c['D'], c['L'], c['M'], c['seed'])
        c['batches'] = [make_batch(c['N'], c['D'], c['L'], b, c['seed'] + 97 * (k + 1)) for k, b in enumerate(sizes)]
        _cases[key] = c
    return _cases[key]


def oracle_state(c, cores=None, l_pos=0):
    return mo.MPSState(c['N'], c['D'], c['L'], c['M'], [np.asarray(a, dtype=np.float64) for a in (c['cores'] if cores is None else cores)], l_pos)


_oracle = {}


def oracle_first_pass(name, k=0, sizes=SIZES):
    """(f of forward, f after one sweep, the cores it reached) of the float64 oracle on batch k from the configuration's cores;
    computed once per (configuration, batch) and shared"""
    key = (name, k, tuple(sizes))
    if key not in _oracle:
        c = case(name, sizes)
        X, y = c['batches'][k]
        X64 = X.astype(np.float64)
        st = oracle_state(c)
        f0 = mo.forward(st, X64)
        f1 = mo.sweep(st, X64, y, f0, HP_KW['lr'], HP_KW['weight_dec'], L2_flag=True, left_dir=False, act_fn=HP_KW['act_fn'],
                      loss_fn=HP_KW['loss_fn'], T=HP_KW['T'], trunc=HP_KW['trunc'])
        _oracle[key] = (f0, f1, [a.copy() for a in st.cores])
    return _oracle[key]
