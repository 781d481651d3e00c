#!/usr/bin/env python3
"""Wall time of one full two-site likelihood sweep at C3 (N = 784, bond 20, 2 labels) and C5 (bond 50,
10 labels) with b = 5000 samples of an attached dataset and the grid's metric, on one context in one run:

    sweep_fixed     Context.nll_sweep_indices, N - 1 steps, max_bond = the bond, threshold 1: every step enqueued, one wait
    sweep_adaptive  the same with threshold 0.999: the host learns the bond once per step
    host            the route through the host, LABELLED AS SUCH: the NumPy statement tests/nll_sweep_reference.step timed on
                    --host-steps steps from the middle of the chain (--host-b samples) and scaled to N - 1 steps and b samples
    nll_steps       for orientation only: N - 1 calls of nll_train_indices on the same batch (783 batch-equivalent nll_steps)

The chain is near-isometric and calibrated on a small batch (tests/orthogonalize_reference.make_cores); the batch is uniformly random
levels of the 256-level grid (timing does not depend on the values).  Sweeps alternate direction, right then left, so that every
round meets a chain of the same bonds; lr is small and B is renormalised.  Every call is timed with time.perf_counter around the
whole Python call (it ends with the stream drained), after `--warmup` untimed rounds, `--reps` times; median and spread (max - min)
are reported.  "Better" is the rule of DESIGN.md section 8: a gain of more than five times the larger spread.  One JSON line per
shape on stdout and, with --out, appended to a file.

    python tools/bench_nll_sweep.py --out profiles/r29_bench_nll_sweep.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p_ in (ROOT, os.path.join(ROOT, 'tests')):
    if p_ not in sys.path:
        sys.path.insert(0, p_)

import mps_algebra_reference as A  # noqa: E402
import nll_reference as R  # noqa: E402
import nll_sweep_reference as SR  # noqa: E402
import orthogonalize_reference as oref  # noqa: E402
from tensornetworkforml_amd import _hip  # noqa: E402

SHAPES = {'c3': (784, 20, 2), 'c5': (784, 50, 10)}      # name: (N, bond, labels)
LR = 1e-4


def stats(ms):
    ms = sorted(ms)
    return {'median_ms': ms[len(ms) // 2] if len(ms) % 2 else 0.5 * (ms[len(ms) // 2 - 1] + ms[len(ms) // 2]),
            'spread_ms': ms[-1] - ms[0], 'min_ms': ms[0], 'reps': len(ms)}


def better(new, old):
    """section 8: the gain against five times the larger spread"""
    return bool(old['median_ms'] - new['median_ms'] > 5 * max(old['spread_ms'], new['spread_ms']))


def run(name, b, reps, warmup, host_steps, host_b, with_nll_steps):
    N, M, L = SHAPES[name]
    D, l = 2, 0
    rng = np.random.default_rng(1)
    cores = oref.make_cores(N, D, L, [M] * (N - 1), l, rng, oref.features(rng, 16, N, D))
    _, phi, w = R.grid(R.K, D)
    S = R.gram(phi, w)
    X = phi[rng.integers(0, R.K, (b, N))].astype(np.float32)
    y = rng.integers(0, L, b).astype(np.int32)
    idx = np.arange(b, dtype=np.int32)
    ctx = _hip.Context(N, D, L, M, 64)
    ctx.set_cores(A.as32(cores), l)
    ctx.dataset_attach(X, y)
    ctx.optim_config('sgd', momentum=0.0, clip=False)

    def sweep(threshold):
        v = ctx.nll_sweep_indices(idx, True, S, ctx.l_pos == N - 1, N - 1, LR, True, M, threshold)
        assert (v[:, 3] == 0).all(), v[:, 3]

    def nll_steps():
        v = ctx.nll_train_indices(np.tile(idx, N - 1), b, True, S, LR, 0.0, True)
        assert (v[:, 3] == 0).all()

    calls = {'sweep_fixed': lambda: sweep(1.0), 'sweep_adaptive': lambda: sweep(0.999)}
    if with_nll_steps:
        calls['nll_steps'] = nll_steps
    ms = {k: [] for k in calls}
    for r in range(warmup + reps):
        for k, fn in calls.items():
            if k != 'nll_steps' and ctx.l_pos not in (0, N - 1):
                raise RuntimeError('the label is inside the chain')
            if k == 'nll_steps':
                ctx.optim_reset()
            t0 = time.perf_counter()
            fn()
            if r >= warmup:
                ms[k].append(1e3 * (time.perf_counter() - t0))
    ctx.close()
    # the route through the host: the NumPy statement on a few steps from the middle of the chain, scaled
    mid = N // 2
    cs = oref.make_cores(N, D, L, [M] * (N - 1), mid, np.random.default_rng(2), oref.features(rng, 16, N, D))
    Xh, yh = X[:host_b], y[:host_b]
    t0 = time.perf_counter()
    SR.sweep(cs, mid, Xh, yh, S, False, host_steps, LR, True, M)
    per_step = 1e3 * (time.perf_counter() - t0) / host_steps
    res = {'shape': name, 'N': N, 'bond': M, 'L': L, 'b': b, 'warmup': warmup}
    res.update({k: stats(v) for k, v in ms.items()})
    res['host_numpy_scaled'] = {'estimate_ms': per_step * (N - 1) * b / host_b, 'timed_steps': host_steps, 'timed_b': host_b,
                                'note': 'NumPy reference timed on timed_steps steps and timed_b samples, scaled to N - 1 steps and b samples'}
    res['adaptive_beats_fixed'] = better(res['sweep_adaptive'], res['sweep_fixed'])
    res['fixed_beats_adaptive'] = better(res['sweep_fixed'], res['sweep_adaptive'])
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--shapes', default='c3,c5')
    ap.add_argument('--b', type=int, default=5000)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--host-steps', dest='host_steps', type=int, default=4)
    ap.add_argument('--host-b', dest='host_b', type=int, default=500)
    ap.add_argument('--no-nll-steps', dest='nll_steps', action='store_false')
    ap.add_argument('--out')
    a = ap.parse_args()
    for name in a.shapes.split(','):
        line = json.dumps(run(name, a.b, a.reps, a.warmup, a.host_steps, a.host_b, a.nll_steps))
        print(line, flush=True)
        if a.out:
            with open(a.out, 'a') as fh:
                fh.write(line + '\n')


if __name__ == '__main__':
    main()
