#!/usr/bin/env python3
"""Wall time of one likelihood step at C3 (N = 784, bond 20, 2 labels) and C5 (bond 50, 10 labels) with
b = 5000 samples of an attached dataset and the grid's metric, on one context in one run:

    step_serial     Context.nll_train_indices, one step, tnml_set_nll_overlap off: chunks, sum, both norm walks, the subtraction,
                    the record, the update with renormalisation; nothing of G reaches the host
    step_overlap    the same with the environment walk on the second stream beside the chunks
    host            the route a caller had before: nll_grad_indices (G to the host), the NumPy update A + lr G with the
                    renormalisation in float64, set_cores
    nll_grad        Context.nll_grad_indices alone, and
    log_norm_grad   Context.log_norm_grad alone: what the chains with the subtraction, and the norm term, cost as calls of their own

The chain is near-isometric and calibrated on a small batch (tests/orthogonalize_reference.make_cores); the batch is uniformly random
levels of the 256-level grid (timing does not depend on the values).  lr is small and the cores are renormalised, so that every
round meets cores of the same size.  Every call is timed with time.perf_counter around the whole Python call (it ends with the
stream drained), after `--warmup` untimed rounds, `--reps` times, the calls alternating within a round; median and spread
(max - min) are reported.  "Better" is the rule of DESIGN.md section 8: a gain of more than five times the larger spread.  One JSON
line per shape on stdout and, with --out, appended to a file.

    python tools/bench_nll_step.py --out profiles/r23_bench_nll_step.json
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


def run(name, b, reps, warmup):
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

    def step(overlap):
        ctx.set_nll_overlap(overlap)
        v = ctx.nll_train_indices(idx, b, True, S, LR, 0.0, True)
        assert v[0, 3] == 0, v

    def host():
        G, _ = ctx.nll_grad_indices(idx, True, S)
        cs, _, lp = ctx.get_cores()
        new = []
        for a, g in zip(cs, G):
            a = a.astype(np.float64)
            n = a + np.float32(LR).astype(np.float64) * g.astype(np.float64)
            new.append((n * np.sqrt((a * a).sum() / (n * n).sum())).astype(np.float32))
        ctx.set_cores(new, lp)

    calls = {'step_serial': lambda: step(False), 'step_overlap': lambda: step(True), 'host': host,
             'nll_grad': lambda: ctx.nll_grad_indices(idx, True, S), 'log_norm_grad': lambda: ctx.log_norm_grad(S)}
    ms = {k: [] for k in calls}
    for r in range(warmup + reps):
        for k, fn in calls.items():
            t0 = time.perf_counter()
            fn()
            if r >= warmup:
                ms[k].append(1e3 * (time.perf_counter() - t0))
    ctx.close()
    res = {'shape': name, 'N': N, 'bond': M, 'L': L, 'b': b, 'warmup': warmup}
    res.update({k: stats(v) for k, v in ms.items()})
    res['device_step_beats_host'] = better(res['step_serial'], res['host'])
    res['overlap_beats_serial'] = better(res['step_overlap'], res['step_serial'])
    res['serial_beats_overlap'] = better(res['step_serial'], res['step_overlap'])
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--shapes', default='c3,c5')
    ap.add_argument('--b', type=int, default=5000)
    ap.add_argument('--reps', type=int, default=12)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--out')
    a = ap.parse_args()
    for name in a.shapes.split(','):
        line = json.dumps(run(name, a.b, a.reps, a.warmup))
        print(line, flush=True)
        if a.out:
            with open(a.out, 'a') as fh:
                fh.write(line + '\n')


if __name__ == '__main__':
    main()
