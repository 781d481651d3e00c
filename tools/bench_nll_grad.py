#!/usr/bin/env python3
"""Wall time of the likelihood gradient of a batch at C3 (N = 784, bond 20, 2 labels) and C5 (bond 50, 10
labels) with b = 5000 samples, on one context in one run:

    nll_grad        Context.nll_grad: prediction, cotangent, core gradients, both norm walks, the subtraction
    core_grad       Context.core_grad at the same shape with a given cotangent: nll_grad minus this is what the norm term costs
    log_norm_grad   Context.log_norm_grad alone
    host            the route a caller had before: predict, a NumPy cotangent, core_grad, get_cores, the float64 NumPy log-norm
                    gradient of tests/nll_reference.py

The chain is near-isometric and calibrated on a small batch (tests/orthogonalize_reference.make_cores); the batch is uniformly random
levels of the 256-level grid (timing does not depend on the values).  Every call is timed with time.perf_counter around the whole
Python call (it ends with the stream drained and the gradient on the host), after `--warmup` untimed rounds, `--reps` times, the four
calls alternating within a round; median and spread (max - min) are reported.  One JSON line per shape on stdout and, with --out,
appended to a file.

    python tools/bench_nll_grad.py --out profiles/r22_bench_nll_grad.json
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


def stats(ms):
    ms = sorted(ms)
    return {'median_ms': ms[len(ms) // 2] if len(ms) % 2 else 0.5 * (ms[len(ms) // 2 - 1] + ms[len(ms) // 2]),
            'spread_ms': ms[-1] - ms[0], 'min_ms': ms[0], 'reps': len(ms)}


def run(name, b, reps, warmup):
    N, M, L = SHAPES[name]
    D, l = 2, 0
    rng = np.random.default_rng(1)
    cores = oref.make_cores(N, D, L, [M] * (N - 1), l, rng, oref.features(rng, 16, N, D))
    _, phi, w = R.grid(R.K, D)
    S = R.gram(phi, w)
    X = phi[rng.integers(0, R.K, (b, N))].astype(np.float32)
    y = rng.integers(0, L, b).astype(np.int32)
    ctx = _hip.Context(N, D, L, M, 64)
    ctx.set_cores(A.as32(cores), l)
    cot = np.zeros((L, b), dtype=np.float32)
    cot[y, np.arange(b)] = 1.0

    def host():
        f = ctx.predict(X)
        c = np.zeros_like(f)
        c[y, np.arange(b)] = 2.0 / (b * f[y, np.arange(b)])
        Gd, _ = ctx.core_grad(X, c)
        cs, _, lp = ctx.get_cores()
        Gz, _ = R.log_norm_gradient(cs, lp, S)
        return [g - z for g, z in zip(Gd, Gz)]

    calls = {'nll_grad': lambda: ctx.nll_grad(X, y, S), 'core_grad': lambda: ctx.core_grad(X, cot),
             'log_norm_grad': lambda: ctx.log_norm_grad(S), 'host': host}
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
    res['norm_term_ms'] = res['nll_grad']['median_ms'] - res['core_grad']['median_ms']
    gain = res['host']['median_ms'] - res['nll_grad']['median_ms']
    res['device_beats_host'] = bool(gain > 5 * max(res['host']['spread_ms'], res['nll_grad']['spread_ms']))
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
