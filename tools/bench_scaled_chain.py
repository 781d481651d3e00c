#!/usr/bin/env python3
"""Price of the range-safe chains (include/tnml.h, tnml_set_chain_scaling) at C3 (N = 784, bond 20, 2 labels,
b = 5000) and C5 (bond 50, 10 labels): `predict`, `input_grad`, `core_grad_indices` and `gd_step` with the switch off and on, on one
context, alternating off / on call by call in one session.

Every call is timed with HIP events on the context's stream (tnml_timer_start / tnml_timer_stop) after `--warmup` untimed rounds, `--reps`
times (at least ten); median and spread (max - min) are reported per call and setting, with the ratio on / off of the medians.  The
window of a call is the whole call, as in tools/bench_input_grad.py, tools/bench_core_grad.py and tools/bench_gradient_step.py.
`gd_step` runs at lr = 0 and no weight decay, so that every repetition sees the same cores.  `predict_scaled` (same kernel as
`predict` with the switch on, mantissas and exponents down instead of f) is timed beside them.  One JSON line per shape on stdout and,
with --out, appended to a file.

    python tools/bench_scaled_chain.py --out profiles/r13_bench_scaled_chain.json
"""
import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tensornetworkforml_amd import _hip  # noqa: E402

SHAPES = {
    # name: (N, bond, labels, batch)
    'c3': (784, 20, 2, 5000),
    'c5': (784, 50, 10, 5000),
}


def synth(N, b, seed):
    """bench.py's synthetic images: about four pixels in five are zero; embedded with the D = 2 feature map."""
    rng = np.random.default_rng(seed)
    p = rng.random((b, N)) * (rng.random((b, N)) > 0.81)
    return np.stack([np.sin(np.pi * p / 2), np.cos(np.pi * p / 2)], -1).astype(np.float32)


def stats(ms):
    ms = sorted(ms)
    return {'median_ms': ms[len(ms) // 2] if len(ms) % 2 else 0.5 * (ms[len(ms) // 2 - 1] + ms[len(ms) // 2]),
            'spread_ms': ms[-1] - ms[0], 'min_ms': ms[0], 'reps': len(ms)}


def run(name, reps, warmup, l_pos):
    N, M, L, b = SHAPES[name]
    D = 2
    rng = np.random.default_rng(1)
    X = synth(N, b, 2)
    y = rng.integers(0, L, b).astype(np.int32)
    cores = []
    for i in range(N):
        ml, mr = (1 if i == 0 else M), (1 if i == N - 1 else M)
        cores.append((rng.random((ml, D, mr, L) if i == l_pos else (ml, D, mr)) / (0.25 * D * math.sqrt(ml * mr))).astype(np.float32))
    ctx = _hip.Context(N, D, L, M, b)
    ctx.set_cores(cores, l_pos)
    ctx.set_input(X, y)
    # calibrate as Network.__init__ does: the plain chains are float32 without renormalisation
    for _ in range(3):
        ctx.scale_cores(math.exp(-ctx.forward_logabsmax() / N))
    ctx.dataset_attach(X, y, 'features')
    ctx.optim_config('sgd', clip=False)
    idx = np.arange(b)
    cot = rng.standard_normal((L, b)).astype(np.float32)
    calls = {
        'predict': lambda: ctx.predict(X),
        'input_grad': lambda: ctx.input_grad(X, cot),
        'core_grad_indices': lambda: ctx.core_grad_indices(idx, cot),
        'gd_step': lambda: ctx.gd_step(X, y, 0.0, 0.0, 'linear', 'MSE', 1.0),
        'predict_scaled': lambda: ctx.predict_scaled(X),
    }
    times = {(k, on): [] for k in calls for on in (0, 1)}
    for rep in range(warmup + reps):
        for k, call in calls.items():
            for on in (0, 1):
                ctx.set_chain_scaling(on)
                ctx.synchronize()
                ctx.timer_start()
                call()
                ms = ctx.timer_stop()
                if rep >= warmup:
                    times[k, on].append(ms)
    # what the two settings return on this calibrated network
    ctx.set_chain_scaling(0)
    f0, (g0, cf0) = ctx.predict(X), ctx.input_grad(X, cot)
    ctx.set_chain_scaling(1)
    f1, (g1, cf1) = ctx.predict(X), ctx.input_grad(X, cot)
    mant, expo = ctx.predict_scaled(X)
    ctx.close()
    out = {'bench': 'scaled_chain', 'shape': name, 'N': N, 'bond': M, 'L': L, 'D': D, 'b': b, 'l_pos': l_pos,
           'timing': 'HIP events around whole calls, switch off / on alternating call by call'}
    for k in calls:
        off, on = stats(times[k, 0]), stats(times[k, 1])
        out[k] = {'off': off, 'on': on, 'on_over_off': on['median_ms'] / off['median_ms']}
    out['finite'] = bool(np.isfinite(f1).all() and np.isfinite(g1).all() and np.isfinite(cf1).all())
    out['predict_on_vs_off_rel'] = float(np.abs(f1.astype(np.float64) - f0).max() / np.abs(f0).max())
    out['input_grad_bit_equal_on_off'] = bool(np.array_equal(g0, g1) and np.array_equal(cf0, cf1))
    out['expo_range'] = [int(expo.min()), int(expo.max())]
    out['mant_absmax_range'] = [float(np.abs(mant).max(axis=0).min()), float(np.abs(mant).max(axis=0).max())]
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--shapes', default='c3,c5')
    ap.add_argument('--reps', type=int, default=12)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--l-pos', type=int, default=0)
    ap.add_argument('--out', default=None)
    args = ap.parse_args(argv)
    if _hip.device_count() < 1:
        raise SystemExit('bench_scaled_chain needs an MI355X: there is no CPU path')
    for name in args.shapes.split(','):
        line = json.dumps(run(name, max(args.reps, 10), args.warmup, args.l_pos))
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, 'a') as fh:
                fh.write(line + '\n')


if __name__ == '__main__':
    main()
