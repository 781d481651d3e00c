#!/usr/bin/env python3
"""Device time of the input-gradient calls (include/tnml.h, tnml_input_grad) at C3 (N = 784, bond 20, 2 labels,
b = 5000) and C5 (bond 50, 10 labels), beside `tnml_forward` and `tnml_predict` on the same context in the same run.

Every call is timed with HIP events on the context's stream (tnml_timer_start / tnml_timer_stop) after `--warmup` untimed calls, `--reps`
times (at least ten), in alternating order; median and spread (max - min) are reported.  The window of a call is the whole call:
  input_grad           host X up (b N D floats), re-tiling, the kernel per chunk, g down (b N D floats), cf down
  input_grad_indices   the same from the attached dataset: no upload of X
  predict              host X up, re-tiling, one chain, f down
  forward              one chain over the resident batch, every environment stored, f down
Algorithmic bytes of the kernel: the stack of stored environments written and read (2 x 4 b sum_i bond_i), X twice (2 x 4 b N D) and
g (4 b N D); `frac_of_8TBs` is those bytes over the median time of input_grad_indices over 8 TB/s -- a whole-call figure, not the
kernel's share of peak (the call also moves g over the bus).  A kernel-only time comes from `rocprofv3 --kernel-trace --stats` around
this script, in a run of its own.  One JSON line per shape on stdout and, with --out, appended to a file.

    python tools/bench_input_grad.py --out profiles/r08_bench_input_grad.json
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
HBM_PEAK_BYTES_S = 8e12


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
    y = rng.integers(0, L, b)
    cores = []
    for i in range(N):
        ml, mr = (1 if i == 0 else M), (1 if i == N - 1 else M)
        cores.append((rng.random((ml, D, mr, L) if i == l_pos else (ml, D, mr)) / (0.25 * D * math.sqrt(ml * mr))).astype(np.float32))
    ctx = _hip.Context(N, D, L, M, b)
    ctx.set_cores(cores, l_pos)
    ctx.set_input(X, y)
    # calibrate as Network.__init__ does: the stored environments are float32 without renormalisation
    for _ in range(3):
        ctx.scale_cores(math.exp(-ctx.forward_logabsmax() / N))
    ctx.dataset_attach(X, y, 'features')
    idx = np.arange(b)
    cot = rng.standard_normal((L, b)).astype(np.float32)
    calls = {
        'input_grad': lambda: ctx.input_grad(X, cot),
        'input_grad_predicted_class': lambda: ctx.input_grad(X),
        'input_grad_indices': lambda: ctx.input_grad_indices(idx, cot, 'features'),
        'predict': lambda: ctx.predict(X),
        'predict_indices': lambda: ctx.predict_indices(idx),
        'forward': lambda: ctx.forward(),
    }
    times = {k: [] for k in calls}
    for rep in range(warmup + reps):
        for k, call in calls.items():
            ctx.synchronize()
            ctx.timer_start()
            call()
            ms = ctx.timer_stop()
            if rep >= warmup:
                times[k].append(ms)
    g, cf = ctx.input_grad_indices(idx, cot, 'features')
    f = ctx.predict(X)
    ctx.close()
    out = {'bench': 'input_grad', 'shape': name, 'N': N, 'bond': M, 'L': L, 'D': D, 'b': b, 'l_pos': l_pos, 'timing': 'HIP events around whole calls'}
    for k in calls:
        out[k] = stats(times[k])
    bytes_alg = 2 * 4.0 * b * (N - 1) * M + 2 * 4.0 * b * N * D + 4.0 * b * N * D
    t = out['input_grad_indices']['median_ms'] * 1e-3
    out['algorithmic_bytes'] = bytes_alg
    out['stack_bytes_written_and_read'] = 2 * 4.0 * b * (N - 1) * M
    out['ratio_to_predict'] = out['input_grad']['median_ms'] / out['predict']['median_ms']
    out['ratio_indices_to_predict_indices'] = out['input_grad_indices']['median_ms'] / out['predict_indices']['median_ms']
    out['ratio_to_forward'] = out['input_grad_indices']['median_ms'] / out['forward']['median_ms']
    out['frac_of_8TBs'] = bytes_alg / t / HBM_PEAK_BYTES_S
    out['finite'] = bool(np.isfinite(g).all() and np.isfinite(cf).all() and np.isfinite(f).all())
    out['max_abs_g'] = float(np.abs(g).max())
    out['euler_identity_worst'] = float(np.abs(np.einsum('bnd,bnd->bn', g.astype(np.float64), X.astype(np.float64)) - cf[:, None]).max()
                                        / max(np.abs(cf).max(), 1e-300))
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
        raise SystemExit('bench_input_grad needs an MI355X: there is no CPU path')
    for name in args.shapes.split(','):
        line = json.dumps(run(name, max(args.reps, 10), args.warmup, args.l_pos))
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, 'a') as fh:
                fh.write(line + '\n')


if __name__ == '__main__':
    main()
