#!/usr/bin/env python3
"""Device time of the core-gradient call (include/tnml.h, tnml_core_grad) at C3 (N = 784, bond 20, 2 labels,
b = 5000) and C5 (bond 50, 10 labels), beside `tnml_input_grad` and `tnml_predict` on the same context in the same run.

Every call is timed with HIP events on the context's stream (tnml_timer_start / tnml_timer_stop) after `--warmup` untimed calls, `--reps`
times (at least ten), in alternating order; median and spread (max - min) are reported.  The window of a call is the whole call:
  core_grad            host X up (b N D floats), re-tiling, the chain kernel and the reduction kernel per chunk, G down
                       (tnml_cores_size floats), cf down; the Python wrapper's tnml_get_cores (it asks for the bonds) is outside
  core_grad_indices    the same from the attached dataset: no upload of X
  input_grad           host X up, re-tiling, the kernel per chunk, g down (b N D floats), cf down
  predict              host X up, re-tiling, one chain, f down
Algorithmic bytes of the two kernels: both stacks written once and read once (4 x 4 b sum_i bond_i), X twice by the chain kernel and
once per workgroup row of the reduction, G once per chunk.  Kernel-only times come from `rocprofv3 --kernel-trace --stats` around this
script, in a run of its own.  One JSON line per shape on stdout and, with --out, appended to a file.

    python tools/bench_core_grad.py --out profiles/r09_bench_core_grad.json
"""
import argparse
import ctypes as C
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
    lib, f32p, i32p = _hip.lib(), C.POINTER(C.c_float), C.POINTER(C.c_int32)
    flat = np.empty(sum(c.size for c in cores), dtype=np.float32)
    cf = np.empty(b, dtype=np.float32)
    idx32 = idx.astype(np.int32)
    Xp, cp, Gp, cfp, ip = (X.ctypes.data_as(f32p), cot.ctypes.data_as(f32p), flat.ctypes.data_as(f32p), cf.ctypes.data_as(f32p),
                           idx32.ctypes.data_as(i32p))

    def ok(rc):
        assert rc == 0, lib.tnml_last_error()

    calls = {
        'core_grad': lambda: ok(lib.tnml_core_grad(ctx._h, Xp, b, cp, Gp, flat.size, cfp)),
        'core_grad_predicted_class': lambda: ok(lib.tnml_core_grad(ctx._h, Xp, b, None, Gp, flat.size, cfp)),
        'core_grad_indices': lambda: ok(lib.tnml_core_grad_indices(ctx._h, ip, b, cp, Gp, flat.size, cfp)),
        'input_grad': lambda: ctx.input_grad(X, cot),
        'predict': lambda: ctx.predict(X),
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
    G, cf = ctx.core_grad_indices(idx, cot)
    A = ctx.get_cores()[0]
    ctx.close()
    out = {'bench': 'core_grad', 'shape': name, 'N': N, 'bond': M, 'L': L, 'D': D, 'b': b, 'l_pos': l_pos, 'timing': 'HIP events around whole calls'}
    for k in calls:
        out[k] = stats(times[k])
    out['stack_bytes_written_and_read'] = 4 * 4.0 * b * (N - 1) * M
    out['gradient_floats'] = int(flat.size)
    out['ratio_to_input_grad'] = out['core_grad']['median_ms'] / out['input_grad']['median_ms']
    out['ratio_to_predict'] = out['core_grad']['median_ms'] / out['predict']['median_ms']
    out['finite'] = bool(all(np.isfinite(g).all() for g in G) and np.isfinite(cf).all())
    out['max_abs_G'] = float(max(np.abs(g).max() for g in G))
    euler = np.array([(g.astype(np.float64) * a.astype(np.float64)).sum() for g, a in zip(G, A)])
    out['euler_identity_worst'] = float(np.abs(euler - cf.astype(np.float64).sum()).max() / max(np.abs(cf).astype(np.float64).sum(), 1e-300))
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
        raise SystemExit('bench_core_grad needs an MI355X: there is no CPU path')
    for name in args.shapes.split(','):
        line = json.dumps(run(name, max(args.reps, 10), args.warmup, args.l_pos))
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, 'a') as fh:
                fh.write(line + '\n')


if __name__ == '__main__':
    main()
