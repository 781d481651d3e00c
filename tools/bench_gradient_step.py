#!/usr/bin/env python3
"""Device time of one optimiser step over all cores (include/tnml.h, tnml_gd_train_indices) at C3 (N = 784,
bond 20, 2 labels, b = 5000) and C5 (bond 50, 10 labels), beside the route a caller had before the call existed, on the same
context in the same run.

Every call is timed with HIP events on the context's stream (tnml_timer_start / tnml_timer_stop) after `--warmup` untimed calls,
`--reps` times (at least ten), in alternating order; median and spread (max - min) are reported.  Every timed call starts from the
same cores (tnml_set_cores outside the window).  The windows:
  device_step          tnml_gd_train_indices, one batch: index list up, gather, prediction chain, metrics, loss derivative, both
                       core-gradient kernels per chunk, the optimiser kernel, three doubles down
  host_route           the same step without the call: tnml_predict_indices (f down), activation and loss derivative in NumPy,
                       tnml_core_grad_indices (cot up, G down), the clipped update in NumPy, tnml_set_cores (every slot up)
  core_grad_indices    tnml_core_grad_indices alone with a cotangent from the host
  predict_indices      tnml_predict_indices alone
  epoch_one_call       four batches in one tnml_gd_train_indices call (one synchronisation)
  epoch_four_calls     the same four batches in four calls
SGD with the clip, softmax / MSE at T = 1, lr = 1e-3.  One JSON line per shape on stdout and, with --out, appended to a file.

    python tools/bench_gradient_step.py --out profiles/r10_bench_gradient_step.json
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
ACT, LOSS, T, LR, WD = 'softmax', 'MSE', 1.0, 1e-3, 0.0


def synth(N, b, seed):
    """bench.py's synthetic images: about four pixels in five are zero; embedded with the D = 2 feature map."""
    rng = np.random.default_rng(seed)
    p = rng.random((b, N)) * (rng.random((b, N)) > 0.81)
    return np.stack([np.sin(np.pi * p / 2), np.cos(np.pi * p / 2)], -1).astype(np.float32)


def stats(ms):
    ms = sorted(ms)
    return {'median_ms': ms[len(ms) // 2] if len(ms) % 2 else 0.5 * (ms[len(ms) // 2 - 1] + ms[len(ms) // 2]),
            'spread_ms': ms[-1] - ms[0], 'min_ms': ms[0], 'reps': len(ms)}


def run(name, reps, warmup, l_pos, chunk):
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
    # calibrate as Network.__init__ does: the stored environments are float32 without renormalisation
    for _ in range(3):
        ctx.scale_cores(math.exp(-ctx.forward_logabsmax() / N))
    start = ctx.get_cores()[0]
    ctx.dataset_attach(X, y, 'features')
    ctx.optim_config('sgd', clip=True)
    ctx.set_core_grad_chunk(chunk)
    idx = np.arange(b, dtype=np.int32)
    idx4 = np.tile(idx, 4)
    lib, f32p, i32p = _hip.lib(), C.POINTER(C.c_float), C.POINTER(C.c_int32)
    sizes = [c.size for c in start]
    offs = np.concatenate([[0], np.cumsum(sizes)])
    flat = np.empty(int(offs[-1]), dtype=np.float32)
    Gp, ip = flat.ctypes.data_as(f32p), idx.ctypes.data_as(i32p)
    onehot = np.zeros((L, b))
    onehot[y, np.arange(b)] = 1.0
    cot0 = rng.standard_normal((L, b)).astype(np.float32)

    def ok(rc):
        assert rc == 0, lib.tnml_last_error()

    def loss_derivative(f):
        z = f.astype(np.float64) / T
        e = np.exp(z - z.max(axis=0, keepdims=True))
        return (onehot - e / e.sum(axis=0, keepdims=True)).astype(np.float32)

    def host_route():
        cot = loss_derivative(ctx.predict_indices(idx))
        ok(lib.tnml_core_grad_indices(ctx._h, ip, b, cot.ctypes.data_as(f32p), Gp, flat.size, None))
        new = []
        for i, a in enumerate(start):
            d = flat[offs[i]:offs[i + 1]].reshape(a.shape).astype(np.float64) - WD * a
            s_a, s_d = np.abs(a, dtype=np.float64).sum(), np.abs(d).sum()
            if s_d > s_a:
                d *= s_a / s_d
            new.append((a + LR * d).astype(np.float32))
        ctx.set_cores(new, l_pos)
        return new

    calls = {
        'device_step': lambda: ctx.gd_train_indices(idx, b, LR, WD, ACT, LOSS, T),
        'host_route': host_route,
        'core_grad_indices': lambda: ok(lib.tnml_core_grad_indices(ctx._h, ip, b, cot0.ctypes.data_as(f32p), Gp, flat.size, None)),
        'predict_indices': lambda: ctx.predict_indices(idx),
        'epoch_one_call': lambda: ctx.gd_train_indices(idx4, b, LR, WD, ACT, LOSS, T),
        'epoch_four_calls': lambda: [ctx.gd_train_indices(idx, b, LR, WD, ACT, LOSS, T) for _ in range(4)],
    }
    times = {k: [] for k in calls}
    for rep in range(warmup + reps):
        for k, call in calls.items():
            ctx.set_cores(start, l_pos)
            ctx.synchronize()
            ctx.timer_start()
            call()
            ms = ctx.timer_stop()
            if rep >= warmup:
                times[k].append(ms)
    # the two routes give the same step
    ctx.set_cores(start, l_pos)
    met = ctx.gd_train_indices(idx, b, LR, WD, ACT, LOSS, T)
    dev = ctx.get_cores()[0]
    ctx.set_cores(start, l_pos)
    host = host_route()
    ctx.close()
    out = {'bench': 'gradient_step', 'shape': name, 'N': N, 'bond': M, 'L': L, 'D': D, 'b': b, 'l_pos': l_pos, 'chunk': chunk, 'optimizer': 'sgd, clip',
           'act_fn': ACT, 'loss_fn': LOSS, 'timing': 'HIP events around whole calls'}
    for k in calls:
        out[k] = stats(times[k])
    spread = max(out['device_step']['spread_ms'], out['host_route']['spread_ms'])
    out['host_minus_device_ms'] = out['host_route']['median_ms'] - out['device_step']['median_ms']
    out['faster_by_more_than_5_spreads'] = bool(out['host_minus_device_ms'] > 5 * spread)
    out['device_minus_core_grad_ms'] = out['device_step']['median_ms'] - out['core_grad_indices']['median_ms']
    out['within_core_grad_plus_predict'] = bool(out['device_minus_core_grad_ms'] <= max(out['device_step']['spread_ms'], out['core_grad_indices']['spread_ms']) +
                                                out['predict_indices']['median_ms'])
    out['gradient_floats'] = int(flat.size)
    out['correct_before_step'] = int(met[0, 0])
    scale = max(np.abs(h.astype(np.float64) - s).max() for h, s in zip(host, start))
    out['device_vs_host_step'] = float(max(np.abs(d.astype(np.float64) - h).max() for d, h in zip(dev, host)) / max(scale, 1e-300))
    out['finite'] = bool(all(np.isfinite(d).all() for d in dev))
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--shapes', default='c3,c5')
    ap.add_argument('--reps', type=int, default=12)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--l-pos', type=int, default=0)
    ap.add_argument('--chunk', type=int, default=0, help='samples per pass of the core-gradient kernels (0: the default rule)')
    ap.add_argument('--out', default=None)
    args = ap.parse_args(argv)
    if _hip.device_count() < 1:
        raise SystemExit('bench_gradient_step needs an MI355X: there is no CPU path')
    for name in args.shapes.split(','):
        line = json.dumps(run(name, max(args.reps, 10), args.warmup, args.l_pos, args.chunk))
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, 'a') as fh:
                fh.write(line + '\n')


if __name__ == '__main__':
    main()
