#!/usr/bin/env python3
"""Device time of tnml_orthogonalize, tnml_compress (to half the bond) and tnml_bond_spectra (include/tnml.h)
at C3 (N = 784, bond 20, 2 labels) and C5 (bond 50, 10 labels), beside the route a caller had before the calls existed, on the
same context in the same run: tnml_get_cores, the float64 NumPy chain of tests/orthogonalize_reference.py, tnml_set_cores
(nothing to set for the spectra).

The cores come from a short training run on the context: one sweep there and back at the fixed bond, then two gradient steps.
Every call is timed with HIP events on the context's stream (tnml_timer_start / tnml_timer_stop) after `--warmup` untimed calls,
`--reps` times (at least ten), in alternating order; median and spread (max - min) are reported.  Every timed call starts from the
same cores (tnml_set_cores outside the window).  After the timed part the orthogonal form of the device is checked against the
host route's through tnml_predict on 64 samples.  One JSON line per shape on stdout and, with --out, appended to a file.

    python tools/bench_orthogonalize.py --out profiles/r11_bench_orthogonalize.json
"""
import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p_ in (ROOT, os.path.join(ROOT, 'tests')):
    if p_ not in sys.path:
        sys.path.insert(0, p_)

import orthogonalize_reference as R  # noqa: E402
from tensornetworkforml_amd import _hip  # noqa: E402

SHAPES = {
    # name: (N, bond, labels, batch of the training run)
    'c3': (784, 20, 2, 1000),
    'c5': (784, 50, 10, 1000),
}
SWEEP = (1e-3, 1e-3, True, 'softmax', 'full_cross_ent', 1.0, 'fixed')


def synth(N, b, seed):
    """bench.py's synthetic images: about four pixels in five are zero; embedded with the D = 2 feature map."""
    rng = np.random.default_rng(seed)
    p = rng.random((b, N)) * (rng.random((b, N)) > 0.81)
    return np.stack([np.sin(np.pi * p / 2), np.cos(np.pi * p / 2)], -1).astype(np.float32)


def stats(ms):
    ms = sorted(ms)
    return {'median_ms': ms[len(ms) // 2] if len(ms) % 2 else 0.5 * (ms[len(ms) // 2 - 1] + ms[len(ms) // 2]),
            'spread_ms': ms[-1] - ms[0], 'min_ms': ms[0], 'reps': len(ms)}


def run(name, reps, warmup):
    N, M, L, b = SHAPES[name]
    D, l_pos = 2, 0
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
    for _ in range(3):                                             # calibrate as Network.__init__ does
        ctx.scale_cores(math.exp(-ctx.forward_logabsmax() / N))
    ctx.forward(want_f=False)
    ctx.sweep(False, N - 1, True, *SWEEP, want_metrics=False, want_f=False)
    ctx.forward(want_f=False)
    ctx.sweep(True, N - 1, True, *SWEEP, want_metrics=False, want_f=False)
    ctx.dataset_attach(X, y, 'features')
    ctx.optim_config('sgd', clip=True)
    ctx.gd_train_indices(np.arange(b, dtype=np.int32), b // 2, 1e-3, 0.0, 'softmax', 'full_cross_ent', 1.0)
    start, bond0, l_pos = ctx.get_cores()
    half = max(1, M // 2)

    def host(which):
        cs, _, lp = ctx.get_cores()
        cs = [c.astype(np.float64) for c in cs]
        if which == 'spectra':
            return R.bond_spectra(cs, lp)
        unit, logn = R.orthogonalize(cs, lp) if which == 'orthogonalize' else (lambda r: (r[0], r[3]))(R.compress(cs, lp, half, 1.0))
        new = [c.astype(np.float32) for c in R.with_gauge(unit, logn)[0]]
        ctx.set_cores(new, lp)
        return new, logn

    calls = {
        'device_orthogonalize': lambda: ctx.orthogonalize(),
        'host_orthogonalize': lambda: host('orthogonalize'),
        'device_compress_half': lambda: ctx.compress(half),
        'host_compress_half': lambda: host('compress'),
        'device_bond_spectra': lambda: ctx.bond_spectra(),
        'host_bond_spectra': lambda: host('spectra'),
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
    # the two routes give the same function
    Xp = X[:64]
    ctx.set_cores(start, l_pos)
    f0 = ctx.predict(Xp).astype(np.float64)
    bond_dev, logn_dev = ctx.orthogonalize()
    f_dev = ctx.predict(Xp).astype(np.float64)
    ctx.set_cores(start, l_pos)
    _, logn_host = host('orthogonalize')
    f_host = ctx.predict(Xp).astype(np.float64)
    ctx.set_cores(start, l_pos)
    bond_c, _, disc, _ = ctx.compress(half)
    f_c = ctx.predict(Xp).astype(np.float64)
    ctx.close()
    out = {'bench': 'orthogonalize', 'shape': name, 'N': N, 'bond': M, 'L': L, 'D': D, 'l_pos': int(l_pos), 'half': half,
           'bonds_before': [int(bond0.min()), int(bond0.max())], 'timing': 'HIP events around whole calls'}
    for k in calls:
        out[k] = stats(times[k])
    for what in ('orthogonalize', 'compress_half', 'bond_spectra'):
        d, h = out['device_' + what], out['host_' + what]
        out[what + '_host_minus_device_ms'] = h['median_ms'] - d['median_ms']
        out[what + '_faster_by_more_than_5_spreads'] = bool(h['median_ms'] - d['median_ms'] > 5 * max(d['spread_ms'], h['spread_ms']))
    scale = np.abs(f0).max()
    out['g'] = math.exp(logn_dev / N)
    out['log_norm'] = logn_dev
    out['log_norm_device_minus_host'] = logn_dev - logn_host
    out['f_after_orthogonalize_vs_before'] = float(np.abs(f_dev - f0).max() / scale)
    out['f_after_host_route_vs_before'] = float(np.abs(f_host - f0).max() / scale)
    out['f_after_compress_vs_before'] = float(np.abs(f_c - f0).max() / scale)
    out['bonds_after_orthogonalize'] = [int(bond_dev.min()), int(bond_dev.max())]
    out['bonds_after_compress'] = [int(bond_c.min()), int(bond_c.max())]
    out['discarded_sum'] = float(disc.sum())
    out['finite'] = bool(np.isfinite(f_dev).all() and np.isfinite(f_c).all())
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--shapes', default='c3,c5')
    ap.add_argument('--reps', type=int, default=12)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--out', default=None)
    args = ap.parse_args(argv)
    if _hip.device_count() < 1:
        raise SystemExit('bench_orthogonalize needs an MI355X: there is no CPU path')
    for name in args.shapes.split(','):
        line = json.dumps(run(name, max(args.reps, 10), args.warmup))
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, 'a') as fh:
                fh.write(line + '\n')


if __name__ == '__main__':
    main()
