#!/usr/bin/env python3
"""Wall time of whole Context.sample_masked calls at N = 784, bond 20 with 2 labels (C3) and bond 50 with 10
labels (C5), K = 256 levels, for n = 16, 64 and 1024 samples, the masks "bottom half known" and "a random half known", with the
walk (draw = 1) and without it (draw = 0), beside the route through the host on the same context in the same run: tnml_get_cores
and the float64 NumPy reference of tests/sample_masked_reference.py at `--host-n` samples, scaled per sample.

The network is a near-isometric chain calibrated on a small batch (tests/orthogonalize_reference.make_cores), the label on site 0,
the class drawn.  Every call is timed with time.perf_counter around the whole Python call (it ends with the outputs on the host),
after `--warmup` untimed rounds, `--reps` times (at least ten), the device calls and the host route alternating within a round;
median and spread (max - min) are reported, and the rule of DESIGN.md section 8 is applied to the per-sample times: a route is
called faster only when the difference of the medians exceeds five times the larger spread -- whichever way it comes out.  One
JSON line per shape on stdout and, with --out, appended to a file.

    python tools/bench_sample_masked.py --out profiles/r19_bench_sample_masked.json
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
import orthogonalize_reference as R  # noqa: E402
import sample_masked_reference as M  # noqa: E402
import sample_reference as S  # noqa: E402
from tensornetworkforml_amd import _hip  # noqa: E402

SHAPES = {'c3': (784, 20, 2), 'c5': (784, 50, 10)}
SIZES = (16, 64, 1024)
K = 256


def stats(ms):
    ms = sorted(ms)
    return {'median_ms': ms[len(ms) // 2] if len(ms) % 2 else 0.5 * (ms[len(ms) // 2 - 1] + ms[len(ms) // 2]),
            'spread_ms': ms[-1] - ms[0], 'min_ms': ms[0], 'reps': len(ms)}


def run(name, reps, warmup, host_n):
    N, Mb, L = SHAPES[name]
    D, l = 2, 0
    rng = np.random.default_rng(1)
    W = R.make_cores(N, D, L, [Mb] * (N - 1), l, rng, R.features(rng, 8, N, D))
    ctx = _hip.Context(N, D, L, Mb, 8)
    ctx.set_any_position(True)
    ctx.set_cores(A.as32(W), l)
    _, phi, w = S.grid(K, D)
    nmax = max(SIZES)
    masks = {'bottom': np.arange(N) >= N // 2, 'random': rng.random(N) < 0.5}
    known = rng.integers(100, 156, (nmax, N)).astype(np.int32)

    def host(mask, draw):
        def call():
            cs, _, lp = ctx.get_cores()
            return M.masked_walk(A.as64(cs), lp, phi, w, np.full(host_n, -1), S.hash_uniforms(3, host_n, N), mask, known[:host_n], draw=draw)
        return call

    calls = {}
    for mname, mask in masks.items():
        for draw in (1, 0):
            for n in SIZES:
                calls['device_%s_draw%d_n%d' % (mname, draw, n)] = lambda n=n, mask=mask, draw=draw: ctx.sample_masked(n, phi, w, mask, known[:n], None, None, 3, bool(draw))
            calls['host_%s_draw%d_n%d' % (mname, draw, host_n)] = host(mask, bool(draw))
    times = {k: [] for k in calls}
    results = {}
    for rep in range(warmup + reps):
        for k, call in calls.items():
            ctx.synchronize()
            t0 = time.perf_counter()
            results[k] = call()
            ms = 1e3 * (time.perf_counter() - t0)
            if rep >= warmup:
                times[k].append(ms)
    out = {'bench': 'sample_masked', 'shape': name, 'N': N, 'bond': Mb, 'L': L, 'D': D, 'l_pos': l, 'K': K, 'host_n': host_n,
           'timing': 'time.perf_counter around whole calls, outputs on the host'}
    for k in calls:
        out[k] = stats(times[k])
    for mname in masks:
        for draw in (1, 0):
            h = out['host_%s_draw%d_n%d' % (mname, draw, host_n)]
            for n in SIZES:
                d = out['device_%s_draw%d_n%d' % (mname, draw, n)]
                dm, hm = d['median_ms'] / n, h['median_ms'] / host_n
                spread = max(d['spread_ms'] / n, h['spread_ms'] / host_n)
                out['%s_draw%d_n%d_per_sample_ms' % (mname, draw, n)] = {
                    'device': dm, 'host': hm, 'host_over_device': hm / dm,
                    'device_faster_by_more_than_5_spreads': bool(hm - dm > 5 * spread), 'host_faster_by_more_than_5_spreads': bool(dm - hm > 5 * spread)}
        # the same seed and the same rows: the device's draws against the host route's, on the samples the reference calls decidable
        lev, lab, logp = ctx.sample_masked(host_n, phi, w, masks[mname], known[:host_n], None, None, 3)
        rlev, rlab, rlogp, mg = results['host_%s_draw1_n%d' % (mname, host_n)]
        ok = S.decidable(mg)
        out['%s_equal_decidable' % mname] = bool(np.array_equal(lev[ok], rlev[ok]) and np.array_equal(lab[ok], rlab[ok]))
        out['%s_decidable' % mname] = int(ok.sum())
        out['%s_dlogp' % mname] = float(np.abs(logp[ok] - rlogp[ok]).max()) if ok.any() else 0.0
    ctx.close()
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--shapes', default='c3,c5')
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--host-n', dest='host_n', type=int, default=2)
    ap.add_argument('--out', default=None)
    args = ap.parse_args(argv)
    if _hip.device_count() < 1:
        raise SystemExit('bench_sample_masked needs an MI355X: there is no CPU path')
    for name in args.shapes.split(','):
        line = json.dumps(run(name, max(args.reps, 10), args.warmup, args.host_n))
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, 'a') as fh:
                fh.write(line + '\n')


if __name__ == '__main__':
    main()
