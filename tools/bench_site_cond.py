#!/usr/bin/env python3
"""Wall time of whole Context.site_conditionals calls at N = 784, bond 20 with 2 labels (C3) and bond 50 with
10 labels (C5), K = 256 levels, for n = 16, 64 and 1024 samples, with the bottom half of the pixels known and with all of them
known, beside the route through the host on the same context in the same run: tnml_get_cores and the float64 NumPy reference of
tests/site_cond_reference.py at `--host-n` samples, scaled per sample.

The network, the timing and the rule are those of tools/bench_sample_masked.py: a near-isometric chain calibrated on a small batch,
the label on site 0 and summed; time.perf_counter around the whole Python call (it ends with all four outputs on the host), after
`--warmup` untimed rounds, `--reps` times (at least ten), the device calls and the host route alternating within a round; median
and spread (max - min); a route is called faster only when the difference of the per-sample medians exceeds five times the larger
spread -- whichever way it comes out.  One JSON line per shape on stdout and, with --out, appended to a file.

    python tools/bench_site_cond.py --out profiles/r25_bench_site_cond.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p_ in (ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tools')):
    if p_ not in sys.path:
        sys.path.insert(0, p_)

import mps_algebra_reference as A  # noqa: E402
import orthogonalize_reference as R  # noqa: E402
import sample_reference as S  # noqa: E402
import site_cond_reference as C  # noqa: E402
from bench_sample_masked import SHAPES, SIZES, K, stats  # noqa: E402
from tensornetworkforml_amd import _hip  # noqa: E402


def run(name, reps, warmup, host_n):
    N, Mb, L = SHAPES[name]
    D, l = 2, 0
    rng = np.random.default_rng(1)
    W = R.make_cores(N, D, L, [Mb] * (N - 1), l, rng, R.features(rng, 8, N, D))
    ctx = _hip.Context(N, D, L, Mb, 8)
    ctx.set_any_position(True)
    ctx.set_cores(A.as32(W), l)
    x, phi, w = S.grid(K, D)
    masks = {'half': np.arange(N) >= N // 2, 'all': np.ones(N, dtype=bool)}
    known = rng.integers(100, 156, (max(SIZES), N)).astype(np.int32)

    def host(mask):
        def call():
            cs, _, lp = ctx.get_cores()
            return C.conditionals(A.as64(cs), lp, phi, w, x, np.full(host_n, -1), mask, known[:host_n])
        return call

    calls = {}
    for mname, mask in masks.items():
        for n in SIZES:
            calls['device_%s_n%d' % (mname, n)] = lambda n=n, mask=mask: ctx.site_conditionals(n, phi, w, mask, known[:n], None, x)
        calls['host_%s_n%d' % (mname, host_n)] = host(mask)
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
    out = {'bench': 'site_cond', 'shape': name, 'N': N, 'bond': Mb, 'L': L, 'D': D, 'l_pos': l, 'K': K, 'host_n': host_n,
           'timing': 'time.perf_counter around whole calls, outputs on the host'}
    for k in calls:
        out[k] = stats(times[k])
    for mname in masks:
        h = out['host_%s_n%d' % (mname, host_n)]
        for n in SIZES:
            d = out['device_%s_n%d' % (mname, n)]
            dm, hm = d['median_ms'] / n, h['median_ms'] / host_n
            spread = max(d['spread_ms'] / n, h['spread_ms'] / host_n)
            out['%s_n%d_per_sample_ms' % (mname, n)] = {
                'device': dm, 'host': hm, 'host_over_device': hm / dm,
                'device_faster_by_more_than_5_spreads': bool(hm - dm > 5 * spread), 'host_faster_by_more_than_5_spreads': bool(dm - hm > 5 * spread)}
        # the same rows on both routes, in the measures of the tests
        q, st, mode, logp = results['device_%s_n%d' % (mname, SIZES[0])]
        dev = {'q': q[:host_n], 'stats': st[:host_n]}
        out['%s_differences' % mname] = C.differences(dev, results['host_%s_n%d' % (mname, host_n)], x)
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
        raise SystemExit('bench_site_cond needs an MI355X: there is no CPU path')
    for name in args.shapes.split(','):
        line = json.dumps(run(name, max(args.reps, 10), args.warmup, args.host_n))
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, 'a') as fh:
                fh.write(line + '\n')


if __name__ == '__main__':
    main()
