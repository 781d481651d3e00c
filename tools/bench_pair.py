#!/usr/bin/env python3
"""Wall time of whole Context.pair_marginals calls that end with the mutual-information map on the host at
N = 784, bond 20 with 2 labels (C3) and bond 50 with 10 labels (C5), all 784 rows (306 936 pairs), the label summed, K = 256 and
K = 16 levels, beside the route through the host on the same context in the same run: tnml_get_cores and the float64 NumPy
reference of tests/pair_reference.py on `--host-rows` rows spread evenly over the chain (their mean number of pairs is the mean over
all rows), scaled to all rows.

The network, the timing and the rule are those of tools/bench_site_cond.py: a near-isometric chain, the label on site 0;
time.perf_counter around the whole Python call, after `--warmup` untimed rounds, `--reps` times (at least ten), the device calls
and the host route alternating within a round (`--host-reps` ends the host route after that many timed rounds and drops its
warm-up: one host call at C5 takes a minute); median and spread (max - min); a route is called faster only when the difference of
the medians for all rows exceeds five times the larger spread -- whichever way it comes out.  One JSON line
per shape on stdout and, with --out, appended to a file.

    python tools/bench_pair.py --out profiles/r27_bench_pair.json
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
import pair_reference as P  # noqa: E402
import sample_reference as S  # noqa: E402
from bench_sample_masked import SHAPES, stats  # noqa: E402
from tensornetworkforml_amd import _hip  # noqa: E402

LEVELS = (256, 16)


def mi_map(stats1, st):
    out = np.triu(st[..., 2], 1)
    out = out + out.T
    out[np.diag_indices_from(out)] = stats1[:, 2]
    return out


def run(name, reps, warmup, host_rows, host_reps):
    N, Mb, L = SHAPES[name]
    D, l = 2, 0
    rng = np.random.default_rng(1)
    W = R.make_cores(N, D, L, [Mb] * (N - 1), l, rng, R.features(rng, 8, N, D))
    ctx = _hip.Context(N, D, L, Mb, 8)
    ctx.set_any_position(True)
    ctx.set_cores(A.as32(W), l)
    rows = np.arange(N, dtype=np.int32)
    some = [int((2 * r + 1) * N / (2 * host_rows)) for r in range(host_rows)]
    calls, grids = {}, {}

    def device(K):
        x, phi, w = grids[K]
        _, stats1, _, st = ctx.pair_marginals(phi, w, rows, -1, x, want=('stats1', 'stats'))
        return mi_map(stats1, st)

    def host(K):
        x, phi, w = grids[K]
        cs, _, lp = ctx.get_cores()
        return P.pair_marginals(A.as64(cs), lp, phi, w, x, -1, some)

    for K in LEVELS:
        grids[K] = S.grid(K, D)
        calls['device_K%d' % K] = lambda K=K: device(K)
        calls['host_K%d_rows%d' % (K, host_rows)] = lambda K=K: host(K)
    times = {k: [] for k in calls}
    results = {}
    for rep in range(warmup + reps):
        for k, call in calls.items():
            if k.startswith('host') and (rep >= warmup + host_reps or (rep < warmup and host_reps < reps)):
                continue                                             # (a shortened host route has no warm-up either: it is NumPy)
            ctx.synchronize()
            t0 = time.perf_counter()
            results[k] = call()
            ms = 1e3 * (time.perf_counter() - t0)
            if rep >= warmup:
                times[k].append(ms)
            print('%s round %d of %d: %s %.1f ms' % (name, rep + 1, warmup + reps, k, ms), file=sys.stderr, flush=True)
    out = {'bench': 'pair', 'shape': name, 'N': N, 'bond': Mb, 'L': L, 'D': D, 'l_pos': l, 'rows': N, 'pairs': N * (N - 1) // 2,
           'host_rows': some, 'timing': 'time.perf_counter around whole calls, the MI map on the host'}
    for k in calls:
        out[k] = stats(times[k])
    for K in LEVELS:
        d, h = out['device_K%d' % K], out['host_K%d_rows%d' % (K, host_rows)]
        scale = N / host_rows
        dm, hm = d['median_ms'], h['median_ms'] * scale
        spread = max(d['spread_ms'], h['spread_ms'] * scale)
        out['K%d_all_rows_ms' % K] = {
            'device': dm, 'host_scaled': hm, 'host_over_device': hm / dm,
            'device_faster_by_more_than_5_spreads': bool(hm - dm > 5 * spread), 'host_faster_by_more_than_5_spreads': bool(dm - hm > 5 * spread)}
        ref = results['host_K%d_rows%d' % (K, host_rows)]
        mi = results['device_K%d' % K]
        out['K%d_mi_difference' % K] = float(max(np.abs(mi[i, i + 1:] - ref['stats'][r, i + 1:, 2]).max() for r, i in enumerate(some)))
        out['K%d_mean_mi_by_distance' % K] = {str(dist): float(np.diagonal(mi, dist).mean()) for dist in (1, 2, 4, 8, 16, 32, 64)}
    ctx.close()
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--shapes', default='c3,c5')
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--host-rows', dest='host_rows', type=int, default=4)
    ap.add_argument('--host-reps', dest='host_reps', type=int, default=None,
                    help='timed rounds of the host route (default: --reps; at C5 one host call takes about a minute)')
    ap.add_argument('--out', default=None)
    args = ap.parse_args(argv)
    if _hip.device_count() < 1:
        raise SystemExit('bench_pair needs an MI355X: there is no CPU path')
    for name in args.shapes.split(','):
        reps = max(args.reps, 10)
        line = json.dumps(run(name, reps, args.warmup, args.host_rows, reps if args.host_reps is None else max(1, args.host_reps)))
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, 'a') as fh:
                fh.write(line + '\n')


if __name__ == '__main__':
    main()
