#!/usr/bin/env python3
"""Wall time of whole Network.sample calls at C3 (N = 784, bond 20, 2 labels) and C5 (bond 50, 10 labels),
K = 256 levels, for n = 16, 256 and 4096 samples with the class given and with the class drawn, beside the route through the host a
caller had before the call existed, on the same context in the same run: tnml_get_cores and the float64 NumPy sampler of
tests/sample_reference.py (environments and walk, vectorised over the samples) at `--host-n` samples, scaled per sample.

The network is a near-isometric chain calibrated on a small batch (tests/orthogonalize_reference.make_cores), the label on site 0.
Every call is timed with time.perf_counter around the whole Python call (it ends with the outputs on the host), after `--warmup`
untimed rounds, `--reps` times (at least ten), the device calls and the host route alternating within a round; median and spread
(max - min) are reported, and the rule of DESIGN.md section 8 is applied to the per-sample times: a route is called faster only when
the difference of the medians exceeds five times the larger spread.  One JSON line per shape on stdout and, with --out, appended to
a file.

    python tools/bench_sample.py --out profiles/r17_bench_sample.json
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
import sample_reference as S  # noqa: E402
import tensornetworkforml_amd as pkg  # noqa: E402
from tensornetworkforml_amd import _hip  # noqa: E402

SHAPES = {'c3': (784, 20, 2), 'c5': (784, 50, 10)}
SIZES = (16, 256, 4096)
K = 256


def stats(ms):
    ms = sorted(ms)
    return {'median_ms': ms[len(ms) // 2] if len(ms) % 2 else 0.5 * (ms[len(ms) // 2 - 1] + ms[len(ms) // 2]),
            'spread_ms': ms[-1] - ms[0], 'min_ms': ms[0], 'reps': len(ms)}


def run(name, reps, warmup, host_n):
    N, M, L = SHAPES[name]
    D, l = 2, 0
    rng = np.random.default_rng(1)
    W = R.make_cores(N, D, L, [M] * (N - 1), l, rng, R.features(rng, 8, N, D))
    net = pkg.Network_class.Network(N, M, D=D, L=L, trunc='fixed')
    net._host_cores, net._l_pos, net._host_newer = A.as64(W), l, True
    net.sample(1)                                                   # creates the context and uploads W
    ctx = net._ctx
    _, phi, w = S.grid(K, D)

    def host(cls):
        def call():
            cs, _, lp = ctx.get_cores()
            classes = np.full(host_n, cls, dtype=np.int32)
            return S.walk(A.as64(cs), lp, phi, w, classes, S.hash_uniforms(3, host_n, N))
        return call

    calls = {}
    for n in SIZES:
        calls['device_given_n%d' % n] = lambda n=n: net.sample(n, classes=1, seed=3)
        calls['device_drawn_n%d' % n] = lambda n=n: net.sample(n, seed=3)
    calls['host_given_n%d' % host_n] = host(1)
    calls['host_drawn_n%d' % host_n] = host(-1)
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
    out = {'bench': 'sample', 'shape': name, 'N': N, 'bond': M, 'L': L, 'D': D, 'l_pos': l, 'K': K, 'host_n': host_n,
           'timing': 'time.perf_counter around whole calls, outputs on the host'}
    for k in calls:
        out[k] = stats(times[k])
    for what in ('given', 'drawn'):
        h = out['host_%s_n%d' % (what, host_n)]
        for n in SIZES:
            d = out['device_%s_n%d' % (what, n)]
            dm, hm = d['median_ms'] / n, h['median_ms'] / host_n
            spread = max(d['spread_ms'] / n, h['spread_ms'] / host_n)
            out['%s_n%d_per_sample_ms' % (what, n)] = {'device': dm, 'host': hm, 'host_over_device': hm / dm,
                                                       'faster_by_more_than_5_spreads': bool(hm - dm > 5 * spread)}
    # the same seed and the same n: the device's draws against the host route's, on the samples the reference calls decidable
    lev, lab, logp = ctx.sample(host_n, phi, w, np.full(host_n, -1, dtype=np.int32), None, None, 3)
    rlev, rlab, rlogp, mg = results['host_drawn_n%d' % host_n]
    ok = S.decidable(mg)
    out['drawn_equal_decidable'] = bool(np.array_equal(lev[ok], rlev[ok]) and np.array_equal(lab[ok], rlab[ok]))
    out['drawn_decidable'] = int(ok.sum())
    out['drawn_dlogp'] = float(np.abs(logp[ok, 0] - rlogp[ok, 0]).max()) if ok.any() else 0.0
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--shapes', default='c3,c5')
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--host-n', dest='host_n', type=int, default=16)
    ap.add_argument('--out', default=None)
    args = ap.parse_args(argv)
    if _hip.device_count() < 1:
        raise SystemExit('bench_sample needs an MI355X: there is no CPU path')
    for name in args.shapes.split(','):
        line = json.dumps(run(name, max(args.reps, 10), args.warmup, args.host_n))
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, 'a') as fh:
                fh.write(line + '\n')


if __name__ == '__main__':
    main()
