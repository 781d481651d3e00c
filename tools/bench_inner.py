#!/usr/bin/env python3
"""Wall time of Network.inner(other) and of Network.add followed by Network.compress at C3 (N = 784, bond 20,
2 labels) and C5 (bond 50, 10 labels), beside the route through the host a caller had before the calls existed, on the same context
in the same run: tnml_get_cores, the float64 NumPy transfer chain (and direct sum / compression) of the reference files under
tests/, tnml_set_cores.

Both networks are near-isometric chains calibrated on a small batch (tests/orthogonalize_reference.make_cores); the second is the
first with every element moved by up to 5 %.  At C5 the second operand of the sum has bond 46: tnml_compress takes bonds up to 96, and
50 + 50 is beyond it (Network_class.combine compresses on the way for that reason).

Every call is timed with time.perf_counter around the whole Python call (it ends with the stream drained), after `--warmup` untimed
rounds, `--reps` times (at least ten), the device and the host route alternating within a round; median and spread (max - min) are
reported.  Every timed sum starts from the same cores (set outside the window).  One JSON line per shape on stdout and, with --out,
appended to a file.

    python tools/bench_inner.py --out profiles/r16_bench_inner.json
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
import tensornetworkforml_amd as pkg  # noqa: E402
from tensornetworkforml_amd import _hip  # noqa: E402

SHAPES = {
    # name: (N, bond, labels, bond of the second operand of the sum)
    'c3': (784, 20, 2, 20),
    'c5': (784, 50, 10, 46),
}


def stats(ms):
    ms = sorted(ms)
    return {'median_ms': ms[len(ms) // 2] if len(ms) % 2 else 0.5 * (ms[len(ms) // 2 - 1] + ms[len(ms) // 2]),
            'spread_ms': ms[-1] - ms[0], 'min_ms': ms[0], 'reps': len(ms)}


def network_of(cores, l, M, D, L):
    net = pkg.Network_class.Network(len(cores), M, D=D, L=L, trunc='fixed')
    net._host_cores = A.as64(cores)
    net._l_pos = l
    net._host_newer = True
    return net


def run(name, reps, warmup):
    N, M, L, M2 = SHAPES[name]
    D, l = 2, 0
    rng = np.random.default_rng(1)
    X = R.features(rng, 8, N, D)
    W = R.make_cores(N, D, L, [M] * (N - 1), l, rng, X)
    V = A.as64(A.as32([c * (1.0 + 0.05 * rng.uniform(-1, 1, c.shape)) for c in W]))
    V2 = V if M2 == M else R.make_cores(N, D, L, [M2] * (N - 1), l, rng, X)
    net, other, other2 = network_of(W, l, M + M2, D, L), network_of(V, l, M, D, L), network_of(V2, l, M2, D, L)
    net.inner(other)                                                # creates the context and uploads W
    ctx = net._ctx
    start = A.as32(W)

    def host_inner():
        cs, _, lp = ctx.get_cores()
        return A.inner3(A.as64(cs), V, lp)

    def host_add_compress():
        cs, _, lp = ctx.get_cores()
        unit, _, disc, logn = R.compress(A.direct_sum(A.as64(cs), V2, lp, 0.5, 0.5), lp, M, 1.0)
        ctx.set_cores(A.as32(R.with_gauge(unit, logn)[0]), lp)
        return disc

    def device_add_compress():
        net.add(other2, 0.5, 0.5)
        return net.compress(max_bond=M)[1]

    calls = {
        'device_inner': lambda: net.inner(other),
        'host_inner': host_inner,
        'device_add_compress': device_add_compress,
        'host_add_compress': host_add_compress,
    }
    times = {k: [] for k in calls}
    results = {}
    for rep in range(warmup + reps):
        for k, call in calls.items():
            ctx.set_cores(start, l)
            ctx.synchronize()
            t0 = time.perf_counter()
            results[k] = call()
            ms = 1e3 * (time.perf_counter() - t0)
            if rep >= warmup:
                times[k].append(ms)
    out = {'bench': 'inner', 'shape': name, 'N': N, 'bond': M, 'L': L, 'D': D, 'l_pos': l, 'bond_of_second_summand': M2,
           'timing': 'time.perf_counter around whole Network calls, stream drained'}
    for k in calls:
        out[k] = stats(times[k])
    for what in ('inner', 'add_compress'):
        d, h = out['device_' + what], out['host_' + what]
        out[what + '_host_minus_device_ms'] = h['median_ms'] - d['median_ms']
        out[what + '_faster_by_more_than_5_spreads'] = bool(h['median_ms'] - d['median_ms'] > 5 * max(d['spread_ms'], h['spread_ms']))
    dev, ref = np.array(results['device_inner']), results['host_inner']
    out['inner_dlog_device_minus_host'] = float(np.abs(dev[:, 1] - ref[:, 1]).max())
    out['relative_distance'] = float(np.sqrt(max(0.0, A.distance2(ref))))
    out['discarded_device_minus_host'] = float(np.abs(np.asarray(results['device_add_compress']) - np.asarray(results['host_add_compress'])).max())
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--shapes', default='c3,c5')
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--out', default=None)
    args = ap.parse_args(argv)
    if _hip.device_count() < 1:
        raise SystemExit('bench_inner needs an MI355X: there is no CPU path')
    for name in args.shapes.split(','):
        line = json.dumps(run(name, max(args.reps, 10), args.warmup))
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, 'a') as fh:
                fh.write(line + '\n')


if __name__ == '__main__':
    main()
