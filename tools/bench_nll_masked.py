#!/usr/bin/env python3
"""Wall time of whole Context.nll_masked_grad calls at N = 784, bond 20 with 2 labels (C3) and bond 50 with
10 labels (C5), K = 256 levels, for n = 64 and 1024 samples, with the bottom half of the pixels known and with a random half known
(per sample), every third sample unlabelled: the gradient call and the value-only call; the full mask beside Context.nll_grad on
the same images for orientation; and the route through the host on the same context in the same run: tnml_get_cores and the
float64 NumPy statement of tests/nll_masked_reference.py on `--host-n` samples, SCALED per sample (the keys say so).

The network and the timing are those of tools/bench_site_cond.py: a near-isometric chain calibrated on a small batch, the label on
site 0; images and labels drawn from the model itself by Context.sample; time.perf_counter around the whole Python call (it ends
with the outputs on the host), after `--warmup` untimed rounds, `--reps` times (at least ten), all calls alternating within a
round; median and spread (max - min); a route is called faster only when the difference of the per-sample medians exceeds five
times the larger spread -- whichever way it comes out.  `--stack-gib`: the budget of
tnml_set_sample_stack_bytes for the run (a tile of C5 takes 63 MB of stack and partial gradient).  One JSON line per shape on
stdout and, with --out, appended to a file.

    python tools/bench_nll_masked.py --out profiles/r31_bench_nll_masked.json
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
import nll_masked_reference as M  # noqa: E402
import orthogonalize_reference as R  # noqa: E402
import sample_reference as S  # noqa: E402
from bench_sample_masked import SHAPES, K, stats  # noqa: E402
from tensornetworkforml_amd import _hip  # noqa: E402


def run(name, sizes, reps, warmup, host_n, stack_gib):
    N, Mb, L = SHAPES[name]
    D, l = 2, 0
    rng = np.random.default_rng(1)
    W = R.make_cores(N, D, L, [Mb] * (N - 1), l, rng, R.features(rng, 8, N, D))
    ctx = _hip.Context(N, D, L, Mb, 8)
    ctx.set_any_position(True)
    ctx.set_cores(A.as32(W), l)
    ctx.set_sample_stack_bytes(int(stack_gib * 2 ** 30))
    _, phi, w = S.grid(K, D)
    nmax = max(sizes)
    known, labels, _ = ctx.sample(nmax, phi, w, seed=7)
    classes = np.where(np.arange(nmax) % 3 == 1, -1, labels).astype(np.int32)
    masks = {'bottom': np.arange(N) >= N // 2, 'random': rng.random((nmax, N)) < 0.5}
    Sg = S.gram(phi, w)
    X = phi[known].astype(np.float32)

    def rows(mask, n):
        return mask if mask.ndim == 1 else mask[:n]

    def host(mask):
        def call():
            cs, _, lp = ctx.get_cores()
            return M.masked_gradient(A.as64(cs), lp, phi, w, classes[:host_n], rows(mask, host_n), known[:host_n])
        return call

    calls = {}
    for mname, mask in masks.items():
        for n in sizes:
            calls['grad_%s_n%d' % (mname, n)] = lambda n=n, mask=mask: ctx.nll_masked_grad(n, phi, w, rows(mask, n), known[:n], classes[:n], want=('G',))
            calls['value_%s_n%d' % (mname, n)] = lambda n=n, mask=mask: ctx.nll_masked_grad(n, phi, w, rows(mask, n), known[:n], classes[:n], want=())
        calls['host_scaled_%s_n%d' % (mname, host_n)] = host(mask)
    for n in sizes:
        calls['grad_full_n%d' % n] = lambda n=n: ctx.nll_masked_grad(n, phi, w, np.ones(N, dtype=bool), known[:n], labels[:n], want=('G',))
        calls['nll_grad_n%d' % n] = lambda n=n: ctx.nll_grad(X[:n], labels[:n], Sg)
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
    out = {'bench': 'nll_masked', 'shape': name, 'N': N, 'bond': Mb, 'L': L, 'D': D, 'l_pos': l, 'K': K, 'host_n': host_n,
           'stack_gib': stack_gib, 'timing': 'time.perf_counter around whole calls, outputs on the host; host route scaled per sample'}
    for k in calls:
        out[k] = stats(times[k])
    for mname in masks:
        h = out['host_scaled_%s_n%d' % (mname, host_n)]
        for n in sizes:
            d = out['grad_%s_n%d' % (mname, n)]
            dm, hm = d['median_ms'] / n, h['median_ms'] / host_n
            spread = max(d['spread_ms'] / n, h['spread_ms'] / host_n)
            out['%s_n%d_per_sample_ms' % (mname, n)] = {
                'device': dm, 'host_scaled': hm, 'host_over_device': hm / dm,
                'device_faster_by_more_than_5_spreads': bool(hm - dm > 5 * spread), 'host_faster_by_more_than_5_spreads': bool(dm - hm > 5 * spread)}
    # the full mask on both device routes: the same gradient
    n = sizes[0]
    Gm, Gn = results['grad_full_n%d' % n][0], results['nll_grad_n%d' % n][0]
    out['full_mask_against_nll_grad'] = max(float(np.abs(a.astype(np.float64) - b).max()) for a, b in zip(Gm, Gn)) / max(float(np.abs(b).max()) for b in Gn)
    ctx.close()
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--shapes', default='c3,c5')
    ap.add_argument('--sizes', default='64,1024')
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--host-n', dest='host_n', type=int, default=2)
    ap.add_argument('--stack-gib', dest='stack_gib', type=float, default=32.0)
    ap.add_argument('--out', default=None)
    args = ap.parse_args(argv)
    if _hip.device_count() < 1:
        raise SystemExit('bench_nll_masked needs an MI355X: there is no CPU path')
    sizes = tuple(int(v) for v in args.sizes.split(','))
    for name in args.shapes.split(','):
        line = json.dumps(run(name, sizes, max(args.reps, 10), args.warmup, args.host_n, args.stack_gib))
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, 'a') as fh:
                fh.write(line + '\n')


if __name__ == '__main__':
    main()
