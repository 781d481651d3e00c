#!/usr/bin/env python3
"""Device time of `tnml_forward` with the label at a chain end and inside the chain (tnml_set_any_position):
the launches of one forward -- one chain, or two half-chains and label_meet_kernel, all on the context's stream -- between two
HIP events (tnml_profile_enable(ctx, 1)), median and spread (max - min) of --reps forwards after three discarded ones.

    python tools/probe_forward_inside.py                 # C3 (bond 20, 2 labels, b = 20000) and C5 (bond 50, 10 labels, b = 5000)
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/probe_forward_inside.py      # the meet kernel's own time
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tensornetworkforml_amd import _hip     # noqa: E402

SHAPES = {'c3': (784, 20, 2, 20000), 'c5': (784, 50, 10, 5000)}


def cores_at(N, M, D, L, l, rng):
    scale = M * 0.5 * 0.64 * D
    out = []
    for i in range(N):
        ml, mr = (1 if i == 0 else M), (1 if i == N - 1 else M)
        out.append((rng.random((ml, D, mr, L) if i == l else (ml, D, mr)) / scale).astype(np.float32))
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--shapes', default='c3,c5')
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--out', default=None)
    args = ap.parse_args(argv)
    lines = []
    for name in args.shapes.split(','):
        N, M, L, b = SHAPES[name]
        D = 2
        rng = np.random.default_rng(3)
        p = rng.random((b, N), dtype=np.float32) * (rng.random((b, N), dtype=np.float32) > 0.81)
        X = np.stack([np.sin(np.pi * p / 2), np.cos(np.pi * p / 2)], -1).astype(np.float32)
        ctx = _hip.Context(N, D, L, M, b)
        ctx.set_any_position(True)
        ctx.set_input(X, rng.integers(0, L, b))
        ctx.profile_enable(1)
        for l in (0, 1, N // 2):
            ctx.set_cores(cores_at(N, M, D, L, l, rng), l)
            ms = []
            for r in range(args.reps + 3):
                ctx.profile_reset()
                ctx.forward(want_f=False)
                ctx.synchronize()
                ms.append(ctx.profile_get(0)[0])
            ms = ms[3:]
            rec = dict(probe='forward_inside', shape=name, N=N, bond=M, L=L, b=b, l_pos=l, forward_ms_median=float(np.median(ms)),
                       forward_ms_spread=float(max(ms) - min(ms)), reps=len(ms))
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
        ctx.close()
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
