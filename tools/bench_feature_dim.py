"""Sweep-step rate of the generic feature-dimension path (D != 2, per-step launches) at N = 784, b = 5000, L = 2, fixed truncation,
L2 on: D = 3 at M = 20 and D = 4 at M = 16.  Prints one JSON object: device sweep-steps/s, forward / predict ms per call, and the
float64 CPU oracle's steps/s on the same shapes.

    python tools/bench_feature_dim.py [--sweeps 2] [--cpu-steps 20] [--out FILE] [--only D] [--probe]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import mps_oracle as mo                     # noqa: E402
from tensornetworkforml_amd import _hip                 # noqa: E402
from tensornetworkforml_amd import data_generator as gen   # noqa: E402

SHAPES = [(3, 20), (4, 16)]


def problem(N, M, D, L, b, seed=0):
    rng = np.random.default_rng(seed)
    X = gen.psi(rng.random((b, N)) * (rng.random((b, N)) > 0.5), D).astype(np.float32)
    y = rng.integers(0, L, b)
    cores = [c.astype(np.float32) for c in mo.random_cores(N, M, D, L, rng=rng, scale=M * 0.5 * 0.64 * D)]
    return X, y, cores


def run_device(D, M, N, L, b, sweeps):
    X, y, cores = problem(N, M, D, L, b)
    ctx = _hip.Context(N, D, L, M, b)
    ctx.set_cores(cores, 0)
    ctx.set_input(X, y)
    ctx.scale_cores(float(np.exp(-ctx.forward_logabsmax() / N)))
    kw = (1e-2, 1e-3, True, 'softmax', 'full_cross_ent', 0.1, 'fixed')
    # warm-up: one sweep each way
    for _ in range(2):
        ctx.forward(want_f=False)
        ctx.sweep(ctx.l_pos == N - 1, N - 1, True, *kw, want_metrics=False, want_f=False)
    ctx.synchronize()
    ms, steps = 0.0, 0
    for _ in range(sweeps):
        ctx.forward(want_f=False)
        ctx.timer_start()
        ctx.sweep(ctx.l_pos == N - 1, N - 1, True, *kw, want_metrics=False, want_f=False)
        ms += ctx.timer_stop()
        steps += N - 1
    ctx.synchronize()
    reps = 5
    ctx.timer_start()
    for _ in range(reps):
        ctx.forward(want_f=False)
    fwd_ms = ctx.timer_stop() / reps
    t0 = time.perf_counter()
    for _ in range(reps):
        ctx.predict(X)
    pred_ms = (time.perf_counter() - t0) * 1e3 / reps
    ctx.close()
    return dict(steps_per_s=steps / (ms * 1e-3), sweep_ms=ms / sweeps, forward_ms=fwd_ms, predict_ms_host_wall=pred_ms)


def probe_update(D, M, N, L, b):
    """One right sweep step by step with the capture on: per step the Jacobi sweeps and the update kernel's phase stamps
    (TNML_DBG_L2 scalars: [3] sweeps, [4] n, [5..7] cycles before / in / after the Jacobi loop, [8] 100 MHz ticks of the kernel,
    [9] cycles of the Gram matrix), summarised by the short side n."""
    X, y, cores = problem(N, M, D, L, b)
    ctx = _hip.Context(N, D, L, M, b)
    ctx.set_cores(cores, 0)
    ctx.set_input(X, y)
    ctx.scale_cores(float(np.exp(-ctx.forward_logabsmax() / N)))
    ctx.forward(want_f=False)
    ctx.debug_enable(True)
    rows = []
    for j in range(N - 1):
        ctx.sweep(False, 1, j == 0, 1e-2, 1e-3, True, 'softmax', 'full_cross_ent', 0.1, 'fixed', want_metrics=False, want_f=False)
        sc = ctx.step_debug('scalars')
        rows.append([sc[3], sc[4], sc[5], sc[6], sc[7], sc[8], sc[9]])
    ctx.close()
    r = np.array(rows)
    out = {}
    for n in sorted(set(r[:, 1].astype(int))):
        q = r[r[:, 1] == n]
        cyc = q[:, 2] + q[:, 3] + q[:, 4]
        out[str(n)] = dict(steps=int(len(q)), jacobi_sweeps_mean=float(q[:, 0].mean()), jacobi_sweeps_min=int(q[:, 0].min()),
                           jacobi_sweeps_max=int(q[:, 0].max()), kernel_us_mean=float(q[:, 5].mean() / 100.0),
                           kernel_us_min=float(q[:, 5].min() / 100.0), kernel_us_max=float(q[:, 5].max() / 100.0),
                           share_before_jacobi=float((q[:, 2] / cyc).mean()), share_gram=float((q[:, 6] / cyc).mean()),
                           share_jacobi=float((q[:, 3] / cyc).mean()), share_after_jacobi=float((q[:, 4] / cyc).mean()),
                           us_per_jacobi_sweep=float((q[:, 5] / 100.0 * q[:, 3] / cyc / np.maximum(q[:, 0], 1)).mean()))
    return out


def run_oracle(D, M, N, L, b, n_steps):
    X, y, cores = problem(N, M, D, L, b)
    st = mo.MPSState(N, D, L, M, [c.astype(np.float64) for c in cores])
    Xd = X.astype(np.float64)
    mo.calibrate(st, Xd)
    f = mo.forward(st, Xd)
    y1h = mo.one_hot(y, L)
    st.Lenv = {}
    t0 = time.perf_counter()
    for _ in range(n_steps):
        f = mo.sweep_step(st, f, y1h, 1e-2, 1e-3, L2_flag=True, left_dir=False, act_fn='softmax', loss_fn='full_cross_ent',
                          T=0.1, trunc='fixed')
    return n_steps / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sweeps', type=int, default=2)
    ap.add_argument('--cpu-steps', type=int, default=20)
    ap.add_argument('--only', type=int, default=0, help='run only this D')
    ap.add_argument('--probe', action='store_true', help='also one sweep step by step with the update kernel\'s phase stamps')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    N, L, b = 784, 2, 5000
    res = dict(N=N, L=L, b=b, trunc='fixed', l2=True, path='generic-D per-step launches', results=[])
    for D, M in SHAPES:
        if a.only and D != a.only:
            continue
        r = dict(D=D, M=M, short_side=min(D * M, D * M * L))
        r.update(run_device(D, M, N, L, b, a.sweeps))
        if a.probe:
            r['update_kernel_by_short_side'] = probe_update(D, M, N, L, b)
        if a.cpu_steps > 0:
            r['cpu_oracle_steps_per_s'] = run_oracle(D, M, N, L, b, a.cpu_steps)
        res['results'].append(r)
        print(json.dumps(r), file=sys.stderr, flush=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
