#!/usr/bin/env python3
"""End-to-end epoch time of `Network.train` (host loaders, `prepare_dataset`) against `Network.train_resident` (dataset uploaded
once, index batches formed on the device), on the same network, seed and batches, in ONE process.

Shapes
  headline       N = 784, D = 2, bond 20, 2 labels, trunc='fixed', batch 5000, 20000 training + 5000 validation samples
  binary_mnist   N = 196 with training_binary_MNIST.py's defaults: bond 3, trunc='reference', ten training batches of 1182, validation
                 batches of 128 over 2956 samples

Per shape and path: epoch 0 is discarded (allocations, first-use costs), the median and the spread (max - min) of `--epochs` more are
reported, and the share of the epoch the device spends inside sweeps (tnml_profile_enable(ctx, 2): one event pair per sweep call,
nothing waits inside the timed region).  Then `Network.evaluate` over all 25000 samples of the headline shape against the loop the
parent offers for it (`predict` + host argmax per batch of 5000).  One JSON line per measurement on stdout and, with --out, in a file.

    python tools/bench_train_epoch.py --out profiles/r05_bench_train_epoch.json
"""
import argparse
import contextlib
import io
import json
import os
import pickle
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import tensornetworkforml_amd  # noqa: E402,F401
import data_generator as gen   # noqa: E402
import Network_class as tn     # noqa: E402

SHAPES = {
    # name: (N, M, trunc, train batch, training samples, validation batch, validation samples)
    'headline': (784, 20, 'fixed', 5000, 20000, 5000, 5000),
    'binary_mnist': (196, 3, 'reference', 1182, 11824, 128, 2956),
}
HP = dict(lr=1e-3, weight_dec=1e-3)


def quiet():
    return contextlib.redirect_stdout(io.StringIO())


def synth_pixels(n, N, seed):
    """Sparse pixels in [0, 1] (bench.py's synthetic images: about four in five are zero) and balanced random labels."""
    rng = np.random.default_rng(seed)
    p = rng.random((n, N), dtype=np.float32) * (rng.random((n, N), dtype=np.float32) > 0.81)
    return p.astype(np.float64), rng.integers(0, 2, n)


def time_epochs(net, one_epoch, n_epochs):
    """Wall seconds and device-in-sweeps milliseconds of n_epochs + 1 single-epoch calls; the first one is dropped.  The network's
    device context must exist already (the profile switches are calls on it)."""
    ctx = net._ctx
    wall, dev = [], []
    ctx.profile_enable(2)
    for ep in range(n_epochs + 1):
        np.random.seed(1000 + ep)                   # the same batch order on both paths
        ctx.synchronize()
        ctx.profile_reset()
        t0 = time.perf_counter()
        with quiet():
            one_epoch()
        ctx.synchronize()
        wall.append(time.perf_counter() - t0)
        dev.append(ctx.profile_get(4)[0])
    ctx.profile_enable(0)
    return wall[1:], dev[1:]


def summary(shape, path, wall, dev, extra):
    med = float(np.median(wall))
    rec = dict(bench='train_epoch', shape=shape, path=path, epochs_timed=len(wall), epoch_s_median=med,
               epoch_s_spread=float(max(wall) - min(wall)), epoch_s=[round(w, 6) for w in wall],
               device_sweep_ms_median=float(np.median(dev)), device_busy_share=float(np.median(np.array(dev) / 1e3 / np.array(wall))))
    rec.update(extra)
    return rec


def run_shape(name, n_epochs, emit):
    N, M, trunc, tb, n_train, vb, n_val = SHAPES[name]
    n = n_train + n_val
    pix, label = synth_pixels(n, N, 7)
    sizes = dict(train_batch_size=tb, val_batch_size=vb, test_batch_size=vb)
    val_perc = n_val / n
    np.random.seed(0)
    with quiet():
        train_loader, val_loader, _ = gen.prepare_dataset(pix, label, 1, val_perc, D=2, **sizes)
        x_cal = next(iter(train_loader)).X
        net0 = tn.Network(N=N, M=M, D=2, L=2, calibration_X=x_cal[:512], normalize=True, act_fn='softmax', loss_fn='full_cross_ent',
                          trunc=trunc)
    blob = pickle.dumps(net0)
    del net0
    extra = dict(N=N, bond=M, trunc=trunc, train_batch=tb, train_batches=len(train_loader), val_batch=vb, val_batches=len(val_loader))
    out = {}
    # loader path: the parent's Network.train, unchanged
    net = pickle.loads(blob)
    with quiet():
        net.forward(x_cal[:64])                       # context exists before the first timed call (profile switches need it)
    wall, dev = time_epochs(net, lambda: net.train(train_loader, val_loader, n_epochs=1, **HP), n_epochs)
    out['loader'] = summary(name, 'loader', wall, dev, extra)
    emit(out['loader'])
    cores_loader = net._ctx.get_cores()[0]
    del net
    # resident path, features form: the same float32 numbers the loader path uploads -> the same training, bit for bit
    for form, pixels in (('resident_features', False), ('resident_pixels', True)):
        net = pickle.loads(blob)
        t0 = time.perf_counter()
        with quiet():
            _, tr_idx, va_idx, _ = gen.prepare_device_dataset(net, pix, label, 1, val_perc, D=2, pixels=pixels, **sizes)
        net._ctx.synchronize()
        attach_s = time.perf_counter() - t0
        wall, dev = time_epochs(net, lambda: net.train_resident(tr_idx, va_idx, n_epochs=1, **HP), n_epochs)
        rec = summary(name, form, wall, dev, dict(extra, attach_s=attach_s))
        if not pixels:
            rec['same_cores_as_loader'] = bool(all(np.array_equal(a, b) for a, b in zip(cores_loader, net._ctx.get_cores()[0])))
        out[form] = rec
        emit(rec)
        if name == 'headline' and not pixels:
            bench_evaluate(net, pix, label, emit)
        del net
    return out


def bench_evaluate(net, pix, label, emit, chunk=5000, reps=5):
    """Network.evaluate over every sample of the attached dataset against predict + host argmax per batch of `chunk`."""
    n = len(pix)
    idx = np.arange(n)
    X = gen.psi(pix, 2)                               # what a host loader hands out: float64 features
    t_dev, t_host = [], []
    for _ in range(reps + 1):
        net._ctx.synchronize()
        t0 = time.perf_counter()
        acc_dev, _ = net.evaluate(idx)
        t_dev.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        correct = 0
        for k in range(0, n, chunk):
            correct += int(round(net.accuracy(X[k:k + chunk], label[k:k + chunk], net.predict(X[k:k + chunk])) * len(X[k:k + chunk])))
        t_host.append(time.perf_counter() - t0)
    emit(dict(bench='evaluate', shape='headline', samples=n, evaluate_s_median=float(np.median(t_dev[1:])),
              evaluate_s_spread=float(max(t_dev[1:]) - min(t_dev[1:])), predict_loop_s_median=float(np.median(t_host[1:])),
              predict_loop_s_spread=float(max(t_host[1:]) - min(t_host[1:])), same_correct_count=bool(round(acc_dev * n) == correct)))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--epochs', type=int, default=4, help='timed epochs per path after the discarded first one (>= 3)')
    ap.add_argument('--shapes', default='headline,binary_mnist')
    ap.add_argument('--out', default=None, help='also write the JSON lines to this file')
    args = ap.parse_args(argv)
    assert args.epochs >= 3
    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    results = {s: run_shape(s, args.epochs, emit) for s in args.shapes.split(',')}
    print('\n| shape | path | epoch median (s) | spread (s) | device busy in sweeps |')
    print('|---|---|---|---|---|')
    for s, paths in results.items():
        for p, r in paths.items():
            print('| %s | %s | %.3f | %.3f | %.0f %% |' % (s, p, r['epoch_s_median'], r['epoch_s_spread'], 100 * r['device_busy_share']))
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')
    return results


if __name__ == '__main__':
    main()
