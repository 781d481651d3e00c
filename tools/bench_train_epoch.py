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

--steps-per-batch K[,K...] measures `train_resident(steps_per_batch=K)` instead, at the headline shape: one context
with the default schedule (a batch per sweep, four batches) and one per K, each on its own copy of the network and the uploaded
dataset, timed in ALTERNATING single-epoch calls.  An epoch of the K schedule draws as many batches of 5000 as bring it to the default
epoch's 4 (N-1) steps (4 at K = 783, 32 at K = 98, 112 at K = 28); segments that end at a chain end are short, so the steps actually
run are reported and the time per step beside the epoch time.  Such an epoch draws its batches from several permutations of the
training samples (`DrawLoader`): it sees a sample more than once.  The default schedule runs in the same build (its launches are the
parent commit's: the call traces of the stand-in runtime are identical).

    python tools/bench_train_epoch.py --steps-per-batch 783,98,28 --out profiles/r07_bench_steps_per_batch.json
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


class DrawLoader:
    """n_batches index batches of batch_size per pass, drawn from `indices` pass after pass of np.random.permutation (an IndexLoader
    that does not stop after one pass over the samples)."""

    def __init__(self, indices, batch_size, n_batches):
        self.indices, self.batch_size, self.n_batches = np.asarray(indices), int(batch_size), int(n_batches)

    def __len__(self):
        return self.n_batches

    def __iter__(self):
        per = len(self.indices) // self.batch_size
        order = None
        for k in range(self.n_batches):
            if k % per == 0:
                order = self.indices[np.random.permutation(len(self.indices))]
            yield order[(k % per) * self.batch_size:(k % per + 1) * self.batch_size]


def run_steps_per_batch(ks, n_epochs, emit):
    """The default schedule and train_resident(steps_per_batch=K) for every K, in alternating single-epoch calls."""
    name = 'headline'
    N, M, trunc, tb, n_train, vb, n_val = SHAPES[name]
    n = n_train + n_val
    pix, label = synth_pixels(n, N, 7)
    sizes = dict(train_batch_size=tb, val_batch_size=vb, test_batch_size=vb)
    val_perc = n_val / n
    np.random.seed(0)
    tr, va, _ = gen.split_indices(n, 1, val_perc)
    x_cal = gen.psi(pix[:512], 2)
    with quiet():
        net0 = tn.Network(N=N, M=M, D=2, L=2, calibration_X=x_cal, normalize=True, act_fn='softmax', loss_fn='full_cross_ent', trunc=trunc)
    blob = pickle.dumps(net0)
    del net0
    runs = []
    for k in [None] + list(ks):
        net = pickle.loads(blob)
        with quiet():
            _, tr_idx, va_idx, _ = gen.prepare_device_dataset(net, pix, label, 1, val_perc, D=2, pixels=True, **sizes)
        if k is not None:
            tr_idx = DrawLoader(tr, tb, max(len(tr_idx), int(round(len(tr_idx) * (N - 1) / k))))
        net._ctx.profile_enable(2)
        runs.append(dict(k=k, net=net, tr=tr_idx, va=va_idx, wall=[], dev=[], steps=[]))
    for ep in range(n_epochs + 1):
        for r in runs:                                 # alternating: one epoch of every schedule per round
            net, ctx = r['net'], r['net']._ctx
            np.random.seed(1000 + ep)
            ctx.synchronize()
            ctx.profile_reset()
            t0 = time.perf_counter()
            with quiet():
                if r['k'] is None:
                    net.train_resident(r['tr'], r['va'], n_epochs=1, **HP)
                else:
                    net.train_resident(r['tr'], r['va'], n_epochs=1, steps_per_batch=r['k'], **HP)
            ctx.synchronize()
            r['wall'].append(time.perf_counter() - t0)
            r['dev'].append(ctx.profile_get(4)[0])
            r['steps'].append(int(ctx.counters()['sweep_steps']))
    out = {}
    for r in runs:
        wall, dev, steps = r['wall'][1:], r['dev'][1:], r['steps'][1:]
        path = 'default' if r['k'] is None else 'steps_per_batch_%d' % r['k']
        rec = summary(name, path, wall, dev, dict(N=N, bond=M, trunc=trunc, train_batch=tb, train_batches=len(r['tr']), val_batch=vb,
                                                  val_batches=len(r['va']), steps_per_batch=r['k'], sweep_steps=steps,
                                                  us_per_step_median=float(np.median(1e6 * np.array(wall) / np.array(steps)))))
        rec['bench'] = 'train_epoch_steps_per_batch'
        out[path] = rec
        emit(rec)
    return {name: out}


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
    ap.add_argument('--steps-per-batch', dest='steps_per_batch', default=None, metavar='K[,K...]',
                    help='measure train_resident(steps_per_batch=K) against the default schedule at the headline shape instead')
    ap.add_argument('--out', default=None, help='also write the JSON lines to this file')
    args = ap.parse_args(argv)
    assert args.epochs >= 3
    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    if args.steps_per_batch:
        results = run_steps_per_batch([int(k) for k in args.steps_per_batch.split(',')], args.epochs, emit)
    else:
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
