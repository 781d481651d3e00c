#!/usr/bin/env python3
"""Diagonals classifier on the MI355X backend: the counterpart of the reference's
training_diagonals.py (same flags and defaults, training_diagonals.py:33-44; same outputs: a pickled
network and, when matplotlib is available, the accuracy / MAE curves).

    python tensornetworkforml_amd/training_diagonals.py [--M 10 --n_epochs 5 ...]
"""
import argparse
import os
import pickle
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tensornetworkforml_amd  # noqa: E402,F401  (registers the bare module names)
import data_generator as gen   # noqa: E402
import Network_class as tn     # noqa: E402


def train_missing(net, data, label, train_idx, val_idx, args):
    """Likelihood training from incomplete data: every batch loses a random fraction --missing of its pixels
    and --unlabelled of its labels, and takes one Network.nll_step_masked step; after every epoch the validation accuracy of
    classify_masked under the same occlusion.  -> (masked NLL (n_epochs, n_batches) before every step, validation accuracy)"""
    rng = np.random.default_rng(0)
    lev = np.rint(np.clip(data.reshape(len(data), -1), 0.0, 1.0) * 255.0).astype(np.int32)
    label = np.asarray(label, dtype=np.int32)
    net.configure_optimizer(args.optimizer)
    hist, val_acc = [], []
    for epoch in range(args.n_epochs):
        row = []
        for idx in train_idx:
            idx = np.asarray(idx)
            mask = rng.random((len(idx), net.N)) >= args.missing
            y = np.where(rng.random(len(idx)) < args.unlabelled, -1, label[idx]).astype(np.int32)
            row.append(net.nll_step_masked(lev[idx], mask, y, lr=args.lr, weight_dec=args.L2_decay, renorm=args.renorm)[0])
        hist.append(row)
        good = total = 0
        for idx in val_idx:
            idx = np.asarray(idx)
            pred, _ = net.classify_masked(lev[idx], rng.random((len(idx), net.N)) >= args.missing)
            good += int((pred == label[idx]).sum())
            total += len(idx)
        val_acc.append(good / max(total, 1))
        print('Epoch %d/%d - masked NLL : %.4f - val accuracy under occlusion: %.4f' % (epoch, args.n_epochs, float(np.mean(row)), val_acc[-1]))
    return np.array(hist), val_acc


def main(argv=None):
    ap = argparse.ArgumentParser(description='Train the Tensor Network to classify the dataset of diagonals')
    ap.add_argument('--n_samples', type=int, default=5000, help='Number of samples to generate')
    ap.add_argument('--linear_dim', type=int, default=8, help='Size of both dimensions of the samples')
    ap.add_argument('--sigma', type=float, default=0.7, help='Sigma of the noise added to the dataset')
    ap.add_argument('--n_train_batch', type=int, default=1, help='Number of batches the training set is split in')
    ap.add_argument('--M', type=int, default=10, help='Size of the bond between tensors of the network')
    ap.add_argument('--n_epochs', type=int, default=5, help='Number of epochs')
    ap.add_argument('--lr', type=float, default=0.01, help='Learning Rate')
    ap.add_argument('--L2_decay', type=float, default=1, help='Weight decay value for L2 regularization')
    ap.add_argument('--act_fn', type=str, default='softmax')
    ap.add_argument('--loss_fn', type=str, default='full_cross_ent')
    ap.add_argument('--trunc', type=str, default='reference', choices=['reference', 'fixed'],
                    help="truncation policy of the SVD split ('reference' = the original's rule)")
    ap.add_argument('--D', type=int, default=2, help='Local feature dimension (components of the feature map)')
    ap.add_argument('--resident', action='store_true',
                    help='upload the data set once and train from index batches formed on the device (Network.train_resident)')
    ap.add_argument('--steps-per-batch', dest='steps_per_batch', type=int, default=None, metavar='K',
                    help='change the batch every K sweep steps instead of every sweep (needs --resident)')
    ap.add_argument('--optimizer', type=str, default=None, choices=['sgd', 'adam'],
                    help='gradient descent over all cores at fixed bonds instead of sweeps (Network.train_gradient; needs --resident)')
    ap.add_argument('--objective', type=str, default='loss', choices=['loss', 'nll'],
                    help="nll: fit the model's own distribution p(x, l) by gradient descent on the negative log-likelihood "
                         '(Network.train_generative; needs --resident; --optimizer defaults to sgd)')
    ap.add_argument('--no-renorm', dest='renorm', action='store_false',
                    help='likelihood steps without the renormalisation of the cores (needs --objective nll)')
    ap.add_argument('--method', type=str, default='gradient', choices=['gradient', 'sweep'],
                    help='sweep: likelihood training by two-site sweeps whose SVD sets every bond (Network.nll_sweep; needs --objective nll)')
    ap.add_argument('--max-bond', dest='max_bond', type=int, default=None, metavar='M',
                    help='largest bond a likelihood sweep may keep (default --M; needs --method sweep)')
    ap.add_argument('--threshold', type=float, default=1.0, metavar='T',
                    help='adaptive truncation threshold of a likelihood sweep in (0, 1] (needs --method sweep)')
    ap.add_argument('--compress', type=int, default=None, metavar='M',
                    help='after training, cut every bond to M on its Schmidt decomposition (Network.compress; needs --resident)')
    ap.add_argument('--scaled-chains', dest='scaled_chains', action='store_true',
                    help='gradient training on range-safe chains (Network.scaled_chains; needs --resident --optimizer)')
    ap.add_argument('--missing', type=float, default=None, metavar='F',
                    help='likelihood training from incomplete data: hide a random fraction F of the pixels of every batch, summed out '
                         'exactly (Network.nll_step_masked in a host loop; needs --objective nll; pixels are put on a grid of 256 levels)')
    ap.add_argument('--unlabelled', type=float, default=0.0, metavar='F2',
                    help='with --missing: hide the label of a random fraction F2 of the samples of every batch as well')
    ap.add_argument('--out', type=str, default='trained_diag_model.dat')
    args = ap.parse_args(argv)
    if args.compress is not None and not args.resident:
        ap.error('--compress needs --resident')
    if args.optimizer is not None and not args.resident:
        ap.error('--optimizer needs --resident')
    if args.objective == 'nll' and not args.resident:
        ap.error('--objective nll needs --resident')
    if not args.renorm and args.objective != 'nll':
        ap.error('--no-renorm needs --objective nll')
    if args.objective == 'nll' and args.optimizer is None:
        args.optimizer = 'sgd'
    if args.missing is not None and (args.objective != 'nll' or args.method != 'gradient'):
        ap.error('--missing needs --objective nll with --method gradient')
    if args.missing is not None and not (0.0 <= args.missing < 1.0 and 0.0 <= args.unlabelled <= 1.0):
        ap.error('--missing takes a fraction in [0, 1), --unlabelled one in [0, 1]')
    if args.unlabelled and args.missing is None:
        ap.error('--unlabelled needs --missing')
    if args.method == 'sweep' and args.objective != 'nll':
        ap.error('--method sweep needs --objective nll')
    if (args.max_bond is not None or args.threshold != 1.0) and args.method != 'sweep':
        ap.error('--max-bond and --threshold need --method sweep')
    if args.scaled_chains and args.optimizer is None:
        ap.error('--scaled-chains needs --resident --optimizer')
    if args.steps_per_batch is not None and not args.resident:
        ap.error('--steps-per-batch needs --resident')

    train_batch = int(args.n_samples * 0.8 / args.n_train_batch)
    data, label = gen.create_dataset(args.n_samples, args.linear_dim, args.sigma)
    if args.resident:
        # the calibration batch is the first batch a training pass would draw, embedded on the host; everything after it is
        # formed on the device from the pixels uploaded once
        tr_idx, _, _ = gen.split_indices(len(data), 1, 0.2)
        x_cal = gen.psi(data.reshape(len(data), -1)[next(iter(gen.IndexLoader(tr_idx, train_batch, drop_last=True)))], args.D)
    else:
        train_loader, val_loader, _ = gen.prepare_dataset(data, label, 1, 0.2, train_batch, 128, 128, D=args.D)
        x_cal = next(iter(train_loader)).X
    net = tn.Network(N=args.linear_dim ** 2, M=args.M, D=args.D, L=2, calibration_X=x_cal, normalize=True,
                     act_fn=args.act_fn, loss_fn=args.loss_fn, trunc=args.trunc)
    if args.resident:
        _, train_idx, val_idx, _ = gen.prepare_device_dataset(net, data, label, 1, 0.2, train_batch, 128, 128, D=args.D)
        if args.missing is not None:
            hist, val_acc = train_missing(net, data, label, train_idx, val_idx, args)
            with open(args.out, 'wb') as fh:
                pickle.dump(net, fh)
            print('masked NLL per epoch:', ['%.4f' % v for v in hist.mean(axis=1)])
            print('validation accuracy of classify_masked per epoch:', ['%.4f' % v for v in val_acc])
            return val_acc, hist
        if args.objective == 'nll':
            net.scaled_chains = args.scaled_chains
            val_nll, nll_hist = net.train_generative(train_idx, val_idx, lr=args.lr, n_epochs=args.n_epochs, weight_dec=args.L2_decay,
                                                     optimizer=args.optimizer, renorm=args.renorm, method=args.method,
                                                     max_bond=args.max_bond, threshold=args.threshold)
            with open(args.out, 'wb') as fh:
                pickle.dump(net, fh)
            print('validation NLL per epoch:', ['%.4f' % v for v in val_nll])
            return val_nll, nll_hist
        if args.optimizer is not None:
            net.scaled_chains = args.scaled_chains
            val_acc, var_hist = net.train_gradient(train_idx, val_idx, lr=args.lr, n_epochs=args.n_epochs, weight_dec=args.L2_decay,
                                                   optimizer=args.optimizer)
        else:
            val_acc, var_hist = net.train_resident(train_idx, val_idx, lr=args.lr, n_epochs=args.n_epochs, weight_dec=args.L2_decay,
                                                   steps_per_batch=args.steps_per_batch)
        if args.compress is not None:
            before = np.mean([net._ctx.eval_indices(idx, net.act_fn, net.T)[0] / len(idx) for idx in val_idx])
            uncompressed = pickle.loads(pickle.dumps(net))          # a host copy of the chain before the cut
            bonds, discarded = net.compress(max_bond=args.compress)
            after = np.mean([net._ctx.eval_indices(idx, net.act_fn, net.T)[0] / len(idx) for idx in val_idx])
            print('compressed to bond %d (largest bond now %d, discarded weight %.3g): validation accuracy %.4f -> %.4f'
                  % (args.compress, max(bonds), float(np.sum(discarded)), before, after))
            print('relative distance |W - W_c| / |W| between the model before and after the compression: %.6g'
                  % uncompressed.distance(net))
    else:
        val_acc, var_hist = net.train(train_loader, val_loader, lr=args.lr, n_epochs=args.n_epochs,
                                      weight_dec=args.L2_decay)
    with open(args.out, 'wb') as fh:
        pickle.dump(net, fh)
    print('validation accuracy per epoch:', ['%.4f' % v for v in val_acc])
    try:
        import matplotlib
        matplotlib.use('Agg')
        import matplotlib.pyplot as plt
    except ImportError:
        print('(matplotlib not installed: curves not drawn)')
        return val_acc, var_hist
    os.makedirs('results', exist_ok=True)
    # (with --steps-per-batch the epochs may differ in their number of steps: var_hist is then a list of one array per epoch)
    xs = np.concatenate([e + np.arange(v.shape[1]) / v.shape[1] for e, v in enumerate(var_hist)])
    for row, name, ylabel in ((0, 'accuracy', 'Accuracy'), (1, 'MAE', '| f(x) - y |')):
        plt.figure()
        plt.plot(xs, np.concatenate([v[row] for v in var_hist]), label='Train ' + name)
        if row == 0:
            plt.plot(np.arange(1, args.n_epochs + 1), val_acc, 'ro', label='Validation acc')
        plt.xlabel('Epoch'); plt.ylabel(ylabel); plt.legend()
        plt.savefig('results/diag_%s.png' % name)
        plt.close()
    return val_acc, var_hist


if __name__ == '__main__':
    main()
