#!/usr/bin/env python3
"""Evaluate a trained binary (0 vs 1) MNIST classifier on the MI355X backend: loads a pickled network
(training_binary_MNIST.py --out), prepares the digits 0 / 1 of the MNIST test files the way the training script does (2x2
max-pooling while the network has fewer sites than the images have pixels), uploads them once and reports accuracy and mean
absolute error through `Network.evaluate`.  MNIST is read from local IDX files under --data_dir (nothing is downloaded).
--saliency OUT.npy also writes the saliency maps of the test digits: the gradient of the predicted class's output with respect to
the pixels, (n, h, w), from `Network.input_gradient_indices` (needs the pixels form of the dataset, the default).

    python tensornetworkforml_amd/evaluate_binary_MNIST.py [--filename trained_MNIST_model.dat --data_dir datasets ...]
"""
import argparse
import os
import pickle
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tensornetworkforml_amd  # noqa: E402,F401
import data_generator as gen   # noqa: E402


def pooling(X):
    """2x2 max pooling of a stack of images, as training_binary_MNIST.py prepares them."""
    n, h, w = X.shape
    return X[:, :h - h % 2, :w - w % 2].reshape(n, h // 2, 2, w // 2, 2).max(axis=(2, 4))


def main(argv=None):
    ap = argparse.ArgumentParser(description='Evaluate a trained Tensor Network on the binary MNIST test set')
    ap.add_argument('--filename', type=str, default='trained_MNIST_model.dat', help='Pickled network to load')
    ap.add_argument('--data_dir', type=str, default='datasets')
    ap.add_argument('--batch_size', type=int, default=128, help='Samples per evaluation batch')
    ap.add_argument('--normalise', action='store_true', help='scale pixels to [0, 1] before the feature map (as in training)')
    ap.add_argument('--features', action='store_true', help='upload host-embedded features instead of pixels')
    ap.add_argument('--saliency', metavar='OUT.npy', default=None, help='write d f[predicted class] / d pixel of every test digit, (n, h, w)')
    ap.add_argument('--spectra', metavar='OUT.npy', default=None,
                    help='write the normalised Schmidt spectrum of every bond, (N - 1, largest rank), zero-padded (Network.bond_spectra)')
    ap.add_argument('--compare', metavar='OTHER.dat', default=None,
                    help='print the cosine and the relative distance between this model and another pickled one (same N, D, L and label position)')
    ap.add_argument('--scaled-chains', dest='scaled_chains', action='store_true',
                    help='carry a power-of-two exponent per sample along the chains (Network.scaled_chains): for a model whose partial products leave float32')
    from tensornetworkforml_amd.evaluate_diagonals import add_sample_arguments
    add_sample_arguments(ap)
    args = ap.parse_args(argv)

    with open(args.filename, 'rb') as fh:
        net = pickle.load(fh)
    net.any_position = True        # a model saved mid-sweep carries its label inside the chain
    net.scaled_chains = args.scaled_chains
    _, _, data, labels = gen.get_MNIST_dataset(args.data_dir)
    while data[0].size > net.N and min(data.shape[1:]) >= 2:
        data = pooling(data)
    if data[0].size != net.N:
        raise SystemExit('the network has N = %d sites, the (pooled) images have %d pixels' % (net.N, data[0].size))
    mask = (labels == 0) | (labels == 1)
    data01, labels01 = data[mask], labels[mask]
    if args.normalise:
        data01 = data01 / 255.0
    _, _, _, test_loader = gen.prepare_device_dataset(net, data01, labels01, 0, 0, 1, 1, args.batch_size, D=net.D,
                                                      pixels=not args.features)
    acc, mae = net.evaluate(test_loader)
    print('\tAccuracy:            ', acc)
    print('\tMean Absolute Error: ', mae)
    if args.spectra:
        from tensornetworkforml_amd.evaluate_diagonals import write_spectra
        write_spectra(net, args.spectra)
    if args.compare:
        from tensornetworkforml_amd.evaluate_diagonals import compare_models
        compare_models(net, args.compare)
    if args.sample:
        from tensornetworkforml_amd.evaluate_diagonals import write_samples
        write_samples(net, args.sample, args.sample_n, args.sample_class, args.seed)
    if args.log_prob:
        from tensornetworkforml_amd.evaluate_diagonals import print_log_prob
        print_log_prob(net, data01, labels01)
    if args.inpaint or args.inpaint_mean or args.surprise or args.mutual_info or args.occluded is not None:
        from tensornetworkforml_amd.evaluate_diagonals import run_masked_arguments
        run_masked_arguments(net, args, data01, labels01)
    if args.saliency:
        import numpy as np
        if args.features:
            raise SystemExit('--saliency differentiates through the feature map on the device: it needs the pixels form (drop --features)')
        sal = net.input_gradient_indices(np.arange(len(data01)), wrt='pixels')
        np.save(args.saliency, sal.reshape((len(data01),) + data01.shape[1:]))
        print('\tSaliency maps:       ', args.saliency, sal.shape)
    return acc, mae


if __name__ == '__main__':
    main()
