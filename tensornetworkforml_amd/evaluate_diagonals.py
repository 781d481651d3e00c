#!/usr/bin/env python3
"""Evaluate a trained diagonals classifier on the MI355X backend: loads a pickled network (training_diagonals.py --out),
draws a fresh data set of noisy diagonals of the network's size, uploads it once and reports accuracy and mean absolute
error over it through `Network.evaluate` (forward chain, activation, argmax and error reduced on the device).

    python tensornetworkforml_amd/evaluate_diagonals.py [--filename trained_diag_model.dat --n_samples 1000 ...]

The two figures are means over the batches of --batch_size samples, the last one ragged when n_samples is not a multiple.
"""
import argparse
import os
import pickle
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tensornetworkforml_amd  # noqa: E402,F401  (registers the bare module names)
import data_generator as gen   # noqa: E402


def write_spectra(net, path):
    spectra, log_norm = net.bond_spectra()
    out = np.zeros((len(spectra), max(len(s) for s in spectra)))
    for i, s in enumerate(spectra):
        out[i, :len(s)] = s
    np.save(path, out)
    entropy = [float(-(s[s > 0] ** 2 * np.log(s[s > 0] ** 2)).sum()) for s in spectra]
    print('\tlog-norm of the chain: %.6g; largest bond entropy %.4f at bond %d; spectra written to %s'
          % (log_norm, max(entropy), int(np.argmax(entropy)), path))


def compare_models(net, path):
    """cosine and relative distance between the loaded network and the pickled network at `path` (Network.cosine / distance)"""
    with open(path, 'rb') as fh:
        other = pickle.load(fh)
    cos, dist = net.cosine(other), net.distance(other)
    print('\tAgainst %s: cosine %.9f, relative distance |W - V| / |W| %.6g' % (path, cos, dist))
    return cos, dist


def write_samples(net, path, n, cls, seed):
    """n images drawn from the model's own distribution |f|^2 over 8-bit pixels (Network.sample), (n, h, w) where N is a square;
    cls None draws the label with the image.  Prints the mean log-probability per class."""
    X, labels, logp, _ = net.sample(n, classes=cls, seed=seed)
    side = int(round(np.sqrt(net.N)))
    np.save(path, X.reshape(n, side, side) if side * side == net.N else X)
    for c in sorted(set(int(v) for v in labels)):
        sel = labels == c
        print('\tSamples of class %d: %d, mean log p(x%s) %.4f' % (c, int(sel.sum()), ', l' if cls is None else ' | l', float(logp[sel, 0].mean())))
    print('\tSamples written to   ', path, X.shape)
    return X, labels, logp


def _levels8(pixels):
    """(n, N) int32 levels 0 .. 255: integer pixels as they are, pixels in [0, 1] rounded to the nearest of 256 levels"""
    pixels = np.asarray(pixels).reshape(len(pixels), -1)
    lev = pixels if np.issubdtype(pixels.dtype, np.integer) else np.rint(np.clip(pixels, 0.0, 1.0) * 255.0)
    return lev.astype(np.int32)


def known_half(which, side):
    """(side * side,) bool: the pixels --inpaint keeps"""
    r, c = np.divmod(np.arange(side * side), side)
    return {'top': r < side // 2, 'bottom': r >= side // 2, 'left': c < side // 2, 'right': c >= side // 2,
            'checker': (r + c) % 2 == 0}[which]


def write_inpainted(net, path, pixels, labels, n, which, seed):
    """The first n test images rounded to 8 bits, one half kept (`which`), the rest and the label drawn by the model given the kept
    pixels (Network.sample with a mask) -> (n, h, w).  Prints the mean log p(completion | known) and the share of drawn labels
    that equal the true ones."""
    lev = _levels8(pixels)[:n]
    n = len(lev)
    side = int(round(np.sqrt(net.N)))
    if side * side != net.N:
        raise SystemExit('--inpaint needs a square image, the network has N = %d sites' % net.N)
    mask = known_half(which, side)
    X, drawn, logp, _ = net.sample(n, given=lev, mask=mask, seed=seed)
    np.save(path, X.reshape(n, side, side))
    hit = float((drawn == np.asarray(labels)[:n]).mean())
    print('\tInpainted %d images, %s known: mean log p(completion | known) %.4f, drawn labels equal to the true ones %.4f'
          % (n, which, float(logp[:, 0].mean()), hit))
    print('\tInpainted images written to', path, (n, side, side))
    return X, drawn, logp


def print_occluded(net, pixels, labels, fraction, seed, chunk=1024):
    """Hides a seeded random `fraction` of every test image's pixels and prints the accuracy of Network.classify_masked (hidden
    pixels summed out by the model) next to the accuracy of Network.predict on the same images with the hidden pixels set to 0."""
    if not 0.0 <= fraction < 1.0:
        raise SystemExit('--occluded takes a fraction in [0, 1)')
    lev = _levels8(pixels)
    labels = np.asarray(labels)
    known = np.random.default_rng(seed).random(lev.shape) >= fraction
    pred = np.concatenate([net.classify_masked(lev[i:i + chunk], known[i:i + chunk])[0] for i in range(0, len(lev), chunk)])
    zeroed = np.where(known, lev, 0) / 255.0
    f = np.concatenate([net.predict(gen.psi(zeroed[i:i + chunk], net.D)).elem for i in range(0, len(lev), chunk)], axis=1)
    acc_m, acc_z = float((pred == labels).mean()), float((f.argmax(axis=0) == labels).mean())
    print('\tOccluded %.2f of the pixels of %d images: accuracy with hidden pixels summed out %.4f, with hidden pixels set to 0 %.4f'
          % (fraction, len(lev), acc_m, acc_z))
    return acc_m, acc_z


def write_inpainted_mean(net, path, pixels, n, which, seed):
    """The first n test images rounded to 8 bits, one half kept (`which`), every hidden pixel the model's posterior mean given the
    kept ones (Network.expected_image) -> (n, h, w).  Prints the mean absolute error on the hidden pixels beside that of one drawn
    completion (Network.sample with the same mask), and the mean posterior standard deviation there."""
    lev = _levels8(pixels)[:n]
    n = len(lev)
    side = int(round(np.sqrt(net.N)))
    if side * side != net.N:
        raise SystemExit('--inpaint-mean needs a square image, the network has N = %d sites' % net.N)
    mask = known_half(which, side)
    img, std = net.expected_image(lev, mask)
    drawn, _, _, _ = net.sample(n, given=lev, mask=mask, seed=seed)
    np.save(path, img.reshape(n, side, side))
    truth = lev[:, ~mask] / 255.0
    print('\tPosterior mean of %d images, %s known: mean absolute error on the hidden pixels %.4f, of one drawn completion %.4f, '
          'mean posterior std %.4f' % (n, which, float(np.abs(img[:, ~mask] - truth).mean()), float(np.abs(drawn[:, ~mask] - truth).mean()),
                                       float(std[:, ~mask].mean())))
    print('\tPosterior means written to', path, (n, side, side))
    return img, std


def write_surprise(net, path, pixels, n):
    """-log p(x_i | all other pixels) of every pixel of the first n test images rounded to 8 bits (Network.pixel_surprise) -> (n, h, w)
    where N is a square.  Prints the mean negative log pseudo-likelihood per image."""
    lev = _levels8(pixels)[:n]
    sur = net.pixel_surprise(lev)
    side = int(round(np.sqrt(net.N)))
    np.save(path, sur.reshape(len(lev), side, side) if side * side == net.N else sur)
    print('\tSurprise maps of %d images: mean -log pseudo-likelihood %.4f (%.4f per pixel)' % (len(lev), float(sur.sum(1).mean()), float(sur.mean())))
    print('\tSurprise maps written to', path, sur.shape)
    return sur


def write_mutual_information(net, path):
    """The (N, N) map of I(x_i; x_j) in nats under the model, the label summed, the entropies on the diagonal
    (Network.mutual_information).  Prints the mean over the pairs at distance |i - j| = 1, 2, 4, ... along the chain and the ten
    sites of largest I(x_i; l) (Network.pixel_label_information)."""
    mi = net.mutual_information()
    np.save(path, mi)
    dist = 1
    while dist < net.N:
        print('\tMutual information at distance %4d: mean %.3e nats over %d pairs' % (dist, float(np.diagonal(mi, dist).mean()), net.N - dist))
        dist *= 2
    info = net.pixel_label_information()
    top = np.argsort(-info, kind='stable')[:10]
    print('\tSites of largest I(x_i; l): ' + ', '.join('%d (%.3e)' % (int(i), float(info[i])) for i in top))
    print('\tMutual information map written to', path, mi.shape)
    return mi, info


def run_masked_arguments(net, args, pixels, labels):
    if args.mutual_info:
        write_mutual_information(net, args.mutual_info)
    if args.inpaint:
        write_inpainted(net, args.inpaint, pixels, labels, args.sample_n, args.inpaint_known, args.seed)
    if args.inpaint_mean:
        write_inpainted_mean(net, args.inpaint_mean, pixels, args.sample_n, args.inpaint_known, args.seed)
    if args.surprise:
        write_surprise(net, args.surprise, pixels, args.sample_n)
    if args.occluded is not None:
        print_occluded(net, pixels, labels, args.occluded, args.seed)


def add_sample_arguments(ap):
    ap.add_argument('--sample', metavar='OUT.npy', default=None, help="write images drawn from the model's distribution |f|^2 over 8-bit pixels (Network.sample)")
    ap.add_argument('--sample-n', dest='sample_n', type=int, default=64, help='number of images of --sample')
    ap.add_argument('--sample-class', dest='sample_class', type=int, default=None, help='condition the images on this class (default: draw the label too)')
    ap.add_argument('--seed', type=int, default=0, help='seed of the uniforms of --sample')
    ap.add_argument('--log-prob', dest='log_prob', action='store_true',
                    help='print the mean log p(x, y) of the test set under the model, pixels rounded to 8 bits (Network.log_prob)')
    ap.add_argument('--inpaint', metavar='OUT.npy', default=None,
                    help='keep one half of the first --sample-n test images (8-bit pixels) and let the model draw the rest and the label')
    ap.add_argument('--inpaint-known', dest='inpaint_known', choices=['top', 'bottom', 'left', 'right', 'checker'], default='top',
                    help='the pixels --inpaint and --inpaint-mean keep')
    ap.add_argument('--inpaint-mean', dest='inpaint_mean', metavar='OUT.npy', default=None,
                    help="keep one half of the first --sample-n test images and fill the rest with the model's posterior mean per pixel "
                         '(Network.expected_image); prints its error on the hidden pixels beside that of one drawn completion')
    ap.add_argument('--surprise', metavar='OUT.npy', default=None,
                    help='write -log p(x_i | all other pixels) per pixel of the first --sample-n test images (Network.pixel_surprise)')
    ap.add_argument('--mutual-info', dest='mutual_info', metavar='OUT.npy', default=None,
                    help='write the map of the mutual information I(x_i; x_j) of every pair of pixels under the model (Network.mutual_information); '
                         'prints its mean by distance along the chain and the ten pixels that carry most information about the class')
    ap.add_argument('--occluded', metavar='FRACTION', type=float, default=None,
                    help='hide a seeded random FRACTION of every test image and print the accuracy of Network.classify_masked next to '
                         'that of the classifier on the same images with the hidden pixels set to 0')


def print_log_prob(net, pixels, labels, chunk=4096):
    """mean log p(x, y) over a data set: integer pixels are levels 0 .. 255, pixels in [0, 1] are rounded to the nearest of 256 levels"""
    lev = _levels8(pixels)
    labels = np.asarray(labels)
    lp = np.concatenate([net.log_prob(lev[i:i + chunk], classes=labels[i:i + chunk], joint=True)[0] for i in range(0, len(lev), chunk)])
    print('\tMean log p(x, y):     %.4f over %d samples (%.4f per pixel)' % (float(lp.mean()), len(lp), float(lp.mean()) / net.N))
    return lp


def main(argv=None):
    ap = argparse.ArgumentParser(description='Evaluate a trained Tensor Network on a generated dataset of diagonals')
    ap.add_argument('--filename', type=str, default='trained_diag_model.dat', help='Pickled network to load')
    ap.add_argument('--n_samples', type=int, default=1000, help='Number of samples to generate')
    ap.add_argument('--sigma', type=float, default=0.6, help='Sigma of the noise added to the dataset')
    ap.add_argument('--batch_size', type=int, default=128, help='Samples per evaluation batch')
    ap.add_argument('--features', action='store_true', help='upload host-embedded features instead of pixels')
    ap.add_argument('--spectra', metavar='OUT.npy', default=None,
                    help='write the normalised Schmidt spectrum of every bond, (N - 1, largest rank), zero-padded (Network.bond_spectra)')
    ap.add_argument('--compare', metavar='OTHER.dat', default=None,
                    help='print the cosine and the relative distance between this model and another pickled one (same N, D, L and label position)')
    ap.add_argument('--scaled-chains', dest='scaled_chains', action='store_true',
                    help='carry a power-of-two exponent per sample along the chains (Network.scaled_chains): for a model whose partial products leave float32')
    add_sample_arguments(ap)
    args = ap.parse_args(argv)

    with open(args.filename, 'rb') as fh:
        net = pickle.load(fh)
    net.any_position = True        # a model saved mid-sweep carries its label inside the chain
    net.scaled_chains = args.scaled_chains
    linear_dim = int(round(np.sqrt(net.N)))
    if linear_dim * linear_dim != net.N:
        raise SystemExit('the network has N = %d sites, which is not a square image' % net.N)
    data, label = gen.create_dataset(args.n_samples, linear_dim, args.sigma)
    _, _, _, test_loader = gen.prepare_device_dataset(net, data, label, 0, 0, 1, 1, args.batch_size, D=net.D,
                                                      pixels=not args.features)
    acc, mae = net.evaluate(test_loader)
    if args.spectra:
        write_spectra(net, args.spectra)
    if args.compare:
        compare_models(net, args.compare)
    if args.sample:
        write_samples(net, args.sample, args.sample_n, args.sample_class, args.seed)
    if args.log_prob:
        print_log_prob(net, data, label)
    run_masked_arguments(net, args, data, label)
    print('\tAccuracy:            ', acc)
    print('\tMean Absolute Error: ', mae)
    return acc, mae


if __name__ == '__main__':
    main()
