"""Optimiser steps over all cores of an MPS in float64 NumPy (test infrastructure): the update rules of
include/tnml.h (TNML_OPT_SGD with the per-core clip and momentum, TNML_OPT_ADAM with decoupled decay) transcribed from their
statement there, on top of oracle.mps_oracle.apply_act_func / compute_loss_derivate / one_hot (the library's training signal) and
tests/core_grad_reference.core_grad_reference (the gradient).  Also the shared test cases of tests/test_gradient_step_host.py (which
checks the conditions on them with this reference alone) and tests/test_gradient_step_gpu.py (which runs them on the device).

lr, weight_dec and T cross the C ABI as float32: the reference rounds them the same way before it computes in float64.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from core_grad_reference import core_grad_reference                                          # noqa: E402
from input_grad_reference import ragged_bonds, scaled_cores                                  # noqa: E402
from oracle.mps_oracle import apply_act_func, compute_loss_derivate, one_hot                 # noqa: E402

ACTS = ('linear', 'sigmoid', 'softmax')
LOSSES = ('MSE', 'cross_entropy', 'full_cross_ent')


def f32(v):
    return float(np.float32(v))


def forward64(cores, l, X):
    """f (L, b) of X (b, N, D) for cores (ml, D, mr[, L]) with the label on site l."""
    b = X.shape[0]
    P = np.ones((b, 1))
    for i in range(l):
        P = np.einsum('ba,bd,adc->bc', P, X[:, i], cores[i])
    Q = np.ones((b, 1))
    for i in range(len(cores) - 1, l, -1):
        Q = np.einsum('adc,bd,bc->ba', cores[i], X[:, i], Q)
    return np.einsum('ba,bd,adcl,bc->lb', P, X[:, l], cores[l], Q)


class GradientStepReference:
    """cores: list of arrays (ml, D, mr[, L]) (taken as float64 copies), label on site l.  step() changes self.cores in place of
    the list and returns what the step saw."""

    def __init__(self, cores, l, kind='sgd', momentum=0.0, betas=(0.9, 0.999), eps=1e-8, clip=True):
        assert kind in ('sgd', 'adam') and not (kind == 'adam' and clip)
        self.cores = [np.array(c, dtype=np.float64) for c in cores]
        self.l, self.kind, self.mu, self.b1, self.b2, self.eps, self.clip = l, kind, float(momentum), betas[0], betas[1], float(eps), bool(clip)
        self.t = 0
        self.vel = [np.zeros_like(c) for c in self.cores]
        self.m = [np.zeros_like(c) for c in self.cores]
        self.v = [np.zeros_like(c) for c in self.cores]

    def signal(self, X, y, act_fn, loss_fn, T):
        """(f, fa, cot, correct, abs_sum) of the batch at the current cores"""
        L = self.cores[self.l].shape[3]
        X = np.asarray(X, dtype=np.float64)
        f = forward64(self.cores, self.l, X)
        fa = apply_act_func(f, act_fn, f32(T))
        y1h = one_hot(y, L)
        cot = compute_loss_derivate(fa, y1h, act_fn, loss_fn, f32(T))
        correct = int((np.argmax(f, axis=0) == np.asarray(y)).sum())
        return f, fa, cot, correct, float(np.abs(y1h - fa).sum())

    def step(self, X, y, lr, wd, act_fn, loss_fn, T):
        lr, wd = f32(lr), f32(wd)
        X = np.asarray(X, dtype=np.float64)
        f, fa, cot, correct, abs_sum = self.signal(X, y, act_fn, loss_fn, T)
        G, _ = core_grad_reference(self.cores, self.l, X, cot)
        ratio = np.zeros(len(self.cores))
        if self.kind == 'adam':
            self.t += 1
        for i, (A, g) in enumerate(zip(self.cores, G)):
            if self.kind == 'sgd':
                d = g - wd * A
                s_A, s_d = np.abs(A).sum(), np.abs(d).sum()
                ratio[i] = s_d / s_A if s_A > 0 else np.inf
                if self.clip and s_d > s_A:
                    d = d * (s_A / s_d)
                if self.mu > 0:
                    self.vel[i] = self.mu * self.vel[i] + d
                    A += lr * self.vel[i]
                else:
                    A += lr * d
            else:
                self.m[i] = self.b1 * self.m[i] + (1 - self.b1) * g
                self.v[i] = self.b2 * self.v[i] + (1 - self.b2) * g * g
                A += lr * ((self.m[i] / (1 - self.b1 ** self.t)) / (np.sqrt(self.v[i] / (1 - self.b2 ** self.t)) + self.eps) - wd * A)
        return dict(f=f, fa=fa, cot=cot, G=G, ratio=ratio, correct=correct, abs_sum=abs_sum)


# ---------------------------------------------------------------------------------------------------------------
# the shared cases of test 1 (one step against the reference)
# ---------------------------------------------------------------------------------------------------------------
# (D, cap, L): bonds that are no multiple of 16, a partial second column tile, an odd number of tiles, a label core larger than LDS,
# D = 3, and D = 8 with L > 16; with the seed chosen on the CPU so that the conditions of tests/test_gradient_step_host.py hold
ROWS = [(2, 5, 3), (2, 20, 2), (2, 33, 2), (2, 50, 10), (3, 7, 3), (8, 16, 17)]
ROW_SEED = {(2, 5, 3): 0, (2, 20, 2): 1, (2, 33, 2): 0, (2, 50, 10): 0, (3, 7, 3): 0, (8, 16, 17): 0}
NINE_PAIRS_ROW = (2, 20, 2)
WD = 1e-2
T_CASES = 2.0
CLIP_MARGIN = 1e-3          # |s_d / s_A - 1| of every core of every case: float32 cannot decide the clip differently
SAFE = 0.05                 # distance of the cross-entropy denominators from zero


def labels_of(N):
    return {2: [0, 1], 3: [0, 1, 2], 17: [0, 5, 11, 16]}[N]


def _features(rng, b, N, D):
    from tensornetworkforml_amd import data_generator as gen
    pix = rng.random((b, N)) * (rng.random((b, N)) > 0.3)
    return np.ascontiguousarray(gen.psi(pix.astype(np.float32).astype(np.float64), D), dtype=np.float32)


def _safe_labels(f, T, rng):
    """per sample a label for which every cross-entropy denominator of every activation stays SAFE away from zero, or -1"""
    L, b = f.shape
    y = np.full(b, -1)
    for s in range(b):
        for cand in rng.permutation(L):
            ok = True
            for act in ACTS:
                fa = apply_act_func(f[:, s:s + 1], act, f32(T))[:, 0]
                z = fa - (np.arange(L) != cand)
                if act != 'softmax' and abs(fa[cand]) < SAFE:
                    ok = False
                if np.abs(z + 1e-4).min() < SAFE:
                    ok = False
            if ok:
                y[s] = cand
                break
    return y


def row_cases(row, seed=None):
    """The cases of a row: N in {2, 3, 17}, the label at both ends and inside, uniform and ragged bonds, b in {1, 70}.  Every case is
    a dict(N, l, ragged, b, cores (float32), X (float32), y).  The cores are scaled_cores, every core divided by the N-th root of the
    median |f| of the case's batch (a calibrated network: f is of order 1 whatever N and D).  Samples are redrawn until a label exists that keeps every cross-entropy denominator SAFE
    away from zero for all three activations."""
    D, cap, L = row
    rng = np.random.default_rng([D, cap, L, ROW_SEED[row] if seed is None else seed])
    for N in (2, 3, 17):
        for l in labels_of(N):
            for ragged in (False, True):
                bond = ragged_bonds(N, cap, rng) if ragged else [cap] * (N - 1)
                base = scaled_cores(N, D, L, bond, l, rng)
                for b in (1, 70):
                    X = _features(rng, b, N, D)
                    f0 = forward64(base, l, X.astype(np.float64))
                    cores = [(c * np.median(np.abs(f0)) ** (-1.0 / N)).astype(np.float32) for c in base]
                    c64 = [c.astype(np.float64) for c in cores]
                    y = _safe_labels(forward64(c64, l, X.astype(np.float64)), T_CASES, rng)
                    for _ in range(200):
                        bad = np.flatnonzero(y < 0)
                        if bad.size == 0:
                            break
                        X[bad] = _features(rng, bad.size, N, D)
                        y[bad] = _safe_labels(forward64(c64, l, X[bad].astype(np.float64)), T_CASES, rng)
                    assert (y >= 0).all(), 'no safe sample found'
                    yield dict(N=N, l=l, ragged=ragged, b=b, cores=cores, X=X, y=y.astype(np.int32))


def pairs_of(row):
    return [(a, lo) for a in ACTS for lo in LOSSES] if row == NINE_PAIRS_ROW else [('linear', 'MSE')]


def case_lr(case, act_fn, loss_fn):
    """(lr, reference info) of a case: 0.5 with the clip on where that moves the cores by at least a tenth of max|A|, else the
    smallest float32 that does."""
    c64 = [c.astype(np.float64) for c in case['cores']]
    amax = max(np.abs(c).max() for c in c64)
    ref = GradientStepReference(c64, case['l'])
    ref.step(case['X'], case['y'], 1.0, WD, act_fn, loss_fn, T_CASES)
    dmax = max(np.abs(a - c).max() for a, c in zip(ref.cores, c64))            # max |d| after the clip (lr = 1)
    lr = 0.5
    if 0.5 * dmax < 0.1 * amax:
        lr = float(np.nextafter(np.float32(0.1001 * amax / dmax), np.float32(np.inf)))
    return lr


# ---------------------------------------------------------------------------------------------------------------
# the short training run of test 5
# ---------------------------------------------------------------------------------------------------------------
RUN = dict(N=16, D=2, L=2, M=4, n=200, batch=50, steps=10, lr=0.05, wd=0.0, act_fn='softmax', loss_fn='full_cross_ent', T=1.0)


def training_run_setup():
    """(X (200, 16, 2) float32, y, start cores float32, index list of the 10 steps): data_generator.create_dataset diagonals at
    N = 16, bond 4, the batches of 50 taken in order, round and round; SGD with the clip."""
    from tensornetworkforml_amd import data_generator as gen
    state = np.random.get_state()
    np.random.seed(1234)
    data, label = gen.create_dataset(RUN['n'], 4, 0.3)
    np.random.set_state(state)
    X = np.ascontiguousarray(gen.psi(np.clip(data.reshape(RUN['n'], -1), 0.0, 1.0), RUN['D']), dtype=np.float32)
    rng = np.random.default_rng(99)
    base = scaled_cores(RUN['N'], RUN['D'], RUN['L'], [RUN['M']] * (RUN['N'] - 1), 0, rng)
    f0 = forward64(base, 0, X.astype(np.float64))
    cores = [(c * np.median(np.abs(f0)) ** (-1.0 / RUN['N'])).astype(np.float32) for c in base]
    idx = np.concatenate([np.arange(RUN['n'])] * 3)[:RUN['batch'] * RUN['steps']]
    return X, np.asarray(label, dtype=np.int32), cores, idx


def training_run_reference():
    """(correct per step, accuracy over all samples before, after) of the float64 trajectory"""
    X, y, cores, idx = training_run_setup()
    ref = GradientStepReference(cores, 0)
    acc0 = ref.signal(X, y, RUN['act_fn'], RUN['loss_fn'], RUN['T'])[3] / RUN['n']
    correct = []
    for k in range(RUN['steps']):
        sel = idx[k * RUN['batch']:(k + 1) * RUN['batch']]
        correct.append(ref.step(X[sel], y[sel], RUN['lr'], RUN['wd'], RUN['act_fn'], RUN['loss_fn'], RUN['T'])['correct'])
    acc1 = ref.signal(X, y, RUN['act_fn'], RUN['loss_fn'], RUN['T'])[3] / RUN['n']
    return correct, acc0, acc1, ref
