"""The cases of tests/test_batch_handover_gpu.py, checked with the float64 oracle alone: the four staged batches of every
configuration must be told apart by what the GPU tests compare.  A hand-over that selected the wrong slot, or kept the labels of the
batch before, then cannot pass them.

  f          any two slots differ by >= 0.1 of max|f| on their first min(b_i, b_j) samples (inputs alone)
  labels     differ on those samples
  cores      after one oracle sweep from the same cores, the cores reached from batch i and from batch j differ by more than 1e-3
             of the largest element (inputs and labels)
The last is also shown for the same inputs under the labels of another slot: a hand-over that kept the old labels moves the cores
as visibly.
"""
import itertools

import numpy as np
import pytest

import batch_handover_cases as bc
from oracle import mps_oracle as mo


def rel(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    assert a.shape == ref.shape, (a.shape, ref.shape)
    return float(np.abs(a - ref).max() / np.abs(ref).max())


def flat(cores):
    return np.concatenate([np.asarray(c).ravel() for c in cores])


@pytest.mark.parametrize('name', list(bc.CONFIGS))
def test_the_four_batches_can_be_told_apart(name):
    c = bc.case(name)
    assert [X.shape for X, _ in c['batches']] == [(b, c['N'], c['D']) for b in bc.SIZES]
    assert all(y.min() >= 0 and y.max() < c['L'] and len(set(y.tolist())) > 1 for _, y in c['batches'])
    first = [bc.oracle_first_pass(name, k) for k in range(len(bc.SIZES))]
    worst = dict(f=np.inf, cores=np.inf)
    for i, j in itertools.combinations(range(len(bc.SIZES)), 2):
        n = min(bc.SIZES[i], bc.SIZES[j])
        df = rel(first[i][0][:, :n], first[j][0][:, :n])
        dc = rel(flat(first[i][2]), flat(first[j][2]))
        worst['f'], worst['cores'] = min(worst['f'], df), min(worst['cores'], dc)
        assert df >= 0.1, (i, j, df)
        assert not np.array_equal(c['batches'][i][1][:n], c['batches'][j][1][:n]), (i, j)
        assert dc > 1e-3, (i, j, dc)
    print(name, 'smallest difference between two slots: f %.3g, cores after a sweep %.3g' % (worst['f'], worst['cores']))
    # the same free of the gauge (the SVD leaves signs open): f of one probe batch through the cores each batch led to
    probe = c['batches'][2][0].astype(np.float64)
    fp = [mo.forward(bc.oracle_state(c, first[k][2], c['N'] - 1), probe) for k in range(len(bc.SIZES))]
    for i, j in itertools.combinations(range(len(bc.SIZES)), 2):
        assert rel(fp[i], fp[j]) > 1e-3, (i, j)


@pytest.mark.parametrize('name', list(bc.CONFIGS))
def test_stale_labels_move_the_cores(name):
    """batch k under the labels slot k - 1 left behind (cut or repeated to its length) against batch k under its own"""
    c = bc.case(name)
    for k in range(len(bc.SIZES)):
        X, y = c['batches'][k]
        stale = np.resize(c['batches'][k - 1][1], y.shape)
        assert not np.array_equal(stale, y)
        st = bc.oracle_state(c)
        X64 = X.astype(np.float64)
        mo.sweep(st, X64, stale, mo.forward(st, X64), bc.HP_KW['lr'], bc.HP_KW['weight_dec'], L2_flag=True, left_dir=False,
                 act_fn='softmax', loss_fn='full_cross_ent', T=0.1, trunc='fixed')
        dc = rel(flat(st.cores), flat(bc.oracle_first_pass(name, k)[2]))
        assert dc > 1e-3, (k, dc)


def test_sizes_cover_the_tiles_they_are_meant_to():
    pad = [(b + 63) // 64 * 64 for b in bc.SIZES]
    assert pad == [128, 320, 64, 192]
    assert bc.SIZES[0] % 64 and bc.SIZES[1] > 4 * 64 and bc.SIZES[2] < 32
    assert max(c['N'] for c in bc.CONFIGS.values()) <= 16
