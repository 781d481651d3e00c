"""Device-resident dataset without a GPU: the index loader against `DataLoader`, the split of `prepare_device_dataset` against
`prepare_dataset`'s, the new entry points in header / library / `_hip.SYMBOLS`, and the host side of the dataset calls under
AddressSanitizer + UBSan (csrc/Makefile target `san-dataset`)."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tensornetworkforml_amd import _hip                    # noqa: E402
from tensornetworkforml_amd import data_generator as gen   # noqa: E402

DATASET_SYMBOLS = ['tnml_dataset_attach', 'tnml_dataset_detach', 'tnml_dataset_size', 'tnml_select_indices', 'tnml_predict_indices',
                   'tnml_eval_indices', 'tnml_resident_metrics', 'tnml_dataset_read']


@pytest.mark.parametrize('drop_last', [True, False])
@pytest.mark.parametrize('n_subset,batch', [(103, 10), (64, 16), (7, 10)])
def test_index_loader_reproduces_dataloader_order(drop_last, n_subset, batch):
    """Same subset, batch size, drop_last and state of NumPy's global generator: the same sample order over three passes (one
    np.random.permutation per pass), the last batch ragged where the subset is not a multiple of the batch."""
    rng = np.random.default_rng(5)
    data = rng.random((150, 6, 2))
    label = rng.integers(0, 2, 150)
    subset = np.arange(20, 20 + n_subset)
    ref = gen.DataLoader(gen.NumpyDataset(data, label), batch, sampler=gen.SubsetRandomSampler(subset), drop_last=drop_last)
    new = gen.IndexLoader(subset, batch, shuffle=True, drop_last=drop_last)
    assert len(new) == len(ref)
    np.random.seed(11)
    want = [[(b.X.copy(), b.y.copy()) for b in ref] for _ in range(3)]
    after_ref = np.random.random()
    np.random.seed(11)
    got = [[np.array(idx) for idx in new] for _ in range(3)]
    after_new = np.random.random()
    assert after_ref == after_new                       # the generator was consumed identically
    sizes = set()
    for p in range(3):
        assert len(got[p]) == len(want[p]) == len(ref)
        for idx, (X, y) in zip(got[p], want[p]):
            assert idx.dtype.kind == 'i' and idx.ndim == 1
            assert np.array_equal(data[idx], X) and np.array_equal(label[idx], y)
            sizes.add(len(idx))
    if not drop_last and n_subset % batch:
        assert n_subset % batch in sizes                # the ragged batch was there
    if len(ref) > 1:
        assert not np.array_equal(np.concatenate(got[0]), np.concatenate(got[1]))      # a fresh order per pass


def test_index_loader_sequential():
    new = gen.IndexLoader(np.arange(5, 30), 8, shuffle=False, drop_last=False)
    state = np.random.get_state()[1].copy()
    got = [np.array(i) for i in new]
    assert np.array_equal(np.random.get_state()[1], state)      # no draw without shuffling
    assert np.array_equal(np.concatenate(got), np.arange(5, 30)) and [len(g) for g in got] == [8, 8, 8, 1]


class _FakeNet:
    """Records what prepare_device_dataset uploads (no device here)."""

    def __init__(self, D):
        self.D = D

    def attach_dataset(self, data, label, pixels=False):
        self.data, self.label, self.pixels = np.array(data), np.array(label), pixels
        return ('dataset', len(data))


@pytest.mark.parametrize('pixels', [True, False])
@pytest.mark.parametrize('D', [2, 3])
def test_prepare_device_dataset_split_equals_prepare_dataset(D, pixels):
    np.random.seed(2)
    data, label = gen.create_dataset(230, 4, 0.5)
    sizes = dict(train_batch_size=25, val_batch_size=10, test_batch_size=16)
    ref_loaders = gen.prepare_dataset(data, label, 0.8, 0.25, D=D, **sizes)
    net = _FakeNet(D)
    ds, *new_loaders = gen.prepare_device_dataset(net, data, label, 0.8, 0.25, D=D, pixels=pixels, **sizes)
    assert ds == ('dataset', 230) and net.pixels == pixels and np.array_equal(net.label, label)
    emb = gen.psi(data.reshape(230, -1), D)
    if pixels:
        assert net.data.shape == (230, 16) and np.array_equal(net.data, data.reshape(230, -1))
    else:
        assert np.array_equal(net.data, emb)
    tr, va, te = gen.split_indices(230, 0.8, 0.25)
    assert (len(tr), len(va), len(te)) == (138, 46, 46) and np.array_equal(np.concatenate([tr, va, te]), np.arange(230))
    for k, (ref, new) in enumerate(zip(ref_loaders, new_loaders)):
        assert len(ref) == len(new)
        for _ in range(2):
            np.random.seed(7 + k)
            want = [(b.X.copy(), b.y.copy()) for b in ref]
            np.random.seed(7 + k)
            got = [np.array(i) for i in new]
            assert len(got) == len(want) > 0
            for idx, (X, y) in zip(got, want):
                assert np.array_equal(emb[idx], X) and np.array_equal(label[idx], y)
    assert [len(i) for i in new_loaders[2]] == [16, 16, 14]                     # the test loader keeps its ragged batch
    with pytest.raises(ValueError):
        gen.prepare_device_dataset(_FakeNet(D + 1), data, label, 0.8, 0.25, D=D, **sizes)


def test_dataset_symbols_in_header_library_and_binding():
    hdr = open(os.path.join(ROOT, 'include', 'tnml.h')).read()
    lib = _hip.lib()
    for s in DATASET_SYMBOLS:
        assert s in _hip.SYMBOLS, s
        assert re.search(r'\bint\s+%s\s*\(' % s, hdr), s
        assert hasattr(lib, s), s
    assert _hip.DATASET_FORM == {'features': 0, 'pixels': 1}
    assert 'TNML_DATASET_FEATURES = 0' in hdr and 'TNML_DATASET_PIXELS = 1' in hdr


def test_network_without_a_dataset_says_so():
    """A dataset belongs to the device context: a network that never had one attached (or was just unpickled) raises a clear
    exception from train_resident / evaluate before anything touches the device."""
    import pickle
    from tensornetworkforml_amd import Network_class as tn
    np.random.seed(0)
    net = tn.Network(N=6, M=3, L=2)
    loader = gen.IndexLoader(np.arange(8), 4)
    for call in (lambda n: n.train_resident(loader, loader, 0.1, n_epochs=1), lambda n: n.evaluate(np.arange(4)),
                 lambda n: n.evaluate(loader)):
        with pytest.raises(RuntimeError, match='attach_dataset'):
            call(net)
    net2 = pickle.loads(pickle.dumps(net))
    assert net2._dataset is None
    with pytest.raises(RuntimeError, match='not pickled'):
        net2.evaluate(np.arange(4))


def test_dataset_host_side_under_sanitizers():
    """csrc/Makefile target `san-dataset`: api_dataset.hip's entry points and the launch wrappers of kernels_dataset.hip,
    built --cuda-host-only with -fsanitize=address,undefined, against the stand-in runtime of csrc/san/hip_stub.cpp
    (csrc/san/plan_dataset_main.cpp): both forms, ragged / one-sample / larger-than-capacity index batches, predict, evaluation of
    more samples than any buffer holds, detach and re-attach with another n, out-of-range and negative indices, at D = 2, 3 and 8;
    every launch of the new kernels has its pointers and extents checked through the uploaded index list."""
    import shutil
    import subprocess
    if shutil.which('g++') is None or not os.path.exists('/opt/rocm/bin/hipcc'):
        pytest.skip('no g++ / hipcc')
    csrc = os.path.join(ROOT, 'tensornetworkforml_amd', 'csrc')
    out = subprocess.run(['make', '-C', csrc, '-j4', 'san-dataset'], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert 'dataset host planning under ASan + UBSan: ok' in out.stdout
    assert 'communicator attached: dataset calls refused' in out.stdout
    for D in (2, 3, 8):
        assert 'planned dataset calls D %d ' % D in out.stdout
    m = re.search(r'dataset launches: (\d+) argument extents checked, (\d+) gathers through (\d+) indices', out.stdout)
    assert m and int(m.group(1)) > 2000 and int(m.group(2)) > 300 and int(m.group(3)) > 10000, out.stdout[-2000:]
    assert re.search(r'san-stub: \d+ launches checked \(\d+ kernels\), \d+ pointer extents checked, 0 live allocations', out.stdout)
