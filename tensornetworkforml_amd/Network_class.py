"""`Network` -- the MPS classifier and its DMRG-style two-site sweep optimiser with the API of the
reference's `Network_class.Network` (/root/reference/TensorNetwork/Network_class.py), executed by
hand-written HIP kernels on an MI355X through the C ABI of include/tnml.h (ctypes, `_hip.py`).

Design: the cores, the batch, both environment stacks and f live in HBM for the whole
life of the object; `forward`, `sweep`, `sweep_step`, `accuracy`, `apply_act_func` and
`compute_loss_derivate` are device calls; `As`, `TX`, `r_cum_contraction` and `l_cum_contraction`
are materialised as `Tensor` objects only when somebody reads them.  There is no NumPy fallback:
without the library or without a gfx950 device every compute method raises.

Differences from the reference, all opt-in or unavoidable:
  * arithmetic is float32 on the device (float64 inside the merged-tensor update and the SVD);
  * `trunc='adaptive'` (not reference behaviour) keeps min(M, index + 1) singular values, `index` being
    the cumulative-share index the reference computes and never uses (Network_class.py:889-891,
    `threshold=0.999`);
  * `trunc='reference'` (default) reproduces the reference's truncation rule, including its
    ValueError for L > 2 (Network_class.py:914); `trunc='fixed'` keeps m = min(M, len(S)) on both
    factors -- the only policy under which the bond dimension M survives the first sweep;
  * the softmax subtracts the per-sample maximum (same function, no overflow at f/T > 709);
  * `update_B`, `tensor_svd` and `compute_L2_reg` are fused into one kernel per sweep step; the
    methods of that name run the same device code on the operands they are given.
"""
import math

import numpy as np

from Tensor_class import Tensor
from custom_linalg_tools import contract, partial_trace  # noqa: F401  (re-exported like the reference)
from data_generator import psi as _psi
from data_generator import psi_gram as _psi_gram

try:
    from tensornetworkforml_amd import _hip
except ImportError:                                       # running from inside the package directory
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from tensornetworkforml_amd import _hip

new = np.newaxis

_ACTS = ['linear', 'sigmoid', 'softmax']
_LOSSES = ['MSE', 'cross_entropy', 'full_cross_ent']


def random_canonical_cores(N, M, D, L, scale=1.0, rng=None):
    """U[0,1)/scale cores in the canonical device layout (ml, D, mr[, L]), label on site 0.

    The draws follow Network.__init__ (Network_class.py:145-148, 186-189): (L,M,D) for site 0,
    (M,M,D) for the interior, (M,D) for the last site, in site order, from the legacy global
    generator when `rng` is None -- so `np.random.seed(s); Network(...)` starts from the same
    numbers as the reference."""
    draw = np.random.random if rng is None else rng.random
    cores = [np.transpose(draw((L, M, D)) / scale, (2, 1, 0))[None]]          # (1, D, M, L)
    for _ in range(1, N - 1):
        cores.append(np.transpose(draw((M, M, D)) / scale, (0, 2, 1)))        # (M, D, M)
    cores.append((draw((M, D)) / scale)[:, :, None])                          # (M, D, 1)
    return [np.ascontiguousarray(c) for c in cores]


def _core_to_tensor(core, site, N, has_label):
    """canonical (ml, D, mr[, L]) -> Tensor with the reference's axis names for that site."""
    names, sl = [], []
    if site > 0:
        names.append('left'); sl.append(slice(None))
    else:
        sl.append(0)
    names.append('d' + str(site)); sl.append(slice(None))
    if site < N - 1:
        names.append('right'); sl.append(slice(None))
    else:
        sl.append(0)
    if has_label:
        names.append('l'); sl.append(slice(None))
    return Tensor(elem=np.array(core[tuple(sl)], dtype=np.float64), axes_names=names)


def _tensor_to_core(T, site, N):
    """Tensor of one site (any axis order, reference names) -> canonical (ml, D, mr[, L])."""
    names = [str(a) for a in T.axes_names]
    order = [names.index(n) for n in ('left', 'd' + str(site), 'right', 'l') if n in names]
    c = np.transpose(np.asarray(T.elem), order)
    if 'left' not in names:
        c = c[None]
    if 'right' not in names:
        c = np.expand_dims(c, 2)
    return np.ascontiguousarray(c), ('l' in names)


class _EnvList:
    """Lazy stand-in for `r_cum_contraction` / `l_cum_contraction`: a list of Tensors that is
    downloaded from the device only when it is indexed.  `entries` is a list of ('env', side, site)
    or ('f',) descriptors in the reference's list order."""

    def __init__(self, net, entries):
        self._net, self._entries, self._cache = net, list(entries), {}
        self._epoch = net._env_epoch

    def __len__(self):
        return len(self._entries)

    def _get(self, i):
        if self._epoch != self._net._env_epoch:
            raise RuntimeError("this environment list belongs to an earlier forward/sweep; read "
                               "net.r_cum_contraction / net.l_cum_contraction again")
        if i not in self._cache:
            e = self._entries[i]
            if e[0] == 'f':
                self._cache[i] = Tensor(elem=self._net._ctx.get_f().astype(np.float64), axes_names=['l', 'b'])
            else:
                _, side, site = e
                arr = self._net._ctx.get_env(side, site).astype(np.float64).T      # (m, b)
                self._cache[i] = Tensor(elem=arr, axes_names=['left' if side == _hip.SIDE_RIGHT else 'right', 'b'])
        return self._cache[i]

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self._get(j) for j in range(*i.indices(len(self)))]
        if i < 0:
            i += len(self)
        if not 0 <= i < len(self):
            raise IndexError(i)
        return self._get(i)

    def __iter__(self):
        return (self._get(i) for i in range(len(self)))


class Network():
    """Matrix Product State classifier trained by alternating two-site sweeps.

    Attributes (as in the reference, Network_class.py:14-47): N, D, L, M, T, act_fn, loss_fn,
    As, l_pos, TX, r_cum_contraction, l_cum_contraction.

    `any_position` (default False, not pickled; not in the reference): when set, `forward`, `predict`, `evaluate` and the dataset
    calls also run with the label at an intermediate site -- `l_cum_contraction` then lists Lenv[0..l-1] and `r_cum_contraction`
    Renv[l+1..N-1], both in site order, and f is only the return value -- and `sweep_step` may follow such a forward in either
    direction (include/tnml.h, tnml_set_any_position).  `train_resident(steps_per_batch=k)` leaves in `segment_log` the list of
    (l_pos, left_dir, n_steps) of the segments of its last call; the direction of the last segment is pickled with the network
    (`seg_left`), so that a model saved mid-sweep goes on in the direction it was moving.

    `scaled_chains` (default False, not pickled; not in the reference): when set, `predict`, `evaluate`, the input and core
    gradients and `train_gradient` carry a power-of-two exponent per sample along their chains, so that a partial product that
    leaves float32 -- after Adam, weight decay or a change of gauge moved the size of single cores -- no longer turns a
    representable result into inf, nan or 0 (include/tnml.h, tnml_set_chain_scaling).  `forward`, the
    resident batch and the sweep are untouched.  `predict_scaled(X)` returns f as (mantissa, exponent) whatever the switch says.

    D (2 <= D <= 8) is the local feature dimension (data_generator.psi(x, D) embeds pixels for it).  D != 2 runs the
    generic per-step device path (include/tnml.h).  Deviation from the reference: with normalize=True and no
    calibration_X the 16 random calibration samples are embedded with psi(u, D); the reference always embeds them
    with the two-component map and therefore fails at D != 2.  At D = 2 the draws and values are the reference's.
    """

    def __init__(self, N, M, D=2, L=10, T=0.1, normalize=False, calibration_X=None, act_fn='linear',
                 loss_fn='cross_entropy', check=False, trunc='reference', device=0, svd_stop=None, threshold=0.999):
        self.N, self.D, self.L, self.M, self.T = N, D, L, M, T
        assert act_fn in _ACTS, "Please select an activation function between 'linear', 'sigmoid', 'softmax'"
        assert loss_fn in _LOSSES, "Please select a loss function between 'MSE', 'cross_entropy', 'full_cross_ent'"
        assert trunc in _hip.TRUNC, "trunc must be 'reference', 'fixed' or 'adaptive'"
        self.act_fn, self.loss_fn, self.trunc = act_fn, loss_fn, trunc
        self._device = device
        self._threshold = threshold        # cumulative-share threshold of trunc='adaptive'
        self._svd_stop = svd_stop          # None: the library default (include/tnml.h, tnml_set_svd_stop)
        self._init_runtime()
        self._l_pos = 0

        if normalize:
            print('Normalizing weights...')
            # output ~ [M E(A) E(x) D]^N with E(A) = 0.5, E(x) = 0.64 (Network_class.py:139-142)
            scale = float(self.M) * 0.5 * 0.64 * self.D
            print('Scaling factor: %.2f' % scale)
            self._host_cores = random_canonical_cores(N, M, D, L, scale)
            self._host_newer = True
            if calibration_X is None:
                B = 16
                u = np.random.random((B, self.N))
                X = _psi(u, self.D)          # D = 2: the reference's [sin, cos]; D != 2: see the class docstring
            else:
                X = calibration_X
                B = X.shape[0]
            print('\nCalibrating weights on dataset...')
            # order of magnitude of the output (Network_class.py:168-170).  max|f| of the raw chain is
            # ~1e-66 at N = 784, below float32: the device evaluates log max|f| with per-site
            # renormalisation instead of max|forward(X)|.
            ctx = self._sync_to_device(B)
            self._X_host, self._b = X, B
            ctx.set_input(X, None)
            self._y_dev = None
            log_fmax = ctx.forward_logabsmax()
            F2 = float(np.exp(log_fmax / self.N))
            if check:
                print('f_max for random input of %d samples : ' % (B), float(np.exp(log_fmax)))
            print("Rescaling factor for calibration: ", F2)
            ctx.scale_cores(1.0 / F2)
            self._device_newer = True
            f = self.forward(X)
            if check:
                print('f_max for random input of %d samples (after): ' % (B), float(np.abs(f.elem).max()))
        else:
            self._host_cores = random_canonical_cores(N, M, D, L)
            self._host_newer = True

    # ------------------------------------------------------------------------------------------
    # runtime state (not pickled)
    # ------------------------------------------------------------------------------------------
    def _init_runtime(self):
        self._ctx = None
        self._host_cores = None       # canonical cores as last seen on the host
        self._host_newer = False      # host copy must be uploaded before the next device call
        self._device_newer = False    # device copy changed since the host copy was taken
        self._As = None               # Tensor list handed to the user (may have been mutated)
        self._As_snapshot = None      # what that list looked like when it was built
        self._X_host = None
        self._b = 0
        self._y_dev = None
        self._env_epoch = 0
        self._r_entries = None
        self._l_entries = None
        self._r_user = None
        self._l_user = None
        self._dataset = None          # DeviceDataset attached to self._ctx (attach_dataset); lives and dies with the context
        self._X_idx = None            # dataset indices of the resident batch when it was formed on the device
        self._any_position = False
        self._scaled_chains = False   # what the user asked for; _scaled_applied: what the context was last told
        self._scaled_applied = False
        self._seg_left = False        # direction of the last segment of train_resident(steps_per_batch=k) (pickled)
        self.segment_log = []         # (l_pos, left_dir, n_steps) of the segments of the last train_resident(steps_per_batch=k)

    def _context(self, b):
        if self._ctx is None:
            self._ctx = _hip.Context(self.N, self.D, self.L, self.M, max(int(b), 1), self._device)
            if getattr(self, '_svd_stop', None) is not None:
                self._ctx.set_svd_stop(self._svd_stop)
            if getattr(self, '_threshold', None) is not None:
                self._ctx.set_trunc_threshold(self._threshold)
            if self._any_position:
                self._ctx.set_any_position(True)
        return self._ctx

    @property
    def any_position(self):
        return self._any_position

    @any_position.setter
    def any_position(self, on):
        self._any_position = bool(on)
        if self._ctx is not None:
            self._ctx.set_any_position(self._any_position)

    @property
    def scaled_chains(self):
        return self._scaled_chains

    @scaled_chains.setter
    def scaled_chains(self, on):
        self._scaled_chains = bool(on)        # (reaches the context with the next device call: _sync_to_device)

    def _check_forward_position(self, lp):
        if lp != 0 and lp != self.N - 1 and not self._any_position:
            raise Exception('### Error ###\n l =', lp, ' -> forward should not be called if l has an intermediate position')

    def _entries_after_forward(self, lp):
        """The environment lists a forward at label position lp leaves (Network_class.py:227-255); with the label inside the
        chain (any_position) both stacks exist and f belongs to neither."""
        S_R, S_L = _hip.SIDE_RIGHT, _hip.SIDE_LEFT
        if lp == 0:
            self._r_entries = [('f',)] + [('env', S_R, i) for i in range(1, self.N)]
            self._l_entries = None
        elif lp == self.N - 1:
            self._l_entries = [('env', S_L, i) for i in range(self.N - 1)] + [('f',)]
            self._r_entries = None
        else:
            self._l_entries = [('env', S_L, i) for i in range(lp)]
            self._r_entries = [('env', S_R, i) for i in range(lp + 1, self.N)]

    def _entries_after_steps(self, left_dir, lp):
        """The list the sweep grows gains one entry per step, as the reference leaves it; with any_position the other list
        is cut to what is still valid on the device (the environments beyond the label site)."""
        S_R, S_L = _hip.SIDE_RIGHT, _hip.SIDE_LEFT
        if left_dir:
            # steps at l = N-2 .. 1 append Renv[l+1]; after reaching l_pos the deepest is Renv[lp+2]
            self._r_entries = [('env', S_R, i) for i in range(self.N - 1, lp + 1, -1)]
            if self._any_position:
                self._l_entries, self._l_user = [('env', S_L, i) for i in range(lp)], None
        else:
            self._l_entries = [('env', S_L, i) for i in range(0, lp - 1)]
            if self._any_position:
                self._r_entries, self._r_user = [('env', S_R, i) for i in range(lp + 1, self.N)], None

    def _collect_user_edits(self):
        """If `net.As` was handed out, fold any edit of those Tensors back into the host cores."""
        if self._As is None:
            return
        cores, lab_site = [], None
        for i, Tn in enumerate(self._As):
            c, has_l = _tensor_to_core(Tn, i, self.N)
            if has_l:
                lab_site = i
            cores.append(c)
        changed = (self._As_snapshot is None or len(cores) != len(self._As_snapshot) or
                   any(a.shape != b.shape or not np.array_equal(a, b) for a, b in zip(cores, self._As_snapshot)))
        if changed:
            if lab_site is None:
                raise Exception("no core carries the label axis 'l'")
            self._host_cores = cores
            self._l_pos = lab_site
            self._host_newer = True
            self._As_snapshot = [c.copy() for c in cores]

    def _sync_to_device(self, b=None):
        self._collect_user_edits()
        ctx = self._context(b if b is not None else max(self._b, 1))
        if self._scaled_applied != self._scaled_chains:
            ctx.set_chain_scaling(self._scaled_chains)
            self._scaled_applied = self._scaled_chains
        if self._host_newer:
            ctx.set_cores(self._host_cores, self._l_pos)
            self._host_newer = False
            self._device_newer = False
            self._invalidate_envs()
        return ctx

    def _sync_to_host(self):
        self._collect_user_edits()
        if self._device_newer and not self._host_newer:
            cores, _, lp = self._ctx.get_cores()
            self._host_cores = [c.astype(np.float64) for c in cores]
            self._l_pos = lp
            self._device_newer = False
            self._As = None

    def _invalidate_envs(self):
        self._env_epoch += 1
        self._r_entries = self._l_entries = None
        self._r_user = self._l_user = None

    # ------------------------------------------------------------------------------------------
    # reference attributes, materialised on demand
    # ------------------------------------------------------------------------------------------
    @property
    def l_pos(self):
        if self._ctx is not None and not self._host_newer:
            return self._ctx.l_pos if self._device_newer else self._l_pos
        return self._l_pos

    @l_pos.setter
    def l_pos(self, v):
        self._sync_to_host()
        self._l_pos = int(v)
        self._host_newer = True

    @property
    def As(self):
        self._sync_to_host()
        if self._As is None:
            self._As = [_core_to_tensor(c, i, self.N, i == self._l_pos) for i, c in enumerate(self._host_cores)]
            self._As_snapshot = [np.array(c, dtype=np.float64) for c in self._host_cores]
        return self._As

    @As.setter
    def As(self, tensors):
        self._sync_to_host()
        self._As = list(tensors)
        self._As_snapshot = None

    @property
    def TX(self):
        if self._X_host is None and getattr(self, '_X_idx', None) is not None and self._dataset is not None:
            self._X_host = self._ctx.dataset_read(self._X_idx).astype(np.float64)      # a batch formed on the device, read on demand
        if self._X_host is None:
            return None
        return [Tensor(elem=self._X_host[:, i, :], axes_names=['b', 'd' + str(i)]) for i in range(self.N)]

    def _env_list(self, which):
        user = self._r_user if which == 'r' else self._l_user
        if user is not None:
            return user
        entries = self._r_entries if which == 'r' else self._l_entries
        return None if entries is None else _EnvList(self, entries)

    @property
    def r_cum_contraction(self):
        return self._env_list('r')

    @r_cum_contraction.setter
    def r_cum_contraction(self, v):
        self._r_user = v

    @property
    def l_cum_contraction(self):
        return self._env_list('l')

    @l_cum_contraction.setter
    def l_cum_contraction(self, v):
        self._l_user = v

    # ------------------------------------------------------------------------------------------
    # forward
    # ------------------------------------------------------------------------------------------
    def forward(self, X):
        """Predictions (pre-activation) for X (b, N, D); builds the environment stack for the next
        sweep: right environments at l_pos == 0, left ones at l_pos == N-1
        (Network_class.py:195-258).  Returns a Tensor ('l', 'b')."""
        assert self.N == X.shape[1], "The 1 dimension of the input data must be the flattened number of pixels"
        lp = self.l_pos
        self._check_forward_position(lp)
        ctx = self._sync_to_device(X.shape[0])
        self._X_host = X
        self._b = X.shape[0]
        ctx.set_input(X, None)
        self._y_dev = None
        f = ctx.forward()
        self._invalidate_envs()
        self._entries_after_forward(lp)
        return Tensor(elem=f.astype(np.float64), axes_names=['l', 'b'])

    def predict(self, X):
        """forward(X)'s return value without making X the resident batch: no environment list is
        rebuilt, `TX` and the training batch stay as they are (the validation loop of `train`,
        Network_class.py:339-346, only needs f).  Not in the reference."""
        assert self.N == X.shape[1], "The 1 dimension of the input data must be the flattened number of pixels"
        self._check_forward_position(self.l_pos)
        ctx = self._sync_to_device(max(self._b, 1))
        return Tensor(elem=ctx.predict(X).astype(np.float64), axes_names=['l', 'b'])

    def predict_scaled(self, X):
        """predict(X) as (mant (L, b) float32, expo (b,) int32): f[l, s] = mant[l, s] * 2 ** expo[s] with
        0.5 <= max_l |mant[l, s]| < 1 per sample, so that the output of a network whose f lies outside float32 (an un-calibrated
        one is about 1e-66 at N = 784) can be read and its argmax taken: `mant.argmax(0)`.  Works with `scaled_chains` on or off.
        Not in the reference."""
        assert self.N == X.shape[1], "The 1 dimension of the input data must be the flattened number of pixels"
        self._check_forward_position(self.l_pos)
        ctx = self._sync_to_device(max(self._b, 1))
        return ctx.predict_scaled(X)

    # ------------------------------------------------------------------------------------------
    # input gradients (not in the reference)
    # ------------------------------------------------------------------------------------------
    def _cotangent(self, cotangent, b):
        """None (the predicted class), an integer array (b,) of classes, or a float array (L, b) used as given -> what the
        device call takes."""
        if cotangent is None:
            return None
        cot = np.asarray(cotangent)
        if cot.dtype.kind in 'iu':
            assert cot.shape == (b,), "one class per sample"
            assert cot.size == 0 or (cot.min() >= 0 and cot.max() < self.L), "class outside [0, L)"
            onehot = np.zeros((self.L, b), dtype=np.float32)
            onehot[cot, np.arange(b)] = 1.0
            return onehot
        assert cot.shape == (self.L, b), "a dense cotangent has shape (L, b)"
        return cot.astype(np.float32)

    def input_gradient(self, X, cotangent=None, return_cf=False):
        """g (b, N, D): g[s, i, d] = sum_l cotangent[l, s] d f[l, s] / d X[s, i, d], computed on the device for a batch that
        does not become resident (saliency, adversarial direction, the cotangent for a layer in front of the MPS).  Works at any
        label position.  cotangent: None = one-hot of the predicted class, an integer array (b,) = one-hot of those classes, a
        float array (L, b) = used as given.  return_cf: also cf (b,) = sum_l cotangent[l, s] f[l, s]."""
        assert self.N == X.shape[1], "The 1 dimension of the input data must be the flattened number of pixels"
        ctx = self._sync_to_device(max(self._b, 1))
        g, cf = ctx.input_grad(X, self._cotangent(cotangent, X.shape[0]))
        return (g, cf) if return_cf else g

    def input_gradient_indices(self, indices, cotangent=None, wrt='pixels'):
        """input_gradient for samples of the attached dataset.  wrt='pixels' (a dataset attached with pixels=True): (b, N),
        the chain rule through the feature map on the device; wrt='features': (b, N, D)."""
        ctx = self._require_dataset()
        idx = np.asarray(indices)
        return ctx.input_grad_indices(idx, self._cotangent(cotangent, idx.size), wrt)[0]

    # ------------------------------------------------------------------------------------------
    # core gradients (not in the reference)
    # ------------------------------------------------------------------------------------------
    def core_gradient(self, X, cotangent=None, return_cf=False):
        """G, a list of N float32 arrays in the canonical layouts (ml, D, mr) and, on l_pos, (ml, D, mr, L): the derivative of
        sum_s sum_l cotangent[l, s] f[l, s] with respect to every core, computed on the device for a batch that does not become
        resident.  Works at any label position.  cotangent as in input_gradient (a Tensor ('l', 'b'), such as
        compute_loss_derivate's, is taken by its elements); return_cf: also cf (b,) = sum_l cotangent[l, s] f[l, s].
        The gradient of a loss: f = net.predict(X); cot = net.compute_loss_derivate(net.apply_act_func(f), y);
        G = net.core_gradient(X, cot)."""
        assert self.N == X.shape[1], "The 1 dimension of the input data must be the flattened number of pixels"
        ctx = self._sync_to_device(max(self._b, 1))
        G, cf = ctx.core_grad(X, self._cotangent(getattr(cotangent, 'elem', cotangent), X.shape[0]))
        return (G, cf) if return_cf else G

    def core_gradient_indices(self, indices, cotangent=None, return_cf=False):
        """core_gradient for samples of the attached dataset."""
        ctx = self._require_dataset()
        idx = np.asarray(indices)
        G, cf = ctx.core_grad_indices(idx, self._cotangent(getattr(cotangent, 'elem', cotangent), idx.size))
        return (G, cf) if return_cf else G

    # ------------------------------------------------------------------------------------------
    # training
    # ------------------------------------------------------------------------------------------
    def train(self, train_loader, val_loader, lr, n_epochs=10, weight_dec=0.001, L2_flag=True, debug=False):
        """One sweep per training batch, direction alternating with the label position, then a
        validation pass per epoch (Network_class.py:261-350).  Returns (val_acc, var_hist) with
        var_hist of shape (n_epochs, 2 | 7, n_batches * (N-1))."""
        val_acc, var_hist = [], []
        print("\n --- TRAINING PROCEDURE ---")
        for epoch in range(n_epochs):
            epoch_train_acc = np.zeros(len(train_loader))
            var_hist.append([[] for _ in range(7 if debug else 2)])
            for i, data in enumerate(train_loader, 0):
                x, y = _unpack_batch(data)
                f = self.forward(x)
                epoch_train_acc[i] = self.accuracy(x, y, f)
                left_dir = (self.l_pos == self.N - 1)
                f = self.sweep(x, y, f, lr, weight_dec, L2_flag=L2_flag, left_dir=left_dir,
                               var_hist=var_hist[epoch], debug=debug)
                print('\r' + "Epoch %d/%d - train accuracy : %.4f - completed : %.2f "
                      % (epoch, n_epochs, epoch_train_acc[i], (i + 1) * 100 / len(train_loader)) + '%', end=' ')
            epoch_val_acc = np.zeros(len(val_loader))
            for i, data in enumerate(val_loader, 0):
                x, y = _unpack_batch(data)
                epoch_val_acc[i] = self.accuracy(x, y, self.predict(x))      # same f as forward(x), nothing rebuilt
            val_acc.append(epoch_val_acc.mean())
            print('\r' + "Epoch %d/%d - train accuracy : %.4f - val accuracy: %.4f"
                  % (epoch, n_epochs, epoch_train_acc.mean(), val_acc[-1]))
        return val_acc, np.array(var_hist)

    # ------------------------------------------------------------------------------------------
    # training and evaluation from a dataset that stays on the device
    # ------------------------------------------------------------------------------------------
    def attach_dataset(self, data, label, pixels=False):
        """Upload a dataset to the device once.  pixels=False: `data` (n, N, D) are embedded features (what `forward`
        takes); pixels=True: `data` (n, N) or (n, h, w) are pixels in [0, 1] and the feature map `data_generator.psi(., D)`
        runs on the device whenever a batch is formed (1 / D of the memory and of the upload).  Replaces an earlier
        dataset.  The dataset belongs to the device context: it is not pickled, and an unpickled network needs it attached
        again.  Returns a `DeviceDataset` description."""
        data = np.asarray(data)
        if pixels:
            data = data.reshape(len(data), -1)
        assert data.ndim == (2 if pixels else 3) and data.shape[1] == self.N, \
            "The 1 dimension of the input data must be the flattened number of pixels"
        label = np.asarray(label)
        assert label.shape == (len(data),), "one label per sample"
        ctx = self._sync_to_device()
        self._dataset = None
        ctx.dataset_attach(data, label, 'pixels' if pixels else 'features')
        self._dataset = DeviceDataset(len(data), self.N, self.D, bool(pixels))
        return self._dataset

    def detach_dataset(self):
        if self._ctx is not None:
            self._ctx.dataset_detach()
        self._dataset = None

    def _require_dataset(self):
        if self._ctx is None or self._dataset is None:
            raise RuntimeError("no dataset is attached to this network's device context (a dataset is not pickled and does "
                               "not survive a new context): call attach_dataset(data, label) first")
        return self._sync_to_device()

    def _forward_indices(self, idx):
        """forward() for the dataset samples idx, without any copy of X or f: the batch is formed on the device, the chain
        builds the environment stack, and (correct, sum |onehot - act(f)|, non-finite) of f come back."""
        lp = self.l_pos
        self._check_forward_position(lp)
        ctx = self._sync_to_device(len(idx))
        ctx.select_indices(idx)
        self._X_host, self._X_idx = None, np.array(idx, dtype=np.int64)
        self._b = len(idx)
        self._y_dev = None
        ctx.forward(want_f=False)
        self._invalidate_envs()
        self._entries_after_forward(lp)
        return ctx.resident_metrics(self.act_fn, self.T)

    def _sweep_resident(self, lr, weight_dec, L2_flag, left_dir, var_hist, n_steps=None, first=True):
        """sweep() on the batch `_forward_indices` left resident: labels and f are already on the device.  n_steps / first: a
        segment of a sweep (train_resident(steps_per_batch=k)); first is set exactly when it starts at a chain end."""
        ctx = self._ctx
        if first:
            if left_dir:
                self._r_entries, self._r_user = [], None
            else:
                self._l_entries, self._l_user = [], None
        met, _ = ctx.sweep(left_dir, self.N - 1 if n_steps is None else n_steps, first, lr, weight_dec, L2_flag, self.act_fn, self.loss_fn,
                           self.T, self.trunc, want_metrics=True, want_f=False)
        var_hist[0].extend(float(v) for v in met[:, 0])
        var_hist[1].extend(float(v) for v in met[:, 1])
        self._device_newer = True
        self._As = None
        self._env_epoch += 1
        self._entries_after_steps(left_dir, ctx.l_pos)

    def _next_segment(self, k):
        """(left_dir, n_steps, first) of the segment that starts at the current label position: right from site 0, left from
        site N-1, otherwise the direction of the previous segment; at most k steps, never past the chain end."""
        l = self.l_pos
        if l == 0:
            self._seg_left = False
        elif l == self.N - 1:
            self._seg_left = True
        left = self._seg_left
        return left, min(int(k), l if left else self.N - 1 - l), l == (self.N - 1 if left else 0)

    def train_resident(self, train_index_loader, val_index_loader, lr, n_epochs=10, weight_dec=0.001, L2_flag=True,
                       steps_per_batch=None):
        """`train` from the attached dataset: the loaders yield index arrays (data_generator.IndexLoader), and per batch
        only the index list goes to the device and the per-step metrics and three scalars come back -- X and f never
        cross the bus.  Same sweeps, same printed lines and same return value (val_acc, var_hist of shape
        (n_epochs, 2, n_batches * (N-1))) as `train` on loaders that yield the same samples in the same order.

        steps_per_batch = k >= 1 (not in the reference) changes the batch every k steps instead of every sweep: per index
        batch a forward at the current label position (its accuracy is the batch's training accuracy), then
        min(k, steps left to the chain end in the current direction) steps.  The direction is right at site 0, left at
        site N-1 and otherwise that of the previous segment; position and direction carry over from batch to batch and from
        epoch to epoch, and a segment that reaches an end is not padded by turning round.  Validation runs wherever the
        label stands.  `any_position` is set for the duration of the call.  var_hist is then a list of one
        (2, n_epoch_steps) array per epoch (the step count may differ between epochs).  k = N-1 from a chain end is the
        default schedule."""
        if steps_per_batch is not None and (int(steps_per_batch) != steps_per_batch or int(steps_per_batch) < 1):
            raise ValueError('steps_per_batch must be an integer >= 1')
        self._require_dataset()
        if steps_per_batch is None:
            return self._train_resident_loop(train_index_loader, val_index_loader, lr, n_epochs, weight_dec, L2_flag, None)
        was = self._any_position
        self.any_position = True
        try:
            return self._train_resident_loop(train_index_loader, val_index_loader, lr, n_epochs, weight_dec, L2_flag, int(steps_per_batch))
        finally:
            self.any_position = was

    def _train_resident_loop(self, train_index_loader, val_index_loader, lr, n_epochs, weight_dec, L2_flag, k):
        """The epoch loop of train_resident.  k = None: a whole sweep per batch from the chain end the label stands on (var_hist
        an array); k: the segments of `_next_segment` (var_hist a list of one array per epoch), each noted in `segment_log`."""
        val_acc, var_hist = [], []
        if k is not None:
            self.segment_log = []
        print("\n --- TRAINING PROCEDURE ---")
        for epoch in range(n_epochs):
            epoch_train_acc = np.zeros(len(train_index_loader))
            vh = [[], []]
            for i, idx in enumerate(train_index_loader, 0):
                correct, _, _ = self._forward_indices(idx)
                epoch_train_acc[i] = correct / len(idx)
                if k is None:
                    left_dir, n, first = (self.l_pos == self.N - 1), None, True
                else:
                    left_dir, n, first = self._next_segment(k)
                    self.segment_log.append((self.l_pos, left_dir, n))
                self._sweep_resident(lr, weight_dec, L2_flag, left_dir, vh, n_steps=n, first=first)
                print('\r' + "Epoch %d/%d - train accuracy : %.4f - completed : %.2f "
                      % (epoch, n_epochs, epoch_train_acc[i], (i + 1) * 100 / len(train_index_loader)) + '%', end=' ')
            var_hist.append(vh if k is None else np.array(vh))
            epoch_val_acc = np.zeros(len(val_index_loader))
            for i, idx in enumerate(val_index_loader, 0):
                correct, _, _ = self._ctx.eval_indices(idx, self.act_fn, self.T)
                epoch_val_acc[i] = correct / len(idx)
            val_acc.append(epoch_val_acc.mean())
            print('\r' + "Epoch %d/%d - train accuracy : %.4f - val accuracy: %.4f"
                  % (epoch, n_epochs, epoch_train_acc.mean(), val_acc[-1]))
        return val_acc, (np.array(var_hist) if k is None else var_hist)

    # ------------------------------------------------------------------------------------------
    # gradient training over all cores at fixed bonds (not in the reference)
    # ------------------------------------------------------------------------------------------
    def _after_device_update(self):
        """Host bookkeeping after the device changed every core in place (that of _sweep_resident; no environment survives)."""
        self._device_newer = True
        self._As = None
        self._invalidate_envs()

    # ------------------------------------------------------------------------------------------
    # orthogonal form about the label, compression, bond spectra (not in the reference)
    # ------------------------------------------------------------------------------------------
    def orthogonalize(self, rank_tol=1e-6):
        """Put the MPS on the device into orthogonal form about the label site: every core left of it becomes g times a left
        isometry, every core right of it g times a right isometry, the label core g times a tensor of norm 1, with
        g = exp(log|W| / N) on all N cores; bonds shrink to the rank of what they cut (directions below rank_tol of the largest
        singular value are dropped).  f is unchanged.  Returns log|W|.  A forward is needed before the next sweep.  The state of a
        stateful optimiser (momentum, Adam) refers to the old gauge: call configure_optimizer again before the next gradient_step
        (it resets the state, as tnml_optim_reset does; train_gradient configures on entry).  The same holds after compress."""
        ctx = self._sync_to_device(max(self._b, 1))
        _, log_norm = ctx.orthogonalize(rank_tol)
        self._after_device_update()
        return log_norm

    def compress(self, max_bond=None, threshold=None, rank_tol=1e-6):
        """Cut every bond to min(max_bond, adaptive rank at `threshold`) on its Schmidt decomposition (the rule of
        trunc='adaptive' on the bond's normalised spectrum) and leave the MPS in orthogonal form about the label.  Returns
        (bonds, discarded): the new bond dimensions and, per bond, the discarded weight sum_{j > m} sigma_j^2."""
        if max_bond is None and threshold is None:
            raise ValueError("compress needs max_bond, threshold or both")
        ctx = self._sync_to_device(max(self._b, 1))
        m_max = ctx.bond_capacity if max_bond is None else int(max_bond)
        bonds, _, discarded, _ = ctx.compress(m_max, 1.0 if threshold is None else threshold, rank_tol)
        self._after_device_update()
        return [int(v) for v in bonds], discarded

    def bond_spectra(self, rank_tol=1e-6):
        """(list of N-1 arrays: the normalised Schmidt spectrum of every bond, log|W|).  Nothing on the device changes."""
        ctx = self._sync_to_device(max(self._b, 1))
        ranks, sigma, log_norm = ctx.bond_spectra(rank_tol)
        return [sigma[i, :int(r)].copy() for i, r in enumerate(ranks)], log_norm

    # ------------------------------------------------------------------------------------------
    # inner products, distances and linear combinations of two MPS (not in the reference)
    # ------------------------------------------------------------------------------------------
    def _algebra_operand(self, other):
        """(cores, l_pos) of the second network, checked against this one"""
        if not isinstance(other, Network):
            raise TypeError('the second operand must be a Network, got %s' % type(other).__name__)
        if (other.N, other.D, other.L) != (self.N, self.D, self.L):
            raise ValueError('the networks differ in (N, D, L): %s and %s' % ((self.N, self.D, self.L), (other.N, other.D, other.L)))
        other._sync_to_host()
        if other._l_pos != self.l_pos:
            raise ValueError('the label sits on site %d of this network and on site %d of the other: move one of them first'
                             % (self.l_pos, other._l_pos))
        return other._host_cores, other._l_pos

    def _metric(self, metric):
        if isinstance(metric, str):
            if metric != 'uniform':
                raise ValueError("metric must be None, an array (D, D) or (N, D, D), or 'uniform'")
            return _psi_gram(self.D)
        return metric

    def inner(self, other=None, metric=None):
        """[(sign, log|.|) of <W|W>, of <V|V>, of <W|V>] for this network W and `other` V (same N, D, L and label position; any
        bonds), in float64 on the device; other None: <W|W> alone, the other two pairs (0, -inf).  metric: None (Euclidean),
        a symmetric (D, D) array for every site or (N, D, D) per site, or 'uniform' -- data_generator.psi_gram(D), with which
        <W|V> is the L2 inner product of the two models as functions of uniformly distributed pixels.  The products are
        returned as logarithms because they leave float64 at N = 784.  Nothing on the device changes."""
        ctx = self._sync_to_device(max(self._b, 1))
        if other is None:
            out = ctx.inner(None, 0, self._metric(metric))
        else:
            cores, lp = self._algebra_operand(other)
            out = ctx.inner(cores, lp, self._metric(metric))
        return [(float(s), float(v)) for s, v in out]

    def cosine(self, other, metric=None):
        """<W|V> / (|W| |V|); exactly 1.0 for a network with the same float32 cores."""
        (_, lww), (_, lvv), (s, lwv) = self.inner(other, metric)
        return s * math.exp(lwv - 0.5 * (lww + lvv)) if s != 0 else 0.0

    def distance(self, other, metric=None, relative=True):
        """|W - V| / |W| (relative) or |W - V|, from the three inner products: sqrt(max(0, 1 + <V|V>/<W|W> - 2 <W|V>/<W|W>)).
        The three terms cancel in float64: a relative distance below about 1e-6 is not resolved (it may come out as 0 or as
        noise of that size); exactly 0.0 for a network with the same float32 cores.  The absolute distance is returned as a
        float and overflows where |W| does."""
        (_, lww), (_, lvv), (s, lwv) = self.inner(other, metric)
        d2 = 1.0 + math.exp(lvv - lww) - 2.0 * s * (math.exp(lwv - lww) if s != 0 else 0.0)
        d = math.sqrt(max(0.0, d2))
        return d if relative else d * math.exp(0.5 * lww)

    def add(self, other, alpha=1.0, beta=1.0):
        """In place W <- alpha W + beta V as the direct sum: every bond becomes the sum of the two bonds, f becomes
        alpha f_W + beta f_V.  The network's M must hold the summed bonds (ValueError naming the M needed otherwise); compress
        brings them down again.  A forward is needed before the next sweep, configure_optimizer before the next stateful
        gradient_step (as after compress).  Returns the new bonds."""
        cores, lp = self._algebra_operand(other)
        ctx = self._sync_to_device(max(self._b, 1))
        _, mine, _ = ctx.get_cores()
        need = max(int(a) + int(c.shape[2]) for a, c in zip(mine, cores[:-1]))
        if need > ctx.bond_capacity:
            raise ValueError('the sum needs bonds up to %d, this network holds %d: create it with M >= %d or compress first'
                             % (need, ctx.bond_capacity, need))
        bonds = ctx.axpby(alpha, beta, cores, lp)
        self._after_device_update()
        return [int(v) for v in bonds]

    # ------------------------------------------------------------------------------------------
    # the gradient of the log-norm (not in the reference)
    # ------------------------------------------------------------------------------------------
    def _checked_metric(self, metric):
        """None, or the metric as a float64 array (D, D) or (N, D, D), symmetric and finite (ValueError otherwise)"""
        metric = self._metric(metric)
        if metric is None:
            return None
        metric = np.ascontiguousarray(metric, dtype=np.float64)
        if metric.shape not in ((self.D, self.D), (self.N, self.D, self.D)):
            raise ValueError('the metric has shape %s, neither (D, D) = %s nor (N, D, D) = %s'
                             % (metric.shape, (self.D, self.D), (self.N, self.D, self.D)))
        if not np.isfinite(metric).all():
            raise ValueError('the metric has an entry that is not finite')
        mt = np.swapaxes(metric, -1, -2)
        if not (np.abs(metric - mt) <= 1e-12 * (np.abs(metric) + np.abs(mt))).all():
            raise ValueError('the metric is not symmetric')
        return metric

    def log_norm_gradient(self, metric=None):
        """(G, (sign, log|Z|)) with Z = <W|W>_S: G a list of N float32 arrays in the canonical core shapes (ml, D, mr[, L]),
        G[i] = d log|Z| / d A_i, formed in float64 on the device from both metric environments of every site and rounded once.
        metric as for inner, 'uniform' included; with the Gram matrix of a pixel grid Z is the normaliser of sample / log_prob and
        G the model term of every likelihood gradient.  sum(G[i] * A_i) = 2 at every site; a step A_i += lr G[i] raises the norm.
        Bonds up to 64.  Nothing on the device changes."""
        metric = self._checked_metric(metric)
        ctx = self._sync_to_device(max(self._b, 1))
        return ctx.log_norm_grad(metric)

    def _likelihood_batch(self, X, y, levels, grid, weights):
        """(features (b, N, D) float32, labels (b,) int32 or None, S (D, D), -mean_s sum_i log w(x_si)) of images on the grid"""
        x, phi, w = self._pixel_grid(levels, grid, weights)
        lev = self._levels_of(X, x, 'X')
        if lev.shape[1] != self.N:
            raise ValueError('images of %d sites for a network of %d' % (lev.shape[1], self.N))
        if lev.min() < 0 or lev.max() >= len(x):
            raise ValueError('X holds levels outside [0, %d)' % len(x))
        if y is not None:
            y = np.ascontiguousarray(y, dtype=np.int32)
            if y.shape != (len(lev),):
                raise ValueError('%d images and labels of shape %s' % (len(lev), y.shape))
            if y.min() < 0 or y.max() >= self.L:
                raise ValueError('y holds labels outside [0, %d)' % self.L)
        S = np.einsum('k,kd,ke->de', w, phi, phi)
        return phi[lev].astype(np.float32), y, S, -float(np.log(w)[lev].sum(axis=1).mean())

    def nll_gradient(self, X, y=None, levels=256, grid=None, weights=None):
        """(G, nll) of a batch of images X (b, N) (pixel values on the grid, or integer levels) under the model's own distribution
        p(x, l) = prod_i w(x_i) f_l(psi(x))^2 / Z: nll = -mean(log p(x, y)), or -mean(log p(x)) with y None (the label summed), equal
        to -mean(log_prob(X, y, joint=True)[0]); G the DESCENT direction over all cores in the canonical shapes, A_i += lr G[i]
        lowers nll.  sum(G[i] * A_i) = 0 at every site: the likelihood does not see the scale of a core.  The network must be
        calibrated (f a float32; a sample with f_y == 0 raises).  Bonds up to 64.  Nothing on the device changes."""
        feats, y, S, logw = self._likelihood_batch(X, y, levels, grid, weights)
        ctx = self._sync_to_device(max(self._b, 1))
        G, out = ctx.nll_grad(feats, y, S)
        return G, float(out[0]) + logw

    def nll_gradient_indices(self, idx, labels=True, levels=256, grid=None, weights=None):
        """The same for the samples idx of the attached dataset, with its labels or (labels=False) without.  The caller sees to it
        that the dataset's pixels lie on the grid; the returned value leaves out the term -mean(sum_i log w(x_i)), which does not
        depend on the model."""
        _, phi, w = self._pixel_grid(levels, grid, weights)
        ctx = self._sync_to_device(max(self._b, 1))
        G, out = ctx.nll_grad_indices(idx, labels, np.einsum('k,kd,ke->de', w, phi, phi))
        return G, float(out[0])

    def nll(self, indices_or_X, y=None, labels=True, levels=256, grid=None, weights=None):
        """The value alone, without a gradient launch: images X (b, N) with y or None, as nll_gradient; or a one-dimensional list
        of dataset indices with `labels`, as nll_gradient_indices (the value then leaves out the sum log w term)."""
        if np.ndim(indices_or_X) == 1:
            _, phi, w = self._pixel_grid(levels, grid, weights)
            ctx = self._sync_to_device(max(self._b, 1))
            return float(ctx.nll_eval_indices(indices_or_X, labels, np.einsum('k,kd,ke->de', w, phi, phi))[0])
        feats, y, S, logw = self._likelihood_batch(indices_or_X, y, levels, grid, weights)
        ctx = self._sync_to_device(max(self._b, 1))
        return float(ctx.nll_eval(feats, y, S)[0]) + logw

    # ------------------------------------------------------------------------------------------
    # likelihood training from incomplete data
    # ------------------------------------------------------------------------------------------
    def _masked_batch(self, X, mask, y, levels, grid, weights):
        """(n, phi, w, mask (N,) or (n, N) bool, levels (n, N) int32, classes (n,) int32 or None) of partially observed images"""
        x, phi, w = self._pixel_grid(levels, grid, weights)
        n = len(X)
        m, lev = self._masked_levels(X, np.ones(self.N, dtype=bool) if mask is None else mask, x, n)
        cls = self._classes_of(y, n)
        if cls is not None and (cls.shape != (n,) or cls.min() < -1 or cls.max() >= self.L):
            raise ValueError('y must be None, an int or (n,) with values in [-1, %d)' % self.L)
        return n, phi, w, m, lev, cls

    def nll_gradient_masked(self, X, mask, y=None, levels=256, grid=None, weights=None):
        """(G, nll) of partially observed images: X (n, N) pixel values on the grid or integer levels, read where mask ((N,) or
        (n, N) bool; None: every pixel known) is set -- the other pixels are summed out exactly; y None, an int, or (n,) with -1 for
        an unlabelled sample, whose label is summed out too.  nll = -mean_s log p(x_G,s [, y_s]), equal to
        -mean(log_prob_masked(X, mask, classes=y, joint=True)) for labelled samples and -mean(log_prob_masked(X, mask)) for
        unlabelled ones; G the DESCENT direction over all cores in the canonical shapes, A_i += lr G[i] lowers nll, and
        sum(G[i] * A_i) = 0 at every site.  Float64 on the device, one rounding to float32.  The cost is O(n N m^3 D) float64 and
        (N + 1) m^2 doubles of stack a sample (2.5 MB at N = 784, bond 20): fully observed, uniformly labelled batches should keep
        using nll_gradient.  Bonds up to 64.  Nothing on the device changes."""
        n, phi, w, m, lev, cls = self._masked_batch(X, mask, y, levels, grid, weights)
        ctx = self._sync_to_device(max(self._b, 1))
        G, _, out = ctx.nll_masked_grad(n, phi, w, m, lev, cls, want=('G',))
        return G, float(out[0])

    def nll_masked(self, X, mask, y=None, levels=256, grid=None, weights=None):
        """The value of nll_gradient_masked alone: only the environments run."""
        n, phi, w, m, lev, cls = self._masked_batch(X, mask, y, levels, grid, weights)
        ctx = self._sync_to_device(max(self._b, 1))
        return float(ctx.nll_masked_grad(n, phi, w, m, lev, cls, want=())[2][0])

    def nll_step_masked(self, X, mask, y=None, lr=1e-3, weight_dec=0.0, renorm=True, levels=256, grid=None, weights=None):
        """One optimiser step (configure_optimizer) on the device on the gradient of nll_gradient_masked, at the current bonds and
        label position; X, mask, y as there, renorm as nll_step.  Returns (nll, log Z) of the batch BEFORE the step.  A batch with a
        sample of zero weight raises and changes nothing.  A forward is needed before the next sweep.  Fully observed, uniformly
        labelled batches should keep using nll_step."""
        n, phi, w, m, lev, cls = self._masked_batch(X, mask, y, levels, grid, weights)
        ctx = self._sync_to_device(max(self._b, 1))
        try:
            v = ctx.nll_masked_step(n, phi, w, m, lev, cls, lr, weight_dec, renorm)
        finally:
            self._after_device_update()
        return float(v[0]), float(v[1])

    # ------------------------------------------------------------------------------------------
    # samples and log-likelihoods of the Born distribution |f|^2 (not in the reference)
    # ------------------------------------------------------------------------------------------
    def _pixel_grid(self, levels, grid, weights):
        """(x (K,), phi (K, D), w (K,)) float64: `grid` (pixel values, default k / (K - 1) for K = levels) through psi, `weights`
        normalised to sum 1 (default 1 / K)"""
        x = np.arange(int(levels), dtype=np.float64) / (int(levels) - 1) if grid is None else np.asarray(grid, dtype=np.float64).ravel()
        K = len(x)
        w = np.full(K, 1.0 / K) if weights is None else np.asarray(weights, dtype=np.float64).ravel()
        if w.shape != (K,):
            raise ValueError('%d weights for a grid of %d levels' % (len(w), K))
        if not (np.all(np.isfinite(w)) and np.all(w > 0)):
            raise ValueError('the weights must be positive and finite')
        return x, np.ascontiguousarray(_psi(x[None, :], self.D)[0], dtype=np.float64), w / w.sum()

    @staticmethod
    def _levels_of(values, x, what):
        """integer levels as they are; pixel values -> the level of the grid point each one equals (ValueError otherwise)"""
        values = np.asarray(values)
        if values.ndim != 2:
            raise ValueError('%s must have shape (n, sites), got %s' % (what, values.shape))
        if np.issubdtype(values.dtype, np.integer):
            return np.ascontiguousarray(values, dtype=np.int32)
        order = np.argsort(x)
        pos = np.clip(np.searchsorted(x[order], values), 1, len(x) - 1)
        lo, hi = x[order][pos - 1], x[order][pos]
        near = np.where(np.abs(values - lo) <= np.abs(hi - values), pos - 1, pos)
        lev = order[near]
        if not np.all(np.abs(x[lev] - values) <= 1e-12 * np.maximum(1.0, np.abs(values))):
            raise ValueError('%s holds pixel values that are not on the grid' % what)
        return np.ascontiguousarray(lev, dtype=np.int32)

    def _classes_of(self, classes, n):
        if classes is None:
            return None
        c = np.asarray(classes)
        if c.ndim == 0:
            c = np.full(n, int(c))
        return np.ascontiguousarray(c, dtype=np.int32)

    def sample(self, n, classes=None, levels=256, grid=None, weights=None, given=None, seed=0, u=None, mask=None):
        """n exact samples of p(x, l) = prod_i w(x_i) f_l(psi(x))^2 / Z over the pixel grid, in one pass over the chain on the
        device -> (X (n, N) pixel values, labels (n,), logp (n, 2), levels (n, N)).  classes: None draws the label with the
        image; an int or an array (n,) conditions on it (-1 in the array: draw it), and the sample comes from p(x | class).
        given: (n, n_given) pixel values on the grid or integer levels of the FIRST n_given sites, which are kept; only a
        prefix can be given.  logp[:, 0] is the log-probability of the whole sample [given the class], logp[:, 1] the part of
        the given sites.  seed: the device generates the uniforms by a counter hash (repeatable); u (n, N + 1) overrides them.
        mask: (N,) or (n, N) bool with given (n, N) -- pixel values on the grid or integer levels, read where the mask is set:
        ANY set of known sites (section 23 of DESIGN.md).  Known sites come back as given; logp[:, 0] is then
        log p(drawn pixels [, drawn label] | known pixels [, class]) and logp[:, 1] is log p(known pixels [| class])."""
        x, phi, w = self._pixel_grid(levels, grid, weights)
        n = int(n)
        if mask is not None:
            m, lev = self._masked_levels(given, mask, x, n)
            ctx = self._sync_to_device(max(self._b, 1))
            lev, labels, logp = ctx.sample_masked(n, phi, w, m, lev, self._classes_of(classes, n), u, seed)
            return x[lev], labels, logp, lev
        g = None if given is None else self._levels_of(given, x, 'given')
        ctx = self._sync_to_device(max(self._b, 1))
        lev, labels, logp = ctx.sample(n, phi, w, self._classes_of(classes, n), g, u, seed)
        return x[lev], labels, logp, lev

    def log_prob(self, X_or_levels, classes=None, levels=256, grid=None, weights=None, joint=False, seed=0, u=None):
        """log-probabilities of images (n, N) (pixel values on the grid, or integer levels) -> (logp (n,), labels (n,)).
        classes None: the label is drawn from P(l | x) and logp is log p(x, that label).  classes given (int or (n,)):
        log p(x | class); with joint=True log p(x, class) = log p(x | class) + log P(class), the class weights by class_log_weights."""
        x, phi, w = self._pixel_grid(levels, grid, weights)
        lev = self._levels_of(X_or_levels, x, 'X_or_levels')
        if lev.shape[1] != self.N:
            raise ValueError('images of %d sites for a network of %d' % (lev.shape[1], self.N))
        n = len(lev)
        cls = self._classes_of(classes, n)
        ctx = self._sync_to_device(max(self._b, 1))
        _, labels, logp = ctx.sample(n, phi, w, cls, lev, u, seed)
        out = logp[:, 0].copy()
        if joint:
            if cls is None or np.any(cls < 0):
                raise ValueError('joint=True needs a class for every image')
            out += self.class_log_weights(levels, grid, weights)[cls]
        return out, labels

    def _masked_levels(self, X, mask, x, n):
        """(mask (N,) or (n, N) bool, levels (n, N) int32): _levels_of applied where the mask is set, 0 elsewhere"""
        m = np.asarray(mask) != 0
        if m.shape not in ((self.N,), (n, self.N)):
            raise ValueError('mask has shape %s, neither (%d,) nor (%d, %d)' % (m.shape, self.N, n, self.N))
        if X is None:
            if m.any():
                raise ValueError('a mask with known sites needs their values')
            return m, None
        X = np.asarray(X)
        if X.shape != (n, self.N):
            raise ValueError('the known values have shape %s, not (%d, %d)' % (X.shape, n, self.N))
        mm = np.broadcast_to(m, X.shape)
        if np.issubdtype(X.dtype, np.integer):
            return m, np.ascontiguousarray(np.where(mm, X, 0), dtype=np.int32)
        return m, self._levels_of(np.where(mm, X, x[0]), x, 'given') * mm.astype(np.int32)

    def log_prob_masked(self, X, mask, classes=None, levels=256, grid=None, weights=None, joint=False):
        """log-probabilities of partially observed images -> (n,).  X (n, N) pixel values on the grid or integer levels, read where
        mask ((N,) or (n, N) bool) is set; the other pixels are summed out by the model.  classes None: log p(x_G), the marginal
        over the label too; classes given (int or (n,)): log p(x_G | c), with joint=True log p(x_G, c)."""
        x, phi, w = self._pixel_grid(levels, grid, weights)
        n = len(X)
        m, lev = self._masked_levels(X, mask, x, n)
        cls = self._classes_of(classes, n)
        if joint and (cls is None or np.any(cls < 0)):
            raise ValueError('joint=True needs a class for every image')
        ctx = self._sync_to_device(max(self._b, 1))
        res = ctx.sample_masked(n, phi, w, m, lev, cls, draw=False, class_logw=joint)
        return res[2][:, 1] + res[3][cls] if joint else res[2][:, 1].copy()

    def classify_masked(self, X, mask, levels=256, grid=None, weights=None):
        """Classify partially observed images with the hidden pixels summed out -> (pred (n,), log_post (n, L)):
        log P(c | x_G) = log p(x_G | c) + log P(c), normalised over c; pred is its first maximum.  One device call over the n L
        rows (sample, class)."""
        x, phi, w = self._pixel_grid(levels, grid, weights)
        n, L = len(X), self.L
        m, lev = self._masked_levels(X, mask, x, n)
        ctx = self._sync_to_device(max(self._b, 1))
        rows_m = m if m.ndim == 1 else np.repeat(m, L, axis=0)
        rows_lev = None if lev is None else np.repeat(lev, L, axis=0)
        cls = np.tile(np.arange(L, dtype=np.int32), n)
        _, _, logp, clw = ctx.sample_masked(n * L, phi, w, rows_m, rows_lev, cls, draw=False, class_logw=True)
        with np.errstate(invalid='ignore'):
            lp = logp[:, 1].reshape(n, L) + clw[None, :]
        top = lp.max(axis=1, keepdims=True)
        log_post = lp - (top + np.log(np.exp(lp - top).sum(axis=1, keepdims=True)))
        return log_post.argmax(axis=1), log_post

    # ------------------------------------------------------------------------------------------
    # per-pixel conditionals: posterior means, uncertainty and surprise maps
    # ------------------------------------------------------------------------------------------
    def pixel_conditionals(self, X, mask=None, classes=None, levels=256, grid=None, weights=None):
        """What the model believes about every single pixel given the pixels it was shown, exactly, in one device call ->
        (mean, std, mode, entropy, logp_known, Q).  X (n, N) pixel values on the grid or integer levels, read where mask ((N,) or
        (n, N) bool; None: every pixel known) is set.  Per (sample, site), each (n, N): mean, std and mode (a pixel value) of
        p(x_i | the known pixels other than i [, class]) -- the posterior marginal of a hidden pixel, the leave-one-out conditional
        of a known one --, its entropy, and log p(x_i = its given value | the others) on a known pixel (0 on a hidden one).
        Q (n, N, D, D) gives the whole table through pixel_probs."""
        x, phi, w = self._pixel_grid(levels, grid, weights)
        n = len(X)
        m, lev = self._masked_levels(X, np.ones(self.N, dtype=bool) if mask is None else mask, x, n)
        ctx = self._sync_to_device(max(self._b, 1))
        q, stats, mode, _ = ctx.site_conditionals(n, phi, w, m, lev, self._classes_of(classes, n), x, want=('q', 'stats', 'mode'))
        return stats[..., 0], np.sqrt(np.maximum(stats[..., 1], 0.0)), x[mode], stats[..., 2], stats[..., 3], q

    def expected_image(self, X, mask, classes=None, levels=256, grid=None, weights=None):
        """Deterministic inpainting -> (image (n, N), std (n, N)): known pixels as given with std 0, hidden pixels the posterior mean
        given the known ones [and the class] with the posterior's standard deviation."""
        mean, std, _, _, _, _ = self.pixel_conditionals(X, mask, classes, levels, grid, weights)
        mm = np.broadcast_to(np.asarray(mask) != 0, mean.shape)
        x, _, _ = self._pixel_grid(levels, grid, weights)
        X = np.asarray(X)
        given = x[np.where(mm, X, 0)] if np.issubdtype(X.dtype, np.integer) else X.astype(np.float64)
        return np.where(mm, given, mean), np.where(mm, 0.0, std)

    def pixel_surprise(self, X, classes=None, levels=256, grid=None, weights=None):
        """-log p(x_i | all other pixels [, class]) per pixel, (n, N): where an image is unlikely.  Its sum over the sites is the
        negative log pseudo-likelihood."""
        return -self.pixel_conditionals(X, None, classes, levels, grid, weights)[4]

    def pixel_probs(self, Q, levels=256, grid=None, weights=None):
        """The table p(x_i = k | ...) (.., K) from Q (.., D, D) of pixel_conditionals, on the host:
        max(0, w_k phi_k^T Q phi_k) (Q is normalised so that the table sums to 1)"""
        _, phi, w = self._pixel_grid(levels, grid, weights)
        return np.maximum(0.0, w * np.einsum('kd,...de,ke->...k', phi, np.asarray(Q, dtype=np.float64), phi))

    # ------------------------------------------------------------------------------------------
    # pixel-pair marginals: mutual information and covariance maps
    # ------------------------------------------------------------------------------------------
    def _class_slot(self, classes):
        if classes is None:
            return -1
        c = int(classes)
        if not -1 <= c < self.L:
            raise ValueError('class %d outside [-1, %d)' % (c, self.L))
        return c

    def _pair_call(self, rows, classes, levels, grid, weights, want):
        x, phi, w = self._pixel_grid(levels, grid, weights)
        rows = np.arange(self.N, dtype=np.int32) if rows is None else np.ascontiguousarray(rows, dtype=np.int32)
        ctx = self._sync_to_device(max(self._b, 1))
        return rows, ctx.pair_marginals(phi, w, rows, self._class_slot(classes), x, want=want)

    def pixel_pair_marginals(self, rows=None, classes=None, levels=256, grid=None, weights=None):
        """The joint marginal of pairs of pixels, exactly, in one device call -> (q (R, N, D, D, D, D), q1 (N, D, D)).  rows: the
        sites i of the pairs (i, j), j > i (None: all sites); q[r, j] is zero for j <= rows[r].  classes None: the label summed; an
        int: given that class.  pair_probs gives the table p(x_i, x_j) of q, pixel_probs the table p(x_j) of q1."""
        rows, (q1, _, q, _) = self._pair_call(rows, classes, levels, grid, weights, ('q1', 'q'))
        D = self.D
        return q.reshape(len(rows), self.N, D, D, D, D), q1

    def pair_probs(self, q, levels=256, grid=None, weights=None):
        """The table p(x_i = k, x_j = k') (.., K, K) from q (.., D, D, D, D) of pixel_pair_marginals, on the host:
        max(0, w_k w_k' sum phi_k[d] phi_k[d'] q[d,d',e,e'] phi_k'[e] phi_k'[e']) (q is normalised so that the table sums to 1)"""
        _, phi, w = self._pixel_grid(levels, grid, weights)
        q = np.asarray(q, dtype=np.float64)
        G = np.einsum('kd,kx,...dxeg->...keg', phi, phi, q)
        return np.maximum(0.0, (w[:, None] * w[None, :]) * np.einsum('...keg,je,jg->...kj', G, phi, phi))

    @staticmethod
    def _symmetric(upper, diagonal):
        """the (N, N) map of its part above the diagonal (rows i, columns j > i) and its diagonal"""
        out = np.triu(upper, 1)
        out = out + out.T
        out[np.diag_indices_from(out)] = diagonal
        return out

    def mutual_information(self, classes=None, levels=256, grid=None, weights=None):
        """I(x_i; x_j) in nats for every pair of pixels, (N, N), symmetric; the diagonal is the entropy of p(x_i).  classes None:
        the label summed; an int: given that class.  How far correlations reach along the chain, and whether the pixel order puts
        strongly coupled pixels close together.  Formed as a difference of entropies: entries below about 1e-14 nats are rounding
        noise and may be slightly negative.  One device call over all rows, the same one as pixel_correlations: a caller who wants
        both maps takes them from one Context.pair_marginals call (stats[..., 0], [..., 1], [..., 2])."""
        _, (_, stats1, _, stats) = self._pair_call(None, classes, levels, grid, weights, ('stats1', 'stats'))
        return self._symmetric(stats[..., 2], stats1[:, 2])

    def pixel_correlations(self, classes=None, levels=256, grid=None, weights=None):
        """-> (cov (N, N), corr (N, N), mean (N,), std (N,)) of the pixel values under the model; both maps symmetric, the diagonals
        the variance and 1.  One device call over all rows (see mutual_information)."""
        _, (_, stats1, _, stats) = self._pair_call(None, classes, levels, grid, weights, ('stats1', 'stats'))
        return (self._symmetric(stats[..., 0], stats1[:, 1]), self._symmetric(stats[..., 1], 1.0), stats1[:, 0].copy(),
                np.sqrt(np.maximum(stats1[:, 1], 0.0)))

    def pixel_label_information(self, levels=256, grid=None, weights=None):
        """I(x_i; l) = sum_c P(c) KL(p(x_i | c) || p(x_i)) in nats, (N,): which pixels carry the class, without data.  L + 1
        per-site device calls (no pair rows) and class_log_weights."""
        none = np.zeros(0, dtype=np.int32)
        p = self.pixel_probs(self._pair_call(none, None, levels, grid, weights, ('q1',))[1][0], levels, grid, weights)
        pc = np.exp(self.class_log_weights(levels, grid, weights))
        out = np.zeros(self.N)
        for c in range(self.L):
            if not pc[c] > 0.0:
                continue
            pk = self.pixel_probs(self._pair_call(none, c, levels, grid, weights, ('q1',))[1][0], levels, grid, weights)
            with np.errstate(divide='ignore', invalid='ignore'):
                out += pc[c] * np.where((pk > 0.0) & (p > 0.0), pk * np.log(pk / p), 0.0).sum(-1)      # (p = 0 < pk: rounding at a node)
        return out

    def class_log_weights(self, levels=256, grid=None, weights=None):
        """log P(l) of the joint distribution, (L,): <W_l|W_l>_S / <W|W>_S by Network.inner under the grid's metric S, W_l the
        chain with every label slice but l zeroed"""
        _, phi, w = self._pixel_grid(levels, grid, weights)
        S = np.einsum('k,kd,ke->de', w, phi, phi)
        ctx = self._sync_to_device(max(self._b, 1))
        cores, _, lp = ctx.get_cores()
        out = np.empty(self.L)
        for c in range(self.L):
            V = list(cores)
            V[lp] = np.zeros_like(cores[lp])
            V[lp][..., c] = cores[lp][..., c]
            t = ctx.inner(V, lp, S)
            out[c] = t[1, 1] - t[0, 1] if t[1, 0] != 0 else -np.inf
        return out

    def configure_optimizer(self, optimizer='sgd', momentum=0.0, betas=(0.9, 0.999), eps=1e-8, clip=True):
        """The optimiser of gradient_step / train_gradient: 'sgd' (momentum, the reference's clip per core) or 'adam' (decoupled
        weight decay, no clip).  Resets the optimiser state."""
        self._sync_to_device().optim_config(optimizer, momentum, betas[0], betas[1], eps, clip and optimizer != 'adam')

    def gradient_step(self, indices_or_X, y=None, lr=1e-3, weight_dec=0.0):
        """One optimiser step over all cores on the device, at the current bonds and label position: the library's loss
        derivative of the batch as the cotangent of the core gradients, then A += lr * (...) in place.
        indices_or_X: indices into the attached dataset (y None), or a batch X (b, N, D) with its labels y.  Returns
        (accuracy, MAE) of the batch BEFORE the step.  A forward is needed before the next sweep."""
        if y is None:
            ctx = self._require_dataset()
            idx = np.asarray(indices_or_X)
            b = idx.size
            correct, abs_sum, _ = ctx.gd_train_indices(idx, max(b, 1), lr, weight_dec, self.act_fn, self.loss_fn, self.T)[0]
        else:
            X = getattr(indices_or_X, 'elem', indices_or_X)
            assert self.N == X.shape[1], "The 1 dimension of the input data must be the flattened number of pixels"
            ctx = self._sync_to_device(max(self._b, 1))
            b = X.shape[0]
            correct, abs_sum, _ = ctx.gd_step(X, y, lr, weight_dec, self.act_fn, self.loss_fn, self.T)
        self._after_device_update()
        return correct / b, abs_sum / (b * self.L)

    def train_gradient(self, train_index_loader, val_index_loader, lr, n_epochs=10, weight_dec=0.0, optimizer='sgd', momentum=0.0,
                       betas=(0.9, 0.999), eps=1e-8, clip=True):
        """Gradient descent over all cores from the attached dataset, the companion of `train_resident`: sweep to find the
        bonds, then fine-tune at fixed bonds (no SVD, any label position).  Every batch of the index loader is one optimiser
        step; an epoch is one device call over the concatenated batches (a ragged last batch is a call of its own).  Validation
        and the printed lines are train_resident's.  Returns (val_acc, hist), hist of shape (n_epochs, 2, n_batches): accuracy
        and MAE of every batch before its step."""
        ctx = self._require_dataset()
        self._check_forward_position(self.l_pos)
        ctx.optim_config(optimizer, momentum, betas[0], betas[1], eps, clip and optimizer != 'adam')
        val_acc, hist = [], []
        print("\n --- TRAINING PROCEDURE ---")
        for epoch in range(n_epochs):
            batches = [np.asarray(idx).ravel() for idx in train_index_loader]
            acc, mae = np.zeros(len(batches)), np.zeros(len(batches))
            i = 0
            while i < len(batches):
                # batches of one size in a row are one call: step k of it takes samples [k * size, (k + 1) * size)
                j = i + 1
                while j < len(batches) and len(batches[j]) == len(batches[i]):
                    j += 1
                try:
                    met = ctx.gd_train_indices(np.concatenate(batches[i:j]), len(batches[i]), lr, weight_dec, self.act_fn, self.loss_fn, self.T)
                finally:
                    self._after_device_update()
                sizes = np.array([len(b) for b in batches[i:j]], dtype=np.float64)
                acc[i:j] = met[:, 0] / sizes
                mae[i:j] = met[:, 1] / (sizes * self.L)
                print('\r' + "Epoch %d/%d - train accuracy : %.4f - completed : %.2f "
                      % (epoch, n_epochs, acc[j - 1], j * 100 / len(batches)) + '%', end=' ')
                i = j
            hist.append([acc, mae])
            epoch_val_acc = np.zeros(len(val_index_loader))
            for i, idx in enumerate(val_index_loader, 0):
                correct, _, _ = ctx.eval_indices(idx, self.act_fn, self.T)
                epoch_val_acc[i] = correct / len(idx)
            val_acc.append(epoch_val_acc.mean())
            print('\r' + "Epoch %d/%d - train accuracy : %.4f - val accuracy: %.4f"
                  % (epoch, n_epochs, acc.mean(), val_acc[-1]))
        return val_acc, np.array(hist)

    def nll_step(self, indices_or_X, y=None, labels=True, lr=1e-3, weight_dec=0.0, renorm=True, levels=256, grid=None, weights=None):
        """One optimiser step (configure_optimizer) on the device on the gradient of the negative log-likelihood, at the current
        bonds and label position.  indices_or_X: a one-dimensional list of indices into the attached dataset,
        with its labels or (labels=False) without -- the value then leaves out the sum log w term, as nll_gradient_indices; or images
        X (b, N) with y or None, as nll_gradient.  The metric is the Gram matrix of the grid, as nll_gradient forms it.  renorm:
        every core keeps its Frobenius norm (a plain step only ever grows it, and the likelihood does not see it).  Returns
        (nll, log Z) of the batch BEFORE the step.  A batch with a sample of f_y == 0 raises and changes nothing.  A forward is needed
        before the next sweep."""
        if np.ndim(indices_or_X) == 1:
            _, phi, w = self._pixel_grid(levels, grid, weights)
            ctx = self._require_dataset()
            idx = np.asarray(indices_or_X)
            try:
                v = ctx.nll_train_indices(idx, max(idx.size, 1), labels, np.einsum('k,kd,ke->de', w, phi, phi), lr, weight_dec, renorm)[0]
            finally:
                self._after_device_update()
            return float(v[0]), float(v[1])
        feats, y, S, logw = self._likelihood_batch(indices_or_X, y, levels, grid, weights)
        ctx = self._sync_to_device(max(self._b, 1))
        try:
            v = ctx.nll_step(feats, y, S, lr, weight_dec, renorm)
        finally:
            self._after_device_update()
        return float(v[0]) + logw, float(v[1])

    def nll_sweep(self, indices_or_X, y=None, labels=True, lr=1e-2, n_steps=None, left_dir=None, max_bond=None, threshold=1.0, renorm=True,
                  levels=256, grid=None, weights=None):
        """Two-site steps on the negative log-likelihood of one batch, on the device: merge the label site
        with its neighbour, step on the merged tensor, split it by SVD and move the label -- the DMRG-style sweep of `sweep`, on the
        objective of `nll_step`, with every bond set by the split.  indices_or_X, y, labels, the grid: as `nll_step`.  n_steps None:
        to the end of the chain.  left_dir None: right from site 0, left from site N - 1, ValueError inside the chain.  max_bond
        None: the network's M; threshold < 1: also the adaptive rank of trunc='adaptive'.
        When the label moves, the merged matrix has rank up to min(ml D, mr L): with max_bond equal to the existing bond the split
        truncates even at lr = 0 and the value can RISE (the reference's sweep geometry).  A sweep meant to descend needs a
        max_bond that holds the full rank; threshold is the way to let bonds come back down.
        Returns (values (n_steps, 6), bonds): per step the value BEFORE the step, log Z, samples with a non-finite cotangent, status
        bits, kept rank, discarded weight; and the bond dimensions after the call.  A forward is needed before the next `sweep`."""
        lp = self.l_pos
        if left_dir is None:
            if lp == 0:
                left_dir = False
            elif lp == self.N - 1:
                left_dir = True
            else:
                raise ValueError('the label is on site %d, inside the chain: nll_sweep needs left_dir' % lp)
        if n_steps is None:
            n_steps = lp if left_dir else self.N - 1 - lp
        max_bond = self.M if max_bond is None else int(max_bond)
        if np.ndim(indices_or_X) == 1:
            _, phi, w = self._pixel_grid(levels, grid, weights)
            ctx = self._require_dataset()
            try:
                vals = ctx.nll_sweep_indices(np.asarray(indices_or_X), labels, np.einsum('k,kd,ke->de', w, phi, phi), left_dir, n_steps, lr,
                                             renorm, max_bond, threshold)
            finally:
                self._after_device_update()
        else:
            feats, y, S, logw = self._likelihood_batch(indices_or_X, y, levels, grid, weights)
            ctx = self._sync_to_device(max(self._b, 1))
            try:
                vals = ctx.nll_sweep(feats, y, S, left_dir, n_steps, lr, renorm, max_bond, threshold)
            finally:
                self._after_device_update()
            vals[:, 0] += logw
        return vals, [int(v) for v in ctx.bonds()[0]]

    def _train_generative_sweep(self, ctx, train_index_loader, val_index_loader, lr, n_epochs, labels, renorm, S, max_bond, threshold):
        """train_generative(method='sweep'): one full sweep per index batch, alternating direction"""
        val_nll, hist = [], []
        max_bond = self.M if max_bond is None else int(max_bond)
        print("\n --- TRAINING PROCEDURE ---")
        for epoch in range(n_epochs):
            batches = [np.asarray(idx).ravel() for idx in train_index_loader]
            nll = np.zeros(len(batches))
            for i, idx in enumerate(batches):
                lp = self.l_pos
                if lp not in (0, self.N - 1):
                    raise ValueError('the label is on site %d, inside the chain: a sweep starts from an end' % lp)
                try:
                    nll[i] = ctx.nll_sweep_indices(idx, labels, S, lp == self.N - 1, self.N - 1, lr, renorm, max_bond, threshold)[:, 0].mean()
                finally:
                    self._after_device_update()
                print('\r' + "Epoch %d/%d - train NLL : %.4f - completed : %.2f "
                      % (epoch, n_epochs, nll[i], (i + 1) * 100 / len(batches)) + '%', end=' ')
            hist.append(nll)
            sizes = np.array([len(idx) for idx in val_index_loader], dtype=np.float64)
            epoch_val = np.array([ctx.nll_eval_indices(idx, labels, S)[0] for idx in val_index_loader])
            val_nll.append(float((epoch_val * sizes).sum() / sizes.sum()) if len(sizes) else float('nan'))
            print('\r' + "Epoch %d/%d - train NLL : %.4f - val NLL: %.4f - val accuracy: %.4f - largest bond: %d"
                  % (epoch, n_epochs, nll.mean(), val_nll[-1], self.evaluate(val_index_loader)[0] if len(sizes) else float('nan'),
                     int(ctx.bonds()[0].max())))
        return val_nll, np.array(hist)

    def train_generative(self, train_index_loader, val_index_loader, lr, n_epochs=10, weight_dec=0.0, optimizer='sgd', momentum=0.0,
                         betas=(0.9, 0.999), eps=1e-8, clip=True, labels=True, renorm=True, levels=256, grid=None, weights=None,
                         method='gradient', max_bond=None, threshold=1.0):
        """Fit the model's own distribution p(x, l) (labels=False: p(x)) to the attached dataset by gradient descent on the negative
        log-likelihood over all cores: the generative companion of `train_gradient`, at fixed bonds and any label position.  Every
        batch of the index loader is one optimiser step; an epoch is one device call with one synchronisation (batches of one size,
        the last one may be shorter; a loader of mixed sizes takes a call per run of equal sizes).  The dataset's pixels must lie on
        the grid.  Prints train_gradient's lines with the mean training NLL, the validation NLL and the validation accuracy.
        Returns (val_nll, hist), hist of shape (n_epochs, n_batches): the NLL of every batch before its step (without the sum log w
        term).
        method='sweep' (default 'gradient', the path above, untouched): every batch is one full two-site sweep of `nll_sweep`,
        alternating direction, so that every bond is set by the split (max_bond, default M; threshold); weight_dec and the
        optimiser arguments are not used, the lines printed end with the largest bond, and hist holds the mean over the steps of
        a sweep.  See `nll_sweep` on max_bond: one that truncates lets the value rise."""
        if method not in ('gradient', 'sweep'):
            raise ValueError("method %r is neither 'gradient' nor 'sweep'" % (method,))
        ctx = self._require_dataset()
        self._check_forward_position(self.l_pos)
        if method == 'sweep':
            _, phi, w = self._pixel_grid(levels, grid, weights)
            return self._train_generative_sweep(ctx, train_index_loader, val_index_loader, lr, n_epochs, labels, renorm,
                                                np.einsum('k,kd,ke->de', w, phi, phi), max_bond, threshold)
        ctx.optim_config(optimizer, momentum, betas[0], betas[1], eps, clip and optimizer != 'adam')
        _, phi, w = self._pixel_grid(levels, grid, weights)
        S = np.einsum('k,kd,ke->de', w, phi, phi)
        val_nll, hist = [], []
        print("\n --- TRAINING PROCEDURE ---")
        for epoch in range(n_epochs):
            batches = [np.asarray(idx).ravel() for idx in train_index_loader]
            nll = np.zeros(len(batches))
            i = 0
            while i < len(batches):
                # batches of one size in a row are one call, and a shorter one behind them is its ragged last step
                j = i + 1
                while j < len(batches) and len(batches[j]) == len(batches[i]):
                    j += 1
                if j == len(batches) - 1 and len(batches[j]) < len(batches[i]):
                    j += 1
                try:
                    nll[i:j] = ctx.nll_train_indices(np.concatenate(batches[i:j]), len(batches[i]), labels, S, lr, weight_dec, renorm)[:, 0]
                finally:
                    self._after_device_update()
                print('\r' + "Epoch %d/%d - train NLL : %.4f - completed : %.2f "
                      % (epoch, n_epochs, nll[j - 1], j * 100 / len(batches)) + '%', end=' ')
                i = j
            hist.append(nll)
            sizes = np.array([len(idx) for idx in val_index_loader], dtype=np.float64)
            epoch_val = np.array([ctx.nll_eval_indices(idx, labels, S)[0] for idx in val_index_loader])
            val_nll.append(float((epoch_val * sizes).sum() / sizes.sum()) if len(sizes) else float('nan'))
            print('\r' + "Epoch %d/%d - train NLL : %.4f - val NLL: %.4f - val accuracy: %.4f"
                  % (epoch, n_epochs, nll.mean(), val_nll[-1], self.evaluate(val_index_loader)[0] if len(sizes) else float('nan')))
        return val_nll, np.array(hist)

    def evaluate(self, indices, activated=True):
        """(accuracy, mean absolute error) of the network over samples of the attached dataset, reduced on the device.
        `indices` is an index loader -- the result is then the mean over its batches of the per-batch accuracy and error,
        which is what the reference's evaluation scripts print (test_diagonals.py:67-81) and differs from the overall mean
        when the last batch is ragged -- or an index array, for the overall figures.  The error is the mean over samples
        and labels of |onehot(y) - act(f)| (the MAE of `var_hist`); activated=False takes f itself."""
        ctx = self._require_dataset()
        self._check_forward_position(self.l_pos)
        act = self.act_fn if activated else 'linear'

        def one(idx):
            correct, abs_sum, nonfinite = ctx.eval_indices(idx, act, self.T)
            n = len(idx)
            return correct / n, (float('nan') if nonfinite else abs_sum / (n * self.L))
        if isinstance(indices, np.ndarray) or (isinstance(indices, (list, tuple)) and (len(indices) == 0 or np.isscalar(indices[0]))):
            return one(np.asarray(indices))
        res = np.array([one(idx) for idx in indices], dtype=np.float64).reshape(-1, 2)
        return float(res[:, 0].mean()), float(res[:, 1].mean())

    def accuracy(self, X, y, f=None):
        """Fraction of samples whose argmax over labels equals y (Network_class.py:354-380)."""
        if f is None:
            f = self.forward(X)
        y_pred = np.argmax(f.elem, axis=0)
        errors = (np.asarray(y) != y_pred).sum()
        return (len(y_pred) - errors) / len(y_pred)

    def _upload_labels(self, y_int):
        y_int = np.ascontiguousarray(y_int, dtype=np.int32)
        if self._y_dev is None or not np.array_equal(self._y_dev, y_int):
            if self._X_host is None:
                raise Exception("forward(X) must run before a sweep: no batch is resident")
            assert y_int.shape[0] == self._b, "labels and resident batch differ in length"
            self._ctx.set_labels(y_int)
            self._y_dev = y_int.copy()

    def _first_of_sweep(self, left_dir):
        return self.l_pos == (self.N - 1 if left_dir else 0)

    def _run_steps(self, f, y_int, n_steps, lr, weight_dec, L2_flag, left_dir, var_hist, debug):
        ctx = self._sync_to_device()
        self._upload_labels(y_int)
        ctx.set_f(np.asarray(f.elem, dtype=np.float32))
        first = self._first_of_sweep(left_dir)
        if first:
            # the list this direction grows starts empty (Network_class.py:426-429)
            if left_dir:
                self._r_entries, self._r_user = [], None
            else:
                self._l_entries, self._l_user = [], None
        out = None
        if debug and var_hist is not None:
            ctx.debug_enable(True)
            for k in range(n_steps):
                f_before = ctx.get_f()
                met, out = ctx.sweep(left_dir, 1, first and k == 0, lr, weight_dec, L2_flag, self.act_fn,
                                     self.loss_fn, self.T, self.trunc)
                B, dB, L2g = ctx.step_debug('B'), ctx.step_debug('dB_raw'), ctx.step_debug('L2_grad')
                sc = ctx.step_debug('scalars')
                var_hist[0].append(np.abs(B).mean())
                var_hist[1].append(np.abs(dB - L2g).mean())
                var_hist[2].append(float(met[0, 0]))
                var_hist[3].append(np.abs(f_before).mean())
                var_hist[4].append(float(met[0, 1]))
                var_hist[5].append(sc[0] if L2_flag else None)
                var_hist[6].append(np.abs(L2g).mean())
            ctx.debug_enable(False)
        else:
            met, out = ctx.sweep(left_dir, n_steps, first, lr, weight_dec, L2_flag, self.act_fn, self.loss_fn,
                                 self.T, self.trunc, want_metrics=var_hist is not None)
            if var_hist is not None:
                var_hist[0].extend(float(v) for v in met[:, 0])
                var_hist[1].extend(float(v) for v in met[:, 1])
        self._device_newer = True
        self._As = None
        self._env_epoch += 1
        # environment lists as the reference leaves them: the grown one gains one entry per step
        self._entries_after_steps(left_dir, ctx.l_pos)
        return Tensor(elem=out.astype(np.float64), axes_names=['l', 'b'])

    def sweep(self, X, y, f, lr, weight_dec, L2_flag=True, left_dir=False, var_hist=None, debug=False):
        """N-1 two-site steps in one direction (Network_class.py:384-436).  `forward(X)` must have
        run on the same batch (the reference's `train` does that); X itself is not read here,
        exactly as in the reference."""
        return self._run_steps(f, np.asarray(y), self.N - 1, lr, weight_dec, L2_flag, left_dir, var_hist, debug)

    def sweep_step(self, f, y, lr, batch_size, weight_dec, L2_flag=True, left_dir=False, var_hist=None,
                   debug=False):
        """One two-site step (Network_class.py:440-573).  `y` is the one-hot target (L, b) the
        reference passes here; the returned Tensor is f recomputed from the updated, un-truncated
        merged tensor."""
        y = np.asarray(y)
        y_int = np.argmax(y, axis=0) if y.ndim == 2 else y
        l = self.l_pos
        if left_dir and not (1 <= l <= self.N - 1):
            raise Exception('### Error ###\n l =', l, ' -> position not allowed for left sweep step')
        if not left_dir and not (0 <= l <= self.N - 2):
            raise Exception('### Error ###\n l =', l, ' -> position not allowed for right sweep step')
        return self._run_steps(f, y_int, 1, lr, weight_dec, L2_flag, left_dir, var_hist, debug)

    # ------------------------------------------------------------------------------------------
    # pieces of a step the reference exposes as methods
    # ------------------------------------------------------------------------------------------
    def _on_device_f(self, f):
        ctx = self._sync_to_device(f.elem.shape[1])
        names = [str(a) for a in f.axes_names]
        arr = np.asarray(f.elem if names[0] == 'l' else f.elem.T, dtype=np.float32)
        if self._X_host is None or arr.shape[1] != self._b:
            # no resident batch of that size: park a dummy one so that f has a home on the device
            self._b = arr.shape[1]
            ctx.set_input(np.zeros((self._b, self.N, self.D), dtype=np.float32), None)
            self._X_host = None
            self._X_idx = None
            self._y_dev = None
            self._invalidate_envs()
        ctx.set_f(arr)
        return ctx

    def apply_act_func(self, f):
        """Activation of the network output (Network_class.py:767-796)."""
        ctx = self._on_device_f(f)
        a, _ = ctx.activation(self.act_fn, self.loss_fn, self.T, want_act=True, want_der=False)
        out = Tensor(elem=a.astype(np.float64), axes_names=['l', 'b'])
        if [str(n) for n in f.axes_names][0] != 'l':
            out.transpose(f.axes_names)
        return out

    def compute_loss_derivate(self, f, y):
        """Derivative of the loss w.r.t. the (activated) output f; y one-hot (L, b)
        (Network_class.py:800-835).  `f` is the ACTIVATED output, as in the reference."""
        fa = np.asarray(f.elem if [str(n) for n in f.axes_names][0] == 'l' else f.elem.T, dtype=np.float64)
        y = np.asarray(y, dtype=np.float64)
        ctx = self._on_device_f(Tensor(elem=fa, axes_names=['l', 'b']))
        ctx.set_labels(np.argmax(y, axis=0).astype(np.int32))
        self._y_dev = None
        d = ctx.loss_derivative_of_activated(self.act_fn, self.loss_fn, self.T)
        return Tensor(elem=d.astype(np.float64), axes_names=['l', 'b'])

    def tensor_svd(self, T, left_dir=False, threshold=0.999):
        """SVD split of a 2-D Tensor ('i', 'j') with sqrt(S) on both factors (Network_class.py:839-962),
        run by the device's Jacobi kernel.  The rank kept follows `self.trunc` at the current l_pos:
        'reference' keeps all singular values next to the chain ends and `aggregations['i']['left']`
        of them elsewhere (:894-945, `threshold` is computed but unused there); 'fixed' keeps
        min(M, len(S))."""
        if type(T) != Tensor:
            raise TypeError("This function only support object from the class Tensor")
        if len(T.shape) != 2:
            raise ValueError("This function only support a 2D tensors")
        rows, cols = T.elem.shape
        nS = min(rows, cols)
        lp = self.l_pos
        adaptive = self.trunc == 'adaptive'
        if self.trunc in ('fixed', 'adaptive'):
            m = min(self.M, nS)
        else:
            interior = (1 < lp < self.N - 1) if left_dir else (0 < lp < self.N - 2)
            m = int(T.aggregations['i']['left']) if interior else nS
            if m > nS:
                # np.eye(m, m) * S[:m] in the reference (:914 / :949)
                raise ValueError("operands could not be broadcast together with shapes (%d,%d) (%d,) " % (m, m, nS))
        ctx = self._sync_to_device()
        US, SVh, sig = ctx.svd_split(np.asarray(T.elem, dtype=np.float32), m)
        if adaptive:
            # the index the reference computes and never uses (:889-891), here it decides the rank
            thr = threshold if getattr(self, '_threshold', None) is None else self._threshold
            m = min(m, int(np.argmax(np.cumsum(sig) / sig.sum() > thr)) + 1)
            US, SVh = US[:, :m], SVh[:m]
        TU = Tensor(elem=US.astype(np.float64), axes_names=['i', 'right'])
        TSVh = Tensor(elem=SVh.astype(np.float64), axes_names=['left', 'j'])
        TU.aggregations['i'] = T.aggregations['i']
        TSVh.aggregations['j'] = T.aggregations['j']
        TU.disaggregate('i')
        TSVh.disaggregate('j')
        return TU, TSVh

    def _merged_to_canonical(self, B, p):
        """Named merged Tensor on sites (p, p+1) -> (array (ml, D, D, mr, L), function mapping a canonical
        array back to a Tensor with B's own axis order)."""
        names = [str(a) for a in B.axes_names]
        want = ['left', 'd%d' % p, 'd%d' % (p + 1), 'right', 'l']
        for n in names:
            if n not in want:
                raise ValueError("axis '%s' does not belong to the merged tensor of sites (%d, %d)" % (n, p, p + 1))
        present = [n for n in want if n in names]
        arr = np.transpose(np.asarray(B.elem), [names.index(n) for n in present])
        full_shape = [arr.shape[present.index(n)] if n in present else 1 for n in want]
        canon = np.ascontiguousarray(arr.reshape(full_shape), dtype=np.float32)

        def back(c):
            t = np.asarray(c, dtype=np.float64).reshape([full_shape[want.index(n)] for n in present])
            return Tensor(elem=np.transpose(t, [present.index(n) for n in names]).copy(), axes_names=list(B.axes_names))
        return canon, back

    def update_B(self, B, f_orig, y, lr, weight_dec, L2_flag=True, ldf=0, var_hist=None, debug=False):
        """Gradient step on the merged tensor B of sites (l-ldf, l+1-ldf) (Network_class.py:577-763):
        extends the environment list behind the sweep, builds dB = sum_b loss'(f_b) phi_b, subtracts
        the L2 / weight-decay term, clips by the L1 ratio and returns B + lr dB.  `forward(X)` must
        have built the environments for this batch; cores and l_pos are left as they are."""
        left_dir = bool(ldf)
        l = self.l_pos
        if left_dir and not (1 <= l <= self.N - 1):
            raise Exception('### Error ###\n l =', l, ' -> position not allowed for left sweep step')
        if not left_dir and not (0 <= l <= self.N - 2):
            raise Exception('### Error ###\n l =', l, ' -> position not allowed for right sweep step')
        p = l - int(left_dir)
        canon, back = self._merged_to_canonical(B, p)
        y = np.asarray(y)
        y_int = np.argmax(y, axis=0) if y.ndim == 2 else y
        ctx = self._sync_to_device()
        self._upload_labels(y_int)
        fnames = [str(a) for a in f_orig.axes_names]
        f32 = np.asarray(f_orig.elem if fnames[0] == 'l' else f_orig.elem.T, dtype=np.float32)
        ctx.set_f(f32)
        if self._first_of_sweep(left_dir):
            if left_dir:
                self._r_entries, self._r_user = [], None
            else:
                self._l_entries, self._l_user = [], None
        Bnew, met = ctx.update_B(canon, left_dir, lr, weight_dec, L2_flag, self.act_fn, self.loss_fn, self.T)
        if var_hist is not None:
            if debug:
                ctx.debug_enable(True)
                Bd, dB, L2g = ctx.step_debug('B'), ctx.step_debug('dB_raw'), ctx.step_debug('L2_grad')
                sc = ctx.step_debug('scalars')
                ctx.debug_enable(False)
                var_hist[0].append(np.abs(Bd).mean())
                var_hist[1].append(np.abs(dB - L2g).mean())
                var_hist[2].append(float(met[0]))
                var_hist[3].append(np.abs(f32).mean())
                var_hist[4].append(float(met[1]))
                var_hist[5].append(sc[0] if L2_flag else None)
                var_hist[6].append(np.abs(L2g).mean())
            else:
                var_hist[0].append(float(met[0]))
                var_hist[1].append(float(met[1]))
        self._env_epoch += 1
        S_R, S_L = _hip.SIDE_RIGHT, _hip.SIDE_LEFT
        if left_dir:
            self._r_entries = [('env', S_R, i) for i in range(self.N - 1, l, -1)]
        else:
            self._l_entries = [('env', S_L, i) for i in range(0, l)]
        return back(Bnew)

    def compute_L2_reg(self, B, weight_dec=0.001, left_dir=False):
        """L2 term of the loss, weight_dec * <psi|psi> with B in place of the two cores at
        (l-ldf, l+1-ldf), and its gradient w.r.t. B (Network_class.py:966-1179).  Returns
        (float, Tensor shaped like B)."""
        left_dir = bool(left_dir)
        l = self.l_pos
        p = l - int(left_dir)
        if p < 0 or p > self.N - 2:
            raise Exception('### Error ###\n l =', l, ' -> position not allowed for %s sweep step'
                            % ('left' if left_dir else 'right'))
        canon, back = self._merged_to_canonical(B, p)
        ctx = self._sync_to_device()
        loss, grad = ctx.l2_term(canon, left_dir, weight_dec)
        return loss, back(grad)

    # ------------------------------------------------------------------------------------------
    # persistence: the whole object is pickled (training_diagonals.py:69-70)
    # ------------------------------------------------------------------------------------------
    def __getstate__(self):
        As = self.As
        return dict(N=self.N, D=self.D, L=self.L, M=self.M, T=self.T, As=As, l_pos=self._l_pos,
                    act_fn=self.act_fn, loss_fn=self.loss_fn, TX=None, r_cum_contraction=None,
                    l_cum_contraction=None, trunc=self.trunc, seg_left=bool(getattr(self, '_seg_left', False)))

    def __setstate__(self, state):
        # accepts both our own pickles and the reference's (plain __dict__ with As as Tensors)
        self.N, self.D, self.L, self.M, self.T = state['N'], state['D'], state['L'], state['M'], state['T']
        self.act_fn, self.loss_fn = state['act_fn'], state['loss_fn']
        self.trunc = state.get('trunc', 'reference')
        self._device = 0
        self._init_runtime()
        self._l_pos = state['l_pos']
        self._seg_left = bool(state.get('seg_left', False))
        cores = []
        for i, Tn in enumerate(state['As']):
            c, _ = _tensor_to_core(Tn, i, self.N)
            cores.append(np.array(c, dtype=np.float64))
        self._host_cores = cores
        self._host_newer = True


class DeviceDataset:
    """Description of the dataset `Network.attach_dataset` uploaded: n samples of N sites, stored as pixels or as
    D-component features.  The data itself lives in the network's device context."""

    def __init__(self, n, N, D, pixels):
        self.n, self.N, self.D, self.pixels = int(n), int(N), int(D), bool(pixels)

    def __len__(self):
        return self.n

    def __repr__(self):
        return 'DeviceDataset(n=%d, N=%d, D=%d, %s)' % (self.n, self.N, self.D, 'pixels' if self.pixels else 'features')


_COMPRESS_MAX_BOND = 96      # the largest bond tnml_compress takes (the LDS of its one workgroup, include/tnml.h)


def combine(nets, coeffs=None, max_bond=None, threshold=None):
    """A new Network holding sum_k coeffs[k] W_k (default: the mean) of networks with the same N, D, L and label position: the
    direct sum on the device in a temporary context (Context.axpby per network), then compress(max_bond, threshold).  Where the
    next sum would exceed the bond compress accepts (96), the partial sum is compressed first with the same arguments.  The
    result has M = max_bond (the largest bond of the sum where max_bond is None) and the first network's T, activation, loss and
    truncation policy."""
    nets = list(nets)
    if not nets:
        raise ValueError('combine needs at least one network')
    coeffs = [1.0 / len(nets)] * len(nets) if coeffs is None else [float(v) for v in coeffs]
    if len(coeffs) != len(nets):
        raise ValueError('%d coefficients for %d networks' % (len(coeffs), len(nets)))
    first = nets[0]
    first._sync_to_host()
    lp = first._l_pos
    operands = [(first._host_cores, lp)] + [first._algebra_operand(n) for n in nets[1:]]
    widths = [max([int(c.shape[2]) for c in cores[:-1]]) for cores, _ in operands]
    cap = min(sum(widths), _COMPRESS_MAX_BOND)
    if max(widths) > cap:
        raise ValueError('a network has bond %d, compress takes %d at the most' % (max(widths), cap))
    ctx = _hip.Context(first.N, first.D, first.L, cap, 1, first._device)
    try:
        cores0 = [np.asarray(c, dtype=np.float32) for c in operands[0][0]]
        ctx.set_cores(cores0, lp)
        cur = widths[0]
        m_arg = ctx.bond_capacity if max_bond is None else int(max_bond)
        thr = 1.0 if threshold is None else threshold
        for k in range(1, len(nets)):
            if cur + widths[k] > ctx.bond_capacity:
                if max_bond is None and threshold is None:
                    raise ValueError('the sum reaches bond %d, beyond %d: combine needs max_bond or threshold to compress on the way'
                                     % (cur + widths[k], ctx.bond_capacity))
                cur = int(max(ctx.compress(m_arg, thr)[0]))
                if cur + widths[k] > ctx.bond_capacity:
                    raise ValueError('the compressed partial sum (bond %d) and the next network (bond %d) exceed bond %d'
                                     % (cur, widths[k], ctx.bond_capacity))
            # the first coefficient rides on the first sum (alpha multiplies the label core once)
            cur = int(max(ctx.axpby(coeffs[0] if k == 1 else 1.0, coeffs[k], operands[k][0], lp)))
        if len(nets) == 1 and coeffs[0] != 1.0:
            cores0[lp] = (coeffs[0] * cores0[lp].astype(np.float64)).astype(np.float32)
            ctx.set_cores(cores0, lp)
        if max_bond is not None or threshold is not None:
            cur = int(max(ctx.compress(m_arg, thr)[0]))
        cores, _, lp_out = ctx.get_cores()
    finally:
        ctx.close()
    out = Network(first.N, int(max_bond) if max_bond is not None else max(cur, 1), D=first.D, L=first.L, T=first.T, act_fn=first.act_fn,
                  loss_fn=first.loss_fn, trunc=first.trunc, device=first._device)
    out._host_cores = [c.astype(np.float64) for c in cores]
    out._l_pos = lp_out
    out._host_newer = True
    return out


def _unpack_batch(data):
    """A loader batch is a list of (x_i (N, D), y_i) tuples (data_generator.py:190-192); loaders of
    this package attach the stacked arrays to the list to skip the Python loop."""
    X = getattr(data, 'X', None)
    if X is not None:
        return X, data.y
    x = np.array([data[i][0] for i in range(len(data))])
    y = np.array([data[i][1] for i in range(len(data))])
    return x, y
