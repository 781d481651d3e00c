"""ctypes binding of libtnml_hip.so (include/tnml.h).

This is the only door to the device: there is no NumPy / CPU fallback behind it.  If the shared
library is missing or no gfx950 device is visible, the calls raise -- they never compute on the
host.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('TNML_LIB', os.path.join(_HERE, 'libtnml_hip.so'))   # TNML_LIB: experiment builds

ACT = {'linear': 0, 'sigmoid': 1, 'softmax': 2}
LOSS = {'MSE': 0, 'cross_entropy': 1, 'full_cross_ent': 2}
TRUNC = {'reference': 0, 'fixed': 1, 'adaptive': 2}
SIDE_LEFT, SIDE_RIGHT = 0, 1
DATASET_FORM = {'features': 0, 'pixels': 1}
WRT = {'features': 0, 'pixels': 1}
OPTIM = {'sgd': 0, 'adam': 1}
DBG = {'B': 0, 'dB_raw': 1, 'B_new': 2, 'sigma': 3, 'scalars': 4, 'L2_grad': 5}
SITE_COND_MAX_BOND = 64      # TNML_SITE_COND_MAX_BOND of include/tnml.h: the largest bond site_conditionals takes
PAIR_MAX_BOND = 64           # TNML_PAIR_MAX_BOND of include/tnml.h: the largest bond pair_marginals takes

# every symbol include/tnml.h declares (tests check the library exports all of them)
SYMBOLS = [
    'tnml_last_error', 'tnml_version', 'tnml_device_count', 'tnml_create', 'tnml_destroy',
    'tnml_synchronize', 'tnml_comm_unique_id', 'tnml_comm_init', 'tnml_set_cores', 'tnml_cores_size',
    'tnml_get_cores', 'tnml_scale_cores', 'tnml_set_input', 'tnml_set_labels', 'tnml_forward', 'tnml_forward_logabsmax', 'tnml_f_absmax',
    'tnml_set_f', 'tnml_get_f', 'tnml_sweep', 'tnml_activation', 'tnml_get_env', 'tnml_debug_enable',
    'tnml_get_step_debug', 'tnml_l_pos', 'tnml_batch', 'tnml_timer_start', 'tnml_timer_stop',
    'tnml_profile_enable', 'tnml_profile_get', 'tnml_profile_reset', 'tnml_svd_stats', 'tnml_trunc_rank',
    'tnml_update_B', 'tnml_l2_term', 'tnml_svd_split', 'tnml_set_svd_stop', 'tnml_set_narrow_path', 'tnml_predict', 'tnml_set_trunc_threshold',
    'tnml_set_sync_interval', 'tnml_set_step_pipeline', 'tnml_stage_batch', 'tnml_select_batch', 'tnml_get_counters',
    'tnml_svd_stats_ex', 'tnml_set_persistent', 'tnml_set_chain_path', 'tnml_marker', 'tnml_set_comm_overlap', 'tnml_comm_probe', 'tnml_set_flag_handoffs',
    'tnml_dataset_attach', 'tnml_dataset_detach', 'tnml_dataset_size', 'tnml_select_indices', 'tnml_predict_indices', 'tnml_eval_indices',
    'tnml_resident_metrics', 'tnml_dataset_read', 'tnml_set_any_position',
    'tnml_input_grad', 'tnml_input_grad_indices', 'tnml_set_input_grad_chunk',
    'tnml_core_grad', 'tnml_core_grad_indices', 'tnml_set_core_grad_chunk',
    'tnml_optim_config', 'tnml_optim_reset', 'tnml_gd_train_indices', 'tnml_gd_step', 'tnml_get_core_slots',
    'tnml_orthogonalize', 'tnml_compress', 'tnml_bond_spectra',
    'tnml_set_chain_scaling', 'tnml_predict_scaled',
    'tnml_set_shape_kernels', 'tnml_fixed_shape_steps', 'tnml_set_persist_reduce', 'tnml_slice_reduce_steps',
    'tnml_inner', 'tnml_axpby',
    'tnml_sample', 'tnml_sample_masked', 'tnml_set_sample_stack_bytes', 'tnml_site_conditionals', 'tnml_pair_marginals',
    'tnml_get_bonds', 'tnml_log_norm_grad', 'tnml_nll_grad', 'tnml_nll_grad_indices', 'tnml_nll_eval', 'tnml_nll_eval_indices',
    'tnml_nll_step', 'tnml_nll_train_indices', 'tnml_set_nll_overlap',
    'tnml_nll_sweep', 'tnml_nll_sweep_indices', 'tnml_nll_sweep_debug',
    'tnml_nll_masked_grad', 'tnml_nll_masked_step',
]
NLL_SWEEP_DBG = {'B': 0, 'Gd': 1, 'Gz': 2, 'B_new': 3, 'sigma': 4}


class TnmlError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__('tnml error %d: %s' % (code, msg))
        self.code = code


_lib = None


def lib():
    """The loaded library; raises if it was not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                "%s is missing: build the HIP extension first (python -c 'import __graft_entry__ as g; "
                "g.build()' or make -C tensornetworkforml_amd/csrc).  There is no CPU fallback." % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        L.tnml_last_error.restype = C.c_char_p
        L.tnml_version.restype = C.c_char_p
        f32p, i32p, f64p = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_double)
        vp = C.c_void_p
        L.tnml_create.argtypes = [C.POINTER(vp), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
        L.tnml_destroy.argtypes = [vp]
        L.tnml_synchronize.argtypes = [vp]
        L.tnml_comm_unique_id.argtypes = [vp]
        L.tnml_comm_init.argtypes = [vp, C.c_int, C.c_int, vp]
        L.tnml_set_cores.argtypes = [vp, f32p, C.c_size_t, i32p, C.c_int]
        L.tnml_cores_size.argtypes = [vp, C.POINTER(C.c_size_t)]
        L.tnml_get_cores.argtypes = [vp, f32p, C.c_size_t, i32p, C.POINTER(C.c_int)]
        L.tnml_scale_cores.argtypes = [vp, C.c_double]
        L.tnml_set_input.argtypes = [vp, f32p, i32p, C.c_int]
        L.tnml_set_labels.argtypes = [vp, i32p, C.c_int]
        L.tnml_forward.argtypes = [vp, f32p]
        L.tnml_f_absmax.argtypes = [vp, f64p]
        L.tnml_forward_logabsmax.argtypes = [vp, f64p]
        L.tnml_set_f.argtypes = [vp, f32p]
        L.tnml_get_f.argtypes = [vp, f32p]
        L.tnml_sweep.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_int, C.c_int,
                                 C.c_int, C.c_float, C.c_int, f32p, f32p]
        L.tnml_activation.argtypes = [vp, C.c_int, C.c_int, C.c_float, C.c_int, f32p, f32p]
        L.tnml_get_env.argtypes = [vp, C.c_int, C.c_int, f32p, C.c_size_t, C.POINTER(C.c_int)]
        L.tnml_debug_enable.argtypes = [vp, C.c_int]
        L.tnml_get_step_debug.argtypes = [vp, C.c_int, f64p, C.c_size_t, C.POINTER(C.c_size_t)]
        L.tnml_l_pos.argtypes = [vp]
        L.tnml_batch.argtypes = [vp]
        L.tnml_timer_start.argtypes = [vp]
        L.tnml_timer_stop.argtypes = [vp, f64p]
        L.tnml_profile_enable.argtypes = [vp, C.c_int]
        L.tnml_profile_get.argtypes = [vp, C.c_int, f64p, C.POINTER(C.c_longlong)]
        L.tnml_profile_reset.argtypes = [vp]
        L.tnml_svd_stats.argtypes = [vp, C.c_int, f64p]
        L.tnml_svd_stats_ex.argtypes = [vp, C.c_int, f64p, C.c_int]
        L.tnml_set_persistent.argtypes = [vp, C.c_int]
        L.tnml_set_shape_kernels.argtypes = [vp, C.c_int]
        L.tnml_fixed_shape_steps.argtypes = [vp, C.POINTER(C.c_int)]
        L.tnml_set_persist_reduce.argtypes = [vp, C.c_int]
        L.tnml_slice_reduce_steps.argtypes = [vp, C.POINTER(C.c_int)]
        L.tnml_trunc_rank.argtypes = [C.c_int] * 9
        L.tnml_update_B.argtypes = [vp, f32p, C.c_int, C.c_float, C.c_float, C.c_int, C.c_int, C.c_int, C.c_float,
                                    f64p, C.c_size_t, f32p]
        L.tnml_l2_term.argtypes = [vp, f32p, C.c_int, C.c_float, f64p, f64p, C.c_size_t]
        L.tnml_set_svd_stop.argtypes = [vp, C.c_double]
        L.tnml_set_narrow_path.argtypes = [vp, C.c_int]
        L.tnml_set_chain_path.argtypes = [vp, C.c_int]
        L.tnml_set_any_position.argtypes = [vp, C.c_int]
        L.tnml_marker.argtypes = [vp, C.c_int]
        L.tnml_set_comm_overlap.argtypes = [vp, C.c_int]
        L.tnml_set_flag_handoffs.argtypes = [vp, C.c_int]
        L.tnml_comm_probe.argtypes = [vp, C.c_int, C.c_int, C.POINTER(C.c_double)]
        L.tnml_predict.argtypes = [vp, f32p, C.c_int, f32p]
        L.tnml_set_trunc_threshold.argtypes = [vp, C.c_double]
        L.tnml_set_sync_interval.argtypes = [vp, C.c_int]
        L.tnml_set_step_pipeline.argtypes = [vp, C.c_int]
        L.tnml_stage_batch.argtypes = [vp, C.c_int, f32p, i32p, C.c_int]
        L.tnml_select_batch.argtypes = [vp, C.c_int]
        L.tnml_get_counters.argtypes = [vp, f64p]
        L.tnml_svd_split.argtypes = [vp, f32p, C.c_int, C.c_int, C.c_int, f32p, f32p, f64p]
        L.tnml_dataset_attach.argtypes = [vp, f32p, i32p, C.c_int, C.c_int, C.c_int, C.c_int]
        L.tnml_dataset_detach.argtypes = [vp]
        L.tnml_dataset_size.argtypes = [vp]
        L.tnml_select_indices.argtypes = [vp, i32p, C.c_int]
        L.tnml_predict_indices.argtypes = [vp, i32p, C.c_int, f32p]
        L.tnml_eval_indices.argtypes = [vp, i32p, C.c_int, C.c_int, C.c_float, f64p]
        L.tnml_resident_metrics.argtypes = [vp, C.c_int, C.c_float, f64p]
        L.tnml_dataset_read.argtypes = [vp, i32p, C.c_int, f32p]
        L.tnml_input_grad.argtypes = [vp, f32p, C.c_int, f32p, f32p, f32p]
        L.tnml_input_grad_indices.argtypes = [vp, i32p, C.c_int, f32p, C.c_int, f32p, f32p]
        L.tnml_set_input_grad_chunk.argtypes = [vp, C.c_int]
        L.tnml_core_grad.argtypes = [vp, f32p, C.c_int, f32p, f32p, C.c_size_t, f32p]
        L.tnml_core_grad_indices.argtypes = [vp, i32p, C.c_int, f32p, f32p, C.c_size_t, f32p]
        L.tnml_set_core_grad_chunk.argtypes = [vp, C.c_int]
        L.tnml_optim_config.argtypes = [vp, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double, C.c_int]
        L.tnml_optim_reset.argtypes = [vp]
        L.tnml_get_core_slots.argtypes = [vp, f32p, C.c_size_t, f32p, C.c_size_t]
        L.tnml_gd_train_indices.argtypes = [vp, i32p, C.c_int, C.c_int, C.c_float, C.c_float, C.c_int, C.c_int, C.c_float, f64p]
        L.tnml_gd_step.argtypes = [vp, f32p, i32p, C.c_int, C.c_float, C.c_float, C.c_int, C.c_int, C.c_float, f64p]
        L.tnml_orthogonalize.argtypes = [vp, C.c_double, i32p, f64p]
        L.tnml_compress.argtypes = [vp, C.c_int, C.c_double, C.c_double, i32p, f64p, f64p, f64p]
        L.tnml_bond_spectra.argtypes = [vp, C.c_double, i32p, f64p, f64p]
        L.tnml_set_chain_scaling.argtypes = [vp, C.c_int]
        L.tnml_predict_scaled.argtypes = [vp, f32p, C.c_int, f32p, i32p]
        L.tnml_inner.argtypes = [vp, f32p, C.c_size_t, i32p, C.c_int, f64p, C.c_int, f64p]
        L.tnml_axpby.argtypes = [vp, C.c_double, C.c_double, f32p, C.c_size_t, i32p, C.c_int, i32p]
        L.tnml_sample.argtypes = [vp, C.c_int, C.c_int, f64p, f64p, i32p, i32p, C.c_int, f64p, C.c_uint64, i32p, i32p, f64p]
        L.tnml_sample_masked.argtypes = [vp, C.c_int, C.c_int, f64p, f64p, i32p, C.POINTER(C.c_uint8), C.c_int, i32p, f64p, C.c_uint64, C.c_int,
                                         i32p, i32p, f64p, f64p]
        L.tnml_set_sample_stack_bytes.argtypes = [vp, C.c_size_t]
        L.tnml_site_conditionals.argtypes = [vp, C.c_int, C.c_int, f64p, f64p, f64p, i32p, C.POINTER(C.c_uint8), C.c_int, i32p, f64p, f64p, i32p, f64p]
        L.tnml_pair_marginals.argtypes = [vp, C.c_int, f64p, f64p, f64p, C.c_int, i32p, C.c_int, f64p, f64p, f64p, f64p]
        L.tnml_get_bonds.argtypes = [vp, i32p, C.POINTER(C.c_int)]
        L.tnml_log_norm_grad.argtypes = [vp, f64p, C.c_int, f32p, C.c_size_t, f64p]
        L.tnml_nll_grad.argtypes = [vp, f32p, i32p, C.c_int, f64p, f32p, C.c_size_t, f64p]
        L.tnml_nll_grad_indices.argtypes = [vp, i32p, C.c_int, C.c_int, f64p, f32p, C.c_size_t, f64p]
        L.tnml_nll_eval.argtypes = [vp, f32p, i32p, C.c_int, f64p, f64p]
        L.tnml_nll_eval_indices.argtypes = [vp, i32p, C.c_int, C.c_int, f64p, f64p]
        L.tnml_nll_step.argtypes = [vp, f32p, i32p, C.c_int, f64p, C.c_float, C.c_float, C.c_int, f64p]
        L.tnml_nll_train_indices.argtypes = [vp, i32p, C.c_int, C.c_int, C.c_int, f64p, C.c_float, C.c_float, C.c_int, f64p]
        L.tnml_nll_sweep.argtypes = [vp, f32p, i32p, C.c_int, f64p, C.c_int, C.c_int, C.c_float, C.c_int, C.c_int, C.c_double, f64p]
        L.tnml_nll_sweep_indices.argtypes = [vp, i32p, C.c_int, C.c_int, f64p, C.c_int, C.c_int, C.c_float, C.c_int, C.c_int, C.c_double,
                                             f64p]
        L.tnml_nll_sweep_debug.argtypes = [vp, C.c_int, f64p, C.c_size_t, C.POINTER(C.c_size_t)]
        L.tnml_set_nll_overlap.argtypes = [vp, C.c_int]
        L.tnml_nll_masked_grad.argtypes = [vp, C.c_int, C.c_int, f64p, f64p, i32p, C.POINTER(C.c_uint8), C.c_int, i32p, f32p, C.c_size_t, f64p, f64p]
        L.tnml_nll_masked_step.argtypes = [vp, C.c_int, C.c_int, f64p, f64p, i32p, C.POINTER(C.c_uint8), C.c_int, i32p, C.c_float, C.c_float, C.c_int,
                                           f64p]
        _lib = L
    return _lib


def device_count():
    return int(lib().tnml_device_count())


def _chk(rc):
    if rc != 0:
        raise TnmlError(rc, lib().tnml_last_error().decode('utf-8', 'replace'))


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _ptr(a, ctype):
    return a.ctypes.data_as(C.POINTER(ctype))


def trunc_rank(policy, left_dir, p, N, ml, D, mr, L, M):
    """Rank kept by tensor_svd; negative where the reference itself raises."""
    return int(lib().tnml_trunc_rank(TRUNC[policy], int(left_dir), p, N, ml, D, mr, L, M))


def comm_unique_id():
    buf = (C.c_ubyte * 128)()
    _chk(lib().tnml_comm_unique_id(C.cast(buf, C.c_void_p)))
    return bytes(buf)


def core_shapes(bond, l_pos, D, L):
    N = len(bond) + 1
    shapes = []
    for i in range(N):
        ml = 1 if i == 0 else int(bond[i - 1])
        mr = 1 if i == N - 1 else int(bond[i])
        shapes.append((ml, D, mr, L) if i == l_pos else (ml, D, mr))
    return shapes


class Context:
    """One device context = one MPS + one resident batch (include/tnml.h)."""

    def __init__(self, N, D, L, M, b_capacity, device=0):
        self.N, self.D, self.L, self.M = int(N), int(D), int(L), int(M)
        self._h = C.c_void_p()
        _chk(lib().tnml_create(C.byref(self._h), self.N, self.D, self.L, self.M, int(b_capacity), int(device)))

    def close(self):
        if getattr(self, '_h', None) is not None and self._h:
            lib().tnml_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- multi-GPU
    def comm_init(self, rank, nranks, uid):
        buf = (C.c_ubyte * 128).from_buffer_copy(uid)
        _chk(lib().tnml_comm_init(self._h, int(rank), int(nranks), C.cast(buf, C.c_void_p)))

    # ---- parameters
    def set_cores(self, cores, l_pos):
        """cores: list of canonical arrays (ml, D, mr[, L])."""
        bond = np.array([cores[i].shape[2] for i in range(self.N - 1)], dtype=np.int32)
        flat = _f32(np.concatenate([np.asarray(c, dtype=np.float32).ravel() for c in cores]))
        _chk(lib().tnml_set_cores(self._h, _ptr(flat, C.c_float), flat.size, _ptr(bond, C.c_int32), int(l_pos)))

    def get_cores(self):
        n = C.c_size_t()
        _chk(lib().tnml_cores_size(self._h, C.byref(n)))
        flat = np.empty(n.value, dtype=np.float32)
        bond = np.empty(self.N - 1, dtype=np.int32)
        lp = C.c_int()
        _chk(lib().tnml_get_cores(self._h, _ptr(flat, C.c_float), flat.size, _ptr(bond, C.c_int32), C.byref(lp)))
        cores, off = [], 0
        for shp in core_shapes(bond, lp.value, self.D, self.L):
            k = int(np.prod(shp))
            cores.append(flat[off:off + k].reshape(shp).copy())
            off += k
        return cores, bond, lp.value

    def core_slots(self):
        """(slots (N, Mcap * D * Mcap), label buffer (Mcap * D * Mcap * L,)) as the device holds them, padding included (tests)."""
        cap = max(self.M, self.D * min(self.L, self.M))
        slots = np.empty((self.N, cap * self.D * cap), dtype=np.float32)
        lab = np.empty(cap * self.D * cap * self.L, dtype=np.float32)
        _chk(lib().tnml_get_core_slots(self._h, _ptr(slots, C.c_float), slots.size, _ptr(lab, C.c_float), lab.size))
        return slots, lab

    def scale_cores(self, factor):
        _chk(lib().tnml_scale_cores(self._h, float(factor)))

    # ---- orthogonal form about the label, compression, bond spectra
    @property
    def bond_capacity(self):
        return max(self.M, self.D * min(self.L, self.M))

    def orthogonalize(self, rank_tol=1e-6):
        """-> (bonds (N-1,), log|W|).  Every core becomes g times an isometry towards the label site, the label core g times a
        tensor of norm 1, g = exp(log|W| / N); f is unchanged."""
        bond = np.empty(self.N - 1, dtype=np.int32)
        logn = C.c_double()
        _chk(lib().tnml_orthogonalize(self._h, float(rank_tol), _ptr(bond, C.c_int32), C.byref(logn)))
        return bond, logn.value

    def compress(self, m_max, threshold=1.0, rank_tol=1e-6):
        """-> (bonds (N-1,), sigma (N-1, capacity) normalised spectra before the cut, discarded (N-1,), log|W| afterwards)"""
        bond = np.empty(self.N - 1, dtype=np.int32)
        sigma = np.zeros((self.N - 1, self.bond_capacity))
        disc = np.zeros(self.N - 1)
        logn = C.c_double()
        _chk(lib().tnml_compress(self._h, int(m_max), float(threshold), float(rank_tol), _ptr(bond, C.c_int32), _ptr(sigma, C.c_double),
                                 _ptr(disc, C.c_double), C.byref(logn)))
        return bond, sigma, disc, logn.value

    def bond_spectra(self, rank_tol=1e-6):
        """-> (ranks (N-1,), sigma (N-1, capacity), log|W|); the context is left bit for bit as it was"""
        rank = np.empty(self.N - 1, dtype=np.int32)
        sigma = np.zeros((self.N - 1, self.bond_capacity))
        logn = C.c_double()
        _chk(lib().tnml_bond_spectra(self._h, float(rank_tol), _ptr(rank, C.c_int32), _ptr(sigma, C.c_double), C.byref(logn)))
        return rank, sigma, logn.value

    # ---- inner products and linear combinations of two MPS
    def _other(self, cores):
        if len(cores) != self.N:
            raise TnmlError(-1, 'the second chain has %d cores, this context %d sites' % (len(cores), self.N))
        bond = np.array([cores[i].shape[2] for i in range(self.N - 1)], dtype=np.int32)
        flat = _f32(np.concatenate([np.asarray(c, dtype=np.float32).ravel() for c in cores]))
        return flat, bond

    def inner(self, cores=None, l_pos=0, metric=None):
        """-> float64 (3, 2): (sign, log|.|) of <W|W>, <V|V>, <W|V> for the second chain V = `cores` (canonical arrays, label on
        l_pos); cores None: <W|W> alone, the other rows (0, -inf).  metric: None, (D, D) or (N, D, D) float64, symmetric.  Nothing
        on the device changes."""
        out = np.zeros(6, dtype=np.float64)
        mp, ms = None, 0
        if metric is not None:
            metric = np.ascontiguousarray(metric, dtype=np.float64)
            if metric.shape == (self.D, self.D):
                ms = 1
            elif metric.shape == (self.N, self.D, self.D):
                ms = self.N
            else:
                raise TnmlError(-1, 'the metric has shape %s, neither (D, D) nor (N, D, D)' % (metric.shape,))
            mp = _ptr(metric, C.c_double)
        if cores is None:
            _chk(lib().tnml_inner(self._h, None, 0, None, 0, mp, ms, _ptr(out, C.c_double)))
        else:
            flat, bond = self._other(cores)
            _chk(lib().tnml_inner(self._h, _ptr(flat, C.c_float), flat.size, _ptr(bond, C.c_int32), int(l_pos), mp, ms, _ptr(out, C.c_double)))
        return out.reshape(3, 2)

    def axpby(self, alpha, beta, cores, l_pos):
        """W <- alpha W + beta V as the direct sum (every bond becomes the sum of the two) -> the new bonds (N-1,)"""
        flat, bond = self._other(cores)
        out = np.empty(self.N - 1, dtype=np.int32)
        _chk(lib().tnml_axpby(self._h, float(alpha), float(beta), _ptr(flat, C.c_float), flat.size, _ptr(bond, C.c_int32), int(l_pos),
                              _ptr(out, C.c_int32)))
        return out

    # ---- samples and log-likelihoods of the Born distribution
    def sample(self, n, phi, w, classes=None, given=None, u=None, seed=0):
        """-> (levels (n, N) int32, labels (n,) int32, logp (n, 2) float64).  phi (K, D), w (K,) float64: the grid; classes (n,) with
        -1 = draw the label (None: all -1); given (n, n_given) levels of the first sites; u (n, N + 1) uniforms in [0, 1), or None:
        the device's counter hash of (seed, sample, site).  Nothing else on the device changes."""
        n = int(n)
        phi = np.ascontiguousarray(phi, dtype=np.float64)
        w = np.ascontiguousarray(w, dtype=np.float64)
        if phi.ndim != 2 or phi.shape[1] != self.D or w.shape != (phi.shape[0],):
            raise TnmlError(-1, 'the grid has phi %s and w %s, not (K, %d) and (K,)' % (phi.shape, w.shape, self.D))
        cp = gp = up = None
        n_given = 0
        if classes is not None:
            classes = np.ascontiguousarray(classes, dtype=np.int32)
            if classes.shape != (n,):
                raise TnmlError(-1, 'classes has shape %s, not (%d,)' % (classes.shape, n))
            cp = _ptr(classes, C.c_int32)
        if given is not None:
            given = np.ascontiguousarray(given, dtype=np.int32)
            if given.ndim != 2 or given.shape[0] != n:
                raise TnmlError(-1, 'given has shape %s, not (%d, n_given)' % (given.shape, n))
            n_given = given.shape[1]
            gp = _ptr(given, C.c_int32) if n_given else None
        if u is not None:
            u = np.ascontiguousarray(u, dtype=np.float64)
            if u.shape != (n, self.N + 1):
                raise TnmlError(-1, 'u has shape %s, not (%d, %d)' % (u.shape, n, self.N + 1))
            up = _ptr(u, C.c_double)
        levels = np.empty((max(n, 0), self.N), dtype=np.int32)
        labels = np.empty(max(n, 0), dtype=np.int32)
        logp = np.empty((max(n, 0), 2), dtype=np.float64)
        _chk(lib().tnml_sample(self._h, n, phi.shape[0], _ptr(phi, C.c_double), _ptr(w, C.c_double), cp, gp, n_given, up,
                               int(seed) & 0xFFFFFFFFFFFFFFFF, _ptr(levels, C.c_int32), _ptr(labels, C.c_int32), _ptr(logp, C.c_double)))
        return levels, labels, logp

    # ---- the same given any set of known pixels
    def sample_masked(self, n, phi, w, mask, known, classes=None, u=None, seed=0, draw=True, class_logw=False):
        """-> (levels (n, N) int32 or None, labels (n,) int32, logp (n, 2) float64[, class_logw (L,)]).  mask (N,) or (n, N): the
        known sites; known (n, N) levels, read where the mask is set (None with an empty mask).  draw: levels hold the known levels
        as given and drawn ones elsewhere, logp[:, 0] = log p(drawn | known [, class]); draw=False: only logp[:, 1] =
        log p(known [| class]), logp[:, 0] = 0, levels None.  class_logw: log P(c) as a fourth result."""
        n = int(n)
        phi = np.ascontiguousarray(phi, dtype=np.float64)
        w = np.ascontiguousarray(w, dtype=np.float64)
        if phi.ndim != 2 or phi.shape[1] != self.D or w.shape != (phi.shape[0],):
            raise TnmlError(-1, 'the grid has phi %s and w %s, not (K, %d) and (K,)' % (phi.shape, w.shape, self.D))
        if mask is None:
            raise TnmlError(-1, 'mask is None')
        mask = np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8)
        if mask.shape not in ((self.N,), (n, self.N)):
            raise TnmlError(-1, 'mask has shape %s, neither (%d,) nor (%d, %d)' % (mask.shape, self.N, n, self.N))
        mask_rows = 1 if mask.ndim == 1 else n
        cp = kp = up = None
        if classes is not None:
            classes = np.ascontiguousarray(classes, dtype=np.int32)
            if classes.shape != (n,):
                raise TnmlError(-1, 'classes has shape %s, not (%d,)' % (classes.shape, n))
            cp = _ptr(classes, C.c_int32)
        if known is not None:
            known = np.ascontiguousarray(known, dtype=np.int32)
            if known.shape != (n, self.N):
                raise TnmlError(-1, 'known has shape %s, not (%d, %d)' % (known.shape, n, self.N))
            kp = _ptr(known, C.c_int32)
        if u is not None:
            u = np.ascontiguousarray(u, dtype=np.float64)
            if u.shape != (n, self.N + 1):
                raise TnmlError(-1, 'u has shape %s, not (%d, %d)' % (u.shape, n, self.N + 1))
            up = _ptr(u, C.c_double)
        levels = np.empty((max(n, 0), self.N), dtype=np.int32) if draw else None
        labels = np.empty(max(n, 0), dtype=np.int32)
        logp = np.empty((max(n, 0), 2), dtype=np.float64)
        clw = np.empty(self.L, dtype=np.float64) if class_logw else None
        _chk(lib().tnml_sample_masked(self._h, n, phi.shape[0], _ptr(phi, C.c_double), _ptr(w, C.c_double), cp, _ptr(mask, C.c_uint8), mask_rows,
                                      kp, up, int(seed) & 0xFFFFFFFFFFFFFFFF, 1 if draw else 0, None if levels is None else _ptr(levels, C.c_int32),
                                      _ptr(labels, C.c_int32), _ptr(logp, C.c_double), None if clw is None else _ptr(clw, C.c_double)))
        return (levels, labels, logp, clw) if class_logw else (levels, labels, logp)

    def set_sample_stack_bytes(self, nbytes):
        """the bytes of environment stack one chunk of sample_masked may take (default 1 GiB)"""
        _chk(lib().tnml_set_sample_stack_bytes(self._h, int(nbytes)))

    # ---- per-pixel conditionals
    def site_conditionals(self, n, phi, w, mask, known, classes=None, values=None, want=('q', 'stats', 'mode', 'logp')):
        """-> (q (n, N, D, D) float64, stats (n, N, 4) float64, mode (n, N) int32, logp (n,) float64), None for what `want` leaves out.
        p(x_i = k | the known pixels other than i [, class]) = max(0, w_k phi_k^T q phi_k) at every site: the posterior marginal of
        a free site, the leave-one-out conditional of a known one.  stats: mean and variance over `values` (K,) (None: the level
        index), entropy, log p(known level) (0 on a free site); mode: the first level of largest density; logp: log p(known
        [| class]).  mask, known, classes as sample_masked."""
        n = int(n)
        phi = np.ascontiguousarray(phi, dtype=np.float64)
        w = np.ascontiguousarray(w, dtype=np.float64)
        if phi.ndim != 2 or phi.shape[1] != self.D or w.shape != (phi.shape[0],):
            raise TnmlError(-1, 'the grid has phi %s and w %s, not (K, %d) and (K,)' % (phi.shape, w.shape, self.D))
        if mask is None:
            raise TnmlError(-1, 'mask is None')
        mask = np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8)
        if mask.shape not in ((self.N,), (n, self.N)):
            raise TnmlError(-1, 'mask has shape %s, neither (%d,) nor (%d, %d)' % (mask.shape, self.N, n, self.N))
        mask_rows = 1 if mask.ndim == 1 else n
        cp = kp = vp = None
        if classes is not None:
            classes = np.ascontiguousarray(classes, dtype=np.int32)
            if classes.shape != (n,):
                raise TnmlError(-1, 'classes has shape %s, not (%d,)' % (classes.shape, n))
            cp = _ptr(classes, C.c_int32)
        if known is not None:
            known = np.ascontiguousarray(known, dtype=np.int32)
            if known.shape != (n, self.N):
                raise TnmlError(-1, 'known has shape %s, not (%d, %d)' % (known.shape, n, self.N))
            kp = _ptr(known, C.c_int32)
        if values is not None:
            values = np.ascontiguousarray(values, dtype=np.float64)
            if values.shape != w.shape:
                raise TnmlError(-1, 'values has shape %s, not %s' % (values.shape, w.shape))
            vp = _ptr(values, C.c_double)
        m = max(n, 0)
        q = np.empty((m, self.N, self.D, self.D), dtype=np.float64) if 'q' in want else None
        stats = np.empty((m, self.N, 4), dtype=np.float64) if 'stats' in want else None
        mode = np.empty((m, self.N), dtype=np.int32) if 'mode' in want else None
        logp = np.empty(m, dtype=np.float64) if 'logp' in want else None
        _chk(lib().tnml_site_conditionals(self._h, n, phi.shape[0], _ptr(phi, C.c_double), _ptr(w, C.c_double), vp, cp, _ptr(mask, C.c_uint8),
                                          mask_rows, kp, None if q is None else _ptr(q, C.c_double),
                                          None if stats is None else _ptr(stats, C.c_double), None if mode is None else _ptr(mode, C.c_int32),
                                          None if logp is None else _ptr(logp, C.c_double)))
        return q, stats, mode, logp

    # ---- pixel-pair marginals
    def pair_marginals(self, phi, w, rows=None, class_slot=-1, values=None, want=('q1', 'stats1', 'q', 'stats')):
        """-> (q1 (N, D, D), stats1 (N, 3), q (R, N, D*D, D*D), stats (R, N, 3)) float64, None for what `want` leaves out.
        p(x_i = k, x_j = k' [| class]) = max(0, w_k w_k' sum phi_k[d] phi_k[d'] q[r, j, (d,d'), (e,e')] phi_k'[e] phi_k'[e']) for
        i = rows[r] < j, zeros for j <= i.  stats1: mean, variance, entropy of p_i over `values` (K,) (None: the level index);
        stats: covariance, correlation, mutual information in nats.  rows: distinct sites (None or empty: the per-site part
        alone); class_slot -1: the label summed, q >= 0: given class q."""
        phi = np.ascontiguousarray(phi, dtype=np.float64)
        w = np.ascontiguousarray(w, dtype=np.float64)
        if phi.ndim != 2 or phi.shape[1] != self.D or w.shape != (phi.shape[0],):
            raise TnmlError(-1, 'the grid has phi %s and w %s, not (K, %d) and (K,)' % (phi.shape, w.shape, self.D))
        rows = np.zeros(0, dtype=np.int32) if rows is None else np.ascontiguousarray(rows, dtype=np.int32)
        if rows.ndim != 1:
            raise TnmlError(-1, 'rows has shape %s, not (R,)' % (rows.shape,))
        vp = None
        if values is not None:
            values = np.ascontiguousarray(values, dtype=np.float64)
            if values.shape != w.shape:
                raise TnmlError(-1, 'values has shape %s, not %s' % (values.shape, w.shape))
            vp = _ptr(values, C.c_double)
        R, DD = rows.shape[0], self.D * self.D
        q1 = np.empty((self.N, self.D, self.D), dtype=np.float64) if 'q1' in want else None
        stats1 = np.empty((self.N, 3), dtype=np.float64) if 'stats1' in want else None
        q = np.empty((R, self.N, DD, DD), dtype=np.float64) if 'q' in want else None
        stats = np.empty((R, self.N, 3), dtype=np.float64) if 'stats' in want else None
        opt = lambda a: None if a is None else _ptr(a, C.c_double)
        _chk(lib().tnml_pair_marginals(self._h, phi.shape[0], _ptr(phi, C.c_double), _ptr(w, C.c_double), vp, int(class_slot),
                                       _ptr(rows, C.c_int32) if R else None, R, opt(q1), opt(stats1), opt(q), opt(stats)))
        return q1, stats1, q, stats

    # ---- batch
    def set_input(self, X, y=None):
        X = _f32(X)
        assert X.ndim == 3 and X.shape[1] == self.N and X.shape[2] == self.D, \
            "The 1 dimension of the input data must be the flattened number of pixels"
        yp = None
        if y is not None:
            y = np.ascontiguousarray(y, dtype=np.int32)
            assert y.shape == (X.shape[0],)
            yp = _ptr(y, C.c_int32)
        _chk(lib().tnml_set_input(self._h, _ptr(X, C.c_float), yp, X.shape[0]))
        self.b = X.shape[0]

    def stage_batch(self, slot, X, y):
        """Copy a batch into device slot `slot` (0..7); `select_batch` later makes it resident without host traffic."""
        X = _f32(X)
        assert X.ndim == 3 and X.shape[1] == self.N and X.shape[2] == self.D
        y = np.ascontiguousarray(y, dtype=np.int32)
        assert y.shape == (X.shape[0],)
        _chk(lib().tnml_stage_batch(self._h, int(slot), _ptr(X, C.c_float), _ptr(y, C.c_int32), X.shape[0]))

    def select_batch(self, slot):
        _chk(lib().tnml_select_batch(self._h, int(slot)))
        self.b = int(lib().tnml_batch(self._h))

    def set_labels(self, y):
        y = np.ascontiguousarray(y, dtype=np.int32)
        _chk(lib().tnml_set_labels(self._h, _ptr(y, C.c_int32), y.shape[0]))

    # ---- device-resident dataset
    def dataset_attach(self, data, labels, form='features'):
        """Upload a dataset once: data (n, N, D) embedded features, or (n, N) pixels in [0, 1] with form='pixels' (the feature
        map then runs on the device when a batch is formed); labels (n,).  Replaces an earlier dataset."""
        data = _f32(data)
        labels = np.ascontiguousarray(labels, dtype=np.int32)
        if form == 'pixels':
            assert data.ndim == 2, "the pixels form takes data of shape (n, N)"
            N, D = data.shape[1], self.D
        else:
            assert data.ndim == 3, "the features form takes data of shape (n, N, D)"
            N, D = data.shape[1], data.shape[2]
        assert labels.shape == (data.shape[0],)
        _chk(lib().tnml_dataset_attach(self._h, _ptr(data, C.c_float), _ptr(labels, C.c_int32), data.shape[0], N, D,
                                       DATASET_FORM[form]))

    def dataset_detach(self):
        _chk(lib().tnml_dataset_detach(self._h))

    @property
    def dataset_size(self):
        return int(lib().tnml_dataset_size(self._h))

    @staticmethod
    def _idx(idx):
        idx = np.asarray(idx)
        if idx.dtype.kind not in 'iu':
            raise TypeError('sample indices must be integers, got %s' % idx.dtype)
        if idx.size and (idx.min() < -2 ** 31 or idx.max() >= 2 ** 31):
            raise TnmlError(-1, 'sample index beyond the int32 range')
        return np.ascontiguousarray(idx.ravel(), dtype=np.int32)

    def select_indices(self, idx):
        """The dataset samples idx become the resident batch, labels included; only the index list crosses the bus."""
        idx = self._idx(idx)
        _chk(lib().tnml_select_indices(self._h, _ptr(idx, C.c_int32), idx.size))
        self.b = idx.size

    def predict_indices(self, idx):
        """f (L, b) of the dataset samples idx; the resident batch stays as it is."""
        idx = self._idx(idx)
        f = np.empty((self.L, idx.size), dtype=np.float32)
        _chk(lib().tnml_predict_indices(self._h, _ptr(idx, C.c_int32), idx.size, _ptr(f, C.c_float)))
        return f

    def eval_indices(self, idx, act_fn, T):
        """(correct samples, sum |onehot - act(f)|, non-finite samples) over the dataset samples idx, reduced on the device."""
        idx = self._idx(idx)
        out = (C.c_double * 3)()
        _chk(lib().tnml_eval_indices(self._h, _ptr(idx, C.c_int32), idx.size, ACT[act_fn], float(T), out))
        return int(out[0]), float(out[1]), int(out[2])

    def resident_metrics(self, act_fn, T):
        """The same three numbers for the resident batch, from the f the last forward / sweep left on the device."""
        out = (C.c_double * 3)()
        _chk(lib().tnml_resident_metrics(self._h, ACT[act_fn], float(T), out))
        return int(out[0]), float(out[1]), int(out[2])

    def dataset_read(self, idx):
        """The embedded samples (b, N, D) as the device forms them (tests, inspection)."""
        idx = self._idx(idx)
        X = np.empty((idx.size, self.N, self.D), dtype=np.float32)
        _chk(lib().tnml_dataset_read(self._h, _ptr(idx, C.c_int32), idx.size, _ptr(X, C.c_float)))
        return X

    # ---- input gradients
    def _cot(self, cot, b):
        if cot is None:
            return None, None
        cot = _f32(cot)
        assert cot.shape == (self.L, b), "the cotangent has shape (L, b)"
        return cot, _ptr(cot, C.c_float)

    def input_grad(self, X, cot=None):
        """(g (b, N, D), cf (b,)): g[s, i, d] = sum_l cot[l, s] d f[l, s] / d X[s, i, d] and cf = sum_l cot f, for a batch that does
        not become resident.  cot (L, b), or None for the one-hot of the predicted class."""
        X = _f32(X)
        assert X.ndim == 3 and X.shape[1] == self.N and X.shape[2] == self.D, \
            "The 1 dimension of the input data must be the flattened number of pixels"
        b = X.shape[0]
        cot, cp = self._cot(cot, b)
        g = np.empty((b, self.N, self.D), dtype=np.float32)
        cf = np.empty(b, dtype=np.float32)
        _chk(lib().tnml_input_grad(self._h, _ptr(X, C.c_float), b, cp, _ptr(g, C.c_float), _ptr(cf, C.c_float)))
        return g, cf

    def input_grad_indices(self, idx, cot=None, wrt='features'):
        """The same for the dataset samples idx.  wrt='features': g (b, N, D); wrt='pixels' (pixels-form dataset): g (b, N), the
        chain rule through the feature map."""
        idx = self._idx(idx)
        b = idx.size
        cot, cp = self._cot(cot, b)
        g = np.empty((b, self.N, self.D) if WRT[wrt] == 0 else (b, self.N), dtype=np.float32)
        cf = np.empty(b, dtype=np.float32)
        _chk(lib().tnml_input_grad_indices(self._h, _ptr(idx, C.c_int32), b, cp, WRT[wrt], _ptr(g, C.c_float), _ptr(cf, C.c_float)))
        return g, cf

    def set_input_grad_chunk(self, n):
        """Samples per pass of the input-gradient calls (rounded up to a multiple of 64); 0: the default (tests, diagnostics)."""
        _chk(lib().tnml_set_input_grad_chunk(self._h, int(n)))

    # ---- core gradients
    def _core_grad(self, call, b, cot):
        """The flat gradient of `call(cot pointer, G pointer, capacity, cf pointer)` cut into the canonical core shapes."""
        cores, bond, lp = self.get_cores()                         # (for the bonds: the C ABI hands them out with the cores)
        cot, cp = self._cot(cot, b)
        flat = np.empty(sum(c.size for c in cores), dtype=np.float32)
        cf = np.empty(b, dtype=np.float32)
        _chk(call(cp, _ptr(flat, C.c_float), flat.size, _ptr(cf, C.c_float)))
        G, off = [], 0
        for shp in core_shapes(bond, lp, self.D, self.L):
            k = int(np.prod(shp))
            G.append(flat[off:off + k].reshape(shp).copy())
            off += k
        return G, cf

    def core_grad(self, X, cot=None):
        """(G, cf): G a list of N arrays in the canonical core shapes (ml, D, mr[, L]), the derivative of sum_s cf[s] with respect to
        every core, cf (b,) = sum_l cot f, for a batch that does not become resident.  cot (L, b), or None for the one-hot of the
        predicted class."""
        X = _f32(X)
        assert X.ndim == 3 and X.shape[1] == self.N and X.shape[2] == self.D, \
            "The 1 dimension of the input data must be the flattened number of pixels"
        b = X.shape[0]
        return self._core_grad(lambda cp, gp, cap, cfp: lib().tnml_core_grad(self._h, _ptr(X, C.c_float), b, cp, gp, cap, cfp), b, cot)

    def core_grad_indices(self, idx, cot=None):
        """The same for the dataset samples idx."""
        idx = self._idx(idx)
        b = idx.size
        return self._core_grad(lambda cp, gp, cap, cfp: lib().tnml_core_grad_indices(self._h, _ptr(idx, C.c_int32), b, cp, gp, cap, cfp), b, cot)

    def set_core_grad_chunk(self, n):
        """Samples per pass of the core-gradient calls (rounded up to a multiple of 64); 0: the default (tests, diagnostics)."""
        _chk(lib().tnml_set_core_grad_chunk(self._h, int(n)))

    # ---- the gradient of the log-norm
    def log_norm_grad(self, metric=None):
        """(G, (sign, log|<W|W>_S|)): G a list of N arrays in the canonical core shapes, d log|<W|W>_S| / d A_i in float64 on the
        device, rounded once to float32.  metric: None, (D, D) or (N, D, D) float64, symmetric.  Nothing on the device changes."""
        mp, per_site = None, 0
        if metric is not None:
            metric = np.ascontiguousarray(metric, dtype=np.float64)
            if metric.shape == (self.N, self.D, self.D):
                per_site = 1
            elif metric.shape != (self.D, self.D):
                raise TnmlError(-1, 'the metric has shape %s, neither (D, D) nor (N, D, D)' % (metric.shape,))
            mp = _ptr(metric, C.c_double)
        n = C.c_size_t()
        _chk(lib().tnml_cores_size(self._h, C.byref(n)))
        flat = np.empty(n.value, dtype=np.float32)
        out = np.zeros(2, dtype=np.float64)
        _chk(lib().tnml_log_norm_grad(self._h, mp, per_site, _ptr(flat, C.c_float), flat.size, _ptr(out, C.c_double)))
        return self._cut(flat), (float(out[0]), float(out[1]))

    # ---- the likelihood of a batch and its gradient
    def _grid_metric(self, S):
        if S is None:
            return None, None
        S = np.ascontiguousarray(S, dtype=np.float64)
        if S.shape != (self.D, self.D):
            raise TnmlError(-1, 'the metric has shape %s, not (D, D)' % (S.shape,))
        return S, _ptr(S, C.c_double)

    def _cut(self, flat):
        """a flat gradient cut into the canonical core shapes (the bonds come from the host's bookkeeping: nothing is copied)"""
        bond = np.empty(self.N - 1, dtype=np.int32)
        lp = C.c_int()
        _chk(lib().tnml_get_bonds(self._h, _ptr(bond, C.c_int32), C.byref(lp)))
        G, off = [], 0
        for shp in core_shapes(bond, lp.value, self.D, self.L):
            k = int(np.prod(shp))
            G.append(flat[off:off + k].reshape(shp).copy())
            off += k
        return G

    def nll_grad(self, X, y=None, S=None):
        """(G, out3): the descent direction of -log p(x, y) (y given) or -log p(x) over all cores in the canonical shapes, and
        out3 = (-mean(log f^2 - log Z), log Z, samples with a non-finite cotangent).  X (b, N, D) features on the grid whose Gram
        matrix is S (D, D) (None: the identity)."""
        X = _f32(X)
        assert X.ndim == 3 and X.shape[1] == self.N and X.shape[2] == self.D, \
            "The 1 dimension of the input data must be the flattened number of pixels"
        yp = None
        if y is not None:
            y = np.ascontiguousarray(y, dtype=np.int32)
            assert y.shape == (X.shape[0],)
            yp = _ptr(y, C.c_int32)
        S, sp = self._grid_metric(S)
        n = C.c_size_t()
        _chk(lib().tnml_cores_size(self._h, C.byref(n)))
        flat = np.empty(n.value, dtype=np.float32)
        out = np.zeros(3, dtype=np.float64)
        _chk(lib().tnml_nll_grad(self._h, _ptr(X, C.c_float), yp, X.shape[0], sp, _ptr(flat, C.c_float), flat.size, _ptr(out, C.c_double)))
        return self._cut(flat), out

    def nll_grad_indices(self, idx, labels=True, S=None):
        """The same for the dataset samples idx, with the dataset's labels or without."""
        idx = self._idx(idx)
        S, sp = self._grid_metric(S)
        n = C.c_size_t()
        _chk(lib().tnml_cores_size(self._h, C.byref(n)))
        flat = np.empty(n.value, dtype=np.float32)
        out = np.zeros(3, dtype=np.float64)
        _chk(lib().tnml_nll_grad_indices(self._h, _ptr(idx, C.c_int32), idx.size, int(bool(labels)), sp, _ptr(flat, C.c_float), flat.size,
                                         _ptr(out, C.c_double)))
        return self._cut(flat), out

    def nll_eval(self, X, y=None, S=None):
        """out3 alone for a host batch, without a gradient launch"""
        X = _f32(X)
        assert X.ndim == 3 and X.shape[1] == self.N and X.shape[2] == self.D, \
            "The 1 dimension of the input data must be the flattened number of pixels"
        yp = None
        if y is not None:
            y = np.ascontiguousarray(y, dtype=np.int32)
            assert y.shape == (X.shape[0],)
            yp = _ptr(y, C.c_int32)
        S, sp = self._grid_metric(S)
        out = np.zeros(3, dtype=np.float64)
        _chk(lib().tnml_nll_eval(self._h, _ptr(X, C.c_float), yp, X.shape[0], sp, _ptr(out, C.c_double)))
        return out

    def nll_eval_indices(self, idx, labels=True, S=None):
        """out3 alone for the dataset samples idx"""
        idx = self._idx(idx)
        S, sp = self._grid_metric(S)
        out = np.zeros(3, dtype=np.float64)
        _chk(lib().tnml_nll_eval_indices(self._h, _ptr(idx, C.c_int32), idx.size, int(bool(labels)), sp, _ptr(out, C.c_double)))
        return out

    # ---- likelihood training
    NLL_BAD_BATCH, NLL_NOT_APPLIED = 8, 16                      # bits of a step's fourth value, beside the norm term's 1 / 2 / 4

    @staticmethod
    def _chk_values(rc, values):
        """_chk, with the per-step values of the call on the error (TNML_ERR_NONFINITE fills them before it returns)"""
        try:
            _chk(rc)
        except TnmlError as e:
            e.values = values
            raise

    def nll_step(self, X, y=None, S=None, lr=1e-3, weight_dec=0.0, renorm=True):
        """One optimiser step (optim_config) on the gradient of -log p(x, y) (y given) or -log p(x) of a host batch X (b, N, D).
        -> float64 (4,): (value before the step as nll_eval gives it, log Z before the step, samples with a non-finite cotangent,
        status bits).  renorm: every core keeps its Frobenius norm."""
        X = _f32(X)
        assert X.ndim == 3 and X.shape[1] == self.N and X.shape[2] == self.D, \
            "The 1 dimension of the input data must be the flattened number of pixels"
        yp = None
        if y is not None:
            y = np.ascontiguousarray(y, dtype=np.int32)
            assert y.shape == (X.shape[0],)
            yp = _ptr(y, C.c_int32)
        S, sp = self._grid_metric(S)
        out = np.zeros(4, dtype=np.float64)
        self._chk_values(lib().tnml_nll_step(self._h, _ptr(X, C.c_float), yp, X.shape[0], sp, float(lr), float(weight_dec),
                                             int(renorm),
                                             _ptr(out, C.c_double)), out)
        return out

    def nll_train_indices(self, idx, batch, labels=True, S=None, lr=1e-3, weight_dec=0.0, renorm=True):
        """ceil(n / batch) such steps over the dataset samples idx, batch after batch, in one call with one synchronisation.
        -> float64 (n_steps, 4), the values of nll_step per step.  After a bad step (a non-finite cotangent or norm term) no later
        step is applied; the call raises TnmlError(-7) whose .values holds the array."""
        idx = self._idx(idx)
        batch = int(batch)
        S, sp = self._grid_metric(S)
        vals = np.zeros((max(-(-idx.size // batch), 1) if batch >= 1 else 1, 4), dtype=np.float64)
        self._chk_values(lib().tnml_nll_train_indices(self._h, _ptr(idx, C.c_int32), idx.size, batch, int(bool(labels)), sp, float(lr),
                                                      float(weight_dec),
                                                      int(renorm),
                                                      _ptr(vals, C.c_double)), vals)
        return vals

    # ---- two-site likelihood sweep
    def bonds(self):
        """(bonds (N - 1,), l_pos) from the host's bookkeeping: nothing is copied from the device"""
        bond = np.empty(self.N - 1, dtype=np.int32)
        lp = C.c_int()
        _chk(lib().tnml_get_bonds(self._h, _ptr(bond, C.c_int32), C.byref(lp)))
        return bond, lp.value

    def nll_sweep(self, X, y=None, S=None, left_dir=False, n_steps=1, lr=1e-2, renorm=True, max_bond=None, threshold=1.0):
        """n_steps two-site steps on -log p(x, y) (y given) or -log p(x) of a host batch X (b, N, D), from the current l_pos in the
        given direction; the SVD of every step sets the bond (kept rank min(max_bond, short side), fewer under threshold < 1).
        -> float64 (n_steps, 6): value before the step, log Z before the step, samples with a non-finite cotangent, status bits,
        kept rank, discarded weight.  With max_bond equal to the existing bond a step truncates even at lr = 0 (the label changes
        sides) and the value may rise: a sweep meant to descend needs a max_bond that holds the full rank."""
        X = _f32(X)
        assert X.ndim == 3 and X.shape[1] == self.N and X.shape[2] == self.D, \
            "The 1 dimension of the input data must be the flattened number of pixels"
        yp = None
        if y is not None:
            y = np.ascontiguousarray(y, dtype=np.int32)
            assert y.shape == (X.shape[0],)
            yp = _ptr(y, C.c_int32)
        S, sp = self._grid_metric(S)
        vals = np.zeros((max(int(n_steps), 1), 6), dtype=np.float64)
        self._chk_values(lib().tnml_nll_sweep(self._h, _ptr(X, C.c_float), yp, X.shape[0], sp, int(bool(left_dir)), int(n_steps), float(lr),
                                              int(renorm), int(self.M if max_bond is None else max_bond), float(threshold),
                                              _ptr(vals, C.c_double)), vals)
        return vals

    def nll_sweep_indices(self, idx, labels=True, S=None, left_dir=False, n_steps=1, lr=1e-2, renorm=True, max_bond=None, threshold=1.0):
        """The same for the dataset samples idx, with the dataset's labels or without."""
        idx = self._idx(idx)
        S, sp = self._grid_metric(S)
        vals = np.zeros((max(int(n_steps), 1), 6), dtype=np.float64)
        self._chk_values(lib().tnml_nll_sweep_indices(self._h, _ptr(idx, C.c_int32), idx.size, int(bool(labels)), sp, int(bool(left_dir)),
                                                      int(n_steps), float(lr), int(renorm), int(self.M if max_bond is None else max_bond),
                                                      float(threshold), _ptr(vals, C.c_double)), vals)
        return vals

    def nll_sweep_debug(self, what):
        """'B', 'Gd', 'Gz', 'B_new' (flat float64, canonical (ml, D, D, mr, L)) or 'sigma' of the last step of the last sweep call"""
        cap = self.bond_capacity ** 2 * self.D * self.D * self.L + 128
        out = np.zeros(cap, dtype=np.float64)
        n = C.c_size_t()
        _chk(lib().tnml_nll_sweep_debug(self._h, NLL_SWEEP_DBG[what], _ptr(out, C.c_double), out.size, C.byref(n)))
        return out[:n.value].copy()

    def set_nll_overlap(self, on):
        """The norm walk of a likelihood step on a second stream beside the step's chunks (bit-equal results either way)."""
        _chk(lib().tnml_set_nll_overlap(self._h, int(on)))

    # ---- likelihood training from incomplete data
    def _masked_batch(self, n, phi, w, mask, known, classes):
        """the arguments tnml_nll_masked_grad / _step share, checked and in the ABI's types (the arrays are returned to keep them alive)"""
        phi = np.ascontiguousarray(phi, dtype=np.float64)
        w = np.ascontiguousarray(w, dtype=np.float64)
        if phi.ndim != 2 or phi.shape[1] != self.D or w.shape != (phi.shape[0],):
            raise TnmlError(-1, 'the grid has phi %s and w %s, not (K, %d) and (K,)' % (phi.shape, w.shape, self.D))
        if mask is None:
            raise TnmlError(-1, 'mask is None')
        mask = np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8)
        if mask.shape not in ((self.N,), (n, self.N)):
            raise TnmlError(-1, 'mask has shape %s, neither (%d,) nor (%d, %d)' % (mask.shape, self.N, n, self.N))
        cp = kp = None
        if classes is not None:
            classes = np.ascontiguousarray(classes, dtype=np.int32)
            if classes.shape != (n,):
                raise TnmlError(-1, 'classes has shape %s, not (%d,)' % (classes.shape, n))
            cp = _ptr(classes, C.c_int32)
        if known is not None:
            known = np.ascontiguousarray(known, dtype=np.int32)
            if known.shape != (n, self.N):
                raise TnmlError(-1, 'known has shape %s, not (%d, %d)' % (known.shape, n, self.N))
            kp = _ptr(known, C.c_int32)
        return (phi, w, mask, known, classes), (phi.shape[0], _ptr(phi, C.c_double), _ptr(w, C.c_double), cp, _ptr(mask, C.c_uint8),
                                                1 if mask.ndim == 1 else n, kp)

    def nll_masked_grad(self, n, phi, w, mask, known, classes=None, want=('G', 'logp')):
        """-> (G, logp (n,), out4): the descent direction of -mean_s log p(known pixels of s [, class of s]) over all cores in the
        canonical shapes, every sample with its own mask (mask (N,) or (n, N), known (n, N) levels read where it is set) and its own
        class (classes (n,), -1: unknown and summed; None: all -1); logp[s] = log p(x_G,s [, c_s]); out4 = (the value -mean(logp),
        log Z, samples of zero weight or a non-finite likelihood, status bits).  `want` without 'G': the value alone, only the
        environments run.  A bad sample raises TnmlError(-7) whose .values holds out4.  Nothing on the device changes."""
        n = int(n)
        keep, (K, pp, wp, cp, mp, mask_rows, kp) = self._masked_batch(n, phi, w, mask, known, classes)
        flat, fp, cap = None, None, 0
        if 'G' in want:
            sz = C.c_size_t()
            _chk(lib().tnml_cores_size(self._h, C.byref(sz)))
            flat = np.empty(sz.value, dtype=np.float32)
            fp, cap = _ptr(flat, C.c_float), flat.size
        logp = np.empty(max(n, 0), dtype=np.float64) if 'logp' in want else None
        out = np.zeros(4, dtype=np.float64)
        self._chk_values(lib().tnml_nll_masked_grad(self._h, n, K, pp, wp, cp, mp, mask_rows, kp, fp, cap,
                                                    None if logp is None else _ptr(logp, C.c_double), _ptr(out, C.c_double)), out)
        return (None if flat is None else self._cut(flat)), logp, out

    def nll_masked_step(self, n, phi, w, mask, known, classes=None, lr=1e-3, weight_dec=0.0, renorm=True):
        """One optimiser step (optim_config) on the gradient of nll_masked_grad -> float64 (4,): out4 of the batch BEFORE the step,
        its bits joined by 8 (a bad sample) and 16 (not applied).  A bad batch raises TnmlError(-7) whose .values holds the array and
        leaves cores and optimiser state untouched."""
        n = int(n)
        keep, (K, pp, wp, cp, mp, mask_rows, kp) = self._masked_batch(n, phi, w, mask, known, classes)
        out = np.zeros(4, dtype=np.float64)
        self._chk_values(lib().tnml_nll_masked_step(self._h, n, K, pp, wp, cp, mp, mask_rows, kp, float(lr), float(weight_dec), int(renorm),
                                                    _ptr(out, C.c_double)), out)
        return out

    # ---- gradient training over all cores
    def optim_config(self, kind='sgd', momentum=0.0, beta1=0.9, beta2=0.999, eps=1e-8, clip=True):
        """The optimiser of gd_train_indices / gd_step: 'sgd' (momentum, per-core clip) or 'adam' (clip must be off).  Also
        resets the optimiser state."""
        if kind not in OPTIM:
            raise TnmlError(-1, 'unknown optimiser %r' % (kind,))
        _chk(lib().tnml_optim_config(self._h, OPTIM[kind], float(momentum), float(beta1), float(beta2), float(eps), int(bool(clip))))

    def optim_reset(self):
        """Zero vel / m / v, t = 0, and bind the state to the current bonds and l_pos."""
        _chk(lib().tnml_optim_reset(self._h))

    def gd_train_indices(self, idx, batch, lr, weight_dec, act_fn, loss_fn, T):
        """ceil(n / batch) optimiser steps over the dataset samples idx, batch after batch, in one call with one
        synchronisation.  -> float64 (n_steps, 3): (correct, sum |onehot - act(f)|, non-finite samples) of every batch before
        its step."""
        idx = self._idx(idx)
        batch = int(batch)
        met = np.zeros((max(-(-idx.size // batch), 1) if batch >= 1 else 1, 3), dtype=np.float64)
        _chk(lib().tnml_gd_train_indices(self._h, _ptr(idx, C.c_int32), idx.size, batch, float(lr), float(weight_dec), ACT[act_fn],
                                         LOSS[loss_fn], float(T), _ptr(met, C.c_double)))
        return met

    def gd_step(self, X, y, lr, weight_dec, act_fn, loss_fn, T):
        """One optimiser step on a host batch X (b, N, D), y (b,) -> (correct, sum |onehot - act(f)|, non-finite samples)
        of the batch before the step."""
        X = _f32(X)
        assert X.ndim == 3 and X.shape[1] == self.N and X.shape[2] == self.D, \
            "The 1 dimension of the input data must be the flattened number of pixels"
        y = np.ascontiguousarray(y, dtype=np.int32)
        assert y.shape == (X.shape[0],)
        out = (C.c_double * 3)()
        _chk(lib().tnml_gd_step(self._h, _ptr(X, C.c_float), _ptr(y, C.c_int32), X.shape[0], float(lr), float(weight_dec), ACT[act_fn],
                                LOSS[loss_fn], float(T), out))
        return int(out[0]), float(out[1]), int(out[2])

    # ---- hot path
    def forward(self, want_f=True):
        if not want_f:
            _chk(lib().tnml_forward(self._h, None))
            return None
        f = np.empty((self.L, self.b), dtype=np.float32)
        _chk(lib().tnml_forward(self._h, _ptr(f, C.c_float)))
        return f

    def predict(self, X):
        """f (L, b) for a batch that does not become resident (no environments are stored)."""
        X = _f32(X)
        assert X.ndim == 3 and X.shape[1] == self.N and X.shape[2] == self.D, \
            "The 1 dimension of the input data must be the flattened number of pixels"
        f = np.empty((self.L, X.shape[0]), dtype=np.float32)
        _chk(lib().tnml_predict(self._h, _ptr(X, C.c_float), X.shape[0], _ptr(f, C.c_float)))
        return f

    def predict_scaled(self, X):
        """(mant (L, b) float32, expo (b,) int32) with f[l, s] = mant[l, s] * 2 ** expo[s] and 0.5 <= max_l |mant[l, s]| < 1: the
        output of a batch that does not become resident, readable where f itself lies outside float32 (include/tnml.h).  A sample
        whose f is all zero or not finite has expo 0 and the values as they are.  np.ldexp(mant.astype(np.float64), expo) is f."""
        X = _f32(X)
        assert X.ndim == 3 and X.shape[1] == self.N and X.shape[2] == self.D, \
            "The 1 dimension of the input data must be the flattened number of pixels"
        mant = np.empty((self.L, X.shape[0]), dtype=np.float32)
        expo = np.empty(X.shape[0], dtype=np.int32)
        _chk(lib().tnml_predict_scaled(self._h, _ptr(X, C.c_float), X.shape[0], _ptr(mant, C.c_float), _ptr(expo, C.c_int32)))
        return mant, expo

    def forward_logabsmax(self):
        """log max|f| of the resident batch, exact even where f under/overflows float32."""
        v = C.c_double()
        _chk(lib().tnml_forward_logabsmax(self._h, C.byref(v)))
        return v.value

    def f_absmax(self):
        v = C.c_double()
        _chk(lib().tnml_f_absmax(self._h, C.byref(v)))
        return v.value

    def set_f(self, f):
        f = _f32(f)
        assert f.shape == (self.L, self.b)
        _chk(lib().tnml_set_f(self._h, _ptr(f, C.c_float)))

    def get_f(self):
        f = np.empty((self.L, self.b), dtype=np.float32)
        _chk(lib().tnml_get_f(self._h, _ptr(f, C.c_float)))
        return f

    def sweep(self, left_dir, n_steps, first_of_sweep, lr, weight_dec, L2_flag, act_fn, loss_fn, T, trunc,
              want_metrics=True, want_f=True):
        met = np.empty((n_steps, 2), dtype=np.float32) if want_metrics else None
        f = np.empty((self.L, self.b), dtype=np.float32) if want_f else None
        _chk(lib().tnml_sweep(self._h, int(bool(left_dir)), int(n_steps), int(bool(first_of_sweep)), float(lr),
                              float(weight_dec), int(bool(L2_flag)), ACT[act_fn], LOSS[loss_fn], float(T),
                              TRUNC[trunc], _ptr(met, C.c_float) if want_metrics else None,
                              _ptr(f, C.c_float) if want_f else None))
        return met, f

    def update_B(self, B, left_dir, lr, weight_dec, L2_flag, act_fn, loss_fn, T):
        """Updated merged tensor of the two sites at l_pos (canonical (ml, D, D, mr, L)) and the step's
        (accuracy, MAE); B = None uses the product of the two cores."""
        shape = None
        bp = None
        if B is not None:
            B = _f32(B)
            shape = B.shape
            bp = _ptr(B, C.c_float)
        cap = 4 * max(self.M, self.D * self.L) ** 2 * self.D * self.D * self.L
        out = np.empty(cap, dtype=np.float64)
        met = np.empty(2, dtype=np.float32)
        _chk(lib().tnml_update_B(self._h, bp, int(bool(left_dir)), float(lr), float(weight_dec), int(bool(L2_flag)),
                                 ACT[act_fn], LOSS[loss_fn], float(T), _ptr(out, C.c_double), out.size,
                                 _ptr(met, C.c_float)))
        return (out[:int(np.prod(shape))].reshape(shape).copy() if shape is not None else out), met

    def l2_term(self, B, left_dir, weight_dec):
        """(wd <B, Ln.B.Rn>, 2 wd Ln.B.Rn) for a merged tensor B (canonical layout) at l_pos."""
        B = _f32(B)
        grad = np.empty(B.size, dtype=np.float64)
        loss = C.c_double()
        _chk(lib().tnml_l2_term(self._h, _ptr(B, C.c_float), int(bool(left_dir)), float(weight_dec), C.byref(loss),
                                _ptr(grad, C.c_double), grad.size))
        return loss.value, grad.reshape(B.shape)

    def svd_split(self, mat, m):
        """(U sqrt(S) [rows, m], sqrt(S) Vh [m, cols], all singular values) of a 2-D matrix."""
        mat = _f32(mat)
        rows, cols = mat.shape
        US = np.empty((rows, int(m)), dtype=np.float32)
        SVh = np.empty((int(m), cols), dtype=np.float32)
        sig = np.empty(min(rows, cols), dtype=np.float64)
        _chk(lib().tnml_svd_split(self._h, _ptr(mat, C.c_float), rows, cols, int(m), _ptr(US, C.c_float),
                                  _ptr(SVh, C.c_float), _ptr(sig, C.c_double)))
        return US, SVh, sig

    def activation(self, act_fn, loss_fn, T, want_act=True, want_der=False, input_is_activated=False):
        a = np.empty((self.L, self.b), dtype=np.float32) if want_act else None
        d = np.empty((self.L, self.b), dtype=np.float32) if want_der else None
        _chk(lib().tnml_activation(self._h, ACT[act_fn], LOSS[loss_fn], float(T), int(bool(input_is_activated)),
                                   _ptr(a, C.c_float) if want_act else None,
                                   _ptr(d, C.c_float) if want_der else None))
        return a, d

    def loss_derivative_of_activated(self, act_fn, loss_fn, T):
        return self.activation(act_fn, loss_fn, T, want_act=False, want_der=True, input_is_activated=True)[1]

    # ---- inspection
    def get_env(self, side, site):
        out = np.empty(self.b * max(self.M, self.D * self.L) * 2, dtype=np.float32)
        m = C.c_int()
        _chk(lib().tnml_get_env(self._h, int(side), int(site), _ptr(out, C.c_float), out.size, C.byref(m)))
        return out[:self.b * m.value].reshape(self.b, m.value).copy()

    def set_svd_stop(self, stop2):
        """Jacobi stopping threshold on g^2 / scale^2 (include/tnml.h); default 1e-6."""
        _chk(lib().tnml_set_svd_stop(self._h, float(stop2)))

    def set_trunc_threshold(self, threshold):
        """Cumulative-share threshold of trunc='adaptive' (default 0.999)."""
        _chk(lib().tnml_set_trunc_threshold(self._h, float(threshold)))

    def set_step_pipeline(self, on):
        """True (default): one launch per sweep step (pipelined); False: the classic launch sequence."""
        _chk(lib().tnml_set_step_pipeline(self._h, int(on)))

    def set_persistent(self, on=True):
        """1 / True (default): a full sweep as ONE persistent launch; 2: one launch per role on three streams; 0 / False: one launch per step."""
        _chk(lib().tnml_set_persistent(self._h, int(on)))

    def set_shape_kernels(self, on=True):
        """True (default): steps of a persistent sweep whose shape is in the compiled table run the body compiled for it; False: the generic body everywhere."""
        _chk(lib().tnml_set_shape_kernels(self._h, int(bool(on))))

    def fixed_shape_steps(self):
        """Steps of the last persistent sweep that ran a body compiled for their shape."""
        v = C.c_int()
        _chk(lib().tnml_fixed_shape_steps(self._h, C.byref(v)))
        return v.value

    def set_persist_reduce(self, mode=1):
        """1 (default): a persistent sweep reduces pre-gradients beyond one level in slices, by many workgroups; 0: by last arrivers."""
        _chk(lib().tnml_set_persist_reduce(self._h, int(mode)))

    def slice_reduce_steps(self):
        """Batch-side iterations of the last persistent sweep that reduced in slices."""
        v = C.c_int()
        _chk(lib().tnml_slice_reduce_steps(self._h, C.byref(v)))
        return v.value

    def set_sync_interval(self, n_steps):
        """Drain the stream every n_steps sweep steps (0: never); for runs under a dispatch-intercepting profiler."""
        _chk(lib().tnml_set_sync_interval(self._h, int(n_steps)))

    def set_comm_overlap(self, on=True):
        """Communicator path: update side and batch side + all-reduce on two streams (default) or one fused launch per step."""
        _chk(lib().tnml_set_comm_overlap(self._h, int(bool(on))))

    def comm_probe(self, n_floats, reps=200):
        """Mean device time (us) of one all-reduce of n_floats floats on the exchange stream (collective call)."""
        v = C.c_double()
        _chk(lib().tnml_comm_probe(self._h, int(n_floats), int(reps), C.byref(v)))
        return v.value

    def set_flag_handoffs(self, on=True):
        """hand-offs between the context's two streams as sequence numbers in memory (default) or as events (tools that
        serialise dispatches: rocprofv3 --pmc)"""
        _chk(lib().tnml_set_flag_handoffs(self._h, int(bool(on))))

    def set_chain_path(self, force_plain):
        """Forward chain as plain FMAs (True) instead of the matrix-core kernel (tests, diagnostics)."""
        _chk(lib().tnml_set_chain_path(self._h, int(bool(force_plain))))

    def set_any_position(self, on=True):
        """True: forward / predict / predict_indices / eval_indices also run with the label at an intermediate site, and a
        forward there lets one sweep call start a segment in either direction (include/tnml.h); False (default): ends only."""
        _chk(lib().tnml_set_any_position(self._h, int(bool(on))))

    def set_chain_scaling(self, on=True):
        """True: predict / predict_indices / eval_indices, both gradient calls and the gradient-training calls carry a power-of-two
        exponent per sample along their chains, so that partial products outside float32 no longer spoil a representable result
        (include/tnml.h); False (default): the plain chains.  Anything but 0 / 1 is refused."""
        _chk(lib().tnml_set_chain_scaling(self._h, int(on)))

    def set_narrow_path(self, force_large):
        """True: every step takes the large-tensor (HBM-resident) path; False: automatic."""
        _chk(lib().tnml_set_narrow_path(self._h, int(bool(force_large))))

    def debug_enable(self, on=True):
        """True / 1: capture every step's tensors; 2: cycle stamps only; 4: check every launch; False / 0: off."""
        _chk(lib().tnml_debug_enable(self._h, int(on)))

    def step_debug(self, what):
        cap = max(4 * max(self.M, self.D * self.L) ** 2 * self.D * self.D * self.L + 64, 512)
        out = np.empty(cap, dtype=np.float64)
        n = C.c_size_t()
        _chk(lib().tnml_get_step_debug(self._h, DBG[what], _ptr(out, C.c_double), out.size, C.byref(n)))
        return out[:n.value].copy()

    @property
    def l_pos(self):
        return int(lib().tnml_l_pos(self._h))

    def synchronize(self):
        _chk(lib().tnml_synchronize(self._h))

    # ---- measurement
    def marker(self, marker_id):
        """Phase boundary for profilers: an empty kernel of `marker_id` workgroups on the context's stream."""
        _chk(lib().tnml_marker(self._h, int(marker_id)))

    def timer_start(self):
        _chk(lib().tnml_timer_start(self._h))

    def timer_stop(self):
        ms = C.c_double()
        _chk(lib().tnml_timer_stop(self._h, C.byref(ms)))
        return ms.value

    def profile_enable(self, on=True):
        """True / 1: events around every launch (synchronising); 2: one event pair per sweep call; False / 0: off."""
        _chk(lib().tnml_profile_enable(self._h, int(on)))

    def profile_reset(self):
        _chk(lib().tnml_profile_reset(self._h))

    def svd_stats(self, reset=False):
        """(total Jacobi sweeps, SVDs, total rounds) since the last reset; `cholesky_steps` holds the fourth counter."""
        out = (C.c_double * 4)()
        _chk(lib().tnml_svd_stats_ex(self._h, int(bool(reset)), out, 4))
        self.cholesky_steps = out[3]
        return out[0], out[1], out[2]

    def counters(self):
        """Work since the last profile_reset: dict of sweep steps, algorithmic bytes / flops, forwards, launches, device ms."""
        out = (C.c_double * 8)()
        _chk(lib().tnml_get_counters(self._h, out))
        keys = ('sweep_steps', 'algorithmic_bytes', 'algorithmic_flops', 'forwards', 'forward_bytes', 'launches', 'pipelined_steps', 'sweep_device_ms')
        return dict(zip(keys, [float(v) for v in out]))

    def profile_get(self, which):
        ms, n = C.c_double(), C.c_longlong()
        _chk(lib().tnml_profile_get(self._h, int(which), C.byref(ms), C.byref(n)))
        return ms.value, n.value
