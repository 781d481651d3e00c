"""Range-safe chains (test infrastructure): networks whose f is of order 1 while partial products of their
chain leave float32.  Imported by tests/test_scaled_chain_host.py and tests/test_scaled_chain_gpu.py.

decalibrate(cores, k) multiplies core i by 2^k[i].  That is exact in float32 (no core of the tests comes near the ends of the
exponent range), so the float64 references -- input_grad_reference, core_grad_reference, forward64 of
tests/gradient_step_reference.py, label_inside_forward of tests/test_any_position_host.py -- run on the very numbers the device
holds.

The balanced pattern for N = 17: k = +20 on sites 0..7, 0 on site 8, -20 on sites 9..16.  The product of the factors is 1, so f
and the input gradient g equal the calibrated network's exactly, and the gradient of core i differs by 2^-k[i].  The prefix
products reach 2^160 and the suffix products 2^-160, outside float32 either way (largest finite value about 2^128, smallest
subnormal 2^-149).
"""
import numpy as np

BALANCED_N = 17


def balanced_pattern():
    """k [17]: +20 on sites 0..7, 0 on site 8, -20 on sites 9..16"""
    return np.array([20] * 8 + [0] + [-20] * 8, dtype=np.int64)


def decalibrate(cores, k):
    """core i times 2^k[i], in the dtype of the core (exact: a power of two only moves the exponent)"""
    assert len(cores) == len(k)
    out = []
    for c, ki in zip(cores, k):
        d = np.ldexp(c, int(ki)).astype(c.dtype)
        assert np.isfinite(d).all() and np.array_equal(np.ldexp(d.astype(np.float64), -int(ki)), c.astype(np.float64)), 'the factor was not exact'
        out.append(d)
    return out


def plain_chain_float32(cores, l, X):
    """f (L, b) the way the unscaled device chain forms it: every product rounded to float32, no renormalisation.  A NumPy
    transcription, site by site: P from the left, Q from the right, the label site last."""
    f32 = np.float32
    b = X.shape[0]
    X = X.astype(f32)
    cores = [c.astype(f32) for c in cores]
    with np.errstate(over='ignore', under='ignore', invalid='ignore'):
        P = np.ones((b, 1), dtype=f32)
        for i in range(l):
            P = np.einsum('ba,bd,adc->bc', P, X[:, i], cores[i]).astype(f32)
        Q = np.ones((b, 1), dtype=f32)
        for i in range(len(cores) - 1, l, -1):
            Q = np.einsum('adc,bd,bc->ba', cores[i], X[:, i], Q).astype(f32)
        return np.einsum('ba,bd,adcl,bc->lb', P, X[:, l], cores[l], Q).astype(f32)
