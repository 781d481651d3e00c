"""Input gradients of an MPS in NumPy (test infrastructure): the two passes of csrc/kernels_inputgrad.hip
transcribed for a whole batch at a time, in the dtype of its arguments (float64 in the tests), and the analytic derivative of the
pixel feature map.  Imported by tests/test_input_grad_host.py and tests/test_input_grad_gpu.py.

f is linear in every x[s][i][:] separately.  With P_i[a] the contraction of sites 0 .. i-1 and Q_i[c] that of sites i+1 .. N-1
(the label axis contracted with cot[:, s] at the label site l; P_0 = Q_{N-1} = 1):
    pass A, i = 0 .. N-2:   P_{i+1}[c] = sum_{a,d} P_i[a] x_i[d] A_i[a][d][c]
    pass B, i = N-1 .. 0:   T[a][d]    = sum_c A_i[a][d][c] Q_i[c]
                            g[i][d]    = sum_a P_i[a] T[a][d]
                            Q_{i-1}[a] = sum_d x_i[d] T[a][d]
    after i = 0:            cf = Q_{-1} = sum_l' cot[l'] f[l']
"""
import math

import numpy as np


def scaled_cores(N, D, L, bond, l_pos, rng):
    """U[0,1) cores in the canonical layout (ml, D, mr[, L]), label on site l_pos, each divided by D sqrt(ml mr) / 4 so that
    environments of inputs in [0, 1) stay O(1) along the chain (the expected growth per site, sqrt(ml / mr), telescopes)."""
    cores = []
    for i in range(N):
        ml = 1 if i == 0 else int(bond[i - 1])
        mr = 1 if i == N - 1 else int(bond[i])
        cores.append(rng.random((ml, D, mr, L) if i == l_pos else (ml, D, mr)) / (0.25 * D * math.sqrt(ml * mr)))
    return cores


def ragged_bonds(N, cap, rng):
    """N-1 bonds in [1, cap] with cap itself among them."""
    bond = rng.integers(1, cap + 1, N - 1)
    bond[rng.integers(0, N - 1)] = cap
    return [int(v) for v in bond]


def input_grad_reference(cores, l, X, cot):
    """(g (b, N, D), cf (b,)) for cores (ml, D, mr[, L]) with the label on site l, X (b, N, D) and cot (L, b)."""
    N = len(cores)
    b = X.shape[0]
    dt = np.result_type(X.dtype, cot.dtype, *[c.dtype for c in cores])
    P = [np.ones((b, 1), dtype=dt)]
    for i in range(N - 1):
        if i == l:
            P.append(np.einsum('ba,bd,lb,adcl->bc', P[i], X[:, i], cot, cores[i]))
        else:
            P.append(np.einsum('ba,bd,adc->bc', P[i], X[:, i], cores[i]))
    g = np.empty(X.shape, dtype=dt)
    Q = np.ones((b, 1), dtype=dt)
    for i in range(N - 1, -1, -1):
        if i == l:
            T = np.einsum('adcl,bc,lb->bad', cores[i], Q, cot)
        else:
            T = np.einsum('adc,bc->bad', cores[i], Q)
        g[:, i, :] = np.einsum('ba,bad->bd', P[i], T)
        Q = np.einsum('bd,bad->ba', X[:, i], T)
    return g, Q[:, 0].copy()


def dpsi(p, D):
    """d psi_k / d p of data_generator.psi(p, D) on a new last axis:
    (pi / 2) sqrt(C(D-1, k)) [(D-1-k) sin^(D-2-k) cos^(k+1) - k sin^(D-k) cos^(k-1)]; a term whose factor is 0 is dropped."""
    p = np.asarray(p, dtype=np.float64)
    sn, cs = np.sin(np.pi * p / 2), np.cos(np.pi * p / 2)
    comps = []
    for k in range(D):
        t = np.zeros_like(p)
        if D - 1 - k > 0:
            t = t + (D - 1 - k) * sn ** (D - 2 - k) * cs ** (k + 1)
        if k > 0:
            t = t - k * sn ** (D - k) * cs ** (k - 1)
        comps.append(np.pi / 2 * math.sqrt(float(math.comb(D - 1, k))) * t)
    return np.stack(comps, axis=-1)
