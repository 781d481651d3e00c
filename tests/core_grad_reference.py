"""Core gradients of an MPS in NumPy (test infrastructure): the formulas of csrc/kernels_coregrad.hip
transcribed with einsum for a whole batch at a time, in the dtype of its arguments (float64 in the tests).  Imported by
tests/test_core_grad_host.py and tests/test_core_grad_gpu.py.

With P_i[s][a] the contraction of sites 0 .. i-1 and Q_i[s][c] that of sites i+1 .. N-1 of sample s (P_0 = Q_{N-1} = 1; the chain
that has passed the label site l carries cot[:, s]):
    G_i[a][d][c]     = sum_s P_i[s][a] x_i[s][d] Q_i[s][c]                    i != l
    G_l[a][d][c][l'] = sum_s cot[l'][s] P_l[s][a] x_l[s][d] Q_l[s][c]
    cf[s]            = sum_l' cot[l'][s] f[l'][s]
G_i is the derivative of sum_s cf[s] with respect to A_i.
"""
import numpy as np


def core_grad_reference(cores, l, X, cot):
    """(G, cf): G a list of N arrays shaped like the cores (ml, D, mr[, L]), cf (b,), for the label on site l, X (b, N, D) and
    cot (L, b)."""
    N = len(cores)
    b = X.shape[0]
    dt = np.result_type(X.dtype, cot.dtype, *[c.dtype for c in cores])
    P = [np.ones((b, 1), dtype=dt)]
    for i in range(N - 1):
        if i == l:
            P.append(np.einsum('ba,bd,lb,adcl->bc', P[i], X[:, i], cot, cores[i]))
        else:
            P.append(np.einsum('ba,bd,adc->bc', P[i], X[:, i], cores[i]))
    Q = [None] * N
    Q[N - 1] = np.ones((b, 1), dtype=dt)
    for i in range(N - 1, 0, -1):
        if i == l:
            Q[i - 1] = np.einsum('adcl,bd,bc,lb->ba', cores[i], X[:, i], Q[i], cot)
        else:
            Q[i - 1] = np.einsum('adc,bd,bc->ba', cores[i], X[:, i], Q[i])
    G = []
    for i in range(N):
        if i == l:
            G.append(np.einsum('lb,ba,bd,bc->adcl', cot, P[i], X[:, i], Q[i]))
        else:
            G.append(np.einsum('ba,bd,bc->adc', P[i], X[:, i], Q[i]))
    if l == 0:
        cf = np.einsum('adcl,bd,bc,lb->b', cores[0], X[:, 0], Q[0], cot)
    else:
        cf = np.einsum('adc,bd,bc->b', cores[0], X[:, 0], Q[0])
    return G, cf
