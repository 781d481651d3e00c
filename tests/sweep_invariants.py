"""Step-level views of a whole sweep that need no per-step capture on the device (test helper, not a conftest).

tensor_svd splits sqrt(S) onto both factors (Network_class.py:912-915, oracle/mps_oracle.py `tensor_svd`), and the
device does the same, so the core that step k leaves BEHIND (the right sweep's site p, the left sweep's site p + 1) holds
U * sqrt(S) or sqrt(S) * Vh of that step's split, and no later step of the same sweep rewrites it.  Its Gram matrix over
the two outer indices is therefore diag(S[:m]):

    right sweep, core (ml, D, m) at site p:       einsum('adk,adj->kj', A, A) = diag(S_k[:m])
    left sweep,  core (m, D, mr) at site p + 1:   einsum('kdc,jdc->kj', A, A) = diag(S_k[:m])

After one launch that runs a whole sweep, `Context.get_cores()` thus gives every step's kept singular values (the
diagonal) and the orthogonality of its kept singular vectors (the off-diagonal).  Both are invariant under the freedom
an SVD leaves -- a sign per singular pair and a rotation inside a cluster of equal singular values.

The behind environments (Lenv after a right sweep, Renv after a left one) are the batch side's step-level output.
Device and oracle may differ by an orthogonal gauge on their bond index, so they are compared after an orthogonal
Procrustes alignment (`env_residual`).
"""
import numpy as np

from oracle import mps_oracle as mo


def behind_site(N, k, left_dir):
    """(p, site) of step k of a sweep: B acts on (p, p + 1); `site` holds the core that step leaves behind."""
    p = N - 2 - k if left_dir else k
    return p, (p + 1 if left_dir else p)


def step_sigmas(cores, bond, left_dir):
    """Per step k (sweep order): the Gram diagonal of its behind core, and max|off-diagonal| / max(diagonal).

    Returns (diag, off): a list of N - 1 arrays of length bond[p], and an array of N - 1 floats."""
    N = len(cores)
    diag, off = [], np.zeros(N - 1)
    for k in range(N - 1):
        p, site = behind_site(N, k, left_dir)
        A = np.asarray(cores[site], dtype=np.float64)
        assert A.ndim == 3, "the behind core of step %d (site %d) carries the label" % (k, site)
        G = np.einsum('kdc,jdc->kj', A, A) if left_dir else np.einsum('adk,adj->kj', A, A)
        assert G.shape == (int(bond[p]), int(bond[p])), (k, G.shape, int(bond[p]))
        d = np.diag(G).copy()
        diag.append(d)
        off[k] = np.abs(G - np.diag(d)).max() / max(d.max(), 1e-300)
    return diag, off


def sigma_errors(diag, S):
    """Per step: max|diag_k - S_k| / S_k[0] (S_k: the reference's kept singular values, descending)."""
    assert len(diag) == len(S)
    out = np.zeros(len(S))
    for k, (d, s) in enumerate(zip(diag, S)):
        s = np.asarray(s, np.float64)
        assert d.shape == s.shape, (k, d.shape, s.shape)
        out[k] = np.abs(d - s).max() / max(s[0], 1e-300)
    return out


def env_residual(E_dev, E_ref):
    """max|E_dev . Q - E_ref| / max|E_ref| with Q the orthogonal matrix that minimises it (Procrustes); E: (b, m)."""
    A = np.asarray(E_dev, np.float64)
    B = np.asarray(E_ref, np.float64)
    assert A.shape == B.shape, (A.shape, B.shape)
    U, _, Vh = np.linalg.svd(A.T @ B)
    return np.abs(A @ (U @ Vh) - B).max() / max(np.abs(B).max(), 1e-300)


def behind_envs(cores, X, left_dir):
    """The behind environments a whole sweep leaves, contracted afresh from the cores: Lenv[0..N-3] after a right
    sweep, Renv[2..N-1] after a left one (the sites the oracle's sweep grows)."""
    N = len(cores)
    X = np.asarray(X, np.float64)
    out = {}
    if not left_dir:
        env = mo.site_matrix(np.asarray(cores[0], np.float64), X[:, 0])[:, 0]
        out[0] = env
        for i in range(1, N - 2):
            env = np.einsum('ba,bac->bc', env, mo.site_matrix(np.asarray(cores[i], np.float64), X[:, i]))
            out[i] = env
    else:
        env = mo.site_matrix(np.asarray(cores[N - 1], np.float64), X[:, N - 1])[:, :, 0]
        out[N - 1] = env
        for i in range(N - 2, 1, -1):
            env = np.einsum('bac,bc->ba', mo.site_matrix(np.asarray(cores[i], np.float64), X[:, i]), env)
            out[i] = env
    return out


def oracle_sweep(st, X, y, f, lr, weight_dec, left_dir=False, **kw):
    """`mo.sweep` recording every step.  `mo.forward(st, X)` must have run on the same X.

    Returns a dict: S (per step, the kept singular values S[:m]), accuracy, MAE (per step), f (after the sweep) and
    env (the behind environments the sweep grew, site -> (b, m) array)."""
    assert st.X is not None and st.X.shape == np.shape(X)
    y1h = mo.one_hot(y, st.L, st.dtype)
    if left_dir:
        st.Renv = {}
    else:
        st.Lenv = {}
    S, acc, mae = [], [], []
    for _ in range(st.N - 1):
        rec = {}
        f = mo.sweep_step(st, f, y1h, lr, weight_dec, left_dir=left_dir, record=rec, **kw)
        S.append(rec['S'][:rec['m']].copy())
        acc.append(rec['accuracy'])
        mae.append(rec['MAE'])
    env = dict(st.Renv if left_dir else st.Lenv)
    return dict(S=S, accuracy=np.array(acc), MAE=np.array(mae), f=f, env=env)
