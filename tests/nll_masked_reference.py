"""Likelihood gradients from incomplete data in float64 NumPy, with a long-double switch (test infrastructure):
the statement of tnml_nll_masked_grad in include/tnml.h, on top of tests/sample_masked_reference.py and tests/sample_reference.py.
Also the shared cases of tests/test_nll_masked_host.py (which checks the conditions on them with this reference alone) and
tests/test_nll_masked_gpu.py (which runs them on the device), and the tables the bounds of the GPU tests are read from.

Cores are arrays (ml, D, mr[, L]) with the label on site l.  Sample s has a mask g_s (N,), levels k_s read where it is set, and a
class slot q_s in {-1, 0 .. L-1} (-1: the label unknown and summed).  With S_{s,i} = w_k phi_k phi_k^T on a known site and S on a
free one, R_{s,i} / Lf_{s,i} the environments from the right / left (all label slices for q_s = -1, slice q_s alone otherwise):

    E_s   = log R_{s,0} (with the exponents of the rescales),   log Z = E of the empty mask with class slot -1
    value = -mean_s (E_s - log Z)
    g_s,i[a,d,c(,l')] = 2 / n_s,i  sum Lf_s,i[a,a'] S_s,i[d,d'] A_i[a',d',c'(,l')] R_s,i+1[c,c'],   n_s,i = <that contraction, A_i>
    G = (1/n) sum_s g_s - g_empty          (the DESCENT direction: A += lr G lowers the value)

Known levels and labels of every shared case are drawn from the case's own chain by sample_reference.walk, as section 24 does.
"""
import functools
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p_ in (ROOT, HERE):
    if p_ not in sys.path:
        sys.path.insert(0, p_)

import nll_reference as nref                                                                 # noqa: E402
import nll_step_reference as sref                                                            # noqa: E402
import sample_masked_reference as MR                                                         # noqa: E402
import sample_reference as SR                                                                # noqa: E402


# ---------------------------------------------------------------------------------------------------------------
# the statement
# ---------------------------------------------------------------------------------------------------------------
def _rescaled(E):
    """(E 2^-e, e) with the largest magnitude in [0.5, 1); (E, 0) for a zero matrix"""
    m = np.abs(E).max()
    if not m > 0:
        return E, 0
    _, e = np.frexp(m)
    return np.ldexp(E, -int(e)), int(e)


def sample_terms(cores, l, phi, w, Sg, q, mask, known):
    """(g list in the cores' shapes, E) of one row: class slot q, mask (N,) bool, known (N,) levels.  Everything in the dtype of the
    cores (float64 or long double)."""
    N = len(cores)
    dt = cores[0].dtype
    C4 = []
    for i, c in enumerate(cores):
        C4.append((c if q < 0 else c[..., q:q + 1]) if i == l else c[..., None])
    Sm = [Sg if not mask[i] else w[int(known[i])] * np.multiply.outer(phi[int(known[i])], phi[int(known[i])]) for i in range(N)]
    R = [None] * (N + 1)
    R[N] = np.ones((1, 1), dtype=dt)
    ex = 0
    for i in range(N - 1, -1, -1):
        E = np.einsum('de,adcl,cf,befl->ab', Sm[i], C4[i], R[i + 1], C4[i], optimize=True)
        R[i], e = _rescaled(E)
        ex += e
    r0 = R[0][0, 0]
    Es = (np.log(r0) + ex * np.log(dt.type(2.0))) if r0 > 0 else dt.type(-np.inf)
    g = []
    Lf = np.ones((1, 1), dtype=dt)
    for i in range(N):
        X = np.einsum('ab,de,becl,fc->adfl', Lf, Sm[i], C4[i], R[i + 1], optimize=True)
        n = (X * C4[i]).sum()
        X = (dt.type(2.0) / n) * X
        if i == l:
            full = np.zeros(cores[i].shape, dtype=dt)
            if q < 0:
                full[...] = X
            else:
                full[..., q] = X[..., 0]
            g.append(full)
        else:
            g.append(X[..., 0])
        Lf, _ = _rescaled(np.einsum('ab,de,adcl,befl->cf', Lf, Sm[i], C4[i], C4[i], optimize=True))
    return g, Es


def masked_gradient(cores, l, phi, w, classes, mask, known, dtype=np.float64):
    """-> dict(G, Gd, Gz: lists in the cores' shapes, value, logz, logp (n,)), all in `dtype` (np.float64 or np.longdouble)"""
    cores = [np.asarray(c, dtype=dtype) for c in cores]
    phi, w = np.asarray(phi, dtype=dtype), np.asarray(w, dtype=dtype)
    classes = np.asarray(classes, dtype=np.int64)
    n, N = len(classes), len(cores)
    mask = np.broadcast_to(np.asarray(mask, dtype=bool), (n, N))
    known = np.zeros((n, N), dtype=np.int64) if known is None else np.asarray(known, dtype=np.int64)
    Sg = np.einsum('k,kd,ke->de', w, phi, phi)
    none = np.zeros(N, dtype=bool)
    Gz, logz = sample_terms(cores, l, phi, w, Sg, -1, none, none.astype(int))
    Gd = [np.zeros_like(c) for c in cores]
    logp = np.zeros(n, dtype=dtype)
    for s in range(n):
        g, Es = sample_terms(cores, l, phi, w, Sg, int(classes[s]), mask[s], known[s])
        for a, b in zip(Gd, g):
            a += b
        logp[s] = Es - logz
    Gd = [a / dtype(n) for a in Gd]
    return dict(G=[a - b for a, b in zip(Gd, Gz)], Gd=Gd, Gz=Gz, value=-logp.sum() / dtype(n), logz=logz, logp=logp)


def masked_value(cores, l, phi, w, classes, mask, known):
    """the value alone, float64 (sample_masked_reference's environments)"""
    cores = [np.asarray(c, dtype=np.float64) for c in cores]
    classes = np.asarray(classes, dtype=np.int64)
    n, N = len(classes), len(cores)
    mask = np.broadcast_to(np.asarray(mask, dtype=bool), (n, N))
    known = np.zeros((n, N), dtype=np.int64) if known is None else np.asarray(known, dtype=np.int64)
    Sg = SR.gram(phi, w)
    logz = MR.normalisers(cores, l, phi, w, [-1])[-1]
    return -float(np.mean([MR.environments(cores, l, phi, w, Sg, int(classes[s]), mask[s], known[s])[1] - logz for s in range(n)]))


def dense_value(cores, l, phi, w, classes, mask, known):
    """the value by dense enumeration (N <= 6): -mean_s log p(known levels [, class]) from sample_reference.dense_joint"""
    P = SR.dense_joint(cores, l, phi, w)
    tot = 0.0
    for s in range(len(classes)):
        q = int(classes[s])
        p = MR.dense_marginal(P, mask[s], known[s], q)
        if q >= 0:
            p = p * P[..., q].sum()                              # dense_marginal conditions on the class: back to the joint
        tot += math.log(p)
    return -tot / len(classes)


def site_sums(G, cores):
    """sum(G_i A_i) per site"""
    return np.array([float((np.asarray(g, dtype=np.float64) * np.asarray(c, dtype=np.float64)).sum()) for g, c in zip(G, cores)])


def ld_differences(ref64, refld):
    """(d_LD per site: max|G64_i - GLD_i|, of the value, of logp): what the float64 statement itself leaves open"""
    dG = np.array([float(np.abs(a.astype(np.longdouble) - b).max()) for a, b in zip(ref64['G'], refld['G'])])
    dv = float(abs(np.longdouble(ref64['value']) - refld['value']))
    dl = float(np.abs(ref64['logp'].astype(np.longdouble) - refld['logp']).max())
    return dG, dv, dl


def gmax(G):
    return max(float(np.abs(g).max()) for g in G)


# ---------------------------------------------------------------------------------------------------------------
# shared cases
# ---------------------------------------------------------------------------------------------------------------
class Case:
    """One shared case: .cores (float32 values as float64), .l, .phi, .w, .classes (n,), .mask (n, N) bool, .known (n, N) int32, and
    the reference computed once: .ref (float64), .d_G (per site), .d_v, .d_logp (the long-double differences)."""

    def __init__(self, name, N, D, L, bond, l, K, n, seed, mask_kind='random', class_kind='mixed'):
        self.name, self.N, self.D, self.L, self.l, self.K, self.n = name, N, D, L, l, K, n
        rng = np.random.default_rng([31, N, D, L, l, K, n, seed])
        self.bond = list(bond) if not isinstance(bond, int) else nref.chain_bonds(N, bond, rng)     # (cap and a bond of 1 among them)
        self.mb = max(self.bond)
        self.cores = SR.chain(N, D, L, self.bond, l, rng)
        _, self.phi, _ = SR.grid(K, D)
        self.w = SR.weights_of(rng, K, seed % 2 == 0)
        lev, lab, _, _ = SR.walk(self.cores, l, self.phi, self.w, np.full(n, -1), rng.random((n, N + 1)))
        self.known = lev.astype(np.int32)
        self.labels = lab.astype(np.int32)
        if mask_kind == 'random':
            self.mask = MR.random_masks(rng, n, N)               # density (0, .3, .7, 1)[s % 4]
        elif mask_kind == 'full':
            self.mask = np.ones((n, N), dtype=bool)
        else:
            self.mask = np.zeros((n, N), dtype=bool)
        if class_kind == 'mixed':
            self.classes = np.where(np.arange(n) % 3 == 1, -1, self.labels).astype(np.int32)
        elif class_kind == 'labels':
            self.classes = self.labels.copy()
        else:
            self.classes = np.full(n, -1, dtype=np.int32)

    @functools.cached_property
    def ref(self):
        return masked_gradient(self.cores, self.l, self.phi, self.w, self.classes, self.mask, self.known)

    @functools.cached_property
    def _ld(self):
        return ld_differences(self.ref, masked_gradient(self.cores, self.l, self.phi, self.w, self.classes, self.mask, self.known, np.longdouble))

    d_G = property(lambda self: self._ld[0])
    d_v = property(lambda self: self._ld[1])
    d_logp = property(lambda self: self._ld[2])

    def bounds(self):
        """(per site bound of |G - G_ref64|, bound of the value and of logp) on the device:
        2^-22 max|G_i| (the one float32 rounding) + N m^2 D^2 2^-52 max|Gz_i| (section 24's float64 accumulation form) + 10 d_LD
        (section 24's margin for the summation order); N m^2 D^2 2^-52 max(1, |v|) + 10 d_LD for the value and logp"""
        acc = self.N * self.mb ** 2 * self.D ** 2 * 2.0 ** -52
        gb = np.array([2.0 ** -22 * float(np.abs(g).max()) + acc * float(np.abs(z).max()) for g, z in zip(self.ref['G'], self.ref['Gz'])])
        gb = gb + 10.0 * self.d_G
        vb = acc * max(1.0, abs(float(self.ref['value']))) + 10.0 * self.d_v
        lb = acc * max(1.0, float(np.abs(self.ref['logp']).max())) + 10.0 * self.d_logp
        return gb, vb, lb


ROWS = [(2, 2, 5), (3, 3, 7), (8, 10, 16)]       # (D, L, bond cap) of the ragged 17-site chains
BATCHES = (1, 17, 70)                            # a lone row, a second tile with padding, several tiles
K_OF = {2: 7, 3: 256, 8: 2}

_SPECS = {}


def _spec(name, *a, **k):
    _SPECS[name] = (a, k)


for ri, (D_, L_, cap_) in enumerate(ROWS):
    for li, l_ in enumerate((0, 8, 16)):
        _spec('ragged_D%d_L%d_M%d_l%d' % (D_, L_, cap_, l_), 17, D_, L_, cap_, l_, K_OF[D_], BATCHES[(ri + li) % 3], li)
_spec('bond20_N5', 5, 2, 2, [20, 20, 20, 20], 2, 256, 9, 0)                       # two 16-row chunks, the second ragged
_spec('bond50_N4', 4, 2, 10, [50, 50, 50], 1, 256, 5, 0)                         # T = 2
_spec('bond64_N4', 4, 2, 2, [2, 64, 2], 2, 7, 3, 1)                              # T = 1
for l_ in (0, 2, 3):
    _spec('dense_l%d' % l_, 4, 2, 2, [3, 3, 3], l_, 3, 48, l_)
# (rows (D, cap, L) = (2, 5, 3) and (3, 7, 3) of nll_reference.EMULATION, whose bounds the comparison with nll_gradient uses)
_spec('full_mask', 17, 2, 3, 5, 8, 256, 17, 7, mask_kind='full', class_kind='labels')
_spec('full_mask_marginal', 17, 3, 3, 7, 0, 256, 17, 8, mask_kind='full', class_kind='none')
_spec('empty', 17, 2, 2, 5, 8, 7, 17, 9, mask_kind='empty', class_kind='none')
_spec('descent', 6, 2, 2, [4] * 5, 2, 7, 20, 3)
_spec('descent_l0', 6, 2, 2, [4] * 5, 0, 7, 20, 4)
DESCENT_LR = 0.05                                # plain SGD with renorm on 'descent': ten steps lower the value (the host test asserts it)

RAGGED = [k for k in _SPECS if k.startswith('ragged')]
WIDE = ['bond20_N5', 'bond50_N4', 'bond64_N4']
DENSE = ['dense_l0', 'dense_l2', 'dense_l3']
GRAD_CASES = RAGGED + WIDE + DENSE
STEP_CASES = ['ragged_D2_L2_M5_l8', 'ragged_D3_L3_M7_l0', 'ragged_D8_L10_M16_l16']
ALL = list(_SPECS)


@functools.lru_cache(maxsize=None)
def case(name):
    a, k = _SPECS[name]
    c = Case(name, *a, **k)
    if name.startswith('dense'):                                 # all 16 masks with classes -1 / 0 / 1
        masks = MR.all_masks(4)
        c.mask = np.array([masks[s // 3] for s in range(48)])
        c.classes = np.array([s % 3 - 1 for s in range(48)], dtype=np.int32)
    return c


# ---------------------------------------------------------------------------------------------------------------
# the step: nll_step_reference's update on the reference G
# ---------------------------------------------------------------------------------------------------------------
STEP_OPTIMS = ('sgd', 'sgd_clip_mom', 'adam')
WD = sref.WD


def step_lr(c, name):
    return sref.case_lr(c.cores, c.l, None, c.ref['G'], name)


def step_reference(c, name, G=None, emulate=False, renorm=True):
    """the cores after one renormalised step of optimiser `name` on G (default: the reference's) from the case's cores"""
    ref = sref.NllStepReference(c.cores, c.l, None, renorm=renorm, emulate=emulate, **sref.OPTIMS[name])
    ref.apply(c.ref['G'] if G is None else G, step_lr(c, name), WD)
    return ref.cores


def step_emulation_figure(c, name):
    """max |A'_emulated - A'_float64| over all cores: the update in float64 on the float32-rounded G with one float32 rounding per
    store against the float64 update on the float64 G"""
    G32 = [np.asarray(g, dtype=np.float32).astype(np.float64) for g in c.ref['G']]
    return sref.moved(step_reference(c, name, G32, emulate=True), step_reference(c, name))


# The emulation's figure per step case and optimiser.  tests/test_nll_masked_host.py asserts that the code still gives these figures
# (within a quarter); the bounds of tests/test_nll_masked_gpu.py are lr times the gradient bound plus ten times the figure.
STEP_EMULATION = {
    'ragged_D2_L2_M5_l8': {'sgd': 5.903e-08, 'sgd_clip_mom': 5.903e-08, 'adam': 4.937e-08},
    'ragged_D3_L3_M7_l0': {'sgd': 5.923e-08, 'sgd_clip_mom': 5.923e-08, 'adam': 5.571e-08},
    'ragged_D8_L10_M16_l16': {'sgd': 6.441e-08, 'sgd_clip_mom': 6.441e-08, 'adam': 5.944e-08},
}


def step_bound(c, name):
    """per site: lr |G bound| + 10 times the emulation's figure"""
    return step_lr(c, name) * c.bounds()[0] + 10.0 * STEP_EMULATION[c.name][name]
