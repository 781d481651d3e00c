"""The NumPy statement of the likelihood gradient from incomplete data (tests/nll_masked_reference.py) against
central differences of a dense enumeration, against its own identities and against tests/nll_reference.py on the full mask; the
long-double differences and the emulation figures that the bounds of tests/test_nll_masked_gpu.py are built from; and what of the
Python wrappers needs no device."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p_ in (ROOT, HERE):
    if p_ not in sys.path:
        sys.path.insert(0, p_)

import nll_masked_reference as M                                   # noqa: E402
import nll_reference as N                                          # noqa: E402
import nll_step_reference as SR                                    # noqa: E402
import sample_masked_reference as MR                               # noqa: E402


@pytest.mark.parametrize('name', M.DENSE)
def test_statement_against_central_differences(name):
    """N = 4, K = 3, D = 2, L = 2, all 16 masks, classes -1 / 0 / 1: -G is the derivative of the value that the dense enumeration
    gives.  Central differences at h and 2 h, h = 1e-4, extrapolated: (4 cd(h) - cd(2 h)) / 3 has no h^2 term (which alone is 1e-5
    here: the third derivative over 6 is about 1e3) and leaves the h^4 term and the rounding 2^-52 |v| / h = 1e-11; the bound of
    3e-9 is what plain central differences at their best step reach in float64 (a quarter of the digits are lost to h)."""
    c = M.case(name)
    r = c.ref
    assert abs(float(r['value']) - M.dense_value(c.cores, c.l, c.phi, c.w, c.classes, c.mask, c.known)) <= 1e-13
    h, worst = 1e-4, 0.0
    for i in range(c.N):
        cd = np.zeros((2,) + c.cores[i].shape)
        for e in np.ndindex(*c.cores[i].shape):
            for k, step in enumerate((h, 2 * h)):
                v = []
                for sgn in (1.0, -1.0):
                    cores = [x.copy() for x in c.cores]
                    cores[i][e] += sgn * step
                    v.append(M.dense_value(cores, c.l, c.phi, c.w, c.classes, c.mask, c.known))
                cd[(k,) + e] = (v[0] - v[1]) / (2 * step)
        worst = max(worst, float(np.abs((4.0 * cd[0] - cd[1]) / 3.0 + r['G'][i]).max()))
    print('%s: central differences %.2e' % (name, worst))
    assert worst <= 3e-9


@pytest.mark.parametrize('name', M.ALL)
def test_identities_and_long_double(name):
    """sum(G_i A_i) = 0 at every site; the value and logp are those of sample_masked_reference's environments; the reference alone
    leaves d_LD <= 1e-12 max|G| on every shared case"""
    c = M.case(name)
    r = c.ref
    gm = max(M.gmax(r['G']), M.gmax(r['Gz']))
    sums = np.abs(M.site_sums(r['G'], c.cores)).max()
    dz = np.abs(M.site_sums(r['Gz'], c.cores) - 2.0).max()
    print('%s: sum(G A) %.2e  sum(Gz A) - 2 %.2e  d_LD %.2e of max|G| %.2e  value %.2e  logp %.2e' % (name, sums, dz, c.d_G.max(), gm, c.d_v, c.d_logp))
    assert sums <= 1e-13 and dz <= 1e-13
    assert c.d_G.max() <= 1e-12 * gm
    assert c.d_v <= 1e-12 * max(1.0, abs(float(r['value']))) and c.d_logp <= 1e-12 * max(1.0, float(np.abs(r['logp']).max()))
    assert abs(float(r['value']) - M.masked_value(c.cores, c.l, c.phi, c.w, c.classes, c.mask, c.known)) <= 1e-12 * max(1.0, abs(float(r['value'])))
    _, _, logp, _ = MR.masked_walk(c.cores, c.l, c.phi, c.w, c.classes, None, c.mask, c.known, draw=False)
    clw = MR.class_log_weights(c.cores, c.l, c.phi, c.w)
    joint = logp[:, 1] + np.where(c.classes >= 0, clw[np.maximum(c.classes, 0)], 0.0)
    assert float(np.abs(joint - r['logp']).max()) <= 1e-11 * max(1.0, float(np.abs(joint).max()))


@pytest.mark.parametrize('name,labelled', [('full_mask', True), ('full_mask_marginal', False)])
def test_full_mask_is_nll_gradient(name, labelled):
    c = M.case(name)
    X = c.phi[c.known]
    Gn, vn, lz = N.nll_gradient(c.cores, c.l, X, c.classes if labelled else None, N.gram(c.phi, c.w))
    vn -= float(np.log(c.w)[c.known].sum(axis=1).mean())          # (the value here carries the w_k of the known sites)
    d = N.deviation(c.ref['G'], Gn)
    print('%s: against nll_reference.nll_gradient %.2e, value %.2e, log Z %.2e' % (name, d, abs(vn - float(c.ref['value'])), abs(lz - float(c.ref['logz']))))
    assert d <= 1e-12 and abs(vn - float(c.ref['value'])) <= 1e-12 * abs(vn) and abs(lz - float(c.ref['logz'])) <= 1e-12


def test_empty_masks():
    c = M.case('empty')
    assert float(c.ref['value']) == 0.0 and M.gmax(c.ref['G']) <= 1e-14 * M.gmax(c.ref['Gz'])


def test_ten_steps_of_the_statement_descend():
    c = M.case('descent')
    ref = SR.NllStepReference(c.cores, c.l, None, kind='sgd', momentum=0.0, clip=False, renorm=True)
    vals = []
    for _ in range(10):
        r = M.masked_gradient(ref.cores, c.l, c.phi, c.w, c.classes, c.mask, c.known)
        vals.append(float(r['value']))
        ref.apply(r['G'], M.DESCENT_LR, 0.0)
    vals.append(float(M.masked_gradient(ref.cores, c.l, c.phi, c.w, c.classes, c.mask, c.known)['value']))
    print(' '.join('%.4f' % v for v in vals))
    assert all(b < a for a, b in zip(vals, vals[1:]))


@pytest.mark.parametrize('name', M.STEP_CASES)
def test_step_emulation_figures(name):
    """the committed figures behind the step bounds of the GPU test are what the code gives (within a quarter: einsum's summation
    order follows the host's vector width), and the step moves the cores by far more than its bound"""
    c = M.case(name)
    for opt in M.STEP_OPTIMS:
        fig, want = M.step_emulation_figure(c, opt), M.STEP_EMULATION[name][opt]
        move = SR.moved(M.step_reference(c, opt), c.cores)
        print('%s %s: %.3e (committed %.3e), move %.2e, bound %.2e' % (name, opt, fig, want, move, M.step_bound(c, opt).max()))
        assert abs(fig - want) <= 0.25 * want
        assert M.step_bound(c, opt).max() <= 1e-3 * move


def test_shared_cases_cover_what_the_kernel_can_get_wrong():
    """bonds of 1 and of the cap in every ragged chain; n on either side of a tile; a mask of every density; both kinds of class"""
    for name in M.RAGGED:
        c = M.case(name)
        assert min(c.bond) == 1 and max(c.bond) == c.mb
        if c.n >= 4:
            assert not c.mask[0].any() and c.mask[3].all() and (c.classes < 0).any() and (c.classes >= 0).any()
    assert sorted({M.case(k).n for k in M.RAGGED}) == [1, 17, 70]
    for (D, L, cap) in M.ROWS:
        assert sorted(M.case(k).n for k in M.RAGGED if '_D%d_' % D in k) == [1, 17, 70]


def test_python_wrappers_without_a_device():
    from tensornetworkforml_amd import _hip
    assert 'tnml_nll_masked_grad' in _hip.SYMBOLS and 'tnml_nll_masked_step' in _hip.SYMBOLS
    hdr = open(os.path.join(ROOT, 'include', 'tnml.h')).read()
    assert 'int tnml_nll_masked_grad(' in hdr and 'int tnml_nll_masked_step(' in hdr
    import tensornetworkforml_amd as pkg
    for m in ('nll_gradient_masked', 'nll_masked', 'nll_step_masked'):
        assert callable(getattr(pkg.Network_class.Network, m))


def test_nll_masked_host_side_under_sanitizers():
    """csrc/Makefile target `san-nll-masked`: tnml_nll_masked_grad / tnml_nll_masked_step of nll_masked_host.hip and the launch wrappers
    of kernels_nll_masked.hip, built --cuda-host-only with -fsanitize=address,undefined, against the stand-in runtime of
    csrc/san/hip_stub.cpp (csrc/san/plan_nll_masked_main.cpp, a stand-alone program): C3 and C5 at true size under the default
    budget and under one tile's, a ragged 17-site chain at D = 2, 3 and 8 at every label position, every refusal (none launches),
    the bond limit taken and refused, every allocation of the new group failing in turn, the row weights and the tiles of every call."""
    import shutil
    import subprocess
    if shutil.which('g++') is None or not os.path.exists('/opt/rocm/bin/hipcc'):
        pytest.skip('no g++ / hipcc')
    csrc = os.path.join(ROOT, 'tensornetworkforml_amd', 'csrc')
    out = subprocess.run(['make', '-C', csrc, '-j4', 'san-nll-masked'], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert 'masked likelihood gradient host planning under ASan + UBSan: ok' in out.stdout
    for name in ('c3 bond 20 L 2, label on 0, tiles of 8', 'c3 inner label', 'c5 bond 50 L 10, label on 783, tiles of 2', 'c5 inner label',
                 'ragged N 17 D 2', 'ragged N 17 D 3', 'ragged N 17 D 8', 'refusals: ok', 'its group is new        7 failed in turn',
                 'the optimiser state is new  2 failed in turn'):
        assert name in out.stdout, name
    assert '0 live allocations' in out.stdout
