"""The tables of the context life-cycle tests (tests/context_lifecycle_cases.py) without a GPU: every mutator x call pair has a verdict,
every 'carried' pair cites a line, every 'refused' pair names its remedy and the words of its refusal; the one factor the tables hold,
computed on the float64 oracle; the host side of the same sequences under AddressSanitizer + UBSan as a stand-alone program
(csrc/Makefile target `san-lifecycle`)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p_ in (ROOT, HERE):
    if p_ not in sys.path:
        sys.path.insert(0, p_)

import context_lifecycle_cases as lc                               # noqa: E402
from nll_reference import round_up_one_digit                       # noqa: E402
from oracle import mps_oracle as mo                                # noqa: E402

CSRC = os.path.join(ROOT, 'tensornetworkforml_amd', 'csrc')


def test_every_pair_has_a_verdict():
    assert len(lc.MUTATORS) == 19 and len(lc.READERS) == 19 and len(lc.CONSUMERS) == 4
    for shape in lc.SHAPES:
        assert set(lc.LEFT_OUT[shape]) <= set(lc.CALLS)
    host = re.compile(r'(?:tnml_api|api_\w+)\.hip')                  # the host files: the call families are split off one by one
    files = {f: open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC)) if host.fullmatch(f)}
    assert set(files) == {'tnml_api.hip', 'api_dataset.hip', 'api_mps.hip'}, sorted(files)
    api = '\n'.join(files.values())                                 # a refusal may come from any call family
    for m in lc.MUTATORS:
        assert callable(lc.MUTATORS[m][0]) and lc.changes(m) in ('model', 'batch', 'labels', 'switch')
        for c in lc.CALLS:
            kind, remedy, cite = lc.verdict(m, c, 3)                # (D = 3: both sweeps of the carried table are complete)
            assert kind in ('equal', 'refused', 'carried'), (m, c)
            if kind == 'refused':
                assert remedy in ('forward', 'optim_reset') and c in lc.REFUSAL_WORDS, (m, c)
                assert lc.REFUSAL_WORDS[c].split('%s')[0] in api, (c, 'the words of the refusal are in no host file')
            if kind == 'carried':
                assert cite and re.search(host.pattern + r', \w+', cite[0]) and cite[1], (m, c)
            assert isinstance(lc.sensitive(m, c), bool)
    for (m, c), cite in lc.CARRIED.items():
        assert m in lc.MUTATORS and c in lc.CALLS
        cited = re.findall('(' + host.pattern + r'), (\w+)', cite[0])
        assert cited, (m, c)
        for name, fn in cited:                                      # every citation, in the file it names
            assert name in files, (m, c, 'the cited file does not exist')
            assert re.search(r'\b%s\(' % fn, files[name]), (m, c, 'the cited function is not in ' + name)


def test_what_the_tables_say_about_known_pairs():
    assert lc.verdict('scale_cores', 'update_B') == ('refused', 'forward', None)
    assert lc.verdict('sweep_right', 'resident_metrics')[0] == 'equal'          # a sweep leaves its f
    assert lc.verdict('sweep_right', 'update_B') == ('refused', 'forward', None)    # the step turns round: that stack was never built
    assert lc.verdict('segment', 'update_B')[0] == lc.verdict('sweep_reference', 'update_B', 2)[0] == 'equal'   # continues behind it
    assert lc.verdict('sweep_reference', 'update_B', 3)[0] == 'refused'
    assert lc.verdict('set_labels', 'update_B')[0] == lc.verdict('chain_scaling_on', 'resident_metrics')[0] == 'equal'
    assert all(lc.verdict(m, r)[0] == 'refused' for m in lc.MUTATORS if lc.changes(m) == 'batch' for r in lc.AFTER_FORWARD)
    assert lc.verdict('axpby', 'gd_step') == ('refused', 'optim_reset', None)
    assert lc.verdict('set_cores', 'gd_step')[0] == 'equal'                      # same bonds, same l_pos: the binding holds
    assert lc.sensitive('set_input_70', 'forward') and not lc.sensitive('set_input_70', 'sample')
    assert not lc.sensitive('set_input_70', 'inner') and lc.sensitive('set_labels', 'sweep')
    assert all(lc.sensitive(m, r) for m in lc.MUTATORS if lc.changes(m) == 'model' and m not in ('scale_cores', 'orthogonalize')
               for r in lc.CALLS)


def test_the_shapes_are_the_ones_the_tables_describe():
    for shape in lc.SHAPES:
        pr = lc.problem(shape)
        assert [c.shape[2] for c in pr['cores'][:-1]] == list(lc.BONDS) and pr['cores'][0].shape == (1, pr['D'], 2, lc.L)
        assert sorted(pr['batches']) == [5, 37, 70] and pr['pixels'].shape == (96, 8) and pr['phi'].shape == (8, pr['D'])
        assert all(b % 16 for b in lc.SIZES)
        cap = max(lc.M, pr['D'] * min(lc.L, lc.M))
        assert max(a + b for a, b in zip(lc.BONDS, lc.ADD_BONDS)) == 8 <= cap and max(lc.OTHER_BONDS) <= cap
    # the reference rule collapses the bonds, and at D = 2, three labels, its last step is the reference's own ValueError
    assert lc.reference_steps(2) == lc.N - 2 and lc.reference_steps(3) == lc.N - 1


def test_the_carried_factor_on_the_oracle():
    """tnml_l2_term behind a complete sweep reads the norm environments the sweep's steps formed one from the other
    (Nh_new = Cb^T (Nh x 1_d) Cb, two products a site); a fresh context contracts them from the cores.  Both routes are correct
    float64 sums of the same terms.  On the oracle: the state a right sweep leaves on shape A (cores rounded to float32, as the device
    hands them on), CARRIED_FACTOR_CASES merged tensors, each route in float64 against the same expression in long double; the
    factor is the largest ratio of the two errors, either way, rounded up to one digit."""
    assert np.finfo(np.longdouble).eps < 2e-19
    pr = lc.problem('A')
    assert lc.CARRIED_FACTOR_SEED == lc.SEED
    X, y = pr['batches'][37]
    _, st = lc.oracle_sweep_from(pr, pr['cores'], 0, X.astype(np.float64), y)
    assert st.l_pos == lc.N - 1
    cores = [c.astype(np.float32) for c in st.cores]
    shape = (st.bond[lc.N - 3], pr['D'], pr['D'], 1, lc.L)
    worst = 0.0
    for k in range(lc.CARRIED_FACTOR_CASES):
        B = np.random.default_rng(lc.CARRIED_FACTOR_SEED + k).random(shape).astype(np.float32)
        ref = lc.l2_oracle(cores, st.l_pos, B, lc.HP[1])
        e = {route: lc.l2_error(lc.l2_oracle(cores, st.l_pos, B, lc.HP[1], np.float64, route), ref) for route in ('rebuilt', 'inherited')}
        assert e['rebuilt'] > 0 and e['inherited'] > 0
        worst = max(worst, e['rebuilt'] / e['inherited'], e['inherited'] / e['rebuilt'])
        if k == 0:                                                   # the 'rebuilt' route is the oracle's own, bit for bit
            s64 = mo.MPSState(lc.N, pr['D'], lc.L, lc.M, [np.asarray(c, np.float64) for c in cores], st.l_pos)
            loss, grad = mo.compute_L2_reg(s64, B.astype(np.float64), lc.N - 2, float(np.float32(lc.HP[1])))
            mine = lc.l2_oracle(cores, st.l_pos, B, lc.HP[1], np.float64, 'rebuilt')
            assert loss == mine[0] and np.array_equal(grad, mine[1])
    print('largest ratio of the two routes\' errors over %d merged tensors: %.2f' % (lc.CARRIED_FACTOR_CASES, worst))
    assert lc.CARRIED_FACTOR == round_up_one_digit(worst)


def test_which_sweeps_are_complete():
    assert lc.verdict('sweep_right', 'l2_term', 2)[0] == lc.verdict('sweep_right', 'l2_term', 3)[0] == 'carried'
    assert lc.verdict('sweep_reference', 'l2_term', 3)[0] == 'carried'       # D = 3: the reference's rule reaches the end of the chain
    assert lc.verdict('sweep_reference', 'l2_term', 2)[0] == 'equal'         # D = 2: it stops inside, the stack behind is rebuilt
    assert lc.verdict('segment', 'l2_term', 2)[0] == lc.verdict('segment', 'l2_term', 3)[0] == 'equal'
    assert set(c for _, c in lc.CARRIED) == {'l2_term'}


def test_lifecycle_host_side_under_sanitizers():
    """warm-up -> mutator -> every call on the stand-in runtime, shapes A, B, C and C3 / C5 at true size: every launch's pointers lie
    inside live allocations of sufficient size, nothing leaks (csrc/san/plan_lifecycle_main.cpp)"""
    import shutil
    if shutil.which('g++') is None or not os.path.exists('/opt/rocm/bin/hipcc'):
        pytest.skip('no g++ / hipcc')
    r = subprocess.run(['make', '-C', CSRC, '-j4', 'san-lifecycle'], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert 'plan_lifecycle: OK' in r.stdout, r.stdout[-3000:]
    for name in ('shape A: N 8 D 2', 'shape B: N 8 D 3', 'shape C: N 8 D 2', 'shape C3: N 784 D 2 L 2 M 20', 'shape C5: N 784 D 2 L 10 M 50',
                 ' 0 live allocations'):
        assert name in r.stdout, name
