"""tnml_sample and tnml_sample_masked against their own recorded results, bit for bit (tests/golden/sample_bits.npz, written by
tools/record_sample_bits.py on the build of the commit the file names).  The two calls share their device helpers
(csrc/sample_device.h) and their host front; a change there that is meant to leave the arithmetic alone must leave every integer and
every float64 bit pattern of these cases alone.  No tolerance: levels and labels are compared as integers, logp and the class
log-weights as uint64.  The cases are the smallest on which every shared helper runs every branch -- ragged 17-site chains at
K = 7 (lanes with fewer than four levels), 256 (all 64 lanes) and 2 (63 lanes empty) with the label at both ends and inside, 40 samples
(padding rows), mixed classes, prefixes, shared and per-sample masks, hashed and explicit uniforms, several chunks, and four sites
at the uniform bonds 64 and 32 (masked tiles of one and of four rows)."""
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p_ in (ROOT, HERE):
    if p_ not in sys.path:
        sys.path.insert(0, p_)

from tensornetworkforml_amd import _hip                            # noqa: E402

pytestmark = pytest.mark.gpu

GOLD = np.load(os.path.join(HERE, 'golden', 'sample_bits.npz'))
CHAINS = json.loads(str(GOLD['chains']))
CALLS = json.loads(str(GOLD['calls']))


def context_M(D, cap, L):
    return next(m for m in range(1, cap + 1) if max(m, D * min(L, m)) >= cap)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def opt(key):
    return GOLD[key] if key in GOLD.files else None


def test_the_fixture_names_its_commit_and_covers_every_chain():
    assert len(str(GOLD['commit'])) == 40
    assert len(CHAINS) == 11 and len(CALLS) == 62
    assert {c['chain'] for c in CALLS} == {ch['name'] for ch in CHAINS}
    assert {c['kind'] for c in CALLS} == {'sample', 'masked'}


@pytest.mark.parametrize('chain', CHAINS, ids=lambda ch: ch['name'])
def test_every_recorded_call_comes_back_bit_for_bit(chain):
    name, N, D, L, n = chain['name'], chain['N'], chain['D'], chain['L'], chain['n']
    cores = [GOLD['%s/core%d' % (name, i)] for i in range(N)]
    phi, w, classes = GOLD[name + '/phi'], GOLD[name + '/w'], GOLD[name + '/classes']
    ctx = _hip.Context(N, D, L, context_M(D, chain['capacity'], L), 8)
    ctx.set_any_position(True)
    ctx.set_cores(cores, chain['l_pos'])
    calls = [c for c in CALLS if c['chain'] == name]
    assert len(calls) >= 4
    for c in calls:
        cid, u = c['id'], opt(c['id'] + '/u')
        if c['kind'] == 'sample':
            lev, lab, lp = ctx.sample(n, phi, w, classes, opt(cid + '/given'), u, c['seed'])
            clw = None
        else:
            ctx.set_sample_stack_bytes(c.get('stack_bytes', 1 << 30))
            res = ctx.sample_masked(n, phi, w, GOLD[cid + '/mask'], opt(cid + '/known'), classes, u, c['seed'], c['draw'], c['class_logw'])
            ctx.set_sample_stack_bytes(1 << 30)
            lev, lab, lp = res[:3]
            clw = res[3] if c['class_logw'] else None
        if c['kind'] == 'sample' or c['draw']:
            assert lev.dtype == np.int32 and np.array_equal(lev, GOLD[cid + '/out_levels']), cid
        else:
            assert lev is None, cid
        assert lab.dtype == np.int32 and np.array_equal(lab, GOLD[cid + '/out_labels']), cid
        assert same_bits(lp, GOLD[cid + '/out_logp']), cid
        if clw is not None:
            assert same_bits(clw, GOLD[cid + '/out_class_logw']), cid
        else:
            assert cid + '/out_class_logw' not in GOLD.files, cid
    ctx.close()
