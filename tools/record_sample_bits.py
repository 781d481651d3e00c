#!/usr/bin/env python3
"""GPU: record what Context.sample and Context.sample_masked return, bit for bit -- the fixture of tests/test_sample_bits_gpu.py.

Run it on the build whose bits are to be the reference (for a change that must not move a bit: the parent commit's build), then
commit the file:

    python tools/record_sample_bits.py tests/golden/sample_bits.npz [commit]

(the commit is read from git where it is not given).

The file holds the commit it was recorded at ('commit'), the list of chains ('chains', JSON) and the list of calls ('calls', JSON).
Per chain: the cores as float32 arrays (they are built through LAPACK and BLAS on the host, whose last bits are not the same
everywhere), the grid phi and w.  Per call: classes, given or mask and known, u where the call has explicit uniforms (otherwise the
seed of the counter hash is in the list), and every output: levels, labels, logp and the class log-weights.  Only calls that succeed
are recorded: a case that ends in a refusal (a sample of zero weight, a non-finite value) gets another seed in SEED_OF below, and
that is said there.  A later, deliberate change of the samplers' numerics re-records the file with this script.
"""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import mps_algebra_reference as A                      # noqa: E402
import sample_masked_reference as M                    # noqa: E402
import sample_reference as S                           # noqa: E402
from tensornetworkforml_amd import _hip                # noqa: E402

# Ragged 17-site chains, bonds 1 to 7: K = 7 leaves lanes with fewer than four levels, K = 256 fills all 64 lanes, K = 2 leaves 63
# lanes empty; the label at both ends and inside.  n = 40 is no multiple of the tile of 16: padding rows exist.
SHAPES = [(2, 2, 7), (3, 3, 256), (8, 10, 2)]           # (D, L, K)
LABELS = (0, 8, 16)
assert S.N_DRAWS == 40
# Four sites at a uniform bond: 64 (lane < mr covers the whole wave; the fourth accumulator of the prefix sampler's environments; a
# masked tile of one row) and 32 (a masked tile of four rows)
UNIFORM_BONDS = (64, 32)
N_UNIFORM = 20
# the seed of a case's counter hash is 1000 + its number in the list of calls unless it is named here (no case needed another one)
SEED_OF = {}


def context_M(D, cap, L):
    return next(m for m in range(1, cap + 1) if max(m, D * min(L, m)) >= cap)


def chain_list():
    """name -> (cores float32, l, phi, w, classes, u, per-sample masks, known, capacity)"""
    out = {}
    for (D, L, K) in SHAPES:
        for l in LABELS:
            case = (17, D, L, l, K)
            cores, phi, w, classes, u = S.build_draw_case(case)
            mask, _, known = M.ragged_inputs(100 * D + l, case)
            out['r_D%d_L%d_K%d_l%d' % (D, L, K, l)] = (A.as32(cores), l, phi, w, classes, u, mask, known, 7)
    for mb in UNIFORM_BONDS:
        N, D, L, K, l, n = 4, 2, 2, 7, 2, N_UNIFORM
        rng = np.random.default_rng([26, mb])
        cores = S.chain(N, D, L, [mb] * (N - 1), l, rng)
        _, phi, _ = S.grid(K, D)
        w = S.weights_of(rng, K, False)
        classes = S.mixed_classes(rng, n, L)
        u = rng.random((n, N + 1))
        mask = M.random_masks(rng, n, N)
        known = rng.integers(0, K, (n, N)).astype(np.int32)
        out['u_bond%d' % mb] = (A.as32(cores), l, phi, w, classes, u, mask, known, mb)
    return out


def calls_of(name, chain):
    """the calls of one chain: dicts of kind, the inputs that are not the chain's, and the switches"""
    cores, l, phi, w, classes, u, mask, known, cap = chain
    N, n = len(cores), len(classes)
    prefix = np.arange(N) < N // 2
    if name.startswith('u_'):
        return [dict(kind='sample', given=None, u=None), dict(kind='sample', given=known[:, :2], u=u),
                dict(kind='masked', mask=mask, known=known, u=None, draw=True, class_logw=True),
                dict(kind='masked', mask=mask, known=known, u=u, draw=True, class_logw=False)]
    out = [dict(kind='sample', given=None, u=None), dict(kind='sample', given=known[:, :5], u=None),
           dict(kind='masked', mask=prefix, known=known, u=None, draw=True, class_logw=True),
           dict(kind='masked', mask=mask, known=known, u=None, draw=True, class_logw=True),
           dict(kind='masked', mask=mask, known=known, u=None, draw=False, class_logw=False)]
    if '_K7_' in name:
        out.append(dict(kind='sample', given=known[:, :5], u=u))
        out.append(dict(kind='masked', mask=mask, known=known, u=u, draw=True, class_logw=False))
    if name.endswith('_K7_l8'):
        out.append(dict(kind='masked', mask=np.zeros(N, dtype=bool), known=None, u=None, draw=True, class_logw=True))
    if name.endswith('_K256_l8'):
        out.append(dict(kind='masked', mask=np.ones(N, dtype=bool), known=known, u=None, draw=True, class_logw=True))
        # a stack of exactly one tile of 16 rows: 40 samples and the normalisers are at least four tiles, so at least four chunks
        mb = max(c.shape[2] for c in cores)
        out.append(dict(kind='masked', mask=mask, known=known, u=None, draw=True, class_logw=True, stack_bytes=16 * (N + 1) * mb * mb * 8))
    return out


def run_call(ctx, chain, call, seed):
    """the outputs of one call as a dict of arrays"""
    cores, l, phi, w, classes, u, mask, known, cap = chain
    n = len(classes)
    if call['kind'] == 'sample':
        lev, lab, lp = ctx.sample(n, phi, w, classes, call['given'], call['u'], seed)
        return dict(levels=lev, labels=lab, logp=lp)
    if 'stack_bytes' in call:
        ctx.set_sample_stack_bytes(call['stack_bytes'])
    try:
        res = ctx.sample_masked(n, phi, w, call['mask'], call['known'], classes, call['u'], seed, call['draw'], call['class_logw'])
    finally:
        ctx.set_sample_stack_bytes(1 << 30)
    out = dict(labels=res[1], logp=res[2])
    if call['draw']:
        out['levels'] = res[0]
    if call['class_logw']:
        out['class_logw'] = res[3]
    return out


def main(out, commit=None):
    if commit is None:
        commit = subprocess.run(['git', '-C', ROOT, 'rev-parse', 'HEAD'], capture_output=True, text=True, check=True).stdout.strip()
    rec, chains, calls, failed, tried = {}, [], [], [], 0
    for name, chain in chain_list().items():
        cores, l, phi, w, classes, u, mask, known, cap = chain
        N, D, L = len(cores), phi.shape[1], cores[l].shape[3]
        chains.append(dict(name=name, N=N, D=D, L=L, K=int(phi.shape[0]), l_pos=l, capacity=cap, n=len(classes)))
        for i, c in enumerate(cores):
            rec['%s/core%d' % (name, i)] = c
        rec[name + '/phi'], rec[name + '/w'], rec[name + '/classes'] = phi, w, classes
        ctx = _hip.Context(N, D, L, context_M(D, cap, L), 8)
        ctx.set_any_position(True)
        ctx.set_cores(cores, l)
        for call in calls_of(name, chain):
            cid = 'c%02d' % tried
            seed = SEED_OF.get(cid, 1000 + tried)
            tried += 1
            meta = dict(id=cid, chain=name, kind=call['kind'], seed=seed)
            for key in ('draw', 'class_logw', 'stack_bytes'):
                if key in call:
                    meta[key] = call[key]
            for key in ('given', 'mask', 'known', 'u'):
                if call.get(key) is not None:
                    a = np.asarray(call[key])
                    rec['%s/%s' % (cid, key)] = a.astype(np.uint8) if key == 'mask' else np.ascontiguousarray(a)
            try:
                res = run_call(ctx, chain, call, seed)
            except _hip.TnmlError as e:
                failed.append((cid, name, str(e)))
                print('%s %-20s %-6s REFUSED: %s' % (cid, name, call['kind'], e))
                continue
            for key, a in res.items():
                rec['%s/out_%s' % (cid, key)] = a
            calls.append(meta)
            print('%s %-20s %-6s seed %d  mean logp %.6f %.6f' % (cid, name, call['kind'], seed, res['logp'][:, 0].mean(), res['logp'][:, 1].mean()))
        ctx.close()
    rec['commit'], rec['chains'], rec['calls'] = np.array(commit), np.array(json.dumps(chains)), np.array(json.dumps(calls))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    np.savez_compressed(out, **rec)
    print('wrote', out, os.path.getsize(out), 'bytes,', len(calls), 'calls at commit', commit)
    if failed:
        sys.exit('refused: %s' % failed)


if __name__ == '__main__':
    main(*sys.argv[1:3])
