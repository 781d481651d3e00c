#!/usr/bin/env python3
"""GPU: record what Context.svd_split returns, bit for bit, on the in-LDS Jacobi kernel (kernels_narrow.hip) -- the fixture of
tests/test_jacobi_role_loops_gpu.py.

Run it on the build whose bits are to be the reference (for a change that must not move a bit: the parent commit's build), then
commit the file:

    python tools/record_svd_split_bits.py tests/golden/svd_split_bits.npz

Per case (family, short side n, cut m) the file holds the input matrix (n x 2n float32: two of the families go through LAPACK and
BLAS on the host, whose last bits are not the same everywhere), US, SVh, sigma and the increments of the sweeps, rounds and Cholesky
counters of svd_stats over the call.  A later, deliberate change of SVD numerics re-records the file with this script.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import svd_split_reference as sr                       # noqa: E402
from tensornetworkforml_amd import _hip                # noqa: E402

# a pair that meets itself; the first sizes with separate V and G waves; the two benchmark sizes; the largest size at one V block
# per lane; two V blocks per lane; a second G item per thread
SIZES = (2, 4, 6, 20, 40, 42, 48, 62)
# gauss and near_equal (nearly orthonormal rows) at every size; graded1e6, which takes the Cholesky step wherever the kernel has it
# (n > 4), at the sizes of SIZES_CHOL -- an n x 2n Gaussian matrix has off(G) / trace(G) ~ 1 / sqrt(2n), under the threshold
FAMILIES = {'gauss': SIZES, 'near_equal': SIZES, 'graded1e6': (4, 6, 20, 40, 42)}


def cuts(n):
    return sorted({1, max(1, n // 2), n})


def case_list():
    return [(f, n, m) for f, sizes in FAMILIES.items() for n in sizes for m in cuts(n)]


def stats(ctx):
    sweeps, svds, rounds = ctx.svd_stats(False)
    return np.array([sweeps, svds, rounds, ctx.cholesky_steps], np.float64)


def main(out):
    ctx = _hip.Context(4, 2, 2, 64, 64)
    rec = {}
    for family, n, m in case_list():
        key = '%s_%d' % (family, n)
        if 'A_' + key not in rec:
            rec['A_' + key] = sr.make(family, n, 2 * n)
        A = rec['A_' + key]
        s0 = stats(ctx)
        US, SVh, sig = ctx.svd_split(A, m)
        d = stats(ctx) - s0
        assert d[1] == 1, d
        key += '_%d' % m
        rec['US_' + key], rec['SVh_' + key], rec['sigma_' + key] = US, SVh, sig
        rec['counters_' + key] = d[[0, 2, 3]].astype(np.int64)          # sweeps, rounds, Cholesky steps
        print('%-12s n %2d m %2d  sweeps %2d rounds %4d cholesky %d  sigma_max %.6e' % (family, n, m, d[0], d[2], d[3], sig[0]))
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    np.savez(out, **rec)
    print('wrote', out, os.path.getsize(out), 'bytes')


if __name__ == '__main__':
    main(sys.argv[1])
