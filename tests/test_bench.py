"""bench.py's command line: a plain run prints the headline and nothing that needs passes of its own, --dump-outputs
writes what the last timed pass computed, --full adds the secondary measurements."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ('metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step')
FULL_ONLY = ('finite', 'breakdown', 'final_accuracy', 'roofline', 'kernels', 'resident_batch', 'cold_start')


def run_bench(*args, timeout=300):
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py')] + list(args), cwd=ROOT, capture_output=True,
                         text=True, timeout=timeout)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, out.stdout[-2000:]
    return json.loads(lines[0])


def test_bench_options():
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--help'], capture_output=True, text=True,
                         timeout=60)
    assert out.returncode == 0, out.stderr
    assert '--full' in out.stdout and '--dump-outputs' in out.stdout


@pytest.mark.gpu
def test_bench_plain_run_dumps_outputs(tmp_path):
    N, b, L = 784, 1000, 2
    res = run_bench('--gpus', '1', '--config', 'c2', '--steps', '2', '--warmup', '1', '--dump-outputs', str(tmp_path))
    for k in HEADLINE:
        assert k in res, k
    assert res['steps'] == 2 and res['unit'] == 'sweep-steps/s' and res['higher_is_better'] is True
    assert res['value'] > 0 and res['ms_per_step'] > 0
    assert abs(res['value'] * res['ms_per_step'] * 1e-3 - (N - 1)) < 1e-6 * (N - 1)
    for k in FULL_ONLY + ('cpu_baseline',):
        assert k not in res, k
    arrs = {n: np.load(str(tmp_path / (n + '.npy'))) for n in ('cores', 'bond', 'l_pos', 'f')}
    assert sum(a.nbytes for a in arrs.values()) <= 64 << 20
    for a in arrs.values():
        assert a.dtype in (np.float32, np.float64)
    # one warm-up + two timed passes from l_pos = 0: right, left, right
    assert int(arrs['l_pos'][0]) == N - 1
    bond = arrs['bond'].astype(int)
    assert bond.shape == (N - 1,) and bond.max() == 10
    ml = np.concatenate([[1], bond])
    mr = np.concatenate([bond, [1]])
    assert arrs['cores'].size == int((ml * 2 * mr).sum()) + int(ml[-1] * 2 * mr[-1]) * (L - 1)
    assert arrs['f'].shape == (L, b)
    assert np.isfinite(arrs['cores']).all() and np.isfinite(arrs['f']).all()


@pytest.mark.gpu
def test_bench_full_run():
    res = run_bench('--gpus', '1', '--config', 'c2', '--steps', '1', '--warmup', '1', '--full', '--cpu-steps', '0')
    for k in HEADLINE + FULL_ONLY:
        assert k in res, k
    assert res['finite'] is True
