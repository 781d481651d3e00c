"""Host side of the slice reduction of the persistent sweep, no GPU: the plan sweep_persist (tnml_api.hip) writes into the step
records, under AddressSanitizer + UBSan (csrc/Makefile target `san-slices`, the stand-alone program csrc/san/plan_slices_main.cpp),
and the planner's mirror that tests/test_slice_reduce_gpu.py counts its expected steps with."""
import os
import re
import shutil
import subprocess

import pytest

import test_slice_reduce_gpu as gpu_side

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES = [(16, 20, 2, b) for b in (33, 512, 513, 1000, 5000)] + [(10, 5, 3, 513)]


def mirror_counts(N, M, L):
    """records beyond one level in three sweeps (right, left, right) from bonds that all equal M"""
    bond, out = [M] * (N - 1), []
    for sw in range(3):
        n, bond = gpu_side.records_beyond_one_level(bond, sw == 1, N, M, L)
        out.append(n)
    return out


def test_slice_plan_host_side_under_sanitizers():
    """Whole sweeps of the shapes of the GPU test and C3 at true size planned through the C ABI against the stand-in runtime of
    csrc/san/hip_stub.cpp, both persistent modes, switch 1 and 0.  The program reads the records back and checks: the runs of the
    reducers cover [0, n4) once, a run is a multiple of 8 elements, R <= workgroups, the helpers' done target is the reducer count
    of the record that forms their Z, the arrival and done words lie in the step's counter block on no word in use, switch 0 plans
    the last-arriver hand-off, and tnml_slice_reduce_steps counts the records.  Here: every uniform bond-20 step reduces in slices
    at each batch size, and the counts are what the GPU test's mirror of the planner says."""
    if shutil.which('g++') is None or not os.path.exists('/opt/rocm/bin/hipcc'):
        pytest.skip('no g++ / hipcc')
    csrc = os.path.join(ROOT, 'tensornetworkforml_amd', 'csrc')
    out = subprocess.run(['make', '-C', csrc, '-j4', 'san-slices'], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert out.stdout.count('slice-reduction host planning under ASan + UBSan: ok') == 1
    got = {}
    for m in re.finditer(r'planned slices N (\d+) bond (\d+) L (\d+) b (\d+) workgroups (\d+) switch (\d) mode (\d): (\d+) (\d+) (\d+) records in slices, '
                         r'(\d+) of (\d+) uniform steps', out.stdout):
        v = [int(x) for x in m.groups()]
        got[tuple(v[:4]) + (v[5], v[6])] = dict(wgs=v[4], counts=v[7:10], uniform=(v[10], v[11]))
    assert len(got) == 4 * len(SHAPES) + 2, sorted(got)
    for (N, M, L, b) in SHAPES:
        for mode in (1, 2):
            on, off = got[(N, M, L, b, 1, mode)], got[(N, M, L, b, 0, mode)]
            assert on['counts'] == mirror_counts(N, M, L), (N, M, L, b, mode, on)
            assert off['counts'] == [0, 0, 0]
            assert on['uniform'][0] == on['uniform'][1] > 0 and off['uniform'][0] == 0
            assert min(on['counts']) > 0
    # the group edges the batch sizes were chosen for (32-sample tiles of the batch padded to 64)
    assert [got[(16, 20, 2, b, 1, 1)]['wgs'] for b in (33, 512, 513, 1000, 5000)] == [2, 16, 18, 32, 158]
    c3 = got[(784, 20, 2, 5000, 1, 1)]
    assert c3['counts'] == mirror_counts(784, 20, 2) and c3['uniform'][0] == c3['uniform'][1] >= 3 * 770
    assert got[(784, 20, 2, 5000, 0, 1)]['counts'] == [0, 0, 0]
    assert len(re.findall(r'san-stub: \d+ launches checked \(\d+ kernels\), \d+ pointer extents checked, 0 live allocations', out.stdout)) == 1


def test_mirror_of_the_one_level_rule():
    """bond 20 at two labels: the 6400-float pre-gradient of a uniform step is beyond one level, the ramp steps are not"""
    f = gpu_side.batch_lds_floats
    assert 16 * (20 * 2 * 4 * 20 * 2 + 4) > f(2, 20, 20, 20, 20, False, True, True, True)
    assert 16 * (2 * 2 * 4 * 8 * 2 + 4) <= f(2, 2, 8, 8, 1, False, True, True, True)
