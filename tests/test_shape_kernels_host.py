"""Host side of the shape-compiled persistent sweep, no GPU: the marks sweep_persist (tnml_api.hip) puts on the step records, under
AddressSanitizer + UBSan (csrc/Makefile target `san-shape`, the stand-alone program csrc/san/plan_shape_main.cpp)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_shape_marks_host_side_under_sanitizers():
    """Whole sweeps at bond 5, 10 and 20 (N = 24) and C3 at true size planned through the C ABI against the stand-in runtime of
    csrc/san/hip_stub.cpp, with tnml_set_shape_kernels on and off: a record is marked exactly where the program finds the uniform
    shape of a table entry in it, tnml_fixed_shape_steps says the same count, nothing is marked with the switch off, at bond 5, at
    three labels or in mode 2, a table constant that disagrees with a step cannot be marked, and the call traces of the two runs
    are the same text apart from the shape field and the kernel instantiation."""
    if shutil.which('g++') is None or not os.path.exists('/opt/rocm/bin/hipcc'):
        pytest.skip('no g++ / hipcc')
    csrc = os.path.join(ROOT, 'tensornetworkforml_amd', 'csrc')
    out = subprocess.run(['make', '-C', csrc, '-j4', 'san-shape'], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert out.stdout.count('shape-kernel host planning under ASan + UBSan: ok') == 2
    assert out.stdout.count('shape constants: 32 disagreeing values refused') == 2
    marked = {}
    for m in re.finditer(r'planned shapes N (\d+) bond (\d+) L (\d+) switch (on|off) mode (\d): (\d+) of (\d+) steps marked', out.stdout):
        marked[(int(m.group(1)), int(m.group(2)), int(m.group(3)), m.group(4), int(m.group(5)))] = (int(m.group(6)), int(m.group(7)))
    assert len(marked) == 12, marked
    for key, (got, steps) in marked.items():
        N, M, L, switch, mode = key
        in_table = switch == 'on' and mode == 1 and L == 2 and M in (10, 20)
        assert (got > 0) == in_table, (key, got)
        assert got < steps                                  # the ramps at the chain ends are never marked
    # C3: 783 steps per sweep; all but the ramps (2, 4, 8, 16 and the step behind them, at both ends) have the uniform shape
    got, steps = marked[(784, 20, 2, 'on', 1)]
    assert steps == 3 * 783 and got >= 3 * 770, got
    m = re.search(r'shape traces: (\d+) lines equal apart from the shape field', out.stdout)
    assert m and int(m.group(1)) > 1000
    assert len(re.findall(r'san-stub: \d+ launches checked \(\d+ kernels\), \d+ pointer extents checked, 0 live allocations', out.stdout)) == 2
