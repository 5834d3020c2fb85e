"""The arithmetic of conv2d on the host, under AddressSanitizer and UndefinedBehaviorSanitizer: tests/host/conv2d_harness.cpp is a
stand-alone program (plain g++, no HIP) that runs include/prost/linop/conv2d.hpp -- the geometry, the tap compaction, the staging of a
tile and the march prost_amd/csrc/kernels_linop_conv2d.hip calls in every lane, and the sums of the host block -- tile by tile in a
plain loop, for fp32 and fp64 and the three shapes, against the explicit sum in long double: |got - exact| <= 1.01 (t + 1) u (|K| |x|)
componentwise in both directions, the accumulating forms bit for bit against res0 + plain, the adjoint from the flipped table equal to
the transpose of the forward matrix entry for entry, the row and column sums within (t + 8) eps_T of the sums of the matrix.  Shapes:
the list of tests/test_gpu_conv2d.py; every buffer has exactly its size."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "conv2d_harness.cpp")


def test_marches_and_sums_under_sanitizers(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "conv2d_harness")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-I" + os.path.join(ROOT, "include"), SRC, "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-4000:])
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "ok" and "FAIL" not in r.stdout
    for t in ("fp32", "fp64"):
        got = [l for l in lines if re.match(r"\d+x\d+x\d+ window \d+x\d+( \(line\))? (full|same|valid) %s: \d+ taps, worst error / bound [0-9.]+, within$" % t, l)]
        assert len(got) == 29, (t, len(got))               # ten shapes, three forms each; 3 x 3 with a 5 x 5 window has no valid part
        for start in ("1x1x1 window 1x1 ", "3x3x1 window 5x5 same", "65x17x1 window 3x3 full", "130x35x3 window 15x15 (line) valid", "40x33x1 window 31x31 same"):
            assert any(l.startswith(start) for l in got), start
        # the check has teeth: some shape comes near its bound's order of magnitude, none passes it
        ratios = [float(re.search(r"bound ([0-9.]+),", l).group(1)) for l in got]
        assert max(ratios) <= 1.0 and max(ratios) > 0.01, ratios
    m = re.match(r"adjoint equal to the transpose entry for entry in (\d+) runs$", lines[-2])
    assert m and int(m.group(1)) >= 20, lines[-2]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
