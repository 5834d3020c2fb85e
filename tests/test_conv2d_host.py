"""The arithmetic of conv2d on the host, under AddressSanitizer and UndefinedBehaviorSanitizer: tests/host/conv2d_harness.cpp is a
stand-alone program (plain g++, no HIP) that runs include/prost/linop/conv2d.hpp -- the geometry, the tap compaction, the staging of a
tile and the march prost_amd/csrc/kernels_linop_conv2d.hip calls in every lane, and the sums of the host block -- tile by tile in a
plain loop, for fp32 and fp64 and the three shapes, against the explicit sum in long double: |got - exact| <= 1.01 (t + 1) u (|K| |x|)
componentwise in both directions, the accumulating forms bit for bit against res0 + plain, the adjoint from the flipped table equal to
the transpose of the forward matrix entry for entry, the row and column sums within (t + 8) eps_T of the sums of the matrix.  Shapes:
the list of tests/test_gpu_conv2d.py; every buffer has exactly its size."""
import re

import host_harness


def test_marches_and_sums_under_sanitizers(tmp_path):
    stdout = host_harness.run_sanitized("conv2d_harness", tmp_path)
    lines = stdout.strip().splitlines()
    assert lines[-1] == "ok" and "FAIL" not in stdout
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
