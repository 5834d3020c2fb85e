"""The arithmetic of radon2d on the host, under AddressSanitizer and UndefinedBehaviorSanitizer: tests/host/radon2d_harness.cpp is a
stand-alone program (plain g++, no HIP, nothing preloaded) that runs include/prost/linop/radon2d.hpp -- the per-angle table, the forward
enumeration, the gather enumeration with its candidate window, the marches prost_amd/csrc/kernels_linop_radon2d.hip calls in every lane,
and the sums of the host block -- for fp32 and fp64: table values at 0, pi / 4, pi / 2 and pi; at the small shapes the gather and the
forward enumeration give the same entry set with the same bits, unit vectors reproduce it and its transpose entry for entry, plain and
accumulating; random vectors stay within 1.01 (t + 1) u (|K| |x|) of the entry list summed in long double; the sums equal a brute-force
sum, empty ones exactly 0; and of 10^6 sampled entries at 8192 x 8192 in fp32, at spacing 0.5, 1 and 8, none lies outside the candidate
window.  Every buffer has exactly its size."""
import re

import host_harness


def test_enumerations_marches_window_and_sums_under_sanitizers(tmp_path):
    stdout = host_harness.run_sanitized("radon2d_harness", tmp_path)
    lines = stdout.strip().splitlines()
    assert lines[-1] == "ok" and "FAIL" not in stdout
    for t in ("fp32", "fp64"):
        got = [l for l in lines if re.match(r"\d+x\d+x\d+ ndet \d+ spacing [0-9.]+ shift [-0-9.]+ %s: \d+ entries, worst error / bound [0-9.]+, within$" % t, l)]
        assert len(got) == 12, (t, len(got))
        for start in ("1x1x1 ndet 1 ", "5x5x2 ndet 63 spacing 0.5 shift -0.3", "9x7x1 ndet 3 ", "65x6x1 ndet 135 spacing 0.5", "33x70x1 ndet 64 "):
            assert any(l.startswith(start) for l in got), start
        # the check has teeth: the worst ratio (carried from shape to shape) comes near the bound's order of magnitude and never passes it
        ratio = float(re.search(r"bound ([0-9.]+),", got[-1]).group(1))
        assert 0.01 < ratio <= 1.0, ratio
    scale = [l for l in lines if l.startswith("8192x8192 fp32 spacing ")]
    assert len(scale) == 3
    for l, (spacing, most) in zip(scale, (("0.5", 4), ("1", 2), ("8", 1))):
        m = re.match(r"8192x8192 fp32 spacing %s: (\d+) sampled entries, 0 outside the window, at most (\d+) bins per pixel and angle \(window (\d+)\)$" % re.escape(spacing), l)
        assert m and int(m.group(1)) >= 10 ** 6 and int(m.group(2)) <= most < int(m.group(3)), l
    m = re.match(r"entry list and transpose reproduced entry for entry in (\d+) runs$", lines[-2])
    assert m and int(m.group(1)) >= 12, lines[-2]
