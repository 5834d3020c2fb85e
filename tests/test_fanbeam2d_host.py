"""The arithmetic of fanbeam2d on the host, under AddressSanitizer and UndefinedBehaviorSanitizer: tests/host/fanbeam2d_harness.cpp is a
stand-alone program (plain g++, no HIP, nothing preloaded) that runs include/prost/linop/fanbeam2d.hpp -- the three tables, the ray
enumeration, the gather enumeration with its candidate window, the marches prost_amd/csrc/kernels_linop_fanbeam2d.hip calls in every
lane, and the sums of the host block -- for fp32 and fp64, flat and curved: at the small shapes the gather and the ray enumeration give
the same entry set with the same bits, unit vectors reproduce it and its transpose entry for entry, plain and accumulating; random
vectors stay within 1.01 (t + 1) u (|K| |x|) of the entry list summed in long double; the sums equal a brute-force sum, empty ones
exactly 0; of 10^6 sampled entries at 8192 x 8192 in fp32 none lies outside the candidate window.  Every buffer has exactly its size.

The harness prints a digest of both products of a fixed input per shape and precision; here the NumPy restatement of
tests/fanbeam2d_reference.py, which repeats the header operation for operation, has to give the same digests."""
import re

import numpy as np

import fanbeam2d_reference as F
import host_harness

DIGEST = re.compile(r"digest (\d+) (\d+) (\d+) (\d+) (\S+) (\S+) (\S+) (\S+) (flat|curved) (fp32|fp64) margin (\d+) forward ([0-9a-f]{16}) adjoint ([0-9a-f]{16})$")


def test_enumerations_marches_window_sums_and_digests_under_sanitizers(tmp_path):
    stdout = host_harness.run_sanitized("fanbeam2d_harness", tmp_path)
    lines = stdout.strip().splitlines()
    assert lines[-1] == "ok" and "FAIL" not in stdout
    for t in ("fp32", "fp64"):
        got = [l for l in lines if re.match(r"\d+x\d+x\d+ ndet \d+ spacing [0-9.]+ shift [-0-9.]+ R [0-9.]+ D [0-9.]+ (flat|curved) %s: \d+ entries, margin \d, worst error / bound [0-9.]+, within$" % t, l)]
        assert len(got) == 12, (t, len(got))
        assert {int(re.search(r"margin (\d)", l).group(1)) for l in got} == {1, 2, 3, 4, 5}
        # the check has teeth: the worst ratio (carried from shape to shape) comes near the bound's order of magnitude and never passes it
        ratio = float(re.search(r"bound ([0-9.]+),", got[-1]).group(1))
        assert 0.01 < ratio <= 1.0, ratio
    scale = [l for l in lines if l.startswith("8192x8192 fp32 ")]
    assert len(scale) == 4
    for l in scale:
        m = re.match(r"8192x8192 fp32 (flat|curved) spacing \S+ R \S+ hd: (\d+) sampled entries, 0 outside the window, at most (\d+) bins per pixel and view \(window (\d+)\)$", l)
        assert m and int(m.group(2)) >= 10 ** 6 and int(m.group(3)) < int(m.group(4)), l
    m = re.match(r"entry list and transpose reproduced entry for entry in (\d+) runs$", lines[-2])
    assert m and int(m.group(1)) >= 12, lines[-2]
    assert any(re.match(r"atan fit: largest error \S+ on", l) for l in lines)
    # the digests against the restatement
    digests = [DIGEST.match(l) for l in lines if l.startswith("digest ")]
    assert len(digests) == 24 and all(digests)
    angles = np.array(F.VIEW_SETS["quad"])
    for d in digests:
        ny, nx, planes, ndet = (int(v) for v in d.group(1, 2, 3, 4))
        spacing, shift, dist, D = (float(v) for v in d.group(5, 6, 7, 8))
        detector, dtype = d.group(9), {"fp32": np.float32, "fp64": np.float64}[d.group(10)]
        args = (nx, ny, planes, angles, dist, D, ndet, spacing, shift, detector)
        assert F.margin(nx, ny, dist, D, ndet, spacing, shift, detector == "curved") == int(d.group(11)), d.group(0)
        u, v = F.digest_input(nx * ny * planes, 1, dtype), F.digest_input(len(angles) * ndet * planes, 2, dtype)
        assert F.digest(F.product(u, *args, False, dtype)) == d.group(12), d.group(0)
        assert F.digest(F.product(v, *args, True, dtype)) == d.group(13), d.group(0)
