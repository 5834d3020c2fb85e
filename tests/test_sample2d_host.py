"""The arithmetic of sample2d on the host, under AddressSanitizer and UndefinedBehaviorSanitizer: tests/host/sample2d_harness.cpp is a
stand-alone program (plain g++, no HIP, nothing preloaded) that runs include/prost/linop/sample2d.hpp -- the entries of a row, the bucket
tables, the gather enumeration, the sums prost_amd/csrc/kernels_linop_sample2d.hip calls in every lane, and the sums of the host block --
for fp32 and fp64 at the case list: every sample with entries stands exactly once in the bucket of its own cell, ascending inside it; the
gather and the forward enumeration give the same entry set with the same bits; unit vectors reproduce it and its transpose entry for
entry, plain and accumulating; random vectors stay within 1.01 (t + 1) u (|K| |x|) of the entry list summed in long double; the sums equal
a brute-force sum, empty ones exactly 0; and 10^6 random positions, huge, negative and non-finite ones included, give offsets and cells
inside a 16384 x 16384 image in fp32 (by value: the image alone would be 1 GiB), and run against exactly sized buffers at 16384 x 2 and
2 x 16384.  Every buffer has exactly its size."""
import re

import host_harness


def test_buckets_enumerations_products_sums_and_index_safety_under_sanitizers(tmp_path):
    stdout = host_harness.run_sanitized("sample2d_harness", tmp_path)
    lines = stdout.strip().splitlines()
    assert lines[-1] == "ok" and "FAIL" not in stdout
    for t in ("fp32", "fp64"):
        got = [l for l in lines if re.match(r"\d+x\d+x\d+ [a-z]+ M \d+ %s: \d+ entries, worst error / bound [0-9.]+, within$" % t, l)]
        assert len(got) == 13, (t, len(got))
        for start in ("1x1x1 random M 1 ", "1x7x2 special M 63 ", "7x1x3 special M 64 ", "1x1x1 special M 65 ", "64x5x1 random M 257 ", "65x6x2 special M 257 ",
                      "7x10x1 onecell M 300 ", "33x70x1 flow M 2310 ", "5x4x1 integers M 20 "):
            assert any(l.startswith(start) for l in got), start
        # the check has teeth: the worst ratio (carried from shape to shape) comes near the bound's order of magnitude and never passes it
        ratio = float(re.search(r"bound ([0-9.]+),", got[-1]).group(1))
        assert 0.01 < ratio <= 1.0, ratio
    m = [re.match(r"16384x16384 fp32: (\d+) positions, (\d+) with entries, (\d+) out of reach, every offset and cell inside$", l) for l in lines]
    m = [v for v in m if v]
    assert len(m) == 1 and int(m[0].group(1)) >= 10 ** 6 and int(m[0].group(2)) > 10 ** 5 and int(m[0].group(3)) > 10 ** 5
    assert len([l for l in lines if re.match(r"(16384x2|2x16384) fp32: 250000 positions against exactly sized buffers, \d+ bucketed$", l)]) == 2
    m = re.match(r"entry list and transpose reproduced entry for entry in (\d+) runs$", lines[-2])
    assert m and int(m.group(1)) >= 16, lines[-2]
