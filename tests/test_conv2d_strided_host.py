"""The arithmetic of conv2d_strided on the host, under AddressSanitizer and UndefinedBehaviorSanitizer:
tests/host/conv2d_strided_harness.cpp is a stand-alone program (plain g++, no HIP, nothing preloaded) that runs
include/prost/linop/conv2d_strided.hpp -- the geometry, the tile table, both tap tables, the staging of the de-interleaved forward tile
and of the adjoint tile, the marches prost_amd/csrc/kernels_linop_conv2d_strided.hip calls in every lane, and the sums of the host block
-- tile by tile in a plain loop, for fp32 and fp64, against the entry list of the matrix summed in long double:
|got - exact| <= 1.01 (t + 1) u (|K| |x|) componentwise in both directions; every tile-table entry that fits gives the bits of the
chosen one; the accumulating forms are res0 + plain bit for bit; at the small shapes unit vectors reproduce the entry list and its
transpose entry for entry; the sums are within (t + 8) eps_T, empty ones exactly 0; every argument combination has a tile within 64 KiB.
Every buffer has exactly its size."""
import re

import host_harness


def test_marches_tiles_and_sums_under_sanitizers(tmp_path):
    stdout = host_harness.run_sanitized("conv2d_strided_harness", tmp_path)
    lines = stdout.strip().splitlines()
    assert lines[-1] == "ok" and "FAIL" not in stdout
    m = re.match(r"largest staged tile: forward (\d+) bytes, adjoint (\d+) bytes$", lines[0])
    assert m and 0 < int(m.group(1)) <= 65536 and 0 < int(m.group(2)) <= 65536, lines[0]
    for t in ("fp32", "fp64"):
        got = [l for l in lines if re.match(r"\d+x\d+x\d+ window \d+x\d+ stride \dx\d phase \d,\d (full|same|valid) %s: \d+ taps, tile \d, worst error / bound [0-9.]+, within$" % t, l)]
        assert len(got) == 24, (t, len(got))
        for start in ("1x1x1 window 1x1 stride 1x1", "7x5x1 window 1x1 stride 4x4 phase 3,3 full", "12x11x2 window 3x3 stride 3x2 phase 1,0 same",
                      "5x4x1 window 5x4 stride 2x2 phase 0,0 valid", "9x6x1 window 31x31 stride 4x4", "257x65x1 window 3x3 stride 4x4", "129x17x1 window 31x31 stride 4x4"):
            assert any(l.startswith(start) for l in got), start
        # the check has teeth: some shape comes near its bound's order of magnitude, none passes it
        ratios = [float(re.search(r"bound ([0-9.]+),", l).group(1)) for l in got]
        assert max(ratios) <= 1.0 and max(ratios) > 0.01, ratios
    # both precisions together exercise more than one entry of the tile table
    assert len(set(re.search(r"tile (\d),", l).group(1) for l in lines if ", tile " in l)) >= 4
    m = re.match(r"entry list and transpose reproduced entry for entry in (\d+) runs$", lines[-2])
    assert m and int(m.group(1)) >= 16, lines[-2]
