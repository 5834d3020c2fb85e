"""The arithmetic of dataterm_sublabel on the host, under AddressSanitizer and UndefinedBehaviorSanitizer:
tests/host/dataterm_sublabel_harness.cpp is a stand-alone program (plain g++, no HIP) that runs include/prost/linop/dataterm_sublabel.hpp
-- the marches prost_amd/csrc/kernels_linop_dataterm_sublabel.hip calls in every lane, and the sum formulas of the host block -- in a
plain loop over the pixels, for fp32 and fp64, against a long-double evaluation of the matrix: |got - exact| <= 1.01 (k + 2) u (|K| |x|)
componentwise, <K x, y> = <x, K^T y> within the same bound, the accumulating and in-place forms and a two-pixel access bit for bit
against the plain march.  Shapes include k = 1 and N = 1; every buffer has exactly its size."""
import re

import host_harness


def test_marches_and_sums_under_sanitizers(tmp_path):
    stdout = host_harness.run_sanitized("dataterm_sublabel_harness", tmp_path)
    lines = stdout.strip().splitlines()
    assert lines[-1] == "ok" and "FAIL" not in stdout
    for t in ("fp32", "fp64"):
        got = [l for l in lines if re.match(r"N=\d+ L=\d+ .* %s: worst error / bound [0-9.]+, within$" % t, l)]
        assert len(got) == 9, (t, len(got))
        assert any(l.startswith("N=1 L=2 ") for l in got) and any(l.startswith("N=1 L=9 ") for l in got) and any(l.startswith("N=7 L=2 ") for l in got)
        # the check has teeth: some shape comes near its bound's order of magnitude, none passes it
        ratios = [float(re.search(r"bound ([0-9.]+),", l).group(1)) for l in got]
        assert max(ratios) <= 1.0 and max(ratios) > 0.01, ratios
