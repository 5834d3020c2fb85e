"""The arithmetic of sym_gradient2d on the host, under AddressSanitizer and UndefinedBehaviorSanitizer:
tests/host/sym_gradient2d_harness.cpp is a stand-alone program (plain g++, no HIP) that runs include/prost/linop/sym_gradient2d.hpp --
the term functions, the forward and the adjoint march prost_amd/csrc/kernels_linop_sym_gradient2d.hip calls in every lane, for W = 1
and the vector widths 2 and 4, and the closed-form sums of the host block -- strip by strip and chunk by chunk in a plain loop, for
fp32 and fp64 and w = 0.5 and sqrt(1/2), against the explicit entry list summed in long double:
|got - exact| <= 1.01 (t + 1) u (|E| |x|) componentwise in both directions (t = 4), the accumulating forms bit for bit against
res0 + plain, every W, strip width and chunk width bit for bit against W = 1, both marches on unit vectors equal to the entry list and
its transpose entry for entry, the row and column sums within (t + 8) eps_T of the sums of the entries (w = 0.5, alpha = 1: equal).
Shapes: the list of tests/test_gpu_sym_gradient2d.py; every buffer has exactly its size."""
import re

import host_harness


def test_marches_and_sums_under_sanitizers(tmp_path):
    stdout = host_harness.run_sanitized("sym_gradient2d_harness", tmp_path)
    lines = stdout.strip().splitlines()
    assert lines[-1] == "ok" and "FAIL" not in stdout
    for t in ("fp32", "fp64"):
        got = [l for l in lines if re.match(r"\d+x\d+x\d+ w 0\.(500|707) %s: \d+ entries, worst error / bound [0-9.]+, within$" % t, l)]
        assert len(got) == 40, (t, len(got))               # twenty shapes, two weights
        for start in ("1x1x1 w 0.500", "1x7x1 w 0.707", "5x1x1 w 0.500", "66x5x1 w 0.707", "1024x3x1 w 0.500", "513x3x1 w 0.707", "4x24577x1 w 0.707", "8x4097x3 w 0.500"):
            assert any(l.startswith(start) for l in got), start
        # the check has teeth: some shape comes within two orders of magnitude of its bound, none passes it
        ratios = [float(re.search(r"bound ([0-9.]+),", l).group(1)) for l in got]
        assert max(ratios) <= 1.0 and max(ratios) > 0.01, ratios
    m = re.match(r"marches equal to the matrix and its transpose entry for entry in (\d+) runs$", lines[-2])
    assert m and int(m.group(1)) >= 20, lines[-2]
