"""The arithmetic of nonlocal_gradient2d on the host, under AddressSanitizer and UndefinedBehaviorSanitizer:
tests/host/nonlocal_gradient2d_harness.cpp is a stand-alone program (plain g++, no HIP, nothing preloaded) that runs
include/prost/linop/nonlocal_gradient2d.hpp -- the staging of the tile, the forward and the adjoint cell that
prost_amd/csrc/kernels_linop_nonlocal_gradient2d.hip calls in every lane, and the sums of the host block -- for fp32 and fp64, forward
and adjoint, plain and accumulating, at every case of tests/nonlocal_gradient2d_reference.py, against exactly sized buffers.  The main
run uses the geometry of the kernels (tiles of 64 x 16, lanes of 16 bytes where the height allows, the tile table's channels per pass);
inside the harness every other lane width, small tiles, few lanes and 1 .. 4 channels per pass have to give the same bits.  Its outputs
are compared here bit for bit with the NumPy restatement (b), and its row and column sums (alpha = 1 and 2) with the sums (c) of the
explicit matrix: equal for the dyadic weights, within (t + 8) eps_T otherwise, t = 2 M.  The tile table has to stay within 64 KiB for
every reach and both precisions, and has to be the table the reference module holds."""
import os
import re

import numpy as np

import host_harness
import nonlocal_gradient2d_reference as R

ALPHAS = (1.0, 2.0)
PRECISIONS = (("fp32", np.float32), ("fp64", np.float64))


def test_header_under_sanitizers_bit_for_bit_with_the_restatement(tmp_path):
    d = str(tmp_path)
    inputs, lines = {}, []
    for case in R.CASES:
        ny, nx, L, key = case
        offsets = R.OFFSETS[key]
        N, M = nx * ny, len(offsets)
        lines.append("%s %d %d %d %d 1" % (R.case_id(case), nx, ny, L, M))
        np.array(offsets, dtype=np.int8).tofile(os.path.join(d, "%s_offsets.bin" % R.case_id(case)))
        planes = R.weights_for(case)
        for name, dtype in PRECISIONS:
            rng = np.random.default_rng(R.case_seed(case, 5))
            arrays = dict(rhs=rng.standard_normal(L * N).astype(dtype), rhst=rng.standard_normal(M * L * N).astype(dtype),
                          res0=rng.standard_normal(M * L * N).astype(dtype), res0t=rng.standard_normal(L * N).astype(dtype),
                          weights=np.concatenate(planes).astype(dtype))
            stem = os.path.join(d, "%s_%s" % (R.case_id(case), name))
            for key_, v in arrays.items():
                v.tofile("%s_%s.bin" % (stem, key_))
            inputs[(case, name)] = (stem, dtype, arrays, planes)
    with open(os.path.join(d, "cases.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    stdout = host_harness.run_sanitized("nonlocal_gradient2d_harness", tmp_path, args=[d])
    out = stdout.strip().splitlines()
    assert out[-1] == "ok" and "FAIL" not in stdout and "%d cases" % len(R.CASES) in out
    # the tile table: within 64 KiB for every reach and both precisions, and the one the shape list was made from
    table = [tuple(int(v) for v in re.match(r"table reach (\d+) bytes (\d+) channels (\d+) lds (\d+)$", l).groups()) for l in out if l.startswith("table ")]
    assert len(table) == 2 * (R.MAX_REACH + 1)
    for r, bytes_, channels, lds in table:
        assert channels == R.PASS_CHANNELS[bytes_][r] and 1 <= channels <= R.MAX_PASS
        assert lds == channels * R.tile_values(r, r) * bytes_ <= R.LDS_LIMIT
        assert channels == R.MAX_PASS or (channels + 1) * R.tile_values(r, r) * bytes_ > R.LDS_LIMIT
    ran = [l for l in out if re.search(r" fp(32|64): \d+ values, W = [124], reach \d+ x \d+, \d channels per pass, forward and adjoint, plain and accumulating, every geometry the same bits$", l)]
    assert len(ran) == 2 * len(R.CASES)
    # the main run is the geometry of the kernels: 16 bytes per lane where the height allows, one row otherwise
    assert any(l.startswith("64x15x1_w1 fp32") and "W = 4" in l for l in ran) and any(l.startswith("65x16x1_grad fp32") and "W = 1" in l for l in ran)
    assert any(l.startswith("66x4x1_pos fp64") and "W = 2" in l for l in ran) and any(l.startswith("66x4x1_pos fp32") and "W = 1" in l for l in ran)
    assert any(l.startswith("24x20x4_far fp32") and "3 channels per pass" in l for l in ran) and any(l.startswith("24x20x4_far fp64") and "1 channels per pass" in l for l in ran)
    for (case, name), (stem, dtype, arrays, planes) in inputs.items():
        ny, nx, L, key = case
        offsets = R.OFFSETS[key]
        for transpose, tag, rhs, res0 in ((False, "fwd", arrays["rhs"], arrays["res0"]), (True, "adj", arrays["rhst"], arrays["res0t"])):
            want = R.product(rhs, nx, ny, L, offsets, planes, transpose, dtype)
            got = np.fromfile("%s_%s.bin" % (stem, tag), dtype)
            assert got.shape == want.shape and np.array_equal(got, want), (case, name, tag, int((got != want).sum()))
            assert np.array_equal(np.signbit(got), np.signbit(want)), (case, name, tag)
            got = np.fromfile("%s_%s_acc.bin" % (stem, tag), dtype)
            assert np.array_equal(got, res0 + want), (case, name, tag, "accumulating")
        tol = (R.sum_terms(len(offsets)) + 8) * np.finfo(dtype).eps
        for a, alpha in enumerate(ALPHAS):
            for tag, want in zip(("rowsum", "colsum"), R.sums(nx, ny, L, offsets, planes, alpha, dtype)):
                got = np.fromfile("%s_%s_%d.bin" % (stem, tag, a), np.float64)
                assert got.shape == want.shape and np.all(np.abs(got - want) <= tol * want), (case, name, alpha, tag)
                if R.is_dyadic(case):
                    assert np.array_equal(got, want), (case, name, alpha, tag)
