"""The arithmetic of fft2d on the host, under AddressSanitizer and UndefinedBehaviorSanitizer: tests/host/fft2d_harness.cpp is a
stand-alone program (plain g++, no HIP, nothing preloaded) that runs include/prost/linop/fft2d.hpp -- the table, the tree, the passes,
the scaling and the closed-form sums that prost_amd/csrc/kernels_linop_fft2d.hip and the host block use -- for fp32 and fp64 at every
case of tests/fft2d_reference.py, forward and transposed, plain and accumulating, against exactly sized buffers.  Its outputs are
compared here bit for bit with the NumPy restatement (-0 and +0 compare equal); the harness itself checks the table's exact entries
and symmetries, the period classes, and the sum table against a brute-force sum."""
import os
import re

import numpy as np

import fft2d_reference as R
import host_harness


def test_header_under_sanitizers_bit_for_bit_with_the_restatement(tmp_path):
    inputs = {}
    for case in R.CASES:
        nx, ny, L = case
        for name, dtype in (("fp32", np.float32), ("fp64", np.float64)):
            rng = np.random.default_rng(R.case_seed(case, 3))
            rhs, res0 = rng.standard_normal(2 * L * nx * ny).astype(dtype), rng.standard_normal(2 * L * nx * ny).astype(dtype)
            stem = os.path.join(str(tmp_path), "%s_%s" % (R.case_id(case), name))
            rhs.tofile(stem + "_rhs.bin")
            res0.tofile(stem + "_res0.bin")
            inputs[(case, name)] = (stem, dtype, rhs, res0)
    stdout = host_harness.run_sanitized("fft2d_harness", tmp_path, args=[str(tmp_path)])
    lines = stdout.strip().splitlines()
    assert lines[-1] == "ok" and "FAIL" not in stdout
    assert "tables of 1 .. 2048 entries: exact entries and symmetries hold" in lines
    ran = [l for l in lines if re.match(r"\d+x\d+x\d+ fp(32|64): \d+ values, forward and transposed, plain and accumulating$", l)]
    assert len(ran) == 2 * len(R.CASES)
    for (case, name), (stem, dtype, rhs, res0) in inputs.items():
        nx, ny, L = case
        assert "%s %s: %d values, forward and transposed, plain and accumulating" % (R.case_id(case), name, rhs.size) in ran
        for transpose, tag in ((False, "fwd"), (True, "inv")):
            want = R.product(rhs, nx, ny, L, transpose, dtype)
            got = np.fromfile("%s_%s.bin" % (stem, tag), dtype)
            assert got.shape == want.shape and np.array_equal(got, want), (case, name, tag, int((got != want).sum()))
            got = np.fromfile("%s_%s_acc.bin" % (stem, tag), dtype)
            assert np.array_equal(got, res0 + want), (case, name, tag, "accumulating")
