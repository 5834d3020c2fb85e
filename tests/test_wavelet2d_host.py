"""The arithmetic of wavelet2d on the host, under AddressSanitizer and UndefinedBehaviorSanitizer: tests/host/wavelet2d_harness.cpp is a
stand-alone program (plain g++, no HIP, nothing preloaded) that runs include/prost/linop/wavelet2d.hpp -- the named taps, the passes,
the order of the levels, the limits and the sums that prost_amd/csrc/kernels_linop_wavelet2d.hip and the host block use -- for fp32 and
fp64 at every case of tests/wavelet2d_reference.py, forward and transposed, plain and accumulating, against exactly sized buffers.
Its outputs are compared here bit for bit with the NumPy restatement (-0 and +0 compare equal), its named taps bit for bit with the
reference's closed forms, and its row and column sums (every case with N <= 4096, alpha = 0.5, 1, 1.5) with the sums of the explicit
matrix within the reference's sums_tolerance."""
import os
import re

import numpy as np

import host_harness
import wavelet2d_reference as R

ALPHAS = (0.5, 1.0, 1.5)


def test_header_under_sanitizers_bit_for_bit_with_the_restatement(tmp_path):
    inputs, lines = {}, []
    for case in R.CASES:
        nx, ny, L, wavelet, levels = case
        h = R.taps(wavelet)
        with_sums = nx * ny <= 4096
        lines.append("%s %d %d %d %d %d %d" % (R.case_id(case), nx, ny, L, levels, len(h), with_sums))
        np.asarray(h, np.float64).tofile(os.path.join(str(tmp_path), R.case_id(case) + "_taps.bin"))
        for name, dtype in (("fp32", np.float32), ("fp64", np.float64)):
            rng = np.random.default_rng(R.case_seed(case, 3))
            rhs, res0 = rng.standard_normal(L * nx * ny).astype(dtype), rng.standard_normal(L * nx * ny).astype(dtype)
            stem = os.path.join(str(tmp_path), "%s_%s" % (R.case_id(case), name))
            rhs.tofile(stem + "_rhs.bin")
            res0.tofile(stem + "_res0.bin")
            inputs[(case, name)] = (stem, dtype, rhs, res0)
    with open(os.path.join(str(tmp_path), "cases.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    stdout = host_harness.run_sanitized("wavelet2d_harness", tmp_path, args=[str(tmp_path)])
    out = stdout.strip().splitlines()
    assert out[-1] == "ok" and "FAIL" not in stdout and "%d cases" % len(R.CASES) in out
    ran = [l for l in out if re.search(r" fp(32|64): \d+ values, forward and transposed, plain and accumulating$", l)]
    assert len(ran) == 2 * len(R.CASES)
    for name in ("haar", "db2", "db3"):
        got = np.fromfile(os.path.join(str(tmp_path), "named_%s.bin" % name), np.float64)
        assert got.shape == R.taps(name).shape and np.array_equal(got, R.taps(name)), name
    for (case, name), (stem, dtype, rhs, res0) in inputs.items():
        nx, ny, L, wavelet, levels = case
        for transpose, tag in ((False, "fwd"), (True, "inv")):
            want = R.product(rhs, nx, ny, L, wavelet, levels, transpose, dtype)
            got = np.fromfile("%s_%s.bin" % (stem, tag), dtype)
            assert got.shape == want.shape and np.array_equal(got, want), (case, name, tag, int((got != want).sum()))
            got = np.fromfile("%s_%s_acc.bin" % (stem, tag), dtype)
            assert np.array_equal(got, res0 + want), (case, name, tag, "accumulating")
    for case in R.CASES:
        nx, ny, L, wavelet, levels = case
        if nx * ny > 4096:
            continue
        for a, alpha in enumerate(ALPHAS):
            want_rows, want_cols = R.sums(nx, ny, 1, wavelet, levels, alpha)
            tol_rows, tol_cols = R.sums_tolerance(nx, ny, wavelet, levels, alpha)
            for tag, want, tol in (("rowsum", want_rows, tol_rows), ("colsum", want_cols, tol_cols)):
                got = np.fromfile(os.path.join(str(tmp_path), "%s_%s_%d.bin" % (R.case_id(case), tag, a)), np.float64)
                assert got.shape == want.shape and np.all(np.abs(got - want) <= tol), (case, alpha, tag, float((np.abs(got - want) / tol).max()))
