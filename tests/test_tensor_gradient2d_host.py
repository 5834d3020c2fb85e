"""The arithmetic of tensor_gradient2d on the host, under AddressSanitizer and UndefinedBehaviorSanitizer:
tests/host/tensor_gradient2d_harness.cpp is a stand-alone program (plain g++, no HIP, nothing preloaded) that runs
include/prost/linop/tensor_gradient2d.hpp -- the term functions, the forward and the adjoint march that
prost_amd/csrc/kernels_linop_tensor_gradient2d.hip calls in every lane, and the sums of the host block -- for fp32 and fp64, every mode
k = 1, 2, 3, forward and adjoint, plain and accumulating, at every case of tests/tensor_gradient2d_reference.py, against exactly sized
buffers.  The main run uses the strip and chunk geometry of the kernels (lanes of 16 bytes where the height allows, strips of 256 lanes,
chunks of PickColumns columns); inside the harness every other lane width, narrow strips and forced chunk widths have to give the same
bits.  Its outputs are compared here bit for bit with the NumPy restatement (b), and its row and column sums (cases up to 4096 pixels,
alpha = 1 and 0.5) with the sums (c) of the explicit matrix: equal for the dyadic tensors at alpha = 1, within (t + 8) eps_T otherwise."""
import os
import re

import numpy as np

import host_harness
import tensor_gradient2d_reference as R

ALPHAS = (1.0, 0.5)
PRECISIONS = (("fp32", np.float32), ("fp64", np.float64))


def test_header_under_sanitizers_bit_for_bit_with_the_restatement(tmp_path):
    d = str(tmp_path)
    inputs, lines = {}, []
    for case in R.CASES:
        ny, nx, L = case
        N = nx * ny
        lines.append("%s %d %d %d %d" % (R.case_id(case), nx, ny, L, N <= 4096))
        for name, dtype in PRECISIONS:
            rng = np.random.default_rng(R.case_seed(case, 5))
            arrays = dict(rhs=rng.standard_normal(L * N).astype(dtype), rhst=rng.standard_normal(2 * L * N).astype(dtype),
                          res0=rng.standard_normal(2 * L * N).astype(dtype), res0t=rng.standard_normal(L * N).astype(dtype))
            stem = os.path.join(d, "%s_%s" % (R.case_id(case), name))
            for key, v in arrays.items():
                v.tofile("%s_%s.bin" % (stem, key))
            for k in R.MODES:
                planes = R.tensor_for(case, k)
                np.concatenate(planes).astype(dtype).tofile("%s_k%d_tensor.bin" % (stem, k))
            inputs[(case, name)] = (stem, dtype, arrays)
    with open(os.path.join(d, "cases.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    stdout = host_harness.run_sanitized("tensor_gradient2d_harness", tmp_path, args=[d])
    out = stdout.strip().splitlines()
    assert out[-1] == "ok" and "FAIL" not in stdout and "%d cases" % len(R.CASES) in out
    ran = [l for l in out if re.search(r" fp(32|64) k=[123]: \d+ values, W = [124], forward and adjoint, plain and accumulating, every geometry the same bits$", l)]
    assert len(ran) == 2 * 3 * len(R.CASES)
    # the main run is the geometry of the kernels: 16 bytes per lane where the height allows, one row otherwise
    assert any(l.startswith("1024x3x1 fp32 k=3") and "W = 4" in l for l in ran) and any(l.startswith("1025x3x1 fp32 k=3") and "W = 1" in l for l in ran)
    assert any(l.startswith("514x3x1 fp64 k=1") and "W = 2" in l for l in ran) and any(l.startswith("514x3x1 fp32 k=1") and "W = 1" in l for l in ran)
    for (case, name), (stem, dtype, arrays) in inputs.items():
        ny, nx, L = case
        for k in R.MODES:
            planes = R.tensor_for(case, k)
            for transpose, tag, rhs, res0 in ((False, "fwd", arrays["rhs"], arrays["res0"]), (True, "adj", arrays["rhst"], arrays["res0t"])):
                want = R.product(rhs, nx, ny, L, planes, transpose, dtype)
                got = np.fromfile("%s_k%d_%s.bin" % (stem, k, tag), dtype)
                assert got.shape == want.shape and np.array_equal(got, want), (case, name, k, tag, int((got != want).sum()))
                got = np.fromfile("%s_k%d_%s_acc.bin" % (stem, k, tag), dtype)
                assert np.array_equal(got, res0 + want), (case, name, k, tag, "accumulating")
            if nx * ny > 4096:
                continue
            tol = (R.T_TERMS + 8) * np.finfo(dtype).eps
            dyadic = R.is_dyadic(case)
            for a, alpha in enumerate(ALPHAS):
                for tag, want in zip(("rowsum", "colsum"), R.sums(nx, ny, L, planes, alpha, dtype)):
                    got = np.fromfile("%s_k%d_%s_%d.bin" % (stem, k, tag, a), np.float64)
                    assert got.shape == want.shape and np.all(np.abs(got - want) <= tol * want), (case, name, k, alpha, tag)
                    if dyadic and alpha == 1.0:
                        assert np.array_equal(got, want), (case, name, k, tag)
