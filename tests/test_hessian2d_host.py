"""The arithmetic of hessian2d on the host, under AddressSanitizer and UndefinedBehaviorSanitizer: tests/host/hessian2d_harness.cpp is a
stand-alone program (plain g++, no HIP) that runs include/prost/linop/hessian2d.hpp -- the two marches
prost_amd/csrc/kernels_linop_hessian2d.hip calls in every lane, and the closed-form sums of the host block -- strip by strip and chunk
by chunk in a plain loop, over the case list of tests/hessian2d_reference.py, every variant (components, w), fp32 and fp64:

  * both products, plain and accumulating, equal the NumPy restatement (b) bit for bit.  The harness cannot run NumPy and the arrays
    of the whole list are too large to hand over, so both sides build the input from the same generator (values(), Values() there)
    and the test hands over digest() of the bits of (b): a sum of bits[i] m[i] modulo 2^64 with odd m[i], which a change of any one
    element changes;
  * they equal the chain the harness writes from the two existing definitions -- a plain forward difference, then
    sym_gradient2d::Apply; sym_gradient2d::Apply transposed, then the plain adjoint difference -- bit for bit;
  * W = 2 and 4, narrow strips and forced chunk widths give the bits of W = 1;
  * RowSum / ColSum are within (7 + 8) eps_T of (c) for alpha = 1 and 0.5 (w = 0.5, alpha = 1: equal), at every case of up to 20000
    pixels (the closed forms do not know about chunks).
Every buffer has exactly its size."""
import re

import numpy as np

import hessian2d_reference as R
import host_harness

M1, M2, M3 = np.uint64(0x9E3779B97F4A7C15), np.uint64(0xBF58476D1CE4E5B9), np.uint64(0x94D049BB133111EB)


def mix(z):
    z = z * M1
    z = (z ^ (z >> np.uint64(30))) * M2
    z = (z ^ (z >> np.uint64(27))) * M3
    return z ^ (z >> np.uint64(31))


def values(seed, n):
    """n float64 values in [-2, 2), each a multiple of 2^-51: Values() of the harness before it rounds to T"""
    z = mix(np.arange(n, dtype=np.uint64) + np.uint64(seed))
    return ((z >> np.uint64(11)).astype(np.float64) * 2.0 ** -53 - 0.5) * 4.0


def digest(a):
    bits = a.view(np.uint32 if a.dtype == np.float32 else np.uint64).astype(np.uint64)
    return int((bits * (mix(np.arange(a.size, dtype=np.uint64)) | np.uint64(1))).sum(dtype=np.uint64))


def test_the_generator_and_the_digest():
    assert mix(np.array([1, 2], dtype=np.uint64)).tolist() == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4]      # splitmix64 from the state 0
    v = values(5, 1000)
    assert v.min() >= -2 and v.max() < 2 and np.array_equal(v * 2.0 ** 51, np.round(v * 2.0 ** 51)) and len(set(v)) == 1000
    a = v.astype(np.float32)
    b = a.copy()
    b[17] = np.nextafter(b[17], np.float32(3))
    assert digest(a) == digest(a.copy()) != digest(b) and digest(np.zeros(3)) == 0 and digest(-np.zeros(3)) != 0


def test_marches_and_sums_under_sanitizers(tmp_path):
    runs, records, expected = [], [], []
    for case in R.CASES:
        ny, nx, L = case
        N = nx * ny
        for components, w in R.VARIANTS:
            for is_double, dtype in ((0, np.float32), (1, np.float64)):
                for transpose in (0, 1):
                    nin, nout = (components * L * N, L * N) if transpose else (L * N, components * L * N)
                    seed_x, seed_r = R.case_seed(case, 1000 * components + transpose), R.case_seed(case, 7 + 1000 * components + transpose)
                    x, res0 = values(seed_x, nin).astype(dtype), values(seed_r, nout).astype(dtype)
                    plain = R.product(x, nx, ny, L, w, components, bool(transpose), dtype)
                    acc = R.product(x, nx, ny, L, w, components, bool(transpose), dtype, res0)
                    assert plain.dtype == acc.dtype == np.dtype(dtype) and plain.shape == acc.shape == (nout,)
                    runs.append("%d %d %d %d %d %d %s %d %d %d %d" % (ny, nx, L, components, transpose, is_double, float(w).hex(), seed_x, seed_r, digest(plain), digest(acc)))
                    expected.append("%dx%dx%d c%d w %.3f %s %s" % (ny, nx, L, components, w, "fp64" if is_double else "fp32", "adjoint" if transpose else "forward"))
                if N <= 20000:
                    for alpha in (1.0, 0.5):
                        rows, cols = R.sums(nx, ny, L, w, components, alpha, dtype)
                        records.append(np.concatenate([[ny, nx, L, components, is_double, w, alpha], rows, cols]))
    (tmp_path / "runs.txt").write_text("\n".join(runs) + "\n")
    np.concatenate(records).astype(np.float64).tofile(str(tmp_path / "sums.bin"))
    stdout = host_harness.run_sanitized("hessian2d_harness", tmp_path, [tmp_path / "runs.txt", tmp_path / "sums.bin"])
    lines = stdout.strip().splitlines()
    assert lines[-1] == "ok" and "FAIL" not in stdout
    assert lines[-2] == "%d products and %d records of sums" % (len(runs), len(records))
    got = [l for l in lines if l.endswith(": restatement, chain and every W equal")]
    assert [l.split(":")[0] for l in got] == expected
    assert len(runs) == 12 * len(R.CASES) and len(R.CASES) >= 30
    summed = [l for l in lines if re.match(r"\d+x\d+x\d+ c[34] w -?[0-9.]+ fp(32|64) sums alpha (1\.0|0\.5): equal$", l)]
    assert len(summed) == len(records) >= 12 * 20
