"""The arithmetic of sense2d on the host, under AddressSanitizer and UndefinedBehaviorSanitizer: tests/host/sense2d_harness.cpp is a
stand-alone program (plain g++, no HIP, nothing preloaded) that runs include/prost/linop/sense2d.hpp -- the complex products, the coil
sum and, through fft2d.hpp, the table, the tree, the passes and the scaling that prost_amd/csrc/kernels_linop_sense2d.hip and the host
block use -- for fp32 and fp64 at every case of tests/sense2d_reference.py, forward and transposed, plain and accumulating, against
exactly sized buffers.  It prints one digest per result, sum_i (bits_i + 0x9E3779B97F4A7C15) (2 i + 1) mod 2^64 over the bit patterns
with a zero of either sign taken as +0; the same digest of the NumPy restatement has to be equal: bit for bit."""
import os

import numpy as np

import host_harness
import sense2d_reference as R


def digest(a):
    a = np.ascontiguousarray(a)
    a = np.where(a == 0, a.dtype.type(0), a)
    bits = a.view(np.uint32 if a.dtype == np.float32 else np.uint64).astype(np.uint64)
    with np.errstate(over="ignore"):
        return int(((bits + np.uint64(0x9E3779B97F4A7C15)) * (2 * np.arange(bits.size, dtype=np.uint64) + np.uint64(1))).sum(dtype=np.uint64))


def test_digest_is_sensitive_to_a_bit_and_to_a_position_and_not_to_the_sign_of_a_zero():
    a = np.array([1.0, -0.0, 3.5, 0.0], np.float32)
    assert digest(a) == digest(np.array([1.0, 0.0, 3.5, -0.0], np.float32))
    assert digest(a) != digest(np.array([1.0, 0.0, np.nextafter(np.float32(3.5), np.float32(4)), 0.0], np.float32))
    assert digest(a) != digest(np.array([3.5, 0.0, 1.0, 0.0], np.float32))
    assert digest(np.array([1.0], np.float32)) == (0x3F800000 + 0x9E3779B97F4A7C15) % 2 ** 64


def test_header_under_sanitizers_bit_for_bit_with_the_restatement(tmp_path):
    want = {}
    for case in R.CASES:
        rows, cols = R.sizes(case)
        for name, dtype in (("fp32", np.float32), ("fp64", np.float64)):
            rng = np.random.default_rng(R.case_seed(case, 3))
            maps = R.make_maps(case, zeros=True)
            x, resx = rng.standard_normal(cols).astype(dtype), rng.standard_normal(cols).astype(dtype)
            y, resy = rng.standard_normal(rows).astype(dtype), rng.standard_normal(rows).astype(dtype)
            stem = os.path.join(str(tmp_path), "%s_%s" % (R.case_id(case), name))
            for tag, a in (("maps", R.rounded(maps, dtype)), ("x", x), ("resx", resx), ("y", y), ("resy", resy)):
                a.tofile("%s_%s.bin" % (stem, tag))
            fwd, inv = R.product(x, case, maps, False, dtype), R.product(y, case, maps, True, dtype)
            assert np.array_equal(R.product(x, case, maps, False, dtype, res0=resy), resy + fwd) and np.array_equal(R.product(y, case, maps, True, dtype, res0=resx), resx + inv)
            for tag, a in (("fwd", fwd), ("fwd_acc", resy + fwd), ("inv", inv), ("inv_acc", resx + inv)):
                assert a.dtype == dtype and np.isfinite(a).all()
                want["%s %s %s" % (R.case_id(case), name, tag)] = (a.size, digest(a))
    stdout = host_harness.run_sanitized("sense2d_harness", tmp_path, args=[str(tmp_path)])
    lines = stdout.strip().splitlines()
    assert lines[-1] == "ok" and "FAIL" not in stdout
    got = {}
    for line in lines[:-1]:
        case, name, tag, count, value = line.split()
        got["%s %s %s" % (case, name, tag)] = (int(count), int(value))
    assert sorted(got) == sorted(want) and len(got) == 8 * len(R.CASES)
    wrong = [k for k in want if got[k] != want[k]]
    assert not wrong, wrong
