"""Throughput of prost.block.dataterm_sublabel (prost_amd/csrc/kernels_linop_dataterm_sublabel.hip) against prost.block.sparse of its
own matrix and against a plain diags product of the same byte count, in one process.
nx x ny pixels (default 1024 x 1024), L = 4, 8 and 16, fp32 and fp64, forward and adjoint.

Two kinds of rows, each saying how it was measured:
  * `chain`: the kernel through the C ABI, `chain` launches back to back between two host synchronisations, divided by `chain`, best of
    `reps` rounds after a warm-up round (the launch latency is amortised, not removed); plain and accumulating.  Compulsory bytes:
    4 N k sizeof(T) (rhs in, res out), plus 2 N k sizeof(T) when accumulating (res in); reported as a fraction of the 8 TB/s HBM
    peak.  Beside it prost_hip_diags_fwd with one diagonal on a vector sized to move the same bytes (it accumulates: three streams of n
    elements), measured the same way: the yardstick of what a plain streaming product of this library reaches.
  * `eval_linop`: the block and the sparse twin through prost.eval_linop, whose time is the mean of 5 products with a host
    synchronisation after each (launch latency included, first product included).  The twin's matrix has 2 k + k (k + 1) / 2 entries per
    pixel.
usage: python tools/dataterm_sublabel_rate.py [nx ny] [reps] [chain] [largest L for the sparse twin]"""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dataterm_sublabel_reference as R  # noqa: E402
import prost_amd as prost  # noqa: E402
from prost_amd import _hip  # noqa: E402

nx = int(sys.argv[1]) if len(sys.argv) > 2 else 1024
ny = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
chain = int(sys.argv[4]) if len(sys.argv) > 4 else 10
sparse_max_L = int(sys.argv[5]) if len(sys.argv) > 5 else 16
PEAK = 8e12
LEFT, RIGHT = -0.3, 1.1
LABELS = (4, 8, 16)

_hip.require_device()
prost.set_gpu(0)
N = nx * ny


def timed(call):
    times = []
    for _ in range(reps + 1):              # the first round warms up
        _hip.sync()
        t0 = time.perf_counter()
        for _ in range(chain):
            _hip.check(call())
        _hip.sync()
        times.append((time.perf_counter() - t0) / chain)
    return min(times[1:])


for dtype in (np.float32, np.float64):
    name = np.dtype(dtype).name
    item = np.dtype(dtype).itemsize
    fn = _hip.fn("linop_dataterm_sublabel", dtype)
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_double, C.c_int, C.c_int, C.c_void_p]
    fn.restype = C.c_int
    diags = _hip.fn("diags_fwd", dtype)
    diags.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
    diags.restype = C.c_int
    offsets = _hip.DeviceArray.from_host(np.zeros(1, np.int64))
    factors = _hip.DeviceArray.from_host(np.full(1, 0.5, np.float32))
    for L in LABELS:
        k = L - 1
        n = 2 * N * k
        delta, gamma = R.labels(L, LEFT, RIGHT, dtype)
        rng = np.random.default_rng(L)
        x = rng.standard_normal(n).astype(dtype)
        rhs, res, g = _hip.DeviceArray.from_host(x), _hip.DeviceArray.zeros(n, dtype), _hip.DeviceArray.from_host(gamma)
        # a spot check before any timing: the first and the last plane pair against the restatement
        for transpose in (0, 1):
            _hip.check(fn(res.ptr, rhs.ptr, N, L, g.ptr, float(delta), transpose, 0, None))
            _hip.sync()
            assert np.array_equal(res.to_host(), R.product(x, N, L, LEFT, RIGHT, bool(transpose), dtype)), "the kernel disagrees with the restatement"
        for transpose in (0, 1):
            for acc in (0, 1):
                t = timed(lambda: fn(res.ptr, rhs.ptr, N, L, g.ptr, float(delta), transpose, acc, None))
                nbytes = (4 + 2 * acc) * N * k * item
                m = nbytes // (3 * item)                  # diags accumulates: rhs in, res in, res out
                t_d = timed(lambda: diags(res.ptr, rhs.ptr, m, m, 1, offsets.ptr, factors.ptr, None))
                print("chain      %s L=%-2d %-7s %-12s: %.4f ms, %.1f MB compulsory = %.1f %% of 8 TB/s | diags, %d elements, same bytes: %.4f ms = %.1f %% of 8 TB/s | block / diags %.2f"
                      % (name, L, "adjoint" if transpose else "forward", "accumulating" if acc else "plain", t * 1e3, nbytes / 1e6, 100 * nbytes / t / PEAK,
                         m, t_d * 1e3, 100 * 3 * m * item / t_d / PEAK, t / t_d), flush=True)
        for v in (rhs, res, g):
            v.free()
        prost.set_precision("single" if dtype == np.float32 else "double")
        block = [prost.block.dataterm_sublabel(nx, ny, L, LEFT, RIGHT)(0, 0, n, n)[0]]
        twin = [prost.block.sparse(R.matrix(nx, ny, L, LEFT, RIGHT, dtype))(0, 0, n, n)[0]] if L <= sparse_max_L else None
        for transpose in (False, True):
            out_b = prost.eval_linop(block, x, transpose)
            line = "eval_linop %s L=%-2d %-7s: block %.4f ms" % (name, L, "adjoint" if transpose else "forward", float(out_b[3]))
            if twin is not None:
                out_s = prost.eval_linop(twin, x, transpose)
                nnz = twin[0][3][0].nnz
                diff = float(np.abs(np.asarray(out_b[0]).ravel() - np.asarray(out_s[0]).ravel()).max())
                line += ", sparse twin (%d entries) %.4f ms: block / twin %.3f, largest difference of the results %.3g" % (nnz, float(out_s[3]), float(out_b[3]) / float(out_s[3]), diff)
            print(line, flush=True)
    offsets.free()
    factors.free()
prost.set_precision("double")
