"""Throughput of prost.block.conv2d (prost_amd/csrc/kernels_linop_conv2d.hip) against prost.block.sparse of its own matrix and against a
plain diags product of the same byte count, in one process.
nx x ny pixels (default 1024 x 1024), L = 3, shape "full", fp32 and fp64, forward and adjoint; windows: the 15 x 15 motion window of
examples/deblurring.py (about 29 non-zero taps), a dense 5 x 5, a dense 15 x 15 and a dense 31 x 31 (standard normal, rounded to fp32
so that one matrix serves both precisions).

Two kinds of rows, each saying how it was measured:
  * `chain`: the kernel through the C ABI, `chain` launches back to back between two host synchronisations, divided by `chain`, best of
    `reps` rounds after a warm-up round (the launch latency is amortised, not removed); plain form.  Compulsory bytes:
    (rows + cols) sizeof(T) (rhs in, res out), reported as a fraction of the 8 TB/s HBM peak.  At this size both vectors fit in the
    last-level cache, so these are warm-cache figures.  Beside it prost_hip_diags_fwd with one diagonal on a vector sized to move the
    same bytes (it accumulates: three streams of n elements), measured the same way: the yardstick of what a plain streaming product
    of this library reaches.
  * `eval_linop`: the block and the sparse twin through prost.eval_linop, whose time is the mean of 5 products with a host
    synchronisation after each (launch latency included, first product included).  The twin is built for the windows named in
    `twins` (default motion,5x5: the dense 15 x 15 has 0.7 G entries per direction).
usage: python tools/conv2d_rate.py [nx ny] [reps] [chain] [twins, comma separated, or none]"""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "examples"))
import conv2d_reference as R  # noqa: E402
import prost_amd as prost  # noqa: E402
from deblurring import motion_kernel  # noqa: E402
from prost_amd import _hip  # noqa: E402

nx = int(sys.argv[1]) if len(sys.argv) > 2 else 1024
ny = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
chain = int(sys.argv[4]) if len(sys.argv) > 4 else 10
twins = (sys.argv[5] if len(sys.argv) > 5 else "motion,5x5").split(",")
PEAK = 8e12
L = 3
SHAPE = "full"

_hip.require_device()
prost.set_gpu(0)
rng = np.random.default_rng(18)
WINDOWS = [("motion", motion_kernel(15, 45.0)), ("5x5", rng.standard_normal((5, 5))), ("15x15", rng.standard_normal((15, 15))), ("31x31", rng.standard_normal((31, 31)))]
WINDOWS = [(name, k.astype(np.float32).astype(np.float64)) for name, k in WINDOWS]


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


for wname, k in WINDOWS:
    ky, kx = k.shape
    (my, mx), _ = R.output_size(nx, ny, ky, kx, SHAPE)
    nrows, ncols = L * my * mx, L * nx * ny
    twin = None
    if wname in twins:
        t0 = time.perf_counter()
        twin = [prost.block.sparse(R.matrix(nx, ny, L, k, SHAPE))(0, 0, nrows, ncols)[0]]
        print("twin       %s: %d entries, built on the host in %.1f s" % (wname, twin[0][3][0].nnz, time.perf_counter() - t0), flush=True)
    for dtype in (np.float32, np.float64):
        name = np.dtype(dtype).name
        item = np.dtype(dtype).itemsize
        fn = _hip.fn("conv2d", dtype)
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        fn.restype = C.c_int
        diags = _hip.fn("diags_fwd", dtype)
        diags.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
        diags.restype = C.c_int
        offsets = _hip.DeviceArray.from_host(np.zeros(1, np.int64))
        factors = _hip.DeviceArray.from_host(np.full(1, 0.5, np.float32))
        x = {False: rng.standard_normal(ncols).astype(dtype), True: rng.standard_normal(nrows).astype(dtype)}
        d_x = {t: _hip.DeviceArray.from_host(v) for t, v in x.items()}
        d_r = {False: _hip.DeviceArray.zeros(nrows, dtype), True: _hip.DeviceArray.zeros(ncols, dtype)}
        for transpose in (False, True):
            geometry, table, ntaps = R.abi_records(nx, ny, L, k, SHAPE, transpose, dtype)
            d_t = _hip.DeviceArray.from_host(table)
            gp = geometry.ctypes.data_as(C.c_void_p)
            # a spot check before any timing: the first plane against the restatement
            _hip.check(fn(gp, d_t.ptr, ntaps, d_r[transpose].ptr, d_x[transpose].ptr, 0, None))
            _hip.sync()
            n_in, n_out = (my * mx, nx * ny) if transpose else (nx * ny, my * mx)
            assert np.array_equal(d_r[transpose].to_host()[:n_out], R.product(x[transpose][:n_in], nx, ny, 1, k, SHAPE, transpose, dtype)), "the kernel disagrees with the restatement"
            t = timed(lambda: fn(gp, d_t.ptr, ntaps, d_r[transpose].ptr, d_x[transpose].ptr, 0, None))
            nbytes = (nrows + ncols) * item
            m = nbytes // (3 * item)                  # diags accumulates: rhs in, res in, res out
            t_d = timed(lambda: diags(d_r[False].ptr, d_x[True].ptr, m, m, 1, offsets.ptr, factors.ptr, None))
            print("chain      %s %-6s %3d taps %-7s: %.4f ms, %.1f MB compulsory = %.1f %% of 8 TB/s, %.1f G taps/s | diags, %d elements, same bytes: %.4f ms = %.1f %% of 8 TB/s | block / diags %.2f"
                  % (name, wname, ntaps, "adjoint" if transpose else "forward", t * 1e3, nbytes / 1e6, 100 * nbytes / t / PEAK,
                     ntaps * (ncols if transpose else nrows) / t / 1e9, m, t_d * 1e3, 100 * 3 * m * item / t_d / PEAK, t / t_d), flush=True)
            d_t.free()
        for v in list(d_x.values()) + list(d_r.values()) + [offsets, factors]:
            v.free()
        prost.set_precision("single" if dtype == np.float32 else "double")
        block = [prost.block.conv2d(nx, ny, L, k, SHAPE)(0, 0, nrows, ncols)[0]]
        for transpose in (False, True):
            out_b = prost.eval_linop(block, x[transpose], transpose)
            line = "eval_linop %s %-6s %-7s: block %.4f ms" % (name, wname, "adjoint" if transpose else "forward", float(out_b[3]))
            if twin is not None:
                out_s = prost.eval_linop(twin, x[transpose], transpose)
                diff = float(np.abs(np.asarray(out_b[0]).ravel() - np.asarray(out_s[0]).ravel()).max())
                line += ", sparse twin %.4f ms: block / twin %.3f, largest difference of the results %.3g" % (float(out_s[3]), float(out_b[3]) / float(out_s[3]), diff)
            print(line, flush=True)
prost.set_precision("double")
