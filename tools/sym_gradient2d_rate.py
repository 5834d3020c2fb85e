"""Throughput of prost.block.sym_gradient2d (prost_amd/csrc/kernels_linop_sym_gradient2d.hip) against the gradient2d vector kernels on
the same image and against prost.block.sparse of its own matrix, in one process.
Sizes: 1024 x 1024 x 3 in fp32 and fp64 (5 N L values = 63 / 126 MB: both vectors fit in the 256 MiB last-level cache, warm-cache
figures) and 4096 x 4096 x 1 in fp32 (5 N values = 335 MB, beyond the cache: an HBM figure).  w = sqrt(1/2).

Two kinds of rows, each saying how it was measured:
  * `chain`: the kernel through the C ABI, `chain` launches back to back between two host synchronisations, divided by `chain`, best of
    `reps` rounds after a warm-up round (the launch latency is amortised, not removed); plain form.  Compulsory bytes:
    (rows + cols) sizeof(T) (rhs in, res out), reported as a fraction of the 8 TB/s HBM peak.  Beside it prost_hip_grad2d_fwd / _adj on
    the same image (3 N L values), measured the same way and alternately with the block: the yardstick is time per compulsory byte.
  * `eval_linop`: the block and the sparse twin through prost.eval_linop, whose time is the mean of 5 products with a host
    synchronisation after each (launch latency included, first product included); the twin is built where nx ny L <= `twin_limit`.
usage: python tools/sym_gradient2d_rate.py [reps] [chain] [twin_limit]"""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import prost_amd as prost  # noqa: E402
import sym_gradient2d_reference as R  # noqa: E402
from prost_amd import _hip  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
chain = int(sys.argv[2]) if len(sys.argv) > 2 else 10
twin_limit = int(sys.argv[3]) if len(sys.argv) > 3 else 1024 * 1024 * 3
PEAK = 8e12
W = R.W_FROB
SIZES = [(1024, 1024, 3, np.float32, "warm cache"), (1024, 1024, 3, np.float64, "warm cache"), (4096, 4096, 1, np.float32, "HBM")]

_hip.require_device()
prost.set_gpu(0)
rng = np.random.default_rng(19)


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


for nx, ny, L, dtype, kind in SIZES:
    name, item = np.dtype(dtype).name, np.dtype(dtype).itemsize
    N = nx * ny
    nrows, ncols = 3 * L * N, 2 * L * N
    fn = _hip.fn("linop_sym_gradient2d", dtype)
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_double, C.c_int, C.c_int, C.c_void_p]
    fn.restype = C.c_int
    grad = {}
    for t, which in ((False, "grad2d_fwd"), (True, "grad2d_adj")):
        grad[t] = _hip.fn(which, dtype)
        grad[t].argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_void_p]
        grad[t].restype = C.c_int
    x = {False: rng.standard_normal(ncols).astype(dtype), True: rng.standard_normal(nrows).astype(dtype)}
    d_x = {t: _hip.DeviceArray.from_host(v) for t, v in x.items()}
    d_r = {False: _hip.DeviceArray.zeros(nrows, dtype), True: _hip.DeviceArray.zeros(ncols, dtype)}
    for transpose in (False, True):
        # a spot check before any timing: the whole product against the restatement
        _hip.check(fn(d_r[transpose].ptr, d_x[transpose].ptr, nx, ny, L, W, int(transpose), 0, None))
        _hip.sync()
        assert np.array_equal(d_r[transpose].to_host(), R.product(x[transpose], nx, ny, L, W, transpose, dtype)), "the kernel disagrees with the restatement"
        # gradient2d on the same image: forward reads N L and writes 2 N L, the adjoint the other way round (both buffers are large enough)
        g_res, g_rhs = (d_r[False], d_x[False]) if not transpose else (d_r[True], d_x[True])
        t_b, t_g = [], []
        for _ in range(2):                  # alternately
            t_b.append(timed(lambda: fn(d_r[transpose].ptr, d_x[transpose].ptr, nx, ny, L, W, int(transpose), 0, None)))
            t_g.append(timed(lambda: grad[transpose](g_res.ptr, g_rhs.ptr, nx, ny, L, 0, 0, None)))
        t_b, t_g = min(t_b), min(t_g)
        nbytes, gbytes = (nrows + ncols) * item, 3 * L * N * item
        print("chain      %s %dx%dx%d %-7s (%s): %.4f ms, %.1f MB compulsory = %.1f %% of 8 TB/s, %.3f ps/byte | gradient2d: %.4f ms, %.1f MB = %.1f %% of 8 TB/s, %.3f ps/byte | per byte, block / gradient2d %.2f"
              % (name, ny, nx, L, "adjoint" if transpose else "forward", kind, t_b * 1e3, nbytes / 1e6, 100 * nbytes / t_b / PEAK, 1e12 * t_b / nbytes,
                 t_g * 1e3, gbytes / 1e6, 100 * gbytes / t_g / PEAK, 1e12 * t_g / gbytes, (t_b / nbytes) / (t_g / gbytes)), flush=True)
    for v in list(d_x.values()) + list(d_r.values()):
        v.free()
    prost.set_precision("single" if dtype == np.float32 else "double")
    block = [prost.block.sym_gradient2d(nx, ny, L, R.weight(W, dtype))(0, 0, nrows, ncols)[0]]
    twin = None
    if N * L <= twin_limit:
        t0 = time.perf_counter()
        twin = [prost.block.sparse(R.matrix(nx, ny, L, W, dtype))(0, 0, nrows, ncols)[0]]
        print("twin       %s %dx%dx%d: %d entries, built on the host in %.1f s" % (name, ny, nx, L, twin[0][3][0].nnz, time.perf_counter() - t0), flush=True)
    for transpose in (False, True):
        out_b = prost.eval_linop(block, x[transpose], transpose)
        line = "eval_linop %s %dx%dx%d %-7s: block %.4f ms" % (name, ny, nx, L, "adjoint" if transpose else "forward", float(out_b[3]))
        if twin is not None:
            out_s = prost.eval_linop(twin, x[transpose], transpose)
            diff = float(np.abs(np.asarray(out_b[0]).ravel() - np.asarray(out_s[0]).ravel()).max())
            line += ", sparse twin %.4f ms: block / twin %.3f, largest difference of the results %.3g" % (float(out_s[3]), float(out_b[3]) / float(out_s[3]), diff)
        print(line, flush=True)
prost.set_precision("double")
