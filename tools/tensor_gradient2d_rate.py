"""Throughput of prost.block.tensor_gradient2d (prost_amd/csrc/kernels_linop_tensor_gradient2d.hip) against a plain device copy of the
same number of bytes and against prost.block.sparse of its own matrix, in one process.
Sizes: 1024 x 1024 and 4096 x 4096, L = 1 and 3, k = 1 and 3, fp32 and fp64, forward and adjoint.  At 1024^2 the compulsory bytes (17 to 101 MB) fit in the
256 MiB last-level cache (warm-cache figures); at 4096^2 they are 268 MB to 1.6 GB (HBM figures; the smallest is exactly the cache's size
and a copy of it still runs above the HBM peak).

Two kinds of rows, each saying how it was measured:
  * `chain`: the kernel through the C ABI, `chain` launches back to back between two host synchronisations, divided by `chain`, best of
    `reps` rounds after a warm-up round (the launch latency is amortised, not removed); plain form.  Compulsory bytes:
    (3 L + k) N sizeof(T) -- u in, gx and gy out (or the other way round), the tensor once -- and the byte model of a workgroup that
    fetches the tensor for its own channel, (3 + k) L N sizeof(T); both as a fraction of the 8 TB/s HBM peak.  Beside it
    prost_hip_memcpy_d2d of half the compulsory bytes (it reads and writes them: the same traffic), measured the same way and
    alternately with the block.
  * `eval_linop`: the block and the sparse twin through prost.eval_linop, whose time is the mean of 5 products with a host
    synchronisation after each (launch latency included, first product included); the twin is built where nx ny L <= `twin_limit`
    (its matrix has 4 L N entries at k = 1 and 6 L N at k = 3, built by scipy on the host).
usage: python tools/tensor_gradient2d_rate.py [reps] [chain] [twin_limit]"""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import prost_amd as prost  # noqa: E402
import tensor_gradient2d_reference as R  # noqa: E402
from prost_amd import _hip  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
chain = int(sys.argv[2]) if len(sys.argv) > 2 else 10
twin_limit = int(sys.argv[3]) if len(sys.argv) > 3 else 1024 * 1024 * 3
PEAK = 8e12
SIZES = [(n, n, L, dtype) for n in (1024, 4096) for dtype in (np.float32, np.float64) for L in (1, 3)]

_hip.require_device()
prost.set_gpu(0)
rng = np.random.default_rng(29)
memcpy = _hip.lib().prost_hip_memcpy_d2d
memcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
memcpy.restype = C.c_int


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


for nx, ny, L, dtype in SIZES:
    name, item = np.dtype(dtype).name, np.dtype(dtype).itemsize
    N = nx * ny
    nrows, ncols = 2 * L * N, L * N
    fn = _hip.fn("linop_tensor_gradient2d", dtype)
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_void_p]
    fn.restype = C.c_int
    x = {False: rng.standard_normal(ncols).astype(dtype), True: rng.standard_normal(nrows).astype(dtype)}
    d_x = {t: _hip.DeviceArray.from_host(v) for t, v in x.items()}
    d_r = {False: _hip.DeviceArray.zeros(nrows, dtype), True: _hip.DeviceArray.zeros(ncols, dtype)}
    mid = (3 * L + 3) * N // 2 // 4 * 4                                   # the copy's two halves: room for the bytes of k = 3
    d_c = _hip.DeviceArray.zeros(2 * mid, dtype)
    prost.set_precision("single" if dtype == np.float32 else "double")
    for k in (1, 3):
        planes = R.rounded(R.random_tensor(nx, ny, k, 100 + k), dtype)
        d_t = _hip.DeviceArray.from_host(np.concatenate(planes).astype(dtype))
        for transpose in (False, True):
            # a spot check before any timing: the whole product against the restatement (the large sizes are the tests' business)
            _hip.check(fn(d_r[transpose].ptr, d_x[transpose].ptr, d_t.ptr, nx, ny, L, k, int(transpose), 0, None))
            _hip.sync()
            assert N > 1024 * 1024 or np.array_equal(d_r[transpose].to_host(), R.product(x[transpose], nx, ny, L, planes, transpose, dtype)), "the kernel disagrees with the restatement"
            nbytes, model = (3 * L + k) * N * item, (3 + k) * L * N * item
            kind = "warm cache" if nbytes < (256 << 20) else "HBM"
            half = (nbytes // 2) // 16 * 16
            assert half <= mid * item
            t_b, t_c = [], []
            for _ in range(2):                  # alternately
                t_b.append(timed(lambda: fn(d_r[transpose].ptr, d_x[transpose].ptr, d_t.ptr, nx, ny, L, k, int(transpose), 0, None)))
                t_c.append(timed(lambda: memcpy(d_c.ptr, d_c.offset(mid), half, None)))
            t_b, t_c = min(t_b), min(t_c)
            print("chain      %s %dx%dx%d k=%d %-7s (%s): %.4f ms, %.1f MB compulsory = %.1f %% of 8 TB/s (tensor per channel: %.1f MB = %.1f %%) | copy of the same bytes: %.4f ms = %.1f %% | block / copy %.2f"
                  % (name, ny, nx, L, k, "adjoint" if transpose else "forward", kind, t_b * 1e3, nbytes / 1e6, 100 * nbytes / t_b / PEAK, model / 1e6, 100 * model / t_b / PEAK,
                     t_c * 1e3, 100 * 2 * half / t_c / PEAK, t_b / t_c), flush=True)
        d_t.free()
        if N * L > twin_limit:
            continue
        block = [prost.block.tensor_gradient2d(nx, ny, L, planes)(0, 0, nrows, ncols)[0]]
        t0 = time.perf_counter()
        twin = [prost.block.sparse(R.matrix(nx, ny, L, planes, dtype))(0, 0, nrows, ncols)[0]]
        print("twin       %s %dx%dx%d k=%d: %d entries, built on the host in %.1f s" % (name, ny, nx, L, k, twin[0][3][0].nnz, time.perf_counter() - t0), flush=True)
        for transpose in (False, True):
            out_b = prost.eval_linop(block, x[transpose], transpose)
            line = "eval_linop %s %dx%dx%d k=%d %-7s: block %.4f ms" % (name, ny, nx, L, k, "adjoint" if transpose else "forward", float(out_b[3]))
            out_s = prost.eval_linop(twin, x[transpose], transpose)
            diff = float(np.abs(np.asarray(out_b[0]).ravel() - np.asarray(out_s[0]).ravel()).max())
            print(line + ", sparse twin %.4f ms: twin / block %.1f, largest difference of the results %.3g" % (float(out_s[3]), float(out_s[3]) / float(out_b[3]), diff), flush=True)
    for v in list(d_x.values()) + list(d_r.values()) + [d_c]:
        v.free()
prost.set_precision("double")
