"""Throughput of prost.block.nonlocal_gradient2d (prost_amd/csrc/kernels_linop_nonlocal_gradient2d.hip) against a plain device copy of the
same number of bytes and against prost.block.sparse of its own matrix, in one process.
Sizes: 1024 x 1024 and 4096 x 4096, M = 8 (the radius-1 window) and M = 24 (the radius-2 window), L = 1 and 3, fp32 and fp64, forward
and adjoint.  Compulsory bytes: (M + M L + L) N sizeof(T) -- the M weight planes once for all channels, the M L range planes, the L
domain planes; 71 MB to 0.83 GB at 1024^2 (the smallest fit in the 256 MiB last-level cache: warm-cache figures) and 1.1 to 13 GB at
4096^2 (HBM figures).  Beside it the byte model of a kernel that fetches the weights once per channel, (2 M L + L) N sizeof(T).

Two kinds of rows, each saying how it was measured:
  * `chain`: the kernel through the C ABI, `chain` launches back to back between two host synchronisations, divided by `chain`, best of
    `reps` rounds after a warm-up round (the launch latency is amortised, not removed); plain form.  Beside it prost_hip_memcpy_d2d of
    half the compulsory bytes (it reads and writes them: the same traffic), measured the same way and alternately with the block.
  * `eval_linop`: the block and the sparse twin through prost.eval_linop, whose time is the mean of 5 products with a host
    synchronisation after each (launch latency included, first product included); the twin is built where its 2 M L N entries are at
    most `twin_limit` (built by scipy on the host, which takes seconds).
Data: one random plane of 1024^2 values repeated; the values do not change what the kernels do.
usage: python tools/nonlocal_gradient2d_rate.py [reps] [chain] [twin_limit]"""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import prost_amd as prost  # noqa: E402
import nonlocal_gradient2d_reference as R  # noqa: E402
from prost_amd import _hip  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
chain = int(sys.argv[2]) if len(sys.argv) > 2 else 10
twin_limit = int(sys.argv[3]) if len(sys.argv) > 3 else 52 * 1024 * 1024
PEAK = 8e12
SIZES = [(n, n, L, dtype) for n in (1024, 4096) for dtype in (np.float32, np.float64) for L in (1, 3)]
WINDOWS = [R.window(1), R.window(2)]

_hip.require_device()
prost.set_gpu(0)
base = np.random.default_rng(30).standard_normal(1024 * 1024)
memcpy = _hip.lib().prost_hip_memcpy_d2d
memcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
memcpy.restype = C.c_int


def values(n, dtype, shift):
    return np.resize(np.roll(base, shift), n).astype(dtype)


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
    fn = _hip.fn("linop_nonlocal_gradient2d", dtype)
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, C.c_char_p, C.c_int, C.c_int, C.c_void_p]
    fn.restype = C.c_int
    prost.set_precision("single" if dtype == np.float32 else "double")
    for offsets in WINDOWS:
        M = len(offsets)
        pairs = np.array(offsets, dtype=np.int8).tobytes()
        nrows, ncols = M * L * N, L * N
        x = {False: values(ncols, dtype, 1), True: values(nrows, dtype, 2)}
        w = values(M * N, dtype, 3)
        d_x = {t: _hip.DeviceArray.from_host(v) for t, v in x.items()}
        d_r = {False: _hip.DeviceArray.zeros(nrows, dtype), True: _hip.DeviceArray.zeros(ncols, dtype)}
        d_w = _hip.DeviceArray.from_host(w)
        nbytes, model = (M + M * L + L) * N * item, (2 * M * L + L) * N * item
        half = (nbytes // 2) // 16 * 16
        d_c = _hip.DeviceArray.zeros(2 * (half // item), dtype)
        for transpose in (False, True):
            _hip.check(fn(d_r[transpose].ptr, d_x[transpose].ptr, d_w.ptr, nx, ny, L, M, pairs, int(transpose), 0, None))
            _hip.sync()
            if N <= 1024 * 1024 and L == 1 and M == 8:     # a spot check before any timing (the tests own the rest)
                want = R.product(x[transpose], nx, ny, L, offsets, [w[m * N:(m + 1) * N] for m in range(M)], transpose, dtype)
                assert np.array_equal(d_r[transpose].to_host(), want), "the kernel disagrees with the restatement"
            kind = "warm cache" if nbytes < (256 << 20) else "HBM"
            t_b, t_c = [], []
            for _ in range(2):                  # alternately
                t_b.append(timed(lambda: fn(d_r[transpose].ptr, d_x[transpose].ptr, d_w.ptr, nx, ny, L, M, pairs, int(transpose), 0, None)))
                t_c.append(timed(lambda: memcpy(d_c.ptr, d_c.offset(half // item), half, None)))
            t_b, t_c = min(t_b), min(t_c)
            print("chain      %s %dx%dx%d M=%d %-7s (%s): %.4f ms, %.1f MB compulsory = %.1f %% of 8 TB/s (weights per channel: %.1f MB = %.1f %%) | copy of the same bytes: %.4f ms = %.1f %% | block / copy %.2f"
                  % (name, ny, nx, L, M, "adjoint" if transpose else "forward", kind, t_b * 1e3, nbytes / 1e6, 100 * nbytes / t_b / PEAK, model / 1e6, 100 * model / t_b / PEAK,
                     t_c * 1e3, 100 * 2 * half / t_c / PEAK, t_b / t_c), flush=True)
        for v in list(d_x.values()) + list(d_r.values()) + [d_c, d_w]:
            v.free()
        if 2 * M * L * N > twin_limit:
            continue
        planes = [w[m * N:(m + 1) * N].astype(np.float64) for m in range(M)]
        block = [prost.block.nonlocal_gradient2d(nx, ny, L, offsets, planes)(0, 0, nrows, ncols)[0]]
        t0 = time.perf_counter()
        twin = [prost.block.sparse(R.matrix(nx, ny, L, offsets, planes, dtype))(0, 0, nrows, ncols)[0]]
        print("twin       %s %dx%dx%d M=%d: %d entries, built on the host in %.1f s" % (name, ny, nx, L, M, twin[0][3][0].nnz, time.perf_counter() - t0), flush=True)
        for transpose in (False, True):
            out_b = prost.eval_linop(block, x[transpose], transpose)
            line = "eval_linop %s %dx%dx%d M=%d %-7s: block %.4f ms" % (name, ny, nx, L, M, "adjoint" if transpose else "forward", float(out_b[3]))
            out_s = prost.eval_linop(twin, x[transpose], transpose)
            diff = float(np.abs(np.asarray(out_b[0]).ravel() - np.asarray(out_s[0]).ravel()).max())
            print(line + ", sparse twin %.4f ms: twin / block %.1f, largest difference of the results %.3g" % (float(out_s[3]), float(out_s[3]) / float(out_b[3]), diff), flush=True)
prost.set_precision("double")
