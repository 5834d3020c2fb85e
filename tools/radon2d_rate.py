"""Time per forward and per adjoint product of prost.block.radon2d (prost_amd/csrc/kernels_linop_radon2d.hip), and at the smallest size
the sparse twin of its own matrix on the same GPU in the same process.
Sizes: 256 x 256 from 180 angles, 512 x 512 from 360 and 1024 x 1024 from 720, evenly over [0, pi), default detector, spacing 1, L = 1,
fp32 and fp64.

Two kinds of rows, each saying how it was measured:
  * `chain`: the kernels through the C ABI, plain form.  One sample is `chain` launches back to back between two host synchronisations,
    divided by `chain` (the launch latency is amortised, not removed); forward and adjoint alternate inside a round; after one warm-up
    round `reps` rounds give the median, the smallest and the largest sample.  Beside it: the matrix entries per second (two per ray
    and driving line inside the image, counted by formula: the work the product does) and what a CSR twin would have to move for them, 8 bytes (fp32; 12 for fp64) per entry.
    At these sizes the image and the sinogram fit in the L2, so these are warm-cache figures.
  * `eval_linop`: the block and the sparse twin through prost.eval_linop, whose time is the mean of 5 products with a host
    synchronisation after each (launch latency included, first product included); the two alternate, median of `reps` calls for the
    block and of three for the twin, whose set-up takes seconds per call.  Only at 256 x 256 / 180 (21 million entries).
usage: python tools/radon2d_rate.py [reps] [chain] [twin: 1 or 0] [largest size: 256, 512 or 1024]"""
import ctypes as C
import math
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import radon2d_reference as R  # noqa: E402
import prost_amd as prost  # noqa: E402
from prost_amd import _hip  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
chain = int(sys.argv[2]) if len(sys.argv) > 2 else 20
with_twin = (int(sys.argv[3]) if len(sys.argv) > 3 else 1) != 0
largest = int(sys.argv[4]) if len(sys.argv) > 4 else 1024
SIZES = [(n, a) for n, a in ((256, 180), (512, 360), (1024, 720)) if n <= largest]
SIG = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]

_hip.require_device()
prost.set_gpu(0)
rng = np.random.default_rng(23)


def rounds(calls):
    """{name: call} -> {name: samples in seconds per launch}; the candidates alternate inside a round, the first round warms up"""
    samples = {name: [] for name in calls}
    for r in range(reps + 1):
        for name, call in calls.items():
            _hip.sync()
            t0 = time.perf_counter()
            for _ in range(chain):
                _hip.check(call())
            _hip.sync()
            if r > 0:
                samples[name].append((time.perf_counter() - t0) / chain)
    return samples


for size, na in SIZES:
    nx = ny = size
    angles = np.arange(na) * (math.pi / na)
    ndet = R.default_ndet(nx, ny, 1.0)
    nrows, ncols = na * ndet, nx * ny
    # two entries per ray and driving line inside the image: a driving line of n pixels meets n / |q| rays, |q| = 1 / max(|cos|, |sin|)
    entries = int(2 * nx * ny * np.maximum(np.abs(np.cos(angles)), np.abs(np.sin(angles))).sum())
    for dtype in (np.float32, np.float64):
        name, item = np.dtype(dtype).name, np.dtype(dtype).itemsize
        fn = _hip.fn("radon2d", dtype)
        fn.argtypes, fn.restype = SIG, C.c_int
        table = R.table(nx, ny, angles, ndet, 1.0, 0.0, dtype)
        x = {False: rng.standard_normal(ncols).astype(dtype), True: rng.standard_normal(nrows).astype(dtype)}
        d_x = {t: _hip.DeviceArray.from_host(v) for t, v in x.items()}
        d_r = {False: _hip.DeviceArray.zeros(nrows, dtype), True: _hip.DeviceArray.zeros(ncols, dtype)}
        d_t = _hip.DeviceArray.from_host(np.ascontiguousarray(table).ravel())
        calls, keep = {}, []
        for transpose in (False, True):
            geometry = R.abi_records(nx, ny, 1, angles, ndet, 1.0, transpose)
            keep.append(geometry)
            if size == 256:                        # a spot check before any timing: the product against the restatement
                _hip.check(fn(geometry.ctypes.data_as(C.c_void_p), d_t.ptr, d_r[transpose].ptr, d_x[transpose].ptr, 0, None))
                _hip.sync()
                assert np.array_equal(d_r[transpose].to_host(), R.product(x[transpose], nx, ny, 1, angles, ndet, 1.0, 0.0, transpose, dtype)), "the kernel disagrees with the restatement"
            calls["adjoint" if transpose else "forward"] = (lambda g=geometry, tr=transpose: fn(g.ctypes.data_as(C.c_void_p), d_t.ptr, d_r[tr].ptr, d_x[tr].ptr, 0, None))
        for cname, s in rounds(calls).items():
            med = statistics.median(s)
            print("chain      %4d^2 / %3d %s %s: median %.4f ms (%.4f .. %.4f over %d samples of %d launches), %.1f G entries/s, a CSR twin would move %.0f MB: %.2f TB/s"
                  % (size, na, name, cname, med * 1e3, min(s) * 1e3, max(s) * 1e3, len(s), chain, entries / med / 1e9, entries * (4 + item) / 1e6, entries * (4 + item) / med / 1e12), flush=True)
        for v in list(d_x.values()) + list(d_r.values()) + [d_t]:
            v.free()
        if size != 256:
            continue
        prost.set_precision("single" if dtype == np.float32 else "double")
        block = [prost.block.radon2d(nx, ny, 1, angles, ndet)(0, 0, nrows, ncols)[0]]
        twin = None
        if with_twin:
            t0 = time.perf_counter()
            K = R.matrix(nx, ny, 1, angles, ndet, 1.0, 0.0, dtype)
            twin = [prost.block.sparse(K)(0, 0, nrows, ncols)[0]]
            print("twin       %4d^2 / %3d %s: %d entries, %.0f MB as CSR, built on the host in %.1f s" % (size, na, name, K.nnz, K.nnz * (4 + item) / 1e6, time.perf_counter() - t0), flush=True)
        for transpose in (False, True):
            tb, ts, diff = [], [], 0.0
            for _ in range(reps):
                out_b = prost.eval_linop(block, x[transpose], transpose)
                tb.append(float(out_b[3]))
                if twin is not None and len(ts) < 3:          # the twin is set up anew for every call: three calls
                    out_s = prost.eval_linop(twin, x[transpose], transpose)
                    ts.append(float(out_s[3]))
                    diff = float(np.abs(np.asarray(out_b[0]).ravel() - np.asarray(out_s[0]).ravel()).max())
            line = "eval_linop %4d^2 / %3d %s %-7s: block median %.4f ms (%.4f .. %.4f)" % (size, na, name, "adjoint" if transpose else "forward", statistics.median(tb), min(tb), max(tb))
            if ts:
                line += ", sparse twin %.4f ms (%.4f .. %.4f): block / twin %.3f, largest difference of the results %.3g" % (statistics.median(ts), min(ts), max(ts), statistics.median(tb) / statistics.median(ts), diff)
            print(line, flush=True)
prost.set_precision("double")
