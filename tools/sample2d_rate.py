"""Time per forward and per adjoint product of prost.block.sample2d (prost_amd/csrc/kernels_linop_sample2d.hip), and at 1024 x 1024 the
sparse twin of its own matrix on the same GPU in the same process.
Workloads, L = 1, fp32 and fp64:
  * `flow`:    a warp by a smooth flow of at most 5 pixels (the shape of synthetic.warp_matrix), M = N, at 1024 x 1024 and 2048 x 2048;
  * `zoom`:    a 2x zoom of a 1024 x 1024 image, M = 4 N samples on a grid of half-pixel steps: four samples in most cells;
  * `scatter`: M = N samples at uniformly random positions of a 1024 x 1024 image: neighbouring samples are unrelated pixels.

Two kinds of rows, each saying how it was measured:
  * `chain`: the kernels through the C ABI, plain form.  One sample is `chain` launches back to back between two host synchronisations,
    divided by `chain` (the launch latency is amortised, not removed); forward and adjoint alternate inside a round; after one warm-up
    round `reps` rounds give the median, the smallest and the largest sample.  Beside it: the matrix entries per second, the device
    bytes of the block (2 M values of T, M int32, (ny + 1)(nx + 1) + 1 int32) and of a sparse twin (one value of T and one int32 per
    entry and side, plus the row pointers).  The vectors of 1024 x 1024 fit in the L2 and those of 2048 x 2048 in the last-level cache,
    so these are warm-cache figures.
  * `eval_linop`: the block and the sparse twin through prost.eval_linop, whose time is the mean of 5 products with a host
    synchronisation after each (launch latency included, first product included); the two alternate, median of `reps` calls for the
    block and of three for the twin.  Only the flow at 1024 x 1024.
usage: python tools/sample2d_rate.py [reps] [chain] [twin: 1 or 0] [largest size: 256, 1024 or 2048]"""
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sample2d_reference as R  # noqa: E402
import prost_amd as prost  # noqa: E402
from prost_amd import _hip  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
chain = int(sys.argv[2]) if len(sys.argv) > 2 else 20
with_twin = (int(sys.argv[3]) if len(sys.argv) > 3 else 1) != 0
largest = int(sys.argv[4]) if len(sys.argv) > 4 else 2048
SIG = [C.c_void_p] * 7 + [C.c_int, C.c_void_p]

_hip.require_device()
prost.set_gpu(0)
rng = np.random.default_rng(24)


def workload(kind, size):
    if kind == "flow":
        return R.positions("flow", size, size, size * size, 0)
    if kind == "zoom":
        g = (np.arange(2 * size) + 0.5) / 2.0 - 0.5
        return np.repeat(g, 2 * size), np.tile(g, 2 * size)
    return rng.uniform(0.0, size - 1.0, size * size), rng.uniform(0.0, size - 1.0, size * size)


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


WORK = [w for w in (("flow", 256), ("flow", 1024), ("flow", 2048), ("zoom", 1024), ("scatter", 1024)) if w[1] <= largest and (w[1] > 256 or largest == 256)]
for kind, size in WORK:
    nx = ny = size
    xs, ys = workload(kind, size)
    m, n = len(xs), nx * ny
    for dtype in (np.float32, np.float64):
        name, item = np.dtype(dtype).name, np.dtype(dtype).itemsize
        fn = _hip.fn("sample2d", dtype)
        fn.argtypes, fn.restype = SIG, C.c_int
        order, cell_start = R.buckets(nx, ny, xs, ys, dtype)
        entries = len(R.entries(nx, ny, xs, ys, dtype)[0])
        block_bytes = 2 * m * item + 4 * m + 4 * cell_start.size
        twin_bytes = 2 * entries * (item + 4) + 4 * (m + 1) + 4 * (n + 1)
        x = {False: rng.standard_normal(n).astype(dtype), True: rng.standard_normal(m).astype(dtype)}
        d_x = {t: _hip.DeviceArray.from_host(v) for t, v in x.items()}
        d_r = {False: _hip.DeviceArray.zeros(m, dtype), True: _hip.DeviceArray.zeros(n, dtype)}
        d_t = [_hip.DeviceArray.from_host(np.ascontiguousarray(t)) for t in (xs.astype(dtype), ys.astype(dtype), order, cell_start)]
        calls, keep = {}, []
        for transpose in (False, True):
            geometry = R.abi_records(nx, ny, 1, m, transpose)
            keep.append(geometry)
            args = lambda g=geometry, tr=transpose: (g.ctypes.data_as(C.c_void_p), d_t[0].ptr, d_t[1].ptr, d_t[2].ptr, d_t[3].ptr, d_r[tr].ptr, d_x[tr].ptr, 0, None)  # noqa: E731
            if size <= 1024 and kind == "flow":    # a spot check before any timing: the product against the restatement
                _hip.check(fn(*args()))
                _hip.sync()
                assert np.array_equal(d_r[transpose].to_host(), R.product(x[transpose], nx, ny, 1, xs, ys, transpose, dtype)), "the kernel disagrees with the restatement"
            calls["adjoint" if transpose else "forward"] = (lambda a=args: fn(*a()))
        for cname, s in rounds(calls).items():
            med = statistics.median(s)
            print("chain      %-7s %4d^2 M = %8d %s %s: median %.4f ms (%.4f .. %.4f over %d samples of %d launches), %.1f G entries/s; device bytes: block %.1f MB, sparse twin %.1f MB"
                  % (kind, size, m, name, cname, med * 1e3, min(s) * 1e3, max(s) * 1e3, len(s), chain, entries / med / 1e9, block_bytes / 1e6, twin_bytes / 1e6), flush=True)
        for v in list(d_x.values()) + list(d_r.values()) + d_t:
            v.free()
        if (kind, size) != ("flow", min(1024, largest)):
            continue
        prost.set_precision("single" if dtype == np.float32 else "double")
        block = [prost.block.sample2d(nx, ny, 1, xs, ys)(0, 0, m, n)[0]]
        twin = None
        if with_twin:
            t0 = time.perf_counter()
            K = R.matrix(nx, ny, 1, xs, ys, dtype)
            twin = [prost.block.sparse(K)(0, 0, m, n)[0]]
            print("twin       %-7s %4d^2 %s: %d entries, built on the host in %.1f s" % (kind, size, name, K.nnz, time.perf_counter() - t0), flush=True)
        for transpose in (False, True):
            tb, ts, diff = [], [], 0.0
            for _ in range(reps):
                out_b = prost.eval_linop(block, x[transpose], transpose)
                tb.append(float(out_b[3]))
                if twin is not None and len(ts) < 3:          # the twin is set up anew for every call: three calls
                    out_s = prost.eval_linop(twin, x[transpose], transpose)
                    ts.append(float(out_s[3]))
                    diff = float(np.abs(np.asarray(out_b[0]).ravel() - np.asarray(out_s[0]).ravel()).max())
            line = "eval_linop %-7s %4d^2 %s %-7s: block median %.4f ms (%.4f .. %.4f)" % (kind, size, name, "adjoint" if transpose else "forward", statistics.median(tb), min(tb), max(tb))
            if ts:
                line += ", sparse twin %.4f ms (%.4f .. %.4f): block / twin %.3f, largest difference of the results %.3g" % (statistics.median(ts), min(ts), max(ts), statistics.median(tb) / statistics.median(ts), diff)
            print(line, flush=True)
prost.set_precision("double")
