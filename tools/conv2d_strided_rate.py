"""Throughput of prost.block.conv2d_strided (prost_amd/csrc/kernels_linop_conv2d_strided.hip) against prost.block.sparse of its own matrix
and against prost.block.conv2d with the same window on the same source, in one process.
nx x ny pixels (default 1024 x 1024), L = 3, shape "same", a 9 x 9 Gaussian window rounded to fp32 (one matrix serves both precisions),
factor 2 and 4, fp32 and fp64, forward and adjoint.

Two kinds of rows, each saying how it was measured:
  * `chain`: the kernels through the C ABI, `chain` launches back to back between two host synchronisations, divided by `chain`; the
    candidates (strided forward, strided adjoint, conv2d forward, conv2d adjoint) alternate inside a round, and the best of `reps`
    rounds after a warm-up round counts (the launch latency is amortised, not removed); plain form.  Compulsory bytes:
    (rows + cols) sizeof(T) of the operator in question (rhs in, res out), and the time per compulsory byte beside it.  The forward
    product at stride s reads the bytes conv2d reads and writes 1 / (sy sx) of its outputs.  At this size the vectors fit in the
    last-level cache, so these are warm-cache figures.
  * `eval_linop`: the block and the sparse twin through prost.eval_linop, whose time is the mean of 5 products with a host
    synchronisation after each (launch latency included, first product included); the two alternate, best of `reps` calls (of two for the twin, whose set-up takes seconds per call).
usage: python tools/conv2d_strided_rate.py [nx ny] [reps] [chain] [twin: 1 or 0]"""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import conv2d_reference as R1  # noqa: E402
import conv2d_strided_reference as R  # noqa: E402
import prost_amd as prost  # noqa: E402
from prost_amd import _hip  # noqa: E402

nx = int(sys.argv[1]) if len(sys.argv) > 2 else 1024
ny = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
chain = int(sys.argv[4]) if len(sys.argv) > 4 else 10
with_twin = (int(sys.argv[5]) if len(sys.argv) > 5 else 1) != 0
L, SHAPE = 3, "same"

_hip.require_device()
prost.set_gpu(0)
rng = np.random.default_rng(21)
k = R.gauss(9, 2.25).astype(np.float32).astype(np.float64)
ky, kx = k.shape
SIG = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]


def rounds(calls):
    """{name: call} -> {name: best seconds per launch}; the candidates alternate inside a round, the first round warms up"""
    best = {}
    for r in range(reps + 1):
        for name, call in calls.items():
            _hip.sync()
            t0 = time.perf_counter()
            for _ in range(chain):
                _hip.check(call())
            _hip.sync()
            t = (time.perf_counter() - t0) / chain
            if r > 0:
                best[name] = min(best.get(name, t), t)
    return best


for factor in (2, 4):
    stride = (factor, factor)
    (my, mx), _, _ = R.output_size(nx, ny, ky, kx, SHAPE, stride)
    nrows, ncols = L * my * mx, L * nx * ny
    twin = None
    if with_twin:
        t0 = time.perf_counter()
        twin = [prost.block.sparse(R.matrix(nx, ny, L, k, SHAPE, stride))(0, 0, nrows, ncols)[0]]
        print("twin       factor %d: %d entries, built on the host in %.1f s" % (factor, twin[0][3][0].nnz, time.perf_counter() - t0), flush=True)
    for dtype in (np.float32, np.float64):
        name, item = np.dtype(dtype).name, np.dtype(dtype).itemsize
        fn, fn1 = _hip.fn("conv2d_strided", dtype), _hip.fn("conv2d", dtype)
        for f in (fn, fn1):
            f.argtypes, f.restype = SIG, C.c_int
        x = {False: rng.standard_normal(ncols).astype(dtype), True: rng.standard_normal(nrows).astype(dtype)}
        d_x = {t: _hip.DeviceArray.from_host(v) for t, v in x.items()}
        d_r = {False: _hip.DeviceArray.zeros(nrows, dtype), True: _hip.DeviceArray.zeros(ncols, dtype)}
        d_full = _hip.DeviceArray.zeros(ncols, dtype)            # conv2d "same": ncols outputs and ncols inputs in both directions
        calls, keep, taps = {}, [], 0
        for transpose in (False, True):
            geometry, table, ntaps = R.abi_records(nx, ny, L, k, SHAPE, stride, (0, 0), transpose, dtype)
            d_t = _hip.DeviceArray.from_host(table)
            keep += [geometry, d_t]
            taps = ntaps
            # a spot check before any timing: the first plane against the restatement
            _hip.check(fn(geometry.ctypes.data_as(C.c_void_p), d_t.ptr, ntaps, d_r[transpose].ptr, d_x[transpose].ptr, 0, None))
            _hip.sync()
            n_in, n_out = (my * mx, nx * ny) if transpose else (nx * ny, my * mx)
            assert np.array_equal(d_r[transpose].to_host()[:n_out], R.product(x[transpose][:n_in], nx, ny, 1, k, SHAPE, stride, (0, 0), transpose, dtype)), "the kernel disagrees with the restatement"
            calls["strided " + ("adjoint" if transpose else "forward")] = (lambda g=geometry, t=d_t, n=ntaps, tr=transpose: fn(g.ctypes.data_as(C.c_void_p), t.ptr, n, d_r[tr].ptr, d_x[tr].ptr, 0, None))
            g1, t1, n1 = R1.abi_records(nx, ny, L, k, SHAPE, transpose, dtype)
            d_t1 = _hip.DeviceArray.from_host(t1)
            keep += [g1, d_t1]
            calls["conv2d  " + ("adjoint" if transpose else "forward")] = (lambda g=g1, t=d_t1, n=n1: fn1(g.ctypes.data_as(C.c_void_p), t.ptr, n, d_full.ptr, d_x[False].ptr, 0, None))
        best = rounds(calls)
        for cname, t in best.items():
            nbytes = (2 * ncols if cname.startswith("conv2d") else nrows + ncols) * item
            print("chain      factor %d %s %d taps %s: %.4f ms, %.1f MB compulsory, %.3f ps per compulsory byte (%.1f %% of 8 TB/s)"
                  % (factor, name, taps, cname, t * 1e3, nbytes / 1e6, t / nbytes * 1e12, 100 * nbytes / t / 8e12), flush=True)
        for d in ("forward", "adjoint"):
            print("chain      factor %d %s %s: strided / conv2d %.2f" % (factor, name, d, best["strided " + d] / best["conv2d  " + d]), flush=True)
        for v in list(d_x.values()) + list(d_r.values()) + [d_full] + [v for v in keep if isinstance(v, _hip.DeviceArray)]:
            v.free()
        prost.set_precision("single" if dtype == np.float32 else "double")
        block = [prost.block.conv2d_strided(nx, ny, L, k, stride, SHAPE)(0, 0, nrows, ncols)[0]]
        for transpose in (False, True):
            tb, ts, diff = [], [], 0.0
            for _ in range(reps):
                out_b = prost.eval_linop(block, x[transpose], transpose)
                tb.append(float(out_b[3]))
                if twin is not None and len(ts) < 2:          # the twin is set up anew for every call: two calls
                    out_s = prost.eval_linop(twin, x[transpose], transpose)
                    ts.append(float(out_s[3]))
                    diff = float(np.abs(np.asarray(out_b[0]).ravel() - np.asarray(out_s[0]).ravel()).max())
            line = "eval_linop factor %d %s %-7s: block %.4f ms" % (factor, name, "adjoint" if transpose else "forward", min(tb))
            if ts:
                line += ", sparse twin %.4f ms: block / twin %.3f, largest difference of the results %.3g" % (min(ts), min(tb) / min(ts), diff)
            print(line, flush=True)
prost.set_precision("double")
