"""Time per forward and per adjoint product of prost.block.fanbeam2d (prost_amd/csrc/kernels_linop_fanbeam2d.hip) against three
baselines on the same GPU in the same process, by the method of tools/radon2d_rate.py:
  * radon2d (prost_amd/csrc/kernels_linop_radon2d.hip) at the same nx, ny, views and ndet;
  * a device-to-device copy of the block's compulsory bytes, one image plus one sinogram (half of them read, half written);
  * at 256 x 256 from 180 views the sparse twin of the block's own matrix through prost.eval_linop (larger twins take minutes to set up).
Sizes: 512 x 512 from 360 views and 1024 x 1024 from 720 (and 256 x 256 from 180 for the twin), evenly over a full turn, the source at
three half diagonals, D = R, default detector, spacing 1, L = 1, flat, fp32 and fp64.

Two kinds of rows, each saying how it was measured:
  * `chain`: the kernels through the C ABI, plain form.  One sample is `chain` launches back to back between two host synchronisations,
    divided by `chain`; the candidates (fan forward, fan adjoint, radon forward, radon adjoint, copy) alternate inside a round; after
    one warm-up round `reps` rounds give the median, the smallest and the largest sample.  Beside each fan row its ratio to the radon
    row (the target of docs/rounds/r34.md is 1.5) and to the copy.
  * `eval_linop`: the block and the sparse twin through prost.eval_linop, whose time is the mean of 5 products with a host
    synchronisation after each; the two alternate, median of `reps` calls for the block and of three for the twin.
usage: python tools/fanbeam2d_rate.py [reps] [chain] [twin: 1 or 0] [largest size: 256, 512 or 1024] [detector: flat or curved]"""
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
import fanbeam2d_reference as F  # noqa: E402
import radon2d_reference as R  # noqa: E402
import prost_amd as prost  # noqa: E402
from prost_amd import _hip  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
chain = int(sys.argv[2]) if len(sys.argv) > 2 else 20
with_twin = (int(sys.argv[3]) if len(sys.argv) > 3 else 1) != 0
largest = int(sys.argv[4]) if len(sys.argv) > 4 else 1024
detector = sys.argv[5] if len(sys.argv) > 5 else "flat"
SIZES = [(n, a) for n, a in ((256, 180), (512, 360), (1024, 720)) if n <= largest and (n > 256 or with_twin)]
SIG = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]

_hip.require_device()
prost.set_gpu(0)
rng = np.random.default_rng(34)
copy = _hip.lib().prost_hip_memcpy_d2d
copy.argtypes, copy.restype = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p], C.c_int


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
    angles = np.arange(na) * (2 * math.pi / na)
    dist = 3.0 * F.half_diagonal(nx, ny)
    ndet = F.default_ndet(nx, ny, dist, dist, 1.0, detector == "curved")
    args = (nx, ny, 1, angles, dist, dist, ndet, 1.0, 0.0, detector)
    nrows, ncols = na * ndet, nx * ny
    for dtype in (np.float32, np.float64):
        name, item = np.dtype(dtype).name, np.dtype(dtype).itemsize
        fan, radon = _hip.fn("fanbeam2d", dtype), _hip.fn("radon2d", dtype)
        fan.argtypes, fan.restype, radon.argtypes, radon.restype = SIG, C.c_int, SIG, C.c_int
        x = {False: rng.standard_normal(ncols).astype(dtype), True: rng.standard_normal(nrows).astype(dtype)}
        d_x = {t: _hip.DeviceArray.from_host(v) for t, v in x.items()}
        d_r = {False: _hip.DeviceArray.zeros(nrows, dtype), True: _hip.DeviceArray.zeros(ncols, dtype)}
        d_fan = _hip.DeviceArray.from_host(F.table(nx, ny, angles, dist, dist, ndet, 1.0, 0.0, detector, dtype))
        d_radon = _hip.DeviceArray.from_host(np.ascontiguousarray(R.table(nx, ny, angles, ndet, 1.0, 0.0, dtype)).ravel())
        half = (nrows + ncols) // 2
        d_a, d_b = _hip.DeviceArray.zeros(half, dtype), _hip.DeviceArray.zeros(half, dtype)
        calls, keep = {}, []
        for transpose in (False, True):
            gf, gr = F.abi_records(*args, transpose), R.abi_records(nx, ny, 1, angles, ndet, 1.0, transpose)
            keep += [gf, gr]
            if size == 256:                          # a spot check before any timing: the product against the restatement
                _hip.check(fan(gf.ctypes.data_as(C.c_void_p), d_fan.ptr, d_r[transpose].ptr, d_x[transpose].ptr, 0, None))
                _hip.sync()
                assert np.array_equal(d_r[transpose].to_host(), F.product(x[transpose], *args, transpose, dtype)), "the kernel disagrees with the restatement"
            way = "adjoint" if transpose else "forward"
            calls["fan " + way] = (lambda g=gf, tr=transpose: fan(g.ctypes.data_as(C.c_void_p), d_fan.ptr, d_r[tr].ptr, d_x[tr].ptr, 0, None))
            calls["radon " + way] = (lambda g=gr, tr=transpose: radon(g.ctypes.data_as(C.c_void_p), d_radon.ptr, d_r[tr].ptr, d_x[tr].ptr, 0, None))
        calls["copy"] = lambda: copy(d_b.ptr, d_a.ptr, half * item, None)
        med = {}
        got = rounds(calls)
        for cname, s in got.items():
            med[cname] = statistics.median(s)
        for cname, s in got.items():
            line = "chain      %4d^2 / %3d x %d %s %s %-14s: median %.4f ms (%.4f .. %.4f over %d samples of %d launches)" % (size, na, ndet, detector, name, cname, med[cname] * 1e3,
                                                                                                                         min(s) * 1e3, max(s) * 1e3, len(s), chain)
            if cname.startswith("fan "):
                line += ", %.2f x radon2d, %.1f x the copy of %.1f MB" % (med[cname] / med["radon " + cname[4:]], med[cname] / med["copy"], 2 * half * item / 1e6)
            print(line, flush=True)
        for v in list(d_x.values()) + list(d_r.values()) + [d_fan, d_radon, d_a, d_b]:
            v.free()
        if size != 256:
            continue
        prost.set_precision("single" if dtype == np.float32 else "double")
        block = [prost.block.fanbeam2d(*args)(0, 0, nrows, ncols)[0]]
        t0 = time.perf_counter()
        K = F.matrix(*args, dtype)
        twin = [prost.block.sparse(K)(0, 0, nrows, ncols)[0]]
        print("twin       %4d^2 / %3d %s: %d entries, %.0f MB as CSR, built on the host in %.1f s" % (size, na, name, K.nnz, K.nnz * (4 + item) / 1e6, time.perf_counter() - t0), flush=True)
        for transpose in (False, True):
            tb, ts, diff = [], [], 0.0
            for _ in range(reps):
                out_b = prost.eval_linop(block, x[transpose], transpose)
                tb.append(float(out_b[3]))
                if len(ts) < 3:                              # the twin is set up anew for every call: three calls
                    out_s = prost.eval_linop(twin, x[transpose], transpose)
                    ts.append(float(out_s[3]))
                    diff = float(np.abs(np.asarray(out_b[0]).ravel() - np.asarray(out_s[0]).ravel()).max())
            print("eval_linop %4d^2 / %3d %s %-7s: block median %.4f ms (%.4f .. %.4f), sparse twin %.4f ms (%.4f .. %.4f): block / twin %.3f, largest difference of the results %.3g"
                  % (size, na, name, "adjoint" if transpose else "forward", statistics.median(tb), min(tb), max(tb), statistics.median(ts), min(ts), max(ts),
                     statistics.median(tb) / statistics.median(ts), diff), flush=True)
prost.set_precision("double")
