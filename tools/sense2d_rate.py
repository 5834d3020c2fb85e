"""Throughput of prost.block.sense2d (prost_amd/csrc/kernels_linop_sense2d.hip) against the cheapest unfused chain the tree could run, in
one process.  The chain has two parts, both timed in the same rounds as the block: (i) prost_hip_fft2d on the L C images, and (ii) a
device copy of the bytes a separate pointwise pass would move -- forward 2 L N + 2 C N values read and 2 L C N written, transposed
2 L C N + 2 C N read and 2 L N written.  The comparator is their sum.
Sizes: 256 x 256 x 8 coils, 512 x 512 x 8, 512 x 512 x 32, 2048 x 2048 x 4, L = 1 in fp32, and 512 x 512 x 8 in fp64; forward and transposed.

Windows of `chain` launches back to back between two host synchronisations, divided by `chain`; `reps` such windows after a warm-up
window; block, fft2d, pointwise copy and a copy of the block's own compulsory bytes (rhs in, maps in, res out) alternately in every
round.  Reported: the median window and the spread (max - min) / median of the windows; the workgroups of the coil-summing pass, and for
the transposed product the same windows with the small tile and with fft2d's tile choice forced through the record's tile selector.
`not slower beyond the spread` holds unless the block's fastest window is above the slowest sum of the chain's windows of the same
round.  Condition, set in advance: at 512 x 512 x 8 and 2048 x 2048 x 4 in fp32 the block is not slower than that sum, in both
directions; exit status 1 otherwise.  At 256 x 256 the launches are short and no threshold is set.
usage: python tools/sense2d_rate.py [reps] [chain]"""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import fft2d_reference as F  # noqa: E402
import sense2d_reference as R  # noqa: E402
import prost_amd as prost  # noqa: E402
from prost_amd import _hip  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
chain = int(sys.argv[2]) if len(sys.argv) > 2 else 30
PEAK = 8e12
SIZES = [(256, 256, 1, 8, np.float32), (512, 512, 1, 8, np.float32), (512, 512, 1, 32, np.float32), (2048, 2048, 1, 4, np.float32), (512, 512, 1, 8, np.float64)]
CONDITION = {(512, 8, "float32"), (2048, 4, "float32")}

_hip.require_device()
prost.set_gpu(0)
rng = np.random.default_rng(33)
memcpy = _hip.lib().prost_hip_memcpy_d2d
memcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
memcpy.restype = C.c_int


def window(call):
    _hip.sync()
    t0 = time.perf_counter()
    for _ in range(chain):
        call()
    _hip.sync()
    return (time.perf_counter() - t0) / chain


def alternately(calls):
    """-> per call the windows of `reps` rounds after a warm-up round"""
    times = [[] for _ in calls]
    for r in range(reps + 1):
        for k, call in enumerate(calls):
            t = window(call)
            if r:
                times[k].append(t)
    return [np.array(t) for t in times]


def spread(t):
    return (max(t) - min(t)) / float(np.median(t))


def sum_pass_workgroups(nx, ny, L, dtype, slab=0):
    """the grid of the coil-summing pass: the x pass (the y pass when nx = 1); slab 0: the library's tile choice (the small tile up to
    nx = 512), 1: the small tile, 2: fft2d's choice (the small tile up to nx = 128)"""
    if nx == 1:
        m, lines, tile = ny, 1, 2048
    else:
        small = slab == 1 or nx <= (512 if slab == 0 else 128)
        m, lines, tile = nx, ny, (2048 if small else 32768 // np.dtype(dtype).itemsize)
    return lines // min(tile // m, lines) * L


missed = []
for nx, ny, L, Cn, dtype in SIZES:
    item = np.dtype(dtype).itemsize
    case = (nx, ny, L, Cn)
    N = nx * ny
    rows, cols = R.sizes(case)
    sense = _hip.fn("sense2d", dtype)
    sense.argtypes = [C.c_void_p] * 6 + [C.c_int, C.c_void_p]
    fft = _hip.fn("fft2d", dtype)
    fft.argtypes = [C.c_void_p] * 5 + [C.c_int, C.c_void_p]
    sense.restype = fft.restype = C.c_int
    maps = R.make_maps(case)
    x = {False: rng.standard_normal(cols).astype(dtype), True: rng.standard_normal(rows).astype(dtype)}
    d_x = {t: _hip.DeviceArray.from_host(v) for t, v in x.items()}
    d_r = {False: _hip.DeviceArray.zeros(rows, dtype), True: _hip.DeviceArray.zeros(cols, dtype)}
    d_maps = _hip.DeviceArray.from_host(R.rounded(maps, dtype).reshape(-1))
    d_table = _hip.DeviceArray.from_host(np.ascontiguousarray(F.table(max(nx, ny), dtype)).reshape(-1))
    d_work, d_work2, d_out = _hip.DeviceArray.zeros(rows, dtype), _hip.DeviceArray.zeros(rows, dtype), _hip.DeviceArray.zeros(rows, dtype)
    d_copy = _hip.DeviceArray.zeros(2 * rows + 2 * Cn * N, dtype)
    keep = list(d_x.values()) + list(d_r.values()) + [d_maps, d_table, d_work, d_work2, d_out, d_copy]
    for transpose in (False, True):
        g_s, g_f = R.abi_record(case, transpose), F.abi_record(nx, ny, L * Cn, transpose)
        # values the separate pointwise pass would read and write; the block's own compulsory values
        read, written = (2 * L * N + 2 * Cn * N, rows) if not transpose else (rows + 2 * Cn * N, 2 * L * N)
        point = (read + written) * item // 2 // 16 * 16                       # the copy reads `point` bytes and writes as many
        own = (rows + cols + 2 * Cn * N) * item // 2 // 16 * 16

        def block():
            _hip.check(sense(g_s.ctypes.data_as(C.c_void_p), d_table.ptr, d_maps.ptr, d_work.ptr, d_r[transpose].ptr, d_x[transpose].ptr, 0, None))

        def block_with(slab):
            rec = R.abi_record(case, transpose, slab)
            return lambda: _hip.check(sense(rec.ctypes.data_as(C.c_void_p), d_table.ptr, d_maps.ptr, d_work.ptr, d_r[transpose].ptr, d_x[transpose].ptr, 0, None))

        def transform():
            _hip.check(fft(g_f.ctypes.data_as(C.c_void_p), d_table.ptr, d_work2.ptr, d_out.ptr, d_x[True].ptr, 0, None))

        def pointwise():
            _hip.check(memcpy(d_copy.ptr, d_copy.offset(point // item), point, None))

        def copy():
            _hip.check(memcpy(d_copy.ptr, d_copy.offset(own // item), own, None))

        # a spot check before any timing, where the restatement is quick
        block()
        _hip.sync()
        assert N > 512 * 512 or Cn > 8 or np.array_equal(d_r[transpose].to_host(), R.product(x[transpose], case, maps, transpose, dtype)), "the kernel disagrees with the restatement"
        t_b, t_f, t_p, t_c, t_small, t_fft = alternately([block, transform, pointwise, copy, block_with(1), block_with(2)])
        t_k = t_f + t_p                                                       # the chain, round by round
        m_b, m_f, m_p, m_k, m_c = (float(np.median(t)) for t in (t_b, t_f, t_p, t_k, t_c))
        ok = not min(t_b) > max(t_k)
        if (nx, Cn, np.dtype(dtype).name) in CONDITION and not ok:
            missed.append((nx, ny, Cn, np.dtype(dtype).name, "transposed" if transpose else "forward"))
        print("%dx%dx%d coils %s %-10s: block %.4f ms (spread %.1f %%) | fft2d on %d images %.4f ms (%.1f %%) + pointwise copy of %.1f MB %.4f ms (%.1f %%) = %.4f ms: chain / block %.2f, "
              "%s | copy of its own %.1f MB %.4f ms (%.1f %%) = %.1f %% of 8 TB/s: block / copy %.2f | coil-summing pass: %d workgroups"
              % (nx, ny, Cn, np.dtype(dtype).name, "transposed" if transpose else "forward", m_b * 1e3, 100 * spread(t_b), L * Cn, m_f * 1e3, 100 * spread(t_f), 2 * point / 1e6,
                 m_p * 1e3, 100 * spread(t_p), m_k * 1e3, m_k / m_b, "not slower than the chain beyond the spread" if ok else "SLOWER than the chain beyond the spread", 2 * own / 1e6,
                 m_c * 1e3, 100 * spread(t_c), 100 * 2 * own / m_c / PEAK, m_b / m_c, sum_pass_workgroups(nx, ny, L, dtype)), flush=True)
        if transpose:
            print("    tile of the coil-summing pass: small tile (%d workgroups) %.4f ms (spread %.1f %%), fft2d's choice (%d workgroups) %.4f ms (spread %.1f %%)"
                  % (sum_pass_workgroups(nx, ny, L, dtype, 1), float(np.median(t_small)) * 1e3, 100 * spread(t_small), sum_pass_workgroups(nx, ny, L, dtype, 2), float(np.median(t_fft)) * 1e3,
                     100 * spread(t_fft)), flush=True)
    for v in keep:
        v.free()
if missed:
    print("the block is SLOWER than fft2d plus the pointwise copy beyond the spread at: %s" % (missed,))
    sys.exit(1)
print("at 512 x 512 x 8 and 2048 x 2048 x 4 in fp32 the block is not slower than fft2d plus the pointwise copy, in both directions")
