"""Throughput of prost.block.hessian2d (prost_amd/csrc/kernels_linop_hessian2d.hip) against three yardsticks that run none of its code, in
one process: (i) prost.block.sparse of its own matrix, (ii) the two existing blocks chained -- prost_hip_grad2d_fwd then
prost_hip_linop_sym_gradient2d, and the latter's adjoint then prost_hip_grad2d_adj, through an intermediate field of 2 L N values --
and (iii) a plain device copy of the block's compulsory bytes.
Sizes: 1024 x 1024 (4 L N values = 17 / 50 MB: warm-cache figures) and 4096 x 4096 (268 / 805 MB, beyond the 256 MiB last-level cache:
HBM figures), L = 1 and 3, fp32, components = 3 with w = sqrt(1/2) and components = 4 with w = 0.5.

Two kinds of rows, each saying how it was measured:
  * `chain`: the kernels through the C ABI, `chain` launches back to back between two host synchronisations, divided by `chain`; `reps`
    such windows after a warm-up window, block, chained blocks and copy alternately in every round; reported: the median window, and the
    spread (max - min) / median of the windows.  Compulsory bytes of the block: (1 + components) L N sizeof(T) (rhs in, res out), reported
    as a fraction of the 8 TB/s HBM peak; the chained blocks move 8 L N values (3 + 5), the copy reads one half of the block's bytes
    and writes the other.  `faster than the chain beyond the spread` holds when the block's slowest window is below the chain's fastest.
  * `eval_linop`: the block and the sparse twin through prost.eval_linop, whose time is the mean of 5 products with a host
    synchronisation after each (launch latency included, first product included); the twin is built where nx ny L <= `twin_limit`
    (13 entries per pixel and channel, once for each side: the 4096 x 4096 twins are not built by default).
Exit status 1 if the block is not faster than the chained blocks beyond the spread at 4096 x 4096.
usage: python tools/hessian2d_rate.py [reps] [chain] [twin_limit]"""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hessian2d_reference as R  # noqa: E402
import prost_amd as prost  # noqa: E402
from prost_amd import _hip  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
chain = int(sys.argv[2]) if len(sys.argv) > 2 else 50
twin_limit = int(sys.argv[3]) if len(sys.argv) > 3 else 1024 * 1024 * 3
PEAK = 8e12
dtype, item = np.float32, 4
SIZES = [(n, n, L) for n in (1024, 4096) for L in (1, 3)]
VARIANTS = [(3, R.W_FROB), (4, R.W_HALF)]

_hip.require_device()
prost.set_gpu(0)
prost.set_precision("single")
rng = np.random.default_rng(32)
memcpy = _hip.lib().prost_hip_memcpy_d2d
memcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
memcpy.restype = C.c_int
hess = _hip.fn("hessian2d", dtype)
hess.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_double, C.c_int, C.c_int, C.c_int, C.c_void_p]
sym = _hip.fn("linop_sym_gradient2d", dtype)
sym.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_double, C.c_int, C.c_int, C.c_void_p]
grad = {False: _hip.fn("grad2d_fwd", dtype), True: _hip.fn("grad2d_adj", dtype)}
for g in grad.values():
    g.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_void_p]
for f in [hess, sym] + list(grad.values()):
    f.restype = C.c_int


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
    return times


def spread(t):
    return (max(t) - min(t)) / float(np.median(t))


slower = []
for nx, ny, L in SIZES:
    N = nx * ny
    for components, w in VARIANTS:
        nrows, ncols = components * L * N, L * N
        x = {False: rng.standard_normal(ncols).astype(dtype), True: rng.standard_normal(nrows).astype(dtype)}
        d_x = {t: _hip.DeviceArray.from_host(v) for t, v in x.items()}
        d_r = {False: _hip.DeviceArray.zeros(nrows, dtype), True: _hip.DeviceArray.zeros(ncols, dtype)}
        d_mid = _hip.DeviceArray.zeros(2 * L * N, dtype)                      # the chain's intermediate field
        d_e = _hip.DeviceArray.zeros(3 * L * N, dtype)                        # the chain's 3 L N side (components = 4 would add a pass; it is timed at 3)
        nbytes = (nrows + ncols) * item
        half = (nbytes // 2) // 16 * 16
        d_c = _hip.DeviceArray.zeros(2 * (half // item), dtype)
        kind = "warm cache" if nbytes < (256 << 20) else "HBM"
        for transpose in (False, True):
            def block():
                _hip.check(hess(d_r[transpose].ptr, d_x[transpose].ptr, nx, ny, L, w, components, int(transpose), 0, None))

            def chained():
                if not transpose:
                    _hip.check(grad[False](d_mid.ptr, d_x[False].ptr, nx, ny, L, 0, 0, None))
                    _hip.check(sym(d_e.ptr, d_mid.ptr, nx, ny, L, w, 0, 0, None))
                else:
                    _hip.check(sym(d_mid.ptr, d_e.ptr, nx, ny, L, w, 1, 0, None))
                    _hip.check(grad[True](d_r[True].ptr, d_mid.ptr, nx, ny, L, 0, 0, None))

            def copy():
                _hip.check(memcpy(d_c.ptr, d_c.offset(half // item), half, None))

            # a spot check before any timing: the whole product against the restatement (the large sizes are the tests' business)
            block()
            _hip.sync()
            assert N > 1024 * 1024 or np.array_equal(d_r[transpose].to_host(), R.product(x[transpose], nx, ny, L, w, components, transpose, dtype)), "the kernel disagrees with the restatement"
            t_b, t_k, t_c = alternately([block, chained, copy])
            m_b, m_k, m_c = (float(np.median(t)) for t in (t_b, t_k, t_c))
            beyond = max(t_b) < min(t_k)
            if N > 1024 * 1024 and not beyond:
                slower.append((ny, nx, L, components, transpose))
            print("chain      %dx%dx%d c%d %-7s (%s): block %.4f ms (spread %.1f %%), %.1f MB compulsory = %.1f %% of 8 TB/s | chained blocks %.4f ms (spread %.1f %%): chain / block %.2f, "
                  "%s | copy of the same bytes %.4f ms (spread %.1f %%) = %.1f %% of 8 TB/s: block / copy %.2f"
                  % (ny, nx, L, components, "adjoint" if transpose else "forward", kind, m_b * 1e3, 100 * spread(t_b), nbytes / 1e6, 100 * nbytes / m_b / PEAK, m_k * 1e3, 100 * spread(t_k),
                     m_k / m_b, "faster than the chain beyond the spread" if beyond else "NOT faster than the chain beyond the spread", m_c * 1e3, 100 * spread(t_c),
                     100 * 2 * half / m_c / PEAK, m_b / m_c), flush=True)
        for v in list(d_x.values()) + list(d_r.values()) + [d_mid, d_e, d_c]:
            v.free()
        if N * L > twin_limit:
            continue
        blk = [prost.block.hessian2d(nx, ny, L, R.weight(w, dtype), components)(0, 0, nrows, ncols)[0]]
        t0 = time.perf_counter()
        twin = [prost.block.sparse(R.matrix(nx, ny, L, w, components, dtype))(0, 0, nrows, ncols)[0]]
        print("twin       %dx%dx%d c%d: %d entries, built on the host in %.1f s" % (ny, nx, L, components, twin[0][3][0].nnz, time.perf_counter() - t0), flush=True)
        for transpose in (False, True):
            out_b = prost.eval_linop(blk, x[transpose], transpose)
            out_s = prost.eval_linop(twin, x[transpose], transpose)
            diff = float(np.abs(np.asarray(out_b[0]).ravel() - np.asarray(out_s[0]).ravel()).max())
            print("eval_linop %dx%dx%d c%d %-7s: block %.4f ms, sparse twin %.4f ms: twin / block %.1f, largest difference of the results %.3g"
                  % (ny, nx, L, components, "adjoint" if transpose else "forward", float(out_b[3]), float(out_s[3]), float(out_s[3]) / float(out_b[3]), diff), flush=True)
prost.set_precision("double")
if slower:
    print("the block is NOT faster than the chained blocks beyond the spread at: %s" % (slower,))
    sys.exit(1)
print("at 4096 x 4096 the block is faster than the chained blocks beyond the spread in every case")
