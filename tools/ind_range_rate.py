"""Times of ind_range (x = A (A'A)^-1 A' y; ProxIndRange) stage by stage, through the C ABI of the kernel library: t = A'y and x = A z
(prost_hip_csr_spmv_*), the dense solve (prost_hip_range_potrs_*, the plan's tier and -- where the size allows -- the other one) and
the one-off factorisation (prost_hip_range_potrf_*).  Protocol of tools/eigen_mass_rate.py: every figure is the best of `reps`
synchronous calls timed with a host clock (enqueue + wait: the launch latencies are inside; the large tier is a chain of dependent
launches, so that is what an evaluation costs).  The solve's effective rate counts n^2 sizeof(T) bytes: each sweep reads one triangle.
Where librocsolver.so loads, rocsolver_<t>potrs on the same factor is timed the same way as a yardstick for the solve stage alone (this
tool only; the product never links it).
usage: python tools/ind_range_rate.py [reps] [--rocsolver]"""
import ctypes as C
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from prost_amd import _hip  # noqa: E402
from prost_amd._hip import DeviceArray, check, fn, sync, sz  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
reps = int(args[0]) if args else 4
SHAPES = [(500, 250, 0.1), (4096, 1024, 8.0 / 1024), (16384, 4096, 8.0 / 4096)]
L = _hip.lib()
_hip.require_device()
for name in ("prost_hip_range_dinv_elements", "prost_hip_range_potrf_workspace_bytes_f32", "prost_hip_range_potrf_workspace_bytes_f64",
             "prost_hip_range_potrs_workspace_bytes_f32", "prost_hip_range_potrs_workspace_bytes_f64"):
    getattr(L, name).argtypes = [C.c_size_t]
    getattr(L, name).restype = C.c_size_t


def best(call):
    times = []
    for _ in range(reps):
        sync()
        t0 = time.perf_counter()
        call()
        sync()
        times.append((time.perf_counter() - t0) * 1e3)
    return min(times)


def plan(n, dtype):
    tier, nb, launches = C.c_int(0), C.c_int(0), C.c_int(0)
    check(L.prost_hip_range_potrs_plan(sz(n), 0 if dtype == np.float32 else 1, C.byref(tier), C.byref(nb), C.byref(launches), None, None))
    return tier.value, nb.value, launches.value


def rocsolver():
    """-> (handle, {dtype: potrs}) or None"""
    try:
        blas, sol = C.CDLL("librocblas.so"), C.CDLL("librocsolver.so")
    except OSError as e:
        print("rocSOLVER yardstick: not available (%s)" % e)
        return None
    handle = C.c_void_p()
    if blas.rocblas_create_handle(C.byref(handle)) != 0:
        print("rocSOLVER yardstick: rocblas_create_handle failed")
        return None
    return handle, {np.float32: sol.rocsolver_spotrs, np.float64: sol.rocsolver_dpotrs}


roc = rocsolver() if "--rocsolver" in sys.argv else None
for m, n, density in SHAPES:
    rng = np.random.default_rng(n)
    A = sp.vstack([sp.identity(n, format="csr"), sp.random(m - n, n, density=density, random_state=rng, data_rvs=rng.standard_normal, format="csr")]).tocsr()
    A = A[rng.permutation(m)]
    At = sp.csr_matrix(A.T)
    AA = np.asfortranarray((A.T @ A).toarray())
    y = rng.standard_normal(m)
    for dtype in (np.float32, np.float64):
        size = np.dtype(dtype).itemsize
        s = _hip.suffix(dtype)
        dev = lambda a, t=dtype: DeviceArray.from_host(np.ascontiguousarray(a), t)
        val, ptr, ind = dev(A.data), dev(A.indptr, np.int32), dev(A.indices, np.int32)
        val_t, ptr_t, ind_t = dev(At.data), dev(At.indptr, np.int32), dev(At.indices, np.int32)
        d_y, d_t, d_x = dev(y), DeviceArray.zeros(n, dtype), DeviceArray.zeros(m, dtype)
        d_L, d_U = dev(AA.ravel(order="F")), DeviceArray.zeros(n * n, dtype)
        d_dinv = DeviceArray.zeros(L.prost_hip_range_dinv_elements(n), dtype)
        ws_f = DeviceArray.zeros(getattr(L, "prost_hip_range_potrf_workspace_bytes_" + s)(n), np.uint8)
        ws_s = DeviceArray.zeros(max(16, getattr(L, "prost_hip_range_potrs_workspace_bytes_" + s)(n)), np.uint8)
        status = DeviceArray.zeros(1, np.int32)
        d_AA = dev(AA.ravel(order="F"))

        def factor():
            check(L.prost_hip_memcpy_d2d(d_L.ptr, d_AA.ptr, sz(n * n * size), None))
            check(fn("range_potrf", dtype)(d_L.ptr, d_U.ptr, d_dinv.ptr, ws_f.ptr, status.ptr, sz(n), None))
        t_factor = best(factor)
        assert status.to_host()[0] == -1, "the factorisation stopped at pivot %d" % status.to_host()[0]
        nnz = A.nnz
        t_aty = best(lambda: check(fn("csr_spmv", dtype)(d_t.ptr, d_y.ptr, sz(n), sz(nnz), val_t.ptr, ptr_t.ptr, ind_t.ptr, None)))
        t_host = d_t.to_host()
        tier, nb, launches = plan(n, dtype)
        solves, results = {}, {}
        for force in (1, 2):

            def solve(force=force):
                check(L.prost_hip_memcpy_h2d(d_t.ptr, t_host.ctypes.data_as(C.c_void_p), sz(t_host.nbytes), None))
                sync()
                t0 = time.perf_counter()
                check(fn("range_potrs", dtype)(d_t.ptr, d_L.ptr, d_U.ptr, d_dinv.ptr, ws_s.ptr, sz(n), force, None))
                sync()
                return (time.perf_counter() - t0) * 1e3
            try:
                solves[force] = min(solve() for _ in range(reps))
                results[force] = d_t.to_host()
            except _hip.HipError:                          # the small tier refuses an n its LDS does not hold
                assert force != tier
        same = "the tiers agree bit for bit" if len(results) == 2 and np.array_equal(results[1], results[2]) else ("THE TIERS DIFFER" if len(results) == 2 else "one tier")
        z = d_t.to_host().astype(np.float64)
        want = np.linalg.solve(AA, t_host.astype(np.float64))
        err = float(np.abs(z - want).max() / np.abs(want).max())
        t_az = best(lambda: check(fn("csr_spmv", dtype)(d_x.ptr, d_t.ptr, sz(m), sz(nnz), val.ptr, ptr.ptr, ind.ptr, None)))
        t_solve = solves[tier]
        line = "(%d, %d) %s: A'y %.3f ms, solve %.3f ms (tier %d, NB %d, %d launches, %.1f GB/s over n^2 sizeof(T)), A z %.3f ms, evaluation %.3f ms; factorisation %.2f ms; solve error %.2g; %s" % (
            m, n, "fp32" if dtype == np.float32 else "fp64", t_aty, t_solve, tier, nb, launches, n * n * size / t_solve / 1e6, t_az, t_aty + t_solve + t_az, t_factor, err, same)
        for force, t in sorted(solves.items()):
            if force != tier:
                line += "; the other tier (%d): %.3f ms" % (force, t)
        if roc is not None:
            handle, potrs = roc
            b = DeviceArray.from_host(t_host)

            def rsolve():
                check(L.prost_hip_memcpy_h2d(b.ptr, t_host.ctypes.data_as(C.c_void_p), sz(t_host.nbytes), None))
                sync()
                t0 = time.perf_counter()
                rc = potrs[dtype](handle, 122, C.c_int(n), C.c_int(1), d_L.ptr, C.c_int(n), b.ptr, C.c_int(n))       # 122 = rocblas_fill_lower
                sync()
                assert rc == 0, rc
                return (time.perf_counter() - t0) * 1e3
            line += "; rocsolver potrs %.3f ms" % min(rsolve() for _ in range(reps))
        print(line, flush=True)
