"""Throughput of the ind_epi_polyhedral kernel (prost_amd/csrc/kernels_prox_epi_polyhedral.hip) through the C ABI.
count = 2^20 groups, dim 2 and 3, m = 4 and 25 constraints per group, per-group lists and one list shared by all groups, fp32 and
fp64, planar layout, constraints randn, points 10 randn.
Reports per case: the time of one launch (`chain` launches back to back between two host synchronisations, divided by `chain`, best
of `reps`: the launch latency is amortised, not removed; for kernel times run this script under `rocprofv3 --kernel-trace --stats`),
groups per second, the compulsory bytes -- argument in, result out, coefficients, count_vec and index_vec, each counted once -- as a
fraction of the 8 TB/s HBM peak, the lanes per group, the mean step count (the NumPy restatement of the algorithm in the same
precision on the first 4096 groups: tests/epi_polyhedral_reference.py) and the fallback counter, which has to read 0.
usage: python tools/epi_polyhedral_rate.py [log2_count] [reps] [chain]"""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import epi_polyhedral_reference as R  # noqa: E402
from prost_amd import _hip  # noqa: E402

log2_count = int(sys.argv[1]) if len(sys.argv) > 1 else 20
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
chain = int(sys.argv[3]) if len(sys.argv) > 3 else 10
PEAK = 8e12

_hip.require_device()
L = _hip.lib()
L.prost_hip_epi_polyhedral_plan.argtypes = [C.c_size_t, C.c_size_t, C.c_int] + [C.POINTER(C.c_int)] * 3
count = 1 << log2_count
rng = np.random.default_rng(1)
for dtype in (np.float32, np.float64):
    fn = _hip.fn("prox_ind_epi_polyhedral", dtype)
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int] + [C.c_void_p] * 4 + [C.c_size_t, C.c_void_p, C.c_void_p]
    for dim in (2, 3):
        d = dim - 1
        z0 = (10 * rng.standard_normal((count, dim))).astype(dtype)
        arg = _hip.DeviceArray.from_host(np.ascontiguousarray(z0.T).ravel())
        res = _hip.DeviceArray.zeros(count * dim, dtype)
        for m in (4, 25):
            for shared in (False, True):
                lists = 1 if shared else count
                a = rng.standard_normal((lists * m, d)).astype(dtype)
                b = rng.standard_normal(lists * m).astype(dtype)
                cnt = np.full(count, m, np.int32)
                idx = np.zeros(count, np.int32) if shared else (np.arange(count, dtype=np.int64) * m).astype(np.int32)
                bufs = [_hip.DeviceArray.from_host(v) for v in (a.ravel(), b, cnt, idx)]
                fb = _hip.DeviceArray.zeros(1, np.uint32)
                lanes = C.c_int(0)
                assert L.prost_hip_epi_polyhedral_plan(m, dim, 0 if dtype == np.float32 else 1, C.byref(lanes), None, None) == 0
                times = []
                for _ in range(reps + 1):              # the first round warms up
                    _hip.sync()
                    t0 = time.perf_counter()
                    for _ in range(chain):
                        _hip.check(fn(res.ptr, arg.ptr, count, dim, 0, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, m, fb.ptr, None))
                    _hip.sync()
                    times.append((time.perf_counter() - t0) / chain)
                t = min(times[1:])
                item = np.dtype(dtype).itemsize
                nbytes = 2 * count * dim * item + (a.size + b.size) * item + 2 * count * 4
                info = {}
                sample = min(count, 4096)
                R.project_active_set(z0[:sample], a, b, cnt[:sample], idx[:sample], dtype, info)
                print("%s dim %d m %2d %-9s G %2d: %.3f ms, %.3g groups/s, %.1f MB compulsory = %.1f %% of 8 TB/s, mean steps %.2f (max %d), fallback %d" % (
                    np.dtype(dtype).name, dim, m, "shared" if shared else "per-group", lanes.value, t * 1e3, count / t, nbytes / 1e6, 100 * nbytes / t / PEAK,
                    info["steps"].mean(), info["steps"].max(), int(fb.to_host()[0])), flush=True)
                for v in bufs + [fb]:
                    v.free()
        arg.free()
        res.free()
