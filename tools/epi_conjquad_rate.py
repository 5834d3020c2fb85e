"""Throughput of the ind_epi_conjquad_1d kernel (prost_amd/csrc/kernels_prox_epi_conjquad.hip) through the C ABI.
count = 2^22 groups, both layouts, fp32 and fp64, coefficients as five vectors or five scalars, three inputs built from their answers
(tests/epi_conjquad_reference.py): all inside, the mixed distribution of the tests (every region), all arc (alpha = -inf, beta = +inf).
Reports per row: the time of one launch (`chain` launches back to back between two host synchronisations, divided by `chain`, best of
`reps`: the launch latency is amortised, not removed), groups per second, the compulsory bytes -- argument in, result out and vector
coefficients, each counted once -- as a fraction of the 8 TB/s HBM peak, the largest and mean Newton step count (the NumPy restatement
in the same precision on the first 2^16 groups) and the fallback counter, which has to read 0.
For the all-arc input in the planar layout the same process also times prost_hip_prox_epi_quad_* at dim = 2 on the equivalent problem
(a' = 1 / (4 a), b' = -b / (2 a), c' = b^2 / (4 a) - c), the only comparable kernel there is.
usage: python tools/epi_conjquad_rate.py [log2_count] [reps] [chain]"""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import epi_conjquad_reference as R  # noqa: E402
from prost_amd import _hip  # noqa: E402

log2_count = int(sys.argv[1]) if len(sys.argv) > 1 else 22
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
chain = int(sys.argv[3]) if len(sys.argv) > 3 else 10
PEAK = 8e12
NAMES = ("a", "b", "c", "alpha", "beta")
SCALARS = dict(a=0.75, b=0.5, c=-0.25)

_hip.require_device()
count = 1 << log2_count


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


def inputs(kind, scalar):
    rng = np.random.default_rng(5)
    fixed = dict(SCALARS) if scalar else {}
    if kind == "mixed":
        if scalar:
            fixed.update(alpha=-1.5, beta=2.0)
        return R.random_cases(rng, count, 10.0, fixed=fixed)
    if kind == "inside":
        if scalar:
            fixed.update(alpha=-1.5, beta=2.0)
        return R.random_cases(rng, count, 10.0, shares=((R.INSIDE, 1.0),), fixed=fixed)
    cs = R.random_cases(rng, count, 10.0, shares=((R.ARC, 1.0),), infinite=1.0, a_values=(0.25, 1.0, 4.0), fixed=fixed)
    assert np.isinf(cs["alpha"]).all() and np.isinf(cs["beta"]).all()
    if scalar:
        cs["alpha"], cs["beta"] = cs["alpha"][:1], cs["beta"][:1]
    return cs


for dtype in (np.float32, np.float64):
    item = np.dtype(dtype).itemsize
    fn = _hip.fn("prox_ind_epi_conjquad_1d", dtype)
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int] + [C.c_void_p, C.c_double] * 5 + [C.c_void_p, C.c_void_p, C.c_void_p]
    quad = _hip.fn("prox_epi_quad", dtype)
    quad.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p]
    for kind in ("inside", "mixed", "arc"):
        for scalar in (False, True):
            cs = inputs(kind, scalar)
            z0 = cs["z0"].astype(dtype)
            info = {}
            sample = min(count, 1 << 16)
            _, _, region = R.project(z0[:sample, 0], z0[:sample, 1], *[cs[n] if cs[n].size == 1 else cs[n][:sample] for n in NAMES], dtype, info=info)
            share = np.bincount(region, minlength=5) / region.size
            bufs, args, vec_bytes = [], [], 0
            for n in NAMES:
                if cs[n].size > 1:
                    bufs.append(_hip.DeviceArray.from_host(cs[n].astype(dtype)))
                    args += [bufs[-1].ptr, C.c_double(0.0)]
                    vec_bytes += count * item
                else:
                    args += [None, C.c_double(float(cs[n][0]))]
            fb = _hip.DeviceArray.zeros(1, np.uint32)
            res = _hip.DeviceArray.zeros(2 * count, dtype)
            nbytes = 4 * count * item + vec_bytes
            for interleaved in (False, True):
                arg = _hip.DeviceArray.from_host(np.ascontiguousarray(z0 if interleaved else z0.T).ravel())
                t = timed(lambda: fn(res.ptr, arg.ptr, count, 1 if interleaved else 0, *args, fb.ptr, None, None))
                print("%s %-6s %-7s %-11s: %.4f ms, %.3g groups/s, %.1f MB compulsory = %.1f %% of 8 TB/s, steps max %d mean %.2f, regions %s, fallback %d" % (
                    np.dtype(dtype).name, kind, "scalars" if scalar else "vectors", "interleaved" if interleaved else "planar", t * 1e3, count / t, nbytes / 1e6,
                    100 * nbytes / t / PEAK, info["steps"].max(), info["steps"].mean(), "/".join("%.2f" % s for s in share), int(fb.to_host()[0])), flush=True)
                if kind == "arc" and not interleaved:
                    a, b, c = (np.broadcast_to(cs[n], (count,)) for n in ("a", "b", "c"))
                    qa, qb, qc = 1 / (4 * a), -b / (2 * a), b * b / (4 * a) - c
                    qbufs = [_hip.DeviceArray.from_host(np.ascontiguousarray(v).astype(dtype)) for v in ((qb,) if scalar else (qa, qb, qc))]
                    if scalar:
                        tq = timed(lambda: quad(res.ptr, arg.ptr, count, 2, None, C.c_double(float(qa[0])), qbufs[0].ptr, None, C.c_double(float(qc[0])), None))
                        qbytes = 4 * count * item + count * item
                    else:
                        tq = timed(lambda: quad(res.ptr, arg.ptr, count, 2, qbufs[0].ptr, C.c_double(0.0), qbufs[1].ptr, qbufs[2].ptr, C.c_double(0.0), None))
                        qbytes = 4 * count * item + 3 * count * item
                    print("%s %-6s %-7s %-11s: %.4f ms with prox_epi_quad at dim 2 (%.1f MB compulsory = %.1f %% of 8 TB/s): the new kernel takes %.2f of its time" % (
                        np.dtype(dtype).name, kind, "scalars" if scalar else "vectors", "planar", tq * 1e3, qbytes / 1e6, 100 * qbytes / tq / PEAK, t / tq), flush=True)
                    for v in qbufs:
                        v.free()
                arg.free()
            for v in bufs + [fb, res]:
                v.free()
