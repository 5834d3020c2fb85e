"""Exact-class K-iteration launches through the kernel C ABI: time of one launch per (K, cols), against the plain pair launch.
usage: iterk_levelwave_probe.py [N] [K,K,...] [cols,cols,...]      (PROST_ITERK_LEVELWAVE=0: the single-wave instances)
Prints one line per (K, cols): ms per launch, us per iteration, and the two pair launches a launch of four replaces."""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from prost_amd import _hip as hip
from prost_amd import synthetic

if os.environ.get("PROST_HIP_LIB"):
    hip.LIB_PATH = os.environ["PROST_HIP_LIB"]


def main(N=4096, ks=(3, 4), cols_list=(0,), iters=200):
    hip.require_device()
    dtype = np.float32
    n, m = N * N, 2 * N * N
    rng = np.random.default_rng(0)
    fh = synthetic.rof_image(N, N, seed=42).astype(dtype)
    xh = (fh + 0.05 * (rng.random(n).astype(dtype) - 0.5)).astype(dtype)
    yh = ((rng.random(m) - 0.5) * 1.2).astype(dtype)
    f = hip.DeviceArray.from_host(fh)
    x = [hip.DeviceArray.from_host(xh), hip.DeviceArray.zeros(n, dtype)]
    y = [hip.DeviceArray.from_host(yh), hip.DeviceArray.zeros(m, dtype)]
    d = hip.FusedDesc(); d.is3d = 0; d.nx, d.ny, d.L = N, N, 1
    d.g_fn = hip.FN_ID["square"]; d.f_fn = hip.FN_ID["ind_leq0"]
    gv = [1, 0, 10, 0, 0, 0, 0]; fv = [1, 1, 1, 0, 0, 0, 0]
    for i in range(7):
        d.g_coeff_val[i] = gv[i]; d.f_coeff_val[i] = fv[i]
    d.g_coeff_ptr[1] = f.ptr.value
    d.T_val, d.S_val = 0.25, 0.5
    d.arith = 0
    L_ = hip.lib()
    I2 = hip.fn("fused_iteration2", dtype)
    IK = L_.prost_hip_fused_iterationk_f32
    taus = (C.c_double * 4)(0.3, 0.29, 0.28, 0.27); sigmas = (C.c_double * 4)(1.0, 1.03, 1.06, 1.09); thetas = (C.c_double * 4)(0.9, 0.91, 0.92, 0.93)
    ev = [C.c_void_p() for _ in range(2)]
    for e in ev:
        hip.check(L_.prost_hip_event_create(C.byref(e)))

    def timed(launch):
        def run(cnt):
            for i in range(cnt):
                launch(i % 2, (i + 1) % 2)
        best = None
        for _ in range(3):
            run(10); hip.sync()
            hip.check(L_.prost_hip_event_record(ev[0], None)); run(iters); hip.check(L_.prost_hip_event_record(ev[1], None))
            hip.check(L_.prost_hip_event_synchronize(ev[1]))
            ms = C.c_float(); hip.check(L_.prost_hip_event_elapsed_ms(ev[0], ev[1], C.byref(ms)))
            best = ms.value / iters if best is None else min(best, ms.value / iters)
        return best
    pair = timed(lambda a, b: hip.check(I2(C.byref(d), x[b].ptr, y[b].ptr, x[a].ptr, y[a].ptr, None, None, taus, sigmas, thetas, 0, None, None, None)))
    print("N=%d levelwave=%s plain pair: %.4f ms/launch, %.1f us/iteration" % (N, os.environ.get("PROST_ITERK_LEVELWAVE", "1"), pair, 500 * pair), flush=True)
    for k in ks:
        for cols in cols_list:
            t = timed(lambda a, b: hip.check(IK(C.byref(d), k, x[b].ptr, y[b].ptr, x[a].ptr, y[a].ptr, taus, sigmas, thetas, cols, None, None, None)))
            print("N=%d K=%d cols=%-3d (auto %d): %.4f ms/launch, %.1f us/iteration, against pairs %+.1f %%" % (
                N, k, cols, L_.prost_hip_fused_iterationk_chunk_cols(C.byref(d), 0, k, 0), t, 1e3 * t / k, 100 * (t / k - pair / 2) / (pair / 2)), flush=True)


if __name__ == "__main__":
    N = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
    ks = tuple(int(v) for v in sys.argv[2].split(",")) if len(sys.argv) > 2 else (3, 4)
    cols = tuple(int(v) for v in sys.argv[3].split(",")) if len(sys.argv) > 3 else (0,)
    main(N, ks, cols)
