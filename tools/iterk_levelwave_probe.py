"""Exact-class K-iteration launches through the kernel C ABI: time of one launch per (K, cols), against the plain pair launch.
usage: iterk_levelwave_probe.py [N] [K,K,...] [cols,cols,...]      (PROST_ITERK_LEVELWAVE=0: the single-wave instances)
       iterk_levelwave_probe.py ring [N] [cols,cols,...]           K = 4: the two-slot ring against the three-slot one, length by length
       iterk_levelwave_probe.py place [N]
Prints one line per (K, cols): ms per launch, us per iteration, and the two pair launches a launch of four replaces.
place: where the wavefronts of the K = 4 launch (square, per-pixel b, auto chunk length) ran -- every wave records its HW_ID and XCC_ID
after its last step: workgroups per CU, which workgroups share a CU, wave -> SIMD, distinct levels per SIMD, launch against launch.
ring: PROST_ITERK_LW_RING is read per launch, so both depths run in one process, alternating, on the same buffers (cols 0: each
depth's own rule)."""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from prost_amd import _hip as hip
from prost_amd import synthetic

if os.environ.get("PROST_HIP_LIB"):
    hip.LIB_PATH = os.environ["PROST_HIP_LIB"]


def _setup(N):
    dtype = np.float32
    n, m = N * N, 2 * N * N
    rng = np.random.default_rng(0)
    fh = synthetic.rof_image(N, N, seed=42).astype(dtype)
    xh = (fh + 0.05 * (rng.random(n).astype(dtype) - 0.5)).astype(dtype)
    f = hip.DeviceArray.from_host(fh)
    x = [hip.DeviceArray.from_host(xh), hip.DeviceArray.zeros(n, dtype)]
    y = [hip.DeviceArray.from_host(((rng.random(m) - 0.5) * 1.2).astype(dtype)), hip.DeviceArray.zeros(m, dtype)]
    d = hip.FusedDesc(); d.is3d = 0; d.nx, d.ny, d.L = N, N, 1
    d.g_fn = hip.FN_ID["square"]; d.f_fn = hip.FN_ID["ind_leq0"]
    for i, (g, fv) in enumerate(zip([1, 0, 10, 0, 0, 0, 0], [1, 1, 1, 0, 0, 0, 0])):
        d.g_coeff_val[i] = g; d.f_coeff_val[i] = fv
    d.g_coeff_ptr[1] = f.ptr.value
    d.T_val, d.S_val = 0.25, 0.5
    d.arith = 0
    return d, f, x, y


def main(N=4096, ks=(3, 4), cols_list=(0,), iters=200):
    hip.require_device()
    dtype = np.float32
    d, f, x, y = _setup(N)
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


def ring(N=4096, cols_list=(0,), iters=200, rounds=3):
    """K = 4, square, per-pixel b: ms per launch with two and with three ring slots at every chunk length, `rounds` times alternating"""
    hip.require_device()
    d, f, x, y = _setup(N)
    L_ = hip.lib()
    IK = L_.prost_hip_fused_iterationk_f32
    taus = (C.c_double * 4)(0.3, 0.29, 0.28, 0.27); sigmas = (C.c_double * 4)(1.0, 1.03, 1.06, 1.09); thetas = (C.c_double * 4)(0.9, 0.91, 0.92, 0.93)
    ev = [C.c_void_p() for _ in range(2)]
    for e in ev:
        hip.check(L_.prost_hip_event_create(C.byref(e)))

    def timed(cols):
        for i in range(10):
            hip.check(IK(C.byref(d), 4, x[(i + 1) % 2].ptr, y[(i + 1) % 2].ptr, x[i % 2].ptr, y[i % 2].ptr, taus, sigmas, thetas, cols, None, None, None))
        hip.sync()
        hip.check(L_.prost_hip_event_record(ev[0], None))
        for i in range(iters):
            hip.check(IK(C.byref(d), 4, x[(i + 1) % 2].ptr, y[(i + 1) % 2].ptr, x[i % 2].ptr, y[i % 2].ptr, taus, sigmas, thetas, cols, None, None, None))
        hip.check(L_.prost_hip_event_record(ev[1], None))
        hip.check(L_.prost_hip_event_synchronize(ev[1]))
        ms = C.c_float(); hip.check(L_.prost_hip_event_elapsed_ms(ev[0], ev[1], C.byref(ms)))
        return ms.value / iters

    for cols in cols_list:
        got = {"2": [], "3": []}
        auto = {}
        for _ in range(rounds):
            for depth in ("3", "2"):
                if depth == "3":
                    os.environ["PROST_ITERK_LW_RING"] = "3"
                else:
                    os.environ.pop("PROST_ITERK_LW_RING", None)
                auto[depth] = L_.prost_hip_fused_iterationk_chunk_cols(C.byref(d), 0, 4, 0)
                got[depth].append(timed(cols))
        os.environ.pop("PROST_ITERK_LW_RING", None)
        m2, m3 = sorted(got["2"])[rounds // 2], sorted(got["3"])[rounds // 2]
        print("N=%d K=4 cols=%-3d (auto: 3 slots %d, 2 slots %d): 3 slots %s ms, 2 slots %s ms, medians %.4f -> %.4f (%+.1f %%)" % (
            N, cols, auto["3"], auto["2"], " ".join("%.4f" % v for v in got["3"]), " ".join("%.4f" % v for v in got["2"]), m3, m2, 100 * (m2 - m3) / m3), flush=True)


def _hist(values):
    h = {}
    for v in values:
        h[v] = h.get(v, 0) + 1
    return " ".join("%s:%d" % (k, h[k]) for k in sorted(h))


def place(N=4096, K=4):
    """the placement record of the real launch (PROST_ITERK_LEVELWAVE_PLACE=1: the workspace argument receives grid x K words)"""
    hip.require_device()
    d, f, x, y = _setup(N)
    L_ = hip.lib()
    IK = L_.prost_hip_fused_iterationk_f32
    taus = (C.c_double * 4)(0.3, 0.29, 0.28, 0.27); sigmas = (C.c_double * 4)(1.0, 1.03, 1.06, 1.09); thetas = (C.c_double * 4)(0.9, 0.91, 0.92, 0.93)
    cols = L_.prost_hip_fused_iterationk_chunk_cols(C.byref(d), 0, K, 0)
    grid = -(-N // 248) * -(-N // cols)
    os.environ["PROST_ITERK_LEVELWAVE_PLACE"] = "1"

    def record(back_to_back):
        rec = hip.DeviceArray.from_host(np.full(grid * K, 0xffffffff, np.uint32))
        for i in range(back_to_back):
            hip.check(IK(C.byref(d), K, x[(i + 1) % 2].ptr, y[(i + 1) % 2].ptr, x[i % 2].ptr, y[i % 2].ptr, taus, sigmas, thetas, 0, None, rec.ptr, None))
        hip.sync()
        w = rec.to_host().reshape(grid, K)
        rec.free()
        assert (w != 0xffffffff).all(), "waves without a record"
        return w

    runs = [("first launch", record(1)), ("second launch", record(1)), ("fifth of five back to back", record(5))]
    first = runs[0][1]
    for name, w in runs:
        simd, cu = (w >> 4) & 3, (w >> 8) & 0xfff          # cu: CU, SH, SE of HW_ID and the XCC above them
        print("N=%d K=%d cols=%d grid=%d, %s" % (N, K, cols, grid, name))
        print("  waves of a workgroup on one CU: %s" % _hist(len(set(cu[b])) == 1 for b in range(grid)))
        print("  (wave, SIMD) pairs: %s" % _hist("w%d@s%d" % (k, simd[b, k]) for b in range(grid) for k in range(K)))
        print("  workgroup b on XCC: b %% 8 == XCC for %d of %d; XCCs seen: %s" % (sum(int((w[b, 0] >> 16) & 15) == b % 8 for b in range(grid)), grid, _hist(int((w[b, 0] >> 16) & 15) for b in range(grid))))
        on = {}
        for b in range(grid):
            on.setdefault(int(cu[b, 0]), []).append(b)
        print("  CUs used: %d; workgroups per CU: %s" % (len(on), _hist(len(v) for v in on.values())))
        most = max(len(v) for v in on.values())
        print("  differences of the workgroups that share a CU (to the lowest b): %s" % _hist(tuple(b - v[0] for b in v[1:]) for v in on.values() if len(v) == most))
        for c in sorted(on)[:4]:
            print("    CU %03x: b = %s" % (c, on[c]))
        levels = []
        for c, v in on.items():
            if len(v) == most:
                for sd in range(4):
                    levels.append(len({k + 1 for b in v for k in range(K) if simd[b, k] == sd}))          # wave k carries level k + 1
        share = sum(1 for v in levels if v >= 3) / max(1, len(levels))
        print("  CUs with %d workgroups: distinct levels per SIMD: %s; SIMDs with >= 3 levels: %.1f %%" % (most, _hist(levels), 100 * share))
        if w is not first:
            print("  against the first launch: same CU for %d of %d workgroups, same SIMD for %d of %d waves" % (
                int((((first >> 8) & 0xfff)[:, 0] == cu[:, 0]).sum()), grid, int((((first >> 4) & 3) == simd).sum()), grid * K), flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "place":
        place(int(sys.argv[2]) if len(sys.argv) > 2 else 4096)
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "ring":
        ring(int(sys.argv[2]) if len(sys.argv) > 2 else 4096, tuple(int(v) for v in sys.argv[3].split(",")) if len(sys.argv) > 3 else (0,))
        sys.exit(0)
    N = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
    ks = tuple(int(v) for v in sys.argv[2].split(",")) if len(sys.argv) > 2 else (3, 4)
    cols = tuple(int(v) for v in sys.argv[3].split(",")) if len(sys.argv) > 3 else (0,)
    main(N, ks, cols)
