"""The level-per-wavefront family of the K-iteration kernel (fused_iter2d_xkw_kernel, kernels_fused_iterk.hip: exact class, plain
launches, K = 3 and 4) and the launch of four iterations in the pair plan (pdhg_pair_plan.hpp).

Every comparison is bit for bit (np.array_equal, NaN positions included where the data has NaNs):
  * prost_hip_fused_iterationk_f32 against tests/pdhg_iteration_reference.py (the CPU oracle's pieces, K iterations) and against K
    launches of the single-iteration kernel: image widths below, at and above the chunk lengths, forced chunks of 2, 3, 18, 72
    columns, one strip / a strip plus one lane / a ragged last strip, 'square' and 'abs', scalar and per-pixel b, different step
    sizes per level;
  * the _rec entry with the record's stop word raised: the outputs stay untouched and the call returns;
  * the directed lanes of tests/test_gpu_elementwise_edges.py (a NaN, a zero, an overflowing and an ordinary norm in one lane);
  * PROST_ITERK_LEVELWAVE=0 and =1 give the same bits;
  * the solver with launches of four (size threshold overridden) against oracle.Solver, and against the pair plan (group_max = 1).
"""
import ctypes as C
import os

import numpy as np
import pytest

import oracle
import prost_amd as prost
from prost_amd import synthetic
from pdhg_iteration_reference import F_COEFFS, SVAL, oracle_iteration
from test_gpu_elementwise_edges import check_lane_classes, fused_edge_data, make_desc

pytestmark = pytest.mark.gpu

TAUS, SIGMAS, THETAS = (0.5, 0.7, 0.6, 0.45), (1.1, 1.4, 1.2, 1.3), (0.85, 0.8, 0.9, 0.75)
TVAL = 0.25
ZERO_TOL = dict(tol_rel_primal=0, tol_rel_dual=0, tol_abs_primal=0, tol_abs_dual=0)


@pytest.fixture(autouse=True)
def _gpu(hip):
    prost.set_gpu(0)
    prost.set_precision("single")
    old = {k: os.environ.get(k) for k in ("PROST_ITERK_LEVELWAVE", "PROST_PDHG_FOURS_MIN_PIXELS")}
    os.environ.pop("PROST_ITERK_LEVELWAVE", None)
    yield
    for k, v in old.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
    prost.set_precision("double")


def _arr(v, k):
    return (C.c_double * k)(*v[:k])


def _same(g, w):
    return bool(((g == w) | (np.isnan(g) & np.isnan(w))).all())


def _launch_k(hip, ref, K, dx, dy, cols, fill=7.0):
    """one launch of K iterations into fresh buffers; returns (x, y) on the host"""
    xo = hip.DeviceArray.from_host(np.full(dx.n, fill, np.float32)); yo = hip.DeviceArray.from_host(np.full(dy.n, fill, np.float32))
    hip.check(hip.lib().prost_hip_fused_iterationk_f32(ref, K, xo.ptr, yo.ptr, dx.ptr, dy.ptr, _arr(TAUS, K), _arr(SIGMAS, K), _arr(THETAS, K), cols, None, None, None))
    out = xo.to_host(), yo.to_host()
    xo.free(); yo.free()
    return out


def _problem(nx, ny, g_fn, bpp, seed):
    rng = np.random.default_rng(seed)
    n = nx * ny
    x = rng.uniform(0, 1, n).astype(np.float32); f = rng.uniform(0, 1, n).astype(np.float32); y = rng.uniform(-1, 1, 2 * n).astype(np.float32)
    g_coeffs = [1.0, f if bpp else 0.4, 8.0, 0.0, 0.0, 0.3, 0.0]
    return x, y, g_coeffs


@pytest.mark.parametrize("nx", [8, 9, 19, 37, 150])
def test_a_launch_equals_the_oracle_and_single_launches_bit_for_bit(hip, nx):
    L_ = hip.lib()
    launches = 0
    for ny in (8, 248, 252, 500):
        for g_fn, bpp in (("square", True), ("square", False), ("abs", True), ("abs", False)):
            shape = (nx, ny, 1)
            x, y, g_coeffs = _problem(nx, ny, g_fn, bpp, 1000 * nx + ny)
            its = [(x, y)]
            for k in range(4):
                x1, y1, _ = oracle_iteration("2d", its[-1][0], its[-1][1], shape, g_coeffs, TVAL, TAUS[k], SIGMAS[k], THETAS[k], np.float32, g_fn, "ind_leq0")
                its.append((x1, y1))
            desc, keep = make_desc(hip, "2d", shape, np.float32, (g_fn, "ind_leq0"), g_coeffs, TVAL)
            ref = C.byref(desc)
            assert L_.prost_hip_fused_iterationk_max(ref, 0) == 4
            dx, dy = hip.DeviceArray.from_host(x), hip.DeviceArray.from_host(y)
            # K launches of the single-iteration kernel
            cur = (dx, dy); singles = []
            for k in range(4):
                nxt = (hip.DeviceArray.zeros(x.size, np.float32), hip.DeviceArray.zeros(y.size, np.float32))
                hip.check(L_.prost_hip_fused_iteration_f32(ref, nxt[0].ptr, nxt[1].ptr, cur[0].ptr, cur[1].ptr, None, hip.dbl(TAUS[k]), hip.dbl(SIGMAS[k]), hip.dbl(THETAS[k]),
                                                           1, 1, 0, 0, None, None, None))
                singles.append(nxt); cur = nxt
            for K in (3, 4):
                sx, sy = singles[K - 1][0].to_host(), singles[K - 1][1].to_host()
                assert np.array_equal(sx, its[K][0]) and np.array_equal(sy, its[K][1]), ("single launches against the oracle", nx, ny, g_fn, bpp, K)
                for cols in (0, 2, 3, 18, 72):
                    if cols > nx:
                        continue                # (longer than the image: one chunk, which 18 / 72 at the next width already are)
                    gx, gy = _launch_k(hip, ref, K, dx, dy, cols)
                    assert np.array_equal(gx, its[K][0]), ("x", nx, ny, g_fn, bpp, K, cols, int((gx != its[K][0]).sum()))
                    assert np.array_equal(gy, its[K][1]), ("y", nx, ny, g_fn, bpp, K, cols, int((gy != its[K][1]).sum()))
                    assert np.array_equal(gx, sx) and np.array_equal(gy, sy)
                    launches += 1
            for a in [dx, dy] + [v for pair in singles for v in pair]:
                a.free()
            del keep
    assert launches >= 4 * 4 * 2 * 3


def test_the_two_families_give_the_same_bits(hip):
    for nx, ny, g_fn, bpp in ((37, 252, "square", True), (150, 500, "abs", False), (300, 1000, "square", True)):
        x, y, g_coeffs = _problem(nx, ny, g_fn, bpp, 7)
        desc, keep = make_desc(hip, "2d", (nx, ny, 1), np.float32, (g_fn, "ind_leq0"), g_coeffs, TVAL)
        dx, dy = hip.DeviceArray.from_host(x), hip.DeviceArray.from_host(y)
        for K in (3, 4):
            for cols in (0, 18):
                got = {}
                for lw in ("0", "1"):
                    os.environ["PROST_ITERK_LEVELWAVE"] = lw
                    got[lw] = _launch_k(hip, C.byref(desc), K, dx, dy, cols)
                assert np.array_equal(got["0"][0], got["1"][0]) and np.array_equal(got["0"][1], got["1"][1]), (nx, ny, K, cols)
                assert np.isfinite(got["1"][0]).all() and not (got["1"][0] == 7.0).any()
        dx.free(); dy.free()
        del keep


def test_the_rec_entry_takes_the_records_steps_and_returns_at_once_when_stopped(hip):
    L_ = hip.lib()
    L_.prost_hip_pdhg_rule_record_bytes.restype = C.c_size_t
    nx, ny = 37, 252
    x, y, g_coeffs = _problem(nx, ny, "square", True, 3)
    desc, keep = make_desc(hip, "2d", (nx, ny, 1), np.float32, ("square", "ind_leq0"), g_coeffs, TVAL)
    ref = C.byref(desc)
    dx, dy = hip.DeviceArray.from_host(x), hip.DeviceArray.from_host(y)
    rec = hip.DeviceArray(L_.prost_hip_pdhg_rule_record_bytes(), np.uint8)
    opts = (C.c_byte * 256)()          # prost_hip_pdhg_rule_opts, variant 0 = PROST_PDHG_RULE_NONE: nothing adapts the steps
    hip.check(L_.prost_hip_pdhg_rule_begin_f32(rec.ptr, opts, ref, hip.dbl(TAUS[0]), hip.dbl(SIGMAS[0]), hip.dbl(THETAS[0]), hip.dbl(0.5), 0, 0, 1, None, None))
    for K in (3, 4):
        xo = hip.DeviceArray.from_host(np.full(x.size, 7.0, np.float32)); yo = hip.DeviceArray.from_host(np.full(y.size, 7.0, np.float32))
        hip.check(L_.prost_hip_fused_iterationk_rec_f32(ref, K, xo.ptr, yo.ptr, dx.ptr, dy.ptr, rec.ptr, 0, None, None, 0, C.c_ulonglong(0), None, None))
        want = hip.DeviceArray.zeros(x.size, np.float32), hip.DeviceArray.zeros(y.size, np.float32)
        hip.check(L_.prost_hip_fused_iterationk_f32(ref, K, want[0].ptr, want[1].ptr, dx.ptr, dy.ptr, _arr(TAUS[:1] * 4, K), _arr(SIGMAS[:1] * 4, K), _arr(THETAS[:1] * 4, K),
                                                    0, None, None, None))
        assert np.array_equal(xo.to_host(), want[0].to_host()) and np.array_equal(yo.to_host(), want[1].to_host()), K
        for a in (xo, yo) + want:
            a.free()
    stop = C.POINTER(C.c_int)()
    hip.check(L_.prost_hip_pdhg_record_view(rec.ptr, 0, None, None, None, C.byref(stop)))
    one = np.ones(1, np.int32)
    hip.check(L_.prost_hip_memcpy_h2d(stop, one.ctypes.data_as(C.c_void_p), C.c_size_t(4), None)); hip.sync()
    for K in (3, 4):
        xo = hip.DeviceArray.from_host(np.full(x.size, 7.0, np.float32)); yo = hip.DeviceArray.from_host(np.full(y.size, 7.0, np.float32))
        hip.check(L_.prost_hip_fused_iterationk_rec_f32(ref, K, xo.ptr, yo.ptr, dx.ptr, dy.ptr, rec.ptr, 0, None, None, 0, C.c_ulonglong(0), None, None))
        hip.sync()
        assert (xo.to_host() == 7.0).all() and (yo.to_host() == 7.0).all(), K
        xo.free(); yo.free()
    dx.free(); dy.free(); rec.free()
    del keep


@pytest.mark.parametrize("g_fn", ["square", "abs"])
def test_directed_lanes_nan_zero_overflow_and_ordinary_norm_in_one_lane(hip, g_fn):
    shape = (8, 16, 1)
    x, f, y, marks = fused_edge_data("2d", shape, np.float32, g_fn)
    g_coeffs = [1.0, f, 8.0, 0.0, 0.0, 0.3, 0.0]
    its = [(x, y)]
    for k in range(4):
        x1, y1, nv = oracle_iteration("2d", its[-1][0], its[-1][1], shape, g_coeffs, TVAL, TAUS[k], SIGMAS[k], THETAS[k], np.float32, g_fn, "ind_leq0")
        if k == 0:
            check_lane_classes(nv, "2d", shape, np.float32, marks)
        its.append((x1, y1))
    desc, keep = make_desc(hip, "2d", shape, np.float32, (g_fn, "ind_leq0"), g_coeffs, TVAL)
    dx, dy = hip.DeviceArray.from_host(x), hip.DeviceArray.from_host(y)
    for K in (3, 4):
        for cols in (0, 2, 3):
            gx, gy = _launch_k(hip, C.byref(desc), K, dx, dy, cols)
            assert _same(gx, its[K][0]) and _same(gy, its[K][1]), (K, cols)
    dx.free(); dy.free()
    del keep


def _solve(prob, period, k, group_max=None):
    b = prost.backend.pdhg(stepsize="alg2", residual_iter=period, alg2_gamma=0.5)
    if group_max is not None:
        b[1]["group_max"] = group_max
    o = prost.options(max_iters=10 ** 6, num_cback_calls=0, verbose=False, **ZERO_TOL)
    s = prost.Solver(prob, b, o)
    info = s.iterate(k, time_kernels=True, sample_every=1)
    st = s.state()
    s.destroy()
    return b, o, st, info


@pytest.mark.parametrize("period,k", [(1, 23), (2, 23), (3, 23), (7, 23), (10, 23), (10, 6), (10, 15), (7, 12)])
def test_the_solver_with_launches_of_four_equals_the_oracle_and_the_pair_plan(period, k):
    """23 iterations; 6 (inside the first residual period, which keeps the pair plan); 15 at period 10 and 12 at period 7: a read-out
    right behind a launch of four (iterations 11 .. 14 and 8 .. 11), whose previous iterate is rebuilt through the K = 3 instance"""
    os.environ["PROST_PDHG_FOURS_MIN_PIXELS"] = "0"
    prob, u, q, f = synthetic.rof_problem(256, 248)
    b, o, st, info = _solve(prob, period, k)
    assert st["arithmetic"] == "exact" and st["path"] == "pdhg:fused-grad2d"
    fours = "fused_iter2d_xk_kernel<4>" in info["kernels"]
    assert fours == (period >= 7 and k >= period + 5), (period, k, info["kernels"])          # five iterations without a residual one, behind the first period
    os_ = oracle.Solver(prob.data, prob.nrows, prob.ncols, b, o, np.float32)
    os_.initialize(); os_.iterate(k)
    ost = os_.state()
    del os_
    _, _, sp, infop = _solve(prob, period, k, group_max=1)
    assert "fused_iter2d_xk_kernel<4>" not in infop["kernels"]
    for v in "xyzw":
        assert np.array_equal(st[v], ost[v]), (v, period, int((st[v] != ost[v]).sum()))
        assert int((st[v] != sp[v]).sum()) == 0, (v, period)
