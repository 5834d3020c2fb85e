"""The level-per-wavefront K-iteration kernel with the two-slot input ring (K = 4, per-pixel b: fused_iter2d_xkw_kernel<4, g, true, 2>,
32 KiB of LDS per workgroup) against the CPU oracle's pieces, K single launches and the three-slot instance (PROST_ITERK_LW_RING=3).

Every comparison is bit for bit, NaN positions included (_same):
  * nx in {2, 3, 8, 9, 37} x ny in {8, 248, 252} x chunks {rule, 1, 2, 3, 7}, 'square' and 'abs', different steps per level (a direct
    launch of the level-wave family takes images from two columns; the solver's plan keeps asking for eight);
  * 152 x 500 in chunks of 15 (last chunk 2) and 55 (last chunk 42); 300 x 500 in chunks of one column (900 workgroups: every CU full);
  * the _rec entry; the solver at 256 x 248, periods 7 and 10, 23 iterations, against oracle.Solver;
  * the chunk length reported for a per-pixel-b description equals the one-round rule restated here, with either ring depth.
"""
import ctypes as C
import os

import numpy as np
import pytest

import oracle
import prost_amd as prost
from prost_amd import synthetic
from pdhg_iteration_reference import oracle_iteration
from test_gpu_elementwise_edges import make_desc
from test_gpu_iterk_levelwave import SIGMAS, TAUS, THETAS, TVAL, ZERO_TOL, _arr, _launch_k, _problem, _same

pytestmark = pytest.mark.gpu

ENV = ("PROST_ITERK_LEVELWAVE", "PROST_ITERK_LW_RING", "PROST_ITERK3_COLS", "PROST_ITERK4_COLS", "PROST_PDHG_FOURS_MIN_PIXELS")


@pytest.fixture(autouse=True)
def _gpu(hip):
    prost.set_gpu(0)
    prost.set_precision("single")
    old = {k: os.environ.get(k) for k in ENV}
    for k in ENV[:4]:
        os.environ.pop(k, None)
    yield
    for k, v in old.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
    prost.set_precision("double")


def _ring(depth):
    if depth == 3:
        os.environ["PROST_ITERK_LW_RING"] = "3"
    else:
        os.environ.pop("PROST_ITERK_LW_RING", None)


def _check(hip, nx, ny, g_fn, chunks, seed):
    """K = 4, per-pixel b: the two-slot launch at every chunk length against the oracle's iterate, four single launches and the
    three-slot launch; returns the two-slot launches run"""
    L_ = hip.lib()
    shape = (nx, ny, 1)
    x, y, g_coeffs = _problem(nx, ny, g_fn, True, seed)
    cur = (x, y)
    for k in range(4):
        x1, y1, _ = oracle_iteration("2d", cur[0], cur[1], shape, g_coeffs, TVAL, TAUS[k], SIGMAS[k], THETAS[k], np.float32, g_fn, "ind_leq0")
        cur = (x1, y1)
    want = cur
    desc, keep = make_desc(hip, "2d", shape, np.float32, (g_fn, "ind_leq0"), g_coeffs, TVAL)
    ref = C.byref(desc)
    dx, dy = hip.DeviceArray.from_host(x), hip.DeviceArray.from_host(y)
    dcur = (dx, dy); made = []
    for k in range(4):
        nxt = (hip.DeviceArray.zeros(x.size, np.float32), hip.DeviceArray.zeros(y.size, np.float32))
        hip.check(L_.prost_hip_fused_iteration_f32(ref, nxt[0].ptr, nxt[1].ptr, dcur[0].ptr, dcur[1].ptr, None, hip.dbl(TAUS[k]), hip.dbl(SIGMAS[k]), hip.dbl(THETAS[k]),
                                                   1, 1, 0, 0, None, None, None))
        made.append(nxt); dcur = nxt
    sx, sy = dcur[0].to_host(), dcur[1].to_host()
    launches = 0
    for cols in chunks:
        _ring(2)
        gx, gy = _launch_k(hip, ref, 4, dx, dy, cols)
        _ring(3)
        tx, ty = _launch_k(hip, ref, 4, dx, dy, cols)
        _ring(2)
        assert _same(gx, want[0]) and _same(gy, want[1]), ("oracle", nx, ny, g_fn, cols, int((gx != want[0]).sum()), int((gy != want[1]).sum()))
        assert _same(gx, sx) and _same(gy, sy), ("single launches", nx, ny, g_fn, cols)
        assert _same(gx, tx) and _same(gy, ty), ("three slots", nx, ny, g_fn, cols)
        launches += 1
    for a in [dx, dy] + [v for pair in made for v in pair]:
        a.free()
    del keep
    return launches


@pytest.mark.parametrize("nx", [2, 3, 8, 9, 37])
def test_two_slots_equal_the_oracle_single_launches_and_three_slots(hip, nx):
    """chunks of the rule (6 columns at these sizes), 1, 2, 3 and 7 columns: first and last chunks of 1, 2, cols - 1 and cols columns"""
    launches = 0
    for ny in (8, 248, 252):
        for g_fn in ("square", "abs"):
            launches += _check(hip, nx, ny, g_fn, (0, 1, 2, 3, 7), 3000 * nx + ny)
    assert launches == 3 * 2 * 5


@pytest.mark.parametrize("g_fn", ["square", "abs"])
def test_chunks_of_15_and_55_columns(hip, g_fn):
    """152 columns: in chunks of 15 the last one has 2 columns, in chunks of 55 it has 42"""
    assert 152 % 15 == 2 and 152 % 55 == 42
    assert _check(hip, 152, 500, g_fn, (15, 55), 41) == 2


@pytest.mark.parametrize("g_fn", ["square", "abs"])
def test_a_grid_of_900_workgroups(hip, g_fn):
    """300 x 500 in chunks of one column: 3 strips x 300 chunks, every CU holds several workgroups of the launch at once"""
    assert _check(hip, 300, 500, g_fn, (1,), 42) == 1


def test_special_values_pass_through_both_rings_alike(hip):
    """a NaN, an infinity and a zero column in the data: the same bits, NaN positions included, with two and with three slots"""
    nx, ny = 37, 252
    x, y, g_coeffs = _problem(nx, ny, "square", True, 43)
    x[5 * ny + 117] = np.nan; y[9 * ny + 3] = np.inf; y[20 * ny:21 * ny] = 0; y[nx * ny + 20 * ny:nx * ny + 21 * ny] = 0
    desc, keep = make_desc(hip, "2d", (nx, ny, 1), np.float32, ("square", "ind_leq0"), g_coeffs, TVAL)
    dx, dy = hip.DeviceArray.from_host(x), hip.DeviceArray.from_host(y)
    os.environ["PROST_ITERK_LEVELWAVE"] = "0"
    wx, wy = _launch_k(hip, C.byref(desc), 4, dx, dy, 0)          # the single-wave family: no ring of this kind
    os.environ.pop("PROST_ITERK_LEVELWAVE")
    assert np.isnan(wx).any()
    for cols in (0, 1, 7):
        got = {}
        for depth in (2, 3):
            _ring(depth)
            got[depth] = _launch_k(hip, C.byref(desc), 4, dx, dy, cols)
        _ring(2)
        assert _same(got[2][0], got[3][0]) and _same(got[2][1], got[3][1]), cols
        assert _same(got[2][0], wx) and _same(got[2][1], wy), cols
    dx.free(); dy.free()
    del keep


def test_the_rec_entry_runs_the_two_slot_instance(hip):
    L_ = hip.lib()
    L_.prost_hip_pdhg_rule_record_bytes.restype = C.c_size_t
    nx, ny = 37, 252
    x, y, g_coeffs = _problem(nx, ny, "square", True, 44)
    desc, keep = make_desc(hip, "2d", (nx, ny, 1), np.float32, ("square", "ind_leq0"), g_coeffs, TVAL)
    ref = C.byref(desc)
    dx, dy = hip.DeviceArray.from_host(x), hip.DeviceArray.from_host(y)
    rec = hip.DeviceArray(L_.prost_hip_pdhg_rule_record_bytes(), np.uint8)
    opts = (C.c_byte * 256)()          # prost_hip_pdhg_rule_opts, variant 0 = PROST_PDHG_RULE_NONE: nothing adapts the steps
    hip.check(L_.prost_hip_pdhg_rule_begin_f32(rec.ptr, opts, ref, hip.dbl(TAUS[0]), hip.dbl(SIGMAS[0]), hip.dbl(THETAS[0]), hip.dbl(0.5), 0, 0, 1, None, None))
    cur = (x, y)
    for k in range(4):
        x1, y1, _ = oracle_iteration("2d", cur[0], cur[1], (nx, ny, 1), g_coeffs, TVAL, TAUS[0], SIGMAS[0], THETAS[0], np.float32, "square", "ind_leq0")
        cur = (x1, y1)
    for cols in (0, 3):
        got = {}
        for depth in (2, 3):
            _ring(depth)
            xo = hip.DeviceArray.from_host(np.full(x.size, 7.0, np.float32)); yo = hip.DeviceArray.from_host(np.full(y.size, 7.0, np.float32))
            hip.check(L_.prost_hip_fused_iterationk_rec_f32(ref, 4, xo.ptr, yo.ptr, dx.ptr, dy.ptr, rec.ptr, cols, None, None, 0, C.c_ulonglong(0), None, None))
            got[depth] = xo.to_host(), yo.to_host()
            xo.free(); yo.free()
        _ring(2)
        assert _same(got[2][0], cur[0]) and _same(got[2][1], cur[1]), ("oracle", cols)
        assert _same(got[2][0], got[3][0]) and _same(got[2][1], got[3][1]), ("three slots", cols)
    dx.free(); dy.free(); rec.free()
    del keep


@pytest.mark.parametrize("period", [7, 10])
def test_the_solver_with_launches_of_four_equals_the_oracle(period):
    os.environ["PROST_PDHG_FOURS_MIN_PIXELS"] = "0"
    prob, u, q, f = synthetic.rof_problem(256, 248)
    b = prost.backend.pdhg(stepsize="alg2", residual_iter=period, alg2_gamma=0.5)
    o = prost.options(max_iters=10 ** 6, num_cback_calls=0, verbose=False, **ZERO_TOL)
    s = prost.Solver(prob, b, o)
    info = s.iterate(23, time_kernels=True, sample_every=1)
    st = s.state()
    s.destroy()
    assert st["arithmetic"] == "exact" and st["path"] == "pdhg:fused-grad2d" and "fused_iter2d_xk_kernel<4>" in info["kernels"], info["kernels"]
    os_ = oracle.Solver(prob.data, prob.nrows, prob.ncols, b, o, np.float32)
    os_.initialize(); os_.iterate(23)
    ost = os_.state()
    del os_
    for v in "xyzw":
        assert _same(st[v], ost[v]), (v, period, int((st[v] != ost[v]).sum()))


def _rule(n, slots=1024, lo=6, hi=72):
    """lw_one_round_cols: the shortest chunk in [lo, hi] whose workgroups run in one round of four per CU (the round of five that the
    two-slot instance fits was measured slower at every size and is not used: docs/rounds/r31.md)"""
    strips = -(-n // 248)
    for c in range(lo, hi + 1):
        if strips * -(-n // c) <= slots:
            return c
    return hi


def test_the_chunk_length_reported_for_per_pixel_b_is_the_rule(hip):
    L_ = hip.lib()
    b = hip.DeviceArray.zeros(64, np.float32)          # a per-pixel b: only asked whether it is there
    assert [_rule(n) for n in (1024, 2048, 3072, 4096, 8192)] == [6, 19, 40, 69, 72]
    for n in (1024, 2048, 3072, 4096, 8192):
        d = hip.FusedDesc(); d.is3d = 0; d.nx, d.ny, d.L = n, n, 1
        d.g_fn = hip.FN_ID["square"]; d.f_fn = hip.FN_ID["ind_leq0"]
        for i, (g, fv) in enumerate(zip([1, 0, 10, 0, 0, 0, 0], [1, 1, 1, 0, 0, 0, 0])):
            d.g_coeff_val[i] = g; d.f_coeff_val[i] = fv
        d.g_coeff_ptr[1] = b.ptr.value
        d.T_val, d.S_val = 0.25, 0.5
        d.arith = 0
        for depth in (2, 3):
            _ring(depth)
            for K in (3, 4):
                assert L_.prost_hip_fused_iterationk_chunk_cols(C.byref(d), 0, K, 0) == _rule(n), (n, K, depth)
        _ring(2)
        os.environ["PROST_ITERK4_COLS"] = "55"
        assert L_.prost_hip_fused_iterationk_chunk_cols(C.byref(d), 0, 4, 0) == 55 and L_.prost_hip_fused_iterationk_chunk_cols(C.byref(d), 0, 3, 0) == _rule(n)
        os.environ.pop("PROST_ITERK4_COLS")
    b.free()
