"""The level-per-wavefront K-iteration kernel (fused_iter2d_xkw_kernel, K = 3 and 4) at the chunk lengths of the one-round rule
(lw_one_round_cols, prost_amd/csrc/iterk_levelwave.hpp) and on grids of more than three workgroups per CU.

Every comparison is bit for bit (np.array_equal) against tests/pdhg_iteration_reference.py (the CPU oracle's pieces, K iterations) and
against K launches of the single-iteration kernel; 'square' and 'abs', scalar and per-pixel b, different step sizes per level:
  * nx in {8, 9, 37}, ny in {8, 248, 252}, forced chunks of 2, 3 and 7 columns (last chunks of 1, 2, 3 columns);
  * nx = 300, ny = 500 with chunks of one column: 900 workgroups, more than three rounds of 256 -- every CU holds workgroups b, b + 256,
    b + 512 (and b + 768), whose waves the hardware starts on different SIMDs (docs/rounds/r26.md);
  * nx = 150, ny = 500 with chunks of 19 and 69 columns, the lengths the rule gives 2048^2 and 4096^2;
  * the solver at 256 x 248 with launches of four (auto chunk length), periods 7 and 10, 23 iterations, against oracle.Solver;
  * the _rec entry with the record's stop word raised returns before the first barrier: the outputs stay untouched.

The level rotation planned beside the rule was measured and not built (docs/rounds/r26.md): there is no rotation to force here.
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
from test_gpu_iterk_levelwave import SIGMAS, TAUS, THETAS, TVAL, ZERO_TOL, _arr, _launch_k, _problem

pytestmark = pytest.mark.gpu

VARIANTS = (("square", True), ("square", False), ("abs", True), ("abs", False))


@pytest.fixture(autouse=True)
def _gpu(hip):
    prost.set_gpu(0)
    prost.set_precision("single")
    old = {k: os.environ.get(k) for k in ("PROST_ITERK_LEVELWAVE", "PROST_ITERK3_COLS", "PROST_ITERK4_COLS", "PROST_PDHG_FOURS_MIN_PIXELS")}
    for k in ("PROST_ITERK_LEVELWAVE", "PROST_ITERK3_COLS", "PROST_ITERK4_COLS"):
        os.environ.pop(k, None)
    yield
    for k, v in old.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
    prost.set_precision("double")


def _check(hip, nx, ny, g_fn, bpp, chunks, seed):
    """launches of K = 3 and 4 at every chunk length against the oracle's iterates and against K single launches; returns the launches run"""
    L_ = hip.lib()
    shape = (nx, ny, 1)
    x, y, g_coeffs = _problem(nx, ny, g_fn, bpp, seed)
    its = [(x, y)]
    for k in range(4):
        x1, y1, _ = oracle_iteration("2d", its[-1][0], its[-1][1], shape, g_coeffs, TVAL, TAUS[k], SIGMAS[k], THETAS[k], np.float32, g_fn, "ind_leq0")
        its.append((x1, y1))
    desc, keep = make_desc(hip, "2d", shape, np.float32, (g_fn, "ind_leq0"), g_coeffs, TVAL)
    ref = C.byref(desc)
    dx, dy = hip.DeviceArray.from_host(x), hip.DeviceArray.from_host(y)
    cur = (dx, dy); singles = []
    for k in range(4):
        nxt = (hip.DeviceArray.zeros(x.size, np.float32), hip.DeviceArray.zeros(y.size, np.float32))
        hip.check(L_.prost_hip_fused_iteration_f32(ref, nxt[0].ptr, nxt[1].ptr, cur[0].ptr, cur[1].ptr, None, hip.dbl(TAUS[k]), hip.dbl(SIGMAS[k]), hip.dbl(THETAS[k]),
                                                   1, 1, 0, 0, None, None, None))
        singles.append(nxt); cur = nxt
    launches = 0
    for K in (3, 4):
        sx, sy = singles[K - 1][0].to_host(), singles[K - 1][1].to_host()
        for cols in chunks:
            gx, gy = _launch_k(hip, ref, K, dx, dy, cols)
            assert np.array_equal(gx, its[K][0]), ("x", nx, ny, g_fn, bpp, K, cols, int((gx != its[K][0]).sum()))
            assert np.array_equal(gy, its[K][1]), ("y", nx, ny, g_fn, bpp, K, cols, int((gy != its[K][1]).sum()))
            assert np.array_equal(gx, sx) and np.array_equal(gy, sy), ("single launches", nx, ny, g_fn, bpp, K, cols)
            launches += 1
    for a in [dx, dy] + [v for pair in singles for v in pair]:
        a.free()
    del keep
    return launches


@pytest.mark.parametrize("nx", [8, 9, 37])
def test_short_and_odd_chunks_equal_the_oracle_and_single_launches(hip, nx):
    """chunks of 2, 3 and 7 columns: at nx = 8, 9 and 37 the last chunk of seven-column chunks is 1, 2 and 2 columns, of three-column
    chunks 2 (cols - 1), 3 and 1, of two-column chunks 2, 1 and 1"""
    launches = 0
    for ny in (8, 248, 252):
        for g_fn, bpp in VARIANTS:
            launches += _check(hip, nx, ny, g_fn, bpp, (2, 3, 7), 2000 * nx + ny)
    assert launches == 3 * 4 * 2 * 3


@pytest.mark.parametrize("g_fn,bpp", VARIANTS)
def test_a_grid_of_900_workgroups_equals_the_oracle(hip, g_fn, bpp):
    """300 x 500 in chunks of one column: 3 strips x 300 chunks, so CUs hold up to four workgroups of the launch at once"""
    assert _check(hip, 300, 500, g_fn, bpp, (1,), 31) == 2


@pytest.mark.parametrize("g_fn,bpp", VARIANTS)
def test_the_lengths_of_the_rule_at_2048_and_4096_equal_the_oracle(hip, g_fn, bpp):
    """150 columns in chunks of 19 (last chunk 17) and 69 (last chunk 12)"""
    assert _check(hip, 150, 500, g_fn, bpp, (19, 69), 32) == 4


def test_the_chunk_length_reported_is_the_one_round_rule(hip):
    L_ = hip.lib()
    for n, want in ((1024, 6), (2048, 19), (3072, 40), (4096, 69), (8192, 72)):
        d = hip.FusedDesc(); d.is3d = 0; d.nx, d.ny, d.L = n, n, 1
        d.g_fn = hip.FN_ID["square"]; d.f_fn = hip.FN_ID["ind_leq0"]
        for i, (g, fv) in enumerate(zip([1, 0, 10, 0, 0, 0, 0], [1, 1, 1, 0, 0, 0, 0])):
            d.g_coeff_val[i] = g; d.f_coeff_val[i] = fv
        d.T_val, d.S_val = 0.25, 0.5
        d.arith = 0
        for K in (3, 4):
            assert L_.prost_hip_fused_iterationk_chunk_cols(C.byref(d), 0, K, 0) == want, (n, K)
        os.environ["PROST_ITERK4_COLS"] = "72"
        assert L_.prost_hip_fused_iterationk_chunk_cols(C.byref(d), 0, 4, 0) == 72 and L_.prost_hip_fused_iterationk_chunk_cols(C.byref(d), 0, 3, 0) == want
        os.environ.pop("PROST_ITERK4_COLS")


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
        assert np.array_equal(st[v], ost[v]), (v, period, int((st[v] != ost[v]).sum()))


def test_the_rec_entry_returns_before_the_first_barrier_when_stopped(hip):
    L_ = hip.lib()
    L_.prost_hip_pdhg_rule_record_bytes.restype = C.c_size_t
    nx, ny = 37, 252
    x, y, g_coeffs = _problem(nx, ny, "square", True, 5)
    desc, keep = make_desc(hip, "2d", (nx, ny, 1), np.float32, ("square", "ind_leq0"), g_coeffs, TVAL)
    ref = C.byref(desc)
    dx, dy = hip.DeviceArray.from_host(x), hip.DeviceArray.from_host(y)
    rec = hip.DeviceArray(L_.prost_hip_pdhg_rule_record_bytes(), np.uint8)
    opts = (C.c_byte * 256)()          # prost_hip_pdhg_rule_opts, variant 0 = PROST_PDHG_RULE_NONE
    hip.check(L_.prost_hip_pdhg_rule_begin_f32(rec.ptr, opts, ref, hip.dbl(TAUS[0]), hip.dbl(SIGMAS[0]), hip.dbl(THETAS[0]), hip.dbl(0.5), 0, 0, 1, None, None))
    stop = C.POINTER(C.c_int)()
    hip.check(L_.prost_hip_pdhg_record_view(rec.ptr, 0, None, None, None, C.byref(stop)))
    one = np.ones(1, np.int32)
    hip.check(L_.prost_hip_memcpy_h2d(stop, one.ctypes.data_as(C.c_void_p), C.c_size_t(4), None)); hip.sync()
    for K in (3, 4):
        for cols in (0, 7):
            xo = hip.DeviceArray.from_host(np.full(x.size, 7.0, np.float32)); yo = hip.DeviceArray.from_host(np.full(y.size, 7.0, np.float32))
            hip.check(L_.prost_hip_fused_iterationk_rec_f32(ref, K, xo.ptr, yo.ptr, dx.ptr, dy.ptr, rec.ptr, cols, None, None, 0, C.c_ulonglong(0), None, None))
            hip.sync()
            assert (xo.to_host() == 7.0).all() and (yo.to_host() == 7.0).all(), (K, cols)
            xo.free(); yo.free()
    dx.free(); dy.free(); rec.free()
    del keep
