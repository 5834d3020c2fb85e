"""The level-per-wavefront K-iteration kernel (fused_iter2d_xkw_kernel, K = 3 and 4) computes on register PAIRS: a lane's four rows
are the pairs (0, 1) and (2, 3), and the exact helpers have 2-wide forms (device_math.hpp).  What pairing can break is the position
of a row inside its pair and its lane, so the directed cases below put ONE special operand into one row at a time.

Every comparison is bit for bit, NaN positions included, over the whole image (so the other row of the pair, the other pair of the
lane and the neighbouring lanes are compared too), against two independent statements of the same bits:
  * K launches of the single-iteration kernel;
  * the single-wave family (PROST_ITERK_LEVELWAVE=0), which keeps the scalar expressions.

  * rows: ny = 252 is two strips; rows 116 .. 119 are the four rows of lane 30 of strip 0, rows 244 .. 247 those of lane 62 of strip 0
    and of lane 0 (halo) of strip 1, rows 248 .. 251 those of lane 63 (halo) of strip 0 and of lane 1 of strip 1.  Each of these twelve
    rows in turn holds: a NaN, +inf, dual components whose squared norm exceeds 2^126 (general path of the prox), a zero norm, -0 in x
    with zero divergence, and an x for which div_to_float_exact_vec must take the full division (asserted with NumPy before the launch);
  * shapes: nx in {8, 9, 37}, ny in {8, 248, 252}, the chunk rule and forced chunks of 2, 3, 7 columns, K in {3, 4}, 'square' and
    'abs', scalar and per-pixel b, different step sizes per level; the _rec entry once;
  * the solver at 256 x 248, period 10, 23 iterations, against oracle.Solver.
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
from test_gpu_iterk_levelwave import SIGMAS, THETAS, TVAL, ZERO_TOL, _arr, _problem, _same

pytestmark = pytest.mark.gpu

# The first step size decides whether a full-division operand EXISTS.  The divisor of Function1DSquare is D = 1. + 8 tau T.  A quotient
# of a 24-bit x by a D of 24 bits is never within 2^-49 (8 units of a double) of a float rounding boundary, so steps in [1, 2) -- and
# 0.5 tau T = 1 / 16, where D = 2 and the quotient is exact -- leave the +-4 window of div_to_float_exact_vec unreachable; a step
# below 1 / 2 gives D 26 bits or more, and then about one significand in 6 x 10^7 falls into it: of the 2^23 there are, none for most
# step sizes.  tau = 0.06 (D = 1.12 - 2.7e-9) has one, 0.49777773 (two units from the boundary); _full_division_operand searches for
# it and the test asserts what it found, so a change of these numbers cannot turn the case into one that never leaves the fast path.
TAUS = (0.06, 0.7, 0.6, 0.45)
VARIANTS = (("square", True), ("square", False), ("abs", True), ("abs", False))
NX, NY, COL = 9, 252, 4
ROWS = tuple(range(116, 120)) + tuple(range(244, 252))
KINDS = ("nan", "inf", "big", "zero", "negzero", "fulldiv")


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


def _launch(hip, ref, K, dx, dy, cols, levelwave=True):
    """one launch of K iterations (level per wavefront, or the single-wave family) into fresh buffers; returns (x, y) on the host"""
    if levelwave:
        os.environ.pop("PROST_ITERK_LEVELWAVE", None)
    else:
        os.environ["PROST_ITERK_LEVELWAVE"] = "0"
    xo = hip.DeviceArray.from_host(np.full(dx.n, 7.0, np.float32)); yo = hip.DeviceArray.from_host(np.full(dy.n, 7.0, np.float32))
    hip.check(hip.lib().prost_hip_fused_iterationk_f32(ref, K, xo.ptr, yo.ptr, dx.ptr, dy.ptr, _arr(TAUS, K), _arr(SIGMAS, K), _arr(THETAS, K), cols, None, None, None))
    os.environ.pop("PROST_ITERK_LEVELWAVE", None)
    out = xo.to_host(), yo.to_host()
    xo.free(); yo.free()
    return out


def _compare(hip, x, y, shape, g_fn, g_coeffs, chunks, tag):
    """K = 3 and 4 at every chunk length against K single launches and against the single-wave family; returns the launches compared"""
    L_ = hip.lib()
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
        wx, wy = _launch(hip, ref, K, dx, dy, 0, levelwave=False)
        assert _same(wx, sx) and _same(wy, sy), ("the single-wave family against single launches", tag, K)
        for cols in chunks:
            gx, gy = _launch(hip, ref, K, dx, dy, cols)
            assert _same(gx, sx), ("x against single launches", tag, K, cols, np.flatnonzero(~((gx == sx) | (np.isnan(gx) & np.isnan(sx))))[:8])
            assert _same(gy, sy), ("y against single launches", tag, K, cols, np.flatnonzero(~((gy == sy) | (np.isnan(gy) & np.isnan(sy))))[:8])
            assert _same(gx, wx) and _same(gy, wy), ("against the single-wave family", tag, K, cols)
            assert not (gx == 7.0).any() and not (gy == 7.0).any(), ("an element was not written", tag, K, cols)
            launches += 1
    for a in [dx, dy] + [v for pair in singles for v in pair]:
        a.free()
    del keep
    return launches


def _square_divisor(tau):
    """1. + step of Function1DSquare as make_uniform_prox forms it (c = 8, a = 1, e = 0): float products, the sum in double"""
    tau_t = np.float32(tau) * np.float32(TVAL)
    step = np.float32(8.0) * np.float32(1.0) * np.float32(1.0) * tau_t
    assert step.dtype == np.float32
    return 1.0 + float(step)


def _window_distance(v, D):
    """distance of the 29 bits a float drops from q0 = float64(v) * (1 / D) to the tie pattern 2^28"""
    q0 = np.asarray(v, np.float32).astype(np.float64) * (1.0 / D)
    return np.abs((q0.view(np.uint64) & np.uint64(0x1FFFFFFF)).astype(np.int64) - (1 << 28))


def _full_division_operand(D):
    """the first float of [0.25, 0.5) -- every significand once; other binades repeat them -- whose fast quotient by D lies within +-4
    units of a float rounding boundary"""
    start = int(np.float32(0.25).view(np.uint32))
    for chunk in range(2):
        bits = np.arange(start + (chunk << 22), start + ((chunk + 1) << 22), dtype=np.uint32)
        hit = np.flatnonzero(_window_distance(bits.view(np.float32), D) <= 4)
        if hit.size:
            return bits[hit[0]:hit[0] + 1].view(np.float32)[0]
    raise AssertionError("no operand found")


_OPERAND = {}


def _directed(kind, r):
    """random data with ONE special operand at column COL, row r; returns x, b, y and checks with NumPy that the operand is what it claims"""
    n = NX * NY
    x, y, g_coeffs = _problem(NX, NY, "square", True, 77)
    x, y, b = x.copy(), y.copy(), g_coeffs[1].copy()
    at = COL * NY + r
    patch = [c * NY + q for c in (COL - 1, COL, COL + 1) for q in (r - 1, r, r + 1) if 0 <= q < NY]
    if kind == "nan":
        x[at] = np.nan
    elif kind == "inf":
        x[at] = np.inf
    elif kind == "big":
        y[at], y[n + at] = np.float32(1.5 * 2.0 ** 63), np.float32(2.0 ** 63)
    else:          # zero divergence at the pixel and its right and lower neighbours
        y[patch] = 0; y[[n + p for p in patch]] = 0
        if kind == "zero":
            for p in (at, at + NY) + ((at + 1,) if r + 1 < NY else ()):
                x[p], b[p] = 0.5, 0.25
        elif kind == "negzero":
            x[at], b[at] = -0.0, 0.0
        else:
            D = _square_divisor(TAUS[0])
            if D not in _OPERAND:
                _OPERAND[D] = _full_division_operand(D)
            x[at], b[at] = _OPERAND[D], 0.0
    g_coeffs = [1.0, b, 8.0, 0.0, 0.0, 0.3, 0.0]
    x1, y1, nv = oracle_iteration("2d", x, y, (NX, NY, 1), g_coeffs, TVAL, TAUS[0], SIGMAS[0], THETAS[0], np.float32, "square", "ind_leq0")
    if kind == "nan":
        assert np.isnan(x1[at]) and np.isnan(nv[at])
    elif kind == "inf":
        assert np.isposinf(x1[at])
    elif kind == "big":
        assert 2.0 ** 126 < nv[at] < 2.0 ** 128          # (x^1 carries it to the pixels around; the reference does the same)
    elif kind == "zero":
        assert nv[at] == 0 and np.count_nonzero(nv == 0) == 1
    else:
        kty = oracle.grad2d(y, NX, NY, 1, adjoint=True)
        assert kty[at] == 0 and b[at] == 0
        parg = np.float32(np.float32(x[at] - np.float32(TAUS[0]) * np.float32(TVAL) * kty[at]) - b[at])
        if kind == "negzero":
            assert parg == 0 and np.signbit(parg)
        else:
            D = _square_divisor(TAUS[0])
            assert D != 2.0 ** np.round(np.log2(D)) and _window_distance(parg, D) <= 4, (parg, D)          # the wave takes the full division
    return x, y, g_coeffs


@pytest.mark.parametrize("kind", KINDS)
def test_one_special_operand_in_one_row_of_one_lane(hip, kind):
    launches = 0
    for r in ROWS:
        x, y, g_coeffs = _directed(kind, r)
        launches += _compare(hip, x, y, (NX, NY, 1), "square", g_coeffs, (0, 3), (kind, r))
    assert launches == len(ROWS) * 2 * 2


@pytest.mark.parametrize("nx", [8, 9, 37])
def test_pairs_at_every_seam_of_the_shapes(hip, nx):
    launches = 0
    for ny in (8, 248, 252):
        for g_fn, bpp in VARIANTS:
            x, y, g_coeffs = _problem(nx, ny, g_fn, bpp, 2800 + 10 * nx + ny)
            launches += _compare(hip, x, y, (nx, ny, 1), g_fn, g_coeffs, (0, 2, 3, 7), (nx, ny, g_fn, bpp))
    assert launches == 3 * 4 * 2 * 4


def test_the_rec_entry_runs_the_same_pairs(hip):
    L_ = hip.lib()
    L_.prost_hip_pdhg_rule_record_bytes.restype = C.c_size_t
    nx, ny = 37, 252
    x, y, g_coeffs = _problem(nx, ny, "square", True, 28)
    desc, keep = make_desc(hip, "2d", (nx, ny, 1), np.float32, ("square", "ind_leq0"), g_coeffs, TVAL)
    ref = C.byref(desc)
    dx, dy = hip.DeviceArray.from_host(x), hip.DeviceArray.from_host(y)
    rec = hip.DeviceArray(L_.prost_hip_pdhg_rule_record_bytes(), np.uint8)
    opts = (C.c_byte * 256)()          # prost_hip_pdhg_rule_opts, variant 0 = PROST_PDHG_RULE_NONE: nothing adapts the steps
    hip.check(L_.prost_hip_pdhg_rule_begin_f32(rec.ptr, opts, ref, hip.dbl(TAUS[0]), hip.dbl(SIGMAS[0]), hip.dbl(THETAS[0]), hip.dbl(0.5), 0, 0, 1, None, None))
    for K in (3, 4):
        xo = hip.DeviceArray.from_host(np.full(x.size, 7.0, np.float32)); yo = hip.DeviceArray.from_host(np.full(y.size, 7.0, np.float32))
        hip.check(L_.prost_hip_fused_iterationk_rec_f32(ref, K, xo.ptr, yo.ptr, dx.ptr, dy.ptr, rec.ptr, 0, None, None, 0, C.c_ulonglong(0), None, None))
        os.environ["PROST_ITERK_LEVELWAVE"] = "0"
        want = hip.DeviceArray.zeros(x.size, np.float32), hip.DeviceArray.zeros(y.size, np.float32)
        hip.check(L_.prost_hip_fused_iterationk_f32(ref, K, want[0].ptr, want[1].ptr, dx.ptr, dy.ptr, _arr(TAUS[:1] * 4, K), _arr(SIGMAS[:1] * 4, K), _arr(THETAS[:1] * 4, K),
                                                    0, None, None, None))
        os.environ.pop("PROST_ITERK_LEVELWAVE", None)
        assert np.array_equal(xo.to_host(), want[0].to_host()) and np.array_equal(yo.to_host(), want[1].to_host()), K
        for a in (xo, yo) + want:
            a.free()
    dx.free(); dy.free(); rec.free()
    del keep


def test_the_solver_with_launches_of_four_equals_the_oracle():
    os.environ["PROST_PDHG_FOURS_MIN_PIXELS"] = "0"
    prob, u, q, f = synthetic.rof_problem(256, 248)
    b = prost.backend.pdhg(stepsize="alg2", residual_iter=10, alg2_gamma=0.5)
    o = prost.options(max_iters=10 ** 6, num_cback_calls=0, verbose=False, **ZERO_TOL)
    s = prost.Solver(prob, b, o)
    info = s.iterate(23, time_kernels=True, sample_every=1)
    st = s.state()
    s.destroy()
    assert st["arithmetic"] == "exact" and "fused_iter2d_xk_kernel<4>" in info["kernels"], info["kernels"]
    os_ = oracle.Solver(prob.data, prob.nrows, prob.ncols, b, o, np.float32)
    os_.initialize(); os_.iterate(23)
    ost = os_.state()
    del os_
    for v in "xyzw":
        assert np.array_equal(st[v], ost[v]), (v, int((st[v] != ost[v]).sum()))
