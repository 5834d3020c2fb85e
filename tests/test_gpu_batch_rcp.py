"""The dual prox with reciprocals shared between the pixels of a lane (device_math.hpp: norm2_leq0_fast, batch_rcp.hpp).

A lane of the fused kernels owns consecutive rows of a column and divides by their norms through refined double reciprocals that
come from one seed per two pixels.  The quotients must stay the correctly rounded ones, so x^(k+2), y^(k+2) of a pair launch and
the iterates of a solver run equal the CPU oracle bit for bit -- here on data that puts the extremes of the divisor range into ONE
lane: in the marked lanes (rows 4j .. 4j+3 of every column) row 4j has a zero gradient (the norm is clamped to 2^-48), row 4j+1
ordinary values, row 4j+3 a norm near 2^60 (a dual variable of that size in the first horizontal component, which moves x^(k+1) in
its own row only), row 4j+2 ordinary or large ones (its vertical difference reaches into row 4j+3, which x^(k+1) leaves where the
signs of two neighbouring columns differ); the other lanes hold ordinary values throughout.  The seed is shared by rows (4j, 4j+1)
and (4j+2, 4j+3), so a second pattern puts the norm near 2^60 into row 4j+1: the clamp 2^-48 and 2^60 under ONE seed.  One further
case puts a norm above 2^63 into a lane: the whole vector then takes the general expansions.
"""
import ctypes as C

import numpy as np
import pytest

import oracle
import prost_amd as prost
from pdhg_iteration_reference import F_COEFFS, SVAL, oracle_iteration
from prost_amd import synthetic

pytestmark = pytest.mark.gpu

DT = np.float32
TAUS, SIGMAS, THETAS = (0.9, 0.7), (1.1, 1.4), (0.85, 0.8)
HUGE = 1.3 * 2.0 ** 60
SHAPES = [(nx, ny) for nx in (5, 19, 37) for ny in (8, 248, 252)]


def marked_lanes(ny, rng):
    """which groups of four rows carry the pattern: every other one at least, the first and the last always"""
    k = ny // 4
    m = rng.random(k) < 0.5
    m[0] = m[-1] = True
    return m


def patterned(nx, ny, planes, comps, huge_comps, rng, huge_row=3):
    """x, f (planes, nx, ny) and y (comps, nx, ny) in the kernels' layout (rows fastest), and the marked lanes.  huge_comps: horizontal
    difference components (K^T y takes them from the pixel's own row only).  huge_row = 1: the huge dual variable sits in the flat row
    4j+1 with ONE sign, so that K^T y cancels between neighbouring columns and x^(k+1) stays flat away from the first and last column"""
    x = rng.uniform(0, 1, (planes, nx, ny)); f = rng.uniform(0, 1, (planes, nx, ny)); y = rng.uniform(-1, 1, (comps, nx, ny))
    m = marked_lanes(ny, rng)
    others = np.setdiff1d(np.arange(comps), huge_comps)
    for j in np.flatnonzero(m):
        r = 4 * j
        x[:, :, r:r + 2] = rng.uniform(0, 1); f[:, :, r:r + 2] = rng.uniform(0, 1)      # flat: K x = 0 at row r, and K^T y = 0 on both rows keeps it flat
        y[:, :, r:r + 2] = 0.0
        for q in (r - 1, r + 3):             # no vertical (or plane) component reaches from here into a flat row
            if q >= 0:
                y[others, :, q] = 0.0
        if huge_row == 3:
            y[huge_comps, :, r + 3] = HUGE * np.where(rng.random((len(huge_comps), nx)) < 0.5, -1.0, 1.0)
        else:
            y[huge_comps, :, r + 1] = HUGE
    return x.reshape(-1).astype(DT), f.reshape(-1).astype(DT), y.reshape(-1).astype(DT), m


def fused_desc(hip, kind, shape, g_coeffs, tval):
    nx, ny, L = shape
    n = nx * ny * L
    d = hip.FusedDesc()
    d.is3d = 1 if kind == "3d" else 0; d.nx, d.ny, d.L = nx, ny, L
    d.g_fn = hip.FN_ID["square"]; d.f_fn = hip.FN_ID["ind_leq0"]
    gp, gv, k1 = hip.coeff_args(g_coeffs, DT, n)
    fp, fv, k2 = hip.coeff_args(F_COEFFS, DT, n)
    for i in range(7):
        d.g_coeff_ptr[i] = gp[i]; d.g_coeff_val[i] = gv[i]
        d.f_coeff_ptr[i] = fp[i]; d.f_coeff_val[i] = fv[i]
    d.T_val, d.S_val = tval, SVAL
    return d, (k1, k2)


def pair_launch_against_oracle(hip, kind, shape, x, f, y, tval, chunk_cols):
    nx, ny, L = shape
    g_coeffs = [1.0, f, 10.0, 0.0, 0.0, 0.3, 0.0]
    x1, y1, nv1 = oracle_iteration(kind, x, y, shape, g_coeffs, tval, TAUS[0], SIGMAS[0], THETAS[0])
    x2, y2, _ = oracle_iteration(kind, x1, y1, shape, g_coeffs, tval, TAUS[1], SIGMAS[1], THETAS[1])
    desc, keep = fused_desc(hip, kind, shape, g_coeffs, tval)
    arr = lambda v: (C.c_double * 2)(*v)
    dx, dy = hip.DeviceArray.from_host(x), hip.DeviceArray.from_host(y)
    for cols in chunk_cols:
        xo = hip.DeviceArray.from_host(np.full(x.size, 7.0, DT)); yo = hip.DeviceArray.from_host(np.full(y.size, 7.0, DT))
        if kind == "2d":
            assert hip.lib().prost_hip_fused_iteration2_profitable(C.byref(desc), 0) == 1
            hip.check(hip.fn("fused_iteration2", DT)(C.byref(desc), xo.ptr, yo.ptr, dx.ptr, dy.ptr, None, None, arr(TAUS), arr(SIGMAS), arr(THETAS), cols, None, None, None))
        else:
            name = "fused_iteration3d_x2" if kind == "3d" else "fused_iteration_mc_x2"
            assert getattr(hip.lib(), "prost_hip_" + name + "_supported")(C.byref(desc), 0) == 1
            hip.check(hip.fn(name, DT)(C.byref(desc), xo.ptr, yo.ptr, dx.ptr, dy.ptr, arr(TAUS), arr(SIGMAS), arr(THETAS), cols, None, None, None))
        gx, gy = xo.to_host(), yo.to_host()
        xo.free(); yo.free()
        assert np.array_equal(gx, x2), (kind, shape, cols, np.flatnonzero(gx != x2)[:8])
        assert np.array_equal(gy, y2), (kind, shape, cols, np.flatnonzero(gy != y2)[:8])
    dx.free(); dy.free()
    del keep
    return nv1


def check_classes(nv, shape, marked, planes):
    """the first iteration's squared norms in every marked lane: zero (row 4j), ordinary (4j+1), near 2^120 (4j+3); nothing above 2^126.
    (A volume's last plane has no zero gradient: the reference's difference across planes ends with a Dirichlet condition, -x.)"""
    nx, ny, L = shape
    nv = nv.reshape(planes, nx, ny)
    assert nv.max() <= 2.0 ** 126
    for j in np.flatnonzero(marked):
        r = 4 * j
        assert np.all(nv[:max(planes - 1, 1), :, r] == 0.0), j
        assert np.all((nv[:, :, r + 1] > 2.0 ** -30) & (nv[:, :, r + 1] < 2.0 ** 10)), j
        assert np.all((nv[:, :, r + 3] >= 2.0 ** 118) & (nv[:, :, r + 3] <= 2.0 ** 123)), j


@pytest.mark.parametrize("nx,ny", SHAPES)
def test_pair_launch_with_the_extremes_of_the_divisor_range_in_one_lane(hip, nx, ny):
    rng = np.random.default_rng(100 * nx + ny)
    x, f, y, m = patterned(nx, ny, 1, 2, [0], rng)
    # the launcher's chunk length, and chunks of two columns: a seam next to every other column
    nv = pair_launch_against_oracle(hip, "2d", (nx, ny, 1), x, f, y, 0.25, (0, 2))
    check_classes(nv, (nx, ny, 1), m, 1)


@pytest.mark.parametrize("nx,ny", [(19, 248), (37, 8)])
def test_pair_launch_with_the_clamp_and_a_norm_near_2_60_under_one_seed(hip, nx, ny):
    rng = np.random.default_rng(5000 + 100 * nx + ny)
    x, f, y, m = patterned(nx, ny, 1, 2, [0], rng, huge_row=1)
    nv = pair_launch_against_oracle(hip, "2d", (nx, ny, 1), x, f, y, 0.25, (0, 2)).reshape(nx, ny)
    assert nv.max() <= 2.0 ** 126
    for j in np.flatnonzero(m):
        r = 4 * j
        assert np.all(nv[1:-1, r] == 0.0), j                                                    # the clamped norm ...
        assert np.all((nv[:, r + 1] >= 2.0 ** 118) & (nv[:, r + 1] <= 2.0 ** 123)), j           # ... and its partner under the same seed


def test_pair_launch_with_a_norm_above_the_short_forms_range(hip):
    """one pixel with a norm of 1.5 * 2^63: its squared norm is above 2^126, the lane's four pixels -- a zero gradient and ordinary
    values among them -- take the general expansions"""
    nx, ny = 19, 248
    rng = np.random.default_rng(7)
    x, f, y, m = patterned(nx, ny, 1, 2, [0], rng)
    j = int(np.flatnonzero(m)[1])
    y.reshape(2, nx, ny)[0, 3, 4 * j + 3] = DT(1.5 * 2.0 ** 63)
    nv = pair_launch_against_oracle(hip, "2d", (nx, ny, 1), x, f, y, 0.25, (0, 2))
    nv = nv.reshape(nx, ny)
    assert np.isfinite(nv).all() and (nv > 2.0 ** 126).sum() == 1 and nv[3, 4 * j + 3] > 2.0 ** 126 and nv[3, 4 * j] == 0.0


def test_volume_pair_launch(hip):
    nx, ny, L = 32, 32, 8
    x, f, y, m = patterned(nx, ny, L, 3 * L, list(range(L)), np.random.default_rng(11))
    nv = pair_launch_against_oracle(hip, "3d", (nx, ny, L), x, f, y, 1.0 / 6.0, (0, 5))
    check_classes(nv, (nx, ny, L), m, L)


def test_rgb_pair_launch(hip):
    nx, ny, L = 6, 8, 3
    x, f, y, m = patterned(nx, ny, L, 2 * L, [0], np.random.default_rng(12))
    nv = pair_launch_against_oracle(hip, "mc", (nx, ny, L), x, f, y, 0.25, (0, 2))
    check_classes(nv, (nx, ny, 1), m, 1)


@pytest.mark.parametrize("nx,ny", SHAPES)
def test_four_solver_iterations_equal_the_oracle(nx, ny):
    """ROF on an image with flat rows and jumps of 2^60 in the marked lanes: pair launches wherever the launch plan puts them (alg2, no residual iteration
    among the four), iterates identical to the CPU oracle's"""
    rng = np.random.default_rng(1000 + 100 * nx + ny)
    f = rng.uniform(0, 1, (nx, ny))
    for j in np.flatnonzero(marked_lanes(ny, rng)):
        f[:, 4 * j:4 * j + 2] = rng.uniform(0, 1)
        f[:, 4 * j + 3] = HUGE * np.where(rng.random(nx) < 0.5, -1.0, 1.0)
    prost.set_precision("single")
    prob, u, q, _ = synthetic.rof_problem(nx, ny, f=f.reshape(-1))
    backend = prost.backend.pdhg(stepsize="alg2", residual_iter=10, alg2_gamma=0.5)
    opts = prost.options(max_iters=10 ** 6, num_cback_calls=0, verbose=False, tol_rel_primal=0, tol_rel_dual=0, tol_abs_primal=0, tol_abs_dual=0)
    s = prost.Solver(prob, backend, opts)
    s.iterate(4)
    st = s.state()
    s.destroy()
    assert st["path"] == "pdhg:fused-grad2d" and int(st["pair_launches"]) >= 1, (st["path"], st["pair_launches"])
    o = oracle.Solver(prob.data, prob.nrows, prob.ncols, backend, opts, DT)
    o.initialize()
    o.iterate(4)
    ost = o.state()
    for v in "xy":
        assert np.array_equal(st[v], ost[v]), (nx, ny, v, np.flatnonzero(st[v] != ost[v])[:8])
    with np.errstate(over="ignore"):
        assert np.abs(ost["y"]).max() <= 1.0 and np.abs(ost["x"]).max() > 2.0 ** 50      # the jumps are still there; the dual variable stays in the unit ball
