"""The paired march of the two-iterations kernel (kernels_fused_iter2.hip, iter2_grid.hpp).

A plain launch of the exact fp32 straight-line instances (square / abs data term, prox_f* = norm2:ind_leq0, height a multiple of 4)
runs workgroups of two wavefronts that start at the seam between their chunks, march away from it and exchange three seam columns
through LDS.  Every pixel is computed by the same expressions from the same operands as before, so x^(k+2), y^(k+2) must equal two
single-iteration launches (fused_iter2d_kernel) and the CPU oracle bit for bit -- for every position of a seam relative to the image
border, every remainder of the last chunk, odd chunk counts (a pair without its second chunk) and strips with few active lanes.
Short chunks come from the launcher's chunk-length argument, so the images stay tiny.

Launches that also form the residual sums are NOT paired (a left-marching wave would add its columns in the opposite order): their
sums are therefore the parent's bit for bit by construction; here they are held to the single-iteration kernel's sums with the
tolerance the existing pair-kernel test uses for the fp32 straight-line instances (fused multiply-add terms, another order).
"""
import ctypes as C

import numpy as np
import pytest

import oracle
import prost_amd as prost
from prost_amd import synthetic

pytestmark = pytest.mark.gpu

DT = np.float32
F_COEFFS = [1.0, 1.0, 1.0, 0.0, 0.0, 0.3, 0.0]
TVAL, SVAL = 0.25, 0.5
# (nx, chunk length): one chunk only; exactly two; 3 and 5 chunks; a last chunk of 1, 2, 3 columns as the left half of an odd pair
# and as the right half of a full one; one-column chunks -- seams at column 1 and nx - 2 (nx = 7) resp. nx - 1 (nx = 6); two-column
# chunks; the launcher's own choice; one 18-column pair with a remainder
GEOMETRIES = [(7, 8), (8, 4), (12, 4), (20, 4), (9, 4), (10, 4), (11, 4), (13, 4), (14, 4), (15, 4), (7, 1), (6, 1), (5, 2), (4, 2), (40, 0), (43, 18)]


class RuleOpts(C.Structure):
    _fields_ = [("variant", C.c_int), ("arg_nu", C.c_double), ("arg_delta", C.c_double), ("arb_delta", C.c_double), ("arb_tau", C.c_double),
                ("tol_abs_primal", C.c_double), ("tol_abs_dual", C.c_double), ("tol_rel_primal", C.c_double), ("tol_rel_dual", C.c_double),
                ("sqrt_rows", C.c_double), ("sqrt_cols", C.c_double)]


def fused_desc(hip, nx, ny, g_fn, g_coeffs):
    d = hip.FusedDesc()
    d.is3d = 0; d.nx, d.ny, d.L = nx, ny, 1
    d.g_fn = hip.FN_ID[g_fn]; d.f_fn = hip.FN_ID["ind_leq0"]
    gp, gv, k1 = hip.coeff_args(g_coeffs, DT, nx * ny)
    fp, fv, k2 = hip.coeff_args(F_COEFFS, DT, nx * ny)
    for i in range(7):
        d.g_coeff_ptr[i] = gp[i]; d.g_coeff_val[i] = gv[i]
        d.f_coeff_ptr[i] = fp[i]; d.f_coeff_val[i] = fv[i]
    d.T_val, d.S_val = TVAL, SVAL
    return d, (k1, k2)


def oracle_iteration(x, y, nx, ny, g_fn, g_coeffs, tau, sigma, theta):
    """one PDHG iteration as the reference evaluates it (backend_pdhg.cu:313-370), every operation rounded to fp32"""
    tau, sigma, theta = DT(tau), DT(sigma), DT(theta)
    Td, Sd = np.full(nx * ny, TVAL, DT), np.full(2 * nx * ny, SVAL, DT)
    kty = oracle.grad2d(y, nx, ny, 1, adjoint=True)
    x1 = oracle.prox_elem(0, g_fn, (x - tau * Td * kty).astype(DT), Td, tau, nx * ny, 1, False, g_coeffs)
    kx, kxp = oracle.grad2d(x1, nx, ny, 1), oracle.grad2d(x, nx, ny, 1)
    y1 = oracle.prox_elem(1, "ind_leq0", (y + sigma * Sd * ((1 + theta) * kx - theta * kxp)).astype(DT), Sd, sigma, nx * ny, 2, False, F_COEFFS)
    return x1, y1


@pytest.mark.parametrize("ny", [248, 252, 8])
@pytest.mark.parametrize("g", ["square+b", "abs", "abs+b", "square"])
def test_paired_launch_equals_two_single_launches_and_the_oracle(hip, ny, g):
    g_fn = g.split("+")[0]
    rng = np.random.default_rng(5)
    L = hip.lib()
    L.prost_hip_pdhg_rule_record_bytes.restype = C.c_size_t
    taus, sigmas, thetas = (0.9, 0.7), (1.1, 1.4), (0.85, 0.8)
    tau = (C.c_double * 2)(*taus); sigma = (C.c_double * 2)(*sigmas); theta = (C.c_double * 2)(*thetas)
    ws = hip.DeviceArray(L.prost_hip_reduce_workspace_bytes() // 8, np.float64)
    record = hip.DeviceArray(L.prost_hip_pdhg_rule_record_bytes(), np.uint8)
    I1, I2, I2R = hip.fn("fused_iteration", DT), hip.fn("fused_iteration2", DT), hip.fn("fused_iteration2_rec", DT)
    for nx, cols in GEOMETRIES:
        n, m = nx * ny, 2 * nx * ny
        x = rng.uniform(0, 1, n).astype(DT); y = rng.uniform(-1, 1, m).astype(DT)
        f = rng.uniform(0, 1, n)
        g_coeffs = [1.0, f if g.endswith("+b") else 0.5, 10.0, 0.0, 0.0, 0.3, 0.0]
        desc, keep = fused_desc(hip, nx, ny, g_fn, g_coeffs)
        assert L.prost_hip_fused_iteration2_profitable(C.byref(desc), 0) == 1
        dx, dy = hip.DeviceArray.from_host(x), hip.DeviceArray.from_host(y)
        # steps: the two iterations of a scalar launch have their own step sizes, those of a record launch share the record's
        for steps in ((0, 1), (0, 0)):
            use_rec = steps == (0, 0)
            a, b = steps
            x1 = hip.DeviceArray.zeros(n, DT); y1 = hip.DeviceArray.zeros(m, DT); xr = hip.DeviceArray.zeros(n, DT); yr = hip.DeviceArray.zeros(m, DT)
            hip.check(I1(C.byref(desc), x1.ptr, y1.ptr, dx.ptr, dy.ptr, None, hip.dbl(taus[a]), hip.dbl(sigmas[a]), hip.dbl(thetas[a]), 1, 1, 0, 0, None, None, None))
            r4s = hip.DeviceArray.zeros(4, np.float64)
            hip.check(I1(C.byref(desc), xr.ptr, yr.ptr, x1.ptr, y1.ptr, dy.ptr, hip.dbl(taus[b]), hip.dbl(sigmas[b]), hip.dbl(thetas[b]), 1, 1, 1, 0, r4s.ptr, ws.ptr, None))
            x_ref, y_ref, res_ref = xr.to_host(), yr.to_host(), r4s.to_host()
            ox, oy = oracle_iteration(x, y, nx, ny, g_fn, g_coeffs, taus[a], sigmas[a], thetas[a])
            ox, oy = oracle_iteration(ox, oy, nx, ny, g_fn, g_coeffs, taus[b], sigmas[b], thetas[b])
            assert np.array_equal(x_ref, ox) and np.array_equal(y_ref, oy), (nx, cols, "single launches against the oracle")
            if use_rec:
                opts = RuleOpts(); opts.variant = 0; opts.sqrt_rows = float(np.sqrt(m)); opts.sqrt_cols = float(np.sqrt(n))
                hip.check(L.prost_hip_pdhg_rule_begin_f32(record.ptr, C.byref(opts), C.byref(desc), hip.dbl(taus[0]), hip.dbl(sigmas[0]), hip.dbl(thetas[0]),
                                                          hip.dbl(0.0), 0, 0, 0, None, None))
            for res in (False, True):
                x2 = hip.DeviceArray.from_host(np.full(n, 7.0, DT)); y2 = hip.DeviceArray.from_host(np.full(m, 7.0, DT)); r4 = hip.DeviceArray.zeros(4, np.float64)
                if use_rec:
                    hip.check(I2R(C.byref(desc), x2.ptr, y2.ptr, dx.ptr, dy.ptr, None, None, record.ptr, cols, r4.ptr if res else None, ws.ptr if res else None,
                                  0, C.c_ulonglong(0), None, None))
                else:
                    hip.check(I2(C.byref(desc), x2.ptr, y2.ptr, dx.ptr, dy.ptr, None, None, tau, sigma, theta, cols, r4.ptr if res else None, ws.ptr if res else None, None))
                gx, gy = x2.to_host(), y2.to_host()
                assert np.array_equal(gx, x_ref), (nx, cols, use_rec, res, np.flatnonzero(gx != x_ref)[:8])
                assert np.array_equal(gy, y_ref), (nx, cols, use_rec, res, np.flatnonzero(gy != y_ref)[:8])
                if res:
                    assert np.allclose(r4.to_host(), res_ref, rtol=2e-6, atol=1e-9 * np.abs(res_ref).max()), (nx, cols, r4.to_host(), res_ref)
                for d_ in (x2, y2, r4):
                    d_.free()
            if use_rec:
                # a raised stop word: the launch returns at once -- both waves of every pair, before their first barrier
                stop = C.c_void_p()
                hip.check(L.prost_hip_pdhg_record_view(record.ptr, 0, None, None, None, C.byref(stop)))
                one = np.ones(1, np.int32)
                hip.check(L.prost_hip_memcpy_h2d(stop, one.ctypes.data_as(C.c_void_p), C.c_size_t(4), None))
                x2 = hip.DeviceArray.from_host(np.full(n, 7.0, DT)); y2 = hip.DeviceArray.from_host(np.full(m, 7.0, DT))
                hip.check(I2R(C.byref(desc), x2.ptr, y2.ptr, dx.ptr, dy.ptr, None, None, record.ptr, cols, None, None, 0, C.c_ulonglong(0), None, None))
                assert np.all(x2.to_host() == 7.0) and np.all(y2.to_host() == 7.0), (nx, cols, "a stopped launch wrote")
                x2.free(); y2.free()
            for d_ in (x1, y1, xr, yr, r4s):
                d_.free()
        dx.free(); dy.free()
        del keep


@pytest.mark.parametrize("shape", [(96, 80), (300, 520)])
def test_solver_iterates_do_not_depend_on_the_pairing(shape):
    """k = 2, 4, 10 iterations through the solver (alg2, residual_iter = 10: plain paired launches, the last one with residual sums)
    equal the path that launches every iteration on its own, bit for bit."""
    nx, ny = shape
    prost.set_precision("single")
    for iters in (2, 4, 10):
        states = []
        for pair in (True, False):
            prob, u, q, f = synthetic.rof_problem(nx, ny, seed=3)
            b = prost.backend.pdhg(stepsize="alg2", residual_iter=10, alg2_gamma=0.5)
            b[1]["allow_pair_kernel"] = pair
            o = prost.options(max_iters=10 ** 6, num_cback_calls=0, verbose=False, tol_rel_primal=0, tol_rel_dual=0, tol_abs_primal=0, tol_abs_dual=0)
            s = prost.Solver(prob, b, o)
            s.iterate(iters)
            states.append(s.state())
            s.destroy()
        for v in "xy":
            assert np.array_equal(states[0][v], states[1][v]), (nx, ny, iters, v)
