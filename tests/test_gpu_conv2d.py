"""prost.block.conv2d on the GPU: the kernels through prost.eval_linop and through the C ABI, the block in the solver and in
examples/deblurring_conv2d.py.

References: tests/conv2d_reference.py, never the code under test.
  * products: forward and adjoint equal the NumPy restatement (b) in T bit for bit, the same call twice gives the same bits; row and
    column sums within (t + 8) eps_T of (c), t the non-zero tap count;
  * composition: [B B] and [B ; B] accumulate in the forward and in the adjoint product (the restatement adds res + value), a 1 x 1
    diags block in front gives the block odd row and column offsets: bit for bit;
  * against the oracle's block.sparse on matrix (a): |got - twin| <= 1.01 (t + 1) u (|K| |x|) componentwise, u the unit roundoff of T
    -- the forward error bound of a t-term sum of rounded products in any order (derived, not measured);
  * the C entry points at element offsets 0, 1 and 4, plain and accumulating: bit for bit;
  * the deblurring problem at 24 x 16 x 3, alg1 with fixed steps, 200 iterations: with the block on the GPU (i), with the sparse twin on
    the GPU (ii) and in the oracle (iii); the distance D between (ii) and (iii), which run no code of the block, was measured once on an
    MI355X (docs/rounds/r18.md) and came out as exactly 0 in both precisions, so (i) is held to 10 * 200 * t * u of (iii) instead
    (measured: 0 in fp32, 5.81e-16 in fp64);
  * the example with the 15 x 15 Gaussian window.

The tile is 64 x 16: the shape list holds an image of exactly one tile and one that is one past it in both axes.
"""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

import conv2d_reference as R
import oracle
import prost_amd as prost
from prost_amd import _hip

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))

pytestmark = pytest.mark.gpu
PRECISIONS = [("single", np.float32), ("double", np.float64)]


@pytest.fixture(autouse=True)
def _gpu(hip):
    prost.set_gpu(0)
    yield
    prost.set_precision("double")


def run(linop, rhs, transpose):
    got, rowsum, colsum, _ = prost.eval_linop(linop, rhs, transpose)
    return np.asarray(got, dtype=np.float64).ravel(), np.asarray(rowsum, dtype=np.float64).ravel(), np.asarray(colsum, dtype=np.float64).ravel()


def within(got, want, tol):
    return bool(np.all(np.abs(got - want) <= tol * want))


@pytest.mark.parametrize("prec,dtype", PRECISIONS)
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_products_bit_for_bit_and_sums(prec, dtype, case):
    prost.set_precision(prec)
    ny, nx, L, _, shapes = case
    k = R.case_window(case)
    rng = np.random.default_rng(R.case_seed(case))
    tol = (R.taps(k, dtype) + 8) * np.finfo(dtype).eps
    for shape in shapes:
        bf = prost.block.conv2d(nx, ny, L, k, shape)
        nrows, ncols = bf(0, 0, 0, 0)[1]
        linop = [bf(0, 0, nrows, ncols)[0]]
        rs, cs = R.sums(nx, ny, L, k, shape, 1.0, dtype)
        for transpose in (False, True):
            x = rng.standard_normal(nrows if transpose else ncols)
            got, rowsum, colsum = run(linop, x, transpose)
            want = R.product(x, nx, ny, L, k, shape, transpose, dtype).astype(np.float64)
            assert got.shape == want.shape and np.array_equal(got, want), (shape, transpose, float(np.abs(got - want).max()))
            assert np.array_equal(run(linop, x, transpose)[0], got)                 # no atomics: the same bits every time
            assert rowsum.shape == rs.shape and colsum.shape == cs.shape
            assert within(rowsum, rs, tol) and within(colsum, cs, tol), shape


@pytest.mark.parametrize("prec,dtype", PRECISIONS)
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_composition_bit_for_bit(prec, dtype, case):
    """[B B]: the second block adds onto the first in the forward product; [B ; B]: in the adjoint; diag(d, B) with a 1 x 1 diags block
    d in front: B's rows and columns start at element 1"""
    prost.set_precision(prec)
    ny, nx, L, _, shapes = case
    k = R.case_window(case)
    rng = np.random.default_rng(R.case_seed(case, 1))
    for shape in shapes:
        bf = prost.block.conv2d(nx, ny, L, k, shape)
        m, n = bf(0, 0, 0, 0)[1]
        arg = (nx, ny, L, k, shape)
        xn2, xn, xm2, xm = rng.standard_normal(2 * n), rng.standard_normal(n), rng.standard_normal(2 * m), rng.standard_normal(m)
        side = [bf(0, 0, m, n)[0], bf(0, n, m, n)[0]]
        want = R.product(xn2[n:], *arg, False, dtype, res0=R.product(xn2[:n], *arg, False, dtype))
        assert np.array_equal(run(side, xn2, False)[0], want.astype(np.float64)), shape
        assert np.array_equal(run(side, xm, True)[0], np.tile(R.product(xm, *arg, True, dtype), 2).astype(np.float64)), shape
        stack = [bf(0, 0, m, n)[0], bf(m, 0, m, n)[0]]
        assert np.array_equal(run(stack, xn, False)[0], np.tile(R.product(xn, *arg, False, dtype), 2).astype(np.float64)), shape
        want = R.product(xm2[m:], *arg, True, dtype, res0=R.product(xm2[:m], *arg, True, dtype))
        assert np.array_equal(run(stack, xm2, True)[0], want.astype(np.float64)), shape
        shifted = [prost.block.diags(1, 1, [2.0], [0])(0, 0, 1, 1)[0], bf(1, 1, m, n)[0]]
        for transpose in (False, True):
            xs = rng.standard_normal((m if transpose else n) + 1)
            got = run(shifted, xs, transpose)[0]
            want = np.concatenate([(np.zeros(1, dtype) + dtype(2.0) * xs[:1].astype(dtype)), R.product(xs[1:], *arg, transpose, dtype)])
            assert np.array_equal(got, want.astype(np.float64)), (shape, transpose)
            assert np.array_equal(run(shifted, xs, transpose)[0], got)


@pytest.mark.parametrize("prec,dtype", PRECISIONS)
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_against_the_sparse_twin_in_the_oracle(prec, dtype, case):
    prost.set_precision(prec)
    ny, nx, L, _, shapes = case
    k = R.case_window(case)
    rng = np.random.default_rng(R.case_seed(case, 2))
    for shape in shapes:
        K = R.matrix(nx, ny, L, k, shape, dtype)
        m, n = K.shape
        twin = [prost.block.sparse(K)(0, 0, m, n)[0]]
        linop = [prost.block.conv2d(nx, ny, L, R.window(k, dtype).astype(np.float64), shape)(0, 0, m, n)[0]]
        for transpose in (False, True):
            x = rng.standard_normal(m if transpose else n).astype(dtype).astype(np.float64)
            got = run(linop, x, transpose)[0]
            want = oracle.eval_linop(twin, x, transpose, dtype)[0]
            bound = R.bound(nx, ny, L, k, shape, transpose, x, dtype)
            err = np.abs(got - want)
            live = bound > 0
            print("%s %s %s transpose=%d: |got - twin| / bound %.3f" % (prec, R.case_id(case), shape, transpose, float((err[live] / bound[live]).max()) if live.any() else 0.0))
            assert np.all(err <= bound), float((err[live] / bound[live]).max())


def call(dtype, x, res0, records, nres, accumulate, offset):
    """one launch through the C ABI; res and rhs start `offset` elements into their allocations"""
    geometry, table, ntaps = records
    pad = np.zeros(offset, dtype)
    keep = [_hip.DeviceArray.from_host(np.concatenate([pad, x.astype(dtype)])), _hip.DeviceArray.from_host(np.concatenate([pad, res0.astype(dtype)])),
            _hip.DeviceArray.from_host(table)]
    rhs, res, taps = keep
    fn = _hip.fn("conv2d", dtype)
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    fn.restype = C.c_int
    try:
        _hip.check(fn(geometry.ctypes.data_as(C.c_void_p), taps.ptr, ntaps, res.offset(offset), rhs.offset(offset), int(accumulate), None))
        _hip.sync()
        out = res.to_host()
        assert out.size == offset + nres and np.array_equal(out[:offset], pad)
        assert np.array_equal(rhs.to_host()[offset:], x.astype(dtype))
        return out[offset:]
    finally:
        for d in keep:
            d.free()


@pytest.mark.parametrize("prec,dtype", PRECISIONS)
def test_c_abi_offset_pointers_plain_and_accumulating(prec, dtype):
    """offset 0 / 4: 16-byte aligned; 1: aligned for one element only"""
    rng = np.random.default_rng(12)
    for case in (R.CASES[0], R.CASES[5], R.CASES[7]):
        ny, nx, L, _, _ = case
        k = R.case_window(case)
        for shape in ("full", "same"):
            K = R.matrix(nx, ny, L, k, shape, dtype)
            for transpose in (False, True):
                nres, nrhs = (K.shape[1], K.shape[0]) if transpose else K.shape
                x, res0 = rng.standard_normal(nrhs).astype(dtype), rng.standard_normal(nres).astype(dtype)
                records = R.abi_records(nx, ny, L, k, shape, transpose, dtype)
                plain = R.product(x, nx, ny, L, k, shape, transpose, dtype)
                for offset in (0, 1, 4):
                    assert np.array_equal(call(dtype, x, res0, records, nres, False, offset), plain), (case, shape, transpose, offset)
                    assert np.array_equal(call(dtype, x, res0, records, nres, True, offset), res0 + plain), (case, shape, transpose, offset)
    # refusals without a launch
    fn = _hip.fn("conv2d", dtype)
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    fn.restype = C.c_int
    good = np.array([4, 4, 4, 4, 1, 1, 3, 3, 1], np.int32)
    assert fn(None, None, 1, None, None, 0, None) != 0
    assert fn(good.ctypes.data_as(C.c_void_p), None, 1, None, None, 0, None) != 0                 # null pointers
    for field, value in ((6, 32), (7, 0), (4, 3), (5, -1), (0, 0), (8, 0)):                        # window, offsets, sizes
        bad = good.copy()
        bad[field] = value
        assert fn(bad.ctypes.data_as(C.c_void_p), C.c_void_p(16), 1, C.c_void_p(16), C.c_void_p(16), 0, None) != 0, (field, value)
    assert fn(good.ctypes.data_as(C.c_void_p), C.c_void_p(16), 10, C.c_void_p(16), C.c_void_p(16), 0, None) != 0      # more taps than the window has
    assert fn(good.ctypes.data_as(C.c_void_p), C.c_void_p(16), 0, C.c_void_p(16), C.c_void_p(16), 0, None) != 0


# ---- the solve ----
# D = |u_ii - u_iii|_inf / |u_iii|_inf after SOLVE_ITERS iterations: the sparse twin on the GPU against the sparse twin in the oracle,
# measured once on an MI355X (docs/rounds/r18.md).  Neither runs code of the block.  The block on the GPU (i) differs from (ii) by
# roundings of the products and of the preconditioner sums only; their amplification over 200 iterations is taken to be at most one decimal.
SOLVE_ITERS = 200
TWIN_DISTANCE = {
    "single": 0.0,
    "double": 0.0,
}
SOLVE_NX, SOLVE_NY, SOLVE_NC = 24, 16, 3


@functools.lru_cache(maxsize=None)
def solve_three_ways(precision):
    import deblurring as twin_ex
    import deblurring_conv2d as ex
    dtype = dict(PRECISIONS)[precision]
    backend = prost.backend.pdhg(stepsize="alg1", residual_iter=10)
    opts = dict(max_iters=SOLVE_ITERS, num_cback_calls=0, verbose=False, tol_rel_primal=0, tol_rel_dual=0, tol_abs_primal=0, tol_abs_dual=0)
    prost.set_precision(precision)
    out = {}
    prob, _, _, u, _, f_blurred, _ = twin_ex.describe(SOLVE_NX, SOLVE_NY, SOLVE_NC)
    r = prost.solve(prob, backend, prost.options(**opts))
    out["ii"] = (np.array(u.val, dtype=np.float64).ravel(), r)
    prob, _, _, u, _, _, _ = twin_ex.describe(SOLVE_NX, SOLVE_NY, SOLVE_NC)
    r = oracle.solve(prob, backend, prost.options(**opts), dtype)
    out["iii"] = (np.array(u.val, dtype=np.float64).ravel(), r)
    prob, _, _, u, _, _, _ = ex.describe(SOLVE_NX, SOLVE_NY, SOLVE_NC, "motion", f_blurred=f_blurred)
    r = prost.solve(prob, backend, prost.options(**opts))
    out["i"] = (np.array(u.val, dtype=np.float64).ravel(), r)
    return out


@pytest.mark.parametrize("precision,dtype", PRECISIONS)
def test_solve_with_the_block_against_the_sparse_twin(precision, dtype):
    out = solve_three_ways(precision)
    (u1, r1), (u2, r2), (u3, r3) = out["i"], out["ii"], out["iii"]
    assert r1["iters"] == SOLVE_ITERS and r2["iters"] == SOLVE_ITERS and r3["iters"] == SOLVE_ITERS
    assert r1["path"] == "pdhg:generic", r1["path"]
    assert np.isfinite(u1).all() and u1.shape == u3.shape == (SOLVE_NX * SOLVE_NY * SOLVE_NC,)
    scale = float(np.abs(u3).max())
    D = float(np.abs(u2 - u3).max()) / scale
    mine = float(np.abs(u1 - u3).max()) / scale
    t = R.taps(R.motion_window(), dtype)
    print("solve %s: D = |u_ii - u_iii| / |u_iii| = %.3g, |u_i - u_iii| / |u_iii| = %.3g, |u_i - u_ii| / |u_iii| = %.3g, %d taps"
          % (precision, D, mine, float(np.abs(u1 - u2).max()) / scale, t))
    # D came out as exactly 0 (the exact-class sparse kernels add in the oracle's order), so the bound is 10 * 200 t u instead: ten times
    # one forward error t u of a product per iteration
    limit = 10 * TWIN_DISTANCE[precision] if TWIN_DISTANCE[precision] > 0 else 10 * SOLVE_ITERS * t * (np.finfo(dtype).eps / 2)
    assert mine <= limit, (mine, limit)


def test_the_example_with_the_gaussian_window():
    import deblurring_conv2d as ex
    prost.set_precision("double")
    nx, ny, nc = 24, 16, 3
    result, img, f, blurred = ex.main(nx, ny, nc, "gauss", max_iters=4000, verbose=False)
    print("example: %s after %d iterations on %s" % (result["result"], result["iters"], result["path"]))
    assert result["result"] in ("Converged.", "Reached maximum iterations.") and (result["result"] == "Converged." or result["iters"] == 4000)
    assert result["path"] == "pdhg:generic", result["path"]
    assert img.size == nx * ny * nc and np.isfinite(img).all()
    k = ex.window("gauss")
    assert k.shape == (15, 15) and np.count_nonzero(k) == 225
    K = R.matrix(nx, ny, nc, k, "full")
    assert blurred.shape == (K.shape[0],)
    assert np.all(np.abs(blurred - K @ f) <= R.bound(nx, ny, nc, k, "full", False, f, np.float64))
