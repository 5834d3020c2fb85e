"""prost.block.conv2d_strided on the GPU: the kernels through prost.eval_linop and through the C ABI, the block in the solver and in
examples/superresolution.py.

References: tests/conv2d_strided_reference.py, never the code under test.
  1. products: forward and adjoint equal the NumPy restatement (b) in T bit for bit, the same call twice gives the same bits; row and
     column sums within (t + 8) eps_T of (c), t the non-zero tap count, an empty row or column exactly 0;
  2. stride (1, 1), phase (0, 0) equals prost.block.conv2d ON THE GPU bit for bit, both directions, all three shapes: the new kernels are
     pinned to the existing one;
  3. composition: [K K] and [K ; K] accumulate in the forward and in the adjoint product (the restatement adds res + value), a 1 x 1
     diags block in front gives the block odd element offsets (the element-store path of the adjoint): bit for bit;
  4. against the oracle's block.sparse on matrix (a): |got - twin| <= 1.01 (t + 1) u (|K| |x|) at every component (derived, (d));
  5. absent terms: Inf in a pixel no output samples stays out of every output, NaN in a sampled pixel reaches exactly the outputs the
     matrix says, the adjoint at stride 4 with a 1 x 1 window writes zeros into the fifteen untouched residues of every 4 x 4 cell and
     its accumulating form leaves them as they were;
  6. the C entry points at element offsets 0, 1 and 4, plain and accumulating, both directions: bit for bit; refusals without a launch;
  7. the super-resolution problem at 24 x 16 x 3, factor 2, 5 x 5 Gaussian, alg1 with fixed steps, 200 iterations, all tolerances 0:
     (i) the block on the GPU, (ii) the sparse twin on the GPU, (iii) the twin in the oracle.  With D = |(ii) - (iii)| / |(iii)| (max
     norms; neither runs code of the block) the block is held to |(i) - (iii)| / |(iii)| <= max(10 D, 10 * 200 * t * u): the rule of
     test_gpu_conv2d.py, the margin measured on the twin pair, never on the block.  Measured on an MI355X: docs/rounds/r21.md;
  8. the example at 24 x 16 x 3, factor 2, lmb = 2000: for this image and lmb the ORACLE WITH THE TWIN on the CPU already reaches an RMSE
     of 0.101 to the ground truth against 0.184 of nearest-neighbour upsampling (875 iterations to "Converged."), so the GPU run with
     the block is asked for the same inequality.

Shapes: conv2d_strided_reference.cases(dtype) -- every stride with every window, the three small images in turn, both phases, all
shapes; for every tile-table entry these select an image whose output is exactly one tile and one a row and a column past it; 31 x 31
once per stride (4, 4) and (1, 1); a ragged last stride; "valid" with the window equal to the image.
"""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

import conv2d_strided_reference as R
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


def builder(case):
    ny, nx, L, name, stride, phase, shape = case
    k = R.make_window(name)
    return prost.block.conv2d_strided(nx, ny, L, k, stride, shape, phase), (nx, ny, L, k, shape, stride, phase)


@pytest.mark.parametrize("prec,dtype", PRECISIONS)
def test_products_bit_for_bit_and_sums(prec, dtype):
    prost.set_precision(prec)
    for case in R.cases(dtype):
        bf, arg = builder(case)
        nrows, ncols = bf(0, 0, 0, 0)[1]
        linop = [bf(0, 0, nrows, ncols)[0]]
        rng = np.random.default_rng(R.case_seed(case))
        tol = (R.taps(arg[3], dtype) + 8) * np.finfo(dtype).eps
        rs, cs = R.sums(*arg, 1.0, dtype)
        for transpose in (False, True):
            x = rng.standard_normal(nrows if transpose else ncols)
            got, rowsum, colsum = run(linop, x, transpose)
            want = R.product(x, *arg, transpose, dtype).astype(np.float64)
            assert got.shape == want.shape and np.array_equal(got, want), (R.case_id(case), transpose, float(np.abs(got - want).max()))
            assert np.array_equal(run(linop, x, transpose)[0], got), R.case_id(case)          # no atomics: the same bits every time
            assert rowsum.shape == rs.shape and colsum.shape == cs.shape
            assert within(rowsum, rs, tol) and within(colsum, cs, tol), R.case_id(case)       # tol * 0: an empty one is exactly 0


@pytest.mark.parametrize("prec,dtype", PRECISIONS)
def test_stride_one_is_conv2d_on_the_gpu_bit_for_bit(prec, dtype):
    prost.set_precision(prec)
    for ny, nx, L, name in ((1, 1, 1, "1x1"), (17, 13, 3, "5x4z"), (17, 13, 3, "2x5"), (65, 17, 1, "3x3"), (64, 16, 2, "9x9g"), (9, 6, 1, "31x31")):
        k = R.make_window(name)
        rng = np.random.default_rng(5 + ny + 31 * nx)
        for shape in R.valid_shapes(ny, nx, *k.shape):
            new, old = prost.block.conv2d_strided(nx, ny, L, k, 1, shape), prost.block.conv2d(nx, ny, L, k, shape)
            m, n = new(0, 0, 0, 0)[1]
            assert [m, n] == old(0, 0, 0, 0)[1]
            for transpose in (False, True):
                x = rng.standard_normal(m if transpose else n)
                assert np.array_equal(run([new(0, 0, m, n)[0]], x, transpose)[0], run([old(0, 0, m, n)[0]], x, transpose)[0]), (ny, nx, name, shape, transpose)
                # and accumulating: [K K] forward, [K ; K] adjoint
                pair_new = [new(0, 0, m, n)[0], new(m, 0, m, n)[0]] if transpose else [new(0, 0, m, n)[0], new(0, n, m, n)[0]]
                pair_old = [old(0, 0, m, n)[0], old(m, 0, m, n)[0]] if transpose else [old(0, 0, m, n)[0], old(0, n, m, n)[0]]
                x2 = rng.standard_normal(2 * (m if transpose else n))
                assert np.array_equal(run(pair_new, x2, transpose)[0], run(pair_old, x2, transpose)[0]), (ny, nx, name, shape, transpose)


@pytest.mark.parametrize("prec,dtype", PRECISIONS)
def test_composition_bit_for_bit(prec, dtype):
    """[K K]: the second block adds onto the first in the forward product; [K ; K]: in the adjoint; diag(d, K) with a 1 x 1 diags block
    d in front: K's rows and columns start at element 1"""
    prost.set_precision(prec)
    for case in R.cases(dtype):
        bf, arg = builder(case)
        m, n = bf(0, 0, 0, 0)[1]
        rng = np.random.default_rng(R.case_seed(case, 1))
        xn2, xn, xm2, xm = rng.standard_normal(2 * n), rng.standard_normal(n), rng.standard_normal(2 * m), rng.standard_normal(m)
        side = [bf(0, 0, m, n)[0], bf(0, n, m, n)[0]]
        want = R.product(xn2[n:], *arg, False, dtype, res0=R.product(xn2[:n], *arg, False, dtype))
        assert np.array_equal(run(side, xn2, False)[0], want.astype(np.float64)), R.case_id(case)
        assert np.array_equal(run(side, xm, True)[0], np.tile(R.product(xm, *arg, True, dtype), 2).astype(np.float64)), R.case_id(case)
        stack = [bf(0, 0, m, n)[0], bf(m, 0, m, n)[0]]
        assert np.array_equal(run(stack, xn, False)[0], np.tile(R.product(xn, *arg, False, dtype), 2).astype(np.float64)), R.case_id(case)
        want = R.product(xm2[m:], *arg, True, dtype, res0=R.product(xm2[:m], *arg, True, dtype))
        assert np.array_equal(run(stack, xm2, True)[0], want.astype(np.float64)), R.case_id(case)
        shifted = [prost.block.diags(1, 1, [2.0], [0])(0, 0, 1, 1)[0], bf(1, 1, m, n)[0]]
        for transpose in (False, True):
            xs = rng.standard_normal((m if transpose else n) + 1)
            got = run(shifted, xs, transpose)[0]
            want = np.concatenate([(np.zeros(1, dtype) + dtype(2.0) * xs[:1].astype(dtype)), R.product(xs[1:], *arg, transpose, dtype)])
            assert np.array_equal(got, want.astype(np.float64)), (R.case_id(case), transpose)
            assert np.array_equal(run(shifted, xs, transpose)[0], got)


@pytest.mark.parametrize("prec,dtype", PRECISIONS)
def test_against_the_sparse_twin_in_the_oracle(prec, dtype):
    prost.set_precision(prec)
    worst = 0.0
    for case in R.cases(dtype):
        ny, nx, L, name, stride, phase, shape = case
        k = R.make_window(name)
        arg = (nx, ny, L, k, shape, stride, phase)
        rng = np.random.default_rng(R.case_seed(case, 2))
        K = R.matrix(*arg, dtype)
        m, n = K.shape
        twin = [prost.block.sparse(K)(0, 0, m, n)[0]]
        linop = [prost.block.conv2d_strided(nx, ny, L, R.window(k, dtype).astype(np.float64), stride, shape, phase)(0, 0, m, n)[0]]
        for transpose in (False, True):
            x = rng.standard_normal(m if transpose else n).astype(dtype).astype(np.float64)
            got = run(linop, x, transpose)[0]
            want = np.asarray(oracle.eval_linop(twin, x, transpose, dtype)[0], dtype=np.float64).ravel()
            bound = R.bound(*arg, transpose, x, dtype)
            err = np.abs(got - want)
            live = bound > 0
            ratio = float((err[live] / bound[live]).max()) if live.any() else 0.0
            worst = max(worst, ratio)
            assert got.shape == want.shape == bound.shape and np.all(err <= bound), (R.case_id(case), transpose, ratio)      # every component, none excluded
    print("%s: largest |got - twin| / bound over %d cases: %.3f" % (prec, len(R.cases(dtype)), worst))


def call(dtype, x, res0, records, nres, accumulate, offset):
    """one launch through the C ABI; res and rhs start `offset` elements into their allocations"""
    geometry, table, ntaps = records
    pad = np.zeros(offset, dtype)
    keep = [_hip.DeviceArray.from_host(np.concatenate([pad, x.astype(dtype)])), _hip.DeviceArray.from_host(np.concatenate([pad, res0.astype(dtype)])),
            _hip.DeviceArray.from_host(table)]
    rhs, res, taps = keep
    fn = _hip.fn("conv2d_strided", dtype)
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    fn.restype = C.c_int
    try:
        _hip.check(fn(geometry.ctypes.data_as(C.c_void_p), taps.ptr, ntaps, res.offset(offset), rhs.offset(offset), int(accumulate), None))
        _hip.sync()
        out = res.to_host()
        assert out.size == offset + nres and np.array_equal(out[:offset], pad)
        assert np.array_equal(rhs.to_host()[offset:], x.astype(dtype), equal_nan=True)
        return out[offset:]
    finally:
        for d in keep:
            d.free()


@pytest.mark.parametrize("prec,dtype", PRECISIONS)
def test_absent_terms(prec, dtype):
    prost.set_precision(prec)
    # pure decimation at stride 2: Inf in a pixel no output samples stays out of every output
    ny, nx = 7, 5
    arg = (nx, ny, 1, np.array([[1.5]]), "same", (2, 2), (0, 0))
    K = R.matrix(*arg, dtype)
    linop = [prost.block.conv2d_strided(nx, ny, 1, arg[3], 2, "same")(0, 0, *K.shape)[0]]
    x = np.random.default_rng(3).standard_normal(nx * ny)
    unsampled = np.flatnonzero(np.asarray(abs(K).sum(axis=0)).ravel() == 0)
    assert unsampled.size == nx * ny - K.shape[0] and 1 in unsampled
    x[unsampled] = np.inf
    got = run(linop, x, False)[0]
    assert np.isfinite(got).all() and np.array_equal(got, R.product(np.where(np.isinf(x), 0.0, x), *arg, False, dtype).astype(np.float64))
    # NaN in a sampled pixel reaches exactly the outputs the matrix says (3 x 3 window, stride 2, three planes)
    ny, nx, L = 17, 13, 3
    arg = (nx, ny, L, R.make_window("3x3"), "same", (2, 2), (1, 0))
    K = R.matrix(*arg, dtype)
    linop = [prost.block.conv2d_strided(nx, ny, L, arg[3], 2, "same", (1, 0))(0, 0, *K.shape)[0]]
    for pixel in (0, 5 + 6 * ny, ny * nx + 16 + 12 * ny):
        x = np.random.default_rng(4).standard_normal(K.shape[1])
        x[pixel] = np.nan
        got = run(linop, x, False)[0]
        assert np.array_equal(np.isnan(got), np.asarray((K[:, [pixel]] != 0).todense()).ravel()), pixel
    # the adjoint at stride 4 with a 1 x 1 window: fifteen residues of every 4 x 4 cell hold no tap
    ny, nx, L = 18, 9, 2
    arg = (nx, ny, L, np.array([[-0.75]]), "same", (4, 4), (1, 2))
    K = R.matrix(*arg, dtype)
    m, n = K.shape
    touched = np.asarray(abs(K).sum(axis=0)).ravel() > 0
    assert touched.sum() == m and n == 2 * 18 * 9 and m == 2 * 5 * 2
    rng = np.random.default_rng(6)
    y, res0 = rng.standard_normal(m).astype(dtype), rng.standard_normal(n).astype(dtype)
    records = R.abi_records(*arg, True, dtype)
    for offset in (0, 1):
        plain = call(dtype, y, res0, records, n, False, offset)
        assert np.array_equal(plain[~touched], np.zeros(n - m, dtype)) and np.array_equal(plain, R.product(y, *arg, True, dtype))
        acc = call(dtype, y, res0, records, n, True, offset)
        assert np.array_equal(acc[~touched], res0[~touched]) and np.array_equal(acc, res0 + plain)
    got = run([prost.block.conv2d_strided(nx, ny, L, arg[3], 4, "same", (1, 2))(0, 0, m, n)[0]], y, True)[0]
    assert np.array_equal(got[~touched], np.zeros(n - m)) and np.array_equal(got, plain.astype(np.float64))


@pytest.mark.parametrize("prec,dtype", PRECISIONS)
def test_c_abi_offset_pointers_plain_and_accumulating(prec, dtype):
    """offset 0 / 4: 16-byte aligned; 1: aligned for one element only (the adjoint's vector stores give way to element stores)"""
    rng = np.random.default_rng(12)
    for case in ((17, 13, 3, "5x4z", (2, 2), (1, 1), "same"), (17, 13, 3, "9x9g", (4, 4), (0, 3), "full"), (65, 17, 1, "3x3", (3, 2), (2, 0), "same")):
        ny, nx, L, name, stride, phase, shape = case
        arg = (nx, ny, L, R.make_window(name), shape, stride, phase)
        K = R.matrix(*arg, dtype)
        for transpose in (False, True):
            nres, nrhs = (K.shape[1], K.shape[0]) if transpose else K.shape
            x, res0 = rng.standard_normal(nrhs).astype(dtype), rng.standard_normal(nres).astype(dtype)
            records = R.abi_records(*arg, transpose, dtype)
            plain = R.product(x, *arg, transpose, dtype)
            for offset in (0, 1, 4):
                assert np.array_equal(call(dtype, x, res0, records, nres, False, offset), plain), (case, transpose, offset)
                assert np.array_equal(call(dtype, x, res0, records, nres, True, offset), res0 + plain), (case, transpose, offset)
    # refusals without a launch
    fn = _hip.fn("conv2d_strided", dtype)
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    fn.restype = C.c_int
    good, _, ntaps = R.abi_records(8, 8, 1, np.ones((3, 3)), "same", (2, 2), (0, 0), True, dtype)
    assert fn(None, None, 1, None, None, 0, None) != 0
    assert fn(good.ctypes.data_as(C.c_void_p), None, ntaps, None, None, 0, None) != 0                # null pointers
    for field, value in ((6, 32), (7, 0), (8, 5), (9, 0), (10, 2), (4, 3), (5, -1), (0, 0), (12, 0), (30, 8)):      # window, stride, phase, offsets, sizes, class table
        bad = good.copy()
        bad[field] = value
        assert fn(bad.ctypes.data_as(C.c_void_p), C.c_void_p(16), ntaps, C.c_void_p(16), C.c_void_p(16), 0, None) != 0, (field, value)
    assert fn(good.ctypes.data_as(C.c_void_p), C.c_void_p(16), 10, C.c_void_p(16), C.c_void_p(16), 0, None) != 0      # more taps than the window has
    assert fn(good.ctypes.data_as(C.c_void_p), C.c_void_p(16), 0, C.c_void_p(16), C.c_void_p(16), 0, None) != 0
    _hip.sync()


# ---- the solve ----
SOLVE_ITERS = 200
SOLVE_NX, SOLVE_NY, SOLVE_NC, SOLVE_FACTOR = 24, 16, 3, 2


@functools.lru_cache(maxsize=None)
def solve_three_ways(precision):
    import superresolution as ex
    dtype = dict(PRECISIONS)[precision]
    backend = prost.backend.pdhg(stepsize="alg1", residual_iter=10)
    opts = dict(max_iters=SOLVE_ITERS, num_cback_calls=0, verbose=False, tol_rel_primal=0, tol_rel_dual=0, tol_abs_primal=0, tol_abs_dual=0)
    prost.set_precision(precision)
    out = {}
    prob, _, _, u, _, f_low = ex.describe(SOLVE_NX, SOLVE_NY, SOLVE_NC, SOLVE_FACTOR, twin=True)
    r = prost.solve(prob, backend, prost.options(**opts))
    out["ii"] = (np.array(u.val, dtype=np.float64).ravel(), r)
    prob, _, _, u, _, _ = ex.describe(SOLVE_NX, SOLVE_NY, SOLVE_NC, SOLVE_FACTOR, twin=True, f_low=f_low)
    r = oracle.solve(prob, backend, prost.options(**opts), dtype)
    out["iii"] = (np.array(u.val, dtype=np.float64).ravel(), r)
    prob, _, _, u, _, _ = ex.describe(SOLVE_NX, SOLVE_NY, SOLVE_NC, SOLVE_FACTOR, twin=False, f_low=f_low)
    r = prost.solve(prob, backend, prost.options(**opts))
    out["i"] = (np.array(u.val, dtype=np.float64).ravel(), r)
    return out


@pytest.mark.parametrize("precision,dtype", PRECISIONS)
def test_solve_with_the_block_against_the_sparse_twin(precision, dtype):
    import superresolution as ex
    out = solve_three_ways(precision)
    (u1, r1), (u2, r2), (u3, r3) = out["i"], out["ii"], out["iii"]
    assert r1["iters"] == SOLVE_ITERS and r2["iters"] == SOLVE_ITERS and r3["iters"] == SOLVE_ITERS
    assert r1["path"] == "pdhg:generic", r1["path"]
    assert np.isfinite(u1).all() and u1.shape == u3.shape == (SOLVE_NX * SOLVE_NY * SOLVE_NC,)
    scale = float(np.abs(u3).max())
    D = float(np.abs(u2 - u3).max()) / scale
    mine = float(np.abs(u1 - u3).max()) / scale
    k = ex.gauss_window(SOLVE_FACTOR)
    t = R.taps(k, dtype)
    assert k.shape == (5, 5) and t == 25
    print("solve %s: D = |u_ii - u_iii| / |u_iii| = %.3g, |u_i - u_iii| / |u_iii| = %.3g, |u_i - u_ii| / |u_iii| = %.3g, %d taps"
          % (precision, D, mine, float(np.abs(u1 - u2).max()) / scale, t))
    limit = max(10 * D, 10 * SOLVE_ITERS * t * (np.finfo(dtype).eps / 2))
    assert mine <= limit, (mine, limit)


def test_the_example_beats_nearest_neighbour_upsampling():
    import superresolution as ex
    prost.set_precision("double")
    nx, ny, nc, factor = 24, 16, 3, 2
    result, img, truth, f_low = ex.main(nx, ny, nc, factor, max_iters=4000, verbose=False, lmb=2000.0)
    mine, baseline = ex.rmse(img, truth), ex.rmse(ex.nearest(f_low, nx, ny, nc, factor), truth)
    print("example: %s after %d iterations on %s; RMSE %.4f, nearest-neighbour upsampling %.4f" % (result["result"], result["iters"], result["path"], mine, baseline))
    assert result["result"] in ("Converged.", "Reached maximum iterations.") and (result["result"] == "Converged." or result["iters"] == 4000)
    assert result["path"] == "pdhg:generic", result["path"]
    assert img.size == nx * ny * nc and np.isfinite(img).all()
    K = R.matrix(nx, ny, nc, ex.gauss_window(factor), "same", factor, 0)
    assert f_low.shape == (K.shape[0],) and (ex.explicit_matrix(nx, ny, nc, ex.gauss_window(factor), factor) != K).nnz == 0
    assert mine < baseline, (mine, baseline)
