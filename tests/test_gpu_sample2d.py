"""prost.block.sample2d on the GPU: the kernels through prost.eval_linop and through the C ABI, the block in the solver and in
examples/tv_scattered.py.

References: tests/sample2d_reference.py, never the code under test.
  * products: forward and adjoint equal the NumPy restatement (b) in T bit for bit, the same call twice gives the same bits; row and
    column sums within (t + 8) eps_T of (c), t the entries of that row or column, and exactly 0 where there are none;
  * composition: [K K] and [K ; K] accumulate in the forward and in the adjoint product (the restatement adds res + value), a 1 x 1
    diags block in front gives the block odd row and column offsets: bit for bit;
  * against block.sparse of matrix (a) on the GPU: |got - twin| <= 1.01 (t + 1) u (|K| |x|) componentwise, u the unit roundoff of T --
    the forward error bound of a t-term sum of rounded products in any order (derived, not measured);
  * an Inf in a pixel no sample touches, and in every pixel next to an integer-position sample, stays out of the result; a NaN in a
    pixel reaches exactly the rows the matrix says, a NaN in a sample exactly the columns;
  * the C entry points at element offsets 0, 1 and 4, plain and accumulating: bit for bit, with tables from the reference;
  * the scattered-data problem at 24 x 24 with 400 samples, alg1 with fixed steps, 200 iterations, tolerances 0: with the block on the
    GPU (i), with the sparse twin on the GPU (ii) and in the oracle (iii).  D = |u_ii - u_iii| / |u_iii|, measured in the test on the
    pair that runs no code of the block; (i) is held to max(10 D, 10 * 200 * t * u) of (iii), the rule of test_gpu_conv2d.py, t = 4 the
    entries of a row;
  * examples/tv_scattered.py at 32 x 32 from 2048 samples.  The oracle with the sparse twin on the CPU reaches an RMSE to the phantom
    of 0.02936 in fp64 (149 iterations, "Converged."); the phantom's own mean image, which needs no reconstruction at all, has 0.21591.
    The inequality asked of the GPU run with the block is RMSE <= 0.3 * 0.21591 = 0.06477, which the oracle meets 2.2 times over.

The kernels' units are 64 samples per wavefront (forward) and 64 rows of one column per wavefront (adjoint), four wavefronts per
workgroup: the case list holds M = 1, 63, 64, 65, 257 and images of exactly 64 rows and of 65.
"""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

import sample2d_reference as R
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
    """|got - want| <= tol want componentwise, and exactly 0 where want is"""
    return bool(np.all(np.abs(got - want) <= tol * want) and np.all(got[want == 0] == 0))


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a, b) and np.array_equal(np.signbit(a), np.signbit(b))


@pytest.mark.parametrize("prec,dtype", PRECISIONS)
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_products_bit_for_bit_and_sums(prec, dtype, case):
    prost.set_precision(prec)
    args = R.case_args(case)
    rng = np.random.default_rng(R.case_seed(case))
    bf = prost.block.sample2d(*args)
    nrows, ncols = bf(0, 0, 0, 0)[1]
    linop = [bf(0, 0, nrows, ncols)[0]]
    rs, cs = R.sums(*args, 1.0, dtype)
    trow, tcol = R.terms(*args, dtype)
    eps = np.finfo(dtype).eps
    for transpose in (False, True):
        x = rng.standard_normal(nrows if transpose else ncols)
        got, rowsum, colsum = run(linop, x, transpose)
        want = R.product(x, *args, transpose, dtype).astype(np.float64)
        assert same_bits(got, want), (transpose, float(np.abs(got - want).max()), int((got != want).sum()))
        assert same_bits(run(linop, x, transpose)[0], got)                      # no atomics: the same bits every time
        assert rowsum.shape == rs.shape and colsum.shape == cs.shape
        assert within(rowsum, rs, (trow + 8) * eps) and within(colsum, cs, (tcol + 8) * eps)


@pytest.mark.parametrize("prec,dtype", PRECISIONS)
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_composition_bit_for_bit(prec, dtype, case):
    """[K K]: the second block adds onto the first in the forward product; [K ; K]: in the adjoint; diag(d, K) with a 1 x 1 diags block
    d in front: K's rows and columns start at element 1"""
    prost.set_precision(prec)
    arg = R.case_args(case)
    rng = np.random.default_rng(R.case_seed(case, 1))
    bf = prost.block.sample2d(*arg)
    m, n = bf(0, 0, 0, 0)[1]
    xn2, xn, xm2, xm = rng.standard_normal(2 * n), rng.standard_normal(n), rng.standard_normal(2 * m), rng.standard_normal(m)
    side = [bf(0, 0, m, n)[0], bf(0, n, m, n)[0]]
    want = R.product(xn2[n:], *arg, False, dtype, res0=R.product(xn2[:n], *arg, False, dtype))
    assert np.array_equal(run(side, xn2, False)[0], want.astype(np.float64))
    assert np.array_equal(run(side, xm, True)[0], np.tile(R.product(xm, *arg, True, dtype), 2).astype(np.float64))
    stack = [bf(0, 0, m, n)[0], bf(m, 0, m, n)[0]]
    assert np.array_equal(run(stack, xn, False)[0], np.tile(R.product(xn, *arg, False, dtype), 2).astype(np.float64))
    want = R.product(xm2[m:], *arg, True, dtype, res0=R.product(xm2[:m], *arg, True, dtype))
    assert np.array_equal(run(stack, xm2, True)[0], want.astype(np.float64))
    shifted = [prost.block.diags(1, 1, [2.0], [0])(0, 0, 1, 1)[0], bf(1, 1, m, n)[0]]
    for transpose in (False, True):
        xs = rng.standard_normal((m if transpose else n) + 1)
        got = run(shifted, xs, transpose)[0]
        want = np.concatenate([(np.zeros(1, dtype) + dtype(2.0) * xs[:1].astype(dtype)), R.product(xs[1:], *arg, transpose, dtype)])
        assert np.array_equal(got, want.astype(np.float64)), transpose
        assert np.array_equal(run(shifted, xs, transpose)[0], got)


@pytest.mark.parametrize("prec,dtype", PRECISIONS)
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_against_the_sparse_twin_on_the_gpu(prec, dtype, case):
    prost.set_precision(prec)
    args = R.case_args(case)
    rng = np.random.default_rng(R.case_seed(case, 2))
    K = R.matrix(*args, dtype)
    m, n = K.shape
    twin = [prost.block.sparse(K)(0, 0, m, n)[0]]
    linop = [prost.block.sample2d(*args)(0, 0, m, n)[0]]
    for transpose in (False, True):
        x = rng.standard_normal(m if transpose else n).astype(dtype).astype(np.float64)
        got = run(linop, x, transpose)[0]
        want = run(twin, x, transpose)[0]
        bound = R.bound(*args, transpose, x, dtype)
        err = np.abs(got - want)
        live = bound > 0
        print("%s %s transpose=%d: |got - twin| / bound %.3f" % (prec, R.case_id(case), transpose, float((err[live] / bound[live]).max()) if live.any() else 0.0))
        assert np.all(err <= bound), float((err[live] / bound[live]).max())


@pytest.mark.parametrize("prec,dtype", PRECISIONS)
def test_inf_stays_out_and_nan_reaches_what_the_matrix_says(prec, dtype):
    prost.set_precision(prec)
    # an Inf in a pixel no sample touches: the one-cell case leaves all but four pixels untouched
    case = next(c for c in R.CASES if c[3] == "onecell")
    args = R.case_args(case)
    K = R.matrix(*args, dtype).tocsc()
    m, n = K.shape
    per_column = np.diff(K.indptr)
    unseen, seen = np.nonzero(per_column == 0)[0], np.nonzero(per_column > 0)[0]
    assert unseen.size == n - 4 and seen.size == 4
    linop = [prost.block.sample2d(*args)(0, 0, m, n)[0]]
    x = np.random.default_rng(4).standard_normal(n)
    clean = run(linop, x, False)[0]
    assert np.isfinite(clean).all()
    for bad in (np.inf, -np.inf, np.nan):
        xi = x.copy()
        xi[unseen] = bad
        assert np.array_equal(run(linop, xi, False)[0], clean), bad
    # a NaN in a pixel reaches exactly the rows of that column; a NaN in a sample exactly the columns of that row
    case = next(c for c in R.CASES if c[:2] == (9, 7))
    args = R.case_args(case)
    K = R.matrix(*args, dtype).tocsc()
    Kr = K.tocsr()
    m, n = K.shape
    linop = [prost.block.sample2d(*args)(0, 0, m, n)[0]]
    x, y = np.random.default_rng(5).standard_normal(n), np.random.default_rng(6).standard_normal(m)
    clean, clean_t = run(linop, x, False)[0], run(linop, y, True)[0]
    for j in (0, n // 2, n - 1):
        xn = x.copy()
        xn[j] = np.nan
        got = run(linop, xn, False)[0]
        hit = np.zeros(m, bool)
        hit[K.indices[K.indptr[j]:K.indptr[j + 1]]] = True
        assert np.array_equal(np.isnan(got), hit), j
        assert np.array_equal(got[~hit], clean[~hit])
    empty = np.nonzero(np.diff(Kr.indptr) == 0)[0]
    assert empty.size                                        # the random samples around the image hold some out of its reach
    for i in (0, m // 2, m - 1, int(empty[0])):
        yn = y.copy()
        yn[i] = np.nan
        got = run(linop, yn, True)[0]
        hit = np.zeros(n, bool)
        hit[Kr.indices[Kr.indptr[i]:Kr.indptr[i + 1]]] = True
        assert np.array_equal(np.isnan(got), hit), i
        assert np.array_equal(got[~hit], clean_t[~hit])
    # samples at integer positions among pixels of Inf: the neighbours' weights are exactly 0, so they are absent
    nx, ny = 6, 5
    xs, ys = np.array([1.0, 4.0, 0.0, 5.0]), np.array([2.0, 0.0, 4.0, 4.0])
    img = np.full(nx * ny, np.inf)
    at = (ys + xs * ny).astype(int)
    img[at] = [3.0, -2.0, 0.5, 7.0]
    linop = [prost.block.sample2d(nx, ny, 1, xs, ys)(0, 0, 4, nx * ny)[0]]
    assert np.array_equal(run(linop, img, False)[0], img[at])
    back = run(linop, np.array([1.0, 2.0, 3.0, 4.0]), True)[0]
    want = np.zeros(nx * ny)
    want[at] = [1.0, 2.0, 3.0, 4.0]
    assert np.array_equal(back, want)


def entry(dtype):
    fn = _hip.fn("sample2d", dtype)
    fn.argtypes = [C.c_void_p] * 7 + [C.c_int, C.c_void_p]
    fn.restype = C.c_int
    return fn


def call(dtype, x, res0, geometry, tables, nres, accumulate, offset):
    """one launch through the C ABI; res and rhs start `offset` elements into their allocations"""
    pad = np.zeros(offset, dtype)
    keep = [_hip.DeviceArray.from_host(np.concatenate([pad, x.astype(dtype)])), _hip.DeviceArray.from_host(np.concatenate([pad, res0.astype(dtype)]))]
    keep += [_hip.DeviceArray.from_host(np.ascontiguousarray(t)) for t in tables]
    rhs, res, px, py, order, cell_start = keep
    try:
        _hip.check(entry(dtype)(geometry.ctypes.data_as(C.c_void_p), px.ptr, py.ptr, order.ptr, cell_start.ptr, res.offset(offset), rhs.offset(offset), int(accumulate), None))
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
    """offset 0 / 4: 16-byte aligned; 1: aligned for one element only.  The tables are the reference's, made from the definition."""
    rng = np.random.default_rng(12)
    for case in (R.CASES[2], R.CASES[7], R.CASES[9]):
        nx, ny, L, xs, ys = args = R.case_args(case)
        with np.errstate(over="ignore"):
            tables = (xs.astype(dtype), ys.astype(dtype)) + R.buckets(nx, ny, xs, ys, dtype)
        m, n = L * len(xs), L * nx * ny
        for transpose in (False, True):
            nres, nrhs = (n, m) if transpose else (m, n)
            x, res0 = rng.standard_normal(nrhs).astype(dtype), rng.standard_normal(nres).astype(dtype)
            geometry = R.abi_records(nx, ny, L, len(xs), transpose)
            plain = R.product(x, *args, transpose, dtype)
            for offset in (0, 1, 4):
                assert np.array_equal(call(dtype, x, res0, geometry, tables, nres, False, offset), plain), (case, transpose, offset)
                assert np.array_equal(call(dtype, x, res0, geometry, tables, nres, True, offset), res0 + plain), (case, transpose, offset)


# ---- the solve ----
SOLVE_ITERS = 200
SOLVE_SIZE, SOLVE_SAMPLES = 24, 400
SOLVE_TERMS = 4                           # entries of a row


@functools.lru_cache(maxsize=None)
def solve_three_ways(precision):
    import tv_scattered as ex
    dtype = dict(PRECISIONS)[precision]
    backend = prost.backend.pdhg(stepsize="alg1", residual_iter=10)
    opts = dict(max_iters=SOLVE_ITERS, num_cback_calls=0, verbose=False, tol_rel_primal=0, tol_rel_dual=0, tol_abs_primal=0, tol_abs_dual=0)
    prost.set_precision(precision)
    out = {}
    prob, _, _, u, _, data = ex.describe(SOLVE_SIZE, SOLVE_SAMPLES, twin=True, dtype=dtype)
    r = prost.solve(prob, backend, prost.options(**opts))
    out["ii"] = (np.array(u.val, dtype=np.float64).ravel(), r)
    prob, _, _, u, _, _ = ex.describe(SOLVE_SIZE, SOLVE_SAMPLES, twin=True, dtype=dtype, data=data)
    r = oracle.solve(prob, backend, prost.options(**opts), dtype)
    out["iii"] = (np.array(u.val, dtype=np.float64).ravel(), r)
    prob, _, _, u, _, _ = ex.describe(SOLVE_SIZE, SOLVE_SAMPLES, data=data)
    r = prost.solve(prob, backend, prost.options(**opts))
    out["i"] = (np.array(u.val, dtype=np.float64).ravel(), r)
    return out


@pytest.mark.parametrize("precision,dtype", PRECISIONS)
def test_solve_with_the_block_against_the_sparse_twin(precision, dtype):
    out = solve_three_ways(precision)
    (u1, r1), (u2, r2), (u3, r3) = out["i"], out["ii"], out["iii"]
    assert r1["iters"] == SOLVE_ITERS and r2["iters"] == SOLVE_ITERS and r3["iters"] == SOLVE_ITERS
    assert r1["path"] == "pdhg:generic", r1["path"]
    assert np.isfinite(u1).all() and u1.shape == u3.shape == (SOLVE_SIZE * SOLVE_SIZE,)
    scale = float(np.abs(u3).max())
    D = float(np.abs(u2 - u3).max()) / scale
    mine = float(np.abs(u1 - u3).max()) / scale
    limit = max(10 * D, 10 * SOLVE_ITERS * SOLVE_TERMS * (np.finfo(dtype).eps / 2))
    print("solve %s: D = |u_ii - u_iii| / |u_iii| = %.3g, |u_i - u_iii| / |u_iii| = %.3g, |u_i - u_ii| / |u_iii| = %.3g, limit %.3g"
          % (precision, D, mine, float(np.abs(u1 - u2).max()) / scale, limit))
    assert mine <= limit, (mine, limit)


def test_the_example_reconstructs_the_phantom():
    import tv_scattered as ex
    prost.set_precision("double")
    size, samples = 32, 2048
    result, img, truth, data = ex.main(size, samples, max_iters=5000, verbose=False)
    mean_image = ex.rmse(np.full(truth.size, truth.mean()), truth)
    print("example: %s after %d iterations on %s, RMSE %.5f, mean image %.5f" % (result["result"], result["iters"], result["path"], ex.rmse(img, truth), mean_image))
    assert result["result"] in ("Converged.", "Reached maximum iterations.") and (result["result"] == "Converged." or result["iters"] == 5000)
    assert result["path"] == "pdhg:generic", result["path"]
    assert img.size == size * size and np.isfinite(img).all()
    assert data.shape == (samples,)
    assert abs(mean_image - 0.21591) < 1e-4                 # the comparator runs no code of the block
    assert ex.rmse(img, truth) <= 0.3 * mean_image
