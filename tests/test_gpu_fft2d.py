"""prost.block.fft2d on the GPU: the kernels through prost.eval_linop and through the C ABI, the block in the solver and in
examples/tv_mri.py.

References: tests/fft2d_reference.py, never the code under test.  u is the unit roundoff of T, B the bound (e) of the reference,
B = t eta / (1 - t eta) + 2 u per plane pair in the 2-norm (derived in include/prost/linop/fft2d.hpp).
  * products: forward and transposed equal the NumPy restatement (b) in T bit for bit (-0 and +0 compare equal), the same call twice
    gives the same bits; row and column sums through prost.eval_linop within (g + 8) eps_T of the closed form (d);
  * against numpy.fft in float64: |got - reference|_2 <= B |x|_2 per plane pair in fp32, 2 B in fp64 (the reference is then itself a
    float64 FFT);
  * composition: [K K] and [K ; K] accumulate in the forward and in the transposed product (the restatement adds res + value), a 1 x 1
    diags block in front gives the block odd row and column offsets: bit for bit;
  * 1 x 2 with L = 70000, more images than the grid's y axis holds: bit for bit;
  * the C entry points at element offsets 0, 1 and 4, plain and accumulating, with the reference's table: bit for bit; rhs is left alone;
  * a NaN or an Inf in image 0 of three leaves images 1 and 2 bit-identical to the clean run;
  * against prost.block.dense of matrix (c) on the GPU at 8 x 4 and 16 x 16: |got - twin|_2 <= B |x|_2 per plane pair in fp32, 2 B in
    fp64 (the twin's matrix and dot products are then themselves float64 arithmetic, as the FFT comparator's); the ratio is printed;
  * the k-space problem at 16 x 16, half of k-space masked, alg1 with fixed steps, 200 iterations, tolerances 0, the default diagonal
    preconditioners (so the block's sums are in use): with the block on the GPU (i), with the dense twin on the GPU (ii) and with the
    same matrix in the oracle (iii; the oracle has no dense block and takes it through its sparse one: twin_as_sparse below).  D = |u_ii - u_iii| / |u_iii|,
    measured on the pair that runs no code of the block; (i) is held to max(10 D, 10 * 200 * c * u) of (iii), the rule of
    test_gpu_sample2d.py, c = B / u;
  * examples/tv_mri.py at 32 x 32 in fp64, default parameters (half of the k-space lines, lmb = 0.005).  The oracle with the twin on the
    CPU reaches an RMSE to the phantom of 0.02834 (424 iterations, "Converged."); the zero-filled inverse transform of the data, which
    needs no reconstruction at all, has 0.10352.  The inequality asked of the GPU run with the block is RMSE <= 0.6 * 0.10352 = 0.06211,
    which the oracle meets 2.19 times over.
"""
import contextlib
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

import fft2d_reference as R
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


def block(case):
    bf = prost.block.fft2d(*case)
    n = bf(0, 0, 0, 0)[1][0]
    return bf, n


@pytest.mark.parametrize("prec,dtype", PRECISIONS)
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_products_bit_for_bit_repeatable_within_the_bound_and_sums(prec, dtype, case):
    prost.set_precision(prec)
    nx, ny, L = case
    rng = np.random.default_rng(R.case_seed(case))
    bf, n = block(case)
    linop = [bf(0, 0, n, n)[0]]
    want_sums, g = R.sums(nx, ny, L, 1.0)
    eps = np.finfo(dtype).eps
    B = R.bound(nx, ny, dtype) * (2 if dtype == np.float64 else 1)
    for transpose in (False, True):
        x = rng.standard_normal(n).astype(dtype).astype(np.float64)
        got, rowsum, colsum = run(linop, x, transpose)
        want = R.product(x, nx, ny, L, transpose, dtype).astype(np.float64)
        assert got.shape == want.shape and np.array_equal(got, want), (transpose, float(np.abs(got - want).max()), int((got != want).sum()))
        assert np.array_equal(run(linop, x, transpose)[0], got)                 # no atomics: the same bits every time
        err = R.pair_norms(got - R.fft_reference(x, nx, ny, L, transpose), nx, ny, L) / R.pair_norms(x, nx, ny, L)
        print("%s %s transpose=%d: |got - numpy.fft| / (B |x|) = %.3f" % (prec, R.case_id(case), transpose, float(err.max()) / B))
        assert np.all(err <= B), float(err.max()) / B
        for s in (rowsum, colsum):
            assert s.shape == want_sums.shape and np.all(np.abs(s - want_sums) <= (g + 8) * eps * want_sums)
    if (nx, ny) == (1, 1):
        assert np.array_equal(run(linop, x, False)[0], x) and np.array_equal(run(linop, x, True)[0], x)      # the identity


@pytest.mark.parametrize("prec,dtype", PRECISIONS)
def test_more_images_than_the_grid_holds(prec, dtype):
    """the images go on the grid's y axis, 65535 at most: with L = 70000 a workgroup loops over a second image (1 x 2: 280 000 values)"""
    prost.set_precision(prec)
    case = nx, ny, L = (1, 2, 70000)
    bf, n = block(case)
    linop = [bf(0, 0, n, n)[0]]
    x = np.random.default_rng(70).standard_normal(n).astype(dtype).astype(np.float64)
    for transpose in (False, True):
        got = run(linop, x, transpose)[0]
        assert np.array_equal(got, R.product(x, nx, ny, L, transpose, dtype).astype(np.float64)), transpose


@pytest.mark.parametrize("prec,dtype", PRECISIONS)
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_composition_bit_for_bit(prec, dtype, case):
    """[K K]: the second block adds onto the first in the forward product; [K ; K]: in the transposed one; diag(d, K) with a 1 x 1 diags
    block d in front: K's rows and columns start at element 1"""
    prost.set_precision(prec)
    rng = np.random.default_rng(R.case_seed(case, 1))
    bf, n = block(case)
    P = lambda v, transpose, res0=None: R.product(v, *case, transpose, dtype, res0=res0)
    x2, x1 = rng.standard_normal(2 * n), rng.standard_normal(n)
    side = [bf(0, 0, n, n)[0], bf(0, n, n, n)[0]]
    assert np.array_equal(run(side, x2, False)[0], P(x2[n:], False, res0=P(x2[:n], False)).astype(np.float64))
    assert np.array_equal(run(side, x1, True)[0], np.tile(P(x1, True), 2).astype(np.float64))
    stack = [bf(0, 0, n, n)[0], bf(n, 0, n, n)[0]]
    assert np.array_equal(run(stack, x1, False)[0], np.tile(P(x1, False), 2).astype(np.float64))
    assert np.array_equal(run(stack, x2, True)[0], P(x2[n:], True, res0=P(x2[:n], True)).astype(np.float64))
    shifted = [prost.block.diags(1, 1, [2.0], [0])(0, 0, 1, 1)[0], bf(1, 1, n, n)[0]]
    for transpose in (False, True):
        xs = rng.standard_normal(n + 1)
        got = run(shifted, xs, transpose)[0]
        want = np.concatenate([(np.zeros(1, dtype) + dtype(2.0) * xs[:1].astype(dtype)), P(xs[1:], transpose)])
        assert np.array_equal(got, want.astype(np.float64)), transpose
        assert np.array_equal(run(shifted, xs, transpose)[0], got)


def entry(dtype):
    fn = _hip.fn("fft2d", dtype)
    fn.argtypes = [C.c_void_p] * 5 + [C.c_int, C.c_void_p]
    fn.restype = C.c_int
    return fn


def call(dtype, x, res0, geometry, table, accumulate, offset):
    """one launch through the C ABI; res, rhs and work start `offset` elements into their allocations"""
    pad = np.zeros(offset, dtype)
    keep = [_hip.DeviceArray.from_host(np.concatenate([pad, x.astype(dtype)])), _hip.DeviceArray.from_host(np.concatenate([pad, res0.astype(dtype)])),
            _hip.DeviceArray.from_host(np.concatenate([pad, np.zeros(x.size, dtype)])), _hip.DeviceArray.from_host(np.ascontiguousarray(table).reshape(-1))]
    rhs, res, work, tab = keep
    try:
        _hip.check(entry(dtype)(geometry.ctypes.data_as(C.c_void_p), tab.ptr, work.offset(offset), res.offset(offset), rhs.offset(offset), int(accumulate), None))
        _hip.sync()
        out = res.to_host()
        assert out.size == offset + x.size and np.array_equal(out[:offset], pad) and np.array_equal(work.to_host()[:offset], pad)
        assert np.array_equal(rhs.to_host()[offset:], x.astype(dtype))
        return out[offset:]
    finally:
        for d in keep:
            d.free()


@pytest.mark.parametrize("prec,dtype", PRECISIONS)
def test_c_abi_offset_pointers_plain_and_accumulating(prec, dtype):
    """offset 0 / 4: 16-byte aligned; 1: aligned for one element only.  The table is the reference's, made from the definition."""
    rng = np.random.default_rng(12)
    for case in ((4, 8, 1), (64, 32, 1), (1, 64, 1), (32, 32, 3)):
        nx, ny, L = case
        n = 2 * L * nx * ny
        table = R.table(max(nx, ny), dtype)
        for transpose in (False, True):
            x, res0 = rng.standard_normal(n).astype(dtype), rng.standard_normal(n).astype(dtype)
            geometry = R.abi_record(nx, ny, L, transpose)
            plain = R.product(x, nx, ny, L, transpose, dtype)
            for offset in (0, 1, 4):
                assert np.array_equal(call(dtype, x, res0, geometry, table, False, offset), plain), (case, transpose, offset)
                assert np.array_equal(call(dtype, x, res0, geometry, table, True, offset), res0 + plain), (case, transpose, offset)


@pytest.mark.parametrize("prec,dtype", PRECISIONS)
def test_a_nan_stays_inside_its_own_image(prec, dtype):
    prost.set_precision(prec)
    case = nx, ny, L = (32, 32, 3)
    bf, n = block(case)
    linop = [bf(0, 0, n, n)[0]]
    N = nx * ny
    x = np.random.default_rng(4).standard_normal(n)
    for transpose in (False, True):
        clean = run(linop, x, transpose)[0].reshape(2, L, N)
        assert np.isfinite(clean).all()
        for at in (0, N // 2 + 5, L * N + 7):                       # re_0 twice, im_0 once
            xn = x.copy()
            xn[at] = np.nan
            got = run(linop, xn, transpose)[0].reshape(2, L, N)
            assert np.isnan(got[:, 0]).any()                            # it reaches its own image (how far is not defined)
            assert np.array_equal(got[:, 1:], clean[:, 1:])
        for bad in (np.inf, -np.inf):
            xn = x.copy()
            xn[3] = bad
            got = run(linop, xn, transpose)[0].reshape(2, L, N)
            assert np.array_equal(got[:, 1:], clean[:, 1:])


@pytest.mark.parametrize("prec,dtype", PRECISIONS)
@pytest.mark.parametrize("case", [(8, 4, 1), (16, 16, 1)], ids=R.case_id)
def test_against_the_dense_twin_on_the_gpu(prec, dtype, case):
    prost.set_precision(prec)
    nx, ny, L = case
    rng = np.random.default_rng(100 + nx)
    K = R.matrix(nx, ny, L)
    n = K.shape[0]
    twin = [prost.block.dense(K)(0, 0, n, n)[0]]
    linop = [prost.block.fft2d(nx, ny, L)(0, 0, n, n)[0]]
    B = R.bound(nx, ny, dtype) * (2 if dtype == np.float64 else 1)
    for transpose in (False, True):
        x = rng.standard_normal(n).astype(dtype).astype(np.float64)
        got, want = run(linop, x, transpose)[0], run(twin, x, transpose)[0]
        err = R.pair_norms(got - want, nx, ny, L) / R.pair_norms(x, nx, ny, L)
        print("%s %s transpose=%d: |got - twin| / (B |x|) = %.3f" % (prec, R.case_id(case), transpose, float(err.max()) / B))
        assert np.all(err <= B), float(err.max()) / B


# ---- the solve ----
SOLVE_ITERS = 200
SOLVE_SIZE = 16


@contextlib.contextmanager
def twin_as_sparse():
    """the oracle has no dense block: while this holds, the example's twin hands its full matrix over through prost.block.sparse"""
    import scipy.sparse as sp
    dense = prost.block.dense
    prost.block.dense = lambda K: prost.block.sparse(sp.csc_matrix(K))
    try:
        yield
    finally:
        prost.block.dense = dense


@functools.lru_cache(maxsize=None)
def solve_three_ways(precision):
    import tv_mri as ex
    dtype = dict(PRECISIONS)[precision]
    backend = prost.backend.pdhg(stepsize="alg1", residual_iter=10)
    opts = dict(max_iters=SOLVE_ITERS, num_cback_calls=0, verbose=False, tol_rel_primal=0, tol_rel_dual=0, tol_abs_primal=0, tol_abs_dual=0)
    prost.set_precision(precision)
    out = {}
    prob, _, _, u, _, data, mask = ex.describe(SOLVE_SIZE, 0.5, twin=True, scaling=None)
    assert mask.mean() == 0.5
    r = prost.solve(prob, backend, prost.options(**opts))
    out["ii"] = (np.array(u.val, dtype=np.float64).ravel(), r)
    with twin_as_sparse():
        prob, _, _, u, _, _, _ = ex.describe(SOLVE_SIZE, 0.5, twin=True, scaling=None, data=data)
    r = oracle.solve(prob, backend, prost.options(**opts), dtype)
    out["iii"] = (np.array(u.val, dtype=np.float64).ravel(), r)
    prob, _, _, u, _, _, _ = ex.describe(SOLVE_SIZE, 0.5, scaling=None, data=data)
    r = prost.solve(prob, backend, prost.options(**opts))
    out["i"] = (np.array(u.val, dtype=np.float64).ravel(), r)
    return out


@pytest.mark.parametrize("precision,dtype", PRECISIONS)
def test_solve_with_the_block_against_the_dense_twin(precision, dtype):
    out = solve_three_ways(precision)
    (u1, r1), (u2, r2), (u3, r3) = out["i"], out["ii"], out["iii"]
    assert r1["iters"] == SOLVE_ITERS and r2["iters"] == SOLVE_ITERS and r3["iters"] == SOLVE_ITERS
    assert r1["path"] == "pdhg:generic", r1["path"]
    assert np.isfinite(u1).all() and u1.shape == u3.shape == (2 * SOLVE_SIZE * SOLVE_SIZE,)
    scale = float(np.abs(u3).max())
    D = float(np.abs(u2 - u3).max()) / scale
    mine = float(np.abs(u1 - u3).max()) / scale
    limit = max(10 * D, 10 * SOLVE_ITERS * R.bound(SOLVE_SIZE, SOLVE_SIZE, dtype))       # c u = B
    print("solve %s: D = |u_ii - u_iii| / |u_iii| = %.3g, |u_i - u_iii| / |u_iii| = %.3g, |u_i - u_ii| / |u_iii| = %.3g, limit %.3g"
          % (precision, D, mine, float(np.abs(u1 - u2).max()) / scale, limit))
    assert mine <= limit, (mine, limit)


def test_the_example_reconstructs_the_phantom():
    import tv_mri as ex
    prost.set_precision("double")
    size = 32
    result, img, truth, data = ex.main(size, max_iters=5000, verbose=False)
    zero_filled = ex.rmse(ex.zero_filled(data, size, size), truth)
    print("example: %s after %d iterations on %s, RMSE %.5f, zero-filled %.5f" % (result["result"], result["iters"], result["path"], ex.rmse(img, truth), zero_filled))
    assert result["result"] in ("Converged.", "Reached maximum iterations.") and (result["result"] == "Converged." or result["iters"] == 5000)
    assert result["path"] == "pdhg:generic", result["path"]
    assert img.size == 2 * size * size and np.isfinite(img).all()
    assert abs(zero_filled - 0.10352) < 1e-4                # the comparator runs no code of the block
    assert ex.rmse(img, truth) <= 0.6 * zero_filled
