"""prost.block.fanbeam2d on the GPU: the kernels through prost.eval_linop and through the C ABI, the block in the solver and in
examples/tv_ct_fan.py.

References: tests/fanbeam2d_reference.py, never the code under test.
  * products: forward and adjoint equal the NumPy restatement (b) in T bit for bit, the same call twice gives the same bits; row and
    column sums within (t + 8) eps_T of the fsum sums (c), t the entries of that row or column, and exactly 0 where there are none;
  * composition: [K K] and [K ; K] accumulate in the forward and in the adjoint product (the restatement adds res + value), a 1 x 1
    diags block in front gives the block odd row and column offsets: bit for bit;
  * against block.sparse of matrix (a) on the GPU: |got - twin| <= 1.01 (t + 1) u (|K| |x|) componentwise, u the unit roundoff of T --
    the forward error bound of a t-term sum of rounded products in any order, the margin of test_gpu_radon2d.py (derived, not measured);
  * an Inf in a pixel no ray samples stays out of every bin; a NaN in a sampled pixel reaches exactly the bins the matrix says;
  * the C entry points at element offsets 0, 1 and 4, plain and accumulating: bit for bit;
  * the CT problem at 24 x 24 with 12 views, alg1 with fixed steps, 200 iterations, tolerances 0: the sparse twin in fp32 and in fp64,
    the block in fp32 and in fp64.  D = |twin32 - twin64| / |twin64| is the twin's own fp32-to-fp64 distance; the fp32 block is held to
    4 D from the twin's fp64 iterates and the fp64 block to 4 D eps64 / eps32, the scaling of test_gpu_hessian2d.py;
  * examples/tv_ct_fan.py at 32 x 32 from 24 views: with the block on the GPU (i), with the sparse twin on the GPU (ii) and in the
    oracle (iii).  D = |u_ii - u_iii| / |u_iii| is measured on the pair that runs no code of the block; (i) is held to
    max(10 D, 10 iters t u) of (iii), the rule of test_gpu_conv2d.py and test_gpu_radon2d.py, t = 64 the entries of a row of the
    projector.  The reconstruction's RMSE to the phantom is below that of the unregularised back-projection K^T f with its
    least-squares step, which runs no code of the block.

The kernels' units are 64 bins of one view (forward) and 64 rows of one column (adjoint) per wavefront, four wavefronts per workgroup:
the case list holds ndet 1 / 63 / 65 / 130 and images of 70 rows.  At a row-driven view the forward kernel reads the image through LDS
slabs of 16 rows by up to 128 columns, whose width it measures: 40 x 150 is three slabs of rows, and at spacing 2 the 64 bins of a wave
span more than 128 columns, which are then read directly.  The margins of the cases are 1 .. 5, one adjoint instance each.
"""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

import fanbeam2d_reference as F
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


@pytest.mark.parametrize("prec,dtype", PRECISIONS)
@pytest.mark.parametrize("case", F.CASES, ids=F.case_id)
def test_products_bit_for_bit_and_sums(prec, dtype, case):
    prost.set_precision(prec)
    args = F.case_args(case)
    rng = np.random.default_rng(F.case_seed(case))
    bf = prost.block.fanbeam2d(*args)
    nrows, ncols = bf(0, 0, 0, 0)[1]
    linop = [bf(0, 0, nrows, ncols)[0]]
    rs, cs = F.sums(*args, 1.0, dtype)
    trow, tcol = F.terms(*args, dtype)
    eps = np.finfo(dtype).eps
    for transpose in (False, True):
        x = rng.standard_normal(nrows if transpose else ncols)
        got, rowsum, colsum = run(linop, x, transpose)
        want = F.product(x, *args, transpose, dtype).astype(np.float64)
        assert got.shape == want.shape and np.array_equal(got, want), (transpose, float(np.abs(got - want).max()), int((got != want).sum()))
        assert np.array_equal(run(linop, x, transpose)[0], got)                 # no atomics: the same bits every time
        assert rowsum.shape == rs.shape and colsum.shape == cs.shape
        assert within(rowsum, rs, (trow + 8) * eps) and within(colsum, cs, (tcol + 8) * eps)
    if case[4] in (63, 130) and case[7] == "closest":
        assert (rs == 0).any()                                                  # a detector longer than the fan needs: rays that miss, exactly 0


@pytest.mark.parametrize("prec,dtype", PRECISIONS)
@pytest.mark.parametrize("case", F.CASES, ids=F.case_id)
def test_composition_bit_for_bit(prec, dtype, case):
    """[K K]: the second block adds onto the first in the forward product; [K ; K]: in the adjoint; diag(d, K) with a 1 x 1 diags block
    d in front: K's rows and columns start at element 1"""
    prost.set_precision(prec)
    arg = F.case_args(case)
    rng = np.random.default_rng(F.case_seed(case, 1))
    bf = prost.block.fanbeam2d(*arg)
    m, n = bf(0, 0, 0, 0)[1]
    xn2, xn, xm2, xm = rng.standard_normal(2 * n), rng.standard_normal(n), rng.standard_normal(2 * m), rng.standard_normal(m)
    side = [bf(0, 0, m, n)[0], bf(0, n, m, n)[0]]
    want = F.product(xn2[n:], *arg, False, dtype, res0=F.product(xn2[:n], *arg, False, dtype))
    assert np.array_equal(run(side, xn2, False)[0], want.astype(np.float64))
    assert np.array_equal(run(side, xm, True)[0], np.tile(F.product(xm, *arg, True, dtype), 2).astype(np.float64))
    stack = [bf(0, 0, m, n)[0], bf(m, 0, m, n)[0]]
    assert np.array_equal(run(stack, xn, False)[0], np.tile(F.product(xn, *arg, False, dtype), 2).astype(np.float64))
    want = F.product(xm2[m:], *arg, True, dtype, res0=F.product(xm2[:m], *arg, True, dtype))
    assert np.array_equal(run(stack, xm2, True)[0], want.astype(np.float64))
    shifted = [prost.block.diags(1, 1, [2.0], [0])(0, 0, 1, 1)[0], bf(1, 1, m, n)[0]]
    for transpose in (False, True):
        xs = rng.standard_normal((m if transpose else n) + 1)
        got = run(shifted, xs, transpose)[0]
        want = np.concatenate([(np.zeros(1, dtype) + dtype(2.0) * xs[:1].astype(dtype)), F.product(xs[1:], *arg, transpose, dtype)])
        assert np.array_equal(got, want.astype(np.float64)), transpose
        assert np.array_equal(run(shifted, xs, transpose)[0], got)


@pytest.mark.parametrize("prec,dtype", PRECISIONS)
@pytest.mark.parametrize("case", F.CASES, ids=F.case_id)
def test_against_the_sparse_twin_on_the_gpu(prec, dtype, case):
    prost.set_precision(prec)
    args = F.case_args(case)
    rng = np.random.default_rng(F.case_seed(case, 2))
    K = F.matrix(*args, dtype)
    m, n = K.shape
    twin = [prost.block.sparse(K)(0, 0, m, n)[0]]
    linop = [prost.block.fanbeam2d(*args)(0, 0, m, n)[0]]
    for transpose in (False, True):
        x = rng.standard_normal(m if transpose else n).astype(dtype).astype(np.float64)
        got = run(linop, x, transpose)[0]
        want = run(twin, x, transpose)[0]
        bound = F.bound(*args, transpose, x, dtype)
        err = np.abs(got - want)
        live = bound > 0
        print("%s %s transpose=%d: |got - twin| / bound %.3f" % (prec, F.case_id(case), transpose, float((err[live] / bound[live]).max()) if live.any() else 0.0))
        assert np.all(err <= bound), float((err[live] / bound[live]).max())


UNSEEN = (7, 9, 1, np.array([0.0, 1.0]), 12.0, 12.0, 3, 1.0, 0.0, "flat")      # two views and three bins over 9 x 7: the corners are never sampled


@pytest.mark.parametrize("prec,dtype", PRECISIONS)
def test_inf_in_an_unsampled_pixel_and_nan_in_a_sampled_one(prec, dtype):
    prost.set_precision(prec)
    args = UNSEEN
    K = F.matrix(*args, dtype).tocsc()
    m, n = K.shape
    per_column = np.diff(K.indptr)
    unseen, seen = np.nonzero(per_column == 0)[0], np.nonzero(per_column > 0)[0]
    assert unseen.size and seen.size
    linop = [prost.block.fanbeam2d(*args)(0, 0, m, n)[0]]
    x = np.random.default_rng(4).standard_normal(n)
    clean = run(linop, x, False)[0]
    assert np.isfinite(clean).all()
    for bad in (np.inf, -np.inf, np.nan):
        xi = x.copy()
        xi[unseen] = bad
        assert np.array_equal(run(linop, xi, False)[0], clean), bad
    for j in (seen[0], seen[len(seen) // 2], seen[-1]):
        xn = x.copy()
        xn[j] = np.nan
        got = run(linop, xn, False)[0]
        hit = np.zeros(m, bool)
        hit[K.indices[K.indptr[j]:K.indptr[j + 1]]] = True
        assert np.array_equal(np.isnan(got), hit), j
        assert np.array_equal(got[~hit], clean[~hit])
    # the adjoint: a bin whose ray misses the image may hold anything
    args = F.case_args(F.CASES[3])                  # 63 bins at spacing 0.5 over 3 x 5: rays that miss the image
    Kr = F.matrix(*args, dtype)
    m, n = Kr.shape
    per_row = np.diff(Kr.indptr)
    assert (per_row == 0).any()
    linop = [prost.block.fanbeam2d(*args)(0, 0, m, n)[0]]
    y = np.random.default_rng(5).standard_normal(m)
    clean = run(linop, y, True)[0]
    yi = y.copy()
    yi[per_row == 0] = np.inf
    assert np.isfinite(clean).all() and np.array_equal(run(linop, yi, True)[0], clean)


def entry(dtype):
    fn = _hip.fn("fanbeam2d", dtype)
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    fn.restype = C.c_int
    return fn


def call(dtype, x, res0, geometry, table, nres, accumulate, offset):
    """one launch through the C ABI; res and rhs start `offset` elements into their allocations"""
    pad = np.zeros(offset, dtype)
    keep = [_hip.DeviceArray.from_host(np.concatenate([pad, x.astype(dtype)])), _hip.DeviceArray.from_host(np.concatenate([pad, res0.astype(dtype)])),
            _hip.DeviceArray.from_host(np.ascontiguousarray(table, dtype=dtype).ravel())]
    rhs, res, tab = keep
    try:
        _hip.check(entry(dtype)(geometry.ctypes.data_as(C.c_void_p), tab.ptr, res.offset(offset), rhs.offset(offset), int(accumulate), None))
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
    for case in (F.CASES[2], F.CASES[5], F.CASES[7]):
        nx, ny, L, angles, dist, D, ndet, spacing, shift, detector = args = F.case_args(case)
        table = F.table(nx, ny, angles, dist, D, ndet, spacing, shift, detector, dtype)
        m, n = L * len(angles) * ndet, L * nx * ny
        for transpose in (False, True):
            nres, nrhs = (n, m) if transpose else (m, n)
            x, res0 = rng.standard_normal(nrhs).astype(dtype), rng.standard_normal(nres).astype(dtype)
            geometry = F.abi_records(*args, transpose)
            plain = F.product(x, *args, transpose, dtype)
            for offset in (0, 1, 4):
                assert np.array_equal(call(dtype, x, res0, geometry, table, nres, False, offset), plain), (case, transpose, offset)
                assert np.array_equal(call(dtype, x, res0, geometry, table, nres, True, offset), res0 + plain), (case, transpose, offset)


# ---- the solve ----
SOLVE_ITERS = 200
SOLVE_SIZE, SOLVE_VIEWS = 24, 12
SOLVE_MULTIPLE = 4


@functools.lru_cache(maxsize=None)
def solve_four_ways():
    import tv_ct_fan as ex
    backend = prost.backend.pdhg(stepsize="alg1", residual_iter=10)
    opts = dict(max_iters=SOLVE_ITERS, num_cback_calls=0, verbose=False, tol_rel_primal=0, tol_rel_dual=0, tol_abs_primal=0, tol_abs_dual=0)
    out, sinogram = {}, None
    for twin, precision, dtype in ((True, "double", np.float64), (True, "single", np.float32), (False, "single", np.float32), (False, "double", np.float64)):
        prost.set_precision(precision)
        prob, _, _, u, _, made = ex.describe(SOLVE_SIZE, SOLVE_VIEWS, twin=twin, dtype=dtype, sinogram=sinogram)
        sinogram = made if sinogram is None else sinogram                          # every run has the data of the first
        r = prost.solve(prob, backend, prost.options(**opts))
        out[(twin, precision)] = (np.array(u.val, dtype=np.float64).ravel(), r)
    return out


def test_solve_with_the_block_against_the_sparse_twin():
    out = solve_four_ways()
    (t64, r1), (t32, r2), (b32, r3), (b64, r4) = out[(True, "double")], out[(True, "single")], out[(False, "single")], out[(False, "double")]
    assert all(r["iters"] == SOLVE_ITERS for r in (r1, r2, r3, r4))
    assert r3["path"] == "pdhg:generic" and r4["path"] == "pdhg:generic"
    assert np.isfinite(b32).all() and np.isfinite(b64).all() and b32.shape == t64.shape == (SOLVE_SIZE * SOLVE_SIZE,)
    scale = float(np.abs(t64).max())
    D = float(np.abs(t32 - t64).max()) / scale
    mine32, mine64 = float(np.abs(b32 - t64).max()) / scale, float(np.abs(b64 - t64).max()) / scale
    limit64 = SOLVE_MULTIPLE * D * (np.finfo(np.float64).eps / np.finfo(np.float32).eps)
    print("solve: D = |twin32 - twin64| / |twin64| = %.3g; fp32 block %.3g (%.2f D); fp64 block %.3g (%.2f of its limit %.3g)" % (D, mine32, mine32 / D, mine64, mine64 / limit64, limit64))
    assert D > 0
    assert mine32 <= SOLVE_MULTIPLE * D, (mine32, D)
    assert mine64 <= limit64, (mine64, limit64)


def test_the_example_reconstructs_the_phantom():
    import tv_ct_fan as ex
    prost.set_precision("double")
    size, n_views = 32, 24
    result, img, truth, sinogram = ex.main(size, n_views, max_iters=5000, verbose=False)
    assert result["result"] in ("Converged.", "Reached maximum iterations.") and (result["result"] == "Converged." or result["iters"] == 5000)
    assert result["path"] == "pdhg:generic", result["path"]
    assert img.size == size * size and np.isfinite(img).all() and img.min() >= 0
    assert sinogram.shape == (n_views * prost.block.fanbeam2d_ndet(size, size, 3.0 * np.hypot(size, size) / 2),)
    # the twin with the same data, on the GPU and in the oracle
    prob, backend, opts, u, _, _ = ex.describe(size, n_views, twin=True, sinogram=sinogram)
    r2 = prost.solve(prob, backend, opts)
    u2 = np.array(u.val, dtype=np.float64).ravel()
    prob, backend, opts, u, _, _ = ex.describe(size, n_views, twin=True, sinogram=sinogram)
    r3 = oracle.solve(prob, backend, opts, np.float64)
    u3 = np.array(u.val, dtype=np.float64).ravel()
    scale = float(np.abs(u3).max())
    D = float(np.abs(u2 - u3).max()) / scale
    mine = float(np.abs(np.asarray(img, dtype=np.float64).ravel() - u3).max()) / scale
    limit = max(10 * D, 10 * result["iters"] * 2 * size * (np.finfo(np.float64).eps / 2))
    back = ex.rmse(ex.back_projection(size, n_views, sinogram), truth)
    print("example: %s after %d iterations (twin %d, oracle %d) on %s; D = %.3g, |u_i - u_iii| / |u_iii| = %.3g, limit %.3g; RMSE %.5f, back-projection %.5f"
          % (result["result"], result["iters"], r2["iters"], r3["iters"], result["path"], D, mine, limit, ex.rmse(img, truth), back))
    assert result["iters"] == r2["iters"] == r3["iters"]
    assert mine <= limit, (mine, limit)
    assert ex.rmse(img, truth) < back
