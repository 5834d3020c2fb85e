"""prost.block.radon2d on the GPU: the kernels through prost.eval_linop and through the C ABI, the block in the solver and in
examples/tv_ct.py.

References: tests/radon2d_reference.py, never the code under test.
  * products: forward and adjoint equal the NumPy restatement (b) in T bit for bit, the same call twice gives the same bits; row and
    column sums within (t + 8) eps_T of (c), t the entries of that row or column, and exactly 0 where there are none;
  * composition: [K K] and [K ; K] accumulate in the forward and in the adjoint product (the restatement adds res + value), a 1 x 1
    diags block in front gives the block odd row and column offsets: bit for bit;
  * against block.sparse of matrix (a) on the GPU: |got - twin| <= 1.01 (t + 1) u (|K| |x|) componentwise, u the unit roundoff of T --
    the forward error bound of a t-term sum of rounded products in any order (derived, not measured);
  * an Inf in a pixel no ray samples stays out of every bin; a NaN in a sampled pixel reaches exactly the bins the matrix says;
  * the C entry points at element offsets 0, 1 and 4, plain and accumulating: bit for bit;
  * the CT problem at 32 x 32 with 24 angles, alg1 with fixed steps, 200 iterations, tolerances 0: with the block on the GPU (i), with
    the sparse twin on the GPU (ii) and in the oracle (iii).  D = |u_ii - u_iii| / |u_iii|, measured in the test on the pair that runs
    no code of the block; (i) is held to max(10 D, 10 * 200 * t * u) of (iii), the rule of test_gpu_conv2d.py, t = 64 the entries of a
    row of the projector;
  * examples/tv_ct.py at 32 x 32 from 24 angles.  The oracle with the sparse twin on the CPU reaches an RMSE to the phantom of 0.00735
    in fp64 (198 iterations, "Converged."); the phantom's own mean image, which needs no reconstruction at all, has 0.2159.  The
    inequality asked of the GPU run with the block is RMSE <= 0.1 * 0.2159 = 0.02159, which the oracle meets 2.9 times over.

The kernels' units are 64 bins of one angle (forward) and 64 rows of one column (adjoint) per wavefront, four wavefronts per workgroup:
the case list holds ndet 63 / 64 / 65 / 130 and images of exactly 64 rows and of 65.  At a row-driven angle the forward kernel reads the
image through LDS slabs of 16 rows by up to 128 columns: 16 x 128 under 64 bins at spacing 2.5 is one slab exactly, 17 x 129 a second
slab and one too wide to be staged; 150 rows are ten slabs, the last of six rows.
"""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

import radon2d_reference as R
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
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_products_bit_for_bit_and_sums(prec, dtype, case):
    prost.set_precision(prec)
    args = R.case_args(case)
    rng = np.random.default_rng(R.case_seed(case))
    bf = prost.block.radon2d(*args)
    nrows, ncols = bf(0, 0, 0, 0)[1]
    linop = [bf(0, 0, nrows, ncols)[0]]
    rs, cs = R.sums(*args, 1.0, dtype)
    trow, tcol = R.terms(*args, dtype)
    eps = np.finfo(dtype).eps
    for transpose in (False, True):
        x = rng.standard_normal(nrows if transpose else ncols)
        got, rowsum, colsum = run(linop, x, transpose)
        want = R.product(x, *args, transpose, dtype).astype(np.float64)
        assert got.shape == want.shape and np.array_equal(got, want), (transpose, float(np.abs(got - want).max()), int((got != want).sum()))
        assert np.array_equal(run(linop, x, transpose)[0], got)                 # no atomics: the same bits every time
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
    bf = prost.block.radon2d(*arg)
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
    linop = [prost.block.radon2d(*args)(0, 0, m, n)[0]]
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
def test_inf_in_an_unsampled_pixel_and_nan_in_a_sampled_one(prec, dtype):
    prost.set_precision(prec)
    case = R.CASES[5]                               # two angles and three bins over 9 x 7: the corners are never sampled
    args = R.case_args(case)
    K = R.matrix(*args, dtype).tocsc()
    m, n = K.shape
    per_column = np.diff(K.indptr)
    unseen, seen = np.nonzero(per_column == 0)[0], np.nonzero(per_column > 0)[0]
    assert unseen.size and seen.size
    linop = [prost.block.radon2d(*args)(0, 0, m, n)[0]]
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
    case = R.CASES[3]                               # 63 bins at spacing 0.5 over 5 x 5: rays that miss the image
    args = R.case_args(case)
    Kr = R.matrix(*args, dtype)
    m, n = Kr.shape
    per_row = np.diff(Kr.indptr)
    assert (per_row == 0).any()
    linop = [prost.block.radon2d(*args)(0, 0, m, n)[0]]
    y = np.random.default_rng(5).standard_normal(m)
    clean = run(linop, y, True)[0]
    yi = y.copy()
    yi[per_row == 0] = np.inf
    assert np.isfinite(clean).all() and np.array_equal(run(linop, yi, True)[0], clean)


def entry(dtype):
    fn = _hip.fn("radon2d", dtype)
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
    for case in (R.CASES[2], R.CASES[6], R.CASES[10]):
        nx, ny, L, angles, ndet, spacing, shift = args = R.case_args(case)
        table = R.table(nx, ny, angles, ndet, spacing, shift, dtype)
        m, n = L * len(angles) * ndet, L * nx * ny
        for transpose in (False, True):
            nres, nrhs = (n, m) if transpose else (m, n)
            x, res0 = rng.standard_normal(nrhs).astype(dtype), rng.standard_normal(nres).astype(dtype)
            geometry = R.abi_records(nx, ny, L, angles, ndet, spacing, transpose)
            plain = R.product(x, *args, transpose, dtype)
            for offset in (0, 1, 4):
                assert np.array_equal(call(dtype, x, res0, geometry, table, nres, False, offset), plain), (case, transpose, offset)
                assert np.array_equal(call(dtype, x, res0, geometry, table, nres, True, offset), res0 + plain), (case, transpose, offset)


# ---- the solve ----
SOLVE_ITERS = 200
SOLVE_SIZE, SOLVE_ANGLES = 32, 24
SOLVE_TERMS = 2 * SOLVE_SIZE              # entries of a row of the projector: two per driving line


@functools.lru_cache(maxsize=None)
def solve_three_ways(precision):
    import tv_ct as ex
    dtype = dict(PRECISIONS)[precision]
    backend = prost.backend.pdhg(stepsize="alg1", residual_iter=10)
    opts = dict(max_iters=SOLVE_ITERS, num_cback_calls=0, verbose=False, tol_rel_primal=0, tol_rel_dual=0, tol_abs_primal=0, tol_abs_dual=0)
    prost.set_precision(precision)
    out = {}
    prob, _, _, u, _, sinogram = ex.describe(SOLVE_SIZE, SOLVE_ANGLES, twin=True, dtype=dtype)
    r = prost.solve(prob, backend, prost.options(**opts))
    out["ii"] = (np.array(u.val, dtype=np.float64).ravel(), r)
    prob, _, _, u, _, _ = ex.describe(SOLVE_SIZE, SOLVE_ANGLES, twin=True, dtype=dtype, sinogram=sinogram)
    r = oracle.solve(prob, backend, prost.options(**opts), dtype)
    out["iii"] = (np.array(u.val, dtype=np.float64).ravel(), r)
    prob, _, _, u, _, _ = ex.describe(SOLVE_SIZE, SOLVE_ANGLES, sinogram=sinogram)
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
    import tv_ct as ex
    prost.set_precision("double")
    size, n_angles = 32, 24
    result, img, truth, sinogram = ex.main(size, n_angles, max_iters=5000, verbose=False)
    mean_image = ex.rmse(np.full(truth.size, truth.mean()), truth)
    print("example: %s after %d iterations on %s, RMSE %.5f, mean image %.5f" % (result["result"], result["iters"], result["path"], ex.rmse(img, truth), mean_image))
    assert result["result"] in ("Converged.", "Reached maximum iterations.") and (result["result"] == "Converged." or result["iters"] == 5000)
    assert result["path"] == "pdhg:generic", result["path"]
    assert img.size == size * size and np.isfinite(img).all() and img.min() >= 0
    assert sinogram.shape == (n_angles * prost.block.radon2d_ndet(size, size),)
    assert abs(mean_image - 0.2159) < 1e-4                  # the comparator runs no code of the block
    assert ex.rmse(img, truth) <= 0.1 * mean_image
