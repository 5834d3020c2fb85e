"""prost.block.sym_gradient2d on the GPU: the kernels through prost.eval_linop and through the C ABI, the block in the solver and in
examples/tgv2_denoise.py.

References: tests/sym_gradient2d_reference.py, never the code under test.
  * products: forward and adjoint equal the NumPy restatement (b) in T bit for bit, the same call twice gives the same bits; row and
    column sums within (t + 8) eps_T of (c), t = 4; both precisions, w = 0.5 and sqrt(1/2);
  * composition: [E E] and [E ; E] accumulate in the forward and in the adjoint product (the restatement adds res + value), a 1 x 1
    diags block in front gives the block odd element offsets and so the element kernels: bit for bit;
  * against the oracle's block.sparse on matrix (a): |got - twin| <= 1.01 (t + 1) u (|E| |x|) componentwise, u the unit roundoff of T
    (derived, not measured); the twin adds in ascending column order, the stated order, so 0 is expected;
  * absent terms: Inf in every domain element whose column of (a) is empty reaches no output, a NaN elsewhere reaches exactly the
    outputs of its column;
  * the C entry points at element offsets 0, 1 and 4, plain and accumulating, both directions: bit for bit; refusals without a launch;
  * TGV^2 at 24 x 16 with L = 1 and L = 3, alg1 with fixed steps, 200 iterations: the block on the GPU (i), the sparse twin on the GPU
    (ii) and in the oracle (iii).  w = 0.5: (i) equals (ii) bit for bit.  The default w: with D = |(ii) - (iii)| / |(iii)|, which runs
    no code of the block, |(i) - (iii)| / |(iii)| <= max(10 D, 10 * 200 * t * u) (figures: docs/rounds/r19.md);
  * the example: converges, and its RMSE to the clean image is below that of TV on the same data.

Shapes (sym_gradient2d_reference.CASES), from the kernel's constants: a workgroup has BLOCK = 256 lanes of VEC = 16 / sizeof(T) rows,
so one strip of the vector path is 1024 rows in fp32 and 512 in fp64 -- the list holds both, each with one row more (the element
kernels) and one vector more (a second strip).  A chunk has kColumnChoices = 12, 6 or 3 columns, the largest that leaves kFillBlocks =
2048 workgroups, else 1: the small shapes run one column per chunk (nx = 1 is exactly one chunk, every other one more); nx = 2048 c at
one strip and one channel is the smallest grid of full chunks of c columns, and nx = 2048 c + 1 adds a chunk of one column.
"""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

import oracle
import prost_amd as prost
import sym_gradient2d_reference as R
from prost_amd import _hip

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))

pytestmark = pytest.mark.gpu
PRECISIONS = [("single", np.float32), ("double", np.float64)]
WEIGHTS = [R.W_HALF, R.W_FROB]


@pytest.fixture(autouse=True)
def _gpu(hip):
    prost.set_gpu(0)
    yield
    prost.set_precision("double")


def run(linop, rhs, transpose):
    got, rowsum, colsum, _ = prost.eval_linop(linop, rhs, transpose)
    return np.asarray(got, dtype=np.float64).ravel(), np.asarray(rowsum, dtype=np.float64).ravel(), np.asarray(colsum, dtype=np.float64).ravel()


def block(nx, ny, L, w, row=0, col=0):
    bf = prost.block.sym_gradient2d(nx, ny, L, w)
    m, n = bf(0, 0, 0, 0)[1]
    return bf(row, col, m, n)[0], m, n


def test_the_shape_list_follows_the_kernel_constants():
    assert R.strip_rows(np.float32) == 1024 and R.strip_rows(np.float64) == 512
    for ny in (512, 513, 514, 1024, 1025, 1028):
        assert any(c[0] == ny for c in R.CASES)
    for c in (3, 6, 12):
        for dtype in (np.float32, np.float64):
            assert R.pick_columns(2048 * c, 4, 1, dtype) == c and R.pick_columns(2048 * c + 1, 4, 1, dtype) == c and R.pick_columns(2048 * c - c, 4, 1, dtype) < c
        assert (4, 2048 * c, 1) in R.CASES and (4, 2048 * c + 1, 1) in R.CASES
    assert R.pick_columns(4097, 8, 3, np.float32) == 6 and 4097 % 6 == 5


@pytest.mark.parametrize("prec,dtype", PRECISIONS)
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_products_bit_for_bit_and_sums(prec, dtype, case):
    prost.set_precision(prec)
    ny, nx, L = case
    rng = np.random.default_rng(R.case_seed(case))
    tol = (R.T_TERMS + 8) * np.finfo(dtype).eps
    for w in WEIGHTS:
        b, nrows, ncols = block(nx, ny, L, w)
        rs, cs = R.sums(nx, ny, L, w, 1.0, dtype)
        for transpose in (False, True):
            x = rng.standard_normal(nrows if transpose else ncols)
            got, rowsum, colsum = run([b], x, transpose)
            want = R.product(x, nx, ny, L, w, transpose, dtype).astype(np.float64)
            assert got.shape == want.shape and np.array_equal(got, want), (w, transpose, float(np.abs(got - want).max()))
            assert np.array_equal(run([b], x, transpose)[0], got)                 # no atomics: the same bits every time
            assert rowsum.shape == rs.shape and colsum.shape == cs.shape
            assert np.all(np.abs(rowsum - rs) <= tol * rs) and np.all(np.abs(colsum - cs) <= tol * cs), w
            if w == R.W_HALF:
                assert np.array_equal(rowsum, rs) and np.array_equal(colsum, cs)


@pytest.mark.parametrize("prec,dtype", PRECISIONS)
@pytest.mark.parametrize("case", R.SMALL + R.STRIPS + R.CHUNKS[1:2] + R.CHUNKS[-1:], ids=R.case_id)
def test_composition_bit_for_bit(prec, dtype, case):
    """[E E]: the second block adds onto the first in the forward product; [E ; E]: in the adjoint; diag(d, E) with a 1 x 1 diags block
    d in front: E's rows and columns start at element 1, the pointers are aligned for one element only"""
    prost.set_precision(prec)
    ny, nx, L = case
    rng = np.random.default_rng(R.case_seed(case, 1))
    for w in WEIGHTS:
        arg = (nx, ny, L, w)
        _, m, n = block(*arg)
        xn2, xn, xm2, xm = rng.standard_normal(2 * n), rng.standard_normal(n), rng.standard_normal(2 * m), rng.standard_normal(m)
        side = [block(*arg)[0], block(*arg, 0, n)[0]]
        want = R.product(xn2[n:], *arg, False, dtype, res0=R.product(xn2[:n], *arg, False, dtype))
        assert np.array_equal(run(side, xn2, False)[0], want.astype(np.float64)), w
        assert np.array_equal(run(side, xm, True)[0], np.tile(R.product(xm, *arg, True, dtype), 2).astype(np.float64)), w
        stack = [block(*arg)[0], block(*arg, m, 0)[0]]
        assert np.array_equal(run(stack, xn, False)[0], np.tile(R.product(xn, *arg, False, dtype), 2).astype(np.float64)), w
        want = R.product(xm2[m:], *arg, True, dtype, res0=R.product(xm2[:m], *arg, True, dtype))
        assert np.array_equal(run(stack, xm2, True)[0], want.astype(np.float64)), w
        shifted = [prost.block.diags(1, 1, [2.0], [0])(0, 0, 1, 1)[0], block(*arg, 1, 1)[0]]
        for transpose in (False, True):
            xs = rng.standard_normal((m if transpose else n) + 1)
            got = run(shifted, xs, transpose)[0]
            want = np.concatenate([(np.zeros(1, dtype) + dtype(2.0) * xs[:1].astype(dtype)), R.product(xs[1:], *arg, transpose, dtype)])
            assert np.array_equal(got, want.astype(np.float64)), (w, transpose)
            assert np.array_equal(run(shifted, xs, transpose)[0], got)


@pytest.mark.parametrize("prec,dtype", PRECISIONS)
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_against_the_sparse_twin_in_the_oracle(prec, dtype, case):
    prost.set_precision(prec)
    ny, nx, L = case
    rng = np.random.default_rng(R.case_seed(case, 2))
    for w in WEIGHTS:
        E = R.matrix(nx, ny, L, w, dtype)
        m, n = E.shape
        linop = [block(nx, ny, L, R.weight(w, dtype))[0]]
        if E.nnz == 0:                                    # 1 x 1: the matrix is empty and so is the product
            for transpose in (False, True):
                assert not run(linop, rng.standard_normal(m if transpose else n), transpose)[0].any()
            continue
        twin = [prost.block.sparse(E)(0, 0, m, n)[0]]
        for transpose in (False, True):
            x = rng.standard_normal(m if transpose else n).astype(dtype).astype(np.float64)
            got = run(linop, x, transpose)[0]
            want = np.asarray(oracle.eval_linop(twin, x, transpose, dtype)[0], dtype=np.float64).ravel()
            bound = R.bound(nx, ny, L, w, transpose, x, dtype)
            err = np.abs(got - want)
            live = bound > 0
            print("%s %s w=%.3f transpose=%d: |got - twin| / bound %.3f" % (prec, R.case_id(case), w, transpose, float((err[live] / bound[live]).max()) if live.any() else 0.0))
            assert np.all(err <= bound), float((err[live] / bound[live]).max())


@pytest.mark.parametrize("prec,dtype", PRECISIONS)
def test_absent_terms_are_absent(prec, dtype):
    prost.set_precision(prec)
    nx = ny = 3
    for w in WEIGHTS:
        b, m, n = block(nx, ny, 1, w)
        x = np.random.default_rng(5).standard_normal(n)
        empty = R.empty_columns(nx, ny, 1)
        assert empty.tolist() == [8, 17]
        x[empty] = np.inf
        got = run([b], x, False)[0]
        assert np.isfinite(got).all() and np.array_equal(got, R.product(x, nx, ny, 1, w, False, dtype).astype(np.float64))
        x[4] = np.nan
        got = run([b], x, False)[0]
        want = R.product(x, nx, ny, 1, w, False, dtype).astype(np.float64)
        assert np.isnan(want).sum() == 4 and np.array_equal(got, want, equal_nan=True)
        # the same behind odd offsets (the element kernels)
        shifted = [prost.block.diags(1, 1, [2.0], [0])(0, 0, 1, 1)[0], block(nx, ny, 1, w, 1, 1)[0]]
        assert np.array_equal(run(shifted, np.concatenate([[1.0], x]), False)[0][1:], want, equal_nan=True)


def entry(dtype):
    fn = _hip.fn("linop_sym_gradient2d", dtype)
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_double, C.c_int, C.c_int, C.c_void_p]
    fn.restype = C.c_int
    return fn


def call(dtype, x, res0, nx, ny, L, w, transpose, accumulate, offset):
    """one launch through the C ABI; res and rhs start `offset` elements into their allocations"""
    pad = np.zeros(offset, dtype)
    keep = [_hip.DeviceArray.from_host(np.concatenate([pad, x.astype(dtype)])), _hip.DeviceArray.from_host(np.concatenate([pad, res0.astype(dtype)]))]
    rhs, res = keep
    try:
        _hip.check(entry(dtype)(res.offset(offset), rhs.offset(offset), nx, ny, L, w, int(transpose), int(accumulate), None))
        _hip.sync()
        out = res.to_host()
        assert out.size == offset + res0.size and np.array_equal(out[:offset], pad)
        assert np.array_equal(rhs.to_host()[offset:], x.astype(dtype))
        return out[offset:]
    finally:
        for d in keep:
            d.free()


@pytest.mark.parametrize("prec,dtype", PRECISIONS)
def test_c_abi_offset_pointers_plain_and_accumulating(prec, dtype):
    """offset 0 / 4: 16-byte aligned (the vector kernels where the height allows); 1: aligned for one element only"""
    rng = np.random.default_rng(12)
    for ny, nx, L in ((3, 3, 2), (8, 5, 2), (17, 13, 3), (1028, 2, 2)):
        for w in WEIGHTS:
            for transpose in (False, True):
                nres, nrhs = (2 * L * nx * ny, 3 * L * nx * ny) if transpose else (3 * L * nx * ny, 2 * L * nx * ny)
                x, res0 = rng.standard_normal(nrhs).astype(dtype), rng.standard_normal(nres).astype(dtype)
                plain = R.product(x, nx, ny, L, w, transpose, dtype)
                for offset in (0, 1, 4):
                    assert np.array_equal(call(dtype, x, res0, nx, ny, L, w, transpose, False, offset), plain), (ny, nx, L, w, transpose, offset)
                    assert np.array_equal(call(dtype, x, res0, nx, ny, L, w, transpose, True, offset), res0 + plain), (ny, nx, L, w, transpose, offset)
    # refusals without a launch
    fn, p = entry(dtype), C.c_void_p(16)
    for args in ((p, p, 0, 4, 1, 0.5), (p, p, 4, 0, 1, 0.5), (p, p, 4, 4, 0, 0.5), (p, p, 4, 4, 1, np.inf), (p, p, 4, 4, 1, np.nan), (p, p, 4, 4, 1, 0.0),
                 (None, p, 4, 4, 1, 0.5), (p, None, 4, 4, 1, 0.5)):
        assert fn(*args, 0, 0, None) != 0 and fn(*args, 1, 1, None) != 0, args
    if dtype == np.float32:
        assert fn(p, p, 4, 4, 1, 1e-60, 0, 0, None) != 0
    _hip.sync()


# ---- the solve ----
SOLVE_ITERS = 200
SOLVE_NX, SOLVE_NY = 24, 16


@functools.lru_cache(maxsize=None)
def solve_three_ways(precision, nc, w):
    import tgv2_denoise as ex
    dtype = dict(PRECISIONS)[precision]
    backend = prost.backend.pdhg(stepsize="alg1", residual_iter=10)
    opts = dict(max_iters=SOLVE_ITERS, num_cback_calls=0, verbose=False, tol_rel_primal=0, tol_rel_dual=0, tol_abs_primal=0, tol_abs_dual=0)
    prost.set_precision(precision)
    _, f = ex.ramp_image(SOLVE_NX, SOLVE_NY, nc)
    out = {}
    for key, twin, solver in (("i", False, None), ("ii", True, None), ("iii", True, oracle)):
        prob, _, _, u, v, _, _ = ex.describe(SOLVE_NX, SOLVE_NY, nc, w=w, f=f, twin=twin)
        r = prost.solve(prob, backend, prost.options(**opts)) if solver is None else oracle.solve(prob, backend, prost.options(**opts), dtype)
        out[key] = (np.concatenate([np.array(u.val, dtype=np.float64).ravel(), np.array(v.val, dtype=np.float64).ravel()]), r)
    return out


@pytest.mark.parametrize("precision,dtype", PRECISIONS)
@pytest.mark.parametrize("nc", [1, 3])
def test_solve_with_w_one_half_equals_the_sparse_twin_bit_for_bit(precision, dtype, nc):
    """every preconditioner sum is exact and the products are the twin's bits"""
    out = solve_three_ways(precision, nc, R.W_HALF)
    (x1, r1), (x2, r2) = out["i"], out["ii"]
    assert r1["iters"] == SOLVE_ITERS and r2["iters"] == SOLVE_ITERS
    assert r1["path"] == "pdhg:generic", r1["path"]
    assert np.isfinite(x1).all() and x1.shape == x2.shape == (3 * nc * SOLVE_NX * SOLVE_NY,)
    print("solve %s L=%d w=0.5: |(i) - (ii)|_inf = %.3g" % (precision, nc, float(np.abs(x1 - x2).max())))
    assert np.array_equal(x1, x2), float(np.abs(x1 - x2).max())


@pytest.mark.parametrize("precision,dtype", PRECISIONS)
@pytest.mark.parametrize("nc", [1, 3])
@pytest.mark.parametrize("w", WEIGHTS)
def test_solve_with_the_block_against_the_sparse_twin(precision, dtype, nc, w):
    out = solve_three_ways(precision, nc, w)
    (x1, r1), (x2, r2), (x3, r3) = out["i"], out["ii"], out["iii"]
    assert r1["iters"] == SOLVE_ITERS and r2["iters"] == SOLVE_ITERS and r3["iters"] == SOLVE_ITERS
    assert r1["path"] == "pdhg:generic", r1["path"]
    assert np.isfinite(x1).all() and x1.shape == x3.shape
    scale = float(np.abs(x3).max())
    D = float(np.abs(x2 - x3).max()) / scale
    mine = float(np.abs(x1 - x3).max()) / scale
    print("solve %s L=%d w=%.3f: D = |(ii) - (iii)| / |(iii)| = %.3g, |(i) - (iii)| / |(iii)| = %.3g, |(i) - (ii)| / |(iii)| = %.3g"
          % (precision, nc, w, D, mine, float(np.abs(x1 - x2).max()) / scale))
    # ten times first-order growth of a preconditioner difference of a few ulps over the iterations, or ten times one forward error t u
    # of a product per iteration, whichever is larger
    limit = max(10 * D, 10 * SOLVE_ITERS * R.T_TERMS * (np.finfo(dtype).eps / 2))
    assert mine <= limit, (mine, limit)


def test_the_example_beats_tv_on_a_ramp_with_a_step():
    import tgv2_denoise as ex
    prost.set_precision("double")
    nx, ny = 24, 16
    result, img, result_tv, img_tv, f, clean = ex.main(nx, ny, 1, max_iters=20000, verbose=False)
    x, y = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    assert np.array_equal(clean, (0.02 * x + 0.03 * y + 0.5 * (x > 12)).reshape(-1))
    assert np.array_equal(f, clean + 0.05 * np.random.default_rng(1).standard_normal(nx * ny))
    print("example: TGV^2 %s after %d iterations on %s, RMSE %.4f; TV %s after %d iterations, RMSE %.4f; data %.4f"
          % (result["result"], result["iters"], result["path"], ex.rmse(img, clean), result_tv["result"], result_tv["iters"], ex.rmse(img_tv, clean), ex.rmse(f, clean)))
    assert result["result"] == "Converged." and result_tv["result"] == "Converged."
    assert result["path"] == "pdhg:generic", result["path"]
    assert img.shape == (nx * ny,) and np.isfinite(img).all()
    assert ex.rmse(img, clean) < ex.rmse(img_tv, clean) < ex.rmse(f, clean)
