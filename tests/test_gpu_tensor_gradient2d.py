"""prost.block.tensor_gradient2d on the GPU: the kernels through prost.eval_linop and through the C ABI, the block in the solver and in
examples/tv_edge_weighted.py.

References: tests/tensor_gradient2d_reference.py, never the code under test.
  * products: forward and adjoint equal the NumPy restatement (b) in T bit for bit for k = 1, 2, 3, the same call twice gives the same
    bits; row and column sums equal to (c) for the dyadic tensors and within (t + 8) eps_T otherwise, t = 6; both precisions;
  * g = 1: the bits of prost.block.gradient2d on the GPU, forward and adjoint;
  * composition: [K K] and [K ; K] accumulate in the forward and in the adjoint product (the restatement adds res + value), a 1 x 1
    diags block in front gives the block odd element offsets and so the element kernels: bit for bit;
  * against the oracle's block.sparse on matrix (a): |got - twin| <= (gamma_block + gamma_twin) B componentwise, B from the unmerged
    absolute values, the roundings counted in the header (derived, not measured); the worst ratio is printed;
  * absent terms: through the C entry points (the front end refuses non-finite tensors) Inf in the last row and the last column of
    every plane reaches only the outputs whose masks keep those terms -- the list for 3 x 3 is asserted, from matrix (a) -- on the
    element and on the vector path; Inf in the only element of a 1 x 1 grid (the one empty column there is) reaches nothing; a NaN in u
    reaches exactly the outputs of its column of (a), also behind odd offsets;
  * the C entry points at element offsets 0, 1 and 4 of res, rhs and the tensor, and at offset 1 of the tensor alone, plain and
    accumulating, both directions: bit for bit, padding untouched, rhs and tensor unchanged; refusals without a launch;
  * weighted ROF at 24 x 16 with L = 1 and L = 3, alg1 with fixed steps, 200 iterations: the block on the GPU (i), the sparse twin on
    the GPU (ii) and in the oracle (iii), for a scalar g of powers of two and for the example's tensors in both modes.  (i) is NOT
    expected to equal (ii) bit for bit, not even for g a power of two: the forward products coincide then (scaling by a power of two
    commutes with rounding), but the adjoint is defined as grad_adj_kernel forms it, (qx[p] - qx[p-ny]) + (qy[p] - qy[p-1]), while a
    CSR row of K^T adds its four products one by one in ascending column order.  So the general criterion holds for every tensor: with
    D = |(ii) - (iii)| / |(iii)|, which runs no code of the block, |(i) - (iii)| / |(iii)| <= max(10 D, 10 * 200 * t * u), t = 4 the
    longest chain of roundings of a product (figures: docs/rounds/r29.md);
  * the example converges in both modes on pdhg:generic; in the scalar mode RMSE(weighted) < RMSE(TV) < RMSE(noisy), confirmed with the
    oracle through the twin for this seed and size (0.0322 < 0.0466 < 0.0921).  In the tensor mode only RMSE(weighted) < RMSE(noisy) is
    asserted: against TV the ordering holds at 24 x 16 (0.0428) but not at 48 x 32 (0.0350 against 0.0319), so it is no property of
    the method at these sizes.

Shapes (tensor_gradient2d_reference.CASES), from the kernel's constants: a workgroup has BLOCK = 256 lanes of VEC = 16 / sizeof(T) rows,
so one strip of the vector path is 1024 rows in fp32 and 512 in fp64 -- the list holds both, each with one row more (the element
kernels) and one vector more (a second strip); a wave is 64 lanes, so 64 VEC and 64 VEC + VEC rows put a wave edge, where the adjoint
recomputes the row neighbour's flux from memory, inside a strip.  A chunk has kColumnChoices = 12, 6 or 3 columns, the largest that
leaves kFillBlocks = 2048 workgroups, else 1: the small shapes run one column per chunk (every chunk but the first computes its halo
flux); nx = 2048 c at 4 rows and one channel is the smallest grid of full chunks of c columns, nx = 2048 c + 1 adds a chunk of one.
"""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

import oracle
import prost_amd as prost
import tensor_gradient2d_reference as R
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


def block(nx, ny, L, planes, row=0, col=0):
    bf = prost.block.tensor_gradient2d(nx, ny, L, planes)
    m, n = bf(0, 0, 0, 0)[1]
    return bf(row, col, m, n)[0], m, n


def test_the_shape_list_follows_the_kernel_constants():
    assert R.BLOCK == 256 and R.WAVE == 64 and R.strip_rows(np.float32) == 1024 and R.strip_rows(np.float64) == 512
    for dtype in (np.float32, np.float64):
        v, s = R.VEC[np.dtype(dtype)], R.strip_rows(dtype)
        assert v * np.dtype(dtype).itemsize == 16
        for ny in (s, s + 1, s + v, R.WAVE * v, R.WAVE * v + v):
            assert any(c[0] == ny for c in R.CASES), ny
    for ny, nx in ((1, 1), (3, 3)):
        assert any(c[:2] == (ny, nx) for c in R.CASES)
    assert any(c[0] == 1 and c[1] > 1 for c in R.CASES) and any(c[1] == 1 and c[0] > 1 for c in R.CASES)
    for c in R.COLUMN_CHOICES:
        for dtype in (np.float32, np.float64):
            assert R.pick_columns(2048 * c, 4, 1, dtype) == c and R.pick_columns(2048 * c + 1, 4, 1, dtype) == c and R.pick_columns(2048 * c - c, 4, 1, dtype) < c
        assert (4, 2048 * c, 1) in R.CASES and (4, 2048 * c + 1, 1) in R.CASES
    assert R.pick_columns(4097, 8, 3, np.float32) == 6 and 4097 % 6 == 5
    assert {c[2] for c in R.CASES} == {1, 3}


@pytest.mark.parametrize("prec,dtype", PRECISIONS)
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_products_bit_for_bit_and_sums(prec, dtype, case):
    prost.set_precision(prec)
    ny, nx, L = case
    rng = np.random.default_rng(R.case_seed(case))
    tol = (R.T_TERMS + 8) * np.finfo(dtype).eps
    for k in R.MODES:
        planes = R.tensor_for(case, k)
        b, nrows, ncols = block(nx, ny, L, planes)
        rs, cs = R.sums(nx, ny, L, planes, 1.0, dtype)
        for transpose in (False, True):
            x = rng.standard_normal(nrows if transpose else ncols)
            got, rowsum, colsum = run([b], x, transpose)
            want = R.product(x, nx, ny, L, planes, transpose, dtype).astype(np.float64)
            assert got.shape == want.shape and np.array_equal(got, want), (k, transpose, float(np.abs(got - want).max()))
            assert np.array_equal(run([b], x, transpose)[0], got)                 # no atomics: the same bits every time
            assert rowsum.shape == rs.shape and colsum.shape == cs.shape
            assert np.all(np.abs(rowsum - rs) <= tol * rs) and np.all(np.abs(colsum - cs) <= tol * cs), k
            if R.is_dyadic(case):
                assert np.array_equal(rowsum, rs) and np.array_equal(colsum, cs)


@pytest.mark.parametrize("prec,dtype", PRECISIONS)
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_g_equal_to_one_is_gradient2d_bit_for_bit(prec, dtype, case):
    prost.set_precision(prec)
    ny, nx, L = case
    rng = np.random.default_rng(R.case_seed(case, 6))
    b, m, n = block(nx, ny, L, R.ones_tensor(nx, ny))
    g = prost.block.gradient2d(nx, ny, L)(0, 0, m, n)[0]
    for transpose in (False, True):
        x = rng.standard_normal(m if transpose else n)
        x[::5] = -0.0
        got, want = run([b], x, transpose)[0], run([g], x, transpose)[0]
        assert np.array_equal(got, want) and np.array_equal(np.signbit(got), np.signbit(want)), transpose


@pytest.mark.parametrize("prec,dtype", PRECISIONS)
@pytest.mark.parametrize("case", R.SMALL + R.WAVES + R.STRIPS + R.CHUNKS[1:2] + R.CHUNKS[-1:], ids=R.case_id)
def test_composition_bit_for_bit(prec, dtype, case):
    """[K K]: the second block adds onto the first in the forward product; [K ; K]: in the adjoint; diag(d, K) with a 1 x 1 diags block
    d in front: K's rows and columns start at element 1, the pointers are aligned for one element only"""
    prost.set_precision(prec)
    ny, nx, L = case
    rng = np.random.default_rng(R.case_seed(case, 1))
    for k in R.MODES:
        arg = (nx, ny, L, R.random_tensor(nx, ny, k, R.case_seed(case, 80 + k)))
        _, m, n = block(*arg)
        xn2, xn, xm2, xm = rng.standard_normal(2 * n), rng.standard_normal(n), rng.standard_normal(2 * m), rng.standard_normal(m)
        side = [block(*arg)[0], block(*arg, 0, n)[0]]
        want = R.product(xn2[n:], *arg, False, dtype, res0=R.product(xn2[:n], *arg, False, dtype))
        assert np.array_equal(run(side, xn2, False)[0], want.astype(np.float64)), k
        assert np.array_equal(run(side, xm, True)[0], np.tile(R.product(xm, *arg, True, dtype), 2).astype(np.float64)), k
        stack = [block(*arg)[0], block(*arg, m, 0)[0]]
        assert np.array_equal(run(stack, xn, False)[0], np.tile(R.product(xn, *arg, False, dtype), 2).astype(np.float64)), k
        want = R.product(xm2[m:], *arg, True, dtype, res0=R.product(xm2[:m], *arg, True, dtype))
        assert np.array_equal(run(stack, xm2, True)[0], want.astype(np.float64)), k
        shifted = [prost.block.diags(1, 1, [2.0], [0])(0, 0, 1, 1)[0], block(*arg, 1, 1)[0]]
        for transpose in (False, True):
            xs = rng.standard_normal((m if transpose else n) + 1)
            got = run(shifted, xs, transpose)[0]
            want = np.concatenate([(np.zeros(1, dtype) + dtype(2.0) * xs[:1].astype(dtype)), R.product(xs[1:], *arg, transpose, dtype)])
            assert np.array_equal(got, want.astype(np.float64)), (k, transpose)
            assert np.array_equal(run(shifted, xs, transpose)[0], got)


@pytest.mark.parametrize("prec,dtype", PRECISIONS)
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_against_the_sparse_twin_in_the_oracle(prec, dtype, case):
    prost.set_precision(prec)
    ny, nx, L = case
    rng = np.random.default_rng(R.case_seed(case, 2))
    for k in R.MODES:
        planes = R.rounded(R.random_tensor(nx, ny, k, R.case_seed(case, 90 + k)), dtype)
        K = R.matrix(nx, ny, L, planes, dtype)
        m, n = K.shape
        linop = [block(nx, ny, L, planes)[0]]
        if K.nnz == 0:                                    # 1 x 1: the matrix is empty and so is the product
            for transpose in (False, True):
                assert not run(linop, rng.standard_normal(m if transpose else n), transpose)[0].any()
            continue
        twin = [prost.block.sparse(K)(0, 0, m, n)[0]]
        for transpose in (False, True):
            x = rng.standard_normal(m if transpose else n).astype(dtype).astype(np.float64)
            got = run(linop, x, transpose)[0]
            want = np.asarray(oracle.eval_linop(twin, x, transpose, dtype)[0], dtype=np.float64).ravel()
            bound = R.bound(nx, ny, L, planes, transpose, x, dtype, twin=True)
            err = np.abs(got - want)
            live = bound > 0
            print("%s %s k=%d transpose=%d: |got - twin| / bound %.3f" % (prec, R.case_id(case), k, transpose, float((err[live] / bound[live]).max()) if live.any() else 0.0))
            assert np.all(err <= bound), float((err[live] / bound[live]).max())


def entry(dtype):
    fn = _hip.fn("linop_tensor_gradient2d", dtype)
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_void_p]
    fn.restype = C.c_int
    return fn


def call(dtype, x, res0, planes, nx, ny, L, transpose, accumulate, offset, tensor_offset=None):
    """one launch through the C ABI; res and rhs start `offset` elements into their allocations, the tensor `tensor_offset` (None: the
    same).  The planes go to the device as they are, non-finite values included."""
    tensor_offset = offset if tensor_offset is None else tensor_offset
    pad, tpad = np.zeros(offset, dtype), np.zeros(tensor_offset, dtype)
    t = np.concatenate(planes).astype(dtype)
    keep = [_hip.DeviceArray.from_host(np.concatenate([pad, x.astype(dtype)])), _hip.DeviceArray.from_host(np.concatenate([pad, res0.astype(dtype)])),
            _hip.DeviceArray.from_host(np.concatenate([tpad, t]))]
    rhs, res, ten = keep
    try:
        _hip.check(entry(dtype)(res.offset(offset), rhs.offset(offset), ten.offset(tensor_offset), nx, ny, L, len(planes), int(transpose), int(accumulate), None))
        _hip.sync()
        out = res.to_host()
        assert out.size == offset + res0.size and np.array_equal(out[:offset], pad)
        assert np.array_equal(rhs.to_host()[offset:], x.astype(dtype), equal_nan=True)
        assert np.array_equal(ten.to_host()[tensor_offset:], t, equal_nan=True)
        return out[offset:]
    finally:
        for d in keep:
            d.free()


def poisoned(nx, ny, k):
    """a finite tensor with Inf in the last row and the last column of every plane"""
    planes = [p.reshape(nx, ny).copy() for p in R.random_tensor(nx, ny, k, 40 + k)]
    for p in planes:
        p[-1, :] = np.inf
        p[:, -1] = np.inf
    return [p.reshape(-1) for p in planes]


def reached(nx, ny, planes, transpose):
    """the outputs that a non-finite entry of (a) reaches"""
    K = R.matrix(nx, ny, 1, planes)
    bad = K.copy()
    bad.data = (~np.isfinite(K.data)).astype(np.float64)
    return np.asarray(bad.sum(axis=0 if transpose else 1)).ravel() > 0


@pytest.mark.parametrize("prec,dtype", PRECISIONS)
def test_absent_terms_are_absent(prec, dtype):
    prost.set_precision(prec)
    # Inf in the last row and column of the tensor, through the C entry points; p = y + 3 x, the poisoned pixels are 2, 5, 6, 7, 8
    want = {(1, False): [2, 5, 9 + 6, 9 + 7], (2, False): [2, 5, 9 + 6, 9 + 7], (3, False): [2, 5, 6, 7, 9 + 2, 9 + 5, 9 + 6, 9 + 7],
            (1, True): [2, 5, 6, 7, 8], (2, True): [2, 5, 6, 7, 8], (3, True): [2, 5, 6, 7, 8]}
    for ny, nx in ((3, 3), (8, 5)):                      # the element kernels; the vector kernels (offsets 0 and 4) and the element kernels (1)
        N = nx * ny
        x, y = np.random.default_rng(5).standard_normal(N), np.random.default_rng(6).standard_normal(2 * N)
        for k in R.MODES:
            planes = poisoned(nx, ny, k)
            for transpose, v in ((False, x), (True, y)):
                hit = reached(nx, ny, planes, transpose)
                if (ny, nx) == (3, 3):
                    assert np.flatnonzero(hit).tolist() == want[(k, transpose)]
                ref = R.product(v, nx, ny, 1, planes, transpose, dtype)
                assert np.array_equal(~np.isfinite(ref), hit)
                for offset in (0, 1, 4):
                    got = call(dtype, v, np.zeros(N if transpose else 2 * N), planes, nx, ny, 1, transpose, False, offset)
                    assert np.array_equal(~np.isfinite(got), hit), (ny, nx, k, transpose, offset)
                    assert np.array_equal(got, ref, equal_nan=True), (ny, nx, k, transpose, offset)
    nx = ny = 3
    for k in R.MODES:
        # the only empty column there is: the single element of a 1 x 1 grid
        b1, _, _ = block(1, 1, 1, R.random_tensor(1, 1, k, 1))
        assert not run([b1], np.array([np.inf]), False)[0].any()
        # a NaN in u reaches exactly the outputs of its column of (a)
        planes = R.random_tensor(nx, ny, k, 50 + k)
        b, m, n = block(nx, ny, 1, planes)
        x = np.random.default_rng(5).standard_normal(n)
        x[4] = np.nan
        K = R.matrix(nx, ny, 1, planes)
        hit = np.asarray(abs(K)[:, [4]].sum(axis=1)).ravel() > 0
        got = run([b], x, False)[0]
        want_x = R.product(x, nx, ny, 1, planes, False, dtype).astype(np.float64)
        assert np.array_equal(np.isnan(got), hit) and np.array_equal(got, want_x, equal_nan=True)
        # the same behind odd offsets (the element kernels)
        shifted = [prost.block.diags(1, 1, [2.0], [0])(0, 0, 1, 1)[0], block(nx, ny, 1, planes, 1, 1)[0]]
        assert np.array_equal(run(shifted, np.concatenate([[1.0], x]), False)[0][1:], want_x, equal_nan=True)


@pytest.mark.parametrize("prec,dtype", PRECISIONS)
def test_c_abi_offset_pointers_plain_and_accumulating(prec, dtype):
    """offset 0 / 4: 16-byte aligned (the vector kernels where the height allows); 1: aligned for one element only; the tensor alone
    at offset 1 must take the element kernels too"""
    rng = np.random.default_rng(12)
    for ny, nx, L in ((3, 3, 2), (8, 5, 2), (17, 13, 3), (260, 2, 3), (1028, 2, 1)):
        for k in R.MODES:
            planes = R.random_tensor(nx, ny, k, 7 * k + ny)
            for transpose in (False, True):
                nres, nrhs = (L * nx * ny, 2 * L * nx * ny) if transpose else (2 * L * nx * ny, L * nx * ny)
                x, res0 = rng.standard_normal(nrhs).astype(dtype), rng.standard_normal(nres).astype(dtype)
                plain = R.product(x, nx, ny, L, planes, transpose, dtype)
                for offset, tensor_offset in ((0, None), (1, None), (4, None), (0, 1), (4, 1), (1, 0)):
                    where = (ny, nx, L, k, transpose, offset, tensor_offset)
                    assert np.array_equal(call(dtype, x, res0, planes, nx, ny, L, transpose, False, offset, tensor_offset), plain), where
                    assert np.array_equal(call(dtype, x, res0, planes, nx, ny, L, transpose, True, offset, tensor_offset), res0 + plain), where
    # refusals without a launch
    fn, p = entry(dtype), C.c_void_p(16)
    for args in ((p, p, p, 0, 4, 1, 1), (p, p, p, 4, 0, 1, 1), (p, p, p, 4, 4, 0, 1), (p, p, p, 4, 4, 1, 0), (p, p, p, 4, 4, 1, 4), (p, p, p, 4, 4, 1, -1),
                 (None, p, p, 4, 4, 1, 1), (p, None, p, 4, 4, 1, 1), (p, p, None, 4, 4, 1, 1), (p, p, p, 2 ** 26, 2 ** 26, 2, 1)):
        assert fn(*args, 0, 0, None) != 0 and fn(*args, 1, 1, None) != 0, args
    _hip.sync()


# ---- the solve ----
SOLVE_ITERS = 200
SOLVE_NX, SOLVE_NY = 24, 16
SOLVE_T = 4                           # the longest chain of roundings of a product (the adjoint at k = 3)
TENSORS = ["power_of_two", "scalar", "tensor"]


def solve_tensor(kind, f, nc):
    import tv_edge_weighted as ex
    if kind == "power_of_two":
        return [2.0 ** -np.random.default_rng(3).integers(0, 3, SOLVE_NX * SOLVE_NY).astype(np.float64)]
    return ex.edge_tensor(f, SOLVE_NX, SOLVE_NY, nc, kind)


@functools.lru_cache(maxsize=None)
def solve_three_ways(precision, nc, kind):
    import tv_edge_weighted as ex
    dtype = dict(PRECISIONS)[precision]
    backend = prost.backend.pdhg(stepsize="alg1", residual_iter=10)
    opts = dict(max_iters=SOLVE_ITERS, num_cback_calls=0, verbose=False, tol_rel_primal=0, tol_rel_dual=0, tol_abs_primal=0, tol_abs_dual=0)
    prost.set_precision(precision)
    _, f = ex.step_image(SOLVE_NX, SOLVE_NY, nc)
    planes = solve_tensor(kind, f, nc)
    out = {}
    for key, twin, solver in (("i", False, None), ("ii", True, None), ("iii", True, oracle)):
        prob, _, _, u, _, _, _ = ex.describe(SOLVE_NX, SOLVE_NY, nc, "scalar" if len(planes) == 1 else "tensor", f=f, twin=twin, planes=planes)
        r = prost.solve(prob, backend, prost.options(**opts)) if solver is None else oracle.solve(prob, backend, prost.options(**opts), dtype)
        out[key] = (np.array(u.val, dtype=np.float64).ravel(), r)
    return out


@pytest.mark.parametrize("precision,dtype", PRECISIONS)
@pytest.mark.parametrize("nc", [1, 3])
@pytest.mark.parametrize("kind", TENSORS)
def test_solve_with_the_block_against_the_sparse_twin(precision, dtype, nc, kind):
    out = solve_three_ways(precision, nc, kind)
    (x1, r1), (x2, r2), (x3, r3) = out["i"], out["ii"], out["iii"]
    assert r1["iters"] == SOLVE_ITERS and r2["iters"] == SOLVE_ITERS and r3["iters"] == SOLVE_ITERS
    assert r1["path"] == "pdhg:generic", r1["path"]
    assert np.isfinite(x1).all() and x1.shape == x3.shape == (nc * SOLVE_NX * SOLVE_NY,)
    scale = float(np.abs(x3).max())
    D = float(np.abs(x2 - x3).max()) / scale
    mine = float(np.abs(x1 - x3).max()) / scale
    print("solve %s L=%d %s: D = |(ii) - (iii)| / |(iii)| = %.3g, |(i) - (iii)| / |(iii)| = %.3g, |(i) - (ii)| / |(iii)| = %.3g"
          % (precision, nc, kind, D, mine, float(np.abs(x1 - x2).max()) / scale))
    # ten times first-order growth of a preconditioner difference of a few ulps over the iterations, or ten times one forward error t u
    # of a product per iteration, whichever is larger
    limit = max(10 * D, 10 * SOLVE_ITERS * SOLVE_T * (np.finfo(dtype).eps / 2))
    assert mine <= limit, (mine, limit)


@pytest.mark.parametrize("mode", ["scalar", "tensor"])
def test_the_example_converges_and_beats_the_noisy_data(mode):
    import tv_edge_weighted as ex
    prost.set_precision("double")
    nx, ny = 24, 16
    result, img, result_tv, img_tv, f, clean = ex.main(nx, ny, 1, mode, max_iters=20000, verbose=False)
    assert np.array_equal(f, clean + 0.1 * np.random.default_rng(1).standard_normal(nx * ny)) and np.unique(clean).size == 3
    print("example %s: weighted TV %s after %d iterations on %s, RMSE %.4f; TV %s after %d iterations, RMSE %.4f; data %.4f"
          % (mode, result["result"], result["iters"], result["path"], ex.rmse(img, clean), result_tv["result"], result_tv["iters"], ex.rmse(img_tv, clean), ex.rmse(f, clean)))
    assert result["result"] == "Converged." and result_tv["result"] == "Converged."
    assert result["path"] == "pdhg:generic", result["path"]
    assert img.shape == (nx * ny,) and np.isfinite(img).all()
    assert ex.rmse(img, clean) < ex.rmse(f, clean) and ex.rmse(img_tv, clean) < ex.rmse(f, clean)
    if mode == "scalar":
        assert ex.rmse(img, clean) < ex.rmse(img_tv, clean)
