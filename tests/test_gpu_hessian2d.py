"""prost.block.hessian2d on the GPU: the kernels through prost.eval_linop and through the C ABI, the block in the solver and in
examples/hessian_denoise.py.

References: tests/hessian2d_reference.py, never the code under test.
  * restatement: forward and adjoint, both precisions, every variant (components, w), equal the NumPy restatement (b) in T bit for
    bit, plain and accumulating -- [H H] accumulates in the forward product and [H ; H] in the adjoint -- and the same call twice gives
    the same bits; row and column sums within (7 + 8) eps_T of (c), equal for w = 0.5;
  * chain: they equal the existing blocks chained through prost.eval_linop bit for bit, signed zeros included: gradient2d then
    sym_gradient2d forward; sym_gradient2d transposed then gradient2d transposed in the adjoint (components = 4: the mixed plane
    twice, and e_xy + e_yx added in T first).  This pins the new kernels to kernels already pinned to the reference;
  * exact product: against (a) applied in fp64, |got - H x| <= 1.01 k u (|H| |x|) componentwise, the bound derived in
    include/prost/linop/hessian2d.hpp (k = 6 forward, 7 adjoint, 8 with components = 4); the worst observed fraction is printed
    (docs/rounds/r32.md);
  * masks: a NaN reaches exactly the outputs whose row of (a) has an entry in its column, through the vector and the element kernels;
  * offsets: the C entry points at element offsets 0, 1 and 4, plain and accumulating, both directions: bit for bit, and a zero sum
    keeps the -0 of an accumulating adjoint; refusals without a launch;
  * solves: TV^2 at 48 x 40 with L = 1 and L = 3, alg1 with fixed steps, 200 iterations.  D is the distance between the sparse
    twin's own fp32 and fp64 iterates, relative to the largest fp64 iterate; it runs no code of the block.  The block's fp32 iterates
    are held to SOLVE_MULTIPLE = 4 times D from the twin's fp64 iterates: the block rounds at most 6 (7) times on a path where the
    twin's CSR row sums round up to 8 (14) times, so its error per product is bounded by the twin's and propagates through the same
    iteration; what differs is the order of summation, hence WHICH roundings occur, and 4 covers the fluctuation of the maximum of two
    such error sequences.  In fp64 the same limit scaled by the ratio of the unit roundoffs, 4 D 2^-29.  Measured on the MI355X:
    D = 8.83e-8 (L = 1), 1.03e-7 (L = 3); fp32 block at 1.03 D and 0.96 D; fp64 at 0.20 and 0.35 of its limit (docs/rounds/r32.md);
  * the example: both modes run 3000 iterations at 48 x 40 with the block and with the sparse twin (the tolerance of 1e-5 is not reached
    by then), stay finite, agree in RMSE, and come closer to the clean roof than TV on the same data and than the data.  The ordering is
    asserted because the run shows it at this size: RMSE 0.0081 in both modes against 0.0288 for TV and 0.0506 for the data
    (docs/rounds/r32.md).

Shapes (hessian2d_reference.CASES), from the kernel's constants: a workgroup has BLOCK = 256 lanes of VEC = 16 / sizeof(T) rows, so one
strip of the vector path is 1024 rows in fp32 and 512 in fp64 -- the list holds one row below, at and one row above both, and one
vector more (a second strip).  A chunk has 12, 6 or 3 columns, the largest that leaves 2048 workgroups, else 1: at one strip and one
channel nx = 2047 c is one below the choice of c, 2047 c + 1 at it, 2048 c the smallest grid of full chunks of c columns, and one
column more adds a chunk of one column.  Sides of 1, 2 and 3 in every combination make every row a boundary row.
"""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

import hessian2d_reference as R
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


def block(nx, ny, L, w, components, row=0, col=0):
    bf = prost.block.hessian2d(nx, ny, L, w, components)
    m, n = bf(0, 0, 0, 0)[1]
    return bf(row, col, m, n)[0], m, n


def same_bits(a, b):
    """float64 arrays that hold values of T: equal with the signs of the zeros (a NaN is a NaN: its sign and payload are not compared)"""
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True) and np.array_equal(np.signbit(a) & ~np.isnan(a), np.signbit(b) & ~np.isnan(b))


def test_the_shape_list_follows_the_kernel_constants():
    assert R.strip_rows(np.float32) == 1024 and R.strip_rows(np.float64) == 512
    for ny in (511, 512, 513, 514, 1023, 1024, 1025, 1028):
        assert any(c[0] == ny for c in R.CASES)
    for c in (3, 6, 12):
        for dtype in (np.float32, np.float64):
            assert R.pick_columns(2047 * c, 4, 1, dtype) < c and all(R.pick_columns(nx, 4, 1, dtype) == c for nx in (2047 * c + 1, 2048 * c, 2048 * c + 1))
        assert all((4, nx, 1) in R.CASES for nx in (2047 * c, 2047 * c + 1, 2048 * c, 2048 * c + 1))
    assert R.pick_columns(4097, 8, 3, np.float32) == 6 and 4097 % 6 == 5
    assert all((ny, nx, 1) in R.CASES for ny in (1, 2, 3) for nx in (1, 2, 3))
    assert {c[2] for c in R.CASES} == {1, 3}


@pytest.mark.parametrize("prec,dtype", PRECISIONS)
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_products_equal_the_restatement_and_the_chain_bit_for_bit(prec, dtype, case):
    prost.set_precision(prec)
    ny, nx, L = case
    N = nx * ny
    rng = np.random.default_rng(R.case_seed(case))
    tol = (R.SUM_TERMS + 8) * np.finfo(dtype).eps
    grad = prost.block.gradient2d(nx, ny, L)(0, 0, 2 * L * N, L * N)[0]
    for components, w in R.VARIANTS:
        arg = (nx, ny, L, w, components)
        b, m, n = block(*arg)
        sym = prost.block.sym_gradient2d(nx, ny, L, w)(0, 0, 3 * L * N, 2 * L * N)[0]
        rs, cs = R.sums(nx, ny, L, w, components, 1.0, dtype)
        for transpose in (False, True):
            x = rng.standard_normal(m if transpose else n)
            got, rowsum, colsum = run([b], x, transpose)
            want = R.product(x, *arg, transpose, dtype).astype(np.float64)
            assert same_bits(got, want), (components, w, transpose, float(np.abs(got - want).max()))
            assert same_bits(run([b], x, transpose)[0], got)                      # no atomics: the same bits every time
            assert rowsum.shape == rs.shape and colsum.shape == cs.shape
            assert np.all(np.abs(rowsum - rs) <= tol * rs) and np.all(np.abs(colsum - cs) <= tol * cs), (components, w)
            if w == R.W_HALF:
                assert np.array_equal(rowsum, rs) and np.array_equal(colsum, cs)
            # the chain
            if not transpose:
                e = run([sym], run([grad], x, False)[0], False)[0].reshape(3, L * N)
                chained = np.concatenate([e[k] for k in R.planes(components)])
            else:
                e = x.astype(dtype).reshape(components, L * N)
                e3 = e if components == 3 else np.stack([e[0], e[3], e[1] + e[2]])
                chained = run([grad], run([sym], e3.reshape(-1).astype(np.float64), True)[0], True)[0]
            assert same_bits(got, chained), (components, w, transpose, float(np.abs(got - chained).max()))
        # accumulating: the second block adds onto the first
        xn2, xm2 = rng.standard_normal(2 * n), rng.standard_normal(2 * m)
        side = [block(*arg)[0], block(*arg, 0, n)[0]]
        want = R.product(xn2[n:], *arg, False, dtype, res0=R.product(xn2[:n], *arg, False, dtype))
        assert same_bits(run(side, xn2, False)[0], want.astype(np.float64)), (components, w)
        stack = [block(*arg)[0], block(*arg, m, 0)[0]]
        want = R.product(xm2[m:], *arg, True, dtype, res0=R.product(xm2[:m], *arg, True, dtype))
        assert same_bits(run(stack, xm2, True)[0], want.astype(np.float64)), (components, w)


@pytest.mark.parametrize("prec,dtype", PRECISIONS)
def test_against_the_exact_product_within_the_derived_bound(prec, dtype):
    prost.set_precision(prec)
    worst = {}
    for case in R.CASES:
        ny, nx, L = case
        rng = np.random.default_rng(R.case_seed(case, 2))
        for components, w in R.VARIANTS:
            H = R.matrix(nx, ny, L, w, components, dtype)
            m, n = H.shape
            linop = [block(nx, ny, L, w, components)[0]]
            for transpose in (False, True):
                x = rng.standard_normal(m if transpose else n).astype(dtype).astype(np.float64)
                got = run(linop, x, transpose)[0]
                bound = R.bound(nx, ny, L, w, components, transpose, x, dtype)
                err = np.abs(got - (H.T if transpose else H) @ x)
                live = bound > 0
                assert np.all(err <= bound), (case, components, w, transpose, float((err[live] / bound[live]).max()))
                if live.any():
                    worst[(components, transpose)] = max(worst.get((components, transpose), 0.0), float((err[live] / bound[live]).max()))
    print("%s: worst |got - H x| / bound: %s" % (prec, ", ".join("c%d %s %.3f" % (c, "adjoint" if t else "forward", v) for (c, t), v in sorted(worst.items()))))
    assert 0.01 < max(worst.values()) <= 1.0


@pytest.mark.parametrize("prec,dtype", PRECISIONS)
@pytest.mark.parametrize("nx,ny", [(3, 3), (3, 8)])
def test_an_absent_term_is_absent(prec, dtype, nx, ny):
    """ny = 8 takes the vector kernels, ny = 3 and everything behind an odd offset the element kernels"""
    prost.set_precision(prec)
    for components, w in R.VARIANTS:
        b, m, n = block(nx, ny, 1, w, components)
        shifted = [prost.block.diags(1, 1, [2.0], [0])(0, 0, 1, 1)[0], block(nx, ny, 1, w, components, 1, 1)[0]]
        H = abs(R.matrix(nx, ny, 1, w, components))
        for transpose, size in ((False, n), (True, m)):
            M = (H.T if transpose else H).tocsc()
            for at in range(size):
                x = np.random.default_rng(5).standard_normal(size)
                x[at] = np.nan
                reached = np.asarray(M[:, [at]].sum(axis=1)).ravel() > 0
                got = run([b], x, transpose)[0]
                assert np.array_equal(np.isnan(got), reached), (components, transpose, at)
                assert same_bits(got, R.product(x, nx, ny, 1, w, components, transpose, dtype).astype(np.float64))
                assert np.array_equal(np.isnan(run(shifted, np.concatenate([[1.0], x]), transpose)[0][1:]), reached), (components, transpose, at)


def entry(dtype):
    fn = _hip.fn("hessian2d", dtype)
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_double, C.c_int, C.c_int, C.c_int, C.c_void_p]
    fn.restype = C.c_int
    return fn


def call(dtype, x, res0, nx, ny, L, w, components, transpose, accumulate, offset):
    """one launch through the C ABI; res and rhs start `offset` elements into their allocations"""
    pad = np.zeros(offset, dtype)
    keep = [_hip.DeviceArray.from_host(np.concatenate([pad, x.astype(dtype)])), _hip.DeviceArray.from_host(np.concatenate([pad, res0.astype(dtype)]))]
    rhs, res = keep
    try:
        _hip.check(entry(dtype)(res.offset(offset), rhs.offset(offset), nx, ny, L, w, components, int(transpose), int(accumulate), None))
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
        for components, w in R.VARIANTS:
            for transpose in (False, True):
                nres, nrhs = (L * nx * ny, components * L * nx * ny) if transpose else (components * L * nx * ny, L * nx * ny)
                x, res0 = rng.standard_normal(nrhs).astype(dtype), rng.standard_normal(nres).astype(dtype)
                plain = R.product(x, nx, ny, L, w, components, transpose, dtype)
                acc = R.product(x, nx, ny, L, w, components, transpose, dtype, res0)
                for offset in (0, 1, 4):
                    assert same_bits(call(dtype, x, res0, nx, ny, L, w, components, transpose, False, offset), plain), (ny, nx, L, w, transpose, offset)
                    assert same_bits(call(dtype, x, res0, nx, ny, L, w, components, transpose, True, offset), acc), (ny, nx, L, w, transpose, offset)
    # the zeros: a zero sum is +0 plain and keeps the -0 of an accumulating adjoint
    for ny in (3, 8):
        zeros, minus = np.zeros(3 * 3 * ny, dtype), -np.zeros(3 * ny, dtype)
        assert not np.signbit(call(dtype, zeros, minus, 3, ny, 1, R.W_FROB, 3, True, False, 0)).any()
        assert np.signbit(call(dtype, zeros, minus, 3, ny, 1, R.W_FROB, 3, True, True, 0)).all()
        assert not np.signbit(call(dtype, np.zeros(3 * ny, dtype), -zeros, 3, ny, 1, R.W_FROB, 3, False, True, 0)).any()
    # refusals without a launch
    fn, p = entry(dtype), C.c_void_p(16)
    for args in ((p, p, 0, 4, 1, 0.5, 3), (p, p, 4, 0, 1, 0.5, 3), (p, p, 4, 4, 0, 0.5, 3), (p, p, 4, 4, 1, np.inf, 3), (p, p, 4, 4, 1, np.nan, 3),
                 (p, p, 4, 4, 1, 0.0, 3), (p, p, 4, 4, 1, 0.5, 2), (None, p, 4, 4, 1, 0.5, 3), (p, None, 4, 4, 1, 0.5, 4)):
        assert fn(*args, 0, 0, None) != 0 and fn(*args, 1, 1, None) != 0, args
    if dtype == np.float32:
        assert fn(p, p, 4, 4, 1, 1e-60, 3, 0, 0, None) != 0
    _hip.sync()


# ---- the solve ----
SOLVE_ITERS = 200
SOLVE_NX, SOLVE_NY = 48, 40
SOLVE_MULTIPLE = 4


@functools.lru_cache(maxsize=None)
def solve(precision, nc, twin):
    import hessian_denoise as ex
    backend = prost.backend.pdhg(stepsize="alg1", residual_iter=10)
    opts = dict(max_iters=SOLVE_ITERS, num_cback_calls=0, verbose=False, tol_rel_primal=0, tol_rel_dual=0, tol_abs_primal=0, tol_abs_dual=0)
    prost.set_precision(precision)
    _, f = ex.roof_image(SOLVE_NX, SOLVE_NY, nc)
    prob, _, _, u, _, _ = ex.describe(SOLVE_NX, SOLVE_NY, nc, "tv2", f=f, twin=twin)
    r = prost.solve(prob, backend, prost.options(**opts))
    return np.array(u.val, dtype=np.float64).ravel(), r


@pytest.mark.parametrize("nc", [1, 3])
def test_solve_with_the_block_against_the_sparse_twin(nc):
    (b32, r1), (b64, r2), (t32, r3), (t64, r4) = solve("single", nc, False), solve("double", nc, False), solve("single", nc, True), solve("double", nc, True)
    assert all(r["iters"] == SOLVE_ITERS for r in (r1, r2, r3, r4))
    assert r1["path"] == "pdhg:generic" and r2["path"] == "pdhg:generic", (r1["path"], r2["path"])
    assert np.isfinite(b32).all() and np.isfinite(b64).all() and b32.shape == t64.shape == (nc * SOLVE_NX * SOLVE_NY,)
    scale = float(np.abs(t64).max())
    D = float(np.abs(t32 - t64).max()) / scale
    mine32, mine64 = float(np.abs(b32 - t64).max()) / scale, float(np.abs(b64 - t64).max()) / scale
    limit64 = SOLVE_MULTIPLE * D * (np.finfo(np.float64).eps / np.finfo(np.float32).eps)
    print("solve L=%d: D = |twin32 - twin64| / |twin64| = %.3g, |block32 - twin64| / |twin64| = %.3g = %.2f D, |block64 - twin64| / |twin64| = %.3g = %.2f of %.3g"
          % (nc, D, mine32, mine32 / D, mine64, mine64 / limit64, limit64))
    assert D > 0
    assert mine32 <= SOLVE_MULTIPLE * D, (mine32, D)
    assert mine64 <= limit64, (mine64, limit64)


@pytest.mark.parametrize("mode", ["tv2", "nuclear"])
def test_the_example_runs_in_both_modes_and_beats_tv_on_the_roof(mode):
    import hessian_denoise as ex
    prost.set_precision("double")
    nx, ny = 48, 40
    result, img, result_tv, img_tv, f, clean = ex.main(nx, ny, 1, mode, max_iters=3000, verbose=False)
    twin = ex.main(nx, ny, 1, mode, max_iters=3000, verbose=False, twin=True)
    x, y = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    assert np.array_equal(clean, (0.04 * np.minimum(x, nx - 1 - x) + 0.02 * y).reshape(-1))
    assert np.array_equal(f, clean + 0.05 * np.random.default_rng(1).standard_normal(nx * ny))
    print("example %s: %s after %d iterations on %s, RMSE %.4f (sparse twin %.4f); TV %s after %d iterations, RMSE %.4f; data %.4f"
          % (mode, result["result"], result["iters"], result["path"], ex.rmse(img, clean), ex.rmse(twin[1], clean), result_tv["result"], result_tv["iters"],
             ex.rmse(img_tv, clean), ex.rmse(f, clean)))
    assert result["path"] == "pdhg:generic", result["path"]
    assert img.shape == (nx * ny,) and np.isfinite(img).all() and np.isfinite(twin[1]).all()
    assert result_tv["result"] == "Converged."
    assert abs(ex.rmse(img, clean) - ex.rmse(twin[1], clean)) <= 1e-3
    assert ex.rmse(img, clean) < ex.rmse(img_tv, clean) < ex.rmse(f, clean)
