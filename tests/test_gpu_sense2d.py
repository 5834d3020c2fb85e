"""prost.block.sense2d on the GPU: the kernels through prost.eval_linop and through the C ABI, the block in the solver and in
examples/sense_mri.py.

References: tests/sense2d_reference.py, never the code under test.  u is the unit roundoff of T; Bf and Bt are the bounds (e) of the
reference, derived in include/prost/linop/sense2d.hpp: per coil image |fl(K x) - K x|_2 <= Bf |sigma_c . x_l|_2, per image
|fl(K^T y) - K^T y|_2 <= Bt sum_c max|sigma_c| |y_{l,c}|_2.
  * products: forward and transposed equal the NumPy restatement (a) in T bit for bit (-0 and +0 compare equal), the same call twice gives
    the same bits; row and column sums through prost.eval_linop within (C + 8) eps_T of the bound sums (d); against the float64 operator
    (c) within Bf / Bt in fp32 and twice that in fp64 (the comparator is then itself float64 arithmetic), and against the explicit
    matrix (b) where N <= 64; the ratio is printed;
  * the chain: forward equal, bit for bit, to prost.block.fft2d(nx, ny, L C) on planes premultiplied in NumPy in T; transposed equal to
    the NumPy coil sum of that block's transposed product; C = 1 with sigma = 1 equals fft2d(nx, ny, L) under == in both directions;
  * composition: [K K] and [K ; K] accumulate in the forward and in the transposed product, a 1 x 1 diags block in front gives the block
    odd row and column offsets (narrow accesses): bit for bit;
  * the C entry points at element offsets 0, 1 and 4, plain and accumulating, with the reference's table: bit for bit; rhs is left alone;
  * the geometry record's tile selector of the coil-summing pass (0 the library's choice, 1 the small tile, 2 fft2d's choice) changes no
    bit at nx = 64, 256, 512 and 2048, and any other value is refused;
  * a NaN in image l reaches every coil image of l and leaves the others bit-identical; a NaN in coil image (l, c) reaches image l of the
    transpose only;
  * against prost.block.dense of matrix (b) on the GPU at (8, 4, 1, 3) and (16, 16, 1, 2): within the block's bound plus the twin's own,
    gamma_{n+4} (sqrt(2) s |sigma|) |x| per dot product of n terms (n - 1 additions, one product, the rounding of the entry to T and the three
    roundings that form it from cos, sin and the map, relative to sqrt(2) s |sigma| >= |cos| |s.re| + |sin| |s.im|); doubled in fp64;
  * the solve at 16 x 16, C = 4, half of the lines, alg1 with fixed steps, 200 iterations, tolerances 0, identity scaling -- the block
    returns BOUNDS for its sums where the twin enumerates them, so the default preconditioners of the two problems differ by design and
    only the identity puts both on the same steps.  D = |twin32 - twin64| / |twin64|_max runs no code of the block.  The fp32 block is held
    to 4 D of the fp64 twin (the multiple the sister tests fixed in advance: the block rounds fewer times per product than the twin's dot
    products of 512 terms, 4 covers the fluctuation of the maximum of two such error sequences); the fp64 block to the limit of
    test_solve_with_the_block_against_the_dense_twin (test_gpu_fft2d.py), 10 * 200 * c u with c u = Bt, the block's own bound.  Measured on
    the MI355X: D = 1.43e-7, the fp32 block at 0.62 D, the fp64 block at 3.3e-16 (docs/rounds/r33.md);
  * examples/sense_mri.py at 32 x 32 in fp64, 8 coils, a quarter of the lines: the RMSE of the reconstruction is below that of the
    coil-combined zero-filled image (measured: 0.0246 against 0.1139), and block and twin=True agree to the
    solve test's limit with the example's iteration count.
"""
import ctypes as C
import functools
import math
import os
import sys

import numpy as np
import pytest

import fft2d_reference as F
import sense2d_reference as R
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


def block(case, maps):
    nx, ny, L, Cn = case
    bf = prost.block.sense2d(nx, ny, maps, L)
    rows, cols = bf(0, 0, 0, 0)[1]
    assert (rows, cols) == R.sizes(case)
    return bf, rows, cols


def errors(got, x, case, maps, transpose, dtype):
    """-> the per-image error against the float64 operator over the scale of the bound, [L C] forward and [L] transposed"""
    nx, ny, L, Cn = case
    N = nx * ny
    err = R.image_norms(got - R.exact(x, case, maps, transpose, dtype), L if transpose else L * Cn, N)
    scale = R.transposed_scales(x, case, maps, dtype) if transpose else R.forward_scales(x, case, maps, dtype)
    return err, scale


@pytest.mark.parametrize("prec,dtype", PRECISIONS)
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_products_bit_for_bit_repeatable_within_the_bound_and_sums(prec, dtype, case):
    prost.set_precision(prec)
    nx, ny, L, Cn = case
    N = nx * ny
    rng = np.random.default_rng(R.case_seed(case))
    maps = R.make_maps(case, zeros=True)
    bf, rows, cols = block(case, maps)
    linop = [bf(0, 0, rows, cols)[0]]
    want_rows, want_cols = R.bound_sums(case, maps, dtype, 1.0)
    eps = np.finfo(dtype).eps
    factor = 2 if dtype == np.float64 else 1
    K = R.matrix(case, maps, dtype) if N <= 64 and rows * cols <= 2 ** 22 else None
    for transpose, B in zip((False, True), R.bounds(case, dtype)):
        x = rng.standard_normal(rows if transpose else cols).astype(dtype).astype(np.float64)
        got, rowsum, colsum = run(linop, x, transpose)
        want = R.product(x, case, maps, transpose, dtype).astype(np.float64)
        assert got.shape == want.shape and np.array_equal(got, want), (transpose, float(np.abs(got - want).max()), int((got != want).sum()))
        assert np.array_equal(run(linop, x, transpose)[0], got)                 # no atomics: the same bits every time
        err, scale = errors(got, x, case, maps, transpose, dtype)
        worst = float((err / np.maximum(scale, 1e-300)).max()) / (factor * B)
        if K is not None:
            errm = R.image_norms(got - (K.T @ x if transpose else K @ x), L if transpose else L * Cn, N)
            worst = max(worst, float((errm / np.maximum(scale, 1e-300)).max()) / (factor * B))
            assert np.all(errm <= factor * B * scale)
        print("%s %s transpose=%d: |got - float64 operator| / (bound scale) = %.3f" % (prec, R.case_id(case), transpose, worst))
        assert np.all(err <= factor * B * scale), worst
        assert rowsum.shape == want_rows.shape and np.all(np.abs(rowsum - want_rows) <= (Cn + 8) * eps * want_rows)
        assert colsum.shape == want_cols.shape and np.all(np.abs(colsum - want_cols) <= (Cn + 8) * eps * want_cols)


@pytest.mark.parametrize("prec,dtype", PRECISIONS)
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_the_chain_on_the_gpu_bit_for_bit(prec, dtype, case):
    """forward: fft2d(nx, ny, L C) on the planes premultiplied in NumPy in T; transposed: the NumPy coil sum of that block's transposed product"""
    prost.set_precision(prec)
    nx, ny, L, Cn = case
    N = nx * ny
    rng = np.random.default_rng(R.case_seed(case, 5))
    maps = R.make_maps(case)
    bf, rows, cols = block(case, maps)
    linop = [bf(0, 0, rows, cols)[0]]
    chain = [prost.block.fft2d(nx, ny, L * Cn)(0, 0, rows, rows)[0]]
    s = R.rounded(maps, dtype)
    x = rng.standard_normal(cols).astype(dtype)
    u = x.reshape(2, L, 1, N)
    z = np.stack([u[0] * s[0] - u[1] * s[1], u[0] * s[1] + u[1] * s[0]])
    assert z.dtype == dtype
    assert np.array_equal(run(linop, x.astype(np.float64), False)[0], run(chain, z.reshape(-1).astype(np.float64), False)[0])
    y = rng.standard_normal(rows).astype(dtype)
    w = run(chain, y.astype(np.float64), True)[0].astype(dtype).reshape(2, L, Cn, N)
    tr, ti = w[0] * s[0] + w[1] * s[1], w[1] * s[0] - w[0] * s[1]
    accr, acci = tr[:, 0].copy(), ti[:, 0].copy()
    for c in range(1, Cn):
        accr, acci = accr + tr[:, c], acci + ti[:, c]
    assert accr.dtype == dtype
    assert np.array_equal(run(linop, y.astype(np.float64), True)[0], np.stack([accr, acci]).reshape(-1).astype(np.float64))


@pytest.mark.parametrize("prec,dtype", PRECISIONS)
@pytest.mark.parametrize("shape", [(1, 1, 3), (8, 4, 2), (64, 32, 1), (256, 64, 1)], ids=lambda s: "%dx%dx%d" % s)
def test_one_coil_of_ones_is_fft2d(prec, dtype, shape):
    """== in both directions: every finite value is fft2d's; the signs of zeros may differ (sense2d.hpp)"""
    prost.set_precision(prec)
    nx, ny, L = shape
    n = 2 * L * nx * ny
    linop = [prost.block.sense2d(nx, ny, np.ones((1, nx * ny), complex), L)(0, 0, n, n)[0]]
    plain = [prost.block.fft2d(nx, ny, L)(0, 0, n, n)[0]]
    x = np.random.default_rng(nx + ny).standard_normal(n).astype(dtype).astype(np.float64)
    x[::7] = 0.0
    for transpose in (False, True):
        got, want = run(linop, x, transpose)[0], run(plain, x, transpose)[0]
        assert np.all(got == want), transpose


@pytest.mark.parametrize("prec,dtype", PRECISIONS)
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_composition_bit_for_bit(prec, dtype, case):
    """[K K]: the second block adds onto the first in the forward product; [K ; K]: in the transposed one; diag(d, K) with a 1 x 1 diags
    block d in front: K's rows and columns start at element 1"""
    prost.set_precision(prec)
    rng = np.random.default_rng(R.case_seed(case, 1))
    maps = R.make_maps(case)
    bf, rows, cols = block(case, maps)
    P = lambda v, transpose, res0=None: R.product(v, case, maps, transpose, dtype, res0=res0)
    side = [bf(0, 0, rows, cols)[0], bf(0, cols, rows, cols)[0]]
    x2, y1 = rng.standard_normal(2 * cols), rng.standard_normal(rows)
    assert np.array_equal(run(side, x2, False)[0], P(x2[cols:], False, res0=P(x2[:cols], False)).astype(np.float64))
    assert np.array_equal(run(side, y1, True)[0], np.tile(P(y1, True), 2).astype(np.float64))
    stack = [bf(0, 0, rows, cols)[0], bf(rows, 0, rows, cols)[0]]
    x1, y2 = rng.standard_normal(cols), rng.standard_normal(2 * rows)
    assert np.array_equal(run(stack, x1, False)[0], np.tile(P(x1, False), 2).astype(np.float64))
    assert np.array_equal(run(stack, y2, True)[0], P(y2[rows:], True, res0=P(y2[:rows], True)).astype(np.float64))
    shifted = [prost.block.diags(1, 1, [2.0], [0])(0, 0, 1, 1)[0], bf(1, 1, rows, cols)[0]]
    for transpose in (False, True):
        xs = rng.standard_normal((rows if transpose else cols) + 1)
        got = run(shifted, xs, transpose)[0]
        want = np.concatenate([(np.zeros(1, dtype) + dtype(2.0) * xs[:1].astype(dtype)), P(xs[1:], transpose)])
        assert np.array_equal(got, want.astype(np.float64)), transpose
        assert np.array_equal(run(shifted, xs, transpose)[0], got)


def entry(dtype):
    fn = _hip.fn("sense2d", dtype)
    fn.argtypes = [C.c_void_p] * 6 + [C.c_int, C.c_void_p]
    fn.restype = C.c_int
    return fn


def call(dtype, x, res0, nwork, geometry, table, maps, accumulate, offset):
    """one launch through the C ABI; res, rhs, work and maps start `offset` elements into their allocations"""
    pad = np.zeros(offset, dtype)
    keep = [_hip.DeviceArray.from_host(np.concatenate([pad, x.astype(dtype)])), _hip.DeviceArray.from_host(np.concatenate([pad, res0.astype(dtype)])),
            _hip.DeviceArray.from_host(np.concatenate([pad, np.zeros(nwork, dtype)])), _hip.DeviceArray.from_host(np.concatenate([pad, maps.reshape(-1).astype(dtype)])),
            _hip.DeviceArray.from_host(np.ascontiguousarray(table).reshape(-1))]
    rhs, res, work, dmaps, tab = keep
    try:
        _hip.check(entry(dtype)(geometry.ctypes.data_as(C.c_void_p), tab.ptr, dmaps.offset(offset), work.offset(offset), res.offset(offset), rhs.offset(offset),
                                int(accumulate), None))
        _hip.sync()
        out = res.to_host()
        assert out.size == offset + res0.size and np.array_equal(out[:offset], pad) and np.array_equal(work.to_host()[:offset], pad)
        assert np.array_equal(rhs.to_host()[offset:], x.astype(dtype)) and np.array_equal(dmaps.to_host()[offset:], maps.reshape(-1).astype(dtype))
        return out[offset:]
    finally:
        for d in keep:
            d.free()


@pytest.mark.parametrize("prec,dtype", PRECISIONS)
def test_c_abi_offset_pointers_plain_and_accumulating(prec, dtype):
    """offset 0 / 4: 16-byte aligned; 1: aligned for one element only.  The table is the reference's, made from the definition."""
    rng = np.random.default_rng(12)
    case = nx, ny, L, Cn = (8, 4, 2, 3)
    rows, cols = R.sizes(case)
    maps = R.make_maps(case)
    table = F.table(max(nx, ny), dtype)
    for transpose in (False, True):
        n_in, n_out = (rows, cols) if transpose else (cols, rows)
        x, res0 = rng.standard_normal(n_in).astype(dtype), rng.standard_normal(n_out).astype(dtype)
        geometry = R.abi_record(case, transpose)
        plain = R.product(x, case, maps, transpose, dtype)
        for offset in (0, 1, 4):
            assert np.array_equal(call(dtype, x, res0, rows, geometry, table, R.rounded(maps, dtype), False, offset), plain), (transpose, offset)
            assert np.array_equal(call(dtype, x, res0, rows, geometry, table, R.rounded(maps, dtype), True, offset), res0 + plain), (transpose, offset)


@pytest.mark.parametrize("prec,dtype", PRECISIONS)
@pytest.mark.parametrize("case", [(256, 64, 1, 2), (512, 8, 2, 3), (2048, 2, 1, 2), (64, 32, 1, 4)], ids=R.case_id)
def test_the_tile_of_the_coil_summing_pass_changes_no_bit(prec, dtype, case):
    """the record's tile selector: 1 (the small tile: slabs of 8, 4, 1 and 32 rows here) and 2 (fft2d's choice) give the bits of 0, in both
    directions, plain and accumulating; any other value is refused without a launch"""
    rng = np.random.default_rng(R.case_seed(case, 9))
    nx, ny, L, Cn = case
    rows, cols = R.sizes(case)
    maps = R.make_maps(case)
    table = F.table(max(nx, ny), dtype)
    for transpose in (False, True):
        n_in, n_out = (rows, cols) if transpose else (cols, rows)
        x, res0 = rng.standard_normal(n_in).astype(dtype), rng.standard_normal(n_out).astype(dtype)
        plain = R.product(x, case, maps, transpose, dtype)
        for slab in (0, 1, 2):
            geometry = R.abi_record(case, transpose, slab)
            assert np.array_equal(call(dtype, x, res0, rows, geometry, table, R.rounded(maps, dtype), False, 0), plain), (transpose, slab)
            assert np.array_equal(call(dtype, x, res0, rows, geometry, table, R.rounded(maps, dtype), True, 0), res0 + plain), (transpose, slab)
    p = C.c_void_p(16)
    for slab in (-1, 3):
        assert entry(dtype)(R.abi_record(case, True, slab).ctypes.data_as(C.c_void_p), p, p, p, p, p, 0, None) != 0
        assert b"tile selector" in _hip.lib().prost_hip_last_error()


@pytest.mark.parametrize("prec,dtype", PRECISIONS)
def test_a_nan_stays_inside_its_own_image(prec, dtype):
    prost.set_precision(prec)
    case = nx, ny, L, Cn = (32, 32, 3, 5)
    N = nx * ny
    maps = R.make_maps(case)
    bf, rows, cols = block(case, maps)
    linop = [bf(0, 0, rows, cols)[0]]
    rng = np.random.default_rng(4)
    x, y = rng.standard_normal(cols), rng.standard_normal(rows)
    clean = run(linop, x, False)[0].reshape(2, L, Cn, N)
    assert np.isfinite(clean).all()
    for l, at in ((0, 5), (1, N + N // 2 + 3), (2, (L + 2) * N + 7)):        # re_0, re_1, im_2
        xn = x.copy()
        xn[at] = np.nan
        got = run(linop, xn, False)[0].reshape(2, L, Cn, N)
        others = [k for k in range(L) if k != l]
        assert all(np.isnan(got[:, l, c]).any() for c in range(Cn))             # every coil image of l
        assert np.array_equal(got[:, others], clean[:, others])
    clean = run(linop, y, True)[0].reshape(2, L, N)
    assert np.isfinite(clean).all()
    for l, c, part in ((0, 0, 0), (1, 4, 1), (2, 2, 0)):
        yn = y.copy()
        yn[(part * L * Cn + l * Cn + c) * N + 11] = np.nan
        got = run(linop, yn, True)[0].reshape(2, L, N)
        others = [k for k in range(L) if k != l]
        assert np.isnan(got[:, l]).any() and np.array_equal(got[:, others], clean[:, others])


@pytest.mark.parametrize("prec,dtype", PRECISIONS)
@pytest.mark.parametrize("case", [(8, 4, 1, 3), (16, 16, 1, 2)], ids=R.case_id)
def test_against_the_dense_twin_on_the_gpu(prec, dtype, case):
    prost.set_precision(prec)
    nx, ny, L, Cn = case
    N = nx * ny
    rng = np.random.default_rng(100 + nx)
    maps = R.make_maps(case, zeros=True)
    K = R.matrix(case, maps, dtype)
    rows, cols = K.shape
    twin = [prost.block.dense(K)(0, 0, rows, cols)[0]]
    linop = [block(case, maps)[0](0, 0, rows, cols)[0]]
    # sqrt(2) s |sigma_c(p)| bounds |cos| |s.re| + |sin| |s.im| of every entry of rows (c, q) and columns p
    mag = math.sqrt(2.0 / N) * np.abs(R.maps64(maps, dtype))
    Kabs = np.tile(np.repeat(mag, N, axis=0), (2, 2))
    u = float(np.finfo(dtype).eps) / 2
    factor = 2 if dtype == np.float64 else 1
    for transpose, B in zip((False, True), R.bounds(case, dtype)):
        n_in = rows if transpose else cols
        x = rng.standard_normal(n_in).astype(dtype).astype(np.float64)
        got, want = run(linop, x, transpose)[0], run(twin, x, transpose)[0]
        gamma = (n_in + 4) * u / (1 - (n_in + 4) * u)
        own = R.image_norms(gamma * ((Kabs.T if transpose else Kabs) @ np.abs(x)), L if transpose else L * Cn, N)
        err = R.image_norms(got - want, L if transpose else L * Cn, N)
        scale = R.transposed_scales(x, case, maps, dtype) if transpose else R.forward_scales(x, case, maps, dtype)
        limit = factor * (B * scale + own)
        print("%s %s transpose=%d: |got - twin| / (bound + twin's own) = %.3f" % (prec, R.case_id(case), transpose, float((err / limit).max())))
        assert np.all(err <= limit), float((err / limit).max())


# ---- the solve ----
SOLVE_ITERS = 200
SOLVE_SIZE = 16
SOLVE_COILS = 4
SOLVE_MULTIPLE = 4


@functools.lru_cache(maxsize=None)
def solve(precision, twin):
    import sense_mri as ex
    dtype = dict(PRECISIONS)[precision]
    backend = prost.backend.pdhg(stepsize="alg1", residual_iter=10)
    opts = dict(max_iters=SOLVE_ITERS, num_cback_calls=0, verbose=False, tol_rel_primal=0, tol_rel_dual=0, tol_abs_primal=0, tol_abs_dual=0)
    prost.set_precision(precision)
    prob, _, _, u, _, _, mask, _ = ex.describe(SOLVE_SIZE, SOLVE_COILS, 0.5, twin=twin, dtype=dtype)
    assert mask.mean() == 0.5
    r = prost.solve(prob, backend, prost.options(**opts))
    return np.array(u.val, dtype=np.float64).ravel(), r


def test_solve_with_the_block_against_the_dense_twin():
    (b32, r1), (b64, r2), (t32, r3), (t64, r4) = solve("single", False), solve("double", False), solve("single", True), solve("double", True)
    assert all(r["iters"] == SOLVE_ITERS for r in (r1, r2, r3, r4))
    assert r1["path"] == "pdhg:generic" and r2["path"] == "pdhg:generic", (r1["path"], r2["path"])
    assert np.isfinite(b32).all() and np.isfinite(b64).all() and b32.shape == t64.shape == (2 * SOLVE_SIZE * SOLVE_SIZE,)
    scale = float(np.abs(t64).max())
    D = float(np.abs(t32 - t64).max()) / scale
    mine32, mine64 = float(np.abs(b32 - t64).max()) / scale, float(np.abs(b64 - t64).max()) / scale
    limit64 = 10 * SOLVE_ITERS * R.bounds((SOLVE_SIZE, SOLVE_SIZE, 1, SOLVE_COILS), np.float64)[1]       # c u = Bt
    print("solve: D = |twin32 - twin64| / |twin64| = %.3g, |block32 - twin64| / |twin64| = %.3g = %.2f D, |block64 - twin64| / |twin64| = %.3g = %.3f of %.3g"
          % (D, mine32, mine32 / D, mine64, mine64 / limit64, limit64))
    assert D > 0
    assert mine32 <= SOLVE_MULTIPLE * D, (mine32, D)
    assert mine64 <= limit64, (mine64, limit64)


def test_the_example_beats_the_zero_filled_image_and_agrees_with_its_twin():
    import sense_mri as ex
    prost.set_precision("double")
    size, coils = 32, 8
    result, img, truth, data, zero_filled = ex.main(size, coils, max_iters=5000, verbose=False)
    twin_result, twin_img, _, _, _ = ex.main(size, coils, max_iters=5000, verbose=False, twin=True, data=data)
    rec, zf = ex.rmse(img, truth), ex.rmse(zero_filled, truth)
    limit = 10 * max(result["iters"], 1) * R.bounds((size, size, 1, coils), np.float64)[1]
    apart = float(np.abs(img - twin_img).max()) / float(np.abs(twin_img).max())
    print("example: %s after %d iterations on %s (twin: %s after %d), RMSE %.5f, coil-combined zero-filled %.5f, |block - twin| / |twin| = %.3g of limit %.3g"
          % (result["result"], result["iters"], result["path"], twin_result["result"], twin_result["iters"], rec, zf, apart, limit))
    assert result["result"] in ("Converged.", "Reached maximum iterations.") and (result["result"] == "Converged." or result["iters"] == 5000)
    assert result["path"] == "pdhg:generic", result["path"]
    assert img.size == 2 * size * size and np.isfinite(img).all() and np.isfinite(twin_img).all()
    assert rec < zf
    assert twin_result["iters"] == result["iters"] and apart <= limit, (apart, limit)
