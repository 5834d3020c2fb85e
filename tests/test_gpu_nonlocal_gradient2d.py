"""prost.block.nonlocal_gradient2d on the GPU: the kernels through prost.eval_linop and through the C ABI, the block in the solver and in
examples/nltv_denoise.py.

References: tests/nonlocal_gradient2d_reference.py, never the code under test.
  * products: forward and adjoint equal the NumPy restatement (b) in T bit for bit, signs of zeros included, the same call twice gives
    the same bits; row and column sums equal to (c) for the dyadic weights and within (t + 8) eps_T otherwise, t = 2 M; both precisions;
  * unit weights and offsets ((0, 1), (1, 0)): the forward product has the bits of prost_hip_grad2d_fwd;
  * the C entry points with res, rhs and the weights each alone at element offset 1 (the element kernels) and all at 0 and 4 (the vector
    kernels where the height allows), plain and accumulating, both directions: bit for bit, padding untouched, rhs and weights
    unchanged; refusals without a launch;
  * against the oracle's block.sparse on matrix (a): |got - twin| <= (gamma_block + gamma_twin) B componentwise, n = 2 forward and 2 M
    for the adjoint on either side (derived in the header, not measured); the worst ratio is printed (docs/rounds/r30.md);
  * absent terms: through the C entry points (the front end refuses non-finite weights) an Inf weight at every position whose target is
    outside the grid reaches no output, on the element and on the vector path;
  * nonlocal TV at 24 x 16 with the example's operator (M = 48), alg1 with fixed steps, 200 iterations: the block on the GPU against the
    sparse twin in the oracle, |difference| / |solution| <= 10 * 200 * n * u with n = 2 M, the longest chain of roundings of a product;
  * the example converges on pdhg:generic and RMSE(NL-TV) < RMSE(TV) < RMSE(noisy): the ordering against TV is asserted because the
    oracle through the twin shows it on the CPU at 24 x 16 and at 48 x 32 for this seed (tests/test_nonlocal_gradient2d_frontend.py).

Shapes (nonlocal_gradient2d_reference.CASES), from the kernel's constants: a workgroup owns a tile of 64 x 16 pixels, so the list holds
each tile side - 1, + 0, + 1 and twice + 1; a lane of the vector path holds 16 bytes of a column, so heights that are no multiple of 4
(fp32) or 2 (fp64) take the element kernels; the channels of a pass come from the tile table (3 in fp32 and 1 in fp64 at reach 15, 4 at
reach 1), so L = 4 at reach 15 and L = 5 at reach 1 are one more than a pass; 1 x 1 masks every term; 5 x 3 is smaller than the reach.
"""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

import oracle
import prost_amd as prost
import nonlocal_gradient2d_reference as R
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


def block(nx, ny, L, offsets, planes, row=0, col=0):
    bf = prost.block.nonlocal_gradient2d(nx, ny, L, offsets, planes)
    m, n = bf(0, 0, 0, 0)[1]
    return bf(row, col, m, n)[0], m, n


def test_the_shape_list_follows_the_kernel_constants():
    assert (R.TILE_Y, R.TILE_X, R.THREADS, R.MAX_PASS) == (64, 16, 256, 4)
    heights, widths = {c[0] for c in R.CASES}, {c[1] for c in R.CASES}
    assert {R.TILE_Y - 1, R.TILE_Y, R.TILE_Y + 1, 2 * R.TILE_Y + 1} <= heights and {R.TILE_X - 1, R.TILE_X, R.TILE_X + 1, 2 * R.TILE_X + 1} <= widths
    assert (1, 1) in {c[:2] for c in R.CASES} and any(c[0] == 1 and c[1] > 1 for c in R.CASES) and any(c[1] == 1 and c[0] > 1 for c in R.CASES)
    assert any(c[0] % 4 and c[0] % 2 == 0 for c in R.CASES) and any(c[0] % 2 for c in R.CASES) and any(c[0] % 4 == 0 for c in R.CASES)
    assert any(c[0] < R.reach(R.OFFSETS[c[3]]) and c[1] < R.reach(R.OFFSETS[c[3]]) for c in R.CASES)
    assert {len(R.OFFSETS[c[3]]) for c in R.CASES} >= {1, 24, 64} and R.OFFSETS["w2"] == R.window(2)
    assert all(dy >= 0 and dx >= 0 for dy, dx in R.OFFSETS["pos"]) and all(dy <= 0 and dx <= 0 for dy, dx in R.OFFSETS["neg"])
    assert {c[2] for c in R.CASES} >= {1, 3}
    for dtype in (np.float32, np.float64):
        far = R.pass_channels(R.OFFSETS["far"], dtype)
        assert R.reach(R.OFFSETS["far"]) == R.MAX_REACH and far == (3 if dtype is np.float32 else 1)
        assert any(c[3] == "far" and c[2] > far for c in R.CASES)
    assert (24, 20, 4, "far") in R.CASES and R.pass_channels(R.OFFSETS["far"], np.float32) + 1 == 4
    assert (16, 9, 5, "w1") in R.CASES and R.pass_channels(R.OFFSETS["w1"], np.float64) + 1 == 5


@pytest.mark.parametrize("prec,dtype", PRECISIONS)
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_products_bit_for_bit_and_sums(prec, dtype, case):
    prost.set_precision(prec)
    ny, nx, L, key = case
    offsets = R.OFFSETS[key]
    rng = np.random.default_rng(R.case_seed(case))
    tol = (R.sum_terms(len(offsets)) + 8) * np.finfo(dtype).eps
    planes = R.weights_for(case)                           # zeros and negative values included
    b, nrows, ncols = block(nx, ny, L, offsets, planes)
    rs, cs = R.sums(nx, ny, L, offsets, planes, 1.0, dtype)
    for transpose in (False, True):
        x = rng.standard_normal(nrows if transpose else ncols)
        got, rowsum, colsum = run([b], x, transpose)
        want = R.product(x, nx, ny, L, offsets, planes, transpose, dtype).astype(np.float64)
        assert got.shape == want.shape and np.array_equal(got, want), (transpose, int((got != want).sum()), float(np.abs(got - want).max()))
        assert np.array_equal(np.signbit(got), np.signbit(want)), transpose
        assert np.array_equal(run([b], x, transpose)[0], got)                 # no atomics: the same bits every time
        assert rowsum.shape == rs.shape and colsum.shape == cs.shape
        assert np.all(np.abs(rowsum - rs) <= tol * rs) and np.all(np.abs(colsum - cs) <= tol * cs)
        if R.is_dyadic(case):
            assert np.array_equal(rowsum, rs) and np.array_equal(colsum, cs)
    if nx * ny == 1:
        assert not run([b], np.array([np.inf] * ncols), False)[0].any()        # every term is masked


def entry(dtype):
    fn = _hip.fn("linop_nonlocal_gradient2d", dtype)
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, C.c_char_p, C.c_int, C.c_int, C.c_void_p]
    fn.restype = C.c_int
    return fn


def pairs(offsets):
    return np.array(offsets, dtype=np.int8).tobytes()


def call(dtype, x, res0, offsets, planes, nx, ny, L, transpose, accumulate, at=(0, 0, 0)):
    """one launch through the C ABI; res, rhs and the weights start at[0], at[1], at[2] elements into their allocations.  The planes go
    to the device as they are, non-finite values included."""
    w = np.concatenate(planes).astype(dtype)
    hosts = [np.concatenate([np.zeros(at[0], dtype), res0.astype(dtype)]), np.concatenate([np.zeros(at[1], dtype), x.astype(dtype)]), np.concatenate([np.zeros(at[2], dtype), w])]
    keep = [_hip.DeviceArray.from_host(h) for h in hosts]
    res, rhs, wts = keep
    try:
        _hip.check(entry(dtype)(res.offset(at[0]), rhs.offset(at[1]), wts.offset(at[2]), nx, ny, L, len(offsets), pairs(offsets), int(transpose), int(accumulate), None))
        _hip.sync()
        out = res.to_host()
        assert out.size == at[0] + res0.size and not out[:at[0]].any()
        assert np.array_equal(rhs.to_host(), hosts[1], equal_nan=True) and np.array_equal(wts.to_host(), hosts[2], equal_nan=True)
        return out[at[0]:]
    finally:
        for d in keep:
            d.free()


@pytest.mark.parametrize("prec,dtype", PRECISIONS)
def test_c_abi_offset_pointers_plain_and_accumulating(prec, dtype):
    """all at 0 or 4: 16-byte aligned (the vector kernels where the height allows); res, rhs or the weights alone at element 1: the
    element kernels"""
    rng = np.random.default_rng(12)
    for case in ((64, 15, 1, "w1"), (8, 33, 3, "w2"), (24, 20, 4, "far"), (66, 4, 1, "pos"), (5, 3, 3, "far")):
        ny, nx, L, key = case
        offsets = R.OFFSETS[key]
        M, N = len(offsets), nx * ny
        planes = R.random_weights(nx, ny, M, 7 + ny)
        for transpose in (False, True):
            nres, nrhs = (L * N, M * L * N) if transpose else (M * L * N, L * N)
            x, res0 = rng.standard_normal(nrhs).astype(dtype), rng.standard_normal(nres).astype(dtype)
            plain = R.product(x, nx, ny, L, offsets, planes, transpose, dtype)
            for at in ((0, 0, 0), (4, 4, 4), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1)):
                where = (case, transpose, at)
                assert np.array_equal(call(dtype, x, res0, offsets, planes, nx, ny, L, transpose, False, at), plain), where
                assert np.array_equal(call(dtype, x, res0, offsets, planes, nx, ny, L, transpose, True, at), res0 + plain), where
    # refusals without a launch
    fn, p, ok = entry(dtype), C.c_void_p(16), pairs([(0, 1), (1, 0)])
    for args in ((p, p, p, 0, 4, 1, 2, ok), (p, p, p, 4, 0, 1, 2, ok), (p, p, p, 4, 4, 0, 2, ok), (p, p, p, 4, 4, 1, 0, ok), (p, p, p, 4, 4, 1, 65, pairs([(1, 0)] * 65)),
                 (None, p, p, 4, 4, 1, 2, ok), (p, None, p, 4, 4, 1, 2, ok), (p, p, None, 4, 4, 1, 2, ok), (p, p, p, 4, 4, 1, 2, None),
                 (p, p, p, 4, 4, 1, 2, pairs([(0, 1), (16, 0)])), (p, p, p, 4, 4, 1, 2, pairs([(0, 1), (0, 0)])), (p, p, p, 2 ** 26, 2 ** 26, 4, 2, ok),
                 (p, p, p, 2 ** 40, 1, 1, 2, ok)):
        assert fn(*args, 0, 0, None) != 0 and fn(*args, 1, 1, None) != 0, args
    _hip.sync()


@pytest.mark.parametrize("prec,dtype", PRECISIONS)
def test_unit_weights_and_the_two_forward_neighbours_are_grad2d_fwd_bit_for_bit(prec, dtype):
    grad = _hip.fn("grad2d_fwd", dtype)
    grad.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_void_p]
    grad.restype = C.c_int
    offsets = R.OFFSETS["grad"]
    for ny, nx, L in ((1, 1, 1), (1, 7, 1), (5, 1, 1), (65, 16, 1), (64, 17, 3), (130, 5, 2)):
        N = nx * ny
        x = np.random.default_rng(R.case_seed((ny, nx, L, "grad"), 6)).standard_normal(L * N).astype(dtype)
        x[::5] = -0.0
        got = call(dtype, x, np.zeros(2 * L * N, dtype), offsets, R.ones_weights(nx, ny, 2), nx, ny, L, False, False)
        rhs, res = _hip.DeviceArray.from_host(x), _hip.DeviceArray.from_host(np.full(2 * L * N, 7, dtype))
        try:
            _hip.check(grad(res.offset(0), rhs.offset(0), nx, ny, L, 0, 0, None))
            _hip.sync()
            want = res.to_host()
        finally:
            rhs.free()
            res.free()
        assert np.array_equal(got, want) and np.array_equal(np.signbit(got), np.signbit(want)), (ny, nx, L)
        assert np.array_equal(want, R.gradient_product(x, nx, ny, L, dtype))


@pytest.mark.parametrize("prec,dtype", PRECISIONS)
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_against_the_sparse_twin_in_the_oracle(prec, dtype, case):
    prost.set_precision(prec)
    ny, nx, L, key = case
    offsets = R.OFFSETS[key]
    rng = np.random.default_rng(R.case_seed(case, 2))
    planes = R.rounded(R.random_weights(nx, ny, len(offsets), R.case_seed(case, 90)), dtype)
    K = R.matrix(nx, ny, L, offsets, planes, dtype)
    m, n = K.shape
    linop = [block(nx, ny, L, offsets, planes)[0]]
    if K.nnz == 0:                                    # 1 x 1: the matrix is empty and so is the product
        for transpose in (False, True):
            assert not run(linop, rng.standard_normal(m if transpose else n), transpose)[0].any()
        return
    twin = [prost.block.sparse(K)(0, 0, m, n)[0]]
    for transpose in (False, True):
        x = rng.standard_normal(m if transpose else n).astype(dtype).astype(np.float64)
        got = run(linop, x, transpose)[0]
        want = np.asarray(oracle.eval_linop(twin, x, transpose, dtype)[0], dtype=np.float64).ravel()
        bound = R.bound(nx, ny, L, offsets, planes, transpose, x, dtype, twin=True)
        err = np.abs(got - want)
        live = bound > 0
        print("%s %s transpose=%d: |got - twin| / bound %.3f" % (prec, R.case_id(case), transpose, float((err[live] / bound[live]).max()) if live.any() else 0.0))
        assert np.all(err <= bound), float((err[live] / bound[live]).max())


@pytest.mark.parametrize("prec,dtype", PRECISIONS)
def test_an_inf_weight_at_a_masked_position_reaches_no_output(prec, dtype):
    for ny, nx, L in ((5, 3, 2), (8, 5, 2), (64, 17, 1)):             # the element kernels; the vector kernels (and offset 1: the element kernels again)
        offsets = R.OFFSETS["w1"] + [(15, 0), (-3, 4)]
        M, N = len(offsets), nx * ny
        clean = R.random_weights(nx, ny, M, 9 + ny)
        planes = [p.copy() for p in clean]
        for m, (dy, dx) in enumerate(offsets):
            planes[m][~R.inside(nx, ny, dy, dx).reshape(-1)] = np.inf if m % 2 else -np.inf
        rng = np.random.default_rng(4)
        for transpose, v in ((False, rng.standard_normal(L * N)), (True, rng.standard_normal(M * L * N))):
            want = R.product(v, nx, ny, L, offsets, clean, transpose, dtype)
            assert np.isfinite(want).all()
            for at in ((0, 0, 0), (1, 1, 1)):
                got = call(dtype, v, np.zeros(want.size), offsets, planes, nx, ny, L, transpose, False, at)
                assert np.array_equal(got, want), (ny, nx, transpose, at)


# ---- the solve ----
SOLVE_ITERS = 200
SOLVE_NX, SOLVE_NY = 24, 16


@functools.lru_cache(maxsize=None)
def solve_both(precision):
    import nltv_denoise as ex
    dtype = dict(PRECISIONS)[precision]
    backend = prost.backend.pdhg(stepsize="alg1", residual_iter=10)
    opts = dict(max_iters=SOLVE_ITERS, num_cback_calls=0, verbose=False, tol_rel_primal=0, tol_rel_dual=0, tol_abs_primal=0, tol_abs_dual=0)
    prost.set_precision(precision)
    _, f = ex.striped_image(SOLVE_NX, SOLVE_NY)
    offsets, planes = ex.nonlocal_weights(f, SOLVE_NX, SOLVE_NY)
    out = {}
    for key, twin, solver in (("block", False, None), ("twin", True, oracle)):
        prob, _, _, u, _, _, _, _ = ex.describe(SOLVE_NX, SOLVE_NY, f=f, twin=twin, offsets=offsets, planes=planes)
        r = prost.solve(prob, backend, prost.options(**opts)) if solver is None else oracle.solve(prob, backend, prost.options(**opts), dtype)
        out[key] = (np.array(u.val, dtype=np.float64).ravel(), r)
    return out, len(offsets)


@pytest.mark.parametrize("precision,dtype", PRECISIONS)
def test_solve_with_the_block_against_the_sparse_twin_in_the_oracle(precision, dtype):
    out, M = solve_both(precision)
    (x1, r1), (x2, r2) = out["block"], out["twin"]
    assert r1["iters"] == SOLVE_ITERS and r2["iters"] == SOLVE_ITERS
    assert r1["path"] == "pdhg:generic", r1["path"]
    assert np.isfinite(x1).all() and x1.shape == x2.shape == (SOLVE_NX * SOLVE_NY,)
    mine = float(np.abs(x1 - x2).max()) / float(np.abs(x2).max())
    limit = 10 * SOLVE_ITERS * R.roundings(M, True) * (np.finfo(dtype).eps / 2)
    print("solve %s M=%d: |block on the GPU - twin in the oracle| / |twin| = %.3g, limit 10 * %d * %d * u = %.3g" % (precision, M, mine, SOLVE_ITERS, R.roundings(M, True), limit))
    assert mine <= limit, (mine, limit)


def test_the_example_converges_and_beats_tv_and_the_noisy_data():
    import nltv_denoise as ex
    prost.set_precision("double")
    nx, ny = 24, 16
    result, img, result_tv, img_tv, f, clean = ex.main(nx, ny, max_iters=20000, verbose=False)
    assert np.array_equal(f, clean + 0.1 * np.random.default_rng(1).standard_normal(nx * ny)) and np.unique(clean).size == 4
    print("example: nonlocal TV %s after %d iterations on %s, RMSE %.4f; TV %s after %d iterations, RMSE %.4f; data %.4f"
          % (result["result"], result["iters"], result["path"], ex.rmse(img, clean), result_tv["result"], result_tv["iters"], ex.rmse(img_tv, clean), ex.rmse(f, clean)))
    assert result["result"] == "Converged." and result_tv["result"] == "Converged."
    assert result["path"] == "pdhg:generic", result["path"]
    assert img.shape == (nx * ny,) and np.isfinite(img).all()
    assert ex.rmse(img, clean) < ex.rmse(img_tv, clean) < ex.rmse(f, clean)
