"""prost.block.wavelet2d on the GPU: the kernels through prost.eval_linop and through the C ABI, the block in the solver and in
examples/wavelet_mri.py.

References: tests/wavelet2d_reference.py, never the code under test.  u is the unit roundoff of T, B the bound (e) of the reference,
B = (1 + eta)^(2 levels) - 1 per plane in the 2-norm (derived in include/prost/linop/wavelet2d.hpp).
  * products: forward and transposed equal the NumPy restatement (b) in T bit for bit (-0 and +0 compare equal), the same call twice
    gives the same bits; within B of the explicit matrix (c) where N <= 4096, in both precisions; row and column sums through
    prost.eval_linop against the sums (d) of the explicit matrix within the reference's sums_tolerance plus 4 eps_T;
  * composition: [K K] and [K ; K] accumulate in the forward and in the transposed product, a 1 x 1 diags block in front gives the
    block odd row and column offsets: bit for bit;
  * 1 x 2 with L = 70000, more planes than the grid holds: bit for bit;
  * the C entry points at element offsets 0, 1 and 4 and with rhs, res or work alone at offset 1, plain and accumulating, with the
    reference's taps, with and without the one-workgroup tail: bit for bit; rhs is left alone, and so is the work buffer in front of
    its offset;
  * a NaN or an Inf in plane 0 of three leaves planes 1 and 2 bit-identical to the clean run;
  * against prost.block.sparse of matrix (c) on the GPU: |got - twin|_2 <= B |x|_2 per plane in both precisions; the ratio is printed;
  * the three-term problem at 16 x 16 (db2, 2 levels, half of k-space), alg1 with fixed steps, 200 iterations, tolerances 0, identity
    scaling: with the blocks on the GPU (i), with the explicit twins on the GPU (ii) and with the same matrices in the oracle (iii; the
    oracle has no dense block and takes the Fourier matrix through its sparse one).  D = |u_ii - u_iii| / |u_iii|, measured on the pair
    that runs no code of the block; (i) is held to max(10 D, 10 * 200 * B) of (iii), the rule of test_gpu_fft2d.py;
  * examples/wavelet_mri.py at 32 x 32 in fp64, default parameters (half of the k-space lines, db2 at 3 levels, lmb_w = 0.001,
    lmb_tv = 0.005).  The oracle with the twins on the CPU reaches an RMSE to the phantom of 0.03090 (410 iterations, "Converged."); the
    zero-filled inverse transform of the data has 0.10352.  The inequality asked of the GPU run with the blocks is
    RMSE <= 0.65 * 0.10352 = 0.06729, which the oracle meets 2.18 times over.
"""
import contextlib
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

import oracle
import prost_amd as prost
import wavelet2d_reference as R
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
    nx, ny, L, wavelet, levels = case
    return prost.block.wavelet2d(nx, ny, L, R.taps(wavelet), levels), L * nx * ny


@pytest.mark.parametrize("prec,dtype", PRECISIONS)
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_products_bit_for_bit_repeatable_within_the_bound_and_sums(prec, dtype, case):
    prost.set_precision(prec)
    nx, ny, L, wavelet, levels = case
    rng = np.random.default_rng(R.case_seed(case))
    bw, n = block(case)
    linop = [bw(0, 0, n, n)[0]]
    small = nx * ny <= 4096
    eps = np.finfo(dtype).eps
    B = R.bound(wavelet, levels, dtype)
    for transpose in (False, True):
        x = rng.standard_normal(n).astype(dtype).astype(np.float64)
        got, rowsum, colsum = run(linop, x, transpose)
        want = R.product(x, nx, ny, L, wavelet, levels, transpose, dtype).astype(np.float64)
        assert got.shape == want.shape and np.array_equal(got, want), (transpose, float(np.abs(got - want).max()), int((got != want).sum()))
        assert np.array_equal(run(linop, x, transpose)[0], got)                 # no atomics: the same bits every time
        if small:
            err = R.plane_norms(got - R.apply_matrix(x, nx, ny, L, wavelet, levels, transpose), nx, ny, L) / R.plane_norms(x, nx, ny, L)
            print("%s %s transpose=%d: |got - K x| / (B |x|) = %.3f" % (prec, R.case_id(case), transpose, float(err.max()) / B))
            assert np.all(err <= B), float(err.max()) / B
            for side, s in enumerate((rowsum, colsum)):
                want_sums = R.sums(nx, ny, L, wavelet, levels, 1.0)[side]
                tol = np.tile(R.sums_tolerance(nx, ny, wavelet, levels, 1.0)[side], L)
                assert s.shape == want_sums.shape and np.all(np.abs(s - want_sums) <= tol + 4 * eps * want_sums)


@pytest.mark.parametrize("prec,dtype", PRECISIONS)
def test_more_planes_than_the_grid_holds(prec, dtype):
    """the planes go on the grid, 65535 at most: with L = 70000 a workgroup loops over a second plane (1 x 2: 140 000 values)"""
    prost.set_precision(prec)
    nx, ny, L = 1, 2, 70000
    n = L * nx * ny
    linop = [prost.block.wavelet2d(nx, ny, L, "haar", 1)(0, 0, n, n)[0]]
    x = np.random.default_rng(70).standard_normal(n).astype(dtype).astype(np.float64)
    for transpose in (False, True):
        got = run(linop, x, transpose)[0]
        assert np.array_equal(got, R.product(x, nx, ny, L, "haar", 1, transpose, dtype).astype(np.float64)), transpose


COMPOSED = [c for c in R.CASES if c[0] * c[1] <= 16384 and min(c[0], c[1]) > 1]


@pytest.mark.parametrize("prec,dtype", PRECISIONS)
@pytest.mark.parametrize("case", COMPOSED, ids=R.case_id)
def test_composition_bit_for_bit(prec, dtype, case):
    """[K K]: the second block adds onto the first in the forward product; [K ; K]: in the transposed one; diag(d, K) with a 1 x 1 diags
    block d in front: K's rows and columns start at element 1"""
    prost.set_precision(prec)
    rng = np.random.default_rng(R.case_seed(case, 1))
    bw, n = block(case)
    P = lambda v, transpose, res0=None: R.product(v, *case, transpose, dtype, res0=res0)
    x2, x1 = rng.standard_normal(2 * n), rng.standard_normal(n)
    side = [bw(0, 0, n, n)[0], bw(0, n, n, n)[0]]
    assert np.array_equal(run(side, x2, False)[0], P(x2[n:], False, res0=P(x2[:n], False)).astype(np.float64))
    assert np.array_equal(run(side, x1, True)[0], np.tile(P(x1, True), 2).astype(np.float64))
    stack = [bw(0, 0, n, n)[0], bw(n, 0, n, n)[0]]
    assert np.array_equal(run(stack, x1, False)[0], np.tile(P(x1, False), 2).astype(np.float64))
    assert np.array_equal(run(stack, x2, True)[0], P(x2[n:], True, res0=P(x2[:n], True)).astype(np.float64))
    shifted = [prost.block.diags(1, 1, [2.0], [0])(0, 0, 1, 1)[0], bw(1, 1, n, n)[0]]
    for transpose in (False, True):
        xs = rng.standard_normal(n + 1)
        got = run(shifted, xs, transpose)[0]
        want = np.concatenate([(np.zeros(1, dtype) + dtype(2.0) * xs[:1].astype(dtype)), P(xs[1:], transpose)])
        assert np.array_equal(got, want.astype(np.float64)), transpose
        assert np.array_equal(run(shifted, xs, transpose)[0], got)


def entry(dtype):
    fn = _hip.fn("wavelet2d", dtype)
    fn.argtypes = [C.c_void_p] * 5 + [C.c_int, C.c_void_p]
    fn.restype = C.c_int
    return fn


def call(dtype, x, res0, geometry, taps, nwork, accumulate, offsets):
    """one call through the C ABI; rhs, res and work start offsets = (rhs, res, work) elements into their allocations, each exactly as
    long as it has to be"""
    pads = [np.zeros(o, dtype) for o in offsets]
    keep = [_hip.DeviceArray.from_host(np.concatenate([pads[0], x.astype(dtype)])), _hip.DeviceArray.from_host(np.concatenate([pads[1], res0.astype(dtype)])),
            _hip.DeviceArray.from_host(np.concatenate([pads[2], np.zeros(nwork, dtype)]))]
    rhs, res, work = keep
    taps = np.ascontiguousarray(taps, dtype)
    try:
        _hip.check(entry(dtype)(geometry.ctypes.data_as(C.c_void_p), taps.ctypes.data_as(C.c_void_p), work.offset(offsets[2]), res.offset(offsets[1]), rhs.offset(offsets[0]),
                                int(accumulate), None))
        _hip.sync()
        out = res.to_host()
        assert out.size == offsets[1] + x.size and np.array_equal(out[:offsets[1]], pads[1]) and np.array_equal(work.to_host()[:offsets[2]], pads[2])
        assert np.array_equal(rhs.to_host()[offsets[0]:], x.astype(dtype))
        return out[offsets[1]:]
    finally:
        for d in keep:
            d.free()


@pytest.mark.parametrize("prec,dtype", PRECISIONS)
def test_c_abi_offset_pointers_plain_and_accumulating_with_and_without_the_tail(prec, dtype):
    """offset 0 / 4: 16-byte aligned; 1: aligned for one element only; then one of rhs, res and work alone at offset 1, so that the load
    side and the store side of a launch decide differently.  The taps are the reference's, made from the definition.  Without the
    tail every level, down to the 2 x 2 corner, runs in the tiled kernels and the work buffer carries every corner"""
    rng = np.random.default_rng(12)
    for case in ((12, 20, 1, "db3", 2), (32, 32, 3, "haar", 5), (1, 64, 2, "db2", 3), (160, 96, 1, "db3", 3), (128, 128, 1, "lat16", 3)):
        nx, ny, L, wavelet, levels = case
        n = L * nx * ny
        taps = R.taps(wavelet).astype(dtype)
        for transpose in (False, True):
            x, res0 = rng.standard_normal(n).astype(dtype), rng.standard_normal(n).astype(dtype)
            plain = R.product(x, nx, ny, L, wavelet, levels, transpose, dtype)
            for no_tail in (False, True):
                geometry = R.abi_record(nx, ny, L, len(taps), levels, transpose, no_tail)
                for offset in ((0, 0, 0), (1, 1, 1), (4, 4, 4), (1, 0, 0), (0, 1, 0), (0, 0, 1)):
                    assert np.array_equal(call(dtype, x, res0, geometry, taps, R.work_size(nx, ny, L, levels), False, offset), plain), (case, transpose, no_tail, offset)
                    assert np.array_equal(call(dtype, x, res0, geometry, taps, R.work_size(nx, ny, L, levels), True, offset), res0 + plain), (case, transpose, no_tail, offset)


@pytest.mark.parametrize("prec,dtype", PRECISIONS)
@pytest.mark.parametrize("case", [(32, 32, 3, "haar", 5), (128, 64, 3, "db2", 3)], ids=R.case_id)
def test_a_nan_stays_inside_its_own_plane(prec, dtype, case):
    prost.set_precision(prec)
    nx, ny, L, wavelet, levels = case
    n = L * nx * ny
    linop = [prost.block.wavelet2d(nx, ny, L, wavelet, levels)(0, 0, n, n)[0]]
    N = nx * ny
    x = np.random.default_rng(4).standard_normal(n)
    for transpose in (False, True):
        clean = run(linop, x, transpose)[0].reshape(L, N)
        assert np.isfinite(clean).all()
        for at, bad in ((0, np.nan), (N // 2 + 5, np.nan), (N - 1, np.nan), (3, np.inf), (N - 2, -np.inf)):
            xn = x.copy()
            xn[at] = bad
            got = run(linop, xn, transpose)[0].reshape(L, N)
            assert not np.isfinite(got[0]).all()                        # it reaches its own plane (how far is not defined)
            assert np.array_equal(got[1:], clean[1:])


@pytest.mark.parametrize("prec,dtype", PRECISIONS)
@pytest.mark.parametrize("case", [(12, 20, 1, "db3", 2), (24, 12, 1, "db2", 2), (32, 32, 3, "haar", 5)], ids=R.case_id)
def test_against_the_sparse_twin_on_the_gpu(prec, dtype, case):
    import scipy.sparse as sp
    prost.set_precision(prec)
    nx, ny, L, wavelet, levels = case
    rng = np.random.default_rng(100 + nx)
    one = sp.csc_matrix(R.matrix(nx, ny, wavelet, levels))
    n = L * nx * ny
    twin = [prost.block.sparse(sp.block_diag([one] * L, format="csc"))(0, 0, n, n)[0]]
    linop = [block(case)[0](0, 0, n, n)[0]]
    B = R.bound(wavelet, levels, dtype)
    for transpose in (False, True):
        x = rng.standard_normal(n).astype(dtype).astype(np.float64)
        got, want = run(linop, x, transpose)[0], run(twin, x, transpose)[0]
        err = R.plane_norms(got - want, nx, ny, L) / R.plane_norms(x, nx, ny, L)
        print("%s %s transpose=%d: |got - twin| / (B |x|) = %.3f" % (prec, R.case_id(case), transpose, float(err.max()) / B))
        assert np.all(err <= B), float(err.max()) / B


# ---- the solve ----
SOLVE_ITERS = 200
SOLVE_SIZE = 16
SOLVE_WAVELET, SOLVE_LEVELS = "db2", 2


@contextlib.contextmanager
def dense_as_sparse():
    """the oracle has no dense block: while this holds, the example's Fourier twin hands its full matrix over through prost.block.sparse"""
    import scipy.sparse as sp
    dense = prost.block.dense
    prost.block.dense = lambda K: prost.block.sparse(sp.csc_matrix(K))
    try:
        yield
    finally:
        prost.block.dense = dense


@functools.lru_cache(maxsize=None)
def solve_three_ways(precision):
    import wavelet_mri as ex
    dtype = dict(PRECISIONS)[precision]
    backend = prost.backend.pdhg(stepsize="alg1", residual_iter=10)
    opts = dict(max_iters=SOLVE_ITERS, num_cback_calls=0, verbose=False, tol_rel_primal=0, tol_rel_dual=0, tol_abs_primal=0, tol_abs_dual=0)
    shape = dict(wavelet=SOLVE_WAVELET, levels=SOLVE_LEVELS, scaling="identity")
    prost.set_precision(precision)
    out = {}
    prob, _, _, u, _, data, mask = ex.describe(SOLVE_SIZE, 0.5, twin=True, **shape)
    assert mask.mean() == 0.5
    r = prost.solve(prob, backend, prost.options(**opts))
    out["ii"] = (np.array(u.val, dtype=np.float64).ravel(), r)
    with dense_as_sparse():
        prob, _, _, u, _, _, _ = ex.describe(SOLVE_SIZE, 0.5, twin=True, data=data, **shape)
    r = oracle.solve(prob, backend, prost.options(**opts), dtype)
    out["iii"] = (np.array(u.val, dtype=np.float64).ravel(), r)
    prob, _, _, u, _, _, _ = ex.describe(SOLVE_SIZE, 0.5, data=data, **shape)
    r = prost.solve(prob, backend, prost.options(**opts))
    out["i"] = (np.array(u.val, dtype=np.float64).ravel(), r)
    return out


@pytest.mark.parametrize("precision,dtype", PRECISIONS)
def test_solve_with_the_block_against_the_twins(precision, dtype):
    out = solve_three_ways(precision)
    (u1, r1), (u2, r2), (u3, r3) = out["i"], out["ii"], out["iii"]
    assert r1["iters"] == SOLVE_ITERS and r2["iters"] == SOLVE_ITERS and r3["iters"] == SOLVE_ITERS
    assert r1["path"] == "pdhg:generic", r1["path"]
    assert np.isfinite(u1).all() and u1.shape == u3.shape == (2 * SOLVE_SIZE * SOLVE_SIZE,)
    scale = float(np.abs(u3).max())
    D = float(np.abs(u2 - u3).max()) / scale
    mine = float(np.abs(u1 - u3).max()) / scale
    limit = max(10 * D, 10 * SOLVE_ITERS * R.bound(SOLVE_WAVELET, SOLVE_LEVELS, dtype))
    print("solve %s: D = |u_ii - u_iii| / |u_iii| = %.3g, |u_i - u_iii| / |u_iii| = %.3g, |u_i - u_ii| / |u_iii| = %.3g, limit %.3g"
          % (precision, D, mine, float(np.abs(u1 - u2).max()) / scale, limit))
    assert mine <= limit, (mine, limit)


def test_the_example_reconstructs_the_phantom():
    import wavelet_mri as ex
    prost.set_precision("double")
    size = 32
    result, img, truth, data = ex.main(size, max_iters=5000, verbose=False)
    zero_filled = ex.rmse(ex.zero_filled(data, size, size), truth)
    print("example: %s after %d iterations on %s, RMSE %.5f, zero-filled %.5f" % (result["result"], result["iters"], result["path"], ex.rmse(img, truth), zero_filled))
    assert result["result"] in ("Converged.", "Reached maximum iterations.") and (result["result"] == "Converged." or result["iters"] == 5000)
    assert result["path"] == "pdhg:generic", result["path"]
    assert img.size == 2 * size * size and np.isfinite(img).all()
    assert abs(zero_filled - 0.10352) < 1e-4                # the comparator runs no code of the block
    assert ex.rmse(img, truth) <= 0.65 * zero_filled
