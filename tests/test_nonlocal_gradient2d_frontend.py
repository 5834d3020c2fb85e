"""prost.block.nonlocal_gradient2d without a GPU: the builders, the registry name, the creation errors, the preconditioners, the entry
points -- and the definition itself, on the references of tests/nonlocal_gradient2d_reference.py.

  * the builder describes { 'nonlocal_gradient2d', row, col, { nx, ny, L, offsets, weights } } with size [M L N, L N] from an (M, N)
    array, an (M, ny, nx) array or a sequence of M planes, and refuses bad arguments with ValueError, each with its own message;
    nonlocal_window(r) is the full window in its documented order;
  * the name is registered for both precisions; every refusal of the factory, by its message, through prost.problem_info;
  * matrix (a) has the entries of the definition, entry by entry;
  * restatement (b) against (a): with dyadic weights and dyadic data every operation is exact and (b) equals (a) x; in general
    |(b) - (a) x| <= gamma_n B componentwise with the roundings n of the header (2 forward, 2 M adjoint); <K x, y> = <x, K^T y> within
    the bound carried through the inner products; K 1 = 0 exactly; unit weights and offsets ((0, 1), (1, 0)) are the gradient
    restatement bit for bit; the accumulating form adds res0 last; an Inf weight at a position whose target is outside the grid
    reaches no output;
  * the preconditioners of a problem with the block for alpha = 1 and 2 within (t + 8) eps_T of (c), t = 2 M, exact for dyadic weights;
  * the oracle solves the problem of examples/nltv_denoise.py with the sparse twin at 24 x 16 and 48 x 32: it converges and
    RMSE(NL-TV) < RMSE(TV) < RMSE(noisy) at both sizes for the committed seed (which is what lets the GPU test assert the ordering);
  * include/prost_hip.h declares the two entry points, the kernel library exports them, they refuse bad arguments without a device, and
    the ABI version is still 10.
"""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

import oracle
import prost_amd as prost
import nonlocal_gradient2d_reference as R
from prost_amd import _hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples"))
PRECISIONS = [("single", np.float32), ("double", np.float64)]
LIGHT = [c for c in R.CASES if c[0] * c[1] * c[2] * len(R.OFFSETS[c[3]]) <= 30000]
GRAD = [(0, 1), (1, 0)]


def test_builder_cells_and_size():
    off = [(0, 1), (1, 0), (-2, 3)]
    w = np.arange(1, 91, dtype=np.float64).reshape(3, 30) / 64
    (name, row, col, data), sz = prost.block.nonlocal_gradient2d(6, 5, 2, off, w)(3, 7, 0, 0)
    assert (name, row, col) == ("nonlocal_gradient2d", 3, 7)
    assert data[:3] == [6, 5, 2] and [type(v) for v in data[:3]] == [int, int, int]
    assert data[3].dtype == np.float64 and data[3].tolist() == [0, 1, 1, 0, -2, 3]
    assert data[4].dtype == np.float64 and np.array_equal(data[4], w.reshape(-1)) and sz == [3 * 2 * 30, 2 * 30]
    # an (M, ny, nx) array w[m, y, x]: every plane flattened with y fastest
    w3 = np.arange(90, dtype=np.float64).reshape(3, 5, 6)
    data = prost.block.nonlocal_gradient2d(6, 5, 1, np.array(off), w3)(0, 0, 0, 0)[0][3]
    assert np.array_equal(data[4], np.concatenate([p.T.reshape(-1) for p in w3])) and data[4][1] == w3[0, 1, 0] and data[4][5] == w3[0, 0, 1]
    # a sequence of planes, vectors or (ny, nx) arrays; zeros and negative values are legal
    data = prost.block.nonlocal_gradient2d(np.int64(6), 5.0, 1, off, [np.zeros(30), w3[1], -2 * np.ones(30)])(0, 0, 0, 0)[0][3]
    assert np.array_equal(data[4][30:60], w3[1].T.reshape(-1)) and not data[4][:30].any() and np.all(data[4][60:] == -2)
    assert prost.block.nonlocal_gradient2d(1, 1, 1, [(1, 0)], [[0.0]])(0, 0, 0, 0)[1] == [1, 1]
    data[4][0] = 99.0                                                                              # the builder copied its input
    assert w3[0, 0, 0] == 0.0
    full = prost.block.nonlocal_gradient2d(4, 4, 1, prost.block.nonlocal_window(3), np.ones((48, 16)))(0, 0, 0, 0)
    assert full[1] == [48 * 16, 16]


def test_nonlocal_window_order():
    w1 = prost.block.nonlocal_window(1)
    assert w1.dtype.kind == "i" and w1.tolist() == [[-1, -1], [0, -1], [1, -1], [-1, 0], [1, 0], [-1, 1], [0, 1], [1, 1]]
    for r in (1, 2, 3, 15):
        w = prost.block.nonlocal_window(r)
        assert w.shape == ((2 * r + 1) ** 2 - 1, 2) and w.tolist() == [list(o) for o in R.window(r)]
        assert len({tuple(o) for o in w.tolist()}) == len(w) and [0, 0] not in w.tolist() and np.abs(w).max() == r
    for bad, message in ((0, "at least 1"), (16, "at most 15"), (1.5, "not an integer"), (True, "not an integer")):
        with pytest.raises(ValueError, match=message):
            prost.block.nonlocal_window(bad)


def test_builder_value_errors():
    one, off = np.ones((2, 16)), GRAD
    for args, message in (((4.5, 4, 1, off, one), "not an integer"), ((4, np.inf, 1, off, one), "not an integer"), ((True, 4, 1, off, one), "not an integer"),
                          ((0, 4, 1, off, one), "at least 1"), ((4, 4, 0, off, one), "at least 1"),
                          ((4, 4, 1, [(0.5, 1), (1, 0)], one), "offsets have to be integers"), ((4, 4, 1, [(np.nan, 1), (1, 0)], one), "offsets have to be integers"),
                          ((4, 4, 1, "ab", one), "offsets have to be an array of numbers"),
                          ((4, 4, 1, [0, 1, 1, 0], one), r"an \(M, 2\) array"), ((4, 4, 1, [(0, 1, 2), (1, 0, 2)], one), r"an \(M, 2\) array"),
                          ((4, 4, 1, [(0, 1), (0, 0)], one), r"offset 1 is \(0, 0\)"),
                          ((4, 4, 1, [(0, 1), (1, 0), (0, 1)], np.ones((3, 16))), "pairwise distinct"),
                          ((4, 4, 1, [(0, 16), (1, 0)], one), "reaches beyond 15"), ((4, 4, 1, [(0, 1), (-16, 0)], one), "reaches beyond 15"),
                          ((4, 4, 1, np.zeros((0, 2)), np.ones((0, 16))), "M = 0 offsets"),
                          ((4, 4, 1, [(dy, dx) for dy in range(-4, 5) for dx in range(1, 9)][:65], np.ones((65, 16))), "M = 65 offsets"),
                          ((4, 4, 1, off, np.ones((3, 16))), "3 planes of weights for M = 2"), ((4, 4, 1, off, [np.ones(16)]), "1 planes of weights for M = 2"),
                          ((4, 4, 1, off, np.ones((2, 15))), "a plane is a vector of nx ny = 16 values"), ((4, 2, 1, off, np.ones((2, 4, 2))), "plane 0 of the weights has shape"),
                          ((4, 4, 1, off, [np.ones(16), np.ones(3)]), "plane 1 of the weights has shape"), ((4, 4, 1, off, np.ones(32)), "the weights have shape"),
                          ((4, 4, 1, off, "abc"), "array of numbers"), ((4, 4, 1, off, one.astype(complex)), "array of numbers"),
                          ((4, 4, 1, off, np.r_[np.ones(31), np.inf].reshape(2, 16)), "non-finite"), ((4, 4, 1, off, [np.ones(16), np.r_[np.nan, np.ones(15)]]), "non-finite"),
                          ((2 ** 26, 2 ** 26, 4, off, one), "within 2\\^53")):
        with pytest.raises(ValueError, match=message):
            prost.block.nonlocal_gradient2d(*args)


@pytest.mark.parametrize("precision", ["single", "double"])
def test_the_name_is_registered(precision):
    prost.set_precision(precision)
    try:
        assert "nonlocal_gradient2d" in prost.registered()["block"]
    finally:
        prost.set_precision("double")


def _raw_problem(data, nrows, ncols):
    x, z = prost.variable(ncols), prost.variable(nrows)
    prob = prost.min_max_problem([x], [z])
    prob.add_dual_pair(x, z, lambda row, col, nr, nc: [["nonlocal_gradient2d", row, col, data], [nrows, ncols]])
    return prob


@pytest.mark.parametrize("precision", ["single", "double"])
def test_every_refusal_of_the_factory_by_message(precision):
    off, one = np.array([0.0, 1, 1, 0]), np.ones(32)
    cells = "BlockNonlocalGradient2D: the data cells are { nx, ny, L, offsets, weights } or { nx, ny, L, offsets, weights, nrows, ncols }."
    many = np.array([(dy, dx) for dy in range(-4, 5) for dx in range(1, 9)][:65], dtype=np.float64).reshape(-1)
    cases = [
        ([4.5, 4, 1, off, one], "BlockNonlocalGradient2D: nx = 4.5 has to be a positive integer."),
        ([4, 0, 1, off, one], "BlockNonlocalGradient2D: ny = 0 has to be a positive integer."),
        ([4, 4, -1, off, one], "BlockNonlocalGradient2D: L = -1 has to be a positive integer."),
        ([4, 4, np.nan, off, one], "BlockNonlocalGradient2D: L = nan has to be a positive integer."),
        ([4, 4, 1, np.array([0.0, 1, 1]), one], "BlockNonlocalGradient2D: the offsets hold 3 values; they are M pairs (dy, dx), M from 1 to 64."),
        ([4, 4, 1, many, np.ones(65 * 16)], "BlockNonlocalGradient2D: the offsets hold 130 values; they are M pairs (dy, dx), M from 1 to 64."),
        ([4, 4, 1, np.array([0.0, np.inf, 1, 0]), one], "BlockNonlocalGradient2D: the offsets hold a non-finite value."),
        ([4, 4, 1, np.array([0.0, 1.5, 1, 0]), one], "BlockNonlocalGradient2D: offset 0 = (0, 1.5) is not a pair of integers."),
        ([4, 4, 1, np.array([0.0, 1, 16, 0]), one], "BlockNonlocalGradient2D: offset 1 = (16, 0) reaches beyond 15."),
        ([4, 4, 1, np.array([0.0, -16, 1, 0]), one], "BlockNonlocalGradient2D: offset 0 = (0, -16) reaches beyond 15."),
        ([4, 4, 1, np.array([0.0, 1, 0, 0]), one], "BlockNonlocalGradient2D: offset 1 is (0, 0), which is no displacement."),
        ([4, 4, 1, np.array([0.0, 1, 1, 0, 0, 1]), np.ones(48)], "BlockNonlocalGradient2D: offsets 0 and 2 are both (0, 1); the offsets have to be distinct."),
        ([4, 4, 1, off, np.ones(31)], "BlockNonlocalGradient2D: the weights hold 31 values, not M = 2 planes of nx ny = 16."),
        ([4, 4, 1, off, np.ones(48)], "BlockNonlocalGradient2D: the weights hold 48 values, not M = 2 planes of nx ny = 16."),
        ([4, 4, 1, off, np.r_[one[:5], np.inf, one[:26]]], "BlockNonlocalGradient2D: value 5 of plane 0 of the weights, inf, is not finite"),
        ([4, 4, 1, off, np.r_[one[:19], np.nan, one[:12]]], "BlockNonlocalGradient2D: value 3 of plane 1 of the weights, nan, is not finite"),
        ([2.0 ** 26, 2.0 ** 26, 4, off, one], "rows; the size has to stay within 2^53."),
        ([4, 4, 1, off, one, 32, 15], "BlockNonlocalGradient2D: the declared size 32 x 15 is not M L nx ny x L nx ny = 32 x 16."),
        ([4, 4, 2, off, one, 32, 16], "BlockNonlocalGradient2D: the declared size 32 x 16 is not M L nx ny x L nx ny = 64 x 32."),
        ([4, 4, 1, off], cells),
        ([4, 4, 1, off, one, 32], cells),
    ]
    prost.set_precision(precision)
    try:
        for data, message in cases:
            with pytest.raises(prost.ProstError, match=re.escape(message)) as err:
                prost.problem_info(_raw_problem(data, 32, 16))
            assert "Creating block with ID 'nonlocal_gradient2d' failed" in str(err.value)
        if precision == "single":              # finite as given, infinite when rounded to T
            with pytest.raises(prost.ProstError, match=re.escape("value 2 of plane 0 of the weights, 1e+60, is not finite in single precision.")):
                prost.problem_info(_raw_problem([4, 4, 1, off, np.r_[one[:2], 1e60, one[:29]]], 32, 16))
        for data in ([4, 4, 1, off, one], [4, 4, 1, off, np.zeros(32), 32, 16], [4, 4, 1, off, -1.5 * one], [2, 4, 2, off, 1e-60 * np.ones(16)]):
            info = prost.problem_info(_raw_problem(data, 32, 16))
            assert int(info["nrows"]) == 32 and int(info["ncols"]) == 16
    finally:
        prost.set_precision("double")


def test_matrix_a_is_the_definition():
    """row (m, c, p): -w_m[p] at c N + p and +w_m[p] at c N + q, q = p + dy + dx ny, only where (y + dy, x + dx) lies in the grid"""
    nx, ny, L = 5, 4, 2
    N = nx * ny
    for key in ("w1", "far", "pos", "neg", "w2"):
        offsets = R.OFFSETS[key]
        M = len(offsets)
        planes = R.dyadic_weights(nx, ny, M, 3 + M)
        K = R.matrix(nx, ny, L, offsets, planes).toarray()
        want = np.zeros_like(K)
        for m, (dy, dx) in enumerate(offsets):
            for c in range(L):
                for x in range(nx):
                    for y in range(ny):
                        if 0 <= y + dy < ny and 0 <= x + dx < nx:
                            p = y + x * ny
                            want[(m * L + c) * N + p, c * N + p] = -planes[m][p]
                            want[(m * L + c) * N + p, c * N + (y + dy) + (x + dx) * ny] = planes[m][p]
        assert np.array_equal(K, want), key
    assert R.matrix(1, 1, 1, R.OFFSETS["w1"], R.ones_weights(1, 1, 8)).nnz == 0
    assert R.matrix(3, 5, 1, [(15, 0), (0, -15)], R.ones_weights(3, 5, 2)).nnz == 0


@pytest.mark.parametrize("case", LIGHT, ids=R.case_id)
def test_restatement_b_equals_matrix_a_on_dyadic_data(case):
    """weights are multiples of 1/8, the data small integers: every difference, product and sum is exact in float32"""
    ny, nx, L, key = case
    offsets = R.OFFSETS[key]
    rng = np.random.default_rng(R.case_seed(case, 1))
    planes = R.dyadic_weights(nx, ny, len(offsets), R.case_seed(case, 10))
    K = R.matrix(nx, ny, L, offsets, planes)
    x, y = rng.integers(-15, 16, K.shape[1]).astype(np.float64), rng.integers(-15, 16, K.shape[0]).astype(np.float64)
    for dtype in (np.float32, np.float64):
        assert np.array_equal(R.product(x, nx, ny, L, offsets, planes, False, dtype).astype(np.float64), K @ x)
        assert np.array_equal(R.product(y, nx, ny, L, offsets, planes, True, dtype).astype(np.float64), K.T @ y)


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_restatement_b_against_matrix_a_adjointness_and_constants(case):
    ny, nx, L, key = case
    offsets = R.OFFSETS[key]
    dtype = np.float64
    rng = np.random.default_rng(R.case_seed(case, 2))
    planes = R.random_weights(nx, ny, len(offsets), R.case_seed(case, 20))
    arg = (nx, ny, L, offsets, planes)
    K = R.matrix(*arg, dtype)
    x, y = rng.standard_normal(K.shape[1]), rng.standard_normal(K.shape[0])
    kx, kty = R.product(x, *arg, False, dtype), R.product(y, *arg, True, dtype)
    bx, by = R.bound(*arg, False, x, dtype), R.bound(*arg, True, y, dtype)
    # the reference product K @ x in float64 has an error of its own of the same kind: the twin's roundings
    tx, ty = R.bound(*arg, False, x, dtype, twin=True), R.bound(*arg, True, y, dtype, twin=True)
    assert kx.shape == (K.shape[0],) and kty.shape == (K.shape[1],)
    assert np.all(np.abs(kx - K @ x) <= tx) and np.all(np.abs(kty - K.T @ y) <= ty)
    assert abs(kx @ y - x @ kty) <= 1.01 * (bx @ np.abs(y) + by @ np.abs(x)) + 4 * np.finfo(dtype).eps * (np.abs(kx) @ np.abs(y) + np.abs(x) @ np.abs(kty))
    res0, res1 = rng.standard_normal(K.shape[0]), rng.standard_normal(K.shape[1])
    assert np.array_equal(R.product(x, *arg, False, dtype, res0), res0 + kx) and np.array_equal(R.product(y, *arg, True, dtype, res1), res1 + kty)
    # K 1 = 0 exactly, for any constant and in both precisions (a negative weight gives w * +0 = -0, which is zero)
    for t in (np.float32, np.float64):
        k1 = R.product(np.full(K.shape[1], 0.3), *arg, False, t)
        assert k1.shape == (K.shape[0],) and not k1.any()


def test_restatement_b_in_float32_against_a_higher_precision_sum_and_the_bound_has_teeth():
    worst = {False: 0.0, True: 0.0}
    for case in LIGHT:
        ny, nx, L, key = case
        offsets = R.OFFSETS[key]
        rng = np.random.default_rng(R.case_seed(case, 3))
        planes = R.random_weights(nx, ny, len(offsets), R.case_seed(case, 30))
        K = R.matrix(nx, ny, L, offsets, planes, np.float32)
        for transpose in (False, True):
            x = rng.standard_normal(K.shape[0] if transpose else K.shape[1]).astype(np.float32).astype(np.float64)
            got = R.product(x, nx, ny, L, offsets, planes, transpose, np.float32).astype(np.float64)
            b = R.bound(nx, ny, L, offsets, planes, transpose, x, np.float32)
            err = np.abs(got - (K.T if transpose else K) @ x)
            assert np.all(err <= b), (case, transpose)
            if (b > 0).any():
                worst[transpose] = max(worst[transpose], float((err[b > 0] / b[b > 0]).max()))
    assert 0.1 < worst[False] <= 1.0 and 0.01 < worst[True] <= 1.0, worst


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("case", LIGHT, ids=R.case_id)
def test_unit_weights_and_the_two_forward_neighbours_are_the_gradient_restatement(case, dtype):
    ny, nx, L, _ = case
    x = np.random.default_rng(R.case_seed(case, 4)).standard_normal(L * nx * ny)
    x[::7] = -0.0
    got, want = R.product(x, nx, ny, L, GRAD, R.ones_weights(nx, ny, 2), False, dtype), R.gradient_product(x, nx, ny, L, dtype)
    assert np.array_equal(got, want) and np.array_equal(np.signbit(got), np.signbit(want))


def masked_everywhere(nx, ny, offsets):
    """[m] -> the positions p whose term m is absent"""
    return [np.flatnonzero(~R.inside(nx, ny, dy, dx).reshape(-1)) for dy, dx in offsets]


def test_an_inf_weight_at_a_masked_position_reaches_no_output():
    nx, ny, L = 5, 4, 2
    offsets = R.OFFSETS["w1"] + [(15, 0), (-3, 4)]
    M = len(offsets)
    planes = R.random_weights(nx, ny, M, 9)
    clean = [p.copy() for p in planes]
    for m, absent in enumerate(masked_everywhere(nx, ny, offsets)):
        planes[m][absent] = np.inf if m % 2 else -np.inf
    assert not np.isfinite(planes[8]).any()                                    # (15, 0) never lands: the whole plane is poisoned
    rng = np.random.default_rng(4)
    x, y = rng.standard_normal(L * nx * ny), rng.standard_normal(M * L * nx * ny)
    for dtype in (np.float32, np.float64):
        for v, transpose in ((x, False), (y, True)):
            got = R.product(v, nx, ny, L, offsets, planes, transpose, dtype)
            assert np.isfinite(got).all() and np.array_equal(got, R.product(v, nx, ny, L, offsets, clean, transpose, dtype))
    # and a NaN in u reaches exactly the outputs of its column of (a), where no weight is zero (the block forms 0 * NaN where one is)
    nonzero = [np.abs(p) + 0.1 for p in clean]
    K = R.matrix(nx, ny, 1, offsets, nonzero)
    x1 = rng.standard_normal(nx * ny)
    x1[7] = np.nan
    hit = np.asarray(abs(K)[:, [7]].sum(axis=1)).ravel() > 0
    assert 5 < hit.sum() < K.shape[0] // 4                                      # its own present terms and those of its neighbours, few rows
    assert np.array_equal(np.isnan(R.product(x1, nx, ny, 1, offsets, nonzero, False, np.float64)), hit)


def nonlocal_problem(nx, ny, L, offsets, planes, alpha):
    """z = K x with only functions that take diagonal steps, so that no preconditioner entry is averaged over a group"""
    bf = prost.block.nonlocal_gradient2d(nx, ny, L, offsets, planes)
    nrows, ncols = bf(0, 0, 0, 0)[1]
    x, z = prost.variable(ncols), prost.variable(nrows)
    prob = prost.min_max_problem([x], [z])
    prob.add_function(x, prost.function.sum_1d("ind_box01"))
    prob.add_function(z, prost.function.sum_1d("ind_box01", 0.5, -0.5))
    prob.add_dual_pair(x, z, bf)
    prob.set_scaling_alpha(alpha)
    return prob


def carried(got, want, carry):
    """the problem takes the reciprocal of a positive sum and carries the last reciprocal over a sum of zero (1 at the start, the rows'
    last value into the columns): -> the positions with a positive sum, and whether every other position holds the carried value"""
    live = want > 0
    previous = np.concatenate([[carry], got[:-1]])
    return live, bool(np.all(got[~live] == previous[~live]))


@pytest.mark.parametrize("precision,dtype", PRECISIONS)
@pytest.mark.parametrize("alpha", [1.0, 2.0])
@pytest.mark.parametrize("case", LIGHT, ids=R.case_id)
def test_preconditioners_within_the_bound_of_the_matrix_sums(precision, dtype, alpha, case):
    """Sigma = 1 / row sums of |K|^alpha, Tau = 1 / column sums of |K|^(2 - alpha); at alpha = 2 the columns count their entries.  Within
    (t + 8) eps_T of (c); rows and columns without entries have a sum of exactly 0 (the problem then carries its last reciprocal on);
    dyadic weights: every sum is exact"""
    ny, nx, L, key = case
    offsets = R.OFFSETS[key]
    tol = (R.sum_terms(len(offsets)) + 8) * np.finfo(dtype).eps
    for dyadic in (True, False):
        planes = (R.dyadic_weights if dyadic else R.random_weights)(nx, ny, len(offsets), R.case_seed(case, 60 + dyadic))
        prost.set_precision(precision)
        try:
            info = prost.problem_info(nonlocal_problem(nx, ny, L, offsets, planes, alpha))
        finally:
            prost.set_precision("double")
        rows = R.sums(nx, ny, L, offsets, planes, alpha, dtype)[0]
        cols = R.sums(nx, ny, L, offsets, planes, 2.0 - alpha, dtype)[1]
        got_left = np.asarray(info["scaling_left"], dtype=np.float64).ravel()
        got_right = np.asarray(info["scaling_right"], dtype=np.float64).ravel()
        carry = 1.0
        for got, want in ((got_left, rows), (got_right, cols)):
            assert got.shape == want.shape
            live, empty_rows_carry = carried(got, want, carry)
            assert empty_rows_carry
            carry = got[-1]
            assert np.all(np.abs(got[live] * want[live] - 1.0) <= tol), float(np.abs(got[live] * want[live] - 1.0).max() / np.finfo(dtype).eps)
            if dyadic:
                assert np.array_equal(got[live], (dtype(1) / want[live].astype(dtype)).astype(np.float64))


def test_the_oracle_solves_the_example_with_the_sparse_twin_and_nltv_beats_tv_at_both_sizes():
    import nltv_denoise as ex
    for nx, ny in ((24, 16), (48, 32)):
        clean, f = ex.striped_image(nx, ny)
        offsets, planes = ex.nonlocal_weights(f, nx, ny)
        M = len(offsets)
        assert M == 48 and offsets.tolist() == [list(o) for o in R.window(3)]
        assert len(planes) == M and all(p.shape == (nx * ny,) and np.isfinite(p).all() and np.all(p >= 0) and np.all(p <= 1) for p in planes)
        kept = np.stack(planes) > 0
        assert 6 <= kept.sum(axis=0).min() and kept.sum(axis=0).max() <= 10                     # the best six and at most four nearest neighbours
        K = ex.spmat_nonlocal_gradient2d(nx, ny, 1, offsets, planes)
        assert abs(K - R.matrix(nx, ny, 1, [tuple(o) for o in offsets.tolist()], planes)).max() == 0
        solve = lambda prob, backend, opts: oracle.solve(prob, backend, opts, np.float64)
        result, img, result_tv, img_tv, f2, clean2 = ex.main(nx, ny, twin=True, verbose=False, solve=solve)
        assert np.array_equal(f2, f) and np.array_equal(clean2, clean)
        assert result["result"] == "Converged." and result_tv["result"] == "Converged." and img.shape == (nx * ny,) and np.isfinite(img).all()
        print("oracle %d x %d: NL-TV %.4f, TV %.4f, data %.4f" % (nx, ny, ex.rmse(img, clean), ex.rmse(img_tv, clean), ex.rmse(f, clean)))
        assert ex.rmse(img, clean) < ex.rmse(img_tv, clean) < ex.rmse(f, clean)


def entry(dtype):
    fn = _hip.fn("linop_nonlocal_gradient2d", dtype)
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, C.c_char_p, C.c_int, C.c_int, C.c_void_p]
    fn.restype = C.c_int
    return fn


def pairs(offsets):
    return np.array(offsets, dtype=np.int8).tobytes()


P16 = C.c_void_p(16)
OK2 = pairs(GRAD)
# res, rhs, weights, nx, ny, L, M, offsets
ABI_REFUSALS = ((P16, P16, P16, 0, 4, 1, 2, OK2), (P16, P16, P16, 4, 0, 1, 2, OK2), (P16, P16, P16, 4, 4, 0, 2, OK2), (P16, P16, P16, 4, 4, 1, 0, OK2),
                (P16, P16, P16, 4, 4, 1, 65, pairs([(1, 0)] * 65)), (P16, P16, P16, 4, 4, 1, -1, OK2), (None, P16, P16, 4, 4, 1, 2, OK2), (P16, None, P16, 4, 4, 1, 2, OK2),
                (P16, P16, None, 4, 4, 1, 2, OK2), (P16, P16, P16, 4, 4, 1, 2, None), (P16, P16, P16, 4, 4, 1, 2, pairs([(0, 1), (16, 0)])),
                (P16, P16, P16, 4, 4, 1, 2, pairs([(0, -16), (1, 0)])), (P16, P16, P16, 4, 4, 1, 2, pairs([(0, 1), (0, 0)])),
                (P16, P16, P16, 2 ** 26, 2 ** 26, 4, 2, OK2), (P16, P16, P16, 2 ** 40, 1, 1, 2, OK2))


def test_header_declares_and_library_exports_the_entry_points_and_they_refuse_without_a_device():
    text = open(os.path.join(ROOT, "include", "prost_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(prost_hip_[a-z0-9_]+)\s*\(", text))
    names = ["prost_hip_linop_nonlocal_gradient2d_f32", "prost_hip_linop_nonlocal_gradient2d_f64"]
    assert not [n for n in names if n not in declared]
    Lb = _hip.lib()
    assert not [n for n in names if not hasattr(Lb, n)]
    assert Lb.prost_hip_abi_version() == 10
    for dtype in (np.float32, np.float64):
        fn = entry(dtype)
        for args in ABI_REFUSALS:
            for transpose in (0, 1):
                assert fn(*args, transpose, 0, None) != 0, args
                assert b"nonlocal_gradient2d" in Lb.prost_hip_last_error()
