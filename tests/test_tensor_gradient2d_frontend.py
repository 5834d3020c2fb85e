"""prost.block.tensor_gradient2d without a GPU: the builder, the registry name, the creation errors, the preconditioners, the entry
points -- and the definition itself, on the references of tests/tensor_gradient2d_reference.py.

  * the builder describes { 'tensor_gradient2d', row, col, { nx, ny, L, k, tensor } } with size [2 L N, L N] from a (k, N) array, a
    (k, ny, nx) array, a vector (k = 1) or a sequence of k planes, and refuses bad arguments with ValueError;
  * the name is registered for both precisions; every refusal of the factory, by its message, through prost.problem_info: nx, ny, L
    below 1, k outside {1, 2, 3}, a tensor that is not k planes of N values, a value that is not finite after rounding to T, 2 L N beyond
    2^53, a wrong declared size;
  * matrix (a) has the entries of the definition, merged diagonal included;
  * restatement (b) against (a): with dyadic tensors and dyadic data every operation is exact and (b) equals (a) x; in general
    |(b) - (a) x| <= gamma_n B componentwise with the roundings n of the header and B from the UNMERGED absolute values (and the same
    test against |K| |x| with the merged diagonal would fail: shown); <K x, y> = <x, K^T y> within the bound carried through the inner
    products; g = 1 is the gradient restatement bit for bit; the accumulating form adds res0 last; absent terms are absent;
  * the preconditioners of a problem with the block for alpha = 1 and 0.5 within (t + 8) eps_T of (c), exact for dyadic tensors at
    alpha = 1;
  * the oracle solves the problem of examples/tv_edge_weighted.py with the sparse twin, in both modes;
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
import tensor_gradient2d_reference as R
from prost_amd import _hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples"))
PRECISIONS = [("single", np.float32), ("double", np.float64)]
LIGHT = [c for c in R.CASES if c[0] * c[1] * c[2] <= 5000]


def test_builder_cells_and_size():
    t = np.arange(1, 61, dtype=np.float64).reshape(2, 30) / 64
    (name, row, col, data), sz = prost.block.tensor_gradient2d(6, 5, 2, t)(3, 7, 0, 0)
    assert (name, row, col) == ("tensor_gradient2d", 3, 7)
    assert data[:4] == [6, 5, 2, 2] and [type(v) for v in data[:4]] == [int, int, int, int]
    assert data[4].dtype == np.float64 and np.array_equal(data[4], t.reshape(-1)) and sz == [2 * 2 * 30, 2 * 30]
    # a (k, ny, nx) array t[i, y, x]: every plane flattened with y fastest
    t3 = np.arange(90, dtype=np.float64).reshape(3, 5, 6)
    data = prost.block.tensor_gradient2d(6, 5, 1, t3)(0, 0, 0, 0)[0][3]
    assert data[3] == 3 and np.array_equal(data[4], np.concatenate([p.T.reshape(-1) for p in t3]))
    assert data[4][1] == t3[0, 1, 0] and data[4][5] == t3[0, 0, 1]
    # a vector: k = 1; a sequence of planes, vectors or (ny, nx) arrays
    assert prost.block.tensor_gradient2d(np.int64(6), 5.0, 1, np.ones(30))(0, 0, 0, 0)[0][3][3] == 1
    data = prost.block.tensor_gradient2d(6, 5, 1, [np.ones(30), t3[1], 2 * np.ones(30)])(0, 0, 0, 0)[0][3]
    assert data[3] == 3 and np.array_equal(data[4][30:60], t3[1].T.reshape(-1))
    assert prost.block.tensor_gradient2d(1, 1, 1, [0.0])(0, 0, 0, 0)[1] == [2, 1]                   # zeros are legal
    data[4][0] = 99.0                                                                              # the builder copied its input
    assert t3[0, 0, 0] == 0.0
    with pytest.raises(TypeError):
        prost.block.tensor_gradient2d(4, 4, 1, np.ones(16), False)                                 # no label_first argument


def test_builder_value_errors():
    one = np.ones(16)
    for args, message in (((4.5, 4, 1, one), "not an integer"), ((4, np.inf, 1, one), "not an integer"), ((4, 4, np.nan, one), "not an integer"),
                          ((True, 4, 1, one), "not an integer"), ((4, 4, "1", one), "not an integer"),
                          ((0, 4, 1, one), "at least 1"), ((4, -2, 1, one), "at least 1"), ((4, 4, 0, one), "at least 1"),
                          ((4, 4, 1, np.ones((4, 16))), "k = 4 planes"), ((4, 4, 1, [one] * 5), "k = 5 planes"), ((4, 4, 1, np.ones((0, 16))), "k = 0 planes"),
                          ((4, 4, 1, np.ones(15)), "a plane is a vector of nx ny = 16 values"), ((4, 4, 1, np.ones((2, 17))), "a plane is a vector of nx ny = 16 values"),
                          ((4, 4, 1, [one, np.ones(3)]), "plane 1 of the tensor has shape"), ((4, 2, 1, np.ones((3, 4, 2))), "plane 0 of the tensor has shape"),
                          ((4, 4, 1, np.ones((1, 2, 2, 4))), "the tensor has shape"),
                          ((4, 4, 1, "abc"), "array of numbers"), ((4, 4, 1, [one, "a"]), "array of numbers"), ((4, 4, 1, one.astype(complex)), "array of numbers"),
                          ((4, 4, 1, np.r_[one[:15], np.inf]), "non-finite"), ((4, 4, 1, [one, np.r_[np.nan, one[:15]]]), "non-finite"),
                          ((2 ** 26, 2 ** 26, 2, [1.0]), "within 2\\^53"), ((2 ** 20, 2 ** 20, 2 ** 13, [1.0]), "within 2\\^53")):
        with pytest.raises(ValueError, match=message):
            prost.block.tensor_gradient2d(*args)


@pytest.mark.parametrize("precision", ["single", "double"])
def test_the_name_is_registered(precision):
    prost.set_precision(precision)
    try:
        assert "tensor_gradient2d" in prost.registered()["block"]
    finally:
        prost.set_precision("double")


def _raw_problem(data, nrows, ncols):
    x, z = prost.variable(ncols), prost.variable(nrows)
    prob = prost.min_max_problem([x], [z])
    prob.add_dual_pair(x, z, lambda row, col, nr, nc: [["tensor_gradient2d", row, col, data], [nrows, ncols]])
    return prob


@pytest.mark.parametrize("precision", ["single", "double"])
def test_every_refusal_of_the_factory_by_message(precision):
    one, cells = np.ones(16), "BlockTensorGradient2D: the data cells are { nx, ny, L, k, tensor } or { nx, ny, L, k, tensor, nrows, ncols }."
    cases = [
        ([4.5, 4, 1, 1, one], "BlockTensorGradient2D: nx = 4.5 has to be a positive integer."),
        ([4, 0, 1, 1, one], "BlockTensorGradient2D: ny = 0 has to be a positive integer."),
        ([4, 4, -1, 1, one], "BlockTensorGradient2D: L = -1 has to be a positive integer."),
        ([4, 4, np.nan, 1, one], "BlockTensorGradient2D: L = nan has to be a positive integer."),
        ([4, 4, 1, 0, one], "BlockTensorGradient2D: the tensor has k = 0 planes; k has to be 1 (scalar), 2 (per axis) or 3 (symmetric tensor)."),
        ([4, 4, 1, 4, np.ones(64)], "BlockTensorGradient2D: the tensor has k = 4 planes"),
        ([4, 4, 1, 1.5, one], "BlockTensorGradient2D: the tensor has k = 1.5 planes"),
        ([4, 4, 1, 2, one], "BlockTensorGradient2D: the tensor holds 16 values, not k = 2 planes of nx ny = 16."),
        ([4, 4, 1, 1, np.ones(15)], "BlockTensorGradient2D: the tensor holds 15 values, not k = 1 planes of nx ny = 16."),
        ([4, 4, 1, 3, np.ones(49)], "BlockTensorGradient2D: the tensor holds 49 values, not k = 3 planes of nx ny = 16."),
        ([4, 4, 1, 1, np.r_[one[:5], np.inf, one[:10]]], "BlockTensorGradient2D: value 5 of plane 0 of the tensor, inf, is not finite"),
        ([4, 4, 1, 2, np.r_[one, one[:3], np.nan, one[:12]]], "BlockTensorGradient2D: value 3 of plane 1 of the tensor, nan, is not finite"),
        ([2.0 ** 26, 2.0 ** 26, 2, 1, one], "rows; the size has to stay within 2^53."),
        ([4, 4, 1, 1, one, 32, 15], "BlockTensorGradient2D: the declared size 32 x 15 is not 2 L nx ny x L nx ny = 32 x 16."),
        ([4, 4, 2, 1, one, 32, 16], "BlockTensorGradient2D: the declared size 32 x 16 is not 2 L nx ny x L nx ny = 64 x 32."),
        ([4, 4, 1, 1], cells),
        ([4, 4, 1, 1, one, 32], cells),
    ]
    prost.set_precision(precision)
    try:
        for data, message in cases:
            with pytest.raises(prost.ProstError, match=re.escape(message)) as err:
                prost.problem_info(_raw_problem(data, 32, 16))
            assert "Creating block with ID 'tensor_gradient2d' failed" in str(err.value)
        if precision == "single":              # finite as given, infinite when rounded to T
            with pytest.raises(prost.ProstError, match=re.escape("value 2 of plane 0 of the tensor, 1e+60, is not finite in single precision.")):
                prost.problem_info(_raw_problem([4, 4, 1, 1, np.r_[one[:2], 1e60, one[:13]]], 32, 16))
        for data in ([4, 4, 1, 1, one], [4, 4, 1, 3, np.zeros(48), 32, 16], [2, 4, 2, 2, -1.5 * one], [4, 4, 1, 1, 1e-60 * one]):
            info = prost.problem_info(_raw_problem(data, 32, 16))
            assert int(info["nrows"]) == 32 and int(info["ncols"]) == 16
    finally:
        prost.set_precision("double")


def test_matrix_a_is_the_definition():
    """row gx[p]: -(ax a + ay b) at p, ax a at p + ny, ay b at p + 1; row gy[p]: the same with (b, c)"""
    nx, ny, L = 4, 3, 2
    N = nx * ny
    for k in R.MODES:
        planes = R.dyadic_tensor(nx, ny, k, 3 + k)
        a, b, c = R.abc(planes)
        b = np.zeros(N) if b is None else b
        K = R.matrix(nx, ny, L, planes).toarray()
        want = np.zeros_like(K)
        for ch in range(L):
            for x in range(nx):
                for y in range(ny):
                    p = y + x * ny
                    ax, ay = x < nx - 1, y < ny - 1
                    for r, (t0, t1) in ((ch * N + p, (a[p], b[p])), ((L + ch) * N + p, (b[p], c[p]))):
                        want[r, ch * N + p] = -(ax * t0 + ay * t1)
                        if ax: want[r, ch * N + p + ny] = t0
                        if ay: want[r, ch * N + p + 1] = t1
        assert np.array_equal(K, want), k
    assert R.matrix(1, 1, 1, [np.ones(1)]).nnz == 0


@pytest.mark.parametrize("k", R.MODES)
@pytest.mark.parametrize("case", LIGHT, ids=R.case_id)
def test_restatement_b_equals_matrix_a_on_dyadic_data(case, k):
    """tensor entries are multiples of 1/8, the data multiples of 1/16 below 8: every difference, product and sum is exact in float32"""
    ny, nx, L = case
    rng = np.random.default_rng(R.case_seed(case, k))
    planes = R.dyadic_tensor(nx, ny, k, R.case_seed(case, 10 + k))
    K = R.matrix(nx, ny, L, planes)
    x, y = rng.integers(-127, 128, K.shape[1]) / 16.0, rng.integers(-127, 128, K.shape[0]) / 16.0
    for dtype in (np.float32, np.float64):
        assert np.array_equal(R.product(x, nx, ny, L, planes, False, dtype).astype(np.float64), K @ x)
        assert np.array_equal(R.product(y, nx, ny, L, planes, True, dtype).astype(np.float64), K.T @ y)


@pytest.mark.parametrize("k", R.MODES)
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_restatement_b_against_matrix_a_and_adjointness(case, k):
    ny, nx, L = case
    dtype = np.float64
    rng = np.random.default_rng(R.case_seed(case, k))
    planes = R.random_tensor(nx, ny, k, R.case_seed(case, 20 + k))
    K = R.matrix(nx, ny, L, planes, dtype)
    x, y = rng.standard_normal(K.shape[1]), rng.standard_normal(K.shape[0])
    kx, kty = R.product(x, nx, ny, L, planes, False, dtype), R.product(y, nx, ny, L, planes, True, dtype)
    bx, by = R.bound(nx, ny, L, planes, False, x, dtype), R.bound(nx, ny, L, planes, True, y, dtype)
    # the reference product K @ x in float64 has an error of its own of the same kind: the twin's roundings
    tx, ty = R.bound(nx, ny, L, planes, False, x, dtype, twin=True), R.bound(nx, ny, L, planes, True, y, dtype, twin=True)
    assert kx.shape == (K.shape[0],) and kty.shape == (K.shape[1],)
    assert np.all(np.abs(kx - K @ x) <= tx) and np.all(np.abs(kty - K.T @ y) <= ty)
    assert abs(kx @ y - x @ kty) <= 1.01 * (bx @ np.abs(y) + by @ np.abs(x)) + 4 * np.finfo(dtype).eps * (np.abs(kx) @ np.abs(y) + np.abs(x) @ np.abs(kty))
    res0 = rng.standard_normal(K.shape[0])
    assert np.array_equal(R.product(x, nx, ny, L, planes, False, dtype, res0), res0 + kx)
    res1 = rng.standard_normal(K.shape[1])
    assert np.array_equal(R.product(y, nx, ny, L, planes, True, dtype, res1), res1 + kty)


def test_restatement_b_against_a_higher_precision_sum_and_the_merged_bound_is_too_small():
    """(b) in float32 against (a) applied in float64: within gamma_n B, and the bound has teeth (some element comes within two orders of
    magnitude of it).  With a = -b the merged diagonal vanishes: |K| |x| misses the cancellation that the block's roundings see."""
    worst = 0.0
    for case in LIGHT:
        ny, nx, L = case
        rng = np.random.default_rng(R.case_seed(case, 3))
        for k in R.MODES:
            planes = R.random_tensor(nx, ny, k, R.case_seed(case, 30 + k))
            K = R.matrix(nx, ny, L, planes, np.float32)
            for transpose in (False, True):
                x = rng.standard_normal(K.shape[0] if transpose else K.shape[1]).astype(np.float32).astype(np.float64)
                got = R.product(x, nx, ny, L, planes, transpose, np.float32).astype(np.float64)
                b = R.bound(nx, ny, L, planes, transpose, x, np.float32)
                err = np.abs(got - (K.T if transpose else K) @ x)
                assert np.all(err <= b), (case, k, transpose)
                if (b > 0).any():
                    worst = max(worst, float((err[b > 0] / b[b > 0]).max()))
    assert 0.01 < worst <= 1.0, worst
    # b = -a (1 - 2e-6) and data on a checkerboard: the exact gx[p] = -(a + b) u[p] is tiny, the block forms a (-u[p]) + b (-u[p]) from
    # two rounded products.  Its error is within gamma_3 B and far beyond gamma_3 |K| |x| with the merged diagonal.
    nx = ny = 8
    a = 0.3 + np.random.default_rng(1).random(64)
    planes = [a, -a * (1 - 2e-6), a]
    K = R.matrix(nx, ny, 1, planes, np.float32)
    xx, yy = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    x = (np.random.default_rng(2).standard_normal(64).astype(np.float32).astype(np.float64) * ((xx + yy) % 2 == 0).reshape(-1))
    err = np.abs(R.product(x, nx, ny, 1, planes, False, np.float32).astype(np.float64) - K @ x)
    assert np.all(err <= R.bound(nx, ny, 1, planes, False, x, np.float32))
    merged = R.gamma(3, np.float32) * (abs(K) @ np.abs(x))
    assert np.any(err > 10 * merged)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("case", LIGHT, ids=R.case_id)
def test_g_equal_to_one_is_the_gradient_restatement(case, dtype):
    ny, nx, L = case
    rng = np.random.default_rng(R.case_seed(case, 4))
    x, y = rng.standard_normal(L * nx * ny), rng.standard_normal(2 * L * nx * ny)
    x[::7] = -0.0
    ones = R.ones_tensor(nx, ny)
    for v, transpose in ((x, False), (y, True)):
        got, want = R.product(v, nx, ny, L, ones, transpose, dtype), R.gradient_product(v, nx, ny, L, transpose, dtype)
        assert np.array_equal(got, want) and np.array_equal(np.signbit(got), np.signbit(want))


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


def test_absent_terms_in_the_restatement():
    """Inf in the last row and column of the tensor reaches only the outputs whose masks keep those terms; the list for 3 x 3"""
    nx = ny = 3
    x, y = np.random.default_rng(5).standard_normal(9), np.random.default_rng(6).standard_normal(18)
    # p = y + 3 x.  gx[p] keeps a (and, k = 3, b) of p where ax (ay) holds; gy[p] keeps c where ay holds (k = 3: b where ax holds);
    # column p keeps the tensor of p where ax or ay holds, of p - 3 and of p - 1: the poisoned pixels are 2, 5, 6, 7, 8
    want = {(1, False): [2, 5, 9 + 6, 9 + 7], (2, False): [2, 5, 9 + 6, 9 + 7], (3, False): [2, 5, 6, 7, 9 + 2, 9 + 5, 9 + 6, 9 + 7],
            (1, True): [2, 5, 6, 7, 8], (2, True): [2, 5, 6, 7, 8], (3, True): [2, 5, 6, 7, 8]}
    for k in R.MODES:
        planes = poisoned(nx, ny, k)
        for transpose, v in ((False, x), (True, y)):
            hit = reached(nx, ny, planes, transpose)
            assert np.flatnonzero(hit).tolist() == want[(k, transpose)], (k, transpose, np.flatnonzero(hit).tolist())
            got = R.product(v, nx, ny, 1, planes, transpose, np.float64)
            assert np.array_equal(~np.isfinite(got), hit), (k, transpose)
    # only the 1 x 1 grid has an empty column: Inf there reaches nothing; a NaN elsewhere reaches exactly its column
    for k in R.MODES:
        assert R.matrix(1, 1, 1, R.random_tensor(1, 1, k, 1)).nnz == 0
        got = R.product(np.array([np.inf]), 1, 1, 1, R.random_tensor(1, 1, k, 1), False, np.float64)
        assert got.shape == (2,) and not got.any()
        planes = R.random_tensor(nx, ny, k, 50 + k)
        K = R.matrix(nx, ny, 1, planes)
        assert not (np.diff(K.indptr) == 0).any()
        x[4] = np.nan
        got = R.product(x, nx, ny, 1, planes, False, np.float64)
        hit = np.asarray(abs(K)[:, [4]].sum(axis=1)).ravel() > 0
        assert np.flatnonzero(hit).tolist() == ([1, 4, 9 + 3, 9 + 4] if k < 3 else [1, 3, 4, 9 + 1, 9 + 3, 9 + 4])
        assert np.array_equal(np.isnan(got), hit) and np.isfinite(got[~np.isnan(got)]).all()
        x[4] = 0.5


def tensor_problem(nx, ny, L, planes, alpha):
    """z = K x with only functions that take diagonal steps, so that no preconditioner entry is averaged over a group"""
    bf = prost.block.tensor_gradient2d(nx, ny, L, planes)
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
@pytest.mark.parametrize("alpha", [1.0, 0.5])
@pytest.mark.parametrize("k", R.MODES)
@pytest.mark.parametrize("case", LIGHT, ids=R.case_id)
def test_preconditioners_within_the_bound_of_the_matrix_sums(precision, dtype, alpha, k, case):
    """Sigma = 1 / row sums of |K|^alpha, Tau = 1 / column sums of |K|^(2 - alpha): within (t + 8) eps_T of (c); rows and columns without
    entries have a sum of exactly 0 (the problem then carries its last reciprocal on); dyadic tensors and alpha = 1: every sum is exact"""
    ny, nx, L = case
    tol = (R.T_TERMS + 8) * np.finfo(dtype).eps
    for dyadic in (True, False):
        planes = R.dyadic_tensor(nx, ny, k, R.case_seed(case, 60 + k)) if dyadic else R.random_tensor(nx, ny, k, R.case_seed(case, 70 + k))
        prost.set_precision(precision)
        try:
            info = prost.problem_info(tensor_problem(nx, ny, L, planes, alpha))
        finally:
            prost.set_precision("double")
        rows = R.sums(nx, ny, L, planes, alpha, dtype)[0]
        cols = R.sums(nx, ny, L, planes, 2.0 - alpha, dtype)[1]
        got_left = np.asarray(info["scaling_left"], dtype=np.float64).ravel()
        got_right = np.asarray(info["scaling_right"], dtype=np.float64).ravel()
        carry = 1.0
        for got, want in ((got_left, rows), (got_right, cols)):
            assert got.shape == want.shape
            live, empty_rows_carry = carried(got, want, carry)
            assert empty_rows_carry
            carry = got[-1]
            assert np.all(np.abs(got[live] * want[live] - 1.0) <= tol), float(np.abs(got[live] * want[live] - 1.0).max() / np.finfo(dtype).eps)
            if dyadic and alpha == 1.0:
                assert np.array_equal(got[live], (dtype(1) / want[live].astype(dtype)).astype(np.float64))


@pytest.mark.parametrize("mode", ["scalar", "tensor"])
def test_the_oracle_solves_the_example_with_the_sparse_twin(mode):
    import tv_edge_weighted as ex
    nx, ny = 24, 16
    clean, f = ex.step_image(nx, ny, 1)
    planes = ex.edge_tensor(f, nx, ny, 1, mode)
    assert len(planes) == (1 if mode == "scalar" else 3) and all(p.shape == (nx * ny,) and np.isfinite(p).all() for p in planes)
    assert np.all(planes[0] > 0) and np.all(planes[0] <= 1)
    if mode == "tensor":                                   # D^(1/2) is positive definite with eigenvalues g and 1
        a, b, c = planes
        assert np.all(a * c - b * b > 0) and np.all(a + c <= 2.0 + 1e-12)
    K = ex.spmat_tensor_gradient2d(nx, ny, 1, planes)
    assert abs(K - R.matrix(nx, ny, 1, planes)).max() == 0
    prob, backend, opts, u, _, _, _ = ex.describe(nx, ny, 1, mode, f=f, twin=True)
    result = oracle.solve(prob, backend, opts, np.float64)
    img = np.array(u.val, dtype=np.float64).ravel()
    assert result["result"] == "Converged." and img.shape == (nx * ny,) and np.isfinite(img).all()
    assert ex.rmse(img, clean) < ex.rmse(f, clean)


def entry(dtype):
    fn = _hip.fn("linop_tensor_gradient2d", dtype)
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_void_p]
    fn.restype = C.c_int
    return fn


P16 = C.c_void_p(16)
ABI_REFUSALS = ((P16, P16, P16, 0, 4, 1, 1), (P16, P16, P16, 4, 0, 1, 1), (P16, P16, P16, 4, 4, 0, 1), (P16, P16, P16, 4, 4, 1, 0), (P16, P16, P16, 4, 4, 1, 4),
                (P16, P16, P16, 4, 4, 1, -1), (None, P16, P16, 4, 4, 1, 1), (P16, None, P16, 4, 4, 1, 1), (P16, P16, None, 4, 4, 1, 1),
                (P16, P16, P16, 2 ** 26, 2 ** 26, 2, 1))


def test_header_declares_and_library_exports_the_entry_points_and_they_refuse_without_a_device():
    text = open(os.path.join(ROOT, "include", "prost_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(prost_hip_[a-z0-9_]+)\s*\(", text))
    names = ["prost_hip_linop_tensor_gradient2d_f32", "prost_hip_linop_tensor_gradient2d_f64"]
    assert not [n for n in names if n not in declared]
    Lb = _hip.lib()
    assert not [n for n in names if not hasattr(Lb, n)]
    assert Lb.prost_hip_abi_version() == 10
    for dtype in (np.float32, np.float64):
        fn = entry(dtype)
        for args in ABI_REFUSALS:
            for transpose in (0, 1):
                assert fn(*args, transpose, 0, None) != 0, args
                assert b"tensor_gradient2d" in Lb.prost_hip_last_error()
