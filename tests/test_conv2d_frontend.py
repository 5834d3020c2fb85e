"""prost.block.conv2d without a GPU: the builder, the registry name, the creation errors, the preconditioners, the entry points -- and
the definition itself, on the references of tests/conv2d_reference.py.

  * the builder describes { 'conv2d', row, col, { nx, ny, L, kernel, shape } } with the sizes of the three shapes and refuses bad
    arguments with ValueError;
  * the name is registered for both precisions; every refusal of the factory, by its message, through prost.problem_info;
  * matrix (a) for "full" is kron(eye(L), convmtx2(kernel, ny, nx)) of examples/deblurring.py entry for entry; for "same" and "valid"
    it is that matrix with the cropped rows;
  * restatement (b) against (a) in both directions: |got - K x| <= 1.01 (t + 1) u (|K| |x|) componentwise, t the non-zero tap count, u
    the unit roundoff -- the forward error bound of a t-term sum of rounded products in any order; <K x, y> = <x, K^T y> within the
    same bound carried through the inner products; the accumulating form adds res0 last;
  * the preconditioners of a problem with the block (row / column sums from the rectangle table) within (t + 8) eps_T of (c);
  * include/prost_hip.h declares the two entry points, the kernel library exports them, the ABI version is still 10.
"""
import os
import re
import sys

import numpy as np
import pytest
import scipy.sparse as sp

import conv2d_reference as R
import prost_amd as prost
from prost_amd import _hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples"))
PRECISIONS = [("single", np.float32), ("double", np.float64)]


def test_builder_cells_and_sizes_for_the_three_shapes():
    k = np.arange(1.0, 13.0).reshape(3, 4)                  # ky = 3, kx = 4
    for shape, (my, mx) in (("full", (5 + 2, 6 + 3)), ("same", (5, 6)), ("valid", (3, 3))):
        (name, row, col, data), sz = prost.block.conv2d(6, 5, 2, k, shape)(3, 7, 0, 0)
        assert (name, row, col) == ("conv2d", 3, 7)
        assert data[:3] == [6, 5, 2] and [type(v) for v in data[:3]] == [int, int, int] and data[4] == shape
        assert data[3].dtype == np.float64 and data[3].flags.f_contiguous and np.array_equal(data[3], k)
        assert sz == [2 * my * mx, 2 * 5 * 6]
    (_, _, _, data), sz = prost.block.conv2d(np.int64(1), 1.0, 1, [[2.0]])(0, 0, 0, 0)
    assert data[:3] == [1, 1, 1] and data[4] == "full" and sz == [1, 1]
    k[0, 0] = 99.0                                           # the builder holds its own copy
    assert prost.block.conv2d(6, 5, 2, np.ones((3, 4)))(0, 0, 0, 0)[0][3][3][0, 0] == 1.0


def test_builder_value_errors():
    one = np.ones((3, 3))
    for args, message in (((4.5, 4, 1, one), "not an integer"), ((4, np.inf, 1, one), "not an integer"), ((4, 4, np.nan, one), "not an integer"),
                          ((4, 4, 1.5, one), "not an integer"), ((0, 4, 1, one), "at least 1"), ((4, -2, 1, one), "at least 1"), ((4, 4, 0, one), "at least 1"),
                          ((4, 4, 1, np.ones((0, 3))), "non-empty matrix"), ((4, 4, 1, np.ones(3)), "non-empty matrix"), ((4, 4, 1, np.ones((2, 2, 2))), "non-empty matrix"),
                          ((4, 4, 1, np.array([[1.0, np.nan]])), "non-finite"), ((4, 4, 1, np.array([[np.inf]])), "non-finite"),
                          ((4, 4, 1, np.zeros((3, 3))), "no non-zero tap"),
                          ((4, 4, 1, one, "circular"), "unknown shape"), ((4, 4, 1, one, 3), "unknown shape"),
                          ((4, 2, 1, one, "valid"), "larger than the image"), ((2, 4, 1, one, "valid"), "larger than the image"),
                          ((40, 40, 1, np.ones((32, 3))), "up to 31 x 31"), ((40, 40, 1, np.ones((3, 32))), "up to 31 x 31"),
                          ((2 ** 16, 2 ** 15, 1, one), "below 2\\^31"), ((2 ** 16 - 1, 2 ** 15, 1, one, "full"), "below 2\\^31")):
        with pytest.raises(ValueError, match=message):
            prost.block.conv2d(*args)
    prost.block.conv2d(40, 40, 1, np.ones((31, 31)))
    prost.block.conv2d(3, 3, 1, one, "valid")


@pytest.mark.parametrize("precision", ["single", "double"])
def test_the_name_is_registered(precision):
    prost.set_precision(precision)
    try:
        assert "conv2d" in prost.registered()["block"]
    finally:
        prost.set_precision("double")


def _raw_problem(data, nrows, ncols):
    x, z = prost.variable(ncols), prost.variable(nrows)
    prob = prost.min_max_problem([x], [z])
    prob.add_dual_pair(x, z, lambda row, col, nr, nc: [["conv2d", row, col, data], [nrows, ncols]])
    return prob


@pytest.mark.parametrize("precision", ["single", "double"])
def test_every_refusal_of_the_factory_by_message(precision):
    one = np.asfortranarray(np.ones((3, 3)))
    cases = [
        ([4.5, 4, 1, one, "same"], "BlockConv2D: nx = 4.5 has to be a positive integer below 2^31."),
        ([4, 0, 1, one, "same"], "BlockConv2D: ny = 0 has to be a positive integer below 2^31."),
        ([4, 4, -1, one, "same"], "BlockConv2D: L = -1 has to be a positive integer below 2^31."),
        ([4, 4, np.nan, one, "same"], "BlockConv2D: L = nan has to be a positive integer below 2^31."),
        ([4, 4, 1, np.zeros((0, 0)), "same"], "BlockConv2D: the window is empty."),
        ([4, 4, 1, np.asfortranarray([[1.0, np.inf]]), "same"], "BlockConv2D: the window holds a non-finite value."),
        ([4, 4, 1, np.asfortranarray([[np.nan]]), "same"], "BlockConv2D: the window holds a non-finite value."),
        ([4, 4, 1, np.asfortranarray(np.zeros((3, 3))), "same"], "BlockConv2D: the window has no non-zero tap"),
        ([4, 4, 1, one, "circular"], "BlockConv2D: unknown shape 'circular' (full, same or valid)."),
        ([4, 4, 1, one, 2.0], "BlockConv2D: the shape has to be a string (full, same or valid)."),
        ([4, 4, 1, "same", "same"], "BlockConv2D: the window has to be a full matrix of type single or double."),
        ([2, 4, 1, one, "valid"], "BlockConv2D: the window (3 x 3) is larger than the image (4 x 2): the valid part is empty."),
        ([40, 40, 1, np.asfortranarray(np.ones((32, 3))), "same"], "BlockConv2D: the window is 32 x 3, windows up to 31 x 31 are supported."),
        ([40, 40, 1, np.asfortranarray(np.ones((3, 32))), "same"], "BlockConv2D: the window is 3 x 32, windows up to 31 x 31 are supported."),
        ([2 ** 16, 2 ** 15, 1, one, "same"], "BlockConv2D: a plane of 2.14748e+09 elements; it has to stay below 2^31."),
        ([4, 4, 1, one, "same", 16, 15], "BlockConv2D: the declared size 16 x 15 is not L my mx x L ny nx = 16 x 16."),
        ([4, 4, 2, one, "full", 72, 16], "BlockConv2D: the declared size 72 x 16 is not L my mx x L ny nx = 72 x 32."),
        ([4, 4, 1, one], "BlockConv2D: the data cells are { nx, ny, L, kernel, shape }"),
    ]
    prost.set_precision(precision)
    try:
        for data, message in cases:
            with pytest.raises(prost.ProstError, match=re.escape(message)) as err:
                prost.problem_info(_raw_problem(data, 16, 16))
            assert "Creating block with ID 'conv2d' failed" in str(err.value)
        if precision == "single":              # a window that vanishes when rounded to T
            with pytest.raises(prost.ProstError, match=re.escape("BlockConv2D: the window has no non-zero tap in single precision.")):
                prost.problem_info(_raw_problem([4, 4, 1, np.asfortranarray([[1e-60]]), "same"], 16, 16))
        for data, nrows in (([4, 4, 1, one, "same"], 16), ([4, 4, 1, one, "same", 16, 16], 16), ([4, 4, 1, one, "full", 36, 16], 36), ([4, 4, 1, one, "valid"], 4)):
            info = prost.problem_info(_raw_problem(data, nrows, 16))
            assert int(info["nrows"]) == nrows and int(info["ncols"]) == 16
    finally:
        prost.set_precision("double")


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_matrix_a_against_convmtx2(case):
    from deblurring import convmtx2
    ny, nx, L, _, shapes = case
    k = R.case_window(case)
    ky, kx = k.shape
    full = sp.kron(sp.eye(L), convmtx2(k, ny, nx)).tocsc()
    full.eliminate_zeros()                 # scipy's kron stores a dense block in full, explicit zeros included; block.sparse drops them too
    full.sort_indices()
    A = R.matrix(nx, ny, L, k, "full")
    assert A.shape == full.shape and A.nnz == full.nnz
    assert np.array_equal(A.indptr, full.indptr) and np.array_equal(A.indices, full.indices) and np.array_equal(A.data, full.data)
    # "same" and "valid" are the rows of the full convolution at (y + oy, x + ox)
    for shape in shapes:
        (my, mx), (oy, ox) = R.output_size(nx, ny, ky, kx, shape)
        y, x, c = np.meshgrid(np.arange(my), np.arange(mx), np.arange(L), indexing="ij")
        rows = ((y + oy) + (x + ox) * (ny + ky - 1) + c * (ny + ky - 1) * (nx + kx - 1)).transpose(2, 1, 0).reshape(-1)
        assert (R.matrix(nx, ny, L, k, shape) != full.tocsr()[rows]).nnz == 0


@pytest.mark.parametrize("prec,dtype", PRECISIONS)
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_restatement_b_against_matrix_a_and_adjointness(prec, dtype, case):
    ny, nx, L, _, shapes = case
    k = R.case_window(case)
    rng = np.random.default_rng(R.case_seed(case))
    for shape in shapes:
        K = R.matrix(nx, ny, L, k, shape, dtype)
        x = rng.standard_normal(K.shape[1]).astype(dtype).astype(np.float64)
        y = rng.standard_normal(K.shape[0]).astype(dtype).astype(np.float64)
        kx_ = R.product(x, nx, ny, L, k, shape, False, dtype).astype(np.float64)
        kty = R.product(y, nx, ny, L, k, shape, True, dtype).astype(np.float64)
        bx, by = R.bound(nx, ny, L, k, shape, False, x, dtype), R.bound(nx, ny, L, k, shape, True, y, dtype)
        assert kx_.shape == (K.shape[0],) and kty.shape == (K.shape[1],)
        assert np.all(np.abs(kx_ - K @ x) <= bx), float((np.abs(kx_ - K @ x) / np.maximum(bx, 1e-300)).max())
        assert np.all(np.abs(kty - K.T @ y) <= by), float((np.abs(kty - K.T @ y) / np.maximum(by, 1e-300)).max())
        assert abs(kx_ @ y - x @ kty) <= bx @ np.abs(y) + by @ np.abs(x)
        res0 = rng.standard_normal(K.shape[0]).astype(dtype)
        assert np.array_equal(R.product(x, nx, ny, L, k, shape, False, dtype, res0), res0 + kx_.astype(dtype))


def conv_problem(nx, ny, L, k, shape, alpha):
    """z = B x with only functions that take diagonal steps, so that no preconditioner entry is averaged over a group"""
    bf = prost.block.conv2d(nx, ny, L, k, shape)
    nrows, ncols = bf(0, 0, 0, 0)[1]
    x, z = prost.variable(ncols), prost.variable(nrows)
    prob = prost.min_max_problem([x], [z])
    prob.add_function(x, prost.function.sum_1d("ind_box01"))
    prob.add_function(z, prost.function.sum_1d("ind_box01", 0.5, -0.5))
    prob.add_dual_pair(x, z, bf)
    prob.set_scaling_alpha(alpha)
    return prob


@pytest.mark.parametrize("precision,dtype", PRECISIONS)
@pytest.mark.parametrize("alpha", [1.0, 0.5])
@pytest.mark.parametrize("case", [c for c in R.CASES if c[0] * c[1] <= 1500], ids=R.case_id)
def test_preconditioners_within_the_bound_of_the_matrix_sums(precision, dtype, alpha, case):
    """Sigma = 1 / row sums of |K|^alpha, Tau = 1 / column sums of |K|^(2 - alpha): within (t + 8) eps_T of (c)"""
    ny, nx, L, _, shapes = case
    k = R.case_window(case)
    tol = (R.taps(k, dtype) + 8) * np.finfo(dtype).eps
    for shape in shapes:
        prost.set_precision(precision)
        try:
            info = prost.problem_info(conv_problem(nx, ny, L, k, shape, alpha))
        finally:
            prost.set_precision("double")
        rows = R.sums(nx, ny, L, k, shape, alpha, dtype)[0]
        cols = R.sums(nx, ny, L, k, shape, 2.0 - alpha, dtype)[1]
        got_left = np.asarray(info["scaling_left"], dtype=np.float64).ravel()
        got_right = np.asarray(info["scaling_right"], dtype=np.float64).ravel()
        for got, want in ((got_left, rows), (got_right, cols)):
            assert (want > 0).all()              # standard-normal windows: every row and every column holds an entry
            assert np.all(np.abs(got * want - 1.0) <= tol), float(np.abs(got * want - 1.0).max() / np.finfo(dtype).eps)


def test_header_declares_and_library_exports_the_entry_points():
    text = open(os.path.join(ROOT, "include", "prost_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(prost_hip_[a-z0-9_]+)\s*\(", text))
    names = ["prost_hip_conv2d_f32", "prost_hip_conv2d_f64"]
    assert not [n for n in names if n not in declared]
    Lb = _hip.lib()
    assert not [n for n in names if not hasattr(Lb, n)]
    assert Lb.prost_hip_abi_version() == 10
