"""prost.block.conv2d_strided without a GPU: the builder, the registry name, the creation errors, the preconditioners, the entry
points -- and the definition itself, on the references of tests/conv2d_strided_reference.py.

  * the builder describes { 'conv2d_strided', row, col, { nx, ny, L, kernel, shape, sy, sx, py, px } } with the decimated sizes, takes
    stride and phase as an int or a pair (y, x), and refuses bad arguments with ValueError;
  * the name is registered for both precisions; every refusal of the factory, by its message, through prost.problem_info;
  * matrix (a) at stride 1 and phase 0 is conv2d_reference.matrix, at stride s the rows (y sy + py, x sx + px) of it;
  * restatement (b) against (a) in both directions within bound (d); <K x, y> = <x, K^T y> within the same bound carried through the
    inner products; the accumulating form adds res0 last;
  * the preconditioners of a problem with the block (row / column sums from the class table) within (t + 8) eps_T of (c); a row or a
    column without an entry has the sum exactly 0 (the preconditioner then carries its neighbour's value on, as for every block);
  * include/prost_hip.h declares the two entry points, the kernel library exports them, they refuse bad geometry and null pointers
    before anything touches a device, and the ABI version is still 10.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import conv2d_strided_reference as R
import prost_amd as prost
from prost_amd import _hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRECISIONS = [("single", np.float32), ("double", np.float64)]


def test_builder_cells_and_sizes():
    k = np.arange(1.0, 13.0).reshape(3, 4)                  # ky = 3, kx = 4
    # image 9 x 10 (ny = 9, nx = 10): full 11 x 13, same 9 x 10, valid 7 x 7
    for shape, stride, phase, (my, mx) in (("full", 2, 0, (6, 7)), ("full", (3, 2), (2, 1), (3, 6)), ("same", (2, 4), (1, 3), (4, 2)), ("valid", 4, (2, 0), (2, 2)),
                                           ("same", 1, 0, (9, 10)), ("valid", (1, 3), (0, 2), (7, 2))):
        (name, row, col, data), sz = prost.block.conv2d_strided(10, 9, 2, k, stride, shape, phase)(3, 7, 0, 0)
        assert (name, row, col) == ("conv2d_strided", 3, 7)
        assert data[:3] == [10, 9, 2] and data[4] == shape and [type(v) for v in data[:3] + data[5:]] == [int] * 7
        assert tuple(data[5:]) == R.pair(stride) + R.pair(phase)
        assert data[3].dtype == np.float64 and data[3].flags.f_contiguous and np.array_equal(data[3], k)
        assert sz == [2 * my * mx, 2 * 9 * 10], (shape, stride, phase, sz)
        assert prost.block.conv2d_strided_size(10, 9, 3, 4, stride, shape, phase) == (my, mx)
        assert R.output_size(10, 9, 3, 4, shape, stride, phase)[0] == (my, mx)
    (_, _, _, data), sz = prost.block.conv2d_strided(np.int64(5), 4.0, 1, [[2.0]], np.int64(2))(0, 0, 0, 0)
    assert data[:3] == [5, 4, 1] and data[4] == "same" and data[5:] == [2, 2, 0, 0] and sz == [2 * 3, 20]
    k[0, 0] = 99.0                                           # the builder holds its own copy
    assert prost.block.conv2d_strided(6, 5, 2, np.ones((3, 4)), 2)(0, 0, 0, 0)[0][3][3][0, 0] == 1.0


def test_builder_value_errors():
    one = np.ones((3, 3))
    for args, message in (((4.5, 4, 1, one, 2), "not an integer"), ((4, np.inf, 1, one, 2), "not an integer"), ((4, 4, np.nan, one, 2), "not an integer"),
                          ((0, 4, 1, one, 2), "at least 1"), ((4, -2, 1, one, 2), "at least 1"), ((4, 4, 0, one, 2), "at least 1"),
                          ((4, 4, 1, np.ones((0, 3)), 2), "non-empty matrix"), ((4, 4, 1, np.ones(3), 2), "non-empty matrix"),
                          ((4, 4, 1, np.array([[1.0, np.nan]]), 2), "non-finite"), ((4, 4, 1, np.zeros((3, 3)), 2), "no non-zero tap"),
                          ((4, 4, 1, one, 2, "circular"), "unknown shape"), ((4, 4, 1, one, 2, 3), "unknown shape"),
                          ((4, 2, 1, one, 2, "valid"), "larger than the image"), ((40, 40, 1, np.ones((32, 3)), 2), "up to 31 x 31"),
                          ((4, 4, 1, one, 0), "stride sy = 0 has to be 1 .. 4"), ((4, 4, 1, one, (2, 5)), "stride sx = 5 has to be 1 .. 4"), ((4, 4, 1, one, -1), "stride sy = -1"),
                          ((4, 4, 1, one, 1.5), "is not an integer"), ((4, 4, 1, one, (1, 2, 3)), "an integer or a pair"), ((4, 4, 1, one, "2"), "an integer or a pair"),
                          ((4, 4, 1, one, None), "an integer or a pair"), ((4, 4, 1, one, True), "an integer or a pair"), ((4, 4, 1, one, 2, "same", (0, 0.5)), "is not an integer"),
                          ((4, 4, 1, one, 2, "same", 2), "phase py = 2 has to be 0 .. 1"), ((4, 4, 1, one, 2, "same", (0, -1)), "phase px = -1 has to be 0 .. 1"),
                          ((4, 4, 1, one, 4, "valid", (0, 2)), "phase px = 2 has to be 0 .. 1"),            # the valid part is 2 x 2: the size of the convolution binds
                          ((2 ** 16, 2 ** 15, 1, one, 1), "below 2\\^31"), ((1, 2 ** 31 - 1000, 1, [[1.0]], 1), "below 2\\^31 - 1055")):
        with pytest.raises(ValueError, match=message):
            prost.block.conv2d_strided(*args)
    with pytest.raises(ValueError, match="unknown shape"):
        prost.block.conv2d_strided_size(4, 4, 3, 3, 2, "circular")
    prost.block.conv2d_strided(40, 40, 1, np.ones((31, 31)), 4, "same", 3)
    prost.block.conv2d_strided(3, 3, 1, one, (4, 4), "valid")


@pytest.mark.parametrize("precision", ["single", "double"])
def test_the_name_is_registered(precision):
    prost.set_precision(precision)
    try:
        assert "conv2d_strided" in prost.registered()["block"]
    finally:
        prost.set_precision("double")


def _raw_problem(data, nrows, ncols):
    x, z = prost.variable(ncols), prost.variable(nrows)
    prob = prost.min_max_problem([x], [z])
    prob.add_dual_pair(x, z, lambda row, col, nr, nc: [["conv2d_strided", row, col, data], [nrows, ncols]])
    return prob


@pytest.mark.parametrize("precision", ["single", "double"])
def test_every_refusal_of_the_factory_by_message(precision):
    one = np.asfortranarray(np.ones((3, 3)))
    cases = [
        ([4.5, 4, 1, one, "same", 2, 2, 0, 0], "BlockConv2DStrided: nx = 4.5 has to be a positive integer below 2^31."),
        ([4, 0, 1, one, "same", 2, 2, 0, 0], "BlockConv2DStrided: ny = 0 has to be a positive integer below 2^31."),
        ([4, 4, np.nan, one, "same", 2, 2, 0, 0], "BlockConv2DStrided: L = nan has to be a positive integer below 2^31."),
        ([4, 4, 1, np.zeros((0, 0)), "same", 2, 2, 0, 0], "BlockConv2DStrided: the window is empty."),
        ([4, 4, 1, np.asfortranarray([[1.0, np.inf]]), "same", 2, 2, 0, 0], "BlockConv2DStrided: the window holds a non-finite value."),
        ([4, 4, 1, np.asfortranarray(np.zeros((3, 3))), "same", 2, 2, 0, 0], "BlockConv2DStrided: the window has no non-zero tap"),
        ([4, 4, 1, one, "circular", 2, 2, 0, 0], "BlockConv2DStrided: unknown shape 'circular' (full, same or valid)."),
        ([4, 4, 1, one, 2.0, 2, 2, 0, 0], "BlockConv2DStrided: the shape has to be a string (full, same or valid)."),
        ([4, 4, 1, "same", "same", 2, 2, 0, 0], "BlockConv2DStrided: the window has to be a full matrix of type single or double."),
        ([2, 4, 1, one, "valid", 2, 2, 0, 0], "BlockConv2DStrided: the window (3 x 3) is larger than the image (4 x 2): the valid part is empty."),
        ([40, 40, 1, np.asfortranarray(np.ones((32, 3))), "same", 2, 2, 0, 0], "BlockConv2DStrided: the window is 32 x 3, windows up to 31 x 31 are supported."),
        ([4, 4, 1, one, "same", 0, 2, 0, 0], "BlockConv2DStrided: the stride sy = 0 has to be an integer from 1 to 4."),
        ([4, 4, 1, one, "same", 2, 5, 0, 0], "BlockConv2DStrided: the stride sx = 5 has to be an integer from 1 to 4."),
        ([4, 4, 1, one, "same", 1.5, 2, 0, 0], "BlockConv2DStrided: the stride sy = 1.5 has to be an integer from 1 to 4."),
        ([4, 4, 1, one, "same", np.nan, 2, 0, 0], "BlockConv2DStrided: the stride sy = nan has to be an integer from 1 to 4."),
        ([4, 4, 1, one, "same", 2, 2, 2, 0], "BlockConv2DStrided: the phase py = 2 has to be an integer from 0 to 1 (below the stride and the size of the convolution)."),
        ([4, 4, 1, one, "same", 2, 2, 0, -1], "BlockConv2DStrided: the phase px = -1 has to be an integer from 0 to 1"),
        ([4, 4, 1, one, "same", 2, 2, 0.5, 0], "BlockConv2DStrided: the phase py = 0.5 has to be an integer from 0 to 1"),
        ([4, 4, 1, one, "valid", 4, 4, 0, 2], "BlockConv2DStrided: the phase px = 2 has to be an integer from 0 to 1"),
        ([2 ** 16, 2 ** 15, 1, one, "same", 1, 1, 0, 0], "BlockConv2DStrided: a plane of 2.14748e+09 elements; it has to stay below 2^31."),
        ([1, 2 ** 31 - 1000, 1, np.asfortranarray([[1.0]]), "same", 1, 1, 0, 0], "BlockConv2DStrided: a side of 2.14748e+09 pixels; it has to stay below 2^31 - 1055."),
        ([4, 4, 1, one, "same", 2, 2, 0, 0, 4, 15], "BlockConv2DStrided: the declared size 4 x 15 is not L my mx x L ny nx = 4 x 16."),
        ([4, 4, 2, one, "full", 2, 2, 0, 0, 16, 32], "BlockConv2DStrided: the declared size 16 x 32 is not L my mx x L ny nx = 18 x 32."),
        ([4, 4, 1, one, "same"], "BlockConv2DStrided: the data cells are { nx, ny, L, kernel, shape, sy, sx, py, px }"),
        ([4, 4, 1, one, "same", 2, 2, 0, 0, 4], "BlockConv2DStrided: the data cells are { nx, ny, L, kernel, shape, sy, sx, py, px }"),
    ]
    prost.set_precision(precision)
    try:
        for data, message in cases:
            with pytest.raises(prost.ProstError, match=re.escape(message)) as err:
                prost.problem_info(_raw_problem(data, 4, 16))
            assert "Creating block with ID 'conv2d_strided' failed" in str(err.value)
        if precision == "single":              # a window that vanishes when rounded to T
            with pytest.raises(prost.ProstError, match=re.escape("BlockConv2DStrided: the window has no non-zero tap in single precision.")):
                prost.problem_info(_raw_problem([4, 4, 1, np.asfortranarray([[1e-60]]), "same", 2, 2, 0, 0], 4, 16))
        for data, nrows in (([4, 4, 1, one, "same", 2, 2, 0, 0], 4), ([4, 4, 1, one, "same", 2, 2, 1, 1, 4, 16], 4), ([4, 4, 1, one, "full", 2, 2, 0, 0, 9, 16], 9),
                            ([4, 4, 1, one, "valid", 4, 4, 1, 1], 1), ([4, 4, 1, one, "same", 1, 3, 0, 2], 4)):
            info = prost.problem_info(_raw_problem(data, nrows, 16))
            assert int(info["nrows"]) == nrows and int(info["ncols"]) == 16
    finally:
        prost.set_precision("double")


FRONT_CASES = [c for c in R.cases(np.float64) if c[0] * c[1] <= 400]


@pytest.mark.parametrize("case", FRONT_CASES, ids=R.case_id)
def test_matrix_a_is_the_selected_rows_of_the_convolution_matrix(case):
    ny, nx, L, name, stride, phase, shape = case
    assert R.self_check(nx, ny, L, R.make_window(name), shape, stride, phase)
    if stride != (1, 1):
        assert R.self_check(nx, ny, L, R.make_window(name), shape, (1, 1), (0, 0))


@pytest.mark.parametrize("prec,dtype", PRECISIONS)
@pytest.mark.parametrize("case", FRONT_CASES, ids=R.case_id)
def test_restatement_b_against_matrix_a_and_adjointness(prec, dtype, case):
    ny, nx, L, name, stride, phase, shape = case
    k = R.make_window(name)
    arg = (nx, ny, L, k, shape, stride, phase)
    rng = np.random.default_rng(R.case_seed(case))
    K = R.matrix(*arg, dtype)
    x = rng.standard_normal(K.shape[1]).astype(dtype).astype(np.float64)
    y = rng.standard_normal(K.shape[0]).astype(dtype).astype(np.float64)
    kx_ = R.product(x, *arg, False, dtype).astype(np.float64)
    kty = R.product(y, *arg, True, dtype).astype(np.float64)
    bx, by = R.bound(*arg, False, x, dtype), R.bound(*arg, True, y, dtype)
    assert kx_.shape == (K.shape[0],) and kty.shape == (K.shape[1],)
    assert np.all(np.abs(kx_ - K @ x) <= bx), float((np.abs(kx_ - K @ x) / np.maximum(bx, 1e-300)).max())
    assert np.all(np.abs(kty - K.T @ y) <= by), float((np.abs(kty - K.T @ y) / np.maximum(by, 1e-300)).max())
    assert abs(kx_ @ y - x @ kty) <= bx @ np.abs(y) + by @ np.abs(x)
    res0 = rng.standard_normal(K.shape[0]).astype(dtype)
    assert np.array_equal(R.product(x, *arg, False, dtype, res0), res0 + kx_.astype(dtype))
    res1 = rng.standard_normal(K.shape[1]).astype(dtype)
    assert np.array_equal(R.product(y, *arg, True, dtype, res1), res1 + kty.astype(dtype))


def strided_problem(arg, alpha):
    """z = K x with only functions that take diagonal steps, so that no preconditioner entry is averaged over a group"""
    nx, ny, L, k, shape, stride, phase = arg
    bf = prost.block.conv2d_strided(nx, ny, L, k, stride, shape, phase)
    nrows, ncols = bf(0, 0, 0, 0)[1]
    x, z = prost.variable(ncols), prost.variable(nrows)
    prob = prost.min_max_problem([x], [z])
    prob.add_function(x, prost.function.sum_1d("ind_box01"))
    prob.add_function(z, prost.function.sum_1d("ind_box01", 0.5, -0.5))
    prob.add_dual_pair(x, z, bf)
    prob.set_scaling_alpha(alpha)
    return prob


def carried_reciprocals(sums, carry):
    """the preconditioner of a sum vector: 1 / sum, a zero sum carries the value before it on (the rows first, then the columns)"""
    out = np.empty_like(sums)
    for i, s in enumerate(sums):
        if s > 0:
            carry = 1.0 / s
        out[i] = carry
    return out, carry


@pytest.mark.parametrize("precision,dtype", PRECISIONS)
@pytest.mark.parametrize("alpha", [1.0, 0.5])
@pytest.mark.parametrize("case", FRONT_CASES, ids=R.case_id)
def test_preconditioners_within_the_bound_of_the_matrix_sums(precision, dtype, alpha, case):
    """Sigma = 1 / row sums of |K|^alpha, Tau = 1 / column sums of |K|^(2 - alpha): within (t + 8) eps_T of (c).  A pixel no output
    samples (a window smaller than the stride) is a column without an entry: its sum has to be exactly 0, which shows as the carried value"""
    ny, nx, L, name, stride, phase, shape = case
    k = R.make_window(name)
    arg = (nx, ny, L, k, shape, stride, phase)
    tol = (R.taps(k, dtype) + 8) * np.finfo(dtype).eps
    prost.set_precision(precision)
    try:
        info = prost.problem_info(strided_problem(arg, alpha))
    finally:
        prost.set_precision("double")
    rows = R.sums(*arg, alpha, dtype)[0]
    cols = R.sums(*arg, 2.0 - alpha, dtype)[1]
    if name == "1x1" and stride == (4, 4):
        assert (cols == 0).sum() >= cols.size // 2          # the case list holds empty columns
    want_left, carry = carried_reciprocals(rows, 1.0)
    want_right, _ = carried_reciprocals(cols, carry)
    got_left = np.asarray(info["scaling_left"], dtype=np.float64).ravel()
    got_right = np.asarray(info["scaling_right"], dtype=np.float64).ravel()
    for got, want in ((got_left, want_left), (got_right, want_right)):
        assert got.shape == want.shape
        assert np.all(np.abs(got / want - 1.0) <= tol), float(np.abs(got / want - 1.0).max() / np.finfo(dtype).eps)


def test_header_declares_and_library_exports_the_entry_points():
    text = open(os.path.join(ROOT, "include", "prost_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(prost_hip_[a-z0-9_]+)\s*\(", text))
    names = ["prost_hip_conv2d_strided_f32", "prost_hip_conv2d_strided_f64"]
    assert not [n for n in names if n not in declared]
    assert "prost_hip_conv2d_strided_geometry" in text
    Lb = _hip.lib()
    assert not [n for n in names if not hasattr(Lb, n)]
    assert Lb.prost_hip_abi_version() == 10


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_entry_points_refuse_bad_geometry_and_null_pointers_without_a_device(dtype):
    """every check comes before the first call into the HIP runtime: the refusals need no device"""
    fn = _hip.fn("conv2d_strided", dtype)
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    fn.restype = C.c_int
    p = C.c_void_p(16)
    for transpose in (False, True):
        good, _, ntaps = R.abi_records(8, 8, 1, np.ones((3, 3)), "same", (2, 2), (0, 0), transpose, dtype)
        assert good.size == 31 and ntaps == 9
        assert fn(None, None, ntaps, None, None, 0, None) != 0
        assert b"null geometry" in _hip.lib().prost_hip_last_error()
        for args in ((None, p, p), (p, None, p), (p, p, None)):                                       # taps, res, rhs
            assert fn(good.ctypes.data_as(C.c_void_p), args[0], ntaps, args[1], args[2], 0, None) != 0
            assert b"null pointer" in _hip.lib().prost_hip_last_error()
        # field, value: window, stride, phase, offsets, sizes, planes, class table
        for field, value, message in ((6, 32, b"window"), (7, 0, b"window"), (8, 0, b"stride"), (9, 5, b"stride"), (10, 2, b"phase"), (11, -1, b"phase"), (4, 3, b"crop offset"),
                                      (5, -1, b"crop offset"), (0, 0, b"at least 1"), (3, 0, b"at least 1"), (12, 0, b"at least 1"), (14, 1, b"class table"), (30, 8, b"class table"),
                                      (0, 2 ** 31 - 1000, b"2^31")):
            bad = good.copy()
            bad[field] = value
            assert fn(bad.ctypes.data_as(C.c_void_p), p, ntaps, p, p, 0, None) != 0, (field, value)
            assert message in _hip.lib().prost_hip_last_error(), (field, value, _hip.lib().prost_hip_last_error())
        bad = good.copy()
        bad[14 + 3], bad[14 + 4] = 9, 8                                                                # a class table that descends
        if transpose:
            assert fn(bad.ctypes.data_as(C.c_void_p), p, ntaps, p, p, 0, None) != 0 and b"ascend" in _hip.lib().prost_hip_last_error()
        assert fn(good.ctypes.data_as(C.c_void_p), p, 10, p, p, 0, None) != 0                       # more taps than the window has
        assert fn(good.ctypes.data_as(C.c_void_p), p, 0, p, p, 0, None) != 0
