"""prost.block.radon2d without a GPU: the builder, the registry name, the creation errors, the preconditioners, the entry points -- and
the definition itself, on the references of tests/radon2d_reference.py.

  * the builder describes { 'radon2d', row, col, { nx, ny, L, angles, ndet, spacing, shift } } with its sizes and the default detector
    length, and refuses bad arguments with ValueError;
  * the name is registered for both precisions; every refusal of the factory, by its message, through prost.problem_info;
  * restatement (b) against matrix (a) in both directions: |got - K x| <= 1.01 (t + 1) u (|K| |x|) componentwise, t the number of terms
    of the row or column, u the unit roundoff -- the forward error bound of a t-term sum of rounded products in any order;
    <K x, y> = <x, K^T y> within the same bound carried through the inner products; the accumulating form adds res0 last;
  * the matrix is a projector: at the axis angles every column sums to na / spacing, and the constant image projects to its row count;
  * the preconditioners of a problem with the block within (t + 8) eps_T of (c); a row or column without an entry sums to exactly 0
    (the problem then repeats the preconditioner in front of it, the reference's rule for an empty row);
  * include/prost_hip.h declares the two entry points, the kernel library exports them, they refuse bad arguments without a device, the
    ABI version is still 10.
"""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import radon2d_reference as R
import prost_amd as prost
from prost_amd import _hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRECISIONS = [("single", np.float32), ("double", np.float64)]


def test_builder_cells_sizes_and_default_detector():
    angles = [0.0, 0.5, 1.0]
    (name, row, col, data), sz = prost.block.radon2d(6, 5, 2, angles)(3, 7, 0, 0)
    assert (name, row, col) == ("radon2d", 3, 7)
    ndet = 2 * math.ceil(math.hypot(6, 5) / 2) + 1
    assert ndet == 9 and prost.block.radon2d_ndet(6, 5, 1.0) == 9 and prost.block.radon2d_ndet(6, 5) == 9
    assert data[:3] == [6, 5, 2] and [type(v) for v in data[:3]] == [int, int, int]
    assert data[3].dtype == np.float64 and data[3].ndim == 1 and np.array_equal(data[3], angles)
    assert data[4:] == [9, 1.0, 0.0] and type(data[4]) is int and type(data[5]) is float and type(data[6]) is float
    assert sz == [2 * 3 * 9, 2 * 5 * 6]
    (_, _, _, data), sz = prost.block.radon2d(np.int64(7), 10.0, 1, np.array([0.25]), ndet=np.int32(4), spacing=2.5, shift=-0.3)(0, 0, 0, 0)
    assert data[:3] == [7, 10, 1] and data[4:] == [4, 2.5, -0.3] and sz == [4, 70]
    assert prost.block.radon2d(1, 1, 1, 0.0)(0, 0, 0, 0)[1] == [3, 1]                # a single angle as a scalar
    for nx, ny, h in ((1, 1, 1.0), (5, 5, 0.5), (131, 150, 1.0), (7, 10, 2.5), (8192, 8192, 8.0)):
        assert prost.block.radon2d_ndet(nx, ny, h) == R.default_ndet(nx, ny, h)
        assert (R.default_ndet(nx, ny, h) - 1) / 2 * h >= math.hypot(nx, ny) / 2              # the outermost bins lie outside the circumcircle
    held = np.array([0.0, 1.0])
    bf = prost.block.radon2d(4, 4, 1, held)
    held[0] = 99.0                                           # the builder holds its own copy
    assert bf(0, 0, 0, 0)[0][3][3][0] == 0.0


def test_builder_value_errors():
    a = [0.0, 1.0]
    for args, kwargs, message in (((4.5, 4, 1, a), {}, "nx = 4.5 is not an integer"), ((4, np.inf, 1, a), {}, "not an integer"), ((4, 4, np.nan, a), {}, "not an integer"),
                                  ((4, 4, True, a), {}, "not an integer"), ((4, 4, "1", a), {}, "not an integer"),
                                  ((0, 4, 1, a), {}, "at least 1"), ((4, -2, 1, a), {}, "at least 1"), ((4, 4, 0, a), {}, "at least 1"),
                                  ((8193, 4, 1, a), {}, "nx = 8193 has to be at most 8192"), ((4, 8193, 1, a), {}, "ny = 8193 has to be at most 8192"),
                                  ((4, 4, 1, a), {"ndet": 0}, "ndet = 0 has to be at least 1"), ((4, 4, 1, a), {"ndet": 2.5}, "ndet = 2.5 is not an integer"),
                                  ((4, 4, 1, []), {}, "non-empty vector"), ((4, 4, 1, np.zeros((2, 2))), {}, "non-empty vector"),
                                  ((4, 4, 1, ["a"]), {}, "vector of numbers"),
                                  ((4, 4, 1, np.zeros(4097)), {}, "4097 angles, up to 4096"),
                                  ((4, 4, 1, [0.0, np.nan]), {}, "non-finite"), ((4, 4, 1, [np.inf]), {}, "non-finite"),
                                  ((4, 4, 1, a), {"spacing": 0.49}, "spacing = 0.49 has to be from 0.5 to 8"), ((4, 4, 1, a), {"spacing": 8.5}, "from 0.5 to 8"),
                                  ((4, 4, 1, a), {"spacing": np.nan}, "from 0.5 to 8"), ((4, 4, 1, a), {"spacing": "1"}, "spacing = '1' is not a number"),
                                  ((4, 4, 1, a), {"shift": np.inf}, "shift = inf has to be finite"), ((4, 4, 1, a), {"shift": None}, "shift = None is not a number"),
                                  ((4, 4, 1, a), {"ndet": 2 ** 31 - 1024}, "below 2\\^31 - 1024"),
                                  ((4, 4, 1, a), {"ndet": 2 ** 30}, "a sinogram of 2147483648 elements; it has to stay below 2\\^31")):
        with pytest.raises(ValueError, match=message):
            prost.block.radon2d(*args, **kwargs)
    prost.block.radon2d(8192, 8192, 1, np.zeros(4096), spacing=8)
    prost.block.radon2d(4, 4, 1, a, spacing=0.5, ndet=1)


@pytest.mark.parametrize("precision", ["single", "double"])
def test_the_name_is_registered(precision):
    prost.set_precision(precision)
    try:
        assert "radon2d" in prost.registered()["block"]
    finally:
        prost.set_precision("double")


def _raw_problem(data, nrows, ncols):
    x, z = prost.variable(ncols), prost.variable(nrows)
    prob = prost.min_max_problem([x], [z])
    prob.add_dual_pair(x, z, lambda row, col, nr, nc: [["radon2d", row, col, data], [nrows, ncols]])
    return prob


@pytest.mark.parametrize("precision", ["single", "double"])
def test_every_refusal_of_the_factory_by_message(precision):
    a = np.array([0.0, 1.0])
    cases = [
        ([4.5, 4, 1, a, 7, 1.0, 0.0], "BlockRadon2D: nx = 4.5 has to be an integer from 1 to 8192."),
        ([4, 0, 1, a, 7, 1.0, 0.0], "BlockRadon2D: ny = 0 has to be an integer from 1 to 8192."),
        ([8193, 4, 1, a, 7, 1.0, 0.0], "BlockRadon2D: nx = 8193 has to be an integer from 1 to 8192."),
        ([4, np.nan, 1, a, 7, 1.0, 0.0], "BlockRadon2D: ny = nan has to be an integer from 1 to 8192."),
        ([4, 4, -1, a, 7, 1.0, 0.0], "BlockRadon2D: L = -1 has to be a positive integer below 2^31."),
        ([4, 4, 1.5, a, 7, 1.0, 0.0], "BlockRadon2D: L = 1.5 has to be a positive integer below 2^31."),
        ([4, 4, 1, np.zeros(0), 7, 1.0, 0.0], "BlockRadon2D: the angles are empty."),
        ([4, 4, 1, np.zeros(4097), 7, 1.0, 0.0], "BlockRadon2D: 4097 angles, up to 4096 are supported."),
        ([4, 4, 1, np.array([0.0, np.inf]), 7, 1.0, 0.0], "BlockRadon2D: the angles hold a non-finite value."),
        ([4, 4, 1, np.array([np.nan]), 7, 1.0, 0.0], "BlockRadon2D: the angles hold a non-finite value."),
        ([4, 4, 1, "angles", 7, 1.0, 0.0], "BlockRadon2D: the angles have to be a full vector of type single or double."),
        ([4, 4, 1, a, 7, 0.25, 0.0], "BlockRadon2D: spacing = 0.25 has to be from 0.5 to 8."),
        ([4, 4, 1, a, 7, 9.0, 0.0], "BlockRadon2D: spacing = 9 has to be from 0.5 to 8."),
        ([4, 4, 1, a, 7, np.nan, 0.0], "BlockRadon2D: spacing = nan has to be from 0.5 to 8."),
        ([4, 4, 1, a, 7, 1.0, np.inf], "BlockRadon2D: shift = inf has to be finite."),
        ([4, 4, 1, a, 0, 1.0, 0.0], "BlockRadon2D: ndet = 0 has to be a positive integer below 2^31 - 1024."),
        ([4, 4, 1, a, 7.5, 1.0, 0.0], "BlockRadon2D: ndet = 7.5 has to be a positive integer below 2^31 - 1024."),
        ([4, 4, 1, a, 2.0 ** 31, 1.0, 0.0], "BlockRadon2D: ndet = 2.14748e+09 has to be a positive integer below 2^31 - 1024."),
        ([4, 4, 1, a, 2 ** 30, 1.0, 0.0], "BlockRadon2D: a sinogram of 2.14748e+09 elements; it has to stay below 2^31."),
        ([4, 4, 1, a, 7, 1.0, 0.0, 14, 15], "BlockRadon2D: the declared size 14 x 15 is not L na ndet x L ny nx = 14 x 16."),
        ([4, 4, 2, a, 7, 1.0, 0.0, 14, 32], "BlockRadon2D: the declared size 14 x 32 is not L na ndet x L ny nx = 28 x 32."),
        ([4, 4, 1, a, 7, 1.0], "BlockRadon2D: the data cells are { nx, ny, L, angles, ndet, spacing, shift }"),
    ]
    prost.set_precision(precision)
    try:
        for data, message in cases:
            with pytest.raises(prost.ProstError, match=re.escape(message)) as err:
                prost.problem_info(_raw_problem(data, 14, 16))
            assert "Creating block with ID 'radon2d' failed" in str(err.value)
        for data, nrows in (([4, 4, 1, a, 7, 1.0, 0.0], 14), ([4, 4, 1, a, 7, 1.0, 0.0, 14, 16], 14), ([4, 4, 1, a, 1, 8.0, -0.3], 2), ([4, 4, 1, 0.5, 7, 0.5, 0.0], 7)):
            info = prost.problem_info(_raw_problem(data, nrows, 16))
            assert int(info["nrows"]) == nrows and int(info["ncols"]) == 16
    finally:
        prost.set_precision("double")


def test_table_values_at_the_axes_and_the_tie():
    """theta = 0: rows are marched, bin d sits at x = d - cd + cx; pi / 2: columns; pi: rows, mirrored; pi / 4: the tie goes to whichever
    of |cos|, |sin| libm makes larger, and either way c = sqrt(2) and |p| = 1 to an ulp"""
    t = R.table(7, 5, [0.0, math.pi / 2, math.pi, math.pi / 4], 11, 1.0, 0.0, np.float64)
    assert np.array_equal(t[0], [1.0, -0.0, -5.0 + 3.0, 1.0, 0.0])
    assert t[1][4] == 1.0 and t[1][0] == 1.0 and abs(t[1][1]) < 1e-16 and abs(t[1][2] - (-5.0 + 2.0)) < 1e-15 and t[1][3] == 1.0
    assert t[2][4] == 0.0 and t[2][0] == -1.0 and abs(t[2][1]) < 1e-15 and abs(t[2][2] - (5.0 + 3.0)) < 1e-15 and t[2][3] == 1.0
    assert abs(t[3][3] - math.sqrt(2)) < 1e-15 and abs(abs(t[3][1]) - 1) < 1e-15 and abs(t[3][0] - math.sqrt(2)) < 1e-15
    assert t[3][4] == (0.0 if abs(math.cos(math.pi / 4)) >= abs(math.sin(math.pi / 4)) else 1.0)


@pytest.mark.parametrize("prec,dtype", PRECISIONS)
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_restatement_b_against_matrix_a_and_adjointness(prec, dtype, case):
    args = R.case_args(case)
    nx, ny, L = args[:3]
    rng = np.random.default_rng(R.case_seed(case))
    K = R.matrix(*args, dtype)
    assert K.shape == (L * len(args[3]) * args[4], L * nx * ny)
    x = rng.standard_normal(K.shape[1]).astype(dtype).astype(np.float64)
    y = rng.standard_normal(K.shape[0]).astype(dtype).astype(np.float64)
    kx_ = R.product(x, *args, False, dtype).astype(np.float64)
    kty = R.product(y, *args, True, dtype).astype(np.float64)
    bx, by = R.bound(*args, False, x, dtype), R.bound(*args, True, y, dtype)
    assert kx_.shape == (K.shape[0],) and kty.shape == (K.shape[1],)
    assert np.all(np.abs(kx_ - K @ x) <= bx), float((np.abs(kx_ - K @ x) / np.maximum(bx, 1e-300)).max())
    assert np.all(np.abs(kty - K.T @ y) <= by), float((np.abs(kty - K.T @ y) / np.maximum(by, 1e-300)).max())
    assert abs(kx_ @ y - x @ kty) <= bx @ np.abs(y) + by @ np.abs(x)
    res0 = rng.standard_normal(K.shape[0]).astype(dtype)
    assert np.array_equal(R.product(x, *args, False, dtype, res0), res0 + kx_.astype(dtype))
    res0 = rng.standard_normal(K.shape[1]).astype(dtype)
    assert np.array_equal(R.product(y, *args, True, dtype, res0), res0 + kty.astype(dtype))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_the_matrix_is_a_projector(dtype):
    """at the axis angles the bins are 1 / spacing pixels apart, and linear interpolation at a whole number of samples per pixel is a
    partition of unity: with the default detector every column of the matrix sums to na / spacing.  The projection of the constant
    image at theta = 0 is the row count ny in every bin that faces the image, and half of it where a bin looks half a pixel past it."""
    angles = [0.0, math.pi / 2, math.pi]
    for nx, ny, spacing in ((9, 7, 1.0), (7, 10, 0.5)):
        K = R.matrix(nx, ny, 1, angles, R.default_ndet(nx, ny, spacing), spacing, 0.0, dtype)
        col = np.asarray(K.sum(axis=0)).ravel()
        assert np.allclose(col, len(angles) / spacing, rtol=1e-5), (col.min(), col.max())
    K = R.matrix(6, 4, 1, [0.0], 9, 1.0, 0.0, dtype)
    proj = np.asarray(K @ np.ones(24)).ravel()            # cd = 4, cx = 2.5: bin d looks at x = d - 1.5, half way between two columns
    assert np.allclose(proj, [0, 2, 4, 4, 4, 4, 4, 2, 0])


def radon_problem(args, alpha):
    """z = R x with only functions that take diagonal steps, so that no preconditioner entry is averaged over a group"""
    bf = prost.block.radon2d(*args)
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
    """Sigma = 1 / row sums of |K|^alpha, Tau = 1 / column sums of |K|^(2 - alpha): within (t + 8) eps_T of (c).  A row or column
    whose sum is exactly 0 repeats the preconditioner in front of it (1 in front of the first row; the last row's in front of the first
    column): a sum that came out as a tiny positive number instead would show as a huge preconditioner."""
    args = R.case_args(case)
    prost.set_precision(precision)
    try:
        info = prost.problem_info(radon_problem(args, alpha))
    finally:
        prost.set_precision("double")
    rows = R.sums(*args, alpha, dtype)[0]
    cols = R.sums(*args, 2.0 - alpha, dtype)[1]
    trow, tcol = R.terms(*args, dtype)
    got_left = np.asarray(info["scaling_left"], dtype=np.float64).ravel()
    got_right = np.asarray(info["scaling_right"], dtype=np.float64).ravel()
    carry = 1.0
    for got, want, t in ((got_left, rows, trow), (got_right, cols, tcol)):
        assert got.shape == want.shape
        live = want > 0
        tol = (t + 8) * np.finfo(dtype).eps
        assert np.all(np.abs(got[live] * want[live] - 1.0) <= tol[live]), float(np.abs(got[live] * want[live] - 1.0).max() / np.finfo(dtype).eps)
        before = np.concatenate([[carry], got[:-1]])
        assert np.array_equal(got[~live], before[~live])
        carry = got[-1]
    if case[4] in (63, 130) and case[0] < 150:
        assert (rows == 0).any()              # the long detectors have rays that miss the image
    if case[4] == 3:
        assert (cols == 0).any()              # the short one with two angles never sees the corners


def _entry(dtype):
    fn = _hip.fn("radon2d", dtype)
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    fn.restype = C.c_int
    return fn


def test_header_declares_and_library_exports_the_entry_points():
    text = open(os.path.join(ROOT, "include", "prost_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(prost_hip_[a-z0-9_]+)\s*\(", text))
    names = ["prost_hip_radon2d_f32", "prost_hip_radon2d_f64"]
    assert not [n for n in names if n not in declared]
    assert "prost_hip_radon2d_geometry" in text
    Lb = _hip.lib()
    assert not [n for n in names if not hasattr(Lb, n)]
    assert Lb.prost_hip_abi_version() == 10


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_entry_points_refuse_bad_arguments_without_a_device(dtype):
    """every refusal comes before anything touches a device: the pointers are never followed"""
    fn = _entry(dtype)
    good = R.abi_records(4, 4, 1, [0.0, 1.0], 7, 1.0, False)
    p = C.c_void_p(16)
    assert fn(None, None, None, None, 0, None) != 0
    assert b"null geometry" in _hip.lib().prost_hip_last_error()
    for table, res, rhs in ((None, p, p), (p, None, p), (p, p, None)):
        assert fn(good.ctypes.data_as(C.c_void_p), table, res, rhs, 0, None) != 0
        assert b"null pointer" in _hip.lib().prost_hip_last_error()
    for field, value, message in ((0, 0, b"nx and ny"), (1, 8193, b"nx and ny"), (0, -3, b"nx and ny"), (2, 0, b"bin count"), (2, 2 ** 31 - 1024, b"bin count"),
                                  (3, 0, b"angle count"), (3, 4097, b"angle count"), (4, 0, b"plane count"), (5, 0, b"margin"), (5, 3, b"margin"),
                                  (2, 2 ** 30, b"below 2^31 elements")):
        for transpose in (0, 1):
            bad = good.copy()
            bad[field] = value
            bad[6] = transpose
            assert fn(bad.ctypes.data_as(C.c_void_p), p, p, p, 0, None) != 0, (field, value)
            assert message in _hip.lib().prost_hip_last_error(), (field, value, _hip.lib().prost_hip_last_error())
