"""prost.block.sample2d without a GPU: the builder, the registry name, the creation errors, the preconditioners, the entry points -- and
the definition itself, on the references of tests/sample2d_reference.py.

  * the builder describes { 'sample2d', row, col, { nx, ny, L, x, y } } with its sizes and refuses bad arguments with ValueError;
  * the name is registered for both precisions; every refusal of the factory, by its message, through prost.problem_info;
  * restatement (b) against matrix (a) in both directions: |got - K x| <= 1.01 (t + 1) u (|K| |x|) componentwise, t the number of terms
    of the row or column, u the unit roundoff -- the forward error bound of a t-term sum of rounded products in any order;
    <K x, y> = <x, K^T y> within the same bound carried through the inner products; the accumulating form adds res0 last;
  * integer positions give the identity bit for bit, with Inf in every other pixel;
  * the case list holds every position the definition singles out;
  * the preconditioners of a problem with the block within (t + 8) eps_T of (c); a row or column without an entry sums to exactly 0
    (the problem then repeats the preconditioner in front of it, the reference's rule for an empty row);
  * include/prost_hip.h declares the two entry points, the kernel library exports them, they refuse bad arguments without a device, the
    ABI version is still 10.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import sample2d_reference as R
import prost_amd as prost
from prost_amd import _hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRECISIONS = [("single", np.float32), ("double", np.float64)]


def test_builder_cells_and_sizes():
    xs, ys = [0.0, 1.5, 2.25], [3.0, 0.5, -0.5]
    (name, row, col, data), sz = prost.block.sample2d(6, 5, 2, xs, ys)(3, 7, 0, 0)
    assert (name, row, col) == ("sample2d", 3, 7)
    assert data[:3] == [6, 5, 2] and [type(v) for v in data[:3]] == [int, int, int]
    for got, want in ((data[3], xs), (data[4], ys)):
        assert got.dtype == np.float64 and got.ndim == 1 and np.array_equal(got, want)
    assert len(data) == 5 and sz == [2 * 3, 2 * 5 * 6]
    (_, _, _, data), sz = prost.block.sample2d(np.int64(7), 10.0, 1, np.array([1, 2], np.int32), np.array([0.5, 1e30], np.float32))(0, 0, 0, 0)
    assert data[:3] == [7, 10, 1] and sz == [2, 70] and data[3].dtype == np.float64 and data[4].dtype == np.float64
    assert prost.block.sample2d(1, 1, 1, 0.0, -1.0)(0, 0, 0, 0)[1] == [1, 1]                # a single sample as scalars
    held = np.array([0.0, 1.0])
    bf = prost.block.sample2d(4, 4, 1, held, held)
    held[0] = 99.0                                           # the builder holds its own copy
    assert bf(0, 0, 0, 0)[0][3][3][0] == 0.0 and bf(0, 0, 0, 0)[0][3][4][0] == 0.0
    assert "x = X + dx" in prost.block.sample2d.__doc__       # the docstring says how a warp by a flow is written


def test_builder_value_errors():
    a = [0.0, 1.0]
    for args, message in (((4.5, 4, 1, a, a), "nx = 4.5 is not an integer"), ((4, np.inf, 1, a, a), "not an integer"), ((4, 4, np.nan, a, a), "not an integer"),
                          ((4, 4, True, a, a), "not an integer"), ((4, 4, "1", a, a), "not an integer"), ((None, 4, 1, a, a), "not an integer"),
                          ((0, 4, 1, a, a), "at least 1"), ((4, -2, 1, a, a), "at least 1"), ((4, 4, 0, a, a), "at least 1"),
                          ((16385, 4, 1, a, a), "nx = 16385 has to be at most 16384"), ((4, 16385, 1, a, a), "ny = 16385 has to be at most 16384"),
                          ((4, 4, 1, ["a"], a), "x has to be a vector of numbers"), ((4, 4, 1, a, "ab"), "y has to be a vector of numbers"),
                          ((4, 4, 1, a, None), "y has to be a vector of numbers"), ((4, 4, 1, [True, False], a), "x has to be a vector of numbers"),
                          ((4, 4, 1, a, [1j, 2j]), "y has to be a vector of numbers"),
                          ((4, 4, 1, np.zeros((2, 2)), np.zeros(4)), "x has to be a vector, got shape"), ((4, 4, 1, a, np.zeros((2, 1))), "y has to be a vector, got shape"),
                          ((4, 4, 1, a, [0.0]), "2 x positions and 1 y positions"), ((4, 4, 1, [], a), "0 x positions and 2 y positions"),
                          ((4, 4, 1, [], []), "the positions are empty"),
                          ((4, 4, 1, [0.0, np.nan], a), "non-finite"), ((4, 4, 1, a, [np.inf, 0.0]), "non-finite"), ((4, 4, 1, a, [-np.inf, 0.0]), "non-finite"),
                          ((4, 4, 2 ** 30, a, a), "M = 2 samples on L = 1073741824 planes; M and L M have to stay below 2\\^31")):
        with pytest.raises(ValueError, match=message):
            prost.block.sample2d(*args)
    prost.block.sample2d(16384, 16384, 1, a, a)
    prost.block.sample2d(4, 4, 2 ** 30 - 1, a, a)
    prost.block.sample2d(4, 4, 1, [1e300, -1e300], a)           # finite in float64: a zero row, not an error


@pytest.mark.parametrize("precision", ["single", "double"])
def test_the_name_is_registered(precision):
    prost.set_precision(precision)
    try:
        assert "sample2d" in prost.registered()["block"]
    finally:
        prost.set_precision("double")


def _raw_problem(data, nrows, ncols):
    x, z = prost.variable(ncols), prost.variable(nrows)
    prob = prost.min_max_problem([x], [z])
    prob.add_dual_pair(x, z, lambda row, col, nr, nc: [["sample2d", row, col, data], [nrows, ncols]])
    return prob


@pytest.mark.parametrize("precision", ["single", "double"])
def test_every_refusal_of_the_factory_by_message(precision):
    a, b = np.array([0.0, 1.0, 2.5]), np.array([0.5, -1.0, 3.0])
    cases = [
        ([4.5, 4, 1, a, b], "BlockSample2D: nx = 4.5 has to be an integer from 1 to 16384."),
        ([4, 0, 1, a, b], "BlockSample2D: ny = 0 has to be an integer from 1 to 16384."),
        ([16385, 4, 1, a, b], "BlockSample2D: nx = 16385 has to be an integer from 1 to 16384."),
        ([4, np.nan, 1, a, b], "BlockSample2D: ny = nan has to be an integer from 1 to 16384."),
        ([4, 4, -1, a, b], "BlockSample2D: L = -1 has to be a positive integer below 2^31."),
        ([4, 4, 1.5, a, b], "BlockSample2D: L = 1.5 has to be a positive integer below 2^31."),
        ([4, 4, 2.0 ** 31, a, b], "BlockSample2D: L = 2.14748e+09 has to be a positive integer below 2^31."),
        ([4, 4, 1, a, b[:2]], "BlockSample2D: 3 x positions and 2 y positions."),
        ([4, 4, 1, np.zeros(0), np.zeros(0)], "BlockSample2D: the positions are empty."),
        ([4, 4, 2 ** 30, a, b], "BlockSample2D: M = 3 samples on L = 1.07374e+09 planes; M and L M have to stay below 2^31."),
        ([4, 4, 1, np.array([0.0, np.inf, 1.0]), b], "BlockSample2D: the positions hold a non-finite value."),
        ([4, 4, 1, a, np.array([np.nan, 0.0, 0.0])], "BlockSample2D: the positions hold a non-finite value."),
        ([4, 4, 1, "x", b], "BlockSample2D: the positions have to be full vectors of type single or double."),
        ([4, 4, 1, a, "y"], "BlockSample2D: the positions have to be full vectors of type single or double."),
        ([4, 4, 1, a, b, 3, 15], "BlockSample2D: the declared size 3 x 15 is not L M x L ny nx = 3 x 16."),
        ([4, 4, 2, a, b, 3, 32], "BlockSample2D: the declared size 3 x 32 is not L M x L ny nx = 6 x 32."),
        ([4, 4, 1, a], "BlockSample2D: the data cells are { nx, ny, L, x, y }"),
        ([4, 4, 1, a, b, 3], "BlockSample2D: the data cells are { nx, ny, L, x, y }"),
    ]
    prost.set_precision(precision)
    try:
        for data, message in cases:
            with pytest.raises(prost.ProstError, match=re.escape(message)) as err:
                prost.problem_info(_raw_problem(data, 3, 16))
            assert "Creating block with ID 'sample2d' failed" in str(err.value)
        for data, nrows in (([4, 4, 1, a, b], 3), ([4, 4, 1, a, b, 3, 16], 3), ([4, 4, 1, 0.5, 1.5], 1), ([4, 4, 1, np.array([1e30, 1e300]), np.array([0.0, 0.0])], 2)):
            info = prost.problem_info(_raw_problem(data, nrows, 16))
            assert int(info["nrows"]) == nrows and int(info["ncols"]) == 16
    finally:
        prost.set_precision("double")


def test_the_case_list_holds_what_the_definition_singles_out():
    ms = {len(R.case_args(c)[3]) for c in R.CASES}
    assert {1, 63, 64, 65, 257, R.ONE_CELL_SAMPLES} <= ms and R.ONE_CELL_SAMPLES == 300
    assert {(1, 1), (1, 7), (7, 1), (33, 70)} <= {c[:2] for c in R.CASES} and {64, 65} <= {c[0] for c in R.CASES}
    assert {1, 2, 3} == {c[2] for c in R.CASES}
    seen = set()
    for case in R.CASES:
        nx, ny, L, x, y = R.case_args(case)
        m, n = len(x), nx * ny
        seen.add("M>N" if m > n else ("M<N" if m < n else "M=N"))
        for v, size in ((x, nx), (y, ny)):
            for name, hit in (("integer", (v == np.floor(v)) & (v >= 0) & (v < size)), ("-1", v == -1), ("n-1", v == size - 1), ("(-1,0)", (v > -1) & (v < 0)),
                              ("(n-1,n)", (v > size - 1) & (v < size)), ("just below", (v < -1) & (v > -1.01)), ("just above", (v >= size) & (v < size + 0.01)),
                              ("1e30", v == 1e30)):
                if hit.any():
                    seen.add(name)
        if case[3] == "onecell":
            rows, cols, _, _ = R.entries(nx, ny, x, y, np.float32)
            assert len(set(np.floor(x))) == 1 and len(set(np.floor(y))) == 1 and len(set(cols)) == 4 and len(rows) == 4 * 300
        if case[3] == "flow":
            ident = R.positions("integers", ny, nx, n, 0)
            assert m == n and 4 < max(np.abs(x - ident[0]).max(), np.abs(y - ident[1]).max()) <= 5
    assert seen >= {"M>N", "M<N", "M=N", "integer", "-1", "n-1", "(-1,0)", "(n-1,n)", "just below", "just above", "1e30"}, seen


@pytest.mark.parametrize("prec,dtype", PRECISIONS)
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_restatement_b_against_matrix_a_and_adjointness(prec, dtype, case):
    args = R.case_args(case)
    nx, ny, L = args[:3]
    rng = np.random.default_rng(R.case_seed(case))
    K = R.matrix(*args, dtype)
    assert K.shape == (L * len(args[3]), L * nx * ny)
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
    trow, tcol = R.terms(*args, dtype)
    assert trow.max() <= 4 and np.all(np.asarray(K.sum(axis=1)).ravel() <= 1 + 4 * np.finfo(dtype).eps)      # a row is a partition of at most unity


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_integer_positions_are_the_identity_bit_for_bit(dtype):
    for case in (c for c in R.CASES if c[3] == "integers"):
        args = R.case_args(case)
        nx, ny, L = args[:3]
        K = R.matrix(*args, dtype)
        assert (K != sp.eye(L * nx * ny)).nnz == 0
        v = np.random.default_rng(R.case_seed(case, 1)).standard_normal(L * nx * ny).astype(dtype)
        v[::3] = -0.0
        for transpose in (False, True):
            got = R.product(v, *args, transpose, dtype)
            assert np.array_equal(got, v) and not np.signbit(got[::3]).any()              # +0 + (1)(-0) = +0: the sum starts at +0
    # one sample at an integer position among pixels of Inf: the neighbours' weights are exactly 0, so they are absent and nothing leaks
    img = np.full(5 * 4, np.inf, dtype)
    img[2 + 1 * 5] = 3.0
    assert np.array_equal(R.product(img, 4, 5, 1, [1.0], [2.0], False, dtype), np.array([3.0], dtype))


def sample_problem(args, alpha):
    """z = S x with only functions that take diagonal steps, so that no preconditioner entry is averaged over a group"""
    bf = prost.block.sample2d(*args)
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
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_preconditioners_within_the_bound_of_the_matrix_sums(precision, dtype, alpha, case):
    """Sigma = 1 / row sums of |K|^alpha, Tau = 1 / column sums of |K|^(2 - alpha): within (t + 8) eps_T of (c).  A row or column
    whose sum is exactly 0 repeats the preconditioner in front of it (1 in front of the first row; the last row's in front of the first
    column): a sum that came out as a tiny positive number instead would show as a huge preconditioner."""
    args = R.case_args(case)
    prost.set_precision(precision)
    try:
        info = prost.problem_info(sample_problem(args, alpha))
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
        assert np.array_equal(live, t > 0)
        tol = (t + 8) * np.finfo(dtype).eps
        assert np.all(np.abs(got[live] * want[live] - 1.0) <= tol[live]), float(np.abs(got[live] * want[live] - 1.0).max() / np.finfo(dtype).eps)
        before = np.concatenate([[carry], got[:-1]])
        assert np.array_equal(got[~live], before[~live])
        carry = got[-1]
    if case[3] in ("special", "onecell"):
        assert (rows == 0).any() or case[3] == "onecell"
        assert (cols == 0).any() or case[:2] == (1, 1)


def _entry(dtype):
    fn = _hip.fn("sample2d", dtype)
    fn.argtypes = [C.c_void_p] * 7 + [C.c_int, C.c_void_p]
    fn.restype = C.c_int
    return fn


def test_header_declares_and_library_exports_the_entry_points():
    text = open(os.path.join(ROOT, "include", "prost_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(prost_hip_[a-z0-9_]+)\s*\(", text))
    names = ["prost_hip_sample2d_f32", "prost_hip_sample2d_f64"]
    assert not [n for n in names if n not in declared]
    assert "prost_hip_sample2d_geometry" in text
    Lb = _hip.lib()
    assert not [n for n in names if not hasattr(Lb, n)]
    assert Lb.prost_hip_abi_version() == 10
    assert re.search(r"#define\s+PROST_HIP_ABI_VERSION\s+10\b", text)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_entry_points_refuse_bad_arguments_without_a_device(dtype):
    """every refusal comes before anything touches a device: the pointers are never followed"""
    fn = _entry(dtype)
    good = R.abi_records(4, 4, 1, 5, False)
    p = C.c_void_p(16)
    assert fn(None, p, p, p, p, p, p, 0, None) != 0
    assert b"null geometry" in _hip.lib().prost_hip_last_error()
    for hole in range(6):
        ptrs = [p] * 6
        ptrs[hole] = None
        for transpose in (0, 1):
            rec = good.copy()
            rec[4] = transpose
            assert fn(rec.ctypes.data_as(C.c_void_p), *ptrs, 0, None) != 0
            assert b"null pointer" in _hip.lib().prost_hip_last_error()
    for field, value, message in ((0, 0, b"nx and ny"), (1, 16385, b"nx and ny"), (0, -3, b"nx and ny"), (1, 0, b"nx and ny"), (0, 16385, b"nx and ny"),
                                  (2, 0, b"sample count"), (2, -1, b"sample count"), (2, -2 ** 31, b"sample count"), (3, 0, b"plane count"), (3, -7, b"plane count")):
        for transpose in (0, 1):
            for accumulate in (0, 1):
                bad = good.copy()
                bad[field] = value
                bad[4] = transpose
                assert fn(bad.ctypes.data_as(C.c_void_p), p, p, p, p, p, p, accumulate, None) != 0, (field, value)
                assert message in _hip.lib().prost_hip_last_error(), (field, value, _hip.lib().prost_hip_last_error())
