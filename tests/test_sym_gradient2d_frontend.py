"""prost.block.sym_gradient2d without a GPU: the builder, the registry name, the creation errors, the preconditioners, the entry points
-- and the definition itself, on the references of tests/sym_gradient2d_reference.py.

  * the builder describes { 'sym_gradient2d', row, col, { nx, ny, L, w } } with size [3 L N, 2 L N] and refuses bad arguments with
    ValueError;
  * the name is registered for both precisions; every refusal of the factory, by its message, through prost.problem_info, a wrong
    declared size included;
  * matrix (a) has the entries of the definition: Bx is the backward difference with the boundary handling of the divergence;
  * restatement (b) in float64 against (a): for w a power of two every product is exact and (b) is within (t + 1) u (|E| |x|) with
    t = 3 additions -- a few ulps; in general |got - E x| <= 1.01 (t + 1) u (|E| |x|) componentwise with t = 4, the forward error
    bound of a t-term sum of rounded products; <E x, y> = <x, E^T y> within the same bound carried through the inner products; the
    accumulating form adds res0 last; absent terms are absent (Inf in an empty column reaches nothing);
  * the preconditioners of a problem with the block for alpha = 1 and 0.5 within (t + 8) eps_T of (c); for w = 0.5 and alpha = 1 every
    sum is exact and the reciprocals are equal;
  * include/prost_hip.h declares the two entry points, the kernel library exports them, they refuse bad arguments without a device,
    and the ABI version is still 10.
"""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

import prost_amd as prost
import sym_gradient2d_reference as R
from prost_amd import _hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples"))
PRECISIONS = [("single", np.float32), ("double", np.float64)]
LIGHT = [c for c in R.CASES if c[0] * c[1] * c[2] <= 5000]


def test_builder_cells_and_size():
    (name, row, col, data), sz = prost.block.sym_gradient2d(6, 5, 2, 0.5)(3, 7, 0, 0)
    assert (name, row, col) == ("sym_gradient2d", 3, 7)
    assert data == [6, 5, 2, 0.5] and [type(v) for v in data] == [int, int, int, float]
    assert sz == [3 * 2 * 30, 2 * 2 * 30]
    (_, _, _, data), sz = prost.block.sym_gradient2d(np.int64(4), 3.0)(0, 0, 0, 0)
    assert data == [4, 3, 1, float(np.sqrt(0.5))] and [type(v) for v in data] == [int, int, int, float] and sz == [36, 24]
    assert prost.block.sym_gradient2d(1, 1)(0, 0, 0, 0)[1] == [3, 2]
    assert prost.block.sym_gradient2d(2, 2, 1, -2)(0, 0, 0, 0)[0][3] == [2, 2, 1, -2.0]
    with pytest.raises(TypeError):
        prost.block.sym_gradient2d(4, 4, 1, 0.5, False)                    # no label_first argument


def test_builder_value_errors():
    for args, message in (((4.5, 4), "not an integer"), ((4, np.inf), "not an integer"), ((4, 4, np.nan), "not an integer"), ((4, 4, 1.5), "not an integer"),
                          ((True, 4), "not an integer"), ((4, False), "not an integer"), ((4, 4, True), "not an integer"), (("4", 4), "not an integer"),
                          ((0, 4), "at least 1"), ((4, -2), "at least 1"), ((4, 4, 0), "at least 1"),
                          ((4, 4, 1, np.inf), "not a finite number"), ((4, 4, 1, np.nan), "not a finite number"), ((4, 4, 1, True), "not a finite number"),
                          ((4, 4, 1, "a"), "not a finite number"), ((4, 4, 1, 0), "non-zero"), ((4, 4, 1, -0.0), "non-zero"),
                          ((2 ** 26, 2 ** 26, 2), "within 2\\^53"), ((2 ** 20, 2 ** 20, 2 ** 12), "within 2\\^53")):
        with pytest.raises(ValueError, match=message):
            prost.block.sym_gradient2d(*args)
    prost.block.sym_gradient2d(2 ** 26, 2 ** 25, 1)                        # 3 * 2^51 < 2^53


@pytest.mark.parametrize("precision", ["single", "double"])
def test_the_name_is_registered(precision):
    prost.set_precision(precision)
    try:
        assert "sym_gradient2d" in prost.registered()["block"]
    finally:
        prost.set_precision("double")


def _raw_problem(data, nrows, ncols):
    x, z = prost.variable(ncols), prost.variable(nrows)
    prob = prost.min_max_problem([x], [z])
    prob.add_dual_pair(x, z, lambda row, col, nr, nc: [["sym_gradient2d", row, col, data], [nrows, ncols]])
    return prob


@pytest.mark.parametrize("precision", ["single", "double"])
def test_every_refusal_of_the_factory_by_message(precision):
    cases = [
        ([4.5, 4, 1, 0.5], "BlockSymGradient2D: nx = 4.5 has to be a positive integer."),
        ([4, 0, 1, 0.5], "BlockSymGradient2D: ny = 0 has to be a positive integer."),
        ([4, 4, -1, 0.5], "BlockSymGradient2D: L = -1 has to be a positive integer."),
        ([4, 4, np.nan, 0.5], "BlockSymGradient2D: L = nan has to be a positive integer."),
        ([4, 4, 1, np.inf], "BlockSymGradient2D: w = inf has to be finite."),
        ([4, 4, 1, np.nan], "BlockSymGradient2D: w = nan has to be finite."),
        ([4, 4, 1, 0.0], "BlockSymGradient2D: w has to be non-zero."),
        ([2.0 ** 26, 2.0 ** 26, 2, 0.5], "rows; the size has to stay within 2^53."),
        ([4, 4, 1, 0.5, 48, 31], "BlockSymGradient2D: the declared size 48 x 31 is not 3 L nx ny x 2 L nx ny = 48 x 32."),
        ([4, 4, 2, 0.5, 48, 32], "BlockSymGradient2D: the declared size 48 x 32 is not 3 L nx ny x 2 L nx ny = 96 x 64."),
        ([4, 4, 1], "BlockSymGradient2D: the data cells are { nx, ny, L, w } or { nx, ny, L, w, nrows, ncols }."),
        ([4, 4, 1, 0.5, 48], "BlockSymGradient2D: the data cells are { nx, ny, L, w } or { nx, ny, L, w, nrows, ncols }."),
    ]
    prost.set_precision(precision)
    try:
        for data, message in cases:
            with pytest.raises(prost.ProstError, match=re.escape(message)) as err:
                prost.problem_info(_raw_problem(data, 48, 32))
            assert "Creating block with ID 'sym_gradient2d' failed" in str(err.value)
        if precision == "single":              # weights that vanish or overflow when rounded to T
            for w in (1e-60, 1e60):
                with pytest.raises(prost.ProstError, match=re.escape("is zero or not finite in single precision.")):
                    prost.problem_info(_raw_problem([4, 4, 1, w], 48, 32))
        for data in ([4, 4, 1, 0.5], [4, 4, 1, 0.5, 48, 32], [2, 4, 2, -1.5]):
            info = prost.problem_info(_raw_problem(data, 48, 32))
            assert int(info["nrows"]) == 48 and int(info["ncols"]) == 32
    finally:
        prost.set_precision("double")


def test_matrix_a_is_the_definition():
    """(Bx v)(y, x) = [x < nx-1] v(y, x) - [x > 0] v(y, x-1), By the same along y; the mixed rows carry w"""
    nx, ny, L, w = 4, 3, 2, 0.25
    N = nx * ny
    E = R.matrix(nx, ny, L, w).toarray()
    want = np.zeros_like(E)
    for c in range(L):
        for x in range(nx):
            for y in range(ny):
                p = y + x * ny
                ax, bx, ay, by = x < nx - 1, x > 0, y < ny - 1, y > 0
                if bx: want[c * N + p, c * N + p - ny] -= 1
                if ax: want[c * N + p, c * N + p] += 1
                if by: want[(L + c) * N + p, (L + c) * N + p - 1] -= 1
                if ay: want[(L + c) * N + p, (L + c) * N + p] += 1
                if by: want[(2 * L + c) * N + p, c * N + p - 1] -= w
                if ay: want[(2 * L + c) * N + p, c * N + p] += w
                if bx: want[(2 * L + c) * N + p, (L + c) * N + p - ny] -= w
                if ax: want[(2 * L + c) * N + p, (L + c) * N + p] += w
    assert np.array_equal(E, want)
    assert R.matrix(1, 1, 1, 0.5).nnz == 0
    assert np.array_equal(R.empty_columns(3, 3, 1), [8, 17])


@pytest.mark.parametrize("w", [R.W_HALF, R.W_FROB, -2.0, 0.3])
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_restatement_b_against_matrix_a_and_adjointness(case, w):
    ny, nx, L = case
    dtype = np.float64
    rng = np.random.default_rng(R.case_seed(case))
    E = R.matrix(nx, ny, L, w, dtype)
    x, y = rng.standard_normal(E.shape[1]), rng.standard_normal(E.shape[0])
    ex = R.product(x, nx, ny, L, w, False, dtype)
    ety = R.product(y, nx, ny, L, w, True, dtype)
    bx, by = R.bound(nx, ny, L, w, False, x, dtype), R.bound(nx, ny, L, w, True, y, dtype)
    if np.log2(abs(w)) % 1 == 0:                 # the products are exact: three additions remain, a few ulps of |E| |x|
        bx, by = bx * 4 / 5, by * 4 / 5
    assert ex.shape == (E.shape[0],) and ety.shape == (E.shape[1],)
    assert np.all(np.abs(ex - E @ x) <= bx) and np.all(np.abs(ety - E.T @ y) <= by)
    assert abs(ex @ y - x @ ety) <= bx @ np.abs(y) + by @ np.abs(x)
    res0 = rng.standard_normal(E.shape[0])
    assert np.array_equal(R.product(x, nx, ny, L, w, False, dtype, res0), res0 + ex)


def test_restatement_b_against_a_higher_precision_sum():
    """(b) in float32 against (a) applied in float64: the bound has teeth (some element comes within two orders of magnitude of it)"""
    worst = 0.0
    for case in LIGHT:
        ny, nx, L = case
        rng = np.random.default_rng(R.case_seed(case, 3))
        for w in (R.W_HALF, R.W_FROB):
            E = R.matrix(nx, ny, L, w, np.float32)
            for transpose in (False, True):
                x = rng.standard_normal(E.shape[0] if transpose else E.shape[1]).astype(np.float32).astype(np.float64)
                got = R.product(x, nx, ny, L, w, transpose, np.float32).astype(np.float64)
                b = R.bound(nx, ny, L, w, transpose, x, np.float32)
                err = np.abs(got - (E.T if transpose else E) @ x)
                assert np.all(err <= b)
                if (b > 0).any():
                    worst = max(worst, float((err[b > 0] / b[b > 0]).max()))
    assert 0.01 < worst <= 1.0, worst


def test_absent_terms_in_the_restatement():
    nx = ny = 3
    x = np.random.default_rng(5).standard_normal(18)
    x[R.empty_columns(3, 3, 1)] = np.inf
    got = R.product(x, nx, ny, 1, R.W_FROB, False, np.float64)
    assert np.isfinite(got).all()
    x[4] = np.nan
    got = R.product(x, nx, ny, 1, R.W_FROB, False, np.float64)
    E = R.matrix(nx, ny, 1, R.W_FROB)
    assert np.array_equal(np.isnan(got), np.asarray(abs(E)[:, [4]].sum(axis=1)).ravel() > 0) and np.isfinite(got[~np.isnan(got)]).all()


def sym_problem(nx, ny, L, w, alpha):
    """z = E x with only functions that take diagonal steps, so that no preconditioner entry is averaged over a group"""
    bf = prost.block.sym_gradient2d(nx, ny, L, w)
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
@pytest.mark.parametrize("w", [R.W_HALF, R.W_FROB])
@pytest.mark.parametrize("case", LIGHT, ids=R.case_id)
def test_preconditioners_within_the_bound_of_the_matrix_sums(precision, dtype, alpha, w, case):
    """Sigma = 1 / row sums of |E|^alpha, Tau = 1 / column sums of |E|^(2 - alpha): within (t + 8) eps_T of (c); rows and columns
    without entries have a sum of exactly 0 (the problem then carries its last reciprocal on); w = 0.5 and alpha = 1: every sum is exact"""
    ny, nx, L = case
    tol = (R.T_TERMS + 8) * np.finfo(dtype).eps
    prost.set_precision(precision)
    try:
        info = prost.problem_info(sym_problem(nx, ny, L, w, alpha))
    finally:
        prost.set_precision("double")
    rows = R.sums(nx, ny, L, w, alpha, dtype)[0]
    cols = R.sums(nx, ny, L, w, 2.0 - alpha, dtype)[1]
    got_left = np.asarray(info["scaling_left"], dtype=np.float64).ravel()
    got_right = np.asarray(info["scaling_right"], dtype=np.float64).ravel()
    carry = 1.0
    for got, want in ((got_left, rows), (got_right, cols)):
        assert got.shape == want.shape
        live, empty_rows_carry = carried(got, want, carry)
        assert empty_rows_carry
        carry = got[-1]
        assert np.all(np.abs(got[live] * want[live] - 1.0) <= tol), float(np.abs(got[live] * want[live] - 1.0).max() / np.finfo(dtype).eps)
        if w == R.W_HALF and alpha == 1.0:
            assert np.array_equal(got[live], (dtype(1) / want[live].astype(dtype)).astype(np.float64))


def entry(dtype):
    fn = _hip.fn("linop_sym_gradient2d", dtype)
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_double, C.c_int, C.c_int, C.c_void_p]
    fn.restype = C.c_int
    return fn


def test_header_declares_and_library_exports_the_entry_points_and_they_refuse_without_a_device():
    text = open(os.path.join(ROOT, "include", "prost_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(prost_hip_[a-z0-9_]+)\s*\(", text))
    names = ["prost_hip_linop_sym_gradient2d_f32", "prost_hip_linop_sym_gradient2d_f64"]
    assert not [n for n in names if n not in declared]
    Lb = _hip.lib()
    assert not [n for n in names if not hasattr(Lb, n)]
    assert Lb.prost_hip_abi_version() == 10
    p = C.c_void_p(16)
    for dtype in (np.float32, np.float64):
        fn = entry(dtype)
        for args in ((p, p, 0, 4, 1, 0.5), (p, p, 4, 0, 1, 0.5), (p, p, 4, 4, 0, 0.5), (p, p, 4, 4, 1, np.inf), (p, p, 4, 4, 1, np.nan), (p, p, 4, 4, 1, 0.0),
                     (None, p, 4, 4, 1, 0.5), (p, None, 4, 4, 1, 0.5), (p, p, 2 ** 26, 2 ** 26, 2, 0.5)):
            for transpose in (0, 1):
                assert fn(*args, transpose, 0, None) != 0, args
                assert b"sym_gradient2d" in Lb.prost_hip_last_error()
    assert entry(np.float32)(p, p, 4, 4, 1, 1e-60, 0, 0, None) != 0            # zero after rounding to T
    assert entry(np.float32)(p, p, 4, 4, 1, 1e60, 0, 0, None) != 0
