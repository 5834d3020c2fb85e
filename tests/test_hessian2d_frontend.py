"""prost.block.hessian2d without a GPU: the builder, the registry name, the creation errors, the preconditioners, the entry points -- and
the definition itself, on the references of tests/hessian2d_reference.py.

  * the builder describes { 'hessian2d', row, col, { nx, ny, L, w, components } } with size [components L N, L N] and refuses bad
    arguments with a ValueError that names the argument; the default of w is sqrt(1/2) whatever components is;
  * the name is registered for both precisions; every refusal of the factory, by its message, through prost.problem_info, a wrong
    declared size included;
  * matrix (a) has the entries include/prost/linop/hessian2d.hpp lists: interior rows (1, -2, 1), (1, -2, 1) and the 7-point mixed row
    with centre -2 w, 13 entries per interior pixel; the edges lose the masked terms; a side of 1 empties the rows that cross it;
  * restatement (b) against (a): |(b) - H x| <= 1.01 k u (|H| |x|) componentwise, k = 6 forward, 7 adjoint (8 with components = 4), the
    derived bound of the header, in float64 against the float64 product and in float32 against it (the bound has teeth);
    <H x, y> = <x, H^T y> within the bounds carried through the inner products; absent terms are absent;
  * the CPU oracle running prost.block.sparse of (a) against (b), within the same bound plus the oracle's own (its rows are sums of up
    to t = 7 products, its columns of up to 13 or 20: 1.01 (t + 1) u (|H| |x|));
  * the preconditioners of a problem with the block for alpha = 1 and 0.5 within (7 + 8) eps_T of (c); for w = 0.5 and alpha = 1 every
    sum is exact and the reciprocals are equal;
  * include/prost_hip.h declares the two entry points, the kernel library exports them, they refuse bad arguments without a device,
    and the ABI version is still 10.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import hessian2d_reference as R
import oracle
import prost_amd as prost
from prost_amd import _hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRECISIONS = [("single", np.float32), ("double", np.float64)]
LIGHT = [c for c in R.CASES if c[0] * c[1] * c[2] <= 5000]


def test_builder_cells_and_size():
    (name, row, col, data), sz = prost.block.hessian2d(6, 5, 2, 0.5)(3, 7, 0, 0)
    assert (name, row, col) == ("hessian2d", 3, 7)
    assert data == [6, 5, 2, 0.5, 3] and [type(v) for v in data] == [int, int, int, float, int]
    assert sz == [3 * 2 * 30, 2 * 30]
    (_, _, _, data), sz = prost.block.hessian2d(np.int64(4), 3.0, components=4)(0, 0, 0, 0)
    assert data == [4, 3, 1, float(np.sqrt(0.5)), 4] and [type(v) for v in data] == [int, int, int, float, int] and sz == [48, 12]
    assert prost.block.hessian2d(1, 1)(0, 0, 0, 0)[1] == [3, 1]
    assert prost.block.hessian2d(2, 2, 1, -2, np.int32(4))(0, 0, 0, 0)[0][3] == [2, 2, 1, -2.0, 4]
    with pytest.raises(TypeError):
        prost.block.hessian2d(4, 4, 1, 0.5, 3, False)                      # no label_first argument


def test_builder_value_errors_name_the_argument():
    for args, message in (((4.5, 4), "nx = 4.5 is not an integer"), ((4, np.inf), "ny = inf is not an integer"), ((4, 4, np.nan), "L = nan is not an integer"),
                          ((True, 4), "nx = True is not an integer"), ((4, "4"), "ny = '4' is not an integer"), ((0, 4), "nx = 0 has to be at least 1"),
                          ((4, -2), "ny = -2 has to be at least 1"), ((4, 4, 0), "L = 0 has to be at least 1"),
                          ((4, 4, 1, np.inf), "w = inf is not a finite number"), ((4, 4, 1, np.nan), "w = nan is not a finite number"),
                          ((4, 4, 1, True), "w = True is not a finite number"), ((4, 4, 1, "a"), "w = 'a' is not a finite number"),
                          ((4, 4, 1, 0), "w has to be non-zero"), ((4, 4, 1, -0.0), "w has to be non-zero"),
                          ((4, 4, 1, 0.5, 2), "components = 2 has to be 3 or 4"), ((4, 4, 1, 0.5, 3.5), "components = 3.5 has to be 3 or 4"),
                          ((4, 4, 1, 0.5, True), "components = True has to be 3 or 4"), ((4, 4, 1, 0.5, "3"), "components = '3' has to be 3 or 4"),
                          ((2 ** 26, 2 ** 26, 2), "within 2^53"), ((2 ** 20, 2 ** 20, 2 ** 12), "within 2^53")):
        with pytest.raises(ValueError, match=re.escape(message)) as err:
            prost.block.hessian2d(*args)
        assert str(err.value).startswith("hessian2d: ")
    prost.block.hessian2d(2 ** 26, 2 ** 25, 1)                             # 3 * 2^51 < 2^53
    prost.block.hessian2d(2 ** 25, 2 ** 25, 1, components=4.0)


@pytest.mark.parametrize("precision", ["single", "double"])
def test_the_name_is_registered(precision):
    prost.set_precision(precision)
    try:
        assert "hessian2d" in prost.registered()["block"]
    finally:
        prost.set_precision("double")


def _raw_problem(data, nrows, ncols):
    x, z = prost.variable(ncols), prost.variable(nrows)
    prob = prost.min_max_problem([x], [z])
    prob.add_dual_pair(x, z, lambda row, col, nr, nc: [["hessian2d", row, col, data], [nrows, ncols]])
    return prob


@pytest.mark.parametrize("precision", ["single", "double"])
def test_every_refusal_of_the_factory_by_message(precision):
    cells = "BlockHessian2D: the data cells are { nx, ny, L, w, components } or { nx, ny, L, w, components, nrows, ncols }."
    cases = [
        ([4.5, 4, 1, 0.5, 3], "BlockHessian2D: nx = 4.5 has to be a positive integer."),
        ([4, 0, 1, 0.5, 3], "BlockHessian2D: ny = 0 has to be a positive integer."),
        ([4, 4, -1, 0.5, 3], "BlockHessian2D: L = -1 has to be a positive integer."),
        ([4, 4, np.nan, 0.5, 3], "BlockHessian2D: L = nan has to be a positive integer."),
        ([4, 4, 1, np.inf, 3], "BlockHessian2D: w = inf has to be finite."),
        ([4, 4, 1, np.nan, 3], "BlockHessian2D: w = nan has to be finite."),
        ([4, 4, 1, 0.0, 3], "BlockHessian2D: w has to be non-zero."),
        ([4, 4, 1, 0.5, 2], "BlockHessian2D: components = 2 has to be 3 (hxx, hyy, hxy) or 4 (hxx, hxy, hxy, hyy)."),
        ([4, 4, 1, 0.5, 3.5], "BlockHessian2D: components = 3.5 has to be 3 (hxx, hyy, hxy) or 4 (hxx, hxy, hxy, hyy)."),
        ([4, 4, 1, 0.5, np.nan], "BlockHessian2D: components = nan has to be 3 (hxx, hyy, hxy) or 4 (hxx, hxy, hxy, hyy)."),
        ([2.0 ** 26, 2.0 ** 26, 2, 0.5, 3], "rows; the size has to stay within 2^53."),
        ([4, 4, 1, 0.5, 3, 48, 15], "BlockHessian2D: the declared size 48 x 15 is not components L nx ny x L nx ny = 48 x 16."),
        ([4, 4, 1, 0.5, 4, 48, 16], "BlockHessian2D: the declared size 48 x 16 is not components L nx ny x L nx ny = 64 x 16."),
        ([4, 4, 1, 0.5], cells),
        ([4, 4, 1, 0.5, 3, 48], cells),
    ]
    prost.set_precision(precision)
    try:
        for data, message in cases:
            with pytest.raises(prost.ProstError, match=re.escape(message)) as err:
                prost.problem_info(_raw_problem(data, 48, 16))
            assert "Creating block with ID 'hessian2d' failed" in str(err.value)
        if precision == "single":              # weights that vanish or overflow when rounded to T
            for w in (1e-60, 1e60):
                with pytest.raises(prost.ProstError, match=re.escape("is zero or not finite in single precision.")):
                    prost.problem_info(_raw_problem([4, 4, 1, w, 3], 48, 16))
        for data in ([4, 4, 1, 0.5, 3], [4, 4, 1, 0.5, 3, 48, 16], [2, 2, 3, -1.5, 4]):
            info = prost.problem_info(_raw_problem(data, 48, 16 if data[0] == 4 else 12))
            assert int(info["nrows"]) == 48 and int(info["ncols"]) == (16 if data[0] == 4 else 12)
    finally:
        prost.set_precision("double")


@pytest.mark.parametrize("components", [3, 4])
def test_matrix_a_is_the_list_of_entries_of_the_header(components):
    nx, ny, L, w = 4, 5, 2, 0.25
    N = nx * ny
    H = R.matrix(nx, ny, L, w, components).toarray()
    want = np.zeros_like(H)
    kxx, kyy, kxy = (0, 1, (2,)) if components == 3 else (0, 3, (1, 2))
    for c in range(L):
        for x in range(nx):
            for y in range(ny):
                p, o = y + x * ny, c * N
                ax, bx, ay, by = x < nx - 1, x > 0, y < ny - 1, y > 0
                for plane, entries in ([(kxx, [(-ny, bx), (0, -(ax + bx)), (ny, ax)]), (kyy, [(-1, by), (0, -(ay + by)), (1, ay)])]
                                       + [(k, [(-1, w * (by and ax)), (-1 + ny, -w * (by and ax)), (-ny, w * (bx and ay)), (-ny + 1, -w * (bx and ay)),
                                               (0, -2 * w * (ax and ay)), (1, w * (ax and ay)), (ny, w * (ax and ay))]) for k in kxy]):
                    for d, value in entries:
                        if value:
                            want[(plane * L + c) * N + p, o + p + d] += value
    assert np.array_equal(H, want)
    interior = 2 + 2 * ny                                                   # pixel (2, 2) of channel 0
    assert [np.count_nonzero(H[(k * L) * N + interior]) for k in range(components)] == ([3, 3, 7] if components == 3 else [3, 7, 7, 3])
    assert R.matrix(1, 1, 1, 0.5, components).nnz == 0
    assert R.matrix(1, 6, 1, 0.5, 3).nnz == 3 * 6 - 2 and R.matrix(6, 1, 1, 0.5, 3).nnz == 3 * 6 - 2     # one second difference, no mixed row


@pytest.mark.parametrize("variant", R.VARIANTS + [(3, 0.3)], ids=lambda v: "c%d_w%.3f" % v)
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_restatement_b_against_matrix_a_and_adjointness(case, variant):
    ny, nx, L = case
    components, w = variant
    dtype = np.float64
    rng = np.random.default_rng(R.case_seed(case))
    H = R.matrix(nx, ny, L, w, components, dtype)
    x, y = rng.standard_normal(H.shape[1]), rng.standard_normal(H.shape[0])
    hx = R.product(x, nx, ny, L, w, components, False, dtype)
    hty = R.product(y, nx, ny, L, w, components, True, dtype)
    bx, by = R.bound(nx, ny, L, w, components, False, x, dtype), R.bound(nx, ny, L, w, components, True, y, dtype)
    assert hx.shape == (H.shape[0],) and hty.shape == (H.shape[1],)
    assert np.all(np.abs(hx - H @ x) <= bx) and np.all(np.abs(hty - H.T @ y) <= by)
    assert abs(hx @ y - x @ hty) <= bx @ np.abs(y) + by @ np.abs(x)
    res0, res1 = rng.standard_normal(H.shape[0]), rng.standard_normal(H.shape[1])
    assert np.array_equal(R.product(x, nx, ny, L, w, components, False, dtype, res0), res0 + hx)
    assert np.array_equal(R.product(y, nx, ny, L, w, components, True, dtype, res1), res1 + hty)       # values; the zeros differ (header)


def test_restatement_b_in_float32_against_the_float64_product():
    """the bound has teeth: some element comes within two orders of magnitude of it"""
    worst = 0.0
    for case in LIGHT:
        ny, nx, L = case
        rng = np.random.default_rng(R.case_seed(case, 3))
        for components, w in R.VARIANTS:
            H = R.matrix(nx, ny, L, w, components, np.float32)
            for transpose in (False, True):
                x = rng.standard_normal(H.shape[0] if transpose else H.shape[1]).astype(np.float32).astype(np.float64)
                got = R.product(x, nx, ny, L, w, components, transpose, np.float32).astype(np.float64)
                b = R.bound(nx, ny, L, w, components, transpose, x, np.float32)
                err = np.abs(got - (H.T if transpose else H) @ x)
                assert np.all(err <= b)
                if (b > 0).any():
                    worst = max(worst, float((err[b > 0] / b[b > 0]).max()))
    assert 0.01 < worst <= 1.0, worst


def test_the_zeros_of_the_restatement():
    """0 - s and res - s: a zero sum gives +0 plain and keeps a -0 that was there"""
    got = R.product(np.zeros(9), 3, 3, 1, R.W_FROB, 3, False, np.float32)
    assert not np.signbit(got).any()
    got = R.product(np.zeros(27), 3, 3, 1, R.W_FROB, 3, True, np.float32)
    assert not np.signbit(got).any()
    got = R.product(np.zeros(27), 3, 3, 1, R.W_FROB, 3, True, np.float32, -np.zeros(9))
    assert np.signbit(got).all()
    got = R.product(np.zeros(9), 3, 3, 1, R.W_FROB, 3, False, np.float32, -np.zeros(27))
    assert not np.signbit(got).any()


def test_absent_terms_in_the_restatement():
    """a NaN reaches exactly the outputs of its column of (a), forward; in the adjoint exactly those of its row"""
    nx = ny = 3
    for components, w in R.VARIANTS:
        H = abs(R.matrix(nx, ny, 1, w, components))
        for transpose, n in ((False, H.shape[1]), (True, H.shape[0])):
            M = (H.T if transpose else H).tocsc()
            for at in range(n):
                x = np.random.default_rng(5).standard_normal(n)
                x[at] = np.nan
                got = R.product(x, nx, ny, 1, w, components, transpose, np.float64)
                assert np.array_equal(np.isnan(got), np.asarray(M[:, [at]].sum(axis=1)).ravel() > 0), (components, transpose, at)


@pytest.mark.parametrize("precision,dtype", PRECISIONS)
@pytest.mark.parametrize("case", LIGHT, ids=R.case_id)
def test_the_oracle_with_the_sparse_twin_against_the_restatement(precision, dtype, case):
    ny, nx, L = case
    rng = np.random.default_rng(R.case_seed(case, 2))
    u = np.finfo(dtype).eps / 2
    for components, w in R.VARIANTS:
        H = R.matrix(nx, ny, L, w, components, dtype)
        m, n = H.shape
        if H.nnz == 0:
            continue
        twin = [prost.block.sparse(H)(0, 0, m, n)[0]]
        for transpose in (False, True):
            x = rng.standard_normal(m if transpose else n).astype(dtype).astype(np.float64)
            want = np.asarray(oracle.eval_linop(twin, x, transpose, dtype)[0], dtype=np.float64).ravel()
            got = R.product(x, nx, ny, L, w, components, transpose, dtype).astype(np.float64)
            mag = (abs(H).T if transpose else abs(H)) @ np.abs(x)
            terms = (3 + 3 + 7 * (components - 2)) if transpose else 7            # the longest column / row of (a)
            limit = R.bound(nx, ny, L, w, components, transpose, x, dtype) + 1.01 * (terms + 1) * u * mag
            assert np.all(np.abs(got - want) <= limit)


def hessian_problem(nx, ny, L, w, components, alpha):
    """z = H x with only functions that take diagonal steps, so that no preconditioner entry is averaged over a group"""
    bf = prost.block.hessian2d(nx, ny, L, w, components)
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
@pytest.mark.parametrize("variant", R.VARIANTS, ids=lambda v: "c%d_w%.3f" % v)
@pytest.mark.parametrize("case", LIGHT, ids=R.case_id)
def test_preconditioners_within_the_bound_of_the_matrix_sums(precision, dtype, alpha, variant, case):
    """Sigma = 1 / row sums of |H|^alpha, Tau = 1 / column sums of |H|^(2 - alpha): within (7 + 8) eps_T of (c); rows and columns
    without entries have a sum of exactly 0 (the problem then carries its last reciprocal on); w = 0.5 and alpha = 1: every sum is exact"""
    ny, nx, L = case
    components, w = variant
    tol = (R.SUM_TERMS + 8) * np.finfo(dtype).eps
    prost.set_precision(precision)
    try:
        info = prost.problem_info(hessian_problem(nx, ny, L, w, components, alpha))
    finally:
        prost.set_precision("double")
    rows = R.sums(nx, ny, L, w, components, alpha, dtype)[0]
    cols = R.sums(nx, ny, L, w, components, 2.0 - alpha, dtype)[1]
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
    fn = _hip.fn("hessian2d", dtype)
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_double, C.c_int, C.c_int, C.c_int, C.c_void_p]
    fn.restype = C.c_int
    return fn


def test_header_declares_and_library_exports_the_entry_points_and_they_refuse_without_a_device():
    text = open(os.path.join(ROOT, "include", "prost_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(prost_hip_[a-z0-9_]+)\s*\(", text))
    names = ["prost_hip_hessian2d_f32", "prost_hip_hessian2d_f64"]
    assert not [n for n in names if n not in declared]
    Lb = _hip.lib()
    assert not [n for n in names if not hasattr(Lb, n)]
    assert Lb.prost_hip_abi_version() == 10
    p = C.c_void_p(16)
    for dtype in (np.float32, np.float64):
        fn = entry(dtype)
        for args in ((p, p, 0, 4, 1, 0.5, 3), (p, p, 4, 0, 1, 0.5, 3), (p, p, 4, 4, 0, 0.5, 3), (p, p, 4, 4, 1, np.inf, 3), (p, p, 4, 4, 1, np.nan, 3),
                     (p, p, 4, 4, 1, 0.0, 3), (p, p, 4, 4, 1, 0.5, 2), (p, p, 4, 4, 1, 0.5, 5), (None, p, 4, 4, 1, 0.5, 3), (p, None, 4, 4, 1, 0.5, 4),
                     (p, p, 2 ** 26, 2 ** 26, 2, 0.5, 3)):
            for transpose in (0, 1):
                assert fn(*args, transpose, 0, None) != 0, args
                assert b"hessian2d" in Lb.prost_hip_last_error()
    assert entry(np.float32)(p, p, 4, 4, 1, 1e-60, 3, 0, 0, None) != 0            # zero after rounding to T
    assert entry(np.float32)(p, p, 4, 4, 1, 1e60, 3, 0, 0, None) != 0
