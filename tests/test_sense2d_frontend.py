"""prost.block.sense2d without a GPU: the builder, the registry name, the creation errors, the bound sums, the entry points -- and the
definition itself, on the references of tests/sense2d_reference.py.

  * the builder describes { 'sense2d', row, col, { nx, ny, L, C, maps } } with its sizes, gives the same description for every accepted
    form of the maps, and refuses bad arguments with ValueError;
  * the name is registered for both precisions; every refusal of the factory, by its message, through prost.problem_info; declared sizes;
  * restatement (a) against the float64 operator (c) within the bounds (e) (doubled in fp64, where the comparator is itself float64
    arithmetic) and against the explicit matrix (b); <K x, y> = <x, K^T y>; the accumulating form adds res0 last;
  * the bound sums (d) against the explicit matrix at (nx, ny, C) in {(4, 2, 1), (4, 8, 3), (8, 8, 2)}, e in {0.5, 1, 1.5, 2}, maps with
    zeros: S <= Sbar (1 + 16 eps), Sbar <= 2^|1 - e/2| S (1 + 16 eps), at e = 2 equality within (C + 8) eps; the preconditioners of a
    problem with the block against (d) within (C + 8) eps_T;
  * include/prost_hip.h declares the entry points, the kernel library exports them, they refuse bad arguments without a device, the ABI
    version is still 10.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import sense2d_reference as R
import prost_amd as prost
from prost_amd import _hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRECISIONS = [("single", np.float32), ("double", np.float64)]
SMALL = [c for c in R.CASES if 2 * c[2] * c[3] * c[0] * c[1] <= 2 ** 16]


def test_builder_cells_sizes_and_every_form_of_the_maps():
    case = nx, ny, L, Cn = (8, 4, 2, 3)
    N = nx * ny
    m = R.make_maps(case, zeros=True)                                   # (C, N), p = y + x ny
    (name, row, col, data), sz = prost.block.sense2d(nx, ny, m, L)(3, 7, 0, 0)
    assert (name, row, col) == ("sense2d", 3, 7) and sz == [2 * L * Cn * N, 2 * L * N]
    assert data[:4] == [nx, ny, L, Cn] and [type(v) for v in data[:4]] == [int] * 4
    flat = data[4]
    assert flat.dtype == np.float64 and flat.shape == (2 * Cn * N,)
    assert np.array_equal(flat, np.concatenate([m.real.reshape(-1), m.imag.reshape(-1)]))      # real planes first
    cube = m.reshape(Cn, nx, ny).transpose(0, 2, 1)                     # cube[c, y, x]
    assert cube[1, 2, 5] == m[1, 2 + 5 * ny]
    forms = [cube, np.asfortranarray(cube), list(m), tuple(cube), [list(p) for p in m], (m.real, m.imag), (cube.real, cube.imag),
             ([p for p in cube.real], [p for p in m.imag]), m.astype(np.complex64).astype(np.complex128)]
    for i, form in enumerate(forms[:-1]):
        other = prost.block.sense2d(nx, ny, form, L)(3, 7, 0, 0)
        assert other[1] == sz and other[0][:3] == ["sense2d", 3, 7] and other[0][3][:4] == data[:4] and np.array_equal(other[0][3][4], flat), i
    assert prost.block.sense2d(np.int64(2), 2.0, np.ones((1, 4), complex))(0, 0, 0, 0)[1] == [8, 8]       # L defaults to 1
    assert prost.block.sense2d(1, 1, [[1j]])(0, 0, 0, 0)[1] == [2, 2]
    assert prost.block.sense2d(4, 4, np.zeros((64, 16), complex))(0, 0, 0, 0)[1] == [2 * 64 * 16, 32]       # all-zero maps are legal
    doc = prost.block.sense2d.__doc__
    assert "set_scaling_identity" in doc and "BOUNDS" in doc and "Pock" in doc and "2^|1 - e/2|" in doc


def test_builder_value_errors():
    one = np.ones((2, 16), complex)
    bad = one.copy()
    bad[1, 3] = np.nan
    inf = one.copy()
    inf[0, 0] = 1j * np.inf
    for args, message in (((4.5, 4, one), "nx = 4.5 is not an integer"), ((4, np.inf, one), "ny = inf is not an integer"), ((4, 4, one, np.nan), "L = nan is not an integer"),
                          ((4, 4, one, True), "L = True is not an integer"), ((None, 4, one), "nx = None is not an integer"), ((0, 4, one), "nx = 0 has to be at least 1"),
                          ((4, 4, one, 0), "L = 0 has to be at least 1"), ((3, 4, one), "nx = 3 has to be a power of two from 1 to 2048"),
                          ((4, 12, one), "ny = 12 has to be a power of two from 1 to 2048"), ((4096, 4, one), "nx = 4096 has to be a power of two from 1 to 2048"),
                          ((4, 4, np.ones((2, 15), complex)), r"the maps have shape \(2, 15\); they are a \(C, ny, nx\) = \(C, 4, 4\) array, a \(C, N\) = \(C, 16\) array"),
                          ((4, 4, np.ones((2, 4, 2), complex)), r"the maps have shape \(2, 4, 2\)"), ((4, 4, np.ones(16, complex)), r"the maps have shape \(16,\)"),
                          ((4, 4, np.ones((2, 2, 4, 4), complex)), r"the maps have shape \(2, 2, 4, 4\)"),
                          ((4, 4, [np.ones(16, complex), np.ones(15, complex)]), r"plane 1 of the maps has shape \(15,\); a plane is a vector of nx ny = 16 values"),
                          ((4, 4, [np.ones((2, 8), complex)]), r"plane 0 of the maps has shape \(2, 8\)"),
                          ((4, 4, np.ones((2, 16))), "the maps have to be complex numbers, or a pair"), ((4, 4, "maps"), "the maps have to be complex numbers"),
                          ((4, 4, []), "the maps are empty"), ((4, 4, (np.ones((2, 16)), np.ones((3, 16)))), "the real parts are 2 planes and the imaginary parts 3"),
                          ((4, 4, np.ones((0, 16), complex)), "the maps are C = 0 planes; C has to be from 1 to 64"),
                          ((4, 4, np.ones((65, 16), complex)), "the maps are C = 65 planes; C has to be from 1 to 64"),
                          ((4, 4, bad), "the maps hold a non-finite value"), ((4, 4, inf), "the maps hold a non-finite value"),
                          ((4, 4, (np.ones((2, 16)), bad.real)), "the maps hold a non-finite value"),
                          ((4, 4, one, 2 ** 25), "L = 33554432 images of 4 x 4 with C = 2 coils; 2 L C nx ny has to stay below 2\\^31")):
        with pytest.raises(ValueError, match="sense2d: " + message):
            prost.block.sense2d(*args)
    prost.block.sense2d(4, 4, one, 2 ** 25 - 1)


@pytest.mark.parametrize("precision", ["single", "double"])
def test_the_name_is_registered(precision):
    prost.set_precision(precision)
    try:
        assert "sense2d" in prost.registered()["block"]
    finally:
        prost.set_precision("double")


def _raw_problem(data, rows, cols):
    x, z = prost.variable(cols), prost.variable(rows)
    prob = prost.min_max_problem([x], [z])
    prob.add_dual_pair(x, z, lambda row, col, nr, nc: [["sense2d", row, col, data], [rows, cols]])
    return prob


@pytest.mark.parametrize("precision", ["single", "double"])
def test_every_refusal_of_the_factory_by_message_and_declared_sizes(precision):
    m = np.ones(2 * 2 * 16)                                             # C = 2 maps of 4 x 4
    nan, huge = m.copy(), m.copy()
    nan[16 + 5] = np.nan
    huge[3 * 16 + 2] = 1e300
    cases = [
        ([4.5, 4, 1, 2, m], "BlockSense2D: nx = 4.5 has to be a power of two from 1 to 2048."),
        ([4, 0, 1, 2, m], "BlockSense2D: ny = 0 has to be a power of two from 1 to 2048."),
        ([3, 4, 1, 2, m], "BlockSense2D: nx = 3 has to be a power of two from 1 to 2048."),
        ([4, 4096, 1, 2, m], "BlockSense2D: ny = 4096 has to be a power of two from 1 to 2048."),
        ([4, np.nan, 1, 2, m], "BlockSense2D: ny = nan has to be a power of two from 1 to 2048."),
        ([4, 4, -1, 2, m], "BlockSense2D: L = -1 has to be a positive integer below 2^31."),
        ([4, 4, 1.5, 2, m], "BlockSense2D: L = 1.5 has to be a positive integer below 2^31."),
        ([4, 4, 1, 0, m], "BlockSense2D: C = 0 coils; C has to be an integer from 1 to 64."),
        ([4, 4, 1, 65, m], "BlockSense2D: C = 65 coils; C has to be an integer from 1 to 64."),
        ([4, 4, 1, 2.5, m], "BlockSense2D: C = 2.5 coils; C has to be an integer from 1 to 64."),
        ([4, 4, 2 ** 25, 2, m], "BlockSense2D: L = 3.35544e+07 images of 4 x 4 with C = 2 coils; 2 L C nx ny has to stay below 2^31."),
        ([4, 4, 1, 3, m], "BlockSense2D: the maps hold 64 values, not 2 C = 6 planes of nx ny = 16."),
        ([4, 4, 1, 2, m[:-1]], "BlockSense2D: the maps hold 63 values, not 2 C = 4 planes of nx ny = 16."),
        ([4, 4, 1, 2, nan], "BlockSense2D: value 5 of the real part of map 1, nan, is not finite"),
        ([4, 4, 1, 2, m, 64, 31], "BlockSense2D: the declared size 64 x 31 is not 2 L C ny nx x 2 L ny nx = 64 x 32."),
        ([4, 4, 2, 2, m, 64, 32], "BlockSense2D: the declared size 64 x 32 is not 2 L C ny nx x 2 L ny nx = 128 x 64."),
        ([4, 4, 1, 2], "BlockSense2D: the data cells are { nx, ny, L, C, maps }"),
        ([4, 4, 1, 2, m, 64], "BlockSense2D: the data cells are { nx, ny, L, C, maps }"),
        ([4, 4, 1, 2, "maps"], "BlockSense2D: the maps have to be a full vector of type single or double."),
    ]
    if precision == "single":
        cases.append(([4, 4, 1, 2, huge], "BlockSense2D: value 2 of the imaginary part of map 1, 1e+300, is not finite in single precision."))
    prost.set_precision(precision)
    try:
        for data, message in cases:
            with pytest.raises(prost.ProstError, match=re.escape(message)) as err:
                prost.problem_info(_raw_problem(data, 64, 32))
            assert "Creating block with ID 'sense2d' failed" in str(err.value)
        for data, rows, cols in (([4, 4, 1, 2, m], 64, 32), ([4, 4, 1, 2, m, 64, 32], 64, 32), ([1, 1, 1, 1, np.ones(2)], 2, 2), ([2, 8, 3, 2, m, 192, 96], 192, 96),
                                 ([4, 4, 1, 2, np.zeros(64)], 64, 32)):
            info = prost.problem_info(_raw_problem(data, rows, cols))
            assert int(info["nrows"]) == rows and int(info["ncols"]) == cols
        if precision == "double":
            prost.problem_info(_raw_problem([4, 4, 1, 2, huge], 64, 32))
    finally:
        prost.set_precision("double")


def test_the_case_list_holds_what_the_issue_names():
    assert set(R.CASES) >= {(1, 1, 1, 1), (1, 1, 2, 3), (1, 2, 1, 2), (2, 1, 1, 2), (2, 2, 1, 3), (4, 8, 1, 2), (8, 4, 2, 3), (1, 64, 1, 2), (64, 1, 1, 2), (64, 32, 1, 4),
                            (32, 64, 2, 3), (256, 64, 1, 2), (64, 256, 1, 2), (2048, 2, 1, 2), (2, 2048, 1, 2), (32, 32, 3, 5), (16, 16, 1, 64), (1, 2, 1100, 64)}
    assert len(R.CASES) == 18 and max(c[2] * c[3] for c in R.CASES) > 65535


@pytest.mark.parametrize("prec,dtype", PRECISIONS)
@pytest.mark.parametrize("case", SMALL, ids=R.case_id)
def test_restatement_against_the_float64_operator_the_matrix_and_adjointness(prec, dtype, case):
    nx, ny, L, Cn = case
    N = nx * ny
    rows, cols = R.sizes(case)
    rng = np.random.default_rng(R.case_seed(case))
    maps = R.make_maps(case, zeros=True)
    Bf, Bt = [b * (2 if dtype == np.float64 else 1) for b in R.bounds(case, dtype)]
    x, y = rng.standard_normal(cols).astype(dtype), rng.standard_normal(rows).astype(dtype)
    kx, kty = R.product(x, case, maps, False, dtype), R.product(y, case, maps, True, dtype)
    assert kx.dtype == dtype and kx.shape == (rows,) and kty.shape == (cols,)
    ef = R.image_norms(kx.astype(np.float64) - R.exact(x, case, maps, False, dtype), L * Cn, N)
    et = R.image_norms(kty.astype(np.float64) - R.exact(y, case, maps, True, dtype), L, N)
    sf, st = R.forward_scales(x, case, maps, dtype), R.transposed_scales(y, case, maps, dtype)
    print("%s %s: forward %.3f of Bf, transposed %.3f of Bt" % (prec, R.case_id(case), float((ef / np.maximum(sf, 1e-300)).max()) / Bf, float((et / np.maximum(st, 1e-300)).max()) / Bt))
    assert np.all(ef <= Bf * sf) and np.all(et <= Bt * st)
    if rows * cols <= 2 ** 22:
        K = R.matrix(case, maps, dtype)
        assert np.abs(K @ x.astype(np.float64) - R.exact(x, case, maps, False, dtype)).max() <= 1e-12 * max(1.0, np.abs(x).max()) * np.sqrt(N) * Cn
        assert np.abs(K.T @ y.astype(np.float64) - R.exact(y, case, maps, True, dtype)).max() <= 1e-12 * max(1.0, np.abs(y).max()) * np.sqrt(N) * Cn
    x64, y64 = x.astype(np.float64), y.astype(np.float64)
    assert abs(kx.astype(np.float64) @ y64 - x64 @ kty.astype(np.float64)) <= 2 * Bt * np.abs(R.maps64(maps, dtype)).max() * np.sqrt(Cn) * np.linalg.norm(x64) * np.linalg.norm(y64)
    resy, resx = rng.standard_normal(rows).astype(dtype), rng.standard_normal(cols).astype(dtype)
    assert np.array_equal(R.product(x, case, maps, False, dtype, resy), resy + kx) and np.array_equal(R.product(y, case, maps, True, dtype, resx), resx + kty)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_one_coil_of_ones_is_fft2d_and_one_by_one_is_the_pointwise_product(dtype):
    import fft2d_reference as F
    case = (8, 4, 2, 1)
    x = np.random.default_rng(3).standard_normal(R.sizes(case)[1]).astype(dtype)
    ones = np.ones((1, 32), complex)
    for transpose in (False, True):
        assert np.array_equal(R.product(x, case, ones, transpose, dtype), F.product(x, 8, 4, 2, transpose, dtype))
    case = (1, 1, 2, 3)
    maps = R.make_maps(case)
    u = np.random.default_rng(4).standard_normal(4).astype(dtype)
    s = R.rounded(maps, dtype)
    got = R.product(u, case, maps, False, dtype).reshape(2, 2, 3)
    assert np.array_equal(got[0], u[:2, None] * s[0, :, 0] - u[2:, None] * s[1, :, 0]) and np.array_equal(got[1], u[:2, None] * s[1, :, 0] + u[2:, None] * s[0, :, 0])


@pytest.mark.parametrize("e", [0.5, 1.0, 1.5, 2.0])
@pytest.mark.parametrize("shape", [(4, 2, 1), (4, 8, 3), (8, 8, 2)], ids=lambda s: "%dx%dx%d" % s)
def test_bound_sums_against_the_explicit_matrix(e, shape):
    nx, ny, Cn = shape
    case = (nx, ny, 1, Cn)
    maps = R.make_maps(case, zeros=True)
    assert (maps == 0).any()
    K = np.abs(R.matrix(case, maps, np.float64))
    with np.errstate(divide="ignore"):
        P = np.where(K > 0, K ** e, 0.0)
    S_rows, S_cols = P.sum(axis=1), np.ascontiguousarray(P.T).sum(axis=1)
    bar_rows, bar_cols = R.bound_sums(case, maps, np.float64, e)
    eps = np.finfo(np.float64).eps
    slack = 2.0 ** abs(1.0 - 0.5 * e)
    for S, bar in ((S_rows, bar_rows), (S_cols, bar_cols)):
        assert S.shape == bar.shape
        assert np.all(S <= bar * (1 + 16 * eps)) and np.all(bar <= slack * S * (1 + 16 * eps))
        if e == 2.0:
            assert np.all(np.abs(S - bar) <= (Cn + 8) * eps * bar)
    if e == 2.0 and Cn > 1:                                             # a row of the all-zero stretch of a map is still counted in its coil's sum
        assert bar_rows.min() > 0


def sense_problem(case, maps, alpha):
    """z = K x with only functions that take diagonal steps, so that no preconditioner entry is averaged over a group"""
    nx, ny, L, Cn = case
    bf = prost.block.sense2d(nx, ny, maps, L)
    rows, cols = bf(0, 0, 0, 0)[1]
    x, z = prost.variable(cols), prost.variable(rows)
    prob = prost.min_max_problem([x], [z])
    prob.add_function(x, prost.function.sum_1d("ind_box01"))
    prob.add_function(z, prost.function.sum_1d("ind_box01", 0.5, -0.5))
    prob.add_dual_pair(x, z, bf)
    prob.set_scaling_alpha(alpha)
    return prob


@pytest.mark.parametrize("precision,dtype", PRECISIONS)
@pytest.mark.parametrize("alpha", [1.0, 0.5])
@pytest.mark.parametrize("case", [(4, 8, 2, 3), (64, 32, 1, 4), (256, 64, 1, 2)], ids=R.case_id)
def test_preconditioners_from_the_bound_sums(precision, dtype, alpha, case):
    """Sigma = 1 / Rbar(alpha), Tau = 1 / Cbar(2 - alpha): within (C + 8) eps_T of (d), whatever N is (compensated sums)"""
    maps = R.make_maps(case)                                            # no zeros: 1 / 0 is not a step
    prost.set_precision(precision)
    try:
        info = prost.problem_info(sense_problem(case, maps, alpha))
    finally:
        prost.set_precision("double")
    rows, _ = R.bound_sums(case, maps, dtype, alpha)
    _, cols = R.bound_sums(case, maps, dtype, 2.0 - alpha)
    for got, want in ((info["scaling_left"], rows), (info["scaling_right"], cols)):
        got = np.asarray(got, dtype=np.float64).ravel()
        assert got.shape == want.shape
        assert np.all(np.abs(got * want - 1.0) <= (case[3] + 8) * np.finfo(dtype).eps), float(np.abs(got * want - 1.0).max() / np.finfo(dtype).eps)


@pytest.mark.parametrize("precision,dtype", PRECISIONS)
@pytest.mark.parametrize("alpha", [0.5, 1.5])
def test_preconditioners_with_exact_zeros_in_the_maps(precision, dtype, alpha):
    """the host block's sums at e = 0.5 and e = 1.5 with maps that hold exact zeros: a zero |sigma| is absent from the sum (0^e is not
    formed), and the bounds still hold against the explicit matrix's sums"""
    case = (4, 8, 2, 3)
    maps = R.make_maps(case, zeros=True)
    assert (maps == 0).sum() >= 10 and (np.abs(maps).sum(axis=0) > 0).all() and (np.abs(maps).sum(axis=1) > 0).all()
    prost.set_precision(precision)
    try:
        info = prost.problem_info(sense_problem(case, maps, alpha))
    finally:
        prost.set_precision("double")
    K = np.abs(R.matrix(case, maps, dtype))
    for got, e, axis in ((info["scaling_left"], alpha, 1), (info["scaling_right"], 2.0 - alpha, 0)):
        got = np.asarray(got, dtype=np.float64).ravel()
        want = R.bound_sums(case, maps, dtype, e)[1 - axis]
        assert got.shape == want.shape and np.isfinite(got).all()
        assert np.all(np.abs(got * want - 1.0) <= (case[3] + 8) * np.finfo(dtype).eps)
        with np.errstate(divide="ignore"):
            S = np.where(K > 0, K ** e, 0.0).sum(axis=axis)
        eps = np.finfo(dtype).eps
        assert np.all(S * got <= 1 + 16 * eps) and np.all(1.0 <= 2.0 ** abs(1.0 - 0.5 * e) * S * got * (1 + 16 * eps))


def _entry(dtype):
    fn = _hip.fn("sense2d", dtype)
    fn.argtypes = [C.c_void_p] * 6 + [C.c_int, C.c_void_p]
    fn.restype = C.c_int
    return fn


def test_header_declares_and_library_exports_the_entry_points():
    text = open(os.path.join(ROOT, "include", "prost_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(prost_hip_[a-z0-9_]+)\s*\(", text))
    names = ["prost_hip_sense2d_f32", "prost_hip_sense2d_f64"]
    assert not [n for n in names if n not in declared]
    assert "prost_hip_sense2d_geometry" in text
    Lb = _hip.lib()
    assert not [n for n in names if not hasattr(Lb, n)]
    assert Lb.prost_hip_abi_version() == 10
    assert re.search(r"#define\s+PROST_HIP_ABI_VERSION\s+10\b", text)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_entry_points_refuse_bad_arguments_without_a_device(dtype):
    """every refusal comes before anything touches a device: the pointers are never followed"""
    fn = _entry(dtype)
    good = R.abi_record((8, 4, 2, 3), False)
    p = C.c_void_p(16)
    assert fn(None, p, p, p, p, p, 0, None) != 0
    assert b"null geometry" in _hip.lib().prost_hip_last_error()
    for hole in range(5):
        ptrs = [p] * 5
        ptrs[hole] = None
        for transpose in (0, 1):
            rec = good.copy()
            rec[4] = transpose
            assert fn(rec.ctypes.data_as(C.c_void_p), *ptrs, 0, None) != 0
            assert b"null pointer" in _hip.lib().prost_hip_last_error()
    for field, value, message in ((0, 0, b"powers of two"), (1, 4096, b"powers of two"), (0, -4, b"powers of two"), (1, 3, b"powers of two"), (2, 0, b"image count"),
                                  (2, -7, b"image count"), (3, 0, b"coil count"), (3, 65, b"coil count"), (3, -1, b"coil count"), (2, 2 ** 24, b"below 2^31")):
        for transpose in (0, 1):
            for accumulate in (0, 1):
                bad = good.copy()
                bad[field] = value
                bad[4] = transpose
                assert fn(bad.ctypes.data_as(C.c_void_p), p, p, p, p, p, accumulate, None) != 0, (field, value)
                assert message in _hip.lib().prost_hip_last_error(), (field, value, _hip.lib().prost_hip_last_error())
