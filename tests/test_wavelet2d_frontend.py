"""prost.block.wavelet2d without a GPU: the builder, the registry name, the creation errors, the preconditioners, the entry points --
and the definition itself, on the references of tests/wavelet2d_reference.py.  u is the unit roundoff, B the bound (e) of the reference.

  * the builder describes { 'wavelet2d', row, col, { nx, ny, L, taps, levels } } with its sizes and refuses bad arguments with
    ValueError; wavelet2d_taps equals the reference's closed forms bit for bit; a filter that misses orthonormality by 1e-9 is refused;
  * the name is registered for both precisions; every refusal of the factory, by its message, through prost.problem_info;
  * restatement (b) against the explicit matrix (c): |got - K x|_2 <= B |x|_2 per plane (2 B in fp64, where the matrix is itself
    float64 arithmetic); <K x, y> = <x, K^T y> within 2 B |x| |y|; K^T K x against x within 2 B |x|; the accumulating form adds
    res0 last; the matrix is orthogonal to 2e-13; 1 x n and n x 1 are the same one-dimensional transform;
  * the preconditioners of a problem with the block against the sums (d) of the explicit matrix, every row and column of every case
    with N <= 4096, alpha in {0.5, 1, 1.5} (Sigma from alpha, Tau from 2 - alpha), within the tolerance of test_wavelet2d_host.py
    carried to 1 / sum plus 4 eps_T;
  * include/prost_hip.h declares the entry points, the kernel library exports them, they refuse bad arguments without a device, the
    ABI version is still 10.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import prost_amd as prost
import wavelet2d_reference as R
from prost_amd import _hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRECISIONS = [("single", np.float32), ("double", np.float64)]
SMALL = [c for c in R.CASES if c[0] * c[1] <= 4096]


def test_builder_cells_and_sizes():
    (name, row, col, data), sz = prost.block.wavelet2d(8, 4, 3, "db2", 1)(3, 7, 0, 0)
    assert (name, row, col) == ("wavelet2d", 3, 7)
    assert data[:3] == [8, 4, 3] and data[4] == 1 and [type(v) for v in data[:3] + data[4:]] == [int] * 4
    assert np.array_equal(data[3], R.taps("db2")) and data[3].dtype == np.float64
    assert sz == [96, 96]
    (_, _, _, data), sz = prost.block.wavelet2d(np.int64(16), 2.0)(0, 0, 0, 0)
    assert data[:3] == [16, 2, 1] and data[4] == 1 and np.array_equal(data[3], R.taps("haar")) and sz == [32, 32]
    (_, _, _, data), sz = prost.block.wavelet2d(64, 64, 2, R.taps("lat8"), 3)(0, 0, 0, 0)
    assert np.array_equal(data[3], R.taps("lat8")) and sz == [8192, 8192]
    assert prost.block.wavelet2d(12, 20, 1, "db3", 2)(0, 0, 0, 0)[1] == [240, 240]
    assert prost.block.wavelet2d(1, 16, 1, list(R.taps("db2")), 2)(0, 0, 0, 0)[1] == [16, 16]
    doc = prost.block.wavelet2d.__doc__
    assert "set_scaling_identity" in doc and "conservative" in doc


def test_named_taps_bit_for_bit_and_known_values():
    for name in ("haar", "db2", "db3"):
        got = prost.block.wavelet2d_taps(name)
        assert got.dtype == np.float64 and np.array_equal(got, R.taps(name)), name
        assert R.ortho_defect(R.taps(name)) <= 1e-15 * len(got)
    assert np.allclose(R.taps("db3"), [0.33267, 0.80689, 0.45988, -0.13501, -0.08544, 0.03523], atol=5e-6, rtol=0)
    for name in ("lat8", "lat16"):
        assert len(R.taps(name)) == int(name[3:]) and R.ortho_defect(R.taps(name)) <= 1e-14
    with pytest.raises(ValueError, match="'db4' is not one of"):
        prost.block.wavelet2d_taps("db4")


def test_builder_value_errors():
    db2 = R.taps("db2")
    off = db2 + 1e-9 * np.array([1.0, -1.0, 1.0, 1.0])
    assert 1e-10 < R.ortho_defect(off) < 1e-8
    for args, message in (((4.5, 4, 1), "nx = 4.5 is not an integer"), ((4, np.inf, 1), "ny = inf is not an integer"), ((4, 4, np.nan), "L = nan is not an integer"),
                          ((4, 4, True), "L = True is not an integer"), ((4, "4", 1), "ny = '4' is not an integer"), ((None, 4, 1), "nx = None is not an integer"),
                          ((0, 4, 1), "nx = 0 has to be at least 1"), ((4, -2, 1), "ny = -2 has to be at least 1"), ((4, 4, 0), "L = 0 has to be at least 1"),
                          ((4, 4, 1, "haar", 0), "levels = 0 has to be at least 1"), ((4, 4, 1, "haar", 1.5), "levels = 1.5 is not an integer"),
                          ((4, 4, 1, "db4"), "'db4' is not one of"), ((4, 4, 1, None), "has to be a name or a vector of taps"),
                          ((4, 4, 1, [[1.0, 1.0]]), "have to be a vector"), ((4, 4, 1, [1.0]), "1 taps; the filter has to have an even number of taps from 2 to 16"),
                          ((4, 4, 1, [0.5] * 3), "3 taps"), ((64, 64, 1, np.ones(18)), "18 taps"), ((4, 4, 1, [np.nan, 1.0]), "non-finite"),
                          ((8, 8, 1, off), "not orthonormal"), ((8, 8, 1, np.round(db2, 10)), "truncated to fewer digits is refused"),
                          ((8, 8, 1, [1.0, 1.0]), "not orthonormal"),
                          ((1, 1, 1), "1 x 1 has nothing to transform"), ((6, 8, 1, "haar", 2), "nx = 6 is not divisible by 2\\^levels = 2\\^2"),
                          ((8, 12, 1, "haar", 3), "ny = 12 is not divisible"), ((8, 8, 1, "db2", 3), "the coarsest line holds 2 values, fewer than the filter's 4 taps"),
                          ((2, 1024, 1, "db2", 1), "nx = 2 at 1 levels: the coarsest line holds 2 values"), ((8, 8, 1, "haar", 31), "not divisible"),
                          ((32768, 32768, 2), "L nx ny has to stay below 2\\^31"), ((1, 2, 2 ** 30), "L nx ny has to stay below 2\\^31")):
        with pytest.raises(ValueError, match=message):
            prost.block.wavelet2d(*args)
    prost.block.wavelet2d(32768, 32768, 1)
    prost.block.wavelet2d(8, 8, 1, db2 + 1e-15, 2)                 # taps rounded from exact values pass
    prost.block.wavelet2d(8, 8, 1, -db2, 2)                        # the sum of the taps is not asked to be sqrt(2)


@pytest.mark.parametrize("precision", ["single", "double"])
def test_the_name_is_registered(precision):
    prost.set_precision(precision)
    try:
        assert "wavelet2d" in prost.registered()["block"]
    finally:
        prost.set_precision("double")


def _raw_problem(data, n):
    x, z = prost.variable(n), prost.variable(n)
    prob = prost.min_max_problem([x], [z])
    prob.add_dual_pair(x, z, lambda row, col, nr, nc: [["wavelet2d", row, col, data], [n, n]])
    return prob


@pytest.mark.parametrize("precision", ["single", "double"])
def test_every_refusal_of_the_factory_by_message(precision):
    haar, db2 = R.taps("haar"), R.taps("db2")
    cases = [
        ([4.5, 8, 1, haar, 1], "BlockWavelet2D: nx has to be a positive integer below 2^31 (nx = 4.5, ny = 8"),
        ([8, 0, 1, haar, 1], "BlockWavelet2D: ny has to be a positive integer below 2^31"),
        ([8, np.nan, 1, haar, 1], "BlockWavelet2D: ny has to be a positive integer below 2^31"),
        ([8, 8, 0, haar, 1], "BlockWavelet2D: L has to be a positive integer below 2^31"),
        ([8, 8, 1.5, haar, 1], "BlockWavelet2D: L has to be a positive integer below 2^31"),
        ([8, 8, 1, haar, 0], "BlockWavelet2D: levels has to be a positive integer"),
        ([8, 8, 1, haar, 1.5], "BlockWavelet2D: levels has to be a positive integer"),
        ([8, 8, 1, np.ones(3), 1], "BlockWavelet2D: the filter has to have an even number of taps from 2 to 16"),
        ([8, 8, 1, np.ones(18), 1], "BlockWavelet2D: the filter has to have an even number of taps from 2 to 16"),
        ([8, 8, 1, np.array([np.inf, 1.0]), 1], "BlockWavelet2D: the taps hold a non-finite value."),
        ([1, 1, 32, haar, 1], "BlockWavelet2D: a plane of 1 x 1 has nothing to transform"),
        ([6, 8, 1, haar, 2], "BlockWavelet2D: a side greater than 1 has to be divisible by 2^levels"),
        ([8, 8, 1, haar, 40], "BlockWavelet2D: a side greater than 1 has to be divisible by 2^levels"),
        ([8, 8, 1, db2, 3], "BlockWavelet2D: the coarsest line, side / 2^(levels-1), has to hold the filter's taps"),
        ([32768, 32768, 2, haar, 1], "BlockWavelet2D: L nx ny has to stay below 2^31"),
        ([8, 8, 1, db2 + 1e-9 * np.array([1.0, -1.0, 1.0, 1.0]), 1], "BlockWavelet2D: the taps are not orthonormal"),
        ([8, 8, 1, np.round(db2, 10), 1], "a table truncated to fewer digits is refused"),
        ([4, 4, 2, haar, 1, 32, 31], "BlockWavelet2D: the declared size 32 x 31 is not L ny nx x L ny nx = 32 x 32."),
        ([4, 4, 1, haar, 1, 32, 32], "BlockWavelet2D: the declared size 32 x 32 is not L ny nx x L ny nx = 16 x 16."),
        ([4, 4, 2, haar], "BlockWavelet2D: the data cells are { nx, ny, L, taps, levels }"),
        ([4, 4, 2, haar, 1, 32], "BlockWavelet2D: the data cells are { nx, ny, L, taps, levels }"),
        ([4, 4, 2, "haar", 1], "BlockWavelet2D: the taps have to be a full vector"),
    ]
    prost.set_precision(precision)
    try:
        for data, message in cases:
            with pytest.raises(prost.ProstError, match=re.escape(message)) as err:
                prost.problem_info(_raw_problem(data, 32))
            assert "Creating block with ID 'wavelet2d' failed" in str(err.value)
        for data, n in (([4, 4, 2, haar, 1], 32), ([4, 4, 2, haar, 2, 32, 32], 32), ([1, 16, 2, db2, 2], 32), ([8, 8, 1, db2, 2], 64)):
            info = prost.problem_info(_raw_problem(data, n))
            assert int(info["nrows"]) == n and int(info["ncols"]) == n
    finally:
        prost.set_precision("double")


def test_the_case_list_holds_what_the_issue_names_and_the_kernel_boundaries():
    assert {(2, 2, 1, "haar", 1), (1, 8, 1, "db2", 1), (8, 1, 1, "db2", 1), (8, 8, 1, "db2", 2), (12, 20, 1, "db3", 2), (24, 12, 1, "db2", 2), (32, 32, 3, "haar", 5),
            (64, 64, 1, "db2", 4), (160, 96, 1, "db3", 3), (256, 128, 1, "haar", 7), (64, 64, 1, "lat8", 3), (128, 128, 1, "lat16", 3), (4, 1024, 1, "haar", 2)} <= set(R.CASES)
    n = lambda c: c[0] * c[1]
    # both sides of the tail's threshold of 4096 values at level 0 and further down; a tiled level that is the last one; tiled 1-D levels
    assert any(n(c) == 4096 for c in R.CASES) and any(n(c) == 8192 and c[4] > 1 for c in R.CASES)
    assert any(n(c) > 4096 and n(c) >> (2 * (c[4] - 1)) > 4096 and min(c[:2]) > 1 for c in R.CASES)
    assert any(c[0] == 1 and n(c) > 4096 for c in R.CASES) and any(c[1] == 1 and n(c) > 4096 for c in R.CASES)
    # partial tiles: ny / 2 no multiple of 32, nx / 2 no multiple of 16, at a tiled level
    assert any(n(c) > 4096 and (c[1] // 2) % 32 for c in R.CASES) and any(n(c) > 4096 and (c[0] // 2) % 16 and c[0] > 32 for c in R.CASES)
    # 16 bytes per lane: tiled heights with no whole groups of 4 in a column (90) and in a sub-band (100, 90)
    assert any(n(c) > 4096 and c[1] % 4 for c in R.CASES) and any(n(c) > 4096 and c[1] % 4 == 0 and c[1] % 8 for c in R.CASES)
    for c in R.CASES:
        prost.block.wavelet2d(c[0], c[1], c[2], R.taps(c[3]), c[4])


@pytest.mark.parametrize("prec,dtype", PRECISIONS)
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_restatement_against_the_matrix_adjointness_and_inverse(prec, dtype, case):
    nx, ny, L, wavelet, levels = case
    n = L * nx * ny
    rng = np.random.default_rng(R.case_seed(case))
    B = R.bound(wavelet, levels, dtype)
    ref = 2 * B if dtype == np.float64 else B
    x, y = rng.standard_normal(n).astype(dtype), rng.standard_normal(n).astype(dtype)
    kx_ = R.product(x, nx, ny, L, wavelet, levels, False, dtype)
    kty = R.product(y, nx, ny, L, wavelet, levels, True, dtype)
    assert kx_.dtype == dtype and kx_.shape == (n,)
    x64, y64 = x.astype(np.float64), y.astype(np.float64)
    if nx * ny <= 4096:
        K = R.matrix(nx, ny, wavelet, levels)
        assert np.abs(K @ K.T - np.eye(nx * ny)).max() <= 2e-13
        worst = 0.0
        for got, v, transpose in ((kx_, x64, False), (kty, y64, True)):
            err = R.plane_norms(got.astype(np.float64) - R.apply_matrix(v, nx, ny, L, wavelet, levels, transpose), nx, ny, L) / R.plane_norms(v, nx, ny, L)
            worst = max(worst, float(err.max()) / ref)
            assert np.all(err <= ref), float(err.max()) / ref
        print("%s %s: worst |restatement - matrix| / bound = %.3f" % (prec, R.case_id(case), worst))
    assert abs(kx_.astype(np.float64) @ y64 - x64 @ kty.astype(np.float64)) <= 2 * B * np.linalg.norm(x64) * np.linalg.norm(y64)
    back = R.product(kx_, nx, ny, L, wavelet, levels, True, dtype).astype(np.float64)
    assert np.all(R.plane_norms(back - x64, nx, ny, L) <= 2 * B * R.plane_norms(x64, nx, ny, L))
    res0 = rng.standard_normal(n).astype(dtype)
    assert np.array_equal(R.product(x, nx, ny, L, wavelet, levels, False, dtype, res0), res0 + kx_)
    assert np.array_equal(R.product(y, nx, ny, L, wavelet, levels, True, dtype, res0), res0 + kty)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_a_side_of_one_is_one_dimensional(dtype):
    x = np.random.default_rng(3).standard_normal(32).astype(dtype)
    for transpose in (False, True):
        assert np.array_equal(R.product(x, 1, 32, 1, "db2", 2, transpose, dtype), R.product(x, 32, 1, 1, "db2", 2, transpose, dtype))
    # one level of haar: sums and differences of neighbours over sqrt(2)
    got = R.product(x, 1, 32, 1, "haar", 1, False, dtype).astype(np.float64)
    s = dtype(1.0 / np.sqrt(2.0))
    assert np.array_equal(got[:16], (s * x[0::2] + s * x[1::2]).astype(np.float64)) and np.array_equal(got[16:], (s * x[0::2] + (-s) * x[1::2]).astype(np.float64))


def wavelet_problem(case, alpha):
    """z = W x with only functions that take diagonal steps, so that no preconditioner entry is averaged over a group"""
    nx, ny, L, wavelet, levels = case
    bw = prost.block.wavelet2d(nx, ny, L, R.taps(wavelet), levels)
    n = L * nx * ny
    x, z = prost.variable(n), prost.variable(n)
    prob = prost.min_max_problem([x], [z])
    prob.add_function(x, prost.function.sum_1d("ind_box01"))
    prob.add_function(z, prost.function.sum_1d("ind_box01", 0.5, -0.5))
    prob.add_dual_pair(x, z, bw)
    prob.set_scaling_alpha(alpha)
    return prob


@pytest.mark.parametrize("precision,dtype", PRECISIONS)
@pytest.mark.parametrize("alpha", [1.0, 0.5])
@pytest.mark.parametrize("case", SMALL, ids=R.case_id)
def test_preconditioners_from_the_sums(precision, dtype, alpha, case):
    """Sigma = 1 / row sums of |K|^alpha, Tau = 1 / column sums of |K|^(2 - alpha); alpha = 1 and 0.5 ask for the exponents 0.5, 1, 1.5"""
    prost.set_precision(precision)
    try:
        info = prost.problem_info(wavelet_problem(case, alpha))
    finally:
        prost.set_precision("double")
    nx, ny, L, wavelet, levels = case
    for side, (got, a) in enumerate(((info["scaling_left"], alpha), (info["scaling_right"], 2.0 - alpha))):
        got = np.asarray(got, dtype=np.float64).ravel()
        want = R.sums(nx, ny, L, wavelet, levels, a)[side]
        tol = np.tile(R.sums_tolerance(nx, ny, wavelet, levels, a)[side], L)
        assert got.shape == want.shape
        # the sum is rounded to T, inverted in T and handed back: 4 eps_T relative on top of the sum's own tolerance
        assert np.all(np.abs(got * want - 1.0) <= tol / want + 4 * np.finfo(dtype).eps), float(np.abs(got * want - 1.0).max())


def _entry(dtype):
    fn = _hip.fn("wavelet2d", dtype)
    fn.argtypes = [C.c_void_p] * 5 + [C.c_int, C.c_void_p]
    fn.restype = C.c_int
    return fn


def test_header_declares_and_library_exports_the_entry_points():
    text = open(os.path.join(ROOT, "include", "prost_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(prost_hip_[a-z0-9_]+)\s*\(", text))
    names = ["prost_hip_wavelet2d_f32", "prost_hip_wavelet2d_f64"]
    assert not [n for n in names if n not in declared]
    assert "prost_hip_wavelet2d_geometry" in text
    Lb = _hip.lib()
    assert not [n for n in names if not hasattr(Lb, n)]
    assert Lb.prost_hip_abi_version() == 10
    assert re.search(r"#define\s+PROST_HIP_ABI_VERSION\s+10\b", text)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_entry_points_refuse_bad_arguments_without_a_device(dtype):
    """every refusal comes before anything touches a device: the device pointers are never followed"""
    fn = _entry(dtype)
    good = R.abi_record(8, 8, 1, 4, 2, False)
    taps = R.taps("db2").astype(dtype)
    t = taps.ctypes.data_as(C.c_void_p)
    p = C.c_void_p(16)
    assert fn(None, t, p, p, p, 0, None) != 0
    assert b"null geometry" in _hip.lib().prost_hip_last_error()
    for hole in range(4):
        ptrs = [t, p, p, p]
        ptrs[hole] = None
        for transpose in (0, 1):
            rec = good.copy()
            rec[5] = transpose
            assert fn(rec.ctypes.data_as(C.c_void_p), *ptrs, 0, None) != 0
            assert b"null pointer" in _hip.lib().prost_hip_last_error()
    for field, value, message in ((0, 0, b"ny has to be"), (1, -4, b"nx has to be"), (2, 0, b"L has to be"), (2, -7, b"L has to be"), (3, 0, b"levels has to be"),
                                  (3, -1, b"levels has to be"), (4, 3, b"even number of taps"), (4, 18, b"even number of taps"), (4, 0, b"even number of taps"),
                                  (3, 3, b"has to hold the filter's taps"), (0, 10, b"divisible by 2^levels"), (3, 31, b"divisible by 2^levels"),
                                  (2, 2 ** 25, b"below 2^31")):
        for transpose in (0, 1):
            for accumulate in (0, 1):
                bad = good.copy()
                bad[field] = value
                bad[5] = transpose
                assert fn(bad.ctypes.data_as(C.c_void_p), t, p, p, p, accumulate, None) != 0, (field, value)
                assert message in _hip.lib().prost_hip_last_error(), (field, value, _hip.lib().prost_hip_last_error())
    one = good.copy()
    one[0] = one[1] = 1
    assert fn(one.ctypes.data_as(C.c_void_p), t, p, p, p, 0, None) != 0 and b"1 x 1" in _hip.lib().prost_hip_last_error()
