"""prost.block.fft2d without a GPU: the builder, the registry name, the creation errors, the preconditioners, the entry points -- and
the definition itself, on the references of tests/fft2d_reference.py.  u is the unit roundoff, B the bound (e) of the reference.

  * the builder describes { 'fft2d', row, col, { nx, ny, L } } with its sizes and refuses bad arguments with ValueError;
  * the name is registered for both precisions; every refusal of the factory, by its message, through prost.problem_info;
  * restatement (b) against numpy.fft.fft2(norm="ortho") in float64: |got - reference|_2 <= B |x|_2 per plane pair (2 B in fp64, where
    the reference is itself a float64 FFT), and against the explicit matrix (c) where it is small;
    <K x, y> = <x, K^T y> within the bound carried through the inner products, 2 B |x| |y|; K^T K x against x within (2 B + B^2) |x|;
    the accumulating form adds res0 last;
  * 1 x 1 is the identity bit for bit; 1 x n and n x 1 are the one-dimensional transform;
  * the closed-form sums (d) against the explicit matrix for every row and column, at every case with N <= 4096, for alpha in
    {0.5, 1, 1.5}, within (g + 8) eps; the preconditioners of a problem with the block against (d);
  * include/prost_hip.h declares the entry points, the kernel library exports them, they refuse bad arguments without a device, the
    ABI version is still 10.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import fft2d_reference as R
import prost_amd as prost
from prost_amd import _hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRECISIONS = [("single", np.float32), ("double", np.float64)]


def test_builder_cells_and_sizes():
    (name, row, col, data), sz = prost.block.fft2d(8, 4, 3)(3, 7, 0, 0)
    assert (name, row, col) == ("fft2d", 3, 7)
    assert data == [8, 4, 3] and [type(v) for v in data] == [int, int, int]
    assert sz == [2 * 3 * 32, 2 * 3 * 32]
    (_, _, _, data), sz = prost.block.fft2d(np.int64(16), 2.0)(0, 0, 0, 0)
    assert data == [16, 2, 1] and sz == [64, 64]
    assert prost.block.fft2d(1, 1)(0, 0, 0, 0)[1] == [2, 2]
    assert prost.block.fft2d(2048, 2048)(0, 0, 0, 0)[1] == [2 ** 23, 2 ** 23]
    doc = prost.block.fft2d.__doc__
    assert "set_scaling_identity" in doc and "conservative" in doc and "mask" in doc


def test_builder_value_errors():
    for args, message in (((4.5, 4, 1), "nx = 4.5 is not an integer"), ((4, np.inf, 1), "ny = inf is not an integer"), ((4, 4, np.nan), "L = nan is not an integer"),
                          ((4, 4, True), "L = True is not an integer"), ((4, "4", 1), "ny = '4' is not an integer"), ((None, 4, 1), "nx = None is not an integer"),
                          ((0, 4, 1), "nx = 0 has to be at least 1"), ((4, -2, 1), "ny = -2 has to be at least 1"), ((4, 4, 0), "L = 0 has to be at least 1"),
                          ((3, 4, 1), "nx = 3 has to be a power of two from 1 to 2048"), ((4, 12, 1), "ny = 12 has to be a power of two from 1 to 2048"),
                          ((4096, 4, 1), "nx = 4096 has to be a power of two from 1 to 2048"), ((4, 2049, 1), "ny = 2049 has to be a power of two from 1 to 2048"),
                          ((2048, 2048, 256), "L = 256 images of 2048 x 2048; 2 L nx ny has to stay below 2\\^31"),
                          ((1, 1, 2 ** 30), "2 L nx ny has to stay below 2\\^31")):
        with pytest.raises(ValueError, match=message):
            prost.block.fft2d(*args)
    prost.block.fft2d(2048, 2048, 255)
    prost.block.fft2d(1, 1, 2 ** 30 - 1)


@pytest.mark.parametrize("precision", ["single", "double"])
def test_the_name_is_registered(precision):
    prost.set_precision(precision)
    try:
        assert "fft2d" in prost.registered()["block"]
    finally:
        prost.set_precision("double")


def _raw_problem(data, n):
    x, z = prost.variable(n), prost.variable(n)
    prob = prost.min_max_problem([x], [z])
    prob.add_dual_pair(x, z, lambda row, col, nr, nc: [["fft2d", row, col, data], [n, n]])
    return prob


@pytest.mark.parametrize("precision", ["single", "double"])
def test_every_refusal_of_the_factory_by_message(precision):
    cases = [
        ([4.5, 4, 1], "BlockFFT2D: nx = 4.5 has to be a power of two from 1 to 2048."),
        ([4, 0, 1], "BlockFFT2D: ny = 0 has to be a power of two from 1 to 2048."),
        ([3, 4, 1], "BlockFFT2D: nx = 3 has to be a power of two from 1 to 2048."),
        ([4, 12, 1], "BlockFFT2D: ny = 12 has to be a power of two from 1 to 2048."),
        ([4096, 4, 1], "BlockFFT2D: nx = 4096 has to be a power of two from 1 to 2048."),
        ([4, np.nan, 1], "BlockFFT2D: ny = nan has to be a power of two from 1 to 2048."),
        ([4, -8, 1], "BlockFFT2D: ny = -8 has to be a power of two from 1 to 2048."),
        ([4, 4, -1], "BlockFFT2D: L = -1 has to be a positive integer below 2^31."),
        ([4, 4, 1.5], "BlockFFT2D: L = 1.5 has to be a positive integer below 2^31."),
        ([4, 4, 2.0 ** 31], "BlockFFT2D: L = 2.14748e+09 has to be a positive integer below 2^31."),
        ([2048, 2048, 256], "BlockFFT2D: L = 256 images of 2048 x 2048; 2 L nx ny has to stay below 2^31."),
        ([4, 4, 1, 32, 31], "BlockFFT2D: the declared size 32 x 31 is not 2 L ny nx x 2 L ny nx = 32 x 32."),
        ([4, 4, 2, 32, 32], "BlockFFT2D: the declared size 32 x 32 is not 2 L ny nx x 2 L ny nx = 64 x 64."),
        ([4, 4], "BlockFFT2D: the data cells are { nx, ny, L }"),
        ([4, 4, 1, 32], "BlockFFT2D: the data cells are { nx, ny, L }"),
    ]
    prost.set_precision(precision)
    try:
        for data, message in cases:
            with pytest.raises(prost.ProstError, match=re.escape(message)) as err:
                prost.problem_info(_raw_problem(data, 32))
            assert "Creating block with ID 'fft2d' failed" in str(err.value)
        for data, n in (([4, 4, 1], 32), ([4, 4, 1, 32, 32], 32), ([1, 1, 1], 2), ([2, 8, 2], 64)):
            info = prost.problem_info(_raw_problem(data, n))
            assert int(info["nrows"]) == n and int(info["ncols"]) == n
    finally:
        prost.set_precision("double")


def test_the_case_list_holds_what_the_issue_names_and_the_kernel_boundaries():
    shapes = {c[:2] for c in R.CASES}
    assert {(1, 1), (1, 2), (2, 1), (2, 2), (4, 8), (8, 4), (1, 64), (64, 1), (2048, 2), (2, 2048)} <= shapes and (32, 32, 3) in R.CASES
    # ny below and at 64 (pitched / plain lines); nx at 128 or below and above (small / large tile of the x pass); more than one tile in
    # either pass; the longest lines with a slab narrower than ny
    assert {32, 64} <= {c[1] for c in R.CASES}
    assert any(1 < nx <= 128 and ny > 2048 // nx for nx, ny, _ in R.CASES) and any(nx > 128 and ny > 8192 // nx for nx, ny, _ in R.CASES)
    assert any(ny >= 64 and nx > 2048 // ny for nx, ny, _ in R.CASES) and any(1 < ny < 64 and nx > 1024 // ny for nx, ny, _ in R.CASES)
    assert any(nx == 2048 and ny > 4 for nx, ny, _ in R.CASES)
    # 16 bytes per lane: a run (ny in the y pass, the slab width in the x pass) below 4 values, of 2 or 3 (on in fp64 only), of 4 and more
    assert {2, 4, 8} <= {ny for nx, ny, _ in R.CASES if nx > 1} and (2048, 2) in shapes and (4, 8) in shapes


def test_the_table_holds_its_exact_entries():
    for n in (1, 2, 4, 8, 64, 2048):
        for dtype in (np.float32, np.float64):
            w = R.table(n, dtype)
            assert w.shape == (n, 2) and w.dtype == dtype and tuple(w[0]) == (1.0, 0.0)
            if n >= 4:
                assert tuple(w[n // 4]) == (0.0, -1.0) and tuple(w[n // 2]) == (-1.0, 0.0)
            if n >= 8:
                assert tuple(w[n // 8]) == (dtype(np.sqrt(0.5)), -dtype(np.sqrt(0.5)))
            angle = 8 * np.arctan(np.longdouble(1)) * np.arange(n).astype(np.longdouble) / n        # the comparator in extended precision
            assert np.abs(w[:, 0] - np.cos(angle)).max() <= np.finfo(dtype).eps and np.abs(w[:, 1] + np.sin(angle)).max() <= np.finfo(dtype).eps


@pytest.mark.parametrize("prec,dtype", PRECISIONS)
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_restatement_against_numpy_fft_adjointness_and_inverse(prec, dtype, case):
    nx, ny, L = case
    n = 2 * L * nx * ny
    rng = np.random.default_rng(R.case_seed(case))
    B = R.bound(nx, ny, dtype)
    ref = 2 * B if dtype == np.float64 else B
    x = rng.standard_normal(n).astype(dtype)
    y = rng.standard_normal(n).astype(dtype)
    kx_ = R.product(x, nx, ny, L, False, dtype)
    kty = R.product(y, nx, ny, L, True, dtype)
    assert kx_.dtype == dtype and kx_.shape == (n,)
    worst = 0.0
    for got, v, transpose in ((kx_, x, False), (kty, y, True)):
        err = R.pair_norms(got.astype(np.float64) - R.fft_reference(v, nx, ny, L, transpose), nx, ny, L) / R.pair_norms(v, nx, ny, L)
        worst = max(worst, float(err.max()) / ref)
        assert np.all(err <= ref), float(err.max()) / ref
    print("%s %s: worst |restatement - numpy.fft| / bound = %.3f" % (prec, R.case_id(case), worst))
    if n <= 2048:                                                     # the explicit matrix
        K = R.matrix(nx, ny, L)
        assert np.all(R.pair_norms(kx_.astype(np.float64) - K @ x.astype(np.float64), nx, ny, L) <= ref * R.pair_norms(x, nx, ny, L))
        assert np.all(R.pair_norms(kty.astype(np.float64) - K.T @ y.astype(np.float64), nx, ny, L) <= ref * R.pair_norms(y, nx, ny, L))
    x64, y64 = x.astype(np.float64), y.astype(np.float64)
    assert abs(kx_.astype(np.float64) @ y64 - x64 @ kty.astype(np.float64)) <= 2 * B * np.linalg.norm(x64) * np.linalg.norm(y64)
    # K^T (K x) = x: two products, the second on an input of norm (1 + B) |x| at most
    back = R.product(kx_, nx, ny, L, True, dtype).astype(np.float64)
    assert np.all(R.pair_norms(back - x64, nx, ny, L) <= (2 * B + B * B) * R.pair_norms(x64, nx, ny, L))
    res0 = rng.standard_normal(n).astype(dtype)
    assert np.array_equal(R.product(x, nx, ny, L, False, dtype, res0), res0 + kx_)
    assert np.array_equal(R.product(y, nx, ny, L, True, dtype, res0), res0 + kty)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_one_by_one_is_the_identity_and_a_side_of_one_is_one_dimensional(dtype):
    v = np.random.default_rng(3).standard_normal(2 * 5).astype(dtype)
    v[::3] = -0.0
    for transpose in (False, True):
        got = R.product(v, 1, 1, 5, transpose, dtype)
        assert np.array_equal(got, v) and np.array_equal(np.signbit(got), np.signbit(v))
    for n in (2, 8, 64):
        x = np.random.default_rng(n).standard_normal(2 * n).astype(dtype)
        want = np.fft.fft(x[:n].astype(np.float64) + 1j * x[n:].astype(np.float64), norm="ortho")
        for nx, ny in ((1, n), (n, 1)):
            got = R.product(x, nx, ny, 1, False, dtype).astype(np.float64)
            assert np.linalg.norm(got - np.concatenate([want.real, want.imag])) <= 2 * R.bound(nx, ny, dtype) * np.linalg.norm(x)
        assert np.array_equal(R.product(x, 1, n, 1, False, dtype), R.product(x, n, 1, 1, False, dtype))     # the same tree on either axis


@pytest.mark.parametrize("alpha", [0.5, 1.0, 1.5])
@pytest.mark.parametrize("case", [c for c in R.CASES if c[0] * c[1] <= 4096], ids=R.case_id)
def test_closed_form_sums_against_the_explicit_matrix(alpha, case):
    """the matrix is block diagonal over the images: one image's 2 N x 2 N matrix is summed and compared with the rows of every image"""
    nx, ny, L = case
    N = nx * ny
    K = np.abs(R.matrix(nx, ny, 1))
    with np.errstate(divide="ignore"):
        P = np.where(K > 0, K ** alpha, 0.0)
    all_sums, all_g = R.sums(nx, ny, L, alpha)
    assert all_sums.shape == (2 * L * N,)
    want, g = all_sums[:2 * N], all_g[:2 * N]
    for c in range(L):                                                # re_c at c N, im_c at (L + c) N
        assert np.array_equal(all_sums[c * N:(c + 1) * N], want[:N]) and np.array_equal(all_sums[(L + c) * N:(L + c + 1) * N], want[N:])
    assert len(np.unique(g)) <= 12
    eps = np.finfo(np.float64).eps
    # both sums along the contiguous axis, where NumPy adds pairwise: a column summed down the rows is added one by one and loses sqrt(N) eps
    for got in (P.sum(axis=1), np.ascontiguousarray(P.T).sum(axis=1)):
        assert got.shape == want.shape
        ratio = np.abs(got - want) / want / ((g + 8) * eps)
        assert ratio.max() <= 1.0, float(ratio.max())


def fft_problem(case, alpha):
    """z = F x with only functions that take diagonal steps, so that no preconditioner entry is averaged over a group"""
    bf = prost.block.fft2d(*case)
    n = bf(0, 0, 0, 0)[1][0]
    x, z = prost.variable(n), prost.variable(n)
    prob = prost.min_max_problem([x], [z])
    prob.add_function(x, prost.function.sum_1d("ind_box01"))
    prob.add_function(z, prost.function.sum_1d("ind_box01", 0.5, -0.5))
    prob.add_dual_pair(x, z, bf)
    prob.set_scaling_alpha(alpha)
    return prob


@pytest.mark.parametrize("precision,dtype", PRECISIONS)
@pytest.mark.parametrize("alpha", [1.0, 0.5])
@pytest.mark.parametrize("case", [c for c in R.CASES if c[0] * c[1] <= 4096], ids=R.case_id)
def test_preconditioners_from_the_closed_form(precision, dtype, alpha, case):
    """Sigma = 1 / row sums of |K|^alpha, Tau = 1 / column sums of |K|^(2 - alpha): within (g + 8) eps_T of (d)"""
    prost.set_precision(precision)
    try:
        info = prost.problem_info(fft_problem(case, alpha))
    finally:
        prost.set_precision("double")
    nx, ny, L = case
    for got, a in ((info["scaling_left"], alpha), (info["scaling_right"], 2.0 - alpha)):
        got = np.asarray(got, dtype=np.float64).ravel()
        want, g = R.sums(nx, ny, L, a)
        assert got.shape == want.shape
        assert np.all(np.abs(got * want - 1.0) <= (g + 8) * np.finfo(dtype).eps), float(np.abs(got * want - 1.0).max() / np.finfo(dtype).eps)


def _entry(dtype):
    fn = _hip.fn("fft2d", dtype)
    fn.argtypes = [C.c_void_p] * 5 + [C.c_int, C.c_void_p]
    fn.restype = C.c_int
    return fn


def test_header_declares_and_library_exports_the_entry_points():
    text = open(os.path.join(ROOT, "include", "prost_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(prost_hip_[a-z0-9_]+)\s*\(", text))
    names = ["prost_hip_fft2d_f32", "prost_hip_fft2d_f64"]
    assert not [n for n in names if n not in declared]
    assert "prost_hip_fft2d_geometry" in text
    Lb = _hip.lib()
    assert not [n for n in names if not hasattr(Lb, n)]
    assert Lb.prost_hip_abi_version() == 10
    assert re.search(r"#define\s+PROST_HIP_ABI_VERSION\s+10\b", text)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_entry_points_refuse_bad_arguments_without_a_device(dtype):
    """every refusal comes before anything touches a device: the pointers are never followed"""
    fn = _entry(dtype)
    good = R.abi_record(8, 4, 1, False)
    p = C.c_void_p(16)
    assert fn(None, p, p, p, p, 0, None) != 0
    assert b"null geometry" in _hip.lib().prost_hip_last_error()
    for hole in range(4):
        ptrs = [p] * 4
        ptrs[hole] = None
        for transpose in (0, 1):
            rec = good.copy()
            rec[3] = transpose
            assert fn(rec.ctypes.data_as(C.c_void_p), *ptrs, 0, None) != 0
            assert b"null pointer" in _hip.lib().prost_hip_last_error()
    for field, value, message in ((0, 0, b"powers of two"), (1, 4096, b"powers of two"), (0, -4, b"powers of two"), (1, 3, b"powers of two"), (0, 12, b"powers of two"),
                                  (1, -2 ** 31, b"powers of two"), (2, 0, b"plane count"), (2, -7, b"plane count"), (2, 2 ** 25, b"below 2^31")):
        for transpose in (0, 1):
            for accumulate in (0, 1):
                bad = good.copy()
                bad[field] = value
                bad[3] = transpose
                assert fn(bad.ctypes.data_as(C.c_void_p), p, p, p, p, accumulate, None) != 0, (field, value)
                assert message in _hip.lib().prost_hip_last_error(), (field, value, _hip.lib().prost_hip_last_error())
