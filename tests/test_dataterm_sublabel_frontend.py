"""prost.block.dataterm_sublabel without a GPU: the builder, the registry name, the creation errors, the preconditioners, the entry
points -- and the definition itself, on the references of tests/dataterm_sublabel_reference.py.

  * the builder describes { 'dataterm_sublabel', row, col, { nx, ny, L, left, right } } of size 2 N (L - 1) square and refuses bad
    arguments with ValueError;
  * the name is registered for both precisions; every refusal of the factory, by its message, through prost.problem_info;
  * preconditioners of a problem that mixes gradient2d on u with the block: alpha = 1 and float-exact delta / gamma equal those of
    oracle.Problem on the block.sparse twin bit for bit (left = 0: the gamma_0 entry is absent on both sides); alpha != 1 equals the
    formulas evaluated in fp64 to a relative (k + 8) eps_T (pow is a library call, the additions are at most k + 1);
  * include/prost_hip.h declares the two entry points, the kernel library exports them, the ABI version is still 10;
  * the definition: on a lifted point u = 1_j^alpha, w = e_j the coefficients m of r are zero off interval j and m_j / w_j is the label
    value left + (j + alpha) delta; the rows of matrix (a) reproduce m and -w; matrix (a) equals restatement (b) to (k + 2) eps.
"""
import os
import re

import numpy as np
import pytest

import dataterm_sublabel_reference as R
import oracle
import prost_amd as prost
from prost_amd import _hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRECISIONS = [("single", np.float32), ("double", np.float64)]


def test_builder_cells_size_and_value_errors():
    (name, row, col, data), sz = prost.block.dataterm_sublabel(6, 5, 4, -0.5, 2.5)(3, 7, 0, 0)
    assert (name, row, col) == ("dataterm_sublabel", 3, 7)
    assert data == [6, 5, 4, -0.5, 2.5] and [type(v) for v in data] == [int, int, int, float, float]
    assert sz == [2 * 30 * 3, 2 * 30 * 3]
    (_, _, _, data), sz = prost.block.dataterm_sublabel(np.int64(1), 1.0, 2, 0, 1)(0, 0, 0, 0)
    assert data == [1, 1, 2, 0.0, 1.0] and sz == [2, 2] and [type(v) for v in data] == [int, int, int, float, float]
    for args, message in (((4, 4, 1, 0, 1), "at least 2"), ((4, 4, 0, 0, 1), "at least 2"), ((4, 4, -3, 0, 1), "at least 2"),
                          ((0, 4, 3, 0, 1), "at least 1"), ((4, 0, 3, 0, 1), "at least 1"), ((-1, 4, 3, 0, 1), "at least 1"),
                          ((4, 4, 3, np.nan, 1), "finite"), ((4, 4, 3, 0, np.inf), "finite"), ((4, 4, 3, -np.inf, 1), "finite"),
                          ((4, 4, 3, 1, 1), "below right"), ((4, 4, 3, 2, 1), "below right"),
                          ((4.5, 4, 3, 0, 1), "not an integer"), ((4, 4, 2.5, 0, 1), "not an integer"), ((4, np.inf, 3, 0, 1), "not an integer"),
                          ((np.nan, 4, 3, 0, 1), "not an integer")):
        with pytest.raises(ValueError, match=message):
            prost.block.dataterm_sublabel(*args)


@pytest.mark.parametrize("precision", ["single", "double"])
def test_the_name_is_registered(precision):
    prost.set_precision(precision)
    try:
        assert "dataterm_sublabel" in prost.registered()["block"]
    finally:
        prost.set_precision("double")


def _raw_problem(data, size):
    x, z = prost.variable(size), prost.variable(size)
    prob = prost.min_max_problem([x], [z])
    prob.add_dual_pair(x, z, lambda row, col, nrows, ncols: [["dataterm_sublabel", row, col, data], [size, size]])
    return prob


@pytest.mark.parametrize("precision", ["single", "double"])
def test_every_refusal_of_the_factory_by_message(precision):
    cases = [
        ([3, 2, 1, 0.0, 1.0], "BlockDatatermSublabel: L = 1 labels, at least 2 are needed."),
        ([3, 2, 0, 0.0, 1.0], "BlockDatatermSublabel: L = 0 labels, at least 2 are needed."),
        ([3, 2, -4, 0.0, 1.0], "BlockDatatermSublabel: L = -4 labels, at least 2 are needed."),
        ([0, 2, 3, 0.0, 1.0], "BlockDatatermSublabel: nx = 0 and ny = 2 have to be at least 1."),
        ([3, 0, 3, 0.0, 1.0], "BlockDatatermSublabel: nx = 3 and ny = 0 have to be at least 1."),
        ([-3, 2, 3, 0.0, 1.0], "BlockDatatermSublabel: nx = -3 and ny = 2 have to be at least 1."),
        ([3, 2, 3, np.nan, 1.0], "BlockDatatermSublabel: the bounds left = nan and right = 1 have to be finite."),
        ([3, 2, 3, 0.0, np.inf], "BlockDatatermSublabel: the bounds left = 0 and right = inf have to be finite."),
        ([3, 2, 3, -np.inf, 1.0], "BlockDatatermSublabel: the bounds left = -inf and right = 1 have to be finite."),
        ([3, 2, 3, 1.0, 1.0], "BlockDatatermSublabel: left = 1 has to be below right = 1."),
        ([3, 2, 3, 2.0, 1.0], "BlockDatatermSublabel: left = 2 has to be below right = 1."),
        ([3, 2, 3, 0.0, 1.0, 24, 23], "BlockDatatermSublabel: the declared size 24 x 23 is not 2 nx ny (L - 1) = 24 square."),
        ([3, 2, 3, 0.0, 1.0, 12, 12], "BlockDatatermSublabel: the declared size 12 x 12 is not 2 nx ny (L - 1) = 24 square."),
        ([3, 2, 3, 0.0], "BlockDatatermSublabel: the data cells are { nx, ny, L, left, right }"),
    ]
    prost.set_precision(precision)
    try:
        for data, message in cases:
            with pytest.raises(prost.ProstError, match=re.escape(message)) as err:
                prost.problem_info(_raw_problem(data, 24))
            assert "Creating block with ID 'dataterm_sublabel' failed" in str(err.value)
        for data in ([3, 2, 3, 0.0, 1.0], [3, 2, 3, 0.0, 1.0, 24, 24]):
            info = prost.problem_info(_raw_problem(data, 24))
            assert int(info["nrows"]) == 24 and int(info["ncols"]) == 24
    finally:
        prost.set_precision("double")


NX, NY = 5, 3


def mixed_problem(L, left, right, twin, alpha, elementwise=False):
    """x = [u ; w]; q = gradient2d u; z = B x with B the block (twin: block.sparse of matrix (a)).  elementwise: only functions that
    take diagonal steps, so that no preconditioner entry is averaged over a group"""
    N, k = NX * NY, L - 1
    x, q, z = prost.variable(2 * N * k), prost.variable(2 * N * k), prost.variable(2 * N * k)
    u = prost.sub_variable(x, N * k)
    w = prost.sub_variable(x, N * k)
    prob = prost.min_max_problem([x], [q, z])
    prob.add_function(u, prost.function.zero())
    prob.add_function(w, prost.function.sum_1d("ind_box01") if elementwise else prost.function.sum_ind_simplex(k, False))
    prob.add_function(q, prost.function.sum_1d("ind_box01", 0.5, -0.5) if elementwise else prost.function.sum_norm2(2, False, "ind_leq0", 1, 1, 1))
    prob.add_function(z, prost.function.sum_1d("ind_box01", 0.5, -0.5))
    prob.add_dual_pair(u, q, prost.block.gradient2d(NX, NY, k))
    prob.add_dual_pair(x, z, prost.block.sparse(R.matrix(NX, NY, L, left, right)) if twin else prost.block.dataterm_sublabel(NX, NY, L, left, right))
    prob.set_scaling_alpha(alpha)
    return prob


@pytest.mark.parametrize("precision,dtype", PRECISIONS)
@pytest.mark.parametrize("left,right,L", [(0.25, 2.0, 8), (0.0, 1.75, 8), (-0.5, 0.0, 3), (0.0, 1.0, 2)])
def test_preconditioners_equal_the_sparse_twin_in_the_oracle(precision, dtype, left, right, L):
    """alpha = 1; delta and every gamma_i are float-exact (multiples of 1/4), so sums in any order are exact"""
    delta, gamma = R.labels(L, left, right, np.float32)
    assert float(delta) == (right - left) / (L - 1) and np.array_equal(gamma.astype(np.float64), left + np.arange(L - 1) * float(delta))
    prost.set_precision(precision)
    try:
        info = prost.problem_info(mixed_problem(L, left, right, False, 1))
    finally:
        prost.set_precision("double")
    twin = mixed_problem(L, left, right, True, 1)
    twin.finalize()
    if left == 0.0:
        # the gamma_0 entry is absent from the twin: plane 0 of r holds (L - 1) entries per row, not L
        K = R.matrix(NX, NY, L, left, right)
        assert K[0].nnz == L - 1 and K[NX * NY * (L - 1) - 1].nnz == (2 if L > 2 else 1)
    P = oracle.Problem(twin.data, twin.nrows, twin.ncols, dtype)
    P.initialize()
    sl, sr = P.scaling()
    assert int(info["nrows"]) == twin.nrows and int(info["ncols"]) == twin.ncols
    assert np.array_equal(np.asarray(info["scaling_left"], dtype=np.float64).ravel(), sl)
    assert np.array_equal(np.asarray(info["scaling_right"], dtype=np.float64).ravel(), sr)


@pytest.mark.parametrize("precision,dtype", PRECISIONS)
@pytest.mark.parametrize("alpha", [0.5, 1.5])
@pytest.mark.parametrize("left,right,L", [(0.1, 0.9, 6), (0.0, 1.0, 4), (-0.7, 0.6, 2)])
def test_preconditioners_for_other_alpha_equal_the_formulas(precision, dtype, alpha, left, right, L):
    """Sigma = 1 / row sums of |K|^alpha, Tau = 1 / column sums of |K|^(2 - alpha) (the problem's rule), rows [q ; z], columns [u ; w];
    gradient2d adds 2 to every row of q and 4 to every column of u.  Formulas in fp64 on the T-rounded delta and gamma."""
    N, k = NX * NY, L - 1
    prost.set_precision(precision)
    try:
        info = prost.problem_info(mixed_problem(L, left, right, False, alpha, elementwise=True))
    finally:
        prost.set_precision("double")
    delta, gamma = R.labels(L, left, right, dtype)
    K = abs(R.matrix(NX, NY, L, left, right, dtype))
    rows = np.asarray(K.power(alpha).sum(axis=1)).ravel()
    cols = np.asarray(K.power(2.0 - alpha).sum(axis=0)).ravel()
    if dtype == np.float64:       # the sum formulas (c), in fp64, are the sums of the matrix
        assert np.allclose(R.sums(N, L, left, right, alpha)[0], rows, rtol=1e-14, atol=0)
        assert np.allclose(R.sums(N, L, left, right, 2.0 - alpha)[1], cols, rtol=1e-14, atol=0)
    cols[:N * k] += 4.0
    want_left = 1.0 / np.concatenate([np.full(2 * N * k, 2.0), rows])
    want_right = 1.0 / cols
    tol = (k + 8) * np.finfo(dtype).eps
    got_left = np.asarray(info["scaling_left"], dtype=np.float64).ravel()
    got_right = np.asarray(info["scaling_right"], dtype=np.float64).ravel()
    assert np.all(np.abs(got_left - want_left) <= tol * want_left), float((np.abs(got_left - want_left) / want_left).max() / np.finfo(dtype).eps)
    assert np.all(np.abs(got_right - want_right) <= tol * want_right), float((np.abs(got_right - want_right) / want_right).max() / np.finfo(dtype).eps)


def test_header_declares_and_library_exports_the_entry_points():
    text = open(os.path.join(ROOT, "include", "prost_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(prost_hip_[a-z0-9_]+)\s*\(", text))
    names = ["prost_hip_linop_dataterm_sublabel_f32", "prost_hip_linop_dataterm_sublabel_f64"]
    assert not [n for n in names if n not in declared]
    Lb = _hip.lib()
    assert not [n for n in names if not hasattr(Lb, n)]
    assert Lb.prost_hip_abi_version() == 10


def test_the_definition_itself():
    """the lifted point of label value t = left + (j + alpha) delta is u = 1_j^alpha, w = e_j; the data term there is
    sum_i sup_{epi phi_i*} (m_i r_i - w_i s_i) = phi_j(m_j / w_j) = phi_j(t), with m the coefficients of r"""
    rng = np.random.default_rng(5)
    left, right, L = -0.3, 1.9, 7
    k = L - 1
    delta, gamma = R.labels(L, left, right)
    K = R.matrix(1, 1, L, left, right)
    a, b, c = rng.uniform(0.5, 2, k), rng.standard_normal(k), rng.standard_normal(k)
    for j in range(k):
        for alpha in (0.0, 0.37, 1.0):
            u = np.r_[np.ones(j), alpha, np.zeros(k - 1 - j)]
            w = np.zeros(k)
            w[j] = 1.0
            suffix = np.r_[np.cumsum(w[::-1])[::-1][1:], 0.0]
            m = gamma * w + delta * (u - suffix)
            off = np.arange(k) != j
            assert np.all(np.abs(m[off]) <= 4 * np.finfo(np.float64).eps)
            t = left + (j + alpha) * delta
            assert abs(m[j] / w[j] - t) <= 8 * np.finfo(np.float64).eps * max(1.0, abs(t))
            assert gamma[j] - 1e-15 <= m[j] / w[j] <= gamma[j] + delta + 1e-15
            # phi_j at m_j / w_j is the data term's value at t
            assert abs((a[j] * m[j] + b[j]) * m[j] + c[j] - ((a[j] * t + b[j]) * t + c[j])) <= 1e-13
            got = K @ np.r_[u, w]
            assert np.all(np.abs(got[:k] - m) <= 4 * np.finfo(np.float64).eps) and np.array_equal(got[k:], -w)


@pytest.mark.parametrize("shape", [(1, 1, 2), (1, 1, 3), (5, 1, 4), (3, 4, 9), (2, 2, 33)])
def test_matrix_equals_restatement(shape):
    """(a) against (b) in fp64, both directions: |K x - march| <= (k + 2) eps (|K| |x|) componentwise; the accumulating forms add res0"""
    nx, ny, L = shape
    N, k = nx * ny, L - 1
    rng = np.random.default_rng(nx + 10 * ny + 100 * L)
    left, right = -0.4, 1.3
    K = R.matrix(nx, ny, L, left, right)
    # entry by entry: delta on the diagonal of (r, u), gamma_i at (r_i, w_i), -delta at (r_i, w_j) for j > i, -1 at (s_i, w_i)
    delta, gamma = R.labels(L, left, right)
    D = K.toarray()
    for p in (0, N - 1):
        for i in range(k):
            row = np.zeros(2 * N * k)
            row[i * N + p] = delta
            row[N * k + i * N + p] = gamma[i]
            for j in range(i + 1, k):
                row[N * k + j * N + p] = -delta
            assert np.array_equal(D[i * N + p], row)
            row = np.zeros(2 * N * k)
            row[N * k + i * N + p] = -1.0
            assert np.array_equal(D[N * k + i * N + p], row)
    eps = np.finfo(np.float64).eps
    for transpose, M in ((False, K), (True, K.T.tocsc())):
        x = rng.standard_normal(2 * N * k)
        got = R.product(x, N, L, left, right, transpose, np.float64)
        assert np.all(np.abs(got - M @ x) <= (k + 2) * eps * (abs(M) @ np.abs(x)))
        res0 = rng.standard_normal(2 * N * k)
        assert np.array_equal(R.product(x, N, L, left, right, transpose, np.float64, res0), res0 + got)
    rs, cs = R.sums(N, L, left, right, 1.0)
    assert np.allclose(rs, np.asarray(abs(K).sum(axis=1)).ravel(), rtol=1e-14) and np.allclose(cs, np.asarray(abs(K).sum(axis=0)).ravel(), rtol=1e-14)
