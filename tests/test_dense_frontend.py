"""The dense blocks without a GPU: dense, dense_kron_id and id_kron_dense.

  * prost.block.dense / dense_kron_id / id_kron_dense produce the cells and sizes of dense.m / dense_kron_id.m / id_kron_dense.m, from
    a copy of the caller's array; sparse input becomes a full matrix, 1-D input is refused;
  * prost.problem_info (host only) builds a problem that mixes a gradient2d block with each of them, and its preconditioners equal
    bit for bit those of oracle.Problem on the twin description (block.sparse / sparse_kron_id / id_kron_sparse of the same K);
  * the factory refuses a sparse cell ("Matrix must be dense!") and a missing or too small diaglength, naming the block;
  * prost_hip.h declares the new entry points and the kernel library exports them.
"""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import oracle
import prost_amd as prost
from prost_amd import _hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRECISIONS = [("single", np.float32), ("double", np.float64)]


def grid_matrix(m, n, seed):
    """zero-free, entries multiples of 1/64 in [-2, 2]: exact in float, so the sparse twins' float storage loses nothing"""
    rng = np.random.default_rng(seed)
    K = rng.integers(1, 129, size=(m, n)) * rng.choice([-1.0, 1.0], size=(m, n)) / 64.0
    assert np.all(K != 0) and np.array_equal(K.astype(np.float32).astype(np.float64), K)
    return K


def test_builders_mirror_the_m_builders():
    K = np.arange(6.0).reshape(2, 3) + 0.5
    keep = K.copy()
    (name, row, col, data), sz = prost.block.dense(K)(5, 7, 0, 0)
    assert (name, row, col, sz) == ("dense", 5, 7, [2, 3]) and len(data) == 1
    assert data[0].dtype == np.float64 and data[0].ndim == 2 and np.array_equal(data[0], K)
    (name, row, col, data), sz = prost.block.dense_kron_id(K, 10)(1, 2, 0, 0)
    assert (name, row, col, sz) == ("dense_kron_id", 1, 2, [20, 30]) and len(data) == 2 and data[1] == 10 and np.array_equal(data[0], K)
    (name, row, col, data), sz = prost.block.id_kron_dense(K, 4)(0, 0, 0, 0)
    assert (name, row, col, sz) == ("id_kron_dense", 0, 0, [8, 12]) and len(data) == 2 and data[1] == 4 and np.array_equal(data[0], K)
    # a copy: the caller's array is neither aliased nor changed
    data[0][0, 0] = 99.0
    assert np.array_equal(K, keep)
    K[1, 1] = -7.0
    assert prost.block.dense(keep)(0, 0, 0, 0)[0][3][0][1, 1] == keep[1, 1]
    # integer and sparse input become a full float64 matrix
    for make in (prost.block.dense, lambda k: prost.block.dense_kron_id(k, 3), lambda k: prost.block.id_kron_dense(k, 3)):
        S = sp.csr_matrix(np.array([[0.0, 2.0], [3.0, 0.0], [0.0, 0.0]]))
        got = make(S)(0, 0, 0, 0)[0][3][0]
        assert isinstance(got, np.ndarray) and got.dtype == np.float64 and np.array_equal(got, S.toarray())
        got = make(np.array([[1, 2], [3, 4]]))(0, 0, 0, 0)[0][3][0]
        assert got.dtype == np.float64 and got.shape == (2, 2)
        with pytest.raises(ValueError, match="2-D"):
            make(np.arange(4.0))


@pytest.mark.parametrize("precision", ["single", "double"])
def test_the_three_names_are_registered(precision):
    prost.set_precision(precision)
    try:
        reg = set(prost.registered()["block"])
    finally:
        prost.set_precision("double")
    assert {"dense", "dense_kron_id", "id_kron_dense"} <= reg


NX, NY, L = 6, 5, 4
D = NX * NY


def mixed_problem(kind, twin, alpha):
    """u in R^(nx ny L); q = gradient2d u; r = B u with B one of the three blocks (twin: the sparse description of the same matrix)"""
    n = D * L
    if kind == "dense":
        A = grid_matrix(7, n, 11)
        blk, rows = (prost.block.sparse(sp.csc_matrix(A)) if twin else prost.block.dense(A)), 7
    else:
        K = grid_matrix(3, L, 12)
        if kind == "dense_kron_id":
            blk = prost.block.sparse_kron_id(sp.csc_matrix(K), D) if twin else prost.block.dense_kron_id(K, D)
        else:
            blk = prost.block.id_kron_sparse(sp.csc_matrix(K), D) if twin else prost.block.id_kron_dense(K, D)
        rows = 3 * D
    u, q, r = prost.variable(n), prost.variable(2 * n), prost.variable(rows)
    prob = prost.min_max_problem([u], [q, r])
    prob.add_function(u, prost.function.sum_1d("square", 1, 0.5, 1))
    prob.add_function(q, prost.function.sum_norm2(2 * L, False, "ind_leq0", 1, 1, 1))
    prob.add_function(r, prost.function.sum_1d("ind_box01", 0.5, -0.5))
    prob.add_dual_pair(u, q, prost.block.gradient2d(NX, NY, L))
    prob.add_dual_pair(u, r, blk)
    prob.set_scaling_alpha(alpha)
    return prob


@pytest.mark.parametrize("precision,dtype", PRECISIONS)
@pytest.mark.parametrize("alpha", [1, 0.5])
@pytest.mark.parametrize("kind", ["dense", "dense_kron_id", "id_kron_dense"])
def test_preconditioners_equal_the_sparse_twin_in_the_oracle(precision, dtype, alpha, kind):
    prost.set_precision(precision)
    try:
        info = prost.problem_info(mixed_problem(kind, False, alpha))
    finally:
        prost.set_precision("double")
    twin = mixed_problem(kind, True, alpha)
    twin.finalize()
    P = oracle.Problem(twin.data, twin.nrows, twin.ncols, dtype)
    P.initialize()
    left, right = P.scaling()
    assert int(info["nrows"]) == twin.nrows and int(info["ncols"]) == twin.ncols
    assert np.array_equal(np.asarray(info["scaling_left"], dtype=np.float64).ravel(), left)
    assert np.array_equal(np.asarray(info["scaling_right"], dtype=np.float64).ravel(), right)


def test_factory_errors():
    K = grid_matrix(3, 4, 1)
    for name, data in (("dense", [sp.csc_matrix(K)]), ("dense_kron_id", [sp.csc_matrix(K), 5]), ("id_kron_dense", [sp.csc_matrix(K), 5])):
        u, q = prost.variable(20), prost.variable(15)
        prob = prost.min_max_problem([u], [q])
        prob.add_dual_pair(u, q, lambda row, col, nrows, ncols, name=name, data=data: [[name, row, col, data], [15, 20]])
        with pytest.raises(prost.ProstError, match="Matrix must be dense!"):
            prost.problem_info(prob)
    for name in ("dense_kron_id", "id_kron_dense"):
        for data in ([K], [K, 0], [K, -3]):
            u, q = prost.variable(20), prost.variable(15)
            prob = prost.min_max_problem([u], [q])
            prob.add_dual_pair(u, q, lambda row, col, nrows, ncols, name=name, data=data: [[name, row, col, data], [15, 20]])
            with pytest.raises(prost.ProstError, match=name + ".*diaglength"):
                prost.problem_info(prob)


def test_header_declares_and_library_exports_the_entry_points():
    text = open(os.path.join(ROOT, "include", "prost_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(prost_hip_[a-z0-9_]+)\s*\(", text))
    names = ["prost_hip_%s%s_%s" % (op, acc, s) for op in ("dense_kron_id", "id_kron_dense", "dense_gemv") for acc in ("", "_acc") for s in ("f32", "f64")]
    names.append("prost_hip_dense_gemv_workspace_bytes")
    assert not [n for n in names if n not in declared]
    Lb = _hip.lib()
    assert not [n for n in names if not hasattr(Lb, n)]
    assert Lb.prost_hip_abi_version() == 10
