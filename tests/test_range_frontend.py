"""ind_range without a GPU: the builder, the registry name, the creation errors, the C ABI additions and the launch plan of the dense
solve (prost_hip_range_potrs_plan).

  * prost.function.ind_range(A, AA=None) mirrors ind_range.m: { 'ind_range', idx, count, false, { A, AA } } with A a CSC float64 copy
    and AA a full float64 copy (A'A when left out); a sparse AA is handed on untouched;
  * the name is registered for both precisions;
  * the three factory messages and the two setter messages of the reference, through prost.problem_info (host only);
  * include/prost_hip.h declares the new entry points, the kernel library exports them, the ABI version is still 10;
  * the plan: tier and launches are monotone in n, the small tier's vector fits its LDS (at most 64 KiB), the large tier takes two
    launches per block of NB, the workspace holds every entry the launches index, n = 0 and n * n >= 2^31 are refused.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import prost_amd as prost
from prost_amd import _hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["prost_hip_range_potrs_plan", "prost_hip_range_dinv_elements"] + [
    "prost_hip_range_%s_%s" % (name, s) for name in ("potrf", "potrs", "potrf_workspace_bytes", "potrs_workspace_bytes") for s in ("f32", "f64")]


def _matrix(m=12, n=5, seed=3):
    rng = np.random.default_rng(seed)
    return sp.vstack([sp.identity(n), sp.random(m - n, n, density=0.4, random_state=rng)]).tocsr()


def test_builder_mirrors_the_m_builder():
    A = _matrix()
    AA = (A.T @ A).toarray()
    d = prost.function.ind_range(A, AA)(3, 12)
    assert d[:4] == ["ind_range", 3, 12, False] and d[3] is False and len(d) == 5 and len(d[4]) == 2
    a, aa = d[4]
    assert sp.isspmatrix_csc(a) and a.dtype == np.float64 and a.shape == (12, 5) and np.array_equal(a.toarray(), A.toarray())
    assert isinstance(aa, np.ndarray) and aa.dtype == np.float64 and aa.shape == (5, 5) and np.array_equal(aa, AA)
    # copies: changing the caller's arrays afterwards does not reach the description
    A.data[:] = 0
    AA[:] = 0
    assert a.nnz > 0 and a.toarray().any() and aa.any()
    # other input types: a dense A, a float32 AA, a CSC input (copied, too)
    Ad = _matrix().toarray()
    a2, aa2 = prost.function.ind_range(Ad, (Ad.T @ Ad).astype(np.float32))(0, 12)[4]
    assert sp.isspmatrix_csc(a2) and a2.dtype == np.float64 and aa2.dtype == np.float64
    Ac = sp.csc_matrix(_matrix())
    a3 = prost.function.ind_range(Ac)(0, 12)[4][0]
    Ac.data[:] = 0
    assert a3.toarray().any()
    # AA = None: A'A as a full matrix
    A = _matrix()
    aa4 = prost.function.ind_range(A)(0, 12)[4][1]
    assert isinstance(aa4, np.ndarray) and aa4.dtype == np.float64 and np.array_equal(aa4, (A.T @ A).toarray())
    # a sparse AA is not converted: the factory's message is what the user sees
    saa = sp.csr_matrix((A.T @ A))
    assert prost.function.ind_range(A, saa)(0, 12)[4][1] is saa


@pytest.mark.parametrize("precision", ["single", "double"])
def test_the_name_is_registered(precision):
    prost.set_precision(precision)
    try:
        assert "ind_range" in prost.registered()["prox"]
    finally:
        prost.set_precision("double")


def _problem(desc, size):
    u, q = prost.variable(size), prost.variable(size)
    prob = prost.min_max_problem([u], [q])
    prob.add_function(u, lambda idx, count: desc)
    prob.add_dual_pair(u, q, prost.block.identity())
    return prob


@pytest.mark.parametrize("precision", ["single", "double"])
def test_the_five_messages_of_the_reference(precision):
    A = _matrix()
    AA = (A.T @ A).toarray()
    cases = [(["ind_range", 0, 12, False, [A.toarray(), AA]], "Matrix A must be sparse!"),
             (["ind_range", 0, 13, False, [sp.csc_matrix(A), AA]], "Matrix A does not fit size of the variable!"),
             (["ind_range", 0, 12, False, [sp.csc_matrix(A), sp.csc_matrix(AA)]], "Matrix AA must be dense!"),
             (["ind_range", 0, 12, False, [sp.csc_matrix(A), np.ones((5, 4))]], "ProxIndRange: Matrix 'AA' must be square!"),
             (["ind_range", 0, 12, False, [sp.csc_matrix(A), np.eye(4)]], "ProxIndRange: Matrix 'AA' must fit dimension of 'A'!")]
    prost.set_precision(precision)
    try:
        for desc, message in cases:
            with pytest.raises(prost.ProstError, match=re.escape(message)) as err:
                prost.problem_info(_problem(desc, desc[2]))
            assert "Creating prox with ID 'ind_range' failed" in str(err.value)
        # the builder's own description passes, under the wrappers too
        fun = prost.function.ind_range(A, AA)
        for f in (fun, prost.function.conjugate(fun), prost.function.transform(fun, 2, 1, 1, 0, 0), prost.function.permute(fun, np.arange(12)[::-1])):
            prost.problem_info(_problem(f(0, 12), 12))
        # through the builder a sparse AA reaches the factory
        with pytest.raises(prost.ProstError, match="Matrix AA must be dense!"):
            prost.problem_info(_problem(prost.function.ind_range(A, sp.csc_matrix(AA))(0, 12), 12))
    finally:
        prost.set_precision("double")


def test_header_declares_and_library_exports_the_entry_points():
    header = open(os.path.join(ROOT, "include", "prost_hip.h")).read()
    L = _hip.lib()
    for name in ENTRY_POINTS:
        assert re.search(r"\b%s\(" % name, header), name
        assert hasattr(L, name), name
    assert re.search(r"#define PROST_HIP_ABI_VERSION 10\b", header)
    L.prost_hip_abi_version.restype = C.c_int
    assert L.prost_hip_abi_version() == 10


def _plan(n, dtype):
    L = _hip.lib()
    L.prost_hip_range_potrs_plan.argtypes = [C.c_size_t, C.c_int] + [C.POINTER(C.c_int)] * 3 + [C.POINTER(C.c_size_t)] * 2
    L.prost_hip_range_potrs_plan.restype = C.c_int
    tier, nb, launches, lds, ws = C.c_int(-1), C.c_int(-1), C.c_int(-1), C.c_size_t(0), C.c_size_t(0)
    rc = L.prost_hip_range_potrs_plan(n, dtype, C.byref(tier), C.byref(nb), C.byref(launches), C.byref(lds), C.byref(ws))
    return rc, tier.value, nb.value, launches.value, lds.value, ws.value


def test_plan_is_monotone_and_consistent():
    L = _hip.lib()
    for fn in ("prost_hip_range_potrs_workspace_bytes_f32", "prost_hip_range_potrs_workspace_bytes_f64", "prost_hip_range_dinv_elements"):
        getattr(L, fn).argtypes = [C.c_size_t]
        getattr(L, fn).restype = C.c_size_t
    sizes = sorted(set(list(range(1, 200)) + [255, 256, 257, 511, 512, 513, 1000, 1023, 1024, 1025, 1026, 2047, 2048, 2049, 4096, 10007, 46340]))
    for dtype, elem in ((0, 4), (1, 8)):
        last = None
        nb0 = _plan(1, dtype)[2]
        assert nb0 >= 1
        for n in sizes:
            rc, tier, nb, launches, lds, ws = _plan(n, dtype)
            assert rc == 0, n
            assert tier in (1, 2) and nb == nb0, (n, tier, nb)
            blocks = -(-n // nb)
            if tier == 1:                                              # one launch, the whole (padded) vector in the workgroup's LDS
                assert launches == 1 and blocks * nb * elem <= lds <= 65536, (n, lds)
            else:                                                      # one launch per block step of each sweep
                assert launches == 2 * blocks and 0 < lds <= 65536, (n, launches, lds)
            assert ws >= blocks * nb * elem and ws % 16 == 0, (n, ws)  # the large tier indexes entries 0 .. n - 1 of the workspace
            assert ws == getattr(L, "prost_hip_range_potrs_workspace_bytes_f%d" % (32 if dtype == 0 else 64))(n)
            assert L.prost_hip_range_dinv_elements(n) == blocks * 2 * nb * nb
            if last is not None:
                assert tier >= last[0] and launches >= last[1] and ws >= last[2], (n, last)
            last = (tier, launches, ws)
        assert _plan(1, dtype)[1] == 1 and _plan(46340, dtype)[1] == 2       # both tiers exist
        for n in (0, 46341, 1 << 20, 1 << 40):                             # n * n >= 2^31 (46341^2 = 2147488281)
            assert _plan(n, dtype)[0] != 0, n
        assert L.prost_hip_range_potrs_plan(8, dtype, None, None, None, None, None) == 0
    assert _plan(8, 2)[0] != 0
