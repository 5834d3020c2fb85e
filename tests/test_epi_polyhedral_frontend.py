"""ind_epi_polyhedral without a GPU: the builder, the registry name, the creation errors and the launch plan.

  * prost.function.sum_ind_epi_polyhedral(dim, interleaved, a, b, count_vec, index_vec) describes
    { 'ind_epi_polyhedral', idx, count, false, { count / dim, dim, interleaved, { a, b, count_vec, index_vec } } };
  * the name is registered for both precisions and a problem that uses it passes prost.problem_info (host only), bare and under
    conjugate / transform / permute;
  * every argument check of the prox, by its message, each naming the prox;
  * include/prost_hip.h declares the entry points, the kernel library exports them, the ABI version is still 10;
  * prost_hip_epi_polyhedral_plan: lanes per group a power of two <= 64 and non-decreasing in max_count, a lane never owns more
    than a handful of constraints until the wave is full, caps positive, other dims / dtypes refused; no device needed.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import prost_amd as prost
from prost_amd import _hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["prost_hip_epi_polyhedral_plan", "prost_hip_prox_ind_epi_polyhedral_f32", "prost_hip_prox_ind_epi_polyhedral_f64"]


def _lists(count=6, dim=3, m=4, seed=5):
    rng = np.random.default_rng(seed)
    a = rng.standard_normal(count * m * (dim - 1))
    b = rng.standard_normal(count * m)
    return a, b, np.full(count, m), np.arange(count) * m


def test_builder_description_cell_by_cell():
    a, b, cv, iv = _lists()
    for il in (False, True, 0, 1):
        d = prost.function.sum_ind_epi_polyhedral(3, il, a, b, cv, iv)(7, 18)
        assert len(d) == 5 and d[0] == "ind_epi_polyhedral" and d[1] == 7 and d[2] == 18 and d[3] is False
        data = d[4]
        assert len(data) == 4 and data[0] == 6 and data[1] == 3 and data[2] is bool(il)
        co = data[3]
        assert len(co) == 4
        for got, want in zip(co, (a, b, cv, iv)):
            assert isinstance(got, np.ndarray) and got.dtype == np.float64 and got.ndim == 1 and np.array_equal(got, want)
    # lists, 2-D input and integer arrays are flattened into float64 vectors; a matrix of rows per constraint keeps its row order
    d = prost.function.sum_ind_epi_polyhedral(3, False, a.reshape(-1, 2).tolist(), list(b), cv.astype(np.int32), iv.astype(np.int64))(0, 18)
    assert np.array_equal(d[4][3][0], a) and np.array_equal(d[4][3][2], cv) and d[4][3][3].dtype == np.float64


@pytest.mark.parametrize("precision", ["single", "double"])
def test_the_name_is_registered(precision):
    prost.set_precision(precision)
    try:
        assert "ind_epi_polyhedral" in prost.registered()["prox"]
    finally:
        prost.set_precision("double")


def _problem(desc, size):
    u, q = prost.variable(size), prost.variable(size)
    prob = prost.min_max_problem([u], [q])
    prob.add_function(u, lambda idx, count: desc)
    prob.add_dual_pair(u, q, prost.block.identity())
    return prob


@pytest.mark.parametrize("precision", ["single", "double"])
def test_problem_info_accepts_the_builders_description(precision):
    F = prost.function
    prost.set_precision(precision)
    try:
        for dim in (2, 3, 4):
            a, b, cv, iv = _lists(dim=dim)
            size = 6 * dim
            for il in (False, True):
                fun = F.sum_ind_epi_polyhedral(dim, il, a, b, cv, iv)
                for f in (fun, F.conjugate(fun), F.transform(fun, 2, 1, 1, 0, 0), F.permute(fun, np.arange(size)[::-1])):
                    info = prost.problem_info(_problem(f(0, size), size))
                    assert info["ncols"] == size
        # shared lists, a non-monotone index_vec, empty groups, no constraints at all
        a, b, _, _ = _lists()
        prost.problem_info(_problem(F.sum_ind_epi_polyhedral(3, False, a[:8], b[:4], np.full(6, 4), np.zeros(6))(0, 18), 18))
        prost.problem_info(_problem(F.sum_ind_epi_polyhedral(3, False, a, b, [4, 0, 4, 1, 0, 2], [20, 3, 0, 23, 24, 8])(0, 18), 18))
        prost.problem_info(_problem(F.sum_ind_epi_polyhedral(3, False, [], [], np.zeros(6), np.zeros(6))(0, 18), 18))
    finally:
        prost.set_precision("double")


@pytest.mark.parametrize("precision", ["single", "double"])
def test_every_validation_error_by_message(precision):
    a, b, cv, iv = _lists()

    def desc(dim=3, count=6, size=18, a=a, b=b, cv=cv, iv=iv):
        return ["ind_epi_polyhedral", 0, size, False, [count, dim, False, [np.asarray(a, float), np.asarray(b, float), np.asarray(cv, float), np.asarray(iv, float)]]]

    big = float(2 ** 31)
    cases = [
        (desc(dim=5, count=6, size=30), "ProxIndEpiPolyhedral: dim = 5 is not supported, dim has to be between 2 and 4."),
        (desc(dim=1, count=18), "ProxIndEpiPolyhedral: dim = 1 is not supported, dim has to be between 2 and 4."),
        (desc(count=5), "ProxIndEpiPolyhedral: size = 18 is not count * dim = 5 * 3."),
        (desc(cv=cv[:5]), "ProxIndEpiPolyhedral: count_vec and index_vec need one entry per group (count = 6, got 5 and 6)."),
        (desc(iv=np.r_[iv, 0]), "ProxIndEpiPolyhedral: count_vec and index_vec need one entry per group (count = 6, got 6 and 7)."),
        (desc(a=a[:-1]), "ProxIndEpiPolyhedral: a has 47 entries, expected len(b) * (dim - 1) = 48."),
        (desc(b=b[:-1]), "ProxIndEpiPolyhedral: a has 48 entries, expected len(b) * (dim - 1) = 46."),
        (desc(cv=[4, 4, 4, 4, 4, 5]), "ProxIndEpiPolyhedral: group 5 names constraints 20 .. 25, but there are only 24."),
        (desc(iv=[0, 4, 8, 12, 21, 16]), "ProxIndEpiPolyhedral: group 4 names constraints 21 .. 25, but there are only 24."),
        (desc(cv=[4, -1, 4, 4, 4, 4]), "ProxIndEpiPolyhedral: count_vec and index_vec have to hold non-negative integers below 2^31 (group 1)."),
        (desc(iv=[0, 4, 8.5, 12, 16, 20]), "ProxIndEpiPolyhedral: count_vec and index_vec have to hold non-negative integers below 2^31 (group 2)."),
        (desc(cv=[4, 4, 4, np.nan, 4, 4]), "ProxIndEpiPolyhedral: count_vec and index_vec have to hold non-negative integers below 2^31 (group 3)."),
        (desc(iv=[big, 4, 8, 12, 16, 20]), "ProxIndEpiPolyhedral: count_vec and index_vec have to hold non-negative integers below 2^31 (group 0)."),
        (desc(cv=[4, 4, 4, 4, 4, big]), "ProxIndEpiPolyhedral: count_vec and index_vec have to hold non-negative integers below 2^31 (group 5)."),
    ]
    prost.set_precision(precision)
    try:
        for d, message in cases:
            with pytest.raises(prost.ProstError, match=re.escape(message)) as err:
                prost.problem_info(_problem(d, d[2]))
            assert "Creating prox with ID 'ind_epi_polyhedral' failed" in str(err.value)
        prost.problem_info(_problem(desc(), 18))
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


def _plan(max_count, dim, dtype):
    L = _hip.lib()
    L.prost_hip_epi_polyhedral_plan.argtypes = [C.c_size_t, C.c_size_t, C.c_int] + [C.POINTER(C.c_int)] * 3
    L.prost_hip_epi_polyhedral_plan.restype = C.c_int
    lanes, ca, cb = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    rc = L.prost_hip_epi_polyhedral_plan(max_count, dim, dtype, C.byref(lanes), C.byref(ca), C.byref(cb))
    return rc, lanes.value, ca.value, cb.value


def test_plan_lanes_and_caps():
    counts = list(range(0, 300)) + [511, 512, 513, 1000, 4096, 10 ** 6, 2 ** 31 - 1]
    for dtype in (0, 1):
        for dim in (2, 3, 4):
            last = 0
            caps = None
            for m in counts:
                rc, lanes, ca, cb = _plan(m, dim, dtype)
                assert rc == 0, (m, dim, dtype)
                assert 1 <= lanes <= 64 and lanes & (lanes - 1) == 0, (m, lanes)
                assert lanes >= last, (m, lanes, last)
                last = lanes
                assert ca >= 1 and cb >= 0 and ca * (m + dim) + cb >= 1, (ca, cb)
                assert caps in (None, (ca, cb))
                caps = (ca, cb)
            assert _plan(0, dim, dtype)[1] == 1 and _plan(1, dim, dtype)[1] == 1 and _plan(10 ** 6, dim, dtype)[1] == 64     # both ends exist
            # until the wave is full no lane scans more than a fixed handful of constraints
            share = max(-(-m // _plan(m, dim, dtype)[1]) for m in range(1, 257) if _plan(m, dim, dtype)[1] < 64)
            assert share <= 8, share
            assert _plan(2 ** 31, dim, dtype)[0] != 0
            assert _hip.lib().prost_hip_epi_polyhedral_plan(8, dim, dtype, None, None, None) == 0
        for dim in (0, 1, 5, 9):
            assert _plan(8, dim, dtype)[0] != 0, dim
    assert _plan(8, 3, 2)[0] != 0
