"""ind_epi_conjquad_1d without a GPU: the builder, the registry name, the creation errors and the entry points.

  * prost.function.sum_ind_epi_conjquad_1d(interleaved, a, b, c, alpha, beta) describes
    { 'ind_epi_conjquad_1d', idx, size, false, { size / 2, 2, interleaved, { a, b, c, alpha, beta } } };
  * the name is registered for both precisions and a problem that uses it passes prost.problem_info (host only) in both layouts, bare
    and under conjugate / transform, with scalar, vector and infinite coefficients;
  * every refusal of the prox, by its message, each naming the prox;
  * include/prost_hip.h declares the three entry points (and the four scaling passes of the Moreau wrap that read the step on the
    device), the kernel library exports them, the ABI version is still 10;
  * prost_hip_epi_conjquad_step_cap answers for both dtypes without a device and refuses another.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import prost_amd as prost
from prost_amd import _hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["prost_hip_epi_conjquad_step_cap", "prost_hip_prox_ind_epi_conjquad_1d_f32", "prost_hip_prox_ind_epi_conjquad_1d_f64"]
# the scaling passes of the Moreau wrap with the step read on the device: what keeps conjugate(sum_ind_epi_conjquad_1d(..)) on the
# device-resident step-size rule
MOREAU_VIEW = ["prost_hip_moreau_%sscale_view_%s" % (w, t) for w in ("pre", "post") for t in ("f32", "f64")]
COUNT = 6


def _coeffs(seed=3):
    rng = np.random.default_rng(seed)
    lo = rng.standard_normal(COUNT)
    return rng.uniform(0.5, 2, COUNT), rng.standard_normal(COUNT), rng.standard_normal(COUNT), lo, lo + rng.uniform(0, 2, COUNT)


def test_builder_description_cell_by_cell():
    co = _coeffs()
    for il in (False, True, 0, 1):
        d = prost.function.sum_ind_epi_conjquad_1d(il, *co)(7, 2 * COUNT)
        assert len(d) == 5 and d[0] == "ind_epi_conjquad_1d" and d[1] == 7 and d[2] == 2 * COUNT and d[3] is False
        data = d[4]
        assert len(data) == 4 and data[0] == COUNT and data[1] == 2 and data[2] is bool(il)
        assert len(data[3]) == 5
        for got, want in zip(data[3], co):
            assert isinstance(got, np.ndarray) and got.dtype == np.float64 and got.ndim == 1 and np.array_equal(got, want)
    # scalars become vectors of one entry, lists and integer arrays float64 vectors, infinities survive
    d = prost.function.sum_ind_epi_conjquad_1d(True, 1, list(co[1]), np.arange(COUNT), -np.inf, float("inf"))(0, 2 * COUNT)
    shapes = [v.shape for v in d[4][3]]
    assert shapes == [(1,), (COUNT,), (COUNT,), (1,), (1,)] and all(v.dtype == np.float64 for v in d[4][3])
    assert d[4][3][3][0] == -np.inf and d[4][3][4][0] == np.inf


@pytest.mark.parametrize("precision", ["single", "double"])
def test_the_name_is_registered(precision):
    prost.set_precision(precision)
    try:
        assert "ind_epi_conjquad_1d" in prost.registered()["prox"]
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
    a, b, c, lo, hi = _coeffs()
    size = 2 * COUNT
    prost.set_precision(precision)
    try:
        for il in (False, True):
            for co in ((a, b, c, lo, hi), (1.0, 0.0, 0.0, -1.0, 2.0), (a, 0.5, c, -np.inf, hi), (a, b, 0.0, lo, np.inf), (2.0, b, c, -np.inf, np.inf),
                       (0.0, b, c, lo, hi), (np.r_[0.0, a[1:]], b, c, lo, lo)):
                fun = F.sum_ind_epi_conjquad_1d(il, *co)
                for f in (fun, F.conjugate(fun), F.transform(fun, 2, 1, 1, 0, 0)):
                    assert prost.problem_info(_problem(f(0, size), size))["ncols"] == size
    finally:
        prost.set_precision("double")


@pytest.mark.parametrize("precision", ["single", "double"])
def test_every_refusal_by_message(precision):
    a, b, c, lo, hi = _coeffs()

    def desc(count=COUNT, size=2 * COUNT, dim=2, a=a, b=b, c=c, alpha=lo, beta=hi):
        return ["ind_epi_conjquad_1d", 0, size, False, [count, dim, True, [np.atleast_1d(np.asarray(v, float)) for v in (a, b, c, alpha, beta)]]]

    def at(v, g, value):
        v = np.array(v, float)
        v[g] = value
        return v

    cases = [
        (desc(a=at(a, 2, -0.5)), "ProxIndEpiConjQuad1D: a = -0.5 is negative, the piece has to be convex (group 2)."),
        (desc(a=-1.0), "ProxIndEpiConjQuad1D: a = -1 is negative, the piece has to be convex (group 0)."),
        (desc(alpha=at(lo, 4, hi[4] + 1)), "is above beta"),
        (desc(alpha=3.0, beta=2.0), "ProxIndEpiConjQuad1D: alpha = 3 is above beta = 2 (group 0)."),
        (desc(a=at(a, 1, np.nan)), "ProxIndEpiConjQuad1D: a, b and c have to be finite (group 1)."),
        (desc(a=at(a, 1, np.inf)), "ProxIndEpiConjQuad1D: a, b and c have to be finite (group 1)."),
        (desc(b=at(b, 5, -np.inf)), "ProxIndEpiConjQuad1D: a, b and c have to be finite (group 5)."),
        (desc(c=np.nan), "ProxIndEpiConjQuad1D: a, b and c have to be finite (group 0)."),
        (desc(alpha=at(lo, 3, np.nan)), "ProxIndEpiConjQuad1D: alpha has to be finite or -inf and beta finite or +inf (group 3)."),
        (desc(beta=at(hi, 3, np.nan)), "ProxIndEpiConjQuad1D: alpha has to be finite or -inf and beta finite or +inf (group 3)."),
        (desc(alpha=np.inf, beta=np.inf), "ProxIndEpiConjQuad1D: alpha has to be finite or -inf and beta finite or +inf (group 0)."),
        (desc(alpha=-np.inf, beta=-np.inf), "ProxIndEpiConjQuad1D: alpha has to be finite or -inf and beta finite or +inf (group 0)."),
        (desc(a=at(a, 2, 0.0), alpha=at(lo, 2, -np.inf)), "ProxIndEpiConjQuad1D: a = 0 needs finite alpha and beta (group 2)."),
        (desc(a=0.0, beta=np.inf), "ProxIndEpiConjQuad1D: a = 0 needs finite alpha and beta (group 0)."),
        (desc(a=a[:5]), "ProxIndEpiConjQuad1D: coefficient a has 5 entries, expected 1 or count = 6."),
        (desc(b=np.r_[b, 0.0]), "ProxIndEpiConjQuad1D: coefficient b has 7 entries, expected 1 or count = 6."),
        (desc(c=c[:2]), "ProxIndEpiConjQuad1D: coefficient c has 2 entries, expected 1 or count = 6."),
        (desc(alpha=lo[:3]), "ProxIndEpiConjQuad1D: coefficient alpha has 3 entries, expected 1 or count = 6."),
        (desc(beta=np.zeros(0)), "ProxIndEpiConjQuad1D: coefficient beta has 0 entries, expected 1 or count = 6."),
        (desc(count=5), "ProxIndEpiConjQuad1D: size = 12 is not 2 * count = 2 * 5."),
        (desc(size=13), "ProxIndEpiConjQuad1D: size = 13 is not 2 * count = 2 * 6."),
        (desc(dim=3, size=18), "ProxIndEpiConjQuad1D: dim = 3 is not supported, a group is (y, t): dim has to be 2."),
    ]
    prost.set_precision(precision)
    try:
        for d, message in cases:
            with pytest.raises(prost.ProstError, match=re.escape(message)) as err:
                prost.problem_info(_problem(d, d[2]))
            assert "Creating prox with ID 'ind_epi_conjquad_1d' failed" in str(err.value)
        prost.problem_info(_problem(desc(), 2 * COUNT))
    finally:
        prost.set_precision("double")


def test_header_declares_and_library_exports_the_entry_points():
    header = open(os.path.join(ROOT, "include", "prost_hip.h")).read()
    L = _hip.lib()
    for name in ENTRY_POINTS + MOREAU_VIEW:
        assert re.search(r"\b%s\(" % name, header), name
        assert hasattr(L, name), name
    assert re.search(r"#define PROST_HIP_ABI_VERSION 10\b", header)
    L.prost_hip_abi_version.restype = C.c_int
    assert L.prost_hip_abi_version() == 10


def test_step_cap_answers_without_a_device():
    L = _hip.lib()
    L.prost_hip_epi_conjquad_step_cap.argtypes = [C.c_int, C.POINTER(C.c_int)]
    L.prost_hip_epi_conjquad_step_cap.restype = C.c_int
    caps = []
    for dtype in (0, 1):
        cap = C.c_int(-1)
        assert L.prost_hip_epi_conjquad_step_cap(dtype, C.byref(cap)) == 0
        assert 8 <= cap.value <= 1024, cap.value
        caps.append(cap.value)
        assert L.prost_hip_epi_conjquad_step_cap(dtype, None) == 0
    for dtype in (-1, 2, 7):
        cap = C.c_int(-1)
        assert L.prost_hip_epi_conjquad_step_cap(dtype, C.byref(cap)) != 0 and cap.value == -1
    text = open(os.path.join(ROOT, "include", "prost", "prox", "epi_conjquad.hpp")).read()
    assert int(re.search(r"constexpr int kStepCap = (\d+);", text).group(1)) in caps
