"""The CPU oracle's projection proxes (ind_halfspace, ind_soc, elem_operation:ind_simplex, elem_operation:ind_sum, the index-family
ind_sum) on the directed operands of tests/prox_wrap_cases.py: operands ON the branches and one ulp either side, zero normals, ties in
the sort, dims either side of the Shell-sort gaps, NaN, infinities, overflow and underflow.

 * every finite in-range group is within the forward-error bound of the float64 reference, entries no group touches are bit-identical;
 * ind_simplex and elem ind_sum are pinned to the reference's own functors (ElemOperationIndSimplex, ElemOperationIndSum), whose answers
   tests/golden/prox_wrap_edges.npz stores as one digest per case (tests/golden/make_golden.py wrap_edges); where oracle/_ref is built
   with these functors (ref.has_nocoeff) their live answers must match the same record.  The NaN groups are part of it: what the functor returns for them is what the
   oracle must return.  Halfspace, cone and index families are kernels inside the reference's .cu files: the float64 reference is
   their witness.
No GPU.  The worst error-to-bound ratio per prox and data type is printed (pytest -s).
"""
import functools
import os

import numpy as np
import pytest

import oracle
import prost_amd as prost
import prox_wrap_cases as W
from oracle import ref
from test_oracle_pinning import GOLD, answer_digest

F = prost.function
# per data type: halfspace 5 dims x 4 counts x 6 normals x 3 kinds of b; cone 4 dims x (3 + 3 + 1 + 1); simplex 14 dims x 4 counts x 2
# layouts; elem ind_sum 3 dims x 4 counts x 2 layouts; index families 3 dims x 4 counts x (2 orders x 3 sums x 2 step flags + the two-family form)
CASES_PER_KIND = {"halfspace": 360, "soc": 32, "simplex": 112, "elem_sum": 24, "ind_sum": 156}


def oracle_answer(case):
    """the oracle on the case, in T"""
    c = case
    if c.kind == "ind_sum" and len(c.families) == 1:          # the step flag as given; Prox::Eval would reach invert_tau only under a Moreau wrap
        dim, inds, s = c.families[0]
        return oracle.prox_ind_sum(c.arg, c.tau_diag, inds, dim, s, c.tau, c.invert)
    return oracle.eval_prox(W.prox_function(F, c), c.arg, c.tau, c.tau_diag, c.dtype).astype(c.dtype)


@functools.lru_cache(maxsize=None)
def _record():
    g = np.load(os.path.join(GOLD, "prox_wrap_edges.npz"))
    return {k.decode(): bytes(d).hex() for k, d in zip(g["digest_keys"], g["digests"])}


def test_the_directed_groups_are_there():
    """the operands sit on the branches: halfspace excess exactly 0 in T, cone norm exactly +-y, simplex ties / points on the simplex /
    vertices, sums exactly on target; and the special values are present"""
    for dt in W.DTYPES:
        counts = dict.fromkeys(CASES_PER_KIND, 0)
        on_plane = on_cone = on_polar = zero_normal = zero_neg = on_simplex = vertices = nan_groups = exact_sums = 0
        for name, c in [nc for k in sorted(CASES_PER_KIND) for nc in W.case_list(dt, k)]:
            counts[c.kind] += 1
            g = c.groups()
            nan_groups += int(np.isnan(g).any(axis=1).sum())
            with np.errstate(all="ignore"):
                if c.kind == "halfspace":
                    d = np.array([W._seq_dot(c.a[t], g[t]) for t in range(c.count)])
                    on_plane += int(((d == c.b) & (c.a != 0).any(axis=1)).sum())
                    zero_normal += int((c.a == 0).all(axis=1).sum())
                if c.kind == "soc":
                    n = np.array([np.sqrt(W._seq_dot(x, x)) for x in g[:, :-1]])
                    on_cone += int(((n == g[:, -1]) & (n > 0)).sum()); on_polar += int(((n == -g[:, -1]) & (n > 0)).sum())
                    zero_neg += int(((n == 0) & (g[:, -1] < 0) & (c.dim > 1)).sum())
                if c.kind == "simplex":
                    g64 = g.astype(np.float64)
                    on_simplex += int(((g64.min(axis=1) >= 0) & (g64.sum(axis=1) == 1)).sum())
                    vertices += int((g.max(axis=1) == 5).sum())
                if c.kind in ("elem_sum", "ind_sum"):
                    exact_sums += int((g.astype(np.float64).sum(axis=1) == (1.0 if c.kind == "elem_sum" else c.s)).sum())
        assert counts == CASES_PER_KIND, counts
        assert min(on_plane, on_cone, on_polar, zero_normal, zero_neg, on_simplex, vertices, nan_groups, exact_sums) >= 20, \
            (on_plane, on_cone, on_polar, zero_normal, zero_neg, on_simplex, vertices, nan_groups, exact_sums)


@pytest.mark.parametrize("dtype", W.DTYPES)
@pytest.mark.parametrize("kind", sorted(CASES_PER_KIND))
def test_oracle_is_within_the_bound_of_the_float64_reference(dtype, kind):
    worst, where, n = 0.0, None, 0
    for name, c in W.case_list(dtype, kind):
        got = oracle_answer(c)
        q = W.ratio_to_bound(c, got)
        if q > worst:
            worst, where = q, name
        assert q <= 1.0, (name, q)
        assert np.array_equal(got[c.untouched()].view(np.uint8), c.arg[c.untouched()].view(np.uint8)), name
        n += 1
    print("%s %s: %d cases, worst error / bound %.3f (%s)" % (kind, np.dtype(dtype).name, n, worst, where))
    assert n == CASES_PER_KIND[kind]


@pytest.mark.parametrize("dtype", W.DTYPES)
def test_special_groups_of_the_oracle(dtype):
    """a zero normal gives NaN whatever the sign of b, as the reference's division does; x = 0 with y < 0 projects onto exactly 0 (none
    of the three branches divides there); a NaN stays inside its own group"""
    for name, c in W.case_list(dtype, "halfspace") + W.case_list(dtype, "soc"):
        got = c.groups(oracle_answer(c))
        g = c.groups()
        with np.errstate(invalid="ignore"):
            if c.kind == "halfspace":
                zn = (c.a == 0).all(axis=1)
                assert np.isnan(got[zn]).all(), name
                clean = np.isfinite(g).all(axis=1) & c.in_range()
                assert np.isfinite(got[clean & ~zn]).all(), name
            else:
                zneg = (g[:, :-1] == 0).all(axis=1) & (g[:, -1] < 0)
                assert (got[zneg] == 0).all(), name
                assert np.isfinite(got[c.in_range()]).all(), name


@pytest.mark.parametrize("dtype", W.DTYPES)
def test_oracle_equals_the_reference_functors(dtype):
    rec = _record()
    checked = 0
    for name, c in W.case_list(dtype, "simplex") + W.case_list(dtype, "elem_sum"):
        answers = [("oracle", oracle_answer(c))]
        if ref.has_nocoeff():
            answers.append(("live reference", ref.prox_elem_nocoeff({"simplex": "ind_simplex", "elem_sum": "ind_sum"}[c.kind], c.arg, c.count, c.dim, c.interleaved)))
        for who, a in answers:
            assert answer_digest(a) == rec[name], (who, name)
        checked += 1
    assert checked == CASES_PER_KIND["simplex"] + CASES_PER_KIND["elem_sum"]
    assert len(rec) == 2 * checked


def test_a_nan_group_of_the_simplex_stays_nan():
    """the planar group (nan, -0.2, 0.1, 0.2): the host build of the reference's functor ends in std::max(val - tmax, 0), whose first
    argument wins when it is a NaN, and returns four NaNs (the digests above hold that); nothing turns the group into a feasible point"""
    for dt in W.DTYPES:
        got = oracle.eval_prox(F.sum_ind_simplex(4, False), np.array([np.nan, -0.2, 0.1, 0.2]), 1.0, np.ones(4), dt)
        assert np.isnan(got).all()
