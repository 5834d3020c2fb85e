"""GPU parity of the projection and wrapper proxes of kernels_prox_wrap.hip at their branches and special values.

 1. every case of tests/prox_wrap_cases.py (operands ON the branches of ind_halfspace / ind_soc and one ulp either side, zero normals,
    simplex groups with ties, on the simplex, at a vertex, with dims either side of the Shell-sort gaps, sums exactly on target, NaN,
    infinities, overflow, underflow; 1, 3, 67 and 260 groups) through prost.eval_prox, plain and under conjugate, against the CPU oracle:
    np.array_equal(got, want, equal_nan=True), the sign of a zero not compared (as in tests/test_gpu_elementwise_edges.py).  The finite
    in-range groups are also held to the float64 reference within the forward-error bounds of the case module, so this file stands on
    its own if the oracle changes.  tests/test_prox_wrap_edges.py pins the oracle on the same cases.
 2. the index-family kernel at its C entry point with the step flag off and on (Prox::Eval reaches invert_tau only under conjugate).
 3. transform prescale / postscale and permute at their C entry points: sizes 1, 3, 5, 65, 260 with every pointer on a 16-byte
    boundary (transform_prescale_kernel<T, VEC> with a tail of 1 to 3 elements) and one element behind it (<T, 1> at n >= VEC), the 32
    pointer-or-scalar mixes of the five coefficients, the four postscale functors, a canary behind the last element.  Expected values
    come from numpy in T, operation for operation.
"""
import ctypes as C
import itertools

import numpy as np
import pytest

import oracle
import prost_amd as prost
import prox_wrap_cases as W
from test_gpu_elementwise_edges import Upload
from test_prox_wrap_edges import CASES_PER_KIND, oracle_answer

pytestmark = pytest.mark.gpu
F = prost.function
PRECISION = {np.float32: "single", np.float64: "double"}
SIZES = (1, 3, 5, 65, 260)
PAD = 4                     # elements behind every buffer: the canary of the outputs


@pytest.fixture(autouse=True)
def _gpu(hip):
    prost.set_gpu(0)
    yield
    prost.set_precision("double")


def differing(got, want):
    return np.flatnonzero(~((got == want) | (np.isnan(got) & np.isnan(want))))


# ---- 1. the projections through the product path ---------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", W.DTYPES)
@pytest.mark.parametrize("kind", sorted(CASES_PER_KIND))
def test_projections_on_directed_operands(dtype, kind):
    prost.set_precision(PRECISION[dtype])
    worst, where, n = 0.0, None, 0
    for name, c in W.case_list(dtype, kind):
        if c.invert:
            continue                                               # the step flag on its own: test_index_family_kernel_with_both_step_flags
        fn = W.prox_function(F, c)
        got, _ = prost.eval_prox(fn, c.arg, c.tau, c.tau_diag)
        got = np.asarray(got, dtype=np.float64).reshape(-1)
        want = oracle_answer(c).astype(np.float64)
        assert np.array_equal(got, want, equal_nan=True), (name, differing(got, want)[:8], got[differing(got, want)[:4]], want[differing(got, want)[:4]])
        q = W.ratio_to_bound(c, got)
        if q > worst:
            worst, where = q, name
        assert q <= 1.0, (name, q)
        assert np.array_equal(got[c.untouched()], c.arg[c.untouched()].astype(np.float64)), name
        conj, _ = prost.eval_prox(F.conjugate(fn), c.arg, c.tau, c.tau_diag)
        conj = np.asarray(conj, dtype=np.float64).reshape(-1)
        want = oracle.eval_prox(F.conjugate(fn), c.arg, c.tau, c.tau_diag, dtype)
        assert np.array_equal(conj, want, equal_nan=True), (name, "conjugate", differing(conj, want)[:8])
        n += 1
    print("%s %s: %d cases, worst error / bound %.3f (%s)" % (kind, np.dtype(dtype).name, n, worst, where))
    assert n == CASES_PER_KIND[kind] - (72 if kind == "ind_sum" else 0)


def test_a_nan_group_of_the_simplex_stays_nan():
    """the planar group (nan, -0.2, 0.1, 0.2) between two clean groups: four NaNs, as the oracle and the reference's functor return, and
    the neighbours in the same wave are projected as if it were not there"""
    groups = np.array([[0.3, 0.9, -0.2, 0.1], [np.nan, -0.2, 0.1, 0.2], [1.5, 0.25, 0.25, -3.0]])
    for dt in W.DTYPES:
        prost.set_precision(PRECISION[dt])
        for il in (False, True):
            arg = (groups if il else groups.T).reshape(-1)
            got, _ = prost.eval_prox(F.sum_ind_simplex(4, il), arg, 1.0, np.ones(12))
            got = np.asarray(got).reshape((3, 4) if il else (4, 3))
            got = got if il else got.T
            assert np.isnan(got[1]).all(), (dt, il, got)
            for t in (0, 2):
                assert np.abs(got[t] - W.projsplx(groups[t].astype(dt).astype(np.float64))).max() <= 16 * np.finfo(dt).eps * 3, (dt, il, t)


# ---- 2. the index-family kernel ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", W.DTYPES)
def test_index_family_kernel_with_both_step_flags(hip, dtype):
    f = hip.fn("prox_ind_sum", dtype)
    f.argtypes = [C.c_void_p] * 4 + [C.c_size_t, C.c_size_t, C.c_double, C.c_double, C.c_int, C.c_void_p]
    worst, ran = 0.0, {False: 0, True: 0}
    for name, c in W.case_list(dtype, "ind_sum"):
        if len(c.families) != 1:
            continue
        dim, inds, s = c.families[0]
        up = Upload(hip, 0)
        res = hip.DeviceArray.from_host(c.arg)                     # res already holds a copy of arg
        hip.check(f(res.ptr, up(c.arg), up(c.tau_diag), up(inds.astype(np.uint64)), c.count, dim, s, c.tau, int(c.invert), None))
        got = res.to_host()
        res.free(); up.free()
        want = oracle_answer(c)
        assert np.array_equal(got, want, equal_nan=True), (name, differing(got, want)[:8])
        assert np.array_equal(got[c.untouched()].view(np.uint8), c.arg[c.untouched()].view(np.uint8)), name
        q = W.ratio_to_bound(c, got)
        assert q <= 1.0, (name, q)
        worst = max(worst, q)
        ran[c.invert] += 1
    print("ind_sum kernel %s: worst error / bound %.3f" % (np.dtype(dtype).name, worst))
    assert ran == {False: 72, True: 72}


# ---- 3. transform and permute at the C entry points --------------------------------------------------------------------------------
def transform_operands(dtype, n, seed):
    """x with a NaN, an infinity and a zero among ordinary values (n >= 5), step sizes and the five coefficient vectors; e > 0 and a != 0"""
    rng = np.random.default_rng([n, seed, np.dtype(dtype).itemsize])
    x = rng.standard_normal(n).astype(dtype)
    if n >= 5:
        x[[1, 2, n - 1]] = (np.nan, np.inf, 0.0)
    td = rng.uniform(0.1, 2, n).astype(dtype)
    vec = [rng.uniform(0.3, 2, n).astype(dtype) * s for s in (-1, 1, 1, -1, 1)]
    return x, td, vec


def expected_prescale(dtype, x, td, cf, tau, invert):
    """(a (x - t d)) / (1 + t e) - b and (a a c t) / (1 + t e) with t = tau tau_diag or 1 / (tau tau_diag), every operation rounded to T"""
    a, b, c, d, e = cf
    with np.errstate(all="ignore"):
        t = dtype(tau) * td
        if invert:
            t = dtype(1) / t
        return (a * (x - t * d)) / (dtype(1) + t * e) - b, (a * a * c * t) / (dtype(1) + t * e)


@pytest.mark.parametrize("dtype", W.DTYPES)
def test_transform_prescale_entry_point(hip, dtype):
    f = hip.fn("transform_prescale", dtype)
    f.argtypes = [C.c_void_p] * 6 + [C.c_double, C.c_int, C.c_size_t, C.c_void_p]
    scal = (1.5, 0.25, 0.75, -0.5, 0.3)
    pad = np.full(PAD, 3.0, dtype)
    launches = 0
    for n, off in itertools.product(SIZES, (0, 1)):
        mixes = list(itertools.product((False, True), repeat=5)) if n == 65 else [(True,) * 5, (False,) * 5, (True, False, True, False, True)]
        x, td, vec = transform_operands(dtype, n, off)
        for mix, invert in itertools.product(mixes, (False, True)):
            up = Upload(hip, off)
            ptrs, vals = (C.c_void_p * 5)(), (C.c_double * 5)(*scal)
            cf = []
            for k in range(5):
                ptrs[k] = up(np.concatenate([vec[k], pad])).value if mix[k] else None
                cf.append(vec[k] if mix[k] else dtype(scal[k]))
            sa, sap = up.result(n + PAD, dtype)
            st, stp = up.result(n + PAD, dtype)
            hip.check(f(sap, stp, up(np.concatenate([x, pad])), up(np.concatenate([td, pad])), ptrs if any(mix) else None, vals, 0.7, int(invert), n, None))
            want = expected_prescale(dtype, x, td, cf, 0.7, invert)
            for who, d, w in (("argument", sa, want[0]), ("step", st, want[1])):
                got = d.to_host()
                assert (got[:off] == 7.0).all() and (got[off + n:] == 7.0).all(), (who, n, off, mix, got[off + n:])
                assert np.array_equal(got[off:off + n], w, equal_nan=True), (who, n, off, mix, invert, differing(got[off:off + n], w)[:8])
            up.free()
            launches += 1
    assert launches == 2 * 2 * (4 * 3 + 32)


@pytest.mark.parametrize("dtype", W.DTYPES)
def test_transform_postscale_entry_point(hip, dtype):
    f = hip.fn("transform_postscale", dtype)
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_double, C.c_size_t, C.c_void_p]
    pad = np.full(PAD, 3.0, dtype)
    launches = 0
    for n, off in itertools.product(SIZES, (0, 1)):
        x, _, vec = transform_operands(dtype, n, 2 + off)
        for a_ptr, b_ptr in itertools.product((False, True), repeat=2):          # TransformPostSF, BF, AF, F
            up = Upload(hip, off)
            buf = np.concatenate([np.full(off, 7.0, dtype), x, np.full(PAD, 7.0, dtype)])
            r = hip.DeviceArray.from_host(buf)
            a = vec[0] if a_ptr else dtype(-1.25)
            b = vec[1] if b_ptr else dtype(0.375)
            hip.check(f(r.offset(off), up(np.concatenate([vec[0], pad])) if a_ptr else None, -1.25, up(np.concatenate([vec[1], pad])) if b_ptr else None, 0.375, n, None))
            got = r.to_host()
            r.free(); up.free()
            with np.errstate(all="ignore"):
                want = (x + b) / a
            assert (got[:off] == 7.0).all() and (got[off + n:] == 7.0).all(), (n, off, a_ptr, b_ptr)
            assert np.array_equal(got[off:off + n], want, equal_nan=True), (n, off, a_ptr, b_ptr, differing(got[off:off + n], want)[:8])
            launches += 1
    assert launches == 5 * 2 * 4


@pytest.mark.parametrize("dtype", W.DTYPES)
def test_permute_entry_point(hip, dtype):
    f = hip.fn("permute", dtype)
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    for n, off in itertools.product(SIZES, (0, 1)):
        rng = np.random.default_rng([n, off])
        x = rng.standard_normal(n).astype(dtype)
        if n >= 5:
            x[[0, 3]] = (np.nan, -0.0)
        forward = rng.permutation(n)
        inverse = np.empty(n, np.int64); inverse[forward] = np.arange(n)
        for perm in (np.arange(n), np.arange(n)[::-1].copy(), forward, inverse):
            up = Upload(hip, off)
            d_perm, d_x = up(perm.astype(np.int32)), up(x)
            gathered, gp = up.result(n + PAD, dtype)
            hip.check(f(gp, d_x, d_perm, n, 0, None))
            g = gathered.to_host()
            assert (g[:off] == 7.0).all() and (g[off + n:] == 7.0).all(), (n, off)
            assert np.array_equal(g[off:off + n].view(np.uint8), x[perm].view(np.uint8)), (n, off)
            scattered, sp = up.result(n + PAD, dtype)
            hip.check(f(sp, d_x, d_perm, n, 1, None))
            s = scattered.to_host()
            want = np.empty_like(x); want[perm] = x
            assert (s[:off] == 7.0).all() and (s[off + n:] == 7.0).all(), (n, off)
            assert np.array_equal(s[off:off + n].view(np.uint8), want.view(np.uint8)), (n, off)
            back, bp = up.result(n + PAD, dtype)                   # permute(inverse) after permute(forward): the input, bit for bit
            hip.check(f(bp, C.c_void_p(gp.value), d_perm, n, 1, None))
            b = back.to_host()
            assert np.array_equal(b[off:off + n].view(np.uint8), x.view(np.uint8)), (n, off)
            up.free()
