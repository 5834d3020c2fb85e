"""Directed operands, float64 references and error bounds for the projection proxes of kernels_prox_wrap.hip: ind_halfspace, ind_soc,
elem_operation:ind_simplex, elem_operation:ind_sum and the index-family ind_sum.  Pure numpy and deterministic: the fixture generator
(tests/golden/make_golden.py wrap_edges), the test of the oracle (tests/test_prox_wrap_edges.py) and the test of the GPU kernels
(tests/test_gpu_prox_wrap_edges.py) all draw their cases from here.

A case (class Case) holds the argument vector in the data type T, the positions of every group in it (gidx: count x dim, which makes the
planar layout, the interleaved one and an index family look alike), the operands of the prox in T and a recipe for the prost.function
description.  Every value is rounded to T before the float64 reference sees it, so both work on the same numbers.

Groups: the group of lane t is of the kind KINDS[(t + rotation) % len(KINDS)] with draws of its own, so a case of 67 or 260 groups holds
every kind several times, and the cases of 1 and 3 groups -- whose rotation differs from case to case -- reach every kind between them.
Counts 1, 3, 67, 260: a single lane, less than a wave, a ragged wave, more than one workgroup of 256 lanes.

References: float64, from the definitions of the projections (not from the kernels' expressions); for every finite group the reference
asserts the optimality conditions of its own answer (feasibility, residual in the normal cone, complementarity).

Bounds: forward-error bounds of the straight-line evaluation in T with eps = eps_T (2^-23 / 2^-52), see the docstrings of the
reference functions.  They apply to groups all of whose operands are zero or have a magnitude in [2^-20, 2^20] (Case.in_range).

Index families are DISJOINT here: groups that share an index race on the GPU (one lane per group, all writing res) and run one after the
other in the oracle, so their result is not defined by the operation.
"""
import functools

import numpy as np

DTYPES = (np.float32, np.float64)
COUNTS = (1, 3, 67, 260)
HALFSPACE_DIMS = (1, 2, 3, 4, 7)
SOC_DIMS = (1, 2, 3, 5)
SIMPLEX_DIMS = (1, 2, 3, 4, 5, 10, 11, 23, 24, 57, 58, 132, 133, 300)          # either side of the Shell-sort gaps 4, 10, 23, 57, 132
SUM_DIMS = (1, 2, 7)
LO, HI = 2.0 ** -20, 2.0 ** 20
TAU = 0.875                                                                     # exact in both data types


def projsplx(y):
    """the sort-based projection of y onto the unit simplex (arXiv:1101.6081, the reference's test_prox_sum_ind_simplex.m)"""
    u = np.sort(y)[::-1]
    css = np.cumsum(u)
    rho = np.nonzero(u * np.arange(1, y.size + 1) > (css - 1))[0][-1]
    return np.maximum(y - (css[rho] - 1) / (rho + 1), 0)


class Case:
    """kind: halfspace | soc | simplex | elem_sum | ind_sum.  arg, tau_diag: the whole vectors in T.  gidx (count, dim): positions of the
    groups.  Operands: a (count, dim) and b (count,) broadcast per group next to the coefficient arrays a_coeff / b_coeff as the prox
    takes them (halfspace); s, invert, families [(dim, indices, s)] (ind_sum)."""

    def __init__(self, kind, arg, gidx, **kw):
        self.kind, self.arg, self.gidx = kind, arg, np.asarray(gidx, dtype=np.int64)
        self.count, self.dim = self.gidx.shape
        self.dtype = arg.dtype.type
        self.interleaved = False
        self.invert = False
        self.tau = TAU
        self.tau_diag = np.ones_like(arg)
        self.__dict__.update(kw)

    def groups(self, vec=None):
        return np.asarray(self.arg if vec is None else vec)[self.gidx]

    def untouched(self):
        m = np.ones(self.arg.size, bool)
        m[self.gidx.reshape(-1)] = False
        if hasattr(self, "second"):
            m[self.second.gidx.reshape(-1)] = False
        return m

    def in_range(self):
        """(count,) groups whose operands are all finite and zero or of a magnitude in [LO, HI]"""
        def ok(x):
            x = np.abs(np.asarray(x, dtype=np.float64))
            with np.errstate(invalid="ignore"):
                return np.isfinite(x) & ((x == 0) | ((x >= LO) & (x <= HI)))
        m = ok(self.groups()).all(axis=1)
        if self.kind == "halfspace":
            m &= ok(self.a).all(axis=1) & ok(self.b)
        if self.kind == "ind_sum":
            m &= ok(self.tau_diag[self.gidx]).all(axis=1)
        return m


def prox_function(F, case):
    """the prost.function description of the case (F: the prost_amd.function module)"""
    c = case
    if c.kind == "halfspace":
        return F.sum_ind_halfspace(c.dim, False, c.a_coeff.astype(np.float64), c.b_coeff.astype(np.float64))
    if c.kind == "soc":
        return F.sum_ind_soc(c.dim, False, 1)
    if c.kind == "simplex":
        return F.sum_ind_simplex(c.dim, c.interleaved)
    if c.kind == "elem_sum":
        return F.sum_ind_sum(c.dim, c.interleaved)
    assert c.kind == "ind_sum" and not c.invert
    if len(c.families) == 1:
        return F.sum_ind_sum2(c.families[0][0], c.families[0][1], c.families[0][2])
    (d1, i1, s1), (d2, i2, s2) = c.families
    return F.sum_ind_sum2(d1, i1, s1, d2, i2, s2)


# ---- helpers ---------------------------------------------------------------------------------------------------------------------
def _draw(rng, dtype, n, scale=1.0):
    """n values of either sign with magnitudes in [scale / 4, 2 scale], rounded to T"""
    return (rng.choice([-1.0, 1.0], n) * rng.uniform(0.25, 2.0, n) * scale).astype(dtype)


def _dyadic(rng, dtype, n, step, top):
    """n non-zero multiples of `step` (a power of two) of either sign up to `top`: sums and products of a few of them are exact in T"""
    k = rng.integers(1, int(top / step) + 1, n) * rng.choice([-1, 1], n)
    return (k * step).astype(dtype)


def _big(dtype):
    """-> (a value whose square overflows in T, one whose square underflows to zero)"""
    return (dtype(2.0 ** 64), dtype(2.0 ** -80)) if dtype == np.float32 else (dtype(2.0 ** 600), dtype(2.0 ** -600))


def _seq_dot(a, v):
    """the inner product summed in T in index order, every product and every sum rounded: where the operands sit ON the branch"""
    s = a.dtype.type(0)
    with np.errstate(all="ignore"):
        for x, y in zip(a, v):
            s = s + x * y
    return s


def _planar(count, dim, offset=0):
    return offset + np.arange(count)[:, None] + count * np.arange(dim)[None, :]


def _layout(count, dim, interleaved):
    return np.arange(count * dim).reshape(count, dim) if interleaved else _planar(count, dim)


def _rng(*key):
    return np.random.default_rng([int(k) for k in key])


def _scatter(dtype, groups, gidx, n=None, fill=None):
    arg = np.zeros(gidx.size if n is None else n, dtype) if fill is None else fill.copy()
    arg[gidx.reshape(-1)] = np.asarray(groups, dtype=dtype).reshape(-1)
    return arg


def _tau_diag(rng, dtype, n):
    return rng.uniform(0.25, 1.5, n).astype(dtype)


# ---- halfspace -------------------------------------------------------------------------------------------------------------------
HALFSPACE_KINDS = ("on", "below", "above", "feasible", "infeasible", "single", "zero_normal", "nan", "clean", "inf", "huge_v", "tiny_a", "huge_a",
                   "small", "big")
HALFSPACE_NORMALS = ("group", "shared", "shared_single", "shared_zero", "shared_huge", "shared_tiny")
HALFSPACE_BS = ("group", "pos", "neg")            # b per group, or one scalar 0.75 / -0.75


def halfspace_case(dtype, dim, count, normal, bmode, rot):
    """v (count x dim), a per group (normal == "group") or one shared normal, b per group (bmode == "group") or the scalar +-0.75.
    With a scalar b the groups that sit on the boundary have dyadic a and v with the last entry solved for <a, v> = b, every partial sum
    exact; with b per group, b = fl_T(<a, v>) summed in index order, and its two neighbours."""
    dtype = np.dtype(dtype).type
    rng = _rng(1, dim, count, HALFSPACE_NORMALS.index(normal), HALFSPACE_BS.index(bmode), np.dtype(dtype).itemsize)
    huge, tiny = _big(dtype)
    b0 = dtype({"pos": 0.75, "neg": -0.75}.get(bmode, 0.0))

    def dyadic_normal():
        a = _dyadic(rng, dtype, dim, 0.25, 2.0)
        a[-1] = rng.choice([-2.0, -1.0, -0.5, 0.5, 1.0, 2.0])
        return a
    shared = None
    if normal != "group":
        shared = dyadic_normal() if bmode != "group" else _draw(rng, dtype, dim)
        if normal == "shared_single":
            keep = shared[-1]; shared[:] = 0; shared[-1] = keep
        if normal == "shared_zero":
            shared[:] = 0
        if normal == "shared_huge":
            shared = (shared * huge).astype(dtype)
        if normal == "shared_tiny":
            shared = (shared * tiny).astype(dtype)
    V, A, B = np.zeros((count, dim), dtype), np.zeros((count, dim), dtype), np.zeros(count, dtype)
    with np.errstate(all="ignore"):
        for t in range(count):
            kind = HALFSPACE_KINDS[(t + rot) % len(HALFSPACE_KINDS)]
            scale = {"small": 2.0 ** -10, "big": 2.0 ** 10}.get(kind, 1.0)
            exact = bmode != "group" and kind in ("on", "below", "above", "single")
            if shared is not None:
                a = shared.copy()
            else:
                a = dyadic_normal() if exact else _draw(rng, dtype, dim, scale)
                if kind == "single":
                    keep = a[-1]; a[:] = 0; a[-1] = keep
                if kind == "zero_normal":
                    a[:] = 0
                if kind == "tiny_a":
                    a = (a * tiny).astype(dtype)
                if kind == "huge_a":
                    a = (a * huge).astype(dtype)
            v = _dyadic(rng, dtype, dim, 0.125, 2.0) if exact else _draw(rng, dtype, dim, scale)
            if exact and a[-1] != 0 and np.isfinite(a).all() and abs(a[-1]) in (0.5, 1.0, 2.0):
                v[-1] = (b0 - _seq_dot(a[:-1], v[:-1])) / a[-1]           # exact: every term a multiple of 2^-5 below 2^5
                assert _seq_dot(a, v) == b0
                if kind == "below":
                    v[-1] = np.nextafter(v[-1], dtype(np.inf) * np.sign(a[-1]))       # <a, v> just above b: b lies below it
                if kind == "above":
                    v[-1] = np.nextafter(v[-1], dtype(-np.inf) * np.sign(a[-1]))
            j = int(rng.integers(dim))
            if kind == "nan":
                v[j] = np.nan
            if kind == "inf":
                v[j] = rng.choice([-np.inf, np.inf])
            if kind == "huge_v":
                v = (np.sign(v) * np.finfo(dtype).max / 2).astype(dtype)
            d = _seq_dot(a, v)
            if bmode == "group":
                b = {"on": d, "single": d, "below": np.nextafter(d, dtype(-np.inf)), "above": np.nextafter(d, dtype(np.inf)), "feasible": d + dtype(scale),
                     "zero_normal": dtype(0.5 if (t // len(HALFSPACE_KINDS)) % 2 == 0 else -0.5)}.get(kind, d - dtype(scale) / 2)
                if not np.isfinite(b):
                    b = dtype(0.5)
            else:
                b = b0
            V[t], A[t], B[t] = v, a, b
    gidx = _planar(count, dim)
    a_coeff = shared if shared is not None else A.T.reshape(-1).copy()
    b_coeff = B.copy() if bmode == "group" else np.array([b0], dtype)
    return Case("halfspace", _scatter(dtype, V, gidx), gidx, a=A, b=B, a_coeff=np.asarray(a_coeff, dtype), b_coeff=b_coeff, tau_diag=_tau_diag(rng, dtype, count * dim))


def halfspace_reference(case):
    """-> (r, bound, checked): r = v - max(0, <a, v> - b) / |a|^2 a in float64.

    Bound on the straight-line evaluation in T, eps = eps_T, per entry i:
        (dim + 4) eps (sum_j |a_j v_j| + |b|) |a_i| / |a|^2 + eps |r_i|.
    With the unit roundoff u = eps / 2 and to first order: the inner product of dim rounded products, summed in order, carries at most
    dim u sum|a_j v_j|, the subtraction of b another u (sum|a_j v_j| + |b|); max(0, .) is 1-Lipschitz, so the excess e carries
    (dim + 1) u (sum|a_j v_j| + |b|).  |a|^2, a sum of positive terms, has the relative error dim u at most, the division and the product
    with a_i add u each; as e <= sum|a_j v_j| + |b| that is (dim + 2) u more of the same quantity.  Times |a_i| / |a|^2 the correction
    carries (2 dim + 3) u = (dim + 3/2) eps <= (dim + 4) eps of it.  The last subtraction rounds the result once: u |r_i| <= eps |r_i|."""
    v, a, b = (np.asarray(x, dtype=np.float64) for x in (case.groups(), case.a, case.b))
    eps = float(np.finfo(case.dtype).eps)
    with np.errstate(all="ignore"):
        sq = (a * a).sum(axis=1)
        excess = np.maximum(0.0, (a * v).sum(axis=1) - b)
        r = v - (excess / sq)[:, None] * a
        bound = (case.dim + 4) * eps * ((np.abs(a * v).sum(axis=1) + np.abs(b)) / sq)[:, None] * np.abs(a) + eps * np.abs(r)
        checked = case.in_range() & np.isfinite(r).all(axis=1) & (sq > 0)
        # optimality of the answer in float64: feasible, v - r = lambda a with lambda >= 0, lambda (<a, r> - b) = 0
        tol = 64 * (case.dim + 4) * 2.0 ** -52
        size = np.abs(a * v).sum(axis=1) + np.abs(b)
        slack = (a * r).sum(axis=1) - b
        lam = excess / sq
        for t in np.flatnonzero(checked):
            assert slack[t] <= tol * size[t], ("halfspace reference: infeasible", t)
            assert lam[t] >= 0 and abs(lam[t] * slack[t]) <= tol * size[t] * max(lam[t], 1.0), ("halfspace reference: complementarity", t)
            assert np.abs((v[t] - r[t]) - lam[t] * a[t]).max() <= tol * (np.abs(v[t]).max() + lam[t] * np.abs(a[t]).max()), ("halfspace reference: residual", t)
    return r, bound, checked


# ---- second-order cone -----------------------------------------------------------------------------------------------------------
SOC_KINDS = ("on_pos", "on_pos_below", "on_pos_above", "on_neg", "on_neg_below", "on_neg_above", "zero_pos", "zero_zero", "zero_neg", "pyth_pos",
             "pyth_neg", "nan_x", "clean", "nan_y", "overflow_x", "inf_y_pos", "inf_y_neg", "overflow_on", "overflow_polar", "inside", "polar", "between", "small", "big")


def soc_case(dtype, dim, count, rot):
    """(x_1 .. x_{dim-1}, y) per group, planar.  y = +-fl_T(||x||) with the norm as T forms it (squares summed in index order, one square
    root) and its neighbours; x = 0; (3k, 4k, 0 ..) with the exact norm 5k; NaN, overflow, infinities.  With finite operands the third
    regime gives the bits of the first at ||x|| == y (its factor is exactly 1) and zeros at ||x|| == -y (its factor is exactly 0), so a
    comparison that is strict by mistake shows only where the squared norm overflows and y = +-inf: inf <= inf keeps the point (or
    gives zero), the third regime forms inf - inf."""
    dtype = np.dtype(dtype).type
    rng = _rng(2, dim, count, np.dtype(dtype).itemsize)
    huge, _ = _big(dtype)
    G = np.zeros((count, dim), dtype)
    inf = dtype(np.inf)
    with np.errstate(all="ignore"):
        for t in range(count):
            kind = SOC_KINDS[(t + rot) % len(SOC_KINDS)]
            scale = {"small": 2.0 ** -10, "big": 2.0 ** 10}.get(kind, 1.0)
            x = _draw(rng, dtype, dim - 1, scale)
            if kind.startswith("zero"):
                x[:] = 0
            if kind.startswith("pyth"):
                k = dtype(rng.choice([0.25, 0.5, 1.0, 3.0]))
                x[:] = 0
                x[:2] = (3 * k, 4 * k)[:dim - 1] if dim >= 3 else (5 * k,)[:dim - 1]
            if kind == "nan_x" and dim > 1:
                x[int(rng.integers(dim - 1))] = np.nan
            if kind.startswith("overflow") and dim > 1:
                x[0] = huge
            n = np.sqrt(_seq_dot(x, x)) if dim > 1 else dtype(0)
            y = {"on_pos": n, "on_pos_below": np.nextafter(n, -inf), "on_pos_above": np.nextafter(n, inf), "on_neg": -n, "on_neg_below": np.nextafter(-n, -inf),
                 "on_neg_above": np.nextafter(-n, inf), "zero_pos": dtype(0.5), "zero_zero": dtype(0), "zero_neg": dtype(-0.5), "pyth_pos": n, "pyth_neg": -n,
                 "nan_y": dtype(np.nan), "inf_y_pos": inf, "inf_y_neg": -inf, "overflow_on": inf, "overflow_polar": -inf, "inside": 2 * n + dtype(scale), "polar": -2 * n - dtype(scale),
                 "overflow_x": dtype(1.5), "nan_x": dtype(0.5)}.get(kind, dtype(rng.uniform(-0.9, 0.9)) * n)
            if kind.startswith("pyth") and dim >= 3:
                assert n == 5 * k
            G[t, :dim - 1], G[t, dim - 1] = x, y
    gidx = _planar(count, dim)
    return Case("soc", _scatter(dtype, G, gidx), gidx, tau_diag=_tau_diag(rng, dtype, count * dim))


def soc_reference(case):
    """-> (r, bound, checked): the projection onto {||x|| <= y}: the point itself inside the cone, 0 inside the polar cone -{||x|| <= y},
    else ((y + n) / (2 n)) (x, n) with n = ||x||.

    Bound, every entry: (dim + 6) eps m with m = max(|y|, ||x||).  With u = eps / 2 and to first order: the sum of dim - 1 rounded
    squares has the relative error (dim - 1) u at most, the root halves it and rounds once: dn <= ((dim + 1) / 2) u n.  In the third
    regime the factor f = (y + n) / (2 n) lies in (0, 1); its numerator carries dn + u |y + n|, the division by the exact 2 n and the
    product with x_i or n round once each and n in the denominator adds f dn / n, so every entry (at most n in magnitude) carries
    dn / 2 + u m + dn + 2 u m <= (3 (dim + 1) / 8 + 3/2) eps m.  The projection is continuous and 1-Lipschitz across the two borders, so a
    comparison that the rounded norm decides the other way moves the result by no more than 2 dn <= ((dim + 1) / 2) eps m on top of
    that: (7 dim / 8 + 19 / 8) eps m <= (dim + 6) eps m in all."""
    g = np.asarray(case.groups(), dtype=np.float64)
    eps = float(np.finfo(case.dtype).eps)
    x, y = g[:, :-1], g[:, -1]
    with np.errstate(all="ignore"):
        n = np.sqrt((x * x).sum(axis=1))
        fac = np.where(n <= y, 1.0, np.where(n <= -y, 0.0, (y + n) / (2 * n)))
        r = np.concatenate([fac[:, None] * x, np.where(n <= y, y, fac * n)[:, None]], axis=1)
        r[(n <= -y) & ~(n <= y)] = 0.0
        size = np.maximum(np.abs(y), n)
        bound = np.repeat(((case.dim + 6) * eps * size)[:, None], case.dim, axis=1)
        checked = case.in_range() & np.isfinite(r).all(axis=1)
        tol = 64 * (case.dim + 6) * 2.0 ** -52
        for t in np.flatnonzero(checked):
            rx, ry = r[t, :-1], r[t, -1]
            w = g[t] - r[t]                                                  # the residual lies in the polar cone and is orthogonal to r
            assert np.sqrt((rx * rx).sum()) <= ry + tol * size[t], ("cone reference: infeasible", t)
            assert np.sqrt((w[:-1] * w[:-1]).sum()) <= -w[-1] + tol * size[t], ("cone reference: residual", t)
            assert abs((w * r[t]).sum()) <= tol * size[t] * size[t], ("cone reference: complementarity", t)
    return r, bound, checked


# ---- simplex ---------------------------------------------------------------------------------------------------------------------
SIMPLEX_KINDS = ("equal", "ties", "ascending", "nan_first", "descending", "nan_middle", "on_simplex", "nan_last", "vertex", "inf", "negative", "positive",
                 "threshold_tie", "random", "small", "big")


def _threshold_tie(dtype, dim, rng):
    """three leading entries a0 >= a1 >= a2 in T (the rest far below) for which the threshold after two entries, fl_T((fl_T(a0 + a1) - 1) / 2)
    with the division in double as the functor does it, EQUALS a2 -- the search stops there with `>=` -- while one more step,
    fl_T((fl_T(fl_T(a0 + a1) + a2) - 1) / 3), rounds to a neighbour of it: a search that went on (`>`) returns other bits.  Found by trying
    draws; None for dim < 3 (with two entries both steps are exact)."""
    if dim < 3:
        return None
    for _ in range(4000):
        a0, a1 = (dtype(v) for v in rng.uniform(1.0, 2.0, 2))
        a0, a1 = max(a0, a1), min(a0, a1)
        s = a0 + a1
        t = dtype((np.float64(s) - 1.0) / np.float64(dtype(2)))
        more = dtype((np.float64(s + t) - 1.0) / np.float64(dtype(3)))
        if dtype(np.float64(a0) - 1.0) < a1 and t <= a1 and more != t:
            x = (-1.0 - rng.uniform(0, 1, dim)).astype(dtype)
            x[:3] = (a0, a1, t)
            return rng.permutation(x)
    raise AssertionError("no threshold tie found")


def _simplex_group(kind, dtype, dim, rng):
    x = _draw(rng, dtype, dim)
    if kind == "threshold_tie":
        tie = _threshold_tie(dtype, dim, rng)
        x = x if tie is None else tie
    if kind == "equal":
        x[:] = dtype(rng.choice([-1.5, 0.25, 0.75, 3.0]))
    if kind == "ties":
        x = (rng.integers(-8, 9, dim) / 4.0).astype(dtype)
    if kind == "ascending":
        x = np.sort(x)
    if kind == "descending":
        x = np.sort(x)[::-1].copy()
    if kind == "on_simplex":                                                      # integers that sum to 2^12, over 2^12: the sum is exactly 1
        k = np.full(dim, 4096 // dim); k[:4096 - k.sum()] += 1
        x = (rng.permutation(k) / 4096.0).astype(dtype)
        assert x.astype(np.float64).sum() == 1.0
    if kind == "vertex":
        x = (x / 2).astype(dtype); x[int(rng.integers(dim))] = dtype(5.0)          # 5 - 1 >= every other entry: the result is a unit vector
    if kind == "negative":
        x = (-np.abs(x) * 2.0 ** 17).astype(dtype)
    if kind == "positive":                                                        # spread below 1 / dim: every entry of the projection is positive
        x = (2.0 + rng.uniform(0, 0.5 / dim, dim)).astype(dtype)
    if kind == "small":
        x = (x * 2.0 ** -10).astype(dtype)
    if kind == "big":
        x = (x * 2.0 ** 10).astype(dtype)
    if kind == "inf":
        x[int(rng.integers(dim))] = np.inf
    if kind.startswith("nan"):                                                    # the neighbouring lanes are clean kinds
        x[{"nan_first": 0, "nan_middle": dim // 2, "nan_last": dim - 1}[kind]] = np.nan
    return x


def simplex_case(dtype, dim, count, interleaved, rot):
    dtype = np.dtype(dtype).type
    rng = _rng(3, dim, count, int(interleaved), np.dtype(dtype).itemsize)
    G = np.array([_simplex_group(SIMPLEX_KINDS[(t + rot) % len(SIMPLEX_KINDS)], dtype, dim, rng) for t in range(count)], dtype=dtype)
    gidx = _layout(count, dim, interleaved)
    return Case("simplex", _scatter(dtype, G, gidx), gidx, interleaved=bool(interleaved), tau_diag=_tau_diag(rng, dtype, count * dim))


def simplex_reference(case):
    """-> (r, bound, checked): the sort-based projection onto the unit simplex in float64.

    Bound, every entry: (2 dim + 8) eps M with M = max(1, max|x|).  With u = eps / 2 and to first order: the threshold is
    t = (sum of the k largest entries - 1) / k.  The sum of k <= dim terms carries (k - 1) u k max|x| at most, after the division by k
    (dim / 2) eps M; the -1 and the division are done in double and rounded to T once, u |t| <= eps M as |t| <= max|x| + 1; the
    subtraction x_i - t rounds once more, u (2 max|x| + 1) <= eps M ... (dim / 2 + 2) eps M for the k of exact arithmetic.  The rounded
    comparison t_k >= x_(k+1) may settle on another k only when the two sides differ by no more than their errors, and then the
    thresholds of the two k differ by no more than that as well: at most the same amount again, (dim + 4) eps M.  The issue that set
    this bound doubles it to cover k that are off by more than one in a run of near-ties."""
    g = np.asarray(case.groups(), dtype=np.float64)
    eps = float(np.finfo(case.dtype).eps)
    checked = case.in_range()
    r = np.full(g.shape, np.nan)
    bound = np.zeros(g.shape)
    tol = 64 * (case.dim + 4) * 2.0 ** -52
    for t in np.flatnonzero(checked):
        x = g[t]
        r[t] = projsplx(x)
        size = max(1.0, np.abs(x).max())
        bound[t] = (2 * case.dim + 8) * eps * size
        # optimality: r >= 0, sum r = 1, x - r = theta on the support and <= theta off it
        assert r[t].min() >= 0 and abs(r[t].sum() - 1) <= tol * size, ("simplex reference: infeasible", t)
        w = x - r[t]
        theta = w[r[t] > 0].max()
        assert np.abs(w[r[t] > 0] - theta).max() <= tol * size and (w[r[t] == 0] <= theta + tol * size).all(), ("simplex reference: residual", t)
    return r, bound, checked


# ---- sums ------------------------------------------------------------------------------------------------------------------------
SUM_KINDS = ("exact", "cancel", "nan", "random", "small", "big")


def _sum_group(kind, dtype, dim, rng, s):
    x = _draw(rng, dtype, dim)
    if kind == "exact":                                                           # dyadic entries whose sum is exactly s
        x = _dyadic(rng, dtype, dim, 0.125, 2.0)
        x[-1] = dtype(s) - x[:-1].astype(np.float64).sum()
    if kind == "cancel":                                                          # (x, -x, ..., small)
        big = _draw(rng, dtype, dim // 2, 2.0 ** 10)
        x[:2 * (dim // 2):2], x[1:2 * (dim // 2):2] = big, -big
        x[2 * (dim // 2):] = _draw(rng, dtype, dim - 2 * (dim // 2), 2.0 ** -10)
    if kind == "nan":
        x[int(rng.integers(dim))] = np.nan
    if kind == "small":
        x = (x * 2.0 ** -10).astype(dtype)
    if kind == "big":
        x = (x * 2.0 ** 10).astype(dtype)
    return x


def elem_sum_case(dtype, dim, count, interleaved, rot):
    dtype = np.dtype(dtype).type
    rng = _rng(4, dim, count, int(interleaved), np.dtype(dtype).itemsize)
    G = np.array([_sum_group(SUM_KINDS[(t + rot) % len(SUM_KINDS)], dtype, dim, rng, 1.0) for t in range(count)], dtype=dtype)
    gidx = _layout(count, dim, interleaved)
    return Case("elem_sum", _scatter(dtype, G, gidx), gidx, interleaved=bool(interleaved), s=1.0, tau_diag=_tau_diag(rng, dtype, count * dim))


def ind_sum_case(dtype, dim, count, permuted, s, invert, two, rot):
    """disjoint index families over a vector with three trailing entries that no group touches.  two: a second family of count groups of
    2 dim entries behind the first, with the target sum s / 2."""
    dtype = np.dtype(dtype).type
    rng = _rng(5, dim, count, int(permuted), int(4 * s) + 8, int(invert), int(two), np.dtype(dtype).itemsize)
    n1 = count * dim
    n2 = count * 2 * dim if two else 0
    n = n1 + n2 + 3
    idx1 = (rng.permutation(n1) if permuted else np.arange(n1)).reshape(count, dim)
    G1 = np.array([_sum_group(SUM_KINDS[(t + rot) % len(SUM_KINDS)], dtype, dim, rng, s) for t in range(count)], dtype=dtype)
    arg = _scatter(dtype, G1, idx1, n, fill=_draw(rng, dtype, n))
    families = [(dim, idx1.reshape(-1).copy(), float(s))]
    gidx, S = idx1, np.full(count, float(s))
    if two:
        idx2 = n1 + (rng.permutation(n2) if permuted else np.arange(n2)).reshape(count, 2 * dim)
        G2 = np.array([_sum_group(SUM_KINDS[(t + rot + 1) % len(SUM_KINDS)], dtype, 2 * dim, rng, s / 2) for t in range(count)], dtype=dtype)
        arg[idx2.reshape(-1)] = G2.reshape(-1)
        families.append((2 * dim, idx2.reshape(-1).copy(), float(s) / 2))
    case = Case("ind_sum", arg, gidx, s=S, invert=bool(invert), families=families, tau_diag=_tau_diag(rng, dtype, n))
    if two:
        case.second = Case("ind_sum", arg, idx2, s=np.full(count, float(s) / 2), invert=bool(invert), families=families[1:], tau_diag=case.tau_diag)
    return case


def sum_reference(case):
    """-> (r, bound, checked): x_k - t_k (sum x - s) / sum t over the group in float64, with t = 1 (elem_operation:ind_sum, s = 1) or
    t = tau tau_diag, or its reciprocal with invert (index families).

    Bound per entry k: (dim + 4) eps (sum|x| + |s|) t_k / sum t + eps |r_k|.  With u = eps / 2 and to first order: the sum of dim entries
    carries (dim - 1) u sum|x|, the subtraction of s another u (sum|x| + |s|): dim u (sum|x| + |s|).  The weights t_k are rounded once or
    (reciprocal) twice and their sum, of positive terms, dim - 1 times more: (dim + 3) u relative in t_k / sum t; the product and the
    division round once each.  Together (2 dim + 5) u = (dim + 5/2) eps of (sum|x| + |s|) t_k / sum t; the last subtraction rounds the
    result once: u |r_k| <= eps |r_k|."""
    x = np.asarray(case.groups(), dtype=np.float64)
    eps = float(np.finfo(case.dtype).eps)
    if case.kind == "elem_sum":
        t = np.ones_like(x)
        s = np.ones(case.count)
    else:
        t = float(case.dtype(case.tau)) * np.asarray(case.tau_diag, dtype=np.float64)[case.gidx]
        t = 1.0 / t if case.invert else t
        s = np.asarray(case.s, dtype=np.float64)
    with np.errstate(all="ignore"):
        viol = x.sum(axis=1) - s
        share = t / t.sum(axis=1, keepdims=True)
        r = x - share * viol[:, None]
        size = np.abs(x).sum(axis=1) + np.abs(s)
        bound = (case.dim + 4) * eps * size[:, None] * share + eps * np.abs(r)
        checked = case.in_range() & np.isfinite(r).all(axis=1)
        tol = 64 * (case.dim + 4) * 2.0 ** -52
        for g in np.flatnonzero(checked):
            assert abs(r[g].sum() - s[g]) <= tol * size[g], ("sum reference: infeasible", g)
            w = (x[g] - r[g]) / t[g]                                         # the residual is a multiple of t: the prox in the metric diag(1 / t)
            assert np.abs(w - w[0]).max() <= tol * size[g] / t[g].min(), ("sum reference: residual", g)
    return r, bound, checked


REFERENCES = {"halfspace": halfspace_reference, "soc": soc_reference, "simplex": simplex_reference, "elem_sum": sum_reference, "ind_sum": sum_reference}


def reference(case):
    """-> (reference (count, dim) in float64, bound (count, dim), checked (count,): the finite in-range groups); computed once per case"""
    if not hasattr(case, "_reference"):
        case._reference = REFERENCES[case.kind](case)
    return case._reference


def ratio_to_bound(case, got):
    """-> the worst |got - reference| / bound over the finite in-range groups of the case (0 when there is none); asserts that every
    such group is finite in `got` (the whole result vector)"""
    worst = 0.0
    for c in [case] + ([case.second] if hasattr(case, "second") else []):
        r, bound, checked = reference(c)
        g = np.asarray(c.groups(got), dtype=np.float64)[checked]
        assert np.isfinite(g).all(), "a finite in-range group has a non-finite answer"
        err = np.abs(g - r[checked])
        with np.errstate(invalid="ignore", divide="ignore"):
            q = np.where(err == 0, 0.0, err / bound[checked])
        if q.size:
            worst = max(worst, float(q.max()))
    return worst


# ---- the cases -------------------------------------------------------------------------------------------------------------------
def cases(dtype, kinds=("halfspace", "soc", "simplex", "elem_sum", "ind_sum")):
    """yields (name, Case).  The rotation of the group kinds advances from case to case and starts anew with every kind of prox, so a case
    is the same whichever kinds are drawn with it."""
    tname = np.dtype(dtype).name
    k = 0
    if "halfspace" in kinds:
        for dim in HALFSPACE_DIMS:
            for count in COUNTS:
                for normal in HALFSPACE_NORMALS:
                    for bmode in HALFSPACE_BS:
                        k += 1
                        yield "%s_halfspace_dim%d_n%d_%s_b%s" % (tname, dim, count, normal, bmode), halfspace_case(dtype, dim, count, normal, bmode, k)
    if "soc" in kinds:
        k = 0
        for dim in SOC_DIMS:
            for count in COUNTS:
                for rep in range(3 if count < 67 else 1):                      # the small counts see more of the kinds
                    k += 5
                    yield "%s_soc_dim%d_n%d_r%d" % (tname, dim, count, rep), soc_case(dtype, dim, count, k)
    if "simplex" in kinds:
        k = 0
        for dim in SIMPLEX_DIMS:
            for count in COUNTS:
                for il in (False, True):
                    k += 1
                    yield "%s_simplex_dim%d_n%d_il%d" % (tname, dim, count, il), simplex_case(dtype, dim, count, il, k)
    if "elem_sum" in kinds:
        k = 0
        for dim in SUM_DIMS:
            for count in COUNTS:
                for il in (False, True):
                    k += 1
                    yield "%s_elemsum_dim%d_n%d_il%d" % (tname, dim, count, il), elem_sum_case(dtype, dim, count, il, k)
    if "ind_sum" in kinds:
        k = 0
        for dim in SUM_DIMS:
            for count in COUNTS:
                for permuted in (False, True):
                    for s in (0.0, 2.0, -1.0):
                        for invert in (False, True):
                            k += 1
                            yield ("%s_indsum_dim%d_n%d_perm%d_s%g_inv%d" % (tname, dim, count, permuted, s, invert),
                                   ind_sum_case(dtype, dim, count, permuted, s, invert, False, k))
                k += 1
                yield "%s_indsum2_dim%d_n%d" % (tname, dim, count), ind_sum_case(dtype, dim, count, True, 2.0, False, True, k)


@functools.lru_cache(maxsize=None)
def case_list(dtype, kind):
    """the cases of one kind, made once per process and shared by the tests that need them (with their references)"""
    return tuple(cases(dtype, kinds=(kind,)))


def fixture_cases(dtype):
    """the cases whose answers the reference's own functors give (ElemOperationIndSimplex, ElemOperationIndSum)"""
    return cases(dtype, kinds=("simplex", "elem_sum"))
