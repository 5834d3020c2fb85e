"""GPU parity at the branch edges and the special values of the elementwise proxes.

Operands come from tests/elem_edge_cases.py: values ON the thresholds of the 14 Function1D maps and one ulp either side, signed zeros,
subnormals, squares that underflow or overflow, the largest finite numbers, infinities and NaN; norm2 groups whose norm is exactly such
a value, whose squared norm overflows, is NaN or is zero.  tests/test_elementwise_edges.py pins the CPU oracle on them to the reference's
own functors; here every kernel instance is compared with the oracle.

Bar for every comparison: np.array_equal(got, want, equal_nan=True).  The one exception is `lq` (Newton on pow(): close_lq, the
tolerance of the whole suite).  The sign of a zero is not compared (device_math.hpp: norm2_leq0_fast documents that zeros of tiny norms
may differ in sign; test_double_iteration_kernel_special_values holds the kernels to each other there).

 1. prost_hip_prox_elem / _moreau / _arg (modes 1, 2) in every instance launch_prox_elem can choose
 2. one launch of every fused PDHG family against the oracle's iterations, with a NaN, a zero, an overflowing and an ordinary norm in
    the four rows of ONE lane
 3. the solver on ROF images with a NaN and an infinite pixel
"""
import ctypes as C

import numpy as np
import pytest

import elem_edge_cases as E
import oracle
import prost_amd as prost
from pdhg_iteration_reference import F_COEFFS, SVAL, oracle_iteration
from prost_amd import synthetic
from test_oracle_pinning import close_lq

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]


def same(got, want, fn, dtype):
    return close_lq(got, want, dtype) if fn == "lq" else np.array_equal(got, want, equal_nan=True)


# ---- 1. the generic prox kernels ------------------------------------------------------------------------------------------------
# (op, dim, interleaved, count, pointer offset in elements): the smallest shapes that reach every instance of launch_prox_elem
# (kernels_prox.hip).  VEC = 4 (fp32) / 2 (fp64); 65 and 161 are multiples of neither; 160 and 260 hold every operand / group.
SCALAR_1D = [(0, 1, False, 1, 0), (0, 1, False, 3, 0), (0, 1, False, 65, 0), (0, 1, False, 64, 1)]      # counts 1, 3, 65; 64 with all pointers one element off 16 bytes
SCALAR_INTERLEAVED = [(1, 2, True, 160, 0), (1, 5, True, 160, 0)]
SCALAR_RAGGED = [(1, 2, False, 161, 0), (1, 7, False, 161, 0)]
VECTOR_1D = [(0, 1, False, 4, 0), (0, 1, False, 260, 0)]
VECTOR_NORM2 = [(1, dim, False, count, 0) for dim in (1, 2, 3, 4, 5, 7) for count in (4, 260)]           # DIM 1-4 in registers, 5 and 7 in two passes
SHAPES = SCALAR_1D + SCALAR_INTERLEAVED + SCALAR_RAGGED + VECTOR_1D + VECTOR_NORM2
ARG_SOURCE_SHAPES = [(0, 1, False, 65, 0), (0, 1, False, 260, 0), (1, 2, False, 260, 0), (1, 4, False, 260, 0), (1, 7, False, 260, 0), (1, 5, True, 160, 0), (1, 2, False, 161, 0)]
assert set(ARG_SOURCE_SHAPES) <= set(SHAPES)


def moreau_case(args):
    """the Moreau wrap (prox_moreau.cu:98-134) whose inner operation sees the operands of `args`: -> (outer argument, outer invert_tau,
    expected result).  Prescale :29-43, the elem operation with the inverted step flag, postscale :45-61, each operation rounded to the
    data type.  (In the exact family tau * tau_diag = 1/2, so the prescaled argument is the edge operand itself unless it overflows.)"""
    op, fn, v, td, tau, count, dim, il, coeffs, inv = args
    T = v.dtype.type
    with np.errstate(all="ignore"):
        s = T(tau) * td
        outer_inv = not inv
        a = (v / s if outer_inv else v * s).astype(v.dtype)
        pre = (a * s if outer_inv else a / s).astype(v.dtype)
        r = oracle.prox_elem(op, fn, pre, td, tau, count, dim, il, coeffs, inv)
        want = (a - r / s if outer_inv else a - s * r).astype(v.dtype)
    return a, outer_inv, want


class Upload:
    """device copies of host arrays, `off` elements behind a 16-byte boundary; freed together"""

    def __init__(self, hip, off):
        self.hip, self.off, self.bufs = hip, off, []

    def __call__(self, a):
        a = np.ascontiguousarray(a)
        d = self.hip.DeviceArray.from_host(np.concatenate([np.zeros(self.off, a.dtype), a]))
        self.bufs.append(d)
        return C.c_void_p(d.ptr.value + self.off * a.dtype.itemsize)

    def result(self, n, dtype):
        d = self.hip.DeviceArray.from_host(np.full(n + self.off, 7.0, dtype))
        self.bufs.append(d)
        return d, C.c_void_p(d.ptr.value + self.off * np.dtype(dtype).itemsize)

    def free(self):
        for d in self.bufs:
            d.free()


def coeff_args(up, coeffs, dtype):
    ptrs, vals = (C.c_void_p * 7)(), (C.c_double * 7)()
    for i, c in enumerate(coeffs):
        c = np.atleast_1d(np.asarray(c, dtype=np.float64)).ravel()
        if c.size > 1:
            ptrs[i] = up(c.astype(dtype)).value
        else:
            ptrs[i] = None; vals[i] = float(c[0])
    return ptrs, vals


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("fn", E.FUNCTIONS)
def test_prox_elem_kernels_on_directed_operands(hip, dtype, fn):
    """prost_hip_prox_elem, _moreau and _arg (the PDHG argument modes with a zero product operand: the argument is the edge value
    itself) against the oracle: every kernel instance, the four coefficient families, invert_tau off and on"""
    launches = 0
    shapes = [s[:4] for s in SHAPES]
    offs = {s[:4]: s[4] for s in SHAPES}
    for name, args in E.cases(dtype, shapes=shapes, functions=(fn,)):
        op, _, arg, td, tau, count, dim, il, coeffs, inv = args
        n = count * dim
        up = Upload(hip, offs[(op, dim, il, count)])
        ptrs, vals = coeff_args(up, coeffs, dtype)
        d_td = up(td)
        zeros, ones = up(np.zeros(n, dtype)), up(np.ones(n, dtype))
        with_sources = (op, dim, il, count, 0) in ARG_SOURCE_SHAPES and ("_exact" in name or "_general" in name)
        m_arg, m_inv, m_want = moreau_case(args)
        for moreau, a, a_inv, want in ((0, arg, inv, oracle.prox_elem(*args)), (1, m_arg, m_inv, m_want)):
            d_a = up(a)
            res, rp = up.result(n, dtype)
            plain = hip.fn("prox_elem_moreau" if moreau else "prox_elem", dtype)
            hip.check(plain(op, hip.FN_ID[fn], rp, d_a, d_td, hip.dbl(tau), int(a_inv), hip.sz(count), hip.sz(dim), int(il), ptrs, vals, None))
            got = res.to_host()[up.off:]
            assert same(got, want, fn, dtype), (name, "moreau" if moreau else "plain", np.flatnonzero(~((got == want) | (np.isnan(got) & np.isnan(want))))[:8])
            launches += 1
            for mode in ((1, 2) if with_sources else ()):
                spec = hip.ArgSpec(); spec.mode = mode
                # mode 1: v0 - s0 v1 v2 with v2 = 0; mode 2: v0 + s0 v1 ((1 + s1) v2 - s1 v3) with v2 = v3 = 0
                for k, p in enumerate((d_a, ones, zeros, zeros)):
                    spec.v[k] = p.value
                spec.s[0], spec.s[1] = 0.37, 0.8
                res, rp = up.result(n, dtype)
                hip.check(hip.fn("prox_elem_arg", dtype)(op, hip.FN_ID[fn], moreau, rp, C.byref(spec), d_td, hip.dbl(tau), int(a_inv), hip.sz(count), hip.sz(dim), int(il),
                                                         ptrs, vals, None))
                got = res.to_host()[up.off:]
                assert same(got, want, fn, dtype), (name, "moreau" if moreau else "plain", "argument mode %d" % mode)
                launches += 1
        up.free()
    # (family, invert flag) combinations: 4 x 2, for lq its four alphas in the exact family; the exact and the general family also run
    # through the two argument sources.  Plain and Moreau each.
    combos, with_src = (14, 10) if fn == "lq" else (8, 4)
    assert launches == 2 * (combos * len(SHAPES) + with_src * len(ARG_SOURCE_SHAPES) * 2)


# ---- 2. the fused PDHG families ----------------------------------------------------------------------------------------------------
TAUS, SIGMAS, THETAS = (0.5, 0.7, 0.6, 0.45), (1.1, 1.4, 1.2, 1.3), (0.85, 0.8, 0.9, 0.75)
LANE_COL = 1           # the column whose marked lanes hold the four classes of norms: K^T y = 0 there and in its right neighbour for nx >= 4


def overflowing(dtype):
    return 2.0 ** 64 if dtype == np.float32 else 2.0 ** 600


def fused_edge_data(kind, shape, dtype, g_fn):
    """x, f (L, nx, ny) and y (components, nx, ny) in the kernels' layout (rows fastest), and {first row of a marked lane: its pattern}.
    A lane of the fused kernels owns rows 4j .. 4j+3 of a column.  In the marked lanes x and f are flat (x - f = 1: the threshold of
    'abs' at the step 8 tau T = 1 of the first iteration) and y is constant along every row, so K^T y = 0 away from the first and last
    column, x^(k+1) stays flat, K x = 0 and the dual argument is y itself: zero, an overflowing value and an ordinary one in the first
    horizontal component of three rows, and a NaN in one column of the fourth: in LANE_COL itself for 'abs' (which maps a NaN argument to
    0, so x^(k+1) stays clean), in the column behind it for 'square' (which hands the NaN of K^T y on to x^(k+1): the row then has a NaN
    norm in LANE_COL through its horizontal difference only, and the other three rows keep theirs).  Pattern 0: (NaN, zero | overflow, ordinary) over the two pairs of rows
    that share a reciprocal seed; pattern 1: (ordinary, NaN | zero, overflow).  Elsewhere x and f carry the primal edge operands and y
    is ordinary."""
    nx, ny, L = shape
    comps = 3 * L if kind == "3d" else 2 * L
    hc = list(range(L)) if kind == "3d" else [0]
    rng = np.random.default_rng(1000 * nx + 10 * ny + L)
    x = rng.uniform(0, 1, (L, nx, ny)); f = rng.uniform(0, 1, (L, nx, ny)); y = rng.uniform(-1, 1, (comps, nx, ny))
    marks = {0: 0}
    if ny >= 10:
        marks[8 if ny >= 16 else 4] = 1
    vals = E.operand_values(dtype, 1.0, 0.75, 1.3125, 1.0).astype(np.float64)
    free = np.ones(ny, bool)
    for r in marks:
        free[max(r - 1, 0):r + 5] = False          # the lane and the rows next to it stay ordinary
    k = 0
    for q in np.flatnonzero(free):                 # every third pixel of the other rows: an edge operand in x, another in f
        for c in range(nx):
            for l in range(L):
                if (q + c + l) % 3 == 0:
                    x[l, c, q] = vals[k % len(vals)]; f[l, c, q] = vals[(k + 17) % len(vals)]
                    k += 1
    for r, pattern in marks.items():
        x[:, :, r:r + 4] = 1.25; f[:, :, r:r + 4] = 0.25
        y[:, :, r:r + 4] = 0.0
        if r > 0 and r - 4 not in marks:
            y[:, :, r - 1] = 0.0                   # nothing reaches into the lane from above (a marked lane above has no vertical component already)
        row = dict(zip(("nan", "zero", "huge", "ord") if pattern == 0 else ("ord", "nan", "zero", "huge"), range(r, r + 4)))
        y[hc, :, row["huge"]] = overflowing(dtype)
        y[hc, :, row["ord"]] = 0.3
        y[hc[0], LANE_COL + (g_fn == "square"), row["nan"]] = np.nan
        marks[r] = row
    return x.reshape(-1).astype(dtype), f.reshape(-1).astype(dtype), y.reshape(-1).astype(dtype), marks


def check_lane_classes(nv, kind, shape, dtype, marks):
    """the squared norms of the first dual step: every marked lane has a NaN, a zero, an overflowing and an ordinary one in the four rows
    of LANE_COL"""
    nx, ny, L = shape
    col = (nv.reshape(L, nx, ny)[0] if kind == "3d" else nv.reshape(nx, ny))[LANE_COL]
    for r, row in marks.items():
        assert np.isnan(col[row["nan"]]) and col[row["zero"]] == 0.0 and col[row["huge"]] > np.finfo(dtype).max and 0.01 < col[row["ord"]] < 100.0, (r, col[r:r + 4])
    assert np.isnan(nv).sum() < nv.size // 2


def make_desc(hip, kind, shape, dtype, fns, g_coeffs, tval):
    nx, ny, L = shape
    n = nx * ny * L
    d = hip.FusedDesc()
    d.is3d = 1 if kind == "3d" else 0; d.nx, d.ny, d.L = nx, ny, L
    d.g_fn = hip.FN_ID[fns[0]]; d.f_fn = hip.FN_ID[fns[1]]
    gp, gv, k1 = hip.coeff_args(g_coeffs, dtype, n)
    fp, fv, k2 = hip.coeff_args(F_COEFFS, dtype, n)
    for i in range(7):
        d.g_coeff_ptr[i] = gp[i]; d.g_coeff_val[i] = gv[i]
        d.f_coeff_ptr[i] = fp[i]; d.f_coeff_val[i] = fv[i]
    d.T_val, d.S_val = tval, SVAL
    return d, (k1, k2)


# (8, 16): the smallest image the K-iteration kernel takes (8 columns, heights that are a multiple of 4)
FUSED_CASES = [("2d", (5, 16, 1)), ("2d", (5, 18, 1)), ("2d", (8, 16, 1)), ("mc", (6, 8, 3)), ("3d", (4, 8, 2)), ("3d", (5, 10, 3))]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("fns", [("square", "ind_leq0"), ("abs", "huber")])
@pytest.mark.parametrize("kind,shape", FUSED_CASES)
def test_fused_families_on_directed_operands(hip, dtype, fns, kind, shape):
    """one launch of every fused family of this shape against the oracle's iterations (one, two for the pair kernels, K for the
    K-iteration kernel): identical x and y, NaN positions included"""
    nx, ny, L = shape
    n = nx * ny * L
    dt = 0 if dtype == np.float32 else 1
    vecw = 4 if dtype == np.float32 else 2
    tval = 1.0 / 6.0 if kind == "3d" else 0.25
    x, f, y, marks = fused_edge_data(kind, shape, dtype, fns[0])
    g_coeffs = [1.0, f, 8.0, 0.0, 0.0, 0.3, 0.0]
    its = [(x, y)]
    for k in range(4):
        x1, y1, nv = oracle_iteration(kind, its[-1][0], its[-1][1], shape, g_coeffs, tval, TAUS[k], SIGMAS[k], THETAS[k], dtype, fns[0], fns[1])
        if k == 0:
            check_lane_classes(nv, kind, shape, dtype, marks)
        its.append((x1, y1))
    desc, keep = make_desc(hip, kind, shape, dtype, fns, g_coeffs, tval)
    L_ = hip.lib()
    ref = C.byref(desc)
    dx, dy = hip.DeviceArray.from_host(x), hip.DeviceArray.from_host(y)
    arr = lambda v, k=2: (C.c_double * k)(*v[:k])
    t0, s0, th0 = hip.dbl(TAUS[0]), hip.dbl(SIGMAS[0]), hip.dbl(THETAS[0])
    straight = fns[1] == "ind_leq0"            # the pair and K-iteration kernels of colour images and volumes take the ROF / TV-L1 shapes only
    ran = []

    def compare(family, k, launch, mid=False):
        xo = hip.DeviceArray.from_host(np.full(x.size, 7.0, dtype)); yo = hip.DeviceArray.from_host(np.full(y.size, 7.0, dtype))
        xm = hip.DeviceArray.from_host(np.full(x.size, 7.0, dtype)); ym = hip.DeviceArray.from_host(np.full(y.size, 7.0, dtype))
        launch(xo, yo, xm, ym)
        outs = [("x", xo, its[k][0]), ("y", yo, its[k][1])] + ([("x_mid", xm, its[1][0]), ("y_mid", ym, its[1][1])] if mid else [])
        got = [(name, d.to_host(), want) for name, d, want in outs]
        for d in (xo, yo, xm, ym):
            d.free()
        for name, g, want in got:
            bad = np.flatnonzero(~((g == want) | (np.isnan(g) & np.isnan(want))))
            assert bad.size == 0, (family, name, bad.size, bad[:8], g[bad[:4]], want[bad[:4]])
        ran.append(family)

    assert L_.prost_hip_fused_supported(ref, dt) == 1
    compare("fused_primal+fused_dual", 1, lambda xo, yo, xm, ym: (
        hip.check(hip.fn("fused_primal", dtype)(ref, xo.ptr, dx.ptr, dy.ptr, None, t0, 1, 0, None, None, None)),
        hip.check(hip.fn("fused_dual", dtype)(ref, yo.ptr, dy.ptr, xo.ptr, dx.ptr, s0, th0, 1, None, None, None))))
    if kind == "2d":
        assert L_.prost_hip_fused_iteration_supported(ref, dt) == 1
        compare("fused_iteration", 1, lambda xo, yo, xm, ym: hip.check(hip.fn("fused_iteration", dtype)(ref, xo.ptr, yo.ptr, dx.ptr, dy.ptr, None, t0, s0, th0, 1, 1, 0, 0, None, None, None)))
        assert L_.prost_hip_fused_iteration2_supported(ref, dt) == 1
        for cols in (0, 2):                     # the launcher's chunking, and chunks of two columns
            compare("fused_iteration2", 2, lambda xo, yo, xm, ym: hip.check(hip.fn("fused_iteration2", dtype)(ref, xo.ptr, yo.ptr, dx.ptr, dy.ptr, xm.ptr, ym.ptr,
                    arr(TAUS), arr(SIGMAS), arr(THETAS), cols, None, None, None)), mid=True)
            compare("fused_iteration2", 2, lambda xo, yo, xm, ym: hip.check(hip.fn("fused_iteration2", dtype)(ref, xo.ptr, yo.ptr, dx.ptr, dy.ptr, None, None,
                    arr(TAUS), arr(SIGMAS), arr(THETAS), cols, None, None, None)))
        # the K-iteration kernel in its exact instance (desc.arith = 0): fp32, at least 8 columns, heights that are a multiple of 4, ind_leq0
        kmax = L_.prost_hip_fused_iterationk_max(ref, dt)
        assert kmax == (4 if kmax_of(dtype, nx, ny, straight) else 0)
        for K in ((1, 4) if kmax else ()):
            compare("fused_iterationk", K, lambda xo, yo, xm, ym: hip.check(hip.fn("fused_iterationk", dtype)(ref, K, xo.ptr, yo.ptr, dx.ptr, dy.ptr,
                    arr(TAUS, K), arr(SIGMAS, K), arr(THETAS, K), 0, None, None, None)))
    if kind == "mc":
        assert L_.prost_hip_fused_iteration_mc_supported(ref, dt) == 1
        compare("fused_iteration_mc", 1, lambda xo, yo, xm, ym: hip.check(hip.fn("fused_iteration_mc", dtype)(ref, xo.ptr, yo.ptr, dx.ptr, dy.ptr, None, t0, s0, th0, 1, 1, 0, 0, None, None, None)))
        assert L_.prost_hip_fused_iteration_mc_x2_supported(ref, dt) == (1 if straight else 0)
        for cols in ((0, 2) if straight else ()):
            compare("fused_iteration_mc_x2", 2, lambda xo, yo, xm, ym: hip.check(hip.fn("fused_iteration_mc_x2", dtype)(ref, xo.ptr, yo.ptr, dx.ptr, dy.ptr,
                    arr(TAUS), arr(SIGMAS), arr(THETAS), cols, None, None, None)))
    if kind == "3d":
        whole = ny % vecw == 0                  # the single-iteration volume kernels need whole 16-byte row groups
        assert L_.prost_hip_fused_iteration3d_supported(ref, dt) == (1 if whole else 0)
        assert L_.prost_hip_fused_iteration3d_pw_supported(ref, dt) == (1 if whole else 0)
        if whole:
            compare("fused_iteration3d", 1, lambda xo, yo, xm, ym: hip.check(hip.fn("fused_iteration3d", dtype)(ref, xo.ptr, yo.ptr, dx.ptr, dy.ptr, None, t0, s0, th0, 1, 1, 0, 0, None, None, None)))
            compare("fused_iteration3d_pw", 1, lambda xo, yo, xm, ym: hip.check(hip.fn("fused_iteration3d_pw", dtype)(ref, xo.ptr, yo.ptr, dx.ptr, dy.ptr, t0, s0, th0, 1, 1, 0, 0, None)))
        assert L_.prost_hip_fused_iteration3d_x2_supported(ref, dt) == (1 if straight else 0)
        for cols in ((0, 2) if straight else ()):
            compare("fused_iteration3d_x2", 2, lambda xo, yo, xm, ym: hip.check(hip.fn("fused_iteration3d_x2", dtype)(ref, xo.ptr, yo.ptr, dx.ptr, dy.ptr,
                    arr(TAUS), arr(SIGMAS), arr(THETAS), cols, None, None, None)))
    dx.free(); dy.free()
    del keep
    expect = {"2d": 2 + 4 + (2 if kmax_of(dtype, nx, ny, straight) else 0), "mc": 2 + (2 if straight else 0),
              "3d": 1 + (2 if ny % vecw == 0 else 0) + (2 if straight else 0)}[kind]
    assert len(ran) == expect, ran


def kmax_of(dtype, nx, ny, straight):
    return dtype == np.float32 and nx >= 8 and ny % 4 == 0 and straight


# ---- 3. the solver -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec,dtype", [("single", np.float32), ("double", np.float64)])
@pytest.mark.parametrize("nx,ny", [(8, 16), (19, 248)])
def test_rof_with_a_nan_and_an_infinite_pixel_equals_the_oracle(prec, dtype, nx, ny):
    """ROF with one NaN and one +inf pixel in f, well apart: four iterations (alg2; no residual iteration among them) on the fused path
    equal the oracle's, NaN positions included.  The reference confines such a pixel -- the dual groups that touch it have a NaN norm
    and are written as zero (elem_operation_norm2.hpp:56, :81-87) --, so y has no NaN and x has one at each of the two pixels and nowhere
    else (at the infinite pixel as well: ElemOperation1D forms (-inf + b) / a with b = f = +inf there)."""
    rng = np.random.default_rng(100 * nx + ny)
    f = rng.uniform(0, 1, (nx, ny))
    f[2, 5] = np.nan
    f[nx - 3, ny - 6] = np.inf
    prost.set_precision(prec)
    prob, u, q, _ = synthetic.rof_problem(nx, ny, f=f.reshape(-1))
    backend = prost.backend.pdhg(stepsize="alg2", residual_iter=10, alg2_gamma=0.5)
    opts = prost.options(max_iters=10 ** 6, num_cback_calls=0, verbose=False, tol_rel_primal=0, tol_rel_dual=0, tol_abs_primal=0, tol_abs_dual=0)
    s = prost.Solver(prob, backend, opts)
    s.iterate(4)
    st = s.state()
    s.destroy()
    assert st["path"] == "pdhg:fused-grad2d", st["path"]
    o = oracle.Solver(prob.data, prob.nrows, prob.ncols, backend, opts, dtype)
    o.initialize()
    o.iterate(4)
    ost = o.state()
    assert np.flatnonzero(np.isnan(ost["x"])).tolist() == [2 * ny + 5, (nx - 3) * ny + ny - 6] and np.isnan(ost["y"]).sum() == 0 and np.isfinite(ost["y"]).all()
    for v in "xy":
        g, w = np.asarray(st[v]), np.asarray(ost[v])
        print(v, "NaNs: kernel", int(np.isnan(g).sum()), "oracle", int(np.isnan(w).sum()))
        assert np.array_equal(g, w, equal_nan=True), (v, int(np.isnan(g).sum()), np.flatnonzero(~((g == w) | (np.isnan(g) & np.isnan(w))))[:8])
