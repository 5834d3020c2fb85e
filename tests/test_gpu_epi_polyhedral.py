"""ind_epi_polyhedral on the GPU: the kernel through the C ABI (with its fallback counter), the prox through prost.eval_prox, through
the solver and in examples/tvl1_epigraph.py.

Reference everywhere: tests/epi_polyhedral_reference.py (NumPy), never the code under test.  The truth is its active-set projection
in fp64 (equal to a KKT enumeration: tests/test_epi_polyhedral_reference.py); e_T is the relative error of the same routine run in
precision T on the same inputs.  Per group

    |z - truth|_inf <= max(4 e_T, 32 eps_T) max(1, |z0|_inf, |b|_inf)      (b: the group's own constraints)

and the same bound holds for the distance by which z lies outside any of the group's halfspaces (<a, x> - y - b) / |(a, -1)|_2: the
projection is feasible, so a point within the bound of it is within the bound of every halfspace.  The inputs are float32 values in
both precisions, so the fp64 truth is computed once per case.  No input may need the fallback: the counter has to read 0.
Shapes come from prost_hip_epi_polyhedral_plan: with G lanes per group, group counts 1, 64/G - 1, 64/G, 64/G + 1 and two workgroups'
worth + 3, list lengths 0, 1, 2, G - 1, G, G + 1, 3 G + 1 mixed inside one wave, plus the shortest length for which the plan answers
G, so that the longest list of the case is one the plan gives G lanes (asserted).  The observed worst ratios are in docs/rounds/r14.md.

Solves: min_z 1/2 |z - f|^2 + ind_epi(z) with K = identity and conjugate(sum_ind_epi_polyhedral(..)) as f* has the closed form
z = P f.  The distance reached after a fixed iteration count was measured once (docs/rounds/r14.md); ten times it is asserted.
"""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

import epi_polyhedral_reference as R
import prost_amd as prost
from prost_amd import _hip

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))

pytestmark = pytest.mark.gpu

PRECISIONS = [("single", np.float32), ("double", np.float64)]
BLOCK = 256
WORST = {}          # (test, precision) -> the largest distance / bound seen; printed per test


def plan(max_count, dim, dtype):
    L = _hip.lib()
    L.prost_hip_epi_polyhedral_plan.argtypes = [C.c_size_t, C.c_size_t, C.c_int] + [C.POINTER(C.c_int)] * 3
    L.prost_hip_epi_polyhedral_plan.restype = C.c_int
    lanes, ca, cb = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    assert L.prost_hip_epi_polyhedral_plan(int(max_count), dim, 0 if np.dtype(dtype) == np.float32 else 1, C.byref(lanes), C.byref(ca), C.byref(cb)) == 0
    return lanes.value, ca.value, cb.value


def f32(x):
    return np.asarray(x, np.float64).astype(np.float32).astype(np.float64)


def run_kernel(dtype, interleaved, z0, a, b, cnt, idx, max_count=None):
    """one launch through the C ABI -> (z (N, dim), fallback counter)"""
    z0 = np.asarray(z0, np.float64)
    N, dim = z0.shape
    flat = (z0 if interleaved else z0.T).ravel().astype(dtype)
    keep = [_hip.DeviceArray.from_host(flat), _hip.DeviceArray.zeros(flat.size, dtype),
            _hip.DeviceArray.from_host(np.asarray(a, np.float64).ravel().astype(dtype)), _hip.DeviceArray.from_host(np.asarray(b, np.float64).ravel().astype(dtype)),
            _hip.DeviceArray.from_host(np.asarray(cnt).astype(np.int32)), _hip.DeviceArray.from_host(np.asarray(idx).astype(np.int32)),
            _hip.DeviceArray.zeros(1, np.uint32)]
    arg, res, da, db, dc, di, fb = keep
    mc = int(np.max(cnt)) if max_count is None else int(max_count)
    fn = _hip.fn("prox_ind_epi_polyhedral", dtype)
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int] + [C.c_void_p] * 4 + [C.c_size_t, C.c_void_p, C.c_void_p]
    fn.restype = C.c_int
    try:
        _hip.check(fn(res.ptr, arg.ptr, N, dim, 1 if interleaved else 0, da.ptr, db.ptr, dc.ptr, di.ptr, mc, fb.ptr, None))
        _hip.sync()
        out = res.to_host().astype(np.float64)
        fallback = int(fb.to_host()[0])
    finally:
        for d in keep:
            d.free()
    return (out.reshape(N, dim) if interleaved else out.reshape(dim, N).T), fallback


def reference(z0, a, b, cnt, idx, dtype):
    """-> truth (fp64), bound per group for precision `dtype`"""
    truth = R.project_active_set(z0, a, b, cnt, idx, np.float64)
    info = {}
    zt = R.project_active_set(z0, a, b, cnt, idx, dtype, info).astype(np.float64)
    assert not info["capped"].any()
    N = z0.shape[0]
    bmax = np.array([np.abs(b[idx[g]:idx[g] + cnt[g]]).max() if cnt[g] else 0.0 for g in range(N)])
    scale = np.maximum(1.0, np.maximum(np.abs(z0).max(axis=1), bmax))
    e_t = np.abs(zt - truth).max(axis=1) / scale
    return truth, np.maximum(4 * e_t, 32 * np.finfo(dtype).eps) * scale


def check(tag, precision, z, fallback, truth, bound, a, b, cnt, idx):
    assert fallback == 0, (tag, fallback)
    assert np.isfinite(z).all(), tag
    dist = np.abs(z - truth).max(axis=1)
    outside = np.maximum(R.halfspace_distance(z, a, b, cnt, idx), 0.0)
    ratio = max(float((dist / bound).max()), float((outside / bound).max()))
    WORST[(tag.split(":")[0], precision)] = max(WORST.get((tag.split(":")[0], precision), 0.0), ratio)
    print("%s %s: distance / bound %.3f, outside / bound %.3f" % (tag, precision, (dist / bound).max(), (outside / bound).max()))
    g = int(np.argmax(dist / bound))
    assert (dist <= bound).all(), (tag, g, dist[g], bound[g])
    assert (outside <= bound).all(), (tag, int(np.argmax(outside / bound)))


@functools.lru_cache(maxsize=None)
def shape_case(dim, lanes, scale, dtype_name):
    """the mixed-length lists of one G, 2 * 256 / G + 3 groups; smaller group counts are prefixes"""
    dtype = np.dtype(dtype_name).type
    G = lanes
    first = next(m for m in range(0, 4096) if plan(m, dim, dtype)[0] == G)        # the shortest longest-list that the plan answers G for
    ks = [0, 1, 2, G - 1, G, G + 1, 3 * G + 1, first]
    assert plan(max(ks), dim, dtype)[0] == G
    count = 2 * BLOCK // G + 3
    rng = np.random.default_rng(1000 * dim + lanes)
    a, b, cnt, idx = R.random_lists(rng, count, dim, ks)
    a, b = f32(a), f32(b)
    z0 = f32(scale * rng.standard_normal((count, dim)))
    truth, bound = reference(z0, a, b, cnt, idx, dtype)
    return a, b, cnt, idx, z0, truth, bound


@pytest.mark.parametrize("lanes", [1, 2, 8, 64])
@pytest.mark.parametrize("dim", [2, 3, 4])
@pytest.mark.parametrize("precision,dtype", PRECISIONS)
def test_shapes_layouts_and_mixed_list_lengths(precision, dtype, dim, lanes):
    per_wave = 64 // lanes
    for scale in (1000.0, 1.0):
        a, b, cnt, idx, z0, truth, bound = shape_case(dim, lanes, scale, np.dtype(dtype).name)
        full = len(cnt)
        for count in sorted({1, max(per_wave - 1, 1), per_wave, per_wave + 1, full}):
            for interleaved in (False, True):
                # max_count stays that of the whole case, so every group count runs with the same G
                z, fb = run_kernel(dtype, interleaved, z0[:count], a, b, cnt[:count], idx[:count], max_count=cnt.max())
                check("shapes:dim%d G%d scale%g count%d %s" % (dim, lanes, scale, count, "interleaved" if interleaved else "planar"),
                      precision, z, fb, truth[:count], bound[:count], a, b, cnt[:count], idx[:count])
    print("worst ratio so far (%s): %.3f" % (precision, WORST[("shapes", precision)]))


@pytest.mark.parametrize("dim", [2, 3, 4])
@pytest.mark.parametrize("precision,dtype", PRECISIONS)
def test_shared_list_and_shuffled_index_vec(precision, dtype, dim):
    rng = np.random.default_rng(77 + dim)
    for shared, shuffle in ((True, False), (False, True)):
        count = 131
        a, b, cnt, idx = R.random_lists(rng, count, dim, [25] if shared else [0, 3, 7, 25, 1, 12], shared=shared, shuffle=shuffle)
        assert (shared and (idx == 0).all()) or (shuffle and (np.diff(idx) < 0).any())
        a, b = f32(a), f32(b)
        for scale in (1000.0, 1.0):
            z0 = f32(scale * rng.standard_normal((count, dim)))
            truth, bound = reference(z0, a, b, cnt, idx, dtype)
            for interleaved in (False, True):
                z, fb = run_kernel(dtype, interleaved, z0, a, b, cnt, idx)
                check("lists:dim%d %s scale%g" % (dim, "shared" if shared else "shuffled", scale), precision, z, fb, truth, bound, a, b, cnt, idx)


@pytest.mark.parametrize("dim", [2, 3, 4])
@pytest.mark.parametrize("precision,dtype", PRECISIONS)
def test_directed_cases(precision, dtype, dim):
    d = dim - 1
    for name, (a, b, pts) in R.directed_cases(dim).items():
        a, b, pts = f32(a), f32(b), f32(pts)
        P, m = len(pts), b.size
        cnt, idx = np.full(P, m), np.zeros(P, int)
        truth, bound = reference(pts, a, b, cnt, idx, dtype)
        for interleaved in (False, True):
            z, fb = run_kernel(dtype, interleaved, pts, a, b, cnt, idx)
            check("directed:dim%d %s" % (dim, name), precision, z, fb, truth, bound, a, b, cnt, idx)
        if name in ("linf_pyramid", "l1_pyramid"):
            assert (np.abs(z[:8]).max(axis=1) <= bound[:8]).all(), name           # the polar cone lands on the apex
    # feasible points, on the boundary and inside, come back bit for bit; so does everything when a group has no constraints
    a, b, pts = R.directed_cases(dim)["linf_pyramid"]
    f = pts.astype(dtype)
    f[:, -1] = np.abs(f[:, :d]).max(axis=1) + np.array([0.0, 1.0] * (len(pts) // 2)).astype(dtype)
    for interleaved in (False, True):
        for cnt in (np.full(len(f), b.size), np.zeros(len(f), int)):
            z, fb = run_kernel(dtype, interleaved, f, a, b, cnt, np.zeros(len(f), int), max_count=b.size)
            assert fb == 0 and np.array_equal(z.astype(dtype), f)


@pytest.mark.parametrize("dim", [2, 3, 4])
@pytest.mark.parametrize("precision,dtype", PRECISIONS)
def test_one_constraint_is_the_halfspace_projection(precision, dtype, dim):
    """k = 1: the epigraph of one affine function is the halfspace <(a, -1), z> <= b, which sum_ind_halfspace projects onto"""
    rng = np.random.default_rng(5 + dim)
    count = 70
    a, b = f32(rng.standard_normal((count, dim - 1))), f32(rng.standard_normal(count))
    z0 = f32(10 * rng.standard_normal((count, dim)))
    cnt, idx = np.ones(count, int), np.arange(count)
    truth, bound = reference(z0, a, b, cnt, idx, dtype)
    prost.set_precision(precision)
    try:
        arg = z0.T.ravel()
        normals = np.concatenate([a, -np.ones((count, 1))], axis=1).T.ravel()               # planar, like the argument
        half, _ = prost.eval_prox(prost.function.sum_ind_halfspace(dim, False, normals, b), arg, 1, np.ones(arg.size))
        epi, _ = prost.eval_prox(prost.function.sum_ind_epi_polyhedral(dim, False, a, b, cnt, idx), arg, 1, np.ones(arg.size))
    finally:
        prost.set_precision("double")
    half, epi = np.asarray(half, np.float64).reshape(dim, count).T, np.asarray(epi, np.float64).reshape(dim, count).T
    assert (np.abs(epi - half).max(axis=1) <= bound).all()
    assert (np.abs(epi - truth).max(axis=1) <= bound).all()


@pytest.mark.parametrize("d", [1, 2])
@pytest.mark.parametrize("precision,dtype", PRECISIONS)
def test_the_reference_projects_own_test_restated(precision, dtype, d):
    """test_prox_sum_ind_epi_polyhedral.m: m = 25 pieces, N = 250 points of scale 1000, the list repeated per point, planar, through
    eval_prox; its bound: |dx|_2 + |dy| <= 1e-3 per point (there against quadprog, here against the fp64 truth)"""
    m, N = 25, 250
    rng = np.random.default_rng(8954 + d)
    coeff_a, coeff_b = f32(rng.standard_normal((m, d))), f32(rng.standard_normal(m))
    x0, y0 = f32(1000 * rng.standard_normal((N, d))), f32(1000 * rng.standard_normal(N))
    rep_a, rep_b = np.tile(coeff_a.ravel(), N), np.tile(coeff_b, N)
    count_vec = np.full(N, m)
    index_vec = np.cumsum(count_vec) - m
    z0 = np.concatenate([x0, y0[:, None]], axis=1)
    truth = R.project_active_set(z0, coeff_a, coeff_b, count_vec, np.zeros(N, int))
    prost.set_precision(precision)
    try:
        for tau, Tau in ((1, np.ones(N * (d + 1))), (0.3, np.linspace(0.5, 2, N * (d + 1)))):     # an indicator's prox ignores the steps
            res, _ = prost.eval_prox(prost.function.sum_ind_epi_polyhedral(d + 1, False, rep_a, rep_b, count_vec, index_vec), z0.T.ravel(), tau, Tau)
            z = np.asarray(res, np.float64).reshape(d + 1, N).T
            diff = np.linalg.norm(z[:, :d] - truth[:, :d], axis=1) + np.abs(z[:, d] - truth[:, d])
            print("d = %d %s: largest |dx| + |dy| = %.3g" % (d, precision, diff.max()))
            assert (diff <= 1e-3).all(), (int(np.argmax(diff)), diff.max())
    finally:
        prost.set_precision("double")


def test_the_example_runs_and_its_solution_is_feasible():
    import tvl1_epigraph
    prost.set_precision("double")
    nx, ny = 32, 24
    result, e_epi, e_abs, u, t, f = tvl1_epigraph.main(nx, ny, max_iters=2000, verbose=False)
    assert np.isfinite(e_epi) and np.isfinite(e_abs) and np.isfinite(u).all() and np.isfinite(t).all()
    assert u.size == nx * ny and t.size == nx * ny
    # (u, t) lies in the epigraph of |u - f|: the primal iterate is the output of the prox, up to the bound of the kernel tests
    bound = 32 * np.finfo(np.float64).eps * np.maximum(1.0, np.maximum(np.maximum(np.abs(u), np.abs(t)), np.abs(f)))
    assert (np.abs(u - f) - t <= np.sqrt(2) * bound).all(), float((np.abs(u - f) - t).max())
    print("energies: epigraph form %.6f, sum_1d('abs') form %.6f" % (e_epi, e_abs))


# relative inf-norm distance to the closed form after SOLVE_ITERS iterations, measured once on an MI355X; ten times it is asserted
SOLVE_ITERS = 1000
SOLVE_DISTANCE = {
    ("plain", "single"): 9.39e-06,
    ("plain", "double"): 4.01e-06,
    ("transform", "single"): 9.39e-06,
    ("transform", "double"): 4.01e-06,
}


def _solve_problem(dtype, wrapped):
    """40 groups, dim 3, m = 7, interleaved; f* = conjugate(ind_epi) or conjugate(transform(ind_epi, 2, 1)): the indicator of
    { z | 2 z - 1 in C }, whose projection is (P_C(2 f - 1) + 1) / 2"""
    rng = np.random.default_rng(314)
    count, dim, m = 40, 3, 7
    a, b, cnt, idx = R.random_lists(rng, count, dim, [m])
    a, b = f32(a), f32(b)
    F = f32(3 * rng.standard_normal((count, dim)))
    fun = prost.function.sum_ind_epi_polyhedral(dim, True, a, b, cnt, idx)
    if wrapped:
        fun = prost.function.transform(fun, 2, 1, 1, 0, 0)
        want = (R.project_active_set(2 * F - 1, a, b, cnt, idx) + 1) / 2
    else:
        want = R.project_active_set(F, a, b, cnt, idx)
    u, q = prost.variable(count * dim), prost.variable(count * dim)
    prob = prost.min_max_problem([u], [q])
    prob.add_function(u, prost.function.sum_1d("square", 1, F.ravel(), 1))
    prob.add_function(q, prost.function.conjugate(fun))
    prob.add_dual_pair(u, q, prost.block.identity())
    return prob, want.ravel()


@pytest.mark.parametrize("kind,precision", sorted(SOLVE_DISTANCE))
def test_solves_reach_the_projection(kind, precision):
    dtype = dict(PRECISIONS)[precision]
    prost.set_precision(precision)
    try:
        prob, want = _solve_problem(dtype, kind == "transform")
        o = prost.options(max_iters=SOLVE_ITERS, num_cback_calls=0, verbose=False, tol_rel_primal=0, tol_rel_dual=0, tol_abs_primal=0, tol_abs_dual=0)
        s = prost.Solver(prob, prost.backend.pdhg(stepsize="alg2", residual_iter=10, alg2_gamma=0.5), o)
        s.iterate(SOLVE_ITERS)
        st = s.state()
        s.destroy()
    finally:
        prost.set_precision("double")
    assert st["path"] == "pdhg:generic", st["path"]
    rel = float(np.abs(st["x"].astype(np.float64).ravel() - want).max()) / float(np.abs(want).max())
    print("solve %s %s: relative distance %.3g after %d iterations" % (kind, precision, rel, SOLVE_ITERS))
    assert rel <= 10 * SOLVE_DISTANCE[(kind, precision)], rel
