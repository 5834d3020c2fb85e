"""ind_epi_conjquad_1d on the GPU: the kernel through the C ABI (with its fallback counter), the prox through prost.eval_prox, through
the solver and in examples/quadratic_data_epigraph.py.

Reference everywhere: tests/epi_conjquad_reference.py (NumPy), never the code under test.  The truth P is its run in fp64 on the
float32-rounded inputs (equal to answers known by construction within 64 eps_64: tests/test_epi_conjquad_reference.py); e_T is the
relative error of the same routine run in precision T.  Per group

    |z - P|_inf <= max(4 e_T, 32 eps_T) max(1, |z0|_inf, |P|_inf)

and the same bound holds for max(phi*(y) - t, 0) of the result (phi* evaluated in long double).  The fallback counter has to read 0
and every result is finite.  Random cases are built from their answers with a prescribed share of every region, asserted from the
reference's labels on the full case (515 groups; smaller group counts are its prefixes): inside, left, right and arc at least 15 %
each and vertex at least 5 %.  Where `a` is ONE scalar for all groups the piece has either an arc (a > 0) or a vertex (a = 0), never
both: the all-scalar cases come in those two flavours and the share of the region that cannot occur is not asked for.

Solves: min_z 1/2 |z - f|^2 + ind_epi(z) with K = identity and conjugate(sum_ind_epi_conjquad_1d(..)) as f* has the closed form
z = P f.  The distance reached after a fixed iteration count was measured once (docs/rounds/r15.md); ten times it is asserted.
"""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

import epi_conjquad_reference as R
import prost_amd as prost
from prost_amd import _hip

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))

pytestmark = pytest.mark.gpu

PRECISIONS = [("single", np.float32), ("double", np.float64)]
NAMES = ("a", "b", "c", "alpha", "beta")
FULL = 515
COUNTS = (1, 63, 64, 65, 255, 256, 257, 515)
# which coefficients are one scalar for all groups
MODES = {
    "scalars_arc": dict(a=0.75, b=0.5, c=-0.25, alpha=-1.5, beta=2.0),
    "scalars_vertex": dict(a=0.0, b=0.5, c=-0.25, alpha=-1.5, beta=2.0),
    "vectors": {},
    "mixed": dict(b=0.5, alpha=-1.5),
}
WORST = {}


def launch(dtype, interleaved, z0, co, offset=0, in_place=False):
    """one launch through the C ABI -> (z (N, 2), fallback counter).  co: dict name -> array of 1 or N values.  offset: arg and res
    start that many elements into their allocations."""
    z0 = np.asarray(z0, np.float64)
    N = z0.shape[0]
    flat = (z0 if interleaved else z0.T).ravel().astype(dtype)
    pad = np.zeros(offset, dtype)
    keep = [_hip.DeviceArray.from_host(np.concatenate([pad, flat])), _hip.DeviceArray.zeros(flat.size + offset, dtype), _hip.DeviceArray.zeros(1, np.uint32)]
    arg, res, fb = keep
    if in_place:
        res = arg
    args = []
    for name in NAMES:
        v = np.atleast_1d(np.asarray(co[name], np.float64))
        assert v.size in (1, N), (name, v.size, N)
        if v.size > 1 or N == 1 and name in co.get("as_vector", ()):
            d = _hip.DeviceArray.from_host(v.astype(dtype))
            keep.append(d)
            args += [d.ptr, C.c_double(0.0)]
        else:
            args += [None, C.c_double(float(v[0]))]
    fn = _hip.fn("prox_ind_epi_conjquad_1d", dtype)
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int] + [C.c_void_p, C.c_double] * 5 + [C.c_void_p, C.c_void_p, C.c_void_p]
    fn.restype = C.c_int
    try:
        _hip.check(fn(res.offset(offset), arg.offset(offset), N, 1 if interleaved else 0, *args, fb.ptr, None, None))
        _hip.sync()
        out = res.to_host()[offset:].astype(np.float64)
        fallback = int(fb.to_host()[0])
    finally:
        for d in keep:
            d.free()
    return (out.reshape(N, 2) if interleaved else out.reshape(2, N).T), fallback


def reference(z0, co, dtype):
    """-> truth (N, 2) in fp64, bound per group for precision `dtype`, region labels"""
    c5 = [co[n] for n in NAMES]
    y, t, region = R.project(z0[:, 0], z0[:, 1], *c5, np.float64)
    info = {}
    yt, tt, _ = R.project(z0[:, 0], z0[:, 1], *c5, dtype, info=info)
    assert not info["capped"].any()
    truth = np.stack([y, t], axis=1)
    scale = np.maximum(1.0, np.maximum(np.abs(z0).max(axis=1), np.abs(truth).max(axis=1)))
    e_t = np.maximum(np.abs(yt.astype(np.float64) - y), np.abs(tt.astype(np.float64) - t)) / scale
    return truth, np.maximum(4 * e_t, 32 * np.finfo(dtype).eps) * scale, region


def check(tag, precision, z, fallback, truth, bound, co):
    assert fallback == 0, (tag, fallback)
    assert np.isfinite(z).all(), tag
    dist = np.abs(z - truth).max(axis=1)
    out = R.outside(z[:, 0], z[:, 1], *[co[n] for n in NAMES])
    ratio = max(float((dist / bound).max()), float((out / bound).max()))
    key = (tag.split(":")[0], precision)
    WORST[key] = max(WORST.get(key, 0.0), ratio)
    print("%s %s: distance / bound %.3f, outside / bound %.3f" % (tag, precision, (dist / bound).max(), (out / bound).max()))
    g = int(np.argmax(dist / bound))
    assert (dist <= bound).all(), (tag, g, dist[g], bound[g])
    assert (out <= bound).all(), (tag, int(np.argmax(out / bound)))


def prefix(co, n):
    return {k: (v if np.size(v) == 1 else v[:n]) for k, v in co.items()}


@functools.lru_cache(maxsize=None)
def shape_case(mode, scale, dtype_name):
    """FULL groups of one coefficient mode and scale, inputs rounded to float32, with the truth and the bound for dtype"""
    dtype = np.dtype(dtype_name).type
    rng = np.random.default_rng(100 * sorted(MODES).index(mode) + int(scale))
    cs = R.random_cases(rng, FULL, scale, fixed=MODES[mode])
    co = {n: cs[n] for n in NAMES}
    z0 = R.f32(cs["z0"])
    truth, bound, region = reference(z0, co, dtype)
    share = np.bincount(region, minlength=5) / region.size
    fixed_a = MODES[mode].get("a")
    for r in (R.INSIDE, R.LEFT, R.RIGHT, R.ARC, R.VERTEX):
        if fixed_a is not None and r == (R.VERTEX if fixed_a > 0 else R.ARC):
            assert share[r] == 0
            continue
        assert share[r] >= (0.05 if r == R.VERTEX else 0.15), (mode, scale, R.REGION_NAMES[r], share)
    return co, z0, truth, bound


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("precision,dtype", PRECISIONS)
def test_shapes_layouts_scales_and_coefficient_modes(precision, dtype, mode):
    for scale in (1.0, 1000.0):
        co, z0, truth, bound = shape_case(mode, scale, np.dtype(dtype).name)
        for count in COUNTS:
            for interleaved in (False, True):
                c = prefix(co, count)
                if count == 1:
                    c["as_vector"] = tuple(n for n in NAMES if np.size(co[n]) > 1)      # a vector of one entry still goes in as a pointer
                z, fb = launch(dtype, interleaved, z0[:count], c)
                check("shapes:%s scale%g count%d %s" % (mode, scale, count, "interleaved" if interleaved else "planar"), precision, z, fb,
                      truth[:count], bound[:count], c)
    print("worst ratio so far (%s): %.3f" % (precision, WORST[("shapes", precision)]))


@pytest.mark.parametrize("precision,dtype", PRECISIONS)
def test_unaligned_interleaved_pointers_and_in_place(precision, dtype):
    """arg / res one element into their allocations (what a prox at an odd index hands in): aligned for an element, not for a pair;
    and res == arg, aligned and not, in both layouts"""
    co, z0, truth, bound = shape_case("vectors", 1000.0, np.dtype(dtype).name)
    for count in (1, 64, 257):
        c = prefix(co, count)
        c["as_vector"] = NAMES
        for offset in (1, 0, 2):
            for in_place in (False, True):
                for interleaved in ((True,) if not in_place else (True, False)):
                    z, fb = launch(dtype, interleaved, z0[:count], c, offset=offset, in_place=in_place)
                    check("alignment:count%d offset%d %s%s" % (count, offset, "interleaved" if interleaved else "planar", " in place" if in_place else ""),
                          precision, z, fb, truth[:count], bound[:count], c)


@pytest.mark.parametrize("precision,dtype", PRECISIONS)
def test_directed_cases(precision, dtype):
    for scale in (1.0, 1000.0):
        for name, cs in R.directed_cases(scale).items():
            co = {n: R.f32(cs[n]) for n in NAMES}
            z0 = R.f32(cs["z0"])
            truth, bound, _ = reference(z0, co, dtype)
            co["as_vector"] = NAMES
            for interleaved in (False, True):
                z, fb = launch(dtype, interleaved, z0, co)
                check("directed:%s scale%g" % (name, scale), precision, z, fb, truth, bound, co)
    # a feasible point, on the boundary in T or above it, comes back bit for bit
    cs = R.random_cases(np.random.default_rng(3), 300, 10.0, shares=((R.INSIDE, 1.0),))
    co = {n: cs[n] for n in NAMES}
    z0 = R.f32(cs["z0"]).astype(dtype)
    z0[:, 1] = np.maximum(z0[:, 1], R.conj(z0[:, 0], *[co[n] for n in NAMES], dtype=dtype)) + np.array([0.0, 1.0] * 150).astype(dtype)
    for interleaved in (False, True):
        z, fb = launch(dtype, interleaved, z0, co)
        assert fb == 0 and np.array_equal(z.astype(dtype), z0)


@pytest.mark.parametrize("precision,dtype", PRECISIONS)
def test_through_eval_prox(precision, dtype):
    """count = 257 through the factory and the prox class, both layouts, three coefficient modes; tau and the diagonal steps are
    ignored.  (prost.eval_prox evaluates a prox on a vector of exactly its own size, so it cannot place one at an odd index of a larger
    variable: the solves below do that, and the alignment test above hands the kernel such pointers.)"""
    count = 257
    prost.set_precision(precision)
    try:
        for mode in ("vectors", "mixed", "scalars_arc"):
            co, z0, truth, bound = shape_case(mode, 1000.0, np.dtype(dtype).name)
            c = prefix(co, count)
            for interleaved in (False, True):
                fun = prost.function.sum_ind_epi_conjquad_1d(interleaved, *[c[n] for n in NAMES])
                arg = (z0[:count] if interleaved else z0[:count].T).ravel()
                for tau, Tau in ((1, np.ones(arg.size)), (0.3, np.linspace(0.5, 2, arg.size))):
                    res, _ = prost.eval_prox(fun, arg, tau, Tau)
                    got = np.asarray(res, np.float64).ravel()
                    z = got.reshape(count, 2) if interleaved else got.reshape(2, count).T
                    check("eval_prox:%s %s" % (mode, "interleaved" if interleaved else "planar"), precision, z, 0, truth[:count], bound[:count], c)
    finally:
        prost.set_precision("double")


@pytest.mark.parametrize("precision,dtype", PRECISIONS)
def test_infinite_bounds_equal_ind_epi_quad(precision, dtype):
    """alpha = -inf, beta = +inf: the epigraph of (y - b)^2 / (4 a) - c, which sum_ind_epi_quad(2, ..) projects onto with
    a' = 1 / (4 a), b' = -b / (2 a), c' = b^2 / (4 a) - c; 2e-5 relative is the figure the project states for that kernel
    (tests/test_gpu_kernels.py), on inputs of the kind it is stated for"""
    rng = np.random.default_rng(6)
    count = 2000
    a, b, c = R.f32(rng.uniform(0.125, 0.5, count)), R.f32(rng.uniform(-1, 1, count)), R.f32(rng.uniform(-1, 1, count))
    z0 = R.f32(rng.uniform(-2, 2, (count, 2)))
    prost.set_precision(precision)
    try:
        # ProxIndEpiQuad is planar whatever its flag says (as in the reference): it runs once, planar, for both layouts of the new prox
        old, _ = prost.eval_prox(prost.function.sum_ind_epi_quad(2, False, 1 / (4 * a), -b / (2 * a), b * b / (4 * a) - c), z0.T.ravel(), 1, np.ones(2 * count))
        old = np.asarray(old, np.float64).ravel().reshape(2, count).T
        for interleaved in (False, True):
            arg = (z0 if interleaved else z0.T).ravel()
            new, _ = prost.eval_prox(prost.function.sum_ind_epi_conjquad_1d(interleaved, a, b, c, -np.inf, np.inf), arg, 1, np.ones(arg.size))
            new = np.asarray(new, np.float64).ravel()
            new = new.reshape(count, 2) if interleaved else new.reshape(2, count).T
            rel = np.abs(new - old).max(axis=1) / np.maximum(1.0, np.maximum(np.abs(z0).max(axis=1), np.abs(old).max(axis=1)))
            print("%s %s: largest relative difference to ind_epi_quad %.3g" % (precision, "interleaved" if interleaved else "planar", rel.max()))
            assert (rel <= 2e-5).all(), rel.max()
            assert (new != z0).any(axis=1).mean() > 0.3                     # the projection moves a good share of the points
    finally:
        prost.set_precision("double")


# relative inf-norm distance to the closed form after SOLVE_ITERS iterations, measured once on an MI355X; ten times it is asserted
SOLVE_ITERS = 1000
SOLVE_DISTANCE = {
    "single": 7.68e-06,
    "double": 4.14e-06,
}


def _solve_case():
    rng = np.random.default_rng(271)
    cs = R.random_cases(rng, 40, 3.0)
    co = [cs[n] for n in NAMES]
    F = R.f32(cs["z0"])
    y, t, region = R.project(F[:, 0], F[:, 1], *co)
    assert len(set(region)) == 5
    return co, F, np.stack([y, t], axis=1)


@pytest.mark.parametrize("precision", sorted(SOLVE_DISTANCE))
def test_solve_reaches_the_projection(precision):
    """40 groups, interleaved, K = identity, g = 1/2 |z - f|^2, f* = conjugate(ind_epi_conjquad_1d), alg2.  Three more entries in
    front of both variables (f* = 0 there, so their part of x goes to its own data) put the prox at index 3: its pairs start at an
    odd element of the dual variable"""
    co, F, want = _solve_case()
    prost.set_precision(precision)
    try:
        w, u, p, q = prost.variable(3), prost.variable(80), prost.variable(3), prost.variable(80)
        prob = prost.min_max_problem([w, u], [p, q])
        prob.add_function(w, prost.function.sum_1d("square", 1, [1.0, 2.0, 3.0], 1))
        prob.add_function(u, prost.function.sum_1d("square", 1, F.ravel(), 1))
        prob.add_function(p, prost.function.sum_1d("ind_eq0", 1, 0, 1))
        prob.add_function(q, prost.function.conjugate(prost.function.sum_ind_epi_conjquad_1d(True, *co)))
        prob.add_dual_pair(w, p, prost.block.identity())
        prob.add_dual_pair(u, q, prost.block.identity())
        o = prost.options(max_iters=SOLVE_ITERS, num_cback_calls=0, verbose=False, tol_rel_primal=0, tol_rel_dual=0, tol_abs_primal=0, tol_abs_dual=0)
        s = prost.Solver(prob, prost.backend.pdhg(stepsize="alg2", residual_iter=10, alg2_gamma=0.5), o)
        s.iterate(SOLVE_ITERS)
        st = s.state()
        s.destroy()
    finally:
        prost.set_precision("double")
    assert st["path"] == "pdhg:generic", st["path"]
    rel = float(np.abs(st["x"].astype(np.float64).ravel()[3:] - want.ravel()).max()) / float(np.abs(want).max())
    print("solve %s: relative distance %.3g after %d iterations" % (precision, rel, SOLVE_ITERS))
    assert rel <= 10 * SOLVE_DISTANCE[precision], rel


@pytest.mark.parametrize("side", ["conjugate", "primal"])
@pytest.mark.parametrize("precision,dtype", PRECISIONS)
def test_boyd_keeps_the_rule_on_the_device(precision, dtype, side):
    """the same solve under boyd with residual_iter = 1 reports the device-resident rule: the prox does not depend on the step, so
    behind conjugate() the Moreau wrap reads the step in its two scaling passes on the device and the kernel only takes the stop word
    (Prox::takes_step_view).  primal: the same minimisation with the indicator as g and conjugate(1/2 |. - f|^2) as f*, where the
    prox itself is in the list; its primal iterate is an output of the prox: feasible within the kernel's bound"""
    co, F, want = _solve_case()
    k = 300
    ind = prost.function.sum_ind_epi_conjquad_1d(True, *co)
    square = prost.function.sum_1d("square", 1, F.ravel(), 1)
    prost.set_precision(precision)
    try:
        w, u, p, q = prost.variable(3), prost.variable(80), prost.variable(3), prost.variable(80)
        prob = prost.min_max_problem([w, u], [p, q])
        prob.add_function(w, prost.function.sum_1d("square", 1, [1.0, 2.0, 3.0], 1))
        prob.add_function(u, square if side == "conjugate" else ind)
        prob.add_function(p, prost.function.sum_1d("ind_eq0", 1, 0, 1))
        prob.add_function(q, prost.function.conjugate(ind if side == "conjugate" else square))
        prob.add_dual_pair(w, p, prost.block.identity())
        prob.add_dual_pair(u, q, prost.block.identity())
        o = prost.options(max_iters=k, num_cback_calls=0, verbose=False, tol_rel_primal=0, tol_rel_dual=0, tol_abs_primal=0, tol_abs_dual=0)
        s = prost.Solver(prob, prost.backend.pdhg(stepsize="boyd", residual_iter=1), o)
        s.iterate(k)
        st = s.state()
        s.destroy()
    finally:
        prost.set_precision("double")
    assert st["path"] == "pdhg:generic", st["path"]
    assert st["device_rule_batches"] > 0, st["device_rule_batches"]
    z = st["x"].astype(np.float64).ravel()[3:].reshape(40, 2)
    assert np.isfinite(z).all()
    rel = float(np.abs(z - want).max()) / float(np.abs(want).max())
    print("boyd %s %s: relative distance %.3g after %d iterations, %d device rule batches" % (side, precision, rel, k, st["device_rule_batches"]))
    # not a rate: x starts at 0 (distance 1) and f itself is at distance O(1) of P f; a tenth of that says the prox took part
    assert rel <= 0.1, rel
    if side == "primal":
        _, bound, _ = reference(z, dict(zip(NAMES, co)), dtype)
        assert (R.outside(z[:, 0], z[:, 1], *co) <= bound).all()


def test_the_example_agrees_with_the_direct_form_and_its_dual_is_feasible():
    import quadratic_data_epigraph as ex
    prost.set_precision("double")
    nx, ny = 32, 24
    result, e_lifted, e_direct, u, r, s, (a, b, c) = ex.main(nx, ny, max_iters=5000, verbose=False)
    print("energies: lifted form %.6f, direct form %.6f, relative difference %.3g" % (e_lifted, e_direct, abs(e_lifted - e_direct) / abs(e_direct)))
    assert np.isfinite([e_lifted, e_direct]).all() and np.isfinite(u).all() and np.isfinite(r).all() and np.isfinite(s).all()
    assert u.size == r.size == s.size == nx * ny
    # ten times the relative difference examples/tvl1_epigraph.py shows between its two forms at this size (docs/rounds/r14.md: 3.2e-6)
    assert abs(e_lifted - e_direct) <= 10 * 3.2e-6 * abs(e_direct), (e_lifted, e_direct)
    # (r, s) lies in the epigraph of phi*: the dual iterate is an output of the prox, up to the bound of the kernel tests
    co = (a, b, c, ex.GAMMA_1, ex.GAMMA_1 + ex.DELTA)
    z0 = np.stack([r, s], axis=1)
    truth, bound, _ = reference(z0, dict(zip(NAMES, co)), np.float64)
    assert (R.outside(r, s, *co) <= bound).all(), float(R.outside(r, s, *co).max())
