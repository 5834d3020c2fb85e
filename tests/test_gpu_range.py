"""ind_range on the MI355X: ProxIndRange (two CSR products around the blocked Cholesky solve of prost_amd/csrc/kernels_prox_range.hip)
behind prost.function.ind_range, through prost.eval_prox and through the solvers.

Reference everywhere: tests/range_reference.py (NumPy / SciPy in fp64), never the code under test.
  * exact family: equality, bit for bit, in both precisions (small integers throughout: see range_reference.py);
  * tolerance family: relative inf-norm distance to the fp64 truth at most max(4 e_T, 32 eps_T), e_T being the error of LAPACK's
    potrf / potrs pipeline in precision T on the same inputs, computed here.  The measured ratios are in docs/rounds/r12.md.
Sizes come from prost_hip_range_potrs_plan: n in {1, 2, NB - 1, NB, NB + 1, 2 NB + 1}, the last n of the small tier, the first n of the
large one, and a large-tier n with more block steps that is no multiple of NB; m = n and m about 1.2 n.

Solves: min_u 1/2 |u - f|^2 + ind_range(u) with K = identity has the closed form u = P f.  The distance reached after a fixed number of
iterations was measured once per case (docs/rounds/r12.md) and ten times that value is asserted (SOLVE_DISTANCE below).
"""
import ctypes as C
import functools

import numpy as np
import pytest

import prost_amd as prost
import range_reference as rr
from prost_amd import _hip

pytestmark = pytest.mark.gpu

PRECISIONS = [("single", np.float32), ("double", np.float64)]


@pytest.fixture(autouse=True)
def _gpu(hip):
    prost.set_gpu(0)
    yield
    prost.set_precision("double")


def plan(n, dtype):
    """-> (tier, NB, launches per solve)"""
    L = _hip.lib()
    L.prost_hip_range_potrs_plan.argtypes = [C.c_size_t, C.c_int] + [C.POINTER(C.c_int)] * 3 + [C.POINTER(C.c_size_t)] * 2
    L.prost_hip_range_potrs_plan.restype = C.c_int
    tier, nb, launches = C.c_int(0), C.c_int(0), C.c_int(0)
    assert L.prost_hip_range_potrs_plan(n, 0 if dtype == np.float32 else 1, C.byref(tier), C.byref(nb), C.byref(launches), None, None) == 0
    return tier.value, nb.value, launches.value


@functools.lru_cache(maxsize=None)
def sizes(precision):
    dtype = dict(PRECISIONS)[precision]
    nb = plan(1, dtype)[1]
    lo, hi = 1, 46340                                        # the tier is monotone in n (tests/test_range_frontend.py): bisect its boundary
    assert plan(lo, dtype)[0] == 1 and plan(hi, dtype)[0] == 2
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if plan(mid, dtype)[0] == 1:
            lo = mid
        else:
            hi = mid
    more = hi + nb + 7                                       # further block steps in the large tier ...
    if more % nb == 0:
        more += 1                                            # ... at an n that is no multiple of NB
    assert plan(more, dtype)[2] >= 2 * 3
    return sorted({1, 2, nb - 1, nb, nb + 1, 2 * nb + 1, lo, hi, more})


def shapes(precision):
    out = []
    for n in sizes(precision):
        out.append((n, n))
        out.append((n, n + max(1, int(round(0.2 * n)))))
    return out


def density_of(n):
    return min(0.2, 8.0 / n)


def rounded(a, dtype):
    return np.asarray(a, dtype=np.float64).astype(dtype).astype(np.float64)


def gpu_prox(fun, y, tau=1.0, Tau=None):
    res, _ = prost.eval_prox(fun, y, tau, np.ones(y.size) if Tau is None else Tau)
    return np.asarray(res, dtype=np.float64).ravel()


# the plan decides the sizes, per precision: nine of them (sizes above), each with m = n and m about 1.2 n.  The cases are numbered, so
# nothing but the count is fixed at collection; a plan whose sizes coincide fails the tests below, it does not break collection.
SHAPE_INDEX = list(range(18))
NAMED_TOLERANCE_SHAPES = [(250, 500, 0.1), (96, 200, 0.2)]       # the shape of the reference's test_prox_ind_range.m, and the one the solves use


# ---- 1. the two families ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SHAPE_INDEX)
@pytest.mark.parametrize("precision,dtype", PRECISIONS)
def test_exact_family_bit_for_bit(case, precision, dtype):
    prost.set_precision(precision)
    assert len(shapes(precision)) == len(SHAPE_INDEX), sizes(precision)
    n, m = shapes(precision)[case]
    A, AA, y, want = rr.exact_family(n, m)
    got = gpu_prox(prost.function.ind_range(A, AA), y)
    assert np.array_equal(got, want), (n, m, int((got != want).sum()), float(np.abs(got - want).max()))


@pytest.mark.parametrize("case", SHAPE_INDEX + [len(SHAPE_INDEX), len(SHAPE_INDEX) + 1])
@pytest.mark.parametrize("precision,dtype", PRECISIONS)
def test_tolerance_family_against_the_lapack_yardstick(case, precision, dtype):
    prost.set_precision(precision)
    if case < len(SHAPE_INDEX):
        assert len(shapes(precision)) == len(SHAPE_INDEX), sizes(precision)
        n, m = shapes(precision)[case]
        density = density_of(n)
    else:
        n, m, density = NAMED_TOLERANCE_SHAPES[case - len(SHAPE_INDEX)]
    A, AA, y, want, e_t, bound = rr.tolerance_case(n, m, density, np.dtype(dtype).name)
    err = rr.rel_inf(gpu_prox(prost.function.ind_range(A, AA), y), want)
    print("tolerance n %d m %d %s: error %.3g, e_T %.3g, ratio %s, bound %.3g" % (n, m, precision, err, e_t, "%.2f" % (err / e_t) if e_t > 0 else "-", bound))
    assert err <= bound, (err, e_t, bound)


# ---- 2. identities ------------------------------------------------------------------------------------------------------------
def identity_shapes(precision):
    s = sizes(precision)
    nb = plan(1, dict(PRECISIONS)[precision])[1]
    return [(2 * nb + 1, 2 * nb + 1 + 26), (s[-1], s[-1] + s[-1] // 5)]          # one per tier


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("precision,dtype", PRECISIONS)
def test_identities(which, precision, dtype):
    prost.set_precision(precision)
    n, m = identity_shapes(precision)[which]
    A, AA, y, want, e_t, bound = rr.tolerance_case(n, m, density_of(n), np.dtype(dtype).name)
    eps = float(np.finfo(dtype).eps)
    fun = prost.function.ind_range(A, AA)
    rng = np.random.default_rng(11)
    plain = gpu_prox(fun, y)
    assert rr.rel_inf(plain, want) <= bound
    # a repeated call repeats its bits; the step does not enter: tau and Tau varied give the same bits
    assert np.array_equal(gpu_prox(fun, y), plain)
    assert np.array_equal(gpu_prox(fun, y, 0.37, rounded(rng.uniform(0.5, 2.0, m), dtype)), plain)
    assert np.array_equal(gpu_prox(fun, y, 5.0, np.full(m, 0.25)), plain)
    # idempotence: P (P y) = P y within the bound of the case
    again = gpu_prox(fun, plain)
    idem = rr.rel_inf(again, plain)
    print("idempotence n %d m %d %s: %.3g (bound %.3g)" % (n, m, precision, idem, bound))
    assert idem <= bound
    scale_p, scale_y = float(np.abs(want).max()), float(np.abs(y).max())
    # conjugate: the Moreau wrap gives y - tau P (y / tau) = y - P y.  With tau = 1 the scalings are exact, so the error is that of P y (bound * max |P y|)
    # plus one rounding of the difference
    conj = gpu_prox(prost.function.conjugate(fun), y)
    err = float(np.abs(conj - (y - want)).max())
    print("conjugate n %d m %d %s: %.3g" % (n, m, precision, err))
    assert err <= bound * scale_p + 2 * eps * scale_y
    # permute: res[perm] = P (arg[perm]) -- data movement only, so the bits of the plain evaluation at the permuted argument
    perm = rng.permutation(m)
    got = gpu_prox(prost.function.permute(fun, perm), y)
    assert np.array_equal(got[perm], gpu_prox(fun, rounded(y[perm], dtype)))
    # transform: h(x) = c f(a x - b) + d x + e / 2 x^2 -> prox_h(y) = (P (a (y - tau d) / (1 + tau e) - b) + b) / a for an indicator f.
    # Error: that of P at the inner argument (bound * max |P inner|), plus P applied to the roundings of the inner argument (at most 4 of them
    # and the rounding of b; P has 2-norm 1, so the inf-norm of P delta is at most sqrt(m) |delta|_inf), two roundings after it, all divided by |a|
    a, b, c, d, e, tau = 2.0, 0.5, 1.0, 0.25, 0.5, 0.75
    inner = a * (y - tau * d) / (1 + tau * e) - b
    want_t = (rr.truth(A, AA, inner) + b) / a
    got_t = gpu_prox(prost.function.transform(fun, a, b, c, d, e), y, tau)
    err_t = float(np.abs(got_t - want_t).max())
    scale_i = float(np.abs(inner).max())
    print("transform n %d m %d %s: %.3g" % (n, m, precision, err_t))
    assert err_t <= (bound * float(np.abs(want_t * a - b).max()) + 8 * eps * np.sqrt(m) * (scale_i + abs(b))) / a


@pytest.mark.parametrize("precision,dtype", PRECISIONS)
def test_indefinite_matrix_raises_and_leaves_the_process_usable(precision, dtype):
    prost.set_precision(precision)
    nb = plan(1, dtype)[1]
    n, m = nb + 1, nb + 14
    A, AA, y, want = rr.exact_family(n, m)
    bad = AA.copy()
    bad[nb, nb] = -1.0                                       # the first pivot of the second block column
    with pytest.raises(prost.ProstError, match=r"ProxIndRange: matrix 'AA' is not positive definite \(pivot %d\)\." % nb):
        gpu_prox(prost.function.ind_range(A, bad), y)
    bad = AA.copy()
    bad[3, 3] = np.nan
    with pytest.raises(prost.ProstError, match=r"not positive definite \(pivot 3\)"):
        gpu_prox(prost.function.ind_range(A, bad), y)
    assert np.array_equal(gpu_prox(prost.function.ind_range(A, AA), y), want)      # a host exception, not a device fault


# ---- 2b. the two tiers through the C ABI --------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision,dtype", PRECISIONS)
def test_both_tiers_give_the_same_bits(precision, dtype):
    """prost_hip_range_potrs_* with tier = 1 and tier = 2 forced at sizes of the small tier (one block, an odd number of blocks with a
    short last one, the last n of the plan's small tier, the first of its large tier, the last n the small tier's LDS holds): both form four partial sums of 16 columns per row and add them in the same order, so
    the bits agree; tier = 0 is the plan's choice; the small tier refuses an n above its bound"""
    from prost_amd._hip import DeviceArray, check, fn, sz
    L = _hip.lib()
    for name in ("prost_hip_range_dinv_elements", "prost_hip_range_potrf_workspace_bytes_f32", "prost_hip_range_potrf_workspace_bytes_f64",
                 "prost_hip_range_potrs_workspace_bytes_f32", "prost_hip_range_potrs_workspace_bytes_f64"):
        getattr(L, name).argtypes = [C.c_size_t]
        getattr(L, name).restype = C.c_size_t
    s = _hip.suffix(dtype)
    nb, last_small = plan(1, dtype)[1], sizes(precision)[-3]
    lds = C.c_size_t(0)
    assert L.prost_hip_range_potrs_plan(1, 0 if dtype == np.float32 else 1, None, None, None, C.byref(lds), None) == 0
    most = lds.value // (2 * np.dtype(dtype).itemsize)           # the small tier's LDS: the padded vector and as many partial sums
    assert last_small <= most
    for n in (nb - 1, 2 * nb + 1, last_small, last_small + 1, most, most + 1):
        A, AA, y, want, e_t, bound = rr.tolerance_case(n, n + n // 5 + 1, density_of(n), np.dtype(dtype).name)
        t = rounded(A.T @ y, dtype)
        d_L, d_U = DeviceArray.from_host(AA.ravel(order="F"), dtype), DeviceArray.zeros(n * n, dtype)
        d_dinv = DeviceArray.zeros(L.prost_hip_range_dinv_elements(n), dtype)
        ws_f = DeviceArray.zeros(getattr(L, "prost_hip_range_potrf_workspace_bytes_" + s)(n), np.uint8)
        ws_s = DeviceArray.zeros(max(16, getattr(L, "prost_hip_range_potrs_workspace_bytes_" + s)(n)), np.uint8)
        status = DeviceArray.zeros(1, np.int32)
        check(fn("range_potrf", dtype)(d_L.ptr, d_U.ptr, d_dinv.ptr, ws_f.ptr, status.ptr, sz(n), None))
        assert status.to_host()[0] == -1
        out = {}
        for tier in (0, 1, 2):
            d_t = DeviceArray.from_host(t, dtype)
            rc = fn("range_potrs", dtype)(d_t.ptr, d_L.ptr, d_U.ptr, d_dinv.ptr, ws_s.ptr, sz(n), tier, None)
            if tier == 1 and n > most:
                assert rc != 0 and b"too large for the small tier" in L.prost_hip_last_error()
                continue
            check(rc)
            out[tier] = d_t.to_host()
        assert np.array_equal(out[0], out[2])
        if n <= most:
            assert np.array_equal(out[0], out[1]) and np.array_equal(out[1], out[2]), n
        z = np.linalg.solve(AA, t)
        assert rr.rel_inf(A @ out[2].astype(np.float64), A @ z) <= bound, n


# ---- 3. solves ------------------------------------------------------------------------------------------------------------------
# relative inf-norm distance to the closed form after the fixed iteration count, measured once on an MI355X; ten times it is asserted
SOLVE_ITERS = {"pdhg": 1000, "admm": 300}
SOLVE_DISTANCE = {
    ("alg2", "single"): 3.74e-05,
    ("alg2", "double"): 4.01e-06,
    ("boyd", "single"): 2.14e-07,
    ("boyd", "double"): 8.92e-16,
    ("admm", "double"): 1.11e-15,
}


def _solve_problem(dtype, primal_side, exact=None):
    """u0 (37 values: an odd length, so the operand of ind_range starts 4 (fp32) / 8 (fp64) bytes behind a 16-byte boundary) and u (200
    values, the (200, 96) matrix of the tolerance family), K = identity.  primal_side: g = ind_range on u itself and f* the conjugate of
    the quadratic; otherwise g the quadratic and f* = conjugate(ind_range), the Moreau wrap"""
    rng = np.random.default_rng(43)
    F0 = rounded(rng.standard_normal(37) * 3, dtype)
    if exact is None:
        A, AA, _, _, _, _ = rr.tolerance_case(96, 200, 0.2, np.dtype(dtype).name)
        F = rounded(rng.standard_normal(200) * 3, dtype)
    else:
        A, AA, F, _ = exact
    fun = prost.function.ind_range(A, AA)
    u0, u, q0, q = prost.variable(37), prost.variable(200), prost.variable(37), prost.variable(200)
    prob = prost.min_max_problem([u0, u], [q0, q])
    quad0, quad = prost.function.sum_1d("square", 1, F0, 1), prost.function.sum_1d("square", 1, F, 1)
    if primal_side:
        prob.add_function(u0, prost.function.sum_1d("abs"))
        prob.add_function(u, fun)
        prob.add_function(q0, prost.function.conjugate(quad0))
        prob.add_function(q, prost.function.conjugate(quad))
    else:
        prob.add_function(u0, quad0)
        prob.add_function(u, quad)
        prob.add_function(q0, prost.function.conjugate(prost.function.sum_1d("abs")))
        prob.add_function(q, prost.function.conjugate(fun))
    prob.add_dual_pair(u0, q0, prost.block.identity())
    prob.add_dual_pair(u, q, prost.block.identity())
    want0 = np.sign(F0) * np.maximum(np.abs(F0) - 1, 0)
    return prob, np.concatenate([want0, rr.truth(A, AA, F)])


@pytest.mark.parametrize("backend_name,precision", sorted(SOLVE_DISTANCE))
def test_solves_reach_the_closed_form(backend_name, precision):
    dtype = dict(PRECISIONS)[precision]
    prost.set_precision(precision)
    prob, want = _solve_problem(dtype, primal_side=backend_name == "boyd")
    backend = {"alg2": prost.backend.pdhg(stepsize="alg2", residual_iter=10, alg2_gamma=0.5), "boyd": prost.backend.pdhg(),
               "admm": prost.backend.admm(rho0=1, residual_iter=4)}[backend_name]
    k = SOLVE_ITERS["admm" if backend_name == "admm" else "pdhg"]
    o = prost.options(max_iters=k, num_cback_calls=0, verbose=False, tol_rel_primal=0, tol_rel_dual=0, tol_abs_primal=0, tol_abs_dual=0)
    s = prost.Solver(prob, backend, o)
    s.iterate(k)
    st = s.state()
    s.destroy()
    if backend_name != "admm":
        assert st["path"] == "pdhg:generic", st["path"]
    rel = float(np.abs(st["x"].astype(np.float64).ravel() - want).max()) / float(np.abs(want).max())
    print("solve %s %s: relative distance %.3g after %d iterations" % (backend_name, precision, rel, k))
    assert rel <= 10 * SOLVE_DISTANCE[(backend_name, precision)], rel


@pytest.mark.parametrize("stepsize", ["alg1", "goldstein"])
def test_the_other_step_size_rules_run_it(stepsize):
    """alg1 and goldstein (alg2 and boyd are above): the prox takes no step, so every rule reaches the same fixed point; 1000 iterations
    stay within 1e-3 of the closed form (alg1 has no acceleration: the bound is that of a run that works, not a measured distance)"""
    prost.set_precision("double")
    prob, want = _solve_problem(np.float64, primal_side=True)
    o = prost.options(max_iters=1000, num_cback_calls=0, verbose=False, tol_rel_primal=0, tol_rel_dual=0, tol_abs_primal=0, tol_abs_dual=0)
    s = prost.Solver(prob, prost.backend.pdhg(stepsize=stepsize), o)
    s.iterate(1000)
    st = s.state()
    s.destroy()
    assert st["path"] == "pdhg:generic", st["path"]
    rel = float(np.abs(st["x"].ravel() - want).max()) / float(np.abs(want).max())
    print("solve %s double: relative distance %.3g" % (stepsize, rel))
    assert rel <= 1e-3, rel


@pytest.mark.parametrize("precision,dtype", PRECISIONS)
def test_operand_behind_an_odd_length_variable(precision, dtype):
    """the launch edge eval_prox cannot reach (it evaluates one prox at index 0 and refuses any other size): ind_range on the second
    sub-variable, 37 values into the variable, so the argument of A'y and the result of A z start 4 (fp32) / 8 (fp64) bytes behind a
    16-byte boundary.  The prox is applied to what the iteration hands it; at the fixed point of min_u 1/2 |u - f|^2 + ind_range(u) that
    is the closed form P f, so the bound of the tolerance family at this matrix, max(4 e_T, 32 eps_T), is asserted on the solution
    (boyd, ind_range on the primal variable, 1000 iterations).  The exact family likewise: f integer, P f = f on the occupied rows and 0
    elsewhere; the iteration is not exact arithmetic, so the same relative bound is asserted there, not equality."""
    prost.set_precision(precision)
    o = prost.options(max_iters=1000, num_cback_calls=0, verbose=False, tol_rel_primal=0, tol_rel_dual=0, tol_abs_primal=0, tol_abs_dual=0)
    _, _, _, _, e_t, bound = rr.tolerance_case(96, 200, 0.2, np.dtype(dtype).name)
    A, AA, y, want = rr.exact_family(96, 200)
    for label, (prob, target) in (("tolerance", _solve_problem(dtype, True)), ("exact", _solve_problem(dtype, True, exact=(A, AA, y, want)))):
        s = prost.Solver(prob, prost.backend.pdhg(), o)
        s.iterate(1000)
        st = s.state()
        s.destroy()
        assert st["path"] == "pdhg:generic", st["path"]
        got = st["x"].astype(np.float64).ravel()
        rel = rr.rel_inf(got[37:], target[37:])
        print("offset 37 %s %s: relative distance %.3g (bound %.3g)" % (label, precision, rel, bound))
        assert rel <= bound, (label, rel, bound)
