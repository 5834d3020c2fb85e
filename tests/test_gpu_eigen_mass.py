"""eigen_nxn, the mass norm and the comass ball on the MI355X: elem_operation:eigen_nxn:*, elem_operation:mass4 / mass5 /
ind_comass4_ball / ind_comass5_ball (prost_amd/csrc/kernels_prox_spectral.hip: one group per lane, n <= 5 and the mass operations;
kernels_prox_eigen_nxn.hip: several lanes per matrix, n >= 6) behind prost.function.sum_eigen_nxn / sum_mass_norm / sum_ind_comass_ball.

Reference everywhere: the fp64 NumPy compositions of tests/spectral_reference.py (np.linalg.eigh, the CPU oracle's pinned sum_1d) and
tests/mass_reference.py (np.linalg.svd), never the code under test.  Bound: inf-norm <= 1e-4, the pass mark of the reference's own
test_prox_sum_eigen_nxn.m, for fp32 and fp64 alike (the decompositions run in fp64 for both).  Inputs are rounded to the data type
first.  The functions with a discontinuous prox leave out the groups the COMPOSITION marks; at most 0.5 % of the groups may be marked.

Solves: min_u 1/2 |u - F|^2 + h(u) with K = identity has the closed form u = prox_h(F).  The distance reached after a fixed number
of iterations was measured once per case (docs/rounds/r11.md) and ten times that value is asserted (SOLVE_DISTANCE below).
"""
import ctypes as C
import functools

import numpy as np
import pytest

import mass_reference as mref
import prost_amd as prost
import spectral_reference as ref
from prost_amd import _hip

pytestmark = pytest.mark.gpu

PRECISIONS = [("single", np.float32), ("double", np.float64)]
GROUPS = {1: 3001, 2: 3001, 3: 3001, 4: 3001, 5: 3001, 6: 3001, 7: 3001, 8: 3001, 13: 1201, 16: 1201, 31: 601, 32: 601}
MASS = {"mass4": (4, False), "ind_comass4_ball": (4, True), "mass5": (5, False), "ind_comass5_ball": (5, True)}


@pytest.fixture(autouse=True)
def _gpu(hip):
    prost.set_gpu(0)
    yield
    prost.set_precision("double")


def rounded(a, dtype):
    return np.asarray(a, dtype=np.float64).astype(dtype).astype(np.float64)


def inputs(rng, G, dim, dtype, per_group_coeffs):
    """the input scheme of tests/test_gpu_spectral.py"""
    vec = rounded(rng.standard_normal((G, dim)) * 10, dtype)
    tau_group = rounded(rng.uniform(0.5, 1.5, G), dtype)
    if per_group_coeffs:
        coeffs = [rounded(rng.uniform(0.5, 2.0, G), dtype), rounded(rng.uniform(-1, 1, G), dtype), rounded(rng.uniform(0.5, 2.0, G), dtype),
                  rounded(rng.uniform(-1, 1, G), dtype), rounded(rng.uniform(0, 1, G), dtype), 0.5, 1.0]
    else:
        coeffs = [1.0, 0.0, 1.0, 0.0, 0.0, 0.5, 1.0]
    return vec, tau_group, coeffs


def step_of(tau, tau_group, dtype, cost=1.0):
    return ((dtype(tau) * np.asarray(cost, dtype=dtype)) * tau_group.astype(dtype)).astype(np.float64)


def gpu_prox(fun, vec, interleaved, tau, tau_group):
    G, dim = vec.shape
    td = np.repeat(tau_group[:, None], dim, axis=1)
    res, _ = prost.eval_prox(fun, ref.flat_from_groups(vec, interleaved), tau, ref.flat_from_groups(td, interleaved))
    return ref.groups_from_flat(res, dim, interleaved)


def mass_builder(name, interleaved, cost=1):
    n, conj = MASS[name]
    return prost.function.sum_ind_comass_ball(n, interleaved) if conj else prost.function.sum_mass_norm(n, interleaved, cost)


def plan(n, dtype):
    L = _hip.lib()
    L.prost_hip_prox_eigen_nxn_plan.argtypes = [C.c_size_t, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_size_t)]
    L.prost_hip_prox_eigen_nxn_plan.restype = C.c_int
    lanes, mats, lds = C.c_int(0), C.c_int(0), C.c_size_t(0)
    assert L.prost_hip_prox_eigen_nxn_plan(n, 0 if dtype == np.float32 else 1, C.byref(lanes), C.byref(mats), C.byref(lds)) == 0
    return lanes.value, mats.value, lds.value


# ---- 1. parity ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def eigen_cases(n, precision):
    """inputs and composition of every function at this n, computed once and shared by both layouts"""
    dtype = dict(PRECISIONS)[precision]
    rng = np.random.default_rng(5)
    tau, out = 1.25, []
    for k, fn in enumerate(ref.FUNCTIONS_1D):
        vec, tau_group, coeffs = inputs(rng, GROUPS[n], n * n, dtype, k % 2 == 0)
        want, mark = ref.compose_eigen(vec, n, fn, step_of(tau, tau_group, dtype), coeffs)
        for a in (vec, tau_group, want, mark):
            a.setflags(write=False)
        out.append((fn, vec, tau_group, coeffs, want, mark))
    return tau, out


@pytest.mark.parametrize("n", sorted(GROUPS))
@pytest.mark.parametrize("interleaved", [False, True])
@pytest.mark.parametrize("precision,dtype", PRECISIONS)
def test_eigen_nxn_parity_sweep(n, interleaved, precision, dtype):
    """every function; scalar and per-group coefficients alternate; tau_diag varies per group; group counts that are no multiple of the
    matrices per workgroup"""
    prost.set_precision(precision)
    tau, cases = eigen_cases(n, precision)
    for fn, vec, tau_group, coeffs, want, mark in cases:
        got = gpu_prox(prost.function.sum_eigen_nxn(n, interleaved, fn, *coeffs), vec, interleaved, tau, tau_group)
        share, err = float(mark.mean()), float(np.abs(got - want)[~mark].max())
        print("eigen_nxn n %d %s %s il=%d: inf-norm %.3g, marked %d of %d" % (n, fn, precision, interleaved, err, int(mark.sum()), mark.size))
        assert share <= 0.005, (fn, share)
        assert err <= 1e-4, (fn, err)


@pytest.mark.parametrize("name", sorted(MASS))
@pytest.mark.parametrize("interleaved", [False, True])
@pytest.mark.parametrize("precision,dtype", PRECISIONS)
def test_mass_parity(name, interleaved, precision, dtype):
    """3001 groups at scales 10 / 1 / 0.3 with the special rows, a per-group cost for mass4, a scalar cost for mass5 (the extension)"""
    prost.set_precision(precision)
    n, conj = MASS[name]
    rng = np.random.default_rng(9)
    G, tau = 3001, 0.75
    for scale in (10.0, 1.0, 0.3):
        vec, special = mref.mass_inputs(rng, G, n, scale, lambda a: rounded(a, dtype))
        tau_group = rounded(rng.uniform(0.5, 1.5, G), dtype)
        cost = rounded(rng.uniform(0.5, 1.5, G), dtype) if name == "mass4" else 0.75 if name == "mass5" else 1.0
        got = gpu_prox(mass_builder(name, interleaved, cost), vec, interleaved, tau, tau_group)
        want = mref.compose_mass(vec, n, conj, step_of(tau, tau_group, dtype, cost))
        err = np.abs(got - want).max(axis=1)
        print("%s scale %g %s il=%d: inf-norm %.3g" % (name, scale, precision, interleaved, err.max()))
        for row, what in enumerate(special):
            assert err[row] <= 1e-4, (what, err[row])
        assert np.array_equal(got[0], np.zeros(mref.DIM[n]))
        assert err.max() <= 1e-4, (scale, err.max())


# ---- 2. launch edges ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [5, 6, 8, 9, 17, 32])
@pytest.mark.parametrize("precision,dtype", PRECISIONS)
def test_eigen_nxn_launch_edges(n, precision, dtype):
    """group counts 1, M - 1, M, M + 1, 3 M + 1 around the matrices per workgroup M of the launch plan, both layouts, continuous
    functions (abs; ind_leq0 with a = -1: the projection onto the PSD cone)"""
    prost.set_precision(precision)
    lanes, M, lds = plan(n, dtype)
    assert lanes * M == 256 and lds <= 65536
    rng = np.random.default_rng(100 + n)
    tau = 0.9
    for G in sorted({1, M - 1, M, M + 1, 3 * M + 1}):
        vec, tau_group, _ = inputs(rng, G, n * n, dtype, False)
        for fn, co in (("abs", [1.0, 0.25, 1.5, 0, 0, 0, 0]), ("ind_leq0", [-1.0, 0, 1.0, 0, 0, 0, 0])):
            want, _ = ref.compose_eigen(vec, n, fn, step_of(tau, tau_group, dtype), co)
            for il in (False, True):
                got = gpu_prox(prost.function.sum_eigen_nxn(n, il, fn, *co), vec, il, tau, tau_group)
                err = float(np.abs(got - want).max())
                assert err <= 1e-4, (n, G, fn, il, err)


@pytest.mark.parametrize("precision,dtype", PRECISIONS)
def test_register_path_tail_at_100003_groups(precision, dtype):
    prost.set_precision(precision)
    rng = np.random.default_rng(11)
    G, tau = 100003, 0.75
    vec, tau_group, coeffs = inputs(rng, G, 16, dtype, True)
    want, _ = ref.compose_eigen(vec, 4, "abs", step_of(tau, tau_group, dtype), coeffs)
    mvec = rounded(rng.standard_normal((G, 10)) * 10, dtype)
    mwant = mref.compose_mass(mvec, 5, False, step_of(tau, tau_group, dtype))
    for il in (False, True):
        got = gpu_prox(prost.function.sum_eigen_nxn(4, il, "abs", *coeffs), vec, il, tau, tau_group)
        assert float(np.abs(got - want).max()) <= 1e-4, il
        got = gpu_prox(prost.function.sum_mass_norm(5, il), mvec, il, tau, tau_group)
        assert float(np.abs(got - mwant).max()) <= 1e-4, il


# ---- 3. the reference's own test, restated ----------------------------------------------------------------------------------
@pytest.mark.parametrize("precision,dtype", PRECISIONS)
def test_30000_5x5_matrices_onto_the_psd_cone(precision, dtype):
    """test_prox_sum_eigen_nxn.m: interleaved, ind_leq0 with a = -ones(N), against V max(L, 0) V^T; every result is positive semidefinite"""
    prost.set_precision(precision)
    rng = np.random.default_rng(30000)
    N, n = 30000, 5
    vec = rounded(rng.standard_normal((N, n * n)) * 10, dtype)
    got = gpu_prox(prost.function.sum_eigen_nxn(n, True, "ind_leq0", -np.ones(N), 0, 1, 0, 0), vec, True, 1.0, np.ones(N))
    M = vec.reshape(N, n, n)
    w, V = np.linalg.eigh((M + M.transpose(0, 2, 1)) / 2)
    psd = np.einsum("gij,gj,gkj->gik", V, np.maximum(w, 0), V).reshape(N, n * n)
    assert float(np.abs(got - psd).max()) <= 1e-4
    assert float(np.linalg.eigvalsh(got.reshape(N, n, n)).min()) >= -1e-4


# ---- 4. identities ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision,dtype", PRECISIONS)
def test_eigen_nxn_identities(precision, dtype):
    prost.set_precision(precision)
    rng = np.random.default_rng(17)
    G, tau = 2051, 0.9
    tau_group = rounded(rng.uniform(0.5, 1.5, G), dtype)
    co = [1.25, 0.5, 0.75, 0.1, 0.2, 0, 0]
    # n = 2, 3 against the operations of their own on the same operands
    for n, make in ((2, prost.function.sum_eigen_2x2), (3, prost.function.sum_eigen_3x3)):
        vec = rounded(rng.standard_normal((G, n * n)) * 10, dtype)
        for il in (False, True):
            a = gpu_prox(prost.function.sum_eigen_nxn(n, il, "abs", *co), vec, il, tau, tau_group)
            b = gpu_prox(make(il, "abs", *co), vec, il, tau, tau_group)
            assert float(np.abs(a - b).max()) <= 1e-4, (n, il)
    # diagonal matrices: sum_1d on the diagonal, nothing next to it
    for n in (4, 7, 16):
        diag = rounded(rng.standard_normal((G, n)) * 10, dtype)
        vec = np.zeros((G, n * n))
        vec[:, ::n + 1] = diag
        got = gpu_prox(prost.function.sum_eigen_nxn(n, True, "abs", *co), vec, True, tau, tau_group)
        want = ref.scalar_prox("abs", diag, step_of(tau, tau_group, dtype), co)
        off = np.ones(n * n, dtype=bool)
        off[::n + 1] = False
        assert float(np.abs(got[:, ::n + 1] - want).max()) <= 1e-4 and float(np.abs(got[:, off]).max()) <= 1e-4, n
    # permute with the identity permutation and transform with the identity coefficients leave the prox unchanged
    for n in (5, 8):
        vec = rounded(rng.standard_normal((G, n * n)) * 10, dtype)
        fun = prost.function.sum_eigen_nxn(n, False, "huber", *[1.0, 0.0, 1.0, 0.0, 0.0, 0.5, 0.0])
        plain = gpu_prox(fun, vec, False, tau, tau_group)
        assert np.array_equal(gpu_prox(prost.function.permute(fun, np.arange(G * n * n)), vec, False, tau, tau_group), plain)
        assert float(np.abs(gpu_prox(prost.function.transform(fun, 1, 0, 1, 0, 0), vec, False, tau, tau_group) - plain).max()) <= 1e-4


@pytest.mark.parametrize("n", [4, 5])
@pytest.mark.parametrize("precision,dtype", PRECISIONS)
def test_mass_identities(n, precision, dtype):
    prost.set_precision(precision)
    rng = np.random.default_rng(23 + n)
    G, tau, dim = 2051, 0.8, mref.DIM[n]
    tau_group = rounded(rng.uniform(0.5, 1.5, G), dtype)
    step = step_of(tau, tau_group, dtype)
    vec = rounded(rng.standard_normal((G, dim)) * 3, dtype)
    for il in (False, True):
        # Moreau: the conjugate of the mass norm is the indicator of the comass ball, at any step
        a = gpu_prox(prost.function.conjugate(prost.function.sum_mass_norm(n, il)), vec, il, tau, tau_group)
        b = gpu_prox(prost.function.sum_ind_comass_ball(n, il), vec, il, tau, tau_group)
        assert float(np.abs(a - b).max()) <= 1e-4, il
        # a simple 2-vector e_1 ^ v has sigma_2 = 0: the mass norm is the Euclidean norm of the group
        simple = np.zeros((G, dim))
        simple[:, :n - 1] = vec[:, :n - 1]
        a = gpu_prox(prost.function.sum_mass_norm(n, il), simple, il, tau, tau_group)
        b = gpu_prox(prost.function.sum_norm2(dim, il, "abs"), simple, il, tau, tau_group)
        nrm = np.linalg.norm(simple, axis=1)
        want = simple * (np.maximum(nrm - step, 0) / nrm)[:, None]
        assert float(np.abs(a - b).max()) <= 1e-4 and float(np.abs(a - want).max()) <= 1e-4, il
        fun = prost.function.sum_mass_norm(n, il, 0.7)
        plain = gpu_prox(fun, vec, il, tau, tau_group)
        assert np.array_equal(gpu_prox(prost.function.permute(fun, np.arange(G * dim)), vec, il, tau, tau_group), plain)
        assert float(np.abs(gpu_prox(prost.function.transform(fun, 1, 0, 1, 0, 0), vec, il, tau, tau_group) - plain).max()) <= 1e-4


# ---- 5. solves --------------------------------------------------------------------------------------------------------------
# relative inf-norm distance to the closed form after the fixed iteration count, measured once on an MI355X; ten times it is asserted
SOLVE_ITERS = {"pdhg": 1000, "admm": 300}
SOLVE_DISTANCE = {
    ("psd6", "alg2", "single"): 4.13e-06,
    ("mass5", "alg2", "single"): 9.09e-06,
    ("psd6", "alg2", "double"): 4.01e-06,
    ("mass5", "alg2", "double"): 8.43e-06,
    ("psd6", "boyd", "single"): 6.14e-08,
    ("mass5", "boyd", "single"): 1.34e-07,
    ("psd6", "boyd", "double"): 1.5e-15,
    ("mass5", "boyd", "double"): 2.19e-15,
    ("psd6", "admm", "double"): 1.34e-15,
    ("mass5", "admm", "double"): 2.54e-15,
}


def _solve_problem(case, dtype, primal_side):
    """u0 (37 values: an odd length, so the operand of the spectral prox starts 4 (fp32) / 8 (fp64) bytes behind a 16-byte boundary and
    the interleaved run takes the narrow branch of its copies) and u, K = identity.  primal_side: g = h on u itself and f* the conjugate
    of the quadratic (every prox reads a device-resident step: the boyd rule stays on the device); otherwise g the quadratic and f* =
    conjugate(h), the Moreau wrap around the spectral prox.  The weighted mass norm is always on the primal side: under invert_tau the
    operation forms 1 / (tau cost tau_diag) like the reference, so its Moreau wrap is the conjugate of mass / cost, not of cost * mass"""
    rng = np.random.default_rng(41)
    if case == "psd6":
        G, dim, fun = 40, 36, prost.function.sum_eigen_nxn(6, True, "ind_leq0", -1, 0, 1, 0, 0)
    elif case in ("psd4", "psd5"):                         # 300 groups: a full tile of 256 and a tail
        G, dim, fun = 300, int(case[3]) ** 2, prost.function.sum_eigen_nxn(int(case[3]), True, "ind_leq0", -1, 0, 1, 0, 0)
    else:
        G, dim, fun = 64, 10, prost.function.sum_mass_norm(5, True, 0.7)
    F0 = rounded(rng.standard_normal(37) * 3, dtype)
    F = rounded(rng.standard_normal((G, dim)) * 3, dtype)
    u0, u, q0, q = prost.variable(37), prost.variable(G * dim), prost.variable(37), prost.variable(G * dim)
    prob = prost.min_max_problem([u0, u], [q0, q])
    quad0, quad = prost.function.sum_1d("square", 1, F0, 1), prost.function.sum_1d("square", 1, F.ravel(), 1)
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
    if case.startswith("psd"):
        want, _ = ref.compose_eigen(F, int(case[3]), "ind_leq0", np.ones(G), [-1.0, 0, 1.0, 0, 0, 0, 0])
    else:
        want = mref.compose_mass(F, 5, False, np.full(G, 0.7))
    want0 = np.sign(F0) * np.maximum(np.abs(F0) - 1, 0)
    return prob, np.concatenate([want0, want.ravel()])


@pytest.mark.parametrize("case", ["psd6", "mass5"])
@pytest.mark.parametrize("backend_name,precision", [("alg2", "single"), ("alg2", "double"), ("boyd", "single"), ("boyd", "double"), ("admm", "double")])
def test_solves_reach_the_closed_form(case, backend_name, precision):
    dtype = dict(PRECISIONS)[precision]
    prost.set_precision(precision)
    prob, want = _solve_problem(case, dtype, primal_side=case == "mass5" or backend_name == "boyd")
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
    if backend_name == "boyd":
        assert st["device_rule_batches"] > 0, st["device_rule_batches"]
    rel = float(np.abs(st["x"].astype(np.float64).ravel() - want).max()) / float(np.abs(want).max())
    print("solve %s %s %s: relative distance %.3g after %d iterations" % (case, backend_name, precision, rel, k))
    assert rel <= 10 * SOLVE_DISTANCE[(case, backend_name, precision)], rel


@pytest.mark.parametrize("case", ["psd4", "psd5"])
@pytest.mark.parametrize("precision,dtype", PRECISIONS)
def test_register_tiles_at_an_operand_behind_an_odd_length_variable(case, precision, dtype):
    """the launch edge eval_prox cannot reach (it evaluates one prox at index 0): the interleaved 4 x 4 / 5 x 5 tile copies -- a rolled
    loop for these sizes -- at an operand that starts 37 values into the variable, 4 (fp32) / 8 (fp64) bytes behind a 16-byte boundary,
    300 groups (a full tile and a tail).  The prox is applied to what the iteration hands it; at the fixed point of
    min_u 1/2 |u - F|^2 + h(u) that is the closed form prox_h(F), so the parity bound of the prox, inf-norm <= 1e-4, is asserted on the
    solution (boyd, h on the primal variable, 1000 iterations: the 6 x 6 case of this construction is 6e-8 / 2e-15 away)"""
    prost.set_precision(precision)
    prob, want = _solve_problem(case, dtype, primal_side=True)
    k = SOLVE_ITERS["pdhg"]
    o = prost.options(max_iters=k, num_cback_calls=0, verbose=False, tol_rel_primal=0, tol_rel_dual=0, tol_abs_primal=0, tol_abs_dual=0)
    s = prost.Solver(prob, prost.backend.pdhg(), o)
    s.iterate(k)
    st = s.state()
    s.destroy()
    assert st["path"] == "pdhg:generic", st["path"]
    err = float(np.abs(st["x"].astype(np.float64).ravel() - want).max())
    print("%s %s behind 37 values: inf-norm %.3g" % (case, precision, err))
    assert err <= 1e-4, err
