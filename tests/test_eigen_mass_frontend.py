"""eigen_nxn, the mass norm and the comass ball without a GPU: builders, registry names, creation errors, the launch plan, the pair
schedule, and the arithmetic of the public functor headers (the functions the gfx950 kernels call) compiled for the host and compared
with an fp64 NumPy composition.

  * prost.function.sum_eigen_nxn / sum_mass_norm / sum_ind_comass_ball produce the nested lists of the .m builders (plus the cost of
    the mass norm for n = 5, which the .m builder drops);
  * the 18 names are registered for both precisions; a bad shape raises ProstError with the operation's name at prost.problem_info;
  * RoundRobinPair: the pairs of a round are disjoint and a sweep holds every unordered pair exactly once, m = 2 .. 32;
  * prost_hip_prox_eigen_nxn_plan: lanes a power of two <= 64, lanes * matrices = 256, at most 64 KiB of LDS, for every n and dtype;
  * tests/host/eigen_mass_functor_harness.cpp runs ElemOperationEigenNxN, EigenNApply<N>, ElemOperationMass4 / Mass5 on the host:
    inf-norm <= 1e-4 (the pass mark of the reference's own tests) against np.linalg.eigh / svd compositions for fp32 and fp64, with the
    exclusion rule of tests/spectral_reference.py for the discontinuous functions (at most 0.5 % of the groups);
  * NaN and Inf groups among finite ones: the run ends (child process under a time limit) and the finite groups keep the bound.
"""
import ctypes as C
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import mass_reference as mref
import prost_amd as prost
import spectral_reference as ref
from prost_amd import _hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
MASS_NAMES = ["elem_operation:mass4", "elem_operation:mass5", "elem_operation:ind_comass4_ball", "elem_operation:ind_comass5_ball"]
# group counts at which the composition marks at most 0.5 % of the groups for the discontinuous functions (seed 5, step 1.25 tau_group)
GROUPS = {1: 3001, 2: 3001, 3: 3001, 4: 3001, 5: 3001, 6: 3001, 7: 3001, 8: 3001, 13: 1201, 16: 1201, 31: 601, 32: 601}


def _same(a, b):
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return np.array_equal(np.asarray(a, dtype=np.float64).ravel(), np.asarray(b, dtype=np.float64).ravel())
    return type(a) == type(b) and a == b


def test_builders_mirror_the_m_builders():
    one = lambda v: np.array([float(v)])
    # sum_eigen_nxn.m:23-25  { strcat('elem_operation:eigen_nxn:', fun), idx, count, false, { count / dim, dim, interleaved, coeffs } }
    d = prost.function.sum_eigen_nxn(5, True, "ind_leq0", -1)(7, 75)
    assert _same(d, ["elem_operation:eigen_nxn:ind_leq0", 7, 75, False, [3, 25, True, [one(-1), one(0), one(1), one(0), one(0), one(0), one(0)]]])
    assert d[3] is False and d[4][2] is True
    b = np.arange(2.0)
    d = prost.function.sum_eigen_nxn(32, False, "huber", 1, b, 2, 0, 0, 0.25)(0, 2048)
    assert _same(d, ["elem_operation:eigen_nxn:huber", 0, 2048, False, [2, 1024, False, [one(1), b, one(2), one(0), one(0), one(0.25), one(0)]]])
    prost.function.sum_eigen_nxn(1, False, "abs")
    for n in (0, -1, 33):
        with pytest.raises(ValueError):
            prost.function.sum_eigen_nxn(n, False, "abs")
    # sum_mass_norm.m:12 / :16
    assert _same(prost.function.sum_mass_norm(4, False)(6, 60), ["elem_operation:mass4", 6, 60, False, [10, 6, False, [one(1)]]])
    cost = np.linspace(0.5, 1.5, 10)
    assert _same(prost.function.sum_mass_norm(4, True, cost)(0, 60), ["elem_operation:mass4", 0, 60, False, [10, 6, True, [cost]]])
    assert _same(prost.function.sum_mass_norm(5, True)(0, 60), ["elem_operation:mass5", 0, 60, False, [6, 10, True]])
    assert _same(prost.function.sum_mass_norm(5, True, 1)(0, 60), ["elem_operation:mass5", 0, 60, False, [6, 10, True]])
    assert _same(prost.function.sum_mass_norm(5, False, 0.7)(0, 60), ["elem_operation:mass5", 0, 60, False, [6, 10, False, [one(0.7)]]])     # the extension
    # sum_ind_comass_ball.m:9 / :13
    assert _same(prost.function.sum_ind_comass_ball(4, True)(0, 60), ["elem_operation:ind_comass4_ball", 0, 60, False, [10, 6, True]])
    assert _same(prost.function.sum_ind_comass_ball(5, False)(20, 60), ["elem_operation:ind_comass5_ball", 20, 60, False, [6, 10, False]])
    for n in (3, 6):
        with pytest.raises(ValueError, match=r"Mass norm not implemented for n \\notin \{4, 5\}"):
            prost.function.sum_mass_norm(n, False)
        with pytest.raises(ValueError, match=r"Indicator of comass norm ball not implemented for n \\notin \{4, 5\}"):
            prost.function.sum_ind_comass_ball(n, False)


@pytest.mark.parametrize("precision", ["single", "double"])
def test_the_eighteen_names_are_registered(precision):
    prost.set_precision(precision)
    try:
        reg = set(prost.registered()["prox"])
    finally:
        prost.set_precision("double")
    names = ["elem_operation:eigen_nxn:" + f for f in ref.FUNCTIONS_1D] + MASS_NAMES
    assert len(names) == 18
    assert not [n for n in names if n not in reg]


def _problem_with_dual_prox(desc, size):
    u, q = prost.variable(size // 2), prost.variable(size)
    prob = prost.min_max_problem([u], [q])
    prob.add_function(q, lambda idx, count: desc)
    prob.add_dual_pair(u, q, prost.block.gradient2d(size // 2, 1, 1))
    return prob


@pytest.mark.parametrize("precision", ["single", "double"])
def test_bad_shapes_raise_at_creation_with_the_name_of_the_operation(precision):
    prost.set_precision(precision)
    try:
        co = [np.array([1.0]), np.array([0.0]), np.array([1.0]), np.array([0.0]), np.array([0.0]), np.array([0.0]), np.array([0.0])]
        cases = [(["elem_operation:eigen_nxn:abs", 0, 60, False, [6, 10, False, co]], "eigen_nxn: dim = 10"),       # 10 is no perfect square
                 (["elem_operation:eigen_nxn:abs", 0, 2178, False, [2, 1089, False, co]], "eigen_nxn: dim = 1089"), # n = 33
                 (["elem_operation:eigen_nxn:zero", 0, 60, False, [3, 25, True, co]], "eigen_nxn: size = 60"),      # size != count * dim
                 (["elem_operation:mass4", 0, 60, False, [6, 10, False, [np.array([1.0])]]], "mass4: Wrong dimension in mass norm prox"),              # dim != 6
                 (["elem_operation:mass5", 0, 60, False, [10, 6, False]], "mass5: Wrong dimension in mass norm prox"),                                 # dim != 10
                 (["elem_operation:ind_comass4_ball", 0, 60, False, [6, 10, True]], "ind_comass4_ball: Wrong dimension in mass norm prox"),
                 (["elem_operation:ind_comass5_ball", 0, 60, False, [10, 6, True]], "ind_comass5_ball: Wrong dimension in mass norm prox"),
                 (["elem_operation:mass5", 0, 60, False, [5, 10, False]], "mass5: size = 60"),                      # size != count * dim
                 (["elem_operation:mass4", 0, 60, False, [9, 6, False, [np.array([1.0])]]], "mass4: size = 60")]
        for desc, inner in cases:                                  # `inner`: the operation's own message, not the registry ID of the wrapper's
            prob = _problem_with_dual_prox(desc, desc[2])
            with pytest.raises(prost.ProstError, match=inner) as err:
                prost.problem_info(prob)
            assert "Creating prox with ID '%s' failed" % desc[0] in str(err.value)
        good = [["elem_operation:eigen_nxn:zero", 0, 100, False, [4, 25, True, co]],
                ["elem_operation:eigen_nxn:abs", 0, 2048, False, [2, 1024, False, co]],
                ["elem_operation:mass4", 0, 60, False, [10, 6, False, [np.linspace(1, 2, 10)]]],
                ["elem_operation:mass4", 0, 60, False, [10, 6, False]],                                             # the cost cell is optional
                ["elem_operation:mass5", 0, 60, False, [6, 10, True]],
                ["elem_operation:mass5", 0, 60, False, [6, 10, True, [np.array([0.7])]]],
                ["elem_operation:ind_comass4_ball", 0, 60, False, [10, 6, True]],
                ["elem_operation:ind_comass4_ball", 0, 60, False, [10, 6, True, [np.array([1.0])]]],                # read by the reference's factory
                ["elem_operation:ind_comass5_ball", 0, 60, False, [6, 10, False]]]
        for desc in good:
            prost.problem_info(_problem_with_dual_prox(desc, desc[2]))
    finally:
        prost.set_precision("double")


def test_wrong_mass_dimension_carries_the_reference_text():
    prob = _problem_with_dual_prox(["elem_operation:mass5", 0, 60, False, [10, 6, False]], 60)
    with pytest.raises(prost.ProstError, match="Wrong dimension in mass norm prox"):
        prost.problem_info(prob)


def test_eigen_nxn_plan_for_every_n_and_dtype():
    L = _hip.lib()
    L.prost_hip_prox_eigen_nxn_plan.argtypes = [C.c_size_t, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_size_t)]
    L.prost_hip_prox_eigen_nxn_plan.restype = C.c_int
    for dtype in (0, 1):
        for n in range(1, 33):
            lanes, mats, lds = C.c_int(-1), C.c_int(-1), C.c_size_t(0)
            assert L.prost_hip_prox_eigen_nxn_plan(n, dtype, C.byref(lanes), C.byref(mats), C.byref(lds)) == 0, n
            assert 1 <= lanes.value <= 64 and lanes.value & (lanes.value - 1) == 0, (n, lanes.value)
            assert lanes.value * mats.value == 256, (n, lanes.value, mats.value)
            assert 0 < lds.value <= 65536, (n, dtype, lds.value)
        for n in (0, 33):
            assert L.prost_hip_prox_eigen_nxn_plan(n, dtype, None, None, None) != 0, n
    assert L.prost_hip_prox_eigen_nxn_plan(8, 2, None, None, None) != 0


# ---- the functor headers on the host ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("eigen_mass") / "eigen_mass_functor_harness")
    cmd = [HIPCC, "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-O2", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "host", "eigen_mass_functor_harness.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert b.returncode == 0, b.stderr[-3000:]
    return exe


def test_round_robin_pairs_are_disjoint_and_cover_every_pair_once(harness):
    out = subprocess.run([harness, "pairs"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0
    rows = np.array([[int(v) for v in line.split()] for line in out.stdout.splitlines()])
    for m in range(2, 33, 2):                                  # an odd n plays with m = n + 1: every m in 2 .. 32 is covered
        r = rows[rows[:, 0] == m]
        assert r.shape[0] == (m - 1) * (m // 2)
        assert (r[:, 3] < r[:, 4]).all() and (r[:, 3] >= 0).all() and (r[:, 4] < m).all()
        for rnd in range(m - 1):
            pq = r[r[:, 1] == rnd][:, 3:5]
            assert pq.shape[0] == m // 2 and sorted(pq.ravel().tolist()) == list(range(m)), (m, rnd)
        assert len({(p, q) for p, q in r[:, 3:5].tolist()}) == m * (m - 1) // 2, m


FAMILY = {"eigen_nxn": 0, "mass4": 1, "ind_comass4_ball": 2, "mass5": 3, "ind_comass5_ball": 4, "eigen_n": 5}


def run_functor(exe, tmp, family, fn, single, vec, interleaved, tau, tau_group, coeffs, invert_tau=False, want_sweeps=False, timeout=600):
    """vec (G, dim) groups -> result (G, dim) from the host-compiled functor [, sweeps (G,)]"""
    G, dim = vec.shape
    path_in, path_out = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    td = np.repeat(tau_group[:, None], dim, axis=1)
    with open(path_in, "wb") as f:
        f.write(struct.pack("8q", FAMILY[family], ref.FUNCTIONS_1D.index(fn) if fn in ref.FUNCTIONS_1D else 0, int(single), dim, G, int(interleaved),
                            int(invert_tau), int(want_sweeps)))
        f.write(struct.pack("d", tau))
        f.write(ref.flat_from_groups(vec, interleaved).astype(np.float64).tobytes())
        f.write(ref.flat_from_groups(td, interleaved).astype(np.float64).tobytes())
        for c in coeffs:
            f.write(ref.per_group(c, G).astype(np.float64).tobytes())
    r = subprocess.run([exe, path_in, path_out], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-2000:]
    out = np.fromfile(path_out, dtype=np.float64)
    res = ref.groups_from_flat(out[:G * dim], dim, interleaved)
    return (res, out[G * dim:]) if want_sweeps else res


def rounder(single):
    return (lambda a: np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)) if single else (lambda a: np.asarray(a, dtype=np.float64))


def inputs(rng, G, dim, single, per_group_coeffs):
    """the input scheme of tests/test_gpu_spectral.py"""
    rnd = rounder(single)
    vec = rnd(rng.standard_normal((G, dim)) * 10)
    tau_group = rnd(rng.uniform(0.5, 1.5, G))
    if per_group_coeffs:
        coeffs = [rnd(rng.uniform(0.5, 2.0, G)), rnd(rng.uniform(-1, 1, G)), rnd(rng.uniform(0.5, 2.0, G)), rnd(rng.uniform(-1, 1, G)),
                  rnd(rng.uniform(0, 1, G)), 0.5, 1.0]
    else:
        coeffs = [1.0, 0.0, 1.0, 0.0, 0.0, 0.5, 1.0]
    return vec, tau_group, coeffs


def step_of(tau, tau_group, single, cost=1.0):
    if single:
        return ((np.float32(tau) * np.asarray(cost, dtype=np.float32)) * tau_group.astype(np.float32)).astype(np.float64)
    return (tau * np.asarray(cost, dtype=np.float64)) * tau_group


def check_eigen(got, vec, n, fn, step, coeffs, what):
    want, mark = ref.compose_eigen(vec, n, fn, step, coeffs)
    share = float(mark.mean())
    err = float(np.abs(got - want)[~mark].max())
    print("%s: inf-norm %.3g, marked %d of %d" % (what, err, int(mark.sum()), mark.size))
    assert share <= 0.005, (what, share)
    assert err <= 1e-4, (what, err)


SPECIAL = ("identity", "all ones", "rank 2", "zero", "diagonal")


def special_matrices(n, rnd):
    rng = np.random.default_rng(n)
    u = rng.standard_normal((n, 2))
    return rnd(np.stack([np.eye(n).ravel() * 2, np.ones(n * n), (u @ u.T).ravel(), np.zeros(n * n), np.diag(np.arange(n) - 1.5).ravel()]))


@pytest.mark.parametrize("single", [True, False])
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 6, 7, 8, 13, 16, 31, 32])
def test_eigen_nxn_functor_equals_the_numpy_composition(harness, tmp_path, n, single):
    """ElemOperationEigenNxN (run-time n, round-robin order), all 14 functions, both layouts, scalar and per-group
    coefficients alternating; the sweeps every decomposition took stay at most half the cap (kJacobiSweepsNxN = 16)"""
    rng = np.random.default_rng(5)
    G, tau, most = GROUPS[n], 1.25, 0
    for k, fn in enumerate(ref.FUNCTIONS_1D):
        vec, tau_group, coeffs = inputs(rng, G, n * n, single, k % 2 == 0)
        for interleaved in (False, True):
            measure = k < 2 and not interleaved                  # the decomposition does not depend on the function: two inputs are measured
            got = run_functor(harness, str(tmp_path), "eigen_nxn", fn, single, vec, interleaved, tau, tau_group, coeffs, want_sweeps=measure)
            if measure:
                got, sweeps = got
                most = max(most, int(sweeps.max()))
            check_eigen(got, vec, n, fn, step_of(tau, tau_group, single), coeffs, "eigen_nxn n %d %s %s il=%d" % (n, fn, "fp32" if single else "fp64", interleaved))
    print("n %d: at most %d sweeps" % (n, most))
    assert 2 * most <= 16, (n, most)


@pytest.mark.parametrize("single", [True, False])
@pytest.mark.parametrize("n", [1, 4, 5])
def test_compile_time_eigen_form_equals_the_numpy_composition(harness, tmp_path, n, single):
    """EigenNApply<T, N>: what the register kernels run for n = 1, 4, 5 (cyclic order, SymEigN)"""
    rng = np.random.default_rng(5)
    G, tau, most = GROUPS[n], 1.25, 0
    for k, fn in enumerate(ref.FUNCTIONS_1D):
        vec, tau_group, coeffs = inputs(rng, G, n * n, single, k % 2 == 0)
        for interleaved in (False, True):
            got, sweeps = run_functor(harness, str(tmp_path), "eigen_n", fn, single, vec, interleaved, tau, tau_group, coeffs, want_sweeps=True)
            most = max(most, int(sweeps.max()))
            check_eigen(got, vec, n, fn, step_of(tau, tau_group, single), coeffs, "EigenNApply n %d %s %s il=%d" % (n, fn, "fp32" if single else "fp64", interleaved))
    print("n %d: at most %d sweeps" % (n, most))
    assert 2 * most <= 16, (n, most)


def test_eigen_nxn_special_matrices_on_their_own(harness, tmp_path):
    for n in (4, 5, 8, 13, 32):
        vec = special_matrices(n, rounder(False))
        one = np.ones(vec.shape[0])
        co = [1.0, 0, 1.0, 0, 0, 0, 0]
        for family in ("eigen_nxn",) + (("eigen_n",) if n <= 5 else ()):
            got, sweeps = run_functor(harness, str(tmp_path), family, "abs", False, vec, True, 0.5, one, co, want_sweeps=True)
            print("n %d %s: sweeps of %s = %s" % (n, family, SPECIAL, sweeps.astype(int).tolist()))
            assert 2 * int(sweeps.max()) <= 16, (n, family, sweeps)
            want, _ = ref.compose_eigen(vec, n, "abs", 0.5 * one, co)
            for row, name in enumerate(SPECIAL):
                assert np.abs(got[row] - want[row]).max() <= 1e-4, (n, family, name)
            assert np.array_equal(got[3], np.zeros(n * n)), (n, family)                    # the zero matrix stays zero under `abs`
            assert np.array_equal(got, got.reshape(-1, n, n).transpose(0, 2, 1).reshape(-1, n * n))      # both triangles written, symmetric


@pytest.mark.parametrize("single", [True, False])
@pytest.mark.parametrize("name,n,conj", [("mass4", 4, False), ("ind_comass4_ball", 4, True), ("mass5", 5, False), ("ind_comass5_ball", 5, True)])
def test_mass_functors_equal_the_svd_composition(harness, tmp_path, name, n, conj, single):
    rng = np.random.default_rng(9)
    G, tau, dim = 2003, 0.75, mref.DIM[n]
    rnd = rounder(single)
    for scale in (10.0, 1.0, 0.3):
        vec, special = mref.mass_inputs(rng, G, n, scale, rnd)
        tau_group = rnd(rng.uniform(0.5, 1.5, G))
        cost = rnd(rng.uniform(0.5, 1.5, G)) if name == "mass4" else np.ones(G)          # ElemOperationMass5 takes no coefficient
        for invert_tau, interleaved in ((False, False), (False, True), (True, False), (True, True)):
            got = run_functor(harness, str(tmp_path), name, "zero", single, vec, interleaved, tau, tau_group, [cost, 0, 0, 0, 0, 0, 0], invert_tau=invert_tau)
            step = step_of(tau, tau_group, single, cost)
            want = mref.compose_mass(vec, n, conj, 1.0 / step if invert_tau else step)
            err = np.abs(got - want).max(axis=1)
            print("%s scale %g %s invert_tau=%d: inf-norm %.3g" % (name, scale, "fp32" if single else "fp64", invert_tau, err.max()))
            for row, what in enumerate(special):
                assert err[row] <= 1e-4, (name, scale, what, err[row])
            assert np.array_equal(got[0], np.zeros(dim))                                    # a zero group gives zeros
            assert err.max() <= 1e-4, (name, scale, err.max())


def test_nan_and_inf_groups_end_and_leave_the_finite_groups_alone(harness, tmp_path):
    """one NaN and one Inf group among finite ones; the child process ends inside its time limit (every sweep loop is capped), and the
    finite groups are within the bound"""
    one = np.ones(12)
    co = [1.0, 0, 1.0, 0, 0, 0, 0]
    rng = np.random.default_rng(21)
    for n in (4, 5, 8, 32):
        vec = rng.standard_normal((12, n * n)) * 10
        vec[3, n + 1 if n > 1 else 0] = np.nan
        vec[7, 1] = np.inf
        fine = np.ones(12, dtype=bool)
        fine[[3, 7]] = False
        for family in ("eigen_nxn",) + (("eigen_n",) if n <= 5 else ()):
            for il in (False, True):
                got = run_functor(harness, str(tmp_path), family, "abs", False, vec, il, 0.5, one, co, timeout=60)
                want, _ = ref.compose_eigen(vec[fine], n, "abs", 0.5 * one[fine], co)
                assert np.abs(got[fine] - want).max() <= 1e-4, (n, family, il)
    for name, n, conj in (("mass4", 4, False), ("ind_comass4_ball", 4, True), ("mass5", 5, False), ("ind_comass5_ball", 5, True)):
        vec = rng.standard_normal((12, mref.DIM[n])) * 10
        vec[3, 2] = np.nan
        vec[7, 1] = np.inf
        fine = np.ones(12, dtype=bool)
        fine[[3, 7]] = False
        for il in (False, True):
            got = run_functor(harness, str(tmp_path), name, "zero", False, vec, il, 0.5, one, [1.0, 0, 0, 0, 0, 0, 0], timeout=60)
            want = mref.compose_mass(vec[fine], n, conj, 0.5 * one[fine])
            assert np.abs(got[fine] - want).max() <= 1e-4, (name, il)
