"""The spectral function family without a GPU: builders, registry names, creation errors, and the arithmetic of the public functor
headers (the same functions the gfx950 kernel calls) compiled for the host and compared with an fp64 NumPy composition.

  * prost.function.sum_singular_nx2 / sum_eigen_2x2 / sum_eigen_3x3 produce the nested list of the .m builders;
  * the 40 names of the reference's factory table are registered for both precisions;
  * a bad shape raises ProstError with the prox's name when the prox is created (prost.problem_info: host only);
  * tests/host/spectral_functor_harness.cpp runs ElemOperationSingularNx2 / Eigen2x2 / Eigen3x3 over Vector views on the host:
    inf-norm <= 1e-4 against tests/spectral_reference.py for every function, both precisions, both layouts, with the exclusion
    rule for the discontinuous functions (at most 0.5 % of the groups).
"""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import prost_amd as prost
import spectral_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def _same(a, b):
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return np.array_equal(np.asarray(a, dtype=np.float64).ravel(), np.asarray(b, dtype=np.float64).ravel())
    return type(a) == type(b) and a == b


def test_builders_mirror_the_m_builders():
    one = lambda v: np.array([float(v)])
    # sum_singular_nx2.m:28  { strcat('elem_operation:singular_nx2:', fun), idx, count, false, { count / dim, dim, interleaved, coeffs } }
    d = prost.function.sum_singular_nx2(6, False, "sum_1d:abs", 2, 3, 4, 5, 6, 0.5, 1.5)(12, 60)
    assert _same(d, ["elem_operation:singular_nx2:sum_1d:abs", 12, 60, False, [10, 6, False, [one(2), one(3), one(4), one(5), one(6), one(0.5), one(1.5)]]])
    d = prost.function.sum_singular_nx2(4, True, "ind_l1_ball")(0, 40)
    assert _same(d, ["elem_operation:singular_nx2:ind_l1_ball", 0, 40, False, [10, 4, True, [one(1), one(0), one(1), one(0), one(0), one(0), one(0)]]])
    b = np.arange(5.0)
    d = prost.function.sum_eigen_2x2(True, "huber", 1, b, 2, 0, 0, 0.25)(8, 20)                          # sum_eigen_2x2.m: dim = 4
    assert _same(d, ["elem_operation:eigen_2x2:huber", 8, 20, False, [5, 4, True, [one(1), b, one(2), one(0), one(0), one(0.25), one(0)]]])
    d = prost.function.sum_eigen_3x3(False, "ind_leq0", -1)(0, 27)                                        # sum_eigen_3x3.m: dim = 9
    assert _same(d, ["elem_operation:eigen_3x3:ind_leq0", 0, 27, False, [3, 9, False, [one(-1), one(0), one(1), one(0), one(0), one(0), one(0)]]])
    assert d[3] is False and d[4][2] is False


@pytest.mark.parametrize("precision", ["single", "double"])
def test_the_reference_names_are_registered(precision):
    prost.set_precision(precision)
    try:
        reg = set(prost.registered()["prox"])
    finally:
        prost.set_precision("double")
    names = ["elem_operation:singular_nx2:sum_1d:" + f for f in ref.SINGULAR_1D]
    names += ["elem_operation:singular_nx2:ind_l1_ball", "elem_operation:singular_nx2:moreau:ind_l1_ball"]
    names += ["elem_operation:eigen_%s:%s" % (k, f) for k in ("2x2", "3x3") for f in ref.FUNCTIONS_1D]
    assert len(names) == 40
    assert not [n for n in names if n not in reg]
    # what the builder produces for a bare function name (the spelling of the example) names the same prox
    assert "elem_operation:singular_nx2:ind_leq0" in reg


def _problem_with_dual_prox(desc, size):
    u, q = prost.variable(size // 2), prost.variable(size)
    prob = prost.min_max_problem([u], [q])
    prob.add_function(q, lambda idx, count: desc)
    prob.add_dual_pair(u, q, prost.block.gradient2d(size // 2, 1, 1))
    return prob


@pytest.mark.parametrize("precision", ["single", "double"])
def test_bad_shapes_raise_at_creation_with_the_name_of_the_prox(precision):
    prost.set_precision(precision)
    try:
        co = [np.array([1.0]), np.array([0.0]), np.array([1.0]), np.array([0.0]), np.array([0.0]), np.array([0.0]), np.array([0.0])]
        cases = [(["elem_operation:singular_nx2:sum_1d:abs", 0, 30, False, [6, 5, False, co]], "singular_nx2"),      # odd dim
                 (["elem_operation:eigen_2x2:abs", 0, 36, False, [4, 9, False, co]], "eigen_2x2"),                  # dim != 4
                 (["elem_operation:eigen_3x3:abs", 0, 36, False, [9, 4, False, co]], "eigen_3x3"),                  # dim != 9
                 (["elem_operation:singular_nx2:ind_l1_ball", 0, 36, False, [5, 6, False, co]], "singular_nx2"),    # size != count * dim
                 (["elem_operation:eigen_2x2:zero", 0, 36, False, [8, 4, True, co]], "eigen_2x2"),
                 (["elem_operation:eigen_3x3:zero", 0, 36, False, [3, 9, True, co]], "eigen_3x3")]
        for desc, name in cases:
            prob = _problem_with_dual_prox(desc, desc[2])
            with pytest.raises(prost.ProstError, match=name) as err:
                prost.problem_info(prob)
            assert "Creating prox with ID '%s' failed" % desc[0] in str(err.value)
        good = _problem_with_dual_prox(["elem_operation:eigen_3x3:zero", 0, 36, False, [4, 9, True, co]], 36)
        prost.problem_info(good)
    finally:
        prost.set_precision("double")


# ---- the functor headers on the host ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("spectral") / "spectral_functor_harness")
    cmd = [HIPCC, "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-O1", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "host", "spectral_functor_harness.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert b.returncode == 0, b.stderr[-3000:]
    return exe


FAMILY = {"singular_nx2": 0, "eigen_2x2": 1, "eigen_3x3": 2}


def _fn_id(fn):
    return {"ind_l1_ball": 100, "moreau:ind_l1_ball": 101}.get(fn, ref.FUNCTIONS_1D.index(fn) if fn in ref.FUNCTIONS_1D else -1)


def run_functor(exe, tmp, family, fn, single, vec, interleaved, tau, tau_group, coeffs, invert_tau=False):
    """vec (G, dim) groups -> result (G, dim) from the host-compiled functor"""
    G, dim = vec.shape
    path_in, path_out = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    td = np.repeat(tau_group[:, None], dim, axis=1)
    with open(path_in, "wb") as f:
        f.write(struct.pack("7q", FAMILY[family], _fn_id(fn), int(single), dim, G, int(interleaved), int(invert_tau)))
        f.write(struct.pack("d", tau))
        f.write(ref.flat_from_groups(vec, interleaved).astype(np.float64).tobytes())
        f.write(ref.flat_from_groups(td, interleaved).astype(np.float64).tobytes())
        for c in coeffs:
            f.write(ref.per_group(c, G).astype(np.float64).tobytes())
    r = subprocess.run([exe, path_in, path_out], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return ref.groups_from_flat(np.fromfile(path_out, dtype=np.float64), dim, interleaved)


def _inputs(rng, G, dim, single, per_group_coeffs):
    rnd = (lambda a: a.astype(np.float32).astype(np.float64)) if single else (lambda a: a)
    vec = rnd(rng.standard_normal((G, dim)) * 10)
    tau_group = rnd(rng.uniform(0.5, 1.5, G))
    if per_group_coeffs:
        coeffs = [rnd(rng.uniform(0.5, 2.0, G)), rnd(rng.uniform(-1, 1, G)), rnd(rng.uniform(0.5, 2.0, G)), rnd(rng.uniform(-1, 1, G)),
                  rnd(rng.uniform(0, 1, G)), 0.5, 1.0]
    else:
        coeffs = [1.0, 0.0, 1.0, 0.0, 0.0, 0.5, 1.0]
    return vec, tau_group, coeffs


def check_against_composition(got, vec, family, fn, tau, coeffs, single, what):
    if family == "singular_nx2":
        want, mark = ref.compose_singular(vec, fn, tau, coeffs)
    else:
        want, mark = ref.compose_eigen(vec, 2 if family == "eigen_2x2" else 3, fn, tau, coeffs)
    share = float(mark.mean())
    err = float(np.abs(got - want)[~mark].max())
    print("%s: inf-norm %.3g, marked %.4f %%" % (what, err, 100 * share))
    assert share <= 0.005, (what, share)
    assert err <= 1e-4, (what, err)


@pytest.mark.parametrize("single", [True, False])
@pytest.mark.parametrize("family,dim", [("eigen_2x2", 4), ("eigen_3x3", 9), ("singular_nx2", 2), ("singular_nx2", 6), ("singular_nx2", 16)])
def test_host_compiled_functors_equal_the_numpy_composition(harness, tmp_path, family, dim, single):
    rng = np.random.default_rng(7)
    fns = ref.FUNCTIONS_1D if family != "singular_nx2" else ref.SINGULAR_1D + ("ind_l1_ball", "moreau:ind_l1_ball")
    for k, fn in enumerate(fns):
        G = 2003
        vec, tau_group, coeffs = _inputs(rng, G, dim, single, per_group_coeffs=k % 2 == 1)
        if fn.endswith("ind_l1_ball"):
            coeffs[5] = 7.5                     # the radius: a ball that cuts through the data
        tau = 0.75
        interleaved = k % 3 != 0
        got = run_functor(harness, str(tmp_path), family, fn, single, vec, interleaved, tau, tau_group, coeffs)
        step = (np.float32(tau) * tau_group.astype(np.float32)).astype(np.float64) if single else tau * tau_group
        check_against_composition(got, vec, family, fn, step, coeffs, single, "%s dim %d %s %s" % (family, dim, fn, "fp32" if single else "fp64"))


def test_host_compiled_functors_keep_the_edge_conventions(harness, tmp_path):
    co = [1.0, 0.0, 1.0, -1.0, 0.0, 0.0, 0.0]          # h(t) = -t: every value moves up by the step, also a zero one
    one = np.ones(3)
    # the zero matrix: res[0] = p1, res[n + 1] = p2, zero elsewhere; rank 1: the part of the zero singular value is dropped
    vec = np.zeros((3, 6))
    vec[1] = np.outer([3.0, 4.0], [1.0, 2.0, 2.0]).ravel()          # columns (3, 6, 6) and (4, 8, 8): singular values 15, 0
    vec[2] = np.outer([0.0, 1.0], [2.0, 0.0, 0.0]).ravel()
    got = run_functor(harness, str(tmp_path), "singular_nx2", "zero", False, vec, False, 0.5, one, co)
    assert np.array_equal(got[0], [0.5, 0, 0, 0, 0.5, 0])
    assert np.abs(got[1] - vec[1] * (15.5 / 15.0)).max() <= 1e-12
    assert np.abs(got[2] - vec[2] * (2.5 / 2.0)).max() <= 1e-12
    # n = 1: a zero row stays inside its group
    got = run_functor(harness, str(tmp_path), "singular_nx2", "zero", False, np.zeros((3, 2)), True, 0.5, one, co)
    assert np.array_equal(got, [[0.5, 0]] * 3)
    # repeated eigenvalues: multiples of the identity and a matrix with a double eigenvalue
    vec = np.array([np.eye(3).ravel() * 2, (np.eye(3) + np.ones((3, 3))).ravel(), np.zeros(9)])
    got = run_functor(harness, str(tmp_path), "eigen_3x3", "abs", False, vec, True, 0.5, one, [1.0, 0, 1.0, 0, 0, 0, 0])
    want, _ = ref.compose_eigen(vec, 3, "abs", 0.5 * one, [1.0, 0, 1.0, 0, 0, 0, 0])
    assert np.abs(got - want).max() <= 1e-12
