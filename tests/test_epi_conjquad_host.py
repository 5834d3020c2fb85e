"""The arithmetic of ind_epi_conjquad_1d on the host, under AddressSanitizer and UndefinedBehaviorSanitizer:
tests/host/epi_conjquad_harness.cpp is a stand-alone program (plain g++, no HIP) that runs include/prost/prox/epi_conjquad.hpp -- the
functions prost_amd/csrc/kernels_prox_epi_conjquad.hip calls in every lane -- in a plain loop, for fp32 and fp64, at scales 1 and 1000,
on cases built from their answers in long double (a boundary point and a move along its outward normal): random ones over every region
and a in {0, 1e-6, 1, 1e3}, alpha = beta, infinite bounds, u0 = 0, on the boundary, on the normal through a contact point, the vertex
cone, and a point high on the other side.  Every family has to print `within` (max(4 e_T, 32 eps_T) max(1, |z0|_inf)), and no point may
reach the step cap, which is the one prost_hip_epi_conjquad_step_cap answers."""
import ctypes as C
import re
import subprocess

import host_harness
from prost_amd import _hip
FAMILIES = ["random", "alpha_eq_beta", "infinite", "below_the_apex", "on_the_boundary", "normal_through_contact", "vertex_cone", "high_on_the_other_side"]


def step_cap(dtype):
    L = _hip.lib()
    L.prost_hip_epi_conjquad_step_cap.argtypes = [C.c_int, C.POINTER(C.c_int)]
    L.prost_hip_epi_conjquad_step_cap.restype = C.c_int
    cap = C.c_int(-1)
    assert L.prost_hip_epi_conjquad_step_cap(dtype, C.byref(cap)) == 0
    return cap.value


def test_projection_under_sanitizers(tmp_path):
    cap = step_cap(0)
    assert cap == step_cap(1)
    stdout = host_harness.run_sanitized("epi_conjquad_harness", tmp_path, [str(cap)])
    lines = stdout.strip().splitlines()
    assert lines[-1] == "ok" and "FAIL" not in stdout and "OUTSIDE" not in stdout
    assert ", reached the cap 0, failures 0" in lines[-2]
    most = int(re.search(r"most steps (\d+) of (\d+)", lines[-2]).group(1))
    assert 1 <= most < cap
    for t in ("fp32", "fp64"):
        for scale in ("1", "1000"):
            for name in FAMILIES:
                assert any(l.startswith("%s scale=%s %s: " % (name, scale, t)) and l.endswith("within") for l in lines), (name, scale, t)
    assert "cap 0: within" in lines
    # all five regions occur in the random family
    counts = re.search(r"regions (\d+)/(\d+)/(\d+)/(\d+)/(\d+)", next(l for l in lines if l.startswith("random scale=1 fp64"))).groups()
    assert all(int(c) > 100 for c in counts), counts
    # another cap is refused: the harness and the kernel's constant cannot drift apart unnoticed
    assert subprocess.run([str(tmp_path / "epi_conjquad_harness"), str(cap + 1)], capture_output=True, text=True, timeout=60, env=host_harness.sanitizer_env()).returncode == 1
