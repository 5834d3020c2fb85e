"""The arithmetic of ind_epi_polyhedral on the host, under AddressSanitizer and UndefinedBehaviorSanitizer:
tests/host/epi_polyhedral_harness.cpp is a stand-alone program (plain g++, no HIP) that runs include/prost/prox/epi_polyhedral.hpp --
the functions prost_amd/csrc/kernels_prox_epi_polyhedral.hip calls in every lane -- in the kernel's step loop with a serial scan, for
fp32 and fp64, dim 2 .. 4, random lists and the degenerate ones (duplicate, parallel, both pyramids, a = 0 rows, no constraints).
Its own brute force in long double is the truth; every case has to print `within` (max(4 e_T, 32 eps_T), e_T from an elimination in
T on the true active set), and no point may reach the step cap, whose constants are those of prost_hip_epi_polyhedral_plan."""
import ctypes as C
import subprocess

import host_harness
from prost_amd import _hip
CASES = ["random", "random1000", "duplicate", "parallel", "linf_pyramid", "l1_pyramid", "zero_rows"]


def plan_caps():
    L = _hip.lib()
    L.prost_hip_epi_polyhedral_plan.argtypes = [C.c_size_t, C.c_size_t, C.c_int] + [C.POINTER(C.c_int)] * 3
    L.prost_hip_epi_polyhedral_plan.restype = C.c_int
    ca, cb = C.c_int(-1), C.c_int(-1)
    assert L.prost_hip_epi_polyhedral_plan(25, 3, 0, None, C.byref(ca), C.byref(cb)) == 0
    return ca.value, cb.value


def test_active_set_projection_under_sanitizers(tmp_path):
    ca, cb = plan_caps()
    stdout = host_harness.run_sanitized("epi_polyhedral_harness", tmp_path, [str(ca), str(cb)])
    lines = stdout.strip().splitlines()
    assert lines[-1] == "ok" and "FAIL" not in stdout
    assert ", reached the cap 0, failures 0" in lines[-2]
    for t in ("fp32", "fp64"):
        for dim in (2, 3, 4):
            for name in CASES:
                assert any(l.startswith("%s %s dim=%d " % (name, t, dim)) and l.endswith("within") for l in lines), (name, t, dim)
            assert "empty %s dim=%d: within" % (t, dim) in lines
    # other cap constants are refused: the harness and the plan cannot drift apart unnoticed
    assert subprocess.run([str(tmp_path / "epi_polyhedral_harness"), str(ca + 1), str(cb)], capture_output=True, text=True, timeout=60, env=host_harness.sanitizer_env()).returncode == 1
