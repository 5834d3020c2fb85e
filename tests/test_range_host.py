"""The per-block arithmetic of the ind_range solve on the host, under AddressSanitizer and UndefinedBehaviorSanitizer:
tests/host/potrs_blocks_harness.cpp is a stand-alone program (plain g++, no HIP) that runs include/prost/prox/potrs_blocks.hpp -- the
functions prost_amd/csrc/kernels_prox_range.hip calls lane by lane -- in loops: the blocked factorisation and both sweeps with the NB of
prost_hip_range_potrs_plan, for fp32 and fp64 and n in {1, 2, NB - 1, NB, NB + 1, 2 NB + 1}.  The exact family must come out bit for bit;
the tolerance family within max(4 e_T, 32 eps_T) of an unblocked loop in long double, e_T being the error of that loop in T."""
import ctypes as C
import subprocess

import host_harness
from prost_amd import _hip


def plan_nb():
    L = _hip.lib()
    L.prost_hip_range_potrs_plan.argtypes = [C.c_size_t, C.c_int] + [C.POINTER(C.c_int)] * 3 + [C.POINTER(C.c_size_t)] * 2
    L.prost_hip_range_potrs_plan.restype = C.c_int
    nb = C.c_int(0)
    assert L.prost_hip_range_potrs_plan(100, 0, None, C.byref(nb), None, None, None) == 0
    return nb.value


def test_blocked_factorisation_and_sweeps_under_sanitizers(tmp_path):
    nb = plan_nb()
    stdout = host_harness.run_sanitized("potrs_blocks_harness", tmp_path, [str(nb)])
    lines = stdout.strip().splitlines()
    assert lines[-1] == "ok" and "FAIL" not in stdout
    sizes = [1, 2, nb - 1, nb, nb + 1, 2 * nb + 1]
    for t in ("fp32", "fp64"):
        for n in sizes:
            assert "exact %s n=%d: equal" % (t, n) in lines, (t, n)
            assert any(l.startswith("tolerance %s n=%d:" % (t, n)) and l.endswith("within") for l in lines), (t, n)
    assert "indefinite: pivot 1" in lines
    # a wrong NB is refused: the harness and the plan cannot drift apart unnoticed
    assert subprocess.run([str(tmp_path / "potrs_blocks_harness"), str(nb + 1)], capture_output=True, text=True, timeout=60, env=host_harness.sanitizer_env()).returncode == 1
