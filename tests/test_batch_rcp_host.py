"""The batched reciprocal of the dual prox (prost_amd/csrc/batch_rcp.hpp), without a GPU.

norm2_leq0_fast (device_math.hpp) divides by the norms of a lane's pixels through refined double reciprocals, two of which come
from ONE seed (Montgomery's batch inversion; the header also holds the form for four, which no kernel uses).  The header is plain
C++; tests/host/batch_rcp_harness.cpp runs both forms on the CPU, built with the host compiler and -ffp-contract=off, and compares
(float)fma((double)n, r_i, 0.0) with the host's n / d_i in float bit for bit: 2^26 random quadruples over the whole clamped range
of the divisors and the directed classes its header lists, every case with the seed perturbed by -2^-23 and +2^-23 relative.  No
mismatch is allowed in any class.

Known and counted, not hidden: exact ties of a subnormal quotient with a power-of-two divisor.  The single reciprocal rounds them
like the division (asserted); the shared ones round about one in eight the other way (5.7 x 10^3 of 4.6 x 10^4 cases, both
forms and all seeds counted; the harness prints the figure).
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "batch_rcp_harness.cpp")
LOG2_RANDOM = 26
# the least number of comparisons per class: four quotients per quadruple, seed (two; three for the directed classes) and form (two)
MIN_CASES = {"random": 15 << LOG2_RANDOM, "extremes": 10 ** 6, "equal": 10 ** 6, "ulp": 10 ** 6, "zero": 10 ** 7, "subnormal": 10 ** 7,
             "boundary": 3 * 10 ** 7, "worst": 10 ** 7}


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("batchrcp") / "batch_rcp_harness")
    b = subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-pthread", "-I" + os.path.join(ROOT, "prost_amd", "csrc"), SRC, "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe, str(LOG2_RANDOM)], capture_output=True, text=True, timeout=600)
    assert r.returncode in (0, 1), r.stderr[-3000:]
    rows = {}
    for ln in r.stdout.split("\n"):
        w = ln.split()
        if len(w) == 3:
            rows[w[0]] = (int(w[1]), int(w[2]))
        elif len(w) == 2 and w[0] == "ties":
            rows["ties"] = int(w[1])
        elif len(w) == 4 and w[0] == "tie_pow2":
            rows["tie_pow2"] = tuple(int(v) for v in w[1:])
    return rows, r.stderr[-3000:]


@pytest.mark.parametrize("cls", sorted(MIN_CASES))
def test_quotients_through_the_batched_reciprocal_equal_the_division(report, cls):
    rows, err = report
    cases, bad = rows[cls]
    assert cases >= MIN_CASES[cls], (cls, cases)
    assert bad == 0, (cls, bad, err)


def test_power_of_two_ties_are_counted_and_the_single_reciprocal_rounds_them_like_the_division(report):
    rows, _ = report
    cases, shared, single = rows["tie_pow2"]
    print("subnormal ties with a power-of-two divisor: %d cases, shared reciprocals differ from the division in %d, the single one in %d" % (cases, shared, single))
    assert cases >= 1000 and single == 0 and shared <= cases, rows["tie_pow2"]


def test_only_subnormal_ties_are_left_out(report):
    """exact ties of a subnormal quotient are outside the guarantee (batch_rcp.hpp); they stay below one case in 10^4"""
    rows, _ = report
    assert rows["ties"] <= sum(rows[c][0] for c in MIN_CASES) // 10 ** 4, rows
