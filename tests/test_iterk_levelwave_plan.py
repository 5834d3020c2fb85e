"""The index rules of the level-per-wavefront K-iteration kernel and the pair plan with launches of four, without a GPU.

tests/host/iterk_levelwave_harness.cpp is a stand-alone program (built with AddressSanitizer and UBSan) that
  * simulates every chunk of an image step by step from prost_amd/csrc/iterk_levelwave.hpp -- the header the kernel and its launcher
    read the same rules from: every column a level reads was written in an earlier step into the other slot, no slot (links and input
    ring) is overwritten before its reader's step, every stage reads only columns that were computed, each owned column is stored
    exactly once, every wave meets the same number of barriers;
  * walks include/prost/backend/pdhg_pair_plan.hpp over periods 1, 2, 3, 7, 10 and budgets 1 .. 12: iterations covered once, no
    group contains or directly precedes a residual iteration, behind the first residual period a group stands exactly where two
    plain pairs would follow one another, and with groups off the plan is the pair plan.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "iterk_levelwave_harness.cpp")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("iterklw") / "iterk_levelwave_harness")
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "prost_amd", "csrc"),
                        "-I" + os.path.join(ROOT, "include"), SRC, "-o", exe], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    return exe


def run(exe, *args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok "), (args, r.stdout[-2000:], r.stderr[-2000:])
    return int(r.stdout.split()[1])


@pytest.mark.parametrize("K", [3, 4])
@pytest.mark.parametrize("cols", [1, 2, 3, 5, 18, 72])
def test_index_rules_hold_for_every_chunk(harness, K, cols):
    """widths with a full, a one-column, an odd and a short last chunk, and images narrower than one chunk"""
    for nx in sorted({8, 9, 19, 37, 150, cols, cols + 1, 2 * cols, 2 * cols + 1, 3 * cols - 1, 5 * cols + 2}):
        assert run(harness, "index", K, cols, nx) > 0


def test_pair_plan_with_launches_of_four(harness):
    assert run(harness, "plan") > 1000
