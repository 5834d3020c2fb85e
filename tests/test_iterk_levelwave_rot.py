"""The one-round chunk rule of the level-per-wavefront K-iteration kernel, without a GPU.

  * tests/host/iterk_levelwave_rot_harness.cpp (stand-alone, built with AddressSanitizer and UBSan) checks lw_one_round_cols of
    prost_amd/csrc/iterk_levelwave.hpp: the length it returns fits one round, the next shorter one does not (or it is the lower bound),
    it is the upper bound where nothing fits, 69 columns / 1020 workgroups at 4096^2, 40 at 3072^2, 19 at 2048^2, 6 at 1024^2, 72 at 8192^2;
  * tests/host/iterk_levelwave_harness.cpp (the index simulation of tests/test_iterk_levelwave_plan.py) runs at the odd chunk lengths the
    rule now produces -- 7, 19, 69 -- over widths whose last chunk is 1, 2 and cols - 1 columns: every owned column is stored once, no slot
    is overwritten before its reader's step.

The level rotation planned beside the rule was measured and not built (docs/rounds/r26.md), so there is no lw_level to check.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp, name):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp / name)
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "prost_amd", "csrc"),
                        "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "host", name + ".cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    return exe


@pytest.fixture(scope="module")
def harnesses(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("iterklwcols")
    return _build(tmp, "iterk_levelwave_rot_harness"), _build(tmp, "iterk_levelwave_harness")


def run(exe, *args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok "), (args, r.stdout[-2000:], r.stderr[-2000:])
    return int(r.stdout.split()[1])


def test_the_one_round_rule_returns_the_shortest_length_that_fits(harnesses):
    assert run(harnesses[0], "cols") > 10000


@pytest.mark.parametrize("K", [3, 4])
@pytest.mark.parametrize("cols", [7, 19, 69])
def test_index_rules_hold_at_the_odd_lengths_of_the_rule(harnesses, K, cols):
    """last chunks of 1, 2 and cols - 1 columns behind one and behind several full chunks, and the full last chunk"""
    widths = sorted({cols + 1, 3 * cols + 1, cols + 2, 4 * cols + 2, 2 * cols - 1, 5 * cols - 1, 2 * cols, 150})
    assert {(nx - 1) % cols + 1 for nx in widths} >= {1, 2, cols - 1, cols}
    for nx in widths:
        assert run(harnesses[1], "index", K, cols, nx) > 0
