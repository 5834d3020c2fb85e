"""The input ring of the level-per-wavefront K-iteration kernel at two and three slots, and the chunk rule at five workgroups per CU,
without a GPU.

tests/host/iterk_levelwave_ring_harness.cpp (stand-alone, built with AddressSanitizer and UBSan) runs wave 1 of every chunk step by
step from prost_amd/csrc/iterk_levelwave.hpp, the header the kernel and its launcher follow:
  * no ring slot receives a batch before the step after its last read (with two slots: the batch of column p + 1 goes into the slot of
    column p - 1, read one barrier ago);
  * the counted wait of a step (lw_ring_wait) equals the number of batches truly issued behind the column being read;
  * every loaded column is read exactly once, columns below 0 and at or beyond nx are never loaded;
  * K = 4 with per-pixel b holds 32 768 bytes of LDS, five workgroups per CU, and the one-round rule at 1280 slots gives 55 / 32 / 15 / 6 /
    72 columns at 4096^2 / 3072^2 / 2048^2 / 1024^2 / 8192^2.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COLS = [1, 2, 3, 7, 15, 55, 69]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("iterklwring") / "iterk_levelwave_ring_harness")
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "prost_amd", "csrc"),
                        "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "host", "iterk_levelwave_ring_harness.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    return exe


def run(exe, *args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok "), (args, r.stdout[-2000:], r.stderr[-2000:])
    return int(r.stdout.split()[1])


def widths(cols):
    """first (= only) and last chunks of 1, 2, cols - 1 and cols columns, behind one and behind several full chunks; nx down to 2"""
    w = {2, 3, cols, cols + 1, 3 * cols + 1, cols + 2, 4 * cols + 2, 2 * cols - 1, 5 * cols - 1, 2 * cols, 150}
    if cols > 1:
        w |= {1, cols - 1}
    return sorted(v for v in w if v >= 1)


@pytest.mark.parametrize("cols", COLS)
@pytest.mark.parametrize("K", [3, 4])
@pytest.mark.parametrize("R", [2, 3])
def test_ring_rules_hold(harness, R, K, cols):
    ws = widths(cols)
    assert {(nx - 1) % cols + 1 for nx in ws} >= {1, min(2, cols), max(1, cols - 1), cols}
    assert {min(nx, cols) for nx in ws} >= {1, min(2, cols), max(1, cols - 1), cols}          # the first chunk
    assert 2 in ws
    for nx in ws:
        assert run(harness, "ring", R, K, cols, nx) > 0


def test_lds_bytes_and_chunk_lengths_at_five_workgroups_per_cu(harness):
    assert run(harness, "geom") > 20


def test_an_unsupported_ring_depth_is_refused(harness):
    """a violated rule ends the harness with status 1: a ring of four slots, which no instance has, is refused, not passed"""
    r = subprocess.run([harness, "ring", "4", "4", "7", "50"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "VIOLATED" in r.stdout
