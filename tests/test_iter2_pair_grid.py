"""The wave grid of the paired two-iterations kernel, without a GPU.

prost_amd/csrc/iter2_grid.hpp maps (workgroup, wave) to a row strip and a column range; the kernel and its launcher
(kernels_fused_iter2.hip) read the grid from that header, and tests/host/iter2_grid_harness.cpp prints it.  With the chunk length the
launcher picks (prost_hip_fused_iteration2_chunk_cols, a host-only entry point) the grid of a plain ROF launch must be a partition:
every column of every strip owned by exactly one wave, the two chunks of a pair adjacent (wave 0 left of the seam, wave 1 right of
it), and a pair on one XCD (both waves are one workgroup, so that holds by construction and is not asserted).
"""
import ctypes as C
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "iter2_grid_harness.cpp")
ROWS = 62 * 4


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("iter2grid") / "iter2_grid_harness")
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "prost_amd", "csrc"), SRC, "-o", exe], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    return exe


def grid(exe, nx, ny, cols, pair):
    r = subprocess.run([exe, str(nx), str(ny), str(cols), "1" if pair else "0"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.split("\n")
    head = lines[0].split()
    rows = [tuple(int(v) for v in ln.split()) for ln in lines[1:] if ln]
    assert len(rows) == int(head[1]) * int(head[3])
    return int(head[1]), rows


def check_partition(nx, ny, cols, pair, blocks, rows):
    strips = -(-ny // ROWS)
    chunks = -(-nx // cols)
    assert blocks == strips * (-(-chunks // 2) if pair else chunks)
    owner = {}
    by_block = {}
    for b, w, strip, xa, xb in rows:
        assert 0 <= strip < strips
        by_block.setdefault(b, {})[w] = (strip, xa, xb)
        if xa >= xb:
            assert pair and w == 1, "only the second wave of an odd last pair may be empty"
            continue
        assert 0 <= xa and xb <= nx and xb - xa <= cols and xa % cols == 0
        for c in range(xa, xb):
            assert (strip, c) not in owner, "column %d of strip %d owned twice" % (c, strip)
            owner[(strip, c)] = (b, w)
    assert len(owner) == strips * nx, "columns without an owner"
    if pair:
        for b, ws in by_block.items():
            (s0, xa0, xb0), (s1, xa1, xb1) = ws[0], ws[1]
            assert s0 == s1 and xb0 > xa0, "the left-marching wave always has a chunk"
            if xa1 < xb1:
                assert xa1 == xb0, "the two chunks of a pair meet at their seam"
            else:
                assert xb0 == nx, "a pair without a second chunk ends at the image border"


def chunk_cols(nx, ny):
    from prost_amd import _hip as hip
    d = hip.FusedDesc(); d.is3d = 0; d.nx, d.ny, d.L = nx, ny, 1
    d.g_fn = hip.FN_ID["square"]; d.f_fn = hip.FN_ID["ind_leq0"]
    for i, (g, f) in enumerate(zip([1, 0.3, 10, 0, 0, 0, 0], [1, 1, 1, 0, 0, 0, 0])):
        d.g_coeff_val[i] = g; d.f_coeff_val[i] = f
    d.T_val, d.S_val = 0.25, 0.5
    return hip.lib().prost_hip_fused_iteration2_chunk_cols(C.byref(d), 0, 0)


@pytest.mark.parametrize("shape", [(4096, 4096), (3072, 3072), (2048, 2048), (5, 4096), (5, 8)])
def test_launch_plan_of_a_plain_rof_launch_is_a_partition_into_adjacent_pairs(harness, shape):
    nx, ny = shape
    cols = chunk_cols(nx, ny)
    assert 1 <= cols <= 36
    blocks, rows = grid(harness, nx, ny, cols, True)
    check_partition(nx, ny, cols, True, blocks, rows)


@pytest.mark.parametrize("pair", [False, True])
@pytest.mark.parametrize("nx,cols", [(5, 8), (5, 5), (16, 8), (17, 8), (18, 8), (19, 8), (24, 8), (25, 8), (7, 1), (8, 3), (2, 1), (9, 4)])
def test_grid_is_a_partition_for_every_chunk_count_and_remainder(harness, nx, cols, pair):
    """one chunk only, exactly two, odd and even counts, a last chunk of 1, 2 and 3 columns; one strip, two and nine (more workgroups
    than XCDs, and a count that is no multiple of 8)"""
    for ny in (8, 252, 2100):
        blocks, rows = grid(harness, nx, ny, cols, pair)
        check_partition(nx, ny, cols, pair, blocks, rows)
