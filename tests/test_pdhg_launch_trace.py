"""The launch plan of the fused PDHG paths, pinned launch by launch on a MOCKED kernel ABI (CPU only).

BackendPDHG decides, for every iteration of every solve, which kernel runs, on which buffers, with which step sizes.
tests/host/pdhg_launch_trace_harness.cpp compiles the solver's host sources against a recording mock of include/prost_hip.h and prints,
per scenario, one line per launch (entry point, iterations per launch, every pointer as the ordinal of its allocation, the step sizes
of every iteration in hex floats, use_* flags, sums / rule / stored intermediate iterate, iteration number) and per host wait, event
operation, all-reduce and D2H copy, followed by the counters the backend reports and the buffers device_iterates() hands out.

Scenarios: every kernel family (two passes, gray single / pairs / groups of 3 and 4 / tolerance class, 3 channels with and without the
single kernel, volumes single / planes-across-waves / pairs, L = 2, the masked pair shape, tolerance-class 3-channel and volume pairs)
x alg1 / alg2 / goldstein / boyd x residual_iter 1, 2, 3, 7, 10 x four ways of driving (Solve with callbacks, Iterate in budgets
1, 2, 3, 5, 247, ..., a stop callback polled after every launch, Solve whose stopping test fires inside a device-resident batch), and a
subset with a communicator, on slabs with either transport, with and without the speculative launch.

tests/golden/pdhg_launch_traces.txt holds what the harness printed when the launch-plan refactor started (full text for a few
scenarios, a SHA-256 for the others).  A host-side change that is meant to leave every launch as it is must leave this file as it is.
After a change that is MEANT to alter the plan: python tests/test_pdhg_launch_trace.py --regenerate, and review the diff of the full
scenarios.
"""
import base64
import hashlib
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "pdhg_launch_trace_harness.cpp")
GOLDEN = os.path.join(ROOT, "tests", "golden", "pdhg_launch_traces.txt")
FAMILIES = ["twopass", "single", "pair", "group3", "group4", "fmad", "mc3", "mc3pair", "vol", "volpw", "volpair", "l2", "mask", "volpaironly", "mc3fmad", "volpairfmad"]
# scenarios kept as text: short runs that between them show pairs with and without the stored intermediate iterate, a speculative
# launch, a group period, a device-resident batch that stops half-way, and a rebuild behind a multi-channel pair
FULL_TEXT = ["pair.alg2.poll.r3", "fmad.alg1.poll.r7", "volpair.boyd.stop.r3", "mc3pair.goldstein.poll.r10"]


def _build(exe):
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-pthread", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "prost_amd", "csrc", "host"), SRC, "-o", exe,
           "-Wl,--unresolved-symbols=ignore-all"]
    return subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=os.path.dirname(SRC))


def _run_all(exe):
    r = subprocess.run([exe, "all"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    traces, name = {}, None
    for line in r.stdout.splitlines():
        if line.startswith("@ "):
            name = line[2:]
            assert name not in traces, name
            traces[name] = []
        else:
            traces[name].append(line)
    return traces


def _digest(lines):
    return base64.urlsafe_b64encode(hashlib.sha256(("\n".join(lines) + "\n").encode()).digest()).decode().rstrip("=")


def _read_golden():
    """{scenario: list of lines (full text) or (number of lines, digest)}"""
    golden, name = {}, None
    with open(GOLDEN) as f:
        for line in f.read().splitlines():
            if line.startswith("@ "):
                name = line[2:]
                golden[name] = []
            elif line.startswith("# "):
                group, *cells = line[2:].split()
                for cell in cells:
                    period, count, digest = cell.split(":")
                    golden["%s.%s" % (group, period)] = (int(count), digest)
                name = None
            elif name is not None:
                golden[name].append(line)
    return golden


def _write_golden(traces):
    groups = {}
    for name, lines in traces.items():
        if name in FULL_TEXT:
            continue
        group, period = name.rsplit(".", 1)
        groups.setdefault(group, []).append("%s:%d:%s" % (period, len(lines), _digest(lines)))
    with open(GOLDEN, "w") as f:
        for name in FULL_TEXT:
            f.write("@ %s\n%s\n" % (name, "\n".join(traces[name])))
        for group, cells in groups.items():
            f.write("# %s %s\n" % (group, " ".join(cells)))


@pytest.fixture(scope="module")
def traces(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("trace") / "pdhg_launch_trace_harness")
    b = _build(exe)
    assert b.returncode == 0, b.stderr[-3000:]
    return _run_all(exe)


def test_every_scenario_of_the_harness_is_pinned_and_nothing_else(traces):
    golden = _read_golden()
    assert sorted(golden) == sorted(traces)
    assert all(name in golden for name in FULL_TEXT)
    assert sorted({name.split(".")[0] for name in golden}) == sorted(FAMILIES)
    # every family with every rule, at an odd and an even residual_iter
    for family in FAMILIES:
        for rule in ("alg1", "alg2", "goldstein", "boyd"):
            periods = {int(name.rsplit(".r", 1)[1]) for name in golden if name.startswith("%s.%s." % (family, rule))}
            assert any(p % 2 for p in periods) and any(p % 2 == 0 for p in periods), (family, rule, periods)


@pytest.mark.parametrize("family", FAMILIES)
def test_launch_traces_equal_the_pinned_ones(traces, family):
    golden = _read_golden()
    names = [name for name in golden if name.split(".")[0] == family]
    assert names
    failures = []
    for name in names:
        got, want = traces[name], golden[name]
        assert not any("EXCEPTION" in line for line in got), (name, got[-1])
        if isinstance(want, tuple):
            if (len(got), _digest(got)) != want:
                failures.append("%s: %d lines with digest %s, pinned: %d lines with digest %s (run the harness with this name to see the trace)"
                                % (name, len(got), _digest(got), want[0], want[1]))
        elif got != want:
            at = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
            failures.append("%s: first difference in line %d\n  now:    %s\n  pinned: %s" % (name, at + 1, got[at] if at < len(got) else "<end>", want[at] if at < len(want) else "<end>"))
    assert not failures, "\n".join(failures[:10]) + "\n(%d of %d scenarios differ)" % (len(failures), len(names))


if __name__ == "__main__":
    if sys.argv[1:] != ["--regenerate"]:
        sys.exit("usage: python tests/test_pdhg_launch_trace.py --regenerate")
    exe = os.path.join(__import__("tempfile").mkdtemp(), "pdhg_launch_trace_harness")
    b = _build(exe)
    assert b.returncode == 0, b.stderr[-3000:]
    _write_golden(_run_all(exe))
    print("wrote", GOLDEN, os.path.getsize(GOLDEN), "bytes")
