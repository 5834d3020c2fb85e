"""What BackendADMM launches, pinned launch by launch on a MOCKED kernel ABI (CPU only) -- the counterpart of test_pdhg_launch_trace.py.

BackendADMM runs its CGLS solve in one of five ways (host-driven, staged rounds, staged rounds replayed from a captured graph, four-launch
rounds with the operator inside, two-launch pixel rounds) and decides per outer iteration which stages, products, proxes, copies, waits
and rescales go with it.  tests/host/admm_launch_trace_harness.cpp compiles the solver's host sources against a recording mock of
include/prost_hip.h and prints, per scenario, one line per launch (entry point, stage / round, every pointer as the ordinal of its
allocation, every scalar as a hex float), host wait, copy, event operation, capture, graph launch and all-reduce, then what KernelTimes
reports and the two read-outs.

Scenarios: the five modes (the pixel rounds on five operator shapes) x cg_max_iter 0, 1, 10 x residual_iter 1, 3 x the device's stop
word never / on round 0 / on round 3 x kernel timing off / every solve / every third; each mode with prox_g = one ProxZero, with
Moreau-wrapped proxes and with a communicator; and every way DescribeOperator turns an operator away, one short scenario each.

tests/golden/admm_launch_traces.txt holds what the harness printed before the host code was reorganised (full text for a few
scenarios, a SHA-256 for the others).  A host-side change that is meant to leave every launch as it is must leave this file as it is.
After a change that is MEANT to alter the launches: python tests/test_admm_launch_trace.py --regenerate, and review the diff of the
full scenarios.
"""
import base64
import hashlib
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "admm_launch_trace_harness.cpp")
GOLDEN = os.path.join(ROOT, "tests", "golden", "admm_launch_traces.txt")
# mode -> (CG solve on the device, rounds that can be sampled by kernel timing, path())
MODES = {"host": (False, False, "admm:generic"), "staged": (True, False, "admm:generic"), "graph": (True, False, "admm:generic"),
         "fused4": (True, True, "admm:fused-op"), "pixdiag1": (True, True, "admm:pixel-op"), "pixdiag2": (True, True, "admm:pixel-op"),
         "pixcsr1": (True, True, "admm:pixel-op"), "pixcsr2": (True, True, "admm:pixel-op"), "pixgrad": (True, True, "admm:pixel-op")}
# what DescribeOperator turns away -> the path that runs instead
REJECTIONS = {"dual": "admm:generic", "manyblocks": "admm:generic", "nodescribe": "admm:generic", "csrrow": "admm:generic", "csrcol": "admm:generic",
              "labelfirst": "admm:generic", "fusedunsupported": "admm:generic", "pixeloff": "admm:fused-op", "threeblocks": "admm:fused-op",
              "gradoffset": "admm:fused-op", "fourchannels": "admm:fused-op", "drows": "admm:fused-op", "dcols": "admm:fused-op", "planes": "admm:fused-op",
              "sigma": "admm:fused-op", "pixelunsupported": "admm:fused-op"}
# scenarios kept as text: short runs that between them show a sampled round 0 closed by the stop word, the four-launch round's eight
# events, the captured graph next to the ProxZero it forbids to exchange, every way out of the host-driven solve, and two rejections
FULL_TEXT = ["pixdiag1.base.m1.s0.t3.r3", "fused4.base.m1.sno.t1.r1", "graph.proxzero.m1.sno.t0.r3", "host.base.m10.sno.t0.r3", "reject.sigma.r1", "reject.dcols.r1"]


def _expected_names():
    names = []
    for mode, (device, timed, _) in MODES.items():
        for maxit in (0, 1, 10):
            for stop in (-1, 0, 3):
                if stop >= 0 and (not device or stop >= maxit):
                    continue
                for every in (0, 1, 3):
                    if every and not timed and not (every == 1 and maxit == 10 and stop < 0):
                        continue
                    names += ["%s.base.m%d.s%s.t%d.r%d" % (mode, maxit, "no" if stop < 0 else stop, every, period) for period in (1, 3)]
        for variant in ("proxzero", "moreau", "comm"):
            for maxit in (1, 10):
                names += ["%s.%s.m%d.s%s.t%d.r%d" % (mode, variant, maxit, 3 if device and maxit > 3 else "no", 3 if timed else 0, period) for period in (1, 3)]
    return names + ["reject.%s.r1" % r for r in REJECTIONS]


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
    exe = str(tmp_path_factory.mktemp("trace") / "admm_launch_trace_harness")
    b = _build(exe)
    assert b.returncode == 0, b.stderr[-3000:]
    return _run_all(exe)


def test_every_scenario_of_the_harness_is_pinned_and_nothing_else(traces):
    golden = _read_golden()
    assert sorted(golden) == sorted(traces)
    assert sorted(golden) == sorted(_expected_names())
    assert all(name in golden for name in FULL_TEXT)


def test_every_scenario_runs_the_path_it_is_named_for(traces):
    for name, lines in traces.items():
        head = name.split(".")
        want = REJECTIONS[head[1]] if head[0] == "reject" else MODES[head[0]][2]
        assert any(line.startswith("-- initialized: path %s " % want) for line in lines), (name, want)
        last = [line for line in lines if line.startswith("-- sizes")][-1]          # (Release may leave a wait behind it)
        assert " path %s " % want in last, (name, last)


def test_every_rejection_ends_where_it_is_meant_to(traces):
    """how far DescribeOperator got: refused before the kernel library was asked about the block table, by that answer, after it and
    before the question about the pixel operator (every test of the pixel shape), or by the answer to that one"""
    before_table = ["dual", "manyblocks", "nodescribe", "csrrow", "csrcol", "labelfirst"]
    for r in REJECTIONS:
        text = "\n".join(traces["reject.%s.r1" % r])
        assert ("fused_op_supported?" in text) == (r not in before_table), r
        assert ("-> 0" in text.split("fused_op_supported?")[-1].split("\n")[0]) == (r == "fusedunsupported"), r
        assert ("pixel_op_supported?" in text) == (r == "pixelunsupported"), r
    asked = [line for line in traces["reject.pixelunsupported.r1"] if line.startswith("pixel_op_supported?")]
    assert len(asked) == 1 and "d_csr=0" in asked[0] and asked[0].endswith("-> 0")
    # the two D-CSR rejections hand over a block that is NOT pointwise, `planes` one that is (its table entry has the same CSR arrays)
    assert "size=29x60" in "\n".join(traces["reject.drows.r1"]) and "size=30x59" in "\n".join(traces["reject.dcols.r1"])
    assert "size=30x30" in "\n".join(traces["reject.planes.r1"])


def test_the_mock_answers_reach_every_branch_they_are_meant_for(traces):
    text = {name: "\n".join(lines) for name, lines in traces.items()}
    # the stop word ends the round loop early, and the record read afterwards is the one behind the last queued round
    t = text["pixdiag1.base.m10.s3.t0.r1"]
    assert "stop word" in t and "cgls_pixel_close 3 " in t and "cgls_pixel_close 9 " in t and "index=4 " in t and "index=10 " in t
    t = text["fused4.base.m10.s0.t0.r1"]
    assert "stop word" in t and "index=1 " in t and "index=10 " in t
    # kernel timing with one round per solve samples round 0, otherwise round 1
    assert "cgls_pixel_round_timed 0 " in text["pixgrad.base.m1.sno.t1.r1"] and "cgls_pixel_round_timed 1 " in text["pixgrad.base.m10.sno.t1.r1"]
    assert "-- kernel cg_pixel_pq_kernel" in text["pixgrad.base.m1.sno.t3.r1"] and "-- kernel cg_step_p2_kernel" in text["fused4.base.m1.sno.t3.r1"]
    # both branches of the rho adaptation (two rescale launches each time), the all-reduce, capture once and replay afterwards
    for name in ("host.base.m10.sno.t0.r1", "staged.base.m10.sno.t0.r1", "pixcsr2.base.m10.sno.t0.r1"):
        rhos = {line.split(" rho ")[1].split()[0] for line in traces[name] if line.startswith("-- iteration")}
        assert len(rhos) >= 3 and text[name].count("admm_elem op=10 ") >= 4, (name, rhos)
    assert "allreduce 4 " in text["fused4.comm.m10.s3.t3.r1"]
    t = text["graph.base.m10.sno.t0.r1"]
    assert t.count("begin_capture") == 1 and t.count("graph_launch") == 12
    # the ProxZero buffer exchange: no copy for it, except under a captured graph
    def copies(name):
        return [line for line in traces[name][:traces[name].index("-- current_solution(primal, dual)")] if line.startswith("d2d ")]
    assert "prox_elem op=0 fn=2" not in text["staged.proxzero.m10.s3.t0.r1"] and not copies("staged.proxzero.m10.s3.t0.r1")
    assert len(copies("graph.proxzero.m10.s3.t0.r1")) == 12
    assert "prox_elem_moreau" in text["pixgrad.moreau.m10.s3.t3.r1"]
    # the host-driven solve leaves by each of its ways out
    iters = {line.split("cg_iterations ")[1].split()[0] for line in traces["host.base.m10.sno.t0.r1"] if line.startswith("-- iteration")}
    assert iters == {"0", "1", "2", "10"}, iters


@pytest.mark.parametrize("mode", list(MODES) + ["reject"])
def test_launch_traces_equal_the_pinned_ones(traces, mode):
    golden = _read_golden()
    names = [name for name in golden if name.split(".")[0] == mode]
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
        sys.exit("usage: python tests/test_admm_launch_trace.py --regenerate")
    exe = os.path.join(__import__("tempfile").mkdtemp(), "admm_launch_trace_harness")
    b = _build(exe)
    assert b.returncode == 0, b.stderr[-3000:]
    _write_golden(_run_all(exe))
    print("wrote", GOLDEN, os.path.getsize(GOLDEN), "bytes")
