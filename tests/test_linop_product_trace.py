"""What every in-tree linear-operator block hands to the kernel C ABI, pinned call by call on a MOCKED ABI (CPU only).

tests/host/linop_product_trace_harness.cpp compiles prost_amd/csrc/host/{common,linop}.cpp against a recording mock of
include/prost_hip.h (device memory is host memory, an upload is a memcpy) and prints, per block and placement, one line per ABI call:
the entry point, every pointer as allocation ordinal + byte offset, every size and flag, every double in hex, and length + FNV digest
of every device array passed (CSR arrays, pattern tables, anchors, gamma, tap tables, per-angle tables, positions and bucket tables,
twiddle tables, tensor planes) and of every host record (the geometry records, the wavelet taps).  Host-only answers
follow: sizes, gpu_mem_amount, describe / stencil_shape / uniform_sums, every row and column sum at alpha 1 and 2 and whether
row_sums / col_sums add exactly those, and the exception text of a product before Initialize().

Blocks: gradient2d / gradient3d (label_first 0 and 1), sparse (a 5 x 7 matrix that stays CSR, the 300 x 300 forward difference that runs
from row patterns, a 300 x 600 matrix that runs from anchored patterns, a matrix without entries), both sparse and both dense Kronecker
blocks, dense, dataterm_sublabel, conv2d, sym_gradient2d, conv2d_strided, radon2d, sample2d, fft2d, wavelet2d, tensor_gradient2d (k = 3
and k = 1), diags and zero, in float and double; each alone at (0, 0), as the second of
two copies stacked below the first and as the second of two side by side, through LinearOperator::Eval / EvalAdjoint and
DualLinearOperator at beta 0 and 1 -- so the exclusive, first-writer and accumulate paths reach all four evaluation virtuals.

tests/golden/linop_product_traces.txt holds what the harness printed at commit c7472ab ("sym_gradient2d: matrix-free symmetrised
gradient block for TGV"), where every block still wrote out its four evaluation virtuals and BlockSparse kept K and K^T as parallel
member lists: the text of a few placements, and for every placement of every scenario its number of lines and a SHA-256 (as in
pdhg_launch_traces.txt).  The lines of the six blocks from conv2d_strided to tensor_gradient2d were added at commit a60a5bd
("tensor_gradient2d: matrix-free weighted / anisotropic gradient block") with the library sources of that commit; the lines from before
did not change, and the whole output is 11 332 lines.  A host-side change that is meant to leave every ABI call as it is must leave this
file as it is.  After a change that is MEANT to alter a call: python tests/test_linop_product_trace.py --regenerate, and review the diff.

The harness is a stand-alone program and runs under AddressSanitizer and UndefinedBehaviorSanitizer: the mock reads every array at the
length the ABI implies, so a short upload is a report.
"""
import base64
import hashlib
import os
import sys
import tempfile

import pytest

import host_harness

GOLDEN = os.path.join(host_harness.ROOT, "tests", "golden", "linop_product_traces.txt")
HARNESS = "linop_product_trace_harness"
EXTRA_FLAGS = ["-pthread", "-I" + os.path.join(host_harness.ROOT, "prost_amd", "csrc", "host"), "-Wl,--unresolved-symbols=ignore-all"]
BLOCKS = ["gradient2d", "gradient3d", "sparse", "sparse_kron_id", "id_kron_sparse", "dense", "dense_kron_id", "id_kron_dense", "dataterm_sublabel", "conv2d",
          "sym_gradient2d", "conv2d_strided", "radon2d", "sample2d", "fft2d", "wavelet2d", "tensor_gradient2d", "diags", "zero"]
PLACEMENTS = ["alone", "below", "right"]
# kept as text: a CSR and a pattern-compressed sparse block and a Kronecker block (the classes with two sides), the second at offset pointers
FULL_TEXT = ["sparse.random5x7.f32 alone", "sparse.difference300.f32 alone", "id_kron_sparse.f64 below"]
# blocks with a guard, and its text
GUARDS = {"sparse": "BlockSparse", "sparse_kron_id": "BlockKronSparse", "id_kron_sparse": "BlockKronSparse", "dense": "BlockDense", "dense_kron_id": "BlockKronDense",
          "id_kron_dense": "BlockKronDense", "dataterm_sublabel": "BlockDatatermSublabel", "conv2d": "BlockConv2D", "conv2d_strided": "BlockConv2DStrided", "radon2d": "BlockRadon2D",
          "sample2d": "BlockSample2D", "fft2d": "BlockFFT2D", "wavelet2d": "BlockWavelet2D", "tensor_gradient2d": "BlockTensorGradient2D", "diags": "BlockDiags"}


def _split(text):
    """{"<scenario> <placement>": lines}"""
    traces, name, key = {}, None, None
    for line in text.splitlines():
        if line.startswith("@ "):
            name, key = line[2:], None
        else:
            if line.startswith("-- placement "):
                key = "%s %s" % (name, PLACEMENTS[sum(1 for k in traces if k.startswith(name + " "))])
                assert key not in traces, key
                traces[key] = []
            traces[key].append(line)
    return traces


def _digest(lines):
    return base64.urlsafe_b64encode(hashlib.sha256(("\n".join(lines) + "\n").encode()).digest()).decode().rstrip("=")


def _read_golden():
    """({key: (number of lines, digest)}, {key of FULL_TEXT: lines})"""
    pinned, text, key = {}, {}, None
    with open(GOLDEN) as f:
        for line in f.read().splitlines():
            if line.startswith("@ "):
                key = line[2:]
                text[key] = []
            elif line.startswith("# "):
                name, *cells = line[2:].split()
                for cell in cells:
                    placement, count, digest = cell.split(":")
                    pinned["%s %s" % (name, placement)] = (int(count), digest)
                key = None
            else:
                text[key].append(line)
    return pinned, text


def _write_golden(traces):
    with open(GOLDEN, "w") as f:
        for key in FULL_TEXT:
            f.write("@ %s\n%s\n" % (key, "\n".join(traces[key])))
        for name in dict.fromkeys(key.split()[0] for key in traces):
            f.write("# %s %s\n" % (name, " ".join("%s:%d:%s" % (p, len(traces["%s %s" % (name, p)]), _digest(traces["%s %s" % (name, p)])) for p in PLACEMENTS)))


def _run(build_dir):
    return _split(host_harness.run_sanitized(HARNESS, build_dir, ["all"], EXTRA_FLAGS))


@pytest.fixture(scope="module")
def traces(tmp_path_factory):
    return _run(tmp_path_factory.mktemp("linop_trace"))


def test_every_block_is_pinned_in_both_precisions_and_reaches_its_entry_points(traces):
    pinned, text = _read_golden()
    assert sorted(pinned) == sorted(traces) and sorted(text) == sorted(FULL_TEXT)
    names = {key.split()[0] for key in traces}
    assert sorted({name.split(".")[0] for name in names}) == sorted(BLOCKS)
    for name in names:
        assert name[-4:] in (".f32", ".f64") and {name[:-2] + "32", name[:-2] + "64"} <= names
        assert all("%s %s" % (name, p) in traces for p in PLACEMENTS)
    calls = {line.split(" ", 1)[0] for lines in traces.values() for line in lines if not line.startswith("--")}
    for t in ("f32", "f64"):
        for entry in ("grad2d_fwd", "grad2d_adj", "grad3d_fwd", "grad3d_adj", "csr_spmv", "csr_spmv_acc", "pattern_spmv", "pattern_spmv_anchored", "sparse_kron_id",
                      "sparse_kron_id_acc", "id_kron_sparse", "id_kron_sparse_acc", "dense_gemv", "dense_gemv_acc", "dense_kron_id", "dense_kron_id_acc", "id_kron_dense",
                      "id_kron_dense_acc", "linop_dataterm_sublabel", "conv2d", "linop_sym_gradient2d", "conv2d_strided", "radon2d", "sample2d", "fft2d", "wavelet2d",
                      "linop_tensor_gradient2d", "diags_fwd", "diags_adj", "scale", "negate"):
            assert "%s_%s" % (entry, t) in calls, (entry, t)
    # the sparse matrices take the paths they are named for, in both directions
    for t in ("f32", "f64"):
        for name, entry in (("sparse.random5x7", "csr_spmv"), ("sparse.difference300", "pattern_spmv"), ("sparse.pairs300x600", "pattern_spmv_anchored"),
                            ("sparse.empty4x6", "csr_spmv")):
            for p in PLACEMENTS:
                products = {l.split(" ", 1)[0] for l in traces["%s.%s %s" % (name, t, p)] if " res=" in l and " rhs=" in l}
                expected = {"%s_%s" % (entry, t)} | ({"%s_acc_%s" % (entry, t)} if entry == "csr_spmv" else set())      # (the pattern products take a flag)
                assert products == expected, (name, p, products)
    # every guard fires, for K and for K^T, with and without accumulation; the other blocks have none
    for key, lines in traces.items():
        block = key.split(".")[0].split()[0]
        thrown = [l for l in lines if l.startswith("-- EXCEPTION")]
        if block in GUARDS and not key.startswith("sparse.empty"):
            assert thrown == ["-- EXCEPTION %s used before Initialize()." % GUARDS[block]] * 4, (key, thrown)
        else:
            assert not thrown, (key, thrown)


@pytest.mark.parametrize("block", BLOCKS)
def test_product_traces_equal_the_pinned_ones(traces, block):
    pinned, text = _read_golden()
    keys = [key for key in pinned if key.split(".")[0].split()[0] == block]
    assert keys
    failures = []
    for key in keys:
        got = traces[key]
        if key in text and got != text[key]:
            want = text[key]
            at = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
            failures.append("%s: first difference in line %d\n  now:    %s\n  pinned: %s" % (key, at + 1, got[at] if at < len(got) else "<end>", want[at] if at < len(want) else "<end>"))
        elif (len(got), _digest(got)) != pinned[key]:
            failures.append("%s: %d lines with digest %s, pinned: %d lines with digest %s (run the harness with the scenario's name, here and on the pinned commit, to see both traces)"
                            % (key, len(got), _digest(got), pinned[key][0], pinned[key][1]))
    assert not failures, "\n".join(failures)


if __name__ == "__main__":
    if sys.argv[1:] != ["--regenerate"]:
        sys.exit("usage: python tests/test_linop_product_trace.py --regenerate")
    _write_golden(_run(tempfile.mkdtemp()))
    print("wrote", GOLDEN, os.path.getsize(GOLDEN), "bytes")
