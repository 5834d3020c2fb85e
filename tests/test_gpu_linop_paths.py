"""Directed GPU parity tests of every dispatch path of prost_amd/csrc/kernels_linop.hip, at the C ABI (include/prost_hip.h) against the
CPU oracle.  The shapes come from tests/linop_path_cases.py, which also says which kernel each of them selects (checked on the CPU by
test_linop_path_cases.py): the column-marching gradient kernels with 12, 6, 3 and 1 columns per workgroup, the interior passes, the
grid-stride loop and the alignment fallbacks of the multi-diagonal kernels, and the 1-, 4-, 16- and 64-lane CSR kernels.

Bar: bit-exact wherever the kernel sums in the oracle's order (everything but the multi-lane CSR kernels, whose allowance is the
summation bound of linop_path_cases.csr_allowance).  Every call runs accumulating onto random values and not accumulating into a buffer
pre-filled with random values."""
import numpy as np
import pytest

import linop_path_cases as cases
import oracle

pytestmark = pytest.mark.gpu

DTYPES = cases.DTYPES

_KEEP = []


def dev(hip, a):
    """host -> device; the buffer is kept alive until the end of the test (kernels are async)."""
    d = hip.DeviceArray.from_host(a)
    _KEEP.append(d)
    return d


@pytest.fixture(autouse=True)
def _release_device_buffers(request):
    yield
    if "hip" in request.fixturenames:
        request.getfixturevalue("hip").sync()
    for d in _KEEP:
        d.free()
    del _KEEP[:]


def dev_at(hip, a, shift):
    """`a` on the device, `shift` elements into a buffer that is `shift` elements longer: (buffer, pointer to a's first element)"""
    a = np.ascontiguousarray(a)
    buf = np.zeros(a.size + shift, a.dtype)
    buf[shift:] = a
    d = dev(hip, buf)
    return d, d.offset(shift)


def differing(got, ref):
    bad = np.flatnonzero(got != ref)
    return "%d of %d elements differ, first at %d: %r != %r" % (bad.size, got.size, bad[0], got[bad[0]], ref[bad[0]]) if bad.size else "equal"


# ---------------------------------------------------------------------------------------------
# 1. gradient: column marching
# ---------------------------------------------------------------------------------------------
def _gradient(hip, dtype, shape, d3, shift):
    """forward and adjoint with acc 0 and 1 against the oracle; returns the four device results"""
    nx, ny, L, lf = shape
    rng = np.random.default_rng(101)
    n = nx * ny * L
    k = 3 if d3 else 2
    x = rng.standard_normal(n).astype(dtype)
    y = rng.standard_normal(k * n).astype(dtype)
    base_r = rng.standard_normal(k * n).astype(dtype)
    base_c = rng.standard_normal(n).astype(dtype)
    og = oracle.grad3d if d3 else oracle.grad2d
    name = "grad3d" if d3 else "grad2d"
    dx, dy = dev_at(hip, x, shift)[1], dev_at(hip, y, shift)[1]
    out = []
    for acc in (0, 1):
        ref_f = og(x, nx, ny, L, lf, adjoint=False, acc=base_r.copy() if acc else None)
        ref_a = og(y, nx, ny, L, lf, adjoint=True, acc=base_c.copy() if acc else None)
        r, pr = dev_at(hip, base_r, shift)
        c, pc = dev_at(hip, base_c, shift)
        hip.check(hip.fn(name + "_fwd", dtype)(pr, dx, hip.sz(nx), hip.sz(ny), hip.sz(L), int(lf), acc, None))
        hip.check(hip.fn(name + "_adj", dtype)(pc, dy, hip.sz(nx), hip.sz(ny), hip.sz(L), int(lf), acc, None))
        got_f, got_a = r.to_host()[shift:], c.to_host()[shift:]
        assert np.array_equal(got_f, ref_f), ("forward", shape, d3, acc, shift, differing(got_f, ref_f))
        assert np.array_equal(got_a, ref_a), ("adjoint", shape, d3, acc, shift, differing(got_a, ref_a))
        out += [got_f, got_a]
    return out


GRAD_PARAMS = [(s, d3) for s in cases.GRAD_SHAPES for d3 in (False, True) if not (d3 and s[3])]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape,d3", GRAD_PARAMS, ids=["%dx%dx%d%s%s" % (s[0], s[1], s[2], "-lf" if s[3] else "", "-3d" if d3 else "") for s, d3 in GRAD_PARAMS])
def test_gradient_column_march(hip, dtype, shape, d3):
    """grad_{fwd,adj}_vec_kernel and grad_{fwd,adj}_lf_vec_kernel with 12, 6, 3 and 1 columns per workgroup: cur / nxt and prev carried in
    registers from column to column, prev reloaded at a chunk seam, has_next across a seam, a ragged last chunk, strip seams"""
    _gradient(hip, dtype, shape, d3, 0)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("index", cases.GRAD_UNALIGNED)
def test_gradient_one_element_into_its_buffers(hip, dtype, index):
    """res and rhs one element into their buffers: the launcher falls back to the scalar kernels, whose results equal the oracle's and
    those of the 16-bytes-per-lane kernels bit for bit"""
    shape = cases.GRAD_SHAPES[index]
    for d3 in ((False,) if shape[3] else (False, True)):
        aligned = _gradient(hip, dtype, shape, d3, 0)
        shifted = _gradient(hip, dtype, shape, d3, 1)
        for a, s in zip(aligned, shifted):
            assert np.array_equal(a, s), (shape, d3, differing(s, a))


# ---------------------------------------------------------------------------------------------
# 2. diags: interior passes, grid stride, alignment
# ---------------------------------------------------------------------------------------------
def _diags(hip, dtype, nrows, ncols, offsets, res_shift=0, rhs_shift=0):
    rng = np.random.default_rng(202)
    nd = len(offsets)
    ofs, fac = oracle.diags_sort(rng.permutation(np.asarray(offsets)), rng.random(nd), dtype)
    x = rng.standard_normal(ncols).astype(dtype)
    y = rng.standard_normal(nrows).astype(dtype)
    base_r = rng.standard_normal(nrows).astype(dtype)
    base_c = rng.standard_normal(ncols).astype(dtype)
    d_ofs, d_fac = dev(hip, ofs), dev(hip, fac)
    r, pr = dev_at(hip, base_r, res_shift)
    hip.check(hip.fn("diags_fwd", dtype)(pr, dev_at(hip, x, rhs_shift)[1], hip.sz(nrows), hip.sz(ncols), hip.sz(nd), d_ofs.ptr, d_fac.ptr, None))
    got, ref = r.to_host()[res_shift:], oracle.diags(x, nrows, ncols, ofs, fac, acc=base_r.copy())
    assert np.array_equal(got, ref), ("forward", differing(got, ref))
    out = [got]
    dy = dev_at(hip, y, rhs_shift)[1]
    for quirk in (0, 1):
        c, pc = dev_at(hip, base_c, res_shift)
        hip.check(hip.fn("diags_adj", dtype)(pc, dy, hip.sz(nrows), hip.sz(ncols), hip.sz(nd), d_ofs.ptr, d_fac.ptr, quirk, None))
        got, ref = c.to_host()[res_shift:], oracle.diags(y, nrows, ncols, ofs, fac, adjoint=True, ref_grid_quirk=bool(quirk), acc=base_c.copy())
        assert np.array_equal(got, ref), ("adjoint", quirk, differing(got, ref))
        out.append(got)
    return out


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", cases.DIAGS_NAMES)
def test_diags_paths(hip, dtype, name):
    """diags_vec_kernel onto a random result: passes that are interior (one unaligned 16-byte load per diagonal, no bounds tests) next to
    border passes, operands that run out of columns / rows, the adjoint grid quirk, more than 16 diagonals, the grid-stride loop with a
    ragged last pass, one row, one column"""
    nrows, ncols, offsets = cases.diags_cases(dtype)[name]
    _diags(hip, dtype, nrows, ncols, offsets)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shifted", ["res", "rhs"])
def test_diags_one_element_into_a_buffer(hip, dtype, shifted):
    """res one element into its buffer: the scalar diags_kernel runs; only rhs: the vector kernel still runs, its loads through
    UnalignedVec.  Both equal the oracle and the aligned call bit for bit."""
    nrows, ncols, offsets = cases.diags_cases(dtype)["banded_square"]
    aligned = _diags(hip, dtype, nrows, ncols, offsets)
    moved = _diags(hip, dtype, nrows, ncols, offsets, res_shift=int(shifted == "res"), rhs_shift=int(shifted == "rhs"))
    for a, m in zip(aligned, moved):
        assert np.array_equal(a, m), differing(m, a)


# ---------------------------------------------------------------------------------------------
# 3. CSR: every lane count, both entry points
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("entry", ["csr_spmv", "csr_spmv_acc"])
@pytest.mark.parametrize("name", cases.CSR_NAMES)
def test_csr_lanes(hip, dtype, entry, name):
    """csr_spmv_kernel<T, 1 | 4 | 16 | 64, ACC>: constant row lengths on both sides of the thresholds 6 / 24 / 96, empty rows, rows that
    are no multiple of the lane count, rows shorter than it, a single row.  One lane: the oracle's sum bit for bit.  More lanes: per
    row within (n_r + 1) eps (sum |v_j x_j| + |base_r|) of the float64 sum (fp32) or twice that of the oracle's (fp64) -- an
    allowance more than ten times smaller than any single term (test_linop_path_cases.py)."""
    c = cases.csr_case(name, dtype)
    acc = entry == "csr_spmv_acc"
    base = c["base"] if acc else np.zeros(c["nrows"], dtype)
    r = dev(hip, c["base"])                     # not accumulating: the random values have to be overwritten
    hip.check(hip.fn(entry, dtype)(r.ptr, dev(hip, c["x"]).ptr, hip.sz(c["nrows"]), hip.sz(len(c["val"])), dev(hip, c["val"]).ptr,
                                   dev(hip, c["ptr"]).ptr, dev(hip, c["ind"]).ptr, None))
    got = r.to_host()
    seq = oracle.csr_spmv_acc(base.copy(), c["x"], c["val"], c["ptr"], c["ind"])
    lanes = cases.csr_lanes(len(c["val"]), c["nrows"])
    if lanes == 1:
        assert np.array_equal(got, seq), (name, differing(got, seq))
        return
    ref = cases.csr_terms(c, base)[0] if dtype == np.float32 else seq.astype(np.float64)
    err = np.abs(got.astype(np.float64) - ref)
    allowance = cases.csr_allowance(c, base, dtype)
    worst = int(np.argmax(err - allowance))
    print(name, np.dtype(dtype).name, entry, "lanes", lanes, "largest error / allowance", float(np.max(err / np.maximum(allowance, np.finfo(np.float64).tiny))))
    assert np.all(err <= allowance), "row %d (%d entries): |%r - %r| = %g > %g" % (worst, c["ptr"][worst + 1] - c["ptr"][worst], got[worst], ref[worst], err[worst], allowance[worst])
    empty = np.diff(c["ptr"]) == 0
    assert np.array_equal(got[empty], base[empty])


# ---------------------------------------------------------------------------------------------
# 4. through the product path
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec,dtype", [("single", np.float32), ("double", np.float64)])
def test_eval_linop_blocks_at_odd_rows_and_columns(hip, prec, dtype):
    """prost.eval_linop == oracle.eval_linop bit for bit on a 2 x 2 arrangement

        [ diags(1, 5003)        diags(1, 197088)        ]      row 0
        [ diags(5000, 5003)     gradient2d(2053, 8, 12) ]      from row 1; the second block column starts at column 5003

    The host library hands res + row and rhs + col of the assembled vectors to the kernels, so the sub-buffers of the two large blocks are
    NOT 16-byte aligned here.  Forward, both results start at row 1: the scalar diags_kernel and the scalar gradient kernel run.
    Transposed, the banded block writes columns from 0 (aligned) and reads its operand from row 1: diags_vec_kernel with interior passes
    through UnalignedVec; the gradient writes from column 5003: the scalar adjoint.  (The reference's adjoint grid of the diags block,
    which the oracle's operator keeps and the product leaves off, changes nothing here: the one-row blocks reach columns 0 and 1 only.)"""
    import prost_amd as prost
    prost.set_gpu(0)
    prost.set_precision(prec)
    try:
        rng = np.random.default_rng(404)
        nx, ny, L = cases.GRAD_SHAPES[0][:3]
        nr, nc, band = cases.diags_cases(dtype)["banded_square"]
        ng = nx * ny * L
        fac, top0, top1 = rng.random(len(band)), rng.random(2), rng.random(2)
        linop = [prost.block.diags(1, nc, top0, [0, 1])(0, 0, 1, nc)[0],
                 prost.block.diags(nr, nc, fac, band)(1, 0, nr, nc)[0],
                 prost.block.gradient2d(nx, ny, L)(1, nc, 2 * ng, ng)[0],
                 prost.block.diags(1, ng, top1, [0, 1])(0, nc, 1, ng)[0]]
        nrows, ncols = 1 + 2 * ng, nc + ng
        assert nc % 2 == 1
        inp, inp_t = rng.standard_normal(ncols), rng.standard_normal(nrows)
        x = np.asarray(prost.eval_linop(linop, inp, False)[0]).ravel()
        ox = oracle.eval_linop(linop, inp, False, dtype)[0]
        assert x.shape == (nrows,) and np.array_equal(x, ox), differing(x, ox)
        x_t = np.asarray(prost.eval_linop(linop, inp_t, True)[0]).ravel()
        ox_t = oracle.eval_linop(linop, inp_t, True, dtype)[0]
        assert x_t.shape == (ncols,) and np.array_equal(x_t, ox_t), differing(x_t, ox_t)
    finally:
        prost.set_precision("double")
