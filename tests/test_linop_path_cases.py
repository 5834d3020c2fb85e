"""CPU check of tests/linop_path_cases.py: the case tables of test_gpu_linop_paths.py select the dispatch paths of
prost_amd/csrc/kernels_linop.hip they claim to.  linop_path_cases.py restates the three dispatch rules (pick_grad_cols, the lane
brackets of launch_csr, the `interior` predicate of diags_vec_kernel) with their source lines.  This documents coverage and does not
replace the GPU comparison: when somebody moves a threshold in the kernels, it fails only if a table stops covering a path."""
import numpy as np
import pytest

import linop_path_cases as cases

DTYPES = cases.DTYPES


@pytest.mark.parametrize("dtype", DTYPES)
def test_gradient_shapes_cover_every_column_count(dtype):
    seen = set()
    for shape, want in zip(cases.GRAD_SHAPES, cases.GRAD_COLS):
        nx, ny, L, lf = shape
        family, cols = cases.grad_path(shape, dtype, d3=False)
        assert family == ("lf_vec" if lf else "vec") and cols == want, (shape, family, cols)
        if not lf:
            assert cases.grad_path(shape, dtype, d3=True) == ("vec", want), shape
        seen.add((family, cols))
        print(np.dtype(dtype).name, shape, family, "cols", cols, "last chunk", cases.grad_last_chunk(nx, cols))
    assert {c for f, c in seen if f == "vec"} == {12, 6, 3, 1}
    assert {c for f, c in seen if f == "lf_vec"} == {12, 3, 1}
    # what the table says about the single shapes
    assert [cases.grad_last_chunk(s[0], c) for s, c in zip(cases.GRAD_SHAPES[:6], cases.GRAD_COLS)] == [1, 5, 2, 2, 1, 2]
    V = cases.vec(dtype)
    assert cases.ceil_div(4, V) == (1 if dtype == np.float32 else 2)                        # active lanes of (6143, 4, 1)
    strips = cases.ceil_div(1028, cases.K_BLOCK * V)
    assert strips == (2 if dtype == np.float32 else 3) and 1028 - (strips - 1) * cases.K_BLOCK * V == 4
    for i in cases.GRAD_UNALIGNED:                                                          # one element into the buffers: the scalar kernels
        assert cases.grad_path(cases.GRAD_SHAPES[i], dtype, d3=False, aligned=False) == ("scalar", None)
        assert cases.GRAD_SHAPES[i][0] <= 65535                                             # which take nx as a grid dimension


@pytest.mark.parametrize("dtype", DTYPES)
def test_diags_cases_cover_interior_border_and_second_passes(dtype):
    table = cases.diags_cases(dtype)
    assert list(table) == cases.DIAGS_NAMES
    for name, (nrows, ncols, offsets) in table.items():
        for adjoint, quirk in ((False, False), (True, False), (True, True)):
            grid, passes = cases.diags_passes(nrows, ncols, offsets, dtype, adjoint, quirk)
            interior = [k for k, p in enumerate(passes) if p]
            print(np.dtype(dtype).name, name, "adjoint" if adjoint else "forward", "quirk" if quirk else "", "workgroups", grid, "passes",
                  len(passes), "interior", (interior[0], interior[-1]) if interior else None)
            if name in cases.DIAGS_BANDED or name == "grid_stride":
                assert any(passes) and not all(passes), (name, adjoint, quirk)
            if name == "grid_stride":
                assert len(offsets) > 16 and grid == 8192 and len(passes) == 8192 + 4      # four workgroups take a second pass ...
                assert passes[8192] and passes[8193] and not passes[8194] and not passes[8195]   # ... two interior, one within 8 rows of the end, the ragged one
                assert nrows - 8195 * cases.K_BLOCK * cases.vec(dtype) == 5
            else:
                assert len(passes) <= grid                                                 # no second pass elsewhere
            if name in ("one_row", "one_column"):
                assert not any(passes)
    nrows, ncols, offsets = table["wide_band"]
    assert len(offsets) == 40 and len(set(offsets)) == 40 and min(offsets) == -700 and max(offsets) == 700
    if dtype == np.float64:
        for adjoint in (False, True):
            passes = cases.diags_passes(nrows, ncols, offsets, dtype, adjoint)[1]
            assert any(passes) and not all(passes)
    # the adjoint quirk cuts the columns of the wide banded case to 3072
    assert len(cases.diags_passes(3000, 5000, cases.BAND, dtype, True, True)[1]) == cases.ceil_div(3072, cases.K_BLOCK * cases.vec(dtype))


@pytest.mark.parametrize("dtype", DTYPES)
def test_csr_cases_cover_every_lane_count_with_a_margin(dtype):
    lanes = {}
    for name in cases.CSR_NAMES:
        c = cases.csr_case(name, dtype)
        ptr, ind = c["ptr"], c["ind"]
        n = np.diff(ptr)
        assert ptr[0] == 0 and len(ptr) == c["nrows"] + 1 and len(ind) == ptr[-1] == len(c["val"]) and c["val"].dtype == dtype
        for r in range(c["nrows"]):
            cols = ind[ptr[r]:ptr[r + 1]]
            assert np.all(np.diff(cols) > 0) and (len(cols) == 0 or (cols[0] >= 0 and cols[-1] < c["ncols"]))   # sorted, no repeats
        assert np.all(np.abs(c["val"]) >= 0.5) and np.all(np.abs(c["val"]) <= 2) and np.all(np.abs(c["x"]) >= 0.5) and np.all(np.abs(c["x"]) <= 2)
        lanes[name] = cases.csr_lanes(int(ptr[-1]), c["nrows"])
        print(np.dtype(dtype).name, name, "mean", float(ptr[-1]) / c["nrows"], "lanes", lanes[name], "row lengths", int(n.min()), "..", int(n.max()))
        # one dropped, doubled or misplaced term cannot hide in the allowance
        for base in (c["base"], np.zeros(c["nrows"], dtype)):
            _, _, _, smallest = cases.csr_terms(c, base)
            allowance = cases.csr_allowance(c, base, dtype)
            assert np.all(smallest[n > 0] > 10 * allowance[n > 0]), (name, float((smallest[n > 0] / allowance[n > 0]).min()))
    assert [lanes["r%d" % r] for r in cases.CSR_CONSTANT] == [1, 1, 4, 4, 16, 16, 64]
    assert lanes["ragged24"] == 4 and lanes["ragged96"] == 16                       # the mean stays in the bracket of the matrix it was cut from
    assert [lanes["short%d_long%d" % p] for p in cases.CSR_SHORT_LONG] == [4, 16, 64]
    assert lanes["single_row5"] == 1 and lanes["single_row200"] == 64
    assert set(lanes.values()) == {1, 4, 16, 64}
    for r, longs in cases.CSR_RAGGED.items():
        c = cases.csr_case("ragged%d" % r, dtype)
        n = np.diff(c["ptr"])
        assert n[0] == 0 and n[-1] == 0 and np.all(n[::7] == 0) and np.count_nonzero(n == 0) == 101
        assert sorted(n[(n != 0) & (n != r)].tolist()) == sorted(longs)
        assert all(m % 16 in (1, 3) and m % 4 != 0 for m in longs) and {m % 16 for m in longs} == {1, 3}
    assert int(np.diff(cases.csr_case("ragged24", dtype)["ptr"]).sum()) == 24 * cases.CSR_ROWS   # every removed entry found a place
    for a, b in cases.CSR_SHORT_LONG:                                              # a row shorter than its lane group, one that is no multiple of it
        L_ = lanes["short%d_long%d" % (a, b)]
        assert 0 < a < L_ and b > L_ and b % L_ != 0
