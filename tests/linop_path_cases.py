"""Case tables of the directed parity tests of prost_amd/csrc/kernels_linop.hip (helper of test_gpu_linop_paths.py and
test_linop_path_cases.py; not a test).

kernels_linop.hip picks one of several kernels per call from the shape, the pointer alignment and the mean row length.  The tables
below hold, per dispatch path, the smallest shapes that select it, and this module restates the three dispatch rules (with their
source lines) so that the CPU test can assert that every path has a case; the GPU test runs the cases against the oracle.  The
restatements document coverage: they are never used to form an expected value."""
import numpy as np

DTYPES = [np.float32, np.float64]
K_BLOCK = 256                                   # common.hpp: kBlock


def vec(dtype):
    """elements in the 16 bytes of a lane (fused_common.hpp: VecOf<T>::N)"""
    return 16 // np.dtype(dtype).itemsize


def ceil_div(a, b):
    return -(-a // b)


# ---------------------------------------------------------------------------------------------
# 1. gradient: (nx, ny, L, label_first) -> columns per workgroup
# ---------------------------------------------------------------------------------------------
GRAD_SHAPES = [
    (2053, 8, 12, False),        # cols 12: ceil(2053 / 12) * 12 = 2064 workgroups, the last chunk is one column
    (12287, 8, 1, False),        # cols 6: 12 gives 1024 workgroups, 6 gives 2048; the last chunk is 5 columns
    (6143, 4, 1, False),         # cols 3: one active lane in fp32, two in fp64; the last chunk is 2 columns
    (383, 1028, 8, False),       # cols 3: two strips in fp32, three in fp64, the last one 4 rows; strip seams and chunk seams together
    (24565, 2, 2, True),         # cols 12: label-first 2-D, runs of ny L = 4; the last chunk is one column
    (6143, 3, 4, True),          # cols 3: label-first 2-D, runs of 12
    (37, 12, 2, False),          # cols 1: the column march degenerates to one column per workgroup (what the other suites run)
    (37, 3, 4, True),            # cols 1, label-first
]
GRAD_COLS = [12, 6, 3, 3, 12, 3, 1, 1]          # what each shape is in the table for, in both precisions
GRAD_UNALIGNED = [0, 4]                         # run once more one element into their buffers: the scalar kernels


def pick_grad_cols(nx, strips, L):
    for c in (12, 6, 3):                        # kernels_linop.hip:313-316
        if strips * ceil_div(nx, c) * L >= 2048:
            return c
    return 1


def grad_path(shape, dtype, d3, aligned=True):
    """(kernel family, cols) launch_grad chooses: "vec" (planar), "lf_vec" (label-first 2-D) or "scalar" """
    nx, ny, L, lf = shape
    V = vec(dtype)
    if not lf and ny % V == 0 and aligned:                              # kernels_linop.hip:322-325
        return "vec", pick_grad_cols(nx, ceil_div(ny, K_BLOCK * V), L)
    if lf and not d3 and (ny * L) % V == 0 and aligned:                 # kernels_linop.hip:335-337
        return "lf_vec", pick_grad_cols(nx, ceil_div(ny * L, K_BLOCK * V), 1)
    return "scalar", None


def grad_last_chunk(nx, cols):
    return nx - (ceil_div(nx, cols) - 1) * cols


# ---------------------------------------------------------------------------------------------
# 2. diags: name -> (nrows, ncols, offsets)
# ---------------------------------------------------------------------------------------------
BAND = [-3, -1, 0, 2, 5]


def wide_band():
    """40 offsets over [-700, 700], both ends included: more than 16 diagonals, fewer than 8192 workgroups"""
    rng = np.random.default_rng(40)
    inner = rng.choice(np.arange(-699, 700), 38, replace=False)
    return sorted(int(o) for o in np.concatenate(([-700, 700], inner)))


def grid_stride_n(dtype):
    """(8192 + 3) full workgroup passes and 5 more rows: with more than 16 diagonals the grid is capped at 8192 workgroups, so the first
    four take a second pass: two interior ones, a whole one within 8 rows of the end and a ragged one of 5 rows"""
    return (8192 + 3) * K_BLOCK * vec(dtype) + 5


def diags_cases(dtype):
    n = grid_stride_n(dtype)
    return {
        "banded_square": (5000, 5003, BAND),
        "banded_tall": (5000, 3000, BAND),              # forward rows run out of columns
        "banded_wide": (3000, 5000, BAND),              # the adjoint quirk cuts limit to 3072
        "wide_band": (6000, 6000, wide_band()),
        "grid_stride": (n, n, list(range(-8, 9))),
        "one_row": (1, 4099, [0, 1]),
        "one_column": (4099, 1, [-1, 0]),
    }


DIAGS_BANDED = ["banded_square", "banded_tall", "banded_wide"]      # an interior and a border pass each, every dtype and direction
DIAGS_NAMES = ["banded_square", "banded_tall", "banded_wide", "wide_band", "grid_stride", "one_row", "one_column"]


def diags_passes(nrows, ncols, offsets, dtype, adjoint, quirk=False):
    """(workgroups, [interior? per workgroup pass in order of base]) of diags_vec_kernel for a 16-byte aligned result"""
    V = vec(dtype)
    span = K_BLOCK * V
    omin, omax = min(offsets), max(offsets)
    limit = ncols if adjoint else nrows
    if adjoint and quirk:
        limit = min(limit, ceil_div(nrows, 256) * 256)                  # kernels_linop.hip:480
    grid = min(max(ceil_div(ceil_div(limit, V), K_BLOCK), 1), 1 << 20)  # kernels_linop.hip:484, common.hpp:66-71
    if len(offsets) > 16 and grid > 8192:
        grid = 8192                                                     # kernels_linop.hip:485
    passes = []
    for base in range(0, limit, span):
        lo, hi = base, base + span - 1
        if adjoint:                                                     # kernels_linop.hip:430-431
            inside = lo - omax >= 0 and hi - omin < nrows
        else:
            inside = lo + omin >= 0 and hi + omax < ncols
        passes.append(hi < limit and inside)
    return grid, passes


# ---------------------------------------------------------------------------------------------
# 3. CSR: matrices whose mean row length selects the lane count for certain
# ---------------------------------------------------------------------------------------------
CSR_ROWS, CSR_COLS = 700, 900
CSR_CONSTANT = [1, 6, 7, 24, 25, 96, 97]        # 1 | 6: one lane, 7 | 24: 4, 25 | 96: 16, 97: 64
# Lengths of the long rows of the two ragged matrices: 1 and 3 modulo 16 (so neither a multiple of 16 nor of 4).  They stay below about
# 330 entries because of the margin test_linop_path_cases.py asserts in fp32: the allowance of a row grows with the square of its length,
# and a single term (at least 0.25 in magnitude) has to stay more than ten times larger.  Twelve rows of 225 / 227 take ALL the 2424
# entries removed from the r = 24 matrix (its mean stays 24 exactly); eight rows of 289 / 291 take 1552 of the 9696 removed from the
# r = 96 one, the rest is dropped (its mean falls to 84.4, still in the 16-lane bracket).
CSR_RAGGED = {24: [225, 227] * 6, 96: [289, 291] * 4}
# rows alternating (short, long): a lane group whose row is shorter than LANES next to one that takes several strides; mean (a + b) / 2
CSR_SHORT_LONG = [(2, 46), (3, 189), (5, 195)]                  # means 24 | 96 | 100: 4 | 16 | 64 lanes
CSR_SINGLE_ROW = [5, 200]                                       # nrows = 1: one lane | 64 lanes
CSR_NAMES = (["r%d" % r for r in CSR_CONSTANT] + ["ragged%d" % r for r in CSR_RAGGED] + ["short%d_long%d" % p for p in CSR_SHORT_LONG] +
             ["single_row%d" % r for r in CSR_SINGLE_ROW])


def csr_lanes(nnz, nrows):
    mean = nnz / nrows                          # kernels_linop.hip:732
    if mean <= 6.0:                             # kernels_linop.hip:734-737
        return 1
    if mean <= 24.0:
        return 4
    if mean <= 96.0:
        return 16
    return 64


def _signed(rng, n):
    """magnitudes uniform in [0.5, 2] with random signs (so a product is at least 0.25 in magnitude)"""
    return rng.uniform(0.5, 2.0, n) * rng.choice([-1.0, 1.0], n)


def _from_lengths(rng, lengths, ncols, dtype):
    ptr = np.zeros(len(lengths) + 1, np.int32)
    ptr[1:] = np.cumsum(lengths)
    ind = np.concatenate([np.sort(rng.choice(ncols, int(n), replace=False)) for n in lengths] + [np.zeros(0, np.int64)]).astype(np.int32)
    return _signed(rng, int(ptr[-1])).astype(dtype), ptr, ind


def _ragged(rng, r, ncols, dtype):
    """the constant matrix of row length r with every 7th row and the last row emptied (so the first row is empty too) and the removed
    entries moved into the long rows of CSR_RAGGED[r], as far as those have room"""
    val, ptr, ind = _from_lengths(rng, [r] * CSR_ROWS, ncols, dtype)
    rows = [(ind[ptr[i]:ptr[i + 1]], val[ptr[i]:ptr[i + 1]]) for i in range(CSR_ROWS)]
    emptied = [i for i in range(CSR_ROWS) if i % 7 == 0 or i == CSR_ROWS - 1]
    pool = np.concatenate([rows[i][1] for i in emptied])
    kept = [i for i in range(CSR_ROWS) if i not in set(emptied)]
    long_rows = [kept[(k + 1) * len(kept) // (len(CSR_RAGGED[r]) + 1)] for k in range(len(CSR_RAGGED[r]))]
    for i in emptied:
        rows[i] = (ind[:0], val[:0])
    used = 0
    for i, n in zip(long_rows, CSR_RAGGED[r]):
        extra = n - r
        free = np.setdiff1d(np.arange(ncols, dtype=np.int32), rows[i][0])
        cols = np.concatenate([rows[i][0], rng.choice(free, extra, replace=False).astype(np.int32)])
        vals = np.concatenate([rows[i][1], pool[used:used + extra]])
        order = np.argsort(cols, kind="stable")
        rows[i] = (cols[order], vals[order])
        used += extra
    lengths = [len(c) for c, _ in rows]
    out_ptr = np.zeros(CSR_ROWS + 1, np.int32)
    out_ptr[1:] = np.cumsum(lengths)
    return np.concatenate([v for _, v in rows]).astype(dtype), out_ptr, np.concatenate([c for c, _ in rows]).astype(np.int32)


def csr_case(name, dtype):
    """name -> dict(val, ptr, ind, x, base, nrows, ncols): a CSR matrix with sorted column indices without repeats in a row, an operand
    and a result to accumulate onto, all in `dtype`"""
    rng = np.random.default_rng(sum(name.encode()) + 1000 * vec(dtype))
    nrows, ncols = CSR_ROWS, CSR_COLS
    if name.startswith("ragged"):
        val, ptr, ind = _ragged(rng, int(name[6:]), ncols, dtype)
    elif name.startswith("single_row"):
        nrows = 1
        val, ptr, ind = _from_lengths(rng, [int(name[10:])], ncols, dtype)
    elif name.startswith("short"):
        a, b = (int(s) for s in name[5:].split("_long"))
        val, ptr, ind = _from_lengths(rng, [a, b] * (nrows // 2), ncols, dtype)
    else:
        val, ptr, ind = _from_lengths(rng, [int(name[1:])] * nrows, ncols, dtype)
    return dict(val=val, ptr=ptr, ind=ind, nrows=nrows, ncols=ncols, x=_signed(rng, ncols).astype(dtype),
                base=rng.standard_normal(nrows).astype(dtype))


def csr_terms(case, base):
    """per row: (the sum base + sum_j v_j x_j in float64 from the stored values, sum_j |v_j x_j| + |base|, the row length,
    the smallest |v_j x_j| or inf for an empty row)"""
    v = case["val"].astype(np.float64) * case["x"].astype(np.float64)[case["ind"]]
    ptr = case["ptr"].astype(np.int64)
    n = np.diff(ptr)
    row_of = np.repeat(np.arange(case["nrows"]), n)
    base = np.asarray(base, dtype=np.float64)
    total = base + np.bincount(row_of, weights=v, minlength=case["nrows"])
    mass = np.abs(base) + np.bincount(row_of, weights=np.abs(v), minlength=case["nrows"])
    smallest = np.full(case["nrows"], np.inf)
    np.minimum.at(smallest, row_of, np.abs(v))
    return total, mass, n, smallest


def csr_allowance(case, base, dtype):
    """|got - ref| per row for a product summed in ANY order: (n_r + 1) eps (sum_j |v_j x_j| + |base_r|), the standard forward bound of
    n_r rounded products, n_r - 1 additions among them and one addition of the base, with eps = 2 u for slack.  fp32 compares with the
    float64 sum of the same stored values (exact to 2^-53, nothing next to 2^-23); fp64 compares with the oracle's sequential sum,
    which is itself within the bound of the exact value, hence twice the bound."""
    _, mass, n, _ = csr_terms(case, base)
    bound = (n + 1) * float(np.finfo(dtype).eps) * mass
    return bound if np.dtype(dtype) == np.float32 else 2 * bound
