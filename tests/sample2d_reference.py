"""References for prost.block.sample2d, written from the definition (the issue text and the comment at the head of
include/prost/linop/sample2d.hpp), never from the code under test.  NumPy and scipy only, vectorised.

Geometry: L column-major planes of ny x nx, element (yy, xx, c) at yy + xx ny + c nx ny; L planes of M samples, sample i of plane c at
i + c M.  Positions are float64, rounded once to T.  With fx, fy in T: j0 = floor(fx), ax = fx - j0, bx = 1 - ax, likewise i0, ay, by;
slot 0: by bx at (i0, j0), slot 1: ay bx at (i0 + 1, j0), slot 2: by ax at (i0, j0 + 1), slot 3: ay ax at (i0 + 1, j0 + 1); every
operation one rounding in T.  An entry is absent outside the image or with a weight of exactly 0; a sample with
not (fx >= -1 and fx < nx and fy >= -1 and fy < ny) has none.

  (a) matrix(..)      the matrix in float64 from the T-rounded entries, a scipy CSR
  (b) product(..)     the restatement in T in the pinned order, from +0: forward in slot order; adjoint by cell (yy-1, xx-1), (yy, xx-1),
                      (yy-1, xx), (yy, xx) -- the pixel is slot 3, 2, 1, 0 of the samples of these cells -- and by ascending sample
                      index inside a cell.  Both run over the ENTRY LIST of the forward enumeration, so the adjoint here knows nothing
                      of bucket tables: a sample the buckets lost or doubled would show.
  (c) sums(..)        row and column sums of |entry|^alpha in float64
  (d) bound(..)       1.01 (t + 1) u (|K| |x|) per component, t the number of terms of that row or column -- the forward error bound
                      of a t-term sum of rounded products, each product of two roundings, in any order
  (e) buckets(..)     the adjoint's tables from the definition (a stable sort by cell), for the tests that call the C entry points
"""
import functools

import numpy as np
import scipy.sparse as sp

ONE_CELL_SAMPLES = 300


def special_values(n):
    """positions along an axis of n pixels that must each occur: integers (0, n - 1), exactly -1, inside (-1, 0) and (n - 1, n), exactly n
    and 2^-10 past either end (just outside; exact in fp32), +-1e30, and two interior fractions"""
    return [0.0, float(n - 1), -1.0, -0.5, -0.25, n - 0.5, n - 0.75, float(n), -1.0 - 2.0 ** -10, n + 2.0 ** -10, 1e30, -1e30,
            min(0.5, n - 1.0), (n - 1) * 0.375, (n - 1) / 2.0]


def positions(kind, ny, nx, m, seed):
    """-> (x, y) float64 of the case's samples"""
    rng = np.random.default_rng(seed)
    N = nx * ny
    if kind == "integers":                      # the pixel grid itself, column-major: K = I
        idx = np.arange(N)
        return (idx // ny).astype(np.float64), (idx % ny).astype(np.float64)
    if kind == "flow":                          # a smooth flow of at most 5 pixels, the shape of synthetic.warp_matrix
        idx = np.arange(N)
        py, px = idx % ny, idx // ny
        dx = 4.5 * np.sin(2 * np.pi * 1.5 * px / nx) * np.cos(2 * np.pi * py / ny)
        dy = 4.5 * np.cos(2 * np.pi * px / nx) * np.sin(2 * np.pi * 2.0 * py / ny)
        return px + dx, py + dy
    if kind == "onecell":                       # every sample inside cell (ny // 2, nx // 2): all other cells are empty
        return nx // 2 + rng.uniform(0.01, 0.99, m), ny // 2 + rng.uniform(0.01, 0.99, m)
    if kind == "random":                        # scattered, a margin of 1.5 pixels around the image
        return rng.uniform(-1.5, nx + 0.5, m), rng.uniform(-1.5, ny + 0.5, m)
    assert kind == "special"                    # the cross product of the special values, then random picks of them
    sx, sy = special_values(nx), special_values(ny)
    i = np.arange(m)
    ix = np.where(i < len(sx) * len(sy), i % len(sx), rng.integers(0, len(sx), m))
    iy = np.where(i < len(sx) * len(sy), (i // len(sx) + i) % len(sy), rng.integers(0, len(sy), m))
    return np.array(sx)[ix], np.array(sy)[iy]


# (ny, nx, L, kind, M (None: nx ny)).  The kernels' units are 64 samples (forward) and 64 rows of one column (adjoint): M = 1, 63, 64, 65,
# 257 and images of 64 and of 65 rows sit on and around them.
CASES = (
    (1, 1, 1, "random", 1),
    (1, 1, 1, "special", 65),
    (1, 7, 2, "special", 63),
    (7, 1, 3, "special", 64),
    (5, 4, 1, "integers", None),
    (65, 3, 2, "integers", None),               # the identity across a wavefront's edge
    (64, 5, 1, "random", 257),                  # exactly one wavefront of rows; M < N
    (65, 6, 2, "special", 257),                 # a row past it; every pair of special values
    (9, 7, 2, "random", 257),                   # M > N
    (7, 10, 1, "onecell", ONE_CELL_SAMPLES),    # 300 samples in one cell
    (33, 70, 1, "flow", None),
    (33, 70, 3, "random", 257),
    (33, 70, 1, "special", 257),
)


def case_id(case):
    ny, nx, L, kind, m = case
    return "%dx%dx%d-%s-M%s" % (ny, nx, L, kind, "N" if m is None else m)


def case_seed(case, salt=0):
    return 1000 * CASES.index(case) + salt


def case_args(case):
    """-> (nx, ny, L, x, y), the arguments of prost.block.sample2d"""
    ny, nx, L, kind, m = case
    x, y = positions(kind, ny, nx, nx * ny if m is None else m, case_seed(case, 7))
    return nx, ny, L, x, y


def _key(nx, ny, x, y, dtype):
    x, y = np.asarray(x, np.float64).ravel(), np.asarray(y, np.float64).ravel()
    return int(nx), int(ny), x.tobytes(), y.tobytes(), np.dtype(dtype).name


@functools.lru_cache(maxsize=64)
def _entries(key):
    """the entry list of one plane in the forward's order -> (rows, cols, vals in T, slots), rows ascending and inside a row slot ascending"""
    nx, ny, xb, yb, name = key
    dtype = np.dtype(name)
    T = dtype.type
    with np.errstate(over="ignore", invalid="ignore"):
        fx, fy = np.frombuffer(xb, np.float64).astype(dtype), np.frombuffer(yb, np.float64).astype(dtype)
        reach = (fx >= T(-1)) & (fx < T(nx)) & (fy >= T(-1)) & (fy < T(ny))
        flx, fly = np.floor(fx), np.floor(fy)
        ax = fx - flx
        bx = T(1) - ax
        ay = fy - fly
        by = T(1) - ay
        w = np.stack([by * bx, ay * bx, by * ax, ay * ax], axis=1)
    assert w.dtype == dtype
    j0 = np.where(reach, flx, 0).astype(np.int64)
    i0 = np.where(reach, fly, 0).astype(np.int64)
    ii = np.stack([i0, i0 + 1, i0, i0 + 1], axis=1)
    jj = np.stack([j0, j0, j0 + 1, j0 + 1], axis=1)
    present = reach[:, None] & (ii >= 0) & (ii < ny) & (jj >= 0) & (jj < nx) & (w != 0)
    rows = np.broadcast_to(np.arange(len(fx))[:, None], w.shape)[present]
    slots = np.broadcast_to(np.arange(4)[None, :], w.shape)[present]
    cols = (ii + jj * ny)[present]
    vals = w[present]
    for v in (rows, cols, vals, slots):
        v.setflags(write=False)
    return rows, cols, vals, slots


def entries(nx, ny, x, y, dtype):
    return _entries(_key(nx, ny, x, y, dtype))


def matrix(nx, ny, L, x, y, dtype=np.float64):
    """(a): L M x L ny nx, float64 values of the T-rounded entries"""
    rows, cols, vals, _ = entries(nx, ny, x, y, dtype)
    one = sp.csr_matrix((vals.astype(np.float64), (rows, cols)), shape=(len(np.ravel(x)), nx * ny))
    K = sp.kron(sp.eye(L), one).tocsr()
    K.sort_indices()
    return K


def _in_order(group, other, vals, x, ngroups, dtype):
    """acc[g] = the sum over the entries of group g, in the order they stand in (a stable sort by group), of vals * x[other], from +0"""
    order = np.argsort(group, kind="stable")
    group, other, vals = group[order], other[order], vals[order]
    count = np.bincount(group, minlength=ngroups)
    start = np.concatenate([[0], np.cumsum(count)])[:-1]
    acc = np.zeros((x.shape[0], ngroups), dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(int(count.max()) if count.size else 0):
            sel = np.nonzero(count > k)[0]
            e = start[sel] + k
            acc[:, sel] = acc[:, sel] + vals[e][None, :] * x[:, other[e]]
    return acc


def product(v, nx, ny, L, x, y, transpose, dtype, res0=None):
    """(b): K v or K^T v in T in the pinned order; res0: the accumulating form, res0 + value"""
    rows, cols, vals, slots = entries(nx, ny, x, y, dtype)
    m, n = len(np.ravel(x)), nx * ny
    if transpose:
        by_cell = np.lexsort((rows, 3 - slots))                # inside a column: slot 3, 2, 1, 0, then ascending sample index
        out = _in_order(cols[by_cell], rows[by_cell], vals[by_cell], np.asarray(v).astype(dtype).reshape(L, m), n, dtype)
    else:
        out = _in_order(rows, cols, vals, np.asarray(v).astype(dtype).reshape(L, n), m, dtype)
    out = out.reshape(-1)
    return out if res0 is None else np.asarray(res0).astype(dtype) + out


def terms(nx, ny, L, x, y, dtype):
    """-> (entries per row, entries per column) of the whole matrix"""
    rows, cols, _, _ = entries(nx, ny, x, y, dtype)
    return np.tile(np.bincount(rows, minlength=len(np.ravel(x))), L), np.tile(np.bincount(cols, minlength=nx * ny), L)


def sums(nx, ny, L, x, y, alpha, dtype):
    """(c): (row sums, column sums) of |entry|^alpha in float64"""
    rows, cols, vals, _ = entries(nx, ny, x, y, dtype)
    v = np.abs(vals.astype(np.float64)) ** alpha
    return np.tile(np.bincount(rows, weights=v, minlength=len(np.ravel(x))), L), np.tile(np.bincount(cols, weights=v, minlength=nx * ny), L)


def bound(nx, ny, L, x, y, transpose, v, dtype):
    """(d): 1.01 (t + 1) u (|K| |v|) per component"""
    K = abs(matrix(nx, ny, L, x, y, dtype))
    t = terms(nx, ny, L, x, y, dtype)[1 if transpose else 0]
    u = np.finfo(dtype).eps / 2
    av = np.abs(np.asarray(v, dtype=np.float64))
    return 1.01 * (t + 1) * u * ((K.T @ av) if transpose else (K @ av))


def buckets(nx, ny, x, y, dtype):
    """(e): -> (order int32 [M], cell_start int32 [(ny + 1)(nx + 1) + 1]): the samples with entries sorted stably by their cell
    (i0 + 1) + (j0 + 1)(ny + 1); the samples without entries stand behind them, ascending"""
    rows, _, _, _ = entries(nx, ny, x, y, dtype)
    m = len(np.ravel(x))
    with np.errstate(over="ignore", invalid="ignore"):
        fx, fy = np.asarray(x, np.float64).ravel().astype(dtype), np.asarray(y, np.float64).ravel().astype(dtype)
    has = np.bincount(rows, minlength=m) > 0
    cell = np.full(m, (ny + 1) * (nx + 1), np.int64)
    cell[has] = (np.floor(fy[has]).astype(np.int64) + 1) + (np.floor(fx[has]).astype(np.int64) + 1) * (ny + 1)
    order = np.argsort(cell, kind="stable").astype(np.int32)
    count = np.bincount(cell[has], minlength=(ny + 1) * (nx + 1))
    return order, np.concatenate([[0], np.cumsum(count)]).astype(np.int32)


def abi_records(nx, ny, L, m, transpose):
    """the geometry record of prost_hip_sample2d_geometry: int32 { ny, nx, m, planes, transpose, reserved }"""
    return np.array([ny, nx, m, L, 1 if transpose else 0, 0], np.int32)
