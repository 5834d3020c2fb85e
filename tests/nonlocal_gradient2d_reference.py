"""References for prost.block.nonlocal_gradient2d (no code of the block is used here):

  (a) matrix(nx, ny, L, offsets, planes, dtype): the explicit scipy matrix K, M L N x L N.  Row (m, c, p) holds -w_m[p] at column
      c N + p and +w_m[p] at column c N + q, q = p + dy_m + dx_m ny, only where (y + dy_m, x + dx_m) lies in the grid (the term is
      present); the planes are rounded to dtype once, a weight of zero is no entry;
  (b) product: both directions of include/prost/linop/nonlocal_gradient2d.hpp restated on NumPy arrays of a given dtype (every NumPy
      operation on arrays of one dtype rounds once in that dtype, and there is no contraction), with explicit masks -- np.where selects,
      nothing is multiplied by a mask -- in the stated order: forward one subtraction and one product; the adjoint starts s = +0 and
      visits m ascending, the outgoing term s - w_m[p] y_m[p] first, then the incoming term s + w_m[p'] y_m[p'], every product rounded on
      its own; the accumulating form is res0 + value;
  (c) sums: the row / column sums of |entries of (a)|^alpha in fp64;
  bound: gamma_n B componentwise, B = |K| |x| forward and |K|^T |y| for the adjoint (p != q and the offsets are distinct, so no two terms
      merge and |K| holds the unmerged absolute values), gamma_n = n u / (1 - n u), n = 2 forward and 2 M for the adjoint, for the
      block and for a CSR twin in dtype alike; against such a twin the two add.  The derivation is in the header.

Grid: N = nx ny, pixel (y, x) at p = y + x ny.  Domain: u_c[p] at c N + p.  Range: plane (m, c) at (m L + c) N + p.  Offsets are (dy, dx)
pairs; weights are a list of M planes of N values.
"""
import numpy as np
import scipy.sparse as sp

MAX_OFFSETS, MAX_REACH = 64, 15


def roundings(M, transpose):
    """the n of gamma_n for the block and for a CSR twin (the same count)"""
    return 2 * M if transpose else 2


def sum_terms(M):
    """the longest sum of |entry|^alpha (a column): the t of (t + 8) eps_T"""
    return 2 * M


def inside(nx, ny, dy, dx):
    """[x, y] boolean: (y + dy, x + dx) lies in the grid"""
    x, y = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    return (y + dy >= 0) & (y + dy < ny) & (x + dx >= 0) & (x + dx < nx)


def rounded(planes, dtype):
    """the planes rounded to dtype once, as float64 vectors"""
    return [np.asarray(p, dtype=np.float64).reshape(-1).astype(dtype).astype(np.float64) for p in planes]


def matrix(nx, ny, L, offsets, planes, dtype=np.float64):
    """(a): csc, float64 entries from the planes rounded to dtype; a zero is no entry"""
    N, M = nx * ny, len(offsets)
    assert len(planes) == M
    rows, cols, vals = [], [], []
    p = np.arange(N)
    for m, ((dy, dx), w) in enumerate(zip(offsets, rounded(planes, dtype))):
        here = p[inside(nx, ny, dy, dx).reshape(-1)]
        for c in range(L):
            r = (m * L + c) * N + here
            rows += [r, r]
            cols += [c * N + here, c * N + here + dy + dx * ny]
            vals += [-w[here], w[here]]
    K = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(M * L * N, L * N)).tocsc()
    K.eliminate_zeros()
    K.sort_indices()
    return K


def _shift(a, dx, dy):
    """a[..., x + dx, y + dy]; cells outside the grid hold a NaN that a mask must select away"""
    out = np.full_like(a, np.nan)
    nx, ny = a.shape[-2:]
    if abs(dx) >= nx or abs(dy) >= ny:
        return out
    xs, xd = (slice(dx, nx), slice(0, nx - dx)) if dx >= 0 else (slice(0, nx + dx), slice(-dx, nx))
    ys, yd = (slice(dy, ny), slice(0, ny - dy)) if dy >= 0 else (slice(0, ny + dy), slice(-dy, ny))
    out[..., xd, yd] = a[..., xs, ys]
    return out


def product(x, nx, ny, L, offsets, planes, transpose, dtype, res0=None):
    """(b): K x (transpose: K^T x) in dtype, or res0 + that"""
    dtype = np.dtype(dtype).type
    M = len(offsets)
    w = [np.asarray(p, dtype=np.float64).reshape(-1).astype(dtype).reshape(1, nx, ny) for p in planes]
    v = np.asarray(x).astype(dtype)
    zero = np.zeros((L, nx, ny), dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        if not transpose:
            u = v.reshape(L, nx, ny)
            out = np.stack([np.where(inside(nx, ny, dy, dx), w[m] * (_shift(u, dx, dy) - u), zero) for m, (dy, dx) in enumerate(offsets)])
        else:
            y = v.reshape(M, L, nx, ny)
            out = zero.copy()
            for m, (dy, dx) in enumerate(offsets):
                prod = w[m] * y[m]
                out = np.where(inside(nx, ny, dy, dx), out - prod, out)                         # outgoing: the term of p itself
                out = np.where(inside(nx, ny, -dy, -dx), out + _shift(prod, -dx, -dy), out)      # incoming: the term of p' = p - d
    assert out.dtype == np.dtype(dtype)
    out = out.reshape(-1)
    return out if res0 is None else np.asarray(res0).astype(dtype) + out


def gradient_product(x, nx, ny, L, dtype):
    """gradient2d(nx, ny, L) forward restated (grad_fwd_kernel): no weights anywhere"""
    dtype = np.dtype(dtype).type
    u = np.asarray(x).astype(dtype).reshape(L, nx, ny)
    zero = np.zeros((L, nx, ny), dtype)
    with np.errstate(invalid="ignore"):
        return np.stack([np.where(inside(nx, ny, 0, 1), _shift(u, 1, 0) - u, zero), np.where(inside(nx, ny, 1, 0), _shift(u, 0, 1) - u, zero)]).reshape(-1)


def sums(nx, ny, L, offsets, planes, alpha=1.0, dtype=np.float64):
    """(c): sum |entry|^alpha of every row and every column of (a), in fp64 -> (rows, cols)"""
    K = abs(matrix(nx, ny, L, offsets, planes, dtype))
    K.data = K.data ** float(alpha)
    return np.asarray(K.sum(axis=1)).ravel(), np.asarray(K.sum(axis=0)).ravel()


def magnitude(nx, ny, L, offsets, planes, transpose, x, dtype):
    """B: |K| |x|, or |K|^T |x| for the transpose, with the planes rounded to dtype"""
    K = abs(matrix(nx, ny, L, offsets, planes, dtype))
    ab = np.abs(np.asarray(x, dtype=np.float64))
    return K.T @ ab if transpose else K @ ab


def gamma(n, dtype):
    u = np.finfo(dtype).eps / 2
    return n * u / (1 - n * u)


def bound(nx, ny, L, offsets, planes, transpose, x, dtype, twin=False):
    """gamma_n B for the block against the exact product; twin: against a CSR twin in dtype, gamma_block B + gamma_twin B"""
    g = gamma(roundings(len(offsets), transpose), dtype)
    return (2 * g if twin else g) * magnitude(nx, ny, L, offsets, planes, transpose, x, dtype)


# ---- the constants of include/prost/linop/nonlocal_gradient2d.hpp and of the kernels' dispatch ----
TILE_Y, TILE_X, THREADS, MAX_PASS, LDS_LIMIT = 64, 16, 256, 4, 65536
VEC = {np.dtype(np.float32): 4, np.dtype(np.float64): 2}
PASS_CHANNELS = {4: (4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 3), 8: (4, 4, 4, 4, 4, 4, 3, 3, 3, 2, 2, 2, 2, 2, 2, 1)}


def tile_values(ry, rx):
    return (TILE_Y + 2 * ry) * (TILE_X + 2 * rx)


def reach(offsets):
    return max(max(abs(dy), abs(dx)) for dy, dx in offsets)


def pass_channels(offsets, dtype):
    return PASS_CHANNELS[np.dtype(dtype).itemsize][reach(offsets)]


# ---- offsets ----
def window(radius):
    """the full window in the documented order of prost.block.nonlocal_window: dx ascending, inside it dy ascending, no (0, 0)"""
    return [(dy, dx) for dx in range(-radius, radius + 1) for dy in range(-radius, radius + 1) if (dy, dx) != (0, 0)]


OFFSETS = {
    "grad": [(0, 1), (1, 0)],
    "w1": window(1),
    "w2": window(2),                                                    # the full radius-2 window, M = 24
    "far": [(15, 0), (-15, 0), (0, 15), (0, -15), (4, -4), (-4, 4), (15, 15), (-15, -15), (-4, 0), (0, 4)],     # reach 15: the smallest pass
    "one": [(2, -3)],                                                   # M = 1
    "m64": window(4)[:64],                                              # M = 64
    "pos": [(1, 0), (0, 1), (2, 3), (5, 1)],                            # one-sided
    "neg": [(-1, 0), (0, -1), (-2, -3), (-5, -1)],
}

# ny, nx, L, offsets.  From the constants: a tile is 64 x 16 pixels, so 63 / 64 / 65 / 129 rows and 15 / 16 / 17 / 33 columns are each tile
# side - 1, + 0, + 1 and twice + 1; a lane of the vector path holds 4 (fp32) or 2 (fp64) rows, so 66 rows are vector rows in fp64 only
# and every odd height takes the element kernels; a pass at reach 15 holds 3 channels in fp32 and 1 in fp64, so L = 4 is one more than
# a pass in fp32 and four passes in fp64, and L = 5 at reach 1 is one more than the pass of 4.
CASES = [
    (1, 1, 1, "w1"),                 # every term is masked
    (1, 7, 1, "w1"), (5, 1, 1, "w1"),
    (5, 3, 1, "far"), (5, 3, 3, "far"),      # a grid smaller than the reach: +-15 never lands, +-4 sometimes
    (63, 5, 1, "w1"), (64, 15, 1, "w1"), (65, 16, 1, "grad"), (129, 17, 1, "w1"), (8, 33, 3, "w2"), (66, 4, 1, "pos"),
    (20, 18, 1, "one"), (20, 18, 2, "m64"),
    (12, 16, 3, "w2"),
    (17, 19, 1, "pos"), (17, 19, 1, "neg"), (16, 20, 3, "neg"),
    (24, 20, 4, "far"), (16, 9, 5, "w1"),
]


def case_id(case):
    return "%dx%dx%d_%s" % case


def case_seed(case, salt=0):
    ny, nx, L, off = case
    return 23 + salt + 13 * ny + 1009 * nx + 100003 * L + 7 * len(OFFSETS[off])


def is_dyadic(case):
    """the cases whose product tests use dyadic weights (every sum of |entries| exact)"""
    return (case[0] + case[1]) % 2 == 0


def dyadic_weights(nx, ny, M, seed):
    """multiples of 1/8 in [-1, 1], zeros included"""
    rng = np.random.default_rng(seed)
    return [rng.integers(-8, 9, nx * ny).astype(np.float64) / 8 for _ in range(M)]


def random_weights(nx, ny, M, seed):
    """normal weights of either sign, one in eight exactly zero"""
    rng = np.random.default_rng(seed)
    return [rng.standard_normal(nx * ny) * (rng.integers(0, 8, nx * ny) > 0) for _ in range(M)]


def ones_weights(nx, ny, M):
    return [np.ones(nx * ny) for _ in range(M)]


def weights_for(case, salt=0):
    ny, nx, _, off = case
    M = len(OFFSETS[off])
    return dyadic_weights(nx, ny, M, case_seed(case, 50 + salt)) if is_dyadic(case) else random_weights(nx, ny, M, case_seed(case, 50 + salt))
