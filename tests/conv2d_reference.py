"""References for prost.block.conv2d (no code of the block is used here):

  (a) matrix(nx, ny, L, kernel, shape): the explicit scipy matrix, L my mx x L ny nx, holding the dtype-rounded window; for "full" it is
      kron(eye(L), convmtx2(kernel, ny, nx)) of examples/deblurring.py entry for entry;
  (b) product: the march of include/prost/linop/conv2d.hpp restated operation for operation on NumPy arrays of a given dtype (every
      NumPy operation on arrays of one dtype rounds once in that dtype, and there is no contraction): zero taps dropped, the others by
      ascending source index (j from kx - 1 down to 0, inside that i from ky - 1 down to 0), out-of-range source cells as zeros, the sum
      started from the first term, the accumulating form res0 + value; the adjoint is the same march with the window flipped, the
      plane sizes exchanged and the offsets mirrored;
  (c) sums: the row / column sums of |entries of (a)|^alpha in fp64.

Images are ny x nx, column-major: element (y, x, c) at y + x ny + c nx ny.
"""
import numpy as np
import scipy.sparse as sp

SHAPES = ("full", "same", "valid")


def output_size(nx, ny, ky, kx, shape):
    """-> (my, mx), (oy, ox)"""
    return {"full": ((ny + ky - 1, nx + kx - 1), (0, 0)),
            "same": ((ny, nx), (ky // 2, kx // 2)),
            "valid": ((ny - ky + 1, nx - kx + 1), (ky - 1, kx - 1))}[shape]


def window(kernel, dtype=np.float64):
    """the window as a ky x kx array rounded to dtype"""
    k = np.atleast_2d(np.asarray(kernel, dtype=np.float64)).astype(dtype)
    assert k.ndim == 2
    return k


def taps(kernel, dtype=np.float64):
    """the number of non-zero taps after rounding to dtype"""
    return int(np.count_nonzero(window(kernel, dtype)))


def matrix(nx, ny, L, kernel, shape, dtype=np.float64):
    """(a): csc, float64 entries holding the dtype-rounded window; a zero tap is no entry"""
    k = window(kernel, dtype).astype(np.float64)
    ky, kx = k.shape
    (my, mx), (oy, ox) = output_size(nx, ny, ky, kx, shape)
    assert my >= 1 and mx >= 1
    sy, sx = np.mgrid[0:ny, 0:nx]
    rows, cols, vals = [], [], []
    for j in range(kx):
        for i in range(ky):
            if k[i, j] == 0:
                continue
            y, x = sy + i - oy, sx + j - ox              # the output that tap (i, j) carries source (sy, sx) to
            ok = (y >= 0) & (y < my) & (x >= 0) & (x < mx)
            rows.append((y + x * my)[ok]); cols.append((sy + sx * ny)[ok]); vals.append(np.full(int(ok.sum()), k[i, j]))
    one = sp.csc_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(my * mx, ny * nx))
    K = sp.kron(sp.identity(L), one, format="csc")
    K.eliminate_zeros()
    K.sort_indices()
    assert K.shape == (L * my * mx, L * ny * nx)
    return K


def direction(nx, ny, kernel, shape, transpose, dtype):
    """-> window of the direction (flipped for the adjoint), (sny, snx), (dny, dnx), (oy, ox)"""
    k = window(kernel, dtype)
    ky, kx = k.shape
    (my, mx), (oy, ox) = output_size(nx, ny, ky, kx, shape)
    if not transpose:
        return k, (ny, nx), (my, mx), (oy, ox)
    return k[::-1, ::-1], (my, mx), (ny, nx), (ky - 1 - oy, kx - 1 - ox)


def product(x, nx, ny, L, kernel, shape, transpose, dtype, res0=None):
    """(b): K x (transpose: K^T x) in dtype, or res0 + that"""
    k, (sny, snx), (dny, dnx), (oy, ox) = direction(nx, ny, kernel, shape, transpose, dtype)
    ky, kx = k.shape
    src = np.asarray(x).astype(dtype).reshape(L, snx, sny)                   # [c, x, y]
    # every source cell an output can ask for, out-of-range cells as zeros: cell (ly, lx) is source (ly + oy - (ky - 1), lx + ox - (kx - 1))
    cells = np.zeros((L, dnx + kx - 1, dny + ky - 1), dtype)
    ly0, lx0 = ky - 1 - oy, kx - 1 - ox                                      # the cell of source (0, 0)
    y_lo, y_hi = max(0, -ly0), min(sny, dny + ky - 1 - ly0)
    x_lo, x_hi = max(0, -lx0), min(snx, dnx + kx - 1 - lx0)
    if y_hi > y_lo and x_hi > x_lo:
        cells[:, lx0 + x_lo:lx0 + x_hi, ly0 + y_lo:ly0 + y_hi] = src[:, x_lo:x_hi, y_lo:y_hi]
    acc = None
    for j in range(kx - 1, -1, -1):
        for i in range(ky - 1, -1, -1):
            if k[i, j] == 0:
                continue
            term = k[i, j] * cells[:, kx - 1 - j:kx - 1 - j + dnx, ky - 1 - i:ky - 1 - i + dny]
            acc = term if acc is None else acc + term
    assert acc is not None and acc.dtype == np.dtype(dtype)
    out = acc.reshape(-1)
    return out if res0 is None else np.asarray(res0).astype(dtype) + out


def sums(nx, ny, L, kernel, shape, alpha=1.0, dtype=np.float64):
    """(c): sum |entry|^alpha of every row and every column of (a), in fp64 -> (rows, cols)"""
    K = abs(matrix(nx, ny, L, kernel, shape, dtype)).power(float(alpha))
    return np.asarray(K.sum(axis=1)).ravel(), np.asarray(K.sum(axis=0)).ravel()


def bound(nx, ny, L, kernel, shape, transpose, x, dtype):
    """1.01 (t + 1) u (|K| |x|): the forward error bound of a t-term sum of rounded products in any order, u the unit roundoff"""
    K = abs(matrix(nx, ny, L, kernel, shape, dtype))
    M = K.T if transpose else K
    return 1.01 * (taps(kernel, dtype) + 1) * (np.finfo(dtype).eps / 2) * (M @ np.abs(np.asarray(x, dtype=np.float64)))


PITCH = 94          # PROST_HIP_CONV2D_PITCH of include/prost_hip.h


def abi_records(nx, ny, L, kernel, shape, transpose, dtype):
    """one direction as include/prost_hip.h describes it for prost_hip_conv2d_*: the nine int32 of the geometry record, the tap table
    as int32 words ({ offset, value } in fp32, { offset, reserved, value } in fp64) and the tap count"""
    k, (sny, snx), (dny, dnx), (oy, ox) = direction(nx, ny, kernel, shape, transpose, dtype)
    ky, kx = k.shape
    rec = np.dtype([("offset", np.int32), ("value", np.float32)] if np.dtype(dtype) == np.float32 else
                   [("offset", np.int32), ("reserved", np.int32), ("value", np.float64)])
    table = [((ky - 1 - i) + (kx - 1 - j) * PITCH, k[i, j]) for j in range(kx - 1, -1, -1) for i in range(ky - 1, -1, -1) if k[i, j] != 0]
    t = np.zeros(len(table), rec)
    t["offset"] = [o for o, _ in table]
    t["value"] = [v for _, v in table]
    return np.array([sny, snx, dny, dnx, oy, ox, ky, kx, L], np.int32), t.view(np.int32).copy(), len(table)


def motion_window():
    """the 15 x 15 motion window of examples/deblurring.py (about 29 non-zero taps)"""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))
    from deblurring import motion_kernel
    return motion_kernel(15, 45.0)


# image ny x nx, L, window ky x kx (None: the motion window), shapes
CASES = [
    (1, 1, 1, (1, 1), SHAPES),
    (1, 7, 1, (1, 3), SHAPES),
    (5, 1, 1, (3, 1), SHAPES),
    (3, 3, 1, (5, 5), ("full", "same")),          # the window is larger than the image
    (17, 13, 3, (2, 2), SHAPES),                  # even window, odd plane size
    (17, 13, 3, (4, 5), SHAPES),
    (64, 16, 1, (3, 3), SHAPES),                  # exactly one tile of 64 x 16 for "same", more than one for "full"
    (65, 17, 1, (3, 3), SHAPES),                  # one past the tile in both axes
    (130, 35, 3, None, SHAPES),
    (40, 33, 1, (31, 31), SHAPES),
]


def case_id(case):
    ny, nx, L, win, _ = case
    return "%dx%dx%d-%s" % (ny, nx, L, "motion" if win is None else "%dx%d" % win)


def case_window(case):
    """standard normal, seeded from the shape; the motion window as it is"""
    ny, nx, L, win, _ = case
    if win is None:
        return motion_window()
    rng = np.random.default_rng(1000003 * ny + 10007 * nx + 101 * L + 31 * win[0] + win[1])
    return rng.standard_normal(win)


def case_seed(case, salt=0):
    ny, nx, L, win, _ = case
    ky, kx = (15, 15) if win is None else win
    return 7 + salt + 13 * ny + 1009 * nx + 100003 * L + 17 * ky + 29 * kx
