"""References for prost.block.sym_gradient2d (no code of the block is used here):

  (a) matrix(nx, ny, L, w, dtype): the explicit scipy matrix, 3 L N x 2 L N, from the project's spmat_gradient2d(nx, ny, 1): with Dx, Dy
      its two N x N halves, Bx = -Dx^T, By = -Dy^T,
          E = [ kron(I_L, Bx)  0 ; 0  kron(I_L, By) ; w kron(I_L, By)  w kron(I_L, Bx) ],  w rounded to dtype once;
  (b) product: the marches of include/prost/linop/sym_gradient2d.hpp restated on NumPy arrays of a given dtype (every NumPy operation
      on arrays of one dtype rounds once in that dtype, and there is no contraction), with explicit masks -- np.where selects, nothing
      is multiplied by a mask -- and the stated order: a sum starts from +0, its present terms are added left to right, every product
      w a is rounded on its own, the accumulating form is res0 + value;
  (c) sums: the row / column sums of |entries of (a)|^alpha in fp64.

Grid: N = nx ny, pixel (y, x) at p = y + x ny.  Domain: vx_c[p] at c N + p, vy_c[p] at (L + c) N + p.  Range: exx_c[p] at c N + p,
eyy_c[p] at (L + c) N + p, exy_c[p] at (2 L + c) N + p.
"""
import os
import sys

import numpy as np
import scipy.sparse as sp

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))

T_TERMS = 4                     # the longest sum: the t of the bound 1.01 (t + 1) u (|E| |x|)
W_HALF, W_FROB = 0.5, float(np.sqrt(0.5))


def weight(w, dtype):
    """w formed in double and rounded to dtype once, as a float64"""
    return float(np.dtype(dtype).type(w))


def backward_differences(nx, ny):
    """Bx = -Dx^T, By = -Dy^T from spmat_gradient2d(nx, ny, 1)"""
    from multilabel_fast import spmat_gradient2d
    N = nx * ny
    D = sp.csr_matrix(spmat_gradient2d(nx, ny, 1))
    assert D.shape == (2 * N, N)
    return (-D[:N].T).tocsr(), (-D[N:].T).tocsr()


def matrix(nx, ny, L=1, w=W_FROB, dtype=np.float64):
    """(a): csc, float64 entries (w rounded to dtype); a zero is no entry"""
    Bx, By = backward_differences(nx, ny)
    I = sp.identity(L, format="csr")
    wt = weight(w, dtype)
    N = nx * ny
    Z = sp.csr_matrix((L * N, L * N))
    E = sp.bmat([[sp.kron(I, Bx), Z], [Z, sp.kron(I, By)], [wt * sp.kron(I, By), wt * sp.kron(I, Bx)]], format="csc")
    E.eliminate_zeros()
    E.sort_indices()
    assert E.shape == (3 * L * N, 2 * L * N)
    return E


def masks(nx, ny):
    """ax, bx, ay, by as [x, y] boolean arrays"""
    x, y = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    return x < nx - 1, x > 0, y < ny - 1, y > 0


def _shift(a, dx, dy):
    """a[c, x + dx, y + dy]; cells outside the grid hold a NaN that a mask must select away"""
    out = np.full_like(a, np.nan)
    nx, ny = a.shape[1:]
    xs, xd = (slice(dx, nx), slice(0, nx - dx)) if dx >= 0 else (slice(0, nx + dx), slice(-dx, nx))
    ys, yd = (slice(dy, ny), slice(0, ny - dy)) if dy >= 0 else (slice(0, ny + dy), slice(-dy, ny))
    out[:, xd, yd] = a[:, xs, ys]
    return out


def _add(acc, mask, term, sign):
    return np.where(mask, acc - term if sign < 0 else acc + term, acc)


def product(x, nx, ny, L, w, transpose, dtype, res0=None):
    """(b): E x (transpose: E^T x) in dtype, or res0 + that"""
    dtype = np.dtype(dtype).type
    wt = dtype(w)
    ax, bx, ay, by = masks(nx, ny)
    v = np.asarray(x).astype(dtype)
    zero = np.zeros((L, nx, ny), dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        if not transpose:
            vx, vy = v.reshape(2, L, nx, ny)                       # [c, x, y]
            exx = _add(_add(zero, bx, _shift(vx, -1, 0), -1), ax, vx, +1)
            eyy = _add(_add(zero, by, _shift(vy, 0, -1), -1), ay, vy, +1)
            exy = _add(zero, by, wt * _shift(vx, 0, -1), -1)
            exy = _add(exy, ay, wt * vx, +1)
            exy = _add(exy, bx, wt * _shift(vy, -1, 0), -1)
            exy = _add(exy, ax, wt * vy, +1)
            out = np.stack([exx, eyy, exy])
        else:
            exx, eyy, exy = v.reshape(3, L, nx, ny)
            vx = _add(_add(zero, ax, exx, +1), ax, _shift(exx, 1, 0), -1)
            vx = _add(_add(vx, ay, wt * exy, +1), ay, wt * _shift(exy, 0, 1), -1)
            vy = _add(_add(zero, ay, eyy, +1), ay, _shift(eyy, 0, 1), -1)
            vy = _add(_add(vy, ax, wt * exy, +1), ax, wt * _shift(exy, 1, 0), -1)
            out = np.stack([vx, vy])
    assert out.dtype == np.dtype(dtype)
    out = out.reshape(-1)
    return out if res0 is None else np.asarray(res0).astype(dtype) + out


def sums(nx, ny, L, w, alpha=1.0, dtype=np.float64):
    """(c): sum |entry|^alpha of every row and every column of (a), in fp64 -> (rows, cols)"""
    E = abs(matrix(nx, ny, L, w, dtype))
    E.data = E.data ** float(alpha)
    return np.asarray(E.sum(axis=1)).ravel(), np.asarray(E.sum(axis=0)).ravel()


def bound(nx, ny, L, w, transpose, x, dtype):
    """1.01 (t + 1) u (|E| |x|), t = 4: the forward error bound of a t-term sum of rounded products, u the unit roundoff"""
    E = abs(matrix(nx, ny, L, w, dtype))
    M = E.T if transpose else E
    return 1.01 * (T_TERMS + 1) * (np.finfo(dtype).eps / 2) * (M @ np.abs(np.asarray(x, dtype=np.float64)))


def empty_columns(nx, ny, L, w=W_HALF):
    """the domain elements whose column of (a) holds no entry"""
    E = matrix(nx, ny, L, w)
    return np.flatnonzero(np.diff(E.indptr) == 0)


# the constants of include/prost/linop/sym_gradient2d.hpp and of the kernels' dispatch (prost_amd/csrc/kernels_linop_sym_gradient2d.hip)
BLOCK = 256                                     # lanes of a workgroup
VEC = {np.dtype(np.float32): 4, np.dtype(np.float64): 2}
COLUMN_CHOICES, FILL_BLOCKS = (12, 6, 3), 2048


def strip_rows(dtype):
    """the rows of one strip of the vector path"""
    return BLOCK * VEC[np.dtype(dtype)]


def pick_columns(nx, ny, L, dtype):
    """the columns of a chunk as the dispatch picks them (vector path)"""
    strips = -(-ny // strip_rows(dtype))
    for c in COLUMN_CHOICES:
        if strips * -(-nx // c) * L >= FILL_BLOCKS:
            return c
    return 1


# ny, nx, L
SMALL = [(1, 1, 1), (1, 7, 1), (5, 1, 1), (2, 2, 1), (3, 3, 2), (17, 13, 3), (66, 5, 1)]
# one strip of the vector path and one row more, per precision (fp32: 1024 rows, fp64: 512); a chunk of 12, 6 or 3 columns is only
# picked when 2048 workgroups remain, so "exactly one chunk width of columns per workgroup, every chunk full" is nx = 2048 c at one
# strip and one channel, and "one column more" adds a last chunk of a single column
STRIPS = [(512, 3, 1), (513, 3, 1), (514, 3, 1), (1024, 3, 1), (1025, 3, 1), (1028, 2, 2)]
CHUNKS = [(4, 2048 * 3, 1), (4, 2048 * 3 + 1, 1), (4, 2048 * 6, 1), (4, 2048 * 6 + 1, 1), (4, 2048 * 12, 1), (4, 2048 * 12 + 1, 1), (8, 4097, 3)]
CASES = SMALL + STRIPS + CHUNKS


def case_id(case):
    return "%dx%dx%d" % case


def case_seed(case, salt=0):
    ny, nx, L = case
    return 11 + salt + 13 * ny + 1009 * nx + 100003 * L
