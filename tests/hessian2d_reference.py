"""References for prost.block.hessian2d (no code of the block is used here):

  (a) matrix(nx, ny, L, w, components, dtype): the explicit scipy matrix H = E @ G, with G = spmat_gradient2d(nx, ny, L) (the project's
      forward differences, the layout of gradient2d) and E = sym_gradient2d_reference.matrix(nx, ny, L, w, dtype) (w rounded to dtype
      once); components = 3: the rows of E, (hxx, hyy, hxy) planes; components = 4: the planes (hxx, hxy, hxy, hyy), the mixed rows
      twice;
  (b) product: the two marches of include/prost/linop/hessian2d.hpp restated on NumPy arrays of a given dtype (every NumPy operation
      on arrays of one dtype rounds once in that dtype, and there is no contraction), with explicit masks -- np.where selects, nothing
      is multiplied by a mask -- and the stated order: the inner differences are rounded once and are +0 where masked, an outer sum
      starts from +0 and adds its present terms left to right, every product w a is rounded on its own, grad^T is
      divx = (ax) vx, (bx) - vx[p-ny]; divy = (ay) vy, (by) - vy[p-1]; 0 - (divx + divy); the accumulating forms are res0 + value
      forward and res0 - (divx + divy) in the adjoint;
  (c) sums: the row / column sums of |entries of (a)|^alpha in fp64.

Grid: N = nx ny, pixel (y, x) at p = y + x ny.  Domain: u_c[p] at c N + p.  Range: plane k of channel c at (k L + c) N + p.
"""
import os
import sys

import numpy as np
import scipy.sparse as sp

import sym_gradient2d_reference as S
from sym_gradient2d_reference import W_FROB, W_HALF, case_id, case_seed, masks, weight  # noqa: F401  (shared with the tests)

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))

ROUNDINGS_FORWARD = 6           # inner difference, product, four additions: the k of the bound 1.01 k u (|H| |x|)
ROUNDINGS_ADJOINT = 7           # product and four additions, divx or divy, divx + divy; one more for components = 4 (e_xy + e_yx)
SUM_TERMS = 7                   # the longest row of (a): the sums are held to (SUM_TERMS + 8) eps_T


def planes(components):
    """the planes of E's range (0 hxx, 1 hyy, 2 hxy) in the order of the block's range"""
    assert components in (3, 4)
    return (0, 1, 2) if components == 3 else (0, 2, 2, 1)


def matrix(nx, ny, L=1, w=W_FROB, components=3, dtype=np.float64):
    """(a): csc, float64 entries (w rounded to dtype); a zero is no entry"""
    from multilabel_fast import spmat_gradient2d
    N = nx * ny
    G = sp.csr_matrix(spmat_gradient2d(nx, ny, L))
    assert G.shape == (2 * L * N, L * N)
    H3 = sp.csr_matrix(S.matrix(nx, ny, L, w, dtype) @ G)
    H = sp.vstack([H3[k * L * N:(k + 1) * L * N] for k in planes(components)], format="csc")
    H.eliminate_zeros()
    H.sort_indices()
    assert H.shape == (components * L * N, L * N)
    return H


def product(x, nx, ny, L, w, components, transpose, dtype, res0=None):
    """(b): H x (transpose: H^T x) in dtype, or the accumulating form on res0"""
    dtype = np.dtype(dtype).type
    wt = dtype(w)
    ax, bx, ay, by = masks(nx, ny)
    v = np.asarray(x).astype(dtype)
    zero = np.zeros((L, nx, ny), dtype)
    add, shift = S._add, S._shift
    with np.errstate(invalid="ignore", over="ignore"):
        if not transpose:
            u = v.reshape(L, nx, ny)                                # [c, x, y]
            gx = np.where(ax, shift(u, 1, 0) - u, zero)
            gy = np.where(ay, shift(u, 0, 1) - u, zero)
            hxx = add(add(zero, bx, shift(gx, -1, 0), -1), ax, gx, +1)
            hyy = add(add(zero, by, shift(gy, 0, -1), -1), ay, gy, +1)
            hxy = add(zero, by, wt * shift(gx, 0, -1), -1)
            hxy = add(hxy, ay, wt * gx, +1)
            hxy = add(hxy, bx, wt * shift(gy, -1, 0), -1)
            hxy = add(hxy, ax, wt * gy, +1)
            out = np.stack([(hxx, hyy, hxy)[k] for k in planes(components)]).reshape(-1)
            assert out.dtype == np.dtype(dtype)
            return out if res0 is None else np.asarray(res0).astype(dtype) + out
        e = v.reshape(components, L, nx, ny)
        exx, eyy, exy = (e[0], e[1], e[2]) if components == 3 else (e[0], e[3], e[1] + e[2])
        vx = add(add(zero, ax, exx, +1), ax, shift(exx, 1, 0), -1)
        vx = add(add(vx, ay, wt * exy, +1), ay, wt * shift(exy, 0, 1), -1)
        vy = add(add(zero, ay, eyy, +1), ay, shift(eyy, 0, 1), -1)
        vy = add(add(vy, ax, wt * exy, +1), ax, wt * shift(exy, 1, 0), -1)
        divx = np.where(ax, vx, zero)
        divx = np.where(bx, divx - shift(vx, -1, 0), divx)
        divy = np.where(ay, vy, zero)
        divy = np.where(by, divy - shift(vy, 0, -1), divy)
        s = (divx + divy).reshape(-1)
        assert s.dtype == np.dtype(dtype)
        return (np.zeros_like(s) if res0 is None else np.asarray(res0).astype(dtype)) - s


def sums(nx, ny, L, w, components=3, alpha=1.0, dtype=np.float64):
    """(c): sum |entry|^alpha of every row and every column of (a), in fp64 -> (rows, cols)"""
    H = abs(matrix(nx, ny, L, w, components, dtype))
    H.data = H.data ** float(alpha)
    return np.asarray(H.sum(axis=1)).ravel(), np.asarray(H.sum(axis=0)).ravel()


def roundings(components, transpose):
    return ROUNDINGS_FORWARD if not transpose else ROUNDINGS_ADJOINT + (1 if components == 4 else 0)


def bound(nx, ny, L, w, components, transpose, x, dtype):
    """1.01 k u (|H| |x|): the derived forward error bound of include/prost/linop/hessian2d.hpp, u the unit roundoff"""
    H = abs(matrix(nx, ny, L, w, components, dtype))
    M = H.T if transpose else H
    return 1.01 * roundings(components, transpose) * (np.finfo(dtype).eps / 2) * (M @ np.abs(np.asarray(x, dtype=np.float64)))


# the constants of include/prost/linop/hessian2d.hpp (those of sym_gradient2d.hpp) and of the kernels' dispatch
# (prost_amd/csrc/kernels_linop_hessian2d.hip)
BLOCK, VEC, COLUMN_CHOICES, FILL_BLOCKS = S.BLOCK, S.VEC, S.COLUMN_CHOICES, S.FILL_BLOCKS
strip_rows, pick_columns = S.strip_rows, S.pick_columns

# ny, nx, L.  Sides 1, 2, 3 in every combination: every row of the matrix is a boundary row
TINY = [(ny, nx, 1) for ny in (1, 2, 3) for nx in (1, 2, 3)] + [(2, 3, 3), (3, 3, 3)]
# odd heights (the element kernels in both precisions), a height that is a multiple of 2 only (fp64 vector, fp32 element)
ODD = [(5, 7, 1), (17, 13, 3), (66, 5, 1)]
# one row below, at and one row above one strip of the vector path (lanes x W rows; fp64: 512, fp32: 1024), and one vector more
STRIPS = [(strip_rows(t) + d, nx, 1) for t in (np.float64, np.float32) for d, nx in ((-1, 3), (0, 3), (1, 2))] + [(514, 3, 1), (1028, 2, 3)]
# a chunk of c = 12, 6 or 3 columns is picked only when FILL_BLOCKS workgroups remain: at one strip and one channel that is
# ceil(nx / c) >= 2048, so nx = 2047 c is one below the choice (the next one is taken), 2047 c + 1 is at it (2047 full chunks and one
# of a single column), 2048 c is the smallest grid of full chunks of c columns and one column more adds a chunk of a single column
CHUNKS = [(4, nx, 1) for c in COLUMN_CHOICES[::-1] for nx in ((FILL_BLOCKS - 1) * c, (FILL_BLOCKS - 1) * c + 1, FILL_BLOCKS * c, FILL_BLOCKS * c + 1)] + [(8, 4097, 3)]
CASES = TINY + ODD + STRIPS + CHUNKS
# (components, w): the Frobenius layout with its default weight, the matrix layout with the true Hessian's, a negative weight
VARIANTS = [(3, W_FROB), (4, W_HALF), (4, -1.3)]
