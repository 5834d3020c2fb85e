"""References for prost.block.radon2d, written from the definition (the issue text and the comment at the head of
include/prost/linop/radon2d.hpp), never from the code under test.  NumPy and scipy only, vectorised.

Geometry: L column-major planes of ny x nx, element (y, x, c) at y + x ny + c nx ny; L sinograms, bin d of angle a of plane c at
d + a ndet + c ndet na.  Per angle the table { q, p, r, c, axis } is formed in Python floats (IEEE double; cos and sin are libm's, as
in the host library) and rounded once to T.  Position of ray (a, d) on driving line t: f = (r + q d) + p t, every operation one rounding
in T; i0 = floor(f), w1 = f - i0, w0 = 1 - w1; entries c w0 at (t, i0) and c w1 at (t, i0 + 1), absent outside the image or with a
weight of exactly 0.

  (a) matrix(..)      the matrix in float64 from the T-rounded table, a scipy CSR
  (b) product(..)     the restatement in T in the pinned order: forward over t ascending, i0 before i0 + 1; adjoint over angles
                      ascending and bins ascending.  Both run over the ENTRY LIST of the forward enumeration (the adjoint groups it by
                      pixel), so the adjoint here knows nothing of a candidate window: a ray the window missed would show.
  (c) sums(..)        row and column sums of |entry|^alpha in float64
  (d) bound(..)       1.01 (t + 1) u (|K| |x|) per component, t the number of terms of that row or column -- the forward error bound
                      of a t-term sum of rounded products, each product of two roundings, in any order
"""
import functools
import math

import numpy as np
import scipy.sparse as sp

ANGLE_SET = (0.0, math.pi / 4, math.pi / 2, 3 * math.pi / 4, math.pi, -math.pi / 4, 2 * math.pi + 0.1)


def default_ndet(nx, ny, spacing):
    return 2 * int(math.ceil(math.hypot(nx, ny) / (2.0 * spacing))) + 1


def angles_of(kind):
    """'set': the seven special angles; 'set+rand': plus a seeded random dozen; an int n: n angles evenly over [0, pi)"""
    if kind == "set":
        return np.array(ANGLE_SET)
    if kind == "set+rand":
        return np.concatenate([np.array(ANGLE_SET), np.random.default_rng(2306).uniform(-math.pi, 2 * math.pi, 12)])
    return np.arange(int(kind)) * (math.pi / int(kind))


# (ny, nx, L, angles, ndet (None: the default), spacing, shift).  The kernels' units are 64 bins of one angle per wavefront (forward) and
# 64 rows of one column per wavefront (adjoint): ndet 63 / 64 / 65 / 130 and images of 64 and of 65 rows sit on and around them.  At
# a row-driven angle the forward kernel stages slabs of 16 rows by up to 128 columns: the last two cases.
CASES = (
    (1, 1, 1, "set", None, 1.0, 0.0),
    (1, 1, 1, "set", 1, 1.0, 0.3),
    (5, 5, 1, "set+rand", None, 1.0, 0.0),
    (5, 5, 3, "set", 63, 0.5, -0.3),                 # a detector much longer than the image: rays that miss it
    (9, 7, 1, "set+rand", 64, 1.0, 0.3),
    (9, 7, 1, 2, 3, 1.0, 0.0),                       # a detector shorter than the image, two angles: the corners are never seen
    (7, 10, 3, "set+rand", 65, 2.5, 0.0),
    (7, 10, 1, "set", 130, 0.5, 0.3),
    (7, 10, 1, "set", None, 2.5, -0.3),
    (64, 5, 1, "set+rand", None, 1.0, 0.0),          # exactly one wavefront of rows
    (65, 6, 1, "set", None, 0.5, 0.3),               # a row and a column past it
    (150, 131, 1, 97, None, 1.0, 0.0),
    (150, 131, 3, "set", 130, 1.0, -0.3),
    (16, 128, 1, "set", 64, 2.5, 0.0),               # one slab of the forward kernel exactly: 16 rows, 128 columns under 64 bins
    (17, 129, 1, "set", 64, 2.5, 0.0),               # a row and a column past it: a second slab, and one too wide to be staged
)


def cases(dtype=None):
    return CASES


def case_id(case):
    ny, nx, L, kind, ndet, spacing, shift = case
    return "%dx%dx%d-%s-ndet%s-h%g-s%g" % (ny, nx, L, kind, "default" if ndet is None else ndet, spacing, shift)


def case_args(case):
    """-> (nx, ny, L, angles, ndet, spacing, shift), the arguments of prost.block.radon2d with ndet resolved"""
    ny, nx, L, kind, ndet, spacing, shift = case
    return nx, ny, L, angles_of(kind), default_ndet(nx, ny, spacing) if ndet is None else ndet, spacing, shift


def case_seed(case, salt=0):
    return 1000 * CASES.index(case) + salt


def table(nx, ny, angles, ndet, spacing, shift, dtype):
    """-> (na, 5) array of T: q, p, r, c, axis"""
    T = np.dtype(dtype).type
    cx, cy, cd, h = (nx - 1) / 2.0, (ny - 1) / 2.0, (ndet - 1) / 2.0, float(spacing)
    shift = float(shift)
    out = np.zeros((len(angles), 5), dtype)
    for a, theta in enumerate(angles):
        co, si = math.cos(float(theta)), math.sin(float(theta))
        if abs(co) >= abs(si):
            row = (h / co, -si / co, ((shift - cd * h) + cy * si) / co + cx, 1 / abs(co), 0.0)
        else:
            row = (h / si, -co / si, ((shift - cd * h) + cx * co) / si + cy, 1 / abs(si), 1.0)
        out[a] = [T(v) for v in row]
    return out


def _key(nx, ny, angles, ndet, spacing, shift, dtype):
    return (int(nx), int(ny), tuple(float(a) for a in np.asarray(angles, np.float64).ravel()), int(ndet), float(spacing), float(shift), np.dtype(dtype).name)


@functools.lru_cache(maxsize=64)
def _entries(key):
    """the entry list of one plane in the forward's order -> (rows, cols, vals in T), rows ascending and inside a row t ascending, i0 first"""
    nx, ny, angles, ndet, spacing, shift, name = key
    dtype = np.dtype(name)
    T = dtype.type
    tab = table(nx, ny, angles, ndet, spacing, shift, dtype)
    rows, cols, vals = [], [], []
    d = np.arange(ndet)
    for a in range(len(angles)):
        q, p, r, c, axis = (T(v) for v in tab[a])
        column = axis != 0
        nt, ni = (nx, ny) if column else (ny, nx)
        t = np.arange(nt)
        base = r + q * d.astype(dtype)                                    # one product, one sum
        f = base[:, None] + (p * t.astype(dtype))[None, :]
        assert f.dtype == dtype
        fl = np.floor(f)
        w1 = f - fl
        w0 = T(1) - w1
        possible = (fl >= -1) & (fl < ni)
        i0 = np.where(possible, fl, -2).astype(np.int64)
        tt = np.broadcast_to(t[None, :], f.shape)
        dd = np.broadcast_to(d[:, None], f.shape)
        slot_i = np.stack([i0, i0 + 1], axis=2)
        slot_w = np.stack([w0, w1], axis=2)
        assert slot_w.dtype == dtype
        present = possible[:, :, None] & (slot_i >= 0) & (slot_i < ni) & (slot_w != 0)
        value = c * slot_w
        assert value.dtype == dtype
        t3 = np.broadcast_to(tt[:, :, None], slot_i.shape)
        pixel = np.where(column, slot_i + t3 * ny, t3 + slot_i * ny)         # y + x ny
        row = np.broadcast_to((a * ndet + dd)[:, :, None], slot_i.shape)
        rows.append(row[present])
        cols.append(pixel[present])
        vals.append(value[present])
    rows, cols, vals = np.concatenate(rows), np.concatenate(cols), np.concatenate(vals)
    for v in (rows, cols, vals):
        v.setflags(write=False)
    return rows, cols, vals


def entries(nx, ny, angles, ndet, spacing, shift, dtype):
    return _entries(_key(nx, ny, angles, ndet, spacing, shift, dtype))


def matrix(nx, ny, L, angles, ndet, spacing, shift, dtype=np.float64):
    """(a): L na ndet x L ny nx, float64 values of the T-rounded entries"""
    rows, cols, vals = entries(nx, ny, angles, ndet, spacing, shift, dtype)
    one = sp.csr_matrix((vals.astype(np.float64), (rows, cols)), shape=(len(angles) * ndet, nx * ny))
    K = sp.kron(sp.eye(L), one).tocsr()
    K.sort_indices()
    return K


def _in_order(group, other, vals, x, ngroups, dtype):
    """acc[g] = the sum over the entries of group g, in the order they stand in, of vals * x[other]; starts from the first term"""
    order = np.argsort(group, kind="stable")
    group, other, vals = group[order], other[order], vals[order]
    count = np.bincount(group, minlength=ngroups)
    start = np.concatenate([[0], np.cumsum(count)])[:-1]
    acc = np.full((x.shape[0], ngroups), -0.0, dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(int(count.max()) if count.size else 0):
            sel = np.nonzero(count > k)[0]
            e = start[sel] + k
            acc[:, sel] = acc[:, sel] + vals[e][None, :] * x[:, other[e]]
    return acc


def product(x, nx, ny, L, angles, ndet, spacing, shift, transpose, dtype, res0=None):
    """(b): K x or K^T x in T in the pinned order; res0: the accumulating form, res0 + value"""
    rows, cols, vals = entries(nx, ny, angles, ndet, spacing, shift, dtype)
    m, n = len(angles) * ndet, nx * ny
    if transpose:
        out = _in_order(cols, rows, vals, np.asarray(x).astype(dtype).reshape(L, m), n, dtype)
    else:
        out = _in_order(rows, cols, vals, np.asarray(x).astype(dtype).reshape(L, n), m, dtype)
    out = out.reshape(-1)
    return out if res0 is None else np.asarray(res0).astype(dtype) + out


def terms(nx, ny, L, angles, ndet, spacing, shift, dtype):
    """-> (entries per row, entries per column) of the whole matrix"""
    rows, cols, _ = entries(nx, ny, angles, ndet, spacing, shift, dtype)
    return np.tile(np.bincount(rows, minlength=len(angles) * ndet), L), np.tile(np.bincount(cols, minlength=nx * ny), L)


def sums(nx, ny, L, angles, ndet, spacing, shift, alpha, dtype):
    """(c): (row sums, column sums) of |entry|^alpha in float64"""
    rows, cols, vals = entries(nx, ny, angles, ndet, spacing, shift, dtype)
    v = np.abs(vals.astype(np.float64)) ** alpha
    return (np.tile(np.bincount(rows, weights=v, minlength=len(angles) * ndet), L), np.tile(np.bincount(cols, weights=v, minlength=nx * ny), L))


def bound(nx, ny, L, angles, ndet, spacing, shift, transpose, x, dtype):
    """(d): 1.01 (t + 1) u (|K| |x|) per component"""
    K = abs(matrix(nx, ny, L, angles, ndet, spacing, shift, dtype))
    t = terms(nx, ny, L, angles, ndet, spacing, shift, dtype)[1 if transpose else 0]
    u = np.finfo(dtype).eps / 2
    ax = np.abs(np.asarray(x, dtype=np.float64))
    return 1.01 * (t + 1) * u * ((K.T @ ax) if transpose else (K @ ax))


def abi_records(nx, ny, L, angles, ndet, spacing, transpose):
    """the geometry record of prost_hip_radon2d_geometry: int32 { ny, nx, ndet, na, planes, m, transpose, reserved }"""
    return np.array([ny, nx, ndet, len(angles), L, int(math.ceil(1.0 / spacing)), 1 if transpose else 0, 0], np.int32)
