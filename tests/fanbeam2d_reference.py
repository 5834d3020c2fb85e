"""References for prost.block.fanbeam2d, written from the definition (the issue text and the comment at the head of
include/prost/linop/fanbeam2d.hpp), never from the code under test.  NumPy and scipy only, vectorised.

Geometry: L column-major planes of ny x nx, element (y, x, c) at y + x ny + c nx ny; L sinograms, bin d of view a of plane c at
d + a ndet + c ndet na.  View beta: e = (cos, sin), n = (-sin, cos), source S = -R n.  Bin d at u_d = (d - (ndet - 1) / 2) spacing + shift
on a detector at distance D from the source, fan angle gamma_d = atan2(u_d, D) (flat) or u_d / D (curved).  The tables are formed in
Python floats (IEEE double; libm's functions, as in the host library) and rounded once to T:
  per view   cos, sin, sx = R sin + (nx - 1) / 2, sy = -R cos + (ny - 1) / 2, axis (0: |cos| >= |sin|, rows; 1: columns)
  per bin    sin gamma_d, cos gamma_d
  inverse    k0 = (ndet - 1) / 2 - shift / spacing, k1 = D / spacing, lo = tan gamma_0, hi = tan gamma_(ndet - 1), a_1 .. a_6
Prologue of ray (a, d), every operation one rounding in T: dx = sg cos - cg sin, dy = sg sin + cg cos; (dt, di, st, si) = (dy, dx, sy, sx)
at a row-driven view and (dx, dy, sx, sy) at a column-driven one; p = di / dt, r = si - st p, c = 1 / |dt|.  Position on driving line t:
f = r + p t; i0 = floor(f), w1 = f - i0, w0 = 1 - w1; entries c w0 at (t, i0) and c w1 at (t, i0 + 1), absent outside the image or with a
weight of exactly 0.

  (a) matrix(..)          the matrix in float64 from the T-rounded tables, a scipy CSR
  (b) product(..)         the restatement in T in the pinned order: forward over t ascending, i0 before i0 + 1, from the RAY enumeration;
                          adjoint over views ascending and bins ascending, from the GATHER enumeration: per pixel and view the window
                          b - m .. b + m + 1 located from the pixel's own s / l, every candidate's weight recomputed
  (c) sums(..)            row and column sums of |entry|^alpha by math.fsum
  (d) bound(..)           1.01 (t + 1) u (|K| |x|) per component, t the number of terms of that row or column
"""
import functools
import math

import numpy as np
import scipy.sparse as sp

MAX_MARGIN = 5
SLACK = 0.25
MAX_FAN = math.radians(30.0)
ATAN = tuple(float.fromhex(h) for h in ("-0x1.555554068e4bfp-2", "0x1.9997596a700bdp-3", "-0x1.24411bcc780e6p-3", "0x1.be972ff58fbf4p-4", "-0x1.3eaccbf0ae46ap-4",
                                        "0x1.21335f33de351p-5"))
ATAN_ERROR = 3.4e-9
VIEW_SETS = {
    # all four quadrants, the axis ties at pi / 4 and 3 pi / 4, the axes themselves, angles outside 0 .. 2 pi
    "quad": (0.0, math.pi / 4, math.pi / 2, 3 * math.pi / 4, math.pi, -math.pi / 4, 5 * math.pi / 4 + 0.1, 2 * math.pi + 0.1, -2.0),
}


def half_diagonal(nx, ny):
    return math.hypot(nx, ny) / 2.0


def centre_radius(nx, ny):
    return math.hypot(nx - 1, ny - 1) / 2.0


def default_ndet(nx, ny, R, D, spacing, curved):
    need = math.asin(half_diagonal(nx, ny) / R)
    return 2 * int(math.ceil((D * need if curved else D * math.tan(need)) / spacing)) + 1


def bin_angle(d, ndet, D, spacing, shift, curved):
    u = (d - (ndet - 1) / 2.0) * spacing + shift
    return u / D if curved else math.atan2(u, D)


def max_fan(ndet, D, spacing, shift, curved):
    return max(abs(bin_angle(0, ndet, D, spacing, shift, curved)), abs(bin_angle(ndet - 1, ndet, D, spacing, shift, curved)))


def window(nx, ny, R, D, ndet, spacing, shift, curved):
    """W: the most bins between a pixel's own bin and a ray that crosses its driving line within one pixel of it"""
    return D / (R - centre_radius(nx, ny)) / (spacing * math.cos(max_fan(ndet, D, spacing, shift, curved)))


def margin(nx, ny, R, D, ndet, spacing, shift, curved):
    return int(math.ceil(window(nx, ny, R, D, ndet, spacing, shift, curved) + SLACK))


def admissible(nx, ny, R, D, ndet, spacing, shift, curved):
    """the three geometric conditions of creation"""
    return (R >= half_diagonal(nx, ny) + 1 and max_fan(ndet, D, spacing, shift, curved) <= MAX_FAN
            and margin(nx, ny, R, D, ndet, spacing, shift, curved) <= MAX_MARGIN)


def closest_source(nx, ny, ndet, spacing, shift, curved, dscale=1.0):
    """the smallest R on a grid of 1 / 16 pixel at which creation passes with D = dscale R (every condition is monotone in R)"""
    lo, hi = 0, int(16 * 1000 * half_diagonal(nx, ny))
    assert admissible(nx, ny, hi / 16.0, dscale * hi / 16.0, ndet, spacing, shift, curved)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if mid > 0 and admissible(nx, ny, mid / 16.0, dscale * mid / 16.0, ndet, spacing, shift, curved):
            hi = mid
        else:
            lo = mid
    return hi / 16.0


def views_of(kind, fan=0.0):
    """'quad': the nine special views; ('short', n): n views evenly over [0, pi + 2 fan); ('full', n): n views over a full turn"""
    if kind == "quad":
        return np.array(VIEW_SETS["quad"])
    name, n = kind
    span = math.pi + 2 * fan if name == "short" else 2 * math.pi
    return np.arange(n) * (span / n)


# (ny, nx, L, views, ndet (None: the default), spacing, shift, R ('closest' or a multiple of the half diagonal), detector, D / R).
# The kernels' units are 64 bins of one view per wavefront (forward) and 64 rows of one column per wavefront (adjoint); at a row-driven
# view the forward kernel stages slabs of 16 rows by up to 128 columns.  The margins of the cases are 1 .. 5: every adjoint instance.
CASES = (
    (1, 1, 1, "quad", 1, 1.0, 0.0, 100.0, "flat", 1.0),
    (1, 1, 1, "quad", 3, 0.5, 0.25, "closest", "curved", 1.0),
    (3, 5, 1, "quad", 1, 0.5, 0.25, "closest", "flat", 1.0),                 # the margin at its cap
    (3, 5, 3, ("full", 8), 63, 0.5, 0.0, "closest", "flat", 1.0),            # a detector much longer than the image: rays that miss it
    (17, 33, 1, "quad", 65, 1.0, 0.25, 4.0, "flat", 1.0),
    (17, 33, 3, ("short", 7), 63, 0.5, 0.0, 2.5, "curved", 1.0),
    (17, 33, 1, ("full", 8), None, 0.5, 0.0, 100.0, "curved", 1.0),
    (17, 33, 1, ("full", 5), None, 2.0, 0.25, 3.0, "curved", 1.5),           # a detector behind the rotation centre
    (70, 45, 1, "quad", 130, 2.0, 0.25, "closest", "flat", 1.0),             # the closest source the 30 degrees admit; rays that miss
    (70, 45, 1, ("full", 8), None, 1.0, 0.0, 100.0, "flat", 1.0),
    (70, 45, 3, ("short", 7), 130, 0.5, 0.25, 3.0, "curved", 1.0),
    (40, 150, 1, "quad", None, 1.0, 0.0, 3.0, "flat", 1.0),                  # taller than one slab, wider than kSlabColumns
    (40, 150, 1, ("full", 8), None, 2.0, 0.25, 3.0, "curved", 1.0),          # 64 bins two pixels apart: slabs too wide to be staged
)


def case_id(case):
    ny, nx, L, kind, ndet, spacing, shift, R, detector, dscale = case
    return "%dx%dx%d-%s-ndet%s-h%g-s%g-R%s-%s-D%g" % (ny, nx, L, kind if isinstance(kind, str) else "%s%d" % kind, "default" if ndet is None else ndet, spacing, shift, R,
                                                      detector, dscale)


@functools.lru_cache(maxsize=None)
def case_args(case):
    """-> (nx, ny, L, angles, R, D, ndet, spacing, shift, detector), the arguments of prost.block.fanbeam2d with everything resolved"""
    ny, nx, L, kind, ndet, spacing, shift, R, detector, dscale = case
    curved = detector == "curved"
    if R == "closest":
        R = closest_source(nx, ny, ndet, spacing, shift, curved, dscale)
    else:
        R = R * half_diagonal(nx, ny)
    D = dscale * R
    if ndet is None:
        ndet = default_ndet(nx, ny, R, D, spacing, curved)
    angles = views_of(kind, max_fan(ndet, D, spacing, shift, curved))
    angles.setflags(write=False)
    return nx, ny, L, angles, R, D, ndet, spacing, shift, detector


def case_margin(case):
    nx, ny, L, angles, R, D, ndet, spacing, shift, detector = case_args(case)
    return margin(nx, ny, R, D, ndet, spacing, shift, detector == "curved")


def case_seed(case, salt=0):
    return 1000 * CASES.index(case) + salt


def tables(nx, ny, angles, R, D, ndet, spacing, shift, detector, dtype):
    """-> views (na, 5), bins (ndet, 2), inverse (10) in T"""
    T = np.dtype(dtype).type
    curved = detector == "curved"
    cx, cy = (nx - 1) / 2.0, (ny - 1) / 2.0
    views = np.zeros((len(angles), 5), dtype)
    for a, beta in enumerate(angles):
        co, si = math.cos(float(beta)), math.sin(float(beta))
        views[a] = [T(co), T(si), T(R * si + cx), T(-R * co + cy), T(0.0 if abs(co) >= abs(si) else 1.0)]
    bins = np.zeros((ndet, 2), dtype)
    for d in range(ndet):
        gamma = bin_angle(d, ndet, D, spacing, shift, curved)
        bins[d] = [T(math.sin(gamma)), T(math.cos(gamma))]
    inverse = np.array([T((ndet - 1) / 2.0 - shift / spacing), T(D / spacing), T(math.tan(bin_angle(0, ndet, D, spacing, shift, curved))),
                        T(math.tan(bin_angle(ndet - 1, ndet, D, spacing, shift, curved)))] + [T(a if curved else 0.0) for a in ATAN], dtype)
    return views, bins, inverse


def table(nx, ny, angles, R, D, ndet, spacing, shift, detector, dtype):
    """the three tables as the one array the entry points take"""
    return np.concatenate([t.ravel() for t in tables(nx, ny, angles, R, D, ndet, spacing, shift, detector, dtype)])


def rays(view, bins, dtype):
    """the prologue of every bin's ray at one view -> (p, r, c), arrays of T over the bins, and whether the view is column-driven"""
    T = np.dtype(dtype).type
    co, si, sx, sy, axis = (T(v) for v in view)
    sg, cg = bins[:, 0], bins[:, 1]
    dx = sg * co - cg * si
    dy = sg * si + cg * co
    column = axis != 0
    dt, di, st, s_i = (dx, dy, sx, sy) if column else (dy, dx, sy, sx)
    with np.errstate(divide="ignore", invalid="ignore"):
        p = di / dt
        r = s_i - st * p
        c = T(1) / np.abs(dt)
    assert p.dtype == r.dtype == c.dtype == np.dtype(dtype)
    return p, r, c, column


def _key(nx, ny, angles, R, D, ndet, spacing, shift, detector, dtype):
    return (int(nx), int(ny), tuple(float(a) for a in np.asarray(angles, np.float64).ravel()), float(R), float(D), int(ndet), float(spacing), float(shift), str(detector),
            np.dtype(dtype).name)


def _frozen(*arrays):
    for v in arrays:
        v.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=64)
def _entries(key):
    """the ray enumeration of one plane -> (rows, cols, vals in T): rows ascending and inside a row t ascending, i0 first"""
    nx, ny, angles, R, D, ndet, spacing, shift, detector, name = key
    dtype = np.dtype(name)
    T = dtype.type
    views, bins, _ = tables(nx, ny, angles, R, D, ndet, spacing, shift, detector, dtype)
    rows, cols, vals = [], [], []
    d = np.arange(ndet)
    for a in range(len(angles)):
        p, r, c, column = rays(views[a], bins, dtype)
        nt, ni = (nx, ny) if column else (ny, nx)
        t = np.arange(nt)
        with np.errstate(invalid="ignore"):
            f = r[:, None] + p[:, None] * t.astype(dtype)[None, :]
            assert f.dtype == dtype
            fl = np.floor(f)
            w1 = f - fl
            w0 = T(1) - w1
            possible = (fl >= -1) & (fl < ni)
        i0 = np.where(possible, fl, -2).astype(np.int64)
        slot_i = np.stack([i0, i0 + 1], axis=2)
        slot_w = np.stack([w0, w1], axis=2)
        present = possible[:, :, None] & (slot_i >= 0) & (slot_i < ni) & (slot_w != 0)
        value = c[:, None, None] * slot_w
        assert value.dtype == dtype
        t3 = np.broadcast_to(t[None, :, None], slot_i.shape)
        pixel = np.where(column, slot_i + t3 * ny, t3 + slot_i * ny)         # y + x ny
        row = np.broadcast_to((a * ndet + d)[:, None, None], slot_i.shape)
        rows.append(row[present])
        cols.append(pixel[present])
        vals.append(value[present])
    return _frozen(np.concatenate(rows), np.concatenate(cols), np.concatenate(vals))


def entries(nx, ny, angles, R, D, ndet, spacing, shift, detector, dtype):
    return _entries(_key(nx, ny, angles, R, D, ndet, spacing, shift, detector, dtype))


@functools.lru_cache(maxsize=64)
def _gathered(key):
    """the gather enumeration of one plane -> (rows, cols, vals in T): pixels ascending (y + x ny) and inside a pixel views ascending,
    bins ascending"""
    nx, ny, angles, R, D, ndet, spacing, shift, detector, name = key
    dtype = np.dtype(name)
    T = dtype.type
    views, bins, inv = tables(nx, ny, angles, R, D, ndet, spacing, shift, detector, dtype)
    m = margin(nx, ny, R, D, ndet, spacing, shift, detector == "curved")
    k0, k1, lo, hi = (T(v) for v in inv[:4])
    poly_c = [T(v) for v in inv[4:]]
    x, y = np.meshgrid(np.arange(nx), np.arange(ny))                       # pixel (y, x) at [y, x]
    x, y = x.T.ravel(), y.T.ravel()                                        # in the order of y + x ny
    pixel = y + x * ny
    rows, cols, vals, order = [], [], [], []
    for a in range(len(angles)):
        co, si, sx, sy, _ = (T(v) for v in views[a])
        p, r, c, column = rays(views[a], bins, dtype)
        t, i, ni = (x, y, ny) if column else (y, x, nx)
        px, py = x.astype(dtype) - sx, y.astype(dtype) - sy
        s = px * co + py * si
        l = py * co - px * si
        with np.errstate(divide="ignore", invalid="ignore"):
            tau = s / l
        tau = np.where(tau > lo, tau, lo)
        tau = np.where(tau < hi, tau, hi)
        z = tau * tau
        poly = np.full(z.shape, poly_c[-1], dtype)
        for coeff in poly_c[-2::-1]:
            poly = poly * z + coeff
        gamma = tau + tau * (z * poly)
        b = np.floor(k0 + k1 * gamma)
        assert b.dtype == dtype
        b = np.where(b > -1, b, -1)
        first = np.where(b < ndet - 1, b, ndet - 1).astype(np.int64) - m
        for k in range(2 * m + 2):
            d = first + k
            ok = (d >= 0) & (d < ndet)
            dc = np.clip(d, 0, ndet - 1)
            with np.errstate(invalid="ignore"):
                f = r[dc] + p[dc] * t.astype(dtype)
                fl = np.floor(f)
                w1 = f - fl
                w0 = T(1) - w1
                possible = (fl >= -1) & (fl < ni)
            i0 = np.where(possible, fl, -2).astype(np.int64)
            w = np.where(i0 == i, w0, w1)
            ok &= ((i0 == i) | (i0 + 1 == i)) & (w != 0)
            value = c[dc] * w
            assert value.dtype == dtype
            rows.append((a * ndet + d)[ok])
            cols.append(pixel[ok])
            vals.append(value[ok])
    rows, cols, vals = np.concatenate(rows), np.concatenate(cols), np.concatenate(vals)
    order = np.lexsort((rows, cols))                                       # candidates ascend inside a view, views ascend: rows ascend
    return _frozen(rows[order], cols[order], vals[order])


def gathered(nx, ny, angles, R, D, ndet, spacing, shift, detector, dtype):
    return _gathered(_key(nx, ny, angles, R, D, ndet, spacing, shift, detector, dtype))


def matrix(nx, ny, L, angles, R, D, ndet, spacing, shift, detector, dtype=np.float64):
    """(a): L na ndet x L ny nx, float64 values of the T-rounded entries"""
    rows, cols, vals = entries(nx, ny, angles, R, D, ndet, spacing, shift, detector, dtype)
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


def product(x, nx, ny, L, angles, R, D, ndet, spacing, shift, detector, transpose, dtype, res0=None):
    """(b): K x from the ray enumeration or K^T x from the gather enumeration, in T in the pinned order; res0: res0 + value"""
    m, n = len(angles) * ndet, nx * ny
    if transpose:
        rows, cols, vals = gathered(nx, ny, angles, R, D, ndet, spacing, shift, detector, dtype)
        out = _in_order(cols, rows, vals, np.asarray(x).astype(dtype).reshape(L, m), n, dtype)
    else:
        rows, cols, vals = entries(nx, ny, angles, R, D, ndet, spacing, shift, detector, dtype)
        out = _in_order(rows, cols, vals, np.asarray(x).astype(dtype).reshape(L, n), m, dtype)
    out = out.reshape(-1)
    return out if res0 is None else np.asarray(res0).astype(dtype) + out


def terms(nx, ny, L, angles, R, D, ndet, spacing, shift, detector, dtype):
    """-> (entries per row, entries per column) of the whole matrix"""
    rows, cols, _ = entries(nx, ny, angles, R, D, ndet, spacing, shift, detector, dtype)
    return np.tile(np.bincount(rows, minlength=len(angles) * ndet), L), np.tile(np.bincount(cols, minlength=nx * ny), L)


def _fsums(group, values, ngroups):
    order = np.argsort(group, kind="stable")
    bounds = np.concatenate([[0], np.cumsum(np.bincount(group, minlength=ngroups))])
    v = values[order]
    return np.array([math.fsum(v[bounds[g]:bounds[g + 1]]) for g in range(ngroups)])


def sums(nx, ny, L, angles, R, D, ndet, spacing, shift, detector, alpha, dtype):
    """(c): (row sums, column sums) of |entry|^alpha, each by math.fsum"""
    rows, cols, vals = entries(nx, ny, angles, R, D, ndet, spacing, shift, detector, dtype)
    v = np.abs(vals.astype(np.float64)) ** alpha
    return np.tile(_fsums(rows, v, len(angles) * ndet), L), np.tile(_fsums(cols, v, nx * ny), L)


def bound(nx, ny, L, angles, R, D, ndet, spacing, shift, detector, transpose, x, dtype):
    """(d): 1.01 (t + 1) u (|K| |x|) per component"""
    K = abs(matrix(nx, ny, L, angles, R, D, ndet, spacing, shift, detector, dtype))
    t = terms(nx, ny, L, angles, R, D, ndet, spacing, shift, detector, dtype)[1 if transpose else 0]
    u = np.finfo(dtype).eps / 2
    ax = np.abs(np.asarray(x, dtype=np.float64))
    return 1.01 * (t + 1) * u * ((K.T @ ax) if transpose else (K @ ax))


def abi_records(nx, ny, L, angles, R, D, ndet, spacing, shift, detector, transpose):
    """the geometry record of prost_hip_fanbeam2d_geometry: int32 { ny, nx, ndet, na, planes, m, transpose, reserved }"""
    return np.array([ny, nx, ndet, len(angles), L, margin(nx, ny, R, D, ndet, spacing, shift, detector == "curved"), 1 if transpose else 0, 0], np.int32)


def digest(values):
    """FNV-1a over the bytes of the values: what tests/host/fanbeam2d_harness.cpp prints"""
    h = 1469598103934665603
    for byte in np.ascontiguousarray(values).tobytes():
        h = ((h ^ byte) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return "%016x" % h


def digest_input(n, salt, dtype):
    """the input vector of a digest: element k is ((k + salt) * 2654435761 mod 2^32) / 2^32 - 1 / 2, exact in double, rounded to T"""
    k = (np.arange(n, dtype=np.uint64) + np.uint64(salt)) * np.uint64(2654435761) % np.uint64(2 ** 32)
    return (k.astype(np.float64) / 2.0 ** 32 - 0.5).astype(dtype)
