"""References for prost.block.conv2d_strided (no code of the block is used here), written from the definition

  forward:  out(y, x) = sum_{i, j} k(i, j) in(y sy + py + oy - i, x sx + px + ox - j)                    (zero outside the image)
  adjoint:  in'(v, u) = sum_{i, j, y, x : y sy + py + oy - i = v, x sx + px + ox - j = u, 0 <= y < my, 0 <= x < mx} k(i, j) out(y, x)

with (cy, cx), (oy, ox) the size and crop offset of the un-decimated convolution (conv2d_reference.output_size) and
my = (cy - 1 - py) // sy + 1, mx likewise:

  (a) matrix(..): the explicit scipy matrix, L my mx x L ny nx, holding the dtype-rounded window;
  (b) product(..): the product restated operation for operation on NumPy arrays of a given dtype (every NumPy operation on arrays of
      one dtype rounds once in that dtype, and there is no contraction): zero taps dropped, the terms by ascending source index --
      forward j from kx - 1 down to 0 and inside that i from ky - 1 down to 0, adjoint j ascending and inside that i ascending over the
      taps of the destination pixel's residue class -- source cells outside the plane as zeros, the sum started from the first term, a
      class without taps zero, the accumulating form res0 + value;
  (c) sums(..): the row / column sums of |entries of (a)|^alpha in fp64;
  (d) bound(..): 1.01 (t + 1) u (|K| |x|), the forward error bound of a t-term sum of rounded products in any order, u the unit
      roundoff, t the number of non-zero taps that can reach a result: all of them forward, the largest residue class for the adjoint;
  (e) self_check(..): (a) at stride 1 and phase 0 is conv2d_reference.matrix, at stride s it is that matrix's rows
      (y sy + py, x sx + px).

Images are ny x nx, column-major: element (y, x, c) at y + x ny + c nx ny.
"""
import numpy as np
import scipy.sparse as sp

import conv2d_reference as C

SHAPES = C.SHAPES
window = C.window
taps = C.taps


def pair(v):
    return (int(v), int(v)) if np.isscalar(v) else (int(v[0]), int(v[1]))


def output_size(nx, ny, ky, kx, shape, stride, phase=(0, 0)):
    """-> (my, mx), (oy, ox), (cy, cx)"""
    (sy, sx), (py, px) = pair(stride), pair(phase)
    (cy, cx), (oy, ox) = C.output_size(nx, ny, ky, kx, shape)
    assert cy >= 1 and cx >= 1 and 0 <= py < min(sy, cy) and 0 <= px < min(sx, cx)
    return ((cy - 1 - py) // sy + 1, (cx - 1 - px) // sx + 1), (oy, ox), (cy, cx)


def largest_phase(nx, ny, ky, kx, shape, stride):
    (cy, cx), _ = C.output_size(nx, ny, ky, kx, shape)
    sy, sx = pair(stride)
    return min(sy, cy) - 1, min(sx, cx) - 1


def matrix(nx, ny, L, kernel, shape, stride, phase=(0, 0), dtype=np.float64):
    """(a): csc, float64 entries holding the dtype-rounded window; a zero tap is no entry"""
    k = window(kernel, dtype).astype(np.float64)
    ky, kx = k.shape
    (sy, sx), (py, px) = pair(stride), pair(phase)
    (my, mx), (oy, ox), _ = output_size(nx, ny, ky, kx, shape, stride, phase)
    y, x = np.mgrid[0:my, 0:mx]
    rows, cols, vals = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)], [np.zeros(0)]
    for j in range(kx):
        for i in range(ky):
            if k[i, j] == 0:
                continue
            v, u = y * sy + py + oy - i, x * sx + px + ox - j          # the source pixel tap (i, j) brings to output (y, x)
            ok = (v >= 0) & (v < ny) & (u >= 0) & (u < nx)
            rows.append((y + x * my)[ok]); cols.append((v + u * ny)[ok]); vals.append(np.full(int(ok.sum()), k[i, j]))
    one = sp.csc_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(my * mx, ny * nx))
    K = sp.kron(sp.identity(L), one, format="csc")
    K.eliminate_zeros()
    K.sort_indices()
    assert K.shape == (L * my * mx, L * ny * nx)
    return K


def self_check(nx, ny, L, kernel, shape, stride, phase=(0, 0), dtype=np.float64):
    """(e)"""
    k = window(kernel, dtype)
    ky, kx = k.shape
    (sy, sx), (py, px) = pair(stride), pair(phase)
    (my, mx), _, (cy, cx) = output_size(nx, ny, ky, kx, shape, stride, phase)
    full = C.matrix(nx, ny, L, kernel, shape, dtype)
    K = matrix(nx, ny, L, kernel, shape, stride, phase, dtype)
    if (sy, sx, py, px) == (1, 1, 0, 0):
        assert K.shape == full.shape and (K != full).nnz == 0
    y, x, c = np.meshgrid(np.arange(my), np.arange(mx), np.arange(L), indexing="ij")
    rows = ((y * sy + py) + (x * sx + px) * cy + c * cy * cx).transpose(2, 1, 0).reshape(-1)
    assert (K != full.tocsr()[rows]).nnz == 0
    return True


def class_taps(k, stride, phase, offset, ry, rx):
    """the non-zero taps (i, j) of the residue class (ry, rx) of a destination pixel, in the order the adjoint adds them"""
    (sy, sx), (py, px), (oy, ox) = pair(stride), pair(phase), offset
    ky, kx = k.shape
    return [(i, j) for j in range(kx) for i in range(ky) if (ry + i - py - oy) % sy == 0 and (rx + j - px - ox) % sx == 0 and k[i, j] != 0]


def adjoint_terms(kernel, shape_offset, stride, phase, dtype):
    """the largest number of non-zero taps in one residue class"""
    k = window(kernel, dtype)
    sy, sx = pair(stride)
    return max(len(class_taps(k, stride, phase, shape_offset, ry, rx)) for ry in range(sy) for rx in range(sx))


def product(x, nx, ny, L, kernel, shape, stride, phase, transpose, dtype, res0=None):
    """(b): K x (transpose: K^T x) in dtype, or res0 + that"""
    k = window(kernel, dtype)
    ky, kx = k.shape
    (sy, sx), (py, px) = pair(stride), pair(phase)
    (my, mx), (oy, ox), (cy, cx) = output_size(nx, ny, ky, kx, shape, stride, phase)
    if not transpose:
        src = np.asarray(x).astype(dtype).reshape(L, nx, ny)                    # [c, x, y]
        # every source cell the un-decimated convolution can ask for: cell (ly, lx) is source (ly + oy - (ky - 1), lx + ox - (kx - 1))
        cells = np.zeros((L, cx + kx - 1, cy + ky - 1), dtype)
        ly0, lx0 = ky - 1 - oy, kx - 1 - ox
        y_lo, y_hi = max(0, -ly0), min(ny, cy + ky - 1 - ly0)
        x_lo, x_hi = max(0, -lx0), min(nx, cx + kx - 1 - lx0)
        if y_hi > y_lo and x_hi > x_lo:
            cells[:, lx0 + x_lo:lx0 + x_hi, ly0 + y_lo:ly0 + y_hi] = src[:, x_lo:x_hi, y_lo:y_hi]
        acc = None
        for j in range(kx - 1, -1, -1):
            for i in range(ky - 1, -1, -1):
                if k[i, j] == 0:
                    continue
                a, b = ky - 1 - i + py, kx - 1 - j + px
                term = k[i, j] * cells[:, b:b + (mx - 1) * sx + 1:sx, a:a + (my - 1) * sy + 1:sy]
                acc = term if acc is None else acc + term
        assert acc is not None and acc.dtype == np.dtype(dtype) and acc.shape == (L, mx, my)
        out = acc.reshape(-1)
    else:
        P = 34                                                                   # more than any tap reaches past the plane
        src = np.zeros((L, mx + 2 * P, my + 2 * P), dtype)
        src[:, P:P + mx, P:P + my] = np.asarray(x).astype(dtype).reshape(L, mx, my)
        dst = np.zeros((L, nx, ny), dtype)
        for ry in range(min(sy, ny)):
            for rx in range(min(sx, nx)):
                nvy, nvx = len(range(ry, ny, sy)), len(range(rx, nx, sx))        # destination (ry + sy a, rx + sx b) reads source (a + ey, b + ex)
                acc = None
                for i, j in class_taps(k, stride, phase, (oy, ox), ry, rx):
                    ey, ex = (ry + i - py - oy) // sy, (rx + j - px - ox) // sx
                    assert -P <= ey and -P <= ex and nvy + ey <= my + P and nvx + ex <= mx + P
                    term = k[i, j] * src[:, P + ex:P + ex + nvx, P + ey:P + ey + nvy]
                    acc = term if acc is None else acc + term
                if acc is not None:
                    dst[:, rx::sx, ry::sy] = acc
        out = dst.reshape(-1)
    return out if res0 is None else np.asarray(res0).astype(dtype) + out


def sums(nx, ny, L, kernel, shape, stride, phase, alpha=1.0, dtype=np.float64):
    """(c): sum |entry|^alpha of every row and every column of (a), in fp64 -> (rows, cols)"""
    K = abs(matrix(nx, ny, L, kernel, shape, stride, phase, dtype)).power(float(alpha))
    return np.asarray(K.sum(axis=1)).ravel(), np.asarray(K.sum(axis=0)).ravel()


def terms(nx, ny, kernel, shape, stride, phase, transpose, dtype):
    """t of (d)"""
    if not transpose:
        return taps(kernel, dtype)
    ky, kx = window(kernel, dtype).shape
    return adjoint_terms(kernel, output_size(nx, ny, ky, kx, shape, stride, phase)[1], stride, phase, dtype)


def bound(nx, ny, L, kernel, shape, stride, phase, transpose, x, dtype):
    """(d)"""
    K = abs(matrix(nx, ny, L, kernel, shape, stride, phase, dtype))
    M = K.T if transpose else K
    t = terms(nx, ny, kernel, shape, stride, phase, transpose, dtype)
    return 1.01 * (t + 1) * (np.finfo(dtype).eps / 2) * (M @ np.abs(np.asarray(x, dtype=np.float64)))


# ---- the records of include/prost_hip.h, restated ----
TILES = ((64, 16, 4), (64, 8, 2), (64, 4, 1), (32, 8, 1), (32, 4, 1))          # kTiles of include/prost/linop/conv2d_strided.hpp
LDS_LIMIT = 65536
ADJ_LANES, ADJ_COLUMNS, CLASSES = 64, 16, 16


def sub_pitch(ty, ky, sy):
    return ty + (ky - 1) // sy


def lds_bytes(tile, dtype, stride, ky, kx):
    """the staged source tile of a forward tile"""
    (ty, tx, _), (sy, sx) = tile, pair(stride)
    return sy * sub_pitch(ty, ky, sy) * ((tx - 1) * sx + kx) * np.dtype(dtype).itemsize


def pick_tile(dtype, stride, ky, kx):
    """the first entry of the table whose staged tile fits"""
    return next(t for t, tile in enumerate(TILES) if lds_bytes(tile, dtype, stride, ky, kx) <= LDS_LIMIT)


def abi_records(nx, ny, L, kernel, shape, stride, phase, transpose, dtype):
    """one direction as include/prost_hip.h describes it for prost_hip_conv2d_strided_*: the 31 int32 of the geometry record, the tap
    table as int32 words and the tap count"""
    k = window(kernel, dtype)
    ky, kx = k.shape
    (sy, sx), (py, px) = pair(stride), pair(phase)
    (my, mx), (oy, ox), _ = output_size(nx, ny, ky, kx, shape, stride, phase)
    rec = np.dtype([("offset", np.int32), ("value", np.float32)] if np.dtype(dtype) == np.float32 else
                   [("offset", np.int32), ("reserved", np.int32), ("value", np.float64)])
    start = [0] * (CLASSES + 1)
    if not transpose:
        sub = sub_pitch(TILES[pick_tile(dtype, stride, ky, kx)][0], ky, sy)
        table = [((ky - 1 - i) // sy + ((ky - 1 - i) % sy) * sub + (kx - 1 - j) * sy * sub, k[i, j])
                 for j in range(kx - 1, -1, -1) for i in range(ky - 1, -1, -1) if k[i, j] != 0]
        start[1:] = [len(table)] * CLASSES
    else:
        lo = (py + oy) // sy
        pitch = ADJ_LANES + lo + (sy + ky - 2 - py - oy) // sy
        table = []
        for ry in range(sy):
            for rx in range(sx):
                start[ry * sx + rx] = len(table)
                table += [((ry + i - py - oy) // sy + lo + ((rx + j - px - ox) // sx) * pitch, k[i, j]) for i, j in class_taps(k, stride, phase, (oy, ox), ry, rx)]
        start[sy * sx:] = [len(table)] * (CLASSES + 1 - sy * sx)
    t = np.zeros(len(table), rec)
    t["offset"] = [o for o, _ in table]
    t["value"] = [v for _, v in table]
    geometry = np.array([ny, nx, my, mx, oy, ox, ky, kx, sy, sx, py, px, L, 1 if transpose else 0] + start, np.int32)
    return geometry, t.view(np.int32).copy(), len(table)


# ---- the cases ----
STRIDES = ((1, 1), (2, 2), (3, 2), (1, 3), (4, 4))
WINDOWS = ("1x1", "3x3", "2x5", "5x4z", "9x9g")
IMAGES = ((1, 1, 1), (7, 5, 1), (17, 13, 3))


def gauss(size, sigma):
    r = (size - 1) / 2.0
    yy, xx = np.mgrid[0:size, 0:size].astype(np.float64) - r
    k = np.exp(-(xx * xx + yy * yy) / (2.0 * sigma * sigma))
    return k / k.sum()


def make_window(name):
    """1x1; 3x3, 2x5 (even, asymmetric), 31x31: standard normal; 5x4z: standard normal with zero taps; 9x9g, 5x5g: Gaussians"""
    if name.endswith("g"):
        n = int(name.split("x")[0])
        return gauss(n, n / 4.0)
    ky, kx = (int(v) for v in name.rstrip("z").split("x"))
    k = np.random.default_rng(97 * ky + kx).standard_normal((ky, kx))
    if name.endswith("z"):
        k[0, 0] = k[2, 1] = k[4, 3] = k[1, 2] = 0.0
        k[:, 1][k[:, 1] > 0.3] = 0.0
    return k


def valid_shapes(ny, nx, ky, kx):
    return tuple(s for s in SHAPES if s != "valid" or (ny >= ky and nx >= kx))


def cases(dtype):
    """(ny, nx, L, window name, stride, phase, shape), the smallest shapes at which each mechanism can fail:
      * every stride with every window, the three images in turn, all shapes, phase (0, 0) and the largest legal phase in turn;
      * for every tile-table entry these select in `dtype`: an image whose output is exactly one tile, and one a row and a column past it;
      * 31 x 31 once per stride (4, 4) and (1, 1); a ragged last stride (my sy + py != cy); "valid" with the window equal to the image"""
    out, entries = [], {}
    for si, stride in enumerate(STRIDES):
        for wi, name in enumerate(WINDOWS):
            ky, kx = make_window(name).shape
            ny, nx, L = IMAGES[(si + wi) % len(IMAGES)]
            entries.setdefault(pick_tile(dtype, stride, ky, kx), (name, stride))
            for hi, shape in enumerate(valid_shapes(ny, nx, ky, kx)):
                phase = (0, 0) if (si + wi + hi) % 2 == 0 else largest_phase(nx, ny, ky, kx, shape, stride)
                out.append((ny, nx, L, name, stride, phase, shape))
    for stride in ((4, 4), (1, 1)):
        entries.setdefault(pick_tile(dtype, stride, 31, 31), ("31x31", stride))
    for entry, (name, stride) in sorted(entries.items()):
        ty, tx, _ = TILES[entry]
        (sy, sx) = stride
        for extra in (0, 1):                                          # "same", phase 0: my = (ny - 1) // sy + 1
            out.append(((ty - 1 + extra) * sy + 1, (tx - 1 + extra) * sx + 1, 1, name, stride, (0, 0), "same"))
    out.append((9, 6, 1, "31x31", (4, 4), (3, 3), "same"))
    out.append((9, 6, 1, "31x31", (1, 1), (0, 0), "full"))
    out.append((12, 11, 2, "3x3", (3, 2), (1, 0), "same"))              # cy = 12: my = 4, my sy + py = 13 != cy
    out.append((5, 4, 1, "5x4z", (2, 2), (0, 0), "valid"))              # the window is the image: one output
    return out


def case_id(case):
    ny, nx, L, name, stride, phase, shape = case
    return "%dx%dx%d-%s-s%d%d-p%d%d-%s" % (ny, nx, L, name, stride[0], stride[1], phase[0], phase[1], shape)


def case_seed(case, salt=0):
    ny, nx, L, name, stride, phase, shape = case
    return 11 + salt + 13 * ny + 1009 * nx + 100003 * L + 17 * len(name) + 29 * stride[0] + 31 * stride[1] + 37 * phase[0] + 41 * phase[1] + SHAPES.index(shape)
