"""Linear-operator block builders -- Python mirror of matlab/+prost/+block/*.m.

Each builder returns ``func(row, col, nrows, ncols) -> [[name, row, col, data], [nrows, ncols]]``
exactly like the MATLAB closures (gradient2d.m:12-14, gradient3d.m:12-14, sparse.m:6-9,
diags.m:17-20, identity.m:11-12, zero.m:3-4, dense.m, dense_kron_id.m, id_kron_dense.m).  Cells are Python lists.
"""
import math

import numpy as np


def gradient2d(nx, ny, L, label_first=False):
    sz = [nx * ny * L * 2, nx * ny * L]
    data = [nx, ny, L, bool(label_first)]
    return lambda row, col, nrows, ncols: [["gradient2d", row, col, data], sz]


def gradient3d(nx, ny, L, label_first=False):
    sz = [nx * ny * L * 3, nx * ny * L]
    data = [nx, ny, L, bool(label_first)]
    return lambda row, col, nrows, ncols: [["gradient3d", row, col, data], sz]


def sparse(K):
    import scipy.sparse as sp
    K = sp.csc_matrix(K, dtype=np.float64, copy=True)      # (copy: the two calls below work in place and K may BE the caller's matrix)
    K.eliminate_zeros()                 # a MATLAB sparse matrix holds no explicit zeros (scipy constructions such as diags / kron do)
    K.sort_indices()
    sz = [K.shape[0], K.shape[1]]
    return lambda row, col, nrows, ncols: [["sparse", row, col, [K]], sz]


def _kron(name, K, diaglength):
    import scipy.sparse as sp
    K = sp.csc_matrix(K, dtype=np.float64, copy=True)
    K.eliminate_zeros()
    K.sort_indices()
    d = int(diaglength)
    sz = [K.shape[0] * d, K.shape[1] * d]
    return lambda row, col, nrows, ncols: [[name, row, col, [K, d]], sz]


def sparse_kron_id(K, diaglength):
    """sparse_kron_id.m:1-14: kron(K, speye(diaglength)) without forming it"""
    return _kron("sparse_kron_id", K, diaglength)


def id_kron_sparse(K, diaglength):
    """id_kron_sparse.m:1-14: kron(speye(diaglength), K) without forming it"""
    return _kron("id_kron_sparse", K, diaglength)


def _full(K):
    import scipy.sparse as sp
    K = K.toarray() if sp.issparse(K) else K
    K = np.array(K, dtype=np.float64, order="F", copy=True)
    if K.ndim != 2:
        raise ValueError("K must be a matrix (2-D), got %d-D" % K.ndim)
    return K


def dense(K):
    """dense.m: a full matrix K, applied without a sparse index structure"""
    K = _full(K)
    sz = [K.shape[0], K.shape[1]]
    return lambda row, col, nrows, ncols: [["dense", row, col, [K]], sz]


def _kron_dense(name, K, diaglength):
    K = _full(K)
    d = int(diaglength)
    sz = [K.shape[0] * d, K.shape[1] * d]
    return lambda row, col, nrows, ncols: [[name, row, col, [K, d]], sz]


def dense_kron_id(K, diaglength):
    """dense_kron_id.m: kron(K, speye(diaglength)) for a full K without forming it"""
    return _kron_dense("dense_kron_id", K, diaglength)


def id_kron_dense(K, diaglength):
    """id_kron_dense.m: kron(speye(diaglength), K) for a full K without forming it"""
    return _kron_dense("id_kron_dense", K, diaglength)


_NUMBER = (int, float, np.integer, np.floating)


def _whole(block, name, v, loose=False):
    """v, a Python or numpy number with an integer value, as an int.  loose: the three oldest builders (dataterm_sublabel, conv2d,
    conv2d_strided) take whatever numpy can test, a 0-d array for instance, and let numpy's TypeError for anything else escape."""
    if isinstance(v, bool) or not (loose or isinstance(v, _NUMBER)) or not np.isfinite(v) or int(v) != v:
        raise ValueError("%s: %s = %r is not an integer" % (block, name, v))
    return int(v)


def _integer(block, name, v, top=None, loose=False):
    """_whole, and 1 <= v (<= top)"""
    n = _whole(block, name, v, loose)
    if v < 1:
        raise ValueError("%s: %s = %r has to be at least 1" % (block, name, v))
    if top is not None and v > top:
        raise ValueError("%s: %s = %r has to be at most %d" % (block, name, v, top))
    return n


def _numbers(block, v, refusal):
    """v, an array of integers or floats, as a new float64 array"""
    try:
        if np.asarray(v).dtype.kind not in "iuf":
            raise TypeError
        return np.array(v, dtype=np.float64, copy=True)
    except (TypeError, ValueError):
        raise ValueError("%s: %s" % (block, refusal))


def dataterm_sublabel(nx, ny, L, left, right):
    """The coupling of the sublabel-accurate data term (Moellenhoff et al., CVPR 2016) for L equidistant labels on [left, right],
    applied without a matrix.  k = L - 1 intervals, N = nx ny pixels, every part k planes of N values (element (p, i) at i N + p, the
    layout of gradient2d(nx, ny, k), sum_ind_simplex(k, False) and sum_ind_epi_conjquad_1d(False, ..)).  Domain [u ; w]: the lifted
    labelling and the interval weights; range [r ; s]: (r_i, s_i) lives in the epigraph of the conjugate of piece i
    (alpha = left + i delta, beta = alpha + delta, delta = (right - left) / (L - 1)).  Per pixel
    r_i = delta u_i + gamma_i w_i - delta sum_{j > i} w_j and s_i = -w_i."""
    nx, ny, L = [_whole("dataterm_sublabel", name, v, loose=True) for name, v in (("nx", nx), ("ny", ny), ("L", L))]
    left, right = float(left), float(right)
    if L < 2:
        raise ValueError("dataterm_sublabel: L = %d labels, at least 2 are needed" % L)
    if nx < 1 or ny < 1:
        raise ValueError("dataterm_sublabel: nx = %d and ny = %d have to be at least 1" % (nx, ny))
    if not (np.isfinite(left) and np.isfinite(right)):
        raise ValueError("dataterm_sublabel: the bounds left = %r and right = %r have to be finite" % (left, right))
    if not left < right:
        raise ValueError("dataterm_sublabel: left = %r has to be below right = %r" % (left, right))
    n = 2 * nx * ny * (L - 1)
    sz = [n, n]
    data = [nx, ny, L, left, right]
    return lambda row, col, nrows, ncols: [["dataterm_sublabel", row, col, data], sz]


CONV2D_MAX_WINDOW = 31


def conv2d_size(nx, ny, ky, kx, shape):
    """-> (my, mx), (oy, ox): the output size and the crop offset into the full convolution"""
    if shape == "full":
        return (ny + ky - 1, nx + kx - 1), (0, 0)
    if shape == "same":
        return (ny, nx), (ky // 2, kx // 2)
    if shape == "valid":
        return (ny - ky + 1, nx - kx + 1), (ky - 1, kx - 1)
    raise ValueError("conv2d: unknown shape %r (full, same or valid)" % (shape,))


def _conv_window(block, kernel):
    """the window of conv2d and conv2d_strided as a new column-major float64 matrix"""
    kernel = np.array(kernel, dtype=np.float64, order="F", copy=True)
    if kernel.ndim != 2 or kernel.size == 0:
        raise ValueError("%s: the window has to be a non-empty matrix (2-D), got shape %r" % (block, kernel.shape))
    ky, kx = kernel.shape
    if ky > CONV2D_MAX_WINDOW or kx > CONV2D_MAX_WINDOW:
        raise ValueError("%s: the window is %d x %d, windows up to %d x %d are supported" % (block, ky, kx, CONV2D_MAX_WINDOW, CONV2D_MAX_WINDOW))
    if not np.isfinite(kernel).all():
        raise ValueError("%s: the window holds a non-finite value" % block)
    if not kernel.any():
        raise ValueError("%s: the window has no non-zero tap" % block)
    return kernel


def conv2d(nx, ny, L, kernel, shape="full"):
    """2-D convolution of L column-major image planes of ny x nx (element (y, x, c) at y + x ny + c nx ny, the layout of
    gradient2d(nx, ny, L)) with one ky x kx window, zero padding, applied without a matrix:
    out(y, x) = sum_{i, j} kernel[i, j] in(y + oy - i, x + ox - j).  shape "full": (ny + ky - 1) x (nx + kx - 1) outputs per plane, the
    matrix kron(eye(L), convmtx2(kernel, ny, nx)); "same": ny x nx, MATLAB's conv2(.., 'same'); "valid": (ny - ky + 1) x (nx - kx + 1).
    Windows up to 31 x 31."""
    nx, ny, L = [_integer("conv2d", name, v, loose=True) for name, v in (("nx", nx), ("ny", ny), ("L", L))]
    kernel = _conv_window("conv2d", kernel)
    ky, kx = kernel.shape
    if not isinstance(shape, str):
        raise ValueError("conv2d: unknown shape %r (full, same or valid)" % (shape,))
    (my, mx), _ = conv2d_size(nx, ny, ky, kx, shape)
    if my < 1 or mx < 1:
        raise ValueError("conv2d: the window (%d x %d) is larger than the image (%d x %d): the valid part is empty" % (ky, kx, ny, nx))
    if nx * ny >= 2 ** 31 or my * mx >= 2 ** 31:
        raise ValueError("conv2d: a plane of %d elements; it has to stay below 2^31" % max(nx * ny, my * mx))
    sz = [L * my * mx, L * ny * nx]
    data = [nx, ny, L, kernel, shape]
    return lambda row, col, nrows, ncols: [["conv2d", row, col, data], sz]


CONV2D_STRIDED_MAX_STRIDE = 4


def _pair(name, v, what):
    """an int or a pair (y, x) of ints -> (y, x)"""
    vs = (v, v) if isinstance(v, _NUMBER) and not isinstance(v, bool) else v
    try:
        vs = tuple(vs)
    except TypeError:
        raise ValueError("%s: the %s %r has to be an integer or a pair (y, x)" % (name, what, v))
    if len(vs) != 2:
        raise ValueError("%s: the %s %r has to be an integer or a pair (y, x)" % (name, what, v))
    for e in vs:
        if isinstance(e, bool) or not isinstance(e, _NUMBER) or not np.isfinite(e) or int(e) != e:
            raise ValueError("%s: the %s %r is not an integer" % (name, what, v))
    return int(vs[0]), int(vs[1])


def conv2d_strided_size(nx, ny, ky, kx, stride, shape="same", phase=(0, 0)):
    """-> (my, mx): the size of one decimated output plane, my = (cy - 1 - py) // sy + 1 with (cy, cx) the size of conv2d's output"""
    (sy, sx), (py, px) = _pair("conv2d_strided", stride, "stride"), _pair("conv2d_strided", phase, "phase")
    try:
        (cy, cx), _ = conv2d_size(nx, ny, ky, kx, shape)
    except ValueError:
        raise ValueError("conv2d_strided: unknown shape %r (full, same or valid)" % (shape,))
    return (cy - 1 - py) // sy + 1, (cx - 1 - px) // sx + 1


def conv2d_strided(nx, ny, L, kernel, stride, shape="same", phase=(0, 0)):
    """Blur, then keep every s-th pixel, K = S B, applied without a matrix: the operator of super-resolution.  Images, window and shape
    as conv2d (L column-major planes of ny x nx, one ky x kx window of up to 31 x 31, zero padding; the shape gives the size (cy, cx)
    and the crop offset (oy, ox) of the un-decimated convolution).  stride: s or (sy, sx), 1 .. 4 each; phase: p or (py, px) with
    0 <= py < min(sy, cy), 0 <= px < min(sx, cx).  out(y, x) = sum_{i, j} kernel[i, j] in(y sy + py + oy - i, x sx + px + ox - j),
    my x mx = conv2d_strided_size(..) outputs per plane: the rows (y sy + py, x sx + px) of conv2d's matrix.  The adjoint is the
    fractionally strided ("transposed") convolution."""
    nx, ny, L = [_integer("conv2d_strided", name, v, loose=True) for name, v in (("nx", nx), ("ny", ny), ("L", L))]
    kernel = _conv_window("conv2d_strided", kernel)
    ky, kx = kernel.shape
    if not isinstance(shape, str) or shape not in ("full", "same", "valid"):
        raise ValueError("conv2d_strided: unknown shape %r (full, same or valid)" % (shape,))
    (sy, sx), (py, px) = _pair("conv2d_strided", stride, "stride"), _pair("conv2d_strided", phase, "phase")
    for name, s in (("sy", sy), ("sx", sx)):
        if not 1 <= s <= CONV2D_STRIDED_MAX_STRIDE:
            raise ValueError("conv2d_strided: the stride %s = %d has to be 1 .. %d" % (name, s, CONV2D_STRIDED_MAX_STRIDE))
    (cy, cx), _ = conv2d_size(nx, ny, ky, kx, shape)
    if cy < 1 or cx < 1:
        raise ValueError("conv2d_strided: the window (%d x %d) is larger than the image (%d x %d): the valid part is empty" % (ky, kx, ny, nx))
    for name, p, s, c in (("py", py, sy, cy), ("px", px, sx, cx)):
        if not 0 <= p < min(s, c):
            raise ValueError("conv2d_strided: the phase %s = %d has to be 0 .. %d (below the stride and the size of the convolution)" % (name, p, min(s, c) - 1))
    my, mx = (cy - 1 - py) // sy + 1, (cx - 1 - px) // sx + 1
    if nx * ny >= 2 ** 31 or my * mx >= 2 ** 31:
        raise ValueError("conv2d_strided: a plane of %d elements; it has to stay below 2^31" % max(nx * ny, my * mx))
    if max(nx, ny) >= 2 ** 31 - 1024 - CONV2D_MAX_WINDOW:
        raise ValueError("conv2d_strided: a side of %d pixels; it has to stay below 2^31 - 1055" % max(nx, ny))
    sz = [L * my * mx, L * ny * nx]
    data = [nx, ny, L, kernel, shape, sy, sx, py, px]
    return lambda row, col, nrows, ncols: [["conv2d_strided", row, col, data], sz]


RADON2D_MAX_SIDE = 8192
RADON2D_MAX_ANGLES = 4096


def _radon2d_number(name, v):
    if isinstance(v, bool) or not isinstance(v, _NUMBER):
        raise ValueError("radon2d: %s = %r is not a number" % (name, v))
    return float(v)


def radon2d_ndet(nx, ny, spacing=1.0):
    """the default detector length of radon2d: 2 ceil(hypot(nx, ny) / (2 spacing)) + 1 bins see every pixel at every angle"""
    return 2 * int(math.ceil(math.hypot(nx, ny) / (2.0 * spacing))) + 1


def radon2d(nx, ny, L, angles, ndet=None, spacing=1.0, shift=0.0):
    """The parallel-beam projector of tomography (Joseph's method), applied without a matrix, and its exact transpose.  Domain: L
    column-major planes of ny x nx, element (y, x, c) at y + x ny + c nx ny.  Range: L sinograms, bin d of angle a of plane c at
    d + a ndet + c ndet na.  Pixel centres sit at X = x - (nx - 1) / 2, Y = y - (ny - 1) / 2 (pixel size 1); a point projects to
    s = X cos(theta) + Y sin(theta), and bin d sits at s_d = (d - (ndet - 1) / 2) spacing + shift.  angles: radians, up to 4096;
    ndet: None for radon2d_ndet(nx, ny, spacing); 0.5 <= spacing <= 8.  Per angle the ray is marched over the rows if
    |cos| >= |sin| and over the columns otherwise, and interpolated linearly along the other axis; a matrix entry is the
    interpolation weight times 1 / max(|cos|, |sin|).  Only five numbers per angle are stored."""
    nx, ny = _integer("radon2d", "nx", nx, RADON2D_MAX_SIDE), _integer("radon2d", "ny", ny, RADON2D_MAX_SIDE)
    L = _integer("radon2d", "L", L)
    if ndet is not None:
        ndet = _integer("radon2d", "ndet", ndet)
    try:
        angles = np.array(angles, dtype=np.float64, copy=True)
    except (TypeError, ValueError):
        raise ValueError("radon2d: the angles have to be a vector of numbers")
    if angles.ndim == 0:
        angles = angles.reshape(1)
    if angles.ndim != 1 or angles.size == 0:
        raise ValueError("radon2d: the angles have to be a non-empty vector, got shape %r" % (angles.shape,))
    if angles.size > RADON2D_MAX_ANGLES:
        raise ValueError("radon2d: %d angles, up to %d are supported" % (angles.size, RADON2D_MAX_ANGLES))
    if not np.isfinite(angles).all():
        raise ValueError("radon2d: the angles hold a non-finite value")
    spacing, shift = _radon2d_number("spacing", spacing), _radon2d_number("shift", shift)
    if not 0.5 <= spacing <= 8:
        raise ValueError("radon2d: spacing = %r has to be from 0.5 to 8" % (spacing,))
    if not np.isfinite(shift):
        raise ValueError("radon2d: shift = %r has to be finite" % (shift,))
    if ndet is None:
        ndet = radon2d_ndet(nx, ny, spacing)
    if ndet > 2 ** 31 - 1025:
        raise ValueError("radon2d: ndet = %d has to be below 2^31 - 1024" % ndet)
    if ndet * angles.size >= 2 ** 31:
        raise ValueError("radon2d: a sinogram of %d elements; it has to stay below 2^31" % (ndet * angles.size))
    sz = [L * angles.size * ndet, L * ny * nx]
    data = [nx, ny, L, angles, ndet, spacing, shift]
    return lambda row, col, nrows, ncols: [["radon2d", row, col, data], sz]


FANBEAM2D_MAX_SIDE = 8192
FANBEAM2D_MAX_VIEWS = 4096
FANBEAM2D_MAX_FAN_DEGREES = 30.0
FANBEAM2D_MAX_MARGIN = 5
FANBEAM2D_SLACK = 0.25


def _fanbeam2d_number(name, v):
    if isinstance(v, bool) or not isinstance(v, _NUMBER):
        raise ValueError("fanbeam2d: %s = %r is not a number" % (name, v))
    return float(v)


def _fanbeam2d_scanner(nx, ny, source_distance, detector_distance, spacing, detector):
    """the checks fanbeam2d and fanbeam2d_ndet share -> (R, D, spacing, curved)"""
    R = _fanbeam2d_number("source_distance", source_distance)
    D = R if detector_distance is None else _fanbeam2d_number("detector_distance", detector_distance)
    spacing = _fanbeam2d_number("spacing", spacing)
    if not isinstance(detector, str) or detector not in ("flat", "curved"):
        raise ValueError("fanbeam2d: unknown detector %r (flat or curved)" % (detector,))
    if not 0.5 <= spacing <= 8:
        raise ValueError("fanbeam2d: spacing = %r has to be from 0.5 to 8" % (spacing,))
    if not (np.isfinite(R) and R > 0):
        raise ValueError("fanbeam2d: source_distance = %r has to be positive and finite" % (R,))
    if not (np.isfinite(D) and D > 0):
        raise ValueError("fanbeam2d: detector_distance = %r has to be positive and finite" % (D,))
    closest = math.hypot(nx, ny) / 2.0 + 1.0
    if not R >= closest:
        raise ValueError("fanbeam2d: source_distance = %r puts the source inside the image's circumscribed circle or less than a pixel off it; "
                         "it has to be at least %r" % (R, closest))
    return R, D, spacing, detector == "curved"


def fanbeam2d_ndet(nx, ny, source_distance, detector_distance=None, spacing=1.0, detector="flat"):
    """the default detector length of fanbeam2d: the smallest odd count of bins whose outermost rays pass outside the image's
    circumscribed circle at every view, 2 ceil(u / spacing) + 1 with u = D tan(asin(hd / R)) on a flat detector and D asin(hd / R) on a
    curved one, hd = hypot(nx, ny) / 2"""
    nx, ny = _integer("fanbeam2d", "nx", nx, FANBEAM2D_MAX_SIDE), _integer("fanbeam2d", "ny", ny, FANBEAM2D_MAX_SIDE)
    R, D, spacing, curved = _fanbeam2d_scanner(nx, ny, source_distance, detector_distance, spacing, detector)
    need = math.asin(math.hypot(nx, ny) / 2.0 / R)
    u = D * need if curved else D * math.tan(need)
    return 2 * int(math.ceil(u / spacing)) + 1


def fanbeam2d(nx, ny, L, angles, source_distance, detector_distance=None, ndet=None, spacing=1.0, shift=0.0, detector="flat"):
    """The fan-beam projector of tomography (a point source, Joseph's method), applied without a matrix, and its exact transpose.
    Domain and range as radon2d: L column-major planes of ny x nx, element (y, x, c) at y + x ny + c nx ny; L sinograms, bin d of view
    a of plane c at d + a ndet + c ndet na.  Pixel centres sit at X = x - (nx - 1) / 2, Y = y - (ny - 1) / 2.  At view beta (radians,
    up to 4096) the detector axis is e = (cos, sin), the central ray n = (-sin, cos) and the source S = -R n, R = source_distance in
    pixels, at least hypot(nx, ny) / 2 + 1.  Bin d sits at u_d = (d - (ndet - 1) / 2) spacing + shift along a detector at distance
    D = detector_distance from the source (None: D = R, a virtual detector through the rotation centre); its ray leaves S at the fan
    angle gamma_d = atan(u_d / D) (detector "flat") or u_d / D ("curved", equiangular) in direction sin(gamma) e + cos(gamma) n.  With
    D = R -> infinity the flat geometry tends to radon2d(.., spacing, shift).  ndet: None for fanbeam2d_ndet(..); 0.5 <= spacing <= 8.
    Per view the rays are marched over the rows if |cos| >= |sin| and over the columns otherwise, interpolated linearly along the other
    axis; no ray may be more than 30 degrees off the central one.  The adjoint gathers, per pixel and view, a window of 2 m + 2
    candidate bins, m = ceil(D / (R - hc) / (spacing cos(gamma_max)) + 1 / 4) with hc = hypot(nx - 1, ny - 1) / 2, and m <= 5 is
    required: a source at R >= hypot(nx, ny) with the default detector always passes.  Stored: five numbers per view, two per bin."""
    nx, ny = _integer("fanbeam2d", "nx", nx, FANBEAM2D_MAX_SIDE), _integer("fanbeam2d", "ny", ny, FANBEAM2D_MAX_SIDE)
    L = _integer("fanbeam2d", "L", L)
    if ndet is not None:
        ndet = _integer("fanbeam2d", "ndet", ndet)
    try:
        angles = np.array(angles, dtype=np.float64, copy=True)
    except (TypeError, ValueError):
        raise ValueError("fanbeam2d: the angles have to be a vector of numbers")
    if angles.ndim == 0:
        angles = angles.reshape(1)
    if angles.ndim != 1 or angles.size == 0:
        raise ValueError("fanbeam2d: the angles have to be a non-empty vector, got shape %r" % (angles.shape,))
    if angles.size > FANBEAM2D_MAX_VIEWS:
        raise ValueError("fanbeam2d: %d views, up to %d are supported" % (angles.size, FANBEAM2D_MAX_VIEWS))
    if not np.isfinite(angles).all():
        raise ValueError("fanbeam2d: the angles hold a non-finite value")
    shift = _fanbeam2d_number("shift", shift)
    if not np.isfinite(shift):
        raise ValueError("fanbeam2d: shift = %r has to be finite" % (shift,))
    R, D, spacing, curved = _fanbeam2d_scanner(nx, ny, source_distance, detector_distance, spacing, detector)
    if ndet is None:
        ndet = fanbeam2d_ndet(nx, ny, R, D, spacing, detector)
    if ndet > 2 ** 31 - 1025:
        raise ValueError("fanbeam2d: ndet = %d has to be below 2^31 - 1024" % ndet)
    if ndet * angles.size >= 2 ** 31:
        raise ValueError("fanbeam2d: a sinogram of %d elements; it has to stay below 2^31" % (ndet * angles.size))
    fan = 0.0
    for d in (0, ndet - 1):
        u = (d - (ndet - 1) / 2.0) * spacing + shift
        fan = max(fan, abs(u / D if curved else math.atan2(u, D)))
    if not math.degrees(fan) <= FANBEAM2D_MAX_FAN_DEGREES:
        raise ValueError("fanbeam2d: the outermost ray is %.6g degrees off the central ray; half fans up to %g degrees are supported"
                         % (math.degrees(fan), FANBEAM2D_MAX_FAN_DEGREES))
    margin = math.ceil(D / (R - math.hypot(nx - 1, ny - 1) / 2.0) / (spacing * math.cos(fan)) + FANBEAM2D_SLACK)
    if margin > FANBEAM2D_MAX_MARGIN:
        raise ValueError("fanbeam2d: the candidate window of the adjoint needs a margin of %d bins, up to %d are supported (a source farther away, "
                         "a detector nearer to it or a larger spacing)" % (margin, FANBEAM2D_MAX_MARGIN))
    sz = [L * angles.size * ndet, L * ny * nx]
    data = [nx, ny, L, angles, R, D, ndet, spacing, shift, detector]
    return lambda row, col, nrows, ncols: [["fanbeam2d", row, col, data], sz]


SAMPLE2D_MAX_SIDE = 16384


def sample2d(nx, ny, L, x, y):
    """Bilinear resampling of an image at M arbitrary positions, applied without a matrix, and its exact transpose.  Domain: L
    column-major planes of ny x nx, element (yy, xx, c) at yy + xx ny + c nx ny.  Range: L planes of M samples, sample i of plane c at
    i + c M, M = len(x) = len(y).  x[i], y[i] are pixel coordinates with the pixel centres at the integers (x along the nx axis); they
    are rounded once to the precision of the problem.  Sample i is the bilinear interpolant of the four pixels around (y[i], x[i]);
    pixels outside the image count as zero, and a position outside [-1, nx) x [-1, ny) gives a zero row.  A warp by a flow field
    (dx, dy) is x = X + dx, y = Y + dy with X, Y the pixel grid in column-major order and M = nx ny.  The device stores the 2 M
    positions, M int32 sample indices sorted by cell and (ny + 1)(nx + 1) + 1 int32 cell offsets: about a quarter of the two sides of
    the sparse matrix.  Many samples inside one cell are correct but slow in the transpose."""
    nx, ny = _integer("sample2d", "nx", nx, SAMPLE2D_MAX_SIDE), _integer("sample2d", "ny", ny, SAMPLE2D_MAX_SIDE)
    L = _integer("sample2d", "L", L)
    pos = []
    for name, v in (("x", x), ("y", y)):
        v = _numbers("sample2d", v, "%s has to be a vector of numbers" % name)
        if v.ndim == 0:
            v = v.reshape(1)
        if v.ndim != 1:
            raise ValueError("sample2d: %s has to be a vector, got shape %r" % (name, v.shape))
        pos.append(v)
    x, y = pos
    if x.size != y.size:
        raise ValueError("sample2d: %d x positions and %d y positions" % (x.size, y.size))
    if x.size == 0:
        raise ValueError("sample2d: the positions are empty")
    if not (np.isfinite(x).all() and np.isfinite(y).all()):
        raise ValueError("sample2d: the positions hold a non-finite value")
    if x.size >= 2 ** 31 or L * x.size >= 2 ** 31:
        raise ValueError("sample2d: M = %d samples on L = %d planes; M and L M have to stay below 2^31" % (x.size, L))
    sz = [L * x.size, L * ny * nx]
    data = [nx, ny, L, x, y]
    return lambda row, col, nrows, ncols: [["sample2d", row, col, data], sz]


FFT2D_MAX_SIDE = 2048


def fft2d(nx, ny, L=1):
    """The unitary 2-D discrete Fourier transform of L complex images of ny x nx, applied without a matrix as a real 2 L N x 2 L N
    operator, N = nx ny; its transpose is the unitary inverse transform, K^T K = I.  Domain: real parts first, re_c[p] at c N + p and
    im_c[p] at (L + c) N + p with p = y + x ny -- the domain layout of gradient2d(nx, ny, 2 L), so gradient2d(nx, ny, 2) followed by
    sum_norm2(4, False, ...) is the isotropic TV of one complex image.  Range: the same layout over frequencies q = ky + kx ny in
    standard FFT order, DC at q = 0:  Y[ky, kx] = s sum X[y, x] exp(-2 pi i (ky y / ny + kx x / nx)), s = 1 / sqrt(nx ny).
    nx and ny are powers of two from 1 to 2048 (a side of 1 makes the transform one-dimensional).  There is no sampling mask in the
    block: a mask goes into the data term as a 0/1 coefficient, sum_1d("square", 1, d, mask, 0, 0) on v = F u, as in
    examples/tv_mri.py.  The device holds a table of 2 max(nx, ny) values and one work buffer of 2 L N values.
    Preconditioning: the row and column sums of |K|^alpha are known in closed form, but a diagonal preconditioner of a dense
    orthogonal operator is very conservative (the sums are about 1.27 sqrt(N) at alpha = 1 where the operator's norm is 1): use
    prob.set_scaling_identity(), as the example does."""
    for name, v in (("nx", nx), ("ny", ny)):
        n = _integer("fft2d", name, v)
        if n > FFT2D_MAX_SIDE or n & (n - 1):
            raise ValueError("fft2d: %s = %r has to be a power of two from 1 to %d" % (name, v, FFT2D_MAX_SIDE))
    nx, ny, L = int(nx), int(ny), _integer("fft2d", "L", L)
    if 2 * L * nx * ny >= 2 ** 31:
        raise ValueError("fft2d: L = %d images of %d x %d; 2 L nx ny has to stay below 2^31" % (L, nx, ny))
    sz = [2 * L * nx * ny, 2 * L * nx * ny]
    data = [nx, ny, L]
    return lambda row, col, nrows, ncols: [["fft2d", row, col, data], sz]


SENSE2D_MAX_COILS = 64


def sense2d(nx, ny, maps, L=1):
    """The multi-coil Fourier operator of SENSE-type parallel MRI, K u = [ F (sigma_1 . u) ; .. ; F (sigma_C . u) ], applied without a
    matrix as a real 2 L C N x 2 L N operator, N = nx ny: F is fft2d, "." the pointwise complex product, sigma_c the complex sensitivity
    map of coil c; K^T y = sum_c conj(sigma_c) . F^H y_c.  The coil product happens while the first pass loads, the coil sum in registers
    while the last pass of the transpose stores: there is no field of C intermediate images and no atomic.  Domain: the domain of
    fft2d(nx, ny, L), re_l[p] at l N + p and im_l[p] at (L + l) N + p with p = y + x ny (L frames of a dynamic series or several contrasts
    share the maps).  Range: the range of fft2d(nx, ny, L C), image j = l C + c holds coil c of image l, so a sampling mask is coefficient
    c of sum_1d("square", 1, d, mask, 0, 0) on all C k-space images, as in examples/sense_mri.py.  nx and ny are powers of two from 1 to
    2048, C = 1 .. 64, 2 L C nx ny < 2^31.
    maps: a complex (C, ny, nx) array m[c, y, x], a complex (C, N) array (each plane flattened with y fastest), a sequence of C complex
    planes, each an (ny, nx) array or a vector of N values, or a pair (re, im) of real arrays of those shapes.  Every value is rounded once
    to the precision of the problem and the operator is defined with the rounded maps; zeros are legal (a map may vanish everywhere),
    non-finite values are refused.  With C = 1 and sigma = 1 the block is fft2d up to the signs of zeros.  The device holds the maps
    (2 C N values), fft2d's table and one work buffer of 2 L C N values.
    Preconditioning: the phase of the maps shifts every angle of the Fourier matrix, so the sums of |K|^e have no closed form except at
    e = 2 and the block returns upper BOUNDS, row (l, c, q): f(e) s^e sum_p |sigma_c(p)|^e, column of pixel p: f(e) s^e N sum_c
    |sigma_c(p)|^e, s = 1 / sqrt(N), f(e) = max(1, 2^(1 - e/2)); S <= Sbar <= 2^|1 - e/2| S, exact at e = 2.  Bounds from above only
    shrink the diagonal steps; convergence (Pock & Chambolle 2011, Lemma 2) holds unchanged.  As for fft2d a diagonal preconditioner of
    this dense operator is very conservative: use prob.set_scaling_identity(), as the example does (with sum_c |sigma_c|^2 = 1 the
    operator's norm is 1)."""
    for name, v in (("nx", nx), ("ny", ny)):
        n = _integer("sense2d", name, v)
        if n > FFT2D_MAX_SIDE or n & (n - 1):
            raise ValueError("sense2d: %s = %r has to be a power of two from 1 to %d" % (name, v, FFT2D_MAX_SIDE))
    nx, ny, L = int(nx), int(ny), _integer("sense2d", "L", L)
    N = nx * ny

    def array(v, kinds, what):
        try:
            a = np.asarray(v)
            if a.dtype.kind not in kinds:
                raise TypeError
            return a
        except (TypeError, ValueError):
            raise ValueError("sense2d: %s" % what)

    def planes(a, what):
        """a (C, ny, nx), (C, N), (ny, nx) or (N,) array -> (C, N), p = y + x ny"""
        if a.ndim == 3 and a.shape[1:] == (ny, nx):
            return a.transpose(0, 2, 1).reshape(a.shape[0], N)
        if a.ndim == 2 and a.shape[1] == N:
            return a
        raise ValueError("sense2d: %s have shape %r; they are a (C, ny, nx) = (C, %d, %d) array, a (C, N) = (C, %d) array or a sequence of C planes"
                         % (what, a.shape, ny, nx, N))

    def plane(a, what):
        if a.ndim == 2 and a.shape == (ny, nx):
            a = a.reshape(-1, order="F")
        if a.ndim != 1 or a.size != N:
            raise ValueError("sense2d: %s has shape %r; a plane is a vector of nx ny = %d values or an (ny, nx) = (%d, %d) array" % (what, a.shape, N, ny, nx))
        return a

    def parts(v, kinds, what):
        """one of the accepted forms, with values of the given dtype kinds -> (C, N)"""
        refusal = "%s have to be %s" % (what, "complex numbers, or a pair (re, im) of real arrays" if kinds == "c" else "real numbers")
        if isinstance(v, (list, tuple)):                     # a sequence of planes
            if len(v) == 0:
                raise ValueError("sense2d: %s are empty" % what)
            return np.stack([plane(array(p, kinds, refusal), "plane %d of %s" % (i, what)) for i, p in enumerate(v)])
        return planes(array(v, kinds, refusal), what)

    def real(v):
        try:
            return np.asarray(v).dtype.kind in "iuf"
        except (TypeError, ValueError):
            return False

    if isinstance(maps, (list, tuple)) and len(maps) == 2 and real(maps[0]) and real(maps[1]):
        re, im = parts(maps[0], "iuf", "the real parts of the maps"), parts(maps[1], "iuf", "the imaginary parts of the maps")
        if re.shape != im.shape:
            raise ValueError("sense2d: the real parts are %d planes and the imaginary parts %d" % (re.shape[0], im.shape[0]))
    else:
        m = parts(maps, "c", "the maps")
        re, im = m.real, m.imag
    C = int(re.shape[0])
    if C < 1 or C > SENSE2D_MAX_COILS:
        raise ValueError("sense2d: the maps are C = %d planes; C has to be from 1 to %d" % (C, SENSE2D_MAX_COILS))
    flat = np.concatenate([np.asarray(re, np.float64).reshape(-1), np.asarray(im, np.float64).reshape(-1)])
    if not np.isfinite(flat).all():
        raise ValueError("sense2d: the maps hold a non-finite value")
    if 2 * L * C * N >= 2 ** 31:
        raise ValueError("sense2d: L = %d images of %d x %d with C = %d coils; 2 L C nx ny has to stay below 2^31" % (L, nx, ny, C))
    sz = [2 * L * C * N, 2 * L * N]
    data = [nx, ny, L, C, flat]
    return lambda row, col, nrows, ncols: [["sense2d", row, col, data], sz]


WAVELET2D_MAX_TAPS = 16
WAVELET2D_ORTHO_TOLERANCE = 1e-12


def wavelet2d_taps(name):
    """the float64 low-pass taps h of a named orthogonal wavelet ("haar", "db2", "db3"), from closed forms; g[t] = (-1)^t h[T-1-t]"""
    if name == "haar":
        d = np.sqrt(2.0)
        return np.array([1.0 / d, 1.0 / d])
    if name == "db2":
        s, d = np.sqrt(3.0), 4.0 * np.sqrt(2.0)
        return np.array([(1.0 + s) / d, (3.0 + s) / d, (3.0 - s) / d, (1.0 - s) / d])
    if name == "db3":
        a = np.sqrt(10.0)
        b, d = np.sqrt(5.0 + 2.0 * a), 16.0 * np.sqrt(2.0)
        return np.array([(1.0 + a + b) / d, (5.0 + a + 3.0 * b) / d, (10.0 - 2.0 * a + 2.0 * b) / d,
                         (10.0 - 2.0 * a - 2.0 * b) / d, (5.0 + a - 3.0 * b) / d, (1.0 + a - b) / d])
    raise ValueError("wavelet2d: the wavelet %r is not one of 'haar', 'db2', 'db3'; any other filter is given as its low-pass taps" % (name,))


def wavelet2d(nx, ny, L=1, wavelet="haar", levels=1):
    """The orthogonal, periodised, separable multi-level discrete wavelet transform (Mallat's pyramid) of L real planes of ny x nx,
    applied without a matrix as a real L N x L N operator, N = nx ny; its transpose is the inverse transform, K^T K = I.  Pixel (y, x)
    of plane c at c N + y + x ny, as in every other block; the range is the in-place quadrant layout with the approximation at the top
    left, so wavelet2d(nx, ny, 2, ...) followed by sum_norm2(2, False, "abs", ...) is the l1-norm of the complex coefficients of the
    image fft2d and gradient2d(nx, ny, 2) act on.  wavelet: "haar", "db2", "db3" (wavelet2d_taps) or the low-pass taps h of an
    orthogonal filter of even length 2 .. 16; they are accepted if |sum_k h[k] h[k+2l] - delta_l| <= 1e-12 for every l (a table
    truncated to ten digits is refused) and rounded once to the precision of the problem; g[t] = (-1)^t h[T-1-t].  One level of a line
    of m values: lo[k] = sum_t h[t] x[(2k+t) mod m], hi[k] = sum_t g[t] x[(2k+t) mod m].  A side greater than 1 has to be divisible by
    2^levels with side / 2^(levels-1) >= T, a side of 1 makes the transform one-dimensional, 1 x 1 is refused, L N < 2^31; sides need
    not be powers of two.  The device holds one work buffer of 5/16 L N values (3/4 with a side of 1).
    Preconditioning: the row and column sums of |K|^alpha are computed from the filter, but a diagonal preconditioner of an orthogonal
    operator is conservative (the operator's norm is 1, the sums grow with the support of the coarse functions): use
    prob.set_scaling_identity(), as examples/wavelet_mri.py does."""
    nx, ny, L, levels = [_integer("wavelet2d", name, v) for name, v in (("nx", nx), ("ny", ny), ("L", L), ("levels", levels))]
    if isinstance(wavelet, str):
        taps = wavelet2d_taps(wavelet)
    else:
        taps = _numbers("wavelet2d", wavelet, "the wavelet has to be a name or a vector of taps")
        if taps.ndim != 1:
            raise ValueError("wavelet2d: the taps have to be a vector, got shape %r" % (taps.shape,))
        if taps.size < 2 or taps.size > WAVELET2D_MAX_TAPS or taps.size % 2:
            raise ValueError("wavelet2d: %d taps; the filter has to have an even number of taps from 2 to %d" % (taps.size, WAVELET2D_MAX_TAPS))
        if not np.isfinite(taps).all():
            raise ValueError("wavelet2d: the taps hold a non-finite value")
        T = taps.size
        defect = max(abs(float(np.dot(taps[:T - 2 * l], taps[2 * l:])) - (1.0 if l == 0 else 0.0)) for l in range(T // 2))
        if not defect <= WAVELET2D_ORTHO_TOLERANCE:
            raise ValueError("wavelet2d: the taps are not orthonormal: |sum_k h[k] h[k+2l] - delta_l| = %.3g for some l, above %g (taps "
                             "rounded from exact values miss by about 1e-15; a table truncated to fewer digits is refused)" % (defect, WAVELET2D_ORTHO_TOLERANCE))
    T = int(taps.size)
    if nx == 1 and ny == 1:
        raise ValueError("wavelet2d: a plane of 1 x 1 has nothing to transform")
    for name, v in (("nx", nx), ("ny", ny)):
        if v == 1:
            continue
        if levels > 30 or v % 2 ** levels:
            raise ValueError("wavelet2d: %s = %d is not divisible by 2^levels = 2^%d" % (name, v, levels))
        if v // 2 ** (levels - 1) < T:
            raise ValueError("wavelet2d: %s = %d at %d levels: the coarsest line holds %d values, fewer than the filter's %d taps" % (name, v, levels, v // 2 ** (levels - 1), T))
    if L * nx * ny >= 2 ** 31:
        raise ValueError("wavelet2d: L = %d planes of %d x %d; L nx ny has to stay below 2^31" % (L, nx, ny))
    sz = [L * nx * ny, L * nx * ny]
    data = [nx, ny, L, taps, levels]
    return lambda row, col, nrows, ncols: [["wavelet2d", row, col, data], sz]


SYM_GRADIENT2D_MAX_SIZE = 2 ** 53          # sizes travel as doubles


def sym_gradient2d(nx, ny, L=1, w=math.sqrt(0.5)):
    """The symmetrised gradient E of a vector field on L channels of an ny x nx grid, applied without a matrix: the second-order
    operator of total generalised variation, K = [grad -I ; 0 E].  N = nx ny, pixel (y, x) at p = y + x ny.  Domain, 2 L N values, the
    range layout of gradient2d(nx, ny, L): vx_c[p] at c N + p, vy_c[p] at (L + c) N + p.  Range, 3 L N values: exx_c[p] at c N + p,
    eyy_c[p] at (L + c) N + p, exy_c[p] at (2 L + c) N + p, so sum_norm2(3, False, ..) groups per channel and pixel.  Backward
    differences with the boundary handling of the divergence (Bx = -Dx^T, By = -Dy^T of gradient2d's forward differences):
    exx = Bx vx, eyy = By vy, exy = w (By vx + Bx vy).  w = sqrt(1/2): the 2-norm of (exx, eyy, exy) is the Frobenius norm of the
    symmetrised Jacobian; w = 0.5: the entries of (J + J^T) / 2."""
    nx, ny, L = [_integer("sym_gradient2d", name, v) for name, v in (("nx", nx), ("ny", ny), ("L", L))]
    if isinstance(w, bool) or not isinstance(w, _NUMBER) or not np.isfinite(w):
        raise ValueError("sym_gradient2d: w = %r is not a finite number" % (w,))
    w = float(w)
    if w == 0:
        raise ValueError("sym_gradient2d: w has to be non-zero")
    if 3 * L * nx * ny > SYM_GRADIENT2D_MAX_SIZE:
        raise ValueError("sym_gradient2d: 3 L nx ny = %d rows; the size has to stay within 2^53" % (3 * L * nx * ny))
    sz = [3 * L * nx * ny, 2 * L * nx * ny]
    data = [nx, ny, L, w]
    return lambda row, col, nrows, ncols: [["sym_gradient2d", row, col, data], sz]


HESSIAN2D_MAX_SIZE = 2 ** 53               # sizes travel as doubles


def hessian2d(nx, ny, L=1, w=math.sqrt(0.5), components=3):
    """The second-order differences H = E grad of L channels of an ny x nx grid, applied without a matrix and without the intermediate
    field: the operator of second-order total variation (TV^2, bounded Hessian), of the TV + TV^2 infimal convolution and of the
    Hessian-Schatten-norm regularisers.  grad is gradient2d(nx, ny, L), E is sym_gradient2d(nx, ny, L, w), and the products have the
    bits of the two blocks chained.  N = nx ny, pixel (y, x) at p = y + x ny.  Domain, L N values: u_c[p] at c N + p.
    components = 3: range of 3 L N values in the layout of sym_gradient2d, hxx_c[p] at c N + p, hyy_c[p] at (L + c) N + p, hxy_c[p] at
    (2 L + c) N + p, so sum_norm2(3, False, ..) groups per channel and pixel; with w = sqrt(1/2) its 2-norm is the Frobenius norm of the
    Hessian.  components = 4: range of 4 L N values, the planes (hxx, hxy, hxy, hyy) at (k L + c) N + p, the column-major symmetric
    2 x 2 matrix sum_eigen_2x2(False, ..) reads; w = 0.5 gives the true Hessian.  The default of w is sqrt(1/2) whatever components
    is.  Interior rows: hxx and hyy are (1, -2, 1), hxy is the 7-point stencil with centre -2 w; the edges lose the masked terms, and
    nx = 1 or ny = 1 are legal (hxx or hyy and hxy are then zero).  w has to be non-zero, as in sym_gradient2d."""
    nx, ny, L = [_integer("hessian2d", name, v) for name, v in (("nx", nx), ("ny", ny), ("L", L))]
    if isinstance(w, bool) or not isinstance(w, _NUMBER) or not np.isfinite(w):
        raise ValueError("hessian2d: w = %r is not a finite number" % (w,))
    w = float(w)
    if w == 0:
        raise ValueError("hessian2d: w has to be non-zero")
    if isinstance(components, bool) or not isinstance(components, _NUMBER) or components not in (3, 4):
        raise ValueError("hessian2d: components = %r has to be 3 or 4" % (components,))
    components = int(components)
    if components * L * nx * ny > HESSIAN2D_MAX_SIZE:
        raise ValueError("hessian2d: components L nx ny = %d rows; the size has to stay within 2^53" % (components * L * nx * ny))
    sz = [components * L * nx * ny, L * nx * ny]
    data = [nx, ny, L, w, components]
    return lambda row, col, nrows, ncols: [["hessian2d", row, col, data], sz]


TENSOR_GRADIENT2D_MAX_SIZE = 2 ** 53       # sizes travel as doubles


def tensor_gradient2d(nx, ny, L, tensor):
    """K = T grad on L channels of an ny x nx grid, applied without a matrix: the gradient weighted per pixel by a scalar (edge-weighted
    TV, g |grad u| with g = exp(-beta |grad f|^gamma)), by one weight per axis, or by a symmetric 2 x 2 tensor (the image-driven diffusion
    tensor D^(1/2) of anisotropic Huber-L1 stereo / flow and anisotropic TGV).  N = nx ny, pixel (y, x) at p = y + x ny.  Domain, L N
    values: u_c[p] at c N + p.  Range, 2 L N values, the range layout of gradient2d(nx, ny, L): gx_c[p] at c N + p, gy_c[p] at
    (L + c) N + p, so sum_norm2(2 L, False, ..) or sum_norm2(2, False, ..) group as they do behind gradient2d.  The tensor is one
    field shared by all channels, k planes of N values, each rounded once to the precision of the problem:
        k = 1  g        gx = g dx,         gy = g dy
        k = 2  a, c     gx = a dx,         gy = c dy
        k = 3  a, b, c  gx = a dx + b dy,  gy = b dx + c dy
    with dx, dy the forward differences of gradient2d (zero in the last column / row).  tensor: a (k, N) array, a (k, ny, nx) array
    t[i, y, x] (each plane is flattened with y fastest), a vector of N values (k = 1), or a sequence of k planes, each a vector of N
    values or an (ny, nx) array.  Zeros are legal (an edge that is switched off); non-finite values are refused.  With g = 1 the block is
    gradient2d bit for bit.  The device stores the k N values of the tensor and nothing per channel; the sparse matrix of the same
    operator stores 4 (k = 1, 2) or 6 (k = 3) entries with their indices per pixel and channel, once for each side."""
    nx, ny, L = [_integer("tensor_gradient2d", name, v) for name, v in (("nx", nx), ("ny", ny), ("L", L))]
    N = nx * ny
    if 2 * L * N > TENSOR_GRADIENT2D_MAX_SIZE:
        raise ValueError("tensor_gradient2d: 2 L nx ny = %d rows; the size has to stay within 2^53" % (2 * L * N))

    def plane(v, what):
        v = _numbers("tensor_gradient2d", v, "%s has to be an array of numbers" % what)
        if v.ndim == 2 and v.shape == (ny, nx):
            v = v.reshape(-1, order="F")                   # p = y + x ny
        if v.ndim != 1 or v.size != N:
            raise ValueError("tensor_gradient2d: %s has shape %r; a plane is a vector of nx ny = %d values or an (ny, nx) = (%d, %d) array"
                             % (what, v.shape, N, ny, nx))
        return v

    if isinstance(tensor, (list, tuple)) and len(tensor) > 0 and not np.isscalar(tensor[0]):
        planes = [plane(v, "plane %d of the tensor" % i) for i, v in enumerate(tensor)]
    else:
        t = _numbers("tensor_gradient2d", tensor, "the tensor has to be an array of numbers")
        if t.ndim == 1:
            planes = [plane(t, "the tensor")]
        elif t.ndim == 2:
            planes = [plane(v, "plane %d of the tensor" % i) for i, v in enumerate(t)]
        elif t.ndim == 3:
            planes = [plane(v, "plane %d of the tensor" % i) for i, v in enumerate(t)]
        else:
            raise ValueError("tensor_gradient2d: the tensor has shape %r; it is a (k, N) or (k, ny, nx) array or a sequence of k planes" % (t.shape,))
    k = len(planes)
    if k not in (1, 2, 3):
        raise ValueError("tensor_gradient2d: the tensor has k = %d planes; k has to be 1 (scalar), 2 (per axis) or 3 (symmetric tensor)" % k)
    flat = np.concatenate(planes)
    if not np.isfinite(flat).all():
        raise ValueError("tensor_gradient2d: the tensor holds a non-finite value")
    sz = [2 * L * N, L * N]
    data = [nx, ny, L, k, flat]
    return lambda row, col, nrows, ncols: [["tensor_gradient2d", row, col, data], sz]


NONLOCAL_GRADIENT2D_MAX_SIZE = 2 ** 53     # sizes travel as doubles
NONLOCAL_GRADIENT2D_MAX_OFFSETS = 64
NONLOCAL_GRADIENT2D_MAX_REACH = 15         # the reach of conv2d's 31 x 31 window


def nonlocal_window(radius):
    """The offsets (dy, dx) of the full (2 r + 1)^2 - 1 window of radius r, an (M, 2) integer array: dx ascending from -r to r and, for
    each dx, dy ascending from -r to r, (0, 0) left out -- the column-major order of the window's pixels.  nonlocal_window(1) is
    (-1,-1), (0,-1), (1,-1), (-1,0), (1,0), (-1,1), (0,1), (1,1)."""
    r = _integer("nonlocal_window", "radius", radius, NONLOCAL_GRADIENT2D_MAX_REACH)
    return np.array([(dy, dx) for dx in range(-r, r + 1) for dy in range(-r, r + 1) if (dy, dx) != (0, 0)], dtype=np.int64)


def nonlocal_gradient2d(nx, ny, L, offsets, weights):
    """The nonlocal gradient (K u)_m[p] = w_m(p) (u[p + d_m] - u[p]) on L channels of an ny x nx grid, applied without a matrix: the
    operator of nonlocal TV denoising and inpainting (Gilboa-Osher) and of the nonlocal Huber / TV-L1 regularisers of flow and depth.
    N = nx ny, pixel (y, x) at p = y + x ny.  Domain, L N values: u_c[p] at c N + p.  Range, M L N values, displacement-major like the
    gx / gy planes of gradient2d: plane (m, c) at (m L + c) N + p, so sum_norm2(M L, False, ..) or sum_norm2(M, False, ..) group per pixel.
    offsets: an (M, 2) integer array of displacements (dy, dx), 1 <= M <= 64, pairwise distinct, not (0, 0), |dy|, |dx| <= 15
    (nonlocal_window(r) gives a full window).  weights: one plane per displacement, shared by all channels and rounded once to the
    precision of the problem -- an (M, N) array, an (M, ny, nx) array w[m, y, x] (each plane is flattened with y fastest), or a sequence
    of M planes, each a vector of N values or an (ny, nx) array.  Zeros and negative values are legal; non-finite values are refused.
    A term whose target p + d_m lies outside the grid is absent: it has no row entry, and its weight reaches no output.  With offsets
    ((0, 1), (1, 0)) and weights 1 the forward product is gradient2d bit for bit.  The device stores the M N weights and nothing per
    channel; the sparse matrix of the same operator stores 2 M entries with their indices per pixel and channel, once for each side."""
    name = "nonlocal_gradient2d"
    nx, ny, L = [_integer(name, what, v) for what, v in (("nx", nx), ("ny", ny), ("L", L))]
    N = nx * ny
    off = _numbers(name, offsets, "the offsets have to be an array of numbers")
    if off.ndim != 2 or off.shape[1] != 2:
        raise ValueError("%s: the offsets have shape %r; they are an (M, 2) array of (dy, dx)" % (name, off.shape))
    M = off.shape[0]
    if M < 1 or M > NONLOCAL_GRADIENT2D_MAX_OFFSETS:
        raise ValueError("%s: M = %d offsets; M has to be 1 .. %d" % (name, M, NONLOCAL_GRADIENT2D_MAX_OFFSETS))
    if not np.isfinite(off).all() or np.any(off != np.floor(off)):
        raise ValueError("%s: the offsets have to be integers" % name)
    off = off.astype(np.int64)
    if np.any(np.all(off == 0, axis=1)):
        raise ValueError("%s: offset %d is (0, 0), which is no displacement" % (name, int(np.flatnonzero(np.all(off == 0, axis=1))[0])))
    if len({(int(dy), int(dx)) for dy, dx in off}) != M:
        raise ValueError("%s: the offsets have to be pairwise distinct" % name)
    if np.abs(off).max() > NONLOCAL_GRADIENT2D_MAX_REACH:
        raise ValueError("%s: an offset reaches beyond %d" % (name, NONLOCAL_GRADIENT2D_MAX_REACH))
    if M * L * N > NONLOCAL_GRADIENT2D_MAX_SIZE:
        raise ValueError("%s: M L nx ny = %d rows; the size has to stay within 2^53" % (name, M * L * N))

    def plane(v, what):
        v = _numbers(name, v, "%s has to be an array of numbers" % what)
        if v.ndim == 2 and v.shape == (ny, nx):
            v = v.reshape(-1, order="F")                   # p = y + x ny
        if v.ndim != 1 or v.size != N:
            raise ValueError("%s: %s has shape %r; a plane is a vector of nx ny = %d values or an (ny, nx) = (%d, %d) array" % (name, what, v.shape, N, ny, nx))
        return v

    if isinstance(weights, (list, tuple)) and len(weights) > 0 and not np.isscalar(weights[0]):
        planes = [plane(v, "plane %d of the weights" % i) for i, v in enumerate(weights)]
    else:
        w = _numbers(name, weights, "the weights have to be an array of numbers")
        if w.ndim not in (2, 3):
            raise ValueError("%s: the weights have shape %r; they are an (M, N) or (M, ny, nx) array or a sequence of M planes" % (name, w.shape))
        planes = [plane(v, "plane %d of the weights" % i) for i, v in enumerate(w)]
    if len(planes) != M:
        raise ValueError("%s: %d planes of weights for M = %d offsets" % (name, len(planes), M))
    flat = np.concatenate(planes)
    if not np.isfinite(flat).all():
        raise ValueError("%s: the weights hold a non-finite value" % name)
    sz = [M * L * N, L * N]
    data = [nx, ny, L, off.reshape(-1).astype(np.float64), flat]
    return lambda row, col, nrows, ncols: [[name, row, col, data], sz]


def diags(nrows, ncols, factors, offsets):
    sz = [nrows, ncols]
    data = [nrows, ncols, np.atleast_1d(np.asarray(factors, dtype=np.float64)),
            np.atleast_1d(np.asarray(offsets, dtype=np.float64))]
    return lambda row, col, nrows_, ncols_: [["diags", row, col, data], sz]


def identity(scal=1):
    return lambda row, col, nrows, ncols: [
        ["diags", row, col, [nrows, ncols, np.array([float(scal)]), np.array([0.0])]], [nrows, ncols]]


def zero():
    return lambda row, col, nrows, ncols: [["zero", row, col, [nrows, ncols]], [nrows, ncols]]
