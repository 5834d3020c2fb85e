"""References for prost.block.wavelet2d, written from the definition (the issue text and the comment at the head of
include/prost/linop/wavelet2d.hpp), never from the code under test.  NumPy only, vectorised pass by pass.

Layout: L real planes of ny x nx, pixel (y, x) of plane c at c N + y + x ny, N = nx ny; the range is the in-place quadrant layout,
the approximation at the top left.  h: the low-pass taps (even length T <= 16), g[t] = (-1)^t h[T-1-t].

  (a) taps(name)          float64 taps: "haar", "db2", "db3" from their closed forms in the pinned order of operations; "lat8" and
                          "lat16": orthonormal filters of length 8 and 16 from rotation angles (lattice factorisation), no table
  (b) product(..)         the restatement in T in the pinned order.  One level on a line of m values: lo[k] = sum_t h[t] x[(2k+t) mod m],
                          hi[k] = sum_t g[t] x[(2k+t) mod m], from +0, t ascending, lows at 0 .. m/2-1, highs at m/2 .. m-1.  Level l
                          acts on the corner (ny >> l) x (nx >> l): the y pass, then the x pass; a side of 1 has no pass.  Transposed:
                          the levels in reverse, x before y; output n is the sum from +0 over t = n mod 2, n mod 2 + 2, .. of
                          h[t] lo[k], then g[t] hi[k], k = ((n - t) / 2) mod (m / 2).  res0: the accumulating form, res0 + value
  (c) matrix(..)          the explicit N x N matrix of one plane in float64, from the dense 1-D one-level matrices by matrix products
  (d) sums(..)            the sums of |K|^alpha over the rows and over the columns of (c), exact zeros absent
  (e) bound(..)           B = (1 + eta)^(2 levels) - 1, eta = gamma_(T+1) sum |h_t|, gamma_n = n u / (1 - n u): a 1-D pass is a T-term
                          dot product with taps rounded to T and | |W1| |_2 <= sum |h_t|; |fl(K x) - K x|_2 <= B |x|_2 per plane
"""
import functools
import math

import numpy as np

# (nx, ny, L, wavelet, levels).  The kernels' dispatch: a level whose corner holds more than 4096 values per plane is one launch of
# tiles of 64 x 32 pixels (32 x 16 positions per sub-band); from the first corner of at most 4096 values on, one workgroup per plane
# finishes the remaining levels (the tail; the transpose begins with it).  Each launch moves 16 bytes per lane (4 values in fp32, 2 in
# fp64) on its load side and on its store side when that side's pointers, column heights and plane strides are multiples of 16 bytes
# and the corner's height (for the loads and stores of a sub-band: half of it) is a multiple of the group, else one value: off at every
# odd element offset (the tests' 1 x 1 diags block in front, the C entry points at offset 1), at heights such as 90, 100, 20 or 12.
CASES = (
    (2, 2, 1, "haar", 1),            # the smallest shape
    (1, 8, 1, "db2", 1), (8, 1, 1, "db2", 1),      # one-dimensional
    (8, 8, 1, "db2", 2),             # the coarsest line equals T: the halo is the whole line
    (12, 20, 1, "db3", 2),           # no powers of two
    (24, 12, 1, "db2", 2),           # rectangular
    (32, 32, 3, "haar", 5),          # down to 1 x 1 corners, several planes
    (64, 64, 1, "db2", 4),           # 4096 values: the whole transform in the tail
    (128, 64, 1, "db2", 3),          # 8192 values: one tiled level, then the tail
    (160, 96, 1, "db3", 3),          # several tiles, partial tiles in both axes, wrap across tile edges, then the tail
    (88, 160, 2, "db3", 1),          # a tiled level is the last one: its low-low band goes to res; partial tiles along x; two planes
    (72, 100, 1, "db2", 1),          # tiled, height 100: whole groups in a column, in fp32 none in a sub-band's 50 rows
    (80, 90, 1, "haar", 1),          # tiled, height 90: no groups in fp32; in fp64 in a column, not in a sub-band's 45 rows
    (256, 128, 1, "haar", 7),        # a deep pyramid: two tiled levels, five in the tail
    (64, 64, 1, "lat8", 3),          # custom taps
    (128, 128, 1, "lat16", 3),       # the longest taps, tiled (halo of 14) and in the tail
    (4, 1024, 1, "haar", 2),         # thin: 4096 values, in the tail
    (4, 2048, 1, "haar", 2),         # thin and tiled: two columns of lows per tile
    (1, 8192, 1, "db2", 2), (8192, 1, 1, "db2", 2),    # one-dimensional in the tiled kernels, then the tail
)


def case_id(case):
    return "%dx%dx%d-%s-%d" % case


def case_seed(case, salt=0):
    return 1000 * CASES.index(case) + salt


def _lattice(angles):
    """an orthonormal low-pass filter of length 2 len(angles): (H, G) <- rotation(theta) (H, z^-2 G), from H = (cos, sin), G = (-sin, cos)"""
    c, s = math.cos(angles[0]), math.sin(angles[0])
    h, g = np.array([c, s]), np.array([-s, c])
    for theta in angles[1:]:
        c, s = math.cos(theta), math.sin(theta)
        hp, gd = np.concatenate([h, [0.0, 0.0]]), np.concatenate([[0.0, 0.0], g])
        h, g = c * hp + s * gd, -s * hp + c * gd
    return h


@functools.lru_cache(maxsize=None)
def _taps(name):
    if name == "haar":
        d = math.sqrt(2.0)
        h = [1.0 / d, 1.0 / d]
    elif name == "db2":
        s, d = math.sqrt(3.0), 4.0 * math.sqrt(2.0)
        h = [(1.0 + s) / d, (3.0 + s) / d, (3.0 - s) / d, (1.0 - s) / d]
    elif name == "db3":
        a = math.sqrt(10.0)
        b, d = math.sqrt(5.0 + 2.0 * a), 16.0 * math.sqrt(2.0)
        h = [(1.0 + a + b) / d, (5.0 + a + 3.0 * b) / d, (10.0 - 2.0 * a + 2.0 * b) / d, (10.0 - 2.0 * a - 2.0 * b) / d, (5.0 + a - 3.0 * b) / d, (1.0 + a - b) / d]
    elif name == "lat8":
        h = _lattice([1.1, -0.6, 0.45, math.pi / 4 - 0.95])
    elif name == "lat16":
        h = _lattice([0.9, -0.4, 0.7, -1.2, 0.25, 0.6, -0.35, math.pi / 4 - 0.5])
    else:
        raise KeyError(name)
    h = np.array(h, np.float64)
    h.setflags(write=False)
    return h


def taps(wavelet):
    """(a): float64 taps of a name; an array passes through"""
    return _taps(wavelet) if isinstance(wavelet, str) else np.asarray(wavelet, np.float64)


def ortho_defect(h):
    T = len(h)
    return max(abs(float(np.dot(h[:T - 2 * l], h[2 * l:])) - (1.0 if l == 0 else 0.0)) for l in range(T // 2))


def high_pass(h):
    g = h[::-1].copy()
    g[1::2] = -g[1::2]
    return g


def _forward_pass(x, h, g):
    """one analysis pass along the last axis, in x's dtype"""
    m = x.shape[-1]
    k = np.arange(m // 2)
    lo, hi = np.zeros(x.shape[:-1] + (m // 2,), x.dtype), np.zeros(x.shape[:-1] + (m // 2,), x.dtype)
    for t in range(len(h)):
        v = x[..., (2 * k + t) % m]
        lo = lo + h[t] * v
        hi = hi + g[t] * v
    return np.concatenate([lo, hi], axis=-1)


def _inverse_pass(x, h, g):
    """one synthesis pass along the last axis, in x's dtype"""
    m = x.shape[-1]
    half = m // 2
    lo, hi = x[..., :half], x[..., half:]
    j = np.arange(half)
    out = np.zeros_like(x)
    for parity in (0, 1):
        acc = np.zeros(x.shape[:-1] + (half,), x.dtype)
        for t in range(parity, len(h), 2):
            k = (j - (t - parity) // 2) % half              # n = 2 j + parity: (n - t) / 2 = j - (t - parity) / 2
            acc = acc + h[t] * lo[..., k]
            acc = acc + g[t] * hi[..., k]
        out[..., parity::2] = acc
    return out


def product(v, nx, ny, L, wavelet, levels, transpose, dtype, res0=None):
    """(b): K v or K^T v in T in the pinned order"""
    dtype = np.dtype(dtype)
    h = taps(wavelet).astype(dtype)                         # rounded once to T
    g = high_pass(h)
    x = np.asarray(v).astype(dtype).reshape(L, nx, ny).copy()
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(levels):
            l = levels - 1 - i if transpose else i
            my, mx = (ny >> l if ny > 1 else 1), (nx >> l if nx > 1 else 1)
            c = x[:, :mx, :my]
            if not transpose:
                if my > 1:
                    c = _forward_pass(c, h, g)
                if mx > 1:
                    c = np.swapaxes(_forward_pass(np.swapaxes(c, 1, 2), h, g), 1, 2)
            else:
                if mx > 1:
                    c = np.swapaxes(_inverse_pass(np.swapaxes(c, 1, 2), h, g), 1, 2)
                if my > 1:
                    c = _inverse_pass(c, h, g)
            assert c.dtype == dtype
            x[:, :mx, :my] = c
        out = x.reshape(-1)
        out = out if res0 is None else np.asarray(res0).astype(dtype) + out
    assert out.dtype == dtype
    return out


def _one_level_matrix(m, h):
    g = high_pass(h)
    W = np.zeros((m, m))
    for k in range(m // 2):
        for t in range(len(h)):
            W[k, (2 * k + t) % m] += h[t]
            W[m // 2 + k, (2 * k + t) % m] += g[t]
    return W


@functools.lru_cache(maxsize=2)
def _matrix(nx, ny, wavelet, levels):
    h = taps(wavelet)
    N = nx * ny
    M = np.eye(N).reshape(nx, ny, N)
    for l in range(levels):
        my, mx = (ny >> l if ny > 1 else 1), (nx >> l if nx > 1 else 1)
        c = M[:mx, :my, :]
        if my > 1:
            c = np.einsum("ab,xbn->xan", _one_level_matrix(my, h), c, optimize=True)
        if mx > 1:
            c = np.einsum("ab,byn->ayn", _one_level_matrix(mx, h), c, optimize=True)
        M[:mx, :my, :] = c
    K = M.reshape(N, N)
    K.setflags(write=False)
    return K


def matrix(nx, ny, wavelet, levels):
    """(c): the N x N matrix of one plane in float64 (the operator is block diagonal over the planes)"""
    return _matrix(int(nx), int(ny), wavelet, int(levels))


def sums(nx, ny, L, wavelet, levels, alpha):
    """(d): (row sums, column sums) of |K|^alpha for all L N rows and columns"""
    K = np.abs(matrix(nx, ny, wavelet, levels))
    with np.errstate(divide="ignore"):
        P = np.where(K > 0, K ** alpha, 0.0)
    return np.tile(P.sum(axis=1), L), np.tile(np.ascontiguousarray(P.T).sum(axis=1), L)


def bound(wavelet, levels, dtype):
    """(e)"""
    h = taps(wavelet)
    u = float(np.finfo(dtype).eps) / 2
    n = len(h) + 1
    eta = n * u / (1 - n * u) * float(np.abs(h).sum())
    return (1 + eta) ** (2 * levels) - 1


def sums_tolerance(nx, ny, wavelet, levels, alpha):
    """[row, column]: what a row or column sum of |K|^alpha may differ by when every entry of K is known to d = B_64 only (an entry is one
    component of K e, |e| = 1, and the reference matrix and the header's tables both come from float64 passes within bound (e)):
    sum (|v| + d)^alpha - |v|^alpha over the non-zero entries, plus the rounding of the sum itself, (count + 8) eps of it"""
    d = bound(wavelet, levels, np.float64)
    A = np.abs(matrix(nx, ny, wavelet, levels))
    with np.errstate(divide="ignore"):
        grow = np.where(A > 0, (A + d) ** alpha - A ** alpha, 0.0)
        P = np.where(A > 0, A ** alpha, 0.0)
    eps = np.finfo(np.float64).eps
    return [grow.sum(axis=ax) + ((A > 0).sum(axis=ax) + 8) * eps * P.sum(axis=ax) for ax in (1, 0)]


def plane_norms(v, nx, ny, L):
    return np.sqrt((np.asarray(v, np.float64).reshape(L, nx * ny) ** 2).sum(axis=1))


def apply_matrix(v, nx, ny, L, wavelet, levels, transpose):
    """K v or K^T v in float64 through (c)"""
    K = matrix(nx, ny, wavelet, levels)
    x = np.asarray(v, np.float64).reshape(L, nx * ny)
    return (x @ (K if transpose else K.T)).reshape(-1)


def work_size(nx, ny, L, levels):
    """values of the work buffer: the corners after one and after two levels"""
    side = lambda s, j: s >> j if s > 1 else 1
    return L * (side(ny, 1) * side(nx, 1) + side(ny, 2) * side(nx, 2))


def abi_record(nx, ny, L, ntaps, levels, transpose, no_tail=False):
    """the geometry record of prost_hip_wavelet2d_geometry: int32 { ny, nx, planes, levels, ntaps, transpose, no_tail, reserved }"""
    return np.array([ny, nx, L, levels, ntaps, 1 if transpose else 0, 1 if no_tail else 0, 0], np.int32)
