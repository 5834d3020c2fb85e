"""References for prost.block.fft2d, written from the definition (the issue text and the comment at the head of
include/prost/linop/fft2d.hpp), never from the code under test.  NumPy only, vectorised stage by stage.

Layout: L complex images of ny x nx as 2 L real planes, re_c[p] at c N + p, im_c[p] at (L + c) N + p, N = nx ny, p = y + x ny; the
range likewise over q = ky + kx ny, DC at 0.  K = s [[C, S], [-S, C]], C = cos(theta), S = sin(theta), theta = 2 pi (ky y / ny +
kx x / nx), s = 1 / sqrt(N); K^T is the unitary inverse transform.

  (a) table(n, dtype)     n entries (cos, -sin)(2 pi j / n): cos and sin (math.cos, math.sin: the C library's, on 2.0 * pi * j / n in
                          that order) in the first octant only, the rest by symmetry, so that w[0] = (1, 0), w[n/4] = (0, -1) and
                          w[n/8] = (sqrt(1/2), -sqrt(1/2)) exactly; rounded once to T
  (b) product(..)         the restatement in T in the pinned order: the radix-2 decimation-in-time tree, breadth first; stage
                          h = 1, 2, .., m / 2 takes butterfly j = k + h r, a = Y[j], b = Y[j + m/2], t = w b with w = table[k n / 2 h]
                          (k = 0: t = b; k = h / 2: t = (b.im, -b.re), transposed (-b.im, b.re); else (br wr - bi wi, br wi + bi wr)
                          with wi negated for the transpose), Y'[k + 2 h r] = a + t, Y'[k + h + 2 h r] = a - t; the y pass, then the
                          x pass, then one multiplication by s rounded to T; res0: the accumulating form, res0 + value
  (c) matrix(..)          the explicit real matrix in float64 from np.cos / np.sin, with exact zeros at the quarter turns
  (d) sums(..)            the closed form: row (ky, kx) has the angles uniform over the multiples of 2 pi / g,
                          g = max(ny / gcd(ky, ny), nx / gcd(kx, nx)), gcd(0, n) = n:
                          s^alpha (N / g) sum_{j < g} (|cos(2 pi j / g)|^alpha + |sin(2 pi j / g)|^alpha), exact zeros absent;
                          the column of pixel (y, x) likewise
  (e) bound(..)           B = t eta / (1 - t eta) + 2 u, t = log2 nx + log2 ny, eta = mu + gamma_4 (sqrt(2) + mu), mu = u,
                          gamma_4 = 4 u / (1 - 4 u): |fl(K x) - K x|_2 <= B |x|_2 per plane pair (Higham, Thm 24.2)
"""
import functools
import math

import numpy as np

# (nx, ny, L).  The kernels' dispatch: the y pass holds min(2048 / ny, nx) columns per workgroup (half as many, pitched at 3 ny / 2, for
# ny < 64); the x pass holds a slab of B = min(tile / nx, ny) rows, tile = 2048 complex values for nx <= 128, else 8192 (fp32) / 4096 (fp64).
# A pass moves 16 bytes per lane when its pointers are 16-byte aligned and ny (y pass) or B (x pass) is at least 4 (fp32) / 2 (fp64):
# off at 1 x 2, 2 x 1, 2 x 2 and 2048 x 2 in fp32 and at every odd element offset (the tests' 1 x 1 diags block in front, the C entry
# points at offset 1), on at 2048 x 2 in fp64, at 4 x 8, 8 x 4 and every larger shape.
CASES = (
    (1, 1, 1), (1, 2, 1), (2, 1, 1), (2, 2, 1), (4, 8, 1), (8, 4, 1), (1, 64, 1), (64, 1, 1),
    (64, 32, 1), (32, 64, 1),            # ny = 32: pitched lines; ny = 64: plain lines; one tile each
    (256, 64, 1), (64, 256, 1),          # several tiles in the y pass; nx = 256: the large tile (two slabs in fp32), nx = 64: the small one
    (256, 32, 1),                        # several tiles of pitched lines
    (2048, 2, 1), (2, 2048, 1),          # the longest lines: a slab of 2; one column per workgroup
    (2048, 8, 1), (8, 2048, 1),          # the longest lines, several tiles: slab of 4 (fp32) and 2 (fp64)
    (32, 32, 3),
)


def case_id(case):
    return "%dx%dx%d" % case


def case_seed(case, salt=0):
    return 1000 * CASES.index(case) + salt


def _angle(j, n):
    """(cos, sin)(2 pi j / n) in float64; cos and sin are called in the first octant only"""
    if n >= 2 and j >= n // 2:
        c, s = _angle(j - n // 2, n)
        return -c, -s
    if n >= 4 and j >= n // 4:
        c, s = _angle(j - n // 4, n)
        return -s, c
    if j == 0:
        return 1.0, 0.0
    if 8 * j == n:
        return math.sqrt(0.5), math.sqrt(0.5)
    if 8 * j > n:
        c, s = _angle(n // 4 - j, n)
        return s, c
    a = 2.0 * math.pi * float(j) / float(n)
    return math.cos(a), math.sin(a)


@functools.lru_cache(maxsize=None)
def _table(n, name):
    w = np.array([(c, -s) for c, s in (_angle(j, n) for j in range(n))], np.float64).astype(np.dtype(name))
    w.setflags(write=False)
    return w


def table(n, dtype):
    """(a): shape (n, 2), the layout of the device table"""
    return _table(int(n), np.dtype(dtype).name)


def scale(nx, ny, dtype):
    return np.dtype(dtype).type(1.0 / math.sqrt(float(ny) * float(nx)))


def _lines(re, im, w, transpose):
    """the tree along the last axis of re, im (any leading shape), in their dtype"""
    m = re.shape[-1]
    lead = re.shape[:-1]
    n = w.shape[0]
    h = 1
    with np.errstate(invalid="ignore", over="ignore"):
        while h < m:
            r = m // 2 // h
            ar, ai = re[..., :m // 2].reshape(lead + (r, h)), im[..., :m // 2].reshape(lead + (r, h))
            br, bi = re[..., m // 2:].reshape(lead + (r, h)), im[..., m // 2:].reshape(lead + (r, h))
            k = np.arange(h)
            wr, wi = w[k * (n // (2 * h)), 0], w[k * (n // (2 * h)), 1]
            if transpose:
                wi = -wi
            tr = br * wr - bi * wi
            ti = br * wi + bi * wr
            tr[..., 0], ti[..., 0] = br[..., 0], bi[..., 0]
            if h > 1:
                q = h // 2
                if transpose:
                    tr[..., q], ti[..., q] = -bi[..., q], br[..., q]
                else:
                    tr[..., q], ti[..., q] = bi[..., q], -br[..., q]
            re = np.stack([ar + tr, ar - tr], axis=-2).reshape(lead + (m,))
            im = np.stack([ai + ti, ai - ti], axis=-2).reshape(lead + (m,))
            h *= 2
    return re, im


def product(v, nx, ny, L, transpose, dtype, res0=None):
    """(b): K v or K^T v in T in the pinned order"""
    dtype = np.dtype(dtype)
    w = table(max(nx, ny), dtype)
    x = np.asarray(v).astype(dtype).reshape(2, L, nx, ny)
    re, im = x[0], x[1]
    if ny > 1:
        re, im = _lines(re, im, w, transpose)
    if nx > 1:
        re, im = _lines(np.swapaxes(re, 1, 2), np.swapaxes(im, 1, 2), w, transpose)
        re, im = np.swapaxes(re, 1, 2), np.swapaxes(im, 1, 2)
    assert re.dtype == dtype and im.dtype == dtype
    with np.errstate(invalid="ignore", over="ignore"):
        out = (np.stack([re, im]) * scale(nx, ny, dtype)).reshape(-1)
        out = out if res0 is None else np.asarray(res0).astype(dtype) + out
    assert out.dtype == dtype
    return out


@functools.lru_cache(maxsize=16)
def _matrix(nx, ny):
    ky = np.arange(ny)
    kx = np.arange(nx)
    # theta[q, p] with q = ky + kx ny, p = y + x ny; the integer products are reduced before the division so that the angles are accurate
    ty = (np.outer(ky, ky) % ny) / float(ny)
    tx = (np.outer(kx, kx) % nx) / float(nx)
    frac = (tx[:, None, :, None] + ty[None, :, None, :]).reshape(nx * ny, nx * ny) % 1.0        # exact: multiples of 1 / max(nx, ny)
    theta = 2.0 * np.pi * frac
    s = 1.0 / math.sqrt(float(nx * ny))
    # at the quarter turns the entries are exactly 0 (np.cos(pi / 2) is 6e-17, which |.|^alpha with alpha < 1 would blow up)
    Cm = s * np.where((frac == 0.25) | (frac == 0.75), 0.0, np.cos(theta))
    Sm = s * np.where((frac == 0.0) | (frac == 0.5), 0.0, np.sin(theta))
    one = np.block([[Cm, Sm], [-Sm, Cm]])
    one.setflags(write=False)
    return one


def matrix(nx, ny, L=1):
    """(c): 2 L N x 2 L N in float64"""
    one = _matrix(int(nx), int(ny))
    if L == 1:
        return one
    N = nx * ny
    K = np.zeros((2 * L * N, 2 * L * N))
    for c in range(L):
        for i in range(2):
            for j in range(2):
                K[(i * L + c) * N:(i * L + c + 1) * N, (j * L + c) * N:(j * L + c + 1) * N] = one[i * N:(i + 1) * N, j * N:(j + 1) * N]
    return K


def periods(nx, ny):
    """g of every frequency q = ky + kx ny (and of every pixel p = y + x ny)"""
    gy = np.array([ny // math.gcd(k, ny) for k in range(ny)])
    gx = np.array([nx // math.gcd(k, nx) for k in range(nx)])
    return np.maximum(gx[:, None], gy[None, :]).reshape(-1)


def sums(nx, ny, L, alpha):
    """(d): the sums of |K|^alpha over every row (equally: over every column) in float64, by the closed form"""
    N = nx * ny
    g = periods(nx, ny)
    s = 1.0 / math.sqrt(float(N))
    out = np.zeros(N)
    for gg in np.unique(g):
        acc = 0.0
        for j in range(int(gg)):
            c, sn = _angle(j, int(gg))
            acc += (abs(c) ** alpha if c != 0 else 0.0) + (abs(sn) ** alpha if sn != 0 else 0.0)
        out[g == gg] = s ** alpha * (N / float(gg)) * acc
    return np.tile(out, 2 * L), np.tile(g, 2 * L)


def bound(nx, ny, dtype):
    """(e)"""
    u = float(np.finfo(dtype).eps) / 2
    t = math.log2(nx) + math.log2(ny)
    gamma4 = 4 * u / (1 - 4 * u)
    eta = u + gamma4 * (math.sqrt(2.0) + u)
    return t * eta / (1 - t * eta) + 2 * u


def pair_norms(v, nx, ny, L):
    """the 2-norm of every plane pair (re_c, im_c) -> [L]"""
    x = np.asarray(v, np.float64).reshape(2, L, nx * ny)
    return np.sqrt((x ** 2).sum(axis=(0, 2)))


def fft_reference(v, nx, ny, L, transpose):
    """K v or K^T v by numpy.fft in float64 (norm="ortho")"""
    x = np.asarray(v, np.float64).reshape(2, L, nx, ny)
    z = x[0] + 1j * x[1]
    z = np.fft.ifft2(z, norm="ortho") if transpose else np.fft.fft2(z, norm="ortho")
    return np.stack([z.real, z.imag]).reshape(-1)


def abi_record(nx, ny, L, transpose):
    """the geometry record of prost_hip_fft2d_geometry: int32 { ny, nx, planes, transpose }"""
    return np.array([ny, nx, L, 1 if transpose else 0], np.int32)
