"""References for prost.block.sense2d, written from the definition (the issue text and the comment at the head of
include/prost/linop/sense2d.hpp), never from the code under test.  NumPy only, around tests/fft2d_reference.py.

K u = [ F (sigma_c . u_l) ] over l < L images and c < C coils, F = fft2d.  N = nx ny, p = y + x ny.  Domain: re_l[p] at l N + p,
im_l[p] at (L + l) N + p.  Range: image j = l C + c, re_j[q] at j N + q, im_j[q] at (L C + j) N + q.  Maps: (2, C, N), real planes
first, rounded once to T; the operator is defined with the rounded maps.

  (a) product(..)         the restatement in T: forward z.re = u.re s.re - u.im s.im, z.im = u.re s.im + u.im s.re, every product and sum one
                          rounding, then fft2d_reference.product on the L C premultiplied images; transposed v = fft2d_reference.product
                          (transposed, scaling included) of the L C images, term (v.re s.re + v.im s.im, v.im s.re - v.re s.im), summed in
                          ascending c starting from the term of coil 0; res0: the accumulating form, res0 + value
  (b) matrix(..)          the explicit real matrix in float64: A = F diag(sigma_c) per coil, [[A.re, -A.im], [A.im, A.re]]
  (c) exact(..)           K v or K^T v in float64 by numpy.fft on the float64 products
  (d) bound_sums(..)      row (l, c, q): f(e) s^e sum_p |sigma_c(p)|^e; column of pixel p: f(e) s^e N sum_c |sigma_c(p)|^e;
                          f(e) = max(1, 2^(1 - e/2)), s = 1 / sqrt(N), an exactly zero |sigma| absent; sums by math.fsum
  (e) bounds(..)          Bf = B + sqrt(2) gamma_2 (1 + B) per coil image against |sigma_c . u_l|_2; Bt = Bf + gamma_{C-1} (1 + Bf) per image
                          against sum_c max|sigma_c| |y_{l,c}|_2; B = fft2d's bound, gamma_k = k u / (1 - k u)
"""
import math

import numpy as np

import fft2d_reference as F

# (nx, ny, L, C).  The kernels' dispatch is fft2d's (fft2d_reference.CASES): the y pass holds min(2048 / ny, nx) columns per workgroup
# (half as many, pitched, for ny < 64); the x pass a slab of B = min(tile / nx, ny) rows, tile = 2048 complex values for nx <= 128, else 8192
# (fp32) / 4096 (fp64).  The forward product forms sigma u in the load of the first pass (the y pass; the x pass when ny = 1) and its grid
# runs over the L C range images; the transposed product sums the coils in the registers of the last pass (the x pass; the y pass when
# nx = 1), 8 accumulators per lane with the small tile (nx <= 512 in this pass), 32 / 16 with the large one (nx >= 1024; the record's tile
# selector forces either: test_the_tile_of_the_coil_summing_pass_changes_no_bit).  16 bytes per lane when rhs, res / work AND the maps are
# 16-byte aligned and ny (y pass) or B (x pass) is at least 4 (fp32) / 2 (fp64).
CASES = (
    (1, 1, 1, 1), (1, 1, 2, 3),                  # no pass: the pointwise product
    (1, 2, 1, 2), (2, 1, 1, 2), (2, 2, 1, 3),    # narrow accesses (1 x 2 and 2 x 2 wide in fp64's y pass)
    (4, 8, 1, 2), (8, 4, 2, 3),                  # wide accesses
    (1, 64, 1, 2), (64, 1, 1, 2),                # one pass only: the y pass does the product AND the coil sum; the x pass with a slab of 1
    (64, 32, 1, 4), (32, 64, 2, 3),              # pitched and plain lines
    (256, 64, 1, 2), (64, 256, 1, 2),            # several tiles; nx = 256: the large x tile forward, the small one in the coil sum
    (2048, 2, 1, 2), (2, 2048, 1, 2),            # the longest lines; nx = 2048: the large tile in the coil sum (32 / 16 accumulators)
    (32, 32, 3, 5),                              # L > 1 and odd C
    (16, 16, 1, 64),                             # the longest coil loop
    (1, 2, 1100, 64),                            # L C = 70 400 images, more than the grid's 65 535
)


def case_id(case):
    return "%dx%dx%dx%d" % case


def case_seed(case, salt=0):
    case = tuple(case)
    return 7000 + 1000 * (CASES.index(case) if case in CASES else 100 + case[0] + 3 * case[1] + 5 * case[2] + 7 * case[3]) + salt


def sizes(case):
    """-> (rows, cols)"""
    nx, ny, L, C = case
    return 2 * L * C * nx * ny, 2 * L * nx * ny


def make_maps(case, seed=None, zeros=False):
    """complex128 (C, N): smooth magnitude times a random phase, plus noise; zeros: a block of exact zeros in map 0 (and all of the last
    map's first quarter)"""
    nx, ny, L, C = case
    N = nx * ny
    rng = np.random.default_rng(case_seed(case, 77) if seed is None else seed)
    m = (0.5 + rng.random((C, N))) * np.exp(2j * np.pi * rng.random((C, N)))
    if zeros:
        m[0, ::3] = 0.0
        m[C - 1, :max(1, N // 4)] = 0.0
    return m


def rounded(maps, dtype):
    """(2, C, N) in T: what the device stores"""
    maps = np.asarray(maps)
    return np.stack([maps.real, maps.imag]).astype(np.dtype(dtype))


def product(v, case, maps, transpose, dtype, res0=None):
    """(a): K v or K^T v in T in the pinned order; maps: complex (C, N)"""
    nx, ny, L, C = case
    N = nx * ny
    dtype = np.dtype(dtype)
    s = rounded(maps, dtype)
    sr, si = s[0], s[1]                                       # (C, N)
    with np.errstate(invalid="ignore", over="ignore"):
        if not transpose:
            u = np.asarray(v).astype(dtype).reshape(2, L, 1, N)
            zr = u[0] * sr - u[1] * si                        # (L, C, N): each product and the difference rounded once
            zi = u[0] * si + u[1] * sr
            assert zr.dtype == dtype
            out = F.product(np.stack([zr, zi]).reshape(-1), nx, ny, L * C, False, dtype)
        else:
            w = F.product(np.asarray(v).astype(dtype), nx, ny, L * C, True, dtype).reshape(2, L, C, N)
            tr = w[0] * sr + w[1] * si
            ti = w[1] * sr - w[0] * si
            accr, acci = tr[:, 0].copy(), ti[:, 0].copy()
            for c in range(1, C):
                accr = accr + tr[:, c]
                acci = acci + ti[:, c]
            out = np.stack([accr, acci]).reshape(-1)
        out = out if res0 is None else np.asarray(res0).astype(dtype) + out
    assert out.dtype == dtype
    return out


def maps64(maps, dtype):
    """the rounded maps as complex128 (C, N)"""
    s = rounded(maps, dtype).astype(np.float64)
    return s[0] + 1j * s[1]


def exact(v, case, maps, transpose, dtype):
    """(c): the float64 operator with the maps rounded to T"""
    nx, ny, L, C = case
    N = nx * ny
    s = maps64(maps, dtype)
    if not transpose:
        u = np.asarray(v, np.float64).reshape(2, L, 1, N)
        z = (u[0] + 1j * u[1]) * s                           # (L, C, N)
        y = np.fft.fft2(z.reshape(L, C, nx, ny), norm="ortho").reshape(L * C, N)
        return np.stack([y.real, y.imag]).reshape(-1)
    y = np.asarray(v, np.float64).reshape(2, L, C, nx, ny)
    w = np.fft.ifft2(y[0] + 1j * y[1], norm="ortho").reshape(L, C, N)
    u = (np.conj(s) * w).sum(axis=1)
    return np.stack([u.real, u.imag]).reshape(-1)


def matrix(case, maps, dtype):
    """(b): 2 L C N x 2 L N in float64"""
    nx, ny, L, C = case
    N = nx * ny
    Kf = F.matrix(nx, ny, 1)
    Cm, Sm = Kf[:N, :N], Kf[:N, N:]                           # F = Cm - i Sm
    s = maps64(maps, dtype)
    K = np.zeros((2 * L * C * N, 2 * L * N))
    for c in range(C):
        Ar = Cm * s[c].real + Sm * s[c].imag                 # A = F diag(sigma_c)
        Ai = Cm * s[c].imag - Sm * s[c].real
        for l in range(L):
            j = l * C + c
            K[j * N:(j + 1) * N, l * N:(l + 1) * N] = Ar
            K[j * N:(j + 1) * N, (L + l) * N:(L + l + 1) * N] = -Ai
            K[(L * C + j) * N:(L * C + j + 1) * N, l * N:(l + 1) * N] = Ai
            K[(L * C + j) * N:(L * C + j + 1) * N, (L + l) * N:(L + l + 1) * N] = Ar
    return K


def bound_sums(case, maps, dtype, e):
    """(d): -> (row bounds [2 L C N], column bounds [2 L N]) in float64"""
    nx, ny, L, C = case
    N = nx * ny
    s = rounded(maps, dtype).astype(np.float64)
    q = s[0] ** 2 + s[1] ** 2                                 # |sigma|^2, (C, N)
    with np.errstate(divide="ignore"):
        a = np.where(q > 0, q ** (0.5 * e), 0.0)
    f = max(1.0, 2.0 ** (1.0 - 0.5 * e)) * (1.0 / math.sqrt(float(N))) ** e
    rows = np.array([f * math.fsum(a[c]) for c in range(C)])
    cols = np.array([f * N * math.fsum(a[:, p]) for p in range(N)])
    return np.tile(np.repeat(rows, N), 2 * L), np.tile(cols, 2 * L)


def bounds(case, dtype):
    """(e): -> (Bf, Bt)"""
    nx, ny, L, C = case
    u = float(np.finfo(dtype).eps) / 2
    B = F.bound(nx, ny, dtype)
    gamma = lambda k: k * u / (1 - k * u)
    Bf = B + math.sqrt(2.0) * gamma(2) * (1 + B)
    return Bf, Bf + gamma(C - 1) * (1 + Bf)


def forward_scales(v, case, maps, dtype):
    """|sigma_c . u_l|_2 per coil image j = l C + c -> [L C]"""
    nx, ny, L, C = case
    N = nx * ny
    u = np.asarray(v, np.float64).reshape(2, L, 1, N)
    z = (u[0] + 1j * u[1]) * maps64(maps, dtype)
    return np.sqrt((np.abs(z) ** 2).sum(axis=2)).reshape(-1)


def transposed_scales(v, case, maps, dtype):
    """sum_c max_p |sigma_c(p)| |y_{l,c}|_2 per image l -> [L]"""
    nx, ny, L, C = case
    N = nx * ny
    y = np.asarray(v, np.float64).reshape(2, L, C, N)
    norms = np.sqrt((y ** 2).sum(axis=(0, 3)))               # (L, C)
    return (norms * np.abs(maps64(maps, dtype)).max(axis=1)).sum(axis=1)


def image_norms(v, images, N):
    """the 2-norm of every complex image of a vector of 2 `images` N values -> [images]"""
    x = np.asarray(v, np.float64).reshape(2, images, N)
    return np.sqrt((x ** 2).sum(axis=(0, 2)))


def abi_record(case, transpose, slab=0):
    """the geometry record of prost_hip_sense2d_geometry: int32 { ny, nx, planes, coils, transpose, slab }; slab: the tile of the
    coil-summing pass, 0 the library's choice, 1 the small tile, 2 fft2d's choice: no bit depends on it"""
    nx, ny, L, C = case
    return np.array([ny, nx, L, C, 1 if transpose else 0, slab], np.int32)
