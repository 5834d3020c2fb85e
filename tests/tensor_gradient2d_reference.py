"""References for prost.block.tensor_gradient2d (no code of the block is used here):

  (a) matrix(nx, ny, L, planes, dtype): the explicit scipy matrix K = T G, 2 L N x L N.  G holds the forward differences of gradient2d
      (an entry only where its mask holds), T = [[diag(a), diag(b)], [diag(b), diag(c)]] per channel with the planes rounded to dtype
      once; the sparse product multiplies stored entries only, so a tensor value whose entries are all masked away never enters, and the
      two terms that meet in column p of one row are one merged entry -(ax a + ay b), formed in float64;
  (b) product: the marches of include/prost/linop/tensor_gradient2d.hpp restated on NumPy arrays of a given dtype (every NumPy
      operation on arrays of one dtype rounds once in that dtype, and there is no contraction), with explicit masks -- np.where selects,
      nothing is multiplied by a mask -- and the stated order: difference, product, the addition of two present terms; the adjoint forms
      the fluxes, then divx, divy, s = divx + divy and 0 - s as grad_adj_kernel does; the accumulating form is res0 + value;
  (c) sums: the row / column sums of |entries of (a)|^alpha in fp64;
  bound: gamma_n B componentwise with B = |T| (|G| |x|) forward and |G|^T (|T| |y|) for the adjoint -- the UNMERGED absolute values --
      gamma_n = n u / (1 - n u), n the roundings of the block by mode (forward 2, 2, 3; adjoint 3, 3, 4), plus those of a CSR twin with
      entries rounded to dtype (forward 3, 3, 4; adjoint 4, 4, 7) when the comparison is against such a twin.  The derivation is in the
      header.

Grid: N = nx ny, pixel (y, x) at p = y + x ny.  Domain: u_c[p] at c N + p.  Range: gx_c[p] at c N + p, gy_c[p] at (L + c) N + p.
A tensor here is a list of k planes of N values (k = 1: g; 2: a, c; 3: a, b, c).
"""
import numpy as np
import scipy.sparse as sp

ROUNDINGS = {False: (2, 2, 3), True: (3, 3, 4)}            # the block, by transpose and mode - 1
TWIN_ROUNDINGS = {False: (3, 3, 4), True: (4, 4, 7)}       # a CSR twin in dtype
T_TERMS = 6                                                 # the longest sum of |entry|^alpha (a column at k = 3): (t + 8) eps_T


def masks(nx, ny):
    """ax, bx, ay, by as [x, y] boolean arrays"""
    x, y = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    return x < nx - 1, x > 0, y < ny - 1, y > 0


def rounded(planes, dtype):
    """the planes rounded to dtype once, as float64 vectors"""
    return [np.asarray(p, dtype=np.float64).reshape(-1).astype(dtype).astype(np.float64) for p in planes]


def abc(planes):
    """(a, b, c) of a tensor; b is None where the mode has none"""
    k = len(planes)
    assert k in (1, 2, 3)
    return (planes[0], None, planes[0]) if k == 1 else ((planes[0], None, planes[1]) if k == 2 else tuple(planes))


def gradient(nx, ny):
    """G of one channel, 2 N x N: rows dx[p] then dy[p]; an entry only where the mask holds"""
    N = nx * ny
    ax, _, ay, _ = masks(nx, ny)
    p = np.arange(N)
    px, py = p[ax.reshape(-1)], p[ay.reshape(-1)]
    rows = np.concatenate([px, px, N + py, N + py])
    cols = np.concatenate([px, px + ny, py, py + 1])
    vals = np.concatenate([-np.ones(px.size), np.ones(px.size), -np.ones(py.size), np.ones(py.size)])
    return sp.csr_matrix((vals, (rows, cols)), shape=(2 * N, N))


def tensor_matrix(planes, N, absolute=False):
    """T of one channel, 2 N x 2 N"""
    a, b, c = abc(planes)
    f = np.abs if absolute else (lambda v: v)
    B = sp.diags(f(b)) if b is not None else sp.csr_matrix((N, N))
    return sp.bmat([[sp.diags(f(a)), B], [B, sp.diags(f(c))]], format="csr")


def _channels(M, L, nrow_planes):
    """kron over channels in the planar layout: plane-major, channel inside"""
    N = M.shape[1]
    blocks = [sp.kron(sp.identity(L), M[i * N:(i + 1) * N]) for i in range(nrow_planes)]
    return sp.vstack(blocks, format="csr")


def matrix(nx, ny, L, planes, dtype=np.float64):
    """(a): csc, float64 entries from the planes rounded to dtype; a zero is no entry"""
    N = nx * ny
    with np.errstate(invalid="ignore", over="ignore"):
        K1 = (tensor_matrix(rounded(planes, dtype), N) @ gradient(nx, ny)).tocsr()
    K = _channels(K1, L, 2).tocsc()
    K.eliminate_zeros()
    K.sort_indices()
    assert K.shape == (2 * L * N, L * N)
    return K


def _shift(a, dx, dy):
    """a[c, x + dx, y + dy]; cells outside the grid hold a NaN that a mask must select away"""
    out = np.full_like(a, np.nan)
    nx, ny = a.shape[1:]
    xs, xd = (slice(dx, nx), slice(0, nx - dx)) if dx >= 0 else (slice(0, nx + dx), slice(-dx, nx))
    ys, yd = (slice(dy, ny), slice(0, ny - dy)) if dy >= 0 else (slice(0, ny + dy), slice(-dy, ny))
    out[:, xd, yd] = a[:, xs, ys]
    return out


def _combine(m0, t0, m1, t1):
    """(m0) t0 + (m1) t1: absent terms are not added"""
    return np.where(m0 & m1, t0 + t1, np.where(m0, t0, np.where(m1, t1, np.zeros_like(t0))))


def product(x, nx, ny, L, planes, transpose, dtype, res0=None):
    """(b): K x (transpose: K^T x) in dtype, or res0 + that"""
    dtype = np.dtype(dtype).type
    ax, bx, ay, by = masks(nx, ny)
    a, b, c = [None if p is None else np.asarray(p, dtype=np.float64).reshape(-1).astype(dtype).reshape(1, nx, ny) for p in abc(planes)]
    v = np.asarray(x).astype(dtype)
    zero = np.zeros((L, nx, ny), dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        if not transpose:
            u = v.reshape(L, nx, ny)
            dx, dy = _shift(u, 1, 0) - u, _shift(u, 0, 1) - u
            if b is None:
                gx, gy = np.where(ax, a * dx, zero), np.where(ay, c * dy, zero)
            else:
                gx, gy = _combine(ax, a * dx, ay, b * dy), _combine(ax, b * dx, ay, c * dy)
            out = np.stack([gx, gy])
        else:
            gx, gy = v.reshape(2, L, nx, ny)
            if b is None:
                qx, qy = a * gx, c * gy
            else:
                qx, qy = a * gx + b * gy, b * gx + c * gy
            divx = np.where(ax, qx, zero)
            divx = np.where(bx, divx - _shift(qx, -1, 0), divx)
            divy = np.where(ay, qy, zero)
            divy = np.where(by, divy - _shift(qy, 0, -1), divy)
            out = zero - (divx + divy)
    assert out.dtype == np.dtype(dtype)
    out = out.reshape(-1)
    return out if res0 is None else np.asarray(res0).astype(dtype) + out


def gradient_product(x, nx, ny, L, transpose, dtype):
    """gradient2d(nx, ny, L) restated (grad_fwd_kernel / grad_adj_kernel): no tensor anywhere"""
    dtype = np.dtype(dtype).type
    ax, bx, ay, by = masks(nx, ny)
    v = np.asarray(x).astype(dtype)
    zero = np.zeros((L, nx, ny), dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        if not transpose:
            u = v.reshape(L, nx, ny)
            return np.stack([np.where(ax, _shift(u, 1, 0) - u, zero), np.where(ay, _shift(u, 0, 1) - u, zero)]).reshape(-1)
        gx, gy = v.reshape(2, L, nx, ny)
        divx = np.where(ax, gx, zero)
        divx = np.where(bx, divx - _shift(gx, -1, 0), divx)
        divy = np.where(ay, gy, zero)
        divy = np.where(by, divy - _shift(gy, 0, -1), divy)
        return (zero - (divx + divy)).reshape(-1)


def sums(nx, ny, L, planes, alpha=1.0, dtype=np.float64):
    """(c): sum |entry|^alpha of every row and every column of (a), in fp64 -> (rows, cols)"""
    K = abs(matrix(nx, ny, L, planes, dtype))
    K.data = K.data ** float(alpha)
    return np.asarray(K.sum(axis=1)).ravel(), np.asarray(K.sum(axis=0)).ravel()


def magnitude(nx, ny, L, planes, transpose, x, dtype):
    """B: |T| (|G| |x|), or |G|^T (|T| |x|) for the transpose, with the planes rounded to dtype"""
    N = nx * ny
    absG = _channels(abs(gradient(nx, ny)), L, 2)
    absT1 = tensor_matrix(rounded(planes, dtype), N, absolute=True)
    I = sp.identity(L)
    absT = sp.bmat([[sp.kron(I, absT1[:N, :N]), sp.kron(I, absT1[:N, N:])], [sp.kron(I, absT1[N:, :N]), sp.kron(I, absT1[N:, N:])]], format="csr")
    ab = np.abs(np.asarray(x, dtype=np.float64))
    return absG.T @ (absT @ ab) if transpose else absT @ (absG @ ab)


def gamma(n, dtype):
    u = np.finfo(dtype).eps / 2
    return n * u / (1 - n * u)


def bound(nx, ny, L, planes, transpose, x, dtype, twin=False):
    """gamma_n B for the block against the exact product; twin: against a CSR twin in dtype, gamma_block B + gamma_twin B"""
    k = len(planes)
    g = gamma(ROUNDINGS[bool(transpose)][k - 1], dtype)
    if twin:
        g = g + gamma(TWIN_ROUNDINGS[bool(transpose)][k - 1], dtype)
    return g * magnitude(nx, ny, L, planes, transpose, x, dtype)


# ---- tensors ----
MODES = (1, 2, 3)


def dyadic_tensor(nx, ny, k, seed):
    """multiples of 1/8 in [-1, 1], b of either sign, zeros included: every sum of |entries| is exact in both precisions"""
    rng = np.random.default_rng(seed)
    return [rng.integers(-8, 9, nx * ny).astype(np.float64) / 8 for _ in range(k)]


def random_tensor(nx, ny, k, seed):
    """k = 1, 2: weights in (0.05, 1.05); k = 3: a, c > 0 and |b|^2 < a c (positive definite), b of either sign"""
    rng = np.random.default_rng(seed)
    N = nx * ny
    if k < 3:
        return [0.05 + rng.random(N) for _ in range(k)]
    a, c = 0.05 + rng.random(N), 0.05 + rng.random(N)
    b = (2 * rng.random(N) - 1) * 0.95 * np.sqrt(a * c)
    return [a, b, c]


def ones_tensor(nx, ny):
    return [np.ones(nx * ny)]


# the constants of include/prost/linop/tensor_gradient2d.hpp and of the kernels' dispatch (prost_amd/csrc/kernels_linop_tensor_gradient2d.hip)
BLOCK = 256                                     # lanes of a workgroup
WAVE = 64
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
SMALL = [(1, 1, 1), (1, 7, 1), (5, 1, 1), (3, 3, 1), (3, 3, 3), (17, 13, 3)]
# the wave edge inside a strip: 64 VEC rows and one vector more, per precision (fp64: 128, 130; fp32: 256, 260)
WAVES = [(128, 3, 1), (130, 3, 1), (256, 3, 1), (260, 2, 3)]
# one strip of the vector path, one row more (the element kernels) and one vector more (a second strip), per precision
STRIPS = [(512, 3, 1), (513, 3, 1), (514, 3, 1), (1024, 3, 1), (1025, 3, 1), (1028, 2, 3)]
# a chunk of 12, 6 or 3 columns is only picked when 2048 workgroups remain: nx = 2048 c at one strip and one channel is the smallest
# grid of full chunks of c columns, nx = 2048 c + 1 adds a last chunk of a single column; 4 rows: one vector in fp32, two in fp64
CHUNKS = [(4, 2048 * 3, 1), (4, 2048 * 3 + 1, 1), (4, 2048 * 6, 1), (4, 2048 * 6 + 1, 1), (4, 2048 * 12, 1), (4, 2048 * 12 + 1, 1), (8, 4097, 3)]
CASES = SMALL + WAVES + STRIPS + CHUNKS


def is_dyadic(case):
    """the cases whose product tests use a dyadic tensor (every sum of |entries| exact): the small ones with nx + ny even"""
    ny, nx, _ = case
    return nx * ny <= 4096 and (nx + ny) % 2 == 0


def tensor_for(case, k):
    """the tensor of a case in the product tests: dyadic where is_dyadic, random positive definite elsewhere"""
    ny, nx, _ = case
    return dyadic_tensor(nx, ny, k, case_seed(case, k)) if is_dyadic(case) else random_tensor(nx, ny, k, case_seed(case, k))


def case_id(case):
    return "%dx%dx%d" % case


def case_seed(case, salt=0):
    ny, nx, L = case
    return 17 + salt + 13 * ny + 1009 * nx + 100003 * L
