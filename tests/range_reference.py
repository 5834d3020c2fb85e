"""Reference values for ind_range (the projection x = A (A'A)^-1 A' y onto the range of a sparse matrix): NumPy / SciPy in fp64, never
the code under test.  The CPU oracle cannot express this prox, so the two families below are all the tests compare with.

Exact family (no tolerance).  h = n // 2; N has min(3 n, h (n - h)) entries +-1 at random positions in rows >= h and columns < h, so
N N = 0; L = I + N and L^-1 = I - N.  The rows of L' sit at n sorted random rows of the m x n matrix A, whose other rows are empty, and
AA = A'A = L L' is formed in fp64.  The argument holds integers in [-8, 8].  Every intermediate value is a small integer, so the Cholesky
factor of AA is L itself and the projection is the argument on the occupied rows and 0 elsewhere -- bit for bit in fp32 and fp64, whatever
the blocking or the summation order.

Tolerance family.  A is a row permutation of [I_n ; S], S an (m - n) x n sparse standard normal matrix, so cond(A'A) stays small (113 at
(500, 250, 0.1), the shape of the reference's test_prox_ind_range.m; 84 at (200, 96, 0.2)).  The argument is standard normal.  Truth:
A @ solve(AA, A' y) in fp64.  Yardstick e_T: the relative inf-norm error of the same pipeline run by LAPACK in precision T
(scipy.linalg.cho_factor / cho_solve on AA.astype(T), the two products in T).  Bound: max(4 e_T, 32 eps_T) -- the factor 4 for another
blocking, another summation order and the inverted diagonal blocks on a matrix this well conditioned, the floor for the cases where LAPACK
lands within a few ulps of the truth.
"""
import functools

import numpy as np
import scipy.linalg
import scipy.sparse as sp


def exact_family(n, m, seed=0):
    """-> (A csc m x n, AA n x n, y m, want m)"""
    rng = np.random.default_rng(1000 * n + m + seed)
    h = n // 2
    L = np.eye(n)
    count = min(3 * n, h * (n - h))
    if count:
        flat = rng.choice(h * (n - h), size=count, replace=False)
        L[h + flat // h, flat % h] = rng.choice([-1.0, 1.0], size=count)
    rows = np.sort(rng.choice(m, size=n, replace=False))
    r, c = np.nonzero(L.T)
    A = sp.csc_matrix(sp.coo_matrix((L.T[r, c], (rows[r], c)), shape=(m, n)))
    AA = L @ L.T
    assert np.array_equal((A.T @ A).toarray(), AA)
    y = rng.integers(-8, 9, size=m).astype(np.float64)
    want = np.zeros(m)
    want[rows] = y[rows]
    return A, AA, y, want


def tolerance_family(n, m, density, seed=0):
    """-> (A csc m x n, AA n x n, y m)"""
    rng = np.random.default_rng(7000 * n + m + seed)
    blocks = [sp.identity(n, format="csr")]
    if m > n:
        blocks.append(sp.random(m - n, n, density=density, random_state=rng, data_rvs=rng.standard_normal, format="csr"))
    A = sp.vstack(blocks).tocsr()[rng.permutation(m)]
    A = sp.csc_matrix(A)
    AA = (A.T @ A).toarray()
    return A, AA, rng.standard_normal(m)


def truth(A, AA, y):
    return A @ np.linalg.solve(AA, A.T @ y)


def rel_inf(got, want):
    scale = float(np.abs(want).max())
    return float(np.abs(np.asarray(got, dtype=np.float64) - want).max()) / (scale if scale > 0 else 1.0)


def lapack_yardstick(A, AA, y, dtype):
    """e_T: relative inf-norm error of the LAPACK pipeline in precision `dtype` against the fp64 truth"""
    At = sp.csc_matrix(A, dtype=dtype)
    t = At.T @ y.astype(dtype)
    z = scipy.linalg.cho_solve(scipy.linalg.cho_factor(AA.astype(dtype), lower=True), t)
    x = At @ z.astype(dtype)
    assert x.dtype == dtype
    return rel_inf(x, truth(A, AA, y))


def bound(e_t, dtype):
    return max(4.0 * e_t, 32.0 * float(np.finfo(dtype).eps))


@functools.lru_cache(maxsize=None)
def tolerance_case(n, m, density, dtype_name):
    """inputs (rounded to the data type: the matrix every run sees), truth and bound, computed once and shared"""
    dtype = np.dtype(dtype_name).type
    A, AA, y = tolerance_family(n, m, density)
    A = sp.csc_matrix(A.astype(dtype).astype(np.float64))
    AA = AA.astype(dtype).astype(np.float64)
    y = y.astype(dtype).astype(np.float64)
    want = truth(A, AA, y)
    e_t = lapack_yardstick(A, AA, y, dtype)
    for a in (AA, y, want):
        a.setflags(write=False)
    return A, AA, y, want, e_t, bound(e_t, dtype)
