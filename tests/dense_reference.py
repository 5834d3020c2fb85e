"""NumPy restatements of the three dense blocks, in the dtype under test (helper of test_dense_frontend.py and
test_gpu_dense_blocks.py; not a test).

The two Kronecker products are formed the way BlockDenseKronIdKernel / BlockIdKronDenseKernel form them
(src/linop/block_dense_kron_id.cu:28-65, block_id_kron_dense.cu:28-65): per output a sum of the dtype that starts at 0, one product
(rounded to the dtype) added per inner index in ascending order, then one add into the result.  NumPy rounds every elementwise
operation on arrays of one dtype to that dtype, so a loop over the inner index with whole-vector operations IS that order."""
import numpy as np


def _apply(K, x, d, id_first, dtype):
    """kron(K, I_d) x (id_first False) or kron(I_d, K) x (True) as an (out rows of K) x d array of sums; K already holds the dtype"""
    m, n = K.shape
    X = x.reshape(d, n).T if id_first else x.reshape(n, d)          # X[i, p]: the operand of inner index i in group p
    S = np.zeros((m, d), dtype=dtype)
    for i in range(n):
        S += K[:, i:i + 1] * X[i:i + 1, :]                          # the product is rounded before the add
    return S.T.ravel() if id_first else S.ravel()


def kron_product(K, x, d, id_first, transpose, dtype, res0=None):
    """res0 + (kron(K, I_d) | kron(I_d, K)) (x | transposed: the adjoint); everything in `dtype`"""
    K = np.asarray(K, dtype=np.float64).astype(dtype)
    x = np.asarray(x, dtype=np.float64).astype(dtype)
    s = _apply(K.T.copy() if transpose else K, x, d, id_first, dtype)
    res = np.zeros_like(s) if res0 is None else np.asarray(res0, dtype=dtype)
    return res + s


def kron_sums(K, d, id_first, alpha, dtype):
    """(row sums, column sums) of one Kronecker block: sum of pow(|K[.]|, alpha) in `dtype`, ascending index
    (block_dense_kron_id.cu:100-121: K's row is row / d, block_id_kron_dense.cu:100-121: row % m)"""
    K = np.asarray(K, dtype=np.float64).astype(dtype)
    P = np.power(np.abs(K), dtype(alpha)).astype(dtype)
    rows = np.zeros(K.shape[0], dtype=dtype)
    for i in range(K.shape[1]):
        rows += P[:, i]
    cols = np.zeros(K.shape[1], dtype=dtype)
    for i in range(K.shape[0]):
        cols += P[i, :]
    if id_first:
        return np.tile(rows, d), np.tile(cols, d)
    return np.repeat(rows, d), np.repeat(cols, d)


def arrangement_2x2(K, x, d, id_first, transpose, dtype):
    """the reference tests' arrangement [[B, B], [B, B]] of four copies of one block B (m d x n d), evaluated in the list order
    (0, 0), (m d, 0), (m d, n d), (0, n d) as LinearOperator::Eval does: the first writer of a range stores 0 + sum, the
    second adds its sum."""
    m, n = np.shape(K)
    rows, cols = (n, m) if transpose else (m, n)
    x = np.asarray(x, dtype=np.float64)
    x0, x1 = x[:cols * d], x[cols * d:]
    out = []
    if not transpose:          # rows [0, m d): blocks (0, 0) then (0, n d); rows [m d, 2 m d): (m d, 0) then (m d, n d)
        for first, second in ((x0, x1), (x0, x1)):
            out.append(kron_product(K, second, d, id_first, False, dtype, kron_product(K, first, d, id_first, False, dtype)))
    else:                      # columns [0, n d): (0, 0) then (m d, 0); columns [n d, 2 n d): (m d, n d) then (0, n d)
        out.append(kron_product(K, x1, d, id_first, True, dtype, kron_product(K, x0, d, id_first, True, dtype)))
        out.append(kron_product(K, x0, d, id_first, True, dtype, kron_product(K, x1, d, id_first, True, dtype)))
    return np.concatenate(out)


def kron_full(K, d, id_first):
    import scipy.sparse as sp
    K = sp.csr_matrix(np.asarray(K, dtype=np.float64))
    return sp.kron(sp.eye(d), K).tocsr() if id_first else sp.kron(K, sp.eye(d)).tocsr()


def dense_terms(A, x, transpose, dtype):
    """(A x in fp64, |A| |x|, 1.01 (L + 1) u) for the bound |got - (A x + res0)| <= 1.01 (L + 1) u (|A| |x| + |res0|): the forward
    error of a dot product of length L in ANY summation order plus the one add into the result, u the unit roundoff of `dtype`;
    A and x as the device holds them (rounded to `dtype`); transpose: A^T in place of A"""
    A = np.asarray(A, dtype=np.float64).astype(dtype).astype(np.float64)
    x = np.asarray(x, dtype=np.float64).astype(dtype).astype(np.float64)
    M = A.T if transpose else A
    u = 2.0 ** -24 if np.dtype(dtype) == np.float32 else 2.0 ** -53
    return M @ x, np.abs(M) @ np.abs(x), 1.01 * (M.shape[1] + 1) * u
