"""References for prost.block.dataterm_sublabel (no code of the block is used here):

  (a) matrix(nx, ny, L, left, right): the explicit scipy matrix of the operator, rows [r ; s], columns [u ; w], planes of N = nx ny;
  (b) forward / adjoint: the two per-pixel marches of include/prost/linop/dataterm_sublabel.hpp restated operation for operation on
      NumPy arrays of a given dtype (every NumPy operation on arrays of one dtype rounds once in that dtype, and there is no
      contraction), with the accumulating form res0 + value;
  (c) sums: the row / column sum formulas, in the order the header adds them.

Labels: delta = (right - left) / (L - 1) and gamma_i = left + i delta are formed in double and then rounded to the dtype.
"""
import numpy as np
import scipy.sparse as sp


def labels(L, left, right, dtype=np.float64):
    """-> delta (a dtype scalar), gamma (k values of dtype)"""
    k = L - 1
    delta = (np.float64(right) - np.float64(left)) / np.float64(k)
    gamma = np.float64(left) + np.arange(k, dtype=np.float64) * delta
    return np.dtype(dtype).type(delta), gamma.astype(dtype)


def matrix(nx, ny, L, left, right, dtype=np.float64):
    """(a): 2 N k x 2 N k, csc, float64 entries holding the dtype-rounded delta and gamma; gamma_i == 0 is no entry"""
    N, k = nx * ny, L - 1
    delta, gamma = labels(L, left, right, dtype)
    delta, gamma = float(delta), gamma.astype(np.float64)
    eye = sp.identity(N, format="csc")
    ru = delta * sp.identity(k)
    rw = sp.diags(gamma) - delta * sp.csc_matrix(np.triu(np.ones((k, k)), 1))
    sw = -sp.identity(k)
    K = sp.bmat([[sp.kron(ru, eye), sp.kron(rw, eye)], [None, sp.kron(sw, eye)]], format="csc")
    K.eliminate_zeros()
    K.sort_indices()
    assert K.shape == (2 * N * k, 2 * N * k)
    return K


def forward(x, N, L, left, right, dtype, res0=None):
    """(b): [r ; s] = K [u ; w], or res0 + that"""
    k = L - 1
    delta, gamma = labels(L, left, right, dtype)
    x = np.asarray(x).astype(dtype)
    u, w = x[:N * k].reshape(k, N), x[N * k:].reshape(k, N)
    r, s = np.empty((k, N), dtype), np.empty((k, N), dtype)
    S = np.zeros(N, dtype)
    for i in range(k - 1, -1, -1):
        r[i] = (delta * u[i] + gamma[i] * w[i]) - delta * S
        s[i] = -w[i]
        S = S + w[i]
    out = np.concatenate([r.ravel(), s.ravel()])
    assert out.dtype == np.dtype(dtype)
    return out if res0 is None else np.asarray(res0).astype(dtype) + out


def adjoint(y, N, L, left, right, dtype, res0=None):
    """(b): [u ; w] = K^T [r ; s], or res0 + that"""
    k = L - 1
    delta, gamma = labels(L, left, right, dtype)
    y = np.asarray(y).astype(dtype)
    r, s = y[:N * k].reshape(k, N), y[N * k:].reshape(k, N)
    u, w = np.empty((k, N), dtype), np.empty((k, N), dtype)
    P = np.zeros(N, dtype)
    for i in range(k):
        u[i] = delta * r[i]
        w[i] = (gamma[i] * r[i] - s[i]) - delta * P
        P = P + r[i]
    out = np.concatenate([u.ravel(), w.ravel()])
    assert out.dtype == np.dtype(dtype)
    return out if res0 is None else np.asarray(res0).astype(dtype) + out


def product(x, N, L, left, right, transpose, dtype, res0=None):
    return (adjoint if transpose else forward)(x, N, L, left, right, dtype, res0)


def sums(N, L, left, right, alpha=1.0, dtype=np.float64):
    """(c): sum |entry|^alpha of every row and every column, one constant per plane -> (rows, cols) of dtype
    r_i row: |delta|^a + |gamma_i|^a + (k - 1 - i) |delta|^a;  s_i row: 1;  u_i column: |delta|^a;  w_i column: |gamma_i|^a + 1 + i |delta|^a"""
    k = L - 1
    t = np.dtype(dtype).type
    delta, gamma = labels(L, left, right, dtype)
    alpha = t(alpha)
    pd = np.power(np.abs(delta), alpha)
    pg = np.where(gamma == 0, t(0), np.power(np.abs(gamma), alpha)).astype(dtype)
    i = np.arange(k).astype(dtype)
    rows = np.concatenate([(pd + pg) + (t(k - 1) - i) * pd, np.ones(k, dtype)])
    cols = np.concatenate([np.full(k, pd, dtype), (pg + t(1)) + i * pd])
    assert rows.dtype == cols.dtype == np.dtype(dtype)
    return np.repeat(rows, N), np.repeat(cols, N)
