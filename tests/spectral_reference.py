"""fp64 NumPy composition of the spectral proxes (elem_operation:singular_nx2 / eigen_2x2 / eigen_3x3), shared by
tests/test_spectral_frontend.py (CPU: the functor headers compiled for the host) and tests/test_gpu_spectral.py (the kernel).

Decompose with np.linalg.eigh / np.linalg.svd, take the scalar prox of the eigen / singular values with the CPU oracle's pinned
sum_1d (oracle.eval_prox), recompose.  The two l1-ball functions are written out here.  Nothing of the code under test is used."""
import numpy as np

import oracle
import prost_amd as prost

FUNCTIONS_1D = prost.function.FUNCTIONS_1D
SINGULAR_1D = FUNCTIONS_1D[:10]                        # zero .. huber: what the reference registers for singular_nx2
DISCONTINUOUS = ("l0", "lq", "trunclin", "truncquad")   # lq with alpha < 1


def per_group(v, G):
    v = np.atleast_1d(np.asarray(v, dtype=np.float64)).ravel()
    return np.full(G, v[0]) if v.size == 1 else v


def scalar_prox(fn, vals, tau, coeffs):
    """prox of c f(a t - b) + d t + (e/2) t^2 at vals (G, k), step tau (G,), coeffs 7 x (scalar | (G,)): the oracle's sum_1d"""
    G, k = vals.shape
    co = [np.repeat(per_group(c, G), k) for c in coeffs]
    out = oracle.eval_prox(prost.function.sum_1d(fn, *co), vals.ravel(), 1.0, np.repeat(tau, k), np.float64)
    return np.asarray(out, dtype=np.float64).reshape(G, k)


def project_l1_ball(y, radius):
    """rows of y (G, 2) onto {|x1| + |x2| <= radius}, radius (G,)"""
    m = np.abs(y)
    inside = m.sum(axis=1) <= radius
    hi, lo = m.max(axis=1), m.min(axis=1)
    both = (hi + lo - radius) / 2
    theta = np.where(lo > both, both, hi - radius)
    out = np.sign(y) * np.maximum(m - theta[:, None], 0.0)
    return np.where(inside[:, None], y, out)


def pair_prox(fn, vals, tau, coeffs):
    """the 2-D functions of singular_nx2 under the coefficient convention of elem_operation_1d.hpp"""
    G = vals.shape[0]
    a, b, c, d, e, alpha, beta = [per_group(v, G) for v in coeffs]
    if fn not in ("ind_l1_ball", "moreau:ind_l1_ball"):
        return scalar_prox(fn, vals, tau, coeffs)
    den = 1 + tau * e
    plain = (vals - (tau * d)[:, None]) / den[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        y = (a[:, None] * (vals - (d * tau)[:, None])) / den[:, None] - b[:, None]
        step = c * a * a * tau / den
        if fn == "ind_l1_ball":
            x = project_l1_ball(y, alpha)
        else:
            x = y - step[:, None] * project_l1_ball(y / step[:, None], alpha)
        full = (x + b[:, None]) / a[:, None]
    degenerate = (a == 0) | (c == 0)
    return np.where(degenerate[:, None], plain, full)


def marked(fn, vals, tau, coeffs):
    """exclusion rule for the discontinuous functions: a group is marked when the scalar prox at lambda +- 1e-3 differs from the value
    at lambda by more than 1e-2 (evaluated on the composition alone)"""
    if fn not in DISCONTINUOUS:
        return np.zeros(vals.shape[0], dtype=bool)
    p0 = scalar_prox(fn, vals, tau, coeffs)
    bad = np.zeros(vals.shape[0], dtype=bool)
    for dlt in (-1e-3, 1e-3):
        bad |= (np.abs(scalar_prox(fn, vals + dlt, tau, coeffs) - p0) > 1e-2).any(axis=1)
    return bad


def groups_from_flat(flat, dim, interleaved):
    flat = np.asarray(flat, dtype=np.float64).ravel()
    return flat.reshape(-1, dim) if interleaved else flat.reshape(dim, -1).T


def flat_from_groups(vec, interleaved):
    return np.ascontiguousarray(vec if interleaved else vec.T).ravel()


def compose_eigen(vec, n, fn, tau, coeffs):
    """vec (G, n*n) column-major matrices -> (result (G, n*n), marked (G,))"""
    G = vec.shape[0]
    M = vec.reshape(G, n, n).transpose(0, 2, 1)
    w, V = np.linalg.eigh((M + M.transpose(0, 2, 1)) / 2)
    p = scalar_prox(fn, w, tau, coeffs)
    R = np.einsum("gij,gj,gkj->gik", V, p, V)
    return R.transpose(0, 2, 1).reshape(G, n * n), marked(fn, w, tau, coeffs)


def compose_singular(vec, fn, tau, coeffs):
    """vec (G, 2n): first column, then second column of the n x 2 matrix -> (result (G, 2n), marked (G,)).  The part of a zero
    singular value is dropped; an all-zero matrix gives res[0] = p1, res[n + 1] = p2 (n > 1)"""
    G, dim = vec.shape
    n = dim // 2
    M = vec.reshape(G, 2, n).transpose(0, 2, 1)
    U, S, Vt = np.linalg.svd(M, full_matrices=False)
    if S.shape[1] == 1:                                   # n = 1: the second singular value is zero
        S = np.concatenate([S, np.zeros((G, 1))], axis=1)
        U = np.concatenate([U, np.zeros((G, 1, 1))], axis=2)
        Vt = np.concatenate([Vt, np.zeros((G, 1, 2))], axis=1)
    p = pair_prox(fn, S, tau, coeffs)
    keep = S > 1e-7 * S[:, :1]
    R = np.einsum("gij,gj,gjk->gik", U, p * keep, Vt)
    out = R.transpose(0, 2, 1).reshape(G, dim)
    zero = S[:, 0] == 0
    if zero.any():
        out[zero] = 0
        out[zero, 0] = p[zero, 0]
        if n > 1:
            out[zero, n + 1] = p[zero, 1]
    return out, marked(fn, S, tau, coeffs)
