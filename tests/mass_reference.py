"""fp64 NumPy composition of the mass-norm operations (elem_operation:mass4 / mass5 / ind_comass4_ball / ind_comass5_ball), shared by
tests/test_eigen_mass_frontend.py (CPU: the functor headers compiled for the host) and tests/test_gpu_eigen_mass.py (the kernels).

A group holds the upper triangle of a skew-symmetric n x n matrix A row by row.  With A = U S V^T (np.linalg.svd) the result is the same
triangle of U f(S) V^T: f(s) = max(s - step, 0) for the mass norm, f(s) = min(s, 1) for the comass ball.  U f(S) V^T = A g(A^T A) is a
matrix function of A, so it does not depend on the bases the SVD picks inside the (always paired) singular subspaces, and f(0) = 0
covers the null space.  Nothing of the code under test is used."""
import numpy as np

DIM = {4: 6, 5: 10}


def pairs(n):
    return [(i, j) for i in range(n) for j in range(i + 1, n)]


def skew_from_groups(vec, n):
    """vec (G, n (n - 1) / 2) -> A (G, n, n)"""
    vec = np.asarray(vec, dtype=np.float64)
    A = np.zeros((vec.shape[0], n, n))
    for k, (i, j) in enumerate(pairs(n)):
        A[:, i, j] = vec[:, k]
        A[:, j, i] = -vec[:, k]
    return A


def groups_from_skew(A, n):
    return np.stack([A[:, i, j] for i, j in pairs(n)], axis=1)


def f_mass(s, step):
    return np.maximum(s - step[:, None], 0.0)


def f_comass(s, step):
    return np.minimum(s, 1.0)


def compose_mass(vec, n, conjugate, step):
    """vec (G, dim) groups, step (G,) -> the prox of step * mass norm (conjugate False) or the projection onto the comass ball"""
    A = skew_from_groups(vec, n)
    U, S, Vt = np.linalg.svd(A)
    p = (f_comass if conjugate else f_mass)(S, np.asarray(step, dtype=np.float64))
    return groups_from_skew(np.einsum("gij,gj,gjk->gik", U, p, Vt), n)


def mass_inputs(rng, G, n, scale, rounded):
    """randn * scale groups whose first rows are the special ones; returns (vec, names of the special rows in order)"""
    dim = DIM[n]
    vec = rng.standard_normal((G, dim)) * scale
    vec[0] = 0                                             # a zero group
    vec[1] = 0
    vec[1, 2] = 3.5 * scale                                # a single non-zero component
    vec[2] = 0
    k12, k34 = pairs(n).index((0, 1)), pairs(n).index((2, 3))
    vec[2, k12] = vec[2, k34] = 2.0 * scale                # omega_12 = omega_34: sigma_1 = sigma_2
    vec[3] = vec[3] * 1e-3                                 # a group scaled by 1e-3
    return rounded(vec), ("zero group", "single component", "omega_12 = omega_34", "scaled by 1e-3")
