"""Function (prox) builders -- Python mirror of matlab/+prost/+function/*.m.

Each builder returns ``func(idx, count) -> [name, idx, size, diagsteps, data]`` like the MATLAB
closures (sum_1d.m:79-80, sum_norm2.m:85-86, conjugate.m:7-15, sum_ind_epi_quad.m:17-20,
zero.m:3).  Models h(x) = c f(ax - b) + dx + 0.5 e x^2.
"""
import numpy as np

FUNCTIONS_1D = ("zero", "abs", "square", "ind_leq0", "ind_geq0", "ind_eq0", "ind_box01",
                "max_pos0", "l0", "huber", "lq", "lq_plus_eps", "trunclin", "truncquad")


def _coeff(v):
    return np.atleast_1d(np.asarray(v, dtype=np.float64)).ravel()


def sum_1d(fun, a=1, b=0, c=1, d=0, e=0, alpha=0, beta=0):
    coeffs = [_coeff(v) for v in (a, b, c, d, e, alpha, beta)]
    return lambda idx, count: ["elem_operation:1d:" + fun, idx, count, True,
                               [count, 1, False, coeffs]]


def sum_norm2(dim, interleaved, fun, a=1, b=0, c=1, d=0, e=0, alpha=0, beta=0):
    coeffs = [_coeff(v) for v in (a, b, c, d, e, alpha, beta)]
    return lambda idx, count: ["elem_operation:norm2:" + fun, idx, count, False,
                               [count // dim, dim, bool(interleaved), coeffs]]


def sum_singular_nx2(dim, interleaved, fun, a=1, b=0, c=1, d=0, e=0, alpha=0, beta=0):
    """sum_singular_nx2.m:1-30: h(sigma_1) + h(sigma_2) of the n x 2 matrix a group of dim = 2n values holds (first column first),
    h as in sum_1d.  `fun` is appended to the name as it stands, like the .m builder does: 'sum_1d:<fn>' for the ten functions
    zero .. huber ('<fn>' alone names the same prox here), 'ind_l1_ball' or 'moreau:ind_l1_ball' (radius alpha)."""
    coeffs = [_coeff(v) for v in (a, b, c, d, e, alpha, beta)]
    return lambda idx, count: ["elem_operation:singular_nx2:" + fun, idx, count, False,
                               [count // dim, dim, bool(interleaved), coeffs]]


def sum_eigen_2x2(interleaved, fun, a=1, b=0, c=1, d=0, e=0, alpha=0, beta=0):
    """sum_eigen_2x2.m:1-22: h(lambda_1) + h(lambda_2) of the symmetrised column-major 2 x 2 matrix a group of 4 values holds"""
    coeffs = [_coeff(v) for v in (a, b, c, d, e, alpha, beta)]
    return lambda idx, count: ["elem_operation:eigen_2x2:" + fun, idx, count, False,
                               [count // 4, 4, bool(interleaved), coeffs]]


def sum_eigen_3x3(interleaved, fun, a=1, b=0, c=1, d=0, e=0, alpha=0, beta=0):
    """sum_eigen_3x3.m:1-24: h(lambda_1) + h(lambda_2) + h(lambda_3) of the symmetrised column-major 3 x 3 matrix a group of 9 values holds"""
    coeffs = [_coeff(v) for v in (a, b, c, d, e, alpha, beta)]
    return lambda idx, count: ["elem_operation:eigen_3x3:" + fun, idx, count, False,
                               [count // 9, 9, bool(interleaved), coeffs]]


def sum_eigen_nxn(n, interleaved, fun, a=1, b=0, c=1, d=0, e=0, alpha=0, beta=0):
    """sum_eigen_nxn.m:1-26: h(lambda_1) + .. + h(lambda_n) of the symmetrised row-major n x n matrix a group of n * n values holds,
    1 <= n <= 32"""
    n = int(n)
    if n < 1 or n > 32:
        raise ValueError("n must be between 1 and 32")
    coeffs = [_coeff(v) for v in (a, b, c, d, e, alpha, beta)]
    return lambda idx, count: ["elem_operation:eigen_nxn:" + fun, idx, count, False,
                               [count // (n * n), n * n, bool(interleaved), coeffs]]


def sum_mass_norm(n, interleaved, cost=1):
    """sum_mass_norm.m:1-21: cost times the mass norm of a 2-vector in R^n, n = 4 (6 components: the upper triangle of a skew-symmetric
    matrix, row by row) or n = 5 (10 components).  cost: a scalar or one value per group.  The .m builder drops the cost for n = 5; here
    a cost other than the scalar 1 is appended to the description and honoured."""
    cost = _coeff(cost)
    if n == 4:
        return lambda idx, count: ["elem_operation:mass4", idx, count, False, [count // 6, 6, bool(interleaved), [cost]]]
    if n == 5:
        if cost.size == 1 and cost[0] == 1:
            return lambda idx, count: ["elem_operation:mass5", idx, count, False, [count // 10, 10, bool(interleaved)]]
        return lambda idx, count: ["elem_operation:mass5", idx, count, False, [count // 10, 10, bool(interleaved), [cost]]]
    raise ValueError("Mass norm not implemented for n \\notin {4, 5}")


def sum_ind_comass_ball(n, interleaved):
    """sum_ind_comass_ball.m:1-18: indicator of the unit ball of the comass norm of a 2-vector in R^n, n = 4 or 5: the conjugate of
    sum_mass_norm(n, interleaved)"""
    if n == 4:
        return lambda idx, count: ["elem_operation:ind_comass4_ball", idx, count, False, [count // 6, 6, bool(interleaved)]]
    if n == 5:
        return lambda idx, count: ["elem_operation:ind_comass5_ball", idx, count, False, [count // 10, 10, bool(interleaved)]]
    raise ValueError("Indicator of comass norm ball not implemented for n \\notin {4, 5}")


def conjugate(fun):
    def make(idx, count):
        child = fun(idx, count)
        return ["moreau", child[1], child[2], child[3], [child]]
    return make


def sum_ind_epi_quad(dim, interleaved, a, b, c):
    coeffs = [_coeff(a), _coeff(b), _coeff(c)]
    return lambda idx, count: ["ind_epi_quad", idx, count, False,
                               [count // dim, dim, bool(interleaved), coeffs]]


def zero():
    return lambda idx, count: ["zero", idx, count, True, []]


def transform(fun, a=1, b=0, c=1, d=0, e=0):
    """transform.m:1-50: c f(ax - b) + dx + (e/2) x^2 around ANY function `fun`"""
    coeffs = [_coeff(v) for v in (a, b, c, d, e)]

    def make(idx, count):
        child = fun(idx, count)
        return ["transform", child[1], child[2], child[3], coeffs + [child]]
    return make


def permute(fun, perm):
    """permute.m:1-17: composition with a permutation (local, 0-based indices)"""
    perm = np.asarray(perm, dtype=np.int64).ravel()

    def make(idx, count):
        child = fun(idx, count)
        return ["permute", child[1], child[2], child[3], [child, perm]]
    return make


def sum_ind_halfspace(dim, interleaved, a, b):
    """sum_ind_halfspace.m:1-19: projection onto a^T x <= b per group (a: dim or dim*count, b: 1 or count)"""
    coeffs = [_coeff(a), _coeff(b)]
    return lambda idx, count: ["ind_halfspace", idx, count, False,
                               [count // dim, dim, bool(interleaved), coeffs]]


def sum_ind_soc(dim, interleaved, alpha):
    """sum_ind_soc.m:1-20: projection onto alpha ||x|| <= y, variables ordered (x_1, .., x_{d-1}, y) planar"""
    return lambda idx, count: ["ind_soc", idx, count, False,
                               [count // dim, dim, bool(interleaved), float(alpha)]]


def sum_ind_sum(dim, interleaved):
    """sum_ind_sum.m:1-9: sum-to-one constraint per group"""
    return lambda idx, count: ["elem_operation:ind_sum", idx, count, False,
                               [count // dim, dim, bool(interleaved)]]


def sum_ind_simplex(dim, interleaved):
    """sum_ind_simplex.m:1-9: indicator of the unit simplex per group"""
    return lambda idx, count: ["elem_operation:ind_simplex", idx, count, False,
                               [count // dim, dim, bool(interleaved)]]


def sum_ind_sum2(dim, inds, s1, dim2=None, inds2=None, s2=None):
    """sum_ind_sum2.m:1-13: sum constraints over index arrays (one or two families)"""
    inds = np.asarray(inds, dtype=np.int64).ravel()
    if dim2 is None:
        return lambda idx, count: ["ind_sum", idx, count, True, [int(dim), inds, float(s1)]]
    inds2 = np.asarray(inds2, dtype=np.int64).ravel()
    return lambda idx, count: ["ind_sum", idx, count, True, [int(dim), inds, float(s1), int(dim2), inds2, float(s2)]]


def ind_range(A, AA=None):
    """ind_range.m:1-11: indicator of the range of the sparse m x n matrix A (full column rank); its prox is the projection
    x = A (A'A)^-1 A' y.  AA = A'A as a full matrix (computed here when left out).  A sparse AA is handed on as it is: the factory
    answers "Matrix AA must be dense!"."""
    import scipy.sparse as sp
    A = sp.csc_matrix(A, dtype=np.float64, copy=True)
    if AA is None:
        AA = (A.T @ A).toarray()
    if not sp.issparse(AA):
        AA = np.array(AA, dtype=np.float64, copy=True)
    return lambda idx, count: ["ind_range", idx, count, False, [A, AA]]


def sum_ind_epi_polyhedral(dim, interleaved, a, b, count_vec, index_vec):
    """sum_ind_epi_polyhedral(dim, interleaved, a, b, count_vec, index_vec): indicator of the epigraphs y >= max_i <a_i, x> - b_i per
    group (x_1 .. x_{dim-1}, y), 2 <= dim <= 4.  Group g owns the count_vec[g] constraints that start at index_vec[g] (0-based,
    counted in constraints; groups may share a list, the starts need not be monotone).  a: the dim - 1 coefficients of one constraint
    adjacent, len(a) = len(b) * (dim - 1).  Its prox is the projection onto the epigraph."""
    def vec(v):
        return np.asarray(v, dtype=np.float64).ravel()
    coeffs = [vec(a), vec(b), vec(count_vec), vec(index_vec)]
    return lambda idx, count: ["ind_epi_polyhedral", idx, count, False,
                               [count // dim, dim, bool(interleaved), coeffs]]


def sum_ind_epi_conjquad_1d(interleaved, a, b, c, alpha, beta):
    """sum_ind_epi_conjquad_1d(interleaved, a, b, c, alpha, beta): indicator of the epigraphs t >= phi*(y) per group (y, t), phi* the
    conjugate of phi(x) = a x^2 + b x + c on [alpha, beta] (+inf elsewhere): a left ray of slope alpha, an arc, a right ray of slope
    beta.  Each coefficient is a scalar or one value per group; a >= 0, alpha <= beta; alpha = -inf / beta = +inf are allowed for
    a > 0.  Its prox is the projection onto the epigraph."""
    coeffs = [np.asarray(v, dtype=np.float64).ravel() for v in (a, b, c, alpha, beta)]
    return lambda idx, count: ["ind_epi_conjquad_1d", idx, count, False,
                               [count // 2, 2, bool(interleaved), coeffs]]
