"""Directed operands for the elementwise proxes (ElemOperation1D / ElemOperationNorm2 over the 14 Function1D maps): values that
sit ON the branch thresholds of the maps, one ulp either side of them, and the special values (signed zeros, subnormals, squares
that underflow or overflow, the largest finite numbers, infinities, NaN).  Pure numpy and deterministic: the fixture generator
(tests/golden/make_golden.py edges) and the tests of the oracle and of the GPU kernels all draw their cases from here.

A case is (name, (op, fn, arg, tau_diag, tau, count, dim, interleaved, coeffs, invert_tau)) -- the arguments of oracle.prox_elem.

Coefficient families
  exact    scalar a = 1, b = 0, c = 1, d = 0, e = 0, tau_diag = 1, tau = 0.5: the step is exactly 0.5 (2 with invert_tau), the
           function's argument is the operand itself, and (alpha, beta) are chosen per function so that its own threshold is a
           representable operand (exact_params; checked there in rational arithmetic)
  general  per-element a, b, c, d, e with e != 0 (the fp64 denominator 1. + tau e), a[1] = 0 and c[2] = 0 (the degenerate branch
           of ElemOperation1D; ElemOperationNorm2 has none and divides by zero as the reference does), tau = 0.37
  a_one    scalar a = 1 with a vector e   } each makes one of the two host-decided shortcuts of the vector kernels true alone
  e_zero   vector a with scalar e = 0     }
"""
import fractions

import numpy as np

FUNCTIONS = ("zero", "abs", "square", "ind_leq0", "ind_geq0", "ind_eq0", "ind_box01", "max_pos0", "l0", "huber", "lq", "lq_plus_eps",
             "trunclin", "truncquad")
FAMILIES = ("exact", "general", "a_one", "e_zero")
LQ_ALPHAS = (1.0, 0.0, 0.5, 0.7)
EXACT_TAU, GENERAL_TAU = 0.5, 0.37
PAD = 0.625                     # the finite value that fills an operand array up to the count
NORM2_DIMS = (1, 2, 3, 4, 5, 7)
# the shapes (op, dim, interleaved, count) of the stored record: every operand / group of a case fits into the count
RECORD_SHAPES = [(0, 1, False, 65)] + [(1, dim, il, 160) for dim in NORM2_DIMS for il in (False, True)]


def exact_params(fn, step):
    """-> (alpha, beta, boundary): the coefficients alpha, beta of `fn` and the operand at which its branch condition holds with
    EQUALITY at the step `step` (0.5 or 2), all exactly representable; asserted in rational arithmetic"""
    F = fractions.Fraction
    s, alpha = F(step), F(3, 4)
    beta, x0 = F(21, 16), s
    if fn in ("abs", "max_pos0"):                    # x0 >= tau / x0 > tau
        assert x0 - s == 0
    elif fn == "l0":                                 # x0 * x0 > 2 tau
        x0 = F(1) if s == F(1, 2) else F(2)
        assert x0 * x0 == 2 * s
    elif fn == "huber":                              # |r| against 1, r = (x0 / tau) / (1 + alpha / tau)
        x0 = alpha + s
        assert (x0 / s) / (1 + alpha / s) == 1
    elif fn == "truncquad":                          # en_sq < beta
        x0 = 1 + 2 * s * alpha
        x_sq = x0 / (1 + 2 * s * alpha)
        beta = alpha * x_sq * x_sq + (x_sq - x0) * (x_sq - x0) / (2 * s)
        assert x_sq == 1 and beta == alpha + 2 * s * alpha * alpha
    elif fn == "trunclin":                           # en_sh < beta
        x0 = 1 + s * alpha
        x_sh = x0 - s * alpha
        beta = (x_sh - x0) * (x_sh - x0) / (2 * s) + alpha * abs(x_sh)
        assert x_sh == 1 and beta == alpha + s * alpha * alpha / 2
    elif fn == "ind_box01":                          # x0 > 1
        x0 = F(1)
    elif fn in ("ind_leq0", "ind_geq0"):             # x0 > 0 / x0 < 0
        x0 = F(0)
    for v in (alpha, beta, x0):                      # a few mantissa bits: exact in both data types
        assert v.denominator & (v.denominator - 1) == 0 and v.numerator < 2 ** 20, (fn, step, v)
    return float(alpha), float(beta), float(x0)


def operand_values(dtype, step, alpha, beta, boundary, lq=False):
    """the edge operands, the ones that matter most first (a short array still holds a threshold, a NaN and an overflowing value):
    every magnitude with both signs, and NaN.  lq: the finite ones with a magnitude in [2^-20, 2^20] only"""
    dt = np.dtype(dtype).type
    fi = np.finfo(dtype)
    lo, hi = (2.0 ** -80, 2.0 ** 64) if dt == np.float32 else (2.0 ** -600, 2.0 ** 600)      # the square underflows to 0 / overflows

    def around(v):
        v = dt(v)
        return [np.nextafter(v, dt(0)), v, np.nextafter(v, dt(np.inf))]
    with np.errstate(all="ignore"):
        mags = around(boundary) + [dt(hi), dt(np.inf), dt(0)] + around(step) + around(1) + [np.sqrt(dt(2) * dt(step)), dt(alpha), dt(alpha) + dt(step), dt(beta),
                                                                                        fi.tiny, fi.tiny / dt(8), fi.tiny * fi.eps, dt(lo), fi.max / dt(4), fi.max]
    vals = [dt(boundary), dt(np.nan), dt(hi)]
    for m in mags:
        vals += [dt(m), dt(-m)]
    vals = np.array(vals, dtype=dtype)
    if lq:
        with np.errstate(invalid="ignore"):
            vals = vals[np.isfinite(vals) & (np.abs(vals) >= 2.0 ** -20) & (np.abs(vals) <= 2.0 ** 20)]
    return vals


def norm2_groups(dtype, vals, dim, lq=False):
    """(groups, dim): for every edge operand s the groups (s, 0, ...) -- norm exactly |s| --, (s, 1, ...) and (s, s, ...); (3k, 4k, 0, ...)
    with the norm exactly 5k; the all-zero group.  The first four hold a threshold, a NaN, an overflowing square and the zero group."""
    dt = np.dtype(dtype).type
    lo, hi = (2.0 ** -80, 2.0 ** 62) if dt == np.float32 else (2.0 ** -600, 2.0 ** 598)
    def g(*lead):
        r = np.zeros(dim, dtype)
        r[:min(len(lead), dim)] = lead[:dim]
        return r
    groups = [g(s) for s in vals[:3]] + [g()] + [g(s) for s in vals[3:]] + [g(s, 1) for s in vals] + [np.full(dim, s, dtype) for s in vals]
    ks = (0.25, 0.5, 1.0) if lq else (0.25, 0.5, 1.0, lo, hi)
    groups += [g(3 * dt(k), 4 * dt(k)) for k in ks] + [g()]
    return np.array(groups, dtype=dtype)


def _vector_coeffs(family, fn, count, rng):
    """the seven coefficients of the families with per-element vectors"""
    alpha = 0.5 if fn == "lq" else 0.7
    a = rng.uniform(0.5, 2, count); b = rng.uniform(-1, 1, count); c = rng.uniform(0.1, 2, count)
    d = rng.uniform(-1, 1, count); e = rng.uniform(0.1, 1, count)
    if family == "general":
        if count > 1: a[1] = 0
        if count > 2: c[2] = 0
    if family == "a_one":
        a = 1.0
    if family == "e_zero":
        e = 0.0
    return [a, b, c, d, e, alpha, 1.3]


def _fill(dtype, items, count):
    """`items` (operands or groups) cut or padded with PAD to `count` of them"""
    items = np.asarray(items, dtype=dtype)
    out = np.full((count,) + items.shape[1:], PAD, dtype=dtype)
    n = min(count, len(items))
    out[:n] = items[:n]
    return out


def cases(dtype, shapes=RECORD_SHAPES, functions=FUNCTIONS):
    """yields (name, (op, fn, arg, tau_diag, tau, count, dim, interleaved, coeffs, invert_tau)) for every function, coefficient family,
    invert_tau and shape (op, dim, interleaved, count).  A count below the number of operands keeps the first ones."""
    dtype = np.dtype(dtype).type
    tname = np.dtype(dtype).name
    for fn in functions:
        lq = fn == "lq"
        for family in FAMILIES:
            for inv in (False, True):
                for sub, lq_alpha in enumerate(LQ_ALPHAS if (lq and family == "exact") else (None,)):
                    for op, dim, il, count in shapes:
                        # a generator of its own per case: a case does not depend on which others are drawn
                        rng = np.random.default_rng([FUNCTIONS.index(fn), FAMILIES.index(family), int(inv), sub, op, dim, int(il), count, np.dtype(dtype).itemsize])
                        if family == "exact":
                            tau = EXACT_TAU
                            step = 1.0 / tau if inv else tau
                            alpha, beta, boundary = exact_params(fn, step)
                            if lq:
                                alpha, beta = lq_alpha, 0.6
                                boundary = {1.0: step, 0.0: float(np.sqrt(2 * step))}.get(lq_alpha, 1.0)
                            coeffs = [1.0, 0.0, 1.0, 0.0, 0.0, alpha, beta]
                            td = np.ones(count * dim, dtype)
                        else:
                            tau = GENERAL_TAU
                            step, (alpha, beta, boundary) = tau, exact_params(fn, 0.5)
                            coeffs = _vector_coeffs(family, fn, count, rng)
                            td = rng.uniform(0.1, 2, count * dim).astype(dtype)
                        vals = operand_values(dtype, step, alpha, beta, boundary, lq)
                        if op == 0:
                            arg = _fill(dtype, vals, count)
                        else:
                            grp = _fill(dtype, norm2_groups(dtype, vals, dim, lq), count)      # (count, dim)
                            arg = np.ascontiguousarray(grp if il else grp.T).reshape(-1)
                        name = "%s_%s_%s%s_inv%d_op%d_dim%d_il%d_n%d" % (tname, fn, family, "" if lq_alpha is None else "_a%g" % lq_alpha, inv, op, dim, il, count)
                        yield name, (op, fn, arg, td, tau, count, dim, il, coeffs, inv)
