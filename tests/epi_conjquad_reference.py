"""NumPy reference of ind_epi_conjquad_1d: the projection of (y0, t0) onto { t >= phi*(y) }, phi(x) = a x^2 + b x + c on
[alpha, beta], a >= 0.

project()      include/prost/prox/epi_conjquad.hpp restated operation for operation (Piece::Set, Piece::Conj, ArcStart,
               Projector::Begin / Step / Finish / Fallback), for many groups in lockstep and in any NumPy precision; returns the
               region label per group.
from_answer()  builds a case from its answer: a boundary point P of the chosen piece and z0 = P + s n with n the outward unit normal
               there, so that the projection of z0 is P by construction and no solver is involved in the truth.  Computed in long
               double and rounded once.
random_cases() groups with a prescribed share of every region, built that way.
"""
import numpy as np

INSIDE, LEFT, RIGHT, VERTEX, ARC = 0, 1, 2, 3, 4
REGION_NAMES = ["inside", "left", "right", "vertex", "arc"]
STEP_CAP = 32            # epi_conjquad.hpp kStepCap; tests that have the library take prost_hip_epi_conjquad_step_cap instead


def _piece(a, b, c, alpha, beta, dtype):
    a, b, c, alpha, beta = (np.asarray(v, dtype) for v in (a, b, c, alpha, beta))
    inf = dtype(np.inf)
    has_left, has_right = alpha > -inf, beta < inf
    al, be = np.where(has_left, alpha, dtype(0)), np.where(has_right, beta, dtype(0))
    ya = np.where(has_left, (dtype(2) * a) * al + b, -inf)
    yb = np.where(has_right, (dtype(2) * a) * be + b, inf)
    fa = (a * al + b) * al + c
    fb = (a * be + b) * be + c
    return dict(a=a, b=b, c=c, alpha=alpha, beta=beta, has_left=has_left, has_right=has_right, ya=ya, yb=yb, fa=fa, fb=fb)


def _conj(p, y, dtype):
    with np.errstate(all="ignore"):
        u = y - p["b"]
        arc = (u * u) / (dtype(4) * p["a"]) - p["c"]
        return np.where(y <= p["ya"], p["alpha"] * y - p["fa"], np.where(y >= p["yb"], p["beta"] * y - p["fb"], arc))


def conj(y, a, b, c, alpha, beta, dtype=np.float64):
    """phi*(y) per group"""
    dtype = np.dtype(dtype).type
    y, a, b, c, alpha, beta = np.broadcast_arrays(*(np.asarray(v, dtype) for v in (y, a, b, c, alpha, beta)))
    return _conj(_piece(a, b, c, alpha, beta, dtype), y, dtype)


def _arc_start(q, k, w, dtype):
    q2 = q * q
    s = np.minimum(w, np.cbrt(w / (dtype(2) * q2)))
    s = np.where(k > dtype(1), np.minimum(s, w / k), s)
    neg = np.minimum(w, np.maximum(np.cbrt(w / q2), np.sqrt(np.abs(k)) / q))
    return np.where(k >= dtype(0), s, neg)


def project(y0, t0, a, b, c, alpha, beta, dtype=np.float64, cap=STEP_CAP, info=None):
    """-> y, t, region (arrays of one entry per group; y, t in `dtype`).  info (a dict) receives `steps` and `capped`."""
    dtype = np.dtype(dtype).type
    y0, t0, a, b, c, alpha, beta = (np.array(v) for v in np.broadcast_arrays(*(np.atleast_1d(np.asarray(v, dtype)) for v in (y0, t0, a, b, c, alpha, beta))))
    p = _piece(a, b, c, alpha, beta, dtype)
    zero, one = dtype(0), dtype(1)
    with np.errstate(all="ignore"):
        y, t = y0.copy(), t0.copy()
        region = np.full(y0.shape, -1)
        inside = t0 >= _conj(p, y0, dtype)
        region[inside] = INSIDE
        viol = (alpha * y0 - t0) - p["fa"]
        pat = alpha * p["ya"] - p["fa"]
        left = ~inside & p["has_left"] & (viol > zero) & ((y0 - p["ya"]) + alpha * (t0 - pat) <= zero)
        m = viol / (alpha * alpha + one)
        y, t = np.where(left, y0 - m * alpha, y), np.where(left, t0 + m, t)
        region[left] = LEFT
        viol = (beta * y0 - t0) - p["fb"]
        pbt = beta * p["yb"] - p["fb"]
        right = ~inside & ~left & p["has_right"] & (viol > zero) & ((y0 - p["yb"]) + beta * (t0 - pbt) >= zero)
        m = viol / (beta * beta + one)
        y, t = np.where(right, y0 - m * beta, y), np.where(right, t0 + m, t)
        region[right] = RIGHT
        rest = ~inside & ~left & ~right
        vertex = rest & ~(a > zero)
        arc = rest & (a > zero)
        region[vertex] = VERTEX
        region[arc] = ARC
        u0, s0 = y0 - b, t0 + c
        neg = u0 < zero
        w = np.abs(u0)
        apex = vertex | (arc & ~(w > zero))
        y, t = np.where(apex, b, y), np.where(apex, -c, t)
        pending = arc & (w > zero)
        q = one / (dtype(4) * a)
        k = one - (dtype(2) * q) * s0
        u = _arc_start(q, k, w, dtype)
        steps = np.zeros(y0.shape, int)
        for _ in range(int(cap)):
            if not pending.any():
                break
            steps[pending] += 1
            q2, uu = q * q, u * u
            g = ((dtype(2) * q2) * uu + k) * u - w
            gp = (dtype(6) * q2) * uu + k
            nxt = u - g / gp
            go = pending & (gp > zero) & (nxt < u) & (nxt > zero)
            fin = pending & ~go
            u = np.where(go, nxt, u)
            y = np.where(fin, b + np.where(neg, -u, u), y)
            t = np.where(fin, q * (u * u) - c, t)
            pending = go
        capped = pending.copy()
        y = np.where(capped, y0, y)
        t = np.where(capped, np.maximum(t0, _conj(p, y0, dtype)), t)
    if info is not None:
        info["steps"], info["capped"] = steps, capped
    return y.astype(dtype), t.astype(dtype), region


def outside(y, t, a, b, c, alpha, beta):
    """max(phi*(y) - t, 0) in long double"""
    L = np.longdouble
    return np.maximum(conj(np.asarray(y, L), a, b, c, alpha, beta, L) - np.asarray(t, L), 0).astype(np.float64)


def from_answer(region, a, b, c, alpha, beta, x, d, s):
    """Cases from their answers, all arguments arrays of one entry per group.
    left / right: P on the ray at distance d >= 0 (in y) from P_a / P_b, z0 = P + s n, s >= 0.
    arc:          P at the slope x in [alpha, beta] (y = 2 a x + b, t = a x^2 - c), z0 = P + s n.
    vertex:       a = 0, P = (b, -c), n the unit vector along (x, -1) with x in [alpha, beta].
    inside:       z0 = P = (b + d, phi*(b + d) + s), d of either sign, s >= 0.
    -> z0 (N, 2), P (N, 2) as float64, computed in long double."""
    L = np.longdouble
    region = np.asarray(region)
    a, b, c, alpha, beta, x, d, s = (np.asarray(v, L) for v in (a, b, c, alpha, beta, x, d, s))
    p = _piece(a, b, c, alpha, beta, L)
    with np.errstate(all="ignore"):
        slope = np.select([region == LEFT, region == RIGHT, region == INSIDE], [alpha, beta, L(0)], x)
        py = np.select([region == LEFT, region == RIGHT, region == VERTEX, region == INSIDE], [p["ya"] - d, p["yb"] + d, b, b + d], (L(2) * a) * x + b)
        pt = np.select([region == LEFT, region == RIGHT, region == VERTEX, region == INSIDE],
                       [alpha * py - p["fa"], beta * py - p["fb"], -c, _conj(p, py, L) + s], a * x * x - c)
        norm = np.sqrt(slope * slope + L(1))
        move = np.where(region == INSIDE, L(0), s)
        z0 = np.stack([py + move * slope / norm, pt - move / norm], axis=1)
    P = np.stack([py, pt], axis=1)
    assert np.isfinite(z0).all() and np.isfinite(P).all()
    return z0.astype(np.float64), P.astype(np.float64)


A_VALUES = (0.0, 1e-6, 1.0, 1e3)
SHARES = ((INSIDE, 0.22), (LEFT, 0.22), (RIGHT, 0.22), (ARC, 0.24), (VERTEX, 0.10))


def f32(x):
    return np.asarray(x, np.float64).astype(np.float32).astype(np.float64)


def random_cases(rng, count, scale=1.0, a_values=A_VALUES, shares=SHARES, infinite=0.15, fixed=None):
    """count groups with the regions in the given shares (shuffled), coefficients that float32 holds exactly, points at `scale`.
    fixed: {name: value} for coefficients that are one scalar for all groups (alpha / beta finite); a region the fixed piece does not
    have (vertex for a > 0, arc for a = 0) is left out and its share goes to the others in proportion.
    -> dict(a, b, c, alpha, beta, z0, P, region): the designed region and its answer P (z0 and P in float64, before any rounding
    of z0 to another precision); fixed coefficients come back as arrays of one entry"""
    fixed = dict(fixed or {})
    if "a" in fixed:
        shares = [(r, w) for r, w in shares if r != (VERTEX if fixed["a"] > 0 else ARC)]
        a_values = [fixed["a"]]
    total = sum(w for _, w in shares)
    kinds = np.concatenate([np.full(int(np.ceil(w / total * count)), r) for r, w in shares])
    kinds = rng.permutation(kinds)[:count]
    assert kinds.size == count
    pos = [v for v in a_values if v > 0] or [1.0]
    a = np.where(kinds == VERTEX, 0.0, np.where(kinds == ARC, rng.choice(pos, size=count), rng.choice(a_values, size=count)))
    lo, hi = np.sort(f32(2 * rng.standard_normal((2, count))), axis=0)
    hi = np.where(hi > lo, hi, lo + 0.5)                                     # vertex and arc want alpha < beta
    same = (rng.random(count) < 0.1) & (kinds != VERTEX) & (kinds != ARC)       # alpha = beta: the epigraph of a line
    width = hi - lo
    if "alpha" in fixed or "beta" in fixed:
        lo = np.full(count, float(fixed["alpha"])) if "alpha" in fixed else f32(fixed["beta"] - width)
        hi = np.full(count, float(fixed["beta"])) if "beta" in fixed else f32(lo + width)
        same &= False
    hi = np.where(same, lo, hi)
    inf_lo = (rng.random(count) < infinite) & (a > 0) & (kinds != LEFT) & ("alpha" not in fixed)
    inf_hi = (rng.random(count) < infinite) & (a > 0) & (kinds != RIGHT) & ("beta" not in fixed)
    alpha, beta = np.where(inf_lo, -np.inf, lo), np.where(inf_hi, np.inf, hi)
    b, c = f32(scale * rng.standard_normal(count)), f32(scale * rng.standard_normal(count))
    if "b" in fixed:
        b = np.full(count, float(fixed["b"]))
    if "c" in fixed:
        c = np.full(count, float(fixed["c"]))
    x = lo + (hi - lo) * rng.random(count)
    x = np.where(inf_lo & (rng.random(count) < 0.5), lo - 3 * rng.random(count), x)
    x = np.where(inf_hi & (rng.random(count) < 0.5), hi + 3 * rng.random(count), x)
    d = scale * rng.random(count) * np.where(kinds == INSIDE, rng.choice([-3.0, 3.0], size=count), 1.0)
    s = scale * rng.random(count) * 2
    a = f32(a)
    z0, P = from_answer(kinds, a, b, c, alpha, beta, x, d, s)
    out = dict(a=a, b=b, c=c, alpha=alpha, beta=beta, z0=z0, P=P, region=kinds)
    for name in fixed:
        assert (out[name] == out[name][0]).all() and out[name][0] == np.float32(fixed[name])
        out[name] = out[name][:1]
    return out


def directed_cases(scale=1.0):
    """the named corner cases -> dict name -> dict like random_cases (a few groups each)"""
    S = scale
    inf = np.inf

    def case(region, a, b, c, alpha, beta, x, d, s):
        n = max(np.size(v) for v in (region, a, b, c, alpha, beta, x, d, s))
        region, a, b, c, alpha, beta, x, d, s = (np.broadcast_to(np.asarray(v, float if i else int), (n,)).copy() for i, v in enumerate((region, a, b, c, alpha, beta, x, d, s)))
        z0, P = from_answer(region, a, b, c, alpha, beta, x, d, s)
        return dict(a=a, b=b, c=c, alpha=alpha, beta=beta, z0=z0, P=P, region=region)

    A4 = np.array(A_VALUES)
    pos = A4[A4 > 0]
    out = {}
    # alpha = beta: a line, whatever a is; both sides of the contact point and exactly below it
    out["alpha_eq_beta"] = case([LEFT, LEFT, RIGHT, RIGHT, LEFT, RIGHT, INSIDE, INSIDE], np.tile(A4, 2), 0.5 * S, -0.25 * S, 0.75, 0.75, 0.75,
                                [S, 0, S, 0, 3 * S, 3 * S, S, -S], [2 * S, S, 2 * S, S, 0, 0, S, 0])
    # infinite bounds: the full parabola, and one ray only
    out["both_infinite"] = case(ARC, np.repeat(pos, 3), 0.5 * S, 0.25 * S, -inf, inf, np.tile([-4.0, 0.5, 7.0], 3), 0, 1.5 * S)
    out["left_infinite"] = case([ARC, ARC, RIGHT, RIGHT, INSIDE] * 3, np.repeat(pos, 5), -S, S, -inf, 1.5, [-6.0, 1.5, 0, 0, 0] * 3, [0, 0, S, 0, -S] * 3, S)
    out["right_infinite"] = case([ARC, ARC, LEFT, LEFT, INSIDE] * 3, np.repeat(pos, 5), S, -S, -0.5, inf, [5.0, -0.5, 0, 0, 0] * 3, [0, 0, S, 0, S] * 3, S)
    # u0 = 0: straight below the apex of the arc
    out["below_the_apex"] = case(ARC, np.repeat(pos, 2), 0.5 * S, 0.25 * S, -1, 2, 0, 0, np.tile([S, 1e-3 * S], 3))
    # exactly on the boundary (s = 0) of every piece, and at the contact points
    out["on_the_boundary"] = case([LEFT, RIGHT, ARC, ARC, ARC, VERTEX, LEFT, RIGHT], [1, 1, 1, 1e3, 1e-6, 0, 0, 1e3], 0.5 * S, -0.5 * S, -1, 2,
                                  [0, 0, 0.5, -1, 2, 0, 0, 0], [S, S, 0, 0, 0, 0, 0, 0], 0)
    # exactly on the normal line through P_a / P_b (d = 0)
    out["normal_through_contact"] = case([LEFT, RIGHT] * 4, np.repeat(A4, 2), -0.5 * S, 0.5 * S, -1.5, 0.75, 0, 0, [S, S, 3 * S, 3 * S] * 2)
    # the vertex of a = 0: the whole normal cone, its two edges included
    out["vertex_cone"] = case(VERTEX, 0, 0.5 * S, 0.25 * S, -1, 2, [-1, -0.5, 0, 1, 2], 0, [S, 2 * S, S, 0.5 * S, S])
    # alpha < 0 < beta with |alpha| beta > 1: a point high on the right, below the right ray, satisfies the left ray's tangential
    # test; only "below its own line" keeps it off the left ray (and the mirror image)
    out["high_on_the_other_side"] = case([RIGHT, LEFT, RIGHT, LEFT], [1, 1, 0, 0], 0, 0, -2, 3, 0, [94 * S, 96 * S, 100 * S, 100 * S], [28.77 * S, 93 * S, 30 * S, 90 * S])
    return out
