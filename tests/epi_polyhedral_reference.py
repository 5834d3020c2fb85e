"""NumPy reference of ind_epi_polyhedral: the projection of z0 = (x_1 .. x_d, y) onto { y >= max_i <a_i, x> - b_i }.

project_bruteforce   KKT enumeration over the subsets of at most dim constraints, fp64.  The projection is the closest feasible
                     point, and it is among the candidates (the equality-constrained projections), so the closest candidate that is
                     feasible is the answer whatever the degeneracy.
project_active_set   the algorithm of include/prost/prox/epi_polyhedral.hpp, statement by statement, for many groups in lockstep
                     in the arithmetic of `dtype`.  In fp64 it is the truth where the enumeration is too expensive; in dtype T it
                     gives e_T, the error a straightforward evaluation in T makes on the same input.

Constraint lists are given like the prox takes them: a (M, d) row per constraint, b (M,), and per group count and first index.
"""
import itertools

import numpy as np

TOL_FACTOR = 4       # kTolFactor
DEP_FACTOR = 64      # kDepFactor
STEP_CAP_A, STEP_CAP_B = 10, 0


def project_bruteforce(z0, a, b):
    """z0 (dim,), a (m, dim - 1), b (m,) -> the projection (dim,), fp64"""
    z0 = np.asarray(z0, np.float64)
    dim = z0.size
    a = np.asarray(a, np.float64).reshape(-1, dim - 1)
    b = np.asarray(b, np.float64).ravel()
    m = b.size
    if m == 0:
        return z0.copy()
    n = np.concatenate([a, -np.ones((m, 1))], axis=1)
    scale = max(1.0, np.abs(z0).max(), np.abs(b).max())
    nrm1 = np.abs(n).sum(axis=1)
    best, best_d = None, np.inf
    for q in range(0, min(dim, m) + 1):
        if q == 0:
            cand = z0[None, :]
        else:
            sub = np.array(list(itertools.combinations(range(m), q)))
            ns = n[sub]                                         # (S, q, dim)
            g = ns @ ns.transpose(0, 2, 1)
            rhs = ns @ z0 - b[sub]
            det = np.linalg.det(g)
            ok = det > 1e-12 * np.prod(np.einsum("sii->si", g), axis=1)
            if not ok.any():
                continue
            g, rhs, ns = g[ok], rhs[ok], ns[ok]
            lam = np.linalg.solve(g, rhs[:, :, None])[:, :, 0]
            cand = z0[None, :] - np.einsum("sq,sqd->sd", lam, ns)
        viol = (cand @ n.T - b[None, :]) / nrm1[None, :]
        feas = viol.max(axis=1) <= 1e-11 * scale
        if not feas.any():
            continue
        dist = np.linalg.norm(cand[feas] - z0[None, :], axis=1)
        k = int(np.argmin(dist))
        if dist[k] < best_d:
            best_d, best = dist[k], cand[feas][k]
    assert best is not None, "no feasible candidate: an epigraph is never empty"
    return best


def _violation(z, ag, bg, eps):
    """z (N, dim), ag (N, K, d), bg (N, K) -> v, violated"""
    d = ag.shape[2]
    s = np.zeros_like(bg)
    mag = np.zeros_like(bg)
    for j in range(d):
        p = ag[:, :, j] * z[:, j, None]
        s = s + p
        mag = mag + np.abs(p)
    v = s - z[:, d, None] - bg
    mag = mag + np.abs(z[:, d, None]) + np.abs(bg)
    return v, v > TOL_FACTOR * eps * mag


def _solve_gram(act, on, r, eps):
    """ActiveSet::SolveGram for every group: act (N, DIM, d), on (N, DIM), r (N, DIM) -> G^-1 r"""
    N, DIM, D = act.shape
    T = act.dtype.type
    one, zero = T(1), T(0)
    r = r.copy()
    L = np.zeros((N, DIM, DIM), T)
    inv = np.zeros((N, DIM), T)
    for s in range(DIM):
        for t in range(s + 1):
            g = np.full(N, one, T)
            for j in range(D):
                g = g + act[:, s, j] * act[:, t, j]
            L[:, s, t] = np.where(on[:, s] & on[:, t], g, one if s == t else zero)
    for j in range(DIM):
        p = L[:, j, j].copy()
        for k in range(j):
            p = p - L[:, j, k] * L[:, j, k]
        p = np.where(p > eps * eps, p, eps * eps)
        root = np.sqrt(p)
        inv[:, j] = one / root
        L[:, j, j] = root
        for i in range(j + 1, DIM):
            s_ = L[:, i, j].copy()
            for k in range(j):
                s_ = s_ - L[:, i, k] * L[:, j, k]
            L[:, i, j] = s_ * inv[:, j]
    for j in range(DIM):
        s_ = r[:, j].copy()
        for k in range(j):
            s_ = s_ - L[:, j, k] * r[:, k]
        r[:, j] = s_ * inv[:, j]
    for j in range(DIM - 1, -1, -1):
        s_ = r[:, j].copy()
        for k in range(j + 1, DIM):
            s_ = s_ - L[:, k, j] * r[:, k]
        r[:, j] = s_ * inv[:, j]
    return r


def project_active_set(z0, a, b, cnt, idx, dtype=np.float64, info=None):
    """z0 (N, dim), a (M, dim - 1), b (M,), cnt (N,), idx (N,) -> (N, dim) in `dtype`.  info, a dict, receives 'steps' (N,) and
    'capped' (N,)."""
    T = np.dtype(dtype).type
    eps = T(np.finfo(T).eps)
    z0 = np.asarray(z0).astype(T)
    N, DIM = z0.shape
    D = DIM - 1
    A = np.asarray(a).astype(T).reshape(-1, D)
    B = np.asarray(b).astype(T).ravel()
    cnt = np.asarray(cnt, np.int64).ravel()
    idx = np.asarray(idx, np.int64).ravel()
    kmax = max(1, int(cnt.max()) if N else 1)
    if B.size == 0:
        A, B = np.zeros((1, D), T), np.zeros(1, T)
    lane = np.arange(kmax)[None, :]
    valid = lane < cnt[:, None]
    cidx = np.where(valid, idx[:, None] + lane, 0)
    ag, bg = A[cidx], B[cidx]
    rows = np.arange(N)
    z = z0.copy()
    act = np.zeros((N, DIM, D), T)
    u = np.zeros((N, DIM), T)
    bs = np.zeros((N, DIM), T)
    on = np.zeros((N, DIM), bool)
    polished = np.zeros(N, bool)
    pa, pb, pu = np.zeros((N, D), T), np.zeros(N, T), np.zeros(N, T)
    pending = np.zeros(N, bool)
    done = np.zeros(N, bool)
    capped = np.zeros(N, bool)
    steps = np.zeros(N, np.int64)
    cap = STEP_CAP_A * (cnt + DIM) + STEP_CAP_B
    one, zero = T(1), T(0)
    dep = T(DEP_FACTOR) * eps
    with np.errstate(all="ignore"):
        while not done.all():
            v, viol = _violation(z, ag, bg, eps)
            viol &= valid
            best = np.argmax(np.where(viol, v, -np.inf), axis=1)
            anyv = viol.any(axis=1)
            need = ~done & ~pending
            fin = need & ~anyv
            pol = fin & ~polished & on.any(axis=1)          # Polish(): once, onto the active hyperplanes, then one more scan
            if pol.any():
                r = np.zeros((N, DIM), T)
                for s in range(DIM):
                    v_ = -z[:, D] - bs[:, s]
                    for j in range(D):
                        v_ = v_ + act[:, s, j] * z[:, j]
                    r[:, s] = np.where(on[:, s], v_, zero)
                r = _solve_gram(act, on, r, eps)
                zn = z.copy()
                for s in range(DIM):
                    for j in range(D):
                        zn[:, j] = zn[:, j] - r[:, s] * act[:, s, j]
                    zn[:, D] = zn[:, D] + r[:, s]
                z = np.where(pol[:, None], zn, z)
                polished |= pol
            done |= fin & ~pol
            start = need & anyv
            pa = np.where(start[:, None], ag[rows, best], pa)
            pb = np.where(start, bg[rows, best], pb)
            pu = np.where(start, zero, pu)
            pending |= start
            hit = ~done & (steps >= cap)
            capped |= hit
            done |= hit
            run = ~done & pending
            if not run.any():
                continue
            steps += run
            r = np.zeros((N, DIM), T)
            q = on.sum(axis=1)
            for s in range(DIM):
                g = np.full(N, one, T)
                for j in range(D):
                    g = g + act[:, s, j] * pa[:, j]
                r[:, s] = np.where(on[:, s], g, zero)
            r = _solve_gram(act, on, r, eps)
            d = np.zeros((N, DIM), T)
            nn = np.full(N, one, T)
            for j in range(D):
                d[:, j] = pa[:, j]
                nn = nn + pa[:, j] * pa[:, j]
            d[:, D] = -one
            rmax = np.zeros(N, T)
            for s in range(DIM):
                for j in range(D):
                    d[:, j] = d[:, j] - r[:, s] * act[:, s, j]
                d[:, D] = d[:, D] + r[:, s]
                rmax = np.maximum(rmax, np.abs(r[:, s]))
            dd = np.zeros(N, T)
            for j in range(DIM):
                dd = dd + d[:, j] * d[:, j]
            indep = (q < DIM) & (dd > dep * dep * nn)
            vp, _ = _violation(z, pa[:, None, :], pb[:, None], eps)
            vp = np.maximum(vp[:, 0], zero)
            t2 = vp / np.where(indep, dd, one)
            t1 = np.zeros(N, T)
            drop = np.full(N, -1)
            for s in range(DIM):
                c = on[:, s] & (r[:, s] > dep * rmax)
                ratio = u[:, s] / np.where(c, r[:, s], one)
                take = c & ((drop < 0) | (ratio < t1))
                t1 = np.where(take, ratio, t1)
                drop = np.where(take, s, drop)
            stuck = run & ~indep & (drop < 0)
            capped |= stuck
            done |= stuck
            run &= ~stuck
            full = indep & ((drop < 0) | (t2 <= t1))
            t = np.where(full, t2, t1)
            move = run & indep
            for j in range(DIM):
                z[:, j] = np.where(move, z[:, j] - t * d[:, j], z[:, j])
            for s in range(DIM):
                un = u[:, s] - t * r[:, s]
                u[:, s] = np.where(run, np.where(on[:, s] & (un > zero), un, zero), u[:, s])
            pu = np.where(run, pu + t, pu)
            placed = np.zeros(N, bool)
            addm = run & full
            for s in range(DIM):
                here = addm & ~placed & ~on[:, s]
                act[:, s, :] = np.where(here[:, None], pa, act[:, s, :])
                bs[:, s] = np.where(here, pb, bs[:, s])
                u[:, s] = np.where(here, pu, u[:, s])
                on[:, s] |= here
                placed |= here
            pending &= ~addm
            dropm = run & ~full
            for s in range(DIM):
                here = dropm & (drop == s)
                on[:, s] &= ~here
                u[:, s] = np.where(here, zero, u[:, s])
        if capped.any():
            worst = np.where(valid, _violation(np.concatenate([z0[:, :D], np.zeros((N, 1), T)], axis=1), ag, bg, eps)[0] , -np.inf).max(axis=1)
            fb = z0.copy()
            fb[:, D] = np.maximum(z0[:, D], worst.astype(T))
            z = np.where(capped[:, None], fb, z)
    if info is not None:
        info["steps"] = steps
        info["capped"] = capped
    return z


def random_lists(rng, count, dim, ks, shared=False, shuffle=False):
    """constraint lists for `count` groups whose lengths cycle through ks: a, b, cnt, idx (randn coefficients).  shared: one list of
    max(ks) constraints that every group names; shuffle: the lists lie in a random order, so idx is not monotone."""
    ks = list(ks)
    if shared:
        m = max(max(ks), 1)
        cnt = np.full(count, max(ks), np.int64)
        idx = np.zeros(count, np.int64)
    else:
        cnt = np.array([ks[g % len(ks)] for g in range(count)], np.int64)
        order = rng.permutation(count) if shuffle else np.arange(count)
        idx = np.zeros(count, np.int64)
        pos = 0
        for g in order:
            idx[g] = pos
            pos += cnt[g]
        m = max(pos, 1)
    a = rng.standard_normal((m, dim - 1))
    b = rng.standard_normal(m)
    return a, b, cnt, idx


def halfspace_distance(z, a, b, cnt, idx):
    """per group: the largest distance by which z lies outside one of its halfspaces (<= 0: feasible), fp64"""
    z = np.asarray(z, np.float64)
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    out = np.full(z.shape[0], -np.inf)
    for g in range(z.shape[0]):
        if cnt[g] == 0:
            continue
        ai, bi = a[idx[g]:idx[g] + cnt[g]], b[idx[g]:idx[g] + cnt[g]]
        out[g] = ((ai @ z[g, :-1] - z[g, -1] - bi) / np.sqrt((ai * ai).sum(axis=1) + 1)).max()
    return out


def directed_cases(dim):
    """name -> (a (m, d), b (m,), points (P, dim)): the degenerate lists of the GPU tests"""
    d = dim - 1
    rng = np.random.default_rng(40 + dim)
    eye = np.eye(d)
    pts = np.concatenate([rng.standard_normal((6, dim)), 1000 * rng.standard_normal((6, dim))])
    a1 = rng.standard_normal((1, d))
    depth = 1 + rng.random((8, 1)) * 50
    below = np.concatenate([rng.uniform(-0.9, 0.9, (8, d)) * depth / d, -depth], axis=1)      # |x|_1 <= 0.9 |y|, y <= -1: the polar cone of both pyramids
    edge = np.zeros((4, dim))
    edge[:, 0] = [2.0, 5.0, -3.0, 40.0]
    edge[:, -1] = [-1.0, 1.0, 0.5, -30.0]                    # x = (t, 0, ..), y < |t|: lands on the facet of +-e_1, an edge of the l1 pyramid for d >= 2
    signs = np.array([[1 if (k >> j) & 1 else -1 for j in range(d)] for k in range(2 ** d)], float)
    return {
        "single": (a1, np.array([0.25]), pts),
        "duplicate": (np.repeat(rng.standard_normal((2, d)), 2, axis=0), np.repeat(rng.standard_normal(2), 2), pts),
        "parallel": (np.concatenate([a1, a1, 2 * a1]), np.array([0.5, -0.5, 0.1]), pts),
        "linf_pyramid": (np.concatenate([eye, -eye]), np.zeros(2 * d), np.concatenate([below, edge, pts])),
        "l1_pyramid": (signs, np.zeros(2 ** d), np.concatenate([below, edge, pts])),
        "zero_rows": (np.zeros((3, d)), np.array([0.5, -2.0, 1.0]), pts),
        "zero_and_slopes": (np.concatenate([np.zeros((1, d)), eye]), np.array([1.0] + [0.0] * d), pts),
    }
