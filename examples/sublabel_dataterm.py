"""TV denoising with a piecewise quadratic data term in the sublabel-accurate lifting (Moellenhoff, Laude, Moeller, Lellmann, Cremers,
CVPR 2016) with L > 2 labels, i.e. k = L - 1 label intervals:

    min_t  sum_p rho_p(t_p) + TV(t),   t_p in [left, right],   rho_p = phi_{p,i} = a_{p,i} x^2 + b_{p,i} x + c_{p,i} on interval i.

Lifted form.  Per pixel x = [u ; w]: u in R^k is the lifted labelling (t = left + delta sum_i u_i; a label value in interval j at the
fraction alpha is u = (1, .., 1, alpha, 0, .., 0)), w in the unit simplex of R^k weighs the intervals.  The data term becomes

    sum_i sup_{(r_i, s_i) in epi phi_i*}  m_i r_i - w_i s_i,     m_i = gamma_i w_i + delta (u_i - sum_{j > i} w_j),

which is <K [u ; w], [r ; s]> with K = prost.block.dataterm_sublabel(nx, ny, L, left, right) (no matrix is formed) and the indicator of
the epigraphs of the conjugate pieces, prost.function.sum_ind_epi_conjquad_1d(False, a, b, c, gamma_i, gamma_i + delta), as f* directly.
u carries no function of its own (zero()): u_i in [0, 1] and the order of the u_i follow from the rays of the phi_i*.  The regulariser is
sum_i delta TV(u_i) through gradient2d(nx, ny, k) on the u sub-variable; in the discrete setting it only dominates TV(t).
Everything is k planes of N = nx ny pixels (element (p, i) at i N + p); x = [u ; w] and z = [r ; s] are sub-variables of one primal and
one dual variable.

Two data terms: a convex quadratic a_p (t - f_p)^2 cut into k pieces (the direct form, sum_1d('ind_box01') with d and e, solves the same
problem: the energies are compared), and the truncated quadratic min(a_p (t - f_p)^2, nu), where piece i is the quadratic or the constant
nu, decided at the interval's midpoint -- non-convex, which is what the relaxation is for.
Prints the energies.
usage: python examples/sublabel_dataterm.py [nx ny L]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import prost_amd as prost
from prost_amd import synthetic

LEFT, RIGHT = 0.0, 1.0
NU = 0.5


def label_grid(L, left=LEFT, right=RIGHT):
    """-> delta, gamma (the left ends of the k = L - 1 intervals)"""
    delta = (right - left) / (L - 1)
    return delta, left + np.arange(L - 1) * delta


def noisy_image(nx, ny):
    """-> f (a noisy image with values in [left, right] and a little beyond), per-pixel weights a"""
    rng = np.random.default_rng(42)
    clean = synthetic.rof_image(nx, ny, 1, seed=2).astype(np.float64)
    f = LEFT + (RIGHT - LEFT) * clean + 0.1 * rng.standard_normal(nx * ny)
    return f, 4.0 * rng.uniform(0.5, 2.0, nx * ny)


def convex_pieces(f, weight, L):
    """weight (t - f)^2 on every interval -> a, b, c of shape N k (plane i holds piece i of every pixel)"""
    k = L - 1
    return np.tile(weight, k), np.tile(-2 * weight * f, k), np.tile(weight * f * f, k)


def truncated_pieces(f, weight, L, nu=NU, left=LEFT, right=RIGHT):
    """min(weight (t - f)^2, nu): piece i is the quadratic where it lies below nu at the midpoint of interval i, the constant nu elsewhere"""
    delta, gamma = label_grid(L, left, right)
    mid = (gamma + delta / 2)[:, None]
    quad = weight[None, :] * (mid - f[None, :]) ** 2 < nu
    a = np.where(quad, weight[None, :], 0.0)
    b = np.where(quad, -2 * weight * f, 0.0)
    c = np.where(quad, weight * f * f, nu)
    return a.ravel(), b.ravel(), c.ravel()


def tv(img):
    """isotropic TV with forward differences (the gradient2d block: y fastest)"""
    dx = np.zeros_like(img)
    dy = np.zeros_like(img)
    dx[:-1, :] = img[1:, :] - img[:-1, :]
    dy[:, :-1] = img[:, 1:] - img[:, :-1]
    return float(np.sqrt(dx ** 2 + dy ** 2).sum())


def piecewise_value(t, a, b, c, L, left=LEFT, right=RIGHT):
    """sum_p phi_{p, i(p)}(t_p), i(p) the interval t_p lies in (t clipped to [left, right])"""
    delta, _ = label_grid(L, left, right)
    n = t.size
    i = np.clip(np.floor((t - left) / delta).astype(int), 0, L - 2)
    g = i * n + np.arange(n)
    tc = np.clip(t, left, right)
    return float(((a[g] * tc + b[g]) * tc + c[g]).sum())


def options(max_iters, tol=1e-6):
    backend = prost.backend.pdhg(stepsize="boyd", residual_iter=10)
    opts = prost.options(max_iters=max_iters, num_cback_calls=250, verbose=False, tol_rel_primal=tol, tol_rel_dual=tol, tol_abs_dual=tol,
                         tol_abs_primal=tol)
    return backend, opts


def describe_lifted(nx, ny, L, a, b, c, regulariser=True, left=LEFT, right=RIGHT):
    """-> prob, (u, w, r, s): the sub-variables, N k values each"""
    n, k = nx * ny, L - 1
    delta, gamma = label_grid(L, left, right)
    x, z = prost.variable(2 * n * k), prost.variable(2 * n * k)
    u, w = prost.sub_variable(x, n * k), prost.sub_variable(x, n * k)
    r, s = prost.sub_variable(z, n * k), prost.sub_variable(z, n * k)
    duals = [z]
    if regulariser:
        q = prost.variable(2 * n * k)
        duals = [q, z]
    prob = prost.min_max_problem([x], duals)
    prob.add_function(u, prost.function.zero())
    prob.add_function(w, prost.function.sum_ind_simplex(k, False))
    alpha = np.repeat(gamma, n)
    prob.add_function(z, prost.function.sum_ind_epi_conjquad_1d(False, a, b, c, alpha, alpha + delta))
    if regulariser:
        prob.add_function(q, prost.function.sum_norm2(2, False, "ind_leq0", 1 / delta, 1, 1))        # sum_i delta TV(u_i)
        prob.add_dual_pair(u, q, prost.block.gradient2d(nx, ny, k))
    prob.add_dual_pair(x, z, prost.block.dataterm_sublabel(nx, ny, L, left, right))
    return prob, (u, w, r, s)


def recover(u, n, L, left=LEFT, right=RIGHT):
    """t = left + delta sum_i u_i"""
    delta, _ = label_grid(L, left, right)
    return left + delta * np.asarray(u).reshape(L - 1, n).sum(axis=0)


def describe_direct(nx, ny, f, weight):
    """the convex quadratic, directly: t = left + R v, v in [0, 1]; weight (left + R v - f)^2 = d v + e / 2 v^2 + const"""
    n, R = nx * ny, RIGHT - LEFT
    v, q = prost.variable(n), prost.variable(2 * n)
    prob = prost.min_max_problem([v], [q])
    prob.add_function(v, prost.function.sum_1d("ind_box01", 1, 0, 1, R * 2 * weight * (LEFT - f), 2 * weight * R ** 2))
    prob.add_function(q, prost.function.sum_norm2(2, False, "ind_leq0", 1 / R, 1, 1))
    prob.add_dual_pair(v, q, prost.block.gradient2d(nx, ny, 1))
    return prob, v


def main(nx=128, ny=96, L=8, max_iters=50000, verbose=True, data="both"):
    """-> dict per data term: result, t, energy (and energy_direct, t_direct for the convex one), the sub-variables' values"""
    n = nx * ny
    f, weight = noisy_image(nx, ny)
    out = {}
    for name in (("convex", "truncated") if data == "both" else (data,)):
        a, b, c = convex_pieces(f, weight, L) if name == "convex" else truncated_pieces(f, weight, L)
        backend, opts = options(max_iters)
        prob, (u, w, r, s) = describe_lifted(nx, ny, L, a, b, c)
        t0 = time.perf_counter()
        result = prost.solve(prob, backend, opts)
        elapsed = time.perf_counter() - t0
        t = recover(u.val, n, L)
        energy = piecewise_value(t, a, b, c, L) + tv(t.reshape(nx, ny))
        res = dict(result=result, t=t, energy=energy, u=u.val, w=w.val, r=r.val, s=s.val, coeffs=(a, b, c))
        if verbose:
            print("%s data, lifted with L = %d: %s after %d iterations, %.3f s, energy %.6f (t in [%.4f, %.4f])"
                  % (name, L, result["result"], result["iters"], elapsed, energy, float(t.min()), float(t.max())))
        if name == "convex":
            backend1, opts1 = options(max_iters)
            prob1, v = describe_direct(nx, ny, f, weight)
            result1 = prost.solve(prob1, backend1, opts1)
            t1 = LEFT + (RIGHT - LEFT) * v.val
            res.update(result_direct=result1, t_direct=t1, energy_direct=piecewise_value(t1, a, b, c, L) + tv(t1.reshape(nx, ny)))
            if verbose:
                print("convex data, direct form (sum_1d('ind_box01') with d, e): %s after %d iterations, energy %.6f; gap of the lifted form %.3g (relative)"
                      % (result1["result"], result1["iters"], res["energy_direct"], (energy - res["energy_direct"]) / abs(res["energy_direct"])))
        out[name] = res
    return out


if __name__ == "__main__":
    main(*[int(v) for v in sys.argv[1:4]])
