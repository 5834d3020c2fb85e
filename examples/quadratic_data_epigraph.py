"""TV denoising with a per-pixel quadratic data term on a label interval, written directly and in the lifted form of the
sublabel-accurate relaxations (Moellenhoff et al., CVPR 2016) with one label interval (L = 2):

    min_{u in [0, 1]}  TV(u) + sum_p a_p t_p^2 + b_p t_p + c_p,    t_p = gamma_1 + Delta u_p.

Direct form: rho_p(u) = a_p (gamma_1 + Delta u)^2 + b_p (gamma_1 + Delta u) + c_p = d_p u + e_p / 2 u^2 + const on [0, 1], which is
sum_1d('ind_box01', 1, 0, 1, d, e) with d = Delta (2 a gamma_1 + b), e = 2 a Delta^2.

Lifted form: with phi_p(x) = a_p x^2 + b_p x + c_p on [gamma_1, gamma_1 + Delta] the biconjugate is

    rho_p**(u) = sup_{v, q} u v - q,   (v / Delta, q + gamma_1 v / Delta) in epi phi_p*
               = sup_{(r, s) in epi phi_p*}  Delta u r + gamma_1 r - s,

a dual pair z = (r, s) per pixel in the epigraph of the conjugate piece -- what prost.function.sum_ind_epi_conjquad_1d projects onto
(alpha = gamma_1, beta = gamma_1 + Delta).  The coupling <u, Delta r> is an identity block scaled by Delta on the r rows and a zero
block on the s rows; the linear term gamma_1 r - s comes from prost.function.transform(..., d) with d = -gamma_1 on the r part and +1
on the s part (the saddle function holds -f*).  The constraint u in [0, 1] is implied by the two rays of phi*.  r and s are
sub-variables of one dual variable in the planar layout (all r, then all s).
Prints the energy of both formulations at their solutions.
usage: python examples/quadratic_data_epigraph.py [nx ny]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import prost_amd as prost
from prost_amd import synthetic

GAMMA_1, DELTA = 0.1, 0.8


def data_term(nx, ny):
    """a_p (t - f_p)^2 with per-pixel weights: -> a, b, c, f (f: a noisy image with values in the label interval and a little beyond)"""
    rng = np.random.default_rng(42)
    clean = synthetic.rof_image(nx, ny, 1, seed=2).astype(np.float64)
    f = clean + 0.1 * rng.standard_normal(nx * ny)
    a = 4.0 * rng.uniform(0.5, 2.0, nx * ny)
    return a, -2 * a * f, a * f * f, f


def energy(u, a, b, c, nx, ny):
    """sum_p a t^2 + b t + c at t = gamma_1 + Delta u, plus isotropic TV of u with forward differences (the gradient2d block: y fastest)"""
    img = u.reshape(nx, ny)
    dx = np.zeros_like(img)
    dy = np.zeros_like(img)
    dx[:-1, :] = img[1:, :] - img[:-1, :]
    dy[:, :-1] = img[:, 1:] - img[:, :-1]
    t = GAMMA_1 + DELTA * u
    return float(((a * t + b) * t + c).sum() + np.sqrt(dx ** 2 + dy ** 2).sum())


def options(max_iters):
    backend = prost.backend.pdhg(stepsize="boyd", residual_iter=10)
    opts = prost.options(max_iters=max_iters, num_cback_calls=250, verbose=False, tol_rel_primal=1e-7, tol_rel_dual=1e-7,
                         tol_abs_dual=1e-7, tol_abs_primal=1e-7)
    return backend, opts


def describe_direct(nx, ny, a, b):
    n = nx * ny
    u, q = prost.variable(n), prost.variable(2 * n)
    prob = prost.min_max_problem([u], [q])
    prob.add_function(u, prost.function.sum_1d("ind_box01", 1, 0, 1, DELTA * (2 * a * GAMMA_1 + b), 2 * a * DELTA ** 2))
    prob.add_function(q, prost.function.sum_norm2(2, False, "ind_leq0", 1, 1, 1))
    prob.add_dual_pair(u, q, prost.block.gradient2d(nx, ny, 1))
    return prob, u


def describe_lifted(nx, ny, a, b, c):
    n = nx * ny
    u, q, z = prost.variable(n), prost.variable(2 * n), prost.variable(2 * n)
    r = prost.sub_variable(z, n)
    s = prost.sub_variable(z, n)
    epi = prost.function.sum_ind_epi_conjquad_1d(False, a, b, c, GAMMA_1, GAMMA_1 + DELTA)
    linear = np.concatenate([np.full(n, -GAMMA_1), np.ones(n)])
    prob = prost.min_max_problem([u], [q, z])
    prob.add_function(u, prost.function.zero())
    prob.add_function(q, prost.function.sum_norm2(2, False, "ind_leq0", 1, 1, 1))
    prob.add_function(z, prost.function.transform(epi, 1, 0, 1, linear, 0))
    prob.add_dual_pair(u, q, prost.block.gradient2d(nx, ny, 1))
    prob.add_dual_pair(u, r, prost.block.identity(DELTA))
    prob.add_dual_pair(u, s, prost.block.zero())
    return prob, u, r, s


def main(nx=256, ny=192, max_iters=20000, verbose=True):
    a, b, c, f = data_term(nx, ny)
    backend, opts = options(max_iters)
    prob, u, r, s = describe_lifted(nx, ny, a, b, c)
    t0 = time.perf_counter()
    result = prost.solve(prob, backend, opts)
    elapsed = time.perf_counter() - t0
    e_lifted = energy(u.val, a, b, c, nx, ny)
    backend1, opts1 = options(max_iters)
    prob1, u1 = describe_direct(nx, ny, a, b)
    result1 = prost.solve(prob1, backend1, opts1)
    e_direct = energy(u1.val, a, b, c, nx, ny)
    if verbose:
        print("lifted form: %s after %d iterations, %.3f s, energy %.6f (u in [%.4f, %.4f])"
              % (result["result"], result["iters"], elapsed, e_lifted, float(u.val.min()), float(u.val.max())))
        print("direct form (sum_1d('ind_box01') with d, e): %s after %d iterations, energy %.6f" % (result1["result"], result1["iters"], e_direct))
    return result, e_lifted, e_direct, u.val, r.val, s.val, (a, b, c)


if __name__ == "__main__":
    main(*[int(v) for v in sys.argv[1:3]])
