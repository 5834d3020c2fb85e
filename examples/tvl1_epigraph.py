"""TV-L1 denoising with the data term written as an epigraph: beside tvl1_salt_and_pepper.py, the same model

    min_u  lmb |u - f|_1 + TV(u)

in the lifted form that the sublabel-accurate relaxations use,

    min_{u, t}  lmb sum t + ind{ t_i >= |u_i - f_i| } + TV(u).

|u - f| is the maximum of the two affine pieces u - f and f - u, so its epigraph is what prost.function.sum_ind_epi_polyhedral
projects onto: dim = 2 (one u and one t per pixel), two constraints per pixel (a = +1, b = f and a = -1, b = -f).  The linear term
sum t comes from prost.function.transform(..., d) with d = 0 on the u part and lmb on the t part.  u and t are sub-variables of one
primal variable in the planar layout (all u, then all t); the gradient acts on u alone.
Prints the energy of both formulations at their solutions.
usage: python examples/tvl1_epigraph.py [nx ny]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import prost_amd as prost
import tvl1_salt_and_pepper


def energy(u, f, nx, ny, lmb=1.0):
    """lmb |u - f|_1 + isotropic TV with forward differences (the gradient2d block: y fastest)"""
    img = u.reshape(nx, ny)
    dx = np.zeros_like(img)
    dy = np.zeros_like(img)
    dx[:-1, :] = img[1:, :] - img[:-1, :]
    dy[:, :-1] = img[:, 1:] - img[:, :-1]
    return float(lmb * np.abs(u - f).sum() + np.sqrt(dx ** 2 + dy ** 2).sum())


def describe(nx=512, ny=384, max_iters=50000):
    """-> (prob, backend, opts, u, t, f, clean); f and clean are those of tvl1_salt_and_pepper.describe"""
    _, backend, opts, _, f, clean = tvl1_salt_and_pepper.describe(nx, ny, 1, max_iters)
    n = nx * ny
    lmb = 1

    # pixel i owns the constraints 2 i and 2 i + 1:  u - t <= f_i  and  -u - t <= -f_i
    a = np.tile([1.0, -1.0], n)
    b = np.stack([f, -f], axis=1).ravel()
    count_vec = np.full(n, 2)
    index_vec = 2 * np.arange(n)
    epi = prost.function.sum_ind_epi_polyhedral(2, False, a, b, count_vec, index_vec)
    linear = np.concatenate([np.zeros(n), np.full(n, float(lmb))])

    z = prost.variable(2 * n)
    u = prost.sub_variable(z, n)
    t = prost.sub_variable(z, n)
    q = prost.variable(2 * n)
    prob = prost.min_max_problem([z], [q])
    prob.add_function(z, prost.function.transform(epi, 1, 0, 1, linear, 0))
    prob.add_function(q, prost.function.sum_norm2(2, False, "ind_leq0", 1, 1, 1))
    prob.add_dual_pair(u, q, prost.block.gradient2d(nx, ny, 1))
    return prob, backend, opts, u, t, f, clean


def main(nx=512, ny=384, max_iters=50000, verbose=True):
    prob, backend, opts, u, t, f, clean = describe(nx, ny, max_iters)
    t0 = time.perf_counter()
    result = prost.solve(prob, backend, opts)
    elapsed = time.perf_counter() - t0
    e_epi = energy(u.val, f, nx, ny)
    prob1, backend1, opts1, u1, _, _ = tvl1_salt_and_pepper.describe(nx, ny, 1, max_iters)
    result1 = prost.solve(prob1, backend1, opts1)
    e_abs = energy(u1.val, f, nx, ny)
    if verbose:
        print("epigraph form: %s after %d iterations, %.3f s, energy %.6f (sum t = %.6f, |u - f|_1 = %.6f)"
              % (result["result"], result["iters"], elapsed, e_epi, float(t.val.sum()), float(np.abs(u.val - f).sum())))
        print("sum_1d('abs') form: %s after %d iterations, energy %.6f" % (result1["result"], result1["iters"], e_abs))
    return result, e_epi, e_abs, u.val, t.val, f


if __name__ == "__main__":
    main(*[int(a) for a in sys.argv[1:3]])
