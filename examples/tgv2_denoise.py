"""Second-order total generalised variation denoising (TGV^2, Bredies / Kunisch / Pock):

    min_{u, v}  lmb/2 |u - f|^2 + a1 |grad u - v|_{2,1} + a0 |E v|_{2,1}

with g = grad u - v and e = E v as constrained variables, K = [grad -I ; 0 E].  E, the symmetrised gradient of the vector field v, is
prost.block.sym_gradient2d(nx, ny, nc): nothing is stored per pixel.  TGV^2 prefers piecewise affine images, where TV prefers
piecewise constant ones (staircasing): on a ramp with a step it comes closer to the clean image than TV on the same data.
twin=True hands E over as prost.block.sparse of the explicit matrix instead.  usage: python examples/tgv2_denoise.py [nx ny nc]"""
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import scipy.sparse as sp

import prost_amd as prost
from multilabel_fast import spmat_gradient2d


def ramp_image(nx, ny, nc=1, noise=0.05, seed=1):
    """clean = 0.02 x + 0.03 y + 0.5 [x > nx / 2], the same in every channel, column-major (y fastest), and clean + noise"""
    x, y = np.meshgrid(np.arange(nx, dtype=np.float64), np.arange(ny, dtype=np.float64), indexing="ij")
    clean = np.tile((0.02 * x + 0.03 * y + 0.5 * (x > nx // 2)).reshape(-1), nc)
    return clean, clean + noise * np.random.default_rng(seed).standard_normal(clean.size)


def spmat_sym_gradient2d(nx, ny, nc=1, w=math.sqrt(0.5)):
    """the explicit E: with Dx, Dy the halves of spmat_gradient2d(nx, ny, 1), Bx = -Dx^T, By = -Dy^T,
    E = [kron(I, Bx) 0 ; 0 kron(I, By) ; w kron(I, By) w kron(I, Bx)]"""
    N = nx * ny
    D = sp.csr_matrix(spmat_gradient2d(nx, ny, 1))
    Bx, By = sp.kron(sp.identity(nc), -D[:N].T), sp.kron(sp.identity(nc), -D[N:].T)
    Z = sp.csr_matrix((nc * N, nc * N))
    return sp.bmat([[Bx, Z], [Z, By], [w * By, w * Bx]], format="csc")


def options(tol, max_iters, num_cback_calls=0):
    return prost.options(max_iters=max_iters, num_cback_calls=num_cback_calls, verbose=False, tol_rel_primal=tol, tol_abs_primal=tol, tol_rel_dual=tol,
                         tol_abs_dual=tol)


def describe(nx, ny, nc=1, lmb=8.0, a1=1.0, a0=2.0, w=math.sqrt(0.5), tol=1e-5, max_iters=20000, f=None, twin=False):
    """-> prob, backend, opts, u, v, f, clean.  f: the data (None: ramp_image); twin: block.sparse of the explicit E"""
    N = nx * ny
    clean = None
    if f is None:
        clean, f = ramp_image(nx, ny, nc)
    u = prost.variable(nc * N)
    v = prost.variable(2 * nc * N)
    g = prost.variable(2 * nc * N)
    e = prost.variable(3 * nc * N)
    prob = prost.min_problem([u, v], [g, e])
    prob.add_function(u, prost.function.sum_1d("square", 1, f, lmb, 0, 0))
    prob.add_function(g, prost.function.sum_norm2(2, False, "abs", 1, 0, a1, 0, 0))
    prob.add_function(e, prost.function.sum_norm2(3, False, "abs", 1, 0, a0, 0, 0))
    prob.add_constraint(u, g, prost.block.gradient2d(nx, ny, nc))
    prob.add_constraint(v, g, prost.block.identity(-1))
    prob.add_constraint(v, e, prost.block.sparse(spmat_sym_gradient2d(nx, ny, nc, w)) if twin else prost.block.sym_gradient2d(nx, ny, nc, w))
    backend = prost.backend.pdhg(stepsize="boyd", residual_iter=1)
    return prob, backend, options(tol, max_iters), u, v, f, clean


def describe_tv(nx, ny, nc, f, lmb=8.0, tol=1e-5, max_iters=20000):
    """min_u lmb/2 |u - f|^2 + |grad u|_{2,1} on the same data, for comparison"""
    u = prost.variable(nc * nx * ny)
    g = prost.variable(2 * nc * nx * ny)
    prob = prost.min_problem([u], [g])
    prob.add_function(u, prost.function.sum_1d("square", 1, f, lmb, 0, 0))
    prob.add_function(g, prost.function.sum_norm2(2, False, "abs", 1, 0, 1, 0, 0))
    prob.add_constraint(u, g, prost.block.gradient2d(nx, ny, nc))
    return prob, prost.backend.pdhg(stepsize="boyd", residual_iter=1), options(tol, max_iters), u


def rmse(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, dtype=np.float64).ravel() - np.asarray(b, dtype=np.float64).ravel()) ** 2)))


def main(nx=256, ny=192, nc=1, max_iters=20000, verbose=True, twin=False):
    prob, backend, opts, u, _, f, clean = describe(nx, ny, nc, max_iters=max_iters, twin=twin)
    t0 = time.perf_counter()
    result = prost.solve(prob, backend, opts)
    elapsed = time.perf_counter() - t0
    img = np.array(u.val, dtype=np.float64).ravel()
    prob_tv, backend_tv, opts_tv, u_tv = describe_tv(nx, ny, nc, f, max_iters=max_iters)
    result_tv = prost.solve(prob_tv, backend_tv, opts_tv)
    img_tv = np.array(u_tv.val, dtype=np.float64).ravel()
    if verbose:
        print("TGV^2: %s after %d iterations, %.3f s on %s; RMSE to the clean image %.4f (TV: %.4f after %d iterations, data: %.4f)"
              % (result["result"], result["iters"], elapsed, result["path"], rmse(img, clean), rmse(img_tv, clean), result_tv["iters"], rmse(f, clean)))
    return result, img, result_tv, img_tv, f, clean


if __name__ == "__main__":
    size = [int(a) for a in sys.argv[1:4]]
    main(*(size + [256, 192, 1][len(size):]))
