"""Second-order regularised denoising with the Hessian H u = (u_xx, u_yy, u_xy) as the linear operator, prost.block.hessian2d:

    mode "tv2":      min_u  lmb/2 |u - f|^2 + a |H u|_{2,1}    second-order total variation (bounded Hessian, Bergounioux / Piffet,
                                                               Papafitsoros / Schoenlieb): sum_norm2(3, ..) behind hessian2d(nx, ny,
                                                               nc), whose default w = sqrt(1/2) makes the 2-norm of (hxx, hyy, hxy)
                                                               the Frobenius norm of the Hessian
    mode "nuclear":  min_u  lmb/2 |u - f|^2 + a |H u|_{S1,1}   the Hessian-Schatten norm of order 1 (Lefkimmiatis / Ward / Unser):
                                                               sum_eigen_2x2(False, "abs", ..) behind hessian2d(nx, ny, nc, 0.5,
                                                               components=4), the true Hessian as a column-major 2 x 2 matrix

with z = H u as the constrained variable.  Nothing is stored per pixel and no auxiliary field is introduced (TGV^2, the sister model
of examples/tgv2_denoise.py, needs one).  Both priors have the affine functions in their null space: on a continuous piecewise-affine
image -- a roof, no jumps -- they do not staircase, where TV on the same data does.  twin=True hands H over as prost.block.sparse of
the explicit matrix instead.  usage: python examples/hessian_denoise.py [nx ny nc mode]"""
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
from tgv2_denoise import describe_tv, options, rmse, spmat_sym_gradient2d

MODES = {"tv2": (3, math.sqrt(0.5)), "nuclear": (4, 0.5)}       # components, w


def roof_image(nx, ny, nc=1, noise=0.05, seed=1):
    """clean = 0.04 min(x, nx - 1 - x) + 0.02 y, a ridge along the middle column and no jump, the same in every channel, column-major
    (y fastest), and clean + noise"""
    x, y = np.meshgrid(np.arange(nx, dtype=np.float64), np.arange(ny, dtype=np.float64), indexing="ij")
    clean = np.tile((0.04 * np.minimum(x, nx - 1 - x) + 0.02 * y).reshape(-1), nc)
    return clean, clean + noise * np.random.default_rng(seed).standard_normal(clean.size)


def spmat_hessian2d(nx, ny, nc=1, w=math.sqrt(0.5), components=3):
    """the explicit H = E grad, E of tgv2_denoise.spmat_sym_gradient2d; components = 4: the planes (hxx, hxy, hxy, hyy)"""
    n = nc * nx * ny
    H = sp.csr_matrix(spmat_sym_gradient2d(nx, ny, nc, w) @ spmat_gradient2d(nx, ny, nc))
    planes = (0, 1, 2) if components == 3 else (0, 2, 2, 1)
    H = sp.vstack([H[k * n:(k + 1) * n] for k in planes], format="csc")
    H.eliminate_zeros()
    return H


def describe(nx, ny, nc=1, mode="tv2", lmb=8.0, a=1.0, tol=1e-5, max_iters=20000, f=None, twin=False):
    """-> prob, backend, opts, u, f, clean.  f: the data (None: roof_image); twin: block.sparse of the explicit H"""
    components, w = MODES[mode]
    n = nc * nx * ny
    clean = None
    if f is None:
        clean, f = roof_image(nx, ny, nc)
    u = prost.variable(n)
    z = prost.variable(components * n)
    prob = prost.min_problem([u], [z])
    prob.add_function(u, prost.function.sum_1d("square", 1, f, lmb, 0, 0))
    if mode == "tv2":
        prob.add_function(z, prost.function.sum_norm2(3, False, "abs", 1, 0, a, 0, 0))
    else:
        prob.add_function(z, prost.function.sum_eigen_2x2(False, "abs", 1, 0, a, 0, 0))
    prob.add_constraint(u, z, prost.block.sparse(spmat_hessian2d(nx, ny, nc, w, components)) if twin else prost.block.hessian2d(nx, ny, nc, w, components))
    backend = prost.backend.pdhg(stepsize="boyd", residual_iter=1)
    return prob, backend, options(tol, max_iters), u, f, clean


def main(nx=256, ny=192, nc=1, mode="tv2", max_iters=20000, verbose=True, twin=False):
    prob, backend, opts, u, f, clean = describe(nx, ny, nc, mode, max_iters=max_iters, twin=twin)
    t0 = time.perf_counter()
    result = prost.solve(prob, backend, opts)
    elapsed = time.perf_counter() - t0
    img = np.array(u.val, dtype=np.float64).ravel()
    prob_tv, backend_tv, opts_tv, u_tv = describe_tv(nx, ny, nc, f, max_iters=max_iters)
    result_tv = prost.solve(prob_tv, backend_tv, opts_tv)
    img_tv = np.array(u_tv.val, dtype=np.float64).ravel()
    if verbose:
        print("%s: %s after %d iterations, %.3f s on %s; RMSE to the clean image %.4f (TV: %.4f after %d iterations, data: %.4f)"
              % (mode, result["result"], result["iters"], elapsed, result["path"], rmse(img, clean), rmse(img_tv, clean), result_tv["iters"], rmse(f, clean)))
    return result, img, result_tv, img_tv, f, clean


if __name__ == "__main__":
    size = [int(a) for a in sys.argv[1:4]]
    main(*(size + [256, 192, 1][len(size):]), mode=sys.argv[4] if len(sys.argv) > 4 else "tv2")
