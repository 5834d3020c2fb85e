"""examples/deblurring.py with the blur operator as a matrix-free block: TV deblurring in the constrained (primal) form --
min_u lmb/2 |B u - f_blurred|^2 + |grad u|_{2,1} with v = B u and g = grad u as constrained variables -- where B is
prost.block.conv2d(nx, ny, nc, kernel, "full") instead of the sparse matrix kron(speye(nc), convmtx2(kernel, ny, nx)).  The block stores
the window's non-zero taps and nothing per pixel, so a dense window costs no set-up: --kernel gauss blurs with a 15 x 15 Gaussian (225
taps), --kernel motion with the 15 x 15 motion window of deblurring.py (about 29 taps).  The data is blurred with the block itself,
through prost.eval_linop.  usage: python examples/deblurring_conv2d.py [nx ny nc] [--kernel motion|gauss]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np

import prost_amd as prost
from deblurring import motion_kernel
from multilabel_fast import spmat_gradient2d
from prost_amd import synthetic


def gauss_kernel(size=15, sigma=2.5):
    """fspecial('gaussian', size, sigma): a normalised, dense Gaussian window"""
    r = (size - 1) / 2.0
    yy, xx = np.mgrid[0:size, 0:size].astype(np.float64) - r
    k = np.exp(-(xx * xx + yy * yy) / (2.0 * sigma * sigma))
    return k / k.sum()


def window(name):
    if name == "motion":
        return motion_kernel(15, 45.0)
    if name == "gauss":
        return gauss_kernel(15, 2.5)
    raise ValueError("kernel %r: motion or gauss" % (name,))


def blur(nx, ny, nc, k, f):
    """B f with the block itself -> (ny + ky - 1)(nx + kx - 1) nc values"""
    B = prost.block.conv2d(nx, ny, nc, k, "full")(0, 0, 0, 0)[0]
    return np.asarray(prost.eval_linop([B], f, False)[0], dtype=np.float64).ravel()


def describe(nx, ny, nc, kernel="motion", lmb=100.0, tol=1e-4, max_iters=25000, num_cback_calls=250, seed=9, f_blurred=None):
    """f_blurred: data to deblur (a caller that compares with deblurring.describe hands that example's data over); None: f blurred with
    the block plus the noise of deblurring.describe"""
    f = synthetic.rof_image(nx, ny, nc, seed).astype(np.float64)
    grad = spmat_gradient2d(nx, ny, nc)
    k = window(kernel)
    ky, kx = k.shape
    nx2, ny2 = nx + kx - 1, ny + ky - 1
    blurred = None
    if f_blurred is None:
        blurred = blur(nx, ny, nc, k, f)
        f_blurred = blurred + 0.05 * np.random.default_rng(7).standard_normal(ny2 * nx2 * nc)
    u = prost.variable(nx * ny * nc)
    v = prost.variable(nx2 * ny2 * nc)
    g = prost.variable(2 * nx * ny * nc)
    prob = prost.min_problem([u], [v, g])
    prob.add_function(v, prost.function.sum_1d("square", 1, f_blurred, lmb, 0, 0))
    prob.add_function(g, prost.function.sum_norm2(2 * nc, False, "abs", 1, 0, 1, 0, 0))
    prob.add_constraint(u, v, prost.block.conv2d(nx, ny, nc, k, "full"))
    prob.add_constraint(u, g, prost.block.sparse(grad))
    backend = prost.backend.pdhg(stepsize="boyd", residual_iter=1)
    opts = prost.options(max_iters=max_iters, num_cback_calls=num_cback_calls, verbose=False, tol_rel_primal=tol, tol_abs_primal=tol,
                         tol_rel_dual=tol, tol_abs_dual=tol)
    return prob, backend, opts, u, f, f_blurred, blurred


def main(nx=256, ny=192, nc=3, kernel="motion", max_iters=25000, verbose=True):
    prob, backend, opts, u, f, _, blurred = describe(nx, ny, nc, kernel, max_iters=max_iters)
    t0 = time.perf_counter()
    result = prost.solve(prob, backend, opts)
    elapsed = time.perf_counter() - t0
    img = np.asarray(u.val)
    if verbose:
        print("%s window: %s after %d iterations, %.3f s on %s; |u - f| mean %.4f" % (kernel, result["result"], result["iters"], elapsed, result["path"], np.abs(img - f).mean()))
    return result, img, f, blurred


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("size", nargs="*", type=int, default=[256, 192, 3], help="nx ny nc")
    ap.add_argument("--kernel", choices=("motion", "gauss"), default="motion")
    a = ap.parse_args()
    main(*(a.size + [256, 192, 3][len(a.size):])[:3], kernel=a.kernel)
