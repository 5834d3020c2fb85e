"""TV super-resolution of one low-resolution colour image with the blur-and-decimate operator as a matrix-free block:
min_u |grad u|_{2,1} + lmb/2 |S B u - f|^2 in the constrained (primal) form of deblurring_conv2d.py, with v = S B u and g = grad u
as constrained variables.  B blurs with a (2 factor + 1)^2 Gaussian window, S keeps every factor-th pixel in both axes; K = S B is
prost.block.conv2d_strided(nx, ny, nc, window, factor, "same"): one small window and four integers, no matrix.  twin=True builds the
same problem with prost.block.sparse of the explicit matrix S @ kron(eye(nc), convmtx2(window)) instead -- what a user had to hand
over before the block existed.  The low-resolution data f is the synthetic ground truth sent through the operator plus a little noise.
usage: python examples/superresolution.py [nx ny nc] [--factor 2|3|4]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import scipy.sparse as sp

import prost_amd as prost
from deblurring import convmtx2
from multilabel_fast import spmat_gradient2d


def gauss_window(factor):
    """a normalised (2 factor + 1)^2 Gaussian with sigma = factor / 2: the anti-aliasing blur of a camera that bins factor^2 pixels"""
    size, sigma = 2 * factor + 1, 0.5 * factor
    yy, xx = np.mgrid[0:size, 0:size].astype(np.float64) - factor
    k = np.exp(-(xx * xx + yy * yy) / (2.0 * sigma * sigma))
    return k / k.sum()


def ground_truth(nx, ny, nc):
    """piecewise constant blocks on a smooth ramp, in [0, 1]: column-major, element (y, x, c) at y + x ny + c nx ny"""
    bs = max(2, max(nx, ny) // 4)
    y, x = np.mgrid[0:ny, 0:nx]
    out = np.empty((nc, nx, ny))
    for c in range(nc):
        blocks = (((y + c * bs // 2) // bs + x // bs) % 2).astype(np.float64)
        out[c] = (0.2 + 0.5 * blocks + 0.2 * (x + y) / float(nx + ny)).T
    return out.reshape(-1)


def low_size(nx, ny, factor):
    """(my, mx) of one low-resolution plane"""
    return (ny - 1) // factor + 1, (nx - 1) // factor + 1


def explicit_matrix(nx, ny, nc, k, factor):
    """S @ kron(eye(nc), convmtx2(k, ny, nx)) for the "same" crop: the rows (y factor + ky // 2, x factor + kx // 2) of the full convolution"""
    ky, kx = k.shape
    my, mx = low_size(nx, ny, factor)
    y, x = np.mgrid[0:my, 0:mx]
    rows = ((y * factor + ky // 2) + (x * factor + kx // 2) * (ny + ky - 1)).T.reshape(-1)
    one = convmtx2(k, ny, nx).tocsr()[rows]
    K = sp.kron(sp.identity(nc), one, format="csc")
    K.eliminate_zeros()
    return K


def nearest(f_low, nx, ny, nc, factor):
    """nearest-neighbour upsampling of the low-resolution image: the baseline a solve has to beat"""
    my, mx = low_size(nx, ny, factor)
    low = np.asarray(f_low, dtype=np.float64).reshape(nc, mx, my)
    y, x = np.minimum((np.arange(ny) + factor // 2) // factor, my - 1), np.minimum((np.arange(nx) + factor // 2) // factor, mx - 1)
    return low[:, x][:, :, y].reshape(-1)


def rmse(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, dtype=np.float64).ravel() - np.asarray(b, dtype=np.float64).ravel()) ** 2)))


def describe(nx, ny, nc, factor=2, lmb=2000.0, tol=1e-4, max_iters=25000, num_cback_calls=250, twin=False, f_low=None):
    """f_low: the data (a caller that compares the block with its twin hands one problem's data to the other); None: the ground truth
    sent through the operator -- the block itself (twin: the matrix) -- plus noise of standard deviation 0.01"""
    truth = ground_truth(nx, ny, nc)
    grad = spmat_gradient2d(nx, ny, nc)
    k = gauss_window(factor)
    my, mx = low_size(nx, ny, factor)
    if twin:
        K = explicit_matrix(nx, ny, nc, k, factor)
        op = prost.block.sparse(K)
    else:
        op = prost.block.conv2d_strided(nx, ny, nc, k, factor, "same")
    if f_low is None:
        if twin:
            clean = K @ truth
        else:
            clean = np.asarray(prost.eval_linop([op(0, 0, 0, 0)[0]], truth, False)[0], dtype=np.float64).ravel()
        f_low = clean + 0.01 * np.random.default_rng(7).standard_normal(my * mx * nc)
    u = prost.variable(nx * ny * nc)
    v = prost.variable(my * mx * nc)
    g = prost.variable(2 * nx * ny * nc)
    prob = prost.min_problem([u], [v, g])
    prob.add_function(v, prost.function.sum_1d("square", 1, f_low, lmb, 0, 0))
    prob.add_function(g, prost.function.sum_norm2(2 * nc, False, "abs", 1, 0, 1, 0, 0))
    prob.add_constraint(u, v, op)
    prob.add_constraint(u, g, prost.block.sparse(grad))
    backend = prost.backend.pdhg(stepsize="boyd", residual_iter=1)
    opts = prost.options(max_iters=max_iters, num_cback_calls=num_cback_calls, verbose=False, tol_rel_primal=tol, tol_abs_primal=tol,
                         tol_rel_dual=tol, tol_abs_dual=tol)
    return prob, backend, opts, u, truth, f_low


def main(nx=256, ny=192, nc=3, factor=2, max_iters=25000, verbose=True, twin=False, lmb=2000.0):
    prob, backend, opts, u, truth, f_low = describe(nx, ny, nc, factor, lmb=lmb, max_iters=max_iters, twin=twin)
    t0 = time.perf_counter()
    result = prost.solve(prob, backend, opts)
    elapsed = time.perf_counter() - t0
    img = np.asarray(u.val)
    if verbose:
        print("factor %d: %s after %d iterations, %.3f s on %s; RMSE to the ground truth %.4f, nearest-neighbour upsampling %.4f"
              % (factor, result["result"], result["iters"], elapsed, result["path"], rmse(img, truth), rmse(nearest(f_low, nx, ny, nc, factor), truth)))
    return result, img, truth, f_low


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("size", nargs="*", type=int, default=[256, 192, 3], help="nx ny nc")
    ap.add_argument("--factor", type=int, choices=(2, 3, 4), default=2)
    ap.add_argument("--twin", action="store_true", help="the sparse matrix instead of the block")
    a = ap.parse_args()
    main(*(a.size + [256, 192, 3][len(a.size):])[:3], factor=a.factor, twin=a.twin)
