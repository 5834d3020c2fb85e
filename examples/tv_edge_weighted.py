"""Edge-weighted and anisotropic total variation denoising of a noisy piecewise-constant image:

    min_u  lmb/2 |u - f|^2 + | T grad u |_{2,1}

with K = T grad as prost.block.tensor_gradient2d(nx, ny, nc, tensor): the device stores the tensor field, no matrix.  The weights come
from the data, pre-smoothed by a Gaussian of width sigma, f_s = G_sigma * f:

    --mode scalar:  T = g I,  g = exp(-beta |grad f_s|^gamma)             (edge-weighted TV: edges of the data are cheap)
    --mode tensor:  T = D^(1/2) = g n n^T + n_perp n_perp^T,  n = grad f_s / |grad f_s|
                    (the image-driven diffusion tensor of anisotropic Huber-L1 / TGV: only the jump ACROSS an edge is cheap)

Plain TV (T = I, prost.block.gradient2d) runs on the same data for comparison: where the weight is small the jump keeps its height,
so the weighted problems can be regularised harder in the flat regions (lmb = 3 against 8 for TV in the scalar mode).  twin=True hands K over as prost.block.sparse of the explicit
matrix T G instead.  usage: python examples/tv_edge_weighted.py [--size NX NY] [--mode scalar|tensor] [--channels NC]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import scipy.ndimage
import scipy.sparse as sp

import prost_amd as prost
from multilabel_fast import spmat_gradient2d

BETA, GAMMA, SIGMA = 12.0, 1.0, 1.0
LMB = {"scalar": 3.0, "tensor": 8.0}
LMB_TV = 8.0


def step_image(nx, ny, nc=1, noise=0.1, seed=1):
    """clean: 0.2, a disc of 0.8 left of the middle and a bar of 0.5 on the right, the same in every channel, column-major (y fastest);
    -> clean, clean + noise"""
    x, y = np.meshgrid(np.arange(nx, dtype=np.float64), np.arange(ny, dtype=np.float64), indexing="ij")
    disc = (x - 0.35 * nx) ** 2 + (y - 0.5 * ny) ** 2 < (0.3 * min(nx, ny)) ** 2
    bar = (x > 0.7 * nx) & (x < 0.88 * nx) & (y > 0.2 * ny) & (y < 0.8 * ny)
    clean = np.tile((0.2 + 0.6 * disc + 0.3 * bar).reshape(-1), nc)
    return clean, clean + noise * np.random.default_rng(seed).standard_normal(clean.size)


def edge_tensor(f, nx, ny, nc=1, mode="scalar", beta=BETA, gamma=GAMMA, sigma=SIGMA):
    """the planes of the tensor from the data: [g] (scalar) or [a, b, c] (tensor), each of nx ny values with y fastest.  The gradient
    of the smoothed data is a central difference, averaged over the channels."""
    fs = scipy.ndimage.gaussian_filter(np.asarray(f, dtype=np.float64).reshape(nc, nx, ny), sigma=(0, sigma, sigma), mode="nearest").mean(axis=0)
    dx, dy = np.gradient(fs) if min(nx, ny) > 1 else (np.zeros_like(fs), np.zeros_like(fs))
    mag = np.sqrt(dx * dx + dy * dy)
    g = np.exp(-beta * mag ** gamma)
    if mode == "scalar":
        return [g.reshape(-1)]
    if mode != "tensor":
        raise ValueError("mode %r is not scalar or tensor" % (mode,))
    flat = mag < 1e-12                                  # no direction: T = I there (g is 1 as well)
    n_x, n_y = np.where(flat, 1.0, dx / np.where(flat, 1.0, mag)), np.where(flat, 0.0, dy / np.where(flat, 1.0, mag))
    g = np.where(flat, 1.0, g)
    a, b, c = g * n_x * n_x + n_y * n_y, (g - 1.0) * n_x * n_y, g * n_y * n_y + n_x * n_x
    return [a.reshape(-1), b.reshape(-1), c.reshape(-1)]


def spmat_tensor_gradient2d(nx, ny, nc, planes):
    """the explicit K = T G: G = spmat_gradient2d(nx, ny, nc) without its stored zeros, T = [[diag(a), diag(b)], [diag(b), diag(c)]]
    repeated for every channel"""
    N = nx * ny
    G = sp.csr_matrix(spmat_gradient2d(nx, ny, nc))
    G.eliminate_zeros()
    a, b, c = (planes[0], None, planes[0]) if len(planes) == 1 else ((planes[0], None, planes[1]) if len(planes) == 2 else planes)
    rep = lambda v: sp.diags(np.tile(np.asarray(v, dtype=np.float64), nc))
    B = rep(b) if b is not None else sp.csr_matrix((nc * N, nc * N))
    return (sp.bmat([[rep(a), B], [B, rep(c)]], format="csr") @ G).tocsc()


def options(tol, max_iters, num_cback_calls=0):
    return prost.options(max_iters=max_iters, num_cback_calls=num_cback_calls, verbose=False, tol_rel_primal=tol, tol_abs_primal=tol, tol_rel_dual=tol,
                         tol_abs_dual=tol)


def describe(nx, ny, nc=1, mode="scalar", lmb=None, tol=1e-5, max_iters=20000, f=None, twin=False, planes=None):
    """-> prob, backend, opts, u, f, clean, planes.  f: the data (None: step_image); planes: the tensor (None: edge_tensor of f);
    twin: block.sparse of the explicit K"""
    clean = None
    lmb = LMB[mode] if lmb is None else lmb
    if f is None:
        clean, f = step_image(nx, ny, nc)
    if planes is None:
        planes = edge_tensor(f, nx, ny, nc, mode)
    u = prost.variable(nc * nx * ny)
    q = prost.variable(2 * nc * nx * ny)
    prob = prost.min_problem([u], [q])
    prob.add_function(u, prost.function.sum_1d("square", 1, f, lmb, 0, 0))
    prob.add_function(q, prost.function.sum_norm2(2 * nc, False, "abs", 1, 0, 1, 0, 0))
    prob.add_constraint(u, q, prost.block.sparse(spmat_tensor_gradient2d(nx, ny, nc, planes)) if twin else prost.block.tensor_gradient2d(nx, ny, nc, planes))
    backend = prost.backend.pdhg(stepsize="boyd", residual_iter=1)
    return prob, backend, options(tol, max_iters), u, f, clean, planes


def describe_tv(nx, ny, nc, f, lmb=LMB_TV, tol=1e-5, max_iters=20000):
    """min_u lmb/2 |u - f|^2 + |grad u|_{2,1} on the same data, for comparison"""
    u = prost.variable(nc * nx * ny)
    q = prost.variable(2 * nc * nx * ny)
    prob = prost.min_problem([u], [q])
    prob.add_function(u, prost.function.sum_1d("square", 1, f, lmb, 0, 0))
    prob.add_function(q, prost.function.sum_norm2(2 * nc, False, "abs", 1, 0, 1, 0, 0))
    prob.add_constraint(u, q, prost.block.gradient2d(nx, ny, nc))
    return prob, prost.backend.pdhg(stepsize="boyd", residual_iter=1), options(tol, max_iters), u


def rmse(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, dtype=np.float64).ravel() - np.asarray(b, dtype=np.float64).ravel()) ** 2)))


def main(nx=256, ny=192, nc=1, mode="scalar", max_iters=20000, verbose=True, twin=False, solve=None):
    """solve: a function (prob, backend, opts) -> result in place of prost.solve"""
    solve = solve or prost.solve
    prob, backend, opts, u, f, clean, _ = describe(nx, ny, nc, mode, max_iters=max_iters, twin=twin)
    t0 = time.perf_counter()
    result = solve(prob, backend, opts)
    elapsed = time.perf_counter() - t0
    img = np.array(u.val, dtype=np.float64).ravel()
    prob_tv, backend_tv, opts_tv, u_tv = describe_tv(nx, ny, nc, f, max_iters=max_iters)
    result_tv = solve(prob_tv, backend_tv, opts_tv)
    img_tv = np.array(u_tv.val, dtype=np.float64).ravel()
    if verbose:
        print("%s-weighted TV: %s after %d iterations, %.3f s on %s; RMSE to the clean image %.4f (TV: %.4f after %d iterations, data: %.4f)"
              % (mode, result["result"], result["iters"], elapsed, result.get("path"), rmse(img, clean), rmse(img_tv, clean), result_tv["iters"], rmse(f, clean)))
    return result, img, result_tv, img_tv, f, clean


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--size", type=int, nargs=2, default=[256, 192], metavar=("NX", "NY"))
    ap.add_argument("--mode", choices=["scalar", "tensor"], default="scalar")
    ap.add_argument("--channels", type=int, default=1)
    ap.add_argument("--twin", action="store_true", help="the explicit matrix through prost.block.sparse")
    args = ap.parse_args()
    main(args.size[0], args.size[1], args.channels, args.mode, twin=args.twin)
