"""Nonlocal total variation denoising (Gilboa-Osher) of a noisy striped / textured phantom:

    min_u  lmb/2 |u - f|^2 + sum_p | ( w_m(p) (u[p + d_m] - u[p]) )_m |_2

with K the nonlocal gradient as prost.block.nonlocal_gradient2d(nx, ny, 1, offsets, weights): the device stores the M weight planes, no
matrix.  The weights come from the data (NumPy, here): the noisy image is pre-smoothed by a Gaussian of width SIGMA, the squared
distances of (2 PATCH + 1)^2 patches are taken to every position of the search window of radius --radius, and every pixel keeps the
--keep most similar positions of the window plus its four nearest neighbours, w = exp(-dist / H^2) (FLOOR for a nearest neighbour that was
not among the best); every other weight is zero, which the block treats as no entry.  Stripes repeat inside the window, so a pixel is
tied to pixels of its own stripe, where TV only knows the neighbour across the stripe's edge.  Plain TV (prost.block.gradient2d) runs on
the same data for comparison.  twin=True hands K over as prost.block.sparse of the explicit matrix instead.
usage: python examples/nltv_denoise.py [--size NX NY] [--radius R] [--keep K]"""
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

SIGMA, PATCH, H = 0.6, 2, 0.2
FLOOR = 0.05                       # the weight of a nearest neighbour that is not among the best: it keeps the graph connected
LMB, LMB_TV = 20.0, 40.0
NEAREST = ((0, 1), (0, -1), (1, 0), (-1, 0))


def striped_image(nx, ny, noise=0.1, seed=1):
    """clean: diagonal stripes of period 6 (0.25 / 0.75) left of the middle, a checker texture of period 4 on the right, column-major
    (y fastest); -> clean, clean + noise"""
    x, y = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    stripes = 0.25 + 0.5 * (((x + y) // 3) % 2)
    checker = 0.3 + 0.4 * (((x // 2) + (y // 2)) % 2)
    clean = np.where(x < nx // 2, stripes, checker).astype(np.float64).reshape(-1)
    return clean, clean + noise * np.random.default_rng(seed).standard_normal(clean.size)


def shifted(a, dy, dx):
    """a[x + dx, y + dy] with the border repeated"""
    nx, ny = a.shape
    xs, ys = np.clip(np.arange(nx) + dx, 0, nx - 1), np.clip(np.arange(ny) + dy, 0, ny - 1)
    return a[np.ix_(xs, ys)]


def nonlocal_weights(f, nx, ny, radius=3, keep=6, sigma=SIGMA, patch=PATCH, h=H):
    """-> offsets (the full window, prost.block.nonlocal_window(radius)), weights (M planes of nx ny values, y fastest)"""
    offsets = prost.block.nonlocal_window(radius)
    fs = scipy.ndimage.gaussian_filter(np.asarray(f, dtype=np.float64).reshape(nx, ny), sigma=sigma, mode="nearest")
    size = 2 * patch + 1
    dist = np.stack([scipy.ndimage.uniform_filter((shifted(fs, dy, dx) - fs) ** 2, size=size, mode="nearest") for dy, dx in offsets])
    M = len(offsets)
    order = np.argsort(dist, axis=0, kind="stable")
    best = np.zeros(dist.shape, dtype=bool)
    np.put_along_axis(best, order[:min(keep, M)], True, axis=0)
    w = np.where(best, np.exp(-dist / (h * h)), 0.0)
    for m, (dy, dx) in enumerate(offsets):
        if (int(dy), int(dx)) in NEAREST:
            w[m] = np.where(best[m], w[m], FLOOR)
    return offsets, [w[m].reshape(-1) for m in range(M)]


def spmat_nonlocal_gradient2d(nx, ny, nc, offsets, planes):
    """the explicit K: row (m, c, p) holds -w_m[p] at c N + p and +w_m[p] at c N + p + dy + dx ny where the target lies in the grid"""
    N, M = nx * ny, len(offsets)
    x, y = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    p = np.arange(N)
    rows, cols, vals = [], [], []
    for m, (dy, dx) in enumerate(offsets):
        dy, dx = int(dy), int(dx)
        ok = ((y + dy >= 0) & (y + dy < ny) & (x + dx >= 0) & (x + dx < nx)).reshape(-1)
        here, w = p[ok], np.asarray(planes[m], dtype=np.float64).reshape(-1)[ok]
        for c in range(nc):
            r = (m * nc + c) * N + here
            rows += [r, r]
            cols += [c * N + here, c * N + here + dy + dx * ny]
            vals += [-w, w]
    K = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(M * nc * N, nc * N)).tocsc()
    K.eliminate_zeros()
    return K


def options(tol, max_iters, num_cback_calls=0):
    return prost.options(max_iters=max_iters, num_cback_calls=num_cback_calls, verbose=False, tol_rel_primal=tol, tol_abs_primal=tol, tol_rel_dual=tol,
                         tol_abs_dual=tol)


def describe(nx, ny, radius=3, keep=6, lmb=LMB, tol=1e-5, max_iters=20000, f=None, twin=False, offsets=None, planes=None):
    """-> prob, backend, opts, u, f, clean, offsets, planes.  f: the data (None: striped_image); offsets, planes: the operator (None:
    nonlocal_weights of f); twin: block.sparse of the explicit K"""
    clean = None
    if f is None:
        clean, f = striped_image(nx, ny)
    if planes is None:
        offsets, planes = nonlocal_weights(f, nx, ny, radius, keep)
    M = len(offsets)
    u = prost.variable(nx * ny)
    q = prost.variable(M * nx * ny)
    prob = prost.min_problem([u], [q])
    prob.add_function(u, prost.function.sum_1d("square", 1, f, lmb, 0, 0))
    prob.add_function(q, prost.function.sum_norm2(M, False, "abs", 1, 0, 1, 0, 0))
    prob.add_constraint(u, q, prost.block.sparse(spmat_nonlocal_gradient2d(nx, ny, 1, offsets, planes)) if twin else prost.block.nonlocal_gradient2d(nx, ny, 1, offsets, planes))
    backend = prost.backend.pdhg(stepsize="boyd", residual_iter=1)
    return prob, backend, options(tol, max_iters), u, f, clean, offsets, planes


def describe_tv(nx, ny, f, lmb=LMB_TV, tol=1e-5, max_iters=20000):
    """min_u lmb/2 |u - f|^2 + |grad u|_{2,1} on the same data, for comparison"""
    u = prost.variable(nx * ny)
    q = prost.variable(2 * nx * ny)
    prob = prost.min_problem([u], [q])
    prob.add_function(u, prost.function.sum_1d("square", 1, f, lmb, 0, 0))
    prob.add_function(q, prost.function.sum_norm2(2, False, "abs", 1, 0, 1, 0, 0))
    prob.add_constraint(u, q, prost.block.gradient2d(nx, ny, 1))
    return prob, prost.backend.pdhg(stepsize="boyd", residual_iter=1), options(tol, max_iters), u


def rmse(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, dtype=np.float64).ravel() - np.asarray(b, dtype=np.float64).ravel()) ** 2)))


def main(nx=192, ny=128, radius=3, keep=6, max_iters=20000, verbose=True, twin=False, solve=None):
    """solve: a function (prob, backend, opts) -> result in place of prost.solve"""
    solve = solve or prost.solve
    prob, backend, opts, u, f, clean, offsets, _ = describe(nx, ny, radius, keep, max_iters=max_iters, twin=twin)
    t0 = time.perf_counter()
    result = solve(prob, backend, opts)
    elapsed = time.perf_counter() - t0
    img = np.array(u.val, dtype=np.float64).ravel()
    prob_tv, backend_tv, opts_tv, u_tv = describe_tv(nx, ny, f, max_iters=max_iters)
    result_tv = solve(prob_tv, backend_tv, opts_tv)
    img_tv = np.array(u_tv.val, dtype=np.float64).ravel()
    if verbose:
        print("nonlocal TV (M = %d): %s after %d iterations, %.3f s on %s; RMSE to the clean image %.4f (TV: %.4f after %d iterations, data: %.4f)"
              % (len(offsets), result["result"], result["iters"], elapsed, result.get("path"), rmse(img, clean), rmse(img_tv, clean), result_tv["iters"], rmse(f, clean)))
    return result, img, result_tv, img_tv, f, clean


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--size", type=int, nargs=2, default=[192, 128], metavar=("NX", "NY"))
    ap.add_argument("--radius", type=int, default=3)
    ap.add_argument("--keep", type=int, default=6)
    ap.add_argument("--twin", action="store_true", help="the explicit matrix through prost.block.sparse")
    args = ap.parse_args()
    main(args.size[0], args.size[1], args.radius, args.keep, twin=args.twin)
