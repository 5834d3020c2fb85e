"""TV-regularised reconstruction of an image from scattered samples: M noisy bilinear samples of the image at random sub-pixel positions,
min_u 1/2 |S u - f|^2 + lmb |grad u|_{2,1}, in the constrained (primal) form with v = S u and g = grad u as constrained variables,
K = [sample2d ; gradient2d].  S is prost.block.sample2d(size, size, 1, x, y): bilinear resampling applied without a matrix, two
coordinates per sample.  twin=True builds the same problem with prost.block.sparse of the explicit matrix instead -- what a user had to
hand over before the block existed (four non-zeros per sample, held twice on the device).  The phantom is that of tv_ct.py; the data f
is its samples through the operator plus a little noise.  The default is two samples per pixel; with fewer samples than pixels the
total variation fills the gaps, at the price of the phantom's thin structures.
usage: python examples/tv_scattered.py [--size 128] [--samples 32768] [--twin]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import scipy.sparse as sp

import prost_amd as prost
from tv_ct import phantom, rmse


def sample_positions(nx, ny, samples, seed=11):
    """M positions uniform over the pixel centres' hull [0, nx - 1] x [0, ny - 1]"""
    rng = np.random.default_rng(seed)
    return rng.uniform(0.0, nx - 1.0, int(samples)), rng.uniform(0.0, ny - 1.0, int(samples))


def explicit_matrix(nx, ny, x, y, dtype=np.float64):
    """the matrix of prost.block.sample2d(nx, ny, 1, x, y) in the arithmetic of `dtype`, as a scipy CSC: the positions rounded once,
    j0 = floor(fx), ax = fx - j0, bx = 1 - ax and likewise i0, ay, by; by bx at (i0, j0), ay bx at (i0 + 1, j0), by ax at (i0, j0 + 1),
    ay ax at (i0 + 1, j0 + 1); an entry outside the image or with a weight of exactly 0 is absent"""
    dtype = np.dtype(dtype)
    T = dtype.type
    fx, fy = np.asarray(x, np.float64).astype(dtype), np.asarray(y, np.float64).astype(dtype)
    reach = (fx >= T(-1)) & (fx < T(nx)) & (fy >= T(-1)) & (fy < T(ny))
    fx, fy = np.where(reach, fx, T(0)), np.where(reach, fy, T(0))
    j0, i0 = np.floor(fx), np.floor(fy)
    ax, ay = fx - j0, fy - i0
    bx, by = T(1) - ax, T(1) - ay
    j0, i0 = j0.astype(np.int64), i0.astype(np.int64)
    rows, cols, vals = [], [], []
    for ii, jj, w in ((i0, j0, by * bx), (i0 + 1, j0, ay * bx), (i0, j0 + 1, by * ax), (i0 + 1, j0 + 1, ay * ax)):
        keep = reach & (ii >= 0) & (ii < ny) & (jj >= 0) & (jj < nx) & (w != 0)
        rows.append(np.nonzero(keep)[0])
        cols.append((ii + jj * ny)[keep])
        vals.append(w[keep].astype(np.float64))
    return sp.csc_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(len(fx), nx * ny))


def describe(size=128, samples=32768, lmb=0.005, tol=1e-4, max_iters=5000, num_cback_calls=50, twin=False, data=None, dtype=np.float64, noise=0.01):
    """data: the samples f (a caller that compares the block with its twin hands one problem's data to the other); None: the phantom
    sent through the operator -- the block itself (twin: the matrix) -- plus noise of standard deviation `noise`.  dtype: the arithmetic
    the twin's matrix is formed in (that of the precision the problem is solved in)."""
    nx = ny = int(size)
    x, y = sample_positions(nx, ny, samples)
    truth = phantom(nx, ny)
    if twin:
        K = explicit_matrix(nx, ny, x, y, dtype=dtype)
        op = prost.block.sparse(K)
    else:
        op = prost.block.sample2d(nx, ny, 1, x, y)
    if data is None:
        if twin:
            clean = K @ truth
        else:
            clean = np.asarray(prost.eval_linop([op(0, 0, 0, 0)[0]], truth, False)[0], dtype=np.float64).ravel()
        data = clean + noise * np.random.default_rng(7).standard_normal(clean.size)
    u = prost.variable(nx * ny)
    v = prost.variable(len(x))
    g = prost.variable(2 * nx * ny)
    prob = prost.min_problem([u], [v, g])
    prob.add_function(v, prost.function.sum_1d("square", 1, data, 1, 0, 0))
    prob.add_function(g, prost.function.sum_norm2(2, False, "abs", 1, 0, lmb, 0, 0))
    prob.add_constraint(u, v, op)
    prob.add_constraint(u, g, prost.block.gradient2d(nx, ny, 1))
    backend = prost.backend.pdhg(stepsize="boyd", residual_iter=1)
    opts = prost.options(max_iters=max_iters, num_cback_calls=num_cback_calls, verbose=False, tol_rel_primal=tol, tol_abs_primal=tol,
                         tol_rel_dual=tol, tol_abs_dual=tol)
    return prob, backend, opts, u, truth, data


def main(size=128, samples=32768, max_iters=5000, verbose=True, twin=False, lmb=0.005):
    prob, backend, opts, u, truth, data = describe(size, samples, lmb=lmb, max_iters=max_iters, twin=twin)
    t0 = time.perf_counter()
    result = prost.solve(prob, backend, opts)
    elapsed = time.perf_counter() - t0
    img = np.asarray(u.val)
    if verbose:
        print("%d x %d from %d samples: %s after %d iterations, %.3f s on %s; RMSE to the phantom %.4f, of the phantom's own mean image %.4f"
              % (size, size, samples, result["result"], result["iters"], elapsed, result["path"], rmse(img, truth), rmse(np.full(truth.size, truth.mean()), truth)))
    return result, img, truth, data


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=128, help="the image is size x size")
    ap.add_argument("--samples", type=int, default=32768, help="bilinear samples at random sub-pixel positions")
    ap.add_argument("--twin", action="store_true", help="the sparse matrix instead of the block")
    a = ap.parse_args()
    main(a.size, a.samples, twin=a.twin)
