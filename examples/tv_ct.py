"""TV-regularised tomographic reconstruction from few parallel-beam projections, the Chambolle-Pock prototype of Sidky, Jorgensen and
Pan: min_u 1/2 |R u - f|^2 + lmb |grad u|_{2,1} subject to u >= 0, in the constrained (primal) form with v = R u and g = grad u as
constrained variables, K = [radon2d ; gradient2d].  R is prost.block.radon2d(size, size, 1, angles): Joseph's projector applied without
a matrix, five numbers per angle.  twin=True builds the same problem with prost.block.sparse of the explicit matrix instead -- what a
user had to hand over before the block existed (about 2 n_angles n_bins size non-zeros).  The phantom is a handful of ellipses generated
here; the data f is its projection through the operator plus a little noise.
usage: python examples/tv_ct.py [--size 128] [--angles 30] [--twin]"""
import argparse
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import scipy.sparse as sp

import prost_amd as prost

# (value, semi-axis a, semi-axis b, centre x, centre y, rotation in degrees) in units of half the image side: a head-like phantom
ELLIPSES = ((1.0, 0.69, 0.92, 0.0, 0.0, 0.0), (-0.8, 0.6624, 0.874, 0.0, -0.0184, 0.0), (-0.2, 0.11, 0.31, 0.22, 0.0, -18.0), (-0.2, 0.16, 0.41, -0.22, 0.0, 18.0),
            (0.1, 0.21, 0.25, 0.0, 0.35, 0.0), (0.1, 0.046, 0.046, 0.0, 0.1, 0.0), (0.1, 0.046, 0.046, 0.0, -0.1, 0.0), (0.1, 0.046, 0.023, -0.08, -0.605, 0.0),
            (0.1, 0.023, 0.023, 0.0, -0.606, 0.0), (0.1, 0.023, 0.046, 0.06, -0.605, 0.0))


def phantom(nx, ny):
    """the sum of the ellipses, column-major: element (y, x) at y + x ny"""
    y, x = np.mgrid[0:ny, 0:nx].astype(np.float64)
    X, Y = (x - (nx - 1) / 2.0) / (nx / 2.0), -(y - (ny - 1) / 2.0) / (ny / 2.0)
    img = np.zeros((ny, nx))
    for value, a, b, x0, y0, deg in ELLIPSES:
        co, si = math.cos(math.radians(deg)), math.sin(math.radians(deg))
        u, v = (X - x0) * co + (Y - y0) * si, -(X - x0) * si + (Y - y0) * co
        img[(u / a) ** 2 + (v / b) ** 2 <= 1.0] += value
    return np.maximum(img, 0.0).T.reshape(-1)


def explicit_matrix(nx, ny, angles, ndet, spacing=1.0, shift=0.0, dtype=np.float64):
    """the matrix of prost.block.radon2d(nx, ny, 1, angles, ndet, spacing, shift) in the arithmetic of `dtype`, as a scipy CSC: per angle
    the table { q, p, r, c } and the driving axis, the position f = (r + q d) + p t of ray d on driving line t, and the two entries
    c (1 - (f - floor f)) and c (f - floor f) at the interpolated indices floor f and floor f + 1"""
    dtype = np.dtype(dtype)
    T = dtype.type
    cx, cy, cd, h = (nx - 1) / 2.0, (ny - 1) / 2.0, (ndet - 1) / 2.0, float(spacing)
    rows, cols, vals = [], [], []
    d = np.arange(ndet)
    for a, theta in enumerate(np.asarray(angles, dtype=np.float64).ravel()):
        co, si = math.cos(float(theta)), math.sin(float(theta))
        column = abs(co) < abs(si)
        if not column:
            q, p, r, c = T(h / co), T(-si / co), T(((shift - cd * h) + cy * si) / co + cx), T(1 / abs(co))
        else:
            q, p, r, c = T(h / si), T(-co / si), T(((shift - cd * h) + cx * co) / si + cy), T(1 / abs(si))
        nt, ni = (nx, ny) if column else (ny, nx)
        t = np.arange(nt)
        f = (r + q * d.astype(dtype))[:, None] + (p * t.astype(dtype))[None, :]
        fl = np.floor(f)
        w1 = f - fl
        i0 = np.where((fl >= -1) & (fl < ni), fl, -2).astype(np.int64)
        for i, w in ((i0, T(1) - w1), (i0 + 1, w1)):
            keep = (i0 >= -1) & (i >= 0) & (i < ni) & (w != 0)
            dd, tt = np.nonzero(keep)
            rows.append(a * ndet + dd)
            cols.append(i[keep] + tt * ny if column else tt + i[keep] * ny)
            vals.append((c * w)[keep].astype(np.float64))
    return sp.csc_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(len(angles) * ndet, nx * ny))


def rmse(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, dtype=np.float64).ravel() - np.asarray(b, dtype=np.float64).ravel()) ** 2)))


def describe(size=128, n_angles=30, lmb=0.05, tol=1e-4, max_iters=5000, num_cback_calls=50, twin=False, sinogram=None, dtype=np.float64, noise=0.002):
    """sinogram: the data (a caller that compares the block with its twin hands one problem's data to the other); None: the phantom
    sent through the operator -- the block itself (twin: the matrix) -- plus noise of standard deviation `noise` times the largest
    projection.  dtype: the arithmetic the twin's matrix is formed in (that of the precision the problem is solved in)."""
    nx = ny = int(size)
    angles = np.arange(int(n_angles)) * (math.pi / int(n_angles))
    ndet = prost.block.radon2d_ndet(nx, ny, 1.0)
    truth = phantom(nx, ny)
    if twin:
        K = explicit_matrix(nx, ny, angles, ndet, dtype=dtype)
        op = prost.block.sparse(K)
    else:
        op = prost.block.radon2d(nx, ny, 1, angles, ndet)
    if sinogram is None:
        if twin:
            clean = K @ truth
        else:
            clean = np.asarray(prost.eval_linop([op(0, 0, 0, 0)[0]], truth, False)[0], dtype=np.float64).ravel()
        sinogram = clean + noise * float(np.abs(clean).max()) * np.random.default_rng(7).standard_normal(clean.size)
    u = prost.variable(nx * ny)
    v = prost.variable(len(angles) * ndet)
    g = prost.variable(2 * nx * ny)
    prob = prost.min_problem([u], [v, g])
    prob.add_function(u, prost.function.sum_1d("ind_geq0"))
    prob.add_function(v, prost.function.sum_1d("square", 1, sinogram, 1, 0, 0))
    prob.add_function(g, prost.function.sum_norm2(2, False, "abs", 1, 0, lmb, 0, 0))
    prob.add_constraint(u, v, op)
    prob.add_constraint(u, g, prost.block.gradient2d(nx, ny, 1))
    backend = prost.backend.pdhg(stepsize="boyd", residual_iter=1)
    opts = prost.options(max_iters=max_iters, num_cback_calls=num_cback_calls, verbose=False, tol_rel_primal=tol, tol_abs_primal=tol,
                         tol_rel_dual=tol, tol_abs_dual=tol)
    return prob, backend, opts, u, truth, sinogram


def main(size=128, n_angles=30, max_iters=5000, verbose=True, twin=False, lmb=0.05):
    prob, backend, opts, u, truth, sinogram = describe(size, n_angles, lmb=lmb, max_iters=max_iters, twin=twin)
    t0 = time.perf_counter()
    result = prost.solve(prob, backend, opts)
    elapsed = time.perf_counter() - t0
    img = np.asarray(u.val)
    if verbose:
        print("%d x %d from %d angles: %s after %d iterations, %.3f s on %s; RMSE to the phantom %.4f, of the phantom's own mean image %.4f"
              % (size, size, n_angles, result["result"], result["iters"], elapsed, result["path"], rmse(img, truth), rmse(np.full(truth.size, truth.mean()), truth)))
    return result, img, truth, sinogram


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=128, help="the image is size x size")
    ap.add_argument("--angles", type=int, default=30, help="projections, evenly over [0, pi)")
    ap.add_argument("--twin", action="store_true", help="the sparse matrix instead of the block")
    a = ap.parse_args()
    main(a.size, a.angles, twin=a.twin)
