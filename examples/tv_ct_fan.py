"""TV-regularised tomographic reconstruction from few fan-beam projections: the problem of examples/tv_ct.py with the geometry of a CT
scanner, a point source on a circle of radius R around the image and a flat or an equiangular detector.
min_u 1/2 |K u - f|^2 + lmb |grad u|_{2,1} subject to u >= 0, in the constrained (primal) form with v = K u and g = grad u as
constrained variables, K = [fanbeam2d ; gradient2d].  K is prost.block.fanbeam2d(size, size, 1, angles, R): Joseph's projector applied
without a matrix, five numbers per view and two per bin.  twin=True builds the same problem with prost.block.sparse of the explicit
matrix instead -- what a user with fan-beam data had to hand over before the block existed (about 2 n_views n_bins size non-zeros), short
of rebinning the data to parallel beams.  The phantom is that of tv_ct.py; the data f is its projection through the operator plus a
little noise.
usage: python examples/tv_ct_fan.py [--size 128] [--views 30] [--distance 3.0] [--detector flat|curved] [--twin]"""
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
from tv_ct import phantom, rmse


def bin_angles(ndet, D, spacing, shift, detector):
    """the fan angle of every bin, in Python floats (libm, as the host library)"""
    u = [(d - (ndet - 1) / 2.0) * spacing + shift for d in range(ndet)]
    return [v / D if detector == "curved" else math.atan2(v, D) for v in u]


def explicit_matrix(nx, ny, angles, R, D, ndet, spacing=1.0, shift=0.0, detector="flat", dtype=np.float64):
    """the matrix of prost.block.fanbeam2d(nx, ny, 1, angles, R, D, ndet, spacing, shift, detector) in the arithmetic of `dtype`, as a
    scipy CSC: per view cos, sin, the source (sx, sy) in index coordinates and the driving axis; per bin sin and cos of its fan angle;
    per ray the direction (dx, dy) = (sg cos - cg sin, sg sin + cg cos), its slope p, intercept r and weight c along the driving axis;
    the position f = r + p t on driving line t and the two entries c (1 - (f - floor f)) and c (f - floor f) at floor f and floor f + 1"""
    dtype = np.dtype(dtype)
    T = dtype.type
    cx, cy = (nx - 1) / 2.0, (ny - 1) / 2.0
    gamma = bin_angles(ndet, D, spacing, shift, detector)
    sg, cg = np.array([math.sin(g) for g in gamma]).astype(dtype), np.array([math.cos(g) for g in gamma]).astype(dtype)
    rows, cols, vals = [], [], []
    for a, beta in enumerate(np.asarray(angles, dtype=np.float64).ravel()):
        co, si = math.cos(float(beta)), math.sin(float(beta))
        column = abs(co) < abs(si)
        sx, sy, co, si = T(R * si + cx), T(-R * co + cy), T(co), T(si)
        dx, dy = sg * co - cg * si, sg * si + cg * co
        dt, di, st, s_i = (dx, dy, sx, sy) if column else (dy, dx, sy, sx)
        p = di / dt
        r = s_i - st * p
        c = T(1) / np.abs(dt)
        nt, ni = (nx, ny) if column else (ny, nx)
        t = np.arange(nt)
        f = r[:, None] + p[:, None] * t.astype(dtype)[None, :]
        fl = np.floor(f)
        w1 = f - fl
        i0 = np.where((fl >= -1) & (fl < ni), fl, -2).astype(np.int64)
        for i, w in ((i0, T(1) - w1), (i0 + 1, w1)):
            keep = (i0 >= -1) & (i >= 0) & (i < ni) & (w != 0)
            dd, tt = np.nonzero(keep)
            rows.append(a * ndet + dd)
            cols.append(i[keep] + tt * ny if column else tt + i[keep] * ny)
            vals.append((c[:, None] * w)[keep].astype(np.float64))
    return sp.csc_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(len(angles) * ndet, nx * ny))


def geometry(size, n_views, distance=3.0, detector="flat"):
    """-> (angles over a full turn, R = distance half diagonals, the default detector length)"""
    angles = np.arange(int(n_views)) * (2 * math.pi / int(n_views))
    R = float(distance) * math.hypot(size, size) / 2.0
    return angles, R, prost.block.fanbeam2d_ndet(size, size, R, detector=detector)


def describe(size=128, n_views=30, lmb=0.05, tol=1e-4, max_iters=5000, num_cback_calls=50, twin=False, sinogram=None, dtype=np.float64, noise=0.002, distance=3.0,
             detector="flat"):
    """sinogram: the data (a caller that compares the block with its twin hands one problem's data to the other); None: the phantom
    sent through the operator -- the block itself (twin: the matrix) -- plus noise of standard deviation `noise` times the largest
    projection.  dtype: the arithmetic the twin's matrix is formed in (that of the precision the problem is solved in)."""
    nx = ny = int(size)
    angles, R, ndet = geometry(size, n_views, distance, detector)
    truth = phantom(nx, ny)
    if twin:
        K = explicit_matrix(nx, ny, angles, R, R, ndet, detector=detector, dtype=dtype)
        op = prost.block.sparse(K)
    else:
        op = prost.block.fanbeam2d(nx, ny, 1, angles, R, ndet=ndet, detector=detector)
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


def back_projection(size, n_views, sinogram, distance=3.0, detector="flat"):
    """the unregularised comparator: K^T f scaled by the least-squares step <K^T f, K^T f> / |K K^T f|^2, through the explicit matrix"""
    angles, R, ndet = geometry(size, n_views, distance, detector)
    K = explicit_matrix(size, size, angles, R, R, ndet, detector=detector)
    b = K.T @ np.asarray(sinogram, dtype=np.float64)
    kb = K @ b
    return b * (float(b @ b) / float(kb @ kb))


def main(size=128, n_views=30, max_iters=5000, verbose=True, twin=False, lmb=0.05, distance=3.0, detector="flat"):
    prob, backend, opts, u, truth, sinogram = describe(size, n_views, lmb=lmb, max_iters=max_iters, twin=twin, distance=distance, detector=detector)
    t0 = time.perf_counter()
    result = prost.solve(prob, backend, opts)
    elapsed = time.perf_counter() - t0
    img = np.asarray(u.val)
    if verbose:
        print("%d x %d from %d %s fan-beam views at %.1f half diagonals: %s after %d iterations, %.3f s on %s; RMSE to the phantom %.4f, of the back-projection %.4f"
              % (size, size, n_views, detector, distance, result["result"], result["iters"], elapsed, result["path"], rmse(img, truth),
                 rmse(back_projection(size, n_views, sinogram, distance, detector), truth)))
    return result, img, truth, sinogram


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=128, help="the image is size x size")
    ap.add_argument("--views", type=int, default=30, help="projections, evenly over a full turn")
    ap.add_argument("--distance", type=float, default=3.0, help="the source's distance from the centre, in half diagonals of the image")
    ap.add_argument("--detector", choices=("flat", "curved"), default="flat")
    ap.add_argument("--twin", action="store_true", help="the sparse matrix instead of the block")
    a = ap.parse_args()
    main(a.size, a.views, twin=a.twin, distance=a.distance, detector=a.detector)
