"""TV-regularised SENSE reconstruction: an image from a quarter of the k-space lines of a coil array (parallel MRI with C = 8 coils),
min_u 1/2 sum_c |M (F (sigma_c . u) - d_c)|^2 + lmb TV(u) over a complex image u, in the constrained (primal) form with v = K u and
g = grad u as constrained variables, K = [sense2d ; gradient2d(nx, ny, 2)].  K u = [F (sigma_c . u)]_c is prost.block.sense2d: the
multi-coil Fourier operator applied without a matrix, the coil product fused into the first pass and the coil sum of the transpose into
the last.  The coils are synthetic: smooth Gaussian magnitude profiles placed on a circle around the field of view, each with a linear
phase, normalised to sum_c |sigma_c|^2 = 1, so that the operator's norm is 1 and the scaling is the identity.  The 0 / 1 sampling mask M
(tv_mri.sampling_mask: a fully sampled centre plus random lines) is coefficient c of the square data term on all C k-space images.  The
phantom is that of tv_ct.py taken as a complex image with zero imaginary part; the data is its multi-coil spectrum on the mask plus noise.
twin=True builds the same problem with prost.block.dense of the explicit matrix, (2 C N) x (2 N) values: small sizes only (32 x 32 with 8
coils is 268 MB in fp64, 256 x 256 would be 550 GB in fp32).  It prints the RMSE to the phantom of the reconstruction and of the
coil-combined zero-filled image K^T d, which needs no reconstruction.
usage: python examples/sense_mri.py [--size 128] [--coils 8] [--fraction 0.25] [--twin]"""
import argparse
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np

import prost_amd as prost
import tv_mri
from tv_ct import phantom, rmse


def coil_maps(nx, ny, coils=8, radius=1.1, width=0.9, turns=0.75):
    """-> complex (C, N), p = y + x ny: coil c sits at angle 2 pi c / C on a circle of `radius` half fields of view, has a Gaussian
    magnitude of standard deviation `width` and a linear phase of `turns` turns across the field of view along its own direction; the
    maps are divided by sqrt(sum_c |sigma_c|^2)"""
    y, x = np.mgrid[0:ny, 0:nx].astype(np.float64)
    X, Y = (x - (nx - 1) / 2.0) / (nx / 2.0), (y - (ny - 1) / 2.0) / (ny / 2.0)
    maps = []
    for c in range(int(coils)):
        a = 2.0 * math.pi * c / int(coils)
        cx, cy = radius * math.cos(a), radius * math.sin(a)
        mag = np.exp(-((X - cx) ** 2 + (Y - cy) ** 2) / (2.0 * width ** 2))
        maps.append(mag * np.exp(1j * math.pi * turns * (X * math.cos(a) + Y * math.sin(a))))
    maps = np.stack(maps)
    maps /= np.sqrt((np.abs(maps) ** 2).sum(axis=0))
    return maps.transpose(0, 2, 1).reshape(int(coils), nx * ny)


def forward(img, maps, nx, ny):
    """K on two real planes by numpy.fft -> the 2 C N values of the C k-space images, real planes first"""
    z = np.asarray(img, np.float64).reshape(2, nx * ny)
    s = np.fft.fft2(((z[0] + 1j * z[1]) * maps).reshape(-1, nx, ny), norm="ortho").reshape(-1, nx * ny)
    return np.concatenate([s.real.reshape(-1), s.imag.reshape(-1)])


def combined(data, maps, nx, ny):
    """K^T d by numpy.fft: the coil-combined inverse transform of the data with zeros where nothing was sampled"""
    C = maps.shape[0]
    d = np.asarray(data, np.float64).reshape(2, C, nx, ny)
    w = np.fft.ifft2(d[0] + 1j * d[1], norm="ortho").reshape(C, nx * ny)
    u = (np.conj(maps) * w).sum(axis=0)
    return np.concatenate([u.real, u.imag])


def explicit_matrix(nx, ny, maps, dtype=np.float64):
    """the matrix of prost.block.sense2d(nx, ny, maps, 1) in float64, the maps rounded to `dtype` as the block rounds them: rows (c, q),
    real parts first, A_c = F diag(sigma_c), K = [[Re A, -Im A], [Im A, Re A]]"""
    N, C = nx * ny, maps.shape[0]
    Kf = tv_mri.explicit_matrix(nx, ny)
    Cm, Sm = Kf[:N, :N], Kf[:N, N:]                                      # F = Cm - i Sm
    sr, si = maps.real.astype(dtype).astype(np.float64), maps.imag.astype(dtype).astype(np.float64)
    K = np.zeros((2 * C * N, 2 * N))
    for c in range(C):
        Ar, Ai = Cm * sr[c] + Sm * si[c], Cm * si[c] - Sm * sr[c]
        K[c * N:(c + 1) * N, :N], K[c * N:(c + 1) * N, N:] = Ar, -Ai
        K[(C + c) * N:(C + c + 1) * N, :N], K[(C + c) * N:(C + c + 1) * N, N:] = Ai, Ar
    return K


def describe(size=128, coils=8, fraction=0.25, lmb=0.002, tol=1e-4, max_iters=5000, num_cback_calls=50, twin=False, data=None, noise=0.005, scaling="identity",
             dtype=np.float64):
    """data: the masked k-space samples of the C coils (a caller that compares the block with its twin hands one problem's data to the
    other); None: the phantom's multi-coil spectrum plus noise of standard deviation `noise`, on the mask.  scaling: "identity", None (the
    problem's default, diagonal preconditioners from the block's bound sums) or the alpha of set_scaling_alpha.  dtype: the precision the
    twin's maps are rounded to (that of the precision the problem is solved in)."""
    nx = ny = int(size)
    N, C = nx * ny, int(coils)
    maps = coil_maps(nx, ny, C)
    truth = np.concatenate([phantom(nx, ny), np.zeros(N)])
    mask = np.tile(tv_mri.sampling_mask(nx, ny, fraction), 2 * C)
    if data is None:
        data = mask * (forward(truth, maps, nx, ny) + noise * np.random.default_rng(7).standard_normal(2 * C * N))
    op = prost.block.dense(explicit_matrix(nx, ny, maps, dtype)) if twin else prost.block.sense2d(nx, ny, maps, 1)
    u = prost.variable(2 * N)
    v = prost.variable(2 * C * N)
    g = prost.variable(4 * N)
    prob = prost.min_problem([u], [v, g])
    prob.add_function(v, prost.function.sum_1d("square", 1, data, mask, 0, 0))
    prob.add_function(g, prost.function.sum_norm2(4, False, "abs", 1, 0, lmb, 0, 0))
    prob.add_constraint(u, v, op)
    prob.add_constraint(u, g, prost.block.gradient2d(nx, ny, 2))
    if scaling == "identity":
        prob.set_scaling_identity()
    elif scaling is not None:
        prob.set_scaling_alpha(scaling)
    backend = prost.backend.pdhg(stepsize="boyd", residual_iter=1)
    opts = prost.options(max_iters=max_iters, num_cback_calls=num_cback_calls, verbose=False, tol_rel_primal=tol, tol_abs_primal=tol,
                         tol_rel_dual=tol, tol_abs_dual=tol)
    return prob, backend, opts, u, truth, data, mask, maps


def main(size=128, coils=8, fraction=0.25, max_iters=5000, verbose=True, twin=False, lmb=0.002, data=None, dtype=np.float64):
    prob, backend, opts, u, truth, data, mask, maps = describe(size, coils, fraction, lmb=lmb, max_iters=max_iters, twin=twin, data=data, dtype=dtype)
    t0 = time.perf_counter()
    result = prost.solve(prob, backend, opts)
    elapsed = time.perf_counter() - t0
    img = np.asarray(u.val)
    zero_filled = combined(data, maps, size, size)
    if verbose:
        print("%d x %d, %d coils, %.0f %% of k-space: %s after %d iterations, %.3f s on %s; RMSE to the phantom %.4f, of the coil-combined zero-filled image %.4f"
              % (size, size, coils, 100.0 * mask.mean(), result["result"], result["iters"], elapsed, result["path"], rmse(img, truth), rmse(zero_filled, truth)))
    return result, img, truth, data, zero_filled


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=128, help="the image is size x size, a power of two")
    ap.add_argument("--coils", type=int, default=8)
    ap.add_argument("--fraction", type=float, default=0.25, help="fraction of the k-space lines that is sampled")
    ap.add_argument("--twin", action="store_true", help="the dense matrix instead of the block (small sizes only)")
    a = ap.parse_args()
    main(a.size, a.coils, a.fraction, twin=a.twin)
