"""TV-regularised reconstruction of an image from a fraction of its Fourier samples (compressed-sensing MRI with one coil):
min_u 1/2 |M (F u - d)|^2 + lmb TV(u) over a complex image u, in the constrained (primal) form with v = F u and g = grad u as
constrained variables, K = [fft2d ; gradient2d(nx, ny, 2)].  F is prost.block.fft2d(size, size): the unitary 2-D Fourier transform
applied without a matrix.  The 0 / 1 sampling mask M is not part of the block; it is coefficient c of the square data term,
sum_1d("square", 1, d, mask, 0, 0) on v, the way tv_inpaint.py masks pixels.  The complex image is two real planes (real parts first),
which is the domain of gradient2d with two channels, so sum_norm2(4, ..) over its four differences is the isotropic TV of the complex
image.  The phantom is that of tv_ct.py taken as a complex image with zero imaginary part; the sampling is a fully sampled
low-frequency centre plus random k-space lines (fixed seed); the data is the phantom's spectrum on the mask plus a little noise.
The operator is orthogonal, so the scaling is the identity (diagonal preconditioners of a dense orthogonal matrix are very
conservative).  twin=True builds the same problem with prost.block.dense of the explicit matrix, (2 N)^2 values: usable only at small
sizes (32 x 32 is 32 MB in fp64, 256 x 256 would be 137 GB).
usage: python examples/tv_mri.py [--size 128] [--fraction 0.5] [--twin]"""
import argparse
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np

import prost_amd as prost
from tv_ct import phantom, rmse


def sampling_mask(nx, ny, fraction, centre=0.08, seed=5):
    """-> 0 / 1 over the frequencies q = ky + kx ny: whole lines kx, those with |kx| (signed frequency) below centre nx / 2 always, the
    rest drawn at random until `fraction` of the lines is taken"""
    rng = np.random.default_rng(seed)
    signed = np.minimum(np.arange(nx), nx - np.arange(nx))
    take = signed <= max(1, int(round(centre * nx / 2)))
    want = max(int(take.sum()), int(round(fraction * nx)))
    rest = rng.permutation(np.nonzero(~take)[0])
    take[rest[:want - int(take.sum())]] = True
    return np.repeat(take.astype(np.float64), ny)


def explicit_matrix(nx, ny):
    """the matrix of prost.block.fft2d(nx, ny, 1) in float64: K = s [[C, S], [-S, C]], C = cos(theta), S = sin(theta),
    theta = 2 pi (ky y / ny + kx x / nx), s = 1 / sqrt(nx ny); rows q = ky + kx ny, columns p = y + x ny"""
    ty = (np.outer(np.arange(ny), np.arange(ny)) % ny) / float(ny)
    tx = (np.outer(np.arange(nx), np.arange(nx)) % nx) / float(nx)
    theta = 2.0 * np.pi * (tx[:, None, :, None] + ty[None, :, None, :]).reshape(nx * ny, nx * ny)
    s = 1.0 / math.sqrt(float(nx * ny))
    Cm, Sm = s * np.cos(theta), s * np.sin(theta)
    return np.block([[Cm, Sm], [-Sm, Cm]])


def spectrum(img, nx, ny, inverse=False):
    """the operator (or its transpose) on two real planes by numpy.fft: for making data and for the zero-filled reconstruction"""
    z = np.asarray(img, np.float64).reshape(2, nx, ny)
    z = z[0] + 1j * z[1]
    z = np.fft.ifft2(z, norm="ortho") if inverse else np.fft.fft2(z, norm="ortho")
    return np.concatenate([z.real.reshape(-1), z.imag.reshape(-1)])


def describe(size=128, fraction=0.5, lmb=0.005, tol=1e-4, max_iters=5000, num_cback_calls=50, twin=False, data=None, noise=0.01, scaling="identity"):
    """data: the masked k-space samples d (a caller that compares the block with its twin hands one problem's data to the other);
    None: the phantom's spectrum plus noise of standard deviation `noise`, on the mask.  scaling: "identity", None (the problem's
    default, diagonal preconditioners from the block's closed-form sums) or the alpha of set_scaling_alpha."""
    nx = ny = int(size)
    N = nx * ny
    truth = np.concatenate([phantom(nx, ny), np.zeros(N)])
    mask = np.tile(sampling_mask(nx, ny, fraction), 2)
    if data is None:
        data = mask * (spectrum(truth, nx, ny) + noise * np.random.default_rng(7).standard_normal(2 * N))
    op = prost.block.dense(explicit_matrix(nx, ny)) if twin else prost.block.fft2d(nx, ny, 1)
    u = prost.variable(2 * N)
    v = prost.variable(2 * N)
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
    return prob, backend, opts, u, truth, data, mask


def zero_filled(data, nx, ny):
    """the inverse transform of the data with zeros where nothing was sampled: what needs no reconstruction"""
    return spectrum(data, nx, ny, inverse=True)


def main(size=128, fraction=0.5, max_iters=5000, verbose=True, twin=False, lmb=0.005):
    prob, backend, opts, u, truth, data, mask = describe(size, fraction, lmb=lmb, max_iters=max_iters, twin=twin)
    t0 = time.perf_counter()
    result = prost.solve(prob, backend, opts)
    elapsed = time.perf_counter() - t0
    img = np.asarray(u.val)
    if verbose:
        print("%d x %d from %.0f %% of k-space: %s after %d iterations, %.3f s on %s; RMSE to the phantom %.4f, of the zero-filled inverse transform %.4f"
              % (size, size, 100.0 * mask.mean(), result["result"], result["iters"], elapsed, result["path"], rmse(img, truth), rmse(zero_filled(data, size, size), truth)))
    return result, img, truth, data


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=128, help="the image is size x size, a power of two")
    ap.add_argument("--fraction", type=float, default=0.5, help="fraction of the k-space lines that is sampled")
    ap.add_argument("--twin", action="store_true", help="the dense matrix instead of the block (small sizes only)")
    a = ap.parse_args()
    main(a.size, a.fraction, twin=a.twin)
