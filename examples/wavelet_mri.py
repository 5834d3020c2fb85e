"""Compressed-sensing MRI with both classical sparsity priors: min_u 1/2 |M (F u - d)|^2 + lmb_w |W u|_1 + lmb_tv TV(u) over a
complex image u, in the constrained (primal) form with v = F u, w = W u and g = grad u as constrained variables,
K = [fft2d ; wavelet2d(nx, ny, 2, ..) ; gradient2d(nx, ny, 2)].  It is examples/tv_mri.py (same phantom, same sampling mask, same data)
plus the l1-norm of the wavelet coefficients: W is prost.block.wavelet2d, the orthogonal periodised multi-level wavelet transform
applied without a matrix to the two real planes of u, and sum_norm2(2, False, "abs", ..) over (re, im) of every coefficient is the
complex magnitude.  All three operators have norm 1 or sqrt(8), so the scaling is the identity.  twin=True builds the same problem from
explicit matrices: prost.block.dense for F and prost.block.sparse for W (its coarse rows wrap around the whole image and are dense);
usable only at small sizes.
usage: python examples/wavelet_mri.py [--size 128] [--fraction 0.5] [--wavelet db2] [--levels 3] [--twin]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np

import prost_amd as prost
import tv_mri
from tv_ct import phantom, rmse
from tv_mri import sampling_mask, spectrum, zero_filled


def wavelet_matrix(nx, ny, taps, levels):
    """the matrix of prost.block.wavelet2d(nx, ny, 1, taps, levels) in float64, N x N: level l applies the one-level matrices of its
    corner, W_y (.) W_x^T, and leaves the rest alone"""
    h = np.asarray(taps, np.float64)
    g = h[::-1] * (-1.0) ** np.arange(h.size)

    def one_level(m):
        W = np.zeros((m, m))
        for k in range(m // 2):
            for t in range(h.size):
                W[k, (2 * k + t) % m] += h[t]
                W[m // 2 + k, (2 * k + t) % m] += g[t]
        return W

    N = nx * ny
    M = np.eye(N).reshape(nx, ny, N)
    for l in range(levels):
        my, mx = (ny >> l if ny > 1 else 1), (nx >> l if nx > 1 else 1)
        c = M[:mx, :my, :]
        if my > 1:
            c = np.einsum("ab,xbn->xan", one_level(my), c, optimize=True)
        if mx > 1:
            c = np.einsum("ab,byn->ayn", one_level(mx), c, optimize=True)
        M[:mx, :my, :] = c
    return M.reshape(N, N)


def describe(size=128, fraction=0.5, lmb_w=0.001, lmb_tv=0.005, wavelet="db2", levels=3, tol=1e-4, max_iters=5000, num_cback_calls=50, twin=False, data=None,
             noise=0.01, scaling="identity"):
    """data: the masked k-space samples d (a caller that compares the blocks with their twins hands one problem's data to the other);
    None: the phantom's spectrum plus noise of standard deviation `noise`, on the mask.  scaling: "identity", None (the problem's
    default, diagonal preconditioners from the blocks' sums) or the alpha of set_scaling_alpha."""
    nx = ny = int(size)
    N = nx * ny
    truth = np.concatenate([phantom(nx, ny), np.zeros(N)])
    mask = np.tile(sampling_mask(nx, ny, fraction), 2)
    if data is None:
        data = mask * (spectrum(truth, nx, ny) + noise * np.random.default_rng(7).standard_normal(2 * N))
    taps = prost.block.wavelet2d_taps(wavelet) if isinstance(wavelet, str) else np.asarray(wavelet, np.float64)
    if twin:
        import scipy.sparse as sp
        fourier = prost.block.dense(tv_mri.explicit_matrix(nx, ny))
        one = sp.csc_matrix(wavelet_matrix(nx, ny, taps, levels))
        transform = prost.block.sparse(sp.block_diag([one, one], format="csc"))
    else:
        fourier = prost.block.fft2d(nx, ny, 1)
        transform = prost.block.wavelet2d(nx, ny, 2, taps, levels)
    u = prost.variable(2 * N)
    v = prost.variable(2 * N)
    w = prost.variable(2 * N)
    g = prost.variable(4 * N)
    prob = prost.min_problem([u], [v, w, g])
    prob.add_function(v, prost.function.sum_1d("square", 1, data, mask, 0, 0))
    prob.add_function(w, prost.function.sum_norm2(2, False, "abs", 1, 0, lmb_w, 0, 0))
    prob.add_function(g, prost.function.sum_norm2(4, False, "abs", 1, 0, lmb_tv, 0, 0))
    prob.add_constraint(u, v, fourier)
    prob.add_constraint(u, w, transform)
    prob.add_constraint(u, g, prost.block.gradient2d(nx, ny, 2))
    if scaling == "identity":
        prob.set_scaling_identity()
    elif scaling is not None:
        prob.set_scaling_alpha(scaling)
    backend = prost.backend.pdhg(stepsize="boyd", residual_iter=1)
    opts = prost.options(max_iters=max_iters, num_cback_calls=num_cback_calls, verbose=False, tol_rel_primal=tol, tol_abs_primal=tol,
                         tol_rel_dual=tol, tol_abs_dual=tol)
    return prob, backend, opts, u, truth, data, mask


def main(size=128, fraction=0.5, max_iters=5000, verbose=True, twin=False, wavelet="db2", levels=3, lmb_w=0.001, lmb_tv=0.005):
    prob, backend, opts, u, truth, data, mask = describe(size, fraction, lmb_w=lmb_w, lmb_tv=lmb_tv, wavelet=wavelet, levels=levels, max_iters=max_iters, twin=twin)
    t0 = time.perf_counter()
    result = prost.solve(prob, backend, opts)
    elapsed = time.perf_counter() - t0
    img = np.asarray(u.val)
    if verbose:
        print("%d x %d from %.0f %% of k-space, %s at %d levels: %s after %d iterations, %.3f s on %s; RMSE to the phantom %.4f, of the zero-filled inverse "
              "transform %.4f" % (size, size, 100.0 * mask.mean(), wavelet if isinstance(wavelet, str) else "%d taps" % len(wavelet), levels, result["result"],
                                  result["iters"], elapsed, result["path"], rmse(img, truth), rmse(zero_filled(data, size, size), truth)))
    return result, img, truth, data


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=128, help="the image is size x size, a power of two divisible by 2^levels")
    ap.add_argument("--fraction", type=float, default=0.5, help="fraction of the k-space lines that is sampled")
    ap.add_argument("--wavelet", default="db2", help="haar, db2 or db3")
    ap.add_argument("--levels", type=int, default=3, help="levels of the pyramid")
    ap.add_argument("--twin", action="store_true", help="explicit matrices instead of the blocks (small sizes only)")
    a = ap.parse_args()
    main(a.size, a.fraction, twin=a.twin, wavelet=a.wavelet, levels=a.levels)
