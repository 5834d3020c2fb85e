"""RGB ROF with nuclear-norm vectorial TV: the channels share their edges.

    min_u  1/2 |u - f|^2  +  lmb sum_pixels |J u(pixel)|_*        J u = the 3 x 2 Jacobian (channels x directions) of a pixel

|.|_* is the nuclear norm (sum of singular values).  Its conjugate is the indicator of the spectral-norm ball, so the dual
function is prost.function.sum_singular_nx2 with 'ind_leq0' on  sigma / lmb - 1:  every singular value of a pixel's dual matrix
stays below lmb.  gradient2d with 3 channels writes, per pixel, the three d/dx entries and then the three d/dy entries in planar
order -- the column-first layout sum_singular_nx2 reads (dim = 6, n = 3).

No image file travels with this repository, so a synthetic RGB image stands in (prost_amd.synthetic.rof_image), as in the
other examples.  The callback prints the primal-dual gap, evaluated in NumPy.
usage: python examples/rof_rgb_nuclear_tv.py [nx ny]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import prost_amd as prost
from prost_amd import synthetic

from rof_rgb_gap_callback import spmat_gradient2d


def describe(nx=256, ny=192, lmb=0.3):
    """-> (prob, u, q, f): the problem description"""
    nc = 3
    f = synthetic.rof_image(nx, ny, nc, seed=1).astype(np.float64)
    u = prost.variable(nx * ny * nc)
    q = prost.variable(2 * nx * ny * nc)
    prob = prost.min_max_problem([u], [q])
    prob.add_function(u, prost.function.sum_1d("square", 1, f, 1))
    prob.add_function(q, prost.function.sum_singular_nx2(2 * nc, False, "ind_leq0", 1 / lmb, 1, 1, 0, 0))
    prob.add_dual_pair(u, q, prost.block.gradient2d(nx, ny, nc))
    return prob, u, q, f


def energies(grad, f, lmb, nx, ny, x, y):
    """(primal, dual) energy in fp64; the dual one is finite because y is feasible after every prox"""
    nc = 3
    jac = (grad @ x).reshape(2, nc, nx * ny).transpose(2, 1, 0)            # (pixel, channel, direction)
    primal = 0.5 * np.sum((x - f) ** 2) + lmb * np.linalg.svd(jac, compute_uv=False).sum()
    div = grad.T @ y
    dual = f @ div - 0.5 * np.sum(div ** 2)                                # -g*(-K^T y), g = 1/2 |. - f|^2
    return primal, dual


def main(nx=256, ny=192, lmb=0.3, max_iters=2000, num_cback_calls=10, verbose=True, backend=None, **solver_opts):
    prob, u, q, f = describe(nx, ny, lmb)
    grad = spmat_gradient2d(nx, ny, 3)
    gaps = []

    def pd_gap_callback(it, x, y):
        primal, dual = energies(grad, f, lmb, nx, ny, np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64))
        gaps.append((primal - dual) / (nx * ny))
        if verbose:
            print("it %5d primal-dual gap per pixel %.3e" % (it, gaps[-1]))
        return False

    if backend is None:
        backend = prost.backend.pdhg(stepsize="boyd", residual_iter=1)      # the reference's default options
    opts = prost.options(max_iters=max_iters, interm_cb=pd_gap_callback, num_cback_calls=num_cback_calls, verbose=False, **solver_opts)
    t0 = time.perf_counter()
    result = prost.solve(prob, backend, opts)
    elapsed = time.perf_counter() - t0
    prost.release()
    if verbose:
        print("%s after %d iterations, %.3f s (%s)" % (result["result"], result["iters"], elapsed, result.get("path")))
    return result, gaps, u.val.reshape(3, nx, ny), q.val


if __name__ == "__main__":
    main(*[int(a) for a in sys.argv[1:3]])
