"""One PDHG iteration on a gradient operator as the reference evaluates it, through the CPU oracle's pieces -- shared by the tests that
compare the fused iteration kernels with it."""
import numpy as np

import oracle

F_COEFFS = [1.0, 1.0, 1.0, 0.0, 0.0, 0.3, 0.0]
SVAL = 0.5


def oracle_iteration(kind, x, y, shape, g_coeffs, tval, tau, sigma, theta, dtype=np.float32, g_fn="square", f_fn="ind_leq0", f_coeffs=F_COEFFS):
    """one PDHG iteration as the reference evaluates it (backend_pdhg.cu:313-370), every operation rounded to `dtype`; also returns
    the squared norms of the dual prox's arguments.  kind: "2d" / "mc" (gradient2d, dual groups of 2 L components) or "3d" (gradient3d)"""
    DT = np.dtype(dtype).type
    nx, ny, L = shape
    n = nx * ny * L
    grad = oracle.grad3d if kind == "3d" else oracle.grad2d
    comps = 3 if kind == "3d" else 2
    tau, sigma, theta = DT(tau), DT(sigma), DT(theta)
    Td, Sd = np.full(n, tval, DT), np.full(comps * n, SVAL, DT)
    with np.errstate(all="ignore"):
        kty = grad(y, nx, ny, L, adjoint=True)
        x1 = oracle.prox_elem(0, g_fn, (x - tau * Td * kty).astype(DT), Td, tau, n, 1, False, g_coeffs)
        kx, kxp = grad(x1, nx, ny, L), grad(x, nx, ny, L)
        arg = (y + sigma * Sd * ((1 + theta) * kx - theta * kxp)).astype(DT)
        count, dim = (n, 3) if kind == "3d" else (nx * ny, 2 * L)
        y1 = oracle.prox_elem(1, f_fn, arg, Sd, sigma, count, dim, False, f_coeffs)
        nv = (arg.astype(np.float64).reshape(dim, count) ** 2).sum(axis=0)
    return x1, y1, nv
