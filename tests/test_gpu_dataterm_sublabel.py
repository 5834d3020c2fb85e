"""prost.block.dataterm_sublabel on the GPU: the kernels through prost.eval_linop and through the C ABI, the block in the solver and in
examples/sublabel_dataterm.py.

References: tests/dataterm_sublabel_reference.py, never the code under test.
  * products: forward and adjoint equal the NumPy restatement (b) in T bit for bit, also where a second block accumulates (the
    restatement adds in the kernel's order, res + value) and where a 1 x 1 block in front gives the block odd row and column offsets;
    the same call twice gives the same bits; row and column sums equal (c);
  * against the oracle's block.sparse on matrix (a) with float-exact delta and gamma: |got - twin| <= 1.01 (k + 2) u (|K| |x|)
    componentwise, u the unit roundoff of T -- the forward error bound of a sum of k + 1 terms in any order (derived, not measured);
  * the C entry points with offset pointers and in place (prost_hip.h allows res == rhs);
  * a solve without regulariser decouples per pixel and has a closed form; the distance reached after a fixed iteration count was
    measured once on an MI355X (docs/rounds/r17.md), ten times it is asserted;
  * the example at 24 x 16, L = 4 with convex data against the direct form.
"""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

import dataterm_sublabel_reference as R
import epi_conjquad_reference as ECQ
import oracle
import prost_amd as prost
from prost_amd import _hip

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))

pytestmark = pytest.mark.gpu
PRECISIONS = [("single", np.float32), ("double", np.float64)]

# (nx, ny, L): one pixel with one and two intervals; fewer pixels than one 16-byte access; ny alone; a workgroup boundary plus a ragged
# element (257 = 256 + 1: the element instance in both precisions); 256 pixels: the vector instance in both precisions, exactly one
# workgroup of the element instance; 1030 pixels, 32 intervals: a long march, more than one workgroup of the element instance (fp32:
# 1030 is no multiple of 4) and of the vector instance (fp64: 515 lanes)
SHAPES = [(1, 1, 2), (1, 1, 3), (5, 1, 4), (1, 7, 2), (257, 1, 9), (16, 16, 5), (103, 10, 33)]
LEFT, RIGHT = -0.3, 1.1          # delta and gamma are not float-representable: they have to reach the device rounded as (b) rounds them


@pytest.fixture(autouse=True)
def _gpu(hip):
    prost.set_gpu(0)
    yield
    prost.set_precision("double")


def ids(s):
    return "x".join(map(str, s))


def run(linop, rhs, transpose):
    got, rowsum, colsum, _ = prost.eval_linop(linop, rhs, transpose)
    return np.asarray(got, dtype=np.float64).ravel(), np.asarray(rowsum, dtype=np.float64).ravel(), np.asarray(colsum, dtype=np.float64).ravel()


@pytest.mark.parametrize("prec,dtype", PRECISIONS)
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_products_and_sums_bit_for_bit(prec, dtype, shape):
    prost.set_precision(prec)
    nx, ny, L = shape
    N, k = nx * ny, L - 1
    n = 2 * N * k
    rng = np.random.default_rng(nx + 10 * ny + 1000 * L)
    linop = [prost.block.dataterm_sublabel(nx, ny, L, LEFT, RIGHT)(0, 0, n, n)[0]]
    for transpose in (False, True):
        x = rng.standard_normal(n)
        got, rowsum, colsum = run(linop, x, transpose)
        want = R.product(x, N, L, LEFT, RIGHT, transpose, dtype).astype(np.float64)
        assert got.shape == want.shape and np.array_equal(got, want), float(np.abs(got - want).max())
        assert np.array_equal(run(linop, x, transpose)[0], got)                 # no atomics: the same bits every time
        rs, cs = R.sums(N, L, LEFT, RIGHT, 1.0, dtype)
        assert np.array_equal(rowsum, rs.astype(np.float64)) and np.array_equal(colsum, cs.astype(np.float64))


@pytest.mark.parametrize("prec,dtype", PRECISIONS)
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_accumulation_and_odd_offsets_bit_for_bit(prec, dtype, shape):
    """[B B]: the second block adds onto the first in the forward product; [B ; B]: in the adjoint; diag(d, B) with a 1 x 1 diags block
    d in front: B's rows and columns start at element 1, so res and rhs are aligned for one element only"""
    prost.set_precision(prec)
    nx, ny, L = shape
    N, k = nx * ny, L - 1
    n = 2 * N * k
    rng = np.random.default_rng(7 * nx + 70 * ny + 700 * L)
    bf = prost.block.dataterm_sublabel(nx, ny, L, LEFT, RIGHT)
    arg = (N, L, LEFT, RIGHT)
    x2, x1 = rng.standard_normal(2 * n), rng.standard_normal(n)
    side = [bf(0, 0, n, n)[0], bf(0, n, n, n)[0]]
    got = run(side, x2, False)[0]
    want = R.forward(x2[n:], *arg, dtype, res0=R.forward(x2[:n], *arg, dtype))
    assert np.array_equal(got, want.astype(np.float64))
    got = run(side, x1, True)[0]
    assert np.array_equal(got, np.tile(R.adjoint(x1, *arg, dtype), 2).astype(np.float64))
    stack = [bf(0, 0, n, n)[0], bf(n, 0, n, n)[0]]
    got = run(stack, x1, False)[0]
    assert np.array_equal(got, np.tile(R.forward(x1, *arg, dtype), 2).astype(np.float64))
    got = run(stack, x2, True)[0]
    want = R.adjoint(x2[n:], *arg, dtype, res0=R.adjoint(x2[:n], *arg, dtype))
    assert np.array_equal(got, want.astype(np.float64))
    shifted = [prost.block.diags(1, 1, [2.0], [0])(0, 0, 1, 1)[0], bf(1, 1, n, n)[0]]
    xs = rng.standard_normal(n + 1)
    for transpose in (False, True):
        got = run(shifted, xs, transpose)[0]
        want = np.concatenate([(np.zeros(1, dtype) + dtype(2.0) * xs[:1].astype(dtype)), R.product(xs[1:], *arg, transpose, dtype)])
        assert np.array_equal(got, want.astype(np.float64))
        assert np.array_equal(run(shifted, xs, transpose)[0], got)


@pytest.mark.parametrize("prec,dtype", PRECISIONS)
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_against_the_sparse_twin_in_the_oracle(prec, dtype, shape):
    """left = 0.25, delta = 0.25: delta and every gamma_i are exact in float, so the twin's matrix is the block's"""
    prost.set_precision(prec)
    nx, ny, L = shape
    N, k = nx * ny, L - 1
    n = 2 * N * k
    left, right = 0.25, 0.25 + 0.25 * k
    delta, gamma = R.labels(L, left, right, np.float32)
    assert float(delta) == 0.25 and np.array_equal(gamma.astype(np.float64), 0.25 + 0.25 * np.arange(k))
    K = R.matrix(nx, ny, L, left, right)
    twin = [prost.block.sparse(K)(0, 0, n, n)[0]]
    linop = [prost.block.dataterm_sublabel(nx, ny, L, left, right)(0, 0, n, n)[0]]
    rng = np.random.default_rng(3 * nx + 30 * ny + 300 * L)
    u = np.finfo(dtype).eps / 2
    for transpose in (False, True):
        x = rng.standard_normal(n).astype(dtype).astype(np.float64)
        got, rowsum, colsum = run(linop, x, transpose)
        want, orow, ocol = oracle.eval_linop(twin, x, transpose, dtype)
        M = K.T if transpose else K
        bound = 1.01 * (k + 2) * u * (abs(M) @ np.abs(x))
        err = np.abs(got - want)
        print("%s %s transpose=%d: |got - twin| / bound %.3f, |got - exact| / bound %.3f" % (prec, shape, transpose, float((err / bound).max()),
                                                                                             float((np.abs(got - M @ x) / bound).max())))
        assert np.all(err <= bound), float((err / bound).max())
        assert np.all(np.abs(got - M @ x) <= bound) and np.all(np.abs(want - M @ x) <= bound)
        assert np.array_equal(rowsum, orow) and np.array_equal(colsum, ocol)


def call(dtype, x, N, L, left, right, transpose, accumulate, offset, in_place, res0=None):
    """one launch through the C ABI; res and rhs start `offset` elements into their allocations"""
    delta, gamma = R.labels(L, left, right, dtype)
    n = 2 * N * (L - 1)
    pad = np.zeros(offset, dtype)
    keep = [_hip.DeviceArray.from_host(np.concatenate([pad, x.astype(dtype)])),
            _hip.DeviceArray.from_host(np.concatenate([pad, (np.zeros(n) if res0 is None else res0).astype(dtype)])),
            _hip.DeviceArray.from_host(gamma)]
    rhs, res, g = keep
    if in_place:
        res = rhs
    fn = _hip.fn("linop_dataterm_sublabel", dtype)
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_double, C.c_int, C.c_int, C.c_void_p]
    fn.restype = C.c_int
    try:
        _hip.check(fn(res.offset(offset), rhs.offset(offset), N, L, g.ptr, float(delta), int(transpose), int(accumulate), None))
        _hip.sync()
        out = res.to_host()
        assert np.array_equal(out[:offset], pad)
        return out[offset:]
    finally:
        for d in keep:
            d.free()


@pytest.mark.parametrize("prec,dtype", PRECISIONS)
def test_c_abi_offset_pointers_and_in_place(prec, dtype):
    """offset 0 / 4: 16-byte aligned (the vector instance where N allows it); 1: aligned for one element only; in place: res == rhs,
    which include/prost_hip.h allows in both directions and with accumulate (then res = x + K x)"""
    rng = np.random.default_rng(12)
    for nx, ny, L in ((16, 16, 5), (257, 1, 9), (1, 1, 2), (6, 1, 3)):
        N = nx * ny
        n = 2 * N * (L - 1)
        x, res0 = rng.standard_normal(n).astype(dtype), rng.standard_normal(n).astype(dtype)
        for offset in (0, 1, 4):
            for transpose in (False, True):
                plain = R.product(x, N, L, LEFT, RIGHT, transpose, dtype)
                assert np.array_equal(call(dtype, x, N, L, LEFT, RIGHT, transpose, False, offset, False, res0), plain)
                assert np.array_equal(call(dtype, x, N, L, LEFT, RIGHT, transpose, True, offset, False, res0), res0 + plain)
                assert np.array_equal(call(dtype, x, N, L, LEFT, RIGHT, transpose, False, offset, True), plain)
                assert np.array_equal(call(dtype, x, N, L, LEFT, RIGHT, transpose, True, offset, True), x + plain)
    # refusals without a launch
    fn = _hip.fn("linop_dataterm_sublabel", dtype)
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_double, C.c_int, C.c_int, C.c_void_p]
    fn.restype = C.c_int
    assert fn(None, None, 4, 1, None, 0.5, 0, 0, None) != 0
    assert fn(None, None, 4, 3, None, 0.5, 0, 0, None) != 0
    assert fn(None, None, 0, 3, None, 0.5, 0, 0, None) == 0


# ---- solves ----
# relative inf-norm distance of the recovered t to the closed form after SOLVE_ITERS iterations, measured once on an MI355X; ten times
# it is asserted.  alg2 shrinks tau by 1 / sqrt(1 + 2 gamma tau) per iteration, which presumes a strongly convex g; here g is an indicator
# (and zero), and with alg2_gamma = 0.5 the primal steps die out before the iterate arrives (a NumPy PDHG on the sparse twin stalls at a
# distance of 0.4 for thousands of iterations, and reaches 1e-15 within 1000 with constant steps).  ALG2_GAMMA keeps tau within a
# factor of about 3 of its start over SOLVE_ITERS iterations (tau_n is about tau_0 / (1 + gamma tau_0 n)).
ALG2_GAMMA = 1e-3
SOLVE_ITERS = 2000
SOLVE_DISTANCE = {
    "single": 1.62e-07,
    "double": 4.58e-16,
}
SOLVE_N, SOLVE_L = 40, 5


@functools.lru_cache(maxsize=None)
def solve_case():
    """40 pixels, L = 5 on [0, 1], the truncated quadratic of the example: f at least 0.1 delta from every label, weights in [1, 3] and
    nu = 0.05 > 3 delta^2 / 4, so the piece that holds f is the quadratic (value 0 at t = f, the unique minimiser) and distant pieces are
    the constant.  -> pieces, closed form t"""
    import sublabel_dataterm as ex
    rng = np.random.default_rng(77)
    L, n = SOLVE_L, SOLVE_N
    delta, gamma = ex.label_grid(L)
    f = gamma[rng.integers(0, L - 1, n)] + delta * rng.uniform(0.1, 0.9, n)
    weight = rng.uniform(1.0, 3.0, n)
    a, b, c = ex.truncated_pieces(f, weight, L, nu=0.05)
    A, B, Cc = a.reshape(L - 1, n), b.reshape(L - 1, n), c.reshape(L - 1, n)
    assert (A == 0).mean() > 0.2 and (A > 0).mean() > 0.2
    lo, hi = gamma[:, None], gamma[:, None] + delta
    with np.errstate(divide="ignore", invalid="ignore"):
        tmin = np.where(A > 0, np.clip(-B / (2 * np.where(A > 0, A, 1.0)), lo, hi), lo + delta / 2)
    val = (A * tmin + B) * tmin + Cc
    best = np.argmin(val, axis=0)
    t = tmin[best, np.arange(n)]
    srt = np.sort(val, axis=0)
    assert np.all(srt[1] - srt[0] > 1e-3)                              # a unique minimiser
    assert np.all(np.abs((t - gamma[0]) / delta - np.round((t - gamma[0]) / delta)) >= 0.1 - 1e-12)
    assert np.allclose(t, f)
    return (a, b, c), t


def solve(precision, backend, iters):
    import sublabel_dataterm as ex
    (a, b, c), _ = solve_case()
    prost.set_precision(precision)
    prob, subs = ex.describe_lifted(SOLVE_N, 1, SOLVE_L, a, b, c, regulariser=False)
    o = prost.options(max_iters=iters, num_cback_calls=0, verbose=False, tol_rel_primal=0, tol_rel_dual=0, tol_abs_primal=0, tol_abs_dual=0)
    s = prost.Solver(prob, backend, o)
    s.iterate(iters)
    st = s.state()
    s.destroy()
    return st


def feasible(r, s, a, b, c, L, dtype):
    """(r, s) in the epigraphs within the bound of tests/test_gpu_epi_conjquad.py: max(4 e_T, 32 eps_T) max(1, |z0|_inf, |P|_inf)"""
    import sublabel_dataterm as ex
    delta, gamma = ex.label_grid(L)
    alpha = np.repeat(gamma, r.size // (L - 1))
    co = (a, b, c, alpha, alpha + delta)
    y, t, _ = ECQ.project(r, s, *co, np.float64)
    yt, tt, _ = ECQ.project(r, s, *co, dtype)
    scale = np.maximum(1.0, np.maximum(np.maximum(np.abs(r), np.abs(s)), np.maximum(np.abs(y), np.abs(t))))
    e_t = np.maximum(np.abs(yt.astype(np.float64) - y), np.abs(tt.astype(np.float64) - t)) / scale
    bound = np.maximum(4 * e_t, 32 * np.finfo(dtype).eps) * scale
    out = ECQ.outside(r, s, *co)
    return bool((out <= bound).all()), float((out / bound).max())


@pytest.mark.parametrize("precision,dtype", PRECISIONS)
def test_solve_without_regulariser_reaches_the_closed_form(precision, dtype):
    import sublabel_dataterm as ex
    (a, b, c), want = solve_case()
    st = solve(precision, prost.backend.pdhg(stepsize="alg2", residual_iter=10, alg2_gamma=ALG2_GAMMA), SOLVE_ITERS)
    assert st["path"] == "pdhg:generic", st["path"]
    n, k = SOLVE_N, SOLVE_L - 1
    x, z = st["x"].astype(np.float64).ravel(), st["y"].astype(np.float64).ravel()
    t = ex.recover(x[:n * k], n, SOLVE_L)
    rel = float(np.abs(t - want).max()) / float(np.abs(want).max())
    print("solve %s: relative distance %.3g after %d iterations" % (precision, rel, SOLVE_ITERS))
    w = x[n * k:].reshape(k, n)
    tol = 32 * k * np.finfo(dtype).eps
    print("solve %s: simplex defect %.3g, smallest w %.3g" % (precision, float(np.abs(w.sum(axis=0) - 1).max()), float(w.min())))
    assert np.all(w >= 0) and np.all(np.abs(w.sum(axis=0) - 1) <= tol)          # x is an output of the simplex projection
    ok, ratio = feasible(z[:n * k], z[n * k:], a, b, c, SOLVE_L, dtype)
    print("solve %s: (r, s) outside / bound %.3f" % (precision, ratio))
    assert ok, ratio
    assert rel <= 10 * SOLVE_DISTANCE[precision], rel


@pytest.mark.parametrize("precision,dtype", PRECISIONS)
def test_boyd_with_residual_iter_1_completes_on_the_generic_path(precision, dtype):
    import sublabel_dataterm as ex
    _, want = solve_case()
    st = solve(precision, prost.backend.pdhg(stepsize="boyd", residual_iter=1), 300)
    assert st["path"] == "pdhg:generic", st["path"]
    x = st["x"].astype(np.float64).ravel()
    assert np.isfinite(x).all() and np.isfinite(st["y"]).all()
    t = ex.recover(x[:SOLVE_N * (SOLVE_L - 1)], SOLVE_N, SOLVE_L)
    print("boyd %s: relative distance %.3g after 300 iterations" % (precision, float(np.abs(t - want).max()) / float(np.abs(want).max())))


def test_the_example_with_convex_data_against_the_direct_form():
    """24 x 16, L = 4.  The lifted regulariser sum_i delta TV(u_i) only dominates TV(t) in the discrete setting, so the lifted t need not
    reach the direct optimum: the gap is printed (docs/rounds/r17.md), not asserted small.  It cannot be negative beyond the tolerance
    the direct solve itself stops at."""
    import sublabel_dataterm as ex
    prost.set_precision("double")
    nx, ny, L = 24, 16, 4
    out = ex.main(nx, ny, L, max_iters=50000, verbose=False, data="convex")["convex"]
    e, e1 = out["energy"], out["energy_direct"]
    print("example: lifted %s after %d iterations, direct %s after %d; energies %.6f / %.6f, relative gap %.3g"
          % (out["result"]["result"], out["result"]["iters"], out["result_direct"]["result"], out["result_direct"]["iters"], e, e1, (e - e1) / abs(e1)))
    assert out["result"]["result"] == "Converged." and out["result_direct"]["result"] == "Converged."
    t = out["t"]
    assert t.size == nx * ny and np.isfinite(t).all()
    assert t.min() >= ex.LEFT - 1e-4 and t.max() <= ex.RIGHT + 1e-4
    assert e >= e1 - 1e-6 * abs(e1), (e, e1)                        # 1e-6: the tolerances of ex.options, which the direct solve stops at
