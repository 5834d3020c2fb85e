"""GPU tests of the dense blocks: dense, dense_kron_id, id_kron_dense through the product path (prost.eval_linop / prost.Solver ->
host C++ -> kernels_linop_dense.hip).

Bars:
  * Kronecker blocks: bit for bit against tests/dense_reference.py (the reference kernels' summation order restated in NumPy), value,
    transposed value and row / column sums; against the oracle's sparse twin where K is exact in float; and the reference tests' own
    1e-4 check against the explicit Kronecker product.
  * dense: |got - exact| <= 1.01 (L + 1) u (|A| |x| + |res0|) componentwise -- the forward error bound of a dot product of length L
    in any summation order plus the one add into the result (derived, not measured) -- and the same call twice gives the same bits.
  * complete PDHG iterations equal the oracle's on the sparse twin bit for bit; ADMM within the tolerance of
    test_gpu_solver.py::test_admm_matches_oracle.
"""
import numpy as np
import pytest
import scipy.sparse as sp

import dense_reference as ref
import oracle
import prost_amd as prost

pytestmark = pytest.mark.gpu
PRECISIONS = [("single", np.float32), ("double", np.float64)]

# kron(I_d, K) runs from LDS tiles while at least 4 groups of (inner | 1) + (rows | 1) elements fit kIdKronLdsBytes = 48 KiB
# (kernels_linop_dense.hip): up to 3072 elements per group in fp32, 1536 in fp64.  5 x 3100 is past both, in both directions.
FALLBACK_SHAPE = (5, 3100, 3)
assert (FALLBACK_SHAPE[0] | 1) + (FALLBACK_SHAPE[1] | 1) > 48 * 1024 // 4 // 4

# (m, n, d): the reference tests' own two; the smallest; d below one 16-byte access; a ragged last tile of 64 * 4 lanes-worth; more rows
# than one register tile (16) in either direction; the plain-kernel shape
KRON_SHAPES = [(13, 14, 122), (49, 83, 271), (1, 1, 1), (1, 7, 3), (7, 1, 3), (3, 3, 64 * 4 + 1), (70, 5, 130), (5, 70, 130), FALLBACK_SHAPE]


@pytest.fixture(autouse=True)
def _gpu(hip):
    prost.set_gpu(0)
    yield
    prost.set_precision("double")


def grid_matrix(m, n, seed):
    """zero-free, entries multiples of 1/64: exact in float, so a sparse twin's float storage loses nothing"""
    rng = np.random.default_rng(seed)
    return rng.integers(1, 129, size=(m, n)) * rng.choice([-1.0, 1.0], size=(m, n)) / 64.0


def four_copies(bf, m, n):
    """the reference tests' 2 x 2 arrangement (test_linop_sparse_kron_id.m): the first block of a range runs the non-accumulating
    kernel, the second the accumulating one, and the second row / column of blocks starts at an offset that is odd for odd sizes"""
    return [bf(0, 0, m, n)[0], bf(m, 0, m, n)[0], bf(m, n, m, n)[0], bf(0, n, m, n)[0]]


@pytest.mark.parametrize("prec,dtype", PRECISIONS)
@pytest.mark.parametrize("name", ["dense_kron_id", "id_kron_dense"])
@pytest.mark.parametrize("shape", KRON_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kronecker_blocks_bit_for_bit(prec, dtype, name, shape):
    prost.set_precision(prec)
    m, n, d = shape
    id_first = name == "id_kron_dense"
    rng = np.random.default_rng(m * 1000 + n * 10 + d)
    K = rng.standard_normal((m, n))                       # not float-representable: K must reach the device as T
    M, N = m * d, n * d
    linop = four_copies(getattr(prost.block, name)(K, d), M, N)
    inp, inp_t = rng.standard_normal(2 * N), rng.standard_normal(2 * M)
    x, rowsum, colsum, _ = prost.eval_linop(linop, inp, False)
    x_t = prost.eval_linop(linop, inp_t, True)[0]
    want = ref.arrangement_2x2(K, inp, d, id_first, False, dtype)
    want_t = ref.arrangement_2x2(K, inp_t, d, id_first, True, dtype)
    x, x_t = np.asarray(x, dtype=np.float64).ravel(), np.asarray(x_t, dtype=np.float64).ravel()
    assert np.array_equal(x, want.astype(np.float64)), float(np.abs(x - want).max())
    assert np.array_equal(x_t, want_t.astype(np.float64)), float(np.abs(x_t - want_t).max())
    rs, cs = ref.kron_sums(K, d, id_first, 1.0, dtype)
    rs, cs = (np.zeros_like(rs) + rs) + rs, (np.zeros_like(cs) + cs) + cs          # two blocks on every row and column, summed in T
    assert np.array_equal(np.asarray(rowsum, dtype=np.float64).ravel(), np.tile(rs, 2).astype(np.float64))
    assert np.array_equal(np.asarray(colsum, dtype=np.float64).ravel(), np.tile(cs, 2).astype(np.float64))
    if dtype == np.float32 and shape in KRON_SHAPES[:2]:
        # the reference tests' own check (test_linop_dense_kron_id.m / test_linop_id_kron_dense.m)
        full = ref.kron_full(K, d, id_first)
        Kf = sp.bmat([[full, full], [full, full]]).tocsr()
        assert np.abs(x - Kf @ inp).max() <= 1e-4 and np.abs(x_t - Kf.T @ inp_t).max() <= 1e-4
        assert np.abs(np.asarray(rowsum).ravel() - np.asarray(abs(Kf).sum(axis=1)).ravel()).max() <= 1e-4
        assert np.abs(np.asarray(colsum).ravel() - np.asarray(abs(Kf).sum(axis=0)).ravel()).max() <= 1e-4


@pytest.mark.parametrize("prec,dtype", PRECISIONS)
@pytest.mark.parametrize("name,twin", [("dense_kron_id", "sparse_kron_id"), ("id_kron_dense", "id_kron_sparse")])
def test_kronecker_blocks_equal_the_sparse_twin_in_the_oracle(prec, dtype, name, twin):
    prost.set_precision(prec)
    m, n, d = 13, 14, 122
    K = grid_matrix(m, n, 4)
    M, N = m * d, n * d
    rng = np.random.default_rng(9)
    inp, inp_t = rng.standard_normal(2 * N), rng.standard_normal(2 * M)
    linop = four_copies(getattr(prost.block, name)(K, d), M, N)
    linop_twin = four_copies(getattr(prost.block, twin)(sp.csc_matrix(K), d), M, N)
    x, rowsum, colsum, _ = prost.eval_linop(linop, inp, False)
    x_t = prost.eval_linop(linop, inp_t, True)[0]
    ox, orow, ocol = oracle.eval_linop(linop_twin, inp, False, dtype)[:3]
    ox_t = oracle.eval_linop(linop_twin, inp_t, True, dtype)[0]
    assert np.array_equal(np.asarray(x).ravel(), ox) and np.array_equal(np.asarray(x_t).ravel(), ox_t)
    assert np.array_equal(np.asarray(rowsum).ravel(), orow) and np.array_equal(np.asarray(colsum).ravel(), ocol)


@pytest.mark.parametrize("prec,dtype", PRECISIONS)
@pytest.mark.parametrize("shape", [(1, 1), (1, 300), (300, 1), (257, 129), (5000, 3), (3, 5000), (1024, 2048)], ids=lambda s: "x".join(map(str, s)))
def test_dense_block(prec, dtype, shape):
    """[A A] accumulates in the forward product (the second block adds onto the first), [A; A] in the adjoint; 1024 x 2048 splits the
    columns of the forward product (and the rows of the adjoint) over workgroups, the partial sums combined in a second pass"""
    prost.set_precision(prec)
    m, n = shape
    rng = np.random.default_rng(m + 7 * n)
    A = rng.standard_normal((m, n))
    bf = prost.block.dense(A)
    for linop, reps in (([bf(0, 0, m, n)[0], bf(0, n, m, n)[0]], (1, 2)), ([bf(0, 0, m, n)[0], bf(m, 0, m, n)[0]], (2, 1))):
        rows, cols = reps[0] * m, reps[1] * n
        inp, inp_t = rng.standard_normal(cols), rng.standard_normal(rows)
        for transpose, rhs in ((False, inp), (True, inp_t)):
            got, rowsum, colsum, _ = prost.eval_linop(linop, rhs, transpose)
            again = prost.eval_linop(linop, rhs, transpose)[0]
            got = np.asarray(got, dtype=np.float64).ravel()
            assert np.array_equal(got, np.asarray(again, dtype=np.float64).ravel())          # no atomics: the same bits every time
            parts = rhs.reshape(2, -1) if (reps == (1, 2)) != transpose else [rhs]
            e1, a1, fac = ref.dense_terms(A, parts[0], transpose, dtype)
            b1 = fac * a1                                                   # the first writer: res0 = 0
            if len(parts) == 2:        # both blocks write the same range: 0 + A x0, then that + A x1 (|res0| <= |A x0| + b1)
                e2, a2, _ = ref.dense_terms(A, parts[1], transpose, dtype)
                exact, bound = e1 + e2, b1 + fac * (a2 + np.abs(e1) + b1)
            else:                      # each block writes its own range from the same operand
                exact, bound = np.tile(e1, 2), np.tile(b1, 2)
            err = np.abs(got - exact)
            print("dense %s %s transpose=%d arrangement=%s: max err / bound = %.3g" % (prec, shape, transpose, reps, float((err / np.maximum(bound, 1e-300)).max())))
            assert np.all(err <= bound), float((err / np.maximum(bound, 1e-300)).max())
        # the sums are the reference's (block_dense.cu:57-74): formed in T in ascending index, then added over the blocks in T.  The NumPy
        # side forms them the same way (cumsum is a running sum in its dtype): a T sum of 5000 terms is itself up to ~5000 u from the fp64
        # sum, so fp64 could not be the yardstick of an rtol of 1e-6 in fp32 (measured at 5000 x 3 fp32: 2.0e-6 from the fp64 sum)
        P = np.abs(A.astype(dtype))
        rs, cs = np.cumsum(P, axis=1, dtype=dtype)[:, -1], np.cumsum(P, axis=0, dtype=dtype)[-1, :]
        rs = np.tile(rs, 2) if reps == (2, 1) else rs + rs
        cs = np.tile(cs, 2) if reps == (1, 2) else cs + cs
        assert np.allclose(np.asarray(rowsum).ravel(), rs.astype(np.float64), rtol=1e-6)
        assert np.allclose(np.asarray(colsum).ravel(), cs.astype(np.float64), rtol=1e-6)


# ---- complete iterations --------------------------------------------------------------------
NX, NY, L = 12, 10, 4
D = NX * NY


def iteration_problem(name, twin):
    """u: a 12 x 10 image with 4 channels; q = gradient2d u under norm2 / ind_leq0, r = B u under a quadratic, B = kron of a 4 x 4 K
    (zero-free, 1/64 grid) with the identity of the image; quadratic data term"""
    K = grid_matrix(L, L, 21)
    if twin:
        blk = getattr(prost.block, {"dense_kron_id": "sparse_kron_id", "id_kron_dense": "id_kron_sparse"}[name])(sp.csc_matrix(K), D)
    else:
        blk = getattr(prost.block, name)(K, D)
    n = D * L
    f = np.random.default_rng(5).random(n)
    u, q, r = prost.variable(n), prost.variable(2 * n), prost.variable(n)
    prob = prost.min_max_problem([u], [q, r])
    prob.add_function(u, prost.function.sum_1d("square", 1, f, 4.0))
    prob.add_function(q, prost.function.sum_norm2(2 * L, False, "ind_leq0", 1, 1, 1))
    prob.add_function(r, prost.function.sum_1d("square", 1, 0, 0.5))
    prob.add_dual_pair(u, q, prost.block.gradient2d(NX, NY, L))
    prob.add_dual_pair(u, r, blk)
    return prob


def run_both(name, backend, opts, iters, dtype):
    s = prost.Solver(iteration_problem(name, False), backend, opts)
    s.iterate(iters)
    st = s.state()
    s.destroy()
    twin = iteration_problem(name, True)
    twin.finalize()
    o = oracle.Solver(twin.data, twin.nrows, twin.ncols, backend, opts, dtype)
    o.initialize()
    o.iterate(iters)
    ost = o.state()
    ost.update(o.scalars())
    return st, ost


@pytest.mark.parametrize("prec,dtype", PRECISIONS)
@pytest.mark.parametrize("name", ["dense_kron_id", "id_kron_dense"])
def test_pdhg_iterates_equal_the_oracle_on_the_sparse_twin(prec, dtype, name):
    """alg1 step sizes: no reduction feeds back into the iterates, so every product and every preconditioner entry being the twin's
    makes the iterates the twin's, bit for bit"""
    prost.set_precision(prec)
    b = prost.backend.pdhg(stepsize="alg1", residual_iter=5)
    o = prost.options(max_iters=100, num_cback_calls=0, verbose=False)
    for k in (1, 2, 25):
        st, ost = run_both(name, b, o, k, dtype)
        assert st["path"] == "pdhg:generic"
        for v in "xyzw":
            assert np.array_equal(st[v], ost[v]), (k, v, float(np.abs(st[v] - ost[v]).max()))
        for s_ in ("tau", "sigma"):
            assert st[s_] == ost[s_], (k, s_)


@pytest.mark.parametrize("prec,dtype", PRECISIONS)
@pytest.mark.parametrize("name", ["dense_kron_id", "id_kron_dense"])
def test_admm_matches_the_oracle_on_the_sparse_twin(prec, dtype, name):
    """tolerance of tests/test_gpu_solver.py::test_admm_matches_oracle (generic operators behind LinearOperator::Eval): 2e-4 (fp32) /
    1e-9 (fp64) of max(1, |oracle|_inf) -- the CG step lengths come from reductions"""
    prost.set_precision(prec)
    b = prost.backend.admm(rho0=1, residual_iter=2)
    o = prost.options(max_iters=100, num_cback_calls=0, verbose=False)
    st, ost = run_both(name, b, o, 10, dtype)
    assert st["path"] == "admm:generic"
    tol = 2e-4 if dtype == np.float32 else 1e-9
    for v in "xyzw":
        scale = max(1.0, float(np.abs(ost[v]).max()))
        assert float(np.abs(st[v] - ost[v]).max()) <= tol * scale, (v, float(np.abs(st[v] - ost[v]).max()))
