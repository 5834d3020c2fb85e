"""The two NumPy references of ind_epi_polyhedral against each other (tests/epi_polyhedral_reference.py): the active-set projection
in fp64 -- the algorithm of include/prost/prox/epi_polyhedral.hpp, the truth of the GPU tests -- has to equal the KKT enumeration
within 64 eps_64 max(1, |z0|_inf, |b|_inf) on dim 2 .. 4, random lists (m <= 25, m <= 12 at dim 4) and the directed cases, and
must never come near its step cap."""
import numpy as np
import pytest

import epi_polyhedral_reference as R

EPS = np.finfo(np.float64).eps


directed_cases = R.directed_cases


def _check(z0, a, b, info_out=None):
    P, dim = z0.shape
    m = b.size
    info = {}
    z = R.project_active_set(z0, a, b, np.full(P, m), np.zeros(P, int), np.float64, info)
    bf = np.array([R.project_bruteforce(z0[i], a, b) for i in range(P)])
    scale = np.maximum(1.0, np.maximum(np.abs(z0).max(axis=1), np.abs(b).max() if m else 0.0))
    err = np.abs(z - bf).max(axis=1) / scale
    assert not info["capped"].any()
    assert info["steps"].max() < 10 * (m + dim), info["steps"].max()
    assert err.max() <= 64 * EPS, (err.max() / EPS, int(np.argmax(err)))
    return info["steps"].max()


@pytest.mark.parametrize("dim", [2, 3, 4])
def test_active_set_equals_enumeration_on_random_lists(dim):
    rng = np.random.default_rng(100 + dim)
    worst = 0
    for m in (1, 2, 3, 7, 12) + ((25,) if dim < 4 else ()):
        for scale in (1.0, 1000.0):
            for rep in range(2):
                a = rng.standard_normal((m, dim - 1))
                b = rng.standard_normal(m)
                worst = max(worst, _check(scale * rng.standard_normal((12, dim)), a, b))
    print("dim %d: at most %d steps" % (dim, worst))


@pytest.mark.parametrize("dim", [2, 3, 4])
def test_active_set_equals_enumeration_on_the_directed_cases(dim):
    for name, (a, b, pts) in directed_cases(dim).items():
        steps = _check(pts, a, b)
        print("dim %d %s: at most %d steps" % (dim, name, steps))


@pytest.mark.parametrize("dim", [2, 3, 4])
def test_apex_edge_and_feasible_points(dim):
    d = dim - 1
    cases = directed_cases(dim)
    for name in ("linf_pyramid", "l1_pyramid"):
        a, b, pts = cases[name]
        z = R.project_active_set(pts[:8], a, b, np.full(8, b.size), np.zeros(8, int))
        assert np.abs(z).max() <= 64 * EPS * np.abs(pts[:8]).max(), name             # the polar cone projects onto the apex
    # feasible points come back bit for bit, k = 0 is the identity
    a, b, pts = cases["linf_pyramid"]
    feas = pts.copy()
    for T in (np.float32, np.float64):
        f = feas.astype(T)
        f[:, -1] = np.abs(f[:, :d]).max(axis=1) + np.array([0.0, 1.0] * (len(pts) // 2)).astype(T)      # on the boundary and inside
        assert np.array_equal(R.project_active_set(f, a, b, np.full(len(f), b.size), np.zeros(len(f), int), T), f)
        assert np.array_equal(R.project_active_set(f, a, b, np.zeros(len(f), int), np.zeros(len(f), int), T), f)


def test_mixed_counts_shared_and_shuffled_lists_agree_group_by_group():
    rng = np.random.default_rng(9)
    for shared, shuffle in ((False, False), (True, False), (False, True)):
        a, b, cnt, idx = R.random_lists(rng, 23, 3, [0, 1, 2, 7, 8, 9, 25], shared=shared, shuffle=shuffle)
        assert (idx + cnt).max() <= b.size and (shuffle is False or (np.diff(idx) < 0).any())
        z0 = 10 * rng.standard_normal((23, 3))
        z = R.project_active_set(z0, a, b, cnt, idx)
        for g in range(23):
            bf = R.project_bruteforce(z0[g], a[idx[g]:idx[g] + cnt[g]], b[idx[g]:idx[g] + cnt[g]])
            assert np.abs(z[g] - bf).max() <= 64 * EPS * max(1.0, np.abs(z0[g]).max(), np.abs(b).max()), g
        assert (R.halfspace_distance(z, a, b, cnt, idx) <= 64 * EPS * 40).all()
