"""tests/epi_conjquad_reference.py against cases built from their answers (no GPU, no library).

from_answer() picks a boundary point P of phi* and sets z0 = P + s n along the outward unit normal, in long double; the projection of
z0 is P by construction.  The fp64 run of project() has to return P within

    64 eps_64 max(1, |z0|_inf, |P|_inf)

per group: scales 1 and 1000, a in {0, 1e-6, 1, 1e3}, alpha = beta, infinite bounds, u0 = 0, points exactly on the boundary and
exactly on a normal line through P_a / P_b, and alpha < 0 < beta with a point high on the other side (the case the tangential test
alone gets wrong by the width of the epigraph).  Observed worst: 2.1 of the 64 (docs/rounds/r15.md)."""
import numpy as np
import pytest

import epi_conjquad_reference as R

EPS = np.finfo(np.float64).eps
FACTOR = 64


def _run(cs, **kw):
    info = {}
    y, t, region = R.project(cs["z0"][:, 0], cs["z0"][:, 1], cs["a"], cs["b"], cs["c"], cs["alpha"], cs["beta"], np.float64, info=info, **kw)
    return np.stack([y, t], axis=1), region, info


def _slope(cs, y):
    """|phi*'| near y, from above: the arc's slope clipped to [alpha, beta]"""
    with np.errstate(all="ignore"):
        arc = np.where(cs["a"] > 0, (y - cs["b"]) / (2 * cs["a"]), 0.0)
        ends = np.maximum(np.where(np.isfinite(cs["alpha"]), np.abs(cs["alpha"]), 0.0), np.where(np.isfinite(cs["beta"]), np.abs(cs["beta"]), 0.0))
    return np.maximum(np.abs(np.clip(arc, cs["alpha"], cs["beta"])), ends)


def _ratio(cs, z):
    scale = np.maximum(1.0, np.maximum(np.abs(cs["z0"]).max(axis=1), np.abs(cs["P"]).max(axis=1)))
    return np.abs(z - cs["P"]).max(axis=1) / (EPS * scale)


@pytest.mark.parametrize("scale", [1.0, 1000.0])
def test_random_cases_return_their_answer(scale):
    rng = np.random.default_rng(20 + int(scale))
    cs = R.random_cases(rng, 6000, scale)
    assert set(np.unique(cs["a"])) == set(R.f32(R.A_VALUES))
    assert (cs["alpha"] == cs["beta"]).any() and np.isinf(cs["alpha"]).any() and np.isinf(cs["beta"]).any()
    z, region, info = _run(cs)
    r = _ratio(cs, z)
    print("scale %g: worst error %.2f eps, most steps %d" % (scale, r.max(), info["steps"].max()))
    assert not info["capped"].any()
    assert (r <= FACTOR).all(), (int(np.argmax(r)), r.max())
    # the designed region is the one the algorithm finds (off the seams between regions), and every region has its share
    assert (region == cs["region"]).mean() >= 0.99
    share = np.bincount(region, minlength=5) / region.size
    assert min(share[R.INSIDE], share[R.LEFT], share[R.RIGHT], share[R.ARC]) >= 0.15 and share[R.VERTEX] >= 0.05, share
    # inside comes back bit for bit
    assert np.array_equal(z[region == R.INSIDE], cs["z0"][region == R.INSIDE])
    # P is feasible and phi* has slopes within [alpha, beta]: a point within r of P is outside by (1 + |slope|) r at most
    scale = np.maximum(1.0, np.maximum(np.abs(cs["z0"]).max(axis=1), np.abs(cs["P"]).max(axis=1)))
    out = R.outside(z[:, 0], z[:, 1], cs["a"], cs["b"], cs["c"], cs["alpha"], cs["beta"])
    assert (out <= (1 + _slope(cs, z[:, 0])) * FACTOR * EPS * scale).all(), float((out / scale / EPS).max())


@pytest.mark.parametrize("scale", [1.0, 1000.0])
def test_directed_cases_return_their_answer(scale):
    cases = R.directed_cases(scale)
    assert {"alpha_eq_beta", "both_infinite", "left_infinite", "right_infinite", "below_the_apex", "on_the_boundary", "normal_through_contact",
            "vertex_cone", "high_on_the_other_side"} <= set(cases)
    for name, cs in cases.items():
        z, region, info = _run(cs)
        r = _ratio(cs, z)
        print("%s scale %g: worst error %.2f eps, regions %s" % (name, scale, r.max(), region))
        assert not info["capped"].any(), name
        assert (r <= FACTOR).all(), (name, int(np.argmax(r)), r.max())
    assert (cases["below_the_apex"]["z0"][:, 0] == cases["below_the_apex"]["b"]).all()                 # u0 == 0 exactly


def test_a_point_high_on_the_other_side_stays_on_its_own_ray():
    """a = 1, b = c = 0, alpha = -2, beta = 3: z0 far up on the right lies below the right ray and on the left ray's side of the normal
    through P_a; the answer is on the right ray"""
    cs = R.directed_cases(1.0)["high_on_the_other_side"]
    y0, t0 = cs["z0"][0]
    ya, fa = 2 * 1 * -2.0, 4.0
    assert (y0 - ya) + -2.0 * (t0 - (-2.0 * ya - fa)) <= 0 and t0 < 3 * y0 - 9 and not t0 < -2 * y0 - fa
    z, region, _ = _run(cs)
    assert list(region) == [R.RIGHT, R.LEFT, R.RIGHT, R.LEFT]
    assert (_ratio(cs, z) <= FACTOR).all()


def test_infinite_bounds_agree_with_the_full_parabola_and_precisions_with_each_other():
    rng = np.random.default_rng(7)
    n = 500
    a, b, c = rng.choice([0.05, 1.0, 1e3], n), rng.standard_normal(n), rng.standard_normal(n)       # (the check below divides by a)
    z0 = 10 * rng.standard_normal((n, 2))
    y, t, region = R.project(z0[:, 0], z0[:, 1], a, b, c, -np.inf, np.inf)
    assert set(region) <= {R.INSIDE, R.ARC}
    # stationarity of the distance on the parabola: (z0 - z) is parallel to the normal (slope, -1) for the arc groups
    arc = region == R.ARC
    slope = (y - b) / (2 * a)
    cross = (z0[:, 0] - y) + slope * (z0[:, 1] - t)
    size = np.abs(z0[:, 0] - y) + np.abs(slope * (z0[:, 1] - t)) + 1e-300
    scale = np.maximum(1.0, np.maximum(np.abs(z0).max(axis=1), np.maximum(np.abs(y), np.abs(t))))      # t carries FACTOR eps scale, times the slope
    assert (np.abs(cross[arc]) <= (1e-9 * size + FACTOR * EPS * (1 + np.abs(slope)) * scale)[arc]).all()
    # the same routine in fp32 and long double stays near the fp64 run
    for dtype, tol in ((np.float32, 64 * np.finfo(np.float32).eps), (np.longdouble, 64 * EPS)):
        z32 = R.f32(z0)
        yy, tt, _ = R.project(z32[:, 0], z32[:, 1], R.f32(a), R.f32(b), R.f32(c), -np.inf, np.inf, dtype)
        y64, t64, _ = R.project(z32[:, 0], z32[:, 1], R.f32(a), R.f32(b), R.f32(c), -np.inf, np.inf)
        scale = np.maximum(1.0, np.abs(z32).max(axis=1))
        assert (np.maximum(np.abs(yy - y64), np.abs(tt - t64)) <= tol * np.maximum(scale, np.maximum(np.abs(y64), np.abs(t64)))).all()


def test_the_cap_writes_the_feasible_point_and_counts():
    cs = R.directed_cases(1.0)["both_infinite"]
    z, region, info = _run(cs, cap=0)
    assert info["capped"].all() and (region == R.ARC).all()
    assert np.array_equal(z[:, 0], cs["z0"][:, 0])
    assert np.allclose(z[:, 1], R.conj(cs["z0"][:, 0], cs["a"], cs["b"], cs["c"], cs["alpha"], cs["beta"]), rtol=1e-15)
