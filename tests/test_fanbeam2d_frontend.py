"""prost.block.fanbeam2d without a GPU: the builder, the registry name, the creation errors, the preconditioners, the entry points --
and the definition itself, on the references of tests/fanbeam2d_reference.py.

  * the builder describes { 'fanbeam2d', row, col, { nx, ny, L, angles, source_distance, detector_distance, ndet, spacing, shift,
    detector } } with its sizes and the default detector length, and refuses bad arguments with ValueError: a half fan above 30
    degrees, a source inside the circumscribed circle, a margin over the cap, an unknown detector, non-finite numbers, the size limits;
  * the name is registered for both precisions; every refusal of the factory, by its message, through prost.problem_info;
  * the two products of the restatement are transposes of each other, exactly: the gather enumeration (a candidate window per pixel and
    view) visits the entries of the ray enumeration, all of them and no other, with the same bits, at every pixel of every case -- the
    window is never too small -- and <K u, v> accumulated entry by entry with math.fsum is the same number from either list;
  * restatement (b) against matrix (a) in both directions within 1.01 (t + 1) u (|K| |x|); the accumulating form adds res0 last;
  * the parallel limit and the accuracy against the analytic chords of a disc (the two tests state their tolerances);
  * the fit of atan the inverse map of a curved detector uses, against libm;
  * the preconditioners of a problem with the block within (t + 8) eps_T of (c);
  * include/prost_hip.h declares the two entry points, the kernel library exports them, they refuse bad arguments without a device, the
    ABI version is still 10.
"""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import fanbeam2d_reference as F
import radon2d_reference as R
import prost_amd as prost
from prost_amd import _hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRECISIONS = [("single", np.float32), ("double", np.float64)]


def test_builder_cells_sizes_and_default_detector():
    angles = [0.0, 0.5, 1.0]
    (name, row, col, data), sz = prost.block.fanbeam2d(6, 5, 2, angles, 12.0)(3, 7, 0, 0)
    assert (name, row, col) == ("fanbeam2d", 3, 7)
    hd = math.hypot(6, 5) / 2
    ndet = 2 * math.ceil(12.0 * math.tan(math.asin(hd / 12.0))) + 1
    assert ndet == 11 and prost.block.fanbeam2d_ndet(6, 5, 12.0) == 11 and prost.block.fanbeam2d_ndet(6, 5, 12.0, 12.0, 1.0, "flat") == 11
    assert data[:3] == [6, 5, 2] and [type(v) for v in data[:3]] == [int, int, int]
    assert data[3].dtype == np.float64 and data[3].ndim == 1 and np.array_equal(data[3], angles)
    assert data[4:] == [12.0, 12.0, 11, 1.0, 0.0, "flat"] and [type(v) for v in data[4:]] == [float, float, int, float, float, str]
    assert sz == [2 * 3 * 11, 2 * 5 * 6]
    (_, _, _, data), sz = prost.block.fanbeam2d(np.int64(7), 10.0, 1, np.array([0.25]), 30, detector_distance=45.0, ndet=np.int32(4), spacing=2.5, shift=-0.3,
                                                detector="curved")(0, 0, 0, 0)
    assert data[:3] == [7, 10, 1] and data[4:] == [30.0, 45.0, 4, 2.5, -0.3, "curved"] and sz == [4, 70]
    assert prost.block.fanbeam2d(1, 1, 1, 0.0, 2.0)(0, 0, 0, 0)[1] == [3, 1]                # a single view as a scalar
    for nx, ny, dist, scale, h, det in ((1, 1, 2.0, 1.0, 1.0, "flat"), (5, 5, 9.0, 1.0, 0.5, "curved"), (131, 150, 400.0, 1.5, 1.0, "flat"), (7, 10, 20.0, 2.0, 2.5, "curved"),
                                        (8192, 8192, 20000.0, 1.0, 8.0, "flat")):
        ndet = prost.block.fanbeam2d_ndet(nx, ny, dist, scale * dist, h, det)
        assert ndet == F.default_ndet(nx, ny, dist, scale * dist, h, det == "curved") and ndet % 2 == 1
        # the outermost ray passes outside the circumscribed circle, the one of a detector two bins shorter does not
        for count, outside in ((ndet, True), (ndet - 2, False)):
            gamma = F.bin_angle(count - 1, count, scale * dist, h, 0.0, det == "curved")
            assert (dist * math.sin(gamma) >= math.hypot(nx, ny) / 2 * (1 - 1e-12)) == outside, (nx, ny, count)
    held = np.array([0.0, 1.0])
    bf = prost.block.fanbeam2d(4, 4, 1, held, 9.0)
    held[0] = 99.0                                           # the builder holds its own copy
    assert bf(0, 0, 0, 0)[0][3][3][0] == 0.0


def test_builder_value_errors():
    a = [0.0, 1.0]
    for args, kwargs, message in (((4.5, 4, 1, a, 9.0), {}, "nx = 4.5 is not an integer"), ((4, np.inf, 1, a, 9.0), {}, "not an integer"), ((4, 4, np.nan, a, 9.0), {}, "not an integer"),
                                  ((4, 4, True, a, 9.0), {}, "not an integer"), ((0, 4, 1, a, 9.0), {}, "at least 1"), ((4, 4, 0, a, 9.0), {}, "at least 1"),
                                  ((8193, 4, 1, a, 9000.0), {}, "nx = 8193 has to be at most 8192"), ((4, 8193, 1, a, 9000.0), {}, "ny = 8193 has to be at most 8192"),
                                  ((4, 4, 1, a, 9.0), {"ndet": 0}, "ndet = 0 has to be at least 1"), ((4, 4, 1, a, 9.0), {"ndet": 2.5}, "ndet = 2.5 is not an integer"),
                                  ((4, 4, 1, [], 9.0), {}, "non-empty vector"), ((4, 4, 1, np.zeros((2, 2)), 9.0), {}, "non-empty vector"),
                                  ((4, 4, 1, ["a"], 9.0), {}, "vector of numbers"),
                                  ((4, 4, 1, np.zeros(4097), 9.0), {}, "4097 views, up to 4096"),
                                  ((4, 4, 1, [0.0, np.nan], 9.0), {}, "non-finite"), ((4, 4, 1, [np.inf], 9.0), {}, "non-finite"),
                                  ((4, 4, 1, a, 9.0), {"spacing": 0.49}, "spacing = 0.49 has to be from 0.5 to 8"), ((4, 4, 1, a, 9.0), {"spacing": 8.5}, "from 0.5 to 8"),
                                  ((4, 4, 1, a, 9.0), {"spacing": np.nan}, "from 0.5 to 8"), ((4, 4, 1, a, 9.0), {"spacing": "1"}, "spacing = '1' is not a number"),
                                  ((4, 4, 1, a, 9.0), {"shift": np.inf}, "shift = inf has to be finite"), ((4, 4, 1, a, 9.0), {"shift": None}, "shift = None is not a number"),
                                  ((4, 4, 1, a, np.inf), {}, "source_distance = inf has to be positive and finite"), ((4, 4, 1, a, np.nan), {}, "source_distance = nan"),
                                  ((4, 4, 1, a, -3.0), {}, "source_distance = -3.0 has to be positive"), ((4, 4, 1, a, "9"), {}, "source_distance = '9' is not a number"),
                                  ((4, 4, 1, a, 9.0), {"detector_distance": 0.0}, "detector_distance = 0.0 has to be positive and finite"),
                                  ((4, 4, 1, a, 9.0), {"detector_distance": np.inf}, "detector_distance = inf"),
                                  ((4, 4, 1, a, 9.0), {"detector": "ring"}, "unknown detector 'ring' \\(flat or curved\\)"), ((4, 4, 1, a, 9.0), {"detector": 1}, "unknown detector 1"),
                                  # the source: hypot(4, 4) / 2 + 1 = 3.828..
                                  ((4, 4, 1, a, 3.8), {"ndet": 1}, "source_distance = 3.8 puts the source inside the image's circumscribed circle or less than a pixel off it"),
                                  ((4, 4, 1, a, 2.0), {"ndet": 1}, "it has to be at least 3.828"),
                                  # the half fan: bin 10 of 21 at u = 10 over D = 17 is atan(10 / 17) = 30.47 degrees, over 17.4 it is 29.89
                                  ((4, 4, 1, a, 17.0), {"ndet": 21}, "the outermost ray is 30.4655 degrees off the central ray; half fans up to 30 degrees"),
                                  ((4, 4, 1, a, 20.0), {"ndet": 21, "detector": "curved", "detector_distance": 19.0}, "the outermost ray is 30.1557 degrees"),
                                  ((4, 4, 1, a, 20.0), {"ndet": 3, "shift": 12.0}, "degrees off the central ray"),
                                  # the margin: D / (R - hc) / spacing = 8 / (4 - 2.12) / 0.5 = 8.5
                                  ((4, 4, 1, a, 4.0), {"ndet": 1, "spacing": 0.5, "detector_distance": 8.0}, "needs a margin of 9 bins, up to 5 are supported"),
                                  ((4, 4, 1, a, 4.0), {"ndet": 1, "spacing": 0.5, "detector_distance": 5.0}, "needs a margin of 6 bins"),
                                  ((4, 4, 1, a, 9.0), {"ndet": 2 ** 31 - 1024}, "below 2\\^31 - 1024"),
                                  ((4, 4, 1, a, 9.0), {"ndet": 2 ** 30}, "a sinogram of 2147483648 elements; it has to stay below 2\\^31")):
        with pytest.raises(ValueError, match=message):
            prost.block.fanbeam2d(*args, **kwargs)
    for args, kwargs, message in (((4, 4, 2.0), {}, "circumscribed circle"), ((4, 4, 9.0), {"spacing": 9}, "from 0.5 to 8"), ((4, 4, 9.0), {"detector": "x"}, "unknown detector"),
                                  ((0, 4, 9.0), {}, "at least 1"), ((4, 4, np.nan), {}, "positive and finite")):
        with pytest.raises(ValueError, match=message):
            prost.block.fanbeam2d_ndet(*args, **kwargs)
    prost.block.fanbeam2d(8192, 8192, 1, np.zeros(4096), 2.01 * math.hypot(8192, 8192) / 2, spacing=0.5)       # the default detector at R >= 2 hd, spacing 0.5
    prost.block.fanbeam2d(8192, 8192, 1, np.zeros(4096), 2.01 * math.hypot(8192, 8192) / 2, spacing=0.5, detector="curved")
    prost.block.fanbeam2d(4, 4, 1, a, 17.4, ndet=21)
    prost.block.fanbeam2d(4, 4, 1, a, 4.0, spacing=1.0, ndet=1)


def test_the_closest_source_of_the_cases_is_the_closest():
    """the builder accepts every case; where a case asks for the closest source, a source 1 / 16 pixel nearer is refused, and the case
    list holds every margin from 1 to the cap"""
    margins = set()
    for case in F.CASES:
        nx, ny, L, angles, dist, D, ndet, spacing, shift, detector = F.case_args(case)
        (_, _, _, data), sz = prost.block.fanbeam2d(nx, ny, L, angles, dist, D, ndet, spacing, shift, detector)(0, 0, 0, 0)
        assert sz == [L * len(angles) * ndet, L * nx * ny] and data[6] == ndet
        margins.add(F.case_margin(case))
        if case[7] == "closest":
            with pytest.raises(ValueError, match="circumscribed circle|degrees off|needs a margin"):
                prost.block.fanbeam2d(nx, ny, L, angles, dist - 1 / 16, case[9] * (dist - 1 / 16), ndet, spacing, shift, detector)
    assert margins == set(range(1, F.MAX_MARGIN + 1))
    assert F.case_margin(F.CASES[2]) == F.MAX_MARGIN and F.CASES[2][7] == "closest"          # the margin at its cap at the closest source


@pytest.mark.parametrize("precision", ["single", "double"])
def test_the_name_is_registered(precision):
    prost.set_precision(precision)
    try:
        assert "fanbeam2d" in prost.registered()["block"]
    finally:
        prost.set_precision("double")


def _raw_problem(data, nrows, ncols):
    x, z = prost.variable(ncols), prost.variable(nrows)
    prob = prost.min_max_problem([x], [z])
    prob.add_dual_pair(x, z, lambda row, col, nr, nc: [["fanbeam2d", row, col, data], [nrows, ncols]])
    return prob


@pytest.mark.parametrize("precision", ["single", "double"])
def test_every_refusal_of_the_factory_by_message(precision):
    a = np.array([0.0, 1.0])
    cases = [
        ([4.5, 4, 1, a, 9.0, 9.0, 7, 1.0, 0.0, "flat"], "BlockFanbeam2D: nx = 4.5 has to be an integer from 1 to 8192."),
        ([4, 0, 1, a, 9.0, 9.0, 7, 1.0, 0.0, "flat"], "BlockFanbeam2D: ny = 0 has to be an integer from 1 to 8192."),
        ([8193, 4, 1, a, 9.0, 9.0, 7, 1.0, 0.0, "flat"], "BlockFanbeam2D: nx = 8193 has to be an integer from 1 to 8192."),
        ([4, np.nan, 1, a, 9.0, 9.0, 7, 1.0, 0.0, "flat"], "BlockFanbeam2D: ny = nan has to be an integer from 1 to 8192."),
        ([4, 4, -1, a, 9.0, 9.0, 7, 1.0, 0.0, "flat"], "BlockFanbeam2D: L = -1 has to be a positive integer below 2^31."),
        ([4, 4, 1, np.zeros(0), 9.0, 9.0, 7, 1.0, 0.0, "flat"], "BlockFanbeam2D: the angles are empty."),
        ([4, 4, 1, np.zeros(4097), 9.0, 9.0, 7, 1.0, 0.0, "flat"], "BlockFanbeam2D: 4097 views, up to 4096 are supported."),
        ([4, 4, 1, np.array([0.0, np.inf]), 9.0, 9.0, 7, 1.0, 0.0, "flat"], "BlockFanbeam2D: the angles hold a non-finite value."),
        ([4, 4, 1, "angles", 9.0, 9.0, 7, 1.0, 0.0, "flat"], "BlockFanbeam2D: the angles have to be a full vector of type single or double."),
        ([4, 4, 1, a, 9.0, 9.0, 7, 1.0, 0.0, "ring"], "BlockFanbeam2D: unknown detector 'ring' (flat or curved)."),
        ([4, 4, 1, a, 9.0, 9.0, 7, 1.0, 0.0, 1.0], "BlockFanbeam2D: the detector has to be a string (flat or curved)."),
        ([4, 4, 1, a, 9.0, 9.0, 7, 0.25, 0.0, "flat"], "BlockFanbeam2D: spacing = 0.25 has to be from 0.5 to 8."),
        ([4, 4, 1, a, 9.0, 9.0, 7, np.nan, 0.0, "flat"], "BlockFanbeam2D: spacing = nan has to be from 0.5 to 8."),
        ([4, 4, 1, a, 9.0, 9.0, 7, 1.0, np.inf, "flat"], "BlockFanbeam2D: shift = inf has to be finite."),
        ([4, 4, 1, a, np.inf, 9.0, 7, 1.0, 0.0, "flat"], "BlockFanbeam2D: source_distance = inf has to be positive and finite."),
        ([4, 4, 1, a, -1.0, 9.0, 7, 1.0, 0.0, "flat"], "BlockFanbeam2D: source_distance = -1 has to be positive and finite."),
        ([4, 4, 1, a, 9.0, 0.0, 7, 1.0, 0.0, "flat"], "BlockFanbeam2D: detector_distance = 0 has to be positive and finite."),
        ([4, 4, 1, a, 9.0, np.nan, 7, 1.0, 0.0, "flat"], "BlockFanbeam2D: detector_distance = nan has to be positive and finite."),
        ([4, 4, 1, a, 9.0, 9.0, 0, 1.0, 0.0, "flat"], "BlockFanbeam2D: ndet = 0 has to be a positive integer below 2^31 - 1024."),
        ([4, 4, 1, a, 9.0, 9.0, 7.5, 1.0, 0.0, "flat"], "BlockFanbeam2D: ndet = 7.5 has to be a positive integer below 2^31 - 1024."),
        ([4, 4, 1, a, 9.0, 9.0, 2 ** 30, 1.0, 0.0, "flat"], "BlockFanbeam2D: a sinogram of 2.14748e+09 elements; it has to stay below 2^31."),
        ([4, 4, 1, a, 9.0, 9.0, 7, 1.0, 0.0, "flat", 14, 15], "BlockFanbeam2D: the declared size 14 x 15 is not L na ndet x L ny nx = 14 x 16."),
        ([4, 4, 1, a, 9.0, 9.0, 7, 1.0], "BlockFanbeam2D: the data cells are { nx, ny, L, angles, source_distance, detector_distance, ndet, spacing, shift, detector }"),
        ([4, 4, 1, a, 3.8, 3.8, 1, 1.0, 0.0, "flat"], "BlockFanbeam2D: source_distance = 3.8 puts the source inside the image's circumscribed circle or less than a pixel off it; "
                                                      "it has to be at least 3.82843."),
        ([4, 4, 1, a, 17.0, 17.0, 21, 1.0, 0.0, "flat"], "BlockFanbeam2D: the outermost ray is 30.4655 degrees off the central ray; half fans up to 30 degrees are supported."),
        ([4, 4, 1, a, 20.0, 19.0, 21, 1.0, 0.0, "curved"], "BlockFanbeam2D: the outermost ray is 30.1557 degrees off the central ray"),
        ([4, 4, 1, a, 4.0, 8.0, 1, 0.5, 0.0, "flat"], "BlockFanbeam2D: the candidate window of the adjoint needs a margin of 9 bins, up to 5 are supported"),
    ]
    prost.set_precision(precision)
    try:
        for data, message in cases:
            with pytest.raises(prost.ProstError, match=re.escape(message)) as err:
                prost.problem_info(_raw_problem(data, 14, 16))
            assert "Creating block with ID 'fanbeam2d' failed" in str(err.value)
        # what only the rounding to T refuses: a source so far away that fp32 cannot place the rays within a quarter of a bin
        far = [4, 4, 1, a, 2.0 ** 22, 2.0 ** 22, 7, 1.0, 0.0, "flat"]
        if precision == "single":
            with pytest.raises(prost.ProstError, match=re.escape("BlockFanbeam2D: source_distance = 4.1943e+06 is too far for the candidate window of the adjoint in single precision.")):
                prost.problem_info(_raw_problem(far, 14, 16))
        else:
            assert int(prost.problem_info(_raw_problem(far, 14, 16))["nrows"]) == 14
        for data, nrows in (([4, 4, 1, a, 9.0, 9.0, 7, 1.0, 0.0, "flat"], 14), ([4, 4, 1, a, 9.0, 9.0, 7, 1.0, 0.0, "curved", 14, 16], 14),
                            ([4, 4, 1, a, 9.0, 13.0, 1, 8.0, -0.3, "flat"], 2), ([4, 4, 1, 0.5, 9.0, 9.0, 7, 0.5, 0.0, "curved"], 7)):
            info = prost.problem_info(_raw_problem(data, nrows, 16))
            assert int(info["nrows"]) == nrows and int(info["ncols"]) == 16
    finally:
        prost.set_precision("double")


def test_table_values_at_the_axes_and_the_tie():
    """beta = 0: rows are marched, the source sits below the image at (cx, cy - R); pi / 2: columns, the source at (cx + R, cy); pi / 4:
    the tie goes to whichever of |cos|, |sin| libm makes larger.  The central bin of an odd detector has gamma = 0; on a flat detector
    at D = 100 the bin at u = 5 has tan gamma = 1 / 20, on a curved one gamma = 1 / 20."""
    views, bins, inv = F.tables(7, 5, [0.0, math.pi / 2, math.pi / 4], 100.0, 100.0, 11, 1.0, 0.0, "flat", np.float64)
    assert np.array_equal(views[0], [1.0, 0.0, 3.0, -98.0, 0.0])
    assert views[1][1] == 1.0 and views[1][2] == 103.0 and abs(views[1][3] - 2.0) < 1e-13 and views[1][4] == 1.0
    assert views[2][4] == (0.0 if abs(math.cos(math.pi / 4)) >= abs(math.sin(math.pi / 4)) else 1.0)
    assert np.array_equal(bins[5], [0.0, 1.0]) and abs(bins[10][0] / bins[10][1] - 0.05) < 1e-16
    assert np.array_equal(inv[:2], [5.0, 100.0]) and abs(inv[2] + 0.05) < 1e-16 and abs(inv[3] - 0.05) < 1e-16 and not inv[4:].any()
    _, bins, inv = F.tables(7, 5, [0.0], 100.0, 100.0, 11, 1.0, 0.0, "curved", np.float64)
    assert abs(bins[10][0] - math.sin(0.05)) < 1e-16 and abs(inv[3] - math.tan(0.05)) < 1e-16 and np.array_equal(inv[4:], F.ATAN)
    p, r, c, column = F.rays(views[0], bins, np.float64)
    assert not column and p[5] == 0.0 and r[5] == 3.0 and c[5] == 1.0          # the central ray at 0 runs along column cx


def test_the_fit_of_atan():
    """g(tau) = tau (1 + z (a_1 + z (a_2 + ..))) against libm on the whole admissible fan, |tau| <= tan 30 degrees"""
    tau = np.linspace(-math.tan(math.radians(30.0)), math.tan(math.radians(30.0)), 400001)
    z = tau * tau
    poly = np.full_like(z, F.ATAN[-1])
    for a in F.ATAN[-2::-1]:
        poly = poly * z + a
    worst = float(np.abs(tau + tau * (z * poly) - np.arctan(tau)).max())
    print("the fit of atan: largest error %.3g" % worst)
    assert worst <= F.ATAN_ERROR


@pytest.mark.parametrize("prec,dtype", PRECISIONS)
@pytest.mark.parametrize("case", F.CASES, ids=F.case_id)
def test_the_gather_visits_exactly_the_entries_of_the_rays(prec, dtype, case):
    """every pixel of the case: the candidate windows together hold each entry of the ray enumeration once, with its bits, and nothing
    else; inside a pixel the rows ascend.  So the two products of the restatement are the two sides of ONE matrix, and the inner
    product <K u, v>, accumulated entry by entry without rounding, is the same number from either enumeration."""
    nx, ny, L, angles, dist, D, ndet, spacing, shift, detector = F.case_args(case)
    rays = F.entries(nx, ny, angles, dist, D, ndet, spacing, shift, detector, dtype)
    gather = F.gathered(nx, ny, angles, dist, D, ndet, spacing, shift, detector, dtype)
    order = np.lexsort((rays[0], rays[1]))
    assert len(gather[0]) == len(rays[0]) > 0
    assert np.array_equal(gather[0], rays[0][order]) and np.array_equal(gather[1], rays[1][order])
    assert np.array_equal(gather[2].view(np.uint8), rays[2][order].view(np.uint8))
    key = gather[1].astype(np.int64) * (len(angles) * ndet) + gather[0]
    assert np.all(np.diff(key) > 0)                                             # pixels ascend, rows ascend inside a pixel, no entry twice
    per_pixel = np.bincount(gather[1], minlength=nx * ny)
    window = 2 * F.case_margin(case) + 2
    assert per_pixel.max() <= len(angles) * window
    if nx * ny * len(angles) * ndet <= 200000:
        rng = np.random.default_rng(F.case_seed(case, 7))
        u, v = rng.standard_normal(nx * ny).astype(dtype).astype(np.float64), rng.standard_normal(len(angles) * ndet).astype(dtype).astype(np.float64)
        from_rays = math.fsum((rays[2].astype(np.float64) * u[rays[1]] * v[rays[0]]).tolist())
        from_gather = math.fsum((gather[2].astype(np.float64) * u[gather[1]] * v[gather[0]]).tolist())
        assert from_rays == from_gather


@pytest.mark.parametrize("prec,dtype", PRECISIONS)
@pytest.mark.parametrize("case", F.CASES, ids=F.case_id)
def test_restatement_b_against_matrix_a_and_adjointness(prec, dtype, case):
    args = F.case_args(case)
    nx, ny, L = args[:3]
    rng = np.random.default_rng(F.case_seed(case))
    K = F.matrix(*args, dtype)
    assert K.shape == (L * len(args[3]) * args[6], L * nx * ny)
    x = rng.standard_normal(K.shape[1]).astype(dtype).astype(np.float64)
    y = rng.standard_normal(K.shape[0]).astype(dtype).astype(np.float64)
    kx_ = F.product(x, *args, False, dtype).astype(np.float64)
    kty = F.product(y, *args, True, dtype).astype(np.float64)
    bx, by = F.bound(*args, False, x, dtype), F.bound(*args, True, y, dtype)
    assert kx_.shape == (K.shape[0],) and kty.shape == (K.shape[1],)
    assert np.all(np.abs(kx_ - K @ x) <= bx), float((np.abs(kx_ - K @ x) / np.maximum(bx, 1e-300)).max())
    assert np.all(np.abs(kty - K.T @ y) <= by), float((np.abs(kty - K.T @ y) / np.maximum(by, 1e-300)).max())
    assert abs(kx_ @ y - x @ kty) <= bx @ np.abs(y) + by @ np.abs(x)
    res0 = rng.standard_normal(K.shape[0]).astype(dtype)
    assert np.array_equal(F.product(x, *args, False, dtype, res0), res0 + kx_.astype(dtype))
    res0 = rng.standard_normal(K.shape[1]).astype(dtype)
    assert np.array_equal(F.product(y, *args, True, dtype, res0), res0 + kty.astype(dtype))
    c_max = float(np.abs(K.data).max())
    assert c_max <= 1 / math.cos(math.radians(75.0)) * (1 + 1e-5)            # the per-view axis: no ray meets its driving lines beyond 75 degrees


def test_the_parallel_limit():
    """float64, flat, D = R = 2^20 hd: the projection of a random 12 x 9 image against the restatement of radon2d with the same bins.

    Tolerance, from the difference of the two geometries.  Ray (a, d) of the fan and of the parallel beam both pass through the point
    u_d e of the virtual detector; they enclose the angle gamma_d = atan(u_d / R) <= u_max / R.  A point of the image's neighbourhood is
    at most hd + 1 from the detector line, so there the two rays are at most dp = (hd + 1) u_max / R apart, and they cross a driving
    line, which they meet at 45 degrees at worst, at positions that differ by at most 1.5 dp.  The weights 1 / |cos(theta - gamma)| and
    1 / |cos theta|, |theta| <= 45 degrees, differ by at most sec tan gamma <= 1.5 u_max / R.  The linear interpolation of the image
    (0 outside) along a driving line has slope at most 2 max |u|.  So each of the nt <= max(nx, ny) terms (c w0 u0 + c w1 u1) changes
    by at most sqrt 2 * 2 max|u| * 1.5 dp + 1.5 (u_max / R) max|u|, and the projection by nt times that.  The roundings of float64,
    R eps = 1e-9 pixels, are three orders below it."""
    nx, ny, spacing, shift = 12, 9, 1.0, 0.25
    hd = F.half_diagonal(nx, ny)
    dist = 2.0 ** 20 * hd
    ndet = R.default_ndet(nx, ny, spacing)
    angles = R.angles_of("set+rand")
    image = np.random.default_rng(34).standard_normal(nx * ny)
    fan = F.product(image, nx, ny, 1, angles, dist, dist, ndet, spacing, shift, "flat", False, np.float64)
    par = R.product(image, nx, ny, 1, angles, ndet, spacing, shift, False, np.float64)
    u_max = (ndet - 1) / 2 * spacing + abs(shift)
    top = float(np.abs(image).max())
    tol = max(nx, ny) * top * (math.sqrt(2) * 2 * 1.5 * (hd + 1) + 1.5) * u_max / dist
    err = float(np.abs(fan - par).max())
    print("parallel limit: |fan - parallel| %.3g, tolerance %.3g, |parallel| %.3g" % (err, tol, float(np.abs(par).max())))
    assert fan.shape == par.shape and np.abs(par).max() > 1 and err <= tol
    assert tol < 1e-3 * np.abs(par).max()                                        # the tolerance resolves the operator: a wrong sign or axis shows


def chord(rho, radius):
    return 2 * np.sqrt(np.maximum(radius * radius - rho * rho, 0.0))


def test_accuracy_against_the_chords_of_a_disc():
    """float64, 64 x 64, a centred disc of radius 0.3 n sampled at the pixel centres, 24 views over a full turn, spacing 1, the
    default detectors, the source at 3 hd.  Ray (a, d) of the fan passes the centre at distance R |sin gamma_d|, ray d of the parallel
    beam at |s_d|; the line integral is the chord.  The RMS error over all rays of either fan is at most twice that of radon2d's
    restatement on the same disc at the same spacing: the outer rays of a fan meet their driving lines at up to 75 degrees under the
    per-view axis, where Joseph's interpolation is coarser.  Measured (docs/rounds/r34.md): the figures the test prints."""
    n, spacing = 64, 1.0
    radius = 0.3 * n
    yy, xx = np.mgrid[0:n, 0:n].astype(np.float64)
    disc = (((xx - (n - 1) / 2) ** 2 + (yy - (n - 1) / 2) ** 2) <= radius * radius).astype(np.float64).T.reshape(-1)      # y + x ny
    angles = np.arange(24) * (2 * math.pi / 24) + 0.1
    nd = R.default_ndet(n, n, spacing)
    par = R.product(disc, n, n, 1, angles, nd, spacing, 0.0, False, np.float64).reshape(len(angles), nd)
    s = (np.arange(nd) - (nd - 1) / 2) * spacing
    rms_par = float(np.sqrt(np.mean((par - chord(np.abs(s), radius)[None, :]) ** 2)))
    dist = 3 * F.half_diagonal(n, n)
    worst = 0.0
    for detector in ("flat", "curved"):
        ndet = F.default_ndet(n, n, dist, dist, spacing, detector == "curved")
        fan = F.product(disc, n, n, 1, angles, dist, dist, ndet, spacing, 0.0, detector, False, np.float64).reshape(len(angles), ndet)
        gamma = np.array([F.bin_angle(d, ndet, dist, spacing, 0.0, detector == "curved") for d in range(ndet)])
        rms_fan = float(np.sqrt(np.mean((fan - chord(dist * np.abs(np.sin(gamma)), radius)[None, :]) ** 2)))
        print("disc of radius %.1f at %d x %d: RMS error %s fan %.4f, parallel %.4f (ratio %.2f)" % (radius, n, n, detector, rms_fan, rms_par, rms_fan / rms_par))
        assert rms_fan <= 2 * rms_par, (detector, rms_fan, rms_par)
        worst = max(worst, rms_fan)
    assert 0 < rms_par < 1 and worst > 0


def fan_problem(args, alpha):
    """z = K x with only functions that take diagonal steps, so that no preconditioner entry is averaged over a group"""
    bf = prost.block.fanbeam2d(*args)
    nrows, ncols = bf(0, 0, 0, 0)[1]
    x, z = prost.variable(ncols), prost.variable(nrows)
    prob = prost.min_max_problem([x], [z])
    prob.add_function(x, prost.function.sum_1d("ind_box01"))
    prob.add_function(z, prost.function.sum_1d("ind_box01", 0.5, -0.5))
    prob.add_dual_pair(x, z, bf)
    prob.set_scaling_alpha(alpha)
    return prob


@pytest.mark.parametrize("precision,dtype", PRECISIONS)
@pytest.mark.parametrize("alpha", [1.0, 0.5])
@pytest.mark.parametrize("case", [c for c in F.CASES if c[0] * c[1] <= 1500], ids=F.case_id)
def test_preconditioners_within_the_bound_of_the_matrix_sums(precision, dtype, alpha, case):
    """Sigma = 1 / row sums of |K|^alpha, Tau = 1 / column sums of |K|^(2 - alpha): within (t + 8) eps_T of (c).  A row or column
    whose sum is exactly 0 repeats the preconditioner in front of it."""
    args = F.case_args(case)
    prost.set_precision(precision)
    try:
        info = prost.problem_info(fan_problem(args, alpha))
    finally:
        prost.set_precision("double")
    rows = F.sums(*args, alpha, dtype)[0]
    cols = F.sums(*args, 2.0 - alpha, dtype)[1]
    trow, tcol = F.terms(*args, dtype)
    got_left = np.asarray(info["scaling_left"], dtype=np.float64).ravel()
    got_right = np.asarray(info["scaling_right"], dtype=np.float64).ravel()
    carry = 1.0
    for got, want, t in ((got_left, rows, trow), (got_right, cols, tcol)):
        assert got.shape == want.shape
        live = want > 0
        tol = (t + 8) * np.finfo(dtype).eps
        assert np.all(np.abs(got[live] * want[live] - 1.0) <= tol[live]), float(np.abs(got[live] * want[live] - 1.0).max() / np.finfo(dtype).eps)
        before = np.concatenate([[carry], got[:-1]])
        assert np.array_equal(got[~live], before[~live])
        carry = got[-1]
    if case[4] == 63 and case[0] == 3:
        assert (rows == 0).any()              # the long detector has rays that miss the image


def _entry(dtype):
    fn = _hip.fn("fanbeam2d", dtype)
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    fn.restype = C.c_int
    return fn


def test_header_declares_and_library_exports_the_entry_points():
    text = open(os.path.join(ROOT, "include", "prost_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(prost_hip_[a-z0-9_]+)\s*\(", text))
    names = ["prost_hip_fanbeam2d_f32", "prost_hip_fanbeam2d_f64"]
    assert not [n for n in names if n not in declared]
    assert "prost_hip_fanbeam2d_geometry" in text
    Lb = _hip.lib()
    assert not [n for n in names if not hasattr(Lb, n)]
    assert Lb.prost_hip_abi_version() == 10


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_entry_points_refuse_bad_arguments_without_a_device(dtype):
    """every refusal comes before anything touches a device: the pointers are never followed"""
    fn = _entry(dtype)
    good = F.abi_records(4, 4, 1, [0.0, 1.0], 9.0, 9.0, 7, 1.0, 0.0, "flat", False)
    p = C.c_void_p(16)
    assert fn(None, None, None, None, 0, None) != 0
    assert b"null geometry" in _hip.lib().prost_hip_last_error()
    for table, res, rhs in ((None, p, p), (p, None, p), (p, p, None)):
        assert fn(good.ctypes.data_as(C.c_void_p), table, res, rhs, 0, None) != 0
        assert b"null pointer" in _hip.lib().prost_hip_last_error()
    for field, value, message in ((0, 0, b"nx and ny"), (1, 8193, b"nx and ny"), (0, -3, b"nx and ny"), (2, 0, b"bin count"), (2, 2 ** 31 - 1024, b"bin count"),
                                  (3, 0, b"view count"), (3, 4097, b"view count"), (4, 0, b"plane count"), (5, 0, b"margin"), (5, 6, b"margin"),
                                  (2, 2 ** 30, b"below 2^31 elements")):
        for transpose in (0, 1):
            bad = good.copy()
            bad[field] = value
            bad[6] = transpose
            assert fn(bad.ctypes.data_as(C.c_void_p), p, p, p, 0, None) != 0, (field, value)
            assert message in _hip.lib().prost_hip_last_error(), (field, value, _hip.lib().prost_hip_last_error())
