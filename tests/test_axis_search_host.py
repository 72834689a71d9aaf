"""The host side of the axis search (paris_hip_axis_search_check / _plan, paris_hip_axis_estimate_from_costs; DESIGN.md section
4.15): no device, no ctx -- the band, the plan and the estimate against the numpy restatement (tests/axis_rule.py) bit for bit, the
refusals one per clause, and the recovery of a known offset from analytic fan-beam sinograms by the rule alone."""
import ctypes as C

import numpy as np
import pytest

import axis_rule as A
from paris_amd import _lib
from paris_amd import backend as B

INV, UNS = _lib.ERROR_INVALID_ARGUMENT, _lib.ERROR_UNSUPPORTED


def geometry(n_row=96, n_col=8, l_px_row=A.L_PX, delta_t=0.0, d_so=A.D_SO, d_od=A.D_OD, delta_s=0.0):
    return B.DetectorGeometry(n_row, n_col, l_px_row, l_px_row, delta_s, delta_t, d_so, d_od, 3.75)


def status(setting=(-8.0, 0.5, 33, 2, 0), det=None, n_frames=96):
    s = _lib.AxisSearch(*setting)
    return _lib.load().paris_hip_axis_search_check(C.byref(s), C.byref(det or geometry()), n_frames, None, None)


# ---- the check and the band -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_col", [7, 8, 9, 16, 64])
@pytest.mark.parametrize("delta_t", [0.0, 0.3, -0.5, 0.5, 1.75, -2.25, 40.0, -40.0])
@pytest.mark.parametrize("rows", [1, 2, 5, 7])
def test_row_first_equals_the_rule(n_col, delta_t, rows):
    """odd and even n_col, fractional delta_t, and offsets that push the band against either end"""
    first, nbytes = B.axis_search_check(-8.0, 0.5, 33, geometry(n_col=n_col, delta_t=delta_t), 96, rows=rows)
    assert first == A.row_first(n_col, delta_t, rows) and 0 <= first <= n_col - rows
    assert nbytes >= 4 * 96 * 96 + 16 * 33 * 96


def test_row_first_by_hand():
    assert B.axis_search_check(0, 1, 1, geometry(n_col=8), 4, rows=2)[0] == 3        # rows 3 and 4 straddle the centre 3.5
    assert B.axis_search_check(0, 1, 1, geometry(n_col=9), 4, rows=1)[0] == 4        # the centre row
    assert B.axis_search_check(0, 1, 1, geometry(n_col=9, delta_t=40.0), 4, rows=2)[0] == 7
    assert B.axis_search_check(0, 1, 1, geometry(n_col=9, delta_t=-40.0), 4, rows=2)[0] == 0


@pytest.mark.parametrize("what,kwargs", [
    ("count 0", dict(setting=(-8.0, 0.5, 0, 2, 0))),
    ("count 1025", dict(setting=(-8.0, 0.5, 1025, 2, 0))),
    ("step 0", dict(setting=(-8.0, 0.0, 33, 2, 0))),
    ("step negative", dict(setting=(-8.0, -0.5, 33, 2, 0))),
    ("step NaN", dict(setting=(-8.0, float("nan"), 33, 2, 0))),
    ("step Inf", dict(setting=(-8.0, float("inf"), 33, 2, 0))),
    ("lo NaN", dict(setting=(float("nan"), 0.5, 33, 2, 0))),
    ("rows 0", dict(setting=(-8.0, 0.5, 33, 0, 0))),
    ("rows 65", dict(setting=(-8.0, 0.5, 33, 65, 0), det=geometry(n_col=128))),
    ("rows above n_col", dict(setting=(-8.0, 0.5, 33, 9, 0))),
    ("3 frames", dict(n_frames=3)),
    ("no columns", dict(det=geometry(n_row=0))),
    ("no rows", dict(det=geometry(n_col=0))),
    ("pixel size 0", dict(det=geometry(l_px_row=0.0))),
    ("pixel size NaN", dict(det=geometry(l_px_row=float("nan")))),
    ("no source distance", dict(det=geometry(d_so=0.0, d_od=0.0))),
    ("delta_t NaN", dict(det=geometry(delta_t=float("nan")))),
])
def test_check_refusals(what, kwargs):
    assert status(**kwargs) == INV, what


def test_check_limits():
    assert status(setting=(-8.0, 0.5, 1, 1, 0), n_frames=4) == _lib.SUCCESS
    assert status(setting=(-8.0, 0.5, 1024, 64, 0), det=geometry(n_col=64)) == _lib.SUCCESS
    assert status(setting=(-8.0, 0.5, 1024, 2, 0), det=geometry(n_row=1 << 22)) == UNS          # n_row count = 2^32
    assert status(setting=(-8.0, 0.5, 1023, 2, 0), det=geometry(n_row=1 << 22)) == _lib.SUCCESS
    assert status(det=geometry(n_row=1 << 16), n_frames=1 << 16) == UNS                          # N n_row = 2^32
    assert status(det=geometry(n_row=1 << 16), n_frames=(1 << 16) - 1) == _lib.SUCCESS
    L, s, det = _lib.load(), _lib.AxisSearch(-8.0, 0.5, 33, 2, 0), geometry()
    first, nbytes = C.c_uint32(77), C.c_size_t(77)
    assert L.paris_hip_axis_search_check(None, C.byref(det), 96, C.byref(first), C.byref(nbytes)) == INV
    assert L.paris_hip_axis_search_check(C.byref(s), None, 96, C.byref(first), C.byref(nbytes)) == INV
    assert (first.value, nbytes.value) == (77, 77)                                               # nothing written


# ---- the plan ---------------------------------------------------------------------------------------------------------------------------

def assert_plan_equals_rule(lo, step, count, n, n_frames, k, **geo):
    det = geometry(n_row=n, **geo)
    got = B.axis_search_plan(lo, step, count, det, n_frames, k)
    c = A.candidates(lo, step, count)[k]
    i0, k0, wi, wf = A.plan(c, n, n_frames, det.l_px_row, det.d_so, det.d_od)
    assert np.array_equal(got["i0"], i0) and np.array_equal(got["k0"], k0), (n, c)
    assert np.array_equal(got["wi"].view(np.int32), wi.view(np.int32)) and np.array_equal(got["wf"].view(np.int32), wf.view(np.int32)), (n, c)
    assert np.all(got["k0"] < n_frames) and np.all((got["i0"] == -1) | ((got["i0"] >= 0) & (got["i0"] <= n - 2)))
    return got


@pytest.mark.parametrize("n", [8, 37, 96])
@pytest.mark.parametrize("n_frames", [4, 90, 97])
def test_plan_equals_the_rule(n, n_frames):
    """candidates -3, -2.75 .. 3: negative, zero, half-integer, integer and quarter values"""
    valid = [np.count_nonzero(assert_plan_equals_rule(-3.0, 0.25, 25, n, n_frames, k)["i0"] >= 0) for k in range(25)]
    assert valid[12] == n - 1 and min(valid) >= n - 7            # c = 0: only column 0, whose conjugate is column n - 1 exactly, is invalid
    for k in (0, 7, 24):                                         # a short source distance: large fan angles
        assert_plan_equals_rule(-3.0, 0.25, 25, n, n_frames, k, d_so=30.0, d_od=20.0)


@pytest.mark.parametrize("n", [8, 37, 96])
def test_plan_at_the_ends_of_the_detector(n):
    """c = 0: ip = n - 1 - i is an integer; ip = n - 1 (column 0) has no right neighbour and is invalid, ip = 0 (column n - 1) is valid
    with wi = 0; c = 0.5: ip = n - i, columns 0 and 1 fall off; c = -0.5: ip = n - 2 - i, column n - 1 has ip = -1"""
    p = assert_plan_equals_rule(-0.5, 0.5, 3, n, 96, 1)
    assert p["i0"][0] == -1 and p["i0"][n - 1] == 0 and p["wi"][n - 1] == 0 and p["i0"][1] == n - 2
    p = assert_plan_equals_rule(-0.5, 0.5, 3, n, 96, 2)
    assert p["i0"][0] == -1 and p["i0"][1] == -1 and p["i0"][2] == n - 2 and p["i0"][n - 1] == 1
    p = assert_plan_equals_rule(-0.5, 0.5, 3, n, 96, 0)
    assert p["i0"][0] == n - 2 and p["i0"][n - 1] == -1 and p["i0"][n - 2] == 0
    q = assert_plan_equals_rule(0.0, 0.3, 2, n, 96, 1)           # a fractional candidate: wi = frac(0.6f)
    assert np.all(q["wi"][q["i0"] >= 0] == np.float32(2.0 * A.f32(0.3) - 0.0))
    mid = assert_plan_equals_rule(0.0, 1.0, 1, 96, 96, 0)
    assert mid["k0"][48] in (47, 48) and mid["k0"][1] < mid["k0"][95]   # the central ray's conjugate is half a turn away


@pytest.mark.parametrize("n", [8, 37, 96])
def test_candidates_without_a_valid_column(n):
    for lo in (-float(n), float(n), -n / 2.0, n / 2.0 + 0.25, 1e6, -1e30):
        p = assert_plan_equals_rule(lo, 1.0, 1, n, 96, 0)
        assert np.all(p["i0"] == -1) and not p["k0"].any() and not p["wi"].any() and not p["wf"].any()
    assert np.count_nonzero(assert_plan_equals_rule(-n / 2.0 + 0.5, 1.0, 1, n, 96, 0)["i0"] >= 0) == 1   # ip = -i: column 0 alone


def test_plan_refusals():
    L, s, det = _lib.load(), _lib.AxisSearch(-8.0, 0.5, 33, 2, 0), geometry()
    out = np.zeros(96, np.dtype([("i0", np.int32), ("k0", np.uint32), ("wi", np.float32), ("wf", np.float32)]))
    assert L.paris_hip_axis_search_plan(C.byref(s), C.byref(det), 96, 33, out.ctypes.data) == INV
    assert L.paris_hip_axis_search_plan(C.byref(s), C.byref(det), 96, 0, None) == INV
    assert L.paris_hip_axis_search_plan(C.byref(s), C.byref(det), 3, 0, out.ctypes.data) == INV
    assert L.paris_hip_axis_search_plan(None, C.byref(det), 96, 0, out.ctypes.data) == INV
    assert L.paris_hip_axis_search_plan(C.byref(s), C.byref(det), 96, 32, out.ctypes.data) == _lib.SUCCESS


# ---- the estimate ---------------------------------------------------------------------------------------------------------------------

INF = float("inf")


def assert_estimate_equals_rule(lo, step, cost, columns=None):
    want = A.estimate(lo, step, cost)
    got = B.axis_estimate_from_costs(lo, step, cost, columns)
    assert np.float32(got.delta_s).view(np.int32) == np.float32(want["delta_s"]).view(np.int32)
    assert (got.best, got.scored, got.at_edge) == (want["best"], want["scored"], want["at_edge"])
    assert got.cost_min == want["cost_min"] and got.cost_median == want["cost_median"]
    assert (got.skipped, got.row_first) == (0, 0) and got.columns == (0 if columns is None else columns[got.best])
    return got


def test_estimate_parabola():
    r = assert_estimate_equals_rule(-1.0, 0.5, [9.0, 4.0, 1.0, 2.0, 7.0])
    assert r.best == 2 and r.at_edge == 0 and r.delta_s == np.float32(0.0 + 0.5 * (0.5 * (4.0 - 2.0) / 4.0)) and r.cost_median == 4.0
    rng = np.random.default_rng(5)
    for _ in range(50):
        n = int(rng.integers(3, 40))
        x = np.arange(n) - rng.uniform(0, n)
        assert_estimate_equals_rule(float(rng.uniform(-5, 5)), float(rng.choice([0.25, 0.3, 1.0])), x * x + rng.normal(0, 0.3, n) + 2,
                                    rng.integers(0, 90, n).astype(np.uint32))


def test_estimate_ties_go_to_the_lowest_index():
    r = assert_estimate_equals_rule(0.0, 1.0, [5.0, 1.0, 1.0, 5.0])
    assert r.best == 1 and r.at_edge == 0 and r.delta_s == np.float32(1.5)       # q = 4, off = 2 / 4 clamped to 1/2
    r = assert_estimate_equals_rule(0.0, 1.0, [1.0, 1.0, 1.0])
    assert r.best == 0 and r.at_edge == 1


def test_estimate_minimum_at_either_end():
    r = assert_estimate_equals_rule(-2.0, 0.5, [1.0, 2.0, 3.0, 4.0])
    assert (r.best, r.at_edge, r.delta_s) == (0, 1, -2.0)
    r = assert_estimate_equals_rule(-2.0, 0.5, [4.0, 3.0, 2.0, 1.0])
    assert (r.best, r.at_edge, r.delta_s) == (3, 1, -0.5)
    r = assert_estimate_equals_rule(3.25, 0.5, [7.0])
    assert (r.best, r.at_edge, r.delta_s, r.scored, r.cost_median) == (0, 1, 3.25, 1, 7.0)


def test_estimate_beside_an_unscored_candidate():
    r = assert_estimate_equals_rule(0.0, 1.0, [INF, 1.0, 3.0, 9.0, INF])
    assert (r.best, r.at_edge, r.delta_s, r.scored) == (1, 1, 1.0, 3) and r.cost_median == 3.0
    r = assert_estimate_equals_rule(0.0, 1.0, [4.0, 1.0, INF, 0.5, INF, 9.0])
    assert (r.best, r.at_edge, r.delta_s, r.scored) == (3, 1, 3.0, 4) and r.cost_median == 1.0   # the lower median of 0.5 1 4 9
    r = assert_estimate_equals_rule(0.0, 1.0, [4.0, 1.0, float("nan"), 7.0])                     # a NaN cost counts as unscored
    assert (r.best, r.at_edge, r.scored) == (1, 1, 3)


def test_estimate_without_curvature():
    """at an interior minimum q = (J[m-1] - J[m]) + (J[m+1] - J[m]) is positive unless the arithmetic gives way: 2 J[m] overflows"""
    r = assert_estimate_equals_rule(0.0, 1.0, [2.0, 1.0, 1.0, 1.0, 2.0])      # m = 1: q = 2 - 2 + 1, off = 1/2
    assert (r.best, r.at_edge, r.delta_s) == (1, 0, 1.5)
    big = [1.5e308, 1e308, 1.5e308]
    assert not big[0] - 2.0 * big[1] + big[2] > 0                             # -inf
    r = assert_estimate_equals_rule(0.0, 1.0, big)
    assert (r.best, r.at_edge, r.delta_s) == (1, 1, 1.0)
    r = assert_estimate_equals_rule(0.0, 1.0, [0.0, 0.0, 0.0, 0.0])           # all equal: m = 0, an end
    assert (r.best, r.at_edge, r.cost_min) == (0, 1, 0.0)


def test_estimate_with_every_candidate_unscored():
    L = _lib.load()
    s, out = _lib.AxisSearch(0.0, 1.0, 3, 2, 0), _lib.AxisResult()
    cost = np.full(3, np.inf)
    out.scored = 9
    assert L.paris_hip_axis_estimate_from_costs(C.byref(s), cost.ctypes.data, None, C.byref(out)) == INV and out.scored == 0
    assert A.estimate(0.0, 1.0, cost) is None
    with pytest.raises(B.ParisHipError):
        B.axis_estimate_from_costs(0.0, 1.0, [INF, float("nan")])


def test_estimate_refusals():
    L = _lib.load()
    out, cost = _lib.AxisResult(), np.ones(3)
    good = _lib.AxisSearch(0.0, 1.0, 3, 2, 0)
    assert L.paris_hip_axis_estimate_from_costs(None, cost.ctypes.data, None, C.byref(out)) == INV
    assert L.paris_hip_axis_estimate_from_costs(C.byref(good), None, None, C.byref(out)) == INV
    assert L.paris_hip_axis_estimate_from_costs(C.byref(good), cost.ctypes.data, None, None) == INV
    for bad in ((0.0, 1.0, 0), (0.0, 1.0, 1025), (0.0, 0.0, 3), (0.0, -1.0, 3), (float("nan"), 1.0, 3), (0.0, float("inf"), 3)):
        s = _lib.AxisSearch(bad[0], bad[1], bad[2], 2, 0)
        assert L.paris_hip_axis_estimate_from_costs(C.byref(s), cost.ctypes.data, None, C.byref(out)) == INV, bad
    assert L.paris_hip_axis_estimate_from_costs(C.byref(_lib.AxisSearch(0.0, 1.0, 3, 0, 0)), cost.ctypes.data, None, C.byref(out)) == _lib.SUCCESS  # rows is not read
    with pytest.raises(ValueError):
        B.axis_estimate_from_costs(0.0, 1.0, np.ones((2, 2)))
    with pytest.raises(ValueError):
        B.axis_estimate_from_costs(0.0, 1.0, np.ones(3), np.ones(2, np.uint32))


# ---- recovery on the rule alone -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_frames,n,true", [(96, 96, 2.4), (90, 64, 1.6)])
def test_the_rule_recovers_the_offset_of_an_analytic_sinogram(n_frames, n, true):
    """candidates -8 .. 8 at step 0.5; the float64 prototype's error was 0.026 px for the first case and 0.032 px at worst: the bound is
    three times that"""
    s = A.disc_sinogram(n_frames, n, true).astype(np.float32)
    est, cost = A.recover(s, -8.0, 0.5, 33)
    print("axis rule: N = %d, n = %d, true %.2f, estimate %.4f, J_min / J_median %.2g" % (n_frames, n, true, est["delta_s"], est["cost_min"] / est["cost_median"]))
    assert est["at_edge"] == 0 and est["scored"] == 33
    assert abs(float(est["delta_s"]) - true) <= A.BOUND_PX
    lib = B.axis_estimate_from_costs(-8.0, 0.5, cost)          # the library's estimate from the rule's costs
    assert lib.delta_s == est["delta_s"]
