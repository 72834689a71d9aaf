"""The host side of the detector roll (paris_hip_detector_roll_check / _host / _source_rows, paris_hip_roll_search_check,
paris_hip_roll_estimate_from_costs): no device, no ctx -- the pixel rule against the numpy restatement
(tests/roll_rule.py) bit for bit, the source rows of a band against brute force, the refusals, the estimate both searches share, and
the recovery of a known roll from analytic cone-beam frames by the rule alone."""
import ctypes as C

import numpy as np
import pytest

import axis_rule as A
import roll_rule as R
from paris_amd import _lib
from paris_amd import backend as B

INV = _lib.ERROR_INVALID_ARGUMENT
INF = float("inf")
GEO = B.DetectorGeometry(*R.HOST_GEO)
FRAME = R.special_frame()


# ---- the pixel rule ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("eta", R.HOST_ETAS)
def test_roll_host_equals_the_rule_bit_for_bit(eta):
    want = R.roll(FRAME, eta, R.HOST_GEO)
    got = B.detector_roll_host(eta, GEO, FRAME)
    R.assert_same(got, want, eta)
    assert np.isnan(want).any() and np.isinf(want).any() and np.isfinite(want).sum() > 0.9 * want.size
    assert not np.array_equal(R.bits(want), R.bits(FRAME))
    # the fp32 rule is the float64 rule up to the rounding of coordinates and taps
    clean = np.where(np.isfinite(FRAME), FRAME, np.float32(1.0))
    err = np.abs(B.detector_roll_host(eta, GEO, clean).astype(np.float64) - R.roll(clean, eta, R.HOST_GEO, np.float64))
    assert err.max() <= 2e-4 * np.abs(clean).max()   # 67 2^-24 (a coordinate's rounding) times the largest step between taps, with room


def test_the_rule_is_a_rotation_in_millimetres_about_the_axis_pixel():
    """a frame linear in the physical coordinates, p = u t + w v, comes out as the same plane rotated: the aspect ratio is honoured"""
    g, eta = R.HOST_GEO, 2.5
    t = ((np.arange(67) + 0.5) - 67 / 2.0 - R.f32(1.3)) * R.f32(0.2)
    v = ((np.arange(45) + 0.5) - 45 / 2.0 - R.f32(-0.7)) * R.f32(0.25)
    plane = lambda tt, vv: 3.0 * tt - 2.0 * vv
    src = plane(t[None, :], v[:, None])
    e = np.radians(eta)
    want = plane(np.cos(e) * t[None, :] - np.sin(e) * v[:, None], np.sin(e) * t[None, :] + np.cos(e) * v[:, None])
    got = R.roll(src, eta, g, np.float64)
    m = 4    # inside the replicated edge: 33 sin(2.5 deg) 1.25 + ... < 3
    assert np.abs(got - want)[m:-m, m:-m].max() <= 1e-12
    got32 = B.detector_roll_host(eta, GEO, src)
    assert np.abs(got32 - want)[m:-m, m:-m].max() <= 1e-5


def test_the_check_s_refusals():
    L = _lib.load()

    def status(eta, geo=R.HOST_GEO):
        return L.paris_hip_detector_roll_check(C.byref(_lib.DetectorRoll(eta)), C.byref(B.DetectorGeometry(*geo)))

    def with_field(k, v):
        g = list(R.HOST_GEO)
        g[k] = v
        return tuple(g)

    assert status(0.3) == status(-10.0) == status(10.0) == _lib.SUCCESS
    for eta in (0.0, -0.0, 10.001, -10.5, float("nan"), INF, -INF):
        assert status(eta) == INV, eta
    assert status(1.0, with_field(0, 1)) == INV and status(1.0, with_field(1, 1)) == INV and status(1.0, with_field(0, 0)) == INV
    assert status(1.0, with_field(0, 2)) == _lib.SUCCESS and status(1.0, with_field(1, 2)) == _lib.SUCCESS
    for k in (2, 3):
        for bad in (0.0, -0.2, float("nan"), INF):
            assert status(1.0, with_field(k, bad)) == INV, (k, bad)
    for k in (4, 5):
        for bad in (float("nan"), INF):
            assert status(1.0, with_field(k, bad)) == INV, (k, bad)
    assert L.paris_hip_detector_roll_check(None, C.byref(GEO)) == INV
    assert L.paris_hip_detector_roll_check(C.byref(_lib.DetectorRoll(1.0)), None) == INV
    out = np.zeros_like(FRAME)
    s = _lib.DetectorRoll(1.0)
    assert L.paris_hip_detector_roll_host(C.byref(s), C.byref(GEO), None, out.ctypes.data) == INV
    assert L.paris_hip_detector_roll_host(C.byref(s), C.byref(GEO), FRAME.ctypes.data, None) == INV
    assert L.paris_hip_detector_roll_host(C.byref(_lib.DetectorRoll(0.0)), C.byref(GEO), FRAME.ctypes.data, out.ctypes.data) == INV
    with pytest.raises(B.ParisHipError):
        B.detector_roll_check(0.0, GEO)
    with pytest.raises(ValueError):
        B.detector_roll_host(1.0, GEO, np.zeros((45, 66), np.float32))


# ---- the source rows of a band ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("eta", R.HOST_ETAS + (10.0, 5.0))
def test_source_rows_are_exact_for_bands_at_the_top_the_middle_and_the_bottom(eta):
    for first, count in ((0, 1), (0, 7), (1, 3), (19, 9), (22, 1), (38, 7), (44, 1), (0, 45)):
        got = B.detector_roll_source_rows(eta, GEO, first, count)
        assert got == R.source_rows(eta, R.HOST_GEO, first, count), (eta, first, count)
        assert got[0] + got[1] <= 45 and got[1] >= 2
    assert B.detector_roll_source_rows(eta, GEO, 45, 0) == (44, 0) and B.detector_roll_source_rows(eta, GEO, 7, 0) == (7, 0)


def test_source_rows_refusals():
    L = _lib.load()
    s, a, b = _lib.DetectorRoll(1.0), C.c_uint32(9), C.c_uint32(9)
    call = lambda st, g, first, count, pa, pb: L.paris_hip_detector_roll_source_rows(st, g, first, count, pa, pb)
    assert call(C.byref(s), C.byref(GEO), 40, 6, C.byref(a), C.byref(b)) == INV
    assert call(C.byref(s), C.byref(GEO), 46, 0, C.byref(a), C.byref(b)) == INV
    assert call(C.byref(s), C.byref(GEO), 2 ** 31, 2 ** 31, C.byref(a), C.byref(b)) == INV
    assert call(C.byref(s), C.byref(GEO), 0, 5, None, C.byref(b)) == INV and call(C.byref(s), C.byref(GEO), 0, 5, C.byref(a), None) == INV
    assert call(None, C.byref(GEO), 0, 5, C.byref(a), C.byref(b)) == INV and call(C.byref(s), None, 0, 5, C.byref(a), C.byref(b)) == INV
    assert call(C.byref(_lib.DetectorRoll(11.0)), C.byref(GEO), 0, 5, C.byref(a), C.byref(b)) == INV
    assert (a.value, b.value) == (9, 9)      # a refusal writes nothing


# ---- the search's check -----------------------------------------------------------------------------------------------------------

def test_search_check_reports_the_rule_s_margins():
    for lo, step, count in (R.SEARCH, (-10.0, 1.0, 21), (0.5, 0.5, 1), (0.0, 0.25, 5)):
        for g in (R.HOST_GEO, R.geo(), R.geo(delta_s=1.3)):
            mx, my, nbytes = B.roll_search_check(lo, step, count, B.DetectorGeometry(*g))
            assert (mx, my) == R.margins(lo, step, count, g), (lo, g)
            assert nbytes >= 2 * 4 * g[0] * g[1] + 8 * g[0] + 16 * count
    assert B.roll_search_check(0.0, 1.0, 1, GEO)[:2] == (1, 1)     # the identity alone: nothing moves


def test_search_check_refusals():
    L = _lib.load()

    def status(lo, step, count, geo=R.HOST_GEO):
        return L.paris_hip_roll_search_check(C.byref(_lib.RollSearch(lo, step, count, 0)), C.byref(B.DetectorGeometry(*geo)), None, None, None)

    assert status(*R.SEARCH) == _lib.SUCCESS and status(-8.0, 0.0625, 256) == _lib.SUCCESS
    assert status(-3.0, 0.25, 0) == INV and status(-3.0, 0.25, 257) == INV
    assert status(-3.0, 0.0, 5) == INV and status(-3.0, -1.0, 5) == INV and status(float("nan"), 1.0, 5) == INV and status(0.0, INF, 2) == INV
    assert status(-10.5, 1.0, 5) == INV and status(8.0, 1.0, 4) == INV          # a candidate beyond 10 degrees
    assert status(-1.0, 1.0, 3) == _lib.SUCCESS                                  # a candidate of exactly 0 is allowed
    assert status(-10.0, 1.0, 21, (4, 4, 1.0, 1.0, 0.0, 0.0, 100.0, 100.0, 4.0)) == INV   # the margins leave nothing to score
    assert L.paris_hip_roll_search_check(None, C.byref(GEO), None, None, None) == INV
    assert L.paris_hip_roll_search_check(C.byref(_lib.RollSearch(-3.0, 0.25, 25, 0)), None, None, None, None) == INV


# ---- the estimate: one implementation for both searches ---------------------------------------------------------------------------

def assert_estimate_equals_both(lo, step, cost):
    want = R.estimate(lo, step, cost)
    axis_rule = A.estimate(lo, step, cost)
    assert R.bits(want["value"]) == R.bits(axis_rule.pop("delta_s")) and axis_rule == {k: v for k, v in want.items() if k != "value"}
    got, axis = B.roll_estimate_from_costs(lo, step, cost), B.axis_estimate_from_costs(lo, step, cost)
    assert R.bits(got.eta_deg) == R.bits(want["value"]) == R.bits(axis.delta_s)
    for r in (got, axis):
        assert (r.best, r.scored, r.at_edge) == (want["best"], want["scored"], want["at_edge"])
        assert r.cost_min == want["cost_min"] and r.cost_median == want["cost_median"]
    assert (got.skipped, got.margin_x, got.margin_y) == (0, 0, 0)
    return got


def test_estimate_gives_the_axis_search_s_answers():
    """the cases of tests/test_axis_search_host.py"""
    r = assert_estimate_equals_both(-1.0, 0.5, [9.0, 4.0, 1.0, 2.0, 7.0])
    assert r.best == 2 and r.at_edge == 0 and r.eta_deg == np.float32(0.0 + 0.5 * (0.5 * (4.0 - 2.0) / 4.0)) and r.cost_median == 4.0
    rng = np.random.default_rng(5)
    for _ in range(50):
        n = int(rng.integers(3, 40))
        x = np.linspace(-3, 3, n) - rng.uniform(-2, 2)
        assert_estimate_equals_both(float(rng.uniform(-5, 5)), float(rng.choice([0.25, 0.3, 1.0])), x * x + rng.normal(0, 0.3, n) + 2)
    r = assert_estimate_equals_both(0.0, 1.0, [5.0, 1.0, 1.0, 5.0])
    assert r.best == 1 and r.at_edge == 0 and r.eta_deg == np.float32(1.5)
    assert assert_estimate_equals_both(0.0, 1.0, [1.0, 1.0, 1.0]).at_edge == 1
    r = assert_estimate_equals_both(-2.0, 0.5, [1.0, 2.0, 3.0, 4.0])
    assert (r.best, r.at_edge, r.eta_deg) == (0, 1, -2.0)
    r = assert_estimate_equals_both(-2.0, 0.5, [4.0, 3.0, 2.0, 1.0])
    assert (r.best, r.at_edge, r.eta_deg) == (3, 1, -0.5)
    r = assert_estimate_equals_both(3.25, 0.5, [7.0])
    assert (r.best, r.at_edge, r.eta_deg, r.scored, r.cost_median) == (0, 1, 3.25, 1, 7.0)
    r = assert_estimate_equals_both(0.0, 1.0, [INF, 1.0, 3.0, 9.0, INF])
    assert (r.best, r.at_edge, r.eta_deg, r.scored) == (1, 1, 1.0, 3) and r.cost_median == 3.0
    r = assert_estimate_equals_both(0.0, 1.0, [4.0, 1.0, INF, 0.5, INF, 9.0])
    assert (r.best, r.at_edge, r.eta_deg, r.scored) == (3, 1, 3.0, 4) and r.cost_median == 1.0
    r = assert_estimate_equals_both(0.0, 1.0, [4.0, 1.0, float("nan"), 7.0])
    assert (r.best, r.at_edge, r.scored) == (1, 1, 3)
    r = assert_estimate_equals_both(0.0, 1.0, [1.5e308, 1e308, 1.5e308])
    assert (r.best, r.at_edge, r.eta_deg) == (1, 1, 1.0)


def test_estimate_refusals():
    L = _lib.load()
    out, cost = _lib.RollResult(), np.ones(3)
    good = _lib.RollSearch(0.0, 1.0, 3, 0)
    assert L.paris_hip_roll_estimate_from_costs(None, cost.ctypes.data, C.byref(out)) == INV
    assert L.paris_hip_roll_estimate_from_costs(C.byref(good), None, C.byref(out)) == INV
    assert L.paris_hip_roll_estimate_from_costs(C.byref(good), cost.ctypes.data, None) == INV
    for bad in ((0.0, 1.0, 0), (0.0, 1.0, 257), (0.0, 0.0, 3), (0.0, -1.0, 3), (float("nan"), 1.0, 3), (0.0, INF, 3)):
        assert L.paris_hip_roll_estimate_from_costs(C.byref(_lib.RollSearch(bad[0], bad[1], bad[2], 0)), cost.ctypes.data, C.byref(out)) == INV, bad
    none = np.full(3, np.inf)
    out.scored = 7
    assert L.paris_hip_roll_estimate_from_costs(C.byref(good), none.ctypes.data, C.byref(out)) == INV and out.scored == 0
    assert R.estimate(0.0, 1.0, none) is None


# ---- recovery on the rule alone ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("eta,delta_s", [(0.0, 0.0), (0.8, 1.3), (-1.7, 0.0)])
def test_the_rule_recovers_a_known_roll_from_analytic_frames(eta, delta_s):
    """90 views of four off-centre spheres on a 96 x 80 detector rolled by eta, float64 frames, candidates -3 ... 3 in steps of 0.25:
    the minimum of the mirror cost of the scan mean is at eta to within 0.05 deg (the float64 prototype: 0.005 deg)"""
    g, frames = R.scan(eta, delta_s)
    cost, pairs, skipped, (m_x, m_y) = R.costs(frames.mean(axis=0), *R.SEARCH, g, dtype=np.float64)
    est = R.estimate(R.SEARCH[0], R.SEARCH[1], cost)
    print("roll rule: true %.2f, delta_s %.1f, estimate %.4f, J_min / J_median %.2g, margins %d %d" %
          (eta, delta_s, est["value"], est["cost_min"] / est["cost_median"], m_x, m_y))
    assert est["at_edge"] == 0 and est["scored"] == 25 and skipped.sum() == 0 and pairs.min() > 96 * 80 // 2
    assert abs(float(est["value"]) - eta) <= R.BOUND_DEG
    lib = B.roll_estimate_from_costs(R.SEARCH[0], R.SEARCH[1], cost)     # the library's estimate from the rule's costs
    assert lib.eta_deg == est["value"]
