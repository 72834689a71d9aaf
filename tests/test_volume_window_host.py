"""Host-only parts of the volume export: the check's refusals and the window from a histogram against the
numpy rule of tests/volume_window_rule.py. No device."""
import ctypes as C

import numpy as np
import pytest

import volume_window_rule as R
from paris_amd import _lib
from paris_amd import backend as B

INVALID = _lib.ERROR_INVALID_ARGUMENT


def check(lo, hi, voxel_type):
    w = _lib.VolumeWindow(lo, hi, voxel_type)
    return _lib.load().paris_hip_volume_window_check(C.byref(w))


def test_check_accepts_windows_the_rule_can_scale():
    for t in (_lib.VOXEL_U8, _lib.VOXEL_U16):
        assert check(0.0, 1.0, t) == 0
        assert check(-3e38, 3e38, t) == 0                 # the width is formed in double
        assert check(0.0, float(2.0 ** -100), t) == 0     # the narrowest window: its scale, L * 2^100, is still a finite float
        assert check(-1.0, float(np.nextafter(np.float32(-1), np.float32(0))), t) == 0


@pytest.mark.parametrize("what,lo,hi,voxel_type", [
    ("an unknown type", 0.0, 1.0, 0),
    ("an unknown type", 0.0, 1.0, 3),
    ("lo not finite", float("nan"), 1.0, _lib.VOXEL_U16),
    ("lo not finite", float("-inf"), 1.0, _lib.VOXEL_U16),
    ("hi not finite", 0.0, float("inf"), _lib.VOXEL_U8),
    ("hi not finite", 0.0, float("nan"), _lib.VOXEL_U8),
    ("hi == lo", 0.25, 0.25, _lib.VOXEL_U16),
    ("hi < lo", 1.0, 0.0, _lib.VOXEL_U16),
    ("narrower than 2^-100", 0.0, float(np.nextafter(np.float32(2.0 ** -100), np.float32(0))), _lib.VOXEL_U16),
    ("narrower than 2^-100", 0.0, 1e-45, _lib.VOXEL_U8),
])
def test_check_refusals(what, lo, hi, voxel_type):
    """One case per clause. The last clause, a scale that is not finite, has no case of its own: with a width of at least 2^-100 the
    scale is at most 65535 * 2^100 < 2^117, a finite float -- the clause guards the arithmetic, no input reaches it."""
    assert check(lo, hi, voxel_type) == INVALID, what


def test_check_refuses_null():
    assert _lib.load().paris_hip_volume_window_check(None) == INVALID


def from_histogram(hist, h_lo, h_hi, p_lo, p_hi):
    h = np.ascontiguousarray(hist, np.uint64)
    lo, hi = C.c_float(-1), C.c_float(-1)
    rc = _lib.load().paris_hip_volume_window_from_histogram(h.ctypes.data, h.size, h_lo, h_hi, p_lo, p_hi, C.byref(lo), C.byref(hi))
    return rc, np.float32(lo.value), np.float32(hi.value)


def assert_rule(hist, h_lo, h_hi, p_lo, p_hi):
    rc, lo, hi = from_histogram(hist, h_lo, h_hi, p_lo, p_hi)
    want = R.window_from_histogram(hist, h_lo, h_hi, p_lo, p_hi)
    assert rc == 0
    assert (lo.tobytes(), hi.tobytes()) == (want[0].tobytes(), want[1].tobytes()), (lo, hi, want, p_lo, p_hi)
    return lo, hi


PERCENTILES = [(0.1, 99.9), (0.0, 100.0), (0.0, 50.0), (50.0, 100.0), (1.0, 99.0), (25.0, 75.0), (49.9, 50.1)]


@pytest.mark.parametrize("seed", range(6))
def test_window_from_seeded_histograms(seed):
    rng = np.random.default_rng(seed)
    n_bins = (1, 2, 255, 1000, 4096, 4096)[seed]
    hist = rng.integers(0, 1 << (10 + 4 * seed), n_bins).astype(np.uint64)
    hist[rng.random(n_bins) < 0.4] = 0     # runs of empty bins
    if hist.sum() == 0:
        hist[0] = 7
    h_lo, h_hi = np.float32(rng.normal()), np.float32(rng.normal() + 5.0)
    for p_lo, p_hi in PERCENTILES:
        lo, hi = assert_rule(hist, h_lo, h_hi, p_lo, p_hi)
        assert h_lo <= lo < hi <= h_hi or n_bins > 1000   # (ends one float apart may round together in the finest histograms)


def test_window_of_a_single_non_empty_bin():
    hist = np.zeros(64, np.uint64)
    hist[17] = 123456789
    for p_lo, p_hi in PERCENTILES:
        lo, hi = assert_rule(hist, -2.0, 6.0, p_lo, p_hi)
        assert (lo, hi) == (np.float32(-2.0 + 17 / 8), np.float32(-2.0 + 18 / 8))   # that bin, whatever the percentiles


def test_window_at_the_percentiles_0_and_100():
    hist = np.array([0, 0, 3, 1, 0, 4, 0], np.uint64)
    lo, hi = assert_rule(hist, 0.0, 7.0, 0.0, 100.0)
    assert (lo, hi) == (2.0, 6.0)   # the first and the last non-empty bin: C(b) > 0 and C(b) >= T


def test_window_ties():
    """T * p / 100 falls exactly on a cumulative count: the low end takes the NEXT bin that adds something (C(b) > ...), the high end
    the bin that reaches the count (C(b) >= ...)."""
    hist = np.array([25, 25, 0, 25, 25], np.uint64)   # cumulative 25 50 50 75 100
    lo, hi = assert_rule(hist, 0.0, 5.0, 25.0, 75.0)
    assert (lo, hi) == (1.0, 4.0)
    lo, hi = assert_rule(hist, 0.0, 5.0, 50.0, 100.0)
    assert (lo, hi) == (3.0, 5.0)
    lo, hi = assert_rule(hist, 0.0, 5.0, 0.0, 50.0)
    assert (lo, hi) == (0.0, 2.0)
    big = np.array([1 << 40, 1 << 40, 1 << 41], np.uint64)   # counts beyond 32 bits, still exact in double
    lo, hi = assert_rule(big, -1.0, 2.0, 25.0, 50.0)
    assert (lo, hi) == (0.0, 1.0)


def test_window_refusals():
    hist = np.array([1, 2, 3], np.uint64)
    assert from_histogram(np.zeros(5, np.uint64), 0.0, 1.0, 0.1, 99.9)[0] == INVALID   # T = 0
    for p_lo, p_hi in ((-0.1, 50.0), (50.0, 50.0), (60.0, 50.0), (0.0, 100.1), (float("nan"), 50.0), (0.0, float("nan"))):
        assert from_histogram(hist, 0.0, 1.0, p_lo, p_hi)[0] == INVALID, (p_lo, p_hi)
    for h_lo, h_hi in ((1.0, 1.0), (2.0, 1.0), (float("nan"), 1.0), (0.0, float("inf"))):
        assert from_histogram(hist, h_lo, h_hi, 0.1, 99.9)[0] == INVALID, (h_lo, h_hi)
    L = _lib.load()
    lo, hi = C.c_float(), C.c_float()
    assert L.paris_hip_volume_window_from_histogram(None, 3, 0.0, 1.0, 0.1, 99.9, C.byref(lo), C.byref(hi)) == INVALID
    assert L.paris_hip_volume_window_from_histogram(hist.ctypes.data, 0, 0.0, 1.0, 0.1, 99.9, C.byref(lo), C.byref(hi)) == INVALID
    assert L.paris_hip_volume_window_from_histogram(hist.ctypes.data, 3, 0.0, 1.0, 0.1, 99.9, None, C.byref(hi)) == INVALID


def test_the_python_mirror_raises_for_a_refused_setting():
    B.volume_window_check(0.0, 1.0, np.uint16)
    assert B.volume_window_from_histogram([1, 2, 3], 0.0, 3.0, 0.0, 100.0) == (0.0, 3.0)
    for lo, hi, dtype in ((1.0, 1.0, np.uint8), (0.0, float("inf"), np.uint16), (0.0, 1.0, np.int16), (0.0, 1.0, np.float32)):
        with pytest.raises(B.ParisHipError) as e:
            B.volume_window_check(lo, hi, dtype)
        assert e.value.status == INVALID
    with pytest.raises(B.ParisHipError):
        B.volume_window_from_histogram(np.zeros(4, np.uint64), 0.0, 1.0)
    with pytest.raises(B.ParisHipError):
        B.volume_window_from_histogram([1, 2], 0.0, 1.0, 50.0, 50.0)


def test_the_numpy_rule_itself():
    """the reference the GPU tests compare with, on values worked out by hand"""
    v = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 0.25, 0.75, 1.25, 63.75, 127.5, 200.0], np.float32)
    assert R.quantize(v, 0.0, 127.5, np.uint8).tolist() == [0, 255, 0, 0, 0, 0, 2, 2, 128, 255, 255]   # scale 2: ties go to even
    assert R.counts(v, 0.0, 127.5) == (11, 0, 1, 3)
    assert R.extremes(v) == (0.0, 200.0) and R.extremes(v[:3]) == (np.inf, -np.inf)
    hist, below, above, not_finite = R.histogram(v, 0.25, 127.5, 2)
    assert hist.tolist() == [4, 1] and (below, above, not_finite) == (2, 1, 3)   # 127.5 = h_hi lands in the last bin
