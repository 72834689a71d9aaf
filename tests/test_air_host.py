"""The host side of the air-region normalisation (paris_hip_air_region_check, paris_hip_air_value_host): no
device, no ctx -- the refusals, one per clause, the resolved default, what a setting occupies, and the library's rule against its
numpy restatement (tests/air_rule.py) bit for bit, on values whose sum depends on the order of the additions."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import air_rule as A
from paris_amd import _lib
from paris_amd import backend as B


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "paris_amd", "host", "demo", "paris.hip")
GEO_KEYS = ("n_row", "n_col", "l_px_row", "l_px_col", "delta_s", "delta_t", "d_so", "d_od", "delta_phi")


def status(x0, y0, w, h, min_pixels, limit_abs, dim_x, dim_y):
    ar = _lib.AirRegion(x0, y0, w, h, min_pixels, limit_abs)
    return _lib.load().paris_hip_air_region_check(C.byref(ar), dim_x, dim_y, None, None)


def test_a_good_setting_is_accepted_with_null_outputs():
    assert status(0, 0, 140, 20, 0, 0.0, 140, 20) == _lib.SUCCESS
    assert status(139, 19, 1, 1, 1, 0.0, 140, 20) == _lib.SUCCESS
    assert status(3, 7, 64, 4, 256, 0.5, 140, 20) == _lib.SUCCESS           # min_pixels = every pixel
    assert status(0, 0, 1024, 1024, 0, 0.0, 2048, 2048) == _lib.SUCCESS     # exactly 2^20 pixels


@pytest.mark.parametrize("what,args", [
    ("zero dim_x", (0, 0, 1, 1, 0, 0.0, 0, 20)),
    ("zero dim_y", (0, 0, 1, 1, 0, 0.0, 140, 0)),
    ("zero width", (3, 3, 0, 2, 0, 0.0, 140, 20)),
    ("zero height", (3, 3, 2, 0, 0, 0.0, 140, 20)),
    ("x0 outside", (140, 3, 1, 1, 0, 0.0, 140, 20)),
    ("y0 outside", (3, 20, 1, 1, 0, 0.0, 140, 20)),
    ("too wide", (100, 3, 41, 2, 0, 0.0, 140, 20)),
    ("too high", (3, 15, 2, 6, 0, 0.0, 140, 20)),
    ("x0 + width wraps", (2, 0, 0xFFFFFFFF, 1, 0, 0.0, 140, 20)),
    ("y0 + height wraps", (0, 2, 1, 0xFFFFFFFF, 0, 0.0, 140, 20)),
    ("more than 2^20 pixels", (0, 0, 1025, 1024, 0, 0.0, 2048, 2048)),
    ("min_pixels above the rectangle", (3, 7, 64, 4, 257, 0.0, 140, 20)),
    ("negative limit", (3, 7, 64, 4, 0, -0.1, 140, 20)),
    ("limit NaN", (3, 7, 64, 4, 0, float("nan"), 140, 20)),
    ("limit Inf", (3, 7, 64, 4, 0, float("inf"), 140, 20)),
])
def test_refusals(what, args):
    assert status(*args) == _lib.ERROR_INVALID_ARGUMENT, what


def test_a_null_setting_is_refused():
    least, nbytes = C.c_uint32(7), C.c_size_t(7)
    assert _lib.load().paris_hip_air_region_check(None, 140, 20, C.byref(least), C.byref(nbytes)) == _lib.ERROR_INVALID_ARGUMENT
    assert (least.value, nbytes.value) == (7, 7)   # nothing written


@pytest.mark.parametrize("rect", A.RECTANGLES + [(0, 0, 1024, 1024)])
def test_the_default_min_pixels_and_the_bytes(rect):
    x0, y0, w, h = rect
    dim = (2048, 2048) if w > A.DIM_X else (A.DIM_X, A.DIM_Y)
    least, nbytes = B.air_region_check(x0, y0, w, h, *dim)
    assert least == (w * h + 1) // 2 == A.default_min_pixels(w, h)
    assert nbytes >= w * h + 8 * A.FRAMES_MAX > 0                      # the mask bytes, a value and a count per frame of a launch
    assert B.air_region_check(x0, y0, w, h, *dim, min_pixels=1) == (1, nbytes)
    assert B.Backend.air_region_check(x0, y0, w, h, *dim, min_pixels=w * h, limit_abs=0.25) == (w * h, nbytes)


def test_the_mirror_raises_for_a_refused_setting():
    with pytest.raises(B.ParisHipError) as e:
        B.air_region_check(0, 0, 0, 1, 140, 20)
    assert e.value.status == _lib.ERROR_INVALID_ARGUMENT
    with pytest.raises(B.ParisHipError) as e:
        B.air_value_host(100, 3, 41, 2, np.zeros((20, 140), np.float32))
    assert e.value.status == _lib.ERROR_INVALID_ARGUMENT
    with pytest.raises(ValueError):
        B.air_value_host(0, 0, 1, 1, np.zeros(5, np.float32))
    with pytest.raises(ValueError):
        B.air_value_host(0, 0, 1, 1, np.zeros((20, 140), np.float32), mask=np.zeros((20, 139), np.uint8))
    assert B.Backend.air_value_host is B.air_value_host and B.Backend.air_region_check is B.air_region_check
    ar = _lib.AirRegion(0, 0, 1, 1, 0, 0.0)
    assert _lib.load().paris_hip_air_value_host(C.byref(ar), None, None, 140, 20, None, None) == _lib.ERROR_INVALID_ARGUMENT


def host(frame, rect, **kw):
    return B.air_value_host(*rect, frame, **kw)


def assert_equals_rule(frame, rect, **kw):
    a, n = host(frame, rect, **kw)
    want_a, want_n, why = A.value(frame, rect, **kw)
    assert n == want_n and A.same_bits(a, want_a), (rect, kw, a, want_a)
    return a, n, why


def test_the_value_equals_the_rule_and_the_order_of_additions_shows():
    differs = 0
    for rect in A.RECTANGLES:
        for f in A.decades_scan(A.DIM_X, A.DIM_Y, 2) + A.cancelling_scan(A.DIM_X, A.DIM_Y, 2, rect):
            a, n, why = assert_equals_rule(f, rect)
            assert why == "normalised" and n == rect[2] * rect[3]
            x0, y0, w, h = rect
            plain = np.float32(np.sum(f[y0:y0 + h, x0:x0 + w].astype(np.float64)) / np.float64(n))
            differs += not A.same_bits(a, plain)
    print("np.sum differs in %d of %d cases" % (differs, 4 * len(A.RECTANGLES)))
    assert differs >= 1      # numpy's pairwise sum of the same pixels gives other bits somewhere: the order is what is tested


def test_a_drifting_scan_gives_back_its_drift():
    frames = A.scan(A.DIM_X, A.DIM_Y, 4, seed=5)
    for f in frames:
        a, n, why = assert_equals_rule(f, (0, 0, 8, 3))
        assert 0 < abs(a) < 0.06 and why == "normalised"


@pytest.mark.parametrize("rect", A.RECTANGLES)
def test_a_mask_and_pixels_that_are_not_finite_do_not_count(rect):
    x0, y0, w, h = rect
    f = A.awkward(A.decades_scan(A.DIM_X, A.DIM_Y, 1, seed=6)[0], rect)
    mask = A.random_mask(A.DIM_X, A.DIM_Y)
    bad = np.count_nonzero(~np.isfinite(f[y0:y0 + h, x0:x0 + w]))
    assert bad >= 1
    a, n, why = assert_equals_rule(f, rect, min_pixels=1)
    assert n == w * h - bad and why == ("normalised" if n else "too_few")
    a, n, why = assert_equals_rule(f, rect, mask=mask)
    assert n == np.count_nonzero((mask[y0:y0 + h, x0:x0 + w] == 0) & np.isfinite(f[y0:y0 + h, x0:x0 + w]))
    assert np.isfinite(a)


def test_too_few_above_limit_and_an_all_masked_rectangle():
    rect = (3, 7, 64, 4)
    f = (0.5 + np.random.default_rng(7).normal(0, 0.01, (A.DIM_Y, A.DIM_X))).astype(np.float32)
    free = assert_equals_rule(f, rect)
    assert free[2] == "normalised" and 0.4 < free[0] < 0.6
    # the limit: just above |a| keeps it, just below zeroes it; 0 is no limit
    assert assert_equals_rule(f, rect, limit_abs=float(np.nextafter(free[0], np.float32(1))))[0] == free[0]
    assert assert_equals_rule(f, rect, limit_abs=float(free[0]))[0] == free[0]                  # |a| > limit is false at equality
    a, n, why = assert_equals_rule(f, rect, limit_abs=float(np.nextafter(free[0], np.float32(0))))
    assert why == "above_limit" and a == 0 and not np.signbit(a) and n == 256
    a, n, why = assert_equals_rule(-f, rect, limit_abs=0.25)
    assert why == "above_limit" and a == 0 and not np.signbit(a)
    # too few: half the rectangle masked, plus one
    mask = np.zeros((A.DIM_Y, A.DIM_X), np.uint8)
    mask[7:9, 3:67] = 1
    assert assert_equals_rule(f, rect, mask=mask)[1:] == (128, "normalised")                    # the default asks for 128
    mask[9, 3] = 7
    a, n, why = assert_equals_rule(f, rect, mask=mask)
    assert (float(a), n, why) == (0.0, 127, "too_few") and not np.signbit(a)
    assert assert_equals_rule(f, rect, mask=mask, min_pixels=127)[2] == "normalised"
    # nothing counts: every pixel masked, or none finite
    mask[7:11, 3:67] = 1
    a, n, why = assert_equals_rule(f, rect, mask=mask, min_pixels=1)
    assert (float(a), n, why) == (0.0, 0, "too_few")
    g = f.copy()
    g[7:11, 3:67] = np.nan
    assert assert_equals_rule(g, rect, min_pixels=1)[1:] == (0, "too_few")
    # a mask outside the rectangle changes nothing
    outside = np.ones((A.DIM_Y, A.DIM_X), np.uint8)
    outside[7:11, 3:67] = 0
    assert A.same_bits(host(f, rect, mask=outside)[0], free[0])


def test_negative_zeros_sum_to_plus_zero():
    f = np.full((A.DIM_Y, A.DIM_X), -0.0, np.float32)
    a, n, why = assert_equals_rule(f, (3, 7, 64, 4))
    assert a == 0 and not np.signbit(a) and why == "normalised"


@pytest.mark.parametrize("value,extra", [("abc", []), ("1:1:7", []), ("1:1:7:5:0.1:3", []), ("1:1:7:", []), ("1:-1:7:5", []), ("1:1:7:5:x", []),
                                         ("1:1:0:5", []), ("60:1:5:5", []), ("1:44:7:5", []), ("1:1:7:5:-0.1", []), ("1:1:7:5:nan", []),
                                         ("30:1:3:3", ["--bin", "2"]), ("1:22:3:3", ["--bin", "2"])])
def test_the_driver_refuses_a_bad_air_region_before_any_device_work(tmp_path, value, extra):
    """the rectangle is checked against the frame the reconstruction sees: 64 x 48, and 32 x 24 with --bin 2"""
    if not os.path.exists(EXE):
        pytest.fail("%s missing: run __graft_entry__.build()" % EXE)
    ini = tmp_path / "geo.ini"
    ini.write_text("\n".join("%s = %s" % kv for kv in zip(GEO_KEYS, A.DRIVER_GEO)) + "\n")
    (tmp_path / "in").mkdir()
    args = [EXE, "--geometry", ini, "--input", tmp_path / "in", "--output", tmp_path / "out", "--air-region", value] + extra
    r = subprocess.run([str(a) for a in args], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1, r.stdout + r.stderr
    assert "Pipeline construction failed" in r.stderr and "--air-region" in r.stderr, r.stderr
    assert not (tmp_path / "out").exists()   # refused before the output was set up, let alone a device
