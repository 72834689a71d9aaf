"""The host side of the ring filter (paris_hip_ring_filter_check, paris_hip_ring_correction_from_mean): no
device, no ctx -- the refusals, one per clause, what a setting occupies, the library's rule against its numpy restatement on frames
small enough to do by hand, and the quality figures of the oracle pipeline."""
import ctypes as C

import numpy as np
import pytest

import ring_rule as R
from paris_amd import _lib
from paris_amd import backend as B


def status(h, floor_abs, limit_abs, dim_x, dim_y):
    rf = _lib.RingFilter(h, floor_abs, limit_abs)
    return _lib.load().paris_hip_ring_filter_check(C.byref(rf), dim_x, dim_y, None, None)


def test_a_good_setting_is_accepted_with_null_outputs():
    for h in (1, 2, 32):
        assert status(h, 0.0, 0.0, 64, 48) == _lib.SUCCESS
    assert status(2, 0.035, 0.0, 64, 48) == _lib.SUCCESS      # no upper limit
    assert status(2, 0.035, 0.25, 64, 48) == _lib.SUCCESS
    assert status(2, 0.0, 0.25, 64, 48) == _lib.SUCCESS
    assert status(32, 0.0, 0.0, 1, 1) == _lib.SUCCESS         # the window may be wider than the row


@pytest.mark.parametrize("what,args", [
    ("zero dim_x", (2, 0.0, 0.0, 0, 48)),
    ("zero dim_y", (2, 0.0, 0.0, 64, 0)),
    ("half_width 0", (0, 0.0, 0.0, 64, 48)),
    ("half_width 33", (33, 0.0, 0.0, 64, 48)),
    ("negative floor", (2, -0.01, 0.0, 64, 48)),
    ("floor NaN", (2, float("nan"), 0.0, 64, 48)),
    ("floor Inf", (2, float("inf"), 0.0, 64, 48)),
    ("limit NaN", (2, 0.0, float("nan"), 64, 48)),
    ("limit Inf", (2, 0.0, float("inf"), 64, 48)),
    ("limit equal to the floor", (2, 0.1, 0.1, 64, 48)),
    ("limit below the floor", (2, 0.1, 0.05, 64, 48)),
    ("negative limit", (2, 0.0, -0.1, 64, 48)),
])
def test_refusals(what, args):
    assert status(*args) == _lib.ERROR_INVALID_ARGUMENT, what


def test_a_null_setting_is_refused():
    a, b = C.c_size_t(7), C.c_size_t(7)
    assert _lib.load().paris_hip_ring_filter_check(None, 64, 48, C.byref(a), C.byref(b)) == _lib.ERROR_INVALID_ARGUMENT
    assert (a.value, b.value) == (7, 7)   # nothing written


def test_a_frame_beyond_32_bit_pixel_indices_is_unsupported():
    assert status(2, 0.0, 0.0, 1 << 16, 1 << 16) == _lib.ERROR_UNSUPPORTED
    assert status(2, 0.0, 0.0, (1 << 16) - 1, 1 << 16) == _lib.SUCCESS


@pytest.mark.parametrize("dim_x,dim_y", [(1, 1), (64, 48), (2048, 2048)])
def test_bytes_are_8_and_4_per_pixel(dim_x, dim_y):
    assert B.ring_filter_check(2, 0.035, 0.25, dim_x, dim_y) == (8 * dim_x * dim_y, 4 * dim_x * dim_y)
    assert B.Backend.ring_filter_check(2, 0.035, 0.25, dim_x, dim_y) == (8 * dim_x * dim_y, 4 * dim_x * dim_y)


def test_the_mirror_raises_for_a_refused_setting():
    with pytest.raises(B.ParisHipError) as e:
        B.ring_filter_check(0, 0.0, 0.0, 64, 48)
    assert e.value.status == _lib.ERROR_INVALID_ARGUMENT
    with pytest.raises(B.ParisHipError) as e:
        B.ring_correction_from_mean(2, 0.1, 0.05, np.zeros((3, 5), np.float32))
    assert e.value.status == _lib.ERROR_INVALID_ARGUMENT
    assert B.Backend.ring_correction_from_mean is B.ring_correction_from_mean


def test_null_arrays_are_refused():
    rf, m = _lib.RingFilter(1, 0.0, 0.0), np.zeros((2, 3), np.float32)
    L = _lib.load()
    assert L.paris_hip_ring_correction_from_mean(C.byref(rf), None, None, 3, 2, m.ctypes.data, None) == _lib.ERROR_INVALID_ARGUMENT
    assert L.paris_hip_ring_correction_from_mean(C.byref(rf), m.ctypes.data, None, 3, 2, None, None) == _lib.ERROR_INVALID_ARGUMENT
    assert L.paris_hip_ring_correction_from_mean(C.byref(rf), m.ctypes.data, None, 3, 2, m.copy().ctypes.data, None) == _lib.SUCCESS


# ---- the library's rule against the numpy restatement ---------------------------------------------------------------------------------

def both(mean, h, floor_abs=0.0, limit_abs=0.0, counts=None):
    """c of the library, after checking that c and the stats equal the numpy rule's"""
    m = np.asarray(mean, np.float32)
    want, want_st = R.correction(m, h, floor_abs, limit_abs, counts)
    got, st = B.ring_correction_from_mean(h, floor_abs, limit_abs, m, counts)
    assert R.same_bits(got, want), (got, want)
    got_st = R.stats_of(st)
    assert got_st.pop("max_abs") == np.float32(want_st.pop("max_abs")) and got_st == want_st
    return got, st


def test_the_rule_by_hand():
    row = np.array([[1, 1, 5, 1, 1, 1, 3, 3, 1, 1]], np.float32)
    c, st = both(row, 1)
    assert np.array_equal(c, [[0, 0, 4, 0, 0, 0, 0, 0, 0, 0]]) and st.corrected == 1   # a pair survives a window of three
    c, st = both(row, 2)
    assert np.array_equal(c, [[0, 0, 4, 0, 0, 0, 2, 2, 0, 0]]) and st.corrected == 3 and st.max_abs == 4
    assert (st.frames_min, st.frames_max) == (0, 0)                                     # no counts given
    c, _ = both(-row, 2)
    assert np.array_equal(c, [[0, 0, -4, 0, 0, 0, -2, -2, 0, 0]])


def test_edges_are_replicated():
    row = np.array([[7, 1, 1, 1, 1, 1, 9]], np.float32)
    c, _ = both(row, 1)
    assert np.array_equal(c, np.zeros((1, 7)))            # windows (7, 7, 1) and (1, 9, 9): the edge pixel is its own median
    c, _ = both(row, 2)
    assert np.array_equal(c, [[0, 0, 0, 0, 0, 0, 0]])     # (7, 7, 7, 1, 1): still
    c, _ = both(row, 3)
    assert np.array_equal(c, np.zeros((1, 7)))            # (7, 7, 7, 7, 1, 1, 1): h + 1 copies -- an edge pixel is never corrected
    row = np.array([[1, 7, 1, 1, 1, 9, 1]], np.float32)
    c, _ = both(row, 2)
    assert np.array_equal(c, [[0, 6, 0, 0, 0, 8, 0]])     # (1, 1, 1, 7, 1) and (1, 9, 1, 1, 1): the next pixel is
    ramp = np.arange(6, dtype=np.float32)[None]
    c, _ = both(ramp, 1)
    assert np.array_equal(c, np.zeros((1, 6)))            # (0, 0, 1) -> 0 and (4, 5, 5) -> 5


def test_degenerate_frames():
    both(np.array([[5.0]], np.float32), 1)
    both(np.array([[5.0]], np.float32), 32)
    both(np.array([[1.0], [2.0], [np.nan]], np.float32), 2)             # dim_x = 1: every window is 2h + 1 copies
    for h in (2, 3, 32):
        both(np.array([[1.0, 9.0, 2.0]], np.float32), h)                 # dim_x <= h
    c, _ = both(np.array([[1.0, 2.0], [4.0, 3.0]], np.float32), 1)       # 2 x 2: windows (1, 1, 2), (1, 2, 2), (4, 4, 3), (4, 3, 3)
    assert np.array_equal(c, np.zeros((2, 2)))
    rng = np.random.default_rng(2)
    for shape, h in [((3, 4), 2), ((5, 33), 32), ((7, 64), 16), ((2, 65), 32)]:
        both(rng.normal(0, 1, shape).astype(np.float32), h)
        both(rng.normal(0, 1, shape).astype(np.float32), h, 0.5, 1.5)


def test_windows_that_touch_a_nan_or_an_inf_give_zero():
    rng = np.random.default_rng(4)
    m = rng.normal(0, 1, (3, 40)).astype(np.float32)
    m[0, 10] = np.nan
    m[1, 20] = np.inf
    m[2, 0] = -np.inf
    c, st = both(m, 3)
    assert not c[0, 7:14].any() and not c[1, 17:24].any() and not c[2, 0:4].any()
    assert c[0, 6] != 0 and c[0, 14] != 0 and c[1, 16] != 0 and c[2, 4] != 0
    assert st.not_finite == 7 + 7 + 4 and st.corrected == np.count_nonzero(c) > 60   # (a window's own median has c = 0)
    assert np.all(np.isfinite(c))


def test_a_row_without_frames_gets_no_correction():
    rng = np.random.default_rng(6)
    m = rng.normal(0, 1, (4, 20)).astype(np.float32)
    m[2, 3] = np.nan                                      # not counted either: the row has no mean
    counts = np.array([5, 5, 0, 7], np.uint32)
    c, st = both(m, 2, counts=counts)
    assert not c[2].any() and c[1].any() and c[3].any()
    assert (st.frames_min, st.frames_max) == (0, 7) and st.not_finite == 0
    assert st.corrected + st.below_floor + st.above_limit + st.not_finite <= 3 * 20
    c, st = both(m, 2, counts=np.zeros(4, np.uint32))
    assert not c.any() and (st.corrected, st.frames_max) == (0, 0)


def test_floor_and_limit_exactly_met_are_kept():
    row = np.array([[0, 0, 0.25, 0, 0, 0, -0.5, 0, 0, 0, 1, 0, 0]], np.float32)   # c = 0.25, -0.5 and 1, exact in fp32
    c, st = both(row, 1, 0.25, 0.0)
    assert np.array_equal(np.flatnonzero(c), [2, 6, 10]) and st.below_floor == 10 and st.above_limit == 0
    c, st = both(row, 1, np.nextafter(np.float32(0.25), np.float32(1)), 0.0)
    assert np.array_equal(np.flatnonzero(c), [6, 10]) and st.below_floor == 11
    c, st = both(row, 1, 0.25, 1.0)
    assert np.array_equal(np.flatnonzero(c), [2, 6, 10]) and st.above_limit == 0
    c, st = both(row, 1, 0.25, np.nextafter(np.float32(1), np.float32(0)))
    assert np.array_equal(np.flatnonzero(c), [2, 6]) and (st.above_limit, st.below_floor, st.corrected) == (1, 10, 2)
    assert st.max_abs == 0.5
    c, st = both(row, 1, 0.0, 0.5)                        # floor 0: zeros are kept as zeros, and are not "corrected"
    assert np.array_equal(np.flatnonzero(c), [2, 6]) and (st.below_floor, st.above_limit, st.corrected) == (0, 1, 2)


def test_a_negative_zero_counts_as_zero():
    row = np.array([[-0.0, 0.0, -0.0, 0.0, 1.0, -0.0]], np.float32)
    c, st = both(row, 1)
    assert np.array_equal(np.flatnonzero(c), [4]) and st.corrected == 1
    assert not np.signbit(c).any()


def test_the_shared_scan_finds_the_planted_offsets():
    frames = R.scan(100, 37, 24)
    off = R.offsets(100, 37)
    c, st = R.correction(R.mean_of(R.sums(frames), 24), R.H, R.FLOOR, R.LIMIT, np.full(37, 24))
    planted = off != 0
    planted[:, [0, -1]] = False                           # (an edge pixel is never corrected)
    # a clean pixel is corrected only where three of its window's five carry an offset of one sign
    assert np.count_nonzero((c != 0) & planted) > 0.9 * planted.sum() and np.count_nonzero((c != 0) & (off == 0)) < 0.002 * c.size
    got, _ = both(R.mean_of(R.sums(frames), 24), R.H, R.FLOOR, R.LIMIT, np.full(37, 24, np.uint32))
    assert R.same_bits(got, c)


def test_quality_figures_of_the_oracle(oracle):
    """calibrates tests/test_gpu_ring_correction.py: the numpy rule and the oracle's weight, filter and backprojection on the 192 x 12
    case of ring_rule.py. The dead band must leave the clean scan exactly alone: not one pixel corrected"""
    import defect_rule as D
    det = oracle.DetectorGeometry(*R.QUALITY_GEO)
    vg = oracle.calculate_volume_geometry(det)
    lines = R.quality_frames(vg.dim_x, vg.l_vx_x)
    off = R.quality_offsets()
    ringed = [p + off for p in lines]
    clean = oracle.reconstruct(det, vg, len(lines), projections=lines)
    corrected, c_ringed, st_ringed = R.through_the_rule(ringed)
    clean_corrected, c_clean, st_clean = R.through_the_rule(lines)
    a = D.relative_rms(oracle.reconstruct(det, vg, len(lines), projections=ringed), clean)
    b = D.relative_rms(oracle.reconstruct(det, vg, len(lines), projections=corrected), clean)
    assert st_clean["corrected"] == 0 and not c_clean.any() and all(R.same_bits(p, q) for p, q in zip(clean_corrected, lines))
    c = D.relative_rms(oracle.reconstruct(det, vg, len(lines), projections=clean_corrected), clean)
    print("ring quality (oracle): relative RMS %.5g uncorrected, %.5g corrected (%d of %d offset pixels), %.5g clean-corrected (%d pixels)"
          % (a, b, st_ringed["corrected"], int((off != 0).sum()), c, st_clean["corrected"]))
    assert a == pytest.approx(R.CAL_UNCORRECTED, rel=0.02) and b == pytest.approx(R.CAL_CORRECTED, rel=0.02)
    assert c == R.CAL_CLEAN_CORRECTED
    assert b < a / 2
    # the library's rule gives the same correction frame
    n = len(lines)
    got, st = B.ring_correction_from_mean(R.QUALITY_H, R.QUALITY_FLOOR, R.QUALITY_LIMIT, R.mean_of(R.sums(ringed), n),
                                          np.full(lines[0].shape[0], n, np.uint32))
    assert R.same_bits(got, c_ringed) and st.corrected == st_ringed["corrected"]
