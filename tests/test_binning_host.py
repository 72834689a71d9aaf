"""Detector binning, the host side: the check, the binned geometry, and paris_hip_bin_frame_host /
paris_hip_bin_mask against the numpy restatement of the rule (tests/binning_rule.py), bit for bit. No device."""
import ctypes as C

import numpy as np
import pytest

import binning_rule as R
from paris_amd import _lib
from paris_amd import backend as B

each_setting = pytest.mark.parametrize("bin_x,bin_y", R.SETTINGS)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- the check --------------------------------------------------------------------------------------------------------------------

@each_setting
def test_binned_sizes_of_a_67_x_45_detector(bin_x, bin_y):
    assert B.binning_check(bin_x, bin_y, 67, 45) == (67 // bin_x, 45 // bin_y) == R.binned_size(bin_x, bin_y, 67, 45)


def test_the_check_s_refusals():
    L = _lib.load()
    ox, oy = C.c_uint32(7), C.c_uint32(7)

    def status(bn, dim_x, dim_y):
        return L.paris_hip_binning_check(None if bn is None else C.byref(_lib.Binning(*bn)), dim_x, dim_y, C.byref(ox), C.byref(oy))

    assert status(None, 67, 45) == _lib.ERROR_INVALID_ARGUMENT
    for bad in (0, 3, 5, 6, 7, 9, 16, 2 ** 31):
        assert status((bad, 2), 67, 45) == _lib.ERROR_INVALID_ARGUMENT, bad
        assert status((2, bad), 67, 45) == _lib.ERROR_INVALID_ARGUMENT, bad
    assert status((8, 1), 7, 45) == _lib.ERROR_INVALID_ARGUMENT      # out_x == 0
    assert status((1, 8), 67, 7) == _lib.ERROR_INVALID_ARGUMENT      # out_y == 0
    assert status((1, 1), 0, 45) == _lib.ERROR_INVALID_ARGUMENT and status((1, 1), 67, 0) == _lib.ERROR_INVALID_ARGUMENT
    assert (ox.value, oy.value) == (7, 7)                            # a refusal writes nothing
    assert status((8, 8), 8, 8) == _lib.SUCCESS and (ox.value, oy.value) == (1, 1)
    assert L.paris_hip_binning_check(C.byref(_lib.Binning(2, 4)), 67, 45, None, None) == _lib.SUCCESS   # both pointers are optional
    with pytest.raises(B.ParisHipError):
        B.binning_check(3, 1, 67, 45)


# ---- the geometry -----------------------------------------------------------------------------------------------------------------

GEO_ULPS = 3
"""The binned pixel pitch, the binned offset and their product each carry one rounding to fp32. With H = n l / 2 the detector's
half-width and u = ulp32(H) >= 2^-24 H: the pitch's rounding, relative 2^-24, scales a coordinate of at most H + |delta'| l' -- one u
for H, one more for the offset's share (|delta'| l' <= H on any detector whose axis is on it); the offset's own rounding moves the
centre by 2^-24 |delta'| l' <= u. The float64 evaluation of either side adds nothing at this scale. For the values below every binned
field is in fact exact (powers of two times short fractions), so the test also pins 0."""


def centres(n, pitch, delta):
    """t = (i + 1/2) l - n l / 2 - delta l in float64 from fp32 fields"""
    pitch, delta = float(np.float32(pitch)), float(np.float32(delta))
    return (np.arange(n) + 0.5) * pitch - n * pitch / 2 - delta * pitch


@each_setting
@pytest.mark.parametrize("n_row", [64, 67])
@pytest.mark.parametrize("n_col", [48, 45])
def test_binned_pixel_centres_are_the_means_of_their_source_pixels_centres(bin_x, bin_y, n_row, n_col):
    geo = (n_row, n_col, 0.2, 0.25, 1.5, -0.75, 100, 200, 45)
    g = B.binned_geometry(bin_x, bin_y, B.DetectorGeometry(*geo))
    want = R.binned_geometry(geo, bin_x, bin_y)
    got = (g.n_row, g.n_col, g.l_px_row, g.l_px_col, g.delta_s, g.delta_t, g.d_so, g.d_od, g.delta_phi)
    assert got[:2] == want[:2] and np.array_equal(bits(got[2:]), bits(want[2:]))
    for n, n_b, b, pitch, delta, pitch_b, delta_b in ((n_row, g.n_row, bin_x, 0.2, 1.5, g.l_px_row, g.delta_s),
                                                      (n_col, g.n_col, bin_y, 0.25, -0.75, g.l_px_col, g.delta_t)):
        src = centres(n, pitch, delta)
        mean = src[:n_b * b].reshape(n_b, b).mean(axis=1)
        ulp = float(np.spacing(np.float32(n * float(np.float32(pitch)) / 2)))
        err = np.abs(centres(n_b, pitch_b, delta_b) - mean).max()
        assert err <= GEO_ULPS * ulp, (err / ulp)
        assert err <= 1e-12   # (these fields are exact: only float64 rounding is left)


def test_the_geometry_s_refusals_and_in_place_use():
    L = _lib.load()
    det, out = B.DetectorGeometry(67, 45, 0.2, 0.25, 1.5, -0.75, 100, 200, 45), B.DetectorGeometry()
    bn = _lib.Binning(2, 2)
    assert L.paris_hip_binned_geometry(None, C.byref(det), C.byref(out)) == _lib.ERROR_INVALID_ARGUMENT
    assert L.paris_hip_binned_geometry(C.byref(bn), None, C.byref(out)) == _lib.ERROR_INVALID_ARGUMENT
    assert L.paris_hip_binned_geometry(C.byref(bn), C.byref(det), None) == _lib.ERROR_INVALID_ARGUMENT
    assert L.paris_hip_binned_geometry(C.byref(_lib.Binning(3, 2)), C.byref(det), C.byref(out)) == _lib.ERROR_INVALID_ARGUMENT
    assert L.paris_hip_binned_geometry(C.byref(bn), C.byref(det), C.byref(det)) == _lib.SUCCESS
    assert (det.n_row, det.n_col, det.delta_s, det.delta_t) == (33, 22, 1.0, -0.125) and det.d_so == 100 and det.delta_phi == 45


# ---- the pixel rule ---------------------------------------------------------------------------------------------------------------

COUNTS = R.counts_frame().astype(np.float32)
ORDERED = R.ordered_frame()
MASK = R.shared_mask()


def test_the_f32_frame_makes_the_summation_order_observable():
    """summing the same bins column-major changes at least one output bit, without and with the mask: a wrong order cannot pass"""
    for mask in (None, MASK):
        for bin_x, bin_y in ((2, 2), (4, 4), (8, 8), (2, 8), (8, 2)):
            a, b = R.bin_frame(ORDERED, bin_x, bin_y, mask), R.bin_frame(ORDERED, bin_x, bin_y, mask, column_major=True)
            assert np.count_nonzero(bits(a) != bits(b)) > 0, (bin_x, bin_y)
    assert np.array_equal(bits(R.bin_frame(COUNTS, 4, 4)), bits(R.bin_frame(COUNTS, 4, 4, column_major=True)))   # counts sum exactly


def test_the_mask_holds_the_cases_the_rule_distinguishes():
    for bin_x, bin_y in R.SETTINGS:
        bad = R._blocks(MASK != 0, bin_x, bin_y).sum(axis=(2, 3))
        assert bad[0, 0] == bin_x * bin_y                                          # a fully bad bin
        assert bad[15 // bin_y, 15 // bin_x] == bin_x * bin_y - 1                  # a bin with exactly one good pixel
        binned = R.bin_mask(MASK, bin_x, bin_y)
        assert binned[0, 0] == 1 and binned[15 // bin_y, 15 // bin_x] == 0
    assert np.all(MASK[29, :] != 0) and np.all(MASK[:, 37] != 0)                   # a bad full row and a bad full column


@each_setting
@pytest.mark.parametrize("frame", ["counts", "ordered"])
@pytest.mark.parametrize("masked", [False, True])
def test_bin_frame_host_equals_the_rule_bit_for_bit(bin_x, bin_y, frame, masked):
    f = COUNTS if frame == "counts" else ORDERED
    mask = MASK if masked else None
    want = R.bin_frame(f, bin_x, bin_y, mask)
    got = B.bin_frame_host(bin_x, bin_y, f, mask)
    assert got.shape == want.shape == (45 // bin_y, 67 // bin_x)
    assert np.array_equal(bits(got), bits(want))
    if frame == "ordered" and not masked:
        assert np.isnan(got[3 // bin_y, 5 // bin_x]) and np.isinf(got[20 // bin_y, 40 // bin_x])   # propagated
    if masked:
        assert bits(got)[0, 0] == 0   # n == 0 gives +0


@each_setting
def test_bin_mask_equals_the_rule(bin_x, bin_y):
    want = R.bin_mask(MASK, bin_x, bin_y)
    got = B.bin_mask(bin_x, bin_y, MASK)
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    # the binned mask marks exactly the bins whose mean is the n == 0 result
    n_good = R._blocks(MASK == 0, bin_x, bin_y).sum(axis=(2, 3))
    assert np.array_equal(got == 1, n_good == 0)


def test_the_host_functions_refusals():
    L = _lib.load()
    bn = _lib.Binning(2, 2)
    src, dst = np.zeros((4, 4), np.float32), np.zeros((2, 2), np.float32)
    m, mo = np.zeros((4, 4), np.uint8), np.zeros((2, 2), np.uint8)
    assert L.paris_hip_bin_frame_host(C.byref(bn), None, None, 4, 4, dst.ctypes.data) == _lib.ERROR_INVALID_ARGUMENT
    assert L.paris_hip_bin_frame_host(C.byref(bn), None, src.ctypes.data, 4, 4, None) == _lib.ERROR_INVALID_ARGUMENT
    assert L.paris_hip_bin_frame_host(C.byref(_lib.Binning(8, 2)), None, src.ctypes.data, 4, 4, dst.ctypes.data) == _lib.ERROR_INVALID_ARGUMENT
    assert L.paris_hip_bin_mask(C.byref(bn), None, 4, 4, mo.ctypes.data) == _lib.ERROR_INVALID_ARGUMENT
    assert L.paris_hip_bin_mask(C.byref(bn), m.ctypes.data, 4, 4, None) == _lib.ERROR_INVALID_ARGUMENT
    assert L.paris_hip_bin_mask(C.byref(_lib.Binning(2, 3)), m.ctypes.data, 4, 4, mo.ctypes.data) == _lib.ERROR_INVALID_ARGUMENT
    with pytest.raises(ValueError):
        B.bin_frame_host(2, 2, src, np.zeros((4, 5), np.uint8))
