"""Row extension for truncated projections, the host side: the check, the response c against the numpy
restatement of tests/row_extension_rule.py, the restatement's own fmaf, and the quality figures of the rule through the CPU oracle
that calibrate tests/test_gpu_row_extension.py. No GPU."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

import row_extension_rule as R
from paris_amd import _lib
from paris_amd import backend as B

INVALID = _lib.ERROR_INVALID_ARGUMENT


def _check(m, w, dim_x):
    return _lib.load().paris_hip_row_extension_check(C.byref(_lib.RowExtension(m, w)), dim_x)


def _response(m, w, dim_x, tau, out="alloc"):
    c = np.empty(max(dim_x, 1), np.float32)
    ptr = c.ctypes.data if out == "alloc" else None
    return _lib.load().paris_hip_row_extension_response(C.byref(_lib.RowExtension(m, w)), dim_x, tau, ptr)


def test_check_refusals():
    L = _lib.load()
    assert L.paris_hip_row_extension_check(None, 64) == INVALID
    for m in (0, 3, 5, 6, 7, 9, 16):
        assert _check(m, 16, 64) == INVALID
    for w in (0, R.TAPER_MAX + 1, 2 ** 31):
        assert _check(4, w, 64) == INVALID
    assert _check(4, 16, 0) == INVALID
    for m in R.EDGE_PIXELS:
        assert _check(m, 16, m) == 0 and _check(m, 1, 64) == 0 and _check(m, R.TAPER_MAX, 64) == 0
        if m > 1:
            assert _check(m, 16, m - 1) == INVALID
    with pytest.raises(B.ParisHipError):
        B.row_extension_check(3, 16, 64)
    B.row_extension_check(8, 16, 8)


def test_response_refusals():
    L = _lib.load()
    c = np.empty(64, np.float32)
    assert L.paris_hip_row_extension_response(None, 64, 0.2, c.ctypes.data) == INVALID
    assert _response(3, 16, 64, 0.2) == INVALID and _response(4, 0, 64, 0.2) == INVALID
    assert _response(4, R.TAPER_MAX + 1, 64, 0.2) == INVALID
    assert _response(4, 16, 0, 0.2) == INVALID and _response(4, 16, 3, 0.2) == INVALID
    for tau in (0.0, -0.2, float("inf"), float("nan")):
        assert _response(4, 16, 64, tau) == INVALID
    assert _response(4, 16, 64, 0.2, out=None) == INVALID
    assert _response(4, 16, 64, 0.2) == 0
    with pytest.raises(B.ParisHipError):
        B.row_extension_response(4, 16, 64, -1.0)


@pytest.mark.parametrize("tau", [0.2, 1.0])
@pytest.mark.parametrize("w", [1, 16, 700])
@pytest.mark.parametrize("n", [1, 7, 300, 2048])
def test_response_against_the_rule(n, w, tau):
    got = B.row_extension_response(1, w, n, tau)
    want64 = R.response64(n, tau, w)
    want = want64.astype(np.float32)
    assert got.dtype == np.float32 and got.shape == (n,)
    # within 1 fp32 ulp: libm's cos may differ from numpy's in the last place, which can move the once-rounded sum across a tie
    ulp = np.spacing(np.abs(want))
    assert np.all(np.abs(got.astype(np.float64) - want.astype(np.float64)) <= ulp)
    # The sign and the shape of c. g vanishes at even distances, so c[s] only collects the taper at the k of one parity: with W = 1
    # every other c[s] is exactly 0, and for any W the two parity classes of s are two interleaved sequences -- c is negative
    # (W >= 2) and increasing towards 0 WITHIN each class, not from one s to the next (c[1] > c[2] for every W tried). That is
    # what is asserted; "increasing in s" as a whole does not hold for the rule as include/paris_hip.h states it.
    g64 = got.astype(np.float64)
    assert np.all(got <= 0)
    if w >= 2:
        assert np.all(got < 0)
    else:
        assert np.all(got[0::2] < 0) and not got[1::2].any()
    assert np.all(np.diff(g64[0::2]) > 0) and (w == 1 or np.all(np.diff(g64[1::2]) > 0))
    # c does not depend on edge_pixels
    assert np.array_equal(B.row_extension_response(8, w, n, tau), got) if n >= 8 else True


def test_restated_fma_is_exact():
    """the rule file's fma32 against exact rational arithmetic, ties of the float64 sum included"""
    rng = np.random.default_rng(5)
    x = rng.standard_normal(400).astype(np.float32)
    y = rng.standard_normal(400).astype(np.float32)
    z = rng.standard_normal(400).astype(np.float32)
    # near-cancellations, and sums that land on fp32 ties before the last bits of the product are added
    z[:100] = -(x[:100].astype(np.float64) * y[:100]).astype(np.float32)
    x[100:200] = np.float32(1) + np.float32(2.0 ** -23) * rng.integers(1, 100, 100).astype(np.float32)
    y[100:200] = np.float32(1) + np.float32(2.0 ** -23) * rng.integers(1, 100, 100).astype(np.float32)
    z[100:200] = np.float32(2.0 ** 24) * rng.integers(1, 3, 100).astype(np.float32) + np.float32(1)
    got = R.fma32(x, y, z)

    def rn32(fr):   # a Fraction rounded to nearest even fp32 (normal range)
        if fr == 0:
            return np.float32(0)
        sign = -1 if fr < 0 else 1
        fr = abs(fr)
        e = 0
        while fr >= 2 ** 24:
            fr /= 2
            e += 1
        while fr < 2 ** 23:
            fr *= 2
            e -= 1
        q, rem = divmod(fr.numerator, fr.denominator)
        twice = 2 * rem
        if twice > fr.denominator or (twice == fr.denominator and q % 2 == 1):
            q += 1
        return np.float32(sign * float(q) * 2.0 ** e)

    for i in range(len(x)):
        want = rn32(Fraction(float(x[i])) * Fraction(float(y[i])) + Fraction(float(z[i])))
        assert got[i] == want, (i, x[i], y[i], z[i], got[i], want)


def test_edge_means_and_update_shapes():
    q = np.arange(24, dtype=np.float32).reshape(2, 12) + np.float32(0.1)
    a, b = R.edge_means(q, 4)
    assert a[0] == np.float32((((q[0, 0] + q[0, 1]) + q[0, 2]) + q[0, 3]) * np.float32(0.25))
    assert b[1] == np.float32((((q[1, 8] + q[1, 9]) + q[1, 10]) + q[1, 11]) * np.float32(0.25))
    a, b = R.edge_means(q[:, :4], 4)   # dim_x == m: both means are the same pixels
    assert np.array_equal(a, b)
    c = R.response(12, 0.2, 16)
    plain = np.ones((2, 12), np.float32)
    assert np.array_equal(R.update(plain, np.zeros(2, np.float32), np.zeros(2, np.float32), c), plain)


def test_quality_figures_of_the_oracle(oracle):
    """calibrates tests/test_gpu_row_extension.py: weight, filter, the rule's update and backprojection through the oracle at the
    64 x 48 driver geometry with a phantom 1.6 x as wide as the grid, against an FDK reconstruction from a detector three times as
    wide in the same grid; relative RMS inside 0.85 of the field-of-view radius on the central half of the slices"""
    det = oracle.DetectorGeometry(*R.QUALITY_GEO)
    wide = oracle.DetectorGeometry(*R.wide_geo())
    vg = oracle.calculate_volume_geometry(det)
    region = R.quality_region((vg.dim_z, vg.dim_y, vg.dim_x), vg.l_vx_x)
    truth = R.oracle_reconstruct(oracle, wide, vg, R.quality_frames(vg.dim_x, vg.l_vx_x, R.TRUNCATED_RADIUS, wide=True))
    frames = R.quality_frames(vg.dim_x, vg.l_vx_x, R.TRUNCATED_RADIUS)
    zero = R.relative_rms(R.oracle_reconstruct(oracle, det, vg, frames), truth, region)
    e1 = R.relative_rms(R.oracle_reconstruct(oracle, det, vg, frames, (R.QUALITY_TAPER, 1)), truth, region)
    e4 = R.relative_rms(R.oracle_reconstruct(oracle, det, vg, frames, (R.QUALITY_TAPER, 4)), truth, region)
    print("row extension quality (oracle): relative RMS %.4g zero-padded, %.4g with (16, 1), %.4g with (16, 4)" % (zero, e1, e4))
    assert zero == pytest.approx(R.CAL_ZERO_PADDED, rel=0.02)
    assert e1 == pytest.approx(R.CAL_EXTENDED_1, rel=0.02) and e4 == pytest.approx(R.CAL_EXTENDED_4, rel=0.02)
    assert e4 < zero / 5
    # an untruncated phantom: the edge pixels are exactly 0, so (16, 1) changes nothing
    clean = R.quality_frames(vg.dim_x, vg.l_vx_x, R.UNTRUNCATED_RADIUS)
    assert all(not f[:, 0].any() and not f[:, -1].any() for f in clean)
    assert np.array_equal(R.oracle_reconstruct(oracle, det, vg, clean, (R.QUALITY_TAPER, 1)), R.oracle_reconstruct(oracle, det, vg, clean))
