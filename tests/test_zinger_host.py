"""The host side of the zinger filter (paris_hip_zinger_filter_check): no device, no ctx -- the refusals, one per
clause, the default max_hits, what a setting occupies, and the numpy restatement of the rule on frames small enough to do by hand."""
import ctypes as C

import numpy as np
import pytest

import zinger_rule as Z
from paris_amd import _lib
from paris_amd import backend as B


def status(t_abs, t_rel, polarity, max_hits, dim_x, dim_y):
    zf = _lib.ZingerFilter(t_abs, t_rel, polarity, max_hits)
    return _lib.load().paris_hip_zinger_filter_check(C.byref(zf), dim_x, dim_y, None, None)


def test_a_good_setting_is_accepted_with_null_outputs():
    for polarity in (-1, 0, 1):
        assert status(0.25, 0.0, polarity, 0, 64, 48) == _lib.SUCCESS
    assert status(0.0, 0.1, 0, 0, 64, 48) == _lib.SUCCESS            # one threshold may be zero
    assert status(0.25, 0.1, 1, 64 * 48, 64, 48) == _lib.SUCCESS     # max_hits may be the whole frame


@pytest.mark.parametrize("what,args", [
    ("zero dim_x", (0.25, 0.0, 1, 0, 0, 48)),
    ("zero dim_y", (0.25, 0.0, 1, 0, 64, 0)),
    ("negative threshold_abs", (-0.25, 0.1, 1, 0, 64, 48)),
    ("negative threshold_rel", (0.25, -0.1, 1, 0, 64, 48)),
    ("threshold_abs NaN", (float("nan"), 0.1, 1, 0, 64, 48)),
    ("threshold_abs Inf", (float("inf"), 0.1, 1, 0, 64, 48)),
    ("threshold_rel NaN", (0.25, float("nan"), 1, 0, 64, 48)),
    ("threshold_rel Inf", (0.25, float("inf"), 1, 0, 64, 48)),
    ("both thresholds zero", (0.0, 0.0, 1, 0, 64, 48)),
    ("polarity 2", (0.25, 0.0, 2, 0, 64, 48)),
    ("polarity -2", (0.25, 0.0, -2, 0, 64, 48)),
    ("max_hits beyond the frame", (0.25, 0.0, 1, 64 * 48 + 1, 64, 48)),
])
def test_refusals(what, args):
    assert status(*args) == _lib.ERROR_INVALID_ARGUMENT, what


def test_a_null_setting_is_refused():
    hits, nbytes = C.c_uint32(7), C.c_size_t(7)
    assert _lib.load().paris_hip_zinger_filter_check(None, 64, 48, C.byref(hits), C.byref(nbytes)) == _lib.ERROR_INVALID_ARGUMENT
    assert (hits.value, nbytes.value) == (7, 7)   # nothing written


def test_a_frame_beyond_32_bit_pixel_indices_is_unsupported():
    assert status(0.25, 0.0, 1, 0, 1 << 16, 1 << 16) == _lib.ERROR_UNSUPPORTED
    assert status(0.25, 0.0, 1, 0, (1 << 16) - 1, 1 << 16) == _lib.SUCCESS


@pytest.mark.parametrize("dim,want", [(8, 64), (512, 1024), (2048, 16384)])
def test_default_max_hits(dim, want):
    hits, nbytes = B.zinger_filter_check(0.25, 0.0, "dark", 0, dim, dim)
    assert hits == want == Z.default_max_hits(dim, dim)
    # three 64-bit accumulators, and per frame of one launch a counter and max_hits (index, value) pairs
    frames = (nbytes - 32) // (8 * hits + 4)
    assert nbytes > 0 and nbytes == 32 + frames * (8 * hits + 4) and 1 <= frames <= _lib.ZINGER_FRAMES_MAX
    assert B.zinger_filter_check(0.25, 0.0, "dark", 5, dim, dim)[0] == 5          # an explicit value is kept
    assert B.Backend.zinger_filter_check(0.25, 0.0, -1, 0, dim, dim) == (hits, nbytes)


def test_the_mirror_raises_for_a_refused_setting():
    with pytest.raises(B.ParisHipError) as e:
        B.zinger_filter_check(0.0, 0.0, "both", 0, 64, 48)
    assert e.value.status == _lib.ERROR_INVALID_ARGUMENT


# ---- the numpy restatement itself, on frames small enough to do by hand -------------------------------------------------------------

def test_the_rule_by_hand():
    f = np.arange(9, dtype=np.float32).reshape(3, 3)
    assert np.array_equal(Z.flagged(f, 0.5, 0, 0)[1], [[1, 2, 2], [3, 4, 5], [6, 6, 7]])   # edges replicated
    f[1, 1] = 100
    out, n, saturated = Z.apply(f, 10, 0, "bright")
    assert (n, saturated) == (1, False) and out[1, 1] == 5 and np.array_equal(out != f, np.arange(9).reshape(3, 3) == 4)
    assert Z.apply(f, 10, 0, "dark")[1] == 0 and Z.apply(f, 10, 0, "both")[1] == 1
    assert Z.apply(f, 0, 20, "both")[1] == 0 and Z.apply(f, 0, 10, "both")[1] == 1        # lim = rel * |5|
    g = np.full((5, 5), 2, np.float32)
    g[1:4, 1:4] = 9                                       # a 3 x 3 blob: only its corners see fewer than five blob pixels
    assert np.array_equal(np.argwhere(Z.flagged(g, 1, 0, 0)[0]), [[1, 1], [1, 3], [3, 1], [3, 3]])
    g[0, 0] = np.nan                                      # a window with a NaN is kept
    assert np.array_equal(np.argwhere(Z.flagged(g, 1, 0, 0)[0]), [[1, 3], [3, 1], [3, 3]])
    one = np.array([[5.0]], np.float32)
    assert Z.apply(one, 0.1, 0, 0)[1] == 0                # a 1 x 1 frame: nine copies of itself


def test_saturation_leaves_the_frame_as_it_was():
    f, planted = Z.scattered_frame(40, 30, 3, share=0.02)
    n = int(Z.flagged(f, Z.T_ABS, 0, 0)[0].sum())
    assert n > 5
    out, replaced, saturated = Z.apply(f, Z.T_ABS, 0, 0, max_hits=n)
    assert (replaced, saturated) == (n, False) and np.count_nonzero(out != f) == n
    out, replaced, saturated = Z.apply(f, Z.T_ABS, 0, 0, max_hits=n - 1)
    assert (replaced, saturated) == (0, True) and np.array_equal(out.view(np.uint32), f.view(np.uint32))


@pytest.mark.parametrize("polarity", ["bright", "dark", "both"])
def test_the_shared_frame_flags_planted_pixels_only(polarity):
    f, planted = Z.planted_frame(100)
    flags, m = Z.flagged(f, Z.T_ABS, 0, polarity)
    assert flags.sum() >= 20 and not np.any(flags & ~planted)
    assert not flags[15, 46] and not flags[15, 56] and not flags[20, 71] and not flags[21, 81]   # blob centres; next to NaN / Inf


def test_quality_figures_of_the_oracle(oracle):
    """calibrates tests/test_gpu_zinger_filter.py: the numpy rule and the oracle's weight, filter and backprojection at the 64 x 48
    driver geometry. The rule applied to the CLEAN frames must change the reconstruction by less than a tenth of what it gains on the
    spiked ones: a threshold that eats skull edges fails this"""
    import defect_rule as R
    det = oracle.DetectorGeometry(*R.QUALITY_GEO)
    vg = oracle.calculate_volume_geometry(det)
    lines = R.quality_frames(vg.dim_x, vg.l_vx_x)
    spiked = Z.quality_spiked(lines)
    clean = oracle.reconstruct(det, vg, len(lines), projections=lines)

    def through_the_rule(frames):
        out = [Z.apply(p, Z.QUALITY_T_ABS, 0.0, "dark") for p in frames]
        assert not any(s for _, _, s in out)
        return [p for p, _, _ in out], sum(n for _, n, _ in out)

    filtered, n_spiked = through_the_rule(spiked)
    clean_filtered, n_clean = through_the_rule(lines)
    a = R.relative_rms(oracle.reconstruct(det, vg, len(lines), projections=spiked), clean)
    b = R.relative_rms(oracle.reconstruct(det, vg, len(lines), projections=filtered), clean)
    c = R.relative_rms(oracle.reconstruct(det, vg, len(lines), projections=clean_filtered), clean)
    print("zinger quality (oracle): relative RMS %.5g unfiltered, %.5g filtered (%d pixels replaced), %.5g clean-filtered (%d replaced)"
          % (a, b, n_spiked, c, n_clean))
    assert a == pytest.approx(Z.CAL_UNFILTERED, rel=0.02) and b == pytest.approx(Z.CAL_FILTERED, rel=0.02)
    assert c == pytest.approx(Z.CAL_CLEAN_FILTERED, abs=1e-6)
    assert c < (a - b) / 10
    assert n_spiked > 0.8 * Z.QUALITY_SHARE * 64 * 48 * len(lines)
