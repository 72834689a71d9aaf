"""Scatter correction on the host: paris_hip_scatter_correction_host against the float64 restatement of
tests/scatter_rule.py, the misreadings of the statement told apart, air, special pixels, the default margin, the check with its sizes,
scratch bytes and refusals, and the figures of the physical check pinned on the float64 model and on its fp32 restatement. No device."""
import numpy as np
import pytest

import metal_rule
import scatter_rule as S
from paris_amd import _lib
from paris_amd import backend as B

P = S.P
INV, UNS = _lib.ERROR_INVALID_ARGUMENT, _lib.ERROR_UNSUPPORTED


def refused(code, f, *args):
    with pytest.raises(B.ParisHipError) as e:
        f(*args)
    return e.value.status == code


def within_one_ulp(got, want):
    """One ulp of fp32 plus the rounding of the double transforms of every iteration: they differ by some 1e-13 in S at these sizes,
    T^n >= 0.05 turns that into 2e-12 in p', and 1e-11 covers it (as tests/test_phase_host.py argues for its filter)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return bool(np.all(np.abs(got - want) <= np.spacing(np.maximum(np.abs(got), np.abs(want)).astype(np.float32)).astype(np.float64) + 1e-11))


@pytest.mark.parametrize("shape", S.SHAPES, ids=lambda s: "%dx%d" % s[:2])
def test_the_host_rule_is_the_float64_restatement_within_one_ulp(shape):
    dim_x, dim_y, margin, n_x, n_y, l_x, l_y = shape
    setting = S.setting_for(l_x, 4, margin)
    assert B.scatter_correction_check(setting, dim_x, dim_y, l_x, l_y) == (n_x, n_y, P.scratch_bytes(dim_y, n_x))
    for p in (S.smooth(dim_x, dim_y), S.ramp(dim_x, dim_y)):
        want = S.correct64(p, setting, l_x, l_y)
        assert np.exp(-float(want.max())) >= 0.05 and S.fraction(p, setting, l_x, l_y).max() < 0.5, "no pixel at the clamp"
        got = B.scatter_correction_host(setting, l_x, l_y, p)
        assert got.dtype == np.float32 and got.shape == p.shape and within_one_ulp(got, want)
        assert not within_one_ulp(got, p), "the correction changes the frame"


@pytest.mark.parametrize("iterations", [1, 2, 3, 16])
def test_every_iteration_count_is_the_restatement_s(iterations):
    dim_x, dim_y, margin, _, _, l_x, l_y = S.SHAPES[2]
    setting = S.setting_for(l_x, iterations, margin)
    p = P.ramp(dim_x, dim_y)                            # unscaled: pixels end at the clamp
    assert within_one_ulp(B.scatter_correction_host(setting, l_x, l_y, p), S.correct64(p, setting, l_x, l_y))


@pytest.mark.parametrize("wrong", S.WRONG)
def test_every_misreading_of_the_statement_is_told_apart(wrong):
    """on the 61 x 45 frame with anisotropic pitches, on the unscaled ramp, where 8 % of the pixels end at the clamp"""
    dim_x, dim_y, margin, _, _, l_x, l_y = S.SHAPES[2]
    setting = S.setting_for(l_x, 4, margin)
    p = P.ramp(dim_x, dim_y)
    share = float(np.mean(S.fraction(p, setting, l_x, l_y) >= S.f32(setting[6]) - 1e-9))
    assert 0.02 <= share <= 0.30
    got = B.scatter_correction_host(setting, l_x, l_y, p)
    assert within_one_ulp(got, S.correct64(p, setting, l_x, l_y))
    assert not within_one_ulp(got, S.correct64(p, setting, l_x, l_y, wrong=wrong))


def test_one_gaussian_is_two_with_a_weight_of_zero():
    dim_x, dim_y, margin, _, _, l_x, l_y = S.SHAPES[5]
    p = S.smooth(dim_x, dim_y)
    one = (0.02, -0.15, 1.0, 3.0, 3.0, 0.0, 0.6, 4, margin)
    other_width = one[:4] + (77.0,) + one[5:]
    got = B.scatter_correction_host(one, l_x, l_y, p)
    assert within_one_ulp(got, S.correct64(p, one, l_x, l_y)) and np.array_equal(got, B.scatter_correction_host(other_width, l_x, l_y, p))


def test_a_frame_of_air_returns_itself_exactly():
    """p = 0: T = 1, L = 0, no source, S = 0, T^n = T_m, p' = -log(1), the value 0 (with the sign the negation gives it)."""
    for dim_x, dim_y in ((1, 1), (7, 5), (33, 2)):
        p = np.zeros((dim_y, dim_x), np.float32)
        got = B.scatter_correction_host(S.setting_for(1.0, 4, 3), 0.4, 0.9, p)
        assert np.array_equal(got, p)
    # a negative line integral (T_m > 1) carries no source either: a frame of them comes back within the rounding of exp and log
    p = np.full((5, 7), -0.25, np.float32)
    assert within_one_ulp(B.scatter_correction_host(S.setting_for(1.0, 4, 3), 0.4, 0.9, p), p)


def test_special_pixels_are_left_as_stored_and_enter_as_air():
    p = S.smooth(21, 13)
    special = {(2, 3): np.nan, (5, 7): np.inf, (6, 1): -np.inf, (9, 20): -200.0, (11, 4): 200.0}   # expf(200) = inf, expf(-200) = 0
    for at, v in special.items():
        p[at] = v
    setting = S.setting_for(1.0, 4, 4)
    got = B.scatter_correction_host(setting, 1.0, 1.0, p)
    air = p.copy()
    for at in special:
        air[at] = 0.0
    want = S.correct64(air, setting, 1.0, 1.0)
    for at in special:
        assert got[at] == p[at] or (np.isnan(got[at]) and np.isnan(p[at]))
    keep = S.entered(p)
    assert np.count_nonzero(~keep) == len(special)
    assert within_one_ulp(got[keep], want[keep]) and within_one_ulp(got[keep], S.correct64(p, setting, 1.0, 1.0)[keep])


def test_the_default_margin():
    for s1, s2, l_x, l_y in ((4.0, 16.0, 1.0, 1.0), (16.0, 4.0, 1.0, 1.0), (1.0, 1.0, 1.0, 1.0), (0.3, 1.0, 0.1, 0.2), (0.3, 1.0, 0.2, 0.1),
                             (3.7, 0.2, 0.0123, 0.4), (1e3, 1.0, 0.01, 0.01)):
        assert B.scatter_default_margin(s1, s2, l_x, l_y) == S.default_margin(s1, s2, l_x, l_y)
    assert B.scatter_default_margin(4.0, 16.0, 1.0, 1.0) == 48 and B.scatter_default_margin(1.0, 1.0, 1.0, 1.0) == 8
    assert B.scatter_default_margin(1e3, 1.0, 0.01, 0.01) == P.MARGIN_MAX
    for bad in ((0.0, 1.0, 1.0, 1.0), (1.0, -1.0, 1.0, 1.0), (np.nan, 1.0, 1.0, 1.0), (1.0, 1.0, 0.0, 1.0), (1.0, 1.0, 1.0, np.inf)):
        assert B.scatter_default_margin(*bad) == 0


def test_the_check_sizes_scratch_and_refusals():
    names = ("amplitude", "alpha", "beta", "sigma1", "sigma2", "w2", "limit", "iterations", "margin")
    ok = (0.02, -0.15, 1.0, 2.1, 7.0, 0.5, 0.6, 4, 8)

    def but(**kw):
        return tuple(kw.get(n, v) for n, v in zip(names, ok))

    assert B.scatter_correction_check(ok, 61, 45, 0.7, 1.1) == (128, 64, 16 * 45 * 65 * 8)
    assert B.scatter_correction_check(but(margin=1), 1, 1, 1.0, 1.0) == (8, 8, 16 * 5 * 8)
    assert B.scatter_correction_check(but(margin=24), 2048, 2048, 0.1, 0.1) == (4096, 4096, 2048 * 2049 * 8)
    assert B.scatter_correction_check(but(margin=24), 1024, 1024, 0.1, 0.1) == (2048, 2048, 7 * 1024 * 1025 * 8)
    # the ends of every range are inside
    for good in (but(alpha=-2.0), but(alpha=2.0), but(beta=0.0), but(beta=4.0), but(w2=0.0), but(iterations=1), but(iterations=S.ITERATIONS_MAX),
                 but(margin=1), but(margin=P.MARGIN_MAX), but(limit=0.999), but(limit=1e-3)):
        assert B.scatter_correction_check(good, 61, 45, 0.7, 1.1)[:2] == (P.padded(61, good[8]), P.padded(45, good[8]))
    for bad in (but(amplitude=0.0), but(amplitude=-1.0), but(amplitude=np.nan), but(amplitude=np.inf), but(alpha=-2.5), but(alpha=2.5),
                but(alpha=np.nan), but(beta=-0.1), but(beta=4.5), but(beta=np.nan), but(sigma1=0.0), but(sigma1=np.inf), but(sigma2=-1.0),
                but(sigma2=np.nan), but(w2=-0.1), but(w2=np.inf), but(w2=np.nan), but(limit=0.0), but(limit=1.0), but(limit=np.nan),
                but(iterations=0), but(iterations=S.ITERATIONS_MAX + 1), but(margin=0), but(margin=P.MARGIN_MAX + 1)):
        assert refused(INV, B.scatter_correction_check, bad, 61, 45, 0.7, 1.1), bad
    for dims in ((0, 45, 0.7, 1.1), (61, 0, 0.7, 1.1), (61, 45, 0.0, 1.1), (61, 45, np.nan, 1.1), (61, 45, 0.7, -1.0), (61, 45, 0.7, np.inf)):
        assert refused(INV, B.scatter_correction_check, ok, *dims), dims
    for big in ((8191, 45, ok), (61, 8200, but(margin=1)), (7000, 45, but(margin=P.MARGIN_MAX))):
        assert refused(UNS, B.scatter_correction_check, big[2], big[0], big[1], 0.7, 1.1), big
    assert refused(UNS, B.scatter_correction_host, but(margin=1), 1.0, 1.0, np.zeros((2, 8191), np.float32))
    n_x, n_y = _lib.C.c_uint32(), _lib.C.c_uint32()
    s = _lib.ScatterCorrection(*but(margin=1))
    assert _lib.load().paris_hip_scatter_correction_check(_lib.C.byref(s), 8191, 9, 1.0, 1.0, _lib.C.byref(n_x), _lib.C.byref(n_y), None) == UNS
    assert (n_x.value, n_y.value) == (16384, 16), "the refusal still names the size"
    assert _lib.load().paris_hip_scatter_correction_check(None, 8, 8, 1.0, 1.0, None, None, None) == INV
    assert _lib.load().paris_hip_scatter_correction_host(_lib.C.byref(s), 1.0, 1.0, None, None, 4, 4) == INV


# ---- the physical check, on the models ----------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def scene():
    det, vg = B.DetectorGeometry(*S.SCENE_DET), B.VolumeGeometry(*S.SCENE_GRID)
    frames = S.scene_frames()
    return det, vg, frames, metal_rule.reconstruct64(frames, det, vg)


def scene_figures(scene, iterations, correct):
    det, vg, frames, exact = scene
    setting = S.scene_setting(iterations)
    f, ratio = S.scattered(frames, setting)
    assert ratio == pytest.approx(0.125, abs=5e-4), "the largest scatter-to-primary ratio"
    before = S.scene_rms(metal_rule.reconstruct64(f, det, vg), exact)
    after = [S.scene_rms(metal_rule.reconstruct64(np.stack([c(x, setting, det.l_px_row, det.l_px_col) for x in f]), det, vg), exact) for c in correct]
    print("scatter correction, scene, %d iteration(s): scattered %.4g, corrected %s" % (iterations, before, ["%.4g" % a for a in after]))
    return before, after


def test_the_scene_on_the_float64_model_its_fp32_restatement_and_the_c_host_rule(scene):
    """Measured: scattered 1.510e-3, corrected 7.977e-7 by the float64 model and by paris_hip_scatter_correction_host alike: ratio
    5.283e-4; the fp32 restatement leaves 7.979e-7, ratio 5.285e-4. The residue is the fp32 rounding of the stored frames."""
    def host(x, setting, l_x, l_y):
        return B.scatter_correction_host(setting, l_x, l_y, x)
    before, (r64, rc, r32) = scene_figures(scene, 4, (S.correct64, host, S.correct32))
    assert before == pytest.approx(1.510e-3, rel=0.01) and r64 == pytest.approx(7.977e-7, rel=0.02) and rc == pytest.approx(r64, rel=1e-3)
    assert r64 / before == pytest.approx(S.SCENE_RATIO_64, rel=0.02) and r32 / before == pytest.approx(S.SCENE_RATIO_32, rel=0.02)


@pytest.mark.parametrize("iterations,ratio", [(1, 0.152), (2, 0.0231)])
def test_the_scene_converges_as_the_model_says(scene, iterations, ratio):
    before, (r64,) = scene_figures(scene, iterations, (S.correct64,))
    assert r64 / before == pytest.approx(ratio, rel=0.01)
