"""Phase retrieval on the host: paris_hip_phase_retrieval_host against the float64 restatement of
tests/phase_rule.py, the misreadings of the statement told apart, alpha, the default margin, the check with its sizes, scratch bytes and
refusals, and the figures of the physical check pinned on the float64 model and on its fp32 restatement. No device."""
import numpy as np
import pytest

import metal_rule
import phase_rule as P
from paris_amd import _lib
from paris_amd import backend as B

INV, UNS = _lib.ERROR_INVALID_ARGUMENT, _lib.ERROR_UNSUPPORTED
ALPHA, T_MIN = 2.5, 1e-6


def refused(code, f, *args):
    with pytest.raises(B.ParisHipError) as e:
        f(*args)
    return e.value.status == code


def within_one_ulp(got, want):
    """One ulp of fp32 plus the rounding of two double transforms: they differ by some 1e-13 in T' <= 1 at these sizes, T' >= 0.05
    turns that into 2e-12 in p', and 1e-11 covers it. (p' may be as small as that rounding where T' is 1: a bare ulp test of a value
    near 0 would ask double transforms of different order for the same last bits.)"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return bool(np.all(np.abs(got - want) <= np.spacing(np.maximum(np.abs(got), np.abs(want)).astype(np.float32)).astype(np.float64) + 1e-11))


@pytest.mark.parametrize("shape", P.SHAPES, ids=lambda s: "%dx%d" % s[:2])
def test_the_host_rule_is_the_float64_restatement_within_one_ulp(shape):
    dim_x, dim_y, margin, n_x, n_y, l_x, l_y = shape
    assert B.phase_retrieval_check(ALPHA, T_MIN, margin, dim_x, dim_y, l_x, l_y) == (n_x, n_y, P.scratch_bytes(dim_y, n_x))
    for p in (P.blob(dim_x, dim_y), P.ramp(dim_x, dim_y)):
        want = P.retrieve64(p, ALPHA, T_MIN, margin, l_x, l_y)
        assert np.exp(-float(want.max())) >= 0.05, "no pixel near the floor"
        got = B.phase_retrieval_host(ALPHA, T_MIN, margin, l_x, l_y, p)
        assert got.dtype == np.float32 and got.shape == p.shape and within_one_ulp(got, want)
        if dim_x * dim_y > 1:
            assert not within_one_ulp(got, p), "the filter changes the frame"


@pytest.mark.parametrize("wrong", P.WRONG)
def test_every_misreading_of_the_statement_is_told_apart(wrong):
    """on the 61 x 45 frame with anisotropic pitches (N - dim is odd on both axes) and a floor of 0.5 that pixels reach"""
    dim_x, dim_y, margin, _, _, l_x, l_y = P.SHAPES[2]
    for p in (P.blob(dim_x, dim_y), P.ramp(dim_x, dim_y)):
        got = B.phase_retrieval_host(ALPHA, 0.5, margin, l_x, l_y, p)
        assert within_one_ulp(got, P.retrieve64(p, ALPHA, 0.5, margin, l_x, l_y))
        assert not within_one_ulp(got, P.retrieve64(p, ALPHA, 0.5, margin, l_x, l_y, wrong=wrong))


def test_a_constant_frame_returns_itself():
    for dim_x, dim_y, value in ((1, 1, 0.5), (7, 5, 0.0), (7, 5, 1.25), (33, 2, 3.0)):
        p = np.full((dim_y, dim_x), value, np.float32)
        assert np.array_equal(B.phase_retrieval_host(ALPHA, T_MIN, 3, 0.4, 0.9, p), p)


def test_special_pixels_are_left_as_stored_and_enter_as_air():
    p = P.blob(21, 13)
    special = {(2, 3): np.nan, (5, 7): np.inf, (6, 1): -np.inf, (9, 20): -200.0}
    for at, v in special.items():
        p[at] = v
    got = B.phase_retrieval_host(ALPHA, T_MIN, 4, 1.0, 1.0, p)
    air = p.copy()
    for at in special:
        air[at] = 0.0
    want = P.retrieve64(air, ALPHA, T_MIN, 4, 1.0, 1.0)
    for at in special:
        assert got[at] == p[at] or (np.isnan(got[at]) and np.isnan(p[at]))
    keep = P.entered(p)
    assert np.count_nonzero(~keep) == len(special)
    assert within_one_ulp(got[keep], want[keep])
    # below the floor: -log(t_min) everywhere
    deep = B.phase_retrieval_host(ALPHA, T_MIN, 4, 1.0, 1.0, np.full((5, 9), 20.0, np.float32))
    assert within_one_ulp(deep, np.full((5, 9), -np.log(float(np.float32(T_MIN))), np.float32))


def test_alpha_is_the_formula_in_double_rounded_once():
    for geo, db, e in (((64, 32, 1.0, 1.0, 0, 0, 500.0, 500.0, 3.0), 1000.0, 30.0), ((8, 8, .1, .1, 0, 0, -120.0, 880.0, 1.0), 2400.0, 18.5),
                       ((8, 8, .1, .1, 0, 0, 35.5, -700.25, 1.0), 350.0, 60.0)):
        got = B.phase_alpha(B.DetectorGeometry(*geo), db, e)
        assert np.float32(got) == P.alpha(geo, db, e) and got > 0
    det = B.DetectorGeometry(64, 32, 1.0, 1.0, 0, 0, 500.0, 500.0, 3.0)
    assert abs(B.phase_alpha(det, 1000.0, 30.0) - np.pi * 1.2398419843e-6 / 30.0 * 1000.0 * 500.0 * 2.0) < 1e-8
    for db, e in ((0.0, 30.0), (-1.0, 30.0), (np.nan, 30.0), (np.inf, 30.0), (100.0, 0.0), (100.0, -2.0), (100.0, np.nan), (1e300, 1e-300)):
        assert refused(INV, B.phase_alpha, det, db, e)
    for d_so, d_od in ((0.0, 500.0), (500.0, 0.0), (np.nan, 500.0), (500.0, np.inf)):
        assert refused(INV, B.phase_alpha, B.DetectorGeometry(64, 32, 1.0, 1.0, 0, 0, d_so, d_od, 3.0), 100.0, 30.0)


def test_the_default_margin():
    for a, l_x, l_y in ((16.0, 1.0, 1.0), (4.0, 1.0, 1.0), (400.0, 0.1, 0.2), (400.0, 0.2, 0.1), (1e-3, 0.05, 0.05), (3.7, 0.0123, 0.4), (1e6, 0.01, 0.01)):
        assert B.phase_default_margin(a, l_x, l_y) == P.default_margin(a, l_x, l_y)
    assert B.phase_default_margin(16.0, 1.0, 1.0) == 8
    assert B.phase_default_margin(1e6, 0.01, 0.01) == P.MARGIN_MAX
    for a, l_x, l_y in ((0.0, 1.0, 1.0), (-1.0, 1.0, 1.0), (np.nan, 1.0, 1.0), (1.0, 0.0, 1.0), (1.0, 1.0, np.inf)):
        assert B.phase_default_margin(a, l_x, l_y) == 0


def test_the_check_sizes_scratch_and_refusals():
    ok = (ALPHA, T_MIN, 8, 61, 45, 0.7, 1.1)
    assert B.phase_retrieval_check(*ok) == (128, 64, 16 * 45 * 65 * 8)
    assert B.phase_retrieval_check(ALPHA, 1.0, 1, 1, 1, 1.0, 1.0) == (8, 8, 16 * 5 * 8)
    assert B.phase_retrieval_check(ALPHA, T_MIN, 24, 2048, 2048, 0.1, 0.1) == (4096, 4096, 2048 * 2049 * 8)         # 64 MiB hold one such frame
    assert B.phase_retrieval_check(ALPHA, T_MIN, 24, 1024, 1024, 0.1, 0.1) == (2048, 2048, 7 * 1024 * 1025 * 8)     # ... seven of these
    assert B.phase_retrieval_check(ALPHA, T_MIN, 1024, 6144, 6144, 0.1, 0.1) == (8192, 8192, 6144 * 4097 * 8)      # ... and not one of these: one frame all the same
    assert B.phase_retrieval_check(ALPHA, T_MIN, 1, 8190, 6, 0.1, 0.1)[:2] == (8192, 8)

    def but(**kw):
        names = ("alpha", "t_min", "margin", "dim_x", "dim_y", "l_x", "l_y")
        return tuple(kw.get(n, v) for n, v in zip(names, ok))

    for bad in (but(alpha=0.0), but(alpha=-1.0), but(alpha=np.nan), but(alpha=np.inf), but(t_min=0.0), but(t_min=-0.5), but(t_min=1.5),
                but(t_min=np.nan), but(margin=0), but(margin=P.MARGIN_MAX + 1), but(dim_x=0), but(dim_y=0), but(l_x=0.0), but(l_x=np.nan),
                but(l_y=-1.0), but(l_y=np.inf)):
        assert refused(INV, B.phase_retrieval_check, *bad), bad
    for big in (but(dim_x=8191), but(dim_y=8200, margin=1), but(dim_x=7000, margin=P.MARGIN_MAX)):
        assert refused(UNS, B.phase_retrieval_check, *big), big
    assert refused(UNS, B.phase_retrieval_host, ALPHA, T_MIN, 1, 1.0, 1.0, np.zeros((2, 8191), np.float32))
    n_x, n_y = _lib.C.c_uint32(), _lib.C.c_uint32()
    s = _lib.PhaseRetrieval(ALPHA, T_MIN, 1)
    assert _lib.load().paris_hip_phase_retrieval_check(_lib.C.byref(s), 8191, 9, 1.0, 1.0, _lib.C.byref(n_x), _lib.C.byref(n_y), None) == UNS
    assert (n_x.value, n_y.value) == (16384, 16), "the refusal still names the size"
    assert _lib.load().paris_hip_phase_retrieval_check(None, 8, 8, 1.0, 1.0, None, None, None) == INV
    assert _lib.load().paris_hip_phase_retrieval_host(_lib.C.byref(s), 1.0, 1.0, None, None, 4, 4) == INV


# ---- the physical check, on the models ----------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def scene():
    det, vg = B.DetectorGeometry(*P.SCENE_DET), B.VolumeGeometry(*P.SCENE_GRID)
    frames = P.scene_frames()
    return det, vg, frames, metal_rule.reconstruct64(frames, det, vg)


def scene_figures(scene, alpha, retrieve, noise=0.0):
    det, vg, frames, exact = scene
    margin = B.phase_default_margin(alpha, det.l_px_row, det.l_px_col)
    f = P.fringed(frames, alpha, noise)
    t = np.exp(-f.astype(np.float64))
    assert margin == 8 and (noise or (0.45 <= t.min() and t.max() <= 1.17))
    before = P.scene_rms(metal_rule.reconstruct64(f, det, vg), exact)
    after = [P.scene_rms(metal_rule.reconstruct64(np.stack([r(x, alpha, P.SCENE_T_MIN, margin, 1.0, 1.0) for x in f]), det, vg), exact)
             for r in retrieve]
    print("phase retrieval, scene: alpha %g noise %g: fringed %.4g, retrieved %s" % (alpha, noise, before, ["%.4g" % a for a in after]))
    return before, after


def test_the_scene_at_alpha_16_on_the_float64_model_and_its_fp32_restatement(scene):
    """Measured: the largest line integral is 0.778; fringed 4.804e-3, retrieved 7.995e-7 (float64 model, and the C host rule to every
    digit shown) and 7.998e-7 (fp32 restatement): ratios 1.664e-4 and 1.665e-4. The residue is the fp32 rounding of the stored frames."""
    assert abs(float(scene[2].max()) - 0.78) < 0.005
    before, (r64, r32) = scene_figures(scene, 16.0, (P.retrieve64, P.retrieve32))
    assert before == pytest.approx(4.80e-3, rel=0.01) and r64 == pytest.approx(8.0e-7, rel=0.02) and r32 == pytest.approx(8.0e-7, rel=0.02)
    assert r64 / before == pytest.approx(1.7e-4, rel=0.05) and r32 / before == pytest.approx(1.665e-4, rel=0.02)


def test_the_scene_at_alpha_4_and_the_c_host_rule(scene):
    """Measured: fringed 1.217e-3, retrieved 2.176e-7 by the float64 model and by paris_hip_phase_retrieval_host alike."""
    def host(x, alpha, t_min, margin, l_x, l_y):
        return B.phase_retrieval_host(alpha, t_min, margin, l_x, l_y, x)
    before, (r64, rc) = scene_figures(scene, 4.0, (P.retrieve64, host))
    assert before == pytest.approx(1.22e-3, rel=0.01) and r64 == pytest.approx(2.2e-7, rel=0.02) and rc == pytest.approx(r64, rel=1e-3)


def test_the_scene_with_noise(scene):
    """Gaussian noise of 0.01 on I at alpha 16. Measured: fringed 4.985e-3, retrieved 4.051e-4, ratio 0.0813 -- the low-pass is the gain."""
    before, (r64,) = scene_figures(scene, 16.0, (P.retrieve64,), noise=0.01)
    assert r64 / before == pytest.approx(0.081, rel=0.02)
