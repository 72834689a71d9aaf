"""Scatter correction on the device: paris_hip_scatter_correction_frames against the float64 restatement of
tests/scatter_rule.py, with the error of the fp32 restatement as the yardstick -- every size class of the launcher --, the clamp, the
iterations one by one, a frame's bits whatever shares its call, canvases, special pixels, more frames than a round of launches
serves, the contracts of a ctx-owned setting and of a frame pass, and the physical check: scatter of the forward model removed from
a reconstruction."""
import numpy as np
import pytest

import metal_rule
import scatter_rule as S
import test_gpu_defect_map as DM
import test_gpu_detector_roll as DR
from paris_amd import _lib
from paris_amd import backend as B

pytestmark = pytest.mark.gpu

P = S.P
bits, read, pending = DM.bits, DM.read, DM.pending
INV, UNS = _lib.ERROR_INVALID_ARGUMENT, _lib.ERROR_UNSUPPORTED
FACTOR = 4.0     # DESIGN.md section 4.22's, on the same grounds: another radix and butterfly order, table twiddles, the device's expf / logf


@pytest.fixture(scope="module")
def be():
    with B.Backend(0) as b:
        yield b
        b.clear_scatter_correction()


def correct(be, frames, n_frames=None):
    """the frames stacked in one buffer, corrected by one call (the setting is in place); returns them as a list"""
    dim_y, dim_x = frames[0].shape
    d = be.make_projection_device(dim_x, dim_y * len(frames))
    be.upload_raw(np.ascontiguousarray(np.vstack(frames), np.float32), d)
    be.scatter_correction(be.wrap_projection(d.ptr, d.pitch, dim_x, dim_y), d.pitch * dim_y, len(frames) if n_frames is None else n_frames)
    out = read(be, d)
    be.free(d)
    return [out[k * dim_y:(k + 1) * dim_y] for k in range(len(frames))]


def refused(code, f, *args, **kw):
    with pytest.raises(B.ParisHipError) as e:
        f(*args, **kw)
    return e.value.status == code


def within_the_bound(name, got, p, setting, l_x, l_y, where=None):
    e_dev = S.error(got, p, setting, l_x, l_y, where)
    e_32 = S.error(S.correct32(p, setting, l_x, l_y), p, setting, l_x, l_y, where)
    print("scatter correction %s: E(device) %.3g, E(correct32) %.3g, ratio %.3g" % (name, e_dev, e_32, e_dev / e_32 if e_32 else 0.0))
    return e_dev <= FACTOR * e_32


# ---- 1. the rule, within FFT rounding -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", S.SHAPES, ids=lambda s: "%dx%d" % s[:2])
def test_the_device_keeps_four_times_the_error_of_the_fp32_restatement(be, shape):
    """E(x) = max |exp(-x) - T64^n| over the pixels that entered; E(device) <= 4 E(correct32), both evaluated here on the same input, at
    A = 0.02, alpha = -0.15, beta = 1, sigma = 3 and 10 pixels, w2 = 0.5, limit = 0.6, 4 iterations. The clamp is idle (the largest
    scatter fraction is below 0.5) and the frame changes by more than 1e-3 (but for the 1 x 1 ramp, whose one pixel holds p = 0.04).
    DESIGN.md section 4.23 has the measured table."""
    dim_x, dim_y, margin, n_x, n_y, l_x, l_y = shape
    setting = S.setting_for(l_x, 4, margin)
    be.set_scatter_correction(setting, dim_x, dim_y, l_x, l_y)
    for name, p in (("smooth", S.smooth(dim_x, dim_y)), ("ramp", S.ramp(dim_x, dim_y))):
        assert S.fraction(p, setting, l_x, l_y).max() < 0.5, "the clamp is idle"
        got, = correct(be, [p])
        assert within_the_bound("%d x %d -> %d x %d, %s" % (dim_x, dim_y, n_x, n_y, name), got, p, setting, l_x, l_y)
        if dim_x * dim_y > 1:
            assert np.abs(got - p).max() > 1e-3, "the correction changes the frame"


def test_the_clamp(be):
    """the unscaled ramp at 61 x 45: in float64 8.2 % of the pixels end at (1 - limit) T_m; the device's pixels there keep the bound"""
    dim_x, dim_y, margin, _, _, l_x, l_y = S.SHAPES[2]
    setting = S.setting_for(l_x, 4, margin)
    p = P.ramp(dim_x, dim_y)
    clamped = S.fraction(p, setting, l_x, l_y) >= S.f32(setting[6]) - 1e-9
    assert 0.02 <= clamped.mean() <= 0.30
    be.set_scatter_correction(setting, dim_x, dim_y, l_x, l_y)
    got, = correct(be, [p])
    assert within_the_bound("61 x 45, clamped pixels", got, p, setting, l_x, l_y, clamped)
    assert within_the_bound("61 x 45, every pixel", got, p, setting, l_x, l_y)


def test_air_returns_itself(be):
    be.set_scatter_correction(S.setting_for(1.0, 4, 3), 7, 5, 0.4, 0.9)
    got, = correct(be, [np.zeros((5, 7), np.float32)])
    assert np.array_equal(got, np.zeros((5, 7), np.float32))     # expf(0) = 1, logf(1) = 0: no source, no scatter, -logf(1)


# ---- 2. the iterations are executed -----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def scene():
    det, vg = B.DetectorGeometry(*S.SCENE_DET), B.VolumeGeometry(*S.SCENE_GRID)
    frames = S.scene_frames()
    return det, vg, frames, metal_rule.reconstruct64(frames, det, vg)


def test_one_two_and_four_iterations_differ_and_each_matches_its_restatement(be, scene):
    det, _, frames, _ = scene
    p = S.scattered(frames[:1], S.scene_setting())[0][0]
    got = {}
    for n in (1, 2, 4):
        setting = S.scene_setting(n)
        be.set_scatter_correction(setting, det.n_row, det.n_col, det.l_px_row, det.l_px_col)
        got[n], = correct(be, [p])
        assert within_the_bound("scene frame, %d iteration(s)" % n, got[n], p, setting, det.l_px_row, det.l_px_col)
    # in the model the steps from 1 to 2 and from 2 to 4 iterations are 1.6e-2 and 2.9e-3 in p: far above the bound's 1e-6
    assert np.abs(got[1] - got[2]).max() > 1e-2 and np.abs(got[2] - got[4]).max() > 1e-3


# ---- 3. a frame's bits do not depend on its company -----------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [S.SHAPES[0], S.SHAPES[2], S.SHAPES[4]], ids=lambda s: "%dx%d" % s[:2])
def test_a_frame_alone_equals_the_frame_anywhere_among_three(be, shape):
    dim_x, dim_y, margin, _, _, l_x, l_y = shape
    be.set_scatter_correction(S.setting_for(l_x, 4, margin), dim_x, dim_y, l_x, l_y)
    a, b, c = S.smooth(dim_x, dim_y), P.ramp(dim_x, dim_y), S.smooth(dim_x, dim_y, seed=3) * np.float32(0.5)
    alone, = correct(be, [a])
    assert np.abs(alone - a).max() > 1e-3
    for frames, at in (([a, b, c], 0), ([b, a, c], 1), ([b, c, a], 2), ([a, b], 0), ([c, a], 1)):
        got = correct(be, frames)
        assert np.array_equal(bits(got[at]), bits(alone)), at
    # n_frames 1 and 2 of three: the frames beyond stay as they were
    for n in (1, 2):
        got = correct(be, [a, b, c], n_frames=n)
        assert np.array_equal(bits(got[0]), bits(alone))
        assert all(np.array_equal(bits(g), bits(f)) for g, f in list(zip(got, [a, b, c]))[n:])


def test_more_frames_than_a_round_of_launches_serves(be):
    """70 frames of 5 x 3 in one call: the scratch holds 16, the call loops five times, and every frame has the bits it has alone"""
    dim_x, dim_y, margin, _, _, l_x, l_y = S.SHAPES[0]
    setting = S.setting_for(l_x, 4, margin)
    be.set_scatter_correction(setting, dim_x, dim_y, l_x, l_y)
    assert B.scatter_correction_check(setting, dim_x, dim_y, l_x, l_y)[2] == 16 * dim_y * 5 * 8
    frames = [S.smooth(dim_x, dim_y, seed=k) for k in range(70)]
    got = correct(be, frames)
    for k in (0, 15, 16, 31, 32, 63, 64, 69):
        alone, = correct(be, [frames[k]])
        assert np.array_equal(bits(got[k]), bits(alone)) and np.abs(alone - frames[k]).max() > 1e-3, k


# ---- 4. canvases ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", [DR.ALIGNED, DR.ALIGNED_WIDE, DR.SCALAR, DR.SCALAR_WIDE], ids=["aligned", "aligned_wide", "scalar", "scalar_wide"])
def test_every_byte_outside_the_frames_comes_back_as_it_went(be, layout):
    dim_x, dim_y, margin, _, _, l_x, l_y = S.SHAPES[5]
    be.set_scatter_correction(S.setting_for(l_x, 4, margin), dim_x, dim_y, l_x, l_y)
    frames = [S.smooth(dim_x, dim_y), P.ramp(dim_x, dim_y), S.smooth(dim_x, dim_y, seed=8)]
    want_frames = [correct(be, [f])[0] for f in frames]
    off, pitch, stride, n_bytes = layout(3, dim_x, dim_y)
    host = np.full(((n_bytes + 255) // 256) * 64, DR.SENTINEL, np.uint32).view(np.float32)
    want = host.copy()
    for k in range(3):
        DR.place(host, off + k * stride, pitch, frames[k])
        DR.place(want, off + k * stride, pitch, want_frames[k])
    canvas = DR.Canvas(be, n_bytes, host.copy())
    be.scatter_correction(canvas.view(off, pitch, dim_x, dim_y), stride, 3)
    got = canvas.read()
    canvas.free()
    assert np.array_equal(bits(got), bits(want))


# ---- 5. special pixels ------------------------------------------------------------------------------------------------------------------

def test_special_pixels_are_left_as_stored_and_their_neighbours_see_air(be):
    setting = S.setting_for(1.0, 4, 4)
    be.set_scatter_correction(setting, 21, 13, 1.0, 1.0)
    p = S.smooth(21, 13)
    special = {(2, 3): np.nan, (5, 7): np.inf, (6, 1): -np.inf, (9, 20): -200.0, (11, 4): 200.0, (12, 0): np.nan}
    for at, v in special.items():
        p[at] = v
    air = p.copy()
    for at in special:
        air[at] = 0.0
    got, = correct(be, [p])
    for at in special:
        assert bits(got)[at] == bits(p)[at], at
    keep = S.entered(p)
    assert np.count_nonzero(~keep) == len(special)
    # the frame with air in their place is the same frame to every other pixel, bit for bit ...
    got_air, = correct(be, [air])
    assert np.array_equal(bits(got)[keep], bits(got_air)[keep])
    # ... and that one keeps the bound
    assert within_the_bound("21 x 13, special pixels as air", got_air, air, setting, 1.0, 1.0, keep)


# ---- 6. contracts -----------------------------------------------------------------------------------------------------------------------

OK = S.setting_for(0.7, 4, 8)


def but(**kw):
    names = ("amplitude", "alpha", "beta", "sigma1", "sigma2", "w2", "limit", "iterations", "margin")
    return tuple(kw.get(n, v) for n, v in zip(names, OK))


def test_the_refusals(be):
    be.set_scatter_correction(OK, 61, 45, 0.7, 1.1)
    d, other = be.make_projection_device(61, 45), be.make_projection_device(60, 45)
    be.scatter_correction(d)
    assert refused(INV, be.scatter_correction, other)
    assert refused(INV, be.scatter_correction, be.wrap_projection(d.ptr, d.pitch, 61, 44))
    assert refused(INV, be.scatter_correction, be.wrap_projection(d.ptr, 61 * 4 - 4, 61, 45))
    assert refused(INV, be.scatter_correction, d, 45 * d.pitch - 4, 2)
    for bad in (but(amplitude=0.0), but(amplitude=np.nan), but(alpha=2.5), but(beta=-1.0), but(sigma1=0.0), but(sigma2=np.inf), but(w2=-1.0),
                but(limit=0.0), but(limit=1.0), but(iterations=0), but(iterations=S.ITERATIONS_MAX + 1), but(margin=0), but(margin=P.MARGIN_MAX + 1)):
        assert refused(INV, be.set_scatter_correction, bad, 61, 45, 0.7, 1.1), bad
    assert refused(INV, be.set_scatter_correction, OK, 61, 45, 0.0, 1.1)
    assert refused(UNS, be.set_scatter_correction, OK, 8180, 45, 0.7, 1.1)
    be.scatter_correction(d)                       # a refused setting leaves the one in place
    be.clear_scatter_correction()
    assert refused(INV, be.scatter_correction, d)
    be.free(d)
    be.free(other)


def test_the_reserve_counts_the_setting():
    with B.Backend(0) as b:
        without = b.projection_reserve_bytes(61, 45)
        b.set_scatter_correction(OK, 61, 45, 0.7, 1.1)
        n_x, n_y, scratch = B.scatter_correction_check(OK, 61, 45, 0.7, 1.1)
        assert b.projection_reserve_bytes(61, 45) == without + scratch + 12 * (n_x + n_y)     # twiddles 4 N, tables 8 N bytes an axis
        b.set_scatter_correction(but(margin=1), 5, 3, 1.0, 1.0)
        assert b.projection_reserve_bytes(61, 45) == without + 16 * 3 * 5 * 8 + 12 * 16
        # the phase retrieval's setting is another one: each keeps its own scratch
        b.set_phase_retrieval(2.5, 1e-6, 1, 5, 3, 1.0, 1.0)
        assert b.projection_reserve_bytes(61, 45) == without + 2 * 16 * 3 * 5 * 8 + (12 + 8) * 16
        b.clear_phase_retrieval()
        b.clear_scatter_correction()
        assert b.projection_reserve_bytes(61, 45) == without


def test_a_replaced_setting_leaves_queued_work_on_the_old_one(be):
    dim_x, dim_y, margin, l_x, l_y = 500, 350, 24, 0.2, 0.2          # 1024 x 512: long enough to be queued behind one another
    p = S.smooth(dim_x, dim_y)
    setting = S.setting_for(l_x, 4, margin)
    be.set_scatter_correction(setting, dim_x, dim_y, l_x, l_y)
    want, = correct(be, [p])
    with B.Backend(0, synchronous=False) as abe:
        abe.set_scatter_correction(setting, dim_x, dim_y, l_x, l_y)
        d = [abe.make_projection_device(dim_x, dim_y) for _ in range(4)]
        for x in d:
            abe.upload_raw(p, x)
        for x in d:
            abe.scatter_correction(x)                               # queued ...
        abe.set_scatter_correction((0.2,) + setting[1:], dim_x, dim_y, l_x, l_y)   # ... while the setting is replaced
        abe.clear_scatter_correction()
        for x in d:
            assert np.array_equal(bits(read(abe, x)), bits(want))


ORD_GEO = DM.ORD_GEO
ORD_X, ORD_Y = ORD_GEO[:2]
ORD_FRAME = np.random.default_rng(9).uniform(0.0, 2.0, (ORD_Y, ORD_X)).astype(np.float32)
ORD_SETTING = S.setting_for(1.0, 4, 4)


def test_a_held_back_weighting_is_flushed_first():
    det = B.DetectorGeometry(*ORD_GEO)

    def run(fusion):
        with B.Backend(0, synchronous=False) as abe:
            abe.set_stage_fusion(fusion)
            abe.set_scatter_correction(ORD_SETTING, ORD_X, ORD_Y, det.l_px_row, det.l_px_col)
            d = B.load(abe, B.Projection(ORD_FRAME.copy(), ORD_X, ORD_Y, idx=2))
            B.weight(abe, d, det)               # with fusion: held back until something touches the frame
            abe.scatter_correction(d)
            return read(abe, d)

    plain, fused = run(False), run(True)
    assert np.array_equal(bits(fused), bits(plain))
    with B.Backend(0) as sbe:
        sbe.set_scatter_correction(ORD_SETTING, ORD_X, ORD_Y, det.l_px_row, det.l_px_col)
        unweighted, = correct(sbe, [ORD_FRAME])
    assert not np.array_equal(bits(plain), bits(unweighted))


@pytest.mark.parametrize("by_reference", [False, True])
def test_a_frame_of_the_pending_group_is_backprojected_as_it_was(by_reference):
    """Correcting in a buffer the pending by-reference group refers to launches that group first: the volume is the one the snapshot
    path gives. With snapshots the group stays pending."""
    det = B.DetectorGeometry(*ORD_GEO)
    vg = B.calculate_volume_geometry(det)

    def run(deferred):
        with B.Backend(0, synchronous=False) as abe:
            if deferred:
                abe.set_backproject_deferral(8)
                abe.set_backproject_references(by_reference)
            abe.set_scatter_correction(ORD_SETTING, ORD_X, ORD_Y, det.l_px_row, det.l_px_col)
            d = B.load(abe, B.Projection(ORD_FRAME.copy(), ORD_X, ORD_Y, idx=1))
            v = abe.make_volume_device(vg.dim_x, vg.dim_y, vg.dim_z)
            B.backproject(abe, d, v, 0, det, vg, False, False, None)
            if deferred:
                assert pending(abe) == 1
            abe.scatter_correction(d)
            if deferred:
                assert pending(abe) == (0 if by_reference else 1)
            return read(abe, d), DM.volume_to_host(abe, v, vg)

    want_p, want_v = run(False)
    got_p, got_v = run(True)
    assert np.abs(want_v).max() > 0 and not np.array_equal(bits(want_p), bits(ORD_FRAME))
    assert np.array_equal(bits(got_v), bits(want_v)) and np.array_equal(bits(got_p), bits(want_p))


# ---- 7. the physical check --------------------------------------------------------------------------------------------------------------

def test_scatter_leaves_the_reconstruction(be, scene):
    """The scene of tests/scatter_rule.py: 120 views of a soft phantom on 64 x 32 pixels of 1 mm, scatter of the forward model at
    A = 0.12, alpha = -0.15, beta = 1, sigma = 4 and 16 mm, w2 = 0.5 (the largest scatter-to-primary ratio is 0.125), corrected on the
    device in one call with limit 0.6, margin 24 and 4 iterations, reconstructed by the float64 model and compared with the volume of
    the exact line integrals. The ratio corrected / scattered is at most 4 times the fp32 restatement's (tests/test_scatter_host.py
    pins it; the float64 model gives 5.283e-4: scattered 1.510e-3, corrected 7.977e-7)."""
    det, vg, frames, exact = scene
    setting = S.scene_setting(4)
    f, _ = S.scattered(frames, setting)
    before = S.scene_rms(metal_rule.reconstruct64(f, det, vg), exact)
    be.set_scatter_correction(setting, det.n_row, det.n_col, det.l_px_row, det.l_px_col)
    got = np.stack(correct(be, list(f)))
    after = S.scene_rms(metal_rule.reconstruct64(got, det, vg), exact)
    print("scatter correction, scene on the device: scattered %.4g, corrected %.4g, ratio %.4g" % (before, after, after / before))
    assert after / before <= FACTOR * S.SCENE_RATIO_32
