"""Phase retrieval on the device: paris_hip_phase_retrieval_frames against the float64 restatement of
tests/phase_rule.py, with the error of the fp32 restatement as the yardstick -- every size class of the launcher --, a frame's bits
whatever shares its call, canvases, special pixels, more frames than a round of launches serves, the contracts of a ctx-owned
setting and of a frame pass, and the physical check: fringes of the transport-of-intensity model removed from a reconstruction."""
import numpy as np
import pytest

import metal_rule
import phase_rule as P
import test_gpu_defect_map as DM
import test_gpu_detector_roll as DR
from paris_amd import _lib
from paris_amd import backend as B

pytestmark = pytest.mark.gpu

bits, read, pending = DM.bits, DM.read, DM.pending
INV, UNS = _lib.ERROR_INVALID_ARGUMENT, _lib.ERROR_UNSUPPORTED
ALPHA, T_MIN = 2.5, 1e-6
FACTOR = 4.0     # another radix and butterfly order, table twiddles, the device's expf / logf


@pytest.fixture(scope="module")
def be():
    with B.Backend(0) as b:
        yield b
        b.clear_phase_retrieval()


def retrieve(be, frames, n_frames=None):
    """the frames stacked in one buffer, retrieved by one call (the setting is in place); returns them as a list"""
    dim_y, dim_x = frames[0].shape
    d = be.make_projection_device(dim_x, dim_y * len(frames))
    be.upload_raw(np.ascontiguousarray(np.vstack(frames), np.float32), d)
    be.phase_retrieval(be.wrap_projection(d.ptr, d.pitch, dim_x, dim_y), d.pitch * dim_y, len(frames) if n_frames is None else n_frames)
    out = read(be, d)
    be.free(d)
    return [out[k * dim_y:(k + 1) * dim_y] for k in range(len(frames))]


def refused(code, f, *args, **kw):
    with pytest.raises(B.ParisHipError) as e:
        f(*args, **kw)
    return e.value.status == code


# ---- 1. the rule, within FFT rounding -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", P.SHAPES, ids=lambda s: "%dx%d" % s[:2])
def test_the_device_keeps_four_times_the_error_of_the_fp32_restatement(be, shape):
    """E(x) = max |exp(-x) - max(T'_64, t_min)| over the pixels that entered the filter; E(device) <= 4 E(retrieve32), both evaluated
    here on the same input. Measured on an MI355X: E(device) 1.2e-7 .. 4.5e-7 against E(retrieve32) 0.8e-7 .. 4.2e-7 (DESIGN.md
    section 4.22 has the table); the 1 x 1 frame gives 0 and 1.35e-8 on both sides."""
    dim_x, dim_y, margin, n_x, n_y, l_x, l_y = shape
    be.set_phase_retrieval(ALPHA, T_MIN, margin, dim_x, dim_y, l_x, l_y)
    for name, p in (("blob", P.blob(dim_x, dim_y)), ("ramp", P.ramp(dim_x, dim_y))):
        assert np.exp(-float(P.retrieve64(p, ALPHA, T_MIN, margin, l_x, l_y).max())) >= 0.05, "no pixel at the floor"
        got, = retrieve(be, [p])
        e_dev = P.error(got, p, ALPHA, T_MIN, margin, l_x, l_y)
        e_32 = P.error(P.retrieve32(p, ALPHA, T_MIN, margin, l_x, l_y), p, ALPHA, T_MIN, margin, l_x, l_y)
        print("phase retrieval %d x %d -> %d x %d, %s: E(device) %.3g, E(retrieve32) %.3g" % (dim_x, dim_y, n_x, n_y, name, e_dev, e_32))
        assert e_dev <= FACTOR * e_32
        if dim_x * dim_y > 1:
            assert np.abs(got - p).max() > 1e-3, "the filter changes the frame"


def test_a_constant_frame_returns_itself_within_rounding(be):
    be.set_phase_retrieval(ALPHA, T_MIN, 3, 7, 5, 0.4, 0.9)
    for value in (0.0, 0.5, 1.25):
        got, = retrieve(be, [np.full((5, 7), value, np.float32)])
        # the spectrum of a constant is its DC bin, exactly, and H(0, 0) = 1: what is left is expf, logf and the store, an ulp or two of
        # T <= 1 each -- eight units of 2^-24 bound it
        assert np.abs(np.exp(-got.astype(np.float64)) - np.exp(-value)).max() <= 8 * 2.0 ** -24, value


# ---- 2. a frame's bits do not depend on its company -----------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [P.SHAPES[0], P.SHAPES[2], P.SHAPES[4]], ids=lambda s: "%dx%d" % s[:2])
def test_a_frame_alone_equals_the_frame_anywhere_among_three(be, shape):
    dim_x, dim_y, margin, _, _, l_x, l_y = shape
    be.set_phase_retrieval(ALPHA, T_MIN, margin, dim_x, dim_y, l_x, l_y)
    a, b, c = P.blob(dim_x, dim_y), P.ramp(dim_x, dim_y), P.blob(dim_x, dim_y, seed=3) * np.float32(0.5)
    alone, = retrieve(be, [a])
    assert np.abs(alone - a).max() > 1e-3
    for frames, at in (([a, b, c], 0), ([b, a, c], 1), ([b, c, a], 2), ([a, b], 0), ([c, a], 1)):
        got = retrieve(be, frames)
        assert np.array_equal(bits(got[at]), bits(alone)), at
    # n_frames 1 and 2 of three: the frames beyond stay as they were
    for n in (1, 2):
        got = retrieve(be, [a, b, c], n_frames=n)
        assert np.array_equal(bits(got[0]), bits(alone))
        assert all(np.array_equal(bits(g), bits(f)) for g, f in list(zip(got, [a, b, c]))[n:])


def test_more_frames_than_a_round_of_launches_serves(be):
    """70 frames of 5 x 3 in one call: the scratch holds 16, the call loops five times, and every frame has the bits it has alone"""
    dim_x, dim_y, margin, _, _, l_x, l_y = P.SHAPES[0]
    be.set_phase_retrieval(ALPHA, T_MIN, margin, dim_x, dim_y, l_x, l_y)
    assert B.phase_retrieval_check(ALPHA, T_MIN, margin, dim_x, dim_y, l_x, l_y)[2] == 16 * dim_y * 5 * 8
    frames = [P.blob(dim_x, dim_y, seed=k) for k in range(70)]
    got = retrieve(be, frames)
    for k in (0, 15, 16, 31, 32, 63, 64, 69):
        alone, = retrieve(be, [frames[k]])
        assert np.array_equal(bits(got[k]), bits(alone)) and np.abs(alone - frames[k]).max() > 1e-3, k


# ---- 3. canvases ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", [DR.ALIGNED, DR.ALIGNED_WIDE, DR.SCALAR, DR.SCALAR_WIDE], ids=["aligned", "aligned_wide", "scalar", "scalar_wide"])
def test_every_byte_outside_the_frames_comes_back_as_it_went(be, layout):
    dim_x, dim_y, margin, _, _, l_x, l_y = P.SHAPES[5]
    be.set_phase_retrieval(ALPHA, T_MIN, margin, dim_x, dim_y, l_x, l_y)
    frames = [P.blob(dim_x, dim_y), P.ramp(dim_x, dim_y), P.blob(dim_x, dim_y, seed=8)]
    want_frames = [retrieve(be, [f])[0] for f in frames]
    off, pitch, stride, n_bytes = layout(3, dim_x, dim_y)
    host = np.full(((n_bytes + 255) // 256) * 64, DR.SENTINEL, np.uint32).view(np.float32)
    want = host.copy()
    for k in range(3):
        DR.place(host, off + k * stride, pitch, frames[k])
        DR.place(want, off + k * stride, pitch, want_frames[k])
    canvas = DR.Canvas(be, n_bytes, host.copy())
    be.phase_retrieval(canvas.view(off, pitch, dim_x, dim_y), stride, 3)
    got = canvas.read()
    canvas.free()
    assert np.array_equal(bits(got), bits(want))


# ---- 4. special pixels ------------------------------------------------------------------------------------------------------------------

def test_special_pixels_are_left_as_stored_and_their_neighbours_see_air(be):
    be.set_phase_retrieval(ALPHA, T_MIN, 4, 21, 13, 1.0, 1.0)
    p = P.blob(21, 13)
    special = {(2, 3): np.nan, (5, 7): np.inf, (6, 1): -np.inf, (9, 20): -200.0, (12, 0): np.nan}
    for at, v in special.items():
        p[at] = v
    air = p.copy()
    for at in special:
        air[at] = 0.0
    got, = retrieve(be, [p])
    for at in special:
        assert bits(got)[at] == bits(p)[at], at
    keep = P.entered(p)
    assert np.count_nonzero(~keep) == len(special)
    want64 = P.retrieve64(air, ALPHA, T_MIN, 4, 1.0, 1.0)
    e_dev = float(np.abs(np.exp(-got.astype(np.float64)) - np.exp(-want64.astype(np.float64)))[keep].max())
    e_32 = P.error(P.retrieve32(air, ALPHA, T_MIN, 4, 1.0, 1.0), air, ALPHA, T_MIN, 4, 1.0, 1.0)
    assert e_dev <= FACTOR * e_32 + 2.0 ** -24      # (want64 is rounded to float before the comparison)


def test_a_frame_below_the_floor_comes_out_at_the_floor(be):
    be.set_phase_retrieval(ALPHA, T_MIN, 4, 9, 5, 1.0, 1.0)
    got, = retrieve(be, [np.full((5, 9), 20.0, np.float32)])
    want = np.float32(-np.log(float(np.float32(T_MIN))))
    assert np.all(np.abs(got - want) <= np.spacing(want))


# ---- 5. contracts -----------------------------------------------------------------------------------------------------------------------

def test_the_refusals(be):
    be.set_phase_retrieval(ALPHA, T_MIN, 8, 61, 45, 0.7, 1.1)
    d, other = be.make_projection_device(61, 45), be.make_projection_device(60, 45)
    be.phase_retrieval(d)
    assert refused(INV, be.phase_retrieval, other)
    assert refused(INV, be.phase_retrieval, be.wrap_projection(d.ptr, d.pitch, 61, 44))
    assert refused(INV, be.phase_retrieval, be.wrap_projection(d.ptr, 61 * 4 - 4, 61, 45))
    assert refused(INV, be.phase_retrieval, d, 45 * d.pitch - 4, 2)
    for bad in ((0.0, T_MIN, 8), (np.nan, T_MIN, 8), (ALPHA, 0.0, 8), (ALPHA, 2.0, 8), (ALPHA, T_MIN, 0), (ALPHA, T_MIN, P.MARGIN_MAX + 1)):
        assert refused(INV, be.set_phase_retrieval, *bad, 61, 45, 0.7, 1.1)
    assert refused(INV, be.set_phase_retrieval, ALPHA, T_MIN, 8, 61, 45, 0.0, 1.1)
    assert refused(UNS, be.set_phase_retrieval, ALPHA, T_MIN, 8, 8180, 45, 0.7, 1.1)
    be.phase_retrieval(d)                       # a refused setting leaves the one in place
    be.clear_phase_retrieval()
    assert refused(INV, be.phase_retrieval, d)
    be.free(d)
    be.free(other)


def test_the_reserve_counts_the_setting():
    with B.Backend(0) as b:
        without = b.projection_reserve_bytes(61, 45)
        b.set_phase_retrieval(ALPHA, T_MIN, 8, 61, 45, 0.7, 1.1)
        n_x, n_y, scratch = B.phase_retrieval_check(ALPHA, T_MIN, 8, 61, 45, 0.7, 1.1)
        assert b.projection_reserve_bytes(61, 45) == without + scratch + 8 * (n_x + n_y)      # twiddles and tables: 4 N + 4 N bytes an axis
        b.set_phase_retrieval(ALPHA, T_MIN, 1, 5, 3, 1.0, 1.0)
        assert b.projection_reserve_bytes(61, 45) == without + 16 * 3 * 5 * 8 + 8 * 16
        b.clear_phase_retrieval()
        assert b.projection_reserve_bytes(61, 45) == without


def test_a_replaced_setting_leaves_queued_work_on_the_old_one(be):
    dim_x, dim_y, margin, _, _, l_x, l_y = P.SHAPES[6]
    p = P.blob(dim_x, dim_y)
    be.set_phase_retrieval(ALPHA, T_MIN, margin, dim_x, dim_y, l_x, l_y)
    want, = retrieve(be, [p])
    with B.Backend(0, synchronous=False) as abe:
        abe.set_phase_retrieval(ALPHA, T_MIN, margin, dim_x, dim_y, l_x, l_y)
        d = [abe.make_projection_device(dim_x, dim_y) for _ in range(4)]
        for x in d:
            abe.upload_raw(p, x)
        for x in d:
            abe.phase_retrieval(x)                                  # queued ...
        abe.set_phase_retrieval(9.0 * ALPHA, T_MIN, margin, dim_x, dim_y, l_x, l_y)   # ... while the setting is replaced
        abe.clear_phase_retrieval()
        for x in d:
            assert np.array_equal(bits(read(abe, x)), bits(want))


ORD_GEO = DM.ORD_GEO
ORD_X, ORD_Y = ORD_GEO[:2]
ORD_FRAME = np.random.default_rng(9).uniform(0.0, 2.0, (ORD_Y, ORD_X)).astype(np.float32)


def test_a_held_back_weighting_is_flushed_first():
    det = B.DetectorGeometry(*ORD_GEO)

    def run(fusion):
        with B.Backend(0, synchronous=False) as abe:
            abe.set_stage_fusion(fusion)
            abe.set_phase_retrieval(ALPHA, T_MIN, 4, ORD_X, ORD_Y, det.l_px_row, det.l_px_col)
            d = B.load(abe, B.Projection(ORD_FRAME.copy(), ORD_X, ORD_Y, idx=2))
            B.weight(abe, d, det)               # with fusion: held back until something touches the frame
            abe.phase_retrieval(d)
            return read(abe, d)

    plain, fused = run(False), run(True)
    assert np.array_equal(bits(fused), bits(plain))
    with B.Backend(0) as sbe:
        sbe.set_phase_retrieval(ALPHA, T_MIN, 4, ORD_X, ORD_Y, det.l_px_row, det.l_px_col)
        unweighted, = retrieve(sbe, [ORD_FRAME])
    assert not np.array_equal(bits(plain), bits(unweighted))


@pytest.mark.parametrize("by_reference", [False, True])
def test_a_frame_of_the_pending_group_is_backprojected_as_it_was(by_reference):
    """Retrieving in a buffer the pending by-reference group refers to launches that group first: the volume is the one the snapshot
    path gives. With snapshots the group stays pending."""
    det = B.DetectorGeometry(*ORD_GEO)
    vg = B.calculate_volume_geometry(det)

    def run(deferred):
        with B.Backend(0, synchronous=False) as abe:
            if deferred:
                abe.set_backproject_deferral(8)
                abe.set_backproject_references(by_reference)
            abe.set_phase_retrieval(ALPHA, T_MIN, 4, ORD_X, ORD_Y, det.l_px_row, det.l_px_col)
            d = B.load(abe, B.Projection(ORD_FRAME.copy(), ORD_X, ORD_Y, idx=1))
            v = abe.make_volume_device(vg.dim_x, vg.dim_y, vg.dim_z)
            B.backproject(abe, d, v, 0, det, vg, False, False, None)
            if deferred:
                assert pending(abe) == 1
            abe.phase_retrieval(d)
            if deferred:
                assert pending(abe) == (0 if by_reference else 1)
            return read(abe, d), DM.volume_to_host(abe, v, vg)

    want_p, want_v = run(False)
    got_p, got_v = run(True)
    assert np.abs(want_v).max() > 0 and not np.array_equal(bits(want_p), bits(ORD_FRAME))
    assert np.array_equal(bits(got_v), bits(want_v)) and np.array_equal(bits(got_p), bits(want_p))


# ---- 6. the physical check --------------------------------------------------------------------------------------------------------------

def test_fringes_leave_the_reconstruction(be):
    """The scene of tests/phase_rule.py: 120 views of a soft phantom on 64 x 32 pixels of 1 mm, fringes of the transport-of-intensity
    model at alpha = 16 mm^2, retrieved on the device in one call, reconstructed by fdk_model and compared with the volume of the
    exact line integrals. The ratio retrieved / fringed is at most 4 times the fp32 restatement's 1.665e-4 (tests/test_phase_host.py
    pins it; the float64 model gives 1.664e-4). Measured on an MI355X: fringed 4.804e-3, retrieved 7.997e-7, ratio 1.665e-4 (DESIGN.md
    section 4.22)."""
    det, vg = B.DetectorGeometry(*P.SCENE_DET), B.VolumeGeometry(*P.SCENE_GRID)
    frames = P.scene_frames()
    exact = metal_rule.reconstruct64(frames, det, vg)
    alpha = 16.0
    margin = B.phase_default_margin(alpha, det.l_px_row, det.l_px_col)
    f = P.fringed(frames, alpha)
    before = P.scene_rms(metal_rule.reconstruct64(f, det, vg), exact)
    be.set_phase_retrieval(alpha, P.SCENE_T_MIN, margin, det.n_row, det.n_col, det.l_px_row, det.l_px_col)
    got = np.stack(retrieve(be, list(f)))
    after = P.scene_rms(metal_rule.reconstruct64(got, det, vg), exact)
    print("phase retrieval, scene on the device: fringed %.4g, retrieved %.4g, ratio %.4g" % (before, after, after / before))
    assert after / before <= FACTOR * 1.665e-4
