"""The ordering contract every in-place frame pass obeys, pinned once per pass: the
Parker weight, the offset-detector weight, the flat-field rows pass, the defect repair and both forms of the beam-hardening pass (its
setting, and the rule as an argument). A held-back weighting runs first, a frame of the pending by-reference group is backprojected
as it was, a call with nothing to launch launches nothing, and the common argument rule refuses the same frame and band descriptions
everywhere. Shapes and geometry are those of tests/test_gpu_defect_map.py."""
import ctypes as C

import numpy as np
import pytest

import test_gpu_defect_map as DM
from paris_amd import _lib
from paris_amd import backend as B

pytestmark = pytest.mark.gpu

DIM_X, DIM_Y = DM.ORD_GEO[:2]
SCAN = B.ShortScan(0.0, 200.0)   # delta = 10 degrees, gamma_m = 1.9 degrees
PHI = np.float32(5.0)            # beta = 5 degrees: every column on the rising ramp
bits, read, pending = DM.bits, DM.read, DM.pending


def references():
    rng = np.random.default_rng(7)
    dark = (0.05 + 0.05 * rng.random((DIM_Y, DIM_X))).astype(np.float32)
    flat = (dark + 3.0 + rng.random((DIM_Y, DIM_X))).astype(np.float32)
    return dark, flat


MASK, FRAME = DM.ordering_frame()
DARK, FLAT = references()


class Pass:
    """one in-place pass: the setting it needs, the call on a whole frame, and its raw C entry point on a band"""

    def __init__(self, name, setup, run, raw):
        self.name, self.setup, self.run, self.raw = name, setup, run, raw

    def __repr__(self):
        return self.name


def _det():
    return B.DetectorGeometry(*DM.ORD_GEO)


def _parker_raw(be, ptr, pitch, stride, n, dim_x, dim_y, row_first, row_count):
    phis = (C.c_float * max(n, 1))(*([PHI] * max(n, 1)))
    return be._L.paris_hip_short_scan_weight_rows(be._ctx, ptr, pitch, stride, n, dim_x, dim_y, row_first, row_count, C.byref(_det()),
                                                  C.byref(SCAN), phis)


def _offset_raw(be, ptr, pitch, stride, n, dim_x, dim_y, row_first, row_count):
    return be._L.paris_hip_offset_detector_weight_rows(be._ctx, ptr, pitch, stride, n, dim_x, dim_y, row_first, row_count, C.byref(_det()))


def _flat_raw(be, ptr, pitch, stride, n, dim_x, dim_y, row_first, row_count):
    return be._L.paris_hip_flat_field_rows(be._ctx, ptr, pitch, stride, n, dim_x, dim_y, row_first, row_count)


def _defect_raw(be, ptr, pitch, stride, n, dim_x, dim_y, row_first, row_count):
    return be._L.paris_hip_defect_repair_rows(be._ctx, ptr, pitch, stride, n, dim_x, dim_y, row_first, row_count)


BH_C = [0.93, 0.11]              # q = 0.93 p + 0.11 p^2: changes every pixel that is not zero


def _bh_raw(be, ptr, pitch, stride, n, dim_x, dim_y, row_first, row_count):
    return be._L.paris_hip_beam_hardening_rows(be._ctx, ptr, pitch, stride, n, dim_x, dim_y, row_first, row_count)


def _bh_with_raw(be, ptr, pitch, stride, n, dim_x, dim_y, row_first, row_count):
    rule = B._bh_setting(BH_C)
    return be._L.paris_hip_beam_hardening_rows_with(be._ctx, C.byref(rule), ptr, pitch, stride, n, dim_x, dim_y, row_first, row_count)


PASSES = [
    Pass("parker", lambda be: None, lambda be, d: be.short_scan_weight(d, _det(), SCAN, PHI), _parker_raw),
    Pass("offset_detector", lambda be: None, lambda be, d: be.offset_detector_weight(d, _det()), _offset_raw),
    Pass("flat_field", lambda be: be.set_flat_field(DARK, FLAT), lambda be, d: be.flat_field_rows(d), _flat_raw),
    Pass("defect_repair", lambda be: be.set_defect_map(MASK), lambda be, d: be.defect_repair_rows(d), _defect_raw),
    Pass("beam_hardening", lambda be: be.set_beam_hardening(BH_C, DIM_X, DIM_Y), lambda be, d: be.beam_hardening(d), _bh_raw),
    Pass("beam_hardening_with", lambda be: None, lambda be, d: be.beam_hardening(d, c=BH_C), _bh_with_raw),
]
each_pass = pytest.mark.parametrize("p", PASSES, ids=repr)


@each_pass
def test_a_held_back_weighting_is_flushed_first(p):
    det = _det()

    def run(fusion):
        with B.Backend(0, synchronous=False) as abe:
            abe.set_stage_fusion(fusion)
            p.setup(abe)
            d_p = B.load(abe, B.Projection(FRAME.copy(), DIM_X, DIM_Y, idx=2))
            B.weight(abe, d_p, det)            # with fusion: held back until something touches the frame
            p.run(abe, d_p)
            return read(abe, d_p)

    plain, fused = run(False), run(True)
    assert not np.array_equal(bits(plain), bits(FRAME)) and np.array_equal(bits(fused), bits(plain))


@each_pass
@pytest.mark.parametrize("by_reference", [False, True])
def test_a_frame_of_the_pending_group_is_backprojected_as_it_was(p, by_reference):
    """by reference: the group that refers to the frame is launched before the pass writes it; snapshots: it stays pending"""
    det = _det()
    vg = B.calculate_volume_geometry(det)

    def run(deferred):
        with B.Backend(0, synchronous=False) as abe:
            if deferred:
                abe.set_backproject_deferral(8)
                abe.set_backproject_references(by_reference)
            p.setup(abe)
            v = abe.make_volume_device(vg.dim_x, vg.dim_y, vg.dim_z)
            d_p = B.load(abe, B.Projection(FRAME.copy(), DIM_X, DIM_Y, idx=1))
            B.backproject(abe, d_p, v, 0, det, vg, False, False, None)
            if deferred:
                assert pending(abe) == 1
            p.run(abe, d_p)
            if deferred:
                assert pending(abe) == (0 if by_reference else 1)
            return read(abe, d_p), DM.volume_to_host(abe, v, vg)

    want_p, want_v = run(False)
    got_p, got_v = run(True)
    assert np.abs(want_v).max() > 0 and not np.array_equal(bits(want_p), bits(FRAME))
    assert np.array_equal(bits(got_v), bits(want_v)) and np.array_equal(bits(got_p), bits(want_p))


def test_the_defect_repair_s_empty_band_launches_nothing():
    """a band without a repairable defect returns before the guards: the pending by-reference group stays pending"""
    det = _det()
    vg = B.calculate_volume_geometry(det)
    mask = np.zeros((DIM_Y, DIM_X), np.uint8)
    mask[10, 20:24] = 1
    with B.Backend(0, synchronous=False) as abe:
        abe.set_backproject_deferral(8)
        abe.set_backproject_references(True)
        abe.set_defect_map(mask)
        v = abe.make_volume_device(vg.dim_x, vg.dim_y, vg.dim_z)
        d_p = B.load(abe, B.Projection(FRAME.copy(), DIM_X, DIM_Y, idx=1))
        B.backproject(abe, d_p, v, 0, det, vg, False, False, None)
        assert pending(abe) == 1
        abe.defect_repair_rows(d_p, row_first=40, row_count=20)
        assert pending(abe) == 1
        abe.defect_repair_rows(d_p, row_first=0, row_count=20)   # the band with the defects: now the group goes first
        assert pending(abe) == 0
        got = read(abe, d_p)
        assert np.array_equal(bits(got)[mask == 0], bits(FRAME)[mask == 0]) and not np.array_equal(bits(got), bits(FRAME))


# what each call changes in the description of the whole first 96 x 80 frame of a buffer that holds two (call() below)
REFUSED = {
    "null d_p": dict(null=True),
    "pitch below the row": dict(pitch=4 * DIM_X - 4),
    "pitch not a multiple of 4": dict(pitch_delta=2),
    "band beyond the frame": dict(row_first=70, row_count=11),
    "empty band beyond the frame": dict(row_first=81, row_count=0),
    "overlapping frames": dict(n_frames=2, stride_delta=-4),
    "frame stride not a multiple of 4": dict(n_frames=2, stride_delta=2),
}
ACCEPTED = {
    "empty band at the end": dict(row_first=80, row_count=0),
    "no frames": dict(n_frames=0),
}


def call(p, be, d, null=False, pitch=None, pitch_delta=0, row_first=0, row_count=DIM_Y, n_frames=1, stride_delta=0):
    pitch = (d.pitch if pitch is None else pitch) + pitch_delta
    stride = pitch * DIM_Y + stride_delta if n_frames > 1 else 0
    return p.raw(be, None if null else d.ptr, pitch, stride, n_frames, DIM_X, DIM_Y, row_first, row_count)


@each_pass
def test_the_common_refusals_and_empty_calls(p):
    two = np.concatenate([FRAME, FRAME[::-1]])
    with B.Backend(0) as be:
        p.setup(be)
        d = be.make_projection_device(DIM_X, 2 * DIM_Y)
        be.upload_raw(two, d)
        for what, args in REFUSED.items():
            assert call(p, be, d, **args) == _lib.ERROR_INVALID_ARGUMENT, what
            assert np.array_equal(bits(read(be, d)), bits(two)), what
        for what, args in ACCEPTED.items():
            assert call(p, be, d, **args) == _lib.SUCCESS, what
            assert np.array_equal(bits(read(be, d)), bits(two)), what
        assert call(p, be, d, n_frames=2) == _lib.SUCCESS   # the same description, valid: both frames change
        got = read(be, d)
        assert not np.array_equal(bits(got[:DIM_Y]), bits(two[:DIM_Y])) and not np.array_equal(bits(got[DIM_Y:]), bits(two[DIM_Y:]))
