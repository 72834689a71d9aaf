"""The beam-hardening pass on the device (paris_hip_set_beam_hardening / paris_hip_beam_hardening_rows / _rows_with, DESIGN.md section
4.17) against the library's host function bit for bit (which tests/test_beam_hardening_host.py holds to the numpy restatement): the
single-pixel and the 16-byte paths, bands, frames per call, what must stay untouched, and the refusals."""
import ctypes as C

import numpy as np
import pytest

import beam_hardening_rule as R
import grid_cap_rule as G
from paris_amd import _lib
from paris_amd import backend as B
from test_gpu_ring_correction import read

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-77.25)
GUARD = 4           # columns of the allocation to the right of (and, shifted, to the left of) the frames


@pytest.fixture(scope="module")
def be():
    with B.Backend(0) as b:
        yield b


class Shifted:
    """n frames one under the other inside a wider allocation whose rows are padded to 256 bytes, starting `shift` floats into each
    row: shift = 1 gives frames whose base is not 16-byte aligned; the columns around them stand for the pitch padding"""

    def __init__(self, be, frames, shift):
        self.be, self.n, self.shift = be, len(frames), shift
        self.dim_y, self.dim_x = frames[0].shape
        self.owner = be.make_projection_device(self.dim_x + GUARD, self.dim_y * self.n)
        self.before = np.full((self.dim_y * self.n, self.dim_x + GUARD), SENTINEL, np.float32)
        self.before[:, shift:shift + self.dim_x] = np.concatenate(frames)
        be.upload_raw(self.before, self.owner)
        self.pitch = self.owner.pitch
        self.stride = self.pitch * self.dim_y
        self.first = be.wrap_projection(self.owner.ptr + 4 * shift, self.pitch, self.dim_x, self.dim_y)

    def read(self):
        return read(self.be, self.owner)

    def free(self):
        self.be.free(self.owner)


def expected(s, c, rows):
    want = s.before.copy()
    first, count = rows
    for k in range(s.n):
        band = slice(k * s.dim_y + first, k * s.dim_y + first + count)
        want[band, s.shift:s.shift + s.dim_x] = B.beam_hardening_host(c, s.before[band, s.shift:s.shift + s.dim_x])
    return want


def assert_pass(be, frames, shift, c, rows, through_setting, what):
    s = Shifted(be, frames, shift)
    try:
        assert (s.first.ptr % 16 == 0) == (shift % 4 == 0) and s.pitch % 256 == 0 and s.pitch > 4 * (s.dim_x + GUARD) - 1
        if through_setting:
            be.set_beam_hardening(c, s.dim_x, s.dim_y)
            be.beam_hardening(s.first, frame_stride=s.stride, n_frames=s.n, rows=rows)
        else:
            be.beam_hardening(s.first, frame_stride=s.stride, n_frames=s.n, rows=rows, c=c)
        got, want = s.read(), expected(s, c, rows)
        assert R.same_pixels(got, want), what
        # outside the band and around the frames not a bit has changed -- NaN payloads included
        keep = np.ones(got.shape, bool)
        for k in range(s.n):
            keep[k * s.dim_y + rows[0]:k * s.dim_y + rows[0] + rows[1], shift:shift + s.dim_x] = False
        assert keep.any() and np.array_equal(R.bits(got)[keep], R.bits(s.before)[keep]), what
    finally:
        if through_setting:
            be.clear_beam_hardening()
        s.free()


@pytest.mark.parametrize("degree", [1, 2, 3, 4])
@pytest.mark.parametrize("dim_x,dim_y,shift", [(37, 5, 1), (64, 4, 0)])
def test_the_pass_equals_the_host_function_on_a_band(be, dim_x, dim_y, shift, degree):
    """37 x 5 from a base that is not 16-byte aligned: single pixels; 64 x 4 aligned: 16-byte vectors. Three frames, padded pitch, rows
    1 .. 3, pixels of both signs, +-0, a NaN with a payload, infinities and denormals"""
    frames = [R.special_pixels((dim_y, dim_x), seed=10 * degree + k) for k in range(3)]
    frames[1][2, 3:11] = [np.nan, np.inf, -np.inf, 1e-40, -2e-45, -0.0, 0.0, -0.5]     # inside the band whatever the seed
    frames[1].view(np.uint32)[2, 3] = R.NAN_PAYLOAD
    band = np.concatenate([f[1:4] for f in frames])
    assert np.isnan(band).any() and np.isinf(band).any() and (band < 0).any() and np.count_nonzero((band != 0) & (np.abs(band) < 1e-38)) >= 1
    for through_setting in (True, False):
        assert_pass(be, frames, shift, R.COEFFICIENTS[degree], (1, 3), through_setting, (dim_x, degree, through_setting))


def test_degree_one_with_c1_one_changes_nothing_but_a_nan_payload(be):
    frames = [R.special_pixels((5, 37), seed=3)]
    s = Shifted(be, frames, 1)
    be.beam_hardening(s.first, c=[1.0])
    assert R.same_pixels(s.read(), s.before)
    s.free()


@pytest.mark.parametrize("dim_x", [260, 261])
def test_whole_frames_over_more_than_one_block(be, dim_x):
    """260 x 70 is 4550 lanes of four pixels, 261 x 70 is 18270 lanes of one: 18 and 72 blocks of 256; five frames on grid y"""
    frames = [R.special_pixels((70, dim_x), seed=dim_x + k) for k in range(5)]
    assert_pass(be, frames, 0, R.COEFFICIENTS[3], (0, 70), True, dim_x)
    assert_pass(be, frames[:2], 0, R.COEFFICIENTS[4], (69, 1), False, dim_x)


@pytest.mark.parametrize("dim_x", G.DIM_XS)
def test_a_band_past_the_grid_cap(be, dim_x):
    """1024 rows of 1025 pixels, or of 4100 in groups of four: 1 049 600 lanes against the cap of 4096 blocks of 256, so four blocks
    come round again and split their lane index a second time, into the band's final row. Two frames a stride larger than the frame
    apart; rows 0 .. 2 and 1027 .. 1029, the pitch padding and the gap keep their bits. The setting form, then the argument form on
    what it left."""
    assert G.lanes(dim_x, dim_x % 4 == 0) > G.CAP_LANES
    frames = [R.special_pixels((G.DIM_Y, dim_x), seed=dim_x + k) for k in range(2)]
    first, count = G.BAND
    s = G.Canvas(be, frames)
    try:
        assert s.first.ptr % 16 == 0 and s.stride % 16 == 0 and s.stride > s.pitch * G.DIM_Y   # dim_x alone decides the path
        c = R.COEFFICIENTS[3]
        be.set_beam_hardening(c, dim_x, G.DIM_Y)
        be.beam_hardening(s.first, frame_stride=s.stride, n_frames=2, rows=G.BAND)
        once = [B.beam_hardening_host(c, f[first:first + count]) for f in frames]
        got = s.read()
        G.assert_canvas(s, got, s.expected(once), (dim_x, "setting"))
        for k in range(2):   # the second visit wrote: nearly every pixel there differs from what it was
            tail_got, tail_was = G.second_visit(s, got, k), G.second_visit(s, s.before, k)
            assert np.count_nonzero(R.bits(tail_got) != R.bits(tail_was)) > 0.9 * tail_was.size
        be.beam_hardening(s.first, frame_stride=s.stride, n_frames=2, rows=G.BAND, c=R.COEFFICIENTS[2])
        twice = [B.beam_hardening_host(R.COEFFICIENTS[2], q) for q in once]
        G.assert_canvas(s, s.read(), s.expected(twice), (dim_x, "argument"))
    finally:
        be.clear_beam_hardening()
        s.free()


def test_an_empty_band_and_no_frame_do_nothing(be):
    frames = [R.special_pixels((5, 37), seed=4)]
    s = Shifted(be, frames, 0)
    be.beam_hardening(s.first, rows=(2, 0), c=[2.0])
    be.beam_hardening(s.first, rows=(5, 0), c=[2.0])
    be.beam_hardening(s.first, n_frames=0, c=[2.0])
    assert np.array_equal(R.bits(s.read()), R.bits(s.before))
    s.free()


def test_a_replaced_setting_and_the_argument_form_leave_each_other_alone(be):
    frames = [np.full((4, 64), 2.0, np.float32)]
    s = Shifted(be, frames, 0)
    be.set_beam_hardening([1.0, 1.0], 64, 4)
    be.set_beam_hardening([0.5], 64, 4)                       # replaces
    be.beam_hardening(s.first, c=[0.0, 0.0, 1.0])             # p^3 = 8: the unit setting of the fit; the backend's stays 0.5
    be.beam_hardening(s.first)                                # 4
    got = s.read()[:, :64]
    assert np.array_equal(got, np.full((4, 64), 4.0, np.float32))
    be.clear_beam_hardening()
    be.clear_beam_hardening()                                 # clearing nothing is fine
    with pytest.raises(B.ParisHipError):
        be.beam_hardening(s.first)
    s.free()


def test_refusals(be):
    L = _lib.load()
    INV = _lib.ERROR_INVALID_ARGUMENT
    d = be.make_projection_device(96, 80)
    other = be.make_projection_device(97, 80)
    good = _lib.BeamHardening(2, (C.c_float * 4)(1.0, 0.1, 0.0, 0.0))
    with pytest.raises(B.ParisHipError) as e:                 # without a setting
        be.beam_hardening(d)
    assert e.value.status == INV
    for bad in ([], [1.0] * 5, [float("nan")], [1.0, float("inf")]):     # a refused setting sets nothing
        with pytest.raises(B.ParisHipError) as e:
            be.set_beam_hardening(bad, 96, 80)
        assert e.value.status == INV
        with pytest.raises(B.ParisHipError):
            be.beam_hardening(d, c=bad)
    with pytest.raises(B.ParisHipError):
        be.set_beam_hardening([1.0], 0, 80)
    with pytest.raises(B.ParisHipError):
        be.set_beam_hardening([1.0], 96, 0)
    assert L.paris_hip_set_beam_hardening(be._ctx, None, 96, 80) == INV
    assert L.paris_hip_set_beam_hardening(None, C.byref(good), 96, 80) == INV
    assert L.paris_hip_clear_beam_hardening(None) == INV
    with pytest.raises(B.ParisHipError):
        be.beam_hardening(d)
    be.set_beam_hardening([1.0, 0.1], 96, 80)
    try:
        with pytest.raises(B.ParisHipError):
            be.beam_hardening(other)                                                          # other dimensions
        with pytest.raises(B.ParisHipError):
            be.beam_hardening(B.Projection(d.ptr, 96, 79, pitch=d.pitch, on_device=True))
        for kw in ({}, {"c": [1.0, 0.1]}):
            with pytest.raises(B.ParisHipError):
                be.beam_hardening(B.Projection(d.ptr, 96, 80, pitch=4 * 96 - 4, on_device=True), **kw)   # a bad pitch
            with pytest.raises(B.ParisHipError):
                be.beam_hardening(B.Projection(d.ptr, 96, 80, pitch=d.pitch + 2, on_device=True), **kw)
            with pytest.raises(B.ParisHipError):
                be.beam_hardening(d, rows=(70, 11), **kw)                                     # a bad band
            with pytest.raises(B.ParisHipError):
                be.beam_hardening(d, rows=(81, 0), **kw)
        be.beam_hardening(other, c=[1.0])                      # the argument form is not bound to the setting's frame size
        fn = L.paris_hip_beam_hardening_rows
        assert fn(be._ctx, d.ptr, d.pitch, d.pitch * 80 - 4, 2, 96, 80, 0, 80) == INV        # overlapping frames
        assert fn(be._ctx, d.ptr, d.pitch, d.pitch * 80 + 2, 2, 96, 80, 0, 80) == INV
        assert fn(be._ctx, None, d.pitch, 0, 1, 96, 80, 0, 80) == INV
        assert fn(None, d.ptr, d.pitch, 0, 1, 96, 80, 0, 80) == INV
        fn = L.paris_hip_beam_hardening_rows_with
        assert fn(be._ctx, None, d.ptr, d.pitch, 0, 1, 96, 80, 0, 80) == INV
        assert fn(be._ctx, C.byref(good), None, d.pitch, 0, 1, 96, 80, 0, 80) == INV
        assert fn(None, C.byref(good), d.ptr, d.pitch, 0, 1, 96, 80, 0, 80) == INV
        assert fn(be._ctx, C.byref(good), d.ptr, d.pitch, d.pitch * 80 - 4, 2, 96, 80, 0, 80) == INV
    finally:
        be.clear_beam_hardening()
    be.free(d)
    be.free(other)
