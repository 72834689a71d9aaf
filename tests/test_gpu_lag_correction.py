"""The detector lag correction on the device (paris_hip_set_lag_correction / paris_hip_lag_begin / paris_hip_lag_correct_rows /
paris_hip_lag_end) against the library's host rule bit for bit (which tests/test_lag_host.py holds to the numpy
restatement): the single-pixel and the 16-byte paths, the state carried from call to call, what must stay untouched, a band past the
grid cap, the sequence's lifecycle and refusals, and the ordering with deferred backprojections."""
import ctypes as C

import numpy as np
import pytest

import grid_cap_rule as G
import lag_rule as R
from paris_amd import _lib
from paris_amd import backend as B
from test_gpu_ring_correction import pending, read, volume_to_host

pytestmark = pytest.mark.gpu

INV = _lib.ERROR_INVALID_ARGUMENT
DIM_Y, BAND, N = 9, (2, 5), 7          # 7 frames of dim_x x 9, band rows 2 .. 6
GAP_ROWS, GUARD = 2, 4                 # rows of the buffer between two frames; columns of it beside them
ORD_GEO = (96, 80, 0.2, 0.25, 1.5, -0.75, 100, 200, 45.0)


@pytest.fixture(scope="module")
def be():
    with B.Backend(0) as b:
        yield b


class Pool:
    """n frames of dim_x x dim_y in one pool buffer (rows padded to 256 bytes) that is GUARD columns wider than the frames, GAP_ROWS
    rows apart, starting `shift` floats into each row: shift = 1 gives a base 4 bytes off a 16-byte boundary. Everything around the
    frames -- the guard columns, the pitch padding, the gap -- holds grid_cap_rule.SENTINEL, a NaN with a payload."""

    def __init__(self, be, frames, shift=0):
        self.be, self.n, self.shift = be, len(frames), shift
        self.dim_y, self.dim_x = frames[0].shape
        self.rows = self.n * (self.dim_y + GAP_ROWS)
        self.owner = be.make_projection_device(self.dim_x + GUARD, self.rows)
        self.pitch = self.owner.pitch
        self.width = self.pitch // 4
        assert self.pitch % 256 == 0 and self.width >= self.dim_x + GUARD and shift < GUARD
        self.stride = self.pitch * (self.dim_y + GAP_ROWS)
        self.first = be.wrap_projection(self.owner.ptr + 4 * shift, self.pitch, self.dim_x, self.dim_y)
        self.all = B.Projection(self.owner.ptr, self.width, self.rows, pitch=self.pitch, on_device=True)
        self.before = np.full((self.rows, self.width), G.SENTINEL, np.uint32).view(np.float32)
        for k, f in enumerate(frames):
            self.frame_of(self.before, k)[:] = f
        be.copy_h2d(B.Projection(self.before.copy(), self.width, self.rows), self.all)

    def frame_of(self, canvas, k):
        first = k * (self.dim_y + GAP_ROWS)
        return canvas[first:first + self.dim_y, self.shift:self.shift + self.dim_x]

    def frame(self, k):
        return self.be.wrap_projection(self.first.ptr + k * self.stride, self.pitch, self.dim_x, self.dim_y)

    def read(self):
        return read(self.be, self.all)

    def assert_bands(self, got, bands, band=BAND, what=""):
        """rows `band` of frame k equal bands[k] bit for bit (a NaN may carry any payload); every other bit of the buffer is as it was"""
        inside = np.zeros(got.shape, bool)
        want = self.before.copy()
        for k in range(self.n):
            self.frame_of(inside, k)[band[0]:band[0] + band[1]] = True
            self.frame_of(want, k)[band[0]:band[0] + band[1]] = bands[k]
        assert np.array_equal(G.bits(got)[~inside], G.bits(self.before)[~inside]), (what, "outside the bands")
        assert R.same_pixels(got[inside], want[inside]), (what, "the bands")

    def free(self):
        self.be.free(self.owner)


def scan_frames(dim_x, seed):
    f = R.special_frames((N, DIM_Y, dim_x), seed=seed)
    f[3, 4, 3:11] = [np.nan, np.inf, -np.inf, 1e-40, -2e-45, -0.0, 0.0, -250.5]     # inside the band whatever the seed
    f.view(np.uint32)[3, 4, 3] = R.NAN_PAYLOAD
    return f


def band_of(frames, band=BAND):
    return np.ascontiguousarray(frames[:, band[0]:band[0] + band[1]])


def run_sequence(be, pool, cuts, band=BAND):
    be.lag_begin(pool.dim_x, pool.dim_y, *band)
    at = 0
    for n in cuts:
        be.lag_correct(pool.frame(at), frame_stride=pool.stride, n_frames=n, row_first=band[0], row_count=band[1])
        at += n
    seen = be.lag_frames()
    be.lag_end()
    return seen


@pytest.mark.parametrize("start", R.STARTS)
@pytest.mark.parametrize("terms", [1, 2, 3, 4])
@pytest.mark.parametrize("dim_x", [37, 64])
def test_the_pass_equals_the_host_rule_on_a_band(be, dim_x, terms, start):
    """37 wide: single pixels; 64 wide from an aligned base: 16-byte vectors. One call of seven frames a stride larger than the frame
    apart. Then the same with a flat-field setting in force: its dark is subtracted and added back, and the flat-field pass afterwards
    gives what it gives on the host rule's output."""
    frames = scan_frames(dim_x, seed=10 * terms + dim_x)
    model = R.MODELS[terms]
    be.set_lag_correction(model, start)
    pool = Pool(be, frames)
    try:
        assert pool.first.ptr % 16 == 0 and pool.stride % 16 == 0 and pool.stride > pool.pitch * DIM_Y
        assert run_sequence(be, pool, (N,)) == N
        want, _, _ = B.lag_correct_host(model, band_of(frames), start=start)
        pool.assert_bands(pool.read(), want, what=(dim_x, terms, start))
    finally:
        pool.free()
    dark = R.dark_frame((DIM_Y, dim_x), seed=terms)
    dark[BAND[0] + 1, 5] = np.nan                                                    # a dead reference pixel inside the band
    flat = (dark + np.float32(30000)).astype(np.float32)
    be.set_flat_field(dark, flat)
    pool, ref = Pool(be, frames), None
    try:
        assert run_sequence(be, pool, (N,)) == N
        want, _, _ = B.lag_correct_host(model, band_of(frames), dark=dark[BAND[0]:BAND[0] + BAND[1]], start=start)
        assert not R.same_pixels(want, B.lag_correct_host(model, band_of(frames), start=start)[0])      # the dark matters
        pool.assert_bands(pool.read(), want, what=(dim_x, terms, start, "dark"))
        # the correction that follows sees x + d where it saw i
        be.flat_field_rows(pool.first, BAND[0], BAND[1], frame_stride=pool.stride, n_frames=N)
        full = frames.copy()
        full[:, BAND[0]:BAND[0] + BAND[1]] = want
        ref = Pool(be, full)
        be.flat_field_rows(ref.first, BAND[0], BAND[1], frame_stride=ref.stride, n_frames=N)
        assert np.array_equal(G.bits(pool.read()), G.bits(ref.read()))
    finally:
        be.clear_flat_field()
        be.clear_lag_correction()
        pool.free()
        if ref is not None:
            ref.free()


@pytest.mark.parametrize("start", R.STARTS)
@pytest.mark.parametrize("dim_x", [37, 64])
def test_split_invariance(be, dim_x, start):
    """the same seven frames as one call, as seven calls and as 3 + 4: the state travels from call to call"""
    frames = scan_frames(dim_x, seed=dim_x)
    be.set_lag_correction(R.MODELS[4], start)
    want, _, _ = B.lag_correct_host(R.MODELS[4], band_of(frames), start=start)
    try:
        results = []
        for cuts in ((N,), (1,) * N, (3, 4)):
            pool = Pool(be, frames)
            try:
                assert run_sequence(be, pool, cuts) == N
                results.append(pool.read())
                pool.assert_bands(results[-1], want, what=cuts)
            finally:
                pool.free()
        assert all(np.array_equal(G.bits(r), G.bits(results[0])) for r in results[1:])
    finally:
        be.clear_lag_correction()


def test_a_misaligned_base_takes_the_single_pixel_path(be):
    frames = scan_frames(64, seed=5)
    be.set_lag_correction(R.MODELS[3])
    pool = Pool(be, frames, shift=1)
    try:
        assert pool.first.ptr % 16 == 4 and pool.pitch % 16 == 0 and pool.stride % 16 == 0
        assert run_sequence(be, pool, (N,)) == N
        want, _, _ = B.lag_correct_host(R.MODELS[3], band_of(frames))
        pool.assert_bands(pool.read(), want)
    finally:
        be.clear_lag_correction()
        pool.free()


@pytest.mark.parametrize("dim_x", G.DIM_XS)
def test_a_band_past_the_grid_cap(be, dim_x):
    """1024 rows of 1025 pixels, or of 4100 in groups of four: 1 049 600 lanes against the cap of 4096 blocks of 256, so four blocks
    come round again for the band's final row -- with a state of their own there. Two frames; rows 0 .. 2 and 1027 .. 1029, the
    pitch padding and the gap keep their bits. The sequence starts at rest: x = y / B moves every pixel of the first frame too (a
    steady start leaves a first frame as it is, to rounding -- the response has unit DC gain)."""
    assert G.lanes(dim_x, dim_x % 4 == 0) > G.CAP_LANES
    frames = R.special_frames((2, G.DIM_Y, dim_x), seed=dim_x)
    first, count = G.BAND
    be.set_lag_correction(R.MODELS[2], "rest")
    s = G.Canvas(be, list(frames))
    try:
        assert s.first.ptr % 16 == 0 and s.stride % 16 == 0 and s.stride > s.pitch * G.DIM_Y       # dim_x alone decides the path
        be.lag_begin(dim_x, G.DIM_Y, first, count)
        be.lag_correct(s.first, frame_stride=s.stride, n_frames=2, row_first=first, row_count=count)
        assert be.lag_frames() == 2
        want, _, _ = B.lag_correct_host(R.MODELS[2], band_of(frames, G.BAND), start="rest")
        got = s.read()
        G.assert_canvas(s, got, s.expected(list(want)), dim_x)
        for k in range(2):   # the second visit wrote: nearly every pixel there differs from what it was
            tail_got, tail_was = G.second_visit(s, got, k), G.second_visit(s, s.before, k)
            assert np.count_nonzero(G.bits(tail_got) != G.bits(tail_was)) > 0.9 * tail_was.size
    finally:
        be.clear_lag_correction()
        s.free()


def test_reserve_bytes_hold_the_state_while_a_sequence_is_open(be):
    before = be.projection_reserve_bytes(96, 80)
    be.set_lag_correction(R.MODELS[3])
    assert be.projection_reserve_bytes(96, 80) == before
    be.lag_begin(96, 80, 10, 20)
    assert be.projection_reserve_bytes(96, 80) == before + 3 * 20 * 96 * 4
    be.lag_end()
    assert be.projection_reserve_bytes(96, 80) == before
    be.clear_lag_correction()


@pytest.mark.parametrize("start", R.STARTS)
def test_a_sequence_ended_and_reopened_behind_queued_work(start):
    """Four frames of 256 x 64 (16-byte vectors) are corrected, the sequence is ended and a new one begun at once, and four other
    frames are corrected, with nothing waited for in between: the first four keep the ended sequence's state -- it is retired behind
    them, not freed -- and the second four start from a state of their own."""
    dim_x, dim_y, band = 256, 64, (0, 64)
    model = R.MODELS[2]
    sets = [R.special_frames((4, dim_y, dim_x), seed=70), R.special_frames((4, dim_y, dim_x), seed=71)]
    with B.Backend(0, synchronous=False) as abe:
        abe.set_lag_correction(model, start)
        pools = [Pool(abe, frames) for frames in sets]
        for pool in pools:
            assert dim_x % 4 == 0 and pool.first.ptr % 16 == 0 and pool.pitch % 16 == 0 and pool.stride % 16 == 0
        for pool in pools:
            abe.lag_begin(dim_x, dim_y)
            for k in range(4):
                abe.lag_correct(pool.frame(k))
            abe.lag_end()                                   # the four passes above may still be queued: they keep their state
        for pool, frames in zip(pools, sets):
            want, _, _ = B.lag_correct_host(model, frames, start=start)
            assert not R.same_pixels(want, frames)
            pool.assert_bands(pool.read(), want, band=band, what=start)
        for pool in pools:
            pool.free()


def test_refusals_write_nothing(be):
    L = _lib.load()
    frames = scan_frames(64, seed=8)
    pool = Pool(be, frames)
    other = be.make_projection_device(65, DIM_Y)
    short = B.Projection(pool.first.ptr, 64, DIM_Y - 1, pitch=pool.pitch, on_device=True)

    def refused(call, *args, **kw):
        with pytest.raises(B.ParisHipError) as e:
            call(*args, **kw)
        assert e.value.status == INV

    try:
        refused(be.lag_begin, 64, DIM_Y, *BAND)                                    # begin without a setting
        refused(be.lag_correct, pool.first, row_first=BAND[0], row_count=BAND[1])  # correct without a setting
        be.lag_end()                                                               # no sequence: fine
        for bad in ([], list(R.MODELS[4]) + [(1e-3, 0.5)], [(0.5, 0.5)], [(float("nan"), 1.0)]):
            refused(be.set_lag_correction, bad)                                    # a refused model sets nothing
            refused(be.lag_begin, 64, DIM_Y, *BAND)
        refused(be.set_lag_correction, R.MODELS[2], "warm")
        be.set_lag_correction(R.MODELS[2])
        refused(be.lag_correct, pool.first, row_first=BAND[0], row_count=BAND[1])  # correct before begin
        for band in ((0, 0), (DIM_Y, 1), (3, DIM_Y - 2), (DIM_Y + 1, 0)):          # a zero or out-of-frame band
            refused(be.lag_begin, 64, DIM_Y, *band)
        refused(be.lag_begin, 0, DIM_Y, *BAND)
        be.set_flat_field(np.zeros((DIM_Y, 65), np.float32), np.ones((DIM_Y, 65), np.float32))
        refused(be.lag_begin, 64, DIM_Y, *BAND)                                    # a flat field of other dimensions
        be.clear_flat_field()
        be.lag_begin(64, DIM_Y, *BAND)
        refused(be.lag_begin, 64, DIM_Y, *BAND)                                    # begin twice
        refused(be.lag_correct, pool.first, row_first=BAND[0] + 1, row_count=BAND[1] - 1)      # another band
        refused(be.lag_correct, pool.first, row_first=BAND[0], row_count=BAND[1] - 1)
        refused(be.lag_correct, other, row_first=BAND[0], row_count=BAND[1])       # another dim_x
        refused(be.lag_correct, short, row_first=BAND[0], row_count=BAND[1])       # another dim_y
        refused(be.lag_correct, B.Projection(pool.first.ptr, 64, DIM_Y, pitch=4 * 64 - 4, on_device=True), row_first=BAND[0], row_count=BAND[1])
        fn = L.paris_hip_lag_correct_rows
        assert fn(be._ctx, pool.first.ptr, pool.pitch, pool.pitch * DIM_Y - 4, 2, 64, DIM_Y, *BAND) == INV     # overlapping frames
        assert fn(be._ctx, None, pool.pitch, 0, 1, 64, DIM_Y, *BAND) == INV
        assert fn(None, pool.first.ptr, pool.pitch, 0, 1, 64, DIM_Y, *BAND) == INV
        assert L.paris_hip_lag_begin(None, 64, DIM_Y, *BAND) == INV and L.paris_hip_lag_end(None) == INV
        assert L.paris_hip_set_lag_correction(be._ctx, None) == INV and L.paris_hip_clear_lag_correction(None) == INV
        assert L.paris_hip_lag_frames(be._ctx, None) == INV and L.paris_hip_lag_frames(None, C.byref(C.c_uint64())) == INV
        assert be.lag_frames() == 0                                                # no refused call counted a frame
        be.lag_correct(pool.first, n_frames=0, row_first=BAND[0], row_count=BAND[1])            # no frame: nothing happens
        assert be.lag_frames() == 0
        be.set_flat_field(np.zeros((DIM_Y, 65), np.float32), np.ones((DIM_Y, 65), np.float32))
        refused(be.lag_correct, pool.first, row_first=BAND[0], row_count=BAND[1])  # a flat field of other dimensions, set meanwhile
        be.clear_flat_field()
        be.clear_lag_correction()                                                  # closes the sequence
        assert be.lag_frames() == 0
        refused(be.lag_correct, pool.first, row_first=BAND[0], row_count=BAND[1])
        be.set_lag_correction(R.MODELS[2])
        be.lag_begin(64, DIM_Y, *BAND)
        be.set_lag_correction(R.MODELS[3])                                         # a replaced setting closes it too
        refused(be.lag_correct, pool.first, row_first=BAND[0], row_count=BAND[1])
        be.lag_end()
        be.lag_end()
        assert np.array_equal(G.bits(pool.read()), G.bits(pool.before))            # nothing was written
    finally:
        be.clear_flat_field()
        be.clear_lag_correction()
        be.clear_lag_correction()                                                  # clearing nothing is fine
        pool.free()
        be.free(other)


@pytest.mark.parametrize("references", [False, True])
def test_a_frame_of_the_pending_group_is_backprojected_as_it_was(references):
    """by reference: the group that refers to the frame is launched before the pass rewrites it; snapshots: it stays pending. Either
    way the volume holds the frame as it was when it was backprojected, and the frame holds the corrected pixels afterwards."""
    det = B.DetectorGeometry(*ORD_GEO)
    vg = B.calculate_volume_geometry(det)
    frame = np.random.default_rng(50).uniform(3000, 60000, (80, 96)).astype(np.float32)
    want_p, _, _ = B.lag_correct_host(R.MODELS[4], frame[None])

    def run(deferred):
        with B.Backend(0, synchronous=False) as abe:
            if deferred:
                abe.set_backproject_deferral(8)
                abe.set_backproject_references(references)
            abe.set_lag_correction(R.MODELS[4])
            abe.lag_begin(96, 80)
            v = abe.make_volume_device(vg.dim_x, vg.dim_y, vg.dim_z)
            d_p = B.load(abe, B.Projection(frame.copy(), 96, 80, idx=1))
            B.backproject(abe, d_p, v, 0, det, vg, False, False, None)
            if deferred:
                assert pending(abe) == 1
            abe.lag_correct(d_p)
            if deferred:
                assert pending(abe) == (0 if references else 1)
            return read(abe, d_p), volume_to_host(abe, v, vg)

    plain_p, plain_v = run(False)
    got_p, got_v = run(True)
    assert np.abs(plain_v).max() > 0 and np.array_equal(G.bits(plain_p), G.bits(want_p[0])) and not np.array_equal(plain_p, frame)
    assert np.array_equal(G.bits(got_v), G.bits(plain_v)) and np.array_equal(G.bits(got_p), G.bits(plain_p))


def test_without_a_setting_the_stages_give_the_bits_they_gave(be, oracle):
    """weight, filter and backprojection of a small case on a backend that never had a setting, on one whose setting was cleared and
    on one whose setting is in force but unused: the same bits, and the weighting is the oracle's"""
    O = oracle
    g = (64, 48, 0.2, 0.25, 1.5, -0.75, 100, 200, 45)
    det, odet = B.DetectorGeometry(*g), O.DetectorGeometry(*g)
    vg = B.calculate_volume_geometry(det)

    def run(mode):
        with B.Backend(0) as b:
            if mode != "never":
                b.set_lag_correction(R.MODELS[4])
                b.lag_begin(64, 48)
            if mode == "cleared":
                b.clear_lag_correction()
            v = b.make_volume_device(vg.dim_x, vg.dim_y, vg.dim_z)
            stages = []
            for i in range(3):
                d_p = B.load(b, B.Projection(O.lcg_projection(64, 48, i), 64, 48, idx=i))
                B.weight(b, d_p, det)
                stages.append(read(b, d_p))
                B.filter(b, d_p, det)
                stages.append(read(b, d_p))
                B.backproject(b, d_p, v, 0, det, vg, False, False, None)
                b.free(d_p)
            return stages, volume_to_host(b, v, vg)

    never, cleared, unused = run("never"), run("cleared"), run("set")
    assert np.array_equal(never[0][0], O.weight(O.lcg_projection(64, 48, 0), odet)) and np.abs(never[1]).max() > 0
    for other in (cleared, unused):
        assert all(np.array_equal(G.bits(a), G.bits(b)) for a, b in zip(never[0], other[0]))
        assert np.array_equal(G.bits(never[1]), G.bits(other[1]))
