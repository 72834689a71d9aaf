"""The ring filter on the device (paris_hip_ring_profile_* / paris_hip_set_ring_correction / paris_hip_ring_correct_rows, DESIGN.md
section 4.12): the profile's sums, the correction frame and the stats against the numpy restatement of the rule (tests/ring_rule.py)
bit for bit, the subtraction, bands, batches, the ordering rules, the settings' lifecycle, the driver and the quality figure."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import grid_cap_rule as G
import ring_rule as R
import test_gpu_flat_field as FF
import test_gpu_paris_hip as P
from oracle import formats as F
from paris_amd import _lib
from paris_amd import backend as B

pytestmark = pytest.mark.gpu

ORD_GEO = (96, 80, 0.2, 0.25, 1.5, -0.75, 100, 200, 45.0)
LAYOUTS = ("padded", "tight", "odd")   # rows padded to 256 B (pool buffer); pitch 4 dim_x; pitch 4 dim_x + 4: never 16-byte rows
SETTING = (R.H, R.FLOOR, R.LIMIT)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


@pytest.fixture(scope="module")
def be():
    with B.Backend(0) as b:
        yield b


def read(be, d):
    h = be.make_projection_host(d.dim_x, d.dim_y)
    be.copy_d2h(d, h)
    return h.buf.copy()


class Stack:
    """n frames of dim_x x dim_y one under the other in one device buffer; .first is frame 0 as a projection, .stride the bytes
    from one frame to the next"""

    def __init__(self, be, frames, layout="padded"):
        self.be, self.n = be, len(frames)
        self.dim_y, self.dim_x = frames[0].shape
        rows = self.dim_y * self.n
        if layout == "padded":
            self.all = self.owner = be.make_projection_device(self.dim_x, rows)
        else:
            cols = self.dim_x + (1 if layout == "odd" else 0)
            self.owner = be.make_volume_device(cols, rows, 1)
            self.all = be.wrap_projection(self.owner.ptr, 4 * cols, self.dim_x, rows)
        self.pitch = self.all.pitch
        self.stride = self.pitch * self.dim_y
        self.first = self.frame(0)
        be.upload_raw(np.concatenate([np.ascontiguousarray(f, np.float32) for f in frames]), self.all)

    def frame(self, k):
        return self.be.wrap_projection(self.all.ptr + k * self.stride, self.pitch, self.dim_x, self.dim_y)

    def read(self):
        return read(self.be, self.all).reshape(self.n, self.dim_y, self.dim_x)

    def free(self):
        self.be.free(self.owner)


def assert_finish_equals_rule(be, frames_in_order, counts, setting=SETTING, start=None, what=""):
    """finish(): the means, the correction frame and the stats equal the numpy rule's for the frames added, in the order added"""
    dim_y = frames_in_order[0].shape[0] if frames_in_order else None
    c, mean, st = be.ring_profile_finish(*setting)
    want_mean = R.mean_of(start if start is not None else R.sums(frames_in_order), counts)
    assert R.same_means(mean, want_mean), what
    counts = np.broadcast_to(np.asarray(counts, np.uint32), (mean.shape[0],))
    want_c, want_st = R.correction(want_mean, *setting, counts=counts)
    assert R.same_bits(c, want_c), what
    got_st = R.stats_of(st)
    assert got_st.pop("max_abs") == np.float32(want_st.pop("max_abs")) and got_st == want_st, what
    assert dim_y is None or mean.shape[0] == dim_y
    return c, mean, st


# ---- 1. the sums ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim_x,layout", [(96, "padded"), (100, "padded"), (100, "tight"), (100, "odd"), (96, "odd")])
def test_sums_equal_the_rule(be, dim_x, layout):
    """four pixels per lane where rows allow 16-byte loads (96 and 100 columns, padded or tight), one per lane otherwise (odd pitch)"""
    frames = R.scan(dim_x, 37, 3)
    s = Stack(be, frames, layout)
    assert (s.pitch % 16 == 0) == (layout != "odd")
    be.ring_profile_begin(dim_x, 37)
    be.ring_profile_add_rows(s.first, frame_stride=s.stride, n_frames=3)
    c, mean, st = assert_finish_equals_rule(be, frames, 3, what=(dim_x, layout))
    assert st.corrected > 50 and (st.frames_min, st.frames_max) == (3, 3)
    assert all(R.same_bits(a, b) for a, b in zip(s.read(), frames))      # the frames are only read
    s.free()


@pytest.mark.parametrize("dim_x", [260, 261])
def test_more_than_one_block(be, dim_x):
    """260 x 70 is 4550 lanes of four pixels, 261 x 70 is 18270 lanes of one: 18 and 72 blocks of 256"""
    frames = R.scan(dim_x, 70, 2, seed=11)
    for layout in ("padded", "tight"):
        s = Stack(be, frames, layout)
        be.ring_profile_begin(dim_x, 70)
        be.ring_profile_add_rows(s.first, frame_stride=s.stride, n_frames=2)
        assert_finish_equals_rule(be, frames, 2, what=(dim_x, layout))
        s.free()


@pytest.mark.parametrize("dim_x", G.DIM_XS)
def test_sums_of_a_band_past_the_grid_cap(be, dim_x):
    """1024 rows of 1025 pixels, or of 4100 in groups of four: 1 049 600 lanes against the cap of 4096 blocks of 256, so four blocks
    come round again and split their lane index a second time, into the band's final row. Two frames a stride larger than the frame
    apart; the frames, the rows around the band, the pitch padding and the gap are only read"""
    assert G.lanes(dim_x, dim_x % 4 == 0) > G.CAP_LANES
    frames = R.scan(dim_x, G.DIM_Y, 2, seed=dim_x)
    first, count = G.BAND
    counts = np.zeros(G.DIM_Y, np.uint32)
    counts[first:first + count] = 2
    s = G.Canvas(be, frames)
    try:
        be.ring_profile_begin(dim_x, G.DIM_Y)
        be.ring_profile_add_rows(s.first, row_first=first, row_count=count, frame_stride=s.stride, n_frames=2)
        c, mean, st = assert_finish_equals_rule(be, frames, counts, what=dim_x)
        assert (st.frames_min, st.frames_max) == (0, 2)
        assert not mean[:first].any() and not mean[first + count:].any()      # no sum landed in a row outside the band
        last = mean[first + count - 1]
        assert (last > 1).all() and c[first + count - 1, dim_x // 3] != 0      # the second visit added, up to the final column
        assert np.array_equal(G.bits(s.read()), G.bits(s.before))
    finally:
        be.ring_profile_discard()
        s.free()


@pytest.mark.parametrize("dim_x,dim_y", [(1, 1), (1, 7), (5, 1), (2, 2), (3, 3)])
def test_degenerate_frames(be, dim_x, dim_y):
    rng = np.random.default_rng(dim_x * 10 + dim_y)
    frames = [(2 + rng.normal(0, 1, (dim_y, dim_x))).astype(np.float32) for _ in range(2)]
    for layout in LAYOUTS:
        for h in (1, 2):
            s = Stack(be, frames, layout)
            be.ring_profile_begin(dim_x, dim_y)
            be.ring_profile_add_rows(s.first, frame_stride=s.stride, n_frames=2)
            assert_finish_equals_rule(be, frames, 2, setting=(h, 0.0, 0.0), what=(dim_x, dim_y, layout, h))
            s.free()


@pytest.mark.parametrize("n", [1, 3, 2 * _lib.RING_FRAMES_MAX + 3])
def test_frames_per_call(be, n):
    """one call of n frames, also more than one launch serves; values of very different size, so the order of the additions shows"""
    rng = np.random.default_rng(8)
    frames = list((rng.normal(0, 1, (n, 9, 12)) * 10.0 ** rng.integers(-6, 7, (n, 9, 12))).astype(np.float32))
    assert _lib.RING_FRAMES_MAX == R.FRAMES_MAX
    if n > 3:   # the sequential sum differs from the sum of per-launch partial sums: the test can tell them apart
        parts = sum(R.sums(frames[k:k + R.FRAMES_MAX]) for k in range(0, n, R.FRAMES_MAX))
        assert np.count_nonzero(parts != R.sums(frames)) > 10
    for layout in ("padded", "odd"):
        s = Stack(be, frames, layout)
        be.ring_profile_begin(12, 9)
        be.ring_profile_add_rows(s.first, frame_stride=s.stride, n_frames=n)
        c, mean, st = assert_finish_equals_rule(be, frames, n, setting=(2, 0.0, 0.0), what=(n, layout))
        assert (st.frames_min, st.frames_max) == (n, n)
        s.free()


def test_three_calls_of_one_frame_equal_one_call_of_three(be):
    frames = R.awkward_scan(100, 37, 3)
    s = Stack(be, frames)
    be.ring_profile_begin(100, 37)
    be.ring_profile_add_rows(s.first, frame_stride=s.stride, n_frames=3)
    c1, m1, _ = assert_finish_equals_rule(be, frames, 3)
    be.ring_profile_begin(100, 37)
    for k in range(3):
        be.ring_profile_add_rows(s.frame(k))
    c2, m2, _ = assert_finish_equals_rule(be, frames, 3)
    assert np.array_equal(bits(m1), bits(m2)) and np.array_equal(bits(c1), bits(c2))
    s.free()


@pytest.mark.parametrize("layout", ["padded", "odd"])
def test_a_band_equals_the_same_rows_of_whole_frame_adds(be, layout):
    first, count = 9, 19
    frames = R.scan(100, 37, 3, seed=21)
    s = Stack(be, frames, layout)
    counts = np.zeros(37, np.uint32)
    counts[first:first + count] = 3
    be.ring_profile_begin(100, 37)
    be.ring_profile_add_rows(s.first, row_first=first, row_count=count, frame_stride=s.stride, n_frames=3)
    be.ring_profile_add_rows(s.first, row_first=37, row_count=0, frame_stride=s.stride, n_frames=3)   # an empty band adds nothing
    c, mean, st = assert_finish_equals_rule(be, frames, counts, what=layout)
    assert (st.frames_min, st.frames_max) == (0, 3)
    assert not mean[:first].any() and not mean[first + count:].any() and not c[:first].any() and not c[first + count:].any()
    be.ring_profile_begin(100, 37)
    be.ring_profile_add_rows(s.first, frame_stride=s.stride, n_frames=3)
    c_whole, mean_whole, _ = assert_finish_equals_rule(be, frames, 3)
    assert np.array_equal(bits(mean[first:first + count]), bits(mean_whole[first:first + count]))
    assert np.array_equal(bits(c[first:first + count]), bits(c_whole[first:first + count]))
    # two whole frames, then one more on the band only: the rows' counts differ
    be.ring_profile_begin(100, 37)
    be.ring_profile_add_rows(s.first, frame_stride=s.stride, n_frames=2)
    be.ring_profile_add_rows(s.frame(2), row_first=first, row_count=count)
    start = R.sums(frames[:2])
    start[first:first + count] += frames[2][first:first + count].astype(np.float64)
    counts = np.full(37, 2, np.uint32)
    counts[first:first + count] = 3
    c, mean, st = assert_finish_equals_rule(be, frames, counts, start=start)
    assert (st.frames_min, st.frames_max) == (2, 3)
    s.free()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_frames_with_a_nan_payload_an_inf_negative_zeros_and_denormals(be, layout):
    frames = R.awkward_scan(100, 37, 5)
    s = Stack(be, frames, layout)
    be.ring_profile_begin(100, 37)
    be.ring_profile_add_rows(s.first, frame_stride=s.stride, n_frames=5)
    c, mean, st = assert_finish_equals_rule(be, frames, 5, what=layout)
    assert np.isnan(mean[1, 2]) and mean[2, 99] == np.inf
    assert np.isfinite(mean[5, 0]) and mean[5, 0] > 1e38                             # 2 x 3e38 is beyond fp32, not beyond the double sum
    assert not mean[3].any() and not np.signbit(mean[3]).any()                       # 0 + -0 = +0
    assert mean[4, 0] == np.float32(1e-41) and mean[4, 0] != 0                       # a denormal mean survives
    assert st.not_finite == 5 + 3                                                    # h = 2: the windows of columns 0 .. 4 and 97 .. 99
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(s.read(), frames))
    s.free()


def test_a_profile_without_a_frame(be):
    be.ring_profile_begin(20, 6)
    c, mean, st = be.ring_profile_finish(*SETTING)
    assert not c.any() and not mean.any() and (st.corrected, st.frames_min, st.frames_max) == (0, 0, 0)


# ---- 2. the subtraction ---------------------------------------------------------------------------------------------------------------

def scan_correction(dim_x, dim_y, n=8, seed=3):
    frames = R.scan(dim_x, dim_y, n, seed)
    c, st = R.correction(R.mean_of(R.sums(frames), n), *SETTING)
    assert st["corrected"] > 20
    return frames, c


@pytest.mark.parametrize("dim_x,dim_y,layout", [(96, 37, "padded"), (100, 37, "tight"), (100, 37, "odd"), (260, 70, "padded"), (261, 70, "padded")])
def test_correct_rows_equals_p_minus_c_and_leaves_the_rest_alone(be, dim_x, dim_y, layout):
    frames, c = scan_correction(dim_x, dim_y, n=3)
    c[6, 4:8] = [0.5, -0.25, 0.125, 1.0]                    # a group of four with a correction each: the 16-byte store
    free = np.argwhere(c == 0)
    for k, (y, x) in enumerate(free[::max(1, len(free) // 12)][:12]):   # pixels without a correction keep every bit
        frames[k % 3].view(np.uint32)[y, x] = R.NAN_PAYLOAD + k
    frames[1][6, 5] = np.nan                                 # a corrected NaN stays a NaN
    be.set_ring_correction(c)
    try:
        first, count = 5, dim_y - 9
        s = Stack(be, frames, layout)
        be.ring_correct_rows(s.first, row_first=first, row_count=count, frame_stride=s.stride, n_frames=3)
        band = s.read()
        for k in range(3):
            want = frames[k].copy()
            want[first:first + count] = R.subtract(frames[k], c)[first:first + count]
            keep = (c == 0) | ~np.isin(np.arange(dim_y), np.arange(first, first + count))[:, None]
            assert np.array_equal(bits(band[k])[keep], bits(frames[k])[keep]), (k, "untouched pixels")
            assert np.array_equal(band[k], want, equal_nan=True) and np.array_equal(bits(band[k])[~np.isnan(want)], bits(want)[~np.isnan(want)]), k
        assert np.count_nonzero(bits(band) != bits(np.stack(frames))) > 50
        s.free()
        s = Stack(be, frames[:1], layout)                    # one whole frame, the last row alone, an empty band
        be.ring_correct_rows(s.first, row_first=0, row_count=dim_y - 1)
        be.ring_correct_rows(s.first, row_first=dim_y - 1, row_count=1)
        be.ring_correct_rows(s.first, row_first=dim_y, row_count=0)
        want = R.subtract(frames[0], c)
        assert np.array_equal(bits(s.read()[0])[~np.isnan(want)], bits(want)[~np.isnan(want)])
        s.free()
    finally:
        be.clear_ring_correction()


@pytest.mark.parametrize("dim_x", G.DIM_XS)
def test_correct_rows_of_a_band_past_the_grid_cap(be, dim_x):
    """the shapes of test_sums_of_a_band_past_the_grid_cap: the correction is non-zero in the lanes of the second visit as well -- in
    the band's final row up to the final columns, as a whole group of four and as single pixels of a group -- and in the rows around the
    band, which must not be written"""
    frames, c = scan_correction(dim_x, G.DIM_Y, n=2, seed=dim_x)
    first, count = G.BAND
    last = first + count - 1
    c[last, dim_x - 4:] = [0.5, -0.25, 0.125, 1.0]          # the final group of four: the 16-byte store
    c[last, dim_x - 8:dim_x - 4] = [0.375, 0, 0, -0.375]    # a group with two corrections: single stores
    c[last, dim_x - 1024] = -0.5                             # the first pixel every shape's second visit serves
    assert c[:first].any() and c[last + 1:].any() and np.count_nonzero(c[last, dim_x - 1024:]) >= 7
    quiet = np.argwhere(c[first:last + 1] == 0)[::100003]    # pixels of the band without a correction keep every bit
    for k, (y, x) in enumerate(quiet):
        frames[k % 2].view(np.uint32)[first + y, x] = R.NAN_PAYLOAD + k
    be.set_ring_correction(c)
    s = G.Canvas(be, frames)
    try:
        be.ring_correct_rows(s.first, row_first=first, row_count=count, frame_stride=s.stride, n_frames=2)
        got = s.read()
        G.assert_canvas(s, got, s.expected([R.subtract(f, c)[first:last + 1] for f in frames]), dim_x)
        for k in range(2):
            band_got, band_was = s.frame_of(got, k)[first:last + 1], frames[k][first:last + 1]
            assert np.array_equal(bits(band_got)[c[first:last + 1] == 0], bits(band_was)[c[first:last + 1] == 0]), "NaN payloads included"
            tail = bits(band_got[-1, dim_x - 1024:]) != bits(band_was[-1, dim_x - 1024:])
            assert np.array_equal(tail, c[last, dim_x - 1024:] != 0)      # the second visit wrote exactly the corrected pixels
    finally:
        be.clear_ring_correction()
        s.free()


def pending(be):
    n, ptr = C.c_uint32(0), C.c_void_p()
    assert be._L.paris_hip_pending_backprojections(be._ctx, C.byref(n), C.byref(ptr)) == 0
    return n.value


def test_a_zero_correction_launches_nothing():
    """with references the pass would launch the pending group the frame belongs to: an all-zero correction frame leaves it pending"""
    det = B.DetectorGeometry(*ORD_GEO)
    vg = B.calculate_volume_geometry(det)
    frames, c = scan_correction(96, 80, n=4, seed=50)
    with B.Backend(0, synchronous=False) as abe:
        abe.set_backproject_deferral(8)
        abe.set_backproject_references(True)
        v = abe.make_volume_device(vg.dim_x, vg.dim_y, vg.dim_z)
        d_p = B.load(abe, B.Projection(frames[0].copy(), 96, 80, idx=1))
        B.backproject(abe, d_p, v, 0, det, vg, False, False, None)
        assert pending(abe) == 1
        zero = np.zeros((80, 96), np.float32)
        zero[3, 3] = -0.0
        abe.set_ring_correction(zero)
        abe.ring_correct_rows(d_p)
        assert pending(abe) == 1
        abe.set_ring_correction(c)
        abe.ring_correct_rows(d_p)
        assert pending(abe) == 0
        assert np.array_equal(bits(read(abe, d_p)), bits(R.subtract(frames[0], c)))


# ---- 3. ordering ----------------------------------------------------------------------------------------------------------------------

def test_a_held_back_weighting_is_flushed_before_add_and_before_correct():
    det = B.DetectorGeometry(*ORD_GEO)
    frames, c = scan_correction(96, 80, n=4, seed=50)

    def run(fusion):
        with B.Backend(0, synchronous=False) as abe:
            abe.set_stage_fusion(fusion)
            abe.set_ring_correction(c)
            abe.ring_profile_begin(96, 80)
            d_p = B.load(abe, B.Projection(frames[0].copy(), 96, 80, idx=2))
            B.weight(abe, d_p, det)            # with fusion: held back until something touches the frame
            abe.ring_profile_add_rows(d_p)
            weighted = read(abe, d_p)
            mean = abe.ring_profile_finish(*SETTING)[1]
            d_q = B.load(abe, B.Projection(frames[1].copy(), 96, 80, idx=3))
            B.weight(abe, d_q, det)
            abe.ring_correct_rows(d_q)
            return weighted, mean, read(abe, d_q)

    plain, fused = run(False), run(True)
    assert not np.array_equal(bits(plain[0]), bits(frames[0])) and np.array_equal(bits(plain[1]), bits(plain[0]))   # one frame: mean = frame
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(plain, fused))
    assert np.array_equal(bits(plain[2]), bits(R.subtract(read_weighted(frames[1], det), c)))


def read_weighted(frame, det):
    with B.Backend(0) as wbe:
        d = B.load(wbe, B.Projection(frame.copy(), det.n_row, det.n_col, idx=0))
        B.weight(wbe, d, det)
        return read(wbe, d)


def volume_to_host(abe, v, vg):
    h = abe.make_volume_host(vg.dim_x, vg.dim_y, vg.dim_z)
    abe.copy_d2h(v, h)
    return h.buf.copy()


@pytest.mark.parametrize("references", [False, True])
@pytest.mark.parametrize("what", ["add", "correct"])
def test_a_frame_of_the_pending_group_is_backprojected_as_it_was(references, what):
    """by reference: the group that refers to the frame is launched before the pass touches it; snapshots: it stays pending"""
    det = B.DetectorGeometry(*ORD_GEO)
    vg = B.calculate_volume_geometry(det)
    frames, c = scan_correction(96, 80, n=4, seed=50)

    def run(deferred):
        with B.Backend(0, synchronous=False) as abe:
            if deferred:
                abe.set_backproject_deferral(8)
                abe.set_backproject_references(references)
            abe.set_ring_correction(c)
            abe.ring_profile_begin(96, 80)
            v = abe.make_volume_device(vg.dim_x, vg.dim_y, vg.dim_z)
            d_p = B.load(abe, B.Projection(frames[0].copy(), 96, 80, idx=1))
            B.backproject(abe, d_p, v, 0, det, vg, False, False, None)
            if deferred:
                assert pending(abe) == 1
            if what == "add":
                abe.ring_profile_add_rows(d_p)
            else:
                abe.ring_correct_rows(d_p)
            if deferred:
                assert pending(abe) == (0 if references else 1)
            mean = abe.ring_profile_finish(*SETTING)[1]
            return read(abe, d_p), volume_to_host(abe, v, vg), mean

    want_p, want_v, want_m = run(False)
    got_p, got_v, got_m = run(True)
    assert np.abs(want_v).max() > 0 and np.array_equal(bits(want_p), bits(frames[0])) == (what == "add")
    assert np.array_equal(bits(got_v), bits(want_v)) and np.array_equal(bits(got_p), bits(want_p)) and np.array_equal(bits(got_m), bits(want_m))


def test_replacement_clear_discard_and_a_second_begin_respect_queued_work():
    dim = 1024
    frames = R.scan(dim, dim, 5, seed=60, off=np.zeros((dim, dim), np.float32))
    rng = np.random.default_rng(61)
    c_a = np.where(rng.random((dim, dim)) < 0.01, np.float32(0.5), np.float32(0))
    c_b = np.where(rng.random((dim, dim)) < 0.01, np.float32(-0.25), np.float32(0))
    with B.Backend(0, synchronous=False) as abe:
        ds = [abe.make_projection_device(dim, dim) for _ in frames]
        for h, d in zip(frames, ds):
            abe.upload_raw(h, d)
        abe.ring_profile_begin(dim, dim)
        for d in ds[:4]:
            abe.ring_profile_add_rows(d)
        abe.ring_profile_begin(dim, dim)        # the four adds above may still be queued: they keep the old sums
        abe.ring_profile_add_rows(ds[4])
        c, mean, st = abe.ring_profile_finish(1, 0.0, 0.0)
        assert np.array_equal(bits(mean), bits(frames[4])) and (st.frames_min, st.frames_max) == (1, 1)
        abe.ring_profile_begin(dim, dim)
        abe.ring_profile_add_rows(ds[0])
        abe.ring_profile_discard()               # the add may still be queued
        abe.ring_profile_discard()               # discarding nothing is fine
        with pytest.raises(B.ParisHipError):
            abe.ring_profile_add_rows(ds[0])
        abe.set_ring_correction(c_a)
        for d in ds[:4]:
            abe.ring_correct_rows(d)
        abe.set_ring_correction(c_b)             # the four passes above may still be queued: they keep the old frame
        abe.ring_correct_rows(ds[4])
        abe.clear_ring_correction()
        for h, d in zip(frames[:4], ds):
            assert np.array_equal(bits(read(abe, d)), bits(R.subtract(h, c_a))), "before the replacement"
        assert np.array_equal(bits(read(abe, ds[4])), bits(R.subtract(frames[4], c_b))), "after the replacement"
        with pytest.raises(B.ParisHipError):     # cleared: the pass is refused
            abe.ring_correct_rows(ds[4])
        for d in ds:
            abe.free(d)


def test_reserve_bytes_grow_by_8_and_4_bytes_per_pixel_and_shrink_again(be):
    before = be.projection_reserve_bytes(96, 80)
    profile, correction = B.ring_filter_check(2, 0.0, 0.0, 96, 80)
    assert (profile, correction) == (8 * 96 * 80, 4 * 96 * 80)
    be.ring_profile_begin(96, 80)
    assert be.projection_reserve_bytes(96, 80) == before + profile
    be.ring_profile_begin(96, 80)                # replaced: one profile's bytes, not both
    assert be.projection_reserve_bytes(96, 80) == before + profile
    be.set_ring_correction(np.zeros((80, 96), np.float32))
    assert be.projection_reserve_bytes(96, 80) == before + profile + correction
    be.ring_profile_finish(*SETTING)
    assert be.projection_reserve_bytes(96, 80) == before + correction
    be.set_ring_correction(np.ones((80, 96), np.float32))
    assert be.projection_reserve_bytes(96, 80) == before + correction
    be.ring_profile_begin(96, 80)
    be.ring_profile_discard()
    be.clear_ring_correction()
    assert be.projection_reserve_bytes(96, 80) == before


# ---- 4. refusals ----------------------------------------------------------------------------------------------------------------------

def test_refusals(be):
    L = _lib.load()
    INV = _lib.ERROR_INVALID_ARGUMENT
    d = be.make_projection_device(96, 80)
    other = be.make_projection_device(97, 80)
    rf = _lib.RingFilter(2, 0.0, 0.0)
    out, st = np.zeros((80, 96), np.float32), _lib.RingStats()
    # without a profile / a setting
    with pytest.raises(B.ParisHipError) as e:
        be.ring_profile_add_rows(d)
    assert e.value.status == INV
    with pytest.raises(B.ParisHipError):
        be.ring_correct_rows(d)
    with pytest.raises(B.ParisHipError):
        be.ring_profile_finish(2)
    assert L.paris_hip_ring_profile_finish(be._ctx, C.byref(rf), out.ctypes.data, None, C.byref(st)) == INV
    be.ring_profile_discard()
    be.clear_ring_correction()                   # clearing nothing is fine
    # begin / set
    assert L.paris_hip_ring_profile_begin(be._ctx, 0, 80) == INV and L.paris_hip_ring_profile_begin(be._ctx, 96, 0) == INV
    assert L.paris_hip_ring_profile_begin(be._ctx, 1 << 16, 1 << 16) == _lib.ERROR_UNSUPPORTED
    assert L.paris_hip_ring_profile_begin(None, 96, 80) == INV
    assert L.paris_hip_set_ring_correction(be._ctx, None, 96, 80) == INV
    assert L.paris_hip_set_ring_correction(be._ctx, out.ctypes.data, 0, 80) == INV
    for bad in (np.nan, np.inf, -np.inf):
        c = out.copy()
        c[79, 95] = bad
        with pytest.raises(B.ParisHipError) as e:
            be.set_ring_correction(c)
        assert e.value.status == INV
    with pytest.raises(B.ParisHipError):         # a refused frame sets nothing
        be.ring_correct_rows(d)
    with pytest.raises(ValueError):
        be.set_ring_correction(np.zeros(5, np.float32))
    be.ring_profile_begin(96, 80)
    be.set_ring_correction(np.ones((80, 96), np.float32))
    try:
        for call in (be.ring_profile_add_rows, be.ring_correct_rows):
            with pytest.raises(B.ParisHipError):
                call(other)                                                                       # other dimensions
            with pytest.raises(B.ParisHipError):
                call(B.Projection(d.ptr, 96, 79, pitch=d.pitch, on_device=True))
            with pytest.raises(B.ParisHipError):
                call(B.Projection(d.ptr, 96, 80, pitch=4 * 96 - 4, on_device=True))              # a bad pitch
            with pytest.raises(B.ParisHipError):
                call(B.Projection(d.ptr, 96, 80, pitch=d.pitch + 2, on_device=True))
            with pytest.raises(B.ParisHipError):
                call(d, row_first=70, row_count=11)                                               # a bad band
            with pytest.raises(B.ParisHipError):
                call(d, row_first=81, row_count=0)
        for fn in (L.paris_hip_ring_profile_add_rows, L.paris_hip_ring_correct_rows):
            assert fn(be._ctx, d.ptr, d.pitch, d.pitch * 80 - 4, 2, 96, 80, 0, 80) == INV       # overlapping frames
            assert fn(be._ctx, d.ptr, d.pitch, d.pitch * 80 + 2, 2, 96, 80, 0, 80) == INV
            assert fn(be._ctx, None, d.pitch, 0, 1, 96, 80, 0, 80) == INV
            assert fn(None, d.ptr, d.pitch, 0, 1, 96, 80, 0, 80) == INV
        # finish: a refused setting or a missing output leaves the profile open
        assert L.paris_hip_ring_profile_finish(be._ctx, None, out.ctypes.data, None, None) == INV
        assert L.paris_hip_ring_profile_finish(be._ctx, C.byref(_lib.RingFilter(0, 0.0, 0.0)), out.ctypes.data, None, None) == INV
        assert L.paris_hip_ring_profile_finish(be._ctx, C.byref(_lib.RingFilter(2, 0.2, 0.1)), out.ctypes.data, None, None) == INV
        assert L.paris_hip_ring_profile_finish(be._ctx, C.byref(rf), None, None, None) == INV
        assert L.paris_hip_ring_profile_finish(be._ctx, C.byref(rf), out.ctypes.data, None, C.byref(st)) == _lib.SUCCESS
        assert (st.frames_min, st.frames_max, st.corrected) == (0, 0, 0)                          # a refused add adds nothing
    finally:
        be.ring_profile_discard()
        be.clear_ring_correction()
    be.free(d)
    be.free(other)


# ---- 5. the driver and the C++ mirror against the Python mirror ------------------------------------------------------------------

def drv_zingers(flat):
    """(threshold, polarity): on line integrals in 0 .. 3 the zinger test's dark 1.5; on counts up to 65535 a bright 30000 -- either flags
    a few percent of the pixels, far from max_hits, so whole frames (pre-pass) and bands (slabs) agree"""
    return (1.5, -1) if flat else (30000.0, 1)


def mirror_volume(frames, dark, flat, zingers, setting):
    """PARIS's loop through the Python mirror, twice over the frames: the pre-pass (correct -> zinger filter -> profile), then correct ->
    zinger filter -> ring correction -> weight -> filter -> backproject. Returns the volume, c and the stats"""
    det = B.DetectorGeometry(*FF.DRV_GEO)
    vg = B.calculate_volume_geometry(det)
    n_row, n_col = FF.DRV_GEO[:2]
    with B.Backend(0) as mbe:
        if flat is not None:
            mbe.set_flat_field(dark, flat, 1e-5)
        if zingers:
            mbe.set_zinger_filter(drv_zingers(flat is not None)[0], 0.0, drv_zingers(flat is not None)[1], n_row, n_col)

        def loaded(i, fr):
            d_p = B.load(mbe, B.Projection(fr.astype(np.float32), n_row, n_col, idx=i))
            if flat is not None:
                mbe.flat_field_rows(d_p)
            if zingers:
                mbe.zinger_filter_rows(d_p)
            return d_p

        mbe.ring_profile_begin(n_row, n_col)
        lines = []
        for i, fr in enumerate(frames):
            d_p = loaded(i, fr)
            lines.append(read(mbe, d_p))
            mbe.ring_profile_add_rows(d_p)
            mbe.free(d_p)
        c, mean, st = mbe.ring_profile_finish(*setting)
        want_c, want_st = R.correction(R.mean_of(R.sums(lines), len(lines)), *setting, counts=np.full(n_col, len(lines), np.uint32))
        assert R.same_bits(c, want_c) and R.stats_of(st)["corrected"] == want_st["corrected"]
        mbe.set_ring_correction(c)
        v = mbe.make_volume_device(vg.dim_x, vg.dim_y, vg.dim_z)
        for i, fr in enumerate(frames):
            d_p = loaded(i, fr)
            mbe.ring_correct_rows(d_p)
            assert np.array_equal(bits(read(mbe, d_p)), bits(R.subtract(lines[i], c))), i
            B.weight(mbe, d_p, det)
            B.filter(mbe, d_p, det)
            B.backproject(mbe, d_p, v, 0, det, vg, False, False, None)
            mbe.free(d_p)
        h = mbe.make_volume_host(vg.dim_x, vg.dim_y, vg.dim_z)
        mbe.copy_d2h(v, h)
    return h.buf.reshape(vg.dim_z, vg.dim_y, vg.dim_x).copy(), c, st


@pytest.mark.parametrize("flat,zingers", [(True, True), (True, False), (False, True), (False, False)])
def test_driver_and_cpp_mirror_against_the_python_mirror(tmp_path, flat, zingers):
    n_row, n_col = FF.DRV_GEO[:2]
    n_frames = 75
    geo, ref, counts_dir, fr, d, f = FF.driver_set(tmp_path, n_frames)
    fr[:, :, 20] = fr[:, :, 20] // 2             # a column with half the gain, two pixels with a third: offsets of ln 2 and ln 3 with --flat
    fr[:, 30, 40:42] = fr[:, 30, 40:42] // 3
    fr[::3, 12, 8] = 65535                       # zingers
    (counts_dir / "a.his").write_bytes(F.his_file_bytes(fr[:70], 4, 32))
    (counts_dir / "b.his").write_bytes(F.his_file_bytes(fr[70:], 4, 32))
    # with --flat the frames are line integrals in 0 .. 3, and a floor of 0.3 keeps the planted offsets and little else; without it
    # they are counts, and the same floor corrects nearly every pixel
    setting = (2, 0.3, 0.0)
    want, c, st = mirror_volume(fr, d if flat else None, f if flat else None, zingers, setting)
    assert np.abs(want).max() > 0 and st.corrected > (40 if flat else 1000) and (not flat or (c[:, 20] > 0.3).sum() > 40)
    base = [P.EXE, "--geometry", geo, "--input", counts_dir, "--rings", "2:0.3"]
    if flat:
        base += ["--flat", ref / "flat.his", "--dark", ref / "dark.his"]
    if zingers:
        base += ["--zingers", drv_zingers(flat)[0]]
    report = "ring filter on: %d frame(s) in the pre-pass" % n_frames
    counts = "%d pixel(s) corrected, %d below the floor, %d above the limit, %d not finite" % (st.corrected, st.below_floor, st.above_limit, st.not_finite)
    for k, extra in enumerate((["--slabs", 1], ["--slabs", 3, "--batch", 7], ["--slabs", 2, "--batch", 1])):   # batch 1: the per-slot path
        o = tmp_path / ("o%d" % k)
        r = subprocess.run([str(a) for a in base + ["--output", o] + extra], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        assert report in r.stdout and counts in r.stdout, r.stdout
        assert np.array_equal(bits(F.ddbvf_read(str(o / "vol.ddbvf"))[1]), bits(want)), extra
    # refused before any device work
    for bad in [] if flat or zingers else ("abc", "0", "33", "2:-1", "2:0.1:0.05", "2:0.1:0.2:3", "2:", "2:x"):
        r = subprocess.run([str(a) for a in base[:5] + ["--output", tmp_path / "bad", "--rings", bad]], capture_output=True, text=True, timeout=300)
        assert r.returncode == 1 and "--rings" in r.stderr, (bad, r.stderr)
    assert not (tmp_path / "bad").exists()
    # PARIS's loop through paris::hip with the pre-pass (paris_hip_demo [--flat] [--zingers] --rings)
    raw = tmp_path / "in.raw"
    fr.astype(np.float32).tofile(raw)
    d.tofile(tmp_path / "dark.raw")
    f.tofile(tmp_path / "flat.raw")
    out = tmp_path / "demo.raw"
    args = [FF.DEMO] + [str(v) for v in FF.DRV_GEO] + [str(n_frames), str(raw), str(out), "--slabs", "2", "--rings", "2", "0.3", "0"]
    if flat:
        args += ["--flat", str(tmp_path / "dark.raw"), str(tmp_path / "flat.raw"), "1e-05"]
    if zingers:
        args += ["--zingers", str(drv_zingers(flat)[0]), "0", str(drv_zingers(flat)[1])]
    r = subprocess.run(args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr + r.stdout
    assert np.array_equal(bits(np.fromfile(out, np.float32).reshape(want.shape)), bits(want))


# ---- 6. quality -----------------------------------------------------------------------------------------------------------------------

def test_quality_of_a_reconstruction_with_corrected_rings(oracle):
    """Relative RMS against the ORACLE's reconstruction from the clean frames: the 192 x 12 case of tests/ring_rule.py, head phantom, 360
    views, stationary offsets in 3 % of the pixels plus a column and a pair of columns, h = 2, floor 0.035, limit 0.25. The oracle with the
    numpy rule (tests/test_ring_host.py): 0.085533 uncorrected, 0.021931 corrected; the device's sums and subtraction are exact, only
    the row filter's FFT rounding differs."""
    import defect_rule as D
    det, odet = B.DetectorGeometry(*R.QUALITY_GEO), oracle.DetectorGeometry(*R.QUALITY_GEO)
    vg, ovg = B.calculate_volume_geometry(det), oracle.calculate_volume_geometry(odet)
    lines = R.quality_frames(vg.dim_x, vg.l_vx_x)
    off = R.quality_offsets()
    ringed = [p + off for p in lines]
    clean = oracle.reconstruct(odet, ovg, len(lines), projections=lines)
    setting = (R.QUALITY_H, R.QUALITY_FLOOR, R.QUALITY_LIMIT)

    def reconstruct(frames, rings):
        with B.Backend(0, synchronous=False) as qbe:
            qbe.set_paris_loop_defaults(48)
            st = None
            if rings:
                s = Stack(qbe, frames)
                qbe.ring_profile_begin(det.n_row, det.n_col)
                for k in range(0, len(frames), 48):
                    qbe.ring_profile_add_rows(s.frame(k), frame_stride=s.stride, n_frames=min(48, len(frames) - k))
                c, mean, st = qbe.ring_profile_finish(*setting)
                s.free()
                qbe.set_ring_correction(c)
            v = qbe.make_volume_device(vg.dim_x, vg.dim_y, vg.dim_z)
            for i, fr in enumerate(frames):
                d_p = qbe.make_projection_device(det.n_row, det.n_col)
                qbe.upload_raw(fr, d_p)
                d_p.idx = i
                if rings:
                    qbe.ring_correct_rows(d_p)
                B.weight(qbe, d_p, det)
                B.filter(qbe, d_p, det)
                B.backproject(qbe, d_p, v, 0, det, vg, False, False, None)
                qbe.free(d_p)
            qbe.flush()
            return volume_to_host(qbe, v, vg), st

    a = D.relative_rms(reconstruct(ringed, False)[0], clean)
    got, st = reconstruct(ringed, True)
    b = D.relative_rms(got, clean)
    untouched, st_clean = reconstruct(lines, True)
    k = D.relative_rms(untouched, clean)
    print("ring quality: relative RMS against the oracle's clean volume %.5g uncorrected, %.5g corrected (%d pixels), %.5g for the clean "
          "frames through the filter (%d pixels)" % (a, b, st.corrected, k, st_clean.corrected))
    assert st.corrected == R.through_the_rule(ringed)[2]["corrected"] and st_clean.corrected == 0
    assert b < a
    assert b <= R.BOUND * R.CAL_CORRECTED
