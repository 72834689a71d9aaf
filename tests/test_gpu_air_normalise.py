"""The air-region normalisation on the device (paris_hip_set_air_region / paris_hip_air_normalize_rows / paris_hip_air_measure /
paris_hip_air_stats): every value, count and pixel against the numpy restatement of the rule
(tests/air_rule.py) bit for bit -- rectangles, layouts, batches, bands, degenerate frames, the counters, the settings' lifecycle, the
refusals and the ordering rules."""
import ctypes as C

import numpy as np
import pytest

import air_rule as A
import grid_cap_rule as G
from paris_amd import _lib
from paris_amd import backend as B
from test_gpu_ring_correction import LAYOUTS, ORD_GEO, Stack, bits, pending, read, volume_to_host

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    with B.Backend(0) as b:
        yield b


def same_pixels(got, want):
    """bit for bit, except that a NaN the subtraction made may carry any payload"""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    made = np.isnan(want)
    return np.array_equal(np.isnan(got), made) and np.array_equal(bits(got)[~made], bits(want)[~made])


def assert_measure_and_normalise(be, frames, rect, layout, rows=None, what="", **setting):
    """air_measure() gives the rule's values and counts and writes nothing; air_normalize() leaves the rule's frames and counts"""
    dim_y, dim_x = frames[0].shape
    n = len(frames)
    a, cnt, whys = A.values(frames, rect, **setting)
    s = Stack(be, frames, layout)
    be.set_air_region(*rect, dim_x, dim_y, **setting)
    try:
        got_a, got_n = be.air_measure(s.first, frame_stride=s.stride, n_frames=n)
        assert A.same_bits(got_a, a) and np.array_equal(got_n, cnt), (what, got_a, a)
        assert all(np.array_equal(bits(g), bits(f)) for g, f in zip(s.read(), frames)), what    # nothing written
        assert A.stats_of(be.air_stats())["frames"] == 0                                        # nothing counted
        be.air_normalize(s.first, frame_stride=s.stride, n_frames=n, rows=rows)
        got = s.read()
        for k in range(n):
            want = A.subtract(frames[k], a[k], rows)
            if a[k] == 0:
                assert np.array_equal(bits(got[k]), bits(frames[k])), (what, k, "a frame that is not written")
            assert same_pixels(got[k], want), (what, k)
            if rows is not None:
                keep = ~np.isin(np.arange(dim_y), np.arange(rows[0], rows[0] + rows[1]))
                assert np.array_equal(bits(got[k])[keep], bits(frames[k])[keep]), (what, k, "rows outside the band")
        want_st = A.counts_of(whys, a) if rows is None or rows[1] != 0 else A.counts_of([], [])
        assert A.stats_of(be.air_stats()) == want_st, what
    finally:
        be.clear_air_region()
        s.free()
    return a, whys


def scan_for(rect, n, seed=8):
    """frame 0 and the even ones from 4 on: a drifting scan (a value of a few percent, which the subtraction shows in every pixel); the
    others: frames whose rectangle cancels (the order of the additions decides every bit of a tiny value) -- of which frame 1 has no
    finite pixel in the rectangle and NaN payloads outside it, and frame 2 a NaN with a payload, an inf and a -inf inside"""
    frames = A.cancelling_scan(A.DIM_X, A.DIM_Y, n, rect, seed)
    drifting = A.scan(A.DIM_X, A.DIM_Y, n, seed)
    for k in [0] + list(range(4, n, 2)):
        frames[k] = drifting[k]
    x0, y0, w, h = rect
    if n > 1:
        frames[1][y0:y0 + h, x0:x0 + w] = np.nan
        frames[1].view(np.uint32)[0, 0] = A.NAN_PAYLOAD
        frames[1].view(np.uint32)[A.DIM_Y - 1, A.DIM_X - 1] = A.NAN_PAYLOAD + 1
        frames[1].view(np.uint32)[y0, x0] = A.NAN_PAYLOAD + 2
    if n > 2 and w * h >= 8:
        frames[2] = A.awkward(frames[2], rect)
    return frames


def test_the_scan_holds_what_the_rule_has_clauses_for():
    rect = (3, 7, 64, 4)
    a, cnt, whys = A.values(scan_for(rect, 6), rect)
    assert whys[1] == "too_few" and a[1] == 0 and np.count_nonzero(a) == 5 and cnt[2] == 253 and 0 < abs(a[3]) < 1e-6 < abs(a[0])


@pytest.mark.parametrize("rect", A.RECTANGLES)
def test_rectangles_and_layouts(be, rect):
    frames = scan_for(rect, 4)
    for layout in LAYOUTS:
        a, whys = assert_measure_and_normalise(be, frames, rect, layout, what=(rect, layout), min_pixels=1)
        assert whys[1] == "too_few" and whys[0] == "normalised" and a[0] != 0


@pytest.mark.parametrize("n", [1, 3, 2 * _lib.AIR_FRAMES_MAX + 3])
def test_frames_per_call(be, n):
    """one call of n frames, also more than one launch pair serves: the values' slots are reused in stream order"""
    assert _lib.AIR_FRAMES_MAX == A.FRAMES_MAX
    rect = (1, 13, 65, 5)
    frames = scan_for(rect, n)
    for layout in ("padded", "odd"):
        a, whys = assert_measure_and_normalise(be, frames, rect, layout, what=(n, layout))
        assert np.count_nonzero(a) >= (n + 1) // 2 and whys.count("too_few") == (n > 1)


@pytest.mark.parametrize("dim_x", [96, 100, 261])
def test_vector_and_single_pixel_subtraction_over_more_than_one_block(be, dim_x):
    """96 and 100 columns take 16-byte vectors where pitch and stride allow, 261 and every odd pitch single pixels; 70 rows are
    6 to 72 blocks of 256 lanes"""
    rect = (dim_x - 9, 1, 8, 5)
    frames = A.scan(dim_x, 70, 3, seed=dim_x)
    for layout in LAYOUTS:
        assert_measure_and_normalise(be, frames, rect, layout, what=(dim_x, layout))


@pytest.mark.parametrize("dim_x", G.DIM_XS)
def test_a_band_past_the_grid_cap(be, dim_x):
    """1024 rows of 1025 pixels, or of 4100 in groups of four: 1 049 600 lanes against the subtraction's cap of 4096 blocks of 256,
    so four blocks come round again and split their lane index a second time, into the band's final row. Two frames a stride larger
    than the frame apart, a small rectangle in a corner; rows 0 .. 2 and 1027 .. 1029, the pitch padding and the gap keep their bits"""
    assert G.lanes(dim_x, dim_x % 4 == 0) > G.CAP_LANES
    rect = (dim_x - 9, 1, 8, 5)
    frames = A.scan(dim_x, G.DIM_Y, 2, seed=dim_x)
    a, cnt, whys = A.values(frames, rect)
    assert whys == ["normalised"] * 2 and (np.abs(a) > 1e-3).all() and a[0] != a[1]
    first, count = G.BAND
    s = G.Canvas(be, frames)
    be.set_air_region(*rect, dim_x, G.DIM_Y)
    try:
        got_a, got_n = be.air_measure(s.first, frame_stride=s.stride, n_frames=2)
        assert A.same_bits(got_a, a) and np.array_equal(got_n, cnt)
        be.air_normalize(s.first, frame_stride=s.stride, n_frames=2, rows=G.BAND)
        got = s.read()
        G.assert_canvas(s, got, s.expected([A.subtract(f, v, G.BAND)[first:first + count] for f, v in zip(frames, a)]), dim_x)
        for k in range(2):   # the second visit wrote
            tail_got, tail_was = G.second_visit(s, got, k), G.second_visit(s, s.before, k)
            assert np.count_nonzero(bits(tail_got) != bits(tail_was)) > 0.99 * tail_was.size
        assert A.stats_of(be.air_stats()) == A.counts_of(whys, a)
    finally:
        be.clear_air_region()
        s.free()


@pytest.mark.parametrize("rows,inside", [((0, 7), False), ((12, 8), False), ((5, 9), True), ((0, 20), True), ((6, 6), True),
                                         ((9, 1), True), ((20, 0), False), ((3, 0), False)])
def test_bands(be, rows, inside):
    """a band that holds the rectangle's rows (3 x 64 at rows 7 .. 10), one that does not, one row, no row: the value is the one of the
    frame as it was before the call, and only the band's rows change"""
    rect = (3, 7, 64, 4)
    assert inside == (rows[0] < rect[1] + rect[3] and rect[1] < rows[0] + rows[1])
    frames = scan_for(rect, 4)
    for layout in ("padded", "odd"):
        assert_measure_and_normalise(be, frames, rect, layout, rows=rows, what=(rows, layout))


@pytest.mark.parametrize("dim_x,dim_y", [(1, 1), (1, 7), (5, 1)])
def test_degenerate_frames(be, dim_x, dim_y):
    rng = np.random.default_rng(dim_x * 10 + dim_y)
    frames = [(2 + rng.normal(0, 1, (dim_y, dim_x))).astype(np.float32) for _ in range(3)]
    frames[1][:] = -0.0                                     # a_f = +0: not written, the zeros keep their sign
    for layout in LAYOUTS:
        for rect in ((0, 0, dim_x, dim_y), (dim_x - 1, dim_y - 1, 1, 1)):
            a, whys = assert_measure_and_normalise(be, frames, rect, layout, what=(dim_x, dim_y, layout, rect))
            assert whys == ["normalised"] * 3 and a[1] == 0 and a[0] != 0


def test_mask_too_few_and_above_limit_are_counted_and_reset(be):
    rect = (1, 0, 65, 3)                                    # a corner the scan's object never reaches
    frames = A.scan(A.DIM_X, A.DIM_Y, 6, seed=12)
    x0, y0, w, h = rect
    frames[2][y0:y0 + 2, x0:x0 + w] = np.inf                # 65 pixels left: too few for the default 98
    frames[4] += np.float32(0.5)                            # beyond the limit
    mask = A.random_mask(A.DIM_X, A.DIM_Y, 0.2)
    for m in (None, mask):
        a, whys = assert_measure_and_normalise(be, frames, rect, "padded", mask=m, limit_abs=0.25, what="mask" if m is not None else "no mask")
        assert whys == ["normalised", "normalised", "too_few", "normalised", "above_limit", "normalised"]
    assert not A.same_bits(A.values(frames, rect)[0], A.values(frames, rect, mask=mask)[0])     # the mask changes the values
    # the counters add up over calls and reset
    s = Stack(be, frames)
    be.set_air_region(*rect, A.DIM_X, A.DIM_Y, limit_abs=0.25)
    try:
        st = be.air_stats()
        assert (st.frames, st.normalised, st.min_a, st.max_a) == (0, 0, np.inf, -np.inf)
        be.air_normalize(s.first, frame_stride=s.stride, n_frames=6)
        be.air_normalize(s.frame(5), rows=(2, 3))
        st = be.air_stats(reset=True)
        assert (st.frames, st.normalised, st.too_few, st.above_limit) == (7, 5, 1, 1)
        a = A.values(frames, rect, limit_abs=0.25)[0]
        second = A.value(A.subtract(frames[5], a[5]), rect)[0]                                   # a second pass finds a value near 0
        assert abs(second) < 1e-6 and st.min_a == min(a[[0, 1, 3, 5]].min(), second) and st.max_a == max(a[[0, 1, 3, 5]].max(), second)
        st = be.air_stats()
        assert (st.frames, st.normalised, st.too_few, st.above_limit, st.min_a, st.max_a) == (0, 0, 0, 0, np.inf, -np.inf)
    finally:
        be.clear_air_region()
        s.free()


def test_replacement_and_clear_respect_queued_work():
    dim = 1024
    rng = np.random.default_rng(70)
    frames = [(rng.normal(0, 0.01, (dim, dim)) + 0.01 * (k + 1)).astype(np.float32) for k in range(5)]
    rect_a, rect_b = (0, 0, 64, 1024), (900, 10, 100, 50)
    for f in frames:
        f[10:60, 900:1000] += np.float32(0.25)              # the two rectangles see different values
    with B.Backend(0, synchronous=False) as abe:
        ds = [abe.make_projection_device(dim, dim) for _ in frames]
        for h, d in zip(frames, ds):
            abe.upload_raw(h, d)
        abe.set_air_region(*rect_a, dim, dim)
        for d in ds[:4]:
            abe.air_normalize(d)
        abe.set_air_region(*rect_b, dim, dim)                # the four passes above may still be queued: they keep the old setting
        abe.air_normalize(ds[4])
        st = abe.air_stats()
        assert (st.frames, st.normalised) == (1, 1)          # the new setting's counts
        abe.clear_air_region()
        for h, d in zip(frames[:4], ds):
            assert np.array_equal(bits(read(abe, d)), bits(A.normalised([h], rect_a)[0])), "before the replacement"
        assert np.array_equal(bits(read(abe, ds[4])), bits(A.normalised([frames[4]], rect_b)[0])), "after the replacement"
        assert not np.array_equal(bits(A.normalised([frames[4]], rect_a)[0]), bits(A.normalised([frames[4]], rect_b)[0]))
        with pytest.raises(B.ParisHipError):                 # cleared: the pass is refused
            abe.air_normalize(ds[4])
        abe.clear_air_region()                               # clearing nothing is fine
        for d in ds:
            abe.free(d)


def test_reserve_bytes_grow_and_shrink_again(be):
    before = be.projection_reserve_bytes(96, 80)
    small, large = B.air_region_check(0, 0, 8, 8, 96, 80)[1], B.air_region_check(0, 0, 96, 80, 96, 80)[1]
    assert 0 < small < large
    be.set_air_region(0, 0, 8, 8, 96, 80)
    assert be.projection_reserve_bytes(96, 80) == before + small
    be.set_air_region(0, 0, 96, 80, 96, 80, mask=np.zeros((80, 96), np.uint8))   # replaced: one setting's bytes, not both
    assert be.projection_reserve_bytes(96, 80) == before + large
    be.clear_air_region()
    assert be.projection_reserve_bytes(96, 80) == before


def test_refusals(be):
    L = _lib.load()
    INV = _lib.ERROR_INVALID_ARGUMENT
    d = be.make_projection_device(96, 80)
    other = be.make_projection_device(97, 80)
    st = _lib.AirCounts()
    a, n = np.zeros(2, np.float32), np.zeros(2, np.uint32)
    # without a setting
    for call in (be.air_normalize, be.air_measure):
        with pytest.raises(B.ParisHipError) as e:
            call(d)
        assert e.value.status == INV
    with pytest.raises(B.ParisHipError):
        be.air_stats()
    # a refused setting sets nothing
    for bad in ((0, 0, 0, 1), (90, 0, 7, 1), (0, 0, 1, 81)):
        with pytest.raises(B.ParisHipError) as e:
            be.set_air_region(*bad, 96, 80)
        assert e.value.status == INV
    with pytest.raises(B.ParisHipError):
        be.set_air_region(0, 0, 4, 4, 96, 80, limit_abs=float("nan"))
    with pytest.raises(ValueError):
        be.set_air_region(0, 0, 4, 4, 96, 80, mask=np.zeros((80, 95), np.uint8))
    assert L.paris_hip_set_air_region(be._ctx, None, None, 96, 80) == INV
    assert L.paris_hip_set_air_region(None, C.byref(_lib.AirRegion(0, 0, 4, 4, 0, 0.0)), None, 96, 80) == INV
    assert L.paris_hip_clear_air_region(None) == INV
    with pytest.raises(B.ParisHipError):
        be.air_normalize(d)
    be.set_air_region(80, 70, 16, 10, 96, 80)
    try:
        assert L.paris_hip_air_stats(be._ctx, None, 0) == INV
        for call in (be.air_normalize, be.air_measure):
            with pytest.raises(B.ParisHipError):
                call(other)                                                                       # other dimensions
            with pytest.raises(B.ParisHipError):
                call(B.Projection(d.ptr, 96, 79, pitch=d.pitch, on_device=True))
            with pytest.raises(B.ParisHipError):
                call(B.Projection(d.ptr, 96, 80, pitch=4 * 96 - 4, on_device=True))              # a bad pitch
            with pytest.raises(B.ParisHipError):
                call(B.Projection(d.ptr, 96, 80, pitch=d.pitch + 2, on_device=True))
        with pytest.raises(B.ParisHipError):
            be.air_normalize(d, rows=(70, 11))                                                    # a bad band
        with pytest.raises(B.ParisHipError):
            be.air_normalize(d, rows=(81, 0))
        fn = L.paris_hip_air_normalize_rows
        assert fn(be._ctx, d.ptr, d.pitch, d.pitch * 80 - 4, 2, 96, 80, 0, 80) == INV            # overlapping frames
        assert fn(be._ctx, d.ptr, d.pitch, d.pitch * 80 + 2, 2, 96, 80, 0, 80) == INV
        assert fn(be._ctx, None, d.pitch, 0, 1, 96, 80, 0, 80) == INV
        assert fn(None, d.ptr, d.pitch, 0, 1, 96, 80, 0, 80) == INV
        fn = L.paris_hip_air_measure
        assert fn(be._ctx, d.ptr, d.pitch, d.pitch * 80 - 4, 2, 96, 80, a.ctypes.data, n.ctypes.data) == INV
        assert fn(be._ctx, None, d.pitch, 0, 1, 96, 80, a.ctypes.data, n.ctypes.data) == INV
        assert fn(None, d.ptr, d.pitch, 0, 1, 96, 80, a.ctypes.data, n.ctypes.data) == INV
        assert L.paris_hip_air_stats(be._ctx, C.byref(st), 0) == _lib.SUCCESS and st.frames == 0  # a refused call counts nothing
    finally:
        be.clear_air_region()
    be.free(d)
    be.free(other)


# ---- ordering -------------------------------------------------------------------------------------------------------------------------

def test_a_held_back_weighting_is_flushed_first():
    det = B.DetectorGeometry(*ORD_GEO)
    frames = A.scan(96, 80, 2, seed=50)
    rect = (0, 0, 10, 10)

    def run(fusion):
        with B.Backend(0, synchronous=False) as abe:
            abe.set_stage_fusion(fusion)
            abe.set_air_region(*rect, 96, 80)
            d_p = B.load(abe, B.Projection(frames[0].copy(), 96, 80, idx=2))
            B.weight(abe, d_p, det)            # with fusion: held back until something touches the frame
            a = abe.air_measure(d_p)[0]
            weighted = read(abe, d_p)
            d_q = B.load(abe, B.Projection(frames[1].copy(), 96, 80, idx=3))
            B.weight(abe, d_q, det)
            abe.air_normalize(d_q)
            return weighted, a, read(abe, d_q)

    plain, fused = run(False), run(True)
    assert not np.array_equal(bits(plain[0]), bits(frames[0])) and A.same_bits(plain[1], A.values([plain[0]], rect)[0])
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(plain, fused))


@pytest.mark.parametrize("references", [False, True])
@pytest.mark.parametrize("what", ["measure", "normalize"])
def test_a_frame_of_the_pending_group_is_backprojected_as_it_was(references, what):
    """by reference: the group that refers to the frame is launched before the pass touches it, so the volume equals the snapshot
    path's; snapshots: it stays pending"""
    det = B.DetectorGeometry(*ORD_GEO)
    vg = B.calculate_volume_geometry(det)
    frames = A.scan(96, 80, 1, seed=51)
    rect = (0, 0, 10, 10)

    def run(deferred):
        with B.Backend(0, synchronous=False) as abe:
            if deferred:
                abe.set_backproject_deferral(8)
                abe.set_backproject_references(references)
            abe.set_air_region(*rect, 96, 80)
            v = abe.make_volume_device(vg.dim_x, vg.dim_y, vg.dim_z)
            d_p = B.load(abe, B.Projection(frames[0].copy(), 96, 80, idx=1))
            B.backproject(abe, d_p, v, 0, det, vg, False, False, None)
            if deferred:
                assert pending(abe) == 1
            if what == "measure":
                abe.air_measure(d_p)
            else:
                abe.air_normalize(d_p)
            if deferred:
                assert pending(abe) == (0 if references else 1)
            return read(abe, d_p), volume_to_host(abe, v, vg)

    want_p, want_v = run(False)
    got_p, got_v = run(True)
    assert np.abs(want_v).max() > 0 and np.array_equal(bits(want_p), bits(frames[0])) == (what == "measure")
    assert np.array_equal(bits(got_v), bits(want_v)) and np.array_equal(bits(got_p), bits(want_p))
    if what == "normalize":
        assert np.array_equal(bits(got_p), bits(A.normalised(frames, rect)[0]))
