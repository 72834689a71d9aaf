"""Metal artefact reduction on the device: paris_hip_metal_collect, _trace_pack, _inpaint_rows and _reinsert
against their host rules and the numpy restatement (tests/metal_rule.py), bit for bit -- the special rows, frames placed in canvases
with sentinel bytes around rows and frames, groups of frames with their views out of order, row bands, every kernel past its grid cap
-- the counts, the ordering contract of the frame passes, the refusals, the two settings' memory, and the physical check: the scene's
soft tissue after Backend.reduce_metal, the inpainted reconstruction and the reinsertion."""
import ctypes as C

import numpy as np
import pytest

import fdk_model
import metal_rule as R
from paris_amd import _lib
from paris_amd import backend as B

pytestmark = pytest.mark.gpu

INV = _lib.ERROR_INVALID_ARGUMENT
SENTINEL = np.uint32(0x7fc0beef)   # a NaN with a payload: never the result of an interpolation
bits = R.f32_bits


@pytest.fixture(scope="module")
def be():
    with B.Backend(0) as b:
        yield b


def read(be, d):
    h = be.make_projection_host(d.dim_x, d.dim_y)
    be.copy_d2h(d, h)
    return h.buf.copy()


def pending(be):
    n, ptr = C.c_uint32(0), C.c_void_p()
    assert be._L.paris_hip_pending_backprojections(be._ctx, C.byref(n), C.byref(ptr)) == 0
    return n.value


def volume_to_device(be, host):
    dz, dy, dx = host.shape
    v = be.make_volume_device(dx, dy, dz)
    be.copy_h2d(B.Volume(np.ascontiguousarray(host, np.float32), dx, dy, dz), v)
    return v


def volume_to_host(be, v):
    h = be.make_volume_host(v.dim_x, v.dim_y, v.dim_z)
    be.copy_d2h(v, h)
    return h.buf.copy()


class Canvas:
    """A stretch of device memory addressed as bytes: a pool buffer of 64-float rows (pitch 256 exactly), so its rows are contiguous.
    Frames live in it at any offset, pitch and stride; reading it back shows every byte, the ones between rows and frames included."""

    def __init__(self, be, frames, offset, pad, gap):
        self.be, self.n = be, len(frames)
        self.dim_y, self.dim_x = frames[0].shape
        self.offset, self.pitch = offset, 4 * self.dim_x + pad
        self.stride = self.pitch * self.dim_y + gap
        rows = (offset + self.n * self.stride + 256 + 255) // 256
        self.host = np.full(rows * 64, SENTINEL, np.uint32).view(np.float32)
        for k, f in enumerate(frames):
            self.place(self.host, k, f)
        self.d = be.make_projection_device(64, rows)
        assert self.d.pitch == 256
        be.upload_raw(self.host.reshape(rows, 64), self.d)
        self.first = be.wrap_projection(self.d.ptr + offset, self.pitch, self.dim_x, self.dim_y)

    def place(self, flat, k, frame, row_first=0):
        for y, row in enumerate(np.asarray(frame, np.float32)):
            at = (self.offset + k * self.stride + (row_first + y) * self.pitch) // 4
            flat[at:at + row.size] = row

    def expected(self, frames):
        want = self.host.copy()
        for k, f in enumerate(frames):
            self.place(want, k, f)
        return want

    def read(self):
        return read(self.be, self.d).reshape(-1)

    def free(self):
        self.be.free(self.d)


LAYOUTS = {"aligned": (0, 16, 32), "misaligned": (4, 4, 8), "wide": (12, 44, 1000)}   # (offset, row padding, gap between frames) in bytes


def same_canvas(got, want):
    """every bit, the sentinel's payload included; elsewhere a NaN may carry any payload"""
    keep = bits(want) == SENTINEL
    nan = np.isnan(want) & ~keep
    return (np.array_equal(bits(got)[keep], bits(want)[keep]) and np.array_equal(np.isnan(got) & ~keep, nan)
            and np.array_equal(bits(got)[~nan & ~keep], bits(want)[~nan & ~keep]))


# ---- 1. the inpainting, bit for bit ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("dim_x", R.DIM_XS)
def test_inpaint_matches_the_host_rule_on_the_special_rows(be, dim_x, layout):
    p, m = R.special_rows(dim_x)
    trace = R.pack_bits(m)
    want, host_counts = B.metal_inpaint_host(p, trace)
    assert R.same_pixels(want, R.inpaint(p, m)[0])
    be.set_metal_trace(trace[None], dim_x)
    try:
        c = Canvas(be, [p], *LAYOUTS[layout])
        be.metal_inpaint(c.first, view=0)
        assert same_canvas(c.read(), c.expected([want]))
        assert R.counts_tuple(be.metal_stats()) == R.counts_tuple(host_counts) == R.inpaint(p, m)[1]
        c.free()
    finally:
        be.clear_metal_trace()


def test_a_pool_buffer_with_padded_rows(be):
    p, m = R.special_rows(130)
    be.set_metal_trace(R.pack_bits(m)[None], 130)
    try:
        d = be.make_projection_device(130, p.shape[0])
        be.upload_raw(p, d)
        d.idx = 0
        be.metal_inpaint(d)                                                              # (view None: the projection's idx)
        assert R.same_pixels(read(be, d), B.metal_inpaint_host(p, R.pack_bits(m))[0])
        be.free(d)
    finally:
        be.clear_metal_trace()


@pytest.mark.parametrize("layout", ["aligned", "wide"])
def test_four_frames_with_views_out_of_order_and_repeated(be, layout):
    """the trace of frame f is the one h_view[f] names; the frame stride is larger than the frame; the counts add up over the frames"""
    rng = np.random.default_rng(4)
    dim_y, dim_x = 11, 130
    masks = rng.random((3, dim_y, dim_x)) < np.array([0.03, 0.3, 0.9])[:, None, None]
    masks[1, 4] = True                                                                   # a row covered whole
    masks[2, 5] = False
    frames = [rng.uniform(-1, 5, (dim_y, dim_x)).astype(np.float32) for _ in range(4)]
    views = [2, 0, 2, 1]
    be.set_metal_trace(R.pack_bits(masks), dim_x)
    try:
        c = Canvas(be, frames, *LAYOUTS[layout])
        be.metal_inpaint(c.first, view=views, frame_stride=c.stride, n_frames=4)
        want = [R.inpaint(f, masks[v]) for f, v in zip(frames, views)]
        assert same_canvas(c.read(), c.expected([w[0] for w in want]))
        assert R.counts_tuple(be.metal_stats(reset=True)) == tuple(sum(w[1][k] for w in want) for k in range(3))
        assert R.counts_tuple(be.metal_stats()) == (0, 0, 0)
        c.free()
    finally:
        be.clear_metal_trace()


@pytest.mark.parametrize("band", [(0, 3), (3, 5), (9, 2), (4, 0), (11, 0)])
def test_a_band_writes_its_rows_only(be, band):
    rng = np.random.default_rng(5)
    dim_y, dim_x = 11, 67
    masks = rng.random((2, dim_y, dim_x)) < 0.2
    frames = [rng.uniform(-1, 5, (dim_y, dim_x)).astype(np.float32) for _ in range(2)]
    be.set_metal_trace(R.pack_bits(masks), dim_x)
    try:
        c = Canvas(be, frames, *LAYOUTS["misaligned"])
        be.metal_inpaint(c.first, view=[1, 0], row_first=band[0], row_count=band[1], frame_stride=c.stride, n_frames=2)
        want = [R.inpaint(f, masks[v], *band) for f, v in zip(frames, (1, 0))]
        assert same_canvas(c.read(), c.expected([w[0] for w in want]))
        assert R.counts_tuple(be.metal_stats()) == tuple(sum(w[1][k] for w in want) for k in range(3))
        c.free()
    finally:
        be.clear_metal_trace()


def test_seventy_frames_in_two_launches(be):
    """a launch serves 64 frames: frames 64 .. 69 belong to a second one"""
    rng = np.random.default_rng(6)
    dim_y, dim_x = 5, 70
    masks = rng.random((70, dim_y, dim_x)) < 0.25
    frames = [rng.uniform(-1, 5, (dim_y, dim_x)).astype(np.float32) for _ in range(70)]
    views = list(range(69, -1, -1))
    be.set_metal_trace(R.pack_bits(masks), dim_x)
    try:
        c = Canvas(be, frames, *LAYOUTS["aligned"])
        be.metal_inpaint(c.first, view=views, frame_stride=c.stride, n_frames=70)
        assert same_canvas(c.read(), c.expected([R.inpaint(f, masks[v])[0] for f, v in zip(frames, views)]))
        c.free()
    finally:
        be.clear_metal_trace()


def test_rows_past_the_grid_cap(be):
    """pack and inpaint deal (frame, row, word) and (frame, row) tasks to at most 4096 blocks of 4 waves: 4 x 4100 rows of 5 pixels are
    16 400 tasks, the last 16 a second visit of the first blocks"""
    rng = np.random.default_rng(7)
    dim_y, dim_x = 4100, 5
    shadows = [np.where(rng.random((dim_y, dim_x)) < 0.15, np.float32(2.0), np.float32(0.0)).astype(np.float32) for _ in range(4)]
    frames = [rng.uniform(-1, 5, (dim_y, dim_x)).astype(np.float32) for _ in range(4)]
    c = Canvas(be, shadows, *LAYOUTS["misaligned"])
    got = be.metal_trace_pack(c.first, 1.0, 1, frame_stride=c.stride, n_frames=4)
    assert np.array_equal(c.read().view(np.uint32), c.host.view(np.uint32))              # the frames are only read
    c.free()
    want = R.pack(np.stack(shadows), 1.0, 1)
    assert np.array_equal(got, want) and want[3, -4:].any()
    be.set_metal_trace(got, dim_x)
    try:
        c = Canvas(be, frames, *LAYOUTS["misaligned"])
        be.metal_inpaint(c.first, view=[0, 1, 2, 3], frame_stride=c.stride, n_frames=4)
        masks = R.unpack_bits(got, dim_x)
        want = [R.inpaint(f, m) for f, m in zip(frames, masks)]
        assert want[3][1][0] > 0 and same_canvas(c.read(), c.expected([w[0] for w in want]))
        assert R.counts_tuple(be.metal_stats()) == tuple(sum(w[1][k] for w in want) for k in range(3))
        c.free()
    finally:
        be.clear_metal_trace()


# ---- 2. the trace ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("grow", (0, 1, 4))
@pytest.mark.parametrize("layout", ["aligned", "misaligned", "wide"])
@pytest.mark.parametrize("shape", ((9, 70), (1, 1), (3, 64), (12, 130)))
def test_pack_matches_the_host_rule(be, shape, layout, grow):
    t = R.corner_frames(shape[1], shape[0])
    want = B.metal_trace_pack_host(t, 1.0, grow)
    assert np.array_equal(want, R.pack(t, 1.0, grow))
    c = Canvas(be, list(t), *LAYOUTS[layout])
    got = be.metal_trace_pack(c.first, 1.0, grow, frame_stride=c.stride, n_frames=len(t))
    assert got.dtype == np.uint64 and np.array_equal(got, want)
    assert np.array_equal(c.read().view(np.uint32), c.host.view(np.uint32))
    c.free()


# ---- 3. the list -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("binarize", [False, True])
@pytest.mark.parametrize("shape", ((3, 5, 67), (9, 129, 130)))
def test_collect_matches_the_host_rule(be, shape, binarize):
    """hits cluster across every boundary between the 4096-voxel chunks one wave counts"""
    v = R.hit_volume(shape, 0.75)
    want_i, want_v, want_mask = B.metal_collect_host(v, 0.75, max_n=v.size, binarize=binarize)
    assert np.array_equal(want_i, R.collect(v, 0.75)[0]) and len(want_i) > 40
    d = volume_to_device(be, v)
    got_i, got_v = be.metal_collect(d, 0.75, max_n=v.size, binarize=binarize)
    assert np.array_equal(got_i, want_i) and np.array_equal(bits(got_v), bits(want_v))
    after = volume_to_host(be, d)
    assert np.array_equal(bits(after), bits(want_mask if binarize else v))                # binarize off: every bit as it was, NaN included
    be.free(d)


def test_collect_cap_and_empty_result(be):
    v = R.hit_volume((3, 5, 67), 0.75)
    n = len(R.collect(v, 0.75)[0])
    d = volume_to_device(be, v)
    with pytest.raises(B.ParisHipError) as e:
        be.metal_collect(d, 0.75, max_n=n - 1, binarize=True)
    assert e.value.status == _lib.ERROR_METAL_TOO_MANY_VOXELS and e.value.n == n
    assert np.array_equal(bits(volume_to_host(be, d)), bits(v))                           # nothing written
    index, value, count = np.full(n + 2, 77, np.uint64), np.full(n + 2, 77.0, np.float32), C.c_uint64(0)
    assert be._L.paris_hip_metal_collect(be._ctx, d.ptr, 67, 5, 3, 0.75, n - 1, index.ctypes.data, value.ctypes.data, C.byref(count), 0) \
        == _lib.ERROR_METAL_TOO_MANY_VOXELS
    assert count.value == n and (index == 77).all() and (value == 77.0).all()
    got_i, _ = be.metal_collect(d, 0.75, max_n=n)                                         # n == max_n
    assert len(got_i) == n
    got_i, got_v = be.metal_collect(d, 1e6)                                               # only +inf
    assert len(got_i) == 1 and np.isinf(got_v[0])
    got_i, got_v = be.metal_collect(d, 3e38, binarize=True)
    assert len(got_i) == 1
    got_i, got_v = be.metal_collect(d, 2.0)                                               # the mask holds nothing above 1
    assert len(got_i) == 0 and len(got_v) == 0
    count = C.c_uint64(0)
    L, ctx = be._L, be._ctx
    assert L.paris_hip_metal_collect(ctx, None, 67, 5, 3, 0.75, 0, None, None, C.byref(count), 0) == INV
    assert L.paris_hip_metal_collect(ctx, d.ptr, 67, 5, 3, 0.75, 0, None, None, None, 0) == INV
    assert L.paris_hip_metal_collect(ctx, d.ptr, 67, 0, 3, 0.75, 0, None, None, C.byref(count), 0) == INV
    assert L.paris_hip_metal_collect(ctx, d.ptr, 67, 5, 3, float("nan"), 0, None, None, C.byref(count), 0) == INV
    assert L.paris_hip_metal_collect(ctx, d.ptr, 67, 5, 3, 0.75, 4, None, None, C.byref(count), 0) == INV
    assert L.paris_hip_metal_collect(None, d.ptr, 67, 5, 3, 0.75, 0, None, None, C.byref(count), 0) == INV
    be.free(d)


def test_collect_past_the_count_kernel_s_grid_cap(be):
    """2048 blocks of 4 waves take 8192 chunks of 4096 voxels per visit: 8193 chunks and 5 voxels need a second visit and a ragged end"""
    n = 8193 * 4096 + 5
    rng = np.random.default_rng(8)
    v = rng.random(n, dtype=np.float32) * np.float32(0.5)
    where = np.concatenate((rng.choice(n, 3000, replace=False), np.arange(8192 * 4096 - 2, 8192 * 4096 + 3), np.arange(n - 7, n)))
    v[where] = np.float32(0.75) + rng.random(where.size, dtype=np.float32)
    v = v.reshape(1, 1, n)
    want_i, want_v = R.collect(v, 0.5)
    d = volume_to_device(be, v)
    got_i, got_v = be.metal_collect(d, 0.5, binarize=True)
    assert np.array_equal(got_i, want_i) and np.array_equal(bits(got_v), bits(want_v)) and got_i[-1] == n - 1
    assert np.array_equal(bits(volume_to_host(be, d)), bits(R.binarized(v, 0.5)))
    be.free(d)


# ---- 4. the reinsertion ---------------------------------------------------------------------------------------------------------------

def test_reinsert_writes_the_listed_voxels_of_the_slab_only(be):
    rng = np.random.default_rng(9)
    grid = (12, 9, 13)
    v = rng.random(grid, dtype=np.float32)
    index = np.sort(rng.choice(v.size, 200, replace=False)).astype(np.uint64)
    index[0], index[-1] = 0, v.size - 1
    value = rng.uniform(5, 6, 200).astype(np.float32)
    value[3] = np.float32(-0.0)
    be.set_metal_voxels(index, value)
    try:
        for first, count in ((0, 12), (0, 1), (3, 4), (11, 1), (5, 0)):
            d = volume_to_device(be, v[first:first + count]) if count else be.make_volume_device(13, 9, 1)
            if count:
                be.metal_reinsert(d, first)
                assert np.array_equal(bits(volume_to_host(be, d)), bits(R.reinsert(v[first:first + count], index, value, first)))
            else:
                assert be._L.paris_hip_metal_reinsert(be._ctx, d.ptr, 13, 9, 0, first) == _lib.SUCCESS
            be.free(d)
        d = volume_to_device(be, v)
        assert be._L.paris_hip_metal_reinsert(be._ctx, None, 13, 9, 12, 0) == INV
        assert be._L.paris_hip_metal_reinsert(be._ctx, d.ptr, 0, 9, 12, 0) == INV
        be.set_metal_voxels(np.zeros(0, np.uint64), np.zeros(0, np.float32))            # an empty list: nothing to write
        be.metal_reinsert(d)
        assert np.array_equal(bits(volume_to_host(be, d)), bits(v))
        be.clear_metal_voxels()
        with pytest.raises(B.ParisHipError) as e:
            be.metal_reinsert(d)
        assert e.value.status == INV
        be.free(d)
        for bad in ([3, 3], [4, 3]):
            with pytest.raises(B.ParisHipError) as e:
                be.set_metal_voxels(np.array(bad, np.uint64), np.zeros(2, np.float32))
            assert e.value.status == INV
    finally:
        be.clear_metal_voxels()


def test_reinsert_orders_itself_behind_deferred_backprojections():
    """the listed voxels hold the listed values although the slab's backprojections were still pending when the call was made"""
    det = B.DetectorGeometry(*R.SCENE_DET)
    vg = B.VolumeGeometry(*R.SCENE_GRID)
    frames = R.scene_frames(3.0)[:6]
    index = np.array([5, 64 * 64 * 12 + 64 * 32 + 32, 64 * 64 * 24 - 1], np.uint64)
    value = np.array([123.0, 456.0, 789.0], np.float32)

    def run(deferred):
        with B.Backend(0, synchronous=False) as abe:
            if deferred:
                abe.set_paris_loop_defaults(8)
            abe.set_metal_voxels(index, value)
            v = abe.make_volume_device(vg.dim_x, vg.dim_y, vg.dim_z)
            for i, f in enumerate(frames):
                d_p = B.load(abe, B.Projection(f.copy(), det.n_row, det.n_col, idx=i))
                B.weight(abe, d_p, det)
                B.filter(abe, d_p, det)
                B.backproject(abe, d_p, v, 0, det, vg, False, False, None)
                abe.free(d_p)
            if deferred:
                assert pending(abe) > 0
            abe.metal_reinsert(v)
            assert pending(abe) == 0
            return volume_to_host(abe, v)

    plain, deferred = run(False), run(True)
    assert np.array_equal(bits(plain), bits(deferred)) and plain.reshape(-1)[index.astype(np.int64)].tolist() == [123.0, 456.0, 789.0]
    assert np.count_nonzero(plain) > 1000


# ---- 5. ordering, refusals, settings ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("by_reference", [False, True])
def test_a_frame_of_the_pending_group_is_backprojected_as_it_was(by_reference):
    """by reference: the group that refers to the frame is launched before the inpainting writes it; snapshots: it stays pending"""
    det = B.DetectorGeometry(*R.SCENE_DET)
    vg = B.VolumeGeometry(*R.SCENE_GRID)
    frame = R.scene_frames(3.0)[7]
    mask = np.zeros(frame.shape, bool)
    mask[:, 20:41] = True

    def run(deferred):
        with B.Backend(0, synchronous=False) as abe:
            if deferred:
                abe.set_backproject_deferral(8)
                abe.set_backproject_references(by_reference)
            abe.set_metal_trace(R.pack_bits(mask)[None], det.n_row)
            d_p = B.load(abe, B.Projection(frame.copy(), det.n_row, det.n_col, idx=7))
            v = abe.make_volume_device(vg.dim_x, vg.dim_y, vg.dim_z)
            B.backproject(abe, d_p, v, 0, det, vg, False, False, None)
            if deferred:
                assert pending(abe) == 1
            abe.metal_inpaint(d_p, view=0)
            if deferred:
                assert pending(abe) == (0 if by_reference else 1)
            return read(abe, d_p), volume_to_host(abe, v)

    (want_p, want_v), (got_p, got_v) = run(False), run(True)
    assert np.abs(want_v).max() > 0 and R.same_pixels(want_p, R.inpaint(frame, mask)[0])
    assert np.array_equal(bits(got_v), bits(want_v)) and np.array_equal(bits(got_p), bits(want_p))


def test_a_held_back_weighting_is_flushed_first():
    det = B.DetectorGeometry(*R.SCENE_DET)
    frame = R.scene_frames(3.0)[3]
    mask = np.zeros(frame.shape, bool)
    mask[:, 20:41] = True

    def run(fusion):
        with B.Backend(0, synchronous=False) as abe:
            abe.set_stage_fusion(fusion)
            abe.set_metal_trace(R.pack_bits(mask)[None], det.n_row)
            d_p = B.load(abe, B.Projection(frame.copy(), det.n_row, det.n_col))
            B.weight(abe, d_p, det)                    # with fusion: held back until something touches the frame
            abe.metal_inpaint(d_p, view=0)
            return read(abe, d_p)

    plain, fused = run(False), run(True)
    assert np.array_equal(bits(plain), bits(fused)) and not np.array_equal(bits(plain), bits(R.inpaint(frame, mask)[0]))


def test_refusals(be):
    p, m = R.special_rows(65)
    rows = p.shape[0]
    d = be.make_projection_device(65, rows)
    be.upload_raw(p, d)
    with pytest.raises(B.ParisHipError) as e:
        be.metal_inpaint(d, view=0)                                                       # no setting
    assert e.value.status == INV
    with pytest.raises(B.ParisHipError) as e:
        be.metal_stats()
    assert e.value.status == INV
    L, ctx = be._L, be._ctx
    trace = R.pack_bits(np.stack([m, m]))
    assert L.paris_hip_set_metal_trace(ctx, None, 2, 65, rows) == INV
    assert L.paris_hip_set_metal_trace(ctx, trace.ctypes.data, 0, 65, rows) == INV
    assert L.paris_hip_set_metal_trace(ctx, trace.ctypes.data, 2, 0, rows) == INV
    assert L.paris_hip_set_metal_trace(ctx, trace.ctypes.data, 2, 65, 0) == INV
    assert L.paris_hip_set_metal_trace(None, trace.ctypes.data, 2, 65, rows) == INV
    be.set_metal_trace(trace, 65)
    try:
        view = (C.c_uint32 * 2)(1, 2)
        args = (d.ptr, d.pitch, 0, 1, 65, rows, 0, rows)
        assert L.paris_hip_metal_inpaint_rows(ctx, *args, view) == _lib.SUCCESS
        assert L.paris_hip_metal_inpaint_rows(ctx, *args, (C.c_uint32 * 1)(2)) == INV      # a view the setting does not hold
        assert L.paris_hip_metal_inpaint_rows(ctx, *args, None) == INV
        assert L.paris_hip_metal_inpaint_rows(ctx, d.ptr, d.pitch, 0, 1, 64, rows, 0, rows, view) == INV   # another frame size
        assert L.paris_hip_metal_inpaint_rows(ctx, d.ptr, d.pitch, 0, 1, 65, rows - 1, 0, rows - 1, view) == INV
        assert L.paris_hip_metal_inpaint_rows(ctx, d.ptr, d.pitch, 0, 1, 65, rows, 1, rows, view) == INV   # a band outside the frame
        assert L.paris_hip_metal_inpaint_rows(ctx, d.ptr, 4 * 64, 0, 1, 65, rows, 0, rows, view) == INV    # a pitch below the row
        assert L.paris_hip_metal_inpaint_rows(ctx, d.ptr, d.pitch, d.pitch, 2, 65, rows, 0, rows, view) == INV   # frames that overlap
        assert L.paris_hip_metal_inpaint_rows(ctx, None, d.pitch, 0, 1, 65, rows, 0, rows, view) == INV
        assert L.paris_hip_metal_stats(ctx, None, 0) == INV
        out = np.zeros((1, rows, 2), np.uint64)
        pack = (d.ptr, d.pitch, 0, 1, 65, rows)
        assert L.paris_hip_metal_trace_pack(ctx, *pack, 0.5, 5, out.ctypes.data) == INV
        assert L.paris_hip_metal_trace_pack(ctx, *pack, -0.5, 0, out.ctypes.data) == INV
        assert L.paris_hip_metal_trace_pack(ctx, *pack, float("nan"), 0, out.ctypes.data) == INV
        assert L.paris_hip_metal_trace_pack(ctx, *pack, 0.5, 0, None) == INV
        assert L.paris_hip_metal_trace_pack(ctx, None, d.pitch, 0, 1, 65, rows, 0.5, 0, out.ctypes.data) == INV
        assert L.paris_hip_metal_trace_pack(ctx, *pack, 0.5, 0, out.ctypes.data) == _lib.SUCCESS
        be.clear_metal_trace()
        with pytest.raises(B.ParisHipError) as e:
            be.metal_inpaint(d, view=0)                                                   # after clearing, as without a setting
        assert e.value.status == INV
    finally:
        be.clear_metal_trace()
        be.free(d)


def test_the_settings_count_towards_the_reserve_and_are_retired():
    with B.Backend(0, synchronous=False) as abe:
        base = abe.projection_reserve_bytes(64, 32)
        trace = np.zeros((120, 32, 1), np.uint64)
        abe.set_metal_trace(trace, 64)
        size = R.COUNTER_BYTES + trace.nbytes
        assert size == _lib.METAL_COUNTER_BYTES + 120 * 32 * 8 and abe.projection_reserve_bytes(64, 32) == base + size
        abe.set_metal_trace(np.zeros((7, 32, 3), np.uint64), 130)                        # replaced: the old one no longer counts
        assert abe.projection_reserve_bytes(64, 32) == base + R.COUNTER_BYTES + 7 * 32 * 3 * 8
        abe.set_metal_voxels(np.arange(1000, dtype=np.uint64), np.zeros(1000, np.float32))
        assert abe.projection_reserve_bytes(64, 32) == base + R.COUNTER_BYTES + 7 * 32 * 3 * 8 + 12 * 1000
        abe.set_metal_voxels(np.arange(10, dtype=np.uint64), np.zeros(10, np.float32))
        assert abe.projection_reserve_bytes(64, 32) == base + R.COUNTER_BYTES + 7 * 32 * 3 * 8 + 12 * 10
        abe.clear_metal_trace()
        assert abe.projection_reserve_bytes(64, 32) == base + 12 * 10
        abe.clear_metal_voxels()
        assert abe.projection_reserve_bytes(64, 32) == base
        abe.clear_metal_trace()                                                          # clearing nothing is no error
        abe.clear_metal_voxels()
        abe.set_metal_trace(trace, 64)                                                   # left set: the ctx's destruction frees them
        abe.set_metal_voxels(np.arange(10, dtype=np.uint64), np.zeros(10, np.float32))


def test_a_replaced_trace_serves_the_work_queued_before():
    """asynchronous: the inpainting queued with the first trace uses it although the second is installed before it has run"""
    rng = np.random.default_rng(11)
    dim_y, dim_x = 9, 130
    m1, m2 = rng.random((1, dim_y, dim_x)) < 0.2, rng.random((1, dim_y, dim_x)) < 0.2
    frame = rng.uniform(-1, 5, (dim_y, dim_x)).astype(np.float32)
    with B.Backend(0, synchronous=False) as abe:
        a, b = abe.make_projection_device(dim_x, dim_y), abe.make_projection_device(dim_x, dim_y)
        abe.upload_raw(frame, a)
        abe.upload_raw(frame, b)
        abe.set_metal_trace(R.pack_bits(m1), dim_x)
        abe.metal_inpaint(a, view=0)
        abe.set_metal_trace(R.pack_bits(m2), dim_x)
        abe.metal_inpaint(b, view=0)
        assert R.same_pixels(read(abe, a), R.inpaint(frame, m1[0])[0]) and R.same_pixels(read(abe, b), R.inpaint(frame, m2[0])[0])
        assert R.counts_tuple(abe.metal_stats()) == R.inpaint(frame, m2[0])[1]           # the counts are the new setting's


# ---- 6. the physical check ------------------------------------------------------------------------------------------------------------

def test_the_remedy_restores_the_scene_s_soft_tissue(be):
    """Backend.reduce_metal on the scene's clipped frames, then the inpainted reconstruction with the reinsertion: the soft-tissue RMS
    error against phantom.density falls to at most 0.25 of what it was (tests/test_metal_host.py pins the float64 model at 0.068; the
    device gave 0.068 as well), and the collected voxels hold exactly the first reconstruction's bits."""
    det, vg = B.DetectorGeometry(*R.SCENE_DET), B.VolumeGeometry(*R.SCENE_GRID)
    clip, density_threshold = R.SCENE_CASES[0]
    scale = fdk_model.scale(det, R.SCENE_VIEWS)
    threshold = float(np.float32(density_threshold * scale))                             # in the volume's own units
    full, frames = R.scene_frames(), R.scene_frames(clip)

    def reconstruct(inpaint):
        v = be.make_volume_device(vg.dim_x, vg.dim_y, vg.dim_z)
        be.memset_volume(v)
        for i, f in enumerate(frames):
            d_p = B.load(be, B.Projection(f.copy(), det.n_row, det.n_col, idx=i))
            if inpaint:
                be.metal_inpaint(d_p)
            B.weight(be, d_p, det)
            B.filter(be, d_p, det)
            B.backproject(be, d_p, v, 0, det, vg, False, False, None)
            be.free(d_p)
        if inpaint:
            be.metal_reinsert(v)
        out = volume_to_host(be, v)
        be.free(v)
        return out

    first = reconstruct(False)
    try:
        mt = be.reduce_metal(list(frames), det, threshold, grow=R.SCENE_GROW, min_path=R.SCENE_MIN_PATH, vol_geo=vg)
        want_i, want_v = R.collect(first, threshold)
        assert np.array_equal(mt.index, want_i) and np.array_equal(bits(mt.value), bits(want_v)) and len(want_i) > 100
        tr = R.unpack_bits(mt.bits, det.n_row)
        assert tr.shape == full.shape and tr[full > clip].all() and mt.trace_pixels == int(tr.sum())
        assert mt.min_path == R.SCENE_MIN_PATH and mt.grow == R.SCENE_GROW
        final = reconstruct(True)
        counts = be.metal_stats()
        assert counts.replaced == mt.trace_pixels and counts.rows_left == 0 and counts.runs > 0
    finally:
        be.clear_metal_trace()
        be.clear_metal_voxels()
    assert np.array_equal(bits(final.reshape(-1)[want_i.astype(np.int64)]), bits(want_v))
    truth = R.scene_truth(vg)
    soft = R.soft_tissue(truth, want_i)
    before, after = R.rms_error(first / scale, truth, soft), R.rms_error(final / scale, truth, soft)
    print("soft-tissue rms %.5f -> %.5f, ratio %.4f; %d voxels, %d trace pixels" % (before, after, after / before, len(want_i), mt.trace_pixels))
    assert soft.sum() > 20000 and after <= R.SCENE_BOUND * before


def test_reduce_metal_default_min_path_and_refusals(be):
    det, vg = B.DetectorGeometry(*R.SCENE_DET), B.VolumeGeometry(*R.SCENE_GRID)
    frames = list(R.scene_frames(3.0)[::10])
    for kw in (dict(threshold=float("nan")), dict(threshold=1.0, grow=5), dict(threshold=1.0, min_path=-1.0)):
        with pytest.raises(B.ParisHipError) as e:
            be.reduce_metal(frames, det, vol_geo=vg, **kw)
        assert e.value.status == INV
    with pytest.raises(B.ParisHipError) as e:                                            # a threshold that marks half the grid
        be.reduce_metal(frames, det, -1e30, vol_geo=vg)
    assert e.value.status == _lib.ERROR_METAL_TOO_MANY_VOXELS and e.value.n == 64 * 64 * 24
    try:
        mt = be.reduce_metal(frames, det, 1e30, vol_geo=vg)                              # nothing above it: an empty trace
        assert mt.min_path == 0.25 and len(mt.index) == 0 and mt.trace_pixels == 0 and not mt.bits.any()
    finally:
        be.clear_metal_trace()
        be.clear_metal_voxels()
