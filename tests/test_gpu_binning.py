"""Detector binning on the device: paris_hip_bin_frames against the numpy restatement of the rule
(tests/binning_rule.py), bit for bit -- every setting, with and without a mask, the 16-byte and the single-pixel path, frame strides,
row bands, the chain into the flat-field correction and the defect repair, the refusals and the ordering contract of the frame passes."""
import ctypes as C

import numpy as np
import pytest

import binning_rule as R
import defect_rule as DR
import test_gpu_defect_map as DM
import test_gpu_flat_field as FF
from paris_amd import _lib
from paris_amd import backend as B

pytestmark = pytest.mark.gpu

bits, read, pending = DM.bits, DM.read, DM.pending
each_setting = pytest.mark.parametrize("bin_x,bin_y", R.SETTINGS)
SENTINEL = np.uint32(0x7fc0beef)   # a NaN with a payload: never the result of an addition or a division


def small_mask():
    m = np.zeros((8, 8), np.uint8)
    m[0:4, 0:4] = 1
    m[5, 6] = 1
    m[:, 7] = 7
    return m


# (u16 counts, order-sensitive f32 frame, mask) per frame size (dim_x, dim_y)
FRAMES = {
    (67, 45): (R.counts_frame(), R.ordered_frame(), R.shared_mask()),
    (8, 8): (R.counts_frame(8, 8, 3), R.ordered_frame(8, 8, 4, special=False), small_mask()),
}


@pytest.fixture(scope="module")
def be():
    with B.Backend(0) as b:
        yield b


class Canvas:
    """A stretch of device memory addressed as bytes: a pool buffer of 64-float rows (pitch 256 exactly), so its rows are contiguous.
    Frames live in it at any offset and pitch; reading it back shows every byte, the ones between rows and frames included."""

    def __init__(self, be, n_bytes, host=None):
        rows = (n_bytes + 255) // 256
        self.be, self.d = be, be.make_projection_device(64, rows)
        assert self.d.pitch == 256
        self.host = np.full(rows * 64, SENTINEL, np.uint32).view(np.float32) if host is None else host
        be.upload_raw(self.host.reshape(rows, 64), self.d)

    def view(self, offset, pitch, dim_x, dim_y):
        return self.be.wrap_projection(self.d.ptr + offset, pitch, dim_x, dim_y)

    def read(self):
        return read(self.be, self.d).reshape(-1)

    def free(self):
        self.be.free(self.d)


def place(flat, offset, pitch, frame):
    """the host model of a frame in a canvas"""
    for y, row in enumerate(np.asarray(frame, np.float32)):
        at = (offset + y * pitch) // 4
        flat[at:at + row.size] = row


def layout(n_frames, dim_x, dim_y, offset, pad, gap):
    """(offset, pitch, stride, bytes) of n_frames frames with rows padded by `pad` bytes and frames `gap` bytes apart"""
    pitch = 4 * dim_x + pad
    stride = pitch * dim_y + gap
    return offset, pitch, stride, offset + n_frames * stride + 256


def run_in_canvases(be, frames, bin_x, bin_y, src_layout, dst_layout, row_first=0, row_count=None):
    """uploads the f32 frames into a source canvas, bins them into a sentinel-filled destination canvas, returns (got, want) -- the
    destination canvas as read back and as the rule says it must be, every byte"""
    n = len(frames)
    dim_y, dim_x = frames[0].shape
    ox, oy = R.binned_size(bin_x, bin_y, dim_x, dim_y)
    s_off, s_pitch, s_stride, s_bytes = src_layout(n, dim_x, dim_y)
    d_off, d_pitch, d_stride, d_bytes = dst_layout(n, ox, oy)
    host = np.full(((s_bytes + 255) // 256) * 64, SENTINEL, np.uint32).view(np.float32)
    for k, f in enumerate(frames):
        place(host, s_off + k * s_stride, s_pitch, f)
    src, dst = Canvas(be, s_bytes, host), Canvas(be, d_bytes)
    count = oy - row_first if row_count is None else row_count
    be.bin_frames(src.view(s_off, s_pitch, dim_x, dim_y), dst.view(d_off, d_pitch, ox, oy), row_first=row_first, row_count=count,
                  src_frame_stride=s_stride if n > 1 else 0, dst_frame_stride=d_stride if n > 1 else 0, n_frames=n)
    got = dst.read()
    assert np.array_equal(src.read().view(np.uint32), host.view(np.uint32))   # the source is only read
    src.free()
    dst.free()
    return got, (d_off, d_pitch, d_stride)


def expected_canvas(got, where, binned, row_first=0, row_count=None):
    d_off, d_pitch, d_stride = where
    want = np.full(got.size, SENTINEL, np.uint32).view(np.float32)
    for k, b in enumerate(binned):
        rows = slice(row_first, b.shape[0] if row_count is None else row_first + row_count)
        place(want, d_off + k * d_stride + rows.start * d_pitch, d_pitch, b[rows])
    return want


ALIGNED = lambda n, x, y: layout(n, x, y, 0, (-4 * x) % 16 + 16, 32)      # bases, pitches and strides multiples of 16: the vector path
SCALAR = lambda n, x, y: layout(n, x, y, 4, 4, 8)                        # base offset by 4 bytes, pitch 4 * dim_x + 4: single pixels


# ---- 1. the rule, every setting ---------------------------------------------------------------------------------------------------

@each_setting
@pytest.mark.parametrize("masked", [False, True])
def test_pool_buffers_take_the_vector_path_bit_for_bit(be, bin_x, bin_y, masked):
    """buffers of make_projection_device (rows padded to 256 bytes): u16 counts through upload_raw, and the order-sensitive f32 frame"""
    for (dim_x, dim_y), (counts, ordered, mask) in FRAMES.items():
        m = mask if masked else None
        ox, oy = be.set_binning(bin_x, bin_y, dim_x, dim_y, m)
        try:
            for h in (counts, ordered):
                src, dst = be.make_projection_device(dim_x, dim_y), be.make_projection_device(ox, oy)
                assert src.pitch % 256 == 0 and dst.pitch % 256 == 0
                be.upload_raw(h, src)
                be.bin_frames(src, dst)
                want = R.bin_frame(h.astype(np.float32), bin_x, bin_y, m)
                assert np.array_equal(bits(read(be, dst)), bits(want)), (dim_x, h.dtype)
                assert np.array_equal(bits(read(be, src)), bits(h.astype(np.float32)))
                be.free(src)
                be.free(dst)
        finally:
            be.clear_binning()


@each_setting
@pytest.mark.parametrize("masked", [False, True])
def test_an_offset_base_and_an_odd_pitch_take_the_scalar_path_bit_for_bit(be, bin_x, bin_y, masked):
    """a wrap_projection view whose base is offset by 4 bytes and whose pitch is 4 * dim_x + 4, on both sides"""
    for (dim_x, dim_y), (counts, ordered, mask) in FRAMES.items():
        m = mask if masked else None
        be.set_binning(bin_x, bin_y, dim_x, dim_y, m)
        try:
            got, where = run_in_canvases(be, [ordered], bin_x, bin_y, SCALAR, SCALAR)
            want = expected_canvas(got, where, [R.bin_frame(ordered, bin_x, bin_y, m)])
            assert np.array_equal(bits(got), bits(want)), dim_x
        finally:
            be.clear_binning()


@pytest.mark.parametrize("bin_x,bin_y", [(1, 2), (2, 2), (4, 1), (8, 1)])
@pytest.mark.parametrize("dim_x", [2100, 2101])
def test_rows_wider_than_one_block_of_lanes(be, bin_x, bin_y, dim_x):
    """more than 256 segments per row: several blocks along x, the last one partly filled; with the mask read as words (2100) and as
    bytes (2101)"""
    rng = np.random.default_rng(dim_x)
    frame = R.ordered_frame(dim_x, 6, 6, special=False)
    mask = (rng.random((6, dim_x)) < 0.3).astype(np.uint8)
    ox, oy = be.set_binning(bin_x, bin_y, dim_x, 6, mask)
    try:
        src, dst = be.make_projection_device(dim_x, 6), be.make_projection_device(ox, oy)
        be.upload_raw(frame, src)
        be.bin_frames(src, dst)
        assert np.array_equal(bits(read(be, dst)), bits(R.bin_frame(frame, bin_x, bin_y, mask)))
        be.free(src)
        be.free(dst)
    finally:
        be.clear_binning()


# ---- 2. strides and bands ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bin_x,bin_y", [(1, 1), (2, 2), (4, 2), (8, 4), (2, 8)])
@pytest.mark.parametrize("path", ["vector", "scalar"])
@pytest.mark.parametrize("masked", [False, True])
def test_three_frames_with_strides_larger_than_the_frames_leave_the_gaps_alone(be, bin_x, bin_y, path, masked):
    """the destination bytes between rows and between frames keep their sentinel"""
    counts, ordered, mask = FRAMES[(67, 45)]
    rng = np.random.default_rng(12)
    frames = [ordered, counts.astype(np.float32), (ordered * rng.uniform(0.5, 2.0, ordered.shape)).astype(np.float32)]
    m = mask if masked else None
    be.set_binning(bin_x, bin_y, 67, 45, m)
    try:
        lay = ALIGNED if path == "vector" else SCALAR
        got, where = run_in_canvases(be, frames, bin_x, bin_y, lay, lay)
        want = expected_canvas(got, where, [R.bin_frame(f, bin_x, bin_y, m) for f in frames])
        assert np.array_equal(bits(got), bits(want))
        assert np.count_nonzero(bits(got) == SENTINEL) > 3 * 8   # (there are gaps to leave alone)
    finally:
        be.clear_binning()


@pytest.mark.parametrize("bin_x,bin_y", [(1, 1), (2, 2), (1, 4), (4, 8)])
@pytest.mark.parametrize("path", ["vector", "scalar"])
def test_a_band_writes_its_rows_only_and_reads_their_source_rows_only(be, bin_x, bin_y, path):
    """binned rows [r0, r0 + n) equal the whole-frame result while every other source row holds NaN, and no other row is written"""
    counts, ordered, mask = FRAMES[(67, 45)]
    ordered = R.ordered_frame(special=False)
    oy = 45 // bin_y
    whole = R.bin_frame(ordered, bin_x, bin_y, mask)
    be.set_binning(bin_x, bin_y, 67, 45, mask)
    try:
        lay = ALIGNED if path == "vector" else SCALAR
        for r0, n in ((0, oy), (1, min(3, oy - 1)), (oy - 1, 1), (oy, 0), (oy // 2, 0)):
            poisoned = np.full_like(ordered, np.nan)
            poisoned[bin_y * r0:bin_y * (r0 + n)] = ordered[bin_y * r0:bin_y * (r0 + n)]
            got, where = run_in_canvases(be, [poisoned, poisoned], bin_x, bin_y, lay, lay, row_first=r0, row_count=n)
            want = expected_canvas(got, where, [whole, whole], row_first=r0, row_count=n)
            assert np.array_equal(bits(got), bits(want)), (r0, n)
            assert not np.isnan(whole[r0:r0 + n]).any()
    finally:
        be.clear_binning()


# ---- 3. the chain: upload -> bin -> correct -> repair -----------------------------------------------------------------------------

@pytest.mark.parametrize("bin_x,bin_y", [(2, 2), (4, 2), (8, 8), (1, 1)])
def test_the_chain_into_the_correction_and_the_repair(be, bin_x, bin_y):
    """upload_raw of u16 counts, bin_frames, flat_field_rows against host-binned references, defect_repair_rows with the binned mask:
    the numpy restatement of the whole chain, bit for bit"""
    dim_x, dim_y, t_min = 67, 45, 1e-5
    mask = R.shared_mask()
    dark, flat = FF.references(dim_y, dim_x, 21, 65535.0)
    counts = FF.counts(np.uint16, dark, flat, 22, t_min)
    dark_b, flat_b = B.bin_frame_host(bin_x, bin_y, dark, mask), B.bin_frame_host(bin_x, bin_y, flat, mask)
    assert np.array_equal(bits(dark_b), bits(R.bin_frame(dark, bin_x, bin_y, mask)))
    assert np.array_equal(bits(flat_b), bits(R.bin_frame(flat, bin_x, bin_y, mask)))
    mask_b = B.bin_mask(bin_x, bin_y, mask)
    assert np.array_equal(mask_b, R.bin_mask(mask, bin_x, bin_y)) and mask_b.any()
    # the restatement: the binning rule, the flat-field contract in float64 rounded once, the repair's fmaf chain over the plan
    binned = R.bin_frame(counts.astype(np.float32), bin_x, bin_y, mask)
    corrected = FF.expected(binned, dark_b, flat_b, t_min)
    plan = B.defect_plan(mask_b)
    defect, first, source = DR.restate(mask_b)[:3]
    assert np.array_equal(plan.defect, defect) and np.array_equal(plan.first_source, first) and np.array_equal(plan.source, source)
    want = R.repair32(corrected, plan)
    assert plan.defect.size > 0 and not np.array_equal(bits(want), bits(corrected))

    ox, oy = be.set_binning(bin_x, bin_y, dim_x, dim_y, mask)
    be.set_flat_field(dark_b, flat_b, t_min)
    be.set_defect_map(mask_b)
    try:
        src, dst = be.make_projection_device(dim_x, dim_y), be.make_projection_device(ox, oy)
        be.upload_raw(counts, src)
        be.bin_frames(src, dst)
        assert np.array_equal(bits(read(be, dst)), bits(binned))
        be.flat_field_rows(dst)
        assert np.array_equal(bits(read(be, dst)), bits(corrected))
        be.defect_repair_rows(dst)
        assert np.array_equal(bits(read(be, dst)), bits(want))
        be.free(src)
        be.free(dst)
    finally:
        be.clear_defect_map()
        be.clear_flat_field()
        be.clear_binning()


# ---- 4. refusals and the setting's lifecycle --------------------------------------------------------------------------------------

def test_refusals(be):
    L = _lib.load()
    src, dst = be.make_projection_device(67, 45), be.make_projection_device(33, 22)
    filled = np.full((22, 33), SENTINEL, np.uint32).view(np.float32)
    be.upload_raw(filled, dst)

    def raw(s=src, d=dst, s_pitch=None, d_pitch=None, s_stride=0, d_stride=0, n=1, dim_x=67, dim_y=45, row_first=0, row_count=22):
        return L.paris_hip_bin_frames(be._ctx, s if s is None or isinstance(s, int) else s.ptr, src.pitch if s_pitch is None else s_pitch,
                                      s_stride, d if d is None or isinstance(d, int) else d.ptr, dst.pitch if d_pitch is None else d_pitch,
                                      d_stride, n, dim_x, dim_y, row_first, row_count)

    assert raw() == _lib.ERROR_INVALID_ARGUMENT                                        # no setting
    bad = _lib.Binning(3, 2)
    assert L.paris_hip_set_binning(be._ctx, C.byref(bad), None, 67, 45) == _lib.ERROR_INVALID_ARGUMENT
    assert L.paris_hip_set_binning(be._ctx, None, None, 67, 45) == _lib.ERROR_INVALID_ARGUMENT
    assert L.paris_hip_set_binning(be._ctx, C.byref(_lib.Binning(8, 8)), None, 7, 45) == _lib.ERROR_INVALID_ARGUMENT
    assert L.paris_hip_set_binning(None, C.byref(_lib.Binning(2, 2)), None, 67, 45) == _lib.ERROR_INVALID_ARGUMENT
    with pytest.raises(ValueError):
        be.set_binning(2, 2, 67, 45, np.zeros((45, 66), np.uint8))
    be.clear_binning()                                                                 # clearing nothing is fine
    assert be.set_binning(2, 2, 67, 45) == (33, 22)
    try:
        assert raw(dim_x=66) == _lib.ERROR_INVALID_ARGUMENT                            # other dimensions than the setting's
        assert raw(dim_y=44) == _lib.ERROR_INVALID_ARGUMENT
        assert raw(row_first=20, row_count=3) == _lib.ERROR_INVALID_ARGUMENT           # a band beyond out_y
        assert raw(row_first=23, row_count=0) == _lib.ERROR_INVALID_ARGUMENT
        assert raw(row_first=2 ** 31, row_count=2 ** 31) == _lib.ERROR_INVALID_ARGUMENT
        assert raw(s=None) == _lib.ERROR_INVALID_ARGUMENT and raw(d=None) == _lib.ERROR_INVALID_ARGUMENT
        assert raw(s_pitch=4 * 67 - 4) == _lib.ERROR_INVALID_ARGUMENT                  # the argument rule, either side
        assert raw(s_pitch=src.pitch + 2) == _lib.ERROR_INVALID_ARGUMENT
        assert raw(d_pitch=4 * 33 - 4) == _lib.ERROR_INVALID_ARGUMENT
        assert raw(d_pitch=dst.pitch + 2) == _lib.ERROR_INVALID_ARGUMENT
        assert raw(n=2, s_stride=src.pitch * 45 - 4, d_stride=dst.pitch * 22) == _lib.ERROR_INVALID_ARGUMENT
        assert raw(n=2, s_stride=src.pitch * 45, d_stride=dst.pitch * 22 - 4) == _lib.ERROR_INVALID_ARGUMENT
        assert raw(n=2, s_stride=src.pitch * 45 + 2, d_stride=dst.pitch * 22) == _lib.ERROR_INVALID_ARGUMENT
        # overlapping source and destination: the same buffer, and a destination that starts inside the source's last row
        assert raw(d=src.ptr, d_pitch=src.pitch) == _lib.ERROR_INVALID_ARGUMENT
        assert raw(d=src.ptr + 44 * src.pitch + 4 * 60, d_pitch=src.pitch) == _lib.ERROR_INVALID_ARGUMENT
        assert raw(s=dst.ptr + 4, s_pitch=src.pitch) == _lib.ERROR_INVALID_ARGUMENT
        assert np.array_equal(bits(read(be, dst)), bits(filled))                       # no refused call wrote anything
        assert raw(row_first=22, row_count=0) == _lib.SUCCESS and raw(n=0) == _lib.SUCCESS   # empty calls
        assert np.array_equal(bits(read(be, dst)), bits(filled))
        assert raw() == _lib.SUCCESS
        assert not np.array_equal(bits(read(be, dst)), bits(filled))
    finally:
        be.clear_binning()
    assert raw() == _lib.ERROR_INVALID_ARGUMENT                                        # cleared
    be.free(src)
    be.free(dst)


def test_reserve_bytes_grow_by_the_mask_and_shrink_again(be):
    before = be.projection_reserve_bytes(67, 45)
    be.set_binning(2, 2, 67, 45)
    assert be.projection_reserve_bytes(67, 45) == before            # no mask: nothing on the device
    be.set_binning(2, 2, 67, 45, R.shared_mask())
    assert be.projection_reserve_bytes(67, 45) == before + 67 * 45
    be.set_binning(4, 4, 8, 8, small_mask())                        # replaced
    assert be.projection_reserve_bytes(67, 45) == before + 64
    be.clear_binning()
    assert be.projection_reserve_bytes(67, 45) == before


def test_a_replaced_mask_serves_the_work_queued_before():
    """asynchronous ctx: the call queued with mask A uses mask A although mask B replaces it right away, and destroy frees both"""
    dim = 1024
    rng = np.random.default_rng(3)
    frame = R.ordered_frame(dim, dim, 8, special=False)
    mask_a, mask_b = (rng.random((dim, dim)) < 0.3).astype(np.uint8), (rng.random((dim, dim)) < 0.3).astype(np.uint8)
    with B.Backend(0, synchronous=False) as abe:
        src, a, b = abe.make_projection_device(dim, dim), abe.make_projection_device(dim // 2, dim // 2), abe.make_projection_device(dim // 2, dim // 2)
        abe.upload_raw(frame, src)
        abe.set_binning(2, 2, dim, dim, mask_a)
        abe.bin_frames(src, a)
        abe.set_binning(2, 2, dim, dim, mask_b)
        abe.bin_frames(src, b)
        abe.clear_binning()
        got_a, got_b = read(abe, a), read(abe, b)
    assert np.array_equal(bits(got_a), bits(R.bin_frame(frame, 2, 2, mask_a)))
    assert np.array_equal(bits(got_b), bits(R.bin_frame(frame, 2, 2, mask_b)))


# ---- 5. ordering (the contract of tests/test_gpu_frame_passes.py) -----------------------------------------------------------------

ORD_X, ORD_Y = DM.ORD_GEO[:2]                      # the binned frame is the one the backprojection geometry describes
ORD_SRC = R.ordered_frame(2 * ORD_X, 2 * ORD_Y, 9, special=False)
ORD_MASK, ORD_FRAME = DM.ordering_frame()


def test_a_held_back_weighting_of_the_source_is_flushed_first():
    det = B.DetectorGeometry(2 * ORD_X, 2 * ORD_Y, *DM.ORD_GEO[2:])

    def run(fusion):
        with B.Backend(0, synchronous=False) as abe:
            abe.set_stage_fusion(fusion)
            abe.set_binning(2, 2, 2 * ORD_X, 2 * ORD_Y)
            src = B.load(abe, B.Projection(ORD_SRC.copy(), 2 * ORD_X, 2 * ORD_Y, idx=2))
            dst = abe.make_projection_device(ORD_X, ORD_Y)
            B.weight(abe, src, det)            # with fusion: held back until something touches the frame
            abe.bin_frames(src, dst)
            return read(abe, dst), read(abe, src)

    (plain, weighted), (fused, weighted_f) = run(False), run(True)
    assert np.array_equal(bits(plain), bits(R.bin_frame(weighted, 2, 2))) and not np.array_equal(bits(weighted), bits(ORD_SRC))
    assert np.array_equal(bits(fused), bits(plain)) and np.array_equal(bits(weighted_f), bits(weighted))


@pytest.mark.parametrize("by_reference", [False, True])
@pytest.mark.parametrize("side", ["destination", "source"])
def test_a_frame_of_the_pending_group_is_backprojected_as_it_was(by_reference, side):
    """Binning INTO a buffer the pending by-reference group refers to launches that group first: the volume is the one the snapshot
    path gives. Binning FROM such a buffer launches it as well (the guard covers both bands). With snapshots the group stays pending."""
    det = B.DetectorGeometry(*DM.ORD_GEO)
    vg = B.calculate_volume_geometry(det)

    def run(deferred):
        with B.Backend(0, synchronous=False) as abe:
            if deferred:
                abe.set_backproject_deferral(8)
                abe.set_backproject_references(by_reference)
            if side == "destination":
                abe.set_binning(2, 2, 2 * ORD_X, 2 * ORD_Y)
                src = B.load(abe, B.Projection(ORD_SRC.copy(), 2 * ORD_X, 2 * ORD_Y))
                held = dst = B.load(abe, B.Projection(ORD_FRAME.copy(), ORD_X, ORD_Y, idx=1))
            else:
                abe.set_binning(2, 2, ORD_X, ORD_Y)
                held = src = B.load(abe, B.Projection(ORD_FRAME.copy(), ORD_X, ORD_Y, idx=1))
                dst = abe.make_projection_device(ORD_X // 2, ORD_Y // 2)
            v = abe.make_volume_device(vg.dim_x, vg.dim_y, vg.dim_z)
            B.backproject(abe, held, v, 0, det, vg, False, False, None)
            if deferred:
                assert pending(abe) == 1
            abe.bin_frames(src, dst)
            if deferred:
                assert pending(abe) == (0 if by_reference else 1)
            return read(abe, dst), DM.volume_to_host(abe, v, vg)

    want_p, want_v = run(False)
    got_p, got_v = run(True)
    assert np.abs(want_v).max() > 0
    assert np.array_equal(bits(want_p), bits(R.bin_frame(ORD_SRC if side == "destination" else ORD_FRAME, 2, 2)))
    assert np.array_equal(bits(got_v), bits(want_v)) and np.array_equal(bits(got_p), bits(want_p))
