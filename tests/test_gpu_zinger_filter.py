"""Removal of per-frame outlier pixels on the device (paris_hip_set_zinger_filter / paris_hip_zinger_filter_rows, DESIGN.md section
4.10): equality with the numpy restatement of the rule (tests/zinger_rule.py), bands, batches, saturation and the counts, the ordering
rules and the setting's lifecycle."""
import ctypes as C

import numpy as np
import pytest

import test_gpu_flat_field as FF
import zinger_rule as Z
from paris_amd import _lib
from paris_amd import backend as B

pytestmark = pytest.mark.gpu

ORD_GEO = (96, 80, 0.2, 0.25, 1.5, -0.75, 100, 200, 45.0)
THRESHOLDS = {"abs": (Z.T_ABS, 0.0), "rel": (0.0, 0.15), "both": (Z.T_ABS, 0.1)}   # rel: 0.22 .. 0.38 on the frames' 1.5 .. 2.5
FRAMES = {dim_x: Z.planted_frame(dim_x) for dim_x in (96, 100)}


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


def filtered(be, frame, tight=False, **band):
    """the frame after one zinger_filter_rows() call with the current setting"""
    dim_y, dim_x = frame.shape
    d, owner = FF.device_frame(be, dim_x, dim_y, tight)
    be.upload_raw(frame, d)
    be.zinger_filter_rows(d, **band)
    got = read(be, d)
    be.free(owner)
    return got


def assert_equals_rule(got, frame, t_abs, t_rel, polarity, max_hits=0, rows=None, what=""):
    """the values equal the rule's; every pixel the rule does not write keeps its bits, NaN payloads included"""
    want, flags, saturated = Z.run(frame, t_abs, t_rel, polarity, max_hits, rows)
    assert np.array_equal(got, want, equal_nan=True), what
    assert np.array_equal(got[flags], want[flags]) and np.all(np.isfinite(got[flags])), what
    assert np.array_equal(bits(got)[~flags], bits(frame)[~flags]), what
    return int(np.count_nonzero(flags))


# ---- 1. equality with the rule ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("thresholds", ["abs", "rel", "both"])
@pytest.mark.parametrize("polarity", ["bright", "dark", "both"])
@pytest.mark.parametrize("dim_x,tight", [(96, False), (100, False), (100, True)])
def test_equality_with_the_rule(be, dim_x, tight, polarity, thresholds):
    frame, planted = FRAMES[dim_x]
    t_abs, t_rel = THRESHOLDS[thresholds]
    flags = Z.flagged(frame, t_abs, t_rel, polarity)[0]
    assert flags.sum() >= 20 and not np.any(flags & ~planted)      # the planted pixels and nothing else: no empty hit list
    assert not flags[15, 46] and not flags[15, 56]                 # the centres of the 3 x 3 blobs survive
    be.set_zinger_filter(t_abs, t_rel, polarity, dim_x, 37)
    try:
        d, owner = FF.device_frame(be, dim_x, 37, tight)
        assert (d.pitch == 4 * dim_x) == tight
        be.free(owner)
        got = filtered(be, frame, tight)
        assert assert_equals_rule(got, frame, t_abs, t_rel, polarity, what=(dim_x, tight, polarity, thresholds)) == flags.sum()
        st = be.zinger_stats(reset=True)
        assert (st.frames, st.replaced, st.saturated_frames) == (1, flags.sum(), 0)
    finally:
        be.clear_zinger_filter()


@pytest.mark.parametrize("dim_x", [260, 261])
def test_more_than_one_block_in_either_direction(be, dim_x):
    """more than 256 columns are two column groups, 70 rows two blocks of four 16-row strips; 260 columns take the 16-byte loads, 261
    (and every pitch that is no multiple of 16 bytes) the scalar ones"""
    frame, planted = Z.scattered_frame(dim_x, 70, 11)
    flags = Z.flagged(frame, Z.T_ABS, 0.0, "both")[0]
    assert flags.sum() >= 100 and not np.any(flags & ~planted) and flags[:, 256:].any() and flags[64:].any()
    be.set_zinger_filter(Z.T_ABS, 0.0, "both", dim_x, 70)
    try:
        for tight in (False, True):
            assert assert_equals_rule(filtered(be, frame, tight), frame, Z.T_ABS, 0.0, "both") == flags.sum()
    finally:
        be.clear_zinger_filter()


@pytest.mark.parametrize("dim_x,dim_y", [(1, 1), (1, 7), (5, 1), (2, 2), (3, 3)])
def test_degenerate_frames(be, dim_x, dim_y):
    rng = np.random.default_rng(dim_x * 10 + dim_y)
    be.set_zinger_filter(Z.T_ABS, 0.0, "both", dim_x, dim_y)
    try:
        for k in range(dim_x * dim_y):   # a spike on every pixel in turn
            frame = (2 + rng.normal(0, Z.SIGMA, (dim_y, dim_x))).astype(np.float32)
            frame.reshape(-1)[k] += Z.SPIKE
            for tight in (False, True):
                assert_equals_rule(filtered(be, frame, tight), frame, Z.T_ABS, 0.0, "both", what=(dim_x, dim_y, k, tight))
    finally:
        be.clear_zinger_filter()


# ---- 2. bands -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim_x", [96, 100])
def test_a_band_equals_the_same_rows_of_the_whole_frame(be, dim_x):
    first, count = 9, 19                       # rows 9 .. 27: crosses the strips of the whole-frame call differently
    last = first + count - 1
    frame = Z.smooth(dim_x, 37, 21)
    planted = np.zeros(frame.shape, bool)
    for k, y in enumerate((first - 1, first, last, last + 1)):
        for x in (0, 13 + k, 50 + 2 * k, dim_x - 1):
            frame[y, x] += np.float32(Z.SPIKE if (x + k) % 2 else -Z.SPIKE)
            planted[y, x] = True
    whole_flags = Z.flagged(frame, Z.T_ABS, 0.0, "both")[0]
    assert np.array_equal(whole_flags, planted)
    be.set_zinger_filter(Z.T_ABS, 0.0, "both", dim_x, 37)
    try:
        whole = filtered(be, frame)
        band = filtered(be, frame, row_first=first, row_count=count)
        assert np.array_equal(bits(band[first:last + 1]), bits(whole[first:last + 1]))
        assert np.array_equal(bits(band[:first]), bits(frame[:first])) and np.array_equal(bits(band[last + 1:]), bits(frame[last + 1:]))
        assert assert_equals_rule(band, frame, Z.T_ABS, 0.0, "both", rows=(first, last + 1)) == 8
        # rows outside the band widened by 1 hold NaN: they are not read
        poisoned = frame.copy()
        poisoned[:first - 1] = np.nan
        poisoned[last + 2:] = np.nan
        got = filtered(be, poisoned, row_first=first, row_count=count)
        assert np.array_equal(bits(got[first - 1:last + 2]), bits(band[first - 1:last + 2]))
        assert np.all(np.isnan(got[:first - 1])) and np.all(np.isnan(got[last + 2:]))
        # the last row alone, then an empty band
        d = be.make_projection_device(dim_x, 37)
        be.upload_raw(frame, d)
        be.zinger_filter_rows(d, row_first=36, row_count=1)
        be.zinger_filter_rows(d, row_first=37, row_count=0)
        assert np.array_equal(bits(read(be, d)), bits(Z.apply(frame, Z.T_ABS, 0.0, "both", rows=(36, 37))[0]))
        be.free(d)
    finally:
        be.clear_zinger_filter()


# ---- 3. frames ----------------------------------------------------------------------------------------------------------------------

def test_three_frames_with_a_frame_stride_equal_three_single_calls(be):
    frames = [Z.planted_frame(100, seed=30 + k)[0] for k in range(3)]
    be.set_zinger_filter(Z.T_ABS, 0.0, "both", 100, 37)
    try:
        d = be.make_projection_device(100, 3 * 37)
        stride = d.pitch * 37
        views = [be.wrap_projection(d.ptr + k * stride, d.pitch, 100, 37) for k in range(3)]
        for h, v in zip(frames, views):
            be.upload_raw(h, v)
        be.zinger_filter_rows(views[0], row_first=2, row_count=33, frame_stride=stride, n_frames=3)
        got = read(be, d).reshape(3, 37, 100)
        for k in range(3):
            single = filtered(be, frames[k], row_first=2, row_count=33)
            assert np.array_equal(bits(got[k]), bits(single)), k
            assert assert_equals_rule(got[k], frames[k], Z.T_ABS, 0.0, "both", rows=(2, 35)) >= 20
        be.free(d)
    finally:
        be.clear_zinger_filter()


def test_more_frames_than_one_launch_serves(be):
    n = 2 * _lib.ZINGER_FRAMES_MAX + 3
    rng = np.random.default_rng(8)
    frames = (2 + rng.normal(0, Z.SIGMA, (n, 8, 8))).astype(np.float32)
    for k in range(n):
        frames[k, 1 + k % 6, 1 + (k // 6) % 6] += Z.SPIKE
        if k % 5 == 0:   # saturated with max_hits = 2
            frames[k, [0, 3, 7], [7, 3, 0]] -= Z.SPIKE
    be.set_zinger_filter(Z.T_ABS, 0.0, "both", 8, 8, max_hits=2)
    try:
        d = be.make_projection_device(8, 8 * n)
        stride = d.pitch * 8
        be.upload_raw(frames.reshape(8 * n, 8), d)
        be.zinger_filter_rows(be.wrap_projection(d.ptr, d.pitch, 8, 8), frame_stride=stride, n_frames=n)
        got = read(be, d).reshape(n, 8, 8)
        replaced = saturated = 0
        for k in range(n):
            want, r, s = Z.apply(frames[k], Z.T_ABS, 0.0, "both", max_hits=2)
            assert np.array_equal(bits(got[k]), bits(want)), k
            replaced, saturated = replaced + r, saturated + s
        assert replaced >= n // 2 and saturated >= n // 6
        st = be.zinger_stats()
        assert (st.frames, st.replaced, st.saturated_frames) == (n, replaced, saturated)
        be.free(d)
    finally:
        be.clear_zinger_filter()


# ---- 4. saturation and the counts ------------------------------------------------------------------------------------------------------

def test_saturation_and_the_counts(be):
    a = Z.smooth(100, 37, 40)
    b = a.copy()
    for y, x in ((3, 3), (20, 50), (36, 99)):
        a[y, x] += Z.SPIKE
        b[y, x] -= Z.SPIKE
    b[10, 10] += Z.SPIKE
    assert Z.flagged(a, Z.T_ABS, 0.0, "both")[0].sum() == 3 and Z.flagged(b, Z.T_ABS, 0.0, "both")[0].sum() == 4
    assert B.zinger_filter_check(Z.T_ABS, 0.0, "both", 3, 100, 37)[0] == 3
    be.set_zinger_filter(Z.T_ABS, 0.0, "both", 100, 37, max_hits=3)
    try:
        got_a, got_b = filtered(be, a), filtered(be, b)
        assert assert_equals_rule(got_a, a, Z.T_ABS, 0.0, "both", max_hits=3) == 3 and not np.array_equal(bits(got_a), bits(a))
        assert np.array_equal(bits(got_b), bits(b))                        # exactly as it was
        st = be.zinger_stats()
        assert (st.frames, st.replaced, st.saturated_frames) == (2, 3, 1)
        filtered(be, a)
        st = be.zinger_stats(reset=True)                                   # accumulated over the second call, then cleared
        assert (st.frames, st.replaced, st.saturated_frames) == (3, 6, 1)
        st = be.zinger_stats()
        assert (st.frames, st.replaced, st.saturated_frames) == (0, 0, 0)
        be.set_zinger_filter(Z.T_ABS, 0.0, "both", 100, 37, max_hits=4)    # a new setting starts from zero, and fits frame b
        assert assert_equals_rule(filtered(be, b), b, Z.T_ABS, 0.0, "both", max_hits=4) == 4
        st = be.zinger_stats()
        assert (st.frames, st.replaced, st.saturated_frames) == (1, 4, 0)
    finally:
        be.clear_zinger_filter()


# ---- 5. ordering, refusals and the setting's lifecycle (the patterns of tests/test_gpu_defect_map.py) ---------------------------------

def pending(be):
    n, ptr = C.c_uint32(0), C.c_void_p()
    assert be._L.paris_hip_pending_backprojections(be._ctx, C.byref(n), C.byref(ptr)) == 0
    return n.value


def ordering_frame():
    frame, planted = Z.scattered_frame(96, 80, 50)
    return frame


def test_a_held_back_weighting_is_flushed_first():
    det = B.DetectorGeometry(*ORD_GEO)
    frame = ordering_frame()

    def run(fusion):
        with B.Backend(0, synchronous=False) as abe:
            abe.set_stage_fusion(fusion)
            abe.set_zinger_filter(Z.T_ABS, 0.0, "both", 96, 80)
            d_p = B.load(abe, B.Projection(frame.copy(), 96, 80, idx=2))
            B.weight(abe, d_p, det)            # with fusion: held back until something touches the frame
            abe.zinger_filter_rows(d_p)
            return read(abe, d_p), abe.zinger_stats().replaced

    (plain, n_plain), (fused, n_fused) = run(False), run(True)
    assert n_plain > 20 and n_fused == n_plain
    assert not np.array_equal(bits(plain), bits(frame)) and np.array_equal(bits(fused), bits(plain))


def volume_to_host(abe, v, vg):
    h = abe.make_volume_host(vg.dim_x, vg.dim_y, vg.dim_z)
    abe.copy_d2h(v, h)
    return h.buf.copy()


@pytest.mark.parametrize("references", [False, True])
def test_a_frame_of_the_pending_group_is_backprojected_as_it_was(references):
    """by reference: the group that refers to the frame is launched before the filter writes it; snapshots: it stays pending"""
    det = B.DetectorGeometry(*ORD_GEO)
    vg = B.calculate_volume_geometry(det)
    frame = ordering_frame()

    def run(deferred):
        with B.Backend(0, synchronous=False) as abe:
            if deferred:
                abe.set_backproject_deferral(8)
                abe.set_backproject_references(references)
            abe.set_zinger_filter(Z.T_ABS, 0.0, "both", 96, 80)
            v = abe.make_volume_device(vg.dim_x, vg.dim_y, vg.dim_z)
            d_p = B.load(abe, B.Projection(frame.copy(), 96, 80, idx=1))
            B.backproject(abe, d_p, v, 0, det, vg, False, False, None)
            if deferred:
                assert pending(abe) == 1
            abe.zinger_filter_rows(d_p)
            if deferred:
                assert pending(abe) == (0 if references else 1)
            return read(abe, d_p), volume_to_host(abe, v, vg)

    want_p, want_v = run(False)
    got_p, got_v = run(True)
    assert np.abs(want_v).max() > 0 and not np.array_equal(bits(want_p), bits(frame))
    assert np.array_equal(bits(got_v), bits(want_v)) and np.array_equal(bits(got_p), bits(want_p))


def test_refusals(be):
    L = _lib.load()
    d = be.make_projection_device(96, 80)
    st = _lib.ZingerCounts()
    zf = _lib.ZingerFilter(Z.T_ABS, 0.0, 0, 0)
    with pytest.raises(B.ParisHipError) as e:   # no setting
        be.zinger_filter_rows(d)
    assert e.value.status == _lib.ERROR_INVALID_ARGUMENT
    assert L.paris_hip_zinger_stats(be._ctx, C.byref(st), 0) == _lib.ERROR_INVALID_ARGUMENT
    assert L.paris_hip_set_zinger_filter(be._ctx, None, 96, 80) == _lib.ERROR_INVALID_ARGUMENT
    assert L.paris_hip_set_zinger_filter(be._ctx, C.byref(zf), 0, 80) == _lib.ERROR_INVALID_ARGUMENT
    assert L.paris_hip_set_zinger_filter(be._ctx, C.byref(_lib.ZingerFilter(0.0, 0.0, 0, 0)), 96, 80) == _lib.ERROR_INVALID_ARGUMENT
    assert L.paris_hip_set_zinger_filter(be._ctx, C.byref(_lib.ZingerFilter(0.1, 0.0, 3, 0)), 96, 80) == _lib.ERROR_INVALID_ARGUMENT
    with pytest.raises(B.ParisHipError):        # a refused setting sets nothing
        be.zinger_filter_rows(d)
    be.clear_zinger_filter()                     # clearing nothing is fine
    be.set_zinger_filter(Z.T_ABS, 0.0, "both", 96, 80)
    try:
        assert L.paris_hip_zinger_stats(be._ctx, None, 0) == _lib.ERROR_INVALID_ARGUMENT
        other = be.make_projection_device(97, 80)
        with pytest.raises(B.ParisHipError):
            be.zinger_filter_rows(other)                                                            # other dimensions
        with pytest.raises(B.ParisHipError):
            be.zinger_filter_rows(B.Projection(d.ptr, 96, 79, pitch=d.pitch, on_device=True))
        with pytest.raises(B.ParisHipError):
            be.zinger_filter_rows(B.Projection(d.ptr, 96, 80, pitch=4 * 96 - 4, on_device=True))    # a bad pitch
        with pytest.raises(B.ParisHipError):
            be.zinger_filter_rows(B.Projection(d.ptr, 96, 80, pitch=d.pitch + 2, on_device=True))
        with pytest.raises(B.ParisHipError):
            be.zinger_filter_rows(d, row_first=70, row_count=11)                                    # a bad band
        with pytest.raises(B.ParisHipError):
            be.zinger_filter_rows(d, row_first=81, row_count=0)
        assert L.paris_hip_zinger_filter_rows(be._ctx, d.ptr, d.pitch, d.pitch * 80 - 4, 2, 96, 80, 0, 80) == _lib.ERROR_INVALID_ARGUMENT
        assert L.paris_hip_zinger_filter_rows(be._ctx, d.ptr, d.pitch, d.pitch * 80 + 2, 2, 96, 80, 0, 80) == _lib.ERROR_INVALID_ARGUMENT
        assert L.paris_hip_zinger_filter_rows(be._ctx, None, d.pitch, 0, 1, 96, 80, 0, 80) == _lib.ERROR_INVALID_ARGUMENT
        st = be.zinger_stats()
        assert (st.frames, st.replaced, st.saturated_frames) == (0, 0, 0)   # a refused call examines nothing
        be.free(other)
    finally:
        be.clear_zinger_filter()
    be.free(d)


def test_reserve_bytes_grow_by_the_scratch_and_shrink_again(be):
    before = be.projection_reserve_bytes(96, 80)
    hits, nbytes = B.zinger_filter_check(Z.T_ABS, 0.0, "both", 0, 96, 80)
    small = B.zinger_filter_check(Z.T_ABS, 0.0, "both", 7, 96, 80)[1]
    assert hits == 1024 and nbytes > small > 0
    be.set_zinger_filter(Z.T_ABS, 0.0, "both", 96, 80)
    assert be.projection_reserve_bytes(96, 80) == before + nbytes
    be.set_zinger_filter(Z.T_ABS, 0.0, "both", 96, 80, max_hits=7)   # replaced: the new scratch's bytes, not both
    assert be.projection_reserve_bytes(96, 80) == before + small
    be.clear_zinger_filter()
    assert be.projection_reserve_bytes(96, 80) == before


def test_replacement_and_clear_respect_queued_work():
    dim = 1024
    frames = [Z.scattered_frame(dim, dim, 60 + k, share=0.0005)[0] for k in range(4)]
    t_b = 0.1   # the second setting: dark only, a lower threshold
    with B.Backend(0, synchronous=False) as abe:
        abe.set_zinger_filter(Z.T_ABS, 0.0, "both", dim, dim)
        ds = [abe.make_projection_device(dim, dim) for _ in frames]
        for h, d in zip(frames, ds):
            abe.upload_raw(h, d)
            abe.zinger_filter_rows(d)
        abe.set_zinger_filter(t_b, 0.0, "dark", dim, dim)   # the four passes above may still be queued: they keep the old scratch
        e = abe.make_projection_device(dim, dim)
        abe.upload_raw(frames[0], e)
        abe.zinger_filter_rows(e)
        n_b = abe.zinger_stats().replaced
        abe.clear_zinger_filter()
        for h, d in zip(frames, ds):
            assert assert_equals_rule(read(abe, d), h, Z.T_ABS, 0.0, "both", what="before the replacement") > 300
        assert assert_equals_rule(read(abe, e), frames[0], t_b, 0.0, "dark", what="after the replacement") == n_b > 100
        with pytest.raises(B.ParisHipError):   # cleared: the pass is refused
            abe.zinger_filter_rows(e)
        for d in ds + [e]:
            abe.free(d)


# ---- 6. the driver and the C++ mirror against the Python mirror ------------------------------------------------------------------

import subprocess   # noqa: E402

import test_gpu_paris_hip as P   # noqa: E402
from oracle import formats as F   # noqa: E402

DRV_T_ABS = 1.5   # on the driver set's line integrals (uniform in 0 .. 3): flags a few percent of the pixels, far from max_hits


def mirror_volume(frames, dark, flat, t_min, mask, bands):
    """PARIS's loop through the Python mirror: correct -> repair -> zinger filter -> weight -> filter -> backproject. Returns the volume
    and, per band of `bands`, what the numpy rule flags in the band's rows of the repaired frames, summed over the frames"""
    det = B.DetectorGeometry(*FF.DRV_GEO)
    vg = B.calculate_volume_geometry(det)
    counts = [0] * len(bands)
    with B.Backend(0) as mbe:
        mbe.set_flat_field(dark, flat, t_min)
        if mask is not None:
            mbe.set_defect_map(mask)
        mbe.set_zinger_filter(DRV_T_ABS, 0.0, "dark", FF.DRV_GEO[0], FF.DRV_GEO[1])
        v = mbe.make_volume_device(vg.dim_x, vg.dim_y, vg.dim_z)
        for i, fr in enumerate(frames):
            d_p = B.load(mbe, B.Projection(fr.astype(np.float32), FF.DRV_GEO[0], FF.DRV_GEO[1], idx=i))
            mbe.flat_field_rows(d_p)
            if mask is not None:
                mbe.defect_repair_rows(d_p)
            repaired = read(mbe, d_p)
            mbe.zinger_filter_rows(d_p)
            want, flags, saturated = Z.run(repaired, DRV_T_ABS, 0.0, "dark")
            assert not saturated and np.array_equal(bits(read(mbe, d_p)), bits(want)), i
            for k, (first, count) in enumerate(bands):
                counts[k] += int(np.count_nonzero(flags[first:first + count]))
            B.weight(mbe, d_p, det)
            B.filter(mbe, d_p, det)
            B.backproject(mbe, d_p, v, 0, det, vg, False, False, None)
            mbe.free(d_p)
        st = mbe.zinger_stats()
        h = mbe.make_volume_host(vg.dim_x, vg.dim_y, vg.dim_z)
        mbe.copy_d2h(v, h)
    return h.buf.reshape(vg.dim_z, vg.dim_y, vg.dim_x).copy(), counts, st


@pytest.mark.parametrize("defects", [False, True])
def test_driver_and_cpp_mirror_against_the_python_mirror(tmp_path, defects):
    det = B.DetectorGeometry(*FF.DRV_GEO)
    vg = B.calculate_volume_geometry(det)
    n_row, n_col = FF.DRV_GEO[:2]
    n_frames = 75
    geo, ref, counts_dir, fr, d, f = FF.driver_set(tmp_path, n_frames)
    dz = vg.dim_z // 3
    bands = [B.slab_row_band(det, vg, vg.dim_x, vg.dim_y, dz + (vg.dim_z % 3 if k == 2 else 0), k * dz) for k in range(3)]
    whole = B.slab_row_band(det, vg, vg.dim_x, vg.dim_y, vg.dim_z, 0)
    assert all(0 < b[0] or b[0] + b[1] < n_col for b in bands)
    # zingers (saturated counts: deep negative line integrals) on and next to the band edges of the middle slab, in every third frame
    lo, hi = bands[1][0], bands[1][0] + bands[1][1] - 1
    for y, x in ((lo - 1, 8), (lo, 16), (lo, 17), (hi, 24), (hi + 1, 40), (lo + 1, 34), (hi, 0), (lo, n_row - 1)):
        fr[::3, y, x] = 65535
    (counts_dir / "a.his").write_bytes(F.his_file_bytes(fr[:70], 4, 32))
    (counts_dir / "b.his").write_bytes(F.his_file_bytes(fr[70:], 4, 32))
    mask = None
    if defects:   # defects on the band edges, next to zingers: the repair must cover the band widened by 1
        mask = np.zeros((n_col, n_row), np.uint8)
        mask[:, 33] = 1
        mask[lo - 1, 10:14] = 1
        mask[hi + 1, 20:23] = 1
        mask[lo, 50] = 1
        mask[0, 0] = 1   # the flat field's dead pixel (driver_set)
        (tmp_path / "mask.raw").write_bytes(mask.tobytes())
    want, counts, st = mirror_volume(fr, d, f, 1e-5, mask, [whole] + bands)
    assert (st.frames, st.saturated_frames) == (n_frames, 0) and counts[0] <= st.replaced and st.replaced > 8 * (n_frames // 3)
    assert np.abs(want).max() > 0
    base = [P.EXE, "--geometry", geo, "--input", counts_dir, "--flat", ref / "flat.his", "--dark", ref / "dark.his", "--zingers", DRV_T_ABS]
    if defects:
        base += ["--defects", tmp_path / "mask.raw"]
    for k, (extra, n_bands, n_replaced) in enumerate(((["--slabs", 1], 1, counts[0]), (["--slabs", 3], 3, sum(counts[1:])),
                                                      (["--slabs", 3, "--batch", 1], 3, sum(counts[1:])))):
        o = tmp_path / ("o%d" % k)
        r = subprocess.run([str(a) for a in base + ["--output", o] + extra], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "zinger filter on: %d frame band(s) examined, %d pixel(s) replaced, 0 saturated" % (n_frames * n_bands, n_replaced) in r.stdout, r.stdout
        assert np.array_equal(bits(F.ddbvf_read(str(o / "vol.ddbvf"))[1]), bits(want)), extra
    # refused before any device work
    for bad, word in [] if defects else ((["--zingers", "abc"], "--zingers"), (["--zingers", "0.5:"], "--zingers"), (["--zingers", "-1"], "--zingers"),
                      (["--zingers", "0:0"], "--zingers"), (["--zingers", "1", "--zinger-polarity", "up"], "--zinger-polarity"),
                      (["--zinger-polarity", "dark"], "--zinger-polarity")):
        r = subprocess.run([str(a) for a in base[:9] + ["--output", tmp_path / "bad"] + bad], capture_output=True, text=True, timeout=300)
        assert r.returncode == 1 and word in r.stderr, (bad, r.stderr)
    assert not (tmp_path / "bad").exists()
    # PARIS's loop through paris::hip with set_flat_field, set_defect_map and set_zinger_filter (paris_hip_demo --flat [--defects] --zingers)
    raw = tmp_path / "in.raw"
    fr.astype(np.float32).tofile(raw)
    d.tofile(tmp_path / "dark.raw")
    f.tofile(tmp_path / "flat.raw")
    out = tmp_path / "demo.raw"
    r = subprocess.run([FF.DEMO] + [str(v) for v in FF.DRV_GEO] + [str(n_frames), str(raw), str(out), "--slabs", "2", "--flat",
                                                                str(tmp_path / "dark.raw"), str(tmp_path / "flat.raw"), "1e-05",
                                                                "--zingers", str(DRV_T_ABS), "0", "-1"]
                       + (["--defects", str(tmp_path / "mask.raw")] if defects else []),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr + r.stdout
    assert np.array_equal(bits(np.fromfile(out, np.float32).reshape(want.shape)), bits(want))


# ---- 7. quality ---------------------------------------------------------------------------------------------------------------------

def test_quality_of_a_reconstruction_with_filtered_zingers():
    """Relative RMS against the reconstruction from clean frames, 64 x 48 driver geometry, head phantom, 360 views, dark spikes of depth
    1.0 in 0.2 % of the pixels of every view, threshold 0.25 dark. The oracle with the numpy rule (tests/test_zinger_host.py): 0.10651
    unfiltered, 0.0076349 filtered, 0 for the clean frames through the rule; the device's filter is exact, only the row filter's FFT
    rounding differs."""
    import defect_rule as R
    det = B.DetectorGeometry(*R.QUALITY_GEO)
    vg = B.calculate_volume_geometry(det)
    lines = R.quality_frames(vg.dim_x, vg.l_vx_x)
    spiked = Z.quality_spiked(lines)

    def reconstruct(frames, zingers):
        with B.Backend(0, synchronous=False) as qbe:
            qbe.set_paris_loop_defaults(48)
            if zingers:
                qbe.set_zinger_filter(Z.QUALITY_T_ABS, 0.0, "dark", det.n_row, det.n_col)
            v = qbe.make_volume_device(vg.dim_x, vg.dim_y, vg.dim_z)
            for i, fr in enumerate(frames):
                d_p = qbe.make_projection_device(det.n_row, det.n_col)
                qbe.upload_raw(fr, d_p)
                d_p.idx = i
                if zingers:
                    qbe.zinger_filter_rows(d_p)
                B.weight(qbe, d_p, det)
                B.filter(qbe, d_p, det)
                B.backproject(qbe, d_p, v, 0, det, vg, False, False, None)
                qbe.free(d_p)
            qbe.flush()
            st = qbe.zinger_stats() if zingers else None
            return volume_to_host(qbe, v, vg), st

    clean = reconstruct(lines, False)[0]
    a = R.relative_rms(reconstruct(spiked, False)[0], clean)
    got, st = reconstruct(spiked, True)
    b = R.relative_rms(got, clean)
    print("zinger quality: relative RMS %.5g unfiltered, %.5g filtered (%d pixels replaced in %d frames)" % (a, b, st.replaced, st.frames))
    assert (st.frames, st.saturated_frames) == (len(lines), 0)
    assert st.replaced == sum(Z.apply(p, Z.QUALITY_T_ABS, 0.0, "dark")[1] for p in spiked)
    assert b < a
    assert b <= Z.BOUND * Z.CAL_FILTERED
