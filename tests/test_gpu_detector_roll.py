"""The detector roll on the device: paris_hip_detector_roll_rows against the host rule and its numpy
restatement (tests/roll_rule.py), bit for bit -- the 16-byte and the single-pixel path, frame strides past the grid's z cap, rows past
its y cap, row bands, the refusals and the ordering contract of the frame passes -- the physical check on analytic frames of a rolled
detector, the roll search's costs and estimate, and the benefit for a reconstruction."""
import ctypes as C

import numpy as np
import pytest

import ring_rule
import roll_rule as R
import test_gpu_defect_map as DM
from paris_amd import _lib
from paris_amd import backend as B

pytestmark = pytest.mark.gpu

bits, read, pending = DM.bits, DM.read, DM.pending
INV = _lib.ERROR_INVALID_ARGUMENT
SENTINEL = np.uint32(0x7fc0beef)   # a NaN with a payload: never the result of an interpolation
GEO = B.DetectorGeometry(*R.HOST_GEO)
FRAME = R.special_frame()
WANT = {eta: R.roll(FRAME, eta, R.HOST_GEO) for eta in R.HOST_ETAS}


@pytest.fixture(scope="module")
def be():
    with B.Backend(0) as b:
        yield b


def same_bits(got, want):
    """every bit, the sentinel's payload included; elsewhere a NaN may carry any payload"""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    keep = bits(want) == SENTINEL
    nan = np.isnan(want) & ~keep
    return (got.shape == want.shape and np.array_equal(bits(got)[keep], bits(want)[keep]) and np.array_equal(np.isnan(got) & ~keep, nan)
            and np.array_equal(bits(got)[~nan & ~keep], bits(want)[~nan & ~keep]))


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


ALIGNED = lambda n, x, y: layout(n, x, y, 0, (-4 * x) % 16 + 16, 32)      # base, pitch and stride multiples of 16: 16-byte stores
ALIGNED_WIDE = lambda n, x, y: layout(n, x, y, 16, (-4 * x) % 16 + 48, 64)  # another aligned layout: the two sides' strides differ
SCALAR = lambda n, x, y: layout(n, x, y, 4, 4, 8)                        # base offset by 4 bytes, pitch 4 * dim_x + 4: single pixels
SCALAR_WIDE = lambda n, x, y: layout(n, x, y, 12, 12, 20)                # misaligned as well, with another pitch and stride


def roll_in_canvases(be, frames, src_layout, dst_layout, rows=None, **setting):
    """uploads the frames into a source canvas, rolls them into a sentinel-filled destination canvas; returns the destination canvas as
    read back and where its frames lie. The source must come back as it went."""
    n = len(frames)
    dim_y, dim_x = frames[0].shape
    s_off, s_pitch, s_stride, s_bytes = src_layout(n, dim_x, dim_y)
    d_off, d_pitch, d_stride, d_bytes = dst_layout(n, dim_x, dim_y)
    host = np.full(((s_bytes + 255) // 256) * 64, SENTINEL, np.uint32).view(np.float32)
    for k, f in enumerate(frames):
        place(host, s_off + k * s_stride, s_pitch, f)
    src, dst = Canvas(be, s_bytes, host), Canvas(be, d_bytes)
    be.detector_roll(src.view(s_off, s_pitch, dim_x, dim_y), dst.view(d_off, d_pitch, dim_x, dim_y), rows=rows,
                     src_frame_stride=s_stride if n > 1 else 0, dst_frame_stride=d_stride if n > 1 else 0, n_frames=n, **setting)
    got = dst.read()
    assert np.array_equal(src.read().view(np.uint32), host.view(np.uint32))   # the source is only read
    src.free()
    dst.free()
    return got, (d_off, d_pitch, d_stride)


def expected_canvas(got, where, rolled, rows=None):
    d_off, d_pitch, d_stride = where
    want = np.full(got.size, SENTINEL, np.uint32).view(np.float32)
    for k, b in enumerate(rolled):
        first, count = (0, b.shape[0]) if rows is None else rows
        place(want, d_off + k * d_stride + first * d_pitch, d_pitch, b[first:first + count])
    return want


# ---- 1. the rule, bit for bit -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("eta", R.HOST_ETAS)
def test_pool_buffers_take_the_vector_path_bit_for_bit(be, eta):
    """buffers of make_projection_device (rows padded to 256 bytes): 67 columns, so every row ends in a ragged segment of three"""
    assert same_bits(B.detector_roll_host(eta, GEO, FRAME), WANT[eta])
    be.set_detector_roll(eta, GEO)
    try:
        src, dst = be.make_projection_device(67, 45), be.make_projection_device(67, 45)
        assert src.pitch % 256 == 0 and dst.pitch % 256 == 0
        be.upload_raw(FRAME, src)
        be.detector_roll(src, dst)
        assert same_bits(read(be, dst), WANT[eta])
        assert np.array_equal(bits(read(be, src)), bits(FRAME))
        be.free(src)
        be.free(dst)
    finally:
        be.clear_detector_roll()


@pytest.mark.parametrize("eta", R.HOST_ETAS)
@pytest.mark.parametrize("path", ["vector", "scalar", "scalar_source", "scalar_destination"])
def test_padded_pitches_and_misaligned_bases_bit_for_bit(be, eta, path):
    """one frame in canvases: both sides aligned to 16 bytes, both misaligned, and one of each -- the destination alone decides the
    store; the bytes around the frame keep their sentinel"""
    lay_s = SCALAR if path in ("scalar", "scalar_source") else ALIGNED
    lay_d = SCALAR if path in ("scalar", "scalar_destination") else ALIGNED
    be.set_detector_roll(eta, GEO)
    try:
        got, where = roll_in_canvases(be, [FRAME], lay_s, lay_d)
        assert same_bits(got, expected_canvas(got, where, [WANT[eta]]))
    finally:
        be.clear_detector_roll()


@pytest.mark.parametrize("path", ["vector", "scalar"])
def test_seventy_frames_past_the_z_cap_with_unequal_strides(be, path):
    """70 frames over a grid z of 64: frames 64 .. 69 are a second visit; the source's and the destination's strides differ, and the
    gaps between rows and frames keep their sentinel"""
    eta = 2.5
    rng = np.random.default_rng(70)
    frames = [FRAME] + [(rng.uniform(-1.0, 3.0, FRAME.shape)).astype(np.float32) for _ in range(69)]
    lay_s, lay_d = (ALIGNED_WIDE, ALIGNED) if path == "vector" else (SCALAR, SCALAR_WIDE)
    got, where = roll_in_canvases(be, frames, lay_s, lay_d, eta_deg=eta, det_geo=GEO)     # (the _with form: nothing installed)
    want = expected_canvas(got, where, [R.roll(f, eta, R.HOST_GEO) for f in frames])
    assert same_bits(got, want)
    assert np.count_nonzero(bits(got) == SENTINEL) > 70 * 45



@pytest.mark.parametrize("dim_x,dim_y", [(4, 8200), (5, 8200), (1030, 6)])
def test_rows_past_the_y_cap_and_rows_wider_than_one_block(be, dim_x, dim_y):
    """a 4-column detector (one lane per row: one block along x) with more rows than the 8192 blocks of the capped grid, so rows
    8192 .. 8199 are a second visit; 5 columns: a whole segment and a ragged one; 1030 columns: two blocks along x, the last lane
    ragged"""
    g = (dim_x, dim_y, 0.2, 0.25, 0.3, -0.7, 100.0, 200.0, 4.0)
    eta = 0.3 if dim_y > 100 else -2.5
    frame = np.random.default_rng(dim_x).uniform(-1.0, 3.0, (dim_y, dim_x)).astype(np.float32)
    src, dst = be.make_projection_device(dim_x, dim_y), be.make_projection_device(dim_x, dim_y)
    be.upload_raw(frame, src)
    be.upload_raw(np.full((dim_y, dim_x), SENTINEL, np.uint32).view(np.float32), dst)
    be.detector_roll(src, dst, eta_deg=eta, det_geo=B.DetectorGeometry(*g))
    got, want = read(be, dst), R.roll(frame, eta, g)
    assert same_bits(got, want)
    assert same_bits(B.detector_roll_host(eta, B.DetectorGeometry(*g), frame), want)
    assert not np.array_equal(bits(want[-8:]), bits(frame[-8:]))      # the second visit's rows are not the identity
    be.free(src)
    be.free(dst)


# ---- 2. bands ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("eta", [2.5, -10.0, 0.3])
@pytest.mark.parametrize("path", ["vector", "scalar"])
def test_a_band_writes_its_rows_only_and_reads_its_source_rows_only(be, eta, path):
    """rows [r0, r0 + n) equal the whole-frame result while every source row outside paris_hip_detector_roll_source_rows holds NaN, and
    no other destination row is written"""
    clean = np.where(np.isfinite(FRAME), FRAME, np.float32(1.5))
    whole = R.roll(clean, eta, R.HOST_GEO)
    lay = ALIGNED if path == "vector" else SCALAR
    be.set_detector_roll(eta, GEO)
    try:
        for r0, n in ((0, 45), (0, 4), (1, 3), (20, 7), (41, 4), (44, 1), (45, 0), (22, 0)):
            first, count = B.detector_roll_source_rows(eta, GEO, r0, n)
            poisoned = np.full_like(clean, np.nan)
            poisoned[first:first + count] = clean[first:first + count]
            got, where = roll_in_canvases(be, [poisoned, poisoned], lay, lay, rows=(r0, n))
            assert same_bits(got, expected_canvas(got, where, [whole, whole], rows=(r0, n))), (r0, n)
            assert not np.isnan(whole[r0:r0 + n]).any()
            if 0 < n < 45:      # the range is exact: one more poisoned row on either side shows
                for cut in ((first + 1, count - 1), (first, count - 1)):
                    less = np.full_like(clean, np.nan)
                    less[cut[0]:cut[0] + cut[1]] = clean[cut[0]:cut[0] + cut[1]]
                    assert np.isnan(R.roll(less, eta, R.HOST_GEO, rows=(r0, n))).any(), (r0, n, cut)
    finally:
        be.clear_detector_roll()


# ---- 3. refusals and the setting's lifecycle --------------------------------------------------------------------------------------

def test_refusals(be):
    L = _lib.load()
    src, dst = be.make_projection_device(67, 45), be.make_projection_device(67, 45)
    filled = np.full((45, 67), SENTINEL, np.uint32).view(np.float32)
    be.upload_raw(FRAME, src)
    be.upload_raw(filled, dst)

    def raw(s=src, d=dst, s_pitch=None, d_pitch=None, s_stride=0, d_stride=0, n=1, dim_x=67, dim_y=45, row_first=0, row_count=45):
        return L.paris_hip_detector_roll_rows(be._ctx, s if s is None or isinstance(s, int) else s.ptr, src.pitch if s_pitch is None else s_pitch,
                                              s_stride, d if d is None or isinstance(d, int) else d.ptr, dst.pitch if d_pitch is None else d_pitch,
                                              d_stride, n, dim_x, dim_y, row_first, row_count)

    def raw_with(setting, geo):
        return L.paris_hip_detector_roll_rows_with(be._ctx, src.ptr, src.pitch, 0, dst.ptr, dst.pitch, 0, 1, 67, 45, 0, 45, setting, geo)

    assert raw() == INV                                                                # no setting
    assert L.paris_hip_set_detector_roll(be._ctx, C.byref(_lib.DetectorRoll(0.0)), C.byref(GEO)) == INV
    assert L.paris_hip_set_detector_roll(be._ctx, C.byref(_lib.DetectorRoll(10.5)), C.byref(GEO)) == INV
    assert L.paris_hip_set_detector_roll(be._ctx, None, C.byref(GEO)) == INV
    assert L.paris_hip_set_detector_roll(be._ctx, C.byref(_lib.DetectorRoll(1.0)), None) == INV
    assert L.paris_hip_set_detector_roll(None, C.byref(_lib.DetectorRoll(1.0)), C.byref(GEO)) == INV
    assert raw() == INV                                                                # a refused setting installs nothing
    assert raw_with(None, C.byref(GEO)) == INV and raw_with(C.byref(_lib.DetectorRoll(1.0)), None) == INV
    assert raw_with(C.byref(_lib.DetectorRoll(0.0)), C.byref(GEO)) == INV
    assert raw_with(C.byref(_lib.DetectorRoll(1.0)), C.byref(B.DetectorGeometry(66, 45, *R.HOST_GEO[2:]))) == INV
    be.clear_detector_roll()                                                           # clearing nothing is fine
    be.set_detector_roll(2.5, GEO)
    try:
        assert raw(dim_x=66) == INV and raw(dim_y=44) == INV                           # other dimensions than the setting's
        assert raw(row_first=43, row_count=3) == INV and raw(row_first=46, row_count=0) == INV    # a band beyond dim_y
        assert raw(row_first=2 ** 31, row_count=2 ** 31) == INV
        assert raw(s=None) == INV and raw(d=None) == INV
        assert raw(s_pitch=4 * 67 - 4) == INV and raw(s_pitch=src.pitch + 2) == INV    # the argument rule, either side
        assert raw(d_pitch=4 * 67 - 4) == INV and raw(d_pitch=dst.pitch + 2) == INV
        assert raw(n=2, s_stride=src.pitch * 45 - 4, d_stride=dst.pitch * 45) == INV
        assert raw(n=2, s_stride=src.pitch * 45, d_stride=dst.pitch * 45 - 4) == INV
        assert raw(n=2, s_stride=src.pitch * 45 + 2, d_stride=dst.pitch * 45) == INV
        # overlapping source and destination: the same buffer, and a destination that starts inside the source's last row
        assert raw(d=src.ptr, d_pitch=src.pitch) == INV
        assert raw(d=src.ptr + 44 * src.pitch + 4 * 60, d_pitch=src.pitch) == INV
        assert raw(s=dst.ptr + 4, s_pitch=src.pitch) == INV
        assert np.array_equal(bits(read(be, dst)), bits(filled))                       # no refused call wrote anything
        assert raw(row_first=45, row_count=0) == _lib.SUCCESS and raw(n=0) == _lib.SUCCESS and raw(row_first=7, row_count=0) == _lib.SUCCESS
        assert np.array_equal(bits(read(be, dst)), bits(filled))                       # empty calls
        assert raw() == _lib.SUCCESS
        assert same_bits(read(be, dst), WANT[2.5])
        assert raw_with(C.byref(_lib.DetectorRoll(-0.3)), C.byref(GEO)) == _lib.SUCCESS   # the _with form leaves the setting alone
        assert same_bits(read(be, dst), WANT[-0.3])
        assert raw() == _lib.SUCCESS and same_bits(read(be, dst), WANT[2.5])
    finally:
        be.clear_detector_roll()
    assert raw() == INV                                                                # cleared
    be.free(src)
    be.free(dst)


def test_nothing_lives_on_the_device(be):
    before = be.projection_reserve_bytes(67, 45)
    be.set_detector_roll(2.5, GEO)
    assert be.projection_reserve_bytes(67, 45) == before
    be.clear_detector_roll()


# ---- 4. ordering (the contract of tests/test_gpu_frame_passes.py) -----------------------------------------------------------------

ORD_GEO = DM.ORD_GEO
ORD_X, ORD_Y = ORD_GEO[:2]
ORD_MASK, ORD_FRAME = DM.ordering_frame()
ORD_SRC = np.random.default_rng(9).uniform(0.0, 2.0, (ORD_Y, ORD_X)).astype(np.float32)


def test_a_held_back_weighting_of_the_source_is_flushed_first():
    det = B.DetectorGeometry(*ORD_GEO)

    def run(fusion):
        with B.Backend(0, synchronous=False) as abe:
            abe.set_stage_fusion(fusion)
            abe.set_detector_roll(1.2, det)
            src = B.load(abe, B.Projection(ORD_SRC.copy(), ORD_X, ORD_Y, idx=2))
            dst = abe.make_projection_device(ORD_X, ORD_Y)
            B.weight(abe, src, det)            # with fusion: held back until something touches the frame
            abe.detector_roll(src, dst)
            return read(abe, dst), read(abe, src)

    (plain, weighted), (fused, weighted_f) = run(False), run(True)
    assert same_bits(plain, R.roll(weighted, 1.2, ORD_GEO)) and not np.array_equal(bits(weighted), bits(ORD_SRC))
    assert np.array_equal(bits(fused), bits(plain)) and np.array_equal(bits(weighted_f), bits(weighted))


@pytest.mark.parametrize("by_reference", [False, True])
@pytest.mark.parametrize("side", ["destination", "source"])
def test_a_frame_of_the_pending_group_is_backprojected_as_it_was(by_reference, side):
    """Rolling INTO a buffer the pending by-reference group refers to launches that group first: the volume is the one the snapshot
    path gives. Rolling FROM such a buffer launches it as well (the guard covers both bands). With snapshots the group stays pending."""
    det = B.DetectorGeometry(*ORD_GEO)
    vg = B.calculate_volume_geometry(det)

    def run(deferred):
        with B.Backend(0, synchronous=False) as abe:
            if deferred:
                abe.set_backproject_deferral(8)
                abe.set_backproject_references(by_reference)
            abe.set_detector_roll(1.2, det)
            if side == "destination":
                src = B.load(abe, B.Projection(ORD_SRC.copy(), ORD_X, ORD_Y))
                held = dst = B.load(abe, B.Projection(ORD_FRAME.copy(), ORD_X, ORD_Y, idx=1))
            else:
                held = src = B.load(abe, B.Projection(ORD_FRAME.copy(), ORD_X, ORD_Y, idx=1))
                dst = abe.make_projection_device(ORD_X, ORD_Y)
            v = abe.make_volume_device(vg.dim_x, vg.dim_y, vg.dim_z)
            B.backproject(abe, held, v, 0, det, vg, False, False, None)
            if deferred:
                assert pending(abe) == 1
            abe.detector_roll(src, dst)
            if deferred:
                assert pending(abe) == (0 if by_reference else 1)
            return read(abe, dst), DM.volume_to_host(abe, v, vg)

    want_p, want_v = run(False)
    got_p, got_v = run(True)
    assert np.abs(want_v).max() > 0
    assert same_bits(want_p, R.roll(ORD_SRC if side == "destination" else ORD_FRAME, 1.2, ORD_GEO))
    assert np.array_equal(bits(got_v), bits(want_v)) and np.array_equal(bits(got_p), bits(want_p))


# ---- 5. the physical check --------------------------------------------------------------------------------------------------------

def test_frames_of_a_rolled_detector_come_back_to_the_analytic_unrolled_frames(be):
    """Eight views of the recovery spheres on the 96 x 80 detector rolled by 1.2 deg (the rays evaluated at the rotated pixel
    positions), corrected on the device, against the analytic frames of the unrolled detector inside the margins. The largest error
    is at most 1.5 times that of the float64 restatement of the same rule on the same frames.
    Measured: the float64 rule's largest error is 5.14 (delta_s = 0) and 3.81 (delta_s = 1.3) on line integrals of at most 48.5 --
    the bilinear taps across a sphere's edge, where the line integral has a square-root singularity; the fp32 rule's differs from it
    in the sixth digit (5.143776 against 5.143760, 3.814765 against 3.814784). Uncorrected the frames differ by 5.39 and 5.63; as an
    RMS over the frame the correction takes 0.342 to 0.226 -- the edges dominate both. fp32 coordinates cost nothing visible."""
    for delta_s in (0.0, 1.3):
        g = R.geo(delta_s=delta_s)
        det = B.DetectorGeometry(*g)
        rolled, ideal = R.sphere_frames(g, 1.2, n_views=8), R.sphere_frames(g, 0.0, n_views=8)
        m_x, m_y = R.margins(1.2, 1.0, 1, g)
        inside = (slice(None), slice(m_y, g[1] - m_y), slice(m_x, g[0] - m_x))
        ref = np.abs(np.stack([R.roll(f, 1.2, g, np.float64) for f in rolled]) - ideal)[inside].max()
        src, dst = be.make_projection_device(g[0], g[1]), be.make_projection_device(g[0], g[1])
        got = []
        for f in rolled:
            be.upload_raw(f.astype(np.float32), src)
            be.detector_roll(src, dst, eta_deg=1.2, det_geo=det)
            got.append(read(be, dst))
        be.free(src)
        be.free(dst)
        err = np.abs(np.stack(got).astype(np.float64) - ideal)[inside].max()
        print("detector roll, physical: delta_s %.1f, largest error %.6f on the device, %.6f by the float64 rule, %.6f uncorrected" %
              (delta_s, err, ref, np.abs(rolled - ideal)[inside].max()))
        assert err <= 1.5 * ref


# ---- 6. the search ----------------------------------------------------------------------------------------------------------------

def device_mean(be, g, frames):
    """the scan mean as the ring profile pre-pass makes it"""
    d = be.make_projection_device(g[0], g[1])
    be.ring_profile_begin(g[0], g[1])
    for f in frames:
        be.upload_raw(f.astype(np.float32), d)
        be.ring_profile_add_rows(d)
    c, mean, st = be.ring_profile_finish(ring_rule.H, ring_rule.FLOOR, ring_rule.LIMIT)
    be.free(d)
    return mean


@pytest.fixture(scope="module")
def means(be):
    return {(eta, ds): device_mean(be, *R.scan(eta, ds)) for eta, ds in ((0.0, 0.0), (0.8, 1.3), (-1.7, 0.0))}


@pytest.mark.parametrize("eta,delta_s", [(0.0, 0.0), (0.8, 1.3), (-1.7, 0.0)])
def test_search_costs_equal_the_rule_s_and_repeat_bit_for_bit(be, means, eta, delta_s):
    g, frames = R.scan(eta, delta_s)
    mean = means[(eta, delta_s)]
    assert np.abs(mean - frames.mean(axis=0)).max() <= 1e-5 * frames.max()
    det = B.DetectorGeometry(*g)
    res, cost, pairs = be.find_detector_roll(mean, *R.SEARCH, det)
    again = be.find_detector_roll(mean, *R.SEARCH, det)
    want, want_pairs, want_skipped, (m_x, m_y) = R.costs(mean, *R.SEARCH, g)
    assert np.array_equal(pairs, want_pairs) and (res.margin_x, res.margin_y) == (m_x, m_y) and res.skipped == 0 == want_skipped.sum()
    assert np.all(np.isfinite(cost)) and np.abs(cost - want).max() <= 1e-9 * np.abs(want).max() and np.all(np.abs(cost - want) <= 1e-9 * want)
    assert np.array_equal(cost.view(np.uint64), again[1].view(np.uint64)) and np.array_equal(pairs, again[2])
    assert again[0].eta_deg == res.eta_deg
    est = R.estimate(R.SEARCH[0], R.SEARCH[1], cost)
    assert (res.best, res.scored, res.at_edge) == (est["best"], 25, 0) and res.eta_deg == est["value"]
    assert res.cost_min == cost[res.best] and res.cost_median == est["cost_median"]
    print("detector roll, search: true %.2f, delta_s %.1f, estimate %.4f, J_min / J_median %.2g" % (eta, delta_s, res.eta_deg, res.cost_min / res.cost_median))
    assert abs(res.eta_deg - eta) <= R.BOUND_DEG


def test_a_range_that_excludes_the_truth_reports_at_edge(be, means):
    g, _ = R.scan(-1.7, 0.0)
    res, cost, pairs = be.find_detector_roll(means[(-1.7, 0.0)], 0.25, 0.25, 12, B.DetectorGeometry(*g))
    assert (res.best, res.at_edge, res.scored) == (0, 1, 12) and res.eta_deg == np.float32(0.25)
    res, cost, pairs = be.find_detector_roll(means[(-1.7, 0.0)], -3.0, 0.25, 4, B.DetectorGeometry(*g))
    assert (res.best, res.at_edge) == (3, 1) and res.eta_deg == np.float32(-2.25)


def test_a_nan_in_the_mean_is_skipped_and_counted(be, means):
    g, _ = R.scan(0.8, 1.3)
    det = B.DetectorGeometry(*g)
    mean = means[(0.8, 1.3)].copy()
    mean[40, 30] = np.nan
    mean[12, 70] = np.inf
    res, cost, pairs = be.find_detector_roll(mean, *R.SEARCH, det)
    want, want_pairs, want_skipped, _ = R.costs(mean, *R.SEARCH, g)
    assert want_skipped.min() >= 4 and res.skipped == want_skipped.sum() and np.array_equal(pairs, want_pairs)
    assert np.all(np.isfinite(cost)) and np.all(np.abs(cost - want) <= 1e-9 * want)
    assert abs(res.eta_deg - 0.8) <= R.BOUND_DEG
    # too few pairs: unscored, and with nothing scored the estimate refuses
    with pytest.raises(B.ParisHipError):
        be.find_detector_roll(mean, *R.SEARCH, det, min_pixels=96 * 80)
    with pytest.raises(B.ParisHipError):
        be.find_detector_roll(mean, -3.0, 0.25, 257, det)
    with pytest.raises(ValueError):
        be.find_detector_roll(mean[:-1], *R.SEARCH, det)


# ---- 7. the benefit ---------------------------------------------------------------------------------------------------------------

def test_the_correction_more_than_halves_the_error_of_a_reconstruction():
    """A 64^3 reconstruction of the benefit scan (tests/roll_rule.py: 72 views of a 192 x 160 detector rolled by 1.2 deg, four spheres
    far from the mid-plane) through the Backend product path: the RMS difference from the reconstruction of the unrolled scan over
    the central cylinder, with the correction, is below half of that without. With the float64 rule and the CPU oracle the two
    numbers are 0.0240 and 0.106."""
    g, eta = R.BENEFIT_GEO, R.BENEFIT_ETA
    det, vg = B.DetectorGeometry(*g), B.VolumeGeometry(*R.BENEFIT_VOLUME)
    ideal = R.sphere_frames(g, 0.0, R.BENEFIT_SPHERES).astype(np.float32)
    rolled = R.sphere_frames(g, eta, R.BENEFIT_SPHERES).astype(np.float32)

    def reconstruct(frames, correct):
        with B.Backend(0, synchronous=False) as qbe:
            qbe.set_paris_loop_defaults(48)
            if correct:
                qbe.set_detector_roll(eta, det)
                raw = qbe.make_projection_device(det.n_row, det.n_col)
            v = qbe.make_volume_device(vg.dim_x, vg.dim_y, vg.dim_z)
            for i, fr in enumerate(frames):
                d_p = qbe.make_projection_device(det.n_row, det.n_col)
                if correct:
                    qbe.upload_raw(fr, raw)
                    qbe.detector_roll(raw, d_p)
                else:
                    qbe.upload_raw(fr, d_p)
                d_p.idx = i
                B.weight(qbe, d_p, det)
                B.filter(qbe, d_p, det)
                B.backproject(qbe, d_p, v, 0, det, vg, False, False, None)
                qbe.free(d_p)
            qbe.flush()
            return DM.volume_to_host(qbe, v, vg).reshape(vg.dim_z, vg.dim_y, vg.dim_x)

    truth = reconstruct(ideal, False)
    without = R.cylinder_rms(reconstruct(rolled, False), truth)
    corrected = R.cylinder_rms(reconstruct(rolled, True), truth)
    print("detector roll, benefit: RMS difference %.5g uncorrected, %.5g corrected (ratio %.3f)" % (without, corrected, corrected / without))
    assert np.abs(truth).max() > 1.0 and corrected < 0.5 * without
