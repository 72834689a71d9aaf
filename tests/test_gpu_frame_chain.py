"""The frame passes between the raw upload and the cosine weight as ONE chain on the Python mirror: upload_raw,
bin_frames, flat_field_rows, air_normalize, defect_repair_rows, zinger_filter_rows, ring_correct_rows and beam_hardening, every frame read
back after every pass and held bit for bit to the composed numpy rule (tests/chain_rule.py) -- on whole frames, and band by band with
exactly the rows the driver derives for a slab. tests/test_frame_chain_host.py shows on the CPU that every pass of the composed rule
changes bits on this scan; the same conditions are asserted here, so no equality below can be met by a pass that does nothing."""
import numpy as np
import pytest

import chain_rule as CH
import ring_rule
from paris_amd import backend as B
from test_gpu_ring_correction import read

pytestmark = pytest.mark.gpu

BATCH = 3
GAP_ROWS = 2            # rows between the frames of a buffer: the frame stride is larger than the frame

# (first, count) on the detector the chain runs on. Unbinned: 45 rows, the repair reaches 8 rows, the air rectangle holds rows 1 .. 6;
# --bin 2: 22 rows, reach 4, rectangle rows 0 .. 3. In order: the first row only, the last row only, (0, 7), an interior band whose
# widened range meets the rectangle's rows, one whose range does not, one with defects within the reach of either edge -- whose `fix`
# ends at the pixel of chain_rule.scan_mask that reads the whole reach below --, one whose `fix` begins at that pixel, which reads the
# whole reach above, and the whole frame
BANDS = {1: [(0, 1), (44, 1), (0, 7), (12, 4), (20, 5), (16, 13), (30, 5), (0, 45)],
         2: [(0, 1), (21, 1), (0, 7), (6, 3), (12, 3), (9, 5), (15, 3), (0, 22)]}
BAND_NAMES = ["first_row", "last_row", "rows_0_to_6", "meets_the_rectangle", "clear_of_the_rectangle", "defects_at_both_edges",
              "whole_reach_above", "whole_frame"]
assert all(len(b) == len(BAND_NAMES) for b in BANDS.values())


@pytest.fixture(scope="module")
def scan():
    return CH.scan()


@pytest.fixture(scope="module", params=[2, 1], ids=["bin2", "unbinned"])
def case(request, scan):
    st = CH.settings(scan, request.param)
    steps, info = CH.chain(scan.counts, st)
    CH.assert_every_pass_counts(scan.counts, st, steps, info)      # numpy alone: holds before anything runs on the device
    return st, steps, info


@pytest.fixture(scope="module")
def be():
    with B.Backend(0) as b:
        yield b


class Frames:
    """n frames of dim_x x dim_y in one pool buffer, GAP_ROWS rows apart; every pixel, the gaps included, starts as CH.SENTINEL"""

    def __init__(self, be, n, dim_x, dim_y):
        self.be, self.n, self.dim_x, self.dim_y = be, n, dim_x, dim_y
        self.owner = be.make_projection_device(dim_x, n * (dim_y + GAP_ROWS))
        self.pitch = self.owner.pitch
        self.stride = self.pitch * (dim_y + GAP_ROWS)
        be.upload_raw(np.full((n * (dim_y + GAP_ROWS), dim_x), CH.SENTINEL, np.uint32).view(np.float32), self.owner)

    def frame(self, k):
        return self.be.wrap_projection(self.owner.ptr + k * self.stride, self.pitch, self.dim_x, self.dim_y)

    def read(self):
        """(frames, gaps)"""
        a = read(self.be, self.owner).reshape(self.n, self.dim_y + GAP_ROWS, self.dim_x)
        return a[:, :self.dim_y], a[:, self.dim_y:]

    def assert_holds(self, want, what):
        got, gaps = self.read()
        assert np.array_equal(CH.bits(got), CH.bits(want)), what
        assert np.all(CH.bits(gaps) == CH.SENTINEL), (what, "the rows between the frames")

    def free(self):
        self.be.free(self.owner)


def configure(be, st):
    if st.bin > 1:
        assert be.set_binning(st.bin, st.bin, st.src_x, st.src_y, st.src_mask) == (st.dim_x, st.dim_y)
    be.set_flat_field(st.dark, st.flat, st.t_min)
    info = be.set_defect_map(st.mask)
    assert (info.reach_rows, info.defects) == (st.plan.reach_rows, st.plan.defects)
    be.set_air_region(*st.rect, st.dim_x, st.dim_y, mask=st.mask)
    be.set_zinger_filter(st.zingers[0], st.zingers[1], st.zingers[2], st.dim_x, st.dim_y)
    be.set_beam_hardening(st.bh, st.dim_x, st.dim_y)
    return info.reach_rows


def clear(be):
    be.clear_beam_hardening()
    be.clear_ring_correction()
    be.clear_zinger_filter()
    be.clear_air_region()
    be.clear_defect_map()
    be.clear_flat_field()
    be.clear_binning()


def test_whole_frames_after_every_pass(be, scan, case):
    """the 36 frames in batches of 3 with a frame stride, read back after every pass; the ring correction from ring_profile_* over the
    whole scan, taken after the zinger filter as the driver's pre-pass takes it"""
    st, steps, info = case
    n = len(scan.counts)
    assert n % BATCH == 0
    configure(be, st)
    raw = Frames(be, n, st.src_x, st.src_y)
    dst = Frames(be, n, st.dim_x, st.dim_y) if st.bin > 1 else raw
    at = dict(frame_stride=dst.stride, n_frames=BATCH)
    try:
        for k in range(n):
            be.upload_raw(scan.counts[k], raw.frame(k))                 # u16: widened on the device
        raw.assert_holds(steps[0], "upload_raw")
        if st.bin > 1:
            for k in range(0, n, BATCH):
                be.bin_frames(raw.frame(k), dst.frame(k), src_frame_stride=raw.stride, dst_frame_stride=dst.stride, n_frames=BATCH)
            raw.assert_holds(steps[0], "the source frames are only read")
        dst.assert_holds(steps[1], "bin_frames")
        for k in range(0, n, BATCH):
            be.flat_field_rows(dst.frame(k), **at)
        dst.assert_holds(steps[2], "flat_field_rows")
        be.air_stats(reset=True)
        for k in range(0, n, BATCH):
            be.air_normalize(dst.frame(k), **at)
        dst.assert_holds(steps[3], "air_normalize")
        air = be.air_stats()
        assert (air.frames, air.normalised, air.too_few, air.above_limit) == (n, n, 0, 0)
        assert (air.min_a, air.max_a) == (info.air.min(), info.air.max())
        for k in range(0, n, BATCH):
            be.defect_repair_rows(dst.frame(k), **at)
        dst.assert_holds(steps[4], "defect_repair_rows")
        be.zinger_stats(reset=True)
        for k in range(0, n, BATCH):
            be.zinger_filter_rows(dst.frame(k), **at)
        dst.assert_holds(steps[5], "zinger_filter_rows")
        z = be.zinger_stats()
        assert (z.frames, z.replaced, z.saturated_frames) == (n, sum(info.replaced), 0)
        be.ring_profile_begin(st.dim_x, st.dim_y)
        for k in range(0, n, BATCH):
            be.ring_profile_add_rows(dst.frame(k), **at)
        c, mean, rs = be.ring_profile_finish(*st.rings)
        assert ring_rule.same_means(mean, info.ring_mean) and ring_rule.same_bits(c, info.ring_c) and c.any()
        got_rs = ring_rule.stats_of(rs)
        assert got_rs.pop("max_abs") == np.float32(info.ring_stats["max_abs"])
        assert got_rs == {k: v for k, v in info.ring_stats.items() if k != "max_abs"}
        dst.assert_holds(steps[5], "the profile only reads")
        be.set_ring_correction(c)
        for k in range(0, n, BATCH):
            be.ring_correct_rows(dst.frame(k), **at)
        dst.assert_holds(steps[6], "ring_correct_rows")
        for k in range(0, n, BATCH):
            be.beam_hardening(dst.frame(k), **at)
        dst.assert_holds(steps[7], "beam_hardening")
    finally:
        clear(be)
        raw.free()
        dst.free()


@pytest.mark.parametrize("which", range(len(BAND_NAMES)), ids=BAND_NAMES)
def test_a_band_with_the_driver_s_rows(be, scan, case, which):
    """One batch of 3 frames through the chain with the ranges of chain_rule.band_rows -- the driver's row rule restated --, into frames
    that hold a NaN with a payload everywhere: only the source rows of `up` are uploaded. The band's rows equal the whole-frame chain's;
    outside `up` every row still holds the sentinel; the rows of `up` outside the band are corrected, normalised where the air value is
    subtracted, repaired inside `fix`, and never zinger-filtered, ring-corrected or linearised. Unbinned, the rows come through the
    corrected upload, as in the driver."""
    st, steps, info = case
    first, count = BANDS[st.bin][which]
    reach = configure(be, st)
    be.set_ring_correction(info.ring_c)
    r = CH.band_rows(first, count, st.dim_y, reach, True, st.rect, st.bin)
    rect_rows = (st.rect[1], st.rect[3])
    overlap = r.air[0] < sum(rect_rows) and rect_rows[0] < sum(r.air)
    if BAND_NAMES[which] == "meets_the_rectangle":
        assert overlap and r.up != r.air
    if BAND_NAMES[which] == "clear_of_the_rectangle":
        assert not overlap and r.up[1] > r.air[1] + rect_rows[1] - 1 and r.air[0] > 0 and sum(r.air) < st.dim_y
    edge_pixel = (CH.EDGE_BLOCK[0] + CH.EDGE_BLOCK[1] // 2) // st.bin          # its sources lie `reach` rows above and below it
    assert st.plan.reach_rows == reach and st.mask[edge_pixel - reach + 1:edge_pixel + reach, 0].all()
    assert not st.mask[edge_pixel - reach, 0] and not st.mask[edge_pixel + reach, 0]
    if BAND_NAMES[which] == "defects_at_both_edges":
        assert st.mask[max(0, first - reach):first].any() and st.mask[first + count:first + count + reach].any()
        assert first + count == edge_pixel and edge_pixel + reach < st.dim_y - 1      # the row below the band holds the pixel
    if BAND_NAMES[which] == "whole_reach_above":
        assert first - 1 == edge_pixel and edge_pixel - reach > 0                     # the row above the band holds the pixel
    raw = Frames(be, BATCH, st.src_x, st.src_y)
    dst = Frames(be, BATCH, st.dim_x, st.dim_y) if st.bin > 1 else raw
    at = dict(frame_stride=dst.stride, n_frames=BATCH)
    try:
        for k in range(BATCH):
            be.upload_raw(scan.counts[k][CH.rows(r.src)], raw.frame(k), row_first=r.src[0], corrected=st.bin == 1)
        if st.bin > 1:
            be.bin_frames(raw.frame(0), dst.frame(0), row_first=r.up[0], row_count=r.up[1], src_frame_stride=raw.stride, dst_frame_stride=dst.stride,
                          n_frames=BATCH)
            be.flat_field_rows(dst.frame(0), row_first=r.up[0], row_count=r.up[1], **at)
        be.air_normalize(dst.frame(0), rows=r.air, **at)
        be.defect_repair_rows(dst.frame(0), row_first=r.fix[0], row_count=r.fix[1], **at)
        be.zinger_filter_rows(dst.frame(0), row_first=first, row_count=count, **at)
        be.ring_correct_rows(dst.frame(0), row_first=first, row_count=count, **at)
        be.beam_hardening(dst.frame(0), rows=(first, count), **at)
        want = CH.expected_band([s[:BATCH] for s in steps], r)
        outside = np.ones(st.dim_y, bool)
        outside[CH.rows(r.up)] = False
        assert np.all(CH.bits(want[:, outside]) == CH.SENTINEL) and not np.isnan(want[:, ~outside]).any()
        dst.assert_holds(want, (first, count))
    finally:
        clear(be)
        raw.free()
        dst.free()
