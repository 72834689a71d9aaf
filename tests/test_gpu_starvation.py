"""The starvation filter on the device: paris_hip_starvation_filter_frames against the host rule
(paris_hip_starvation_filter_host, which tests/test_starvation_host.py holds to the numpy restatement), bit for bit on the same inputs --
canvases with sentinels around rows and frames, aligned and misaligned bases, strides, more frames than a launch serves, a shape past the
grid cap, tile corners --, the counts, a frame's bits whatever shares its call, the contracts of a frame pass and of a ctx-owned
setting, the C++ mirror's paris::weight() with the setting, and the physical check of tests/starvation_scene.py on the device."""
import numpy as np
import pytest

import chain_rule as CH
import starvation_rule as R
import starvation_scene as SC
import test_gpu_defect_map as DM
import test_gpu_detector_roll as DR
from paris_amd import _lib
from paris_amd import backend as B

pytestmark = pytest.mark.gpu

bits, read, pending = DM.bits, DM.read, DM.pending
INV = _lib.ERROR_INVALID_ARGUMENT
FRAMES_MAX = _lib.STARVATION_FRAMES_MAX
GRID_CAP = 1024                       # ST_GRID_MAX of starvation.hip: workgroups of one launch; a workgroup walks 64 x 16 tiles
GAIN = 1.0


@pytest.fixture(scope="module")
def be():
    with B.Backend(0) as b:
        yield b
        b.clear_starvation_filter()


def host(frame, radius, p0=R.P0, gain=GAIN):
    return B.starvation_filter_host((p0, gain, radius), frame)


def refused(code, f, *args, **kw):
    with pytest.raises(B.ParisHipError) as e:
        f(*args, **kw)
    return e.value.status == code


def same(got, want):
    return got.shape == want.shape and np.array_equal(bits(got), bits(want))


def filtered(be, frames, layout=DR.ALIGNED, n_frames=None):
    """the frames in a canvas of sentinels at this layout, filtered by one call (the setting is in place): the frames read back, after
    the check that every byte outside them -- and every frame beyond n_frames -- is as it went"""
    dim_y, dim_x = frames[0].shape
    n = len(frames)
    off, pitch, stride, n_bytes = layout(n, dim_x, dim_y)
    host_canvas = np.full(((n_bytes + 255) // 256) * 64, DR.SENTINEL, np.uint32).view(np.float32)
    inside = np.zeros(host_canvas.size, bool)
    for k in range(n):
        DR.place(host_canvas, off + k * stride, pitch, frames[k])
        if n_frames is None or k < n_frames:
            for y in range(dim_y):
                at = (off + k * stride + y * pitch) // 4
                inside[at:at + dim_x] = True
    canvas = DR.Canvas(be, n_bytes, host_canvas.copy())
    be.starvation_filter(canvas.view(off, pitch, dim_x, dim_y), stride, n if n_frames is None else n_frames)
    got = canvas.read()
    canvas.free()
    assert np.array_equal(bits(got)[~inside], bits(host_canvas)[~inside]), "outside the frames"
    out = []
    for k in range(n):
        rows = [got[(off + k * stride + y * pitch) // 4:(off + k * stride + y * pitch) // 4 + dim_x] for y in range(dim_y)]
        out.append(np.stack(rows))
    return out


def counts_of(be):
    c = be.starvation_stats(reset=True)
    return c.frames, c.filtered, c.last_level


def host_counts(frames, radius):
    got = [host(f, radius)[1] for f in frames]
    return len(frames), sum(c.filtered for c in got), sum(c.last_level for c in got)


# ---- 1. the rule, bit for bit --------------------------------------------------------------------------------------------------------

LAYOUTS = {"aligned": DR.ALIGNED, "aligned_wide": DR.ALIGNED_WIDE, "scalar": DR.SCALAR, "scalar_wide": DR.SCALAR_WIDE}


@pytest.mark.parametrize("radius", (1, 2, 3, 4))
@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "%dx%d" % s)
def test_the_device_gives_the_host_rule_s_bits(be, shape, radius):
    """three frames with a stride in one call, in an aligned canvas and in one whose base is 4 bytes off; the counts are the host's"""
    dim_x, dim_y = shape
    frames = [R.frame(dim_x, dim_y, 11 + R.SHAPES.index(shape)), R.below(dim_x, dim_y, 5), R.frame(dim_x, dim_y, 77)]
    want = [host(f, radius)[0] for f in frames]
    assert same(want[1], frames[1]) and (dim_x * dim_y < 64 * 3 or not same(want[0], frames[0]))
    be.set_starvation_filter((R.P0, GAIN, radius), dim_x, dim_y)
    for name in ("aligned", "scalar"):
        got = filtered(be, frames, LAYOUTS[name])
        for k in range(3):
            assert same(got[k], want[k]), (name, k)
        assert counts_of(be) == host_counts(frames, radius), name


@pytest.mark.parametrize("name", sorted(LAYOUTS))
def test_every_byte_outside_the_frames_comes_back_as_it_went(be, name):
    dim_x, dim_y = 65, 17
    frames = [R.frame(dim_x, dim_y, 3), R.frame(dim_x, dim_y, 4), R.frame(dim_x, dim_y, 6)]
    be.set_starvation_filter((R.P0, 0.5, 3), dim_x, dim_y)
    got = filtered(be, frames, LAYOUTS[name])           # (the check of the canvas is in there)
    for k in range(3):
        assert same(got[k], host(frames[k], 3, gain=0.5)[0]), k
    # n_frames 1 and 2 of three: the frames beyond stay as they were
    for n in (1, 2):
        got = filtered(be, frames, LAYOUTS[name], n_frames=n)
        assert same(got[0], host(frames[0], 3, gain=0.5)[0]) and all(same(got[k], frames[k]) for k in range(n, 3))


def test_more_frames_than_one_launch_serves(be):
    """2 FRAMES_MAX + 3 frames of 61 x 7 in one call: the scratch holds FRAMES_MAX, the call loops three times"""
    dim_x, dim_y = 61, 7
    n = 2 * FRAMES_MAX + 3
    frames = [R.frame(dim_x, dim_y, 100 + k) for k in range(n)]
    be.set_starvation_filter((R.P0, GAIN, 2), dim_x, dim_y)
    counts_of(be)
    got = filtered(be, frames, DR.SCALAR_WIDE)
    for k in range(n):
        assert same(got[k], host(frames[k], 2)[0]), k
    assert counts_of(be) == host_counts(frames, 2)


def test_a_shape_past_the_grid_cap(be):
    """4 frames of 4100 rows x 5 pixels: 4 x 257 tiles of 64 x 16 = 1028 work items for at most 1024 workgroups, so the first four
    workgroups come round a second time -- for the last tiles of the last frame"""
    dim_x, dim_y = 5, 4100
    assert 4 * ((dim_y + 15) // 16) * ((dim_x + 63) // 64) == GRID_CAP + 4
    frames = [R.frame(dim_x, dim_y, 200 + k) for k in range(4)]
    for f in frames:
        f[-40:] = np.float32(R.P0 + 0.2) + f[-40:] % np.float32(0.5)          # the second visit's rows: every pixel is filtered
    want = [host(f, 3)[0] for f in frames]
    assert not same(want[3][-40:], frames[3][-40:])
    be.set_starvation_filter((R.P0, GAIN, 3), dim_x, dim_y)
    counts_of(be)
    got = filtered(be, frames, DR.SCALAR)
    for k in range(4):
        assert same(got[k], want[k]), k
    assert counts_of(be) == host_counts(frames, 3)


def test_frames_whose_only_filtered_pixel_sits_on_a_tile_corner(be):
    """130 x 33: tiles of 64 x 16 start at x = 0, 64, 128 and y = 0, 16, 32. One pixel above p0 per frame, on each side of those
    corners; everything else below p0 and finite, so the pixel becomes a mean that needs the neighbouring tiles' pixels"""
    dim_x, dim_y = 130, 33
    spots = [(0, 0), (15, 63), (15, 64), (16, 63), (16, 64), (31, 127), (31, 128), (32, 127), (32, 128), (32, 129), (0, 129), (16, 0)]
    rng = np.random.default_rng(8)
    frames = []
    for y, x in spots:
        f = (R.P0 - 0.1 - 2.0 * rng.random((dim_y, dim_x))).astype(np.float32)
        f[y, x] = np.float32(R.P0 + 2.0)
        frames.append(f)
    for radius in (1, 4):
        want = [host(f, radius)[0] for f in frames]
        be.set_starvation_filter((R.P0, GAIN, radius), dim_x, dim_y)
        counts_of(be)
        got = filtered(be, frames, DR.SCALAR)
        for k, (y, x) in enumerate(spots):
            assert same(got[k], want[k]), (radius, y, x)
            assert want[k][y, x] != frames[k][y, x] and np.count_nonzero(bits(want[k]) != bits(frames[k])) == 1
        assert counts_of(be) == (len(spots), len(spots), 0)


def test_a_frame_s_bits_do_not_depend_on_its_company(be):
    dim_x, dim_y = 65, 17
    a, b, c = R.frame(dim_x, dim_y, 1), R.frame(dim_x, dim_y, 2), R.below(dim_x, dim_y, 3)
    be.set_starvation_filter((R.P0, 2.0, 2), dim_x, dim_y)
    alone, = filtered(be, [a])
    assert same(alone, host(a, 2, gain=2.0)[0]) and not same(alone, a)
    for frames, at in (([a, b, c], 0), ([b, a, c], 1), ([c, b, a], 2), ([a] * (FRAMES_MAX + 1), FRAMES_MAX)):
        assert same(filtered(be, frames, DR.SCALAR)[at], alone), at


def test_the_counts_accumulate_and_reset(be):
    dim_x, dim_y = 64, 16
    f = R.frame(dim_x, dim_y, 9)
    be.set_starvation_filter((R.P0, GAIN, 3), dim_x, dim_y)
    assert counts_of(be) == (0, 0, 0)
    one = host_counts([f], 3)
    assert one[1] > 0 and 0 < one[2] < one[1]
    filtered(be, [f])
    filtered(be, [f, f])
    c = be.starvation_stats()
    assert (c.frames, c.filtered, c.last_level) == tuple(3 * v for v in one)
    assert counts_of(be) == tuple(3 * v for v in one) and counts_of(be) == (0, 0, 0)


# ---- 2. contracts --------------------------------------------------------------------------------------------------------------------

def test_the_refusals(be):
    be.set_starvation_filter((R.P0, GAIN, 3), 61, 45)
    d, other = be.make_projection_device(61, 45), be.make_projection_device(60, 45)
    be.starvation_filter(d)
    assert refused(INV, be.starvation_filter, other)
    assert refused(INV, be.starvation_filter, be.wrap_projection(d.ptr, d.pitch, 61, 44))
    assert refused(INV, be.starvation_filter, be.wrap_projection(d.ptr, 61 * 4 - 4, 61, 45))
    assert refused(INV, be.starvation_filter, d, 45 * d.pitch - 4, 2)
    for bad in ((np.nan, 1.0, 3), (np.inf, 1.0, 3), (3.0, 0.0, 3), (3.0, -1.0, 3), (3.0, np.inf, 3), (3.0, 1.0, 0), (3.0, 1.0, 5)):
        assert refused(INV, be.set_starvation_filter, bad, 61, 45), bad
    assert refused(INV, be.set_starvation_filter, (3.0, 1.0, 3), 0, 45)
    be.starvation_filter(d)                        # a refused setting leaves the one in place
    be.clear_starvation_filter()
    assert refused(INV, be.starvation_filter, d)
    assert refused(INV, be.starvation_stats)
    be.free(d)
    be.free(other)


def test_the_reserve_counts_the_setting_and_a_set_clear_set_cycle_behaves():
    f = R.frame(61, 45, 2)
    with B.Backend(0) as b:
        without = b.projection_reserve_bytes(61, 45)
        b.set_starvation_filter((R.P0, GAIN, 3), 61, 45)
        assert b.projection_reserve_bytes(61, 45) == without + B.starvation_filter_check((R.P0, GAIN, 3), 61, 45)
        first, = filtered(b, [f])
        b.set_starvation_filter((R.P0, GAIN, 1), 5, 3)                        # replaced: the old buffer leaves the reserve
        assert b.projection_reserve_bytes(61, 45) == without + B.starvation_filter_check((R.P0, GAIN, 1), 5, 3)
        b.clear_starvation_filter()
        assert b.projection_reserve_bytes(61, 45) == without
        b.clear_starvation_filter()                                           # clearing nothing is allowed
        b.set_starvation_filter((R.P0, GAIN, 3), 61, 45)
        assert counts_of(b) == (0, 0, 0)                                      # a new setting counts from zero
        again, = filtered(b, [f])
        assert same(again, first) and same(first, host(f, 3)[0])
        b.clear_starvation_filter()
        assert b.projection_reserve_bytes(61, 45) == without


def test_a_replaced_setting_leaves_queued_work_on_the_old_one(be):
    dim_x, dim_y = 130, 33
    f = R.frame(dim_x, dim_y, 16)
    want = host(f, 4)[0]
    with B.Backend(0, synchronous=False) as abe:
        abe.set_starvation_filter((R.P0, GAIN, 4), dim_x, dim_y)
        d = [abe.make_projection_device(dim_x, dim_y) for _ in range(4)]
        for x in d:
            abe.upload_raw(f, x)
        for x in d:
            abe.starvation_filter(x)                                          # queued ...
        abe.set_starvation_filter((R.P0 + 1.0, 0.5, 1), dim_x, dim_y)          # ... while the setting is replaced
        abe.clear_starvation_filter()
        for x in d:
            assert same(read(abe, x), want)


ORD_GEO = DM.ORD_GEO
ORD_X, ORD_Y = ORD_GEO[:2]
ORD_FRAME = np.random.default_rng(9).uniform(0.0, 2.0, (ORD_Y, ORD_X)).astype(np.float32)
ORD_SETTING = (1.0, 1.0, 3)


def test_a_held_back_weighting_is_flushed_first():
    det = B.DetectorGeometry(*ORD_GEO)

    def run(fusion):
        with B.Backend(0, synchronous=False) as abe:
            abe.set_stage_fusion(fusion)
            abe.set_starvation_filter(ORD_SETTING, ORD_X, ORD_Y)
            d = B.load(abe, B.Projection(ORD_FRAME.copy(), ORD_X, ORD_Y, idx=2))
            B.weight(abe, d, det)               # with fusion: held back until something touches the frame
            abe.starvation_filter(d)
            return read(abe, d)

    plain, fused = run(False), run(True)
    assert same(fused, plain)
    unweighted = B.starvation_filter_host(ORD_SETTING, ORD_FRAME)[0]
    assert not same(plain, unweighted)


@pytest.mark.parametrize("by_reference", [False, True])
def test_a_frame_of_the_pending_group_is_backprojected_as_it_was(by_reference):
    """Filtering in a buffer the pending by-reference group refers to launches that group first: the volume is the one the snapshot
    path gives. With snapshots the group stays pending."""
    det = B.DetectorGeometry(*ORD_GEO)
    vg = B.calculate_volume_geometry(det)

    def run(deferred):
        with B.Backend(0, synchronous=False) as abe:
            if deferred:
                abe.set_backproject_deferral(8)
                abe.set_backproject_references(by_reference)
            abe.set_starvation_filter(ORD_SETTING, ORD_X, ORD_Y)
            d = B.load(abe, B.Projection(ORD_FRAME.copy(), ORD_X, ORD_Y, idx=1))
            v = abe.make_volume_device(vg.dim_x, vg.dim_y, vg.dim_z)
            B.backproject(abe, d, v, 0, det, vg, False, False, None)
            if deferred:
                assert pending(abe) == 1
            abe.starvation_filter(d)
            if deferred:
                assert pending(abe) == (0 if by_reference else 1)
            return read(abe, d), DM.volume_to_host(abe, v, vg)

    want_p, want_v = run(False)
    got_p, got_v = run(True)
    assert np.abs(want_v).max() > 0 and not same(want_p, ORD_FRAME)
    assert same(got_v, want_v) and same(got_p, want_p)
    assert same(want_p, B.starvation_filter_host(ORD_SETTING, ORD_FRAME)[0])


# ---- 3. the C++ mirror ---------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def mirror_scan(tmp_path_factory):
    import test_gpu_cpp_mirror_stages as MS
    import test_gpu_starvation_driver as SD
    root = tmp_path_factory.mktemp("starvation_mirror")
    s = CH.scan()
    st = CH.settings(s, 1)
    st.mask = (s.mask != 0).astype(np.uint8)
    st.plan = B.defect_plan(st.mask)
    MS.write_scan(root, s)
    s.counts.astype(np.float32).tofile(root / "in.raw")
    MS.write_settings(root, st)
    return dict(root=root, s=s, st=st, MS=MS, SD=SD)


@pytest.mark.parametrize("slabs", [1, 3])
def test_the_cpp_mirror_s_weight_runs_the_pass_between_the_rings_and_the_scatter_correction(mirror_scan, slabs):
    """paris_hip_demo --flat --air-region --defects --zingers --rings --starvation --scatter --beam-hardening: the Python chain with
    Backend.starvation_filter between ring_correct_rows and scatter_correction, bit for bit; with the pass behind the scatter
    correction instead, and without it, the volume is another one"""
    MS, SD, st, s, root = (mirror_scan[k] for k in ("MS", "SD", "st", "s", "root"))
    scatter = MS.setting_for(st)
    want = SD.mirror(s, st, SD.SETTING, scatter=scatter, roll=None)
    assert np.abs(want).max() > 0
    assert not same(SD.mirror(s, st, None, scatter=scatter, roll=None), want)
    assert not same(SD.mirror(s, st, SD.SETTING, scatter=scatter, roll=None, after_scatter=True), want)
    flags = (MS.chain_flags(root, st) + ["--starvation"] + ["%.9g" % v for v in SD.SETTING[:2]] + [SD.SETTING[2]] + MS.scatter_flags(scatter)
             + MS.bh_flags(st) + ["--slabs", slabs])
    got = MS.demo(root, CH.GEO, CH.N_FRAMES, "in.raw", "s.raw", flags)
    assert got.size == want.size and same(got.reshape(want.shape), want)


def test_the_cpp_mirror_refuses_what_the_library_refuses(mirror_scan):
    MS, st, root = (mirror_scan[k] for k in ("MS", "st", "root"))
    err = MS.demo(root, CH.GEO, CH.N_FRAMES, "in.raw", "refused.raw", MS.chain_flags(root, st) + ["--starvation", "1.5", "1", 5], ok=False)
    assert "set_starvation_filter()" in err and MS.INVALID in err


# ---- 4. the physical check -----------------------------------------------------------------------------------------------------------

def test_starved_rays_leave_fewer_streaks(be):
    """The scene of tests/starvation_scene.py filtered on the device in one call and reconstructed by the float64 model: the ratio of
    the RMS differences to the noise-free reconstruction keeps the bound that tests/test_starvation_scene_host.py states, and so do the
    conditions that keep the check honest"""
    sc = SC.scene()
    be.set_starvation_filter(SC.SETTING, sc.det.n_row, sc.det.n_col)
    counts_of(be)
    got = np.stack(filtered(be, list(sc.noisy), DR.ALIGNED))
    frames, n_filtered, n_last = counts_of(be)
    want = np.stack([B.starvation_filter_host(SC.SETTING, f)[0] for f in sc.noisy])
    assert same(got, want)
    share = n_filtered / sc.noisy.size
    print("starvation scene on the device: %d of %d pixels filtered (%.4g), %d at the last level (%.4g of them)"
          % (n_filtered, sc.noisy.size, share, n_last, n_last / max(1, n_filtered)))
    assert frames == len(sc.noisy) and SC.SHARE_MIN <= share <= SC.SHARE_MAX and n_last < 0.5 * n_filtered
    before, after, far = SC.measure(sc, got)
    print("starvation scene on the device: unfiltered %.4g, filtered %.4g, ratio %.4g, far region changes by %.4g" % (before, after, after / before, far))
    assert after / before <= SC.RATIO_BOUND
    assert far <= SC.FAR_BOUND
