"""paris.hip --starvation on the u16 scan of tests/chain_rule.py with the whole chain in front of it -- --flat
--dark --defects --air-region --zingers --rings -- and --beam-hardening and --detector-roll behind it, against the Python mirror's chain
with Backend.starvation_filter between ring_correct_rows and the scatter correction, bit for bit: in one slab and in three, frame by
frame, with --scatter behind it. Without the option, and with a p0 above every pixel, the volume is the chain's as it was; the report
line gives the setting and the counts; the refusals print their reason."""
import re

import numpy as np
import pytest

import chain_rule as CH
import test_gpu_defect_map as DM
from paris_amd import backend as B
from test_gpu_chain_driver import chain_options, write_scan
from test_gpu_frame_chain import Frames, clear, configure
from test_gpu_phase_driver import ETA, bits, drive, volume_of
from test_gpu_scatter_driver import OPTION as SCATTER_OPTION
from test_gpu_scatter_driver import setting_for as scatter_setting_for

pytestmark = pytest.mark.gpu

LINE = re.compile(r"^starvation filter on: p0 (\S+), gain (\S+), radius (\d+), (\d+) pixel\(s\) filtered of (\d+) in (\d+) frame\(s\) \((\S+) %\), "
                  r"(\S+) % of them at the last level, whole frames \(planned as --no-row-band\)$", re.M)
SETTING = (1.25, 1.5, 3)              # the scan's line integrals reach 2.5: the levels go up to 20
OPTION = "%.9g:%.9g:%d" % SETTING


def mirror(s, st, starvation, scatter=None, beam_hardening=True, roll=ETA, after_scatter=False, stats=None):
    """the Python mirror's chain on all frames, one call per pass -- starvation: the setting or None, between the ring correction and
    the scatter correction (after_scatter: behind it, which is another rule) --, then the loop -- roll, weight, filter, backproject --
    frame by frame. stats: a list that receives the filter's counts."""
    n = len(s.counts)
    det = B.DetectorGeometry(*st.geo)
    vg = B.calculate_volume_geometry(det)
    with B.Backend(0) as be:
        configure(be, st)
        raw = Frames(be, n, st.src_x, st.src_y)
        dst = Frames(be, n, st.dim_x, st.dim_y) if st.bin > 1 else raw
        at = dict(frame_stride=dst.stride, n_frames=n)
        for k in range(n):
            be.upload_raw(s.counts[k], raw.frame(k))
        if st.bin > 1:
            be.bin_frames(raw.frame(0), dst.frame(0), src_frame_stride=raw.stride, dst_frame_stride=dst.stride, n_frames=n)
        be.flat_field_rows(dst.frame(0), **at)
        be.air_normalize(dst.frame(0), **at)
        be.defect_repair_rows(dst.frame(0), **at)
        be.zinger_filter_rows(dst.frame(0), **at)
        be.ring_profile_begin(st.dim_x, st.dim_y)
        be.ring_profile_add_rows(dst.frame(0), **at)
        c, _, _ = be.ring_profile_finish(*st.rings)
        be.set_ring_correction(c)
        be.ring_correct_rows(dst.frame(0), **at)

        def starve():
            if starvation is not None:
                be.set_starvation_filter(starvation, st.dim_x, st.dim_y)
                be.starvation_filter(dst.frame(0), **at)
                if stats is not None:
                    stats.append(be.starvation_stats())
                be.clear_starvation_filter()

        if not after_scatter:
            starve()
        if scatter is not None:
            be.set_scatter_correction(scatter, st.dim_x, st.dim_y, det.l_px_row, det.l_px_col)
            be.scatter_correction(dst.frame(0), **at)
            be.clear_scatter_correction()
        if after_scatter:
            starve()
        if beam_hardening:
            be.set_beam_hardening(st.bh, st.dim_x, st.dim_y)
            be.beam_hardening(dst.frame(0), **at)
        frames = dst.read()[0].copy()
        clear(be)
        raw.free()
        if dst is not raw:
            dst.free()
        if roll is not None:
            be.set_detector_roll(roll, det)
        v = be.make_volume_device(vg.dim_x, vg.dim_y, vg.dim_z)
        for i, fr in enumerate(frames):
            d_p, rolled = be.make_projection_device(det.n_row, det.n_col), be.make_projection_device(det.n_row, det.n_col)
            be.upload_raw(np.ascontiguousarray(fr, np.float32), d_p)
            if roll is not None:
                be.detector_roll(d_p, rolled)
            else:
                d_p, rolled = rolled, d_p
            be.free(d_p)
            rolled.idx = i
            B.weight(be, rolled, det)
            B.filter(be, rolled, det)
            B.backproject(be, rolled, v, 0, det, vg, False, False, None)
            be.free(rolled)
        return DM.volume_to_host(be, v, vg).reshape(vg.dim_z, vg.dim_y, vg.dim_x).copy()


def scan_on_disk(tmp_path_factory, bin_factor):
    root = tmp_path_factory.mktemp("starvation_scan_%d" % bin_factor)
    s = CH.scan()
    st = CH.settings(s, bin_factor)
    write_scan(root, s)
    options = (["--bin", st.bin] if st.bin > 1 else []) + chain_options(root, st) + [
        "--beam-hardening", "%.9g:%.9g" % st.bh, "--detector-roll", "%.9g" % ETA]
    stats = []
    want = mirror(s, st, SETTING, stats=stats)
    return dict(root=root, s=s, st=st, options=options, want=want, counts=stats[0], plain=mirror(s, st, None))


@pytest.fixture(scope="module")
def given(tmp_path_factory):
    return scan_on_disk(tmp_path_factory, 1)


@pytest.fixture(scope="module")
def binned(tmp_path_factory):
    return scan_on_disk(tmp_path_factory, 2)


def assert_the_line(text, st, setting, counts, slabs):
    """the counts are the Python chain's, once per slab: every slab filters every frame whole"""
    line = LINE.search(text)
    assert line, text
    assert tuple(np.float32(line.group(k)) for k in (1, 2)) == tuple(np.float32(v) for v in setting[:2]) and int(line.group(3)) == setting[2]
    n_filtered, n_pixels, n_frames = (int(line.group(k)) for k in (4, 5, 6))
    assert (n_filtered, n_frames) == (slabs * counts.filtered, slabs * counts.frames)
    assert n_pixels == n_frames * st.dim_x * st.dim_y
    assert float(line.group(7)) == pytest.approx(100.0 * n_filtered / n_pixels, rel=1e-3)
    assert float(line.group(8)) == pytest.approx(100.0 * counts.last_level / max(1, counts.filtered), rel=1e-3, abs=1e-12)


FORMS = {"slabs_1": (["--slabs", 1], 1), "slabs_3": (["--slabs", 3], 3), "batch_1": (["--slabs", 2, "--batch", 1], 2)}


def assert_equals_the_python_chain(given, form):
    st, root = given["st"], given["root"]
    text = drive(root, form, given["options"] + ["--starvation", OPTION] + FORMS[form][0])
    got = volume_of(root, form)
    assert np.abs(given["want"]).max() > 0 and not np.array_equal(bits(given["want"]), bits(given["plain"]))
    assert got.shape == given["want"].shape and np.array_equal(bits(got), bits(given["want"])), form
    assert 0.02 * st.dim_x * st.dim_y * CH.N_FRAMES < given["counts"].filtered
    assert_the_line(text, st, SETTING, given["counts"], FORMS[form][1])
    assert "detector roll on" in text and "beam hardening on" in text and "ring filter on" in text and "zinger filter on" in text
    return text


@pytest.mark.parametrize("form", sorted(FORMS))
def test_starvation_equals_the_python_chain(given, form):
    assert_equals_the_python_chain(given, form)


def test_with_bin_2_the_size_is_the_binned_detector_s(binned):
    text = assert_equals_the_python_chain(binned, "slabs_3")
    assert "binning on: 2 x 2 bins" in text and (binned["st"].dim_x, binned["st"].dim_y) == (33, 22)


def test_with_the_scatter_correction_behind_it(given):
    st, root = given["st"], given["root"]
    text = drive(root, "scatter", given["options"] + ["--starvation", OPTION, "--scatter", SCATTER_OPTION, "--slabs", 2])
    scatter = scatter_setting_for(st)
    want = mirror(given["s"], st, SETTING, scatter=scatter)
    assert not np.array_equal(bits(want), bits(given["want"]))
    assert not np.array_equal(bits(want), bits(mirror(given["s"], st, SETTING, scatter=scatter, after_scatter=True)))
    assert np.array_equal(bits(volume_of(root, "scatter")), bits(want))
    assert text.index("starvation filter on") < text.index("scatter correction on")


def test_the_defaults_and_another_radius(given):
    """P0 alone: GAIN 1 and RADIUS 3; P0:GAIN:RADIUS with radius 1"""
    st, root = given["st"], given["root"]
    for out, option, setting in (("defaults", "1.5", (1.5, 1.0, 3)), ("radius_1", "1:0.5:1", (1.0, 0.5, 1))):
        text = drive(root, out, given["options"] + ["--starvation", option, "--slabs", 2])
        stats = []
        want = mirror(given["s"], st, setting, stats=stats)
        assert not np.array_equal(bits(want), bits(given["want"])) and np.array_equal(bits(volume_of(root, out)), bits(want))
        assert_the_line(text, st, setting, stats[0], 2)


def test_without_the_option_nothing_changes(given):
    text = drive(given["root"], "plain", given["options"] + ["--slabs", 3])
    assert "starvation filter on" not in text
    assert np.array_equal(bits(volume_of(given["root"], "plain")), bits(given["plain"]))


def test_a_p0_above_every_pixel_changes_nothing_and_says_so(given):
    text = drive(given["root"], "high", given["options"] + ["--starvation", "50", "--slabs", 3])
    line = LINE.search(text)
    assert line and int(line.group(4)) == 0 and int(line.group(6)) == 3 * CH.N_FRAMES and float(line.group(7)) == 0.0
    assert np.array_equal(bits(volume_of(given["root"], "high")), bits(given["plain"]))


USAGE = "--starvation P0[:GAIN[:RADIUS]]"


@pytest.mark.parametrize("extra,words", [
    (["--starvation", "1.5:"], "cannot read"),
    (["--starvation", "1.5:1:3:4"], "cannot read"),
    (["--starvation", "much"], "cannot read"),
    (["--starvation", "1.5:1:3.5"], "cannot read"),
    (["--starvation", "nan"], USAGE + ": P0 must be finite"),
    (["--starvation", "inf:1"], USAGE + ": P0 must be finite"),
    (["--starvation", "1.5:0"], "GAIN finite and greater than 0"),
    (["--starvation", "1.5:-1"], "GAIN finite and greater than 0"),
    (["--starvation", "1.5:inf"], "GAIN finite and greater than 0"),
    (["--starvation", "1.5:1:0"], "RADIUS must lie in 1 .. 4"),
    (["--starvation", "1.5:1:5"], "RADIUS must lie in 1 .. 4"),
    (["--starvation", OPTION, "--find-axis", "-1:1", "--axis-only"], "cannot be combined with --axis-only or --roll-only"),
    (["--starvation", OPTION, "--find-roll", "-1:1", "--roll-only"], "cannot be combined with --axis-only or --roll-only"),
])
def test_refusals(given, extra, words):
    err = drive(given["root"], "refused", given["options"] + extra, ok=False)
    assert words in err, err
