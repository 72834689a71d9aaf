"""paris.hip --scatter on the u16 scan of tests/chain_rule.py with the whole chain in front of it -- --flat --dark
--defects --air-region --zingers --rings -- and --beam-hardening and --detector-roll behind it, against the Python mirror's chain with
Backend.scatter_correction between ring_correct_rows and the phase retrieval, bit for bit: in one slab and in three, frame by frame,
with --phase-alpha behind it, binned. Without the option the volume is the chain's as it was; the refusals print their reason; the
report line gives the setting as the library resolved it."""
import re

import numpy as np
import pytest

import chain_rule as CH
import test_gpu_defect_map as DM
from paris_amd import backend as B
from test_gpu_chain_driver import chain_options, write_scan
from test_gpu_frame_chain import Frames, clear, configure
from test_gpu_phase_driver import ETA, alpha_for, bits, drive, volume_of

pytestmark = pytest.mark.gpu

PHASE_MARGIN = 6
LINE = re.compile(r"^scatter correction on: A (\S+), alpha (\S+), beta (\S+), sigma (\S+) and (\S+) mm \((\S+) x (\S+) and (\S+) x (\S+) px\), "
                  r"weight (\S+), limit (\S+), (\d+) iteration\(s\), margin (\d+), padded (\d+) x (\d+), (\d+) launch\(es\) per round, "
                  r"(\d+) scratch byte\(s\) per device, whole frames \(planned as --no-row-band\)$", re.M)
# A, alpha, beta, sigma1, sigma2, w2 as typed: kernels 3 and 10 pixels of 0.2 mm wide
TYPED = (0.05, -0.15, 1.0, 0.6, 2.0, 0.5)
OPTION = "%.9g:%.9g:%.9g:%.9g:%.9g:%.9g" % TYPED


def setting_for(st, limit=0.8, iterations=4, margin=None, typed=TYPED):
    if margin is None:
        margin = B.scatter_default_margin(typed[3], typed[4], st.geo[2], st.geo[3])
    return typed + (limit, iterations, margin)


ORDER = ("scatter", "phase", "beam_hardening", "roll")


def mirror(s, st, scatter, alpha=None, rings=True, beam_hardening=True, roll=ETA, extend=None, order=ORDER, last=None):
    """the Python mirror's chain on all frames, one call per pass; scatter: the setting or None, alpha: the phase retrieval's or None;
    then the loop -- roll, weight, filter, backproject -- frame by frame. rings, beam_hardening False, roll None: without that pass;
    extend (W, M): the row extension in the filter; order: the passes behind the ring correction in another order, which is another
    rule -- those named behind "roll" run on the resampled frame in the loop; last: scatter, phase and beam_hardening act on the frames
    0 .. last only"""
    n = len(s.counts)
    det = B.DetectorGeometry(*st.geo)
    vg = B.calculate_volume_geometry(det)
    assert sorted(order) == sorted(ORDER)
    passed = n if last is None else last + 1
    with B.Backend(0) as be:

        def run(name, p, **at):
            if name == "scatter" and scatter is not None:
                be.set_scatter_correction(scatter, st.dim_x, st.dim_y, det.l_px_row, det.l_px_col)
                be.scatter_correction(p, **at)
                be.clear_scatter_correction()
            if name == "phase" and alpha is not None:
                be.set_phase_retrieval(alpha, st.t_min, PHASE_MARGIN, st.dim_x, st.dim_y, det.l_px_row, det.l_px_col)
                be.phase_retrieval(p, **at)
                be.clear_phase_retrieval()
            if name == "beam_hardening" and beam_hardening:
                be.set_beam_hardening(st.bh, st.dim_x, st.dim_y)
                be.beam_hardening(p, **at)

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
        if rings:
            be.ring_profile_begin(st.dim_x, st.dim_y)
            be.ring_profile_add_rows(dst.frame(0), **at)
            c, _, _ = be.ring_profile_finish(*st.rings)
            be.set_ring_correction(c)
            be.ring_correct_rows(dst.frame(0), **at)
        for name in order[:order.index("roll")]:
            run(name, dst.frame(0), frame_stride=dst.stride, n_frames=passed)
        frames = dst.read()[0].copy()
        clear(be)
        raw.free()
        if dst is not raw:
            dst.free()
        if roll is not None:
            be.set_detector_roll(roll, det)
        if extend is not None:
            be.set_row_extension(extend[1], extend[0])
        v = be.make_volume_device(vg.dim_x, vg.dim_y, vg.dim_z)
        for i, fr in enumerate(frames):
            d_p, rolled = be.make_projection_device(det.n_row, det.n_col), be.make_projection_device(det.n_row, det.n_col)
            be.upload_raw(np.ascontiguousarray(fr, np.float32), d_p)
            if roll is not None:
                be.detector_roll(d_p, rolled)
            else:
                d_p, rolled = rolled, d_p
            be.free(d_p)
            for name in order[order.index("roll") + 1:] if i < passed else ():
                run(name, rolled)
            rolled.idx = i
            B.weight(be, rolled, det)
            B.filter(be, rolled, det)
            B.backproject(be, rolled, v, 0, det, vg, False, False, None)
            be.free(rolled)
        return DM.volume_to_host(be, v, vg).reshape(vg.dim_z, vg.dim_y, vg.dim_x).copy()


def scan_on_disk(tmp_path_factory, bin_factor):
    root = tmp_path_factory.mktemp("scatter_scan_%d" % bin_factor)
    s = CH.scan()
    st = CH.settings(s, bin_factor)
    write_scan(root, s)
    options = (["--bin", st.bin] if st.bin > 1 else []) + chain_options(root, st) + [
        "--beam-hardening", "%.9g:%.9g" % st.bh, "--detector-roll", "%.9g" % ETA]
    return dict(root=root, s=s, st=st, options=options, want=mirror(s, st, setting_for(st)), plain=mirror(s, st, None))


@pytest.fixture(scope="module")
def given(tmp_path_factory):
    return scan_on_disk(tmp_path_factory, 1)


@pytest.fixture(scope="module")
def binned(tmp_path_factory):
    return scan_on_disk(tmp_path_factory, 2)


def assert_the_line(text, st, setting):
    line = LINE.search(text)
    assert line, text
    n_x, n_y, scratch = B.scatter_correction_check(setting, st.dim_x, st.dim_y, st.geo[2], st.geo[3])
    assert tuple(np.float32(line.group(k)) for k in (1, 2, 3, 4, 5, 10, 11)) == tuple(np.float32(v) for v in setting[:7])
    widths = tuple(float(line.group(k)) for k in (6, 7, 8, 9))
    assert widths == pytest.approx((setting[3] / st.geo[2], setting[3] / st.geo[3], setting[4] / st.geo[2], setting[4] / st.geo[3]), rel=1e-3)
    assert tuple(int(line.group(k)) for k in (12, 13, 14, 15, 16, 17)) == (setting[7], setting[8], n_x, n_y, 2 * setting[7] + 1, scratch)


FORMS = {"slabs_1": ["--slabs", 1], "slabs_3": ["--slabs", 3], "batch_1": ["--slabs", 2, "--batch", 1]}


def assert_equals_the_python_chain(given, form):
    st, root = given["st"], given["root"]
    text = drive(root, form, given["options"] + ["--scatter", OPTION] + FORMS[form])
    got = volume_of(root, form)
    assert np.abs(given["want"]).max() > 0 and not np.array_equal(bits(given["want"]), bits(given["plain"]))
    assert got.shape == given["want"].shape and np.array_equal(bits(got), bits(given["want"])), form
    assert_the_line(text, st, setting_for(st))
    assert "detector roll on" in text and "beam hardening on" in text and "ring filter on" in text
    return text


@pytest.mark.parametrize("form", sorted(FORMS))
def test_scatter_equals_the_python_chain(given, form):
    assert_equals_the_python_chain(given, form)


def test_with_bin_2_the_pitches_and_sizes_are_the_binned_detector_s(binned):
    text = assert_equals_the_python_chain(binned, "slabs_3")
    st = binned["st"]
    assert "binning on: 2 x 2 bins" in text and st.geo[2] == 2 * CH.GEO[2]
    assert setting_for(st)[8] == 15 and B.scatter_correction_check(setting_for(st), st.dim_x, st.dim_y, st.geo[2], st.geo[3])[:2] == (64, 64)


def test_with_the_phase_retrieval_behind_it(given):
    st, root = given["st"], given["root"]
    alpha = alpha_for(st)
    text = drive(root, "phase", given["options"] + ["--scatter", OPTION, "--phase-alpha", "%.9g:%d" % (alpha, PHASE_MARGIN), "--slabs", 2])
    want = mirror(given["s"], st, setting_for(st), alpha)
    assert not np.array_equal(bits(want), bits(given["want"]))
    assert np.array_equal(bits(volume_of(root, "phase")), bits(want))
    assert text.index("scatter correction on") < text.index("phase retrieval on")


def test_one_gaussian_and_the_other_options(given):
    """without the last two fields one Gaussian, W2 = 0 and SIGMA2 = SIGMA1; --scatter-iterations, --scatter-limit, --scatter-margin"""
    st, root = given["st"], given["root"]
    text = drive(root, "one", given["options"] + ["--scatter", "0.3:0.25:0.5:0.6", "--scatter-iterations", 2, "--scatter-limit", "0.05",
                                                  "--scatter-margin", 11, "--slabs", 2])
    setting = setting_for(st, 0.05, 2, 11, (0.3, 0.25, 0.5, 0.6, 0.6, 0.0))
    assert_the_line(text, st, setting)
    want = mirror(given["s"], st, setting)
    assert not np.array_equal(bits(want), bits(given["want"])) and np.array_equal(bits(volume_of(root, "one")), bits(want))


def test_without_the_option_nothing_changes(given):
    text = drive(given["root"], "plain", given["options"] + ["--slabs", 3])
    assert "scatter correction on" not in text
    assert np.array_equal(bits(volume_of(given["root"], "plain")), bits(given["plain"]))


USAGE = "--scatter A:ALPHA:BETA:SIGMA1_MM[:SIGMA2_MM:W2]"


@pytest.mark.parametrize("extra,words", [
    (["--scatter", "0.05:-0.15:1"], "cannot read"),
    (["--scatter", "0.05:-0.15:1:0.6:2"], "cannot read"),
    (["--scatter", "0.05:-0.15:1:0.6:2:0.5:1"], "cannot read"),
    (["--scatter", "much:-0.15:1:0.6"], "cannot read"),
    (["--scatter", "0:-0.15:1:0.6"], USAGE + ": A and the widths must be finite and greater than 0"),
    (["--scatter", "nan:-0.15:1:0.6"], USAGE + ": A and the widths must be finite and greater than 0"),
    (["--scatter", "0.05:-2.5:1:0.6"], "ALPHA must lie in [-2, 2]"),
    (["--scatter", "0.05:-0.15:4.5:0.6"], "BETA in [0, 4]"),
    (["--scatter", "0.05:-0.15:1:0"], "the widths must be finite and greater than 0"),
    (["--scatter", "0.05:-0.15:1:0.6:inf:0.5"], "the widths must be finite and greater than 0"),
    (["--scatter", "0.05:-0.15:1:0.6:2:-1"], "W2 must be finite and not negative"),
    (["--scatter", OPTION, "--scatter-iterations", "0"], "N must lie in 1 .. 16"),
    (["--scatter", OPTION, "--scatter-iterations", "17"], "N must lie in 1 .. 16"),
    (["--scatter", OPTION, "--scatter-iterations", "2.5"], "cannot read"),
    (["--scatter", OPTION, "--scatter-limit", "0"], "F must lie in (0, 1)"),
    (["--scatter", OPTION, "--scatter-limit", "1"], "F must lie in (0, 1)"),
    (["--scatter", OPTION, "--scatter-limit", "nan"], "F must lie in (0, 1)"),
    (["--scatter", OPTION, "--scatter-margin", "0"], "M must lie in 1 .. 1024"),
    (["--scatter", OPTION, "--scatter-margin", "1025"], "the margin must lie in 1 .. 1024"),
    (["--scatter", OPTION, "--scatter-margin", "-3"], "cannot read"),
    (["--scatter-iterations", "3"], "need --scatter"),
    (["--scatter-limit", "0.5"], "need --scatter"),
    (["--scatter-margin", "12"], "need --scatter"),
])
def test_refusals(given, extra, words):
    err = drive(given["root"], "refused", given["options"] + extra, ok=False)
    assert words in err, err
