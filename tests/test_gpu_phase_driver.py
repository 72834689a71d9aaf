"""paris.hip --phase / --phase-alpha on the u16 scan of tests/chain_rule.py with the whole chain in front of it --
--flat --dark --defects --air-region --zingers --rings -- and --beam-hardening and --detector-roll behind it, against the Python mirror's
chain with Backend.phase_retrieval between ring_correct_rows and beam_hardening, bit for bit: in one slab and in three, frame by frame,
binned, on two devices where the machine has them. --phase D:E is --phase-alpha of phase_alpha(D, E); without the option the volume is
the chain's as it was; the refusals print their reason."""
import re
import subprocess

import numpy as np
import pytest

import chain_rule as CH
import test_gpu_defect_map as DM
import test_gpu_paris_hip as P
from oracle import formats as F
from paris_amd import backend as B
from test_gpu_chain_driver import chain_options, write_scan
from test_gpu_frame_chain import Frames, clear, configure

pytestmark = pytest.mark.gpu

ETA = 0.8
MARGIN = 6
LINE = re.compile(r"^phase retrieval on: alpha (\S+) mm\^2, kernel length (\S+) x (\S+) px, margin (\d+), floor (\S+), padded (\d+) x (\d+), "
                  r"(\d+) scratch byte\(s\) per device, whole frames \(planned as --no-row-band\)$", re.M)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def alpha_for(st):
    """a kernel length of 0.4 pixels: sqrt(alpha) / 2 pi = 0.4 l"""
    return float(np.float32((0.4 * 2.0 * np.pi * st.geo[2]) ** 2))


def mirror(s, st, alpha, margin=MARGIN, t_min=None):
    """the Python mirror's chain on all frames, one call per pass, alpha None: without the phase retrieval; then the loop -- roll,
    weight, filter, backproject -- frame by frame"""
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
        if alpha is not None:
            be.set_phase_retrieval(alpha, st.t_min if t_min is None else t_min, margin, st.dim_x, st.dim_y, det.l_px_row, det.l_px_col)
            be.phase_retrieval(dst.frame(0), **at)
            be.clear_phase_retrieval()
        be.beam_hardening(dst.frame(0), **at)
        frames = dst.read()[0].copy()
        clear(be)
        raw.free()
        if dst is not raw:
            dst.free()
        be.set_detector_roll(ETA, det)
        v = be.make_volume_device(vg.dim_x, vg.dim_y, vg.dim_z)
        for i, fr in enumerate(frames):
            d_p, rolled = be.make_projection_device(det.n_row, det.n_col), be.make_projection_device(det.n_row, det.n_col)
            be.upload_raw(np.ascontiguousarray(fr, np.float32), d_p)
            be.detector_roll(d_p, rolled)
            be.free(d_p)
            rolled.idx = i
            B.weight(be, rolled, det)
            B.filter(be, rolled, det)
            B.backproject(be, rolled, v, 0, det, vg, False, False, None)
            be.free(rolled)
        return DM.volume_to_host(be, v, vg).reshape(vg.dim_z, vg.dim_y, vg.dim_x).copy()


def drive(root, out, extra, ok=True):
    args = [P.EXE, "--geometry", root / "geo.ini", "--input", root / "counts", "--output", root / out] + extra
    r = subprocess.run([str(a) for a in args], capture_output=True, text=True, timeout=300)
    assert (r.returncode == 0) == ok, r.stdout + r.stderr
    return r.stdout if ok else r.stderr


def volume_of(root, out):
    return F.ddbvf_read(str(root / out / "vol.ddbvf"))[1]


def scan_on_disk(tmp_path_factory, bin_factor):
    root = tmp_path_factory.mktemp("phase_scan_%d" % bin_factor)
    s = CH.scan()
    st = CH.settings(s, bin_factor)
    write_scan(root, s)
    alpha = alpha_for(st)
    options = (["--bin", st.bin] if st.bin > 1 else []) + chain_options(root, st) + [
        "--beam-hardening", "%.9g:%.9g" % st.bh, "--detector-roll", "%.9g" % ETA]
    return dict(root=root, s=s, st=st, alpha=alpha, options=options, want=mirror(s, st, alpha), plain=mirror(s, st, None))


@pytest.fixture(scope="module")
def given(tmp_path_factory):
    return scan_on_disk(tmp_path_factory, 1)


@pytest.fixture(scope="module")
def binned(tmp_path_factory):
    return scan_on_disk(tmp_path_factory, 2)


def two_devices():
    return ["--devices", 2 if len(B.get_devices()) >= 2 else 1]


FORMS = {"slabs_1": ["--slabs", 1], "slabs_3": ["--slabs", 3], "batch_1": ["--slabs", 2, "--batch", 1], "devices": None}


def assert_equals_the_python_chain(given, form):
    st, root = given["st"], given["root"]
    extra = ["--slabs", 4] + two_devices() if FORMS[form] is None else FORMS[form]
    text = drive(root, form, given["options"] + ["--phase-alpha", "%.9g:%d" % (given["alpha"], MARGIN)] + extra)
    got = volume_of(root, form)
    assert np.abs(given["want"]).max() > 0 and not np.array_equal(bits(given["want"]), bits(given["plain"]))
    assert got.shape == given["want"].shape and np.array_equal(bits(got), bits(given["want"])), form
    line = LINE.search(text)
    assert line, text
    n_x, n_y, scratch = B.phase_retrieval_check(given["alpha"], st.t_min, MARGIN, st.dim_x, st.dim_y, st.geo[2], st.geo[3])
    assert np.float32(line.group(1)) == np.float32(given["alpha"]) and abs(float(line.group(2)) - 0.4) < 1e-3 and int(line.group(4)) == MARGIN
    assert np.float32(line.group(5)) == np.float32(st.t_min) and (int(line.group(6)), int(line.group(7)), int(line.group(8))) == (n_x, n_y, scratch)
    assert "detector roll on" in text and "beam hardening on" in text and "ring filter on" in text
    return text


@pytest.mark.parametrize("form", sorted(FORMS))
def test_phase_alpha_equals_the_python_chain(given, form):
    assert_equals_the_python_chain(given, form)


def test_with_bin_2_the_pitches_and_sizes_are_the_binned_detector_s(binned):
    text = assert_equals_the_python_chain(binned, "slabs_3")
    assert "binning on: 2 x 2 bins" in text and binned["st"].geo[2] == 2 * CH.GEO[2]


def test_the_material_form_and_the_defaults(given):
    """--phase D:E is --phase-alpha of phase_alpha(D, E) with the default margin; --phase-floor replaces the flat field's t_min"""
    st, root = given["st"], given["root"]
    det = B.DetectorGeometry(*st.geo)
    energy = 30.0
    ratio = alpha_for(st) / B.phase_alpha(det, 1.0, energy)          # alpha is linear in delta / beta
    alpha = B.phase_alpha(det, ratio, energy)
    margin = B.phase_default_margin(alpha, det.l_px_row, det.l_px_col)
    a = drive(root, "material", given["options"] + ["--phase", "%.17g:%.17g" % (ratio, energy), "--phase-floor", "0.25", "--slabs", 2])
    b = drive(root, "alpha", given["options"] + ["--phase-alpha", "%.9g" % alpha, "--phase-floor", "0.25", "--slabs", 1])
    la, lb = LINE.search(a), LINE.search(b)
    assert la and lb and la.groups() == lb.groups(), a + b
    assert np.float32(la.group(1)) == np.float32(alpha) and int(la.group(4)) == margin == 8 and float(la.group(5)) == 0.25
    want = mirror(given["s"], st, alpha, margin, 0.25)
    assert not np.array_equal(bits(want), bits(given["want"]))          # the floor of 0.25 is reached
    assert np.array_equal(bits(volume_of(root, "material")), bits(want)) and np.array_equal(bits(volume_of(root, "alpha")), bits(want))


def test_without_the_option_nothing_changes(given):
    st, root = given["st"], given["root"]
    text = drive(root, "plain", given["options"] + ["--slabs", 3])
    assert "phase retrieval on" not in text
    assert np.array_equal(bits(volume_of(root, "plain")), bits(given["plain"]))


@pytest.mark.parametrize("extra,words", [
    (["--phase-alpha", "0"], "MM2 must be finite and greater than 0"),
    (["--phase-alpha", "-3"], "MM2 must be finite and greater than 0"),
    (["--phase-alpha", "nan"], "MM2 must be finite and greater than 0"),
    (["--phase-alpha", "inf:4"], "MM2 must be finite and greater than 0"),
    (["--phase-alpha", "3:0"], "MARGIN must lie in 1 .. 1024"),
    (["--phase-alpha", "3:1025"], "MARGIN must lie in 1 .. 1024"),
    (["--phase-alpha", "3:4:5"], "cannot read"),
    (["--phase-alpha", "much"], "cannot read"),
    (["--phase-alpha", "3:1.5"], "cannot read"),
    (["--phase", "1000"], "cannot read"),
    (["--phase", "1000:0"], "both must be finite and greater than 0"),
    (["--phase", "-5:30"], "both must be finite and greater than 0"),
    (["--phase", "nan:30"], "both must be finite and greater than 0"),
    (["--phase", "1000:30", "--phase-alpha", "3"], "cannot be combined"),
    (["--phase-alpha", "3", "--phase-floor", "0"], "T must lie in (0, 1]"),
    (["--phase-alpha", "3", "--phase-floor", "1.5"], "T must lie in (0, 1]"),
    (["--phase-floor", "0.5"], "--phase-floor needs --phase or --phase-alpha"),
])
def test_refusals(given, extra, words):
    err = drive(given["root"], "refused", given["options"] + extra, ok=False)
    assert words in err, err
