"""paris.hip --metal: the scene of tests/metal_rule.py as u16 counts in two HIS files, with --flat and a
--min-transmission that clips the line integrals at 3.0, against the Python chain -- the correction's rule, Backend.reduce_metal, then
metal_inpaint / weight / filter / backproject per view and metal_reinsert -- bit for bit: in one slab and in three, frame by frame,
without the row band, on two devices where the machine has them, together with --detector-roll and --zingers, and as u16 voxels over
an automatic window. The report line's numbers are the Python chain's counts; the refusals; and without --metal the volume is the
plain Python chain's."""
import math
import re
import subprocess

import numpy as np
import pytest

import binning_rule as BR
import chain_rule as CH
import fdk_model
import metal_rule as R
import test_gpu_flat_field as FF
import test_gpu_paris_hip as P
import volume_window_rule as VW
from oracle import formats as F
from paris_amd import backend as B

pytestmark = pytest.mark.gpu

CLIP = 3.0
T_MIN = float(np.float32(math.exp(-CLIP)))
FLAT = 60000
ROLL = 0.8
ZINGERS = (0.5, 0.0)
DET = B.DetectorGeometry(*R.SCENE_DET)
VG = B.calculate_volume_geometry(DET)
THRESHOLD = float(np.float32(R.SCENE_CASES[0][1] * fdk_model.scale(DET, R.SCENE_VIEWS)))   # 0.3 per mm in the volume's own units
METAL = "%.9g:%d:%.9g" % (THRESHOLD, R.SCENE_GROW, R.SCENE_MIN_PATH)
LINE = re.compile(r"^metal reduction on: (\d+) voxel\(s\) above (\S+) collected, grow (\d+), min_path (\S+) mm, (\d+) trace pixel\(s\) over all views, "
                  r"(\d+) frame\(s\) in the pre-pass \(\S+ s\), (\d+) pixel\(s\) replaced in (\d+) run\(s\) and (\d+) row\(s\) left in the main pass$", re.M)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def scene_scan():
    """(counts, flat, frames): the scene as u16 counts with its flat, and the line integrals the driver's correction makes of them"""
    p = R.scene_frames().astype(np.float64)
    rng = np.random.default_rng(31)
    counts = np.clip(np.rint(FLAT * np.exp(-p)), 0, 65535).astype(np.uint16)
    for k in range(0, len(counts), 7):                                                     # a few zingers, for the run that filters them
        counts[k, rng.integers(0, 32), rng.integers(0, 64)] = 65535
    flat = np.full(counts.shape[1:], FLAT, np.uint16)
    frames = CH.flat_field(counts.astype(np.float32), np.zeros(flat.shape, np.float32), flat.astype(np.float32), T_MIN)
    assert frames.max() == np.float32(-math.log(np.float32(T_MIN))) and (frames == frames.max()).sum() > 1000   # the floor clips the metal's rays
    return counts, flat, frames


@pytest.fixture(scope="module")
def scan(tmp_path_factory):
    """the inputs on disk and the line integrals the driver's correction makes of them"""
    root = tmp_path_factory.mktemp("metal_scan")
    counts, flat, frames = scene_scan()
    (root / "ref").mkdir()
    (root / "ref" / "flat.his").write_bytes(F.his_file_bytes(flat[None], 4))
    (root / "counts").mkdir()
    (root / "counts" / "a.his").write_bytes(F.his_file_bytes(counts[:70], 4, 32))
    (root / "counts" / "b.his").write_bytes(F.his_file_bytes(counts[70:], 4, 32))
    (root / "geo.ini").write_text("\n".join("%s = %s" % (k, v if isinstance(v, int) else "%.9g" % float(v)) for k, v in zip(FF.GEO_KEYS, R.SCENE_DET)) + "\n")
    return root, frames


def drive(root, out, extra, ok=True):
    args = [P.EXE, "--geometry", root / "geo.ini", "--input", root / "counts", "--output", root / out, "--flat", root / "ref" / "flat.his",
            "--min-transmission", "%.9g" % T_MIN] + extra
    r = subprocess.run([str(a) for a in args], capture_output=True, text=True, timeout=300)
    assert (r.returncode == 0) == ok, r.stdout + r.stderr
    return r.stdout if ok else r.stderr


def volume_of(root, out):
    return F.ddbvf_read(str(root / out / "vol.ddbvf"))[1]


def python_chain(frames, metal, roll=None, zingers=None, view=None, reinsert=True, last=None):
    """(volume, MetalTrace or None, MetalCounts or None): the frames through [zinger filter,] [roll,] [the remedy,] weight, filter and
    backprojection in the Python mirror. view: the trace frame i is inpainted with, as a function of i (None: its own); reinsert False:
    the metal voxels are not put back; last: only the frames 0 .. last are inpainted"""
    with B.Backend(0) as be:
        frames = [np.ascontiguousarray(f, np.float32) for f in frames]
        if zingers is not None or roll is not None:
            if zingers is not None:
                be.set_zinger_filter(zingers[0], zingers[1], 0, DET.n_row, DET.n_col)
            if roll is not None:
                be.set_detector_roll(roll, DET)
            passed = []
            for f in frames:
                src, dst = be.make_projection_device(DET.n_row, DET.n_col), be.make_projection_device(DET.n_row, DET.n_col)
                be.upload_raw(f, src)
                if zingers is not None:
                    be.zinger_filter_rows(src)
                if roll is not None:
                    be.detector_roll(src, dst)
                h = be.make_projection_host(DET.n_row, DET.n_col)
                be.copy_d2h(dst if roll is not None else src, h)
                passed.append(h.buf.copy())
                be.free(src)
                be.free(dst)
            frames = passed
        mt = be.reduce_metal(frames, DET, THRESHOLD, grow=R.SCENE_GROW, min_path=R.SCENE_MIN_PATH, vol_geo=VG) if metal else None
        v = be.make_volume_device(VG.dim_x, VG.dim_y, VG.dim_z)
        be.memset_volume(v)
        for i, f in enumerate(frames):
            d_p = B.load(be, B.Projection(f, DET.n_row, DET.n_col, idx=i))
            if metal and (last is None or i <= last):
                be.metal_inpaint(d_p, None if view is None else view(i))
            B.weight(be, d_p, DET)
            B.filter(be, d_p, DET)
            B.backproject(be, d_p, v, 0, DET, VG, False, False, None)
            be.free(d_p)
        if metal and reinsert:
            be.metal_reinsert(v)
        h = be.make_volume_host(VG.dim_x, VG.dim_y, VG.dim_z)
        be.copy_d2h(v, h)
        return h.buf.reshape(VG.dim_z, VG.dim_y, VG.dim_x).copy(), mt, (be.metal_stats() if metal else None)


@pytest.fixture(scope="module")
def want(scan):
    return python_chain(scan[1], True)


def two_devices():
    return ["--devices", 2 if len(B.get_devices()) >= 2 else 1]


FORMS = {"slabs_1": (["--slabs", 1], 1), "slabs_3": (["--slabs", 3], 3), "batch_1": (["--slabs", 2, "--batch", 1], 2),
         "no_row_band": (["--slabs", 3, "--no-row-band"], 3), "devices": (None, 4)}


@pytest.mark.parametrize("form", sorted(FORMS))
def test_metal_equals_the_python_chain(scan, want, form):
    root, frames = scan
    volume, mt, counts = want
    extra, slabs = FORMS[form]
    extra = ["--slabs", 4] + two_devices() if extra is None else extra
    text = drive(root, form, ["--metal", METAL] + extra)
    got = volume_of(root, form)
    assert len(mt.index) > 100 and np.abs(volume).max() > 0 and got.shape == volume.shape
    assert np.array_equal(bits(got), bits(volume)), form
    line = LINE.search(text)
    assert line, text
    assert int(line.group(1)) == len(mt.index) and np.float32(line.group(2)) == np.float32(THRESHOLD) and int(line.group(3)) == R.SCENE_GROW
    assert float(line.group(4)) == R.SCENE_MIN_PATH and int(line.group(5)) == mt.trace_pixels and int(line.group(6)) == R.SCENE_VIEWS
    # the main pass: without the row band every slab inpaints whole frames, exactly what the Python chain counts, once per slab; with
    # it each slab inpaints the detector rows it can read
    replaced, runs, left = (int(line.group(k)) for k in (7, 8, 9))
    assert left == counts.rows_left == 0 and counts.replaced == mt.trace_pixels
    if form == "no_row_band":
        assert (replaced, runs) == (counts.replaced * slabs, counts.runs * slabs)
    else:
        assert 0 < replaced <= counts.replaced * slabs and 0 < runs <= counts.runs * slabs


def test_the_default_min_path_is_half_a_voxel(scan):
    root, _ = scan
    text = drive(root, "default", ["--metal", "%.9g" % THRESHOLD, "--slabs", 1])
    line = LINE.search(text)
    assert line and int(line.group(3)) == 1 and np.float32(line.group(4)) == np.float32(0.5) * np.float32(VG.l_vx_x)


def test_with_the_roll_and_the_zinger_filter(scan):
    """the trace lives on the detector the roll writes, and the pre-pass sees the frames the main pass sees"""
    root, frames = scan
    volume, mt, _ = python_chain(frames, True, roll=ROLL, zingers=ZINGERS)
    plain, _, _ = python_chain(frames, True)
    text = drive(root, "roll", ["--metal", METAL, "--slabs", 2, "--detector-roll", "%.9g" % ROLL, "--zingers", "%.9g:%.9g" % ZINGERS, "--zinger-polarity", "both"])
    got = volume_of(root, "roll")
    assert "detector roll on" in text and "zinger filter on" in text and int(LINE.search(text).group(5)) == mt.trace_pixels
    assert np.array_equal(bits(got), bits(volume)) and not np.array_equal(bits(volume), bits(plain))


def test_with_bin_the_pre_pass_bins_as_the_main_pass_does(tmp_path):
    """--metal --bin 2 on a source detector of twice the pixels each way, whose 2 x 2 bins make the scene's detector: the pre-pass reads
    source frames into the full-width slots and bins them as the main pass does, so the volume and the report are those of the driver
    without --bin on frames, flat and geometry binned on the host by the numpy rule (as tests/test_gpu_binning_driver.py compares --bin)"""
    rng = np.random.default_rng(37)
    src_geo = (2 * R.SCENE_DET[0], 2 * R.SCENE_DET[1], 0.5 * R.SCENE_DET[2], 0.5 * R.SCENE_DET[3]) + R.SCENE_DET[4:]
    assert R.SCENE_DET[4:6] == (0.0, 0.0) and tuple(float(v) for v in BR.binned_geometry(src_geo, 2, 2)) == tuple(float(v) for v in R.SCENE_DET)
    p = np.repeat(np.repeat(R.scene_frames().astype(np.float64), 2, axis=1), 2, axis=2)
    counts = np.clip(np.rint(FLAT * np.exp(-p)) + rng.integers(-3, 4, p.shape), 0, 65535).astype(np.uint16)   # bins of unequal pixels
    flat = (FLAT + rng.integers(-200, 200, counts.shape[1:])).astype(np.uint16)
    for root, geo, code, ref, frames in (
            (tmp_path / "src", src_geo, 4, flat, counts),
            (tmp_path / "binned", BR.binned_geometry(src_geo, 2, 2), 128, BR.bin_frame(flat.astype(np.float32), 2, 2, None),
             np.stack([BR.bin_frame(f.astype(np.float32), 2, 2, None) for f in counts]))):
        (root / "ref").mkdir(parents=True)
        (root / "ref" / "flat.his").write_bytes(F.his_file_bytes(ref[None], code))
        (root / "counts").mkdir()
        (root / "counts" / "a.his").write_bytes(F.his_file_bytes(frames[:70], code, 32))
        (root / "counts" / "b.his").write_bytes(F.his_file_bytes(frames[70:], code, 32))
        (root / "geo.ini").write_text("\n".join("%s = %s" % (k, v if isinstance(v, int) else "%.9g" % float(v)) for k, v in zip(FF.GEO_KEYS, geo)) + "\n")
    text = drive(tmp_path / "src", "bin", ["--metal", METAL, "--bin", "2", "--slabs", 2])
    plain = drive(tmp_path / "binned", "pre", ["--metal", METAL, "--slabs", 2])
    got, want = volume_of(tmp_path / "src", "bin"), volume_of(tmp_path / "binned", "pre")
    assert "binning on: 2 x 2 bins, detector 128 x 64 -> 64 x 32" in text and "binning on" not in plain
    a, b = LINE.search(text), LINE.search(plain)
    assert a and b and a.groups() == b.groups() and int(a.group(1)) > 100 and int(a.group(5)) > 0 and int(a.group(6)) == R.SCENE_VIEWS, (text, plain)
    assert got.shape == want.shape == (VG.dim_z, VG.dim_y, VG.dim_x) and np.abs(want).max() > 0
    assert np.array_equal(bits(got), bits(want))


def test_as_u16_voxels_over_an_automatic_window(scan, want):
    """--voxel-type u16 --voxel-range auto: the window and the voxels see the metal that was put back"""
    root, _ = scan
    volume = want[0]
    drive(root, "u16", ["--metal", METAL, "--slabs", 1, "--devices", 1, "--voxel-type", "u16", "--voxel-range", "auto"])
    header, got = VW.read_mhd(str(root / "u16" / "vol.mhd"))
    with B.Backend(0) as be:
        d_v = be.make_volume_device(VG.dim_x, VG.dim_y, VG.dim_z)
        be.copy_h2d(B.Volume(np.ascontiguousarray(volume), VG.dim_x, VG.dim_y, VG.dim_z), d_v)
        st, _ = be.volume_stats(d_v)
        st, hist = be.volume_stats(d_v, st.min, st.max, 4096)
        lo, hi = B.volume_window_from_histogram(hist, st.min, st.max, 0.1, 99.9)       # (the driver's default percentiles)
        wanted = be.quantize_volume(d_v, lo, hi, np.uint16)
        be.free(d_v)
    assert st.max == volume.max() and volume.max() > THRESHOLD                            # the metal is there
    assert got.dtype == np.uint16 and np.array_equal(got.ravel(), np.asarray(wanted).ravel())


def test_without_the_option_nothing_changes(scan, want):
    root, frames = scan
    text = drive(root, "plain", ["--slabs", 2])
    plain, _, _ = python_chain(frames, False)
    assert "metal reduction on" not in text
    assert np.array_equal(bits(volume_of(root, "plain")), bits(plain)) and not np.array_equal(bits(plain), bits(want[0]))


@pytest.mark.parametrize("extra,words", [
    (["--metal", METAL, "--roi", "--roi-x2", 32, "--roi-y2", 32, "--roi-z2", 16], "--metal cannot be combined with --roi"),
    (["--metal", "%.9g:5" % THRESHOLD], "GROW must lie in 0 .. 4"),
    (["--metal", "%.9g:1:-0.5" % THRESHOLD], "MIN_PATH must be finite and not negative"),
    (["--metal", "nan"], "THR must be finite"),
    (["--metal", "inf:1"], "THR must be finite"),
    (["--metal", "%.9g:1:0.25:7" % THRESHOLD], "cannot read"),
    (["--metal", "much"], "cannot read"),
    (["--metal", "%.9g:1.5" % THRESHOLD], "cannot read"),
    (["--metal", "-1e30"], "a wrong threshold, not metal"),
])
def test_refusals(scan, extra, words):
    root, _ = scan
    err = drive(root, "refused", extra, ok=False)
    assert words in err and len([ln for ln in err.splitlines() if "--metal" in ln]) == 1, err
