"""The whole frame chain through the driver and the C++ mirror: paris.hip with every option of the chain given
at once on the scan of tests/chain_rule.py, against the Python mirror's chain -- Backend.upload_raw, bin_frames, flat_field_rows,
air_normalize, defect_repair_rows, zinger_filter_rows, ring_correct_rows, beam_hardening, which tests/test_gpu_frame_chain.py holds to
the composed numpy rule pass by pass -- followed by the weights, the row filter and the backprojection. Every slab form derives its
bands' rows from all the options together; each must give the one-slab volume bit for bit."""
import os
import re
import subprocess

import numpy as np
import pytest

import chain_rule as CH
import ring_rule
import test_gpu_flat_field as FF
import test_gpu_paris_hip as P
import volume_window_rule as VW
import zinger_rule
from oracle import formats as F
from paris_amd import backend as B
from test_gpu_binning_driver import write_geometry
from test_gpu_frame_chain import Frames, clear, configure

pytestmark = pytest.mark.gpu

N = CH.N_FRAMES
EXTEND = (16, 4)                       # --extend-rows W:M -- a taper of 16 pixels from the mean of 4 edge pixels
SCAN_RANGE = 10.0 * (N - 1)            # --short-scan: from the first to the last angle of the 36 views, 10 degrees apart


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def mirror_frames(be, counts, st):
    """the chain of tests/test_gpu_frame_chain.py on the device, all frames in one call per pass: (final frames, ring correction,
    the frames after the zinger filter)"""
    n = len(counts)
    configure(be, st)
    raw = Frames(be, n, st.src_x, st.src_y)
    dst = Frames(be, n, st.dim_x, st.dim_y) if st.bin > 1 else raw
    at = dict(frame_stride=dst.stride, n_frames=n)
    try:
        for k in range(n):
            be.upload_raw(counts[k], raw.frame(k))
        if st.bin > 1:
            be.bin_frames(raw.frame(0), dst.frame(0), src_frame_stride=raw.stride, dst_frame_stride=dst.stride, n_frames=n)
        be.flat_field_rows(dst.frame(0), **at)
        be.air_normalize(dst.frame(0), **at)
        be.defect_repair_rows(dst.frame(0), **at)
        be.zinger_filter_rows(dst.frame(0), **at)
        filtered = dst.read()[0].copy()
        be.ring_profile_begin(st.dim_x, st.dim_y)
        be.ring_profile_add_rows(dst.frame(0), **at)
        c, _, stats = be.ring_profile_finish(*st.rings)
        be.set_ring_correction(c)
        be.ring_correct_rows(dst.frame(0), **at)
        be.beam_hardening(dst.frame(0), **at)
        return dst.read()[0].copy(), c, stats, filtered
    finally:
        clear(be)
        raw.free()
        dst.free()


def mirror_volume(be, frames, geo, prepare=None, extend=None):
    """PARIS's loop through the Python mirror from the chain's frames on: [redundancy weight,] weight, filter, backproject"""
    det = B.DetectorGeometry(*geo)
    vg = B.calculate_volume_geometry(det)
    if extend is not None:
        be.set_row_extension(extend[1], extend[0])
    try:
        v = be.make_volume_device(vg.dim_x, vg.dim_y, vg.dim_z)
        for i, fr in enumerate(frames):
            d_p = B.load(be, B.Projection(np.ascontiguousarray(fr, np.float32), det.n_row, det.n_col, idx=i))
            if prepare is not None:
                prepare(be, d_p, det)
            B.weight(be, d_p, det)
            B.filter(be, d_p, det)
            B.backproject(be, d_p, v, 0, det, vg, False, False, None)
            be.free(d_p)
        h = be.make_volume_host(vg.dim_x, vg.dim_y, vg.dim_z)
        be.copy_d2h(v, h)
        be.free(v)
    finally:
        if extend is not None:
            be.clear_row_extension()
    return h.buf.reshape(vg.dim_z, vg.dim_y, vg.dim_x).copy(), det, vg


def write_scan(root, s):
    """the scan on disk as the other driver tests write theirs: u16 HIS files, one dark and one flat frame, the mask as raw bytes"""
    (root / "ref").mkdir()
    (root / "ref" / "dark.his").write_bytes(F.his_file_bytes(s.dark[None].astype(np.uint16), 4, 32))
    (root / "ref" / "flat.his").write_bytes(F.his_file_bytes(s.flat[None].astype(np.uint16), 4))
    (root / "counts").mkdir()
    (root / "counts" / "a.his").write_bytes(F.his_file_bytes(s.counts[:20], 4, 32))
    (root / "counts" / "b.his").write_bytes(F.his_file_bytes(s.counts[20:], 4, 32))
    (root / "mask.raw").write_bytes(s.mask.tobytes())
    write_geometry(root / "geo.ini", s.geo)


def chain_options(root, st, from_flat=True):
    rect, z, r = st.rect, st.zingers, st.rings
    return ["--flat", root / "ref" / "flat.his", "--dark", root / "ref" / "dark.his", "--defects", root / "mask.raw"] + (
        ["--defects-from-flat"] if from_flat else []) + ["--air-region", "%d:%d:%d:%d" % rect, "--zingers", "%.9g:%.9g" % z[:2],
                                                        "--zinger-polarity", {0: "both", 1: "bright", -1: "dark"}[z[2]],
                                                        "--rings", "%d:%.9g:%.9g" % r]


def drive(root, out, extra, env=None):
    args = [P.EXE, "--geometry", root / "geo.ini", "--input", root / "counts", "--output", root / out] + extra
    r = subprocess.run([str(a) for a in args], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


AIR_LINE = re.compile(r"air region (on|in the pre-pass): .* frame, (\d+) frame band\(s\) measured, (\d+) normalised, (\d+) with too few pixels, (\d+) above the limit")
ZINGER_LINE = re.compile(r"zinger filter on: (\d+) frame band\(s\) examined, (\d+) pixel\(s\) replaced, (\d+) saturated")
RING_LINE = re.compile(r"ring filter on: (\d+) frame\(s\) in the pre-pass \(\S+ s\), (.*)$", re.M)


def ring_text(st):
    return "%d pixel(s) corrected, %d below the floor, %d above the limit, %d not finite, largest |c| %.6g" % (
        st["corrected"], st["below_floor"], st["above_limit"], st["not_finite"], float(np.float32(st["max_abs"])))


def assert_reports(out, slabs, ring_stats, replaced):
    """the pre-pass measured every frame once; the main run measured and examined every frame once per slab (as
    tests/test_gpu_air_driver.py states for the frame bands), normalised them all, saturated none, and replaced in each slab's band what
    the zinger rule replaces in those rows"""
    air = {m.group(1): tuple(int(v) for v in m.groups()[1:]) for m in AIR_LINE.finditer(out)}
    assert air["in the pre-pass"] == (N, N, 0, 0) and air["on"] == (slabs * N, slabs * N, 0, 0), out
    z = tuple(int(v) for v in ZINGER_LINE.search(out).groups())
    assert (z[0], z[2]) == (slabs * N, 0) and z[1] > 0 and (replaced is None or z[1] == replaced), out
    ring = RING_LINE.search(out)
    assert (int(ring.group(1)), ring.group(2)) == (N, ring_text(ring_stats)), out


# ---- 1. everything given -----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def given(tmp_path_factory):
    root = tmp_path_factory.mktemp("chain_given")
    s = CH.scan()
    st = CH.settings(s, 2)
    steps, info = CH.chain(s.counts, st)
    CH.assert_every_pass_counts(s.counts, st, steps, info)
    write_scan(root, s)
    scan = B.ShortScan(0.0, SCAN_RANGE)
    with B.Backend(0) as be:
        final, c, _, _ = mirror_frames(be, s.counts, st)
        assert np.array_equal(bits(final), bits(steps[-1])) and ring_rule.same_bits(c, info.ring_c)
        want, det, vg = mirror_volume(be, final, st.geo, lambda b, d, g: B.stage_short_scan_weight(b, d, g, scan), EXTEND)
        plain, _, _ = mirror_volume(be, steps[2], st.geo)
    assert np.abs(want).max() > 0 and not np.array_equal(bits(want), bits(plain))
    options = ["--bin", 2] + chain_options(root, st) + ["--beam-hardening", "%.9g:%.9g" % st.bh, "--extend-rows", "%d:%d" % EXTEND, "--short-scan"]
    return dict(root=root, st=st, steps=steps, info=info, want=want, det=det, vg=vg, options=options)


def replaced_in_bands(given, slabs, row_band):
    """what the zinger rule replaces over the scan when every slab filters its own band of the repaired frames"""
    det, vg, st = given["det"], given["vg"], given["st"]
    dz = vg.dim_z // slabs
    total = 0
    for k in range(slabs):
        first, count = (B.slab_row_band(det, vg, vg.dim_x, vg.dim_y, dz + (vg.dim_z % slabs if k == slabs - 1 else 0), k * dz) if row_band
                        else (0, st.dim_y))
        total += sum(zinger_rule.apply(f, *st.zingers, rows=(first, first + count))[1] for f in given["steps"][4])
    return total


FORMS = {"slabs_1": (["--slabs", 1], 1, True, None),
         "slabs_3": (["--slabs", 3], 3, True, None),
         "slabs_3_batch_1": (["--slabs", 3, "--batch", 1], 3, True, None),
         "slabs_2_no_row_band": (["--slabs", 2, "--no-row-band"], 2, False, None),
         "slabs_3_batch_7_on_3_devices": (["--slabs", 3, "--batch", 7], 3, True, "3")}


@pytest.mark.parametrize("form", sorted(FORMS))
def test_everything_given_equals_the_python_chain(given, form):
    """--bin 2 --flat --dark --defects --defects-from-flat --air-region --zingers --rings --beam-hardening --extend-rows --short-scan:
    every slab form gives the volume of the Python mirror's chain followed by short_scan_weight, weight, filter with set_row_extension
    and backproject -- so each equals --slabs 1 -- and reports the counts of the numpy rules"""
    extra, slabs, row_band, devices = FORMS[form]
    env = dict(os.environ, PARIS_HIP_VIRTUAL_DEVICES=devices) if devices else None
    out = drive(given["root"], form, given["options"] + extra, env)
    got = F.ddbvf_read(str(given["root"] / form / "vol.ddbvf"))[1]
    assert got.shape == given["want"].shape and np.array_equal(bits(got), bits(given["want"])), form
    assert_reports(out, slabs, given["info"].ring_stats, replaced_in_bands(given, slabs, row_band))
    assert "binning on: 2 x 2 bins, detector 67 x 45 -> 33 x 22" in out and "beam hardening on: coefficients %.9g:%.9g" % tuple(float(np.float32(c)) for c in given["st"].bh) in out
    assert "row extension on: cos^2 taper of %d pixel(s), mean of %d edge pixel(s)" % EXTEND in out


def test_everything_given_as_u16_voxels(given):
    """--voxel-type u16 --voxel-range LO:HI: Backend.quantize_volume of the reference volume"""
    v = given["want"]
    lo, hi = np.float32(np.percentile(v, 5)), np.float32(np.percentile(v, 95))      # a window that cuts both ends
    assert lo < hi
    drive(given["root"], "u16", given["options"] + ["--slabs", 1, "--voxel-type", "u16", "--voxel-range", "%r:%r" % (float(lo), float(hi))])
    _, got = VW.read_mhd(str(given["root"] / "u16" / "vol.mhd"))
    with B.Backend(0) as be:
        d_v = be.make_volume_device(v.shape[2], v.shape[1], v.shape[0])
        be.copy_h2d(B.Volume(np.ascontiguousarray(v), v.shape[2], v.shape[1], v.shape[0]), d_v)
        want = be.quantize_volume(d_v, lo, hi, np.uint16)
        be.free(d_v)
    assert got.dtype == np.uint16 and np.array_equal(got.ravel(), np.asarray(want).ravel())
    assert len(np.unique(got)) > 100 and got.min() == 0 and got.max() == 65535


# ---- 2. the C++ mirror -------------------------------------------------------------------------------------------------------------

OFFSET_GEO = CH.GEO[:4] + (-16.0,) + CH.GEO[5:]       # the detector shifted sideways by 16 pixels: half a fan over the full circle


def test_the_cpp_mirror_equals_the_driver(tmp_path):
    """PARIS's loop through paris::hip with the flags paris_hip_demo has together -- --flat --air-region --defects --zingers --rings
    --extend-rows --offset-detector, no --bin -- on a geometry paris_hip_offset_detector_check accepts: the volume of paris.hip with the
    same options, which is the Python chain's"""
    s = CH.scan(geo=OFFSET_GEO)
    st = CH.settings(s, 1)
    st.mask = (s.mask != 0).astype(np.uint8)          # --defects alone: the demo has no --defects-from-flat
    st.plan = B.defect_plan(st.mask)
    steps, info = CH.chain(s.counts, st, upto=6)
    assert info.ring_stats["corrected"] > 20 and not any(info.saturated) and info.air_why == ["normalised"] * N
    det = B.DetectorGeometry(*OFFSET_GEO)
    B.offset_detector_check(det)
    write_scan(tmp_path, s)
    with B.Backend(0) as be:
        want, _, vg = mirror_volume(be, steps[6], OFFSET_GEO, lambda b, d, g: B.stage_offset_detector_weight(b, d, g), EXTEND)
    options = chain_options(tmp_path, st, from_flat=False) + ["--extend-rows", "%d:%d" % EXTEND, "--offset-detector"]
    drive(tmp_path, "drv", options + ["--slabs", 2])
    got = F.ddbvf_read(str(tmp_path / "drv" / "vol.ddbvf"))[1]
    assert np.abs(want).max() > 0 and np.array_equal(bits(got), bits(want))
    s.counts.astype(np.float32).tofile(tmp_path / "in.raw")
    s.dark.tofile(tmp_path / "dark.raw")
    s.flat.tofile(tmp_path / "flat.raw")
    out = tmp_path / "demo.raw"
    args = [FF.DEMO] + [str(v) for v in OFFSET_GEO] + [N, tmp_path / "in.raw", out, "--slabs", 2,
            "--flat", tmp_path / "dark.raw", tmp_path / "flat.raw", "1e-05", "--air-region"] + list(st.rect) + [0, "--defects", tmp_path / "mask.raw",
            "--zingers", "%.9g" % st.zingers[0], "%.9g" % st.zingers[1], st.zingers[2], "--rings", st.rings[0], "%.9g" % st.rings[1], "%.9g" % st.rings[2],
            "--extend-rows", EXTEND[0], EXTEND[1], "--offset-detector"]
    r = subprocess.run([str(a) for a in args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr + r.stdout
    assert np.array_equal(bits(np.fromfile(out, np.float32).reshape(want.shape)), bits(want))


# ---- 3. everything found -----------------------------------------------------------------------------------------------------------

AXIS = (0.0, 3.0, 0.25)                # --find-axis LO:HI at the default step: 13 candidates about the scan's 1.5
FIT = (2, 16, 1)                       # --fit-beam-hardening N:SLICES:MARGIN
AXIS_LINE = re.compile(r"^axis search on: delta_s = (\S+) px \(the geometry file gave (\S+)\), candidate (\d+) of (\d+) at step (\S+), .* (\d+) candidate\(s\) scored, "
                       r"(\d+) pair\(s\) skipped, (\d+) frame\(s\) of (\d+) row\(s\)", re.M)
BH_LINE = re.compile(r"^beam hardening on: coefficients (\S+)$", re.M)


@pytest.fixture(scope="module")
def found(tmp_path_factory):
    """the full circle without --bin: the pre-passes' results from the Python mirror, each fed the composed frames -- the axis from the
    frames after the zinger filter, the fit from the frames after the ring correction under the found axis -- and the volume of the
    Python chain with them. (A full circle needs no redundancy weight, so fit_beam_hardening's prepare= stays empty.)"""
    root = tmp_path_factory.mktemp("chain_found")
    s = CH.scan()
    st = CH.settings(s, 1)
    st.mask = (s.mask != 0).astype(np.uint8)          # --defects alone
    st.plan = B.defect_plan(st.mask)
    steps, info = CH.chain(s.counts, st, upto=6)
    assert info.ring_stats["corrected"] > 20 and not any(info.saturated) and info.air_why == ["normalised"] * N
    write_scan(root, s)
    count = int(np.floor((AXIS[1] - AXIS[0]) / AXIS[2] + 0.5)) + 1
    with B.Backend(0) as be:
        det0 = B.DetectorGeometry(*s.geo)
        be.axis_search_begin(AXIS[0], AXIS[2], count, det0, N)
        for i, f in enumerate(steps[5]):
            d_p = B.load(be, B.Projection(np.ascontiguousarray(f), det0.n_row, det0.n_col, idx=i))
            be.axis_search_add(d_p, i)
            be.free(d_p)
        axis = be.axis_search_finish()[0]
        geo = s.geo[:4] + (float(np.float32(axis.delta_s)),) + s.geo[5:]
        det = B.DetectorGeometry(*geo)
        vg = B.calculate_volume_geometry(det)
        fit = be.fit_beam_hardening(list(steps[6]), det, degree=FIT[0], margin=FIT[2], slices=((vg.dim_z - FIT[1]) // 2, FIT[1]))
        final = B.beam_hardening_host(fit.c, steps[6])
        want, _, _ = mirror_volume(be, final, geo)
        plain, _, _ = mirror_volume(be, steps[6], s.geo)
    assert np.abs(want).max() > 0 and not np.array_equal(bits(want), bits(plain))
    options = chain_options(root, st, from_flat=False) + ["--find-axis", "%g:%g" % AXIS[:2], "--fit-beam-hardening", "%d:%d:%d" % FIT]
    return dict(root=root, st=st, info=info, want=want, axis=axis, count=count, fit=fit, options=options)


@pytest.mark.parametrize("slabs", [1, 3])
def test_everything_found_equals_the_python_chain(found, slabs):
    """--flat --dark --defects --air-region --zingers --rings --find-axis --fit-beam-hardening on the full circle: the ring pre-pass and
    the axis search run together, the fit after them; the reported axis and coefficients are the Python mirror's on the composed
    frames, and the volume is the Python chain's with them, in one slab and in three"""
    out = drive(found["root"], "found_%d" % slabs, found["options"] + ["--slabs", slabs])
    axis, fit = found["axis"], found["fit"]
    m = AXIS_LINE.search(out)
    assert m is not None, out
    assert m.group(1) == "%.4f" % axis.delta_s and m.group(2) == "%.4f" % CH.GEO[4], out
    assert [int(m.group(k)) for k in (3, 4, 6, 7, 8, 9)] == [axis.best, found["count"], axis.scored, axis.skipped, N, 2], out
    assert abs(axis.delta_s - CH.GEO[4]) < 0.25                                  # the search finds the scan's axis
    c = np.array([float(t) for t in BH_LINE.search(out).group(1).split(":")], np.float32)
    assert np.array_equal(bits(c), bits(fit.c)), (c, fit.c)
    assert "beam-hardening fit on: degree %d, %d frame(s)" % (FIT[0], N) in out
    assert_reports(out, slabs, found["info"].ring_stats, None)
    got = F.ddbvf_read(str(found["root"] / ("found_%d" % slabs) / "vol.ddbvf"))[1]
    assert got.shape == found["want"].shape and np.array_equal(bits(got), bits(found["want"]))
