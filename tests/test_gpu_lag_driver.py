"""paris.hip --lag: a scan of u16 counts on a 64 x 48 detector, 36 views, whose counts went through the
float64 forward model of the detector's lag, reconstructed with --lag, against the same driver WITHOUT --lag on f32 frames that the
library's host rule (paris_amd.backend.lag_correct_host, dark included) made from the same counts. The volumes are bit-identical: no
tolerance, and any pass of the driver that opened its sequence wrongly -- late, once for two slabs, for other rows -- would show.
With --bin the driver corrects the binned counts, so there the frames without --lag are the host rule's on host-binned counts, with
the binned references and geometry (as tests/test_gpu_binning_driver.py compares --bin)."""
import subprocess

import numpy as np
import pytest

import binning_rule as BR
import lag_rule as R
import test_gpu_flat_field as FF
import test_gpu_paris_hip as P
from oracle import formats as F
from paris_amd import backend as B

pytestmark = pytest.mark.gpu

GEO = (64, 48, 0.2, 0.25, 1.5, -0.75, 100, 200, 10.0)
N_FRAMES = 36
MODEL = R.MODELS[4]
OPTION = ":".join("%.9g:%.9g" % (np.float32(b), np.float32(a)) for b, a in MODEL)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def write_geometry(path, geo):
    path.write_text("\n".join("%s = %s" % (k, v if isinstance(v, int) else "%.9g" % float(v)) for k, v in zip(FF.GEO_KEYS, geo)) + "\n")
    return path


@pytest.fixture(scope="module")
def scan(tmp_path_factory):
    """the inputs on disk -- u16 counts with lag in them, a dark and a flat -- and what they hold"""
    root = tmp_path_factory.mktemp("lag_scan")
    rng = np.random.default_rng(23)
    shape = (GEO[1], GEO[0])
    darks = rng.integers(150, 450, (3,) + shape).astype(np.uint16)
    flats = (rng.integers(30000, 60000, shape)[None] + rng.integers(-400, 400, (5,) + shape)).astype(np.uint16)
    dark, flat = FF.mean(darks), FF.mean(flats)
    # an absorber whose edge sweeps across the detector from view to view: every pixel sees steps in time
    col = np.arange(shape[1])[None, None, :]
    k = np.arange(N_FRAMES)[:, None, None]
    behind = np.abs(col - (8 + 1.4 * k)) < 9
    t = np.where(behind, 0.06, 0.9) * np.exp(-0.3 * rng.random((N_FRAMES,) + shape))
    signal = (flat.astype(np.float64) - dark) * t                                  # what a detector without lag would add to its dark
    lagged = R.forward64(MODEL, signal)
    assert np.abs(lagged - signal).max() > 0.01 * 30000
    frames = np.clip(np.rint(dark + lagged + rng.normal(0, 20, t.shape)), 0, 65535).astype(np.uint16)
    (root / "ref").mkdir()
    (root / "ref" / "dark.his").write_bytes(F.his_file_bytes(darks, 4, 32))
    (root / "ref" / "flat.his").write_bytes(F.his_file_bytes(flats, 4))
    (root / "counts").mkdir()
    (root / "counts" / "a.his").write_bytes(F.his_file_bytes(frames[:20], 4, 32))
    (root / "counts" / "b.his").write_bytes(F.his_file_bytes(frames[20:], 4, 32))
    write_geometry(root / "geo.ini", GEO)
    return root, frames, dark, flat


def corrected_set(root, frames, dark, flat, geo, start="steady"):
    """the inputs of the run without --lag: f32 frames made by the host rule from the counts, the references as f32"""
    root.mkdir()
    fixed, _, _ = B.lag_correct_host(MODEL, frames.astype(np.float32), dark=dark, start=start)
    (root / "ref").mkdir()
    (root / "ref" / "dark.his").write_bytes(F.his_file_bytes(dark[None], 128))
    (root / "ref" / "flat.his").write_bytes(F.his_file_bytes(flat[None], 128))
    (root / "counts").mkdir()
    (root / "counts" / "a.his").write_bytes(F.his_file_bytes(fixed[:20], 128, 32))
    (root / "counts" / "b.his").write_bytes(F.his_file_bytes(fixed[20:], 128, 32))
    write_geometry(root / "geo.ini", geo)
    return fixed


def command(root, out, extra):
    return [str(a) for a in [P.EXE, "--geometry", root / "geo.ini", "--input", root / "counts", "--output", out, "--flat", root / "ref" / "flat.his",
                             "--dark", root / "ref" / "dark.his"] + extra]


def drive(root, out, extra):
    r = subprocess.run(command(root, out, extra), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout, F.ddbvf_read(str(out / "vol.ddbvf"))[1]


@pytest.mark.parametrize("start", R.STARTS)
def test_lag_equals_the_driver_on_frames_the_host_rule_corrected(tmp_path, scan, start):
    src, frames, dark, flat = scan
    fixed = corrected_set(tmp_path / "fixed", frames, dark, flat, GEO, start)
    assert np.abs(fixed - frames).max() > 100                                      # the correction moves counts
    extra = ["--lag", OPTION] + (["--lag-start", start] if start != "steady" else [])
    for slabs in (1, 2):   # two slabs: two passes over the scan, each restarts the state for its own rows
        text, got = drive(src, tmp_path / ("lag%d" % slabs), extra + ["--slabs", slabs])
        plain, want = drive(tmp_path / "fixed", tmp_path / ("fixed%d" % slabs), ["--slabs", slabs])
        assert ("lag correction on: 4 term(s)" in text and "b_0 = 0.950308" in text
                and ("starts steady" if start == "steady" else "starts at rest") in text), text
        assert "lag correction on" not in plain
        assert np.abs(want).max() > 0 and got.shape == want.shape
        assert np.array_equal(bits(got), bits(want)), slabs
    _, uncorrected = drive(src, tmp_path / "none", ["--slabs", 1])
    assert not np.array_equal(bits(uncorrected), bits(want))


def test_lag_on_binned_counts(tmp_path, scan):
    src, frames, dark, flat = scan
    binned = np.stack([BR.bin_frame(f.astype(np.float32), 2, 2, None) for f in frames])
    corrected_set(tmp_path / "fixed", binned, BR.bin_frame(dark, 2, 2, None), BR.bin_frame(flat, 2, 2, None), BR.binned_geometry(GEO, 2, 2))
    text, got = drive(src, tmp_path / "lag", ["--lag", OPTION, "--bin", "2", "--slabs", 2])
    _, want = drive(tmp_path / "fixed", tmp_path / "plain", ["--slabs", 2])
    assert "lag correction on" in text and "binning on" in text
    assert np.abs(want).max() > 0 and np.array_equal(bits(got), bits(want))


@pytest.mark.parametrize("binned", [False, True])
def test_lag_frame_by_frame(tmp_path, scan, binned):
    """--batch 1: every frame goes through the chain on its own, behind its upload -- the lag route alone and the one behind --bin --,
    against the references of the two tests above, which the driver makes group by group"""
    src, frames, dark, flat = scan
    if binned:
        counts = np.stack([BR.bin_frame(f.astype(np.float32), 2, 2, None) for f in frames])
        corrected_set(tmp_path / "fixed", counts, BR.bin_frame(dark, 2, 2, None), BR.bin_frame(flat, 2, 2, None), BR.binned_geometry(GEO, 2, 2))
    else:
        corrected_set(tmp_path / "fixed", frames, dark, flat, GEO)
    text, got = drive(src, tmp_path / "lag", ["--lag", OPTION, "--slabs", 2, "--batch", 1] + (["--bin", "2"] if binned else []))
    _, want = drive(tmp_path / "fixed", tmp_path / "plain", ["--slabs", 2])
    assert "lag correction on" in text and ("binning on" in text) == binned
    assert np.abs(want).max() > 0 and np.array_equal(bits(got), bits(want))


def test_the_pre_passes_open_sequences_of_their_own(tmp_path, scan):
    """--rings reads the scan once more before the reconstruction, --fit-beam-hardening once again: each pass corrects the lag from
    frame 0, so the volume and the reports are those of the run on the corrected frames"""
    src, frames, dark, flat = scan
    corrected_set(tmp_path / "fixed", frames, dark, flat, GEO)
    extra = ["--rings", "2:0.01", "--fit-beam-hardening", "2:8:0", "--slabs", 2]
    text, got = drive(src, tmp_path / "lag", ["--lag", OPTION] + extra)
    plain, want = drive(tmp_path / "fixed", tmp_path / "plain", extra)
    assert np.array_equal(bits(got), bits(want))
    for begin in ("ring filter on", "beam hardening on"):
        a, b = ([l.split(" s)")[-1] for l in t.splitlines() if l.startswith(begin)] for t in (text, plain))
        assert a and a == b, (a, b)


def test_the_metal_pre_pass_opens_a_sequence_of_its_own(tmp_path, scan):
    """--metal reconstructs the scan once more, after the other two pre-passes: with THR taken from the volume of the run without it, so
    that a few voxels lie above, the volume and the reports are again those of the run on the corrected frames"""
    src, frames, dark, flat = scan
    corrected_set(tmp_path / "fixed", frames, dark, flat, GEO)
    extra = ["--rings", "2:0.01", "--fit-beam-hardening", "2:8:0", "--slabs", 2]
    _, ref = drive(tmp_path / "fixed", tmp_path / "ref", extra)                     # what the metal pre-pass reconstructs
    thr = np.sort(ref.ravel())[-(ref.size // 64)]
    above = int((ref > thr).sum())
    assert 1 <= above <= ref.size // 32
    extra += ["--metal", "%.9g" % thr]
    text, got = drive(src, tmp_path / "lag", ["--lag", OPTION] + extra)
    plain, want = drive(tmp_path / "fixed", tmp_path / "plain", extra)
    assert np.array_equal(bits(got), bits(want)) and not np.array_equal(bits(want), bits(ref))
    for begin in ("ring filter on", "beam hardening on", "metal reduction on"):
        a, b = ([l.split(" s)")[-1] for l in t.splitlines() if l.startswith(begin)] for t in (text, plain))
        assert a and a == b, (a, b)
    for t in (text, plain):
        assert "metal reduction on: %d voxel(s) above %.9g collected" % (above, thr) in t, t


def test_the_cpp_mirror_corrects_as_the_driver_does(tmp_path, scan):
    """PARIS's loop through paris::hip with set_lag_correction(), lag_begin(), lag_correct() and lag_end() (paris_hip_demo --lag), fed
    the counts as f32 and the mean references: the volume of paris.hip --lag, each of its two slabs a sequence of its own"""
    src, frames, dark, flat = scan
    _, want = drive(src, tmp_path / "lag", ["--lag", OPTION, "--lag-start", "rest", "--slabs", 2])
    frames.astype(np.float32).tofile(tmp_path / "in.raw")
    dark.tofile(tmp_path / "dark.raw")
    flat.tofile(tmp_path / "flat.raw")
    out = tmp_path / "demo.raw"
    args = [FF.DEMO] + [str(v) for v in GEO] + [str(N_FRAMES), str(tmp_path / "in.raw"), str(out), "--slabs", "2", "--flat", str(tmp_path / "dark.raw"),
                                               str(tmp_path / "flat.raw"), "1e-05"]
    r = subprocess.run(args + ["--lag", "rest", OPTION], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr + r.stdout
    assert np.array_equal(bits(np.fromfile(out, np.float32).reshape(want.shape)), bits(want))
    r = subprocess.run(args + ["--lag", "steady", "0.5:0.5"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "set_lag_correction()" in r.stderr, r.stderr


def test_refusals_are_made_before_any_device_work(tmp_path, scan):
    src = scan[0]
    out = tmp_path / "bad"
    no_flat = [str(a) for a in [P.EXE, "--geometry", src / "geo.ini", "--input", src / "counts", "--output", out, "--lag", OPTION]]
    cases = [(no_flat, "--lag needs --flat"),
             (command(src, out, ["--lag", OPTION, "--quality", "2"]), "--quality 2"),
             (command(src, out, ["--lag", "0.5:0.5"]), "b_0"),
             (command(src, out, ["--lag", "0.01"]), "cannot read"),
             (command(src, out, ["--lag", "0.01:x"]), "cannot read"),
             (command(src, out, ["--lag", OPTION + ":0.001:0.5"]), "cannot read"),
             (command(src, out, ["--lag", OPTION, "--lag-start", "warm"]), "--lag-start"),
             (command(src, out, ["--lag-start", "rest"]), "--lag-start needs --lag")]
    for args, reason in cases:
        r = subprocess.run(args, capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "Pipeline construction failed" in r.stderr and reason in r.stderr, (args, r.stderr)
    assert "skipped frames" in subprocess.run(cases[1][0], capture_output=True, text=True, timeout=60).stderr
    assert not out.exists()


def test_help_lists_the_flag():
    r = subprocess.run([P.EXE, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--lag B1:A1[:B2:A2[:B3:A3[:B4:A4]]] [--lag-start rest|steady]" in r.stdout
    assert "--lag:" in r.stdout and "Needs --flat" in r.stdout
