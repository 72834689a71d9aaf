"""paris.hip --bin: a scan of u16 counts on a 67 x 45 detector with a dark, a flat and a defect file,
reconstructed with --bin, against the same driver WITHOUT --bin on inputs binned on the host by the numpy rule (tests/binning_rule.py):
f32 frames, references and mask at binned size, with the binned geometry. The volumes are bit-identical, slab by slab as well."""
import subprocess

import numpy as np
import pytest

import binning_rule as R
import test_gpu_flat_field as FF
import test_gpu_paris_hip as P
from oracle import formats as F

pytestmark = pytest.mark.gpu

GEO = (67, 45, 0.2, 0.25, 1.5, -0.75, 100, 200, 10.0)
N_FRAMES = 36


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def write_geometry(path, geo):
    path.write_text("\n".join("%s = %s" % (k, v if isinstance(v, int) else "%.9g" % float(v)) for k, v in zip(FF.GEO_KEYS, geo)) + "\n")
    return path


@pytest.fixture(scope="module")
def scan(tmp_path_factory):
    """the source inputs on disk, and what they hold"""
    root = tmp_path_factory.mktemp("binning_scan")
    rng = np.random.default_rng(17)
    shape = (GEO[1], GEO[0])
    darks = rng.integers(150, 450, (3,) + shape).astype(np.uint16)
    flats = (rng.integers(30000, 60000, shape)[None] + rng.integers(-400, 400, (5,) + shape)).astype(np.uint16)
    darks[:, 20, 21] = flats[:, 20, 21] = 300          # a dead pixel of the references: --defects-from-flat leaves it out of its bin
    dark, flat = FF.mean(darks), FF.mean(flats)
    t = np.exp(-3 * rng.random((N_FRAMES,) + shape))
    frames = np.clip(np.rint(dark + (flat - dark) * t + rng.normal(0, 30, t.shape)), 0, 65535).astype(np.uint16)
    mask = R.shared_mask(*GEO[:2])
    (root / "ref").mkdir()
    (root / "ref" / "dark.his").write_bytes(F.his_file_bytes(darks, 4, 32))
    (root / "ref" / "flat.his").write_bytes(F.his_file_bytes(flats, 4))
    (root / "counts").mkdir()
    (root / "counts" / "a.his").write_bytes(F.his_file_bytes(frames[:20], 4, 32))
    (root / "counts" / "b.his").write_bytes(F.his_file_bytes(frames[20:], 4, 32))
    (root / "mask.raw").write_bytes(mask.tobytes())
    write_geometry(root / "geo.ini", GEO)
    return root, frames, dark, flat, mask


def prebinned(root, scan, bin_x, bin_y):
    """the inputs of the run without --bin: everything binned on the host by the numpy rule"""
    _, frames, dark, flat, mask = scan
    dead = mask.copy()
    dead[20, 21] = 1
    assert mask[20, 21] == 0
    root.mkdir()
    binned = np.stack([R.bin_frame(f.astype(np.float32), bin_x, bin_y, dead) for f in frames])
    (root / "ref").mkdir()
    (root / "ref" / "dark.his").write_bytes(F.his_file_bytes(R.bin_frame(dark, bin_x, bin_y, dead)[None], 128))
    (root / "ref" / "flat.his").write_bytes(F.his_file_bytes(R.bin_frame(flat, bin_x, bin_y, dead)[None], 128))
    (root / "counts").mkdir()
    (root / "counts" / "a.his").write_bytes(F.his_file_bytes(binned, 128, 32))
    small = R.bin_mask(dead, bin_x, bin_y)
    (root / "mask.raw").write_bytes(small.tobytes())
    write_geometry(root / "geo.ini", R.binned_geometry(GEO, bin_x, bin_y))
    return small


def drive(root, out, extra):
    args = [P.EXE, "--geometry", root / "geo.ini", "--input", root / "counts", "--output", out, "--flat", root / "ref" / "flat.his", "--dark",
            root / "ref" / "dark.his", "--defects", root / "mask.raw", "--defects-from-flat"] + extra
    r = subprocess.run([str(a) for a in args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout, F.ddbvf_read(str(out / "vol.ddbvf"))[1]


@pytest.mark.parametrize("option,bin_x,bin_y", [("2", 2, 2), ("4:2", 4, 2)])
def test_bin_equals_the_driver_on_host_binned_inputs(tmp_path, scan, option, bin_x, bin_y):
    src = scan[0]
    small = prebinned(tmp_path / "binned", scan, bin_x, bin_y)
    assert small.any() and not small.all()
    for slabs in (1, 2):   # two slabs: row bands of the binned detector and their source rows
        text, got = drive(src, tmp_path / ("bin%d" % slabs), ["--bin", option, "--slabs", slabs])
        plain, want = drive(tmp_path / "binned", tmp_path / ("pre%d" % slabs), ["--slabs", slabs])
        assert "binning on: %d x %d bins, detector 67 x 45 -> %d x %d, %d binned pixel(s)" % (
            bin_x, bin_y, 67 // bin_x, 45 // bin_y, int(small.sum())) in text, text
        assert "binning on" not in plain
        assert np.abs(want).max() > 0 and got.shape == want.shape
        assert np.array_equal(bits(got), bits(want)), slabs
        # the same map on the device in both runs
        line = [l for l in text.splitlines() if l.startswith("defect map on")]
        assert line and line == [l for l in plain.splitlines() if l.startswith("defect map on")]


def test_bin_frame_by_frame(tmp_path, scan):
    """--batch 1: every frame is binned, corrected and repaired on its own, behind its upload, against the reference of the test above,
    which the driver makes group by group"""
    prebinned(tmp_path / "binned", scan, 2, 2)
    text, got = drive(scan[0], tmp_path / "bin", ["--bin", "2", "--slabs", 2, "--batch", 1])
    _, want = drive(tmp_path / "binned", tmp_path / "pre", ["--slabs", 2])
    assert "binning on: 2 x 2 bins" in text
    assert np.abs(want).max() > 0 and np.array_equal(bits(got), bits(want))


def test_the_later_passes_run_on_binned_frames(tmp_path, scan):
    """--zingers and --rings (whose pre-pass reads the scan once more) see binned frames: the same volume and the same counts as on
    host-binned inputs"""
    prebinned(tmp_path / "binned", scan, 2, 2)
    extra = ["--zingers", "0.5:0.1", "--rings", "2:0.01", "--slabs", 2]
    text, got = drive(scan[0], tmp_path / "bin", ["--bin", "2"] + extra)
    plain, want = drive(tmp_path / "binned", tmp_path / "pre", extra)
    assert np.array_equal(bits(got), bits(want))
    for start in ("zinger filter on", "ring filter on"):
        a, b = ([l.split(" s)")[-1] for l in t.splitlines() if l.startswith(start)] for t in (text, plain))
        assert a and a == b, (a, b)


def test_the_cpp_mirror_bins_as_the_driver_does(tmp_path, scan):
    """PARIS's loop through paris::hip with set_binning(), bin_frame() and binned_geometry() (paris_hip_demo --bin), fed the source
    frames and the host-binned references and map: the volume of paris.hip --bin"""
    src, frames, dark, flat, mask = scan
    small = prebinned(tmp_path / "binned", scan, 2, 2)
    text, want = drive(src, tmp_path / "bin", ["--bin", "2"])
    assert "defect map on: %d defective pixel(s)" % int(small.sum()) in text, text   # (the binned references add no dead pixel)
    dead = mask.copy()
    dead[20, 21] = 1
    frames.astype(np.float32).tofile(tmp_path / "in.raw")
    R.bin_frame(dark, 2, 2, dead).tofile(tmp_path / "dark.raw")
    R.bin_frame(flat, 2, 2, dead).tofile(tmp_path / "flat.raw")
    (tmp_path / "dead.raw").write_bytes(dead.tobytes())
    (tmp_path / "small.raw").write_bytes(small.tobytes())
    out = tmp_path / "demo.raw"
    r = subprocess.run([FF.DEMO] + [str(v) for v in GEO] + [str(N_FRAMES), str(tmp_path / "in.raw"), str(out), "--slabs", "2", "--bin", "2", "2",
                                                           str(tmp_path / "dead.raw"), "--flat", str(tmp_path / "dark.raw"),
                                                           str(tmp_path / "flat.raw"), "1e-05", "--defects", str(tmp_path / "small.raw")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr + r.stdout
    assert np.array_equal(bits(np.fromfile(out, np.float32).reshape(want.shape)), bits(want))
    r = subprocess.run([FF.DEMO] + [str(v) for v in GEO] + [str(N_FRAMES), str(tmp_path / "in.raw"), str(out), "--bin", "2", "3", "none"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "binned_geometry()" in r.stderr, r.stderr


def test_bin_1_is_no_option_and_bad_settings_are_refused_before_any_device_work(tmp_path, scan):
    src = scan[0]
    _, one = drive(src, tmp_path / "one", ["--bin", "1"])
    _, none = drive(src, tmp_path / "none", [])
    assert np.array_equal(bits(one), bits(none))
    for bad in ("3", "2:5", "0", "2:", "16", "x"):
        r = subprocess.run([P.EXE, "--geometry", str(src / "geo.ini"), "--input", str(src / "counts"), "--output", str(tmp_path / "bad"), "--bin", bad],
                           capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "--bin" in r.stderr, (bad, r.stderr)
    assert not (tmp_path / "bad").exists()
