"""The detector roll through the driver (paris.hip --detector-roll / --find-roll / --roll-only): the volume
against the Python-mirror chain bit for bit -- in one slab and in three, with the row band on and off, a group at a time and frame by
frame -- alone and behind --bin, --defects and --zingers, whose reach widens the roll's source rows; the estimate of the search and
the run that uses it; the C++ mirror; and the combinations the driver refuses."""
import re
import subprocess

import numpy as np
import pytest

import binning_rule as BR
import roll_rule as R
import test_gpu_defect_map as DM
import test_gpu_flat_field as FF
import test_gpu_paris_hip as P
from oracle import formats as F
from paris_amd import backend as B

pytestmark = pytest.mark.gpu

ETA = 1.2
N_VIEWS = 36
SCALE = 1000.0                                         # line integrals of at most 48.5 as u16 counts
GEO = R.geo(delta_s=1.3, n_views=N_VIEWS)              # the 96 x 80 detector
SRC_GEO = R.geo(192, 160, 0.6, 0.5, delta_s=2.6, delta_t=1.4, n_views=N_VIEWS)   # the same detector at twice the pixels, for --bin 2
ZINGERS = (0.5 * SCALE / 10, 0.1)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def write_geometry(path, geo):
    path.write_text("\n".join("%s = %s" % (k, v if isinstance(v, int) else "%.9g" % float(v)) for k, v in zip(FF.GEO_KEYS, geo)) + "\n")


def counts(geo):
    return np.rint(R.sphere_frames(geo, ETA) * SCALE).astype(np.uint16)


@pytest.fixture(scope="module")
def scan(tmp_path_factory):
    """u16 frames of the recovery spheres on the detector rolled by 1.2 degrees, in two HIS files; the same at 192 x 160 with a mask"""
    root = tmp_path_factory.mktemp("roll_scan")
    frames, wide = counts(GEO), counts(SRC_GEO)
    rng = np.random.default_rng(3)
    for f in wide:                                      # a few bright outliers for the zinger filter, away from the mask's pixels
        f[rng.integers(4, 156, 6), rng.integers(4, 188, 6)] = 60000
    mask = BR.shared_mask(192, 160)
    for name, g, fr in (("plain", GEO, frames), ("wide", SRC_GEO, wide)):
        (root / name).mkdir()
        (root / name / "a.his").write_bytes(F.his_file_bytes(fr[:20], 4, 32))
        (root / name / "b.his").write_bytes(F.his_file_bytes(fr[20:], 4))
        write_geometry(root / (name + ".ini"), g)
    (root / "mask.raw").write_bytes(mask.tobytes())
    return {"root": root, "frames": frames, "wide": wide, "mask": mask}


def drive(scan, name, out, extra, ok=True):
    root = scan["root"]
    args = [P.EXE, "--geometry", root / (name + ".ini"), "--input", root / name, "--output", root / out] + extra
    r = subprocess.run([str(a) for a in args], capture_output=True, text=True, timeout=300)
    if not ok:
        return r
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout, F.ddbvf_read(str(root / out / "vol.ddbvf"))[1]


def python_chain(frames, det, prepare=None, eta=ETA):
    """PARIS's loop through the Backend: every frame uploaded as stored, through `prepare`, rolled into a second buffer, weighted,
    filtered and backprojected"""
    vg = B.calculate_volume_geometry(det)
    with B.Backend(0, synchronous=False) as qbe:
        qbe.set_paris_loop_defaults(48)
        if prepare is not None:
            prepare(qbe, None)      # the settings
        if eta is not None:
            qbe.set_detector_roll(eta, det)
        v = qbe.make_volume_device(vg.dim_x, vg.dim_y, vg.dim_z)
        for i, fr in enumerate(frames):
            d_p = prepare(qbe, fr) if prepare is not None else qbe.make_projection_device(det.n_row, det.n_col)
            if prepare is None:
                qbe.upload_raw(fr, d_p)
            if eta is not None:
                rolled = qbe.make_projection_device(det.n_row, det.n_col)
                qbe.detector_roll(d_p, rolled)
                qbe.free(d_p)
                d_p = rolled
            d_p.idx = i
            B.weight(qbe, d_p, det)
            B.filter(qbe, d_p, det)
            B.backproject(qbe, d_p, v, 0, det, vg, False, False, None)
            qbe.free(d_p)
        qbe.flush()
        return DM.volume_to_host(qbe, v, vg).reshape(vg.dim_z, vg.dim_y, vg.dim_x)


ROLL_LINE = re.compile(r"^detector roll on: (\S+) deg$", re.M)
SEARCH_LINE = re.compile(r"^roll search on: eta = (\S+) deg, candidate (\d+) of (\d+) at step (\S+), J_min = (\S+), J_median = (\S+), J_min / J_median = (\S+), "
                         r"(\d+) candidate\(s\) scored, (\d+) pair\(s\) skipped, margins (\d+) x (\d+), (\d+) frame\(s\) in the pre-pass", re.M)


def test_the_volume_is_the_python_chain_s_in_slabs_and_bands(scan):
    det = B.DetectorGeometry(*GEO)
    want = python_chain(scan["frames"], det)
    plain = python_chain(scan["frames"], det, eta=None)
    assert np.abs(want).max() > 0 and not np.array_equal(bits(want), bits(plain))
    for k, extra in enumerate((["--slabs", 1], ["--slabs", 3], ["--slabs", 1, "--no-row-band"], ["--slabs", 3, "--no-row-band"],
                               ["--slabs", 2, "--batch", 1])):
        out, got = drive(scan, "plain", "roll_%d" % k, ["--detector-roll", ETA] + extra)
        assert got.shape == want.shape and np.array_equal(bits(got), bits(want)), extra
        assert np.float32(ROLL_LINE.search(out).group(1)) == np.float32(ETA) and "roll search" not in out
    out, got = drive(scan, "plain", "none", ["--slabs", 3])
    assert "detector roll" not in out and np.array_equal(bits(got), bits(plain))


def test_behind_binning_repair_and_zingers_the_bands_widen_and_the_volume_stays(scan):
    """--bin 2 --defects --zingers in front of the roll: the rows a slab uploads, bins, repairs and filters are the roll's source range
    widened by the repair's reach and the zinger row"""
    mask = scan["mask"]
    det = B.binned_geometry(2, 2, B.DetectorGeometry(*SRC_GEO))
    small = B.bin_mask(2, 2, mask)
    assert small.any() and (det.n_row, det.n_col) == (96, 80)

    def prepare(qbe, fr):
        if fr is None:
            qbe.set_binning(2, 2, 192, 160, mask)
            qbe.set_defect_map(small)
            qbe.set_zinger_filter(ZINGERS[0], ZINGERS[1], "bright", 96, 80)
            return None
        src = qbe.make_projection_device(192, 160)
        d_p = qbe.make_projection_device(96, 80)
        qbe.upload_raw(fr, src)
        qbe.bin_frames(src, d_p)
        qbe.free(src)
        qbe.defect_repair_rows(d_p)
        qbe.zinger_filter_rows(d_p)
        return d_p

    want = python_chain(scan["wide"], det, prepare)
    chain = ["--bin", 2, "--defects", scan["root"] / "mask.raw", "--zingers", "%g:%g" % ZINGERS, "--detector-roll", ETA]
    for k, extra in enumerate((["--slabs", 1], ["--slabs", 3], ["--slabs", 3, "--no-row-band"], ["--slabs", 3, "--batch", 1])):
        out, got = drive(scan, "wide", "chain_%d" % k, chain + extra)
        assert got.shape == want.shape and np.array_equal(bits(got), bits(want)), extra
        assert "zinger filter on" in out and "defect map on" in out and "binning on" in out
        replaced = int(re.search(r"(\d+) pixel\(s\) replaced", out).group(1))
        assert replaced > 0


def test_find_roll_prints_the_estimate_and_the_run_uses_it(scan):
    out = drive(scan, "plain", "only", ["--find-roll", "-3:3:0.25", "--roll-only"], ok=False)
    assert out.returncode == 0, out.stdout + out.stderr
    m = SEARCH_LINE.search(out.stdout)
    assert m is not None, out.stdout
    eta = float(m.group(1))
    print("detector roll, driver: estimate %.4f for a roll of %.1f, J_min / J_median %s" % (eta, ETA, m.group(7)))
    assert abs(eta - ETA) <= R.BOUND_DEG
    assert (int(m.group(3)), int(m.group(8)), int(m.group(9)), int(m.group(12))) == (25, 25, 0, N_VIEWS)
    assert "warning" not in out.stdout and "volume" not in out.stdout and not (scan["root"] / "only").exists()
    # the device's search on the mean of the frames as the driver uploads them
    with B.Backend(0) as be:
        res, cost, pairs = be.find_detector_roll(scan["frames"].astype(np.float64).mean(axis=0), -3.0, 0.25, 25, B.DetectorGeometry(*GEO))
    assert abs(res.eta_deg - eta) <= 1e-3
    # the whole run: the search, then the reconstruction with its estimate
    text, got = drive(scan, "plain", "found", ["--find-roll", "-3:3:0.25", "--slabs", 2])
    used = ROLL_LINE.search(text).group(1)
    assert float(SEARCH_LINE.search(text).group(1)) == pytest.approx(float(used), abs=1e-4)
    _, want = drive(scan, "plain", "given", ["--detector-roll", used, "--slabs", 2])
    assert np.array_equal(bits(got), bits(want))
    # a range that excludes the truth: the warning
    out = drive(scan, "plain", "edge", ["--find-roll", "-3:0:0.5", "--roll-only"], ok=False)
    assert out.returncode == 0 and "widen the range of --find-roll" in out.stdout


def test_the_cpp_mirror_rolls_as_the_driver_does(tmp_path, scan):
    _, want = drive(scan, "plain", "mirror", ["--detector-roll", ETA, "--slabs", 2])
    scan["frames"].astype(np.float32).tofile(tmp_path / "in.raw")
    out = tmp_path / "demo.raw"
    r = subprocess.run([FF.DEMO] + [str(v) for v in GEO] + [str(N_VIEWS), str(tmp_path / "in.raw"), str(out), "--slabs", "2", "--detector-roll", str(ETA)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr + r.stdout
    assert np.array_equal(bits(np.fromfile(out, np.float32).reshape(want.shape)), bits(want))
    r = subprocess.run([FF.DEMO] + [str(v) for v in GEO] + [str(N_VIEWS), str(tmp_path / "in.raw"), str(out), "--detector-roll", "0"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "set_detector_roll()" in r.stderr, r.stderr


@pytest.mark.parametrize("extra,names", [
    (["--find-roll", "-3:3", "--short-scan"], ["--find-roll", "--short-scan"]),
    (["--find-roll", "-3:3", "--offset-detector"], ["--find-roll", "--offset-detector"]),
    (["--find-roll", "-3:3", "--detector-roll", "1"], ["--find-roll", "--detector-roll"]),
    (["--find-roll", "-3:3", "--fit-beam-hardening", "2"], ["--find-roll", "--fit-beam-hardening"]),
    (["--find-roll", "-11:3"], ["--find-roll"]),
    (["--find-roll", "3:-3"], ["--find-roll"]),
    (["--find-roll", "-3:3:0.01"], ["--find-roll", "256"]),
    (["--find-roll", "-3"], ["--find-roll"]),
    (["--find-roll", "-3:x"], ["--find-roll"]),
    (["--roll-only"], ["--roll-only", "--find-roll"]),
    (["--detector-roll", "0"], ["--detector-roll"]),
    (["--detector-roll", "10.5"], ["--detector-roll"]),
    (["--detector-roll", "nan"], ["--detector-roll"]),
    (["--detector-roll", "1x"], ["--detector-roll"]),
])
def test_refused_combinations_are_refused_before_any_output(scan, extra, names):
    r = drive(scan, "plain", "refused", extra, ok=False)
    assert r.returncode == 1, r.stdout + r.stderr
    assert "Pipeline construction failed" in r.stderr and all(n in r.stderr for n in names), r.stderr
    assert not (scan["root"] / "refused").exists()
