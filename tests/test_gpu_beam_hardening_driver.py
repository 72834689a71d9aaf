"""The beam-hardening correction through the driver (paris.hip --beam-hardening / --fit-beam-hardening): the
volume of given coefficients against the Python chain bit for bit, in one slab and in three, the fitted coefficients against
Backend.fit_beam_hardening on the same frames, the report, and the combinations the driver refuses."""
import re
import subprocess

import numpy as np
import pytest

import beam_hardening_rule as R
import test_gpu_flat_field as FF
import test_gpu_paris_hip as P
from oracle import formats as F
from paris_amd import backend as B
from test_gpu_bh_fit import reconstruct

pytestmark = pytest.mark.gpu

COEFFICIENTS = (np.float32(0.28331566), np.float32(0.3664067))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


@pytest.fixture(scope="module")
def scan(tmp_path_factory):
    """the polychromatic two-ellipsoid scan of the fit's end-to-end test as float line integrals in two HIS files"""
    root = tmp_path_factory.mktemp("bh")
    det = B.DetectorGeometry(*R.SCAN_GEO)
    frames = R.polychromatic(R.path_lengths())
    (root / "geo.ini").write_text("\n".join("%s = %s" % kv for kv in zip(FF.GEO_KEYS, R.SCAN_GEO)) + "\n")
    (root / "in").mkdir()
    (root / "in" / "a.his").write_bytes(F.his_file_bytes(np.stack(frames[:50]), 128, 32))
    (root / "in" / "b.his").write_bytes(F.his_file_bytes(np.stack(frames[50:]), 128))
    return {"root": root, "det": det, "vg": B.calculate_volume_geometry(det), "frames": frames}


def drive(scan, out, extra, ok=True):
    root = scan["root"]
    args = [P.EXE, "--geometry", root / "geo.ini", "--input", root / "in", "--output", root / out] + extra
    r = subprocess.run([str(a) for a in args], capture_output=True, text=True, timeout=300)
    if not ok:
        return r
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout, F.ddbvf_read(str(root / out / "vol.ddbvf"))[1]


ON_LINE = re.compile(r"^beam hardening on: coefficients (\S+)$", re.M)
FIT_LINE = re.compile(r"^beam-hardening fit on: degree (\d+), (\d+) frame\(s\) into slices (\d+) \.\. (\d+) in the pre-pass \((\S+) s\), threshold (\S+), "
                      r"(\d+) object and (\d+) air voxel\(s\), (\d+) not finite, level (\S+), residual (\S+) before and (\S+) after$", re.M)


def reported(stdout):
    return np.array([float(t) for t in ON_LINE.search(stdout).group(1).split(":")], np.float32)


def test_given_coefficients_give_the_volume_of_the_python_chain(scan):
    with B.Backend(0) as be:
        want = reconstruct(be, scan["frames"], scan["det"], scan["vg"], c=COEFFICIENTS)
        plain = reconstruct(be, scan["frames"], scan["det"], scan["vg"])
    value = "%.9g:%.9g" % COEFFICIENTS
    for k, extra in enumerate((["--slabs", 1], ["--slabs", 3], ["--slabs", 2, "--batch", 1])):
        out, got = drive(scan, "given_%d" % k, ["--beam-hardening", value] + extra)
        assert np.array_equal(bits(got), bits(want)), extra
        assert np.array_equal(bits(reported(out)), bits(COEFFICIENTS)) and "beam-hardening fit" not in out
    out, got = drive(scan, "none", ["--slabs", 1])
    assert "beam hardening" not in out and np.array_equal(bits(got), bits(plain)) and not np.array_equal(bits(plain), bits(want))


def test_the_fit_reports_the_coefficients_of_the_python_fit_and_uses_them(scan):
    with B.Backend(0) as be:
        fit = be.fit_beam_hardening(scan["frames"], scan["det"], degree=2, margin=1, slices=(16, 32))
        want = reconstruct(be, scan["frames"], scan["det"], scan["vg"], c=fit.c)
    out, got = drive(scan, "fit", ["--fit-beam-hardening", "2:32:1", "--slabs", 2])
    c = reported(out)
    assert np.array_equal(bits(c), bits(fit.c)), (c, fit.c)
    m = FIT_LINE.search(out)
    assert m is not None, out
    assert [int(m.group(k)) for k in (1, 2, 3, 4, 7, 8, 9)] == [2, R.SCAN_VIEWS, 16, 47, fit.counts.n_object, fit.counts.n_air, 0]
    assert np.float32(m.group(6)) == fit.threshold and abs(float(m.group(10)) - fit.level) <= 1e-8 * abs(fit.level)
    assert abs(float(m.group(11)) - fit.residual_before) < 1e-5 and abs(float(m.group(12)) - fit.residual_after) < 1e-5
    assert np.array_equal(bits(got), bits(want))                       # the main run used them
    # the defaults: 32 slices, margin 2
    out, _ = drive(scan, "fit_default", ["--fit-beam-hardening", "2", "--slabs", 1])
    m = FIT_LINE.search(out)
    assert (m.group(3), m.group(4)) == ("16", "47") and int(m.group(7)) < fit.counts.n_object


@pytest.mark.parametrize("extra,names", [
    (["--beam-hardening", "1:0.1", "--fit-beam-hardening", "2"], ["--beam-hardening", "--fit-beam-hardening"]),
    (["--fit-beam-hardening", "2", "--bin", "2"], ["--fit-beam-hardening", "--bin"]),
    (["--fit-beam-hardening", "2", "--find-axis", "-1:1", "--axis-only"], ["--fit-beam-hardening", "--axis-only"]),
    (["--fit-beam-hardening", "0"], ["--fit-beam-hardening"]),
    (["--fit-beam-hardening", "5"], ["--fit-beam-hardening"]),
    (["--fit-beam-hardening", "2:32:5"], ["--fit-beam-hardening"]),
    (["--fit-beam-hardening", "2:4:2"], ["--fit-beam-hardening"]),
    (["--fit-beam-hardening", "2:65"], ["--fit-beam-hardening", "64 slice"]),
    (["--fit-beam-hardening", "2:x"], ["--fit-beam-hardening"]),
    (["--fit-beam-hardening", "2:32:1:0"], ["--fit-beam-hardening"]),
    (["--beam-hardening", "1"], ["--beam-hardening"]),
    (["--beam-hardening", "1:0:0:0:0"], ["--beam-hardening"]),
    (["--beam-hardening", "1:nan"], ["--beam-hardening"]),
    (["--beam-hardening", "1:"], ["--beam-hardening"]),
])
def test_refused_combinations_are_refused_before_any_output(scan, extra, names):
    r = drive(scan, "refused", extra, ok=False)
    assert r.returncode == 1, r.stdout + r.stderr
    assert "Pipeline construction failed" in r.stderr and all(n in r.stderr for n in names), r.stderr
    assert not (scan["root"] / "refused").exists()
