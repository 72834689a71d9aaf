"""Short scans on the host: paris_hip_short_scan_check against a float64 restatement of its contract, and the refusals of
paris.hip --short-scan, which come before any device work (no GPU needed)."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from oracle import formats as F
from paris_amd import _lib
from paris_amd import backend as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "paris_amd", "host", "demo", "paris.hip")
GEO_KEYS = ("n_row", "n_col", "l_px_row", "l_px_col", "delta_s", "delta_t", "d_so", "d_od", "delta_phi")


def gamma_max(det):
    """gamma_m [rad]: the largest |atan(t / d_sd)| over the two outermost pixel centres, t in the backprojector's coordinates"""
    l, n, ds = float(np.float32(det.l_px_row)), det.n_row, float(np.float32(det.delta_s))
    d_sd = abs(float(np.float32(det.d_so))) + abs(float(np.float32(det.d_od)))
    t = np.array([0.5, n - 0.5]) * l - n * l / 2 - ds * l
    return float(np.abs(np.arctan(t / d_sd)).max())


def minimal_range(det):
    """the smallest float32 range [deg] a float64 reading of the contract accepts, and the float32 just below it"""
    need = math.pi + 2 * gamma_max(det)
    r = np.float32(need * 180 / math.pi)
    while float(r) * math.pi / 180 - math.pi < 2 * gamma_max(det):
        r = np.nextafter(r, np.float32(np.inf))
    return float(r), float(np.nextafter(r, np.float32(-np.inf)))


@pytest.mark.parametrize("delta_s", [0.0, 3.5, -7.25])
def test_gamma_max_includes_the_detector_offset(delta_s):
    det = B.DetectorGeometry(128, 96, 0.8, 0.8, delta_s, 1.0, 500, 500, 1.0)
    g = B.short_scan_check(det, 37.0, 360.0)
    assert g == pytest.approx(math.degrees(gamma_max(det)), rel=1e-6)
    if delta_s:
        assert g > math.degrees(gamma_max(B.DetectorGeometry(128, 96, 0.8, 0.8, 0.0, 1.0, 500, 500, 1.0)))


@pytest.mark.parametrize("geo", [(128, 128, 0.8, 0.8, 0.0, 0.0, 500, 500, 1.0), (128, 128, 0.8, 0.8, 3.5, 0.0, 500, 500, 1.0),
                                 (2048, 2048, 0.2, 0.2, 0.0, 0.0, 500, 500, 0.25), (64, 48, 0.2, 0.25, 1.5, -0.75, 100, 200, 1.0)])
def test_accepts_the_minimal_range_and_refuses_just_below(geo):
    det = B.DetectorGeometry(*geo)
    ok, below = minimal_range(det)
    B.short_scan_check(det, 37.0, ok)
    B.short_scan_check(det, -412.5, ok)   # the start is any angle
    with pytest.raises(B.ParisHipError) as e:
        B.short_scan_check(det, 37.0, below)
    assert e.value.status == _lib.ERROR_INVALID_ARGUMENT


def test_refuses_more_than_a_circle_and_non_finite_values():
    det = B.DetectorGeometry(128, 128, 0.8, 0.8, 0.0, 0.0, 500, 500, 1.0)
    B.short_scan_check(det, 0.0, 360.0)
    for start, rng in ((0.0, float(np.nextafter(np.float32(360), np.float32(400)))), (0.0, 400.0), (float("nan"), 200.0),
                       (0.0, float("nan")), (float("inf"), 200.0), (0.0, float("inf")), (0.0, 90.0), (0.0, -200.0)):
        with pytest.raises(B.ParisHipError):
            B.short_scan_check(det, start, rng)
    L = _lib.load()
    g = C.c_float(-1.0)
    assert L.paris_hip_short_scan_check(C.byref(det), C.byref(B.ShortScan(0.0, 90.0)), C.byref(g)) == _lib.ERROR_INVALID_ARGUMENT
    assert g.value == pytest.approx(math.degrees(gamma_max(det)), rel=1e-6)   # reported for a refused scan too
    assert L.paris_hip_short_scan_check(None, C.byref(B.ShortScan(0.0, 200.0)), None) == _lib.ERROR_INVALID_ARGUMENT
    assert L.paris_hip_short_scan_check(C.byref(det), None, None) == _lib.ERROR_INVALID_ARGUMENT


def write_set(d, geo, n_frames, angles=None):
    d.mkdir()
    fr = np.full((n_frames, geo[1], geo[0]), 1000, np.uint16)
    (d / "scan.his").write_bytes(F.his_file_bytes(fr, 4, 32))
    ini = d.parent / "geo.ini"
    ini.write_text("\n".join("%s = %s" % kv for kv in zip(GEO_KEYS, geo)) + "\n")
    if angles is None:
        return ini, None
    ang = d.parent / "angles.txt"
    ang.write_text("\n".join(repr(float(a)) for a in angles))
    return ini, ang


def run_driver(args):
    if not os.path.exists(EXE):
        pytest.fail("%s missing: run __graft_entry__.build()" % EXE)
    return subprocess.run([EXE] + [str(a) for a in args], capture_output=True, text=True, timeout=120)


def test_driver_refuses_an_insufficient_range_before_device_work(tmp_path):
    geo = (64, 48, 0.2, 0.25, 1.5, -0.75, 100, 200, 1.0)
    g = math.degrees(gamma_max(B.DetectorGeometry(*geo)))
    # 180 frames at 1 degree: 179 degrees from the first to the last, short of 180 + 2 gamma_m
    ini, _ = write_set(tmp_path / "in", geo, 180)
    r = run_driver(["--geometry", ini, "--input", tmp_path / "in", "--output", tmp_path / "out", "--short-scan"])
    assert r.returncode == 1, r.stdout + r.stderr
    need = 180 + 2 * g
    assert "179.0000 degrees" in r.stderr and ("%.4f" % need) in r.stderr and ("%.4f degrees short" % (need - 179)) in r.stderr, r.stderr
    assert not (tmp_path / "out").exists()   # refused before the output was set up, let alone a device
    # --quality 2 keeps every other frame: still 178 degrees
    r = run_driver(["--geometry", ini, "--input", tmp_path / "in", "--output", tmp_path / "out", "--short-scan", "--quality", 2])
    assert r.returncode == 1 and "178.0000 degrees" in r.stderr, r.stderr


def test_driver_refuses_non_monotonic_angles_and_more_than_a_circle(tmp_path):
    geo = (64, 48, 0.2, 0.25, 1.5, -0.75, 100, 200, 1.0)
    angles = list(range(0, 200, 2))
    angles[40], angles[41] = angles[41], angles[40]
    ini, ang = write_set(tmp_path / "in", geo, len(angles), angles)
    r = run_driver(["--geometry", ini, "--input", tmp_path / "in", "--output", tmp_path / "out", "--short-scan", "--angles", ang])
    assert r.returncode == 1 and "not monotonic" in r.stderr and "frame 41" in r.stderr, r.stderr
    # repeated angle
    ang.write_text("\n".join(repr(float(a)) for a in [0.0, 5.0, 5.0] + [10.0 + k for k in range(len(angles) - 3)]))
    r = run_driver(["--geometry", ini, "--input", tmp_path / "in", "--output", tmp_path / "out", "--short-scan", "--angles", ang])
    assert r.returncode == 1 and "not monotonic" in r.stderr, r.stderr
    # descending over more than 360 degrees
    ang.write_text("\n".join(repr(-4.0 * k) for k in range(len(angles))))
    r = run_driver(["--geometry", ini, "--input", tmp_path / "in", "--output", tmp_path / "out", "--short-scan", "--angles", ang])
    assert r.returncode == 1 and "396.0000 degrees, more than 360" in r.stderr, r.stderr
    assert not (tmp_path / "out").exists()
