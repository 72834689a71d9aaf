"""Offset detectors on the host: paris_hip_offset_detector_check against a float64 restatement of its contract, the refusals of
paris.hip --offset-detector, which come before any device work, and the calibration of the quality bounds the GPU tests pin:
analytic half-fan projections weighted by a float64 restatement of the weight, filtered and backprojected by the oracle, against a
centred detector as wide as the extended field of view (no GPU needed)."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import phantom
from oracle import formats as F
from paris_amd import _lib
from paris_amd import backend as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "paris_amd", "host", "demo", "paris.hip")
GEO_KEYS = ("n_row", "n_col", "l_px_row", "l_px_col", "delta_s", "delta_t", "d_so", "d_od", "delta_phi")

# The calibration scans: 360 one-degree views, 500 / 500 mm, 0.8 mm pixels. The half fan has 128 columns at delta_s = +-40 (an
# extended field of view of 104 columns' half-width), the reference a centred detector of 208 columns.
CAL_N_COL = 32
# Measured by test_calibration_against_the_centred_detector with the oracle (both signs of delta_s agree to 1e-4):
CAL_RMS = 0.1953          # relative RMS of the weighted half fan against the reference (the unweighted one: 0.607)
CAL_INSIDE = 2.7e-3       # max |weighted - reference| inside the overlap, relative to max |reference| (unweighted: 0.43)
CAL_OUTSIDE = 0.329       # mean (weighted - reference) / mean reference outside the overlap (unweighted: 0.335)
BOUND = 1.3               # the pinned bounds: this many times the oracle's figures


def f64(x):
    return float(np.float32(x))


def overlap(det):
    """(tau [mm], gamma_tau [rad], sigma) of the contract in float64 from the float32 fields"""
    l, n = f64(det.l_px_row), det.n_row
    d_sd = abs(f64(det.d_so)) + abs(f64(det.d_od))
    t_half = n * l / 2 + f64(det.delta_s) * l
    tau = min(t_half, n * l - t_half)
    return tau, math.atan(tau / d_sd), 1.0 if f64(det.delta_s) <= 0 else -1.0


def twice_weight(det):
    """2 w of every column in float64"""
    l, n = f64(det.l_px_row), det.n_row
    d_sd = abs(f64(det.d_so)) + abs(f64(det.d_od))
    t = (np.arange(n) + 0.5) * l - (n * l / 2 + f64(det.delta_s) * l)
    _, g_tau, sigma = overlap(det)
    x = sigma * np.arctan(t / d_sd) / g_tau
    return np.where(x >= 1, 2.0, np.where(x <= -1, 0.0, 2 * np.sin(math.pi / 4 * (1 + np.clip(x, -1, 1))) ** 2))


@pytest.mark.parametrize("n_row,delta_s", [(128, -40.0), (128, 40.0), (128, -40.5), (128, 20.25), (128, 0.0), (2048, -700.0),
                                           (2048, 700.0), (2048, 0.0)])
def test_check_matches_float64(n_row, delta_s):
    det = B.DetectorGeometry(n_row, 96, 0.8 if n_row == 128 else 0.2, 0.8, delta_s, 1.0, 500, 500, 1.0)
    g = B.offset_detector_check(det)
    assert g == pytest.approx(math.degrees(overlap(det)[1]), rel=1e-6)


def test_accepts_two_pixels_of_overlap_and_refuses_just_below():
    for n_row, l in ((128, 0.8), (2048, 0.2), (333, 0.127)):
        edge = n_row / 2 - 2                                 # tau = (n_row / 2 - |delta_s|) l = 2 l
        for sign in (-1.0, 1.0):
            det = B.DetectorGeometry(n_row, 64, l, l, sign * edge, 0.0, 500, 500, 1.0)
            tau, _, _ = overlap(det)
            assert tau == pytest.approx(2 * f64(l), rel=1e-12)
            B.offset_detector_check(det)
            beyond = float(np.nextafter(np.float32(sign * edge), np.float32(sign * 1e9)))
            with pytest.raises(B.ParisHipError) as e:
                B.offset_detector_check(B.DetectorGeometry(n_row, 64, l, l, beyond, 0.0, 500, 500, 1.0))
            assert e.value.status == _lib.ERROR_INVALID_ARGUMENT


def test_refuses_degenerate_and_non_finite_geometry():
    good = (128, 96, 0.8, 0.8, -40.0, 0.0, 500, 500, 1.0)
    B.offset_detector_check(B.DetectorGeometry(*good))
    for k, v in ((0, 0), (2, float("nan")), (2, float("inf")), (2, 0.0), (2, -0.8), (4, float("nan")), (4, float("inf")),
                 (4, -64.0), (4, 70.0), (6, float("inf")), (7, float("nan"))):
        g = list(good)
        g[k] = v
        with pytest.raises(B.ParisHipError):
            B.offset_detector_check(B.DetectorGeometry(*g))
    with pytest.raises(B.ParisHipError):
        B.offset_detector_check(B.DetectorGeometry(128, 96, 0.8, 0.8, -40.0, 0.0, 0, 0, 1.0))   # d_sd = 0
    L = _lib.load()
    det = B.DetectorGeometry(128, 96, 0.8, 0.8, -63.0, 0.0, 500, 500, 1.0)                      # tau = 1 pixel
    g = C.c_float(-1.0)
    assert L.paris_hip_offset_detector_check(C.byref(det), C.byref(g)) == _lib.ERROR_INVALID_ARGUMENT
    assert g.value == pytest.approx(math.degrees(overlap(det)[1]), rel=1e-6)                     # reported for a refused geometry too
    assert L.paris_hip_offset_detector_check(None, C.byref(g)) == _lib.ERROR_INVALID_ARGUMENT
    assert L.paris_hip_offset_detector_check(C.byref(B.DetectorGeometry(*good)), None) == 0


def test_weight_restatement_properties():
    """the float64 table the GPU tests compare against: 2 beyond the overlap, conjugate columns add up to 2"""
    det = B.DetectorGeometry(128, 96, 0.8, 0.8, -40.5, 0.0, 500, 500, 1.0)
    w2 = twice_weight(det)
    n, ds = det.n_row, f64(det.delta_s)
    i = np.arange(n)
    j = (n - 1 + 2 * ds - i).astype(int)                       # the column at -t
    ok = (j >= 0) & (j < n)
    assert np.abs(w2[i[ok]] + w2[j[ok]] - 2).max() < 1e-12
    tau, _, _ = overlap(det)
    t = (i + 0.5) * f64(det.l_px_row) - (n * f64(det.l_px_row) / 2 + ds * f64(det.l_px_row))
    assert (w2[t >= tau] == 2).all() and (w2[t <= -tau] == 0).all() and ((w2 > 0) & (w2 < 2)).sum() >= 40


# ---- the driver's refusals -----------------------------------------------------------------------------------------------------

DRV_GEO = (64, 48, 0.2, 0.25, -16.0, -0.75, 100, 200, 1.0)


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


def test_driver_refuses_a_short_scan_and_a_detector_without_overlap(tmp_path):
    ini, _ = write_set(tmp_path / "in", DRV_GEO, 360)
    r = run_driver(["--geometry", ini, "--input", tmp_path / "in", "--output", tmp_path / "out", "--offset-detector", "--short-scan"])
    assert r.returncode == 1 and "--offset-detector and --short-scan" in r.stderr, r.stderr
    geo = list(DRV_GEO)
    geo[4] = -31.5                                          # tau = 0.5 pixels
    ini.write_text("\n".join("%s = %s" % kv for kv in zip(GEO_KEYS, geo)) + "\n")
    r = run_driver(["--geometry", ini, "--input", tmp_path / "in", "--output", tmp_path / "out", "--offset-detector"])
    assert r.returncode == 1 and "0.5000 pixels" in r.stderr and "at least 2" in r.stderr, r.stderr
    geo[4] = 33.0                                           # the central ray misses the detector
    ini.write_text("\n".join("%s = %s" % kv for kv in zip(GEO_KEYS, geo)) + "\n")
    r = run_driver(["--geometry", ini, "--input", tmp_path / "in", "--output", tmp_path / "out", "--offset-detector"])
    assert r.returncode == 1 and "-1.0000 pixels" in r.stderr, r.stderr
    assert not (tmp_path / "out").exists()                  # refused before the output was set up, let alone a device


def test_driver_refuses_less_than_a_circle_and_non_monotonic_angles(tmp_path):
    # 180 frames at 1 degree: 179 degrees plus one step
    ini, _ = write_set(tmp_path / "in", DRV_GEO, 180)
    r = run_driver(["--geometry", ini, "--input", tmp_path / "in", "--output", tmp_path / "out", "--offset-detector"])
    assert r.returncode == 1 and "180.0000 degrees" in r.stderr and "360" in r.stderr, r.stderr
    angles = [2.0 * k for k in range(180)]                  # 358 + 2: a full circle
    angles[40], angles[41] = angles[41], angles[40]
    ang = tmp_path / "angles.txt"
    ang.write_text("\n".join(repr(a) for a in angles))
    r = run_driver(["--geometry", ini, "--input", tmp_path / "in", "--output", tmp_path / "out", "--offset-detector", "--angles", ang])
    assert r.returncode == 1 and "not monotonic" in r.stderr and "frame 41" in r.stderr, r.stderr
    # descending, but short by more than half a step: 180 frames 1.99 degrees apart cover 356.21 + 1.99 = 358.2
    ang.write_text("\n".join(repr(-1.99 * k) for k in range(180)))
    r = run_driver(["--geometry", ini, "--input", tmp_path / "in", "--output", tmp_path / "out", "--offset-detector", "--angles", ang])
    assert r.returncode == 1 and "358.2000 degrees" in r.stderr, r.stderr
    assert not (tmp_path / "out").exists()


# ---- the calibration of the quality bounds -------------------------------------------------------------------------------------

def cal_geometry(n_row, delta_s):
    return (n_row, CAL_N_COL, 0.8, 0.8, delta_s, 0.0, 500.0, 500.0, 1.0)


def central_slices(dim_z):
    return 3 * dim_z // 8, 5 * dim_z // 8


def rel_rms(got, ref, scale=None):
    """over the given slices, inside 0.45 dim_x of the axis; scale None: the best scale for got (tests/test_gpu_short_scan.py)"""
    dz, dy, dx = ref.shape
    y, x = np.mgrid[:dy, :dx]
    mask = np.hypot(x - (dx - 1) / 2, y - (dy - 1) / 2) <= 0.45 * dx
    a = got[:, mask].astype(np.float64)
    b = ref[:, mask].astype(np.float64)
    if scale is None:
        scale = (a * b).sum() / (a * a).sum()
    return float(np.sqrt(((scale * a - b) ** 2).mean() / (b ** 2).mean()))


def structure(got, ref, det, vg):
    """(max |got - ref| inside the overlap / max |ref|, mean (got - ref) / mean ref outside it): inside are the voxels whose ray stays
    within |t| < tau at every angle (radius below d_so sin gamma_tau), less a margin of 2 voxels; outside, those 2 voxels beyond it
    and inside 0.45 dim_x"""
    dz, dy, dx = ref.shape
    y, x = np.mgrid[:dy, :dx]
    rho = np.hypot(x - (dx - 1) / 2, y - (dy - 1) / 2) * vg.l_vx_x
    rho_tau = abs(f64(det.d_so)) * math.sin(overlap(det)[1])
    inside = rho <= rho_tau - 2 * vg.l_vx_x
    outside = (rho >= rho_tau + 2 * vg.l_vx_x) & (rho <= 0.45 * dx * vg.l_vx_x)
    d = got.astype(np.float64) - ref
    return float(np.abs(d[:, inside]).max() / np.abs(ref).max()), float(d[:, outside].mean() / ref[:, outside].astype(np.float64).mean())


def cal_volume_geometry(B_or_O):
    """the half fan's grid, which both scans use (the centred detector's rounds to one voxel more)"""
    return B_or_O.calculate_volume_geometry(B_or_O.DetectorGeometry(*cal_geometry(128, -40.0)))


def cal_radius(vg):
    """between the centred 128-column field of view (25.6 mm) and the extended one (41 mm)"""
    return 0.9 * vg.dim_x * vg.l_vx_x / 2


def cal_frame(n_row, delta_s, i, radius):
    return phantom.projection(n_row, CAL_N_COL, 0.8, 0.8, 500.0, 500.0, f64(np.float32(i) * np.float32(1.0)), radius, delta_s)


def oracle_reconstruct(oracle, n_row, delta_s, weighted):
    det = oracle.DetectorGeometry(*cal_geometry(n_row, delta_s))
    vg = cal_volume_geometry(oracle)
    z0, z1 = central_slices(vg.dim_z)
    w2 = twice_weight(det).astype(np.float32)
    fs = oracle.filter_size(n_row)
    k = oracle.make_filter(fs, det.l_px_row)
    vol = np.zeros((z1 - z0, vg.dim_y, vg.dim_x), np.float32)
    for i in range(360):
        p = cal_frame(n_row, delta_s, i, cal_radius(vg))
        if weighted:
            p = p * w2[None, :]                                   # the device's product: float32 frame times the float32 2 w
        p = np.ascontiguousarray(p, np.float32)
        oracle.weight(p, det)
        oracle.apply_filter(p, k, fs)
        s, c, ds, dt = oracle.backproject_constants(det, i)
        oracle.backproject(vol, p, z0, det, vg, s, c, ds, dt)
    return vol


def test_calibration_against_the_centred_detector(oracle):
    vg = cal_volume_geometry(oracle)
    assert 25.6 < cal_radius(vg) < 41.0
    ref = oracle_reconstruct(oracle, 208, 0.0, False)
    det = oracle.DetectorGeometry(*cal_geometry(128, -40.0))
    figures = {}
    for ds in (-40.0, 40.0):
        got = oracle_reconstruct(oracle, 128, ds, True)
        figures[ds] = (rel_rms(got, ref, 1.0),) + structure(got, ref, det, vg)
    unweighted = oracle_reconstruct(oracle, 128, -40.0, False)
    figures["unweighted"] = (rel_rms(unweighted, ref, 1.0),) + structure(unweighted, ref, det, vg)
    print("offset detector calibration (relative RMS, inside max, outside mean): %s"
          % ", ".join("%s %.4f %.2e %.4f" % ((k,) + v) for k, v in figures.items()))
    for ds in (-40.0, 40.0):
        rms, inside, outside = figures[ds]
        assert rms == pytest.approx(CAL_RMS, rel=0.02)
        assert inside <= CAL_INSIDE * BOUND and inside == pytest.approx(CAL_INSIDE, rel=0.2)
        assert outside == pytest.approx(CAL_OUTSIDE, rel=0.02)
    rms, inside, _ = figures["unweighted"]
    assert rms >= 2.5 * CAL_RMS
    assert inside > 10 * CAL_INSIDE * BOUND
