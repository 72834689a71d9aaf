"""The forward projector's statement on the host (no GPU needed): the float64 restatement of tests/forward_model.py against
analytic line integrals of Gaussian blobs and against the analytic projections of tests/phantom.py, the additivity of disjoint slabs,
and what fp32 arithmetic costs the same statement (FP32_CAL, the figure the GPU tests bound the device with)."""
import numpy as np
import pytest

import forward_model as M
import phantom
from paris_amd import backend as B

ANGLES = (0.0, 30.0, 45.0, 90.0, 137.0, 200.0, 225.0, 315.0)
# Measured by test_restatement_against_analytic_line_integrals for the blob configuration of forward_model.py (128 x 160 pixels of
# 1.0 x 0.8 mm, offsets (5, -2), a 96 x 104 x 88 grid of 0.5 mm voxels, blobs of sigma 4.1 to 8.2 voxels), the largest over ANGLES.
# The error is the bilinear smoothing of the blobs, not rounding:
CAL_MAX = 5.64e-3         # max |restatement - analytic| over max |analytic|     (per angle: 3.9e-3 ... 5.6e-3)
CAL_RMS = 2.60e-3         # relative RMS                                          (per angle: 1.9e-3 ... 2.6e-3)
BOUND = 1.3               # the pinned bounds: this many times the measured figures (as tests/test_offset_detector_host.py)
# The same volume mirrored in x gives 6.1e-2 (at 0 degrees, where the mirror moves the blobs along the rays) to 0.90 of the maximum;
# delta_s with the opposite sign 0.70 to 0.82.

# max |fp32 transcription - float64 restatement| over max |restatement| on the uniform random volume of forward_model.random_volume,
# by grid size n (detector n x 5 n / 4), the largest over the angles the GPU tests use. 64 and 256: all of 0, 30, 45, 90, 137, 315
# degrees (worst at 45); 512: 45 and 200 degrees, every pixel (50 to 75 s per view and dtype in numpy: test_fp32_figure re-measures
# 16 rows of it).
FP32_CAL = {64: 1.480e-5, 256: 8.161e-6, 512: 8.111e-6}


def errors(got, want):
    d = got.astype(np.float64) - want
    return np.abs(d).max() / np.abs(want).max(), float(np.sqrt((d * d).sum() / (want * want).sum()))


def blob_errors(vol, delta_s_mm=None):
    det, vg = M.blob_geometry(B)
    ds, dt = M.offsets_mm(det)
    out = []
    for phi in ANGLES:
        s, c = M.view_sin_cos(phi)
        got = M.forward_project(vol, 0, det, vg, s, c, ds if delta_s_mm is None else delta_s_mm, dt)
        out.append(errors(got, M.blob_line_integrals(det, s, c, ds, dt)))
    return out


def test_restatement_against_analytic_line_integrals():
    det, vg = M.blob_geometry(B)
    assert det.n_col != det.n_row and det.l_px_col != det.l_px_row and det.delta_s != 0 and det.delta_t != 0
    figures = blob_errors(M.blob_volume(vg))
    print("forward restatement against analytic blobs (max over max, relative RMS): %s"
          % ", ".join("%g deg %.3e %.3e" % ((phi,) + f) for phi, f in zip(ANGLES, figures)))
    assert max(f[0] for f in figures) <= CAL_MAX * BOUND
    assert max(f[1] for f in figures) <= CAL_RMS * BOUND
    # the constants are this measurement, not a loose guess
    assert max(f[0] for f in figures) >= CAL_MAX / BOUND and max(f[1] for f in figures) >= CAL_RMS / BOUND


def test_the_analytic_check_can_fail():
    det, vg = M.blob_geometry(B)
    vol = M.blob_volume(vg)
    ds, _ = M.offsets_mm(det)
    for name, figures in (("mirrored in x", blob_errors(vol[:, :, ::-1].copy())), ("delta_s with the opposite sign", blob_errors(vol, -ds))):
        print("forward restatement, %s: %s" % (name, ", ".join("%.3e %.3e" % f for f in figures)))
        assert min(f[0] for f in figures) > CAL_MAX * BOUND, name
        assert min(f[1] for f in figures) > CAL_RMS * BOUND, name


def test_centroids_against_the_analytic_phantom():
    """The restatement on the voxelised Shepp-Logan phantom against tests/phantom.py, whose conventions the backprojector's tests
    use: the total agrees within 1 % and the centroid within 0.1 pixel along both detector axes. The voxels are half a pixel wide,
    so a wrong sign or a lost half pixel moves the centroid by at least half a pixel (the offsets by 10 and 4); the prototype of the
    statement measured 0.03 pixel and 0.1 to 0.2 %."""
    det, vg = M.blob_geometry(B)
    radius = 20.0
    x, y, z = M.voxel_centres(vg)
    vol = np.zeros((vg.dim_z, vg.dim_y, vg.dim_x))
    for val, a, b, c, x0, y0, z0, rot in phantom.ELLIPSOIDS:
        r = np.deg2rad(rot)
        px, py, pz = x[None, None, :] - x0 * radius, y[None, :, None] - y0 * radius, z[:, None, None] - z0 * radius
        ox, oy = px * np.cos(r) + py * np.sin(r), -px * np.sin(r) + py * np.cos(r)
        vol += val * ((ox / (a * radius)) ** 2 + (oy / (b * radius)) ** 2 + (pz / (c * radius)) ** 2 <= 1.0)
    ds, dt = M.offsets_mm(det)
    ii, jj = np.meshgrid(np.arange(det.n_row), np.arange(det.n_col))
    for phi in (0.0, 60.0, 135.0, 250.0):
        s, c = M.view_sin_cos(phi)
        got = M.forward_project(vol, 0, det, vg, s, c, ds, dt)
        want = phantom.projection(det.n_row, det.n_col, M.f64(det.l_px_row), M.f64(det.l_px_col), M.f64(det.d_so), M.f64(det.d_od), phi, radius,
                                  M.f64(det.delta_s), M.f64(det.delta_t)).astype(np.float64)
        total = got.sum() / want.sum()
        shift = [(got * k).sum() / got.sum() - (want * k).sum() / want.sum() for k in (ii, jj)]
        print("forward restatement against phantom.py at %g deg: total %.4f, centroid shift %.4f / %.4f pixel" % (phi, total, shift[0], shift[1]))
        assert abs(total - 1.0) <= 0.01 and abs(shift[0]) <= 0.1 and abs(shift[1]) <= 0.1


def test_disjoint_slabs_add_up():
    det, vg = M.geometry(B, 64)
    vol = M.random_volume(64)
    ds, dt = M.offsets_mm(det)
    for phi in (45.0, 200.0):
        s, c = M.view_sin_cos(phi)
        whole = M.forward_project(vol, 0, det, vg, s, c, ds, dt)
        parts = sum(M.forward_project(vol[z0:z1], z0, det, vg, s, c, ds, dt) for z0, z1 in ((0, 21), (21, 30), (30, 64)))
        err = np.abs(parts - whole).max()
        print("forward restatement, three slabs against the whole at %g deg: %.3g absolute on a maximum of %.3g" % (phi, err, whole.max()))
        assert whole.max() > 10 and err <= 1e-12 * whole.max()


@pytest.mark.parametrize("n,angles,rows", [(64, (0.0, 30.0, 45.0, 90.0, 137.0, 315.0), None), (256, (45.0,), None),
                                           (512, (45.0,), list(range(312, 328)))])
def test_fp32_figure(n, angles, rows):
    """FP32_CAL is what this measures: in full at 64 (all six angles) and at 256 (45 degrees, the worst), on 16 middle rows at 512"""
    det, vg = M.geometry(B, n)
    vol = M.random_volume(n)
    ds, dt = M.offsets_mm(det)
    worst = 0.0
    for phi in angles:
        s, c = M.view_sin_cos(phi)
        want = M.forward_project(vol, 0, det, vg, s, c, ds, dt, rows=rows)
        got = M.forward_project(vol, 0, det, vg, s, c, ds, dt, rows=rows, dtype=np.float32)
        assert got.dtype == np.float32
        worst = max(worst, np.abs(got - want).max() / np.abs(want).max())
    print("forward restatement in fp32 against float64 at %d: %.3e of the maximum (FP32_CAL %.3e)" % (n, worst, FP32_CAL[n]))
    assert worst <= FP32_CAL[n] * 1.05
    assert worst >= FP32_CAL[n] * (0.95 if rows is None else 0.25)
