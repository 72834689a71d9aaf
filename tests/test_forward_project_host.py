"""The forward projector's statement on the host (no GPU needed): the float64 restatement of tests/forward_model.py against
analytic line integrals of Gaussian blobs and against the analytic projections of tests/phantom.py, the additivity of disjoint slabs,
and what fp32 arithmetic costs the same statement (FP32_CAL, the figure the GPU tests bound the device with)."""
import os

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


# ---- the edge cases of tests/test_gpu_forward_project_edges.py -------------------------------------------------------------------

# max |fp32 transcription - float64 restatement| over max |restatement|, the largest over the case's views (edge_runs), on the
# uniform random volume of forward_model.grid_volume: what test_edge_fp32_figure measures. The device's bound for a case is
# edge_bound: twice the larger of this figure and the smallest entry of FP32_CAL.
EDGE_CAL = {"aniso": 2.676e-5, "source_inside": 9.806e-7, "detector_inside": 4.216e-6, "detector_at_axis": 2.776e-6, "partial_miss": 2.472e-5,
            "axis_aligned": 2.230e-5, "thin_slabs": 6.563e-6, "views_131": 2.778e-5, "views_wide_70": 1.297e-5}


def edge_bound(figure):
    return 2 * max(figure, min(FP32_CAL.values()))


def edge_runs(case):
    """what a case compares with the restatement: [(label, det, vg, v_offset, v_dim_z, sin, cos)]"""
    if case == "detector_at_axis":
        det, vg = M.edge_geometry(B, "detector_inside", d_od=0.0)
    elif case in ("views_131", "views_wide_70"):
        det, vg = M.edge_geometry(B, "launch")
    else:
        det, vg = M.edge_geometry(B, case)
    if case == "axis_aligned":
        return [("sin %g cos %g" % sc, det, vg, 0, vg.dim_z) + sc for sc in M.AXIS_SIN_COS]
    angles = {"views_131": M.circle(131), "views_wide_70": M.WIDE_70}.get(case, M.EDGE_ANGLES)
    slabs = [(0, vg.dim_z)]
    if case == "thin_slabs":
        slabs += [(z0, z1) for z0, z1 in M.thin_slab_ranges(vg.dim_z) if z1 > z0]
    return [("%g deg, slices %d to %d" % (a, z0, z1), det, vg, z0, z1 - z0) + M.view_sin_cos(a) for z0, z1 in slabs for a in angles]


_EDGE_REFERENCE = {}


def edge_reference(case):
    """(runs, the float64 restatement of every run, the fp32 transcription's distance from it per run); computed once, read-only"""
    if case not in _EDGE_REFERENCE:
        runs, wants, figures = edge_runs(case), [], []
        vol = M.grid_volume(runs[0][2])
        for _, det, vg, z0, nz, s, c in runs:
            ds, dt = M.offsets_mm(det)
            want = M.forward_project(vol[z0:z0 + nz], z0, det, vg, s, c, ds, dt)
            got = M.forward_project(vol[z0:z0 + nz], z0, det, vg, s, c, ds, dt, dtype=np.float32)
            want.setflags(write=False)
            wants.append(want)
            figures.append(np.abs(got - want).max() / np.abs(want).max())
        _EDGE_REFERENCE[case] = (runs, wants, figures)
    return _EDGE_REFERENCE[case]


def restate(vol, det, vg, z0, nz, s, c, **kw):
    ds, dt = M.offsets_mm(det)
    return M.forward_project(vol[z0:z0 + nz], z0, det, vg, s, c, ds, dt, **kw)


def relative(got, want):
    return np.abs(got.astype(np.float64) - want).max() / np.abs(want).max()


@pytest.mark.parametrize("case", sorted(EDGE_CAL))
def test_edge_fp32_figure(case):
    """EDGE_CAL is what this measures"""
    _, _, figures = edge_reference(case)
    print("forward restatement in fp32 against float64, %s: %.3e to %.3e of the maximum over %d views (EDGE_CAL %.3e)"
          % (case, min(figures), max(figures), len(figures), EDGE_CAL[case]))
    assert EDGE_CAL[case] * 0.95 <= max(figures) <= EDGE_CAL[case] * 1.05


def edge_preconditions(case):
    """What a case is there for, asserted of its inputs with the float64 statement alone (the device tests call this too)"""
    runs, wants, _ = edge_reference(case) if case != "miss" else (edge_runs(case), None, None)
    _, det, vg = runs[0][:3]
    ds, dt = M.offsets_mm(det)
    setups = [M.ray_setup(det, vg, s, c, ds, dt) for _, _, _, _, _, s, c in runs]
    h = [0.5 * n * M.f64(l) for n, l in ((vg.dim_x, vg.l_vx_x), (vg.dim_y, vg.l_vx_y), (vg.dim_z, vg.l_vx_z))]
    assert len({vg.dim_x, vg.dim_y, vg.dim_z}) == 3 and len({vg.l_vx_x, vg.l_vx_y, vg.l_vx_z}) == 3
    for (label, _, _, _, _, s, c), su in zip(runs, setups):
        cut, margin = M.clipped(su.a)
        if case in ("source_inside", "detector_inside", "detector_at_axis"):
            # the clip removes planes in every view, and no a is so close to 0 or 1 that two float64 evaluations could disagree
            assert cut.any() and margin > 1e-9, (label, margin)
            src = (-M.f64(det.d_so) * M.f64(c), -M.f64(det.d_so) * M.f64(s))
            assert (case == "source_inside") == (abs(src[0]) < h[0] and abs(src[1]) < h[1]), label
            if case == "source_inside":
                assert (su.a <= 0).any() and not (su.a > 1).any(), label             # planes behind the source, none behind the detector
            else:
                assert (su.a > 1).any() and not (su.a <= 0).any(), label
        else:
            assert not cut.any(), label
    if case == "miss":
        vol = M.grid_volume(vg)
        for label, _, _, z0, nz, s, c in runs:
            assert not restate(vol, det, vg, z0, nz, s, c).any(), label              # no ray meets the grid
    if case == "partial_miss":
        for label, want in zip((r[0] for r in runs), wants):
            assert 0.1 <= (want == 0).mean() <= 0.9, label
    if case == "thin_slabs":
        # the outermost rows leave the grid in z between its first and last plane: they cross every slab through its faces
        for su in setups:
            w = np.nanmax(su.a, axis=0).min() * np.abs(su.z).max(), np.nanmin(su.a, axis=0).max() * np.abs(su.z).max()
            assert w[0] > h[2] + M.f64(vg.l_vx_z) and np.abs(su.z).max() / (2 * M.f64(det.d_so)) > 0.25
    if case == "axis_aligned":
        i0, j0 = det.n_row // 2, det.n_col // 2
        vol = M.grid_volume(vg)
        for k, ((label, _, _, z0, nz, s, c), su) in enumerate(zip(runs, setups)):
            assert su.t[i0] == 0.0 and su.z[j0] == 0.0, label
            assert (su.dx[i0] == 0.0 or su.dy[i0] == 0.0) == (k < 4) and (abs(su.dx[i0]) == abs(su.dy[i0])) == (k >= 4), label
            if k >= 4:
                # the tie: the statement marches the column along x, and marching it along y gives another column by far more than the bound
                assert su.x_march[i0] and np.count_nonzero(np.abs(su.dx) == np.abs(su.dy)) == 1, label
                other = restate(vol, det, vg, z0, nz, s, c, perturb="tie_gt")
                moved = np.abs(other - wants[k])
                assert not np.delete(moved, i0, axis=1).any(), label
                assert moved[:, i0].max() / np.abs(wants[k]).max() > 100 * edge_bound(EDGE_CAL[case]), label


@pytest.mark.parametrize("case", sorted(EDGE_CAL) + ["miss"])
def test_edge_case_preconditions(case):
    edge_preconditions(case)


@pytest.mark.parametrize("case,perturb", [("aniso", "swap_l_p_l_u"), ("views_wide_70", "swap_l_p_l_u"), ("source_inside", "no_clip"),
                                          ("detector_inside", "no_clip"), ("detector_at_axis", "no_clip"), ("axis_aligned", "tie_gt")])
def test_the_edge_checks_can_fail(case, perturb):
    """The fp32 transcription with one slip the kernel could make -- the voxel sizes of the marching axis and the other axis exchanged,
    the clip to 0 < a <= 1 dropped, > for >= at the tie -- is past the case's bound in EVERY view that has the feature (all of them;
    for the tie, the four diagonal views), by a factor of more than 100"""
    runs, wants, figures = edge_reference(case)
    vol = M.grid_volume(runs[0][2])
    bound = edge_bound(EDGE_CAL[case])
    hit = range(4, 8) if perturb == "tie_gt" else range(len(runs))
    errs = [relative(restate(vol, det, vg, z0, nz, s, c, dtype=np.float32, perturb=perturb), wants[k])
            for k, (_, det, vg, z0, nz, s, c) in enumerate(runs) if k in hit]
    print("forward restatement in fp32 with %s, %s: %.3e to %.3e of the maximum, bound %.3e" % (perturb, case, min(errs), max(errs), bound))
    assert max(figures) <= bound and min(errs) > 100 * bound


# ---- the seeded random geometries ------------------------------------------------------------------------------------------------

FUZZ_SEEDS = int(os.environ.get("PARIS_FP_FUZZ_SEEDS", "24"))
_FUZZ_REFERENCE = {}


def fuzz_reference(seed):
    """(the case, the float64 restatement of its slab per angle, the fp32 transcription's distance per angle); computed once, read-only"""
    if seed not in _FUZZ_REFERENCE:
        f = M.fuzz_case(B, seed)
        wants, figures = [], []
        for a in f.angles:
            s, c = M.view_sin_cos(a)
            want = restate(f.vol, f.det, f.vg, f.slab[0], f.slab[1], s, c)
            figures.append(relative(restate(f.vol, f.det, f.vg, f.slab[0], f.slab[1], s, c, dtype=np.float32), want))
            want.setflags(write=False)
            wants.append(want)
        f.vol.setflags(write=False)
        _FUZZ_REFERENCE[seed] = (f, wants, figures)
    return _FUZZ_REFERENCE[seed]


def test_fuzz_seeds_exercise_what_they_are_for():
    """A condition on the generator's inputs, from the float64 statement alone: every family is there and has its feature in every
    view, no view is all zero, and at least half of the views march some columns along x and others along y."""
    families = {name: 0 for name in M.FUZZ_FAMILIES}
    views = mixed = 0
    for seed in range(FUZZ_SEEDS):
        f, wants, _ = fuzz_reference(seed)
        assert f.family == M.FUZZ_FAMILIES[seed % 4]
        families[f.family] += 1
        det, vg = f.det, f.vg
        assert 17 <= det.n_row <= 64 and 9 <= det.n_col <= 64 and all(9 <= d <= 64 for d in (vg.dim_x, vg.dim_y, vg.dim_z))
        assert len({vg.dim_x, vg.dim_y, vg.dim_z}) == 3 and len({vg.l_vx_x, vg.l_vx_y, vg.l_vx_z}) == 3
        assert f.slab[1] >= 1 and f.slab[0] + f.slab[1] <= vg.dim_z and f.pad >= 1 and len(f.angles) == 3
        ds, dt = M.offsets_mm(det)
        h = [0.5 * n * M.f64(l) for n, l in ((vg.dim_x, vg.l_vx_x), (vg.dim_y, vg.l_vx_y))]
        for a, want in zip(f.angles, wants):
            s, c = M.view_sin_cos(a)
            su = M.ray_setup(det, vg, s, c, ds, dt)
            cut, margin = M.clipped(su.a)
            inside = abs(M.f64(det.d_so) * c) < h[0] and abs(M.f64(det.d_so) * s) < h[1]
            assert margin > 1e-9 and want.any(), (seed, a)
            assert inside == (f.family == "source_inside"), (seed, a)
            if f.family == "source_inside":
                assert (su.a <= 0).any(), (seed, a)
            elif f.family == "detector_inside":
                assert (su.a > 1).any(), (seed, a)
            if f.family == "miss":
                assert (want == 0).mean() >= 0.1, (seed, a)
            views += 1
            mixed += bool(su.x_march.any() and not su.x_march.all())
    print("forward fuzz: %d seeds %s, %d of %d views march along both axes" % (FUZZ_SEEDS, families, mixed, views))
    if FUZZ_SEEDS >= 24:
        assert min(families.values()) >= 5
    assert 2 * mixed >= views
