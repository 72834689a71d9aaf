"""The forward projector on the device (forward_project.hip) at the geometries where its branches part, every pixel against the float64
restatement (tests/forward_model.py): anisotropic voxels, the source inside the grid, the detector plane through it, rays that miss,
rays along the axes and exact 45-degree ties, thin slabs under a steep cone, more views than one launch serves, both launch shapes,
and seeded random geometries. The bound of a case is twice the larger of its own fp32-transcription figure (EDGE_CAL in
tests/test_forward_project_host.py, or measured here for the seeded cases) and the smallest entry of FP32_CAL."""
import os

import numpy as np
import pytest

import forward_model as M
import test_forward_project_host as H
import test_gpu_forward_project as G
from paris_amd import backend as B

pytestmark = pytest.mark.gpu

WIDE_MIN_SIN = 0.92        # FP_WIDE_MIN_SIN of forward_project.hip: a launch whose views all have |sin| >= this runs 64 x 4 workgroups
MAX_VIEWS = 64             # FP_MAX_VIEWS: views per launch


@pytest.fixture
def be():
    with B.Backend(0) as b:
        yield b


bits = G.bits


def project(be, d_v, z0, det, vg, sin_cos, pad=0, fill=None, accumulate=False):
    """the views with the given (sin, cos) in ONE call into a stack of frames holding fill: (n, n_col, n_row + pad) float32"""
    ds, dt = M.offsets_mm(det)
    d, first, stride = G.frame_stack(be, len(sin_cos), det, pad, fill)
    be.forward_project(d_v, z0, det, vg, first, [s for s, _ in sin_cos], [c for _, c in sin_cos], ds, dt, accumulate=accumulate,
                       frame_stride=stride)
    out = G.read_stack(be, d, len(sin_cos), det)
    be.free(d)
    return out


def run_case(be, case):
    """Every run of the case (H.edge_runs) on the device, one call per slab with all its views; asserts the case's bound per view and
    returns the device's frames in the order of the runs"""
    H.edge_preconditions(case)
    runs, wants, _ = H.edge_reference(case)
    vol = M.grid_volume(runs[0][2])
    got = [None] * len(runs)
    for slab in sorted({(r[3], r[4]) for r in runs}):
        ks = [k for k, r in enumerate(runs) if (r[3], r[4]) == slab]
        _, det, vg, z0, nz = runs[ks[0]][:5]
        d_v = G.upload_volume(be, vol[z0:z0 + nz])
        out = project(be, d_v, z0, det, vg, [runs[k][5:7] for k in ks])
        be.free(d_v)
        for k, frame in zip(ks, out):
            got[k] = frame
    errs = [H.relative(g, w) for g, w in zip(got, wants)]
    bound = H.edge_bound(H.EDGE_CAL[case])
    print("forward projector, %s, against float64 (max error over max): %.3e to %.3e over %d views, worst at %s; fp32 transcription %.3e, bound %.3e"
          % (case, min(errs), max(errs), len(errs), runs[int(np.argmax(errs))][0], H.EDGE_CAL[case], bound))
    assert max(errs) <= bound
    return got


# ---- 1. the named edge cases -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["aniso", "source_inside", "partial_miss", "axis_aligned"])
def test_edge_case_against_float64(be, case):
    run_case(be, case)


def test_detector_plane_through_the_grid(be):
    """d_od of 4.1 mm, of 0, and of -4.1 mm, which is the same detector: d_sd = |d_so| + |d_od|"""
    got = run_case(be, "detector_inside")
    run_case(be, "detector_at_axis")
    det, vg = M.edge_geometry(B, "detector_inside", d_od=-M.EDGE_CASES["detector_inside"][0][7])
    assert det.d_od < 0
    d_v = G.upload_volume(be, M.grid_volume(vg))
    mirrored = project(be, d_v, 0, det, vg, [M.view_sin_cos(a) for a in M.EDGE_ANGLES])
    be.free(d_v)
    assert np.array_equal(bits(mirrored), bits(np.stack(got)))


def test_rays_that_miss_the_grid(be):
    """no ray meets the grid: +0.0 in every pixel, and with accumulate the frame as it was"""
    H.edge_preconditions("miss")
    det, vg = M.edge_geometry(B, "miss")
    d_v = G.upload_volume(be, M.grid_volume(vg))
    sin_cos = [M.view_sin_cos(a) for a in M.EDGE_ANGLES]
    fill = np.random.default_rng(11).random((len(sin_cos), det.n_col, det.n_row + 8), dtype=np.float32)
    got = project(be, d_v, 0, det, vg, sin_cos, 8, fill)
    assert not bits(got[:, :, :det.n_row]).any() and np.array_equal(bits(got[:, :, det.n_row:]), bits(fill[:, :, det.n_row:]))
    assert np.array_equal(bits(project(be, d_v, 0, det, vg, sin_cos, 8, fill, accumulate=True)), bits(fill))


def test_thin_slabs_under_a_steep_cone(be):
    """slabs of 1, 1, 7, 0 and 27 slices: each alone against the restatement of that slab (run_case), and all of them accumulated
    into one frame against the whole grid's"""
    got = run_case(be, "thin_slabs")
    runs, wants, _ = H.edge_reference("thin_slabs")
    n = len(M.EDGE_ANGLES)
    _, det, vg = runs[0][:3]
    vol = M.grid_volume(vg)
    ranges = M.thin_slab_ranges(vg.dim_z)
    assert [z1 - z0 for z0, z1 in ranges] == [1, 1, 7, 0, vg.dim_z - 9]
    ds, dt = M.offsets_mm(det)
    sin_cos = [r[5:7] for r in runs[:n]]
    d, first, stride = G.frame_stack(be, n, det, 8, np.random.default_rng(13).random((n, det.n_col, det.n_row + 8), dtype=np.float32))
    for j, (z0, z1) in enumerate(ranges):
        d_s = G.upload_volume(be, vol[z0:z1]) if z1 > z0 else B.Volume(None, vg.dim_x, vg.dim_y, 0, on_device=True)
        be.forward_project(d_s, z0, det, vg, first, [s for s, _ in sin_cos], [c for _, c in sin_cos], ds, dt, accumulate=j > 0, frame_stride=stride)
        if z1 > z0:
            be.free(d_s)
    total = G.read_stack(be, d, n, det)[:, :, :det.n_row]
    be.free(d)
    errs = [H.relative(total[k], wants[k]) for k in range(n)]
    bound = H.edge_bound(H.EDGE_CAL["thin_slabs"])
    print("forward projector, thin slabs accumulated against the whole grid's restatement: %s; bound %.3e"
          % (", ".join("%g deg %.3e" % ae for ae in zip(M.EDGE_ANGLES, errs)), bound))
    assert max(errs) <= bound
    assert all(np.abs(g).max() > 1 for g in got)                                                # every slab is seen in every view


# ---- 2. the launch forms ---------------------------------------------------------------------------------------------------------

def singles(be, d_v, det, vg, sin_cos, pad, fill):
    return np.stack([project(be, d_v, 0, det, vg, [sc], pad, fill[k:k + 1])[0] for k, sc in enumerate(sin_cos)])


def is_wide(sin_cos):
    return all(abs(np.float32(s)) >= WIDE_MIN_SIN for s, _ in sin_cos)


def launch_case(be, case, single):
    runs, wants, _ = H.edge_reference(case)
    _, det, vg = runs[0][:3]
    sin_cos = [r[5:7] for r in runs]
    d_v = G.upload_volume(be, M.grid_volume(vg))
    pad = 8
    fill = np.random.default_rng(17).random((len(runs), det.n_col, det.n_row + pad), dtype=np.float32)
    got = project(be, d_v, 0, det, vg, sin_cos, pad, fill)
    assert np.array_equal(bits(got[:, :, det.n_row:]), bits(fill[:, :, det.n_row:]))            # the padding of every frame is untouched
    errs = [H.relative(got[k][:, :det.n_row], wants[k]) for k in range(len(runs))]
    bound = H.edge_bound(H.EDGE_CAL[case])
    print("forward projector, %s in one call, against float64: %.3e to %.3e, worst at %s; fp32 transcription %.3e, bound %.3e"
          % (case, min(errs), max(errs), runs[int(np.argmax(errs))][0], H.EDGE_CAL[case], bound))
    assert max(errs) <= bound
    alone = singles(be, d_v, det, vg, [sin_cos[k] for k in single], pad, fill[list(single)])
    assert np.array_equal(bits(got[list(single)]), bits(alone))
    return sin_cos


def test_131_views_in_one_call(be):
    """two full launches of 64 views and one of 3, each on 16 x 16 workgroups; the views at the launches' edges as single calls"""
    sin_cos = launch_case(be, "views_131", (0, 63, 64, 127, 128, 130))
    assert len(sin_cos) == 2 * MAX_VIEWS + 3 and not any(is_wide(sin_cos[f0:f0 + MAX_VIEWS]) for f0 in range(0, len(sin_cos), MAX_VIEWS))


def test_70_views_near_the_y_axis_in_one_call(be):
    """35 views around 90 and 35 around 270 degrees: both launches (64 and 6 views) on 64 x 4 workgroups; every view as a single call"""
    sin_cos = launch_case(be, "views_wide_70", range(len(M.WIDE_70)))
    assert len(sin_cos) == 70 and is_wide(sin_cos) and min(s for s, _ in sin_cos) < 0 < max(s for s, _ in sin_cos)


def test_the_result_does_not_depend_on_the_launch_shape(be):
    """a view just inside the threshold: alone on 64 x 4 workgroups, behind a 0 degree view on 16 x 16, bit for bit the same"""
    det, vg = M.edge_geometry(B, "launch")
    d_v = G.upload_volume(be, M.grid_volume(vg))
    first = M.view_sin_cos(0.0)
    for a in (67.0, 113.0, 247.0):
        sc = M.view_sin_cos(a)
        assert is_wide([sc]) and abs(sc[0]) < 0.925 and not is_wide([first, sc])
        alone = project(be, d_v, 0, det, vg, [sc])[0]
        assert np.abs(alone).max() > 1 and np.array_equal(bits(alone), bits(project(be, d_v, 0, det, vg, [first, sc])[1])), a


# ---- 3. seeded random geometries -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", range(H.FUZZ_SEEDS))
def test_forward_project_random_geometries(be, seed):
    """Seeded random cases (forward_model.fuzz_case; what the seeds exercise: test_fuzz_seeds_exercise_what_they_are_for), the family
    by seed % 4: source and detector far away, the source inside the grid, the detector plane through it, rays that miss. Three views
    of a slab in one call, written to or added onto random frames with pitch padding."""
    f, wants, figures = H.fuzz_reference(seed)
    det, z0, nz = f.det, f.slab[0], f.slab[1]
    d_v = G.upload_volume(be, f.vol[z0:z0 + nz])
    fill = np.random.default_rng(seed).random((len(f.angles), det.n_col, det.n_row + f.pad), dtype=np.float32)
    got = project(be, d_v, z0, det, f.vg, [M.view_sin_cos(a) for a in f.angles], f.pad, fill, accumulate=f.accumulate)
    assert np.array_equal(bits(got[:, :, det.n_row:]), bits(fill[:, :, det.n_row:]))
    errs = []
    for k, want in enumerate(wants):
        onto = fill[k][:, :det.n_row].astype(np.float64) if f.accumulate else 0.0
        errs.append(np.abs(got[k][:, :det.n_row].astype(np.float64) - (onto + want)).max() / np.abs(want).max())
    bound = H.edge_bound(max(figures))
    print("forward projector, seed %d (%s, %d x %d pixels, grid %d x %d x %d, slices %d to %d%s): %s; fp32 transcription %.3e, bound %.3e"
          % (seed, f.family, det.n_row, det.n_col, f.vg.dim_x, f.vg.dim_y, f.vg.dim_z, z0, z0 + nz, ", accumulate" if f.accumulate else "",
             ", ".join("%.1f deg %.3e" % ae for ae in zip(f.angles, errs)), max(figures), bound))
    assert max(errs) <= bound
