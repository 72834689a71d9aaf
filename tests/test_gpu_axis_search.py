"""The axis search on the device (paris_hip_axis_search_begin / _add_rows / _finish / _discard): the
sinogram against the numpy restatement of the rule (tests/axis_rule.py) bit for bit, the costs to the rounding of a double sum, the
estimate end to end on an analytic sinogram, the sign convention against the project's own forward projector, the lifecycle and the
refusals, and the driver."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import axis_rule as A
import forward_model as M
import phantom
import test_gpu_flat_field as FF
import test_gpu_paris_hip as P
from oracle import formats as F
from paris_amd import _lib
from paris_amd import backend as B

pytestmark = pytest.mark.gpu

INV = _lib.ERROR_INVALID_ARGUMENT


def geometry(n, n_col, delta_t=0.0, delta_s=0.0, n_frames=96):
    return B.DetectorGeometry(n, n_col, A.L_PX, A.L_PX, delta_s, delta_t, A.D_SO, A.D_OD, 360.0 / n_frames)


@pytest.fixture(scope="module")
def be():
    with B.Backend(0) as b:
        yield b


class Frames:
    """frames (N, n_col, n) one under the other in one device buffer whose rows are wider than the frames (pitch > 4 n); shift = 1
    puts every row one float further right, so that the base is misaligned by 4 bytes. .frame(k): frame k as a projection"""

    def __init__(self, be, frames, pad=8, shift=0):
        frames = np.asarray(frames, np.float32)
        self.be, (self.n_frames, self.n_col, self.n) = be, frames.shape
        wide = np.full((self.n_frames * self.n_col, self.n + pad), np.float32(777.0))
        wide[:, shift:shift + self.n] = frames.reshape(-1, self.n)
        self.owner = be.make_projection_device(self.n + pad, self.n_frames * self.n_col)
        be.upload_raw(wide, self.owner)
        self.pitch, self.shift = self.owner.pitch, shift
        self.stride = self.pitch * self.n_col
        assert self.pitch > 4 * self.n

    def frame(self, k):
        return self.be.wrap_projection(self.owner.ptr + 4 * self.shift + k * self.stride, self.pitch, self.n, self.n_col)

    def free(self):
        self.be.free(self.owner)


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.int32), np.ascontiguousarray(b, np.float32).view(np.int32))


def uneven_frames(n_frames, n_col, n, seed):
    """values of very different size, so that the order of the additions shows"""
    rng = np.random.default_rng(seed)
    return (rng.normal(0, 1, (n_frames, n_col, n)) * 10.0 ** rng.integers(-3, 4, (n_frames, n_col, n))).astype(np.float32)


# ---- 1. collect -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [37, 64])
@pytest.mark.parametrize("n_col", [9, 16])
@pytest.mark.parametrize("rows", [1, 2, 5])
def test_the_sinogram_equals_the_rule(be, n, n_col, rows):
    """12 frames added in groups of 8, 3 and 1, out of order, from a frame_stride layout; 64 columns take 16-byte loads, 37 single
    pixels, and so does a base misaligned by 4 bytes"""
    n_frames, delta_t = 12, 0.3 if n_col == 9 else -1.25
    frames = uneven_frames(n_frames, n_col, n, seed=n + n_col + rows)
    det = geometry(n, n_col, delta_t, n_frames=n_frames)
    first = A.row_first(n_col, delta_t, rows)
    want = A.sinogram_of(frames, first, rows)
    if rows > 2:   # the test can tell ascending from descending order (two rows add to the same sum either way)
        assert not same_bits(want, A.sinogram_of(frames[:, ::-1], n_col - first - rows, rows))
    for shift in (0, 1):
        s = Frames(be, frames, shift=shift)
        assert (s.frame(0).ptr % 16 == 0) == (shift == 0) and s.stride % 16 == 0
        be.axis_search_begin(-2.0, 1.0, 5, det, n_frames, rows=rows)
        be.axis_search_add(s.frame(4), 4, frame_stride=s.stride, n_frames=8)
        be.axis_search_add(s.frame(1), 1, frame_stride=s.stride, n_frames=3)
        be.axis_search_add(s.frame(0), 0)
        res, cost, columns, got = be.axis_search_finish(sinogram=True)
        assert res.row_first == first and same_bits(got, want), (n, n_col, rows, shift)
        s.free()


def test_70_frames_in_one_call(be):
    """more frames than one launch serves"""
    n_frames, n, n_col = 70, 16, 4
    assert n_frames > _lib.AXIS_FRAMES_MAX == 64
    frames = uneven_frames(n_frames, n_col, n, seed=70)
    s = Frames(be, frames)
    be.axis_search_begin(-1.0, 0.5, 5, geometry(n, n_col, n_frames=n_frames), n_frames, rows=3)
    be.axis_search_add(s.frame(0), 0, frame_stride=s.stride, n_frames=n_frames)
    res, cost, columns, got = be.axis_search_finish(sinogram=True)
    assert same_bits(got, A.sinogram_of(frames, A.row_first(n_col, 0.0, 3), 3))
    s.free()


def test_a_row_added_twice_and_a_missing_row_are_refused(be):
    n_frames, n, n_col = 12, 37, 9
    frames = uneven_frames(n_frames, n_col, n, seed=3)
    s = Frames(be, frames)
    be.axis_search_begin(-2.0, 1.0, 5, geometry(n, n_col, n_frames=n_frames), n_frames)
    be.axis_search_add(s.frame(0), 0, frame_stride=s.stride, n_frames=5)
    for first, count in ((4, 1), (0, 1), (3, 4), (12, 1), (8, 5), (2 ** 32 - 1, 2)):
        with pytest.raises(B.ParisHipError) as e:
            be.axis_search_add(s.frame(min(first, 11)), first, frame_stride=s.stride, n_frames=count)
        assert e.value.status == INV, (first, count)
    be.axis_search_add(s.frame(6), 6, frame_stride=s.stride, n_frames=6)        # frame 5 is missing: a refused add added nothing
    with pytest.raises(B.ParisHipError) as e:
        be.axis_search_finish()
    assert e.value.status == INV
    be.axis_search_add(s.frame(5), 5)                                           # the search stayed open
    res, cost, columns, got = be.axis_search_finish(sinogram=True)
    assert same_bits(got, A.sinogram_of(frames, A.row_first(n_col, 0.0, 2), 2))
    with pytest.raises(B.ParisHipError):                                        # closed
        be.axis_search_add(s.frame(5), 5)
    s.free()


# ---- 2. score -------------------------------------------------------------------------------------------------------------------------

def score(be, sino, lo, step, count, min_columns=0):
    """the sinogram goes up as N frames of one row each; returns finish()'s values"""
    n_frames, n = sino.shape
    s = Frames(be, sino[:, None, :])
    be.axis_search_begin(lo, step, count, geometry(n, 1, n_frames=n_frames), n_frames, rows=1, min_columns=min_columns)
    be.axis_search_add(s.frame(0), 0, frame_stride=s.stride, n_frames=n_frames)
    out = be.axis_search_finish(sinogram=True)
    s.free()
    assert same_bits(out[3], sino)
    return out


def assert_costs_equal_rule(got, sino, lo, step, count, min_columns=0):
    res, cost, columns, _ = got
    n_frames = sino.shape[0]
    want, want_columns, pairs, skipped = A.costs(sino, lo, step, count, n_frames, A.L_PX, A.D_SO, A.D_OD, min_columns)
    assert np.array_equal(columns, want_columns) and res.skipped == skipped.sum()
    assert np.array_equal(np.isfinite(cost), np.isfinite(want)) and np.all(cost[~np.isfinite(cost)] == np.inf)
    ok = np.isfinite(want)
    err = np.abs(cost[ok] - want[ok]) / want[ok]
    print("axis costs N = %d n = %d: largest relative difference %.3g of the bound M 2^-52 = %.3g" % (n_frames, sino.shape[1], err.max(), (pairs[ok] * 2.0 ** -52).min()))
    assert np.all(err <= pairs[ok] * 2.0 ** -52)       # a double sum of M non-negative terms in any order
    est = A.estimate(lo, step, cost)
    assert (res.best, res.scored, res.at_edge, res.columns) == (est["best"], est["scored"], est["at_edge"], want_columns[est["best"]])
    assert res.delta_s == est["delta_s"] and res.cost_min == est["cost_min"] and res.cost_median == est["cost_median"]
    return want, want_columns, pairs, skipped


SCORE_CASES = [(12, 37, 9, -20.0, 5.0), (96, 96, 33, -48.0, 3.0), (4, 4099, 3, -2049.5, 2049.75)]


@pytest.mark.parametrize("n_frames,n,count,lo,step", SCORE_CASES)
def test_costs_equal_the_rule(be, n_frames, n, count, lo, step):
    """candidates on both sides of zero; the first has no valid column at all, others too few to be scored; 4099 columns: 17 column
    tiles, the last with 3 columns; 96 views: 3 view tiles"""
    sino = np.random.default_rng(n).normal(0, 1, (n_frames, n)).astype(np.float32)
    got = score(be, sino, lo, step, count)
    want, columns, pairs, skipped = assert_costs_equal_rule(got, sino, lo, step, count)
    assert columns[0] == 0 and want[0] == np.inf and np.isfinite(want).sum() >= 1 and not skipped.any()
    if n == 37:
        assert columns[1] == 7 and pairs[1] == 7 * 12 and want[1] == np.inf     # pairs, but fewer than min_columns = 8 columns
        low = score(be, sino, lo, step, count, min_columns=7)
        assert_costs_equal_rule(low, sino, lo, step, count, min_columns=7)
        assert np.isfinite(low[1][1])
    again = score(be, sino, lo, step, count)
    assert np.array_equal(got[1].view(np.int64), again[1].view(np.int64)) and again[0].delta_s == got[0].delta_s    # two runs, the same bits


def test_pairs_that_are_not_finite_are_skipped_as_the_rule_skips_them(be):
    n_frames, n, count, lo, step = 12, 37, 9, -20.0, 5.0
    sino = np.random.default_rng(1).normal(0, 1, (n_frames, n)).astype(np.float32)
    sino[3, 10], sino[7, 30], sino[11, 0] = np.nan, np.inf, -np.inf
    sino[5, 20], sino[6, 20] = 3e38, -3e38                                       # finite samples whose difference overflows
    got = score(be, sino, lo, step, count)
    want, columns, pairs, skipped = assert_costs_equal_rule(got, sino, lo, step, count)
    assert skipped.sum() > 20 and got[0].skipped == skipped.sum() and np.isfinite(want).sum() >= 5


# ---- 3. end to end --------------------------------------------------------------------------------------------------------------------

def test_the_estimate_of_an_analytic_sinogram(be):
    """the 96 x 96 disc sinogram at delta_s = 2.4 as 96 frames of 8 rows, every row a copy of the line; R = 2, candidates -8 .. 8 at
    step 0.5"""
    line = A.disc_sinogram(96, 96, 2.4).astype(np.float32)
    frames = np.repeat(line[:, None, :], 8, axis=1)
    s = Frames(be, frames)
    be.axis_search_begin(-8.0, 0.5, 33, geometry(96, 8), 96, rows=2)
    for k in range(0, 96, 48):
        be.axis_search_add(s.frame(k), k, frame_stride=s.stride, n_frames=48)
    res, cost, columns, sino = be.axis_search_finish(sinogram=True)
    s.free()
    assert same_bits(sino, A.sinogram_of(frames, 3, 2)) and res.row_first == 3
    want, _ = A.recover(sino, -8.0, 0.5, 33)
    print("axis search end to end: estimate %.5f (the rule: %.5f), J_min / J_median %.3g" % (res.delta_s, want["delta_s"], res.cost_min / res.cost_median))
    assert abs(float(res.delta_s) - float(want["delta_s"])) <= 1e-5 and (res.at_edge, res.scored, res.skipped) == (0, 33, 0)
    assert abs(float(res.delta_s) - 2.4) <= A.BOUND_PX


# ---- 4. the convention: the project's own projector -----------------------------------------------------------------------------------

def head_volume(n, l_vx):
    """the Shepp-Logan ellipsoids of tests/phantom.py sampled at the centres of n^3 voxels, radius 0.45 n l_vx"""
    radius = 0.45 * n * l_vx
    x = (np.arange(n) + 0.5 - n / 2.0) * l_vx / radius
    X, Y, Z = x[None, None, :], x[None, :, None], x[:, None, None]
    v = np.zeros((n, n, n))
    for val, a, b, c, x0, y0, z0, rot in phantom.ELLIPSOIDS:
        r = np.deg2rad(rot)
        u, w = (X - x0) * np.cos(r) + (Y - y0) * np.sin(r), -(X - x0) * np.sin(r) + (Y - y0) * np.cos(r)
        v += val * ((u / a) ** 2 + (w / b) ** 2 + ((Z - z0) / c) ** 2 <= 1.0)
    return v.astype(np.float32)


@pytest.mark.parametrize("true", [2.4, -2.4])
def test_the_sign_and_the_geometry_against_the_forward_projector(be, true):
    """a 48^3 head phantom projected by paris_hip_forward_project to 96 views of 96 x 16 pixels with the axis at +-2.4 px: the estimate
    lies within one candidate step of the truth (the voxel model and the cone across the two rows are the projector's, not the rule's)"""
    n_frames = 96
    det = geometry(96, 16, delta_s=true)
    vg = B.VolumeGeometry(48, 48, 48, 1.2, 1.2, 1.2)
    vol = head_volume(48, 1.2)
    d_v = be.make_volume_device(48, 48, 48)
    be.copy_h2d(B.Volume(vol, 48, 48, 48), d_v)
    sc = [M.view_sin_cos(a) for a in M.circle(n_frames)]
    ds, dt = M.offsets_mm(det)
    d = be.make_projection_device(96, 16 * n_frames)
    first = be.wrap_projection(d.ptr, d.pitch, 96, 16)
    stride = d.pitch * 16
    be.forward_project(d_v, 0, det, vg, first, [s for s, _ in sc], [c for _, c in sc], ds, dt, frame_stride=stride)
    be.axis_search_begin(-6.0, 0.5, 25, det, n_frames, rows=2)      # det.delta_s is not read by the search
    be.axis_search_add(first, 0, frame_stride=stride, n_frames=n_frames)
    res, cost, columns = be.axis_search_finish()
    be.free(d)
    be.free(d_v)
    print("axis search on forward projections: true %+.2f, estimate %+.4f, error %.4f px, J_min / J_median %.3g"
          % (true, res.delta_s, abs(res.delta_s - true), res.cost_min / res.cost_median))
    assert res.at_edge == 0 and abs(float(res.delta_s) - true) <= 0.5


# ---- 5. lifecycle, ordering, refusals -------------------------------------------------------------------------------------------------

def test_reserve_bytes_grow_by_the_search_and_shrink_again(be):
    det = geometry(96, 8)
    first, nbytes = B.axis_search_check(-8.0, 0.5, 33, det, 96)
    assert nbytes >= 4 * 96 * 96 + 16 * 33 * 96 + 16 * 33 * 3 + 24 * 33
    before = be.projection_reserve_bytes(96, 8)
    be.axis_search_begin(-8.0, 0.5, 33, det, 96)
    assert be.projection_reserve_bytes(96, 8) == before + nbytes
    be.axis_search_begin(-8.0, 0.5, 33, det, 96)             # replaced: one search's bytes, not both
    assert be.projection_reserve_bytes(96, 8) == before + nbytes
    be.axis_search_discard()
    be.axis_search_discard()                                 # discarding nothing is fine
    assert be.projection_reserve_bytes(96, 8) == before


def test_a_second_begin_and_a_destroy_respect_queued_work():
    n_frames, n, n_col = 8, 2048, 64
    rng = np.random.default_rng(9)
    frames = rng.normal(0, 1, (n_frames, n_col, n)).astype(np.float32)
    det = geometry(n, n_col, n_frames=n_frames)
    with B.Backend(0, synchronous=False) as abe:
        s = Frames(abe, frames)
        abe.axis_search_begin(-1.0, 1.0, 3, det, n_frames, rows=64)
        abe.axis_search_add(s.frame(0), 0, frame_stride=s.stride, n_frames=4)
        abe.axis_search_begin(-1.0, 1.0, 3, det, n_frames, rows=1)     # the adds above may still be queued: they keep the old sinogram
        abe.axis_search_add(s.frame(0), 0, frame_stride=s.stride, n_frames=n_frames)
        res, cost, columns, sino = abe.axis_search_finish(sinogram=True)
        assert same_bits(sino, frames[:, 32, :]) and res.row_first == 32
        abe.axis_search_begin(-1.0, 1.0, 3, det, n_frames)
        abe.axis_search_add(s.frame(0), 0, frame_stride=s.stride, n_frames=n_frames)   # left open: the ctx's destroy frees it


def test_a_held_back_weighting_runs_before_the_rows_are_collected():
    det = B.DetectorGeometry(96, 80, 0.2, 0.25, 1.5, -0.75, 100, 200, 90.0)
    frame = np.random.default_rng(4).normal(2, 1, (80, 96)).astype(np.float32)

    def run(fusion):
        with B.Backend(0, synchronous=False) as abe:
            abe.set_stage_fusion(fusion)
            abe.axis_search_begin(-1.0, 1.0, 3, det, 4, rows=2)
            ds = []
            for k in range(4):
                d_p = B.load(abe, B.Projection(frame.copy(), 96, 80, idx=k))
                B.weight(abe, d_p, det)            # with fusion: held back until something touches the frame
                abe.axis_search_add(d_p, k)
                ds.append(d_p)
            return abe.axis_search_finish(sinogram=True)[3]

    plain, fused = run(False), run(True)
    assert same_bits(plain, fused) and not same_bits(plain, A.sinogram_of(frame[None].repeat(4, 0), A.row_first(80, -0.75, 2), 2))


def test_refusals(be):
    L = _lib.load()
    det = geometry(96, 8)
    d = be.make_projection_device(96, 8)
    other = be.make_projection_device(97, 8)
    cost, res = np.zeros(33), _lib.AxisResult()
    with pytest.raises(B.ParisHipError) as e:                 # without a search
        be.axis_search_add(d, 0)
    assert e.value.status == INV
    with pytest.raises(B.ParisHipError):
        be.axis_search_finish()
    assert L.paris_hip_axis_search_finish(be._ctx, cost.ctypes.data, None, C.byref(res), None) == INV
    s = _lib.AxisSearch(-8.0, 0.5, 33, 2, 0)
    assert L.paris_hip_axis_search_begin(None, C.byref(s), C.byref(det), 96) == INV
    assert L.paris_hip_axis_search_begin(be._ctx, None, C.byref(det), 96) == INV
    assert L.paris_hip_axis_search_begin(be._ctx, C.byref(s), None, 96) == INV
    assert L.paris_hip_axis_search_begin(be._ctx, C.byref(s), C.byref(det), 3) == INV
    assert L.paris_hip_axis_search_begin(be._ctx, C.byref(_lib.AxisSearch(-8.0, 0.0, 33, 2, 0)), C.byref(det), 96) == INV
    assert L.paris_hip_axis_search_begin(be._ctx, C.byref(s), C.byref(geometry(1 << 16, 8)), 1 << 16) == _lib.ERROR_UNSUPPORTED
    with pytest.raises(B.ParisHipError):                      # a refused begin opens nothing
        be.axis_search_add(d, 0)
    be.axis_search_begin(-8.0, 0.5, 33, det, 96)
    try:
        with pytest.raises(B.ParisHipError):
            be.axis_search_add(other, 0)                                                          # other dimensions
        with pytest.raises(B.ParisHipError):
            be.axis_search_add(B.Projection(d.ptr, 96, 7, pitch=d.pitch, on_device=True), 0)
        with pytest.raises(B.ParisHipError):
            be.axis_search_add(B.Projection(d.ptr, 96, 8, pitch=4 * 96 - 4, on_device=True), 0)  # a bad pitch
        with pytest.raises(B.ParisHipError):
            be.axis_search_add(B.Projection(d.ptr, 96, 8, pitch=d.pitch + 2, on_device=True), 0)
        fn = L.paris_hip_axis_search_add_rows
        assert fn(be._ctx, d.ptr, d.pitch, d.pitch * 8 - 4, 2, 96, 8, 0) == INV                  # overlapping frames
        assert fn(be._ctx, d.ptr, d.pitch, d.pitch * 8 + 2, 2, 96, 8, 0) == INV
        assert fn(be._ctx, None, d.pitch, 0, 1, 96, 8, 0) == INV
        assert fn(None, d.ptr, d.pitch, 0, 1, 96, 8, 0) == INV
        assert fn(be._ctx, d.ptr, d.pitch, 0, 1, 96, 8, 96) == INV                               # beyond the circle
        assert fn(be._ctx, d.ptr, d.pitch, 0, 0, 96, 8, 96) == _lib.SUCCESS                      # no frame: nothing to add
        assert L.paris_hip_axis_search_finish(be._ctx, None, None, C.byref(res), None) == INV
        assert L.paris_hip_axis_search_finish(be._ctx, cost.ctypes.data, None, None, None) == INV
        assert L.paris_hip_axis_search_finish(be._ctx, cost.ctypes.data, None, C.byref(res), None) == INV   # every row is missing
    finally:
        be.axis_search_discard()
    be.free(d)
    be.free(other)


def test_a_search_without_a_scored_candidate_is_closed(be):
    sino = np.random.default_rng(2).normal(0, 1, (12, 37)).astype(np.float32)
    s = Frames(be, sino[:, None, :])
    be.axis_search_begin(-40.0, 1.0, 2, geometry(37, 1, n_frames=12), 12, rows=1)
    be.axis_search_add(s.frame(0), 0, frame_stride=s.stride, n_frames=12)
    with pytest.raises(B.ParisHipError) as e:
        be.axis_search_finish()
    assert e.value.status == INV
    with pytest.raises(B.ParisHipError):       # closed
        be.axis_search_add(s.frame(0), 0)
    s.free()


# ---- 6. the driver and the C++ mirror -------------------------------------------------------------------------------------------------

DRV_GEO = (96, 8, A.L_PX, A.L_PX, 0.0, 0.0, A.D_SO, A.D_OD, 3.75)
GEO_KEYS = ("n_row", "n_col", "l_px_row", "l_px_col", "delta_s", "delta_t", "d_so", "d_od", "delta_phi")


def write_geo(path, values):
    path.write_text("\n".join("%s = %s" % kv for kv in zip(GEO_KEYS, values)) + "\n")
    return path


def driver(args):
    return subprocess.run([str(a) for a in args], capture_output=True, text=True, timeout=300)


class Scan:
    pass


@pytest.fixture(scope="module")
def scan_set(tmp_path_factory):
    """a HIS scan written from the analytic sinogram: 96 frames of 96 x 8 float pixels in two files, every row a copy of the line; the
    estimate of the Python path; the driver's arguments and the line it reports"""
    tmp_path = tmp_path_factory.mktemp("axis")
    line = A.disc_sinogram(96, 96, 2.4).astype(np.float32)
    frames = np.repeat(line[:, None, :], 8, axis=1)
    scan = tmp_path / "scan"
    scan.mkdir()
    (scan / "a.his").write_bytes(F.his_file_bytes(frames[:60], 128, 32))
    (scan / "b.his").write_bytes(F.his_file_bytes(frames[60:], 128, 32))
    geo = write_geo(tmp_path / "geo.ini", DRV_GEO)
    with B.Backend(0) as pbe:
        s = Frames(pbe, frames)
        pbe.axis_search_begin(-6.0, 0.5, 25, B.DetectorGeometry(*DRV_GEO), 96, rows=2)
        pbe.axis_search_add(s.frame(0), 0, frame_stride=s.stride, n_frames=96)
        want, cost, columns = pbe.axis_search_finish()
    assert abs(float(want.delta_s) - 2.4) <= A.BOUND_PX
    report = "axis search on: delta_s = %.4f px (the geometry file gave 0.0000), candidate %d of 25" % (want.delta_s, want.best)
    base = [P.EXE, "--geometry", geo, "--input", scan, "--output", tmp_path / "none", "--find-axis", "-6:6:0.5"]
    out = Scan()
    out.frames, out.scan, out.want, out.report, out.base, out.tmp_path = frames, scan, want, report, base, tmp_path
    return out


def test_the_driver_finds_the_axis_the_python_path_finds(scan_set):
    base, report, tmp_path = scan_set.base, scan_set.report, scan_set.tmp_path
    # the band alone; whole frames that feed the profile too; the band widened by a row (no pixel is a zinger); groups of 7 frames
    for extra in ([], ["--rings", "2:0.3"], ["--zingers", "1000"], ["--batch", "7", "--axis-rows", "2"]):
        r = driver(base + ["--axis-only"] + extra)
        assert r.returncode == 0, r.stdout + r.stderr
        assert report in r.stdout and "25 candidate(s) scored, 0 pair(s) skipped, 96 frame(s) of 2 row(s) from row 3" in r.stdout, r.stdout
        assert ("ring filter on: 96 frame(s)" in r.stdout) == (extra[:1] == ["--rings"]) and "warning" not in r.stdout and "volume" not in r.stdout
    assert not (tmp_path / "none").exists()
    r = driver(base + ["--axis-only", "--axis-rows", "1"])     # another band: row 4 alone, the same lines
    assert r.returncode == 0 and "96 frame(s) of 1 row(s) from row 4" in r.stdout and report in r.stdout, r.stdout
    r = driver(base[:7] + ["--find-axis", "-6:1:0.5", "--axis-only"])   # the minimum beyond the last candidate
    assert r.returncode == 0 and "delta_s = 1.0000 px" in r.stdout and "warning: the axis search's minimum" in r.stdout, r.stdout


def test_the_driver_reconstructs_with_the_found_axis(scan_set):
    """the volume is that of the found geometry"""
    base, report, tmp_path, want, scan = scan_set.base, scan_set.report, scan_set.tmp_path, scan_set.want, scan_set.scan
    found = write_geo(tmp_path / "found.ini", DRV_GEO[:4] + ("%.9g" % want.delta_s,) + DRV_GEO[5:])
    r = driver(base[:5] + ["--output", tmp_path / "a", "--find-axis", "-6:6:0.5", "--slabs", "1"])
    assert r.returncode == 0 and report in r.stdout and "volume" in r.stdout, r.stdout + r.stderr
    r = driver([P.EXE, "--geometry", found, "--input", scan, "--output", tmp_path / "b", "--slabs", "1"])
    assert r.returncode == 0 and "axis search" not in r.stdout, r.stdout + r.stderr
    va, vb = F.ddbvf_read(str(tmp_path / "a" / "vol.ddbvf"))[1], F.ddbvf_read(str(tmp_path / "b" / "vol.ddbvf"))[1]
    assert va.shape == vb.shape and np.abs(va).max() > 0 and np.array_equal(va.view(np.uint32), vb.view(np.uint32))


def test_the_driver_and_the_cpp_mirror_refuse_and_agree(scan_set):
    base, tmp_path, want, frames = scan_set.base, scan_set.tmp_path, scan_set.want, scan_set.frames
    # refused before any device work
    angles = tmp_path / "angles.txt"
    angles.write_text("\n".join("%g" % (3.75 * k) for k in range(96)) + "\n")
    short = write_geo(tmp_path / "short.ini", DRV_GEO[:8] + (3.0,))             # 96 x 3 = 288 degrees
    back = write_geo(tmp_path / "back.ini", DRV_GEO[:8] + (-3.75,))
    for args, word in ((base + ["--short-scan"], "--short-scan"), (base + ["--angles", angles], "--angles"),
                       ([P.EXE, "--geometry", short] + base[3:], "full circle"), ([P.EXE, "--geometry", back] + base[3:], "full circle"),
                       (base + ["--quality", "2", "--axis-rows", "9"], "--axis-rows"), (base[:7] + ["--axis-only"], "--find-axis"),
                       (base[:7] + ["--find-axis", "6:-6"], "--find-axis"), (base[:7] + ["--find-axis", "-6"], "--find-axis"),
                       (base[:7] + ["--find-axis", "-600:600:0.5"], "1024"), (base[:7] + ["--find-axis", "-6:6:x"], "--find-axis")):
        r = driver(args)
        assert r.returncode == 1 and "--find-axis" in r.stderr and word in r.stderr, (args[7:], r.stderr)
    assert not (tmp_path / "none").exists()
    # PARIS's loop through paris::hip with the pre-pass (paris_hip_demo --find-axis [--rings])
    raw = tmp_path / "in.raw"
    frames.tofile(raw)
    for extra in ([], ["--rings", "2", "0.3", "0"]):
        r = driver([FF.DEMO] + list(DRV_GEO) + [96, raw, tmp_path / "demo.raw", "--no-out", "--find-axis", "-6", "0.5", "25", "2"] + extra)
        assert r.returncode == 0, r.stderr + r.stdout
        got = [l for l in r.stdout.splitlines() if l.startswith("axis: delta_s = ")]
        assert len(got) == 1 and np.float32(got[0].split()[3]) == np.float32(want.delta_s), r.stdout
