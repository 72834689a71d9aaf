"""Offset detectors on the device: the redundancy weight (paris_hip_offset_detector_weight_rows, short_scan.hip) against a float64
restatement of its formula, its conjugate columns, its launch forms and refusals, the backprojectors at detector offsets that cover
one side only, the quality of half-fan reconstructions against the bounds calibrated on the CPU, the product paths against each
other and the oracle, and the C++ mirror and driver."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import test_gpu_paris_hip as P
import test_gpu_whole_circle as W
import test_offset_detector_host as H
from oracle import formats as F
from paris_amd import _lib
from paris_amd import backend as B

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEMO = os.path.join(ROOT, "paris_amd", "host", "demo", "paris_hip_demo")
CONJ_TOL = 2.4e-7   # |2 w(t) + 2 w(-t) - 2|: two float roundings of values below 2
GEO_KEYS = H.GEO_KEYS


@pytest.fixture
def be():
    with B.Backend(0) as b:
        yield b


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def frames_device(be, frames, dim_x=None):
    """(n, dim_y, w) float32 -> one device buffer of n frames one under the other, w columns each; a Projection of the first frame
    with dim_x columns (default w: the columns beyond dim_x play pitch padding) and the frame stride in bytes"""
    n, dim_y, w = frames.shape
    d = be.make_projection_device(w, n * dim_y)
    be.copy_h2d(B.Projection(np.ascontiguousarray(frames.reshape(n * dim_y, w)), w, n * dim_y), d)
    return d, B.Projection(d.ptr, dim_x or w, dim_y, pitch=d.pitch, on_device=True), d.pitch * dim_y


def frames_host(be, d, n, dim_y):
    h = be.make_projection_host(d.dim_x, d.dim_y)
    be.copy_d2h(d, h)
    return h.buf.reshape(n, dim_y, d.dim_x).copy()


def device_weights(be, det, rows=2):
    d, first, _ = frames_device(be, np.ones((1, rows, det.n_row), np.float32))
    be.offset_detector_weight(first, det)
    w2 = frames_host(be, d, 1, rows)[0]
    be.free(d)
    assert (w2 == w2[:1]).all()                                     # one weight per column, every row
    return w2[0]


def lcg_frames(oracle, n, dim_y, dim_x, seed=0):
    return np.stack([oracle.lcg_projection(dim_x, dim_y, seed + k) for k in range(n)])


# ---- 1. the formula and 2. the conjugates --------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_row,delta_s", [(128, -40.0), (128, 40.0), (128, -40.5), (128, 20.25), (2048, -700.0)])
def test_formula_against_float64(be, n_row, delta_s):
    l = 0.8 if n_row == 128 else 0.2
    det = B.DetectorGeometry(n_row, 16, l, l, delta_s, 0.0, 500, 500, 1.0)
    want = H.twice_weight(det)
    got = device_weights(be, det)
    err = np.abs(got.astype(np.float64) - want)
    print("offset detector n_row %d delta_s %g: max |2w - 2w_float64| = %.3g" % (n_row, delta_s, err.max()))
    assert (err <= np.spacing(want.astype(np.float32)).astype(np.float64)).all()   # within one float rounding
    tau, _, _ = H.overlap(det)
    t = (np.arange(n_row) + 0.5) * H.f64(l) - (n_row * H.f64(l) / 2 + H.f64(delta_s) * H.f64(l))
    long_side = t >= tau if delta_s <= 0 else t <= -tau
    assert long_side.sum() >= 2 * abs(delta_s) - 1 and (got[long_side] == np.float32(2.0)).all()
    assert (got[want == 0] == 0).all() and ((got > 0) & (got < 2)).sum() >= 2 * (n_row / 2 - abs(delta_s)) - 2


@pytest.mark.parametrize("delta_s", [-40.5, 40.5, -20.5])
def test_conjugate_columns_add_up_to_two(be, delta_s):
    """half-integer delta_s: columns i and n - 1 + 2 delta_s - i lie at t and -t"""
    det = B.DetectorGeometry(128, 16, 0.8, 0.8, delta_s, 0.0, 500, 500, 1.0)
    w2 = device_weights(be, det).astype(np.float64)
    i = np.arange(128)
    j = (127 + 2 * delta_s - i).astype(int)
    ok = (j >= 0) & (j < 128)
    err = np.abs(w2[i[ok]] + w2[j[ok]] - 2.0)
    print("offset detector delta_s %g: max |2w(t) + 2w(-t) - 2| = %.3g over %d pairs" % (delta_s, err.max(), ok.sum()))
    assert ok.sum() >= 40 and err.max() <= CONJ_TOL


# ---- 3. the launch forms -------------------------------------------------------------------------------------------------------

def test_row_band_batch_and_stage_forms(be, oracle):
    det = B.DetectorGeometry(128, 96, 0.8, 0.8, -40.0, 0.0, 500, 500, 1.0)
    w2 = device_weights(be, det)
    raw = lcg_frames(oracle, 5, 96, 160, 3)                         # 32 columns beyond the detector's 128: the pitch padding
    want = raw.copy()
    want[:, :, :128] = raw[:, :, :128] * w2[None, None, :]
    d, first, stride = frames_device(be, raw, 128)
    be.offset_detector_weight(first, det, frame_stride=stride, n_frames=5)
    assert np.array_equal(bits(frames_host(be, d, 5, 96)), bits(want))
    be.free(d)
    d, first, stride = frames_device(be, raw, 128)
    be.offset_detector_weight(first, det, row_first=37, row_count=50, frame_stride=stride, n_frames=5)
    band = frames_host(be, d, 5, 96)
    assert np.array_equal(bits(band[:, 37:87]), bits(want[:, 37:87]))
    assert np.array_equal(bits(band[:, :37]), bits(raw[:, :37])) and np.array_equal(bits(band[:, 87:]), bits(raw[:, 87:]))
    be.free(d)
    d = B.load(be, B.Projection(np.ascontiguousarray(raw[2, :, :128]), 128, 96, idx=7))
    B.stage_offset_detector_weight(be, d, det)
    h = be.make_projection_host(128, 96)
    be.copy_d2h(d, h)
    assert np.array_equal(bits(h.buf), bits(want[2, :, :128]))
    be.free(d)


def test_argument_refusals(be, oracle):
    det = B.DetectorGeometry(64, 32, 0.8, 0.8, -16.0, 0.0, 500, 500, 1.0)
    L, ctx = be._L, be._ctx
    d = be.make_projection_device(64, 64)

    def call(pitch=d.pitch, stride=d.pitch * 32, n=1, dim_x=64, dim_y=32, r0=0, rc=32, det_=det, ptr=d.ptr):
        return L.paris_hip_offset_detector_weight_rows(ctx, ptr, pitch, stride, n, dim_x, dim_y, r0, rc,
                                                       C.byref(det_) if det_ is not None else None)
    assert call() == 0 and call(n=2) == 0
    inv = _lib.ERROR_INVALID_ARGUMENT
    assert call(ptr=None) == inv and call(det_=None) == inv
    assert call(pitch=64 * 4 - 4) == inv and call(pitch=d.pitch + 2) == inv    # short pitch, not whole floats
    assert call(r0=33) == inv and call(r0=8, rc=25) == inv                     # band out of range
    assert call(dim_x=32) == inv                                               # columns are the detector's n_row
    assert call(n=2, stride=d.pitch * 31) == inv                               # overlapping frames
    assert call(det_=B.DetectorGeometry(64, 32, 0.8, 0.8, -30.5, 0.0, 500, 500, 1.0)) == inv   # tau = 1.5 pixels
    assert call(det_=B.DetectorGeometry(64, 32, 0.8, 0.8, -30.0, 0.0, 500, 500, 1.0)) == 0     # tau = 2 pixels
    assert L.paris_hip_stage_offset_detector_weight(ctx, d.ptr, d.pitch, 64, 32, None) == inv
    assert L.paris_hip_stage_offset_detector_weight(ctx, None, d.pitch, 64, 32, C.byref(det)) == inv
    assert call(rc=0) == 0 and call(n=0) == 0                                  # nothing to do
    be.free(d)
    raw = lcg_frames(oracle, 1, 32, 64)                                        # still usable
    d, first, _ = frames_device(be, raw)
    be.offset_detector_weight(first, det)
    assert np.array_equal(bits(frames_host(be, d, 1, 32)), bits(raw * device_weights(be, det)[None, None, :]))
    be.free(d)


# ---- 5. the backprojectors at offsets that cover one side only -----------------------------------------------------------------

def backproject_three_ways(oracle, g, vg_dims, idxs, slabs):
    """the oracle, the one-projection tile kernel (deferral 1) and the fused batch kernel (deferral 8) on raw lcg frames, into slabs
    (v_offset, dim_z) of the volume grid vg_dims = (dim, l_vx); each pair of results compared bit for bit"""
    det, odet = B.DetectorGeometry(*g), oracle.DetectorGeometry(*g)
    dim, l_vx = vg_dims
    vg, ovg = B.VolumeGeometry(dim, dim, dim, l_vx, l_vx, l_vx), oracle.VolumeGeometry(dim, dim, dim, l_vx, l_vx, l_vx)
    frames = {i: oracle.lcg_projection(det.n_row, det.n_col, i) for i in idxs}
    problems = []
    for z0, dz in slabs:
        want = np.zeros((dz, dim, dim), np.float32)
        for i in idxs:
            s, c, ods, odt = oracle.backproject_constants(odet, i)
            oracle.backproject(want, frames[i], z0, odet, ovg, s, c, ods, odt)
        assert np.count_nonzero(want) > dim * dim // 4
        for depth in (1, 8):
            with B.Backend(0) as be:
                be.set_backproject_deferral(depth)
                v = be.make_volume_device(dim, dim, dz)
                for i in idxs:
                    d_p = B.load(be, B.Projection(frames[i].copy(), det.n_row, det.n_col, idx=i))
                    B.backproject(be, d_p, v, z0, det, vg, False, False, None)
                    be.free(d_p)
                be.flush()
                h = be.make_volume_host(dim, dim, dz)
                be.copy_d2h(v, h)
                got = h.buf.reshape(dz, dim, dim)
            if not np.array_equal(got.view(np.int32), want.view(np.int32)):
                bad = np.argwhere(got.view(np.int32) != want.view(np.int32))
                problems.append("delta_s %g, slab at %d, deferral %d: %d voxels differ, first at %s (%r against %r)"
                                % (g[4], z0, depth, len(bad), tuple(bad[0]), float(got[tuple(bad[0])]), float(want[tuple(bad[0])])))
    return problems


@pytest.mark.parametrize("delta_s", [-40.0, 40.0])
def test_backprojectors_at_a_half_fan_offset_against_the_oracle(oracle, delta_s):
    g = (128, 96, 0.8, 0.8, delta_s, 0.0, 500, 500, 15.0)                     # 24 angles 15 degrees apart: the whole circle
    vg = B.calculate_volume_geometry(B.DetectorGeometry(*g))                  # the extended volume, about 207 voxels wide
    assert vg.dim_x >= 200
    problems = backproject_three_ways(oracle, g, (vg.dim_x, vg.l_vx_x), list(range(24)), [(0, vg.dim_z)])
    assert not problems, "\n".join(problems)


def test_backprojectors_at_1024_with_delta_s_minus_320(oracle):
    g = (1024, 1024, 0.2, 0.2, -320.0, 0.0, 500, 500, 45.0)                   # 8 angles over the circle
    nat = B.calculate_volume_geometry(B.DetectorGeometry(*g))
    grid = 1024
    l_vx = float(np.float32(nat.l_vx_x) * np.float32(nat.dim_x) / np.float32(grid))   # the extended field of view on a 1024 grid
    # the coarser voxels make the grid taller than the cone (slices 0 and 1023 lie outside it): three depths inside it
    problems = backproject_three_ways(oracle, g, (grid, l_vx), list(range(8)), [(200, 2), (511, 2), (822, 2)])
    assert not problems, "\n".join(problems)


# ---- 6. quality against the calibrated bounds ----------------------------------------------------------------------------------

def reconstruct(n_row, delta_s, weighted):
    """the calibration scan through the Backend product path (set_paris_loop_defaults), PARIS's loop, on the half fan's grid"""
    det = B.DetectorGeometry(*H.cal_geometry(n_row, delta_s))
    vg = H.cal_volume_geometry(B)
    with B.Backend(0, synchronous=False) as abe:
        abe.set_paris_loop_defaults(48)
        v = abe.make_volume_device(vg.dim_x, vg.dim_y, vg.dim_z)
        for i in range(360):
            d_p = abe.make_projection_device(det.n_row, det.n_col)
            W.upload(abe, d_p, H.cal_frame(n_row, delta_s, i, H.cal_radius(vg)))
            d_p.idx = i
            if weighted:
                B.stage_offset_detector_weight(abe, d_p, det)
            B.weight(abe, d_p, det)
            B.filter(abe, d_p, det)
            B.backproject(abe, d_p, v, 0, det, vg, False, False, None)
            abe.free(d_p)
        abe.flush()
        h = abe.make_volume_host(vg.dim_x, vg.dim_y, vg.dim_z)
        abe.copy_d2h(v, h)
        abe.free(v)
    z0, z1 = H.central_slices(vg.dim_z)
    return h.buf.reshape(vg.dim_z, vg.dim_y, vg.dim_x)[z0:z1].copy()


def test_quality_against_the_calibrated_bounds(oracle):
    vg = H.cal_volume_geometry(B)
    det = B.DetectorGeometry(*H.cal_geometry(128, -40.0))
    ref = reconstruct(208, 0.0, False)
    figures = {}
    vols = {}
    for name, ds, weighted in (("-40", -40.0, True), ("+40", 40.0, True), ("unweighted", -40.0, False)):
        vols[name] = reconstruct(128, ds, weighted)
        figures[name] = (H.rel_rms(vols[name], ref, 1.0),) + H.structure(vols[name], ref, det, vg)
    print("offset detector quality on the device (relative RMS, inside max, outside mean): %s"
          % ", ".join("%s %.4f %.2e %.4f" % ((k,) + v) for k, v in figures.items()))
    for name in ("-40", "+40"):
        rms, inside, outside = figures[name]
        assert rms <= H.CAL_RMS * H.BOUND
        assert inside <= H.CAL_INSIDE * H.BOUND
        assert 0 < outside <= H.CAL_OUTSIDE * H.BOUND
    rms, inside, _ = figures["unweighted"]
    assert rms > H.CAL_RMS * H.BOUND and rms >= 2.5 * H.CAL_RMS
    assert inside > H.CAL_INSIDE * H.BOUND
    # the oracle on the same weighted frames: the filter's FFT rounding apart, the same volume
    want = H.oracle_reconstruct(oracle, 128, -40.0, True)
    err = np.abs(vols["-40"].astype(np.float64) - want).max() / np.abs(want).max()
    print("offset detector: device against the oracle, max-abs error %.3g of max" % err)
    assert err <= W.FILTER_TOL


# ---- 7. the product paths ------------------------------------------------------------------------------------------------------

def test_product_paths_at_1024(oracle):
    import torch
    n, grid, pairs = 1024, 1024, (200, 511, 822)   # the grid is taller than the cone: three depths inside it
    g = (n, n, 0.2, 0.2, -320.0, 0, 500, 500, 1.0)
    det, odet = B.DetectorGeometry(*g), oracle.DetectorGeometry(*g)
    idxs = list(range(360))
    nat = B.calculate_volume_geometry(det)
    l_vx = float(np.float32(nat.l_vx_x) * np.float32(nat.dim_x) / np.float32(grid))
    vg, ovg = B.VolumeGeometry(grid, grid, grid, l_vx, l_vx, l_vx), oracle.VolumeGeometry(grid, grid, grid, l_vx, l_vx, l_vx)
    free, _ = torch.cuda.mem_get_info(0)
    if free < 2 * 4 * grid ** 3 + (8 << 30):
        pytest.skip("needs two 4 GiB volumes and room")
    dev = torch.device("cuda", 0)
    problems = []
    want = [np.zeros((2, grid, grid), np.float32) for _ in pairs]

    def run(configure, read_back):
        be = B.Backend(0, synchronous=False)
        configure(be)
        v = be.make_volume_device(grid, grid, grid)
        for j, i, raw in W.frames_ahead(oracle, n, idxs):
            d_p = be.make_projection_device(n, n)
            W.upload(be, d_p, raw)
            d_p.idx = i
            B.stage_offset_detector_weight(be, d_p, det)
            B.weight(be, d_p, det)
            B.filter(be, d_p, det)
            if read_back:
                frame = W.to_host(be, d_p)
                s, c, ods, odt = oracle.backproject_constants(odet, i)
                for w, z in zip(want, pairs):
                    oracle.backproject(w, frame, z, odet, ovg, s, c, ods, odt, None)
            B.backproject(be, d_p, v, 0, det, vg, False, False, None)
            be.free(d_p)
        be.flush()
        be.synchronize()
        torch.cuda.synchronize()
        return be, v

    def plain(be):
        be.set_backproject_deferral(1)
        be.set_stage_fusion(False)
        be.set_backproject_references(False)

    def fusion(be):
        be.set_backproject_deferral(1)
        be.set_stage_fusion(True)
        be.set_backproject_references(False)

    def snapshots(be):
        be.set_paris_loop_defaults(37)
        be.set_backproject_references(False)

    pbe, v_plain = run(plain, True)
    try:
        t_plain = W.device_view(torch, v_plain, dev)
        for w, z in zip(want, pairs):
            W.compare_slices("offset detector: plain run against the oracle", t_plain[z:z + 2].cpu().numpy(), w, z, problems)
            assert np.count_nonzero(w) > grid * grid // 2
        for name, configure in (("stage fusion", fusion), ("references, depth 48", lambda be: be.set_paris_loop_defaults(48)),
                                ("snapshots, depth 37", snapshots)):
            abe, v = run(configure, False)
            W.compare_volumes(torch, "offset detector: %s against the plain run" % name, W.device_view(torch, v, dev), t_plain, problems)
            torch.cuda.synchronize()
            abe.free(v)
            abe.close()
        del t_plain
        pbe.free(v_plain)
    finally:
        pbe.close()
    assert not problems, "\n".join(problems)


# ---- 8. the C++ mirror and the driver ------------------------------------------------------------------------------------------

DRV_GEO = H.DRV_GEO   # 64 columns at delta_s = -16: an overlap of 16 pixels


def mirror_volume(frames, weighted, flat=None):
    det = B.DetectorGeometry(*DRV_GEO)
    vg = B.calculate_volume_geometry(det)
    with B.Backend(0) as mbe:
        if flat is not None:
            mbe.set_flat_field(None, flat)
        v = mbe.make_volume_device(vg.dim_x, vg.dim_y, vg.dim_z)
        for i, fr in enumerate(frames):
            d_p = B.load(mbe, B.Projection(fr.astype(np.float32), 64, 48, idx=i))
            if flat is not None:
                mbe.flat_field_rows(d_p)
            if weighted:
                B.stage_offset_detector_weight(mbe, d_p, det)
            B.weight(mbe, d_p, det)
            B.filter(mbe, d_p, det)
            B.backproject(mbe, d_p, v, 0, det, vg, False, False, None)
            mbe.free(d_p)
        h = mbe.make_volume_host(vg.dim_x, vg.dim_y, vg.dim_z)
        mbe.copy_d2h(v, h)
    return h.buf.reshape(vg.dim_z, vg.dim_y, vg.dim_x).copy()


def test_driver_and_cpp_mirror_against_the_python_mirror(tmp_path, oracle):
    n_frames = 360
    fr = np.stack([(oracle.lcg_projection(64, 48, i) * 30000 + 1000).astype(np.uint16) for i in range(n_frames)])
    d = tmp_path / "in"
    d.mkdir()
    (d / "a.his").write_bytes(F.his_file_bytes(fr[:170], 4, 32))
    (d / "b.his").write_bytes(F.his_file_bytes(fr[170:], 4, 32))
    flat = np.full((2, 48, 64), 40000, np.uint16)
    flat[1] += 2
    (tmp_path / "flat.his").write_bytes(F.his_file_bytes(flat, 4))
    geo = tmp_path / "geo.ini"
    geo.write_text("\n".join("%s = %s" % kv for kv in zip(GEO_KEYS, DRV_GEO)) + "\n")
    want = mirror_volume(fr, True)
    want_off = mirror_volume(fr, False)
    assert H.rel_rms(want, want_off, 1.0) > 0.1                # the weight made a difference
    for k, extra in enumerate((["--slabs", 1], ["--slabs", 3], ["--slabs", 3, "--no-row-band"], ["--slabs", 1, "--batch", 1],
                               ["--slabs", 3, "--batch", 5, "--no-read-ahead"], ["--slabs", 3, "--batch", 1, "--no-read-ahead"])):
        P.run(["--geometry", geo, "--input", d, "--output", tmp_path / ("o%d" % k), "--offset-detector"] + extra)
        _, vol = F.ddbvf_read(str(tmp_path / ("o%d" % k) / "vol.ddbvf"))
        assert np.array_equal(bits(vol), bits(want)), extra
    # with --flat (a zero dark): corrected first, then weighted
    want_flat = mirror_volume(fr, True, flat=np.full((48, 64), 40001, np.float32))
    for k, extra in enumerate((["--slabs", 1], ["--slabs", 3, "--batch", 1])):
        P.run(["--geometry", geo, "--input", d, "--output", tmp_path / ("f%d" % k), "--offset-detector", "--flat", tmp_path / "flat.his"] + extra)
        _, vol = F.ddbvf_read(str(tmp_path / ("f%d" % k) / "vol.ddbvf"))
        assert np.array_equal(bits(vol), bits(want_flat)), extra
    # PARIS's loop through paris::hip with set_offset_detector (paris_hip_demo --offset-detector)
    raw = tmp_path / "in.raw"
    fr.astype(np.float32).tofile(raw)
    out = tmp_path / "demo.raw"
    demo = [DEMO] + [str(v) for v in DRV_GEO] + [str(n_frames), str(raw), str(out)]
    r = subprocess.run(demo + ["--slabs", "2", "--offset-detector"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr + r.stdout
    got = np.fromfile(out, np.float32).reshape(want.shape)
    assert np.array_equal(bits(got), bits(want))
    # a short scan and an offset detector on the same ctx: whichever setter comes second throws
    r = subprocess.run(demo + ["--offset-detector", "--short-scan", "0", "359"], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "set_short_scan(): an offset detector is set" in (r.stderr + r.stdout), r.stderr + r.stdout
    r = subprocess.run(demo + ["--short-scan", "0", "359", "--offset-detector"], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "set_offset_detector(): a short scan is set" in (r.stderr + r.stdout), r.stderr + r.stdout
