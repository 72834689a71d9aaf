"""Short scans on the device: the Parker redundancy weight (paris_hip_short_scan_weight_rows, short_scan.hip) against a float64
restatement of its table, its convention checked by conjugate rays alone, its launch forms, the quality of short-scan
reconstructions against the full circle, the product paths against each other and the oracle, and the C++ mirror and driver."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import phantom
import test_gpu_paris_hip as P
import test_gpu_whole_circle as W
from oracle import formats as F
from paris_amd import _lib
from paris_amd import backend as B

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEMO = os.path.join(ROOT, "paris_amd", "host", "demo", "paris_hip_demo")
W_TOL = 1e-7       # |w - w_float64| of the formula (measured: 3.0e-8, the rounding of 2 w to fp32)
CONJ_TOL = 4e-7    # |2 w(ray) + 2 w(conjugate) - 2| (measured: 8.9e-8)
GEO_KEYS = ("n_row", "n_col", "l_px_row", "l_px_col", "delta_s", "delta_t", "d_so", "d_od", "delta_phi")


def f64(x):
    return float(np.float32(x))


def gammas(det):
    """fan angle [rad] of every column, in the backprojector's coordinates"""
    l, n = f64(det.l_px_row), det.n_row
    d_sd = abs(f64(det.d_so)) + abs(f64(det.d_od))
    t = (np.arange(n) + 0.5) * l - n * l / 2 - f64(det.delta_s) * l
    return np.arctan(t / d_sd)


def parker(det, start, rng, phis):
    """the weight table of DESIGN.md section 4.5 in float64: w[frame, column]"""
    g = gammas(det)[None, :]
    delta = (f64(rng) * math.pi / 180 - math.pi) / 2
    b = (np.mod(np.asarray(phis, np.float32).astype(np.float64) - f64(start), 360.0) * math.pi / 180)[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        rise = np.sin(math.pi / 4 * b / (delta - g)) ** 2
        fall = np.sin(math.pi / 4 * (math.pi + 2 * delta - b) / (delta + g)) ** 2
    w = np.zeros(np.broadcast(b, g).shape)
    w = np.where((b >= 0) & (b < 2 * delta - 2 * g), rise, w)
    w = np.where((b >= 2 * delta - 2 * g) & (b <= math.pi - 2 * g), 1.0, w)
    w = np.where((b > math.pi - 2 * g) & (b <= math.pi + 2 * delta), fall, w)
    return w


def minimal_range(det):
    g = float(np.abs(gammas(det)[[0, -1]]).max())
    r = np.float32(math.degrees(math.pi + 2 * g))
    while float(r) * math.pi / 180 - math.pi < 2 * g:
        r = np.nextafter(r, np.float32(np.inf))
    return float(r)


@pytest.fixture
def be():
    with B.Backend(0) as b:
        yield b


def frames_device(be, frames):
    """(n, dim_y, dim_x) float32 -> one device buffer of n frames one under the other; (first frame, frame stride in bytes)"""
    n, dim_y, dim_x = frames.shape
    d = be.make_projection_device(dim_x, n * dim_y)
    be.copy_h2d(B.Projection(np.ascontiguousarray(frames.reshape(n * dim_y, dim_x)), dim_x, n * dim_y), d)
    return d, B.Projection(d.ptr, dim_x, dim_y, pitch=d.pitch, on_device=True), d.pitch * dim_y


def frames_host(be, d, n, dim_y):
    h = be.make_projection_host(d.dim_x, d.dim_y)
    be.copy_d2h(d, h)
    return h.buf.reshape(n, dim_y, d.dim_x)


def weigh(be, det, start, rng, phis, frames):
    d, first, stride = frames_device(be, frames)
    be.short_scan_weight(first, det, (start, rng), phis, frame_stride=stride)
    out = frames_host(be, d, *frames.shape[:2])
    be.free(d)
    return out


def lcg_frames(oracle, n, dim_y, dim_x, seed=0):
    return np.stack([oracle.lcg_projection(dim_x, dim_y, seed + k) for k in range(n)])


# ---- 1. the formula ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("delta_s", [0.0, 1.5, -3.5])
def test_formula_against_float64(be, oracle, delta_s):
    det = B.DetectorGeometry(128, 128, 0.8, 0.8, delta_s, 0.0, 500, 500, 1.0)
    start, rng = 37.0, 200.0
    g = gammas(det)
    delta = (rng * math.pi / 180 - math.pi) / 2
    beta = list(np.linspace(-20.0, rng + 20.0, 121))                   # across the interval and outside it
    for i in (0, 17, 64, 127):                                         # just inside and outside every region boundary of 4 columns
        for edge in (0.0, 2 * delta - 2 * g[i], math.pi - 2 * g[i], math.pi + 2 * delta):
            beta += [math.degrees(edge) + e for e in (-1e-3, -1e-5, 1e-5, 1e-3)]
    phis = np.array([start + b for b in beta], np.float32)
    assert len(phis) >= 180
    want = parker(det, start, rng, phis)
    ones = weigh(be, det, start, rng, phis, np.ones((len(phis), 4, 128), np.float32))
    assert (ones == ones[:, :1, :]).all()                              # one weight per column, every row
    w2 = ones[:, 0, :]
    err = np.abs(w2.astype(np.float64) / 2 - want)
    print("short scan, delta_s %g: max |w - w_float64| = %.3g" % (delta_s, err.max()))
    assert err.max() <= W_TOL
    raw = lcg_frames(oracle, len(phis), 4, 128)
    got = weigh(be, det, start, rng, phis, raw)
    assert np.array_equal(got.view(np.uint32), (raw * w2[:, None, :]).view(np.uint32))
    middle = (want == 1.0).all(axis=1)
    outside = (want == 0.0).all(axis=1)
    assert middle.sum() >= 20 and outside.sum() >= 10
    assert (w2[middle] == 2.0).all() and np.array_equal(got[middle].view(np.uint32), (raw[middle] * 2).view(np.uint32))
    assert (got[outside] == 0).all()


# ---- 2. the convention ---------------------------------------------------------------------------------------------------------

def test_conjugate_rays_add_up_to_one(be):
    """delta_s = 0: column n-1-i has fan angle -gamma_i, so the ray (phi, i) is measured again as (phi + pi + 2 gamma_i, n-1-i). The
    weights read back for the two must add up to 1 -- a flipped sign of gamma breaks this, whatever the formula. The scan starts at
    -190 degrees so that the conjugates of the first ramp lie near 0 degrees, where float32 angles are fine enough."""
    det = B.DetectorGeometry(128, 128, 0.8, 0.8, 0.0, 0.0, 500, 500, 1.0)
    n = det.n_row
    g = gammas(det)
    assert np.array_equal(g[::-1], -g)
    start, rng = -190.0, 200.0
    delta = (rng * math.pi / 180 - math.pi) / 2
    beta = np.concatenate([np.linspace(0, math.degrees(2 * delta - 2 * g.min()), 20),
                           np.linspace(math.degrees(2 * delta), math.degrees(math.pi - 2 * g.max()), 6)])
    phi = np.array([start + b for b in beta], np.float32)
    conj = np.array([[p + 180.0 + 2 * math.degrees(gi) for gi in g] for p in phi.astype(np.float64)], np.float32)   # (k, i)
    phis = np.concatenate([phi, conj.ravel()])
    w2 = weigh(be, det, start, rng, phis, np.ones((len(phis), 2, n), np.float32))[:, 0, :].astype(np.float64)
    a = w2[:len(phi)]                                                   # w(phi_k, i)
    b = w2[len(phi):].reshape(len(phi), n, n)[:, np.arange(n), np.arange(n)[::-1]]   # w(conj_{k,i}, n-1-i)
    err = np.abs(a + b - 2.0)
    print("short scan: max |2w + 2w_conjugate - 2| = %.3g" % err.max())
    assert err.max() <= CONJ_TOL
    assert (a > 0).any() and (a < 2).any() and (b > 0).any()           # the ramps were sampled


def test_minimal_range_gives_finite_weights(be):
    for ds in (0.0, 3.5):
        det = B.DetectorGeometry(128, 128, 0.8, 0.8, ds, 0.0, 500, 500, 1.0)
        rng = minimal_range(det)
        B.short_scan_check(det, 37.0, rng)
        phis = np.array([37.0 + b for b in np.linspace(-2.0, rng + 2.0, 1201)], np.float32)
        w2 = weigh(be, det, 37.0, rng, phis, np.ones((len(phis), 2, 128), np.float32))
        assert np.isfinite(w2).all() and (w2 >= 0).all() and (w2 <= 2).all()
        assert np.abs(w2[:, 0, :] / 2 - parker(det, 37.0, rng, phis)).max() <= W_TOL


# ---- 3. the launch forms -------------------------------------------------------------------------------------------------------

def test_row_band_batch_and_stage_forms(be, oracle):
    det = B.DetectorGeometry(128, 96, 0.8, 0.8, 1.5, 0.0, 500, 500, 1.0)
    scan = B.ShortScan(37.0, 200.0)
    phis = np.array([37.0, 40.5, 120.0, 230.0, 236.5], np.float32)
    raw = lcg_frames(oracle, len(phis), 96, 128, 7)
    whole = weigh(be, det, 37.0, 200.0, phis, raw)
    single = np.stack([weigh(be, det, 37.0, 200.0, phis[k:k + 1], raw[k:k + 1])[0] for k in range(len(phis))])
    assert np.array_equal(whole.view(np.uint32), single.view(np.uint32))
    d, first, stride = frames_device(be, raw)
    be.short_scan_weight(first, det, scan, phis, row_first=37, row_count=50, frame_stride=stride)
    band = frames_host(be, d, len(phis), 96)
    assert np.array_equal(band[:, 37:87].view(np.uint32), whole[:, 37:87].view(np.uint32))
    assert np.array_equal(band[:, :37].view(np.uint32), raw[:, :37].view(np.uint32))
    assert np.array_equal(band[:, 87:].view(np.uint32), raw[:, 87:].view(np.uint32))
    be.free(d)
    # the stage form resolves the angle as the backprojection does: idx * delta_phi, or phi with angles enabled
    for k in (1, 3):
        d = B.load(be, B.Projection(raw[k].copy(), 128, 96, idx=int(round(float(phis[k]))), phi=float(phis[k])))
        B.stage_short_scan_weight(be, d, det, scan, enable_angles=True)
        h = be.make_projection_host(128, 96)
        be.copy_d2h(d, h)
        assert np.array_equal(h.buf.view(np.uint32), whole[k].view(np.uint32))
        be.free(d)
    d = B.load(be, B.Projection(raw[2].copy(), 128, 96, idx=120))
    B.stage_short_scan_weight(be, d, det, scan)
    h = be.make_projection_host(128, 96)
    be.copy_d2h(d, h)
    assert np.array_equal(h.buf.view(np.uint32), whole[2].view(np.uint32))
    be.free(d)


def test_argument_refusals(be, oracle):
    det = B.DetectorGeometry(64, 32, 0.8, 0.8, 0.0, 0.0, 500, 500, 1.0)
    L, ctx = be._L, be._ctx
    d = be.make_projection_device(64, 64)
    phi = (C.c_float * 2)(40.0, 41.0)
    ok, bad = B.ShortScan(37.0, 200.0), B.ShortScan(37.0, 180.0)

    def call(pitch=d.pitch, stride=d.pitch * 32, n=1, dim_x=64, dim_y=32, r0=0, rc=32, scan=ok, phis=phi, det_=det, ptr=d.ptr):
        return L.paris_hip_short_scan_weight_rows(ctx, ptr, pitch, stride, n, dim_x, dim_y, r0, rc, C.byref(det_),
                                                  C.byref(scan) if scan is not None else None, phis)
    assert call() == 0
    assert call(n=2) == 0
    inv = _lib.ERROR_INVALID_ARGUMENT
    assert call(pitch=64 * 4 - 4) == inv                         # pitch below a row
    assert call(pitch=d.pitch + 2) == inv                         # pitch not a whole number of floats
    assert call(r0=33) == inv and call(r0=8, rc=25) == inv        # rows out of range
    assert call(scan=bad) == inv and call(scan=None) == inv       # invalid scan
    assert call(scan=B.ShortScan(float("nan"), 200.0)) == inv
    assert call(phis=(C.c_float * 1)(float("nan"))) == inv         # non-finite angle
    assert call(phis=None) == inv
    assert call(dim_x=32) == inv                                  # columns are the detector's n_row
    assert call(n=2, stride=d.pitch * 31) == inv                  # overlapping frames
    assert call(ptr=None) == inv
    assert L.paris_hip_stage_short_scan_weight(ctx, d.ptr, d.pitch, 64, 32, C.byref(det), C.byref(bad), 40, 0, 0.0) == inv
    assert L.paris_hip_stage_short_scan_weight(ctx, d.ptr, d.pitch, 64, 32, None, C.byref(ok), 40, 0, 0.0) == inv
    assert call(rc=0) == 0 and call(n=0, phis=None) == 0          # nothing to do
    be.free(d)
    # still usable
    raw = lcg_frames(oracle, 1, 32, 64)
    got = weigh(be, det, 37.0, 200.0, np.array([150.0], np.float32), raw)
    assert np.array_equal(got.view(np.uint32), (raw * 2).view(np.uint32))


# ---- 4. quality against the full circle ----------------------------------------------------------------------------------------

def reconstruct(oracle, det, idxs, scan, frame):
    """the phantom through the Backend product path (set_paris_loop_defaults), PARIS's loop; scan None: no redundancy weight"""
    vg = B.calculate_volume_geometry(det)
    with B.Backend(0, synchronous=False) as abe:
        abe.set_paris_loop_defaults(48)
        v = abe.make_volume_device(vg.dim_x, vg.dim_y, vg.dim_z)
        for i in idxs:
            d_p = abe.make_projection_device(det.n_row, det.n_col)
            W.upload(abe, d_p, frame(i))
            d_p.idx = i
            if scan is not None:
                B.stage_short_scan_weight(abe, d_p, det, scan)
            B.weight(abe, d_p, det)
            B.filter(abe, d_p, det)
            B.backproject(abe, d_p, v, 0, det, vg, False, False, None)
            abe.free(d_p)
        abe.flush()
        h = abe.make_volume_host(vg.dim_x, vg.dim_y, vg.dim_z)
        abe.copy_d2h(v, h)
        abe.free(v)
    return h.buf.reshape(vg.dim_z, vg.dim_y, vg.dim_x).copy()


def rel_rms(got, ref, scale=None):
    """over the central quarter of the slices, inside 0.45 dim_x of the axis; scale None: the best scale for got"""
    dz, dy, dx = ref.shape
    y, x = np.mgrid[:dy, :dx]
    mask = np.hypot(x - (dx - 1) / 2, y - (dy - 1) / 2) <= 0.45 * dx
    a = got[3 * dz // 8:5 * dz // 8][:, mask].astype(np.float64)
    b = ref[3 * dz // 8:5 * dz // 8][:, mask].astype(np.float64)
    if scale is None:
        scale = (a * b).sum() / (a * a).sum()
    return float(np.sqrt(((scale * a - b) ** 2).mean() / (b ** 2).mean()))


def test_quality_against_the_full_circle(oracle):
    results = {}
    full = {}
    for ds in (0.0, 3.5):
        det = B.DetectorGeometry(128, 128, 0.8, 0.8, ds, 0.0, 500, 500, 1.0)
        vg = B.calculate_volume_geometry(det)
        radius = 0.9 * vg.dim_x * vg.l_vx_x / 2

        def frame(i, det=det, radius=radius):
            return phantom.projection(128, 128, 0.8, 0.8, 500, 500, f64(np.float32(i) * det.delta_phi), radius, det.delta_s)
        full[ds] = (det, frame, reconstruct(oracle, det, list(range(360)), None, frame))
    det, frame, ref = full[0.0]
    results["186 degrees"] = rel_rms(reconstruct(oracle, det, list(range(37, 224)), B.ShortScan(37.0, 186.0), frame), ref, 1.0)
    unweighted = reconstruct(oracle, det, list(range(37, 224)), None, frame)
    results["unweighted"] = rel_rms(unweighted, ref, 1.0)
    results["unweighted, best scale"] = rel_rms(unweighted, ref)
    det3, frame3, ref3 = full[3.5]
    results["197 degrees, delta_s 3.5"] = rel_rms(reconstruct(oracle, det3, list(range(37, 235)), B.ShortScan(37.0, 197.0), frame3), ref3, 1.0)
    down = B.DetectorGeometry(128, 128, 0.8, 0.8, 0.0, 0.0, 500, 500, -1.0)
    vg = B.calculate_volume_geometry(down)

    def frame_down(i, radius=0.9 * vg.dim_x * vg.l_vx_x / 2):
        return phantom.projection(128, 128, 0.8, 0.8, 500, 500, f64(np.float32(i) * np.float32(-1.0)), radius)
    results["186 degrees descending"] = rel_rms(reconstruct(oracle, down, list(range(187)), B.ShortScan(-186.0, 186.0), frame_down), ref, 1.0)
    print("short scan quality (relative RMS against the full circle): %s" % ", ".join("%s %.4f" % kv for kv in results.items()))
    assert results["186 degrees"] <= 0.03
    assert results["197 degrees, delta_s 3.5"] <= 0.03
    assert results["186 degrees descending"] <= 0.03
    assert results["unweighted"] > 0.3
    assert results["186 degrees"] < results["unweighted, best scale"]   # the weight does more than fix the scale


# ---- 5. the product paths ------------------------------------------------------------------------------------------------------

def test_product_paths_at_1024(oracle):
    import torch
    n, grid, pairs = 1024, 1024, (0, 511, 1022)
    g = (n, n, 0.2, 0.2, 0, 0, 500, 500, 0.5)
    det, odet = B.DetectorGeometry(*g), oracle.DetectorGeometry(*g)
    rng = math.ceil(minimal_range(det) / 0.5) * 0.5
    idxs = list(range(int(rng / 0.5) + 1))
    scan = B.ShortScan(0.0, rng)
    nat = B.calculate_volume_geometry(det)
    l_vx = float(np.float32(nat.l_vx_x) * np.float32(n) / np.float32(grid))
    vg, ovg = B.VolumeGeometry(grid, grid, grid, l_vx, l_vx, l_vx), oracle.VolumeGeometry(grid, grid, grid, l_vx, l_vx, l_vx)
    free, _ = torch.cuda.mem_get_info(0)
    if free < 2 * 4 * grid ** 3 + (8 << 30):
        pytest.skip("needs two 4 GiB volumes and room")
    dev = torch.device("cuda", 0)
    problems = []
    want = [np.zeros((2, grid, grid), np.float32) for _ in pairs]

    def run(name, configure, read_back):
        be = B.Backend(0, synchronous=False)
        configure(be)
        v = be.make_volume_device(grid, grid, grid)
        for j, i, raw in W.frames_ahead(oracle, n, idxs):
            d_p = be.make_projection_device(n, n)
            W.upload(be, d_p, raw)
            d_p.idx = i
            B.stage_short_scan_weight(be, d_p, det, scan)
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

    pbe, v_plain = run("plain", plain, True)
    try:
        t_plain = W.device_view(torch, v_plain, dev)
        for w, z in zip(want, pairs):
            W.compare_slices("short scan: plain run against the oracle", t_plain[z:z + 2].cpu().numpy(), w, z, problems)
            assert np.count_nonzero(w) > grid * grid
        for name, configure in (("stage fusion", fusion), ("references, depth 48", lambda be: be.set_paris_loop_defaults(48)),
                                ("snapshots, depth 37", snapshots)):
            abe, v = run(name, configure, False)
            W.compare_volumes(torch, "short scan: %s against the plain run" % name, W.device_view(torch, v, dev), t_plain, problems)
            torch.cuda.synchronize()
            abe.free(v)
            abe.close()
        del t_plain
        pbe.free(v_plain)
    finally:
        pbe.close()
    assert not problems, "\n".join(problems)


# ---- 6. the C++ mirror and the driver ------------------------------------------------------------------------------------------

DRV_GEO = (64, 48, 0.2, 0.25, 1.5, -0.75, 100, 200, 1.0)


def mirror_volume(frames, scan):
    det = B.DetectorGeometry(*DRV_GEO)
    vg = B.calculate_volume_geometry(det)
    with B.Backend(0) as be:
        v = be.make_volume_device(vg.dim_x, vg.dim_y, vg.dim_z)
        for i, fr in enumerate(frames):
            d_p = B.load(be, B.Projection(fr.astype(np.float32), 64, 48, idx=i))
            if scan is not None:
                B.stage_short_scan_weight(be, d_p, det, scan)
            B.weight(be, d_p, det)
            B.filter(be, d_p, det)
            B.backproject(be, d_p, v, 0, det, vg, False, False, None)
            be.free(d_p)
        h = be.make_volume_host(vg.dim_x, vg.dim_y, vg.dim_z)
        be.copy_d2h(v, h)
    return h.buf.reshape(vg.dim_z, vg.dim_y, vg.dim_x).copy()


def test_driver_and_cpp_mirror_against_the_python_mirror(tmp_path, oracle):
    det = B.DetectorGeometry(*DRV_GEO)
    n_frames = int(math.ceil(minimal_range(det))) + 1          # 1 degree steps from 0: the smallest whole-degree range
    rng = float(n_frames - 1)
    fr = np.stack([(oracle.lcg_projection(64, 48, i) * 60000).astype(np.uint16) for i in range(n_frames)])
    d = tmp_path / "in"
    d.mkdir()
    (d / "a.his").write_bytes(F.his_file_bytes(fr[:70], 4, 32))
    (d / "b.his").write_bytes(F.his_file_bytes(fr[70:], 4, 32))
    geo = tmp_path / "geo.ini"
    geo.write_text("\n".join("%s = %s" % kv for kv in zip(GEO_KEYS, DRV_GEO)) + "\n")
    want = mirror_volume(fr, B.ShortScan(0.0, rng))
    want_off = mirror_volume(fr, None)
    assert rel_rms(want, want_off, 1.0) > 0.1                # the weight made a difference
    for k, extra in enumerate((["--slabs", 1], ["--slabs", 3], ["--slabs", 3, "--no-row-band"], ["--slabs", 1, "--batch", 1],
                               ["--slabs", 3, "--batch", 5, "--no-read-ahead"])):
        P.run(["--geometry", geo, "--input", d, "--output", tmp_path / ("o%d" % k), "--short-scan"] + extra)
        _, vol = F.ddbvf_read(str(tmp_path / ("o%d" % k) / "vol.ddbvf"))
        assert np.array_equal(vol.view(np.uint32), want.view(np.uint32)), extra
    P.run(["--geometry", geo, "--input", d, "--output", tmp_path / "off", "--slabs", 3])   # the feature off: today's volume
    _, vol = F.ddbvf_read(str(tmp_path / "off" / "vol.ddbvf"))
    assert np.array_equal(vol.view(np.uint32), want_off.view(np.uint32))
    # PARIS's loop through paris::hip with set_short_scan (paris_hip_demo --short-scan)
    raw = tmp_path / "in.raw"
    fr.astype(np.float32).tofile(raw)
    out = tmp_path / "demo.raw"
    r = subprocess.run([DEMO] + [str(v) for v in DRV_GEO] + [str(n_frames), str(raw), str(out), "--slabs", "2", "--short-scan", "0", repr(rng)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr + r.stdout
    got = np.fromfile(out, np.float32).reshape(want.shape)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # an insufficient range is a stage_runtime_error at the first weight()
    r = subprocess.run([DEMO] + [str(v) for v in DRV_GEO] + [str(n_frames), str(raw), str(out), "--short-scan", "0", "180"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "weight()" in (r.stderr + r.stdout)
