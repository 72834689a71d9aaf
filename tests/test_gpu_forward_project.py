"""The forward projector on the device (paris_hip_forward_project, forward_project.hip) against the float64 restatement of its
statement (tests/forward_model.py) within the fp32 figures calibrated on the CPU (tests/test_forward_project_host.py): its launch
forms, refusals and ordering against deferred work, analytic blobs, a 512^3 and a 2048^3 volume, and the C++ mirror."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import forward_model as M
import test_forward_project_host as H
from paris_amd import _lib
from paris_amd import backend as B

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEMO = os.path.join(ROOT, "paris_amd", "host", "demo", "paris_hip_demo")
ANGLES = (0.0, 30.0, 45.0, 90.0, 137.0, 315.0)


@pytest.fixture
def be():
    with B.Backend(0) as b:
        yield b


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def upload_volume(be, vol):
    dz, dy, dx = vol.shape
    d = be.make_volume_device(dx, dy, dz)
    be.copy_h2d(B.Volume(np.ascontiguousarray(vol, np.float32), dx, dy, dz), d)
    return d


def frame_stack(be, n, det, pad=0, fill=None):
    """n frames one under the other in one device buffer of n_row + pad columns (the columns beyond n_row play pitch padding),
    holding fill (n, n_col, n_row + pad) if given; the buffer, a Projection of the first frame and the frame stride in bytes"""
    w = det.n_row + pad
    d = be.make_projection_device(w, n * det.n_col)
    if fill is not None:
        be.copy_h2d(B.Projection(np.ascontiguousarray(fill.reshape(n * det.n_col, w), np.float32), w, n * det.n_col), d)
    return d, B.Projection(d.ptr, det.n_row, det.n_col, pitch=d.pitch, on_device=True), d.pitch * det.n_col


def read_stack(be, d, n, det):
    h = be.make_projection_host(d.dim_x, d.dim_y)
    be.copy_d2h(d, h)
    return h.buf.reshape(n, det.n_col, d.dim_x).copy()


def to_host(be, d_p):
    h = be.make_projection_host(d_p.dim_x, d_p.dim_y)
    be.copy_d2h(d_p, h)
    return h.buf.copy()


def device_views(be, d_v, v_offset, det, vg, angles):
    """the views at `angles` (degrees) in one call: (n, n_col, n_row) float32"""
    sc = [M.view_sin_cos(a) for a in angles]
    ds, dt = M.offsets_mm(det)
    d, first, stride = frame_stack(be, len(angles), det)
    be.forward_project(d_v, v_offset, det, vg, first, [s for s, _ in sc], [c for _, c in sc], ds, dt, frame_stride=stride)
    out = read_stack(be, d, len(angles), det)
    be.free(d)
    return out


def restated(vol, v_offset, det, vg, angle, **kw):
    s, c = M.view_sin_cos(angle)
    ds, dt = M.offsets_mm(det)
    return M.forward_project(vol, v_offset, det, vg, s, c, ds, dt, **kw)


def rel_max(got, want):
    return np.abs(got.astype(np.float64) - want).max() / np.abs(want).max()


# ---- 1. the device against the float64 restatement -----------------------------------------------------------------------------

@pytest.mark.parametrize("n", [64, 256])
def test_device_against_float64(be, n):
    det, vg = M.geometry(B, n)
    vol = M.random_volume(n)
    d_v = upload_volume(be, vol)
    got = device_views(be, d_v, 0, det, vg, ANGLES)
    errs = [rel_max(got[k], restated(vol, 0, det, vg, a)) for k, a in enumerate(ANGLES)]
    print("forward projector at %d^3 against float64 (max error over max): %s; fp32 transcription %.3e"
          % (n, ", ".join("%g deg %.3e" % ae for ae in zip(ANGLES, errs)), H.FP32_CAL[n]))
    assert max(errs) <= 2 * H.FP32_CAL[n]


# ---- 2. the forms --------------------------------------------------------------------------------------------------------------

def test_batch_single_stage_and_accumulate_forms(be):
    n = 64
    det, vg = M.geometry(B, n)
    vol = M.random_volume(n)
    d_v = upload_volume(be, vol)
    ds, dt = M.offsets_mm(det)
    sc = [M.view_sin_cos(a) for a in ANGLES]
    rng = np.random.default_rng(5)
    fill = rng.random((len(ANGLES), det.n_col, n + 32), dtype=np.float32)
    d, first, stride = frame_stack(be, len(ANGLES), det, 32, fill)
    be.forward_project(d_v, 0, det, vg, first, [s for s, _ in sc], [c for _, c in sc], ds, dt, frame_stride=stride)
    batch = read_stack(be, d, len(ANGLES), det)
    be.free(d)
    assert np.array_equal(bits(batch[:, :, n:]), bits(fill[:, :, n:]))                  # the padding is untouched
    assert not np.array_equal(bits(batch[:, :, :n]), bits(fill[:, :, :n]))
    singles = []
    for k, (s, c) in enumerate(sc):
        d, first, _ = frame_stack(be, 1, det, 32, fill[k:k + 1])
        be.forward_project(d_v, 0, det, vg, first, s, c, ds, dt)
        singles.append(read_stack(be, d, 1, det)[0])
        be.free(d)
    assert np.array_equal(bits(batch), bits(np.stack(singles)))                         # n views in one call: n single calls
    # the stage wrapper: the angle from idx * delta_phi, the offsets from the geometry
    sdet = B.DetectorGeometry(det.n_row, det.n_col, det.l_px_row, det.l_px_col, det.delta_s, det.delta_t, det.d_so, det.d_od, 7.5)
    for idx, phi, enable in ((5, 0.0, False), (0, 137.0, True)):
        d_p = be.make_projection_device(det.n_row, det.n_col)
        d_p.idx, d_p.phi = idx, phi
        B.forward_project(be, d_v, 0, d_p, sdet, vg, enable_angles=enable)
        s, c = B.stage_angle(sdet, idx, enable, phi)
        d_q = be.make_projection_device(det.n_row, det.n_col)
        be.forward_project(d_v, 0, sdet, vg, d_q, s, c, ds, dt)
        assert np.array_equal(bits(to_host(be, d_p)), bits(to_host(be, d_q)))
        be.free(d_p)
        be.free(d_q)
    # accumulate onto a random frame: frame + single result, one fp32 addition
    k = 2
    d, first, _ = frame_stack(be, 1, det, 32, fill[k:k + 1])
    be.forward_project(d_v, 0, det, vg, first, sc[k][0], sc[k][1], ds, dt, accumulate=True)
    acc = read_stack(be, d, 1, det)[0]
    be.free(d)
    assert np.array_equal(bits(acc[:, :n]), bits(fill[k, :, :n] + singles[k][:, :n])) and np.array_equal(bits(acc[:, n:]), bits(fill[k, :, n:]))
    # three slabs with accumulate: the whole volume's projection, each added slab rounding the pixel once more
    worst = 0.0
    for a in (45.0, 137.0):
        s, c = M.view_sin_cos(a)
        d_p = be.make_projection_device(det.n_row, det.n_col)
        for j, (z0, z1) in enumerate(((0, 21), (21, 30), (30, 64))):
            d_s = upload_volume(be, vol[z0:z1])
            be.forward_project(d_s, z0, det, vg, d_p, s, c, ds, dt, accumulate=j > 0)
            be.free(d_s)
        worst = max(worst, rel_max(to_host(be, d_p), restated(vol, 0, det, vg, a)))
        be.free(d_p)
    print("forward projector, three slabs with accumulate against the whole volume's restatement: %.3e" % worst)
    assert worst <= 3 * H.FP32_CAL[n]


# ---- 3. the refusals -----------------------------------------------------------------------------------------------------------

def test_argument_refusals(be):
    n = 64
    det, vg = M.geometry(B, n)
    vol = M.random_volume(n)
    d_v = upload_volume(be, vol)
    ds, dt = M.offsets_mm(det)
    L, ctx = be._L, be._ctx
    fill = np.random.default_rng(9).random((2, det.n_col, n), dtype=np.float32)
    d, first, stride = frame_stack(be, 2, det, 0, fill)
    fp = C.POINTER(C.c_float)
    s0, c0 = M.view_sin_cos(30.0)

    def call(v=d_v.ptr, vx=n, vy=n, vz=n, off=0, det_=det, vg_=vg, p=d.ptr, pitch=d.pitch, stride_=stride, nv=1, px=det.n_row, py=det.n_col,
             sins=(s0, s0), coss=(c0, c0), ds_=ds, dt_=dt, acc=0):
        sa = (C.c_float * 2)(*sins) if sins is not None else None
        ca = (C.c_float * 2)(*coss) if coss is not None else None
        return L.paris_hip_forward_project(ctx, v, vx, vy, vz, off, C.byref(det_) if det_ is not None else None,
                                           C.byref(vg_) if vg_ is not None else None, p, pitch, stride_, nv, px, py,
                                           C.cast(sa, fp) if sa is not None else None, C.cast(ca, fp) if ca is not None else None, ds_, dt_, acc)

    def geo(k, v):
        g = [det.n_row, det.n_col, det.l_px_row, det.l_px_col, det.delta_s, det.delta_t, det.d_so, det.d_od, det.delta_phi]
        g[k] = v
        return B.DetectorGeometry(*g)

    def grid(k, v):
        g = [vg.dim_x, vg.dim_y, vg.dim_z, vg.l_vx_x, vg.l_vx_y, vg.l_vx_z]
        g[k] = v
        return B.VolumeGeometry(*g)

    inv = _lib.ERROR_INVALID_ARGUMENT
    nan, inf = float("nan"), float("inf")
    assert call() == 0 and call(nv=2) == 0
    assert L.paris_hip_forward_project(None, d_v.ptr, n, n, n, 0, C.byref(det), C.byref(vg), d.ptr, d.pitch, stride, 0, det.n_row, det.n_col,
                                       None, None, ds, dt, 0) == inv
    assert call(v=None) == inv and call(p=None) == inv and call(det_=None) == inv and call(vg_=None) == inv
    assert call(sins=None) == inv and call(coss=None) == inv
    assert call(px=n - 1) == inv and call(py=det.n_col - 1) == inv                          # the frame is the detector's
    assert call(pitch=4 * n - 4) == inv and call(pitch=d.pitch + 2) == inv                  # short pitch, not whole floats
    assert call(nv=2, stride_=d.pitch * (det.n_col - 1)) == inv and call(nv=2, stride_=stride + 2) == inv   # overlapping frames
    assert call(vx=n - 1) == inv and call(vy=n + 1) == inv                                  # the slab spans the grid in x and y
    assert call(vz=n, off=1) == inv and call(vz=n + 1) == inv and call(vz=1, off=n) == inv  # and lies inside it in z
    for k in (2, 3):
        for bad in (0.0, -1.0, nan, inf):
            assert call(det_=geo(k, bad)) == inv                                            # pixel sizes
    for k in (3, 4, 5):
        for bad in (0.0, -0.5, nan, inf):
            assert call(vg_=grid(k, bad)) == inv                                            # voxel sizes
    for bad in (0.0, -500.0, nan, inf):
        assert call(det_=geo(6, bad)) == inv                                                # d_so
    assert call(det_=geo(7, nan)) == inv and call(det_=geo(7, inf)) == inv                  # d_od
    assert call(sins=(nan, s0)) == inv and call(coss=(inf, c0)) == inv and call(nv=2, sins=(s0, nan)) == inv
    assert call(ds_=nan) == inv and call(dt_=inf) == inv
    # nothing to do; an empty slab writes zeros
    be.copy_h2d(B.Projection(np.ascontiguousarray(fill.reshape(2 * det.n_col, n)), n, 2 * det.n_col), d)
    assert call(nv=0) == 0 and call(nv=0, sins=None, coss=None) == 0 and call(vz=0, acc=1) == 0 and call(v=None, vz=0, acc=1) == 0
    assert np.array_equal(bits(read_stack(be, d, 2, det)), bits(fill))
    assert call(vz=0, off=n) == 0
    after = read_stack(be, d, 2, det)
    assert not after[0].any() and np.array_equal(bits(after[1]), bits(fill[1]))
    assert call(v=None, vz=0, nv=2) == 0
    assert not read_stack(be, d, 2, det).any()
    be.free(d)
    got = device_views(be, d_v, 0, det, vg, (30.0,))                                        # still usable
    assert rel_max(got[0], restated(vol, 0, det, vg, 30.0)) <= 2 * H.FP32_CAL[n]


# ---- 4. ordering against deferred work -----------------------------------------------------------------------------------------

def pending(be):
    n, ptr = C.c_uint32(0), C.c_void_p()
    assert be._L.paris_hip_pending_backprojections(be._ctx, C.byref(n), C.byref(ptr)) == 0
    return n.value


ORD_GEO = (64, 48, 0.2, 0.25, 1.5, -0.75, 100, 200, 45.0)


def test_reads_the_volume_behind_pending_backprojections(oracle):
    det = B.DetectorGeometry(*ORD_GEO)
    vg = B.calculate_volume_geometry(det)
    frames = [oracle.lcg_projection(det.n_row, det.n_col, i) for i in range(5)]

    def run(flush_first):
        with B.Backend(0, synchronous=False) as abe:
            abe.set_backproject_deferral(8)
            v = abe.make_volume_device(vg.dim_x, vg.dim_y, vg.dim_z)
            d_ps = [B.load(abe, B.Projection(f.copy(), det.n_row, det.n_col, idx=i)) for i, f in enumerate(frames)]
            out = abe.make_projection_device(det.n_row, det.n_col)
            out.idx = 3
            for d_p in d_ps:
                B.backproject(abe, d_p, v, 0, det, vg, False, False, None)
            assert pending(abe) == 5
            if flush_first:
                abe.flush()
                assert pending(abe) == 0
            B.forward_project(abe, v, 0, out, det, vg)
            assert pending(abe) == 0
            return to_host(abe, out)

    deferred, flushed = run(False), run(True)
    assert np.abs(flushed).max() > 0 and np.array_equal(bits(deferred), bits(flushed))


def test_writes_behind_a_held_back_weighting(oracle):
    det = B.DetectorGeometry(*ORD_GEO)
    vg = B.calculate_volume_geometry(det)
    vol = np.random.default_rng(3).random((vg.dim_z, vg.dim_y, vg.dim_x), dtype=np.float32)
    frame = oracle.lcg_projection(det.n_row, det.n_col, 11)

    def run(fusion, accumulate):
        with B.Backend(0, synchronous=False) as abe:
            abe.set_stage_fusion(fusion)
            v = upload_volume(abe, vol)
            d_p = B.load(abe, B.Projection(frame.copy(), det.n_row, det.n_col, idx=2))
            B.weight(abe, d_p, det)                                   # with fusion: held back until something touches the frame
            weighted = to_host(abe, d_p) if not fusion else None
            if fusion or accumulate is not None:
                B.forward_project(abe, v, 0, d_p, det, vg, accumulate=bool(accumulate))
            return weighted, to_host(abe, d_p)

    weighted, single = run(False, False)
    assert not np.array_equal(bits(weighted), bits(frame))
    assert np.array_equal(bits(run(True, True)[1]), bits(weighted + single))      # the weighting ran first, then the addition
    assert np.array_equal(bits(run(True, False)[1]), bits(single))                # and is not applied to the new frame afterwards


def test_destination_in_the_pending_group_by_reference(oracle):
    det = B.DetectorGeometry(*ORD_GEO)
    vg = B.calculate_volume_geometry(det)
    frame = oracle.lcg_projection(det.n_row, det.n_col, 4)

    def run(deferred):
        with B.Backend(0, synchronous=False) as abe:
            if deferred:
                abe.set_backproject_deferral(8)
                abe.set_backproject_references(True)
            v = abe.make_volume_device(vg.dim_x, vg.dim_y, vg.dim_z)
            d_p = B.load(abe, B.Projection(frame.copy(), det.n_row, det.n_col, idx=1))
            B.backproject(abe, d_p, v, 0, det, vg, False, False, None)
            if deferred:
                assert pending(abe) == 1
            B.forward_project(abe, v, 0, d_p, det, vg)                # the destination is the buffer the pending group reads
            p = to_host(abe, d_p)
            h = abe.make_volume_host(vg.dim_x, vg.dim_y, vg.dim_z)
            abe.copy_d2h(v, h)
            return p, h.buf.copy()

    want_p, want_v = run(False)
    got_p, got_v = run(True)
    assert np.abs(want_v).max() > 0 and np.abs(want_p).max() > 0
    assert np.array_equal(bits(got_v), bits(want_v)) and np.array_equal(bits(got_p), bits(want_p))


# ---- 5. analytic blobs ---------------------------------------------------------------------------------------------------------

def test_analytic_blobs_on_the_device(be):
    det, vg = M.blob_geometry(B)
    d_v = upload_volume(be, M.blob_volume(vg))
    ds, dt = M.offsets_mm(det)
    got = device_views(be, d_v, 0, det, vg, H.ANGLES)
    figures = [H.errors(got[k], M.blob_line_integrals(det, *M.view_sin_cos(a), ds, dt)) for k, a in enumerate(H.ANGLES)]
    print("forward projector against analytic blobs (max over max, relative RMS): %s"
          % ", ".join("%g deg %.3e %.3e" % ((a,) + f) for a, f in zip(H.ANGLES, figures)))
    assert max(f[0] for f in figures) <= H.CAL_MAX * H.BOUND
    assert max(f[1] for f in figures) <= H.CAL_RMS * H.BOUND


# ---- 6. size -------------------------------------------------------------------------------------------------------------------

def test_512_cube_in_full(be):
    n = 512
    det, vg = M.geometry(B, n)
    vol = M.random_volume(n)
    d_v = upload_volume(be, vol)
    angles = (45.0, 200.0)
    got = device_views(be, d_v, 0, det, vg, angles)
    errs = [rel_max(got[k], restated(vol, 0, det, vg, a)) for k, a in enumerate(angles)]
    print("forward projector at 512^3 against float64: %s; fp32 transcription %.3e"
          % (", ".join("%g deg %.3e" % ae for ae in zip(angles, errs)), H.FP32_CAL[n]))
    assert max(errs) <= 2 * H.FP32_CAL[n]


def test_2048_cube_on_sampled_rows():
    """32 GiB: voxel offsets beyond 2^32 floats and 2^32 bytes. The volume is a closed form of the voxel index that differs between
    the two halves of the address space, filled on the device; the restatement reads the same closed form."""
    import torch
    n = 2048
    free, _ = torch.cuda.mem_get_info(0)
    if free < 4 * n ** 3 + (6 << 30):
        pytest.skip("needs a 32 GiB volume and room: %.1f GiB free" % (free / 2.0 ** 30))
    det, vg = M.geometry(B, n, n_col=n, scale=0.25)
    rows = [int(r) for r in np.linspace(3, n - 4, 16)]
    angles = (45.0, 200.0)
    tap = M.closed_form_tap(n, n, n)
    assert tap(np.array([5]), np.array([7]), np.array([100]))[0] != tap(np.array([5]), np.array([7]), np.array([100 + n // 2]))[0]
    t = torch.empty((n, n, n), dtype=torch.float32, device=torch.device("cuda", 0))
    M.closed_form_fill(torch, t)
    torch.cuda.synchronize()
    probe = [(0, 0, 0), (n - 1, n - 1, n - 1), (1023, 77, 1024), (5, 7, 100), (5, 7, 100 + n // 2)]
    for ix, iy, iz in probe:
        assert float(t[iz, iy, ix]) == float(tap(np.array([ix]), np.array([iy]), np.array([iz]))[0])
    with B.Backend(0) as be:
        d_v = be.wrap_volume(t.data_ptr(), n, n, n, owner=t)
        got = device_views(be, d_v, 0, det, vg, angles)
    del t
    torch.cuda.empty_cache()
    for k, a in enumerate(angles):
        want = restated(tap, 0, det, vg, a, rows=rows, v_dim_z=n)
        single = restated(tap, 0, det, vg, a, rows=rows, v_dim_z=n, dtype=np.float32)
        cal = rel_max(single, want)
        err = rel_max(got[k][rows], want)
        print("forward projector at 2048^3, %g deg, 16 rows: %.3e of the maximum; fp32 transcription on those rows %.3e" % (a, err, cal))
        assert np.abs(want).max() > 100 and err <= 2 * cal


# ---- 7. the C++ mirror ---------------------------------------------------------------------------------------------------------

DEMO_GEO = (64, 48, 0.2, 0.25, 1.5, -0.75, 100, 200, 15.0)
DEMO_VIEWS = 24


def python_reprojection(oracle, slabs):
    """what paris_hip_demo --reproject does, through the Python mirror: per slab the reconstruction loop, then every view loaded from
    the host copy so far, the slab's part added (the first slab writes) and the view copied back"""
    det = B.DetectorGeometry(*DEMO_GEO)
    vg = B.calculate_volume_geometry(det)
    frames = [oracle.lcg_projection(det.n_row, det.n_col, i) for i in range(DEMO_VIEWS)]
    out = np.zeros((DEMO_VIEWS, det.n_col, det.n_row), np.float32)
    dz = vg.dim_z // slabs
    with B.Backend(0) as mbe:
        for k in range(slabs):
            v = mbe.make_volume_device(vg.dim_x, vg.dim_y, dz + (vg.dim_z % slabs if k == slabs - 1 else 0))
            for i, fr in enumerate(frames):
                d_p = B.load(mbe, B.Projection(fr.copy(), det.n_row, det.n_col, idx=i))
                B.weight(mbe, d_p, det)
                B.filter(mbe, d_p, det)
                B.backproject(mbe, d_p, v, k * dz, det, vg, False, False, None)
                mbe.free(d_p)
            for i in range(DEMO_VIEWS):
                d_p = mbe.make_projection_device(det.n_row, det.n_col)
                if k > 0:
                    mbe.copy_h2d(B.Projection(out[i].copy(), det.n_row, det.n_col), d_p)
                d_p.idx = i
                B.forward_project(mbe, v, k * dz, d_p, det, vg, accumulate=k > 0)
                out[i] = to_host(mbe, d_p)
                mbe.free(d_p)
            mbe.free(v)
    return out


def test_cpp_mirror_reprojects_like_the_python_mirror(tmp_path, oracle):
    demo = [DEMO] + [str(v) for v in DEMO_GEO] + [str(DEMO_VIEWS), "lcg", str(tmp_path / "vol.raw")]
    shape = (DEMO_VIEWS, DEMO_GEO[1], DEMO_GEO[0])
    for slabs in (1, 3):
        path = tmp_path / ("reprojected%d.raw" % slabs)
        r = subprocess.run(demo + ["--slabs", str(slabs), "--reproject", str(path)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr + r.stdout
        got = np.fromfile(path, np.float32).reshape(shape)
        want = python_reprojection(oracle, slabs)
        assert np.abs(want).max() > 0 and np.array_equal(bits(got), bits(want)), slabs
    r = subprocess.run(demo + ["--reproject", str(tmp_path / "x.raw"), "--roi", "0", "8", "0", "8", "0", "8"], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode != 0 and "--reproject cannot be combined with --roi" in (r.stderr + r.stdout)
