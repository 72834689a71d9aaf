"""Repair of defective detector pixels on the device (paris_hip_set_defect_map / paris_hip_defect_repair_rows):
the repaired values against float64, what must stay untouched, bands and batches, the ordering rules, the setting's lifecycle, the
flat field's dead pixels, paris.hip and the C++ mirror against the Python mirror, and the quality of a reconstruction."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import defect_rule as R
import test_gpu_flat_field as FF
import test_gpu_paris_hip as P
from oracle import formats as F
from paris_amd import _lib
from paris_amd import backend as B

pytestmark = pytest.mark.gpu

NAN_PAYLOAD = 0x7fc12345
ORD_GEO = (96, 80, 0.2, 0.25, 1.5, -0.75, 100, 200, 45.0)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def be():
    with B.Backend(0) as b:
        yield b


def read(be, d):
    h = be.make_projection_host(d.dim_x, d.dim_y)
    be.copy_d2h(d, h)
    return h.buf.copy()


def case(dim_x):
    """(mask, plan, frame): defective pixels hold NaN -- one used as a source would poison its defect -- and a few good pixels no
    defect uses as a source hold a NaN with a payload, as do the unrepairable pixels"""
    mask = R.shared_mask(dim_x, 80)
    plan = B.defect_plan(mask)
    rng = np.random.default_rng(dim_x)
    frame = (rng.random(mask.shape) * 4 - 0.5).astype(np.float32)
    frame[mask != 0] = np.nan
    unused = np.setdiff1d(np.flatnonzero(mask.reshape(-1) == 0), plan.source)
    payload = unused[[0, len(unused) // 3, len(unused) // 2, len(unused) - 1]]
    bits(frame).reshape(-1)[payload] = NAN_PAYLOAD
    lost = np.setdiff1d(np.flatnonzero(mask.reshape(-1)), plan.defect)
    bits(frame).reshape(-1)[lost] = NAN_PAYLOAD + 1 + np.arange(len(lost), dtype=np.uint32)
    return mask, plan, frame


CASES = {dim_x: case(dim_x) for dim_x in (96, 100)}


def assert_repaired(got, frame, plan, rows=None, what=""):
    """every repairable defect (of the rows given) within the fmaf chain's bound of the float64 sum of the plan's fp32 weights times the
    frame's pixels, (n + 1) 2^-24 sum w |p|; every other pixel keeps its bits"""
    want, mag, cnt = R.repair64(np.where(np.isnan(frame), 0.0, frame), plan.defect, plan.first_source, plan.source, plan.weight)
    dim_x = frame.shape[1]
    sel = np.ones(len(plan.defect), bool) if rows is None else (plan.defect // dim_x >= rows[0]) & (plan.defect // dim_x < rows[1])
    q = plan.defect[sel]
    err = np.abs(got.reshape(-1)[q].astype(np.float64) - want.reshape(-1)[q])
    bound = (cnt[sel] + 1) * 2.0 ** -24 * mag[sel]
    assert np.all(np.isfinite(got.reshape(-1)[q])), what
    assert np.all(err <= bound), (what, float((err / bound).max()))
    keep = np.ones(frame.size, bool)
    keep[q] = False
    assert np.array_equal(bits(got).reshape(-1)[keep], bits(frame).reshape(-1)[keep]), what
    return int(sel.sum())


# ---- 1. the repaired values -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim_x", [96, 100])
@pytest.mark.parametrize("tight", [False, True])
def test_repair_against_float64_and_what_stays_untouched(be, dim_x, tight):
    mask, plan, frame = CASES[dim_x]
    info = be.set_defect_map(mask)
    try:
        assert (info.defects, info.unrepairable, info.sources) == (plan.defects, plan.unrepairable, plan.sources)
        assert (info.reach_rows, info.reach_cols, info.device_bytes) == (plan.reach_rows, plan.reach_cols, plan.device_bytes)
        assert info.unrepairable == 9
        d, owner = FF.device_frame(be, dim_x, 80, tight)
        assert (d.pitch > 4 * dim_x) == (not tight)
        be.upload_raw(frame, d)
        assert np.array_equal(bits(read(be, d)), bits(frame))
        be.defect_repair_rows(d)
        once = read(be, d)
        assert assert_repaired(once, frame, plan, what=(dim_x, tight)) == len(plan.defect) > 400
        be.defect_repair_rows(d)   # sources are good pixels only: a second pass gives the same bits
        assert np.array_equal(bits(read(be, d)), bits(once))
        be.free(owner)
    finally:
        be.clear_defect_map()


def test_a_map_without_a_defect_is_a_no_op(be):
    frame = CASES[96][2]
    info = be.set_defect_map(np.zeros((80, 96), np.uint8))
    try:
        assert (info.defects, info.device_bytes) == (0, 0)
        d = be.make_projection_device(96, 80)
        be.upload_raw(frame, d)
        be.defect_repair_rows(d)
        assert np.array_equal(bits(read(be, d)), bits(frame))
        be.free(d)
    finally:
        be.clear_defect_map()


# ---- 2. bands and batches -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim_x", [96, 100])
def test_a_band_equals_the_same_rows_of_the_whole_frame(be, dim_x):
    mask, plan, frame = CASES[dim_x]
    first = plan.first_source[np.searchsorted(plan.defect, 16 * dim_x + 60)]
    assert plan.defect[np.searchsorted(plan.defect, 16 * dim_x + 60)] == 16 * dim_x + 60 and plan.source[first] // dim_x == 15
    be.set_defect_map(mask)
    try:
        whole, band = be.make_projection_device(dim_x, 80), be.make_projection_device(dim_x, 80)
        for d in (whole, band):
            be.upload_raw(frame, d)
        be.defect_repair_rows(whole)
        be.defect_repair_rows(band, row_first=16, row_count=32)
        w, b = read(be, whole), read(be, band)
        assert np.array_equal(bits(b[16:48]), bits(w[16:48]))
        assert np.array_equal(bits(b[:16]), bits(frame[:16])) and np.array_equal(bits(b[48:]), bits(frame[48:]))
        assert assert_repaired(b, frame, plan, rows=(16, 48)) > 100
        be.defect_repair_rows(band, row_first=79, row_count=1)   # the last row alone, then an empty band
        be.defect_repair_rows(band, row_first=80, row_count=0)
        assert np.array_equal(bits(read(be, band)[79]), bits(w[79]))
        be.free(whole)
        be.free(band)
    finally:
        be.clear_defect_map()


def test_three_frames_with_a_frame_stride_equal_three_single_calls(be):
    mask, plan, frame = CASES[100]
    rng = np.random.default_rng(9)
    frames = [np.where(np.isnan(frame), frame, (frame * rng.uniform(0.5, 2.0)).astype(np.float32)) for _ in range(3)]
    be.set_defect_map(mask)
    try:
        d = be.make_projection_device(100, 3 * 80)
        stride = d.pitch * 80
        views = [be.wrap_projection(d.ptr + k * stride, d.pitch, 100, 80) for k in range(3)]
        for h, v in zip(frames, views):
            be.upload_raw(h, v)
        be.defect_repair_rows(views[0], row_first=3, row_count=70, frame_stride=stride, n_frames=3)
        got = read(be, d).reshape(3, 80, 100)
        for k in range(3):
            e = be.make_projection_device(100, 80)
            be.upload_raw(frames[k], e)
            be.defect_repair_rows(e, row_first=3, row_count=70)
            assert np.array_equal(bits(got[k]), bits(read(be, e))), k
            assert assert_repaired(got[k], frames[k], plan, rows=(3, 73)) > 300
            be.free(e)
        be.free(d)
    finally:
        be.clear_defect_map()


# ---- 3. ordering (the three cases of tests/test_gpu_forward_project.py) ----------------------------------------------------------

def pending(be):
    n, ptr = C.c_uint32(0), C.c_void_p()
    assert be._L.paris_hip_pending_backprojections(be._ctx, C.byref(n), C.byref(ptr)) == 0
    return n.value


def ordering_frame():
    mask, plan, frame = CASES[96]
    return mask, np.where(np.isnan(frame), np.float32(1000.0), frame)   # finite garbage in the defects: the frame is backprojected


def test_a_held_back_weighting_is_flushed_first():
    det = B.DetectorGeometry(*ORD_GEO)
    mask, frame = ordering_frame()

    def run(fusion):
        with B.Backend(0, synchronous=False) as abe:
            abe.set_stage_fusion(fusion)
            abe.set_defect_map(mask)
            d_p = B.load(abe, B.Projection(frame.copy(), 96, 80, idx=2))
            B.weight(abe, d_p, det)            # with fusion: held back until something touches the frame
            abe.defect_repair_rows(d_p)
            return read(abe, d_p)

    plain, fused = run(False), run(True)
    assert not np.array_equal(bits(plain), bits(frame)) and np.array_equal(bits(fused), bits(plain))


def volume_to_host(abe, v, vg):
    h = abe.make_volume_host(vg.dim_x, vg.dim_y, vg.dim_z)
    abe.copy_d2h(v, h)
    return h.buf.copy()


@pytest.mark.parametrize("references", [False, True])
def test_a_frame_of_the_pending_group_is_backprojected_as_it_was(references):
    """by reference: the group that refers to the frame is launched before the repair writes it; snapshots: it stays pending"""
    det = B.DetectorGeometry(*ORD_GEO)
    vg = B.calculate_volume_geometry(det)
    mask, frame = ordering_frame()

    def run(deferred):
        with B.Backend(0, synchronous=False) as abe:
            if deferred:
                abe.set_backproject_deferral(8)
                abe.set_backproject_references(references)
            abe.set_defect_map(mask)
            v = abe.make_volume_device(vg.dim_x, vg.dim_y, vg.dim_z)
            d_p = B.load(abe, B.Projection(frame.copy(), 96, 80, idx=1))
            B.backproject(abe, d_p, v, 0, det, vg, False, False, None)
            if deferred:
                assert pending(abe) == 1
            abe.defect_repair_rows(d_p)
            if deferred:
                assert pending(abe) == (0 if references else 1)
            return read(abe, d_p), volume_to_host(abe, v, vg)

    want_p, want_v = run(False)
    got_p, got_v = run(True)
    assert np.abs(want_v).max() > 0 and not np.array_equal(bits(want_p), bits(frame))
    assert np.array_equal(bits(got_v), bits(want_v)) and np.array_equal(bits(got_p), bits(want_p))


# ---- 4. refusals and the setting's lifecycle ----------------------------------------------------------------------------------------

def test_refusals(be):
    L = _lib.load()
    mask = CASES[96][0]
    d = be.make_projection_device(96, 80)
    st = _lib.DefectStats()
    with pytest.raises(B.ParisHipError) as e:   # no setting
        be.defect_repair_rows(d)
    assert e.value.status == _lib.ERROR_INVALID_ARGUMENT
    assert L.paris_hip_defect_map_info(be._ctx, C.byref(st)) == _lib.ERROR_INVALID_ARGUMENT
    assert L.paris_hip_set_defect_map(be._ctx, None, 96, 80) == _lib.ERROR_INVALID_ARGUMENT
    assert L.paris_hip_set_defect_map(be._ctx, mask.ctypes.data, 0, 80) == _lib.ERROR_INVALID_ARGUMENT
    assert L.paris_hip_set_defect_map(be._ctx, mask.ctypes.data, 96, 0) == _lib.ERROR_INVALID_ARGUMENT
    be.clear_defect_map()                        # clearing nothing is fine
    be.set_defect_map(mask)
    try:
        other = be.make_projection_device(97, 80)
        with pytest.raises(B.ParisHipError):
            be.defect_repair_rows(other)                                                            # other dimensions
        with pytest.raises(B.ParisHipError):
            be.defect_repair_rows(B.Projection(d.ptr, 96, 79, pitch=d.pitch, on_device=True))
        with pytest.raises(B.ParisHipError):
            be.defect_repair_rows(B.Projection(d.ptr, 96, 80, pitch=4 * 96 - 4, on_device=True))    # a bad pitch
        with pytest.raises(B.ParisHipError):
            be.defect_repair_rows(B.Projection(d.ptr, 96, 80, pitch=d.pitch + 2, on_device=True))
        with pytest.raises(B.ParisHipError):
            be.defect_repair_rows(d, row_first=70, row_count=11)                                    # a bad band
        with pytest.raises(B.ParisHipError):
            be.defect_repair_rows(d, row_first=81, row_count=0)
        assert L.paris_hip_defect_repair_rows(be._ctx, d.ptr, d.pitch, d.pitch * 80 - 4, 2, 96, 80, 0, 80) == _lib.ERROR_INVALID_ARGUMENT
        assert L.paris_hip_defect_repair_rows(be._ctx, d.ptr, d.pitch, d.pitch * 80 + 2, 2, 96, 80, 0, 80) == _lib.ERROR_INVALID_ARGUMENT
        assert L.paris_hip_defect_repair_rows(be._ctx, None, d.pitch, 0, 1, 96, 80, 0, 80) == _lib.ERROR_INVALID_ARGUMENT
        be.free(other)
    finally:
        be.clear_defect_map()
    be.free(d)


def test_reserve_bytes_grow_by_the_plan_and_shrink_again(be):
    mask, plan, _ = CASES[96]
    before = be.projection_reserve_bytes(96, 80)
    info = be.set_defect_map(mask)
    assert info.device_bytes == 4 * (2 * len(plan.defect) + 1 + 2 * len(plan.source)) > 0
    assert be.projection_reserve_bytes(96, 80) == before + info.device_bytes
    small = be.set_defect_map(np.eye(80, 96, dtype=np.uint8))   # replaced: the new plan's bytes, not both
    assert be.projection_reserve_bytes(96, 80) == before + small.device_bytes != before + info.device_bytes
    be.clear_defect_map()
    assert be.projection_reserve_bytes(96, 80) == before


def test_replacement_and_clear_respect_queued_work():
    dim = 1024
    rng = np.random.default_rng(2)
    mask_a = (rng.random((dim, dim)) < 0.002).astype(np.uint8)
    mask_a[300, :] = 1
    mask_b = np.zeros_like(mask_a)
    mask_b[:, 500] = 1
    mask_b[10:14, 10:14] = 1
    plan_a, plan_b = B.defect_plan(mask_a), B.defect_plan(mask_b)
    frames = [(rng.random((dim, dim)) * 3).astype(np.float32) for _ in range(6)]
    with B.Backend(0, synchronous=False) as abe:
        abe.set_defect_map(mask_a)
        ds = [abe.make_projection_device(dim, dim) for _ in frames]
        for h, d in zip(frames, ds):
            abe.upload_raw(h, d)
            abe.defect_repair_rows(d)
        abe.set_defect_map(mask_b)   # the six repairs above may still be queued: they keep the old plan
        e = abe.make_projection_device(dim, dim)
        abe.upload_raw(frames[0], e)
        abe.defect_repair_rows(e)
        abe.clear_defect_map()
        for h, d in zip(frames, ds):
            assert_repaired(read(abe, d), h, plan_a, what="before the replacement")
        assert_repaired(read(abe, e), frames[0], plan_b, what="after the replacement")
        with pytest.raises(B.ParisHipError):   # cleared: the repair is refused
            abe.defect_repair_rows(e)
        for d in ds + [e]:
            abe.free(d)


# ---- 5. the flat field's dead pixels ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("with_dark", [True, False])
def test_flat_field_dead_pixels_follow_numpy_s_rule(be, with_dark):
    L = _lib.load()
    out = np.empty((40, 100), np.uint8)
    assert L.paris_hip_flat_field_dead_pixels(be._ctx, out.ctypes.data) == _lib.ERROR_INVALID_ARGUMENT   # no setting
    with pytest.raises(B.ParisHipError):
        be.flat_field_dead_pixels()
    rng = np.random.default_rng(4)
    dark = (100 + 50 * rng.random((40, 100))).astype(np.float32)
    flat = (dark + 1000 * rng.random((40, 100))).astype(np.float32)
    flat[3, 4], flat[3, 5], flat[3, 6] = np.nan, np.inf, -np.inf
    dark[7, 1], dark[7, 2], dark[7, 3] = np.nan, np.inf, -np.inf
    flat[9, 9] = dark[9, 9]            # F == D
    flat[9, 10] = dark[9, 10] - 1      # F < D
    flat[9, 11] = 0.0
    flat[20, 20], dark[20, 20] = np.inf, np.inf
    dk = dark if with_dark else None
    d64 = dark.astype(np.float64) if with_dark else np.zeros(flat.shape)
    with np.errstate(invalid="ignore"):
        want = ~np.isfinite(d64) | ~np.isfinite(flat) | ~(flat.astype(np.float64) - d64 > 0)
    assert np.count_nonzero(want) == (10 if with_dark else 5)
    be.set_flat_field(dk, flat)
    try:
        got = be.flat_field_dead_pixels()
        assert got.dtype == np.uint8 and set(np.unique(got)) == {0, 1} and np.array_equal(got != 0, want)
        assert L.paris_hip_flat_field_dead_pixels(be._ctx, None) == _lib.ERROR_INVALID_ARGUMENT
        # the device's correction agrees: those pixels, and no others, are 0 for a frame that is nowhere else dead
        d = be.make_projection_device(100, 40)
        be.upload_raw(np.full((40, 100), 60.0, np.float32), d, corrected=True)
        assert np.array_equal(read(be, d) == 0, want)
        be.free(d)
    finally:
        be.clear_flat_field()
    with pytest.raises(B.ParisHipError):
        be.flat_field_dead_pixels()


# ---- 6. the driver and the C++ mirror against the Python mirror ------------------------------------------------------------------

def mirror_volume(frames, dark, flat, t_min, mask):
    """PARIS's loop through the Python mirror: correct -> repair -> weight -> filter -> backproject"""
    det = B.DetectorGeometry(*FF.DRV_GEO)
    vg = B.calculate_volume_geometry(det)
    with B.Backend(0) as mbe:
        mbe.set_flat_field(dark, flat, t_min)
        mbe.set_defect_map(mask)
        v = mbe.make_volume_device(vg.dim_x, vg.dim_y, vg.dim_z)
        for i, fr in enumerate(frames):
            d_p = B.load(mbe, B.Projection(fr.astype(np.float32), FF.DRV_GEO[0], FF.DRV_GEO[1], idx=i))
            mbe.flat_field_rows(d_p)
            mbe.defect_repair_rows(d_p)
            B.weight(mbe, d_p, det)
            B.filter(mbe, d_p, det)
            B.backproject(mbe, d_p, v, 0, det, vg, False, False, None)
            mbe.free(d_p)
        h = mbe.make_volume_host(vg.dim_x, vg.dim_y, vg.dim_z)
        mbe.copy_d2h(v, h)
    return h.buf.reshape(vg.dim_z, vg.dim_y, vg.dim_x).copy()


def test_driver_and_cpp_mirror_against_the_python_mirror(tmp_path):
    det = B.DetectorGeometry(*FF.DRV_GEO)
    vg = B.calculate_volume_geometry(det)
    n_row, n_col = FF.DRV_GEO[:2]
    n_frames = 75
    geo, ref, counts_dir, fr, d, f = FF.driver_set(tmp_path, n_frames)
    # the detector rows each of three slabs reads: defects sit on the band edges, so their sources lie outside the band
    dz = vg.dim_z // 3
    bands = [B.slab_row_band(det, vg, vg.dim_x, vg.dim_y, dz + (vg.dim_z % 3 if k == 2 else 0), k * dz) for k in range(3)]
    assert all(0 < b[0] or b[0] + b[1] < n_col for b in bands)
    mask = np.zeros((n_col, n_row), np.uint8)
    mask[:, 33] = 1                                   # a dead column: crosses every band edge
    mask[bands[1][0], 10:14] = 1                      # on the first row of the middle slab's band
    mask[bands[1][0] + bands[1][1] - 1, 20] = 1       # on its last row
    mask[bands[2][0], :20] = 1                        # a run on the first row of the last slab's band
    mask[bands[0][0] + bands[0][1] - 3:bands[0][0] + bands[0][1], 50:53] = 1   # a 3 x 3 block against the first slab's last row
    (tmp_path / "mask.raw").write_bytes(mask.tobytes())
    full = mask.copy()
    full[0, 0] = 1                                    # the flat field's dead pixel (driver_set): --defects-from-flat adds it
    n_def = int(np.count_nonzero(full))
    want = mirror_volume(fr, d, f, 1e-5, full)
    unrepaired = FF.mirror_volume(fr, d, f, 1e-5)
    assert np.abs(want).max() > 0 and not np.array_equal(bits(want), bits(unrepaired))
    base = [P.EXE, "--geometry", geo, "--input", counts_dir, "--flat", ref / "flat.his", "--dark", ref / "dark.his"]
    repair = ["--defects", tmp_path / "mask.raw", "--defects-from-flat"]
    for k, extra in enumerate((["--slabs", 1], ["--slabs", 3], ["--slabs", 3, "--batch", 1])):
        o = tmp_path / ("o%d" % k)
        r = subprocess.run([str(a) for a in base + ["--output", o] + repair + extra], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "defect map on: %d defective pixel(s), 0 unrepairable" % n_def in r.stdout, r.stdout
        assert np.array_equal(bits(F.ddbvf_read(str(o / "vol.ddbvf"))[1]), bits(want)), extra
    # refused before any device work: a map of another size, --defects-from-flat without --flat
    (tmp_path / "short.raw").write_bytes(mask.tobytes()[:-1])
    (tmp_path / "long.raw").write_bytes(mask.tobytes() + b"\0")
    for bad in ("short.raw", "long.raw"):
        r = subprocess.run([str(a) for a in base + ["--output", tmp_path / "bad", "--defects", tmp_path / bad]], capture_output=True,
                           text=True, timeout=300)
        assert r.returncode == 1 and "--defects" in r.stderr and "pixels" in r.stderr, r.stderr
    r = subprocess.run([str(a) for a in base[:5] + ["--output", tmp_path / "bad", "--defects-from-flat"]], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 1 and "--defects-from-flat needs --flat" in r.stderr, r.stderr
    assert not (tmp_path / "bad").exists()
    # PARIS's loop through paris::hip with set_flat_field and set_defect_map (paris_hip_demo --flat --defects)
    raw = tmp_path / "in.raw"
    fr.astype(np.float32).tofile(raw)
    d.tofile(tmp_path / "dark.raw")
    f.tofile(tmp_path / "flat.raw")
    (tmp_path / "full.raw").write_bytes(full.tobytes())
    out = tmp_path / "demo.raw"
    r = subprocess.run([FF.DEMO] + [str(v) for v in FF.DRV_GEO] + [str(n_frames), str(raw), str(out), "--slabs", "2", "--flat",
                                                                str(tmp_path / "dark.raw"), str(tmp_path / "flat.raw"), "1e-05",
                                                                "--defects", str(tmp_path / "full.raw")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr + r.stdout
    assert np.array_equal(bits(np.fromfile(out, np.float32).reshape(want.shape)), bits(want))


# ---- 7. quality -------------------------------------------------------------------------------------------------------------------

def test_quality_of_a_reconstruction_with_repaired_pixels():
    """Relative RMS against the reconstruction from clean frames, 64 x 48 driver geometry, 130 dead pixels (a row, a column, a cluster,
    0.5 % scattered). The oracle with the float64 repair (tests/test_defect_map_host.py): 0.4305 with the dead pixels left at 0,
    0.05021 repaired; the device differs from it only by the filter's FFT rounding."""
    det = B.DetectorGeometry(*R.QUALITY_GEO)
    vg = B.calculate_volume_geometry(det)
    lines = R.quality_frames(vg.dim_x, vg.l_vx_x)
    mask = R.quality_mask()
    zeroed = [np.where(mask != 0, np.float32(0), p) for p in lines]

    def reconstruct(frames, repair):
        with B.Backend(0, synchronous=False) as qbe:
            qbe.set_paris_loop_defaults(48)
            if repair:
                qbe.set_defect_map(mask)
            v = qbe.make_volume_device(vg.dim_x, vg.dim_y, vg.dim_z)
            for i, fr in enumerate(frames):
                d_p = qbe.make_projection_device(det.n_row, det.n_col)
                qbe.upload_raw(fr, d_p)
                d_p.idx = i
                if repair:
                    qbe.defect_repair_rows(d_p)
                B.weight(qbe, d_p, det)
                B.filter(qbe, d_p, det)
                B.backproject(qbe, d_p, v, 0, det, vg, False, False, None)
                qbe.free(d_p)
            qbe.flush()
            return volume_to_host(qbe, v, vg)

    clean = reconstruct(lines, False)
    a = R.relative_rms(reconstruct(zeroed, False), clean)
    b = R.relative_rms(reconstruct(zeroed, True), clean)
    print("defect map quality: relative RMS %.4g with the dead pixels at 0, %.4g repaired" % (a, b))
    assert b <= R.BOUND * R.CAL_REPAIRED
    assert b < a
