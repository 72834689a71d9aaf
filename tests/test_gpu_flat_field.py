"""Dark / flat correction on the device (flat_field.hip, widen.hip CORRECT): the formula against float64 numpy for every stored type,
the fused upload against the raw upload + in-place pass bit for bit, the setting's lifecycle and refusals, the C++ mirror and the
driver against the Python mirror, and the quality of a reconstruction from detector counts."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import grid_cap_rule as G
import phantom
import test_gpu_paris_hip as P
from oracle import formats as F
from paris_amd import _lib
from paris_amd import backend as B

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEMO = os.path.join(ROOT, "paris_amd", "host", "demo", "paris_hip_demo")
GEO_KEYS = ("n_row", "n_col", "l_px_row", "l_px_col", "delta_s", "delta_t", "d_so", "d_od", "delta_phi")
DRV_GEO = (64, 48, 0.2, 0.25, 1.5, -0.75, 100, 200, 1.0)
QUALITY_TOL = 1e-3   # relative RMS of the corrected-count reconstruction against the exact line integrals


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def expected(i, d, f, t_min):
    """the contract in float64, rounded once: -ln(max((I - D) / (F - D), t_min)), 0 for a dead pixel"""
    i64 = np.asarray(i).astype(np.float32).astype(np.float64)
    d64 = np.zeros_like(i64) if d is None else np.asarray(d, np.float32).astype(np.float64)
    f64 = np.asarray(f, np.float32).astype(np.float64)
    num, den = i64 - d64, f64 - d64
    ok = np.isfinite(i64) & np.isfinite(d64) & np.isfinite(f64) & (den > 0)
    with np.errstate(all="ignore"):
        p = -np.log(np.maximum(num / den, np.float64(np.float32(t_min))))
    return np.where(ok, p, 0.0).astype(np.float32)


def ordered(a):
    """fp32 bits as integers ordered like the values (ulp distance = difference)"""
    b = np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64)
    return np.where(b < 0, -(b & 0x7FFFFFFF), b)


def assert_formula(got, want, what):
    ulps = np.abs(ordered(got) - ordered(want))
    off = int(np.count_nonzero(ulps))
    assert ulps.max() <= 1 and off <= 1e-6 * want.size, (what, off, int(ulps.max()))


def references(dim_y, dim_x, seed, top):
    """non-uniform dark and gain; a few dead pixels: flat == dark, flat < dark, NaN / inf references"""
    rng = np.random.default_rng(seed)
    dark = (0.02 * top * (1 + rng.random((dim_y, dim_x)))).astype(np.float32)
    flat = (dark + 0.8 * top * (0.6 + 0.5 * rng.random((dim_y, dim_x)))).astype(np.float32)
    flat[0, 0] = dark[0, 0]
    flat[0, 1] = dark[0, 1] - 1
    flat[1, 2] = np.nan
    dark[1, 3] = np.inf
    flat[1, 4] = np.inf
    dark[1, 5] = -np.inf
    return dark, flat


def counts(dtype, dark, flat, seed, t_min):
    """intensities of every regime: transmissions in (0, 1], below t_min, below the dark (T < 0), above the flat (T > 1)"""
    rng = np.random.default_rng(seed)
    top = {np.uint8: 255, np.uint16: 65535, np.uint32: 2 ** 32 - 1, np.float32: None}[dtype]
    d = np.nan_to_num(dark.astype(np.float64), posinf=0, neginf=0)
    f = np.nan_to_num(flat.astype(np.float64), posinf=1000, neginf=0)
    t = np.exp(-rng.random(dark.shape) * 6)
    kind = rng.integers(0, 8, dark.shape)
    t = np.where(kind == 0, t_min * rng.random(dark.shape), t)           # below t_min
    t = np.where(kind == 1, -rng.random(dark.shape), t)                  # below the dark
    t = np.where(kind == 2, 1 + 0.1 * rng.random(dark.shape), t)         # above the flat
    i = d + (f - d) * t
    if dtype == np.float32:
        h = i.astype(np.float32)
        h.reshape(-1)[7:13] = [np.nan, np.inf, -np.inf, 0.0, -0.0, d.reshape(-1)[12]]
        return h
    h = np.clip(np.rint(i), 0, top)
    h.reshape(-1)[7:10] = [0, top, 1]
    return h.astype(dtype)


@pytest.fixture(scope="module")
def be():
    with B.Backend(0) as b:
        yield b


def read(be, d):
    h = be.make_projection_host(d.dim_x, d.dim_y)
    be.copy_d2h(d, h)
    return h.buf.copy()


def device_frame(be, dim_x, dim_y, tight):
    """a pool buffer (rows padded to 256 B), or wrapped caller memory with pitch 4 * dim_x; (projection, owner to free)"""
    if not tight:
        d = be.make_projection_device(dim_x, dim_y)
        return d, d
    v = be.make_volume_device(dim_x, dim_y, 1)
    return be.wrap_projection(v.ptr, 4 * dim_x, dim_x, dim_y), v


# ---- 1. the formula ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.uint32, np.float32])
@pytest.mark.parametrize("shape", [(40, 128), (37, 100)])
@pytest.mark.parametrize("with_dark", [True, False])
def test_formula_for_every_stored_type(be, dtype, shape, with_dark):
    dim_y, dim_x = shape
    top = {np.uint8: 255.0, np.uint16: 65535.0, np.uint32: 4e9, np.float32: 1e4}[dtype]
    dark, flat = references(dim_y, dim_x, dim_x, top)
    if not with_dark:
        dark = None
        flat = np.abs(flat)
    t_min = 1e-5 if dtype != np.uint8 else 0.01
    h = counts(dtype, np.zeros_like(flat) if dark is None else dark, flat, dim_y, t_min)
    want = expected(h, dark, flat, t_min)
    assert np.count_nonzero(want) > 0.9 * want.size and np.count_nonzero(want < 0) > 0
    assert np.count_nonzero(want == np.float32(-math.log(np.float32(t_min)))) > 0   # clamped pixels
    be.set_flat_field(dark, flat, t_min)
    try:
        for tight in (False, True):
            d, owner = device_frame(be, dim_x, dim_y, tight)
            be.upload_raw(h, d, corrected=True)
            fused = read(be, d)
            assert_formula(fused, want, ("fused", dtype, tight))
            be.upload_raw(h, d)
            be.flat_field_rows(d)
            in_place = read(be, d)
            assert np.array_equal(bits(in_place), bits(fused))
            be.free(owner)
    finally:
        be.clear_flat_field()


# ---- 2. fused upload == raw upload + in-place pass -------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.uint32, np.float32])
@pytest.mark.parametrize("dim_x", [256, 97, 24])
def test_fused_upload_equals_raw_upload_and_in_place_pass_on_row_bands(be, dtype, dim_x):
    """bands at odd offsets read the references of their ABSOLUTE rows; vector (256; 24 for u32 / f32) and scalar paths"""
    dim_y = 29
    top = {np.uint8: 255.0, np.uint16: 65535.0, np.uint32: 4e9, np.float32: 1e4}[dtype]
    dark, flat = references(dim_y, dim_x, 3, top)
    full = counts(dtype, dark, flat, 4, 1e-5)
    be.set_flat_field(dark, flat, 1e-5)
    try:
        for tight in (False, True):
            for r0, n in ((0, dim_y), (5, 13), (17, 12), (28, 1)):
                a, oa = device_frame(be, dim_x, dim_y, tight)
                b, ob = device_frame(be, dim_x, dim_y, tight)
                be.upload_raw(full[r0:r0 + n], a, row_first=r0, corrected=True)
                be.upload_raw(full[r0:r0 + n], b, row_first=r0)
                be.flat_field_rows(b, row_first=r0, row_count=n)
                ga, gb = read(be, a)[r0:r0 + n], read(be, b)[r0:r0 + n]
                assert np.array_equal(bits(ga), bits(gb)), (tight, r0, n)
                assert_formula(ga, expected(full[r0:r0 + n], dark[r0:r0 + n], flat[r0:r0 + n], 1e-5), (tight, r0))
                be.free(oa)
                be.free(ob)
    finally:
        be.clear_flat_field()


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.uint32, np.float32])
@pytest.mark.parametrize("dim_x", G.WIDEN_DIM_XS)
def test_fused_upload_of_more_rows_than_the_widening_grid_has_blocks(be, dtype, dim_x):
    """4100 rows from detector row 3 on against WIDEN_MAX_BLOCKS = 2048: every block comes round for a second row, four of them for a
    third, and reads the references of that row. 5 pixels a row: one per lane; 8: whole 16-byte vectors. The contract in float64
    rounded once, bit for bit (as tests/test_gpu_binning.py holds its chain: on these seeded pixels the device's double logarithm
    rounds to the fp32 value numpy's does); the in-place pass on a raw upload gives the same bits; rows 0 .. 2 and the padding of every row are not written"""
    r0, n = 3, G.WIDEN_ROWS
    dim_y = n + r0
    top = {np.uint8: 255.0, np.uint16: 65535.0, np.uint32: 4e9, np.float32: 1e4}[dtype]
    rng = np.random.default_rng(dim_x)
    dark = (0.02 * top * (1 + rng.random((dim_y, dim_x)))).astype(np.float32)
    flat = (dark + 0.8 * top * (0.6 + 0.5 * rng.random((dim_y, dim_x)))).astype(np.float32)
    flat[dim_y - 1, dim_x - 1] = dark[dim_y - 1, dim_x - 1]          # a dead pixel at the very end: 0
    t_min = 1e-5 if dtype != np.uint8 else 0.01
    full = counts(dtype, dark, flat, 4, t_min)
    want = expected(full[r0:], dark[r0:], flat[r0:], t_min)
    assert want[-1, -1] == 0 and np.count_nonzero(want) > 0.9 * want.size
    sentinel = np.uint32(0x7FC0BEEF)
    be.set_flat_field(dark, flat, t_min)
    try:
        a, b = be.make_projection_device(dim_x, dim_y), be.make_projection_device(dim_x, dim_y)
        wide = B.Projection(a.ptr, a.pitch // 4, dim_y, pitch=a.pitch, on_device=True)
        assert a.pitch > 4 * dim_x
        be.copy_h2d(B.Projection(np.full((dim_y, a.pitch // 4), sentinel, np.uint32).view(np.float32), a.pitch // 4, dim_y), wide)
        be.upload_raw(full[r0:], a, row_first=r0, corrected=True)
        be.upload_raw(full[r0:], b, row_first=r0)
        be.flat_field_rows(b, row_first=r0, row_count=n)
        h = be.make_projection_host(a.pitch // 4, dim_y)
        be.copy_d2h(wide, h)
        got = bits(h.buf)
        assert np.array_equal(got[r0:, :dim_x], bits(want))
        assert np.array_equal(bits(read(be, b)[r0:]), got[r0:, :dim_x])
        assert np.all(got[:r0] == sentinel) and np.all(got[:, dim_x:] == sentinel)
        be.free(a)
        be.free(b)
    finally:
        be.clear_flat_field()


def test_batched_frames_with_a_frame_stride(be):
    dim_x, dim_y, n = 96, 20, 5
    dark, flat = references(dim_y, dim_x, 8, 65535.0)
    frames = np.stack([counts(np.uint16, dark, flat, 10 + k, 1e-5) for k in range(n)])
    be.set_flat_field(dark, flat, 1e-5)
    try:
        d = be.make_projection_device(dim_x, n * dim_y)
        stride = d.pitch * dim_y
        first = B.Projection(d.ptr, dim_x, dim_y, pitch=d.pitch, on_device=True)
        for k in range(n):
            be.upload_raw(frames[k], be.wrap_projection(d.ptr + k * stride, d.pitch, dim_x, dim_y))
        be.flat_field_rows(first, row_first=3, row_count=11, frame_stride=stride, n_frames=n)
        got = read(be, d).reshape(n, dim_y, dim_x)
        for k in range(n):
            e = be.make_projection_device(dim_x, dim_y)
            be.upload_raw(frames[k][3:14], e, row_first=3, corrected=True)
            assert np.array_equal(bits(got[k, 3:14]), bits(read(be, e)[3:14])), k
            assert np.array_equal(bits(got[k, :3]), bits(frames[k][:3].astype(np.float32)))   # rows outside the band untouched
            assert np.array_equal(bits(got[k, 14:]), bits(frames[k][14:].astype(np.float32)))
            be.free(e)
        be.free(d)
    finally:
        be.clear_flat_field()


# ---- 3. the setting's lifecycle ------------------------------------------------------------------------------------------------

def test_replacement_and_clear_respect_queued_work():
    dim = 1024
    dark_a, flat_a = references(dim, dim, 1, 65535.0)
    dark_b, flat_b = dark_a + 50, flat_a - 3000
    frames = [counts(np.uint16, dark_a, flat_a, 20 + k, 1e-5) for k in range(6)]
    with B.Backend(0, synchronous=False) as abe:
        abe.set_flat_field(dark_a, flat_a, 1e-5)
        ds = [abe.make_projection_device(dim, dim) for _ in frames]
        for h, d in zip(frames, ds):
            abe.upload_raw(h, d, corrected=True)
        abe.set_flat_field(dark_b, flat_b, 1e-4)   # the six uploads above may still be queued: they keep the old frames
        e = abe.make_projection_device(dim, dim)
        abe.upload_raw(frames[0], e, corrected=True)
        abe.clear_flat_field()
        for h, d in zip(frames, ds):
            assert_formula(read(abe, d), expected(h, dark_a, flat_a, 1e-5), "before the replacement")
        first = read(abe, ds[0])
        assert_formula(read(abe, e), expected(frames[0], dark_b, flat_b, 1e-4), "after the replacement")
        # cleared: the raw upload is today's again, the corrected one is refused
        abe.upload_raw(frames[1], e)
        assert np.array_equal(bits(read(abe, e)), bits(frames[1].astype(np.float32)))
        with pytest.raises(B.ParisHipError):
            abe.upload_raw(frames[1], e, corrected=True)
        # the references are never written: the same frame corrected again after many passes gives the same bits
        abe.set_flat_field(dark_a, flat_a, 1e-5)
        for h, d in zip(frames, ds):
            abe.upload_raw(h, d)
            abe.flat_field_rows(d)
            abe.flat_field_rows(d)
        abe.upload_raw(frames[0], e, corrected=True)
        assert np.array_equal(bits(read(abe, e)), bits(first))
        for d in ds + [e]:
            abe.free(d)


def test_refusals(be):
    L = _lib.load()
    dark, flat = references(16, 32, 2, 1000.0)
    d = be.make_projection_device(32, 16)
    h = np.zeros((16, 32), np.uint16)
    for call in (lambda: be.flat_field_rows(d), lambda: be.upload_raw(h, d, corrected=True)):
        with pytest.raises(B.ParisHipError) as e:   # no setting
            call()
        assert e.value.status == _lib.ERROR_INVALID_ARGUMENT
    for t in (0.0, -1e-5, 1.5, float("nan"), float("inf")):
        with pytest.raises(B.ParisHipError):
            be.set_flat_field(dark, flat, t)
    assert L.paris_hip_set_flat_field(be._ctx, None, None, 32, 16, C.c_float(1e-5)) == _lib.ERROR_INVALID_ARGUMENT
    assert L.paris_hip_set_flat_field(be._ctx, None, flat.ctypes.data, 0, 16, C.c_float(1e-5)) == _lib.ERROR_INVALID_ARGUMENT
    assert L.paris_hip_set_flat_field(be._ctx, None, flat.ctypes.data, 32, 0, C.c_float(1e-5)) == _lib.ERROR_INVALID_ARGUMENT
    be.set_flat_field(dark, flat, 1.0)
    try:
        other = be.make_projection_device(33, 16)
        with pytest.raises(B.ParisHipError):
            be.flat_field_rows(other)                                    # size mismatch
        with pytest.raises(B.ParisHipError):
            be.upload_raw(np.zeros((16, 33), np.uint16), other, corrected=True)
        with pytest.raises(B.ParisHipError):
            be.flat_field_rows(B.Projection(d.ptr, 32, 15, pitch=d.pitch, on_device=True))
        with pytest.raises(B.ParisHipError):
            be.flat_field_rows(d, row_first=10, row_count=7)             # band out of range
        with pytest.raises(B.ParisHipError):
            be.flat_field_rows(d, row_first=17, row_count=0)
        assert L.paris_hip_upload_projection_raw_corrected(be._ctx, d.ptr, d.pitch, h.ctypes.data, 64, 32, 16, 9, 8,
                                                           _lib.PIXEL_U16) == _lib.ERROR_INVALID_ARGUMENT
        assert L.paris_hip_flat_field_rows(be._ctx, d.ptr, d.pitch, d.pitch * 16 - 4, 2, 32, 16, 0, 16) == _lib.ERROR_INVALID_ARGUMENT
        be.free(other)
    finally:
        be.clear_flat_field()
    be.free(d)


# ---- 4 / 5. the C++ mirror and the driver against the Python mirror ----------------------------------------------------------

def mirror_volume(frames, dark, flat, t_min, scan=None):
    """PARIS's loop through the Python mirror: each count frame loaded as fp32 and corrected in place before the weight"""
    det = B.DetectorGeometry(*DRV_GEO)
    vg = B.calculate_volume_geometry(det)
    with B.Backend(0) as mbe:
        mbe.set_flat_field(dark, flat, t_min)
        v = mbe.make_volume_device(vg.dim_x, vg.dim_y, vg.dim_z)
        for i, fr in enumerate(frames):
            d_p = B.load(mbe, B.Projection(fr.astype(np.float32), DRV_GEO[0], DRV_GEO[1], idx=i))
            mbe.flat_field_rows(d_p)
            if scan is not None:
                B.stage_short_scan_weight(mbe, d_p, det, scan)
            B.weight(mbe, d_p, det)
            B.filter(mbe, d_p, det)
            B.backproject(mbe, d_p, v, 0, det, vg, False, False, None)
            mbe.free(d_p)
        h = mbe.make_volume_host(vg.dim_x, vg.dim_y, vg.dim_z)
        mbe.copy_d2h(v, h)
    return h.buf.reshape(vg.dim_z, vg.dim_y, vg.dim_x).copy()


def mean(frames):
    acc = np.zeros(frames.shape[1:], np.float64)
    for f in frames:
        acc += f.astype(np.float32).astype(np.float64)
    return (acc / len(frames)).astype(np.float32)


def driver_set(tmp_path, n_frames):
    rng = np.random.default_rng(5)
    shape = (DRV_GEO[1], DRV_GEO[0])
    darks = rng.integers(150, 450, (3,) + shape).astype(np.uint16)
    flats = (rng.integers(30000, 60000, shape)[None] + rng.integers(-400, 400, (5,) + shape)).astype(np.uint16)
    darks[:, 0, 0] = flats[:, 0, 0] = 300    # a dead pixel: the mean flat equals the mean dark
    d, f = mean(darks), mean(flats)
    t = np.exp(-3 * rng.random((n_frames,) + shape))
    fr = np.clip(np.rint(d + (f - d) * t + rng.normal(0, 30, t.shape)), 0, 65535).astype(np.uint16)
    fr[:, 5, 5] = 0                          # below the dark: clamped to t_min
    ref = tmp_path / "ref"
    ref.mkdir()
    (ref / "dark.his").write_bytes(F.his_file_bytes(darks, 4, 32))
    (ref / "flat.his").write_bytes(F.his_file_bytes(flats, 4))
    counts_dir = tmp_path / "counts"
    counts_dir.mkdir()
    (counts_dir / "a.his").write_bytes(F.his_file_bytes(fr[:70], 4, 32))
    (counts_dir / "b.his").write_bytes(F.his_file_bytes(fr[70:], 4, 32))
    geo = tmp_path / "geo.ini"
    geo.write_text("\n".join("%s = %s" % kv for kv in zip(GEO_KEYS, DRV_GEO)) + "\n")
    return geo, ref, counts_dir, fr, d, f


def corrected_on_device(fr, d, f, t_min):
    with B.Backend(0) as cbe:
        cbe.set_flat_field(d, f, t_min)
        out = []
        for h in fr:
            p = cbe.make_projection_device(DRV_GEO[0], DRV_GEO[1])
            cbe.upload_raw(h, p)
            cbe.flat_field_rows(p)
            out.append(read(cbe, p))
            cbe.free(p)
    return np.stack(out)


def test_driver_and_cpp_mirror_against_the_python_mirror(tmp_path):
    det = B.DetectorGeometry(*DRV_GEO)
    g = max(abs(math.atan(((k + 0.5) * 0.2 - 6.4 - 1.5 * 0.2) / 300)) for k in (0, 63))
    n_frames = int(math.ceil(180 + 2 * math.degrees(g))) + 2
    geo, ref, counts_dir, fr, d, f = driver_set(tmp_path, n_frames)
    lines = corrected_on_device(fr, d, f, 1e-5)
    li_dir = tmp_path / "lines"
    li_dir.mkdir()
    (li_dir / "a.his").write_bytes(F.his_file_bytes(lines, 128))
    flat_args = ["--flat", ref / "flat.his", "--dark", ref / "dark.his"]
    want = mirror_volume(fr, d, f, 1e-5)
    assert np.abs(want).max() > 0
    env3 = dict(os.environ, PARIS_HIP_VIRTUAL_DEVICES="3")
    for k, (extra, env) in enumerate(((["--slabs", 1], None), (["--slabs", 3], env3), (["--slabs", 3, "--batch", 1], env3),
                                      (["--short-scan", "--slabs", 2], None))):
        outs, h2d = [], []
        for name, src, more in (("c", counts_dir, flat_args), ("l", li_dir, [])):
            o = tmp_path / ("%s%d" % (name, k))
            args = [P.EXE, "--geometry", geo, "--input", src, "--output", o] + more + extra
            r = subprocess.run([str(a) for a in args], capture_output=True, text=True, timeout=300, env=env)
            assert r.returncode == 0, r.stdout + r.stderr
            assert ("dark / flat correction on: 5 flat frame(s), 3 dark frame(s)" in r.stdout) == (name == "c"), r.stdout
            h2d.append(sum(int(l.split(":")[1].split()[0]) for l in r.stdout.splitlines() if l.startswith("  H2D of device")))
            outs.append(F.ddbvf_read(str(o / "vol.ddbvf"))[1])
        assert np.array_equal(bits(outs[0]), bits(outs[1])), extra
        assert 0 < 2 * h2d[0] == h2d[1], h2d   # the same bands: 2 B per pixel of u16 counts against 4 of f32 line integrals
        if k < 3:
            assert np.array_equal(bits(outs[0]), bits(want)), extra
    # PARIS's loop through paris::hip with set_flat_field (paris_hip_demo --flat): by-reference deferral, the second stream
    raw = tmp_path / "in.raw"
    fr.astype(np.float32).tofile(raw)
    d.tofile(tmp_path / "dark.raw")
    f.tofile(tmp_path / "flat.raw")
    out = tmp_path / "demo.raw"
    r = subprocess.run([DEMO] + [str(v) for v in DRV_GEO] + [str(n_frames), str(raw), str(out), "--slabs", "2", "--flat",
                                                          str(tmp_path / "dark.raw"), str(tmp_path / "flat.raw"), "1e-05"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr + r.stdout
    got = np.fromfile(out, np.float32).reshape(want.shape)
    assert np.array_equal(bits(got), bits(want))


# ---- 6. quality --------------------------------------------------------------------------------------------------------------

def test_quality_of_a_reconstruction_from_counts():
    n, step = 128, 2.0
    det = B.DetectorGeometry(n, n, 0.8, 0.8, 0.0, 0.0, 500, 500, step)
    vg = B.calculate_volume_geometry(det)
    radius = 0.9 * vg.dim_x * vg.l_vx_x / 2
    idxs = range(int(360 / step))
    lines = [phantom.projection(n, n, 0.8, 0.8, 500, 500, float(np.float32(i) * np.float32(step)), radius) for i in idxs]
    mu = 2.5 / max(float(p.max()) for p in lines)   # attenuation scale: at most 2.5 (8 % transmission)
    lines = [(mu * p).astype(np.float32) for p in lines]
    rng = np.random.default_rng(3)
    dark = (100 + 200 * rng.random((n, n))).astype(np.float32)
    flat = (dark + 60000 * (0.85 + 0.15 * rng.random((n, n)))).astype(np.float32)   # per-pixel gain spread
    cnt = [np.clip(np.rint(dark + (flat - dark) * np.exp(-p.astype(np.float64))), 0, 65535).astype(np.uint16) for p in lines]

    def reconstruct(frames, corrected):
        with B.Backend(0, synchronous=False) as qbe:
            qbe.set_paris_loop_defaults(48)
            if corrected:
                qbe.set_flat_field(dark, flat)
            v = qbe.make_volume_device(vg.dim_x, vg.dim_y, vg.dim_z)
            for i, fr in zip(idxs, frames):
                d_p = qbe.make_projection_device(n, n)
                qbe.upload_raw(fr, d_p, corrected=corrected)
                d_p.idx = i
                B.weight(qbe, d_p, det)
                B.filter(qbe, d_p, det)
                B.backproject(qbe, d_p, v, 0, det, vg, False, False, None)
                qbe.free(d_p)
            qbe.flush()
            h = qbe.make_volume_host(vg.dim_x, vg.dim_y, vg.dim_z)
            qbe.copy_d2h(v, h)
            qbe.free(v)
        return h.buf.reshape(vg.dim_z, vg.dim_y, vg.dim_x).astype(np.float64)

    exact = reconstruct(lines, False)
    got = reconstruct(cnt, True)
    raw = reconstruct(cnt, False)
    scale = np.sqrt((exact ** 2).mean())
    err = float(np.sqrt(((got - exact) ** 2).mean()) / scale)
    err_raw = float(np.sqrt(((raw - exact) ** 2).mean()) / scale)
    print("flat field quality: relative RMS %.3g from corrected u16 counts, %.3g from the uncorrected counts" % (err, err_raw))
    assert err <= QUALITY_TOL
    assert err_raw > 1e3 * err
