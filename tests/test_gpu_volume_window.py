"""Volume export on the device: voxels quantised to 8 / 16 bits over a grey window, the statistics a window
is chosen from, and paris.hip's --voxel-type / --voxel-range -- all against the numpy rule of tests/volume_window_rule.py, bit for
bit and count for count."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import test_gpu_flat_field as FF
import test_gpu_parity as PAR
import test_gpu_paris_hip as P
import volume_window_rule as R
from oracle import formats as F
from paris_amd import _lib
from paris_amd import backend as B

pytestmark = pytest.mark.gpu

INVALID = _lib.ERROR_INVALID_ARGUMENT
DTYPES = [np.uint8, np.uint16]
VOXEL_TYPE = {np.uint8: _lib.VOXEL_U8, np.uint16: _lib.VOXEL_U16}
# one pass of the quantise kernel's capped grid covers 1024 blocks x 256 lanes x 16 bytes of output: 4 Mi voxels as u8, 2 Mi as u16
BEYOND_ONE_PASS = 1024 * 256 * 16 + 4099


@pytest.fixture(scope="module")
def be():
    b = B.set_device(B.get_devices()[0])
    yield b
    b.close()


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def on_device(torch, v, offset=0):
    """the floats v on the device, `offset` floats behind a 16-byte boundary; (keep-alive, Volume)"""
    t = torch.zeros(v.size + 8, dtype=torch.float32, device="cuda")
    assert t.data_ptr() % 16 == 0
    t[offset:offset + v.size].copy_(torch.from_numpy(np.ascontiguousarray(v)))
    torch.cuda.synchronize()
    return t, B.Volume(t.data_ptr() + 4 * offset, v.size, 1, 1, on_device=True)


def mixed_volume(n, seed=11):
    """seeded normal voxels that reach beyond [0, 1] on both sides, with the special values among them"""
    v = R.normal_volume(n, seed)
    s = R.specials(0.0, 1.0)
    if n >= 4 * s.size:
        v[::max(1, n // s.size)][:s.size] = s
    return v


def quantize_d2d(be, torch, src, n, lo, hi, dtype, dst_offset=0, guard=64):
    """paris_hip_volume_quantize into a byte buffer whose first voxel lies dst_offset ELEMENTS behind a 16-byte boundary; returns
    (status, voxels, the bytes before, the bytes behind)"""
    elem = np.dtype(dtype).itemsize
    buf = torch.full((guard + dst_offset * elem + n * elem + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0 and guard % 16 == 0
    torch.cuda.synchronize()
    w = _lib.VolumeWindow(lo, hi, VOXEL_TYPE[dtype])
    first = guard + dst_offset * elem
    rc = be._L.paris_hip_volume_quantize(be._ctx, src.ptr, n, C.byref(w), buf.data_ptr() + first)
    be.synchronize()
    host = buf.cpu().numpy()
    return rc, host[first:first + n * elem].view(dtype), host[:first], host[first + n * elem:]


# ---- 1. quantise ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [1, 3, 15, 16, 17, 255, 4099, 67 * 33 * 5, BEYOND_ONE_PASS])
def test_quantize_bit_for_bit(be, torch, dtype, n):
    v = mixed_volume(n)
    keep, d_v = on_device(torch, v)
    got = be.quantize_volume(d_v, 0.0, 1.0, dtype)
    assert got.dtype == dtype and got.shape == (1, 1, n)
    want = R.quantize(v, 0.0, 1.0, dtype)
    assert np.array_equal(got.ravel(), want), np.flatnonzero(got.ravel() != want)[:8]
    if n > 1000:   # the data does reach every case of the rule
        levels = R.LEVELS[np.dtype(dtype)]
        assert (want == 0).any() and (want == levels).any() and ((want > 0) & (want < levels)).any()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [255, 4099])
def test_quantize_alignments(be, torch, dtype, n):
    """Source and destination offset from 16-byte alignment, separately and together (single voxels: the scalar kernel), and offset so
    that both reach a boundary at the same voxel (vectors with a head of 3 voxels and a tail). Nothing outside the destination is
    written."""
    v = mixed_volume(n, seed=5)
    want = R.quantize(v, 0.0, 1.0, dtype)
    elem = np.dtype(dtype).itemsize
    for src_off, dst_off in ((0, 0), (1, 0), (0, 1), (1, 1), (1, 16 // elem - 3), (2, 16 // elem - 2), (3, 3)):
        keep, d_v = on_device(torch, v, src_off)
        rc, got, before, behind = quantize_d2d(be, torch, d_v, n, 0.0, 1.0, dtype, dst_off)
        assert rc == 0
        assert np.array_equal(got, want), (src_off, dst_off, np.flatnonzero(got != want)[:8])
        assert (before == 0xA5).all() and (behind == 0xA5).all(), (src_off, dst_off)


@pytest.mark.parametrize("dtype", DTYPES)
def test_quantize_special_values_and_window_ends(be, torch, dtype):
    levels = R.LEVELS[np.dtype(dtype)]
    for lo, hi in ((0.0, 1.0), (-3.5, 7.25), (1e-3, 1.001e-3), (-2e38, 3e38)):
        v = np.tile(R.specials(lo, hi), 3)
        keep, d_v = on_device(torch, v)
        got = be.quantize_volume(d_v, lo, hi, dtype).ravel()
        assert np.array_equal(got, R.quantize(v, lo, hi, dtype)), (lo, hi, got)
        nan, pinf, ninf, zero, nzero, at_lo, at_hi, lo_down, lo_up, hi_down, hi_up = got[:11]
        assert (nan, pinf, ninf, at_lo, lo_down, hi_up) == (0, levels, 0, 0, 0, levels) and zero == nzero


@pytest.mark.parametrize("dtype", DTYPES)
def test_quantize_ties_round_to_even(be, torch, dtype):
    """lo = 0 and hi = L / 2 make the scale exactly 2; v = (k + 0.5) / 2 is exact for every k, and x = k + 0.5 a tie"""
    levels = R.LEVELS[np.dtype(dtype)]
    assert R.scale(0.0, levels / 2, levels) == 2.0
    k = np.arange(levels, dtype=np.float64)
    v = ((k + 0.5) / 2).astype(np.float32)
    assert np.array_equal(v.astype(np.float64) * 2, k + 0.5)
    keep, d_v = on_device(torch, v)
    got = be.quantize_volume(d_v, 0.0, levels / 2, dtype).ravel().astype(np.int64)
    want = np.where(k % 2 == 0, k, k + 1).astype(np.int64)
    assert np.array_equal(got, want)
    assert np.array_equal(R.quantize(v, 0.0, levels / 2, dtype).astype(np.int64), want)


def test_counts_accumulate_reset_and_are_per_ctx(torch):
    a, b = mixed_volume(4099, seed=1), mixed_volume(70000, seed=2)
    with B.Backend(0) as one, B.Backend(0) as other:
        zero = one.volume_quantize_counts()
        assert (zero.voxels, zero.below, zero.above, zero.not_finite) == (0, 0, 0, 0)
        keep_a, d_a = on_device(torch, a)
        keep_b, d_b = on_device(torch, b, 1)
        one.quantize_volume(d_a, 0.0, 1.0, np.uint16)
        c = one.volume_quantize_counts()
        assert (c.voxels, c.below, c.above, c.not_finite) == R.counts(a, 0.0, 1.0) and c.below > 0 and c.above > 0 and c.not_finite == 3
        one.quantize_volume(d_b, 0.25, 0.5, np.uint8)
        c = one.volume_quantize_counts(reset=True)
        want = tuple(x + y for x, y in zip(R.counts(a, 0.0, 1.0), R.counts(b, 0.25, 0.5)))
        assert (c.voxels, c.below, c.above, c.not_finite) == want
        c = one.volume_quantize_counts()
        assert (c.voxels, c.below, c.above, c.not_finite) == (0, 0, 0, 0)
        one.quantize_volume(d_b, 0.25, 0.5, np.uint8)
        c = one.volume_quantize_counts()
        assert (c.voxels, c.below, c.above, c.not_finite) == R.counts(b, 0.25, 0.5)
        c = other.volume_quantize_counts()
        assert (c.voxels, c.below, c.above, c.not_finite) == (0, 0, 0, 0)


@pytest.mark.parametrize("dtype", DTYPES)
def test_device_to_device_and_d2h_forms_agree(be, torch, dtype):
    v = mixed_volume(67 * 33 * 5, seed=3)
    keep, d_v = on_device(torch, v)
    d2h = be.quantize_volume(d_v, 0.1, 0.9, dtype).ravel()
    rc, d2d, _, _ = quantize_d2d(be, torch, d_v, v.size, 0.1, 0.9, dtype)
    assert rc == 0 and d2h.tobytes() == d2d.tobytes()
    out = torch.zeros(v.size * np.dtype(dtype).itemsize, dtype=torch.uint8, device="cuda")   # the mirror's out= form
    torch.cuda.synchronize()
    assert be.quantize_volume(d_v, 0.1, 0.9, dtype, out=out.data_ptr()) == out.data_ptr()
    be.synchronize()
    assert out.cpu().numpy().tobytes() == d2h.tobytes()


def test_quantize_refusals(be, torch):
    v = mixed_volume(4099, seed=4)
    keep, d_v = on_device(torch, v)
    L, ctx = be._L, be._ctx
    ok = _lib.VolumeWindow(0.0, 1.0, _lib.VOXEL_U16)
    dst = torch.full((4 * v.size,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    before = be.volume_quantize_counts()
    # an overlapping destination: inside the source, and ending / starting one byte inside it
    for q in (d_v.ptr, d_v.ptr + 4 * v.size - 2, d_v.ptr - 2 * v.size + 2):
        assert L.paris_hip_volume_quantize(ctx, d_v.ptr, v.size, C.byref(ok), q) == INVALID
    assert L.paris_hip_volume_quantize(ctx, d_v.ptr, v.size // 2, C.byref(ok), d_v.ptr + 4 * (v.size // 2)) == 0   # adjacent is fine
    keep, d_v = on_device(torch, v)
    # n_voxels == 0 does nothing
    assert L.paris_hip_volume_quantize(ctx, d_v.ptr, 0, C.byref(ok), dst.data_ptr()) == 0
    assert L.paris_hip_volume_quantize_d2h(ctx, d_v.ptr, 0, C.byref(ok), dst.data_ptr()) == 0
    be.synchronize()
    assert (dst.cpu().numpy() == 0xA5).all()
    after = be.volume_quantize_counts()
    assert after.voxels == before.voxels + v.size // 2
    # null pointers, a refused setting, alignment
    assert L.paris_hip_volume_quantize(ctx, None, 8, C.byref(ok), dst.data_ptr()) == INVALID
    assert L.paris_hip_volume_quantize(ctx, d_v.ptr, 8, C.byref(ok), None) == INVALID
    assert L.paris_hip_volume_quantize(ctx, d_v.ptr, 8, None, dst.data_ptr()) == INVALID
    assert L.paris_hip_volume_quantize(None, d_v.ptr, 8, C.byref(ok), dst.data_ptr()) == INVALID
    for bad in (_lib.VolumeWindow(1.0, 1.0, _lib.VOXEL_U16), _lib.VolumeWindow(0.0, 1.0, 7), _lib.VolumeWindow(0.0, float("nan"), _lib.VOXEL_U8)):
        assert L.paris_hip_volume_quantize(ctx, d_v.ptr, 8, C.byref(bad), dst.data_ptr()) == INVALID
        assert L.paris_hip_volume_quantize_d2h(ctx, d_v.ptr, 8, C.byref(bad), dst.data_ptr()) == INVALID
    assert L.paris_hip_volume_quantize(ctx, d_v.ptr + 2, 8, C.byref(ok), dst.data_ptr()) == INVALID
    assert L.paris_hip_volume_quantize(ctx, d_v.ptr, 8, C.byref(ok), dst.data_ptr() + 1) == INVALID   # u16 on an odd address
    assert L.paris_hip_volume_quantize_counts(ctx, None, 0) == INVALID
    with pytest.raises(B.ParisHipError):
        be.quantize_volume(d_v, 1.0, 0.0, np.uint16)
    with pytest.raises(B.ParisHipError):
        be.quantize_volume(d_v, 0.0, 1.0, np.int16)
    be.synchronize()
    assert (dst.cpu().numpy() == 0xA5).all()


def test_quantizing_into_a_volume_marks_it_dirty(be, torch, oracle):
    """A fresh zero-filled volume may skip the tiles no ray reaches. Quantised voxels written into it are arbitrary bits -- here every
    word becomes the bit pattern of -0 -- so from then on it must take every addition: the result equals what
    paris_hip_set_backproject_skip_invalid(0) gives from the same bits, and no -0 is left. Geometry of
    test_gpu_parity.test_backproject_tiles_no_ray_reaches: most tiles lie outside the cone."""
    g = (64, 48, 0.4, 0.4, 1.5, -2.0, 200, 150, 23.0)
    det = B.DetectorGeometry(*g)
    nat = B.calculate_volume_geometry(det)
    dz, dy, dx = 96, 72, 192
    l_vx = float(nat.l_vx_x)
    vg = B.VolumeGeometry(dx, dy, dz, l_vx * 1.1, l_vx * 2.6, l_vx * 1.7)
    proj = oracle.lcg_projection(64, 48, 3) - np.float32(0.5)

    def add(d_v):
        d_p = PAR.to_device(be, proj, idx=3)
        B.backproject(be, d_p, d_v, 0, det, vg, False, False, None)
        be.free(d_p)
        return PAR.volume_to_host(be, d_v)

    n = dx * dy * dz
    pairs = np.zeros(2 * n, np.float32)
    pairs[1::2] = 32768.0   # u16 pairs (0, 0x8000): little-endian, the word 0x80000000
    keep, d_src = on_device(torch, pairs)
    be.set_backproject_skip_invalid(True)
    d_v = be.make_volume_device(dx, dy, dz)
    try:
        be.quantize_volume(d_src, 0.0, 65535.0, np.uint16, out=d_v)
        start = PAR.volume_to_host(be, d_v)
        assert (start.view(np.uint32) == 0x80000000).all()
        got = add(d_v)
        # the same bits in a volume that takes every addition: uploaded from the host, the skip switched off
        d_w = be.make_volume_device(dx, dy, dz)
        be.copy_h2d(B.Volume(start.copy(), dx, dy, dz), d_w)
        be.set_backproject_skip_invalid(False)
        want = add(d_w)
        be.free(d_w)
    finally:
        be.set_backproject_skip_invalid(True)
        be.free(d_v)
    PAR.assert_bit_equal(got, want)
    assert (want == 0).any() and not np.signbit(got[got == 0]).any()   # voxels outside the rays stay zero; every -0 became +0


def test_pending_projections_are_seen(torch, oracle):
    """with a deferral depth > 1 and projections pending into the volume, quantize_volume and volume_stats see the finished volume"""
    det = B.DetectorGeometry(*PAR.KAT)
    vg = B.calculate_volume_geometry(det)
    projs = [oracle.lcg_projection(64, 48, i) for i in range(3)]
    with B.Backend(0) as dbe:
        dbe.set_backproject_deferral(8)

        d_ps = [PAR.to_device(dbe, p, idx=i) for i, p in enumerate(projs)]   # (uploads and frees run what is pending: none in between)

        def pend(d_v):
            for d_p in d_ps:
                B.backproject(dbe, d_p, d_v, 0, det, vg, False, False, None)
            n, ptr = C.c_uint32(0), C.c_void_p()
            assert dbe._L.paris_hip_pending_backprojections(dbe._ctx, C.byref(n), C.byref(ptr)) == 0
            assert n.value == 3 and ptr.value == d_v.ptr

        d_v = dbe.make_volume_device(vg.dim_x, vg.dim_y, vg.dim_z)
        pend(d_v)
        q = dbe.quantize_volume(d_v, 0.0, 40.0, np.uint16)
        after_three = PAR.volume_to_host(dbe, d_v)
        assert np.abs(after_three).max() > 0 and np.array_equal(q, R.quantize(after_three, 0.0, 40.0, np.uint16))
        pend(d_v)
        st, hist = dbe.volume_stats(d_v, 0.0, 40.0, 255)
        after_six = PAR.volume_to_host(dbe, d_v)
        assert not np.array_equal(after_six, after_three)
        assert (st.min, st.max) == R.extremes(after_six)
        want, below, above, not_finite = R.histogram(after_six, 0.0, 40.0, 255)
        assert np.array_equal(hist, want) and (st.below, st.above, st.not_finite) == (below, above, not_finite)


# ---- 2. statistics ----------------------------------------------------------------------------------------------------------

def assert_stats(st, v):
    mn, mx = R.extremes(v)
    assert st.min == mn and st.max == mx, (st.min, st.max, mn, mx)
    assert (st.voxels, st.not_finite) == (v.size, int((~np.isfinite(v)).sum()))
    assert (st.below, st.above) == (0, 0)   # no histogram: no range


@pytest.mark.parametrize("n,offset", [(1, 0), (3, 1), (17, 3), (4099, 1), (67 * 33 * 5, 0), (BEYOND_ONE_PASS, 2)])
def test_stats_against_numpy(be, torch, n, offset):
    v = mixed_volume(n)
    keep, d_v = on_device(torch, v, offset)
    st, hist = be.volume_stats(d_v)
    assert hist is None
    assert_stats(st, v)


def test_stats_of_special_volumes(be, torch):
    for v in (np.full(1000, np.nan, np.float32), np.array([np.inf, -np.inf, np.nan], np.float32), np.tile(R.specials(-1.0, 2.0), 7),
              np.array([-0.0, 0.0, -0.0], np.float32), np.array([-5.0, np.nan], np.float32), -np.abs(R.normal_volume(999)) - 1):
        keep, d_v = on_device(torch, v)
        st, _ = be.volume_stats(d_v)
        assert_stats(st, v)
    st, _ = be.volume_stats(on_device(torch, np.full(64, np.nan, np.float32))[1])
    assert st.min == np.inf and st.max == -np.inf and st.not_finite == 64
    # refusals
    keep, d_v = on_device(torch, mixed_volume(100))
    L, ctx, out = be._L, be._ctx, _lib.VolumeStatistics()
    hist = np.zeros(4097, np.uint64)
    assert L.paris_hip_volume_stats(ctx, None, 100, 0.0, 1.0, 0, None, C.byref(out)) == INVALID
    assert L.paris_hip_volume_stats(ctx, d_v.ptr, 100, 0.0, 1.0, 0, None, None) == INVALID
    assert L.paris_hip_volume_stats(ctx, d_v.ptr, 100, 0.0, 1.0, 4097, hist.ctypes.data, C.byref(out)) == INVALID
    assert L.paris_hip_volume_stats(ctx, d_v.ptr, 100, 0.0, 1.0, 16, None, C.byref(out)) == INVALID
    assert L.paris_hip_volume_stats(ctx, d_v.ptr, 100, 1.0, 1.0, 16, hist.ctypes.data, C.byref(out)) == INVALID
    assert L.paris_hip_volume_stats(ctx, d_v.ptr + 2, 100, 0.0, 1.0, 0, None, C.byref(out)) == INVALID
    assert L.paris_hip_volume_stats(ctx, d_v.ptr, 100, 1.0, 1.0, 0, None, C.byref(out)) == 0   # no histogram: the range is ignored
    assert L.paris_hip_volume_stats(ctx, d_v.ptr, 0, 0.0, 1.0, 16, hist.ctypes.data, C.byref(out)) == 0
    assert (out.min, out.max, out.voxels, out.not_finite) == (np.inf, -np.inf, 0, 0)


@pytest.mark.parametrize("n_bins", [1, 2, 255, 4096])
def test_histogram_counter_for_counter(be, torch, n_bins):
    h_lo, h_hi = np.float32(-1.0), np.float32(3.0)
    edges = (h_lo + np.arange(n_bins + 1, dtype=np.float64) * (4.0 / n_bins)).astype(np.float32)   # h_lo, the interior edges, h_hi
    inf = np.float32(np.inf)
    v = np.concatenate([R.normal_volume(50000, seed=n_bins) * 2, edges, np.nextafter(edges, -inf), np.nextafter(edges, inf), R.specials(h_lo, h_hi)])
    np.random.default_rng(3).shuffle(v)
    keep, d_v = on_device(torch, v, 1)
    st, hist = be.volume_stats(d_v, h_lo, h_hi, n_bins)
    want, below, above, not_finite = R.histogram(v, h_lo, h_hi, n_bins)
    assert hist.dtype == np.uint64 and np.array_equal(hist, want), np.flatnonzero(hist != want)[:8]
    assert (st.below, st.above, st.not_finite, st.voxels) == (below, above, not_finite, v.size)
    assert below > 0 and above > 0 and int(hist.sum()) + below + above + not_finite == v.size
    assert (st.min, st.max) == R.extremes(v)


def test_histogram_where_every_lane_hits_one_bin(be, torch):
    v = R.mostly_one_value(BEYOND_ONE_PASS // 4, value=0.0)
    keep, d_v = on_device(torch, v)
    mn, mx = R.extremes(v)
    st, hist = be.volume_stats(d_v, mn, mx, R.BINS_MAX)
    want, below, above, not_finite = R.histogram(v, mn, mx, R.BINS_MAX)
    assert np.array_equal(hist, want) and hist.max() > 0.89 * v.size
    assert (st.min, st.max, st.below, st.above, st.not_finite) == (mn, mx, 0, 0, 0)
    got = be.volume_window_from_histogram(hist, mn, mx, 0.1, 99.9)
    assert got == tuple(float(x) for x in R.auto_window(v))


# ---- 3. the driver ------------------------------------------------------------------------------------------------------------

N_FRAMES = 75
CONFIGS = {"one": ["--slabs", 1, "--devices", 1], "three": ["--slabs", 3, "--batch", 7]}


def run_driver(args, **kw):
    return subprocess.run([str(a) for a in args], capture_output=True, text=True, timeout=300, **kw)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """the small driver set of the flat-field tests, and the float volume of each configuration, reconstructed once"""
    tmp = tmp_path_factory.mktemp("voxels")
    geo, ref, counts_dir, fr, d, f = FF.driver_set(tmp, N_FRAMES)
    base = [P.EXE, "--geometry", geo, "--input", counts_dir, "--flat", ref / "flat.his", "--dark", ref / "dark.his"]
    floats = {}
    for name, extra in CONFIGS.items():
        o = tmp / ("float_" + name)
        r = run_driver(base + ["--output", o] + extra)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "written as" not in r.stdout and sorted(os.listdir(o)) == ["vol.ddbvf"]
        floats[name] = F.ddbvf_read(str(o / "vol.ddbvf"))[1]
    return {"tmp": tmp, "base": base, "floats": floats, "frames": (fr, d, f)}


def test_driver_without_the_option_writes_the_same_ddbvf(driver):
    fr, d, f = driver["frames"]
    want = FF.mirror_volume(fr, d, f, 1e-5)
    for name in CONFIGS:
        assert np.array_equal(FF.bits(driver["floats"][name]), FF.bits(want)), name
    raw = open(driver["tmp"] / "float_one" / "vol.ddbvf", "rb").read()
    assert len(raw) == 32 + want.nbytes and raw[32:] == want.tobytes()


def counts_line(v, lo, hi, dtype):
    n, below, above, not_finite = R.counts(v, lo, hi)
    return "%d voxel(s) written as %s over [%.9g, %.9g]: %d below, %d above, %d not finite" % (
        n, "u8" if dtype == np.uint8 else "u16", float(lo), float(hi), below, above, not_finite)


def check_output(o, v, lo, hi, dtype, stdout):
    det = B.DetectorGeometry(*FF.DRV_GEO)
    vg = B.calculate_volume_geometry(det)
    assert sorted(os.listdir(o)) == ["vol.mhd", "vol.raw"]
    fields, q = R.read_mhd(str(o / "vol.mhd"))
    want = R.quantize(v, lo, hi, dtype)
    assert q.dtype == dtype and q.shape == v.shape and os.path.getsize(o / "vol.raw") == want.nbytes
    assert np.array_equal(q, want), np.argwhere(q != want)[:4]
    levels = R.LEVELS[np.dtype(dtype)]
    assert fields["ObjectType"] == "Image" and fields["NDims"] == "3" and fields["BinaryData"] == "True"
    assert fields["BinaryDataByteOrderMSB"] == "False" and fields["ElementDataFile"] == "vol.raw"
    assert fields["DimSize"] == "%d %d %d" % (vg.dim_x, vg.dim_y, vg.dim_z)
    assert fields["ElementSpacing"] == "%.9g %.9g %.9g" % (vg.l_vx_x, vg.l_vx_y, vg.l_vx_z)
    assert fields["ElementType"] == ("MET_UCHAR" if dtype == np.uint8 else "MET_USHORT")
    assert fields["ElementToIntensityFunctionSlope"] == "%.9g" % ((float(hi) - float(lo)) / levels)
    assert fields["ElementToIntensityFunctionOffset"] == "%.9g" % float(lo)
    assert counts_line(v, lo, hi, dtype) in stdout, stdout


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_driver_quantised_output_equals_the_rule_on_the_float_volume(driver, config, dtype):
    v = driver["floats"][config]
    lo, hi = np.float32(np.percentile(v, 5)), np.float32(np.percentile(v, 95))   # a window that cuts both ends
    o = driver["tmp"] / ("q_%s_%s" % (config, np.dtype(dtype).name))
    r = run_driver(driver["base"] + ["--output", o, "--voxel-type", "u8" if dtype == np.uint8 else "u16", "--voxel-range",
                                     "%r:%r" % (float(lo), float(hi))] + CONFIGS[config])
    assert r.returncode == 0, r.stdout + r.stderr
    check_output(o, v, lo, hi, dtype, r.stdout)
    assert R.counts(v, lo, hi)[1] > 0 and R.counts(v, lo, hi)[2] > 0


def test_driver_chunks_of_a_few_slices(driver):
    """a drain chunk smaller than the slab: several quantise calls per slab, each at its slice offset"""
    v = driver["floats"]["three"]
    lo, hi = np.float32(np.percentile(v, 5)), np.float32(np.percentile(v, 95))
    o = driver["tmp"] / "q_chunks"
    slice_bytes = v.shape[1] * v.shape[2] * 2
    r = run_driver(driver["base"] + ["--output", o, "--voxel-type", "u16", "--voxel-range", "%r:%r" % (float(lo), float(hi)), "--slabs", 2,
                                     "--drain-chunk-kib", max(1, 3 * slice_bytes // 1024)])
    assert r.returncode == 0, r.stdout + r.stderr
    check_output(o, v, lo, hi, np.uint16, r.stdout)


@pytest.mark.parametrize("spec,percentiles", [("auto", (0.1, 99.9)), ("auto:2.5:90", (2.5, 90.0))])
def test_driver_automatic_window(driver, spec, percentiles):
    v = driver["floats"]["one"]
    lo, hi = R.auto_window(v, *percentiles)
    o = driver["tmp"] / ("q_" + spec.replace(":", "_"))
    r = run_driver(driver["base"] + ["--output", o, "--voxel-type", "u16", "--voxel-range", spec] + CONFIGS["one"])
    assert r.returncode == 0, r.stdout + r.stderr
    check_output(o, v, lo, hi, np.uint16, r.stdout)


def test_driver_refuses_before_any_device_work(driver):
    bad = driver["tmp"] / "bad"
    cases = [(["--voxel-type", "u16", "--voxel-range", "auto", "--slabs", 3], "--voxel-range auto"),
             (["--voxel-type", "u16", "--voxel-range", "auto"], "--voxel-range auto"),   # memory-driven slabs: not one slab for sure
             (["--voxel-type", "u16"], "--voxel-type"),
             (["--voxel-range", "0:1"], "--voxel-range"),
             (["--voxel-type", "u32", "--voxel-range", "0:1"], "--voxel-type"),
             (["--voxel-type", "float", "--voxel-range", "0:1"], "--voxel-type")]
    for spec in ("abc", "1", "1:2:3", "0:", ":1", "0:x", "2:1", "1:1", "nan:1", "0:inf", "auto:5", "auto:60:40", "auto:-1:50", "auto:0:101",
                 "auto:a:b", ""):
        cases.append((["--voxel-type", "u8", "--voxel-range", spec, "--slabs", 1], "--voxel-range"))
    for extra, name in cases:
        r = run_driver(driver["base"] + ["--output", bad] + extra)
        assert r.returncode == 1 and name in r.stderr, (extra, r.returncode, r.stderr)
        assert not bad.exists(), extra
