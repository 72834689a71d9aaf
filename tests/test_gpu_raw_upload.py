"""paris_hip_upload_projection_raw: detector frames uploaded in their stored pixel type (u8 / u16 / u32 / f32) and widened to fp32
on the device, in place -- bit for bit the host's static_cast<float> -- through the Python mirror (Backend.upload_raw), PARIS's own
loop, and the paris.hip driver (paris_amd/host/paris/reconstruct.h), which now uploads every frame that way."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import grid_cap_rule as G
import test_gpu_paris_hip as P
from oracle import formats as F
from paris_amd import _lib
from paris_amd import backend as B

pytestmark = pytest.mark.gpu

SENTINEL = np.uint32(0x7F7F7F7F)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def values(dtype, dim_y, dim_x, seed):
    rng = np.random.default_rng(seed)
    if dtype == np.uint8:
        h = rng.integers(0, 256, (dim_y, dim_x), dtype=np.uint8)
        special = [0, 1, 127, 128, 254, 255]
    elif dtype == np.uint16:
        h = rng.integers(0, 65536, (dim_y, dim_x), dtype=np.uint16)
        special = [0, 1, 255, 256, 32768, 65535]
    elif dtype == np.uint32:
        h = rng.integers(0, 2 ** 32, (dim_y, dim_x), dtype=np.uint64).astype(np.uint32)
        # exact, rounding ties to even (2^24 + 1 -> 2^24, 2^24 + 3 -> 2^24 + 4, ...), and the top of the range (-> 2^32)
        special = [0, 1, 2 ** 24, 2 ** 24 + 1, 2 ** 24 + 2, 2 ** 24 + 3, 2 ** 25 + 2, 2 ** 25 + 6, 2 ** 31 + 128, 2 ** 31 + 384,
                   2 ** 32 - 129, 2 ** 32 - 128, 2 ** 32 - 1]
    else:
        h = (rng.standard_normal((dim_y, dim_x)) * 1e3).astype(np.float32)
        # NaN payloads (quiet and signalling, both signs), +-0, +-inf, denormals
        special = np.array([0x7FC01234, 0x7F800001, 0xFFC00007, 0x7FBFFFFF, 0x00000000, 0x80000000, 0x7F800000, 0xFF800000,
                            0x00000001, 0x007FFFFF, 0x80000001, 0x80400000], np.uint32).view(np.float32)
    flat = h.reshape(-1)
    flat[:len(special)] = np.asarray(special).astype(h.dtype) if dtype != np.float32 else special
    return h


def host_rows(h, padded):
    """h itself, or the same rows inside a wider array (h_pitch > s * dim_x)"""
    if not padded:
        return np.ascontiguousarray(h)
    wide = np.full((h.shape[0], h.shape[1] + 5), 0xAB, h.dtype)
    wide[:, :h.shape[1]] = h
    return wide[:, :h.shape[1]]


def read_rows(be, ptr, pitch, dim_y):
    """the whole pitch of every row, padding included"""
    h = be.make_projection_host(pitch // 4, dim_y)
    be.copy_d2h(B.Projection(ptr, pitch // 4, dim_y, pitch=pitch, on_device=True), h)
    return bits(h.buf)


def fill(be, ptr, pitch, dim_y):
    src = np.full((dim_y, pitch // 4), SENTINEL, np.uint32).view(np.float32)
    be.copy_h2d(B.Projection(src, pitch // 4, dim_y), B.Projection(ptr, pitch // 4, dim_y, pitch=pitch, on_device=True))


@pytest.fixture(scope="module")
def be():
    with B.Backend(0) as b:
        yield b


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.uint32, np.float32])
@pytest.mark.parametrize("dim_x", [64, 97, 2048])
@pytest.mark.parametrize("wrapped", [False, True])
@pytest.mark.parametrize("padded", [False, True])
def test_bit_exact_widening(be, dtype, dim_x, wrapped, padded):
    """pool buffer (rows padded to 256 B) or caller memory with d_pitch = 4 * dim_x (97: neither aligned nor a whole number of
    16-byte vectors -- the one-pixel-per-lane path), tight or padded host rows: the rows read back as h.astype(np.float32), and the
    padding of the rows is not written"""
    dim_y = 7
    h = values(dtype, dim_y, dim_x, dim_x)
    if wrapped:
        v = be.make_volume_device(dim_x, dim_y, 1)
        d = be.wrap_projection(v.ptr, 4 * dim_x, dim_x, dim_y)
    else:
        d = be.make_projection_device(dim_x, dim_y)
    fill(be, d.ptr, d.pitch, dim_y)
    be.upload_raw(host_rows(h, padded), d)
    got = read_rows(be, d.ptr, d.pitch, dim_y)
    assert np.array_equal(got[:, :dim_x], bits(h.astype(np.float32)))
    assert np.all(got[:, dim_x:] == SENTINEL)
    be.free(d)
    if wrapped:
        be.free(v)


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.uint32, np.float32])
@pytest.mark.parametrize("dim_x", G.WIDEN_DIM_XS)
def test_more_rows_than_the_widening_grid_has_blocks(be, dtype, dim_x):
    """4100 rows against WIDEN_MAX_BLOCKS = 2048: every block comes round for a second row, four of them for a third. 5 pixels a row:
    one per lane; 8: whole 16-byte vectors of every stored type. Rows 0 .. 2 of the buffer and the padding of every row are not written"""
    assert G.WIDEN_ROWS > 2 * 2048
    r0, dim_y = 3, G.WIDEN_ROWS + 3
    h = values(dtype, G.WIDEN_ROWS, dim_x, dim_x)
    d = be.make_projection_device(dim_x, dim_y)
    assert d.pitch > 4 * dim_x
    fill(be, d.ptr, d.pitch, dim_y)
    be.upload_raw(h, d, row_first=r0)
    got = read_rows(be, d.ptr, d.pitch, dim_y)
    assert np.array_equal(got[r0:, :dim_x], bits(h.astype(np.float32)))
    assert np.all(got[:r0] == SENTINEL) and np.all(got[:, dim_x:] == SENTINEL)
    be.free(d)


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.uint32])
@pytest.mark.parametrize("dim_x", [97, 256])
def test_row_band_leaves_other_rows_and_padding(be, dtype, dim_x):
    dim_y, r0, n = 12, 3, 5
    d = be.make_projection_device(dim_x, dim_y)
    assert d.pitch > 4 * dim_x or dim_x == 256
    fill(be, d.ptr, d.pitch, dim_y)
    h = values(dtype, n, dim_x, 5)
    band = be.wrap_projection(d.ptr + r0 * d.pitch, d.pitch, dim_x, n)
    be.upload_raw(h, band)
    got = read_rows(be, d.ptr, d.pitch, dim_y)
    assert np.array_equal(got[r0:r0 + n, :dim_x], bits(h.astype(np.float32)))
    assert np.all(got[:r0] == SENTINEL) and np.all(got[r0 + n:] == SENTINEL) and np.all(got[:, dim_x:] == SENTINEL)
    be.free(d)


def test_rejects_and_stays_usable(be):
    dim_x, dim_y = 64, 4
    d = be.make_projection_device(dim_x, dim_y)
    h = values(np.uint16, dim_y, dim_x, 1)
    L, ctx = be._L, be._ctx
    hp = h.ctypes.data
    bad = [(d.ptr, d.pitch, hp, 2 * dim_x, 5),                   # unknown type
           (d.ptr, d.pitch, hp, 8 * dim_x, 0),                   # unknown type
           (d.ptr, d.pitch, hp, 8 * dim_x, 64),                  # f64's HIS number: not a pixel type (f64 stays on the host)
           (d.ptr, 4 * dim_x - 4, hp, 2 * dim_x, _lib.PIXEL_U16),  # d_pitch short
           (d.ptr, 4 * dim_x + 2, hp, 2 * dim_x, _lib.PIXEL_U16),  # d_pitch not a multiple of 4
           (d.ptr, d.pitch, hp, 2 * dim_x - 1, _lib.PIXEL_U16),    # h_pitch short
           (d.ptr, d.pitch, hp, 4 * dim_x - 4, _lib.PIXEL_U32),    # h_pitch short for u32
           (None, d.pitch, hp, 2 * dim_x, _lib.PIXEL_U16),         # null device pointer
           (d.ptr, d.pitch, None, 2 * dim_x, _lib.PIXEL_U16)]      # null host pointer
    for dp, dpitch, src, hpitch, t in bad:
        assert L.paris_hip_upload_projection_raw(ctx, dp, dpitch, src, hpitch, dim_x, dim_y, t) == _lib.ERROR_INVALID_ARGUMENT
    assert L.paris_hip_upload_projection_raw(None, d.ptr, d.pitch, hp, 2 * dim_x, dim_x, dim_y, _lib.PIXEL_U16) == _lib.ERROR_INVALID_ARGUMENT
    with pytest.raises(TypeError, match="float64"):
        be.upload_raw(h.astype(np.float64), d)
    with pytest.raises(TypeError):
        be.upload_raw(h.astype(np.int16), d)
    be.upload_raw(h, d)  # the ctx goes on as if nothing had happened
    got = read_rows(be, d.ptr, d.pitch, dim_y)
    assert np.array_equal(got[:, :dim_x], bits(h.astype(np.float32)))
    be.free(d)


G96 = (96, 40, 0.2173, 0.2671, 0.75, -1.25, 137.5, 91.25, 3.0)


@pytest.mark.parametrize("one_pinned_buffer", [False, True])
def test_through_paris_loop_by_reference(oracle, one_pinned_buffer):
    """PARIS's loop as paris::hip runs it (set_paris_loop_defaults: stage fusion, deferral by reference with overlap, the filter in
    place): 40 u16 frames at 96 x 40, each uploaded raw into a fresh buffer, weighted, filtered, backprojected, freed. The same
    volume, bit for bit, as the loop fed the host-cast frames through upload(); with weight and filter off the oracle's
    backprojection bit for bit. one_pinned_buffer: every frame goes through ONE pinned buffer, refilled after a fence -- more
    uploads than the ctx has upload events."""
    det, odet = B.DetectorGeometry(*G96), oracle.DetectorGeometry(*G96)
    vg, ovg = B.calculate_volume_geometry(det), oracle.calculate_volume_geometry(odet)
    n_proj = 40
    frames = [(oracle.lcg_projection(96, 40, i) * 60000).astype(np.uint16) for i in range(n_proj)]
    want = np.zeros((vg.dim_z, vg.dim_y, vg.dim_x), np.float32)
    for i, f in enumerate(frames):
        s, c, ds, dt = oracle.backproject_constants(odet, i)
        oracle.backproject(want, f.astype(np.float32), 0, odet, ovg, s, c, ds, dt)

    def run(raw, stages):
        with B.Backend(0, synchronous=False) as abe:
            abe.set_paris_loop_defaults(depth=4)
            L, ctx = abe._L, abe._ctx
            d_v = abe.make_volume_device(vg.dim_x, vg.dim_y, vg.dim_z)
            fence = C.c_void_p()
            assert L.paris_hip_fence_create(ctx, C.byref(fence)) == 0
            shared = C.c_void_p()
            assert L.paris_hip_malloc_host(ctx, 96 * 40 * 4, C.byref(shared)) == 0
            for i in range(n_proj):
                d_p = abe.make_projection_device(96, 40)
                h = C.c_void_p()
                if one_pinned_buffer:
                    assert L.paris_hip_fence_wait(ctx, fence) == 0  # the previous frame's copy has read the buffer
                    h = shared
                else:
                    assert L.paris_hip_malloc_host(ctx, 96 * 40 * 4, C.byref(h)) == 0
                if raw:
                    pinned = np.ctypeslib.as_array((C.c_uint16 * (96 * 40)).from_address(h.value)).reshape(40, 96)
                    pinned[:] = frames[i]
                    abe.upload_raw(pinned, d_p)
                else:
                    pinned = np.ctypeslib.as_array((C.c_float * (96 * 40)).from_address(h.value)).reshape(40, 96)
                    pinned[:] = frames[i].astype(np.float32)
                    abe.upload(B.Projection(pinned, 96, 40), d_p)
                assert L.paris_hip_fence_record(ctx, fence) == 0
                if not one_pinned_buffer:
                    assert L.paris_hip_free_host(ctx, h) == 0
                d_p.idx = i
                if stages:
                    B.weight(abe, d_p, det)
                    B.filter(abe, d_p, det)
                B.backproject(abe, d_p, d_v, 0, det, vg, False, False, None)
                abe.free(d_p)
            got = abe.make_volume_host(vg.dim_x, vg.dim_y, vg.dim_z)
            abe.copy_d2h(d_v, got)
            assert L.paris_hip_fence_destroy(ctx, fence) == 0
            assert L.paris_hip_free_host(ctx, shared) == 0
            return got.buf.copy()

    assert np.array_equal(bits(run(True, True)), bits(run(False, True)))
    assert np.array_equal(bits(run(True, False)), bits(want))


def his_set(d, frames_by_file):
    d.mkdir()
    for k, (nt, fr) in enumerate(frames_by_file):
        (d / ("proj_%03d.his" % k)).write_bytes(F.his_file_bytes(fr, nt, 32))
    geo = d.parent / "geo.ini"
    geo.write_text("\n".join("%s = %s" % kv for kv in zip(
        ("n_row", "n_col", "l_px_row", "l_px_col", "delta_s", "delta_t", "d_so", "d_od", "delta_phi"), P.KAT)) + "\n")
    return geo


def lcg_frames(oracle, first, n, scale, dtype):
    return np.stack([oracle.lcg_projection(64, 48, first + j) * scale for j in range(n)]).astype(dtype)


def h2d_bytes(out):
    lines = [l for l in out.splitlines() if l.startswith("  H2D of device ")]
    assert lines, out
    return sum(int(l.split(":")[1].split()[0]) for l in lines)


SETS = {
    "u8": [(2, (2, 255.0, np.uint8)), (2, (3, 255.0, np.uint8))],
    "u32": [(32, (3, 4.0e9, np.uint32)), (32, (2, 3.0e9, np.uint32))],  # far above 2^24: the f32 cast rounds
    "f32": [(128, (3, 1.0, np.float32)), (128, (2, 1.0, np.float32))],
    "f64": [(64, (3, 1.0, np.float64)), (64, (2, 1.0, np.float64))],
    "mixed": [(4, (2, 60000.0, np.uint16)), (2, (1, 255.0, np.uint8)), (128, (2, 1.0, np.float32)), (32, (2, 4.0e9, np.uint32)),
              (64, (1, 1.0, np.float64))],
}


@pytest.mark.parametrize("name", sorted(SETS))
def test_paris_hip_driver_every_number_type(tmp_path, oracle, name):
    """paris.hip on HIS sets of each number type and a directory that changes type from file to file: the DDBVF the oracle's
    pipeline makes of the frames' f32 casts, under test_gpu_paris_hip.py's comparison"""
    frames_by_file, first = [], 0
    for nt, (n, scale, dtype) in SETS[name]:
        frames_by_file.append((nt, lcg_frames(oracle, first, n, scale, dtype)))
        first += n
    geo = his_set(tmp_path / "in", frames_by_file)
    P.run(["--geometry", geo, "--input", tmp_path / "in", "--output", tmp_path / "out", "--name", "kat"])
    _, vol = F.ddbvf_read(str(tmp_path / "out" / "kat.ddbvf"))
    det = oracle.DetectorGeometry(*P.KAT)
    vg = oracle.calculate_volume_geometry(det)
    proj = [f.astype(np.float32) for _, fr in frames_by_file for f in fr]
    P.assert_close(vol, oracle.reconstruct(det, vg, len(proj), projections=proj))


def test_paris_hip_driver_slabs_shared_source_and_h2d_bytes(tmp_path, oracle):
    """--slabs 3 on three device threads sharing the read-once frame source (row bands, the raw ring), on the mixed directory; and
    the report's H2D bytes: a u16 set moves exactly half the bytes of the same frames stored as f32"""
    frames_by_file, first = [], 0
    for nt, (n, scale, dtype) in SETS["mixed"]:
        frames_by_file.append((nt, lcg_frames(oracle, first, n, scale, dtype)))
        first += n
    geo = his_set(tmp_path / "in", frames_by_file)
    env = dict(os.environ, PARIS_HIP_VIRTUAL_DEVICES="3")
    r = subprocess.run([P.EXE, "--geometry", str(geo), "--input", str(tmp_path / "in"), "--output", str(tmp_path / "out"), "--name", "kat",
                        "--slabs", "3", "--share-frames", "1"], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert any(l.startswith("shared frame source:") for l in r.stdout.splitlines())
    _, vol = F.ddbvf_read(str(tmp_path / "out" / "kat.ddbvf"))
    det = oracle.DetectorGeometry(*P.KAT)
    vg = oracle.calculate_volume_geometry(det)
    proj = [f.astype(np.float32) for _, fr in frames_by_file for f in fr]
    P.assert_close(vol, oracle.reconstruct(det, vg, len(proj), projections=proj))

    u16 = lcg_frames(oracle, 0, 6, 60000.0, np.uint16)
    outs = {}
    for nt, fr in ((4, u16), (128, u16.astype(np.float32))):
        d = tmp_path / ("h%d" % nt)
        g = his_set(d, [(nt, fr)])
        outs[nt] = P.run(["--geometry", g, "--input", d, "--output", tmp_path / ("o%d" % nt), "--name", "kat", "--slabs", 3])
        _, v = F.ddbvf_read(str(tmp_path / ("o%d" % nt) / "kat.ddbvf"))
        outs[nt] = (h2d_bytes(outs[nt]), v)
    assert outs[4][0] * 2 == outs[128][0] > 0
    assert np.array_equal(bits(outs[4][1]), bits(outs[128][1]))  # the same frames, the same volume
