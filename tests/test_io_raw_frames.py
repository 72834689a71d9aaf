"""Frames handed out in their stored pixel type (paris_amd/host/paris/{his,source}.h: his::reader::read_rows_raw,
frame_stream::next_raw, shared_frames::next_raw through paris_io_stream_scan_raw / paris_io_shared_scan_raw of libparis_io.so):
the bytes the HIS file holds, bit for bit, with the frame's type -- f64 as its f32 cast -- for paris_hip_upload_projection_raw.
Pure host code: runs without a GPU."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import formats as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_fp = C.POINTER(C.c_float)
_u32p = C.POINTER(C.c_uint32)
_i32p = C.POINTER(C.c_int32)
# HIS number type -> (pixel type of the raw scan: PARIS_HIP_PIXEL_*, numpy type of the bytes it returns)
RAW = {2: (1, np.uint8), 4: (2, np.uint16), 32: (3, np.uint32), 64: (4, np.float32), 128: (4, np.float32)}


@pytest.fixture(scope="module")
def io():
    lib = C.CDLL(os.environ.get("PARIS_IO_LIB") or os.path.join(ROOT, "paris_amd", "lib", "libparis_io.so"))
    lib.paris_io_stream_scan_raw.argtypes = [C.c_char_p, C.c_int, C.c_char_p, C.c_uint16, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                             C.c_uint32, _u32p, _u32p, _fp, C.c_void_p, _i32p, _u32p]
    lib.paris_io_shared_scan_raw.argtypes = [C.c_char_p, C.c_int, C.c_char_p, C.c_uint16, C.c_uint32, C.c_uint32, C.c_uint32, _u32p, _u32p,
                                             _u32p, C.c_uint32, C.c_uint32, _u32p, _u32p, _fp, C.c_void_p, _i32p, C.POINTER(C.c_uint64)]
    return lib


def frames_of(number_type, n, h, w, seed):
    rng = np.random.default_rng(seed)
    if number_type == 2:
        return rng.integers(0, 256, (n, h, w), dtype=np.uint8)
    if number_type == 4:
        return rng.integers(0, 65536, (n, h, w), dtype=np.uint16)
    if number_type == 32:  # above 2^24: the f32 cast rounds, the raw bytes do not
        return rng.integers(0, 2 ** 32, (n, h, w), dtype=np.uint64).astype(np.uint32)
    if number_type == 64:
        return rng.standard_normal((n, h, w)) * 1e3 + 1e-9
    f = (rng.standard_normal((n, h, w)) * 1e3).astype(np.float32)
    f.reshape(-1)[:4] = np.array([0x7fc01234, 0x80000000, 0x00000001, 0xff800000], np.uint32).view(np.float32)  # NaN payload, -0, denormal, -inf
    return f


def stored(frame, number_type):
    """what the raw scan must return for one frame, as its raw bytes"""
    return np.ascontiguousarray(frame.astype(RAW[number_type][1]))


def stream_scan_raw(io, d, w, h, first=0, count=None, quality=1, cap=64, sentinel=0xA5):
    count = h - first if count is None else count
    data = np.full((cap, h, w * 4), sentinel, np.uint8)  # 4 bytes per pixel of room, the stored rows at their own offsets
    n, idx, phi, types, skipped = C.c_uint32(), (C.c_uint32 * cap)(), (C.c_float * cap)(), (C.c_int32 * cap)(), C.c_uint32()
    rc = io.paris_io_stream_scan_raw(str(d).encode(), 0, None, quality, w, h, first, count, cap, C.byref(n), idx, phi, data.ctypes.data,
                                     types, C.byref(skipped))
    assert rc == 0
    return n.value, list(idx)[:n.value], list(types)[:n.value], data[:n.value], skipped.value


def frame_bytes(data_k, ptype, w, h):
    """the dim_x * dim_y stored pixels at the start of a 4-byte-per-pixel frame slot"""
    s = {1: 1, 2: 2, 3: 4, 4: 4}[ptype]
    return data_k.reshape(-1)[:w * h * s]


@pytest.mark.parametrize("number_type", [2, 4, 32, 64, 128])
@pytest.mark.parametrize("image_header", [0, 32])
def test_stream_scan_raw_returns_the_stored_bytes(io, tmp_path, number_type, image_header):
    h, w = 9, 13
    fr = frames_of(number_type, 3, h, w, number_type)
    d = tmp_path / "in"
    d.mkdir()
    (d / "a.his").write_bytes(F.his_file_bytes(fr, number_type, image_header))
    n, idx, types, data, skipped = stream_scan_raw(io, d, w, h)
    assert n == 3 and idx == [0, 1, 2] and skipped == 0
    ptype = RAW[number_type][0]
    assert types == [ptype] * 3
    for k in range(3):
        got = frame_bytes(data[k], ptype, w, h)
        assert np.array_equal(got, stored(fr[k], number_type).view(np.uint8).reshape(-1))
        rest = data[k].reshape(-1)[got.size:]
        assert np.all(rest == 0xA5)  # nothing past the stored frame


@pytest.mark.parametrize("number_type", [2, 4, 32, 64])
def test_row_bands_quality_stride_and_truncation(io, tmp_path, number_type):
    h, w = 11, 6
    fr = frames_of(number_type, 5, h, w, 7)
    ptype, t = RAW[number_type]
    s = np.dtype(t).itemsize
    d = tmp_path / "in"
    d.mkdir()
    (d / "a.his").write_bytes(F.his_file_bytes(fr, number_type, 16))
    # a band of rows: exactly those rows at their own offsets, the rest of the slot untouched
    n, idx, types, data, _ = stream_scan_raw(io, d, w, h, first=3, count=4, quality=2)
    assert n == 3 and idx == [0, 2, 4] and types == [ptype] * 3
    for k, i in enumerate(idx):
        flat = data[k].reshape(-1)
        want = stored(fr[i], number_type).view(np.uint8).reshape(-1)
        assert np.array_equal(flat[3 * w * s:7 * w * s], want[3 * w * s:7 * w * s])
        assert np.all(flat[:3 * w * s] == 0xA5) and np.all(flat[7 * w * s:] == 0xA5)
    # a file cut off in the middle of frame 1: the missing elements read as 0, as the float reader has them
    whole = F.his_file_bytes(fr[:2], number_type)
    cut = len(whole) - (w * h * np.dtype(F.HIS_TYPES[number_type]).itemsize) // 2
    e = tmp_path / "cut"
    e.mkdir()
    (e / "a.his").write_bytes(whole[:cut])
    n, idx, types, data, _ = stream_scan_raw(io, e, w, h)
    assert n == 2
    got = frame_bytes(data[1], ptype, w, h).view(t).reshape(h, w)
    have = (w * h) // 2
    want = stored(fr[1], number_type).reshape(-1).copy()
    want[have:] = 0
    assert np.array_equal(got.reshape(-1).view(np.uint8), want.view(np.uint8))


def test_directory_mixing_number_types(io, tmp_path):
    """the type goes with each frame: a directory may change it from file to file"""
    h, w = 5, 8
    d = tmp_path / "in"
    d.mkdir()
    order = [4, 2, 128, 32, 64]
    frames = []
    for k, nt in enumerate(order):
        fr = frames_of(nt, 2, h, w, 30 + k)
        frames += [(nt, f) for f in fr]
        (d / ("f%d.his" % k)).write_bytes(F.his_file_bytes(fr, nt))
    (d / "notes.txt").write_text("not HIS")
    n, idx, types, data, skipped = stream_scan_raw(io, d, w, h)
    assert n == 10 and skipped == 1 and idx == list(range(10))
    assert types == [RAW[nt][0] for nt, _ in frames]
    for k, (nt, f) in enumerate(frames):
        assert np.array_equal(frame_bytes(data[k], types[k], w, h), stored(f, nt).view(np.uint8).reshape(-1))


@pytest.mark.parametrize("capacity,delays", [(32, (0, 0, 0)), (2, (0, 3000, 0))])
def test_shared_scan_raw_serves_the_same_bytes(io, tmp_path, capacity, delays):
    """several consumers with different row bands, one of them slow enough to fall out of a small ring (its own fallback stream):
    every consumer gets the stored bytes of its band, the type of every frame, and -- from the ring -- each frame read once"""
    h, w = 12, 10
    d = tmp_path / "in"
    d.mkdir()
    frames = []
    for k, nt in enumerate([4, 2, 32, 128]):
        fr = frames_of(nt, 3, h, w, 50 + k)
        frames += [(nt, f) for f in fr]
        (d / ("f%d.his" % k)).write_bytes(F.his_file_bytes(fr, nt, 8))
    nt_ = len(delays)
    bands = [(0, h), (2, 5), (7, 5)]
    cap = 16
    data = np.full((nt_, cap, h, w * 4), 0x5A, np.uint8)
    got = (C.c_uint32 * nt_)()
    idx, phi, types = (C.c_uint32 * (nt_ * cap))(), (C.c_float * (nt_ * cap))(), (C.c_int32 * (nt_ * cap))()
    cnt = (C.c_uint64 * 3)()
    rc = io.paris_io_shared_scan_raw(str(d).encode(), 0, None, 1, w, h, nt_, (C.c_uint32 * nt_)(*[b[0] for b in bands]),
                                     (C.c_uint32 * nt_)(*[b[1] for b in bands]), (C.c_uint32 * nt_)(*delays), capacity, cap, got, idx, phi,
                                     data.ctypes.data, types, cnt)
    assert rc == 0 and list(got) == [12] * nt_
    if delays == (0, 0, 0):
        assert cnt[0] == 12 and cnt[2] == 0  # read once, served from the ring
    else:
        assert cnt[2] > 0  # the slow consumer re-read through its own stream
    for i, (first, count) in enumerate(bands):
        for k, (nt, f) in enumerate(frames):
            ptype, t = RAW[nt]
            s = np.dtype(t).itemsize
            assert types[i * cap + k] == ptype and idx[i * cap + k] == k
            flat = data[i, k].reshape(-1)
            want = stored(f, nt).view(np.uint8).reshape(-1)
            a, b = first * w * s, (first + count) * w * s
            assert np.array_equal(flat[a:b], want[a:b])
            assert np.all(flat[:a] == 0x5A) and np.all(flat[b:] == 0x5A)
