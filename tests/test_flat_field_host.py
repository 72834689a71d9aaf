"""Dark / flat correction on the host: the mean of a reference file (his::mean_frame through libparis_io) against numpy, and the
refusals of paris.hip --flat / --dark / --min-transmission, which come before any device work (no GPU needed)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle import formats as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "paris_amd", "host", "demo", "paris.hip")
GEO_KEYS = ("n_row", "n_col", "l_px_row", "l_px_col", "delta_s", "delta_t", "d_so", "d_od", "delta_phi")
GEO = (64, 48, 0.2, 0.25, 1.5, -0.75, 100, 200, 1.0)

_u32p = C.POINTER(C.c_uint32)
_fp = C.POINTER(C.c_float)


@pytest.fixture(scope="module")
def io():
    lib = C.CDLL(os.environ.get("PARIS_IO_LIB") or os.path.join(ROOT, "paris_amd", "lib", "libparis_io.so"))
    lib.paris_io_his_mean_frame.argtypes = [C.c_char_p, _u32p, _u32p, _u32p, C.POINTER(_fp)]
    lib.paris_io_free.argtypes = [C.c_void_p]
    return lib


def mean_frame(io, path):
    n, w, h, data = C.c_uint32(), C.c_uint32(), C.c_uint32(), _fp()
    if io.paris_io_his_mean_frame(str(path).encode(), C.byref(n), C.byref(w), C.byref(h), C.byref(data)):
        raise OSError("cannot open %s" % path)
    if n.value == 0:
        assert not data
        return 0, None
    a = np.ctypeslib.as_array(data, shape=(h.value, w.value)).copy()
    io.paris_io_free(data)
    return n.value, a


def numpy_mean(frames):
    """each frame as the reader gives it (fp32; f64 as its fp32 cast), summed in float64 in frame order, / n, rounded once"""
    acc = np.zeros(frames.shape[1:], np.float64)
    for f in frames:
        acc += f.astype(np.float32).astype(np.float64)
    return (acc / len(frames)).astype(np.float32)


@pytest.mark.parametrize("number_type", sorted(F.HIS_TYPES))
@pytest.mark.parametrize("n_frames", [1, 3, 7])
def test_mean_frame_equals_numpy_bit_for_bit(tmp_path, io, number_type, n_frames):
    rng = np.random.default_rng(number_type * 10 + n_frames)
    dt = np.dtype(F.HIS_TYPES[number_type])
    if dt.kind == "u":
        hi = np.iinfo(dt).max
        frames = rng.integers(0, hi, size=(n_frames, 24, 40), endpoint=True, dtype=np.uint64).astype(dt)
        frames[0, 0, :4] = [0, hi, hi - 1, 1]
    else:
        # values whose float64 sums round: several magnitudes, both signs, and f64 values that are not fp32 numbers
        frames = (rng.standard_normal((n_frames, 24, 40)) * 10.0 ** rng.integers(-3, 6, size=(n_frames, 24, 40))).astype(dt)
        frames[0, 0, :3] = [1e30, -1e30, 1.0 / 3.0]
    p = tmp_path / "ref.his"
    p.write_bytes(F.his_file_bytes(frames, number_type, 32))
    n, got = mean_frame(io, p)
    assert n == n_frames
    want = numpy_mean(frames)
    assert got.shape == want.shape
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_mean_frame_of_a_file_without_frames_and_a_missing_file(tmp_path, io):
    p = tmp_path / "empty.his"
    p.write_bytes(F.his_file_bytes(np.zeros((0, 8, 8), np.uint16), 4))
    assert mean_frame(io, p) == (0, None)
    with pytest.raises(OSError):
        mean_frame(io, tmp_path / "missing.his")


def write_set(tmp_path, n_frames=4):
    d = tmp_path / "in"
    d.mkdir()
    fr = np.full((n_frames, GEO[1], GEO[0]), 1000, np.uint16)
    (d / "scan.his").write_bytes(F.his_file_bytes(fr, 4, 32))
    ini = tmp_path / "geo.ini"
    ini.write_text("\n".join("%s = %s" % kv for kv in zip(GEO_KEYS, GEO)) + "\n")
    return ini, d


def reference(path, shape=(GEO[1], GEO[0]), n=3, value=4000):
    path.write_bytes(F.his_file_bytes(np.full((n,) + shape, value, np.uint16), 4))
    return path


def run_driver(args):
    if not os.path.exists(EXE):
        pytest.fail("%s missing: run __graft_entry__.build()" % EXE)
    return subprocess.run([EXE] + [str(a) for a in args], capture_output=True, text=True, timeout=120)


def refused(tmp_path, ini, d, extra, *words):
    r = run_driver(["--geometry", ini, "--input", d, "--output", tmp_path / "out"] + extra)
    assert r.returncode == 1, r.stdout + r.stderr
    assert "Pipeline construction failed" in r.stderr, r.stderr
    for w in words:
        assert w in r.stderr, (w, r.stderr)
    assert not (tmp_path / "out").exists()   # refused before the output was set up, let alone a device


def test_driver_refuses_a_dark_without_a_flat(tmp_path):
    ini, d = write_set(tmp_path)
    refused(tmp_path, ini, d, ["--dark", reference(tmp_path / "dark.his", value=100)], "--dark needs --flat")


def test_driver_refuses_missing_and_empty_reference_files(tmp_path):
    ini, d = write_set(tmp_path)
    refused(tmp_path, ini, d, ["--flat", tmp_path / "nope.his"], "--flat", "nope.his", "no such file")
    empty = tmp_path / "empty.his"
    empty.write_bytes(F.his_file_bytes(np.zeros((0, GEO[1], GEO[0]), np.uint16), 4))
    refused(tmp_path, ini, d, ["--flat", empty], "--flat", "empty.his", "holds no frames")
    junk = tmp_path / "junk.his"
    junk.write_bytes(b"not a HIS file")
    refused(tmp_path, ini, d, ["--flat", reference(tmp_path / "flat.his"), "--dark", junk], "--dark", "junk.his", "holds no frames")


def test_driver_refuses_a_reference_of_another_size(tmp_path):
    ini, d = write_set(tmp_path)
    refused(tmp_path, ini, d, ["--flat", reference(tmp_path / "flat.his", shape=(GEO[1], GEO[0] + 1))], "--flat", "65 x 48",
            "detector is 64 x 48")
    refused(tmp_path, ini, d, ["--flat", reference(tmp_path / "flat2.his"), "--dark", reference(tmp_path / "dark.his", shape=(GEO[0], GEO[1]))],
            "--dark", "48 x 64", "detector is 64 x 48")


def test_driver_refuses_a_reference_inside_the_input(tmp_path):
    ini, d = write_set(tmp_path)
    inside = reference(d / "zz_flat.his")
    refused(tmp_path, ini, d, ["--flat", inside], "--flat", "lies inside --input", "read as a projection")
    sub = tmp_path / "link"
    sub.symlink_to(d)   # the same file through another path
    refused(tmp_path, ini, d, ["--flat", reference(tmp_path / "flat.his"), "--dark", sub / "zz_flat.his"], "--dark", "lies inside --input")


@pytest.mark.parametrize("t", ["0", "-1e-5", "1.5", "nan", "inf"])
def test_driver_refuses_a_min_transmission_out_of_range(tmp_path, t):
    ini, d = write_set(tmp_path)
    refused(tmp_path, ini, d, ["--flat", reference(tmp_path / "flat.his"), "--min-transmission", t], "--min-transmission", "outside (0, 1]")
