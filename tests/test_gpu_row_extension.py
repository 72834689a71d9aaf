"""Row extension for laterally truncated projections on the device (the rule is in include/paris_hip.h and
restated in tests/row_extension_rule.py). "Setting on" must equal fmaf(b, c_rev, fmaf(a, c, plain)) bit for bit, where plain is the
device's own filter without the setting, a and b are the edge means of the device's weighted rows and c comes from
row_extension_response."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import row_extension_rule as R
import test_gpu_flat_field as FF
import test_gpu_paris_hip as P
from oracle import formats as F
from paris_amd import _lib
from paris_amd import backend as B

pytestmark = pytest.mark.gpu

TAU = 0.2
W = 16
ROWS = 5   # odd: the last workgroup has no second row


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if np.asarray(a).dtype == np.float32 else np.uint16)


def geometry(dim_x, dim_y=ROWS):
    return B.DetectorGeometry(dim_x, dim_y, TAU, 0.25, 1.5, -0.75, 100, 200, 1.0)


def frame_of(dim_x, dim_y=ROWS, seed=0):
    """positive everywhere (a truncated row: the edges are far from 0), with structure"""
    rng = np.random.default_rng(dim_x * 31 + seed)
    return (1.0 + rng.random((dim_y, dim_x)) + np.sin(np.arange(dim_x) / 17.0)[None, :] * 0.5).astype(np.float32)


@pytest.fixture(scope="module")
def be():
    with B.Backend(0) as b:
        yield b


def read(be, d):
    h = be.make_projection_host(d.dim_x, d.dim_y)
    be.copy_d2h(d, h)
    return h.buf.copy()


def run(be, frame, det, stages, setting=None, variant=0):
    """frame through `stages` -- "weight", "filter" (the separate calls), "fused" (paris_hip_stage_weight_filter_rows) -- with the
    setting (m, W) in force, or none"""
    dim_y, dim_x = frame.shape
    be.set_filter_variant(variant)
    if setting is not None:
        be.set_row_extension(*setting)
    try:
        d = B.load(be, B.Projection(frame.copy(), dim_x, dim_y))
        for s in stages:
            if s == "weight":
                B.weight(be, d, det)
            elif s == "filter":
                B.filter(be, d, det)
            else:
                B.weight_filter_rows(be, d, det, 0, dim_y)
        out = read(be, d)
        be.free(d)
    finally:
        be.clear_row_extension()
        be.set_filter_variant(0)
    return out


def expected(weighted, plain, m, dim_x, w=W):
    return R.extend(weighted, plain, m, B.row_extension_response(m, w, dim_x, TAU))


def run_with_k(be, frame, n, stages, setting=None):
    """the same through the explicit entry points with a K of length n: "weight" (paris_hip_weight), "filter"
    (paris_hip_apply_filter), "fused" (paris_hip_weight_filter_rows)"""
    dim_y, dim_x = frame.shape
    f32 = np.float32
    consts = (float(f32(1.5) * f32(TAU) - f32(dim_x) * f32(TAU) / f32(2)), float(f32(-0.75) * f32(0.25) - f32(dim_y) * f32(0.25) / f32(2)),
              300.0, TAU, 0.25)   # h_min, v_min, d_sd, l_px_row, l_px_col as paris_hip_stage_weight derives them
    if setting is not None:
        be.set_row_extension(*setting)
    try:
        k = be.make_filter(n, TAU)
        d = B.load(be, B.Projection(frame.copy(), dim_x, dim_y))
        for s in stages:
            if s == "weight":
                be.weight(d, *consts)
            elif s == "filter":
                be.apply_filter(d, k, n, dim_y)
            else:
                be.weight_filter_rows(d, 0, dim_y, *consts, k, n)
        out = read(be, d)
        be.free(d)
        be.free(k)
    finally:
        be.clear_row_extension()
    return out


# ---- 1. the rule, at the shapes at which each transform length places the edge owners differently: a row of dim_x pixels in a
#      transform of n. Up to 2048 pixels n is the reference's length (dim_x <= n / 2: the upper half of the input is zero); 4100 and
#      8200 pixels in 8192 and 16384 fill more than half of the transform (the other instantiation), and 4000 / 4100 pixels in 8192
#      / 16384 are the half-empty forms of the two longest transforms ---------------------------------------------------------------

@pytest.mark.parametrize("m", R.EDGE_PIXELS)
@pytest.mark.parametrize("dim_x,n", [(300, 1024), (301, 1024), (1000, 2048), (2048, 4096), (4100, 8192), (8200, 16384), (4000, 8192),
                                     (4100, 16384)])
def test_setting_on_equals_the_update_of_plain(be, dim_x, n, m):
    frame = frame_of(dim_x)
    weighted = run_with_k(be, frame, n, ["weight"])
    plain = run_with_k(be, frame, n, ["weight", "filter"])
    want = expected(weighted, plain, m, dim_x)
    assert not np.array_equal(bits(want), bits(plain))
    separate = run_with_k(be, frame, n, ["weight", "filter"], (m, W))   # the stored pixels feed the transform
    fused = run_with_k(be, frame, n, ["fused"], (m, W))                 # the weight rides in the load
    assert np.array_equal(bits(run_with_k(be, frame, n, ["fused"])), bits(plain))
    assert np.array_equal(bits(separate), bits(want))
    assert np.array_equal(bits(fused), bits(want))


@pytest.mark.parametrize("dim_x,variant", [(100, 0), (300, 1), (301, 1)])
def test_the_radix_2_kernel(be, dim_x, variant):
    det = geometry(dim_x)
    frame = frame_of(dim_x)
    weighted = run(be, frame, det, ["weight"])
    plain = run(be, frame, det, ["weight", "filter"], variant=variant)
    for m in (1, 8):
        got = run(be, frame, det, ["weight", "filter"], (m, W), variant=variant)
        assert np.array_equal(bits(got), bits(expected(weighted, plain, m, dim_x)))
        # the stage form for a band takes the two-stage route on this path: the same bits
        assert np.array_equal(bits(run(be, frame, det, ["fused"], (m, W), variant=variant)), bits(got))


@pytest.mark.parametrize("dim_x", [4, 8])
def test_rows_of_exactly_edge_pixels(be, dim_x):
    """dim_x == m: both means are taken over the same pixels (the radix-2 kernel; no detector this narrow reaches the other)"""
    det = geometry(dim_x)
    frame = frame_of(dim_x)
    weighted = run(be, frame, det, ["weight"])
    plain = run(be, frame, det, ["weight", "filter"])
    got = run(be, frame, det, ["weight", "filter"], (dim_x, W))
    assert np.array_equal(bits(got), bits(expected(weighted, plain, dim_x, dim_x)))
    be.set_row_extension(8, W)
    try:
        d = B.load(be, B.Projection(frame_of(4), 4, ROWS))
        with pytest.raises(B.ParisHipError) as e:   # dim_x < m
            B.filter(be, d, geometry(4))
        assert e.value.status == _lib.ERROR_INVALID_ARGUMENT
        be.free(d)
    finally:
        be.clear_row_extension()


def test_long_tapers(be):
    """a taper longer than the row, and the longest one: c has no wrap to get wrong"""
    dim_x = 300
    det = geometry(dim_x)
    frame = frame_of(dim_x)
    weighted = run(be, frame, det, ["weight"])
    plain = run(be, frame, det, ["weight", "filter"])
    for w in (700, R.TAPER_MAX):
        got = run(be, frame, det, ["fused"], (2, w))
        assert np.array_equal(bits(got), bits(expected(weighted, plain, 2, dim_x, w)))


@pytest.mark.parametrize("dim_x", [300, 2048])
def test_rows_with_zero_edges_stay_bit_identical_to_plain(be, dim_x):
    det = geometry(dim_x)
    frame = frame_of(dim_x)
    frame[:, :8] = 0
    frame[:, -8:] = 0
    frame[1, 0] = 0.5      # ... but one row's left edge and another's right edge are not
    frame[3, -1] = 0.25
    plain = run(be, frame, det, ["fused"])
    got = run(be, frame, det, ["fused"], (8, W))
    same = [np.array_equal(bits(got[r]), bits(plain[r])) for r in range(ROWS)]
    assert same == [True, False, True, False, True]
    weighted = run(be, frame, det, ["weight"])
    assert np.array_equal(bits(got), bits(expected(weighted, plain, 8, dim_x)))


# ---- 2. the other outputs and groupings of the filter ---------------------------------------------------------------------------

@pytest.mark.parametrize("dim_x", [300, 2048])
def test_half_precision_output(be, dim_x):
    det = geometry(dim_x)
    frame = frame_of(dim_x)
    weighted = run(be, frame, det, ["weight"])
    plain = run(be, frame, det, ["weight", "filter"])
    want = expected(weighted, plain, 4, dim_x).astype(np.float16)   # rounded to nearest even
    be.set_row_extension(4, W)
    try:
        d = B.load(be, B.Projection(frame.copy(), dim_x, ROWS))
        half_pitch = (dim_x * 2 + 255) // 256 * 256
        half = be.make_projection_device(half_pitch // 4, ROWS)
        B.weight_filter_rows(be, d, det, 0, ROWS, half.ptr, half_pitch)
        raw = read(be, half).view(np.float16).reshape(ROWS, -1)[:, :dim_x]
        assert np.array_equal(bits(read(be, d)), bits(frame))   # the fp32 rows stay as they were
        assert np.array_equal(bits(raw), bits(want))
        be.free(d)
        be.free(half)
    finally:
        be.clear_row_extension()


@pytest.mark.parametrize("dim_x", [300, 100])
def test_a_band_equals_the_same_rows_of_the_whole_frame(be, dim_x):
    det = geometry(dim_x, 6)
    frame = frame_of(dim_x, 6)
    whole = run(be, frame, det, ["fused"], (4, W))
    be.set_row_extension(4, W)
    try:
        d = B.load(be, B.Projection(frame.copy(), dim_x, 6))
        B.weight_filter_rows(be, d, det, 2, 2)   # whole row pairs: the transform packs rows (2t, 2t + 1) as one complex signal
        got = read(be, d)
        be.free(d)
    finally:
        be.clear_row_extension()
    assert np.array_equal(bits(got[2:4]), bits(whole[2:4]))
    assert np.array_equal(bits(got[:2]), bits(frame[:2])) and np.array_equal(bits(got[4:]), bits(frame[4:]))


@pytest.mark.parametrize("dim_x", [300, 100])
def test_a_three_frame_batch_equals_three_single_calls(be, dim_x):
    det = geometry(dim_x)
    frames = [frame_of(dim_x, seed=k) for k in range(3)]
    singles = [run(be, f, det, ["fused"], (2, W)) for f in frames]
    be.set_row_extension(2, W)
    try:
        d = be.make_projection_device(dim_x, 3 * ROWS)   # three frames one behind the other
        be.copy_h2d(B.Projection(np.concatenate(frames), dim_x, 3 * ROWS), d)
        B.weight_filter_batch(be, d.ptr, d.pitch, d.pitch * ROWS, 3, dim_x, ROWS, det, 0, ROWS)
        got = read(be, d).reshape(3, ROWS, dim_x)
        be.free(d)
    finally:
        be.clear_row_extension()
    for k in range(3):
        assert np.array_equal(bits(got[k]), bits(singles[k])), k


# ---- 3. deferral, ordering and the setting's lifecycle --------------------------------------------------------------------------

def volume_to_host(abe, v, vg):
    h = abe.make_volume_host(vg.dim_x, vg.dim_y, vg.dim_z)
    abe.copy_d2h(v, h)
    return h.buf.copy()


def loop_volume(det, vg, frames, setting, mode):
    """PARIS's loop; mode: "immediate", "snapshots" (filter deferral into the ring) or "references" (in place, the frame_tab launch)"""
    with B.Backend(0, synchronous=False) as abe:
        if mode == "references":
            abe.set_paris_loop_defaults(8)
        elif mode == "snapshots":
            abe.set_paris_loop_defaults(8)
            abe.set_backproject_references(False)
            abe.set_filter_deferral(1)
        if setting is not None:
            abe.set_row_extension(*setting)
        v = abe.make_volume_device(vg.dim_x, vg.dim_y, vg.dim_z)
        for i, fr in enumerate(frames):
            d_p = B.load(abe, B.Projection(fr.copy(), det.n_row, det.n_col, idx=i))
            B.weight(abe, d_p, det)
            B.filter(abe, d_p, det)
            B.backproject(abe, d_p, v, 0, det, vg, False, False, None)
            abe.free(d_p)
        abe.flush()
        return volume_to_host(abe, v, vg)


@pytest.mark.parametrize("mode", ["snapshots", "references"])
def test_filter_deferral_gives_the_volume_of_the_immediate_path(mode):
    det = B.DetectorGeometry(300, 12, TAU, 0.25, 1.5, -0.75, 100, 200, 15.0)
    vg = B.calculate_volume_geometry(det)
    vg.dim_x = vg.dim_y = 40   # a few tiles are enough: the filter is what is compared
    vg.dim_z = 8
    frames = [frame_of(300, 12, seed=k) for k in range(20)]
    want = loop_volume(det, vg, frames, (4, W), "immediate")
    plain = loop_volume(det, vg, frames, None, "immediate")
    assert np.abs(want).max() > 0 and not np.array_equal(bits(want), bits(plain))
    assert np.array_equal(bits(loop_volume(det, vg, frames, (4, W), mode)), bits(want))


def test_set_and_clear_between_a_held_back_filter_and_its_launch():
    """the held rows get the setting that was in force when they were queued"""
    dim_x = 300
    det = geometry(dim_x, 6)
    frame = frame_of(dim_x, 6)
    with B.Backend(0) as sbe:
        plain = run(sbe, frame, det, ["fused"])
        extended = run(sbe, frame, det, ["fused"], (4, W))
    assert not np.array_equal(bits(plain), bits(extended))
    for first_on in (False, True):
        with B.Backend(0, synchronous=False) as abe:
            abe.set_paris_loop_defaults(8)
            if first_on:
                abe.set_row_extension(4, W)
            d = B.load(abe, B.Projection(frame.copy(), dim_x, 6))
            B.weight(abe, d, det)    # held back
            B.filter(abe, d, det)    # held back with it (filter deferral)
            if first_on:
                abe.clear_row_extension()
            else:
                abe.set_row_extension(4, W)
            got = read(abe, d)
            assert np.array_equal(bits(got), bits(extended if first_on else plain)), first_on
            # ... and the next frame gets the new one
            e = B.load(abe, B.Projection(frame.copy(), dim_x, 6))
            B.weight(abe, e, det)
            B.filter(abe, e, det)
            assert np.array_equal(bits(read(abe, e)), bits(plain if first_on else extended)), first_on
            abe.free(d)
            abe.free(e)


def test_a_foreign_filter_is_unsupported_and_refusals(be):
    dim_x, fs = 300, 1024
    det = geometry(dim_x)
    k = be.make_filter(fs, TAU)
    host_k = be.filter_to_host(k)
    foreign = be.make_projection_device(fs // 2 + 1, 1)   # the same values in memory this ctx did not make as a K
    be.copy_h2d(B.Projection(host_k.reshape(1, -1).copy(), fs // 2 + 1, 1), foreign)
    d = B.load(be, B.Projection(frame_of(dim_x), dim_x, ROWS))
    L = be._L
    assert L.paris_hip_apply_filter(be._ctx, d.ptr, d.pitch, dim_x, ROWS, foreign.ptr, fs, ROWS) == 0   # no setting: the radix-2 kernel
    assert L.paris_hip_set_row_extension(be._ctx, None) == _lib.ERROR_INVALID_ARGUMENT
    assert L.paris_hip_set_row_extension(None, C.byref(_lib.RowExtension(4, W))) == _lib.ERROR_INVALID_ARGUMENT
    assert L.paris_hip_set_row_extension(be._ctx, C.byref(_lib.RowExtension(3, W))) == _lib.ERROR_INVALID_ARGUMENT
    assert L.paris_hip_set_row_extension(be._ctx, C.byref(_lib.RowExtension(4, 0))) == _lib.ERROR_INVALID_ARGUMENT
    assert L.paris_hip_clear_row_extension(None) == _lib.ERROR_INVALID_ARGUMENT
    be.clear_row_extension()   # clearing nothing is fine
    be.set_row_extension(4, W)
    try:
        before = read(be, d)
        assert L.paris_hip_apply_filter(be._ctx, d.ptr, d.pitch, dim_x, ROWS, foreign.ptr, fs, ROWS) == _lib.ERROR_UNSUPPORTED
        assert np.array_equal(bits(read(be, d)), bits(before))   # a refused call filters nothing
        assert L.paris_hip_apply_filter(be._ctx, d.ptr, d.pitch, dim_x, ROWS, k.ptr, fs, ROWS) == 0
    finally:
        be.clear_row_extension()
    for o in (d, foreign, k):
        be.free(o)


def test_reserve_bytes_grow_by_the_cached_vectors_and_shrink_again(be):
    before = be.projection_reserve_bytes(300, ROWS)
    be.set_row_extension(4, W)
    try:
        assert be.projection_reserve_bytes(300, ROWS) == before   # nothing cached yet
        run_det = geometry(300)
        d = B.load(be, B.Projection(frame_of(300), 300, ROWS))
        B.weight_filter_rows(be, d, run_det, 0, ROWS)
        assert be.projection_reserve_bytes(300, ROWS) == before + 4 * 300
        B.weight_filter_rows(be, d, run_det, 0, ROWS)             # the same vector again
        assert be.projection_reserve_bytes(300, ROWS) == before + 4 * 300
        e = B.load(be, B.Projection(frame_of(100), 100, ROWS))
        B.weight(be, e, geometry(100))
        B.filter(be, e, geometry(100))                            # another width: another vector
        assert be.projection_reserve_bytes(300, ROWS) == before + 4 * 300 + 4 * 100
        be.set_row_extension(2, W)                                # replaced: the old vectors go
        assert be.projection_reserve_bytes(300, ROWS) == before
        be.free(d)
        be.free(e)
    finally:
        be.clear_row_extension()
    assert be.projection_reserve_bytes(300, ROWS) == before


# ---- 4. the driver and the C++ mirror against the Python mirror ------------------------------------------------------------------

def test_driver_and_cpp_mirror_against_the_python_mirror(tmp_path):
    det = B.DetectorGeometry(*FF.DRV_GEO)
    vg = B.calculate_volume_geometry(det)
    n_row, n_col = FF.DRV_GEO[:2]
    n_frames = 75
    rng = np.random.default_rng(9)
    fr = rng.integers(500, 3000, (n_frames, n_col, n_row)).astype(np.uint16)   # line integrals, nonzero at both edges
    counts_dir = tmp_path / "counts"
    counts_dir.mkdir()
    (counts_dir / "a.his").write_bytes(F.his_file_bytes(fr[:70], 4, 32))
    (counts_dir / "b.his").write_bytes(F.his_file_bytes(fr[70:], 4, 32))
    geo = tmp_path / "geo.ini"
    geo.write_text("\n".join("%s = %s" % kv for kv in zip(FF.GEO_KEYS, FF.DRV_GEO)) + "\n")

    def mirror(setting):
        with B.Backend(0) as mbe:
            if setting is not None:
                mbe.set_row_extension(*setting)
            v = mbe.make_volume_device(vg.dim_x, vg.dim_y, vg.dim_z)
            for i, f in enumerate(fr):
                d_p = B.load(mbe, B.Projection(f.astype(np.float32), n_row, n_col, idx=i))
                B.weight(mbe, d_p, det)
                B.filter(mbe, d_p, det)
                B.backproject(mbe, d_p, v, 0, det, vg, False, False, None)
                mbe.free(d_p)
            return volume_to_host(mbe, v, vg).reshape(vg.dim_z, vg.dim_y, vg.dim_x)

    want, plain = mirror((4, 16)), mirror(None)
    assert np.abs(want).max() > 0 and not np.array_equal(bits(want), bits(plain))
    base = [P.EXE, "--geometry", geo, "--input", counts_dir]
    for k, extra in enumerate((["--slabs", 1], ["--slabs", 3])):
        o = tmp_path / ("o%d" % k)
        r = subprocess.run([str(a) for a in base + ["--output", o, "--extend-rows", "16:4"] + extra], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "row extension on: cos^2 taper of 16 pixel(s), mean of 4 edge pixel(s)" in r.stdout, r.stdout
        assert np.array_equal(bits(F.ddbvf_read(str(o / "vol.ddbvf"))[1]), bits(want)), extra
    o = tmp_path / "default_m"   # M defaults to 4
    r = subprocess.run([str(a) for a in base + ["--output", o, "--extend-rows", "16"]], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and np.array_equal(bits(F.ddbvf_read(str(o / "vol.ddbvf"))[1]), bits(want))
    # refused with exit status 1 before any output exists
    for bad in ("abc", "16:", ":4", "16:3", "0", "16385", "16:128", "-16", "16:4:1", "1.5"):
        r = subprocess.run([str(a) for a in base + ["--output", tmp_path / "bad", "--extend-rows", bad]], capture_output=True, text=True,
                           timeout=300)
        assert r.returncode == 1 and "--extend-rows" in r.stderr, (bad, r.stderr)
    assert not (tmp_path / "bad").exists()
    # PARIS's loop through paris::hip with set_row_extension (paris_hip_demo --extend-rows W M)
    raw = tmp_path / "in.raw"
    fr.astype(np.float32).tofile(raw)
    out = tmp_path / "demo.raw"
    r = subprocess.run([FF.DEMO] + [str(v) for v in FF.DRV_GEO] + [str(n_frames), str(raw), str(out), "--slabs", "2", "--extend-rows", "16", "4"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr + r.stdout
    assert np.array_equal(bits(np.fromfile(out, np.float32).reshape(want.shape)), bits(want))


# ---- 5. quality -----------------------------------------------------------------------------------------------------------------

def test_quality_of_a_truncated_reconstruction():
    """Relative RMS against an FDK reconstruction from a detector three times as wide in the same grid: 64 x 48 driver geometry, a head
    phantom 1.6 x as wide as the grid, 360 views, inside 0.85 of the field-of-view radius on the central half of the slices. The oracle
    with the numpy rule (tests/test_row_extension_host.py): 0.4737 zero-padded, 0.06415 with taper 16 / 4 edge pixels; the device
    differs from it only by the row filter's FFT rounding."""
    det = B.DetectorGeometry(*R.QUALITY_GEO)
    wide = B.DetectorGeometry(*R.wide_geo())
    vg = B.calculate_volume_geometry(det)
    region = R.quality_region((vg.dim_z, vg.dim_y, vg.dim_x), vg.l_vx_x)

    def reconstruct(d, frames, setting):
        with B.Backend(0, synchronous=False) as qbe:
            qbe.set_paris_loop_defaults(48)
            if setting is not None:
                qbe.set_row_extension(*setting)
            v = qbe.make_volume_device(vg.dim_x, vg.dim_y, vg.dim_z)
            for i, fr in enumerate(frames):
                d_p = qbe.make_projection_device(d.n_row, d.n_col)
                qbe.upload_raw(fr, d_p)
                d_p.idx = i
                B.weight(qbe, d_p, d)
                B.filter(qbe, d_p, d)
                B.backproject(qbe, d_p, v, 0, d, vg, False, False, None)
                qbe.free(d_p)
            qbe.flush()
            return volume_to_host(qbe, v, vg).reshape(vg.dim_z, vg.dim_y, vg.dim_x)

    truth = reconstruct(wide, R.quality_frames(vg.dim_x, vg.l_vx_x, R.TRUNCATED_RADIUS, wide=True), None)
    frames = R.quality_frames(vg.dim_x, vg.l_vx_x, R.TRUNCATED_RADIUS)
    zero = R.relative_rms(reconstruct(det, frames, None), truth, region)
    ext = R.relative_rms(reconstruct(det, frames, (4, R.QUALITY_TAPER)), truth, region)
    print("row extension quality: relative RMS %.5g zero-padded, %.5g with taper %d / 4 edge pixels" % (zero, ext, R.QUALITY_TAPER))
    assert ext < zero
    assert ext <= R.BOUND * R.CAL_EXTENDED_4
