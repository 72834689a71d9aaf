"""The host side of the metal artefact reduction (paris_hip_metal_check, paris_hip_metal_collect_host, paris_hip_metal_trace_pack_host,
paris_hip_metal_inpaint_host): no device, no ctx -- the library's rules against their numpy restatement
(tests/metal_rule.py) bit for bit on the rows the rule distinguishes, every refusal, the wrong restatements that show the comparisons
can fail, and the float64 scene that makes the GPU's physical check honest."""
import ctypes as C

import numpy as np
import pytest

import metal_rule as R
from paris_amd import _lib
from paris_amd import backend as B

INV = _lib.ERROR_INVALID_ARGUMENT


# ---- the restatement's own pieces ---------------------------------------------------------------------------------------------------

def test_the_packed_layout():
    m = np.zeros((2, 130), bool)
    m[0, [0, 63, 64, 129]] = True
    m[1, 65] = True
    b = R.pack_bits(m)
    assert b.dtype == np.uint64 and b.shape == (2, 3)
    assert [int(x) for x in b[0]] == [1 | 1 << 63, 1, 2] and [int(x) for x in b[1]] == [0, 2, 0]
    assert np.array_equal(R.unpack_bits(b, 130), m)
    assert R.words(1) == 1 and R.words(64) == 1 and R.words(65) == 2 and B.metal_words(130) == 3


def test_runs_of_a_row():
    assert R.runs_of([0, 1, 1, 0, 1]) == [(1, 2), (4, 4)]
    assert R.runs_of([1, 1, 1]) == [(0, 2)] and R.runs_of([0, 0]) == []


# ---- the inpainting ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim_x", R.DIM_XS)
def test_inpaint_host_matches_the_rule_on_the_special_rows(dim_x):
    p, m = R.special_rows(dim_x)
    want, counts = R.inpaint(p, m)
    got, st = B.metal_inpaint_host(p, R.pack_bits(m))
    assert R.same_pixels(got, want)
    assert R.counts_tuple(st) == counts
    outside = ~m
    assert np.array_equal(R.f32_bits(got)[outside], R.f32_bits(p)[outside])           # pixels outside the trace keep their bits
    whole = m.all(axis=1)
    assert np.array_equal(R.f32_bits(got)[whole], R.f32_bits(p)[whole]) and counts[2] == int(whole.sum())


def test_inpaint_host_values_by_hand():
    p = np.array([[1.0, 9.0, 9.0, 9.0, 3.0, 9.0, 7.0]], np.float32)
    m = np.array([[0, 1, 1, 1, 0, 1, 0]], bool)
    got, st = B.metal_inpaint_host(p, R.pack_bits(m))
    assert got.tolist() == [[1.0, 1.5, 2.0, 2.5, 3.0, 5.0, 7.0]] and R.counts_tuple(st) == (4, 2, 0)
    m = np.array([[1, 1, 0, 0, 0, 1, 1]], bool)
    got, st = B.metal_inpaint_host(p, R.pack_bits(m))
    assert got.tolist() == [[9.0, 9.0, 9.0, 9.0, 3.0, 3.0, 3.0]] and R.counts_tuple(st) == (4, 2, 0)
    nan = np.float32(np.nan)
    p = np.array([[np.inf, 0, 0, np.inf, 0, nan, 5.0, 0, 2.0]], np.float32)
    m = np.array([[0, 1, 1, 0, 0, 1, 0, 1, 0]], bool)
    got, _ = B.metal_inpaint_host(p, R.pack_bits(m))
    assert np.isnan(got[0, 1:3]).all()                                                  # inf - inf
    assert got[0, 5] == 2.5 and got[0, 7] == 3.5                                        # a NaN inside a run goes away


def test_inpaint_host_bands_and_counts_accumulate():
    p, m = R.special_rows(130)
    bits = R.pack_bits(m)
    rows = p.shape[0]
    want, counts = R.inpaint(p, m, 3, rows - 5)
    got, st = B.metal_inpaint_host(p, bits, 3, rows - 5)
    assert R.same_pixels(got, want) and R.counts_tuple(st) == counts
    assert np.array_equal(R.f32_bits(got[:3]), R.f32_bits(p[:3])) and np.array_equal(R.f32_bits(got[-2:]), R.f32_bits(p[-2:]))
    got, st = B.metal_inpaint_host(p, bits, 4, 0)                                       # an empty band
    assert np.array_equal(R.f32_bits(got), R.f32_bits(p)) and R.counts_tuple(st) == (0, 0, 0)
    L, st, a = _lib.load(), _lib.MetalCounts(5, 6, 7), p.copy()
    assert L.paris_hip_metal_inpaint_host(a.ctypes.data, bits.ctypes.data, 130, rows, 0, rows, C.byref(st)) == _lib.SUCCESS
    full = R.inpaint(p, m)[1]
    assert R.counts_tuple(st) == (5 + full[0], 6 + full[1], 7 + full[2])
    assert L.paris_hip_metal_inpaint_host(a.ctypes.data, bits.ctypes.data, 130, rows, 0, rows, None) == _lib.SUCCESS
    assert L.paris_hip_metal_inpaint_host(a.ctypes.data, bits.ctypes.data, 130, rows, rows, 1, None) == INV
    assert L.paris_hip_metal_inpaint_host(a.ctypes.data, bits.ctypes.data, 130, rows, rows + 1, 0, None) == INV
    assert L.paris_hip_metal_inpaint_host(None, bits.ctypes.data, 130, rows, 0, 1, None) == INV
    assert L.paris_hip_metal_inpaint_host(a.ctypes.data, None, 130, rows, 0, 1, None) == INV
    assert L.paris_hip_metal_inpaint_host(None, None, 130, rows, 0, 0, None) == _lib.SUCCESS


@pytest.mark.parametrize("wrong", R.WRONG_INPAINT)
def test_every_wrong_inpainting_is_told_apart(wrong):
    differs = 0
    for dim_x in R.DIM_XS:
        p, m = R.special_rows(dim_x)
        got, _ = B.metal_inpaint_host(p, R.pack_bits(m))
        differs += not R.same_pixels(got, R.inpaint(p, m, wrong=wrong)[0])
    assert differs >= 3, wrong


# ---- the trace -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("grow", (0, 1, 4))
@pytest.mark.parametrize("shape", ((9, 70), (1, 1), (3, 64), (2, 65), (12, 130)))
def test_pack_host_matches_the_rule(shape, grow):
    t = R.corner_frames(shape[1], shape[0])
    got = B.metal_trace_pack_host(t, 1.0, grow)
    want = R.pack(t, 1.0, grow)
    assert got.shape == want.shape == (4, shape[0], R.words(shape[1])) and np.array_equal(got, want)
    if shape == (9, 70) and grow == 4:                                                  # the corners' windows are clipped to the frame
        tr = R.unpack_bits(got, 70)
        assert tr[0, :, :5].all() and tr[0, :, -5:].all() and tr[0].sum() == 9 * 10   # (rows 0 .. 4 and 4 .. 8: the windows meet)
    if shape == (9, 70) and grow == 0:                                                  # NaN, inf, at and above the threshold
        tr = R.unpack_bits(got, 70)
        assert not tr[2, 2, 2] and tr[2, 4, 5] and not tr[2, 6, 7] and tr[2, 6, 20] and tr[2].sum() == 2


def test_every_wrong_trace_is_told_apart():
    t = R.corner_frames()
    for grow in (1, 4):
        assert not np.array_equal(B.metal_trace_pack_host(t, 1.0, grow), R.pack(t, 1.0, grow, wrong=R.WRONG_PACK[0]))
    assert np.array_equal(B.metal_trace_pack_host(t, 1.0, 0), R.pack(t, 1.0, 0, wrong=R.WRONG_PACK[0]))  # (no grow: nothing to get wrong)


def test_pack_host_refusals():
    L, t, out = _lib.load(), np.zeros((2, 3), np.float32), np.zeros(2, np.uint64)
    assert L.paris_hip_metal_trace_pack_host(t.ctypes.data, 1, 3, 2, 0.5, 5, out.ctypes.data) == INV
    assert L.paris_hip_metal_trace_pack_host(t.ctypes.data, 1, 3, 2, -0.5, 0, out.ctypes.data) == INV
    assert L.paris_hip_metal_trace_pack_host(t.ctypes.data, 1, 3, 2, float("nan"), 0, out.ctypes.data) == INV
    assert L.paris_hip_metal_trace_pack_host(t.ctypes.data, 1, 3, 2, float("inf"), 0, out.ctypes.data) == INV
    assert L.paris_hip_metal_trace_pack_host(None, 1, 3, 2, 0.5, 0, out.ctypes.data) == INV
    assert L.paris_hip_metal_trace_pack_host(t.ctypes.data, 1, 3, 2, 0.5, 0, None) == INV
    assert L.paris_hip_metal_trace_pack_host(None, 0, 3, 2, 0.5, 0, None) == _lib.SUCCESS
    assert L.paris_hip_metal_trace_pack_host(t.ctypes.data, 1, 3, 2, 0.0, 4, out.ctypes.data) == _lib.SUCCESS


# ---- the list ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", ((3, 5, 67), (9, 129, 130), (1, 1, 1)))
def test_collect_host_matches_the_rule(shape):
    v = R.hit_volume(shape, 0.75)
    index, value = R.collect(v, 0.75)
    assert np.array_equal(index, np.flatnonzero(np.nan_to_num(v.ravel(), nan=-1.0) > np.float32(0.75)))
    got_i, got_v, mask = B.metal_collect_host(v, 0.75, max_n=v.size, binarize=True)
    assert got_i.dtype == np.uint64 and np.array_equal(got_i, index) and np.array_equal(R.f32_bits(got_v), R.f32_bits(value))
    assert np.array_equal(R.f32_bits(mask), R.f32_bits(R.binarized(v, 0.75)))
    assert B.metal_collect_host(v, 0.75, max_n=v.size)[2] is None
    if v.size > 1:
        assert np.isinf(got_v).any() and not np.isnan(got_v).any()                      # +inf is a hit; NaN and -inf are not


def test_collect_host_cap_and_empty_result():
    v = R.hit_volume((3, 5, 67), 0.75)
    n = len(R.collect(v, 0.75)[0])
    L = _lib.load()
    for max_n, status in ((n, _lib.SUCCESS), (n + 1, _lib.SUCCESS), (n - 1, _lib.ERROR_METAL_TOO_MANY_VOXELS), (0, _lib.ERROR_METAL_TOO_MANY_VOXELS)):
        a = v.copy()
        index, value, count = np.full(n + 2, 77, np.uint64), np.full(n + 2, 77.0, np.float32), C.c_uint64(0)
        assert L.paris_hip_metal_collect_host(a.ctypes.data, 67, 5, 3, 0.75, max_n, index.ctypes.data, value.ctypes.data, C.byref(count), 1) == status
        assert count.value == n
        if status != _lib.SUCCESS:                                                      # nothing written: neither the lists nor the volume
            assert (index == 77).all() and (value == 77.0).all() and np.array_equal(R.f32_bits(a), R.f32_bits(v))
        else:
            assert (index[n:] == 77).all() and np.array_equal(R.f32_bits(a), R.f32_bits(R.binarized(v, 0.75)))
    with pytest.raises(B.ParisHipError) as e:
        B.metal_collect_host(v, 0.75, max_n=n - 1)
    assert e.value.status == _lib.ERROR_METAL_TOO_MANY_VOXELS and e.value.n == n and b"more voxels" in L.paris_hip_strerror(e.value.status)
    index, value, _ = B.metal_collect_host(v, 1e6)                                      # only +inf is above it
    assert len(index) == 1 and np.isinf(value[0])
    index, value, mask = B.metal_collect_host(np.zeros((2, 3, 4), np.float32), 0.5, binarize=True)
    assert len(index) == 0 and len(value) == 0 and not mask.any()
    count = C.c_uint64(9)
    a = np.zeros(4, np.float32)
    assert L.paris_hip_metal_collect_host(a.ctypes.data, 4, 1, 1, 0.5, 0, None, None, C.byref(count), 0) == _lib.SUCCESS and count.value == 0
    assert L.paris_hip_metal_collect_host(None, 4, 1, 1, 0.5, 0, None, None, C.byref(count), 0) == INV
    assert L.paris_hip_metal_collect_host(a.ctypes.data, 4, 1, 1, 0.5, 0, None, None, None, 0) == INV
    assert L.paris_hip_metal_collect_host(a.ctypes.data, 4, 1, 1, 0.5, 1, None, None, C.byref(count), 0) == INV
    assert L.paris_hip_metal_collect_host(a.ctypes.data, 4, 0, 1, 0.5, 0, None, None, C.byref(count), 0) == INV
    assert L.paris_hip_metal_collect_host(a.ctypes.data, 4, 1, 1, float("nan"), 0, None, None, C.byref(count), 0) == INV


def test_reinsert_rule():
    v = np.zeros((4, 3, 5), np.float32)
    index, value = np.array([0, 14, 15, 44, 59], np.uint64), np.array([1, 2, 3, 4, 5], np.float32)
    whole = R.reinsert(v, index, value)
    assert whole.reshape(-1)[[0, 14, 15, 44, 59]].tolist() == [1, 2, 3, 4, 5] and np.count_nonzero(whole) == 5
    slab = R.reinsert(v[1:3], index, value, v_offset=1)
    assert np.array_equal(slab, whole[1:3])


# ---- the check -----------------------------------------------------------------------------------------------------------------------

def test_metal_check_cap_and_refusals():
    assert B.metal_check(64, 64, 24, 0.3, 1, 0.25) == 64 * 64 * 24 // 32 == R.voxel_cap(64, 64, 24)
    assert B.metal_check(8, 8, 8, -1.0) == 1024 == R.voxel_cap(8, 8, 8)
    assert B.metal_check(2048, 2048, 2048, 0.0, 4, 0.0) == 2 ** 28
    L = _lib.load()
    assert L.paris_hip_metal_check(4, 4, 4, 0.5, 0, 0.0, None) == _lib.SUCCESS
    for args in ((0, 4, 4, 0.5, 0, 0.0), (4, 0, 4, 0.5, 0, 0.0), (4, 4, 0, 0.5, 0, 0.0), (4, 4, 4, float("nan"), 0, 0.0),
                 (4, 4, 4, float("inf"), 0, 0.0), (4, 4, 4, 0.5, 5, 0.0), (4, 4, 4, 0.5, 0, -0.25), (4, 4, 4, 0.5, 0, float("nan")),
                 (4, 4, 4, 0.5, 0, float("inf"))):
        with pytest.raises(B.ParisHipError) as e:
            B.metal_check(*args)
        assert e.value.status == INV, args


# ---- the float64 scene -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("clip,threshold", R.SCENE_CASES)
def test_the_remedy_works_on_the_float64_scene(clip, threshold):
    """What the GPU's physical check relies on, pinned on the float64 model: with the line integrals clipped the trace covers every
    clipped pixel of every view, and the soft-tissue RMS error against the phantom falls to at most SCENE_BOUND of what it was
    (measured: 0.068 at clip 3.0 / threshold 0.3, 0.100 at clip 2.0 / threshold 0.25)."""
    det, vg = B.DetectorGeometry(*R.SCENE_DET), B.VolumeGeometry(*R.SCENE_GRID)
    full, frames = R.scene_frames(), R.scene_frames(clip)
    assert (full > clip).any(axis=(1, 2)).all()                                         # every view is clipped somewhere
    first, final, index, tr = R.reduce64(frames, det, vg, threshold)
    assert 0 < len(index) <= R.voxel_cap(vg.dim_x, vg.dim_y, vg.dim_z)
    assert tr[full > clip].all()
    truth = R.scene_truth(vg)
    soft = R.soft_tissue(truth, index)
    assert soft.sum() > 20000
    before, after = R.rms_error(first, truth, soft), R.rms_error(final, truth, soft)
    print("clip %.1f: soft-tissue rms %.5f -> %.5f, ratio %.4f" % (clip, before, after, after / before))
    assert after <= R.SCENE_BOUND * before
    assert np.array_equal(R.f32_bits(final.reshape(-1)[index.astype(np.int64)]), R.f32_bits(R.collect(first, threshold)[1]))
