"""The beam-hardening fit on the device (paris_hip_bh_classify, paris_hip_bh_gram, Backend.fit_beam_hardening; DESIGN.md section
4.17): the labels byte for byte against the numpy restatement (tests/beam_hardening_rule.py), the Gram sums bit for bit against the
library's host function, and the whole fit on a polychromatic scan of a homogeneous object, judged by the flatness it restores."""
import ctypes as C
import math

import numpy as np
import pytest

import beam_hardening_rule as R
from paris_amd import _lib
from paris_amd import backend as B
from test_beam_hardening_host import gram_case

pytestmark = pytest.mark.gpu

TILE = (32, 16, 8)      # the classify kernel's tile (x, y, z): 37 x 35 x 11 crosses it in every axis


@pytest.fixture(scope="module")
def be():
    with B.Backend(0) as b:
        yield b


def to_device(be, a):
    a = np.ascontiguousarray(a, np.float32)
    h = B.Volume(a, a.shape[2], a.shape[1], a.shape[0])
    d = be.make_volume_device(h.dim_x, h.dim_y, h.dim_z)
    be.copy_h2d(h, d)
    return d


def classified(be, d_v, thr, margin):
    lab = be.bh_classify(d_v, thr, margin)
    got = be.labels_to_host(lab)
    be.free(lab)
    return got


# ---- the labels -----------------------------------------------------------------------------------------------------------------------

THR = np.float32(0.375)


def slab(dim_x, dim_y, dim_z, seed=0):
    """a block of object in noisy air, large enough to keep a core at margin 4, with voxels exactly at the threshold on both sides of
    the block's faces, a NaN with a payload inside the core and an infinity in the air"""
    rng = np.random.default_rng(seed)
    v = rng.uniform(0.0, 0.3, (dim_z, dim_y, dim_x)).astype(np.float32)
    x0, x1, y0, y1 = dim_x // 4, dim_x - dim_x // 6, 2, dim_y - 2
    v[:, y0:y1, x0:x1] = rng.uniform(0.45, 1.0, (dim_z, y1 - y0, x1 - x0)).astype(np.float32)
    v[:, y0, x0:x1:2] = THR                                   # at the threshold: air (v <= thr), so the face is ragged
    v[:, y1, x0:x1:3] = THR
    v[:, y0 + 1, x0 + 1] = np.nextafter(THR, np.float32(1))   # the next float above: object
    v[dim_z // 2, dim_y // 2, dim_x // 2 + 6] = np.nan
    v.view(np.uint32)[dim_z // 2, dim_y // 2, dim_x // 2 + 6] = R.NAN_PAYLOAD
    v[0, 0, dim_x // 2] = np.inf
    v[dim_z - 1, dim_y // 2, dim_x // 2] = -np.inf
    return v


@pytest.mark.parametrize("margin", [0, 1, 4])
@pytest.mark.parametrize("shape", [(19, 17, 11), (37, 35, 11)])
def test_labels_equal_the_restatement_byte_for_byte(be, shape, margin):
    assert shape == (19, 17, 11) or all(s > t for s, t in zip(shape, TILE))
    v = slab(*shape, seed=margin)
    assert np.count_nonzero(v == THR) > 10
    want = R.labels(v, THR, margin)
    assert (want == 2).any() and (want == 0).any() and ((want == 1).any() or margin == 4)   # (the small slab has no air 9 voxels wide)
    d_v = to_device(be, v)
    lab = be.bh_classify(d_v, THR, margin)
    got = be.labels_to_host(lab)
    assert got.shape == want.shape and np.array_equal(got, want), (shape, margin)
    if margin:
        assert not np.array_equal(got, R.PERTURBATIONS["margin in x and y only"](v, THR, margin))     # the comparison can fail
    # into labels the caller made, over what they held
    be.bh_classify(d_v, np.nextafter(THR, np.float32(0)), margin, labels=lab)
    assert np.array_equal(be.labels_to_host(lab), R.labels(v, np.nextafter(THR, np.float32(0)), margin))
    be.free(lab)
    be.free(d_v)


def test_the_field_of_view_and_the_slab_faces(be):
    """a slab of object only: at margin 0 the labels are the field of view; at margin 1 the faces go, in z too"""
    v = np.ones((9, 21, 34), np.float32)
    d_v = to_device(be, v)
    for margin in (0, 1):
        got = classified(be, d_v, 0.5, margin)
        assert np.array_equal(got, R.labels(v, 0.5, margin))
        inside = R.field_of_view(34, 21)
        if margin == 0:
            assert np.array_equal(got, np.broadcast_to(np.where(inside, 2, 0), got.shape)) and not inside[0, 0] and inside[10, 17]
        else:
            assert not got[0].any() and not got[-1].any() and got[1, 10, 17] == 2 and not got[:, 0].any() and not got[:, :, 0].any()
    be.free(d_v)


@pytest.mark.parametrize("margin,dim_z", [(1, 2), (4, 8), (2, 1)])
def test_a_slab_thinner_than_the_neighbourhood_has_no_label(be, margin, dim_z):
    v = slab(37, 19, dim_z, seed=7)
    d_v = to_device(be, v)
    got = classified(be, d_v, THR, margin)
    assert not got.any() and not R.labels(v, THR, margin).any()
    assert classified(be, d_v, THR, 0).any()
    be.free(d_v)


def test_classify_refusals(be):
    L = _lib.load()
    INV = _lib.ERROR_INVALID_ARGUMENT
    d_v = to_device(be, np.zeros((4, 5, 6), np.float32))
    lab = be.make_labels_device(6, 5, 4)
    fn = L.paris_hip_bh_classify
    assert fn(be._ctx, d_v.ptr, 6, 5, 4, 0.5, 5, lab.ptr) == INV                             # margin beyond the maximum
    assert fn(be._ctx, d_v.ptr, 6, 5, 4, float("nan"), 1, lab.ptr) == INV
    assert fn(be._ctx, d_v.ptr, 6, 5, 4, float("inf"), 1, lab.ptr) == INV
    assert fn(be._ctx, d_v.ptr, 0, 5, 4, 0.5, 1, lab.ptr) == INV
    assert fn(be._ctx, d_v.ptr, 6, 0, 4, 0.5, 1, lab.ptr) == INV
    assert fn(be._ctx, d_v.ptr, 6, 5, 0, 0.5, 1, lab.ptr) == INV
    assert fn(be._ctx, None, 6, 5, 4, 0.5, 1, lab.ptr) == INV
    assert fn(be._ctx, d_v.ptr, 6, 5, 4, 0.5, 1, None) == INV
    assert fn(be._ctx, d_v.ptr + 2, 6, 5, 4, 0.5, 1, lab.ptr) == INV                         # misaligned floats
    assert fn(be._ctx, d_v.ptr, 6, 5, 4, 0.5, 1, d_v.ptr + 8) == INV                         # the labels inside the slab
    assert fn(None, d_v.ptr, 6, 5, 4, 0.5, 1, lab.ptr) == INV
    assert fn(be._ctx, d_v.ptr, 1, 1 << 21, 1, 0.5, 1, lab.ptr) == _lib.ERROR_UNSUPPORTED    # refused before anything is touched
    with pytest.raises(ValueError):
        be.bh_classify(d_v, 0.5, 1, labels=be.make_labels_device(6, 5, 3))
    be.free(lab)
    be.free(d_v)


# ---- the Gram sums --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [3, R.L + 1, 3 * R.L + 7])
@pytest.mark.parametrize("degree", [1, 2, 3, 4])
def test_gram_sums_equal_the_host_function_bit_for_bit(be, n, degree):
    basis, lab = gram_case(n, degree, seed=n % 1000 + degree)
    want, want_cnt = B.bh_gram_host(basis, lab)
    d_f = [to_device(be, f.reshape(1, 1, n)) for f in basis]
    d_lab = be.labels_from_host(lab.reshape(1, 1, n))
    assert np.array_equal(be.labels_to_host(d_lab).ravel(), lab)
    got, cnt = be.bh_gram(d_f, d_lab)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (n, degree, got, want)
    counts = (cnt.n_object, cnt.n_air, cnt.n_ignored, cnt.n_not_finite)
    assert counts == (want_cnt.n_object, want_cnt.n_air, want_cnt.n_ignored, want_cnt.n_not_finite) and counts[3] == 1 and sum(counts) == n
    again, _ = be.bh_gram(d_f, d_lab)                         # the same bits every time
    assert np.array_equal(again.view(np.uint64), got.view(np.uint64))
    for d in d_f + [d_lab]:
        be.free(d)


def test_gram_refusals_and_nothing(be):
    L = _lib.load()
    INV = _lib.ERROR_INVALID_ARGUMENT
    d_f = to_device(be, np.ones((1, 1, 8), np.float32))
    d_lab = be.labels_from_host(np.ones((1, 1, 8), np.uint8))
    out, cnt = np.full(15, 7.0), _lib.BhCounts()
    ptrs = (C.c_void_p * 4)(d_f.ptr, d_f.ptr, d_f.ptr, d_f.ptr)
    fn = L.paris_hip_bh_gram
    assert fn(be._ctx, ptrs, 1, d_lab.ptr, 0, out.ctypes.data, C.byref(cnt)) == 0 and not out[:3].any() and cnt.n_air == 0
    assert fn(be._ctx, ptrs, 4, d_lab.ptr, 8, out.ctypes.data, C.byref(cnt)) == 0 and cnt.n_air == 8 and out[0] == 8.0 and out[14] == 0.0
    assert fn(be._ctx, ptrs, 0, d_lab.ptr, 8, out.ctypes.data, C.byref(cnt)) == INV
    assert fn(be._ctx, ptrs, 5, d_lab.ptr, 8, out.ctypes.data, C.byref(cnt)) == INV
    assert fn(be._ctx, None, 1, d_lab.ptr, 8, out.ctypes.data, C.byref(cnt)) == INV
    assert fn(be._ctx, ptrs, 1, None, 8, out.ctypes.data, C.byref(cnt)) == INV
    assert fn(be._ctx, ptrs, 1, d_lab.ptr, 8, None, C.byref(cnt)) == INV
    assert fn(be._ctx, ptrs, 1, d_lab.ptr, 8, out.ctypes.data, None) == INV
    assert fn(be._ctx, (C.c_void_p * 1)(None), 1, d_lab.ptr, 8, out.ctypes.data, C.byref(cnt)) == INV
    assert fn(be._ctx, (C.c_void_p * 1)(d_f.ptr + 2), 1, d_lab.ptr, 8, out.ctypes.data, C.byref(cnt)) == INV
    assert fn(None, ptrs, 1, d_lab.ptr, 8, out.ctypes.data, C.byref(cnt)) == INV
    with pytest.raises(ValueError):
        be.bh_gram([d_f], be.make_labels_device(7, 1, 1))
    be.free(d_f)
    be.free(d_lab)


# ---- end to end -----------------------------------------------------------------------------------------------------------------------

SLICES = (16, 32)       # slices 16 .. 47
MARGIN = 1


def reconstruct(be, frames, det, vg, c=None):
    """the whole volume through the Python chain: upload, the pass (with c), weight, filter, backproject"""
    v = be.make_volume_device(vg.dim_x, vg.dim_y, vg.dim_z)
    be.memset_volume(v)
    if c is not None:
        be.set_beam_hardening(c, det.n_row, det.n_col)
    for i, f in enumerate(frames):
        d_p = B.load(be, B.Projection(f, det.n_row, det.n_col, idx=i))
        if c is not None:
            be.beam_hardening(d_p)
        B.weight(be, d_p, det)
        B.filter(be, d_p, det)
        B.backproject(be, d_p, v, 0, det, vg, False, False, None)
        be.free(d_p)
    if c is not None:
        be.clear_beam_hardening()
    h = be.make_volume_host(vg.dim_x, vg.dim_y, vg.dim_z)
    be.copy_d2h(v, h)
    be.free(v)
    return h.buf.copy()


@pytest.fixture(scope="module")
def scan(be):
    """the frames, and the two reconstructions every case shares: uncorrected and monochromatic"""
    det = B.DetectorGeometry(*R.SCAN_GEO)
    vg = B.calculate_volume_geometry(det)
    assert (vg.dim_x, vg.dim_y, vg.dim_z) == (64, 64, 64)
    lengths = R.path_lengths()
    poly, mono = R.polychromatic(lengths), R.monochromatic(lengths)
    assert 2.0 < max(p.max() for p in poly) < 2.6
    return det, vg, poly, reconstruct(be, poly, det, vg), reconstruct(be, mono, det, vg)


@pytest.mark.parametrize("degree", [2, 3])
def test_the_fit_flattens_a_homogeneous_object(be, scan, degree):
    """Measured on the CPU with the oracle: spread 0.114 uncorrected, 0.0157 (N = 2) and 0.0154 (N = 3) fitted, 0.0129 monochromatic.
    The residual's tolerance: the corrected slab is FDK(sum c_k p^k) and the fit's figure belongs to sum c_k FDK(p^k) with the same
    float coefficients; the two differ by fp32 roundings only -- the N roundings of the Horner steps and the multiplication, two
    per butterfly stage of the row filter's forward and inverse transforms, one per view added in the backprojection -- each at most
    2^-24 of a term c_k f_k, whose rms size over the labelled voxels is |c_k| sqrt(G[k][k] / n) from the fit's own Gram sums."""
    det, vg, poly, uncorrected, mono = scan
    fit = be.fit_beam_hardening(poly, det, degree=degree, margin=MARGIN, slices=SLICES)
    assert fit.c.shape == (degree,) and fit.c.dtype == np.float32 and fit.slices == SLICES and fit.labels.shape == (32, 64, 64)
    core = np.zeros((64, 64, 64), bool)
    core[SLICES[0]:SLICES[0] + SLICES[1]] = fit.labels == 2
    assert core.sum() == fit.counts.n_object > 2000 and fit.counts.n_air > 2000 and fit.counts.n_not_finite == 0
    corrected = reconstruct(be, poly, det, vg, c=fit.c)
    s_un, s_fit, s_mono = R.spread(uncorrected, core), R.spread(corrected, core), R.spread(mono, core)
    print("degree %d: c = %s, spread uncorrected %.4f, fitted %.4f, monochromatic %.4f; residual before %.4f, after %.4f"
          % (degree, fit.c, s_un, s_fit, s_mono, fit.residual_before, fit.residual_after))
    assert s_fit <= 0.25 * s_un
    assert s_fit <= 1.5 * s_mono
    assert fit.residual_after < fit.residual_before
    # the reported residual is the corrected slab's
    used = fit.labels != 0
    sl = corrected[SLICES[0]:SLICES[0] + SLICES[1]].astype(np.float64)
    direct = math.sqrt(np.mean((sl[used] - fit.level * (fit.labels[used] == 2)) ** 2)) / abs(fit.level)
    g = R.gram_matrix(fit.gram, degree)
    n = fit.counts.n_object + fit.counts.n_air
    size = sum(abs(float(fit.c[k])) * math.sqrt(g[k, k] / n) for k in range(degree)) / abs(fit.level)
    roundings = degree + 1 + 4 * int(math.log2(B.filter_size(det.n_row))) + R.SCAN_VIEWS
    tol = roundings * 2.0 ** -24 * size
    print("degree %d: residual after %.9f, from the corrected slab %.9f, tolerance %.3g" % (degree, fit.residual_after, direct, tol))
    assert abs(direct - fit.residual_after) <= tol


def test_the_fit_uses_prepare_and_frees_what_it_made(be, scan):
    det, vg, poly, _, _ = scan
    owned = set(be._owned)
    seen = []
    fit = be.fit_beam_hardening(poly[:6], det, degree=2, margin=MARGIN, slices=SLICES, min_voxels=1,
                                prepare=lambda b, p: seen.append(p.idx))
    assert seen == [0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5] and fit.c.shape == (2,)             # every basis of every frame
    assert set(be._owned) == owned
    with pytest.raises(B.ParisHipError):                      # also when the fit is refused
        be.fit_beam_hardening(poly[:2], det, degree=2, margin=5, slices=SLICES)
    assert set(be._owned) == owned


def test_the_fit_refuses(be, scan):
    det, vg, poly, _, _ = scan
    for kw in ({"degree": 0}, {"degree": 5}, {"slices": (60, 8)}, {"slices": (0, 0)}, {"margin": 5}):
        with pytest.raises(B.ParisHipError) as e:
            be.fit_beam_hardening(poly[:2], det, **{"degree": 2, "slices": SLICES, **kw})
        assert e.value.status == _lib.ERROR_INVALID_ARGUMENT, kw
    air = [np.zeros_like(poly[0])] * 2                        # nothing in the beam: no range to take a histogram over
    with pytest.raises(B.ParisHipError):
        be.fit_beam_hardening(air, det, degree=2, slices=SLICES)
    with pytest.raises(B.ParisHipError) as e:                 # a margin that leaves no core: too few voxels
        be.fit_beam_hardening(poly, det, degree=2, margin=4, slices=(28, 8))
    assert e.value.status == _lib.ERROR_BH_TOO_FEW_VOXELS
