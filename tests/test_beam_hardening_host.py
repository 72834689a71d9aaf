"""The host side of the beam-hardening correction (paris_hip_beam_hardening_check / _host, paris_hip_bh_threshold_from_histogram,
paris_hip_bh_gram_host, paris_hip_bh_solve): no device, no ctx -- the library's rule, threshold and Gram sum
against their numpy restatement (tests/beam_hardening_rule.py) bit for bit, the solver against numpy.linalg.solve, every refusal, and
the wrong restatements that show the comparisons can fail."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import beam_hardening_rule as R
from paris_amd import _lib
from paris_amd import backend as B

INV = _lib.ERROR_INVALID_ARGUMENT


# ---- the pixel rule -----------------------------------------------------------------------------------------------------------------

def test_the_restatements_fused_multiply_add_is_exact():
    """against exact rational arithmetic on values chosen to make double rounding bite: the sum lies next to a float's midpoint"""
    from fractions import Fraction
    rng = np.random.default_rng(1)
    a = rng.uniform(-2, 2, 400).astype(np.float32)
    b = rng.uniform(-2, 2, 400).astype(np.float32)
    c = rng.uniform(-2, 2, 400).astype(np.float32)
    a[:100] = np.float32(1) + np.float32(2.0 ** -12)          # a * a = 1 + 2^-11 + 2^-24: half an ulp of 1 beyond a float
    b[:100] = a[:100]
    c[:100] = (rng.integers(1, 9, 100) * 2.0 ** -50).astype(np.float32) * rng.choice([-1, 1], 100).astype(np.float32)
    got = R.fmaf(a, b, c)
    for x, y, z, g in zip(a, b, c, got):
        exact = Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))
        lo = np.float32(float(exact))                            # a float near the exact value: the nearest is it or a neighbour
        cands = [lo, np.nextafter(lo, np.float32(np.inf)), np.nextafter(lo, np.float32(-np.inf))]
        err = [abs(Fraction(float(v)) - exact) for v in cands]
        best = min(err)
        nearest = [v for v, e in zip(cands, err) if e == best]
        if len(nearest) == 2:                                    # a tie: the even one
            nearest = [v for v in nearest if v.view(np.uint32) % 2 == 0]
        assert g.view(np.uint32) == nearest[0].view(np.uint32), (x, y, z)


@pytest.mark.parametrize("degree", [1, 2, 3, 4])
def test_the_rule_equals_the_restatement_bit_for_bit(degree):
    p = R.special_pixels((41, 53), seed=degree)
    assert np.count_nonzero(p < 0) > 100 and np.isnan(p).any() and np.isinf(p).any()
    assert np.count_nonzero((p != 0) & (np.abs(p) < 1.1754944e-38)) >= 4                     # denormals
    assert np.count_nonzero(R.bits(p) == 0x80000000) >= 1 and np.count_nonzero(R.bits(p) == 0) >= 1
    c = R.COEFFICIENTS[degree]
    got = B.beam_hardening_host(c, p)
    want = R.apply(c, p)
    assert R.same_pixels(got, want)
    if degree > 1:
        wrong = R.PERTURBATIONS["higher terms on negative pixels"](c, p)
        assert not R.same_pixels(got, wrong)                                                 # the comparison can fail


def test_degree_one_with_c1_one_is_the_identity_on_every_bit_but_a_nan_payload():
    p = R.special_pixels((7, 33), seed=9)
    got = B.beam_hardening_host([1.0], p)
    assert R.same_pixels(got, p) and R.same_pixels(got, R.apply([1.0], p))


def test_a_fused_multiply_add_is_what_the_library_uses():
    """a pixel where fmaf and multiply-then-add differ in the last bit"""
    p = np.array([1 + 2.0 ** -12], np.float32)
    c = [float(np.float32(-1 - 2.0 ** -11)), 1.0 + 2.0 ** -12]                               # acc = fmaf(c2, p, c1) = 2^-24 exactly
    got = B.beam_hardening_host(c, p)
    unfused = (np.float32(c[1]) * p + np.float32(c[0])) * p
    assert R.same_pixels(got, R.apply(c, p)) and got[0] != unfused[0] and got[0] == np.float32(2.0 ** -24) * p[0]


def test_the_rule_in_place_and_on_nothing():
    s = B._bh_setting([0.5, 0.25])
    p = np.array([1.0, -2.0, 4.0], np.float32)
    L = _lib.load()
    assert L.paris_hip_beam_hardening_host(C.byref(s), p.ctypes.data, p.ctypes.data, 3) == 0
    assert np.array_equal(p, np.array([0.75, -1.0, 6.0], np.float32))
    assert L.paris_hip_beam_hardening_host(C.byref(s), None, None, 0) == 0
    assert B.beam_hardening_host([1.0, 2.0], np.zeros((0, 4), np.float32)).shape == (0, 4)


@pytest.mark.parametrize("what,c", [("degree 0", []), ("degree 5", [1, 0, 0, 0, 0]), ("c_1 NaN", [float("nan"), 1.0]),
                                     ("c_3 Inf", [1.0, 0.0, float("inf")]), ("c_4 -Inf", [1.0, 0.0, 0.0, float("-inf")])])
def test_the_check_refuses(what, c):
    with pytest.raises(B.ParisHipError) as e:
        B.beam_hardening_check(c)
    assert e.value.status == INV, what
    with pytest.raises(B.ParisHipError):
        B.beam_hardening_host(c, np.zeros(3, np.float32))


def test_the_check_accepts_and_ignores_what_lies_beyond_the_degree():
    L = _lib.load()
    s = _lib.BeamHardening(2, (C.c_float * 4)(1.0, 0.5, float("nan"), float("inf")))
    assert L.paris_hip_beam_hardening_check(C.byref(s)) == 0
    assert L.paris_hip_beam_hardening_check(None) == INV
    p = np.ones(2, np.float32)
    assert L.paris_hip_beam_hardening_host(C.byref(s), None, p.ctypes.data, 2) == INV
    assert L.paris_hip_beam_hardening_host(C.byref(s), p.ctypes.data, None, 2) == INV
    for c in R.COEFFICIENTS.values():
        B.beam_hardening_check(c)
    assert B.Backend.beam_hardening_check is B.beam_hardening_check and B.Backend.beam_hardening_host is B.beam_hardening_host


# ---- (a) Otsu's threshold -----------------------------------------------------------------------------------------------------------

def bimodal(n_bins=R.BINS, seed=3):
    rng = np.random.default_rng(seed)
    v = np.concatenate([rng.normal(0.02, 0.01, 60000), rng.normal(0.21, 0.02, 25000)])
    return np.histogram(v, n_bins, (v.min(), v.max()))[0].astype(np.uint64), float(np.float32(v.min())), float(np.float32(v.max()))


def test_otsu_on_a_bimodal_histogram():
    hist, lo, hi = bimodal()
    thr = B.bh_threshold_from_histogram(hist, lo, hi)
    assert R.bits(thr) == R.bits(R.otsu_threshold(hist, lo, hi))
    assert 0.06 < thr < 0.16                                                                 # between the modes
    b, score = R.otsu_bin(hist)
    assert score[b] > score[b - 1] > 0 and score[b + 1] == score[b]        # the empty bins between the modes tie: the first one wins
    other = R.bits(np.float32(np.float64(np.float32(lo)) + b * ((np.float64(np.float32(hi)) - np.float64(np.float32(lo))) / len(hist))))
    assert other != R.bits(thr)                                                              # the bin's upper edge, not its lower


def test_otsu_on_one_bin_and_on_one_filled_bin():
    assert R.bits(B.bh_threshold_from_histogram([7], -1.0, 3.0)) == R.bits(np.float32(3.0)) == R.bits(R.otsu_threshold([7], -1.0, 3.0))
    hist = np.zeros(16, np.uint64)
    hist[5] = 9                                                                              # no split has two sides: every score 0
    assert R.bits(B.bh_threshold_from_histogram(hist, 0.0, 16.0)) == R.bits(np.float32(1.0)) == R.bits(R.otsu_threshold(hist, 0.0, 16.0))


@pytest.mark.parametrize("hist,want_bin", [([5, 0, 0, 5], 0), ([0, 3, 0, 0, 0, 3, 0], 1), ([2, 0, 2, 0, 0, 0], 0)])
def test_otsu_ties_go_to_the_smallest_bin(hist, want_bin):
    b, score = R.otsu_bin(hist)
    assert b == want_bin and np.count_nonzero(score == score[b]) >= 2                        # tied maxima
    thr = B.bh_threshold_from_histogram(hist, 0.0, float(len(hist)))
    assert thr == np.float32(want_bin + 1) and R.bits(thr) == R.bits(R.otsu_threshold(hist, 0.0, float(len(hist))))


def test_otsu_on_random_histograms():
    rng = np.random.default_rng(4)
    for n_bins in (2, 3, 17, 256, R.BINS):
        for _ in range(4):
            hist = (rng.integers(0, 1000, n_bins) * (rng.uniform(0, 1, n_bins) < 0.6)).astype(np.uint64)
            hist[rng.integers(0, n_bins)] += 1
            lo, hi = -0.37, 1.91
            assert R.bits(B.bh_threshold_from_histogram(hist, lo, hi)) == R.bits(R.otsu_threshold(hist, lo, hi)), n_bins


@pytest.mark.parametrize("what,hist,lo,hi", [("empty", [0, 0, 0], 0.0, 1.0), ("no bins", [], 0.0, 1.0), ("hi == lo", [1, 2], 1.0, 1.0),
                                              ("hi < lo", [1, 2], 1.0, 0.0), ("lo NaN", [1, 2], float("nan"), 1.0),
                                              ("hi Inf", [1, 2], 0.0, float("inf")), ("too narrow", [1, 2], 0.0, 1e-40)])
def test_the_threshold_refuses(what, hist, lo, hi):
    with pytest.raises(B.ParisHipError) as e:
        B.bh_threshold_from_histogram(hist, lo, hi)
    assert e.value.status == INV, what


def test_the_threshold_refuses_null_pointers():
    L = _lib.load()
    h, thr = np.ones(4, np.uint64), C.c_float(7.0)
    assert L.paris_hip_bh_threshold_from_histogram(None, 4, 0.0, 1.0, C.byref(thr)) == INV
    assert L.paris_hip_bh_threshold_from_histogram(h.ctypes.data, 4, 0.0, 1.0, None) == INV
    assert thr.value == 7.0
    with pytest.raises(ValueError):
        B.bh_threshold_from_histogram(np.ones((2, 2)), 0.0, 1.0)


# ---- the labels' restatement can fail -----------------------------------------------------------------------------------------------

def test_the_label_restatement_and_its_wrong_twin_differ():
    rng = np.random.default_rng(5)
    v = rng.uniform(0, 1, (11, 17, 19)).astype(np.float32)
    v[:, 4:13, 5:15] += 2
    v[5, 8, 9] = 0                                                                           # a hole in the middle slice
    right = R.labels(v, 1.5, 1)
    wrong = R.PERTURBATIONS["margin in x and y only"](v, 1.5, 1)
    assert right[4, 8, 9] == 0 and wrong[4, 8, 9] == 2 and wrong[0].any() and not right[0].any()
    assert set(np.unique(right)) == {0, 1, 2}


# ---- (c) the Gram sum ---------------------------------------------------------------------------------------------------------------

def gram_case(n, degree, seed):
    """values over many decades, so that the order of the additions decides the low bits; random labels, 3 among them; one
    labelled voxel that is not finite"""
    rng = np.random.default_rng(seed)
    basis = [(rng.normal(0, 1, n) * 10.0 ** rng.integers(-4, 5, n)).astype(np.float32) for _ in range(degree)]
    lab = rng.choice(np.array([0, 1, 2, 3], np.uint8), n, p=[0.2, 0.35, 0.35, 0.1])
    lab[0] = 2
    lab[n - 1] = 1
    basis[degree - 1][n // 2] = np.inf
    lab[n // 2] = 2
    return basis, lab


@pytest.mark.parametrize("n", [3, R.L + 1, 3 * R.L + 7])
@pytest.mark.parametrize("degree", [1, 2, 3, 4])
def test_the_gram_sum_equals_the_restatement_bit_for_bit(n, degree):
    basis, lab = gram_case(n, degree, seed=n % 1000 + degree)
    g, cnt = B.bh_gram_host(basis, lab)
    want, counts = R.gram(basis, lab)
    assert g.shape == (R.terms(degree),) and np.array_equal(g.view(np.uint64), want.view(np.uint64))
    assert (cnt.n_object, cnt.n_air, cnt.n_ignored, cnt.n_not_finite) == counts and counts[3] == 1 and sum(counts) == n
    assert g[-1] == counts[0]                                                                # G[m][m] = n_object
    if n > R.L:
        wrong, wrong_counts = R.PERTURBATIONS["blockwise partial sums"](basis, lab)
        assert wrong_counts == counts and not np.array_equal(wrong.view(np.uint64), want.view(np.uint64))   # the order shows
        assert np.allclose(wrong, want, rtol=1e-6, atol=1e-6 * np.abs(want).max())             # ... in the low bits only


def test_the_gram_sum_of_nothing_and_its_refusals():
    L = _lib.load()
    g, cnt = B.bh_gram_host([np.zeros(0, np.float32)], np.zeros(0, np.uint8))
    assert not g.any() and (cnt.n_object, cnt.n_air, cnt.n_ignored, cnt.n_not_finite) == (0, 0, 0, 0)
    f, lab, out, c = np.ones(4, np.float32), np.ones(4, np.uint8), np.zeros(15), _lib.BhCounts()
    ptrs = (C.c_void_p * 4)(f.ctypes.data, f.ctypes.data, f.ctypes.data, f.ctypes.data)
    fn = L.paris_hip_bh_gram_host
    assert fn(ptrs, 4, lab.ctypes.data, 4, out.ctypes.data, C.byref(c)) == 0 and c.n_air == 4 and out[0] == 4.0
    assert fn(ptrs, 0, lab.ctypes.data, 4, out.ctypes.data, C.byref(c)) == INV
    assert fn(ptrs, 5, lab.ctypes.data, 4, out.ctypes.data, C.byref(c)) == INV
    assert fn(None, 1, lab.ctypes.data, 4, out.ctypes.data, C.byref(c)) == INV
    assert fn(ptrs, 1, None, 4, out.ctypes.data, C.byref(c)) == INV
    assert fn(ptrs, 1, lab.ctypes.data, 4, None, C.byref(c)) == INV
    assert fn(ptrs, 1, lab.ctypes.data, 4, out.ctypes.data, None) == INV
    assert fn((C.c_void_p * 1)(None), 1, lab.ctypes.data, 4, out.ctypes.data, C.byref(c)) == INV
    with pytest.raises(ValueError):
        B.bh_gram_host([np.zeros(3, np.float32)], np.zeros(4, np.uint8))


# ---- (d) the solver -----------------------------------------------------------------------------------------------------------------

def cupped_sample(degree, n=5000, seed=6):
    """basis values as a cupped reconstruction has them: f_k of an object voxel grows like level^k, air is noise near 0"""
    rng = np.random.default_rng(seed)
    lab = rng.choice(np.array([1, 2], np.uint8), n)
    level = np.where(lab == 2, rng.uniform(0.15, 0.25, n), rng.normal(0, 0.01, n))
    basis = [(level ** (k + 1) * (1 + rng.normal(0, 0.02, n)) * 3.0 ** k).astype(np.float32) for k in range(degree)]
    return basis, lab


@pytest.mark.parametrize("degree", [1, 2, 3, 4])
def test_the_solver_against_numpy(degree):
    """Tolerance, from the test's own matrix: Cholesky here and LU in numpy are both backward stable, so each solution lies within
    about 8 N u cond(A) of the exact one in relative norm (u = 2^-53; Higham, Accuracy and Stability, theorems 9.4 and 10.4, with the
    usual constants), the two within 64 cond(A) u of each other for N <= 4; on top, each coefficient is rounded once to float,
    2^-24 of itself."""
    basis, lab = cupped_sample(degree)
    g, cnt = B.bh_gram_host(basis, lab)
    fit = B.bh_solve(g, degree, cnt)
    a, b, t = R.normal_equations(g, degree, cnt.n_object)
    want = np.linalg.solve(a, b)
    cond = np.linalg.cond(a)
    tol = 64.0 * cond * 2.0 ** -53
    print("degree %d: cond(A) = %.3g, tolerance %.3g relative" % (degree, cond, tol))
    assert tol < 1e-3                                                                        # the test means something
    c = np.array(fit.setting.c[:degree], np.float64)
    assert fit.setting.degree == degree and np.all(np.abs(c - want) <= tol * np.abs(want).max() + 2.0 ** -24 * np.abs(want))
    assert fit.level == t and math.isclose(t, np.mean(basis[0].astype(np.float64)[lab == 2]), rel_tol=1e-12)
    counts = (cnt.n_object, cnt.n_air, cnt.n_ignored, cnt.n_not_finite)
    assert math.isclose(fit.residual_before, R.residual(g, degree, counts, [1.0] + [0.0] * (degree - 1)), rel_tol=1e-9)
    assert math.isclose(fit.residual_after, R.residual(g, degree, counts, c), rel_tol=1e-6, abs_tol=1e-12)
    assert fit.residual_after <= fit.residual_before * (1 + 1e-6)
    # the residual from the Gram sums is the residual of the voxels
    f = np.stack([x.astype(np.float64) for x in basis])
    direct = np.sqrt(np.mean((c @ f - t * (lab == 2)) ** 2)) / abs(t)
    assert math.isclose(fit.residual_after, direct, rel_tol=1e-6)


def test_the_solver_refuses_too_few_voxels():
    basis, lab = cupped_sample(2)
    g, cnt = B.bh_gram_host(basis, lab)
    for field in ("n_object", "n_air"):
        few = _lib.BhCounts(cnt.n_object, cnt.n_air, 0, 0)
        setattr(few, field, 63)
        with pytest.raises(B.ParisHipError) as e:
            B.bh_solve(g, 2, few)
        assert e.value.status == _lib.ERROR_BH_TOO_FEW_VOXELS and "too few" in str(e.value)
        setattr(few, field, 64)
        B.bh_solve(g, 2, few)                                                                # the default minimum is 64
        with pytest.raises(B.ParisHipError) as e:
            B.bh_solve(g, 2, few, min_voxels=65)
        assert e.value.status == _lib.ERROR_BH_TOO_FEW_VOXELS
        setattr(few, field, 1)
        B.bh_solve(g, 2, few, min_voxels=1)


def test_the_solver_refuses_a_pivot_that_is_not_positive():
    basis, lab = cupped_sample(2)
    twice = [basis[0], basis[0]]                                                             # f_2 = f_1: A is singular
    g, cnt = B.bh_gram_host(twice, lab)
    with pytest.raises(B.ParisHipError) as e:
        B.bh_solve(g, 2, cnt)
    assert e.value.status == _lib.ERROR_BH_NOT_POSITIVE and "positive definite" in str(e.value)
    g, cnt = B.bh_gram_host(basis, lab)
    g[0] = float("nan")
    with pytest.raises(B.ParisHipError) as e:
        B.bh_solve(g, 2, cnt)
    assert e.value.status == _lib.ERROR_BH_NOT_POSITIVE
    g[0] = -1.0
    with pytest.raises(B.ParisHipError) as e:
        B.bh_solve(g, 2, cnt)
    assert e.value.status == _lib.ERROR_BH_NOT_POSITIVE


def test_the_solver_refuses_a_coefficient_that_is_not_finite():
    cnt = _lib.BhCounts(100, 100, 0, 0)
    g = np.array([1e-300, 1e10, 100.0], np.float64)                                          # c_1 = T b / A = 1e8 * 1e10 / 1e-300: no float
    with pytest.raises(B.ParisHipError) as e:
        B.bh_solve(g, 1, cnt)
    assert e.value.status == _lib.ERROR_BH_NOT_FINITE and "not finite" in str(e.value)
    g = np.array([1.0, float("inf"), 100.0], np.float64)                                     # T itself
    with pytest.raises(B.ParisHipError) as e:
        B.bh_solve(g, 1, cnt)
    assert e.value.status == _lib.ERROR_BH_NOT_FINITE


def test_the_solver_refuses_bad_arguments_and_words_its_statuses():
    L = _lib.load()
    g, cnt, fit = np.ones(3), _lib.BhCounts(100, 100, 0, 0), _lib.BhFit()
    fn = L.paris_hip_bh_solve
    assert fn(None, 1, C.byref(cnt), 0, C.byref(fit)) == INV
    assert fn(g.ctypes.data, 1, None, 0, C.byref(fit)) == INV
    assert fn(g.ctypes.data, 1, C.byref(cnt), 0, None) == INV
    assert fn(g.ctypes.data, 0, C.byref(cnt), 0, C.byref(fit)) == INV
    assert fn(g.ctypes.data, 5, C.byref(cnt), 0, C.byref(fit)) == INV
    with pytest.raises(ValueError):
        B.bh_solve(np.ones(4), 1, cnt)
    texts = {L.paris_hip_strerror(s) for s in (_lib.ERROR_BH_TOO_FEW_VOXELS, _lib.ERROR_BH_NOT_POSITIVE, _lib.ERROR_BH_NOT_FINITE, INV)}
    assert len(texts) == 4 and all(b"beam-hardening" in t for t in texts if b"invalid" not in t)
    assert B.Backend.bh_solve is B.bh_solve and B.Backend.bh_gram_host is B.bh_gram_host


# ---- the driver refuses before any device work ------------------------------------------------------------------------------------

@pytest.mark.parametrize("extra,names", [
    (["--beam-hardening", "1:0.1", "--fit-beam-hardening", "2"], ["--beam-hardening", "--fit-beam-hardening"]),
    (["--fit-beam-hardening", "2", "--bin", "2"], ["--fit-beam-hardening", "--bin"]),
    (["--fit-beam-hardening", "5"], ["--fit-beam-hardening"]),
    (["--fit-beam-hardening", "2:32:5"], ["--fit-beam-hardening"]),
    (["--fit-beam-hardening", "2:4:2"], ["--fit-beam-hardening"]),
    (["--fit-beam-hardening", "2:65"], ["--fit-beam-hardening", "64 slice"]),
    (["--fit-beam-hardening", ""], ["--fit-beam-hardening"]),
    (["--beam-hardening", "1"], ["--beam-hardening"]),
    (["--beam-hardening", "1:inf"], ["--beam-hardening"]),
    (["--beam-hardening", "1:2:3:4:5"], ["--beam-hardening"]),
    (["--beam-hardening", "1:x"], ["--beam-hardening"]),
])
def test_the_driver_refuses_before_any_device_work(tmp_path, extra, names):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "paris_amd", "host", "demo", "paris.hip")
    if not os.path.exists(exe):
        pytest.fail("%s missing: run __graft_entry__.build()" % exe)
    keys = ("n_row", "n_col", "l_px_row", "l_px_col", "delta_s", "delta_t", "d_so", "d_od", "delta_phi")
    ini = tmp_path / "geo.ini"
    ini.write_text("\n".join("%s = %s" % kv for kv in zip(keys, R.SCAN_GEO)) + "\n")
    (tmp_path / "in").mkdir()
    args = [exe, "--geometry", ini, "--input", tmp_path / "in", "--output", tmp_path / "out"] + extra
    r = subprocess.run([str(a) for a in args], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1, r.stdout + r.stderr
    assert "Pipeline construction failed" in r.stderr and all(n in r.stderr for n in names), r.stderr
    assert not (tmp_path / "out").exists()   # refused before the output was set up, let alone a device
