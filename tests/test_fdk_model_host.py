"""The CPU oracle against a float64 model written from the equations, and that model against the phantom's own densities (no GPU).

Every GPU check of the hot path -- cosine weight, ramp filter, voxel-driven backprojection -- compares with oracle/paris_oracle.c, a
float32 restatement of the reference line by line. A convention that it and the kernels read wrongly alike (a half-pixel shift, a
mirrored axis, a swapped offset sign, a missing U^2, a wrong 0.5) would pass all of them. Here
  (a) the oracle stays within its recorded error of tests/fdk_model.py, per stage and over the chain, on the cases of
      tests/fdk_cases.py (tests/golden/fdk_model_bounds.json, written by tests/golden/make_golden.py);
  (b) on the single views a voxel whose ray passes within 1e-3 pixel of a validity limit may hold the value with that sample zeroed,
      at most 0.2 % of a volume's voxels (the oracle needs none);
  (c) the model alone reconstructs the phantom: density to 0.5 % inside each ball, each ball's centroid to 0.1 voxel. Each ball
      sits on its own positive half-axis with its own density, so a flip or a transpose moves a known value; a half-pixel error is
      half a voxel at this magnification, a delta_t sign error 1.5 voxels in z, a delta_s error doubles edges and lowers the means.
tests/test_gpu_fdk_model.py holds the kernels to the same model and the same truth.
"""
import numpy as np
import pytest

import fdk_cases as K
import fdk_model as M
import phantom


@pytest.fixture(scope="module")
def w_model(oracle):
    return K.WModel(oracle)


def test_bounds_file_lists_every_case_and_stage(golden_dir):
    bounds = K.load_bounds(golden_dir)
    assert set(bounds) == set(K.ORACLE_CASES)
    v_stages = {"weight", "filter", "weight_filter", "chain"} | {"backproject_%s%s" % (s, v) for s in ("", "sum3_", "sum9_")
                                                                 for v in K.V_VOLUMES}
    assert set(bounds["v61"]) == set(bounds["v64"]) == v_stages
    assert set(bounds["f97"]) == {"filter", "weight_filter"}
    assert set(bounds["w"]) == {"weight", "filter", "weight_filter", "backproject", "chain"}
    for stages in bounds.values():
        for b in stages.values():
            # float32 rounding, not a convention: the largest recorded figure is a few 1e-6 of the maximum
            assert 0 < b["error"] < 1e-5 and 0 <= b["boundary_share"] <= K.BOUNDARY_SHARE


@pytest.mark.parametrize("case", list(K.ORACLE_CASES))
def test_oracle_stays_within_its_recorded_error_of_the_model(oracle, golden_dir, case, w_model):
    bounds = K.load_bounds(golden_dir)[case]
    measured = K.ORACLE_CASES[case](oracle, w_model) if case == "w" else K.oracle_errors(oracle, case)
    assert set(measured) == set(bounds)
    problems = []
    for stage, (err, share) in sorted(measured.items()):
        print("%s %s: error %.3g (recorded %.3g), boundary rule on %.4f %% of the voxels" % (case, stage, err, bounds[stage]["error"],
                                                                                            100 * share))
        if not err <= bounds[stage]["error"]:
            problems.append("%s: %.4g of the model's maximum, recorded %.4g" % (stage, err, bounds[stage]["error"]))
        if not share <= K.BOUNDARY_SHARE:
            problems.append("%s: %.3f %% of the voxels needed the boundary rule" % (stage, 100 * share))
    assert not problems, "\n".join(problems)


def test_case_geometry_is_what_the_cases_say(oracle):
    for name, g in K.V_DETECTORS.items():
        vg = oracle.calculate_volume_geometry(oracle.DetectorGeometry(*g))
        assert (vg.dim_x, vg.dim_y, vg.dim_z) == K.V_NATURAL[name]
        det = oracle.DetectorGeometry(*g)
        # each volume leaves some voxels outside the detector and most inside, at every angle
        for vol in K.V_VOLUMES:
            for phi in K.V_ANGLES:
                outside = float((K.v_view(oracle, name, vol, phi).total == 0).mean())
                assert (0.0 if vol == "roi_slab" else 0.05) <= outside <= 0.7, (name, vol, phi, outside)
        over = K.v_placement(oracle, det, "overshoot").vol_geo
        assert len({over.l_vx_x, over.l_vx_y, over.l_vx_z}) == 3
    p = K.v_projection(61, 45)
    for edge in (p[0], p[-1], p[:, 0], p[:, -1]):                                         # non-zero along every edge
        assert np.abs(edge).min() > 0 and np.abs(edge).mean() > 0.5
    assert np.abs(p - p[:, ::-1]).max() > 0.1 and np.abs(p - p[::-1]).max() > 0.1       # asymmetric in both axes


def test_model_truth_densities_and_centroids(w_model):
    """(c): nothing here is compared with the code under test."""
    for mean, want, centroid in K.truth_figures(w_model.boxes, w_model.vol_geo):
        print("inner mean %.5f (phantom %.2f), centroid error (x, y, z) = (%.4f, %.4f, %.4f) voxels" % ((mean, want) + centroid))
    assert not K.truth_problems(w_model.boxes, w_model.vol_geo)


def test_truth_assertions_see_a_shift_a_flip_and_a_scale(w_model):
    """the assertions of (c) on volumes that are wrong in a known way: half a voxel along each axis, a mirrored or transposed axis, 1 %"""
    vg = w_model.vol_geo
    balls = K.w_balls(vg)
    # the phantom itself, sampled on the grid, smoothed a little: what a perfect reconstruction would be
    x, y, z = ((np.arange(d) + 0.5) * l - d * l / 2 for d, l in ((vg.dim_x, vg.l_vx_x), (vg.dim_y, vg.l_vx_y), (vg.dim_z, vg.l_vx_z)))
    fine = np.linspace(-0.375, 0.375, 4)
    exact = np.zeros((vg.dim_z, vg.dim_y, vg.dim_x))
    for oz in fine:
        for oy in fine:
            for ox in fine:
                exact += phantom.density(x[None, None, :] + ox * vg.l_vx_x, y[None, :, None] + oy * vg.l_vx_y,
                                         z[:, None, None] + oz * vg.l_vx_z, K.w_radius_mm(vg), K.W_ELLIPSOIDS)
    exact /= fine.size ** 3

    def problems(vol):
        return K.truth_problems([K.crop(vol, b) for b in balls], vg)

    assert not problems(exact)
    assert problems(exact * 1.01)
    for axis in range(3):
        half = 0.5 * (exact + np.roll(exact, 1, axis))
        assert problems(half), "half a voxel along axis %d" % axis
        assert problems(np.flip(exact, axis)), "axis %d mirrored" % axis
    assert problems(exact.transpose(0, 2, 1)) and problems(exact.transpose(2, 1, 0))


def test_ramp_is_the_references_zero_padded_circular_product():
    """fdk_model.ramp convolves in the spatial domain; the reference multiplies spectra at N = 2 * 2^ceil(log2 n_row). The same
    thing: the kernel's DFT is real and positive (so |.| and the two equal components change nothing) and no tap wraps around."""
    rng = np.random.default_rng(7)
    for n, tau in ((61, 0.7), (64, 0.7), (97, 0.7), (128, 0.8), (5, 0.2)):
        size = 2 * 2 ** int(np.ceil(np.log2(n)))
        j = np.arange(-(size - 2) // 2, size // 2 + 1)                  # the reference's tap order, j = -(N/2 - 1) .. N/2
        r = np.where(j % 2 != 0, -1.0 / (2.0 * np.maximum(j * j, 1) * np.pi ** 2 * tau ** 2), 0.0)
        r[j == 0] = 1.0 / (8.0 * tau ** 2)
        circular = np.roll(r, -int(np.flatnonzero(j == 0)[0]))           # tap j at index j mod N
        spectrum = np.fft.fft(circular)
        assert np.abs(spectrum.imag).max() <= 1e-12 * spectrum.real.max() and spectrum.real.min() > 0
        k = tau * np.abs(np.fft.rfft(r))
        assert np.allclose(k, tau * spectrum.real[:size // 2 + 1], rtol=1e-12, atol=0)
        p = rng.standard_normal((3, n))
        want = np.fft.irfft(np.fft.rfft(p, size, axis=1) * k[None, :], size, axis=1)[:, :n]
        got = M.ramp(p, tau)
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
        assert np.array_equal(M.ramp_kernel(n, tau), r[(j > -n) & (j < n)])


def test_scale_is_the_three_factors():
    det = type("D", (), dict(n_row=8, n_col=8, l_px_row=1.0, l_px_col=1.0, delta_s=0.0, delta_t=0.0, d_so=500.0, d_od=300.0))
    assert M.scale(det, 120) == pytest.approx((500.0 / 800.0) * 0.5 * 120 / (2 * np.pi), rel=1e-15)


def test_phantom_density_integrates_to_its_projection():
    """density() and projection() describe the same object in the same frame: central and oblique rays of one view, integrated by
    sampling the density, against the analytic line integrals; and the default table still is the head phantom."""
    g, radius = K.W_DETECTOR, 26.0
    phi = 33.0
    proj = phantom.projection(g[0], g[1], g[2], g[3], g[6], g[7], phi, radius, delta_s=g[4], delta_t=g[5], ellipsoids=K.W_ELLIPSOIDS)
    c, s = np.cos(np.deg2rad(phi)), np.sin(np.deg2rad(phi))
    src = np.array([-g[6] * c, -g[6] * s, 0.0])
    lam = (np.arange(200000) + 0.5) / 200000
    for i, j in ((64, 48), (30, 40), (100, 60), (75, 20)):
        t = (i + 0.5) * g[2] - g[0] * g[2] / 2 - g[4] * g[2]
        zz = (j + 0.5) * g[3] - g[1] * g[3] / 2 - g[5] * g[3]
        pix = np.array([g[7] * c - t * s, g[7] * s + t * c, zz])
        pts = src[None, :] + lam[:, None] * (pix - src)[None, :]
        integral = phantom.density(pts[:, 0], pts[:, 1], pts[:, 2], radius, K.W_ELLIPSOIDS).mean() * np.linalg.norm(pix - src)
        assert proj[j, i] > 1.0 and abs(integral - proj[j, i]) <= 2e-3 * proj[j, i], (i, j, integral, proj[j, i])
    same = phantom.projection(64, 48, 0.8, 1.0, 500, 300, 12.0, 20.0, ellipsoids=phantom.ELLIPSOIDS)
    assert np.array_equal(same, phantom.projection(64, 48, 0.8, 1.0, 500, 300, 12.0, 20.0))
    table = phantom.ELLIPSOIDS      # callers that swap the module's table for their own (tests/beam_hardening_rule.py) still get theirs
    phantom.ELLIPSOIDS = K.W_ELLIPSOIDS
    try:
        swapped = phantom.projection(g[0], g[1], g[2], g[3], g[6], g[7], phi, radius, delta_s=g[4], delta_t=g[5])
        assert phantom.density(0.55 * radius, 0.0, 0.0, radius) == pytest.approx(1.1)
    finally:
        phantom.ELLIPSOIDS = table
    assert np.array_equal(swapped, proj)
    assert phantom.density(0.0, 0.0, 0.0, 20.0) == pytest.approx(0.2) and phantom.density(0.0, 0.0, 19.0, 20.0) == 0.0
