"""The starvation filter's physical check on the float64 model: the scene of tests/starvation_scene.py -- a
dense body with a denser bar, Poisson noise at a flux that leaves the rays along the bar two photons -- filtered by the host rule and
reconstructed by tests/fdk_model.py. The streaks the starved rays throw over the body shrink: the RMS difference to the noise-free
reconstruction over the soft voxels away from the bar keeps the bound of starvation_scene.RATIO_BOUND, which comes from the
measurement with the numpy rule recorded there (8.942e-3 -> 4.881e-3 per mm, ratio 0.5459), not from the code under test. The conditions
that keep the check honest are asserted with it. tests/test_gpu_starvation.py repeats it with the device's frames. No device."""
import numpy as np

import starvation_rule as R
import starvation_scene as SC
from paris_amd import backend as B


def test_the_scene_is_what_the_check_needs():
    sc = SC.scene()
    p0 = np.float32(SC.SETTING[0])
    assert SC.SOFT * 2 * SC.RADIUS < p0 < SC.SOFT * 2 * SC.RADIUS + 0.5            # a little above the longest soft-only path
    soft_only = sc.exact[:, :8].max()                                              # the detector's first rows see the body, never the bar
    assert 2.0 < soft_only < p0
    long_rays = sc.exact > p0 + 2.0
    assert 0.01 < long_rays.mean() < 0.08                                          # a few per cent of the rays are long
    assert 1.0 < SC.N0 * np.exp(-float(sc.exact.max())) < 5.0                      # the longest counts a few photons
    assert sc.soft.sum() > 10000 and sc.far.sum() > 2000


def test_the_host_rule_on_the_scene_s_frames_is_the_numpy_rule():
    sc = SC.scene()
    for k in (0, 37, 90):                                                          # across the bar, along it, in between
        want, filtered, last = R.apply(sc.noisy[k], *SC.SETTING)
        got, counts = B.starvation_filter_host(SC.SETTING, sc.noisy[k])
        assert R.same(got, want) and (counts.filtered, counts.last_level) == (filtered, last) and filtered > 0


def test_starved_rays_leave_fewer_streaks():
    sc = SC.scene()
    out = [B.starvation_filter_host(SC.SETTING, f) for f in sc.noisy]
    frames = np.stack([o[0] for o in out])
    n_filtered, n_last = sum(o[1].filtered for o in out), sum(o[1].last_level for o in out)
    share = n_filtered / sc.noisy.size
    before, after, far = SC.measure(sc, frames)
    print("starvation scene, float64 model: unfiltered %.4g, filtered %.4g, ratio %.4g; %.4g of the pixels filtered, %.4g of them at the last "
          "level; the far region changes by %.3g" % (before, after, after / before, share, n_last / n_filtered, far))
    assert SC.SHARE_MIN <= share <= SC.SHARE_MAX
    assert n_last < 0.5 * n_filtered
    assert far <= SC.FAR_BOUND
    assert after / before <= SC.RATIO_BOUND
    assert abs(after / before - SC.RATIO_64) < 0.01                                # the recorded measurement is this scene's
