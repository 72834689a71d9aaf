"""The starvation filter's host rule (paris_hip_starvation_filter_host, starvation_rule.cpp) against the numpy
restatement of tests/starvation_rule.py, bit for bit; the tables against float64; every refusal of the check; and the wrong readings of
the rule, each of which must differ from it on these inputs. No device."""
import numpy as np
import pytest

import starvation_rule as R
from paris_amd import _lib
from paris_amd import backend as B

RADII = (1, 2, 3, 4)
GAIN = 1.0


def host(frame, radius, p0=R.P0, gain=GAIN):
    out, counts = B.starvation_filter_host((p0, gain, radius), frame)
    return out, counts


@pytest.fixture(scope="module")
def cases():
    """every frame once, with the restatement's answer per radius, computed when first asked for"""
    frames = {shape: R.frame(shape[0], shape[1], 11 + k) for k, shape in enumerate(R.SHAPES)}
    cache = {}

    def want(shape, radius):
        if (shape, radius) not in cache:
            cache[(shape, radius)] = R.apply(frames[shape], R.P0, GAIN, radius)
        return cache[(shape, radius)]

    return frames, want


@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("shape", R.SHAPES)
def test_the_host_rule_gives_the_restatement_s_bits(cases, shape, radius):
    frames, want = cases
    a = frames[shape]
    w, filtered, last = want(shape, radius)
    got, counts = host(a, radius)
    assert R.same(got, w)
    assert (counts.frames, counts.filtered, counts.last_level) == (1, filtered, last)
    untouched = ~(a > np.float32(R.P0))
    assert np.array_equal(R.bits(got)[untouched], R.bits(a)[untouched])
    if a.size >= 64 * 3:
        assert filtered > 0.1 * a.size and 0 < last < filtered


def test_the_frames_hold_what_the_rule_must_tell_apart(cases):
    frames, _ = cases
    a = frames[(130, 33)]
    p0 = np.float32(R.P0)
    for k in range(64):
        b = np.float32(p0 + np.float32(k / 16.0))
        assert (a == b).any() and (a == R.ulp_steps(b, -1)).any() and (a == R.ulp_steps(b, 1)).any(), k
    levels = {R.level(c, p0) for c in a[(a > p0) & np.isfinite(a)]}
    assert levels == set(range(64))
    assert np.isposinf(a).sum() >= 2 and np.isneginf(a).any() and (R.bits(a) == R.NAN_PAYLOAD).any()
    assert ((a == 0) & np.signbit(a)).any()
    for yy in (0, a.shape[0] - 1):
        for xx in (0, a.shape[1] - 1):
            assert a[yy, xx] > p0
    assert (a[0, 1:-1] > p0).any() and (a[-1, 1:-1] > p0).any() and (a[1:-1, 0] > p0).any() and (a[1:-1, -1] > p0).any()


@pytest.mark.parametrize("radius", RADII)
def test_a_centre_all_of_whose_taps_are_non_finite_is_not_written(cases, radius):
    frames, want = cases
    a = frames[(130, 33)]
    cy, cx = a.shape[0] // 2, a.shape[1] // 2
    assert np.isposinf(a[cy, cx]) and not np.isfinite(a[cy - 4:cy + 5, cx - 4:cx + 5]).any()
    got, _ = host(a, radius)
    assert np.isposinf(got[cy, cx])
    # another +inf centre, which has finite neighbours, is replaced by their mean
    others = [(y, x) for y, x in zip(*np.nonzero(np.isposinf(a))) if (y, x) != (cy, cx)]
    assert any(np.isfinite(got[y, x]) for y, x in others)


@pytest.mark.parametrize("shape", R.SHAPES)
def test_at_or_below_p0_nothing_is_written(shape):
    a = R.below(shape[0], shape[1], 5)
    for radius in RADII:
        got, counts = host(a, radius)
        assert np.array_equal(R.bits(got), R.bits(a))
        assert (counts.frames, counts.filtered, counts.last_level) == (1, 0, 0)


def test_the_pass_is_not_idempotent(cases):
    frames, _ = cases
    once, _ = host(frames[(65, 17)], 2)
    twice, _ = host(once, 2)
    assert not R.same(twice, once)


@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("gain", [0.25, 1.0, 3.0])
def test_the_tables_against_float64(radius, gain):
    sigma, g = B.starvation_filter_tables((R.P0, gain, radius))
    assert sigma.shape == (64,) and g.shape == (64, radius + 1)
    k = np.arange(64, dtype=np.float64)
    s64 = np.minimum(radius / 2.0, float(np.float32(gain)) * np.sqrt(np.expm1((k + 0.5) / 16.0) / (4.0 * np.pi)))
    d = np.arange(radius + 1, dtype=np.float64)
    g64 = np.exp(-d[None, :] ** 2 / (2.0 * s64[:, None] ** 2))
    # one rounding to float32 of a double that may differ from numpy's in its last bits: half an ulp of float32 and a little
    assert np.allclose(sigma, s64, rtol=2.0 ** -23, atol=0)
    assert np.allclose(g, g64, rtol=2.0 ** -23, atol=2.0 ** -149)
    assert (g[:, 0] == 1).all() and (np.diff(g, axis=1) <= 0).all() and (np.diff(sigma) >= 0).all()
    assert sigma.max() <= radius / 2.0
    rs, rg = R.tables(R.P0, gain, radius)
    assert np.allclose(sigma, rs, rtol=2.0 ** -23, atol=0) and np.allclose(g, rg, rtol=2.0 ** -23, atol=2.0 ** -149)


def test_the_width_law_equalises_the_noise():
    """sigma_k below the cap: 4 pi sigma^2 = gain^2 expm1(e_k) pixels"""
    sigma, _ = B.starvation_filter_tables((0.0, 1.0, 4))
    k = np.arange(64)
    free = sigma < 2.0
    assert free.sum() > 40
    assert np.allclose(4 * np.pi * sigma[free].astype(np.float64) ** 2, np.expm1((k[free] + 0.5) / 16.0), rtol=1e-6)


@pytest.mark.parametrize("setting", [(np.nan, 1.0, 3), (np.inf, 1.0, 3), (-np.inf, 1.0, 3), (3.0, np.nan, 3), (3.0, np.inf, 3), (3.0, 0.0, 3),
                                     (3.0, -1.0, 3), (3.0, 1.0, 0), (3.0, 1.0, 5), (3.0, 1.0, 2 ** 32 - 1)])
def test_the_check_refuses(setting):
    for call in (lambda: B.starvation_filter_check(setting, 8, 8), lambda: B.starvation_filter_tables(setting),
                 lambda: B.starvation_filter_host(setting, np.zeros((8, 8), np.float32))):
        with pytest.raises(B.ParisHipError) as e:
            call()
        assert e.value.status == _lib.ERROR_INVALID_ARGUMENT


def test_the_check_s_other_refusals_and_its_bytes():
    L = _lib.load()
    assert L.paris_hip_starvation_filter_check(None, 8, 8, None) == _lib.ERROR_INVALID_ARGUMENT
    for dims in ((0, 8), (8, 0)):
        with pytest.raises(B.ParisHipError) as e:
            B.starvation_filter_check((3.0, 1.0, 3), *dims)
        assert e.value.status == _lib.ERROR_INVALID_ARGUMENT
    for dims in ((65536, 65536), (2 ** 32 - 1, 2)):
        with pytest.raises(B.ParisHipError) as e:
            B.starvation_filter_check((3.0, 1.0, 3), *dims)
        assert e.value.status == _lib.ERROR_UNSUPPORTED
    assert B.starvation_filter_check((3.0, 1.0, 3), 65535, 65537) > 0        # 2^32 - 1 pixels
    assert B.starvation_filter_check((-7.5, 1e-3, 1), 1, 1) == B.starvation_filter_check((3.0, 1.0, 4), 1, 1)
    head = 32 + 4 * 64 * 5
    assert B.starvation_filter_check((3.0, 1.0, 3), 2048, 2048) == head + _lib.STARVATION_FRAMES_MAX * 2048 * 2048 * 4
    assert abs(B.starvation_filter_check((3.0, 1.0, 3), 2048, 2048) - (128 << 20)) < (1 << 20)


WRONG = {
    "an in-place sweep that reads filtered values": dict(in_place=True),
    "edge replication instead of skipped taps": dict(replicate=True),
    "dx as the outer loop": dict(x_outer=True),
    "non-finite taps kept": dict(keep_non_finite=True),
}


@pytest.mark.parametrize("wrong", sorted(WRONG) + ["levels sampled at the lower bin edge"])
def test_the_inputs_tell_the_wrong_readings_apart(cases, wrong):
    frames, want = cases
    shape, radius = (65, 17), 2
    a = frames[shape]
    if wrong in WRONG:
        other = R.apply(a, R.P0, GAIN, radius, **WRONG[wrong])[0]
    else:
        other = R.apply(a, R.P0, GAIN, radius, g=R.tables(R.P0, GAIN, radius, centre=0.0)[1])[0]
    assert not R.same(other, want(shape, radius)[0]), wrong
