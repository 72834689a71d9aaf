"""The host side of the detector lag correction (paris_hip_lag_model_check / _coefficients / _correct_host): no
device, no ctx -- the library's rule against its numpy restatement (tests/lag_rule.py) bit for bit, the wrong restatements that show
the comparison can fail, split invariance, the coefficients, every refusal, the physics in float64 and the precision of the fp32
rule."""
import ctypes as C

import numpy as np
import pytest

import lag_rule as R
from paris_amd import _lib
from paris_amd import backend as B

INV = _lib.ERROR_INVALID_ARGUMENT


@pytest.fixture(scope="module")
def frames():
    f = R.special_frames((7, 9, 37), seed=1)
    assert np.isnan(f).any() and np.isinf(f).any() and (f < 0).any() and np.count_nonzero((f != 0) & (np.abs(f) < 1.1754944e-38)) >= 4
    assert np.count_nonzero(R.bits(f) == 0x80000000) >= 1 and np.count_nonzero(R.bits(f) == 0) >= 1
    assert np.count_nonzero(R.bits(f) == R.NAN_PAYLOAD) >= 1
    f.setflags(write=False)
    return f


@pytest.mark.parametrize("start", R.STARTS)
@pytest.mark.parametrize("with_dark", [False, True])
@pytest.mark.parametrize("terms", [1, 2, 3, 4])
def test_the_rule_equals_the_restatement_bit_for_bit(frames, terms, with_dark, start):
    dark = R.dark_frame(frames.shape[1:]) if with_dark else None
    got, state, started = B.lag_correct_host(R.MODELS[terms], frames, dark=dark, start=start)
    want, want_state, _ = R.correct(R.MODELS[terms], frames, dark=dark, start=start)
    assert started and R.same_pixels(got, want) and R.same_pixels(state, want_state)
    assert np.isfinite(state).all()                       # no bad sample reached the state
    bad = ~np.isfinite(frames - (0 if dark is None else dark))
    assert bad.any() and np.array_equal(R.bits(got)[bad], R.bits(frames)[bad])      # stored unchanged, payload included


@pytest.mark.parametrize("wrong", R.WRONG)
def test_each_wrong_restatement_differs(frames, wrong):
    dark = R.dark_frame(frames.shape[1:])
    got, state, _ = B.lag_correct_host(R.MODELS[4], frames, dark=dark, start="steady")
    bad, bad_state, _ = R.correct(R.MODELS[4], frames, dark=dark, start="steady", wrong=wrong)
    assert not R.same_pixels(got, bad) or not R.same_pixels(state, bad_state)


@pytest.mark.parametrize("start", R.STARTS)
def test_split_invariance(frames, start):
    dark = R.dark_frame(frames.shape[1:])
    one, one_state, _ = B.lag_correct_host(R.MODELS[3], frames, dark=dark, start=start)
    for cuts in ((1,) * 7, (3, 4)):
        state, started, at, parts = None, False, 0, []
        for n in cuts:
            out, state, started = B.lag_correct_host(R.MODELS[3], frames[at:at + n], dark=dark, start=start, state=state, started=started)
            parts.append(out)
            at += n
        assert np.array_equal(R.bits(np.concatenate(parts)), R.bits(one)) and np.array_equal(R.bits(state), R.bits(one_state)), cuts


@pytest.mark.parametrize("terms", [1, 2, 3, 4])
def test_the_coefficients_are_the_float64_values_rounded_once(terms):
    g, c, w, inv_b, b0 = B.lag_coefficients(R.MODELS[terms])
    wg, wc, ww, winv, wb0 = R.coefficients(R.MODELS[terms])
    for got, want in ((g, wg), (c, wc), (w, ww), (inv_b, winv)):
        assert np.array_equal(R.bits(got), R.bits(want))
    assert b0 == wb0 and (terms != 4 or abs(b0 - 0.9503) < 1e-4)
    # the slots beyond `terms` are zeroed
    m = B._lag_setting(R.MODELS[terms], "steady")
    arrays = [(C.c_float * 4)(9, 9, 9, 9) for _ in range(3)]
    assert _lib.load().paris_hip_lag_coefficients(C.byref(m), *arrays, None, None) == 0
    assert all(list(a)[terms:] == [0.0] * (4 - terms) for a in arrays)


def test_every_refusal_of_the_check():
    L = _lib.load()
    good = list(R.MODELS[4])
    B.lag_model_check(good)
    B.lag_model_check(good, start="rest")
    assert L.paris_hip_lag_model_check(None) == INV
    nan, inf = float("nan"), float("inf")
    one_ulp_up = float(np.nextafter(np.float32(1), np.float32(2)))
    refused = [[], good + [(1e-3, 0.5)],                                    # terms outside 1 .. 4
               [(nan, 1.0)], [(inf, 1.0)], [(0.0, 1.0)], [(-1e-3, 1.0)],    # b_n
               [(1e-3, nan)], [(1e-3, inf)], [(1e-3, 0.0)], [(1e-3, -1.0)],  # a_n
               good[:2] + [(1e-3, nan)],                                    # ... in a later term
               [(1.0, 40.0)],            # b_0 exactly 0: exp(-40) vanishes beside 1 in double, so b_0 = 1 - 1 / 1
               [(one_ulp_up, 40.0)],     # b_0 slightly negative: -1.2e-7
               [(0.5, 0.5)]]             # b_0 = 1 - 0.5 / 0.393: negative
    for bad in refused:
        with pytest.raises(B.ParisHipError) as e:
            B.lag_model_check(bad)
        assert e.value.status == INV, bad
        with pytest.raises(B.ParisHipError):
            B.lag_coefficients(bad)
        with pytest.raises(B.ParisHipError):
            B.lag_correct_host(bad, np.ones((1, 4), np.float32))
    for start in (2, -1, "warm"):                                           # an unknown start
        with pytest.raises(B.ParisHipError) as e:
            B.lag_model_check(good, start=start)
        assert e.value.status == INV
    B.lag_model_check([(float(np.nextafter(np.float32(1), np.float32(0))), 40.0)])  # b_0 = 6e-8 > 0 passes
    m = B._lag_setting(good, "steady")
    g = (C.c_float * 4)()
    assert L.paris_hip_lag_coefficients(C.byref(m), None, g, g, None, None) == INV
    flag, px = C.c_int(0), (C.c_float * 4)()
    assert L.paris_hip_lag_correct_host(C.byref(m), None, None, px, C.byref(flag), 1, 1) == INV
    assert L.paris_hip_lag_correct_host(C.byref(m), None, px, None, C.byref(flag), 1, 1) == INV
    assert L.paris_hip_lag_correct_host(C.byref(m), None, px, px, None, 1, 1) == INV
    assert L.paris_hip_lag_correct_host(C.byref(m), None, None, None, None, 0, 5) == 0    # nothing to do


# ---- physics, in float64 ----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def sweep():
    x = R.edge_sweep()                                 # 400 frames x 64 pixels, 60000 -> 3000 counts
    y = R.forward64(R.MODELS[4], x)
    return x, y


def test_the_inverse_of_the_forward_model_returns_the_input(sweep):
    x, y = sweep
    back = R.inverse64(R.MODELS[4], y)
    assert np.abs((back - x) / x).max() <= 1e-12       # an exact algebraic inverse: 6e-16 measured
    rest = R.inverse64(R.MODELS[4], R.forward64(R.MODELS[4], x, "rest"), "rest")
    assert np.abs((rest - x) / x).max() <= 1e-12


def test_the_input_has_lag_in_it(sweep):
    x, y = sweep
    assert np.abs(y - x).max() > 0.01 * R.FULL_SCALE   # 2.8 % of full scale measured


def test_precision_of_the_fp32_rule_on_the_edge_sweep(sweep):
    """against the float64 inverse of the same fp32 input. The host rule measures 1.8e-7 of full scale (0.011 counts) here -- a
    numpy prototype without fmaf gave 2.0e-7; the bound is four times the measured value, which covers rounding over other seeds
    (1.74e-7 .. 1.82e-7 over five)."""
    _, y = sweep
    y32 = y.astype(np.float32)
    got, _, _ = B.lag_correct_host(R.MODELS[4], y32)
    err = np.abs(got.astype(np.float64) - R.inverse64(R.MODELS[4], y32.astype(np.float64))).max() / R.FULL_SCALE
    print("fp32 rule against the float64 inverse, 400 frames: %.3g of full scale" % err)
    assert err <= 4 * 1.8e-7


def test_precision_of_the_fp32_rule_over_4000_frames_without_drift():
    """a constant 30000 counts plus noise, 4000 frames: 0.0060 counts measured (the prototype: 0.007), the same in the first and the
    last 400 frames; the bound is four times that"""
    y32 = R.forward64(R.MODELS[4], R.constant_with_noise()).astype(np.float32)
    got, _, _ = B.lag_correct_host(R.MODELS[4], y32)
    err = np.abs(got.astype(np.float64) - R.inverse64(R.MODELS[4], y32.astype(np.float64)))
    print("fp32 rule against the float64 inverse, 4000 frames: %.3g counts (first 400: %.3g, last 400: %.3g)"
          % (err.max(), err[:400].max(), err[-400:].max()))
    assert err.max() <= 4 * 0.0061
    assert err[-400:].max() <= 2 * err[:400].max()     # no drift


def test_a_bad_sample_does_not_poison_its_pixel():
    rng = np.random.default_rng(9)
    f = rng.uniform(3000, 60000, (12, 5)).astype(np.float32)
    f[3, 0], f[3, 1], f[3, 2] = np.nan, np.inf, -np.inf
    dark = np.full(5, 1000, np.float32)
    got, state, _ = B.lag_correct_host(R.MODELS[4], f, dark=dark)
    want, _, _ = R.correct(R.MODELS[4], f, dark=dark)
    assert np.array_equal(R.bits(got[3, :3]), R.bits(f[3, :3]))
    assert np.isfinite(got[4:]).all() and np.isfinite(state).all()
    assert np.array_equal(R.bits(got[4:]), R.bits(want[4:]))
