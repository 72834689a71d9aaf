"""The row filter's checks calibrated on the CPU (tests/filter_rule.py): what the oracle's fp32 radix-2 transcription costs the float64
statement per filter length and input family (the *CAL constants the device is bounded with), and proof that the checks can fail: every
deliberate error of filter_rule.ERRORS moves one of the non-white families by at least four times its bound, while three of them pass the
white-noise bar at N = 16384. The oracle is the calibration instrument here, never the device."""
import numpy as np
import pytest

import filter_rule as R
from filter_instrument import measure_cal, measure_circular, measure_kcal, oracle_filter, white


def within_a_tenth(measured, recorded):
    return recorded * 0.9 <= measured <= recorded * 1.1


# ---- the statement is the oracle's -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", R.SIZES)
def test_r_is_the_oracles_bit_for_bit(oracle, n):
    for tau in R.TAUS + (0.5,):
        assert np.array_equal(R.r32(n, tau).view(np.uint32), oracle.make_filter_real(n, tau).view(np.uint32)), tau


def test_the_statement_in_its_own_terms():
    """apply() through the packing is apply(); the circular gains of apply() are K; a windowed K is the ramp's times sinc"""
    n = 512
    k = R.k64(n, R.TAU)
    rng = np.random.default_rng(5)
    frame = rng.standard_normal((3, 300))
    assert np.abs(R.apply_packed(frame, R.full_k(k), n) - R.apply(frame, k, n)).max() < 1e-12 * np.abs(R.apply(frame, k, n)).max()
    circ, pos, amp = R.circular(n)
    gains = R.bin_gains(R.apply(circ, k, n), pos, amp, n)
    assert np.abs(gains - R.full_k(k)[None, :]).max() < 1e-12 * k.max()
    sl = R.k64(n, R.TAU, R.WINDOW_SHEPP_LOGAN)
    assert sl[0] == k[0] and abs(sl[n // 2] / k[n // 2] - 2 / np.pi) < 1e-15
    # a NaN or an infinity in a row is never within a bound, wherever it sits and whatever stands beside it
    want = np.ones((3, 8))
    for bad in (np.nan, np.inf, -np.inf):
        for row in range(3):
            got = want.copy()
            got[row, 5] = bad
            assert R.frame_error(got, want) == np.inf and not R.frame_error(got, want) <= max(R.bound(key, n) for key in R.CAL for n in R.CAL[key])
    assert R.frame_error(want, want) == 0.0
    assert R.first_pass_stride(1024) == 256 and R.first_pass_stride(4096) == 256 and R.first_pass_stride(8192) == 4096
    assert R.first_pass_stride(16384) == 4096 and R.first_pass_stride(2048) == 256


# ---- calibration -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", R.SIZES)
def test_calibration_figures(oracle, n):
    """KCAL, GAINCAL and CAL are what this measures"""
    kcal = measure_kcal(oracle, n)
    gaincal = measure_circular(oracle, n)[0]
    cal = measure_cal(oracle, n)
    k32, want = oracle.make_filter(n, R.TAU).astype(np.float64), R.k64(n, R.TAU)
    print("filter calibration, N = %d: KCAL %.3e (recorded %.3e), GAINCAL %.3e (%.3e); the oracle's K[0] %.3e and K[1] %.3e from float64, relative"
          % (n, kcal, R.KCAL[n], gaincal, R.GAINCAL[n], abs(k32[0] / want[0] - 1), abs(k32[1] / want[1] - 1)))
    for key in sorted(cal):
        print("filter calibration, N = %d, %-13s: %.3e of the pair's maximum (recorded %.3e), bound %.3e" % (n, key, cal[key], R.CAL[key][n], R.bound(key, n)))
    assert within_a_tenth(kcal, R.KCAL[n]) and within_a_tenth(gaincal, R.GAINCAL[n])
    assert sorted(cal) == sorted(key for key in R.CAL if n in R.CAL[key])
    for key in cal:
        assert within_a_tenth(cal[key], R.CAL[key][n]), key


# ---- conditions -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", R.FUSED_SIZES)
def test_every_deliberate_error_moves_a_non_white_family_four_bounds(n):
    """with the float64 statement alone: the frames of filter_rule.plan at the reference's width and at dim_x == N"""
    k = R.k64(n, R.TAU)
    frames = [(key, label, frame) for key, label, dim_x, frame, w in R.plan(n, weightings=False) if dim_x in (n // 2, n)]
    rights = [R.apply(frame, k, n) for _, _, frame in frames]
    for error in R.ERRORS:
        best = (0.0, None)
        for (key, label, frame), right in zip(frames, rights):
            factor = R.frame_error(R.broken_apply(error, frame, k, n), right) / R.bound(key, n)
            if factor > best[0] and np.isfinite(factor):
                best = (factor, label)
        print("N = %5d, %-40s: caught by %s, %.3g times its bound" % (n, error, best[1], best[0]))
        assert best[0] >= 4.0, error


@pytest.mark.parametrize("n", R.FUSED_SIZES)
def test_one_impulse_pair_separates_every_bin_from_its_neighbours(n):
    k = R.k64(n, R.TAU)
    step = np.abs(np.diff(k)).min() / k.max()
    print("N = %5d: smallest neighbour step %.3e of K_max, gain bound %.3e: margin %.0f" % (n, step, R.gain_bound(n), step / R.gain_bound(n)))
    assert R.gain_bound(n) < step / 4
    # ... and every K error moves a bin's gain by four gain bounds or more (a zeroed DC bin the least: K[0] / K_max)
    for error, make in R.K_ERRORS.items():
        moved = np.abs(make(k, n) - k).max() / k.max()
        print("N = %5d, %-36s: a bin's gain moves by %.3e of K_max, %.0f gain bounds" % (n, error, moved, moved / R.gain_bound(n)))
        assert moved >= 4 * R.gain_bound(n), error


def test_what_the_white_noise_bar_alone_misses(oracle):
    """at N = 16384 three of the errors stay below FILTER_TOL of the frame's maximum on the white frame, oracle and float64 alike"""
    n = 16384
    frame = white(oracle, n // 2)
    k32 = oracle.make_filter(n, R.TAU)
    k = R.k64(n, R.TAU)
    right = R.apply(frame, k, n)
    for error in R.K_ERRORS:
        moved = np.abs(R.broken_apply(error, frame, k, n) - right).max() / np.abs(right).max()
        through_oracle = oracle_filter(oracle, frame, R.K_ERRORS[error](k32, n).astype(np.float32), n)
        seen_by_the_suite = np.abs(through_oracle - right).max() / np.abs(right).max()
        print("N = 16384, white, %-36s: %.3e of the frame's maximum in float64, %.3e through the oracle (bar %.0e)"
              % (error, moved, seen_by_the_suite, R.FILTER_TOL))
        assert (moved < R.FILTER_TOL and seen_by_the_suite < R.FILTER_TOL) == (error in R.WHITE_BLIND), error
