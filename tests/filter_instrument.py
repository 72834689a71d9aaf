"""The row filter tests' instrument: the CPU oracle (oracle/, an independent fp32 radix-2 transcription of the filter) applied to the
frames of tests/filter_rule.py, and the figures measured with it. The oracle module is passed in (the `oracle` fixture); this is shared
by tests/test_filter_host.py, which asserts the figures, and tests/test_gpu_filter_bins.py, which needs the weighted rows and the fp32 K.
The oracle is the calibration instrument, never the device."""
import numpy as np

import filter_rule as R

F32 = np.float32


def weighted(O, frame, which):
    """the frame as the transform sees it under a weighting: the oracle's bit-exact weight with filter_rule.weight_constants"""
    p = np.ascontiguousarray(frame, np.float32).copy()
    O.lib().po_weight(O._f32(p), p.shape[1], p.shape[0], *R.weight_constants(which, p.shape[1]))
    return p


def seen(O, frame, weighting):
    return np.ascontiguousarray(frame, np.float32) if weighting is None else weighted(O, frame, weighting)


def white(O, dim_x, rows=3):
    """the white-noise frame of tests/test_gpu_parity.py::test_apply_filter"""
    return O.lcg_projection(dim_x, rows, 11) - F32(0.25)


def oracle_filter(O, frame, k32, n):
    return O.apply_filter(np.ascontiguousarray(frame, np.float32).copy(), k32, n)


def k_fp32(O, n, tau, window):
    """the oracle's K; the window in fp32 as make_filter_kernel forms it: x, sinf(x) / x and the product rounded once each (the sine
    correctly rounded, from float64, so that the figure does not depend on the host's fp32 sine)"""
    k = O.make_filter(n, tau)
    if window == R.WINDOW_SHEPP_LOGAN:
        x = (F32(np.pi) * np.arange(1, n // 2 + 1, dtype=np.float32)) / F32(n)
        k[1:] = k[1:] * (np.sin(x.astype(np.float64)).astype(np.float32) / x)
    return k


def measure_kcal(O, n):
    worst = 0.0
    for tau in R.TAUS:
        for window in (R.WINDOW_RAMP, R.WINDOW_SHEPP_LOGAN):
            want = R.k64(n, tau, window)
            worst = max(worst, np.abs(k_fp32(O, n, tau, window) - want).max() / want.max())
    return float(worst)


def measure_circular(O, n):
    """-> (GAINCAL figure, the time-domain figure of the circular frame)"""
    frame, pos, amp = R.circular(n)
    k32 = O.make_filter(n, R.TAU)
    k = k32.astype(np.float64)
    got = oracle_filter(O, frame, k32, n)
    gain = np.abs(R.bin_gains(got, pos, amp, n) - R.full_k(k)[None, :]).max() / k.max()
    return float(gain), R.frame_error(got, R.apply(frame, k, n))


def measure_cal(O, n):
    """-> {key: figure} for every key of filter_rule.CAL"""
    k32 = O.make_filter(n, R.TAU)
    k = k32.astype(np.float64)
    out = {}

    def note(key, frame):
        out[key] = max(out.get(key, 0.0), R.frame_error(oracle_filter(O, frame, k32, n), R.apply(frame, k, n)))

    for dim_x in R.padded_widths(n) + R.unpadded_widths(n):
        note("white", white(O, dim_x))
    for key, _, _, frame, weighting in R.plan(n):
        note(key, seen(O, frame, weighting))
    for _, _, pair in R.tiny_partner(n, n // 2):
        for _, frame in R.frames_of(pair)[:2]:
            note("tiny_partner", frame)
    out["circular"] = measure_circular(O, n)[1]
    return out
