"""The ramp row filter (filter.hip, filter_fused.hip; src/openmp/filtering.cpp:52-219) restated in float64, the inputs the filter tests
share, deliberately broken forms of the statement, and what fp32 arithmetic costs it (the *CAL constants: measured with the oracle's
radix-2 fp32 transcription by tests/test_filter_host.py, which asserts them). No library call in here: this is what the oracle and the
device are compared against.

A frame is filtered the way the device does it: rows (2t, 2t + 1) are one complex signal, a last row without a partner is alone. A
row's error is therefore judged relative to the larger row of its pair (frame_error)."""
import numpy as np

SIZES = (8, 128, 512, 1024, 2048, 4096, 8192, 16384)   # filter lengths N
FUSED_SIZES = SIZES[3:]                                 # the radix-16 kernel of filter_fused.hip
TAUS = (0.1, 0.127, 0.2)
TAU = 0.2                                               # the apply tests' pixel pitch
WINDOW_RAMP, WINDOW_SHEPP_LOGAN = 0, 1
FILTER_TOL = 1e-5                                       # the white-noise tests' bar (tests/test_gpu_parity.py)


# ---- the statement --------------------------------------------------------------------------------------------------------------

def r32(n, tau):
    """r as make_filter_kernel and src/openmp/filtering.cpp:52-73 form it: fp32 operations, left to right"""
    f = np.float32
    t = f(tau)
    j = np.arange(n, dtype=np.int64) - (n - 2) // 2
    pi_f = f(np.pi)
    jj = (j * j).astype(np.float32)
    with np.errstate(divide="ignore"):
        odd = -(f(1) / (((f(2) * jj) * (pi_f * pi_f)) * (t * t)))
    r = np.where(j % 2 == 0, f(0), odd).astype(np.float32)
    r[j == 0] = (f(1) / f(8)) * (f(1) / (t * t))
    return r


def k64(n, tau, window=WINDOW_RAMP):
    """K = tau |rfft(r)|, n / 2 + 1 float64 values; window 1: times sinc(pi f / n) (the Shepp-Logan extension)"""
    k = float(np.float32(tau)) * np.abs(np.fft.rfft(r32(n, tau).astype(np.float64)))
    if window == WINDOW_SHEPP_LOGAN:
        x = np.pi * np.arange(1, n // 2 + 1, dtype=np.float64) / n
        k[1:] *= np.sin(x) / x
    return k


def apply(rows, k, n):
    """rows (..., dim_x) zero-padded to n, times K, back, the first dim_x samples; K: n / 2 + 1 values taken as float64"""
    rows = np.asarray(rows, np.float64)
    k = np.asarray(k, np.float64)
    assert k.shape == (n // 2 + 1,) and rows.shape[-1] <= n
    return np.fft.irfft(np.fft.rfft(rows, n, axis=-1) * k, n, axis=-1)[..., :rows.shape[-1]]


def full_k(k):
    """the n values of the real and even K"""
    return np.concatenate([k, k[-2:0:-1]])


def apply_packed(frame, kfull, n, padded=None):
    """the same through the packing: z = a + i b per row pair, times a K given for all n bins (which need not be even: then the rows
    of a pair leak into each other). padded: the (rows, n) transform input if it is not the zero-padded frame."""
    frame = np.asarray(frame, np.float64)
    rows, dim_x = frame.shape
    x = np.zeros((rows + (rows & 1), n))
    x[:rows, :dim_x] = frame
    if padded is not None:
        x[:rows] = padded
    z = np.fft.ifft(np.fft.fft(x[0::2] + 1j * x[1::2], axis=-1) * kfull, axis=-1)
    out = np.empty_like(x)
    out[0::2], out[1::2] = z.real, z.imag
    return out[:rows, :dim_x]


def frame_error(got, want):
    """the largest error of a frame: each pair (2t, 2t + 1) over the maximum of the pair, a lone last row over its own. Rows whose
    statement is all zero must be zero, and a row that holds a NaN or an infinity is infinitely wrong."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    worst = 0.0
    for t in range(0, want.shape[0], 2):
        scale = np.abs(want[t:t + 2]).max()
        d = np.abs(got[t:t + 2] - want[t:t + 2]).max()
        if not np.isfinite(d):   # a NaN or an infinity anywhere in the rows: never within any bound (max() would drop a NaN)
            return float("inf")
        worst = max(worst, (0.0 if d == 0 else np.inf) if scale == 0 else d / scale)
    return float(worst)


def bin_gains(rows, positions, amplitudes, n):
    """circular case (dim_x == n, an impulse per row): the DFT of each filtered row rotated by the impulse's position and divided by
    its amplitude: the gain the filter applied to every one of the n bins, complex"""
    f = np.arange(n, dtype=np.float64)
    out = []
    for row, p, a in zip(np.asarray(rows, np.float64), positions, amplitudes):
        out.append(np.fft.fft(row) * np.exp(2j * np.pi * ((f * p) % n) / n) / a)
    return np.array(out)


# ---- shapes -----------------------------------------------------------------------------------------------------------------------

def first_pass_stride(n):
    """NO of filter_rows_kernel: the first pass's radix-2^RF butterflies join pixels this far apart"""
    log2n = n.bit_length() - 1
    npass = (log2n + 3) // 4
    return n >> (log2n - 4 * (npass - 1))


ODD_WIDTHS = {1024: 300, 2048: 1000, 16384: 4097}


def padded_widths(n):
    """dim_x <= n / 2: the upper half of the transform's input is zero (HALF = true)"""
    return sorted({n // 2, n // 2 - 1} | ({ODD_WIDTHS[n]} if n in ODD_WIDTHS else set()))


def unpadded_widths(n):
    """n / 2 < dim_x <= n (HALF = false)"""
    return sorted({n // 2 + 1, 3 * n // 4, n})


# ---- inputs: (key, label, pair): key names the calibration figure, pair is (2, dim_x) float32 -------------------------------------

def impulse_positions(n, dim_x):
    no = first_pass_stride(n)
    return sorted({p for p in (0, 1, no - 1, no, dim_x // 2, dim_x - 2, dim_x - 1) if 0 <= p < dim_x})


def impulses(n, dim_x):
    pos = impulse_positions(n, dim_x)
    for i, p in enumerate(pos):
        q = pos[(i + 1) % len(pos)]
        pair = np.zeros((2, dim_x), np.float32)
        pair[0, p] = 1.0
        pair[1, q] = 0.75
        yield "impulses", "impulses at %d and %d" % (p, q), pair


def chord(dim_x, c, w):
    """the chord profile of an ellipse centred at c * dim_x with half width w * dim_x, 100 deep"""
    x = np.arange(dim_x, dtype=np.float64)
    return (2.0 * np.sqrt(np.maximum(0.0, 1.0 - ((x - c * dim_x) / (w * dim_x)) ** 2)) * 50.0).astype(np.float32)


ELLIPSE_A = (0.45, 0.35)
ELLIPSE_B = (0.60, 0.25)
TINY = 1e-3


def smooth(n, dim_x):
    a, b = chord(dim_x, *ELLIPSE_A), chord(dim_x, *ELLIPSE_B)
    yield "ellipses", "two ellipses", np.stack([a, b])
    yield "ellipse_zero", "ellipse and an all-zero partner", np.stack([a, np.zeros_like(a)])
    const = np.full(dim_x, 50.0, np.float32)
    ramp = (100.0 * (np.arange(dim_x, dtype=np.float64) + 1.0) / dim_x).astype(np.float32)
    yield "constant_ramp", "constant and linear ramp", np.stack([const, ramp])


def tiny_partner(n, dim_x):
    a, b = chord(dim_x, *ELLIPSE_A), chord(dim_x, *ELLIPSE_B)
    yield "tiny_partner", "ellipse and one at 1e-3 of its scale", np.stack([a, (b.astype(np.float64) * TINY).astype(np.float32)])


TONE_PAIRS = {   # key: the two bins of the pair, as functions of n
    "tones_low": (lambda n: 1, lambda n: 2),
    "tones_mid": (lambda n: 3, lambda n: n // 16 + 1),
    "tones_quarter": (lambda n: n // 4, lambda n: n // 4 + 1),
    "tones_nyquist": (lambda n: n // 2 - 9, lambda n: n // 2 - 1),
}


def tone_bins(n):
    """key -> (f, g) for the pairs whose bins lie strictly between DC and Nyquist (at n = 8 the pair below Nyquist does not)"""
    out = {key: (f(n), g(n)) for key, (f, g) in TONE_PAIRS.items()}
    return {key: fg for key, fg in out.items() if all(0 < b < n // 2 for b in fg)}


def tone(n, dim_x, f, phase):
    """cos(2 pi f x / n + phase) under a Hann window of dim_x samples"""
    x = np.arange(dim_x, dtype=np.float64)
    hann = 0.5 - 0.5 * np.cos(2.0 * np.pi * (x + 0.5) / dim_x)
    return (np.cos(2.0 * np.pi * ((f * x) % n) / n + phase) * hann).astype(np.float32)


def tones(n, dim_x):
    for key, (f, g) in tone_bins(n).items():
        yield key, "tones at bins %d and %d" % (f, g), np.stack([tone(n, dim_x, f, 0.3), tone(n, dim_x, g, 1.1)])


def pairs(n, dim_x, families=("impulses", "smooth", "tones")):
    for fam in families:
        yield from {"impulses": impulses, "smooth": smooth, "tones": tones, "tiny_partner": tiny_partner}[fam](n, dim_x)


def frames_of(pair):
    """a pair (a, b) as the frames the device is given: [a, b, a] and [b, a, b] (the pair both ways round, each row once as the lone
    last row of a three-row frame), [a] and [b] (the lone row of a one-row frame)"""
    a, b = pair
    return [("a b | a", np.stack([a, b, a])), ("b a | b", np.stack([b, a, b])), ("a", a[None].copy()), ("b", b[None].copy())]


def circular(n):
    """dim_x == n, no padding: a unit impulse at 1, one of 0.75 at n / 3, and the first again as the lone row -> frame, positions,
    amplitudes"""
    pos, amp = (1, n // 3, 1), (1.0, 0.75, 1.0)
    frame = np.zeros((3, n), np.float32)
    for r, (p, a) in enumerate(zip(pos, amp)):
        frame[r, p] = a
    return frame, pos, amp


# the two weighting geometries of the device tests: (h_min, v_min, d_sd, l_px_row, l_px_col) of paris_hip_weight for a frame of dim_x
# columns. "ordinary": the detector centred 1.5 pixels off the axis; "h0": column 0 at h = 0 exactly (l_px_row / 2 + h_min == 0), the
# weight's maximum at the row's first pixel
def weight_constants(which, dim_x, rows=3):
    f = np.float32
    l_row, l_col = f(TAU), f(0.25)
    v_min = float(f(-0.75) * l_col - (f(rows) * l_col) / f(2))
    if which == "h0":
        return (float(-(l_row / f(2))), v_min, 300.0, float(l_row), float(l_col))
    assert which == "ordinary"
    return (float(f(1.5) * l_row - (f(dim_x) * l_row) / f(2)), v_min, 300.0, float(l_row), float(l_col))


WEIGHTINGS = ("ordinary", "h0")


def width_key(key, n, dim_x, weighting=None):
    """a row that fills the whole transform is its own case: without padding a smooth row has no edge inside the transform, the ramp
    leaves little of it, and the same rounding is a larger part of what is left. So is a weighted row: the weight bends a constant,
    whose raw transform is exact, into a smooth bump"""
    return key + ("/full" if dim_x == n else "") + ("/weighted" if weighting is not None else "")


def plan(n, weightings=True):
    """every frame the device tests filter with a transform of n, and the host test calibrates: (key, label, dim_x, raw frame, weighting
    or None). All families at every width raw; from n = 1024 the smooth rows and the impulses once more under each weighting. (White
    noise, the circular case and the tiny partner are planned by their own tests.)"""
    widths = padded_widths(n) + unpadded_widths(n)
    for dim_x in widths:
        for key, label, pair in pairs(n, dim_x):
            for how, frame in frames_of(pair):
                yield width_key(key, n, dim_x), "%s, %d of %d, rows %s" % (label, dim_x, n, how), dim_x, frame, None
    if weightings and n >= 1024:
        for dim_x in widths:
            for key, label, pair in pairs(n, dim_x, ("smooth", "impulses")):
                for how, frame in frames_of(pair):
                    for w in WEIGHTINGS:
                        yield width_key(key, n, dim_x, w), "%s, %d of %d, rows %s, weighted (%s)" % (label, dim_x, n, how, w), dim_x, frame, w


# ---- deliberately broken statements -----------------------------------------------------------------------------------------------

def _swapped(k, i, j):
    k = np.array(k, np.float64)
    k[[i, j]] = k[[j, i]]
    return k


def _with(k, i, v):
    k = np.array(k, np.float64)
    k[i] = v
    return k


# a broken K from the right one
K_ERRORS = {
    "K[N/4] and K[N/4+1] exchanged": lambda k, n: _swapped(k, n // 4, n // 4 + 1),
    "two bins exchanged 8 below Nyquist": lambda k, n: _swapped(k, n // 2 - 8, n // 2 - 9),
    "DC bin multiplied by 0": lambda k, n: _with(k, 0, 0.0),
    "K[0] := K[1]": lambda k, n: _with(k, 0, k[1]),
}
MODEL_ERRORS = ("upper half of K shifted by one bin", "pixel dim_x - 1 dropped", "pixel dim_x read as column 0")
ERRORS = tuple(K_ERRORS) + MODEL_ERRORS
WHITE_BLIND = tuple(K_ERRORS)[:3]   # what the white-noise bar misses at N = 16384


def broken_apply(error, frame, k, n):
    """the filtered frame under one of ERRORS"""
    frame = np.asarray(frame, np.float64)
    rows, dim_x = frame.shape
    if error in K_ERRORS:
        return apply(frame, K_ERRORS[error](k, n), n)
    kf = full_k(np.asarray(k, np.float64))
    if error == MODEL_ERRORS[0]:
        kb = kf.copy()
        kb[n // 2 + 1:] = kf[n // 2:-1]   # bin n - f gets K[f + 1]
        return apply_packed(frame, kb, n)
    padded = np.zeros((rows, n))
    padded[:, :dim_x] = frame
    if error == MODEL_ERRORS[1]:
        padded[:, dim_x - 1] = 0.0
    else:
        assert error == MODEL_ERRORS[2]
        if dim_x < n:
            padded[:, dim_x] = frame[:, 0]
    return apply_packed(frame, kf, n, padded)


# ---- what fp32 costs: the oracle (an independent fp32 radix-2 transcription, twiddles rounded from double) against this module,
#      measured by tests/test_filter_host.py ------------------------------------------------------------------------------------------

# max_f |K_fp32[f] - K64[f]| / K_max over TAUS and both windows (the window in fp32 as make_filter_kernel forms it)
KCAL = {8: 4.950e-08, 128: 1.611e-07, 512: 3.117e-07, 1024: 3.515e-07, 2048: 3.104e-07, 4096: 3.211e-07, 8192: 3.761e-07, 16384: 3.865e-07}
# circular: the largest |gain[f] - K[f]| / K_max over all n bins and the three rows, K the oracle's own
GAINCAL = {8: 1.061e-07, 128: 2.051e-07, 512: 2.127e-07, 1024: 2.134e-07, 2048: 2.116e-07, 4096: 2.920e-07, 8192: 2.969e-07, 16384: 3.835e-07}
# max frame_error of the oracle's rows against apply() with the oracle's own K, over every width and frame the device tests use at
# that N (padded_widths, unpadded_widths; frames_of). ".../full": dim_x == N; ".../weighted": from N = 1024, the same frames under
# either weighting, a case of their own (width_key).
# The smooth figures grow with N because the ramp leaves ever less of a smooth row while the rounding of its large low bins leaks
# into all the others: a lone tone in bin 1 keeps about K[1] / K_max = 2 / N of its amplitude.
CAL = {
    "white": {8: 1.434e-07, 128: 3.699e-07, 512: 2.509e-07, 1024: 2.602e-07, 2048: 2.868e-07, 4096: 3.198e-07, 8192: 3.388e-07, 16384: 3.958e-07},
    "impulses": {8: 1.125e-07, 128: 1.366e-07, 512: 1.058e-07, 1024: 1.041e-07, 2048: 1.054e-07, 4096: 1.672e-07, 8192: 1.699e-07, 16384: 1.708e-07},
    "ellipses": {8: 1.122e-07, 128: 1.174e-06, 512: 2.482e-06, 1024: 5.057e-06, 2048: 6.879e-06, 4096: 1.099e-05, 8192: 1.520e-05, 16384: 2.239e-05},
    "ellipse_zero": {8: 1.122e-07, 128: 1.174e-06, 512: 2.482e-06, 1024: 5.057e-06, 2048: 6.879e-06, 4096: 1.099e-05, 8192: 1.520e-05, 16384: 2.239e-05},
    "constant_ramp": {8: 1.241e-07, 128: 1.908e-07, 512: 2.908e-07, 1024: 3.917e-07, 2048: 3.911e-07, 4096: 4.699e-07, 8192: 4.556e-07, 16384: 5.466e-07},
    "tones_low": {8: 1.474e-07, 128: 2.580e-06, 512: 1.362e-05, 1024: 3.584e-05, 2048: 6.585e-05, 4096: 1.554e-04, 8192: 3.428e-04, 16384: 7.327e-04},
    "tones_mid": {8: 1.264e-07, 128: 1.077e-06, 512: 5.803e-06, 1024: 1.256e-05, 2048: 3.621e-05, 4096: 6.438e-05, 8192: 1.365e-04, 16384: 3.280e-04},
    "tones_quarter": {8: 1.090e-07, 128: 1.789e-07, 512: 2.768e-07, 1024: 2.534e-07, 2048: 3.246e-07, 4096: 3.200e-07, 8192: 3.555e-07, 16384: 3.453e-07},
    "impulses/full": {8: 1.125e-07, 128: 1.366e-07, 512: 1.058e-07, 1024: 1.041e-07, 2048: 1.054e-07, 4096: 1.672e-07, 8192: 1.699e-07, 16384: 1.708e-07},
    "ellipses/full": {8: 1.744e-07, 128: 1.372e-06, 512: 2.870e-06, 1024: 5.453e-06, 2048: 9.522e-06, 4096: 1.115e-05, 8192: 1.659e-05, 16384: 2.763e-05},
    "ellipse_zero/full": {8: 1.744e-07, 128: 1.372e-06, 512: 2.870e-06, 1024: 5.453e-06, 2048: 9.522e-06, 4096: 1.115e-05, 8192: 1.659e-05, 16384: 2.763e-05},
    "constant_ramp/full": {8: 9.865e-08, 128: 5.917e-08, 512: 1.132e-07, 1024: 1.117e-07, 2048: 6.653e-08, 4096: 1.265e-07, 8192: 8.015e-08, 16384: 1.454e-07},
    "tones_low/full": {8: 9.992e-08, 128: 4.229e-06, 512: 1.534e-05, 1024: 3.176e-05, 2048: 7.200e-05, 4096: 1.463e-04, 8192: 3.720e-04, 16384: 9.544e-04},
    "tones_mid/full": {8: 6.901e-08, 128: 9.325e-07, 512: 6.170e-06, 1024: 1.287e-05, 2048: 3.505e-05, 4096: 5.593e-05, 8192: 1.674e-04, 16384: 3.070e-04},
    "tones_quarter/full": {8: 8.892e-08, 128: 1.543e-07, 512: 2.140e-07, 1024: 2.644e-07, 2048: 2.626e-07, 4096: 2.900e-07, 8192: 3.256e-07, 16384: 3.624e-07},
    "tiny_partner": {8: 8.137e-08, 128: 8.839e-07, 512: 1.957e-06, 1024: 2.497e-06, 2048: 4.332e-06, 4096: 7.047e-06, 8192: 1.032e-05, 16384: 1.974e-05},
    "circular": {8: 1.125e-07, 128: 1.366e-07, 512: 7.931e-08, 1024: 9.789e-08, 2048: 8.535e-08, 4096: 8.710e-08, 8192: 8.441e-08, 16384: 1.281e-07},
    "tones_nyquist": {128: 1.944e-07, 512: 2.041e-07, 1024: 2.549e-07, 2048: 4.733e-07, 4096: 2.593e-07, 8192: 3.695e-07, 16384: 3.164e-07},
    "tones_nyquist/full": {128: 1.596e-07, 512: 1.968e-07, 1024: 2.410e-07, 2048: 2.171e-07, 4096: 2.871e-07, 8192: 3.279e-07, 16384: 2.837e-07},
    "ellipses/weighted": {1024: 7.648e-06, 2048: 7.711e-06, 4096: 1.207e-05, 8192: 2.642e-05, 16384: 7.487e-05},
    "ellipse_zero/weighted": {1024: 7.648e-06, 2048: 7.542e-06, 4096: 1.216e-05, 8192: 3.093e-05, 16384: 7.487e-05},
    "constant_ramp/weighted": {1024: 6.595e-07, 2048: 8.987e-07, 4096: 1.311e-06, 8192: 1.302e-06, 16384: 2.006e-06},
    "impulses/weighted": {1024: 2.785e-07, 2048: 2.548e-07, 4096: 2.977e-07, 8192: 2.653e-07, 16384: 2.930e-07},
    "ellipses/full/weighted": {1024: 5.370e-06, 2048: 1.091e-05, 4096: 1.413e-05, 8192: 3.720e-05, 16384: 1.247e-04},
    "ellipse_zero/full/weighted": {1024: 5.694e-06, 2048: 1.091e-05, 4096: 1.445e-05, 8192: 3.720e-05, 16384: 1.278e-04},
    "constant_ramp/full/weighted": {1024: 2.843e-04, 2048: 4.413e-04, 4096: 4.427e-04, 8192: 6.586e-04, 16384: 1.093e-03},
    "impulses/full/weighted": {1024: 2.031e-07, 2048: 2.226e-07, 4096: 2.626e-07, 8192: 2.335e-07, 16384: 1.938e-07},
}


def bound(key, n):
    """a case's bound: twice the larger of its own figure and white noise's at that N. Two covers an FFT of another radix, whose
    roundings differ from the oracle's but are not more."""
    return 2.0 * max(CAL[key][n], CAL["white"][n])


def k_bound(n):
    return 2.0 * KCAL[n]


def gain_bound(n):
    return 2.0 * GAINCAL[n]
