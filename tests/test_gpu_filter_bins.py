"""The row filter on the device per bin, per position and on smooth rows, against the float64 statement of tests/filter_rule.py.

K-making and K-applying are judged separately: make_filter against K64 per bin (bound 2 KCAL), and every filtered row against
apply(...) with the K the device itself made, read back and promoted, normalised by the larger row of its pair (bound: twice the larger
of the case's own oracle figure and white noise's, filter_rule.bound; calibrated by tests/test_filter_host.py, which also shows that each
deliberate error of filter_rule.ERRORS breaks one of these cases by four bounds or more). Both kernels: variant 0 (radix-16 passes,
filter_fused.hip, N >= 1024), variant 1 (radix-2 in LDS, filter.hip) and, in the experiments build, variant 2 (the first radix-16
kernel). PARIS_FILTER_BINS_REPORT=<file>: the measured figures are appended there (profiles/r23_filter_bins.txt is such a run)."""
import os

import numpy as np
import pytest

import filter_instrument as H
import filter_rule as R
import row_extension_rule as RX
from paris_amd import _lib
from paris_amd import backend as B

pytestmark = pytest.mark.gpu

RADIX2_SIZES = (8, 128, 512, 1024, 16384)   # variant 1: the lengths only it serves, and the shortest and longest it shares
REPORT = []


def report(line):
    print(line)
    REPORT.append(line)


@pytest.fixture(scope="module")
def be():
    with B.Backend(0) as b:
        yield b
    path = os.environ.get("PARIS_FILTER_BINS_REPORT")
    if path:
        with open(path, "a") as f:
            f.write("library: %s\n" % ("experiments build" if _lib.has_experiments() else "product build"))
            f.write("\n".join(REPORT) + "\n")


@pytest.fixture(scope="module")
def filters(be):
    """n -> (the device's K for TAU, its values read back and promoted)"""
    made = {}

    def get(n):
        if n not in made:
            k = be.make_filter(n, R.TAU)
            made[n] = (k, be.filter_to_host(k).astype(np.float64))
        return made[n]

    yield get
    for k, _ in made.values():
        be.free(k)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint16)


def read(be, d):
    h = be.make_projection_host(d.dim_x, d.dim_y)
    be.copy_d2h(d, h)
    return h.buf.copy()


def load(be, frame):
    frame = np.ascontiguousarray(frame, np.float32)
    return B.load(be, B.Projection(frame.copy(), frame.shape[1], frame.shape[0]))


def product_refuses_variant(be, variant):
    """variant 2 lives in the experiments build only (tests/test_gpu_parity.py::product_refuses)"""
    if variant != 2 or _lib.has_experiments():
        return False
    with pytest.raises(_lib.ParisHipError) as e:
        be.set_filter_variant(2)
    assert e.value.status == _lib.ERROR_UNSUPPORTED
    return True


def filtered(be, frame, k, n, variant=0):
    """paris_hip_apply_filter on a frame"""
    d = load(be, frame)
    be.set_filter_variant(variant)
    try:
        be.apply_filter(d, k, n, frame.shape[0])
    finally:
        be.set_filter_variant(0)
    out = read(be, d)
    be.free(d)
    return out


def weight_filtered(be, frame, k, n, weighting):
    """paris_hip_weight_filter_rows on a whole frame"""
    d = load(be, frame)
    be.weight_filter_rows(d, 0, frame.shape[0], *R.weight_constants(weighting, frame.shape[1]), k, n)
    out = read(be, d)
    be.free(d)
    return out


class Worst:
    """the largest figure per key, as a fraction of its bound too"""

    def __init__(self):
        self.by_key = {}

    def note(self, key, n, label, err):
        ratio = err / R.bound(key, n)
        if key not in self.by_key or not ratio <= self.by_key[key][1]:   # (a NaN replaces whatever is stored, and then stays)
            self.by_key[key] = (err, ratio, label)

    def assert_all(self, what, n):
        bad = []
        for key, (err, ratio, label) in sorted(self.by_key.items()):
            line = ("%s, N = %5d, %-18s: %.3e of the pair's maximum, %.2f of its bound %.3e (oracle %.3e), worst at %s"
                    % (what, n, key, err, ratio, R.bound(key, n), R.CAL[key][n], label))
            report(line)
            if not ratio <= 1.0:
                bad.append(line)
        assert self.by_key and not bad, "\n".join(bad)


# ---- 1. K per bin -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", R.SIZES)
def test_k_per_bin_against_float64(be, oracle, n):
    for tau in R.TAUS:
        for window in (R.WINDOW_RAMP, R.WINDOW_SHEPP_LOGAN):
            k = be.make_filter(n, tau, window=window)
            got = be.filter_to_host(k).astype(np.float64)
            be.free(k)
            want = R.k64(n, tau, window)
            assert got.shape == want.shape
            err = np.abs(got - want) / want.max()
            ora = np.abs(H.k_fp32(oracle, n, tau, window) - want) / want.max()
            rel0, rel1 = abs(got[0] / want[0] - 1), abs(got[1] / want[1] - 1)
            o32 = H.k_fp32(oracle, n, tau, window).astype(np.float64)
            line = ("K per bin, N = %5d, tau %.3f, window %d: device %.3e of K_max at bin %d (oracle %.3e, bound %.3e); K[0] off by %.3e, K[1] by %.3e, "
                    "relative (oracle %.3e, %.3e)" % (n, tau, window, err.max(), int(err.argmax()), ora.max(), R.k_bound(n), rel0, rel1,
                                                      abs(o32[0] / want[0] - 1), abs(o32[1] / want[1] - 1)))
            report(line)
            assert err.max() <= R.k_bound(n), line


# ---- 2. every bin's gain and position ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant,n", [(0, n) for n in R.FUSED_SIZES] + [(1, n) for n in R.SIZES] + [(2, n) for n in R.FUSED_SIZES])
def test_every_bins_gain_is_the_devices_own_k(be, filters, variant, n):
    """dim_x == N, an impulse per row: a misplaced entry of the permuted K copy shows as a neighbour's gain in one bin"""
    if product_refuses_variant(be, variant):
        return
    k, k_dev = filters(n)
    frame, pos, amp = R.circular(n)
    got = filtered(be, frame, k, n, variant)
    gains = R.bin_gains(got, pos, amp, n)
    err = np.abs(gains - R.full_k(k_dev)[None, :]) / k_dev.max()
    time_err = R.frame_error(got, R.apply(frame, k_dev, n))
    line = ("every bin's gain, variant %d, N = %5d: %.3e of K_max at bin %d of row %d (oracle %.3e, bound %.3e); the rows %.3e of the pair's maximum (bound %.3e)"
            % (variant, n, err.max(), int(err.max(axis=0).argmax()), int(err.max(axis=1).argmax()), R.GAINCAL[n], R.gain_bound(n), time_err,
               R.bound("circular", n)))
    report(line)
    assert err.max() <= R.gain_bound(n), line
    assert time_err <= R.bound("circular", n), line


# ---- 3. the families, padded and unpadded, raw and weighted ---------------------------------------------------------------------------

@pytest.mark.parametrize("variant,n", [(0, n) for n in R.FUSED_SIZES] + [(1, n) for n in RADIX2_SIZES] + [(2, n) for n in R.FUSED_SIZES])
def test_rows_against_float64(be, filters, variant, n):
    """impulses, smooth rows and tones at every width of filter_rule.padded_widths (HALF = true) and unpadded_widths (HALF = false), each
    pair both ways round and each row as the lone last row of a three-row and of a one-row frame"""
    if product_refuses_variant(be, variant):
        return
    k, k_dev = filters(n)
    worst = {True: Worst(), False: Worst()}
    for key, label, dim_x, frame, _ in R.plan(n, weightings=False):
        got = filtered(be, frame, k, n, variant)
        worst[dim_x <= n // 2].note(key, n, label, R.frame_error(got, R.apply(frame, k_dev, n)))
    worst[True].assert_all("rows, variant %d, padded" % variant, n)
    worst[False].assert_all("rows, variant %d, unpadded" % variant, n)


@pytest.mark.parametrize("n", R.FUSED_SIZES)
def test_weighted_rows_against_float64(be, oracle, filters, n):
    """the smooth rows and the impulses through paris_hip_weight_filter_rows, against apply() of the oracle-weighted rows: an ordinary
    geometry, and one whose h_min puts column 0 at h = 0"""
    k, k_dev = filters(n)
    assert np.float32(R.weight_constants("h0", 300)[3]) / np.float32(2) + np.float32(R.weight_constants("h0", 300)[0]) == 0
    worst = {True: Worst(), False: Worst()}
    for key, label, dim_x, frame, weighting in R.plan(n):
        if weighting is None:
            continue
        got = weight_filtered(be, frame, k, n, weighting)
        want = R.apply(H.weighted(oracle, frame, weighting), k_dev, n)
        worst[dim_x <= n // 2].note(key, n, label, R.frame_error(got, want))
    worst[True].assert_all("weighted rows, padded", n)
    worst[False].assert_all("weighted rows, unpadded", n)


@pytest.mark.parametrize("n", R.FUSED_SIZES)
def test_a_row_is_bounded_relative_to_the_larger_row_of_its_pair(be, filters, n):
    """row b at 1e-3 of row a's scale: the pair-normalised bound holds; b's error relative to b itself is recorded, not bounded"""
    k, k_dev = filters(n)
    for _, label, pair in R.tiny_partner(n, n // 2):
        for how, frame in R.frames_of(pair)[:2]:
            got = filtered(be, frame, k, n)
            want = R.apply(frame, k_dev, n)
            small = 1 if how.startswith("a b") else 0   # where b rides as the partner
            own = np.abs(got[small] - want[small]).max() / np.abs(want[small]).max()
            err = R.frame_error(got[:2], want[:2])
            line = ("tiny partner, N = %5d, rows %s: %.3e of the pair's maximum (bound %.3e); the small row's error relative to itself %.3e"
                    % (n, how, err, R.bound("tiny_partner", n), own))
            report(line)
            assert err <= R.bound("tiny_partner", n), line


@pytest.mark.parametrize("n", [1024, 16384])
def test_a_foreign_k(be, filters, n):
    """a K this ctx did not make (the same values in other memory) is served by another kernel: the same bounds"""
    k, k_dev = filters(n)
    foreign = be.make_projection_device(n // 2 + 1, 1)
    be.copy_h2d(B.Projection(be.filter_to_host(k).reshape(1, -1).copy(), n // 2 + 1, 1), foreign)
    fake = B.FilterBuffer(foreign.ptr, n, be)
    worst = Worst()
    for dim_x in (n // 2, n):
        for key, label, pair in R.pairs(n, dim_x):
            frame = R.frames_of(pair)[0][1]
            got = filtered(be, frame, fake, n)
            worst.note(R.width_key(key, n, dim_x), n, "%s, %d of %d" % (label, dim_x, n), R.frame_error(got, R.apply(frame, k_dev, n)))
    be.free(foreign)
    worst.assert_all("rows, a foreign K", n)


# ---- 4. every instantiation of filter_rows_kernel once -------------------------------------------------------------------------------

# (LOG2N, HALF, WEIGHT, F16OUT) -> the call that reaches it, as launch_flags of filter_fused.hip dispatches: HALF = dim_x <= N / 2, WEIGHT =
# a weighting rides in the load, F16OUT = a half-precision destination. The table restates the dispatch; what makes (WEIGHT = false,
# F16OUT = true) unreachable is read off the callers of paris_hip_fused_filter_launch: paris_hip_apply_filter (filter.hip) is the only one
# that passes weight = false, and it passes d_half = nullptr; paris_hip_weight_filter_rows and paris_hip_weight_filter_batch
# (filter.hip), paris_hip_flush_pending_weight (weight.hip) and the deferred group's launches (backproject.hip: defer_backproject) all
# pass weight = true, and only the first two ever pass a d_half.
GRID = {(log2n, half, weight, f16): ("paris_hip_apply_filter" if not weight else "paris_hip_weight_filter_rows") if weight or not f16 else None
        for log2n in range(10, 15) for half in (True, False) for weight in (False, True) for f16 in (False, True)}


def instantiation(n, dim_x, weight, f16):
    return (n.bit_length() - 1, dim_x <= n // 2, weight, f16)


def test_every_instantiation_once(be, oracle, filters):
    assert len(GRID) == 40 and [key for key, call in GRID.items() if call is None] == [(l, h, False, True) for l in range(10, 15) for h in (True, False)]
    visited, extended = set(), set()
    for n in R.FUSED_SIZES:
        k, k_dev = filters(n)
        for dim_x in (n // 2, n // 2 + 1):
            key, label, pair = list(R.smooth(n, dim_x))[2]   # constant and ramp: the edges are not zero, so EXTEND has something to add
            frame = R.frames_of(pair)[0][1]
            consts = R.weight_constants("ordinary", dim_x)
            bound, weighted_bound = R.bound(key, n), R.bound(R.width_key(key, n, dim_x, "ordinary"), n)
            # no weighting, fp32 in place
            plain = filtered(be, frame, k, n)
            assert R.frame_error(plain, R.apply(frame, k_dev, n)) <= bound, (n, dim_x)
            visited.add(instantiation(n, dim_x, False, False))
            # the weight kernel, then the same launch
            d = load(be, frame)
            be.weight(d, *consts)
            weighted = read(be, d)
            assert np.array_equal(bits(weighted), bits(H.weighted(oracle, frame, "ordinary"))), (n, dim_x)
            be.apply_filter(d, k, n, 3)
            two = read(be, d)
            be.free(d)
            assert R.frame_error(two, R.apply(weighted, k_dev, n)) <= weighted_bound, (n, dim_x)   # (and so `two` is finite)
            # one launch: the same bits
            one = weight_filtered(be, frame, k, n, "ordinary")
            assert np.array_equal(bits(one), bits(two)), (n, dim_x)
            visited.add(instantiation(n, dim_x, True, False))
            # the half store: the fp32 result rounded to half; the fp32 rows and the half buffer's padding stay untouched
            half_pitch = (dim_x * 2 + 6 + 255) // 256 * 256
            sentinel = np.full((3, half_pitch // 4), -3.0, np.float32)
            half = load(be, sentinel)
            d = load(be, frame)
            be.weight_filter_rows(d, 0, 3, *consts, k, n, half.ptr, half.pitch)
            raw = read(be, half).view(np.float16).reshape(3, -1)
            assert np.array_equal(bits(read(be, d)), bits(np.ascontiguousarray(frame, np.float32))), (n, dim_x)
            assert np.array_equal(bits(raw[:, :dim_x]), bits(two.astype(np.float16))), (n, dim_x)
            assert np.array_equal(bits(raw[:, dim_x:]), bits(sentinel.view(np.float16).reshape(3, -1)[:, dim_x:])), (n, dim_x)
            be.free(d)
            be.free(half)
            visited.add(instantiation(n, dim_x, True, True))
            # EXTEND: the rule tests/test_gpu_row_extension.py states, on this launch
            be.set_row_extension(4, 16)
            try:
                got = weight_filtered(be, frame, k, n, "ordinary")
            finally:
                be.clear_row_extension()
            want = RX.extend(weighted, two, 4, B.row_extension_response(4, 16, dim_x, R.TAU))
            assert not np.array_equal(bits(want), bits(two)) and np.array_equal(bits(got), bits(want)), (n, dim_x)
            extended.add(instantiation(n, dim_x, True, False)[:2])
    assert visited == {key for key, call in GRID.items() if call is not None}
    assert extended == {(l, h) for l in range(10, 15) for h in (True, False)}
