"""The ring rule of include/paris_hip.h restated in numpy: float64 sequential sums, float32 elsewhere, each
operation rounded once -- and the seeded frames the ring tests share. A helper, not a test."""
import numpy as np

NAN_PAYLOAD = 0x7fc54321
FRAMES_MAX = 64  # PARIS_HIP_RING_FRAMES_MAX: what one accumulate launch serves


def sums(frames, start=None):
    """S: the float64 sum of the float32 frames, added to zeros (or to `start`) one after the other in the order given"""
    s = np.zeros(np.shape(frames[0]), np.float64) if start is None else np.array(start, np.float64)
    with np.errstate(all="ignore"):
        for f in frames:
            assert np.asarray(f).dtype == np.float32
            s = s + np.asarray(f).astype(np.float64)
    return s


def mean_of(s, counts):
    """mean[y][x] = (float)(S[y][x] / (double)N[y]); rows without a frame hold 0"""
    s = np.asarray(s, np.float64)
    n = np.broadcast_to(np.asarray(counts, np.uint32), (s.shape[0],)).astype(np.float64)[:, None]
    with np.errstate(all="ignore"):
        return np.where(n != 0, s / np.where(n != 0, n, 1.0), 0.0).astype(np.float32)


def correction(mean, half_width, floor_abs=0.0, limit_abs=0.0, counts=None):
    """(c, stats): the rule on a mean frame; stats as paris_hip_ring_stats, a dict"""
    m = np.ascontiguousarray(mean, np.float32)
    dim_y, dim_x = m.shape
    h = int(half_width)
    pad = np.pad(m, ((0, 0), (h, h)), mode="edge")
    win = np.stack([pad[:, d:d + dim_x] for d in range(2 * h + 1)])
    ok = np.all(np.isfinite(win), axis=0)
    present = np.ones(dim_y, bool) if counts is None else np.asarray(counts) != 0
    ok_here = ok & present[:, None]
    med = np.sort(np.where(ok, win, np.float32(0)), axis=0)[h]
    with np.errstate(all="ignore"):
        diff = np.where(ok, m, np.float32(0)) - med
    assert diff.dtype == np.float32
    a = np.abs(diff)
    below = ok_here & (a < np.float32(floor_abs))
    above = ok_here & ~below & (np.float32(limit_abs) != 0) & (a > np.float32(limit_abs))
    kept = ok_here & ~below & ~above & (diff != 0)
    c = np.where(kept, diff, np.float32(0)).astype(np.float32)
    stats = dict(corrected=int(kept.sum()), below_floor=int(below.sum()), above_limit=int(above.sum()),
                 not_finite=int((~ok & present[:, None]).sum()), max_abs=float(a[kept].max()) if kept.any() else 0.0,
                 frames_min=0 if counts is None else int(np.min(counts)), frames_max=0 if counts is None else int(np.max(counts)))
    return c, stats


def stats_of(st):
    """a RingStats as the dict correction() returns"""
    return dict(corrected=int(st.corrected), below_floor=int(st.below_floor), above_limit=int(st.above_limit),
                not_finite=int(st.not_finite), max_abs=float(st.max_abs), frames_min=int(st.frames_min), frames_max=int(st.frames_max))


def subtract(frame, c):
    """p - c where c != 0, in float32; every other pixel keeps its bits"""
    f = np.ascontiguousarray(frame, np.float32)
    with np.errstate(all="ignore"):
        return np.where(c != 0, f - c, f).astype(np.float32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


def same_means(a, b):
    """bit for bit, except that a NaN equals any NaN: which payload a sum that met a NaN carries is not part of the rule"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(a.view(np.uint32)[~nan], b.view(np.uint32)[~nan])


# ---- the seeded frames of the GPU tests ------------------------------------------------------------------------------------------

SIGMA = 0.02
OFFSET = 0.08          # planted stationary offsets, either sign: 4 sigma of one frame, 4 sqrt(n) sigma of the mean of n
H, FLOOR, LIMIT = 2, 0.04, 0.25


def offsets(dim_x, dim_y, seed=3, share=0.04):
    """a stationary offset in a share of the pixels, and one whole column"""
    rng = np.random.default_rng(seed + 500)
    hit = rng.random((dim_y, dim_x)) < share
    off = np.zeros((dim_y, dim_x), np.float32)
    off[hit] = (OFFSET * rng.choice([-1.0, 1.0], int(hit.sum()))).astype(np.float32)
    off[:, dim_x // 3] = np.float32(OFFSET)
    return off


def scan(dim_x, dim_y, n, seed=3, off=None):
    """n frames: a ramp from 1.5 to about 2.5 plus Gaussian noise, new in every frame, plus the stationary offsets"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[:dim_y, :dim_x]
    base = 1.5 + 0.7 * x / max(dim_x - 1, 1) + 0.3 * y / max(dim_y - 1, 1)
    off = offsets(dim_x, dim_y, seed) if off is None else off
    return [(base + rng.normal(0, SIGMA, (dim_y, dim_x))).astype(np.float32) + off for _ in range(n)]


def awkward_scan(dim_x, dim_y, n, seed=5):
    """the same with a NaN payload, an Inf, a -0 column and denormals in fixed places of some frames"""
    frames = scan(dim_x, dim_y, n, seed)
    frames[0].view(np.uint32)[1, 2] = NAN_PAYLOAD
    frames[n - 1][2, dim_x - 1] = np.inf
    for f in frames:
        f[3, :] = np.float32(-0.0)
        f[4, 0] = np.float32(1e-41)
    frames[0][4, 1] = np.float32(-3e-45)
    frames[0][5, 0] = np.float32(3e38)
    if n > 1:
        frames[1][5, 0] = np.float32(3e38)
    return frames


# ---- the quality case: a 192 x 12 detector, otherwise the driver geometry and head phantom of tests/defect_rule.py over a full
#      circle (l_px_row = 0.2 / 3 keeps the fan), with stationary offsets of +-0.04 .. 0.10 in 3 % of the pixels, one whole column and
#      one pair of columns. Setting and figures chosen on the CPU (oracle pipeline, the rule above; the figures are pinned by
#      tests/test_ring_host.py and recorded in profiles/r15_ring_correction.txt) --------------------------------------------------------

QUALITY_GEO = (192, 12, 0.2 / 3, 0.25, 1.5, -0.75, 100, 200, 1.0)
QUALITY_SEED = 15
QUALITY_SHARE = 0.03
QUALITY_H, QUALITY_FLOOR, QUALITY_LIMIT = 2, 0.035, 0.25
CAL_UNCORRECTED = 0.085533   # relative RMS against the clean reconstruction, oracle: the frames with the offsets as they are
CAL_CORRECTED = 0.021931     # the same frames through the rule
CAL_CLEAN_CORRECTED = 0.0    # the CLEAN frames through the rule: it corrects no pixel of them
BOUND = 1.3                  # the pinned bound: this many times the oracle's figure (tests/defect_rule.py)


def quality_offsets():
    n_row, n_col = QUALITY_GEO[:2]
    rng = np.random.default_rng(QUALITY_SEED)
    hit = rng.random((n_col, n_row)) < QUALITY_SHARE
    off = np.zeros((n_col, n_row), np.float32)
    off[hit] = (rng.uniform(0.04, 0.10, int(hit.sum())) * rng.choice([-1.0, 1.0], int(hit.sum()))).astype(np.float32)
    off[:, 70] = np.float32(0.06)        # a miscalibrated column
    off[:, 120:122] = np.float32(-0.05)  # and a pair
    return off


def quality_frames(vol_dim_x, l_vx_x):
    """the clean line integrals of the 360 views, float32 (n_col, n_row) each"""
    import phantom
    n_row, n_col, lr, lc, ds, dt, d_so, d_od, step = QUALITY_GEO
    radius = 0.9 * vol_dim_x * l_vx_x / 2
    return [phantom.projection(n_row, n_col, lr, lc, d_so, d_od, float(np.float32(i) * np.float32(step)), radius, ds, dt)
            for i in range(int(360 / step))]


def through_the_rule(frames, h=QUALITY_H, floor_abs=QUALITY_FLOOR, limit_abs=QUALITY_LIMIT):
    """(corrected frames, c, stats)"""
    n = len(frames)
    c, st = correction(mean_of(sums(frames), n), h, floor_abs, limit_abs, np.full(frames[0].shape[0], n, np.uint32))
    return [subtract(f, c) for f in frames], c, st
