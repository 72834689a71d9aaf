"""The zinger rule of include/paris_hip.h restated in numpy, and the seeded frames the zinger tests share.
A helper, not a test."""
import numpy as np

SIGMA = 0.02          # noise of the test frames
SPIKE = 1.0           # planted spikes, either sign
T_ABS = 0.25          # 12 sigma: flags the planted pixels and nothing else
POLARITIES = {"bright": 1, "dark": -1, "both": 0}
NAN_PAYLOAD = 0x7fc54321


def default_max_hits(dim_x, dim_y):
    n = dim_x * dim_y
    return min(n, max(1024, n // 256))


def windows(frame):
    """(9, dim_y, dim_x): the nine window values of every pixel, edges replicated"""
    f = np.ascontiguousarray(frame, np.float32)
    dim_y, dim_x = f.shape
    pad = np.pad(f, 1, mode="edge")
    return np.stack([pad[1 + dy:1 + dy + dim_y, 1 + dx:1 + dx + dim_x] for dy in (-1, 0, 1) for dx in (-1, 0, 1)])


def flagged(frame, t_abs, t_rel, polarity, rows=None):
    """(flags, medians): the pixels the rule flags (those of rows [rows[0], rows[1]) only) and every pixel's median; float32 arithmetic,
    each operation rounded once"""
    f = np.ascontiguousarray(frame, np.float32)
    win = windows(f)
    ok = np.all(np.isfinite(win), axis=0)
    m = np.sort(np.where(ok, win, np.float32(0)), axis=0)[4]
    assert m.dtype == np.float32
    with np.errstate(all="ignore"):
        d = np.where(ok, f, np.float32(0)) - m
        lim = np.float32(t_abs) + np.float32(t_rel) * np.abs(m)
    assert d.dtype == np.float32 and lim.dtype == np.float32
    s = {1: d, -1: -d, 0: np.abs(d)}[POLARITIES.get(polarity, polarity)]
    flags = ok & (s > lim)
    if rows is not None:
        flags[:rows[0]] = False
        flags[rows[1]:] = False
    return flags, m


def run(frame, t_abs, t_rel, polarity, max_hits=0, rows=None):
    """(result, written, saturated): `written` marks the pixels replaced -- none in a frame with more than max_hits flagged pixels,
    which is returned as it was"""
    f = np.ascontiguousarray(frame, np.float32)
    flags, m = flagged(f, t_abs, t_rel, polarity, rows)
    hits = max_hits if max_hits else default_max_hits(f.shape[1], f.shape[0])
    if np.count_nonzero(flags) > hits:
        return f.copy(), np.zeros(f.shape, bool), True
    return np.where(flags, m, f), flags, False


def apply(frame, t_abs, t_rel, polarity, max_hits=0, rows=None):
    """(result, replaced, saturated)"""
    out, written, saturated = run(frame, t_abs, t_rel, polarity, max_hits, rows)
    return out, int(np.count_nonzero(written)), saturated


def smooth(dim_x, dim_y, seed):
    """a ramp from 1.5 to about 2.5 plus Gaussian noise"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[:dim_y, :dim_x]
    return (1.5 + 0.7 * x / max(dim_x - 1, 1) + 0.3 * y / max(dim_y - 1, 1) + rng.normal(0, SIGMA, (dim_y, dim_x))).astype(np.float32)


def planted_frame(dim_x, dim_y=37, seed=1):
    """(frame, planted): spikes of both signs on the four corners, on each edge, as horizontal pairs, 2 x 2 blobs and 3 x 3 blobs
    (the blob on rows 14 .. 16 crosses a strip of 16 rows), 24 single ones, one next to a NaN and one diagonal to an Inf; `planted`
    marks every pixel that holds a spike"""
    assert dim_x >= 90 and dim_y >= 33
    f = smooth(dim_x, dim_y, seed)
    w, h = dim_x - 1, dim_y - 1
    spikes = [(0, 0, 1), (0, w, -1), (h, 0, -1), (h, w, 1),
              (0, 10, 1), (0, 20, -1), (h, 30, 1), (h, 40, -1), (10, 0, 1), (20, 0, -1), (12, w, 1), (22, w, -1),
              (5, 5, 1), (5, 6, 1), (5, 15, -1), (5, 16, -1)]
    spikes += [(8 + j, 25 + i, 1) for j in range(2) for i in range(2)] + [(8 + j, 35 + i, -1) for j in range(2) for i in range(2)]
    spikes += [(14 + j, 45 + i, 1) for j in range(3) for i in range(3)] + [(14 + j, 55 + i, -1) for j in range(3) for i in range(3)]
    spikes += [(25 + 5 * r, 5 + 7 * k, 1 if (k + r) % 2 else -1) for r in range(2) for k in range(12)]
    spikes += [(20, 71, 1), (21, 81, -1)]
    planted = np.zeros(f.shape, bool)
    for y, x, sign in spikes:
        assert not planted[y, x]
        f[y, x] += np.float32(sign * SPIKE)
        planted[y, x] = True
    f.view(np.uint32)[20, 70] = NAN_PAYLOAD
    f[20, 80] = np.inf
    return f, planted


def scattered_frame(dim_x, dim_y, seed, share=0.01):
    """(frame, planted): single spikes of either sign in a share of the pixels"""
    f = smooth(dim_x, dim_y, seed)
    rng = np.random.default_rng(seed + 1000)
    planted = rng.random(f.shape) < share
    f[planted] += (SPIKE * rng.choice([-1.0, 1.0], int(planted.sum()))).astype(np.float32)
    return f, planted


# ---- the quality case: the 64 x 48 driver geometry and head phantom of tests/defect_rule.py over a full circle, seeded dark spikes in
#      0.2 % of the pixels of every view. Depth and threshold chosen on the CPU (oracle pipeline, the rule above; the figures are
#      pinned by tests/test_zinger_host.py and recorded in profiles/r13_zinger_filter.txt) ----------------------------------------------

QUALITY_SHARE = 0.002
QUALITY_DEPTH = 1.0          # about the largest line integral of the phantom (1.114)
QUALITY_T_ABS = 0.25         # "dark", no relative part
CAL_UNFILTERED = 0.10651     # relative RMS against the clean reconstruction, oracle: the spiked frames as they are
CAL_FILTERED = 0.0076349     # the spiked frames through the rule
CAL_CLEAN_FILTERED = 0.0     # the CLEAN frames through the rule: it replaces no pixel of them
BOUND = 1.3                  # the pinned bound: this many times the oracle's figure (as tests/defect_rule.py)


def quality_spiked(lines):
    rng = np.random.default_rng(13)
    out = []
    for p in lines:
        q = p.copy()
        q[rng.random(p.shape) < QUALITY_SHARE] -= np.float32(QUALITY_DEPTH)
        out.append(q)
    return out
