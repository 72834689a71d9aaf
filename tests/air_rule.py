"""The air-region rule (include/paris_hip.h) restated in numpy, for the tests: the 256 partial sums, each a
sequential float64 sum, their ordered combination, the division, the two refusals per frame and the subtraction -- and small scans
whose frames drift. Nothing here calls the library."""
import numpy as np

LANES = 256
WAVE_COLUMNS = 64
ROW_STEP = LANES // WAVE_COLUMNS
FRAMES_MAX = 64          # PARIS_HIP_AIR_FRAMES_MAX
PIXELS_MAX = 1 << 20
NAN_PAYLOAD = 0x7FC12345

# (x0, y0, width, height) in a 140 x 20 frame: 1 x 1, 3 x 2, 63 x 3, 64 x 4, 65 x 5, 130 x 9 and the whole frame; x0 unaligned where
# the rectangle leaves room
DIM_X, DIM_Y = 140, 20
RECTANGLES = [(7, 3, 1, 1), (5, 11, 3, 2), (13, 2, 63, 3), (3, 7, 64, 4), (1, 13, 65, 5), (9, 10, 130, 9), (0, 0, DIM_X, DIM_Y)]


def default_min_pixels(width, height):
    return (width * height + 1) // 2


def sequential_sum(values):
    """+0.0, then every value added in order, in float64 (np.cumsum adds one after the other; np.sum adds pairwise)"""
    return np.cumsum(np.concatenate([[0.0], np.asarray(values, np.float64)]))[-1]


def counting(frame, rect, mask=None):
    """the rectangle's pixels and which of them count: mask byte 0 and a finite value"""
    x0, y0, w, h = rect
    px = np.asarray(frame, np.float32)[y0:y0 + h, x0:x0 + w]
    ok = np.isfinite(px)
    if mask is not None:
        ok &= np.asarray(mask)[y0:y0 + h, x0:x0 + w] == 0
    return px, ok


def partial_sums(frame, rect, mask=None):
    """(acc[256] float64, n[256]): lane l owns columns l % 64, + 64, ... of rows l // 64, + 4, ... of the rectangle, row after row"""
    px, ok = counting(frame, rect, mask)
    acc, n = np.zeros(LANES, np.float64), np.zeros(LANES, np.int64)
    for lane in range(LANES):
        c, r = lane % WAVE_COLUMNS, lane // WAVE_COLUMNS
        mine, keep = px[r::ROW_STEP, c::WAVE_COLUMNS].ravel(), ok[r::ROW_STEP, c::WAVE_COLUMNS].ravel()
        acc[lane] = sequential_sum(mine[keep])
        n[lane] = np.count_nonzero(keep)
    return acc, n


def value(frame, rect, mask=None, min_pixels=0, limit_abs=0.0):
    """(a_f as np.float32, n, why) -- why is "normalised", "too_few" or "above_limit" """
    acc, n = partial_sums(frame, rect, mask)
    total, pixels = np.cumsum(acc)[-1], int(n.sum())
    least = min_pixels if min_pixels else default_min_pixels(rect[2], rect[3])
    if pixels < least:
        return np.float32(0), pixels, "too_few"
    a = np.float32(total / np.float64(pixels))
    if limit_abs != 0 and abs(a) > np.float32(limit_abs):
        return np.float32(0), pixels, "above_limit"
    return a, pixels, "normalised"


def values(frames, rect, mask=None, min_pixels=0, limit_abs=0.0):
    got = [value(f, rect, mask, min_pixels, limit_abs) for f in frames]
    return np.array([g[0] for g in got], np.float32), np.array([g[1] for g in got], np.uint32), [g[2] for g in got]


def subtract(frame, a, rows=None):
    """p - a_f over the band's rows, one fp32 subtraction; a frame whose a_f is zero of either sign keeps every bit"""
    out = np.array(frame, np.float32, copy=True)
    if a == 0:
        return out
    first, count = (0, out.shape[0]) if rows is None else rows
    with np.errstate(invalid="ignore", over="ignore"):
        out[first:first + count] = out[first:first + count] - np.float32(a)
    return out


def normalised(frames, rect, mask=None, min_pixels=0, limit_abs=0.0, rows=None):
    a = values(frames, rect, mask, min_pixels, limit_abs)[0]
    return [subtract(f, v, rows) for f, v in zip(frames, a)]


def counts_of(whys, a):
    """what paris_hip_air_stats reports for these frames"""
    kept = [v for v, w in zip(a, whys) if w == "normalised"]
    return {"frames": len(whys), "normalised": len(kept), "too_few": whys.count("too_few"), "above_limit": whys.count("above_limit"),
            "min_a": np.float32(min(kept)) if kept else np.float32(np.inf), "max_a": np.float32(max(kept)) if kept else np.float32(-np.inf)}


def stats_of(st):
    return {"frames": st.frames, "normalised": st.normalised, "too_few": st.too_few, "above_limit": st.above_limit,
            "min_a": np.float32(st.min_a), "max_a": np.float32(st.max_a)}


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.int32), np.ascontiguousarray(b, np.float32).view(np.int32))


def scan(dim_x, dim_y, n, seed=1, drift=0.05):
    """n frames of line integrals: an object in the middle, noise, and per frame the constant -ln(1 + e_f), e_f uniform in +-drift"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:dim_y, 0:dim_x]
    r2 = ((x + 0.5 - dim_x / 2.0) / (0.3 * dim_x)) ** 2 + ((y + 0.5 - dim_y / 2.0) / (0.35 * dim_y)) ** 2
    body = 1.5 * np.clip(1.0 - r2, 0.0, None)        # an ellipse that leaves the corners in air
    eps = rng.uniform(-drift, drift, n)
    return [(body + rng.normal(0, 0.01, (dim_y, dim_x)) - np.log1p(e)).astype(np.float32) for e in eps]


def decades_scan(dim_x, dim_y, n, seed=2):
    """values spread over 12 decades, of either sign: the order of the additions shows in the sum's last bits"""
    rng = np.random.default_rng(seed)
    return list((rng.normal(0, 1, (n, dim_y, dim_x)) * 10.0 ** rng.integers(-6, 7, (n, dim_y, dim_x))).astype(np.float32))


def cancelling_scan(dim_x, dim_y, n, rect, seed=8):
    """decades_scan() whose rectangle holds every value twice, once with either sign, at shuffled places (an odd pixel holds 0): the
    exact sum is 0, so the float64 sum is nothing but the roundings of its additions, and their order decides every bit of the value"""
    x0, y0, w, h = rect
    rng = np.random.default_rng(seed)
    frames = decades_scan(dim_x, dim_y, n, seed + 1)
    for f in frames:
        half = f[y0:y0 + h, x0:x0 + w].ravel()[:w * h // 2]
        inside = np.concatenate([half, -half, np.zeros(w * h % 2, np.float32)])
        f[y0:y0 + h, x0:x0 + w] = rng.permutation(inside).reshape(h, w)
    return frames


def awkward(frame, rect, seed=3):
    """the frame with a NaN (with a payload), +inf and -inf inside the rectangle where it has room, and a NaN outside it"""
    x0, y0, w, h = rect
    out = np.array(frame, np.float32, copy=True)
    rng = np.random.default_rng(seed)
    spots = [(y0 + int(rng.integers(h)), x0 + int(rng.integers(w))) for _ in range(3)]
    for (y, x), bad in zip(spots[:min(3, max(1, w * h - 1))], (np.nan, np.inf, -np.inf)):
        out[y, x] = bad
    y, x = spots[0]
    if np.isnan(out[y, x]):
        out.view(np.uint32)[y, x] = NAN_PAYLOAD
    return out


def random_mask(dim_x, dim_y, fraction=0.2, seed=4):
    return (np.random.default_rng(seed).random((dim_y, dim_x)) < fraction).astype(np.uint8)


# ---- the driver's scan: 64 x 48, 72 views of the head phantom as u16 counts against one flat, clean and drifting -----------------------

DRIVER_GEO = (64, 48, 0.2, 0.25, 0.0, 0.0, 100, 200, 5.0)
DRIVER_VIEWS = 72
DRIVER_RECT = (1, 1, 7, 5)       # a corner the phantom never reaches (driver_scan checks it)
DRIVER_DRIFT = 0.05


def driver_scan(radius_mm, seed=31):
    """(dark, flat, clean counts, drifting counts, eps, exact line integrals): every frame's counts are dark + (flat - dark) exp(-p),
    the drifting ones with exp(-p) times 1 + eps_f, eps_f uniform in +-DRIVER_DRIFT, both rounded to u16. The attenuation is scaled to
    at most 2.5 (8 % transmission), as the flat-field quality test does; the flat stays below 65535 / 1.05."""
    import phantom
    n_row, n_col, lr, lc, _, _, d_so, d_od, step = DRIVER_GEO
    rng = np.random.default_rng(seed)
    lines = [phantom.projection(n_row, n_col, lr, lc, d_so, d_od, float(np.float32(i) * np.float32(step)), radius_mm) for i in range(DRIVER_VIEWS)]
    mu = 2.5 / max(float(p.max()) for p in lines)
    lines = [(mu * p).astype(np.float32) for p in lines]
    x0, y0, w, h = DRIVER_RECT
    assert all(not p[y0:y0 + h, x0:x0 + w].any() for p in lines), "the phantom reaches the air region"
    dark = np.rint(100 + 200 * rng.random((n_col, n_row))).astype(np.float32)        # whole counts: one u16 frame each is their mean
    flat = np.rint(dark + 60000 * (0.85 + 0.15 * rng.random((n_col, n_row)))).astype(np.float32)
    eps = rng.uniform(-DRIVER_DRIFT, DRIVER_DRIFT, DRIVER_VIEWS)
    eps[:2] = (-DRIVER_DRIFT, DRIVER_DRIFT)

    def counts(p, e):
        return np.clip(np.rint(dark + (flat - dark) * np.exp(-p.astype(np.float64)) * (1.0 + e)), 0, 65535).astype(np.uint16)

    clean = np.stack([counts(p, 0.0) for p in lines])
    drifting = np.stack([counts(p, e) for p, e in zip(lines, eps)])
    assert drifting.max() < 65535
    return dark, flat, clean, drifting, eps, lines


def line_integrals(counts, dark, flat, t_min=1e-5):
    """the dark / flat correction in float64, rounded once: what the device's correction gives to within an ulp"""
    t = (counts.astype(np.float64) - dark) / (flat.astype(np.float64) - dark)
    return (-np.log(np.maximum(t, t_min))).astype(np.float32)
