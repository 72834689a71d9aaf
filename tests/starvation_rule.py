"""The starvation filter's tables and rule (include/paris_hip.h) restated in numpy from the header's text, pixel
by pixel and tap by tap in float32, and the wrong readings of that text a kernel or a wrapper could make. A helper, not a test."""
import numpy as np

LEVELS = 64
RADIUS_MAX = 4
F = np.float32


def tables(p0, gain, radius, centre=0.5):
    """(sigma float32[64], g float32[64, radius + 1]), made in float64 and rounded once; centre: where in its bin a level is sampled
    (0.5 is the rule's)"""
    k = np.arange(LEVELS, dtype=np.float64)
    e = (k + centre) / 16.0
    gain64 = float(F(gain))
    sigma = np.minimum(radius / 2.0, gain64 * np.sqrt(np.expm1(e) / (4.0 * np.pi)))
    d = np.arange(radius + 1, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore", under="ignore"):
        g = np.exp(-(d[None, :] ** 2) / (2.0 * sigma[:, None] ** 2))
    g[:, 0] = 1.0
    return sigma.astype(F), g.astype(F)


def level(c, p0):
    with np.errstate(over="ignore"):
        t = F(F(c - p0) * F(16.0))
    return int(t) if t < F(64.0) else 63


def apply(frame, p0, gain, radius, g=None, x_outer=False, keep_non_finite=False, replicate=False, in_place=False):
    """the rule on one frame (dim_y, dim_x): (the new frame, filtered, last_level). The keywords are the WRONG readings: dx as the outer
    loop, non-finite taps kept, edge replication instead of skipped taps, a sweep that reads what it has written."""
    src = np.ascontiguousarray(frame, F)
    out = src.copy()
    if in_place:
        src = out
    p0 = F(p0)
    if g is None:
        g = tables(p0, gain, radius)[1]
    ny, nx = src.shape
    filtered = last = 0
    offsets = [(dy, dx) for dy in range(-radius, radius + 1) for dx in range(-radius, radius + 1)]
    if x_outer:
        offsets = [(dy, dx) for dx in range(-radius, radius + 1) for dy in range(-radius, radius + 1)]
    with np.errstate(all="ignore"):
        for y in range(ny):
            for x in range(nx):
                c = src[y, x]
                if not c > p0:
                    continue
                k = level(c, p0)
                num = den = F(0)
                for dy, dx in offsets:
                    ty, tx = y + dy, x + dx
                    if replicate:
                        ty, tx = min(max(ty, 0), ny - 1), min(max(tx, 0), nx - 1)
                    elif ty < 0 or ty >= ny or tx < 0 or tx >= nx:
                        continue
                    v = src[ty, tx]
                    if not np.isfinite(v) and not keep_non_finite:
                        continue
                    w = F(g[k, abs(dy)] * g[k, abs(dx)])
                    num = F(num + F(w * v))
                    den = F(den + w)
                if den == 0:
                    continue
                out[y, x] = F(num / den)
                filtered += 1
                last += k == 63
    return out, filtered, last


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def same(a, b):
    """bit for bit, except that a NaN the rule COMPUTED may carry any payload"""
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    nan = np.isnan(b)
    return a.shape == b.shape and np.array_equal(np.isnan(a), nan) and np.array_equal(bits(a)[~nan], bits(b)[~nan])


P0 = 3.0
SHAPES = ((1, 1), (5, 3), (61, 7), (64, 16), (65, 17), (130, 33))   # (dim_x, dim_y)
NAN_PAYLOAD = np.uint32(0x7FC0BEEF)


def ulp_steps(v, n):
    v = F(v)
    for _ in range(abs(n)):
        v = np.nextafter(v, F(np.inf if n > 0 else -np.inf), dtype=F)
    return v


def frame(dim_x, dim_y, seed, p0=P0):
    """a frame for the rule's tests: smooth values around p0 with noise, so that about a third of the pixels lie above it at every
    level, then -- where the frame has room -- the special values: level boundaries p0 + k / 16 and their neighbours one ulp to either
    side, +inf centres, NaN (with a payload) and +-inf neighbours, -0, a centre all of whose taps are non-finite, and hits in every
    corner and on every edge"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:dim_y, 0:dim_x]
    a = (p0 - 1.5 + 2.5 * np.sin(0.37 * x + 0.2) * np.cos(0.23 * y) + 1.2 * rng.random((dim_y, dim_x)) ** 3 * 4.0).astype(F)
    free = np.ones((dim_y, dim_x), bool)                   # where the special values may go: not on the rim, not in the block
    free[0], free[-1], free[:, 0], free[:, -1] = False, False, False, False
    if dim_x >= 12 and dim_y >= 12:                        # a +inf centre in a block of non-finite values wider than every radius
        cy, cx = dim_y // 2, dim_x // 2
        a[cy - 4:cy + 5, cx - 4:cx + 5] = np.nan
        a[cy - 4:cy + 5:2, cx - 4:cx + 5:3] = -np.inf
        a[cy, cx] = np.inf
        free[cy - 4:cy + 5, cx - 4:cx + 5] = False
    flat = a.reshape(-1)
    where = np.flatnonzero(free)
    if where.size >= 64 * 3 + 24:
        at = rng.choice(where, 64 * 3 + 24, replace=False)
        for k in range(64):
            b = F(F(p0) + F(k / 16.0))
            flat[at[3 * k]], flat[at[3 * k + 1]], flat[at[3 * k + 2]] = b, ulp_steps(b, -1), ulp_steps(b, 1)
        flat[at[192]] = F(p0 + 4.0)                       # the first value of the overflow: t = 64
        flat[at[193]] = ulp_steps(F(p0 + 4.0), -1)
        flat[at[194]] = F(p0 + 40.0)
        flat[at[195:199]] = np.inf
        flat[at[199:203]] = -np.inf
        flat[at[203:207]] = np.nan
        flat.view(np.uint32)[at[207:210]] = NAN_PAYLOAD
        flat[at[210:213]] = -0.0
        flat[at[213]] = F(3.0e38)                         # num overflows beside its like
        flat[at[214]] = F(3.0e38)
    hot = F(p0 + 1.7)
    for yy in (0, dim_y - 1):
        for xx in (0, dim_x - 1):
            a[yy, xx] = hot
    a[0, dim_x // 2], a[dim_y - 1, dim_x // 3], a[dim_y // 2, 0], a[dim_y // 3, dim_x - 1] = hot, F(p0 + 0.3), F(p0 + 2.9), F(p0 + 5.0)
    return a


def below(dim_x, dim_y, seed, p0=P0):
    """everything at or below p0 (p0 itself included), with NaN payloads, -0 and -inf: the rule writes nothing"""
    rng = np.random.default_rng(seed)
    a = (p0 - 3.0 * rng.random((dim_y, dim_x))).astype(F)
    flat = a.reshape(-1)
    n = flat.size
    flat[rng.integers(0, n, max(1, n // 7))] = F(p0)
    flat[rng.integers(0, n, max(1, n // 9))] = -0.0
    flat[rng.integers(0, n, max(1, n // 11))] = -np.inf
    flat.view(np.uint32)[rng.integers(0, n, max(1, n // 8))] = NAN_PAYLOAD
    assert not (a > F(p0)).any()
    return a
