"""The row-extension rule of include/paris_hip.h restated in numpy, and the truncated quality set the tests
share. No library call in here: this is what the host functions and the device are compared against."""
import numpy as np

import defect_rule

EDGE_PIXELS = (1, 2, 4, 8)
TAPER_MAX = 16384


def taper(w):
    """t(k) = cos^2(pi k / (2 (W + 1))), k = 1 .. W, float64"""
    k = np.arange(1, w + 1, dtype=np.float64)
    return np.cos(np.pi * k / (2.0 * (w + 1.0))) ** 2


def response64(n, tau, w):
    """c[s] = sum_k t(k) g[s + k], g[d] = -1 / (2 pi^2 d^2 tau) for odd d, 0 for even d; float64, summed in ascending k"""
    t = taper(w)
    d = np.arange(n, dtype=np.float64)[:, None] + np.arange(1, w + 1, dtype=np.float64)[None, :]
    g = np.where(d.astype(np.int64) % 2 == 1, -1.0 / (2.0 * np.pi ** 2 * d * d * float(np.float32(tau))), 0.0)
    terms = t[None, :] * g
    c = np.zeros(n, np.float64)
    for k in range(w):   # ascending k, one rounding per addition (np.sum adds pairwise)
        c += terms[:, k]
    return c


def response(n, tau, w):
    """the response rounded once to fp32"""
    return response64(n, tau, w).astype(np.float32)


def edge_means(rows, m):
    """rows: (..., n) float32 as the transform sees them -> (a, b): the means of the first / last m pixels, a sequential fp32 sum in
    ascending index followed by the exact scaling by 1 / m"""
    q = np.asarray(rows, np.float32)
    assert q.shape[-1] >= m and m in EDGE_PIXELS
    a, b = q[..., 0].copy(), q[..., q.shape[-1] - m].copy()
    for e in range(1, m):
        a = (a + q[..., e]).astype(np.float32)
        b = (b + q[..., q.shape[-1] - m + e]).astype(np.float32)
    inv = np.float32(1.0) / np.float32(m)
    return (a * inv).astype(np.float32), (b * inv).astype(np.float32)


def fma32(x, y, z):
    """fmaf(x, y, z) of fp32 arrays, exactly: the product of two fp32 numbers is exact in float64; the float64 sum is turned into the
    round-to-odd sum with the error term of a two-sum, and a round-to-odd float64 rounds to fp32 as the exact value does (53 bits
    hold more than 24 + 2). Finite values away from the fp32 range limits only."""
    x, y, z = np.broadcast_arrays(np.asarray(x, np.float32), np.asarray(y, np.float32), np.asarray(z, np.float32))
    p = x.astype(np.float64) * y.astype(np.float64)
    c = z.astype(np.float64)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)   # exact: s + err == p + c
    inexact = err != 0.0
    # truncate towards zero where the rounded sum overshot, then set the sticky bit
    over = inexact & (np.sign(err) != np.sign(s))
    s = np.where(over, np.nextafter(s, 0.0), s)
    bits = s.copy().view(np.int64)
    bits = np.where(inexact, bits | 1, bits)
    return bits.view(np.float64).astype(np.float32)


def update(plain, a, b, c):
    """plain: (rows, n) fp32, what the plain filter stores; a, b: (rows,) edge means; c: (n,) response -> the stored pixels
    fmaf(b, c[n - 1 - s], fmaf(a, c[s], y))"""
    c = np.asarray(c, np.float32)
    inner = fma32(np.asarray(a, np.float32)[:, None], c[None, :], plain)
    return fma32(np.asarray(b, np.float32)[:, None], c[::-1][None, :], inner)


def extend(weighted, plain, m, c):
    """the rule's update of `plain` (the filtered rows) with the edge means of `weighted` (the rows the transform saw)"""
    a, b = edge_means(weighted, m)
    return update(plain, a, b, c)


# ---- the truncated quality case: the 64 x 48 driver geometry of defect_rule.QUALITY_GEO, a head phantom 1.6 x as wide as the grid
#      (so every row is truncated on both sides) over a full circle; the truth is an FDK reconstruction from a detector three times
#      as wide, backprojected into the same grid --------------------------------------------------------------------------------

QUALITY_GEO = defect_rule.QUALITY_GEO
BOUND = defect_rule.BOUND
TRUNCATED_RADIUS = 1.6     # phantom radius over the grid's half width
UNTRUNCATED_RADIUS = 0.9
WIDE = 3                   # the truth's detector is this many times as wide
QUALITY_TAPER = 16
CAL_ZERO_PADDED = 0.4737   # relative RMS against the truth, oracle, zero padding
CAL_EXTENDED_1 = 0.07114   # taper_pixels = 16, edge_pixels = 1
CAL_EXTENDED_4 = 0.06415   # taper_pixels = 16, edge_pixels = 4


def wide_geo():
    g = list(QUALITY_GEO)
    g[0] *= WIDE
    return tuple(g)


def quality_frames(vol_dim_x, l_vx_x, radius, wide=False):
    """the line integrals of the 360 views, float32 (n_col, n_row) each; wide: on the detector WIDE times as wide"""
    import phantom
    n_row, n_col, lr, lc, ds, dt, d_so, d_od, step = wide_geo() if wide else QUALITY_GEO
    r_mm = radius * vol_dim_x * l_vx_x / 2
    return [phantom.projection(n_row, n_col, lr, lc, d_so, d_od, float(np.float32(i) * np.float32(step)), r_mm, ds, dt)
            for i in range(int(360 / step))]


def quality_region(vol_shape, l_vx_x):
    """boolean (dim_z, dim_y, dim_x): inside 0.85 of the field-of-view radius, on the central half of the slices"""
    dim_z, dim_y, dim_x = vol_shape
    x = (np.arange(dim_x) + 0.5 - dim_x / 2) * l_vx_x
    y = (np.arange(dim_y) + 0.5 - dim_y / 2) * l_vx_x
    disc = (x[None, :] ** 2 + y[:, None] ** 2) <= (0.85 * dim_x * l_vx_x / 2) ** 2
    z = np.zeros(dim_z, bool)
    z[dim_z // 4: dim_z - dim_z // 4] = True
    return z[:, None, None] & disc[None, :, :]


def relative_rms(got, truth, region):
    g, t = np.asarray(got, np.float64)[region], np.asarray(truth, np.float64)[region]
    return float(np.sqrt(((g - t) ** 2).mean()) / np.sqrt((t ** 2).mean()))


def oracle_reconstruct(oracle, det, vol_geo, frames, setting=None, bp_det=None):
    """weight, filter, the rule's update (setting = (taper_pixels, edge_pixels) or None) and backprojection as oracle.reconstruct
    runs them; the volume has vol_geo's grid whatever the detector"""
    vol = np.zeros((vol_geo.dim_z, vol_geo.dim_y, vol_geo.dim_x), np.float32)
    fs = oracle.filter_size(det.n_row)
    k = oracle.make_filter(fs, det.l_px_row)
    c = response(det.n_row, det.l_px_row, setting[0]) if setting is not None else None
    for i, frame in enumerate(frames):
        p = frame.copy()
        oracle.weight(p, det)
        if setting is not None:
            weighted = p.copy()
        oracle.apply_filter(p, k, fs)
        if setting is not None:
            p = np.ascontiguousarray(extend(weighted, p, setting[1], c))
        s, cs, ds, dt = oracle.backproject_constants(det, i)
        oracle.backproject(vol, p, 0, det, vol_geo, s, cs, ds, dt)
    return vol
