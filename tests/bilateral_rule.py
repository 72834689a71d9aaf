"""The 3-D bilateral filter of include/paris_hip.h restated in numpy, one np.float32 operation per operation of the rule, the taps in
the rule's order (dz, then dy, then dx, ascending from -r). Whole-volume arrays stand for the per-voxel scalars: every element sees
the same sequence of roundings as one voxel of the C++ rule. The keyword arguments switch on ONE misreading each, for the tests that
show the parity tests discriminate; float64_model is the independent model with the exact Gaussian."""
import math

import numpy as np

BINS = 1024


def tables(sigma_r, sigma_s, r):
    """(spatial [dz, dy, dx], range, rscale): made in double with math.exp, rounded once to float32"""
    side = 2 * r + 1
    spatial = np.empty((side, side, side), np.float32)
    two_s2 = 2.0 * float(np.float32(sigma_s)) * float(np.float32(sigma_s))
    for dz in range(-r, r + 1):
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                spatial[dz + r, dy + r, dx + r] = np.float32(math.exp(-float(dx * dx + dy * dy + dz * dz) / two_s2))
    rng = np.array([math.exp(-0.5 * ((i + 0.5) * 4.0 / BINS) ** 2) for i in range(BINS)], np.float64).astype(np.float32)
    rscale = np.float32(BINS / (4.0 * float(np.float32(sigma_r))))
    return spatial, rng, rscale


def bilateral(v, sigma_r, sigma_s, r, z_first=0, z_count=None, centre=True, border="skip", order="zyx", contract=False,
              cutoff_weight=False):
    """slices [z_first, z_first + z_count) of v (dim_z, dim_y, dim_x) filtered; taps outside v are skipped"""
    v = np.ascontiguousarray(v, np.float32)
    nz, ny, nx = v.shape
    z_count = nz - z_first if z_count is None else z_count
    spatial, rng, rscale = tables(sigma_r, sigma_s, r)
    if border == "skip":
        pad = np.pad(v, r, mode="constant", constant_values=np.float32(np.nan))  # NaN fails `t < 1024` exactly as a skipped tap does ...
        inside = np.pad(np.ones(v.shape, bool), r, mode="constant", constant_values=False)  # ... but a stored NaN is told apart here
    else:
        pad = np.pad(v, r, mode="edge")
        inside = np.ones(pad.shape, bool)
    zs = slice(z_first, z_first + z_count)
    vc = v[zs]
    num = np.zeros(vc.shape, np.float32)
    den = np.zeros(vc.shape, np.float32)
    span = range(-r, r + 1)
    if order == "zyx":
        taps = [(dz, dy, dx) for dz in span for dy in span for dx in span]
    else:  # the misreading: dx outermost
        taps = [(dz, dy, dx) for dx in span for dy in span for dz in span]
    limit = np.float32(BINS)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore", under="ignore"):
        for dz, dy, dx in taps:
            if not centre and (dz, dy, dx) == (0, 0, 0):
                continue
            window = (slice(z_first + r + dz, z_first + r + dz + z_count), slice(r + dy, r + dy + ny), slice(r + dx, r + dx + nx))
            vn = pad[window]
            d = np.abs(vn - vc)
            t = d * rscale
            take = (t < limit) & inside[window]
            index = np.where(take, t, np.float32(0)).astype(np.uint32)
            w = spatial[dz + r, dy + r, dx + r] * rng[index]
            if cutoff_weight:  # the misreading: a tap at or beyond the cutoff gets the last bin's weight
                beyond = (t >= limit) & inside[window]
                w = np.where(beyond, spatial[dz + r, dy + r, dx + r] * rng[BINS - 1], w)
                take = take | beyond
            if contract:  # the misreading: w * v_n contracted into the add (the product of two floats is exact in double)
                s = (w.astype(np.float64) * vn.astype(np.float64) + num.astype(np.float64)).astype(np.float32)
            else:
                p = w * vn
                s = num + p
            num = np.where(take, s, num)
            den = np.where(take, den + w, den)
        out = num / den
    return np.where(np.isfinite(vc), out, vc)


def float64_model(v, sigma_r, sigma_s, r, with_bound=False):
    """The bilateral filter in float64 with the exact Gaussian exp(-d^2 / (2 sigma_r^2)) at every tap and no cutoff; taps outside v
    are skipped; for finite volumes. with_bound: also, per voxel, how far the library's rule may lie from this model because of its
    table: with dw_n the difference of a tap's weight, out_rule - out_model = sum dw_n (v_n - out_model) / den_rule and
    den_rule >= den_model - sum |dw_n|, where |dw_n| <= s_n (2 / 1024) e^-1/2 inside the cutoff (bin width times the Gaussian's
    steepest slope, in units of sigma_r) and dw_n is the model's own weight, at most s_n e^-8, beyond it."""
    v = np.asarray(v, np.float64)
    nz, ny, nx = v.shape
    pad = np.pad(v, r, mode="constant", constant_values=np.nan)
    num, den = np.zeros(v.shape), np.zeros(v.shape)
    span = range(-r, r + 1)
    windows = [((dz, dy, dx), (slice(r + dz, r + dz + nz), slice(r + dy, r + dy + ny), slice(r + dx, r + dx + nx)))
               for dz in span for dy in span for dx in span]

    def weight(tap, vn):
        dz, dy, dx = tap
        s = math.exp(-(dx * dx + dy * dy + dz * dz) / (2.0 * sigma_s * sigma_s))
        return s, s * np.exp(-0.5 * ((vn - v) / sigma_r) ** 2)

    for tap, window in windows:
        vn = pad[window]
        ok = ~np.isnan(vn)
        _, w = weight(tap, np.where(ok, vn, v))
        num += np.where(ok, w * np.where(ok, vn, 0.0), 0.0)
        den += np.where(ok, w, 0.0)
    out = num / den
    if not with_bound:
        return out
    slope = (2.0 / BINS) * math.exp(-0.5)
    moved, mass = np.zeros(v.shape), np.zeros(v.shape)
    for tap, window in windows:
        vn = pad[window]
        ok = ~np.isnan(vn)
        vn = np.where(ok, vn, v)
        s, w = weight(tap, vn)
        dw = np.where(np.abs(vn - v) < 4.0 * sigma_r, s * slope, w)
        dw = np.where(ok, dw, 0.0)
        moved += dw * np.abs(vn - out)
        mass += dw
    return out, moved / (den - mass)
