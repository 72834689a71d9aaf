"""The volume-export rule of include/paris_hip.h in numpy, a reader for the .mhd / .raw pair paris.hip
writes, and the seeded volumes the tests share. A helper, not a test."""
import os

import numpy as np

LEVELS = {np.dtype(np.uint8): 255, np.dtype(np.uint16): 65535}
MET_TYPES = {"MET_UCHAR": np.uint8, "MET_USHORT": np.uint16}
BINS_MAX = 4096


def f32(x):
    return np.float32(x)


def scale(lo, hi, levels):
    """(float)(levels / ((double)hi - (double)lo)), rounded once"""
    return np.float32(levels / (float(f32(hi)) - float(f32(lo))))


def quantize(v, lo, hi, dtype):
    """x = (v - lo) * scale in float32, each operation rounded once; 0 for NaN or x <= 0, L for x >= L, else rint(x)"""
    dtype = np.dtype(dtype)
    levels = LEVELS[dtype]
    v = np.asarray(v, np.float32)
    s = scale(lo, hi, levels)
    with np.errstate(all="ignore"):
        x = (v - f32(lo)) * s
        assert x.dtype == np.float32
        q = np.rint(x)
    q = np.where(x >= f32(levels), f32(levels), q)
    q = np.where(x > 0, q, f32(0))  # x <= 0 and NaN
    return q.astype(dtype)


def counts(v, lo, hi):
    """(voxels, below, above, not_finite)"""
    v = np.asarray(v, np.float32).ravel()
    finite = np.isfinite(v)
    with np.errstate(invalid="ignore"):
        return v.size, int((finite & (v < f32(lo))).sum()), int((finite & (v > f32(hi))).sum()), int((~finite).sum())


def extremes(v):
    """(min, max) of the finite voxels; (+inf, -inf) without one"""
    v = np.asarray(v, np.float32).ravel()
    v = v[np.isfinite(v)]
    return (f32(np.inf), f32(-np.inf)) if v.size == 0 else (v.min(), v.max())


def histogram(v, h_lo, h_hi, n_bins):
    """(hist uint64[n_bins], below, above, not_finite)"""
    v = np.asarray(v, np.float32).ravel()
    _, below, above, not_finite = counts(v, h_lo, h_hi)
    bscale = scale(h_lo, h_hi, n_bins)
    with np.errstate(invalid="ignore"):
        inside = v[np.isfinite(v) & (v >= f32(h_lo)) & (v <= f32(h_hi))]
    with np.errstate(over="ignore"):
        x = (inside - f32(h_lo)) * bscale
    assert x.dtype == np.float32
    b = np.minimum(np.floor(x.astype(np.float64)), n_bins - 1).astype(np.int64)  # the conversion truncates; x >= 0
    return np.bincount(b, minlength=n_bins).astype(np.uint64), below, above, not_finite


def window_from_histogram(hist, h_lo, h_hi, p_lo, p_hi):
    """everything in float64, rounded once at the end"""
    hist = np.asarray(hist, np.uint64)
    n_bins = hist.size
    total = float(int(hist.sum(dtype=np.uint64)))
    assert total > 0
    cum = np.cumsum(hist, dtype=np.uint64).astype(np.float64)
    width = (float(f32(h_hi)) - float(f32(h_lo))) / n_bins
    lo_hits = np.nonzero(cum > total * p_lo / 100.0)[0]
    hi_hits = np.nonzero(cum >= total * p_hi / 100.0)[0]
    b_lo = int(lo_hits[0]) if lo_hits.size else n_bins - 1
    b_hi = int(hi_hits[0]) if hi_hits.size else n_bins - 1
    return f32(float(f32(h_lo)) + b_lo * width), f32(float(f32(h_lo)) + (b_hi + 1) * width)


def auto_window(v, p_lo=0.1, p_hi=99.9):
    """what paris.hip --voxel-range auto does: extremes, BINS_MAX bins over them, the percentile window"""
    mn, mx = extremes(v)
    hist = histogram(v, mn, mx, BINS_MAX)[0]
    return window_from_histogram(hist, mn, mx, p_lo, p_hi)


def read_mhd(path):
    """(fields, voxels): the header's key = value pairs and the .raw beside it as an array (z, y, x)"""
    fields = {}
    with open(path) as fh:
        for line in fh:
            if "=" in line:
                k, val = line.split("=", 1)
                fields[k.strip()] = val.strip()
    assert list(fields)[-1] == "ElementDataFile"
    dim_x, dim_y, dim_z = (int(t) for t in fields["DimSize"].split())
    raw = np.fromfile(os.path.join(os.path.dirname(path), fields["ElementDataFile"]), MET_TYPES[fields["ElementType"]])
    return fields, raw.reshape(dim_z, dim_y, dim_x)


def normal_volume(n, seed=11):
    """seeded normal voxels around 0.5: with the window [0, 1] a third of them lie outside on either side"""
    return np.random.default_rng(seed).normal(0.5, 1.0, n).astype(np.float32)


def mostly_one_value(n, seed=12, value=0.0):
    """90 % one value (air), the rest seeded noise"""
    rng = np.random.default_rng(seed)
    v = np.full(n, value, np.float32)
    pick = rng.random(n) < 0.1
    v[pick] = rng.normal(0.5, 0.3, int(pick.sum())).astype(np.float32)
    return v


def specials(lo, hi):
    """NaN, the infinities, both zeros, the window's ends and their neighbours"""
    lo, hi = f32(lo), f32(hi)
    inf = f32(np.inf)
    return np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, lo, hi, np.nextafter(lo, -inf), np.nextafter(lo, inf), np.nextafter(hi, -inf),
                     np.nextafter(hi, inf)], np.float32)
