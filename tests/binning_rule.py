"""The detector-binning rule of include/paris_hip.h restated in numpy, and the frames and masks the tests
share. No library call in here: this is what the host functions and the device are compared against."""
from fractions import Fraction

import numpy as np

FACTORS = (1, 2, 4, 8)
SETTINGS = [(bx, by) for bx in FACTORS for by in FACTORS]


def binned_size(bin_x, bin_y, dim_x, dim_y):
    return dim_x // bin_x, dim_y // bin_y


def _blocks(a, bin_x, bin_y):
    """(out_y, out_x, bin_y, bin_x) view of the source pixels of every bin, the remainder dropped"""
    dim_y, dim_x = a.shape
    ox, oy = binned_size(bin_x, bin_y, dim_x, dim_y)
    return a[:oy * bin_y, :ox * bin_x].reshape(oy, bin_y, ox, bin_x).transpose(0, 2, 1, 3)


def bin_frame(frame, bin_x, bin_y, mask=None, column_major=False):
    """acc = +0; for each good source pixel, rows outer and columns inner: acc = acc + p in fp32; out = acc / (float)n, +0 for n = 0.
    column_major: the WRONG order (columns outer), for showing that a frame makes the order observable."""
    f = np.ascontiguousarray(frame, np.float32)
    b = _blocks(f, bin_x, bin_y)
    good = np.ones(b.shape, bool) if mask is None else _blocks(np.asarray(mask) == 0, bin_x, bin_y)
    acc = np.zeros(b.shape[:2], np.float32)
    n = np.zeros(b.shape[:2], np.uint32)
    order = [(r, c) for c in range(bin_x) for r in range(bin_y)] if column_major else [(r, c) for r in range(bin_y) for c in range(bin_x)]
    with np.errstate(all="ignore"):
        for r, c in order:
            g = good[:, :, r, c]
            acc = np.where(g, acc + b[:, :, r, c], acc)   # float32 + float32: one rounding
            n += g
        out = np.where(n > 0, acc / np.maximum(n, 1).astype(np.float32), np.float32(0))
    assert out.dtype == np.float32
    return out


def bin_mask(mask, bin_x, bin_y):
    """1 where no source pixel of the bin is good"""
    bad = _blocks(np.asarray(mask) != 0, bin_x, bin_y)
    return bad.all(axis=(2, 3)).astype(np.uint8)


def binned_geometry(geo, bin_x, bin_y):
    """geo = (n_row, n_col, l_px_row, l_px_col, delta_s, delta_t, d_so, d_od, delta_phi), the float fields as fp32 values; every
    binned field from them in float64, rounded once"""
    n_row, n_col = geo[:2]
    lr, lc, ds, dt = (float(np.float32(v)) for v in geo[2:6])
    ox, oy = binned_size(bin_x, bin_y, n_row, n_col)
    r_x, r_y = n_row - ox * bin_x, n_col - oy * bin_y
    return (ox, oy, np.float32(bin_x * lr), np.float32(bin_y * lc), np.float32((ds + r_x / 2) / bin_x), np.float32((dt + r_y / 2) / bin_y),
            np.float32(geo[6]), np.float32(geo[7]), np.float32(geo[8]))


def shared_mask(dim_x=67, dim_y=45):
    """for every setting: a fully bad bin (the 8 x 8 block at the origin), a bin with exactly one good pixel (the 8 x 8 block beside it
    but for its last pixel -- which is the one good pixel of its bin for every setting), a bad full row and a bad full column, and
    scattered pixels"""
    m = np.zeros((dim_y, dim_x), np.uint8)
    m[0:8, 0:8] = 1
    m[8:16, 8:16] = 255      # (any nonzero byte marks)
    m[15, 15] = 0
    m[29, :] = 1
    m[:, 37] = 1
    rng = np.random.default_rng(5)
    m.reshape(-1)[rng.choice(m.size, m.size // 40, replace=False)] = 1
    m[15, 15] = 0
    return m


def counts_frame(dim_x=67, dim_y=45, seed=1):
    """u16 detector counts"""
    return np.random.default_rng(seed).integers(0, 65536, (dim_y, dim_x)).astype(np.uint16)


def ordered_frame(dim_x=67, dim_y=45, seed=2, special=True):
    """an f32 frame whose bin sums depend on the order of the additions: magnitudes spanning 2^20, both signs; with a NaN and an inf"""
    rng = np.random.default_rng(seed)
    f = (rng.standard_normal((dim_y, dim_x)) * np.exp2(rng.uniform(0, 20, (dim_y, dim_x)))).astype(np.float32)
    if special:
        f[3, 5] = np.nan
        f[20, 40] = np.inf
        f[21, 50] = -0.0
    return f


# ---- exact fp32 arithmetic for the chain test: fmaf(a, b, c) rounded once ---------------------------------------------------------

def round_f32(q):
    """the Fraction q rounded to the nearest float32, ties to even (finite, normal range)"""
    f = np.float32(float(q))   # rounded twice: right or one step off
    best = None
    for c in (np.nextafter(f, np.float32(-np.inf)), f, np.nextafter(f, np.float32(np.inf))):
        d = abs(Fraction(float(c)) - q)
        even = (int(np.float32(c).view(np.uint32)) & 1) == 0
        if best is None or d < best[0] or (d == best[0] and even):
            best = (d, c)
    return np.float32(best[1])


def fmaf(a, b, c):
    return round_f32(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def repair32(frame, plan):
    """the defect repair as the device runs it (paris_amd/csrc/defect_map.hip): per defect acc = 0, then acc = fmaf(w, p, acc) over
    its sources in the plan's order, with the plan's fp32 weights; sources are good pixels, so the order of the defects is free"""
    out = np.array(frame, np.float32)
    flat = out.reshape(-1)
    src = np.array(frame, np.float32).reshape(-1)
    for k, q in enumerate(plan.defect):
        acc = np.float32(0)
        for s in range(plan.first_source[k], plan.first_source[k + 1]):
            acc = fmaf(plan.weight[s], src[plan.source[s]], acc)
        flat[q] = acc
    return out
