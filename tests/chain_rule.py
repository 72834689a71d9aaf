"""The frame chain between the raw upload and the cosine weight as ONE rule: the numpy rules of the single
passes composed in the documented order -- binning, dark / flat correction, air normalisation, defect repair, zinger filter, ring
correction, beam hardening (README; DESIGN.md sections 4.6, 4.9, 4.10, 4.12, 4.14, 4.16, 4.17) --, the driver's row rule for a slab's
band restated, and the scan the chain tests share. Nothing here touches a device. A helper, not a test."""
import types

import numpy as np

import air_rule
import beam_hardening_rule
import binning_rule
import phantom
import ring_rule
import zinger_rule
from paris_amd import backend as B

STEPS = ("bin", "flat", "air", "repair", "zingers", "rings", "beam_hardening")

GEO = (67, 45, 0.2, 0.25, 1.5, -0.75, 100, 200, 10.0)     # the detector of tests/test_gpu_binning_driver.py, a full circle of 36 views
N_FRAMES = 36
T_MIN = 1e-5
RADIUS = 1.4                          # [mm] of the head phantom: it leaves the detector's first and last rows in air
P_MAX = 2.5                           # the largest line integral: 8 % transmission
DRIFT = 0.05                          # per-frame flux drift: the counts times 1 + e_f, e_f uniform in +-DRIFT
ZINGERS = (0.25, 0.0, 0)              # threshold_abs, threshold_rel, polarity (both)
RINGS = (ring_rule.H, ring_rule.FLOOR, ring_rule.LIMIT)
BH = (0.93, 0.11)
# the air rectangle (x0, y0, width, height) on the detector the chain runs on, by bin factor: the corner at the last columns of the
# first rows, which the phantom never reaches and where the shared mask has only scattered pixels
AIR_RECT = {1: (54, 1, 12, 6), 2: (27, 0, 6, 4)}
SENTINEL = np.uint32(0x7FC0FEED)      # a NaN with a payload, for the rows a band run must not write


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- the scan ---------------------------------------------------------------------------------------------------------------------

def scan(seed=17, geo=None):
    """u16 counts (N_FRAMES, 45, 67) with a dark, a flat (whole counts: one u16 frame each is their mean) and the shared defect mask.
    counts = dark + (flat - dark) exp(-p) exp(-off) (1 + e_f) + noise: p the head phantom's line integrals, off the stationary offsets
    of ring_rule.offsets, e_f the frame's flux drift; then zingers -- counts cut to a third or tripled -- on the corners, on the edges,
    as a pair, as 2 x 2 blocks that cover whole bins and as single pixels, at places that move from frame to frame. A dead pixel of the
    references at (20, 21), as in tests/test_gpu_binning_driver.py."""
    geo = GEO if geo is None else geo
    n_row, n_col, lr, lc, ds, dt, d_so, d_od, step = geo
    rng = np.random.default_rng(seed)
    lines = [phantom.projection(n_row, n_col, lr, lc, d_so, d_od, float(np.float32(i) * np.float32(step)), RADIUS, ds, dt) for i in range(N_FRAMES)]
    mu = P_MAX / max(float(p.max()) for p in lines)
    lines = np.stack([(mu * p).astype(np.float32) for p in lines])
    for b, (x0, y0, w, h) in AIR_RECT.items():
        assert not lines[:, b * y0:b * (y0 + h), b * x0:b * (x0 + w)].any(), "the phantom reaches the air rectangle"
    shape = (n_col, n_row)
    dark = np.rint(150 + 300 * rng.random(shape)).astype(np.float32)
    flat = np.rint(dark + 50000 * (0.85 + 0.15 * rng.random(shape))).astype(np.float32)
    dark[20, 21] = flat[20, 21] = 300
    off = ring_rule.offsets(n_row, n_col, seed)
    eps = rng.uniform(-DRIFT, DRIFT, N_FRAMES)
    eps[:2] = (-DRIFT, DRIFT)
    signal = (flat - dark) * np.exp(-lines.astype(np.float64) - off) * (1.0 + eps)[:, None, None]
    signal = signal + rng.normal(0, 30, signal.shape)
    planted = np.zeros(signal.shape, bool)
    for f in range(N_FRAMES):
        spots = [(0, 0, 3.0), (0, n_row - 1, 1 / 3), (n_col - 1, 0, 1 / 3), (n_col - 1, n_row - 1, 3.0),                  # corners
                 (0, 20 + f % 9, 1 / 3), (n_col - 1, 30 + f % 9, 3.0), (10 + f % 20, 0, 1 / 3), (12 + f % 20, n_row - 1, 1 / 3),  # edges
                 (18 + f % 5, 24, 1 / 3), (18 + f % 5, 25, 1 / 3)]                                                          # a pair
        for y, x, g in ((16 + 2 * (f % 6), 40 + 2 * (f % 4), 1 / 3), (24 + 2 * (f % 3), 28 + 2 * (f % 5), 3.0)):             # whole bins
            spots += [(y + j, x + i, g) for j in range(2) for i in range(2)]
        spots += [(int(y), int(x), 1 / 3 if k % 2 else 3.0) for k, (y, x) in enumerate(zip(rng.integers(2, n_col - 2, 8), rng.integers(2, n_row - 2, 8)))]
        for y, x, g in spots:
            signal[f, y, x] *= g
            planted[f, y, x] = True
    counts = np.clip(np.rint(dark + signal), 0, 65535).astype(np.uint16)
    return types.SimpleNamespace(counts=counts, dark=dark, flat=flat, mask=scan_mask(n_row, n_col), eps=eps, lines=lines,
                                 planted=planted, off=off, geo=geo)


EDGE_BLOCK = (22, 15, 8)     # first row, rows, columns of a bad block on the detector's left edge


def scan_mask(n_row, n_col):
    """binning_rule.shared_mask plus a bad block of 15 rows x 8 columns on the left edge. The pixel in the middle of its edge column,
    (29, 0), has no good pixel on the rings 1 .. 7: its sources lie on ring 8, in rows 21 and 37 and in column 8 between them -- the
    repair's whole reach, above and below (binned 2 x 2: (14, 0), ring 4, rows 10 and 18). A band whose widened range ends at that pixel
    needs every row of `up`: one row short, and the repair reads a row that was never uploaded."""
    m = binning_rule.shared_mask(n_row, n_col)
    first, count, width = EDGE_BLOCK
    m[first:first + count, :width] = 1
    return m


def dead_pixels(dark, flat):
    """what paris_hip_flat_field_dead_pixels marks: a reference that is not finite, or a flat that is not above its dark"""
    with np.errstate(invalid="ignore"):
        return (~(np.isfinite(dark) & np.isfinite(flat) & (flat > dark))).astype(np.uint8)


def settings(s, bin_factor):
    """What the driver sets from the scan's files with --bin B --flat --dark --defects --defects-from-flat --air-region --zingers --rings
    --beam-hardening (B = 1: no --bin): the references and the map at the size the chain runs on. With --bin the source mask -- the
    file's OR the source references' dead pixels -- leaves pixels out of their bins, the references are binned by the same rule, and the
    map is the binned mask OR the binned references' dead pixels."""
    b = int(bin_factor)
    st = types.SimpleNamespace(bin=b, src_x=GEO[0], src_y=GEO[1], t_min=T_MIN, zingers=ZINGERS, rings=RINGS, bh=BH, rect=AIR_RECT[b])
    if b == 1:
        st.src_mask = None
        st.dark, st.flat = s.dark, s.flat
        st.mask = s.mask | dead_pixels(s.dark, s.flat)
        st.geo = s.geo
    else:
        st.src_mask = ((s.mask != 0) | (dead_pixels(s.dark, s.flat) != 0)).astype(np.uint8)
        st.dark, st.flat = binning_rule.bin_frame(s.dark, b, b, st.src_mask), binning_rule.bin_frame(s.flat, b, b, st.src_mask)
        st.mask = binning_rule.bin_mask(st.src_mask, b, b) | dead_pixels(st.dark, st.flat)
        st.geo = binning_rule.binned_geometry(s.geo, b, b)
    st.mask = (st.mask != 0).astype(np.uint8)
    st.dim_x, st.dim_y = GEO[0] // b, GEO[1] // b
    st.plan = B.defect_plan(st.mask)          # host only: tests/test_defect_map_host.py holds the plan to its numpy restatement
    return st


# ---- the passes the other rule files do not state for a stack of frames ----------------------------------------------------------

def flat_field(frames, dark, flat, t_min):
    """the contract in float64, rounded once: -ln(max((I - D) / (F - D), t_min)), 0 for a dead pixel"""
    i64 = np.asarray(frames, np.float32).astype(np.float64)
    d64, f64 = np.asarray(dark, np.float32).astype(np.float64), np.asarray(flat, np.float32).astype(np.float64)
    ok = np.isfinite(i64) & np.isfinite(d64) & np.isfinite(f64) & (f64 - d64 > 0)
    with np.errstate(all="ignore"):
        p = -np.log(np.maximum((i64 - d64) / (f64 - d64), np.float64(np.float32(t_min))))
    return np.where(ok, p, 0.0).astype(np.float32)


def repair(frames, plan):
    """binning_rule.repair32 for a stack of frames at once: per defect acc = 0, then acc = fmaf(w, p, acc) over its sources in the
    plan's order (sources are good pixels, so every defect reads the frame as it was)"""
    out = np.array(frames, np.float32)
    n = out.shape[0]
    flat, src = out.reshape(n, -1), np.array(frames, np.float32).reshape(n, -1)
    first, count = plan.first_source[:-1].astype(np.int64), np.diff(plan.first_source.astype(np.int64))
    acc = np.zeros((n, len(plan.defect)), np.float32)
    for j in range(int(count.max()) if len(count) else 0):
        has = count > j
        at = first[has] + j
        acc[:, has] = beam_hardening_rule.fmaf(plan.weight[at][None, :], src[:, plan.source[at]], acc[:, has])
    flat[:, plan.defect] = acc
    return out


def decimate(frames, b):
    """NOT the binning rule: the first source pixel of every bin. What `without="bin"` puts in its place, so that the shapes still fit"""
    f = np.asarray(frames, np.float32)
    return np.ascontiguousarray(f[:, :f.shape[1] // b * b:b, :f.shape[2] // b * b:b])


# ---- the chain --------------------------------------------------------------------------------------------------------------------

def chain(counts, st, upto=len(STEPS), without=None, order=STEPS):
    """The stack of frames after every step: result[0] the counts as float32, result[k] the frames after step k of `order`, for k up
    to `upto`. The ring correction is the rule's on the mean of ALL frames given, taken after the zinger filter, as the driver's pre-pass
    takes it. Returns (steps, info): info holds the air values with their reasons, the zingers replaced per frame and whether a frame
    saturated, and the ring correction with its stats. without: a step that is left out (the final frames must then differ:
    assert_every_pass_counts); order: the steps in another order, which is another rule."""
    f = np.asarray(counts).astype(np.float32)
    steps, info = [f], types.SimpleNamespace()
    for name in order[:upto]:
        if name == without:
            f = decimate(f, st.bin) if name == "bin" else f
        elif name == "bin":
            f = f if st.bin == 1 else np.stack([binning_rule.bin_frame(x, st.bin, st.bin, st.src_mask) for x in f])
        elif name == "flat":
            f = flat_field(f, st.dark, st.flat, st.t_min)
        elif name == "air":
            info.air, info.air_pixels, info.air_why = air_rule.values(list(f), st.rect, mask=st.mask)
            f = np.stack([air_rule.subtract(x, a) for x, a in zip(f, info.air)])
        elif name == "repair":
            f = repair(f, st.plan)
        elif name == "zingers":
            got = [zinger_rule.apply(x, *st.zingers) for x in f]
            info.replaced, info.saturated = [g[1] for g in got], [g[2] for g in got]
            f = np.stack([g[0] for g in got]).astype(np.float32)
        elif name == "rings":
            counts_per_row = np.full(f.shape[1], len(f), np.uint32)
            info.ring_mean = ring_rule.mean_of(ring_rule.sums(list(f)), len(f))
            info.ring_c, info.ring_stats = ring_rule.correction(info.ring_mean, *st.rings, counts=counts_per_row)
            f = np.stack([ring_rule.subtract(x, info.ring_c) for x in f])
        elif name == "beam_hardening":
            f = beam_hardening_rule.apply(st.bh, f)
        else:
            raise ValueError(name)
        steps.append(f)
    return steps, info


def assert_every_pass_counts(counts, st, steps, info):
    """Every pass of the chain changes bits of the final frames -- the chain without it gives others --, no frame saturates the zinger
    filter, the ring correction is not all zero, every frame is air-normalised and the map has defects to repair: with these, an equality
    with the composed frames cannot be met by passes that do nothing. Numpy alone, no device."""
    final = steps[-1]
    assert final.shape == (len(counts), st.dim_y, st.dim_x) and np.isfinite(final).all()
    for k, name in enumerate(STEPS):
        if name == "bin" and st.bin == 1:
            continue                       # no --bin: the pass is not part of the chain
        assert not np.array_equal(bits(steps[k + 1]), bits(steps[k])) or name == "bin", name
        without = chain(counts, st, without=name)[0][-1]
        differing = np.count_nonzero(bits(without) != bits(final))
        assert differing > 0, "the chain without %s gives the same final frames" % name
    assert not any(info.saturated) and sum(info.replaced) > len(counts)
    assert info.ring_stats["corrected"] > 20 and np.count_nonzero(info.ring_c) == info.ring_stats["corrected"]
    assert info.air_why == ["normalised"] * len(counts) and np.all(info.air != 0)
    assert st.plan.defects - st.plan.unrepairable == len(st.plan.defect) > 20


# ---- the rows of a band -----------------------------------------------------------------------------------------------------------

def band_rows(band_first, band_count, dim_y, reach_rows, zingers, rect, bin_y):
    """The driver's row rule for the band a slab needs (paris_amd/host/paris/reconstruct.h), each range as (first, count):
      band  the rows that are zinger-filtered, ring-corrected, linearised, weighted and filtered;
      fix   the band widened by the zinger windows' one row: the rows whose defects are repaired;
      air   the band widened by that row plus the repair's reach: the rows the frame's air value is subtracted from;
      up    `air` hulled with the air rectangle's rows: the rows that are uploaded, binned and corrected;
      src   the source rows of `up`: bin_y times as many.
    Every widening is clipped to the detector; an empty band stays empty."""
    zinger_rows = 1 if zingers else 0

    def widened(by):
        first = band_first - min(band_first, by)
        return first, min(dim_y - (band_first + band_count), by) + band_first + band_count - first

    band = (band_first, band_count)
    if band_count == 0:
        return types.SimpleNamespace(band=band, fix=band, air=band, up=band, src=(bin_y * band_first, 0))
    up, fix = widened(reach_rows + zinger_rows), widened(zinger_rows)
    air = up
    if rect is not None:
        lo, hi = min(up[0], rect[1]), max(up[0] + up[1], rect[1] + rect[3])
        up = (lo, hi - lo)
    return types.SimpleNamespace(band=band, fix=fix, air=air, up=up, src=(bin_y * up[0], bin_y * up[1]))


def rows(r):
    return slice(r[0], r[0] + r[1])


def expected_band(steps, r):
    """What a band run leaves in frames that held SENTINEL everywhere, from the whole-frame chain's steps: outside `up` the sentinel;
    in `up` the corrected rows; in `air` the normalised ones; in `fix` the repaired ones; in `band` the final ones"""
    final = steps[-1]
    out = np.full(final.shape, SENTINEL, np.uint32).view(np.float32)
    out[:, rows(r.up)] = steps[2][:, rows(r.up)]
    out[:, rows(r.air)] = steps[3][:, rows(r.air)]
    out[:, rows(r.fix)] = steps[4][:, rows(r.fix)]
    out[:, rows(r.band)] = final[:, rows(r.band)]
    return out
