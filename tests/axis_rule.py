"""The axis search's rule restated in numpy (include/paris_hip.h): the band, the plan and the estimate in
float64, the pair in np.float32 operations (each rounded once), the sum in float64 -- and the analytic fan-beam sinogram of discs the
tests recover an offset from. atan is math.atan, the C library's, as the library's own: numpy's vector arctan may differ in the last
bit."""
import math

import numpy as np

# the issue's recovery case: N = n = 96, l = 1.2, d_so = 300, d_od = 200, four discs (cx, cy, r, rho), true delta_s 2.4
DISCS = ((0.0, 0.0, 20.0, 1.0), (7.0, -4.0, 5.0, 1.5), (-9.0, 6.0, 3.0, -0.8), (3.0, 11.0, 2.0, 2.0))
L_PX, D_SO, D_OD = 1.2, 300.0, 200.0
BOUND_PX = 0.1       # three times the float64 prototype's worst error (0.032 px)


def f32(v):
    return float(np.float32(v))


def candidates(lo, step, count):
    """c_k = (float)((double)lo + k (double)step), as float64 values"""
    return np.array([f32(f32(lo) + k * f32(step)) for k in range(count)], np.float64)


def resolved_min_columns(min_columns, n):
    return min_columns if min_columns != 0 else max(8, n // 16)


def row_first(n_col, delta_t, rows):
    j_c = n_col / 2.0 + f32(delta_t) - 0.5
    first = math.floor(j_c - (rows - 1) / 2.0 + 0.5)
    return int(min(max(first, 0), n_col - rows))


def plan(c, n, n_frames, l_px_row, d_so, d_od):
    """candidate c (a float64 that holds a float32): (i0, k0, wi, wf) per column; i0 = -1 and zeros where the column is invalid"""
    l, d_sd = f32(l_px_row), abs(f32(d_so)) + abs(f32(d_od))
    i = np.arange(n, dtype=np.float64)
    ip = (n - 1 - i) + 2.0 * c
    fl = np.floor(ip)
    valid = (fl >= 0) & (fl + 1 <= n - 1)
    gamma = np.array([math.atan(v) for v in (((i + 0.5) - n / 2.0 - c) * l) / d_sd])
    kk = n_frames / 2.0 + (gamma * n_frames) / math.pi
    kf = np.floor(kk)
    i0 = np.where(valid, fl, -1).astype(np.int64)
    k0 = np.where(valid, np.mod(kf, n_frames), 0).astype(np.int64)
    wi = np.where(valid, (ip - fl).astype(np.float32), np.float32(0))
    wf = np.where(valid, (kk - kf).astype(np.float32), np.float32(0))
    return i0, k0, wi.astype(np.float32), wf.astype(np.float32)


def sinogram_of(frames, first, rows):
    """S[f][i]: acc = +0, acc = acc + p over the band's rows in ascending order, in fp32"""
    frames = np.asarray(frames, np.float32)
    acc = np.zeros((frames.shape[0], frames.shape[2]), np.float32)
    with np.errstate(all="ignore"):
        for r in range(rows):
            acc = acc + frames[:, first + r, :]
    return acc


def differences(s, i0, k0, wi, wf):
    """d for every view and every valid column, in fp32: (N, valid columns)"""
    n_frames = s.shape[0]
    cols = np.nonzero(i0 >= 0)[0]
    fa = (np.arange(n_frames)[:, None] + k0[cols][None, :]) % n_frames
    fb = (fa + 1) % n_frames
    j, w, v = i0[cols][None, :], wi[cols][None, :], wf[cols][None, :]
    with np.errstate(all="ignore"):
        a = s[fa, j] + w * (s[fa, j + 1] - s[fa, j])
        b = s[fb, j] + w * (s[fb, j + 1] - s[fb, j])
        d = s[:, cols] - (a + v * (b - a))
    assert d.dtype == np.float32
    return d


def costs(s, lo, step, count, n_frames, l_px_row, d_so, d_od, min_columns=0):
    """(J, columns, pairs, skipped) per candidate: J = +inf where the candidate is unscored"""
    s = np.ascontiguousarray(s, np.float32)
    n = s.shape[1]
    need = resolved_min_columns(min_columns, n)
    out = np.full(count, np.inf), np.zeros(count, np.int64), np.zeros(count, np.int64), np.zeros(count, np.int64)
    for k, c in enumerate(candidates(lo, step, count)):
        i0, k0, wi, wf = plan(c, n, n_frames, l_px_row, d_so, d_od)
        d = differences(s, i0, k0, wi, wf)
        ok = np.isfinite(d)
        out[1][k], out[2][k], out[3][k] = np.count_nonzero(i0 >= 0), np.count_nonzero(ok), d.size - np.count_nonzero(ok)
        if out[1][k] >= need and out[2][k] > 0:
            out[0][k] = np.sum(d[ok].astype(np.float64) ** 2) / int(out[2][k])
    return out


def estimate(lo, step, cost):
    """the host's estimate: dict(delta_s, best, cost_min, cost_median, scored, at_edge), or None when nothing is scored"""
    cost = np.asarray(cost, np.float64)
    c = candidates(lo, step, cost.size)
    scored = np.isfinite(cost)
    if not scored.any():
        return None
    m = int(np.argmin(np.where(scored, cost, np.inf)))      # the first of equal minima
    js = np.sort(cost[scored])
    out = dict(best=m, cost_min=cost[m], cost_median=js[(js.size - 1) // 2], scored=int(scored.sum()), at_edge=1, delta_s=np.float32(c[m]))
    if 1 <= m < cost.size - 1 and scored[m - 1] and scored[m + 1]:
        with np.errstate(over="ignore"):
            q = cost[m - 1] - 2.0 * cost[m] + cost[m + 1]
        if q > 0:
            off = min(max(0.5 * (cost[m - 1] - cost[m + 1]) / q, -0.5), 0.5)
            out.update(delta_s=np.float32(c[m] + off * f32(step)), at_edge=0)
    return out


def disc_sinogram(n_frames, n, delta_s, discs=DISCS, l_px_row=L_PX, d_so=D_SO, d_od=D_OD):
    """the analytic fan-beam sinogram, float64 (N, n): for a disc, distance = (C - S) . (-sin theta, cos theta) with theta = phi +
    gamma, value = 2 rho sqrt(max(r^2 - distance^2, 0))"""
    phi = (2.0 * np.pi * np.arange(n_frames) / n_frames)[:, None]
    t = ((np.arange(n) + 0.5) - n / 2.0 - delta_s) * l_px_row
    theta = phi + np.arctan(t / (abs(d_so) + abs(d_od)))[None, :]
    sx, sy = -d_so * np.cos(phi), -d_so * np.sin(phi)
    out = np.zeros((n_frames, n))
    for cx, cy, r, rho in discs:
        dist = (cx - sx) * -np.sin(theta) + (cy - sy) * np.cos(theta)
        out += 2.0 * rho * np.sqrt(np.maximum(r * r - dist * dist, 0.0))
    return out


def recover(s, lo, step, count, **geo):
    n_frames = s.shape[0]
    g = dict(l_px_row=L_PX, d_so=D_SO, d_od=D_OD)
    g.update(geo)
    j, columns, pairs, skipped = costs(s, lo, step, count, n_frames, g["l_px_row"], g["d_so"], g["d_od"])
    return estimate(lo, step, j), j
