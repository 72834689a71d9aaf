"""The detector roll's rule restated in numpy (include/paris_hip.h): the constants in float64 rounded once,
the pixel in np.float32 operations (each rounded once) -- or, as the float64 variant, everything in float64 with unrounded constants;
the search's margins and mirror plan in float64, its differences in the pixel's type, its sum in float64 -- and the analytic cone-beam
frames of spheres on a rolled detector that the tests recover the angle from. A helper, not a test."""
import math

import numpy as np

# the recovery case: a 96 x 80 detector, 90 views of a full circle, four off-centre spheres (x, y, z, r, rho) [mm]
N_ROW, N_COL, N_VIEWS = 96, 80, 90
L_ROW, L_COL, D_SO, D_OD = 1.2, 1.0, 300.0, 200.0
SPHERES = ((2.0, -1.0, 3.0, 16.0, 1.0), (8.0, -5.0, 13.0, 5.0, 1.5), (-10.0, 6.0, -14.0, 4.0, 1.2), (4.0, 12.0, 9.0, 3.0, 2.0))
SEARCH = (-3.0, 0.25, 25)     # lo, step, count: -3 ... 3 degrees
BOUND_DEG = 0.05              # the issue's cap; the float64 prototype gave 0.005


def geo(n_row=N_ROW, n_col=N_COL, l_row=L_ROW, l_col=L_COL, delta_s=0.0, delta_t=0.7, d_so=D_SO, d_od=D_OD, n_views=N_VIEWS):
    """the nine fields of paris_detector_geometry"""
    return (n_row, n_col, l_row, l_col, delta_s, delta_t, d_so, d_od, 360.0 / n_views)


def f32(v):
    return float(np.float32(v))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def constants(eta_deg, g, dtype=np.float32):
    """(a, b, c, d, cx, cy): computed in float64 from the fp32 fields, each rounded once to dtype"""
    n_row, n_col, l_row, l_col, delta_s, delta_t = g[0], g[1], f32(g[2]), f32(g[3]), f32(g[4]), f32(g[5])
    eta = f32(eta_deg) * math.pi / 180.0
    rho = l_col / l_row
    k = (math.cos(eta), -math.sin(eta) * rho, math.sin(eta) / rho, math.cos(eta), n_row / 2.0 + delta_s - 0.5, n_col / 2.0 + delta_t - 0.5)
    return tuple(dtype(v) for v in k)


def taps(eta_deg, g, dtype=np.float32, rows=None):
    """(i0, j0, wx, wy) of every output pixel of rows `rows` (None: all), arrays (rows, n_row)"""
    n_row, n_col = g[0], g[1]
    a, b, c, d, cx, cy = constants(eta_deg, g, dtype)
    j = np.arange(n_col)[slice(None) if rows is None else slice(rows[0], rows[0] + rows[1])]
    di = (np.arange(n_row).astype(dtype) - cx)[None, :]
    dj = (j.astype(dtype) - cy)[:, None]
    x = (a * di + b * dj) + cx
    y = (c * di + d * dj) + cy
    assert x.dtype == dtype and y.dtype == dtype
    x = np.where(x < 0, dtype(0), np.where(x > n_row - 1, dtype(n_row - 1), x))
    y = np.where(y < 0, dtype(0), np.where(y > n_col - 1, dtype(n_col - 1), y))
    i0 = np.minimum(np.floor(x).astype(np.int64), n_row - 2)
    j0 = np.minimum(np.floor(y).astype(np.int64), n_col - 2)
    wx, wy = x - i0.astype(dtype), y - j0.astype(dtype)
    assert wx.dtype == dtype and wy.dtype == dtype
    return i0, j0, wx, wy


def roll(frame, eta_deg, g, dtype=np.float32, rows=None):
    """the rule on one frame (n_col, n_row): rows `rows` of the output (None: all)"""
    p = np.ascontiguousarray(frame, dtype)
    assert p.shape == (g[1], g[0])
    i0, j0, wx, wy = taps(eta_deg, g, dtype, rows)
    with np.errstate(all="ignore"):
        top = p[j0, i0] + wx * (p[j0, i0 + 1] - p[j0, i0])
        bot = p[j0 + 1, i0] + wx * (p[j0 + 1, i0 + 1] - p[j0 + 1, i0])
        out = top + wy * (bot - top)
    assert out.dtype == dtype
    return out


def source_rows(eta_deg, g, row_first, row_count):
    """(first, count) by brute force: min j0 .. max j0 + 1 over every pixel of the band"""
    j0 = taps(eta_deg, g, np.float32, (row_first, row_count))[1]
    return int(j0.min()), int(j0.max()) + 2 - int(j0.min())


def assert_same(got, want, what=""):
    """bit for bit, except that a NaN may carry any payload"""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    nan = np.isnan(want)
    assert got.shape == want.shape and np.array_equal(np.isnan(got), nan), what
    assert np.array_equal(bits(got)[~nan], bits(want)[~nan]), what


# ---- the search -----------------------------------------------------------------------------------------------------------------------

def candidates(lo, step, count):
    """eta_k = (float)((double)lo + k (double)step), as float64 values"""
    return np.array([f32(f32(lo) + k * f32(step)) for k in range(count)], np.float64)


def margins(lo, step, count, g):
    """(m_x, m_y), from the constants as the fp32 rule rounds them"""
    n_row, n_col = g[0], g[1]
    ex = ey = 0.0
    for eta in candidates(lo, step, count):
        a, b, c, d, cx, cy = (float(v) for v in constants(eta, g))
        far_x, far_y = max(cx, n_row - 1 - cx), max(cy, n_col - 1 - cy)
        ex = max(ex, abs(b) * far_y + abs(1.0 - a) * far_x)
        ey = max(ey, abs(c) * far_x + abs(1.0 - d) * far_y)
    return int(math.ceil(ex)) + 1, int(math.ceil(ey)) + 1


def mirror_plan(g, m_x):
    """(i0, w) per column, i0 = -1 where the column is not scored; cx in float64, unrounded"""
    n_row = g[0]
    cx = n_row / 2.0 + f32(g[4]) - 0.5
    i = np.arange(n_row, dtype=np.float64)
    ip = 2.0 * cx - i
    fl = np.floor(ip)
    last = n_row - 1 - m_x
    valid = (i >= m_x) & (i <= last) & (fl >= m_x) & (fl + 1 <= last)
    return np.where(valid, fl, -1).astype(np.int64), np.where(valid, ip - fl, 0.0).astype(np.float32)


def costs(mean, lo, step, count, g, min_pixels=0, dtype=np.float32):
    """(J, pairs, skipped, (m_x, m_y)) per candidate: J = +inf where the candidate is unscored. dtype: the type of the rolled frame
    and of the differences (np.float64: the prototype)"""
    m = np.ascontiguousarray(mean, dtype)
    n_row, n_col = g[0], g[1]
    need = min_pixels if min_pixels != 0 else n_row * n_col // 16
    m_x, m_y = margins(lo, step, count, g)
    i0, w = mirror_plan(g, m_x)
    cols = np.nonzero(i0 >= 0)[0]
    j0, wc = i0[cols][None, :], w[cols].astype(dtype)[None, :]
    out = np.full(count, np.inf), np.zeros(count, np.int64), np.zeros(count, np.int64)
    for k, eta in enumerate(candidates(lo, step, count)):
        r = (m if eta == 0.0 else roll(m, eta, g, dtype))[m_y:n_col - m_y]
        with np.errstate(all="ignore"):
            d = r[:, cols] - (r[:, j0[0]] + wc * (r[:, j0[0] + 1] - r[:, j0[0]]))
        assert d.dtype == dtype
        ok = np.isfinite(d)
        out[1][k], out[2][k] = np.count_nonzero(ok), d.size - np.count_nonzero(ok)
        if out[1][k] >= need and out[1][k] > 0:
            out[0][k] = math.fsum(d[ok].astype(np.float64) ** 2) / int(out[1][k])
    return out + ((m_x, m_y),)


def estimate(lo, step, cost):
    """the shared estimate: dict(value, best, cost_min, cost_median, scored, at_edge), or None when nothing is scored"""
    cost = np.asarray(cost, np.float64)
    c = candidates(lo, step, cost.size)
    scored = np.isfinite(cost)
    if not scored.any():
        return None
    m = int(np.argmin(np.where(scored, cost, np.inf)))
    js = np.sort(cost[scored])
    out = dict(best=m, cost_min=cost[m], cost_median=js[(js.size - 1) // 2], scored=int(scored.sum()), at_edge=1, value=np.float32(c[m]))
    if 1 <= m < cost.size - 1 and scored[m - 1] and scored[m + 1]:
        with np.errstate(over="ignore"):
            q = cost[m - 1] - 2.0 * cost[m] + cost[m + 1]
        if q > 0:
            off = min(max(0.5 * (cost[m - 1] - cost[m + 1]) / q, -0.5), 0.5)
            out.update(value=np.float32(c[m] + off * f32(step)), at_edge=0)
    return out


# ---- analytic frames --------------------------------------------------------------------------------------------------------------

def sphere_frames(g, eta_deg=0.0, spheres=SPHERES, n_views=None):
    """float64 (views, n_col, n_row): the line integrals of the spheres on a detector rolled by eta_deg -- pixel (i, j) of it sits at
    (t, v) = (cos eta t_i + sin eta v_j, -sin eta t_i + cos eta v_j) [mm], t_i = ((i + 1/2) - n_row / 2 - delta_s) l_px_row and v_j
    likewise: the rays are evaluated at the rotated pixel positions, nothing is interpolated. The rule with the same eta_deg undoes
    it. Source (-d_so cos phi, -d_so sin phi, 0); the pixel at (d_od cos phi - t sin phi, d_od sin phi + t cos phi, v)."""
    n_row, n_col, l_row, l_col, delta_s, delta_t, d_so, d_od, delta_phi = g
    n_views = int(round(360.0 / delta_phi)) if n_views is None else n_views
    eta = math.radians(eta_deg)
    t0 = (((np.arange(n_row) + 0.5) - n_row / 2.0 - f32(delta_s)) * f32(l_row))[None, :]
    v0 = (((np.arange(n_col) + 0.5) - n_col / 2.0 - f32(delta_t)) * f32(l_col))[:, None]
    t = math.cos(eta) * t0 + math.sin(eta) * v0
    v = -math.sin(eta) * t0 + math.cos(eta) * v0
    out = np.zeros((n_views, n_col, n_row))
    for f in range(n_views):
        phi = 2.0 * math.pi * f / n_views
        cp, sp = math.cos(phi), math.sin(phi)
        s = np.array([-d_so * cp, -d_so * sp, 0.0])
        u = np.stack([d_od * cp - t * sp - s[0], d_od * sp + t * cp - s[1], v - s[2]], axis=-1)
        u /= np.linalg.norm(u, axis=-1, keepdims=True)
        for x, y, z, r, rho in spheres:
            w = np.array([x, y, z]) - s
            along = u @ w
            d2 = w @ w - along * along
            out[f] += 2.0 * rho * np.sqrt(np.maximum(r * r - d2, 0.0))
    return out


_CACHE = {}


def scan(eta_deg, delta_s=0.0, n_views=N_VIEWS):
    """(geometry, frames float64, read-only) of the recovery case, made once per setting"""
    key = (eta_deg, delta_s, n_views)
    if key not in _CACHE:
        g = geo(delta_s=delta_s, n_views=n_views)
        frames = sphere_frames(g, eta_deg)
        frames.setflags(write=False)
        _CACHE[key] = (g, frames)
    return _CACHE[key]


def special_frame(n_row=67, n_col=45, seed=5):
    """an fp32 frame whose interpolation rounds, with NaN, +-Inf and -0 pixels"""
    rng = np.random.default_rng(seed)
    f = (rng.uniform(-1.0, 3.0, (n_col, n_row)) * rng.choice([1.0, 1e-3, 1e3], (n_col, n_row))).astype(np.float32)
    f[3, 5] = np.nan
    f[20, 40] = np.inf
    f[30, 11] = -np.inf
    f[10, 60] = -0.0
    f[0, 0] = -0.0
    f[n_col - 1, n_row - 1] = np.nan
    return f


# The benefit case: the same detector area at 192 x 160 pixels, 72 views, four spheres far from the mid-plane, reconstructed into 64^3
# voxels of 1.05 x 1.05 x 0.72 mm. The rule blurs by up to half a detector pixel, so its gain shows where the roll moves edges by more
# than that and the voxels are coarser than the blur. With the float64 rule and the CPU oracle, RMS difference from the reconstruction
# of the unrolled scan over the central cylinder: 0.106 uncorrected, 0.0240 corrected (ratio 0.23). With the recovery spheres, which
# sit near the mid-plane, the ratio is 0.67; on a 96 x 80 detector no phantom reached one half (0.62 at best).
BENEFIT_ETA = 1.2
BENEFIT_GEO = (192, 160, 0.6, 0.5, 0.0, 0.7, D_SO, D_OD, 5.0)
BENEFIT_VOLUME = (64, 64, 64, 1.05, 1.05, 0.72)
BENEFIT_SPHERES = ((20.0, 5.0, 17.0, 4.0, 1.0), (-18.0, -10.0, -17.0, 4.0, 1.0), (5.0, -22.0, 16.0, 4.0, 1.0), (-8.0, 21.0, -16.0, 4.0, 1.0))


def cylinder_rms(a, b):
    """the RMS difference of two volumes (dim_z, dim_y, dim_x) inside 0.45 dim_x of the axis, every slice"""
    dz, dy, dx = a.shape
    y, x = np.mgrid[:dy, :dx]
    m = np.hypot(x - (dx - 1) / 2, y - (dy - 1) / 2) <= 0.45 * dx
    return float(np.sqrt(np.mean((a[:, m].astype(np.float64) - b[:, m].astype(np.float64)) ** 2)))


HOST_GEO = (67, 45, 0.2, 0.25, 1.3, -0.7, 100.0, 200.0, 4.0)     # odd width, no multiple of 4; l_px_col != l_px_row
HOST_ETAS = (0.3, -0.3, 2.5, -10.0)
