"""The FDK chain -- cosine weight, ramp filter, voxel-driven backprojection -- restated in float64 from its equations.

A test helper, not a test: numpy only, float64 throughout, no call into oracle/ or paris_amd/. The geometry arguments are read by
attribute (n_row, n_col, l_px_row, l_px_col, delta_s, delta_t, d_so, d_od; dim_x .. l_vx_z; x1 .. z2), so the oracle's and the
library's ctypes structures both serve; their float32 fields are taken as the exact numbers they hold. What follows is the contract:
the reference's conventions, which the oracle and the kernels have to share with this file.

Detector. Pixel (i, j), i along a row (n_row pixels of pitch l_px_row), j along a column (n_col rows of pitch l_px_col); a
projection is an (n_col, n_row) array. delta_s, delta_t are detector offsets in pixels. d_sd = |d_so| + |d_od|.

weight (Q6: the offset enters with a PLUS sign here)
    h_i = (i + 1/2) l_px_row + delta_s l_px_row - n_row l_px_row / 2,   v_j likewise with l_px_col, delta_t, n_col
    w_ij = d_sd / sqrt(d_sd^2 + h_i^2 + v_j^2),                          p_ij <- p_ij w_ij

ramp (Q11, Q16: the only filter; the band-limited ramp's spatial kernel, halved)
    r[0] = 1 / (8 tau^2),  r[j] = 0 for even j != 0,  r[j] = -1 / (2 j^2 pi^2 tau^2) for odd j,        tau = l_px_row
    q[x] = sum_i p[i] tau r[x - i]      over the whole row, i.e. |x - i| <= n_row - 1: a direct spatial convolution, no FFT.
    The reference multiplies the row's spectrum, zero-padded to N = 2 * 2^ceil(log2 n_row), by K = tau |DFT_N(r)| in both
    components and keeps the first n_row samples. That is this sum, because (1) r is even in j and r[N/2] = 0 (N/2 is even), so its
    DFT is real, and it is positive -- at DC it is 1/(8 tau^2) minus a partial sum of 1/(pi^2 tau^2) * sum_{odd j} 1/j^2 =
    1/(8 tau^2), elsewhere larger -- so |.| changes nothing and K is the spectrum of tau r itself (zero phase, Q11); (2) the product of
    spectra is the circular convolution of period N with taps j = -(N/2 - 1) .. N/2, and N >= 2 n_row keeps every x - i with
    0 <= x, i < n_row inside |x - i| <= N/2 - 1: no tap wraps around onto the row.

backproject (one view at angle phi, added to the volume)
    voxel centre of GLOBAL index K on an axis of dim voxels of edge l:  (K + 1/2) l - dim l / 2;
        the global index of voxel (k, l, m) of the array is (k + roi.x1, l + roi.y1, m + roi.z1 + v_offset) (no roi: zeros)
    s = x cos phi + y sin phi,   t = -x sin phi + y cos phi,   f = d_sd / (s + d_so)      (d_so as given, with its sign)
    h = (t f + n_row l_px_row / 2 + delta_s l_px_row) / l_px_row - 1/2
    v = (z f + n_col l_px_col / 2 + delta_t l_px_col) / l_px_col - 1/2
        (Q6: the opposite sign to the weight -- here pixel i is centred at t f = (i + 1/2) l_px_row - n_row l_px_row / 2 - delta_s l_px_row)
    sample = bilinear interpolation of p at (h, v); Q7: zero unless floor(h) >= 0, floor(h) + 1 < n_row, floor(v) >= 0 and
             floor(v) + 1 < n_col (all four neighbours strictly inside)
    voxel += 0.5 sample (d_so / (s + d_so))^2                                             (Q10: no delta-beta, a constant 0.5)

scale. FDK for a full circle of n_proj equal steps is  mu = (delta_beta / 2) sum_views U^2 q_iso,  U = d_so / (s + d_so),
    delta_beta = 2 pi / n_proj, where q_iso is the weighted row convolved with the FULL ramp kernel (1/(4 tau^2), -1/(j^2 pi^2 tau^2))
    at the pitch the detector has when scaled back to the isocentre, tau_iso = tau d_so / d_sd. The reference differs in three factors:
    the ramp is homogeneous of degree -1 in the pitch (tau r ~ 1/tau) and is applied at detector pitch, which gives d_so / d_sd; the
    kernel is halved, 1/2; the sum carries its 0.5 but no delta_beta, n_proj / (2 pi). So
        reference sum = mu * (d_so / d_sd) * (1/2) * n_proj / (2 pi) = mu * n_proj / (4 pi d_sd / d_so)
    and model / scale is density per mm when the projections are line integrals in mm.
"""
import numpy as np

LIMIT_EPS = 1e-3   # pixels: a ray this close to a validity limit may fall on either side of it in float32


def _geometry(det):
    g = {k: float(getattr(det, k)) for k in ("l_px_row", "l_px_col", "delta_s", "delta_t", "d_so", "d_od")}
    g["n_row"], g["n_col"] = int(det.n_row), int(det.n_col)
    g["d_sd"] = abs(g["d_so"]) + abs(g["d_od"])
    return g


def weight(p, det):
    """p (n_col, n_row) times the cosine weight; a new float64 array."""
    g = _geometry(det)
    h = (np.arange(g["n_row"]) + 0.5) * g["l_px_row"] + g["delta_s"] * g["l_px_row"] - g["n_row"] * g["l_px_row"] / 2
    v = (np.arange(g["n_col"]) + 0.5) * g["l_px_col"] + g["delta_t"] * g["l_px_col"] - g["n_col"] * g["l_px_col"] / 2
    w = g["d_sd"] / np.sqrt(g["d_sd"] ** 2 + h[None, :] ** 2 + v[:, None] ** 2)
    return np.asarray(p, np.float64) * w


def ramp_kernel(n, tau):
    """r[j] for j = -(n - 1) .. n - 1 (index j + n - 1)"""
    tau = float(tau)
    j = np.arange(-(n - 1), n)
    r = np.zeros(2 * n - 1, np.float64)
    odd = j % 2 != 0
    r[odd] = -1.0 / (2.0 * j[odd].astype(np.float64) ** 2 * np.pi ** 2 * tau ** 2)
    r[n - 1] = 1.0 / (8.0 * tau ** 2)
    return r


def ramp(p, tau):
    """Every row of p (rows, n_row) convolved with tau r in the spatial domain; a new float64 array."""
    p = np.asarray(p, np.float64)
    n = p.shape[-1]
    r = float(tau) * ramp_kernel(n, tau)
    x = np.arange(n)
    toeplitz = r[(x[None, :] - x[:, None]) + n - 1]    # [i, x] = tau r[x - i]
    return p @ toeplitz


def backproject(vol, zs, p, det, vol_geo, phi_deg, roi=None, v_offset=0):
    """Adds the view p (n_col, n_row) at phi_deg degrees to vol (len(zs), dim_y, dim_x), float64, whose slice n is slice zs[n] of
    the array the caller means (of that array's x and y extent); roi and v_offset place that array in the grid vol_geo as above.
    Returns (h, v, contribution): the detector coordinates of every voxel's ray and what was added to it, each shaped like vol."""
    g = _geometry(det)
    p = np.asarray(p, np.float64)
    assert p.shape == (g["n_col"], g["n_row"]) and vol.dtype == np.float64 and vol.shape[0] == len(zs)
    x1, y1, z1 = (int(roi.x1), int(roi.y1), int(roi.z1)) if roi is not None else (0, 0, 0)
    _, dy, dx = vol.shape

    def centre(idx, dim, edge):
        return (np.asarray(idx, np.float64) + 0.5) * float(edge) - int(dim) * float(edge) / 2

    x = centre(np.arange(dx) + x1, vol_geo.dim_x, vol_geo.l_vx_x)[None, None, :]
    y = centre(np.arange(dy) + y1, vol_geo.dim_y, vol_geo.l_vx_y)[None, :, None]
    z = centre(np.asarray(zs, np.int64) + z1 + int(v_offset), vol_geo.dim_z, vol_geo.l_vx_z)[:, None, None]
    phi = np.deg2rad(float(phi_deg))
    c, sn = np.cos(phi), np.sin(phi)
    s = x * c + y * sn
    t = -x * sn + y * c
    f = g["d_sd"] / (s + g["d_so"])
    h = (t * f + g["n_row"] * g["l_px_row"] / 2 + g["delta_s"] * g["l_px_row"]) / g["l_px_row"] - 0.5
    v = (z * f + g["n_col"] * g["l_px_col"] / 2 + g["delta_t"] * g["l_px_col"]) / g["l_px_col"] - 0.5
    h, v = np.broadcast_arrays(h, v)
    h0, v0 = np.floor(h), np.floor(v)
    valid = (h0 >= 0) & (h0 + 1 < g["n_row"]) & (v0 >= 0) & (v0 + 1 < g["n_col"])
    i0 = np.where(valid, h0, 0).astype(np.int64)
    j0 = np.where(valid, v0, 0).astype(np.int64)
    a, b = h - h0, v - v0
    sample = (1 - b) * ((1 - a) * p[j0, i0] + a * p[j0, i0 + 1]) + b * ((1 - a) * p[j0 + 1, i0] + a * p[j0 + 1, i0 + 1])
    u = g["d_so"] / (s + g["d_so"])
    add = np.where(valid, 0.5 * sample * u * u, 0.0)
    vol += add
    return np.array(h), np.array(v), add


def near_limit(h, v, det, eps=LIMIT_EPS):
    """True where a ray passes within eps pixels of a limit of the validity rule: h at 0 or n_row - 1, v at 0 or n_col - 1"""
    n_row, n_col = int(det.n_row), int(det.n_col)
    return ((np.abs(h) <= eps) | (np.abs(h - (n_row - 1)) <= eps) | (np.abs(v) <= eps) | (np.abs(v - (n_col - 1)) <= eps))


def scale(det, n_proj):
    """model / scale(det, n_proj) is density per mm for a full circle of n_proj equal steps (derivation above)"""
    g = _geometry(det)
    return n_proj / (4.0 * np.pi * g["d_sd"] / g["d_so"])
