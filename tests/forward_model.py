"""The forward projector's statement (include/paris_hip.h paris_hip_forward_project) restated in numpy, and the
test objects of the forward-projection tests. A helper module, not a conftest.

Joseph's method in the backprojector's geometry: one ray per detector pixel from the source to the pixel's centre, one bilinear
sample per voxel plane along the axis (x or y) the ray runs more nearly parallel to. Written from the statement, vectorised over the
detector with a loop over the planes. The choice of the marching axis is ALWAYS made in float64 from the float32 arguments, exactly
as the statement writes it, so every dtype marches every ray the same way; everything else runs in `dtype`: float64 is the
restatement the device is compared with, float32 is an independent single-precision transcription whose distance from the float64
one says what fp32 arithmetic costs (FP32_CAL).
"""
import math

import numpy as np


def f64(x):
    return float(np.float32(x))


def view_sin_cos(phi_deg):
    """sin / cos of an angle in degrees as paris_hip_stage_angle forms them: fp32 radians, fp32 results"""
    a = np.float32(phi_deg) * (np.float32(math.pi) / np.float32(180.0))
    return float(np.float32(math.sin(a))), float(np.float32(math.cos(a)))


def offsets_mm(det):
    """delta_s l_px_row and delta_t l_px_col in fp32, as paris_hip_stage_backproject derives them"""
    return (float(np.float32(det.delta_s) * np.float32(det.l_px_row)), float(np.float32(det.delta_t) * np.float32(det.l_px_col)))


def _taps(vol, v_offset, v_dim_z):
    """tap(ix, iy, iz) -> values (float64) of the voxels at global indices, all inside the grid and the slab"""
    if callable(vol):
        return vol
    return lambda ix, iy, iz: vol[iz - v_offset, iy, ix]


def forward_project(vol, v_offset, det, vg, sin_phi, cos_phi, delta_s_mm, delta_t_mm, rows=None, dtype=np.float64, v_dim_z=None):
    """One view: p[j, i] for detector rows j in `rows` -- a tuple (first, end) or a list / array of row numbers; default: all -- and every column
    i, as an array of `dtype`.
    vol is the slab (v_dim_z, dim_y, dim_x) whose first slice is global slice v_offset, or a callable (ix, iy, iz) -> values for
    global voxel indices (then v_dim_z says how many slices the slab has)."""
    T = dtype
    n_row, n_col = int(det.n_row), int(det.n_col)
    dim = (int(vg.dim_x), int(vg.dim_y), int(vg.dim_z))
    l_vx = (f64(vg.l_vx_x), f64(vg.l_vx_y), f64(vg.l_vx_z))
    if v_dim_z is None:
        v_dim_z = vol.shape[0]
    tap = _taps(vol, v_offset, v_dim_z)
    l_r, l_c = f64(det.l_px_row), f64(det.l_px_col)
    d_so = f64(det.d_so)
    d_sd = abs(d_so) + abs(f64(det.d_od))
    s, c, ds, dt = f64(sin_phi), f64(cos_phi), f64(delta_s_mm), f64(delta_t_mm)
    jj = np.arange(n_col) if rows is None else (np.arange(*rows) if isinstance(rows, tuple) else np.asarray(rows, np.int64))

    # the marching axis, in float64 for every dtype
    t64 = (np.arange(n_row) + 0.5) * l_r - n_row * l_r / 2 - ds
    x_march = np.abs(d_sd * c - t64 * s) >= np.abs(d_sd * s + t64 * c)

    t = (np.arange(n_row, dtype=T) + T(0.5)) * T(l_r) - T(n_row) * T(l_r) / T(2) - T(ds)
    z = (jj.astype(T) + T(0.5)) * T(l_c) - T(n_col) * T(l_c) / T(2) - T(dt)
    src = (T(-d_so) * T(c), T(-d_so) * T(s))
    dirs = (T(d_sd) * T(c) - t * T(s), T(d_sd) * T(s) + t * T(c))
    out = np.zeros((jj.size, n_row), T)
    for axis in (0, 1):                                     # 0: x-marching, 1: y-marching (x and y exchanged)
        cols = np.nonzero(x_march if axis == 0 else ~x_march)[0]
        if cols.size == 0:
            continue
        other = 1 - axis
        d_p, d_u = dirs[axis][cols], dirs[other][cols]
        dz = z[:, None]
        n_p, n_u, n_z = dim[axis], dim[other], dim[2]
        l_p, l_u, l_z = T(l_vx[axis]), T(l_vx[other]), T(l_vx[2])
        acc = np.zeros((jj.size, cols.size), T)
        for k in range(n_p):
            p_k = -(T(n_p) * l_p / T(2)) + l_p / T(2) + T(k) * l_p
            a = (p_k - src[axis]) / d_p
            valid = (a > 0) & (a <= 1)
            if not valid.any():
                continue
            u = src[other] + a * d_u
            w = a[None, :] * dz
            fu = (u + T(n_u) * l_u / T(2)) / l_u - T(0.5)
            fz = (w + T(n_z) * l_z / T(2)) / l_z - T(0.5)
            iu, iz = np.floor(fu), np.floor(fz)
            wu, wz = (fu - iu)[None, :], fz - iz
            iu, iz = iu.astype(np.int64)[None, :], iz.astype(np.int64)
            sample = np.zeros_like(acc)
            for du, dzz, wt in ((0, 0, (T(1) - wu) * (T(1) - wz)), (1, 0, wu * (T(1) - wz)), (0, 1, (T(1) - wu) * wz), (1, 1, wu * wz)):
                ju, jz = np.broadcast_to(iu + du, acc.shape), iz + dzz
                ok = (ju >= 0) & (ju < n_u) & (jz >= v_offset) & (jz < v_offset + v_dim_z) & (jz < n_z) & valid[None, :]
                if not ok.any():
                    continue
                ju, jz = ju[ok], jz[ok]
                kk = np.full(ju.shape, k, np.int64)
                vals = tap(kk, ju, jz) if axis == 0 else tap(ju, kk, jz)
                sample[ok] += wt[ok] * np.asarray(vals).astype(T)
            acc += sample
        length = np.sqrt(dirs[0][cols] ** 2 + dirs[1][cols] ** 2 + dz ** 2) / np.abs(d_p)
        out[:, cols] = acc * l_p * length
    return out


# ---- test objects --------------------------------------------------------------------------------------------------------------

def geometry(B, n, n_col=None, scale=1.0):
    """The forward-projection tests' configuration at n detector columns: 1.25 : 1 pixels (1.0 x 0.8 mm times scale), n_col rows
    (default 5 n / 4), offsets (5, -2) pixels, 500 / 500 mm, and a grid of n^3 voxels of half the column width"""
    det = B.DetectorGeometry(n, 5 * n // 4 if n_col is None else n_col, 1.0 * scale, 0.8 * scale, 5.0, -2.0, 500, 500, 1.0)
    return det, B.VolumeGeometry(n, n, n, 0.5 * scale, 0.5 * scale, 0.5 * scale)


def random_volume(n, seed=7):
    """uniform in [0, 1), float32, (n, n, n)"""
    return np.random.default_rng(seed + n).random((n, n, n), dtype=np.float32)


# three off-centre isotropic Gaussian blobs: (amplitude, centre / R, sigma / R), R = BLOB_RADIUS_MM
BLOBS = ((1.0, (0.30, -0.25, 0.20), 0.10), (-0.6, (-0.35, 0.30, -0.30), 0.08), (0.8, (0.05, 0.10, 0.05), 0.16))
BLOB_N = 128                       # detector columns of the blob configuration
BLOB_GRID = (96, 104, 88)          # its grid: different along every axis, so an exchange of axes shows
BLOB_RADIUS_MM = 25.6              # 0.2 n l_px_row; sigma = 2.56, 2.05 and 4.10 mm = 5.1, 4.1 and 8.2 voxels of 0.5 mm


def blob_geometry(B):
    det, _ = geometry(B, BLOB_N)
    return det, B.VolumeGeometry(BLOB_GRID[0], BLOB_GRID[1], BLOB_GRID[2], 0.5, 0.5, 0.5)


def voxel_centres(vg):
    """world coordinates [mm] of the voxel centres along x, y, z (vol_centered_coordinate)"""
    return [-(n * f64(l) / 2) + f64(l) / 2 + np.arange(n) * f64(l)
            for n, l in ((vg.dim_x, vg.l_vx_x), (vg.dim_y, vg.l_vx_y), (vg.dim_z, vg.l_vx_z))]


def blob_volume(vg):
    """the blobs sampled at the voxel centres, float32 (dim_z, dim_y, dim_x)"""
    x, y, z = voxel_centres(vg)
    v = np.zeros((vg.dim_z, vg.dim_y, vg.dim_x))
    for amp, ctr, sig in BLOBS:
        bx, by, bz = (q * BLOB_RADIUS_MM for q in ctr)
        r2 = (x[None, None, :] - bx) ** 2 + (y[None, :, None] - by) ** 2 + (z[:, None, None] - bz) ** 2
        v += amp * np.exp(-r2 / (2 * (sig * BLOB_RADIUS_MM) ** 2))
    return v.astype(np.float32)


def blob_line_integrals(det, sin_phi, cos_phi, delta_s_mm, delta_t_mm):
    """analytic line integrals of the blobs along the rays of one view: A sigma sqrt(2 pi) exp(-d^2 / 2 sigma^2), d the distance
    from the blob's centre to the ray; float64 (n_col, n_row)"""
    n_row, n_col = det.n_row, det.n_col
    d_so = f64(det.d_so)
    d_sd = abs(d_so) + abs(f64(det.d_od))
    s, c = f64(sin_phi), f64(cos_phi)
    t = (np.arange(n_row) + 0.5) * f64(det.l_px_row) - n_row * f64(det.l_px_row) / 2 - f64(delta_s_mm)
    z = (np.arange(n_col) + 0.5) * f64(det.l_px_col) - n_col * f64(det.l_px_col) / 2 - f64(delta_t_mm)
    d = np.stack(np.broadcast_arrays((d_sd * c - t * s)[None, :], (d_sd * s + t * c)[None, :], z[:, None]), -1)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    src = np.array([-d_so * c, -d_so * s, 0.0])
    out = np.zeros((n_col, n_row))
    for amp, ctr, sig in BLOBS:
        rel = np.array(ctr) * BLOB_RADIUS_MM - src
        dist2 = rel @ rel - (d @ rel) ** 2
        sg = sig * BLOB_RADIUS_MM
        out += amp * sg * math.sqrt(2 * math.pi) * np.exp(-dist2 / (2 * sg * sg))
    return out


# a closed form of the voxel index for volumes no host holds: a small table with periods 61, 67 and 71 along x, y and z times a
# slow ramp that differs between the two halves of the address space (a wrapped 32-bit index reads another value)
_TAB = [np.random.default_rng(p).random(p) for p in (61, 67, 71)]


def closed_form_tap(dim_x, dim_y, dim_z):
    half = dim_z // 2

    def tap(ix, iy, iz):
        ramp = np.where(iz < half, 0.5 + iz / (2.0 * dim_z), 1.5 - iz / (2.0 * dim_z))
        return ((_TAB[0][ix % 61] + _TAB[1][iy % 67] + _TAB[2][iz % 71]) * ramp).astype(np.float32).astype(np.float64)
    return tap


def closed_form_fill(torch, out):
    """fills the device tensor out (dim_z, dim_y, dim_x), float32, with closed_form_tap's values, slice by slice"""
    dim_z, dim_y, dim_x = out.shape
    dev = out.device
    tx = torch.tensor(_TAB[0], dtype=torch.float64, device=dev)[torch.arange(dim_x, device=dev) % 61]
    ty = torch.tensor(_TAB[1], dtype=torch.float64, device=dev)[torch.arange(dim_y, device=dev) % 67]
    plane = tx[None, :] + ty[:, None]
    half = dim_z // 2
    for z in range(dim_z):
        ramp = 0.5 + z / (2.0 * dim_z) if z < half else 1.5 - z / (2.0 * dim_z)
        out[z] = ((plane + float(_TAB[2][z % 71])) * ramp).to(torch.float32)
