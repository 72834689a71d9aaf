"""The forward projector's statement (include/paris_hip.h paris_hip_forward_project) restated in numpy, and the
test objects of the forward-projection tests. A helper module, not a conftest.

Joseph's method in the backprojector's geometry: one ray per detector pixel from the source to the pixel's centre, one bilinear
sample per voxel plane along the axis (x or y) the ray runs more nearly parallel to. Written from the statement, vectorised over the
detector with a loop over the planes. The two discrete decisions -- the marching axis |dx| >= |dy| and the planes between source
and detector 0 < a <= 1 -- are ALWAYS made in float64 from the float32 arguments, exactly as the statement writes them (ray_setup),
so every dtype marches every ray the same way over the same planes; everything else runs in `dtype`: float64 is the restatement the
device is compared with, float32 is an independent single-precision transcription whose distance from the float64 one says what
fp32 arithmetic costs (FP32_CAL, EDGE_CAL): rounding only, never a plane won or lost at the clip.
"""
import math
import types

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


def ray_setup(det, vg, sin_phi, cos_phi, delta_s_mm, delta_t_mm):
    """What the statement decides once per ray, in float64 from the float32 arguments: t (n_row), z (n_col), dx, dy (n_row), x_march
    (n_row, bool) and a (max(dim_x, dim_y), n_row): a of plane K along the column's own marching axis, NaN beyond that axis' planes.
    a does not depend on the detector row."""
    n_row, n_col = int(det.n_row), int(det.n_col)
    l_r, l_c = f64(det.l_px_row), f64(det.l_px_col)
    d_so = f64(det.d_so)
    d_sd = abs(d_so) + abs(f64(det.d_od))
    s, c = f64(sin_phi), f64(cos_phi)
    t = (np.arange(n_row) + 0.5) * l_r - n_row * l_r / 2 - f64(delta_s_mm)
    z = (np.arange(n_col) + 0.5) * l_c - n_col * l_c / 2 - f64(delta_t_mm)
    dx, dy = d_sd * c - t * s, d_sd * s + t * c
    x_march = np.abs(dx) >= np.abs(dy)
    dims, l_vx = (int(vg.dim_x), int(vg.dim_y)), (f64(vg.l_vx_x), f64(vg.l_vx_y))
    a = np.full((max(dims), n_row), np.nan)
    for axis, (cols, d_p, s_p) in enumerate(((x_march, dx, -d_so * c), (~x_march, dy, -d_so * s))):
        n_p, l_p = dims[axis], l_vx[axis]
        planes = -(n_p * l_p / 2) + l_p / 2 + np.arange(n_p) * l_p
        a[:n_p, cols] = (planes[:, None] - s_p) / d_p[None, cols]
    return types.SimpleNamespace(t=t, z=z, dx=dx, dy=dy, x_march=x_march, a=a)


def clipped(a):
    """of ray_setup's a: the planes the clip 0 < a <= 1 removes (bool, NaN entries False), and the smallest distance of any a from
    0 and from 1"""
    with np.errstate(invalid="ignore"):
        out = (a <= 0) | (a > 1)
    return out, float(np.nanmin(np.minimum(np.abs(a), np.abs(a - 1))))


# Deliberately wrong transcriptions, to show that a test can fail (test_forward_project_host.py): each is one slip the kernel could make
PERTURBATIONS = ("swap_l_p_l_u", "no_clip", "tie_gt")


def forward_project(vol, v_offset, det, vg, sin_phi, cos_phi, delta_s_mm, delta_t_mm, rows=None, dtype=np.float64, v_dim_z=None,
                    perturb=None):
    """One view: p[j, i] for detector rows j in `rows` -- a tuple (first, end) or a list / array of row numbers; default: all -- and every column
    i, as an array of `dtype`.
    vol is the slab (v_dim_z, dim_y, dim_x) whose first slice is global slice v_offset, or a callable (ix, iy, iz) -> values for
    global voxel indices (then v_dim_z says how many slices the slab has). perturb: one of PERTURBATIONS, None for the statement."""
    assert perturb is None or perturb in PERTURBATIONS
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

    # the marching axis and the planes between source and detector, in float64 for every dtype
    setup = ray_setup(det, vg, sin_phi, cos_phi, delta_s_mm, delta_t_mm)
    x_march = setup.x_march if perturb != "tie_gt" else np.abs(setup.dx) > np.abs(setup.dy)
    if perturb == "tie_gt":
        setup = None                                        # a of the other axis for the columns that changed sides: as `dtype` has it

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
        if perturb == "swap_l_p_l_u":
            l_p, l_u = l_u, l_p
        acc = np.zeros((jj.size, cols.size), T)
        for k in range(n_p):
            p_k = -(T(n_p) * l_p / T(2)) + l_p / T(2) + T(k) * l_p
            a = (p_k - src[axis]) / d_p
            a64 = a if setup is None else setup.a[k, cols]
            valid = (a64 > 0) & (a64 <= 1) if perturb != "no_clip" else np.ones(a.shape, bool)
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


# ---- the edge cases (tests/test_gpu_forward_project_edges.py; their fp32 figures: EDGE_CAL in tests/test_forward_project_host.py) ----

EDGE_ANGLES = (0.0, 30.0, 45.0, 90.0, 137.0, 270.0, 315.0)
ANISO = (0.4, 0.55, 0.7)           # voxel sizes [mm] different along every axis: an exchange of two of them shows
# name: detector (n_row, n_col, l_px_row, l_px_col, delta_s, delta_t [pixels], d_so, d_od), grid (dim_x, dim_y, dim_z, l_vx_x, l_vx_y, l_vx_z)
EDGE_CASES = {
    "aniso":           ((48, 40, 1.0, 0.8, 5.0, -2.0, 500.0, 500.0), (40, 52, 36) + ANISO),
    # the source 8.3 mm from the axis inside a box of +-11 x +-10.4 mm, for every view; fan of +-35 degrees, cone of +-25
    "source_inside":   ((48, 40, 2.0, 1.6, 0.5, -0.5, 8.3, 60.0), (40, 52, 36, 0.55, 0.4, 0.7)),
    # the detector plane 4.1 mm behind the axis, through the same box; 24 x 16 mm of detector inside it
    "detector_inside": ((48, 40, 0.5, 0.4, 0.5, -0.5, 60.0, 4.1), (40, 52, 36, 0.55, 0.4, 0.7)),
    # the detector 60 mm to one side and 36 mm up: its nearest column looks 18 mm past the axis, the grid ends at 16.4 + 0.55 mm
    "miss":            ((48, 40, 1.0, 0.8, 60.0, -45.0, 500.0, 500.0), (40, 52, 36) + ANISO),
    "partial_miss":    ((48, 40, 1.0, 0.8, 20.0, -15.0, 500.0, 500.0), (40, 52, 36) + ANISO),
    # power-of-two pixels, offsets of exactly half a pixel, even counts: t == 0.0 at column 24, z == 0.0 at row 20
    "axis_aligned":    ((48, 40, 1.0, 0.5, 0.5, 0.5, 500.0, 500.0), (40, 52, 36) + ANISO),
    # rows reach +-32 mm at 120 mm, +-16 mm at the axis, over a grid of +-9 mm in z: rays cross every slab through its faces
    "thin_slabs":      ((48, 40, 1.0, 1.6, 5.0, -2.0, 60.0, 60.0), (40, 52, 36, 0.55, 0.4, 0.5)),
    # the launch forms: many views on a small detector
    "launch":          ((32, 24, 1.0, 0.8, 5.0, -2.0, 500.0, 500.0), (24, 28, 20) + ANISO),
}
THIN_SLABS = (1, 1, 7, 0)          # slices of the first slabs of the thin_slabs case; the last slab is the rest
_S45 = float(np.float32(0.70710677))
# (sin, cos) of the axis_aligned case: along the axes both ways, and the four exact diagonals, where the column with t == 0 ties
AXIS_SIN_COS = ((0.0, 1.0), (1.0, 0.0), (0.0, -1.0), (-1.0, 0.0), (_S45, _S45), (_S45, -_S45), (-_S45, _S45), (-_S45, -_S45))


def edge_geometry(B, case, **change):
    """the detector and the grid of a named edge case; change: detector fields to replace (d_od=0.0)"""
    d, g = EDGE_CASES[case]
    d = dict(zip(("n_row", "n_col", "l_px_row", "l_px_col", "delta_s", "delta_t", "d_so", "d_od"), d), **change)
    det = B.DetectorGeometry(d["n_row"], d["n_col"], d["l_px_row"], d["l_px_col"], d["delta_s"], d["delta_t"], d["d_so"], d["d_od"], 1.0)
    return det, B.VolumeGeometry(*g)


def grid_volume(vg, seed=7):
    """uniform in [0, 1), float32, (dim_z, dim_y, dim_x): random_volume for a grid that is no cube"""
    return np.random.default_rng(seed + vg.dim_x + vg.dim_y + vg.dim_z).random((vg.dim_z, vg.dim_y, vg.dim_x), dtype=np.float32)


def thin_slab_ranges(dim_z):
    """[(first, end)] of the thin_slabs case's slabs"""
    edges = np.concatenate(([0], np.cumsum(THIN_SLABS), [dim_z]))
    return [(int(a), int(b)) for a, b in zip(edges[:-1], edges[1:])]


def circle(n, first=0.0):
    """n view angles [degrees] evenly over the circle"""
    return tuple(first + 360.0 * k / n for k in range(n))


WIDE_70 = tuple(90.0 + 180.0 * (k % 2) + (k // 2 - 17) * 1.25 for k in range(70))   # 35 within 21.25 degrees of 90, 35 of 270


# ---- seeded random geometries --------------------------------------------------------------------------------------------------

FUZZ_FAMILIES = ("far", "source_inside", "detector_inside", "miss")


def fuzz_case(B, seed):
    """A seeded random forward-projection case: .det, .vg, .slab = (v_offset, v_dim_z), .angles (three, degrees), .vol (the whole
    grid's volume, float32 (dim_z, dim_y, dim_x)), and .family = FUZZ_FAMILIES[seed % 4], .accumulate, .pad (columns of pitch padding).
    Lengths in units of the grid: h = its half extents, R the half diagonal in x / y. Two of the angles are placed so that the fan
    straddles a diagonal (some columns march along x, others along y), the third is anywhere."""
    rng = np.random.default_rng(7000 + seed)
    family = FUZZ_FAMILIES[seed % 4]
    n_row, n_col = int(rng.integers(17, 65)), int(rng.integers(9, 65))
    dims = [int(d) for d in rng.choice(np.arange(9, 65), 3, replace=False)]
    l_vx = [float(np.float32(0.5 * f)) for f in rng.choice(np.linspace(0.6, 1.6, 21), 3, replace=False)]
    h = [0.5 * n * l for n, l in zip(dims, l_vx)]
    R = math.hypot(h[0], h[1])
    u = rng.uniform
    off = [float(u(0.5, 3.0) * rng.choice([-1, 1])) for _ in range(2)]                  # [pixels]
    if family == "source_inside":
        d_so, d_od = u(0.2, 0.8) * min(h[0], h[1]), u(2.0, 6.0) * R
        width, height = 2 * (d_so + d_od) * math.tan(math.radians(u(25, 45))), 2 * (d_so + d_od) * math.tan(math.radians(u(15, 35)))
    else:
        if family == "detector_inside":
            d_so, d_od = u(3.0, 8.0) * R, u(0.1, 0.7) * min(h[0], h[1]) * rng.choice([-1, 1])
        else:
            d_so, d_od = u(3.0, 12.0) * R, u(1.5, 8.0) * R
        mag = (d_so + abs(d_od)) / d_so
        width, height = mag * 2 * R * u(0.6, 1.3), mag * 2 * h[2] * u(0.6, 1.5)
        if family == "miss":
            if (seed // 4) % 2:
                width = mag * 2 * R * u(2.2, 3.0)                                       # a fan much wider than the grid
            else:
                off[0] = float(u(0.4, 0.6) * n_row * rng.choice([-1, 1]))               # or half of it looking past the grid
    det = B.DetectorGeometry(n_row, n_col, width / n_row, height / n_col, off[0], off[1], d_so, d_od, 1.0)
    vg = B.VolumeGeometry(dims[0], dims[1], dims[2], *l_vx)
    # the slab holds the middle slice, which the middle rows see
    first, end = int(rng.integers(0, dims[2] // 2 + 1)), int(rng.integers(dims[2] // 2 + 1, dims[2] + 1))
    ds_mm, _ = offsets_mm(det)
    t = (np.array([0, n_row - 1]) + 0.5) * f64(det.l_px_row) - n_row * f64(det.l_px_row) / 2 - ds_mm
    fan = np.degrees(np.arctan(t / (abs(f64(det.d_so)) + abs(f64(det.d_od)))))          # the columns' directions against the view's
    angles = [float((45.0 + 90.0 * rng.integers(4) - u(fan[0] + 0.1 * (fan[1] - fan[0]), fan[1] - 0.1 * (fan[1] - fan[0]))) % 360.0)
              for _ in range(2)] + [float(u(0.0, 360.0))]
    vol = rng.random((dims[2], dims[1], dims[0]), dtype=np.float32)
    return types.SimpleNamespace(det=det, vg=vg, slab=(first, end - first), angles=tuple(angles), vol=vol, family=family,
                                 accumulate=bool(rng.integers(2)), pad=int(rng.integers(1, 33)))


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
