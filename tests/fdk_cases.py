"""The cases that pin the FDK chain to tests/fdk_model.py and to the phantom's densities, shared by tests/test_fdk_model_host.py (the
oracle against the model, the model against the truth), tests/test_gpu_fdk_model.py (the kernels against the model and the truth)
and tests/golden/make_golden.py (which records the oracle's own error as fdk_model_bounds.json). Numbers and float64 numpy only;
geometry structures come in as a module `G` that has DetectorGeometry, VolumeGeometry, RegionOfInterest and
calculate_volume_geometry (oracle.oracle or paris_amd.backend).

Case V: single views. Two detectors, 61 x 45 and 64 x 48 (rows of whole 16-byte lanes), pitches (0.7, 1.1) mm, offsets (2.25, -1.5)
        pixels, d_so 400, d_od 250; a smooth projection that is non-zero at every edge and asymmetric in both axes; three volumes
        each; nine angles handed over as angle-file values.
Case W: a whole circle. Detector 128 x 96, pitches (0.8, 1.0), offsets (1.5, -0.75), d_so 500, d_od 300, 120 views, the natural
        volume; a phantom of one ball per positive half-axis, each of its own density, so any flip or transpose moves a known value.
Case F: filter only, rows of 97 pixels (61, 64 and 128 come with V and W).
"""
import collections
import functools
import itertools
import json
import os

import numpy as np

import fdk_model as M
import phantom

BOUNDS_FILE = "fdk_model_bounds.json"

V_DETECTORS = {"v61": (61, 45, 0.7, 1.1, 2.25, -1.5, 400.0, 250.0, 1.0),
               "v64": (64, 48, 0.7, 1.1, 2.25, -1.5, 400.0, 250.0, 1.0)}
V_ANGLES = (0.0, 37.0, 45.0, 90.0, 135.5, 180.0, 225.0, 270.0, 301.25)
V_BATCH_ANGLES = (37.0, 135.5, 301.25)          # the three views of the fused launch
V_VOLUMES = ("natural", "overshoot", "roi_slab")
V_NATURAL = {"v61": (65, 65, 75), "v64": (68, 68, 80)}

W_DETECTOR = (128, 96, 0.8, 1.0, 1.5, -0.75, 500.0, 300.0, 3.0)
W_VIEWS = 120
W_NATURAL = (131, 131, 122)
W_RADIUS_FRACTION = 0.40
# (value, a, b, c, x0, y0, z0, rotation): tests/phantom.py's table format
W_ELLIPSOIDS = [(0.1, .8, .8, .8, 0., 0., 0., 0.),
                (1.0, .12, .12, .12, .55, 0., 0., 0.),
                (0.6, .12, .12, .12, 0., .45, 0., 0.),
                (0.3, .12, .12, .12, 0., 0., .35, 0.)]
W_BACKGROUND = 0.1
MEAN_TOL = 0.005        # inner mean of a ball: relative
CENTROID_TOL = 0.1      # voxels, per axis
INNER, OUTER = 0.6, 1.5  # of a ball's radius: where the mean is taken, where the centroid is

F_DETECTOR = (97, 12, 0.7, 1.1, 2.25, -1.5, 400.0, 250.0, 1.0)

BOUNDARY_SHARE = 0.002  # of a volume's voxels may need rule (b)

Placement = collections.namedtuple("Placement", "vol_geo roi v_offset dims")   # dims = (dz, dy, dx) of the array


def v_projection(n_row, n_col):
    i = np.arange(n_row, dtype=np.float64)[None, :]
    j = np.arange(n_col, dtype=np.float64)[:, None]
    p = 1 + 0.5 * np.cos(0.21 * i + 0.4) + 0.3 * np.sin(0.17 * j - 0.3) + 0.01 * i - 0.02 * j + 0.2 * np.cos(0.11 * i + 0.07 * j)
    return p.astype(np.float32)


def v_placement(G, det, name):
    nat = G.calculate_volume_geometry(det)
    if name == "natural":
        return Placement(nat, None, 0, (nat.dim_z, nat.dim_y, nat.dim_x))
    if name == "overshoot":    # three different edges, every axis reaches past the detector's field of view
        l = float(nat.l_vx_x)
        vg = G.VolumeGeometry(70, 57, 66, float(np.float32(l * 1.3)), float(np.float32(l * 1.6)), float(np.float32(l * 1.45)))
        return Placement(vg, None, 0, (66, 57, 70))
    if name == "roi_slab":     # x1, y1, z1 > 0 and a slab that starts 11 slices into the region
        roi = G.RegionOfInterest(7, 52, 5, 48, 6, 60)
        return Placement(nat, roi, 11, (20, 43, 45))
    raise KeyError(name)


def staged_inputs(det, raw):
    """What each stage is fed when it is tested alone: the model's output of the stage before, rounded to float32 -- the same
    numbers for the model, the oracle and the kernels."""
    weighted = M.weight(raw, det).astype(np.float32)
    filtered = M.ramp(weighted, det.l_px_row).astype(np.float32)
    return weighted, filtered


def rel_err(got, want):
    """largest absolute error relative to the largest model magnitude"""
    return float(np.max(np.abs(np.asarray(got, np.float64) - want)) / np.max(np.abs(want)))


class ViewSum:
    """The model's backprojection of some views into one array, with what rule (b) needs: per view, where its ray passes within
    LIMIT_EPS pixels of a validity limit and what it added there."""

    def __init__(self, det, place, frames, angles, zs=None):
        dz, dy, dx = place.dims
        self.zs = list(range(dz)) if zs is None else list(zs)
        self.total = np.zeros((len(self.zs), dy, dx), np.float64)
        self.near, self.added = [], []
        for p, phi in zip(frames, angles):
            h, v, add = M.backproject(self.total, self.zs, p, det, place.vol_geo, phi, place.roi, place.v_offset)
            idx = np.flatnonzero(M.near_limit(h, v, det))
            self.near.append(idx)
            self.added.append(add.ravel()[idx])

    @classmethod
    def merged(cls, parts):
        """the sum of ViewSums over the same array"""
        out = cls.__new__(cls)
        out.zs = parts[0].zs
        out.total = sum(p.total for p in parts)
        out.near = [n for p in parts for n in p.near]
        out.added = [a for p in parts for a in p.added]
        return out

    def compare(self, got):
        """got: the same slices. Returns (error relative to the model's largest magnitude, share of voxels that needed rule (b)): a
        voxel within LIMIT_EPS of a limit in some views may hold the model's value or the value with any of those views' samples
        zeroed."""
        got = np.asarray(got, np.float64)
        assert got.shape == self.total.shape
        err = np.abs(got - self.total).ravel()
        flagged = collections.defaultdict(list)
        for idx, add in zip(self.near, self.added):
            for i, a in zip(idx.tolist(), add.tolist()):
                if a != 0.0:
                    flagged[i].append(a)
        used = 0
        for i, adds in flagged.items():
            best = min(abs(got.ravel()[i] - (self.total.ravel()[i] - sum(sub)))
                       for k in range(1, len(adds) + 1) for sub in itertools.combinations(adds, k))
            if best < err[i]:
                used += 1
                err[i] = best
        return float(err.max() / np.abs(self.total).max()), used / err.size


_v_views = {}


def v_view(G, name, vol, phi):
    """the model's single view of case V, detector `name`, volume `vol`: the projection itself is backprojected; computed once"""
    key = (name, vol, phi)
    if key not in _v_views:
        det = G.DetectorGeometry(*V_DETECTORS[name])
        _v_views[key] = ViewSum(det, v_placement(G, det, vol), [v_projection(det.n_row, det.n_col)], [phi])
    return _v_views[key]


def v_sum(G, name, vol, angles):
    return ViewSum.merged([v_view(G, name, vol, phi) for phi in angles])


# ---- Case W ---------------------------------------------------------------------------------------------------------

def w_radius_mm(vol_geo):
    return W_RADIUS_FRACTION * vol_geo.dim_x * float(vol_geo.l_vx_x)


def w_angle(det, i):
    return i * float(det.delta_phi)


@functools.lru_cache(maxsize=1)
def _w_frames(radius_mm):
    g = W_DETECTOR
    return [phantom.projection(g[0], g[1], g[2], g[3], g[6], g[7], i * g[8], radius_mm, delta_s=g[4], delta_t=g[5],
                               ellipsoids=W_ELLIPSOIDS) for i in range(W_VIEWS)]


def w_frames(vol_geo):
    """the 120 raw float32 views of the phantom"""
    return _w_frames(w_radius_mm(vol_geo))


def w_slices(vol_geo):
    """six z slices: both volume ends, the two about z = 0 (the centres of the x and y balls) and the two about the z ball's centre"""
    zc = W_ELLIPSOIDS[3][6] * w_radius_mm(vol_geo) / float(vol_geo.l_vx_z) + vol_geo.dim_z / 2 - 0.5
    mid = vol_geo.dim_z // 2
    return [0, mid - 1, mid, int(np.floor(zc)), int(np.floor(zc)) + 1, vol_geo.dim_z - 1]


Ball = collections.namedtuple("Ball", "density centre radius lo hi")   # centre, radius in voxels (x, y, z); box [lo, hi) per axis


def w_balls(vol_geo):
    r_mm = w_radius_mm(vol_geo)
    dims = (vol_geo.dim_x, vol_geo.dim_y, vol_geo.dim_z)
    edges = (float(vol_geo.l_vx_x), float(vol_geo.l_vx_y), float(vol_geo.l_vx_z))
    out = []
    for val, a, _, _, x0, y0, z0, _ in W_ELLIPSOIDS[1:]:
        centre = tuple(c * r_mm / e + d / 2 - 0.5 for c, e, d in zip((x0, y0, z0), edges, dims))
        radius = tuple(a * r_mm / e for e in edges)
        lo = tuple(int(np.floor(c - OUTER * r)) - 1 for c, r in zip(centre, radius))
        hi = tuple(int(np.ceil(c + OUTER * r)) + 2 for c, r in zip(centre, radius))
        out.append(Ball(val, centre, radius, lo, hi))
    return out


def truth_figures(boxes, vol_geo):
    """boxes[n]: density per mm in ball n's box, (z, y, x). Per ball: (inner mean, expected mean, centroid error per axis in
    voxels). The centroid is that of the density above the background within OUTER radii of the true centre."""
    out = []
    for ball, box in zip(w_balls(vol_geo), boxes):
        x, y, z = (np.arange(lo, hi, dtype=np.float64) for lo, hi in zip(ball.lo, ball.hi))
        dx, dy, dz = x[None, None, :] - ball.centre[0], y[None, :, None] - ball.centre[1], z[:, None, None] - ball.centre[2]
        rho = np.sqrt((dx / ball.radius[0]) ** 2 + (dy / ball.radius[1]) ** 2 + (dz / ball.radius[2]) ** 2)
        box = np.asarray(box, np.float64)
        assert box.shape == rho.shape
        mean = float(box[rho <= INNER].mean())
        w = np.where(rho <= OUTER, box - W_BACKGROUND, 0.0)
        centroid = tuple(float((w * d).sum() / w.sum()) for d in (dx, dy, dz))
        out.append((mean, ball.density + W_BACKGROUND, centroid))
    return out


def truth_problems(boxes, vol_geo):
    problems = []
    for n, (mean, want, centroid) in enumerate(truth_figures(boxes, vol_geo)):
        if not abs(mean - want) <= MEAN_TOL * want:
            problems.append("ball %d: inner mean %.5f, the phantom's %.5f" % (n, mean, want))
        if not max(abs(c) for c in centroid) <= CENTROID_TOL:
            problems.append("ball %d: centroid off by (%.4f, %.4f, %.4f) voxels" % ((n,) + centroid))
    return problems


def crop(volume, ball):
    return volume[ball.lo[2]:ball.hi[2], ball.lo[1]:ball.hi[1], ball.lo[0]:ball.hi[0]]


class WModel:
    """The float64 chain of case W: the filtered views, the six slices, and the three ball boxes as density per mm."""

    def __init__(self, G):
        self.det = G.DetectorGeometry(*W_DETECTOR)
        self.vol_geo = G.calculate_volume_geometry(self.det)
        vg = self.vol_geo
        assert (vg.dim_x, vg.dim_y, vg.dim_z) == W_NATURAL
        self.raw = w_frames(vg)
        self.filtered = [M.ramp(M.weight(p, self.det), self.det.l_px_row) for p in self.raw]
        self.angles = [w_angle(self.det, i) for i in range(W_VIEWS)]
        self.zs = w_slices(vg)
        self.place = Placement(vg, None, 0, (vg.dim_z, vg.dim_y, vg.dim_x))
        self.scale = M.scale(self.det, W_VIEWS)

    @functools.cached_property
    def slices(self):
        return ViewSum(self.det, self.place, self.filtered, self.angles, self.zs)

    @functools.cached_property
    def staged(self):
        """the filtered views rounded to float32: what the backprojection is fed when it is tested alone"""
        return [f.astype(np.float32) for f in self.filtered]

    @functools.cached_property
    def staged_slices(self):
        return ViewSum(self.det, self.place, self.staged, self.angles, self.zs)

    @functools.cached_property
    def boxes(self):
        out = []
        for ball in w_balls(self.vol_geo):
            roi = collections.namedtuple("Roi", "x1 y1 z1")(*ball.lo)
            box = np.zeros(tuple(h - l for l, h in zip(ball.lo, ball.hi))[::-1], np.float64)
            for p, phi in zip(self.filtered, self.angles):
                M.backproject(box, list(range(box.shape[0])), p, self.det, self.vol_geo, phi, roi)
            out.append(box / self.scale)
        return out


# ---- the recorded error of the reference port -------------------------------------------------------------------------

def load_bounds(golden_dir):
    with open(os.path.join(golden_dir, BOUNDS_FILE)) as f:
        return json.load(f)


def oracle_backproject(O, det, place, frames, angles, zs=None):
    """the oracle's sum of the views, as float32 (dz, dy, dx) or only the slices zs of it"""
    dz, dy, dx = place.dims
    spans = [(0, dz)] if zs is None else [(z, 1) for z in zs]
    out = np.zeros((sum(n for _, n in spans), dy, dx), np.float32)
    for p, phi in zip(frames, angles):
        s, c, ds, dt = O.backproject_constants(det, 0, True, phi)
        at = 0
        for z, n in spans:
            O.backproject(out[at:at + n], np.ascontiguousarray(p, np.float32), place.v_offset + z, det, place.vol_geo, s, c, ds, dt,
                          place.roi)
            at += n
    return out


def oracle_filter(O, det, p):
    fs = O.filter_size(det.n_row)
    return O.apply_filter(np.ascontiguousarray(p, np.float32).copy(), O.make_filter(fs, det.l_px_row), fs)


def _oracle_errors_v(O, name):
    det = O.DetectorGeometry(*V_DETECTORS[name])
    raw = v_projection(det.n_row, det.n_col)      # every stage alone is fed the projection itself
    e = {}
    e["weight"] = (rel_err(O.weight(raw.copy(), det), M.weight(raw, det)), 0.0)
    e["filter"] = (rel_err(oracle_filter(O, det, raw), M.ramp(raw, det.l_px_row)), 0.0)
    chain32 = oracle_filter(O, det, O.weight(raw.copy(), det))
    chain64 = M.ramp(M.weight(raw, det), det.l_px_row)
    e["weight_filter"] = (rel_err(chain32, chain64), 0.0)
    for vol in V_VOLUMES:
        place = v_placement(O, det, vol)
        single, used = 0.0, 0.0
        for phi in V_ANGLES:
            err, share = v_view(O, name, vol, phi).compare(oracle_backproject(O, det, place, [raw], [phi]))
            single, used = max(single, err), max(used, share)
        e["backproject_" + vol] = (single, used)
        e["backproject_sum3_" + vol] = v_sum(O, name, vol, V_BATCH_ANGLES).compare(
            oracle_backproject(O, det, place, [raw] * 3, V_BATCH_ANGLES))
        e["backproject_sum9_" + vol] = v_sum(O, name, vol, V_ANGLES).compare(oracle_backproject(O, det, place, [raw] * 9, V_ANGLES))
    place = v_placement(O, det, "natural")
    e["chain"] = ViewSum(det, place, [chain64] * 9, V_ANGLES).compare(oracle_backproject(O, det, place, [chain32] * 9, V_ANGLES))
    return e


def _oracle_errors_f(O):
    det = O.DetectorGeometry(*F_DETECTOR)
    raw = v_projection(det.n_row, det.n_col)
    return {"filter": (rel_err(oracle_filter(O, det, raw), M.ramp(raw, det.l_px_row)), 0.0),
            "weight_filter": (rel_err(oracle_filter(O, det, O.weight(raw.copy(), det)), M.ramp(M.weight(raw, det), det.l_px_row)), 0.0)}


W_SAMPLED = range(0, W_VIEWS, 8)   # the views whose weight and filter are looked at alone


def _oracle_errors_w(O, w=None):
    w = w or WModel(O)
    e = {"weight": 0.0, "filter": 0.0, "weight_filter": 0.0}
    chain32 = []
    for i, raw in enumerate(w.raw):
        chain32.append(oracle_filter(O, w.det, O.weight(raw.copy(), w.det)))
        if i in W_SAMPLED:
            weighted = staged_inputs(w.det, raw)[0]
            e["weight"] = max(e["weight"], rel_err(O.weight(raw.copy(), w.det), M.weight(raw, w.det)))
            e["filter"] = max(e["filter"], rel_err(oracle_filter(O, w.det, weighted), M.ramp(weighted, w.det.l_px_row)))
            e["weight_filter"] = max(e["weight_filter"], rel_err(chain32[-1], w.filtered[i]))
    e = {k: (v, 0.0) for k, v in e.items()}
    e["backproject"] = w.staged_slices.compare(oracle_backproject(O, w.det, w.place, w.staged, w.angles, w.zs))
    e["chain"] = w.slices.compare(oracle_backproject(O, w.det, w.place, chain32, w.angles, w.zs))
    return e


ORACLE_CASES = {"v61": lambda O: _oracle_errors_v(O, "v61"), "v64": lambda O: _oracle_errors_v(O, "v64"), "f97": _oracle_errors_f,
                "w": _oracle_errors_w}


def oracle_errors(O, case):
    """{stage: (error of the oracle against the model relative to the model's largest magnitude, share of voxels that needed rule
    (b))} of one of ORACLE_CASES -- what make_golden.py records and the host test measures again. In case V every stage alone is fed
    the projection itself; in case W the filter alone is fed the model's weighted view and the backprojection alone the model's
    filtered views, rounded to float32."""
    return ORACLE_CASES[case](O)
