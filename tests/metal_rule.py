"""Linear-interpolation metal artefact reduction in numpy (test infrastructure), written from the statement in
include/paris_hip.h and not from the library's code: the ordered list of the metal voxels, the packed trace with its grow window, the
run-wise inpainting in fp32 with an explicit fused multiply-add, the reinsertion and the counts. Plus, as forward_model.PERTURBATIONS
does for the projector, wrong restatements that a test must tell from the right one, the special rows both test files use, and the
float64 scene of the physical check."""
import numpy as np

import fdk_model
import forward_model
import phantom
from beam_hardening_rule import bits as f32_bits, fmaf, same_pixels  # noqa: F401 - same_pixels is for the tests

GROW_MAX = 4
MIN_VOXELS_CAP = 1024
NAN_PAYLOAD = 0x7FC12345
COUNTER_BYTES = 64          # the counters at the head of a trace setting


def words(dim_x):
    return (dim_x + 63) // 64


def voxel_cap(dim_x, dim_y, dim_z):
    return max(MIN_VOXELS_CAP, dim_x * dim_y * dim_z // 32)


def collect(v, threshold):
    """(index uint64[n], value float32[n]) of the voxels above the threshold, in ascending linear index; a NaN compares false"""
    flat = np.ascontiguousarray(v, np.float32).ravel()
    with np.errstate(invalid="ignore"):
        index = np.flatnonzero(flat > np.float32(threshold))
    return index.astype(np.uint64), flat[index].copy()


def binarized(v, threshold):
    with np.errstate(invalid="ignore"):
        return (np.asarray(v, np.float32) > np.float32(threshold)).astype(np.float32)


# Deliberately wrong restatements, each one slip an implementation could make
WRONG_PACK = ("grow along rows only",)
WRONG_INPAINT = ("t from b - a + 1", "anchors inside the run", "edge run interpolated towards 0")


def trace(t, min_path, grow, wrong=None):
    """bool (n_frames, dim_y, dim_x): the pixels of the trace of the frames t (n_frames, dim_y, dim_x)"""
    assert wrong is None or wrong in WRONG_PACK
    a = np.asarray(t, np.float32)
    with np.errstate(invalid="ignore"):
        hit = a > np.float32(min_path)
    n, dy, dx = hit.shape
    out = np.zeros_like(hit)
    reach_y = 0 if wrong == "grow along rows only" else grow
    for sy in range(-reach_y, reach_y + 1):
        for sx in range(-grow, grow + 1):
            # out[y, x] |= hit[y + sy, x + sx], the window clipped to the frame
            y0, y1 = max(0, -sy), min(dy, dy - sy)
            x0, x1 = max(0, -sx), min(dx, dx - sx)
            if y0 < y1 and x0 < x1:
                out[:, y0:y1, x0:x1] |= hit[:, y0 + sy:y1 + sy, x0 + sx:x1 + sx]
    return out


def pack_bits(mask):
    """a bool array (..., dim_x) as uint64 (..., words): pixel x is bit x & 63 of word x >> 6, the bits beyond dim_x are 0"""
    m = np.asarray(mask, bool)
    dx = m.shape[-1]
    padded = np.zeros(m.shape[:-1] + (words(dx) * 64,), np.uint8)
    padded[..., :dx] = m
    b = padded.reshape(m.shape[:-1] + (words(dx), 64)).astype(np.uint64)
    return (b << np.arange(64, dtype=np.uint64)).sum(axis=-1, dtype=np.uint64)


def unpack_bits(bits, dim_x):
    b = np.asarray(bits, np.uint64)
    m = (b[..., :, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)
    return m.reshape(b.shape[:-1] + (b.shape[-1] * 64,))[..., :dim_x].astype(bool)


def pack(t, min_path, grow, wrong=None):
    return pack_bits(trace(t, min_path, grow, wrong))


def runs_of(row_mask):
    """the maximal runs [a, b] of set pixels of one row"""
    m = np.concatenate(([False], np.asarray(row_mask, bool), [False]))
    d = np.diff(m.astype(np.int8))
    return list(zip(np.flatnonzero(d == 1), np.flatnonzero(d == -1) - 1))


def inpaint(p, mask, row_first=0, row_count=None, wrong=None):
    """(the inpainted float32 copy of the frame p (dim_y, dim_x), (replaced, runs, rows_left)) for the bool trace `mask` of its shape"""
    assert wrong is None or wrong in WRONG_INPAINT
    out = np.array(p, np.float32)
    dy, dx = out.shape
    count = dy - row_first if row_count is None else row_count
    replaced = n_runs = rows_left = 0
    f32 = np.float32
    with np.errstate(all="ignore"):
        for y in range(row_first, row_first + count):
            row = out[y]
            for a, b in runs_of(mask[y]):
                if a == 0 and b == dx - 1:
                    rows_left += 1
                    continue
                n_runs += 1
                replaced += b - a + 1
                x = np.arange(a, b + 1)
                if a == 0 or b == dx - 1:
                    anchor = row[b + 1] if a == 0 else row[a - 1]
                    if wrong == "edge run interpolated towards 0":
                        t = ((x + 1) if a == 0 else (dx - x)).astype(f32) / f32(b - a + 2)
                        row[a:b + 1] = fmaf(t, anchor, f32(0))
                    else:
                        row[a:b + 1] = anchor
                    continue
                pl, pr = (row[a], row[b]) if wrong == "anchors inside the run" else (row[a - 1], row[b + 1])
                t = (x - (a - 1)).astype(f32) / f32(b - a + (1 if wrong == "t from b - a + 1" else 2))
                row[a:b + 1] = fmaf(t, f32(pr - pl), pl)
    return out, (replaced, n_runs, rows_left)


def reinsert(v, index, value, v_offset=0):
    """the slab v (v_dim_z, dim_y, dim_x), first slice v_offset of its grid, with the listed voxels that fall into it set"""
    out = np.array(v, np.float32)
    plane = out.shape[1] * out.shape[2]
    i = np.asarray(index, np.int64) - v_offset * plane
    ok = (i >= 0) & (i < out.size)
    out.reshape(-1)[i[ok]] = np.asarray(value, np.float32)[ok]
    return out


def counts_tuple(st):
    return (int(st.replaced), int(st.runs), int(st.rows_left))


# ---- special rows ----------------------------------------------------------------------------------------------------------------

DIM_XS = (1, 5, 61, 64, 65, 130)


def special_rows(dim_x, seed=0):
    """(p float32 (rows, dim_x), mask bool (rows, dim_x)): one row per case the rule distinguishes that fits into dim_x pixels --
    single pixels, runs that end at bit 63 and start at bit 64, a run longer than 128, runs at either edge and at both, a row covered
    whole, an empty row, two runs one good pixel apart, NaN and +-inf anchors, a NaN inside a run"""
    rng = np.random.default_rng(seed + dim_x)
    cases = []

    def add(runs, edit=None):
        m = np.zeros(dim_x, bool)
        for a, b in runs:
            if 0 <= a <= b < dim_x:
                m[a:b + 1] = True
        p = (rng.random(dim_x, dtype=np.float32) * np.float32(6.0) - np.float32(1.0))
        if edit is not None:
            edit(p)
        cases.append((p, m))

    def put(where, what):
        def edit(p):
            for x, v in zip(where, what):
                if 0 <= x < dim_x:
                    p[x] = v
        return edit

    nan = np.array([NAN_PAYLOAD], np.uint32).view(np.float32)[0]
    add([])
    add([(0, dim_x - 1)])                                   # covered whole
    add([(dim_x // 2, dim_x // 2)])                         # one pixel
    add([(1, 1), (3, 3)])                                   # two runs one good pixel apart
    add([(0, 0)])
    add([(dim_x - 1, dim_x - 1)])
    add([(0, 1), (dim_x - 2, dim_x - 1)])                   # both edges
    add([(0, dim_x - 2)])                                   # everything but the last pixel
    add([(1, dim_x - 1)])                                   # everything but the first
    add([(1, dim_x - 2)])                                   # one interior run between the edge pixels
    add([(60, 63)])                                         # ends at bit 63
    add([(64, 66)])                                         # starts at bit 64
    add([(62, 65)])                                         # across the word boundary
    add([(1, 128)])                                         # longer than 128: two whole words inside
    add([(63, 63), (65, 127)])
    add([(2, 4)], put((1,), (nan,)))                        # NaN anchor on the left
    add([(2, 4)], put((5,), (nan,)))
    add([(2, 4)], put((1,), (np.inf,)))
    add([(2, 4)], put((5,), (-np.inf,)))
    add([(2, 4)], put((1, 5), (np.inf, np.inf)))            # inf - inf
    add([(2, 4)], put((1, 5), (np.float32(3e38), np.float32(-3e38))))   # the difference overflows
    add([(2, 4)], put((3,), (nan,)))                        # a NaN inside the run goes away
    add([(0, 2)], put((3,), (nan,)))                        # an edge run copies a NaN anchor
    return np.stack([c[0] for c in cases]), np.stack([c[1] for c in cases])


def corner_frames(dim_x=70, dim_y=9):
    """(n, dim_y, dim_x) float32 frames for the grow window: a hit in every corner, at the word boundary, a NaN, an inf, values at and
    just above the threshold 1.0"""
    t = np.zeros((4, dim_y, dim_x), np.float32)

    def put(f, y, x, value):                                             # (clamped into a small frame)
        t[f, min(y, dim_y - 1), min(x, dim_x - 1)] = value

    for y, x in ((0, 0), (0, dim_x - 1), (dim_y - 1, 0), (dim_y - 1, dim_x - 1)):
        put(0, y, x, 2.0)
    put(1, dim_y // 2, 63, 2.0)
    put(1, 1, 64, 2.0)
    put(2, 6, 7, 1.0)                                                    # at the threshold: not in
    put(2, 6, 20, np.nextafter(np.float32(1.0), np.float32(2.0)))
    put(2, 4, 5, np.inf)
    put(2, 2, 2, np.nan)
    t[3] = np.random.default_rng(3).random((dim_y, dim_x), dtype=np.float32) * np.float32(1.05)
    return t


def hit_volume(shape, threshold, seed=0, chunk=4096):
    """float32 (dim_z, dim_y, dim_x) with a cluster of hits across every multiple of `chunk` voxels, isolated hits, NaN and +-inf"""
    rng = np.random.default_rng(seed)
    v = (rng.random(shape, dtype=np.float32) * np.float32(threshold)).astype(np.float32)   # all below or at the threshold
    flat = v.reshape(-1)
    n = flat.size
    for edge in list(range(chunk, n, chunk))[:64] + [64, 63]:
        lo, hi = max(0, min(n, edge - 3)), min(n, edge + 4)
        flat[lo:hi] = np.float32(threshold) + rng.random(hi - lo, dtype=np.float32) + np.float32(0.5)
    some = rng.choice(n, size=min(n, 40), replace=False)
    flat[some] = np.float32(threshold) + np.float32(1.0) + rng.random(some.size, dtype=np.float32)
    flat[0] = np.nan
    flat[n - 1] = np.inf
    flat[n // 2] = -np.inf
    flat[n // 3] = np.float32(threshold)                                 # at the threshold: not a hit
    return v


# ---- the scene of the physical check ---------------------------------------------------------------------------------------------

SCENE_DET = (64, 32, 1.0, 1.0, 0.0, 0.0, 500.0, 500.0, 3.0)            # 64 x 32 pixels of 1 mm at 500 / 500 mm, views 3 degrees apart
SCENE_VIEWS = 120
SCENE_GRID = (64, 64, 24, 0.5, 0.5, 0.5)
SCENE_RADIUS = 12.0
SCENE_ELLIPSOIDS = [(0.02, 1, 1, .45, 0, 0, 0, 0), (2.0, .125, .125, .125, .5, 0, 0, 0), (2.0, .125, .125, .125, -.5, .1, 0, 0)]
SCENE_MIN_PATH = 0.25
SCENE_GROW = 1
SCENE_CASES = ((3.0, 0.3), (2.0, 0.25))                                  # (clip of the line integrals, threshold on density per mm)
SCENE_BOUND = 0.25                                                       # soft-tissue RMS error after / before


def scene_frames(clip=None):
    """the scene's line integrals, float32 (views, n_col, n_row); clip: the detector's floor as a largest line integral"""
    n_row, n_col, l_r, l_c, _, _, d_so, d_od, step = SCENE_DET
    p = np.stack([phantom.projection(n_row, n_col, l_r, l_c, d_so, d_od, i * step, SCENE_RADIUS, ellipsoids=SCENE_ELLIPSOIDS)
                  for i in range(SCENE_VIEWS)])
    return p if clip is None else np.minimum(p, np.float32(clip))


def scene_truth(vg):
    """the phantom's density at the voxel centres of the grid, float64 (dim_z, dim_y, dim_x)"""
    def centres(n, edge):
        return (np.arange(int(n)) + 0.5) * float(edge) - int(n) * float(edge) / 2
    return phantom.density(centres(vg.dim_x, vg.l_vx_x)[None, None, :], centres(vg.dim_y, vg.l_vx_y)[None, :, None],
                           centres(vg.dim_z, vg.l_vx_z)[:, None, None], SCENE_RADIUS, SCENE_ELLIPSOIDS)


def soft_tissue(truth, index):
    """bool mask of truth's shape: truth below 1 and above 0.01, and not within 2 voxels in x or y of a collected voxel"""
    metal = np.zeros(truth.shape, bool)
    metal.reshape(-1)[np.asarray(index, np.int64)] = True
    near = np.zeros_like(metal)
    dy, dx = truth.shape[1:]
    for sy in range(-2, 3):
        for sx in range(-2, 3):
            y0, y1, x0, x1 = max(0, -sy), min(dy, dy - sy), max(0, -sx), min(dx, dx - sx)
            near[:, y0:y1, x0:x1] |= metal[:, y0 + sy:y1 + sy, x0 + sx:x1 + sx]
    return (truth < 1.0) & (truth > 0.01) & ~near


def rms_error(volume, truth, where):
    return float(np.sqrt(np.mean((np.asarray(volume, np.float64)[where] - truth[where]) ** 2)))


def reconstruct64(frames, det, vg):
    """fdk_model's chain on every view, in density per mm, float64"""
    vol = np.zeros((int(vg.dim_z), int(vg.dim_y), int(vg.dim_x)), np.float64)
    zs = np.arange(int(vg.dim_z))
    for i, p in enumerate(frames):
        q = fdk_model.ramp(fdk_model.weight(p, det), det.l_px_row)
        fdk_model.backproject(vol, zs, q, det, vg, i * float(det.delta_phi))
    return vol / fdk_model.scale(det, len(frames))


def reduce64(frames, det, vg, threshold, min_path=SCENE_MIN_PATH, grow=SCENE_GROW):
    """The whole remedy on the float64 model: (first volume, final volume, index, trace bool (views, n_col, n_row)), volumes in density
    per mm"""
    first = reconstruct64(frames, det, vg)
    index, value = collect(first, threshold)
    mask = binarized(first, threshold).astype(np.float64)
    shadow = np.stack([forward_model.forward_project(mask, 0, det, vg, *forward_model.view_sin_cos(i * float(det.delta_phi)), 0.0, 0.0)
                       for i in range(len(frames))])
    tr = trace(shadow, min_path, grow)
    painted = np.stack([inpaint(p, m)[0] for p, m in zip(frames, tr)])
    final = reinsert(reconstruct64(painted, det, vg), index, value)
    return first, final, index, tr
