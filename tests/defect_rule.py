"""The defect-map repair rule of include/paris_hip.h restated in numpy float64, and the mask the tests
share. No library call in here: this is what the plan builder and the device are compared against."""
import numpy as np

R_MAX = 8


def shared_mask(dim_x=96, dim_y=80):
    """isolated pixel, corner pixel, 2 x 2 cluster, a dead row, a dead column crossing it, a 5 x 5 block (centre r = 3), a 19 x 19
    block (centre unrepairable), and a defect on row 16 whose sources lie on rows 15 and 17"""
    m = np.zeros((dim_y, dim_x), np.uint8)
    m[5, 7] = 1                 # isolated
    m[0, 0] = 255               # corner (any nonzero byte marks)
    m[dim_y - 1, dim_x - 1] = 1  # the opposite corner
    m[10:12, 20:22] = 1         # 2 x 2
    m[30, :] = 1                # dead row
    m[:, 40] = 1                # dead column crossing it
    m[16, 60] = 1               # on a band edge of the GPU tests
    m[16, 61] = 1
    m[20:25, 50:55] = 1         # 5 x 5: the centre (22, 52) has r = 3
    m[50:69, 60:79] = 1         # 19 x 19: the centre (59, 69) has no good pixel within 8
    return m


def restate(mask):
    """-> (defect[n], first_source[n + 1], source[m], weight64[m], unrepairable[u], reach_rows, reach_cols): linear indices
    y * dim_x + x, repairable defects row-major, each one's sources row-major, weights in float64"""
    bad = np.asarray(mask) != 0
    dim_y, dim_x = bad.shape
    defect, first, source, weight, lost = [], [0], [], [], []
    reach_r = reach_c = 0
    for y, x in zip(*np.nonzero(bad)):   # row-major
        found = None
        for r in range(1, R_MAX + 1):
            y0, y1, x0, x1 = max(0, y - r), min(dim_y, y + r + 1), max(0, x - r), min(dim_x, x + r + 1)
            good = ~bad[y0:y1, x0:x1]
            if good.any():
                sy, sx = np.nonzero(good)   # row-major
                found = (sy + y0, sx + x0)
                break
        if found is None:
            lost.append(y * dim_x + x)
            continue
        sy, sx = found
        d2 = ((sy - y) ** 2 + (sx - x) ** 2).astype(np.float64)
        assert np.all(np.maximum(np.abs(sy - y), np.abs(sx - x)) == r) and len(sy) <= 8 * r
        inv = 1.0 / d2
        weight.extend(inv / inv.sum())
        source.extend(sy * dim_x + sx)
        defect.append(y * dim_x + x)
        first.append(len(source))
        reach_r, reach_c = max(reach_r, int(np.abs(sy - y).max())), max(reach_c, int(np.abs(sx - x).max()))
    return (np.array(defect, np.int64), np.array(first, np.int64), np.array(source, np.int64), np.array(weight, np.float64),
            np.array(lost, np.int64), reach_r, reach_c)


def repair64(frame, plan_defect, plan_first, plan_source, plan_weight):
    """frame (float) with every repairable defect replaced by the float64 sum of weight * source pixel; -> (repaired float64 frame,
    per-defect sum of |w p|, per-defect source count)"""
    f = np.asarray(frame, np.float64)
    out = f.copy().reshape(-1)
    flat = f.reshape(-1)
    w = np.asarray(plan_weight, np.float64)
    mag = np.zeros(len(plan_defect))
    cnt = np.diff(plan_first)
    for k, q in enumerate(plan_defect):
        a, b = plan_first[k], plan_first[k + 1]
        terms = w[a:b] * flat[plan_source[a:b]]
        out[q] = terms.sum()
        mag[k] = np.abs(terms).sum()
    return out.reshape(f.shape), mag, cnt


# ---- the quality case: the 64 x 48 driver geometry, a head phantom over a full circle, a detector with a dead row, a dead column,
#      a 2 x 2 cluster and 0.5 % scattered dead pixels ------------------------------------------------------------------------------

QUALITY_GEO = (64, 48, 0.2, 0.25, 1.5, -0.75, 100, 200, 1.0)
CAL_ZEROED = 0.4305       # relative RMS against the clean reconstruction with the dead pixels left at 0 (oracle, float64 repair)
CAL_REPAIRED = 0.05021   # the same with the dead pixels repaired
BOUND = 1.3               # the pinned bound: this many times the oracle's figure (as tests/test_offset_detector_host.py)


def quality_mask():
    n_row, n_col = QUALITY_GEO[:2]
    m = np.zeros((n_col, n_row), np.uint8)
    m[20, :] = 1
    m[:, 30] = 1
    m[33:35, 44:46] = 1
    rng = np.random.default_rng(11)
    m.reshape(-1)[rng.choice(m.size, m.size // 200, replace=False)] = 1
    return m


def quality_frames(vol_dim_x, l_vx_x):
    """the clean line integrals of the 360 views, float32 (n_col, n_row) each"""
    import phantom
    n_row, n_col, lr, lc, ds, dt, d_so, d_od, step = QUALITY_GEO
    radius = 0.9 * vol_dim_x * l_vx_x / 2
    return [phantom.projection(n_row, n_col, lr, lc, d_so, d_od, float(np.float32(i) * np.float32(step)), radius, ds, dt)
            for i in range(int(360 / step))]


def relative_rms(got, clean):
    got, clean = np.asarray(got, np.float64), np.asarray(clean, np.float64)
    return float(np.sqrt(((got - clean) ** 2).mean()) / np.sqrt((clean ** 2).mean()))
