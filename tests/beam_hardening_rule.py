"""The beam-hardening correction and its fit in numpy (test infrastructure), written from the statement in
include/paris_hip.h and not from the library's code: the pixel rule, Otsu's threshold, the labels, the fixed-order Gram sum and the
least-squares fit. Plus, as forward_model.PERTURBATIONS does for the projector, wrong restatements that a test must tell from the
right one, and the polychromatic two-ellipsoid scan the end-to-end tests use."""
import itertools

import numpy as np

import phantom

L = 65536          # partial sums of the Gram sum
FOLD = 256
DEGREE_MAX = 4
MARGIN_MAX = 4
BINS = 4096
NAN_PAYLOAD = 0x7FC12345


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_pixels(got, want):
    """bit for bit, except that a NaN may carry any payload (the statement leaves it open)"""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(bits(got)[~nan], bits(want)[~nan])


def fmaf(a, b, c):
    """fp32 fused multiply-add, a * b + c rounded once. The product of two floats is exact in double; the sum is rounded to double
    TO ODD (the error of the addition is known exactly from the two-sum), and a round-to-odd result of 53 bits rounds to 24 bits as
    the exact value does."""
    a, b, c = (np.asarray(x, np.float32).astype(np.float64) for x in np.broadcast_arrays(a, b, c))
    with np.errstate(all="ignore"):
        s = a * b
        t = np.array(s + c, np.float64)
        bb = t - s
        e = (s - (t - bb)) + (c - bb)
    inexact = np.isfinite(t) & np.isfinite(e) & (e != 0)
    raw = t.view(np.int64)
    even = (raw & 1) == 0
    towards = np.where((e > 0) == (t > 0), 1, -1)          # the neighbour on the exact value's side, in magnitude steps
    raw[inexact & even] += towards[inexact & even]
    with np.errstate(all="ignore"):
        return t.astype(np.float32)


def apply(c, p, negatives_linear=True):
    """q for every pixel of p; negatives_linear=False is the WRONG rule that applies the higher terms to negative pixels"""
    c = np.asarray(c, np.float32)
    p = np.ascontiguousarray(p, np.float32)
    n = len(c)
    assert 1 <= n <= DEGREE_MAX
    acc = np.full(p.shape, c[n - 1], np.float32)
    for k in range(n - 1, 0, -1):
        acc = fmaf(acc, p, c[k - 1])
    with np.errstate(all="ignore"):
        q = acc * p
        if negatives_linear:
            q = np.where(p < 0, c[0] * p, q)
    return q.astype(np.float32)


def special_pixels(shape, seed=0):
    """line integrals of both signs between 0 and 3 with the values the rule has clauses or roundings for sprinkled in"""
    rng = np.random.default_rng(seed)
    p = (rng.uniform(-0.3, 3.0, shape) * 10.0 ** rng.integers(-3, 1, shape)).astype(np.float32)
    flat = p.reshape(-1)
    special = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, 1e-45, -1e-45, 1e-39, -3e-39, 1.1754944e-38, 3.4e38, -3.4e38, 1.0, -1.0],
                       np.float32)
    at = rng.choice(flat.size, special.size, replace=False)
    flat[at] = special
    flat.view(np.uint32)[at[2]] = NAN_PAYLOAD
    return p


COEFFICIENTS = {1: [1.0], 2: [0.93, 0.11], 3: [1.07, -0.21, 0.083], 4: [0.3, 0.55, -0.17, 0.021]}


# ---- (a) the threshold ------------------------------------------------------------------------------------------------------------

def otsu_bin(hist):
    h = np.asarray(hist, np.uint64)
    total = h.sum(dtype=np.uint64)
    k = np.arange(h.size, dtype=np.uint64)
    c = np.cumsum(h, dtype=np.uint64)
    s = np.cumsum(k * h, dtype=np.uint64)
    valid = (c != 0) & (c != total)
    with np.errstate(all="ignore"):
        w0 = c.astype(np.float64) / np.float64(total)
        mu0 = s.astype(np.float64) / c.astype(np.float64)
        mu1 = (s[-1] - s).astype(np.float64) / (total - c).astype(np.float64)
        d = mu0 - mu1
        score = (w0 * (1.0 - w0)) * (d * d)
    score[~valid] = 0.0
    return int(np.argmax(score)), score            # argmax: the first of equals


def otsu_threshold(hist, h_lo, h_hi):
    b, _ = otsu_bin(hist)
    width = (np.float64(np.float32(h_hi)) - np.float64(np.float32(h_lo))) / np.float64(len(hist))
    return np.float32(np.float64(np.float32(h_lo)) + (np.float64(b) + 1.0) * width)


# ---- (b) the labels ---------------------------------------------------------------------------------------------------------------

def classes(v, thr):
    v = np.asarray(v, np.float32)
    with np.errstate(invalid="ignore"):
        return np.where(np.isfinite(v), np.where(v > np.float32(thr), 2, 1), 0).astype(np.uint8)


def field_of_view(dim_x, dim_y):
    x, y = np.arange(dim_x, dtype=np.int64), np.arange(dim_y, dtype=np.int64)
    r = np.int64(min(dim_x, dim_y) - 2)
    return (2 * x[None, :] - dim_x + 1) ** 2 + (2 * y[:, None] - dim_y + 1) ** 2 <= r * r


def labels(v, thr, margin, margin_z=None):
    """(dim_z, dim_y, dim_x) uint8; margin_z=0 with margin > 0 is the WRONG rule that erodes in x and y only"""
    v = np.asarray(v, np.float32)
    dz, dy, dx = v.shape
    mz = margin if margin_z is None else margin_z
    cls = classes(v, thr)
    padded = np.full((dz + 2 * mz, dy + 2 * margin, dx + 2 * margin), 255, np.uint8)        # outside the slab: differs from every class
    padded[mz:mz + dz, margin:margin + dy, margin:margin + dx] = cls
    same = cls != 0
    for oz, oy, ox in itertools.product(range(2 * mz + 1), range(2 * margin + 1), range(2 * margin + 1)):
        same &= padded[oz:oz + dz, oy:oy + dy, ox:ox + dx] == cls
    return np.where(same & field_of_view(dx, dy)[None, :, :], cls, 0).astype(np.uint8)


# ---- (c) the Gram sum -------------------------------------------------------------------------------------------------------------

def terms(degree):
    return (degree + 1) * (degree + 2) // 2


def gram(basis, lab, blockwise=False):
    """The packed upper triangle and the counts (n_object, n_air, n_ignored, n_not_finite). blockwise=True is the WRONG order that
    gives partial l a contiguous run of voxels instead of i mod L."""
    f = [np.ascontiguousarray(b, np.float32).reshape(-1) for b in basis]
    lab = np.ascontiguousarray(lab, np.uint8).reshape(-1)
    n, deg = lab.size, len(f)
    labelled = (lab == 1) | (lab == 2)
    finite = np.ones(n, bool)
    for fk in f:
        finite &= np.isfinite(fk)
    use = labelled & finite
    counts = (int(np.count_nonzero(use & (lab == 2))), int(np.count_nonzero(use & (lab == 1))), int(np.count_nonzero(~labelled)),
              int(np.count_nonzero(labelled & ~finite)))
    g = [np.where(use, fk, 0).astype(np.float64) for fk in f] + [np.where(use & (lab == 2), 1.0, 0.0)]
    rows = max(1, -(-n // L))
    out = []
    for a in range(deg + 1):
        for b in range(a, deg + 1):
            term = np.zeros(rows * L, np.float64)
            term[:n] = g[a] * g[b]                      # exact: two floats; +0 where the voxel is not summed, which changes no sum
            if blockwise:
                per = term.reshape(L, rows).T           # partial l: voxels l * rows ... l * rows + rows - 1
            else:
                per = term.reshape(rows, L)             # partial l: voxels l, l + L, ...
            acc = np.zeros(L, np.float64)
            for r in range(rows):                       # ascending i within every partial
                acc = acc + per[r]
            fold = acc.reshape(L // FOLD, FOLD)         # fold[m, j] = acc[j + 256 m]
            bj = fold[0].copy()
            for m in range(1, L // FOLD):
                bj = bj + fold[m]
            total = bj[0]
            for j in range(1, FOLD):
                total = total + bj[j]
            out.append(total)
    return np.array(out, np.float64), counts


def gram_matrix(packed, degree):
    n = degree + 1
    m = np.zeros((n, n), np.float64)
    m[np.triu_indices(n)] = packed
    return m + np.triu(m, 1).T


# ---- (d) the fit ------------------------------------------------------------------------------------------------------------------

def normal_equations(packed, degree, n_object):
    """A, b and T of the fit with the fixed template level"""
    g = gram_matrix(packed, degree)
    t = g[0, degree] / np.float64(n_object)
    return g[:degree, :degree], t * g[:degree, degree], t


def residual(packed, degree, counts, c):
    """the rms of sum c_k f_k - T m over the summed voxels, relative to |T|, from the Gram sums alone"""
    a, _, t = normal_equations(packed, degree, counts[0])
    gm = gram_matrix(packed, degree)[:degree, degree]
    c = np.asarray(c, np.float64)
    ss = c @ a @ c - 2.0 * t * (c @ gm) + t * t * counts[0]
    return np.sqrt(max(0.0, ss) / (counts[0] + counts[1])) / abs(t)


# what a test must be able to tell from the rule: name -> a callable with the signature of the right function
PERTURBATIONS = {
    "margin in x and y only": lambda v, thr, margin: labels(v, thr, margin, margin_z=0),
    "blockwise partial sums": lambda basis, lab: gram(basis, lab, blockwise=True),
    "higher terms on negative pixels": lambda c, p: apply(c, p, negatives_linear=False),
}


# ---- the polychromatic scan -------------------------------------------------------------------------------------------------------

TWO_ELLIPSOIDS = [(1, .55, .75, .60, .10, -.05, 0, 20), (1, .18, .18, .30, -.62, .45, .1, 0)]
SPECTRUM = ((0.30, 0.6), (0.06, 0.4))          # (mu per mm, weight) of the two energy bins
MU_MONO = 0.6 * 0.30 + 0.4 * 0.06              # the slope of p at L = 0
SCAN_GEO = (64, 64, 1.0, 1.0, 0.0, 0.0, 500.0, 500.0, 4.0)    # 64 x 64 pixels of 1 mm at 500 / 500 mm, 90 views
SCAN_VIEWS = 90
SCAN_RADIUS = 14.4


def path_lengths(n_views=SCAN_VIEWS, geo=SCAN_GEO, radius=SCAN_RADIUS):
    """the path length through the two ellipsoids of one material, per view: float64-derived float32 (n_col, n_row)"""
    table = phantom.ELLIPSOIDS
    phantom.ELLIPSOIDS = TWO_ELLIPSOIDS
    try:
        return [phantom.projection(geo[0], geo[1], geo[2], geo[3], geo[6], geo[7], i * geo[8], radius) for i in range(n_views)]
    finally:
        phantom.ELLIPSOIDS = table


def polychromatic(lengths):
    out = []
    for ln in lengths:
        ln = ln.astype(np.float64)
        out.append((-np.log(sum(w * np.exp(-mu * ln) for mu, w in SPECTRUM))).astype(np.float32))
    return out


def monochromatic(lengths):
    return [(MU_MONO * ln.astype(np.float64)).astype(np.float32) for ln in lengths]


def spread(volume, mask):
    """std / mean over the masked voxels, in double"""
    x = np.asarray(volume, np.float64)[mask]
    return float(x.std() / x.mean())
