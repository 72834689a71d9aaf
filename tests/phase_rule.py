"""Single-distance phase retrieval (Paganin), restated in numpy from the statement in include/paris_hip.h:
retrieve64 is the rule in float64 with np.fft.fft2, retrieve32 the same rule with an explicit radix-2 transform whose every operation
is rounded to fp32 -- the independent fp32 yardstick the device's error is measured against. `wrong` selects a plausible misreading
of the statement; the tests show that each one is told apart. A helper, not a test."""
import numpy as np

import metal_rule
import phantom

SIZE_MAX = 8192
MARGIN_MAX = 1024
WRONG = ("wrap_floor", "f_from_dim", "laplacian", "floor_first", "pitches_swapped")

# (dim_x, dim_y, margin, n_x, n_y, l_x, l_y): the shapes of the host and the device tests
SHAPES = [(5, 3, 1, 8, 8, 1.0, 1.0),            # the minimum size
          (1, 1, 1, 8, 8, 1.0, 1.0),            # a constant frame
          (61, 45, 8, 128, 64, 0.7, 1.1),       # N_x != N_y, anisotropic pitches
          (64, 64, 1, 128, 128, 1.0, 1.0),      # a power-of-two frame still pads
          (130, 9, 12, 256, 64, 0.5, 0.5),      # few rows, an odd row count for the row pairs
          (67, 45, 8, 128, 64, 1.0, 0.8),       # ragged row tails
          (1000, 700, 24, 2048, 1024, 0.2, 0.2),  # the large case: 1024 threads, 8 columns of 1024 in 64 KiB of LDS (16 up to N_y = 512)
          (9, 1100, 1, 16, 2048, 1.0, 1.0),     # the column pass holds 4 columns of N_y = 2048 ...
          (6, 2100, 2, 16, 4096, 1.0, 1.0),     # ... 2 of 4096 ...
          (5, 4100, 1, 8, 8192, 1.0, 1.0),      # ... and 1 of 8192, the largest size
          (4100, 3, 1, 8192, 8, 1.0, 1.0)]      # the longest row


def padded(dim, margin):
    n = 8
    while n < max(8, dim + 2 * margin):
        n *= 2
    return n


def source(dim, n, wrong=None):
    """which of the dim samples each of the n padded samples reads"""
    s = np.arange(n)
    split = (n - dim) // 2 if wrong == "wrap_floor" else (n - dim + 1) // 2
    return np.where(s < dim, s, np.where(s - dim < split, dim - 1, 0))


def extend(t, n_x, n_y, wrong=None):
    dim_y, dim_x = t.shape
    return t[source(dim_y, n_y, wrong)][:, source(dim_x, n_x, wrong)]


def table(alpha, n, pitch, dim=None, wrong=None):
    """a[k] = alpha f^2 in float64, rounded once to float32"""
    k = np.arange(n, dtype=np.float64)
    k = np.where(k <= n // 2, k, k - n)
    if wrong == "laplacian":
        f2 = (2.0 - 2.0 * np.cos(2.0 * np.pi * k / n)) / (2.0 * np.pi * float(pitch)) ** 2
    else:
        f2 = (k / ((dim if wrong == "f_from_dim" else n) * float(pitch))) ** 2
    return (float(np.float32(alpha)) * f2).astype(np.float32)


def transfer(alpha, n_x, n_y, l_x, l_y, dtype=np.float64, dims=None, wrong=None):
    """H (n_y, n_x) from the two float32 tables: in float64, or in fp32 as (1 + a_x) + a_y and one division"""
    if wrong == "pitches_swapped":
        l_x, l_y = l_y, l_x
    a_x = table(alpha, n_x, l_x, dims and dims[0], wrong).astype(dtype)
    a_y = table(alpha, n_y, l_y, dims and dims[1], wrong).astype(dtype)
    return dtype(1) / ((dtype(1) + a_x)[None, :] + a_y[:, None])


def alpha(det, delta_over_beta, energy_kev):
    """pi lambda (delta / beta) d_od (d_so + d_od) / d_so in mm^2, float32; det: the nine numbers of a detector geometry"""
    d_so, d_od = abs(float(np.float32(det[6]))), abs(float(np.float32(det[7])))
    return np.float32(np.pi * (1.2398419843e-6 / energy_kev) * delta_over_beta * d_od * (d_so + d_od) / d_so)


def default_margin(alpha_mm2, l_x, l_y):
    return int(min(MARGIN_MAX, max(8, np.ceil(6.0 * np.sqrt(float(np.float32(alpha_mm2))) / (2.0 * np.pi * float(min(np.float32(l_x), np.float32(l_y))))))))


def scratch_bytes(dim_y, n_x):
    frame = dim_y * (n_x // 2 + 1) * 8
    return max(1, min(16, (64 << 20) // frame)) * frame


def entered(p):
    """the pixels that enter the filter: p and the fp32 expf(-p) finite"""
    p = np.asarray(p, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        return np.isfinite(p) & np.isfinite(np.exp(-p))


def transmission64(p, alpha_mm2, t_min, margin, l_x, l_y, wrong=None):
    """T' of the rule in float64 on the dim_x x dim_y pixels, before the floor"""
    p = np.asarray(p, np.float32)
    dim_y, dim_x = p.shape
    n_x, n_y = padded(dim_x, margin), padded(dim_y, margin)
    ok = entered(p)
    t = np.where(ok, np.exp(-np.where(ok, p, 0).astype(np.float64)), 1.0)
    if wrong == "floor_first":
        t = np.maximum(t, float(np.float32(t_min)))
    h = transfer(alpha_mm2, n_x, n_y, l_x, l_y, np.float64, (dim_x, dim_y), wrong)
    return np.fft.ifft2(np.fft.fft2(extend(t, n_x, n_y, wrong)) * h).real[:dim_y, :dim_x]


def retrieve64(p, alpha_mm2, t_min, margin, l_x, l_y, wrong=None):
    p = np.asarray(p, np.float32)
    t = transmission64(p, alpha_mm2, t_min, margin, l_x, l_y, wrong)
    return np.where(entered(p), (-np.log(np.maximum(t, float(np.float32(t_min))))).astype(np.float32), p)


def _bit_reversal(n):
    bits = n.bit_length() - 1
    r = np.zeros(n, np.int64)
    for b in range(bits):
        r |= ((np.arange(n) >> b) & 1) << (bits - 1 - b)
    return r


def fft32(re, im, inverse=False):
    """radix 2, decimation in time along the last axis, unnormalised; float32 arrays in, every product, sum and difference rounded to
    fp32 (numpy rounds each float32 array operation), twiddles rounded from float64"""
    n = re.shape[-1]
    rev = _bit_reversal(n)
    re, im = np.ascontiguousarray(re[..., rev], np.float32), np.ascontiguousarray(im[..., rev], np.float32)
    ang = -2.0 * np.pi * np.arange(n // 2) / n
    wr, wi = np.cos(ang).astype(np.float32), (np.sin(ang) * (-1.0 if inverse else 1.0)).astype(np.float32)
    lead = re.shape[:-1]
    half = 1
    while half < n:
        shape = lead + (n // (2 * half), 2, half)
        re, im = re.reshape(shape), im.reshape(shape)
        cr, ci = wr[::n // (2 * half)], wi[::n // (2 * half)]
        ar, ai, br, bi = re[..., 0, :], im[..., 0, :], re[..., 1, :], im[..., 1, :]
        tr = br * cr - bi * ci
        ti = br * ci + bi * cr
        re = np.stack([ar + tr, ar - tr], axis=-2)
        im = np.stack([ai + ti, ai - ti], axis=-2)
        half *= 2
    return re.reshape(lead + (n,)), im.reshape(lead + (n,))


def retrieve32(p, alpha_mm2, t_min, margin, l_x, l_y):
    """the rule in fp32 throughout: exp, transforms, H, scaling, log"""
    p = np.asarray(p, np.float32)
    dim_y, dim_x = p.shape
    n_x, n_y = padded(dim_x, margin), padded(dim_y, margin)
    ok = entered(p)
    t = np.where(ok, np.exp(-np.where(ok, p, np.float32(0))), np.float32(1)).astype(np.float32)
    re = extend(t, n_x, n_y)
    re, im = fft32(re, np.zeros_like(re))
    re, im = fft32(re.T, im.T)                                   # (n_x, n_y): columns along the last axis
    h = transfer(alpha_mm2, n_x, n_y, l_x, l_y, np.float32).T
    re, im = fft32(re * h, im * h, inverse=True)
    re, im = fft32(re.T[:dim_y], im.T[:dim_y], inverse=True)
    t1 = re[:, :dim_x] * np.float32(1.0 / (n_x * n_y))
    return np.where(ok, -np.log(np.maximum(t1, np.float32(t_min))), p).astype(np.float32)


def error(p_out, p_in, alpha_mm2, t_min, margin, l_x, l_y):
    """E of DESIGN.md section 4.22: the largest |exp(-p') - max(T'_64, t_min)| over the pixels that entered the filter"""
    ok = entered(p_in)
    t = np.maximum(transmission64(p_in, alpha_mm2, t_min, margin, l_x, l_y), float(np.float32(t_min)))
    return float(np.abs(np.exp(-np.asarray(p_out, np.float64)[ok]) - t[ok]).max())


# ---- inputs -----------------------------------------------------------------------------------------------------------------------

def blob(dim_x, dim_y, seed=0):
    """a smooth blob plus 2 % noise with one pixel at p = 6: 0 <= p, T' stays above 0.05"""
    rng = np.random.default_rng(seed + 31 * dim_x + dim_y)
    y, x = np.mgrid[0:dim_y, 0:dim_x]
    r2 = ((x - 0.4 * dim_x) / (0.3 * dim_x + 1)) ** 2 + ((y - 0.55 * dim_y) / (0.3 * dim_y + 1)) ** 2
    p = 1.5 * np.exp(-r2) * (1.0 + 0.02 * rng.standard_normal((dim_y, dim_x)))
    if p.size > 1:
        p[dim_y // 2, dim_x // 3] = 6.0
    return p.astype(np.float32)


def ramp(dim_x, dim_y):
    """a ramp whose left and right, top and bottom edges differ: the extension matters"""
    y, x = np.mgrid[0:dim_y, 0:dim_x]
    return (0.1 + 1.6 * x / max(1, dim_x - 1) + 0.7 * y / max(1, dim_y - 1)).astype(np.float32)


# ---- the scene of the physical check ------------------------------------------------------------------------------------------------

SCENE_DET = metal_rule.SCENE_DET
SCENE_GRID = metal_rule.SCENE_GRID
SCENE_VIEWS = metal_rule.SCENE_VIEWS
SCENE_RADIUS = 12.0
SCENE_ELLIPSOIDS = [(0.02, 1, 1, .45, 0, 0, 0, 0), (0.05, .25, .25, .25, .4, 0, 0, 0), (0, .2, .2, .2, -.4, .1, 0, 0)]
SCENE_T_MIN = 1e-6
SCENE_FRINGE_GRID = 256


def scene_frames():
    """the scene's exact line integrals, float32 (views, n_col, n_row): every frame ends in air on every edge"""
    n_row, n_col, l_r, l_c, _, _, d_so, d_od, step = SCENE_DET
    return np.stack([phantom.projection(n_row, n_col, l_r, l_c, d_so, d_od, i * step, SCENE_RADIUS, ellipsoids=SCENE_ELLIPSOIDS)
                     for i in range(SCENE_VIEWS)])


def fringed(frames, alpha_mm2, noise=0.0, seed=5):
    """Propagation fringes from the transport-of-intensity model, I = IFFT2((1 + alpha f^2) FFT2(T)) on a 256^2 grid in float64 (the
    frame extended by its edge, which is air), optional Gaussian noise on I, p = -ln I as float32"""
    n = SCENE_FRINGE_GRID
    l_x, l_y = SCENE_DET[2], SCENE_DET[3]
    k = np.fft.fftfreq(n) * n
    g = 1.0 + alpha_mm2 * ((k / (n * l_x)) ** 2)[None, :] + alpha_mm2 * ((k / (n * l_y)) ** 2)[:, None]
    rng = np.random.default_rng(seed)
    out = []
    for p in frames:
        dim_y, dim_x = p.shape
        t = np.pad(np.exp(-p.astype(np.float64)), ((0, n - dim_y), (0, n - dim_x)), mode="edge")
        i = np.fft.ifft2(np.fft.fft2(t) * g).real[:dim_y, :dim_x]
        if noise:
            i = i + noise * rng.standard_normal(i.shape)
        out.append((-np.log(i)).astype(np.float32))
    return np.stack(out)


def scene_rms(volume, exact):
    """RMS over the grid against the volume of the exact line integrals"""
    return float(np.sqrt(np.mean((np.asarray(volume, np.float64) - exact) ** 2)))
