"""Scatter kernel superposition, restated in numpy from the statement in include/paris_hip.h: correct64 is
the rule in float64 with np.fft.fft2, correct32 the same rule with phase_rule's explicit radix-2 transform and every operation
rounded to fp32 -- the independent fp32 yardstick the device's error is measured against. `wrong` selects a plausible misreading of
the statement; the tests show that each one is told apart. A setting is the tuple (A, alpha, beta, sigma1_mm, sigma2_mm, w2, limit,
iterations, margin), the fields of paris_hip_scatter_correction in order. A helper, not a test."""
import numpy as np

import phase_rule as P

ITERATIONS_MAX = 16
WRONG = ("sigma_is_fwhm", "pitches_swapped", "update_from_estimate", "clamp_to_estimate", "dc_gain", "source_from_measured")

# (dim_x, dim_y, margin, n_x, n_y, l_x, l_y): phase_rule's shapes without its large case, and 20 x 600, which pads to 32 x 1024 --
# the 8-column class of the column pass
SHAPES = [s for s in P.SHAPES if s[:2] != (1000, 700)] + [(20, 600, 4, 32, 1024, 1.0, 1.0)]


def setting_for(l_x, iterations=4, margin=1):
    """the parameters of the device tests: kernels 3 and 10 pixels wide, a clamp that stays idle on the smooth inputs"""
    return (0.02, -0.15, 1.0, 3.0 * l_x, 10.0 * l_x, 0.5, 0.6, iterations, margin)


def f32(v):
    return float(np.float32(v))


def gaussian(weight, sigma, n, pitch):
    """weight exp(-2 pi^2 sigma^2 f^2) in float64, rounded once to float32"""
    k = np.arange(n, dtype=np.float64)
    k = np.where(k <= n // 2, k, k - n)
    f = k / (n * f32(pitch))
    return (weight * np.exp(-2.0 * np.pi ** 2 * f32(sigma) ** 2 * f * f)).astype(np.float32)


def tables(setting, n_x, n_y, l_x, l_y, wrong=None):
    """g1x, g2x, g1y, g2y as float32"""
    _, _, _, s1, s2, w2, _, _, _ = setting
    if wrong == "pitches_swapped":
        l_x, l_y = l_y, l_x
    if wrong == "sigma_is_fwhm":
        s1, s2 = (f32(s) / (2.0 * np.sqrt(2.0 * np.log(2.0))) for s in (s1, s2))
    w2 = f32(w2)
    norm = 1.0 if wrong == "dc_gain" else 1.0 + w2
    return (gaussian(1.0 / norm, s1, n_x, l_x), gaussian(w2 / norm, s2, n_x, l_x), gaussian(1.0, s1, n_y, l_y), gaussian(1.0, s2, n_y, l_y))


def transfer(setting, n_x, n_y, l_x, l_y, dtype=np.float64, wrong=None):
    """G (n_y, n_x) from the four float32 tables: two products and one sum in `dtype`"""
    g1x, g2x, g1y, g2y = (g.astype(dtype) for g in tables(setting, n_x, n_y, l_x, l_y, wrong))
    return g1x[None, :] * g1y[:, None] + g2x[None, :] * g2y[:, None]


def default_margin(sigma1, sigma2, l_x, l_y):
    return int(min(P.MARGIN_MAX, max(8, np.ceil(3.0 * float(max(np.float32(sigma1), np.float32(sigma2))) / float(min(np.float32(l_x), np.float32(l_y)))))))


def entered(p):
    """the pixels that enter the correction: p finite and 0 < expf(-p) < inf in fp32"""
    p = np.asarray(p, np.float32)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        t = np.exp(-p)
        return np.isfinite(p) & np.isfinite(t) & (t > 0)


def source(t, setting, dtype):
    """q = A exp(alpha lnT + beta log(L)) where L = -lnT > 0, else 0; every operation in `dtype`"""
    a, alpha, beta = (dtype(np.float32(v)) for v in setting[:3])
    with np.errstate(divide="ignore", invalid="ignore"):
        ln_t = np.log(t)
        path = -ln_t
        q = a * np.exp(alpha * ln_t + beta * np.log(path))
    return np.where(path > 0, q, dtype(0)).astype(dtype)


def primary64(p, setting, l_x, l_y, wrong=None, history=False):
    """T^n of the rule in float64 on the dim_x x dim_y pixels (the measured T_m where a pixel did not enter: 1)"""
    p = np.asarray(p, np.float32)
    dim_y, dim_x = p.shape
    limit, iterations, margin = setting[6:]
    n_x, n_y = P.padded(dim_x, margin), P.padded(dim_y, margin)
    ok = entered(p)
    t_m = np.where(ok, np.exp(-np.where(ok, p, 0).astype(np.float64)), 1.0)
    g = transfer(setting, n_x, n_y, l_x, l_y, np.float64, wrong)
    keep = 1.0 - f32(limit)
    t, steps = t_m, []
    for _ in range(iterations):
        q = source(t_m if wrong == "source_from_measured" else t, setting, np.float64)
        s = np.fft.ifft2(np.fft.fft2(P.extend(q, n_x, n_y)) * g).real[:dim_y, :dim_x]
        t = np.maximum((t if wrong == "update_from_estimate" else t_m) - s, keep * (t if wrong == "clamp_to_estimate" else t_m))
        steps.append(t)
    return (t, steps) if history else t


def correct64(p, setting, l_x, l_y, wrong=None):
    p = np.asarray(p, np.float32)
    t = primary64(p, setting, l_x, l_y, wrong)
    return np.where(entered(p), (-np.log(t)).astype(np.float32), p)


def correct32(p, setting, l_x, l_y):
    """the rule in fp32 throughout: exp, source, transforms, G, scaling, update, log"""
    p = np.asarray(p, np.float32)
    dim_y, dim_x = p.shape
    limit, iterations, margin = setting[6:]
    n_x, n_y = P.padded(dim_x, margin), P.padded(dim_y, margin)
    ok = entered(p)
    t_m = np.where(ok, np.exp(-np.where(ok, p, np.float32(0))), np.float32(1)).astype(np.float32)
    g = transfer(setting, n_x, n_y, l_x, l_y, np.float32).T
    keep = np.float32(1) - np.float32(limit)
    scale = np.float32(1.0 / (n_x * n_y))
    t = t_m
    for _ in range(iterations):
        re = P.extend(source(t, setting, np.float32), n_x, n_y)
        re, im = P.fft32(re, np.zeros_like(re))
        re, im = P.fft32(re.T, im.T)                               # (n_x, n_y): columns along the last axis
        re, im = P.fft32(re * g, im * g, inverse=True)
        re, im = P.fft32(re.T[:dim_y], im.T[:dim_y], inverse=True)
        t = np.maximum(t_m - re[:, :dim_x] * scale, keep * t_m).astype(np.float32)
    return np.where(ok, -np.log(t), p).astype(np.float32)


def error(p_out, p_in, setting, l_x, l_y, where=None):
    """E of DESIGN.md section 4.23: the largest |exp(-p') - T64^n| over the pixels that entered (and lie in `where`)"""
    ok = entered(p_in)
    if where is not None:
        ok = ok & where
    t = primary64(p_in, setting, l_x, l_y)
    return float(np.abs(np.exp(-np.asarray(p_out, np.float64)[ok]) - t[ok]).max())


def fraction(p, setting, l_x, l_y):
    """the scatter fraction 1 - T^n / T_m the rule removes, float64 (dim_y, dim_x)"""
    p = np.asarray(p, np.float32)
    ok = entered(p)
    t_m = np.where(ok, np.exp(-np.where(ok, p, 0).astype(np.float64)), 1.0)
    return 1.0 - primary64(p, setting, l_x, l_y) / t_m


# ---- inputs -----------------------------------------------------------------------------------------------------------------------

def smooth(dim_x, dim_y, seed=0):
    """phase_rule.blob with its p = 6 pixel replaced by its left neighbour"""
    p = P.blob(dim_x, dim_y, seed)
    if p.size > 1:
        x = dim_x // 3
        p[dim_y // 2, x] = p[dim_y // 2, x - 1 if x > 0 else x + 1]
    return p


def ramp(dim_x, dim_y):
    """0.4 phase_rule.ramp: the extension matters, and the clamp stays idle"""
    return (np.float32(0.4) * P.ramp(dim_x, dim_y)).astype(np.float32)


# ---- the scene of the physical check ------------------------------------------------------------------------------------------------

SCENE_DET, SCENE_GRID = P.SCENE_DET, P.SCENE_GRID
SCENE_FORWARD_GRID = 256
SCENE_MARGIN = 24
SCENE_RATIO_64 = 5.283e-4     # corrected / scattered RMS of the reconstruction at 4 iterations, float64 model (tests/test_scatter_host.py pins
SCENE_RATIO_32 = 5.285e-4     # both) and fp32 restatement: the device's may be at most 4 times the latter


def scene_setting(iterations=4):
    return (0.12, -0.15, 1.0, 4.0, 16.0, 0.5, 0.6, iterations, SCENE_MARGIN)


scene_frames = P.scene_frames
scene_rms = P.scene_rms


def scattered(frames, setting):
    """The forward model: T_m = T + IFFT2(FFT2(q(T), edge-padded to 256^2) G) in float64, p = -ln T_m as float32. Returns the frames and
    the largest scatter-to-primary ratio."""
    n = SCENE_FORWARD_GRID
    g = transfer(setting, n, n, SCENE_DET[2], SCENE_DET[3])
    out, ratio = [], 0.0
    for p in frames:
        dim_y, dim_x = p.shape
        t = np.exp(-p.astype(np.float64))
        q = np.pad(source(t, setting, np.float64), ((0, n - dim_y), (0, n - dim_x)), mode="edge")
        s = np.fft.ifft2(np.fft.fft2(q) * g).real[:dim_y, :dim_x]
        ratio = max(ratio, float((s / t).max()))
        out.append((-np.log(t + s)).astype(np.float32))
    return np.stack(out), ratio
