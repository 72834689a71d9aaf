"""The scene of the starvation filter's physical check: the detector and grid of section 4.21's check, a soft
ellipsoid that holds a dense bar, Poisson noise at a flux for which the rays along the bar count a few photons. Everything is float64
model code (tests/phantom.py, tests/fdk_model.py through tests/metal_rule.py) and a seeded numpy generator; nothing here touches a
device. The numbers below were measured once with the numpy rule of tests/starvation_rule.py. A helper, not a test."""
import functools
import types

import numpy as np

import metal_rule
import phantom
from paris_amd import backend as B

DET = metal_rule.SCENE_DET            # 64 x 32 pixels of 1 mm at 500 / 500 mm, views 3 degrees apart
VIEWS = metal_rule.SCENE_VIEWS        # 120
GRID = metal_rule.SCENE_GRID          # 64 x 64 x 24 voxels of 0.5 mm
RADIUS = metal_rule.SCENE_RADIUS      # 12 mm
SOFT, BAR = 0.2, 0.32                 # [1 / mm] the body's density -- at most 24 mm of it: 4.8 -- and what the bar adds: 5.4 along its 16.8 mm
ELLIPSOIDS = [(SOFT, 1, 1, .45, 0, 0, 0, 0), (BAR, .7, .25, .3, 0, 0, 0, 20)]
N0 = 50000.0                          # photons per pixel in air: 410 behind the longest soft path, 2 behind the longest ray along the bar
SEED = 4
SETTING = (5.0, 1.0, 3)               # p0 a little above the longest soft-only path, full equalisation, the driver's default radius
SHARE_MIN, SHARE_MAX = 0.02, 0.5      # of the scan's pixels the filter may touch for the check to mean anything
# Measured on the float64 model with the numpy rule: RMS difference to the noise-free reconstruction over the soft voxels away from the
# bar 8.942e-3 per mm without the filter and 4.881e-3 with it, ratio 0.5459; 10.76 % of the pixels filtered, 3.26 % of those at level 63.
RATIO_64 = 0.5459
# The bound: the measured ratio plus 0.15. Section 4.21 doubled its ratio of 0.1; doubled, this one would allow a filter that does
# nothing. The margin need not cover a projector or fp32 arithmetic: the device's frames are the host rule's bit for bit, and both
# tests reconstruct them with the same float64 model, so it only keeps the bound from being a copy of the measurement.
RATIO_BOUND = 0.70
# The far region's change: the model's chain never mixes detector rows (the weight is per pixel, the ramp runs along a row, a voxel
# reads the rows its ray meets), and the rays of the far slices stay clear of the bar's shadow, so the filter leaves every input of
# those voxels as it was: the change measured on the model is exactly 0. The bound leaves float64 rounding of a density of 0.2 per mm.
FAR_BOUND = 1e-12
FAR_Z = 8.0                           # [voxels] from the mid-plane: the slices whose rays never cross the bar's shadow


@functools.lru_cache(maxsize=None)
def scene():
    """the exact line integrals, the noisy ones, the reconstructions of both and the two regions, computed once per process"""
    n_row, n_col, l_r, l_c, _, _, d_so, d_od, step = DET
    det, vg = B.DetectorGeometry(*DET), B.VolumeGeometry(*GRID)
    exact = np.stack([phantom.projection(n_row, n_col, l_r, l_c, d_so, d_od, i * step, RADIUS, ellipsoids=ELLIPSOIDS) for i in range(VIEWS)])
    rng = np.random.default_rng(SEED)
    counts = rng.poisson(N0 * np.exp(-exact.astype(np.float64)))
    noisy = (-np.log(np.maximum(counts, 0.5) / N0)).astype(np.float32)       # a pixel without a photon reads as half a photon
    truth = truth_of(vg)
    bar = truth > SOFT + 0.5 * BAR
    near = np.zeros_like(bar)
    dy, dx = truth.shape[1:]
    for sy in range(-3, 4):
        for sx in range(-3, 4):
            y0, y1, x0, x1 = max(0, -sy), min(dy, dy - sy), max(0, -sx), min(dx, dx - sx)
            near[:, y0:y1, x0:x1] |= bar[:, y0 + sy:y1 + sy, x0 + sx:x1 + sx]
    near |= near.any(axis=0)[None]                                             # the bar's footprint through every slice
    soft = (truth > 0.5 * SOFT) & ~near
    z = np.abs(np.arange(truth.shape[0]) + 0.5 - truth.shape[0] / 2)
    far = (truth > 0.5 * SOFT) & (z >= FAR_Z)[:, None, None]
    sc = types.SimpleNamespace(det=det, vg=vg, exact=exact, noisy=noisy, soft=soft, far=far)
    sc.v_exact = metal_rule.reconstruct64(exact, det, vg)
    sc.v_noisy = metal_rule.reconstruct64(noisy, det, vg)
    return sc


def truth_of(vg):
    def centres(n, edge):
        return (np.arange(int(n)) + 0.5) * float(edge) - int(n) * float(edge) / 2
    return phantom.density(centres(vg.dim_x, vg.l_vx_x)[None, None, :], centres(vg.dim_y, vg.l_vx_y)[None, :, None],
                           centres(vg.dim_z, vg.l_vx_z)[:, None, None], RADIUS, ELLIPSOIDS)


def rms(a, b, where):
    return float(np.sqrt(np.mean((a[where] - b[where]) ** 2)))


def measure(sc, filtered_frames):
    """(RMS difference to the noise-free reconstruction over the soft voxels away from the bar without the filter, the same with it,
    the largest change of a voxel of the far region)"""
    v = metal_rule.reconstruct64(filtered_frames, sc.det, sc.vg)
    return rms(sc.v_noisy, sc.v_exact, sc.soft), rms(v, sc.v_exact, sc.soft), float(np.abs(v - sc.v_noisy)[sc.far].max())
