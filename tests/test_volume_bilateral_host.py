"""The 3-D bilateral filter on the host: paris_hip_volume_bilateral_host against the numpy restatement of
tests/bilateral_rule.py bit for bit, the tables against math.exp, the misreadings the parity tests must tell apart, voxels that are
not finite, chunking, every refusal, and the filter's effect against a float64 model with the exact Gaussian. No device."""
import ctypes as C
import math

import numpy as np
import pytest

import bilateral_rule as R
from paris_amd import _lib
from paris_amd import backend as B

INVALID = _lib.ERROR_INVALID_ARGUMENT
SIGMA_R, SIGMA_S = 0.25, 1.25


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def noisy(shape, seed=7):
    """a smooth ramp plus noise of about sigma_r: taps land in every part of the range table, some beyond the cutoff"""
    rng = np.random.default_rng(seed)
    z, y, x = np.meshgrid(*[np.arange(n, dtype=np.float32) for n in shape], indexing="ij")
    return (np.float32(0.02) * (x + y - z) + rng.normal(0.0, 0.3, shape).astype(np.float32)).astype(np.float32)


@pytest.fixture(scope="module")
def volume():
    v = noisy((11, 19, 37))
    v.setflags(write=False)
    return v


@pytest.fixture(scope="module")
def rule_r2(volume):
    out = R.bilateral(volume, SIGMA_R, SIGMA_S, 2)
    out.setflags(write=False)
    return out


@pytest.mark.parametrize("r", [1, 2, 3])
def test_host_rule_equals_the_restatement(volume, r):
    got = B.volume_bilateral_host(volume, SIGMA_R, SIGMA_S, r)
    assert same_bits(got, R.bilateral(volume, SIGMA_R, SIGMA_S, r))
    assert not same_bits(got, volume)


@pytest.mark.parametrize("shape", [(3, 4, 5), (1, 1, 1)])
@pytest.mark.parametrize("r", [1, 2, 3])
def test_volumes_thinner_than_the_stencil(shape, r):
    v = noisy(shape, seed=11)
    got = B.volume_bilateral_host(v, SIGMA_R, SIGMA_S, r)
    assert same_bits(got, R.bilateral(v, SIGMA_R, SIGMA_S, r))
    if shape == (1, 1, 1):  # one tap: w v / w
        w = np.float32(R.tables(SIGMA_R, SIGMA_S, r)[0][r, r, r] * R.tables(SIGMA_R, SIGMA_S, r)[1][0])
        assert same_bits(got, ((w * v) / w).astype(np.float32))


@pytest.mark.parametrize("r", [1, 2, 3])
def test_tables(r):
    """The range table against math.exp of the bin's own edges: the Gaussian is monotonic, so R[i] lies between its values at the two
    edges, and no weight inside a bin is further from R[i] than (2 / 1024) e^-1/2 -- half a bin times the steepest slope -- plus the
    rounding to float. Beyond the table the exact weight is at most e^-8. The spatial table is math.exp rounded once."""
    spatial, rng, rscale = B.volume_bilateral_tables(SIGMA_R, SIGMA_S, r)
    want_s, want_r, want_scale = R.tables(SIGMA_R, SIGMA_S, r)
    assert same_bits(spatial, want_s) and same_bits(rng, want_r) and np.float32(rscale) == want_scale
    assert rscale == float(np.float32(1024.0 / (4.0 * float(np.float32(SIGMA_R)))))
    bound = (2.0 / 1024.0) * math.exp(-0.5)
    assert bound < 0.0012
    worst = 0.0
    for i in range(R.BINS):
        lo, hi = math.exp(-0.5 * (i * 4.0 / 1024) ** 2), math.exp(-0.5 * ((i + 1) * 4.0 / 1024) ** 2)
        assert hi <= float(rng[i]) <= lo
        worst = max(worst, lo - float(rng[i]), float(rng[i]) - hi)
    assert worst <= bound + 2.0 ** -24
    assert math.exp(-0.5 * 4.0 ** 2) == math.exp(-8.0) and float(rng[-1]) > math.exp(-8.0)
    assert spatial[r, r, r] == 1.0
    for (dz, dy, dx) in [(-r, 0, r), (1, -1, 0), (r, r, r)]:
        exact = math.exp(-(dx * dx + dy * dy + dz * dz) / (2.0 * float(np.float32(SIGMA_S)) ** 2))
        assert float(spatial[dz + r, dy + r, dx + r]) == float(np.float32(exact))


@pytest.mark.parametrize("misreading", [dict(centre=False), dict(border="clamp"), dict(order="xyz"), dict(contract=True), dict(cutoff_weight=True)],
                         ids=lambda m: "%s=%s" % next(iter(m.items())))
def test_misreadings_differ_in_bits(volume, rule_r2, misreading):
    """the parity tests discriminate: each misreading of the statement changes bits of this volume, and the host rule has the rule's"""
    assert same_bits(B.volume_bilateral_host(volume, SIGMA_R, SIGMA_S, 2), rule_r2)
    wrong = R.bilateral(volume, SIGMA_R, SIGMA_S, 2, **misreading)
    assert not same_bits(wrong, rule_r2)
    if "border" in misreading:  # only voxels within r of a face see the border
        assert same_bits(wrong[2:-2, 2:-2, 2:-2], rule_r2[2:-2, 2:-2, 2:-2])


def special_volume():
    v = noisy((7, 9, 12), seed=3)
    v[3, 4, 5] = np.nan
    v[1, 1, 1] = np.inf
    v[5, 7, 10] = -np.inf
    v[0, 0, 0] = np.nan
    v[6, 8, 11] = np.inf
    return v


@pytest.mark.parametrize("r", [1, 3])
def test_voxels_that_are_not_finite(r):
    v = special_volume()
    got = B.volume_bilateral_host(v, SIGMA_R, SIGMA_S, r)
    assert same_bits(got, R.bilateral(v, SIGMA_R, SIGMA_S, r))
    bad = ~np.isfinite(v)
    assert same_bits(got[bad], v[bad])          # a centre that is not finite is written as stored
    assert np.isfinite(got[~bad]).all()        # and as a neighbour it drops out
    # a finite voxel surrounded by nothing finite keeps its value up to the division w v / w
    lone = np.full((3, 3, 3), np.nan, np.float32)
    lone[1, 1, 1] = 0.7
    out = B.volume_bilateral_host(lone, SIGMA_R, SIGMA_S, 1)
    assert abs(float(out[1, 1, 1]) - 0.7) <= 2.0 ** -23 and np.isnan(out).sum() == 26


def test_a_step_above_the_cutoff_keeps_both_plateaus():
    """Two plateaus more than 4 sigma_r apart: no tap crosses the edge, and within a plateau every tap has d = 0, so the result is
    (sum of w v) / (sum of w) over the plateau's own taps. With levels 0 and a power of two, w * v only shifts the exponent of w,
    every partial sum of num is den times v exactly, and every voxel -- at the edge too -- comes back unchanged in bits. A level
    with more mantissa bits rounds once per product and once per sum: 2 * 125 + 1 roundings bound its departure."""
    v = np.zeros((8, 10, 14), np.float32)
    v[:, :, 7:] = 2.0                               # 8 sigma_r
    v[:, 5:, :7] = -0.0                             # (and the sign of a zero plateau: +0 + w * -0 = +0)
    got = B.volume_bilateral_host(v, SIGMA_R, SIGMA_S, 2)
    assert same_bits(got, R.bilateral(v, SIGMA_R, SIGMA_S, 2))
    assert same_bits(got[:, :, 7:], v[:, :, 7:])
    assert same_bits(got[:, :, :7], np.zeros((8, 10, 7), np.float32))
    hi = np.float32(4.5 * SIGMA_R)
    v2 = np.zeros((8, 10, 14), np.float32)
    v2[:, :, 7:] = hi
    got2 = B.volume_bilateral_host(v2, SIGMA_R, SIGMA_S, 2)
    assert same_bits(got2, R.bilateral(v2, SIGMA_R, SIGMA_S, 2))
    assert same_bits(got2[:, :, :7], v2[:, :, :7])
    assert np.abs(got2[:, :, 7:] - hi).max() <= 251 * 2.0 ** -24 * float(hi)


def test_a_result_can_be_negative_zero():
    """why the device call marks its destination dirty: the smallest negative denormal everywhere, neighbours' products round to -0 or
    stay, and num / den with den > 2 rounds to -0"""
    v = np.full((3, 3, 3), -np.float32(1.4e-45), np.float32)
    out = B.volume_bilateral_host(v, 1.0, 0.8, 1)
    assert same_bits(out, R.bilateral(v, 1.0, 0.8, 1))
    assert bits(out)[1, 1, 1] == 0x80000000


@pytest.mark.parametrize("cuts", [(0, 11), (0, 1, 11), (0, 4, 5, 9, 11), tuple(range(12))])
def test_chunks_equal_the_whole(volume, rule_r2, cuts):
    parts = [B.volume_bilateral_host(volume, SIGMA_R, SIGMA_S, 2, z_first=a, z_count=b - a) for a, b in zip(cuts[:-1], cuts[1:])]
    assert same_bits(np.concatenate(parts), rule_r2)


def test_a_slab_with_its_halo_equals_the_whole(volume, rule_r2):
    """what the driver does: slab [4, 8) of the grid, passed with r slices on each side and without them in the range"""
    got = B.volume_bilateral_host(volume[2:10], SIGMA_R, SIGMA_S, 2, z_first=2, z_count=4)
    assert same_bits(got, rule_r2[4:8])


def check(sigma_r, sigma_s, radius):
    b = _lib.VolumeBilateral(sigma_r, sigma_s, radius)
    return _lib.load().paris_hip_volume_bilateral_check(C.byref(b))


def test_check_accepts():
    for r in (1, 2, 3):
        assert check(0.25, 1.0, r) == 0
    assert check(3e38, 1e-3, 1) == 0          # rscale = 256 / 3e38 is a denormal above 0
    assert check(1e-36, 1e30, 3) == 0         # rscale = 2.56e38 is finite


@pytest.mark.parametrize("what,sigma_r,sigma_s,radius", [
    ("sigma_r not finite", float("nan"), 1.0, 1),
    ("sigma_r not finite", float("inf"), 1.0, 1),
    ("sigma_s not finite", 0.25, float("nan"), 1),
    ("sigma_s not finite", 0.25, float("inf"), 1),
    ("sigma_r not above 0", 0.0, 1.0, 1),
    ("sigma_r not above 0", -0.25, 1.0, 1),
    ("sigma_s not above 0", 0.25, 0.0, 1),
    ("sigma_s not above 0", 0.25, -1.0, 1),
    ("radius 0", 0.25, 1.0, 0),
    ("radius 4", 0.25, 1.0, 4),
    ("rscale not finite", 1e-37, 1.0, 1),
    ("rscale not finite", 1e-45, 1.0, 1),
])
def test_check_refusals(what, sigma_r, sigma_s, radius):
    """One case per clause. `rscale is 0` has none: the largest float gives 256 / 3.4e38 = 7.5e-37 -- the clause guards the arithmetic."""
    assert check(sigma_r, sigma_s, radius) == INVALID, what


def test_check_and_tables_refuse_null_and_what_the_check_refuses():
    L = _lib.load()
    assert L.paris_hip_volume_bilateral_check(None) == INVALID
    out = np.empty(1024, np.float32)
    assert L.paris_hip_volume_bilateral_tables(None, None, out.ctypes.data, None) == INVALID
    bad = _lib.VolumeBilateral(0.25, 1.0, 4)
    assert L.paris_hip_volume_bilateral_tables(C.byref(bad), None, out.ctypes.data, None) == INVALID
    good = _lib.VolumeBilateral(0.25, 1.0, 1)
    assert L.paris_hip_volume_bilateral_tables(C.byref(good), None, None, None) == 0   # any output may be NULL


def test_entry_point_refusals():
    L = _lib.load()
    v = noisy((4, 3, 5))
    out = np.empty((5, 3, 5), np.float32)
    good, bad = _lib.VolumeBilateral(0.25, 1.0, 1), _lib.VolumeBilateral(0.25, 1.0, 0)

    def call(src=v.ctypes.data, dim_x=5, dim_y=3, dim_z=4, z_first=0, z_count=4, setting=good, dst=out.ctypes.data):
        return L.paris_hip_volume_bilateral_host(src, dim_x, dim_y, dim_z, z_first, z_count, C.byref(setting) if setting is not None else None, dst)

    assert call() == 0
    assert call(src=None) == INVALID and call(dst=None) == INVALID and call(setting=None) == INVALID
    assert call(setting=bad) == INVALID
    assert call(dim_x=0) == INVALID and call(dim_y=0) == INVALID
    assert call(z_count=0) == INVALID
    assert call(z_first=1, z_count=4) == INVALID and call(z_first=4, z_count=1) == INVALID and call(z_first=5, z_count=0) == INVALID
    assert call(z_first=0xFFFFFFFF, z_count=2) == INVALID      # the sum does not wrap
    assert call(z_first=3, z_count=1) == 0
    assert call(src=v.ctypes.data + 2) == INVALID and call(dst=out.ctypes.data + 1) == INVALID   # not 4-byte aligned
    # destination ranges that overlap the source buffer: the same memory, its tail, its head
    both = np.zeros(2 * v.size, np.float32)
    both[:v.size] = v.ravel()
    assert call(src=both.ctypes.data, dst=both.ctypes.data) == INVALID
    assert call(src=both.ctypes.data, dst=both.ctypes.data + 4 * (v.size - 1)) == INVALID
    assert call(src=both.ctypes.data + 4 * 15, z_count=1, dst=both.ctypes.data + 4) == INVALID
    assert call(src=both.ctypes.data, dst=both.ctypes.data + 4 * v.size) == 0              # adjacent is apart
    assert call(src=both.ctypes.data + 4 * 15, z_count=1, dst=both.ctypes.data) == 0


# ---- effect --------------------------------------------------------------------------------------------------
E_SIGMA_R, E_SIGMA_S, E_R = 0.1, 1.0, 2


def phantom():
    """two levels 10 sigma_r apart: a block in a background, seeded Gaussian noise of sigma_r / 2"""
    clean = np.zeros((12, 24, 32), np.float64)
    clean[:, 6:18, 8:24] = 10 * E_SIGMA_R
    noise = np.random.default_rng(2026).normal(0.0, E_SIGMA_R / 2, clean.shape)
    return clean, (clean + noise).astype(np.float32)


def test_effect_against_a_float64_model():
    """Measured on the CPU that ran this first (model / library):
         flat-region noise (std of out - clean inside the block, 2 voxels from its faces), input 0.05027: 0.01448 / 0.01448, a reduction to 0.288;
         edge profile (mean over z and the block's rows of |out - clean| in the 4 columns around each x face of the block): 0.01284 / 0.01284;
         largest |library - model|: 2.55e-5, where the largest per-voxel table bound is 4.53e-4 and the fp32 share 2.78e-5.
       The library may exceed the model by a factor of 2 in the first two. The third is held voxel by voxel to the bound that follows
       from the table's error (bilateral_rule.float64_model) plus 400 roundings of fp32 accumulation at the volume's scale."""
    clean, v = phantom()
    model, bound = R.float64_model(v, float(np.float32(E_SIGMA_R)), E_SIGMA_S, E_R, with_bound=True)
    got = B.volume_bilateral_host(v, E_SIGMA_R, E_SIGMA_S, E_R).astype(np.float64)
    inner = (slice(2, -2), slice(8, 16), slice(10, 22))
    noise_in = (v[inner] - clean[inner]).std()
    noise_model, noise_got = (model[inner] - clean[inner]).std(), (got[inner] - clean[inner]).std()
    edge = (slice(None), slice(6, 18), [6, 7, 8, 9, 22, 23, 24, 25])
    edge_model, edge_got = np.abs(model[edge] - clean[edge]).mean(), np.abs(got[edge] - clean[edge]).mean()
    diff = np.abs(got - model)
    fp32 = 400 * 2.0 ** -24 * float(np.abs(v).max())
    print("noise in %.4g model %.4g library %.4g; edge model %.4g library %.4g; max diff %.3g, max bound %.3g, fp32 share %.3g"
          % (noise_in, noise_model, noise_got, edge_model, edge_got, diff.max(), bound.max(), fp32))
    assert noise_model < 0.5 * noise_in                      # the model itself denoises: the phantom is a fair one
    assert noise_got <= 2.0 * noise_model
    assert edge_got <= 2.0 * edge_model
    assert edge_model < 0.05 * 10 * E_SIGMA_R                # the edge stays an edge: a Gaussian blur of sigma_s = 1 leaves 0.2 of the step here
    assert (diff <= bound + fp32).all()
