"""The 3-D bilateral filter on the device: volume_bilateral_kernel<R> against paris_hip_volume_bilateral_host
bit for bit -- on sizes around the tile (64 x 16, 64 x 8 for r = 3) and the 2r + 1 ring, past the capped grid, on a misaligned source, on a range of
slices with a sentinel canvas, on voxels that are not finite --, the retire path of its tables, work pending at the call, the
destination's clean mark and the refusals. The host rule is held to the numpy restatement by tests/test_volume_bilateral_host.py."""
import ctypes as C

import numpy as np
import pytest

import test_gpu_parity as PAR
from test_volume_bilateral_host import SIGMA_R, SIGMA_S, bits, noisy, same_bits, special_volume
from paris_amd import _lib
from paris_amd import backend as B

pytestmark = pytest.mark.gpu

INVALID = _lib.ERROR_INVALID_ARGUMENT
TILE_Y = {1: 16, 2: 16, 3: 8}   # the tile heights of volume_bilateral.hip by radius; a tile is 64 wide
SENTINEL = 0xA5A5A5A5


@pytest.fixture(scope="module")
def be():
    b = B.set_device(B.get_devices()[0])
    yield b
    b.close()


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def on_device(torch, v, offset=0):
    """the volume v on the device, `offset` floats behind a 16-byte boundary; (keep-alive, Volume)"""
    t = torch.zeros(v.size + 8, dtype=torch.float32, device="cuda")
    assert t.data_ptr() % 16 == 0
    t[offset:offset + v.size].copy_(torch.from_numpy(np.ascontiguousarray(v).ravel()))
    torch.cuda.synchronize()
    return t, B.Volume(t.data_ptr() + 4 * offset, v.shape[2], v.shape[1], v.shape[0], on_device=True)


def filtered(be, torch, v, sigma_r, sigma_s, r, z_first=0, z_count=None, offset=0, extra=0):
    """be.volume_bilateral of v into a canvas of sentinel words with `extra` slices more than the call writes: (result, the rest)"""
    keep, d_v = on_device(torch, v, offset)
    n = v.shape[0] - z_first if z_count is None else z_count
    plane = v.shape[1] * v.shape[2]
    canvas = torch.full(((n + extra) * plane + 4,), SENTINEL - (1 << 32), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    be.set_volume_bilateral(sigma_r, sigma_s, r)
    be.volume_bilateral(d_v, out=canvas.data_ptr(), z_first=z_first, z_count=n)
    be.synchronize()
    host = canvas.cpu().numpy().view(np.uint32)
    del keep
    return host[:n * plane].view(np.float32).reshape(n, v.shape[1], v.shape[2]), host[n * plane:]


def cases():
    out = []
    for r in (1, 2, 3):
        out += [(r, 1, 1, 1), (r, 63, 2 * r, 2 * r), (r, 64, 2 * r + 1, 2 * r + 1), (r, 65, TILE_Y[r] - 1, 40), (r, 130, TILE_Y[r] + 1, 2 * r + 1),
                (r, 64, TILE_Y[r] + 1, 40), (r, 130, 1, 2 * r), (r, 1, 2 * r + 1, 1), (r, 65, 2 * TILE_Y[r] + 1, 9)]
    return out


@pytest.mark.parametrize("r,dim_x,dim_y,dim_z", cases())
def test_device_equals_the_host_rule(be, torch, r, dim_x, dim_y, dim_z):
    v = noisy((dim_z, dim_y, dim_x), seed=dim_x + dim_y + dim_z)
    got, rest = filtered(be, torch, v, SIGMA_R, SIGMA_S, r)
    assert same_bits(got, B.volume_bilateral_host(v, SIGMA_R, SIGMA_S, r))
    assert (rest == SENTINEL).all()


def test_more_work_items_than_the_grid_holds(be, torch):
    """3 x 31 tiles of 64 x 16 x 23 chunks of 8 slices = 2139 work items on a grid capped at 2048 workgroups: some walk two items
    through one ring"""
    v = noisy((184, 16 * 30 + 1, 130), seed=5)
    got, rest = filtered(be, torch, v, SIGMA_R, SIGMA_S, 1)
    assert same_bits(got, B.volume_bilateral_host(v, SIGMA_R, SIGMA_S, 1))
    assert (rest == SENTINEL).all()


@pytest.mark.parametrize("offset", [1, 2, 3])
def test_a_misaligned_source_goes_voxel_by_voxel(be, torch, offset):
    v = noisy((9, TILE_Y[2] + 3, 68), seed=offset)     # dim_x is a multiple of 4: only the base keeps the vector path away
    got, _ = filtered(be, torch, v, SIGMA_R, SIGMA_S, 2, offset=offset)
    assert same_bits(got, B.volume_bilateral_host(v, SIGMA_R, SIGMA_S, 2))


@pytest.mark.parametrize("r", [1, 3])
def test_a_range_of_slices_and_nothing_beyond(be, torch, r):
    v = noisy((13, 21, 72), seed=r)
    whole = B.volume_bilateral_host(v, SIGMA_R, SIGMA_S, r)
    for z_first, z_count in [(4, 5), (1, 1), (12, 1), (0, 12)]:
        got, rest = filtered(be, torch, v, SIGMA_R, SIGMA_S, r, z_first=z_first, z_count=z_count, extra=2)
        assert same_bits(got, whole[z_first:z_first + z_count]), (z_first, z_count)
        assert rest.size == 2 * 21 * 72 + 4 and (rest == SENTINEL).all(), (z_first, z_count)


@pytest.mark.parametrize("r", [1, 3])
def test_voxels_that_are_not_finite(be, torch, r):
    v = special_volume()
    got, _ = filtered(be, torch, v, SIGMA_R, SIGMA_S, r)
    assert same_bits(got, B.volume_bilateral_host(v, SIGMA_R, SIGMA_S, r))
    bad = ~np.isfinite(v)
    assert same_bits(got[bad], v[bad]) and np.isfinite(got[~bad]).all()


def test_a_step_above_the_cutoff(be, torch):
    v = np.zeros((8, 20, 70), np.float32)
    v[:, :, 33:] = 2.0
    got, _ = filtered(be, torch, v, SIGMA_R, SIGMA_S, 2)
    assert same_bits(got, v)
    v[:, :, 33:] = np.float32(4.5 * SIGMA_R)
    got, _ = filtered(be, torch, v, SIGMA_R, SIGMA_S, 2)
    assert same_bits(got, B.volume_bilateral_host(v, SIGMA_R, SIGMA_S, 2))


def test_a_new_setting_replaces_the_old_one(torch):
    """the tables are the ctx's: counted in the reserve once made, replaced -- the old ones retired behind the queued kernel -- when a
    call brings another setting, and the results are each setting's own whatever came before"""
    v = noisy((9, 19, 66), seed=21)
    with B.Backend(0) as b:
        base = b.projection_reserve_bytes(64, 48)
        keep, d_v = on_device(torch, v)
        outs = []
        settings = [(SIGMA_R, SIGMA_S, 1), (0.5, 0.7, 3), (SIGMA_R, SIGMA_S, 1), (SIGMA_R, SIGMA_S, 2)]
        for s in settings:      # queued back to back, no wait in between
            b.set_volume_bilateral(*s)
            outs.append(b.volume_bilateral(d_v))
            assert b.projection_reserve_bytes(64, 48) == base + 4 * (1024 + (2 * s[2] + 1) ** 3)
        b.synchronize()
        for s, d_o in zip(settings, outs):
            assert same_bits(PAR.volume_to_host(b, d_o), B.volume_bilateral_host(v, *s)), s
            b.free(d_o)
        assert not same_bits(B.volume_bilateral_host(v, *settings[0]), B.volume_bilateral_host(v, *settings[1]))
        b.set_volume_bilateral(None)
        with pytest.raises(B.ParisHipError):
            b.volume_bilateral(d_v)
        del keep


def test_pending_projections_are_seen(torch, oracle):
    """with a deferral depth > 1 and projections pending into the source volume, the filter sees the finished volume"""
    det = B.DetectorGeometry(*PAR.KAT)
    vg = B.calculate_volume_geometry(det)
    projs = [oracle.lcg_projection(64, 48, i) for i in range(3)]
    with B.Backend(0) as dbe:
        dbe.set_backproject_deferral(8)
        d_ps = [PAR.to_device(dbe, p, idx=i) for i, p in enumerate(projs)]
        d_v = dbe.make_volume_device(vg.dim_x, vg.dim_y, vg.dim_z)
        dbe.memset_volume(d_v)
        for d_p in d_ps:
            B.backproject(dbe, d_p, d_v, 0, det, vg, False, False, None)
        n, ptr = C.c_uint32(0), C.c_void_p()
        assert dbe._L.paris_hip_pending_backprojections(dbe._ctx, C.byref(n), C.byref(ptr)) == 0
        assert n.value == 3 and ptr.value == d_v.ptr
        dbe.set_volume_bilateral(2.0, 1.0, 1)
        d_o = dbe.volume_bilateral(d_v)
        got = PAR.volume_to_host(dbe, d_o)
        after_three = PAR.volume_to_host(dbe, d_v)
        assert np.abs(after_three).max() > 0
        assert same_bits(got, B.volume_bilateral_host(after_three, 2.0, 1.0, 1))
        assert not same_bits(got, after_three)


def test_filtering_into_a_volume_marks_it_dirty(be, torch, oracle):
    """A result can be -0 (tests/test_volume_bilateral_host.py::test_a_result_can_be_negative_zero), so a fresh zero-filled volume --
    which may skip the tiles no ray reaches -- must take every addition once the filter has written into it: the result equals what
    paris_hip_set_backproject_skip_invalid(0) gives from the same bits, and no -0 is left. Geometry of
    test_gpu_volume_window.test_quantizing_into_a_volume_marks_it_dirty."""
    g = (64, 48, 0.4, 0.4, 1.5, -2.0, 200, 150, 23.0)
    det = B.DetectorGeometry(*g)
    nat = B.calculate_volume_geometry(det)
    dz, dy, dx = 96, 72, 192
    l_vx = float(nat.l_vx_x)
    vg = B.VolumeGeometry(dx, dy, dz, l_vx * 1.1, l_vx * 2.6, l_vx * 1.7)
    proj = oracle.lcg_projection(64, 48, 3) - np.float32(0.5)

    def add(d_v):
        d_p = PAR.to_device(be, proj, idx=3)
        B.backproject(be, d_p, d_v, 0, det, vg, False, False, None)
        be.free(d_p)
        return PAR.volume_to_host(be, d_v)

    src = np.full((dz, dy, dx), -np.float32(1.4e-45), np.float32)
    keep, d_src = on_device(torch, src)
    be.set_backproject_skip_invalid(True)
    d_v = be.make_volume_device(dx, dy, dz)
    try:
        be.memset_volume(d_v)
        be.set_volume_bilateral(1.0, 0.8, 1)
        be.volume_bilateral(d_src, out=d_v)
        start = PAR.volume_to_host(be, d_v)
        assert same_bits(start, B.volume_bilateral_host(src, 1.0, 0.8, 1))
        assert (bits(start)[1:-1, 1:-1, 1:-1] == 0x80000000).all()
        got = add(d_v)
        d_w = be.make_volume_device(dx, dy, dz)
        be.copy_h2d(B.Volume(start.copy(), dx, dy, dz), d_w)
        be.set_backproject_skip_invalid(False)
        want = add(d_w)
        be.free(d_w)
    finally:
        be.set_backproject_skip_invalid(True)
        be.free(d_v)
    PAR.assert_bit_equal(got, want)
    assert (want == 0).any() and not np.signbit(got[got == 0]).any()


def test_refusals(be, torch):
    v = noisy((4, 3, 8))
    keep, d_v = on_device(torch, v)
    dst = torch.full((2 * v.size,), 7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    good, bad = _lib.VolumeBilateral(0.25, 1.0, 1), _lib.VolumeBilateral(0.25, 1.0, 4)

    def call(src=d_v.ptr, dim_x=8, dim_y=3, dim_z=4, z_first=0, z_count=4, setting=good, out=dst.data_ptr()):
        return be._L.paris_hip_volume_bilateral(be._ctx, src, dim_x, dim_y, dim_z, z_first, z_count, C.byref(setting) if setting is not None else None,
                                                out)

    assert call(src=None) == INVALID and call(out=None) == INVALID and call(setting=None) == INVALID and call(setting=bad) == INVALID
    assert call(dim_x=0) == INVALID and call(dim_y=0) == INVALID and call(z_count=0) == INVALID
    assert call(z_first=1, z_count=4) == INVALID and call(z_first=0xFFFFFFFF, z_count=2) == INVALID
    assert call(src=d_v.ptr + 2) == INVALID and call(out=dst.data_ptr() + 1) == INVALID
    assert call(out=d_v.ptr) == INVALID and call(out=d_v.ptr + 4 * (v.size - 1)) == INVALID                  # overlapping ranges
    assert call(src=dst.data_ptr() + 4 * v.size, z_first=3, z_count=1, out=dst.data_ptr() + 4 * (v.size - 1)) == INVALID
    assert be._L.paris_hip_volume_bilateral(None, d_v.ptr, 8, 3, 4, 0, 4, C.byref(good), dst.data_ptr()) != 0
    be.synchronize()
    assert (dst.cpu().numpy() == 7).all()           # nothing was written by a refused call
    assert call() == 0
    be.synchronize()
    assert same_bits(dst.cpu().numpy()[:v.size].view(np.float32).reshape(v.shape), B.volume_bilateral_host(v, 0.25, 1.0, 1))
    del keep
