"""paris.hip --denoise on the scene of tests/test_gpu_metal_driver.py against the Python chain -- the Backend
reconstruction of the whole volume, then Backend.volume_bilateral on it -- bit for bit: in one slab and in three with a remainder,
with drain chunks of one slice, on two devices where the machine has them, as u16 voxels over a given and an automatic window, after
the metal reinsertion and inside a region of interest. The report line, the refusals, and without --denoise the plain chain's volume."""
import re

import numpy as np
import pytest

import test_gpu_metal_driver as MD
import volume_window_rule as VW
from test_gpu_metal_driver import scan  # noqa: F401  (the fixture: the scene's inputs on disk)
from paris_amd import backend as B

pytestmark = pytest.mark.gpu

VG = MD.VG
SETTING = (0.05, 1.25, 2)      # sigma_r: half the soft tissue's value in the volume's units
DENOISE = "%.9g:%.9g:%d" % SETTING
LINE = re.compile(r"^denoising on: 3-D bilateral filter, sigma_r (\S+), sigma_s (\S+) voxel\(s\), radius (\d) \((\d+) taps\), (\d) halo slice\(s\) per slab side$",
                  re.M)
bits = MD.bits


def denoised(volume, setting=SETTING):
    """Backend.volume_bilateral on a whole volume: the second half of the Python chain"""
    with B.Backend(0) as be:
        dz, dy, dx = volume.shape
        d_v = be.make_volume_device(dx, dy, dz)
        be.copy_h2d(B.Volume(np.ascontiguousarray(volume, np.float32), dx, dy, dz), d_v)
        be.set_volume_bilateral(*setting)
        d_o = be.volume_bilateral(d_v)
        h = be.make_volume_host(dx, dy, dz)
        be.copy_d2h(d_o, h)
        return h.buf.reshape(dz, dy, dx).copy()


@pytest.fixture(scope="module")
def plain(scan):  # noqa: F811
    v = MD.python_chain(scan[1], False)[0]
    v.setflags(write=False)
    return v


@pytest.fixture(scope="module")
def want(plain):
    v = denoised(plain)
    assert not np.array_equal(bits(v), bits(plain)) and np.isfinite(v).all()
    assert np.array_equal(bits(v), bits(B.volume_bilateral_host(plain, *SETTING)))     # the device filter is the rule's
    v.setflags(write=False)
    return v


FORMS = {"slabs_1": ["--slabs", 1], "slabs_3": ["--slabs", 3], "slabs_32": ["--slabs", 32], "chunk_of_one_slice": ["--slabs", 2, "--drain-chunk-kib", 1],
         "one_volume": ["--slabs", 3, "--one-volume"], "no_row_band": ["--slabs", 3, "--no-row-band"], "devices": None}


@pytest.mark.parametrize("form", sorted(FORMS))
def test_denoise_equals_the_python_chain(scan, want, form):  # noqa: F811
    """three slabs of the 32 slices are 10, 10 and 12: a remainder slab; 32 slabs are all halo"""
    root, _ = scan
    extra = FORMS[form] if FORMS[form] is not None else ["--slabs", 4] + MD.two_devices()
    text = MD.drive(root, "dn_" + form, ["--denoise", DENOISE] + extra)
    got = MD.volume_of(root, "dn_" + form)
    assert got.shape == want.shape and np.array_equal(bits(got), bits(want)), form
    line = LINE.search(text)
    assert line, text
    assert (np.float32(line.group(1)), np.float32(line.group(2))) == (np.float32(SETTING[0]), np.float32(SETTING[1]))
    assert (int(line.group(3)), int(line.group(4)), int(line.group(5))) == (2, 125, 2)


def test_defaults(scan, plain):  # noqa: F811
    """SIGMA_S = 1 and RADIUS = min(3, ceil(2 SIGMA_S)) = 2; SIGMA_S = 1.75 gives 3, 0.4 gives 1"""
    root, _ = scan
    for spec, setting in [("0.05", (0.05, 1.0, 2)), ("0.05:1.75", (0.05, 1.75, 3)), ("0.05:0.4", (0.05, 0.4, 1))]:
        text = MD.drive(root, "dn_default", ["--denoise", spec, "--slabs", 3])
        assert int(LINE.search(text).group(3)) == setting[2], text
        assert np.array_equal(bits(MD.volume_of(root, "dn_default")), bits(denoised(plain, setting))), spec


def test_as_u16_voxels_over_a_given_window(scan, want):  # noqa: F811
    root, _ = scan
    lo, hi = -0.05, 0.4
    MD.drive(root, "dn_u16", ["--denoise", DENOISE, "--slabs", 3, "--voxel-type", "u16", "--voxel-range", "%.9g:%.9g" % (lo, hi)])
    header, got = VW.read_mhd(str(root / "dn_u16" / "vol.mhd"))
    assert got.dtype == np.uint16 and np.array_equal(got.ravel(), VW.quantize(want, lo, hi, np.uint16).ravel())
    assert not np.array_equal(got.ravel(), VW.quantize(MD.python_chain(scan[1], False)[0], lo, hi, np.uint16).ravel())


def test_the_automatic_window_sees_the_filtered_voxels(scan, want):  # noqa: F811
    root, _ = scan
    MD.drive(root, "dn_auto", ["--denoise", DENOISE, "--slabs", 1, "--devices", 1, "--drain-chunk-kib", 64, "--voxel-type", "u8", "--voxel-range", "auto"])
    header, got = VW.read_mhd(str(root / "dn_auto" / "vol.mhd"))
    with B.Backend(0) as be:
        d_v = be.make_volume_device(VG.dim_x, VG.dim_y, VG.dim_z)
        be.copy_h2d(B.Volume(np.ascontiguousarray(want), VG.dim_x, VG.dim_y, VG.dim_z), d_v)
        st, _ = be.volume_stats(d_v)
        st, hist = be.volume_stats(d_v, st.min, st.max, 4096)
        lo, hi = B.volume_window_from_histogram(hist, st.min, st.max, 0.1, 99.9)
        wanted = be.quantize_volume(d_v, lo, hi, np.uint8)
        be.free(d_v)
    assert got.dtype == np.uint8 and np.array_equal(got.ravel(), np.asarray(wanted).ravel())


def test_after_the_metal_reinsertion(scan):  # noqa: F811
    root, frames = scan
    metal = MD.python_chain(frames, True)[0]
    assert metal.max() > MD.THRESHOLD
    MD.drive(root, "dn_metal", ["--denoise", DENOISE, "--metal", MD.METAL, "--slabs", 3])
    assert np.array_equal(bits(MD.volume_of(root, "dn_metal")), bits(denoised(metal)))


def test_inside_a_region_of_interest(scan):  # noqa: F811
    """the grid is the region's: taps beyond its faces are skipped, though the volume continues there. The region's reconstruction is
    the driver's own without the option (held to the oracle by tests/test_gpu_paris_hip.py), filtered whole by the Backend."""
    root, _ = scan
    roi = ["--roi", "--roi-x1", 8, "--roi-x2", 53, "--roi-y1", 4, "--roi-y2", 36, "--roi-z1", 5, "--roi-z2", 28]
    MD.drive(root, "roi_plain", roi + ["--slabs", 1])
    region = MD.volume_of(root, "roi_plain")
    assert region.shape == (23, 32, 45)
    MD.drive(root, "dn_roi", roi + ["--denoise", DENOISE, "--slabs", 4])
    assert np.array_equal(bits(MD.volume_of(root, "dn_roi")), bits(denoised(region)))


def test_without_the_option_nothing_changes(scan, plain, want):  # noqa: F811
    root, _ = scan
    text = MD.drive(root, "dn_off", ["--slabs", 3])
    assert "denoising on" not in text
    assert np.array_equal(bits(MD.volume_of(root, "dn_off")), bits(plain))


@pytest.mark.parametrize("extra,words", [
    (["--denoise", "0"], "SIGMA_R must be finite and greater than 0"),
    (["--denoise", "-0.05"], "SIGMA_R must be finite and greater than 0"),
    (["--denoise", "nan:1"], "SIGMA_R must be finite and greater than 0"),
    (["--denoise", "inf"], "SIGMA_R must be finite and greater than 0"),
    (["--denoise", "0.05:0"], "SIGMA_S must be finite and greater than 0"),
    (["--denoise", "0.05:inf:2"], "SIGMA_S must be finite and greater than 0"),
    (["--denoise", "0.05:1:0"], "RADIUS must lie in 1 .. 3 (got 0)"),
    (["--denoise", "0.05:1:4"], "RADIUS must lie in 1 .. 3 (got 4)"),
    (["--denoise", "1e-37"], "SIGMA_R is too small for the range table"),
    (["--denoise", "0.05:1:2:9"], "cannot read '0.05:1:2:9'"),
    (["--denoise", "0.05:1:2.5"], "cannot read '0.05:1:2.5'"),
    (["--denoise", "soft"], "cannot read 'soft'"),
    (["--denoise", DENOISE, "--find-axis", "-1:1", "--axis-only"], "--denoise cannot be combined with --axis-only or --roll-only"),
    (["--denoise", DENOISE, "--find-roll", "-1:1", "--roll-only"], "--denoise cannot be combined with --axis-only or --roll-only"),
])
def test_refusals_come_before_any_output(scan, extra, words):  # noqa: F811
    root, _ = scan
    err = MD.drive(root, "dn_refused", extra, ok=False)
    assert words in err, err
    assert not (root / "dn_refused").exists()
