"""The kernels of the hot path against the float64 model of tests/fdk_model.py and against the phantom's own densities.

The other GPU tests compare with the CPU oracle, mostly bit for bit; tests/test_fdk_model_host.py pins that oracle to the model.
This file does not lean on that: every expected value here comes from the model (equations, float64) or from the phantom, on the
cases of tests/fdk_cases.py. The tolerances are the reference port's own float32 error against the model, recorded per case and
stage in tests/golden/fdk_model_bounds.json -- never anything a kernel gave:
  weight, backprojection (fed the same float32 input)  2 x the recorded error;
  filter, weight + filter, whole chain                  4 x the recorded error (the device FFT is ordered differently from the
                                                        oracle's radix-2, and float32 FFT error differs by a small factor
                                                        between orderings); tighter than the suite's FILTER_TOL of 1e-5.
Single views follow rule (b): a voxel whose ray passes within 1e-3 pixel of a validity limit may hold the value with that sample
zeroed, on at most 0.2 % of a volume's voxels.
"""
import numpy as np
import pytest

import fdk_cases as K
import fdk_model as M
from paris_amd import _lib
from paris_amd import backend as B

pytestmark = pytest.mark.gpu

SAME_INPUT, FFT = 2.0, 4.0


@pytest.fixture(scope="module")
def be():
    b = B.set_device(B.get_devices()[0])
    yield b
    b.close()


@pytest.fixture(scope="module")
def bounds(golden_dir):
    return K.load_bounds(golden_dir)


@pytest.fixture(scope="module")
def w_model():
    return K.WModel(B)


def to_device(be, host_array, idx=0, phi=0.0):
    h = B.Projection(np.ascontiguousarray(host_array, np.float32), host_array.shape[1], host_array.shape[0], idx, phi)
    return B.load(be, h)


def to_host(be, d_p):
    h = be.make_projection_host(d_p.dim_x, d_p.dim_y)
    be.copy_d2h(d_p, h)
    return h.buf


def volume_to_host(be, d_v):
    h = be.make_volume_host(d_v.dim_x, d_v.dim_y, d_v.dim_z)
    be.copy_d2h(d_v, h)
    return h.buf


def product_refuses(call, *args):
    """What lost its A/B runs is compiled into the experiments build only (tests/test_gpu_experiments_build.py runs this file's
    variant tests against it); the product library must answer PARIS_HIP_ERROR_UNSUPPORTED, and then there is nothing more to test."""
    if _lib.has_experiments():
        return False
    with pytest.raises(_lib.ParisHipError) as e:
        call(*args)
    assert e.value.status == _lib.ERROR_UNSUPPORTED
    return True


def detector(case):
    return B.DetectorGeometry(*{"f97": K.F_DETECTOR, "w": K.W_DETECTOR, **K.V_DETECTORS}[case])


def report(what, err, bound, factor, share=None):
    print("%s: %.3g of the model's maximum (allowed %g x %.3g)%s" % (what, err, factor, bound,
                                                                     "" if share is None else ", boundary rule on %.4f %%" % (100 * share)))
    return err <= factor * bound and (share is None or share <= K.BOUNDARY_SHARE)


# ---- weight -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["v61", "v64", "w"])
def test_weight_against_the_model(be, bounds, case):
    det = detector(case)
    bound = bounds[case]["weight"]["error"]
    frames = [K.v_projection(det.n_row, det.n_col)] if case != "w" else [K.w_frames(B.calculate_volume_geometry(det))[i]
                                                                         for i in K.W_SAMPLED]
    ok = True
    for n, raw in enumerate(frames):
        want = M.weight(raw, det)
        d_p = to_device(be, raw)
        B.weight(be, d_p, det)
        ok &= report("%s view %d, whole frame" % (case, n), K.rel_err(to_host(be, d_p), want), bound, SAME_INPUT)
        be.free(d_p)
        first, count = 6, 21            # a row band: rows outside it stay as they were
        d_q = to_device(be, raw)
        B.weight_rows(be, d_q, det, first, count)
        band = to_host(be, d_q)
        be.free(d_q)
        err = float(np.abs(band[first:first + count] - want[first:first + count]).max() / np.abs(want).max())
        ok &= report("%s view %d, rows %d..%d" % (case, n, first, first + count - 1), err, bound, SAME_INPUT)
        assert np.array_equal(band[:first], raw[:first]) and np.array_equal(band[first + count:], raw[first + count:])
    assert ok


# ---- filter -----------------------------------------------------------------------------------------------------------

def filter_inputs(case, det):
    """what tests/fdk_cases.py fed the oracle's filter when its error was recorded"""
    if case != "w":
        return [K.v_projection(det.n_row, det.n_col)]
    raws = K.w_frames(B.calculate_volume_geometry(det))
    return [K.staged_inputs(det, raws[i])[0] for i in K.W_SAMPLED]


@pytest.mark.parametrize("variant", [0, 1, 2])
@pytest.mark.parametrize("case", ["v61", "v64", "f97", "w"])
def test_filter_against_the_model(be, bounds, case, variant):
    det = detector(case)
    assert det.n_row == {"v61": 61, "v64": 64, "f97": 97, "w": 128}[case]
    if variant == 2 and product_refuses(be.set_filter_variant, 2):
        return
    fs = B.filter_size(det.n_row)
    k = be.make_filter(fs, det.l_px_row)
    ok = True
    be.set_filter_variant(variant)
    try:
        for n, x in enumerate(filter_inputs(case, det)):
            d_p = to_device(be, x)
            be.apply_filter(d_p, k, fs, det.n_col)
            ok &= report("%s input %d, variant %d" % (case, n, variant), K.rel_err(to_host(be, d_p), M.ramp(x, det.l_px_row)),
                         bounds[case]["filter"]["error"], FFT)
            be.free(d_p)
    finally:
        be.set_filter_variant(0)
        be.free(k)
    assert ok


@pytest.mark.parametrize("case", ["v61", "v64", "f97", "w"])
def test_fused_weight_and_filter_against_the_model(be, bounds, case):
    """weighting riding along in the row filter's load, one launch: the stage wrapper on the whole frame, and the pair of stage
    calls (B.filter after B.weight) it has to equal within the same bound"""
    det = detector(case)
    raws = [K.v_projection(det.n_row, det.n_col)] if case != "w" else [K.w_frames(B.calculate_volume_geometry(det))[i]
                                                                       for i in K.W_SAMPLED]
    ok = True
    for n, raw in enumerate(raws):
        want = M.ramp(M.weight(raw, det), det.l_px_row)
        d_p = to_device(be, raw)
        B.weight_filter_rows(be, d_p, det, 0, det.n_col)
        ok &= report("%s view %d, one launch" % (case, n), K.rel_err(to_host(be, d_p), want), bounds[case]["weight_filter"]["error"], FFT)
        be.free(d_p)
        d_q = to_device(be, raw)
        B.weight(be, d_q, det)
        B.filter(be, d_q, det)
        ok &= report("%s view %d, two stages" % (case, n), K.rel_err(to_host(be, d_q), want), bounds[case]["weight_filter"]["error"], FFT)
        be.free(d_q)
    assert ok


# ---- backprojection: case V, every voxel ----------------------------------------------------------------------------------

def single_view(be, det, place, raw, phi):
    """one view through paris::backproject with the angle as an angle-file value, into a fresh array"""
    dz, dy, dx = place.dims
    d_v = be.make_volume_device(dx, dy, dz)
    d_p = to_device(be, raw, phi=phi)
    B.backproject(be, d_p, d_v, place.v_offset, det, place.vol_geo, True, place.roi is not None, place.roi)
    be.free(d_p)
    out = volume_to_host(be, d_v)
    be.free(d_v)
    return out


def check_single_views(be, bounds, name, vol, run):
    det = detector(name)
    place = K.v_placement(B, det, vol)
    raw = K.v_projection(det.n_row, det.n_col)
    ok = True
    for phi in K.V_ANGLES:
        err, share = K.v_view(B, name, vol, phi).compare(run(det, place, raw, phi))
        ok &= report("%s %s at %g degrees" % (name, vol, phi), err, bounds[name]["backproject_" + vol]["error"], SAME_INPUT, share)
    assert ok


@pytest.mark.parametrize("vol", K.V_VOLUMES)
@pytest.mark.parametrize("name", list(K.V_DETECTORS))
@pytest.mark.parametrize("variant", [0, 1, 2, 3, 4])
def test_backproject_kernel_variants_against_the_model(be, bounds, variant, name, vol):
    if variant == 3 and product_refuses(be.set_backproject_variant, 3):   # the slice kernel: experiments build only
        return
    be.set_backproject_variant(variant)
    try:
        check_single_views(be, bounds, name, vol, lambda *a: single_view(be, *a))
    finally:
        be.set_backproject_variant(0)


@pytest.mark.parametrize("vol", K.V_VOLUMES)
@pytest.mark.parametrize("name", list(K.V_DETECTORS))
@pytest.mark.parametrize("vector", [False, True])
def test_backproject_detector_staging_against_the_model(be, bounds, vector, name, vol):
    """4-pixel and 1-pixel staging of the detector box (61-pixel rows cannot take whole 16-byte lanes, 64-pixel rows can)"""
    be.set_backproject_vector_staging(vector)
    try:
        check_single_views(be, bounds, name, vol, lambda *a: single_view(be, *a))
    finally:
        be.set_backproject_vector_staging(True)


@pytest.mark.parametrize("vol", K.V_VOLUMES)
@pytest.mark.parametrize("name", list(K.V_DETECTORS))
def test_backproject_f16_against_the_model(be, bounds, name, vol):
    """paris_hip_backproject_f16: the model is fed the projection rounded through np.float16; the same 2 x bound"""
    det = detector(name)
    place = K.v_placement(B, det, vol)
    raw = K.v_projection(det.n_row, det.n_col)
    rounded = raw.astype(np.float16).astype(np.float32)
    assert not np.array_equal(rounded, raw)
    dz, dy, dx = place.dims
    ok = True
    for phi in K.V_ANGLES:
        d_v = be.make_volume_device(dx, dy, dz)
        d_p = to_device(be, raw)
        h_ptr, h_pitch = be.convert_projection_f16(d_p)
        s, c = B.stage_angle(det, 0, True, phi)
        be.backproject_f16(h_ptr, h_pitch, det.n_row, det.n_col, d_v, place.v_offset, det, place.vol_geo, place.roi is not None, place.roi,
                           s, c, det.delta_s * det.l_px_row, det.delta_t * det.l_px_col)
        be.free(h_ptr)
        be.free(d_p)
        got = volume_to_host(be, d_v)
        be.free(d_v)
        err, share = K.ViewSum(det, place, [rounded], [phi]).compare(got)
        ok &= report("%s %s at %g degrees, half frames" % (name, vol, phi), err, bounds[name]["backproject_" + vol]["error"], SAME_INPUT, share)
    assert ok


@pytest.mark.parametrize("vol", K.V_VOLUMES)
@pytest.mark.parametrize("name", list(K.V_DETECTORS))
def test_backproject_batch_against_the_models_sum(be, bounds, name, vol):
    """paris_hip_backproject_batch: three of the angles in one fused launch"""
    det = detector(name)
    place = K.v_placement(B, det, vol)
    raw = K.v_projection(det.n_row, det.n_col)
    n, rows, cols = len(K.V_BATCH_ANGLES), det.n_col, det.n_row
    stack = be.make_projection_device(cols, rows * n)
    be.copy_h2d(B.Projection(np.ascontiguousarray(np.concatenate([raw] * n)), cols, rows * n), stack)
    sc = [B.stage_angle(det, 0, True, phi) for phi in K.V_BATCH_ANGLES]
    dz, dy, dx = place.dims
    d_v = be.make_volume_device(dx, dy, dz)
    be.backproject_batch(stack.ptr, stack.pitch, stack.pitch * rows, n, cols, rows, d_v, place.v_offset, det, place.vol_geo,
                         place.roi is not None, place.roi, [s for s, _ in sc], [c for _, c in sc], det.delta_s * det.l_px_row,
                         det.delta_t * det.l_px_col)
    got = volume_to_host(be, d_v)
    be.free(d_v)
    be.free(stack)
    err, share = K.v_sum(B, name, vol, K.V_BATCH_ANGLES).compare(got)
    assert report("%s %s, 3 views in one launch" % (name, vol), err, bounds[name]["backproject_sum3_" + vol]["error"], SAME_INPUT, share)


@pytest.mark.parametrize("vol", K.V_VOLUMES)
@pytest.mark.parametrize("name", list(K.V_DETECTORS))
def test_backproject_product_loop_against_the_models_sum(bounds, name, vol):
    """The product path (Backend.set_paris_loop_defaults(48)): a buffer per view, backprojected by reference and freed, the nine
    views pending until the flush"""
    det = detector(name)
    place = K.v_placement(B, det, vol)
    raw = K.v_projection(det.n_row, det.n_col)
    dz, dy, dx = place.dims
    with B.Backend(0, synchronous=False) as abe:
        abe.set_paris_loop_defaults(48)
        d_v = abe.make_volume_device(dx, dy, dz)
        for phi in K.V_ANGLES:
            d_p = to_device(abe, raw, phi=phi)
            B.backproject(abe, d_p, d_v, place.v_offset, det, place.vol_geo, True, place.roi is not None, place.roi)
            abe.free(d_p)
        abe.flush()
        got = volume_to_host(abe, d_v)
    err, share = K.v_sum(B, name, vol, K.V_ANGLES).compare(got)
    assert report("%s %s, 9 views by reference" % (name, vol), err, bounds[name]["backproject_sum9_" + vol]["error"], SAME_INPUT, share)


# ---- case W: the whole circle -----------------------------------------------------------------------------------------------

def check_w_volume(w, vol, bound, factor, model):
    err, share = model.compare(vol[w.zs])
    ok = report("case W, slices %s" % w.zs, err, bound, factor, share)
    boxes = [K.crop(vol, ball).astype(np.float64) / w.scale for ball in K.w_balls(w.vol_geo)]
    for mean, want, centroid in K.truth_figures(boxes, w.vol_geo):
        print("inner mean %.5f (phantom %.2f), centroid error (x, y, z) = (%.4f, %.4f, %.4f) voxels" % ((mean, want) + centroid))
    return ok, K.truth_problems(boxes, w.vol_geo)


def test_whole_circle_backprojection_against_the_model(be, bounds, w_model):
    """the model's filtered views, rounded to float32, through B.backproject by index: six slices against the model's"""
    w = w_model
    dx, dy, dz = K.W_NATURAL
    d_v = be.make_volume_device(dx, dy, dz)
    for i, f in enumerate(w.staged):
        d_p = to_device(be, f, idx=i)
        B.backproject(be, d_p, d_v, 0, w.det, w.vol_geo, False, False, None)
        be.free(d_p)
    vol = volume_to_host(be, d_v)
    be.free(d_v)
    ok, problems = check_w_volume(w, vol, bounds["w"]["backproject"]["error"], SAME_INPUT, w.staged_slices)
    assert ok and not problems, problems


@pytest.mark.parametrize("path", ["plain", "product"])
def test_whole_circle_chain_against_the_model_and_the_phantom(be, bounds, w_model, path):
    """raw views through B.weight, B.filter and B.backproject, one launch per call and on the product path: the six slices against
    the model's chain, and the volume itself against the phantom -- density to 0.5 % inside each ball, centroids to 0.1 voxel"""
    w = w_model
    dx, dy, dz = K.W_NATURAL

    def loop(b):
        d_v = b.make_volume_device(dx, dy, dz)
        for i, raw in enumerate(w.raw):
            d_p = to_device(b, raw, idx=i)
            B.weight(b, d_p, w.det)
            B.filter(b, d_p, w.det)
            B.backproject(b, d_p, d_v, 0, w.det, w.vol_geo, False, False, None)
            b.free(d_p)
        return d_v

    if path == "plain":
        d_v = loop(be)
        vol = volume_to_host(be, d_v)
        be.free(d_v)
    else:
        with B.Backend(0, synchronous=False) as abe:
            abe.set_paris_loop_defaults(48)
            d_v = loop(abe)
            abe.flush()
            vol = volume_to_host(abe, d_v)
    ok, problems = check_w_volume(w, vol, bounds["w"]["chain"]["error"], FFT, w.slices)
    assert ok and not problems, problems
