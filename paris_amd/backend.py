"""Host-side mirror of the PARIS backend surface for the MI355X HIP backend.

The reference's backend is a C++ namespace with 14 free functions plus buffer types
(src/generic/backend.h:54-88, src/openmp/backend.h:42-89, src/cuda/backend.h:50-103). This module exposes
the same names, argument meaning and error behaviour over the C ABI of include/paris_hip.h, so the parity
tests read like a PARIS driver loop (src/main.cpp:98-105). The C++ equivalent is paris_amd/host/.

All numeric work happens in libparis_hip.so on the GPU; there is no CPU path here.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import (StarvationFilter, StarvationCounts, VolumeBilateral, ScatterCorrection, PhaseRetrieval, BeamHardening, BhCounts, BhFit, LagModel, MetalCounts, DetectorRoll, RollSearch, RollResult, AirCounts, AirRegion, AxisEntry, AxisResult, AxisSearch, Binning, DefectStats, DetectorGeometry, ParisHipError, RegionOfInterest, RingFilter, RingStats, RowExtension, ShortScan,
                   SubvolumeGeometry, SubvolumeInfo, VolumeCounts, VolumeGeometry, VolumeStatistics, VolumeWindow, ZingerCounts,
                   ZingerFilter, check)

__all__ = ["DetectorGeometry", "VolumeGeometry", "SubvolumeGeometry", "RegionOfInterest", "SubvolumeInfo",
           "ParisHipError", "ShortScan", "Projection", "Volume", "FilterBuffer", "Backend", "get_devices", "set_device",
           "calculate_volume_geometry", "apply_roi", "filter_size", "load", "make_volume", "weight", "filter",
           "backproject", "forward_project", "short_scan_check", "offset_detector_check", "DefectPlan", "defect_plan",
           "ZingerFilter", "zinger_filter_check", "RowExtension", "row_extension_check", "row_extension_response",
           "RingFilter", "RingStats", "ring_filter_check", "ring_correction_from_mean", "VolumeWindow", "VolumeCounts",
           "VolumeStatistics", "VolumeBilateral", "volume_bilateral_check", "volume_bilateral_tables", "volume_bilateral_host",
           "volume_window_check", "volume_window_from_histogram", "Binning", "binning_check",
           "binned_geometry", "bin_frame_host", "bin_mask", "AirRegion", "AirCounts", "air_region_check", "air_value_host",
           "BeamHardening", "BhCounts", "BhFit", "Labels", "BeamHardeningFit", "beam_hardening_check", "beam_hardening_host",
           "bh_threshold_from_histogram", "bh_gram_host", "bh_gram_matrix", "bh_solve", "DetectorRoll", "RollSearch", "RollResult",
           "detector_roll_check", "detector_roll_host", "detector_roll_source_rows", "roll_search_check", "roll_estimate_from_costs",
           "LagModel", "lag_model_check", "lag_coefficients", "lag_correct_host", "MetalCounts", "MetalTrace", "metal_check",
           "metal_collect_host", "metal_trace_pack_host", "metal_inpaint_host", "metal_words", "PhaseRetrieval", "phase_alpha",
           "phase_default_margin", "phase_retrieval_check", "phase_retrieval_host", "ScatterCorrection", "scatter_default_margin",
           "scatter_correction_check", "scatter_correction_host", "StarvationFilter", "StarvationCounts", "starvation_filter_check",
           "starvation_filter_tables", "starvation_filter_host"]


class Projection:
    """paris::projection<Buffer, Metadata> (src/projection.h:31-46). `buf` is a numpy array (host) or a device
    address (device); `pitch` is the row stride in bytes."""

    def __init__(self, buf, dim_x, dim_y, idx=0, phi=0.0, pitch=None, on_device=False, owner=None):
        self.buf = buf
        self.dim_x = dim_x
        self.dim_y = dim_y
        self.idx = idx
        self.phi = phi
        self.pitch = pitch if pitch is not None else dim_x * 4
        self.on_device = on_device
        self._owner = owner  # Backend that must free buf, or an object that keeps it alive

    @property
    def ptr(self):
        return self.buf if self.on_device else self.buf.ctypes.data


class Volume:
    """paris::volume<Buffer> (src/volume.h:31-45); x fastest, then y, then z."""

    def __init__(self, buf, dim_x, dim_y, dim_z, off=0, on_device=False, owner=None):
        self.buf = buf
        self.dim_x = dim_x
        self.dim_y = dim_y
        self.dim_z = dim_z
        self.off = off
        self.on_device = on_device
        self._owner = owner

    @property
    def ptr(self):
        return self.buf if self.on_device else self.buf.ctypes.data


class FilterBuffer:
    """backend::filter_buffer_type: K = tau * |rFFT(r)|, size/2+1 floats on the device."""

    def __init__(self, ptr, size, backend):
        self.ptr = ptr
        self.size = size
        self._backend = backend


class DefectPlan:
    """The repair plan of a defect map (paris_hip_defect_plan_*), as numpy arrays: defect[n] the linear index y * dim_x + x of every
    repairable defect, sorted row-major; first_source[n + 1]; source[m] and weight[m] (float32), defect k's at
    [first_source[k], first_source[k + 1]). The counts of paris_hip_defect_stats are attributes."""

    def __init__(self, stats, defect, first_source, source, weight):
        self.defects = int(stats.defects)
        self.unrepairable = int(stats.unrepairable)
        self.sources = int(stats.sources)
        self.reach_rows = int(stats.reach_rows)
        self.reach_cols = int(stats.reach_cols)
        self.device_bytes = int(stats.device_bytes)
        self.defect = defect
        self.first_source = first_source
        self.source = source
        self.weight = weight


def _mask_bytes(mask, what):
    m = np.ascontiguousarray(np.asarray(mask) != 0, np.uint8)
    if m.ndim != 2:
        raise ValueError("%s: the defect map must be a 2-D array (n_col, n_row)" % what)
    return m


def defect_plan(mask):
    """Host only, no device: the repair plan of a defect map -- a 2-D array of the detector's size (n_col, n_row), nonzero = defective
    (paris_hip_defect_plan_create). Returns a DefectPlan."""
    m = _mask_bytes(mask, "defect_plan")
    L = _lib.load()
    plan = C.c_void_p()
    check(L.paris_hip_defect_plan_create(m.ctypes.data, m.shape[1], m.shape[0], C.byref(plan)), "paris_hip_defect_plan_create")
    try:
        st = DefectStats()
        check(L.paris_hip_defect_plan_stats(plan, C.byref(st)), "paris_hip_defect_plan_stats")
        n = int(st.defects - st.unrepairable)
        defect, first = np.empty(n, np.uint32), np.empty(n + 1, np.uint32)
        source, weight = np.empty(int(st.sources), np.uint32), np.empty(int(st.sources), np.float32)
        check(L.paris_hip_defect_plan_copy(plan, defect.ctypes.data, first.ctypes.data, source.ctypes.data, weight.ctypes.data),
              "paris_hip_defect_plan_copy")
    finally:
        L.paris_hip_defect_plan_destroy(plan)
    return DefectPlan(st, defect, first, source, weight)


_POLARITIES = {"bright": 1, "dark": -1, "both": 0}


def _zinger_setting(threshold_abs, threshold_rel, polarity, max_hits):
    return ZingerFilter(threshold_abs, threshold_rel, _POLARITIES.get(polarity, polarity), max_hits)


def zinger_filter_check(threshold_abs, threshold_rel, polarity, max_hits, dim_x, dim_y):
    """Host only, no device (paris_hip_zinger_filter_check): checks a zinger-filter setting for a dim_x x dim_y detector -- polarity
    +1 / "bright", -1 / "dark" or 0 / "both"; max_hits 0 = default -- and returns (max_hits resolved, device_bytes). Raises
    ParisHipError for a setting the library refuses."""
    L = _lib.load()
    hits, nbytes = C.c_uint32(0), C.c_size_t(0)
    zf = _zinger_setting(threshold_abs, threshold_rel, polarity, max_hits)
    check(L.paris_hip_zinger_filter_check(C.byref(zf), dim_x, dim_y, C.byref(hits), C.byref(nbytes)), "paris_hip_zinger_filter_check")
    return hits.value, nbytes.value


def ring_filter_check(half_width, floor_abs, limit_abs, dim_x, dim_y):
    """Host only, no device (paris_hip_ring_filter_check): checks a ring-filter setting for a dim_x x dim_y detector -- half_width in
    [1, 32], floor_abs >= 0, limit_abs 0 (none) or above floor_abs -- and returns (profile_bytes, correction_bytes). Raises
    ParisHipError for a setting the library refuses."""
    rf = RingFilter(half_width, floor_abs, limit_abs)
    profile, correction = C.c_size_t(0), C.c_size_t(0)
    check(_lib.load().paris_hip_ring_filter_check(C.byref(rf), dim_x, dim_y, C.byref(profile), C.byref(correction)),
          "paris_hip_ring_filter_check")
    return profile.value, correction.value


def ring_correction_from_mean(half_width, floor_abs, limit_abs, mean, count_per_row=None):
    """Host only, no device (paris_hip_ring_correction_from_mean): the ring rule from a scan's mean frame, a 2-D array of the
    detector's size (n_col, n_row) taken as float32, to (c, RingStats) -- c the stationary offset to subtract from every frame, 0
    where the rule keeps none. count_per_row: how many frames each row's mean holds (rows with 0 get
    c = 0); None = every row present."""
    m = np.ascontiguousarray(mean, np.float32)
    if m.ndim != 2:
        raise ValueError("ring_correction_from_mean: the mean must be a 2-D array (n_col, n_row)")
    counts = None if count_per_row is None else np.ascontiguousarray(count_per_row, np.uint32)
    if counts is not None and counts.shape != (m.shape[0],):
        raise ValueError("ring_correction_from_mean: count_per_row must hold one count per detector row")
    rf = RingFilter(half_width, floor_abs, limit_abs)
    c, st = np.empty(m.shape, np.float32), RingStats()
    check(_lib.load().paris_hip_ring_correction_from_mean(C.byref(rf), m.ctypes.data, None if counts is None else counts.ctypes.data,
                                                          m.shape[1], m.shape[0], c.ctypes.data, C.byref(st)),
          "paris_hip_ring_correction_from_mean")
    return c, st


def _axis_setting(lo, step, count, rows=2, min_columns=0):
    return AxisSearch(lo, step, count, rows, min_columns)


def axis_search_check(lo, step, count, det_geo, n_frames, rows=2, min_columns=0):
    """Host only, no device (paris_hip_axis_search_check): checks an axis search -- `count` candidates lo, lo + step, ... for delta_s in
    detector pixels, `rows` detector rows summed into the mid-plane line -- for det_geo's detector and a full circle of n_frames
    frames, and returns (row_first, device_bytes). Raises ParisHipError for what the library refuses."""
    s, first, nbytes = _axis_setting(lo, step, count, rows, min_columns), C.c_uint32(0), C.c_size_t(0)
    check(_lib.load().paris_hip_axis_search_check(C.byref(s), C.byref(det_geo), n_frames, C.byref(first), C.byref(nbytes)),
          "paris_hip_axis_search_check")
    return first.value, nbytes.value


def axis_search_plan(lo, step, count, det_geo, n_frames, k, rows=2, min_columns=0):
    """Host only, no device (paris_hip_axis_search_plan): candidate k's plan as a structured array of n_row entries with the fields
    i0 (-1: no conjugate on the detector), k0, wi and wf."""
    s = _axis_setting(lo, step, count, rows, min_columns)
    entries = np.empty(det_geo.n_row, np.dtype([("i0", np.int32), ("k0", np.uint32), ("wi", np.float32), ("wf", np.float32)]))
    check(_lib.load().paris_hip_axis_search_plan(C.byref(s), C.byref(det_geo), n_frames, k, entries.ctypes.data), "paris_hip_axis_search_plan")
    return entries


def axis_estimate_from_costs(lo, step, cost, columns=None):
    """Host only, no device (paris_hip_axis_estimate_from_costs): the estimate from one cost per candidate lo, lo + step, ... --
    +inf marks an unscored candidate. Returns the AxisResult: delta_s, best, cost_min, cost_median, scored, columns, at_edge."""
    j = np.ascontiguousarray(cost, np.float64)
    if j.ndim != 1:
        raise ValueError("axis_estimate_from_costs: one cost per candidate")
    cols = None if columns is None else np.ascontiguousarray(columns, np.uint32)
    if cols is not None and cols.shape != j.shape:
        raise ValueError("axis_estimate_from_costs: one column count per candidate")
    s, out = _axis_setting(lo, step, j.size), AxisResult()
    check(_lib.load().paris_hip_axis_estimate_from_costs(C.byref(s), j.ctypes.data, None if cols is None else cols.ctypes.data, C.byref(out)),
          "paris_hip_axis_estimate_from_costs")
    return out


def binning_check(bin_x, bin_y, dim_x, dim_y):
    """Host only, no device (paris_hip_binning_check): checks detector binning by bin_x x bin_y, each 1, 2, 4 or 8, for a dim_x x dim_y
    detector and returns the binned size (out_x, out_y). Raises ParisHipError for a setting the library refuses."""
    bn = Binning(bin_x, bin_y)
    ox, oy = C.c_uint32(0), C.c_uint32(0)
    check(_lib.load().paris_hip_binning_check(C.byref(bn), dim_x, dim_y, C.byref(ox), C.byref(oy)), "paris_hip_binning_check")
    return ox.value, oy.value


def binned_geometry(bin_x, bin_y, det_geo):
    """Host only, no device (paris_hip_binned_geometry): the DetectorGeometry of det_geo's detector binned by bin_x x bin_y -- the
    pixel pitches scaled, the offsets chosen so that the dropped remainder does not shift the rotation axis."""
    bn, out = Binning(bin_x, bin_y), DetectorGeometry()
    check(_lib.load().paris_hip_binned_geometry(C.byref(bn), C.byref(det_geo), C.byref(out)), "paris_hip_binned_geometry")
    return out


def bin_frame_host(bin_x, bin_y, frame, mask=None):
    """Host only, no device (paris_hip_bin_frame_host): the binning rule on a 2-D array of the detector's size (n_col, n_row), taken as
    float32 -- every binned pixel the mean of its good source pixels, summed row-major in fp32, +0 without one. mask: the same
    shape, nonzero = bad; None = every pixel good. For dark and flat frames."""
    a = np.ascontiguousarray(frame, np.float32)
    if a.ndim != 2:
        raise ValueError("bin_frame_host: the frame must be a 2-D array (n_col, n_row)")
    m = None if mask is None else _mask_bytes(mask, "bin_frame_host")
    if m is not None and m.shape != a.shape:
        raise ValueError("bin_frame_host: frame and mask differ in shape")
    ox, oy = binning_check(bin_x, bin_y, a.shape[1], a.shape[0])
    bn, out = Binning(bin_x, bin_y), np.empty((oy, ox), np.float32)
    check(_lib.load().paris_hip_bin_frame_host(C.byref(bn), None if m is None else m.ctypes.data, a.ctypes.data, a.shape[1], a.shape[0],
                                               out.ctypes.data), "paris_hip_bin_frame_host")
    return out


def bin_mask(bin_x, bin_y, mask):
    """Host only, no device (paris_hip_bin_mask): the binned mask, uint8 0 / 1 -- 1 where no source pixel of the bin is good. Hand it
    to set_defect_map() at binned size."""
    m = _mask_bytes(mask, "bin_mask")
    ox, oy = binning_check(bin_x, bin_y, m.shape[1], m.shape[0])
    bn, out = Binning(bin_x, bin_y), np.empty((oy, ox), np.uint8)
    check(_lib.load().paris_hip_bin_mask(C.byref(bn), m.ctypes.data, m.shape[1], m.shape[0], out.ctypes.data), "paris_hip_bin_mask")
    return out


def detector_roll_check(eta_deg, det_geo):
    """Host only, no device (paris_hip_detector_roll_check): raises ParisHipError unless eta_deg is finite, nonzero and at most 10 in
    magnitude and det_geo describes a detector of at least 2 x 2 pixels with positive pixel sizes and finite offsets."""
    s = DetectorRoll(eta_deg)
    check(_lib.load().paris_hip_detector_roll_check(C.byref(s), C.byref(det_geo)), "paris_hip_detector_roll_check")


def detector_roll_host(eta_deg, det_geo, frame):
    """Host only, no device (paris_hip_detector_roll_host): the roll rule on a 2-D array of the detector's size (n_col, n_row), taken
    as float32 -- the frame resampled bilinearly, edge replicated, onto a detector rotated back by eta_deg about the projected axis
    (DESIGN.md section 4.19). Returns a float32 array of the same shape."""
    f = np.ascontiguousarray(frame, np.float32)
    if f.shape != (det_geo.n_col, det_geo.n_row):
        raise ValueError("detector_roll_host: the frame must have the detector's size (n_col, n_row)")
    s, out = DetectorRoll(eta_deg), np.empty_like(f)
    check(_lib.load().paris_hip_detector_roll_host(C.byref(s), C.byref(det_geo), f.ctypes.data, out.ctypes.data), "paris_hip_detector_roll_host")
    return out


def detector_roll_source_rows(eta_deg, det_geo, row_first, row_count):
    """Host only, no device (paris_hip_detector_roll_source_rows): (first, count) of the source rows that destination rows
    [row_first, row_first + row_count) read."""
    s, first, count = DetectorRoll(eta_deg), C.c_uint32(0), C.c_uint32(0)
    check(_lib.load().paris_hip_detector_roll_source_rows(C.byref(s), C.byref(det_geo), row_first, row_count, C.byref(first), C.byref(count)),
          "paris_hip_detector_roll_source_rows")
    return first.value, count.value


def roll_search_check(lo, step, count, det_geo, min_pixels=0):
    """Host only, no device (paris_hip_roll_search_check): checks a roll search -- candidates (float)(lo + k step) degrees, k < count
    <= 256, each nonzero one a valid roll -- for det_geo's detector and returns (margin_x, margin_y, device_bytes)."""
    s, mx, my, nbytes = RollSearch(lo, step, count, min_pixels), C.c_uint32(0), C.c_uint32(0), C.c_size_t(0)
    check(_lib.load().paris_hip_roll_search_check(C.byref(s), C.byref(det_geo), C.byref(mx), C.byref(my), C.byref(nbytes)),
          "paris_hip_roll_search_check")
    return mx.value, my.value, nbytes.value


def roll_estimate_from_costs(lo, step, cost):
    """Host only, no device (paris_hip_roll_estimate_from_costs): the estimate from one cost per candidate -- the smallest scored
    (finite) one, refined by the parabola through its neighbours; the rule of the axis search. Returns the RollResult."""
    j = np.ascontiguousarray(cost, np.float64)
    s, out = RollSearch(lo, step, j.size, 0), RollResult()
    check(_lib.load().paris_hip_roll_estimate_from_costs(C.byref(s), j.ctypes.data, C.byref(out)), "paris_hip_roll_estimate_from_costs")
    return out


def _air_setting(x0, y0, width, height, min_pixels=0, limit_abs=0.0):
    return AirRegion(x0, y0, width, height, min_pixels, limit_abs)


def air_region_check(x0, y0, width, height, dim_x, dim_y, min_pixels=0, limit_abs=0.0):
    """Host only, no device (paris_hip_air_region_check): checks an air region -- columns [x0, x0 + width), rows [y0, y0 + height) of a
    dim_x x dim_y frame, at most 2^20 pixels; min_pixels 0 = half of them, rounded up; limit_abs 0 = no limit -- and returns
    (min_pixels resolved, device_bytes). Raises ParisHipError for a setting the library refuses."""
    ar, least, nbytes = _air_setting(x0, y0, width, height, min_pixels, limit_abs), C.c_uint32(0), C.c_size_t(0)
    check(_lib.load().paris_hip_air_region_check(C.byref(ar), dim_x, dim_y, C.byref(least), C.byref(nbytes)), "paris_hip_air_region_check")
    return least.value, nbytes.value


def air_value_host(x0, y0, width, height, frame, mask=None, min_pixels=0, limit_abs=0.0):
    """Host only, no device (paris_hip_air_value_host): the air rule on a 2-D array of the detector's size (n_col, n_row), taken as
    float32 -- the mean of the rectangle's counting pixels (mask byte 0, value finite), summed in double through 256 partial sums in
    the order DESIGN.md section 4.16 fixes, +0 with fewer than min_pixels of them or beyond limit_abs. Returns (a as np.float32, n)."""
    f = np.ascontiguousarray(frame, np.float32)
    if f.ndim != 2:
        raise ValueError("air_value_host: the frame must be a 2-D array (n_col, n_row)")
    m = None if mask is None else _mask_bytes(mask, "air_value_host")
    if m is not None and m.shape != f.shape:
        raise ValueError("air_value_host: frame and mask differ in shape")
    ar, a, n = _air_setting(x0, y0, width, height, min_pixels, limit_abs), C.c_float(0.0), C.c_uint32(0)
    check(_lib.load().paris_hip_air_value_host(C.byref(ar), None if m is None else m.ctypes.data, f.ctypes.data, f.shape[1], f.shape[0],
                                               C.byref(a), C.byref(n)), "paris_hip_air_value_host")
    return np.float32(a.value), n.value


def _bh_setting(c):
    """the setting for a sequence of coefficients c_1 ... c_N; a length outside 1 .. 4 gets the degree as it is, which the library
    refuses"""
    c = [float(x) for x in np.atleast_1d(np.asarray(c, np.float64))]
    s = BeamHardening()
    s.degree = len(c)
    for k, x in enumerate(c[:_lib.BH_DEGREE_MAX]):
        s.c[k] = x
    return s


def beam_hardening_check(c):
    """Host only, no device (paris_hip_beam_hardening_check): raises ParisHipError unless c holds 1 to 4 finite coefficients
    c_1 ... c_N of q = c_1 p + ... + c_N p^N."""
    s = _bh_setting(c)
    check(_lib.load().paris_hip_beam_hardening_check(C.byref(s)), "paris_hip_beam_hardening_check")


def beam_hardening_host(c, frame):
    """Host only, no device (paris_hip_beam_hardening_host): the beam-hardening rule on an array of line integrals, taken as float32
    -- Horner with fused multiply-adds and a final multiplication for p >= 0 or NaN, c_1 p for p < 0.
    Returns a float32 array of the same shape."""
    f = np.ascontiguousarray(frame, np.float32)
    out = np.empty_like(f)
    s = _bh_setting(c)
    check(_lib.load().paris_hip_beam_hardening_host(C.byref(s), f.ctypes.data if f.size else None, out.ctypes.data if f.size else None,
                                                    f.size), "paris_hip_beam_hardening_host")
    return out


def phase_alpha(det_geo, delta_over_beta, energy_kev):
    """Host only, no device (paris_hip_phase_alpha): alpha = pi lambda (delta / beta) d_od (d_so + d_od) / d_so in mm^2 at the detector
    plane, lambda = 1.2398419843e-6 mm keV / energy_kev, in double and rounded once to float."""
    a = C.c_float()
    check(_lib.load().paris_hip_phase_alpha(C.byref(det_geo), delta_over_beta, energy_kev, C.byref(a)), "paris_hip_phase_alpha")
    return a.value


def phase_default_margin(alpha_mm2, l_x, l_y):
    """Host only (paris_hip_phase_default_margin): max(8, ceil(6 sqrt(alpha) / (2 pi min(l_x, l_y)))) pixels, at most 1024; 0 for
    arguments that are not finite and positive."""
    return _lib.load().paris_hip_phase_default_margin(alpha_mm2, l_x, l_y)


def phase_retrieval_check(alpha_mm2, t_min, margin, dim_x, dim_y, l_x, l_y):
    """Host only (paris_hip_phase_retrieval_check): raises ParisHipError for a setting the library refuses -- a padded size above 8192
    is ERROR_UNSUPPORTED --, else returns (n_x, n_y, scratch_bytes)."""
    s = PhaseRetrieval(alpha_mm2, t_min, margin)
    nx, ny, b = C.c_uint32(), C.c_uint32(), C.c_size_t()
    check(_lib.load().paris_hip_phase_retrieval_check(C.byref(s), dim_x, dim_y, l_x, l_y, C.byref(nx), C.byref(ny), C.byref(b)),
          "paris_hip_phase_retrieval_check")
    return nx.value, ny.value, b.value


def phase_retrieval_host(alpha_mm2, t_min, margin, l_x, l_y, frame):
    """Host only (paris_hip_phase_retrieval_host): the phase-retrieval rule in double on one frame of line integrals, a 2-D array
    (dim_y, dim_x) taken as float32, rounded to float32 at the store. Returns a new array."""
    f = np.ascontiguousarray(frame, np.float32)
    if f.ndim != 2:
        raise ValueError("phase_retrieval_host: the frame must be a 2-D array (dim_y, dim_x)")
    out = np.empty_like(f)
    s = PhaseRetrieval(alpha_mm2, t_min, margin)
    check(_lib.load().paris_hip_phase_retrieval_host(C.byref(s), l_x, l_y, f.ctypes.data if f.size else None,
                                                     out.ctypes.data if f.size else None, f.shape[1], f.shape[0]),
          "paris_hip_phase_retrieval_host")
    return out


def scatter_default_margin(sigma1_mm, sigma2_mm, l_x, l_y):
    """Host only (paris_hip_scatter_default_margin): max(8, ceil(3 max(sigma) / min(l))) pixels, at most 1024; 0 for arguments that
    are not finite and positive."""
    return _lib.load().paris_hip_scatter_default_margin(sigma1_mm, sigma2_mm, l_x, l_y)


def scatter_correction_check(setting, dim_x, dim_y, l_x, l_y):
    """Host only (paris_hip_scatter_correction_check): setting is a ScatterCorrection (or the nine values of one). Raises ParisHipError
    for a setting the library refuses -- a padded size above 8192 is ERROR_UNSUPPORTED --, else returns (n_x, n_y, scratch_bytes)."""
    s = setting if isinstance(setting, ScatterCorrection) else ScatterCorrection(*setting)
    nx, ny, b = C.c_uint32(), C.c_uint32(), C.c_size_t()
    check(_lib.load().paris_hip_scatter_correction_check(C.byref(s), dim_x, dim_y, l_x, l_y, C.byref(nx), C.byref(ny), C.byref(b)),
          "paris_hip_scatter_correction_check")
    return nx.value, ny.value, b.value


def scatter_correction_host(setting, l_x, l_y, frame):
    """Host only (paris_hip_scatter_correction_host): the scatter rule in double on one frame of line integrals, a 2-D array
    (dim_y, dim_x) taken as float32, rounded to float32 at the store. Returns a new array."""
    f = np.ascontiguousarray(frame, np.float32)
    if f.ndim != 2:
        raise ValueError("scatter_correction_host: the frame must be a 2-D array (dim_y, dim_x)")
    out = np.empty_like(f)
    s = setting if isinstance(setting, ScatterCorrection) else ScatterCorrection(*setting)
    check(_lib.load().paris_hip_scatter_correction_host(C.byref(s), l_x, l_y, f.ctypes.data if f.size else None,
                                                        out.ctypes.data if f.size else None, f.shape[1], f.shape[0]),
          "paris_hip_scatter_correction_host")
    return out


def _starvation_filter(setting):
    return setting if isinstance(setting, StarvationFilter) else StarvationFilter(*setting)


def starvation_filter_check(setting, dim_x, dim_y):
    """Host only (paris_hip_starvation_filter_check): setting is a StarvationFilter (or its three values p0, gain, radius). Raises
    ParisHipError for a setting the library refuses -- dim_x * dim_y beyond 32 bits is ERROR_UNSUPPORTED --, else returns the bytes the
    setting occupies on a device."""
    s, b = _starvation_filter(setting), C.c_size_t()
    check(_lib.load().paris_hip_starvation_filter_check(C.byref(s), dim_x, dim_y, C.byref(b)), "paris_hip_starvation_filter_check")
    return b.value


def starvation_filter_tables(setting):
    """Host only (paris_hip_starvation_filter_tables): (sigma float32[64], g float32[64, radius + 1]) -- the width of every level in
    pixels and its weights g[k, d] for the distances d = 0 .. radius."""
    s = _starvation_filter(setting)
    r = s.radius if 1 <= s.radius <= _lib.STARVATION_RADIUS_MAX else 0
    sigma, g = np.zeros(_lib.STARVATION_LEVELS, np.float32), np.zeros((_lib.STARVATION_LEVELS, r + 1), np.float32)
    check(_lib.load().paris_hip_starvation_filter_tables(C.byref(s), sigma.ctypes.data, g.ctypes.data), "paris_hip_starvation_filter_tables")
    return sigma, g


def starvation_filter_host(setting, frame):
    """Host only (paris_hip_starvation_filter_host): the rule on one frame of line integrals, a 2-D array (dim_y, dim_x) taken as
    float32. Returns (a new array, the frame's StarvationCounts). The device gives these bits."""
    f = np.ascontiguousarray(frame, np.float32)
    if f.ndim != 2:
        raise ValueError("starvation_filter_host: the frame must be a 2-D array (dim_y, dim_x)")
    out, counts, s = np.empty_like(f), StarvationCounts(), _starvation_filter(setting)
    check(_lib.load().paris_hip_starvation_filter_host(C.byref(s), f.ctypes.data if f.size else None, out.ctypes.data if f.size else None,
                                                       f.shape[1], f.shape[0], C.byref(counts)), "paris_hip_starvation_filter_host")
    return out, counts


_LAG_STARTS = {"rest": _lib.LAG_START_REST, "steady": _lib.LAG_START_STEADY}


def _lag_setting(terms, start):
    """the model for a sequence of (b_n, a_n) pairs and start "steady" / "rest"; a length outside 1 .. 4 gets the term count as it is
    and an unknown start the value -1, both of which the library refuses"""
    pairs = [(float(b), float(a)) for b, a in terms]
    m = LagModel()
    m.terms = len(pairs)
    for n, (b, a) in enumerate(pairs[:_lib.LAG_TERMS_MAX]):
        m.b[n], m.a[n] = b, a
    m.start = _LAG_STARTS.get(start, start if isinstance(start, int) else -1)
    return m


def lag_model_check(terms, start="steady"):
    """Host only, no device (paris_hip_lag_model_check): raises ParisHipError unless terms holds 1 to 4 pairs (b_n, a_n), each finite
    and > 0, with b_0 = 1 - sum b_n / (1 - exp(-a_n)) > 0, and start is "steady" or "rest" (DESIGN.md section 4.20)."""
    m = _lag_setting(terms, start)
    check(_lib.load().paris_hip_lag_model_check(C.byref(m)), "paris_hip_lag_model_check")


def lag_coefficients(terms, start="steady"):
    """Host only, no device (paris_hip_lag_coefficients): (g, c, w, inv_b, b0) of the model -- g_n = exp(-a_n), c_n = b_n g_n / B,
    w_n = 1 / (1 - g_n) as float32[N], inv_b = 1 / B as np.float32, each computed in double and rounded once, and b0 as a float."""
    m = _lag_setting(terms, start)
    g, c, w = (np.zeros(_lib.LAG_TERMS_MAX, np.float32) for _ in range(3))
    inv_b, b0 = C.c_float(0.0), C.c_double(0.0)
    check(_lib.load().paris_hip_lag_coefficients(C.byref(m), g.ctypes.data, c.ctypes.data, w.ctypes.data, C.byref(inv_b), C.byref(b0)),
          "paris_hip_lag_coefficients")
    n = m.terms
    return g[:n].copy(), c[:n].copy(), w[:n].copy(), np.float32(inv_b.value), b0.value


def lag_correct_host(terms, frames, dark=None, start="steady", state=None, started=False):
    """Host only, no device (paris_hip_lag_correct_host): the lag rule on frames[f] (float32 counts, f in time order, every frame of
    one shape), with the dark frame `dark` (None: zero). state: None opens a sequence; otherwise the (N, *frame shape) float32 array
    and the `started` flag an earlier call returned. Returns (corrected frames, state, started): the inputs are not written."""
    f = np.array(frames, np.float32, order="C")
    if f.ndim < 1:
        raise ValueError("lag_correct_host: frames must hold a leading frame axis")
    m = _lag_setting(terms, start)
    n_frames, n_pixels = f.shape[0], int(np.prod(f.shape[1:], dtype=np.int64))
    d = None if dark is None else np.ascontiguousarray(dark, np.float32)
    if d is not None and d.size != n_pixels:
        raise ValueError("lag_correct_host: the dark frame and the frames differ in size")
    st = np.zeros((max(m.terms, 0),) + f.shape[1:], np.float32) if state is None else np.array(state, np.float32, order="C")
    if st.size != m.terms * n_pixels:
        raise ValueError("lag_correct_host: the state does not belong to these frames and terms")
    flag = C.c_int(1 if (started and state is not None) else 0)
    check(_lib.load().paris_hip_lag_correct_host(C.byref(m), None if d is None else d.ctypes.data, f.ctypes.data if f.size else None,
                                                 st.ctypes.data if st.size else None, C.byref(flag), n_pixels, n_frames),
          "paris_hip_lag_correct_host")
    return f, st, bool(flag.value)


def metal_words(dim_x):
    """the uint64 words a packed trace holds per row of dim_x pixels"""
    return (dim_x + 63) // 64


def metal_check(dim_x, dim_y, dim_z, threshold, grow=0, min_path=0.0):
    """Host only, no device (paris_hip_metal_check): raises ParisHipError for a zero dimension, a threshold that is not finite, grow > 4
    or a min_path that is negative or not finite; returns the cap on the voxels a threshold may mark -- 1/32 of the grid, 1024 at
    least."""
    cap = C.c_uint64(0)
    check(_lib.load().paris_hip_metal_check(dim_x, dim_y, dim_z, threshold, grow, min_path, C.byref(cap)), "paris_hip_metal_check")
    return int(cap.value)


def metal_collect_host(v, threshold, max_n=None, binarize=False):
    """Host only, no device (paris_hip_metal_collect_host): (index uint64[n], value float32[n], mask) of the voxels of the 3-D array v
    (dim_z, dim_y, dim_x; taken as float32) above threshold, in ascending linear index; mask is the binarized copy of v with
    binarize, else None. v is not written. max_n None: the cap of metal_check(). More than max_n hits raise ParisHipError with the
    status ERROR_METAL_TOO_MANY_VOXELS and the count as .n."""
    a = np.array(v, np.float32, order="C")
    if a.ndim != 3:
        raise ValueError("metal_collect_host: the volume must be a 3-D array (dim_z, dim_y, dim_x)")
    dz, dy, dx = a.shape
    cap = metal_check(dx, dy, dz, threshold) if max_n is None else int(max_n)
    room = min(cap, a.size)
    index, value, n = np.empty(room, np.uint64), np.empty(room, np.float32), C.c_uint64(0)
    status = _lib.load().paris_hip_metal_collect_host(a.ctypes.data, dx, dy, dz, threshold, room, index.ctypes.data if room else None,
                                                      value.ctypes.data if room else None, C.byref(n), 1 if binarize else 0)
    if status == _lib.SUCCESS and n.value > cap:
        status = _lib.ERROR_METAL_TOO_MANY_VOXELS
    _metal_collect_check(status, n.value, "paris_hip_metal_collect_host")
    return index[:n.value].copy(), value[:n.value].copy(), (a if binarize else None)


def _metal_collect_check(status, n, what):
    if status == _lib.ERROR_METAL_TOO_MANY_VOXELS:
        e = ParisHipError(status, what)
        e.n = int(n)
        raise e
    check(status, what)


def metal_trace_pack_host(t, min_path, grow=0):
    """Host only, no device (paris_hip_metal_trace_pack_host): the packed trace uint64[(n_frames, dim_y, words)] of the frames t
    (n_frames, dim_y, dim_x; a 2-D array is one frame), taken as float32: a pixel is in it when any pixel of its frame at most grow
    away in x and in y is above min_path."""
    a = np.ascontiguousarray(t, np.float32)
    if a.ndim == 2:
        a = a[None]
    if a.ndim != 3:
        raise ValueError("metal_trace_pack_host: the frames must be a 2-D or 3-D array")
    n, dy, dx = a.shape
    bits = np.zeros((n, dy, metal_words(dx)), np.uint64)
    check(_lib.load().paris_hip_metal_trace_pack_host(a.ctypes.data if a.size else None, n, dx, dy, min_path, grow,
                                                      bits.ctypes.data if bits.size else None), "paris_hip_metal_trace_pack_host")
    return bits


def metal_inpaint_host(p, bits, row_first=0, row_count=None):
    """Host only, no device (paris_hip_metal_inpaint_host): (the inpainted copy of the 2-D float32 frame p, MetalCounts) for the
    trace bits uint64[(dim_y, words)] and the rows [row_first, row_first + row_count) -- None: to the last row."""
    a = np.array(p, np.float32, order="C")
    b = np.ascontiguousarray(bits, np.uint64)
    if a.ndim != 2 or b.shape != (a.shape[0], metal_words(a.shape[1])):
        raise ValueError("metal_inpaint_host: the trace does not belong to this frame")
    count = a.shape[0] - row_first if row_count is None else row_count
    st = MetalCounts()
    check(_lib.load().paris_hip_metal_inpaint_host(a.ctypes.data if a.size else None, b.ctypes.data if b.size else None, a.shape[1], a.shape[0],
                                                   row_first, count, C.byref(st)), "paris_hip_metal_inpaint_host")
    return a, st


class MetalTrace:
    """What Backend.reduce_metal returns: index / value -- the metal voxels of the first reconstruction, as metal_collect_host lists
    them --, bits -- the packed traces uint64[(n_views, dim_y, words)] --, trace_pixels -- the set bits --, threshold, grow, min_path."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def bh_threshold_from_histogram(hist, h_lo, h_hi):
    """Host only, no device (paris_hip_bh_threshold_from_histogram): Otsu's threshold of a linear histogram over [h_lo, h_hi] -- the
    upper edge of the smallest bin that maximises the between-class variance -- as np.float32."""
    h = np.ascontiguousarray(hist, np.uint64)
    if h.ndim != 1:
        raise ValueError("bh_threshold_from_histogram: the histogram must be a 1-D array")
    thr = C.c_float(0)
    check(_lib.load().paris_hip_bh_threshold_from_histogram(h.ctypes.data if h.size else None, h.size, h_lo, h_hi, C.byref(thr)),
          "paris_hip_bh_threshold_from_histogram")
    return np.float32(thr.value)


def _bh_terms(degree):
    return (degree + 1) * (degree + 2) // 2


def bh_gram_host(basis, labels):
    """Host only, no device (paris_hip_bh_gram_host): the Gram sums of g = (f_1 ... f_N, m) over the labelled voxels in the order
    DESIGN.md section 4.17 fixes. basis: N arrays of one shape, taken as float32; labels: uint8 of that shape. Returns
    (float64[(N + 1)(N + 2) / 2], BhCounts)."""
    fs = [np.ascontiguousarray(f, np.float32) for f in basis]
    lab = np.ascontiguousarray(labels, np.uint8)
    if any(f.shape != lab.shape for f in fs):
        raise ValueError("bh_gram_host: the basis volumes and the labels differ in shape")
    ptrs = (C.c_void_p * max(len(fs), 1))(*[f.ctypes.data for f in fs])
    g, cnt = np.zeros(_bh_terms(len(fs)), np.float64), BhCounts()
    check(_lib.load().paris_hip_bh_gram_host(ptrs, len(fs), lab.ctypes.data, lab.size, g.ctypes.data, C.byref(cnt)), "paris_hip_bh_gram_host")
    return g, cnt


def bh_gram_matrix(gram, degree):
    """the packed upper triangle paris_hip_bh_gram returns as the full symmetric (degree + 1) x (degree + 1) float64 matrix"""
    n = degree + 1
    m = np.zeros((n, n), np.float64)
    m[np.triu_indices(n)] = np.asarray(gram, np.float64)
    return m + np.triu(m, 1).T


def bh_solve(gram, degree, counts, min_voxels=0):
    """Host only, no device (paris_hip_bh_solve): the coefficients that make sum c_k f_k as close as possible, in the least-squares
    sense over the labelled voxels, to the two-level template T m, with T the mean of f_1 over the object's core -- by Cholesky in
    double. Returns the BhFit: .setting (degree, c), .level, .residual_before, .residual_after. Raises ParisHipError with the status
    ERROR_BH_TOO_FEW_VOXELS, ERROR_BH_NOT_POSITIVE or ERROR_BH_NOT_FINITE for a fit the library refuses."""
    g = np.ascontiguousarray(gram, np.float64)
    if g.size != _bh_terms(degree):
        raise ValueError("bh_solve: %d Gram sums do not belong to degree %d" % (g.size, degree))
    fit = BhFit()
    check(_lib.load().paris_hip_bh_solve(g.ctypes.data, degree, C.byref(counts), min_voxels, C.byref(fit)), "paris_hip_bh_solve")
    return fit


class Labels:
    """one byte per voxel of a dim_x x dim_y x dim_z slab on the device (Backend.bh_classify / Backend.labels_from_host)"""

    def __init__(self, store, dim_x, dim_y, dim_z):
        self._store = store  # the device allocation that holds the bytes
        self.dim_x, self.dim_y, self.dim_z = dim_x, dim_y, dim_z

    @property
    def ptr(self):
        return self._store.ptr

    @property
    def size(self):
        return self.dim_x * self.dim_y * self.dim_z


class BeamHardeningFit:
    """What Backend.fit_beam_hardening returns: c (float32[N], as solved), level, residual_before, residual_after, threshold,
    counts (BhCounts), gram (float64, packed), labels (uint8 (dim_z, dim_y, dim_x) of the fitted slab) and slices (first, count)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def row_extension_check(edge_pixels, taper_pixels, dim_x):
    """Host only, no device (paris_hip_row_extension_check): raises ParisHipError unless edge_pixels is 1, 2, 4 or 8, taper_pixels lies
    in [1, 16384] and rows of dim_x pixels hold at least edge_pixels."""
    re = RowExtension(edge_pixels, taper_pixels)
    check(_lib.load().paris_hip_row_extension_check(C.byref(re), dim_x), "paris_hip_row_extension_check")


def row_extension_response(edge_pixels, taper_pixels, dim_x, tau):
    """Host only, no device (paris_hip_row_extension_response): the ramp's response c[dim_x] (float32) to the cos^2 taper of
    taper_pixels pixels beyond a row's edge, for the pixel pitch tau -- what the filter adds at its store, times the edge means
    (DESIGN.md section 4.11)."""
    re = RowExtension(edge_pixels, taper_pixels)
    c = np.empty(max(int(dim_x), 0), np.float32)
    check(_lib.load().paris_hip_row_extension_response(C.byref(re), dim_x, tau, c.ctypes.data), "paris_hip_row_extension_response")
    return c


_VOXEL_TYPES = {np.dtype(np.uint8): _lib.VOXEL_U8, np.dtype(np.uint16): _lib.VOXEL_U16}


def _volume_window(lo, hi, dtype):
    """the setting for a numpy integer type; an unknown one gets the voxel type 0, which the library refuses"""
    try:
        voxel_type = _VOXEL_TYPES.get(np.dtype(dtype), 0)
    except TypeError:
        voxel_type = 0
    return VolumeWindow(lo, hi, voxel_type)


def volume_window_check(lo, hi, dtype):
    """Host only, no device (paris_hip_volume_window_check): raises ParisHipError unless dtype is uint8 or uint16, lo and hi are
    finite, hi > lo and the window is neither too narrow nor too wide for the rule's scale."""
    w = _volume_window(lo, hi, dtype)
    check(_lib.load().paris_hip_volume_window_check(C.byref(w)), "paris_hip_volume_window_check")


def _volume_bilateral(sigma_r, sigma_s=1.0, radius=None):
    """the setting; radius None: min(3, ceil(2 sigma_s)), at least 1"""
    if radius is None:
        radius = int(min(3, max(1, np.ceil(2.0 * sigma_s)))) if np.isfinite(sigma_s) else 0
    return VolumeBilateral(sigma_r, sigma_s, radius)


def volume_bilateral_check(sigma_r, sigma_s=1.0, radius=None):
    """Host only, no device (paris_hip_volume_bilateral_check): raises ParisHipError unless both sigmas are finite and > 0, the radius
    is 1, 2 or 3 and 1024 / (4 sigma_r) is a finite float above 0. Returns the VolumeBilateral."""
    b = _volume_bilateral(sigma_r, sigma_s, radius)
    check(_lib.load().paris_hip_volume_bilateral_check(C.byref(b)), "paris_hip_volume_bilateral_check")
    return b


def volume_bilateral_tables(sigma_r, sigma_s=1.0, radius=None):
    """Host only (paris_hip_volume_bilateral_tables): (spatial float32[2r+1, 2r+1, 2r+1] indexed [dz, dy, dx], range float32[1024],
    rscale as a Python float that is an exact float32) of the setting."""
    b = _volume_bilateral(sigma_r, sigma_s, radius)
    side = 2 * min(int(b.radius), _lib.BILATERAL_RADIUS_MAX) + 1
    spatial, rng, rscale = np.empty((side, side, side), np.float32), np.empty(_lib.BILATERAL_BINS, np.float32), C.c_float(0)
    check(_lib.load().paris_hip_volume_bilateral_tables(C.byref(b), spatial.ctypes.data, rng.ctypes.data, C.byref(rscale)),
          "paris_hip_volume_bilateral_tables")
    return spatial, rng, float(rscale.value)


def volume_bilateral_host(v, sigma_r, sigma_s=1.0, radius=None, z_first=0, z_count=None):
    """Host only, no device (paris_hip_volume_bilateral_host): slices [z_first, z_first + z_count) of the 3-D array v (dim_z, dim_y,
    dim_x; taken as float32) filtered by the rule, as a new float32 array of z_count slices. z_count None: all from z_first on."""
    a = np.ascontiguousarray(v, np.float32)
    if a.ndim != 3:
        raise ValueError("volume_bilateral_host: the volume must be a 3-D array")
    dim_z, dim_y, dim_x = a.shape
    n = dim_z - z_first if z_count is None else z_count
    b = _volume_bilateral(sigma_r, sigma_s, radius)
    out = np.empty((max(int(n), 0), dim_y, dim_x), np.float32)
    check(_lib.load().paris_hip_volume_bilateral_host(a.ctypes.data if a.size else None, dim_x, dim_y, dim_z, z_first, max(int(n), 0), C.byref(b),
                                                      out.ctypes.data if out.size else None), "paris_hip_volume_bilateral_host")
    return out


def volume_window_from_histogram(hist, h_lo, h_hi, p_lo=0.1, p_hi=99.9):
    """Host only, no device (paris_hip_volume_window_from_histogram): the window (w_lo, w_hi) between the percentiles p_lo and p_hi
    of a linear histogram over [h_lo, h_hi], as two Python floats that are exact float32 values."""
    h = np.ascontiguousarray(hist, np.uint64)
    if h.ndim != 1:
        raise ValueError("volume_window_from_histogram: the histogram must be a 1-D array")
    w_lo, w_hi = C.c_float(0), C.c_float(0)
    check(_lib.load().paris_hip_volume_window_from_histogram(h.ctypes.data if h.size else None, h.size, h_lo, h_hi, p_lo, p_hi,
                                                             C.byref(w_lo), C.byref(w_hi)), "paris_hip_volume_window_from_histogram")
    return w_lo.value, w_hi.value


class Backend:
    """One device + stream: the state the reference keeps in thread_local statics after set_device
    (src/main.cpp:87). synchronous=True reproduces the reference's blocking calls. stream: None = a private stream of
    the ctx, a hipStream_t handle = that stream, 0 = the legacy default stream."""

    def __init__(self, device=0, stream=None, synchronous=True):
        self._L = _lib.load()
        ctx = C.c_void_p()
        flags = _lib.CTX_SYNCHRONOUS if synchronous else _lib.CTX_DEFAULT
        if stream is not None and stream == 0:
            # the caller's stream is the legacy default stream (what torch.cuda.current_stream().cuda_stream returns unless a
            # stream was set): enqueue there too, so that the caller's own work and these kernels stay ordered
            flags |= _lib.CTX_LEGACY_STREAM
        check(self._L.paris_hip_ctx_create(device, C.c_void_p(stream) if stream else None, flags, C.byref(ctx)),
              "paris_hip_ctx_create")
        self._ctx = ctx
        self.device = device
        self._owned = set()
        self._wrapped = {}  # device address of a wrapped volume -> weak reference to its owner (None: wrapped without one)

    # ---- lifetime ------------------------------------------------------------------------------------
    def close(self):
        if self._ctx is not None:
            # projections still deferred into a wrapped (caller-owned) volume: run them while the caller's memory is certainly
            # still there -- paris_hip_ctx_destroy itself only runs pending work into volumes the library allocated
            if self._pending_volume_alive():
                self._L.paris_hip_flush(self._ctx)
            for p in list(self._owned):
                self._L.paris_hip_free(self._ctx, C.c_void_p(p))
            self._owned.clear()
            self._L.paris_hip_ctx_destroy(self._ctx)
            self._ctx = None

    def _pending_volume_alive(self):
        """True when projections are pending into a wrapped volume whose owner (wrap_volume(owner=...)) is still alive. Decided
        for THAT volume alone (one owner-less wrap used to switch the close-time flush off for every volume). A
        volume wrapped without an owner is never flushed into at close: nothing says its memory still belongs to the caller --
        callers of owner-less wraps call flush() before they let go of the memory."""
        n, ptr = C.c_uint32(0), C.c_void_p()
        if self._L.paris_hip_pending_backprojections(self._ctx, C.byref(n), C.byref(ptr)) != 0 or n.value == 0 or not ptr.value:
            return False
        for base, (ref, nbytes) in self._wrapped.items():
            if base <= ptr.value < base + nbytes:
                return ref is not None and ref() is not None
        return False

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def synchronize(self):
        check(self._L.paris_hip_ctx_synchronize(self._ctx), "paris_hip_ctx_synchronize")

    @property
    def stream(self):
        """the hipStream_t handle the ctx enqueues on (0 = the legacy default stream)"""
        return self._L.paris_hip_ctx_stream(self._ctx) or 0

    def free(self, obj):
        ptr = obj.ptr if hasattr(obj, "ptr") else obj
        if ptr in self._owned:
            check(self._L.paris_hip_free(self._ctx, C.c_void_p(ptr)), "paris_hip_free")
            self._owned.discard(ptr)

    # ---- memory (src/openmp/memory.cpp:33-79, src/cuda/memory.cpp:33-102) -------------------------------
    def make_projection_host(self, dim_x, dim_y):
        return Projection(np.empty((dim_y, dim_x), np.float32), dim_x, dim_y)

    def make_projection_device(self, dim_x, dim_y):
        ptr, pitch = C.c_void_p(), C.c_size_t()
        check(self._L.paris_hip_malloc_projection(self._ctx, dim_x, dim_y, C.byref(ptr), C.byref(pitch)),
              "paris_hip_malloc_projection")
        self._owned.add(ptr.value)
        return Projection(ptr.value, dim_x, dim_y, pitch=pitch.value, on_device=True, owner=self)

    def make_volume_host(self, dim_x, dim_y, dim_z):
        return Volume(np.zeros((dim_z, dim_y, dim_x), np.float32), dim_x, dim_y, dim_z)

    def make_volume_device(self, dim_x, dim_y, dim_z):
        ptr = C.c_void_p()
        check(self._L.paris_hip_malloc_volume(self._ctx, dim_x, dim_y, dim_z, C.byref(ptr)),
              "paris_hip_malloc_volume")
        self._owned.add(ptr.value)
        return Volume(ptr.value, dim_x, dim_y, dim_z, on_device=True, owner=self)

    def wrap_projection(self, ptr, pitch, dim_x, dim_y, idx=0, phi=0.0, owner=None):
        """Adopts device memory allocated elsewhere (e.g. a torch tensor's data_ptr())."""
        return Projection(ptr, dim_x, dim_y, idx, phi, pitch=pitch, on_device=True, owner=owner)

    def wrap_volume(self, ptr, dim_x, dim_y, dim_z, off=0, owner=None, clean=None):
        """Adopts device memory allocated elsewhere as a volume. The library knows nothing about its contents, so every
        addition is performed (paris_hip_set_backproject_skip_invalid does not apply) unless the caller vouches with clean=True
        that it holds no -0 right now (e.g. torch.zeros) and will call volume_mark_dirty before writing anything but zeros into
        it; clean=False withdraws an earlier promise for the range; clean="scan" lets the device look for -0 once
        (paris_hip_volume_scan_clean) and skip when there is none, under the same duty."""
        v = Volume(ptr, dim_x, dim_y, dim_z, off, on_device=True, owner=owner)
        import weakref
        for base in [b for b, (ref, _) in self._wrapped.items() if ref is not None and ref() is None]:
            del self._wrapped[base]  # owners that have been collected: their wraps are history
        try:
            ref = weakref.ref(owner) if owner is not None else None
        except TypeError:
            ref = None
        self._wrapped[ptr] = (ref, 4 * dim_x * dim_y * dim_z)
        if clean is True:
            self.volume_mark_clean(v)
        elif clean is False:
            self.volume_mark_dirty(v)
        elif clean == "scan":
            self.volume_scan_clean(v)
        elif clean is not None:
            raise ValueError("clean must be None, True, False or 'scan'")
        return v

    def volume_mark_dirty(self, v):
        """the caller wrote the volume itself and may have stored a -0 (paris_hip_volume_mark_dirty)"""
        check(self._L.paris_hip_volume_mark_dirty(self._ctx, v.ptr, 4 * v.dim_x * v.dim_y * v.dim_z), "paris_hip_volume_mark_dirty")

    def volume_mark_clean(self, v):
        """the caller vouches that the volume holds no -0 right now (paris_hip_volume_mark_clean)"""
        check(self._L.paris_hip_volume_mark_clean(self._ctx, v.ptr, 4 * v.dim_x * v.dim_y * v.dim_z), "paris_hip_volume_mark_clean")

    def volume_scan_clean(self, v):
        """reads the volume once on the device; lists it as clean when it holds no -0; returns the number of -0 found"""
        n = C.c_uint64(0)
        check(self._L.paris_hip_volume_scan_clean(self._ctx, v.ptr, 4 * v.dim_x * v.dim_y * v.dim_z, C.byref(n)),
              "paris_hip_volume_scan_clean")
        return int(n.value)

    # ---- volume export ----------------------------------------------------------
    volume_window_check = staticmethod(volume_window_check)
    volume_window_from_histogram = staticmethod(volume_window_from_histogram)

    def volume_stats(self, v, lo=None, hi=None, n_bins=0):
        """paris_hip_volume_stats of a device volume: (VolumeStatistics, hist). The statistics hold min and max of the finite voxels
        (+inf / -inf without one), not_finite and voxels; with n_bins > 0 hist is the linear histogram of n_bins uint64 counters over
        [lo, hi], and below / above count the finite voxels outside it; with n_bins == 0 hist is None. Runs what is deferred first
        and waits for the result."""
        st = VolumeStatistics()
        hist = np.zeros(n_bins, np.uint64) if n_bins else None
        if n_bins and (lo is None or hi is None):
            raise ParisHipError(_lib.ERROR_INVALID_ARGUMENT, "paris_hip_volume_stats")
        check(self._L.paris_hip_volume_stats(self._ctx, v.ptr, v.dim_x * v.dim_y * v.dim_z, lo if n_bins else 0.0, hi if n_bins else 0.0,
                                             n_bins, hist.ctypes.data if n_bins else None, C.byref(st)), "paris_hip_volume_stats")
        return st, hist

    def quantize_volume(self, v, lo, hi, dtype, out=None):
        """The device volume v as unsigned integers over the window [lo, hi] (dtype numpy uint8 or uint16): q = rint((v - lo) * scale)
        clamped to [0, L], NaN as 0. Without `out` the voxels come back as a numpy array of the volume's shape
        (paris_hip_volume_quantize_d2h, then a wait). With `out` -- a device address, or an object with .ptr -- they are written
        there, device to device (paris_hip_volume_quantize; no wait), and out is returned. Runs what is deferred first and adds to
        volume_quantize_counts()."""
        w = _volume_window(lo, hi, dtype)
        n = v.dim_x * v.dim_y * v.dim_z
        if out is not None:
            check(self._L.paris_hip_volume_quantize(self._ctx, v.ptr, n, C.byref(w), out.ptr if hasattr(out, "ptr") else out),
                  "paris_hip_volume_quantize")
            return out
        check(self._L.paris_hip_volume_window_check(C.byref(w)), "paris_hip_volume_window_check")
        q = np.empty((v.dim_z, v.dim_y, v.dim_x), np.dtype(dtype))
        check(self._L.paris_hip_volume_quantize_d2h(self._ctx, v.ptr, n, C.byref(w), q.ctypes.data), "paris_hip_volume_quantize_d2h")
        self.synchronize()
        return q

    def volume_quantize_counts(self, reset=False):
        """The VolumeCounts of this backend's quantize_volume() calls since it was made or last reset
        (paris_hip_volume_quantize_counts): voxels, below, above, not_finite. Waits for the ctx stream."""
        st = VolumeCounts()
        check(self._L.paris_hip_volume_quantize_counts(self._ctx, C.byref(st), 1 if reset else 0), "paris_hip_volume_quantize_counts")
        return st

    # ---- volume denoising --------------------------------------------------------
    volume_bilateral_check = staticmethod(volume_bilateral_check)
    volume_bilateral_tables = staticmethod(volume_bilateral_tables)
    volume_bilateral_host = staticmethod(volume_bilateral_host)

    def set_volume_bilateral(self, sigma_r, sigma_s=1.0, radius=None):
        """The setting volume_bilateral() filters with from here on: sigma_r in the volume's units, sigma_s in voxels, radius 1 .. 3
        (None: min(3, ceil(2 sigma_s))). Checked on the host (raises ParisHipError); the device tables are made by the first call that
        uses it. sigma_r None: no setting, volume_bilateral() refuses."""
        self._bilateral = None if sigma_r is None else volume_bilateral_check(sigma_r, sigma_s, radius)

    def volume_bilateral(self, v, out=None, z_first=0, z_count=None):
        """paris_hip_volume_bilateral with the setting of set_volume_bilateral(): slices [z_first, z_first + z_count) of the device
        volume v (z_count None: all from z_first on) filtered into z_count slices at out -- a device Volume, a device address or an
        object with .ptr, which must not overlap v; None: a new device volume of z_count slices. A z tap outside v is skipped, so a
        slab of a larger grid is passed with its halo slices and without them in the range. Runs what is deferred first; does not
        wait. Returns out."""
        b = getattr(self, "_bilateral", None)
        if b is None:
            raise ParisHipError(_lib.ERROR_INVALID_ARGUMENT, "paris_hip_volume_bilateral")
        n = v.dim_z - z_first if z_count is None else z_count
        if out is None:
            if n <= 0:
                raise ParisHipError(_lib.ERROR_INVALID_ARGUMENT, "paris_hip_volume_bilateral")
            out = self.make_volume_device(v.dim_x, v.dim_y, n)
        check(self._L.paris_hip_volume_bilateral(self._ctx, v.ptr, v.dim_x, v.dim_y, v.dim_z, z_first, max(int(n), 0), C.byref(b),
                                                 out.ptr if hasattr(out, "ptr") else out), "paris_hip_volume_bilateral")
        return out

    def memset_volume(self, v):
        check(self._L.paris_hip_memset_volume(self._ctx, v.ptr, v.dim_x, v.dim_y, v.dim_z), "paris_hip_memset_volume")

    def copy_h2d(self, h, d):
        """copy_h2d for projections (carries idx, phi: src/openmp/memory.cpp:60-62) and volumes (off: :73)."""
        if isinstance(h, Projection):
            assert h.buf.dtype == np.float32 and h.dim_x == d.dim_x and h.dim_y == d.dim_y
            check(self._L.paris_hip_memcpy_projection_h2d(self._ctx, d.ptr, d.pitch, h.ptr, h.buf.strides[0],
                                                          h.dim_x, h.dim_y), "paris_hip_memcpy_projection_h2d")
            d.idx, d.phi = h.idx, h.phi
        else:
            assert h.buf.dtype == np.float32 and (h.dim_x, h.dim_y, h.dim_z) == (d.dim_x, d.dim_y, d.dim_z)
            check(self._L.paris_hip_memcpy_volume_h2d(self._ctx, d.ptr, h.ptr, h.dim_x, h.dim_y, h.dim_z),
                  "paris_hip_memcpy_volume_h2d")
            d.off = h.off
        self.synchronize()

    def upload(self, h, d):
        """copy_h2d for a projection on the ctx's upload stream (paris_hip_upload_projection): returns without waiting;
        kernels enqueued afterwards are ordered behind the transfer, kernels already queued overlap it."""
        assert h.buf.dtype == np.float32 and h.dim_x == d.dim_x and h.dim_y == d.dim_y
        check(self._L.paris_hip_upload_projection(self._ctx, d.ptr, d.pitch, h.ptr, h.buf.strides[0],
                                                  h.dim_x, h.dim_y), "paris_hip_upload_projection")
        d.idx, d.phi = h.idx, h.phi

    _PIXEL_TYPES = {np.dtype(np.uint8): _lib.PIXEL_U8, np.dtype(np.uint16): _lib.PIXEL_U16, np.dtype(np.uint32): _lib.PIXEL_U32,
                    np.dtype(np.float32): _lib.PIXEL_F32}

    def upload_raw(self, h, d, row_first=0, corrected=False):
        """upload() of a frame in its stored pixel type (paris_hip_upload_projection_raw): h is a 2-D uint8, uint16, uint32 or float32
        ndarray (rows may be padded: h.strides[0] is the host pitch); the copy carries its bytes as they are and the device widens
        them to fp32 in place -- bit for bit h.astype(np.float32). Returns without waiting, like upload().
        h may be a band of rows: they go to rows [row_first, row_first + len(h)) of d. corrected: the same pass also applies the
        dark / flat correction of set_flat_field() (paris_hip_upload_projection_raw_corrected) -- bit for bit upload_raw()
        followed by flat_field_rows() on those rows."""
        if not isinstance(h, np.ndarray) or h.ndim != 2:
            raise TypeError("upload_raw: h must be a 2-D ndarray")
        if h.dtype == np.float64:
            raise TypeError("upload_raw: float64 frames are not uploaded raw -- convert them on the host (h.astype(np.float32))")
        pixel = self._PIXEL_TYPES.get(h.dtype)
        if pixel is None:
            raise TypeError("upload_raw: unsupported dtype %s (uint8, uint16, uint32 or float32)" % h.dtype)
        if h.strides[1] != h.itemsize or h.strides[0] < h.shape[1] * h.itemsize:
            raise ValueError("upload_raw: the rows of h must be contiguous")
        rows = h.shape[0]
        assert h.shape[1] == d.dim_x and 0 <= row_first and row_first + rows <= d.dim_y
        if corrected:
            check(self._L.paris_hip_upload_projection_raw_corrected(self._ctx, d.ptr, d.pitch, h.ctypes.data, h.strides[0], d.dim_x,
                                                                    d.dim_y, row_first, rows, pixel),
                  "paris_hip_upload_projection_raw_corrected")
            return
        check(self._L.paris_hip_upload_projection_raw(self._ctx, d.ptr + row_first * d.pitch, d.pitch, h.ctypes.data, h.strides[0],
                                                      d.dim_x, rows, pixel), "paris_hip_upload_projection_raw")

    def set_flat_field(self, dark, flat, t_min=1e-5):
        """Dark / flat correction to line integrals (paris_hip_set_flat_field): dark (None = zeros) and flat are 2-D arrays of the
        detector's size (n_col, n_row), taken as float32. p = -ln(max((I - D) / (F - D), t_min)), in double, rounded once; a pixel
        whose I, D or F is not finite or whose flat is not above its dark becomes 0. Replaces an earlier setting safely: work already
        queued keeps the old frames."""
        f = np.ascontiguousarray(flat, np.float32)
        if f.ndim != 2:
            raise ValueError("set_flat_field: flat must be a 2-D array")
        dk = None if dark is None else np.ascontiguousarray(dark, np.float32)
        if dk is not None and dk.shape != f.shape:
            raise ValueError("set_flat_field: dark and flat differ in shape")
        check(self._L.paris_hip_set_flat_field(self._ctx, None if dk is None else dk.ctypes.data, f.ctypes.data, f.shape[1], f.shape[0],
                                               t_min), "paris_hip_set_flat_field")
        self._flat_shape = f.shape

    def clear_flat_field(self):
        """paris_hip_clear_flat_field: no correction from here on"""
        check(self._L.paris_hip_clear_flat_field(self._ctx), "paris_hip_clear_flat_field")
        self._flat_shape = None

    def flat_field_rows(self, p, row_first=0, row_count=None, frame_stride=0, n_frames=1):
        """The correction of set_flat_field() in place on float frames (paris_hip_flat_field_rows): rows [row_first, row_first +
        row_count) of n_frames frames frame_stride bytes apart starting at p, each with the reference rows of the same detector rows"""
        count = p.dim_y - row_first if row_count is None else row_count
        check(self._L.paris_hip_flat_field_rows(self._ctx, p.ptr, p.pitch, frame_stride, n_frames, p.dim_x, p.dim_y, row_first, count),
              "paris_hip_flat_field_rows")

    def flat_field_dead_pixels(self):
        """The pixels of the current set_flat_field() setting that are dead whatever a frame holds -- dark or flat not finite, or flat
        not above dark -- as a uint8 array (n_col, n_row) of 0 / 1 (paris_hip_flat_field_dead_pixels); OR it into a defect map"""
        if getattr(self, "_flat_shape", None) is None:
            raise ParisHipError(_lib.ERROR_INVALID_ARGUMENT, "paris_hip_flat_field_dead_pixels")
        out = np.empty(self._flat_shape, np.uint8)
        check(self._L.paris_hip_flat_field_dead_pixels(self._ctx, out.ctypes.data), "paris_hip_flat_field_dead_pixels")
        return out

    # ---- defect map ---------------------------------------------------------------
    defect_plan = staticmethod(defect_plan)

    def set_defect_map(self, mask):
        """paris_hip_set_defect_map: mask is a 2-D array of the detector's size (n_col, n_row), nonzero = defective. Each defective
        pixel is then replaced, by defect_repair_rows(), with the inverse-square-distance weighted mean of the good pixels on the
        nearest ring that holds one (up to 8 pixels away). Replaces an earlier setting safely: work already queued keeps the old
        plan. Returns defect_map_info()."""
        m = _mask_bytes(mask, "set_defect_map")
        check(self._L.paris_hip_set_defect_map(self._ctx, m.ctypes.data, m.shape[1], m.shape[0]), "paris_hip_set_defect_map")
        return self.defect_map_info()

    def clear_defect_map(self):
        """paris_hip_clear_defect_map: no repair from here on"""
        check(self._L.paris_hip_clear_defect_map(self._ctx), "paris_hip_clear_defect_map")

    def defect_map_info(self):
        """The DefectStats of the current setting (paris_hip_defect_map_info): defects, unrepairable, sources, reach_rows, reach_cols,
        device_bytes"""
        st = DefectStats()
        check(self._L.paris_hip_defect_map_info(self._ctx, C.byref(st)), "paris_hip_defect_map_info")
        return st

    def defect_repair_rows(self, p, row_first=0, row_count=None, frame_stride=0, n_frames=1):
        """The repair of set_defect_map() in place on float frames (paris_hip_defect_repair_rows): the defects in rows [row_first,
        row_first + row_count) of n_frames frames frame_stride bytes apart starting at p. Sources lie up to reach_rows rows outside
        the band: those rows must hold valid pixels. Call it on line integrals, before every weight."""
        count = p.dim_y - row_first if row_count is None else row_count
        check(self._L.paris_hip_defect_repair_rows(self._ctx, p.ptr, p.pitch, frame_stride, n_frames, p.dim_x, p.dim_y, row_first, count),
              "paris_hip_defect_repair_rows")

    # ---- zinger filter ----------------------------------------------------------
    zinger_filter_check = staticmethod(zinger_filter_check)

    def set_zinger_filter(self, threshold_abs, threshold_rel, polarity, dim_x, dim_y, max_hits=0):
        """paris_hip_set_zinger_filter for a dim_x x dim_y detector: zinger_filter_rows() then replaces every pixel that differs from
        the median m of its 3 x 3 window (edges replicated) by more than threshold_abs + threshold_rel * |m| -- above it (polarity +1 /
        "bright"), below it (-1 / "dark") or either (0 / "both") -- with m, unless more than max_hits (0 = default) pixels of the
        frame are flagged. Replaces an earlier setting and its counts safely: work already queued keeps the old one."""
        zf = _zinger_setting(threshold_abs, threshold_rel, polarity, max_hits)
        check(self._L.paris_hip_set_zinger_filter(self._ctx, C.byref(zf), dim_x, dim_y), "paris_hip_set_zinger_filter")

    def clear_zinger_filter(self):
        """paris_hip_clear_zinger_filter: no zinger filter from here on"""
        check(self._L.paris_hip_clear_zinger_filter(self._ctx), "paris_hip_clear_zinger_filter")

    def zinger_filter_rows(self, p, row_first=0, row_count=None, frame_stride=0, n_frames=1):
        """The rule of set_zinger_filter() in place on float frames (paris_hip_zinger_filter_rows): the pixels in rows [row_first,
        row_first + row_count) of n_frames frames frame_stride bytes apart starting at p. Windows reach one row outside the band:
        those rows must hold valid pixels. Every window is read from the frame as it was before the call; not idempotent. Call it
        after the defect repair, before every weight."""
        count = p.dim_y - row_first if row_count is None else row_count
        check(self._L.paris_hip_zinger_filter_rows(self._ctx, p.ptr, p.pitch, frame_stride, n_frames, p.dim_x, p.dim_y, row_first, count),
              "paris_hip_zinger_filter_rows")

    # ---- ring filter ------------------------------------------------------------
    ring_filter_check = staticmethod(ring_filter_check)
    ring_correction_from_mean = staticmethod(ring_correction_from_mean)

    def ring_profile_begin(self, dim_x, dim_y):
        """paris_hip_ring_profile_begin: opens the scan's profile for a dim_x x dim_y detector -- zeroed double sums on the device.
        Replaces an open one safely: work already queued keeps the old sums."""
        check(self._L.paris_hip_ring_profile_begin(self._ctx, dim_x, dim_y), "paris_hip_ring_profile_begin")
        self._ring_shape = (dim_y, dim_x)

    def ring_profile_add_rows(self, p, row_first=0, row_count=None, frame_stride=0, n_frames=1):
        """Adds rows [row_first, row_first + row_count) of n_frames frames frame_stride bytes apart starting at p to the open
        profile, frame after frame (paris_hip_ring_profile_add_rows). The frames are only read. Call it on line integrals, after the
        zinger filter and before every weight."""
        count = p.dim_y - row_first if row_count is None else row_count
        check(self._L.paris_hip_ring_profile_add_rows(self._ctx, p.ptr, p.pitch, frame_stride, n_frames, p.dim_x, p.dim_y, row_first, count),
              "paris_hip_ring_profile_add_rows")

    def ring_profile_finish(self, half_width, floor_abs=0.0, limit_abs=0.0):
        """paris_hip_ring_profile_finish: waits for the ctx stream, forms every pixel's mean over the frames added and applies the
        ring rule to it. Returns (c, mean, RingStats), float32 arrays (n_col, n_row); the profile is closed. Hand c to
        set_ring_correction()."""
        shape = getattr(self, "_ring_shape", None)
        if shape is None:
            raise ParisHipError(_lib.ERROR_INVALID_ARGUMENT, "paris_hip_ring_profile_finish")
        rf = RingFilter(half_width, floor_abs, limit_abs)
        c, mean, st = np.empty(shape, np.float32), np.empty(shape, np.float32), RingStats()
        check(self._L.paris_hip_ring_profile_finish(self._ctx, C.byref(rf), c.ctypes.data, mean.ctypes.data, C.byref(st)),
              "paris_hip_ring_profile_finish")
        self._ring_shape = None
        return c, mean, st

    def ring_profile_discard(self):
        """paris_hip_ring_profile_discard: closes an open profile without a result"""
        check(self._L.paris_hip_ring_profile_discard(self._ctx), "paris_hip_ring_profile_discard")
        self._ring_shape = None

    def set_ring_correction(self, c):
        """paris_hip_set_ring_correction: c is a 2-D array of the detector's size (n_col, n_row), taken as float32, every value
        finite; ring_correct_rows() then subtracts it from frames. Replaces an earlier one safely: work already queued keeps the
        old frame."""
        a = np.ascontiguousarray(c, np.float32)
        if a.ndim != 2:
            raise ValueError("set_ring_correction: c must be a 2-D array (n_col, n_row)")
        check(self._L.paris_hip_set_ring_correction(self._ctx, a.ctypes.data, a.shape[1], a.shape[0]), "paris_hip_set_ring_correction")

    def clear_ring_correction(self):
        """paris_hip_clear_ring_correction: no ring correction from here on"""
        check(self._L.paris_hip_clear_ring_correction(self._ctx), "paris_hip_clear_ring_correction")

    def ring_correct_rows(self, p, row_first=0, row_count=None, frame_stride=0, n_frames=1):
        """p <- p - c in place on float frames (paris_hip_ring_correct_rows): the pixels with c != 0 in rows [row_first, row_first +
        row_count) of n_frames frames frame_stride bytes apart starting at p; every other pixel keeps its bits. Call it after the
        zinger filter, before every weight."""
        count = p.dim_y - row_first if row_count is None else row_count
        check(self._L.paris_hip_ring_correct_rows(self._ctx, p.ptr, p.pitch, frame_stride, n_frames, p.dim_x, p.dim_y, row_first, count),
              "paris_hip_ring_correct_rows")

    # ---- axis search --------------------------------------------------------------
    axis_search_check = staticmethod(axis_search_check)
    axis_search_plan = staticmethod(axis_search_plan)
    axis_estimate_from_costs = staticmethod(axis_estimate_from_costs)

    def axis_search_begin(self, lo, step, count, det_geo, n_frames, rows=2, min_columns=0):
        """paris_hip_axis_search_begin: opens the search for delta_s among `count` candidates lo, lo + step, ... [px] on a full circle
        of n_frames frames of det_geo's detector -- the plan and an n_frames x n_row sinogram on the device. Replaces an open one
        safely: work already queued keeps the old one."""
        s = _axis_setting(lo, step, count, rows, min_columns)
        check(self._L.paris_hip_axis_search_begin(self._ctx, C.byref(s), C.byref(det_geo), n_frames), "paris_hip_axis_search_begin")
        self._axis_shape = (count, n_frames, det_geo.n_row)

    def axis_search_add(self, p, frame_first, frame_stride=0, n_frames=1):
        """Sums the mid-plane band of n_frames frames frame_stride bytes apart starting at p into the sinogram rows frame_first ...
        (paris_hip_axis_search_add_rows). The frames are only read; every frame of the circle is added exactly once, in any order.
        Call it on line integrals, after the zinger filter and before every weight."""
        check(self._L.paris_hip_axis_search_add_rows(self._ctx, p.ptr, p.pitch, frame_stride, n_frames, p.dim_x, p.dim_y, frame_first),
              "paris_hip_axis_search_add_rows")

    def axis_search_finish(self, sinogram=False):
        """paris_hip_axis_search_finish: scores every candidate on the device, waits for the ctx stream and runs the estimate. Returns
        (AxisResult, cost, columns) -- float64 costs (+inf: unscored) and the valid columns per candidate -- and the float32 sinogram
        (n_frames, n_row) as a fourth value when asked for. The search is closed, unless a frame is still missing."""
        shape = getattr(self, "_axis_shape", None)
        if shape is None:
            raise ParisHipError(_lib.ERROR_INVALID_ARGUMENT, "paris_hip_axis_search_finish")
        cost, columns, out = np.empty(shape[0], np.float64), np.empty(shape[0], np.uint32), AxisResult()
        s = np.empty(shape[1:], np.float32) if sinogram else None
        out.scored = 0xFFFFFFFF          # a finish refused before scoring writes no result and leaves the search open
        rc = self._L.paris_hip_axis_search_finish(self._ctx, cost.ctypes.data, columns.ctypes.data, C.byref(out), None if s is None else s.ctypes.data)
        if rc == _lib.SUCCESS or out.scored == 0:
            self._axis_shape = None      # scored -- also when no candidate had a cost -- and closed
        check(rc, "paris_hip_axis_search_finish")
        return (out, cost, columns, s) if sinogram else (out, cost, columns)

    def axis_search_discard(self):
        """paris_hip_axis_search_discard: closes an open search without a result"""
        check(self._L.paris_hip_axis_search_discard(self._ctx), "paris_hip_axis_search_discard")
        self._axis_shape = None

    # ---- detector binning --------------------------------------------------------
    binning_check = staticmethod(binning_check)
    binned_geometry = staticmethod(binned_geometry)
    bin_frame_host = staticmethod(bin_frame_host)
    bin_mask = staticmethod(bin_mask)

    def set_binning(self, bin_x, bin_y, dim_x, dim_y, mask=None):
        """paris_hip_set_binning for dim_x x dim_y source frames: bin_frames() then makes every binned pixel the mean of the good ones
        among its bin_x x bin_y source pixels. mask: a 2-D array of the source detector's size (n_col, n_row), nonzero = bad; None =
        every pixel good. Replaces an earlier setting safely: work already queued keeps the old mask. Returns (out_x, out_y)."""
        m = None if mask is None else _mask_bytes(mask, "set_binning")
        if m is not None and m.shape != (dim_y, dim_x):
            raise ValueError("set_binning: the mask must have the source detector's size (n_col, n_row)")
        bn = Binning(bin_x, bin_y)
        check(self._L.paris_hip_set_binning(self._ctx, C.byref(bn), None if m is None else m.ctypes.data, dim_x, dim_y),
              "paris_hip_set_binning")
        return binning_check(bin_x, bin_y, dim_x, dim_y)

    def clear_binning(self):
        """paris_hip_clear_binning: no binning setting from here on"""
        check(self._L.paris_hip_clear_binning(self._ctx), "paris_hip_clear_binning")

    def bin_frames(self, src, dst, row_first=0, row_count=None, src_frame_stride=0, dst_frame_stride=0, n_frames=1):
        """The rule of set_binning() from float source frames into binned frames (paris_hip_bin_frames): binned rows [row_first,
        row_first + row_count) of n_frames frames dst_frame_stride bytes apart starting at dst, from source rows [bin_y * row_first,
        bin_y * (row_first + row_count)) of the frames src_frame_stride bytes apart starting at src. The source is only read. Call it
        on detector counts, after upload_raw() and before flat_field_rows()."""
        count = dst.dim_y - row_first if row_count is None else row_count
        check(self._L.paris_hip_bin_frames(self._ctx, src.ptr, src.pitch, src_frame_stride, dst.ptr, dst.pitch, dst_frame_stride, n_frames,
                                           src.dim_x, src.dim_y, row_first, count), "paris_hip_bin_frames")

    # ---- detector roll -----------------------------------------------------------
    detector_roll_check = staticmethod(detector_roll_check)
    detector_roll_host = staticmethod(detector_roll_host)
    detector_roll_source_rows = staticmethod(detector_roll_source_rows)
    roll_search_check = staticmethod(roll_search_check)
    roll_estimate_from_costs = staticmethod(roll_estimate_from_costs)

    def set_detector_roll(self, eta_deg, det_geo):
        """paris_hip_set_detector_roll for det_geo's detector: detector_roll() then resamples every frame onto a detector rotated back
        by eta_deg degrees about the projected rotation axis. Replaces an earlier setting; work already queued keeps the old one."""
        s = DetectorRoll(eta_deg)
        check(self._L.paris_hip_set_detector_roll(self._ctx, C.byref(s), C.byref(det_geo)), "paris_hip_set_detector_roll")

    def clear_detector_roll(self):
        """paris_hip_clear_detector_roll: no detector roll from here on"""
        check(self._L.paris_hip_clear_detector_roll(self._ctx), "paris_hip_clear_detector_roll")

    def detector_roll(self, src, dst, rows=None, src_frame_stride=0, dst_frame_stride=0, n_frames=1, eta_deg=None, det_geo=None):
        """The rule of set_detector_roll() from float frames into frames of the same size (paris_hip_detector_roll_rows): rows
        (first, count) -- None: every row -- of the n_frames frames dst_frame_stride bytes apart starting at dst, from the frames
        src_frame_stride bytes apart starting at src, of which only the rows detector_roll_source_rows() names are read. With eta_deg
        and det_geo the setting is taken from the arguments and the backend's is neither used nor changed
        (paris_hip_detector_roll_rows_with). Call it on line integrals, after the beam-hardening correction and before every weight."""
        first, count = (0, dst.dim_y) if rows is None else rows
        if eta_deg is None:
            check(self._L.paris_hip_detector_roll_rows(self._ctx, src.ptr, src.pitch, src_frame_stride, dst.ptr, dst.pitch, dst_frame_stride,
                                                       n_frames, src.dim_x, src.dim_y, first, count), "paris_hip_detector_roll_rows")
            return
        s = DetectorRoll(eta_deg)
        check(self._L.paris_hip_detector_roll_rows_with(self._ctx, src.ptr, src.pitch, src_frame_stride, dst.ptr, dst.pitch, dst_frame_stride,
                                                        n_frames, src.dim_x, src.dim_y, first, count, C.byref(s), C.byref(det_geo)),
              "paris_hip_detector_roll_rows_with")

    def find_detector_roll(self, mean, lo, step, count, det_geo, min_pixels=0):
        """paris_hip_roll_search_run: finds the detector roll from the scan mean of a full equidistant circle of line integrals on a
        centred detector -- mean: (n_col, n_row), what ring_profile_finish() returns -- by the mirror symmetry of that mean about the
        projected axis. Candidates (float)(lo + k step) degrees, k < count. Returns (RollResult, cost, pairs): float64 costs (+inf:
        unscored) and the pairs summed per candidate. Waits for the ctx stream."""
        m = np.ascontiguousarray(mean, np.float32)
        if m.shape != (det_geo.n_col, det_geo.n_row):
            raise ValueError("find_detector_roll: the mean must have the detector's size (n_col, n_row)")
        n = max(int(count), 0)
        s, out, cost, pairs = RollSearch(lo, step, n, min_pixels), RollResult(), np.empty(n, np.float64), np.empty(n, np.uint64)
        check(self._L.paris_hip_roll_search_run(self._ctx, C.byref(s), C.byref(det_geo), m.ctypes.data, cost.ctypes.data, pairs.ctypes.data,
                                                C.byref(out)), "paris_hip_roll_search_run")
        return out, cost, pairs

    # ---- air region --------------------------------------------------------------
    air_region_check = staticmethod(air_region_check)
    air_value_host = staticmethod(air_value_host)

    def set_air_region(self, x0, y0, width, height, dim_x, dim_y, min_pixels=0, limit_abs=0.0, mask=None):
        """paris_hip_set_air_region for dim_x x dim_y frames: air_normalize() then subtracts from every frame the mean line integral
        of the rectangle columns [x0, x0 + width), rows [y0, y0 + height) -- the frame's flux drift against the flat. mask: a 2-D
        array of the detector's size (n_col, n_row), nonzero = bad; None = every pixel good. Replaces an earlier setting and its
        counts safely: work already queued keeps the old one."""
        m = None if mask is None else _mask_bytes(mask, "set_air_region")
        if m is not None and m.shape != (dim_y, dim_x):
            raise ValueError("set_air_region: the mask must have the detector's size (n_col, n_row)")
        ar = _air_setting(x0, y0, width, height, min_pixels, limit_abs)
        check(self._L.paris_hip_set_air_region(self._ctx, C.byref(ar), None if m is None else m.ctypes.data, dim_x, dim_y),
              "paris_hip_set_air_region")

    def clear_air_region(self):
        """paris_hip_clear_air_region: no air region from here on"""
        check(self._L.paris_hip_clear_air_region(self._ctx), "paris_hip_clear_air_region")

    def air_normalize(self, p, frame_stride=0, n_frames=1, rows=None):
        """The rule of set_air_region() in place on float frames (paris_hip_air_normalize_rows): every frame's value a_f is measured
        from the rectangle, then rows (first, count) -- None: every row -- of the n_frames frames frame_stride bytes apart starting at
        p become p - a_f; a frame whose a_f is zero keeps its bits. The rectangle's rows must hold corrected pixels. Call it on line
        integrals, directly after the dark / flat correction and before the defect repair."""
        first, count = (0, p.dim_y) if rows is None else rows
        check(self._L.paris_hip_air_normalize_rows(self._ctx, p.ptr, p.pitch, frame_stride, n_frames, p.dim_x, p.dim_y, first, count),
              "paris_hip_air_normalize_rows")

    def air_measure(self, p, frame_stride=0, n_frames=1):
        """paris_hip_air_measure: the values air_normalize() would subtract, and the counting pixels, of n_frames frames frame_stride
        bytes apart starting at p -- (float32[n_frames], uint32[n_frames]). Nothing is written to the frames or added to the
        counts. Waits for the ctx stream."""
        a, n = np.empty(n_frames, np.float32), np.empty(n_frames, np.uint32)
        check(self._L.paris_hip_air_measure(self._ctx, p.ptr, p.pitch, frame_stride, n_frames, p.dim_x, p.dim_y, a.ctypes.data, n.ctypes.data),
              "paris_hip_air_measure")
        return a, n

    def air_stats(self, reset=False):
        """The AirCounts of the air_normalize() calls since set_air_region() or the last reset (paris_hip_air_stats): frames,
        normalised, too_few, above_limit, min_a, max_a. Waits for the ctx stream."""
        st = AirCounts()
        check(self._L.paris_hip_air_stats(self._ctx, C.byref(st), 1 if reset else 0), "paris_hip_air_stats")
        return st

    # ---- scatter correction --------------------------------------------------------
    scatter_default_margin = staticmethod(scatter_default_margin)
    scatter_correction_check = staticmethod(scatter_correction_check)
    scatter_correction_host = staticmethod(scatter_correction_host)

    def set_scatter_correction(self, setting, dim_x, dim_y, l_x, l_y):
        """paris_hip_set_scatter_correction for dim_x x dim_y frames with pixel pitches l_x, l_y; setting is a ScatterCorrection (or
        the nine values of one): scatter_correction() then solves T_m = T + (q(T) (*) g) for the primary of whole frames. Twiddles,
        tables and scratch live on the device and count towards projection_reserve_bytes. Replaces an earlier setting; work already
        queued keeps the old one."""
        s = setting if isinstance(setting, ScatterCorrection) else ScatterCorrection(*setting)
        check(self._L.paris_hip_set_scatter_correction(self._ctx, C.byref(s), dim_x, dim_y, l_x, l_y), "paris_hip_set_scatter_correction")

    def clear_scatter_correction(self):
        """paris_hip_clear_scatter_correction: no scatter correction from here on"""
        check(self._L.paris_hip_clear_scatter_correction(self._ctx), "paris_hip_clear_scatter_correction")

    def scatter_correction(self, p, frame_stride=0, n_frames=1):
        """The rule of set_scatter_correction() in place on whole float frames of line integrals (paris_hip_scatter_correction_frames):
        the n_frames frames frame_stride bytes apart starting at p. Call it after the ring correction and before the phase retrieval.
        A frame's result does not depend on the other frames of the call."""
        check(self._L.paris_hip_scatter_correction_frames(self._ctx, p.ptr, p.pitch, frame_stride, n_frames, p.dim_x, p.dim_y),
              "paris_hip_scatter_correction_frames")

    # ---- starvation filter ---------------------------------------------------------
    starvation_filter_check = staticmethod(starvation_filter_check)
    starvation_filter_tables = staticmethod(starvation_filter_tables)
    starvation_filter_host = staticmethod(starvation_filter_host)

    def set_starvation_filter(self, setting, dim_x, dim_y):
        """paris_hip_set_starvation_filter for dim_x x dim_y frames; setting is a StarvationFilter (or p0, gain, radius):
        starvation_filter() then smooths whole frames where the line integral lies above p0. Counters, tables and scratch live on the
        device and count towards projection_reserve_bytes. Replaces an earlier setting; work already queued keeps the old one."""
        s = _starvation_filter(setting)
        check(self._L.paris_hip_set_starvation_filter(self._ctx, C.byref(s), dim_x, dim_y), "paris_hip_set_starvation_filter")

    def clear_starvation_filter(self):
        """paris_hip_clear_starvation_filter: no starvation filter from here on"""
        check(self._L.paris_hip_clear_starvation_filter(self._ctx), "paris_hip_clear_starvation_filter")

    def starvation_filter(self, p, frame_stride=0, n_frames=1):
        """The rule of set_starvation_filter() in place on whole float frames of line integrals (paris_hip_starvation_filter_frames):
        the n_frames frames frame_stride bytes apart starting at p. Call it after the ring correction and before the scatter
        correction. A frame's result does not depend on the other frames of the call."""
        check(self._L.paris_hip_starvation_filter_frames(self._ctx, p.ptr, p.pitch, frame_stride, n_frames, p.dim_x, p.dim_y),
              "paris_hip_starvation_filter_frames")

    def starvation_stats(self, reset=False):
        """The StarvationCounts since set_starvation_filter() or the last reset (paris_hip_starvation_stats): frames, filtered,
        last_level. Waits for the ctx stream."""
        st = StarvationCounts()
        check(self._L.paris_hip_starvation_stats(self._ctx, C.byref(st), 1 if reset else 0), "paris_hip_starvation_stats")
        return st

    # ---- phase retrieval -----------------------------------------------------------
    phase_alpha = staticmethod(phase_alpha)
    phase_default_margin = staticmethod(phase_default_margin)
    phase_retrieval_check = staticmethod(phase_retrieval_check)
    phase_retrieval_host = staticmethod(phase_retrieval_host)

    def set_phase_retrieval(self, alpha_mm2, t_min, margin, dim_x, dim_y, l_x, l_y):
        """paris_hip_set_phase_retrieval for dim_x x dim_y frames with pixel pitches l_x, l_y: phase_retrieval() then low-passes the
        transmission of whole frames with 1 / (1 + alpha f^2). Twiddles, tables and scratch live on the device and count towards
        projection_reserve_bytes. Replaces an earlier setting; work already queued keeps the old one."""
        s = PhaseRetrieval(alpha_mm2, t_min, margin)
        check(self._L.paris_hip_set_phase_retrieval(self._ctx, C.byref(s), dim_x, dim_y, l_x, l_y), "paris_hip_set_phase_retrieval")

    def clear_phase_retrieval(self):
        """paris_hip_clear_phase_retrieval: no phase retrieval from here on"""
        check(self._L.paris_hip_clear_phase_retrieval(self._ctx), "paris_hip_clear_phase_retrieval")

    def phase_retrieval(self, p, frame_stride=0, n_frames=1):
        """The rule of set_phase_retrieval() in place on whole float frames of line integrals (paris_hip_phase_retrieval_frames):
        the n_frames frames frame_stride bytes apart starting at p. Call it after the ring correction and before the beam-hardening
        polynomial. A frame's result does not depend on the other frames of the call."""
        check(self._L.paris_hip_phase_retrieval_frames(self._ctx, p.ptr, p.pitch, frame_stride, n_frames, p.dim_x, p.dim_y),
              "paris_hip_phase_retrieval_frames")

    # ---- beam hardening ------------------------------------------------------------
    beam_hardening_check = staticmethod(beam_hardening_check)
    beam_hardening_host = staticmethod(beam_hardening_host)
    bh_threshold_from_histogram = staticmethod(bh_threshold_from_histogram)
    bh_gram_host = staticmethod(bh_gram_host)
    bh_solve = staticmethod(bh_solve)

    def set_beam_hardening(self, c, dim_x, dim_y):
        """paris_hip_set_beam_hardening for dim_x x dim_y frames: beam_hardening() then turns every line integral p into
        q = c_1 p + ... + c_N p^N (c: 1 to 4 finite coefficients, c_1 first). Replaces an earlier setting; work already queued keeps
        the old one."""
        s = _bh_setting(c)
        check(self._L.paris_hip_set_beam_hardening(self._ctx, C.byref(s), dim_x, dim_y), "paris_hip_set_beam_hardening")

    def clear_beam_hardening(self):
        """paris_hip_clear_beam_hardening: no beam-hardening correction from here on"""
        check(self._L.paris_hip_clear_beam_hardening(self._ctx), "paris_hip_clear_beam_hardening")

    def beam_hardening(self, p, frame_stride=0, n_frames=1, rows=None, c=None):
        """The rule of set_beam_hardening() in place on float frames (paris_hip_beam_hardening_rows): rows (first, count) -- None:
        every row -- of the n_frames frames frame_stride bytes apart starting at p. With c the coefficients are taken from the
        argument and the backend's setting is neither used nor changed (paris_hip_beam_hardening_rows_with). Call it on line
        integrals, after the ring correction and before every weight."""
        first, count = (0, p.dim_y) if rows is None else rows
        if c is None:
            check(self._L.paris_hip_beam_hardening_rows(self._ctx, p.ptr, p.pitch, frame_stride, n_frames, p.dim_x, p.dim_y, first, count),
                  "paris_hip_beam_hardening_rows")
            return
        s = _bh_setting(c)
        check(self._L.paris_hip_beam_hardening_rows_with(self._ctx, C.byref(s), p.ptr, p.pitch, frame_stride, n_frames, p.dim_x, p.dim_y,
                                                         first, count), "paris_hip_beam_hardening_rows_with")

    # ---- detector lag ---------------------------------------------------------------
    lag_model_check = staticmethod(lag_model_check)
    lag_coefficients = staticmethod(lag_coefficients)
    lag_correct_host = staticmethod(lag_correct_host)

    def set_lag_correction(self, terms, start="steady"):
        """paris_hip_set_lag_correction: terms is 1 to 4 pairs (b_n, a_n) of the detector's multi-exponential impulse response, start
        "steady" (the beam was on before the first frame: the default) or "rest". Runs what is deferred first; replaces an earlier
        setting and closes an open sequence."""
        m = _lag_setting(terms, start)
        check(self._L.paris_hip_set_lag_correction(self._ctx, C.byref(m)), "paris_hip_set_lag_correction")

    def clear_lag_correction(self):
        """paris_hip_clear_lag_correction: no lag correction from here on; an open sequence is closed"""
        check(self._L.paris_hip_clear_lag_correction(self._ctx), "paris_hip_clear_lag_correction")

    def lag_begin(self, dim_x, dim_y, row_first=0, row_count=None):
        """paris_hip_lag_begin: opens the sequence of rows [row_first, row_first + row_count) -- None: to the last row -- of dim_x x
        dim_y frames: the band's zeroed state on the device, frame counter 0. One open sequence per backend."""
        count = dim_y - row_first if row_count is None else row_count
        check(self._L.paris_hip_lag_begin(self._ctx, dim_x, dim_y, row_first, count), "paris_hip_lag_begin")

    def lag_correct(self, p, frame_stride=0, n_frames=1, row_first=0, row_count=None):
        """The lag rule in place on float frames of counts (paris_hip_lag_correct_rows): the begun band of the n_frames frames
        frame_stride bytes apart starting at p, which follow the previous call's frames in time. Call it after the raw upload and
        the binning, before flat_field_rows()."""
        count = p.dim_y - row_first if row_count is None else row_count
        check(self._L.paris_hip_lag_correct_rows(self._ctx, p.ptr, p.pitch, frame_stride, n_frames, p.dim_x, p.dim_y, row_first, count),
              "paris_hip_lag_correct_rows")

    def lag_end(self):
        """paris_hip_lag_end: closes the open sequence (none open: nothing happens)"""
        check(self._L.paris_hip_lag_end(self._ctx), "paris_hip_lag_end")

    def lag_frames(self):
        """paris_hip_lag_frames: how many frames the open sequence has seen (0 without one)"""
        n = C.c_uint64(0)
        check(self._L.paris_hip_lag_frames(self._ctx, C.byref(n)), "paris_hip_lag_frames")
        return int(n.value)

    # ---- metal artefact reduction ---------------------------------------------------
    metal_check = staticmethod(metal_check)
    metal_collect_host = staticmethod(metal_collect_host)
    metal_trace_pack_host = staticmethod(metal_trace_pack_host)
    metal_inpaint_host = staticmethod(metal_inpaint_host)

    def metal_collect(self, v, threshold, max_n=None, binarize=False):
        """paris_hip_metal_collect of the device volume v: (index uint64[n], value float32[n]) of the voxels above threshold in
        ascending linear index -- bit for bit metal_collect_host(). binarize: v then holds 1.0 where a voxel was listed and 0.0
        elsewhere. max_n None: the cap of metal_check(). More than max_n hits raise ParisHipError with the status
        ERROR_METAL_TOO_MANY_VOXELS and the count as .n; v is then as it was. Runs what is deferred first and waits."""
        cap = metal_check(v.dim_x, v.dim_y, v.dim_z, threshold) if max_n is None else int(max_n)
        room = min(cap, v.dim_x * v.dim_y * v.dim_z)
        index, value, n = np.empty(room, np.uint64), np.empty(room, np.float32), C.c_uint64(0)
        status = self._L.paris_hip_metal_collect(self._ctx, v.ptr, v.dim_x, v.dim_y, v.dim_z, threshold, room,
                                                 index.ctypes.data if room else None, value.ctypes.data if room else None, C.byref(n),
                                                 1 if binarize else 0)
        _metal_collect_check(status, n.value, "paris_hip_metal_collect")
        return index[:n.value].copy(), value[:n.value].copy()

    def metal_trace_pack(self, p, min_path, grow=0, frame_stride=0, n_frames=1):
        """paris_hip_metal_trace_pack of n_frames device frames frame_stride bytes apart starting at p: the packed trace
        uint64[(n_frames, dim_y, words)] -- bit for bit metal_trace_pack_host(). Waits for the result."""
        bits = np.zeros((n_frames, p.dim_y, metal_words(p.dim_x)), np.uint64)
        check(self._L.paris_hip_metal_trace_pack(self._ctx, p.ptr, p.pitch, frame_stride, n_frames, p.dim_x, p.dim_y, min_path, grow,
                                                 bits.ctypes.data if bits.size else None), "paris_hip_metal_trace_pack")
        return bits

    def set_metal_trace(self, bits, dim_x):
        """paris_hip_set_metal_trace: bits uint64[(n_views, dim_y, words)] are the packed traces of every view of a scan on frames of
        dim_x x dim_y pixels; metal_inpaint() reads them on the device. Replaces an earlier setting and its counts safely."""
        b = np.ascontiguousarray(bits, np.uint64)
        if b.ndim != 3 or b.shape[2] != metal_words(dim_x):
            raise ValueError("set_metal_trace: bits must be (n_views, dim_y, words) for rows of dim_x pixels")
        check(self._L.paris_hip_set_metal_trace(self._ctx, b.ctypes.data if b.size else None, b.shape[0], dim_x, b.shape[1]),
              "paris_hip_set_metal_trace")

    def clear_metal_trace(self):
        """paris_hip_clear_metal_trace: no trace from here on; metal_inpaint() refuses"""
        check(self._L.paris_hip_clear_metal_trace(self._ctx), "paris_hip_clear_metal_trace")

    def metal_inpaint(self, p, view=None, row_first=0, row_count=None, frame_stride=0, n_frames=1):
        """The inpainting of set_metal_trace() in place on float frames (paris_hip_metal_inpaint_rows): in rows [row_first, row_first +
        row_count) of n_frames frames frame_stride bytes apart starting at p every run of the trace is replaced by the linear
        interpolation between the pixels beside it. view: the trace of each frame -- a number or a sequence; None: p.idx. Call it on
        line integrals after the detector roll, before every weight."""
        count = p.dim_y - row_first if row_count is None else row_count
        views = np.atleast_1d(np.asarray(p.idx if view is None else view, np.int64))
        if views.ndim != 1 or len(views) != n_frames or (views < 0).any() or (views > 0xffffffff).any():
            raise ParisHipError(_lib.ERROR_INVALID_ARGUMENT, "paris_hip_metal_inpaint_rows")
        h = views.astype(np.uint32)
        check(self._L.paris_hip_metal_inpaint_rows(self._ctx, p.ptr, p.pitch, frame_stride, n_frames, p.dim_x, p.dim_y, row_first, count,
                                                   h.ctypes.data if n_frames else None), "paris_hip_metal_inpaint_rows")

    def metal_stats(self, reset=False):
        """The MetalCounts since set_metal_trace() or the last reset (paris_hip_metal_stats): replaced, runs, rows_left. Waits for the
        ctx stream."""
        st = MetalCounts()
        check(self._L.paris_hip_metal_stats(self._ctx, C.byref(st), 1 if reset else 0), "paris_hip_metal_stats")
        return st

    def set_metal_voxels(self, index, value):
        """paris_hip_set_metal_voxels: the list of metal_collect() -- strictly ascending indices and their values -- for
        metal_reinsert()"""
        i, x = np.ascontiguousarray(index, np.uint64), np.ascontiguousarray(value, np.float32)
        if i.ndim != 1 or i.shape != x.shape:
            raise ValueError("set_metal_voxels: index and value must be 1-D arrays of one length")
        check(self._L.paris_hip_set_metal_voxels(self._ctx, i.ctypes.data if i.size else None, x.ctypes.data if x.size else None, i.size),
              "paris_hip_set_metal_voxels")

    def clear_metal_voxels(self):
        """paris_hip_clear_metal_voxels: no list from here on; metal_reinsert() refuses"""
        check(self._L.paris_hip_clear_metal_voxels(self._ctx), "paris_hip_clear_metal_voxels")

    def metal_reinsert(self, v, v_offset=0, dim_x=None, dim_y=None):
        """paris_hip_metal_reinsert: the listed voxels that fall into the device slab v -- slices [v_offset, v_offset + v.dim_z) of a
        grid with v.dim_x x v.dim_y voxels per slice -- get their listed values. Runs what is deferred first; does not wait."""
        check(self._L.paris_hip_metal_reinsert(self._ctx, v.ptr, v.dim_x if dim_x is None else dim_x, v.dim_y if dim_y is None else dim_y,
                                               v.dim_z, v_offset), "paris_hip_metal_reinsert")

    def reduce_metal(self, frames, det_geo, threshold, grow=1, min_path=None, prepare=None, vol_geo=None, enable_angles=False, angles=None):
        """Linear-interpolation metal artefact reduction, the part before the second reconstruction. frames: the scan's line
        integrals, one 2-D float32 array (n_col, n_row) per view, in view order. They are reconstructed once -- upload,
        prepare(backend, projection) if given (the redundancy weights of a short or offset scan), weight, filter, backprojection --
        into the whole grid vol_geo (None: the natural volume of det_geo); the voxels above threshold (in the volume's own units) are
        collected and the volume binarized; the mask is forward-projected view by view and each projection packed with min_path (mm;
        None: half the smallest voxel edge) and grow; the traces are installed with set_metal_trace() and the list with
        set_metal_voxels(). Returns a MetalTrace. The caller's loop then calls metal_inpaint(p, view) before weight() and
        metal_reinsert() on the finished volume. Every device buffer made here is freed before the call returns; raises
        ParisHipError where the library refuses."""
        vg = vol_geo if vol_geo is not None else calculate_volume_geometry(det_geo)
        path = 0.5 * min(vg.l_vx_x, vg.l_vx_y, vg.l_vx_z) if min_path is None else min_path
        metal_check(vg.dim_x, vg.dim_y, vg.dim_z, threshold, grow, path)
        vol, d_p = self.make_volume_device(vg.dim_x, vg.dim_y, vg.dim_z), None
        try:
            self.memset_volume(vol)
            n_views = 0
            for i, frame in enumerate(frames):
                f = np.ascontiguousarray(frame, np.float32)
                d_p = load(self, Projection(f, det_geo.n_row, det_geo.n_col, idx=i, phi=0.0 if angles is None else float(angles[i])))
                if prepare is not None:
                    prepare(self, d_p)
                weight(self, d_p, det_geo)
                filter(self, d_p, det_geo)
                backproject(self, d_p, vol, 0, det_geo, vg, enable_angles, False, None)
                self.free(d_p)
                d_p = None
                n_views += 1
            index, value = self.metal_collect(vol, threshold, binarize=True)
            bits = np.zeros((n_views, det_geo.n_col, metal_words(det_geo.n_row)), np.uint64)
            d_p = self.make_projection_device(det_geo.n_row, det_geo.n_col)
            for i in range(n_views):
                d_p.idx, d_p.phi = i, 0.0 if angles is None else float(angles[i])
                forward_project(self, vol, 0, d_p, det_geo, vg, enable_angles)
                bits[i] = self.metal_trace_pack(d_p, path, grow)[0]
            self.set_metal_trace(bits, det_geo.n_row)
            self.set_metal_voxels(index, value)
            pixels = int(sum(bin(int(w)).count("1") for w in bits.ravel()[np.flatnonzero(bits.ravel())]))
            return MetalTrace(index=index, value=value, bits=bits, trace_pixels=pixels, threshold=threshold, grow=grow, min_path=path)
        finally:
            self.flush()
            self.synchronize()
            if d_p is not None:
                self.free(d_p)
            self.free(vol)

    def make_labels_device(self, dim_x, dim_y, dim_z):
        """one byte per voxel of a slab, uninitialised; free() takes it"""
        return Labels(self.make_volume_device((dim_x * dim_y * dim_z + 3) // 4, 1, 1), dim_x, dim_y, dim_z)

    def labels_from_host(self, labels):
        """a uint8 array (dim_z, dim_y, dim_x) as Labels on the device"""
        h = np.ascontiguousarray(labels, np.uint8)
        if h.ndim != 3:
            raise ValueError("labels_from_host: the labels must be a 3-D array (dim_z, dim_y, dim_x)")
        d = self.make_labels_device(h.shape[2], h.shape[1], h.shape[0])
        words = np.zeros(d._store.dim_x, np.float32)
        words.view(np.uint8)[:h.size] = h.ravel()
        check(self._L.paris_hip_memcpy_volume_h2d(self._ctx, d.ptr, words.ctypes.data, d._store.dim_x, 1, 1), "paris_hip_memcpy_volume_h2d")
        self.synchronize()
        return d

    def labels_to_host(self, labels):
        """the Labels as a uint8 array (dim_z, dim_y, dim_x); waits for the ctx stream"""
        words = np.empty(labels._store.dim_x, np.float32)
        check(self._L.paris_hip_memcpy_volume_d2h(self._ctx, words.ctypes.data, labels.ptr, labels._store.dim_x, 1, 1),
              "paris_hip_memcpy_volume_d2h")
        self.synchronize()
        return words.view(np.uint8)[:labels.size].reshape(labels.dim_z, labels.dim_y, labels.dim_x).copy()

    def bh_classify(self, v, thr, margin, labels=None):
        """paris_hip_bh_classify of the device slab v: label 2 (object, v > thr) or 1 (air, v <= thr) for every voxel whose whole
        neighbourhood of Chebyshev radius margin (0 .. 4) lies in the slab and has its class and which lies inside the field of
        view, 0 otherwise. Returns the Labels (made here unless given). Runs what is deferred first; does not wait."""
        out = labels if labels is not None else self.make_labels_device(v.dim_x, v.dim_y, v.dim_z)
        if (out.dim_x, out.dim_y, out.dim_z) != (v.dim_x, v.dim_y, v.dim_z):
            raise ValueError("bh_classify: the labels and the slab differ in size")
        status = self._L.paris_hip_bh_classify(self._ctx, v.ptr, v.dim_x, v.dim_y, v.dim_z, thr, margin, out.ptr)
        if status != _lib.SUCCESS and labels is None:
            self.free(out)
        check(status, "paris_hip_bh_classify")
        return out

    def bh_gram(self, basis, labels):
        """paris_hip_bh_gram: the Gram sums of (f_1 ... f_N, m) over the labelled voxels of the device slabs basis[0 .. N) -- bit for
        bit bh_gram_host() of the same data. Returns (float64[(N + 1)(N + 2) / 2], BhCounts). Waits for the result."""
        n = len(basis)
        if any((f.dim_x, f.dim_y, f.dim_z) != (labels.dim_x, labels.dim_y, labels.dim_z) for f in basis):
            raise ValueError("bh_gram: the basis slabs and the labels differ in size")
        ptrs = (C.c_void_p * max(n, 1))(*[f.ptr for f in basis])
        g, cnt = np.zeros(_bh_terms(n), np.float64), BhCounts()
        check(self._L.paris_hip_bh_gram(self._ctx, ptrs, n, labels.ptr, labels.size, g.ctypes.data, C.byref(cnt)), "paris_hip_bh_gram")
        return g, cnt

    def fit_beam_hardening(self, frames, det_geo, degree=2, margin=2, slices=None, vol_geo=None, min_voxels=0, prepare=None,
                           enable_angles=False, angles=None):
        """Empirical cupping correction: fits the coefficients of set_beam_hardening() from the scan itself. frames: the scan's line
        integrals, one 2-D float32 array (n_col, n_row) per view, in view order, as they are after the ring correction. For each view
        and each k = 1 .. degree the frame is uploaded, turned into p^k by the pass with the unit setting e_k, handed to
        prepare(backend, projection) if given (the redundancy weights of a short or offset scan), weighted, filtered and
        backprojected into the k-th basis slab: slices (first, count) of vol_geo's volume -- None: every slice; vol_geo None: the
        natural volume of det_geo. Then Otsu's threshold of f_1, the labels with the given margin, the Gram sums and the solve
        (DESIGN.md section 4.17). Returns a BeamHardeningFit; raises ParisHipError where the library refuses. The backend's own
        beam-hardening setting is neither used nor changed; every device buffer made here is freed before the call returns."""
        vg = vol_geo if vol_geo is not None else calculate_volume_geometry(det_geo)
        first, count = (0, vg.dim_z) if slices is None else slices
        if degree < 1 or degree > _lib.BH_DEGREE_MAX or count < 1 or first < 0 or first + count > vg.dim_z:
            raise ParisHipError(_lib.ERROR_INVALID_ARGUMENT, "fit_beam_hardening")
        slabs, labels = [], None
        try:
            for _ in range(degree):
                slabs.append(self.make_volume_device(vg.dim_x, vg.dim_y, count))
                self.memset_volume(slabs[-1])
            for i, frame in enumerate(frames):
                f = np.ascontiguousarray(frame, np.float32)
                for k in range(degree):
                    h = Projection(f, det_geo.n_row, det_geo.n_col, idx=i, phi=0.0 if angles is None else float(angles[i]))
                    d_p = load(self, h)
                    try:
                        self.beam_hardening(d_p, c=[0.0] * k + [1.0])
                        if prepare is not None:
                            prepare(self, d_p)
                        weight(self, d_p, det_geo)
                        filter(self, d_p, det_geo)
                        backproject(self, d_p, slabs[k], first, det_geo, vg, enable_angles, False, None)
                    finally:
                        self.free(d_p)
            st, _ = self.volume_stats(slabs[0])
            st, hist = self.volume_stats(slabs[0], st.min, st.max, _lib.BH_HISTOGRAM_BINS)
            thr = bh_threshold_from_histogram(hist, st.min, st.max)
            labels = self.bh_classify(slabs[0], thr, margin)
            gram, counts = self.bh_gram(slabs, labels)
            fit = bh_solve(gram, degree, counts, min_voxels)
            return BeamHardeningFit(c=np.array(fit.setting.c[:degree], np.float32), level=fit.level, residual_before=fit.residual_before,
                                    residual_after=fit.residual_after, threshold=thr, counts=counts, gram=gram,
                                    labels=self.labels_to_host(labels), slices=(first, count))
        finally:
            self.flush()
            self.synchronize()
            for v in slabs:
                self.free(v)
            if labels is not None:
                self.free(labels._store)

    # ---- row extension -----------------------------------------------------------
    row_extension_check = staticmethod(row_extension_check)
    row_extension_response = staticmethod(row_extension_response)

    def set_row_extension(self, edge_pixels, taper_pixels):
        """paris_hip_set_row_extension: from here on every row filter acts as if each row continued beyond either edge as the mean of
        its edge_pixels (1, 2, 4 or 8) outermost pixels times a cos^2 taper of taper_pixels pixels -- for laterally truncated
        projections. Runs what is held back or pending first."""
        re = RowExtension(edge_pixels, taper_pixels)
        check(self._L.paris_hip_set_row_extension(self._ctx, C.byref(re)), "paris_hip_set_row_extension")

    def clear_row_extension(self):
        """paris_hip_clear_row_extension: zero padding from here on"""
        check(self._L.paris_hip_clear_row_extension(self._ctx), "paris_hip_clear_row_extension")

    def zinger_stats(self, reset=False):
        """The ZingerCounts since set_zinger_filter() or the last reset (paris_hip_zinger_stats): frames, replaced, saturated_frames.
        Waits for the ctx stream."""
        st = ZingerCounts()
        check(self._L.paris_hip_zinger_stats(self._ctx, C.byref(st), 1 if reset else 0), "paris_hip_zinger_stats")
        return st

    def copy_d2h(self, d, h):
        if isinstance(d, Projection):
            assert h.buf.dtype == np.float32 and h.dim_x == d.dim_x and h.dim_y == d.dim_y
            check(self._L.paris_hip_memcpy_projection_d2h(self._ctx, h.ptr, h.buf.strides[0], d.ptr, d.pitch,
                                                          d.dim_x, d.dim_y), "paris_hip_memcpy_projection_d2h")
            h.idx, h.phi = d.idx, d.phi
        else:
            assert h.buf.dtype == np.float32 and (h.dim_x, h.dim_y, h.dim_z) == (d.dim_x, d.dim_y, d.dim_z)
            check(self._L.paris_hip_memcpy_volume_d2h(self._ctx, h.ptr, d.ptr, d.dim_x, d.dim_y, d.dim_z),
                  "paris_hip_memcpy_volume_d2h")
            h.off = d.off
        self.synchronize()

    def make_subvolume_information(self, vol_geo, det_geo, n_devices=0):
        """src/cuda/subvolume_information.cpp:63-118"""
        out = SubvolumeInfo()
        check(self._L.paris_hip_make_subvolume_information(C.byref(vol_geo), C.byref(det_geo), n_devices,
                                                           C.byref(out)), "paris_hip_make_subvolume_information")
        return out

    # ---- the three numeric stages --------------------------------------------------------------------------
    def weight(self, p, h_min, v_min, d_sd, l_px_row, l_px_col):
        """backend::weight (src/openmp/weighting.cpp:32-57)"""
        check(self._L.paris_hip_weight(self._ctx, p.ptr, p.pitch, p.dim_x, p.dim_y, h_min, v_min, d_sd,
                                       l_px_row, l_px_col), "paris_hip_weight")

    def short_scan_weight(self, p, det_geo, scan, phi_deg, row_first=0, row_count=None, frame_stride=0):
        """Parker redundancy weighting of a short scan (paris_hip_short_scan_weight_rows), on the raw frame before weight():
        rows [row_first, row_first + row_count) of each column i are multiplied by 2 w(beta, gamma_i). scan is a ShortScan or
        (start_deg, range_deg); phi_deg is the projection angle in degrees as the backprojection resolves it, or a sequence of
        them for len(phi_deg) frames frame_stride bytes apart starting at p (one launch)."""
        if not isinstance(scan, ShortScan):
            scan = ShortScan(*scan)
        phis = np.atleast_1d(np.asarray(phi_deg, np.float32))
        count = p.dim_y - row_first if row_count is None else row_count
        check(self._L.paris_hip_short_scan_weight_rows(self._ctx, p.ptr, p.pitch, frame_stride, len(phis), p.dim_x, p.dim_y, row_first,
                                                       count, C.byref(det_geo), C.byref(scan),
                                                       phis.ctypes.data_as(C.POINTER(C.c_float))),
              "paris_hip_short_scan_weight_rows")

    def offset_detector_weight(self, p, det_geo, row_first=0, row_count=None, frame_stride=0, n_frames=1):
        """Redundancy weighting of an offset-detector (half-fan) full circle (paris_hip_offset_detector_weight_rows), on the raw
        frame before weight(): rows [row_first, row_first + row_count) of each column i of n_frames frames frame_stride bytes
        apart, starting at p, are multiplied by 2 w(gamma_i); the weight does not depend on the angle."""
        count = p.dim_y - row_first if row_count is None else row_count
        check(self._L.paris_hip_offset_detector_weight_rows(self._ctx, p.ptr, p.pitch, frame_stride, n_frames, p.dim_x, p.dim_y, row_first,
                                                            count, C.byref(det_geo)), "paris_hip_offset_detector_weight_rows")

    def make_filter(self, size, tau, window=0):
        """backend::make_filter (src/openmp/filtering.cpp:139-165); window 1 = Shepp-Logan (extension)"""
        ptr = C.c_void_p()
        check(self._L.paris_hip_make_filter_windowed(self._ctx, size, tau, window, C.byref(ptr)), "paris_hip_make_filter")
        self._owned.add(ptr.value)
        return FilterBuffer(ptr.value, size, self)

    def filter_to_host(self, k):
        n = k.size // 2 + 1
        out = np.empty((1, n), np.float32)
        check(self._L.paris_hip_memcpy_projection_d2h(self._ctx, out.ctypes.data, n * 4, k.ptr, n * 4, n, 1),
              "paris_hip_memcpy_projection_d2h")
        self.synchronize()
        return out[0]

    def apply_filter(self, p, k, filter_size, n_col):
        """backend::apply_filter (src/openmp/filtering.cpp:167-219)"""
        check(self._L.paris_hip_apply_filter(self._ctx, p.ptr, p.pitch, p.dim_x, p.dim_y, k.ptr, filter_size,
                                             n_col), "paris_hip_apply_filter")

    def set_filter_variant(self, variant):
        check(self._L.paris_hip_set_filter_variant(self._ctx, variant), "paris_hip_set_filter_variant")

    def set_backproject_skip_invalid(self, enable=True):
        """paris_hip_set_backproject_skip_invalid: tiles no ray of a projection reaches are left untouched (library-allocated
        volumes only; default on)"""
        check(self._L.paris_hip_set_backproject_skip_invalid(self._ctx, int(bool(enable))), "paris_hip_set_backproject_skip_invalid")

    def set_stage_fusion(self, enable=True):
        """weight() is held back and rides along in the load of the apply_filter() that follows (one launch)"""
        check(self._L.paris_hip_set_stage_fusion(self._ctx, int(bool(enable))), "paris_hip_set_stage_fusion")

    def weight_filter_rows(self, p, row_first, row_count, h_min, v_min, d_sd, l_px_row, l_px_col, k, filter_size, half_ptr=None,
                           half_pitch=0):
        """weighting + row filter of a band of rows in one launch (extension); half_ptr: store IEEE half there instead"""
        check(self._L.paris_hip_weight_filter_rows(self._ctx, p.ptr, p.pitch, p.dim_x, p.dim_y, row_first, row_count, h_min, v_min,
                                                   d_sd, l_px_row, l_px_col, k.ptr, filter_size, half_ptr, half_pitch),
              "paris_hip_weight_filter_rows")

    def backproject(self, p, v, v_offset, det_geo, vol_geo, enable_roi, roi, sin, cos, delta_s, delta_t):
        """backend::backproject (src/openmp/backprojection.cpp:156-199)"""
        r = roi if roi is not None else RegionOfInterest()
        check(self._L.paris_hip_backproject(self._ctx, p.ptr, p.pitch, p.dim_x, p.dim_y, v.ptr, v.dim_x, v.dim_y,
                                            v.dim_z, v_offset, C.byref(det_geo), C.byref(vol_geo),
                                            int(bool(enable_roi)), C.byref(r), sin, cos, delta_s, delta_t),
              "paris_hip_backproject")

    def convert_projection_f16(self, p):
        """fp32 device projection -> new device buffer of IEEE half pixels (round to nearest even); returns
        (device address, pitch in bytes). Free with Backend.free(address)."""
        pitch = (p.dim_x * 2 + 255) // 256 * 256
        d, dp = C.c_void_p(), C.c_size_t()
        # the projection allocator hands out rows of `pitch` bytes (pitch / 4 fp32 slots, already a 256 B multiple)
        check(self._L.paris_hip_malloc_projection(self._ctx, pitch // 4, p.dim_y, C.byref(d), C.byref(dp)),
              "paris_hip_malloc_projection")
        self._owned.add(d.value)
        check(self._L.paris_hip_convert_projection_f16(self._ctx, p.ptr, p.pitch, d.value, dp.value, p.dim_x, p.dim_y),
              "paris_hip_convert_projection_f16")
        return d.value, dp.value

    def backproject_f16(self, p_ptr, p_pitch, p_dim_x, p_dim_y, v, v_offset, det_geo, vol_geo, enable_roi, roi, sin, cos,
                        delta_s, delta_t):
        r = roi if roi is not None else RegionOfInterest()
        check(self._L.paris_hip_backproject_f16(self._ctx, p_ptr, p_pitch, p_dim_x, p_dim_y, v.ptr, v.dim_x, v.dim_y,
                                                v.dim_z, v_offset, C.byref(det_geo), C.byref(vol_geo),
                                                int(bool(enable_roi)), C.byref(r), sin, cos, delta_s, delta_t),
              "paris_hip_backproject_f16")

    def backproject_batch(self, p_ptr, p_pitch, p_stride, n_proj, p_dim_x, p_dim_y, v, v_offset, det_geo, vol_geo,
                          enable_roi, roi, sins, coss, delta_s, delta_t):
        r = roi if roi is not None else RegionOfInterest()
        s = (C.c_float * n_proj)(*sins)
        c = (C.c_float * n_proj)(*coss)
        check(self._L.paris_hip_backproject_batch(self._ctx, p_ptr, p_pitch, p_stride, n_proj, p_dim_x, p_dim_y,
                                                  v.ptr, v.dim_x, v.dim_y, v.dim_z, v_offset, C.byref(det_geo),
                                                  C.byref(vol_geo), int(bool(enable_roi)), C.byref(r), s, c,
                                                  delta_s, delta_t), "paris_hip_backproject_batch")

    def backproject_batch_f16(self, p_ptr, p_pitch, p_stride, n_proj, p_dim_x, p_dim_y, v, v_offset, det_geo, vol_geo,
                              enable_roi, roi, sins, coss, delta_s, delta_t):
        r = roi if roi is not None else RegionOfInterest()
        s = (C.c_float * n_proj)(*sins)
        c = (C.c_float * n_proj)(*coss)
        check(self._L.paris_hip_backproject_batch_f16(self._ctx, p_ptr, p_pitch, p_stride, n_proj, p_dim_x, p_dim_y,
                                                      v.ptr, v.dim_x, v.dim_y, v.dim_z, v_offset, C.byref(det_geo),
                                                      C.byref(vol_geo), int(bool(enable_roi)), C.byref(r), s, c,
                                                      delta_s, delta_t), "paris_hip_backproject_batch_f16")

    def forward_project(self, v, v_offset, det_geo, vol_geo, p, sin, cos, delta_s, delta_t, accumulate=False, frame_stride=0):
        """Cone-beam projections of the slab v (first slice: global slice v_offset of the grid vol_geo) by Joseph's method
        (paris_hip_forward_project), in the backprojector's geometry. sin / cos are scalars for one view or sequences for n views,
        written frame_stride bytes apart starting at p; delta_s / delta_t in mm. accumulate: each ray sum is added to the stored
        pixel instead of replacing it."""
        sins = np.atleast_1d(np.asarray(sin, np.float32))
        coss = np.atleast_1d(np.asarray(cos, np.float32))
        if sins.shape != coss.shape or sins.ndim != 1:
            raise ValueError("forward_project: sin and cos must be scalars or sequences of one length")
        fp = C.POINTER(C.c_float)
        check(self._L.paris_hip_forward_project(self._ctx, v.ptr, v.dim_x, v.dim_y, v.dim_z, v_offset, C.byref(det_geo), C.byref(vol_geo),
                                                p.ptr, p.pitch, frame_stride, len(sins), p.dim_x, p.dim_y, sins.ctypes.data_as(fp),
                                                coss.ctypes.data_as(fp), delta_s, delta_t, int(bool(accumulate))),
              "paris_hip_forward_project")

    # ---- diagnostics ------------------------------------------------------------------------------------------
    def last_backproject_ms(self):
        ms = C.c_float()
        check(self._L.paris_hip_last_backproject_ms(self._ctx, C.byref(ms)), "paris_hip_last_backproject_ms")
        return ms.value

    def backproject_timing_arm(self, capacity):
        check(self._L.paris_hip_backproject_timing_arm(self._ctx, capacity), "paris_hip_backproject_timing_arm")

    def backproject_timing_collect(self, max_n=65536):
        ms = (C.c_float * max_n)()
        n = C.c_uint32()
        check(self._L.paris_hip_backproject_timing_collect(self._ctx, ms, max_n, C.byref(n)),
              "paris_hip_backproject_timing_collect")
        return list(ms[:n.value])

    def set_backproject_variant(self, variant):
        check(self._L.paris_hip_set_backproject_variant(self._ctx, variant), "paris_hip_set_backproject_variant")

    def set_backproject_order(self, order=-1, nontemporal=-1):
        check(self._L.paris_hip_set_backproject_order(self._ctx, order, nontemporal), "paris_hip_set_backproject_order")

    def fast_division_is_exact(self, divisor):
        ok = C.c_int()
        check(self._L.paris_hip_fast_division_is_exact(self._ctx, divisor, C.byref(ok)), "paris_hip_fast_division_is_exact")
        return bool(ok.value)

    def set_backproject_vector_staging(self, enable=True):
        check(self._L.paris_hip_set_backproject_vector_staging(self._ctx, int(bool(enable))),
              "paris_hip_set_backproject_vector_staging")

    def set_backproject_fast_division(self, enable=True):
        check(self._L.paris_hip_set_backproject_fast_division(self._ctx, int(bool(enable))),
              "paris_hip_set_backproject_fast_division")

    def set_backproject_slice_shape(self, waves=0, row_groups=0):
        check(self._L.paris_hip_set_backproject_slice_shape(self._ctx, waves, row_groups),
              "paris_hip_set_backproject_slice_shape")

    def set_filter_window(self, window):
        """window of the K that the filter stage wrapper builds: 0 = the reference's ramp, 1 = Shepp-Logan"""
        check(self._L.paris_hip_set_filter_window(self._ctx, window), "paris_hip_set_filter_window")

    def set_filter_deferral(self, enable):
        """paris_hip_set_filter_deferral: with stage fusion and a deferral depth > 1, the filter() that follows a weight() is held back
        too and runs on the library's snapshot, a group per launch, if the next call backprojects that projection (whose buffer then
        keeps its unfiltered pixels); bit-identical volume"""
        check(self._L.paris_hip_set_filter_deferral(self._ctx, 2 if enable == 2 else int(bool(enable))), "paris_hip_set_filter_deferral")

    def set_backproject_deferral(self, depth):
        """depth > 1: backproject() calls are snapshotted and added by one fused launch per `depth` calls (bit-identical)"""
        check(self._L.paris_hip_set_backproject_deferral(self._ctx, depth), "paris_hip_set_backproject_deferral")

    def set_backproject_overlap(self, enable=True):
        """deferred fused launches run on a second stream beside the caller's next calls (default off: measured slower)"""
        check(self._L.paris_hip_set_backproject_overlap(self._ctx, int(bool(enable))), "paris_hip_set_backproject_overlap")

    def set_backproject_references(self, enable=True):
        """deferral by reference: a deferred backproject() of a whole make_projection_device buffer takes no snapshot, the group's
        fused launch reads the buffer itself; free() of it returns at once and the buffer is recycled behind the launch; any other
        call that touches it launches the pending group first (bit-identical; paris::hip switches it on)"""
        check(self._L.paris_hip_set_backproject_references(self._ctx, int(bool(enable))), "paris_hip_set_backproject_references")

    def set_async_validation(self, enable=True):
        """validators of the hand-expanded IEEE sequences are launched and not waited for; the compiler's forms serve until they
        have answered (same bits)"""
        check(self._L.paris_hip_set_async_validation(self._ctx, int(bool(enable))), "paris_hip_set_async_validation")

    def projection_reserve_bytes(self, dim_x, dim_y):
        """what this ctx may keep allocated for projections of that size beside the volume (buffer rotation, pending group or ring)"""
        n = C.c_size_t(0)
        check(self._L.paris_hip_projection_reserve_bytes(self._ctx, dim_x, dim_y, C.byref(n)), "paris_hip_projection_reserve_bytes")
        return int(n.value)

    def set_paris_loop_defaults(self, depth=48):
        """The settings the C++ mirror paris::hip makes in set_device() (paris_amd/host/paris/hip/backend.h) for PARIS's own loop --
        a buffer allocated, filled, weighted, filtered, backprojected and freed per projection (src/main.cpp:98-105): stage fusion,
        `depth` backprojections per fused launch on the second stream, projections by reference, the filter in place a group at a
        time, validators beside the first projections. Every result stays bit-identical; needs an asynchronous backend."""
        self.set_stage_fusion(True)
        self.set_backproject_deferral(depth)
        self.set_backproject_overlap(True)
        self.set_backproject_references(True)
        self.set_filter_deferral(2)
        self.set_async_validation(True)

    def flush(self):
        check(self._L.paris_hip_flush(self._ctx), "paris_hip_flush")

    def set_backproject_tuning(self, vx=0, unroll=0, tz=0, lds_bytes=0):
        check(self._L.paris_hip_set_backproject_tuning(self._ctx, vx, unroll, tz, lds_bytes),
              "paris_hip_set_backproject_tuning")


# ---- device management (src/cuda/device.cpp:31-47, src/openmp/backend.h:87-89) --------------------------------

def get_devices():
    n = C.c_int()
    check(_lib.load().paris_hip_device_count(C.byref(n)), "paris_hip_device_count")
    return list(range(n.value))


def set_device(device, stream=None, synchronous=True):
    """Binds the calling thread's work to `device`; returns the Backend that carries the per-device state."""
    return Backend(device, stream, synchronous)


# ---- geometry (src/geometry.cpp) -----------------------------------------------------------------------------

def calculate_volume_geometry(det_geo):
    out = VolumeGeometry()
    check(_lib.load().paris_hip_calculate_volume_geometry(C.byref(det_geo), C.byref(out)),
          "paris_hip_calculate_volume_geometry")
    return out


def apply_roi(vol_geo, x1, x2, y1, y2, z1, z2):
    out = VolumeGeometry()
    roi = RegionOfInterest(x1, x2, y1, y2, z1, z2)
    check(_lib.load().paris_hip_apply_roi(C.byref(vol_geo), C.byref(roi), C.byref(out)), "paris_hip_apply_roi")
    return out


def filter_size(n_row):
    return int(_lib.load().paris_hip_filter_size(n_row))


# ---- stage wrappers (src/loader.cpp, make_volume.cpp, weighting.cpp, filtering.cpp, backprojection.cpp) --------

def load(backend, p):
    """paris::load (src/loader.cpp:28-33)"""
    d_p = backend.make_projection_device(p.dim_x, p.dim_y)
    backend.copy_h2d(p, d_p)
    return d_p


def make_volume(backend, subvol_geo, last):
    """paris::make_volume (src/make_volume.cpp:30-37)"""
    dim_z = subvol_geo.dim_z
    if last:
        dim_z += subvol_geo.remainder
    return backend.make_volume_device(subvol_geo.dim_x, subvol_geo.dim_y, dim_z)


def weight(backend, p, det_geo):
    """paris::weight (src/weighting.cpp:32-45)"""
    check(backend._L.paris_hip_stage_weight(backend._ctx, p.ptr, p.pitch, p.dim_x, p.dim_y, C.byref(det_geo)),
          "paris_hip_stage_weight")


def filter(backend, p, det_geo):  # noqa: A001 - the reference's name
    """paris::filter (src/filtering.cpp:32-45)"""
    check(backend._L.paris_hip_stage_filter(backend._ctx, p.ptr, p.pitch, p.dim_x, p.dim_y, C.byref(det_geo)),
          "paris_hip_stage_filter")


def short_scan_check(det_geo, start_deg, range_deg):
    """gamma_m in degrees -- the largest |fan angle| over the outermost pixel centres -- of a valid short scan over
    [start_deg, start_deg + range_deg] (paris_hip_short_scan_check); raises ParisHipError when range_deg < 180 + 2 gamma_m,
    range_deg > 360 or a value is not finite"""
    g = C.c_float()
    check(_lib.load().paris_hip_short_scan_check(C.byref(det_geo), C.byref(ShortScan(start_deg, range_deg)), C.byref(g)),
          "paris_hip_short_scan_check")
    return g.value


def stage_short_scan_weight(backend, p, det_geo, scan, enable_angles=False):
    """The redundancy weight of one whole projection, its angle resolved from p.idx / p.phi as the backprojection does
    (paris_hip_stage_short_scan_weight)"""
    if not isinstance(scan, ShortScan):
        scan = ShortScan(*scan)
    check(backend._L.paris_hip_stage_short_scan_weight(backend._ctx, p.ptr, p.pitch, p.dim_x, p.dim_y, C.byref(det_geo), C.byref(scan),
                                                       p.idx, int(bool(enable_angles)), p.phi), "paris_hip_stage_short_scan_weight")


def offset_detector_check(det_geo):
    """gamma_tau in degrees -- the half-angle of the overlap |t| < tau = (n_row / 2 - |delta_s|) l_px_row that an offset detector
    measures twice per circle (paris_hip_offset_detector_check); raises ParisHipError when tau < 2 l_px_row or the geometry is
    degenerate or not finite"""
    g = C.c_float()
    check(_lib.load().paris_hip_offset_detector_check(C.byref(det_geo), C.byref(g)), "paris_hip_offset_detector_check")
    return g.value


def stage_offset_detector_weight(backend, p, det_geo):
    """The offset-detector redundancy weight of one whole projection (paris_hip_stage_offset_detector_weight)"""
    check(backend._L.paris_hip_stage_offset_detector_weight(backend._ctx, p.ptr, p.pitch, p.dim_x, p.dim_y, C.byref(det_geo)),
          "paris_hip_stage_offset_detector_weight")


def slab_row_band(det_geo, vol_geo, v_dim_x, v_dim_y, v_dim_z, v_offset=0, roi=None):
    """f4: (first row, row count) of the detector band the slab can read (paris_hip_slab_row_band)."""
    r = roi if roi is not None else RegionOfInterest()
    first, count = C.c_uint32(), C.c_uint32()
    check(_lib.load().paris_hip_slab_row_band(C.byref(det_geo), C.byref(vol_geo), v_dim_x, v_dim_y, v_dim_z, v_offset,
                                              int(roi is not None), C.byref(r), C.byref(first), C.byref(count)),
          "paris_hip_slab_row_band")
    return first.value, count.value


def weight_rows(backend, p, det_geo, row_first, row_count):
    """paris::weight on the rows of a band only (paris_hip_stage_weight_rows)"""
    check(backend._L.paris_hip_stage_weight_rows(backend._ctx, p.ptr, p.pitch, p.dim_x, p.dim_y, row_first, row_count,
                                                 C.byref(det_geo)), "paris_hip_stage_weight_rows")


def filter_rows(backend, p, det_geo, row_first, row_count):
    """paris::filter on the rows of a band only (paris_hip_stage_filter_rows)"""
    check(backend._L.paris_hip_stage_filter_rows(backend._ctx, p.ptr, p.pitch, p.dim_x, p.dim_y, row_first, row_count,
                                                 C.byref(det_geo)), "paris_hip_stage_filter_rows")


def weight_filter_rows(backend, p, det_geo, row_first, row_count, half_ptr=None, half_pitch=0):
    """paris::weight + paris::filter of a row band in one launch (paris_hip_stage_weight_filter_rows); half_ptr: store the
    filtered band as IEEE half there instead of fp32 in place"""
    check(backend._L.paris_hip_stage_weight_filter_rows(backend._ctx, p.ptr, p.pitch, p.dim_x, p.dim_y, row_first, row_count,
                                                        C.byref(det_geo), half_ptr, half_pitch), "paris_hip_stage_weight_filter_rows")


def weight_filter_batch(backend, ptr, pitch, frame_stride, n_frames, dim_x, dim_y, det_geo, row_first, row_count, half_ptr=None,
                        half_pitch=0, half_frame_stride=0):
    """paris::weight + paris::filter of a row band for a group of n_frames projections frame_stride bytes apart, in ONE launch
    (paris_hip_stage_weight_filter_batch); bit-identical to the per-frame calls"""
    check(backend._L.paris_hip_stage_weight_filter_batch(backend._ctx, ptr, pitch, frame_stride, n_frames, dim_x, dim_y, row_first,
                                                         row_count, C.byref(det_geo), half_ptr, half_pitch, half_frame_stride),
          "paris_hip_stage_weight_filter_batch")


def backproject(backend, p, v, v_offset, det_geo, vol_geo, enable_angles, enable_roi, roi):
    """paris::backproject (src/backprojection.cpp:37-69)"""
    r = roi if roi is not None else RegionOfInterest()
    check(backend._L.paris_hip_stage_backproject(backend._ctx, p.ptr, p.pitch, p.dim_x, p.dim_y, p.idx, p.phi,
                                                 v.ptr, v.dim_x, v.dim_y, v.dim_z, v_offset, C.byref(det_geo),
                                                 C.byref(vol_geo), int(bool(enable_angles)),
                                                 int(bool(enable_roi)), C.byref(r)),
          "paris_hip_stage_backproject")


def forward_project(backend, v, v_offset, p, det_geo, vol_geo, enable_angles=False, accumulate=False):
    """The projection of the slab v at the angle of p.idx / p.phi, resolved as backproject() resolves it, written into (or, with
    accumulate, added to) p (paris_hip_stage_forward_project)"""
    check(backend._L.paris_hip_stage_forward_project(backend._ctx, v.ptr, v.dim_x, v.dim_y, v.dim_z, v_offset, C.byref(det_geo),
                                                     C.byref(vol_geo), p.ptr, p.pitch, p.dim_x, p.dim_y, p.idx, p.phi,
                                                     int(bool(enable_angles)), int(bool(accumulate))),
          "paris_hip_stage_forward_project")


def stage_angle(det_geo, idx, enable_angles=False, phi=0.0):
    s, c = C.c_float(), C.c_float()
    check(_lib.load().paris_hip_stage_angle(C.byref(det_geo), idx, int(bool(enable_angles)), phi, C.byref(s),
                                            C.byref(c)), "paris_hip_stage_angle")
    return s.value, c.value
