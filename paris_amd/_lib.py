"""Loader and ctypes signatures of paris_amd/lib/libparis_hip.so (the C ABI of include/paris_hip.h).

There is no CPU fallback: if the HIP library is missing or fails to load, importing the backend raises.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# the product library; PARIS_HIP_LIBRARY names another build of the same C ABI -- the experiments build of `make EXPERIMENTS=1`
# (lib/libparis_hip_experiments.so: the kernels, tile orders and switches that lost their A/B runs) for tools/ and the variant tests
EXPERIMENTS_LIB_PATH = os.path.join(_HERE, "lib", "libparis_hip_experiments.so")
LIB_PATH = os.environ.get("PARIS_HIP_LIBRARY") or os.path.join(_HERE, "lib", "libparis_hip.so")

SUCCESS = 0
ERROR_INVALID_ARGUMENT = 10001
ERROR_NO_DEVICE = 10002
ERROR_UNSUPPORTED = 10003
CTX_DEFAULT = 0
CTX_SYNCHRONOUS = 1
CTX_LEGACY_STREAM = 2
CTX_WARM = 4
# pixel types of paris_hip_upload_projection_raw
PIXEL_U8 = 1
PIXEL_U16 = 2
PIXEL_U32 = 3
PIXEL_F32 = 4


class DetectorGeometry(C.Structure):
    """paris::detector_geometry (src/geometry.h:30-46)"""
    _fields_ = [("n_row", C.c_uint32), ("n_col", C.c_uint32),
                ("l_px_row", C.c_float), ("l_px_col", C.c_float),
                ("delta_s", C.c_float), ("delta_t", C.c_float),
                ("d_so", C.c_float), ("d_od", C.c_float),
                ("delta_phi", C.c_float)]


class VolumeGeometry(C.Structure):
    """paris::volume_geometry (src/geometry.h:48-57)"""
    _fields_ = [("dim_x", C.c_uint32), ("dim_y", C.c_uint32), ("dim_z", C.c_uint32),
                ("l_vx_x", C.c_float), ("l_vx_y", C.c_float), ("l_vx_z", C.c_float)]


class SubvolumeGeometry(C.Structure):
    """paris::subvolume_geometry (src/geometry.h:59-69)"""
    _fields_ = [("dim_x", C.c_uint32), ("dim_y", C.c_uint32), ("dim_z", C.c_uint32),
                ("remainder", C.c_uint32)]


class RegionOfInterest(C.Structure):
    """paris::region_of_interest (src/region_of_interest.h:30-38)"""
    _fields_ = [("x1", C.c_uint32), ("x2", C.c_uint32), ("y1", C.c_uint32),
                ("y2", C.c_uint32), ("z1", C.c_uint32), ("z2", C.c_uint32)]


class ShortScan(C.Structure):
    """paris_short_scan: the projection angles [start_deg, start_deg + range_deg] a short scan covers (extension)"""
    _fields_ = [("start_deg", C.c_float), ("range_deg", C.c_float)]


class DefectStats(C.Structure):
    """paris_hip_defect_stats: what a defect map's repair plan holds (extension)"""
    _fields_ = [("defects", C.c_uint64), ("unrepairable", C.c_uint64), ("sources", C.c_uint64),
                ("reach_rows", C.c_uint32), ("reach_cols", C.c_uint32), ("device_bytes", C.c_uint64)]


class ZingerFilter(C.Structure):
    """paris_hip_zinger_filter: the parameters of the zinger rule (extension)"""
    _fields_ = [("threshold_abs", C.c_float), ("threshold_rel", C.c_float), ("polarity", C.c_int), ("max_hits", C.c_uint32)]


class ZingerCounts(C.Structure):
    """paris_hip_zinger_counts: what paris_hip_zinger_stats reports (extension)"""
    _fields_ = [("frames", C.c_uint64), ("replaced", C.c_uint64), ("saturated_frames", C.c_uint64)]


ZINGER_FRAMES_MAX = 64  # PARIS_HIP_ZINGER_FRAMES_MAX


class RingFilter(C.Structure):
    """paris_hip_ring_filter: the parameters of the ring rule (extension)"""
    _fields_ = [("half_width", C.c_uint32), ("floor_abs", C.c_float), ("limit_abs", C.c_float)]


class RingStats(C.Structure):
    """paris_hip_ring_stats: what the ring rule did to a mean frame (extension)"""
    _fields_ = [("corrected", C.c_uint64), ("below_floor", C.c_uint64), ("above_limit", C.c_uint64), ("not_finite", C.c_uint64),
                ("max_abs", C.c_float), ("frames_min", C.c_uint32), ("frames_max", C.c_uint32)]


RING_FRAMES_MAX = 64  # PARIS_HIP_RING_FRAMES_MAX


class Binning(C.Structure):
    """paris_hip_binning: detector binning factors, each 1, 2, 4 or 8 (extension)"""
    _fields_ = [("bin_x", C.c_uint32), ("bin_y", C.c_uint32)]


class AxisSearch(C.Structure):
    """paris_hip_axis_search: the candidates and the band of the axis search (extension)"""
    _fields_ = [("lo", C.c_float), ("step", C.c_float), ("count", C.c_uint32), ("rows", C.c_uint32), ("min_columns", C.c_uint32)]


class AxisEntry(C.Structure):
    """paris_hip_axis_entry: where one column's conjugate lies for one candidate (extension)"""
    _fields_ = [("i0", C.c_int32), ("k0", C.c_uint32), ("wi", C.c_float), ("wf", C.c_float)]


class AxisResult(C.Structure):
    """paris_hip_axis_result: the estimate of the axis search (extension)"""
    _fields_ = [("delta_s", C.c_float), ("best", C.c_uint32), ("cost_min", C.c_double), ("cost_median", C.c_double),
                ("scored", C.c_uint32), ("columns", C.c_uint32), ("skipped", C.c_uint64), ("at_edge", C.c_uint32),
                ("row_first", C.c_uint32)]


AXIS_FRAMES_MAX = 64  # PARIS_HIP_AXIS_FRAMES_MAX


class DetectorRoll(C.Structure):
    """paris_hip_detector_roll: the detector's in-plane rotation [deg] (extension)"""
    _fields_ = [("eta_deg", C.c_float)]


class RollSearch(C.Structure):
    """paris_hip_roll_search: the candidates of the roll search (extension)"""
    _fields_ = [("lo_deg", C.c_float), ("step_deg", C.c_float), ("count", C.c_uint32), ("min_pixels", C.c_uint32)]


class RollResult(C.Structure):
    """paris_hip_roll_result: the estimate of the roll search (extension)"""
    _fields_ = [("eta_deg", C.c_float), ("best", C.c_uint32), ("cost_min", C.c_double), ("cost_median", C.c_double),
                ("scored", C.c_uint32), ("at_edge", C.c_uint32), ("skipped", C.c_uint64), ("margin_x", C.c_uint32),
                ("margin_y", C.c_uint32)]


class AirRegion(C.Structure):
    """paris_hip_air_region: the rectangle of the detector that sees only air, and when a frame is not normalised (extension)"""
    _fields_ = [("x0", C.c_uint32), ("y0", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32), ("min_pixels", C.c_uint32),
                ("limit_abs", C.c_float)]


class AirCounts(C.Structure):
    """paris_hip_air_counts: what paris_hip_air_stats reports (extension)"""
    _fields_ = [("frames", C.c_uint64), ("normalised", C.c_uint64), ("too_few", C.c_uint64), ("above_limit", C.c_uint64),
                ("min_a", C.c_float), ("max_a", C.c_float)]


AIR_FRAMES_MAX = 64  # PARIS_HIP_AIR_FRAMES_MAX

# what paris_hip_bh_solve refuses
ERROR_BH_TOO_FEW_VOXELS = 10004
ERROR_BH_NOT_POSITIVE = 10005
ERROR_BH_NOT_FINITE = 10006
BH_DEGREE_MAX = 4  # PARIS_HIP_BH_DEGREE_MAX
BH_MARGIN_MAX = 4  # PARIS_HIP_BH_MARGIN_MAX
BH_HISTOGRAM_BINS = 4096  # PARIS_HIP_BH_HISTOGRAM_BINS
BH_PARTIALS = 65536  # PARIS_HIP_BH_PARTIALS
BH_MIN_VOXELS_DEFAULT = 64  # PARIS_HIP_BH_MIN_VOXELS_DEFAULT


class BeamHardening(C.Structure):
    """paris_hip_beam_hardening: the polynomial q = c_1 p + ... + c_N p^N of the line integral (extension)"""
    _fields_ = [("degree", C.c_uint32), ("c", C.c_float * BH_DEGREE_MAX)]


class BhCounts(C.Structure):
    """paris_hip_bh_counts: what paris_hip_bh_gram counts (extension)"""
    _fields_ = [("n_object", C.c_uint64), ("n_air", C.c_uint64), ("n_ignored", C.c_uint64), ("n_not_finite", C.c_uint64)]


class BhFit(C.Structure):
    """paris_hip_bh_fit: what paris_hip_bh_solve returns (extension)"""
    _fields_ = [("setting", BeamHardening), ("level", C.c_double), ("residual_before", C.c_double), ("residual_after", C.c_double)]


PHASE_MARGIN_MAX = 1024  # PARIS_HIP_PHASE_MARGIN_MAX
PHASE_SIZE_MAX = 8192  # PARIS_HIP_PHASE_SIZE_MAX


class PhaseRetrieval(C.Structure):
    """paris_hip_phase_retrieval: Paganin's single-distance filter on the transmission image (extension)"""
    _fields_ = [("alpha_mm2", C.c_float), ("t_min", C.c_float), ("margin", C.c_uint32)]


SCATTER_ITERATIONS_MAX = 16  # PARIS_HIP_SCATTER_ITERATIONS_MAX


class ScatterCorrection(C.Structure):
    """paris_hip_scatter_correction: scatter kernel superposition, iterated (extension)"""
    _fields_ = [("amplitude", C.c_float), ("alpha", C.c_float), ("beta", C.c_float), ("sigma1_mm", C.c_float), ("sigma2_mm", C.c_float),
                ("weight2", C.c_float), ("limit", C.c_float), ("iterations", C.c_uint32), ("margin", C.c_uint32)]


STARVATION_RADIUS_MAX = 4  # PARIS_HIP_STARVATION_RADIUS_MAX
STARVATION_LEVELS = 64  # PARIS_HIP_STARVATION_LEVELS
STARVATION_FRAMES_MAX = 8  # PARIS_HIP_STARVATION_FRAMES_MAX


class StarvationFilter(C.Structure):
    """paris_hip_starvation_filter: adaptive frame filter above the line integral p0 (extension)"""
    _fields_ = [("p0", C.c_float), ("gain", C.c_float), ("radius", C.c_uint32)]


class StarvationCounts(C.Structure):
    """paris_hip_starvation_counts: what paris_hip_starvation_stats reports (extension)"""
    _fields_ = [("frames", C.c_uint64), ("filtered", C.c_uint64), ("last_level", C.c_uint64)]


LAG_TERMS_MAX = 4  # PARIS_HIP_LAG_TERMS_MAX
LAG_START_REST = 0  # PARIS_HIP_LAG_START_REST
LAG_START_STEADY = 1  # PARIS_HIP_LAG_START_STEADY


class LagModel(C.Structure):
    """paris_hip_lag_model: the multi-exponential impulse response of the detector's lag (extension)"""
    _fields_ = [("terms", C.c_uint32), ("b", C.c_float * LAG_TERMS_MAX), ("a", C.c_float * LAG_TERMS_MAX), ("start", C.c_int)]


# what paris_hip_metal_collect refuses
ERROR_METAL_TOO_MANY_VOXELS = 10007
METAL_GROW_MAX = 4  # PARIS_HIP_METAL_GROW_MAX
METAL_MIN_VOXELS_CAP = 1024  # PARIS_HIP_METAL_MIN_VOXELS_CAP
METAL_COUNTER_BYTES = 64  # what the counters at the head of a metal trace setting occupy on the device


class MetalCounts(C.Structure):
    """paris_hip_metal_counts: what paris_hip_metal_stats reports (extension)"""
    _fields_ = [("replaced", C.c_uint64), ("runs", C.c_uint64), ("rows_left", C.c_uint64)]


class RowExtension(C.Structure):
    """paris_hip_row_extension: the row extension for truncated projections (extension)"""
    _fields_ = [("edge_pixels", C.c_uint32), ("taper_pixels", C.c_uint32)]


# voxel types of paris_hip_volume_quantize
VOXEL_U8 = 1
VOXEL_U16 = 2
VOLUME_HISTOGRAM_BINS_MAX = 4096  # PARIS_HIP_VOLUME_HISTOGRAM_BINS_MAX


BILATERAL_BINS = 1024  # PARIS_HIP_BILATERAL_BINS
BILATERAL_RADIUS_MAX = 3  # PARIS_HIP_BILATERAL_RADIUS_MAX


class VolumeBilateral(C.Structure):
    """struct paris_hip_volume_bilateral: range sigma (the volume's units), spatial sigma (voxels) and radius of the 3-D bilateral
    filter (extension)"""
    _fields_ = [("sigma_r", C.c_float), ("sigma_s", C.c_float), ("radius", C.c_uint32)]


class VolumeWindow(C.Structure):
    """paris_hip_volume_window: the grey window and integer type a volume is quantised to (extension)"""
    _fields_ = [("lo", C.c_float), ("hi", C.c_float), ("voxel_type", C.c_int)]


class VolumeCounts(C.Structure):
    """paris_hip_volume_counts: what paris_hip_volume_quantize_counts reports (extension)"""
    _fields_ = [("voxels", C.c_uint64), ("below", C.c_uint64), ("above", C.c_uint64), ("not_finite", C.c_uint64)]


class VolumeStatistics(C.Structure):
    """paris_hip_volume_statistics: what paris_hip_volume_stats reports (extension)"""
    _fields_ = [("min", C.c_float), ("max", C.c_float), ("below", C.c_uint64), ("above", C.c_uint64), ("not_finite", C.c_uint64),
                ("voxels", C.c_uint64)]


class SubvolumeInfo(C.Structure):
    """paris::subvolume_info (src/subvolume_information.h:30-34)"""
    _fields_ = [("geo", SubvolumeGeometry), ("num", C.c_int)]


_vp = C.c_void_p
_u32 = C.c_uint32
_f = C.c_float
_sz = C.c_size_t
_P = C.POINTER

# name -> (restype, argtypes); every symbol include/paris_hip.h declares
SIGNATURES = {
    "paris_hip_device_count": (C.c_int, [_P(C.c_int)]),
    "paris_hip_ctx_create": (C.c_int, [C.c_int, _vp, C.c_uint, _P(_vp)]),
    "paris_hip_ctx_destroy": (C.c_int, [_vp]),
    "paris_hip_ctx_synchronize": (C.c_int, [_vp]),
    "paris_hip_ctx_stream": (_vp, [_vp]),
    "paris_hip_fence_create": (C.c_int, [_vp, _P(_vp)]),
    "paris_hip_fence_record": (C.c_int, [_vp, _vp]),
    "paris_hip_fence_wait": (C.c_int, [_vp, _vp]),
    "paris_hip_fence_destroy": (C.c_int, [_vp, _vp]),
    "paris_hip_malloc_projection": (C.c_int, [_vp, _u32, _u32, _P(_vp), _P(_sz)]),
    "paris_hip_malloc_volume": (C.c_int, [_vp, _u32, _u32, _u32, _P(_vp)]),
    "paris_hip_free": (C.c_int, [_vp, _vp]),
    "paris_hip_malloc_host": (C.c_int, [_vp, _sz, _P(_vp)]),
    "paris_hip_free_host": (C.c_int, [_vp, _vp]),
    "paris_hip_memcpy_projection_h2d": (C.c_int, [_vp, _vp, _sz, _vp, _sz, _u32, _u32]),
    "paris_hip_upload_projection": (C.c_int, [_vp, _vp, _sz, _vp, _sz, _u32, _u32]),
    "paris_hip_upload_projection_raw": (C.c_int, [_vp, _vp, _sz, _vp, _sz, _u32, _u32, C.c_int]),
    "paris_hip_upload_projection_raw_corrected": (C.c_int, [_vp, _vp, _sz, _vp, _sz, _u32, _u32, _u32, _u32, C.c_int]),
    "paris_hip_set_flat_field": (C.c_int, [_vp, _vp, _vp, _u32, _u32, _f]),
    "paris_hip_clear_flat_field": (C.c_int, [_vp]),
    "paris_hip_flat_field_rows": (C.c_int, [_vp, _vp, _sz, _sz, _u32, _u32, _u32, _u32, _u32]),
    "paris_hip_flat_field_dead_pixels": (C.c_int, [_vp, _vp]),
    "paris_hip_defect_plan_create": (C.c_int, [_vp, _u32, _u32, _P(_vp)]),
    "paris_hip_defect_plan_destroy": (C.c_int, [_vp]),
    "paris_hip_defect_plan_stats": (C.c_int, [_vp, _P(DefectStats)]),
    "paris_hip_defect_plan_copy": (C.c_int, [_vp, _vp, _vp, _vp, _vp]),
    "paris_hip_set_defect_map": (C.c_int, [_vp, _vp, _u32, _u32]),
    "paris_hip_clear_defect_map": (C.c_int, [_vp]),
    "paris_hip_defect_map_info": (C.c_int, [_vp, _P(DefectStats)]),
    "paris_hip_defect_repair_rows": (C.c_int, [_vp, _vp, _sz, _sz, _u32, _u32, _u32, _u32, _u32]),
    "paris_hip_zinger_filter_check": (C.c_int, [_P(ZingerFilter), _u32, _u32, _P(_u32), _P(_sz)]),
    "paris_hip_set_zinger_filter": (C.c_int, [_vp, _P(ZingerFilter), _u32, _u32]),
    "paris_hip_clear_zinger_filter": (C.c_int, [_vp]),
    "paris_hip_zinger_filter_rows": (C.c_int, [_vp, _vp, _sz, _sz, _u32, _u32, _u32, _u32, _u32]),
    "paris_hip_zinger_stats": (C.c_int, [_vp, _P(ZingerCounts), C.c_int]),
    "paris_hip_ring_filter_check": (C.c_int, [_P(RingFilter), _u32, _u32, _P(_sz), _P(_sz)]),
    "paris_hip_ring_correction_from_mean": (C.c_int, [_P(RingFilter), _vp, _vp, _u32, _u32, _vp, _P(RingStats)]),
    "paris_hip_ring_profile_begin": (C.c_int, [_vp, _u32, _u32]),
    "paris_hip_ring_profile_add_rows": (C.c_int, [_vp, _vp, _sz, _sz, _u32, _u32, _u32, _u32, _u32]),
    "paris_hip_ring_profile_finish": (C.c_int, [_vp, _P(RingFilter), _vp, _vp, _P(RingStats)]),
    "paris_hip_ring_profile_discard": (C.c_int, [_vp]),
    "paris_hip_set_ring_correction": (C.c_int, [_vp, _vp, _u32, _u32]),
    "paris_hip_clear_ring_correction": (C.c_int, [_vp]),
    "paris_hip_ring_correct_rows": (C.c_int, [_vp, _vp, _sz, _sz, _u32, _u32, _u32, _u32, _u32]),
    "paris_hip_axis_search_check": (C.c_int, [_P(AxisSearch), _P(DetectorGeometry), _u32, _P(_u32), _P(_sz)]),
    "paris_hip_axis_search_plan": (C.c_int, [_P(AxisSearch), _P(DetectorGeometry), _u32, _u32, _vp]),
    "paris_hip_axis_estimate_from_costs": (C.c_int, [_P(AxisSearch), _vp, _vp, _P(AxisResult)]),
    "paris_hip_axis_search_begin": (C.c_int, [_vp, _P(AxisSearch), _P(DetectorGeometry), _u32]),
    "paris_hip_axis_search_add_rows": (C.c_int, [_vp, _vp, _sz, _sz, _u32, _u32, _u32, _u32]),
    "paris_hip_axis_search_finish": (C.c_int, [_vp, _vp, _vp, _P(AxisResult), _vp]),
    "paris_hip_axis_search_discard": (C.c_int, [_vp]),
    "paris_hip_binning_check": (C.c_int, [_P(Binning), _u32, _u32, _P(_u32), _P(_u32)]),
    "paris_hip_binned_geometry": (C.c_int, [_P(Binning), _P(DetectorGeometry), _P(DetectorGeometry)]),
    "paris_hip_bin_frame_host": (C.c_int, [_P(Binning), _vp, _vp, _u32, _u32, _vp]),
    "paris_hip_bin_mask": (C.c_int, [_P(Binning), _vp, _u32, _u32, _vp]),
    "paris_hip_set_binning": (C.c_int, [_vp, _P(Binning), _vp, _u32, _u32]),
    "paris_hip_clear_binning": (C.c_int, [_vp]),
    "paris_hip_bin_frames": (C.c_int, [_vp, _vp, _sz, _sz, _vp, _sz, _sz, _u32, _u32, _u32, _u32, _u32]),
    "paris_hip_detector_roll_check": (C.c_int, [_P(DetectorRoll), _P(DetectorGeometry)]),
    "paris_hip_detector_roll_host": (C.c_int, [_P(DetectorRoll), _P(DetectorGeometry), _vp, _vp]),
    "paris_hip_detector_roll_source_rows": (C.c_int, [_P(DetectorRoll), _P(DetectorGeometry), _u32, _u32, _P(_u32), _P(_u32)]),
    "paris_hip_set_detector_roll": (C.c_int, [_vp, _P(DetectorRoll), _P(DetectorGeometry)]),
    "paris_hip_clear_detector_roll": (C.c_int, [_vp]),
    "paris_hip_detector_roll_rows": (C.c_int, [_vp, _vp, _sz, _sz, _vp, _sz, _sz, _u32, _u32, _u32, _u32, _u32]),
    "paris_hip_detector_roll_rows_with": (C.c_int, [_vp, _vp, _sz, _sz, _vp, _sz, _sz, _u32, _u32, _u32, _u32, _u32, _P(DetectorRoll),
                                                    _P(DetectorGeometry)]),
    "paris_hip_roll_search_check": (C.c_int, [_P(RollSearch), _P(DetectorGeometry), _P(_u32), _P(_u32), _P(_sz)]),
    "paris_hip_roll_estimate_from_costs": (C.c_int, [_P(RollSearch), _vp, _P(RollResult)]),
    "paris_hip_roll_search_run": (C.c_int, [_vp, _P(RollSearch), _P(DetectorGeometry), _vp, _vp, _vp, _P(RollResult)]),
    "paris_hip_air_region_check": (C.c_int, [_P(AirRegion), _u32, _u32, _P(_u32), _P(_sz)]),
    "paris_hip_air_value_host": (C.c_int, [_P(AirRegion), _vp, _vp, _u32, _u32, _P(_f), _P(_u32)]),
    "paris_hip_set_air_region": (C.c_int, [_vp, _P(AirRegion), _vp, _u32, _u32]),
    "paris_hip_clear_air_region": (C.c_int, [_vp]),
    "paris_hip_air_normalize_rows": (C.c_int, [_vp, _vp, _sz, _sz, _u32, _u32, _u32, _u32, _u32]),
    "paris_hip_air_measure": (C.c_int, [_vp, _vp, _sz, _sz, _u32, _u32, _u32, _vp, _vp]),
    "paris_hip_air_stats": (C.c_int, [_vp, _P(AirCounts), C.c_int]),
    "paris_hip_phase_alpha": (C.c_int, [_P(DetectorGeometry), C.c_double, C.c_double, _P(C.c_float)]),
    "paris_hip_phase_default_margin": (C.c_uint32, [C.c_float, C.c_float, C.c_float]),
    "paris_hip_phase_retrieval_check": (C.c_int, [_P(PhaseRetrieval), _u32, _u32, C.c_float, C.c_float, _P(C.c_uint32), _P(C.c_uint32),
                                                  _P(C.c_size_t)]),
    "paris_hip_phase_retrieval_host": (C.c_int, [_P(PhaseRetrieval), C.c_float, C.c_float, _vp, _vp, _u32, _u32]),
    "paris_hip_set_phase_retrieval": (C.c_int, [_vp, _P(PhaseRetrieval), _u32, _u32, C.c_float, C.c_float]),
    "paris_hip_clear_phase_retrieval": (C.c_int, [_vp]),
    "paris_hip_phase_retrieval_frames": (C.c_int, [_vp, _vp, _sz, _sz, _u32, _u32, _u32]),
    "paris_hip_scatter_default_margin": (C.c_uint32, [C.c_float, C.c_float, C.c_float, C.c_float]),
    "paris_hip_scatter_correction_check": (C.c_int, [_P(ScatterCorrection), _u32, _u32, C.c_float, C.c_float, _P(C.c_uint32), _P(C.c_uint32),
                                                     _P(C.c_size_t)]),
    "paris_hip_scatter_correction_host": (C.c_int, [_P(ScatterCorrection), C.c_float, C.c_float, _vp, _vp, _u32, _u32]),
    "paris_hip_set_scatter_correction": (C.c_int, [_vp, _P(ScatterCorrection), _u32, _u32, C.c_float, C.c_float]),
    "paris_hip_clear_scatter_correction": (C.c_int, [_vp]),
    "paris_hip_scatter_correction_frames": (C.c_int, [_vp, _vp, _sz, _sz, _u32, _u32, _u32]),
    "paris_hip_starvation_filter_check": (C.c_int, [_P(StarvationFilter), _u32, _u32, _P(_sz)]),
    "paris_hip_starvation_filter_tables": (C.c_int, [_P(StarvationFilter), _vp, _vp]),
    "paris_hip_starvation_filter_host": (C.c_int, [_P(StarvationFilter), _vp, _vp, _u32, _u32, _P(StarvationCounts)]),
    "paris_hip_set_starvation_filter": (C.c_int, [_vp, _P(StarvationFilter), _u32, _u32]),
    "paris_hip_clear_starvation_filter": (C.c_int, [_vp]),
    "paris_hip_starvation_filter_frames": (C.c_int, [_vp, _vp, _sz, _sz, _u32, _u32, _u32]),
    "paris_hip_starvation_stats": (C.c_int, [_vp, _P(StarvationCounts), C.c_int]),
    "paris_hip_beam_hardening_check": (C.c_int, [_P(BeamHardening)]),
    "paris_hip_beam_hardening_host": (C.c_int, [_P(BeamHardening), _vp, _vp, C.c_uint64]),
    "paris_hip_set_beam_hardening": (C.c_int, [_vp, _P(BeamHardening), _u32, _u32]),
    "paris_hip_clear_beam_hardening": (C.c_int, [_vp]),
    "paris_hip_beam_hardening_rows": (C.c_int, [_vp, _vp, _sz, _sz, _u32, _u32, _u32, _u32, _u32]),
    "paris_hip_beam_hardening_rows_with": (C.c_int, [_vp, _P(BeamHardening), _vp, _sz, _sz, _u32, _u32, _u32, _u32, _u32]),
    "paris_hip_bh_threshold_from_histogram": (C.c_int, [_vp, _u32, _f, _f, _P(_f)]),
    "paris_hip_bh_classify": (C.c_int, [_vp, _vp, _u32, _u32, _u32, _f, _u32, _vp]),
    "paris_hip_bh_gram": (C.c_int, [_vp, _P(_vp), _u32, _vp, C.c_uint64, _vp, _P(BhCounts)]),
    "paris_hip_bh_gram_host": (C.c_int, [_P(_vp), _u32, _vp, C.c_uint64, _vp, _P(BhCounts)]),
    "paris_hip_bh_solve": (C.c_int, [_vp, _u32, _P(BhCounts), C.c_uint64, _P(BhFit)]),
    "paris_hip_lag_model_check": (C.c_int, [_P(LagModel)]),
    "paris_hip_lag_coefficients": (C.c_int, [_P(LagModel), _vp, _vp, _vp, _P(_f), _P(C.c_double)]),
    "paris_hip_lag_correct_host": (C.c_int, [_P(LagModel), _vp, _vp, _vp, _P(C.c_int), C.c_uint64, _u32]),
    "paris_hip_set_lag_correction": (C.c_int, [_vp, _P(LagModel)]),
    "paris_hip_clear_lag_correction": (C.c_int, [_vp]),
    "paris_hip_lag_begin": (C.c_int, [_vp, _u32, _u32, _u32, _u32]),
    "paris_hip_lag_end": (C.c_int, [_vp]),
    "paris_hip_lag_correct_rows": (C.c_int, [_vp, _vp, _sz, _sz, _u32, _u32, _u32, _u32, _u32]),
    "paris_hip_lag_frames": (C.c_int, [_vp, _P(C.c_uint64)]),
    "paris_hip_metal_check": (C.c_int, [_u32, _u32, _u32, _f, _u32, _f, _P(C.c_uint64)]),
    "paris_hip_metal_collect_host": (C.c_int, [_vp, _u32, _u32, _u32, _f, C.c_uint64, _vp, _vp, _P(C.c_uint64), C.c_int]),
    "paris_hip_metal_collect": (C.c_int, [_vp, _vp, _u32, _u32, _u32, _f, C.c_uint64, _vp, _vp, _P(C.c_uint64), C.c_int]),
    "paris_hip_metal_trace_pack_host": (C.c_int, [_vp, _u32, _u32, _u32, _f, _u32, _vp]),
    "paris_hip_metal_trace_pack": (C.c_int, [_vp, _vp, _sz, _sz, _u32, _u32, _u32, _f, _u32, _vp]),
    "paris_hip_metal_inpaint_host": (C.c_int, [_vp, _vp, _u32, _u32, _u32, _u32, _P(MetalCounts)]),
    "paris_hip_set_metal_trace": (C.c_int, [_vp, _vp, _u32, _u32, _u32]),
    "paris_hip_clear_metal_trace": (C.c_int, [_vp]),
    "paris_hip_metal_inpaint_rows": (C.c_int, [_vp, _vp, _sz, _sz, _u32, _u32, _u32, _u32, _u32, _vp]),
    "paris_hip_metal_stats": (C.c_int, [_vp, _P(MetalCounts), C.c_int]),
    "paris_hip_set_metal_voxels": (C.c_int, [_vp, _vp, _vp, C.c_uint64]),
    "paris_hip_clear_metal_voxels": (C.c_int, [_vp]),
    "paris_hip_metal_reinsert": (C.c_int, [_vp, _vp, _u32, _u32, _u32, _u32]),
    "paris_hip_row_extension_check": (C.c_int, [_P(RowExtension), _u32]),
    "paris_hip_row_extension_response": (C.c_int, [_P(RowExtension), _u32, _f, _vp]),
    "paris_hip_set_row_extension": (C.c_int, [_vp, _P(RowExtension)]),
    "paris_hip_clear_row_extension": (C.c_int, [_vp]),
    "paris_hip_memcpy_projection_d2h": (C.c_int, [_vp, _vp, _sz, _vp, _sz, _u32, _u32]),
    "paris_hip_memcpy_volume_h2d": (C.c_int, [_vp, _vp, _vp, _u32, _u32, _u32]),
    "paris_hip_memcpy_volume_d2h": (C.c_int, [_vp, _vp, _vp, _u32, _u32, _u32]),
    "paris_hip_memset_volume": (C.c_int, [_vp, _vp, _u32, _u32, _u32]),
    "paris_hip_make_subvolume_information": (C.c_int, [_P(VolumeGeometry), _P(DetectorGeometry), C.c_int,
                                                       _P(SubvolumeInfo)]),
    "paris_hip_make_subvolume_information_reserving": (C.c_int, [_P(VolumeGeometry), _P(DetectorGeometry), C.c_int, _sz,
                                                                 _P(SubvolumeInfo)]),
    "paris_hip_device_memory": (C.c_int, [C.c_int, _P(_sz), _P(_sz)]),
    "paris_hip_weight": (C.c_int, [_vp, _vp, _sz, _u32, _u32, _f, _f, _f, _f, _f]),
    "paris_hip_weight_rows": (C.c_int, [_vp, _vp, _sz, _u32, _u32, _u32, _u32, _f, _f, _f, _f, _f]),
    "paris_hip_make_filter": (C.c_int, [_vp, _u32, _f, _P(_vp)]),
    "paris_hip_make_filter_windowed": (C.c_int, [_vp, _u32, _f, C.c_int, _P(_vp)]),
    "paris_hip_set_filter_window": (C.c_int, [_vp, C.c_int]),
    "paris_hip_apply_filter": (C.c_int, [_vp, _vp, _sz, _u32, _u32, _vp, _u32, _u32]),
    "paris_hip_set_filter_variant": (C.c_int, [_vp, C.c_int]),
    "paris_hip_set_stage_fusion": (C.c_int, [_vp, C.c_int]),
    "paris_hip_set_backproject_skip_invalid": (C.c_int, [_vp, C.c_int]),
    "paris_hip_volume_mark_dirty": (C.c_int, [_vp, _vp, _sz]),
    "paris_hip_volume_mark_clean": (C.c_int, [_vp, _vp, _sz]),
    "paris_hip_set_filter_deferral": (C.c_int, [_vp, C.c_int]),
    "paris_hip_volume_scan_clean": (C.c_int, [_vp, _vp, _sz, C.POINTER(C.c_uint64)]),
    "paris_hip_weight_filter_rows": (C.c_int, [_vp, _vp, _sz, _u32, _u32, _u32, _u32, _f, _f, _f, _f, _f, _vp, _u32, _vp, _sz]),
    "paris_hip_weight_filter_batch": (C.c_int, [_vp, _vp, _sz, _sz, _u32, _u32, _u32, _u32, _u32, _f, _f, _f, _f, _f, _vp, _u32, _vp, _sz, _sz]),
    "paris_hip_stage_weight_filter_batch": (C.c_int, [_vp, _vp, _sz, _sz, _u32, _u32, _u32, _u32, _u32, _P(DetectorGeometry), _vp, _sz, _sz]),
    "paris_hip_backproject": (C.c_int, [_vp, _vp, _sz, _u32, _u32, _vp, _u32, _u32, _u32, _u32,
                                        _P(DetectorGeometry), _P(VolumeGeometry), C.c_int,
                                        _P(RegionOfInterest), _f, _f, _f, _f]),
    "paris_hip_backproject_f16": (C.c_int, [_vp, _vp, _sz, _u32, _u32, _vp, _u32, _u32, _u32, _u32,
                                            _P(DetectorGeometry), _P(VolumeGeometry), C.c_int,
                                            _P(RegionOfInterest), _f, _f, _f, _f]),
    "paris_hip_convert_projection_f16": (C.c_int, [_vp, _vp, _sz, _vp, _sz, _u32, _u32]),
    "paris_hip_backproject_batch": (C.c_int, [_vp, _vp, _sz, _sz, _u32, _u32, _u32, _vp, _u32, _u32, _u32, _u32,
                                              _P(DetectorGeometry), _P(VolumeGeometry), C.c_int,
                                              _P(RegionOfInterest), _P(_f), _P(_f), _f, _f]),
    "paris_hip_backproject_batch_f16": (C.c_int, [_vp, _vp, _sz, _sz, _u32, _u32, _u32, _vp, _u32, _u32, _u32, _u32,
                                              _P(DetectorGeometry), _P(VolumeGeometry), C.c_int,
                                              _P(RegionOfInterest), _P(_f), _P(_f), _f, _f]),
    "paris_hip_calculate_volume_geometry": (C.c_int, [_P(DetectorGeometry), _P(VolumeGeometry)]),
    "paris_hip_apply_roi": (C.c_int, [_P(VolumeGeometry), _P(RegionOfInterest), _P(VolumeGeometry)]),
    "paris_hip_stage_weight": (C.c_int, [_vp, _vp, _sz, _u32, _u32, _P(DetectorGeometry)]),
    "paris_hip_filter_size": (_u32, [_u32]),
    "paris_hip_stage_filter": (C.c_int, [_vp, _vp, _sz, _u32, _u32, _P(DetectorGeometry)]),
    "paris_hip_stage_weight_rows": (C.c_int, [_vp, _vp, _sz, _u32, _u32, _u32, _u32, _P(DetectorGeometry)]),
    "paris_hip_stage_filter_rows": (C.c_int, [_vp, _vp, _sz, _u32, _u32, _u32, _u32, _P(DetectorGeometry)]),
    "paris_hip_stage_weight_filter_rows": (C.c_int, [_vp, _vp, _sz, _u32, _u32, _u32, _u32, _P(DetectorGeometry), _vp, _sz]),
    "paris_hip_set_backproject_deferral": (C.c_int, [_vp, _u32]),
    "paris_hip_flush": (C.c_int, [_vp]),
    "paris_hip_lean_division_is_exact": (C.c_int, [_vp, _f, _f, _P(C.c_int)]),
    "paris_hip_lean_weighting_is_exact": (C.c_int, [_vp, _f, _f, _f, _P(C.c_int)]),
    "paris_hip_set_lean_validation": (C.c_int, [_vp, C.c_int]),
    "paris_hip_pending_backprojections": (C.c_int, [_vp, _P(_u32), _P(C.c_void_p)]),
    "paris_hip_set_backproject_overlap": (C.c_int, [_vp, C.c_int]),
    "paris_hip_set_backproject_references": (C.c_int, [_vp, C.c_int]),
    "paris_hip_set_async_validation": (C.c_int, [_vp, C.c_int]),
    "paris_hip_has_experiments": (C.c_int, []),
    "paris_hip_projection_reserve_bytes": (C.c_int, [_vp, _u32, _u32, _P(_sz)]),
    "paris_hip_slab_row_band": (C.c_int, [_P(DetectorGeometry), _P(VolumeGeometry), _u32, _u32, _u32, _u32, C.c_int,
                                          _P(RegionOfInterest), _P(_u32), _P(_u32)]),
    "paris_hip_stage_angle": (C.c_int, [_P(DetectorGeometry), _u32, C.c_int, _f, _P(_f), _P(_f)]),
    "paris_hip_short_scan_check": (C.c_int, [_P(DetectorGeometry), _P(ShortScan), _P(_f)]),
    "paris_hip_short_scan_weight_rows": (C.c_int, [_vp, _vp, _sz, _sz, _u32, _u32, _u32, _u32, _u32, _P(DetectorGeometry), _P(ShortScan),
                                                   _P(_f)]),
    "paris_hip_stage_short_scan_weight": (C.c_int, [_vp, _vp, _sz, _u32, _u32, _P(DetectorGeometry), _P(ShortScan), _u32, C.c_int,
                                                    _f]),
    "paris_hip_offset_detector_check": (C.c_int, [_P(DetectorGeometry), _P(_f)]),
    "paris_hip_offset_detector_weight_rows": (C.c_int, [_vp, _vp, _sz, _sz, _u32, _u32, _u32, _u32, _u32, _P(DetectorGeometry)]),
    "paris_hip_stage_offset_detector_weight": (C.c_int, [_vp, _vp, _sz, _u32, _u32, _P(DetectorGeometry)]),
    "paris_hip_stage_backproject": (C.c_int, [_vp, _vp, _sz, _u32, _u32, _u32, _f, _vp, _u32, _u32, _u32, _u32,
                                              _P(DetectorGeometry), _P(VolumeGeometry), C.c_int, C.c_int,
                                              _P(RegionOfInterest)]),
    "paris_hip_forward_project": (C.c_int, [_vp, _vp, _u32, _u32, _u32, _u32, _P(DetectorGeometry), _P(VolumeGeometry), _vp, _sz, _sz,
                                            _u32, _u32, _u32, _P(_f), _P(_f), _f, _f, C.c_int]),
    "paris_hip_stage_forward_project": (C.c_int, [_vp, _vp, _u32, _u32, _u32, _u32, _P(DetectorGeometry), _P(VolumeGeometry), _vp, _sz,
                                                  _u32, _u32, _u32, _f, C.c_int, C.c_int]),
    "paris_hip_volume_window_check": (C.c_int, [_P(VolumeWindow)]),
    "paris_hip_volume_window_from_histogram": (C.c_int, [_vp, _u32, _f, _f, C.c_double, C.c_double, _P(_f), _P(_f)]),
    "paris_hip_volume_quantize": (C.c_int, [_vp, _vp, C.c_uint64, _P(VolumeWindow), _vp]),
    "paris_hip_volume_quantize_d2h": (C.c_int, [_vp, _vp, C.c_uint64, _P(VolumeWindow), _vp]),
    "paris_hip_volume_quantize_counts": (C.c_int, [_vp, _P(VolumeCounts), C.c_int]),
    "paris_hip_volume_stats": (C.c_int, [_vp, _vp, C.c_uint64, _f, _f, _u32, _vp, _P(VolumeStatistics)]),
    "paris_hip_volume_bilateral_check": (C.c_int, [_P(VolumeBilateral)]),
    "paris_hip_volume_bilateral_tables": (C.c_int, [_P(VolumeBilateral), _vp, _vp, _P(_f)]),
    "paris_hip_volume_bilateral_host": (C.c_int, [_vp, _u32, _u32, _u32, _u32, _u32, _P(VolumeBilateral), _vp]),
    "paris_hip_volume_bilateral": (C.c_int, [_vp, _vp, _u32, _u32, _u32, _u32, _u32, _P(VolumeBilateral), _vp]),
    "paris_hip_strerror": (C.c_char_p, [C.c_int]),
    "paris_hip_version": (C.c_char_p, []),
    "paris_hip_last_backproject_ms": (C.c_int, [_vp, _P(_f)]),
    "paris_hip_backproject_timing_arm": (C.c_int, [_vp, _u32]),
    "paris_hip_backproject_timing_collect": (C.c_int, [_vp, _P(_f), _u32, _P(_u32)]),
    "paris_hip_set_backproject_variant": (C.c_int, [_vp, C.c_int]),
    "paris_hip_set_backproject_tuning": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int]),
    "paris_hip_set_backproject_order": (C.c_int, [_vp, C.c_int, C.c_int]),
    "paris_hip_set_backproject_slice_shape": (C.c_int, [_vp, C.c_int, C.c_int]),
    "paris_hip_set_backproject_fast_division": (C.c_int, [_vp, C.c_int]),
    "paris_hip_set_backproject_vector_staging": (C.c_int, [_vp, C.c_int]),
    "paris_hip_fast_division_is_exact": (C.c_int, [_vp, _f, _P(C.c_int)]),
}

_lib = None


def load():
    """Loads libparis_hip.so; raises if it is missing (the product has no CPU path)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                "paris_amd: %s not found -- build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "or `make -C paris_amd/csrc`; there is no CPU fallback" % LIB_PATH)
        if os.environ.get("PARIS_AMD_NO_TORCH") != "1":
            # PyTorch ships its own libamdhip64.so.7; loading it first makes this library bind to that same
            # runtime instance, so device pointers and streams can be shared with torch (plumbing only).
            try:
                import torch  # noqa: F401
            except ImportError:
                pass
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)  # AttributeError if the library lacks a declared symbol
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


def has_experiments():
    """True when the loaded library is the experiments build (make EXPERIMENTS=1)"""
    return bool(load().paris_hip_has_experiments())


class ParisHipError(RuntimeError):
    """Raised for a non-zero status; plays the role of paris::stage_runtime_error (src/exception.h:37-41)."""

    def __init__(self, status, where):
        self.status = status
        msg = load().paris_hip_strerror(status)
        super().__init__("%s failed: %s (status %d)" % (where, msg.decode() if msg else "?", status))


def check(status, where):
    if status != SUCCESS:
        raise ParisHipError(status, where)
