// Backend-neutral stage functions of the hot loop (src/main.cpp:100-104) for the HIP backend:
// load (src/loader.cpp:28-33), make_volume (src/make_volume.cpp:30-37), weight (src/weighting.cpp:32-45),
// filter (src/filtering.cpp:32-45), backproject (src/backprojection.cpp:37-69).
//
// The reference caches every derived constant in function-local statics (one geometry per process, SURVEY.md
// Q1/Q2); these versions derive them on every call through the paris_hip_stage_* entry points, so a process may
// reconstruct any number of geometries, slabs and ROIs.
#ifndef PARIS_AMD_HOST_STAGES_H_
#define PARIS_AMD_HOST_STAGES_H_

#include "hip/backend.h"

namespace paris
{
    namespace backend = hip;

    inline auto load(const backend::projection_host_type& p) -> backend::projection_device_type
    {
        auto d_p = backend::make_projection_device(p.dim_x, p.dim_y);
        backend::copy_h2d(p, d_p);
        return d_p;
    }

    inline auto make_volume(const subvolume_geometry& subvol_geo, bool last) -> backend::volume_device_type
    {
        // the last slab also takes the slices that did not divide evenly
        const auto dim_z = subvol_geo.dim_z + (last ? subvol_geo.remainder : 0u);
        return backend::make_volume_device(subvol_geo.dim_x, subvol_geo.dim_y, dim_z);
    }

    namespace detail
    {
        // the part of the chain that makes the line integrals the ring profile sums: correction, air normalisation, repair, zinger
        // filter
        inline auto line_integrals(backend::projection_device_type& p, const char* what) -> void
        {
            if(backend::detail::has_flat_field(backend::current_ctx()))
                backend::detail::runtime_check(paris_hip_flat_field_rows(backend::current_ctx(), p.buf.get(), p.buf.pitch(), 0u, 1u, p.dim_x, p.dim_y,
                                                                         0u, p.dim_y), what);
            if(backend::detail::has_air_region(backend::current_ctx()))
                backend::detail::runtime_check(paris_hip_air_normalize_rows(backend::current_ctx(), p.buf.get(), p.buf.pitch(), 0u, 1u, p.dim_x,
                                                                            p.dim_y, 0u, p.dim_y), what);
            if(backend::detail::has_defect_map(backend::current_ctx()))
                backend::detail::runtime_check(paris_hip_defect_repair_rows(backend::current_ctx(), p.buf.get(), p.buf.pitch(), 0u, 1u, p.dim_x,
                                                                            p.dim_y, 0u, p.dim_y), what);
            if(backend::detail::has_zinger_filter(backend::current_ctx()))
                backend::detail::runtime_check(paris_hip_zinger_filter_rows(backend::current_ctx(), p.buf.get(), p.buf.pitch(), 0u, 1u, p.dim_x,
                                                                            p.dim_y, 0u, p.dim_y), what);
        }
    }

    // the ring filter's pre-pass over one loaded frame, between backend::ring_profile_begin() and backend::ring_profile_finish(): the
    // frame goes through the chain paris::weight() runs in front of the ring correction and is added to the profile. It is not
    // weighted: reconstruct from a fresh load.
    inline auto ring_profile_add(backend::projection_device_type& p) -> void
    {
        detail::line_integrals(p, "ring_profile_add()");
        backend::ring_profile_add(p.buf.get(), p.buf.pitch(), p.dim_x, p.dim_y);
    }

    // the axis search's pre-pass over one loaded frame, between backend::axis_search_begin() and backend::axis_search_finish(): the
    // frame goes through the same chain and its mid-plane band becomes row `frame` of the sinogram. A frame that also feeds the ring
    // profile goes through ring_profile_add() first and then straight to backend::axis_search_add(): the chain runs once.
    inline auto axis_search_add(backend::projection_device_type& p, std::uint32_t frame) -> void
    {
        detail::line_integrals(p, "axis_search_add()");
        backend::axis_search_add(p.buf.get(), p.buf.pitch(), p.dim_x, p.dim_y, frame);
    }

    // with a dark / flat setting (backend::set_flat_field), the correction to line integrals comes first, then with an air region
    // (backend::set_air_region) the subtraction of the frame's own flux drift, measured where the detector sees only air (a constant
    // over the frame, so it must be gone before the repair averages pixels, before the zinger filter compares them with thresholds
    // and before the ring profile sums the frames), then with a defect map
    // (backend::set_defect_map) the repair of the defective pixels, then with a zinger filter (backend::set_zinger_filter) the removal
    // of the frame's outlier pixels, then with a ring correction (backend::set_ring_correction) the subtraction of the detector's
    // stationary offsets (additive in line integrals, so before every weight), then with an offset detector
    // (backend::set_offset_detector) or a short scan set (backend::set_short_scan) its redundancy weight, then the cosine weight: the only correct order (the weights are linear in the
    // line integrals, the correction is not; the repair averages line integrals, and every weight varies from pixel to pixel, so a
    // repaired pixel must get its OWN weight afterwards; a dead pixel the correction left at 0 must be repaired before the zinger
    // filter sees it, or it would be patched as a dark outlier by the wrong rule; and a median of weighted pixels is no weighted median)
    inline auto weight(backend::projection_device_type& p, const detector_geometry& det_geo) -> void
    {
        detail::line_integrals(p, "weight()");
        if(backend::detail::has_ring_correction(backend::current_ctx()))
            backend::detail::runtime_check(paris_hip_ring_correct_rows(backend::current_ctx(), p.buf.get(), p.buf.pitch(), 0u, 1u, p.dim_x,
                                                                       p.dim_y, 0u, p.dim_y), "weight()");
        // then with a starvation filter (backend::set_starvation_filter) the adaptive smoothing of the starved pixels: a ring offset
        // would shift a pixel's level, and the scatter estimate's source is steep exactly where the starved pixels are noisy
        if(backend::detail::has_starvation_filter(backend::current_ctx()))
            backend::starvation_filter(p.buf.get(), p.buf.pitch(), 0u, 1u, p.dim_x, p.dim_y);
        // then with a scatter setting (backend::set_scatter_correction) the kernel superposition: scatter is additive on the measured
        // intensity and must be gone before a filter or a polynomial acts on what is taken for the primary
        if(backend::detail::has_scatter_correction(backend::current_ctx()))
            backend::scatter_correction(p.buf.get(), p.buf.pitch(), 0u, 1u, p.dim_x, p.dim_y);
        // then with a phase-retrieval setting (backend::set_phase_retrieval) the low-pass of the transmission image: a ring offset is a
        // per-pixel gain in transmission and must be gone before a 2-D filter smears it; the polynomial acts on the retrieved integral
        if(backend::detail::has_phase_retrieval(backend::current_ctx()))
            backend::phase_retrieval(p.buf.get(), p.buf.pitch(), 0u, 1u, p.dim_x, p.dim_y);
        // then with a beam-hardening setting (backend::set_beam_hardening) the polynomial of the line integral: the last step that is
        // not linear in it, so before every weight
        if(backend::detail::has_beam_hardening(backend::current_ctx()))
            backend::detail::runtime_check(paris_hip_beam_hardening_rows(backend::current_ctx(), p.buf.get(), p.buf.pitch(), 0u, 1u, p.dim_x,
                                                                         p.dim_y, 0u, p.dim_y), "weight()");
        // then with a detector roll (backend::set_detector_roll) the resampling, the last frame pass: it reads one buffer and writes
        // another, so the projection takes the resampled buffer and lets go of its own
        if(backend::detail::has_detector_roll(backend::current_ctx()))
        {
            auto rolled = backend::make_projection_device(p.dim_x, p.dim_y);
            backend::detail::runtime_check(paris_hip_detector_roll_rows(backend::current_ctx(), p.buf.get(), p.buf.pitch(), 0u, rolled.buf.get(),
                                                                        rolled.buf.pitch(), 0u, 1u, p.dim_x, p.dim_y, 0u, p.dim_y), "weight()");
            std::swap(p.buf, rolled.buf);
        }
        // then with a metal trace (backend::set_metal_trace) the inpainting of the trace of view p.idx, on the detector the roll wrote
        if(backend::detail::has_metal_trace(backend::current_ctx()))
            backend::metal_inpaint(p.buf.get(), p.buf.pitch(), p.dim_x, p.dim_y, 0u, p.dim_y, p.idx);
        if(backend::detail::has_offset_detector(backend::current_ctx()))
            backend::detail::runtime_check(paris_hip_stage_offset_detector_weight(backend::current_ctx(), p.buf.get(), p.buf.pitch(), p.dim_x,
                                                                                  p.dim_y, &det_geo), "weight()");
        if(const auto* s = backend::detail::short_scan_of(backend::current_ctx()))
            backend::detail::runtime_check(paris_hip_stage_short_scan_weight(backend::current_ctx(), p.buf.get(), p.buf.pitch(), p.dim_x, p.dim_y,
                                                                             &det_geo, &s->scan, p.idx, s->enable_angles ? 1 : 0, p.phi),
                                           "weight()");
        backend::detail::runtime_check(paris_hip_stage_weight(backend::current_ctx(), p.buf.get(), p.buf.pitch(), p.dim_x,
                                                              p.dim_y, &det_geo), "weight()");
    }

    inline auto filter(backend::projection_device_type& p, const detector_geometry& det_geo) -> void
    {
        backend::detail::runtime_check(paris_hip_stage_filter(backend::current_ctx(), p.buf.get(), p.buf.pitch(), p.dim_x,
                                                              p.dim_y, &det_geo), "filter()");
    }

    inline auto backproject(const backend::projection_device_type& p, backend::volume_device_type& v,
                            std::uint32_t v_offset, const detector_geometry& det_geo, const volume_geometry& vol_geo,
                            bool enable_angles, bool enable_roi, const region_of_interest& roi) -> void
    {
        backend::detail::runtime_check(
            paris_hip_stage_backproject(backend::current_ctx(), p.buf.get(), p.buf.pitch(), p.dim_x, p.dim_y, p.idx, p.phi,
                                        v.buf.get(), v.dim_x, v.dim_y, v.dim_z, v_offset, &det_geo, &vol_geo,
                                        enable_angles ? 1 : 0, enable_roi ? 1 : 0, &roi),
            "backproject()");
    }
}

#endif
