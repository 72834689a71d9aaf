// namespace paris::hip -- the MI355X backend behind the PARIS backend surface.
//
// Same types and the same 14 free functions as src/openmp/backend.h:42-89 / src/cuda/backend.h:50-103 (cleanest
// statement: src/generic/backend.h:54-88), implemented over the C ABI of include/paris_hip.h. A maintainer adds
//     #elif defined(PARIS_ENABLE_HIP)
//     #include "hip/backend.h"          // + `namespace backend = hip;` in the alias block
// to src/backend.h:26-47.
//
// Per-device state: the reference binds a host thread to a device with set_device() and keeps everything else
// in thread_local statics. Here set_device() creates (once per thread and device) the paris_hip_ctx that holds
// that state; every other function uses the calling thread's current ctx. Calls enqueue on the ctx's stream and only
// the copies to the host wait (PARIS_HIP_SYNCHRONOUS_CALLS=1 restores the reference's sync-per-call). A non-zero C status becomes stage_runtime_error (stage_construction_error for allocation and
// subvolume planning), after which the reference's main() aborts (src/main.cpp:181-192).
#ifndef PARIS_AMD_HOST_HIP_BACKEND_H_
#define PARIS_AMD_HOST_HIP_BACKEND_H_

#ifndef PARIS_HIP_BACKPROJECT_DEFERRAL
#define PARIS_HIP_BACKPROJECT_DEFERRAL 48
#endif
// 1 (default): weight() is held back and rides along in the load of the apply_filter() call that follows (one launch per
// weight / filter pair of src/main.cpp:102-103; paris_hip_set_stage_fusion). 0: one launch per call.
#ifndef PARIS_HIP_STAGE_FUSION
#define PARIS_HIP_STAGE_FUSION 1
#endif
// 2 (default): the apply_filter() of that pair is held back too when nobody can tell -- the projection is a make_projection_device
// buffer that a deferred backproject() takes by reference (PARIS_HIP_BACKPROJECT_REFERENCES): weighting + filter then run IN PLACE, one
// launch for the whole group right before its fused backprojection, and every other call that touches the buffer runs them first
// (paris_hip_set_filter_deferral(2)). 1: held back whenever a backprojection follows (a snapshotted projection's own buffer then
// keeps its unfiltered pixels). 0: the filter runs when it is called. Round 4 left this off: the ring's snapshots made it visible
// in the caller's buffer, and the loop was bound elsewhere; with references it is invisible and removes a launch per projection
// from the host's path (profiles/r05_demo_paris_hip_mirror.txt).
#ifndef PARIS_HIP_FILTER_DEFERRAL
#define PARIS_HIP_FILTER_DEFERRAL 2
#endif
// 1: every backend call returns after its work has finished, like the reference's backends (stream sync before return:
// src/cuda/weighting.cu:72, filtering.cu:260, backprojection.cu:236). 0 (default): calls enqueue and return; only the
// copies to the host wait. The call sequence of src/main.cpp:98-105 observes results through copy_d2h alone, and the
// library hands a released host / device projection buffer out again only after the work that used it has finished, so
// the loop's allocate / fill / load / free per projection stays correct while host and GPU work overlap.
#ifndef PARIS_HIP_SYNCHRONOUS_CALLS
#define PARIS_HIP_SYNCHRONOUS_CALLS 0
#endif
// 1 (default): a full group's fused backprojection runs on the ctx's second stream and copy_h2d(projection) on its upload stream, so
// that the next group's uploads, filters and snapshots -- which PARIS's loop keeps issuing, src/main.cpp:98-105 -- pass the running
// launch instead of queueing behind it (paris_hip_set_backproject_overlap, paris_hip_upload_projection). The library orders every
// observer of the volume behind the launches; results are bit-identical. 0: one stream for everything.
#ifndef PARIS_HIP_BACKPROJECT_OVERLAP
#define PARIS_HIP_BACKPROJECT_OVERLAP 1
#endif

// 1 (default): a deferred backproject() of a make_projection_device buffer takes no snapshot -- the group's fused launch reads the
// buffer itself, the buffer PARIS's loop frees right after the call (src/main.cpp:98-105, src/loader.cpp:28-33) goes back to the
// pool behind that launch, and anything else that touches it first launches the group (paris_hip_set_backproject_references). 0:
// every call snapshots its projection into the library's ring.
#ifndef PARIS_HIP_BACKPROJECT_REFERENCES
#define PARIS_HIP_BACKPROJECT_REFERENCES 1
#endif

// Which stream copy_h2d(projection) runs on. 1: the ctx's upload stream (paris_hip_upload_projection; the compute stream is ordered
// behind every copy by an event pair, ~2.3 us of runtime calls per frame): what the loop needs when kernels of its own -- a filter
// per projection, snapshot copies -- share the compute stream with the copies. 0: the compute stream itself. Default: 0 when the
// projections are taken by reference and filtered in place a group at a time (PARIS_HIP_BACKPROJECT_REFERENCES with
// PARIS_HIP_FILTER_DEFERRAL 2, which needs PARIS_HIP_STAGE_FUSION): the loop then enqueues NOTHING but its copies on the compute stream -- the group's filter and fused
// launch run on the second stream, ordered behind the copies by the one event each launch records anyway -- so a stream of their own
// buys the copies nothing and costs the event pair; 1 otherwise.
#ifndef PARIS_HIP_UPLOAD_ON_ITS_OWN_STREAM
#define PARIS_HIP_UPLOAD_ON_ITS_OWN_STREAM                                                                                        \
    (PARIS_HIP_BACKPROJECT_OVERLAP                                                                                               \
     && !(PARIS_HIP_BACKPROJECT_REFERENCES && PARIS_HIP_FILTER_DEFERRAL == 2 && PARIS_HIP_STAGE_FUSION && PARIS_HIP_BACKPROJECT_DEFERRAL > 1))
#endif

#include <cstddef>
#include <cstdint>
#include <map>
#include <set>
#include <memory>
#include <string>
#include <vector>

#if defined(PARIS_HIP_INSIDE_PARIS)
// Installed as src/hip/backend.h of a PARIS checkout: PARIS's own value types are used and handed to the C ABI by
// pointer (they are field-for-field the C structs: checked below).
#include "../exception.h"
#include "../geometry.h"
#include "../projection.h"
#include "../region_of_interest.h"
#include "../subvolume_information.h"
#include "../volume.h"
#include "paris_hip.h"
#else
#include "../types.h"
#endif

namespace paris
{
    namespace hip
    {
        using device_handle = int;

        namespace detail
        {
            // PARIS value types -> C ABI structs. With ../types.h they are the same types; inside PARIS they are
            // layout-identical PODs.
            template <typename To, typename From>
            inline auto as_c(const From& v) noexcept -> const To*
            {
                static_assert(sizeof(To) == sizeof(From) && alignof(To) == alignof(From), "PARIS type and C ABI struct differ");
                return reinterpret_cast<const To*>(&v);
            }
            static_assert(offsetof(detector_geometry, delta_phi) == offsetof(paris_detector_geometry, delta_phi), "detector_geometry");
            static_assert(offsetof(volume_geometry, l_vx_z) == offsetof(paris_volume_geometry, l_vx_z), "volume_geometry");
            static_assert(offsetof(region_of_interest, z2) == offsetof(paris_region_of_interest, z2), "region_of_interest");
            static_assert(offsetof(subvolume_info, num) == offsetof(paris_subvolume_info, num), "subvolume_info");

            struct ctx_deleter { void operator()(paris_hip_ctx* c) const noexcept { paris_hip_ctx_destroy(c); } };

            struct short_scan_setting
            {
                paris_short_scan scan;
                bool enable_angles;
            };

            struct thread_state
            {
                std::map<device_handle, std::unique_ptr<paris_hip_ctx, ctx_deleter>> per_device;
                paris_hip_ctx* current = nullptr;
                std::map<const paris_hip_ctx*, short_scan_setting> short_scans; // set_short_scan(), per device of this thread
                std::set<const paris_hip_ctx*> flat_fields; // set_flat_field(), per device of this thread
                std::set<const paris_hip_ctx*> offset_detectors; // set_offset_detector(), per device of this thread
                std::set<const paris_hip_ctx*> defect_maps; // set_defect_map(), per device of this thread
                std::set<const paris_hip_ctx*> zinger_filters; // set_zinger_filter(), per device of this thread
                std::set<const paris_hip_ctx*> ring_corrections; // set_ring_correction(), per device of this thread
                std::set<const paris_hip_ctx*> air_regions; // set_air_region(), per device of this thread
                std::set<const paris_hip_ctx*> beam_hardenings; // set_beam_hardening(), per device of this thread
                std::set<const paris_hip_ctx*> phase_retrievals; // set_phase_retrieval(), per device of this thread
                std::set<const paris_hip_ctx*> scatter_corrections; // set_scatter_correction(), per device of this thread
                std::set<const paris_hip_ctx*> starvation_filters;  // set_starvation_filter(), per device of this thread
                std::set<const paris_hip_ctx*> detector_rolls; // set_detector_roll(), per device of this thread
                std::set<const paris_hip_ctx*> metal_traces;   // set_metal_trace(), per device of this thread
            };

            inline auto state() -> thread_state&
            {
                thread_local thread_state s;
                return s;
            }

            inline void runtime_check(int rc, const char* what)
            {
                if(rc != PARIS_HIP_SUCCESS)
                    throw stage_runtime_error{std::string{what} + " failed: " + paris_hip_strerror(rc)};
            }

            inline void construction_check(int rc, const char* what)
            {
                if(rc != PARIS_HIP_SUCCESS)
                    throw stage_construction_error{std::string{what} + " failed: " + paris_hip_strerror(rc)};
            }
        }

        // ---- device management (src/cuda/device.cpp:31-47) --------------------------------------------------
        inline auto get_devices() -> std::vector<device_handle>
        {
            int n = 0;
            detail::construction_check(paris_hip_device_count(&n), "get_devices()");
            auto v = std::vector<device_handle>{};
            for(int d = 0; d < n; ++d)
                v.push_back(d);
            return v;
        }

        inline auto set_device(device_handle& d) -> int
        {
            auto& s = detail::state();
            auto it = s.per_device.find(d);
            if(it == s.per_device.end())
            {
                paris_hip_ctx* c = nullptr;
                detail::construction_check(paris_hip_ctx_create(d, nullptr, (PARIS_HIP_SYNCHRONOUS_CALLS ? PARIS_HIP_CTX_SYNCHRONOUS : PARIS_HIP_CTX_DEFAULT) | PARIS_HIP_CTX_WARM, &c),
                                           "set_device()");
                // PARIS calls backproject() once per projection (src/main.cpp:98-105). The library snapshots each call's
                // projection and adds PARIS_HIP_BACKPROJECT_DEFERRAL of them with one fused launch -- bit-identical, the
                // slab is read and written once per group instead of once per projection -- and flushes before anything
                // observes the volume (copy_d2h, free): see paris_hip_set_backproject_deferral. 1 = one launch per call.
                detail::construction_check(paris_hip_set_backproject_deferral(c, PARIS_HIP_BACKPROJECT_DEFERRAL), "set_device()");
                detail::construction_check(paris_hip_set_stage_fusion(c, PARIS_HIP_STAGE_FUSION), "set_device()");
                detail::construction_check(paris_hip_set_filter_deferral(c, PARIS_HIP_FILTER_DEFERRAL), "set_device()");
                detail::construction_check(paris_hip_set_backproject_overlap(c, PARIS_HIP_BACKPROJECT_OVERLAP), "set_device()");
                detail::construction_check(paris_hip_set_backproject_references(c, PARIS_HIP_BACKPROJECT_REFERENCES && !PARIS_HIP_SYNCHRONOUS_CALLS),
                                           "set_device()");
                // validators of the hand-expanded IEEE sequences run beside the first projections instead of in front of them
                detail::construction_check(paris_hip_set_async_validation(c, !PARIS_HIP_SYNCHRONOUS_CALLS), "set_device()");
                it = s.per_device.emplace(d, std::unique_ptr<paris_hip_ctx, detail::ctx_deleter>{c}).first;
            }
            s.current = it->second.get();
            return 0;
        }

        inline auto current_ctx() -> paris_hip_ctx*
        {
            auto& s = detail::state();
            if(s.current == nullptr)
            {
                auto d = device_handle{0}; // the reference's single-device path never calls set_device explicitly
                set_device(d);
            }
            return s.current;
        }

        // Extension (no reference counterpart): the projections of this thread's current device form a short scan over
        // [start_deg, start_deg + range_deg] (paris_short_scan). Until clear_short_scan(), paris::weight() first applies the Parker
        // redundancy weight to each projection, its angle taken from p.idx / p.phi as backproject() takes it (enable_angles: the
        // angle file's phi). The scan is checked against the detector at each weight(): a range below 180 degrees plus twice the fan
        // angle throws stage_runtime_error.
        inline auto set_short_scan(float start_deg, float range_deg, bool enable_angles) -> void
        {
            if(detail::state().offset_detectors.count(current_ctx()) != 0u)
                throw stage_runtime_error{"set_short_scan(): an offset detector is set on this device; a short scan with an offset detector needs "
                                          "a different weight"};
            detail::state().short_scans[current_ctx()] = detail::short_scan_setting{paris_short_scan{start_deg, range_deg}, enable_angles};
        }

        inline auto clear_short_scan() -> void
        {
            detail::state().short_scans.erase(current_ctx());
        }

        namespace detail
        {
            // the short scan set for the calling thread's current device, or nullptr
            inline auto short_scan_of(const paris_hip_ctx* ctx) -> const short_scan_setting*
            {
                const auto& m = state().short_scans;
                if(m.empty())
                    return nullptr;
                const auto it = m.find(ctx);
                return it == m.end() ? nullptr : &it->second;
            }
        }

        // Extension (no reference counterpart): the projections of this thread's current device come from an offset detector (half fan)
        // over a full circle. Until clear_offset_detector(), paris::weight() applies the offset-detector redundancy weight to each
        // projection, after a dark / flat correction and before the cosine weight (paris_hip_stage_offset_detector_weight). The detector
        // is checked at each weight(): an overlap tau below 2 pixels throws stage_runtime_error. Set together with a short scan on
        // the same device, whichever setter comes second throws stage_runtime_error.
        inline auto set_offset_detector() -> void
        {
            if(detail::state().short_scans.count(current_ctx()) != 0u)
                throw stage_runtime_error{"set_offset_detector(): a short scan is set on this device; a short scan with an offset detector needs "
                                          "a different weight"};
            detail::state().offset_detectors.insert(current_ctx());
        }

        inline auto clear_offset_detector() -> void
        {
            detail::state().offset_detectors.erase(current_ctx());
        }

        namespace detail
        {
            inline auto has_offset_detector(const paris_hip_ctx* ctx) -> bool
            {
                const auto& s = state().offset_detectors;
                return !s.empty() && s.count(ctx) != 0u;
            }
        }

        // Extension (no reference counterpart): the projections of this thread's current device are intensities. Until
        // clear_flat_field(), paris::weight() first turns each into line integrals with these dark and flat frames (n_row x n_col
        // floats each, rows n_row apart; dark nullptr = zeros): p = -ln(max((I - D) / (F - D), t_min)), dead pixels 0
        // (paris_hip_set_flat_field). The library keeps its own copy of the frames.
        inline auto set_flat_field(const float* dark, const float* flat, std::uint32_t n_row, std::uint32_t n_col, float t_min = 1e-5f) -> void
        {
            detail::runtime_check(paris_hip_set_flat_field(current_ctx(), dark, flat, n_row, n_col, t_min), "set_flat_field()");
            detail::state().flat_fields.insert(current_ctx());
        }

        inline auto clear_flat_field() -> void
        {
            detail::runtime_check(paris_hip_clear_flat_field(current_ctx()), "clear_flat_field()");
            detail::state().flat_fields.erase(current_ctx());
        }

        namespace detail
        {
            inline auto has_flat_field(const paris_hip_ctx* ctx) -> bool
            {
                const auto& s = state().flat_fields;
                return !s.empty() && s.count(ctx) != 0u;
            }
        }

        // Extension (no reference counterpart): the source's output drifts from frame to frame while the flat was taken once, and
        // the rectangle columns [x0, x0 + width), rows [y0, y0 + height) of this thread's current device's frames (n_row x n_col
        // pixels) sees only air in every view. Until clear_air_region(), paris::weight() subtracts from every
        // frame the mean line integral of the rectangle's counting pixels -- mask byte 0 (mask: n_col rows of n_row bytes, nonzero =
        // bad, or nullptr) and a finite value -- directly after the dark / flat correction and before the defect repair
        // (paris_hip_air_normalize_rows). A frame with fewer than min_pixels (0 = half the rectangle) of them, or whose value exceeds
        // limit_abs (0 = no limit), stays as it is; air_stats() counts both.
        inline auto set_air_region(std::uint32_t x0, std::uint32_t y0, std::uint32_t width, std::uint32_t height, std::uint32_t n_row,
                                   std::uint32_t n_col, std::uint32_t min_pixels = 0u, float limit_abs = 0.f,
                                   const std::uint8_t* mask = nullptr) -> void
        {
            const auto setting = paris_hip_air_region{x0, y0, width, height, min_pixels, limit_abs};
            detail::runtime_check(paris_hip_set_air_region(current_ctx(), &setting, mask, n_row, n_col), "set_air_region()");
            detail::state().air_regions.insert(current_ctx());
        }

        inline auto clear_air_region() -> void
        {
            detail::runtime_check(paris_hip_clear_air_region(current_ctx()), "clear_air_region()");
            detail::state().air_regions.erase(current_ctx());
        }

        // what paris::weight() has counted since set_air_region() or the last reset; waits for the device
        inline auto air_stats(bool reset = false) -> paris_hip_air_counts
        {
            auto out = paris_hip_air_counts{};
            detail::runtime_check(paris_hip_air_stats(current_ctx(), &out, reset ? 1 : 0), "air_stats()");
            return out;
        }

        namespace detail
        {
            inline auto has_air_region(const paris_hip_ctx* ctx) -> bool
            {
                const auto& s = state().air_regions;
                return !s.empty() && s.count(ctx) != 0u;
            }
        }

        // Extension (no reference counterpart): at magnification the frames of this thread's current device (n_row x n_col pixels with
        // the pitches l_px_row, l_px_col) show propagation fringes. Until clear_phase_retrieval(),
        // paris::weight() low-passes the transmission of every frame with 1 / (1 + alpha f^2) -- Paganin's single-distance filter --
        // after the ring correction and before the beam-hardening polynomial (paris_hip_phase_retrieval_frames).
        inline auto set_phase_retrieval(float alpha_mm2, float t_min, std::uint32_t margin, std::uint32_t n_row, std::uint32_t n_col, float l_px_row,
                                        float l_px_col) -> void
        {
            const auto setting = paris_hip_phase_retrieval{alpha_mm2, t_min, margin};
            detail::runtime_check(paris_hip_set_phase_retrieval(current_ctx(), &setting, n_row, n_col, l_px_row, l_px_col), "set_phase_retrieval()");
            detail::state().phase_retrievals.insert(current_ctx());
        }

        inline auto clear_phase_retrieval() -> void
        {
            detail::runtime_check(paris_hip_clear_phase_retrieval(current_ctx()), "clear_phase_retrieval()");
            detail::state().phase_retrievals.erase(current_ctx());
        }

        // the pass itself, on n_frames whole frames frame_stride bytes apart
        inline auto phase_retrieval(float* d_p, std::size_t pitch, std::size_t frame_stride, std::uint32_t n_frames, std::uint32_t n_row,
                                    std::uint32_t n_col) -> void
        {
            detail::runtime_check(paris_hip_phase_retrieval_frames(current_ctx(), d_p, pitch, frame_stride, n_frames, n_row, n_col), "phase_retrieval()");
        }

        namespace detail
        {
            inline auto has_phase_retrieval(const paris_hip_ctx* ctx) -> bool
            {
                const auto& s = state().phase_retrievals;
                return !s.empty() && s.count(ctx) != 0u;
            }
        }

        // Extension (no reference counterpart): the frames of this thread's current device (n_row x n_col pixels with the pitches l_px_row,
        // l_px_col) carry object scatter. Until clear_scatter_correction(), paris::weight() solves
        // T_m = T + (q(T) (*) g) for the primary of every frame -- kernel superposition, iterated -- after the ring correction and before
        // the phase retrieval (paris_hip_scatter_correction_frames).
        inline auto set_scatter_correction(const paris_hip_scatter_correction& setting, std::uint32_t n_row, std::uint32_t n_col, float l_px_row,
                                           float l_px_col) -> void
        {
            detail::runtime_check(paris_hip_set_scatter_correction(current_ctx(), &setting, n_row, n_col, l_px_row, l_px_col), "set_scatter_correction()");
            detail::state().scatter_corrections.insert(current_ctx());
        }

        inline auto clear_scatter_correction() -> void
        {
            detail::runtime_check(paris_hip_clear_scatter_correction(current_ctx()), "clear_scatter_correction()");
            detail::state().scatter_corrections.erase(current_ctx());
        }

        // the pass itself, on n_frames whole frames frame_stride bytes apart
        inline auto scatter_correction(float* d_p, std::size_t pitch, std::size_t frame_stride, std::uint32_t n_frames, std::uint32_t n_row,
                                       std::uint32_t n_col) -> void
        {
            detail::runtime_check(paris_hip_scatter_correction_frames(current_ctx(), d_p, pitch, frame_stride, n_frames, n_row, n_col), "scatter_correction()");
        }

        namespace detail
        {
            inline auto has_scatter_correction(const paris_hip_ctx* ctx) -> bool
            {
                const auto& s = state().scatter_corrections;
                return !s.empty() && s.count(ctx) != 0u;
            }
        }

        // Extension (no reference counterpart): along the longest paths the frames of this thread's current device (n_row x n_col pixels)
        // count a handful of photons. Until clear_starvation_filter(), paris::weight() smooths every frame where
        // its line integral lies above setting.p0, the more the higher it is, after the ring correction and before the scatter correction
        // (paris_hip_starvation_filter_frames).
        inline auto set_starvation_filter(const paris_hip_starvation_filter& setting, std::uint32_t n_row, std::uint32_t n_col) -> void
        {
            detail::runtime_check(paris_hip_set_starvation_filter(current_ctx(), &setting, n_row, n_col), "set_starvation_filter()");
            detail::state().starvation_filters.insert(current_ctx());
        }

        inline auto clear_starvation_filter() -> void
        {
            detail::runtime_check(paris_hip_clear_starvation_filter(current_ctx()), "clear_starvation_filter()");
            detail::state().starvation_filters.erase(current_ctx());
        }

        // the pass itself, on n_frames whole frames frame_stride bytes apart
        inline auto starvation_filter(float* d_p, std::size_t pitch, std::size_t frame_stride, std::uint32_t n_frames, std::uint32_t n_row,
                                      std::uint32_t n_col) -> void
        {
            detail::runtime_check(paris_hip_starvation_filter_frames(current_ctx(), d_p, pitch, frame_stride, n_frames, n_row, n_col), "starvation_filter()");
        }

        namespace detail
        {
            inline auto has_starvation_filter(const paris_hip_ctx* ctx) -> bool
            {
                const auto& s = state().starvation_filters;
                return !s.empty() && s.count(ctx) != 0u;
            }
        }

        // Extension (no reference counterpart): the tube is polychromatic, so the line integrals of this thread's current device's
        // frames (n_row x n_col pixels) are concave in the path length. Until clear_beam_hardening(),
        // paris::weight() turns every line integral p >= 0 into c[0] p + c[1] p^2 + ... (degree coefficients, 1 .. 4, each finite) and a
        // negative one into c[0] p, after the ring correction and before every weight (paris_hip_beam_hardening_rows).
        inline auto set_beam_hardening(const float* c, std::uint32_t degree, std::uint32_t n_row, std::uint32_t n_col) -> void
        {
            auto setting = paris_hip_beam_hardening{};
            setting.degree = degree;
            for(std::uint32_t k = 0; c != nullptr && k < degree && k < PARIS_HIP_BH_DEGREE_MAX; ++k)
                setting.c[k] = c[k];
            detail::runtime_check(c == nullptr ? PARIS_HIP_ERROR_INVALID_ARGUMENT : paris_hip_set_beam_hardening(current_ctx(), &setting, n_row, n_col),
                                  "set_beam_hardening()");
            detail::state().beam_hardenings.insert(current_ctx());
        }

        inline auto clear_beam_hardening() -> void
        {
            detail::runtime_check(paris_hip_clear_beam_hardening(current_ctx()), "clear_beam_hardening()");
            detail::state().beam_hardenings.erase(current_ctx());
        }

        // The pieces of the fit on this thread's current device, thin wrappers over the C calls: the labels of a slab of f_1, the
        // Gram sums of the basis slabs over them (waits for the device), and -- host only -- the threshold and the solve.
        inline auto bh_threshold_from_histogram(const std::uint64_t* hist, std::uint32_t n_bins, float h_lo, float h_hi) -> float
        {
            float thr = 0.f;
            detail::runtime_check(paris_hip_bh_threshold_from_histogram(hist, n_bins, h_lo, h_hi, &thr), "bh_threshold_from_histogram()");
            return thr;
        }

        inline auto bh_classify(const float* d_v, std::uint32_t dim_x, std::uint32_t dim_y, std::uint32_t dim_z, float thr, std::uint32_t margin,
                                std::uint8_t* d_labels) -> void
        {
            detail::runtime_check(paris_hip_bh_classify(current_ctx(), d_v, dim_x, dim_y, dim_z, thr, margin, d_labels), "bh_classify()");
        }

        inline auto bh_gram(const float* const* d_f, std::uint32_t degree, const std::uint8_t* d_labels, std::uint64_t n_voxels, double* gram)
            -> paris_hip_bh_counts
        {
            auto counts = paris_hip_bh_counts{};
            detail::runtime_check(paris_hip_bh_gram(current_ctx(), d_f, degree, d_labels, n_voxels, gram, &counts), "bh_gram()");
            return counts;
        }

        inline auto bh_solve(const double* gram, std::uint32_t degree, const paris_hip_bh_counts& counts, std::uint64_t min_voxels = 0u) -> paris_hip_bh_fit
        {
            auto fit = paris_hip_bh_fit{};
            detail::runtime_check(paris_hip_bh_solve(gram, degree, &counts, min_voxels, &fit), "bh_solve()");
            return fit;
        }

        namespace detail
        {
            inline auto has_beam_hardening(const paris_hip_ctx* ctx) -> bool
            {
                const auto& s = state().beam_hardenings;
                return !s.empty() && s.count(ctx) != 0u;
            }
        }

        // Extension (no reference counterpart): the detector of this thread's current device's frames is rotated in its own plane by
        // eta_deg degrees. Until clear_detector_roll(), paris::weight() resamples every frame onto a detector
        // whose rows are perpendicular to the projected rotation axis, after the beam-hardening correction and before every weight
        // (paris_hip_detector_roll_rows): the projection's buffer is exchanged for the resampled one. Off unless called.
        inline auto set_detector_roll(float eta_deg, const detector_geometry& det_geo) -> void
        {
            const auto setting = paris_hip_detector_roll{eta_deg};
            detail::runtime_check(paris_hip_set_detector_roll(current_ctx(), &setting, detail::as_c<paris_detector_geometry>(det_geo)), "set_detector_roll()");
            detail::state().detector_rolls.insert(current_ctx());
        }

        inline auto clear_detector_roll() -> void
        {
            detail::runtime_check(paris_hip_clear_detector_roll(current_ctx()), "clear_detector_roll()");
            detail::state().detector_rolls.erase(current_ctx());
        }

        namespace detail
        {
            inline auto has_detector_roll(const paris_hip_ctx* ctx) -> bool
            {
                const auto& s = state().detector_rolls;
                return !s.empty() && s.count(ctx) != 0u;
            }
        }

        // Extension (no reference counterpart): the detector of this thread's current device has defective pixels -- mask is n_col
        // rows of n_row bytes, nonzero = defective. Until clear_defect_map(), paris::weight() replaces each defective pixel by the
        // inverse-square-distance weighted mean of the good pixels on the nearest ring that holds one (paris_hip_set_defect_map), after
        // a dark / flat correction and before every weight. The library keeps its own plan of the map.
        inline auto set_defect_map(const std::uint8_t* mask, std::uint32_t n_row, std::uint32_t n_col) -> void
        {
            detail::runtime_check(paris_hip_set_defect_map(current_ctx(), mask, n_row, n_col), "set_defect_map()");
            detail::state().defect_maps.insert(current_ctx());
        }

        inline auto clear_defect_map() -> void
        {
            detail::runtime_check(paris_hip_clear_defect_map(current_ctx()), "clear_defect_map()");
            detail::state().defect_maps.erase(current_ctx());
        }

        namespace detail
        {
            inline auto has_defect_map(const paris_hip_ctx* ctx) -> bool
            {
                const auto& s = state().defect_maps;
                return !s.empty() && s.count(ctx) != 0u;
            }
        }

        // Extension (no reference counterpart): the frames of this thread's current device (n_row x n_col pixels) hold zingers --
        // direct hits in the sensor, in one frame only. Until clear_zinger_filter(), paris::weight() replaces every pixel that differs
        // from the median m of its 3 x 3 window by more than threshold_abs + threshold_rel * |m| -- above it (polarity +1), below it
        // (-1) or either (0) -- with m, unless more than max_hits (0 = default) pixels of the frame are flagged
        // (paris_hip_set_zinger_filter), after the defect repair and before every weight.
        inline auto set_zinger_filter(float threshold_abs, float threshold_rel, int polarity, std::uint32_t n_row, std::uint32_t n_col,
                                      std::uint32_t max_hits = 0u) -> void
        {
            const auto setting = paris_hip_zinger_filter{threshold_abs, threshold_rel, polarity, max_hits};
            detail::runtime_check(paris_hip_set_zinger_filter(current_ctx(), &setting, n_row, n_col), "set_zinger_filter()");
            detail::state().zinger_filters.insert(current_ctx());
        }

        inline auto clear_zinger_filter() -> void
        {
            detail::runtime_check(paris_hip_clear_zinger_filter(current_ctx()), "clear_zinger_filter()");
            detail::state().zinger_filters.erase(current_ctx());
        }

        // Extension (no reference counterpart): the projections of this thread's current device are laterally truncated -- the object
        // is wider than the detector. Until clear_row_extension(), paris::filter() acts as if every row continued beyond either edge
        // as the mean of its edge_pixels (1, 2, 4 or 8) outermost weighted pixels times a cos^2 taper of taper_pixels pixels, instead
        // of dropping to 0 (paris_hip_set_row_extension). Runs what is held back or pending first.
        inline auto set_row_extension(std::uint32_t edge_pixels, std::uint32_t taper_pixels) -> void
        {
            const auto setting = paris_hip_row_extension{edge_pixels, taper_pixels};
            detail::runtime_check(paris_hip_set_row_extension(current_ctx(), &setting), "set_row_extension()");
        }

        inline auto clear_row_extension() -> void
        {
            detail::runtime_check(paris_hip_clear_row_extension(current_ctx()), "clear_row_extension()");
        }

        namespace detail
        {
            inline auto has_zinger_filter(const paris_hip_ctx* ctx) -> bool
            {
                const auto& s = state().zinger_filters;
                return !s.empty() && s.count(ctx) != 0u;
            }
        }

        // Extension (no reference counterpart): the pixels of this thread's current device's detector carry stationary offsets, which
        // reconstruct to rings. A pre-pass over the scan sums the frames -- ring_profile_begin(), then
        // ring_profile_add() on every frame as paris::weight() would see it after the zinger filter, then ring_profile_finish(), which
        // returns the correction frame c (n_row x n_col floats, rows n_row apart) of the rule in include/paris_hip.h. Until
        // clear_ring_correction(), paris::weight() subtracts the c given to set_ring_correction() from every frame, after the zinger
        // filter and before every weight (paris_hip_ring_correct_rows). The library keeps its own copy of c.
        inline auto ring_profile_begin(std::uint32_t n_row, std::uint32_t n_col) -> void
        {
            detail::runtime_check(paris_hip_ring_profile_begin(current_ctx(), n_row, n_col), "ring_profile_begin()");
        }

        inline auto ring_profile_add(const float* d_p, std::size_t pitch, std::uint32_t n_row, std::uint32_t n_col) -> void
        {
            detail::runtime_check(paris_hip_ring_profile_add_rows(current_ctx(), d_p, pitch, 0u, 1u, n_row, n_col, 0u, n_col), "ring_profile_add()");
        }

        inline auto ring_profile_finish(std::uint32_t half_width, float floor_abs, float limit_abs, float* c, paris_hip_ring_stats* stats = nullptr)
            -> void
        {
            const auto setting = paris_hip_ring_filter{half_width, floor_abs, limit_abs};
            detail::runtime_check(paris_hip_ring_profile_finish(current_ctx(), &setting, c, nullptr, stats), "ring_profile_finish()");
        }

        // Extension (no reference counterpart): the rotation axis, delta_s, found from the scan itself. A
        // pre-pass over a full, equidistant circle of n_frames frames -- axis_search_begin(), then axis_search_add() on every frame
        // as paris::weight() would see it after the zinger filter, each exactly once, then axis_search_finish(), which returns the
        // estimate of the rule in include/paris_hip.h. cost and columns (may be NULL) receive one value per candidate.
        inline auto axis_search_begin(const paris_hip_axis_search& setting, const detector_geometry& det_geo, std::uint32_t n_frames) -> void
        {
            detail::runtime_check(paris_hip_axis_search_begin(current_ctx(), &setting, detail::as_c<paris_detector_geometry>(det_geo), n_frames),
                                  "axis_search_begin()");
        }

        inline auto axis_search_add(const float* d_p, std::size_t pitch, std::uint32_t n_row, std::uint32_t n_col, std::uint32_t frame) -> void
        {
            detail::runtime_check(paris_hip_axis_search_add_rows(current_ctx(), d_p, pitch, 0u, 1u, n_row, n_col, frame), "axis_search_add()");
        }

        inline auto axis_search_finish(double* cost, std::uint32_t* columns = nullptr) -> paris_hip_axis_result
        {
            auto result = paris_hip_axis_result{};
            detail::runtime_check(paris_hip_axis_search_finish(current_ctx(), cost, columns, &result, nullptr), "axis_search_finish()");
            return result;
        }

        inline auto set_ring_correction(const float* c, std::uint32_t n_row, std::uint32_t n_col) -> void
        {
            detail::runtime_check(paris_hip_set_ring_correction(current_ctx(), c, n_row, n_col), "set_ring_correction()");
            detail::state().ring_corrections.insert(current_ctx());
        }

        inline auto clear_ring_correction() -> void
        {
            detail::runtime_check(paris_hip_clear_ring_correction(current_ctx()), "clear_ring_correction()");
            detail::state().ring_corrections.erase(current_ctx());
        }

        namespace detail
        {
            inline auto has_ring_correction(const paris_hip_ctx* ctx) -> bool
            {
                const auto& s = state().ring_corrections;
                return !s.empty() && s.count(ctx) != 0u;
            }
        }

        // Extension (no reference counterpart): detector binning. The frames of this thread's current device
        // arrive as n_row x n_col detector counts and are to be reconstructed as bin_x x bin_y bins (each 1, 2, 4 or 8): until
        // clear_binning(), bin_frame() makes every binned pixel the mean of the good ones among its source pixels, between the raw
        // upload and the dark / flat correction. mask: n_col rows of n_row bytes, nonzero = bad, or nullptr; the library keeps its own
        // copy. The geometry, the references and the defect map of everything downstream are the binned ones (binned_geometry(),
        // paris_hip_bin_frame_host, paris_hip_bin_mask).
        inline auto set_binning(std::uint32_t bin_x, std::uint32_t bin_y, const std::uint8_t* mask, std::uint32_t n_row, std::uint32_t n_col) -> void
        {
            const auto setting = paris_hip_binning{bin_x, bin_y};
            detail::runtime_check(paris_hip_set_binning(current_ctx(), &setting, mask, n_row, n_col), "set_binning()");
        }

        inline auto clear_binning() -> void
        {
            detail::runtime_check(paris_hip_clear_binning(current_ctx()), "clear_binning()");
        }

        inline auto binned_geometry(std::uint32_t bin_x, std::uint32_t bin_y, const detector_geometry& det_geo) -> detector_geometry
        {
            const auto setting = paris_hip_binning{bin_x, bin_y};
            auto out = detector_geometry{};
            detail::construction_check(paris_hip_binned_geometry(&setting, &det_geo, &out), "binned_geometry()");
            return out;
        }

        // one whole n_row x n_col source frame at d_src into the binned frame at d_dst, all its binned_n_col rows
        inline auto bin_frame(const float* d_src, std::size_t src_pitch, float* d_dst, std::size_t dst_pitch, std::uint32_t n_row, std::uint32_t n_col,
                              std::uint32_t binned_n_col) -> void
        {
            detail::runtime_check(paris_hip_bin_frames(current_ctx(), d_src, src_pitch, 0u, d_dst, dst_pitch, 0u, 1u, n_row, n_col, 0u, binned_n_col),
                                  "bin_frame()");
        }

        // Extension (no reference counterpart): the detector of this thread's current device carries part of every frame's signal
        // over into the following frames (lag). b and a hold `terms` weights and decay rates per frame of
        // its impulse response (1 .. 4 terms), start is PARIS_HIP_LAG_START_STEADY or _REST. The pass carries state from frame to
        // frame, so a caller that knows where a scan begins drives it itself: lag_begin() for the rows it will upload, then
        // lag_correct() on every frame of counts in time order -- after the raw upload and bin_frame(), before the dark / flat
        // correction -- then lag_end(). PARIS's per-projection stage loop (stages.h) has no notion of where a scan begins and does not
        // apply it.
        inline auto set_lag_correction(const float* b, const float* a, std::uint32_t terms, int start = PARIS_HIP_LAG_START_STEADY) -> void
        {
            auto model = paris_hip_lag_model{};
            model.terms = terms;
            model.start = start;
            for(std::uint32_t n = 0; b != nullptr && a != nullptr && n < terms && n < PARIS_HIP_LAG_TERMS_MAX; ++n)
            {
                model.b[n] = b[n];
                model.a[n] = a[n];
            }
            detail::runtime_check(b == nullptr || a == nullptr ? PARIS_HIP_ERROR_INVALID_ARGUMENT : paris_hip_set_lag_correction(current_ctx(), &model),
                                  "set_lag_correction()");
        }

        inline auto clear_lag_correction() -> void
        {
            detail::runtime_check(paris_hip_clear_lag_correction(current_ctx()), "clear_lag_correction()");
        }

        inline auto lag_begin(std::uint32_t n_row, std::uint32_t n_col, std::uint32_t row_first, std::uint32_t row_count) -> void
        {
            detail::runtime_check(paris_hip_lag_begin(current_ctx(), n_row, n_col, row_first, row_count), "lag_begin()");
        }

        // the begun rows of one n_row x n_col frame of counts at d_p, the next in time
        inline auto lag_correct(float* d_p, std::size_t pitch, std::uint32_t n_row, std::uint32_t n_col, std::uint32_t row_first, std::uint32_t row_count)
            -> void
        {
            detail::runtime_check(paris_hip_lag_correct_rows(current_ctx(), d_p, pitch, 0u, 1u, n_row, n_col, row_first, row_count), "lag_correct()");
        }

        inline auto lag_end() -> void
        {
            detail::runtime_check(paris_hip_lag_end(current_ctx()), "lag_end()");
        }

        // Extension (no reference counterpart): metal artefact reduction by linear interpolation. bits holds
        // the packed traces of all n_views views of the scan on n_row x n_col frames (paris_hip_metal_trace_pack's layout). Until
        // clear_metal_trace(), paris::weight() replaces the trace's pixels of every frame -- the trace of view p.idx -- by linear
        // interpolation along the row, after the detector roll and before the redundancy and cosine weights
        // (paris_hip_metal_inpaint_rows). Off unless called.
        inline auto set_metal_trace(const std::uint64_t* bits, std::uint32_t n_views, std::uint32_t n_row, std::uint32_t n_col) -> void
        {
            detail::runtime_check(paris_hip_set_metal_trace(current_ctx(), bits, n_views, n_row, n_col), "set_metal_trace()");
            detail::state().metal_traces.insert(current_ctx());
        }

        inline auto clear_metal_trace() -> void
        {
            detail::runtime_check(paris_hip_clear_metal_trace(current_ctx()), "clear_metal_trace()");
            detail::state().metal_traces.erase(current_ctx());
        }

        namespace detail
        {
            inline auto has_metal_trace(const paris_hip_ctx* ctx) -> bool
            {
                const auto& s = state().metal_traces;
                return s.find(ctx) != s.end();
            }
        }

        // the rows [row_first, row_first + row_count) of one n_row x n_col frame of line integrals at d_p, with the trace of `view`
        inline auto metal_inpaint(float* d_p, std::size_t pitch, std::uint32_t n_row, std::uint32_t n_col, std::uint32_t row_first, std::uint32_t row_count,
                                  std::uint32_t view) -> void
        {
            detail::runtime_check(paris_hip_metal_inpaint_rows(current_ctx(), d_p, pitch, 0u, 1u, n_row, n_col, row_first, row_count, &view), "metal_inpaint()");
        }

        // the metal voxels of the first reconstruction (paris_hip_metal_collect's list: n strictly ascending indices and their values),
        // which metal_reinsert() puts back into a finished slab: slices [v_offset, v_offset + v_dim_z) of a grid of dim_x x dim_y
        // voxels per slice
        inline auto set_metal_voxels(const std::uint64_t* index, const float* value, std::uint64_t n) -> void
        {
            detail::runtime_check(paris_hip_set_metal_voxels(current_ctx(), index, value, n), "set_metal_voxels()");
        }

        inline auto clear_metal_voxels() -> void
        {
            detail::runtime_check(paris_hip_clear_metal_voxels(current_ctx()), "clear_metal_voxels()");
        }

        inline auto metal_reinsert(float* d_v, std::uint32_t dim_x, std::uint32_t dim_y, std::uint32_t v_dim_z, std::uint32_t v_offset) -> void
        {
            detail::runtime_check(paris_hip_metal_reinsert(current_ctx(), d_v, dim_x, dim_y, v_dim_z, v_offset), "metal_reinsert()");
        }

        // the edge-preserving 3-D bilateral filter: slices [z_first, z_first + z_count) of the device buffer
        // d_src (dim_x x dim_y x src_dim_z voxels) filtered into z_count slices at d_dst, which must not overlap it, on the calling
        // thread's current device; sigma_r in the volume's units, sigma_s in voxels, radius 1 .. 3. A z tap outside the buffer is
        // skipped: a slab of a larger grid is passed with its halo slices and without them in the range
        inline auto volume_bilateral(const float* d_src, std::uint32_t dim_x, std::uint32_t dim_y, std::uint32_t src_dim_z, std::uint32_t z_first,
                                     std::uint32_t z_count, float sigma_r, float sigma_s, std::uint32_t radius, float* d_dst) -> void
        {
            const struct paris_hip_volume_bilateral setting{sigma_r, sigma_s, radius};
            detail::runtime_check(paris_hip_volume_bilateral(current_ctx(), d_src, dim_x, dim_y, src_dim_z, z_first, z_count, &setting, d_dst),
                                  "volume_bilateral()");
        }

        // ---- buffers ------------------------------------------------------------------------------------------
        struct device_free { void operator()(float* p) const noexcept { paris_hip_free(current_ctx(), p); } };
        struct host_free { void operator()(float* p) const noexcept { paris_hip_free_host(current_ctx(), p); } };

        // device projection buffer with a row pitch in bytes, like cuda::pitched_device_ptr
        class pitched_buffer
        {
        public:
            pitched_buffer() noexcept = default;
            pitched_buffer(float* p, std::size_t pitch_bytes) noexcept : ptr_{p}, pitch_{pitch_bytes} {}
            auto get() const noexcept -> float* { return ptr_.get(); }
            auto pitch() const noexcept -> std::size_t { return pitch_; }
            explicit operator bool() const noexcept { return static_cast<bool>(ptr_); }
        private:
            std::unique_ptr<float, device_free> ptr_{};
            std::size_t pitch_ = 0;
        };

        using projection_host_buffer_type = std::unique_ptr<float, host_free>;
        using projection_device_buffer_type = pitched_buffer;
        using volume_host_buffer_type = std::unique_ptr<float, host_free>;
        using volume_device_buffer_type = std::unique_ptr<float, device_free>;
        using filter_buffer_type = std::unique_ptr<float, device_free>;

        struct metadata {};

        using projection_host_type = projection<projection_host_buffer_type, metadata>;
        using projection_device_type = projection<projection_device_buffer_type, metadata>;
        using volume_host_type = volume<volume_host_buffer_type>;
        using volume_device_type = volume<volume_device_buffer_type>;

        // ---- memory (src/cuda/memory.cpp:33-102) ------------------------------------------------------------------
        inline auto make_projection_host(std::uint32_t dim_x, std::uint32_t dim_y) -> projection_host_type
        {
            void* p = nullptr;
            detail::construction_check(paris_hip_malloc_host(current_ctx(), std::size_t{dim_x} * dim_y * sizeof(float), &p),
                                       "make_projection_host()");
            return {projection_host_buffer_type{static_cast<float*>(p)}, dim_x, dim_y, 0, 0.f, metadata{}};
        }

        inline auto make_projection_device(std::uint32_t dim_x, std::uint32_t dim_y) -> projection_device_type
        {
            float* p = nullptr;
            std::size_t pitch = 0;
            detail::construction_check(paris_hip_malloc_projection(current_ctx(), dim_x, dim_y, &p, &pitch),
                                       "make_projection_device()");
            return {pitched_buffer{p, pitch}, dim_x, dim_y, 0, 0.f, metadata{}};
        }

        inline auto make_volume_host(std::uint32_t dim_x, std::uint32_t dim_y, std::uint32_t dim_z) -> volume_host_type
        {
            const auto n = std::size_t{dim_x} * dim_y * dim_z;
            void* p = nullptr;
            detail::construction_check(paris_hip_malloc_host(current_ctx(), n * sizeof(float), &p), "make_volume_host()");
            auto f = static_cast<float*>(p);
            for(std::size_t i = 0; i < n; ++i)
                f[i] = 0.f; // zero-filled like src/openmp/memory.cpp:46-47
            return {volume_host_buffer_type{f}, dim_x, dim_y, dim_z, 0};
        }

        inline auto make_volume_device(std::uint32_t dim_x, std::uint32_t dim_y, std::uint32_t dim_z) -> volume_device_type
        {
            float* p = nullptr;
            detail::construction_check(paris_hip_malloc_volume(current_ctx(), dim_x, dim_y, dim_z, &p), "make_volume_device()");
            return {volume_device_buffer_type{p}, dim_x, dim_y, dim_z, 0};
        }

        inline auto copy_h2d(const projection_host_type& h_p, projection_device_type& d_p) -> void
        {
            // on the upload stream when the loop's own kernels share the compute stream: the transfer does not wait behind them, and
            // the pinned source is released when this copy is done (the compute stream is ordered behind the copy by the library);
            // on the compute stream when nothing else is enqueued there (PARIS_HIP_UPLOAD_ON_ITS_OWN_STREAM above)
            detail::runtime_check((PARIS_HIP_UPLOAD_ON_ITS_OWN_STREAM && !PARIS_HIP_SYNCHRONOUS_CALLS ? paris_hip_upload_projection : paris_hip_memcpy_projection_h2d)(
                                      current_ctx(), d_p.buf.get(), d_p.buf.pitch(), h_p.buf.get(), std::size_t{h_p.dim_x} * sizeof(float), h_p.dim_x, h_p.dim_y),
                                  "copy_h2d(projection)");
            d_p.idx = h_p.idx; // src/openmp/memory.cpp:60-62
            d_p.phi = h_p.phi;
            d_p.meta = h_p.meta;
        }

        inline auto copy_d2h(const projection_device_type& d_p, projection_host_type& h_p) -> void
        {
            detail::runtime_check(paris_hip_memcpy_projection_d2h(current_ctx(), h_p.buf.get(), std::size_t{h_p.dim_x} * sizeof(float),
                                                                  d_p.buf.get(), d_p.buf.pitch(), d_p.dim_x, d_p.dim_y),
                                  "copy_d2h(projection)");
            detail::runtime_check(paris_hip_ctx_synchronize(current_ctx()), "copy_d2h(projection)"); // the host reads h_p next
            h_p.idx = d_p.idx;
            h_p.phi = d_p.phi;
            h_p.meta = d_p.meta;
        }

        inline auto copy_h2d(const volume_host_type& h_v, volume_device_type& d_v) -> void
        {
            detail::runtime_check(paris_hip_memcpy_volume_h2d(current_ctx(), d_v.buf.get(), h_v.buf.get(), h_v.dim_x, h_v.dim_y, h_v.dim_z),
                                  "copy_h2d(volume)");
            d_v.off = h_v.off; // src/openmp/memory.cpp:73
        }

        inline auto copy_d2h(const volume_device_type& d_v, volume_host_type& h_v) -> void
        {
            detail::runtime_check(paris_hip_memcpy_volume_d2h(current_ctx(), h_v.buf.get(), d_v.buf.get(), d_v.dim_x, d_v.dim_y, d_v.dim_z),
                                  "copy_d2h(volume)");
            detail::runtime_check(paris_hip_ctx_synchronize(current_ctx()), "copy_d2h(volume)"); // the host reads h_v next
            h_v.off = d_v.off;
        }

        // Extension (no reference counterpart): runs what is deferred and waits for everything enqueued on this thread's device.
        inline auto synchronize() -> void
        {
            detail::runtime_check(paris_hip_ctx_synchronize(current_ctx()), "synchronize()");
        }

        // ---- subvolume planning (src/cuda/subvolume_information.cpp:63-118) ---------------------------------------
        inline auto make_subvolume_information(const volume_geometry& vol_geo, const detector_geometry& det_geo) -> subvolume_info
        {
            paris_subvolume_info c_info{};
            // beside the slab a device also holds this backend's projection buffers: the rotation of make_projection_device buffers
            // and the pending group (or the snapshot ring) -- they do not shrink when the slab count doubles
            std::size_t reserve = 0;
            detail::construction_check(paris_hip_projection_reserve_bytes(current_ctx(), det_geo.n_row, det_geo.n_col, &reserve),
                                       "make_subvolume_information()");
            detail::construction_check(paris_hip_make_subvolume_information_reserving(detail::as_c<paris_volume_geometry>(vol_geo),
                                                                                      detail::as_c<paris_detector_geometry>(det_geo), 0, reserve, &c_info),
                                       "make_subvolume_information()");
            subvolume_info info{};
            info.geo.dim_x = c_info.geo.dim_x;
            info.geo.dim_y = c_info.geo.dim_y;
            info.geo.dim_z = c_info.geo.dim_z;
            info.geo.remainder = c_info.geo.remainder;
            info.num = c_info.num;
            return info;
        }

        // ---- the numeric stages ---------------------------------------------------------------------------------------
        inline auto weight(projection_device_type& p, float h_min, float v_min, float d_sd, float l_px_row, float l_px_col) -> void
        {
            detail::runtime_check(paris_hip_weight(current_ctx(), p.buf.get(), p.buf.pitch(), p.dim_x, p.dim_y, h_min, v_min, d_sd,
                                                   l_px_row, l_px_col), "weight()");
        }

        inline auto make_filter(std::uint32_t size, float tau) -> filter_buffer_type
        {
            float* k = nullptr;
            detail::construction_check(paris_hip_make_filter(current_ctx(), size, tau, &k), "make_filter()");
            return filter_buffer_type{k};
        }

        inline auto apply_filter(projection_device_type& p, const filter_buffer_type& k, std::uint32_t filter_size,
                                 std::uint32_t n_col) -> void
        {
            detail::runtime_check(paris_hip_apply_filter(current_ctx(), p.buf.get(), p.buf.pitch(), p.dim_x, p.dim_y, k.get(),
                                                         filter_size, n_col), "apply_filter()");
        }

        inline auto backproject(const projection_device_type& p, volume_device_type& v, std::uint32_t v_offset,
                                const detector_geometry& det_geo, const volume_geometry& vol_geo, bool enable_roi,
                                const region_of_interest& roi, float sin, float cos, float delta_s, float delta_t) -> void
        {
            detail::runtime_check(paris_hip_backproject(current_ctx(), p.buf.get(), p.buf.pitch(), p.dim_x, p.dim_y, v.buf.get(),
                                                        v.dim_x, v.dim_y, v.dim_z, v_offset, detail::as_c<paris_detector_geometry>(det_geo),
                                                        detail::as_c<paris_volume_geometry>(vol_geo), enable_roi ? 1 : 0,
                                                        detail::as_c<paris_region_of_interest>(roi), sin, cos, delta_s, delta_t),
                                  "backproject()");
        }

        // Extension (no reference counterpart): the cone-beam projections of the slab v (first slice: global slice v_offset of the
        // grid vol_geo) by Joseph's method, in backproject()'s geometry and with its arguments (paris_hip_forward_project). One view
        // into p, or -- accumulate -- added to what p holds: the projections of disjoint slabs add up to the whole volume's.
        inline auto forward_project(const volume_device_type& v, std::uint32_t v_offset, const detector_geometry& det_geo,
                                    const volume_geometry& vol_geo, projection_device_type& p, float sin, float cos, float delta_s,
                                    float delta_t, bool accumulate = false) -> void
        {
            detail::runtime_check(paris_hip_forward_project(current_ctx(), v.buf.get(), v.dim_x, v.dim_y, v.dim_z, v_offset,
                                                            detail::as_c<paris_detector_geometry>(det_geo),
                                                            detail::as_c<paris_volume_geometry>(vol_geo), p.buf.get(), p.buf.pitch(), 0u, 1u,
                                                            p.dim_x, p.dim_y, &sin, &cos, delta_s, delta_t, accumulate ? 1 : 0),
                                  "forward_project()");
        }
    }
}

#endif
