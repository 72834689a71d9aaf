// Internal declarations shared by the translation units of libparis_hip.so (gfx950 only).
#ifndef PARIS_HIP_INTERNAL_H_
#define PARIS_HIP_INTERNAL_H_

#include <hip/hip_runtime.h>

#include <cstddef>
#include <array>
#include <cstdint>
#include <initializer_list>
#include <map>
#include <vector>

#include "paris_hip.h"

// Every fp32 operation of the numeric path must round once, in the reference's order (DESIGN.md,
// "Numerics"): no FMA contraction anywhere in this library. The Makefile passes -ffp-contract=off as well.
#pragma clang fp contract(off)

#define PARIS_HIP_TRY(expr)                                   \
    do                                                        \
    {                                                         \
        hipError_t paris_hip_err__ = (expr);                  \
        if(paris_hip_err__ != hipSuccess)                     \
            return static_cast<int>(paris_hip_err__);         \
    } while(0)

struct paris_hip_fft_plan
{
    float2* d_twiddle = nullptr; // exp(-2 pi i k / n), k < n/2
    // fused weight + filter kernel (filter_fused.hip), n >= 1024: inter-pass twiddle tables W_B^(o q), rounded from double
    float2* d_tab_first = nullptr;                  // first / last pass, B = n
    float2* d_tab_mid[3] = {nullptr, nullptr, nullptr}; // middle passes with B = 256, 4096, 65536
};

// a filter K made by paris_hip_make_filter*: its length and the copy of K in the order the fused kernel's middle pass reads it
struct paris_hip_filter_info
{
    uint32_t size = 0;
    float* d_kp = nullptr;
    float tau = 0.f; // the pixel pitch K was made for (the row extension's response needs it)
};

// device memory a ctx setting owns: `bytes` is what paris_hip_projection_reserve_bytes counts for it
struct paris_hip_device_buffer
{
    void* d = nullptr;
    size_t bytes = 0;
    template <class T>
    T* as() const
    {
        return static_cast<T*>(d);
    }
};

// what paris_hip_ctx::volume_window_t::mem occupies: 32 bytes of quantise counters, 32 bytes of stats results, the 64-bit bins
constexpr size_t PARIS_HIP_VOLUME_WINDOW_ACC_BYTES = 64u + 8u * PARIS_HIP_VOLUME_HISTOGRAM_BINS_MAX;

struct paris_hip_ctx
{
    int device = 0;
    hipStream_t stream = nullptr;
    bool owns_stream = false;
    unsigned flags = 0;
    // ring of HIP event pairs recorded on the ctx stream around backprojection launches (bench.py's
    // roofline figure); capacity 1 by default, i.e. "the last launch"
    std::vector<hipEvent_t> bp_start, bp_stop;
    uint64_t bp_launches = 0; // launches recorded since the ring was (re)armed
    int bp_variant = 0;
    int bp_vx = 0, bp_unroll = 0; // 0 = automatic
    uint32_t bp_tz = 0, bp_lds_bytes = 0;
    int bp_order = -1; // -1 = default mapping
    int bp_slice_nw = 0, bp_slice_rpl = 0; // slice kernel shape, 0 = default
    int bp_nt = -1;    // volume stream policy: -1 automatic by slab size, 0 plain, 1 nontemporal, 2 nontemporal + write-through stores
    int bp_stage_vec4 = 1; // stage the detector box 4 pixels per lane when the projection's alignment allows
    int bp_fastdiv = 1; // use the validated multiply+2 FMA division by the pixel pitch when it is exact
    int bp_skip_invalid = 1; // waves none of whose columns a projection's rays reach leave their tile untouched (clean volumes only)
    // Volumes known to hold no -0: allocated (zero-filled) or zero-filled again by this library and written by nothing but
    // backprojections since (base address -> bytes). A host upload into one removes it; memory the library did not allocate is
    // never listed.
    std::map<uintptr_t, size_t> clean_volumes;
    // every volume paris_hip_malloc_volume handed out and paris_hip_free has not taken back (base address -> bytes): the only
    // memory paris_hip_ctx_destroy will run still-deferred projections into (a foreign address may have changed hands)
    std::map<uintptr_t, size_t> volume_allocs;
    int bp_lean_div = 1; // share one reciprocal between the two per-column divisions by s + d_so when the operands are in range
    std::map<uint32_t, bool> fastdiv_exact; // divisor bits -> exhaustive check result
    std::map<std::array<uint32_t, 4>, bool> lean_checks; // (kind, operand bits...) -> device validation result (validate.hip)
    int lean_validate = 1; // 0: trust the range tests alone (A/B and tests of the validators themselves)
    bool filter_lds_attr_set = false;
    bool filter_r16_attr_set[5] = {false, false, false, false, false}; // LOG2N 10..14
    int filter_variant = 0; // 0: radix-16 register passes for N >= 1024, 1: radix-2 kernel for every N
    std::map<uint32_t, paris_hip_fft_plan> plans; // keyed by FFT length
    std::map<const float*, paris_hip_filter_info> filters; // K buffers handed out by paris_hip_make_filter*, until paris_hip_free
    // Stage fusion (paris_hip_set_stage_fusion): a paris_hip_weight[_rows] call is held back; the paris_hip_apply_filter call
    // that follows on the same rows runs ONE kernel that weights in its load (filter_fused.hip). Anything else that touches a
    // projection or completes work first runs the held-back weighting as its own kernel (paris_hip_flush_pending_weight).
    int stage_fusion = 0;
    struct pending_weight_t
    {
        bool active = false;
        float* d_p = nullptr;
        size_t pitch = 0;
        uint32_t dim_x = 0, dim_y = 0, row_first = 0, row_count = 0;
        float h_min = 0.f, v_min = 0.f, d_sd = 0.f, l_px_row = 0.f, l_px_col = 0.f;
        // filter deferral (below): the row filter that followed on the same rows is held back too
        bool filter = false;
        const float* d_kp = nullptr;
        const paris_hip_fft_plan* plan = nullptr;
        uint32_t filter_size = 0;
    } pending_weight;
    // Filter deferral (paris_hip_set_filter_deferral; needs stage fusion and a backprojection deferral depth > 1): the
    // paris_hip_apply_filter call that would run the one weight + filter launch is held back as well. If the next call backprojects
    // those rows' projection, the UNFILTERED frame is snapshotted into the deferral ring and weighting + filter run on the ring, one
    // launch for the whole group, right before the fused backprojection; any other call runs the held-back launch first, in place.
    int filter_deferral = 0;
    std::vector<pending_weight_t> defer_wf; // per ring slot of the current group: the weight + filter it still needs
    // dedicated upload stream + ring of events ordering the compute stream behind each upload (paris_hip_upload_projection)
    hipStream_t upload_stream = nullptr;
    std::vector<hipEvent_t> upload_events;
    uint64_t uploads = 0;
    // device buffers that have been the destination of paris_hip_upload_projection: the event marks the last library call
    // enqueued on the compute stream that reads or writes the buffer, so the next upload into it (slot reuse) waits for
    // exactly that work and nothing else. Buffers never uploaded into this way are not tracked (no cost for other callers).
    struct upload_target
    {
        hipEvent_t last_use = nullptr;
        bool used = false;
        size_t bytes = 0; // extent of the buffer as uploaded (pitch x rows): stage calls on a row band pass interior pointers
    };
    std::map<const void*, upload_target> upload_targets;
    // Settings that own device memory (DESIGN.md section 1.1 gives the one rule they all follow). Each keeps its memory in a
    // paris_hip_device_buffer `mem`; what is said below is what is particular to the setting.
    // Dark / flat correction (paris_hip_set_flat_field): the dark frame, the flat right behind it (each dim_x x dim_y, rows dim_x
    // floats apart).
    struct flat_field_t
    {
        paris_hip_device_buffer mem;
        uint32_t dim_x = 0, dim_y = 0;
        double t_min = 1.0;
        std::vector<uint8_t> dead; // host: 1 where D or F is not finite or F - D <= 0 (paris_hip_flat_field_dead_pixels)
    } flat_field;
    // Defect map (paris_hip_set_defect_map): the plan of defect_plan.cpp -- defect[n], first_source[n + 1], source[m], weight[m], 4
    // bytes each. A plan without a repairable defect has no buffer (mem.d == nullptr while set).
    struct defect_map_t
    {
        bool set = false;
        paris_hip_device_buffer mem;
        uint32_t dim_x = 0, dim_y = 0;
        uint32_t n = 0, m = 0; // repairable defects, sources
        paris_hip_defect_stats stats{};
        std::vector<uint32_t> row_start; // host, dim_y + 1: the sorted defect list's range per detector row
    } defect_map;
    // Zinger filter (paris_hip_set_zinger_filter): the rule with max_hits resolved; three 64-bit accumulators (padded to 32 bytes),
    // `frames` x max_hits (index, value) pairs, `frames` hit counters.
    struct zinger_t
    {
        bool set = false;
        paris_hip_zinger_filter rule{};
        uint32_t dim_x = 0, dim_y = 0;
        uint32_t frames = 0; // frames one launch serves
        paris_hip_device_buffer mem;
    } zinger;
    // Ring filter. The open profile (paris_hip_ring_profile_begin): the double sums, rows dim_x doubles
    // apart (the copy of finish reads them too, on the compute stream), and on the host how many frames each row has received.
    struct ring_profile_t
    {
        paris_hip_device_buffer mem;
        uint32_t dim_x = 0, dim_y = 0;
        std::vector<uint32_t> count;
    } ring_profile;
    // The correction frame (paris_hip_set_ring_correction): rows dim_x floats apart; `zero`: it holds no pixel to correct,
    // paris_hip_ring_correct_rows is idle.
    struct ring_correction_t
    {
        bool set = false, zero = false;
        paris_hip_device_buffer mem;
        uint32_t dim_x = 0, dim_y = 0;
    } ring_correction;
    // Axis search (paris_hip_axis_search_begin): in this order the sinogram (n_frames rows of n floats), the
    // plan (count rows of n 16-byte entries), the score kernel's partial sums and the per-candidate totals (paris_hip_axis_layout);
    // finish copies from it on the compute stream. On the host: which sinogram rows have been added and every candidate's valid columns.
    struct axis_t
    {
        paris_hip_device_buffer mem;
        paris_hip_axis_search setting{};
        uint32_t n = 0, n_col = 0, n_frames = 0, row_first = 0, missing = 0;
        std::vector<uint8_t> seen;
        std::vector<uint32_t> columns;
    } axis;
    // Detector binning (paris_hip_set_binning): the setting for one source detector, the binned size, and the
    // optional source-size mask (mem.d == nullptr: every pixel good).
    struct binning_t
    {
        bool set = false;
        paris_hip_binning rule{};
        paris_hip_device_buffer mem;
        uint32_t dim_x = 0, dim_y = 0, out_x = 0, out_y = 0;
    } binning;
    // Air region (paris_hip_set_air_region): the rule with min_pixels resolved; the buffer is laid out by
    // paris_hip_air_layout_of -- the counters, the values and counts of one launch, the rectangle's mask bytes (measure and stats copy
    // from it on the compute stream).
    struct air_t
    {
        bool set = false;
        paris_hip_air_region rule{};
        uint32_t dim_x = 0, dim_y = 0;
        paris_hip_device_buffer mem;
    } air;
    // Beam hardening (paris_hip_set_beam_hardening): the setting and the frame size it was made for. It
    // travels to the kernel by value: nothing on the device, nothing to retire.
    struct beam_hardening_t
    {
        bool set = false;
        paris_hip_beam_hardening rule{};
        uint32_t dim_x = 0, dim_y = 0;
    } beam_hardening;
    // Detector roll (paris_hip_set_detector_roll): the setting and the geometry it was made for. The six
    // constants are made per call and travel to the kernel by value: nothing on the device, nothing to retire.
    struct detector_roll_t
    {
        bool set = false;
        paris_hip_detector_roll rule{};
        paris_detector_geometry geo{};
    } detector_roll;
    // Detector lag (paris_hip_set_lag_correction): the model and the coefficients made from it, which travel
    // to the kernel by value. `seq` is the open sequence (paris_hip_lag_begin), which ends without the model: the band it was begun
    // for, how many frames it has seen, and the band's state -- model.terms planes of row_count x dim_x floats, zeroed on the compute
    // stream.
    struct lag_t
    {
        bool set = false;
        paris_hip_lag_model model{};
        float g[PARIS_HIP_LAG_TERMS_MAX] = {0.f, 0.f, 0.f, 0.f}, c[PARIS_HIP_LAG_TERMS_MAX] = {0.f, 0.f, 0.f, 0.f},
              w[PARIS_HIP_LAG_TERMS_MAX] = {0.f, 0.f, 0.f, 0.f}, inv_b = 0.f;
        struct sequence_t
        {
            paris_hip_device_buffer mem; // mem.d != nullptr: a sequence is open
            uint32_t dim_x = 0, dim_y = 0, row_first = 0, row_count = 0;
            uint64_t frames = 0;
        } seq;
    } lag;
    // Metal trace (paris_hip_set_metal_trace): PARIS_HIP_METAL_COUNTER_BYTES of counters -- replaced, runs,
    // rows_left, 64-bit each, zeroed at install --, then the packed traces of all views.
    struct metal_trace_t
    {
        bool set = false;
        paris_hip_device_buffer mem;
        uint32_t n_views = 0, dim_x = 0, dim_y = 0, words = 0;
    } metal_trace;
    // Metal voxels (paris_hip_set_metal_voxels): n 64-bit indices, ascending, then their n values; the indices on the host as well,
    // for the bisection per slab. An empty list has no buffer (mem.d == nullptr while set).
    struct metal_voxels_t
    {
        bool set = false;
        paris_hip_device_buffer mem;
        std::vector<uint64_t> index;
    } metal_voxels;
    // Phase retrieval (paris_hip_set_phase_retrieval): in this order the twiddles of N_x (N_x / 2 complex
    // floats) and of N_y, the tables a_x (N_x floats) and a_y, and the scratch -- `frames` frames of dim_y x (N_x / 2 + 1) complex floats.
    struct phase_t
    {
        bool set = false;
        paris_hip_phase_retrieval rule{};
        paris_hip_device_buffer mem;
        uint32_t dim_x = 0, dim_y = 0, n_x = 0, n_y = 0;
        uint32_t frames = 0; // frames one round of launches serves
    } phase;
    // Scatter correction (paris_hip_set_scatter_correction): in this order the twiddles of N_x and of N_y, the
    // tables g1x, g2x (N_x floats each), g1y, g2y, and the scratch -- `frames` frames of dim_y x (N_x / 2 + 1) complex floats.
    struct scatter_t
    {
        bool set = false;
        paris_hip_scatter_correction rule{};
        paris_hip_device_buffer mem;
        uint32_t dim_x = 0, dim_y = 0, n_x = 0, n_y = 0;
        uint32_t frames = 0; // frames one round of launches serves
    } scatter;
    // Row extension (paris_hip_set_row_extension): the rule, and the responses c made so far, one buffer per (dim_x, tau bits, W) --
    // the second stream reads them too, behind a join.
    struct row_extension_t
    {
        bool set = false;
        paris_hip_row_extension rule{};
        std::map<std::array<uint32_t, 3>, paris_hip_device_buffer> cache;
    } row_extension;
    // Volume export (volume_window.hip), both made on first use. mem: the three 64-bit counters of the
    // quantise calls (padded to 32 bytes), then the stats kernel's results -- two 32-bit extremes, three 64-bit counters (32 bytes) --
    // and its PARIS_HIP_VOLUME_HISTOGRAM_BINS_MAX 64-bit bins; zeroed on the compute stream. stage: where
    // paris_hip_volume_quantize_d2h quantises to before its copy to the host; grows on demand, the outgrown one is retired. `voxels`
    // is kept here: it is the sum of the calls' n_voxels.
    struct volume_window_t
    {
        paris_hip_device_buffer mem, stage;
        uint64_t voxels = 0;
    } volume_window;
    // Volume denoising (paris_hip_volume_bilateral), made at the first call with a setting and replaced when a
    // call brings another: the PARIS_HIP_BILATERAL_BINS floats of the range table, then the (2r + 1)^3 of the spatial table.
    struct volume_bilateral_t
    {
        bool set = false;
        struct paris_hip_volume_bilateral rule{};
        float rscale = 0.f;
        paris_hip_device_buffer mem;
    } volume_bilateral;
    // Starvation filter (paris_hip_set_starvation_filter): in this order three 64-bit counters (frames,
    // filtered, last_level; padded to 32 bytes, zeroed at install), the table g -- PARIS_HIP_STARVATION_LEVELS rows of radius + 1 floats,
    // in room for the largest radius --, and the scratch of PARIS_HIP_STARVATION_FRAMES_MAX dense frames of dim_x x dim_y floats.
    struct starvation_t
    {
        bool set = false;
        paris_hip_starvation_filter rule{};
        uint32_t dim_x = 0, dim_y = 0;
        paris_hip_device_buffer mem;
    } starvation;
    // every setting above that owns device memory: what paris_hip_ctx_destroy releases and paris_hip_projection_reserve_bytes counts
    template <class F>
    void each_setting(F&& f)
    {
        f(flat_field), f(defect_map), f(zinger), f(ring_profile), f(ring_correction), f(axis), f(binning), f(air), f(lag.seq);
        f(row_extension), f(volume_window), f(metal_trace), f(metal_voxels), f(phase), f(scatter), f(volume_bilateral), f(starvation);
    }
    // Buffers of replaced or cleared settings (paris_hip_retire_device_buffer): each behind an event recorded on the compute stream, freed
    // once that event has completed -- at a later set / clear, or at destroy.
    std::vector<std::pair<void*, hipEvent_t>> retired;
    // K cached by paris_hip_stage_filter (reference: thread_local static in src/filtering.cpp:42)
    float* stage_k = nullptr;
    uint32_t stage_k_size = 0;
    float stage_k_tau = 0.f;
    int stage_window = 0, stage_k_window = 0; // requested window / window of the cached K
    // Projection-sized buffers are recycled instead of returned to the runtime (the reference's CUDA backend pools its device
    // projection buffers too, src/cuda/memory.cpp:42-44): PARIS allocates and frees one host and one device buffer per
    // projection (src/loader.cpp:28-33), and hipMalloc / hipFree / hipHostMalloc cost more than the kernels of a small frame.
    // A released buffer carries an event recorded behind its LAST USER, on the stream that ran it: for a pinned host buffer the
    // H2D copy that read it (the upload stream when the frame went through paris_hip_upload_projection -- nothing queued on the
    // compute stream holds it back), for a device buffer the compute stream at release time (its last reader -- the filter, the
    // deferral ring's snapshot copy -- was enqueued there just before). A buffer nothing used is free at once (no event). It is
    // handed out again only after that event has completed, so the new owner may touch it from the host or from any stream. While
    // the oldest released buffer is still busy and fewer than pool_capacity(bytes) are parked, a fresh one is allocated instead of
    // waiting: an asynchronous caller ends up rotating through a few buffers and never stalls.
    struct pooled_buffer
    {
        void* ptr;
        hipEvent_t released; // nullptr: free at once
        uint64_t group = 0;  // the fused launch (group_seq) that reads it last, by reference (0: none): free once that group is done
    };
    struct proj_alloc
    {
        size_t bytes = 0;
        bool touched = false; // a library call has read or written it since it was handed out
        uint32_t held = 0;    // slots of the PENDING deferred group that refer to this buffer itself (no snapshot was taken)
        uint64_t group = 0;   // the last LAUNCHED group that reads it by reference
    };
    struct host_alloc
    {
        size_t bytes = 0;
        unsigned used = 0; // streams with copies from / into it since it was handed out (USED_*)
    };
    static constexpr unsigned USED_COMPUTE = 1u, USED_UPLOAD = 2u;
    std::map<void*, proj_alloc> proj_allocs;           // live buffers of paris_hip_malloc_projection
    std::multimap<size_t, pooled_buffer> proj_pool;    // released ones, by size, oldest first (at most pool_capacity(size) per size)
    std::map<void*, host_alloc> host_allocs;           // live pinned buffers of paris_hip_malloc_host up to POOL_HOST_BYTES
    std::multimap<size_t, pooled_buffer> host_pool;
    static constexpr size_t POOL_HOST_BYTES = size_t{64} << 20; // a 4096 x 4096 frame
    // How far the host may run ahead of the device in PINNED buffers of one size: 8 at least, up to 64 MiB worth, 16 at most (a caller
    // that allocates and frees a buffer per projection blocks in paris_hip_malloc_host once that many are parked and busy). A pinned
    // buffer is busy only until its own H2D copy is done, so a few suffice, and pinning costs ~0.25 ms per MiB (64 buffers of a
    // 1024^2 frame: 60 ms of a 500 ms job, measured).
    static constexpr size_t pool_capacity(size_t bytes)
    {
        const size_t by_bytes = bytes ? (size_t{64} << 20) / bytes : 16u;
        return by_bytes < 8u ? 8u : (by_bytes > 16u ? 16u : by_bytes);
    }
    // DEVICE projection buffers stay busy until the compute stream has run their filter and snapshot -- beside a running fused
    // launch that takes milliseconds per frame (the filter's waves do not fit next to the fused kernel's) -- so the rotation holds
    // a whole group of deferred projections and a few more, as far as 2 GiB go: a host that supplies frames faster than that trickle
    // keeps filling while the launch runs, and the backlog drains in a millisecond once the launch ends (2048^2 frames into a
    // 256-slice slab, filter in place: the loop waited 0.38 ms per frame on its 8 buffers). Device allocations cost ~0.1 ms each.
    // Deferral by reference (defer_refs): the pending group's buffers are not in the pool at all, the group in flight and the one
    // queued behind it are parked and busy -- two groups and a few more, as far as 4 GiB go.
    size_t device_pool_capacity(size_t bytes) const
    {
        const size_t want = (defer_refs != 0 && defer_depth > 1u) ? 2u * defer_depth + 8u : 56u;
        const size_t by_bytes = bytes ? (size_t{defer_refs != 0 ? 4u : 2u} << 30) / bytes : want;
        return by_bytes < 8u ? 8u : (by_bytes > want ? want : by_bytes);
    }
    // what the pools of ALL sizes may keep parked per ctx. Beyond it idle buffers (their last user has finished) are
    // returned to the runtime, other sizes than the one being parked first; on hipErrorOutOfMemory every pool is drained and the
    // allocation tried once more (paris_hip_drain_device_pool).
    static constexpr size_t PARKED_DEVICE_LIMIT = size_t{6} << 30;
    size_t parked_device_bytes = 0;
    // validators (backproject.hip: fast division; validate.hip) never run on the caller's stream -- it may be capturing, or hold
    // queued work the caller does not want to wait for -- but on a small stream of the ctx's own (round 4 borrowed the upload
    // stream: a check could then wait behind uploads that wait for a fused launch), with 8-byte mismatch counters;
    // made on first use (or by PARIS_HIP_CTX_WARM) and kept: creating and destroying a stream per check cost more than the checks
    hipStream_t aux_stream = nullptr;
    unsigned long long* aux_counter = nullptr; // AUX_SLOTS mismatch counters on the device (slot 0: the blocking checks)
    unsigned long long* aux_result = nullptr;  // their values read back, pinned host memory
    static constexpr int AUX_SLOTS = 8;
    // Asynchronous validation (paris_hip_set_async_validation; off in the bare library, on in paris::hip): a validator whose answer
    // is not cached yet is launched and NOT waited for -- the kernels use the compiler's IEEE forms (same bits, a few instructions
    // more per column) until a later call finds the check finished. The first call of a reconstruction no longer blocks for the
    // 2.3 ms exhaustive check of the division by the pixel pitch: for 360 small frames that was a tenth of the whole job.
    int async_validate = 0;
    struct pending_check
    {
        std::array<uint32_t, 4> key;
        int slot;
        hipEvent_t done;
    };
    std::vector<pending_check> pending_checks;
    std::vector<hipEvent_t> spare_events; // timing-disabled events ready for reuse (pool releases, upload targets)
    // deferred backprojection (paris_hip_set_backproject_deferral): projections copied at call time into a device ring and
    // added by one fused launch per `defer_depth` calls; the key_* fields are the arguments the pending calls share
    // Deferral BY REFERENCE (paris_hip_set_backproject_references; off in the bare library, on in paris::hip): a call whose projection
    // is a whole buffer of paris_hip_malloc_projection puts the buffer itself into the group -- no snapshot copy, no ring. The
    // library then owns what happens to that buffer until the group has run: paris_hip_free() of it only marks it (it is parked
    // behind the group's launch, ONE event per group), and any other library call that reads or writes it launches the group first
    // (paris_hip_projection_guard). With filter deferral the held-back weight + filter of such a projection runs IN PLACE, in the
    // group's one filter launch -- the buffer holds what the caller asked for whenever anything looks at it. Work the caller enqueues
    // on the ctx stream by itself is invisible to the library: callers that write a projection buffer with kernels of their own
    // keep the snapshots (the default).
    int defer_refs = 0;
    uint32_t held_count = 0;                              // slots of the pending group that are references
    std::vector<const void*> defer_ptr;                   // per slot of the pending group: where the projection lives
    std::vector<std::pair<void*, size_t>> defer_zombies;  // buffers the caller freed while the pending group refers to them
    bool defer_uses_ring = false;                         // the pending group has snapshot slots in ring half defer_half
    // fused launches in sequence: group g's completion is event group_events[g % GROUP_EVENTS] (recorded behind the launch, on the
    // stream that ran it; launches complete in sequence order -- every launch is ordered behind the one before it). A slot that
    // has been recorded again by a later group answers for the earlier one too.
    static constexpr uint32_t GROUP_EVENTS = 8;
    hipEvent_t group_events[GROUP_EVENTS] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    uint64_t group_seq = 0, group_done_seq = 0;
    uint32_t defer_depth = 1; // 1 = immediate
    uint32_t defer_count = 0; // projections pending in the ring
    // The first groups of a reconstruction are launched early -- after 8, 16, 32 ... calls, until the depth is reached -- so that
    // the device starts on the volume while the caller is still feeding the first full group (48 frames of 2048^2 take a host loop
    // ~60 ms to supply). Reset when a call with other arguments starts a new sequence. Same additions in the same order.
    uint32_t defer_ramp = 8;
    float* defer_ring = nullptr;
    size_t defer_pitch = 0;
    uint32_t defer_dim_x = 0, defer_dim_y = 0, defer_slots = 0;
    bool defer_f16 = false; // the ring holds IEEE half pixels (calls through paris_hip_backproject_f16)
    float* key_v = nullptr;
    bool key_valid = false; // the key_* fields describe the group launched last (or pending): a matching call continues it
    uint32_t key_dims[4] = {0, 0, 0, 0}; // v_dim_x, v_dim_y, v_dim_z, v_offset
    paris_detector_geometry key_det{};
    paris_volume_geometry key_vol{};
    int key_enable_roi = 0;
    paris_region_of_interest key_roi{};
    float key_delta_s = 0.f, key_delta_t = 0.f;
    std::vector<float> defer_sin, defer_cos;
    // The fused launch of a full ring runs on a stream of its own (bp_stream), ordered behind the group's snapshot copies by an
    // event, so that the copies / weightings / filters of the NEXT group, which the caller keeps enqueuing on `stream`, run
    // beside it instead of behind it. Round 3 measured a loss and kept it off -- but its first call of every group still joined
    // the streams, so nothing overlapped; since round 4 a call that continues the reconstruction of the group launched
    // last (key_valid) starts the next group without a join, and PARIS's per-projection loop through paris::hip -- whose uploads,
    // filters, snapshots and buffer releases otherwise queue behind the running launch -- gains 19 ... 100 %
    // (profiles/r04_demo_paris_hip_mirror.txt). Off by default in the bare library, on in paris::hip. The ring has two halves,
    // written alternately; a half is written again only after the launch that read it has finished (bp_half_done). Every entry
    // point that observes a volume or completes work joins: `stream` is made to wait for the last fused launch
    // (paris_hip_flush_deferred); a group that runs on `stream` itself (a single projection, a synchronous ctx) joins first.
    int bp_overlap = 0;               // knob (paris_hip_set_backproject_overlap), off by default; ignored under PARIS_HIP_CTX_SYNCHRONOUS
    hipStream_t bp_stream = nullptr;
    hipEvent_t bp_ring_ready = nullptr;            // recorded on `stream`: the group's snapshots are in the ring
    hipEvent_t bp_half_done[2] = {nullptr, nullptr}; // recorded on bp_stream behind the launch that read ring half h
    bool bp_half_busy[2] = {false, false};         // bp_half_done[h] is pending: wait for it before writing half h again
    bool bp_inflight = false;                      // fused work on bp_stream that `stream` has not been ordered behind yet
    uint32_t bp_last_half = 0;
    uint32_t defer_half = 0;                       // ring half the pending group is being written to
    // two-pass backprojection (variant 5): factor / h / u planes of the slab's (x, y) plane, rewritten per projection
    float* colstate = nullptr;
    size_t colstate_floats = 0;
    // device copies of the per-projection sin/cos for the batched launch
    float* d_sincos = nullptr;
    uint32_t d_sincos_cap = 0;
};

// finishes a call: propagates launch errors, honours PARIS_HIP_CTX_SYNCHRONOUS
inline int paris_hip_finish(paris_hip_ctx* ctx)
{
    PARIS_HIP_TRY(hipGetLastError());
    if(ctx->flags & PARIS_HIP_CTX_SYNCHRONOUS)
        PARIS_HIP_TRY(hipStreamSynchronize(ctx->stream));
    return PARIS_HIP_SUCCESS;
}

// a pooled projection buffer that contains d_p is no longer "nothing has used it since it was handed out"
inline void paris_hip_mark_touched(paris_hip_ctx* ctx, const void* d_p)
{
    if(ctx->proj_allocs.empty())
        return;
    auto a = ctx->proj_allocs.upper_bound(const_cast<void*>(d_p));
    if(a == ctx->proj_allocs.begin())
        return;
    --a;
    if(static_cast<const char*>(d_p) < static_cast<const char*>(a->first) + a->second.bytes)
        a->second.touched = true;
}

// called by every stage entry point after it has enqueued work that reads or writes `bytes` bytes of projection memory
// starting at d_p (a whole frame, or the rows of a band): every registered upload destination that overlaps the range gets
// its last-use event re-recorded. Uploads and stage calls may address different row ranges of one frame buffer.
inline int paris_hip_note_projection_use(paris_hip_ctx* ctx, const void* d_p, size_t bytes)
{
    const char* lo = static_cast<const char*>(d_p);
    const char* hi = lo + (bytes ? bytes : 1u);
    paris_hip_mark_touched(ctx, d_p);
    if(ctx->upload_targets.empty())
        return PARIS_HIP_SUCCESS;
    // Targets may overlap (a driver uploads to interior band pointers that change per task), so ANY earlier-starting target can
    // still reach into the range: all targets that start before hi are tested (a handful of slots per ctx).
    for(auto it = ctx->upload_targets.begin(); it != ctx->upload_targets.end() && static_cast<const char*>(it->first) < hi; ++it)
    {
        if(static_cast<const char*>(it->first) + it->second.bytes <= lo)
            continue;
        PARIS_HIP_TRY(hipEventRecord(it->second.last_use, ctx->stream));
        it->second.used = true;
    }
    return PARIS_HIP_SUCCESS;
}

void paris_hip_forget_upload_target(paris_hip_ctx* ctx, const void* d_p);

// capi.hip: has fused launch `group` (a paris_hip_ctx::group_seq value) finished? wait = true: blocks until it has
int paris_hip_group_done(paris_hip_ctx* ctx, uint64_t group, bool wait, bool* done);
// capi.hip: every parked device buffer goes back to the runtime (after the streams have drained): the answer to hipErrorOutOfMemory
int paris_hip_drain_device_pool(paris_hip_ctx* ctx);
#pragma GCC visibility push(hidden) // (library-internal: not in the dynamic symbol table)
// capi.hip: hipMalloc; on hipErrorOutOfMemory the device pool is drained and the allocation tried once more. *out is nullptr on failure.
int paris_hip_device_malloc(paris_hip_ctx* ctx, void** out, size_t bytes);
// capi.hip: a ctx-owned device buffer that only kernels of the compute stream read leaves the ctx (nullptr: nothing to do). Work already
// queued there may still read it, so it is freed by a later sweep, once that work has run; now = true, or no event to be had: the
// stream is waited for and the buffer freed at once.
void paris_hip_retire_device_buffer(paris_hip_ctx* ctx, void* d, bool now);
// capi.hip: frees the retired buffers no queued work can read any more (all = true: every one -- the streams have been drained)
void paris_hip_sweep_retired(paris_hip_ctx* ctx, bool all);
// capi.hip: makes the memory of a new setting: `bytes` from paris_hip_device_malloc, every fill enqueued on the ctx's auxiliary
// stream, and that stream waited for whether or not a copy failed. *out is the buffer, or empty with the first error returned.
struct paris_hip_fill
{
    size_t offset;
    const void* h_src; // nullptr: zeros
    size_t bytes;
};
int paris_hip_install(paris_hip_ctx* ctx, size_t bytes, std::initializer_list<paris_hip_fill> fills, paris_hip_device_buffer* out);
// the buffers of one setting (a member of paris_hip_ctx::each_setting)
template <class S, class F>
void paris_hip_each_buffer(S& s, F&& f)
{
    f(s.mem);
}
template <class F>
void paris_hip_each_buffer(paris_hip_ctx::row_extension_t& s, F&& f)
{
    for(auto& kv : s.cache)
        f(kv.second);
}
template <class F>
void paris_hip_each_buffer(paris_hip_ctx::volume_window_t& s, F&& f)
{
    f(s.mem), f(s.stage);
}
// A setting is replaced, cleared or ended: its buffers are retired (destroying = true: freed at once), the setting is as a new ctx
// has it, and the retired buffers no queued work can read any more are freed.
template <class S>
void paris_hip_release(paris_hip_ctx* ctx, S& s, bool destroying = false)
{
    paris_hip_each_buffer(s, [&](paris_hip_device_buffer& b) { paris_hip_retire_device_buffer(ctx, b.d, destroying); });
    s = S{};
    paris_hip_sweep_retired(ctx, destroying);
}
#pragma GCC visibility pop
// capi.hip: the pending group has been launched as `group` (0: dropped) -- buffers freed meanwhile are parked behind it, the others
// remember it as their last reader
int paris_hip_release_group_references(paris_hip_ctx* ctx, uint64_t group);
// backproject.hip: a library call is about to read (writer == nullptr) or write (on stream `writer`) [d_p, d_p + bytes) of a
// projection buffer. A buffer the pending deferred group refers to: the group is launched first. A write into a buffer a launched
// group may still be reading: `writer` is made to wait for that group.
int paris_hip_projection_guard_slow(paris_hip_ctx* ctx, const void* d_p, size_t bytes, hipStream_t writer, bool writes);
inline int paris_hip_projection_guard(paris_hip_ctx* ctx, const void* d_p, size_t bytes, hipStream_t writer, bool writes)
{
    if(ctx == nullptr || (ctx->held_count == 0u && ctx->group_seq == ctx->group_done_seq))
        return PARIS_HIP_SUCCESS; // nothing pending by reference, no launch outstanding
    return paris_hip_projection_guard_slow(ctx, d_p, bytes, writer, writes);
}

// capi.hip: the ctx's lazily made pieces (PARIS_HIP_CTX_WARM makes them all at once)
int paris_hip_ensure_aux(paris_hip_ctx* ctx);           // aux_stream + aux_counter
// capi.hip: runs one validator -- enqueue(stream, counter) launches a kernel that adds its mismatches to *counter -- on the ctx's
// auxiliary stream. *known = true: *ok is the answer (no mismatch). *known = false (asynchronous validation only): the check is
// running, ask again later with the same key; the caller uses the unvalidated-safe form meanwhile and caches nothing.
int paris_hip_run_check(paris_hip_ctx* ctx, const std::array<uint32_t, 4>& key, void (*enqueue)(hipStream_t, unsigned long long*, const void*),
                        const void* arg, bool* ok, bool* known);
int paris_hip_ensure_upload_stream(paris_hip_ctx* ctx); // upload_stream + its event ring
int paris_hip_ensure_bp_stream(paris_hip_ctx* ctx);     // bp_stream + its events
// one cheap query per translation unit with kernels, which makes the runtime load its code object now rather than at the first launch
void paris_hip_warm_backproject();
void paris_hip_warm_backproject_fused();
void paris_hip_warm_filter();
void paris_hip_warm_filter_fused();
void paris_hip_warm_weight();
void paris_hip_warm_validate();
void paris_hip_warm_widen();
void paris_hip_warm_redundancy_weights(); // short_scan.hip: the Parker and offset-detector kernels
void paris_hip_warm_flat_field();
void paris_hip_warm_forward_project();
void paris_hip_warm_defect_map();
#pragma GCC visibility push(hidden)
void paris_hip_warm_zinger();
void paris_hip_warm_ring();
void paris_hip_warm_volume_window();
void paris_hip_warm_binning();
void paris_hip_warm_axis_search();
void paris_hip_warm_air_region();
void paris_hip_warm_beam_hardening();
void paris_hip_warm_detector_roll();
void paris_hip_warm_lag();
void paris_hip_warm_metal();
void paris_hip_warm_phase();
// phase_rule.cpp: a[k] = alpha f^2 of n bins at this pitch, in double and rounded once; the extension's source sample of padded sample s
void paris_hip_phase_table(float alpha, uint32_t n, float pitch, float* a);
uint32_t paris_hip_phase_source(uint32_t s, uint32_t dim, uint32_t n);
void paris_hip_warm_scatter();
// scatter_rule.cpp: the four tables of G = g1x g1y + g2x g2y, in double and rounded once; the x tables carry the weights
void paris_hip_scatter_tables(const paris_hip_scatter_correction* s, uint32_t n_x, uint32_t n_y, float l_x, float l_y, float* g1x, float* g2x,
                              float* g1y, float* g2y);
void paris_hip_warm_volume_bilateral();
void paris_hip_warm_starvation();
// bilateral_rule.cpp: what paris_hip_volume_bilateral and its host rule refuse (the pointers are only compared, never read)
int paris_hip_volume_bilateral_check_call(const float* src, uint32_t dim_x, uint32_t dim_y, uint32_t src_dim_z, uint32_t z_first, uint32_t z_count,
                                          const struct paris_hip_volume_bilateral* setting, const float* dst);
#pragma GCC visibility pop

// widen.hip: enqueues on the ctx stream the in-place widening of rows whose stored pixels (PARIS_HIP_PIXEL_U8 / U16 / U32) sit in the
// tail of their float rows (paris_hip_upload_projection_raw)
int paris_hip_widen_rows(paris_hip_ctx* ctx, float* d_dst, size_t d_pitch, uint32_t dim_x, uint32_t dim_y, int pixel_type);
// widen.hip: the same pass for any stored type (PARIS_HIP_PIXEL_F32 included), each pixel then corrected with the ctx's dark and flat
// frames at detector row row0 + r (paris_hip_upload_projection_raw_corrected). PARIS_HIP_ERROR_INVALID_ARGUMENT without a setting, for
// another dim_x or rows outside the setting's.
int paris_hip_widen_correct_rows(paris_hip_ctx* ctx, float* d_dst, size_t d_pitch, uint32_t dim_x, uint32_t dim_y, int pixel_type,
                                 uint32_t row0);
#pragma GCC visibility push(hidden)
// filter.hip: what a filter launch of rows of dim_x pixels with the K whose permuted copy is d_kp (d_k: the K itself) adds at its
// store: *d_c = nullptr without a setting, else the device copy of c (made and cached on first use) and *m = edge_pixels.
// PARIS_HIP_ERROR_INVALID_ARGUMENT for dim_x < m, PARIS_HIP_ERROR_UNSUPPORTED for a K this ctx did not make.
int paris_hip_row_extension_for(paris_hip_ctx* ctx, const float* d_kp, uint32_t dim_x, const float** d_c, uint32_t* m);
int paris_hip_row_extension_for_k(paris_hip_ctx* ctx, const float* d_k, uint32_t dim_x, const float** d_c, uint32_t* m);

// axis_rule.cpp: the estimate both searches share (the rule is stated with paris_hip_axis_search in include/paris_hip.h). Candidates
// are (float)(lo + k step), k < count; a candidate is scored iff its cost is finite. PARIS_HIP_ERROR_INVALID_ARGUMENT when none is
// (out->scored = 0 then). The callers have checked lo, step, count and the pointers.
struct paris_hip_cost_estimate
{
    float value;                  // the estimate
    uint32_t best, scored, at_edge;
    double cost_min, cost_median; // J[best], the lower median of the scored J
};
int paris_hip_estimate_from_costs(double lo, double step, uint32_t count, const double* cost, paris_hip_cost_estimate* out);

// roll_rule.cpp: the six constants of the detector roll's rule, each computed in double and rounded to float once (the setting and
// the geometry have passed paris_hip_detector_roll_check, or eta_deg is exactly 0: the identity)
struct paris_hip_roll_constants
{
    float a, b, c, d, cx, cy;
};
paris_hip_roll_constants paris_hip_roll_constants_of(float eta_deg, const paris_detector_geometry& g);
// roll_rule.cpp: the mirror plan of the roll search and its margins (setting and geometry have passed paris_hip_roll_search_check)
struct paris_hip_roll_mirror
{
    int32_t i0; // the mirror column's left tap; -1: the column is not scored
    float w;    // the weight of column i0 + 1
};
void paris_hip_roll_search_plan(const paris_hip_roll_search& s, const paris_detector_geometry& g, uint32_t* margin_x, uint32_t* margin_y,
                                paris_hip_roll_mirror* columns);
// detector_roll.hip: enqueues the roll kernel on ctx->stream for a destination band and constants that have been checked
struct paris_hip_frame_band;
void paris_hip_detector_roll_launch(paris_hip_ctx* ctx, const paris_hip_frame_band& src, const paris_hip_frame_band& dst,
                                    const paris_hip_roll_constants& k);
#pragma GCC visibility pop

// Where the pieces of a roll search's one allocation lie (detector_roll.hip); roll_rule.cpp reports the total. In this order: the
// mean M and the rolled scratch frame R (n_col rows of n_row floats each, the row length padded to 16 bytes), the mirror plan (n_row
// 8-byte entries), the score kernel's partial sums (16 bytes per candidate and tile of 256 columns x 32 rows) and the totals (24
// bytes per candidate).
constexpr uint32_t PARIS_HIP_ROLL_TILE_COLUMNS = 256u, PARIS_HIP_ROLL_TILE_ROWS = 32u;
struct paris_hip_roll_layout
{
    size_t pitch, mean, rolled, plan, partial, total_of, bytes;
    uint32_t col_tiles, row_tiles;
};
inline paris_hip_roll_layout paris_hip_roll_layout_of(uint32_t n_row, uint32_t n_col, uint32_t count)
{
    paris_hip_roll_layout l{};
    const auto pad = [](size_t b) { return (b + 255u) / 256u * 256u; };
    l.pitch = (static_cast<size_t>(n_row) * sizeof(float) + 15u) / 16u * 16u;
    l.col_tiles = (n_row + PARIS_HIP_ROLL_TILE_COLUMNS - 1u) / PARIS_HIP_ROLL_TILE_COLUMNS;
    l.row_tiles = (n_col + PARIS_HIP_ROLL_TILE_ROWS - 1u) / PARIS_HIP_ROLL_TILE_ROWS;
    l.mean = 0u;
    l.rolled = l.mean + pad(l.pitch * n_col);
    l.plan = l.rolled + pad(l.pitch * n_col);
    l.partial = l.plan + pad(static_cast<size_t>(n_row) * 8u);
    l.total_of = l.partial + pad(static_cast<size_t>(count) * l.col_tiles * l.row_tiles * 16u);
    l.bytes = l.total_of + pad(static_cast<size_t>(count) * 24u);
    return l;
}

// what lies in front of the scratch in paris_hip_ctx::starvation_t::mem (starvation.hip; starvation_rule.cpp reports the total)
constexpr size_t PARIS_HIP_STARVATION_COUNTER_BYTES = 32u;
constexpr size_t PARIS_HIP_STARVATION_HEAD_BYTES =
    PARIS_HIP_STARVATION_COUNTER_BYTES + sizeof(float) * PARIS_HIP_STARVATION_LEVELS * (PARIS_HIP_STARVATION_RADIUS_MAX + 1u);

// what the counters at the head of paris_hip_ctx::metal_trace_t::mem occupy (metal.hip)
constexpr size_t PARIS_HIP_METAL_COUNTER_BYTES = 64u;

// Where the pieces of an air region's one allocation lie (air_region.hip); air_rule.cpp reports the total. The counters: four 64-bit
// counts (frames, normalised, too_few, above_limit), then the smallest and the largest value as ordered 32-bit keys, padded to 64 bytes.
constexpr size_t PARIS_HIP_AIR_COUNTER_BYTES = 64u;
struct paris_hip_air_layout
{
    size_t value, count, mask, bytes; // byte offsets of the launch's values, its counts and the mask; the whole size
};
inline paris_hip_air_layout paris_hip_air_layout_of(uint32_t width, uint32_t height)
{
    paris_hip_air_layout l{};
    l.value = PARIS_HIP_AIR_COUNTER_BYTES;
    l.count = l.value + PARIS_HIP_AIR_FRAMES_MAX * sizeof(float);
    l.mask = l.count + PARIS_HIP_AIR_FRAMES_MAX * sizeof(uint32_t);
    l.bytes = l.mask + ((static_cast<size_t>(width) * height + 15u) & ~static_cast<size_t>(15u));
    return l;
}

// Where the pieces of an open axis search lie in its one allocation (axis_search.hip), each 256-byte aligned; axis_rule.cpp reports
// the total. The score kernel's grid: a workgroup takes one candidate, PARIS_HIP_AXIS_TILE_COLUMNS columns (one per lane) and
// PARIS_HIP_AXIS_TILE_VIEWS consecutive views, and leaves one 16-byte partial sum.
constexpr uint32_t PARIS_HIP_AXIS_TILE_COLUMNS = 256u, PARIS_HIP_AXIS_TILE_VIEWS = 32u;
struct paris_hip_axis_layout
{
    uint32_t col_tiles, view_tiles;
    size_t plan, partial, total_of, bytes; // byte offsets of the plan, the partial sums and the totals; the whole size
};
inline paris_hip_axis_layout paris_hip_axis_layout_of(uint32_t n, uint32_t n_frames, uint32_t count)
{
    const auto up = [](size_t v) { return (v + 255u) & ~static_cast<size_t>(255u); };
    paris_hip_axis_layout l{};
    l.col_tiles = (n + PARIS_HIP_AXIS_TILE_COLUMNS - 1u) / PARIS_HIP_AXIS_TILE_COLUMNS;
    l.view_tiles = (n_frames + PARIS_HIP_AXIS_TILE_VIEWS - 1u) / PARIS_HIP_AXIS_TILE_VIEWS;
    l.plan = up(static_cast<size_t>(n_frames) * n * sizeof(float));
    l.partial = l.plan + up(static_cast<size_t>(count) * n * sizeof(paris_hip_axis_entry));
    l.total_of = l.partial + up(static_cast<size_t>(count) * l.col_tiles * l.view_tiles * 16u);
    l.bytes = l.total_of + up(static_cast<size_t>(count) * 24u);
    return l;
}

// capi.hip: timing-disabled events, recycled through ctx->spare_events
int paris_hip_take_event(paris_hip_ctx* ctx, hipEvent_t* out);
void paris_hip_give_event(paris_hip_ctx* ctx, hipEvent_t e);
// capi.hip: a copy on `stream_bit`'s stream (paris_hip_ctx::USED_*) reads or writes pinned host memory at h_ptr
void paris_hip_note_host_use(paris_hip_ctx* ctx, const void* h_ptr, unsigned stream_bit);

inline int paris_hip_bind(paris_hip_ctx* ctx)
{
    if(ctx == nullptr)
        return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    PARIS_HIP_TRY(hipSetDevice(ctx->device));
    return PARIS_HIP_SUCCESS;
}

int paris_hip_get_plan(paris_hip_ctx* ctx, uint32_t n, paris_hip_fft_plan** out);

// weight.hip: runs a held-back weighting (stage fusion) as its own kernel; no-op when none is pending
int paris_hip_flush_pending_weight(paris_hip_ctx* ctx);

// filter_fused.hip
bool paris_hip_volume_is_clean(const paris_hip_ctx* ctx, const void* d_v, size_t bytes); // capi.hip
int paris_hip_fused_filter_tables(paris_hip_ctx* ctx, uint32_t n, paris_hip_fft_plan* plan);
int paris_hip_fused_filter_permute_k(paris_hip_ctx* ctx, const float* d_k, uint32_t n, float** d_kp);
int paris_hip_fused_filter_launch(paris_hip_ctx* ctx, float* d_rows, uint32_t pitch_f, uint32_t dim_x, uint32_t n_rows, uint32_t row_first,
                                  bool weight, float h_min, float v_min, float d_sd, float l_px_row, float l_px_col, const float* d_kp,
                                  const paris_hip_fft_plan* plan, uint32_t filter_size, uint16_t* d_half, uint32_t half_pitch,
                                  uint32_t n_frames = 1u, size_t frame_stride_f = 0u, size_t half_frame_stride = 0u,
                                  float* const* frame_rows = nullptr); // frame_rows: the first band row of each frame instead of d_rows + f * stride

// backproject.hip: runs the projections pending in the deferral ring (no-op when there are none). Called by every entry
// point that observes or changes a volume, completes work, or changes how backprojection runs.
int paris_hip_flush_deferred(paris_hip_ctx* ctx);
// the same without the join: the pending projections are launched (on bp_stream when overlapping) and `stream` is NOT made to
// wait for them -- for the deferring call itself when its ring is full
int paris_hip_launch_deferred(paris_hip_ctx* ctx);

// validate.hip: device validators of the hand-expanded IEEE sequences of ieee_lean.h, cached per process, device and operand range
// (*ok = false: the kernels use the compiler's IEEE forms). lean division: both quotients d_sd / den and d_so / den for every fp32
// den in [0.09, 1.92] x d_so. lean weighting: sqrt and d_sd / sqrt for every fp32 radicand in [dd, q_max] (widened a little).
int paris_hip_lean_division_check(paris_hip_ctx* ctx, float d_sd, float d_so, bool* ok);
int paris_hip_lean_weighting_check(paris_hip_ctx* ctx, float d_sd, double dd, double q_max, bool* ok);

// backproject.hip: exhaustive validation of the fast division by the detector's pixel pitches, ahead of the first
// backprojection (cached per process and device; a no-op once known or when the fast division is switched off)
int paris_hip_prevalidate_fast_division(paris_hip_ctx* ctx, float l_px_row, float l_px_col);
int paris_hip_prevalidate_lean_division(paris_hip_ctx* ctx, float d_so, float d_od);

#endif
