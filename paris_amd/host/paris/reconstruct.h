// The reconstruction driver: tasks, per-device loop, device fan-out -- src/task.{h,cpp}, src/main.cpp:79-109,132-169.
//
// What is kept: one task per z-slab (src/task.cpp:38-48), a shared task queue drained by one host thread per device
// (src/main.cpp:157-167), the stage order load -> weight -> filter -> backproject per projection (:98-105), one
// sink shared by all threads.
// What is rebuilt for the GPU:
//   - the per-projection chain is enqueued asynchronously on the device's stream; the host thread meanwhile reads the
//     next HIS frame, as stored, into a pinned upload slot (slot = pinned host + device frame); the upload runs on a
//     second stream and the compute stream waits for it by event, so file I/O, PCIe upload and GPU work all overlap;
//     the device widens the stored pixels to fp32 (paris_hip_upload_projection_raw): a u16 frame crosses PCIe at 2 B per pixel;
//   - slots form two groups of `batch` frames; a full group is backprojected by one fused launch and guarded by a
//     stream fence, the host fills the other group meanwhile;
//   - per slab only the detector rows it can read are converted, uploaded, weighted and filtered (8f-4,
//     paris_hip_slab_row_band); the slab reaches the file through two pinned chunks (D2H of one overlapping the write
//     of the other) instead of a pinned copy of the whole slab, on a drain thread with a ctx of its own: a device that has
//     another slab to do works on it in a second volume buffer while the finished one is copied down and written;
//   - geometry constants are derived per call and the slab offset is passed per task (Q1, Q2), the source restarts
//     its frame index per task (Q5), slabs are written at their own slice offset (Q4);
//   - slab planning is 64-bit and memory driven (paris_hip_make_subvolume_information) with an optional fixed count.
#ifndef PARIS_AMD_HOST_RECONSTRUCT_H_
#define PARIS_AMD_HOST_RECONSTRUCT_H_

#include <chrono>
#include <condition_variable>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <deque>
#include <exception>
#include <functional>
#include <future>
#include <map>
#include <memory>
#include <mutex>
#include <queue>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "frame_rows.h"
#include "options.h"
#include "sink.h"
#include "source.h"
#include "types.h"

namespace paris
{
    static_assert(his::pixel_u8 == PARIS_HIP_PIXEL_U8 && his::pixel_u16 == PARIS_HIP_PIXEL_U16 && his::pixel_u32 == PARIS_HIP_PIXEL_U32
                      && his::pixel_f32 == PARIS_HIP_PIXEL_F32,
                  "his::pixel_type names the pixel types of paris_hip_upload_projection_raw");

    // src/task.h:33-57
    struct task
    {
        std::uint32_t id, num;
        std::string input_path;
        detector_geometry det_geo;
        volume_geometry vol_geo;
        subvolume_geometry subvol_geo;
        bool enable_roi;
        region_of_interest roi;
        bool enable_angles;
        std::string angle_path;
        std::uint16_t quality;
    };

    // src/task.cpp:33-51
    inline auto make_tasks(const program_options& po, const volume_geometry& vol_geo, const subvolume_info& info) -> std::queue<task>
    {
        auto q = std::queue<task>{};
        for(int i = 0; i < info.num; ++i)
            q.push(task{static_cast<std::uint32_t>(i), static_cast<std::uint32_t>(info.num), po.input_path, po.det_geo, vol_geo,
                        info.geo, po.enable_roi, po.roi, po.enable_angles, po.angle_path, po.quality});
        return q;
    }

    // the part of GLADOS' task_queue the driver uses: thread-safe pop / empty
    class task_queue
    {
    public:
        explicit task_queue(std::queue<task> q) : q_{std::move(q)} {}
        auto pop(task& out) -> bool
        {
            std::lock_guard<std::mutex> lock{m_};
            if(q_.empty())
                return false;
            out = q_.front();
            q_.pop();
            return true;
        }
    private:
        std::queue<task> q_;
        std::mutex m_;
    };

    // One read-once frame source (source.h: shared_frames) per pass of the task queue over the devices: tasks
    // [p * n_dev, (p + 1) * n_dev) are popped at about the same time by the n_dev device threads and all need every frame,
    // so the first thread to reach a frame reads it and the others copy their detector band from memory. A thread that
    // arrives after the others have finished the pass gets a fresh source (= its own read of the files, as before).
    class frame_pool
    {
    public:
        frame_pool(int n_dev, std::uint32_t n_row, std::uint32_t n_col) : n_dev_{n_dev < 1 ? 1 : n_dev}, n_row_{n_row}, n_col_{n_col} {}

        auto get(const struct task& t) -> std::shared_ptr<shared_frames>;

        struct totals
        {
            std::uint64_t produced = 0, served = 0, reread = 0;
        };
        auto stats() -> totals
        {
            std::lock_guard<std::mutex> lock{m_};
            auto sum = done_;
            for(auto& kv : live_)
                if(auto s = kv.second.lock())
                {
                    const auto c = s->stats();
                    sum.produced += c.produced;
                    sum.served += c.served;
                    sum.reread += c.reread;
                }
            return sum;
        }
        auto skipped_files() -> std::vector<std::string>
        {
            std::lock_guard<std::mutex> lock{m_};
            return skipped_;
        }
        // called by the last user of a pass's source (shared_ptr deleter)
        void retire(shared_frames* s)
        {
            {
                std::lock_guard<std::mutex> lock{m_};
                const auto c = s->stats();
                done_.produced += c.produced;
                done_.served += c.served;
                done_.reread += c.reread;
                if(skipped_.empty())
                    skipped_ = s->skipped_files();
            }
            delete s;
        }

    private:
        int n_dev_;
        std::uint32_t n_row_, n_col_;
        std::mutex m_;
        std::map<std::uint32_t, std::weak_ptr<shared_frames>> live_;
        totals done_;
        std::vector<std::string> skipped_;
    };

    struct device_report
    {
        int device = 0;
        std::uint32_t tasks = 0, projections = 0;
        std::uint64_t band_rows = 0; // sum over tasks of the detector rows processed per projection (f4)
        double source_s = 0, enqueue_s = 0, drain_s = 0, save_s = 0;
        double setup_s = 0;       // ctx, pinned slots, device frames: before the first task is popped
        double source_wait_s = 0; // the device thread waiting for the feed thread's next frame (read_ahead)
        double drain_wait_s = 0; // the device thread waiting for the drain thread (a volume buffer to come free; the end of the run)
        std::uint64_t h2d_bytes = 0; // projection rows uploaded, in their stored pixel type (paris_hip_upload_projection_raw)
        bool two_volumes = false; // a second slab buffer was in use: slab k went to the file while slab k + 1 was reconstructed
        bool defect_map = false;  // --defects / --defects-from-flat: a defect map was set; its counts:
        paris_hip_defect_stats defects{};
        bool zinger_filter = false; // --zingers: a zinger filter was set; its counts over this device's tasks:
        paris_hip_zinger_counts zingers{};
        bool air_region = false; // --air-region: the setting was made; its counts over this device's tasks:
        paris_hip_air_counts air{};
        bool row_extension = false; // --extend-rows: the setting was made on this device's ctx
        paris_hip_metal_counts metal{}; // --metal: the inpainting's counts over this device's tasks
        paris_hip_starvation_counts starvation{}; // --starvation: the filter's counts over this device's tasks
        paris_hip_volume_counts voxels{}; // --voxel-type: the counts of this device's drain ctx
        std::vector<std::string> skipped;
    };

    inline auto frame_pool::get(const task& t) -> std::shared_ptr<shared_frames>
    {
        const auto pass = t.id / static_cast<std::uint32_t>(n_dev_);
        std::lock_guard<std::mutex> lock{m_};
        auto& slot = live_[pass];
        if(auto s = slot.lock())
            return s;
        // ring depth: how far the device threads may drift apart before the slower one re-reads; at most ~1 GiB of frames
        const auto frame_bytes = static_cast<std::size_t>(n_row_) * n_col_ * sizeof(float);
        const auto capacity = std::max<std::size_t>(4, std::min<std::size_t>(32, (std::size_t{1} << 30) / std::max<std::size_t>(1, frame_bytes)));
        auto s = std::shared_ptr<shared_frames>{new shared_frames{t.input_path, t.enable_angles, t.angle_path, t.quality, n_row_, n_col_, capacity},
                                                [this](shared_frames* p) { retire(p); }};
        slot = s;
        return s;
    }

    namespace detail
    {
        using clock = std::chrono::steady_clock;
        inline double since(clock::time_point t) { return std::chrono::duration<double>(clock::now() - t).count(); }

        // a ctx of `device` for as long as the object lives. Declared before everything that lives in the ctx: destroyed after it
        class device_ctx
        {
        public:
            explicit device_ctx(int device) { rt(paris_hip_ctx_create(device, nullptr, PARIS_HIP_CTX_DEFAULT, &ctx_), "set_device()"); }
            device_ctx(const device_ctx&) = delete;
            auto operator=(const device_ctx&) -> device_ctx& = delete;
            ~device_ctx() { paris_hip_ctx_destroy(ctx_); }
            operator paris_hip_ctx*() const { return ctx_; }

        private:
            paris_hip_ctx* ctx_ = nullptr;
        };

        // the settings of the frame chain up to the zinger filter, the same for every device ctx of a run and for the pre-passes: --bin,
        // --flat / --dark, --lag, --air-region, --defects / --defects-from-flat and --zingers
        inline void set_frame_chain(paris_hip_ctx* ctx, const program_options& po, device_report& rep)
        {
            if(po.binning()) // --bin: the source detector's setting; everything below is at binned size
            {
                const auto setting = paris_hip_binning{po.bin_x, po.bin_y};
                rt(paris_hip_set_binning(ctx, &setting, po.bin_mask ? po.bin_mask->data() : nullptr, po.src_row, po.src_col), "set_binning()");
            }
            if(po.flat)
                rt(paris_hip_set_flat_field(ctx, po.dark ? po.dark->pixels.data() : nullptr, po.flat->pixels.data(), po.det_geo.n_row, po.det_geo.n_col,
                                            po.t_min), "set_flat_field()");
            if(po.lag)
                rt(paris_hip_set_lag_correction(ctx, &po.lag_model), "set_lag_correction()");
            auto mask = std::vector<std::uint8_t>{}; // the defect map's, which the air region leaves out as well
            if(po.defect_mask || po.defects_from_flat)
            {
                const auto n_px = static_cast<std::size_t>(po.det_geo.n_row) * po.det_geo.n_col;
                mask = po.defect_mask ? *po.defect_mask : std::vector<std::uint8_t>(n_px, 0u);
                int rc = PARIS_HIP_SUCCESS;
                if(po.defects_from_flat)
                {
                    auto dead = std::vector<std::uint8_t>(n_px, 0u);
                    rc = paris_hip_flat_field_dead_pixels(ctx, dead.data());
                    for(std::size_t k = 0; k < n_px; ++k)
                        mask[k] |= dead[k];
                }
                if(rc == PARIS_HIP_SUCCESS)
                    rc = paris_hip_set_defect_map(ctx, mask.data(), po.det_geo.n_row, po.det_geo.n_col);
                if(rc == PARIS_HIP_SUCCESS)
                    rc = paris_hip_defect_map_info(ctx, &rep.defects);
                rt(rc, "set_defect_map()");
                rep.defect_map = true;
            }
            if(po.air)
            {
                rt(paris_hip_set_air_region(ctx, &po.air_region, mask.empty() ? nullptr : mask.data(), po.det_geo.n_row, po.det_geo.n_col),
                   "set_air_region()");
                rep.air_region = true;
            }
            if(po.zingers)
            {
                const auto setting = paris_hip_zinger_filter{po.zinger_abs, po.zinger_rel, po.zinger_polarity, 0u};
                rt(paris_hip_set_zinger_filter(ctx, &setting, po.det_geo.n_row, po.det_geo.n_col), "set_zinger_filter()");
                rep.zinger_filter = true;
            }
        }

        // the settings of the chain behind the zinger filter, the same for every device ctx of a run and for the fit pre-pass (which
        // runs before there is a polynomial, and never with a roll): the correction frame of --rings from run()'s pre-pass,
        // --beam-hardening or the coefficients run()'s fit found, --detector-roll or the angle run()'s search found, --extend-rows and
        // the filter window. The ring / axis / roll pre-pass sets none of them: it stops in front of them, and a setting holds device
        // memory that counts against the reserve.
        inline void set_chain_back(paris_hip_ctx* ctx, const program_options& po, device_report& rep)
        {
            if(po.ring_c)
                rt(paris_hip_set_ring_correction(ctx, po.ring_c->data(), po.det_geo.n_row, po.det_geo.n_col), "set_ring_correction()");
            if(po.starvation)
                rt(paris_hip_set_starvation_filter(ctx, &po.starvation_setting, po.det_geo.n_row, po.det_geo.n_col), "set_starvation_filter()");
            if(po.scatter)
                rt(paris_hip_set_scatter_correction(ctx, &po.scatter_setting, po.det_geo.n_row, po.det_geo.n_col, po.det_geo.l_px_row, po.det_geo.l_px_col),
                   "set_scatter_correction()");
            if(po.phase)
                rt(paris_hip_set_phase_retrieval(ctx, &po.phase_setting, po.det_geo.n_row, po.det_geo.n_col, po.det_geo.l_px_row, po.det_geo.l_px_col),
                   "set_phase_retrieval()");
            if(po.beam_hardening)
                rt(paris_hip_set_beam_hardening(ctx, &po.bh, po.det_geo.n_row, po.det_geo.n_col), "set_beam_hardening()");
            if(po.roll)
            {
                const auto setting = paris_hip_detector_roll{po.roll_deg};
                rt(paris_hip_set_detector_roll(ctx, &setting, &po.det_geo), "set_detector_roll()");
            }
            if(po.extend_rows)
            {
                const auto setting = paris_hip_row_extension{po.extend_edge, po.extend_taper};
                rt(paris_hip_set_row_extension(ctx, &setting), "set_row_extension()");
                rep.row_extension = true;
            }
            if(po.metal_bits) // (the metal pre-pass itself runs before there are any)
            {
                rt(paris_hip_set_metal_trace(ctx, po.metal_bits->data(), po.metal_views, po.det_geo.n_row, po.det_geo.n_col), "set_metal_trace()");
                rt(paris_hip_set_metal_voxels(ctx, po.metal_index->data(), po.metal_value->data(), po.metal_index->size()), "set_metal_voxels()");
            }
            rt(paris_hip_set_filter_window(ctx, po.window), "filter window");
        }

        // frames per group and groups, as reconstruct() lays its slots out
        inline auto slot_shape(const program_options& po) -> std::pair<std::uint32_t, std::uint32_t>
        {
            const std::uint32_t batch = po.batch < 1 ? 1u : static_cast<std::uint32_t>(po.batch > 64 ? 64 : po.batch);
            const std::uint32_t groups = batch == 1u ? static_cast<std::uint32_t>(po.slots < 1 ? 1 : po.slots) : 2u;
            return {batch, groups};
        }

        // device memory reconstruct() keeps per device beside the slab: every slot's fp32 frame (rows padded to 256 B), its
        // half copy with --f16, and two drain chunks' worth of slack for the runtime's own staging; with --voxel-type the drain ctx's
        // scratch, one more chunk (a chunk is a whole slice at least: for slices beyond the chunk size the slack covers it), and its counters
        inline auto driver_bytes(const program_options& po) -> std::size_t
        {
            const auto shape = slot_shape(po);
            const auto slots = static_cast<std::size_t>(shape.first) * shape.second;
            const auto row = (static_cast<std::size_t>(po.det_geo.n_row) * sizeof(float) + 255u) / 256u * 256u;
            const auto half_row = (static_cast<std::size_t>(po.det_geo.n_row) * 2u + 255u) / 256u * 256u;
            // with --flat, the ctx's dark and flat frames (paris_hip_set_flat_field)
            const auto references = po.flat_path.empty() ? 0u : 2u * sizeof(float) * po.det_geo.n_row * static_cast<std::size_t>(po.det_geo.n_col);
            // (with --defects, the plan of the file's map; the few pixels --defects-from-flat may add are not known before a ctx exists)
            // with --bin, every slot's full-width source frame as well, and the source-size mask
            const auto src_row = (static_cast<std::size_t>(po.src_row) * sizeof(float) + 255u) / 256u * 256u;
            const auto binning = po.binning() ? slots * po.src_col * src_row + (po.bin_mask ? po.bin_mask->size() : 0u) : 0u;
            // with --detector-roll / --find-roll, every slot's rolled frame as well
            const auto rolled = po.roll || po.find_roll ? slots * po.det_geo.n_col * row : 0u;
            // with --lag, the state of a whole-detector sequence at most
            const auto lag_state = po.lag ? static_cast<std::size_t>(po.lag_model.terms) * sizeof(float) * po.det_geo.n_row * po.det_geo.n_col : 0u;
            return lag_state + rolled + slots * po.det_geo.n_col * (row + (po.f16 ? half_row : 0u)) + 2u * po.drain_chunk_bytes + references + po.defect_bytes + po.zinger_bytes + po.extend_bytes + po.ring_bytes + po.air_bytes + po.metal_bytes + po.phase_bytes + po.scatter_bytes + po.starvation_bytes + po.denoise_bytes
                   + binning + (po.voxels.type != 0 ? po.drain_chunk_bytes + (std::size_t{64} << 10) : 0u);
        }

        // Large detectors: halve the frames per group until the driver's buffers take at most a quarter of the smallest
        // device's free memory (8192^2 frames: 64 slots would be 16 GiB of device frames plus as much pinned host memory)
        inline auto fit_batch(program_options po, int n_dev) -> program_options
        {
            std::size_t smallest = ~std::size_t{0};
            for(int d = 0; d < n_dev; ++d)
            {
                std::size_t free_b = 0, total_b = 0;
                rt(paris_hip_device_memory(d, &free_b, &total_b), "device memory");
                smallest = std::min(smallest, free_b);
            }
            while(po.batch > 1 && driver_bytes(po) > smallest / 4u)
                po.batch /= 2;
            return po;
        }

        // The frame slots of a ctx, and their owner. A slot is a pinned host buffer with room for a frame as stored at 4 bytes per pixel,
        // and a device frame at the detector's size; the device frames of all slots lie one under the other in one allocation (slot s
        // starts at row s * n_col), so that a group of slots is n frames at a stride. With --bin a slot also has a full-width source
        // frame, which the frame is binned from; with `rolled` a second frame, same pitch and stride, that the roll writes and
        // everything after it reads; with `half` an IEEE half frame that the row filter writes. `fences` fences come with the slots,
        // one per group of the main loop.
        class frame_slots
        {
        public:
            frame_slots(paris_hip_ctx* ctx, const program_options& po, std::uint32_t count, std::uint32_t fences, bool rolled, bool half)
            : frame_slots{ctx} // the object is complete from here on: the destructor frees what was allocated before a throw
            {
                const auto n_row = po.det_geo.n_row, n_col = po.det_geo.n_col;
                const auto sn_row = po.binning() ? po.src_row : n_row, sn_col = po.binning() ? po.src_col : n_col;
                const auto frames = [&](std::uint32_t dim_x, std::uint32_t dim_y, float** d, std::size_t* d_pitch, const char* what) {
                    if(static_cast<std::uint64_t>(dim_y) * count > 0xffffffffull)
                        throw stage_construction_error{"too many projection slots for this detector"};
                    rt(paris_hip_malloc_projection(ctx, dim_x, dim_y * count, d, d_pitch), what);
                };
                frames(n_row, n_col, &d_all_, &pitch, "make_projection_device()");
                stride = pitch * n_col;
                if(po.binning())
                {
                    frames(sn_row, sn_col, &d_src_all_, &src_pitch, "make_projection_device()");
                    src_stride_ = src_pitch * sn_col;
                }
                if(rolled)
                {
                    std::size_t r_pitch = 0;
                    frames(n_row, n_col, &d_roll_all_, &r_pitch, "make_projection_device()");
                    if(r_pitch != pitch)
                        throw stage_runtime_error{"the rolled frames' pitch differs from the frames'"};
                }
                host_.assign(count, nullptr);
                for(auto& h : host_)
                {
                    void* p = nullptr;
                    rt(paris_hip_malloc_host(ctx, static_cast<std::size_t>(sn_row) * sn_col * sizeof(float), &p), "make_projection_host()");
                    h = static_cast<float*>(p);
                }
                fence_.assign(fences, nullptr);
                for(auto& f : fence_)
                    rt(paris_hip_fence_create(ctx, &f), "fence");
                if(half)
                {
                    float* raw = nullptr;
                    frames(static_cast<std::uint32_t>((static_cast<std::size_t>(n_row) * 2 + 255) / 256 * 256 / 4), n_col, &raw, &half_pitch, "half projection");
                    d_half_ = reinterpret_cast<std::uint16_t*>(raw);
                    half_stride = half_pitch * n_col;
                }
            }
            frame_slots(const frame_slots&) = delete;
            auto operator=(const frame_slots&) -> frame_slots& = delete;
            ~frame_slots()
            {
                for(auto f : fence_)
                    paris_hip_fence_destroy(ctx_, f);
                for(auto h : host_)
                    paris_hip_free_host(ctx_, h);
                paris_hip_free(ctx_, d_all_);
                paris_hip_free(ctx_, d_src_all_);
                paris_hip_free(ctx_, d_roll_all_);
                paris_hip_free(ctx_, d_half_);
            }

            auto host(std::uint32_t s) const -> float* { return host_[s]; }
            auto frame(std::uint32_t s) const -> float* { return at(d_all_, stride, s); }
            auto source(std::uint32_t s) const -> float* { return at(d_src_all_, src_stride_, s); } // --bin
            // the frame of slot s that the weights, the filter and the backprojection read: the rolled one if there is one
            auto out(std::uint32_t s) const -> float* { return d_roll_all_ != nullptr ? at(d_roll_all_, stride, s) : frame(s); }
            auto half(std::uint32_t s) const -> std::uint16_t* { return d_half_ != nullptr ? at(d_half_, half_stride, s) : nullptr; }
            auto hosts() const -> const std::vector<float*>& { return host_; }
            auto fences() const -> const std::vector<paris_hip_fence*>& { return fence_; }

            std::size_t pitch = 0, stride = 0;           // bytes from row to row of a frame, and from one slot's frame to the next
            std::size_t src_pitch = 0;                   // --bin: of the full-width frames
            std::size_t half_pitch = 0, half_stride = 0; // of the half frames (0 without them)

        private:
            explicit frame_slots(paris_hip_ctx* ctx) : ctx_{ctx} {}
            template<class T>
            static auto at(T* base, std::size_t bytes, std::uint32_t s) -> T* { return reinterpret_cast<T*>(reinterpret_cast<char*>(base) + bytes * s); }

            paris_hip_ctx* ctx_;
            std::vector<float*> host_;
            std::vector<paris_hip_fence*> fence_;
            float *d_all_ = nullptr, *d_src_all_ = nullptr, *d_roll_all_ = nullptr;
            std::uint16_t* d_half_ = nullptr;
            std::size_t src_stride_ = 0;
        };

        // The driver's frame chain, written once: from a frame as stored in a pinned slot to filtered rows, for one frame behind its
        // upload (grouped = false: n = 1 at stride 0) or for n slots from `first` on in one call each (grouped: at the slots' stride).
        // reconstruct() runs all of it either way; the ring / axis / roll pre-pass stops after clean(), the fit pre-pass puts its unit
        // polynomial into linearise(). Every pass runs only where its setting was made, on the rows the plan gives it (frame_rows.h).
        // The settings themselves are read and checked in options.h; the three pre-passes run the chain from the callbacks of one
        // walk over the scan (prepass_scope and walk_scan, below), the main loop from its own read-ahead feed (frame_feed).
        struct frame_chain
        {
            paris_hip_ctx* ctx;
            const program_options& po;
            const frame_slots& slots;
            bool repair; // a defect map is set

            // Slot s's pinned frame to corrected line integrals in its device frame, for the rows of `up`. The rows arrive as stored
            // (u8 / u16 / u32 / f32; f64 as f32): the upload carries those bytes and the device widens them, bit for bit the host's
            // conversion (:101 -- on the upload stream, overlapping the kernels of the previous projections). With --flat alone the
            // same pass corrects them with the reference rows of their absolute detector rows. With --bin the source rows go as stored
            // into the slot's full-width frame and are binned from there into the slot's frame; with --lag the detector's memory of
            // the frames before is taken off the (binned) counts -- unless that was done already (lag_applied: the fit pre-pass, which
            // uploads every group once per basis) --; either way the dark / flat correction then runs in place as a pass of its own:
            // the same bits as the corrected upload of such counts.
            void upload(std::uint32_t s, int pixel, const frame_rows& rows, bool lag_applied = false) const
            {
                const auto n_row = po.det_geo.n_row, n_col = po.det_geo.n_col;
                const bool binning = po.binning();
                const auto sn_row = binning ? po.src_row : n_row, sn_col = binning ? po.src_col : n_col;
                const auto px = his::pixel_size(pixel);
                const auto* h_band = reinterpret_cast<const char*>(slots.host(s)) + static_cast<std::size_t>(rows.src.first) * sn_row * px;
                auto* d_frame = slots.frame(s);
                if(!binning && !po.lag && po.flat)
                {
                    rt(paris_hip_upload_projection_raw_corrected(ctx, d_frame, slots.pitch, h_band, n_row * px, n_row, n_col, rows.up.first, rows.up.count,
                                                                 pixel), "load()");
                    return;
                }
                auto* d_raw = binning ? slots.source(s) : d_frame;
                const auto raw_pitch = binning ? slots.src_pitch : slots.pitch;
                rt(paris_hip_upload_projection_raw(ctx, reinterpret_cast<float*>(reinterpret_cast<char*>(d_raw) + static_cast<std::size_t>(rows.src.first) * raw_pitch),
                                                   raw_pitch, h_band, sn_row * px, sn_row, rows.src.count, pixel), "load()");
                if(binning)
                    rt(paris_hip_bin_frames(ctx, d_raw, raw_pitch, 0u, d_frame, slots.pitch, 0u, 1u, sn_row, sn_col, rows.up.first, rows.up.count), "bin()");
                if(po.lag && !lag_applied)
                    rt(paris_hip_lag_correct_rows(ctx, d_frame, slots.pitch, 0u, 1u, n_row, n_col, rows.up.first, rows.up.count), "lag correction");
                if((binning || po.lag) && po.flat)
                    rt(paris_hip_flat_field_rows(ctx, d_frame, slots.pitch, 0u, 1u, n_row, n_col, rows.up.first, rows.up.count), "flat field");
            }

            // the frames' own flux drift, straight after the correction; the band's defective pixels; then its outlier pixels
            void clean(std::uint32_t first, std::uint32_t n, bool grouped, const frame_rows& rows) const
            {
                const auto n_row = po.det_geo.n_row, n_col = po.det_geo.n_col;
                const auto stride = grouped ? slots.stride : 0u;
                auto* d = slots.frame(first);
                if(po.air)
                    rt(paris_hip_air_normalize_rows(ctx, d, slots.pitch, stride, n, n_row, n_col, rows.air.first, rows.air.count), "air normalisation");
                if(repair)
                    rt(paris_hip_defect_repair_rows(ctx, d, slots.pitch, stride, n, n_row, n_col, rows.fix.first, rows.fix.count), "defect repair");
                if(po.zingers)
                    rt(paris_hip_zinger_filter_rows(ctx, d, slots.pitch, stride, n, n_row, n_col, rows.band.first, rows.band.count), "zinger filter");
            }

            // the detector's stationary offsets, the starvation filter, the scatter correction and the phase retrieval -- 2-D passes over
            // whole frames: the run has no row band --, then the polynomial of the line integral: the run's, or `unit` in its place
            void linearise(std::uint32_t first, std::uint32_t n, bool grouped, const frame_rows& rows, const paris_hip_beam_hardening* unit = nullptr) const
            {
                const auto n_row = po.det_geo.n_row, n_col = po.det_geo.n_col;
                const auto stride = grouped ? slots.stride : 0u;
                auto* d = slots.frame(first);
                if(po.ring_c)
                    rt(paris_hip_ring_correct_rows(ctx, d, slots.pitch, stride, n, n_row, n_col, rows.band.first, rows.band.count), "ring correction");
                if(po.starvation)
                {
                    if(rows.band.first != 0u || rows.band.count != n_col)
                        throw stage_runtime_error{"starvation filter: the plan gave a row band to a pass that filters whole frames"};
                    rt(paris_hip_starvation_filter_frames(ctx, d, slots.pitch, stride, n, n_row, n_col), "starvation filter");
                }
                if(po.scatter)
                {
                    if(rows.band.first != 0u || rows.band.count != n_col)
                        throw stage_runtime_error{"scatter correction: the plan gave a row band to a pass that corrects whole frames"};
                    rt(paris_hip_scatter_correction_frames(ctx, d, slots.pitch, stride, n, n_row, n_col), "scatter correction");
                }
                if(po.phase)
                {
                    if(rows.band.first != 0u || rows.band.count != n_col)
                        throw stage_runtime_error{"phase retrieval: the plan gave a row band to a pass that filters whole frames"};
                    rt(paris_hip_phase_retrieval_frames(ctx, d, slots.pitch, stride, n, n_row, n_col), "phase retrieval");
                }
                if(unit != nullptr)
                    rt(paris_hip_beam_hardening_rows_with(ctx, unit, d, slots.pitch, stride, n, n_row, n_col, rows.band.first, rows.band.count), "beam hardening");
                else if(po.beam_hardening)
                    rt(paris_hip_beam_hardening_rows(ctx, d, slots.pitch, stride, n, n_row, n_col, rows.band.first, rows.band.count), "beam hardening");
            }

            // The roll, the last frame pass, into the slots' second frames, which everything after it reads; the redundancy weight of
            // an offset detector or of a short scan (angles: one per frame, in degrees) on the raw band, before the cosine weight;
            // then :102-103 in one launch: the weight rides along in the row filter's load, and with half frames the filtered band is
            // stored as IEEE half straight into them. One frame goes through the entry point for a frame, a group -- of one frame
            // too -- through the one for a batch.
            // With --metal the trace's pixels are inpainted between the two, on the ideal detector the roll writes (views: the trace
            // of each frame).
            void finish(std::uint32_t first, std::uint32_t n, bool grouped, const frame_rows& rows, const float* angles, const std::uint32_t* views = nullptr) const
            {
                const auto n_row = po.det_geo.n_row, n_col = po.det_geo.n_col;
                const auto stride = grouped ? slots.stride : 0u;
                const auto out = rows.out;
                auto* d = slots.out(first);
                if(po.roll)
                    rt(paris_hip_detector_roll_rows(ctx, slots.frame(first), slots.pitch, stride, d, slots.pitch, stride, n, n_row, n_col, out.first, out.count),
                       "detector roll");
                if(po.metal_bits)
                    rt(paris_hip_metal_inpaint_rows(ctx, d, slots.pitch, stride, n, n_row, n_col, out.first, out.count, views), "metal inpainting");
                if(po.offset_detector)
                    rt(paris_hip_offset_detector_weight_rows(ctx, d, slots.pitch, stride, n, n_row, n_col, out.first, out.count, &po.det_geo),
                       "offset-detector weight()");
                if(po.short_scan)
                    rt(paris_hip_short_scan_weight_rows(ctx, d, slots.pitch, stride, n, n_row, n_col, out.first, out.count, &po.det_geo, &po.scan, angles),
                       "short-scan weight()");
                if(grouped)
                    rt(paris_hip_stage_weight_filter_batch(ctx, d, slots.pitch, stride, n, n_row, n_col, out.first, out.count, &po.det_geo, slots.half(first),
                                                           slots.half_pitch, slots.half_stride), "weight() + filter()");
                else
                    rt(paris_hip_stage_weight_filter_rows(ctx, d, slots.pitch, n_row, n_col, out.first, out.count, &po.det_geo, slots.half(first),
                                                          slots.half_pitch), "weight() + filter()");
            }

            void run(std::uint32_t first, std::uint32_t n, bool grouped, const frame_rows& rows, const float* angles, const std::uint32_t* views = nullptr) const
            {
                clean(first, n, grouped, rows);
                linearise(first, n, grouped, rows);
                finish(first, n, grouped, rows, angles, views);
            }
        };
    }

    namespace detail
    {
        // A finished slab's way to the file (src/sink.cpp:72-82), on a thread and a ctx of its own: waits for the fence the device
        // thread recorded behind the slab's last kernel, copies the slab down in chunks of whole slices through two pinned buffers
        // (D2H of chunk k + 1 on the drain ctx's stream overlaps the file write of chunk k) and writes them at the slab's slice
        // offset. The device thread meanwhile reconstructs its next slab in another volume buffer; it only waits when it wants a
        // buffer back (wait) or is done (finish). An error in here is rethrown in the device thread by the next wait / finish.
        // With --voxel-type each chunk is quantised on the device into a scratch of the drain ctx and 1 or 2 bytes per voxel come down
        // (paris_hip_volume_quantize_d2h in the place of the copy); chunks stay whole slices, the two pinned buffers stay. With
        // --voxel-range auto the thread first takes the slab's extremes and histogram on the device and chooses the window.
        // With --denoise the slab buffer carries halo slices around the slab's own, and each chunk of own slices is first filtered
        // into a scratch of the drain ctx (paris_hip_volume_bilateral: its taps read the halo and the neighbouring chunks, which stay
        // as reconstructed); the copy, the quantisation and the statistics then take the chunk from the scratch.
        class volume_drain
        {
        public:
            struct job
            {
                const float* d_v = nullptr;
                std::uint32_t dim_x = 0, dim_y = 0, dim_z = 0, first = 0; // `first`: global slice of the slab's slice 0
                paris_hip_fence* ready = nullptr;                          // recorded by the device thread on its own ctx
                int buffer = 0;                                            // which of the device thread's volume buffers d_v is
                // --denoise: the buffer holds `halo` more slices in front of slice 0 and buf_z slices in all; d_v is the BUFFER's start
                std::uint32_t halo = 0, buf_z = 0;
            };

            volume_drain(int device, sink& out, std::size_t chunk_bytes, const voxel_output& voxels,
                         const struct paris_hip_volume_bilateral* denoise = nullptr)
            : device_{device}, out_(out), chunk_bytes_{chunk_bytes}, voxels_(voxels), denoise_{denoise != nullptr}
            {
                if(denoise != nullptr)
                    bilateral_ = *denoise;
                thread_ = std::thread{[this] { work(); }};
            }
            volume_drain(const volume_drain&) = delete;
            auto operator=(const volume_drain&) -> volume_drain& = delete;
            ~volume_drain()
            {
                {
                    std::lock_guard<std::mutex> lock{m_};
                    quit_ = true;
                }
                cv_.notify_all();
                if(thread_.joinable())
                    thread_.join();
            }

            void submit(const job& j)
            {
                {
                    std::lock_guard<std::mutex> lock{m_};
                    if(error_)
                        std::rethrow_exception(error_);
                    jobs_.push_back(j);
                    ++busy_[j.buffer & 1];
                }
                cv_.notify_all();
            }
            // until no submitted slab lives in volume buffer `buffer` any more
            void wait(int buffer)
            {
                std::unique_lock<std::mutex> lock{m_};
                cv_.wait(lock, [&] { return error_ || busy_[buffer & 1] == 0; });
                if(error_)
                    std::rethrow_exception(error_);
            }
            void finish()
            {
                wait(0);
                wait(1);
            }
            auto drain_seconds() -> double { std::lock_guard<std::mutex> lock{m_}; return drain_s_; }
            auto save_seconds() -> double { std::lock_guard<std::mutex> lock{m_}; return save_s_; }
            auto voxel_counts() -> paris_hip_volume_counts { std::lock_guard<std::mutex> lock{m_}; return counts_; }

        private:
            void work()
            {
                paris_hip_ctx* ctx = nullptr;
                char* h_stage[2] = {nullptr, nullptr};
                paris_hip_fence* stage_fence[2] = {nullptr, nullptr};
                std::size_t stage_voxels = 0;
                float* d_filtered = nullptr; // --denoise: a chunk's filtered floats, what is copied down or quantised (stream order: one is enough)
                const std::size_t voxel_bytes = voxels_.type == 0 ? sizeof(float) : (voxels_.type == PARIS_HIP_VOXEL_U8 ? 1u : 2u);
                auto window = paris_hip_volume_window{voxels_.lo, voxels_.hi, voxels_.type};
                try
                {
                    rt(paris_hip_ctx_create(device_, nullptr, PARIS_HIP_CTX_DEFAULT, &ctx), "set_device()");
                    for(;;)
                    {
                        job j;
                        {
                            std::unique_lock<std::mutex> lock{m_};
                            cv_.wait(lock, [&] { return quit_ || !jobs_.empty(); });
                            if(jobs_.empty())
                                break;
                            j = jobs_.front();
                            jobs_.pop_front();
                        }
                        double drain_s = 0, save_s = 0;
                        auto t0 = clock::now();
                        rt(paris_hip_fence_wait(ctx, j.ready), "fence wait"); // the slab's last kernel has run
                        // the host side of the slab is two pinned chunks of whole slices (the reference allocates the whole slab:
                        // src/sink.cpp:76); pinning gigabytes costs more than the reconstruction of a small data set
                        const auto slice_floats = static_cast<std::size_t>(j.dim_x) * j.dim_y;
                        const auto voxels = slice_floats * j.dim_z;
                        const auto want_voxels = std::max(slice_floats, std::min(voxels, chunk_bytes_ / voxel_bytes) / slice_floats * slice_floats);
                        if(want_voxels > stage_voxels)
                        {
                            for(int s = 0; s < 2; ++s)
                            {
                                rt(paris_hip_free_host(ctx, h_stage[s]), "free");
                                h_stage[s] = nullptr;
                                void* p = nullptr;
                                rt(paris_hip_malloc_host(ctx, want_voxels * voxel_bytes, &p), "make_volume_host()");
                                h_stage[s] = static_cast<char*>(p);
                                if(stage_fence[s] == nullptr)
                                    rt(paris_hip_fence_create(ctx, &stage_fence[s]), "fence");
                            }
                            if(denoise_)
                            {
                                rt(paris_hip_free(ctx, d_filtered), "free");
                                d_filtered = nullptr;
                                rt(paris_hip_malloc_volume(ctx, j.dim_x, j.dim_y, static_cast<std::uint32_t>(want_voxels / slice_floats), &d_filtered), "make_volume()");
                            }
                            stage_voxels = want_voxels;
                        }
                        const auto chunk_z = static_cast<std::uint32_t>(stage_voxels / slice_floats);
                        const auto n_chunks = (j.dim_z + chunk_z - 1u) / chunk_z;
                        // chunk c of the slab's own slices on the device: with --denoise filtered into the scratch first -- the taps reach
                        // into the halo slices and the neighbouring chunks, which stay as reconstructed --, else where it lies
                        const auto chunk_on_device = [&](std::uint32_t c) -> const float* {
                            const auto z0 = c * chunk_z;
                            const auto nz = std::min(chunk_z, j.dim_z - z0);
                            if(!denoise_)
                                return j.d_v + static_cast<std::size_t>(z0) * slice_floats;
                            rt(paris_hip_volume_bilateral(ctx, j.d_v, j.dim_x, j.dim_y, j.buf_z, j.halo + z0, nz, &bilateral_, d_filtered), "denoise");
                            return d_filtered;
                        };
                        if(voxels_.automatic) // the window from the finished volume: extremes, then 4096 bins over them, then the percentiles
                        {
                            // (with --denoise the finished volume is the filtered one, which exists a chunk at a time: every statistic is a
                            // sum, a minimum or a maximum over the chunks)
                            auto st = paris_hip_volume_statistics{};
                            auto hist = std::vector<std::uint64_t>(PARIS_HIP_VOLUME_HISTOGRAM_BINS_MAX, 0u);
                            const auto stats = [&](float lo, float hi, std::uint32_t n_bins, const char* what) {
                                if(!denoise_)
                                {
                                    rt(paris_hip_volume_stats(ctx, j.d_v, voxels, lo, hi, n_bins, n_bins != 0u ? hist.data() : nullptr, &st), what);
                                    return;
                                }
                                auto part = std::vector<std::uint64_t>(n_bins, 0u);
                                for(std::uint32_t c = 0; c < n_chunks; ++c)
                                {
                                    auto s = paris_hip_volume_statistics{};
                                    const auto nz = std::min(chunk_z, j.dim_z - c * chunk_z);
                                    rt(paris_hip_volume_stats(ctx, chunk_on_device(c), static_cast<std::uint64_t>(slice_floats) * nz, lo, hi, n_bins,
                                                              n_bins != 0u ? part.data() : nullptr, &s), what);
                                    st.min = c == 0u ? s.min : std::min(st.min, s.min);
                                    st.max = c == 0u ? s.max : std::max(st.max, s.max);
                                    for(std::uint32_t b = 0; b < n_bins; ++b)
                                        hist[b] = (c == 0u ? 0u : hist[b]) + part[b];
                                }
                            };
                            stats(0.f, 0.f, 0u, "volume stats");
                            if(!(st.min < st.max))
                                throw stage_runtime_error{"--voxel-range auto: the volume holds fewer than two different finite values"};
                            const float lo = st.min, hi = st.max;
                            stats(lo, hi, PARIS_HIP_VOLUME_HISTOGRAM_BINS_MAX, "volume histogram");
                            rt(paris_hip_volume_window_from_histogram(hist.data(), PARIS_HIP_VOLUME_HISTOGRAM_BINS_MAX, lo, hi, voxels_.p_lo,
                                                                      voxels_.p_hi, &window.lo, &window.hi), "window from histogram");
                            if(paris_hip_volume_window_check(&window) != PARIS_HIP_SUCCESS)
                                throw stage_runtime_error{"--voxel-range auto: the percentiles leave no window (" + std::to_string(window.lo) + " .. "
                                                          + std::to_string(window.hi) + ")"};
                            out_.set_window(window.lo, window.hi); // writes the .mhd
                        }
                        const auto copy_down = [&](std::uint32_t c) {
                            const auto z0 = c * chunk_z;
                            const auto nz = std::min(chunk_z, j.dim_z - z0);
                            const float* d_chunk = chunk_on_device(c);
                            if(voxels_.type == 0)
                                rt(paris_hip_memcpy_volume_d2h(ctx, reinterpret_cast<float*>(h_stage[c % 2u]), d_chunk, j.dim_x, j.dim_y, nz), "copy_d2h()");
                            else
                                rt(paris_hip_volume_quantize_d2h(ctx, d_chunk, static_cast<std::uint64_t>(slice_floats) * nz, &window, h_stage[c % 2u]),
                                   "quantize_d2h()");
                            rt(paris_hip_fence_record(ctx, stage_fence[c % 2u]), "fence record");
                        };
                        copy_down(0);
                        drain_s += since(t0);
                        for(std::uint32_t c = 0; c < n_chunks; ++c)
                        {
                            t0 = clock::now();
                            if(c + 1u < n_chunks)
                                copy_down(c + 1u); // its buffer was written to the file in the previous iteration
                            rt(paris_hip_fence_wait(ctx, stage_fence[c % 2u]), "fence wait");
                            drain_s += since(t0);
                            t0 = clock::now();
                            const auto z0 = c * chunk_z;
                            if(voxels_.type == 0)
                                out_.save(reinterpret_cast<const float*>(h_stage[c % 2u]), j.dim_x, j.dim_y, std::min(chunk_z, j.dim_z - z0), j.first + z0); // :107
                            else
                                out_.save_quantised(h_stage[c % 2u], j.dim_x, j.dim_y, std::min(chunk_z, j.dim_z - z0), j.first + z0);
                            save_s += since(t0);
                        }
                        auto counts = paris_hip_volume_counts{};
                        if(voxels_.type != 0) // (every copy of the slab has been waited for: this reads, and zeroes, at once)
                            rt(paris_hip_volume_quantize_counts(ctx, &counts, 1), "quantize counts");
                        {
                            std::lock_guard<std::mutex> lock{m_};
                            counts_.voxels += counts.voxels;
                            counts_.below += counts.below;
                            counts_.above += counts.above;
                            counts_.not_finite += counts.not_finite;
                            --busy_[j.buffer & 1];
                            drain_s_ += drain_s;
                            save_s_ += save_s;
                        }
                        cv_.notify_all();
                    }
                }
                catch(...)
                {
                    std::lock_guard<std::mutex> lock{m_};
                    error_ = std::current_exception();
                    jobs_.clear();
                    cv_.notify_all();
                }
                for(int s = 0; s < 2; ++s)
                {
                    paris_hip_fence_destroy(ctx, stage_fence[s]);
                    paris_hip_free_host(ctx, h_stage[s]);
                }
                paris_hip_free(ctx, d_filtered);
                paris_hip_ctx_destroy(ctx);
            }

            int device_;
            sink& out_;
            std::size_t chunk_bytes_;
            voxel_output voxels_;
            bool denoise_;
            struct paris_hip_volume_bilateral bilateral_{};
            paris_hip_volume_counts counts_{};
            std::mutex m_;
            std::condition_variable cv_;
            std::deque<job> jobs_;
            int busy_[2] = {0, 0};
            bool quit_ = false;
            std::exception_ptr error_;
            double drain_s_ = 0, save_s_ = 0;
            std::thread thread_; // last: started when everything above exists
        };
    }

    namespace detail
    {
        // The frames of one task, read and converted ahead of the device thread on a thread of their own, straight into the pinned
        // upload slots (src/main.cpp:100 `load`, taken off the device thread: converting a frame costs about as much host time as
        // enqueueing its upload, filter and share of a launch, and the two now overlap). The slots are filled in order, group after
        // group; before it overwrites a group's slots the reader waits until the device thread has enqueued the launch that last used
        // them (flushed) and for that launch's fence (paris_hip_fence_wait touches no ctx state: any thread may call it). The device
        // thread takes the frames in the same order. An error while reading is rethrown by take().
        class frame_feed
        {
        public:
            frame_feed(paris_hip_ctx* ctx, std::function<frame_info(float*)> next, const std::vector<float*>& slots, std::uint32_t batch,
                       const std::vector<paris_hip_fence*>& fences)
            : ctx_{ctx}, next_{std::move(next)}, slots_(slots), batch_{batch}, fences_(fences)
            {
                thread_ = std::thread{[this] { work(); }};
            }
            frame_feed(const frame_feed&) = delete;
            auto operator=(const frame_feed&) -> frame_feed& = delete;
            ~frame_feed()
            {
                {
                    std::lock_guard<std::mutex> lock{m_};
                    quit_ = true;
                }
                cv_.notify_all();
                if(thread_.joinable())
                    thread_.join();
            }

            // the next frame's metadata; its pixels are in slot (taken so far) % slots. !valid(): the set is exhausted
            auto take() -> frame_info
            {
                std::unique_lock<std::mutex> lock{m_};
                cv_.wait(lock, [&] { return error_ || !ready_.empty(); });
                if(ready_.empty())
                    std::rethrow_exception(error_);
                const auto info = ready_.front();
                ready_.pop_front();
                return info;
            }
            // the device thread has enqueued (and fenced) the launch over one more group of slots
            void flushed()
            {
                {
                    std::lock_guard<std::mutex> lock{m_};
                    ++flushed_;
                }
                cv_.notify_all();
            }
            auto read_seconds() -> double { std::lock_guard<std::mutex> lock{m_}; return read_s_; }

        private:
            void work()
            {
                try
                {
                    const auto groups = static_cast<std::uint64_t>(fences_.size());
                    for(std::uint64_t round = 0;; ++round)
                    {
                        {
                            std::unique_lock<std::mutex> lock{m_};
                            cv_.wait(lock, [&] { return quit_ || round < groups || flushed_ + groups > round; });
                            if(quit_)
                                return;
                        }
                        const auto g = static_cast<std::size_t>(round % groups);
                        rt(paris_hip_fence_wait(ctx_, fences_[g]), "fence wait"); // whatever last used this group's slots is done
                        for(std::uint32_t i = 0; i < batch_; ++i)
                        {
                            const auto t0 = clock::now();
                            const auto info = next_(slots_[g * batch_ + i]);
                            const auto dt = since(t0);
                            {
                                std::lock_guard<std::mutex> lock{m_};
                                read_s_ += dt;
                                ready_.push_back(info);
                                if(quit_)
                                    return;
                            }
                            cv_.notify_all();
                            if(!info.valid())
                                return;
                        }
                    }
                }
                catch(...)
                {
                    std::lock_guard<std::mutex> lock{m_};
                    error_ = std::current_exception();
                    cv_.notify_all();
                }
            }

            paris_hip_ctx* ctx_;
            std::function<frame_info(float*)> next_;
            std::vector<float*> slots_;
            std::uint32_t batch_;
            std::vector<paris_hip_fence*> fences_;
            std::mutex m_;
            std::condition_variable cv_;
            std::deque<frame_info> ready_;
            std::uint64_t flushed_ = 0;
            bool quit_ = false;
            std::exception_ptr error_;
            double read_s_ = 0;
            std::thread thread_; // last: started when everything above exists
        };
    }

    // src/main.cpp:79-109, pipelined
    inline auto reconstruct(task_queue& queue, int device, sink& out, const program_options& po, frame_pool* pool = nullptr) -> device_report
    {
        using namespace detail;
        auto rep = device_report{};
        rep.device = device;
        const auto t_setup = clock::now();
        const device_ctx ctx{device}; // :87
        set_frame_chain(ctx, po, rep);
        set_chain_back(ctx, po, rep);

        // Projections travel in groups: a group of `batch` frames is converted, uploaded, weighted and filtered one by one,
        // then backprojected with ONE fused launch (paris_hip_backproject_batch[_f16]: bit-identical to the sequence, the slab
        // is read and written once per group). While the GPU works on one group the host fills the next. batch = 1 is the
        // reference's one launch per projection with `slots` single-frame groups.
        const std::uint32_t batch = slot_shape(po).first, groups = slot_shape(po).second;
        const auto n_row = po.det_geo.n_row, n_col = po.det_geo.n_col;
        // --bin: frames are read and uploaded at the source detector's size into full-width slots of their own and binned from there
        // into the slots everything downstream works on; without it the two sizes are one and there are no full-width slots
        const bool binning = po.binning();
        const auto sn_row = binning ? po.src_row : n_row, sn_col = binning ? po.src_col : n_col;
        // Two volume buffers when the device has room for them: the slab just finished is copied down and written by the drain
        // thread while the next one is reconstructed in the other buffer. The second buffer is allocated when (and if) this device
        // thread pops a second task and a slab's worth of memory is still free.
        struct slab_buffers
        {
            paris_hip_ctx* ctx;
            float* d_vol[2];
            std::size_t cap[2];
            paris_hip_fence* done[2];
            ~slab_buffers()
            {
                for(int s = 0; s < 2; ++s)
                {
                    paris_hip_free(ctx, d_vol[s]);
                    paris_hip_fence_destroy(ctx, done[s]);
                }
            }
        } slab{ctx, {nullptr, nullptr}, {0, 0}, {nullptr, nullptr}};
        const frame_slots slots{ctx, po, batch * groups, groups, po.roll, po.f16};
        const frame_chain chain{ctx, po, slots, rep.defect_map};
        for(auto& f : slab.done)
            rt(paris_hip_fence_create(ctx, &f), "fence");
        // (declared last: its destructor joins the drain thread before anything above is freed -- nothing reads the volumes or the
        // fences after that --, and the ctx is destroyed last of all)
        volume_drain drain{device, out, po.drain_chunk_bytes, po.voxels, po.denoise ? &po.denoise_setting : nullptr};
        rep.setup_s = since(t_setup);
        task t{};
        bool two = false, decided = false;
        while(queue.pop(t)) // :89-91
        {
            const bool last = (t.num - t.id) <= 1;                                    // :92
            const auto own_z = t.subvol_geo.dim_z + (last ? t.subvol_geo.remainder : 0u); // make_volume: src/make_volume.cpp:32-34
            const auto own_offset = t.id * t.subvol_geo.dim_z;                         // :96
            // --denoise: the slab is reconstructed with up to RADIUS more slices on each side, as far as the output grid goes: the taps
            // of its own slices read them. Everything below sees the larger slab; the drain thread writes the own slices only
            const std::uint32_t grid_z = t.num * t.subvol_geo.dim_z + t.subvol_geo.remainder;
            const std::uint32_t reach = po.denoise ? po.denoise_setting.radius : 0u;
            const std::uint32_t halo_lo = std::min(reach, own_offset), halo_hi = std::min(reach, grid_z - (own_offset + own_z));
            const auto dim_z = halo_lo + own_z + halo_hi;
            const auto offset = own_offset - halo_lo;
            const auto voxels = static_cast<std::size_t>(t.subvol_geo.dim_x) * t.subvol_geo.dim_y * dim_z;
            if(rep.tasks == 1u && !decided) // a second slab for this device: is there room to keep the first while it is written?
            {
                std::size_t free_b = 0, total_b = 0;
                rt(paris_hip_device_memory(device, &free_b, &total_b), "device memory");
                // a slab the size of the largest of the run (the last one carries the remainder) plus slack for the runtime
                const auto need = static_cast<std::size_t>(t.subvol_geo.dim_x) * t.subvol_geo.dim_y * (t.subvol_geo.dim_z + t.subvol_geo.remainder + 2u * reach) * sizeof(float);
                two = po.two_volumes && free_b > need + need / 8u + (std::size_t{256} << 20);
                decided = true;
                rep.two_volumes = two;
            }
            const int b = two ? static_cast<int>(rep.tasks & 1u) : 0;
            auto t0 = clock::now();
            drain.wait(b); // the slab that lived in this buffer is in the file
            rep.drain_wait_s += since(t0);
            float*& d_v = slab.d_vol[b];
            if(voxels > slab.cap[b]) // slabs of one run have (almost) the same size: allocate once, re-zero per task
            {
                rt(paris_hip_free(ctx, d_v), "free");
                d_v = nullptr;
                slab.cap[b] = 0;
                rt(paris_hip_malloc_volume(ctx, t.subvol_geo.dim_x, t.subvol_geo.dim_y, dim_z, &d_v), "make_volume()");
                slab.cap[b] = voxels;
            }
            else
                rt(paris_hip_memset_volume(ctx, d_v, t.subvol_geo.dim_x, t.subvol_geo.dim_y, dim_z), "make_volume()");

            auto band = row_range{0u, n_col};
            if(po.row_band)
                rt(paris_hip_slab_row_band(&t.det_geo, &t.vol_geo, t.subvol_geo.dim_x, t.subvol_geo.dim_y, dim_z, offset, t.enable_roi,
                                           &t.roi, &band.first, &band.count), "slab_row_band()");
            rep.band_rows += band.count;
            // f4: only the detector rows this slab can read are converted, uploaded, weighted and filtered; the buffers keep
            // their full size, rows outside the band are never read for a voxel of the slab. Which rows each pass covers: the plan
            const auto roll = paris_hip_detector_roll{po.roll_deg};
            const auto rows = plan_frame_rows(band, n_col, rep.defects.reach_rows, po.zingers, po.air ? &po.air_region : nullptr,
                                              binning ? po.bin_y : 1u, po.roll ? &roll : nullptr, &t.det_geo);

            // --lag: this pass over the scan is a sequence of its own, from frame 0 of the file, for the rows it uploads
            if(po.lag && rows.band.count != 0)
                rt(paris_hip_lag_begin(ctx, n_row, n_col, rows.up.first, rows.up.count), "lag_begin()");

            t0 = clock::now();
            // :93 (index restarts per task). Several devices: the frames come from the pass's read-once source
            auto shared = pool != nullptr ? pool->get(t) : std::shared_ptr<shared_frames>{};
            auto cur = shared_frames::cursor{};
            auto own = std::unique_ptr<frame_stream>{};
            if(!shared)
                own.reset(new frame_stream{t.input_path, t.enable_angles, t.angle_path, t.quality});
            rep.source_s += since(t0);
            std::uint32_t group = 0, filled = 0; // frames of the current group already enqueued
            auto feed = std::unique_ptr<frame_feed>{};
            auto sines = std::vector<float>(batch), cosines = std::vector<float>(batch);
            auto angles = std::vector<float>(batch); // --short-scan: each frame's angle [deg], resolved as paris_hip_stage_angle does
            auto views = std::vector<std::uint32_t>(batch); // --metal: each frame's trace, its index in the scan after the quality stride
            const float delta_s = t.det_geo.delta_s * t.det_geo.l_px_row, delta_t = t.det_geo.delta_t * t.det_geo.l_px_col; // src/backprojection.cpp:49-50
            // frames of up to 1024 x 1024 are weighted and filtered group by group (one launch for up to `batch` frames when the
            // group is flushed) instead of frame by frame behind each upload: their launches are mostly latency
            const bool filter_by_group = batch > 1u && static_cast<std::uint64_t>(n_row) * n_col <= (1ull << 20);
            const auto flush = [&] { // one fused launch for the frames of the current group, then on to the other group
                if(filled == 0)
                    return;
                const auto t1 = clock::now();
                if(filter_by_group && rows.band.count != 0) // the chain for the group: one call per pass
                    chain.run(group * batch, filled, true, rows, angles.data(), views.data());
                if(po.f16)
                    rt(paris_hip_backproject_batch_f16(ctx, slots.half(group * batch), slots.half_pitch, slots.half_stride, filled, n_row, n_col, d_v,
                                                       t.subvol_geo.dim_x, t.subvol_geo.dim_y, dim_z, offset, &t.det_geo, &t.vol_geo, t.enable_roi, &t.roi,
                                                       sines.data(), cosines.data(), delta_s, delta_t), "backproject()");
                else
                    rt(paris_hip_backproject_batch(ctx, slots.out(group * batch), slots.pitch, slots.stride, filled, n_row, n_col, d_v, t.subvol_geo.dim_x,
                                                   t.subvol_geo.dim_y, dim_z, offset, &t.det_geo, &t.vol_geo, t.enable_roi, &t.roi, sines.data(),
                                                   cosines.data(), delta_s, delta_t), "backproject()"); // :104
                rt(paris_hip_fence_record(ctx, slots.fences()[group]), "fence record"); // the group's slots are free once this has run
                rep.enqueue_s += since(t1);
                group = (group + 1u) % groups;
                filled = 0;
                if(feed)
                    feed->flushed();
            };
            const auto next_frame = [&](float* dst) {
                return shared ? shared->next_raw(cur, dst, sn_row, sn_col, rows.src.first, rows.src.count)
                              : own->next_raw(dst, sn_row, sn_col, rows.src.first, rows.src.count); // :100, straight into pinned memory
            };
            if(po.read_ahead)
                feed.reset(new frame_feed{ctx, next_frame, slots.hosts(), batch, slots.fences()});
            for(;;) // :98
            {
                const auto slot = group * batch + filled;
                auto p = frame_info{};
                if(feed)
                {
                    t0 = clock::now();
                    p = feed->take(); // read by the feed thread, which also waited for the slot to be free
                    rep.source_wait_s += since(t0);
                }
                else
                {
                    t0 = clock::now();
                    if(filled == 0)
                        rt(paris_hip_fence_wait(ctx, slots.fences()[group]), "fence wait"); // everything that last used this group's slots is done
                    rep.enqueue_s += since(t0);
                    t0 = clock::now();
                    p = next_frame(slots.host(slot));
                    rep.source_s += since(t0);
                }
                if(!p.valid())
                    break;
                if(p.dim_x != sn_row || p.dim_y != sn_col)
                    throw stage_runtime_error{"projection size does not match the detector geometry"};
                t0 = clock::now();
                if(rows.band.count != 0)
                {
                    chain.upload(slot, p.pixel, rows);
                    rep.h2d_bytes += static_cast<std::uint64_t>(rows.src.count) * sn_row * his::pixel_size(p.pixel);
                    angles[filled] = t.enable_angles ? p.phi : static_cast<float>(p.idx) * t.det_geo.delta_phi; // src/backprojection.cpp:52-57
                    views[filled] = p.idx / std::max<std::uint32_t>(1u, t.quality);
                    // (small frames: the whole group by one call per pass when it is flushed -- a launch per 512^2 frame is mostly latency)
                    if(!filter_by_group)
                        chain.run(slot, 1u, false, rows, &angles[filled], &views[filled]);
                }
                rt(paris_hip_stage_angle(&t.det_geo, p.idx, t.enable_angles, p.phi, &sines[filled], &cosines[filled]), "angle"); // src/backprojection.cpp:52-63
                rep.enqueue_s += since(t0);
                if(++filled == batch)
                    flush();
                ++rep.projections;
            }
            flush(); // the last, possibly partial group
            if(po.lag)
                rt(paris_hip_lag_end(ctx), "lag_end()");
            if(feed)
            {
                rep.source_s += feed->read_seconds();
                feed.reset(); // joins the feed thread: the source objects are this thread's again
            }
            for(const auto& s : (shared ? cur.skipped_files() : own->skipped_files())) // the shared source's list: run_report
                rep.skipped.push_back(s);

            if(po.metal_index) // the slab's last backprojection is queued: its metal voxels go back, ahead of the fence the drain waits for
                rt(paris_hip_metal_reinsert(ctx, d_v, t.subvol_geo.dim_x, t.subvol_geo.dim_y, dim_z, offset), "metal reinsertion");
            // src/sink.cpp:76-82: the slab is complete behind this fence; the drain thread takes it from there
            rt(paris_hip_fence_record(ctx, slab.done[b]), "fence record");
            auto j = volume_drain::job{};
            j.d_v = d_v;
            j.dim_x = t.subvol_geo.dim_x;
            j.dim_y = t.subvol_geo.dim_y;
            j.dim_z = own_z;
            j.first = own_offset;
            j.halo = halo_lo;
            j.buf_z = dim_z;
            j.ready = slab.done[b];
            j.buffer = b;
            drain.submit(j);
            ++rep.tasks;
        }
        const auto t_end = clock::now();
        drain.finish();
        rep.drain_wait_s += since(t_end);
        if(po.zingers)
            rt(paris_hip_zinger_stats(ctx, &rep.zingers, 0), "zinger stats");
        if(po.air)
            rt(paris_hip_air_stats(ctx, &rep.air, 0), "air stats");
        if(po.metal_bits)
            rt(paris_hip_metal_stats(ctx, &rep.metal, 0), "metal stats");
        if(po.starvation)
            rt(paris_hip_starvation_stats(ctx, &rep.starvation, 0), "starvation stats");
        rep.drain_s = drain.drain_seconds();
        rep.save_s = drain.save_seconds();
        rep.voxels = drain.voxel_counts();
        return rep;
    }

    struct run_report
    {
        volume_geometry vol_geo{}, roi_geo{};
        subvolume_info info{};
        std::vector<device_report> devices;
        std::uint64_t frames_read = 0, frames_requested = 0; // several devices: frames converted from the files / frames handed to device threads
        bool shared_source = false;   // several devices: the read-once shared frame source was used
        double rows_per_pass = 0.0;   // several devices: detector rows the slabs of one pass need between them, in detectors
        std::vector<std::string> skipped;                  // several devices: invalid files skipped by the shared source
        int batch = 0; // frames per fused launch actually used (program_options::batch, halved until the slots fit the devices)
        std::uint32_t flat_frames = 0, dark_frames = 0; // --flat / --dark: frames averaged into the reference frames (0: no correction)
        bool defect_map = false;                        // --defects / --defects-from-flat: a map was set, with these counts
        paris_hip_defect_stats defects{};
        bool zinger_filter = false;                     // --zingers: the filter was on; its counts over all devices and slabs (a
        paris_hip_zinger_counts zingers{};              // frame counts once per slab: each slab filters its own row band)
        bool air_region = false;                        // --air-region: the setting was on; its counts over all devices and slabs (a
        paris_hip_air_counts air{};                     // frame counts once per slab), and with --rings / --find-axis the pre-pass's
        paris_hip_air_counts air_prepass{};
        std::uint32_t air_row = 0, air_col = 0;         // the frame the rectangle was checked against (binned with --bin)
        bool row_extension = false;                     // --extend-rows: every device filtered with the setting
        bool ring_filter = false;                       // --rings: the pre-pass ran; what the rule did to the scan's mean frame, and
        paris_hip_ring_stats rings{};                   // how long the pre-pass took (reading the scan included)
        std::uint32_t ring_frames = 0;
        double ring_prepass_s = 0;
        bool axis_search = false;                       // --find-axis: the search ran over axis_frames frames and axis_count
        paris_hip_axis_result axis{};                   // candidates; the delta_s of the geometry file it replaced, and how long the
        std::uint32_t axis_frames = 0, axis_count = 0;  // pre-pass took (reading the scan included; with --rings the same pre-pass)
        float axis_given = 0.f;
        double axis_prepass_s = 0;
        bool beam_hardening = false;                    // --beam-hardening / --fit-beam-hardening: every frame went through this
        paris_hip_beam_hardening bh{};                  // setting; with the fit: what it found -- coefficients, template level and the
        bool bh_fitted = false;                         // two residuals --, the threshold, the counts, the frames and the slab
        paris_hip_bh_fit bh_fit{};                      // (slices from bh_slice_first) of its pre-pass, and how long that took
        paris_hip_bh_counts bh_counts{};                // (reading the scan included)
        float bh_threshold = 0.f;
        std::uint32_t bh_frames = 0, bh_slice_first = 0, bh_slices = 0;
        double bh_prepass_s = 0;
        bool starvation = false;                        // --starvation: every frame went through this setting; its counts over all
        paris_hip_starvation_filter starvation_setting{}; // devices and slabs (a frame counts once per slab) and the pixels examined
        paris_hip_starvation_counts starvation_counts{};
        std::uint64_t starvation_pixels = 0;
        bool scatter = false;                           // --scatter: every frame went through this setting at these pitches; the
        paris_hip_scatter_correction scatter_setting{}; // padded size and the scratch a device keeps for it
        float scatter_l_x = 0.f, scatter_l_y = 0.f;
        std::uint32_t scatter_nx = 0, scatter_ny = 0;
        std::size_t scatter_scratch = 0;
        bool phase = false;                             // --phase / --phase-alpha: every frame went through this setting at these
        paris_hip_phase_retrieval phase_setting{};      // pitches; the padded size and the scratch a device keeps for it
        float phase_l_x = 0.f, phase_l_y = 0.f;
        std::uint32_t phase_nx = 0, phase_ny = 0;
        std::size_t phase_scratch = 0;
        bool metal = false;                             // --metal: the pre-pass ran; what it found, and the main pass's counts over all devices
        float metal_threshold = 0.f, metal_min_path = 0.f;
        std::uint32_t metal_grow = 0, metal_frames = 0;
        std::uint64_t metal_voxels = 0, metal_trace_pixels = 0;
        paris_hip_metal_counts metal_counts{};
        double metal_prepass_s = 0;
        bool detector_roll = false;                     // --detector-roll / --find-roll: every frame was resampled by roll_deg;
        float roll_deg = 0.f;                           // with the search: the estimate and its costs' summary, the frames of its
        bool roll_search = false;                       // pre-pass, the candidates, and how long the pre-pass took (reading the
        paris_hip_roll_result roll{};                   // scan included; with --rings / --find-axis the same pre-pass)
        std::uint32_t roll_frames = 0, roll_count = 0;
        double roll_prepass_s = 0;
        bool binning = false;                           // --bin: the factors, the source and the binned detector, and how many binned
        std::uint32_t bin_x = 1, bin_y = 1;             // pixels have no good source pixel (they join the defect map)
        std::uint32_t src_row = 0, src_col = 0, binned_row = 0, binned_col = 0;
        std::uint64_t binned_defective = 0;
        bool lag = false;                               // --lag: every pass over the scan corrected the frames' counts with this model,
        paris_hip_lag_model lag_model{};                // whose instantaneous weight is lag_b0
        double lag_b0 = 0.0;
        bool denoise = false;                           // --denoise: every voxel written passed the bilateral filter with this setting
        struct paris_hip_volume_bilateral denoise_setting{};
        int voxel_type = 0;                             // --voxel-type: the voxels were quantised over [voxel_lo, voxel_hi] (with
        float voxel_lo = 0.f, voxel_hi = 0.f;           // --voxel-range auto: the window chosen); the counts of every drain ctx, added
        paris_hip_volume_counts voxels{};
        double wall_s = 0;
        std::string output_file;
    };

    namespace detail
    {
        // --short-scan: the scan the frames of the run cover, from their first and last angle (after the quality stride). The
        // angles must be strictly monotonic, and the range must be at least 180 degrees plus twice the fan angle: otherwise some
        // rays are never measured, and the run is refused here, before any device work.
        inline auto derive_short_scan(const program_options& po) -> paris_short_scan
        {
            const auto a = frame_angles(po.input_path, po.enable_angles, po.angle_path, po.quality, po.det_geo.delta_phi);
            if(a.size() < 2u)
                throw stage_construction_error{"--short-scan needs at least two projections"};
            const bool up = a[1] > a[0];
            for(std::size_t i = 1; i < a.size(); ++i)
                if(up ? !(a[i] > a[i - 1]) : !(a[i] < a[i - 1]))
                    throw stage_construction_error{"--short-scan: the projection angles are not monotonic (frame " + std::to_string(i) + ": "
                                                   + std::to_string(a[i]) + " degrees after " + std::to_string(a[i - 1]) + ")"};
            const auto scan = paris_short_scan{up ? a.front() : a.back(), std::abs(a.back() - a.front())};
            float gamma_m = 0.f;
            if(paris_hip_short_scan_check(&po.det_geo, &scan, &gamma_m) != PARIS_HIP_SUCCESS)
            {
                const double need = 180.0 + 2.0 * gamma_m;
                char msg[256];
                if(scan.range_deg > 360.f)
                    std::snprintf(msg, sizeof msg, "--short-scan: the projections cover %.4f degrees, more than 360", scan.range_deg);
                else
                    std::snprintf(msg, sizeof msg, "--short-scan: the projections cover %.4f degrees, a short scan needs at least 180 + 2 * %.4f = %.4f "
                                  "(%.4f degrees short)", scan.range_deg, gamma_m, need, need - scan.range_deg);
                throw stage_construction_error{msg};
            }
            return scan;
        }

        // --flat / --dark: each file's frames averaged into one reference frame (his::mean_frame), refused here -- before any device
        // work -- when the file cannot be read or holds no frames, when its frames are not the detector's size, when it lies inside
        // --input (it would be read as a projection too), or when t_min is outside (0, 1]
        inline auto load_reference(const std::string& option, const std::string& path, const program_options& po) -> std::shared_ptr<const his::mean>
        {
            char in_dir[PATH_MAX], file[PATH_MAX];
            if(::realpath(path.c_str(), file) == nullptr)
                throw stage_construction_error{option + " " + path + ": no such file"};
            if(::realpath(po.input_path.c_str(), in_dir) != nullptr)
            {
                const auto dir = std::string{in_dir} + "/";
                if(std::string{file}.compare(0, dir.size(), dir) == 0)
                    throw stage_construction_error{option + " " + path + " lies inside --input " + po.input_path
                                                   + ": it would be read as a projection as well"};
            }
            auto m = std::make_shared<his::mean>();
            try { *m = his::mean_frame(path); }
            catch(const std::system_error&) { throw stage_construction_error{option + " " + path + ": cannot open the file"}; }
            if(m->n_frames == 0)
                throw stage_construction_error{option + " " + path + ": the file holds no frames"};
            if(m->dim_x != po.det_geo.n_row || m->dim_y != po.det_geo.n_col)
                throw stage_construction_error{option + " " + path + ": its frames are " + std::to_string(m->dim_x) + " x " + std::to_string(m->dim_y)
                                               + " pixels, the geometry's detector is " + std::to_string(po.det_geo.n_row) + " x "
                                               + std::to_string(po.det_geo.n_col)};
            return m;
        }

        inline auto load_flat_field(program_options& po) -> void
        {
            if(po.flat_path.empty())
            {
                if(!po.dark_path.empty())
                    throw stage_construction_error{"--dark needs --flat: a dark frame alone does not make line integrals"};
                return;
            }
            if(!(po.t_min > 0.f && po.t_min <= 1.f))
                throw stage_construction_error{"--min-transmission " + std::to_string(po.t_min) + " is outside (0, 1]"};
            po.flat = load_reference("--flat", po.flat_path, po);
            if(!po.dark_path.empty())
                po.dark = load_reference("--dark", po.dark_path, po);
        }
    }

    namespace detail
    {
        // --defects: n_col x n_row raw bytes, refused here -- before any device work -- when the file cannot be read or has another size;
        // --defects-from-flat: refused without --flat
        inline auto load_defects(program_options& po) -> void
        {
            if(po.defects_from_flat && po.flat_path.empty())
                throw stage_construction_error{"--defects-from-flat needs --flat: the dead pixels are those of the flat-field setting"};
            if(po.defects_path.empty())
                return;
            const auto n = static_cast<std::size_t>(po.det_geo.n_row) * po.det_geo.n_col;
            auto mask = std::make_shared<std::vector<std::uint8_t>>(n + 1u);
            std::FILE* f = std::fopen(po.defects_path.c_str(), "rb");
            if(f == nullptr)
                throw stage_construction_error{"--defects " + po.defects_path + ": cannot open the file"};
            const auto got = std::fread(mask->data(), 1u, n + 1u, f); // (one byte more than wanted: a longer file is seen as well)
            std::fclose(f);
            if(got != n)
                throw stage_construction_error{"--defects " + po.defects_path + ": the file holds " + (got > n ? "more than " : "") + std::to_string(std::min(got, n))
                                               + " bytes, the geometry's detector has " + std::to_string(po.det_geo.n_row) + " x "
                                               + std::to_string(po.det_geo.n_col) + " = " + std::to_string(n) + " pixels"};
            mask->resize(n);
            paris_hip_defect_plan* plan = nullptr;
            auto st = paris_hip_defect_stats{};
            rt(paris_hip_defect_plan_create(mask->data(), po.det_geo.n_row, po.det_geo.n_col, &plan), "--defects");
            (void)paris_hip_defect_plan_stats(plan, &st);
            (void)paris_hip_defect_plan_destroy(plan);
            po.defect_bytes = static_cast<std::size_t>(st.device_bytes);
            po.defect_mask = std::move(mask);
        }
    }

    namespace detail
    {
        // --bin: checked here, before any device work; 1 x 1 changes nothing. Otherwise the dark and flat means and the defect mask are
        // binned on the host by the rule the device applies to the frames (paris_hip_bin_frame_host, paris_hip_bin_mask), the dead
        // pixels of the SOURCE references (--defects-from-flat: paris_hip_set_flat_field's rule on D and F) join the source mask first,
        // so that they are left out of their bins, and po.det_geo becomes the binned geometry. --defects-from-flat stays on: a binned
        // reference pixel that is dead all the same joins the binned map on each ctx, as without --bin.
        inline auto apply_binning(program_options& po, run_report& r) -> void
        {
            if(po.bin_x == 1u && po.bin_y == 1u)
                return;
            const auto setting = paris_hip_binning{po.bin_x, po.bin_y};
            const auto s_row = po.det_geo.n_row, s_col = po.det_geo.n_col;
            std::uint32_t b_row = 0, b_col = 0;
            if(paris_hip_binning_check(&setting, s_row, s_col, &b_row, &b_col) != PARIS_HIP_SUCCESS)
                throw stage_construction_error{"--bin " + std::to_string(po.bin_x) + ":" + std::to_string(po.bin_y) + ": each factor is 1, 2, 4 or 8 and the "
                                               + std::to_string(s_row) + " x " + std::to_string(s_col) + " detector must hold at least one bin"};
            const auto n_src = static_cast<std::size_t>(s_row) * s_col, n_bin = static_cast<std::size_t>(b_row) * b_col;
            auto mask = std::shared_ptr<std::vector<std::uint8_t>>{};
            if(po.defect_mask || po.defects_from_flat)
                mask = po.defect_mask ? std::make_shared<std::vector<std::uint8_t>>(*po.defect_mask) : std::make_shared<std::vector<std::uint8_t>>(n_src, 0u);
            if(po.defects_from_flat)
                for(std::size_t k = 0; k < n_src; ++k)
                {
                    const double dk = po.dark ? static_cast<double>(po.dark->pixels[k]) : 0.0, fl = static_cast<double>(po.flat->pixels[k]);
                    if(!(fl - dk > 0.0) || !std::isfinite(dk) || !std::isfinite(fl))
                        (*mask)[k] = 1u;
                }
            const auto binned = [&](const std::shared_ptr<const his::mean>& m) -> std::shared_ptr<const his::mean> {
                auto out = std::make_shared<his::mean>();
                out->dim_x = b_row;
                out->dim_y = b_col;
                out->n_frames = m->n_frames;
                out->pixels.resize(n_bin);
                rt(paris_hip_bin_frame_host(&setting, mask ? mask->data() : nullptr, m->pixels.data(), s_row, s_col, out->pixels.data()), "--bin");
                return out;
            };
            if(po.flat)
                po.flat = binned(po.flat);
            if(po.dark)
                po.dark = binned(po.dark);
            if(mask)
            {
                auto small = std::make_shared<std::vector<std::uint8_t>>(n_bin);
                rt(paris_hip_bin_mask(&setting, mask->data(), s_row, s_col, small->data()), "--bin");
                for(const auto b : *small)
                    r.binned_defective += b;
                paris_hip_defect_plan* plan = nullptr;
                auto st = paris_hip_defect_stats{};
                rt(paris_hip_defect_plan_create(small->data(), b_row, b_col, &plan), "--bin");
                (void)paris_hip_defect_plan_stats(plan, &st);
                (void)paris_hip_defect_plan_destroy(plan);
                po.defect_bytes = static_cast<std::size_t>(st.device_bytes);
                po.defect_mask = std::move(small);
                po.bin_mask = std::move(mask);
            }
            auto geo = po.det_geo;
            rt(paris_hip_binned_geometry(&setting, &po.det_geo, &geo), "--bin");
            po.det_geo = geo;
            po.src_row = s_row;
            po.src_col = s_col;
            r.binning = true;
            r.bin_x = po.bin_x;
            r.bin_y = po.bin_y;
            r.src_row = s_row;
            r.src_col = s_col;
            r.binned_row = b_row;
            r.binned_col = b_col;
        }

        // What every pre-pass keeps on the first device while it reads the scan: a ctx, the chain's settings up to the zinger filter
        // (set_frame_chain) -- with `whole`, those behind it as well (set_chain_back) and, with a roll, the slots' second frames --, one
        // group of slots, the chain, and the row plan of `band`. A pre-pass declares its own device buffers after the scope, so that
        // they are freed before the slots and the ctx; everything is gone when the scope ends, before run() plans the slabs.
        struct prepass_scope
        {
            prepass_scope(const program_options& po, bool whole, row_range band)
            : rep{settings(ctx, po, whole)}, slots{ctx, po, slot_shape(po).first, 0u, whole && po.roll, false}, chain{ctx, po, slots, rep.defect_map}
            {
                const auto roll = paris_hip_detector_roll{po.roll_deg};
                rows = plan_frame_rows(band, po.det_geo.n_col, rep.defects.reach_rows, po.zingers, po.air ? &po.air_region : nullptr,
                                       po.binning() ? po.bin_y : 1u, whole && po.roll ? &roll : nullptr, &po.det_geo);
            }

            const device_ctx ctx{0};
            const device_report rep;
            const frame_slots slots;
            const frame_chain chain;
            frame_rows rows;

        private:
            static auto settings(paris_hip_ctx* ctx, const program_options& po, bool whole) -> device_report
            {
                auto rep = device_report{};
                set_frame_chain(ctx, po, rep);
                if(whole)
                    set_chain_back(ctx, po, rep);
                return rep;
            }
        };

        // a group of frames the walk has read into slots 0 .. count - 1: `first` frames came before it; each frame's metadata; and,
        // where the pre-pass asked for them, each frame's angle [deg] with its sine and cosine (paris_hip_stage_angle)
        struct scan_group
        {
            std::uint32_t first, count;
            frame_info* infos;
            const float *angles, *sines, *cosines;
        };

        // One pass over the scan for a pre-pass, in groups of po.batch frames as the main loop groups them: every projection the run
        // uses is read as stored, at the source size, over the plan's source rows, into the scope's pinned slots. each_frame(slot, info)
        // is called for every frame read, each_group(scan_group) for every group; the walk then synchronizes, so that the group's
        // pinned buffers and device frames are free again. With --lag the walk is a sequence of its own, from frame 0 of the file, for
        // the rows the plan uploads. Returns the number of frames. (The main loop's feed, frame_feed, reads ahead on a thread of its
        // own and is not this.)
        template<class Frame, class Group>
        inline auto walk_scan(const prepass_scope& s, const program_options& po, bool with_angles, Frame&& each_frame, Group&& each_group) -> std::uint32_t
        {
            const auto n_row = po.det_geo.n_row, n_col = po.det_geo.n_col;
            const auto sn_row = po.binning() ? po.src_row : n_row, sn_col = po.binning() ? po.src_col : n_col;
            const std::uint32_t batch = slot_shape(po).first;
            auto infos = std::vector<frame_info>(batch);
            auto angles = std::vector<float>(batch), sines = std::vector<float>(batch), cosines = std::vector<float>(batch);
            auto source = frame_stream{po.input_path, po.enable_angles, po.angle_path, po.quality};
            if(po.lag)
                rt(paris_hip_lag_begin(s.ctx, n_row, n_col, s.rows.up.first, s.rows.up.count), "lag_begin()");
            std::uint32_t frames = 0;
            for(bool more = true; more;)
            {
                std::uint32_t filled = 0;
                for(; filled < batch; ++filled)
                {
                    auto& p = infos[filled];
                    p = source.next_raw(s.slots.host(filled), sn_row, sn_col, s.rows.src.first, s.rows.src.count);
                    if(!p.valid())
                    {
                        more = false;
                        break;
                    }
                    if(p.dim_x != sn_row || p.dim_y != sn_col)
                        throw stage_runtime_error{"projection size does not match the detector geometry"};
                    if(with_angles)
                    {
                        angles[filled] = po.enable_angles ? p.phi : static_cast<float>(p.idx) * po.det_geo.delta_phi;
                        rt(paris_hip_stage_angle(&po.det_geo, p.idx, po.enable_angles, p.phi, &sines[filled], &cosines[filled]), "angle");
                    }
                    each_frame(filled, p);
                }
                if(filled == 0)
                    break;
                each_group(scan_group{frames, filled, infos.data(), angles.data(), sines.data(), cosines.data()});
                rt(paris_hip_ctx_synchronize(s.ctx), "synchronize");
                frames += filled;
            }
            if(po.lag)
                rt(paris_hip_lag_end(s.ctx), "lag_end()");
            return frames;
        }

        // --rings and --find-axis: the pre-pass. Every projection the run uses goes through the chain the reconstruction uses, as far
        // as the zinger filter (frame_chain: upload() and clean()), into the ring profile (rings), into the axis search's sinogram
        // (axis), or into both. With rings the frames are read whole; for the axis alone only the search's band of rows, widened by
        // the row plan as a slab's band is. Then the ring rule makes the correction frame, which is kept in po, and the search gives
        // its estimate, which is kept in r.
        inline auto prepass(program_options& po, run_report& r, bool rings, bool axis, bool roll = false) -> void
        {
            const bool profile = rings || roll; // --find-roll scores the scan mean, which the ring profile makes
            const auto t_start = clock::now();
            const auto n_row = po.det_geo.n_row, n_col = po.det_geo.n_col;
            const auto search = paris_hip_axis_search{po.axis_lo, po.axis_step, po.axis_count, po.axis_rows, 0u};
            {
                // the rows of every frame that are filtered and consumed: all of them, or the search's band; the plan widens them.
                // (--bin: the profile is taken on binned frames; the source frames go through the slots' full-width frames)
                auto band = row_range{0u, n_col};
                if(axis && !profile)
                {
                    rt(paris_hip_axis_search_check(&search, &po.det_geo, po.axis_frames, &band.first, nullptr), "axis_search_check()");
                    band.count = po.axis_rows;
                }
                const prepass_scope s{po, false, band};
                const auto& ctx = s.ctx;
                if(profile)
                    rt(paris_hip_ring_profile_begin(ctx, n_row, n_col), "ring_profile_begin()");
                if(axis)
                    rt(paris_hip_axis_search_begin(ctx, &search, &po.det_geo, po.axis_frames), "axis_search_begin()");
                const auto frames = walk_scan(
                    s, po, false, [&](std::uint32_t slot, const frame_info& p) { s.chain.upload(slot, p.pixel, s.rows); },
                    [&](const scan_group& g) {
                        if(axis && g.count > po.axis_frames - g.first)
                            throw stage_runtime_error{"--find-axis: the input holds more frames than were counted"};
                        s.chain.clean(0u, g.count, true, s.rows);
                        if(profile)
                            rt(paris_hip_ring_profile_add_rows(ctx, s.slots.frame(0u), s.slots.pitch, s.slots.stride, g.count, n_row, n_col, 0u, n_col),
                               "ring_profile_add_rows()");
                        if(axis)
                            rt(paris_hip_axis_search_add_rows(ctx, s.slots.frame(0u), s.slots.pitch, s.slots.stride, g.count, n_row, n_col, g.first),
                               "axis_search_add_rows()");
                    });
                if(po.air)
                    rt(paris_hip_air_stats(ctx, &r.air_prepass, 0), "air stats");
                auto mean = std::vector<float>(roll ? static_cast<std::size_t>(n_row) * n_col : 0u); // --find-roll: the scan mean
                if(profile)
                {
                    auto c = std::make_shared<std::vector<float>>(static_cast<std::size_t>(n_row) * n_col);
                    // (without --rings the profile is closed with the smallest valid setting and its correction frame is dropped)
                    const auto setting = rings ? paris_hip_ring_filter{po.ring_half_width, po.ring_floor, po.ring_limit} : paris_hip_ring_filter{1u, 0.f, 0.f};
                    auto unused = paris_hip_ring_stats{};
                    rt(paris_hip_ring_profile_finish(ctx, &setting, c->data(), roll ? mean.data() : nullptr, rings ? &r.rings : &unused), "ring_profile_finish()");
                    if(rings)
                    {
                        for(std::size_t k = 0; k < mean.size(); ++k) // the search sees the mean as the corrected frames will give it
                            mean[k] = mean[k] - (*c)[k];
                        po.ring_c = std::move(c);
                        r.ring_filter = true;
                        r.ring_frames = frames;
                    }
                }
                if(axis)
                {
                    if(frames != po.axis_frames)
                        throw stage_runtime_error{"--find-axis: the input holds fewer frames than were counted"};
                    auto cost = std::vector<double>(po.axis_count);
                    const int rc = paris_hip_axis_search_finish(ctx, cost.data(), nullptr, &r.axis, nullptr);
                    if(rc == PARIS_HIP_ERROR_INVALID_ARGUMENT && r.axis.scored == 0u)
                        throw stage_runtime_error{"--find-axis: no candidate has enough detector columns with a conjugate on the detector"};
                    rt(rc, "axis_search_finish()");
                    r.axis_search = true;
                    r.axis_frames = frames;
                    r.axis_count = po.axis_count;
                }
                if(roll) // after the axis search: the mirror line is the axis just found
                {
                    auto geo = po.det_geo;
                    if(axis)
                        geo.delta_s = r.axis.delta_s;
                    const auto roll_search = paris_hip_roll_search{po.roll_lo, po.roll_step, po.roll_count, 0u};
                    auto cost = std::vector<double>(po.roll_count);
                    const int rc = paris_hip_roll_search_run(ctx, &roll_search, &geo, mean.data(), cost.data(), nullptr, &r.roll);
                    if(rc == PARIS_HIP_ERROR_INVALID_ARGUMENT && r.roll.scored == 0u)
                        throw stage_runtime_error{"--find-roll: no candidate has enough finite pixel pairs inside the margins"};
                    rt(rc, "roll_search()");
                    r.roll_search = true;
                    r.roll_frames = frames;
                    r.roll_count = po.roll_count;
                }
            } // (the buffers and the ctx are gone: the times below include that)
            if(roll)
                r.roll_prepass_s = since(t_start);
            if(rings)
                r.ring_prepass_s = since(t_start);
            if(axis)
                r.axis_prepass_s = since(t_start);
        }

        // --fit-beam-hardening: the pre-pass, after the ring pre-pass and the axis search, whose results it uses. Every projection is
        // read whole; each group goes N times through the main loop's frame stages -- the raw upload (corrected with --flat), the air
        // normalisation, the defect repair, the zinger filter, the ring correction -- then, the k-th time, through the pass with the
        // unit setting e_k, the redundancy weights, weight + filter and the backprojection into the k-th basis slab: the central
        // po.bh_slices slices of the whole volume. (The group is uploaded again for each k from the pinned frames, which are read once:
        // no device copy of it is kept.) Then threshold, labels, Gram sums and the solve.
        inline auto bh_prepass(const program_options& po, run_report& r) -> void
        {
            const auto t_start = clock::now();
            const auto n_row = po.det_geo.n_row, n_col = po.det_geo.n_col;
            const auto& vg = r.vol_geo;
            const std::uint32_t degree = po.bh.degree, slices = po.bh_slices, z_first = (vg.dim_z - slices) / 2u;
            {
                // whole frames: every range of the plan is the detector. (No polynomial and no roll yet: check_beam_hardening, check_roll)
                const prepass_scope s{po, true, row_range{0u, n_col}};
                const auto& ctx = s.ctx;
                const auto& slots = s.slots;
                struct fit_buffers // the basis slabs and the labels
                {
                    paris_hip_ctx* ctx;
                    float* d_slab[PARIS_HIP_BH_DEGREE_MAX];
                    std::uint8_t* d_labels;
                    ~fit_buffers()
                    {
                        for(auto d : d_slab)
                            paris_hip_free(ctx, d);
                        paris_hip_free(ctx, d_labels);
                    }
                } fit{ctx, {nullptr, nullptr, nullptr, nullptr}, nullptr};
                for(std::uint32_t k = 0; k < degree; ++k)
                    rt(paris_hip_malloc_volume(ctx, vg.dim_x, vg.dim_y, slices, &fit.d_slab[k]), "make_volume()");
                {
                    float* words = nullptr; // the labels: one byte per voxel, in memory of the volume allocator
                    const auto voxels = static_cast<std::uint64_t>(vg.dim_x) * vg.dim_y * slices;
                    if((voxels + 3u) / 4u > 0xffffffffull)
                        throw stage_construction_error{"--fit-beam-hardening: the slab holds too many voxels"};
                    rt(paris_hip_malloc_volume(ctx, static_cast<std::uint32_t>((voxels + 3u) / 4u), 1u, 1u, &words), "make_volume()");
                    fit.d_labels = reinterpret_cast<std::uint8_t*>(words);
                }
                const float delta_s = po.det_geo.delta_s * po.det_geo.l_px_row, delta_t = po.det_geo.delta_t * po.det_geo.l_px_col;
                const auto no_roi = region_of_interest{};
                const auto frames = walk_scan(s, po, true, [](std::uint32_t, const frame_info&) {}, [&](const scan_group& g) {
                    if(po.lag)
                    {
                        // The group goes through the stages once per basis, but the sequence's state must see every frame once: the
                        // counts are corrected once, in time order, and the pinned frames (a slot holds 4 bytes per pixel) are replaced
                        // by the corrected counts as f32, which every basis then uploads (chain.upload: lag already applied).
                        for(std::uint32_t f = 0; f < g.count; ++f)
                            rt(paris_hip_upload_projection_raw(ctx, slots.frame(f), slots.pitch, slots.host(f), n_row * his::pixel_size(g.infos[f].pixel), n_row,
                                                               n_col, g.infos[f].pixel), "load()");
                        rt(paris_hip_lag_correct_rows(ctx, slots.frame(0u), slots.pitch, slots.stride, g.count, n_row, n_col, 0u, n_col), "lag correction");
                        for(std::uint32_t f = 0; f < g.count; ++f)
                        {
                            rt(paris_hip_memcpy_projection_d2h(ctx, slots.host(f), n_row * sizeof(float), slots.frame(f), slots.pitch, n_row, n_col), "copy_d2h()");
                            g.infos[f].pixel = his::pixel_f32;
                        }
                        rt(paris_hip_ctx_synchronize(ctx), "synchronize");
                    }
                    for(std::uint32_t k = 0; k < degree; ++k)
                    {
                        for(std::uint32_t f = 0; f < g.count; ++f)
                            s.chain.upload(f, g.infos[f].pixel, s.rows, true);
                        auto unit = paris_hip_beam_hardening{};
                        unit.degree = k + 1u;
                        unit.c[k] = 1.f;
                        s.chain.clean(0u, g.count, true, s.rows);
                        s.chain.linearise(0u, g.count, true, s.rows, &unit);
                        s.chain.finish(0u, g.count, true, s.rows, g.angles);
                        rt(paris_hip_backproject_batch(ctx, slots.out(0u), slots.pitch, slots.stride, g.count, n_row, n_col, fit.d_slab[k], vg.dim_x, vg.dim_y, slices,
                                                       z_first, &po.det_geo, &vg, 0, &no_roi, g.sines, g.cosines, delta_s, delta_t), "backproject()");
                        if(k + 1u < degree) // the device frames are free for the next basis (after the last one the walk synchronizes)
                            rt(paris_hip_ctx_synchronize(ctx), "synchronize");
                    }
                });
                if(frames == 0u)
                    throw stage_runtime_error{"--fit-beam-hardening: the input holds no projection"};
                const auto voxels = static_cast<std::uint64_t>(vg.dim_x) * vg.dim_y * slices;
                auto stats = paris_hip_volume_statistics{};
                rt(paris_hip_volume_stats(ctx, fit.d_slab[0], voxels, 0.f, 0.f, 0u, nullptr, &stats), "volume_stats()");
                auto hist = std::vector<std::uint64_t>(PARIS_HIP_BH_HISTOGRAM_BINS);
                if(paris_hip_volume_stats(ctx, fit.d_slab[0], voxels, stats.min, stats.max, PARIS_HIP_BH_HISTOGRAM_BINS, hist.data(), &stats) != PARIS_HIP_SUCCESS
                   || paris_hip_bh_threshold_from_histogram(hist.data(), PARIS_HIP_BH_HISTOGRAM_BINS, stats.min, stats.max, &r.bh_threshold) != PARIS_HIP_SUCCESS)
                    throw stage_runtime_error{"--fit-beam-hardening: the reconstruction of the scan has no range of values to take a threshold from"};
                rt(paris_hip_bh_classify(ctx, fit.d_slab[0], vg.dim_x, vg.dim_y, slices, r.bh_threshold, po.bh_margin, fit.d_labels), "bh_classify()");
                double gram[(PARIS_HIP_BH_DEGREE_MAX + 1) * (PARIS_HIP_BH_DEGREE_MAX + 2) / 2];
                rt(paris_hip_bh_gram(ctx, fit.d_slab, degree, fit.d_labels, voxels, gram, &r.bh_counts), "bh_gram()");
                rt(paris_hip_bh_solve(gram, degree, &r.bh_counts, 0u, &r.bh_fit), "--fit-beam-hardening: bh_solve()");
                r.bh_fitted = true;
                r.bh_frames = frames;
                r.bh_slice_first = z_first;
                r.bh_slices = slices;
            } // (the buffers and the ctx are gone: the time below includes that)
            r.bh_prepass_s = since(t_start);
        }

        // --metal: the pre-pass, after every other pre-pass, with their results in force (po holds the ring correction, the axis, the
        // polynomial and the roll by now). Every projection is read whole and goes through the main loop's whole frame chain and the
        // backprojection into ONE buffer that holds the whole grid; each frame's sine and cosine are kept. Then the voxels above the
        // threshold are collected and the volume binarized, the mask is forward-projected group by group into the slots' frames, and
        // each group packed to the host.
        inline auto metal_prepass(program_options& po, run_report& r) -> void
        {
            const auto t_start = clock::now();
            const auto n_row = po.det_geo.n_row, n_col = po.det_geo.n_col;
            const auto& vg = r.vol_geo;
            const std::uint32_t batch = slot_shape(po).first;
            const std::uint32_t words = (n_row + 63u) / 64u;
            const auto voxels = static_cast<std::uint64_t>(vg.dim_x) * vg.dim_y * vg.dim_z;
            std::uint64_t cap = 0;
            if(paris_hip_metal_check(vg.dim_x, vg.dim_y, vg.dim_z, po.metal_threshold, po.metal_grow, po.metal_min_path, &cap) != PARIS_HIP_SUCCESS)
                throw stage_construction_error{"--metal: the library refuses the setting"};
            {
                std::size_t free_b = 0, total_b = 0;
                rt(paris_hip_device_memory(0, &free_b, &total_b), "device memory");
                const auto need = voxels * sizeof(float) + driver_bytes(po);
                if(need > free_b)
                    throw stage_construction_error{"--metal: the pre-pass needs the whole volume and its frame slots on one device, " + std::to_string(need)
                                                   + " bytes, and " + std::to_string(free_b) + " are free: try --bin"};
            }
            auto bits = std::make_shared<std::vector<std::uint64_t>>();
            auto index = std::make_shared<std::vector<std::uint64_t>>();
            auto value = std::make_shared<std::vector<float>>();
            std::uint32_t frames = 0, n_views = 0;
            {
                // whole frames: every range of the plan is the detector. (No trace and no list yet)
                const prepass_scope s{po, true, row_range{0u, n_col}};
                const auto& ctx = s.ctx;
                const auto& slots = s.slots;
                struct whole_volume
                {
                    paris_hip_ctx* ctx;
                    float* d_v;
                    ~whole_volume() { paris_hip_free(ctx, d_v); }
                } vol{ctx, nullptr};
                rt(paris_hip_malloc_volume(ctx, vg.dim_x, vg.dim_y, vg.dim_z, &vol.d_v), "make_volume()");
                const float delta_s = po.det_geo.delta_s * po.det_geo.l_px_row, delta_t = po.det_geo.delta_t * po.det_geo.l_px_col;
                const auto no_roi = region_of_interest{};
                auto all_sin = std::vector<float>{}, all_cos = std::vector<float>{}; // per view, for the forward projection
                const std::uint32_t stride = std::max<std::uint32_t>(1u, po.quality);
                frames = walk_scan(
                    s, po, true, [&](std::uint32_t slot, const frame_info& p) { s.chain.upload(slot, p.pixel, s.rows); },
                    [&](const scan_group& g) {
                        for(std::uint32_t f = 0; f < g.count; ++f)
                        {
                            const std::uint32_t view = g.infos[f].idx / stride;
                            if(view >= all_sin.size())
                            {
                                all_sin.resize(view + 1u, 0.f);
                                all_cos.resize(view + 1u, 1.f);
                            }
                            all_sin[view] = g.sines[f];
                            all_cos[view] = g.cosines[f];
                        }
                        s.chain.run(0u, g.count, true, s.rows, g.angles);
                        rt(paris_hip_backproject_batch(ctx, slots.out(0u), slots.pitch, slots.stride, g.count, n_row, n_col, vol.d_v, vg.dim_x, vg.dim_y, vg.dim_z, 0u,
                                                       &po.det_geo, &vg, 0, &no_roi, g.sines, g.cosines, delta_s, delta_t), "backproject()");
                    });
                if(frames == 0u)
                    throw stage_runtime_error{"--metal: the input holds no projection"};
                n_views = static_cast<std::uint32_t>(all_sin.size());
                // the list: counted first, so that the host arrays hold what is there and not what the cap allows
                std::uint64_t n = 0;
                const int counted = paris_hip_metal_collect(ctx, vol.d_v, vg.dim_x, vg.dim_y, vg.dim_z, po.metal_threshold, 0u, nullptr, nullptr, &n, 0);
                if(counted != PARIS_HIP_SUCCESS && counted != PARIS_HIP_ERROR_METAL_TOO_MANY_VOXELS)
                    rt(counted, "metal_collect()");
                if(n > cap)
                    throw stage_runtime_error{"--metal: " + std::to_string(n) + " voxel(s) lie above the threshold, more than 1/32 of the grid ("
                                              + std::to_string(cap) + "): that is a wrong threshold, not metal"};
                index->resize(n);
                value->resize(n);
                rt(paris_hip_metal_collect(ctx, vol.d_v, vg.dim_x, vg.dim_y, vg.dim_z, po.metal_threshold, n, index->data(), value->data(), &n, 1),
                   "metal_collect()");
                // the mask's projections, in groups of the slots, packed to the host
                bits->assign(static_cast<std::size_t>(n_views) * n_col * words, 0u);
                for(std::uint32_t v0 = 0; v0 < n_views; v0 += batch)
                {
                    const std::uint32_t nv = std::min(batch, n_views - v0);
                    rt(paris_hip_forward_project(ctx, vol.d_v, vg.dim_x, vg.dim_y, vg.dim_z, 0u, &po.det_geo, &vg, slots.frame(0u), slots.pitch, slots.stride, nv,
                                                 n_row, n_col, all_sin.data() + v0, all_cos.data() + v0, delta_s, delta_t, 0), "forward_project()");
                    rt(paris_hip_metal_trace_pack(ctx, slots.frame(0u), slots.pitch, slots.stride, nv, n_row, n_col, po.metal_min_path, po.metal_grow,
                                                  bits->data() + static_cast<std::size_t>(v0) * n_col * words), "metal_trace_pack()");
                }
            } // (the buffers and the ctx are gone: the time below includes that)
            std::uint64_t pixels = 0;
            for(const auto w : *bits)
                pixels += static_cast<std::uint64_t>(__builtin_popcountll(w));
            po.metal_views = n_views;
            po.metal_bytes = 64u + bits->size() * sizeof(std::uint64_t) + index->size() * (sizeof(std::uint64_t) + sizeof(float));
            r.metal = true;
            r.metal_threshold = po.metal_threshold;
            r.metal_grow = po.metal_grow;
            r.metal_min_path = po.metal_min_path;
            r.metal_frames = frames;
            r.metal_voxels = index->size();
            r.metal_trace_pixels = pixels;
            po.metal_bits = std::move(bits);
            po.metal_index = std::move(index);
            po.metal_value = std::move(value);
            r.metal_prepass_s = since(t_start);
        }
    }

    // src/main.cpp:120-178
    inline auto run(const program_options& requested) -> run_report
    {
        auto po = requested; // batch may shrink to fit the devices' memory (detail::fit_batch)
        auto r = run_report{};
        const auto start = detail::clock::now();
        detail::check_lag(po);
        detail::load_flat_field(po);
        r.flat_frames = po.flat ? po.flat->n_frames : 0u;
        r.dark_frames = po.dark ? po.dark->n_frames : 0u;
        detail::load_defects(po);
        detail::apply_binning(po, r); // from here on po.det_geo is the binned detector
        detail::check_air_region(po);
        if(po.air) // the frame the rectangle was checked against
        {
            r.air_row = po.det_geo.n_row;
            r.air_col = po.det_geo.n_col;
        }
        detail::check_zingers(po);
        detail::check_extend_rows(po);
        detail::check_rings(po);
        detail::check_voxels(po);
        detail::check_axis(po);
        detail::check_starvation(po);
        detail::check_scatter(po);
        detail::check_phase(po);
        detail::check_beam_hardening(po);
        detail::check_roll(po);
        detail::check_metal(po);
        detail::check_denoise(po);
        // --find-roll: the estimate becomes the run's roll (an estimate of exactly 0 is no roll)
        const auto adopt_roll = [&] {
            po.roll_deg = r.roll.eta_deg;
            po.roll = po.roll_deg != 0.f;
        };
        if(po.find_axis)
        {
            // before anything is derived from delta_s: the offset-detector check, the short-scan check and the volume geometry below
            // are those of the found axis. The pre-pass sizes its groups as the run will (the slot frames do not depend on delta_s).
            int n_pre = 0;
            detail::rt(paris_hip_device_count(&n_pre), "get_devices()");
            if(n_pre == 0)
                throw stage_construction_error{"no HIP device"};
            auto pre = detail::fit_batch(po, po.devices > 0 && po.devices < n_pre ? po.devices : n_pre);
            detail::prepass(pre, r, po.rings, true, po.find_roll);
            po.ring_c = pre.ring_c;
            if(po.find_roll)
                adopt_roll();
            r.axis_given = po.det_geo.delta_s;
            po.det_geo.delta_s = r.axis.delta_s;
            if(po.axis_only || po.roll_only)
            {
                r.wall_s = detail::since(start);
                return r;
            }
        }
        if(po.offset_detector)
            detail::check_offset_detector(po);
        if(po.short_scan)
            po.scan = detail::derive_short_scan(po);
        r.vol_geo = calculate_volume_geometry(po.det_geo); // :122
        r.roi_geo = r.vol_geo;
        if(po.enable_roi)                                  // :124-130
            r.roi_geo = apply_roi(r.vol_geo, po.roi.x1, po.roi.x2, po.roi.y1, po.roi.y2, po.roi.z1, po.roi.z2);
        if(po.fit_beam_hardening && po.bh_slices > r.vol_geo.dim_z)
            throw stage_construction_error{"--fit-beam-hardening: the volume has " + std::to_string(r.vol_geo.dim_z) + " slice(s), fewer than the "
                                           + std::to_string(po.bh_slices) + " asked for"};

        r.denoise = po.denoise;
        r.denoise_setting = po.denoise_setting;
        if(po.denoise) // beside a slab: its 2 RADIUS halo slices, the drain ctx's scratch of one chunk of floats (a slice at least) and its tables
        {
            const auto slice = static_cast<std::size_t>(r.roi_geo.dim_x) * r.roi_geo.dim_y * sizeof(float);
            const std::size_t voxel_bytes = po.voxels.type == 0 ? sizeof(float) : (po.voxels.type == PARIS_HIP_VOXEL_U8 ? 1u : 2u);
            const auto side = static_cast<std::size_t>(2u * po.denoise_setting.radius + 1u);
            po.denoise_bytes = 2u * po.denoise_setting.radius * slice + std::max(slice, po.drain_chunk_bytes / voxel_bytes * sizeof(float))
                               + sizeof(float) * (PARIS_HIP_BILATERAL_BINS + side * side * side);
        }
        int n_dev = 0;
        detail::rt(paris_hip_device_count(&n_dev), "get_devices()"); // :145
        if(n_dev == 0)
            throw stage_construction_error{"no HIP device"};
        if(po.devices > 0 && po.devices < n_dev)
            n_dev = po.devices;
        if(po.voxels.automatic && n_dev != 1)
            throw stage_construction_error{"--voxel-range auto needs the whole volume in one slab on one device: give --devices 1 (" + std::to_string(n_dev)
                                           + " devices would be used)"};
        po = detail::fit_batch(po, n_dev);
        r.batch = po.batch;
        if((po.rings || po.find_roll) && !po.find_axis) // before the slabs are planned: the pre-pass's buffers are gone by then, the correction frame is in the reserve
        {
            detail::prepass(po, r, po.rings, false, po.find_roll);
            if(po.find_roll)
                adopt_roll();
            if(po.roll_only)
            {
                r.wall_s = detail::since(start);
                return r;
            }
        }
        if(po.fit_beam_hardening) // after the ring pre-pass and the axis search, whose results it uses; its slabs are gone before the run's are planned
        {
            detail::bh_prepass(po, r);
            po.bh = r.bh_fit.setting;
            po.beam_hardening = true;
        }
        r.beam_hardening = po.beam_hardening;
        r.bh = po.bh;
        if(po.metal) // after every other pre-pass, whose results it uses; its volume is gone before the run's slabs are planned
        {
            if(po.metal_min_path < 0.f) // not given: half the smallest voxel edge
                po.metal_min_path = 0.5f * std::min(r.vol_geo.l_vx_x, std::min(r.vol_geo.l_vx_y, r.vol_geo.l_vx_z));
            detail::metal_prepass(po, r);
        }
        r.starvation = po.starvation;
        r.starvation_setting = po.starvation_setting;
        r.scatter = po.scatter;
        r.scatter_setting = po.scatter_setting;
        r.scatter_l_x = po.det_geo.l_px_row;
        r.scatter_l_y = po.det_geo.l_px_col;
        r.scatter_nx = po.scatter_nx;
        r.scatter_ny = po.scatter_ny;
        r.scatter_scratch = po.scatter_scratch;
        r.phase = po.phase;
        r.phase_setting = po.phase_setting;
        r.phase_l_x = po.det_geo.l_px_row;
        r.phase_l_y = po.det_geo.l_px_col;
        r.phase_nx = po.phase_nx;
        r.phase_ny = po.phase_ny;
        r.phase_scratch = po.phase_scratch;
        r.detector_roll = po.roll;
        r.roll_deg = po.roll_deg;
        r.lag = po.lag;
        r.lag_model = po.lag_model;
        if(po.lag)
        {
            float g[4], c[4], w[4];
            detail::rt(paris_hip_lag_coefficients(&po.lag_model, g, c, w, nullptr, &r.lag_b0), "lag_coefficients()");
        }

        if(po.slabs > 0) // fixed split (src/cuda/subvolume_information.cpp:112-116 with a given count)
        {
            const auto num = static_cast<std::uint32_t>(po.slabs) > r.roi_geo.dim_z ? r.roi_geo.dim_z : static_cast<std::uint32_t>(po.slabs);
            r.info.num = static_cast<int>(num);
            r.info.geo = {r.roi_geo.dim_x, r.roi_geo.dim_y, r.roi_geo.dim_z / num, r.roi_geo.dim_z % num};
        }
        else // :137, with the driver's own per-device buffers charged next to the slab
        {
            detail::rt(paris_hip_make_subvolume_information_reserving(&r.roi_geo, &po.det_geo, n_dev, detail::driver_bytes(po), &r.info),
                       "make_subvolume_information()");
            // The volume fits (one slab per device): nothing of it could reach the file before the last projection is in. Thinner
            // slabs, several per device, let the drain thread write slab k while slab k + 1 is reconstructed (two volume buffers:
            // they fit where the one big slab did); each slab only reads its own detector rows, so the extra passes over the
            // projections cost little (row band, f4).
            const auto per = static_cast<std::uint32_t>(po.pipeline_slabs > 0 ? po.pipeline_slabs : 0);
            const auto slab_bytes = static_cast<std::uint64_t>(r.info.geo.dim_x) * r.info.geo.dim_y * r.info.geo.dim_z * sizeof(float);
            if(po.two_volumes && po.row_band && per > 1u && r.info.num == n_dev && slab_bytes >= (std::uint64_t{1} << 30)
               && r.info.geo.dim_z >= 32u * per)
            {
                const auto num = static_cast<std::uint32_t>(n_dev) * per;
                r.info.num = static_cast<int>(num);
                r.info.geo = {r.roi_geo.dim_x, r.roi_geo.dim_y, r.roi_geo.dim_z / num, r.roi_geo.dim_z % num};
            }
        }

        task_queue queue{make_tasks(po, r.vol_geo, r.info)}; // :140-141
        sink out{po.output_path, po.prefix, r.roi_geo, po.voxels.type == 0 ? 0u : (po.voxels.type == PARIS_HIP_VOXEL_U8 ? 1u : 2u)}; // :154
        r.output_file = out.file_path();
        if(po.voxels.type != 0 && !po.voxels.automatic)
            out.set_window(po.voxels.lo, po.voxels.hi); // (with auto the drain thread does, once it has chosen the window)

        if(n_dev > 1) // :157-167
        {
            // Where the frames come from. Every device thread needs every projection, but with the row band (f4) only the detector
            // rows its slab can read: z-slabs of one pass over the queue need little more than one detector's worth of rows between
            // them, and a stream per thread that reads and converts just its band does less work per frame than one whole-frame
            // conversion plus a band copy per thread, with nothing shared to wait for (8 bands of a 2048^2 frame: 0.67 against
            // 1.8 ms per frame on 8 cores, tools/shared_source_bench.py). Bands that overlap widely (no row band, thick cones, few
            // rows: the pass would read the files more than twice over) are read once and shared instead.
            const auto first_pass = std::min<std::uint32_t>(static_cast<std::uint32_t>(n_dev), static_cast<std::uint32_t>(r.info.num));
            if(po.row_band && po.det_geo.n_col != 0)
            {
                std::uint64_t rows = 0;
                for(std::uint32_t i = 0; i < first_pass; ++i)
                {
                    const bool last = i + 1u == static_cast<std::uint32_t>(r.info.num);
                    std::uint32_t band_first = 0, band_count = po.det_geo.n_col;
                    detail::rt(paris_hip_slab_row_band(&po.det_geo, &r.vol_geo, r.info.geo.dim_x, r.info.geo.dim_y,
                                                       r.info.geo.dim_z + (last ? r.info.geo.remainder : 0u), i * r.info.geo.dim_z, po.enable_roi,
                                                       &po.roi, &band_first, &band_count), "slab_row_band()");
                    rows += band_count;
                }
                r.rows_per_pass = static_cast<double>(rows) / po.det_geo.n_col;
            }
            else
                r.rows_per_pass = static_cast<double>(first_pass);
            r.shared_source = po.share_frames < 0 ? r.rows_per_pass > 2.0 : po.share_frames != 0;
            // every HIS frame is read once per pass, not once per device (with --bin: at the source detector's size)
            frame_pool pool{n_dev, po.binning() ? po.src_row : po.det_geo.n_row, po.binning() ? po.src_col : po.det_geo.n_col};
            auto* shared = r.shared_source ? &pool : nullptr;
            auto futures = std::vector<std::future<device_report>>{};
            for(int d = 0; d < n_dev; ++d)
                futures.emplace_back(std::async(std::launch::async, [&queue, &out, &po, shared, d] { return reconstruct(queue, d, out, po, shared); }));
            for(auto& f : futures)
                r.devices.push_back(f.get());
            if(r.shared_source)
            {
                const auto st = pool.stats();
                r.frames_read = st.produced + st.reread;
                r.frames_requested = st.served + st.reread;
                r.skipped = pool.skipped_files();
            }
        }
        else
            r.devices.push_back(reconstruct(queue, 0, out, po)); // :169
        r.defect_map = r.devices.front().defect_map; // (every device sets the same map)
        r.defects = r.devices.front().defects;
        for(const auto& d : r.devices)
        {
            r.row_extension = r.row_extension || d.row_extension;
            r.zinger_filter = r.zinger_filter || d.zinger_filter;
            r.air_region = r.air_region || d.air_region;
            r.air.frames += d.air.frames;
            r.air.normalised += d.air.normalised;
            r.air.too_few += d.air.too_few;
            r.air.above_limit += d.air.above_limit;
            r.air.min_a = &d == &r.devices.front() ? d.air.min_a : std::min(r.air.min_a, d.air.min_a);
            r.air.max_a = &d == &r.devices.front() ? d.air.max_a : std::max(r.air.max_a, d.air.max_a);
            r.zingers.frames += d.zingers.frames;
            r.zingers.replaced += d.zingers.replaced;
            r.zingers.saturated_frames += d.zingers.saturated_frames;
            r.metal_counts.replaced += d.metal.replaced;
            r.metal_counts.runs += d.metal.runs;
            r.metal_counts.rows_left += d.metal.rows_left;
            r.starvation_counts.frames += d.starvation.frames;
            r.starvation_counts.filtered += d.starvation.filtered;
            r.starvation_counts.last_level += d.starvation.last_level;
            r.voxels.voxels += d.voxels.voxels;
            r.voxels.below += d.voxels.below;
            r.voxels.above += d.voxels.above;
            r.voxels.not_finite += d.voxels.not_finite;
        }
        r.starvation_pixels = r.starvation_counts.frames * po.det_geo.n_row * po.det_geo.n_col;
        r.voxel_type = po.voxels.type;
        if(po.voxels.type != 0)
            out.window(r.voxel_lo, r.voxel_hi);
        r.wall_s = detail::since(start);
        return r;
    }
}

#endif
