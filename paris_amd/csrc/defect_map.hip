// Repair of defective detector pixels for gfx950 (the statement is in include/paris_hip.h).
//
// The ctx holds one setting: the plan defect_plan.cpp builds on the host from the map, copied as it is into one device buffer by
// paris_hip_set_defect_map. The repair (paris_hip_defect_repair_rows) is one sparse launch: one lane per (defect of the band, frame),
// defects on grid x, frames on grid z; a lane walks its own sources and stores one pixel. Sources are good pixels, destinations are
// defective ones, so lanes never read what another lane writes: in place, no races, idempotent.
// The launch moves a few bytes per defect -- a 2048^2 detector with a dead row, a dead column and 0.1 % scattered pixels has about
// 8 000 defects -- so it is sized by latency, not bandwidth: nothing here is tuned beyond the block size.
#include <algorithm>

#include "defect_plan.h"
#include "frame_pass.h"

namespace
{
    constexpr uint32_t DM_THREADS = 256u;
    constexpr uint32_t DM_MAX_FRAMES = 65535u;    // grid z
    constexpr uint32_t DM_MAX_BLOCKS = 0x7fffffffu; // grid x

    // p: the first frame's base (row 0) of this launch; rows pitch_f floats apart, frames frame_stride bytes apart (grid z).
    // Defects [k_first, k_end) of the sorted list; a pixel index is y * dim_x + x.
    __global__ void __launch_bounds__(DM_THREADS)
        defect_repair_kernel(char* p, size_t frame_stride, size_t pitch_f, uint32_t dim_x, const uint32_t* __restrict__ defect,
                             const uint32_t* __restrict__ first_source, const uint32_t* __restrict__ source,
                             const float* __restrict__ weight, uint32_t k_first, uint32_t k_end)
    {
        const uint64_t k = static_cast<uint64_t>(k_first) + static_cast<uint64_t>(blockIdx.x) * DM_THREADS + threadIdx.x;
        if(k >= k_end)
            return;
        float* frame = reinterpret_cast<float*>(p + static_cast<size_t>(blockIdx.z) * frame_stride);
        float acc = 0.f;
        for(uint32_t s = first_source[k], e = first_source[k + 1u]; s < e; ++s)
        {
            const uint32_t i = source[s];
            const uint32_t sy = i / dim_x, sx = i - sy * dim_x;
            acc = __builtin_fmaf(weight[s], frame[static_cast<size_t>(sy) * pitch_f + sx], acc);
        }
        const uint32_t q = defect[k];
        const uint32_t y = q / dim_x, x = q - y * dim_x;
        frame[static_cast<size_t>(y) * pitch_f + x] = acc;
    }
}

extern "C" int paris_hip_set_defect_map(paris_hip_ctx* ctx, const uint8_t* mask, uint32_t dim_x, uint32_t dim_y)
{
    if(int rc = paris_hip_bind(ctx))
        return rc;
    if(mask == nullptr || dim_x == 0 || dim_y == 0)
        return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    paris_hip_defect_plan* plan = nullptr;
    if(int rc = paris_hip_defect_plan_create(mask, dim_x, dim_y, &plan))
        return rc;
    const size_t n = plan->defect.size(), m = plan->source.size();
    paris_hip_device_buffer mem; // (none for a plan without a repairable defect)
    if(n != 0)
    {
        const size_t w = sizeof(uint32_t); // of every entry, the float weights too
        if(int rc = paris_hip_install(ctx, static_cast<size_t>(plan->stats.device_bytes),
                                      {{0u, plan->defect.data(), n * w},
                                       {n * w, plan->first_source.data(), (n + 1u) * w},
                                       {(2u * n + 1u) * w, plan->source.data(), m * w},
                                       {(2u * n + 1u + m) * w, plan->weight.data(), m * w}},
                                      &mem))
        {
            paris_hip_defect_plan_destroy(plan);
            return rc;
        }
    }
    paris_hip_ctx::defect_map_t& dm = ctx->defect_map;
    paris_hip_release(ctx, dm);
    dm.set = true;
    dm.mem = mem;
    dm.dim_x = dim_x;
    dm.dim_y = dim_y;
    dm.n = static_cast<uint32_t>(n);
    dm.m = static_cast<uint32_t>(m);
    dm.stats = plan->stats;
    dm.row_start.swap(plan->row_start);
    paris_hip_defect_plan_destroy(plan);
    return PARIS_HIP_SUCCESS;
}

extern "C" int paris_hip_clear_defect_map(paris_hip_ctx* ctx)
{
    if(int rc = paris_hip_bind(ctx))
        return rc;
    paris_hip_release(ctx, ctx->defect_map);
    return PARIS_HIP_SUCCESS;
}

extern "C" int paris_hip_defect_map_info(paris_hip_ctx* ctx, paris_hip_defect_stats* out)
{
    if(ctx == nullptr || out == nullptr || !ctx->defect_map.set)
        return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    *out = ctx->defect_map.stats;
    return PARIS_HIP_SUCCESS;
}

extern "C" int paris_hip_defect_repair_rows(paris_hip_ctx* ctx, float* d_p, size_t pitch, size_t frame_stride, uint32_t n_frames,
                                            uint32_t dim_x, uint32_t dim_y, uint32_t row_first, uint32_t row_count)
{
    const paris_hip_frame_band band{d_p, pitch, frame_stride, n_frames, dim_x, dim_y, row_first, row_count};
    uint32_t k_first = 0, k_end = 0; // the band's defects in the sorted list
    const auto refuse = [&]() -> int {
        const paris_hip_ctx::defect_map_t& dm = ctx->defect_map;
        return !dm.set || dim_x != dm.dim_x || dim_y != dm.dim_y ? PARIS_HIP_ERROR_INVALID_ARGUMENT : PARIS_HIP_SUCCESS;
    };
    const auto idle = [&] { // (a map without a repairable defect in the band)
        k_first = ctx->defect_map.row_start[row_first];
        k_end = ctx->defect_map.row_start[row_first + row_count];
        return k_first == k_end;
    };
    const auto launch = [&] {
        const paris_hip_ctx::defect_map_t& dm = ctx->defect_map;
        const uint32_t* defect = dm.mem.as<uint32_t>();
        const uint32_t* first_source = defect + dm.n;
        const uint32_t* source = first_source + dm.n + 1u;
        const float* weight = reinterpret_cast<const float*>(source + dm.m);
        const uint64_t blocks = (static_cast<uint64_t>(k_end - k_first) + DM_THREADS - 1u) / DM_THREADS;
        for(uint64_t b0 = 0; b0 < blocks; b0 += DM_MAX_BLOCKS)
        {
            const uint32_t gx = static_cast<uint32_t>(std::min<uint64_t>(DM_MAX_BLOCKS, blocks - b0));
            const uint32_t k0 = k_first + static_cast<uint32_t>(b0 * DM_THREADS);
            for(uint32_t f0 = 0; f0 < n_frames; f0 += DM_MAX_FRAMES)
                hipLaunchKernelGGL(defect_repair_kernel, dim3(gx, 1u, std::min(DM_MAX_FRAMES, n_frames - f0)), dim3(DM_THREADS), 0, ctx->stream,
                                   band.frame(f0), frame_stride, pitch / sizeof(float), dim_x, defect, first_source, source, weight, k0, k_end);
        }
    };
    const auto touched = [&] { // the launch reads up to reach_rows rows beyond the band on either side
        const uint32_t reach = ctx->defect_map.stats.reach_rows, end = row_first + row_count;
        const uint32_t lo = row_first - std::min(row_first, reach);
        return paris_hip_row_range{lo, end + std::min(dim_y - end, reach) - lo};
    };
    return paris_hip_frame_pass(ctx, band, refuse, idle, launch, touched);
}

void paris_hip_warm_defect_map()
{
    hipFuncAttributes a{};
    (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&defect_repair_kernel));
}
