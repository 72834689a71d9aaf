// The axis search on the device, for gfx950 (the statement is in include/paris_hip.h). The check, the plan and
// the estimate are host code (axis_rule.cpp); the device does the two passes over the data:
//   axis_collect_kernel  sums the band's rows of every frame of a call into that frame's sinogram row, through the frame-pass
//                        scaffold: a lane owns four columns of one frame (16-byte loads) where base, pitch, stride and dim_x allow
//                        (VEC), one otherwise; the host chooses per launch;
//   axis_score_kernel    the hot path, count x N x n pairs. A workgroup takes one candidate, 256 columns and 32 consecutive views. A
//                        lane owns ONE column: its plan entry is read once (one coalesced 16-byte load) and stays in registers for
//                        all the views the lane walks, so the plan needs no LDS and the kernel is the same for every n. Walking
//                        consecutive views, the conjugate's second view row of pair f is the first of pair f + 1: the column
//                        interpolation is done once per row -- three loads per pair (the sample, reversed-contiguous taps i0 and
//                        i0 + 1), all served from L2 / Infinity Cache: the sinogram is re-read per candidate and is tens of MB at most.
//                        The lane's double sum is reduced through the wave (shuffles, fixed order), the four waves through LDS,
//                        and the workgroup writes ONE partial sum that it alone owns;
//   axis_total_kernel    one workgroup per candidate adds that candidate's partial sums in a fixed order.
// No atomics anywhere: the grid and the order of every addition follow from (count, N, n) alone, so two runs give the same bits.
#include <algorithm>
#include <cmath>
#include <limits>

#include "frame_pass.h"

namespace
{
    constexpr uint32_t AXIS_THREADS = PARIS_HIP_AXIS_TILE_COLUMNS;
    constexpr uint32_t AXIS_WAVES = AXIS_THREADS / 64u;
    constexpr uint32_t AXIS_MAX_BLOCKS = 4096u; // the collect pass is memory bound: cap the grid and stride over the rest (as ring.hip)
    static_assert(AXIS_THREADS % 64u == 0, "whole waves");

    struct axis_partial // one per (candidate, view tile, column tile)
    {
        double sum;
        uint32_t pairs, skipped;
    };
    struct axis_total // one per candidate
    {
        double sum;
        uint64_t pairs, skipped;
    };
    static_assert(sizeof(axis_partial) == 16u && sizeof(axis_total) == 24u, "paris_hip_axis_layout_of counts these sizes");

    // p: row 0 of this launch's first frame; s: the sinogram row of that frame, rows n floats apart. Lane i: frame i / groups_x.
    template <bool VEC>
    __global__ void __launch_bounds__(AXIS_THREADS)
        axis_collect_kernel(const char* __restrict__ p, size_t frame_stride, size_t pitch, uint32_t n, uint32_t row_first, uint32_t rows,
                            uint32_t groups_x, uint64_t lanes, float* __restrict__ s)
    {
        constexpr uint32_t PER_LANE = VEC ? 4u : 1u;
        for(uint64_t i = static_cast<uint64_t>(blockIdx.x) * AXIS_THREADS + threadIdx.x; i < lanes; i += static_cast<uint64_t>(gridDim.x) * AXIS_THREADS)
        {
            const uint32_t f = static_cast<uint32_t>(i / groups_x);
            const uint32_t col = static_cast<uint32_t>(i % groups_x) * PER_LANE;
            const char* px = p + f * frame_stride + row_first * pitch + static_cast<size_t>(col) * sizeof(float);
            float* out = s + static_cast<size_t>(f) * n + col;
            if constexpr(VEC)
            {
                float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
                for(uint32_t r = 0; r < rows; ++r)
                {
                    const float4 v = *reinterpret_cast<const float4*>(px + r * pitch);
                    acc.x = acc.x + v.x;
                    acc.y = acc.y + v.y;
                    acc.z = acc.z + v.z;
                    acc.w = acc.w + v.w;
                }
                *reinterpret_cast<float4*>(out) = acc;
            }
            else
            {
                float acc = 0.f;
                for(uint32_t r = 0; r < rows; ++r)
                    acc = acc + *reinterpret_cast<const float*>(px + r * pitch);
                *out = acc;
            }
        }
    }

    // lanes 63 .. 1 fold onto lane 0 in six fixed steps; lane 0 holds the wave's sum
    __device__ inline void axis_wave_reduce(double& sum, uint32_t& pairs, uint32_t& skipped)
    {
#pragma unroll
        for(int d = 32; d >= 1; d >>= 1)
        {
            sum = sum + __shfl_down(sum, d);
            pairs += __shfl_down(pairs, d);
            skipped += __shfl_down(skipped, d);
        }
    }

    // the interpolated value of sinogram row `row` at the conjugate column: one fp32 subtraction, multiplication and addition
    __device__ inline float axis_tap(const float* __restrict__ row, float wi)
    {
        const float lo = row[0], hi = row[1];
        return lo + wi * (hi - lo);
    }

    // grid x: column tile fastest, then view tile; grid y: the candidate
    __global__ void __launch_bounds__(AXIS_THREADS)
        axis_score_kernel(const float* __restrict__ s, const paris_hip_axis_entry* __restrict__ plan, uint32_t n, uint32_t n_frames,
                          uint32_t col_tiles, axis_partial* __restrict__ partial)
    {
        __shared__ axis_partial of_wave[AXIS_WAVES];
        const uint32_t k = blockIdx.y, ct = blockIdx.x % col_tiles, vt = blockIdx.x / col_tiles;
        const uint32_t i = ct * PARIS_HIP_AXIS_TILE_COLUMNS + threadIdx.x;
        const uint32_t f_first = vt * PARIS_HIP_AXIS_TILE_VIEWS;
        const uint32_t f_end = f_first + min(PARIS_HIP_AXIS_TILE_VIEWS, n_frames - f_first); // (vt < view_tiles: f_first < n_frames)
        double sum = 0.0;
        uint32_t pairs = 0u, skipped = 0u;
        if(i < n)
        {
            const float4 raw = *reinterpret_cast<const float4*>(plan + static_cast<size_t>(k) * n + i);
            const int32_t i0 = __float_as_int(raw.x);
            if(i0 >= 0) // (the host made the plan: 0 <= i0 <= n - 2 and k0 < N)
            {
                const uint32_t k0 = __float_as_uint(raw.y);
                const float wi = raw.z, wf = raw.w;
                uint64_t fa = static_cast<uint64_t>(f_first) + k0;
                if(fa >= n_frames)
                    fa -= n_frames;
                const float* conj = s + i0;
                float a = axis_tap(conj + fa * n, wi);
#pragma unroll 4
                for(uint32_t f = f_first; f < f_end; ++f)
                {
                    fa = fa + 1u == n_frames ? 0u : fa + 1u;
                    const float b = axis_tap(conj + fa * n, wi);
                    const float m = a + wf * (b - a);
                    const float d = s[static_cast<size_t>(f) * n + i] - m;
                    if(isfinite(d))
                    {
                        sum = sum + static_cast<double>(d) * static_cast<double>(d);
                        ++pairs;
                    }
                    else
                        ++skipped;
                    a = b;
                }
            }
        }
        axis_wave_reduce(sum, pairs, skipped);
        if(threadIdx.x % 64u == 0)
            of_wave[threadIdx.x / 64u] = axis_partial{sum, pairs, skipped};
        __syncthreads();
        if(threadIdx.x == 0)
        {
            axis_partial t = of_wave[0];
            for(uint32_t w = 1; w < AXIS_WAVES; ++w)
            {
                t.sum = t.sum + of_wave[w].sum;
                t.pairs += of_wave[w].pairs;
                t.skipped += of_wave[w].skipped;
            }
            partial[static_cast<size_t>(k) * gridDim.x + blockIdx.x] = t;
        }
    }

    // lane t adds partial sums t, t + 256, ... of its candidate in ascending order; then the same two-level fold
    __global__ void __launch_bounds__(AXIS_THREADS) axis_total_kernel(const axis_partial* __restrict__ partial, uint32_t tiles, axis_total* __restrict__ total)
    {
        __shared__ double sum_of_wave[AXIS_WAVES];
        __shared__ unsigned long long pairs_of_wave[AXIS_WAVES], skipped_of_wave[AXIS_WAVES];
        const axis_partial* mine = partial + static_cast<size_t>(blockIdx.x) * tiles;
        double sum = 0.0;
        unsigned long long pairs = 0u, skipped = 0u;
        for(uint32_t t = threadIdx.x; t < tiles; t += AXIS_THREADS)
        {
            sum = sum + mine[t].sum;
            pairs += mine[t].pairs;
            skipped += mine[t].skipped;
        }
#pragma unroll
        for(int d = 32; d >= 1; d >>= 1)
        {
            sum = sum + __shfl_down(sum, d);
            pairs += __shfl_down(pairs, d);
            skipped += __shfl_down(skipped, d);
        }
        if(threadIdx.x % 64u == 0)
        {
            sum_of_wave[threadIdx.x / 64u] = sum;
            pairs_of_wave[threadIdx.x / 64u] = pairs;
            skipped_of_wave[threadIdx.x / 64u] = skipped;
        }
        __syncthreads();
        if(threadIdx.x == 0)
        {
            axis_total t{sum_of_wave[0], pairs_of_wave[0], skipped_of_wave[0]};
            for(uint32_t w = 1; w < AXIS_WAVES; ++w)
            {
                t.sum = t.sum + sum_of_wave[w];
                t.pairs += pairs_of_wave[w];
                t.skipped += skipped_of_wave[w];
            }
            total[blockIdx.x] = t;
        }
    }

    float* axis_sinogram(const paris_hip_ctx::axis_t& a)
    {
        return a.mem.as<float>();
    }
}

extern "C" int paris_hip_axis_search_begin(paris_hip_ctx* ctx, const paris_hip_axis_search* setting, const paris_detector_geometry* det_geo,
                                           uint32_t n_frames)
{
    if(int rc = paris_hip_bind(ctx))
        return rc;
    paris_hip_ctx::axis_t next;
    if(int rc = paris_hip_axis_search_check(setting, det_geo, n_frames, &next.row_first, nullptr))
        return rc;
    const uint32_t n = det_geo->n_row, count = setting->count;
    const paris_hip_axis_layout lay = paris_hip_axis_layout_of(n, n_frames, count);
    std::vector<paris_hip_axis_entry> plan(static_cast<size_t>(count) * n);
    next.columns.assign(count, 0u);
    for(uint32_t k = 0; k < count; ++k)
    {
        paris_hip_axis_entry* row = plan.data() + static_cast<size_t>(k) * n;
        if(int rc = paris_hip_axis_search_plan(setting, det_geo, n_frames, k, row))
            return rc;
        next.columns[k] = static_cast<uint32_t>(std::count_if(row, row + n, [](const paris_hip_axis_entry& e) { return e.i0 >= 0; }));
    }
    if(int rc = paris_hip_install(ctx, lay.bytes, {{lay.plan, plan.data(), plan.size() * sizeof(paris_hip_axis_entry)}}, &next.mem))
        return rc;
    paris_hip_release(ctx, ctx->axis);
    next.setting = *setting;
    next.n = n;
    next.n_col = det_geo->n_col;
    next.n_frames = next.missing = n_frames;
    next.seen.assign(n_frames, 0u);
    ctx->axis = std::move(next);
    return PARIS_HIP_SUCCESS;
}

extern "C" int paris_hip_axis_search_add_rows(paris_hip_ctx* ctx, const float* d_p, size_t pitch, size_t frame_stride, uint32_t n_frames,
                                              uint32_t dim_x, uint32_t dim_y, uint32_t frame_first)
{
    if(ctx == nullptr)
        return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    const bool open = ctx->axis.mem.d != nullptr && dim_x == ctx->axis.n && dim_y == ctx->axis.n_col;
    const paris_hip_frame_band band{const_cast<float*>(d_p), pitch,   frame_stride, n_frames, dim_x, dim_y, open ? ctx->axis.row_first : 0u,
                                    open ? ctx->axis.setting.rows : 0u};
    const auto refuse = [&]() -> int {
        const paris_hip_ctx::axis_t& a = ctx->axis;
        if(!open || frame_first > a.n_frames || n_frames > a.n_frames - frame_first)
            return PARIS_HIP_ERROR_INVALID_ARGUMENT;
        for(uint32_t f = frame_first; f < frame_first + n_frames; ++f)
            if(a.seen[f] != 0u)
                return PARIS_HIP_ERROR_INVALID_ARGUMENT;
        return PARIS_HIP_SUCCESS;
    };
    const auto launch = [&] {
        paris_hip_ctx::axis_t& a = ctx->axis;
        const bool vec = dim_x % 4u == 0 && pitch % 16u == 0 && reinterpret_cast<uintptr_t>(d_p) % 16u == 0 && (n_frames == 1u || frame_stride % 16u == 0);
        const uint32_t groups_x = vec ? dim_x / 4u : dim_x;
        const auto kernel = vec ? &axis_collect_kernel<true> : &axis_collect_kernel<false>;
        // larger calls loop: every launch writes sinogram rows of its own
        for(uint32_t f0 = 0; f0 < n_frames; f0 += PARIS_HIP_AXIS_FRAMES_MAX)
        {
            const uint32_t frames = std::min<uint32_t>(PARIS_HIP_AXIS_FRAMES_MAX, n_frames - f0);
            const uint64_t lanes = static_cast<uint64_t>(groups_x) * frames;
            const uint32_t blocks = static_cast<uint32_t>(std::min<uint64_t>(AXIS_MAX_BLOCKS, (lanes + AXIS_THREADS - 1u) / AXIS_THREADS));
            hipLaunchKernelGGL(kernel, dim3(blocks), dim3(AXIS_THREADS), 0, ctx->stream, band.frame(f0), frame_stride, pitch, dim_x, a.row_first,
                               a.setting.rows, groups_x, lanes, axis_sinogram(a) + static_cast<size_t>(frame_first + f0) * a.n);
        }
        std::fill(a.seen.begin() + frame_first, a.seen.begin() + frame_first + n_frames, uint8_t{1});
        a.missing -= n_frames;
    };
    return paris_hip_frame_pass(ctx, band, refuse, launch);
}

extern "C" int paris_hip_axis_search_finish(paris_hip_ctx* ctx, double* cost, uint32_t* columns, paris_hip_axis_result* result, float* h_sinogram)
{
    if(int rc = paris_hip_bind(ctx))
        return rc;
    paris_hip_ctx::axis_t& a = ctx->axis;
    if(a.mem.d == nullptr || cost == nullptr || result == nullptr || a.missing != 0u)
        return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    if(int rc = paris_hip_flush_pending_weight(ctx))
        return rc;
    const uint32_t count = a.setting.count;
    const paris_hip_axis_layout lay = paris_hip_axis_layout_of(a.n, a.n_frames, count);
    const uint32_t tiles = lay.col_tiles * lay.view_tiles;
    char* d_mem = a.mem.as<char>();
    axis_partial* d_partial = reinterpret_cast<axis_partial*>(d_mem + lay.partial);
    axis_total* d_total = reinterpret_cast<axis_total*>(d_mem + lay.total_of);
    hipLaunchKernelGGL(axis_score_kernel, dim3(tiles, count), dim3(AXIS_THREADS), 0, ctx->stream, axis_sinogram(a),
                       reinterpret_cast<const paris_hip_axis_entry*>(d_mem + lay.plan), a.n, a.n_frames, lay.col_tiles, d_partial);
    hipLaunchKernelGGL(axis_total_kernel, dim3(count), dim3(AXIS_THREADS), 0, ctx->stream, d_partial, tiles, d_total);
    PARIS_HIP_TRY(hipGetLastError());
    std::vector<axis_total> total(count);
    PARIS_HIP_TRY(hipMemcpyAsync(total.data(), d_total, count * sizeof(axis_total), hipMemcpyDeviceToHost, ctx->stream));
    if(h_sinogram != nullptr)
        PARIS_HIP_TRY(hipMemcpyAsync(h_sinogram, axis_sinogram(a), static_cast<size_t>(a.n_frames) * a.n * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    PARIS_HIP_TRY(hipStreamSynchronize(ctx->stream));
    const uint32_t min_columns = a.setting.min_columns != 0u ? a.setting.min_columns : std::max(8u, a.n / 16u);
    uint64_t skipped = 0;
    for(uint32_t k = 0; k < count; ++k)
    {
        const bool scored = a.columns[k] >= min_columns && total[k].pairs != 0u;
        cost[k] = scored ? total[k].sum / static_cast<double>(total[k].pairs) : std::numeric_limits<double>::infinity();
        skipped += total[k].skipped;
        if(columns != nullptr)
            columns[k] = a.columns[k];
    }
    const int rc = paris_hip_axis_estimate_from_costs(&a.setting, cost, a.columns.data(), result);
    result->skipped = skipped;
    result->row_first = a.row_first;
    paris_hip_release(ctx, a);
    return rc;
}

extern "C" int paris_hip_axis_search_discard(paris_hip_ctx* ctx)
{
    if(int rc = paris_hip_bind(ctx))
        return rc;
    paris_hip_release(ctx, ctx->axis);
    return PARIS_HIP_SUCCESS;
}

void paris_hip_warm_axis_search()
{
    hipFuncAttributes a{};
    (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&axis_score_kernel));
}
