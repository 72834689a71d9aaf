// Detector roll for gfx950 (the statement is in include/paris_hip.h; the host rule is roll_rule.cpp).
//
//   roll_kernel<VEC>    resamples frames: 4 bytes read and 4 written per pixel, the last frame pass before the weights and the filter.
//                       One lane owns four adjacent output pixels of one row and stores them as one 16-byte vector where the
//                       destination's base, pitch and stride allow (VEC), as single pixels otherwise and in a row's ragged last
//                       segment. The sixteen taps of a lane are plain cached loads, all issued before the first interpolation: for
//                       |eta| <= 10 deg the 256 output pixels of a wave lie on a handful of source rows, in runs the cache lines
//                       hold whole, so the loads need no LDS box. The constants travel by value.
//                       Grid as flat_field.hip: x over a row's segments, y over rows, z over frames, y and z capped and strided over.
//   roll_score_kernel   the search's cost: a workgroup takes 256 columns and 32 consecutive rows of the rolled mean. A lane owns ONE
//                       column, reads its mirror entry once and walks the rows; its double sum is reduced through the wave (shuffles,
//                       fixed order), the four waves through LDS, and the workgroup writes ONE partial sum that it alone owns;
//   roll_total_kernel   one workgroup per candidate adds that candidate's partial sums in a fixed order.
// No atomics: the grid and the order of every addition follow from (count, n_row, n_col) alone, so two runs give the same bits -- the
// structure of axis_search.hip.
#include <algorithm>
#include <cmath>
#include <limits>
#include <vector>

#include "frame_pass.h"

namespace
{
    constexpr uint32_t ROLL_THREADS = 256u;
    constexpr uint32_t ROLL_WAVES = ROLL_THREADS / 64u;
    constexpr uint32_t ROLL_MAX_FRAMES = 64u;   // grid z
    constexpr uint32_t ROLL_MAX_BLOCKS = 8192u; // memory bound: cap the grid and stride over the rest
    static_assert(ROLL_THREADS == PARIS_HIP_ROLL_TILE_COLUMNS, "a lane per column of a score tile");

    struct roll_args
    {
        const char* src; // row 0 of the first source frame
        char* dst;       // row 0 of the first destination frame
        size_t src_pitch, src_stride, dst_pitch, dst_stride; // bytes
        uint32_t n_frames, dim_x, dim_y, row_first, row_end;  // destination rows [row_first, row_end)
        paris_hip_roll_constants k;
    };

    template <bool VEC>
    __global__ void __launch_bounds__(ROLL_THREADS) roll_kernel(roll_args a)
    {
        const uint64_t X0 = (static_cast<uint64_t>(blockIdx.x) * ROLL_THREADS + threadIdx.x) * 4u; // the lane's first column
        if(X0 >= a.dim_x)
            return;
        const uint32_t x0 = static_cast<uint32_t>(X0);
        const uint32_t cols = min(4u, a.dim_x - x0);
        const float x_last = static_cast<float>(a.dim_x - 1u), y_last = static_cast<float>(a.dim_y - 1u);
        const int32_t i_last = static_cast<int32_t>(a.dim_x - 2u), j_last = static_cast<int32_t>(a.dim_y - 2u);
        float a_di[4], c_di[4];
#pragma unroll
        for(uint32_t c = 0; c < 4u; ++c)
        {
            // (a column past the row's end is computed as the last one and not stored: every tap stays inside the frame)
            const float di = static_cast<float>(min(x0 + c, a.dim_x - 1u)) - a.k.cx;
            a_di[c] = a.k.a * di;
            c_di[c] = a.k.c * di;
        }
        for(uint32_t f = blockIdx.z; f < a.n_frames; f += gridDim.z)
        {
            const char* sframe = a.src + static_cast<size_t>(f) * a.src_stride;
            char* dframe = a.dst + static_cast<size_t>(f) * a.dst_stride;
            for(uint32_t Y = a.row_first + blockIdx.y; Y < a.row_end; Y += gridDim.y)
            {
                const float dj = static_cast<float>(Y) - a.k.cy;
                const float b_dj = a.k.b * dj, d_dj = a.k.d * dj;
                float p00[4], p01[4], p10[4], p11[4], wx[4], wy[4];
#pragma unroll
                for(uint32_t c = 0; c < 4u; ++c)
                {
                    float x = (a_di[c] + b_dj) + a.k.cx, y = (c_di[c] + d_dj) + a.k.cy;
                    x = x < 0.f ? 0.f : x > x_last ? x_last : x;
                    y = y < 0.f ? 0.f : y > y_last ? y_last : y;
                    const int32_t i0 = min(static_cast<int32_t>(floorf(x)), i_last), j0 = min(static_cast<int32_t>(floorf(y)), j_last);
                    wx[c] = x - static_cast<float>(i0);
                    wy[c] = y - static_cast<float>(j0);
                    const float* r0 = reinterpret_cast<const float*>(sframe + static_cast<size_t>(j0) * a.src_pitch) + i0;
                    const float* r1 = reinterpret_cast<const float*>(sframe + (static_cast<size_t>(j0) + 1u) * a.src_pitch) + i0;
                    p00[c] = r0[0];
                    p01[c] = r0[1];
                    p10[c] = r1[0];
                    p11[c] = r1[1];
                }
                float out[4];
#pragma unroll
                for(uint32_t c = 0; c < 4u; ++c)
                {
                    const float top = p00[c] + wx[c] * (p01[c] - p00[c]);
                    const float bot = p10[c] + wx[c] * (p11[c] - p10[c]);
                    out[c] = top + wy[c] * (bot - top);
                }
                float* q = reinterpret_cast<float*>(dframe + static_cast<size_t>(Y) * a.dst_pitch) + x0;
                if(VEC && cols == 4u)
                    *reinterpret_cast<float4*>(q) = make_float4(out[0], out[1], out[2], out[3]);
                else
                {
#pragma unroll
                    for(uint32_t c = 0; c < 4u; ++c)
                        if(c < cols)
                            q[c] = out[c];
                }
            }
        }
    }

    // 16-byte stores: the destination's base, pitch and (between frames) stride are multiples of 16
    bool roll_vector_rows(const paris_hip_frame_band& b)
    {
        return b.pitch % 16u == 0 && reinterpret_cast<uintptr_t>(b.d_p) % 16u == 0 && (b.n_frames <= 1u || b.frame_stride % 16u == 0);
    }

    struct roll_partial // one per (candidate, row tile, column tile)
    {
        double sum;
        uint32_t pairs, skipped;
    };
    struct roll_total // one per candidate
    {
        double sum;
        uint64_t pairs, skipped;
    };
    static_assert(sizeof(roll_partial) == 16u && sizeof(roll_total) == 24u && sizeof(paris_hip_roll_mirror) == 8u,
                  "paris_hip_roll_layout_of counts these sizes");

    // r: the rolled mean, rows pitch_f floats apart; rows [row_first, row_end) are scored. grid x: column tile fastest, then row tile.
    __global__ void __launch_bounds__(ROLL_THREADS)
        roll_score_kernel(const float* __restrict__ r, size_t pitch_f, const paris_hip_roll_mirror* __restrict__ plan, uint32_t n, uint32_t row_first,
                          uint32_t row_end, uint32_t col_tiles, roll_partial* __restrict__ partial)
    {
        __shared__ roll_partial of_wave[ROLL_WAVES];
        const uint32_t ct = blockIdx.x % col_tiles, rt = blockIdx.x / col_tiles;
        const uint32_t i = ct * PARIS_HIP_ROLL_TILE_COLUMNS + threadIdx.x;
        const uint32_t j_first = max(row_first, rt * PARIS_HIP_ROLL_TILE_ROWS);
        const uint32_t j_end = min(row_end, (rt + 1u) * PARIS_HIP_ROLL_TILE_ROWS);
        double sum = 0.0;
        uint32_t pairs = 0u, skipped = 0u;
        if(i < n)
        {
            const paris_hip_roll_mirror e = plan[i];
            if(e.i0 >= 0) // (the host made the plan: 0 <= i0 <= n - 2)
                for(uint32_t j = j_first; j < j_end; ++j)
                {
                    const float* row = r + j * pitch_f;
                    const float lo = row[e.i0], hi = row[e.i0 + 1];
                    const float mir = lo + e.w * (hi - lo);
                    const float d = row[i] - mir;
                    if(isfinite(d))
                    {
                        sum = sum + static_cast<double>(d) * static_cast<double>(d);
                        ++pairs;
                    }
                    else
                        ++skipped;
                }
        }
#pragma unroll
        for(int d = 32; d >= 1; d >>= 1) // lanes 63 .. 1 fold onto lane 0 in six fixed steps
        {
            sum = sum + __shfl_down(sum, d);
            pairs += __shfl_down(pairs, d);
            skipped += __shfl_down(skipped, d);
        }
        if(threadIdx.x % 64u == 0)
            of_wave[threadIdx.x / 64u] = roll_partial{sum, pairs, skipped};
        __syncthreads();
        if(threadIdx.x == 0)
        {
            roll_partial t = of_wave[0];
            for(uint32_t w = 1; w < ROLL_WAVES; ++w)
            {
                t.sum = t.sum + of_wave[w].sum;
                t.pairs += of_wave[w].pairs;
                t.skipped += of_wave[w].skipped;
            }
            partial[blockIdx.x] = t;
        }
    }

    // lane t adds partial sums t, t + 256, ... of its candidate in ascending order; then the same two-level fold
    __global__ void __launch_bounds__(ROLL_THREADS) roll_total_kernel(const roll_partial* __restrict__ partial, uint32_t tiles, roll_total* __restrict__ total)
    {
        __shared__ double sum_of_wave[ROLL_WAVES];
        __shared__ unsigned long long pairs_of_wave[ROLL_WAVES], skipped_of_wave[ROLL_WAVES];
        const roll_partial* mine = partial + static_cast<size_t>(blockIdx.x) * tiles;
        double sum = 0.0;
        unsigned long long pairs = 0u, skipped = 0u;
        for(uint32_t t = threadIdx.x; t < tiles; t += ROLL_THREADS)
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
            roll_total t{sum_of_wave[0], pairs_of_wave[0], skipped_of_wave[0]};
            for(uint32_t w = 1; w < ROLL_WAVES; ++w)
            {
                t.sum = t.sum + sum_of_wave[w];
                t.pairs += pairs_of_wave[w];
                t.skipped += skipped_of_wave[w];
            }
            total[blockIdx.x] = t;
        }
    }

    // the two bands of a call: the destination band and the source rows it reads (the setting and the geometry have been checked)
    int roll_rows(paris_hip_ctx* ctx, const paris_hip_detector_roll* setting, const paris_detector_geometry* geo, const float* d_src, size_t src_pitch,
                  size_t src_stride, float* d_dst, size_t dst_pitch, size_t dst_stride, uint32_t n_frames, uint32_t dim_x, uint32_t dim_y,
                  uint32_t row_first, uint32_t row_count)
    {
        if(ctx == nullptr)
            return PARIS_HIP_ERROR_INVALID_ARGUMENT;
        uint32_t src_first = 0, src_count = 0;
        const bool known = setting != nullptr && geo != nullptr && dim_x == geo->n_row && dim_y == geo->n_col
                           && paris_hip_detector_roll_source_rows(setting, geo, row_first, row_count, &src_first, &src_count) == PARIS_HIP_SUCCESS;
        const paris_hip_frame_band src{const_cast<float*>(d_src), src_pitch, src_stride, n_frames, dim_x, dim_y, src_first, src_count};
        const paris_hip_frame_band dst{d_dst, dst_pitch, dst_stride, n_frames, dim_x, dim_y, known ? row_first : 0u, known ? row_count : 0u};
        const auto refuse = [&] { return known ? PARIS_HIP_SUCCESS : PARIS_HIP_ERROR_INVALID_ARGUMENT; };
        return paris_hip_frame_pass(ctx, src, dst, refuse, [&] { paris_hip_detector_roll_launch(ctx, src, dst, paris_hip_roll_constants_of(setting->eta_deg, *geo)); });
    }
}

void paris_hip_detector_roll_launch(paris_hip_ctx* ctx, const paris_hip_frame_band& src, const paris_hip_frame_band& dst,
                                    const paris_hip_roll_constants& k)
{
    const bool vec = roll_vector_rows(dst);
    const uint32_t lanes = (dst.dim_x + 3u) / 4u;
    const uint32_t gx = (lanes + ROLL_THREADS - 1u) / ROLL_THREADS;
    const uint32_t gz = std::min(dst.n_frames, ROLL_MAX_FRAMES);
    const uint32_t gy = std::max(1u, std::min({dst.row_count, 65535u, ROLL_MAX_BLOCKS / std::max(1u, gx * gz)}));
    roll_args a{};
    a.src = src.frame(0);
    a.dst = dst.frame(0);
    a.src_pitch = src.pitch;
    a.src_stride = src.frame_stride;
    a.dst_pitch = dst.pitch;
    a.dst_stride = dst.frame_stride;
    a.n_frames = dst.n_frames;
    a.dim_x = dst.dim_x;
    a.dim_y = dst.dim_y;
    a.row_first = dst.row_first;
    a.row_end = dst.row_first + dst.row_count;
    a.k = k;
    hipLaunchKernelGGL(vec ? &roll_kernel<true> : &roll_kernel<false>, dim3(gx, gy, gz), dim3(ROLL_THREADS), 0, ctx->stream, a);
}

extern "C" int paris_hip_set_detector_roll(paris_hip_ctx* ctx, const paris_hip_detector_roll* setting, const paris_detector_geometry* det_geo)
{
    if(int rc = paris_hip_bind(ctx))
        return rc;
    if(int rc = paris_hip_detector_roll_check(setting, det_geo))
        return rc;
    paris_hip_ctx::detector_roll_t& s = ctx->detector_roll;
    s.set = true;
    s.rule = *setting;
    s.geo = *det_geo;
    return PARIS_HIP_SUCCESS;
}

extern "C" int paris_hip_clear_detector_roll(paris_hip_ctx* ctx)
{
    if(int rc = paris_hip_bind(ctx))
        return rc;
    ctx->detector_roll = paris_hip_ctx::detector_roll_t{};
    return PARIS_HIP_SUCCESS;
}

extern "C" int paris_hip_detector_roll_rows(paris_hip_ctx* ctx, const float* d_src, size_t src_pitch, size_t src_frame_stride, float* d_dst,
                                            size_t dst_pitch, size_t dst_frame_stride, uint32_t n_frames, uint32_t dim_x, uint32_t dim_y,
                                            uint32_t row_first, uint32_t row_count)
{
    if(ctx == nullptr)
        return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    const paris_hip_ctx::detector_roll_t& s = ctx->detector_roll;
    return roll_rows(ctx, s.set ? &s.rule : nullptr, s.set ? &s.geo : nullptr, d_src, src_pitch, src_frame_stride, d_dst, dst_pitch, dst_frame_stride,
                     n_frames, dim_x, dim_y, row_first, row_count);
}

extern "C" int paris_hip_detector_roll_rows_with(paris_hip_ctx* ctx, const float* d_src, size_t src_pitch, size_t src_frame_stride, float* d_dst,
                                                 size_t dst_pitch, size_t dst_frame_stride, uint32_t n_frames, uint32_t dim_x, uint32_t dim_y,
                                                 uint32_t row_first, uint32_t row_count, const paris_hip_detector_roll* setting,
                                                 const paris_detector_geometry* det_geo)
{
    return roll_rows(ctx, setting, det_geo, d_src, src_pitch, src_frame_stride, d_dst, dst_pitch, dst_frame_stride, n_frames, dim_x, dim_y, row_first,
                     row_count);
}

extern "C" int paris_hip_roll_search_run(paris_hip_ctx* ctx, const paris_hip_roll_search* setting, const paris_detector_geometry* det_geo,
                                         const float* h_mean, double* cost, uint64_t* pairs, paris_hip_roll_result* result)
{
    if(int rc = paris_hip_bind(ctx))
        return rc;
    if(int rc = paris_hip_roll_search_check(setting, det_geo, nullptr, nullptr, nullptr))
        return rc;
    if(h_mean == nullptr || cost == nullptr || result == nullptr)
        return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    if(int rc = paris_hip_flush_pending_weight(ctx))
        return rc;
    const uint32_t n = det_geo->n_row, rows = det_geo->n_col, count = setting->count;
    const paris_hip_roll_layout lay = paris_hip_roll_layout_of(n, rows, count);
    const uint32_t tiles = lay.col_tiles * lay.row_tiles;
    uint32_t m_x = 0, m_y = 0;
    std::vector<paris_hip_roll_mirror> plan(n);
    paris_hip_roll_search_plan(*setting, *det_geo, &m_x, &m_y, plan.data());
    // the call's own memory
    char* d = nullptr;
    if(int rc = paris_hip_device_malloc(ctx, reinterpret_cast<void**>(&d), lay.bytes))
        return rc;
    float* d_mean = reinterpret_cast<float*>(d + lay.mean);
    float* d_rolled = reinterpret_cast<float*>(d + lay.rolled);
    roll_partial* d_partial = reinterpret_cast<roll_partial*>(d + lay.partial);
    roll_total* d_total = reinterpret_cast<roll_total*>(d + lay.total_of);
    std::vector<roll_total> total(count);
    const auto run = [&]() -> int {
        PARIS_HIP_TRY(hipMemcpy2DAsync(d_mean, lay.pitch, h_mean, static_cast<size_t>(n) * sizeof(float), static_cast<size_t>(n) * sizeof(float), rows,
                                       hipMemcpyHostToDevice, ctx->stream));
        PARIS_HIP_TRY(hipMemcpyAsync(d + lay.plan, plan.data(), plan.size() * sizeof(paris_hip_roll_mirror), hipMemcpyHostToDevice, ctx->stream));
        const paris_hip_frame_band src{d_mean, lay.pitch, 0u, 1u, n, rows, 0u, rows};
        const paris_hip_frame_band dst{d_rolled, lay.pitch, 0u, 1u, n, rows, 0u, rows};
        for(uint32_t k = 0; k < count; ++k)
        {
            const float eta = static_cast<float>(static_cast<double>(setting->lo_deg) + k * static_cast<double>(setting->step_deg));
            if(eta != 0.f) // (the stream orders the candidates' use of the one scratch frame)
                paris_hip_detector_roll_launch(ctx, src, dst, paris_hip_roll_constants_of(eta, *det_geo));
            hipLaunchKernelGGL(roll_score_kernel, dim3(tiles), dim3(ROLL_THREADS), 0, ctx->stream, eta != 0.f ? d_rolled : d_mean, lay.pitch / sizeof(float),
                               reinterpret_cast<const paris_hip_roll_mirror*>(d + lay.plan), n, m_y, rows - m_y, lay.col_tiles,
                               d_partial + static_cast<size_t>(k) * tiles);
        }
        hipLaunchKernelGGL(roll_total_kernel, dim3(count), dim3(ROLL_THREADS), 0, ctx->stream, d_partial, tiles, d_total);
        PARIS_HIP_TRY(hipGetLastError());
        PARIS_HIP_TRY(hipMemcpyAsync(total.data(), d_total, count * sizeof(roll_total), hipMemcpyDeviceToHost, ctx->stream));
        PARIS_HIP_TRY(hipStreamSynchronize(ctx->stream));
        return PARIS_HIP_SUCCESS;
    };
    int rc = run();
    if(rc != PARIS_HIP_SUCCESS)
        (void)hipStreamSynchronize(ctx->stream); // nothing queued may still use the memory when it goes
    (void)hipFree(d);
    if(rc != PARIS_HIP_SUCCESS)
        return rc;
    const uint64_t min_pixels = setting->min_pixels != 0u ? setting->min_pixels : static_cast<uint64_t>(n) * rows / 16u;
    uint64_t skipped = 0;
    for(uint32_t k = 0; k < count; ++k)
    {
        const bool scored = total[k].pairs >= min_pixels && total[k].pairs != 0u;
        cost[k] = scored ? total[k].sum / static_cast<double>(total[k].pairs) : std::numeric_limits<double>::infinity();
        skipped += total[k].skipped;
        if(pairs != nullptr)
            pairs[k] = total[k].pairs;
    }
    rc = paris_hip_roll_estimate_from_costs(setting, cost, result);
    result->skipped = skipped;
    result->margin_x = m_x;
    result->margin_y = m_y;
    return rc;
}

void paris_hip_warm_detector_roll()
{
    hipFuncAttributes a{};
    (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&roll_kernel<true>));
    (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&roll_kernel<false>));
    (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&roll_score_kernel));
}
