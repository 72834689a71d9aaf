// Adaptive frame filter against photon starvation for gfx950 (the statement is in include/paris_hip.h, the
// host rule in starvation_rule.cpp -- these kernels give its bits).
//
// The ctx holds one setting: three 64-bit counters, the table g and a scratch of PARIS_HIP_STARVATION_FRAMES_MAX dense frames.
// paris_hip_starvation_filter_frames is, per launch of up to that many frames, two kernels on the compute stream:
//   starvation_filter_kernel<R>  a workgroup of 4 waves walks tiles of ST_TX x ST_TY = 64 x 16 pixels. It reads the tile's own pixels
//                                once and asks whether any lies above p0; the usual tile has none and is done. Otherwise the tile and a
//                                halo of R go to LDS -- what lies outside the frame as NaN, which the rule's finite test drops as it
//                                drops a skipped tap, so the tap loop has no bounds test -- and every pixel above p0 takes its
//                                (2R + 1)^2 taps in the rule's order, dy then dx, with its level's R + 1 weights in registers. The
//                                results go to the scratch, never to the frame; the counts are popcounts of ballots, added once per wave.
//   starvation_store_kernel      reads every pixel once more and stores the scratch's value where the pixel lies above p0.
// The filter kernel never writes a frame and the store kernel reads no neighbour, so every window sees the frame as it was before the
// call; the kernel boundary is the only ordering needed. Work items are (frame, y tile, x tile), walked by a capped grid with 64-bit
// indices. All loads are single pixels: a row of a tile is one 256-byte segment per wave, whatever the base's alignment.
#include <algorithm>
#include <cmath>
#include <vector>

#include "frame_pass.h"

namespace
{
    constexpr uint32_t ST_THREADS = 256u, ST_TX = 64u, ST_TY = 16u, ST_WAVES = ST_THREADS / 64u;
    constexpr uint32_t ST_PW = ST_TX + 2u * PARIS_HIP_STARVATION_RADIUS_MAX; // floats per LDS row, whatever the radius
    constexpr uint32_t ST_GRID_MAX = 1024u;                                   // 4 workgroups per CU; larger calls stride

    struct st_item
    {
        uint32_t f;      // frame of this launch
        uint64_t x0, y0; // the tile's first pixel
        bool first;      // the frame's first tile
    };
    __device__ __forceinline__ st_item st_decode(uint64_t item, uint32_t tiles_x, uint32_t tiles_y)
    {
        const uint64_t tiles = static_cast<uint64_t>(tiles_x) * tiles_y, t = item % tiles;
        return {static_cast<uint32_t>(item / tiles), (t % tiles_x) * ST_TX, (t / tiles_x) * ST_TY, t == 0u};
    }

    // p: row 0 of this launch's first frame. g: PARIS_HIP_STARVATION_LEVELS rows of R + 1 weights. scratch: dense frames of
    // dim_x x dim_y. acc: frames, filtered, last_level.
    template <int R>
    __global__ void __launch_bounds__(ST_THREADS)
        starvation_filter_kernel(const char* __restrict__ p, size_t frame_stride, size_t pitch_f, uint32_t dim_x, uint32_t dim_y, uint32_t tiles_x,
                                 uint32_t tiles_y, uint64_t items, float p0, const float* __restrict__ g, float* __restrict__ scratch,
                                 unsigned long long* __restrict__ acc)
    {
        constexpr uint32_t ROWS = ST_TY + 2u * R, W = ST_TX + 2u * R, SIDE = R + 1u;
        __shared__ float tile[ROWS * ST_PW];
        __shared__ float weight[PARIS_HIP_STARVATION_LEVELS * SIDE];
        for(uint32_t i = threadIdx.x; i < PARIS_HIP_STARVATION_LEVELS * SIDE; i += ST_THREADS)
            weight[i] = g[i];
        const uint32_t lx = threadIdx.x & 63u, wave = threadIdx.x >> 6;
        const size_t plane = static_cast<size_t>(dim_x) * dim_y;
        uint32_t n_filtered = 0, n_last = 0; // (wave-uniform)
        for(uint64_t item = blockIdx.x; item < items; item += gridDim.x)
        {
            const st_item it = st_decode(item, tiles_x, tiles_y);
            const float* __restrict__ frame = reinterpret_cast<const float*>(p + static_cast<size_t>(it.f) * frame_stride);
            if(it.first && threadIdx.x == 0u)
                atomicAdd(&acc[0], 1ull);
            const uint64_t gx = it.x0 + lx;
            bool any = false;
#pragma unroll
            for(uint32_t j = 0; j < ST_TY / ST_WAVES; ++j)
            {
                const uint64_t gy = it.y0 + wave + ST_WAVES * j;
                if(gx < dim_x && gy < dim_y)
                    any = any || frame[gy * pitch_f + gx] > p0;
            }
            // also the barrier behind the last tile's taps (and, the first time, behind the weights)
            if(!__syncthreads_or(any ? 1 : 0))
                continue;
            for(uint32_t i = threadIdx.x; i < ROWS * W; i += ST_THREADS)
            {
                const uint32_t row = i / W, col = i % W;
                const int64_t ty = static_cast<int64_t>(it.y0) + row - R, tx = static_cast<int64_t>(it.x0) + col - R;
                float v = __builtin_nanf("");
                if(ty >= 0 && ty < static_cast<int64_t>(dim_y) && tx >= 0 && tx < static_cast<int64_t>(dim_x))
                    v = frame[static_cast<uint64_t>(ty) * pitch_f + static_cast<uint64_t>(tx)];
                tile[row * ST_PW + col] = v;
            }
            __syncthreads();
#pragma unroll 1
            for(uint32_t j = 0; j < ST_TY / ST_WAVES; ++j)
            {
                const uint32_t row = wave + ST_WAVES * j;
                const float* __restrict__ corner = tile + row * ST_PW + lx; // tap (-R, -R) of the lane's pixel
                const float c = corner[R * ST_PW + R];
                const bool hit = c > p0; // (false for the NaN outside the frame)
                if(__ballot(hit) == 0ull) // (wave-uniform)
                    continue;
                bool written = false, last = false;
                if(hit)
                {
                    const float t = (c - p0) * 16.f;
                    const uint32_t k = t < 64.f ? static_cast<uint32_t>(t) : 63u;
                    float wg[SIDE];
#pragma unroll
                    for(uint32_t d = 0; d < SIDE; ++d)
                        wg[d] = weight[k * SIDE + d];
                    float num = 0.f, den = 0.f;
#pragma unroll
                    for(int dy = -R; dy <= R; ++dy)
#pragma unroll
                        for(int dx = -R; dx <= R; ++dx)
                        {
                            const float v = corner[(dy + R) * static_cast<int>(ST_PW) + dx + R];
                            const bool in = __builtin_fabsf(v) < __builtin_inff(); // (false for NaN)
                            const float w = wg[dy < 0 ? -dy : dy] * wg[dx < 0 ? -dx : dx];
                            const float q = w * v; // (rounded on its own: contraction is off in this library)
                            num = in ? num + q : num;
                            den = in ? den + w : den;
                        }
                    written = den != 0.f;
                    last = written && k == 63u;
                    // a pixel the rule does not write gets its own bits back from the store kernel
                    scratch[static_cast<size_t>(it.f) * plane + (it.y0 + row) * dim_x + gx] = written ? num / den : c;
                }
                n_filtered += static_cast<uint32_t>(__popcll(__ballot(written)));
                n_last += static_cast<uint32_t>(__popcll(__ballot(last)));
            }
        }
        if(lx == 0u && n_filtered != 0u)
        {
            atomicAdd(&acc[1], static_cast<unsigned long long>(n_filtered));
            if(n_last != 0u)
                atomicAdd(&acc[2], static_cast<unsigned long long>(n_last));
        }
    }

    __global__ void __launch_bounds__(ST_THREADS)
        starvation_store_kernel(char* __restrict__ p, size_t frame_stride, size_t pitch_f, uint32_t dim_x, uint32_t dim_y, uint32_t tiles_x,
                                uint32_t tiles_y, uint64_t items, float p0, const float* __restrict__ scratch)
    {
        const uint32_t lx = threadIdx.x & 63u, wave = threadIdx.x >> 6;
        const size_t plane = static_cast<size_t>(dim_x) * dim_y;
        for(uint64_t item = blockIdx.x; item < items; item += gridDim.x)
        {
            const st_item it = st_decode(item, tiles_x, tiles_y);
            float* __restrict__ frame = reinterpret_cast<float*>(p + static_cast<size_t>(it.f) * frame_stride);
            const uint64_t gx = it.x0 + lx;
#pragma unroll
            for(uint32_t j = 0; j < ST_TY / ST_WAVES; ++j)
            {
                const uint64_t gy = it.y0 + wave + ST_WAVES * j;
                if(gx < dim_x && gy < dim_y && frame[gy * pitch_f + gx] > p0)
                    frame[gy * pitch_f + gx] = scratch[static_cast<size_t>(it.f) * plane + gy * dim_x + gx];
            }
        }
    }

    const void* st_filter_kernel_of(uint32_t radius)
    {
        switch(radius)
        {
        case 1u: return reinterpret_cast<const void*>(&starvation_filter_kernel<1>);
        case 2u: return reinterpret_cast<const void*>(&starvation_filter_kernel<2>);
        case 3u: return reinterpret_cast<const void*>(&starvation_filter_kernel<3>);
        default: return reinterpret_cast<const void*>(&starvation_filter_kernel<4>);
        }
    }
}

extern "C" int paris_hip_set_starvation_filter(paris_hip_ctx* ctx, const paris_hip_starvation_filter* setting, uint32_t dim_x, uint32_t dim_y)
{
    if(int rc = paris_hip_bind(ctx))
        return rc;
    size_t bytes = 0;
    if(int rc = paris_hip_starvation_filter_check(setting, dim_x, dim_y, &bytes))
        return rc;
    std::vector<float> g(static_cast<size_t>(PARIS_HIP_STARVATION_LEVELS) * (setting->radius + 1u));
    if(int rc = paris_hip_starvation_filter_tables(setting, nullptr, g.data()))
        return rc;
    paris_hip_device_buffer mem; // the counters start at zero
    if(int rc = paris_hip_install(ctx, bytes,
                                  {{0u, nullptr, PARIS_HIP_STARVATION_COUNTER_BYTES}, {PARIS_HIP_STARVATION_COUNTER_BYTES, g.data(), g.size() * sizeof(float)}},
                                  &mem))
        return rc;
    paris_hip_ctx::starvation_t& s = ctx->starvation;
    paris_hip_release(ctx, s);
    s.set = true;
    s.rule = *setting;
    s.dim_x = dim_x;
    s.dim_y = dim_y;
    s.mem = mem;
    return PARIS_HIP_SUCCESS;
}

extern "C" int paris_hip_clear_starvation_filter(paris_hip_ctx* ctx)
{
    if(int rc = paris_hip_bind(ctx))
        return rc;
    paris_hip_release(ctx, ctx->starvation);
    return PARIS_HIP_SUCCESS;
}

extern "C" int paris_hip_starvation_filter_frames(paris_hip_ctx* ctx, float* d_p, size_t pitch, size_t frame_stride, uint32_t n_frames,
                                                  uint32_t dim_x, uint32_t dim_y)
{
    const paris_hip_frame_band band{d_p, pitch, frame_stride, n_frames, dim_x, dim_y, 0u, dim_y};
    const auto refuse = [&]() -> int {
        const paris_hip_ctx::starvation_t& s = ctx->starvation;
        return !s.set || dim_x != s.dim_x || dim_y != s.dim_y ? PARIS_HIP_ERROR_INVALID_ARGUMENT : PARIS_HIP_SUCCESS;
    };
    const auto launch = [&] {
        const paris_hip_ctx::starvation_t& s = ctx->starvation;
        unsigned long long* acc = s.mem.as<unsigned long long>();
        const float* g = reinterpret_cast<const float*>(s.mem.as<char>() + PARIS_HIP_STARVATION_COUNTER_BYTES);
        float* scratch = reinterpret_cast<float*>(s.mem.as<char>() + PARIS_HIP_STARVATION_HEAD_BYTES);
        uint32_t tiles_x = (dim_x - 1u) / ST_TX + 1u, tiles_y = (dim_y - 1u) / ST_TY + 1u;
        const uint64_t tiles = static_cast<uint64_t>(tiles_x) * tiles_y;
        size_t pitch_f = pitch / sizeof(float);
        float p0 = s.rule.p0;
        const void* filter = st_filter_kernel_of(s.rule.radius);
        // the scratch holds PARIS_HIP_STARVATION_FRAMES_MAX frames: larger calls loop, each round behind the last in stream order
        for(uint32_t f0 = 0; f0 < n_frames; f0 += PARIS_HIP_STARVATION_FRAMES_MAX)
        {
            const uint32_t nf = std::min<uint32_t>(PARIS_HIP_STARVATION_FRAMES_MAX, n_frames - f0);
            uint64_t items = tiles * nf;
            const dim3 grid(static_cast<uint32_t>(std::min<uint64_t>(ST_GRID_MAX, items)));
            char* first = band.frame(f0);
            void* args[] = {&first, &frame_stride, &pitch_f, &dim_x, &dim_y, &tiles_x, &tiles_y, &items, &p0, &g, &scratch, &acc};
            (void)hipLaunchKernel(filter, grid, dim3(ST_THREADS), args, 0, ctx->stream); // (errors surface in paris_hip_finish)
            hipLaunchKernelGGL(starvation_store_kernel, grid, dim3(ST_THREADS), 0, ctx->stream, first, frame_stride, pitch_f, dim_x, dim_y, tiles_x, tiles_y,
                               items, p0, scratch);
        }
    };
    return paris_hip_frame_pass(ctx, band, refuse, launch);
}

extern "C" int paris_hip_starvation_stats(paris_hip_ctx* ctx, paris_hip_starvation_counts* out, int reset)
{
    if(int rc = paris_hip_bind(ctx))
        return rc;
    if(out == nullptr || !ctx->starvation.set)
        return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    if(int rc = paris_hip_flush_pending_weight(ctx))
        return rc;
    unsigned long long acc[3] = {0, 0, 0};
    PARIS_HIP_TRY(hipMemcpyAsync(acc, ctx->starvation.mem.d, sizeof(acc), hipMemcpyDeviceToHost, ctx->stream));
    if(reset)
        PARIS_HIP_TRY(hipMemsetAsync(ctx->starvation.mem.d, 0, PARIS_HIP_STARVATION_COUNTER_BYTES, ctx->stream));
    PARIS_HIP_TRY(hipStreamSynchronize(ctx->stream));
    out->frames = acc[0];
    out->filtered = acc[1];
    out->last_level = acc[2];
    return PARIS_HIP_SUCCESS;
}

void paris_hip_warm_starvation()
{
    hipFuncAttributes a{};
    for(uint32_t r = 1; r <= PARIS_HIP_STARVATION_RADIUS_MAX; ++r)
        (void)hipFuncGetAttributes(&a, st_filter_kernel_of(r));
    (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&starvation_store_kernel));
}
