// Removal of ring artefacts -- stationary detector offsets -- for gfx950 (the statement is in
// include/paris_hip.h). The rule that turns the scan's mean frame into the correction frame c is host code (ring_rule.cpp); the device
// does the two passes that touch every frame, both streaming and both through the frame-pass scaffold:
//   ring_accumulate_kernel  adds the frames of one call, in order, to the profile's double sums: a lane owns its pixels, reads its
//                           sums once, walks the frames in registers and writes the sums once -- 4 n + 16 bytes per pixel and call;
//   ring_subtract_kernel    p <- p - c where c != 0, and touches nothing else: 12 bytes per pixel at most, 4 where c == 0.
// A lane takes four pixels along x through 16-byte loads where base, pitch, stride and dim_x allow (VEC), one otherwise; the host
// chooses per launch, so no lane of a launch differs from another in how it loads. Every sum has exactly one owner per launch and the
// launches of a stream run in order: no atomics, and S is the sequential sum whatever the grid.
#include <algorithm>
#include <cmath>

#include "frame_pass.h"

namespace
{
    constexpr uint32_t RING_THREADS = 256u;
    constexpr uint32_t RING_MAX_BLOCKS = 4096u; // memory bound: cap the grid and stride over the rest (as flat_field.hip)

    // The band's pixels are dealt to the lanes as one list, row after row, `groups_x` lanes per row: rows narrower than a block
    // still fill it. p: row 0 of this launch's first frame; sum: the profile, rows dim_x doubles apart.
    template <bool VEC>
    __global__ void __launch_bounds__(RING_THREADS)
        ring_accumulate_kernel(const char* __restrict__ p, size_t frame_stride, uint32_t n_frames, size_t pitch_f, uint32_t dim_x,
                               uint32_t row_first, uint32_t groups_x, uint64_t lanes, double* __restrict__ sum)
    {
        constexpr uint32_t PER_LANE = VEC ? 4u : 1u;
        for(uint64_t i = static_cast<uint64_t>(blockIdx.x) * RING_THREADS + threadIdx.x; i < lanes; i += static_cast<uint64_t>(gridDim.x) * RING_THREADS)
        {
            const uint32_t row = row_first + static_cast<uint32_t>(i / groups_x);
            const uint32_t col = static_cast<uint32_t>(i % groups_x) * PER_LANE;
            double* s = sum + static_cast<size_t>(row) * dim_x + col;
            const char* px = p + (static_cast<size_t>(row) * pitch_f + col) * sizeof(float);
            if constexpr(VEC)
            {
                double2 lo = *reinterpret_cast<const double2*>(s), hi = *reinterpret_cast<const double2*>(s + 2);
#pragma unroll 4
                for(uint32_t f = 0; f < n_frames; ++f)
                {
                    const float4 v = *reinterpret_cast<const float4*>(px + static_cast<size_t>(f) * frame_stride);
                    lo.x += static_cast<double>(v.x);
                    lo.y += static_cast<double>(v.y);
                    hi.x += static_cast<double>(v.z);
                    hi.y += static_cast<double>(v.w);
                }
                *reinterpret_cast<double2*>(s) = lo;
                *reinterpret_cast<double2*>(s + 2) = hi;
            }
            else
            {
                double acc = *s;
#pragma unroll 4
                for(uint32_t f = 0; f < n_frames; ++f)
                    acc += static_cast<double>(*reinterpret_cast<const float*>(px + static_cast<size_t>(f) * frame_stride));
                *s = acc;
            }
        }
    }

    // the same dealing on grid x, frames on grid y (strided); c: the correction frame, rows dim_x floats apart
    template <bool VEC>
    __global__ void __launch_bounds__(RING_THREADS)
        ring_subtract_kernel(char* __restrict__ p, size_t frame_stride, uint32_t n_frames, size_t pitch_f, uint32_t dim_x, uint32_t row_first,
                             uint32_t groups_x, uint64_t lanes, const float* __restrict__ c)
    {
        constexpr uint32_t PER_LANE = VEC ? 4u : 1u;
        for(uint64_t i = static_cast<uint64_t>(blockIdx.x) * RING_THREADS + threadIdx.x; i < lanes; i += static_cast<uint64_t>(gridDim.x) * RING_THREADS)
        {
            const uint32_t row = row_first + static_cast<uint32_t>(i / groups_x);
            const uint32_t col = static_cast<uint32_t>(i % groups_x) * PER_LANE;
            const float* cp = c + static_cast<size_t>(row) * dim_x + col;
            char* px = p + (static_cast<size_t>(row) * pitch_f + col) * sizeof(float);
            if constexpr(VEC)
            {
                const float4 k = *reinterpret_cast<const float4*>(cp);
                const bool x = k.x != 0.f, y = k.y != 0.f, z = k.z != 0.f, w = k.w != 0.f;
                if(!(x || y || z || w))
                    continue;
                for(uint32_t f = blockIdx.y; f < n_frames; f += gridDim.y)
                {
                    float* q = reinterpret_cast<float*>(px + static_cast<size_t>(f) * frame_stride);
                    const float4 v = *reinterpret_cast<const float4*>(q);
                    if(x && y && z && w)
                        *reinterpret_cast<float4*>(q) = make_float4(v.x - k.x, v.y - k.y, v.z - k.z, v.w - k.w);
                    else // only the pixels that have a correction are written
                    {
                        if(x)
                            q[0] = v.x - k.x;
                        if(y)
                            q[1] = v.y - k.y;
                        if(z)
                            q[2] = v.z - k.z;
                        if(w)
                            q[3] = v.w - k.w;
                    }
                }
            }
            else
            {
                const float k = *cp;
                if(k == 0.f)
                    continue;
                for(uint32_t f = blockIdx.y; f < n_frames; f += gridDim.y)
                {
                    float* q = reinterpret_cast<float*>(px + static_cast<size_t>(f) * frame_stride);
                    *q = *q - k;
                }
            }
        }
    }

    bool ring_vector_rows(const paris_hip_frame_band& b)
    {
        return b.dim_x % 4u == 0 && b.pitch % 16u == 0 && reinterpret_cast<uintptr_t>(b.d_p) % 16u == 0
               && (b.n_frames == 1u || b.frame_stride % 16u == 0);
    }

    // the lanes of a band and the grid x that serves them
    struct ring_dealing
    {
        uint32_t groups_x, blocks;
        uint64_t lanes;
    };
    ring_dealing ring_deal(const paris_hip_frame_band& b, bool vec)
    {
        ring_dealing d{};
        d.groups_x = vec ? b.dim_x / 4u : b.dim_x;
        d.lanes = static_cast<uint64_t>(d.groups_x) * b.row_count;
        d.blocks = static_cast<uint32_t>(std::min<uint64_t>(RING_MAX_BLOCKS, (d.lanes + RING_THREADS - 1u) / RING_THREADS));
        return d;
    }
}

extern "C" int paris_hip_ring_profile_begin(paris_hip_ctx* ctx, uint32_t dim_x, uint32_t dim_y)
{
    if(int rc = paris_hip_bind(ctx))
        return rc;
    if(dim_x == 0 || dim_y == 0)
        return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    const uint64_t n = static_cast<uint64_t>(dim_x) * dim_y;
    if(n > 0xffffffffull)
        return PARIS_HIP_ERROR_UNSUPPORTED;
    const size_t bytes = static_cast<size_t>(n) * sizeof(double);
    paris_hip_device_buffer mem; // the sums start at zero
    if(int rc = paris_hip_install(ctx, bytes, {{0u, nullptr, bytes}}, &mem))
        return rc;
    paris_hip_ctx::ring_profile_t& r = ctx->ring_profile;
    paris_hip_release(ctx, r);
    r.mem = mem;
    r.dim_x = dim_x;
    r.dim_y = dim_y;
    r.count.assign(dim_y, 0u);
    return PARIS_HIP_SUCCESS;
}

extern "C" int paris_hip_ring_profile_add_rows(paris_hip_ctx* ctx, const float* d_p, size_t pitch, size_t frame_stride, uint32_t n_frames,
                                               uint32_t dim_x, uint32_t dim_y, uint32_t row_first, uint32_t row_count)
{
    const paris_hip_frame_band band{const_cast<float*>(d_p), pitch, frame_stride, n_frames, dim_x, dim_y, row_first, row_count};
    const auto refuse = [&]() -> int {
        const paris_hip_ctx::ring_profile_t& r = ctx->ring_profile;
        return r.mem.d == nullptr || dim_x != r.dim_x || dim_y != r.dim_y ? PARIS_HIP_ERROR_INVALID_ARGUMENT : PARIS_HIP_SUCCESS;
    };
    const auto launch = [&] {
        paris_hip_ctx::ring_profile_t& r = ctx->ring_profile;
        const bool vec = ring_vector_rows(band);
        const ring_dealing d = ring_deal(band, vec);
        const auto kernel = vec ? &ring_accumulate_kernel<true> : &ring_accumulate_kernel<false>;
        // larger calls loop: the launches add to the same sums, in stream order
        for(uint32_t f0 = 0; f0 < n_frames; f0 += PARIS_HIP_RING_FRAMES_MAX)
            hipLaunchKernelGGL(kernel, dim3(d.blocks), dim3(RING_THREADS), 0, ctx->stream, band.frame(f0), frame_stride,
                               std::min<uint32_t>(PARIS_HIP_RING_FRAMES_MAX, n_frames - f0), pitch / sizeof(float), dim_x, row_first, d.groups_x,
                               d.lanes, r.mem.as<double>());
        for(uint32_t y = row_first; y < row_first + row_count; ++y)
            r.count[y] += n_frames;
    };
    return paris_hip_frame_pass(ctx, band, refuse, launch);
}

extern "C" int paris_hip_ring_profile_finish(paris_hip_ctx* ctx, const paris_hip_ring_filter* setting, float* h_c, float* h_mean,
                                             paris_hip_ring_stats* out)
{
    if(int rc = paris_hip_bind(ctx))
        return rc;
    paris_hip_ctx::ring_profile_t& r = ctx->ring_profile;
    if(r.mem.d == nullptr || h_c == nullptr)
        return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    const uint32_t dim_x = r.dim_x, dim_y = r.dim_y;
    if(int rc = paris_hip_ring_filter_check(setting, dim_x, dim_y, nullptr, nullptr))
        return rc;
    if(int rc = paris_hip_flush_pending_weight(ctx))
        return rc;
    const size_t n = static_cast<size_t>(dim_x) * dim_y;
    std::vector<double> sum(n);
    PARIS_HIP_TRY(hipMemcpyAsync(sum.data(), r.mem.d, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    PARIS_HIP_TRY(hipStreamSynchronize(ctx->stream));
    std::vector<float> mean_own(h_mean == nullptr ? n : 0u);
    float* mean = h_mean != nullptr ? h_mean : mean_own.data();
    for(uint32_t y = 0; y < dim_y; ++y)
    {
        const double frames = static_cast<double>(r.count[y]);
        for(size_t k = static_cast<size_t>(y) * dim_x; k < static_cast<size_t>(y + 1u) * dim_x; ++k)
            mean[k] = r.count[y] != 0u ? static_cast<float>(sum[k] / frames) : 0.f;
    }
    const int rc = paris_hip_ring_correction_from_mean(setting, mean, r.count.data(), dim_x, dim_y, h_c, out);
    paris_hip_release(ctx, r);
    return rc;
}

extern "C" int paris_hip_ring_profile_discard(paris_hip_ctx* ctx)
{
    if(int rc = paris_hip_bind(ctx))
        return rc;
    paris_hip_release(ctx, ctx->ring_profile);
    return PARIS_HIP_SUCCESS;
}

extern "C" int paris_hip_set_ring_correction(paris_hip_ctx* ctx, const float* h_c, uint32_t dim_x, uint32_t dim_y)
{
    if(int rc = paris_hip_bind(ctx))
        return rc;
    if(h_c == nullptr || dim_x == 0 || dim_y == 0)
        return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    const size_t n = static_cast<size_t>(dim_x) * dim_y;
    bool zero = true;
    for(size_t k = 0; k < n; ++k)
    {
        if(!std::isfinite(h_c[k]))
            return PARIS_HIP_ERROR_INVALID_ARGUMENT;
        zero = zero && h_c[k] == 0.f;
    }
    paris_hip_device_buffer mem;
    if(int rc = paris_hip_install(ctx, n * sizeof(float), {{0u, h_c, n * sizeof(float)}}, &mem))
        return rc;
    paris_hip_ctx::ring_correction_t& r = ctx->ring_correction;
    paris_hip_release(ctx, r);
    r.set = true;
    r.zero = zero;
    r.mem = mem;
    r.dim_x = dim_x;
    r.dim_y = dim_y;
    return PARIS_HIP_SUCCESS;
}

extern "C" int paris_hip_clear_ring_correction(paris_hip_ctx* ctx)
{
    if(int rc = paris_hip_bind(ctx))
        return rc;
    paris_hip_release(ctx, ctx->ring_correction);
    return PARIS_HIP_SUCCESS;
}

extern "C" int paris_hip_ring_correct_rows(paris_hip_ctx* ctx, float* d_p, size_t pitch, size_t frame_stride, uint32_t n_frames, uint32_t dim_x,
                                           uint32_t dim_y, uint32_t row_first, uint32_t row_count)
{
    const paris_hip_frame_band band{d_p, pitch, frame_stride, n_frames, dim_x, dim_y, row_first, row_count};
    const auto refuse = [&]() -> int {
        const paris_hip_ctx::ring_correction_t& r = ctx->ring_correction;
        return !r.set || dim_x != r.dim_x || dim_y != r.dim_y ? PARIS_HIP_ERROR_INVALID_ARGUMENT : PARIS_HIP_SUCCESS;
    };
    const auto launch = [&] {
        const bool vec = ring_vector_rows(band);
        const ring_dealing d = ring_deal(band, vec);
        const auto kernel = vec ? &ring_subtract_kernel<true> : &ring_subtract_kernel<false>;
        hipLaunchKernelGGL(kernel, dim3(d.blocks, std::min(n_frames, 65535u)), dim3(RING_THREADS), 0, ctx->stream, band.frame(0), frame_stride, n_frames,
                           pitch / sizeof(float), dim_x, row_first, d.groups_x, d.lanes, ctx->ring_correction.mem.as<float>());
    };
    return paris_hip_frame_pass(ctx, band, refuse, [&] { return ctx->ring_correction.zero; }, launch, [&band] { return band.rows(); });
}

void paris_hip_warm_ring()
{
    hipFuncAttributes a{};
    (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&ring_accumulate_kernel<true>));
    (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&ring_subtract_kernel<true>));
}
