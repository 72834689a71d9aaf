// Detector binning for gfx950 (the statement is in include/paris_hip.h): bin_x x bin_y source pixels, detector
// counts as fp32, become the mean of the good ones among them. A streaming pass between the raw upload and the flat-field correction:
// 4 bytes read per source pixel (5 with a mask), 4 / (bin_x bin_y) written.
//
// One lane owns whole bins, so the rule's order -- rows outer, columns inner, one fp32 addition per good pixel -- is the order of the
// lane's own instructions: no cross-lane work, no LDS, no atomics, nothing depends on scheduling. A lane takes one SEGMENT of a binned
// row: max(4, bin_x) source columns by bin_y source rows where 16-byte loads are possible (VEC), that is 4, 2, 1 or 1 bins for
// bin_x = 1, 2, 4, 8, and one bin otherwise. Consecutive lanes take consecutive segments, so a wave's loads of one source row are one
// contiguous run of 1 KiB (2 KiB for bin_x = 8). All loads of a segment, bin_y (or 2 bin_y) 16-byte vectors, are issued before the
// first addition. The bins of a segment leave in one 16-, 8- or 4-byte store. The last segment of a row may reach past dim_x (a
// detector whose width is no multiple of 4): it is read pixel by pixel. Mask bytes are read as one 32-bit word per 4 pixels where
// dim_x % 4 == 0 (the mask's rows are dim_x bytes apart), singly otherwise; the MASK = false instantiations have no mask loads at all
// and divide by the constant bin_x bin_y.
// Grid as flat_field.hip: x over a row's segments, y over binned rows, z over frames, y and z capped and strided over.
#include <algorithm>

#include "frame_pass.h"

namespace
{
    constexpr uint32_t BIN_THREADS = 256u;
    constexpr uint32_t BIN_MAX_FRAMES = 64u;   // grid z
    constexpr uint32_t BIN_MAX_BLOCKS = 8192u; // memory bound: cap the grid and stride over the rest

    struct bin_args
    {
        const char* src; // row 0 of the first source frame
        char* dst;       // row 0 of the first binned frame
        size_t src_pitch, src_stride, dst_pitch, dst_stride; // bytes
        const uint8_t* mask;                                 // dim_y rows of dim_x bytes (MASK only)
        uint32_t n_frames, dim_x, out_x, row_first, row_end; // binned rows [row_first, row_end)
        uint32_t mask_words;                                 // dim_x % 4 == 0: the mask bytes of 4 aligned pixels are one aligned word
    };

    // the rule for one bin whose pixels and mask bytes are in registers: p[r][c], m[r][c], r < BY, c in [c0, c0 + BX)
    template <uint32_t BX, uint32_t BY, bool MASK, uint32_t SEG>
    __device__ __forceinline__ float bin_mean(const float (&p)[BY][SEG], const uint8_t (&m)[BY][SEG], uint32_t c0)
    {
        float acc = 0.f;
        uint32_t n = 0;
#pragma unroll
        for(uint32_t r = 0; r < BY; ++r)
#pragma unroll
            for(uint32_t c = 0; c < BX; ++c)
            {
                if constexpr(MASK)
                {
                    if(m[r][c0 + c] == 0u)
                    {
                        acc = acc + p[r][c0 + c];
                        ++n;
                    }
                }
                else
                    acc = acc + p[r][c0 + c];
            }
        if constexpr(MASK)
            return n != 0u ? acc / static_cast<float>(n) : 0.f;
        else
            return acc / static_cast<float>(BX * BY);
    }

    template <uint32_t BX, uint32_t BY, bool MASK, bool VEC>
    __global__ void __launch_bounds__(BIN_THREADS) bin_frames_kernel(bin_args a)
    {
        constexpr uint32_t SEG = VEC ? (BX > 4u ? BX : 4u) : BX; // source columns of a lane
        constexpr uint32_t BINS = SEG / BX;                      // bins of a lane
        const uint32_t seg = blockIdx.x * BIN_THREADS + threadIdx.x;
        const uint64_t X0 = static_cast<uint64_t>(seg) * BINS; // the lane's first bin
        if(X0 >= a.out_x)
            return;
        const uint32_t x0 = static_cast<uint32_t>(X0) * BX; // its first source column (a multiple of SEG)
        const uint32_t bins = min(BINS, a.out_x - static_cast<uint32_t>(X0));
        const bool whole = VEC && x0 + SEG <= a.dim_x; // every column of the segment exists
        for(uint32_t f = blockIdx.z; f < a.n_frames; f += gridDim.z)
        {
            const char* sframe = a.src + static_cast<size_t>(f) * a.src_stride;
            char* dframe = a.dst + static_cast<size_t>(f) * a.dst_stride;
            for(uint32_t Y = a.row_first + blockIdx.y; Y < a.row_end; Y += gridDim.y)
            {
                float p[BY][SEG];
                uint8_t m[BY][SEG];
                const size_t y0 = static_cast<size_t>(Y) * BY;
                if(whole)
                {
#pragma unroll
                    for(uint32_t r = 0; r < BY; ++r)
                    {
                        const float* row = reinterpret_cast<const float*>(sframe + (y0 + r) * a.src_pitch) + x0;
#pragma unroll
                        for(uint32_t c = 0; c < SEG; c += 4u)
                        {
                            const float4 v = *reinterpret_cast<const float4*>(row + c);
                            p[r][c] = v.x;
                            p[r][c + 1u] = v.y;
                            p[r][c + 2u] = v.z;
                            p[r][c + 3u] = v.w;
                        }
                        if constexpr(MASK)
                        {
                            const uint8_t* mrow = a.mask + (y0 + r) * a.dim_x + x0;
                            if(a.mask_words)
                            {
#pragma unroll
                                for(uint32_t c = 0; c < SEG; c += 4u)
                                {
                                    const uint32_t w = *reinterpret_cast<const uint32_t*>(mrow + c);
                                    m[r][c] = static_cast<uint8_t>(w);
                                    m[r][c + 1u] = static_cast<uint8_t>(w >> 8);
                                    m[r][c + 2u] = static_cast<uint8_t>(w >> 16);
                                    m[r][c + 3u] = static_cast<uint8_t>(w >> 24);
                                }
                            }
                            else
                            {
#pragma unroll
                                for(uint32_t c = 0; c < SEG; ++c)
                                    m[r][c] = mrow[c];
                            }
                        }
                    }
                }
                else
                {
                    const uint32_t cols = bins * BX; // x0 + cols <= out_x * BX <= dim_x
#pragma unroll
                    for(uint32_t r = 0; r < BY; ++r)
                    {
                        const float* row = reinterpret_cast<const float*>(sframe + (y0 + r) * a.src_pitch) + x0;
#pragma unroll
                        for(uint32_t c = 0; c < SEG; ++c)
                        {
                            p[r][c] = c < cols ? row[c] : 0.f;
                            if constexpr(MASK)
                                m[r][c] = c < cols ? a.mask[(y0 + r) * a.dim_x + x0 + c] : uint8_t{1};
                        }
                    }
                }
                float out[BINS];
#pragma unroll
                for(uint32_t b = 0; b < BINS; ++b)
                    out[b] = bin_mean<BX, BY, MASK, SEG>(p, m, b * BX);
                float* q = reinterpret_cast<float*>(dframe + static_cast<size_t>(Y) * a.dst_pitch) + X0;
                if constexpr(BINS == 4u)
                {
                    if(bins == 4u)
                    {
                        *reinterpret_cast<float4*>(q) = make_float4(out[0], out[1], out[2], out[3]);
                        continue;
                    }
                }
                if constexpr(BINS == 2u)
                {
                    if(bins == 2u)
                    {
                        *reinterpret_cast<float2*>(q) = make_float2(out[0], out[1]);
                        continue;
                    }
                }
#pragma unroll
                for(uint32_t b = 0; b < BINS; ++b)
                    if(b < bins)
                        q[b] = out[b];
            }
        }
    }

    using bin_kernel_t = void (*)(bin_args);

    template <uint32_t BX, uint32_t BY>
    bin_kernel_t bin_kernel_for(bool mask, bool vec)
    {
        if(mask)
            return vec ? &bin_frames_kernel<BX, BY, true, true> : &bin_frames_kernel<BX, BY, true, false>;
        return vec ? &bin_frames_kernel<BX, BY, false, true> : &bin_frames_kernel<BX, BY, false, false>;
    }

    template <uint32_t BX>
    bin_kernel_t bin_kernel_for(uint32_t by, bool mask, bool vec)
    {
        switch(by)
        {
            case 1u: return bin_kernel_for<BX, 1u>(mask, vec);
            case 2u: return bin_kernel_for<BX, 2u>(mask, vec);
            case 4u: return bin_kernel_for<BX, 4u>(mask, vec);
            default: return bin_kernel_for<BX, 8u>(mask, vec);
        }
    }

    bin_kernel_t bin_kernel_for(uint32_t bx, uint32_t by, bool mask, bool vec)
    {
        switch(bx)
        {
            case 1u: return bin_kernel_for<1u>(by, mask, vec);
            case 2u: return bin_kernel_for<2u>(by, mask, vec);
            case 4u: return bin_kernel_for<4u>(by, mask, vec);
            default: return bin_kernel_for<8u>(by, mask, vec);
        }
    }

    // 16-byte loads and stores: bases, pitches and (between frames) strides of both sides are multiples of 16
    bool bin_vector_rows(const paris_hip_frame_band& b)
    {
        return b.pitch % 16u == 0 && reinterpret_cast<uintptr_t>(b.d_p) % 16u == 0 && (b.n_frames <= 1u || b.frame_stride % 16u == 0);
    }
}

extern "C" int paris_hip_set_binning(paris_hip_ctx* ctx, const paris_hip_binning* setting, const uint8_t* mask, uint32_t dim_x, uint32_t dim_y)
{
    if(int rc = paris_hip_bind(ctx))
        return rc;
    uint32_t out_x = 0, out_y = 0;
    if(int rc = paris_hip_binning_check(setting, dim_x, dim_y, &out_x, &out_y))
        return rc;
    paris_hip_device_buffer mem; // (none without a mask)
    if(mask != nullptr)
    {
        const size_t n = static_cast<size_t>(dim_x) * dim_y;
        if(int rc = paris_hip_install(ctx, n, {{0u, mask, n}}, &mem))
            return rc;
    }
    paris_hip_ctx::binning_t& bn = ctx->binning;
    paris_hip_release(ctx, bn);
    bn.set = true;
    bn.rule = *setting;
    bn.mem = mem;
    bn.dim_x = dim_x;
    bn.dim_y = dim_y;
    bn.out_x = out_x;
    bn.out_y = out_y;
    return PARIS_HIP_SUCCESS;
}

extern "C" int paris_hip_clear_binning(paris_hip_ctx* ctx)
{
    if(int rc = paris_hip_bind(ctx))
        return rc;
    paris_hip_release(ctx, ctx->binning);
    return PARIS_HIP_SUCCESS;
}

extern "C" int paris_hip_bin_frames(paris_hip_ctx* ctx, const float* d_src, size_t src_pitch, size_t src_frame_stride, float* d_dst,
                                    size_t dst_pitch, size_t dst_frame_stride, uint32_t n_frames, uint32_t dim_x, uint32_t dim_y,
                                    uint32_t row_first, uint32_t row_count)
{
    if(ctx == nullptr)
        return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    const paris_hip_ctx::binning_t& bn = ctx->binning;
    if(!bn.set || dim_x != bn.dim_x || dim_y != bn.dim_y || row_first > bn.out_y || row_count > bn.out_y - row_first)
        return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    const uint32_t by = bn.rule.bin_y;
    const paris_hip_frame_band src{const_cast<float*>(d_src), src_pitch, src_frame_stride, n_frames, dim_x, dim_y, by * row_first, by * row_count};
    const paris_hip_frame_band dst{d_dst, dst_pitch, dst_frame_stride, n_frames, bn.out_x, bn.out_y, row_first, row_count};
    const auto launch = [&] {
        const bool vec = bin_vector_rows(src) && bin_vector_rows(dst);
        const uint32_t bins_per_lane = vec ? std::max(4u, bn.rule.bin_x) / bn.rule.bin_x : 1u;
        const uint32_t lanes = (bn.out_x + bins_per_lane - 1u) / bins_per_lane;
        const uint32_t gx = (lanes + BIN_THREADS - 1u) / BIN_THREADS;
        const uint32_t gz = std::min(n_frames, BIN_MAX_FRAMES);
        const uint32_t gy = std::max(1u, std::min({row_count, 65535u, BIN_MAX_BLOCKS / std::max(1u, gx * gz)}));
        bin_args a{};
        a.src = src.frame(0);
        a.dst = dst.frame(0);
        a.src_pitch = src_pitch;
        a.src_stride = src_frame_stride;
        a.dst_pitch = dst_pitch;
        a.dst_stride = dst_frame_stride;
        a.mask = bn.mem.as<uint8_t>();
        a.n_frames = n_frames;
        a.dim_x = dim_x;
        a.out_x = bn.out_x;
        a.row_first = row_first;
        a.row_end = row_first + row_count;
        a.mask_words = dim_x % 4u == 0 ? 1u : 0u;
        hipLaunchKernelGGL(bin_kernel_for(bn.rule.bin_x, by, bn.mem.d != nullptr, vec), dim3(gx, gy, gz), dim3(BIN_THREADS), 0, ctx->stream, a);
    };
    return paris_hip_frame_pass(ctx, src, dst, [] { return PARIS_HIP_SUCCESS; }, launch);
}

void paris_hip_warm_binning()
{
    hipFuncAttributes a{};
    (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&bin_frames_kernel<2u, 2u, false, true>));
}
