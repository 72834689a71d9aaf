// Dark / flat ("offset / gain") correction of detector frames to line integrals for gfx950.
//
// A flat-panel detector records intensities I; FDK needs p = -ln(I / I0). With D the dark frame (offset) and F the flat frame
// (open beam, gain) of the same detector, p = -ln(max((I - D) / (F - D), t_min)), dead pixels 0 (flat_field.h). The ctx holds one
// setting: the two reference frames at full detector size, copied to the device by paris_hip_set_flat_field. A frame's pixel is
// always corrected with the reference pixel of its own ABSOLUTE detector row and column.
//
// Two kernels apply it, both through flat_field_line_integral, so that they agree bit for bit:
// - the fused upload path (widen.hip, CORRECT): the widening of a raw upload corrects each pixel on the way;
// - the in-place pass here, on float frames that are already on the device (paris_hip_flat_field_rows): grid x over columns
//   (4 per lane when rows allow 16-byte vectors), y over row slices, z over frames, each capped, grid-stride loops in y and z.
// Both are memory bound: s bytes read and 4 written per pixel, plus 8 bytes of reference reads.
#include <algorithm>
#include <cmath>

#include "flat_field.h"
#include "frame_pass.h"

namespace
{
    constexpr uint32_t FF_THREADS = 256u;
    constexpr uint32_t FF_ROWS_PER_THREAD = 8u; // rows a lane walks down at least (grid y strides over the band)
    constexpr uint32_t FF_MAX_FRAMES = 64u;     // grid z: frames per launch wave
    constexpr uint32_t FF_MAX_BLOCKS = 4096u;   // memory bound: cap the grid (cdna_hip_programming.md Guideline 11)

    // p: the first frame's base (row 0); rows pitch_f floats apart, frames frame_stride bytes apart; references dim_x floats per row.
    // VEC: dim_x, pitch_f and frame_stride / 4 are multiples of 4 and p is 16-byte aligned: a lane takes 4 columns as float4s.
    template <bool VEC>
    __global__ void __launch_bounds__(FF_THREADS)
        flat_field_kernel(char* p, size_t frame_stride, uint32_t n_frames, size_t pitch_f, uint32_t dim_x, uint32_t row_first,
                          uint32_t row_end, const float* __restrict__ dark, const float* __restrict__ flat, double t_min)
    {
        constexpr uint32_t PER_LANE = VEC ? 4u : 1u;
        const uint32_t col = (blockIdx.x * FF_THREADS + threadIdx.x) * PER_LANE;
        if(col >= dim_x)
            return;
        for(uint32_t f = blockIdx.z; f < n_frames; f += gridDim.z)
        {
            float* frame = reinterpret_cast<float*>(p + static_cast<size_t>(f) * frame_stride);
            for(uint32_t t = row_first + blockIdx.y; t < row_end; t += gridDim.y)
            {
                float* px = frame + static_cast<size_t>(t) * pitch_f + col;
                const size_t r = static_cast<size_t>(t) * dim_x + col;
                if constexpr(VEC)
                {
                    const float4 i = *reinterpret_cast<const float4*>(px);
                    const float4 d = *reinterpret_cast<const float4*>(dark + r);
                    const float4 fl = *reinterpret_cast<const float4*>(flat + r);
                    *reinterpret_cast<float4*>(px) = make_float4(flat_field_line_integral(i.x, d.x, fl.x, t_min),
                                                                 flat_field_line_integral(i.y, d.y, fl.y, t_min),
                                                                 flat_field_line_integral(i.z, d.z, fl.z, t_min),
                                                                 flat_field_line_integral(i.w, d.w, fl.w, t_min));
                }
                else
                    *px = flat_field_line_integral(*px, dark[r], flat[r], t_min);
            }
        }
    }
}

extern "C" int paris_hip_set_flat_field(paris_hip_ctx* ctx, const float* h_dark, const float* h_flat, uint32_t dim_x, uint32_t dim_y,
                                        float t_min)
{
    if(int rc = paris_hip_bind(ctx))
        return rc;
    if(h_flat == nullptr || dim_x == 0 || dim_y == 0 || !(t_min > 0.f && t_min <= 1.f)) // (NaN fails both, +inf the second)
        return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    const size_t n = static_cast<size_t>(dim_x) * dim_y;
    // the pixels that are dead whatever a frame holds (flat_field_line_integral's rule on D and F alone), for
    // paris_hip_flat_field_dead_pixels
    std::vector<uint8_t> dead(n);
    for(size_t k = 0; k < n; ++k)
    {
        const double dk = h_dark != nullptr ? static_cast<double>(h_dark[k]) : 0.0;
        const double den = static_cast<double>(h_flat[k]) - dk;
        dead[k] = (!(den > 0.0) || !std::isfinite(dk) || !std::isfinite(static_cast<double>(h_flat[k]))) ? 1u : 0u;
    }
    paris_hip_device_buffer mem; // the dark (zeros without one), the flat right behind it
    if(int rc = paris_hip_install(ctx, 2u * n * sizeof(float), {{0u, h_dark, n * sizeof(float)}, {n * sizeof(float), h_flat, n * sizeof(float)}}, &mem))
        return rc;
    paris_hip_ctx::flat_field_t& ff = ctx->flat_field;
    paris_hip_release(ctx, ff);
    ff.mem = mem;
    ff.dim_x = dim_x;
    ff.dim_y = dim_y;
    ff.t_min = t_min;
    ff.dead.swap(dead);
    return PARIS_HIP_SUCCESS;
}

extern "C" int paris_hip_flat_field_dead_pixels(paris_hip_ctx* ctx, uint8_t* mask)
{
    if(ctx == nullptr || mask == nullptr || ctx->flat_field.mem.d == nullptr)
        return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    std::copy(ctx->flat_field.dead.begin(), ctx->flat_field.dead.end(), mask);
    return PARIS_HIP_SUCCESS;
}

extern "C" int paris_hip_clear_flat_field(paris_hip_ctx* ctx)
{
    if(int rc = paris_hip_bind(ctx))
        return rc;
    paris_hip_release(ctx, ctx->flat_field);
    return PARIS_HIP_SUCCESS;
}

extern "C" int paris_hip_flat_field_rows(paris_hip_ctx* ctx, float* d_p, size_t pitch, size_t frame_stride, uint32_t n_frames,
                                         uint32_t dim_x, uint32_t dim_y, uint32_t row_first, uint32_t row_count)
{
    const paris_hip_frame_band band{d_p, pitch, frame_stride, n_frames, dim_x, dim_y, row_first, row_count};
    const auto refuse = [&]() -> int {
        const paris_hip_ctx::flat_field_t& ff = ctx->flat_field;
        return ff.mem.d == nullptr || dim_x != ff.dim_x || dim_y != ff.dim_y ? PARIS_HIP_ERROR_INVALID_ARGUMENT : PARIS_HIP_SUCCESS;
    };
    const auto launch = [&] {
        const paris_hip_ctx::flat_field_t& ff = ctx->flat_field;
        const bool vec = dim_x % 4u == 0 && pitch % 16u == 0 && reinterpret_cast<uintptr_t>(d_p) % 16u == 0
                         && (n_frames == 1u || frame_stride % 16u == 0);
        const uint32_t lanes = vec ? dim_x / 4u : dim_x;
        const uint32_t gx = (lanes + FF_THREADS - 1u) / FF_THREADS;
        const uint32_t gz = std::min(n_frames, FF_MAX_FRAMES);
        const uint32_t slices = (row_count + FF_ROWS_PER_THREAD - 1u) / FF_ROWS_PER_THREAD;
        const uint32_t gy = std::max(1u, std::min({slices, 65535u, FF_MAX_BLOCKS / std::max(1u, gx * gz)}));
        const float* dark = ff.mem.as<float>();
        const float* flat = dark + static_cast<size_t>(ff.dim_x) * ff.dim_y;
        const dim3 grid(gx, gy, gz);
        if(vec)
            hipLaunchKernelGGL(flat_field_kernel<true>, grid, dim3(FF_THREADS), 0, ctx->stream, band.frame(0), frame_stride, n_frames,
                               pitch / sizeof(float), dim_x, row_first, row_first + row_count, dark, flat, ff.t_min);
        else
            hipLaunchKernelGGL(flat_field_kernel<false>, grid, dim3(FF_THREADS), 0, ctx->stream, band.frame(0), frame_stride, n_frames,
                               pitch / sizeof(float), dim_x, row_first, row_first + row_count, dark, flat, ff.t_min);
    };
    return paris_hip_frame_pass(ctx, band, refuse, launch);
}

void paris_hip_warm_flat_field()
{
    hipFuncAttributes a{};
    (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&flat_field_kernel<true>));
}
