// Scatter kernel superposition for gfx950: the second client of the 2-D transform in frame_fft2.h (the
// statement is in include/paris_hip.h, the host rule in scatter_rule.cpp). The fixed-point iteration T = T_m - (q(T) (*) g) keeps its
// estimate out of memory: T^k is a function of the unchanged frame p and of the scatter S, which sits in LDS after a row inverse. One
// round of frames takes 2 iterations + 1 launches:
//   scatter_rows_forward_kernel   one workgroup per pair of detector rows: the source q(T_m) of rows 2r and 2r + 1, extended, packed as
//                                 a + ib, transformed and split into the scratch (iteration 0).
//   frame_fft2_columns_kernel     with the transfer function G = g1x g1y + g2x g2y, once per iteration.
//   scatter_rows_turn_kernel      one residency of LDS per row pair and iteration: merge, inverse transform, scale to S, the update to
//                                 T^(k+1) from p re-read from the frame, the source q(T^(k+1)) in place, extension, forward transform,
//                                 split into the same rows of the scratch.
//   scatter_rows_inverse_kernel   the last iteration's merge, inverse and update; -logf(T^n) stored on the pixels that entered.
// A frame is served by its own workgroups whatever else the call holds: its bits do not depend on the other frames of the call.
#include "frame_fft2.h"

namespace
{
    using namespace frame_fft2;

    // G(k_x, k_y) from the four tables: two products and one sum
    struct two_gaussians
    {
        const float* __restrict__ g1x;
        const float* __restrict__ g2x;
        const float* __restrict__ g1y;
        const float* __restrict__ g2y;
        __device__ __forceinline__ float operator()(uint32_t kx, uint32_t ky) const
        {
            return g1x[kx] * g1y[ky] + g2x[kx] * g2y[ky];
        }
    };

    struct scatter_terms
    {
        float amplitude, alpha, beta;
        float keep; // 1 - limit
    };

    // step 1: does the pixel enter the correction, and with which measured transmission
    __device__ __forceinline__ bool enters(float p, float* tm)
    {
        *tm = expf(-p);
        return isfinite(p) && *tm > 0.f && isfinite(*tm);
    }
    __device__ __forceinline__ float measured(float p) // ... air where it does not
    {
        float tm;
        return enters(p, &tm) ? tm : 1.f;
    }

    // the source of an estimate: A T^alpha L^beta through expf and logf, as the rule prescribes
    __device__ __forceinline__ float source_of(float t, const scatter_terms& c)
    {
        const float ln_t = logf(t), path = -ln_t;
        return path > 0.f ? c.amplitude * expf(c.alpha * ln_t + c.beta * logf(path)) : 0.f;
    }

    // the update: both terms from the measured transmission
    __device__ __forceinline__ float primary(float tm, float scatter, const scatter_terms& c)
    {
        return fmaxf(tm - scatter, c.keep * tm);
    }

    // samples dim_x .. n - 1 of the row from its first and last sample; barriers on both sides
    __device__ __forceinline__ void extend_row(float2* fx, uint32_t dim_x, uint32_t n, uint32_t tid, uint32_t nthreads)
    {
        __syncthreads();
        for(uint32_t s = dim_x + tid; s < n; s += nthreads)
            fx[s] = fx[source(s, dim_x, n)];
        __syncthreads();
    }

    struct row_pair
    {
        float* pa;
        float* pb;
        float2* sa; // the pair's half-spectra: rows 2r and 2r + 1 of the frame's scratch
        float2* sb;
        bool has_b;
    };

    // grid: (row pairs, frames of this round). p: row 0 of the round's first frame; scratch: its first frame's spectra, frames
    // scratch_frame complex values apart.
    __device__ __forceinline__ row_pair pair_of_this_workgroup(char* p, size_t pitch, size_t frame_stride, uint32_t dim_y, uint32_t w, float2* scratch,
                                                               size_t scratch_frame)
    {
        const uint32_t row_a = 2u * blockIdx.x;
        char* frame = p + static_cast<size_t>(blockIdx.y) * frame_stride;
        float2* sa = scratch + static_cast<size_t>(blockIdx.y) * scratch_frame + static_cast<size_t>(row_a) * w;
        return {reinterpret_cast<float*>(frame + static_cast<size_t>(row_a) * pitch),
                reinterpret_cast<float*>(frame + static_cast<size_t>(row_a + 1u) * pitch), sa, sa + w, row_a + 1u < dim_y};
    }

    __global__ void __launch_bounds__(MAX_THREADS)
        scatter_rows_forward_kernel(char* p, size_t pitch, size_t frame_stride, uint32_t dim_x, uint32_t dim_y, uint32_t log2n,
                                    const float2* __restrict__ tw, float2* scratch, size_t scratch_frame, scatter_terms c)
    {
        extern __shared__ __attribute__((aligned(16))) float2 fx[];
        const uint32_t n = 1u << log2n;
        const uint32_t tid = threadIdx.x, nthreads = blockDim.x;
        const row_pair r = pair_of_this_workgroup(p, pitch, frame_stride, dim_y, n / 2u + 1u, scratch, scratch_frame);
        for(uint32_t s = tid; s < dim_x; s += nthreads)
            fx[s] = make_float2(source_of(measured(r.pa[s]), c), r.has_b ? source_of(measured(r.pb[s]), c) : 0.f);
        extend_row(fx, dim_x, n, tid, nthreads);
        fft_dif(fx, 1u, 0u, tw, log2n, tid, nthreads);
        split_store(fx, r.sa, r.sb, r.has_b, log2n, tid, nthreads);
    }

    __global__ void __launch_bounds__(MAX_THREADS)
        scatter_rows_turn_kernel(char* p, size_t pitch, size_t frame_stride, uint32_t dim_x, uint32_t dim_y, uint32_t log2n,
                                 const float2* __restrict__ tw, float2* scratch, size_t scratch_frame, float scale, scatter_terms c)
    {
        extern __shared__ __attribute__((aligned(16))) float2 fx[];
        const uint32_t n = 1u << log2n;
        const uint32_t tid = threadIdx.x, nthreads = blockDim.x;
        const row_pair r = pair_of_this_workgroup(p, pitch, frame_stride, dim_y, n / 2u + 1u, scratch, scratch_frame);
        merge_load(fx, r.sa, r.sb, r.has_b, log2n, tid, nthreads);
        __syncthreads();
        fft_dit_inverse(fx, 1u, 0u, tw, log2n, tid, nthreads);
        for(uint32_t s = tid; s < dim_x; s += nthreads)
        {
            const float2 v = fx[s];
            fx[s] = make_float2(source_of(primary(measured(r.pa[s]), v.x * scale, c), c),
                                r.has_b ? source_of(primary(measured(r.pb[s]), v.y * scale, c), c) : 0.f);
        }
        extend_row(fx, dim_x, n, tid, nthreads);
        fft_dif(fx, 1u, 0u, tw, log2n, tid, nthreads);
        // this workgroup alone reads and writes the pair's two rows of the scratch, and has read them all
        split_store(fx, r.sa, r.sb, r.has_b, log2n, tid, nthreads);
    }

    __global__ void __launch_bounds__(MAX_THREADS)
        scatter_rows_inverse_kernel(char* p, size_t pitch, size_t frame_stride, uint32_t dim_x, uint32_t dim_y, uint32_t log2n,
                                    const float2* __restrict__ tw, float2* scratch, size_t scratch_frame, float scale, scatter_terms c)
    {
        extern __shared__ __attribute__((aligned(16))) float2 fx[];
        const uint32_t n = 1u << log2n;
        const uint32_t tid = threadIdx.x, nthreads = blockDim.x;
        const row_pair r = pair_of_this_workgroup(p, pitch, frame_stride, dim_y, n / 2u + 1u, scratch, scratch_frame);
        merge_load(fx, r.sa, r.sb, r.has_b, log2n, tid, nthreads);
        __syncthreads();
        fft_dit_inverse(fx, 1u, 0u, tw, log2n, tid, nthreads);
        for(uint32_t s = tid; s < dim_x; s += nthreads)
        {
            const float2 v = fx[s];
            float tm;
            if(enters(r.pa[s], &tm))
                r.pa[s] = -logf(primary(tm, v.x * scale, c));
            if(r.has_b && enters(r.pb[s], &tm))
                r.pb[s] = -logf(primary(tm, v.y * scale, c));
        }
    }
}

extern "C" int paris_hip_set_scatter_correction(paris_hip_ctx* ctx, const paris_hip_scatter_correction* setting, uint32_t dim_x, uint32_t dim_y,
                                                float l_x, float l_y)
{
    if(int rc = paris_hip_bind(ctx))
        return rc;
    uint32_t nx = 0, ny = 0;
    size_t scratch = 0;
    if(int rc = paris_hip_scatter_correction_check(setting, dim_x, dim_y, l_x, l_y, &nx, &ny, &scratch))
        return rc;
    // up to 64 KiB of dynamic LDS, and the columns' padding (the attribute is per device)
    PARIS_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(frame_fft2_columns_kernel<two_gaussians>),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, COLUMN_LDS_MAX));
    for(const void* kernel : {reinterpret_cast<const void*>(scatter_rows_forward_kernel), reinterpret_cast<const void*>(scatter_rows_turn_kernel),
                              reinterpret_cast<const void*>(scatter_rows_inverse_kernel)})
        PARIS_HIP_TRY(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, ROW_LDS_MAX));
    const std::vector<float2> wx = twiddles(nx), wy = twiddles(ny);
    std::vector<float> gx(2u * nx), gy(2u * ny); // g1x, g2x and g1y, g2y
    paris_hip_scatter_tables(setting, nx, ny, l_x, l_y, gx.data(), gx.data() + nx, gy.data(), gy.data() + ny);
    const size_t wx_bytes = wx.size() * sizeof(float2), wy_bytes = wy.size() * sizeof(float2), gx_bytes = gx.size() * sizeof(float),
                 gy_bytes = gy.size() * sizeof(float);
    const size_t head = wx_bytes + wy_bytes + gx_bytes + gy_bytes; // (12 (N_x + N_y), a multiple of 16: both are powers of two >= 8)
    paris_hip_device_buffer mem;
    if(int rc = paris_hip_install(ctx, head + scratch,
                                  {{0u, wx.data(), wx_bytes},
                                   {wx_bytes, wy.data(), wy_bytes},
                                   {wx_bytes + wy_bytes, gx.data(), gx_bytes},
                                   {wx_bytes + wy_bytes + gx_bytes, gy.data(), gy_bytes}},
                                  &mem))
        return rc;
    paris_hip_ctx::scatter_t& s = ctx->scatter;
    paris_hip_release(ctx, s);
    s.set = true;
    s.rule = *setting;
    s.mem = mem;
    s.dim_x = dim_x;
    s.dim_y = dim_y;
    s.n_x = nx;
    s.n_y = ny;
    s.frames = static_cast<uint32_t>(scratch / (static_cast<size_t>(dim_y) * (nx / 2u + 1u) * sizeof(float2)));
    return PARIS_HIP_SUCCESS;
}

extern "C" int paris_hip_clear_scatter_correction(paris_hip_ctx* ctx)
{
    if(int rc = paris_hip_bind(ctx))
        return rc;
    paris_hip_release(ctx, ctx->scatter);
    return PARIS_HIP_SUCCESS;
}

extern "C" int paris_hip_scatter_correction_frames(paris_hip_ctx* ctx, float* d_p, size_t pitch, size_t frame_stride, uint32_t n_frames,
                                                   uint32_t dim_x, uint32_t dim_y)
{
    const paris_hip_frame_band band{d_p, pitch, frame_stride, n_frames, dim_x, dim_y, 0u, dim_y};
    const auto refuse = [&]() -> int {
        const paris_hip_ctx::scatter_t& s = ctx->scatter;
        return !s.set || dim_x != s.dim_x || dim_y != s.dim_y ? PARIS_HIP_ERROR_INVALID_ARGUMENT : PARIS_HIP_SUCCESS;
    };
    const auto launch = [&] {
        const paris_hip_ctx::scatter_t& s = ctx->scatter;
        const plan pl(dim_y, s.n_x, s.n_y);
        const float2* tw_x = s.mem.as<float2>();
        const float2* tw_y = tw_x + s.n_x / 2u;
        const float* g1x = reinterpret_cast<const float*>(tw_y + s.n_y / 2u);
        const float* g1y = g1x + 2u * s.n_x;
        const two_gaussians g{g1x, g1x + s.n_x, g1y, g1y + s.n_y};
        float2* scratch = reinterpret_cast<float2*>(const_cast<float*>(g1y + 2u * s.n_y));
        const scatter_terms c{s.rule.amplitude, s.rule.alpha, s.rule.beta, 1.f - s.rule.limit};
        // the scratch holds s.frames frames: larger calls loop, each round behind the last in stream order
        for(uint32_t f0 = 0; f0 < n_frames; f0 += s.frames)
        {
            const dim3 rows(pl.pairs, std::min(s.frames, n_frames - f0)), columns(pl.sets, rows.y);
            hipLaunchKernelGGL(scatter_rows_forward_kernel, rows, dim3(pl.row_threads), pl.row_lds, ctx->stream, band.frame(f0), pitch, frame_stride,
                               dim_x, dim_y, pl.log2nx, tw_x, scratch, pl.scratch_frame, c);
            for(uint32_t k = 0; k < s.rule.iterations; ++k)
            {
                hipLaunchKernelGGL(frame_fft2_columns_kernel<two_gaussians>, columns, dim3(pl.col_threads), pl.col_lds, ctx->stream, scratch,
                                   pl.scratch_frame, dim_y, pl.w, pl.log2nx, pl.log2ny, pl.log2c, tw_y, g);
                hipLaunchKernelGGL(k + 1u < s.rule.iterations ? scatter_rows_turn_kernel : scatter_rows_inverse_kernel, rows, dim3(pl.row_threads),
                                   pl.row_lds, ctx->stream, band.frame(f0), pitch, frame_stride, dim_x, dim_y, pl.log2nx, tw_x, scratch,
                                   pl.scratch_frame, pl.scale, c);
            }
        }
    };
    return paris_hip_frame_pass(ctx, band, refuse, launch);
}

void paris_hip_warm_scatter()
{
    hipFuncAttributes a{};
    (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&scatter_rows_forward_kernel));
    (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&frame_fft2_columns_kernel<two_gaussians>));
    (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&scatter_rows_turn_kernel));
    (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&scatter_rows_inverse_kernel));
}
