// Single-distance phase retrieval (Paganin) for gfx950: the first client of the 2-D transform in frame_fft2.h (DESIGN.md section
// 4.22; the statement is in include/paris_hip.h, the host rule in phase_rule.cpp). Three launches per round of frames, every
// transform in LDS:
//   phase_rows_forward_kernel   one workgroup per pair of detector rows: T = expf(-p) through the extension's column map, rows 2r and
//                               2r + 1 packed as a + ib, one transform of N_x, split into the two Hermitian half-spectra, which go to
//                               the scratch as rows 2r and 2r + 1 of N_x / 2 + 1 columns.
//   frame_fft2_columns_kernel   with the transfer function H = 1 / ((1 + a_x) + a_y): transforms each column, multiplies by H,
//                               transforms back.
//   phase_rows_inverse_kernel   merges the two half-spectra of a row pair, transforms back, scales by 1 / (N_x N_y) and stores
//                               -logf(fmaxf(T', t_min)) on the dim_x pixels that entered the filter.
// A frame is served by its own workgroups whatever else the call holds: its bits do not depend on the other frames of the call.
#include "frame_fft2.h"

namespace
{
    using namespace frame_fft2;

    // step 4: H(k_x, k_y) from the two tables, (1 + a_x) + a_y and one IEEE division
    struct paganin
    {
        const float* __restrict__ ax;
        const float* __restrict__ ay;
        __device__ __forceinline__ float operator()(uint32_t kx, uint32_t ky) const
        {
            return 1.f / ((1.f + ax[kx]) + ay[ky]);
        }
    };

    // step 1: does the pixel enter the filter, and as what
    __device__ __forceinline__ bool enters(float p, float* t)
    {
        *t = expf(-p);
        return isfinite(p) && isfinite(*t);
    }
    __device__ __forceinline__ float transmission(float p)
    {
        float t;
        return enters(p, &t) ? t : 1.f;
    }

    // grid: (row pairs, frames of this round). p: row 0 of the round's first frame; scratch: its first frame's spectra, frames
    // scratch_frame complex values apart.
    __global__ void __launch_bounds__(MAX_THREADS)
        phase_rows_forward_kernel(const char* __restrict__ p, size_t pitch, size_t frame_stride, uint32_t dim_x, uint32_t dim_y, uint32_t log2n,
                                  const float2* __restrict__ tw, float2* __restrict__ scratch, size_t scratch_frame)
    {
        extern __shared__ __attribute__((aligned(16))) float2 fx[];
        const uint32_t n = 1u << log2n, w = n / 2u + 1u;
        const uint32_t tid = threadIdx.x, nthreads = blockDim.x;
        const uint32_t row_a = 2u * blockIdx.x;
        const bool has_b = row_a + 1u < dim_y;
        const char* frame = p + static_cast<size_t>(blockIdx.y) * frame_stride;
        const float* pa = reinterpret_cast<const float*>(frame + static_cast<size_t>(row_a) * pitch);
        const float* pb = reinterpret_cast<const float*>(frame + static_cast<size_t>(row_a + 1u) * pitch);
        for(uint32_t s = tid; s < n; s += nthreads)
        {
            const uint32_t xs = source(s, dim_x, n);
            fx[s] = make_float2(transmission(pa[xs]), has_b ? transmission(pb[xs]) : 0.f);
        }
        __syncthreads();
        fft_dif(fx, 1u, 0u, tw, log2n, tid, nthreads);
        float2* sa = scratch + static_cast<size_t>(blockIdx.y) * scratch_frame + static_cast<size_t>(row_a) * w;
        split_store(fx, sa, sa + w, has_b, log2n, tid, nthreads);
    }

    __global__ void __launch_bounds__(MAX_THREADS)
        phase_rows_inverse_kernel(char* __restrict__ p, size_t pitch, size_t frame_stride, uint32_t dim_x, uint32_t dim_y, uint32_t log2n,
                                  const float2* __restrict__ tw, const float2* __restrict__ scratch, size_t scratch_frame, float scale, float t_min)
    {
        extern __shared__ __attribute__((aligned(16))) float2 fx[];
        const uint32_t n = 1u << log2n, w = n / 2u + 1u;
        const uint32_t tid = threadIdx.x, nthreads = blockDim.x;
        const uint32_t row_a = 2u * blockIdx.x;
        const bool has_b = row_a + 1u < dim_y;
        const float2* sa = scratch + static_cast<size_t>(blockIdx.y) * scratch_frame + static_cast<size_t>(row_a) * w;
        merge_load(fx, sa, sa + w, has_b, log2n, tid, nthreads);
        __syncthreads();
        fft_dit_inverse(fx, 1u, 0u, tw, log2n, tid, nthreads);
        char* frame = p + static_cast<size_t>(blockIdx.y) * frame_stride;
        float* pa = reinterpret_cast<float*>(frame + static_cast<size_t>(row_a) * pitch);
        float* pb = reinterpret_cast<float*>(frame + static_cast<size_t>(row_a + 1u) * pitch);
        for(uint32_t s = tid; s < dim_x; s += nthreads)
        {
            const float2 v = fx[s];
            float t;
            if(enters(pa[s], &t))
                pa[s] = -logf(fmaxf(v.x * scale, t_min));
            if(has_b && enters(pb[s], &t))
                pb[s] = -logf(fmaxf(v.y * scale, t_min));
        }
    }
}

extern "C" int paris_hip_set_phase_retrieval(paris_hip_ctx* ctx, const paris_hip_phase_retrieval* setting, uint32_t dim_x, uint32_t dim_y,
                                             float l_x, float l_y)
{
    if(int rc = paris_hip_bind(ctx))
        return rc;
    uint32_t nx = 0, ny = 0;
    size_t scratch = 0;
    if(int rc = paris_hip_phase_retrieval_check(setting, dim_x, dim_y, l_x, l_y, &nx, &ny, &scratch))
        return rc;
    // the column pass asks for 64 KiB of dynamic LDS and the columns' padding (the attribute is per device)
    PARIS_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(frame_fft2_columns_kernel<paganin>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      COLUMN_LDS_MAX));
    PARIS_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(phase_rows_forward_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      ROW_LDS_MAX));
    PARIS_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(phase_rows_inverse_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      ROW_LDS_MAX));
    const std::vector<float2> wx = twiddles(nx), wy = twiddles(ny);
    std::vector<float> ax(nx), ay(ny);
    paris_hip_phase_table(setting->alpha_mm2, nx, l_x, ax.data());
    paris_hip_phase_table(setting->alpha_mm2, ny, l_y, ay.data());
    const size_t wx_bytes = wx.size() * sizeof(float2), wy_bytes = wy.size() * sizeof(float2), ax_bytes = nx * sizeof(float),
                 ay_bytes = ny * sizeof(float);
    const size_t head = wx_bytes + wy_bytes + ax_bytes + ay_bytes; // (a multiple of 16: every length is a power of two >= 8)
    paris_hip_device_buffer mem;
    if(int rc = paris_hip_install(ctx, head + scratch,
                                  {{0u, wx.data(), wx_bytes},
                                   {wx_bytes, wy.data(), wy_bytes},
                                   {wx_bytes + wy_bytes, ax.data(), ax_bytes},
                                   {wx_bytes + wy_bytes + ax_bytes, ay.data(), ay_bytes}},
                                  &mem))
        return rc;
    paris_hip_ctx::phase_t& s = ctx->phase;
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

extern "C" int paris_hip_clear_phase_retrieval(paris_hip_ctx* ctx)
{
    if(int rc = paris_hip_bind(ctx))
        return rc;
    paris_hip_release(ctx, ctx->phase);
    return PARIS_HIP_SUCCESS;
}

extern "C" int paris_hip_phase_retrieval_frames(paris_hip_ctx* ctx, float* d_p, size_t pitch, size_t frame_stride, uint32_t n_frames,
                                                uint32_t dim_x, uint32_t dim_y)
{
    const paris_hip_frame_band band{d_p, pitch, frame_stride, n_frames, dim_x, dim_y, 0u, dim_y};
    const auto refuse = [&]() -> int {
        const paris_hip_ctx::phase_t& s = ctx->phase;
        return !s.set || dim_x != s.dim_x || dim_y != s.dim_y ? PARIS_HIP_ERROR_INVALID_ARGUMENT : PARIS_HIP_SUCCESS;
    };
    const auto launch = [&] {
        const paris_hip_ctx::phase_t& s = ctx->phase;
        const plan pl(dim_y, s.n_x, s.n_y);
        const float2* tw_x = s.mem.as<float2>();
        const float2* tw_y = tw_x + s.n_x / 2u;
        const float* ax = reinterpret_cast<const float*>(tw_y + s.n_y / 2u);
        const float* ay = ax + s.n_x;
        float2* scratch = reinterpret_cast<float2*>(const_cast<float*>(ay + s.n_y));
        // the scratch holds s.frames frames: larger calls loop, each round behind the last in stream order
        for(uint32_t f0 = 0; f0 < n_frames; f0 += s.frames)
        {
            const uint32_t nf = std::min(s.frames, n_frames - f0);
            hipLaunchKernelGGL(phase_rows_forward_kernel, dim3(pl.pairs, nf), dim3(pl.row_threads), pl.row_lds, ctx->stream, band.frame(f0), pitch,
                               frame_stride, dim_x, dim_y, pl.log2nx, tw_x, scratch, pl.scratch_frame);
            hipLaunchKernelGGL(frame_fft2_columns_kernel<paganin>, dim3(pl.sets, nf), dim3(pl.col_threads), pl.col_lds, ctx->stream, scratch,
                               pl.scratch_frame, dim_y, pl.w, pl.log2nx, pl.log2ny, pl.log2c, tw_y, paganin{ax, ay});
            hipLaunchKernelGGL(phase_rows_inverse_kernel, dim3(pl.pairs, nf), dim3(pl.row_threads), pl.row_lds, ctx->stream, band.frame(f0), pitch,
                               frame_stride, dim_x, dim_y, pl.log2nx, tw_x, scratch, pl.scratch_frame, pl.scale, s.rule.t_min);
        }
    };
    return paris_hip_frame_pass(ctx, band, refuse, launch);
}

void paris_hip_warm_phase()
{
    hipFuncAttributes a{};
    (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&phase_rows_forward_kernel));
    (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&frame_fft2_columns_kernel<paganin>));
    (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&phase_rows_inverse_kernel));
}
