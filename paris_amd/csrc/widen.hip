// Widening of detector frames uploaded in their stored pixel type (paris_hip_upload_projection_raw) to fp32, in place.
//
// The host copies the s stored bytes per pixel of row r into the TAIL of that row's float row: bytes [(4 - s) * dim_x, 4 * dim_x)
// of the row. This kernel then rewrites every row in place, front to back, in chunks: each chunk's stored pixels are loaded (and
// converted) by the whole workgroup, a barrier, then the chunk's floats are stored.
//
// Why in place is safe: storing float i writes row bytes [4i, 4i + 4); stored pixel j sits at (4 - s) * dim_x + s * j. For any
// j > i that is at least (4 - s) * (i + 1) + s * (i + 1) = 4 * (i + 1), because dim_x >= i + 1: past the end of float i. So a store
// only ever clobbers pixels j <= i -- pixels of its own chunk, loaded before the barrier that precedes the store, or of earlier
// chunks, loaded before an earlier barrier. Rows are disjoint.
// Bytes past 4 * dim_x of a row are never touched.
//
// Memory bound: s bytes read and 4 written per pixel. Conversions: u8 -> v_cvt_f32_ubyte*, u16 -> zero extension + v_cvt_f32_u32,
// u32 -> v_cvt_f32_u32 (round to nearest even in the default mode) -- static_cast<float>, exactly what the host's conversion does.
//
// CORRECT (paris_hip_upload_projection_raw_corrected): the same pass also turns each widened pixel into its line integral with the
// ctx's dark and flat frames (flat_field_line_integral, flat_field.h), reading them at the pixel's own index of its ABSOLUTE
// detector row (band row r is detector row row0 + r). The in-place argument above is unchanged: the correction only adds reads
// of the reference frames, which are separate buffers, and the values stored are still those of the chunk's own pixels, loaded
// before the barrier. An f32 instantiation exists for this path only: its tail offset is 0, so each lane reads and writes just
// its own pixels -- trivially in place -- and every stored type takes exactly one pass over the frame. 8 more bytes read per
// pixel (the 32 MiB references of a 2048^2 detector may stay in the Infinity Cache from frame to frame).
#include "flat_field.h"
#include "paris_hip_internal.h"

namespace
{
    constexpr uint32_t WIDEN_THREADS = 256u;
    constexpr uint32_t WIDEN_MAX_BLOCKS = 2048u; // memory bound: cap the grid, grid-stride over rows (cdna_hip_programming.md Guideline 11)

    // the loads of a chunk must have returned before any lane of the workgroup stores into bytes they read: a plain
    // __syncthreads() does not wait for outstanding global loads
    __device__ inline void loads_done_then_barrier()
    {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }

    // vec (uniform per launch): the stored rows start 16-byte aligned and are a whole number of 16-byte vectors: a lane loads 16
    // bytes (16 / s pixels) and stores 16 / s floats as float4s. Otherwise a lane loads and stores one pixel. Same values either way.
    // the reference frames of a CORRECT launch: rows dim_x floats apart, band row r reads detector row row0 + r
    struct correction
    {
        const float* dark = nullptr;
        const float* flat = nullptr;
        uint32_t row0 = 0;
        double t_min = 1.0;
    };

    template <typename T, bool CORRECT>
    __global__ void __launch_bounds__(WIDEN_THREADS) widen_rows_kernel(char* d, size_t pitch, uint32_t dim_x, uint32_t dim_y, bool vec,
                                                                       correction c)
    {
        constexpr uint32_t S = sizeof(T);
        constexpr uint32_t VEC_PIXELS = 16u / S;
        const uint32_t per_lane = vec ? VEC_PIXELS : 1u;
        const uint32_t chunk = WIDEN_THREADS * per_lane; // pixels per chunk
        const size_t tail = static_cast<size_t>(4u - S) * dim_x;
        for(uint32_t r = blockIdx.x; r < dim_y; r += gridDim.x)
        {
            char* row = d + static_cast<size_t>(r) * pitch;
            const T* src = reinterpret_cast<const T*>(row + tail);
            float* dst = reinterpret_cast<float*>(row);
            const size_t ref_row = CORRECT ? static_cast<size_t>(c.row0 + r) * dim_x : 0u;
            for(uint32_t c0 = 0; c0 < dim_x; c0 += chunk) // (uniform trip count: every lane reaches every barrier)
            {
                const uint32_t j = c0 + threadIdx.x * per_lane;
                const bool live = j < dim_x; // vec: dim_x is a multiple of VEC_PIXELS, so a live lane's vector is whole
                float f[VEC_PIXELS];
                if(live)
                {
                    if(vec)
                    {
                        T v[VEC_PIXELS];
                        *reinterpret_cast<uint4*>(v) = *reinterpret_cast<const uint4*>(src + j);
#pragma unroll
                        for(uint32_t k = 0; k < VEC_PIXELS; ++k)
                            f[k] = static_cast<float>(v[k]);
                        if constexpr(CORRECT) // (vec: dim_x is a multiple of 4, so the reference rows start on 16 bytes too)
                        {
#pragma unroll
                            for(uint32_t k = 0; k < VEC_PIXELS; k += 4u)
                            {
                                const float4 dk = *reinterpret_cast<const float4*>(c.dark + ref_row + j + k);
                                const float4 fk = *reinterpret_cast<const float4*>(c.flat + ref_row + j + k);
                                f[k] = flat_field_line_integral(f[k], dk.x, fk.x, c.t_min);
                                f[k + 1] = flat_field_line_integral(f[k + 1], dk.y, fk.y, c.t_min);
                                f[k + 2] = flat_field_line_integral(f[k + 2], dk.z, fk.z, c.t_min);
                                f[k + 3] = flat_field_line_integral(f[k + 3], dk.w, fk.w, c.t_min);
                            }
                        }
                    }
                    else
                    {
                        f[0] = static_cast<float>(src[j]);
                        if constexpr(CORRECT)
                            f[0] = flat_field_line_integral(f[0], c.dark[ref_row + j], c.flat[ref_row + j], c.t_min);
                    }
                }
                loads_done_then_barrier();
                if(live)
                {
                    if(vec)
                    {
#pragma unroll
                        for(uint32_t k = 0; k < VEC_PIXELS; k += 4u)
                            *reinterpret_cast<float4*>(dst + j + k) = make_float4(f[k], f[k + 1], f[k + 2], f[k + 3]);
                    }
                    else
                        dst[j] = f[0];
                }
            }
        }
    }

    template <typename T, bool CORRECT>
    int launch(paris_hip_ctx* ctx, float* d_dst, size_t d_pitch, uint32_t dim_x, uint32_t dim_y, const correction& c)
    {
        const dim3 grid(dim_y < WIDEN_MAX_BLOCKS ? dim_y : WIDEN_MAX_BLOCKS);
        char* d = reinterpret_cast<char*>(d_dst);
        // s * dim_x a multiple of 16 (then 4 * dim_x is one as well) and 16-byte aligned rows: every stored row starts on 16 bytes
        const bool vec = (static_cast<size_t>(sizeof(T)) * dim_x) % 16u == 0 && d_pitch % 16u == 0 && reinterpret_cast<uintptr_t>(d) % 16u == 0;
        hipLaunchKernelGGL((widen_rows_kernel<T, CORRECT>), grid, dim3(WIDEN_THREADS), 0, ctx->stream, d, d_pitch, dim_x, dim_y, vec, c);
        PARIS_HIP_TRY(hipGetLastError());
        return PARIS_HIP_SUCCESS;
    }
}

int paris_hip_widen_rows(paris_hip_ctx* ctx, float* d_dst, size_t d_pitch, uint32_t dim_x, uint32_t dim_y, int pixel_type)
{
    if(dim_x == 0 || dim_y == 0)
        return PARIS_HIP_SUCCESS;
    switch(pixel_type)
    {
        case PARIS_HIP_PIXEL_U8: return launch<uint8_t, false>(ctx, d_dst, d_pitch, dim_x, dim_y, correction{});
        case PARIS_HIP_PIXEL_U16: return launch<uint16_t, false>(ctx, d_dst, d_pitch, dim_x, dim_y, correction{});
        case PARIS_HIP_PIXEL_U32: return launch<uint32_t, false>(ctx, d_dst, d_pitch, dim_x, dim_y, correction{});
        default: return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    }
}

int paris_hip_widen_correct_rows(paris_hip_ctx* ctx, float* d_dst, size_t d_pitch, uint32_t dim_x, uint32_t dim_y, int pixel_type,
                                 uint32_t row0)
{
    const paris_hip_ctx::flat_field_t& ff = ctx->flat_field;
    if(ff.mem.d == nullptr || dim_x != ff.dim_x || row0 > ff.dim_y || dim_y > ff.dim_y - row0)
        return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    if(dim_x == 0 || dim_y == 0)
        return PARIS_HIP_SUCCESS;
    correction c;
    c.dark = ff.mem.as<float>();
    c.flat = c.dark + static_cast<size_t>(ff.dim_x) * ff.dim_y;
    c.row0 = row0;
    c.t_min = ff.t_min;
    switch(pixel_type)
    {
        case PARIS_HIP_PIXEL_U8: return launch<uint8_t, true>(ctx, d_dst, d_pitch, dim_x, dim_y, c);
        case PARIS_HIP_PIXEL_U16: return launch<uint16_t, true>(ctx, d_dst, d_pitch, dim_x, dim_y, c);
        case PARIS_HIP_PIXEL_U32: return launch<uint32_t, true>(ctx, d_dst, d_pitch, dim_x, dim_y, c);
        case PARIS_HIP_PIXEL_F32: return launch<float, true>(ctx, d_dst, d_pitch, dim_x, dim_y, c);
        default: return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    }
}

void paris_hip_warm_widen()
{
    hipFuncAttributes a{};
    (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&widen_rows_kernel<uint16_t, false>));
}
