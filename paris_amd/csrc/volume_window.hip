// Volume export for gfx950: voxels quantised to 8 or 16 bits over a grey window, and the statistics a window is chosen from
// (the statement is in include/paris_hip.h).
//
// Both kernels are streams -- every voxel is read once, nothing is reused -- so they read 16-byte vectors with nontemporal loads,
// as count_negative_zero_kernel (capi.hip) does, in a grid-stride loop over a capped grid:
//   volume_quantize_kernel<TYPE, VEC>  4 bytes read and 1 or 2 written per voxel. VEC: a lane turns 16 (u8) or 8 (u16) voxels into ONE
//                                      16-byte store; the few voxels before the source's first 16-byte boundary and behind the last
//                                      whole group are done one by one by block 0. The host picks VEC when the destination reaches
//                                      a 16-byte boundary at the same voxel as the source; otherwise every voxel goes one by one.
//   volume_stats_kernel<HIST>          extremes reduced per wave, then per block, then across blocks by atomic max on an order-
//                                      preserving integer code; the histogram in LDS (32-bit integer atomics), flushed with one
//                                      64-bit global add per non-empty bin and block.
// Every counter is an integer: no result depends on the order of the atomics.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "paris_hip_internal.h"

namespace
{
    typedef float f32x4 __attribute__((ext_vector_type(4)));
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

    constexpr uint32_t VW_THREADS = 256u;
    // One pass of the quantise grid covers VW_QUANT_GRID_MAX * VW_THREADS * 16 bytes of output: 4 Mi voxels as u8, 2 Mi as u16, at 4 waves
    // per SIMD on 256 CUs. Twice the blocks made the u16 kernel 7 % SLOWER (reads and writes mix in HBM) and the read-only stats kernel
    // 14 to 27 % faster (profiles/r16_volume_window.txt): the stats grid is capped where every SIMD holds its 8 waves.
    constexpr uint32_t VW_QUANT_GRID_MAX = 1024u, VW_STATS_GRID_MAX = 2048u;
    constexpr size_t VW_QUANT_OFFSET = 0u, VW_STATS_OFFSET = 32u, VW_BINS_OFFSET = 64u; // within paris_hip_ctx::volume_window_t::mem

    struct vw_tally
    {
        uint32_t below = 0, above = 0, not_finite = 0;
    };

    __device__ __forceinline__ bool vw_finite(float v)
    {
        return __builtin_fabsf(v) < __builtin_inff(); // (false for NaN)
    }

    // the rule, for one voxel; L = 255 or 65535
    template <uint32_t L>
    __device__ __forceinline__ uint32_t vw_quantize_one(float v, float lo, float hi, float scale, vw_tally& t)
    {
        const bool finite = vw_finite(v);
        t.not_finite += finite ? 0u : 1u;
        t.below += (finite && v < lo) ? 1u : 0u;
        t.above += (finite && v > hi) ? 1u : 0u;
        const float x = (v - lo) * scale; // (a subtraction, then a multiply: contraction is off in this library)
        if(!(x > 0.f)) // x <= 0, or v is NaN
            return 0u;
        if(x >= static_cast<float>(L))
            return L;
        return static_cast<uint32_t>(__builtin_rintf(x)); // to nearest, ties to even
    }

    // the sum of each counter over the wave, added by its first lane; every lane of the wave calls it
    __device__ __forceinline__ void vw_add_wave(uint32_t a, uint32_t b, uint32_t c, unsigned long long* __restrict__ acc)
    {
#pragma unroll
        for(int off = 32; off != 0; off >>= 1)
        {
            a += __shfl_xor(a, off);
            b += __shfl_xor(b, off);
            c += __shfl_xor(c, off);
        }
        if((threadIdx.x & 63u) == 0u)
        {
            if(a != 0u)
                atomicAdd(&acc[0], static_cast<unsigned long long>(a));
            if(b != 0u)
                atomicAdd(&acc[1], static_cast<unsigned long long>(b));
            if(c != 0u)
                atomicAdd(&acc[2], static_cast<unsigned long long>(c));
        }
    }

    template <int TYPE>
    __device__ __forceinline__ void vw_store_one(void* __restrict__ q, uint64_t i, uint32_t value)
    {
        if(TYPE == PARIS_HIP_VOXEL_U8)
            static_cast<uint8_t*>(q)[i] = static_cast<uint8_t>(value);
        else
            static_cast<uint16_t*>(q)[i] = static_cast<uint16_t>(value);
    }

    // v[0, n) -> q[0, n). VEC: v + head is 16-byte aligned and so is element `head` of q (head < 4); groups of PER voxels from there.
    template <int TYPE, bool VEC>
    __global__ void __launch_bounds__(VW_THREADS)
        volume_quantize_kernel(const float* __restrict__ v, uint64_t n, uint32_t head, float lo, float hi, float scale, void* __restrict__ q,
                               unsigned long long* __restrict__ acc)
    {
        constexpr uint32_t L = TYPE == PARIS_HIP_VOXEL_U8 ? 255u : 65535u;
        constexpr uint32_t PER = TYPE == PARIS_HIP_VOXEL_U8 ? 16u : 8u; // voxels per 16-byte store
        const uint64_t first = static_cast<uint64_t>(blockIdx.x) * VW_THREADS + threadIdx.x, stride = static_cast<uint64_t>(gridDim.x) * VW_THREADS;
        vw_tally t;
        if(VEC)
        {
            const uint64_t groups = (n - head) / PER;
            const f32x4* __restrict__ src = reinterpret_cast<const f32x4*>(v + head);
            u32x4* __restrict__ dst = reinterpret_cast<u32x4*>(static_cast<char*>(q) + static_cast<size_t>(head) * (16u / PER));
            for(uint64_t g = first; g < groups; g += stride)
            {
                f32x4 in[PER / 4u];
#pragma unroll
                for(uint32_t k = 0; k < PER / 4u; ++k)
                    in[k] = __builtin_nontemporal_load(src + g * (PER / 4u) + k);
                uint32_t w[4];
#pragma unroll
                for(uint32_t k = 0; k < 4u; ++k)
                {
                    if constexpr(TYPE == PARIS_HIP_VOXEL_U8) // word k: voxels 4k .. 4k + 3, the first in the lowest byte
                        w[k] = vw_quantize_one<L>(in[k].x, lo, hi, scale, t) | (vw_quantize_one<L>(in[k].y, lo, hi, scale, t) << 8)
                               | (vw_quantize_one<L>(in[k].z, lo, hi, scale, t) << 16) | (vw_quantize_one<L>(in[k].w, lo, hi, scale, t) << 24);
                    else // word k: voxels 2k, 2k + 1
                    {
                        const f32x4 p = in[k / 2u];
                        w[k] = (k & 1u) == 0u ? (vw_quantize_one<L>(p.x, lo, hi, scale, t) | (vw_quantize_one<L>(p.y, lo, hi, scale, t) << 16))
                                              : (vw_quantize_one<L>(p.z, lo, hi, scale, t) | (vw_quantize_one<L>(p.w, lo, hi, scale, t) << 16));
                    }
                }
                u32x4 out;
                out.x = w[0];
                out.y = w[1];
                out.z = w[2];
                out.w = w[3];
                dst[g] = out;
            }
            if(blockIdx.x == 0u) // the voxels before the first and behind the last group: fewer than 4 and fewer than PER
            {
                const uint64_t tail0 = head + groups * PER;
                if(threadIdx.x < head)
                    vw_store_one<TYPE>(q, threadIdx.x, vw_quantize_one<L>(v[threadIdx.x], lo, hi, scale, t));
                if(tail0 + threadIdx.x < n)
                    vw_store_one<TYPE>(q, tail0 + threadIdx.x, vw_quantize_one<L>(v[tail0 + threadIdx.x], lo, hi, scale, t));
            }
        }
        else
        {
            for(uint64_t i = first; i < n; i += stride)
                vw_store_one<TYPE>(q, i, vw_quantize_one<L>(__builtin_nontemporal_load(v + i), lo, hi, scale, t));
        }
        vw_add_wave(t.below, t.above, t.not_finite, acc);
    }

    // fp32 -> a 32-bit code with the same order (finite values and infinities): negative values have all bits flipped, others the sign
    __device__ __forceinline__ uint32_t vw_order_code(float f)
    {
        const uint32_t b = __float_as_uint(f);
        return (b & 0x80000000u) != 0u ? ~b : (b | 0x80000000u);
    }

    struct vw_extremes
    {
        float mn = __builtin_inff(), mx = -__builtin_inff();
    };

    template <bool HIST>
    __device__ __forceinline__ void vw_stats_one(float v, float h_lo, float h_hi, float bscale, uint32_t n_bins, uint32_t* __restrict__ lds_hist,
                                                 vw_extremes& e, vw_tally& t)
    {
        const bool finite = vw_finite(v);
        t.not_finite += finite ? 0u : 1u;
        e.mn = finite ? __builtin_fminf(e.mn, v) : e.mn;
        e.mx = finite ? __builtin_fmaxf(e.mx, v) : e.mx;
        if(HIST && finite)
        {
            if(v < h_lo)
                ++t.below;
            else if(v > h_hi)
                ++t.above;
            else
            {
                const float x = (v - h_lo) * bscale; // >= 0; +inf when the subtraction overflows
                const uint32_t b = x >= static_cast<float>(n_bins) ? n_bins - 1u : static_cast<uint32_t>(x); // = min(n_bins - 1, trunc(x))
                atomicAdd(&lds_hist[b], 1u);
            }
        }
    }

    // ext[0]: the largest ~code of a finite voxel (the minimum), ext[1]: the largest code (the maximum); 0 stands for "none" in both --
    // no finite value has the code 0 or ~0. cnt: below, above, not_finite. A block's LDS bins are 32-bit: a block sees n / gridDim.x
    // voxels, far below 2^32 for anything a device holds.
    template <bool HIST>
    __global__ void __launch_bounds__(VW_THREADS)
        volume_stats_kernel(const float* __restrict__ v, uint64_t n, float h_lo, float h_hi, float bscale, uint32_t n_bins, uint32_t* __restrict__ ext,
                            unsigned long long* __restrict__ cnt, unsigned long long* __restrict__ bins)
    {
        __shared__ uint32_t lds_hist[HIST ? PARIS_HIP_VOLUME_HISTOGRAM_BINS_MAX : 1];
        __shared__ float lds_mn[VW_THREADS / 64u], lds_mx[VW_THREADS / 64u];
        if(HIST)
        {
            for(uint32_t b = threadIdx.x; b < n_bins; b += VW_THREADS)
                lds_hist[b] = 0u;
            __syncthreads();
        }
        const uint32_t to_boundary = ((16u - static_cast<uint32_t>(reinterpret_cast<uintptr_t>(v) & 15u)) & 15u) / 4u;
        const uint32_t head = n < to_boundary ? static_cast<uint32_t>(n) : to_boundary;
        const uint64_t n4 = (n - head) / 4u;
        const f32x4* __restrict__ body = reinterpret_cast<const f32x4*>(v + head);
        vw_extremes e;
        vw_tally t;
        for(uint64_t i = static_cast<uint64_t>(blockIdx.x) * VW_THREADS + threadIdx.x; i < n4; i += static_cast<uint64_t>(gridDim.x) * VW_THREADS)
        {
            const f32x4 p = __builtin_nontemporal_load(body + i);
            vw_stats_one<HIST>(p.x, h_lo, h_hi, bscale, n_bins, lds_hist, e, t);
            vw_stats_one<HIST>(p.y, h_lo, h_hi, bscale, n_bins, lds_hist, e, t);
            vw_stats_one<HIST>(p.z, h_lo, h_hi, bscale, n_bins, lds_hist, e, t);
            vw_stats_one<HIST>(p.w, h_lo, h_hi, bscale, n_bins, lds_hist, e, t);
        }
        if(blockIdx.x == 0u)
        {
            const uint64_t tail0 = head + 4u * n4;
            if(threadIdx.x < head)
                vw_stats_one<HIST>(v[threadIdx.x], h_lo, h_hi, bscale, n_bins, lds_hist, e, t);
            if(tail0 + threadIdx.x < n)
                vw_stats_one<HIST>(v[tail0 + threadIdx.x], h_lo, h_hi, bscale, n_bins, lds_hist, e, t);
        }
        vw_add_wave(t.below, t.above, t.not_finite, cnt);
#pragma unroll
        for(int off = 32; off != 0; off >>= 1)
        {
            e.mn = __builtin_fminf(e.mn, __shfl_xor(e.mn, off));
            e.mx = __builtin_fmaxf(e.mx, __shfl_xor(e.mx, off));
        }
        if((threadIdx.x & 63u) == 0u)
        {
            lds_mn[threadIdx.x / 64u] = e.mn;
            lds_mx[threadIdx.x / 64u] = e.mx;
        }
        __syncthreads(); // (also: every LDS bin update of the block is done)
        if(threadIdx.x == 0u)
        {
            float mn = lds_mn[0], mx = lds_mx[0];
#pragma unroll
            for(uint32_t w = 1; w < VW_THREADS / 64u; ++w)
            {
                mn = __builtin_fminf(mn, lds_mn[w]);
                mx = __builtin_fmaxf(mx, lds_mx[w]);
            }
            if(mn <= mx) // the block saw a finite voxel
            {
                atomicMax(&ext[0], ~vw_order_code(mn));
                atomicMax(&ext[1], vw_order_code(mx));
            }
        }
        if(HIST)
            for(uint32_t b = threadIdx.x; b < n_bins; b += VW_THREADS)
            {
                const uint32_t c = lds_hist[b];
                if(c != 0u)
                    atomicAdd(&bins[b], static_cast<unsigned long long>(c));
            }
    }

    float vw_decode(uint32_t code)
    {
        const uint32_t b = (code & 0x80000000u) != 0u ? (code & 0x7fffffffu) : ~code;
        float f;
        static_assert(sizeof(f) == sizeof(b), "fp32");
        std::memcpy(&f, &b, sizeof(f));
        return f;
    }

    // the rule's scale for `levels` steps over [lo, hi]; false for a range the rule refuses
    bool vw_scale(float lo, float hi, double levels, float* scale)
    {
        if(!std::isfinite(lo) || !std::isfinite(hi) || !(hi > lo))
            return false;
        const double width = static_cast<double>(hi) - static_cast<double>(lo);
        if(width < 0x1p-100)
            return false;
        const float s = static_cast<float>(levels / width);
        if(!std::isfinite(s))
            return false;
        *scale = s;
        return true;
    }

    bool vw_setting_scale(const paris_hip_volume_window* w, float* scale, uint32_t* elem)
    {
        if(w == nullptr || (w->voxel_type != PARIS_HIP_VOXEL_U8 && w->voxel_type != PARIS_HIP_VOXEL_U16))
            return false;
        *elem = w->voxel_type == PARIS_HIP_VOXEL_U8 ? 1u : 2u;
        return vw_scale(w->lo, w->hi, w->voxel_type == PARIS_HIP_VOXEL_U8 ? 255.0 : 65535.0, scale);
    }

    // the ctx's counters, made and zeroed in stream order before their first use
    int vw_ensure_acc(paris_hip_ctx* ctx)
    {
        if(ctx->volume_window.mem.d != nullptr)
            return PARIS_HIP_SUCCESS;
        char* d = nullptr;
        if(int rc = paris_hip_device_malloc(ctx, reinterpret_cast<void**>(&d), PARIS_HIP_VOLUME_WINDOW_ACC_BYTES))
            return rc;
        const hipError_t err = hipMemsetAsync(d + VW_QUANT_OFFSET, 0, VW_STATS_OFFSET - VW_QUANT_OFFSET, ctx->stream);
        if(err != hipSuccess)
        {
            (void)hipFree(d);
            return static_cast<int>(err);
        }
        ctx->volume_window.mem = paris_hip_device_buffer{d, PARIS_HIP_VOLUME_WINDOW_ACC_BYTES};
        return PARIS_HIP_SUCCESS;
    }

    // enqueues the quantise kernel for arguments already checked; d_q is device memory
    int vw_launch_quantize(paris_hip_ctx* ctx, const float* d_v, uint64_t n, const paris_hip_volume_window* w, float scale, uint32_t elem, void* d_q)
    {
        if(int rc = vw_ensure_acc(ctx))
            return rc;
        unsigned long long* acc = reinterpret_cast<unsigned long long*>(ctx->volume_window.mem.as<char>() + VW_QUANT_OFFSET);
        const uint32_t per = 16u / elem;
        const uint32_t head = ((16u - static_cast<uint32_t>(reinterpret_cast<uintptr_t>(d_v) & 15u)) & 15u) / 4u;
        const bool vec = n >= static_cast<uint64_t>(head) + per && (reinterpret_cast<uintptr_t>(d_q) + head * elem) % 16u == 0u;
        const uint64_t items = vec ? (n - head) / per : n; // what the grid-stride loop walks over
        const uint32_t blocks = static_cast<uint32_t>(std::min<uint64_t>(VW_QUANT_GRID_MAX, (items + VW_THREADS - 1u) / VW_THREADS));
        const bool u8 = w->voxel_type == PARIS_HIP_VOXEL_U8;
        const auto kernel = u8 ? (vec ? &volume_quantize_kernel<PARIS_HIP_VOXEL_U8, true> : &volume_quantize_kernel<PARIS_HIP_VOXEL_U8, false>)
                               : (vec ? &volume_quantize_kernel<PARIS_HIP_VOXEL_U16, true> : &volume_quantize_kernel<PARIS_HIP_VOXEL_U16, false>);
        hipLaunchKernelGGL(kernel, dim3(blocks), dim3(VW_THREADS), 0, ctx->stream, d_v, n, head, w->lo, w->hi, scale, d_q, acc);
        PARIS_HIP_TRY(hipGetLastError());
        ctx->volume_window.voxels += n;
        return PARIS_HIP_SUCCESS;
    }
}

extern "C" int paris_hip_volume_window_check(const paris_hip_volume_window* setting)
{
    float scale = 0.f;
    uint32_t elem = 0;
    return vw_setting_scale(setting, &scale, &elem) ? PARIS_HIP_SUCCESS : PARIS_HIP_ERROR_INVALID_ARGUMENT;
}

extern "C" int paris_hip_volume_window_from_histogram(const uint64_t* hist, uint32_t n_bins, float h_lo, float h_hi, double p_lo, double p_hi,
                                                      float* w_lo, float* w_hi)
{
    float bscale = 0.f;
    if(hist == nullptr || w_lo == nullptr || w_hi == nullptr || n_bins == 0u || !vw_scale(h_lo, h_hi, static_cast<double>(n_bins), &bscale))
        return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    if(!(p_lo >= 0.0) || !(p_lo < p_hi) || !(p_hi <= 100.0))
        return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    uint64_t total = 0;
    for(uint32_t b = 0; b < n_bins; ++b)
        total += hist[b];
    if(total == 0u)
        return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    const double t = static_cast<double>(total);
    const double t_lo = t * p_lo / 100.0, t_hi = t * p_hi / 100.0;
    const double width = (static_cast<double>(h_hi) - static_cast<double>(h_lo)) / static_cast<double>(n_bins);
    uint32_t b_lo = n_bins - 1u, b_hi = n_bins - 1u; // (where rounding leaves no bin that qualifies: the last)
    bool have_lo = false, have_hi = false;
    uint64_t c = 0;
    for(uint32_t b = 0; b < n_bins && !(have_lo && have_hi); ++b)
    {
        c += hist[b];
        if(!have_lo && static_cast<double>(c) > t_lo)
        {
            b_lo = b;
            have_lo = true;
        }
        if(!have_hi && static_cast<double>(c) >= t_hi)
        {
            b_hi = b;
            have_hi = true;
        }
    }
    *w_lo = static_cast<float>(static_cast<double>(h_lo) + static_cast<double>(b_lo) * width);
    *w_hi = static_cast<float>(static_cast<double>(h_lo) + (static_cast<double>(b_hi) + 1.0) * width);
    return PARIS_HIP_SUCCESS;
}

namespace
{
    // what both quantise entry points refuse; *bytes: what the destination holds
    int vw_check_call(const float* d_v, uint64_t n, const paris_hip_volume_window* setting, const void* q, float* scale, uint32_t* elem, size_t* bytes)
    {
        if(d_v == nullptr || q == nullptr || !vw_setting_scale(setting, scale, elem))
            return PARIS_HIP_ERROR_INVALID_ARGUMENT;
        if(reinterpret_cast<uintptr_t>(d_v) % sizeof(float) != 0u || reinterpret_cast<uintptr_t>(q) % *elem != 0u)
            return PARIS_HIP_ERROR_INVALID_ARGUMENT;
        if(n > (~uint64_t{0}) / sizeof(float))
            return PARIS_HIP_ERROR_INVALID_ARGUMENT;
        *bytes = static_cast<size_t>(n) * *elem;
        return PARIS_HIP_SUCCESS;
    }
}

extern "C" int paris_hip_volume_quantize(paris_hip_ctx* ctx, const float* d_v, uint64_t n_voxels, const paris_hip_volume_window* setting, void* d_q)
{
    if(int rc = paris_hip_flush_deferred(ctx))
        return rc;
    if(int rc = paris_hip_bind(ctx))
        return rc;
    float scale = 0.f;
    uint32_t elem = 0;
    size_t bytes = 0;
    if(int rc = vw_check_call(d_v, n_voxels, setting, d_q, &scale, &elem, &bytes))
        return rc;
    const uintptr_t v0 = reinterpret_cast<uintptr_t>(d_v), q0 = reinterpret_cast<uintptr_t>(d_q);
    if(n_voxels != 0u && v0 < q0 + bytes && q0 < v0 + n_voxels * sizeof(float))
        return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    if(n_voxels == 0u)
        return PARIS_HIP_SUCCESS;
    if(int rc = paris_hip_volume_mark_dirty(ctx, d_q, bytes)) // a volume the destination overlaps holds arbitrary bits from here on
        return rc;
    if(int rc = vw_launch_quantize(ctx, d_v, n_voxels, setting, scale, elem, d_q))
        return rc;
    return paris_hip_finish(ctx);
}

extern "C" int paris_hip_volume_quantize_d2h(paris_hip_ctx* ctx, const float* d_v, uint64_t n_voxels, const paris_hip_volume_window* setting,
                                             void* h_q)
{
    if(int rc = paris_hip_flush_deferred(ctx))
        return rc;
    if(int rc = paris_hip_bind(ctx))
        return rc;
    float scale = 0.f;
    uint32_t elem = 0;
    size_t bytes = 0;
    if(int rc = vw_check_call(d_v, n_voxels, setting, h_q, &scale, &elem, &bytes))
        return rc;
    if(n_voxels == 0u)
        return PARIS_HIP_SUCCESS;
    paris_hip_ctx::volume_window_t& vw = ctx->volume_window;
    if(bytes > vw.stage.bytes)
    {
        // work already queued still copies out of the old scratch: it is retired, not freed
        const size_t want = (bytes + 255u) & ~static_cast<size_t>(255u);
        char* d = nullptr;
        if(int rc = paris_hip_device_malloc(ctx, reinterpret_cast<void**>(&d), want))
            return rc;
        paris_hip_retire_device_buffer(ctx, vw.stage.d, false);
        paris_hip_sweep_retired(ctx, false);
        vw.stage = paris_hip_device_buffer{d, want};
    }
    if(int rc = vw_launch_quantize(ctx, d_v, n_voxels, setting, scale, elem, vw.stage.d))
        return rc;
    PARIS_HIP_TRY(hipMemcpyAsync(h_q, vw.stage.d, bytes, hipMemcpyDeviceToHost, ctx->stream));
    paris_hip_note_host_use(ctx, h_q, paris_hip_ctx::USED_COMPUTE);
    return paris_hip_finish(ctx);
}

extern "C" int paris_hip_volume_quantize_counts(paris_hip_ctx* ctx, paris_hip_volume_counts* out, int reset)
{
    if(int rc = paris_hip_flush_deferred(ctx))
        return rc;
    if(int rc = paris_hip_bind(ctx))
        return rc;
    if(out == nullptr)
        return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    paris_hip_ctx::volume_window_t& vw = ctx->volume_window;
    unsigned long long acc[3] = {0, 0, 0};
    if(vw.mem.d != nullptr)
    {
        PARIS_HIP_TRY(hipMemcpyAsync(acc, vw.mem.as<char>() + VW_QUANT_OFFSET, sizeof(acc), hipMemcpyDeviceToHost, ctx->stream));
        if(reset)
            PARIS_HIP_TRY(hipMemsetAsync(vw.mem.as<char>() + VW_QUANT_OFFSET, 0, VW_STATS_OFFSET - VW_QUANT_OFFSET, ctx->stream));
    }
    PARIS_HIP_TRY(hipStreamSynchronize(ctx->stream));
    out->voxels = vw.voxels;
    out->below = acc[0];
    out->above = acc[1];
    out->not_finite = acc[2];
    if(reset)
        vw.voxels = 0;
    return PARIS_HIP_SUCCESS;
}

extern "C" int paris_hip_volume_stats(paris_hip_ctx* ctx, const float* d_v, uint64_t n_voxels, float h_lo, float h_hi, uint32_t n_bins,
                                      uint64_t* hist, paris_hip_volume_statistics* out)
{
    if(int rc = paris_hip_flush_deferred(ctx))
        return rc;
    if(int rc = paris_hip_bind(ctx))
        return rc;
    if(d_v == nullptr || out == nullptr || reinterpret_cast<uintptr_t>(d_v) % sizeof(float) != 0u || n_bins > PARIS_HIP_VOLUME_HISTOGRAM_BINS_MAX
       || n_voxels > (~uint64_t{0}) / sizeof(float))
        return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    float bscale = 0.f;
    if(n_bins != 0u && (hist == nullptr || !vw_scale(h_lo, h_hi, static_cast<double>(n_bins), &bscale)))
        return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    struct
    {
        uint32_t ext[2];
        unsigned long long cnt[3];
    } head = {{0u, 0u}, {0ull, 0ull, 0ull}};
    static_assert(sizeof(head) == VW_BINS_OFFSET - VW_STATS_OFFSET, "the stats results are 32 bytes");
    if(n_voxels != 0u)
    {
        if(int rc = vw_ensure_acc(ctx))
            return rc;
        char* d = ctx->volume_window.mem.as<char>();
        PARIS_HIP_TRY(hipMemsetAsync(d + VW_STATS_OFFSET, 0, sizeof(head) + sizeof(uint64_t) * n_bins, ctx->stream));
        const uint64_t items = std::max<uint64_t>(1u, n_voxels / 4u);
        const uint32_t blocks = static_cast<uint32_t>(std::min<uint64_t>(VW_STATS_GRID_MAX, (items + VW_THREADS - 1u) / VW_THREADS));
        const auto kernel = n_bins != 0u ? &volume_stats_kernel<true> : &volume_stats_kernel<false>;
        hipLaunchKernelGGL(kernel, dim3(blocks), dim3(VW_THREADS), 0, ctx->stream, d_v, n_voxels, h_lo, h_hi, bscale, n_bins,
                           reinterpret_cast<uint32_t*>(d + VW_STATS_OFFSET), reinterpret_cast<unsigned long long*>(d + VW_STATS_OFFSET + 8u),
                           reinterpret_cast<unsigned long long*>(d + VW_BINS_OFFSET));
        PARIS_HIP_TRY(hipGetLastError());
        PARIS_HIP_TRY(hipMemcpyAsync(&head, d + VW_STATS_OFFSET, sizeof(head), hipMemcpyDeviceToHost, ctx->stream));
        if(n_bins != 0u)
            PARIS_HIP_TRY(hipMemcpyAsync(hist, d + VW_BINS_OFFSET, sizeof(uint64_t) * n_bins, hipMemcpyDeviceToHost, ctx->stream));
    }
    else
        for(uint32_t b = 0; b < n_bins; ++b)
            hist[b] = 0u;
    PARIS_HIP_TRY(hipStreamSynchronize(ctx->stream));
    out->min = head.ext[0] != 0u ? vw_decode(~head.ext[0]) : INFINITY;
    out->max = head.ext[1] != 0u ? vw_decode(head.ext[1]) : -INFINITY;
    out->below = head.cnt[0];
    out->above = head.cnt[1];
    out->not_finite = head.cnt[2];
    out->voxels = n_voxels;
    return PARIS_HIP_SUCCESS;
}

void paris_hip_warm_volume_window()
{
    hipFuncAttributes a{};
    (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&volume_quantize_kernel<PARIS_HIP_VOXEL_U8, true>));
    (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&volume_quantize_kernel<PARIS_HIP_VOXEL_U8, false>));
    (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&volume_quantize_kernel<PARIS_HIP_VOXEL_U16, true>));
    (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&volume_quantize_kernel<PARIS_HIP_VOXEL_U16, false>));
    (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&volume_stats_kernel<true>));
    (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&volume_stats_kernel<false>));
}
