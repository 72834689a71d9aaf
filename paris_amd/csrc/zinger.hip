// Removal of per-frame outlier pixels ("zingers") for gfx950 (the statement is in include/paris_hip.h).
//
// The ctx holds one setting: the rule's parameters and one scratch buffer -- three 64-bit accumulators, then per frame of one launch
// max_hits (index, value) pairs, then per frame a hit counter. paris_hip_zinger_filter_rows is, per launch of up to `frames` frames, a
// memset of the counters and two kernels on the compute stream:
//   zinger_detect_kernel  reads every pixel of the band once (plus one row beyond each strip of rows), writes only the hit list;
//   zinger_apply_kernel   writes the listed medians into the frames whose count fits max_hits, and adds to the accumulators.
// Detect never writes a frame and apply never reads one, so every window sees the frame as it was before the call; the kernel boundary
// is the only ordering needed. The hit count is a sum of integers and the list's content a set, so neither depends on scheduling.
#include <algorithm>
#include <cmath>

#include "frame_pass.h"

namespace
{
    constexpr uint32_t ZD_LANES = 64u;  // one wave per strip: the hit list is appended per wave
    constexpr uint32_t ZD_WAVES = 4u;   // strips per block
    constexpr uint32_t ZD_ROWS = 16u;   // rows per strip: 18 rows read for 16 examined
    constexpr uint32_t ZD_PX = 4u;      // consecutive pixels per lane: one 16-byte load
    constexpr uint32_t ZD_MAX_GRID_Y = 65535u;
    constexpr uint32_t ZA_THREADS = 256u;
    constexpr size_t Z_ACC_BYTES = 32u;               // three 64-bit accumulators, padded: the pairs behind them stay 8-byte aligned
    constexpr size_t Z_SCRATCH_BUDGET = size_t{4} << 20; // what the frames of one launch may occupy when more than one fits

    // columns x0 - 1 .. x0 + 4 of one row, clamped to [0, x_last]: v[k] is column x0 - 1 + k. VEC: the lane's own four columns exist
    // and sit on a 16-byte boundary.
    template <bool VEC>
    __device__ __forceinline__ void zinger_load_row(const float* __restrict__ row, uint32_t x0, uint32_t x_last, float (&v)[ZD_PX + 2u])
    {
        if(VEC)
        {
            const float4 q = *reinterpret_cast<const float4*>(row + x0);
            v[1] = q.x;
            v[2] = q.y;
            v[3] = q.z;
            v[4] = q.w;
        }
        else
        {
#pragma unroll
            for(uint32_t i = 0; i < ZD_PX; ++i)
                v[1u + i] = row[x0 + min(i, x_last - x0)];
        }
        v[0] = row[x0 - (x0 != 0u ? 1u : 0u)];
        v[ZD_PX + 1u] = row[x0 + min(ZD_PX, x_last - x0)];
    }

    __device__ __forceinline__ float zinger_min3(float a, float b, float c)
    {
        return __builtin_fminf(__builtin_fminf(a, b), c);
    }
    __device__ __forceinline__ float zinger_max3(float a, float b, float c)
    {
        return __builtin_fmaxf(__builtin_fmaxf(a, b), c);
    }
    __device__ __forceinline__ float zinger_med3(float a, float b, float c)
    {
        return __builtin_amdgcn_fmed3f(a, b, c);
    }

    // p: row 0 of this launch's first frame; frames on grid z, strips of ZD_ROWS band rows on grid x (ZD_WAVES per block), groups of
    // ZD_LANES * ZD_PX columns on grid y from col_block_first. A lane owns ZD_PX pixels of a row and walks down its strip with the rows
    // y - 1, y, y + 1 in registers; each column's vertical triple is sorted once and serves the three windows it belongs to.
    // VEC (16-byte loads) is the host's choice per launch, for frames whose base and pitch are multiples of 16 bytes and whose dim_x
    // is a multiple of ZD_PX; every other frame takes the scalar loads: no lane of a launch differs from another in how it loads.
    template <bool VEC>
    __global__ void __launch_bounds__(ZD_LANES* ZD_WAVES)
        zinger_detect_kernel(const char* __restrict__ p, size_t frame_stride, size_t pitch_f, uint32_t dim_x, uint32_t dim_y, uint32_t row_first,
                             uint32_t row_end, uint32_t col_block_first, float t_abs, float t_rel, int polarity, uint32_t max_hits,
                             uint32_t* __restrict__ count, uint2* __restrict__ pairs)
    {
        const uint64_t strip = static_cast<uint64_t>(blockIdx.x) * ZD_WAVES + threadIdx.y;
        const uint64_t strip_row = row_first + strip * ZD_ROWS;
        if(strip_row >= row_end) // (wave-uniform: a wave is one strip)
            return;
        const uint32_t ys = static_cast<uint32_t>(strip_row), ye = ys + min(ZD_ROWS, row_end - ys);
        const uint32_t f = blockIdx.z;
        const float* frame = reinterpret_cast<const float*>(p + static_cast<size_t>(f) * frame_stride);
        const uint64_t column = ((static_cast<uint64_t>(col_block_first) + blockIdx.y) * ZD_LANES + threadIdx.x) * ZD_PX;
        const bool live = column < dim_x; // the other lanes stay for the ballots, on column 0
        const uint32_t x_last = dim_x - 1u, y_last = dim_y - 1u, x0 = live ? static_cast<uint32_t>(column) : 0u;
        const uint32_t owned = live ? min(ZD_PX, x_last - x0 + 1u) : 0u;

        // One load site for every row: the walk starts two rows early (rows ys - 1 and ys only fill the window), so that no
        // separately compiled prologue has to agree with the loop about where the window's rows live.
        float a[ZD_PX + 2u] = {}, b[ZD_PX + 2u] = {}, c[ZD_PX + 2u];
        const uint32_t steps = ye - ys + 2u;
        for(uint32_t r = 0; r < steps; ++r)
        {
            const uint64_t below = static_cast<uint64_t>(ys) + r; // the row to load, plus one: ys - 1 + r, clamped to the frame
            const uint32_t row = below == 0u ? 0u : static_cast<uint32_t>(min(below - 1u, static_cast<uint64_t>(y_last)));
            zinger_load_row<VEC>(frame + static_cast<size_t>(row) * pitch_f, x0, x_last, c);
            if(r < 2u) // (wave-uniform)
            {
#pragma unroll
                for(uint32_t k = 0; k < ZD_PX + 2u; ++k)
                {
                    a[k] = b[k];
                    b[k] = c[k];
                }
                continue;
            }
            const uint32_t y = ys + r - 2u; // the window's middle row
            float lo[ZD_PX + 2u], mid[ZD_PX + 2u], hi[ZD_PX + 2u];
            bool finite[ZD_PX + 2u];
#pragma unroll
            for(uint32_t k = 0; k < ZD_PX + 2u; ++k)
            {
                lo[k] = zinger_min3(a[k], b[k], c[k]);
                mid[k] = zinger_med3(a[k], b[k], c[k]);
                hi[k] = zinger_max3(a[k], b[k], c[k]);
                finite[k] = __builtin_isfinite(a[k]) && __builtin_isfinite(b[k]) && __builtin_isfinite(c[k]);
            }
            float m[ZD_PX];
            bool hit[ZD_PX];
            bool any = false;
#pragma unroll
            for(uint32_t i = 0; i < ZD_PX; ++i)
            {
                m[i] = zinger_med3(zinger_max3(lo[i], lo[i + 1u], lo[i + 2u]), zinger_med3(mid[i], mid[i + 1u], mid[i + 2u]),
                                   zinger_min3(hi[i], hi[i + 1u], hi[i + 2u]));
                const float d = b[i + 1u] - m[i];
                const float lim = t_abs + t_rel * __builtin_fabsf(m[i]); // (a multiply, then an add: contraction is off in this library)
                const float s = polarity > 0 ? d : (polarity < 0 ? -d : __builtin_fabsf(d));
                hit[i] = i < owned && finite[i] && finite[i + 1u] && finite[i + 2u] && s > lim;
                any = any || hit[i];
            }
            if(__ballot(any) != 0ull) // (wave-uniform, and rare: a few rows of a frame hold a hit)
            {
                // one counter update per wave: the ballots give every hit its rank among the wave's
                unsigned long long mask[ZD_PX];
                uint32_t total = 0;
#pragma unroll
                for(uint32_t i = 0; i < ZD_PX; ++i)
                {
                    mask[i] = __ballot(hit[i]);
                    total += static_cast<uint32_t>(__popcll(mask[i]));
                }
                uint32_t base = 0;
                if(threadIdx.x == 0u)
                    base = atomicAdd(&count[f], total); // (keeps counting past max_hits: the apply kernel reads the true count)
                base = __builtin_amdgcn_readfirstlane(base);
#pragma unroll
                for(uint32_t i = 0; i < ZD_PX; ++i)
                {
                    if(hit[i])
                    {
                        const uint32_t rank = __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(mask[i] >> 32),
                                                                        __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(mask[i]), 0u));
                        const uint64_t pos = static_cast<uint64_t>(base) + rank;
                        if(pos < max_hits)
                            pairs[static_cast<size_t>(f) * max_hits + pos] = make_uint2(y * dim_x + x0 + i, __float_as_uint(m[i]));
                    }
                    base += static_cast<uint32_t>(__popcll(mask[i]));
                }
            }
#pragma unroll
            for(uint32_t k = 0; k < ZD_PX + 2u; ++k)
            {
                a[k] = b[k];
                b[k] = c[k];
            }
        }
    }

    // one lane per (slot of the hit list on grid x, frame on grid y); acc: frames, replaced, saturated_frames
    __global__ void __launch_bounds__(ZA_THREADS)
        zinger_apply_kernel(char* __restrict__ p, size_t frame_stride, size_t pitch_f, uint32_t dim_x, uint32_t max_hits,
                            const uint32_t* __restrict__ count, const uint2* __restrict__ pairs, unsigned long long* __restrict__ acc)
    {
        const uint32_t f = blockIdx.y;
        const uint64_t slot = static_cast<uint64_t>(blockIdx.x) * ZA_THREADS + threadIdx.x;
        const uint32_t n = count[f];
        const bool saturated = n > max_hits; // the frame stays as it was
        if(slot == 0u)
        {
            atomicAdd(&acc[0], 1ull);
            atomicAdd(&acc[saturated ? 2 : 1], saturated ? 1ull : static_cast<unsigned long long>(n));
        }
        if(saturated || slot >= n)
            return;
        const uint2 e = pairs[static_cast<size_t>(f) * max_hits + slot];
        const uint32_t y = e.x / dim_x, x = e.x - y * dim_x;
        float* frame = reinterpret_cast<float*>(p + static_cast<size_t>(f) * frame_stride);
        frame[static_cast<size_t>(y) * pitch_f + x] = __uint_as_float(e.y);
    }

    // how many frames one launch serves: as many as fit the budget, one at least, PARIS_HIP_ZINGER_FRAMES_MAX at most
    uint32_t zinger_frames_per_launch(uint32_t max_hits)
    {
        const size_t per_frame = sizeof(uint2) * static_cast<size_t>(max_hits) + sizeof(uint32_t);
        return static_cast<uint32_t>(std::min<size_t>(PARIS_HIP_ZINGER_FRAMES_MAX, std::max<size_t>(1u, Z_SCRATCH_BUDGET / per_frame)));
    }
}

extern "C" int paris_hip_zinger_filter_check(const paris_hip_zinger_filter* zf, uint32_t dim_x, uint32_t dim_y, uint32_t* max_hits,
                                             size_t* device_bytes)
{
    if(zf == nullptr || dim_x == 0 || dim_y == 0)
        return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    if(!std::isfinite(zf->threshold_abs) || !std::isfinite(zf->threshold_rel) || zf->threshold_abs < 0.f || zf->threshold_rel < 0.f
       || (zf->threshold_abs == 0.f && zf->threshold_rel == 0.f) || zf->polarity < -1 || zf->polarity > 1)
        return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    const uint64_t n = static_cast<uint64_t>(dim_x) * dim_y;
    if(zf->max_hits > n)
        return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    if(n > 0xffffffffull) // (a hit is listed by its 32-bit pixel index)
        return PARIS_HIP_ERROR_UNSUPPORTED;
    const uint32_t hits = zf->max_hits != 0u ? zf->max_hits : static_cast<uint32_t>(std::min<uint64_t>(n, std::max<uint64_t>(1024u, n / 256u)));
    if(max_hits != nullptr)
        *max_hits = hits;
    if(device_bytes != nullptr)
        *device_bytes = Z_ACC_BYTES + zinger_frames_per_launch(hits) * (sizeof(uint2) * static_cast<size_t>(hits) + sizeof(uint32_t));
    return PARIS_HIP_SUCCESS;
}

extern "C" int paris_hip_set_zinger_filter(paris_hip_ctx* ctx, const paris_hip_zinger_filter* zf, uint32_t dim_x, uint32_t dim_y)
{
    if(int rc = paris_hip_bind(ctx))
        return rc;
    uint32_t hits = 0;
    size_t bytes = 0;
    if(int rc = paris_hip_zinger_filter_check(zf, dim_x, dim_y, &hits, &bytes))
        return rc;
    paris_hip_device_buffer mem; // the accumulators start at zero
    if(int rc = paris_hip_install(ctx, bytes, {{0u, nullptr, Z_ACC_BYTES}}, &mem))
        return rc;
    paris_hip_ctx::zinger_t& z = ctx->zinger;
    paris_hip_release(ctx, z);
    z.set = true;
    z.rule = *zf;
    z.rule.max_hits = hits;
    z.dim_x = dim_x;
    z.dim_y = dim_y;
    z.frames = zinger_frames_per_launch(hits);
    z.mem = mem;
    return PARIS_HIP_SUCCESS;
}

extern "C" int paris_hip_clear_zinger_filter(paris_hip_ctx* ctx)
{
    if(int rc = paris_hip_bind(ctx))
        return rc;
    paris_hip_release(ctx, ctx->zinger);
    return PARIS_HIP_SUCCESS;
}

extern "C" int paris_hip_zinger_filter_rows(paris_hip_ctx* ctx, float* d_p, size_t pitch, size_t frame_stride, uint32_t n_frames, uint32_t dim_x,
                                            uint32_t dim_y, uint32_t row_first, uint32_t row_count)
{
    const paris_hip_frame_band band{d_p, pitch, frame_stride, n_frames, dim_x, dim_y, row_first, row_count};
    const auto refuse = [&]() -> int {
        const paris_hip_ctx::zinger_t& z = ctx->zinger;
        return !z.set || dim_x != z.dim_x || dim_y != z.dim_y ? PARIS_HIP_ERROR_INVALID_ARGUMENT : PARIS_HIP_SUCCESS;
    };
    int memset_rc = PARIS_HIP_SUCCESS; // of a launch's counter memset: nothing more is enqueued after a failure
    const auto launch = [&] {
        const paris_hip_ctx::zinger_t& z = ctx->zinger;
        const uint32_t hits = z.rule.max_hits;
        unsigned long long* acc = z.mem.as<unsigned long long>();
        uint2* pairs = reinterpret_cast<uint2*>(z.mem.as<char>() + Z_ACC_BYTES);
        uint32_t* count = reinterpret_cast<uint32_t*>(pairs + static_cast<size_t>(z.frames) * hits);
        const uint32_t strips = (row_count + ZD_ROWS - 1u) / ZD_ROWS;
        const bool vec = dim_x % ZD_PX == 0u && pitch % 16u == 0u && frame_stride % 16u == 0u && reinterpret_cast<uintptr_t>(d_p) % 16u == 0u;
        const auto detect = vec ? &zinger_detect_kernel<true> : &zinger_detect_kernel<false>;
        const uint64_t col_blocks = (static_cast<uint64_t>(dim_x) + ZD_LANES * ZD_PX - 1u) / (ZD_LANES * ZD_PX);
        // larger calls loop: the launches share the scratch, in stream order
        for(uint32_t f0 = 0; f0 < n_frames; f0 += z.frames)
        {
            const uint32_t nf = std::min(z.frames, n_frames - f0);
            memset_rc = static_cast<int>(hipMemsetAsync(count, 0, nf * sizeof(uint32_t), ctx->stream));
            if(memset_rc != PARIS_HIP_SUCCESS)
                return; // (returned below; frames of earlier launches of this call have been filtered)
            for(uint64_t c0 = 0; c0 < col_blocks; c0 += ZD_MAX_GRID_Y)
                hipLaunchKernelGGL(detect, dim3((strips + ZD_WAVES - 1u) / ZD_WAVES, static_cast<uint32_t>(std::min<uint64_t>(ZD_MAX_GRID_Y, col_blocks - c0)), nf),
                                   dim3(ZD_LANES, ZD_WAVES), 0, ctx->stream, band.frame(f0), frame_stride, pitch / sizeof(float), dim_x, dim_y, row_first,
                                   row_first + row_count, static_cast<uint32_t>(c0), z.rule.threshold_abs, z.rule.threshold_rel, z.rule.polarity, hits, count,
                                   pairs);
            hipLaunchKernelGGL(zinger_apply_kernel, dim3((hits + ZA_THREADS - 1u) / ZA_THREADS, nf), dim3(ZA_THREADS), 0, ctx->stream, band.frame(f0),
                               frame_stride, pitch / sizeof(float), dim_x, hits, count, pairs, acc);
        }
    };
    const auto touched = [&] { // the windows reach one row beyond the band on either side
        const uint32_t end = row_first + row_count, lo = row_first - std::min(row_first, 1u);
        return paris_hip_row_range{lo, end + std::min(dim_y - end, 1u) - lo};
    };
    const int rc = paris_hip_frame_pass(ctx, band, refuse, [] { return false; }, launch, touched);
    return memset_rc != PARIS_HIP_SUCCESS ? memset_rc : rc;
}

extern "C" int paris_hip_zinger_stats(paris_hip_ctx* ctx, paris_hip_zinger_counts* out, int reset)
{
    if(int rc = paris_hip_bind(ctx))
        return rc;
    if(out == nullptr || !ctx->zinger.set)
        return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    if(int rc = paris_hip_flush_pending_weight(ctx))
        return rc;
    unsigned long long acc[3] = {0, 0, 0};
    PARIS_HIP_TRY(hipMemcpyAsync(acc, ctx->zinger.mem.d, sizeof(acc), hipMemcpyDeviceToHost, ctx->stream));
    if(reset)
        PARIS_HIP_TRY(hipMemsetAsync(ctx->zinger.mem.d, 0, Z_ACC_BYTES, ctx->stream));
    PARIS_HIP_TRY(hipStreamSynchronize(ctx->stream));
    out->frames = acc[0];
    out->replaced = acc[1];
    out->saturated_frames = acc[2];
    return PARIS_HIP_SUCCESS;
}

void paris_hip_warm_zinger()
{
    hipFuncAttributes a{};
    (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&zinger_detect_kernel<true>));
    (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&zinger_detect_kernel<false>));
    (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&zinger_apply_kernel));
}
