// Normalisation of every frame to an air region for gfx950 (the statement is in include/paris_hip.h).
//
// The ctx holds one setting: the rule's parameters and one device buffer (paris_hip_air_layout_of) -- the counters, the values and
// counts of one launch, the rectangle's mask bytes. paris_hip_air_normalize_rows is, per launch pair of up to
// PARIS_HIP_AIR_FRAMES_MAX frames, two kernels on the compute stream:
//   air_value_kernel     one 256-lane workgroup per frame reads the rectangle once and leaves a_f, the count and the counters;
//   air_subtract_kernel  p <- p - a_f over the band's rows of every frame whose a_f is not zero, and touches nothing else.
// The first never writes a frame and the second reads a_f only, so the rectangle is measured as it was before the call, also when
// it lies inside the band; the kernel boundary is the only ordering needed. Every partial sum has one owner and lane 0 adds them in
// ascending order: no floating-point atomics, and the value is the statement's whatever the grid.
#include <algorithm>
#include <cmath>
#include <limits>

#include "frame_pass.h"

namespace
{
    constexpr uint32_t AIR_THREADS = 256u;
    constexpr uint32_t AIR_WAVE_COLUMNS = 64u; // a wave reads 64 consecutive columns of a row
    constexpr uint32_t AIR_ROW_STEP = AIR_THREADS / AIR_WAVE_COLUMNS;
    constexpr uint32_t AIR_BATCH = 16u;        // pixels a lane loads before it adds them, in order
    constexpr uint32_t AIR_MAX_BLOCKS = 4096u; // memory bound: cap the grid and stride over the rest (as ring.hip)

    // the counters of the normalise calls, as they lie at the start of the ctx's buffer
    struct air_counters
    {
        unsigned long long frames, normalised, too_few, above_limit;
        uint32_t min_key, max_key; // ordered keys of the smallest and the largest kept value
    };
    static_assert(sizeof(air_counters) <= PARIS_HIP_AIR_COUNTER_BYTES, "the counters fit their slot");

    // fp32 values as unsigned integers that compare as the values do (-0 below +0)
    __host__ __device__ inline uint32_t air_key(uint32_t bits)
    {
        return (bits & 0x80000000u) != 0u ? ~bits : bits | 0x80000000u;
    }
    inline float air_unkey(uint32_t key)
    {
        const uint32_t bits = (key & 0x80000000u) != 0u ? key & 0x7fffffffu : ~key;
        float v;
        static_assert(sizeof(v) == sizeof(bits), "fp32");
        __builtin_memcpy(&v, &bits, sizeof(v));
        return v;
    }
    air_counters air_counters_empty()
    {
        air_counters c{};
        c.min_key = air_key(0x7f800000u); // +inf
        c.max_key = air_key(0xff800000u); // -inf
        return c;
    }

    // p: row 0 of this launch's first frame; one workgroup per frame on grid x. Lane l owns partial sum l: columns x0 + l % 64,
    // + 64, ... of rows y0 + l / 64, + 4, ..., both ascending. mask: the rectangle's bytes, rows `width` apart. acc == nullptr (the
    // measure call): the counters stay as they are.
    __global__ void __launch_bounds__(AIR_THREADS)
        air_value_kernel(const char* __restrict__ p, size_t frame_stride, size_t pitch_f, uint32_t x0, uint32_t y0, uint32_t width,
                         uint32_t height, uint32_t min_pixels, float limit_abs, const uint8_t* __restrict__ mask, float* __restrict__ value,
                         uint32_t* __restrict__ count, air_counters* __restrict__ acc)
    {
        __shared__ double part_sum[AIR_THREADS];
        __shared__ uint32_t part_n[AIR_THREADS];
        const uint32_t f = blockIdx.x, l = threadIdx.x;
        const float* frame = reinterpret_cast<const float*>(p + static_cast<size_t>(f) * frame_stride);
        double s = 0.0;
        uint32_t n = 0;
        // The lane's pixels in the rule's order -- rows ascending, columns ascending within a row -- AIR_BATCH at a time: the loads of
        // a batch are independent and issued together, the additions follow one by one in order. A lane's walk is a chain of
        // dependent additions, and with one load per addition the kernel would wait out the memory latency once per pixel.
        const uint32_t c = l % AIR_WAVE_COLUMNS, r = l / AIR_WAVE_COLUMNS;
        uint32_t x = c, y = c < width ? r : height; // the cursor; y >= height: the lane is done
        while(y < height)
        {
            float v[AIR_BATCH];
            uint8_t bad[AIR_BATCH];
            uint32_t live = 0; // bit k: slot k holds a pixel of the lane (the others reload its first pixel and are not added)
#pragma unroll
            for(uint32_t k = 0; k < AIR_BATCH; ++k)
            {
                const bool more = y < height;
                const uint32_t px = more ? x : c, py = more ? y : r;
                v[k] = frame[static_cast<size_t>(y0 + py) * pitch_f + x0 + px];
                bad[k] = mask[static_cast<size_t>(py) * width + px];
                live |= (more ? 1u : 0u) << k;
                x += AIR_WAVE_COLUMNS;
                if(x >= width)
                {
                    x = c;
                    y = more ? y + AIR_ROW_STEP : y;
                }
            }
#pragma unroll
            for(uint32_t k = 0; k < AIR_BATCH; ++k)
                if((live >> k & 1u) != 0u && bad[k] == 0u && __builtin_isfinite(v[k]))
                {
                    s += static_cast<double>(v[k]);
                    ++n;
                }
        }
        part_sum[l] = s;
        part_n[l] = n;
        __syncthreads();
        if(l != 0u)
            return;
        double total = part_sum[0];
        uint32_t pixels = part_n[0];
        for(uint32_t k = 1; k < AIR_THREADS; ++k) // ascending, one double addition each
        {
            total = total + part_sum[k];
            pixels += part_n[k];
        }
        float a = 0.f;
        const bool too_few = pixels < min_pixels;
        bool above = false;
        if(!too_few)
        {
            a = static_cast<float>(total / static_cast<double>(pixels));
            above = limit_abs != 0.f && __builtin_fabsf(a) > limit_abs;
            if(above)
                a = 0.f;
        }
        value[f] = a;
        count[f] = pixels;
        if(acc != nullptr)
        {
            atomicAdd(&acc->frames, 1ull);
            atomicAdd(too_few ? &acc->too_few : (above ? &acc->above_limit : &acc->normalised), 1ull);
            if(!too_few && !above)
            {
                const uint32_t key = air_key(__float_as_uint(a));
                atomicMin(&acc->min_key, key);
                atomicMax(&acc->max_key, key);
            }
        }
    }

    // The band's pixels are dealt to the lanes of grid x as one list, row after row, `groups_x` lanes per row (as ring.hip); frames on
    // grid y, strided. A workgroup reads a_f once per frame and skips the frame before any load when it is zero.
    template <bool VEC>
    __global__ void __launch_bounds__(AIR_THREADS)
        air_subtract_kernel(char* __restrict__ p, size_t frame_stride, uint32_t n_frames, size_t pitch_f, uint32_t row_first, uint32_t groups_x,
                            uint64_t lanes, const float* __restrict__ value)
    {
        constexpr uint32_t PER_LANE = VEC ? 4u : 1u;
        for(uint32_t f = blockIdx.y; f < n_frames; f += gridDim.y)
        {
            const float a = value[f];
            if(a == 0.f) // (workgroup-uniform; zero of either sign: the frame is not written)
                continue;
            char* frame = p + static_cast<size_t>(f) * frame_stride;
            for(uint64_t i = static_cast<uint64_t>(blockIdx.x) * AIR_THREADS + threadIdx.x; i < lanes; i += static_cast<uint64_t>(gridDim.x) * AIR_THREADS)
            {
                const uint32_t row = row_first + static_cast<uint32_t>(i / groups_x);
                const uint32_t col = static_cast<uint32_t>(i % groups_x) * PER_LANE;
                float* q = reinterpret_cast<float*>(frame) + static_cast<size_t>(row) * pitch_f + col;
                if constexpr(VEC)
                {
                    const float4 v = *reinterpret_cast<const float4*>(q);
                    *reinterpret_cast<float4*>(q) = make_float4(v.x - a, v.y - a, v.z - a, v.w - a);
                }
                else
                    *q = *q - a;
            }
        }
    }

    bool air_vector_rows(const paris_hip_frame_band& b)
    {
        return b.dim_x % 4u == 0 && b.pitch % 16u == 0 && reinterpret_cast<uintptr_t>(b.d_p) % 16u == 0
               && (b.n_frames == 1u || b.frame_stride % 16u == 0);
    }

    // the value kernel for frames [f0, f0 + nf) of the band's frames, into the launch's slots
    void air_launch_values(paris_hip_ctx* ctx, const paris_hip_frame_band& b, uint32_t f0, uint32_t nf, bool counted)
    {
        const paris_hip_ctx::air_t& s = ctx->air;
        const paris_hip_air_layout lay = paris_hip_air_layout_of(s.rule.width, s.rule.height);
        char* d_mem = s.mem.as<char>();
        hipLaunchKernelGGL(air_value_kernel, dim3(nf), dim3(AIR_THREADS), 0, ctx->stream, b.frame(f0), b.frame_stride, b.pitch / sizeof(float),
                           s.rule.x0, s.rule.y0, s.rule.width, s.rule.height, s.rule.min_pixels, s.rule.limit_abs,
                           reinterpret_cast<const uint8_t*>(d_mem + lay.mask), reinterpret_cast<float*>(d_mem + lay.value),
                           reinterpret_cast<uint32_t*>(d_mem + lay.count), counted ? reinterpret_cast<air_counters*>(d_mem) : nullptr);
    }

    int air_refuse(const paris_hip_ctx* ctx, uint32_t dim_x, uint32_t dim_y)
    {
        const paris_hip_ctx::air_t& s = ctx->air;
        return !s.set || dim_x != s.dim_x || dim_y != s.dim_y ? PARIS_HIP_ERROR_INVALID_ARGUMENT : PARIS_HIP_SUCCESS;
    }
}

extern "C" int paris_hip_set_air_region(paris_hip_ctx* ctx, const paris_hip_air_region* ar, const uint8_t* mask, uint32_t dim_x, uint32_t dim_y)
{
    if(int rc = paris_hip_bind(ctx))
        return rc;
    uint32_t min_pixels = 0;
    size_t bytes = 0;
    if(int rc = paris_hip_air_region_check(ar, dim_x, dim_y, &min_pixels, &bytes))
        return rc;
    // the buffer's first content on the host: empty counters, the rectangle's mask bytes (zeros without a mask)
    const paris_hip_air_layout lay = paris_hip_air_layout_of(ar->width, ar->height);
    std::vector<char> init(bytes, 0);
    const air_counters empty = air_counters_empty();
    __builtin_memcpy(init.data(), &empty, sizeof(empty));
    if(mask != nullptr)
        for(uint32_t y = 0; y < ar->height; ++y)
            for(uint32_t x = 0; x < ar->width; ++x)
                init[lay.mask + static_cast<size_t>(y) * ar->width + x] = mask[static_cast<size_t>(ar->y0 + y) * dim_x + ar->x0 + x] != 0u ? 1 : 0;
    paris_hip_device_buffer mem;
    if(int rc = paris_hip_install(ctx, bytes, {{0u, init.data(), bytes}}, &mem))
        return rc;
    paris_hip_ctx::air_t& s = ctx->air;
    paris_hip_release(ctx, s);
    s.set = true;
    s.rule = *ar;
    s.rule.min_pixels = min_pixels;
    s.dim_x = dim_x;
    s.dim_y = dim_y;
    s.mem = mem;
    return PARIS_HIP_SUCCESS;
}

extern "C" int paris_hip_clear_air_region(paris_hip_ctx* ctx)
{
    if(int rc = paris_hip_bind(ctx))
        return rc;
    paris_hip_release(ctx, ctx->air);
    return PARIS_HIP_SUCCESS;
}

extern "C" int paris_hip_air_normalize_rows(paris_hip_ctx* ctx, float* d_p, size_t pitch, size_t frame_stride, uint32_t n_frames, uint32_t dim_x,
                                            uint32_t dim_y, uint32_t row_first, uint32_t row_count)
{
    const paris_hip_frame_band band{d_p, pitch, frame_stride, n_frames, dim_x, dim_y, row_first, row_count};
    const auto launch = [&] {
        const paris_hip_ctx::air_t& s = ctx->air;
        const float* value = reinterpret_cast<const float*>(s.mem.as<char>() + paris_hip_air_layout_of(s.rule.width, s.rule.height).value);
        const bool vec = air_vector_rows(band);
        const uint32_t groups_x = vec ? dim_x / 4u : dim_x;
        const uint64_t lanes = static_cast<uint64_t>(groups_x) * row_count;
        const uint32_t blocks = static_cast<uint32_t>(std::min<uint64_t>(AIR_MAX_BLOCKS, (lanes + AIR_THREADS - 1u) / AIR_THREADS));
        const auto subtract = vec ? &air_subtract_kernel<true> : &air_subtract_kernel<false>;
        // larger calls loop: the launch pairs share the values' slots, in stream order
        for(uint32_t f0 = 0; f0 < n_frames; f0 += PARIS_HIP_AIR_FRAMES_MAX)
        {
            const uint32_t nf = std::min<uint32_t>(PARIS_HIP_AIR_FRAMES_MAX, n_frames - f0);
            air_launch_values(ctx, band, f0, nf, true);
            hipLaunchKernelGGL(subtract, dim3(blocks, nf), dim3(AIR_THREADS), 0, ctx->stream, band.frame(f0), frame_stride, nf, pitch / sizeof(float),
                               row_first, groups_x, lanes, value);
        }
    };
    const auto touched = [&] { // the band's rows are written, the rectangle's read: one range that holds both
        const paris_hip_ctx::air_t& s = ctx->air;
        const uint32_t lo = std::min(row_first, s.rule.y0), hi = std::max(row_first + row_count, s.rule.y0 + s.rule.height);
        return paris_hip_row_range{lo, hi - lo};
    };
    return paris_hip_frame_pass(ctx, band, [&] { return air_refuse(ctx, dim_x, dim_y); }, [] { return false; }, launch, touched);
}

extern "C" int paris_hip_air_measure(paris_hip_ctx* ctx, const float* d_p, size_t pitch, size_t frame_stride, uint32_t n_frames, uint32_t dim_x,
                                     uint32_t dim_y, float* h_a, uint32_t* h_n)
{
    // the whole frame as the band: the scaffold's checks and guards, nothing written
    const paris_hip_frame_band band{const_cast<float*>(d_p), pitch, frame_stride, n_frames, dim_x, dim_y, 0u, dim_y};
    int copy_rc = PARIS_HIP_SUCCESS;
    const auto launch = [&] {
        const paris_hip_ctx::air_t& s = ctx->air;
        const paris_hip_air_layout lay = paris_hip_air_layout_of(s.rule.width, s.rule.height);
        // the launches share the values' slots: each one's results are copied down, in stream order, before the next
        for(uint32_t f0 = 0; f0 < n_frames && copy_rc == PARIS_HIP_SUCCESS; f0 += PARIS_HIP_AIR_FRAMES_MAX)
        {
            const uint32_t nf = std::min<uint32_t>(PARIS_HIP_AIR_FRAMES_MAX, n_frames - f0);
            air_launch_values(ctx, band, f0, nf, false);
            if(h_a != nullptr)
                copy_rc = static_cast<int>(hipMemcpyAsync(h_a + f0, s.mem.as<char>() + lay.value, nf * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
            if(h_n != nullptr && copy_rc == PARIS_HIP_SUCCESS)
                copy_rc = static_cast<int>(hipMemcpyAsync(h_n + f0, s.mem.as<char>() + lay.count, nf * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
            if(copy_rc == PARIS_HIP_SUCCESS) // (the host arrays may be pageable: each copy is complete before the slots are reused)
                copy_rc = static_cast<int>(hipStreamSynchronize(ctx->stream));
        }
    };
    const auto touched = [&] {
        const paris_hip_ctx::air_t& s = ctx->air;
        return paris_hip_row_range{s.rule.y0, s.rule.height};
    };
    const int rc = paris_hip_frame_pass(ctx, band, [&] { return air_refuse(ctx, dim_x, dim_y); }, [] { return false; }, launch, touched);
    if(copy_rc != PARIS_HIP_SUCCESS)
        return copy_rc;
    if(rc != PARIS_HIP_SUCCESS)
        return rc;
    PARIS_HIP_TRY(hipStreamSynchronize(ctx->stream));
    return PARIS_HIP_SUCCESS;
}

extern "C" int paris_hip_air_stats(paris_hip_ctx* ctx, paris_hip_air_counts* out, int reset)
{
    if(int rc = paris_hip_bind(ctx))
        return rc;
    if(out == nullptr || !ctx->air.set)
        return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    if(int rc = paris_hip_flush_pending_weight(ctx))
        return rc;
    air_counters acc{};
    const air_counters empty = air_counters_empty();
    PARIS_HIP_TRY(hipMemcpyAsync(&acc, ctx->air.mem.d, sizeof(acc), hipMemcpyDeviceToHost, ctx->stream));
    if(reset)
        PARIS_HIP_TRY(hipMemcpyAsync(ctx->air.mem.d, &empty, sizeof(empty), hipMemcpyHostToDevice, ctx->stream));
    PARIS_HIP_TRY(hipStreamSynchronize(ctx->stream));
    out->frames = acc.frames;
    out->normalised = acc.normalised;
    out->too_few = acc.too_few;
    out->above_limit = acc.above_limit;
    out->min_a = acc.normalised != 0u ? air_unkey(acc.min_key) : std::numeric_limits<float>::infinity();
    out->max_a = acc.normalised != 0u ? air_unkey(acc.max_key) : -std::numeric_limits<float>::infinity();
    return PARIS_HIP_SUCCESS;
}

void paris_hip_warm_air_region()
{
    hipFuncAttributes a{};
    (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&air_value_kernel));
    (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&air_subtract_kernel<true>));
    (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&air_subtract_kernel<false>));
}
