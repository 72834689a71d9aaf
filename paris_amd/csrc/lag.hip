// Detector lag correction for gfx950 (the statement is in include/paris_hip.h).
//
//   lag_kernel<TERMS, VEC>   the recursive deconvolution in place on the band's rows of the call's frames. A lane owns one pixel, or
//                            four columns as a float4, for the WHOLE call: it loads its TERMS (x 4) state words and its dark pixel(s)
//                            once, walks the frames in time order with the state in registers, and stores the state once at the end.
//                            The frames are loaded LAG_BATCH at a time, the next batch ahead of the arithmetic of the current one: the
//                            loads do not depend on the state, only the chain S -> x -> S is serial. The grid runs over the band's
//                            lanes -- no z over frames, frames are not independent here -- capped as bh_apply_kernel's, with a
//                            grid-stride loop. Memory bound: per pixel and call 8 n_frames + 8 TERMS bytes, plus 4 for the dark.
// The model's coefficients travel by value; the only thing on the device is the open sequence's state.
#include <algorithm>
#include <cmath>

#include "frame_pass.h"

namespace
{
    constexpr uint32_t LAG_THREADS = 256u;
    constexpr uint32_t LAG_MAX_BLOCKS = 4096u; // memory bound: cap the grid and stride over the rest (as beam_hardening.hip)
    constexpr uint32_t LAG_BATCH = 4u;         // frames whose loads are in flight while the batch before them is computed

    struct lag_setting // the coefficients as a kernel argument
    {
        uint32_t steady;
        float inv_b;
        float g[PARIS_HIP_LAG_TERMS_MAX], c[PARIS_HIP_LAG_TERMS_MAX], w[PARIS_HIP_LAG_TERMS_MAX];
    };

    // one pixel of one frame: i the stored count, d its dark, s the pixel's state; returns what is stored
    template <uint32_t TERMS>
    __device__ __forceinline__ float lag_step(float i, float d, float (&s)[TERMS], const lag_setting& k, bool first)
    {
        const float y = i - d;
        const bool finite = __builtin_fabsf(y) < __builtin_inff();
        if(first)
        {
#pragma unroll
            for(uint32_t n = 0; n < TERMS; ++n)
                s[n] = finite && k.steady != 0u ? k.w[n] * y : 0.f;
        }
        float x = 0.f, out = i; // a pixel that is not finite keeps its bits, and its state advances with x = 0
        if(finite)
        {
            float acc = y * k.inv_b;
#pragma unroll
            for(uint32_t n = 0; n < TERMS; ++n)
                acc = __builtin_fmaf(-k.c[n], s[n], acc);
            x = acc;
            out = x + d;
        }
#pragma unroll
        for(uint32_t n = 0; n < TERMS; ++n)
            s[n] = __builtin_fmaf(k.g[n], s[n], x);
        return out;
    }

    template <bool VEC>
    struct lag_pixels // what a lane holds of one frame
    {
        float v[VEC ? 4 : 1];
    };

    template <bool VEC>
    __device__ __forceinline__ lag_pixels<VEC> lag_load(const float* q)
    {
        lag_pixels<VEC> r;
        if constexpr(VEC)
        {
            const float4 t = *reinterpret_cast<const float4*>(q);
            r.v[0] = t.x, r.v[1] = t.y, r.v[2] = t.z, r.v[3] = t.w;
        }
        else
            r.v[0] = *q;
        return r;
    }

    template <bool VEC>
    __device__ __forceinline__ void lag_store(float* q, const lag_pixels<VEC>& r)
    {
        if constexpr(VEC)
            *reinterpret_cast<float4*>(q) = make_float4(r.v[0], r.v[1], r.v[2], r.v[3]);
        else
            *q = r.v[0];
    }

    // p: row 0 of the call's first frame. The band's pixels are dealt to the lanes as one list, row after row, `groups_x` lanes per
    // row. dark: the ctx's dark frame (rows dim_x floats apart, absolute rows) or nullptr. state: TERMS planes of `plane` floats, the
    // band's rows dense. first: the call's frame 0 is the sequence's frame 0 -- the state is made, not loaded.
    template <uint32_t TERMS, bool VEC>
    __global__ void __launch_bounds__(LAG_THREADS)
        lag_kernel(char* __restrict__ p, size_t frame_stride, uint32_t n_frames, size_t pitch_f, uint32_t dim_x, uint32_t row_first,
                   uint32_t groups_x, uint64_t lanes, const float* __restrict__ dark, float* __restrict__ state, uint64_t plane, int first,
                   lag_setting k)
    {
        constexpr uint32_t PER_LANE = VEC ? 4u : 1u;
        for(uint64_t i = static_cast<uint64_t>(blockIdx.x) * LAG_THREADS + threadIdx.x; i < lanes; i += static_cast<uint64_t>(gridDim.x) * LAG_THREADS)
        {
            const uint32_t band_row = static_cast<uint32_t>(i / groups_x);
            const uint32_t col = static_cast<uint32_t>(i % groups_x) * PER_LANE;
            const uint32_t row = row_first + band_row;
            char* px = p + (static_cast<size_t>(row) * pitch_f + col) * sizeof(float); // the lane's pixel(s) in frame 0
            float* st = state + static_cast<uint64_t>(band_row) * dim_x + col;
            lag_pixels<VEC> d;
#pragma unroll
            for(uint32_t e = 0; e < PER_LANE; ++e)
                d.v[e] = 0.f;
            if(dark != nullptr)
                d = lag_load<VEC>(dark + static_cast<size_t>(row) * dim_x + col);
            float s[PER_LANE][TERMS];
#pragma unroll
            for(uint32_t n = 0; n < TERMS; ++n)
            {
                lag_pixels<VEC> t;
#pragma unroll
                for(uint32_t e = 0; e < PER_LANE; ++e)
                    t.v[e] = 0.f;
                if(!first)
                    t = lag_load<VEC>(st + n * plane);
#pragma unroll
                for(uint32_t e = 0; e < PER_LANE; ++e)
                    s[e][n] = t.v[e];
            }
            lag_pixels<VEC> cur[LAG_BATCH] = {}, nxt[LAG_BATCH] = {};
#pragma unroll
            for(uint32_t b = 0; b < LAG_BATCH; ++b)
                if(b < n_frames)
                    cur[b] = lag_load<VEC>(reinterpret_cast<const float*>(px + b * frame_stride));
            for(uint32_t f0 = 0; f0 < n_frames; f0 += LAG_BATCH)
            {
#pragma unroll
                for(uint32_t b = 0; b < LAG_BATCH; ++b) // the next batch's loads: nothing below feeds them
                    if(f0 + LAG_BATCH + b < n_frames)
                        nxt[b] = lag_load<VEC>(reinterpret_cast<const float*>(px + static_cast<size_t>(f0 + LAG_BATCH + b) * frame_stride));
#pragma unroll
                for(uint32_t b = 0; b < LAG_BATCH; ++b) // this batch, in time order
                {
                    if(f0 + b >= n_frames)
                        break;
                    lag_pixels<VEC> out;
#pragma unroll
                    for(uint32_t e = 0; e < PER_LANE; ++e)
                        out.v[e] = lag_step<TERMS>(cur[b].v[e], d.v[e], s[e], k, first != 0 && f0 + b == 0u);
                    lag_store<VEC>(reinterpret_cast<float*>(px + static_cast<size_t>(f0 + b) * frame_stride), out);
                }
#pragma unroll
                for(uint32_t b = 0; b < LAG_BATCH; ++b)
                    cur[b] = nxt[b];
            }
#pragma unroll
            for(uint32_t n = 0; n < TERMS; ++n)
            {
                lag_pixels<VEC> t;
#pragma unroll
                for(uint32_t e = 0; e < PER_LANE; ++e)
                    t.v[e] = s[e][n];
                lag_store<VEC>(st + n * plane, t);
            }
        }
    }

    bool lag_vector_rows(const paris_hip_frame_band& b) // (the test of paris_hip_flat_field_rows)
    {
        return b.dim_x % 4u == 0 && b.pitch % 16u == 0 && reinterpret_cast<uintptr_t>(b.d_p) % 16u == 0
               && (b.n_frames == 1u || b.frame_stride % 16u == 0);
    }

    template <uint32_t TERMS>
    void lag_launch_terms(paris_hip_ctx* ctx, const paris_hip_frame_band& b, bool vec, uint32_t blocks, uint32_t groups_x, uint64_t lanes,
                          const float* dark, const lag_setting& k)
    {
        const paris_hip_ctx::lag_t::sequence_t& q = ctx->lag.seq;
        const uint64_t plane = static_cast<uint64_t>(q.row_count) * q.dim_x;
        const auto kernel = vec ? &lag_kernel<TERMS, true> : &lag_kernel<TERMS, false>;
        hipLaunchKernelGGL(kernel, dim3(blocks), dim3(LAG_THREADS), 0, ctx->stream, b.frame(0), b.frame_stride, b.n_frames, b.pitch / sizeof(float),
                           b.dim_x, b.row_first, groups_x, lanes, dark, q.mem.as<float>(), plane, q.frames == 0u ? 1 : 0, k);
    }

    void lag_launch(paris_hip_ctx* ctx, const paris_hip_frame_band& b)
    {
        const paris_hip_ctx::lag_t& l = ctx->lag;
        lag_setting k{};
        k.steady = l.model.start == PARIS_HIP_LAG_START_STEADY ? 1u : 0u;
        k.inv_b = l.inv_b;
        for(uint32_t n = 0; n < PARIS_HIP_LAG_TERMS_MAX; ++n)
            k.g[n] = l.g[n], k.c[n] = l.c[n], k.w[n] = l.w[n];
        const bool vec = lag_vector_rows(b);
        const uint32_t groups_x = vec ? b.dim_x / 4u : b.dim_x;
        const uint64_t lanes = static_cast<uint64_t>(groups_x) * b.row_count;
        const uint32_t blocks = static_cast<uint32_t>(std::min<uint64_t>(LAG_MAX_BLOCKS, (lanes + LAG_THREADS - 1u) / LAG_THREADS));
        const float* dark = ctx->flat_field.mem.as<float>(); // (nullptr without a flat-field setting: d = 0)
        switch(l.model.terms)
        {
        case 1u: lag_launch_terms<1u>(ctx, b, vec, blocks, groups_x, lanes, dark, k); break;
        case 2u: lag_launch_terms<2u>(ctx, b, vec, blocks, groups_x, lanes, dark, k); break;
        case 3u: lag_launch_terms<3u>(ctx, b, vec, blocks, groups_x, lanes, dark, k); break;
        default: lag_launch_terms<4u>(ctx, b, vec, blocks, groups_x, lanes, dark, k); break;
        }
    }
}

extern "C" int paris_hip_set_lag_correction(paris_hip_ctx* ctx, const paris_hip_lag_model* model)
{
    if(ctx == nullptr)
        return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    paris_hip_ctx::lag_t fresh{};
    if(int rc = paris_hip_lag_coefficients(model, fresh.g, fresh.c, fresh.w, &fresh.inv_b, nullptr)) // (runs the check)
        return rc;
    if(int rc = paris_hip_flush_deferred(ctx))
        return rc;
    if(int rc = paris_hip_bind(ctx))
        return rc;
    paris_hip_release(ctx, ctx->lag.seq); // a replaced setting closes the sequence
    fresh.set = true;
    fresh.model = *model;
    ctx->lag = fresh;
    return PARIS_HIP_SUCCESS;
}

extern "C" int paris_hip_clear_lag_correction(paris_hip_ctx* ctx)
{
    if(ctx == nullptr)
        return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    if(int rc = paris_hip_flush_deferred(ctx))
        return rc;
    if(int rc = paris_hip_bind(ctx))
        return rc;
    paris_hip_release(ctx, ctx->lag.seq);
    ctx->lag = paris_hip_ctx::lag_t{};
    return PARIS_HIP_SUCCESS;
}

extern "C" int paris_hip_lag_begin(paris_hip_ctx* ctx, uint32_t dim_x, uint32_t dim_y, uint32_t row_first, uint32_t row_count)
{
    if(int rc = paris_hip_bind(ctx))
        return rc;
    paris_hip_ctx::lag_t& l = ctx->lag;
    const paris_hip_ctx::flat_field_t& ff = ctx->flat_field;
    if(!l.set || l.seq.mem.d != nullptr || dim_x == 0u || row_count == 0u || row_first > dim_y || row_count > dim_y - row_first
       || (ff.mem.d != nullptr && (ff.dim_x != dim_x || ff.dim_y != dim_y)))
        return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    const size_t bytes = static_cast<size_t>(l.model.terms) * row_count * dim_x * sizeof(float);
    float* d = nullptr;
    if(int rc = paris_hip_device_malloc(ctx, reinterpret_cast<void**>(&d), bytes))
        return rc;
    // zeroed on the compute stream, ahead of the kernels that will read and write it there
    const hipError_t err = hipMemsetAsync(d, 0, bytes, ctx->stream);
    if(err != hipSuccess)
    {
        (void)hipStreamSynchronize(ctx->stream);
        (void)hipFree(d);
        return static_cast<int>(err);
    }
    l.seq.mem = paris_hip_device_buffer{d, bytes};
    l.seq.dim_x = dim_x;
    l.seq.dim_y = dim_y;
    l.seq.row_first = row_first;
    l.seq.row_count = row_count;
    l.seq.frames = 0;
    return paris_hip_finish(ctx);
}

extern "C" int paris_hip_lag_end(paris_hip_ctx* ctx)
{
    if(int rc = paris_hip_bind(ctx))
        return rc;
    paris_hip_release(ctx, ctx->lag.seq);
    return PARIS_HIP_SUCCESS;
}

extern "C" int paris_hip_lag_correct_rows(paris_hip_ctx* ctx, float* d_p, size_t pitch, size_t frame_stride, uint32_t n_frames, uint32_t dim_x,
                                          uint32_t dim_y, uint32_t row_first, uint32_t row_count)
{
    const paris_hip_frame_band band{d_p, pitch, frame_stride, n_frames, dim_x, dim_y, row_first, row_count};
    const auto refuse = [&]() -> int {
        const paris_hip_ctx::lag_t::sequence_t& q = ctx->lag.seq;
        const paris_hip_ctx::flat_field_t& ff = ctx->flat_field;
        const bool same = ctx->lag.set && q.mem.d != nullptr && dim_x == q.dim_x && dim_y == q.dim_y && row_first == q.row_first && row_count == q.row_count;
        return !same || (ff.mem.d != nullptr && (ff.dim_x != dim_x || ff.dim_y != dim_y)) ? PARIS_HIP_ERROR_INVALID_ARGUMENT : PARIS_HIP_SUCCESS;
    };
    return paris_hip_frame_pass(ctx, band, refuse, [&] {
        lag_launch(ctx, band);
        ctx->lag.seq.frames += n_frames;
    });
}

extern "C" int paris_hip_lag_frames(paris_hip_ctx* ctx, uint64_t* frames)
{
    if(ctx == nullptr || frames == nullptr)
        return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    *frames = ctx->lag.seq.mem.d != nullptr ? ctx->lag.seq.frames : 0u;
    return PARIS_HIP_SUCCESS;
}

void paris_hip_warm_lag()
{
    hipFuncAttributes a{};
    (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&lag_kernel<4u, true>));
    (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&lag_kernel<4u, false>));
}
