// Beam-hardening correction for gfx950 (the statement is in include/paris_hip.h).
//
//   bh_apply_kernel<VEC>   the polynomial of the line integral, in place on the band's rows; the setting is a kernel argument, so a
//                          replaced setting needs no care and nothing lives on the device. A stream: 4 bytes read and written per
//                          pixel, dealt to the lanes as air_subtract_kernel deals them.
//   bh_classify_kernel     one 256-lane workgroup per tile of 32 x 16 x 8 voxels: the classes of the tile and of its halo of `margin`
//                          voxels as bytes in LDS (bit 0: air, bit 1: object, 0: none or outside the slab), then the erosion as
//                          three passes of ANDs, along x, y and z -- a box is a product, so the passes separate. 15360 + 12288 bytes
//                          of LDS: five workgroups per CU.
//   bh_gram_kernel<N>      PARIS_HIP_BH_PARTIALS lanes, lane l owns partial sum l and walks voxels l, l + L, ... ascending; the
//                          loads of a batch are issued together, the additions follow in order (as air_value_kernel).
//   bh_gram_fold_kernel    one workgroup per term: lane j adds acc_{j + 256 m}, m ascending, lane 0 adds the 256 B_j, j ascending.
// Every sum has one owner and a fixed order: no floating-point atomics, and the bits are the statement's whatever the grid.
#include <algorithm>
#include <cmath>

#include "frame_pass.h"

namespace
{
    constexpr uint32_t BH_THREADS = 256u;
    constexpr uint32_t BH_MAX_BLOCKS = 4096u; // memory bound: cap the grid and stride over the rest (as ring.hip)
    constexpr uint32_t BH_TX = 32u, BH_TY = 16u, BH_TZ = 8u, BH_M = PARIS_HIP_BH_MARGIN_MAX;
    constexpr uint32_t BH_A_BYTES = (BH_TX + 2u * BH_M) * (BH_TY + 2u * BH_M) * (BH_TZ + 2u * BH_M); // classes with their halo
    constexpr uint32_t BH_B_BYTES = BH_TX * (BH_TY + 2u * BH_M) * (BH_TZ + 2u * BH_M);                // after the pass along x
    static_assert(BH_TX * BH_TY * (BH_TZ + 2u * BH_M) <= BH_A_BYTES, "the pass along y writes into the first array");
    constexpr uint32_t BH_GRAM_BATCH = 4u;
    constexpr uint32_t BH_FOLD = 256u;
    static_assert(PARIS_HIP_BH_PARTIALS % BH_FOLD == 0u && PARIS_HIP_BH_PARTIALS % BH_THREADS == 0u, "whole workgroups, whole folds");

    struct bh_setting // the rule as a kernel argument
    {
        uint32_t degree;
        float c[PARIS_HIP_BH_DEGREE_MAX];
    };

    __device__ __forceinline__ float bh_apply(float p, const bh_setting& s)
    {
        if(p < 0.f) // noise in air: the linear term only
            return s.c[0] * p;
        float acc = s.c[s.degree - 1u];
        for(uint32_t k = s.degree - 1u; k >= 1u; --k)
            acc = __builtin_fmaf(acc, p, s.c[k - 1u]);
        return acc * p; // (one multiplication: contraction is off in this library)
    }

    // The band's pixels are dealt to the lanes of grid x as one list, row after row, `groups_x` lanes per row; frames on grid y, strided.
    template <bool VEC>
    __global__ void __launch_bounds__(BH_THREADS)
        bh_apply_kernel(char* __restrict__ p, size_t frame_stride, uint32_t n_frames, size_t pitch_f, uint32_t row_first, uint32_t groups_x,
                        uint64_t lanes, bh_setting s)
    {
        constexpr uint32_t PER_LANE = VEC ? 4u : 1u;
        for(uint32_t f = blockIdx.y; f < n_frames; f += gridDim.y)
        {
            char* frame = p + static_cast<size_t>(f) * frame_stride;
            for(uint64_t i = static_cast<uint64_t>(blockIdx.x) * BH_THREADS + threadIdx.x; i < lanes; i += static_cast<uint64_t>(gridDim.x) * BH_THREADS)
            {
                const uint32_t row = row_first + static_cast<uint32_t>(i / groups_x);
                const uint32_t col = static_cast<uint32_t>(i % groups_x) * PER_LANE;
                float* q = reinterpret_cast<float*>(frame) + static_cast<size_t>(row) * pitch_f + col;
                if constexpr(VEC)
                {
                    const float4 v = *reinterpret_cast<const float4*>(q);
                    *reinterpret_cast<float4*>(q) = make_float4(bh_apply(v.x, s), bh_apply(v.y, s), bh_apply(v.z, s), bh_apply(v.w, s));
                }
                else
                    *q = bh_apply(*q, s);
            }
        }
    }

    bool bh_vector_rows(const paris_hip_frame_band& b)
    {
        return b.dim_x % 4u == 0 && b.pitch % 16u == 0 && reinterpret_cast<uintptr_t>(b.d_p) % 16u == 0
               && (b.n_frames == 1u || b.frame_stride % 16u == 0);
    }

    void bh_launch_apply(paris_hip_ctx* ctx, const paris_hip_frame_band& b, const paris_hip_beam_hardening& rule)
    {
        bh_setting s{};
        s.degree = rule.degree;
        for(uint32_t k = 0; k < PARIS_HIP_BH_DEGREE_MAX; ++k)
            s.c[k] = k < rule.degree ? rule.c[k] : 0.f;
        const bool vec = bh_vector_rows(b);
        const uint32_t groups_x = vec ? b.dim_x / 4u : b.dim_x;
        const uint64_t lanes = static_cast<uint64_t>(groups_x) * b.row_count;
        const uint32_t blocks = static_cast<uint32_t>(std::min<uint64_t>(BH_MAX_BLOCKS, (lanes + BH_THREADS - 1u) / BH_THREADS));
        const auto kernel = vec ? &bh_apply_kernel<true> : &bh_apply_kernel<false>;
        hipLaunchKernelGGL(kernel, dim3(blocks, std::min(b.n_frames, 65535u)), dim3(BH_THREADS), 0, ctx->stream, b.frame(0), b.frame_stride, b.n_frames,
                           b.pitch / sizeof(float), b.row_first, groups_x, lanes, s);
    }

    // v: the slab; labels: one byte per voxel. Grid: the tiles along x, y and z.
    __global__ void __launch_bounds__(BH_THREADS)
        bh_classify_kernel(const float* __restrict__ v, uint32_t dim_x, uint32_t dim_y, uint32_t dim_z, float thr, uint32_t margin,
                           long long fov_r2, uint8_t* __restrict__ labels)
    {
        __shared__ uint8_t lds_a[BH_A_BYTES];
        __shared__ uint8_t lds_b[BH_B_BYTES];
        const uint32_t hx = BH_TX + 2u * margin, hy = BH_TY + 2u * margin, hz = BH_TZ + 2u * margin;
        const long long x0 = static_cast<long long>(blockIdx.x) * BH_TX - margin, y0 = static_cast<long long>(blockIdx.y) * BH_TY - margin,
                        z0 = static_cast<long long>(blockIdx.z) * BH_TZ - margin;
        // the classes of the tile and its halo: a[(z * hy + y) * hx + x]
        for(uint32_t i = threadIdx.x; i < hx * hy * hz; i += BH_THREADS)
        {
            const uint32_t lx = i % hx, ly = (i / hx) % hy, lz = i / (hx * hy);
            const long long x = x0 + lx, y = y0 + ly, z = z0 + lz;
            uint8_t cls = 0u;
            if(x >= 0 && x < dim_x && y >= 0 && y < dim_y && z >= 0 && z < dim_z)
            {
                const float val = v[(static_cast<uint64_t>(z) * dim_y + static_cast<uint64_t>(y)) * dim_x + static_cast<uint64_t>(x)];
                if(__builtin_fabsf(val) < __builtin_inff()) // finite
                    cls = val > thr ? 2u : 1u;
            }
            lds_a[i] = cls;
        }
        __syncthreads();
        const uint32_t span = 2u * margin + 1u;
        // along x: b[(z * hy + y) * TX + x], x over the tile, y and z still with their halo
        for(uint32_t i = threadIdx.x; i < BH_TX * hy * hz; i += BH_THREADS)
        {
            const uint32_t lx = i % BH_TX, row = i / BH_TX;
            uint8_t r = 3u;
            for(uint32_t d = 0; d < span; ++d)
                r &= lds_a[row * hx + lx + d];
            lds_b[i] = r;
        }
        __syncthreads();
        // along y: a[(z * TY + y) * TX + x], z still with its halo
        for(uint32_t i = threadIdx.x; i < BH_TX * BH_TY * hz; i += BH_THREADS)
        {
            const uint32_t lx = i % BH_TX, ly = (i / BH_TX) % BH_TY, lz = i / (BH_TX * BH_TY);
            uint8_t r = 3u;
            for(uint32_t d = 0; d < span; ++d)
                r &= lds_b[(lz * hy + ly + d) * BH_TX + lx];
            lds_a[i] = r;
        }
        __syncthreads();
        // along z, the field of view, the store
        for(uint32_t i = threadIdx.x; i < BH_TX * BH_TY * BH_TZ; i += BH_THREADS)
        {
            const uint32_t lx = i % BH_TX, ly = (i / BH_TX) % BH_TY, lz = i / (BH_TX * BH_TY);
            const uint64_t x = static_cast<uint64_t>(blockIdx.x) * BH_TX + lx, y = static_cast<uint64_t>(blockIdx.y) * BH_TY + ly,
                           z = static_cast<uint64_t>(blockIdx.z) * BH_TZ + lz;
            if(x >= dim_x || y >= dim_y || z >= dim_z)
                continue;
            uint8_t r = 3u;
            for(uint32_t d = 0; d < span; ++d)
                r &= lds_a[((lz + d) * BH_TY + ly) * BH_TX + lx];
            const long long fx = 2ll * static_cast<long long>(x) - dim_x + 1ll, fy = 2ll * static_cast<long long>(y) - dim_y + 1ll;
            if(fx * fx + fy * fy > fov_r2)
                r = 0u;
            labels[(z * dim_y + y) * dim_x + x] = r; // 0, 1 (air) or 2 (object): a voxel has one class, so both bits never survive
        }
    }

    // acc: terms x L doubles, acc[t * L + l]; cnt: n_object, n_air, n_ignored, n_not_finite
    template <uint32_t N>
    __global__ void __launch_bounds__(BH_THREADS)
        bh_gram_kernel(const float* __restrict__ f0, const float* __restrict__ f1, const float* __restrict__ f2, const float* __restrict__ f3,
                       const uint8_t* __restrict__ labels, uint64_t n, double* __restrict__ acc, unsigned long long* __restrict__ cnt)
    {
        constexpr uint32_t D = N + 1u, TERMS = D * (D + 1u) / 2u;
        constexpr uint64_t L = PARIS_HIP_BH_PARTIALS;
        const float* const f[4] = {f0, f1, f2, f3};
        const uint64_t l = static_cast<uint64_t>(blockIdx.x) * BH_THREADS + threadIdx.x;
        double sum[TERMS];
#pragma unroll
        for(uint32_t t = 0; t < TERMS; ++t)
            sum[t] = 0.0;
        uint32_t n_object = 0, n_air = 0, n_ignored = 0, n_not_finite = 0; // (a lane sees n / L voxels: far below 2^32)
        for(uint64_t i = l; i < n; i += L * BH_GRAM_BATCH)
        {
            uint8_t label[BH_GRAM_BATCH];
            float val[BH_GRAM_BATCH][N];
#pragma unroll
            for(uint32_t k = 0; k < BH_GRAM_BATCH; ++k) // the loads of a batch, independent of each other
            {
                const uint64_t ik = i + k * L;
                const bool live = ik < n;
                label[k] = live ? labels[ik] : 0u; // (beyond the slab: neither counted nor summed)
#pragma unroll
                for(uint32_t a = 0; a < N; ++a)
                    val[k][a] = live ? f[a][ik] : 0.f;
            }
#pragma unroll
            for(uint32_t k = 0; k < BH_GRAM_BATCH; ++k) // the additions, in ascending i
            {
                if(i + k * L >= n)
                    continue;
                if(label[k] != 1u && label[k] != 2u)
                {
                    ++n_ignored;
                    continue;
                }
                bool finite = true;
                double g[D];
#pragma unroll
                for(uint32_t a = 0; a < N; ++a)
                {
                    finite = finite && __builtin_fabsf(val[k][a]) < __builtin_inff();
                    g[a] = static_cast<double>(val[k][a]);
                }
                if(!finite)
                {
                    ++n_not_finite;
                    continue;
                }
                g[N] = label[k] == 2u ? 1.0 : 0.0;
                n_object += label[k] == 2u ? 1u : 0u;
                n_air += label[k] == 2u ? 0u : 1u;
                uint32_t t = 0;
#pragma unroll
                for(uint32_t a = 0; a < D; ++a)
#pragma unroll
                    for(uint32_t b = a; b < D; ++b, ++t)
                        sum[t] += g[a] * g[b]; // (the product of two floats is exact in double; no contraction in this library)
            }
        }
#pragma unroll
        for(uint32_t t = 0; t < TERMS; ++t)
            acc[static_cast<uint64_t>(t) * L + l] = sum[t];
#pragma unroll
        for(int off = 32; off != 0; off >>= 1)
        {
            n_object += __shfl_xor(n_object, off);
            n_air += __shfl_xor(n_air, off);
            n_ignored += __shfl_xor(n_ignored, off);
            n_not_finite += __shfl_xor(n_not_finite, off);
        }
        if((threadIdx.x & 63u) == 0u)
        {
            atomicAdd(&cnt[0], static_cast<unsigned long long>(n_object));
            atomicAdd(&cnt[1], static_cast<unsigned long long>(n_air));
            atomicAdd(&cnt[2], static_cast<unsigned long long>(n_ignored));
            atomicAdd(&cnt[3], static_cast<unsigned long long>(n_not_finite));
        }
    }

    __global__ void __launch_bounds__(BH_FOLD) bh_gram_fold_kernel(const double* __restrict__ acc, double* __restrict__ gram)
    {
        __shared__ double part[BH_FOLD];
        constexpr uint64_t L = PARIS_HIP_BH_PARTIALS;
        const double* a = acc + static_cast<uint64_t>(blockIdx.x) * L;
        const uint32_t j = threadIdx.x;
        double b = a[j];
        for(uint32_t m = 1; m < L / BH_FOLD; ++m) // ascending m, one double addition each
            b = b + a[j + BH_FOLD * m];
        part[j] = b;
        __syncthreads();
        if(j != 0u)
            return;
        double total = part[0];
        for(uint32_t k = 1; k < BH_FOLD; ++k) // ascending j
            total = total + part[k];
        gram[blockIdx.x] = total;
    }
}

extern "C" int paris_hip_set_beam_hardening(paris_hip_ctx* ctx, const paris_hip_beam_hardening* bh, uint32_t dim_x, uint32_t dim_y)
{
    if(int rc = paris_hip_bind(ctx))
        return rc;
    if(int rc = paris_hip_beam_hardening_check(bh))
        return rc;
    if(dim_x == 0u || dim_y == 0u)
        return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    paris_hip_ctx::beam_hardening_t& s = ctx->beam_hardening;
    s.set = true;
    s.rule = *bh;
    s.dim_x = dim_x;
    s.dim_y = dim_y;
    return PARIS_HIP_SUCCESS;
}

extern "C" int paris_hip_clear_beam_hardening(paris_hip_ctx* ctx)
{
    if(int rc = paris_hip_bind(ctx))
        return rc;
    ctx->beam_hardening = paris_hip_ctx::beam_hardening_t{};
    return PARIS_HIP_SUCCESS;
}

extern "C" int paris_hip_beam_hardening_rows(paris_hip_ctx* ctx, float* d_p, size_t pitch, size_t frame_stride, uint32_t n_frames, uint32_t dim_x,
                                             uint32_t dim_y, uint32_t row_first, uint32_t row_count)
{
    const paris_hip_frame_band band{d_p, pitch, frame_stride, n_frames, dim_x, dim_y, row_first, row_count};
    const auto refuse = [&]() -> int {
        const paris_hip_ctx::beam_hardening_t& s = ctx->beam_hardening;
        return !s.set || dim_x != s.dim_x || dim_y != s.dim_y ? PARIS_HIP_ERROR_INVALID_ARGUMENT : PARIS_HIP_SUCCESS;
    };
    return paris_hip_frame_pass(ctx, band, refuse, [&] { bh_launch_apply(ctx, band, ctx->beam_hardening.rule); });
}

extern "C" int paris_hip_beam_hardening_rows_with(paris_hip_ctx* ctx, const paris_hip_beam_hardening* bh, float* d_p, size_t pitch,
                                                  size_t frame_stride, uint32_t n_frames, uint32_t dim_x, uint32_t dim_y, uint32_t row_first,
                                                  uint32_t row_count)
{
    const paris_hip_frame_band band{d_p, pitch, frame_stride, n_frames, dim_x, dim_y, row_first, row_count};
    return paris_hip_frame_pass(ctx, band, [&] { return paris_hip_beam_hardening_check(bh); }, [&] { bh_launch_apply(ctx, band, *bh); });
}

extern "C" int paris_hip_bh_classify(paris_hip_ctx* ctx, const float* d_v, uint32_t dim_x, uint32_t dim_y, uint32_t dim_z, float thr,
                                     uint32_t margin, uint8_t* d_labels)
{
    if(int rc = paris_hip_flush_deferred(ctx))
        return rc;
    if(int rc = paris_hip_bind(ctx))
        return rc;
    if(d_v == nullptr || d_labels == nullptr || dim_x == 0u || dim_y == 0u || dim_z == 0u || !std::isfinite(thr) || margin > PARIS_HIP_BH_MARGIN_MAX
       || reinterpret_cast<uintptr_t>(d_v) % sizeof(float) != 0u)
        return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    const uint32_t gx = (dim_x + BH_TX - 1u) / BH_TX, gy = (dim_y + BH_TY - 1u) / BH_TY, gz = (dim_z + BH_TZ - 1u) / BH_TZ;
    if(gy > 65535u || gz > 65535u)
        return PARIS_HIP_ERROR_UNSUPPORTED;
    const uint64_t n = static_cast<uint64_t>(dim_x) * dim_y * dim_z;
    const uintptr_t v0 = reinterpret_cast<uintptr_t>(d_v), q0 = reinterpret_cast<uintptr_t>(d_labels);
    if(v0 < q0 + n && q0 < v0 + n * sizeof(float))
        return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    if(int rc = paris_hip_volume_mark_dirty(ctx, d_labels, n)) // a volume the labels overlap holds arbitrary bits from here on
        return rc;
    const long long r = static_cast<long long>(std::min(dim_x, dim_y)) - 2ll;
    hipLaunchKernelGGL(bh_classify_kernel, dim3(gx, gy, gz), dim3(BH_THREADS), 0, ctx->stream, d_v, dim_x, dim_y, dim_z, thr, margin, r * r, d_labels);
    PARIS_HIP_TRY(hipGetLastError());
    return paris_hip_finish(ctx);
}

extern "C" int paris_hip_bh_gram(paris_hip_ctx* ctx, const float* const* d_f, uint32_t degree, const uint8_t* d_labels, uint64_t n_voxels,
                                 double* gram, paris_hip_bh_counts* counts)
{
    if(int rc = paris_hip_flush_deferred(ctx))
        return rc;
    if(int rc = paris_hip_bind(ctx))
        return rc;
    if(d_f == nullptr || gram == nullptr || counts == nullptr || degree < 1u || degree > PARIS_HIP_BH_DEGREE_MAX
       || (n_voxels != 0u && d_labels == nullptr))
        return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    const float* f[PARIS_HIP_BH_DEGREE_MAX] = {nullptr, nullptr, nullptr, nullptr};
    for(uint32_t k = 0; k < degree; ++k)
    {
        f[k] = d_f[k];
        if(n_voxels != 0u && (f[k] == nullptr || reinterpret_cast<uintptr_t>(f[k]) % sizeof(float) != 0u))
            return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    }
    const uint32_t terms = (degree + 1u) * (degree + 2u) / 2u;
    *counts = paris_hip_bh_counts{};
    for(uint32_t t = 0; t < terms; ++t)
        gram[t] = 0.0;
    if(n_voxels == 0u)
        return PARIS_HIP_SUCCESS;
    // the call's own memory: the partial sums, then the folded terms, then the four counters
    constexpr uint64_t L = PARIS_HIP_BH_PARTIALS;
    const size_t acc_bytes = static_cast<size_t>(terms) * L * sizeof(double), gram_bytes = terms * sizeof(double);
    char* d = nullptr;
    if(int rc = paris_hip_device_malloc(ctx, reinterpret_cast<void**>(&d), acc_bytes + gram_bytes + 4u * sizeof(unsigned long long)))
        return rc;
    double* d_acc = reinterpret_cast<double*>(d);
    double* d_gram = reinterpret_cast<double*>(d + acc_bytes);
    unsigned long long* d_cnt = reinterpret_cast<unsigned long long*>(d + acc_bytes + gram_bytes);
    unsigned long long cnt[4] = {0ull, 0ull, 0ull, 0ull};
    const auto run = [&]() -> int {
        PARIS_HIP_TRY(hipMemsetAsync(d_cnt, 0, sizeof(cnt), ctx->stream));
        const auto kernel = degree == 1u ? &bh_gram_kernel<1u> : degree == 2u ? &bh_gram_kernel<2u> : degree == 3u ? &bh_gram_kernel<3u> : &bh_gram_kernel<4u>;
        hipLaunchKernelGGL(kernel, dim3(static_cast<uint32_t>(L / BH_THREADS)), dim3(BH_THREADS), 0, ctx->stream, f[0], f[1], f[2], f[3], d_labels,
                           n_voxels, d_acc, d_cnt);
        PARIS_HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(bh_gram_fold_kernel, dim3(terms), dim3(BH_FOLD), 0, ctx->stream, d_acc, d_gram);
        PARIS_HIP_TRY(hipGetLastError());
        PARIS_HIP_TRY(hipMemcpyAsync(gram, d_gram, gram_bytes, hipMemcpyDeviceToHost, ctx->stream));
        PARIS_HIP_TRY(hipMemcpyAsync(cnt, d_cnt, sizeof(cnt), hipMemcpyDeviceToHost, ctx->stream));
        PARIS_HIP_TRY(hipStreamSynchronize(ctx->stream));
        return PARIS_HIP_SUCCESS;
    };
    const int rc = run();
    if(rc != PARIS_HIP_SUCCESS)
        (void)hipStreamSynchronize(ctx->stream); // nothing queued may still use the memory when it goes
    (void)hipFree(d);
    if(rc != PARIS_HIP_SUCCESS)
        return rc;
    counts->n_object = cnt[0];
    counts->n_air = cnt[1];
    counts->n_ignored = cnt[2];
    counts->n_not_finite = cnt[3];
    return PARIS_HIP_SUCCESS;
}

void paris_hip_warm_beam_hardening()
{
    hipFuncAttributes a{};
    (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&bh_apply_kernel<true>));
    (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&bh_apply_kernel<false>));
    (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&bh_classify_kernel));
    (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&bh_gram_kernel<2u>));
    (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&bh_gram_fold_kernel));
}
