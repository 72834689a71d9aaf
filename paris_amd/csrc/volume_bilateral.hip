// Volume denoising for gfx950: the edge-preserving 3-D bilateral filter (the statement is in
// include/paris_hip.h, the host rule in bilateral_rule.cpp -- this kernel gives its bits).
//
// Unlike the other volume passes this one is no stream: a voxel is a tap of (2R + 1)^3 outputs. volume_bilateral_kernel<R, TY>:
//   - a workgroup of 4 waves owns a tile of BL_TX x TY = 64 x 16 (R = 1, 2) or 64 x 8 (R = 3) outputs in x and y plus a halo of R, and
//     walks a chunk of z;
//   - the 2R + 1 source slices of the footprint are a ring in LDS: every step loads ONE slice (16-byte nontemporal loads for the 64
//     interior columns where base and dim_x allow, single voxels for the halo columns and otherwise), so a source voxel comes from
//     memory about once per tile; a row of the ring is BL_PW = 72 floats with the interior at column 4, 16-byte aligned for the
//     vector store, and a wave's 64 consecutive columns fall in 64 consecutive banks;
//   - what lies outside the source buffer is stored in the ring as NaN: the rule's own test `t < 1024` is false for NaN, so such a
//     tap drops out exactly as a skipped one does, and the inner loop has no bounds test;
//   - the range table (4 KiB) and the spatial table sit in LDS; the range gather is the one LDS read whose banks the data decide;
//   - a lane owns TY / 4 consecutive rows of one column: the outputs share the spatial weight of a tap and, from one dx to the same dx of
//     the next dy, the neighbour values, so the compiler keeps them in registers;
//   - every output has its own num and den and takes its taps in the rule's order dz, dy, dx: nothing is reassociated.
// Work items are (x tile, y tile, z chunk), walked by a capped grid with 64-bit indices.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "paris_hip_internal.h"

namespace
{
    typedef float f32x4 __attribute__((ext_vector_type(4)));

    // The tile height TY is a template parameter, decided per radius by A/B: 16 rows, 4 per lane, for R = 1 and
    // 2; 8 rows, 2 per lane, for R = 3, whose ring of 7 slices then leaves room for 4 workgroups a CU instead of 3. The experiments
    // build also holds the three arms that lost, picked by PARIS_BILATERAL_TILE_Y=8 or 16 in the environment.
    constexpr uint32_t BL_THREADS = 256u, BL_TX = 64u, BL_PW = 72u, BL_COL0 = 4u;
    constexpr uint32_t BL_TY_SHALLOW = 16u, BL_TY_DEEP = 8u; // for R <= 2 and for R = 3
    // LDS per workgroup: 15.2 KiB (R = 1), 28.1 KiB (R = 2), 27.6 KiB (R = 3) of ring and 4 KiB + (2R + 1)^3 floats of tables: 8, 4 and 4
    // workgroups fit a CU's 160 KiB. The grid is capped at 8 workgroups per CU; larger volumes loop.
    constexpr uint32_t BL_GRID_MAX = 2048u;
    constexpr uint32_t BL_Z_CHUNK_MAX = 64u, BL_Z_CHUNK_MIN = 8u;

    template <int R, uint32_t TY>
    struct bl_shape
    {
        static constexpr uint32_t SIDE = 2u * R + 1u, ROWS = TY + 2u * R, SLICE = ROWS * BL_PW, TAPS = SIDE * SIDE * SIDE;
        static constexpr uint32_t PER_LANE = TY / (BL_THREADS / 64u); // rows of one column a lane owns
    };

    // slice gz = gzr - R of the source (NaN where it lies outside the buffer) -> its slot of the ring
    template <int R, uint32_t TY>
    __device__ __forceinline__ void bl_load_slice(float* __restrict__ ring, const float* __restrict__ src, uint32_t dim_x, uint32_t dim_y,
                                                  uint32_t src_dim_z, uint64_t plane, uint64_t gzr, uint32_t x0, uint32_t y0, bool vec)
    {
        using S = bl_shape<R, TY>;
        float* __restrict__ sl = ring + static_cast<uint32_t>(gzr % S::SIDE) * S::SLICE;
        const bool z_in = gzr >= static_cast<uint64_t>(R) && gzr - R < src_dim_z;
        const float* __restrict__ sp = src + (z_in ? (gzr - R) * plane : 0u);
        const float nan = __builtin_nanf("");
        if(vec)
        {
            for(uint32_t i = threadIdx.x; i < S::ROWS * (BL_TX / 4u); i += BL_THREADS)
            {
                const uint32_t row = i / (BL_TX / 4u), g = i % (BL_TX / 4u);
                const int64_t gy = static_cast<int64_t>(y0) + row - R;
                const uint64_t gx = static_cast<uint64_t>(x0) + 4u * g;
                f32x4 v = {nan, nan, nan, nan};
                if(z_in && gy >= 0 && gy < static_cast<int64_t>(dim_y) && gx < dim_x) // (dim_x is a multiple of 4 here: gx + 3 < dim_x)
                    v = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(sp + static_cast<uint64_t>(gy) * dim_x + gx));
                *reinterpret_cast<f32x4*>(sl + row * BL_PW + BL_COL0 + 4u * g) = v;
            }
            for(uint32_t i = threadIdx.x; i < S::ROWS * 2u * R; i += BL_THREADS)
            {
                const uint32_t row = i / (2u * R), h = i % (2u * R);
                const int32_t col = h < static_cast<uint32_t>(R) ? static_cast<int32_t>(h) - R : static_cast<int32_t>(BL_TX + h) - R;
                const int64_t gy = static_cast<int64_t>(y0) + row - R, gx = static_cast<int64_t>(x0) + col;
                float v = nan;
                if(z_in && gy >= 0 && gy < static_cast<int64_t>(dim_y) && gx >= 0 && gx < static_cast<int64_t>(dim_x))
                    v = __builtin_nontemporal_load(sp + static_cast<uint64_t>(gy) * dim_x + static_cast<uint64_t>(gx));
                sl[row * BL_PW + static_cast<uint32_t>(static_cast<int32_t>(BL_COL0) + col)] = v;
            }
        }
        else
        {
            constexpr uint32_t W = BL_TX + 2u * R;
            for(uint32_t i = threadIdx.x; i < S::ROWS * W; i += BL_THREADS)
            {
                const uint32_t row = i / W, c = i % W;
                const int64_t gy = static_cast<int64_t>(y0) + row - R, gx = static_cast<int64_t>(x0) + c - R;
                float v = nan;
                if(z_in && gy >= 0 && gy < static_cast<int64_t>(dim_y) && gx >= 0 && gx < static_cast<int64_t>(dim_x))
                    v = __builtin_nontemporal_load(sp + static_cast<uint64_t>(gy) * dim_x + static_cast<uint64_t>(gx));
                sl[row * BL_PW + BL_COL0 - R + c] = v;
            }
        }
    }

    // tables: the range table, then the spatial table. items = tiles_x * tiles_y * chunks of z_chunk slices.
    template <int R, uint32_t TY>
    __global__ void __launch_bounds__(BL_THREADS)
        volume_bilateral_kernel(const float* __restrict__ src, uint32_t dim_x, uint32_t dim_y, uint32_t src_dim_z, uint32_t z_first, uint32_t z_count,
                                uint32_t z_chunk, uint32_t tiles_x, uint32_t tiles_y, uint64_t items, const float* __restrict__ tables, float rscale,
                                int vec, float* __restrict__ dst)
    {
        using S = bl_shape<R, TY>;
        __shared__ __attribute__((aligned(16))) float ring[S::SIDE * S::SLICE];
        __shared__ float range[PARIS_HIP_BILATERAL_BINS];
        __shared__ float spatial[S::TAPS];
        for(uint32_t i = threadIdx.x; i < PARIS_HIP_BILATERAL_BINS; i += BL_THREADS)
            range[i] = tables[i];
        for(uint32_t i = threadIdx.x; i < S::TAPS; i += BL_THREADS)
            spatial[i] = tables[PARIS_HIP_BILATERAL_BINS + i];
        const uint64_t plane = static_cast<uint64_t>(dim_x) * dim_y;
        const uint32_t lx = threadIdx.x & 63u, row0 = (threadIdx.x >> 6) * S::PER_LANE;
        const uint64_t tiles = static_cast<uint64_t>(tiles_x) * tiles_y;
        const uint64_t z_end = static_cast<uint64_t>(z_first) + z_count;
        for(uint64_t item = blockIdx.x; item < items; item += gridDim.x)
        {
            const uint64_t chunk = item / tiles, tile = item % tiles;
            const uint32_t x0 = static_cast<uint32_t>(tile % tiles_x) * BL_TX, y0 = static_cast<uint32_t>(tile / tiles_x) * TY;
            const uint64_t z0 = z_first + chunk * z_chunk, z1 = z0 + z_chunk < z_end ? z0 + z_chunk : z_end;
            __syncthreads(); // the last item's taps have been read (and, the first time, the tables are written)
            // slice z sits at ring position (z + R) mod SIDE: the prologue brings z0 - R .. z0 + R - 1
            for(uint64_t gzr = z0; gzr < z0 + 2u * R; ++gzr)
                bl_load_slice<R, TY>(ring, src, dim_x, dim_y, src_dim_z, plane, gzr, x0, y0, vec != 0);
            const uint64_t gx = static_cast<uint64_t>(x0) + lx;
            for(uint64_t z = z0; z < z1; ++z)
            {
                bl_load_slice<R, TY>(ring, src, dim_x, dim_y, src_dim_z, plane, z + 2u * R, x0, y0, vec != 0);
                __syncthreads();
                const float* __restrict__ centre = ring + static_cast<uint32_t>((z + R) % S::SIDE) * S::SLICE + (row0 + R) * BL_PW + BL_COL0 + lx;
                float vc[S::PER_LANE], num[S::PER_LANE], den[S::PER_LANE];
#pragma unroll
                for(uint32_t k = 0; k < S::PER_LANE; ++k)
                {
                    vc[k] = centre[k * BL_PW];
                    num[k] = 0.f;
                    den[k] = 0.f;
                }
#pragma unroll 1
                for(uint32_t dz = 0; dz < S::SIDE; ++dz)
                {
                    const float* __restrict__ sl = ring + static_cast<uint32_t>((z + dz) % S::SIDE) * S::SLICE + row0 * BL_PW + (BL_COL0 - R) + lx;
                    const float* __restrict__ sp = spatial + dz * S::SIDE * S::SIDE;
#pragma unroll
                    for(uint32_t dy = 0; dy < S::SIDE; ++dy)
#pragma unroll
                        for(uint32_t dx = 0; dx < S::SIDE; ++dx)
                        {
                            const float s = sp[dy * S::SIDE + dx];
#pragma unroll
                            for(uint32_t k = 0; k < S::PER_LANE; ++k)
                            {
                                const float vn = sl[(k + dy) * BL_PW + dx];
                                const float d = __builtin_fabsf(vn - vc[k]);
                                const float t = d * rscale;
                                const bool in = t < static_cast<float>(PARIS_HIP_BILATERAL_BINS); // (false for NaN)
                                const float w = s * range[in ? static_cast<uint32_t>(t) : 0u];
                                const float p = w * vn; // (rounded on its own: contraction is off in this library)
                                num[k] = in ? num[k] + p : num[k];
                                den[k] = in ? den[k] + w : den[k];
                            }
                        }
                }
                if(gx < dim_x)
                {
                    float* __restrict__ out = dst + (z - z_first) * plane + gx;
#pragma unroll
                    for(uint32_t k = 0; k < S::PER_LANE; ++k)
                    {
                        const uint64_t gy = static_cast<uint64_t>(y0) + row0 + k;
                        if(gy < dim_y)
                            out[gy * dim_x] = __builtin_fabsf(vc[k]) < __builtin_inff() ? num[k] / den[k] : vc[k];
                    }
                }
                __syncthreads(); // before the next step overwrites slice z - R
            }
        }
    }

    // the ctx's tables for this setting, uploaded when it differs from the one last used
    int bl_ensure_tables(paris_hip_ctx* ctx, const struct paris_hip_volume_bilateral* setting)
    {
        paris_hip_ctx::volume_bilateral_t& b = ctx->volume_bilateral;
        if(b.set && std::memcmp(&b.rule, setting, sizeof(*setting)) == 0)
            return PARIS_HIP_SUCCESS;
        const uint32_t side = 2u * setting->radius + 1u, taps = side * side * side;
        std::vector<float> spatial(taps), range(PARIS_HIP_BILATERAL_BINS);
        float rscale = 0.f;
        if(int rc = paris_hip_volume_bilateral_tables(setting, spatial.data(), range.data(), &rscale))
            return rc;
        const size_t range_bytes = range.size() * sizeof(float), spatial_bytes = spatial.size() * sizeof(float);
        paris_hip_device_buffer mem;
        if(int rc = paris_hip_install(ctx, range_bytes + spatial_bytes, {{0u, range.data(), range_bytes}, {range_bytes, spatial.data(), spatial_bytes}},
                                      &mem))
            return rc;
        paris_hip_release(ctx, b); // kernels already queued still read the old tables: retired, not freed
        b.set = true;
        std::memcpy(&b.rule, setting, sizeof(*setting));
        b.rscale = rscale;
        b.mem = mem;
        return PARIS_HIP_SUCCESS;
    }
}

namespace
{
    // enqueues the kernel of radius R and tiles TY rows high for arguments already checked, with the ctx's tables
    template <int R, uint32_t TY>
    void bl_launch(paris_hip_ctx* ctx, const float* d_src, uint32_t dim_x, uint32_t dim_y, uint32_t src_dim_z, uint32_t z_first, uint32_t z_count,
                   float* d_dst)
    {
        const uint32_t tiles_x = (dim_x + BL_TX - 1u) / BL_TX, tiles_y = (dim_y + TY - 1u) / TY;
        const uint64_t tiles = static_cast<uint64_t>(tiles_x) * tiles_y;
        // deep chunks pay the 2R slices of the prologue less often; shallow ones give a small volume enough workgroups
        uint32_t z_chunk = BL_Z_CHUNK_MAX;
        while(z_chunk > BL_Z_CHUNK_MIN && tiles * ((z_count + z_chunk - 1u) / z_chunk) < BL_GRID_MAX)
            z_chunk /= 2u;
        const uint64_t items = tiles * ((static_cast<uint64_t>(z_count) + z_chunk - 1u) / z_chunk);
        const uint32_t blocks = static_cast<uint32_t>(std::min<uint64_t>(BL_GRID_MAX, items));
        const int vec = reinterpret_cast<uintptr_t>(d_src) % 16u == 0u && dim_x % 4u == 0u ? 1 : 0;
        const paris_hip_ctx::volume_bilateral_t& b = ctx->volume_bilateral;
        hipLaunchKernelGGL((volume_bilateral_kernel<R, TY>), dim3(blocks), dim3(BL_THREADS), 0, ctx->stream, d_src, dim_x, dim_y, src_dim_z, z_first, z_count, z_chunk, tiles_x,
                           tiles_y, items, b.mem.as<float>(), b.rscale, vec, d_dst);
    }
}

extern "C" int paris_hip_volume_bilateral(paris_hip_ctx* ctx, const float* d_src, uint32_t dim_x, uint32_t dim_y, uint32_t src_dim_z,
                                          uint32_t z_first, uint32_t z_count, const struct paris_hip_volume_bilateral* setting, float* d_dst)
{
    if(int rc = paris_hip_flush_deferred(ctx))
        return rc;
    if(int rc = paris_hip_bind(ctx))
        return rc;
    if(int rc = paris_hip_volume_bilateral_check_call(d_src, dim_x, dim_y, src_dim_z, z_first, z_count, setting, d_dst))
        return rc;
    if(int rc = bl_ensure_tables(ctx, setting))
        return rc;
    const uint64_t plane = static_cast<uint64_t>(dim_x) * dim_y;
    if(int rc = paris_hip_volume_mark_dirty(ctx, d_dst, plane * z_count * sizeof(float))) // (a result can be -0)
        return rc;
    const uint32_t r = setting->radius;
#ifdef PARIS_HIP_EXPERIMENTS
    static const int forced = [] { const char* e = std::getenv("PARIS_BILATERAL_TILE_Y"); return e ? std::atoi(e) : 0; }(); // A/B switch
    if(forced == 16 && r == 3u)
        bl_launch<3, BL_TY_SHALLOW>(ctx, d_src, dim_x, dim_y, src_dim_z, z_first, z_count, d_dst);
    else if(forced == 8 && r == 1u)
        bl_launch<1, BL_TY_DEEP>(ctx, d_src, dim_x, dim_y, src_dim_z, z_first, z_count, d_dst);
    else if(forced == 8 && r == 2u)
        bl_launch<2, BL_TY_DEEP>(ctx, d_src, dim_x, dim_y, src_dim_z, z_first, z_count, d_dst);
    else
#endif
    if(r == 1u)
        bl_launch<1, BL_TY_SHALLOW>(ctx, d_src, dim_x, dim_y, src_dim_z, z_first, z_count, d_dst);
    else if(r == 2u)
        bl_launch<2, BL_TY_SHALLOW>(ctx, d_src, dim_x, dim_y, src_dim_z, z_first, z_count, d_dst);
    else
        bl_launch<3, BL_TY_DEEP>(ctx, d_src, dim_x, dim_y, src_dim_z, z_first, z_count, d_dst);
    return paris_hip_finish(ctx);
}

void paris_hip_warm_volume_bilateral()
{
    hipFuncAttributes a{};
    (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&volume_bilateral_kernel<1, BL_TY_SHALLOW>));
    (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&volume_bilateral_kernel<2, BL_TY_SHALLOW>));
    (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&volume_bilateral_kernel<3, BL_TY_DEEP>));
}
