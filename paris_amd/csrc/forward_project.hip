// Cone-beam forward projection for gfx950: the projections of a volume on the device, in the backprojector's geometry.
//
// Joseph's method. Every detector pixel casts one ray from the source to its centre; the ray is sampled once per voxel plane along
// the axis (x or y) it runs more nearly parallel to, bilinearly in that plane. No step size: the result is fully defined. For a
// view with s = sin phi, c = cos phi (fp32 arguments), d_sd = |d_so| + |d_od| and the offsets delta_s, delta_t in mm:
//
//   pixel (i, j), column i in [0, n_row), row j in [0, n_col):
//     t = (i + 1/2) l_px_row - n_row l_px_row / 2 - delta_s,   z = (j + 1/2) l_px_col - n_col l_px_col / 2 - delta_t
//     source S = (-d_so c, -d_so s, 0),   direction (dx, dy, dz) = (d_sd c - t s, d_sd s + t c, z)
//   x-marching when |dx| >= |dy|, else y-marching (the same with x and y exchanged):
//     for every plane K in [0, dim_x):  x_K = -(dim_x l_vx_x / 2) + l_vx_x / 2 + K l_vx_x
//       a = (x_K - S_x) / dx;  planes with a <= 0 or a > 1 add nothing
//       y = S_y + a dy,  w = a dz,  fy = (y + dim_y l_vx_y / 2) / l_vx_y - 1/2,  fz = (w + dim_z l_vx_z / 2) / l_vx_z - 1/2
//       sample = bilinear over the taps (floor fy, floor fz), (+1, .), (., +1), (+1, +1) of plane K; a tap outside the grid or
//                outside the slab [v_offset, v_offset + v_dim_z) counts as 0 on its own
//     p(i, j) = (sum_K sample_K) l_vx_x sqrt(dx^2 + dy^2 + dz^2) / |dx|
//
// One lane per detector pixel, views on grid.z, workgroups of 64 x 4 or 16 x 16 pixels (below). What is done once per ray is
// formed in double from the fp32 arguments (nothing contracted): t, z, the direction, the choice of the marching axis -- |dx| >=
// |dy| exactly as written, so a float64 restatement makes the same choice for every ray, at 45 degrees too --, the range of
// planes between source and detector, the fractional indices at the middle plane of the run (integer part and fraction), their
// increments per plane and the length factor. fy and fz are linear in K, so the per-plane work is fp32: two fmaf from the middle
// plane's indices, two floors, four taps, the sum in plane order (in runs of 16 planes). The planes on which neither tap column
// can lie inside the grid and the slab are cut off the run beforehand (with a margin far beyond the fp32 rounding of the indices;
// every tap still checks its own bounds), so a ray that misses the grid leaves at once and the result does not depend on the
// cut. With accumulate the finished sum is added to the stored pixel in one fp32 addition.
//
// Memory pattern: with y-marching the taps of neighbouring columns are neighbours in x and a wave's loads coalesce; with x-marching
// every lane reads 128-byte lines of its own and comes back to them on the next planes: that case lives on L1 reuse, which the
// launch shapes below protect, and is bound by the rate of L1 line accesses (DESIGN.md section 4.8 has the measurements, and what
// would cut the accesses: a box of planes staged through LDS, or 16-byte loads along x). Voxel offsets are 64-bit.
#include <cmath>
#include <cstdlib>

#include "frame_pass.h"

namespace
{
    // Detector pixels of a workgroup, columns x rows. 64 x 4 (a wave = 64 columns of one row) where every ray of the view marches
    // along y: the taps of a wave are 2 to 4 runs of consecutive floats. 16 x 16 (a wave = 16 columns x 4 rows) otherwise: with
    // x-marching every lane has lines of its own, and the squarer patch shares more of them between lanes (DESIGN.md section 4.8:
    // -7 % at 0 degrees, -32 % at 45 degrees, +15 % at 90 degrees against 64 x 4); those launches also run one workgroup per CU
    // (lds_pad below). The result does not depend on the shape.
    constexpr uint32_t FP_THREADS = 256u;
    constexpr double FP_WIDE_MIN_SIN = 0.92; // 64 x 4 when |sin phi| >= this: the central ray within 23 degrees of the y axis
    constexpr uint32_t FP_MAX_VIEWS = 64u;   // views per launch: their angles travel as a kernel argument
    constexpr double FP_INDEX_MARGIN = 1e-2; // [voxels] by which the plane cut widens the grid: the fp32 indices are off by < 1e-3

    struct view_angles
    {
        double sin_phi[FP_MAX_VIEWS], cos_phi[FP_MAX_VIEWS];
    };

    struct fp_geometry
    {
        double l_px_row, l_px_col, t_half, z_half; // n_row l_px_row / 2, n_col l_px_col / 2
        double delta_s, delta_t;                   // [mm]
        double d_so, d_sd;
        double l_vx[3];
        uint32_t dim[3];     // the full grid
        uint32_t z_first, z_count; // the slab
        uint32_t n_row, n_col;
    };

    // the planes K in [lo, hi] on which f0 + K df lies within (first - 1 - margin, end + margin): outside it both taps miss
    __host__ __device__ inline void cut_planes(double f0, double df, double first, double end, double& lo, double& hi)
    {
        const double a = first - 1.0 - FP_INDEX_MARGIN, b = end + FP_INDEX_MARGIN;
        if(df == 0.0)
        {
            if(!(f0 > a && f0 < b))
                hi = lo - 1.0;
            return;
        }
        const double k_a = (a - f0) / df, k_b = (b - f0) / df;
        lo = fmax(lo, floor(fmin(k_a, k_b)) - 1.0);
        hi = fmin(hi, ceil(fmax(k_a, k_b)) + 1.0);
    }

    // p(i, j) of the view with sine s and cosine c. Plain C++ on purpose (host too): the ray loop can be stepped through in a CPU build.
    __host__ __device__ inline float ray_integral(const float* __restrict__ vol, const fp_geometry& g, double s, double c, uint32_t i, uint32_t j)
    {
        const double t = (static_cast<double>(i) + 0.5) * g.l_px_row - g.t_half - g.delta_s;
        const double dz = (static_cast<double>(j) + 0.5) * g.l_px_col - g.z_half - g.delta_t;
        const double dx = g.d_sd * c - t * s, dy = g.d_sd * s + t * c;
        const bool x_march = fabs(dx) >= fabs(dy);
        // p: the marching axis, u: the other one of x and y
        const double d_p = x_march ? dx : dy, d_u = x_march ? dy : dx;
        const double s_p = x_march ? -g.d_so * c : -g.d_so * s, s_u = x_march ? -g.d_so * s : -g.d_so * c;
        const double l_p = x_march ? g.l_vx[0] : g.l_vx[1], l_u = x_march ? g.l_vx[1] : g.l_vx[0], l_z = g.l_vx[2];
        const uint32_t n_p = x_march ? g.dim[0] : g.dim[1], n_u = x_march ? g.dim[1] : g.dim[0];
        const auto plane = [&](double k) { return -(static_cast<double>(n_p) * l_p / 2.0) + l_p / 2.0 + k * l_p; };
        const auto a_of = [&](double k) { return (plane(k) - s_p) / d_p; };

        // planes between source and detector: 0 < a <= 1. a is monotone in K, so an estimate is walked to the exact edges with
        // the statement's own expression
        double lo = 0.0, hi = static_cast<double>(n_p) - 1.0;
        {
            const double k_src = (s_p - plane(0.0)) / l_p, k_det = (s_p + d_p - plane(0.0)) / l_p; // a = 0 and a = 1
            double k_lo = d_p > 0.0 ? floor(k_src) : ceil(k_det), k_hi = d_p > 0.0 ? floor(k_det) : ceil(k_src);
            k_lo = fmax(k_lo - 1.0, lo);
            k_hi = fmin(k_hi + 1.0, hi);
            const auto inside = [&](double k) { const double a = a_of(k); return a > 0.0 && a <= 1.0; };
            while(k_lo <= k_hi && !inside(k_lo))
                k_lo += 1.0;
            while(k_hi >= k_lo && !inside(k_hi))
                k_hi -= 1.0;
            lo = k_lo;
            hi = k_hi;
        }
        // fu = fu_0 + K dfu, fz = fz_0 + K dfz
        const double a_0 = a_of(0.0), da = l_p / d_p;
        const double fu_0 = (s_u + a_0 * d_u + static_cast<double>(n_u) * l_u / 2.0) / l_u - 0.5, dfu = da * d_u / l_u;
        const double fz_0 = (a_0 * dz + static_cast<double>(g.dim[2]) * l_z / 2.0) / l_z - 0.5, dfz = da * dz / l_z;
        cut_planes(fu_0, dfu, 0.0, static_cast<double>(n_u), lo, hi);
        cut_planes(fz_0, dfz, static_cast<double>(g.z_first), static_cast<double>(g.z_first) + static_cast<double>(g.z_count), lo, hi);

        // the sum in plane order, 16 planes at a time: the partial sums stay small, so the long sum rounds a sixteenth as often
        float sum = 0.f, part = 0.f;
        if(lo <= hi)
        {
            const uint32_t k_first = static_cast<uint32_t>(lo), planes = static_cast<uint32_t>(hi - lo) + 1u;
            // the indices at the run's middle plane in double (the slab's first slice taken off fz), split into their integer parts
            // and fp32 fractions: the fp32 indices then run about zero, where they are finest
            const int k_mid = static_cast<int>(planes / 2u);
            const double mid = lo + static_cast<double>(k_mid);
            const double fu_m = fu_0 + mid * dfu, fz_m = fz_0 + mid * dfz - static_cast<double>(g.z_first);
            const double fl_um = floor(fu_m), fl_zm = floor(fz_m);
            const int u_base = static_cast<int>(fl_um), z_base = static_cast<int>(fl_zm);
            const float fu_s = static_cast<float>(fu_m - fl_um), fz_s = static_cast<float>(fz_m - fl_zm);
            const float dfu_f = static_cast<float>(dfu), dfz_f = static_cast<float>(dfz);
            const size_t st_p = x_march ? size_t{1} : size_t{g.dim[0]}, st_u = x_march ? size_t{g.dim[0]} : size_t{1};
            const size_t st_z = static_cast<size_t>(g.dim[0]) * g.dim[1];
            const float* base = vol + static_cast<size_t>(k_first) * st_p;
            const int u_last = static_cast<int>(n_u) - 1, z_last = static_cast<int>(g.z_count) - 1;
#pragma unroll 4
            for(uint32_t k = 0; k < planes; ++k)
            {
                const float kf = static_cast<float>(static_cast<int>(k) - k_mid);
                const float fu = fmaf(kf, dfu_f, fu_s), fz = fmaf(kf, dfz_f, fz_s);
                const float fl_u = floorf(fu), fl_z = floorf(fz);
                const float wu = fu - fl_u, wz = fz - fl_z;
                const int iu = u_base + static_cast<int>(fl_u), iz = z_base + static_cast<int>(fl_z);
                const bool u0 = iu >= 0 && iu <= u_last, u1 = iu >= -1 && iu < u_last;
                const bool z0 = iz >= 0 && iz <= z_last, z1 = iz >= -1 && iz < z_last;
                const float* q = base + static_cast<size_t>(k) * st_p + static_cast<ptrdiff_t>(iu) * static_cast<ptrdiff_t>(st_u)
                                 + static_cast<ptrdiff_t>(iz) * static_cast<ptrdiff_t>(st_z);
                const float v00 = (u0 && z0) ? q[0] : 0.f;
                const float v10 = (u1 && z0) ? q[st_u] : 0.f;
                const float v01 = (u0 && z1) ? q[st_z] : 0.f;
                const float v11 = (u1 && z1) ? q[st_u + st_z] : 0.f;
                const float lo_z = (1.f - wu) * v00 + wu * v10, hi_z = (1.f - wu) * v01 + wu * v11;
                part += (1.f - wz) * lo_z + wz * hi_z;
                if((k & 15u) == 15u)
                {
                    sum += part;
                    part = 0.f;
                }
            }
            sum += part;
        }
        const float length = static_cast<float>(l_p * sqrt(dx * dx + dy * dy + dz * dz) / fabs(d_p));
        return sum * length;
    }

    // grid: x = columns, y = rows from row_first, z = views (frame_stride bytes apart)
    template <uint32_t FP_BLOCK_X, uint32_t FP_BLOCK_Y>
    __global__ void __launch_bounds__(FP_THREADS)
        forward_project_kernel(const float* __restrict__ vol, char* p, size_t frame_stride, uint32_t pitch_f, uint32_t row_first,
                               fp_geometry g, view_angles angles, int accumulate)
    {
        const uint32_t i = blockIdx.x * FP_BLOCK_X + threadIdx.x;
        const uint32_t j = row_first + blockIdx.y * FP_BLOCK_Y + threadIdx.y;
        if(i >= g.n_row || j >= g.n_col)
            return;
        const float result = ray_integral(vol, g, angles.sin_phi[blockIdx.z], angles.cos_phi[blockIdx.z], i, j);
        float* out = reinterpret_cast<float*>(p + static_cast<size_t>(blockIdx.z) * frame_stride) + static_cast<size_t>(j) * pitch_f + i;
        *out = accumulate ? *out + result : result;
    }

    // Unused dynamic LDS of the 16 x 16 launches. Their rays have lines of their own, a 128-byte line per lane and tap row that the
    // lane comes back to on the next planes, and with every wave a CU can hold those lines evict each other from its 32 KiB L1
    // before they are used again: the launches wait for L2. 96 KiB per workgroup leaves ONE workgroup (4
    // waves, about 290 lines) on a CU instead of five: 11.7 -> 8.0 ms at 0 degrees, 11.5 -> 6.1 ms at 45 degrees at 1024^3 (64 KiB,
    // two workgroups: 9.7 and 9.3 ms). PARIS_FP_LDS_PAD=bytes (experiments build) sets another amount for an A/B, up to 160 KiB.
    constexpr uint32_t FP_LDS_PAD = 96u * 1024u;

    uint32_t lds_pad()
    {
        uint32_t v = FP_LDS_PAD;
#ifdef PARIS_HIP_EXPERIMENTS
        static const int env = [] { const char* e = std::getenv("PARIS_FP_LDS_PAD"); return e ? std::atoi(e) : -1; }();
        if(env >= 0 && env <= 160 * 1024)
            v = static_cast<uint32_t>(env);
#endif
        if(v > 65536u) // beyond the default limit of dynamic LDS: allowed per kernel (and device)
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&forward_project_kernel<16u, 16u>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      static_cast<int>(v));
        return v;
    }

    bool positive_finite(double v)
    {
        return v > 0.0 && std::isfinite(v);
    }
}

extern "C" int paris_hip_forward_project(paris_hip_ctx* ctx, const float* d_v, uint32_t v_dim_x, uint32_t v_dim_y, uint32_t v_dim_z,
                                         uint32_t v_offset, const paris_detector_geometry* det_geo, const paris_volume_geometry* vol_geo,
                                         float* d_p, size_t p_pitch, size_t p_stride_bytes, uint32_t n_views, uint32_t p_dim_x,
                                         uint32_t p_dim_y, const float* sin_phi, const float* cos_phi, float delta_s, float delta_t,
                                         int accumulate)
{
    if(int rc = paris_hip_bind(ctx))
        return rc;
    if(int rc = paris_hip_flush_deferred(ctx)) // the call reads a volume: what is deferred into it comes first
        return rc;
    // and writes projection buffers, whole frames: the rest is the frame passes' scaffold
    const paris_hip_frame_band frames{d_p, p_pitch, p_stride_bytes, n_views, p_dim_x, p_dim_y, 0u, p_dim_y};
    const auto refuse = [&]() -> int {
        if(det_geo == nullptr || vol_geo == nullptr || (d_v == nullptr && v_dim_z != 0u)
           || (n_views != 0u && (sin_phi == nullptr || cos_phi == nullptr)))
            return PARIS_HIP_ERROR_INVALID_ARGUMENT;
        if(p_dim_x != det_geo->n_row || p_dim_y != det_geo->n_col)
            return PARIS_HIP_ERROR_INVALID_ARGUMENT;
        if(v_dim_x != vol_geo->dim_x || v_dim_y != vol_geo->dim_y || v_offset > vol_geo->dim_z || v_dim_z > vol_geo->dim_z - v_offset)
            return PARIS_HIP_ERROR_INVALID_ARGUMENT;
        if(!positive_finite(det_geo->l_px_row) || !positive_finite(det_geo->l_px_col) || !positive_finite(vol_geo->l_vx_x)
           || !positive_finite(vol_geo->l_vx_y) || !positive_finite(vol_geo->l_vx_z) || !positive_finite(det_geo->d_so)
           || !std::isfinite(det_geo->d_od) || !std::isfinite(delta_s) || !std::isfinite(delta_t))
            return PARIS_HIP_ERROR_INVALID_ARGUMENT;
        for(uint32_t f = 0; f < n_views; ++f)
            if(!std::isfinite(sin_phi[f]) || !std::isfinite(cos_phi[f]))
                return PARIS_HIP_ERROR_INVALID_ARGUMENT;
        return PARIS_HIP_SUCCESS;
    };
    const auto idle = [&] { return v_dim_z == 0u && accumulate != 0; }; // nothing to add
    const auto launch = [&] {
        fp_geometry g{};
        g.l_px_row = det_geo->l_px_row;
        g.l_px_col = det_geo->l_px_col;
        g.t_half = static_cast<double>(p_dim_x) * g.l_px_row / 2.0;
        g.z_half = static_cast<double>(p_dim_y) * g.l_px_col / 2.0;
        g.delta_s = delta_s;
        g.delta_t = delta_t;
        g.d_so = det_geo->d_so;
        g.d_sd = std::abs(static_cast<double>(det_geo->d_so)) + std::abs(static_cast<double>(det_geo->d_od));
        g.l_vx[0] = vol_geo->l_vx_x;
        g.l_vx[1] = vol_geo->l_vx_y;
        g.l_vx[2] = vol_geo->l_vx_z;
        g.dim[0] = vol_geo->dim_x;
        g.dim[1] = vol_geo->dim_y;
        g.dim[2] = vol_geo->dim_z;
        g.z_first = v_offset;
        g.z_count = v_dim_z;
        g.n_row = p_dim_x;
        g.n_col = p_dim_y;
        for(uint32_t f0 = 0; f0 < n_views; f0 += FP_MAX_VIEWS)
        {
            const uint32_t n = std::min(n_views - f0, FP_MAX_VIEWS);
            view_angles a{};
            bool wide = true; // every view of the launch close to the y axis
            for(uint32_t f = 0; f < n; ++f)
            {
                a.sin_phi[f] = sin_phi[f0 + f];
                a.cos_phi[f] = cos_phi[f0 + f];
                wide = wide && std::abs(a.sin_phi[f]) >= FP_WIDE_MIN_SIN;
            }
            const uint32_t bx = wide ? 64u : 16u, by = FP_THREADS / bx;
            const uint32_t rows_per_launch = 65535u * by; // grid.y
            for(uint32_t r0 = 0; r0 < p_dim_y; r0 += rows_per_launch)
            {
                const uint32_t rows = std::min(p_dim_y - r0, rows_per_launch);
                const dim3 grid((p_dim_x + bx - 1u) / bx, (rows + by - 1u) / by, n);
                const auto kernel = wide ? forward_project_kernel<64u, 4u> : forward_project_kernel<16u, 16u>;
                hipLaunchKernelGGL(kernel, grid, dim3(bx, by), wide ? 0u : lds_pad(), ctx->stream, d_v, frames.frame(f0), p_stride_bytes,
                                   static_cast<uint32_t>(p_pitch / sizeof(float)), r0, g, a, accumulate);
            }
        }
    };
    return paris_hip_frame_pass(ctx, frames, refuse, idle, launch, [&] { return frames.rows(); });
}

extern "C" int paris_hip_stage_forward_project(paris_hip_ctx* ctx, const float* d_v, uint32_t v_dim_x, uint32_t v_dim_y, uint32_t v_dim_z,
                                               uint32_t v_offset, const paris_detector_geometry* det_geo,
                                               const paris_volume_geometry* vol_geo, float* d_p, size_t p_pitch, uint32_t p_dim_x,
                                               uint32_t p_dim_y, uint32_t p_idx, float p_phi, int enable_angles, int accumulate)
{
    if(det_geo == nullptr)
        return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    // as paris_hip_stage_backproject derives them (src/backprojection.cpp:49-50)
    const float delta_s = det_geo->delta_s * det_geo->l_px_row;
    const float delta_t = det_geo->delta_t * det_geo->l_px_col;
    float sin_phi = 0.f, cos_phi = 0.f;
    if(int rc = paris_hip_stage_angle(det_geo, p_idx, enable_angles, p_phi, &sin_phi, &cos_phi))
        return rc;
    return paris_hip_forward_project(ctx, d_v, v_dim_x, v_dim_y, v_dim_z, v_offset, det_geo, vol_geo, d_p, p_pitch, 0u, 1u, p_dim_x, p_dim_y,
                                     &sin_phi, &cos_phi, delta_s, delta_t, accumulate);
}

void paris_hip_warm_forward_project()
{
    hipFuncAttributes a{};
    (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&forward_project_kernel<64u, 4u>));
    (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&forward_project_kernel<16u, 16u>));
}
