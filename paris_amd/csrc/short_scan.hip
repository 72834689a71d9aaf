// Redundancy weights for gfx950: Parker's for short scans and Wang's for offset detectors. Both multiply each column of a raw
// frame by twice a weight of that column's ray, before the cosine weighting, through the frame-pass scaffold (frame_pass.h).
//
// Short scans.
// A short scan covers [start, start + range] in the projection angle phi (the angle the backprojection uses), with
// pi + 2 gamma_m <= range <= 2 pi. The ray of column i at phi has fan angle gamma_i = atan(t_i / d_sd) in the
// backprojector's coordinates, t_i = (i + 1/2) l_px_row - n_row l_px_row / 2 - delta_s l_px_row, and direction angle phi +
// gamma_i, so its conjugate ray is (phi + pi + 2 gamma_i, -gamma_i). With beta = (phi - start) mod 2 pi and delta = (range - pi) / 2:
//
//   w = sin^2(pi/4 * beta / (delta - gamma))                  0               <= beta < 2 delta - 2 gamma
//   w = 1                                                     2 delta - 2 gamma <= beta <= pi - 2 gamma
//   w = sin^2(pi/4 * (pi + 2 delta - beta) / (delta + gamma)) pi - 2 gamma      <  beta <= pi + 2 delta
//   w = 0                                                     otherwise
//
// The weights of a ray and its conjugate add up to 1. Every pixel of column i is multiplied by 2 w: the factor 2 cancels the
// 0.5 of the backprojection (a full circle measures each ray twice), so a short scan reconstructs at the full circle's scale.
// This pass runs on the raw frame before the cosine weighting; everything after it sees an ordinary frame.
//
// One thread per column: it forms 2 w once per frame and streams it down its rows. The weight is formed in double and
// rounded once: near the smallest valid range the ramps of the outermost columns are a fraction of a milliradian wide, and
// the fp32 rounding of gamma or beta would be magnified by (pi / 4) / (delta -+ gamma). In the middle region the factor is
// exactly 2.0f. Memory bound: 8 B per pixel (one read, one write).
//
// Offset detectors (half fan). The detector covers [-t_half, n_row l_px_row - t_half] in t, so the rays within the overlap
// |t| < tau = min(t_half, n_row l_px_row - t_half) are measured twice per circle and the others once. With gamma_tau =
// atan(tau / d_sd), sigma = +1 when the detector reaches further to +t (delta_s <= 0, else -1) and x = sigma gamma_i / gamma_tau:
//
//   2 w = 2                          x >= 1       (the long side: measured once)
//   2 w = 2 sin^2(pi/4 (1 + x))      -1 < x < 1   (the overlap)
//   2 w = 0                          x <= -1
//
// The weights of t and -t add up to 2, and the conjugate of (phi, gamma) is (phi + pi + 2 gamma, -gamma), so a full circle
// counts every ray once; the factor 2 again cancels the backprojection's 0.5. The weight does not depend on the angle. It is
// formed per column in double and rounded once, like Parker's.
#include <cmath>

#include "frame_pass.h"

namespace
{
    constexpr uint32_t SS_THREADS = 256u;
    constexpr uint32_t SS_MAX_FRAMES = 64u;      // frames per launch: their angles travel as a kernel argument
    constexpr uint32_t SS_ROWS_PER_THREAD = 8u;  // rows a thread streams its column's weight down (grid-y strides over the band)

    struct frame_angles
    {
        double beta[SS_MAX_FRAMES]; // (phi - start) mod 2 pi of each frame of the launch, radians
    };

    // 2 w(beta, gamma) of the table above; never divides unless the divisor is positive (beta >= 0)
    __device__ inline float twice_weight(double beta, double gamma, double delta)
    {
        const double rest = M_PI + 2.0 * delta - beta; // the scan's end lies this far ahead
        if(!(rest >= 0.0))
            return 0.f;
        const double rise = delta - gamma;
        if(beta < 2.0 * rise)
        {
            const double s = sin(M_PI_4 * beta / rise);
            return static_cast<float>(2.0 * s * s);
        }
        const double fall = delta + gamma;
        if(rest < 2.0 * fall)
        {
            const double s = sin(M_PI_4 * rest / fall);
            return static_cast<float>(2.0 * s * s);
        }
        return 2.f;
    }

    // grid: x = columns, y = row slices striding over [row_first, row_end), z = frames (frame_stride bytes apart)
    __global__ void __launch_bounds__(SS_THREADS)
        short_scan_kernel(char* p, size_t frame_stride, uint32_t pitch_f, uint32_t dim_x, uint32_t row_first, uint32_t row_end,
                          double t_half, double l_px_row, double d_sd, double delta, frame_angles angles)
    {
        const uint32_t s = blockIdx.x * SS_THREADS + threadIdx.x;
        if(s >= dim_x)
            return;
        const double t_s = (static_cast<double>(s) + 0.5) * l_px_row - t_half;
        const float w2 = twice_weight(angles.beta[blockIdx.z], atan(t_s / d_sd), delta);
        float* frame = reinterpret_cast<float*>(p + static_cast<size_t>(blockIdx.z) * frame_stride);
        for(uint32_t t = row_first + blockIdx.y; t < row_end; t += gridDim.y)
            frame[static_cast<size_t>(t) * pitch_f + s] *= w2;
    }

    // 2 w of the offset-detector table above, x = sigma gamma / gamma_tau
    __device__ inline float twice_offset_weight(double x)
    {
        if(x >= 1.0)
            return 2.f;
        if(!(x > -1.0))
            return 0.f;
        const double s = sin(M_PI_4 * (1.0 + x));
        return static_cast<float>(2.0 * s * s);
    }

    // grid: as short_scan_kernel's; one weight per column for every frame
    __global__ void __launch_bounds__(SS_THREADS)
        offset_detector_kernel(char* p, size_t frame_stride, uint32_t pitch_f, uint32_t dim_x, uint32_t row_first, uint32_t row_end,
                               double t_half, double l_px_row, double d_sd, double sigma, double gamma_tau)
    {
        const uint32_t s = blockIdx.x * SS_THREADS + threadIdx.x;
        if(s >= dim_x)
            return;
        const double t_s = (static_cast<double>(s) + 0.5) * l_px_row - t_half;
        const float w2 = twice_offset_weight(sigma * atan(t_s / d_sd) / gamma_tau);
        float* frame = reinterpret_cast<float*>(p + static_cast<size_t>(blockIdx.z) * frame_stride);
        for(uint32_t t = row_first + blockIdx.y; t < row_end; t += gridDim.y)
            frame[static_cast<size_t>(t) * pitch_f + s] *= w2;
    }

    // d_sd and the two terms of t_i that do not depend on i, in double (the same statement as the check and the tests)
    struct column_geometry
    {
        double t_half; // n_row l_px_row / 2 + delta_s l_px_row
        double l_px_row, d_sd;
    };

    column_geometry columns_of(const paris_detector_geometry& det)
    {
        const double l = det.l_px_row;
        return {static_cast<double>(det.n_row) * l / 2.0 + static_cast<double>(det.delta_s) * l, l,
                std::abs(static_cast<double>(det.d_so)) + std::abs(static_cast<double>(det.d_od))};
    }

    // gamma_m: the largest |fan angle| over the two outermost pixel centres (delta_s included)
    double gamma_max_of(const paris_detector_geometry& det)
    {
        const column_geometry c = columns_of(det);
        const double t_lo = 0.5 * c.l_px_row - c.t_half, t_hi = (det.n_row - 0.5) * c.l_px_row - c.t_half;
        return std::max(std::abs(std::atan(t_lo / c.d_sd)), std::abs(std::atan(t_hi / c.d_sd)));
    }

    // the scan's delta = (range - pi) / 2, or an error for a scan that does not cover every ray once
    int check_scan(const paris_detector_geometry* det, const paris_short_scan* scan, double* delta)
    {
        if(det == nullptr || scan == nullptr || det->n_row == 0)
            return PARIS_HIP_ERROR_INVALID_ARGUMENT;
        const double g = gamma_max_of(*det);
        const double start = scan->start_deg, range = scan->range_deg;
        if(!(columns_of(*det).d_sd > 0.0) || !std::isfinite(g) || !std::isfinite(start) || !std::isfinite(range) || range > 360.0)
            return PARIS_HIP_ERROR_INVALID_ARGUMENT;
        const double d = (range * (M_PI / 180.0) - M_PI) / 2.0;
        if(!(d >= g)) // range < pi + 2 gamma_m: some rays are never measured
            return PARIS_HIP_ERROR_INVALID_ARGUMENT;
        *delta = d;
        return PARIS_HIP_SUCCESS;
    }

    // the offset detector's overlap: sigma (+1: the detector reaches further to +t) and gamma_tau, or an error for a geometry
    // whose central ray misses the detector or lies within 2 pixels of its edge (tau < 2 l_px_row)
    struct overlap
    {
        double tau, gamma_tau, sigma;
    };

    overlap overlap_of(const paris_detector_geometry& det)
    {
        const column_geometry c = columns_of(det);
        const double tau = std::min(c.t_half, static_cast<double>(det.n_row) * c.l_px_row - c.t_half);
        return {tau, std::atan(tau / c.d_sd), det.delta_s <= 0.f ? 1.0 : -1.0};
    }

    int check_offset_detector(const paris_detector_geometry* det, overlap* o)
    {
        if(det == nullptr || det->n_row == 0)
            return PARIS_HIP_ERROR_INVALID_ARGUMENT;
        const column_geometry c = columns_of(*det);
        const overlap v = overlap_of(*det);
        if(!(c.d_sd > 0.0) || !(c.l_px_row > 0.0) || !std::isfinite(c.d_sd) || !std::isfinite(c.t_half) || !std::isfinite(v.gamma_tau))
            return PARIS_HIP_ERROR_INVALID_ARGUMENT;
        if(!(v.tau >= 2.0 * c.l_px_row))
            return PARIS_HIP_ERROR_INVALID_ARGUMENT;
        *o = v;
        return PARIS_HIP_SUCCESS;
    }

    // What the two redundancy weights add to the frame-pass scaffold (frame_pass.h): the frame's columns are the geometry's, then
    // refuse() -- the weight's own checks; launch(grid) enqueues on ctx->stream, grid.z is left for it to set.
    template <typename Refuse, typename Launch>
    int weight_columns(paris_hip_ctx* ctx, const paris_hip_frame_band& b, const paris_detector_geometry* det_geo, Refuse refuse, Launch launch)
    {
        return paris_hip_frame_pass(
            ctx, b,
            [&]() -> int {
                if(det_geo == nullptr || b.dim_x != det_geo->n_row)
                    return PARIS_HIP_ERROR_INVALID_ARGUMENT;
                return refuse();
            },
            [&] {
                const uint32_t slices = (b.row_count + SS_ROWS_PER_THREAD - 1u) / SS_ROWS_PER_THREAD;
                launch(dim3((b.dim_x + SS_THREADS - 1u) / SS_THREADS, slices < 65535u ? slices : 65535u, 1u));
            });
    }
}

extern "C" int paris_hip_short_scan_check(const paris_detector_geometry* det_geo, const paris_short_scan* scan, float* gamma_max_deg)
{
    double delta = 0.0;
    const int rc = check_scan(det_geo, scan, &delta);
    if(gamma_max_deg != nullptr && det_geo != nullptr && det_geo->n_row != 0) // refused scans too: the caller can name the range it needs
        *gamma_max_deg = static_cast<float>(gamma_max_of(*det_geo) * (180.0 / M_PI));
    return rc;
}

extern "C" int paris_hip_short_scan_weight_rows(paris_hip_ctx* ctx, float* d_p, size_t pitch, size_t frame_stride, uint32_t n_frames,
                                                uint32_t dim_x, uint32_t dim_y, uint32_t row_first, uint32_t row_count,
                                                const paris_detector_geometry* det_geo, const paris_short_scan* scan, const float* phi_deg)
{
    const paris_hip_frame_band band{d_p, pitch, frame_stride, n_frames, dim_x, dim_y, row_first, row_count};
    double delta = 0.0;
    const auto refuse = [&]() -> int {
        if(n_frames != 0 && phi_deg == nullptr)
            return PARIS_HIP_ERROR_INVALID_ARGUMENT;
        if(int rc = check_scan(det_geo, scan, &delta))
            return rc;
        for(uint32_t f = 0; f < n_frames; ++f)
            if(!std::isfinite(phi_deg[f]))
                return PARIS_HIP_ERROR_INVALID_ARGUMENT;
        return PARIS_HIP_SUCCESS;
    };
    const auto launch = [&](dim3 grid) {
        const column_geometry c = columns_of(*det_geo);
        for(uint32_t f0 = 0; f0 < n_frames; f0 += SS_MAX_FRAMES)
        {
            const uint32_t n = std::min(n_frames - f0, SS_MAX_FRAMES);
            frame_angles a{};
            for(uint32_t f = 0; f < n; ++f)
            {
                // (phi - start) mod 360 degrees in double, then radians
                double b = std::fmod(static_cast<double>(phi_deg[f0 + f]) - static_cast<double>(scan->start_deg), 360.0);
                if(b < 0.0)
                    b += 360.0;
                a.beta[f] = b * (M_PI / 180.0);
            }
            grid.z = n;
            hipLaunchKernelGGL(short_scan_kernel, grid, dim3(SS_THREADS), 0, ctx->stream, band.frame(f0), frame_stride,
                               static_cast<uint32_t>(pitch / sizeof(float)), dim_x, row_first, row_first + row_count, c.t_half, c.l_px_row,
                               c.d_sd, delta, a);
        }
    };
    return weight_columns(ctx, band, det_geo, refuse, launch);
}

extern "C" int paris_hip_stage_short_scan_weight(paris_hip_ctx* ctx, float* d_p, size_t pitch, uint32_t dim_x, uint32_t dim_y,
                                                 const paris_detector_geometry* det_geo, const paris_short_scan* scan, uint32_t idx,
                                                 int enable_angles, float phi)
{
    if(det_geo == nullptr)
        return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    // the angle of paris_hip_stage_angle (src/backprojection.cpp:52-63), in degrees
    const float a = enable_angles ? phi : static_cast<float>(idx) * det_geo->delta_phi;
    return paris_hip_short_scan_weight_rows(ctx, d_p, pitch, 0u, 1u, dim_x, dim_y, 0u, dim_y, det_geo, scan, &a);
}

extern "C" int paris_hip_offset_detector_check(const paris_detector_geometry* det_geo, float* gamma_tau_deg)
{
    overlap o{};
    const int rc = check_offset_detector(det_geo, &o);
    if(gamma_tau_deg != nullptr && det_geo != nullptr && det_geo->n_row != 0) // refused geometries too: the caller can name the overlap
        *gamma_tau_deg = static_cast<float>(overlap_of(*det_geo).gamma_tau * (180.0 / M_PI));
    return rc;
}

extern "C" int paris_hip_offset_detector_weight_rows(paris_hip_ctx* ctx, float* d_p, size_t pitch, size_t frame_stride, uint32_t n_frames,
                                                     uint32_t dim_x, uint32_t dim_y, uint32_t row_first, uint32_t row_count,
                                                     const paris_detector_geometry* det_geo)
{
    const paris_hip_frame_band band{d_p, pitch, frame_stride, n_frames, dim_x, dim_y, row_first, row_count};
    overlap o{};
    const auto refuse = [&]() -> int { return check_offset_detector(det_geo, &o); };
    const auto launch = [&](dim3 grid) {
        const column_geometry c = columns_of(*det_geo);
        // the weight does not depend on the angle: no per-frame arguments, only the grid-z limit splits a batch
        for(uint32_t f0 = 0; f0 < n_frames; f0 += 65535u)
        {
            grid.z = std::min(n_frames - f0, 65535u);
            hipLaunchKernelGGL(offset_detector_kernel, grid, dim3(SS_THREADS), 0, ctx->stream, band.frame(f0), frame_stride,
                               static_cast<uint32_t>(pitch / sizeof(float)), dim_x, row_first, row_first + row_count, c.t_half, c.l_px_row,
                               c.d_sd, o.sigma, o.gamma_tau);
        }
    };
    return weight_columns(ctx, band, det_geo, refuse, launch);
}

extern "C" int paris_hip_stage_offset_detector_weight(paris_hip_ctx* ctx, float* d_p, size_t pitch, uint32_t dim_x, uint32_t dim_y,
                                                      const paris_detector_geometry* det_geo)
{
    return paris_hip_offset_detector_weight_rows(ctx, d_p, pitch, 0u, 1u, dim_x, dim_y, 0u, dim_y, det_geo);
}

void paris_hip_warm_redundancy_weights()
{
    hipFuncAttributes a{};
    (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&short_scan_kernel));
    (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&offset_detector_kernel));
}
