// The 3-D bilateral filter on the host (the statement is in include/paris_hip.h). Plain host code: it needs no
// device and no ctx. The check and the tables have their only implementation here -- the device path (volume_bilateral.hip) calls
// them -- and the rule is restated voxel by voxel, tap by tap, in the order the statement gives; the kernel must give the same bits.
#include <cmath>
#include <cstdint>
#include <vector>

#include "paris_hip_internal.h"

namespace
{
    // rscale of the rule; false for a setting the check refuses
    bool bilateral_rscale(const struct paris_hip_volume_bilateral* s, float* rscale)
    {
        if(s == nullptr || !std::isfinite(s->sigma_r) || !std::isfinite(s->sigma_s) || !(s->sigma_r > 0.f) || !(s->sigma_s > 0.f))
            return false;
        if(s->radius < 1u || s->radius > PARIS_HIP_BILATERAL_RADIUS_MAX)
            return false;
        const float r = static_cast<float>(static_cast<double>(PARIS_HIP_BILATERAL_BINS) / (4.0 * static_cast<double>(s->sigma_r)));
        if(!std::isfinite(r) || !(r > 0.f))
            return false;
        *rscale = r;
        return true;
    }
}

extern "C" int paris_hip_volume_bilateral_check(const struct paris_hip_volume_bilateral* setting)
{
    float rscale = 0.f;
    return bilateral_rscale(setting, &rscale) ? PARIS_HIP_SUCCESS : PARIS_HIP_ERROR_INVALID_ARGUMENT;
}

extern "C" int paris_hip_volume_bilateral_tables(const struct paris_hip_volume_bilateral* setting, float* spatial, float* range, float* rscale)
{
    float rs = 0.f;
    if(!bilateral_rscale(setting, &rs))
        return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    if(rscale != nullptr)
        *rscale = rs;
    if(spatial != nullptr)
    {
        const int r = static_cast<int>(setting->radius);
        const double two_s2 = 2.0 * static_cast<double>(setting->sigma_s) * static_cast<double>(setting->sigma_s);
        for(int dz = -r; dz <= r; ++dz)
            for(int dy = -r; dy <= r; ++dy)
                for(int dx = -r; dx <= r; ++dx)
                    *spatial++ = static_cast<float>(std::exp(-static_cast<double>(dx * dx + dy * dy + dz * dz) / two_s2));
    }
    if(range != nullptr)
        for(int i = 0; i < PARIS_HIP_BILATERAL_BINS; ++i)
        {
            const double u = (static_cast<double>(i) + 0.5) * 4.0 / static_cast<double>(PARIS_HIP_BILATERAL_BINS);
            range[i] = static_cast<float>(std::exp(-0.5 * u * u));
        }
    return PARIS_HIP_SUCCESS;
}

int paris_hip_volume_bilateral_check_call(const float* src, uint32_t dim_x, uint32_t dim_y, uint32_t src_dim_z, uint32_t z_first, uint32_t z_count,
                                          const struct paris_hip_volume_bilateral* setting, const float* dst)
{
    if(src == nullptr || dst == nullptr || paris_hip_volume_bilateral_check(setting) != PARIS_HIP_SUCCESS)
        return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    if(reinterpret_cast<uintptr_t>(src) % sizeof(float) != 0u || reinterpret_cast<uintptr_t>(dst) % sizeof(float) != 0u)
        return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    if(dim_x == 0u || dim_y == 0u || z_count == 0u || z_first > src_dim_z || z_count > src_dim_z - z_first)
        return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    const uint64_t plane = static_cast<uint64_t>(dim_x) * dim_y; // < 2^64; times a 32-bit depth and 4 it must still fit
    if(plane > (~uint64_t{0}) / sizeof(float) / src_dim_z)
        return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    const uintptr_t s0 = reinterpret_cast<uintptr_t>(src), d0 = reinterpret_cast<uintptr_t>(dst);
    const uint64_t s_bytes = plane * src_dim_z * sizeof(float), d_bytes = plane * z_count * sizeof(float);
    if(s0 < d0 + d_bytes && d0 < s0 + s_bytes)
        return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    return PARIS_HIP_SUCCESS;
}

extern "C" int paris_hip_volume_bilateral_host(const float* src, uint32_t dim_x, uint32_t dim_y, uint32_t src_dim_z, uint32_t z_first,
                                               uint32_t z_count, const struct paris_hip_volume_bilateral* setting, float* dst)
{
    if(int rc = paris_hip_volume_bilateral_check_call(src, dim_x, dim_y, src_dim_z, z_first, z_count, setting, dst))
        return rc;
    const int r = static_cast<int>(setting->radius);
    const int side = 2 * r + 1;
    std::vector<float> spatial(static_cast<size_t>(side) * side * side), range(PARIS_HIP_BILATERAL_BINS);
    float rscale = 0.f;
    (void)paris_hip_volume_bilateral_tables(setting, spatial.data(), range.data(), &rscale);
    const int64_t nx = dim_x, ny = dim_y, nz = src_dim_z;
    const uint64_t plane = static_cast<uint64_t>(dim_x) * dim_y;
    for(int64_t z = z_first; z < static_cast<int64_t>(z_first) + z_count; ++z)
        for(int64_t y = 0; y < ny; ++y)
            for(int64_t x = 0; x < nx; ++x)
            {
                const float vc = src[static_cast<uint64_t>(z) * plane + static_cast<uint64_t>(y) * dim_x + static_cast<uint64_t>(x)];
                float* out = dst + static_cast<uint64_t>(z - z_first) * plane + static_cast<uint64_t>(y) * dim_x + static_cast<uint64_t>(x);
                if(!std::isfinite(vc))
                {
                    *out = vc;
                    continue;
                }
                float num = 0.f, den = 0.f;
                const float* s = spatial.data();
                for(int dz = -r; dz <= r; ++dz)
                    for(int dy = -r; dy <= r; ++dy)
                        for(int dx = -r; dx <= r; ++dx, ++s)
                        {
                            const int64_t tx = x + dx, ty = y + dy, tz = z + dz;
                            if(tx < 0 || tx >= nx || ty < 0 || ty >= ny || tz < 0 || tz >= nz)
                                continue;
                            const float vn = src[static_cast<uint64_t>(tz) * plane + static_cast<uint64_t>(ty) * dim_x + static_cast<uint64_t>(tx)];
                            const float d = std::fabs(vn - vc);
                            const float t = d * rscale;
                            if(!(t < static_cast<float>(PARIS_HIP_BILATERAL_BINS)))
                                continue;
                            const float w = *s * range[static_cast<uint32_t>(t)];
                            const float p = w * vn; // (rounded on its own: contraction is off in this library)
                            num = num + p;
                            den = den + w;
                        }
                *out = num / den;
            }
    return PARIS_HIP_SUCCESS;
}
