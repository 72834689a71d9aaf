// The adaptive frame filter against photon starvation on the host (the statement is in include/paris_hip.h).
// Plain host code: it needs no device and no ctx. The check and the tables have their only implementation here -- the device path
// (starvation.hip) calls them -- and the rule is restated pixel by pixel, tap by tap, in the order the statement gives; the kernels
// must give the same bits.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "paris_hip_internal.h"

extern "C" int paris_hip_starvation_filter_check(const paris_hip_starvation_filter* s, uint32_t dim_x, uint32_t dim_y, size_t* device_bytes)
{
    if(s == nullptr || dim_x == 0u || dim_y == 0u)
        return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    if(!std::isfinite(s->p0) || !std::isfinite(s->gain) || !(s->gain > 0.f) || s->radius < 1u || s->radius > PARIS_HIP_STARVATION_RADIUS_MAX)
        return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    const uint64_t n = static_cast<uint64_t>(dim_x) * dim_y;
    if(n > 0xffffffffull)
        return PARIS_HIP_ERROR_UNSUPPORTED;
    if(device_bytes != nullptr)
        *device_bytes = PARIS_HIP_STARVATION_HEAD_BYTES + static_cast<size_t>(PARIS_HIP_STARVATION_FRAMES_MAX) * n * sizeof(float);
    return PARIS_HIP_SUCCESS;
}

extern "C" int paris_hip_starvation_filter_tables(const paris_hip_starvation_filter* s, float* sigma, float* g)
{
    if(paris_hip_starvation_filter_check(s, 1u, 1u, nullptr) != PARIS_HIP_SUCCESS)
        return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    const double pi = 3.14159265358979323846, r = static_cast<double>(s->radius), gain = static_cast<double>(s->gain);
    for(uint32_t k = 0; k < PARIS_HIP_STARVATION_LEVELS; ++k)
    {
        const double e = (static_cast<double>(k) + 0.5) / 16.0;
        const double sg = std::min(r / 2.0, gain * std::sqrt(std::expm1(e) / (4.0 * pi)));
        if(sigma != nullptr)
            sigma[k] = static_cast<float>(sg);
        if(g != nullptr)
        {
            g[k * (s->radius + 1u)] = 1.f;
            for(uint32_t d = 1; d <= s->radius; ++d)
                g[k * (s->radius + 1u) + d] = static_cast<float>(std::exp(-static_cast<double>(d * d) / (2.0 * sg * sg)));
        }
    }
    return PARIS_HIP_SUCCESS;
}

extern "C" int paris_hip_starvation_filter_host(const paris_hip_starvation_filter* s, const float* src, float* dst, uint32_t dim_x, uint32_t dim_y,
                                                paris_hip_starvation_counts* counts)
{
    if(int rc = paris_hip_starvation_filter_check(s, dim_x, dim_y, nullptr))
        return rc;
    if(src == nullptr || dst == nullptr)
        return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    const int r = static_cast<int>(s->radius);
    std::vector<float> g(static_cast<size_t>(PARIS_HIP_STARVATION_LEVELS) * (s->radius + 1u));
    (void)paris_hip_starvation_filter_tables(s, nullptr, g.data());
    const float p0 = s->p0;
    const int64_t nx = dim_x, ny = dim_y;
    uint64_t filtered = 0, last = 0;
    for(int64_t y = 0; y < ny; ++y)
        for(int64_t x = 0; x < nx; ++x)
        {
            const size_t at = static_cast<size_t>(y) * dim_x + static_cast<size_t>(x);
            const float c = src[at];
            dst[at] = c;
            if(!(c > p0))
                continue;
            const float t = (c - p0) * 16.f;
            const uint32_t k = t < 64.f ? static_cast<uint32_t>(t) : 63u;
            const float* gk = g.data() + k * (s->radius + 1u);
            float num = 0.f, den = 0.f;
            for(int dy = -r; dy <= r; ++dy)
                for(int dx = -r; dx <= r; ++dx)
                {
                    const int64_t tx = x + dx, ty = y + dy;
                    if(tx < 0 || tx >= nx || ty < 0 || ty >= ny)
                        continue;
                    const float v = src[static_cast<size_t>(ty) * dim_x + static_cast<size_t>(tx)];
                    if(!std::isfinite(v))
                        continue;
                    const float w = gk[dy < 0 ? -dy : dy] * gk[dx < 0 ? -dx : dx];
                    const float p = w * v; // (rounded on its own: contraction is off in this library)
                    num = num + p;
                    den = den + w;
                }
            if(den == 0.f)
                continue;
            dst[at] = num / den;
            ++filtered;
            last += k == 63u ? 1u : 0u;
        }
    if(counts != nullptr)
    {
        counts->frames = 1u;
        counts->filtered = filtered;
        counts->last_level = last;
    }
    return PARIS_HIP_SUCCESS;
}
