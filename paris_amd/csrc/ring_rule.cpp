// The correction frame of the ring filter (the statement is in include/paris_hip.h). Plain host code: it needs
// no device and no ctx, and it is the only implementation of the rule -- the device (ring.hip) sums the frames and subtracts the
// frame made here.
//
// One mean frame is read once per scan, so the running median is a plain selection per pixel: 2h + 1 <= 65 values each.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>

#include "paris_hip.h"

extern "C" int paris_hip_ring_filter_check(const paris_hip_ring_filter* rf, uint32_t dim_x, uint32_t dim_y, size_t* profile_bytes,
                                           size_t* correction_bytes)
{
    if(rf == nullptr || dim_x == 0 || dim_y == 0)
        return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    if(rf->half_width < 1u || rf->half_width > 32u)
        return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    if(!std::isfinite(rf->floor_abs) || rf->floor_abs < 0.f)
        return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    if(!std::isfinite(rf->limit_abs) || (rf->limit_abs != 0.f && !(rf->limit_abs > rf->floor_abs)))
        return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    const uint64_t n = static_cast<uint64_t>(dim_x) * dim_y;
    if(n > std::numeric_limits<uint32_t>::max()) // (the kernels index a frame's pixels with 32 bits)
        return PARIS_HIP_ERROR_UNSUPPORTED;
    if(profile_bytes != nullptr)
        *profile_bytes = static_cast<size_t>(n) * sizeof(double);
    if(correction_bytes != nullptr)
        *correction_bytes = static_cast<size_t>(n) * sizeof(float);
    return PARIS_HIP_SUCCESS;
}

extern "C" int paris_hip_ring_correction_from_mean(const paris_hip_ring_filter* rf, const float* mean, const uint32_t* count_per_row,
                                                   uint32_t dim_x, uint32_t dim_y, float* c, paris_hip_ring_stats* out)
{
    if(int rc = paris_hip_ring_filter_check(rf, dim_x, dim_y, nullptr, nullptr))
        return rc;
    if(mean == nullptr || c == nullptr)
        return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    const int64_t h = rf->half_width, x_last = static_cast<int64_t>(dim_x) - 1;
    paris_hip_ring_stats st{};
    if(count_per_row != nullptr)
    {
        st.frames_min = *std::min_element(count_per_row, count_per_row + dim_y);
        st.frames_max = *std::max_element(count_per_row, count_per_row + dim_y);
    }
    float window[65];
    for(uint32_t y = 0; y < dim_y; ++y)
    {
        const float* row = mean + static_cast<size_t>(y) * dim_x;
        float* c_row = c + static_cast<size_t>(y) * dim_x;
        if(count_per_row != nullptr && count_per_row[y] == 0u)
        {
            std::fill(c_row, c_row + dim_x, 0.f);
            continue;
        }
        for(int64_t x = 0; x <= x_last; ++x)
        {
            bool finite = true;
            for(int64_t d = -h; d <= h; ++d)
            {
                const float v = row[std::min(std::max<int64_t>(x + d, 0), x_last)];
                finite = finite && std::isfinite(v);
                window[d + h] = v;
            }
            c_row[x] = 0.f;
            if(!finite)
            {
                ++st.not_finite;
                continue;
            }
            std::nth_element(window, window + h, window + 2 * h + 1);
            const float diff = row[x] - window[h];
            const float a = std::fabs(diff);
            if(a < rf->floor_abs)
                ++st.below_floor;
            else if(rf->limit_abs != 0.f && a > rf->limit_abs)
                ++st.above_limit;
            else if(a != 0.f) // (a kept -0 counts as 0)
            {
                c_row[x] = diff;
                ++st.corrected;
                st.max_abs = std::max(st.max_abs, a);
            }
        }
    }
    if(out != nullptr)
        *out = st;
    return PARIS_HIP_SUCCESS;
}
