// Air-region normalisation on the host (the statement is in include/paris_hip.h). Plain host code: it needs no
// device and no ctx. The check has its only implementation here; the value of a frame is restated for a dense frame, in the order
// the statement fixes, and the device (air_region.hip) implements the same rule for the frames of a scan.
#include <cmath>
#include <cstdint>

#include "paris_hip_internal.h"

extern "C" int paris_hip_air_region_check(const paris_hip_air_region* ar, uint32_t dim_x, uint32_t dim_y, uint32_t* min_pixels,
                                          size_t* device_bytes)
{
    if(ar == nullptr || dim_x == 0 || dim_y == 0)
        return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    if(ar->width == 0 || ar->height == 0 || ar->x0 >= dim_x || ar->y0 >= dim_y || ar->width > dim_x - ar->x0 || ar->height > dim_y - ar->y0)
        return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    const uint64_t pixels = static_cast<uint64_t>(ar->width) * ar->height;
    if(pixels > (uint64_t{1} << 20) || ar->min_pixels > pixels)
        return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    if(!std::isfinite(ar->limit_abs) || ar->limit_abs < 0.f)
        return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    if(min_pixels != nullptr)
        *min_pixels = ar->min_pixels != 0u ? ar->min_pixels : static_cast<uint32_t>((pixels + 1u) / 2u);
    if(device_bytes != nullptr)
        *device_bytes = paris_hip_air_layout_of(ar->width, ar->height).bytes;
    return PARIS_HIP_SUCCESS;
}

extern "C" int paris_hip_air_value_host(const paris_hip_air_region* ar, const uint8_t* mask, const float* frame, uint32_t dim_x, uint32_t dim_y,
                                        float* a, uint32_t* n)
{
    uint32_t min_pixels = 0;
    if(int rc = paris_hip_air_region_check(ar, dim_x, dim_y, &min_pixels, nullptr))
        return rc;
    if(frame == nullptr)
        return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    double total = 0.0;
    uint32_t count = 0;
    for(uint32_t l = 0; l < 256u; ++l) // the partial sums, combined in ascending order as they are formed
    {
        const uint32_t c = l % 64u, r = l / 64u;
        double acc = 0.0;
        for(uint32_t y = r; y < ar->height; y += 4u)
            for(uint32_t x = c; x < ar->width; x += 64u)
            {
                const size_t k = static_cast<size_t>(ar->y0 + y) * dim_x + ar->x0 + x;
                if((mask != nullptr && mask[k] != 0u) || !std::isfinite(frame[k]))
                    continue;
                acc += static_cast<double>(frame[k]);
                ++count;
            }
        total = l == 0u ? acc : total + acc;
    }
    float value = 0.f;
    if(count >= min_pixels)
    {
        value = static_cast<float>(total / static_cast<double>(count));
        if(ar->limit_abs != 0.f && std::fabs(value) > ar->limit_abs)
            value = 0.f;
    }
    if(a != nullptr)
        *a = value;
    if(n != nullptr)
        *n = count;
    return PARIS_HIP_SUCCESS;
}
