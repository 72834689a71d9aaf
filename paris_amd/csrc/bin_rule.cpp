// Detector binning on the host (the statement is in include/paris_hip.h). Plain host code: it needs no device
// and no ctx. The check, the binned geometry and the binned mask have their only implementation here; the pixel rule is restated for
// dense frames -- the dark and flat references a driver bins once -- and the device (bin_frames.hip) implements the same rule for the
// frames of a scan.
#include <cstdint>

#include "paris_hip.h"

namespace
{
    bool factor_valid(uint32_t b)
    {
        return b == 1u || b == 2u || b == 4u || b == 8u;
    }
}

extern "C" int paris_hip_binning_check(const paris_hip_binning* bn, uint32_t dim_x, uint32_t dim_y, uint32_t* out_x, uint32_t* out_y)
{
    if(bn == nullptr || !factor_valid(bn->bin_x) || !factor_valid(bn->bin_y))
        return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    const uint32_t ox = dim_x / bn->bin_x, oy = dim_y / bn->bin_y;
    if(ox == 0u || oy == 0u)
        return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    if(out_x != nullptr)
        *out_x = ox;
    if(out_y != nullptr)
        *out_y = oy;
    return PARIS_HIP_SUCCESS;
}

extern "C" int paris_hip_binned_geometry(const paris_hip_binning* bn, const paris_detector_geometry* det_geo, paris_detector_geometry* out_geo)
{
    if(det_geo == nullptr || out_geo == nullptr)
        return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    uint32_t ox = 0, oy = 0;
    if(int rc = paris_hip_binning_check(bn, det_geo->n_row, det_geo->n_col, &ox, &oy))
        return rc;
    // every field from the source fields in double, rounded once
    const double bx = bn->bin_x, by = bn->bin_y;
    const double r_x = det_geo->n_row - ox * bn->bin_x, r_y = det_geo->n_col - oy * bn->bin_y;
    paris_detector_geometry g = *det_geo; // (d_so, d_od, delta_phi stay)
    g.n_row = ox;
    g.n_col = oy;
    g.l_px_row = static_cast<float>(bx * static_cast<double>(det_geo->l_px_row));
    g.l_px_col = static_cast<float>(by * static_cast<double>(det_geo->l_px_col));
    g.delta_s = static_cast<float>((static_cast<double>(det_geo->delta_s) + r_x / 2.0) / bx);
    g.delta_t = static_cast<float>((static_cast<double>(det_geo->delta_t) + r_y / 2.0) / by);
    *out_geo = g;
    return PARIS_HIP_SUCCESS;
}

extern "C" int paris_hip_bin_frame_host(const paris_hip_binning* bn, const uint8_t* mask, const float* src, uint32_t dim_x, uint32_t dim_y,
                                        float* dst)
{
    uint32_t ox = 0, oy = 0;
    if(int rc = paris_hip_binning_check(bn, dim_x, dim_y, &ox, &oy))
        return rc;
    if(src == nullptr || dst == nullptr)
        return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    for(uint32_t Y = 0; Y < oy; ++Y)
        for(uint32_t X = 0; X < ox; ++X)
        {
            float acc = 0.f;
            uint32_t n = 0;
            for(uint32_t y = Y * bn->bin_y; y < (Y + 1u) * bn->bin_y; ++y)
                for(uint32_t x = X * bn->bin_x; x < (X + 1u) * bn->bin_x; ++x)
                {
                    const size_t k = static_cast<size_t>(y) * dim_x + x;
                    if(mask != nullptr && mask[k] != 0u)
                        continue;
                    acc = acc + src[k];
                    ++n;
                }
            dst[static_cast<size_t>(Y) * ox + X] = n != 0u ? acc / static_cast<float>(n) : 0.f;
        }
    return PARIS_HIP_SUCCESS;
}

extern "C" int paris_hip_bin_mask(const paris_hip_binning* bn, const uint8_t* mask, uint32_t dim_x, uint32_t dim_y, uint8_t* out_mask)
{
    uint32_t ox = 0, oy = 0;
    if(int rc = paris_hip_binning_check(bn, dim_x, dim_y, &ox, &oy))
        return rc;
    if(mask == nullptr || out_mask == nullptr)
        return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    for(uint32_t Y = 0; Y < oy; ++Y)
        for(uint32_t X = 0; X < ox; ++X)
        {
            bool good = false; // a bin with one good pixel is good
            for(uint32_t y = Y * bn->bin_y; y < (Y + 1u) * bn->bin_y; ++y)
                for(uint32_t x = X * bn->bin_x; x < (X + 1u) * bn->bin_x; ++x)
                    good = good || mask[static_cast<size_t>(y) * dim_x + x] == 0u;
            out_mask[static_cast<size_t>(Y) * ox + X] = good ? 0u : 1u;
        }
    return PARIS_HIP_SUCCESS;
}
