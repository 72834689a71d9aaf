// Metal artefact reduction on the host (the statement is in include/paris_hip.h). Plain host code: it needs no
// device and no ctx. The check has its only implementation here -- the device path (metal.hip) calls it -- and the four rules are
// restated for dense host arrays, pixel by pixel and run by run; the kernels implement the same definitions with ballots and bit scans.
#include <cmath>
#include <cstdint>

#include "paris_hip_internal.h"

extern "C" int paris_hip_metal_check(uint32_t dim_x, uint32_t dim_y, uint32_t dim_z, float threshold, uint32_t grow, float min_path,
                                     uint64_t* max_voxels)
{
    if(dim_x == 0u || dim_y == 0u || dim_z == 0u || !std::isfinite(threshold) || grow > PARIS_HIP_METAL_GROW_MAX || !std::isfinite(min_path)
       || min_path < 0.f)
        return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    if(max_voxels != nullptr)
    {
        const uint64_t n = static_cast<uint64_t>(dim_x) * dim_y * dim_z / 32u;
        *max_voxels = n < PARIS_HIP_METAL_MIN_VOXELS_CAP ? PARIS_HIP_METAL_MIN_VOXELS_CAP : n;
    }
    return PARIS_HIP_SUCCESS;
}

extern "C" int paris_hip_metal_collect_host(float* v, uint32_t dim_x, uint32_t dim_y, uint32_t dim_z, float threshold, uint64_t max_n,
                                            uint64_t* index, float* value, uint64_t* n, int binarize)
{
    if(v == nullptr || n == nullptr || paris_hip_metal_check(dim_x, dim_y, dim_z, threshold, 0u, 0.f, nullptr) != PARIS_HIP_SUCCESS
       || (max_n != 0u && (index == nullptr || value == nullptr)))
        return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    const uint64_t voxels = static_cast<uint64_t>(dim_x) * dim_y * dim_z;
    uint64_t count = 0;
    for(uint64_t i = 0; i < voxels; ++i)
        count += v[i] > threshold ? 1u : 0u;
    *n = count;
    if(count > max_n)
        return PARIS_HIP_ERROR_METAL_TOO_MANY_VOXELS;
    uint64_t k = 0;
    for(uint64_t i = 0; i < voxels; ++i)
    {
        const bool hit = v[i] > threshold;
        if(hit)
        {
            index[k] = i;
            value[k] = v[i];
            ++k;
        }
        if(binarize)
            v[i] = hit ? 1.f : 0.f;
    }
    return PARIS_HIP_SUCCESS;
}

extern "C" int paris_hip_metal_trace_pack_host(const float* t, uint32_t n_frames, uint32_t dim_x, uint32_t dim_y, float min_path, uint32_t grow,
                                               uint64_t* bits)
{
    if(grow > PARIS_HIP_METAL_GROW_MAX || !std::isfinite(min_path) || min_path < 0.f)
        return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    if(n_frames == 0u || dim_x == 0u || dim_y == 0u)
        return PARIS_HIP_SUCCESS;
    if(t == nullptr || bits == nullptr)
        return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    const uint32_t words = (dim_x + 63u) / 64u;
    for(uint32_t f = 0; f < n_frames; ++f)
    {
        const float* frame = t + static_cast<uint64_t>(f) * dim_x * dim_y;
        uint64_t* out = bits + static_cast<uint64_t>(f) * dim_y * words;
        for(uint32_t y = 0; y < dim_y; ++y)
        {
            const uint32_t y0 = y - (y < grow ? y : grow), y1 = dim_y - 1u - y < grow ? dim_y - 1u : y + grow;
            for(uint32_t w = 0; w < words; ++w)
                out[static_cast<uint64_t>(y) * words + w] = 0u;
            for(uint32_t x = 0; x < dim_x; ++x)
            {
                const uint32_t x0 = x - (x < grow ? x : grow), x1 = dim_x - 1u - x < grow ? dim_x - 1u : x + grow;
                bool hit = false;
                for(uint32_t yy = y0; yy <= y1 && !hit; ++yy)
                    for(uint32_t xx = x0; xx <= x1 && !hit; ++xx)
                        hit = frame[static_cast<uint64_t>(yy) * dim_x + xx] > min_path;
                if(hit)
                    out[static_cast<uint64_t>(y) * words + (x >> 6)] |= uint64_t{1} << (x & 63u);
            }
        }
    }
    return PARIS_HIP_SUCCESS;
}

extern "C" int paris_hip_metal_inpaint_host(float* p, const uint64_t* bits, uint32_t dim_x, uint32_t dim_y, uint32_t row_first, uint32_t row_count,
                                            paris_hip_metal_counts* counts)
{
    if(row_first > dim_y || row_count > dim_y - row_first)
        return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    if(dim_x == 0u || row_count == 0u)
        return PARIS_HIP_SUCCESS;
    if(p == nullptr || bits == nullptr)
        return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    const uint32_t words = (dim_x + 63u) / 64u;
    paris_hip_metal_counts c{0u, 0u, 0u};
    for(uint32_t y = row_first; y < row_first + row_count; ++y)
    {
        float* row = p + static_cast<uint64_t>(y) * dim_x;
        const uint64_t* b = bits + static_cast<uint64_t>(y) * words;
        const auto set = [&](uint32_t x) { return ((b[x >> 6] >> (x & 63u)) & 1u) != 0u; };
        for(uint32_t a = 0; a < dim_x;)
        {
            if(!set(a))
            {
                ++a;
                continue;
            }
            uint32_t e = a; // the run is [a, e)
            while(e < dim_x && set(e))
                ++e;
            if(a == 0u && e == dim_x)
                ++c.rows_left;
            else
            {
                ++c.runs;
                c.replaced += e - a;
                if(a == 0u)
                    for(uint32_t x = a; x < e; ++x)
                        row[x] = row[e];
                else if(e == dim_x)
                    for(uint32_t x = a; x < e; ++x)
                        row[x] = row[a - 1u];
                else
                {
                    const float pl = row[a - 1u], pr = row[e];
                    const float d = pr - pl, len = static_cast<float>(e - a + 1u);
                    for(uint32_t x = a; x < e; ++x)
                        row[x] = std::fmaf(static_cast<float>(x - a + 1u) / len, d, pl);
                }
            }
            a = e;
        }
    }
    if(counts != nullptr)
    {
        counts->replaced += c.replaced;
        counts->runs += c.runs;
        counts->rows_left += c.rows_left;
    }
    return PARIS_HIP_SUCCESS;
}
