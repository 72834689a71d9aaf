// The repair plan of a detector defect map (the statement is in include/paris_hip.h). Plain host code: it
// needs no device and no ctx, and it is the only implementation of the rule -- the device kernel (defect_map.hip) just walks the
// arrays made here.
//
// For every defective pixel the ring radius r_q is found with a summed-area table of the good pixels (one clipped window count per
// candidate radius), then only ring r_q is walked, row-major, for the sources. Weights are formed in double and rounded once.
#include <algorithm>
#include <cstdint>
#include <limits>
#include <memory>
#include <new>

#include "defect_plan.h"

namespace
{
    // good pixels in rows [y0, y1) x columns [x0, x1); sat has (dim_x + 1) entries per row
    inline uint32_t window_count(const std::vector<uint32_t>& sat, size_t w1, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1)
    {
        return sat[y1 * w1 + x1] - sat[y0 * w1 + x1] - sat[y1 * w1 + x0] + sat[y0 * w1 + x0];
    }
}

extern "C" int paris_hip_defect_plan_create(const uint8_t* mask, uint32_t dim_x, uint32_t dim_y, paris_hip_defect_plan** out)
{
    if(mask == nullptr || out == nullptr || dim_x == 0 || dim_y == 0)
        return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    *out = nullptr;
    if(static_cast<uint64_t>(dim_x) * dim_y > std::numeric_limits<uint32_t>::max())
        return PARIS_HIP_ERROR_UNSUPPORTED; // linear pixel indices are 32-bit
    constexpr int64_t R = PARIS_HIP_DEFECT_R_MAX;
    try
    {
        auto plan = std::make_unique<paris_hip_defect_plan>();
        plan->dim_x = dim_x;
        plan->dim_y = dim_y;
        const size_t w1 = static_cast<size_t>(dim_x) + 1u;
        std::vector<uint32_t> sat(w1 * (static_cast<size_t>(dim_y) + 1u), 0u);
        for(uint32_t y = 0; y < dim_y; ++y)
        {
            uint32_t run = 0;
            for(uint32_t x = 0; x < dim_x; ++x)
            {
                run += mask[static_cast<size_t>(y) * dim_x + x] == 0 ? 1u : 0u;
                sat[(y + 1u) * w1 + x + 1u] = sat[y * w1 + x + 1u] + run;
            }
        }
        paris_hip_defect_stats& st = plan->stats;
        plan->row_start.assign(static_cast<size_t>(dim_y) + 1u, 0u);
        plan->first_source.push_back(0u);
        for(uint32_t y = 0; y < dim_y; ++y)
        {
            plan->row_start[y] = static_cast<uint32_t>(plan->defect.size());
            for(uint32_t x = 0; x < dim_x; ++x)
            {
                if(mask[static_cast<size_t>(y) * dim_x + x] == 0)
                    continue;
                ++st.defects;
                int64_t r = 1;
                for(; r <= R; ++r)
                {
                    const uint32_t x0 = static_cast<uint32_t>(std::max<int64_t>(0, x - r)), x1 = static_cast<uint32_t>(std::min<int64_t>(dim_x, x + r + 1));
                    const uint32_t y0 = static_cast<uint32_t>(std::max<int64_t>(0, y - r)), y1 = static_cast<uint32_t>(std::min<int64_t>(dim_y, y + r + 1));
                    if(window_count(sat, w1, x0, y0, x1, y1) != 0u)
                        break;
                }
                if(r > R)
                {
                    ++st.unrepairable;
                    continue;
                }
                // every good pixel within distance r lies ON ring r (a nearer one would have ended the search earlier)
                const size_t begin = plan->source.size();
                double sum = 0.0;
                for(int64_t dy = -r; dy <= r; ++dy)
                {
                    const int64_t sy = y + dy;
                    if(sy < 0 || sy >= dim_y)
                        continue;
                    const int64_t step = (dy == -r || dy == r) ? 1 : 2 * r; // the ring's top and bottom rows whole, else its two ends
                    for(int64_t dx = -r; dx <= r; dx += step)
                    {
                        const int64_t sx = x + dx;
                        if(sx < 0 || sx >= dim_x || mask[static_cast<size_t>(sy) * dim_x + sx] != 0)
                            continue;
                        if(plan->source.size() >= std::numeric_limits<uint32_t>::max())
                            return PARIS_HIP_ERROR_UNSUPPORTED;
                        plan->source.push_back(static_cast<uint32_t>(sy * dim_x + sx));
                        sum += 1.0 / static_cast<double>(dx * dx + dy * dy);
                        st.reach_rows = std::max(st.reach_rows, static_cast<uint32_t>(dy < 0 ? -dy : dy));
                        st.reach_cols = std::max(st.reach_cols, static_cast<uint32_t>(dx < 0 ? -dx : dx));
                    }
                }
                for(size_t k = begin; k < plan->source.size(); ++k)
                {
                    const int64_t dx = static_cast<int64_t>(plan->source[k] % dim_x) - x, dy = static_cast<int64_t>(plan->source[k] / dim_x) - y;
                    plan->weight.push_back(static_cast<float>((1.0 / static_cast<double>(dx * dx + dy * dy)) / sum));
                }
                plan->defect.push_back(y * dim_x + x);
                plan->first_source.push_back(static_cast<uint32_t>(plan->source.size()));
            }
        }
        plan->row_start[dim_y] = static_cast<uint32_t>(plan->defect.size());
        st.sources = plan->source.size();
        const uint64_t n = plan->defect.size();
        st.device_bytes = n == 0 ? 0u : sizeof(uint32_t) * (2u * n + 1u + 2u * st.sources);
        *out = plan.release();
    }
    catch(const std::bad_alloc&)
    {
        return 2; // hipErrorOutOfMemory
    }
    return PARIS_HIP_SUCCESS;
}

extern "C" int paris_hip_defect_plan_destroy(paris_hip_defect_plan* plan)
{
    delete plan;
    return PARIS_HIP_SUCCESS;
}

extern "C" int paris_hip_defect_plan_stats(const paris_hip_defect_plan* plan, paris_hip_defect_stats* out)
{
    if(plan == nullptr || out == nullptr)
        return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    *out = plan->stats;
    return PARIS_HIP_SUCCESS;
}

extern "C" int paris_hip_defect_plan_copy(const paris_hip_defect_plan* plan, uint32_t* defect_index, uint32_t* first_source,
                                          uint32_t* source_index, float* weight)
{
    if(plan == nullptr)
        return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    if(defect_index != nullptr)
        std::copy(plan->defect.begin(), plan->defect.end(), defect_index);
    if(first_source != nullptr)
        std::copy(plan->first_source.begin(), plan->first_source.end(), first_source);
    if(source_index != nullptr)
        std::copy(plan->source.begin(), plan->source.end(), source_index);
    if(weight != nullptr)
        std::copy(plan->weight.begin(), plan->weight.end(), weight);
    return PARIS_HIP_SUCCESS;
}
