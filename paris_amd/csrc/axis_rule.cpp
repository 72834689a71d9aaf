// The host side of the axis search (the statement is in include/paris_hip.h). Plain host code: it needs no
// device and no ctx, and it is the only implementation of the three host rules -- the check with the band, the plan that says where
// every column's conjugate lies, and the estimate from the costs. The device (axis_search.hip) sums the band into the sinogram and
// scores the pairs the plan names.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>
#include <vector>

#include "paris_hip_internal.h"

namespace
{
    constexpr double AXIS_PI = 3.14159265358979323846;

    bool axis_candidates_valid(const paris_hip_axis_search* s)
    {
        return s != nullptr && s->count >= 1u && s->count <= 1024u && std::isfinite(s->lo) && std::isfinite(s->step) && s->step > 0.f;
    }

    double axis_candidate(const paris_hip_axis_search& s, uint32_t k)
    {
        return static_cast<double>(static_cast<float>(static_cast<double>(s.lo) + k * static_cast<double>(s.step)));
    }
}

extern "C" int paris_hip_axis_search_check(const paris_hip_axis_search* s, const paris_detector_geometry* g, uint32_t n_frames,
                                           uint32_t* row_first, size_t* device_bytes)
{
    if(g == nullptr || !axis_candidates_valid(s))
        return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    if(g->n_row == 0u || g->n_col == 0u || s->rows < 1u || s->rows > 64u || s->rows > g->n_col || n_frames < 4u)
        return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    const double d_sd = std::fabs(static_cast<double>(g->d_so)) + std::fabs(static_cast<double>(g->d_od));
    if(!std::isfinite(g->l_px_row) || !(g->l_px_row > 0.f) || !std::isfinite(d_sd) || !(d_sd > 0.0) || !std::isfinite(g->delta_t))
        return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    const uint64_t limit = std::numeric_limits<uint32_t>::max();
    if(static_cast<uint64_t>(g->n_row) * s->count > limit || static_cast<uint64_t>(g->n_row) * n_frames > limit
       || g->n_row > static_cast<uint32_t>(std::numeric_limits<int32_t>::max())) // (i0 is an int32)
        return PARIS_HIP_ERROR_UNSUPPORTED;
    if(row_first != nullptr)
    {
        const double j_c = g->n_col / 2.0 + static_cast<double>(g->delta_t) - 0.5;
        const double first = std::floor(j_c - (s->rows - 1u) / 2.0 + 0.5);
        *row_first = static_cast<uint32_t>(std::min(std::max(first, 0.0), static_cast<double>(g->n_col - s->rows)));
    }
    if(device_bytes != nullptr)
        *device_bytes = paris_hip_axis_layout_of(g->n_row, n_frames, s->count).bytes;
    return PARIS_HIP_SUCCESS;
}

extern "C" int paris_hip_axis_search_plan(const paris_hip_axis_search* s, const paris_detector_geometry* g, uint32_t n_frames, uint32_t k,
                                          paris_hip_axis_entry* entries)
{
    if(int rc = paris_hip_axis_search_check(s, g, n_frames, nullptr, nullptr))
        return rc;
    if(k >= s->count || entries == nullptr)
        return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    const uint32_t n = g->n_row;
    const double c = axis_candidate(*s, k), l = static_cast<double>(g->l_px_row), views = static_cast<double>(n_frames);
    const double d_sd = std::fabs(static_cast<double>(g->d_so)) + std::fabs(static_cast<double>(g->d_od));
    for(uint32_t i = 0; i < n; ++i)
    {
        paris_hip_axis_entry e{-1, 0u, 0.f, 0.f};
        const double ip = static_cast<double>(n - 1u - i) + 2.0 * c;
        const double i0 = std::floor(ip);
        if(i0 >= 0.0 && i0 + 1.0 <= static_cast<double>(n - 1u))
        {
            const double gamma = std::atan((((i + 0.5) - n / 2.0 - c) * l) / d_sd);
            const double kk = views / 2.0 + (gamma * views) / AXIS_PI;
            const double k_floor = std::floor(kk);
            double k0 = std::fmod(k_floor, views); // (|gamma| < pi / 2: kk lies in [0, N], and only rounding puts it on an end)
            if(k0 < 0.0)
                k0 += views;
            e.i0 = static_cast<int32_t>(i0);
            e.k0 = static_cast<uint32_t>(k0);
            e.wi = static_cast<float>(ip - i0);
            e.wf = static_cast<float>(kk - k_floor);
        }
        entries[i] = e;
    }
    return PARIS_HIP_SUCCESS;
}

int paris_hip_estimate_from_costs(double lo, double step, uint32_t count, const double* cost, paris_hip_cost_estimate* out)
{
    paris_hip_cost_estimate r{};
    std::vector<double> scored;
    uint32_t m = 0;
    for(uint32_t k = 0; k < count; ++k)
        if(std::isfinite(cost[k]))
        {
            if(scored.empty() || cost[k] < cost[m])
                m = k;
            scored.push_back(cost[k]);
        }
    r.scored = static_cast<uint32_t>(scored.size());
    if(scored.empty())
    {
        *out = r;
        return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    }
    std::nth_element(scored.begin(), scored.begin() + (scored.size() - 1u) / 2u, scored.end());
    r.cost_median = scored[(scored.size() - 1u) / 2u];
    r.best = m;
    r.cost_min = cost[m];
    const double c_m = static_cast<double>(static_cast<float>(lo + m * step));
    r.value = static_cast<float>(c_m);
    r.at_edge = 1u;
    if(m >= 1u && m + 1u < count && std::isfinite(cost[m - 1u]) && std::isfinite(cost[m + 1u]))
    {
        const double q = cost[m - 1u] - 2.0 * cost[m] + cost[m + 1u];
        if(q > 0.0)
        {
            const double off = std::min(std::max(0.5 * (cost[m - 1u] - cost[m + 1u]) / q, -0.5), 0.5);
            r.value = static_cast<float>(c_m + off * step);
            r.at_edge = 0u;
        }
    }
    *out = r;
    return PARIS_HIP_SUCCESS;
}

extern "C" int paris_hip_axis_estimate_from_costs(const paris_hip_axis_search* s, const double* cost, const uint32_t* columns,
                                                  paris_hip_axis_result* result)
{
    if(!axis_candidates_valid(s) || cost == nullptr || result == nullptr)
        return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    paris_hip_cost_estimate e{};
    const int rc = paris_hip_estimate_from_costs(static_cast<double>(s->lo), static_cast<double>(s->step), s->count, cost, &e);
    paris_hip_axis_result r{};
    r.scored = e.scored;
    if(rc == PARIS_HIP_SUCCESS)
    {
        r.cost_median = e.cost_median;
        r.best = e.best;
        r.cost_min = e.cost_min;
        r.columns = columns != nullptr ? columns[e.best] : 0u;
        r.delta_s = e.value;
        r.at_edge = e.at_edge;
    }
    *result = r;
    return rc;
}
