// The host side of the detector roll (the statement is in include/paris_hip.h). Plain host code: it needs
// no device and no ctx, and it is the only host implementation of the rule -- the check, the constants, the pixel, the source rows of
// a band -- and of the search's check, margins, mirror plan and estimate. The device (detector_roll.hip) resamples the frames and
// scores the candidates.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>

#include "paris_hip_internal.h"

namespace
{
    constexpr double ROLL_PI = 3.14159265358979323846;

    bool roll_geometry_valid(const paris_detector_geometry* g)
    {
        return g != nullptr && g->n_row >= 2u && g->n_col >= 2u && g->n_row <= (1u << 30) && g->n_col <= (1u << 30) && std::isfinite(g->l_px_row)
               && g->l_px_row > 0.f && std::isfinite(g->l_px_col) && g->l_px_col > 0.f && std::isfinite(g->delta_s) && std::isfinite(g->delta_t);
    }

    bool roll_angle_valid(float eta_deg)
    {
        return std::isfinite(eta_deg) && eta_deg != 0.f && std::fabs(eta_deg) <= 10.f;
    }

    // where output pixel (i, j) reads: its upper left tap and the two weights
    struct roll_tap
    {
        uint32_t i0, j0;
        float wx, wy;
    };

    roll_tap roll_tap_of(const paris_hip_roll_constants& k, uint32_t n_row, uint32_t n_col, uint32_t i, uint32_t j)
    {
        const float di = static_cast<float>(i) - k.cx, dj = static_cast<float>(j) - k.cy;
        float x = (k.a * di + k.b * dj) + k.cx, y = (k.c * di + k.d * dj) + k.cy;
        const float x_last = static_cast<float>(n_row - 1u), y_last = static_cast<float>(n_col - 1u);
        x = x < 0.f ? 0.f : x > x_last ? x_last : x; // (the constants are finite and the detector below 2^30: x and y are finite)
        y = y < 0.f ? 0.f : y > y_last ? y_last : y;
        roll_tap t{};
        t.i0 = static_cast<uint32_t>(std::min(static_cast<int32_t>(std::floor(x)), static_cast<int32_t>(n_row - 2u)));
        t.j0 = static_cast<uint32_t>(std::min(static_cast<int32_t>(std::floor(y)), static_cast<int32_t>(n_col - 2u)));
        t.wx = x - static_cast<float>(t.i0);
        t.wy = y - static_cast<float>(t.j0);
        return t;
    }

    bool roll_candidates_valid(const paris_hip_roll_search* s)
    {
        return s != nullptr && s->count >= 1u && s->count <= 256u && std::isfinite(s->lo_deg) && std::isfinite(s->step_deg) && s->step_deg > 0.f;
    }

    float roll_candidate(const paris_hip_roll_search& s, uint32_t k)
    {
        return static_cast<float>(static_cast<double>(s.lo_deg) + k * static_cast<double>(s.step_deg));
    }

    void roll_margins(const paris_hip_roll_search& s, const paris_detector_geometry& g, double* m_x, double* m_y)
    {
        double ex = 0.0, ey = 0.0;
        for(uint32_t k = 0; k < s.count; ++k)
        {
            const paris_hip_roll_constants c = paris_hip_roll_constants_of(roll_candidate(s, k), g);
            const double cx = c.cx, cy = c.cy;
            const double far_x = std::max(cx, static_cast<double>(g.n_row - 1u) - cx), far_y = std::max(cy, static_cast<double>(g.n_col - 1u) - cy);
            ex = std::max(ex, std::fabs(static_cast<double>(c.b)) * far_y + std::fabs(1.0 - static_cast<double>(c.a)) * far_x);
            ey = std::max(ey, std::fabs(static_cast<double>(c.c)) * far_x + std::fabs(1.0 - static_cast<double>(c.d)) * far_y);
        }
        *m_x = std::ceil(ex) + 1.0;
        *m_y = std::ceil(ey) + 1.0;
    }
}

paris_hip_roll_constants paris_hip_roll_constants_of(float eta_deg, const paris_detector_geometry& g)
{
    const double eta = static_cast<double>(eta_deg) * ROLL_PI / 180.0;
    const double rho = static_cast<double>(g.l_px_col) / static_cast<double>(g.l_px_row);
    paris_hip_roll_constants k{};
    k.a = static_cast<float>(std::cos(eta));
    k.b = static_cast<float>(-std::sin(eta) * rho);
    k.c = static_cast<float>(std::sin(eta) / rho);
    k.d = static_cast<float>(std::cos(eta));
    k.cx = static_cast<float>(g.n_row / 2.0 + static_cast<double>(g.delta_s) - 0.5);
    k.cy = static_cast<float>(g.n_col / 2.0 + static_cast<double>(g.delta_t) - 0.5);
    return k;
}

extern "C" int paris_hip_detector_roll_check(const paris_hip_detector_roll* s, const paris_detector_geometry* g)
{
    return s != nullptr && roll_angle_valid(s->eta_deg) && roll_geometry_valid(g) ? PARIS_HIP_SUCCESS : PARIS_HIP_ERROR_INVALID_ARGUMENT;
}

extern "C" int paris_hip_detector_roll_host(const paris_hip_detector_roll* s, const paris_detector_geometry* g, const float* src, float* dst)
{
    if(int rc = paris_hip_detector_roll_check(s, g))
        return rc;
    if(src == nullptr || dst == nullptr)
        return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    const paris_hip_roll_constants k = paris_hip_roll_constants_of(s->eta_deg, *g);
    const size_t n = g->n_row;
    for(uint32_t j = 0; j < g->n_col; ++j)
        for(uint32_t i = 0; i < g->n_row; ++i)
        {
            const roll_tap t = roll_tap_of(k, g->n_row, g->n_col, i, j);
            const float* p0 = src + t.j0 * n + t.i0;
            const float* p1 = p0 + n;
            const float top = p0[0] + t.wx * (p0[1] - p0[0]);
            const float bot = p1[0] + t.wx * (p1[1] - p1[0]);
            dst[j * n + i] = top + t.wy * (bot - top);
        }
    return PARIS_HIP_SUCCESS;
}

extern "C" int paris_hip_detector_roll_source_rows(const paris_hip_detector_roll* s, const paris_detector_geometry* g, uint32_t row_first,
                                                   uint32_t row_count, uint32_t* src_first, uint32_t* src_count)
{
    if(int rc = paris_hip_detector_roll_check(s, g))
        return rc;
    if(src_first == nullptr || src_count == nullptr || row_first > g->n_col || row_count > g->n_col - row_first)
        return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    if(row_count == 0u)
    {
        *src_first = std::min(row_first, g->n_col - 1u);
        *src_count = 0u;
        return PARIS_HIP_SUCCESS;
    }
    const paris_hip_roll_constants k = paris_hip_roll_constants_of(s->eta_deg, *g);
    uint32_t lo = std::numeric_limits<uint32_t>::max(), hi = 0u;
    for(const uint32_t i : {0u, g->n_row - 1u})
        for(const uint32_t j : {row_first, row_first + row_count - 1u})
        {
            const uint32_t j0 = roll_tap_of(k, g->n_row, g->n_col, i, j).j0;
            lo = std::min(lo, j0);
            hi = std::max(hi, j0);
        }
    *src_first = lo;
    *src_count = hi + 2u - lo;
    return PARIS_HIP_SUCCESS;
}

extern "C" int paris_hip_roll_search_check(const paris_hip_roll_search* s, const paris_detector_geometry* g, uint32_t* margin_x,
                                           uint32_t* margin_y, size_t* device_bytes)
{
    if(!roll_candidates_valid(s) || !roll_geometry_valid(g))
        return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    for(uint32_t k = 0; k < s->count; ++k)
    {
        const float eta = roll_candidate(*s, k);
        if(eta != 0.f && !roll_angle_valid(eta))
            return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    }
    double m_x = 0.0, m_y = 0.0;
    roll_margins(*s, *g, &m_x, &m_y);
    if(!(2.0 * m_x < static_cast<double>(g->n_row)) || !(2.0 * m_y < static_cast<double>(g->n_col)))
        return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    if(margin_x != nullptr)
        *margin_x = static_cast<uint32_t>(m_x);
    if(margin_y != nullptr)
        *margin_y = static_cast<uint32_t>(m_y);
    if(device_bytes != nullptr)
        *device_bytes = paris_hip_roll_layout_of(g->n_row, g->n_col, s->count).bytes;
    return PARIS_HIP_SUCCESS;
}

void paris_hip_roll_search_plan(const paris_hip_roll_search& s, const paris_detector_geometry& g, uint32_t* margin_x, uint32_t* margin_y,
                                paris_hip_roll_mirror* columns)
{
    double m_x = 0.0, m_y = 0.0;
    roll_margins(s, g, &m_x, &m_y);
    *margin_x = static_cast<uint32_t>(m_x);
    *margin_y = static_cast<uint32_t>(m_y);
    const double cx = g.n_row / 2.0 + static_cast<double>(g.delta_s) - 0.5, last = static_cast<double>(g.n_row - 1u) - m_x;
    for(uint32_t i = 0; i < g.n_row; ++i)
    {
        paris_hip_roll_mirror e{-1, 0.f};
        const double ip = 2.0 * cx - static_cast<double>(i), i0 = std::floor(ip);
        if(static_cast<double>(i) >= m_x && static_cast<double>(i) <= last && i0 >= m_x && i0 + 1.0 <= last)
        {
            e.i0 = static_cast<int32_t>(i0);
            e.w = static_cast<float>(ip - i0);
        }
        columns[i] = e;
    }
}

extern "C" int paris_hip_roll_estimate_from_costs(const paris_hip_roll_search* s, const double* cost, paris_hip_roll_result* result)
{
    if(!roll_candidates_valid(s) || cost == nullptr || result == nullptr)
        return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    paris_hip_cost_estimate e{};
    const int rc = paris_hip_estimate_from_costs(static_cast<double>(s->lo_deg), static_cast<double>(s->step_deg), s->count, cost, &e);
    paris_hip_roll_result r{};
    r.scored = e.scored;
    if(rc == PARIS_HIP_SUCCESS)
    {
        r.eta_deg = e.value;
        r.best = e.best;
        r.cost_min = e.cost_min;
        r.cost_median = e.cost_median;
        r.at_edge = e.at_edge;
    }
    *result = r;
    return rc;
}
