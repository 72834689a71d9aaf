// Detector lag correction on the host (the statement is in include/paris_hip.h). Plain host code: it needs no
// device and no ctx. The check and the coefficients have their only implementation here -- the device path (lag.hip) calls them --
// and the pixel rule is restated for dense host frames in the order the statement fixes; lag_kernel implements the same definition.
#include <cmath>
#include <cstdint>

#include "paris_hip_internal.h"

namespace
{
    // b_0 = 1 - sum_n b_n / (1 - exp(-a_n)) in double, terms in ascending n (the model's b_n and a_n have been checked)
    double lag_b0(const paris_hip_lag_model& m)
    {
        double sum = 0.0;
        for(uint32_t n = 0; n < m.terms; ++n)
            sum += static_cast<double>(m.b[n]) / (1.0 - std::exp(-static_cast<double>(m.a[n])));
        return 1.0 - sum;
    }
}

extern "C" int paris_hip_lag_model_check(const paris_hip_lag_model* m)
{
    if(m == nullptr || m->terms < 1u || m->terms > PARIS_HIP_LAG_TERMS_MAX)
        return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    if(m->start != PARIS_HIP_LAG_START_REST && m->start != PARIS_HIP_LAG_START_STEADY)
        return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    for(uint32_t n = 0; n < m->terms; ++n)
        if(!std::isfinite(m->b[n]) || !std::isfinite(m->a[n]) || !(m->b[n] > 0.f) || !(m->a[n] > 0.f))
            return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    return lag_b0(*m) > 0.0 ? PARIS_HIP_SUCCESS : PARIS_HIP_ERROR_INVALID_ARGUMENT; // (NaN fails too)
}

extern "C" int paris_hip_lag_coefficients(const paris_hip_lag_model* m, float g[4], float c[4], float w[4], float* inv_b, double* b0)
{
    if(int rc = paris_hip_lag_model_check(m))
        return rc;
    if(g == nullptr || c == nullptr || w == nullptr)
        return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    const double first = lag_b0(*m);
    double big_b = first;
    for(uint32_t n = 0; n < m->terms; ++n)
        big_b += static_cast<double>(m->b[n]);
    for(uint32_t n = 0; n < PARIS_HIP_LAG_TERMS_MAX; ++n)
    {
        g[n] = c[n] = w[n] = 0.f;
        if(n >= m->terms)
            continue;
        const double gn = std::exp(-static_cast<double>(m->a[n]));
        g[n] = static_cast<float>(gn);
        c[n] = static_cast<float>(static_cast<double>(m->b[n]) * gn / big_b);
        w[n] = static_cast<float>(1.0 / (1.0 - gn));
    }
    if(inv_b != nullptr)
        *inv_b = static_cast<float>(1.0 / big_b);
    if(b0 != nullptr)
        *b0 = first;
    return PARIS_HIP_SUCCESS;
}

extern "C" int paris_hip_lag_correct_host(const paris_hip_lag_model* m, const float* dark, float* frames, float* state, int* started,
                                          uint64_t n_pixels, uint32_t n_frames)
{
    float g[4], c[4], w[4], inv_b = 0.f;
    if(int rc = paris_hip_lag_coefficients(m, g, c, w, &inv_b, nullptr))
        return rc;
    if(n_pixels == 0u || n_frames == 0u)
        return PARIS_HIP_SUCCESS;
    if(frames == nullptr || state == nullptr || started == nullptr)
        return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    const uint32_t terms = m->terms;
    for(uint32_t f = 0; f < n_frames; ++f)
    {
        const bool first = *started == 0;
        float* frame = frames + static_cast<uint64_t>(f) * n_pixels;
        for(uint64_t k = 0; k < n_pixels; ++k)
        {
            const float d = dark != nullptr ? dark[k] : 0.f;
            const float y = frame[k] - d;
            const bool finite = std::isfinite(y);
            float s[4] = {0.f, 0.f, 0.f, 0.f};
            for(uint32_t n = 0; n < terms; ++n)
            {
                if(!first)
                    s[n] = state[static_cast<uint64_t>(n) * n_pixels + k];
                else if(finite && m->start == PARIS_HIP_LAG_START_STEADY)
                    s[n] = w[n] * y;
            }
            float x = 0.f;
            if(finite)
            {
                float acc = y * inv_b;
                for(uint32_t n = 0; n < terms; ++n)
                    acc = std::fmaf(-c[n], s[n], acc);
                x = acc;
                frame[k] = x + d;
            }
            for(uint32_t n = 0; n < terms; ++n)
                state[static_cast<uint64_t>(n) * n_pixels + k] = std::fmaf(g[n], s[n], x);
        }
        *started = 1;
    }
    return PARIS_HIP_SUCCESS;
}
