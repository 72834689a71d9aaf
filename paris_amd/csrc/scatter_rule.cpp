// Scatter kernel superposition on the host (the statement is in include/paris_hip.h). Plain host code: it
// needs no device and no ctx. The default margin and the check have their only implementation here; the four Gaussian tables are made
// here for the device as well (scatter.hip uploads them). paris_hip_scatter_correction_host is the rule in double with a radix-2
// transform of its own: the C statement of the model, which the device meets within FFT rounding -- not a mirror of its bits.
#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdint>
#include <vector>

#include "paris_hip_internal.h"

namespace
{
    bool positive(double v)
    {
        return std::isfinite(v) && v > 0.0;
    }

    using cplx = std::complex<double>;

    // in place, natural order in and out: bit reversal, then decimation in time with exp(sign 2 pi i k / n) from one table
    void fft(cplx* x, uint32_t n, size_t stride, const std::vector<cplx>& w, bool inverse)
    {
        for(uint32_t i = 1, j = 0; i < n; ++i)
        {
            uint32_t bit = n >> 1;
            for(; j & bit; bit >>= 1)
                j ^= bit;
            j ^= bit;
            if(i < j)
                std::swap(x[i * stride], x[j * stride]);
        }
        for(uint32_t half = 1; half < n; half *= 2u)
        {
            const uint32_t step = n / (2u * half);
            for(uint32_t base = 0; base < n; base += 2u * half)
                for(uint32_t k = 0; k < half; ++k)
                {
                    const cplx t = (inverse ? std::conj(w[k * step]) : w[k * step]) * x[(base + k + half) * stride];
                    const cplx a = x[(base + k) * stride];
                    x[(base + k) * stride] = a + t;
                    x[(base + k + half) * stride] = a - t;
                }
        }
    }

    std::vector<cplx> twiddles(uint32_t n)
    {
        std::vector<cplx> w(n / 2u);
        for(uint32_t k = 0; k < n / 2u; ++k)
        {
            const double a = -2.0 * M_PI * static_cast<double>(k) / static_cast<double>(n);
            w[k] = cplx(std::cos(a), std::sin(a));
        }
        return w;
    }

    // weight exp(-2 pi^2 sigma^2 f^2) in double, rounded once
    void gaussian(double weight, float sigma, uint32_t n, float pitch, float* g)
    {
        for(uint32_t k = 0; k < n; ++k)
        {
            const double kk = k <= n / 2u ? static_cast<double>(k) : static_cast<double>(k) - static_cast<double>(n);
            const double f = kk / (static_cast<double>(n) * static_cast<double>(pitch));
            g[k] = static_cast<float>(weight * std::exp(-2.0 * M_PI * M_PI * static_cast<double>(sigma) * static_cast<double>(sigma) * f * f));
        }
    }
}

#pragma GCC visibility push(hidden)
// the four tables of G = g1x g1y + g2x g2y (scatter.hip uploads these): the x tables carry the weights 1 / (1 + w2) and w2 / (1 + w2)
void paris_hip_scatter_tables(const paris_hip_scatter_correction* s, uint32_t n_x, uint32_t n_y, float l_x, float l_y, float* g1x, float* g2x,
                              float* g1y, float* g2y)
{
    const double w2 = static_cast<double>(s->weight2);
    gaussian(1.0 / (1.0 + w2), s->sigma1_mm, n_x, l_x, g1x);
    gaussian(w2 / (1.0 + w2), s->sigma2_mm, n_x, l_x, g2x);
    gaussian(1.0, s->sigma1_mm, n_y, l_y, g1y);
    gaussian(1.0, s->sigma2_mm, n_y, l_y, g2y);
}
#pragma GCC visibility pop

extern "C" uint32_t paris_hip_scatter_default_margin(float sigma1_mm, float sigma2_mm, float l_x, float l_y)
{
    if(!positive(sigma1_mm) || !positive(sigma2_mm) || !positive(l_x) || !positive(l_y))
        return 0u;
    const double px = 3.0 * static_cast<double>(std::max(sigma1_mm, sigma2_mm)) / static_cast<double>(std::min(l_x, l_y));
    return static_cast<uint32_t>(std::min<double>(PARIS_HIP_PHASE_MARGIN_MAX, std::max(8.0, std::ceil(px))));
}

extern "C" int paris_hip_scatter_correction_check(const paris_hip_scatter_correction* s, uint32_t dim_x, uint32_t dim_y, float l_x, float l_y,
                                                  uint32_t* n_x, uint32_t* n_y, size_t* scratch_bytes)
{
    if(s == nullptr || !positive(s->amplitude) || !(s->alpha >= -2.f && s->alpha <= 2.f) || !(s->beta >= 0.f && s->beta <= 4.f)
       || !positive(s->sigma1_mm) || !positive(s->sigma2_mm) || !(std::isfinite(s->weight2) && s->weight2 >= 0.f)
       || !(s->limit > 0.f && s->limit < 1.f) || s->iterations < 1u || s->iterations > PARIS_HIP_SCATTER_ITERATIONS_MAX)
        return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    // the padded sizes, the size limit and the scratch are the phase filter's: its check with a setting that differs in nothing but
    // the margin gives them, and refuses margin, dimensions and pitches as it does there
    const paris_hip_phase_retrieval as_phase{1.f, 1.f, s->margin};
    return paris_hip_phase_retrieval_check(&as_phase, dim_x, dim_y, l_x, l_y, n_x, n_y, scratch_bytes);
}

extern "C" int paris_hip_scatter_correction_host(const paris_hip_scatter_correction* s, float l_x, float l_y, const float* src, float* dst,
                                                 uint32_t dim_x, uint32_t dim_y)
{
    uint32_t nx = 0, ny = 0;
    if(int rc = paris_hip_scatter_correction_check(s, dim_x, dim_y, l_x, l_y, &nx, &ny, nullptr))
        return rc;
    if(src == nullptr || dst == nullptr)
        return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    // step 1: the measured transmission of the pixels that enter; the others are air
    const size_t pixels = static_cast<size_t>(dim_x) * dim_y;
    std::vector<uint8_t> kept(pixels);
    std::vector<double> tm(pixels), t(pixels);
    for(size_t i = 0; i < pixels; ++i)
    {
        const float p = src[i], t32 = std::exp(-p); // (the fp32 expf: what the rule judges the pixel on)
        kept[i] = !(std::isfinite(p) && t32 > 0.f && std::isfinite(t32));
        t[i] = tm[i] = kept[i] ? 1.0 : std::exp(-static_cast<double>(p));
    }
    const std::vector<cplx> wx = twiddles(nx), wy = twiddles(ny);
    std::vector<float> g1x(nx), g2x(nx), g1y(ny), g2y(ny);
    paris_hip_scatter_tables(s, nx, ny, l_x, l_y, g1x.data(), g2x.data(), g1y.data(), g2y.data());
    const double amplitude = s->amplitude, alpha = s->alpha, beta = s->beta, keep = 1.0 - static_cast<double>(s->limit);
    const double scale = 1.0 / (static_cast<double>(nx) * static_cast<double>(ny));
    std::vector<double> q(pixels);
    std::vector<cplx> z(static_cast<size_t>(nx) * ny);
    // step 2
    for(uint32_t k = 0; k < s->iterations; ++k)
    {
        for(size_t i = 0; i < pixels; ++i)
        {
            const double ln_t = std::log(t[i]), path = -ln_t;
            q[i] = path > 0.0 ? amplitude * std::exp(alpha * ln_t + beta * std::log(path)) : 0.0;
        }
        for(uint32_t y = 0; y < ny; ++y)
        {
            const size_t row = static_cast<size_t>(paris_hip_phase_source(y, dim_y, ny)) * dim_x;
            for(uint32_t x = 0; x < nx; ++x)
                z[static_cast<size_t>(y) * nx + x] = q[row + paris_hip_phase_source(x, dim_x, nx)];
        }
        for(uint32_t y = 0; y < ny; ++y)
            fft(z.data() + static_cast<size_t>(y) * nx, nx, 1u, wx, false);
        for(uint32_t x = 0; x < nx; ++x)
        {
            fft(z.data() + x, ny, nx, wy, false);
            for(uint32_t y = 0; y < ny; ++y)
                z[static_cast<size_t>(y) * nx + x] *= static_cast<double>(g1x[x]) * static_cast<double>(g1y[y])
                                                      + static_cast<double>(g2x[x]) * static_cast<double>(g2y[y]);
            fft(z.data() + x, ny, nx, wy, true);
        }
        for(uint32_t y = 0; y < dim_y; ++y) // (only the rows that are stored)
        {
            cplx* row = z.data() + static_cast<size_t>(y) * nx;
            fft(row, nx, 1u, wx, true);
            for(uint32_t x = 0; x < dim_x; ++x)
            {
                const size_t i = static_cast<size_t>(y) * dim_x + x;
                t[i] = std::max(tm[i] - row[x].real() * scale, keep * tm[i]);
            }
        }
    }
    // step 3
    for(size_t i = 0; i < pixels; ++i)
        dst[i] = kept[i] ? src[i] : static_cast<float>(-std::log(t[i]));
    return PARIS_HIP_SUCCESS;
}
