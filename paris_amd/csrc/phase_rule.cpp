// Single-distance phase retrieval on the host (the statement is in include/paris_hip.h). Plain host code: it
// needs no device and no ctx. alpha, the default margin and the check have their only implementation here; the tables a_x / a_y are
// made here for the device as well (phase.hip uploads them). paris_hip_phase_retrieval_host is the rule in double with a radix-2
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

    uint32_t padded(uint32_t dim, uint32_t margin) // the smallest power of two >= max(8, dim + 2 margin); dim <= 2^31, margin <= 1024
    {
        const uint64_t want = std::max<uint64_t>(8u, static_cast<uint64_t>(dim) + 2u * margin);
        uint64_t n = 8u;
        while(n < want)
            n *= 2u;
        return static_cast<uint32_t>(std::min<uint64_t>(n, 0x80000000ull));
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
}

#pragma GCC visibility push(hidden)
// a[k] = alpha f^2 in double, rounded once (phase.hip uploads these)
void paris_hip_phase_table(float alpha, uint32_t n, float pitch, float* a)
{
    for(uint32_t k = 0; k < n; ++k)
    {
        const double kk = k <= n / 2u ? static_cast<double>(k) : static_cast<double>(k) - static_cast<double>(n);
        const double f = kk / (static_cast<double>(n) * static_cast<double>(pitch));
        a[k] = static_cast<float>(static_cast<double>(alpha) * f * f);
    }
}
// the extension's map: which of the dim source samples padded sample s reads
uint32_t paris_hip_phase_source(uint32_t s, uint32_t dim, uint32_t n)
{
    if(s < dim)
        return s;
    return s - dim < (n - dim + 1u) / 2u ? dim - 1u : 0u;
}
#pragma GCC visibility pop

extern "C" int paris_hip_phase_alpha(const paris_detector_geometry* det_geo, double delta_over_beta, double energy_kev, float* alpha_mm2)
{
    if(det_geo == nullptr || alpha_mm2 == nullptr || !positive(delta_over_beta) || !positive(energy_kev))
        return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    const double d_so = std::fabs(static_cast<double>(det_geo->d_so)), d_od = std::fabs(static_cast<double>(det_geo->d_od));
    if(!positive(d_so) || !positive(d_od))
        return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    const double lambda = 1.2398419843e-6 / energy_kev; // mm
    const float alpha = static_cast<float>(M_PI * lambda * delta_over_beta * d_od * (d_so + d_od) / d_so);
    if(!positive(alpha))
        return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    *alpha_mm2 = alpha;
    return PARIS_HIP_SUCCESS;
}

extern "C" uint32_t paris_hip_phase_default_margin(float alpha_mm2, float l_x, float l_y)
{
    if(!positive(alpha_mm2) || !positive(l_x) || !positive(l_y))
        return 0u;
    const double px = 6.0 * std::sqrt(static_cast<double>(alpha_mm2)) / (2.0 * M_PI * static_cast<double>(std::min(l_x, l_y)));
    return static_cast<uint32_t>(std::min<double>(PARIS_HIP_PHASE_MARGIN_MAX, std::max(8.0, std::ceil(px))));
}

extern "C" int paris_hip_phase_retrieval_check(const paris_hip_phase_retrieval* s, uint32_t dim_x, uint32_t dim_y, float l_x, float l_y,
                                               uint32_t* n_x, uint32_t* n_y, size_t* scratch_bytes)
{
    if(s == nullptr || !positive(s->alpha_mm2) || !(s->t_min > 0.f && s->t_min <= 1.f) || s->margin < 1u || s->margin > PARIS_HIP_PHASE_MARGIN_MAX
       || dim_x == 0u || dim_y == 0u || dim_x > 0x7fffffffu || dim_y > 0x7fffffffu || !positive(l_x) || !positive(l_y))
        return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    const uint32_t nx = padded(dim_x, s->margin), ny = padded(dim_y, s->margin);
    if(n_x != nullptr)
        *n_x = nx;
    if(n_y != nullptr)
        *n_y = ny;
    if(nx > PARIS_HIP_PHASE_SIZE_MAX || ny > PARIS_HIP_PHASE_SIZE_MAX)
        return PARIS_HIP_ERROR_UNSUPPORTED;
    if(scratch_bytes != nullptr)
    {
        const size_t frame = static_cast<size_t>(dim_y) * (nx / 2u + 1u) * 2u * sizeof(float);
        const size_t frames = std::max<size_t>(1u, std::min<size_t>(16u, (size_t{64u} << 20) / frame));
        *scratch_bytes = frames * frame;
    }
    return PARIS_HIP_SUCCESS;
}

extern "C" int paris_hip_phase_retrieval_host(const paris_hip_phase_retrieval* s, float l_x, float l_y, const float* src, float* dst,
                                              uint32_t dim_x, uint32_t dim_y)
{
    uint32_t nx = 0, ny = 0;
    if(int rc = paris_hip_phase_retrieval_check(s, dim_x, dim_y, l_x, l_y, &nx, &ny, nullptr))
        return rc;
    if(src == nullptr || dst == nullptr)
        return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    // steps 1 and 3: the transmission of the dim_x x dim_y pixels, then the extension
    std::vector<uint8_t> kept(static_cast<size_t>(dim_x) * dim_y);
    std::vector<double> t(kept.size());
    for(size_t i = 0; i < kept.size(); ++i)
    {
        const float p = src[i];
        kept[i] = !std::isfinite(p) || !std::isfinite(std::exp(-p)); // (the fp32 expf: what the rule judges the pixel on)
        t[i] = kept[i] ? 1.0 : std::exp(-static_cast<double>(p));
    }
    std::vector<cplx> z(static_cast<size_t>(nx) * ny);
    for(uint32_t y = 0; y < ny; ++y)
    {
        const size_t row = static_cast<size_t>(paris_hip_phase_source(y, dim_y, ny)) * dim_x;
        for(uint32_t x = 0; x < nx; ++x)
            z[static_cast<size_t>(y) * nx + x] = t[row + paris_hip_phase_source(x, dim_x, nx)];
    }
    // step 4
    const std::vector<cplx> wx = twiddles(nx), wy = twiddles(ny);
    std::vector<float> ax(nx), ay(ny);
    paris_hip_phase_table(s->alpha_mm2, nx, l_x, ax.data());
    paris_hip_phase_table(s->alpha_mm2, ny, l_y, ay.data());
    for(uint32_t y = 0; y < ny; ++y)
        fft(z.data() + static_cast<size_t>(y) * nx, nx, 1u, wx, false);
    for(uint32_t x = 0; x < nx; ++x)
    {
        fft(z.data() + x, ny, nx, wy, false);
        for(uint32_t y = 0; y < ny; ++y)
            z[static_cast<size_t>(y) * nx + x] /= 1.0 + static_cast<double>(ax[x]) + static_cast<double>(ay[y]);
        fft(z.data() + x, ny, nx, wy, true);
    }
    // step 5, on the rows that are stored
    const double scale = 1.0 / (static_cast<double>(nx) * static_cast<double>(ny));
    for(uint32_t y = 0; y < dim_y; ++y)
    {
        cplx* row = z.data() + static_cast<size_t>(y) * nx;
        fft(row, nx, 1u, wx, true);
        for(uint32_t x = 0; x < dim_x; ++x)
        {
            const size_t i = static_cast<size_t>(y) * dim_x + x;
            dst[i] = kept[i] ? src[i] : static_cast<float>(-std::log(std::max(row[x].real() * scale, static_cast<double>(s->t_min))));
        }
    }
    return PARIS_HIP_SUCCESS;
}
