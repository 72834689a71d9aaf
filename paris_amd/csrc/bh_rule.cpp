// Beam-hardening correction on the host (the statement is in include/paris_hip.h). Plain host code: it needs no
// device and no ctx. The check, the Otsu threshold and the solver have their only implementation here; the pixel rule and the Gram
// sum are restated for dense host arrays, in the order the statement fixes, and the device (beam_hardening.hip) implements the same
// definitions.
#include <cmath>
#include <cstdint>
#include <vector>

#include "paris_hip_internal.h"

extern "C" int paris_hip_beam_hardening_check(const paris_hip_beam_hardening* bh)
{
    if(bh == nullptr || bh->degree < 1u || bh->degree > PARIS_HIP_BH_DEGREE_MAX)
        return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    for(uint32_t k = 0; k < bh->degree; ++k)
        if(!std::isfinite(bh->c[k]))
            return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    return PARIS_HIP_SUCCESS;
}

extern "C" int paris_hip_beam_hardening_host(const paris_hip_beam_hardening* bh, const float* src, float* dst, uint64_t n)
{
    if(int rc = paris_hip_beam_hardening_check(bh))
        return rc;
    if(n != 0u && (src == nullptr || dst == nullptr))
        return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    for(uint64_t i = 0; i < n; ++i)
    {
        const float p = src[i];
        if(p < 0.f) // noise in air: the linear term only
        {
            dst[i] = bh->c[0] * p;
            continue;
        }
        float acc = bh->c[bh->degree - 1u];
        for(uint32_t k = bh->degree - 1u; k >= 1u; --k)
            acc = std::fmaf(acc, p, bh->c[k - 1u]);
        dst[i] = acc * p; // (one multiplication: contraction is off in this library)
    }
    return PARIS_HIP_SUCCESS;
}

extern "C" int paris_hip_bh_threshold_from_histogram(const uint64_t* hist, uint32_t n_bins, float h_lo, float h_hi, float* thr)
{
    if(hist == nullptr || thr == nullptr || n_bins == 0u)
        return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    const paris_hip_volume_window range{h_lo, h_hi, PARIS_HIP_VOXEL_U8}; // the range rules of the window check
    if(int rc = paris_hip_volume_window_check(&range))
        return rc;
    uint64_t total = 0, moment = 0; // sum of h_k, sum of k h_k
    for(uint32_t b = 0; b < n_bins; ++b)
    {
        total += hist[b];
        moment += static_cast<uint64_t>(b) * hist[b];
    }
    if(total == 0u)
        return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    const double t = static_cast<double>(total);
    uint32_t best = 0;
    double best_score = -1.0;
    uint64_t c = 0, s = 0;
    for(uint32_t b = 0; b < n_bins; ++b)
    {
        c += hist[b];
        s += static_cast<uint64_t>(b) * hist[b];
        double score = 0.0;
        if(c != 0u && c != total)
        {
            const double w0 = static_cast<double>(c) / t;
            const double mu0 = static_cast<double>(s) / static_cast<double>(c);
            const double mu1 = static_cast<double>(moment - s) / static_cast<double>(total - c);
            const double d = mu0 - mu1;
            score = (w0 * (1.0 - w0)) * (d * d);
        }
        if(score > best_score) // (strictly: the smallest bin among equals wins)
        {
            best_score = score;
            best = b;
        }
    }
    const double width = (static_cast<double>(h_hi) - static_cast<double>(h_lo)) / static_cast<double>(n_bins);
    *thr = static_cast<float>(static_cast<double>(h_lo) + (static_cast<double>(best) + 1.0) * width);
    return PARIS_HIP_SUCCESS;
}

extern "C" int paris_hip_bh_gram_host(const float* const* f, uint32_t degree, const uint8_t* labels, uint64_t n_voxels, double* gram,
                                      paris_hip_bh_counts* counts)
{
    if(f == nullptr || gram == nullptr || counts == nullptr || degree < 1u || degree > PARIS_HIP_BH_DEGREE_MAX || (n_voxels != 0u && labels == nullptr))
        return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    for(uint32_t k = 0; k < degree; ++k)
        if(n_voxels != 0u && f[k] == nullptr)
            return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    const uint32_t n = degree + 1u, terms = n * (n + 1u) / 2u;
    constexpr uint64_t L = PARIS_HIP_BH_PARTIALS;
    std::vector<double> acc(static_cast<size_t>(terms) * L, 0.0); // acc[t * L + l]
    paris_hip_bh_counts cnt{};
    for(uint64_t i = 0; i < n_voxels; ++i) // ascending i: ascending within every partial
    {
        const uint8_t label = labels[i];
        if(label != 1u && label != 2u)
        {
            ++cnt.n_ignored;
            continue;
        }
        double g[PARIS_HIP_BH_DEGREE_MAX + 1u];
        bool finite = true;
        for(uint32_t k = 0; k < degree; ++k)
        {
            finite = finite && std::isfinite(f[k][i]);
            g[k] = static_cast<double>(f[k][i]);
        }
        if(!finite)
        {
            ++cnt.n_not_finite;
            continue;
        }
        g[degree] = label == 2u ? 1.0 : 0.0;
        ++(label == 2u ? cnt.n_object : cnt.n_air);
        const uint64_t l = i % L;
        uint32_t t = 0;
        for(uint32_t a = 0; a < n; ++a)
            for(uint32_t b = a; b < n; ++b, ++t)
                acc[static_cast<size_t>(t) * L + l] += g[a] * g[b];
    }
    for(uint32_t t = 0; t < terms; ++t)
    {
        double total = 0.0;
        for(uint32_t j = 0; j < 256u; ++j)
        {
            double bj = 0.0;
            for(uint32_t m = 0; m < L / 256u; ++m)
                bj = m == 0u ? acc[static_cast<size_t>(t) * L + j] : bj + acc[static_cast<size_t>(t) * L + j + 256u * m];
            total = j == 0u ? bj : total + bj;
        }
        gram[t] = total;
    }
    *counts = cnt;
    return PARIS_HIP_SUCCESS;
}

extern "C" int paris_hip_bh_solve(const double* gram, uint32_t degree, const paris_hip_bh_counts* counts, uint64_t min_voxels, paris_hip_bh_fit* out)
{
    if(gram == nullptr || counts == nullptr || out == nullptr || degree < 1u || degree > PARIS_HIP_BH_DEGREE_MAX)
        return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    const uint64_t least = min_voxels != 0u ? min_voxels : PARIS_HIP_BH_MIN_VOXELS_DEFAULT;
    if(counts->n_object < least || counts->n_air < least)
        return PARIS_HIP_ERROR_BH_TOO_FEW_VOXELS;
    const uint32_t N = degree, n = degree + 1u;
    const auto G = [&](uint32_t a, uint32_t b) { // a <= b
        return gram[a * n - a * (a - 1u) / 2u + (b - a)];
    };
    const double n_object = static_cast<double>(counts->n_object);
    const double T = G(0, N) / n_object;
    if(!std::isfinite(T) || T == 0.0)
        return PARIS_HIP_ERROR_BH_NOT_FINITE;
    double A[PARIS_HIP_BH_DEGREE_MAX][PARIS_HIP_BH_DEGREE_MAX], gm[PARIS_HIP_BH_DEGREE_MAX], rhs[PARIS_HIP_BH_DEGREE_MAX];
    for(uint32_t i = 0; i < N; ++i)
    {
        for(uint32_t j = 0; j < N; ++j)
            A[i][j] = i <= j ? G(i, j) : G(j, i);
        gm[i] = G(i, N);
        rhs[i] = T * gm[i];
    }
    // A = R^T R, R upper triangular, row by row
    double R[PARIS_HIP_BH_DEGREE_MAX][PARIS_HIP_BH_DEGREE_MAX] = {};
    for(uint32_t i = 0; i < N; ++i)
    {
        double d = A[i][i];
        for(uint32_t k = 0; k < i; ++k)
            d -= R[k][i] * R[k][i];
        if(!(d > 0.0)) // (NaN included)
            return PARIS_HIP_ERROR_BH_NOT_POSITIVE;
        R[i][i] = std::sqrt(d);
        for(uint32_t j = i + 1u; j < N; ++j)
        {
            double s = A[i][j];
            for(uint32_t k = 0; k < i; ++k)
                s -= R[k][i] * R[k][j];
            R[i][j] = s / R[i][i];
        }
    }
    double y[PARIS_HIP_BH_DEGREE_MAX], x[PARIS_HIP_BH_DEGREE_MAX];
    for(uint32_t i = 0; i < N; ++i) // R^T y = rhs
    {
        double s = rhs[i];
        for(uint32_t k = 0; k < i; ++k)
            s -= R[k][i] * y[k];
        y[i] = s / R[i][i];
    }
    for(uint32_t i = N; i-- > 0u;) // R x = y
    {
        double s = y[i];
        for(uint32_t k = i + 1u; k < N; ++k)
            s -= R[i][k] * x[k];
        x[i] = s / R[i][i];
    }
    paris_hip_bh_fit fit{};
    fit.setting.degree = N;
    for(uint32_t i = 0; i < N; ++i)
    {
        fit.setting.c[i] = static_cast<float>(x[i]); // rounded once
        if(!std::isfinite(fit.setting.c[i]))
            return PARIS_HIP_ERROR_BH_NOT_FINITE;
    }
    const double voxels = n_object + static_cast<double>(counts->n_air);
    const auto residual = [&](const double* c) {
        double quad = 0.0, lin = 0.0;
        for(uint32_t i = 0; i < N; ++i)
        {
            double row = 0.0;
            for(uint32_t j = 0; j < N; ++j)
                row += A[i][j] * c[j];
            quad += c[i] * row;
            lin += c[i] * gm[i];
        }
        const double ss = quad - 2.0 * T * lin + T * T * n_object;
        return std::sqrt(std::fmax(0.0, ss) / voxels) / std::fabs(T);
    };
    double unit[PARIS_HIP_BH_DEGREE_MAX] = {1.0, 0.0, 0.0, 0.0}, solved[PARIS_HIP_BH_DEGREE_MAX] = {};
    for(uint32_t i = 0; i < N; ++i)
        solved[i] = static_cast<double>(fit.setting.c[i]);
    fit.level = T;
    fit.residual_before = residual(unit);
    fit.residual_after = residual(solved);
    *out = fit;
    return PARIS_HIP_SUCCESS;
}
