// The 2-D transform of whole frames in LDS, shared by the passes that filter a frame in two dimensions (phase.hip, scatter.hip;
// DESIGN.md sections 4.22 and 4.23). Radix 2, decimation in frequency forward and in time inverse as in filter.hip -- nothing is
// ever reordered. A client packs rows 2r and 2r + 1 of a frame as one complex row a + ib, transforms it (fft_dif), splits it into
// the two Hermitian half-spectra (split_store), which go to the scratch as rows 2r and 2r + 1 of N_x / 2 + 1 columns; the column
// pass (frame_fft2_columns_kernel) transforms every column, multiplies by the client's transfer function and transforms back; the
// client merges the half-spectra of a row pair (merge_load) and transforms back (fft_dit_inverse).
//   Scratch layout: column j < N_x / 2 holds k_x = the bit reversal of j in log2 N_x - 1 bits (the even positions of the
//   transform's output, in order), column N_x / 2 holds the Nyquist bin: contiguous stores. Only the dim_y rows that exist are
//   transformed; the column pass reads the N_y padded rows through the row map.
//   A transfer functor has `float operator()(uint32_t k_x, uint32_t k_y) const`, real and even in both axes, k in natural order.
// Kernels and device functions are templates or inline: every client's translation unit gets its own.
#ifndef PARIS_HIP_FRAME_FFT2_H_
#define PARIS_HIP_FRAME_FFT2_H_

#include <algorithm>
#include <cmath>
#include <vector>

#include "frame_pass.h"

namespace frame_fft2
{
    constexpr uint32_t MAX_THREADS = 1024u;
    constexpr uint32_t COLUMNS_MAX = 16u;              // columns per workgroup of the column pass
    constexpr uint32_t COLUMN_SAMPLES = 8192u;         // ... and samples: 64 KiB, two workgroups to a CU's 160 KiB (measured
                                                       // against 16384: the column pass 18 % faster)
    constexpr size_t COLUMN_LDS_MAX = (COLUMN_SAMPLES + COLUMNS_MAX) * sizeof(float2);
    constexpr size_t ROW_LDS_MAX = PARIS_HIP_PHASE_SIZE_MAX * sizeof(float2);

    __device__ __forceinline__ float2 cmul(float2 a, float2 b)
    {
        return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
    }

    __device__ __forceinline__ uint32_t bit_reverse(uint32_t p, uint32_t bits)
    {
        return __brev(p) >> (32u - bits);
    }

    // `count` transforms of n = 2^log2n samples side by side in LDS, `stride` values apart; natural order in, bit-reversed order out
    __device__ __forceinline__ void fft_dif(float2* lds, uint32_t count, uint32_t stride, const float2* __restrict__ tw, uint32_t log2n,
                                            uint32_t tid, uint32_t nthreads)
    {
        const uint32_t nb = 1u << (log2n - 1u); // butterflies per transform and stage
        for(uint32_t lh = log2n - 1u;; --lh)
        {
            const uint32_t half = 1u << lh;
            for(uint32_t t = tid; t < count * nb; t += nthreads)
            {
                float2* x = lds + (t >> (log2n - 1u)) * stride;
                const uint32_t bf = t & (nb - 1u);
                const uint32_t pos = bf & (half - 1u);
                const uint32_t i = ((bf >> lh) << (lh + 1u)) + pos;
                const uint32_t j = i + half;
                const float2 w = tw[pos << (log2n - 1u - lh)];
                const float2 a = x[i];
                const float2 c = x[j];
                x[i] = make_float2(a.x + c.x, a.y + c.y);
                x[j] = cmul(make_float2(a.x - c.x, a.y - c.y), w);
            }
            __syncthreads();
            if(lh == 0u)
                break;
        }
    }

    // the unnormalised inverse: bit-reversed order in, natural order out
    __device__ __forceinline__ void fft_dit_inverse(float2* lds, uint32_t count, uint32_t stride, const float2* __restrict__ tw,
                                                    uint32_t log2n, uint32_t tid, uint32_t nthreads)
    {
        const uint32_t nb = 1u << (log2n - 1u);
        for(uint32_t lh = 0; lh < log2n; ++lh)
        {
            const uint32_t half = 1u << lh;
            for(uint32_t t = tid; t < count * nb; t += nthreads)
            {
                float2* x = lds + (t >> (log2n - 1u)) * stride;
                const uint32_t bf = t & (nb - 1u);
                const uint32_t pos = bf & (half - 1u);
                const uint32_t i = ((bf >> lh) << (lh + 1u)) + pos;
                const uint32_t j = i + half;
                float2 w = tw[pos << (log2n - 1u - lh)];
                w.y = -w.y;
                const float2 a = x[i];
                const float2 c = cmul(x[j], w);
                x[i] = make_float2(a.x + c.x, a.y + c.y);
                x[j] = make_float2(a.x - c.x, a.y - c.y);
            }
            __syncthreads();
        }
    }

    // the extension: which of the dim samples padded sample s reads
    __device__ __forceinline__ uint32_t source(uint32_t s, uint32_t dim, uint32_t n)
    {
        if(s < dim)
            return s;
        return s - dim < (n - dim + 1u) / 2u ? dim - 1u : 0u;
    }

    // fx holds the transform of a + ib (fft_dif's order): the Hermitian half-spectra of a and -- with has_b -- of b go to sa and sb,
    // w = n / 2 + 1 columns each. Z = A + iB: A[k] = (Z[k] + conj Z[n - k]) / 2, B[k] = (Z[k] - conj Z[n - k]) / 2i, k <= n / 2
    __device__ __forceinline__ void split_store(const float2* fx, float2* __restrict__ sa, float2* __restrict__ sb, bool has_b, uint32_t log2n,
                                                uint32_t tid, uint32_t nthreads)
    {
        const uint32_t n = 1u << log2n, w = n / 2u + 1u;
        for(uint32_t j = tid; j < w; j += nthreads)
        {
            const uint32_t pos = j < n / 2u ? 2u * j : 1u;
            const uint32_t k = bit_reverse(pos, log2n);
            const float2 zk = fx[pos], zm = fx[bit_reverse((n - k) & (n - 1u), log2n)];
            sa[j] = make_float2(0.5f * (zk.x + zm.x), 0.5f * (zk.y - zm.y));
            if(has_b)
                sb[j] = make_float2(0.5f * (zk.y + zm.y), 0.5f * (zm.x - zk.x));
        }
    }

    // the reverse, into fft_dit_inverse's order: Z'[k] = A'[k] + i B'[k] for k <= n / 2, conj A'[n - k] + i conj B'[n - k] above -- the
    // transfer function is even in k_x, so both stay Hermitian. No barrier behind it.
    __device__ __forceinline__ void merge_load(float2* fx, const float2* __restrict__ sa, const float2* __restrict__ sb, bool has_b, uint32_t log2n,
                                               uint32_t tid, uint32_t nthreads)
    {
        const uint32_t n = 1u << log2n;
        for(uint32_t pos = tid; pos < n; pos += nthreads)
        {
            const uint32_t k = bit_reverse(pos, log2n);
            const bool upper = k > n / 2u;
            const uint32_t kk = upper ? n - k : k;
            const uint32_t j = kk == n / 2u ? n / 2u : bit_reverse(kk, log2n) >> 1u;
            const float2 a = sa[j], b = has_b ? sb[j] : make_float2(0.f, 0.f);
            fx[pos] = upper ? make_float2(a.x + b.y, b.x - a.y) : make_float2(a.x - b.y, a.y + b.x);
        }
    }

    // One workgroup per set of C = 2^log2c adjacent columns: reads the N_y padded rows through the row map, transforms each column,
    // multiplies by the transfer function indexed through the bit-reversed k_y and the column's k_x, transforms back and stores rows
    // 0 .. dim_y - 1 where it read them. In LDS a column is N_y + 1 complex values long: the transposing load and store walk the
    // columns, and a power-of-two stride would put them all on one bank.
    // grid: (sets of 2^log2c columns, frames of this round); w = N_x / 2 + 1 columns, dim_y rows stored
    template <class Transfer>
    __global__ void __launch_bounds__(MAX_THREADS)
        frame_fft2_columns_kernel(float2* __restrict__ scratch, size_t scratch_frame, uint32_t dim_y, uint32_t w, uint32_t log2nx, uint32_t log2ny,
                                  uint32_t log2c, const float2* __restrict__ tw, const Transfer transfer)
    {
        extern __shared__ __attribute__((aligned(16))) float2 fx[];
        const uint32_t ny = 1u << log2ny, cols = 1u << log2c, stride = ny + 1u;
        const uint32_t tid = threadIdx.x, nthreads = blockDim.x;
        const uint32_t j0 = blockIdx.x << log2c;
        float2* sf = scratch + static_cast<size_t>(blockIdx.y) * scratch_frame;
        for(uint32_t t = tid; t < cols * ny; t += nthreads)
        {
            const uint32_t c = t & (cols - 1u), y = t >> log2c, j = j0 + c;
            fx[c * stride + y] = j < w ? sf[static_cast<size_t>(source(y, dim_y, ny)) * w + j] : make_float2(0.f, 0.f);
        }
        __syncthreads();
        fft_dif(fx, cols, stride, tw, log2ny, tid, nthreads);
        for(uint32_t t = tid; t < cols * ny; t += nthreads)
        {
            const uint32_t c = t >> log2ny, pos = t & (ny - 1u), j = j0 + c;
            if(j < w)
            {
                const uint32_t kx = j < w - 1u ? bit_reverse(j, log2nx - 1u) : w - 1u;
                const float h = transfer(kx, bit_reverse(pos, log2ny));
                float2 v = fx[c * stride + pos];
                v.x *= h;
                v.y *= h;
                fx[c * stride + pos] = v;
            }
        }
        __syncthreads();
        fft_dit_inverse(fx, cols, stride, tw, log2ny, tid, nthreads);
        for(uint32_t t = tid; t < cols * dim_y; t += nthreads)
        {
            const uint32_t c = t & (cols - 1u), y = t >> log2c, j = j0 + c;
            if(j < w)
                sf[static_cast<size_t>(y) * w + j] = fx[c * stride + y];
        }
    }

    inline uint32_t log2_of(uint32_t n) // n is a power of two
    {
        uint32_t l = 0;
        while((1u << l) < n)
            ++l;
        return l;
    }

    inline uint32_t threads_for(uint32_t butterflies)
    {
        return std::min(MAX_THREADS, std::max(64u, butterflies / 2u));
    }

    inline std::vector<float2> twiddles(uint32_t n) // exp(-2 pi i k / n), k < n / 2, rounded from double
    {
        std::vector<float2> w(n / 2u);
        for(uint32_t k = 0; k < n / 2u; ++k)
        {
            const double a = -2.0 * M_PI * static_cast<double>(k) / static_cast<double>(n);
            w[k] = make_float2(static_cast<float>(std::cos(a)), static_cast<float>(std::sin(a)));
        }
        return w;
    }

    // how one round of launches covers a setting's frames: the sizes both clients derive from (dim_y, N_x, N_y)
    struct plan
    {
        uint32_t w, log2nx, log2ny, cols, log2c, pairs, sets, row_threads, col_threads;
        size_t scratch_frame, row_lds, col_lds;
        float scale; // 1 / (N_x N_y), a power of two: exact

        plan(uint32_t dim_y, uint32_t n_x, uint32_t n_y)
            : w(n_x / 2u + 1u), log2nx(log2_of(n_x)), log2ny(log2_of(n_y)), cols(std::min(COLUMNS_MAX, COLUMN_SAMPLES / n_y)), log2c(log2_of(cols)),
              pairs((dim_y + 1u) / 2u), sets((w + cols - 1u) / cols), row_threads(threads_for(n_x / 2u)), col_threads(threads_for(cols * (n_y / 2u))),
              scratch_frame(static_cast<size_t>(dim_y) * w), row_lds(n_x * sizeof(float2)), col_lds(static_cast<size_t>(cols) * (n_y + 1u) * sizeof(float2)),
              scale(1.f / (static_cast<float>(n_x) * static_cast<float>(n_y)))
        {
        }
    };
}

#endif
