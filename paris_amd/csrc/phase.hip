// Single-distance phase retrieval (Paganin) for gfx950: the library's 2-D filter (the statement is in
// include/paris_hip.h, the host rule in phase_rule.cpp). Three launches per round of frames, every transform in LDS, radix 2,
// decimation in frequency forward and in time inverse as in filter.hip -- nothing is ever reordered:
//   phase_rows_forward_kernel   one workgroup per pair of detector rows: T = expf(-p) through the extension's column map, rows 2r and
//                               2r + 1 packed as a + ib, one transform of N_x, split into the two Hermitian half-spectra, which go to
//                               the scratch as rows 2r and 2r + 1 of N_x / 2 + 1 columns. Column j < N_x / 2 holds k_x = the bit
//                               reversal of j in log2 N_x - 1 bits (the even positions of the transform's output, in order), column
//                               N_x / 2 holds the Nyquist bin: contiguous stores. Only the dim_y rows that exist are transformed.
//   phase_columns_kernel        one workgroup per set of C adjacent columns: reads the N_y padded rows through the row map, transforms
//                               each column, multiplies by H indexed through the bit-reversed k_y and the column's k_x, transforms
//                               back and stores rows 0 .. dim_y - 1 where it read them. In LDS a column is N_y + 1 complex values
//                               long: the transposing load and store walk the columns, and a power-of-two stride would put them all
//                               on one bank.
//   phase_rows_inverse_kernel   merges the two half-spectra of a row pair, transforms back, scales by 1 / (N_x N_y) and stores
//                               -logf(fmaxf(T', t_min)) on the dim_x pixels that entered the filter.
// A frame is served by its own workgroups whatever else the call holds: its bits do not depend on the other frames of the call.
#include <algorithm>
#include <cmath>
#include <vector>

#include "frame_pass.h"

namespace
{
    constexpr uint32_t PHASE_MAX_THREADS = 1024u;
    constexpr uint32_t PHASE_COLUMNS_MAX = 16u;              // columns per workgroup of the column pass
    constexpr uint32_t PHASE_COLUMN_SAMPLES = 8192u;         // ... and samples: 64 KiB, two workgroups to a CU's 160 KiB (measured
                                                             // against 16384: the column pass 18 % faster)
    constexpr size_t PHASE_COLUMN_LDS_MAX = (PHASE_COLUMN_SAMPLES + PHASE_COLUMNS_MAX) * sizeof(float2);
    constexpr size_t PHASE_ROW_LDS_MAX = PARIS_HIP_PHASE_SIZE_MAX * sizeof(float2);

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

    // step 3: which of the dim samples padded sample s reads
    __device__ __forceinline__ uint32_t source(uint32_t s, uint32_t dim, uint32_t n)
    {
        if(s < dim)
            return s;
        return s - dim < (n - dim + 1u) / 2u ? dim - 1u : 0u;
    }

    // step 1: does the pixel enter the filter, and as what
    __device__ __forceinline__ bool enters(float p, float* t)
    {
        *t = expf(-p);
        return isfinite(p) && isfinite(*t);
    }
    __device__ __forceinline__ float transmission(float p)
    {
        float t;
        return enters(p, &t) ? t : 1.f;
    }

    // grid: (row pairs, frames of this round). p: row 0 of the round's first frame; scratch: its first frame's spectra, frames
    // scratch_frame complex values apart.
    __global__ void __launch_bounds__(PHASE_MAX_THREADS)
        phase_rows_forward_kernel(const char* __restrict__ p, size_t pitch, size_t frame_stride, uint32_t dim_x, uint32_t dim_y, uint32_t log2n,
                                  const float2* __restrict__ tw, float2* __restrict__ scratch, size_t scratch_frame)
    {
        extern __shared__ __attribute__((aligned(16))) float2 fx[];
        const uint32_t n = 1u << log2n, w = n / 2u + 1u;
        const uint32_t tid = threadIdx.x, nthreads = blockDim.x;
        const uint32_t row_a = 2u * blockIdx.x;
        const bool has_b = row_a + 1u < dim_y;
        const char* frame = p + static_cast<size_t>(blockIdx.y) * frame_stride;
        const float* pa = reinterpret_cast<const float*>(frame + static_cast<size_t>(row_a) * pitch);
        const float* pb = reinterpret_cast<const float*>(frame + static_cast<size_t>(row_a + 1u) * pitch);
        for(uint32_t s = tid; s < n; s += nthreads)
        {
            const uint32_t xs = source(s, dim_x, n);
            fx[s] = make_float2(transmission(pa[xs]), has_b ? transmission(pb[xs]) : 0.f);
        }
        __syncthreads();
        fft_dif(fx, 1u, 0u, tw, log2n, tid, nthreads);
        // Z = A + iB with A, B Hermitian: A[k] = (Z[k] + conj Z[n - k]) / 2, B[k] = (Z[k] - conj Z[n - k]) / 2i, k <= n / 2
        float2* sa = scratch + static_cast<size_t>(blockIdx.y) * scratch_frame + static_cast<size_t>(row_a) * w;
        float2* sb = sa + w;
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

    // grid: (sets of 2^log2c columns, frames of this round); w = N_x / 2 + 1 columns, dim_y rows stored
    __global__ void __launch_bounds__(PHASE_MAX_THREADS)
        phase_columns_kernel(float2* __restrict__ scratch, size_t scratch_frame, uint32_t dim_y, uint32_t w, uint32_t log2nx, uint32_t log2ny,
                             uint32_t log2c, const float2* __restrict__ tw, const float* __restrict__ ax, const float* __restrict__ ay)
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
                const float h = 1.f / ((1.f + ax[kx]) + ay[bit_reverse(pos, log2ny)]);
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

    __global__ void __launch_bounds__(PHASE_MAX_THREADS)
        phase_rows_inverse_kernel(char* __restrict__ p, size_t pitch, size_t frame_stride, uint32_t dim_x, uint32_t dim_y, uint32_t log2n,
                                  const float2* __restrict__ tw, const float2* __restrict__ scratch, size_t scratch_frame, float scale, float t_min)
    {
        extern __shared__ __attribute__((aligned(16))) float2 fx[];
        const uint32_t n = 1u << log2n, w = n / 2u + 1u;
        const uint32_t tid = threadIdx.x, nthreads = blockDim.x;
        const uint32_t row_a = 2u * blockIdx.x;
        const bool has_b = row_a + 1u < dim_y;
        const float2* sa = scratch + static_cast<size_t>(blockIdx.y) * scratch_frame + static_cast<size_t>(row_a) * w;
        const float2* sb = sa + w;
        // Z'[k] = A'[k] + i B'[k] for k <= n / 2, conj A'[n - k] + i conj B'[n - k] above: H is even in k_x, so both stay Hermitian
        for(uint32_t pos = tid; pos < n; pos += nthreads)
        {
            const uint32_t k = bit_reverse(pos, log2n);
            const bool upper = k > n / 2u;
            const uint32_t kk = upper ? n - k : k;
            const uint32_t j = kk == n / 2u ? n / 2u : bit_reverse(kk, log2n) >> 1u;
            const float2 a = sa[j], b = has_b ? sb[j] : make_float2(0.f, 0.f);
            fx[pos] = upper ? make_float2(a.x + b.y, b.x - a.y) : make_float2(a.x - b.y, a.y + b.x);
        }
        __syncthreads();
        fft_dit_inverse(fx, 1u, 0u, tw, log2n, tid, nthreads);
        char* frame = p + static_cast<size_t>(blockIdx.y) * frame_stride;
        float* pa = reinterpret_cast<float*>(frame + static_cast<size_t>(row_a) * pitch);
        float* pb = reinterpret_cast<float*>(frame + static_cast<size_t>(row_a + 1u) * pitch);
        for(uint32_t s = tid; s < dim_x; s += nthreads)
        {
            const float2 v = fx[s];
            float t;
            if(enters(pa[s], &t))
                pa[s] = -logf(fmaxf(v.x * scale, t_min));
            if(has_b && enters(pb[s], &t))
                pb[s] = -logf(fmaxf(v.y * scale, t_min));
        }
    }

    uint32_t log2_of(uint32_t n) // n is a power of two
    {
        uint32_t l = 0;
        while((1u << l) < n)
            ++l;
        return l;
    }

    uint32_t threads_for(uint32_t butterflies)
    {
        return std::min(PHASE_MAX_THREADS, std::max(64u, butterflies / 2u));
    }

    std::vector<float2> twiddles(uint32_t n) // exp(-2 pi i k / n), k < n / 2, rounded from double
    {
        std::vector<float2> w(n / 2u);
        for(uint32_t k = 0; k < n / 2u; ++k)
        {
            const double a = -2.0 * M_PI * static_cast<double>(k) / static_cast<double>(n);
            w[k] = make_float2(static_cast<float>(std::cos(a)), static_cast<float>(std::sin(a)));
        }
        return w;
    }
}

extern "C" int paris_hip_set_phase_retrieval(paris_hip_ctx* ctx, const paris_hip_phase_retrieval* setting, uint32_t dim_x, uint32_t dim_y,
                                             float l_x, float l_y)
{
    if(int rc = paris_hip_bind(ctx))
        return rc;
    uint32_t nx = 0, ny = 0;
    size_t scratch = 0;
    if(int rc = paris_hip_phase_retrieval_check(setting, dim_x, dim_y, l_x, l_y, &nx, &ny, &scratch))
        return rc;
    // the column pass asks for 64 KiB of dynamic LDS and the columns' padding (the attribute is per device)
    PARIS_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(phase_columns_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      PHASE_COLUMN_LDS_MAX));
    PARIS_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(phase_rows_forward_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      PHASE_ROW_LDS_MAX));
    PARIS_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(phase_rows_inverse_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      PHASE_ROW_LDS_MAX));
    const std::vector<float2> wx = twiddles(nx), wy = twiddles(ny);
    std::vector<float> ax(nx), ay(ny);
    paris_hip_phase_table(setting->alpha_mm2, nx, l_x, ax.data());
    paris_hip_phase_table(setting->alpha_mm2, ny, l_y, ay.data());
    const size_t wx_bytes = wx.size() * sizeof(float2), wy_bytes = wy.size() * sizeof(float2), ax_bytes = nx * sizeof(float),
                 ay_bytes = ny * sizeof(float);
    const size_t head = wx_bytes + wy_bytes + ax_bytes + ay_bytes; // (a multiple of 16: every length is a power of two >= 8)
    paris_hip_device_buffer mem;
    if(int rc = paris_hip_install(ctx, head + scratch,
                                  {{0u, wx.data(), wx_bytes},
                                   {wx_bytes, wy.data(), wy_bytes},
                                   {wx_bytes + wy_bytes, ax.data(), ax_bytes},
                                   {wx_bytes + wy_bytes + ax_bytes, ay.data(), ay_bytes}},
                                  &mem))
        return rc;
    paris_hip_ctx::phase_t& s = ctx->phase;
    paris_hip_release(ctx, s);
    s.set = true;
    s.rule = *setting;
    s.mem = mem;
    s.dim_x = dim_x;
    s.dim_y = dim_y;
    s.n_x = nx;
    s.n_y = ny;
    s.frames = static_cast<uint32_t>(scratch / (static_cast<size_t>(dim_y) * (nx / 2u + 1u) * sizeof(float2)));
    return PARIS_HIP_SUCCESS;
}

extern "C" int paris_hip_clear_phase_retrieval(paris_hip_ctx* ctx)
{
    if(int rc = paris_hip_bind(ctx))
        return rc;
    paris_hip_release(ctx, ctx->phase);
    return PARIS_HIP_SUCCESS;
}

extern "C" int paris_hip_phase_retrieval_frames(paris_hip_ctx* ctx, float* d_p, size_t pitch, size_t frame_stride, uint32_t n_frames,
                                                uint32_t dim_x, uint32_t dim_y)
{
    const paris_hip_frame_band band{d_p, pitch, frame_stride, n_frames, dim_x, dim_y, 0u, dim_y};
    const auto refuse = [&]() -> int {
        const paris_hip_ctx::phase_t& s = ctx->phase;
        return !s.set || dim_x != s.dim_x || dim_y != s.dim_y ? PARIS_HIP_ERROR_INVALID_ARGUMENT : PARIS_HIP_SUCCESS;
    };
    const auto launch = [&] {
        const paris_hip_ctx::phase_t& s = ctx->phase;
        const uint32_t w = s.n_x / 2u + 1u, lx = log2_of(s.n_x), ly = log2_of(s.n_y);
        const size_t scratch_frame = static_cast<size_t>(dim_y) * w;
        const float2* tw_x = s.mem.as<float2>();
        const float2* tw_y = tw_x + s.n_x / 2u;
        const float* ax = reinterpret_cast<const float*>(tw_y + s.n_y / 2u);
        const float* ay = ax + s.n_x;
        float2* scratch = reinterpret_cast<float2*>(const_cast<float*>(ay + s.n_y));
        const uint32_t cols = std::min(PHASE_COLUMNS_MAX, PHASE_COLUMN_SAMPLES / s.n_y), lc = log2_of(cols);
        const uint32_t pairs = (dim_y + 1u) / 2u, sets = (w + cols - 1u) / cols;
        const uint32_t row_threads = threads_for(s.n_x / 2u), col_threads = threads_for(cols * (s.n_y / 2u));
        const size_t row_lds = s.n_x * sizeof(float2), col_lds = static_cast<size_t>(cols) * (s.n_y + 1u) * sizeof(float2);
        const float scale = 1.f / (static_cast<float>(s.n_x) * static_cast<float>(s.n_y)); // a power of two: exact
        // the scratch holds s.frames frames: larger calls loop, each round behind the last in stream order
        for(uint32_t f0 = 0; f0 < n_frames; f0 += s.frames)
        {
            const uint32_t nf = std::min(s.frames, n_frames - f0);
            hipLaunchKernelGGL(phase_rows_forward_kernel, dim3(pairs, nf), dim3(row_threads), row_lds, ctx->stream, band.frame(f0), pitch,
                               frame_stride, dim_x, dim_y, lx, tw_x, scratch, scratch_frame);
            hipLaunchKernelGGL(phase_columns_kernel, dim3(sets, nf), dim3(col_threads), col_lds, ctx->stream, scratch, scratch_frame, dim_y, w, lx,
                               ly, lc, tw_y, ax, ay);
            hipLaunchKernelGGL(phase_rows_inverse_kernel, dim3(pairs, nf), dim3(row_threads), row_lds, ctx->stream, band.frame(f0), pitch,
                               frame_stride, dim_x, dim_y, lx, tw_x, scratch, scratch_frame, scale, s.rule.t_min);
        }
    };
    return paris_hip_frame_pass(ctx, band, refuse, launch);
}

void paris_hip_warm_phase()
{
    hipFuncAttributes a{};
    (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&phase_rows_forward_kernel));
    (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&phase_columns_kernel));
    (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&phase_rows_inverse_kernel));
}
