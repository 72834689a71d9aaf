// Metal artefact reduction for gfx950 (the statement is in include/paris_hip.h).
//
//   metal_count_kernel     a WAVE owns MC_CHUNK contiguous voxels at a time: 64 per step, lane l the l-th, the 64-bit __ballot of
//                          v > threshold popcounted. One 32-bit count per chunk.
//   metal_scan_kernel      the exclusive scan of the chunk counts to 64-bit offsets, by ONE block: 1024 counts per step, scanned in
//                          the waves with shuffles, across the waves through LDS, the carry in a register. The total goes behind
//                          the last offset.
//   metal_write_kernel     the same walk as the count: a hit's place is its chunk's offset, plus the hits of the steps before, plus
//                          the popcount of the ballot's lanes below its own. No atomics: the list is in ascending voxel index.
//   metal_binarize_kernel  v = v > threshold ? 1 : 0, 16 bytes per lane where the alignment allows.
//   metal_pack_kernel      a wave owns one word of one row: lane l decides for column 64 w + l whether any pixel of that column in
//                          rows y - grow .. y + grow is above min_path; the first 2 grow lanes do the same for the grow columns on
//                          either side of the word. The two ballots, shifted by -grow .. grow and ORed, are the word.
//   metal_inpaint_kernel   a wave owns one row of one frame. Its lanes read the row's words, one each; no bit set: done. Otherwise
//                          word after word, each lane whose bit is set finds the nearest clear bit on either side with leading /
//                          trailing zero counts -- walking further words if need be -- loads the two anchors and stores its pixel.
//                          The counts are popcounts of ballots, added once per wave: integers, whatever the order.
//   metal_reinsert_kernel  v[index[k] - base] = value[k] for the slab's part of the list.
// Every kernel runs on a capped grid with a stride loop; voxel indices are 64-bit.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "frame_pass.h"

namespace
{
    constexpr uint32_t M_THREADS = 256u, M_WAVES = M_THREADS / 64u;
    constexpr uint32_t MC_CHUNK = 4096u;      // voxels per count: 64 steps of a wave
    constexpr uint32_t MC_GRID_MAX = 2048u;   // streams: every SIMD holds its 8 waves (as the stats kernel of volume_window.hip)
    constexpr uint32_t MS_THREADS = 1024u;    // the scan's one block
    constexpr uint32_t MP_GRID_MAX = 4096u;   // pack and inpaint: a wave per task, M_WAVES tasks per block and step
    constexpr uint32_t MI_VIEWS = 64u;        // frames one inpaint launch serves: their view numbers travel by value

    __device__ __forceinline__ uint32_t m_lane()
    {
        return threadIdx.x & 63u;
    }

    // the hits of this wave's step of chunk `c`: lane l looks at voxel c * MC_CHUNK + 64 s + l
    __device__ __forceinline__ bool metal_hit(const float* __restrict__ v, uint64_t n, uint64_t i, float thr, float* value)
    {
        const float x = i < n ? __builtin_nontemporal_load(v + i) : 0.f;
        *value = x;
        return i < n && x > thr; // (false for NaN)
    }

    __global__ void __launch_bounds__(M_THREADS)
        metal_count_kernel(const float* __restrict__ v, uint64_t n, uint64_t chunks, float thr, uint32_t* __restrict__ count)
    {
        const uint32_t lane = m_lane();
        for(uint64_t c = static_cast<uint64_t>(blockIdx.x) * M_WAVES + threadIdx.x / 64u; c < chunks; c += static_cast<uint64_t>(gridDim.x) * M_WAVES)
        {
            const uint64_t base = c * MC_CHUNK + lane;
            uint32_t hits = 0;
#pragma unroll 8
            for(uint32_t s = 0; s < MC_CHUNK / 64u; ++s)
            {
                float x;
                hits += static_cast<uint32_t>(__popcll(__ballot(metal_hit(v, n, base + s * 64u, thr, &x))));
            }
            if(lane == 0u)
                count[c] = hits;
        }
    }

    // offset[c] = count[0] + ... + count[c - 1], c <= chunks (offset[chunks]: the total)
    __global__ void __launch_bounds__(MS_THREADS) metal_scan_kernel(const uint32_t* __restrict__ count, uint64_t chunks, uint64_t* __restrict__ offset)
    {
        __shared__ uint32_t wave_sum[MS_THREADS / 64u];
        const uint32_t lane = m_lane(), wave = threadIdx.x / 64u;
        uint64_t carry = 0;
        for(uint64_t c0 = 0; c0 < chunks; c0 += MS_THREADS)
        {
            const uint64_t c = c0 + threadIdx.x;
            const uint32_t mine = c < chunks ? count[c] : 0u;
            uint32_t incl = mine; // inclusive within the wave; a step holds at most 1024 * 4096 hits
#pragma unroll
            for(uint32_t d = 1; d < 64u; d <<= 1)
            {
                const uint32_t up = __shfl_up(incl, d);
                incl += lane >= d ? up : 0u;
            }
            if(lane == 63u)
                wave_sum[wave] = incl;
            __syncthreads();
            uint32_t before = 0, all = 0;
#pragma unroll
            for(uint32_t w = 0; w < MS_THREADS / 64u; ++w)
            {
                const uint32_t s = wave_sum[w];
                before += w < wave ? s : 0u;
                all += s;
            }
            if(c < chunks)
                offset[c] = carry + before + (incl - mine);
            carry += all;
            __syncthreads();
        }
        if(threadIdx.x == 0u)
            offset[chunks] = carry;
    }

    __global__ void __launch_bounds__(M_THREADS)
        metal_write_kernel(const float* __restrict__ v, uint64_t n, uint64_t chunks, float thr, const uint64_t* __restrict__ offset,
                           uint64_t* __restrict__ index, float* __restrict__ value)
    {
        const uint32_t lane = m_lane();
        const uint64_t below = (uint64_t{1} << lane) - 1u;
        for(uint64_t c = static_cast<uint64_t>(blockIdx.x) * M_WAVES + threadIdx.x / 64u; c < chunks; c += static_cast<uint64_t>(gridDim.x) * M_WAVES)
        {
            uint64_t at = offset[c];
            if(offset[c + 1u] == at)
                continue; // (wave-uniform: nothing in this chunk)
            const uint64_t base = c * MC_CHUNK + lane;
            for(uint32_t s = 0; s < MC_CHUNK / 64u; ++s)
            {
                float x;
                const bool hit = metal_hit(v, n, base + s * 64u, thr, &x);
                const uint64_t b = __ballot(hit);
                if(hit)
                {
                    const uint64_t k = at + static_cast<uint64_t>(__popcll(b & below));
                    index[k] = base + s * 64u;
                    value[k] = x;
                }
                at += static_cast<uint64_t>(__popcll(b));
            }
        }
    }

    // v[0, n): head < 4 voxels before the first 16-byte boundary, then whole groups of 4, then the rest
    __global__ void __launch_bounds__(M_THREADS) metal_binarize_kernel(float* __restrict__ v, uint64_t n, uint32_t head, float thr)
    {
        const uint64_t first = static_cast<uint64_t>(blockIdx.x) * M_THREADS + threadIdx.x, stride = static_cast<uint64_t>(gridDim.x) * M_THREADS;
        const uint64_t groups = (n - head) / 4u;
        float4* __restrict__ q = reinterpret_cast<float4*>(v + head);
        for(uint64_t g = first; g < groups; g += stride)
        {
            float4 t = q[g];
            t.x = t.x > thr ? 1.f : 0.f;
            t.y = t.y > thr ? 1.f : 0.f;
            t.z = t.z > thr ? 1.f : 0.f;
            t.w = t.w > thr ? 1.f : 0.f;
            q[g] = t;
        }
        if(blockIdx.x == 0u)
        {
            const uint64_t tail0 = head + groups * 4u;
            if(threadIdx.x < head)
                v[threadIdx.x] = v[threadIdx.x] > thr ? 1.f : 0.f;
            if(tail0 + threadIdx.x < n)
                v[tail0 + threadIdx.x] = v[tail0 + threadIdx.x] > thr ? 1.f : 0.f;
        }
    }

    // is any pixel of column x in rows [y0, y1] of the frame above min_path? (x outside the frame: no)
    __device__ __forceinline__ bool metal_column_hit(const char* __restrict__ frame, size_t pitch, uint32_t dim_x, int64_t x, uint32_t y0, uint32_t y1,
                                                     float min_path)
    {
        bool hit = false;
        if(x >= 0 && x < static_cast<int64_t>(dim_x))
            for(uint32_t y = y0; y <= y1; ++y)
                hit = hit || reinterpret_cast<const float*>(frame + static_cast<size_t>(y) * pitch)[x] > min_path;
        return hit;
    }

    // t: row 0 of the first frame. Task = (frame, row, word), the word fastest. bits: frame after frame, dense.
    __global__ void __launch_bounds__(M_THREADS)
        metal_pack_kernel(const char* __restrict__ t, size_t pitch, size_t frame_stride, uint32_t dim_x, uint32_t dim_y, uint32_t words, uint64_t tasks,
                          float min_path, uint32_t grow, uint64_t* __restrict__ bits)
    {
        const uint32_t lane = m_lane();
        for(uint64_t k = static_cast<uint64_t>(blockIdx.x) * M_WAVES + threadIdx.x / 64u; k < tasks; k += static_cast<uint64_t>(gridDim.x) * M_WAVES)
        {
            const uint32_t w = static_cast<uint32_t>(k % words);
            const uint64_t fy = k / words;
            const uint32_t y = static_cast<uint32_t>(fy % dim_y), f = static_cast<uint32_t>(fy / dim_y);
            const char* frame = t + static_cast<size_t>(f) * frame_stride;
            const uint32_t y0 = y - (y < grow ? y : grow), y1 = dim_y - 1u - y < grow ? dim_y - 1u : y + grow;
            const int64_t x = static_cast<int64_t>(w) * 64 + lane;
            const uint64_t own = __ballot(metal_column_hit(frame, pitch, dim_x, x, y0, y1, min_path));
            // the columns beside the word: lanes [0, grow) take x0 - grow + l, lanes [grow, 2 grow) take x0 + 64 + (l - grow)
            const int64_t xs = lane < grow ? x - grow : x + 64 - grow;
            const uint64_t side = __ballot(lane < 2u * grow && metal_column_hit(frame, pitch, dim_x, xs, y0, y1, min_path));
            const uint64_t left = side & ((uint64_t{1} << grow) - 1u), right = side >> grow; // (bit j: column x0 - grow + j / x0 + 64 + j)
            uint64_t word = own;
            for(uint32_t d = 1; d <= grow; ++d)
                word |= (own << d) | (left >> (grow - d)) | (own >> d) | (right << (64u - d));
            const uint32_t valid = dim_x - w * 64u; // columns of the frame from this word on
            if(valid < 64u)
                word &= (uint64_t{1} << valid) - 1u;
            if(lane == 0u)
                bits[k] = word;
        }
    }

    struct metal_views // the trace of each frame of a launch
    {
        uint32_t v[MI_VIEWS];
    };

    // p: row 0 of the launch's first frame. Task = (frame, band row), the row fastest. trace: the setting's words; acc: its counters.
    __global__ void __launch_bounds__(M_THREADS)
        metal_inpaint_kernel(char* __restrict__ p, size_t pitch, size_t frame_stride, uint32_t dim_x, uint32_t dim_y, uint32_t words, uint32_t row_first,
                             uint32_t row_count, uint64_t tasks, const uint64_t* __restrict__ trace, unsigned long long* __restrict__ acc, metal_views views)
    {
        const uint32_t lane = m_lane();
        uint32_t replaced = 0, runs = 0, rows_left = 0; // of this wave (wave-uniform)
        for(uint64_t k = static_cast<uint64_t>(blockIdx.x) * M_WAVES + threadIdx.x / 64u; k < tasks; k += static_cast<uint64_t>(gridDim.x) * M_WAVES)
        {
            const uint32_t f = static_cast<uint32_t>(k / row_count), y = row_first + static_cast<uint32_t>(k % row_count);
            const uint64_t* __restrict__ b = trace + (static_cast<uint64_t>(views.v[f]) * dim_y + y) * words;
            bool any = false;
            for(uint32_t w0 = 0; w0 < words; w0 += 64u)
                any = any || (w0 + lane < words && b[w0 + lane] != 0u);
            if(__ballot(any) == 0u)
                continue; // the usual row: no metal on it
            float* row = reinterpret_cast<float*>(p + static_cast<size_t>(f) * frame_stride + static_cast<size_t>(y) * pitch);
            for(uint32_t w = 0; w < words; ++w)
            {
                const uint64_t word = b[w];
                if(word == 0u)
                    continue;
                const bool set = ((word >> lane) & 1u) != 0u;
                bool wrote = false, starts = false, whole = false;
                if(set)
                {
                    const uint32_t x = w * 64u + lane;
                    // the nearest clear bit to the left (-1: the run touches the edge) ...
                    int64_t lo = -1;
                    uint64_t clear = ~word & ((uint64_t{1} << lane) - 1u);
                    for(uint32_t ww = w;;)
                    {
                        if(clear != 0u)
                        {
                            lo = static_cast<int64_t>(ww) * 64 + 63 - __clzll(static_cast<long long>(clear));
                            break;
                        }
                        if(ww == 0u)
                            break;
                        clear = ~b[--ww];
                    }
                    // ... and to the right (dim_x: the edge). The last word's bits beyond the row are clear: a find there is the edge.
                    int64_t hi = dim_x;
                    clear = ~word & ~((uint64_t{2} << lane) - 1u);
                    for(uint32_t ww = w;;)
                    {
                        if(clear != 0u)
                        {
                            const int64_t at = static_cast<int64_t>(ww) * 64 + __ffsll(static_cast<unsigned long long>(clear)) - 1;
                            hi = at < static_cast<int64_t>(dim_x) ? at : static_cast<int64_t>(dim_x);
                            break;
                        }
                        if(++ww == words)
                            break;
                        clear = ~b[ww];
                    }
                    starts = lo == static_cast<int64_t>(x) - 1;
                    if(lo < 0 && hi >= static_cast<int64_t>(dim_x))
                        whole = true;
                    else
                    {
                        float out;
                        if(lo < 0)
                            out = row[hi];
                        else if(hi >= static_cast<int64_t>(dim_x))
                            out = row[lo];
                        else
                        {
                            const float pl = row[lo], pr = row[hi];
                            const float t = static_cast<float>(static_cast<int64_t>(x) - lo) / static_cast<float>(hi - lo);
                            out = __builtin_fmaf(t, pr - pl, pl);
                        }
                        row[x] = out; // anchors lie outside the trace: no lane writes what another reads
                        wrote = true;
                    }
                }
                replaced += static_cast<uint32_t>(__popcll(__ballot(wrote)));
                runs += static_cast<uint32_t>(__popcll(__ballot(wrote && starts)));
                rows_left += static_cast<uint32_t>(__popcll(__ballot(whole && starts)));
            }
        }
        if(lane == 0u)
        {
            if(replaced != 0u)
                atomicAdd(&acc[0], static_cast<unsigned long long>(replaced));
            if(runs != 0u)
                atomicAdd(&acc[1], static_cast<unsigned long long>(runs));
            if(rows_left != 0u)
                atomicAdd(&acc[2], static_cast<unsigned long long>(rows_left));
        }
    }

    __global__ void __launch_bounds__(M_THREADS)
        metal_reinsert_kernel(float* __restrict__ v, uint64_t base, const uint64_t* __restrict__ index, const float* __restrict__ value, uint64_t n)
    {
        for(uint64_t k = static_cast<uint64_t>(blockIdx.x) * M_THREADS + threadIdx.x; k < n; k += static_cast<uint64_t>(gridDim.x) * M_THREADS)
            v[index[k] - base] = value[k];
    }

    uint32_t metal_blocks(uint64_t items, uint32_t per_block, uint32_t cap)
    {
        return static_cast<uint32_t>(std::min<uint64_t>(cap, (items + per_block - 1u) / per_block));
    }
}

extern "C" int paris_hip_metal_collect(paris_hip_ctx* ctx, float* d_v, uint32_t dim_x, uint32_t dim_y, uint32_t dim_z, float threshold, uint64_t max_n,
                                       uint64_t* h_index, float* h_value, uint64_t* n, int binarize)
{
    if(int rc = paris_hip_flush_deferred(ctx))
        return rc;
    if(int rc = paris_hip_bind(ctx))
        return rc;
    if(d_v == nullptr || n == nullptr || reinterpret_cast<uintptr_t>(d_v) % sizeof(float) != 0u
       || paris_hip_metal_check(dim_x, dim_y, dim_z, threshold, 0u, 0.f, nullptr) != PARIS_HIP_SUCCESS
       || (max_n != 0u && (h_index == nullptr || h_value == nullptr)))
        return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    const uint64_t voxels = static_cast<uint64_t>(dim_x) * dim_y * dim_z;
    const uint64_t chunks = (voxels + MC_CHUNK - 1u) / MC_CHUNK;
    // one allocation: the offsets (chunks + 1), the counts, and -- once the count is known -- a second one for the lists
    const size_t offset_bytes = (chunks + 1u) * sizeof(uint64_t);
    char* scratch = nullptr;
    if(int rc = paris_hip_device_malloc(ctx, reinterpret_cast<void**>(&scratch), offset_bytes + chunks * sizeof(uint32_t)))
        return rc;
    uint64_t* offset = reinterpret_cast<uint64_t*>(scratch);
    uint32_t* count = reinterpret_cast<uint32_t*>(scratch + offset_bytes);
    char* lists = nullptr;
    const auto done = [&](int rc) { // nothing of this call is left on the stream or on the device
        (void)hipStreamSynchronize(ctx->stream);
        (void)hipFree(scratch);
        if(lists != nullptr)
            (void)hipFree(lists);
        return rc;
    };
    const uint32_t blocks = metal_blocks(chunks, M_WAVES, MC_GRID_MAX);
    hipLaunchKernelGGL(metal_count_kernel, dim3(blocks), dim3(M_THREADS), 0, ctx->stream, d_v, voxels, chunks, threshold, count);
    hipLaunchKernelGGL(metal_scan_kernel, dim3(1), dim3(MS_THREADS), 0, ctx->stream, count, chunks, offset);
    hipError_t err = hipGetLastError();
    uint64_t total = 0;
    if(err == hipSuccess)
        err = hipMemcpyAsync(&total, offset + chunks, sizeof(total), hipMemcpyDeviceToHost, ctx->stream);
    if(err == hipSuccess)
        err = hipStreamSynchronize(ctx->stream);
    if(err != hipSuccess)
        return done(static_cast<int>(err));
    *n = total;
    if(total > max_n)
        return done(PARIS_HIP_ERROR_METAL_TOO_MANY_VOXELS);
    if(total != 0u)
    {
        if(int rc = paris_hip_device_malloc(ctx, reinterpret_cast<void**>(&lists), total * (sizeof(uint64_t) + sizeof(float))))
            return done(rc);
        uint64_t* d_index = reinterpret_cast<uint64_t*>(lists);
        float* d_value = reinterpret_cast<float*>(lists + total * sizeof(uint64_t));
        hipLaunchKernelGGL(metal_write_kernel, dim3(blocks), dim3(M_THREADS), 0, ctx->stream, d_v, voxels, chunks, threshold, offset, d_index, d_value);
        err = hipGetLastError();
        if(err == hipSuccess)
            err = hipMemcpyAsync(h_index, d_index, total * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream);
        if(err == hipSuccess)
            err = hipMemcpyAsync(h_value, d_value, total * sizeof(float), hipMemcpyDeviceToHost, ctx->stream);
        if(err != hipSuccess)
            return done(static_cast<int>(err));
    }
    if(binarize)
    {
        if(int rc = paris_hip_volume_mark_dirty(ctx, d_v, voxels * sizeof(float)))
            return done(rc);
        const uint32_t to_boundary = ((16u - static_cast<uint32_t>(reinterpret_cast<uintptr_t>(d_v) & 15u)) & 15u) / 4u;
        const uint32_t head = static_cast<uint32_t>(std::min<uint64_t>(voxels, to_boundary));
        const uint64_t items = std::max<uint64_t>(1u, (voxels - head) / 4u);
        hipLaunchKernelGGL(metal_binarize_kernel, dim3(metal_blocks(items, M_THREADS, MC_GRID_MAX)), dim3(M_THREADS), 0, ctx->stream, d_v, voxels, head,
                           threshold);
        err = hipGetLastError();
        if(err != hipSuccess)
            return done(static_cast<int>(err));
    }
    err = hipStreamSynchronize(ctx->stream);
    return done(static_cast<int>(err));
}

extern "C" int paris_hip_metal_trace_pack(paris_hip_ctx* ctx, const float* d_t, size_t pitch, size_t frame_stride, uint32_t n_frames, uint32_t dim_x,
                                          uint32_t dim_y, float min_path, uint32_t grow, uint64_t* h_bits)
{
    const paris_hip_frame_band band{const_cast<float*>(d_t), pitch, frame_stride, n_frames, dim_x, dim_y, 0u, dim_y};
    const uint32_t words = (dim_x + 63u) / 64u;
    const uint64_t tasks = static_cast<uint64_t>(n_frames) * dim_y * words;
    uint64_t* d_bits = nullptr;
    int own_rc = PARIS_HIP_SUCCESS;
    const auto refuse = [&]() -> int {
        if(grow > PARIS_HIP_METAL_GROW_MAX || !std::isfinite(min_path) || min_path < 0.f || (tasks != 0u && h_bits == nullptr))
            return PARIS_HIP_ERROR_INVALID_ARGUMENT;
        return PARIS_HIP_SUCCESS;
    };
    const auto launch = [&] {
        own_rc = paris_hip_device_malloc(ctx, reinterpret_cast<void**>(&d_bits), tasks * sizeof(uint64_t));
        if(own_rc != PARIS_HIP_SUCCESS)
            return;
        hipLaunchKernelGGL(metal_pack_kernel, dim3(metal_blocks(tasks, M_WAVES, MP_GRID_MAX)), dim3(M_THREADS), 0, ctx->stream,
                           reinterpret_cast<const char*>(d_t), pitch, frame_stride, dim_x, dim_y, words, tasks, min_path, grow, d_bits);
        own_rc = static_cast<int>(hipMemcpyAsync(h_bits, d_bits, tasks * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    };
    const int rc = paris_hip_frame_pass(ctx, band, refuse, launch);
    if(d_bits != nullptr)
    {
        const hipError_t waited = hipStreamSynchronize(ctx->stream);
        (void)hipFree(d_bits);
        if(own_rc == PARIS_HIP_SUCCESS)
            own_rc = static_cast<int>(waited);
    }
    return own_rc != PARIS_HIP_SUCCESS ? own_rc : rc;
}

extern "C" int paris_hip_set_metal_trace(paris_hip_ctx* ctx, const uint64_t* h_bits, uint32_t n_views, uint32_t dim_x, uint32_t dim_y)
{
    if(int rc = paris_hip_bind(ctx))
        return rc;
    if(h_bits == nullptr || n_views == 0u || dim_x == 0u || dim_y == 0u)
        return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    const uint32_t words = (dim_x + 63u) / 64u;
    const size_t bytes = static_cast<size_t>(n_views) * dim_y * words * sizeof(uint64_t);
    paris_hip_device_buffer mem; // the counters start at zero
    if(int rc = paris_hip_install(ctx, PARIS_HIP_METAL_COUNTER_BYTES + bytes,
                                  {{0u, nullptr, PARIS_HIP_METAL_COUNTER_BYTES}, {PARIS_HIP_METAL_COUNTER_BYTES, h_bits, bytes}}, &mem))
        return rc;
    paris_hip_ctx::metal_trace_t& m = ctx->metal_trace;
    paris_hip_release(ctx, m);
    m.set = true;
    m.mem = mem;
    m.n_views = n_views;
    m.dim_x = dim_x;
    m.dim_y = dim_y;
    m.words = words;
    return PARIS_HIP_SUCCESS;
}

extern "C" int paris_hip_clear_metal_trace(paris_hip_ctx* ctx)
{
    if(int rc = paris_hip_bind(ctx))
        return rc;
    paris_hip_release(ctx, ctx->metal_trace);
    return PARIS_HIP_SUCCESS;
}

extern "C" int paris_hip_metal_inpaint_rows(paris_hip_ctx* ctx, float* d_p, size_t pitch, size_t frame_stride, uint32_t n_frames, uint32_t dim_x,
                                            uint32_t dim_y, uint32_t row_first, uint32_t row_count, const uint32_t* h_view)
{
    const paris_hip_frame_band band{d_p, pitch, frame_stride, n_frames, dim_x, dim_y, row_first, row_count};
    const auto refuse = [&]() -> int {
        const paris_hip_ctx::metal_trace_t& m = ctx->metal_trace;
        if(!m.set || dim_x != m.dim_x || dim_y != m.dim_y || (n_frames != 0u && h_view == nullptr))
            return PARIS_HIP_ERROR_INVALID_ARGUMENT;
        for(uint32_t f = 0; f < n_frames; ++f)
            if(h_view[f] >= m.n_views)
                return PARIS_HIP_ERROR_INVALID_ARGUMENT;
        return PARIS_HIP_SUCCESS;
    };
    return paris_hip_frame_pass(ctx, band, refuse, [&] {
        const paris_hip_ctx::metal_trace_t& m = ctx->metal_trace;
        unsigned long long* acc = m.mem.as<unsigned long long>();
        const uint64_t* trace = reinterpret_cast<const uint64_t*>(m.mem.as<char>() + PARIS_HIP_METAL_COUNTER_BYTES);
        for(uint32_t f0 = 0; f0 < n_frames; f0 += MI_VIEWS)
        {
            const uint32_t nf = std::min(MI_VIEWS, n_frames - f0);
            metal_views views{};
            for(uint32_t f = 0; f < nf; ++f)
                views.v[f] = h_view[f0 + f];
            const uint64_t tasks = static_cast<uint64_t>(nf) * row_count;
            hipLaunchKernelGGL(metal_inpaint_kernel, dim3(metal_blocks(tasks, M_WAVES, MP_GRID_MAX)), dim3(M_THREADS), 0, ctx->stream, band.frame(f0),
                               pitch, frame_stride, dim_x, dim_y, m.words, row_first, row_count, tasks, trace, acc, views);
        }
    });
}

extern "C" int paris_hip_metal_stats(paris_hip_ctx* ctx, paris_hip_metal_counts* out, int reset)
{
    if(int rc = paris_hip_bind(ctx))
        return rc;
    if(out == nullptr || !ctx->metal_trace.set)
        return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    if(int rc = paris_hip_flush_pending_weight(ctx))
        return rc;
    unsigned long long acc[3] = {0, 0, 0};
    PARIS_HIP_TRY(hipMemcpyAsync(acc, ctx->metal_trace.mem.d, sizeof(acc), hipMemcpyDeviceToHost, ctx->stream));
    if(reset)
        PARIS_HIP_TRY(hipMemsetAsync(ctx->metal_trace.mem.d, 0, PARIS_HIP_METAL_COUNTER_BYTES, ctx->stream));
    PARIS_HIP_TRY(hipStreamSynchronize(ctx->stream));
    out->replaced = acc[0];
    out->runs = acc[1];
    out->rows_left = acc[2];
    return PARIS_HIP_SUCCESS;
}

extern "C" int paris_hip_set_metal_voxels(paris_hip_ctx* ctx, const uint64_t* h_index, const float* h_value, uint64_t n)
{
    if(int rc = paris_hip_bind(ctx))
        return rc;
    if(n != 0u && (h_index == nullptr || h_value == nullptr))
        return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    for(uint64_t k = 1; k < n; ++k)
        if(h_index[k] <= h_index[k - 1u])
            return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    paris_hip_device_buffer mem;
    if(n != 0u)
        if(int rc = paris_hip_install(ctx, n * (sizeof(uint64_t) + sizeof(float)),
                                      {{0u, h_index, n * sizeof(uint64_t)}, {n * sizeof(uint64_t), h_value, n * sizeof(float)}}, &mem))
            return rc;
    paris_hip_ctx::metal_voxels_t& m = ctx->metal_voxels;
    paris_hip_release(ctx, m);
    m.set = true;
    m.mem = mem;
    m.index.assign(h_index, h_index + n);
    return PARIS_HIP_SUCCESS;
}

extern "C" int paris_hip_clear_metal_voxels(paris_hip_ctx* ctx)
{
    if(int rc = paris_hip_bind(ctx))
        return rc;
    paris_hip_release(ctx, ctx->metal_voxels);
    return PARIS_HIP_SUCCESS;
}

extern "C" int paris_hip_metal_reinsert(paris_hip_ctx* ctx, float* d_v, uint32_t dim_x, uint32_t dim_y, uint32_t v_dim_z, uint32_t v_offset)
{
    if(int rc = paris_hip_flush_deferred(ctx))
        return rc;
    if(int rc = paris_hip_bind(ctx))
        return rc;
    const paris_hip_ctx::metal_voxels_t& m = ctx->metal_voxels;
    if(!m.set || d_v == nullptr || dim_x == 0u || dim_y == 0u || reinterpret_cast<uintptr_t>(d_v) % sizeof(float) != 0u)
        return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    const uint64_t plane = static_cast<uint64_t>(dim_x) * dim_y;
    const uint64_t base = plane * v_offset, end = base + plane * v_dim_z;
    const uint64_t lo = static_cast<uint64_t>(std::lower_bound(m.index.begin(), m.index.end(), base) - m.index.begin());
    const uint64_t hi = static_cast<uint64_t>(std::lower_bound(m.index.begin(), m.index.end(), end) - m.index.begin());
    if(hi == lo)
        return PARIS_HIP_SUCCESS;
    if(int rc = paris_hip_volume_mark_dirty(ctx, d_v, plane * v_dim_z * sizeof(float))) // (a listed value may be a -0)
        return rc;
    const uint64_t* index = m.mem.as<uint64_t>();
    const float* value = reinterpret_cast<const float*>(m.mem.as<char>() + m.index.size() * sizeof(uint64_t));
    hipLaunchKernelGGL(metal_reinsert_kernel, dim3(metal_blocks(hi - lo, M_THREADS, MC_GRID_MAX)), dim3(M_THREADS), 0, ctx->stream, d_v, base, index + lo,
                       value + lo, hi - lo);
    return paris_hip_finish(ctx);
}

void paris_hip_warm_metal()
{
    hipFuncAttributes a{};
    (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&metal_count_kernel));
    (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&metal_pack_kernel));
    (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&metal_inpaint_kernel));
}
