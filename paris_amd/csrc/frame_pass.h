// The one launch scaffold of the passes that rewrite projection frames in place on the compute stream (DESIGN.md section 1,
// "Ordering"): the redundancy weights, the flat-field rows pass, the defect repair and the forward projector -- and, in its two-band
// form, of the binning pass, which reads one set of frames and writes another. Inline host code.
#ifndef PARIS_HIP_FRAME_PASS_H_
#define PARIS_HIP_FRAME_PASS_H_

#include "paris_hip_internal.h"

#pragma GCC visibility push(hidden) // (library-internal: not in the dynamic symbol table)

struct paris_hip_row_range
{
    uint32_t first, count;
};

// rows [row_first, row_first + row_count) of n_frames frames frame_stride bytes apart, starting at d_p, each dim_x x dim_y with rows
// pitch bytes apart
struct paris_hip_frame_band
{
    float* d_p;
    size_t pitch, frame_stride;
    uint32_t n_frames, dim_x, dim_y, row_first, row_count;

    char* frame(uint32_t f) const // row 0 of frame f
    {
        return reinterpret_cast<char*>(d_p) + f * frame_stride;
    }
    paris_hip_row_range rows() const
    {
        return {row_first, row_count};
    }
};

// the argument rule: float rows that hold dim_x pixels, a band inside the frame, frames that do not overlap
inline bool paris_hip_frame_band_valid(const paris_hip_frame_band& b)
{
    if(b.d_p == nullptr || b.pitch < static_cast<size_t>(b.dim_x) * sizeof(float) || b.pitch % sizeof(float) != 0 || b.row_first > b.dim_y
       || b.row_count > b.dim_y - b.row_first)
        return false;
    return b.n_frames <= 1u || (b.frame_stride % sizeof(float) == 0 && b.frame_stride >= b.pitch * static_cast<size_t>(b.dim_y));
}

// Deferral by reference: a buffer the pending group reads must not be rewritten before that group has run, and one a running group
// reads makes the compute stream wait. Always the whole frame, whatever the band.
inline int paris_hip_frame_band_guard(paris_hip_ctx* ctx, const paris_hip_frame_band& b)
{
    for(uint32_t f = 0; f < b.n_frames; ++f)
        if(int rc = paris_hip_projection_guard(ctx, b.frame(f), b.pitch * b.dim_y, ctx->stream, true))
            return rc;
    return PARIS_HIP_SUCCESS;
}

// Binds the ctx, runs an earlier weighting nobody filtered, checks the band, then the pass's own part:
//   refuse()  -> int    its own argument checks, a status;
//   idle()    -> bool   true: nothing to launch for this band -- the call ends BEFORE the guards, no pending group is launched;
//   launch()            enqueues the kernels on ctx->stream, split over the grid limits as the pass needs;
//   touched() -> paris_hip_row_range   the rows of each frame the kernels read or write, for the upload slots' ordering.
// Launch errors surface in paris_hip_finish.
template <typename Refuse, typename Idle, typename Launch, typename Touched>
inline int paris_hip_frame_pass(paris_hip_ctx* ctx, const paris_hip_frame_band& b, Refuse refuse, Idle idle, Launch launch, Touched touched)
{
    if(int rc = paris_hip_bind(ctx))
        return rc;
    if(int rc = paris_hip_flush_pending_weight(ctx))
        return rc;
    if(!paris_hip_frame_band_valid(b))
        return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    if(int rc = refuse())
        return rc;
    if(b.dim_x == 0 || b.row_count == 0 || b.n_frames == 0 || idle())
        return paris_hip_finish(ctx);
    if(int rc = paris_hip_frame_band_guard(ctx, b))
        return rc;
    launch();
    const paris_hip_row_range r = touched();
    for(uint32_t f = 0; f < b.n_frames; ++f)
        if(int rc = paris_hip_note_projection_use(ctx, b.frame(f) + static_cast<size_t>(r.first) * b.pitch, b.pitch * r.count))
            return rc;
    return paris_hip_finish(ctx);
}

// a pass that launches whenever the band is not empty and touches the band's rows only
template <typename Refuse, typename Launch>
inline int paris_hip_frame_pass(paris_hip_ctx* ctx, const paris_hip_frame_band& b, Refuse refuse, Launch launch)
{
    return paris_hip_frame_pass(ctx, b, refuse, [] { return false; }, launch, [&b] { return b.rows(); });
}

// the bytes from row 0 of the first frame to the end of the last frame's last row (band_valid has passed)
inline size_t paris_hip_frame_band_extent(const paris_hip_frame_band& b)
{
    if(b.n_frames == 0u || b.dim_y == 0u)
        return 0u;
    return (b.n_frames - 1u) * b.frame_stride + (b.dim_y - 1u) * b.pitch + static_cast<size_t>(b.dim_x) * sizeof(float);
}

// A pass that reads the band `src` of one set of frames and writes the band `dst` of another (the two may differ in size): the same
// order of steps, both bands checked, both sets of frames guarded and noted as used. Ranges that overlap are refused.
template <typename Refuse, typename Launch>
inline int paris_hip_frame_pass(paris_hip_ctx* ctx, const paris_hip_frame_band& src, const paris_hip_frame_band& dst, Refuse refuse, Launch launch)
{
    if(int rc = paris_hip_bind(ctx))
        return rc;
    if(int rc = paris_hip_flush_pending_weight(ctx))
        return rc;
    if(!paris_hip_frame_band_valid(src) || !paris_hip_frame_band_valid(dst) || src.n_frames != dst.n_frames)
        return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    if(int rc = refuse())
        return rc;
    const char* s = reinterpret_cast<const char*>(src.d_p);
    const char* d = reinterpret_cast<const char*>(dst.d_p);
    if(s < d + paris_hip_frame_band_extent(dst) && d < s + paris_hip_frame_band_extent(src))
        return PARIS_HIP_ERROR_INVALID_ARGUMENT;
    if(dst.dim_x == 0 || dst.row_count == 0 || dst.n_frames == 0)
        return paris_hip_finish(ctx);
    if(int rc = paris_hip_frame_band_guard(ctx, src))
        return rc;
    if(int rc = paris_hip_frame_band_guard(ctx, dst))
        return rc;
    launch();
    for(const paris_hip_frame_band* b : {&src, &dst})
        for(uint32_t f = 0; f < b->n_frames; ++f)
            if(int rc = paris_hip_note_projection_use(ctx, b->frame(f) + static_cast<size_t>(b->row_first) * b->pitch, b->pitch * b->row_count))
                return rc;
    return paris_hip_finish(ctx);
}

#pragma GCC visibility pop

#endif
