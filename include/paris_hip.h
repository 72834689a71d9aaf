/*
 * paris_hip.h -- C ABI of the MI355X (gfx950) backend for the hzdr/PARIS FDK hot path.
 *
 * This is the drop-in boundary. PARIS selects a backend at compile time through a namespace alias
 * (src/backend.h:26-47); a backend is a set of types plus 14 free functions (src/generic/backend.h:54-88,
 * src/openmp/backend.h:42-89, src/cuda/backend.h:50-103). The C++ header paris_amd/host/hip/backend.h
 * implements that surface (namespace paris::hip) on top of the entry points below; INTEGRATION.md shows
 * the `#elif defined(PARIS_ENABLE_HIP)` arm a maintainer adds to src/backend.h.
 *
 * Conventions
 *   - plain pointers and sizes only; every function returns 0 (PARIS_HIP_SUCCESS) or a non-zero status
 *     (hipError_t values are passed through, library-specific ones start at 10000); no exceptions cross
 *     this boundary. paris_hip_strerror() turns a status into text. The C++ wrappers translate a non-zero
 *     status into paris::stage_runtime_error / stage_construction_error (src/exception.h:31-41).
 *   - a paris_hip_ctx replaces every function-local `static` / `thread_local static` of the reference
 *     (src/weighting.cpp:37-42, src/filtering.cpp:37-42, src/backprojection.cpp:49-50,
 *     src/cuda/filtering.cu:189-240, src/cuda/backprojection.cu:160-185): device, stream, FFT scratch.
 *     One ctx per device and host thread; a ctx is not thread-safe (reference contract "thread == device",
 *     src/main.cpp:87,157-167).
 *   - all device work is enqueued on the ctx stream. Calls are asynchronous unless the ctx was created with
 *     PARIS_HIP_CTX_SYNCHRONOUS, in which case every call synchronises the stream before it returns, as
 *     the reference's CUDA backend does (src/cuda/weighting.cu:72, filtering.cu:260, backprojection.cu:236).
 *   - projections are row-major `buf[s + t * pitch/4]`, s in [0, dim_x) fastest (src/openmp/weighting.cpp:41);
 *     `pitch` is the row stride in BYTES (>= dim_x*4, multiple of 4), the same meaning as
 *     cuda::projection_device_buffer_type::pitch() (src/cuda/weighting.cu:43-45).
 *     Volumes are dense `buf[k + l*dim_x + m*dim_x*dim_y]` (src/openmp/backprojection.cpp:102) with 64-bit
 *     indexing (the reference's 32-bit arithmetic, SURVEY.md Q3, is not reproduced).
 */
#ifndef PARIS_HIP_H_
#define PARIS_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PARIS_HIP_SUCCESS 0
#define PARIS_HIP_ERROR_INVALID_ARGUMENT 10001
#define PARIS_HIP_ERROR_NO_DEVICE 10002
#define PARIS_HIP_ERROR_UNSUPPORTED 10003
/* what paris_hip_bh_solve refuses (the beam-hardening fit below) */
#define PARIS_HIP_ERROR_BH_TOO_FEW_VOXELS 10004 /* fewer object or air voxels than the caller's minimum */
#define PARIS_HIP_ERROR_BH_NOT_POSITIVE 10005   /* a Cholesky pivot of the normal equations is not positive */
#define PARIS_HIP_ERROR_BH_NOT_FINITE 10006     /* a coefficient is not a finite float */
/* what paris_hip_metal_collect may return beside those */
#define PARIS_HIP_ERROR_METAL_TOO_MANY_VOXELS 10007 /* the threshold marks more voxels than the caller's cap */

/* ctx flags */
#define PARIS_HIP_CTX_DEFAULT 0u
#define PARIS_HIP_CTX_SYNCHRONOUS 1u /* sync the stream before every call returns (reference behaviour) */
#define PARIS_HIP_CTX_LEGACY_STREAM 2u /* with stream == NULL: enqueue on the legacy default stream instead of a private one */
/* paris_hip_ctx_create also does the one-off work a per-projection loop would otherwise pay inside its first iterations: the
 * ctx's upload, second and auxiliary streams and their events are created (a stream costs 2-20 ms), the library's code objects are
 * loaded and the runtime's host-to-device path is exercised once. What set_device() of the C++ mirror asks for (src/main.cpp:87
 * binds the device once per thread, before the task loop). Results never depend on it. */
#define PARIS_HIP_CTX_WARM 4u

/* src/geometry.h:30-46, field for field */
typedef struct paris_detector_geometry {
    uint32_t n_row;   /* pixels per row */
    uint32_t n_col;   /* pixels per column */
    float l_px_row;   /* pixel size, horizontal [mm] */
    float l_px_col;   /* pixel size, vertical [mm] */
    float delta_s;    /* horizontal offset [px] */
    float delta_t;    /* vertical offset [px] */
    float d_so;       /* source -> object */
    float d_od;       /* object -> detector */
    float delta_phi;  /* angle step [deg] */
} paris_detector_geometry;

/* src/geometry.h:48-57 */
typedef struct paris_volume_geometry {
    uint32_t dim_x, dim_y, dim_z;
    float l_vx_x, l_vx_y, l_vx_z;
} paris_volume_geometry;

/* src/geometry.h:59-69 */
typedef struct paris_subvolume_geometry {
    uint32_t dim_x, dim_y, dim_z;
    uint32_t remainder;
} paris_subvolume_geometry;

/* src/region_of_interest.h:30-38 */
typedef struct paris_region_of_interest {
    uint32_t x1, x2, y1, y2, z1, z2;
} paris_region_of_interest;

/* src/subvolume_information.h:30-34 */
typedef struct paris_subvolume_info {
    paris_subvolume_geometry geo;
    int num;
} paris_subvolume_info;

typedef struct paris_hip_ctx paris_hip_ctx;

/* ---- device management: backend::get_devices / set_device (src/cuda/device.cpp:31-47,
 *      src/openmp/backend.h:87-89) -------------------------------------------------------------------- */
/* Environment switches (diagnostics, read once per process): PARIS_HIP_VIRTUAL_DEVICES=k reports k device handles
 * mapped round-robin onto the physical GPUs (exercises the one-thread-per-device driver on a one-GPU box);
 * PARIS_HIP_UPLOAD_STREAM=0 keeps paris_hip_upload_projection on the compute stream (A/B of the overlap; experiments build only). */
int paris_hip_device_count(int* count);

/* Creates the per-device state. `stream` is a hipStream_t to enqueue on (e.g. the caller's torch stream),
 * or NULL to let the ctx create and own a non-blocking stream -- which is NOT ordered with work on the legacy
 * default stream: a caller whose own work runs on the default stream (handle 0, e.g. PyTorch without an explicit
 * stream) passes NULL together with PARIS_HIP_CTX_LEGACY_STREAM. Replaces set_device + all thread_local statics. */
int paris_hip_ctx_create(int device, void* stream, unsigned flags, paris_hip_ctx** out);
int paris_hip_ctx_destroy(paris_hip_ctx* ctx);
/* synchronize_stream (src/cuda/stream.cpp) */
int paris_hip_ctx_synchronize(paris_hip_ctx* ctx);
/* the hipStream_t the ctx enqueues on */
void* paris_hip_ctx_stream(paris_hip_ctx* ctx);

/* ---- fences (extension): a marker in the ctx stream the host can wait on, so a pipelined driver can reuse a pinned
 *      upload buffer as soon as the copy that reads it has finished, without draining the whole stream ---------- */
typedef struct paris_hip_fence paris_hip_fence;
int paris_hip_fence_create(paris_hip_ctx* ctx, paris_hip_fence** out);
int paris_hip_fence_record(paris_hip_ctx* ctx, paris_hip_fence* fence);
/* returns at once if never recorded. Touches no ctx state (ctx only names the device): a thread other than the ctx's own may wait for a
 * fence that thread has been told is recorded -- paris.hip's feed and drain threads do (paris_amd/host/paris/reconstruct.h) -- and a fence of
 * one ctx may be waited for through another ctx of the same device. Every other entry point of a ctx belongs to one thread at a time. */
int paris_hip_fence_wait(paris_hip_ctx* ctx, paris_hip_fence* fence);
int paris_hip_fence_destroy(paris_hip_ctx* ctx, paris_hip_fence* fence);

/* ---- memory: make_projection_device / make_volume_device / copy_h2d / copy_d2h
 *      (src/cuda/memory.cpp:33-102, src/openmp/memory.cpp:33-79) ------------------------------------- */
/* device projection, rows padded to a 256-byte multiple; *pitch receives the row stride in bytes */
int paris_hip_malloc_projection(paris_hip_ctx* ctx, uint32_t dim_x, uint32_t dim_y, float** d_ptr, size_t* pitch);
/* device volume, zero-filled (make_volume_device semantics: src/openmp/memory.cpp:46-47) */
int paris_hip_malloc_volume(paris_hip_ctx* ctx, uint32_t dim_x, uint32_t dim_y, uint32_t dim_z, float** d_ptr);
int paris_hip_free(paris_hip_ctx* ctx, void* d_ptr);
/* pinned host memory for projection/volume host buffers (cuda: pinned_host_ptr).
 * Projection-sized buffers (host ones up to 64 MiB) are recycled: paris_hip_free / paris_hip_free_host return at once, and the
 * buffer is handed out again only after the work of THIS API that used it has finished -- a pinned buffer after the last copy from /
 * into it (an upload-stream copy does not wait for anything queued on the ctx stream), a device buffer after everything queued on
 * the ctx stream when it was released. Work the CALLER enqueues itself on a pinned buffer (its own hipMemcpyAsync) is not seen:
 * finish it (paris_hip_ctx_synchronize, a fence) before releasing that buffer. */
int paris_hip_malloc_host(paris_hip_ctx* ctx, size_t bytes, void** h_ptr);
int paris_hip_free_host(paris_hip_ctx* ctx, void* h_ptr);
/* 2-D copies, pitches in bytes; projection rows are dim_x floats */
int paris_hip_memcpy_projection_h2d(paris_hip_ctx* ctx, float* d_dst, size_t d_pitch, const float* h_src,
                                    size_t h_pitch, uint32_t dim_x, uint32_t dim_y);
/* Extension: the same host -> device copy on a dedicated upload stream of the ctx, with the compute stream made to wait
 * for it (hipStreamWaitEvent): the transfer overlaps kernels already queued. Use pinned host memory, and do not
 * refill h_src or overwrite d_dst before the work that reads them has passed a fence; at most 16 uploads in flight. An upload into
 * a buffer of paris_hip_malloc_projection that no call of this API has touched since it was handed out starts at once, whatever the
 * compute stream still holds: work the CALLER enqueued on such a buffer itself (own kernels on the ctx stream) must be complete
 * before the upload -- the library sees only its own entry points. */
int paris_hip_upload_projection(paris_hip_ctx* ctx, float* d_dst, size_t d_pitch, const float* h_src, size_t h_pitch,
                                uint32_t dim_x, uint32_t dim_y);
/* Extension: paris_hip_upload_projection for frames in the detector's stored pixel type: the copy carries s bytes per pixel
 * (1, 2 or 4) instead of 4, and in stream order the dim_x floats of every row of d_dst then hold exactly static_cast<float>(v) of the
 * stored pixels -- bit for bit what the fp32 upload leaves after the host's conversion (u32: round to nearest even; f32: a bit copy,
 * NaN payloads, -0 and denormals included). No staging memory: each stored row goes into the tail of its own float row (bytes
 * [(4 - s) * dim_x, 4 * dim_x)) and a kernel on the ctx stream widens it in place; bytes past 4 * dim_x of a row are not written.
 * h_pitch is in bytes. PARIS_HIP_ERROR_INVALID_ARGUMENT for an unknown pixel type (f64 included: convert it on the host), d_pitch <
 * 4 * dim_x or not a multiple of 4, h_pitch < s * dim_x, or null pointers. Same ordering rules as paris_hip_upload_projection. */
#define PARIS_HIP_PIXEL_U8 1
#define PARIS_HIP_PIXEL_U16 2
#define PARIS_HIP_PIXEL_U32 3
#define PARIS_HIP_PIXEL_F32 4
int paris_hip_upload_projection_raw(paris_hip_ctx* ctx, float* d_dst, size_t d_pitch, const void* h_src, size_t h_pitch,
                                    uint32_t dim_x, uint32_t dim_y, int pixel_type);
int paris_hip_memcpy_projection_d2h(paris_hip_ctx* ctx, float* h_dst, size_t h_pitch, const float* d_src,
                                    size_t d_pitch, uint32_t dim_x, uint32_t dim_y);
int paris_hip_memcpy_volume_h2d(paris_hip_ctx* ctx, float* d_dst, const float* h_src, uint32_t dim_x,
                                uint32_t dim_y, uint32_t dim_z);
int paris_hip_memcpy_volume_d2h(paris_hip_ctx* ctx, float* h_dst, const float* d_src, uint32_t dim_x,
                                uint32_t dim_y, uint32_t dim_z);
int paris_hip_memset_volume(paris_hip_ctx* ctx, float* d_ptr, uint32_t dim_x, uint32_t dim_y, uint32_t dim_z);

/* ---- make_subvolume_information (src/cuda/subvolume_information.cpp:63-118) ---------------------- */
/* Splits dim_z into `num` slabs (+ remainder on the last) so that (volume + 10 projections) / devices fits in the free
 * memory of each of `n_devices` devices, doubling the slab count until it does. n_devices <= 0: all visible devices. */
int paris_hip_make_subvolume_information(const paris_volume_geometry* vol_geo,
                                         const paris_detector_geometry* det_geo, int n_devices,
                                         paris_subvolume_info* out);
/* Extension: the same rule for a driver that keeps `reserve_bytes` of its own buffers per device beside the slab (upload
 * slots, half-precision copies, the deferral ring): a slab plus max(reserve_bytes, the reference's 10-projection allowance)
 * must fit. hipErrorOutOfMemory when reserve_bytes alone does not fit a device. */
int paris_hip_make_subvolume_information_reserving(const paris_volume_geometry* vol_geo,
                                                   const paris_detector_geometry* det_geo, int n_devices,
                                                   size_t reserve_bytes, paris_subvolume_info* out);
/* Extension: free and total memory of a device handle (hipMemGetInfo), for sizing driver buffers before planning. */
int paris_hip_device_memory(int device, size_t* free_bytes, size_t* total_bytes);

/* ---- weighting: backend::weight (src/openmp/weighting.cpp:32-57, src/cuda/weighting.cu:62-73) ---- */
/* p[t][s] *= d_sd / sqrt(d_sd^2 + h_s^2 + v_t^2), h_s = l_px_row/2 + s*l_px_row + h_min, v_t likewise.
 * IEEE sqrt and divide: bit-identical to the OpenMP backend. */
int paris_hip_weight(paris_hip_ctx* ctx, float* d_p, size_t pitch, uint32_t dim_x, uint32_t dim_y, float h_min,
                     float v_min, float d_sd, float l_px_row, float l_px_col);

/* Extension (f4): the same weighting restricted to rows [row_first, row_first + row_count) of the dim_y-row projection
 * at d_p; row t keeps its own v_t, so the band is bit-identical to the same rows of a full paris_hip_weight. */
int paris_hip_weight_rows(paris_hip_ctx* ctx, float* d_p, size_t pitch, uint32_t dim_x, uint32_t dim_y,
                          uint32_t row_first, uint32_t row_count, float h_min, float v_min, float d_sd,
                          float l_px_row, float l_px_col);

/* ---- filtering: backend::make_filter / apply_filter (src/openmp/filtering.cpp:139-219,
 *      src/cuda/filtering.cu:172-261) --------------------------------------------------------------- */
/* K = tau * |rFFT_size(r)| with r the band-limited ramp of src/openmp/filtering.cpp:52-73. *d_k receives a
 * device buffer of size/2+1 floats (the reference stores the same value in re and im of a complex; the
 * product is identical) owned by the caller: release with paris_hip_free. size must be a
 * power of two in [8, 16384]. */
int paris_hip_make_filter(paris_hip_ctx* ctx, uint32_t size, float tau, float** d_k);
/* Extension: the same K multiplied by a window. The reference implements the ramp only;
 * PARIS_HIP_WINDOW_SHEPP_LOGAN multiplies bin f by sinc(pi f / size) (1 at DC, 2/pi at Nyquist). */
#define PARIS_HIP_WINDOW_RAMP 0
#define PARIS_HIP_WINDOW_SHEPP_LOGAN 1
int paris_hip_make_filter_windowed(paris_hip_ctx* ctx, uint32_t size, float tau, int window, float** d_k);
/* Selects the window of the K that paris_hip_stage_filter builds and caches (default: the reference's ramp). */
int paris_hip_set_filter_window(paris_hip_ctx* ctx, int window);
/* In place, per detector row: zero-pad to filter_size, FFT, multiply by K, inverse FFT, keep the first dim_x
 * samples, divide by filter_size. n_col is the number of rows (== dim_y; kept because the reference passes
 * it, src/filtering.cpp:44). */
int paris_hip_apply_filter(paris_hip_ctx* ctx, float* d_p, size_t pitch, uint32_t dim_x, uint32_t dim_y,
                           const float* d_k, uint32_t filter_size, uint32_t n_col);

/* Row-filter kernel: 0 = default (filter_size >= 1024 and a K of paris_hip_make_filter*: radix-16 register passes with
 * table twiddles, the kernel that can also weight in its load; radix-2 below 1024), 1 = the radix-2 kernel for every size,
 * 2 = the first radix-16 kernel (twiddles formed per stage; experiments build only: paris_hip_has_experiments, else
 * PARIS_HIP_ERROR_UNSUPPORTED). A K this ctx did not make runs the radix-2 kernel. Same transform; results differ by fp32 rounding only. */
int paris_hip_set_filter_variant(paris_hip_ctx* ctx, int variant);

/* Extension: stage fusion. With enable != 0 a paris_hip_weight / paris_hip_weight_rows call is held back, and the
 * paris_hip_apply_filter call that follows on the same rows runs ONE kernel that applies the weight as it loads the row
 * (same operations, each rounded once: the transform sees the bits the separate weighting would have stored) -- one launch
 * and 8 instead of 16 bytes of memory traffic per pixel for PARIS's unchanged weight(); filter() call pair
 * (src/main.cpp:102-103). Every other entry point that reads, writes, frees or waits for device data first runs a held-back
 * weighting as its own kernel, so results never depend on the switch; only work the CALLER enqueues on the ctx stream between
 * the two calls would see the rows unweighted. Off by default in the C library (reference behaviour call by call), switched
 * on by paris::hip (C++ mirror) and bench.py. Ignored under PARIS_HIP_CTX_SYNCHRONOUS. */
int paris_hip_set_stage_fusion(paris_hip_ctx* ctx, int enable);

/* Extension: tiles no ray reaches. Where none of a projection's rays reaches any voxel column of a wave's tile -- the corners of
 * the grid outside the field of view, slices above / below the cone on the source side: about a tenth of a 2048^3 launch at the
 * natural grid -- the reference adds 0.5 * 0 * u * u = +0 to every voxel (src/openmp/backprojection.cpp:71,140). Adding +0 changes
 * a float only if it is -0, and a volume that paris_hip_malloc_volume allocated (zero-filled) and that nothing but backprojections
 * wrote since cannot hold one (a sum is -0 only if both terms are). For such volumes, with enable != 0 (the default), those waves
 * neither load nor store their tile; the result is bit-identical. Volumes the library did not allocate, and volumes a
 * paris_hip_memcpy_volume_h2d wrote into, always take every addition. */
int paris_hip_set_backproject_skip_invalid(paris_hip_ctx* ctx, int enable);
/* The library learns of writes into a volume only through its own entry points. A caller that writes one some other way -- its own
 * kernel, a torch tensor over the same memory -- and may have stored a -0 says so with paris_hip_volume_mark_dirty: every volume
 * that overlaps [d_ptr, d_ptr + bytes) takes every addition from then on (until a paris_hip_memset_volume covers it whole again).
 * paris_hip_volume_mark_clean is the opposite promise, for ANY device memory, the caller's own included: the range holds no -0
 * right now (freshly zero-filled; written by nothing but backprojections since) and the caller will mark it dirty before writing
 * anything else into it -- and before releasing memory the library did not allocate: the entry is keyed by address and would vouch
 * for whatever is mapped there next. Writing zeros (hipMemset, tensor.zero_()) needs neither call. */
int paris_hip_volume_mark_dirty(paris_hip_ctx* ctx, const void* d_ptr, size_t bytes);
int paris_hip_volume_mark_clean(paris_hip_ctx* ctx, const void* d_ptr, size_t bytes);
/* For memory whose history the caller does not know (a tensor handed in from elsewhere): reads [d_ptr, d_ptr + bytes) once on the
 * device (bytes a multiple of 4, about 5 ms for 32 GiB), stores the number of -0 words found in *negative_zeros (may be NULL) and
 * lists the range as clean when there is none; when there is one the range takes every addition, as if marked dirty. The same
 * duty as after paris_hip_volume_mark_clean holds from then on. Synchronises the ctx stream. */
int paris_hip_volume_scan_clean(paris_hip_ctx* ctx, const void* d_ptr, size_t bytes, uint64_t* negative_zeros);

/* Extension: weighting and row filter of rows [row_first, row_first + row_count) in one launch, explicitly. d_half != NULL:
 * the filtered rows are stored as IEEE half (round to nearest even) into d_half (same row numbering, half_pitch bytes per
 * row) and the fp32 rows stay as they were (BASELINE config 5: saves the conversion pass). d_k must come from
 * paris_hip_make_filter* on this ctx and filter_size must be >= 1024: PARIS_HIP_ERROR_UNSUPPORTED otherwise. */
int paris_hip_weight_filter_rows(paris_hip_ctx* ctx, float* d_p, size_t pitch, uint32_t dim_x, uint32_t dim_y,
                                 uint32_t row_first, uint32_t row_count, float h_min, float v_min, float d_sd,
                                 float l_px_row, float l_px_col, const float* d_k, uint32_t filter_size, uint16_t* d_half,
                                 size_t half_pitch);

/* Extension: the same for a GROUP of n_frames projections in one launch: frame f starts frame_stride bytes behind frame f - 1
 * (>= pitch * dim_y: frames must not overlap; d_half likewise, half_frame_stride bytes apart). For a driver that holds a group of
 * uploaded frames before a paris_hip_backproject_batch: with small detectors a launch per frame is mostly launch latency.
 * Bit-identical to n_frames paris_hip_weight_filter_rows calls. n_frames <= 65535. */
int paris_hip_weight_filter_batch(paris_hip_ctx* ctx, float* d_p, size_t pitch, size_t frame_stride, uint32_t n_frames, uint32_t dim_x,
                                  uint32_t dim_y, uint32_t row_first, uint32_t row_count, float h_min, float v_min, float d_sd,
                                  float l_px_row, float l_px_col, const float* d_k, uint32_t filter_size, uint16_t* d_half,
                                  size_t half_pitch, size_t half_frame_stride);

/* ---- backprojection: backend::backproject (src/openmp/backprojection.cpp:156-199,
 *      src/cuda/backprojection.cu:133-243) ---------------------------------------------------------- */
/* Adds one filtered projection into the (sub)volume d_v of v_dim_x*v_dim_y*v_dim_z voxels whose first
 * slice is global slice v_offset (+ roi->z1 when enable_roi). Voxel-driven, bilinear, zero unless all four
 * neighbours lie inside the detector (OpenMP rule, src/openmp/backprojection.cpp:52-84); every fp32
 * operation is rounded once in the reference's order, so the result is bit-identical to the OpenMP
 * backend's for the same input. sin/cos/delta_s/delta_t are what the wrapper src/backprojection.cpp:49-68
 * derives (delta_* in mm). */
int paris_hip_backproject(paris_hip_ctx* ctx, const float* d_p, size_t p_pitch, uint32_t p_dim_x,
                          uint32_t p_dim_y, float* d_v, uint32_t v_dim_x, uint32_t v_dim_y, uint32_t v_dim_z,
                          uint32_t v_offset, const paris_detector_geometry* det_geo,
                          const paris_volume_geometry* vol_geo, int enable_roi,
                          const paris_region_of_interest* roi, float sin_phi, float cos_phi, float delta_s,
                          float delta_t);

/* Extension (no reference counterpart; BASELINE config 5 "fp16-in / fp32-accum"): the filtered projection is stored
 * as IEEE half (p_pitch in bytes, >= 2*p_dim_x); pixels are widened to fp32 exactly when they are staged and every
 * operation afterwards is the fp32 one of paris_hip_backproject, so the result equals paris_hip_backproject on the
 * half-rounded projection, bit for bit. paris_hip_convert_projection_f16 rounds to nearest even. */
int paris_hip_convert_projection_f16(paris_hip_ctx* ctx, const float* d_src, size_t src_pitch, uint16_t* d_dst,
                                     size_t dst_pitch, uint32_t dim_x, uint32_t dim_y);
int paris_hip_backproject_f16(paris_hip_ctx* ctx, const uint16_t* d_p, size_t p_pitch, uint32_t p_dim_x,
                              uint32_t p_dim_y, float* d_v, uint32_t v_dim_x, uint32_t v_dim_y, uint32_t v_dim_z,
                              uint32_t v_offset, const paris_detector_geometry* det_geo,
                              const paris_volume_geometry* vol_geo, int enable_roi,
                              const paris_region_of_interest* roi, float sin_phi, float cos_phi, float delta_s,
                              float delta_t);

/* Extension (no reference counterpart): backprojects n_proj projections per launch (fused kernel, up to 64 per
 * launch, more are split); projection i is at d_p + i * p_stride_bytes. Every voxel's sum is accumulated in
 * projection order in registers, so the result is bit-identical to n_proj successive paris_hip_backproject calls
 * while the volume is read and written once per launch: 8 / n_proj bytes of HBM traffic per voxel-update. Any volume
 * width and alignment; n_proj == 1 is the single-projection kernel. */
int paris_hip_backproject_batch(paris_hip_ctx* ctx, const float* d_p, size_t p_pitch, size_t p_stride_bytes,
                                uint32_t n_proj, uint32_t p_dim_x, uint32_t p_dim_y, float* d_v,
                                uint32_t v_dim_x, uint32_t v_dim_y, uint32_t v_dim_z, uint32_t v_offset,
                                const paris_detector_geometry* det_geo, const paris_volume_geometry* vol_geo,
                                int enable_roi, const paris_region_of_interest* roi, const float* sin_phi,
                                const float* cos_phi, float delta_s, float delta_t);

/* The same for IEEE-half projections (paris_hip_backproject_f16 semantics; p_pitch / p_stride_bytes in bytes of half rows). */
int paris_hip_backproject_batch_f16(paris_hip_ctx* ctx, const uint16_t* d_p, size_t p_pitch, size_t p_stride_bytes,
                                    uint32_t n_proj, uint32_t p_dim_x, uint32_t p_dim_y, float* d_v, uint32_t v_dim_x,
                                    uint32_t v_dim_y, uint32_t v_dim_z, uint32_t v_offset,
                                    const paris_detector_geometry* det_geo, const paris_volume_geometry* vol_geo,
                                    int enable_roi, const paris_region_of_interest* roi, const float* sin_phi,
                                    const float* cos_phi, float delta_s, float delta_t);

/* Extension: deferred backprojection. With depth n > 1 (n <= 64), paris_hip_backproject (and paris_hip_backproject_f16:
 * half-precision calls form groups of their own) copies its projection into a ring
 * owned by the ctx (stream-ordered device-to-device copy: the caller may reuse its buffer as after any asynchronous
 * call) and returns; the pending projections are added by ONE fused launch, in call order and bit-identical to n
 * single launches, when n are pending, when a call with another volume, slab, geometry or ROI arrives, and before
 * every entry point that observes or changes a volume, completes work or changes how backprojection runs
 * (paris_hip_ctx_synchronize, _fence_record, _memcpy_volume_*, _memset_volume, _free, _backproject_batch, a call of the
 * other precision, the timing and tuning calls, paris_hip_flush). The volume is then read and written once per n projections instead of
 * once per projection. Two caveats: work the caller enqueues on the ctx's stream OUTSIDE this API does not see deferred
 * projections (call paris_hip_flush first), and paris_hip_ctx_destroy runs what is still pending only into a volume that
 * paris_hip_malloc_volume of this ctx allocated and paris_hip_free has not taken back (pending projections of any other volume
 * are dropped: the library cannot know whether that address still belongs to the caller). Depth 1 (the
 * default) is immediate execution. The C++ mirror paris::hip enables depth 48, so PARIS's unchanged per-projection loop
 * (src/main.cpp:98-105) runs at the fused kernel's rate. */
int paris_hip_set_backproject_deferral(paris_hip_ctx* ctx, uint32_t depth);
/* (The first groups of a sequence of calls into one volume are launched early -- after 8, 16 and 32 calls, then every `depth` -- so
 * that the device starts while the caller is still feeding the first full group; a call with other arguments, or a change of the
 * depth, starts a new sequence.) */
int paris_hip_flush(paris_hip_ctx* ctx);
/* Extension: deferral BY REFERENCE. With enable != 0 a deferred paris_hip_backproject[_f16] whose projection is a whole buffer of
 * paris_hip_malloc_projection (the pointer it returned, its pitch) takes NO snapshot: the group's fused launch reads the buffer
 * itself. The library answers for such a buffer until that launch has been made: paris_hip_free of it returns at once and the
 * buffer goes back to the pool behind the launch (one event per group instead of one per buffer, no copy enqueued per call); any
 * other entry point that reads or writes the buffer -- a second weighting or filter, an upload into it, a copy to the host --
 * launches the pending group first, so every result is what the snapshot would have given, bit for bit. With filter deferral
 * the held-back weight + filter of such a projection runs IN PLACE in the group's one filter launch: the buffer holds the filtered
 * pixels whenever anything looks at it through this API. The one thing the library cannot see is work the caller enqueues on
 * the ctx stream by itself: a caller whose own kernels write projection buffers after backprojecting them leaves this off (the
 * default; snapshots). Projections in memory the library did not allocate, row-band pointers into a buffer, other pitches and
 * calls made while a caller-supplied ctx stream is being captured into a graph are snapshotted as before (a group may mix both).
 * A caller that REFILLS one buffer for every projection gains nothing from it -- each refill finds the buffer referenced and launches
 * the pending group, one projection per launch -- and keeps the snapshots. paris::hip switches it on: PARIS's loop
 * (src/main.cpp:98-105) allocates, fills, backprojects and frees one buffer per projection (src/loader.cpp:28-33) and touches
 * nothing outside the backend. */
int paris_hip_set_backproject_references(paris_hip_ctx* ctx, int enable);
/* What this ctx may keep allocated for projections of dim_x x dim_y pixels beside the volume, with its present deferral settings (the
 * rotation of paris_hip_malloc_projection buffers, the pending group's buffers or the snapshot ring): the reserve_bytes a driver
 * passes to paris_hip_make_subvolume_information_reserving. */
int paris_hip_projection_reserve_bytes(paris_hip_ctx* ctx, uint32_t dim_x, uint32_t dim_y, size_t* bytes);
/* How many projections are pending right now and into which volume (NULL when none): what a wrapper that lends the library memory
 * it does not own needs to decide whether a last paris_hip_flush is still safe (paris_amd.backend.Backend.close). */
int paris_hip_pending_backprojections(paris_hip_ctx* ctx, uint32_t* count, void** d_v);
/* Extension: filter deferral, for small projections whose weight + filter launch is mostly latency (512^2: 7 us alone, 0.9 us as one
 * of 48 in a group launch). With enable != 0, stage fusion on and a deferral depth > 1, the paris_hip_apply_filter call that
 * follows a held-back weighting of the same rows is held back as well. If the NEXT call backprojects that projection
 * (paris_hip_backproject into the deferral ring), the library snapshots the still unfiltered frame and runs weighting + filter on
 * its snapshots, one launch for the whole group, right before the group's fused backprojection: the volume is bit-identical. Any
 * other entry point runs the held-back launch first, in place, as if it had never been held. The one thing that changes: after
 * such a backprojection the caller's projection buffer still holds the UNFILTERED pixels (PARIS's loop, src/main.cpp:98-105,
 * never looks at a projection again after backprojecting it; a caller that does leaves this off). Off by default in the bare
 * library. enable == 2 holds a filter back ONLY where nobody can tell: with deferral by reference on
 * (paris_hip_set_backproject_references) and a projection that is a whole buffer of paris_hip_malloc_projection -- the filter then
 * runs IN PLACE in the group's one filter launch and every other call that touches the buffer runs it first, so the buffer holds
 * the filtered pixels whenever anything looks at it through this API; everything else is filtered at once. That is what the C++
 * mirror paris::hip switches on (macro PARIS_HIP_FILTER_DEFERRAL = 2): one filter launch per group instead of one per projection
 * (config 1 through PARIS's loop: profiles/r05_demo_paris_hip_mirror.txt). */
int paris_hip_set_filter_deferral(paris_hip_ctx* ctx, int enable);
/* Extension: asynchronous validation. The hand-expanded IEEE sequences (fast division by the pixel pitch, shared-reciprocal
 * divisions, short sqrt / divide of the weighting) are used only after a device validator has proved them for the operands at hand,
 * once per process, device and operand range; by default the call that needs an answer first waits for the validator (2.3 ms for
 * the exhaustive check of a pixel pitch). With enable != 0 that call launches the validator on the ctx's auxiliary stream and
 * goes on with the compiler's IEEE forms -- the same bits, a few instructions more per voxel column -- until a later call finds
 * the answer there. Results never depend on it; paris_hip_fast_division_is_exact and the paris_hip_lean_*_is_exact queries always
 * wait. Off by default in the bare library (which kernel form a given launch uses then depends on timing), on in paris::hip. */
int paris_hip_set_async_validation(paris_hip_ctx* ctx, int enable);
/* Where the fused launch of a full group runs: with enable != 0 on a second stream of the ctx, ordered behind the
 * group's snapshot copies, so that the uploads, weightings and filters of the NEXT group -- which the caller keeps enqueuing on
 * the ctx stream -- execute beside it instead of behind it (what small volumes need: a 256^3 launch of 16 projections takes about
 * as long as the sixteen copy + filter launches of the next group). Every entry point that flushes (see above) also makes the ctx
 * stream wait for the launches on the second stream, so the caller sees one stream's worth of ordering. Not used under
 * PARIS_HIP_CTX_SYNCHRONOUS or while the ctx stream is being captured into a graph. Results never depend on it. Off by default in
 * the bare library; the C++ mirror paris::hip switches it on (macro PARIS_HIP_BACKPROJECT_OVERLAP): PARIS's loop uploads, filters and
 * snapshots the next group while a launch runs, and without the second stream all of that -- and the release of every buffer of
 * the loop -- queues behind the launch: whole circles through the mirror 1.65 -> 1.97 TVox/s at 2048^2, 1.30 -> 1.90 at 1024^2,
 * 0.88 -> 1.78 at 512^2 (profiles/r04_demo_paris_hip_mirror.txt; a call with the same arguments as the group launched last
 * continues without joining the streams -- until round 4 every group's first call joined, and nothing overlapped). With the
 * projections already resident on the device there is nothing to pass and the switch changes nothing (bench.py --overlap). */
int paris_hip_set_backproject_overlap(paris_hip_ctx* ctx, int enable);

/* ---- stage wrappers and geometry (host code of the hot path) ----------------------------------------
 * The reference derives the kernels' scalar arguments in backend-neutral wrappers and caches them in
 * function-local statics; these entry points restate them per call (no statics). */
/* calculate_volume_geometry (src/geometry.cpp:36-84) */
int paris_hip_calculate_volume_geometry(const paris_detector_geometry* det_geo, paris_volume_geometry* out);
/* apply_roi (src/geometry.cpp:86-130); an invalid ROI returns the input geometry, as the reference does */
int paris_hip_apply_roi(const paris_volume_geometry* vol_geo, const paris_region_of_interest* roi,
                        paris_volume_geometry* out);
/* paris::weight (src/weighting.cpp:32-45): derives h_min, v_min, d_sd and calls paris_hip_weight */
int paris_hip_stage_weight(paris_hip_ctx* ctx, float* d_p, size_t pitch, uint32_t dim_x, uint32_t dim_y,
                           const paris_detector_geometry* det_geo);
/* filter_size = 2 * 2^ceil(log2(n_row)) (src/filtering.cpp:37) */
uint32_t paris_hip_filter_size(uint32_t n_row);
/* paris::filter (src/filtering.cpp:32-45): builds K once per ctx, then paris_hip_apply_filter */
int paris_hip_stage_filter(paris_hip_ctx* ctx, float* d_p, size_t pitch, uint32_t dim_x, uint32_t dim_y,
                           const paris_detector_geometry* det_geo);
/* Extensions (f4): the two wrappers above on rows [row_first, row_first + row_count) of the projection at d_p only. With a
 * band from paris_hip_slab_row_band (whole filter row pairs) the band's pixels are bit-identical to a full call. */
int paris_hip_stage_weight_rows(paris_hip_ctx* ctx, float* d_p, size_t pitch, uint32_t dim_x, uint32_t dim_y,
                                uint32_t row_first, uint32_t row_count, const paris_detector_geometry* det_geo);
int paris_hip_stage_filter_rows(paris_hip_ctx* ctx, float* d_p, size_t pitch, uint32_t dim_x, uint32_t dim_y,
                                uint32_t row_first, uint32_t row_count, const paris_detector_geometry* det_geo);
/* Extension: paris::weight + paris::filter of a row band in one launch (paris_hip_weight_filter_rows with the wrappers'
 * constants and cached K); d_half != NULL stores the band as IEEE half there (half_pitch bytes per row, same row numbering)
 * and leaves the fp32 rows unfiltered. Narrow detectors (filter length < 1024) run the separate stages: same result. */
int paris_hip_stage_weight_filter_rows(paris_hip_ctx* ctx, float* d_p, size_t pitch, uint32_t dim_x, uint32_t dim_y,
                                       uint32_t row_first, uint32_t row_count, const paris_detector_geometry* det_geo,
                                       uint16_t* d_half, size_t half_pitch);
/* Extension: paris_hip_stage_weight_filter_rows for a group of n_frames projections frame_stride bytes apart in one launch
 * (paris_hip_weight_filter_batch with the wrappers' constants and cached K; narrow detectors run frame by frame: same result). */
int paris_hip_stage_weight_filter_batch(paris_hip_ctx* ctx, float* d_p, size_t pitch, size_t frame_stride, uint32_t n_frames,
                                        uint32_t dim_x, uint32_t dim_y, uint32_t row_first, uint32_t row_count,
                                        const paris_detector_geometry* det_geo, uint16_t* d_half, size_t half_pitch,
                                        size_t half_frame_stride);
/* Extension (f4; no reference counterpart): the detector rows [*row_first, *row_first +
 * *row_count) that backprojecting into the slab (v_dim_*, v_offset, optional ROI; arguments as paris_hip_backproject)
 * can read for ANY projection angle. Rows outside the band never contribute to the slab, so a driver may upload,
 * weight (paris_hip_weight_rows) and filter (paris_hip_apply_filter on the band's rows) only the band and still get
 * the bit-identical volume; the projection buffer keeps its full size. The band starts on an even row and ends on an
 * odd one (or the last row): the filter transforms row pairs. Conservative: the whole detector when no bound
 * exists (source distance inside the slab's circle), *row_count = 0 when the slab never projects onto the detector. */
int paris_hip_slab_row_band(const paris_detector_geometry* det_geo, const paris_volume_geometry* vol_geo,
                            uint32_t v_dim_x, uint32_t v_dim_y, uint32_t v_dim_z, uint32_t v_offset, int enable_roi,
                            const paris_region_of_interest* roi, uint32_t* row_first, uint32_t* row_count);
/* angle of projection idx -> sin/cos on the host in fp32 (src/backprojection.cpp:52-63) */
int paris_hip_stage_angle(const paris_detector_geometry* det_geo, uint32_t idx, int enable_angles, float phi,
                          float* sin_phi, float* cos_phi);

/* Extension (no reference counterpart): short scans. A scan covers the projection angles [start_deg, start_deg + range_deg]
 * -- the angle the backprojection uses, idx * delta_phi or phi with angles enabled -- and is valid when
 * 180 + 2 gamma_m <= range_deg <= 360, gamma_m the largest |fan angle| atan(t / d_sd) over the two outermost pixel centres in the
 * backprojector's coordinates, t = (i + 1/2) l_px_row - n_row l_px_row / 2 - delta_s l_px_row (delta_s included). */
typedef struct paris_short_scan {
    float start_deg;  /* first projection angle [deg] */
    float range_deg;  /* angle covered from the first to the last projection [deg] */
} paris_short_scan;
/* Host only. PARIS_HIP_ERROR_INVALID_ARGUMENT when range_deg < 180 + 2 gamma_m, range_deg > 360, or a value is not finite.
 * gamma_max_deg (may be NULL) receives gamma_m in degrees, for refused scans too. */
int paris_hip_short_scan_check(const paris_detector_geometry* det_geo, const paris_short_scan* scan, float* gamma_max_deg);
/* Parker redundancy weighting: every row in [row_first, row_first + row_count) of n_frames projections frame_stride bytes apart
 * has column i multiplied by 2 w(beta, gamma_i), beta = (phi_deg[f] - start_deg) mod 360 (DESIGN.md "Short scans"); the 2 cancels
 * the backprojection's 0.5, so the volume has the full circle's scale. Where w == 1 the pixel becomes exactly 2 p. Call it on the
 * raw frame, before the cosine weighting; dim_x must equal det_geo->n_row. Runs the check above. */
int paris_hip_short_scan_weight_rows(paris_hip_ctx* ctx, float* d_p, size_t pitch, size_t frame_stride, uint32_t n_frames,
                                     uint32_t dim_x, uint32_t dim_y, uint32_t row_first, uint32_t row_count,
                                     const paris_detector_geometry* det_geo, const paris_short_scan* scan, const float* phi_deg);
/* The same for one whole projection, its angle resolved from idx / phi exactly as paris_hip_stage_angle does */
int paris_hip_stage_short_scan_weight(paris_hip_ctx* ctx, float* d_p, size_t pitch, uint32_t dim_x, uint32_t dim_y,
                                      const paris_detector_geometry* det_geo, const paris_short_scan* scan, uint32_t idx,
                                      int enable_angles, float phi);
/* Extension (no reference counterpart): offset detectors (half fan, extended field of view) over a full circle. The detector is
 * shifted sideways (delta_s) so that it covers the rotation axis and one side further than the other; in the backprojector's
 * coordinates it spans [-t_half, n_row l - t_half], t_half = n_row l / 2 + delta_s l, l = l_px_row, and the rays within the overlap
 * |t| < tau = min(t_half, n_row l - t_half) = (n_row / 2 - |delta_s|) l are measured twice per circle, the others once.
 * Host only. gamma_tau_deg (may be NULL) receives the overlap half-angle atan(tau / d_sd) in degrees, for refused geometries too.
 * PARIS_HIP_ERROR_INVALID_ARGUMENT when tau < 2 l (the central ray misses the detector or lies within 2 pixels of its edge), for
 * n_row == 0, l_px_row <= 0, d_sd = |d_so| + |d_od| <= 0 or a value that is not finite. A centred detector is accepted: the weight
 * is valid there, only pointless. */
int paris_hip_offset_detector_check(const paris_detector_geometry* det_geo, float* gamma_tau_deg);
/* Wang's redundancy weighting: every row in [row_first, row_first + row_count) of n_frames projections frame_stride bytes apart has
 * column i multiplied by 2 w(x_i), x_i = sigma gamma_i / gamma_tau, gamma_i = atan(t_i / d_sd), sigma = +1 for delta_s <= 0 and -1
 * otherwise: 2 w = 2 for x >= 1, 2 sin^2(pi/4 (1 + x)) for -1 < x < 1, 0 for x <= -1 (DESIGN.md "Offset detectors"). Columns at t and
 * -t add up to 2; beyond the overlap a pixel becomes exactly 2 p. The weight does not depend on the angle. Call it on the raw frame
 * of a full-circle scan, before the cosine weighting; dim_x must equal det_geo->n_row. Runs the check above. */
int paris_hip_offset_detector_weight_rows(paris_hip_ctx* ctx, float* d_p, size_t pitch, size_t frame_stride, uint32_t n_frames,
                                          uint32_t dim_x, uint32_t dim_y, uint32_t row_first, uint32_t row_count,
                                          const paris_detector_geometry* det_geo);
/* The same for one whole projection */
int paris_hip_stage_offset_detector_weight(paris_hip_ctx* ctx, float* d_p, size_t pitch, uint32_t dim_x, uint32_t dim_y,
                                           const paris_detector_geometry* det_geo);
/* Extension (no reference counterpart): dark / flat ("offset / gain") correction of intensity frames to line integrals. With I a
 * pixel as fp32 and D, F the dark and flat reference pixels of the same detector row and column, in double, rounded once:
 *   p = -ln(max((I - D) / (F - D), t_min))   when I, D and F are finite and F - D > 0,   p = 0 otherwise (dead pixel).
 * There is no upper clamp: noise may make p negative.
 * paris_hip_set_flat_field copies the two dim_x x dim_y frames (rows dim_x floats apart; h_dark NULL = zeros) into memory the ctx
 * owns, replacing an earlier setting; the old frames are freed once the work queued before the call no longer reads them.
 * PARIS_HIP_ERROR_INVALID_ARGUMENT for a NULL h_flat, a zero dimension, or t_min outside (0, 1]. The frames count towards
 * paris_hip_projection_reserve_bytes while set; paris_hip_ctx_destroy frees them. Without a setting nothing else changes. */
int paris_hip_set_flat_field(paris_hip_ctx* ctx, const float* h_dark, const float* h_flat, uint32_t dim_x, uint32_t dim_y, float t_min);
int paris_hip_clear_flat_field(paris_hip_ctx* ctx);
/* In place on float frames: rows [row_first, row_first + row_count) of n_frames frames frame_stride bytes apart, d_p the first
 * frame's row 0, each pixel corrected with the reference pixel of its own row. PARIS_HIP_ERROR_INVALID_ARGUMENT without a setting,
 * when dim_x / dim_y differ from the setting's, or for a band, pitch or stride the short-scan pass would refuse. */
int paris_hip_flat_field_rows(paris_hip_ctx* ctx, float* d_p, size_t pitch, size_t frame_stride, uint32_t n_frames, uint32_t dim_x,
                              uint32_t dim_y, uint32_t row_first, uint32_t row_count);
/* paris_hip_upload_projection_raw of rows [row_first, row_first + row_count) -- h_src points at the band's first stored row,
 * d_frame at the full frame's row 0 -- widened and corrected in one pass on the device: bit for bit the raw upload into those rows
 * followed by paris_hip_flat_field_rows on them. Any pixel type of the raw upload, PARIS_HIP_PIXEL_F32 included; its ordering rules.
 * PARIS_HIP_ERROR_INVALID_ARGUMENT without a setting or when dim_x / dim_y differ from the setting's. */
int paris_hip_upload_projection_raw_corrected(paris_hip_ctx* ctx, float* d_frame, size_t d_pitch, const void* h_src, size_t h_pitch,
                                              uint32_t dim_x, uint32_t dim_y, uint32_t row_first, uint32_t row_count, int pixel_type);
/* The pixels of the current flat-field setting that are dead by the rule above whatever the frame holds -- D or F not finite, or
 * F - D <= 0 -- as dim_x * dim_y bytes (1 = dead), rows dim_x apart. Computed on the host by paris_hip_set_flat_field and kept with the
 * setting; callers OR it into the defect map they set below. PARIS_HIP_ERROR_INVALID_ARGUMENT without a setting or for a NULL mask. */
int paris_hip_flat_field_dead_pixels(paris_hip_ctx* ctx, uint8_t* mask);

/* Extension (no reference counterpart): repair of defective detector pixels (dead pixels, lines, hot pixels) on the device, after
 * the dark / flat correction and before every weight.
 * A defect map is dim_y rows of dim_x bytes at full detector size; a nonzero byte marks a defective pixel, every other pixel is good.
 * For a defective pixel q = (x, y):
 *   r_q     = the smallest r in 1 .. PARIS_HIP_DEFECT_R_MAX for which some good pixel inside the detector has Chebyshev distance
 *             max(|dx|, |dy|) <= r from q;
 *   sources = all good pixels within that distance -- by the choice of r_q they all lie on ring r_q, at most 8 r_q of them -- in
 *             row-major order;
 *   w_k     = (1 / d_k^2) / sum_j (1 / d_j^2), d^2 = dx^2 + dy^2, formed in double on the host when the map is set and rounded once
 *             to fp32;
 *   value   = acc = 0; for k in order: acc = fmaf(w_k, p_k, acc), in fp32.
 * A defective pixel with no good pixel within PARIS_HIP_DEFECT_R_MAX is unrepairable: it is left as it is, and counted.
 * Sources are good pixels only and only defective pixels are written, so the pass runs in place without races, and running it twice
 * gives the bits of running it once. A pixel that is bad in one frame only (a NaN in an f32 frame) is no map defect: it stays 0
 * as the dark / flat correction leaves it. */
#define PARIS_HIP_DEFECT_R_MAX 8
typedef struct paris_hip_defect_stats {
    uint64_t defects;      /* pixels the map marks */
    uint64_t unrepairable; /* of those, pixels with no good pixel within PARIS_HIP_DEFECT_R_MAX */
    uint64_t sources;      /* source entries over all repairable defects */
    uint32_t reach_rows;   /* the largest |dy| any source has */
    uint32_t reach_cols;   /* the largest |dx| any source has */
    uint64_t device_bytes; /* what the plan occupies on the device while set (0 for a plan without a repairable defect) */
} paris_hip_defect_stats;
/* The plan of a map, on the host alone (no device, no ctx): the only implementation of the rule above. dim_x * dim_y and the number
 * of sources must each fit 32 bits (PARIS_HIP_ERROR_UNSUPPORTED). PARIS_HIP_ERROR_INVALID_ARGUMENT for a NULL pointer or a zero
 * dimension. */
typedef struct paris_hip_defect_plan paris_hip_defect_plan;
int paris_hip_defect_plan_create(const uint8_t* mask, uint32_t dim_x, uint32_t dim_y, paris_hip_defect_plan** out);
int paris_hip_defect_plan_destroy(paris_hip_defect_plan* plan);
int paris_hip_defect_plan_stats(const paris_hip_defect_plan* plan, paris_hip_defect_stats* out);
/* The plan as CSR arrays, n = defects - unrepairable, m = sources: defect_index[n] the linear index y * dim_x + x of every repairable
 * defect, sorted row-major; first_source[n + 1]; source_index[m] and weight[m], defect k's at [first_source[k], first_source[k + 1]).
 * Any of the four may be NULL (not copied). */
int paris_hip_defect_plan_copy(const paris_hip_defect_plan* plan, uint32_t* defect_index, uint32_t* first_source, uint32_t* source_index,
                               float* weight);
/* paris_hip_set_defect_map builds the plan and copies it into memory the ctx owns, replacing an earlier setting; the old plan is
 * freed once the work queued before the call no longer reads it. A map without a defect is accepted and makes the repair a no-op.
 * PARIS_HIP_ERROR_INVALID_ARGUMENT for a NULL mask or a zero dimension. The plan's bytes count towards
 * paris_hip_projection_reserve_bytes while set; paris_hip_ctx_destroy frees them. Without a setting nothing else changes. */
int paris_hip_set_defect_map(paris_hip_ctx* ctx, const uint8_t* mask, uint32_t dim_x, uint32_t dim_y);
int paris_hip_clear_defect_map(paris_hip_ctx* ctx);
/* The stats of the current setting. PARIS_HIP_ERROR_INVALID_ARGUMENT without one. */
int paris_hip_defect_map_info(paris_hip_ctx* ctx, paris_hip_defect_stats* out);
/* In place on float frames: the repairable defects whose row lies in [row_first, row_first + row_count) of n_frames frames
 * frame_stride bytes apart, d_p the first frame's row 0, are replaced by their repaired value. Their sources may lie up to reach_rows
 * rows OUTSIDE the band (clipped to the detector): the caller guarantees that those rows of every frame hold valid pixels -- a driver
 * that processes a row band uploads and corrects the band widened by reach_rows on each side, and repairs, weights and filters the
 * band itself. Call it on line integrals, before the redundancy and cosine weights. PARIS_HIP_ERROR_INVALID_ARGUMENT without a setting,
 * when dim_x / dim_y differ from the setting's, or for a band, pitch or stride paris_hip_flat_field_rows would refuse. */
int paris_hip_defect_repair_rows(paris_hip_ctx* ctx, float* d_p, size_t pitch, size_t frame_stride, uint32_t n_frames, uint32_t dim_x,
                                 uint32_t dim_y, uint32_t row_first, uint32_t row_count);

/* Extension (no reference counterpart): removal of per-frame outlier pixels ("zingers": direct hits in the sensor, one pixel or a
 * small blob, in one frame only) on the device, after the defect repair and before every weight.
 * For pixel (x, y) with value p of a dim_x x dim_y frame:
 *   window  = the nine values at (clamp(x + dx, 0, dim_x - 1), clamp(y + dy, 0, dim_y - 1)), dx, dy in {-1, 0, 1}: edges are
 *             replicated, so there are always nine, in a 1-pixel-wide frame too; the clamp is to the FRAME, never to the band;
 *   if any of the nine is not finite, the pixel is kept as it is;
 *   m       = the 5th smallest of the nine by value (zeros of either sign compare equal; the sign of a zero result is unspecified);
 *   d = p - m,  lim = threshold_abs + threshold_rel * |m|, each operation rounded once to fp32 (a multiply, then an add);
 *   flagged = d > lim (polarity +1),  -d > lim (polarity -1),  |d| > lim (polarity 0);  a flagged pixel becomes m.
 * Every window is read from the frame AS IT WAS BEFORE THE CALL: a replaced neighbour never feeds another pixel's median, and the
 * result is a pure function of the input frame. The pass is NOT idempotent: a second call sees the first one's medians.
 * A frame (the rows of one frame one call examines) in which more than max_hits pixels are flagged is left ENTIRELY as it was and
 * counted as saturated: it means the threshold is wrong, not that the frame holds that many zingers. max_hits == 0 stands for the
 * default max(1024, dim_x * dim_y / 256), capped at dim_x * dim_y. The count is per call and band: a frame that saturates as a
 * whole may be filtered when it is processed band by band, so banded and whole-frame results agree only while neither saturates. */
typedef struct paris_hip_zinger_filter {
    float threshold_abs;   /* >= 0, frame units */
    float threshold_rel;   /* >= 0, times |median| */
    int polarity;          /* +1 bright (p above its surroundings), -1 dark (below), 0 both */
    uint32_t max_hits;     /* most pixels replaced per frame; 0 = default */
} paris_hip_zinger_filter;
/* what paris_hip_zinger_stats reports (a struct cannot share the function's name in C) */
typedef struct paris_hip_zinger_counts {
    uint64_t frames;           /* frames examined (per call: each frame of a non-empty band) */
    uint64_t replaced;         /* pixels replaced */
    uint64_t saturated_frames; /* frames left as they were because more than max_hits pixels were flagged */
} paris_hip_zinger_counts;
/* one launch serves at most this many frames; calls with more loop */
#define PARIS_HIP_ZINGER_FRAMES_MAX 64
/* Host only, no ctx and no device: checks a setting for a detector, resolves the default max_hits (max_hits may be NULL) and reports
 * what the setting occupies on the device while set (device_bytes may be NULL): three 64-bit accumulators and, per frame of one
 * launch, a hit counter and max_hits (index, value) pairs. PARIS_HIP_ERROR_INVALID_ARGUMENT for a NULL setting, a zero dimension, a
 * threshold that is negative or not finite, both thresholds zero, a polarity outside {-1, 0, 1} or max_hits > dim_x * dim_y;
 * PARIS_HIP_ERROR_UNSUPPORTED when dim_x * dim_y does not fit 32 bits. */
int paris_hip_zinger_filter_check(const paris_hip_zinger_filter* setting, uint32_t dim_x, uint32_t dim_y, uint32_t* max_hits,
                                  size_t* device_bytes);
/* paris_hip_set_zinger_filter runs the check and allocates the scratch in memory the ctx owns, replacing an earlier setting (and
 * its counts); the old scratch is freed once the work queued before the call no longer uses it. The scratch counts towards
 * paris_hip_projection_reserve_bytes while set; paris_hip_ctx_destroy frees it. Without a setting nothing else changes. */
int paris_hip_set_zinger_filter(paris_hip_ctx* ctx, const paris_hip_zinger_filter* setting, uint32_t dim_x, uint32_t dim_y);
int paris_hip_clear_zinger_filter(paris_hip_ctx* ctx);
/* In place on float frames: the pixels whose row lies in [row_first, row_first + row_count) of n_frames frames frame_stride bytes
 * apart, d_p the first frame's row 0, are examined and possibly replaced. Their windows reach one row OUTSIDE the band on either
 * side (clipped to the frame): the caller guarantees that those rows of every frame hold valid pixels. Call it on line integrals,
 * after the defect repair and before the redundancy and cosine weights. PARIS_HIP_ERROR_INVALID_ARGUMENT without a setting, when
 * dim_x / dim_y differ from the setting's, or for a band, pitch or stride paris_hip_flat_field_rows would refuse. */
int paris_hip_zinger_filter_rows(paris_hip_ctx* ctx, float* d_p, size_t pitch, size_t frame_stride, uint32_t n_frames, uint32_t dim_x,
                                 uint32_t dim_y, uint32_t row_first, uint32_t row_count);
/* The counts since the setting was made or last reset: runs what is pending, waits for the ctx stream and reads them; reset != 0
 * zeroes them afterwards. PARIS_HIP_ERROR_INVALID_ARGUMENT without a setting or for a NULL out. */
int paris_hip_zinger_stats(paris_hip_ctx* ctx, paris_hip_zinger_counts* out, int reset);
/* Extension (no reference counterpart): removal of ring artefacts -- stationary detector offsets, a small constant error a working
 * pixel carries in every frame, which FDK turns into a ring around the rotation axis. The mean of every
 * pixel over the scan is compared with a running median of that mean along the detector row; clear outliers are subtracted from
 * every frame.
 * Setting paris_hip_ring_filter { uint32_t half_width; float floor_abs; float limit_abs; }.
 *   half_width h is in [1, 32].
 *   floor_abs is >= 0 and finite.
 *   limit_abs is finite. It is either 0, which means no upper limit, or > floor_abs.
 * Profile. For pixel (x, y), S[y][x] is the sum, in DOUBLE, of the fp32 pixel values of every frame added. The order is the one in
 * which they were added: call order, and frame 0 .. n - 1 within a call.
 *   N[y] is the number of frames added for row y. Bands may differ, so the host keeps the count per row.
 *   Every pixel has one owner thread per launch, and there are no atomics. The sum is therefore reproducible and equals numpy's
 *   sequential float64 sum bit for bit.
 * Mean. mean[y][x] = (float)(S[y][x] / (double)N[y]), rounded once. Rows with N[y] == 0 have no mean and get c = 0.
 * Correction.
 *   window is the 2h + 1 values mean[y][clamp(x + d, 0, dim_x - 1)], d = -h .. h. Edges are replicated.
 *   If any value of the window is not finite, c = +0.
 *   med is the (h + 1)-th smallest value by value.
 *   c = mean - med in fp32.
 *   c is kept iff floor_abs <= |c| and (limit_abs == 0 or |c| <= limit_abs). Otherwise c = +0.
 *   A kept c that is -0 counts as 0.
 * Apply. p <- p - c[y][x], one fp32 subtraction. Pixels with c == 0 are NOT WRITTEN: their bits stay, NaN payloads included.
 * Further properties of the rule:
 *   It runs on line integrals, after the zinger filter and before the redundancy and cosine weights.
 *   The correction of a row depends on that row only, so a row band needs no extra rows.
 *   The rule for c reads one frame once per scan. It has ONE implementation, on the host (paris_hip_ring_correction_from_mean), as
 *   the defect plan and the row-extension response have.
 *   The device does the two passes that touch every frame. */
typedef struct paris_hip_ring_filter {
    uint32_t half_width; /* h: the running median spans 2h + 1 pixels of a row, 1 .. 32 */
    float floor_abs;     /* dead band: smaller |c| are not corrected; >= 0, frame units */
    float limit_abs;     /* larger |c| are not corrected; 0 = no limit, else > floor_abs */
} paris_hip_ring_filter;
typedef struct paris_hip_ring_stats {
    uint64_t corrected;   /* pixels with c != 0 */
    uint64_t below_floor; /* pixels whose |c| was below floor_abs */
    uint64_t above_limit; /* pixels whose |c| was above limit_abs */
    uint64_t not_finite;  /* pixels whose window held a value that is not finite */
    float max_abs;        /* the largest kept |c| (0 when none) */
    uint32_t frames_min;  /* the smallest and the largest N[y] over the rows; both 0 when the counts were not given */
    uint32_t frames_max;
} paris_hip_ring_stats;
/* one accumulate launch serves at most this many frames; calls with more loop */
#define PARIS_HIP_RING_FRAMES_MAX 64
/* Host only, no ctx and no device: checks a setting for a detector and reports what an open profile (8 bytes per pixel) and a
 * correction frame (4 bytes per pixel) occupy on the device; either pointer may be NULL. PARIS_HIP_ERROR_INVALID_ARGUMENT for a NULL
 * setting, a zero dimension, or a setting the rule excludes; PARIS_HIP_ERROR_UNSUPPORTED when dim_x * dim_y does not fit 32 bits. */
int paris_hip_ring_filter_check(const paris_hip_ring_filter* setting, uint32_t dim_x, uint32_t dim_y, size_t* profile_bytes,
                                size_t* correction_bytes);
/* Host only: the rule above from the mean frame (dim_y rows of dim_x floats) to c (the same shape) -- the single implementation
 * of c. count_per_row is N[y], dim_y entries; NULL stands for "every row present" (frames_min and frames_max are then 0). out may be
 * NULL. PARIS_HIP_ERROR_INVALID_ARGUMENT as the check, or for a NULL mean or c. */
int paris_hip_ring_correction_from_mean(const paris_hip_ring_filter* setting, const float* mean, const uint32_t* count_per_row,
                                        uint32_t dim_x, uint32_t dim_y, float* c, paris_hip_ring_stats* out);
/* The profile: paris_hip_ring_profile_begin opens one for dim_x x dim_y frames -- zeroed double sums in memory the ctx owns, which
 * count towards paris_hip_projection_reserve_bytes while open and are freed by finish, discard or paris_hip_ctx_destroy. begin on an
 * open profile replaces it; work queued before keeps the old one. PARIS_HIP_ERROR_INVALID_ARGUMENT for a zero dimension,
 * PARIS_HIP_ERROR_UNSUPPORTED when dim_x * dim_y does not fit 32 bits.
 * paris_hip_ring_profile_add_rows adds rows [row_first, row_first + row_count) of n_frames frames frame_stride bytes apart, d_p the
 * first frame's row 0, to the sums, and n_frames to N[y] of those rows; the frames are only read. A held-back weighting runs first,
 * and a frame of the pending by-reference group has that group launched first. PARIS_HIP_ERROR_INVALID_ARGUMENT without an open
 * profile, when dim_x / dim_y differ from the profile's, or for a band, pitch or stride paris_hip_flat_field_rows would refuse.
 * paris_hip_ring_profile_finish runs what is pending, waits for the ctx stream, copies the sums down, forms the means and calls
 * paris_hip_ring_correction_from_mean with the counts; h_c and h_mean (may be NULL) receive dim_y rows of dim_x floats, rows without
 * a frame a mean of 0. The profile is then closed and its memory freed. A profile with no frame at all gives c = 0 everywhere and
 * frames_max = 0. PARIS_HIP_ERROR_INVALID_ARGUMENT without an open profile, for a NULL h_c, or as the check; the profile stays open.
 * paris_hip_ring_profile_discard closes an open profile (no error without one). */
int paris_hip_ring_profile_begin(paris_hip_ctx* ctx, uint32_t dim_x, uint32_t dim_y);
int paris_hip_ring_profile_add_rows(paris_hip_ctx* ctx, const float* d_p, size_t pitch, size_t frame_stride, uint32_t n_frames,
                                    uint32_t dim_x, uint32_t dim_y, uint32_t row_first, uint32_t row_count);
int paris_hip_ring_profile_finish(paris_hip_ctx* ctx, const paris_hip_ring_filter* setting, float* h_c, float* h_mean,
                                  paris_hip_ring_stats* out);
int paris_hip_ring_profile_discard(paris_hip_ctx* ctx);
/* paris_hip_set_ring_correction copies the dim_x x dim_y correction frame c (rows dim_x floats apart) into memory the ctx owns,
 * replacing an earlier one; the old frame is freed once the work queued before the call no longer reads it. The frame counts towards
 * paris_hip_projection_reserve_bytes while set; paris_hip_ctx_destroy frees it. PARIS_HIP_ERROR_INVALID_ARGUMENT for a NULL h_c, a
 * zero dimension or a value that is not finite. Without a setting nothing else changes. */
int paris_hip_set_ring_correction(paris_hip_ctx* ctx, const float* h_c, uint32_t dim_x, uint32_t dim_y);
int paris_hip_clear_ring_correction(paris_hip_ctx* ctx);
/* In place on float frames: every pixel with c != 0 in rows [row_first, row_first + row_count) of n_frames frames frame_stride
 * bytes apart, d_p the first frame's row 0, becomes p - c. A correction frame that is zero everywhere makes the call idle: nothing
 * is launched, no pending group either. PARIS_HIP_ERROR_INVALID_ARGUMENT without a setting, when dim_x / dim_y differ from the
 * setting's, or for a band, pitch or stride paris_hip_flat_field_rows would refuse. */
int paris_hip_ring_correct_rows(paris_hip_ctx* ctx, float* d_p, size_t pitch, size_t frame_stride, uint32_t n_frames, uint32_t dim_x,
                                uint32_t dim_y, uint32_t row_first, uint32_t row_count);
/* Extension (no reference counterpart): finding the rotation axis, delta_s, from the scan itself by the fan-beam consistency of
 * the mid-plane. With the ray the backprojector and paris_hip_forward_project define -- source
 * (-d_so cos phi, -d_so sin phi), direction (d_sd cos phi - t sin phi, d_sd sin phi + t cos phi) -- the ray at view angle phi and
 * fan angle gamma = atan(t / d_sd) is the same line as the ray at phi + 180 deg + 2 gamma and fan angle -gamma. With
 * t_i = ((i + 1/2) - n / 2 - c) l the conjugate of column i lies at column (n - 1 - i) + 2 c. The cost of a candidate c is the mean
 * squared difference between every mid-plane sample and its conjugate, interpolated linearly in column and in view; it has its
 * minimum at the true c.
 * Setting paris_hip_axis_search { float lo; float step; uint32_t count; uint32_t rows; uint32_t min_columns; }.
 *   Candidates are c_k = (float)((double)lo + k (double)step), k = 0 .. count - 1, in detector pixels: values of delta_s.
 *   1 <= count <= 1024; lo is finite; step > 0 and finite.
 *   rows R is in [1, 64] and R <= n_col.
 *   min_columns = 0 stands for max(8, n_row / 16).
 * Scan. N frames, N >= 4, frame f taken at f 360 / N degrees: a full, equidistant circle. The pixels are line integrals, as the ring
 *   profile sees them: after the zinger filter, before the ring correction and every weight. n = n_row.
 *   The geometry needs l_px_row > 0, d_sd = |d_so| + |d_od| > 0 and delta_t, all finite.
 * Band. j_c = n_col / 2 + delta_t - 1/2; row_first = floor(j_c - (R - 1) / 2 + 1/2), in double, clamped to [0, n_col - R].
 * Sinogram. S[f][i] is the fp32 sum of rows row_first .. row_first + R - 1 of frame f at column i: acc = +0; acc = acc + p in ascending
 *   row order, each addition rounded once, no contraction.
 * Plan (host only, the single implementation: paris_hip_axis_search_plan). For candidate c and column i, everything in double and
 *   rounded once:
 *   ip = (n - 1 - i) + 2 c; i0 = floor(ip); wi = (float)(ip - i0). The column is valid iff 0 <= i0 and i0 + 1 <= n - 1.
 *   gamma = atan((((i + 1/2) - n / 2 - c) l_px_row) / d_sd).
 *   kk = N / 2 + (gamma N) / pi; k0 = floor(kk) reduced into [0, N); wf = (float)(kk - floor(kk)).
 *   One 16-byte entry per (c, i): { int32 i0 (-1 = invalid); uint32 k0; float wi; float wf }; an invalid entry is { -1, 0, 0, 0 }.
 * Pair (device). For a valid column, with fa = (f + k0) mod N and fb = (fa + 1) mod N, all in fp32, each operation rounded once, no
 *   contraction:
 *   a = S[fa][i0] + wi (S[fa][i0 + 1] - S[fa][i0]); b is the same on fb.
 *   m = a + wf (b - a); d = S[f][i] - m. A pair whose d is not finite is skipped and counted.
 * Cost. J[k] = sum of (double)d (double)d over all f and valid i, divided by the integer number of pairs summed. The sum is
 *   accumulated in double. There are no floating-point atomics: every partial sum has one owner and the partial sums are combined in
 *   a fixed order, so two runs give the same bits. A candidate with fewer than min_columns valid columns, or with no pair summed, is
 *   unscored: J = +inf.
 * Estimate (host only, the single implementation: paris_hip_axis_estimate_from_costs). A candidate is scored iff its J is finite.
 *   m = the index of the smallest J among the scored; ties go to the lowest index.
 *   The parabola applies if m - 1 and m + 1 exist and are scored, and q = J[m-1] - 2 J[m] + J[m+1] > 0. Then
 *   off = (1/2) (J[m-1] - J[m+1]) / q, clamped to [-1/2, 1/2], and delta_s = (float)(c_m + off step), in double.
 *   Otherwise delta_s = c_m and at_edge = 1.
 *   The median reported is the lower one: the ((s - 1) / 2 + 1)-th smallest of the s scored J.
 * Limits: the mid-plane only -- the cone angle across the R rows is ignored; a full equidistant circle; detector tilt is not
 * estimated. The detector's in-plane rotation is found by a search of its own, paris_hip_roll_search_run below. */
typedef struct paris_hip_axis_search {
    float lo;             /* the first candidate [px] */
    float step;           /* the distance between candidates [px], > 0 */
    uint32_t count;       /* candidates, 1 .. 1024 */
    uint32_t rows;        /* R: detector rows summed into the mid-plane line, 1 .. 64 */
    uint32_t min_columns; /* a candidate with fewer valid columns is unscored; 0 = max(8, n_row / 16) */
} paris_hip_axis_search;
typedef struct paris_hip_axis_entry {
    int32_t i0;  /* the conjugate's left column; -1: the column has no conjugate on the detector */
    uint32_t k0; /* the conjugate's first view is (f + k0) mod N */
    float wi;    /* the weight of column i0 + 1 */
    float wf;    /* the weight of view (f + k0 + 1) mod N */
} paris_hip_axis_entry;
typedef struct paris_hip_axis_result {
    float delta_s;      /* the estimate [px] */
    uint32_t best;      /* m: the index of the smallest scored J */
    double cost_min;    /* J[m] */
    double cost_median; /* the lower median of the scored J */
    uint32_t scored;    /* candidates with a finite J */
    uint32_t columns;   /* the valid columns of candidate m (0 when the columns were not given) */
    uint64_t skipped;   /* pairs whose difference was not finite, over all candidates (paris_hip_axis_search_finish only) */
    uint32_t at_edge;   /* 1: no parabola -- the minimum is at an end, beside an unscored candidate, or not convex */
    uint32_t row_first; /* the band's first row (paris_hip_axis_search_finish only) */
} paris_hip_axis_result;
/* one collect launch serves at most this many frames; calls with more loop */
#define PARIS_HIP_AXIS_FRAMES_MAX 64
/* Host only, no ctx and no device: checks a setting for a detector and a scan of n_frames frames, and reports the band's first row
 * and what an open search occupies on the device (sinogram, plan, partial sums); either pointer may be NULL.
 * PARIS_HIP_ERROR_INVALID_ARGUMENT for a NULL setting or geometry or for what the rule above excludes; PARIS_HIP_ERROR_UNSUPPORTED when
 * n_row count or n_frames n_row does not fit 32 bits, or n_row does not fit 31. */
int paris_hip_axis_search_check(const paris_hip_axis_search* setting, const paris_detector_geometry* det_geo, uint32_t n_frames,
                                uint32_t* row_first, size_t* device_bytes);
/* Host only: the n_row plan entries of candidate k -- the single implementation of the plan. PARIS_HIP_ERROR_INVALID_ARGUMENT as the
 * check, for k >= count or a NULL entries. */
int paris_hip_axis_search_plan(const paris_hip_axis_search* setting, const paris_detector_geometry* det_geo, uint32_t n_frames, uint32_t k,
                               paris_hip_axis_entry* entries);
/* Host only: the estimate from the `count` costs -- the single implementation. columns (count entries, may be NULL) only supplies
 * result->columns; skipped and row_first are set to 0. Only lo, step and count of the setting are read.
 * PARIS_HIP_ERROR_INVALID_ARGUMENT for a NULL setting, cost or result, a count outside 1 .. 1024, a lo or step the rule excludes, or
 * when no candidate is scored (the result then has scored = 0). */
int paris_hip_axis_estimate_from_costs(const paris_hip_axis_search* setting, const double* cost, const uint32_t* columns,
                                       paris_hip_axis_result* result);
/* The search: paris_hip_axis_search_begin runs the check, makes the plan of every candidate on the host and copies it into memory the
 * ctx owns, beside the n_frames x n_row sinogram and the partial sums. That memory counts towards
 * paris_hip_projection_reserve_bytes while the search is open and is freed by finish, discard or paris_hip_ctx_destroy. begin on an
 * open search replaces it; work queued before keeps the old one.
 * paris_hip_axis_search_add_rows sums the band of n_frames frames frame_stride bytes apart, d_p the first frame's row 0, into the
 * sinogram rows frame_first .. frame_first + n_frames - 1; the frames are only read. 16-byte loads are used where the base, the pitch,
 * the stride (n_frames > 1) and dim_x are multiples of 16 bytes, single pixels otherwise. The host counts each sinogram row: a row
 * added twice, or one beyond n_frames, is PARIS_HIP_ERROR_INVALID_ARGUMENT and adds nothing. A held-back weighting runs first, and a
 * frame of the pending by-reference group has that group launched first. PARIS_HIP_ERROR_INVALID_ARGUMENT also without an open
 * search, when dim_x / dim_y differ from n_row / n_col, or for a pitch or stride paris_hip_flat_field_rows would refuse.
 * paris_hip_axis_search_finish refuses while a sinogram row is missing (PARIS_HIP_ERROR_INVALID_ARGUMENT; the search stays open, as
 * for a NULL cost or result). Otherwise it scores every candidate on the device, waits for the ctx stream, fills cost[count] and
 * columns[count] (may be NULL; the valid columns per candidate), runs the estimate and closes the search, whatever the estimate
 * answers. h_sinogram (may be NULL) receives n_frames rows of n_row floats.
 * paris_hip_axis_search_discard closes an open search (no error without one). */
int paris_hip_axis_search_begin(paris_hip_ctx* ctx, const paris_hip_axis_search* setting, const paris_detector_geometry* det_geo,
                                uint32_t n_frames);
int paris_hip_axis_search_add_rows(paris_hip_ctx* ctx, const float* d_p, size_t pitch, size_t frame_stride, uint32_t n_frames,
                                   uint32_t dim_x, uint32_t dim_y, uint32_t frame_first);
int paris_hip_axis_search_finish(paris_hip_ctx* ctx, double* cost, uint32_t* columns, paris_hip_axis_result* result, float* h_sinogram);
int paris_hip_axis_search_discard(paris_hip_ctx* ctx);
/* Extension (no reference counterpart): detector binning on the device, between paris_hip_upload_projection_raw and
 * paris_hip_flat_field_rows, where the pixels are detector counts as fp32. One definition; the device
 * (paris_hip_bin_frames) and the host (paris_hip_bin_frame_host) both implement it.
 * Setting paris_hip_binning { uint32_t bin_x, bin_y; }. Each factor is 1, 2, 4 or 8, chosen independently.
 *   A dim_x x dim_y source frame gives a binned frame of out_x = dim_x / bin_x by out_y = dim_y / bin_y pixels (integer division).
 *   The trailing r_x = dim_x - out_x bin_x columns and r_y = dim_y - out_y bin_y rows are dropped.
 *   out_x == 0 or out_y == 0 is PARIS_HIP_ERROR_INVALID_ARGUMENT.
 * Mask (optional): dim_y rows of dim_x bytes at SOURCE size, in the defect map's format: nonzero = bad. Without one every pixel is good.
 * Binned pixel (X, Y).
 *   Its source pixels are (x, y), x in [X bin_x, (X + 1) bin_x), y in [Y bin_y, (Y + 1) bin_y), visited row-major: y outer, x inner.
 *   acc = +0, n = 0. For each GOOD source pixel p in that order: acc = acc + p, one fp32 addition, no contraction; n += 1.
 *   out = acc / (float)n, one IEEE fp32 division, when n >= 1; out = +0 when n == 0.
 *   Pixels that are not finite get no special treatment and propagate (the flat-field rule turns them into dead pixels).
 * What follows from it:
 *   u8 and u16 counts widened to fp32 sum exactly in any order (64 * 65535 < 2^24); for u32 and f32 frames the order above is the
 *   definition.
 *   The binned mask (paris_hip_bin_mask) has byte (X, Y) = 1 iff n == 0 -- a bin with one good pixel is good. It is what
 *   paris_hip_set_defect_map takes at binned size.
 *   Dark and flat frames are binned by the same rule with the same mask, on the host; the correction then runs unchanged on the
 *   binned frame against the binned references.
 * Binned geometry (paris_hip_binned_geometry), each field computed in double and rounded once to fp32:
 *   n_row' = out_x, n_col' = out_y, l_px_row' = bin_x l_px_row, l_px_col' = bin_y l_px_col,
 *   delta_s' = (delta_s + r_x / 2) / bin_x, delta_t' = (delta_t + r_y / 2) / bin_y; d_so, d_od and delta_phi are unchanged.
 *   In the backprojector's coordinates, t = (i + 1/2) l - n l / 2 - delta_s l and the same form for rows, the centre of a binned
 *   pixel is then the mean of its source pixels' centres: the dropped remainder does not shift the rotation axis. */
typedef struct paris_hip_binning {
    uint32_t bin_x; /* source columns per binned pixel: 1, 2, 4 or 8 */
    uint32_t bin_y; /* source rows per binned pixel: 1, 2, 4 or 8 */
} paris_hip_binning;
/* Host only, no ctx and no device: checks a setting for a dim_x x dim_y detector and returns the binned size (either pointer may be
 * NULL). PARIS_HIP_ERROR_INVALID_ARGUMENT for a NULL setting, a factor outside {1, 2, 4, 8}, or a binned size of 0. */
int paris_hip_binning_check(const paris_hip_binning* setting, uint32_t dim_x, uint32_t dim_y, uint32_t* out_x, uint32_t* out_y);
/* Host only: the geometry rule above for det_geo's n_row x n_col detector. PARIS_HIP_ERROR_INVALID_ARGUMENT as the check, or for a NULL
 * geometry. out_geo may be det_geo. */
int paris_hip_binned_geometry(const paris_hip_binning* setting, const paris_detector_geometry* det_geo, paris_detector_geometry* out_geo);
/* Host only: the pixel rule on a dense frame -- src dim_y rows of dim_x floats, dst out_y rows of out_x floats, mask as above or
 * NULL. For the references. PARIS_HIP_ERROR_INVALID_ARGUMENT as the check, or for a NULL src or dst. */
int paris_hip_bin_frame_host(const paris_hip_binning* setting, const uint8_t* mask, const float* src, uint32_t dim_x, uint32_t dim_y,
                             float* dst);
/* Host only: the binned mask, out_y rows of out_x bytes of 0 / 1. PARIS_HIP_ERROR_INVALID_ARGUMENT as the check, or for a NULL pointer. */
int paris_hip_bin_mask(const paris_hip_binning* setting, const uint8_t* mask, uint32_t dim_x, uint32_t dim_y, uint8_t* out_mask);
/* paris_hip_set_binning runs the check and stores the setting for dim_x x dim_y source frames; the mask (may be NULL) is copied into
 * memory the ctx owns, replacing an earlier setting; the old mask is freed once the work queued before the call no longer reads it.
 * The mask counts towards paris_hip_projection_reserve_bytes while set; paris_hip_ctx_destroy frees it. Without a setting nothing
 * else changes. */
int paris_hip_set_binning(paris_hip_ctx* ctx, const paris_hip_binning* setting, const uint8_t* mask, uint32_t dim_x, uint32_t dim_y);
int paris_hip_clear_binning(paris_hip_ctx* ctx);
/* Writes BINNED rows [row_first, row_first + row_count) of n_frames binned frames (out_x x out_y, rows dst_pitch bytes apart, frames
 * dst_frame_stride bytes apart, d_dst the first frame's row 0) from source rows [bin_y row_first, bin_y (row_first + row_count)) of
 * n_frames source frames (dim_x x dim_y, src_pitch, src_frame_stride, d_src the first frame's row 0). The source is only read; bytes
 * of a destination row past 4 out_x are not written. 16-byte vectors are used where both bases, both pitches and (n_frames > 1)
 * both strides are multiples of 16, single pixels otherwise. A held-back weighting runs first; a source or destination frame of the
 * pending by-reference group has that group launched first, and both are noted as used, so a later upload into either waits.
 * PARIS_HIP_ERROR_INVALID_ARGUMENT without a setting, when dim_x / dim_y differ from the setting's, for a band outside out_y, for a
 * pitch or stride paris_hip_flat_field_rows would refuse (the source's for dim_x x dim_y, the destination's for out_x x out_y), or
 * when the source and destination ranges overlap. */
int paris_hip_bin_frames(paris_hip_ctx* ctx, const float* d_src, size_t src_pitch, size_t src_frame_stride, float* d_dst, size_t dst_pitch,
                         size_t dst_frame_stride, uint32_t n_frames, uint32_t dim_x, uint32_t dim_y, uint32_t row_first,
                         uint32_t row_count);
/* Extension (no reference counterpart): correction of the detector's in-plane rotation ("roll", eta) about its normal -- every
 * frame is resampled onto a detector whose rows are perpendicular to the projected rotation axis, after every correction that is
 * stationary in detector coordinates and before the redundancy weights and the row filter. One definition;
 * the device (paris_hip_detector_roll_rows) and the host (paris_hip_detector_roll_host) both implement it and give the same bits.
 * Setting paris_hip_detector_roll { float eta_deg; }. eta_deg is finite, nonzero and |eta_deg| <= 10; "no roll" is no setting.
 *   The detector needs n_row >= 2 and n_col >= 2, l_px_row, l_px_col > 0 and finite, delta_s and delta_t finite.
 * Constants, each computed on the host in double and rounded to float once: eta = eta_deg pi / 180, rho = l_px_col / l_px_row,
 *   cx = n_row / 2 + delta_s - 1/2, cy = n_col / 2 + delta_t - 1/2 (the axis column of the axis search and its band's centre row),
 *   a = cos eta, b = -sin eta rho, c = sin eta / rho, d = cos eta: a rotation in millimetres about (cx, cy).
 * Output pixel (i, j) -- column i, row j -- of a frame p, all in fp32, each operation rounded once, no contraction:
 *   di = (float)i - cx, dj = (float)j - cy;
 *   x = (a di + b dj) + cx, y = (c di + d dj) + cy (two products, their sum, then the centre);
 *   x is clamped to [0, n_row - 1] and y to [0, n_col - 1] (x < 0 becomes 0, x > n_row - 1 becomes n_row - 1): the edge is replicated;
 *   i0 = min((int)floor(x), n_row - 2), wx = x - (float)i0; j0 = min((int)floor(y), n_col - 2), wy = y - (float)j0;
 *   top = p[j0][i0] + wx (p[j0][i0 + 1] - p[j0][i0]); bot is the same on row j0 + 1; out = top + wy (bot - top).
 *   A tap that is not finite propagates by this arithmetic alone.
 * Source rows of a destination band. Every step is monotone in i and in j, so the extremes of y over a band lie at its four
 *   corner pixels: the band reads rows min j0 .. max j0 + 1 over the corners (paris_hip_detector_roll_source_rows), exactly. */
typedef struct paris_hip_detector_roll {
    float eta_deg; /* the detector's in-plane rotation [deg], nonzero, |eta_deg| <= 10 */
} paris_hip_detector_roll;
/* Host only, no ctx and no device. PARIS_HIP_ERROR_INVALID_ARGUMENT for a NULL setting or geometry or for what the rule excludes. */
int paris_hip_detector_roll_check(const paris_hip_detector_roll* setting, const paris_detector_geometry* det_geo);
/* Host only: the rule on one dense frame -- src and dst n_col rows of n_row floats, which must not overlap. The single host
 * implementation. PARIS_HIP_ERROR_INVALID_ARGUMENT as the check, or for a NULL src or dst. */
int paris_hip_detector_roll_host(const paris_hip_detector_roll* setting, const paris_detector_geometry* det_geo, const float* src,
                                 float* dst);
/* Host only: the source rows [*src_first, *src_first + *src_count) that destination rows [row_first, row_first + row_count) read.
 * An empty band gives (row_first clamped to n_col - 1, 0). PARIS_HIP_ERROR_INVALID_ARGUMENT as the check, for a band outside n_col or
 * a NULL pointer. */
int paris_hip_detector_roll_source_rows(const paris_hip_detector_roll* setting, const paris_detector_geometry* det_geo, uint32_t row_first,
                                        uint32_t row_count, uint32_t* src_first, uint32_t* src_count);
/* paris_hip_set_detector_roll runs the check and stores the setting with the geometry; nothing lives on the device.
 * paris_hip_clear_detector_roll removes it (no error without one). Without a setting nothing else changes. */
int paris_hip_set_detector_roll(paris_hip_ctx* ctx, const paris_hip_detector_roll* setting, const paris_detector_geometry* det_geo);
int paris_hip_clear_detector_roll(paris_hip_ctx* ctx);
/* Writes rows [row_first, row_first + row_count) of n_frames destination frames (dim_x x dim_y, rows dst_pitch bytes apart, frames
 * dst_frame_stride bytes apart, d_dst the first frame's row 0) from source frames of the same size (src_pitch, src_frame_stride,
 * d_src the first frame's row 0), of which only the rows paris_hip_detector_roll_source_rows names are read. Nothing else is
 * written, bytes of a row past 4 dim_x included. A lane owns four adjacent pixels and stores them as one 16-byte vector where the
 * destination's base, pitch and (n_frames > 1) stride are multiples of 16, single pixels otherwise and in a row's ragged last
 * segment. A held-back weighting runs first; a source or destination frame of the pending by-reference group has that group
 * launched first, and both bands are noted as used. PARIS_HIP_ERROR_INVALID_ARGUMENT without a setting, when dim_x / dim_y differ
 * from the setting's n_row / n_col, for a band outside dim_y, for a pitch or stride paris_hip_flat_field_rows would refuse, or when
 * the source and destination ranges overlap. _with takes the setting and the geometry as arguments; the ctx's own setting is neither
 * used nor changed. */
int paris_hip_detector_roll_rows(paris_hip_ctx* ctx, const float* d_src, size_t src_pitch, size_t src_frame_stride, float* d_dst,
                                 size_t dst_pitch, size_t dst_frame_stride, uint32_t n_frames, uint32_t dim_x, uint32_t dim_y,
                                 uint32_t row_first, uint32_t row_count);
int paris_hip_detector_roll_rows_with(paris_hip_ctx* ctx, const float* d_src, size_t src_pitch, size_t src_frame_stride, float* d_dst,
                                      size_t dst_pitch, size_t dst_frame_stride, uint32_t n_frames, uint32_t dim_x, uint32_t dim_y,
                                      uint32_t row_first, uint32_t row_count, const paris_hip_detector_roll* setting,
                                      const paris_detector_geometry* det_geo);
/* Finding the roll from the scan itself. Over a full circle a point at cylinder coordinates (r, phi0, z)
 * is seen at detector position (t, v) in view phi0 - psi and at (-t, v) in view phi0 + psi: the scan mean of the line integrals is
 * mirror-symmetric about the projected axis column in every detector row, whatever the object and the cone angle. A rolled detector
 * tilts that line by eta; the cost of a candidate is the mean squared asymmetry of the mean frame rolled back by it.
 * Setting paris_hip_roll_search { float lo_deg; float step_deg; uint32_t count; uint32_t min_pixels; }.
 *   Candidates are eta_k = (float)((double)lo_deg + k (double)step_deg), k = 0 .. count - 1; 1 <= count <= 256; lo_deg finite;
 *   step_deg > 0 and finite. Every candidate passes paris_hip_detector_roll_check or is exactly 0; a candidate of exactly 0 is
 *   scored on the mean itself. min_pixels = 0 stands for n_row n_col / 16.
 * Input. The scan mean M, n_col rows of n_row floats, of a full equidistant circle of line integrals on a centred detector: the
 *   h_mean of paris_hip_ring_profile_finish.
 * Margins keep replicated pixels out of the score. With the constants of candidate k as the pixel rule rounds them,
 *   m_x = ceil(max_k(|b_k| max(cy, n_col - 1 - cy) + |1 - a_k| max(cx, n_row - 1 - cx))) + 1, in double, and m_y the same with c_k,
 *   d_k and cx and cy exchanged. The rows scored are [m_y, n_col - m_y). 2 m_x >= n_row or 2 m_y >= n_col is refused.
 * Mirror plan, on the host in double, once per search, with cx = n_row / 2 + delta_s - 1/2 in double: for column i,
 *   ip = 2 cx - i, i0 = floor(ip), w = (float)(ip - i0); the column is valid iff m_x <= i <= n_row - 1 - m_x, m_x <= i0 and
 *   i0 + 1 <= n_row - 1 - m_x.
 * Score (device). R_k is M rolled by eta_k, by the kernel of paris_hip_detector_roll_rows. For every scored row j and valid column
 *   i, in fp32, each operation rounded once: mir = R[j][i0] + w (R[j][i0 + 1] - R[j][i0]), dd = R[j][i] - mir. A dd that is not
 *   finite is skipped and counted. J[k] = the sum of (double)dd (double)dd divided by the integer number of pairs summed. Every
 *   partial sum has one owner and the partial sums are combined in a fixed order: two runs give the same bits. A candidate with
 *   fewer than min_pixels pairs, or none, is unscored: J = +inf.
 * Estimate: the rule of paris_hip_axis_estimate_from_costs -- both call one implementation.
 * Limits: a full equidistant circle on a centred detector (not short or offset scans); out-of-plane tilts are not estimated. */
typedef struct paris_hip_roll_search {
    float lo_deg;        /* the first candidate [deg] */
    float step_deg;      /* the distance between candidates [deg], > 0 */
    uint32_t count;      /* candidates, 1 .. 256 */
    uint32_t min_pixels; /* a candidate with fewer pairs is unscored; 0 = n_row n_col / 16 */
} paris_hip_roll_search;
typedef struct paris_hip_roll_result {
    float eta_deg;      /* the estimate [deg] */
    uint32_t best;      /* m: the index of the smallest scored J */
    double cost_min;    /* J[m] */
    double cost_median; /* the lower median of the scored J */
    uint32_t scored;    /* candidates with a finite J */
    uint32_t at_edge;   /* 1: no parabola -- the minimum is at an end, beside an unscored candidate, or not convex */
    uint64_t skipped;   /* pairs whose difference was not finite, over all candidates (paris_hip_roll_search_run only) */
    uint32_t margin_x;  /* m_x (paris_hip_roll_search_run only) */
    uint32_t margin_y;  /* m_y (paris_hip_roll_search_run only) */
} paris_hip_roll_result;
/* Host only, no ctx and no device: checks a search for a detector and reports the margins and what the search occupies on the
 * device while it runs (any pointer may be NULL). PARIS_HIP_ERROR_INVALID_ARGUMENT for a NULL setting or geometry or for what the
 * rule above excludes. */
int paris_hip_roll_search_check(const paris_hip_roll_search* setting, const paris_detector_geometry* det_geo, uint32_t* margin_x,
                                uint32_t* margin_y, size_t* device_bytes);
/* Host only: the estimate from the `count` costs. Only lo_deg, step_deg and count are read; skipped and the margins are set to 0.
 * PARIS_HIP_ERROR_INVALID_ARGUMENT for a NULL pointer, a count outside 1 .. 256, a lo_deg or step_deg the rule excludes, or when no
 * candidate is scored (the result then has scored = 0). */
int paris_hip_roll_estimate_from_costs(const paris_hip_roll_search* setting, const double* cost, paris_hip_roll_result* result);
/* The search (paris_hip_roll_search_run; the setting has the plain name): runs the check, uploads h_mean into memory of its own, scores every candidate on the ctx stream, waits for it, fills
 * cost[count] and pairs[count] (may be NULL), runs the estimate and frees its memory, whatever the estimate answers. The ctx's
 * own roll setting is neither used nor changed. */
int paris_hip_roll_search_run(paris_hip_ctx* ctx, const paris_hip_roll_search* setting, const paris_detector_geometry* det_geo,
                              const float* h_mean, double* cost, uint64_t* pairs, paris_hip_roll_result* result);
/* Extension (no reference counterpart): normalisation of every frame to an air region -- the flat is taken once, but the source's
 * output drifts from frame to frame; a frame taken at (1 + e) of the flat's flux comes out of the dark / flat correction as
 * p - ln(1 + e), a constant over the frame, which FDK turns into shading and streaks. A rectangle of the
 * detector that sees only air in every view measures that constant: its mean line integral is subtracted from the whole frame.
 * One definition; the device (paris_hip_air_normalize_rows, paris_hip_air_measure) and the host (paris_hip_air_value_host) both
 * implement it and give the same bits.
 * Setting paris_hip_air_region { uint32_t x0, y0, width, height; uint32_t min_pixels; float limit_abs; }.
 *   The rectangle is columns [x0, x0 + width) and rows [y0, y0 + height) of the dim_x x dim_y frame as the reconstruction sees it
 *   (the binned frame with binning). width, height >= 1, the rectangle lies inside the frame, width * height <= 2^20.
 *   min_pixels = 0 stands for (width * height + 1) / 2; otherwise 1 <= min_pixels <= width * height.
 *   limit_abs is finite and >= 0; 0 means no limit.
 * Mask (optional, given with the setting): dim_y rows of dim_x bytes in the defect map's format, nonzero = bad. Only the rectangle's
 *   bytes are kept.
 * A pixel of the rectangle COUNTS iff its mask byte is 0 and its value is finite.
 * Value of frame f, with 256 partial sums:
 *   for l in 0 .. 255, c = l mod 64, r = l div 64: acc_l = +0.0 in DOUBLE, n_l = 0;
 *   for y = y0 + r, y0 + r + 4, ... ascending, and within a row x = x0 + c, x0 + c + 64, ... ascending: if the pixel counts,
 *   acc_l += (double)p and n_l += 1;
 *   S = ((acc_0 + acc_1) + acc_2) + ..., ascending l, in double; n = sum of the n_l.
 *   n < min_pixels: a_f = +0, the frame is counted as too_few.
 *   Otherwise a_f = (float)(S / (double)n), rounded once.
 *   limit_abs != 0 and |a_f| > limit_abs: a_f = +0, the frame is counted as above_limit -- the object has entered the rectangle,
 *   which is a wrong setting, not drift.
 * Apply. Every pixel of rows [row_first, row_first + row_count) of frame f becomes p - a_f, one fp32 subtraction. A frame whose a_f
 *   is zero of either sign is NOT WRITTEN at all: its bits stay, NaN payloads included.
 * Order. The pass runs on line integrals, directly after the dark / flat correction and before the defect repair, the zinger filter,
 *   the ring profile and correction, the axis search and every weight. It reads the rectangle's rows of each frame and writes the
 *   band's rows: the caller guarantees that the rectangle's rows hold corrected pixels. The value is read before anything is written,
 *   also when the rectangle lies inside the band. The pass is not idempotent in bits: a second call finds a value near 0.
 * Limits: one rectangle; a mean, so a zinger inside the rectangle shifts a_f by its value / n; no smoothing of a_f over the scan. */
typedef struct paris_hip_air_region {
    uint32_t x0, y0;        /* the rectangle's first column and row */
    uint32_t width, height; /* >= 1 each, width * height <= 2^20 */
    uint32_t min_pixels;    /* a frame with fewer counting pixels is not normalised; 0 = (width * height + 1) / 2 */
    float limit_abs;        /* a frame whose |a_f| is larger is not normalised; 0 = no limit */
} paris_hip_air_region;
/* what paris_hip_air_stats reports */
typedef struct paris_hip_air_counts {
    uint64_t frames;      /* frames the normalise calls measured (per call: each frame of a non-empty band) */
    uint64_t normalised;  /* of those, frames whose a_f was kept (it may still be zero) */
    uint64_t too_few;     /* frames with fewer than min_pixels counting pixels */
    uint64_t above_limit; /* frames whose |a_f| exceeded limit_abs */
    float min_a, max_a;   /* the smallest and the largest a_f over the normalised frames; +inf / -inf without one */
} paris_hip_air_counts;
/* one launch pair serves at most this many frames; calls with more loop */
#define PARIS_HIP_AIR_FRAMES_MAX 64
/* Host only, no ctx and no device: checks a setting for a dim_x x dim_y frame, resolves the default min_pixels (may be NULL) and
 * reports what the setting occupies on the device while set (may be NULL): the rectangle's mask bytes, the values and counts of one
 * launch and the counters. PARIS_HIP_ERROR_INVALID_ARGUMENT for a NULL setting, a zero dimension or anything the rule excludes. */
int paris_hip_air_region_check(const paris_hip_air_region* setting, uint32_t dim_x, uint32_t dim_y, uint32_t* min_pixels,
                               size_t* device_bytes);
/* Host only: the rule on a dense frame (dim_y rows of dim_x floats; mask as above or NULL) -- the second implementation of the one
 * definition. *a is the value after the too_few / above_limit rule, *n the count (either may be NULL).
 * PARIS_HIP_ERROR_INVALID_ARGUMENT as the check, or for a NULL frame. */
int paris_hip_air_value_host(const paris_hip_air_region* setting, const uint8_t* mask, const float* frame, uint32_t dim_x, uint32_t dim_y,
                             float* a, uint32_t* n);
/* paris_hip_set_air_region runs the check and keeps the setting for dim_x x dim_y frames; the rectangle's mask bytes (zeros for a
 * NULL mask), the per-launch values and the counters live in memory the ctx owns, replacing an earlier setting (and its counts); the
 * old memory is freed once the work queued before the call no longer uses it. It counts towards paris_hip_projection_reserve_bytes
 * while set; paris_hip_ctx_destroy frees it. Without a setting nothing else changes. */
int paris_hip_set_air_region(paris_hip_ctx* ctx, const paris_hip_air_region* setting, const uint8_t* mask, uint32_t dim_x, uint32_t dim_y);
int paris_hip_clear_air_region(paris_hip_ctx* ctx);
/* In place on float frames, asynchronous: per launch pair of up to PARIS_HIP_AIR_FRAMES_MAX frames, a_f of every frame is measured
 * from the rectangle, then rows [row_first, row_first + row_count) of every frame with a_f != 0 become p - a_f (n_frames frames
 * frame_stride bytes apart, d_p the first frame's row 0). A band of zero rows does nothing. 16-byte vectors are used for the
 * subtraction where the base, the pitch, the stride (n_frames > 1) and dim_x allow, single pixels otherwise. The rectangle's rows
 * are noted as used beside the band's, so a later upload into either waits. PARIS_HIP_ERROR_INVALID_ARGUMENT without a setting, when
 * dim_x / dim_y differ from the setting's, or for a band, pitch or stride paris_hip_flat_field_rows would refuse. */
int paris_hip_air_normalize_rows(paris_hip_ctx* ctx, float* d_p, size_t pitch, size_t frame_stride, uint32_t n_frames, uint32_t dim_x,
                                 uint32_t dim_y, uint32_t row_first, uint32_t row_count);
/* Synchronous: the same reduction, nothing written to the frames and nothing added to the counters; h_a and h_n (either may be NULL)
 * receive n_frames values (after the too_few / above_limit rule) and counts. Refusals as paris_hip_air_normalize_rows. */
int paris_hip_air_measure(paris_hip_ctx* ctx, const float* d_p, size_t pitch, size_t frame_stride, uint32_t n_frames, uint32_t dim_x,
                          uint32_t dim_y, float* h_a, uint32_t* h_n);
/* The counts of the normalise calls since the setting was made or last reset: runs what is pending, waits for the ctx stream and
 * reads them; reset != 0 zeroes them afterwards. PARIS_HIP_ERROR_INVALID_ARGUMENT without a setting or for a NULL out. */
int paris_hip_air_stats(paris_hip_ctx* ctx, paris_hip_air_counts* out, int reset);
/* Extension (no reference counterpart): beam-hardening correction -- a polychromatic tube makes the line integral
 * p = -ln(sum s_E exp(-mu_E L)) concave in the path length L, and FDK turns that into cupping. The correction is a polynomial of the
 * line integral without a constant term, q = c_1 p + c_2 p^2 + ... + c_N p^N, and its coefficients can be fitted from the scan itself
 * (empirical cupping correction, Kachelriess et al. 2006). One definition of every piece; where the device and
 * the host both implement one they give the same bits.
 * Setting paris_hip_beam_hardening { uint32_t degree; float c[PARIS_HIP_BH_DEGREE_MAX]; }: 1 <= degree <= 4, every c_k finite, c[0] is
 *   c_1. Air (p = 0) stays 0.
 * Rule, per pixel, in fp32, N = degree:
 *   p >= 0, or p is NaN: acc = c_N; acc = fmaf(acc, p, c_k) for k = N-1 ... 1; q = acc * p -- the last step is one multiplication.
 *   p < 0 (noise in air): q = c_1 * p; the higher terms would bias air.
 *   Explicit fused multiply-adds, no contraction elsewhere. A NaN pixel gives a NaN whose payload is unspecified.
 * Order. The pass runs on line integrals, after the ring correction and before every weight (short-scan, offset-detector, cosine).
 * Fit, on a slab of dim_x x dim_y x dim_z voxels (a volume or a run of whole slices of it), from the basis volumes f_k = FDK(p^k):
 *   (a) Threshold (paris_hip_bh_threshold_from_histogram, host, the single implementation): Otsu's rule in double on the histogram
 *       paris_hip_volume_stats returns for f_1 over [min, max]. T = sum of the bins, width = ((double)h_hi - h_lo) / n_bins. For the
 *       inclusive cumulative split at bin b: w0 = C(b) / T, mu0 = (sum_{k <= b} k h_k) / C(b), mu1 = (sum_{k > b} k h_k) / (T - C(b));
 *       score(b) = w0 (1 - w0) (mu0 - mu1)^2, and 0 where either side is empty. b is the smallest bin with the largest score;
 *       thr = (float)(h_lo + (b + 1) width).
 *   (b) Labels (paris_hip_bh_classify, device): the class of a voxel is object if v > thr, air if v <= thr, none if v is not finite.
 *       A voxel gets the label 2 (object) or 1 (air) iff every voxel within Chebyshev distance `margin` of it, along all three axes,
 *       has its class -- positions outside the slab count as differing -- and it lies inside the field of view,
 *       (2x - dim_x + 1)^2 + (2y - dim_y + 1)^2 <= (min(dim_x, dim_y) - 2)^2 in integers. Every other voxel gets 0. Voxels outside
 *       the field of view still lend their class to their neighbours. 0 <= margin <= PARIS_HIP_BH_MARGIN_MAX.
 *   (c) Gram matrix (paris_hip_bh_gram on the device, paris_hip_bh_gram_host): per labelled voxel g = (f_1 ... f_N, m), m = 1 for
 *       label 2 and 0 for label 1; G = sum g g^T, the upper triangle row by row: (N + 1)(N + 2) / 2 doubles, G[a][b] (a <= b) at
 *       a (N + 1) - a (a - 1) / 2 + (b - a). A labelled voxel where any f_k is not finite is skipped and counted. The order of the
 *       additions is fixed. With L = 65536 partial sums, voxel i (its 64-bit linear index) belongs to partial l = i mod L; within a
 *       partial voxels are taken in ascending i; each term is (double)a * (double)b, exact for two floats, added in double to an
 *       accumulator that starts at +0; then B_j = sum_m acc_{j + 256 m}, m ascending, for j = 0 ... 255, and G = sum_j B_j, j ascending.
 *       Counts: n_object and n_air are the voxels summed, n_not_finite those skipped, n_ignored the voxels with another label.
 *   (d) Solve (paris_hip_bh_solve, host): T = G[f_1][m] / n_object -- the mean of f_1 over the object's core, the FIXED template
 *       level. Minimise sum (sum c_k f_k - T m)^2 over c_1 ... c_N: A = G[1..N][1..N], b_i = T G[f_i][m], by Cholesky in double, each
 *       coefficient rounded once to float and used as solved (no normalisation by c_1). The rms residual relative to T,
 *       sqrt(max(0, c^T A c - 2 T c^T G[f][m] + T^2 n_object) / (n_object + n_air)) / |T|, is reported for c = e_1 (before) and for
 *       the rounded coefficients (after).
 * Limits: one material; no metal. */
#define PARIS_HIP_BH_DEGREE_MAX 4
#define PARIS_HIP_BH_MARGIN_MAX 4
#define PARIS_HIP_BH_HISTOGRAM_BINS 4096 /* what the fit asks paris_hip_volume_stats for */
#define PARIS_HIP_BH_PARTIALS 65536      /* L of the Gram sum */
#define PARIS_HIP_BH_MIN_VOXELS_DEFAULT 64
typedef struct paris_hip_beam_hardening {
    uint32_t degree;                  /* N: 1 .. PARIS_HIP_BH_DEGREE_MAX */
    float c[PARIS_HIP_BH_DEGREE_MAX]; /* c[0] = c_1 ... c[N - 1] = c_N, each finite; the rest is ignored */
} paris_hip_beam_hardening;
/* what paris_hip_bh_gram counts */
typedef struct paris_hip_bh_counts {
    uint64_t n_object;     /* voxels with label 2 that were summed */
    uint64_t n_air;        /* voxels with label 1 that were summed */
    uint64_t n_ignored;    /* voxels with any other label */
    uint64_t n_not_finite; /* labelled voxels skipped because an f_k is not finite */
} paris_hip_bh_counts;
/* what paris_hip_bh_solve returns */
typedef struct paris_hip_bh_fit {
    paris_hip_beam_hardening setting; /* the coefficients as solved */
    double level;                     /* T */
    double residual_before;           /* rms residual / |T| for c = e_1 */
    double residual_after;            /* the same for the fitted coefficients */
} paris_hip_bh_fit;
/* Host only, no ctx and no device. PARIS_HIP_ERROR_INVALID_ARGUMENT for a NULL setting, a degree outside 1 .. 4 or a c_k (k <= degree)
 * that is not finite. */
int paris_hip_beam_hardening_check(const paris_hip_beam_hardening* setting);
/* Host only: the rule on n dense pixels, src to dst (which may be the same array) -- the second implementation of the one definition.
 * PARIS_HIP_ERROR_INVALID_ARGUMENT as the check, or for a NULL src or dst with n != 0. */
int paris_hip_beam_hardening_host(const paris_hip_beam_hardening* setting, const float* src, float* dst, uint64_t n);
/* paris_hip_set_beam_hardening runs the check and keeps the setting for dim_x x dim_y frames (both >= 1); it travels to the kernel by
 * value, so work queued before a replacement keeps the old one and nothing lives on the device. Without a setting nothing else
 * changes. */
int paris_hip_set_beam_hardening(paris_hip_ctx* ctx, const paris_hip_beam_hardening* setting, uint32_t dim_x, uint32_t dim_y);
int paris_hip_clear_beam_hardening(paris_hip_ctx* ctx);
/* In place on float frames, asynchronous: every pixel of rows [row_first, row_first + row_count) of n_frames frames frame_stride bytes
 * apart, d_p the first frame's row 0, becomes q. 16-byte vectors are used where the base, the pitch, the stride (n_frames > 1) and
 * dim_x allow, single pixels otherwise. PARIS_HIP_ERROR_INVALID_ARGUMENT without a setting, when dim_x / dim_y differ from the
 * setting's, or for a band, pitch or stride paris_hip_flat_field_rows would refuse. */
int paris_hip_beam_hardening_rows(paris_hip_ctx* ctx, float* d_p, size_t pitch, size_t frame_stride, uint32_t n_frames, uint32_t dim_x,
                                  uint32_t dim_y, uint32_t row_first, uint32_t row_count);
/* The same with the setting as an argument (the ctx's, if any, is neither used nor changed): the fit forms p^k with the unit
 * settings e_k. PARIS_HIP_ERROR_INVALID_ARGUMENT as the check, or for a band, pitch or stride paris_hip_flat_field_rows would refuse. */
int paris_hip_beam_hardening_rows_with(paris_hip_ctx* ctx, const paris_hip_beam_hardening* setting, float* d_p, size_t pitch,
                                       size_t frame_stride, uint32_t n_frames, uint32_t dim_x, uint32_t dim_y, uint32_t row_first,
                                       uint32_t row_count);
/* Host only: (a). PARIS_HIP_ERROR_INVALID_ARGUMENT for a NULL pointer, n_bins == 0, a range paris_hip_volume_window_check's rules
 * refuse, or an empty histogram. */
int paris_hip_bh_threshold_from_histogram(const uint64_t* hist, uint32_t n_bins, float h_lo, float h_hi, float* thr);
/* (b), asynchronous on the ctx stream; what is deferred runs first. d_v: dim_x * dim_y * dim_z floats, 4-byte aligned; d_labels: as
 * many bytes, which must not overlap them and are treated as paris_hip_volume_mark_dirty treats a range.
 * PARIS_HIP_ERROR_INVALID_ARGUMENT for a NULL pointer, a zero dimension, a thr that is not finite, margin > PARIS_HIP_BH_MARGIN_MAX or
 * overlapping ranges; PARIS_HIP_ERROR_UNSUPPORTED for a slab beyond the grid's limits (more than 65535 tiles of 16 rows or of 8 slices). */
int paris_hip_bh_classify(paris_hip_ctx* ctx, const float* d_v, uint32_t dim_x, uint32_t dim_y, uint32_t dim_z, float thr, uint32_t margin,
                          uint8_t* d_labels);
/* (c), synchronous; what is deferred runs first. d_f: a host array of `degree` device pointers, f_1 first, each n_voxels floats;
 * d_labels: n_voxels bytes on the device; gram receives (degree + 1)(degree + 2) / 2 doubles. The partial sums live in device
 * memory the call allocates and frees. n_voxels == 0 gives zeros. PARIS_HIP_ERROR_INVALID_ARGUMENT for a NULL pointer, a degree
 * outside 1 .. 4 or a misaligned f_k. */
int paris_hip_bh_gram(paris_hip_ctx* ctx, const float* const* d_f, uint32_t degree, const uint8_t* d_labels, uint64_t n_voxels, double* gram,
                      paris_hip_bh_counts* counts);
/* Host only: the same definition on host arrays -- the second implementation. */
int paris_hip_bh_gram_host(const float* const* f, uint32_t degree, const uint8_t* labels, uint64_t n_voxels, double* gram,
                           paris_hip_bh_counts* counts);
/* Host only: (d). min_voxels == 0 stands for PARIS_HIP_BH_MIN_VOXELS_DEFAULT. PARIS_HIP_ERROR_INVALID_ARGUMENT for a NULL pointer or a
 * degree outside 1 .. 4; PARIS_HIP_ERROR_BH_TOO_FEW_VOXELS when n_object or n_air is below min_voxels;
 * PARIS_HIP_ERROR_BH_NOT_POSITIVE when a pivot is not positive (NaN included); PARIS_HIP_ERROR_BH_NOT_FINITE when T is zero or not
 * finite or a coefficient is not a finite float. *out is written on success only. */
int paris_hip_bh_solve(const double* gram, uint32_t degree, const paris_hip_bh_counts* counts, uint64_t min_voxels, paris_hip_bh_fit* out);
/* Extension (no reference counterpart): detector lag -- an a-Si flat panel carries a few per cent of every frame's signal over into
 * the following frames (afterglow), which blurs the volume azimuthally and draws tails behind dense edges. The correction is the
 * recursive deconvolution of a multi-exponential impulse response (Hsieh et al. 2000; for flat panels Starman et al. 2011; DESIGN.md
 * section 4.20). It is the one pass that carries per-pixel STATE from frame to frame: the frames of one pass over the scan form an
 * ordered sequence. One definition; the host function and the device give the same bits.
 * Setting paris_hip_lag_model { uint32_t terms; float b[4]; float a[4]; int start; }: N = terms in 1 .. 4, term n with the weight
 *   b_n > 0 and the decay rate per frame a_n > 0, both finite. The impulse response is h(k) = b_0 delta(k) + sum_n b_n exp(-a_n k),
 *   k >= 0, normalised to unit DC gain: b_0 = 1 - sum_n b_n / (1 - exp(-a_n)), and b_0 > 0 is required (in double). With every b_n > 0
 *   and b_0 > 0 the poles of the inverse filter lie in (0, 1) on the real axis.
 *   With B = b_0 + sum b_n and the state S_n,k = x_(k-1) + exp(-a_n) S_n,(k-1) the detector's forward model is
 *   y_k = B x_k + sum_n b_n exp(-a_n) S_n,k; the correction is its exact algebraic inverse.
 * Coefficients (paris_hip_lag_coefficients, the single implementation), each computed in double and rounded once to fp32:
 *   g_n = exp(-a_n), c_n = b_n g_n / B, invB = 1 / B, w_n = 1 / (1 - g_n).
 * Rule, per pixel and frame, in fp32, in this order, explicit fused multiply-adds and no contraction elsewhere:
 *   y = i - d             d: the ctx's dark pixel at the frame's absolute row and column when a flat-field setting is in force, else 0
 *                         (the host function: the caller's dark array, or 0 without one)
 *   first frame of a sequence, start = PARIS_HIP_LAG_START_STEADY: S_n = w_n * y for every n   (PARIS_HIP_LAG_START_REST: S_n = 0)
 *   acc = y * invB;  for n = 0 .. N-1: acc = fmaf(-c_n, S_n, acc);  x = acc
 *   for n = 0 .. N-1: S_n = fmaf(g_n, S_n, x)
 *   store x + d
 *   A pixel whose y is not finite is stored unchanged and its state advances with x = 0 (on a sequence's first frame from S_n = 0):
 *   one bad sample does not poison a pixel for the rest of the scan.
 *   STEADY: the beam was on and the first view had been seen for a long time -- how scans are taken.
 * Order. The pass runs on COUNTS: after the raw upload and the binning, before the dark / flat correction, which afterwards sees
 * x + d where it saw i. Every later pass is as it was. */
#define PARIS_HIP_LAG_TERMS_MAX 4
#define PARIS_HIP_LAG_START_REST 0
#define PARIS_HIP_LAG_START_STEADY 1
typedef struct paris_hip_lag_model {
    uint32_t terms;                   /* N: 1 .. PARIS_HIP_LAG_TERMS_MAX */
    float b[PARIS_HIP_LAG_TERMS_MAX]; /* the weights b_n > 0; the rest is ignored */
    float a[PARIS_HIP_LAG_TERMS_MAX]; /* the decay rates per frame a_n > 0; the rest is ignored */
    int start;                        /* PARIS_HIP_LAG_START_REST or PARIS_HIP_LAG_START_STEADY */
} paris_hip_lag_model;
/* Host only, no ctx and no device. PARIS_HIP_ERROR_INVALID_ARGUMENT for a NULL model, terms outside 1 .. 4, a b_n or a_n (n < terms)
 * that is not finite or not > 0, b_0 <= 0, or an unknown start. */
int paris_hip_lag_model_check(const paris_hip_lag_model* model);
/* Host only: the one place the coefficients are derived (the device path calls it too). g, c and w receive 4 floats each, those
 * from `terms` on are 0; inv_b and b0 (the latter in double) may be NULL. PARIS_HIP_ERROR_INVALID_ARGUMENT as the check, or for a NULL
 * g, c or w. */
int paris_hip_lag_coefficients(const paris_hip_lag_model* model, float g[4], float c[4], float w[4], float* inv_b, double* b0);
/* Host only: the rule on n_frames dense frames of n_pixels pixels each, in time order, in place -- the second implementation of the
 * one definition. dark: n_pixels floats or NULL (zero). state: terms x n_pixels floats, planar per term, which the caller keeps
 * between calls; *started: 0 before frame 0 of the sequence (the state's contents are then ignored), set to 1 by the first frame.
 * Calls that split a sequence anywhere give the bits of one call. PARIS_HIP_ERROR_INVALID_ARGUMENT as the check, or for a NULL
 * frames, state or started with work to do. */
int paris_hip_lag_correct_host(const paris_hip_lag_model* model, const float* dark_or_null, float* frames, float* state, int* started,
                               uint64_t n_pixels, uint32_t n_frames);
/* Both run the check, then whatever is deferred, and close an open sequence. The model travels to the kernel by value. Without a
 * setting nothing else changes. */
int paris_hip_set_lag_correction(paris_hip_ctx* ctx, const paris_hip_lag_model* model);
int paris_hip_clear_lag_correction(paris_hip_ctx* ctx);
/* Opens the sequence of one band, rows [row_first, row_first + row_count) of dim_x x dim_y frames: one open sequence per ctx. The
 * band's state -- terms x row_count x dim_x floats, planar per term, rows dense -- is allocated, zeroed on the compute stream and
 * counts towards paris_hip_projection_reserve_bytes while the sequence is open; the frame counter starts at 0.
 * PARIS_HIP_ERROR_INVALID_ARGUMENT without a setting, when a flat-field setting has other dimensions than dim_x x dim_y, for a zero or
 * out-of-frame band, or while a sequence is open. */
int paris_hip_lag_begin(paris_hip_ctx* ctx, uint32_t dim_x, uint32_t dim_y, uint32_t row_first, uint32_t row_count);
/* Closes the sequence; its state is freed once no queued work can touch it. Without an open sequence: no error. */
int paris_hip_lag_end(paris_hip_ctx* ctx);
/* In place on float frames of counts, asynchronous: the rule on the band's rows of n_frames frames frame_stride bytes apart, d_p the
 * first frame's row 0. The call's frames are consecutive in time and follow the previous call's; the frame counter advances by
 * n_frames. 16-byte vectors are used where the base, the pitch, the stride (n_frames > 1) and dim_x allow, single pixels otherwise.
 * PARIS_HIP_ERROR_INVALID_ARGUMENT without an open sequence, when dim_x, dim_y or the band differ from the begun ones (a pass over other
 * rows would leave their state stale), or for a pitch or stride paris_hip_flat_field_rows would refuse. */
int paris_hip_lag_correct_rows(paris_hip_ctx* ctx, float* d_p, size_t pitch, size_t frame_stride, uint32_t n_frames, uint32_t dim_x,
                               uint32_t dim_y, uint32_t row_first, uint32_t row_count);
/* The open sequence's frame counter (0 without one). PARIS_HIP_ERROR_INVALID_ARGUMENT for a NULL argument. */
int paris_hip_lag_frames(paris_hip_ctx* ctx, uint64_t* frames);
/* Extension (no reference counterpart): metal artefact reduction by linear interpolation (LI-MAR; Kalender et al. 1987; DESIGN.md
 * section 4.21). Metal drives its rays to the detector's floor; the ramp filter spreads that non-linearity as streaks. The remedy:
 * reconstruct once, take the metal voxels out of the volume (1), forward-project their mask and mark where it casts a shadow -- the
 * metal TRACE (2) --, replace the trace's pixels of every frame by linear interpolation along the row before the row filter (3),
 * reconstruct again and put the metal voxels back (4). Each of the four has ONE definition; the host function and the device give
 * the same bits.
 * (1) collect: every voxel with v > threshold (a NaN compares false), in ascending linear index (z * dim_y + y) * dim_x + x, with its
 *     value. With binarize != 0 the volume then becomes the mask: 1.0f where a voxel was reported, 0.0f elsewhere. More than max_n
 *     hits: nothing is written, neither the lists nor the volume, *n still holds the count, PARIS_HIP_ERROR_METAL_TOO_MANY_VOXELS.
 * (2) pack: pixel (x, y) of a frame is in the trace when any pixel (x', y') of that frame with |x' - x| <= grow and |y' - y| <= grow,
 *     the window clipped to the frame, has t > min_path (a NaN compares false); grow in 0 .. PARIS_HIP_METAL_GROW_MAX. Layout:
 *     words = (dim_x + 63) / 64 uint64_t per row, pixel x is bit x & 63 of word x >> 6, rows in order, frame f from word
 *     f * dim_y * words; the bits at and beyond dim_x are 0.
 * (3) inpaint: in every row of the band, for every maximal run [a, b] of set bits, with pL = p[a - 1] and pR = p[b + 1] as stored:
 *       interior run:  t = (float)(x - (a - 1)) / (float)(b - a + 2)  (one fp32 division);  p[x] = fmaf(t, pR - pL, pL)
 *       a = 0:  p[x] = pR;    b = dim_x - 1:  p[x] = pL;    both: the row is left as it is.
 *     Anchors that are not finite propagate by this arithmetic (which payload a resulting NaN carries is left open). Pixels outside
 *     the trace are not written. Counted: the pixels
 *     replaced, the runs replaced, and the rows left because the trace covers them whole.
 * (4) reinsert: every listed voxel whose index falls into a slab gets its listed value; nothing else is written.
 * Order. The inpainting runs on line integrals on the ideal detector -- after the detector roll, before the redundancy and cosine
 * weights. */
#define PARIS_HIP_METAL_GROW_MAX 4
#define PARIS_HIP_METAL_MIN_VOXELS_CAP 1024
typedef struct paris_hip_metal_counts {
    uint64_t replaced;  /* pixels replaced */
    uint64_t runs;      /* runs replaced */
    uint64_t rows_left; /* rows left as they were because the trace covers them whole */
} paris_hip_metal_counts;
/* Host only, no ctx and no device: the checks every entry point below shares, and the cap on the list a threshold may mark --
 * *max_voxels (may be NULL) = max(PARIS_HIP_METAL_MIN_VOXELS_CAP, dim_x * dim_y * dim_z / 32): a threshold that marks more is a wrong
 * threshold, not metal. PARIS_HIP_ERROR_INVALID_ARGUMENT for a zero dimension, a threshold that is not finite, grow >
 * PARIS_HIP_METAL_GROW_MAX, or a min_path that is negative or not finite. */
int paris_hip_metal_check(uint32_t dim_x, uint32_t dim_y, uint32_t dim_z, float threshold, uint32_t grow, float min_path,
                          uint64_t* max_voxels);
/* Host only: (1) on a host volume. index and value receive up to max_n entries (either may be NULL when max_n == 0).
 * PARIS_HIP_ERROR_INVALID_ARGUMENT for a NULL v or n, a zero dimension or a threshold that is not finite. */
int paris_hip_metal_collect_host(float* v, uint32_t dim_x, uint32_t dim_y, uint32_t dim_z, float threshold, uint64_t max_n,
                                 uint64_t* index, float* value, uint64_t* n, int binarize);
/* (1) on a device volume, synchronous; what is deferred runs first. h_index and h_value are host arrays. The scratch -- a count per
 * 4096 voxels, their exclusive scan and the lists -- lives in device memory the call allocates and frees. A binarized volume is
 * treated as paris_hip_volume_mark_dirty treats a range. Errors as the host function's. */
int paris_hip_metal_collect(paris_hip_ctx* ctx, float* d_v, uint32_t dim_x, uint32_t dim_y, uint32_t dim_z, float threshold, uint64_t max_n,
                            uint64_t* h_index, float* h_value, uint64_t* n, int binarize);
/* Host only: (2) on n_frames dense frames of dim_x x dim_y floats. PARIS_HIP_ERROR_INVALID_ARGUMENT for a NULL pointer with work to do,
 * grow > PARIS_HIP_METAL_GROW_MAX, or a min_path that is negative or not finite. */
int paris_hip_metal_trace_pack_host(const float* t, uint32_t n_frames, uint32_t dim_x, uint32_t dim_y, float min_path, uint32_t grow,
                                    uint64_t* bits);
/* (2) on device frames frame_stride bytes apart with rows pitch bytes apart, synchronous: h_bits, a host array, receives
 * n_frames * dim_y * words words. A held-back weighting runs first, and a frame of the pending by-reference group has that group
 * launched first. The packed words pass through device memory the call allocates and frees. Errors as the host function's, or for
 * a pitch or stride paris_hip_flat_field_rows would refuse. */
int paris_hip_metal_trace_pack(paris_hip_ctx* ctx, const float* d_t, size_t pitch, size_t frame_stride, uint32_t n_frames, uint32_t dim_x,
                               uint32_t dim_y, float min_path, uint32_t grow, uint64_t* h_bits);
/* Host only: (3) on the rows [row_first, row_first + row_count) of one dense dim_x x dim_y frame, with the dim_y * words words of its
 * trace; adds to *counts (may be NULL). PARIS_HIP_ERROR_INVALID_ARGUMENT for a NULL p or bits with work to do or a band outside the
 * frame. */
int paris_hip_metal_inpaint_host(float* p, const uint64_t* bits, uint32_t dim_x, uint32_t dim_y, uint32_t row_first, uint32_t row_count,
                                 paris_hip_metal_counts* counts);
/* The traces of all n_views views of a scan on dim_x x dim_y frames, in the layout of (2), as a setting of the ctx: 64 bytes of
 * counters, then n_views * dim_y * words words on the device, which count towards paris_hip_projection_reserve_bytes while set;
 * paris_hip_ctx_destroy frees them. Replaces an earlier setting and its counts safely: work already queued keeps the old one.
 * PARIS_HIP_ERROR_INVALID_ARGUMENT for a NULL h_bits or a zero n_views or dimension. Without a setting nothing else changes. */
int paris_hip_set_metal_trace(paris_hip_ctx* ctx, const uint64_t* h_bits, uint32_t n_views, uint32_t dim_x, uint32_t dim_y);
int paris_hip_clear_metal_trace(paris_hip_ctx* ctx);
/* (3) in place on float frames, asynchronous: the band's rows of n_frames frames frame_stride bytes apart, d_p the first frame's row
 * 0; frame f is inpainted with the trace of view h_view[f] (a host array, read before the call returns). A row without a set bit
 * costs the read of its words. The pass reads no row outside the band. PARIS_HIP_ERROR_INVALID_ARGUMENT without a setting, when
 * dim_x / dim_y differ from the setting's, for a NULL h_view or an h_view[f] >= n_views, or for a band, pitch or stride
 * paris_hip_flat_field_rows would refuse. */
int paris_hip_metal_inpaint_rows(paris_hip_ctx* ctx, float* d_p, size_t pitch, size_t frame_stride, uint32_t n_frames, uint32_t dim_x,
                                 uint32_t dim_y, uint32_t row_first, uint32_t row_count, const uint32_t* h_view);
/* The counts since paris_hip_set_metal_trace or the last reset; waits for the work queued on the ctx stream that still adds to them
 * and reads them; reset != 0 zeroes them afterwards. PARIS_HIP_ERROR_INVALID_ARGUMENT without a setting or for a NULL out. */
int paris_hip_metal_stats(paris_hip_ctx* ctx, paris_hip_metal_counts* out, int reset);
/* The list of (1) as a setting of the ctx: n indices, strictly ascending, and their values, copied to the device (12 bytes per
 * voxel, counted towards paris_hip_projection_reserve_bytes while set) and, the indices, kept on the host. n == 0 is a setting
 * without memory. PARIS_HIP_ERROR_INVALID_ARGUMENT for a NULL array with n != 0 or indices that do not ascend strictly. */
int paris_hip_set_metal_voxels(paris_hip_ctx* ctx, const uint64_t* h_index, const float* h_value, uint64_t n);
int paris_hip_clear_metal_voxels(paris_hip_ctx* ctx);
/* (4), asynchronous: d_v holds slices [v_offset, v_offset + v_dim_z) of a grid of dim_x x dim_y voxels per slice; the slab's part of
 * the list is found by bisection on the host. What is deferred into a volume runs first, as for paris_hip_volume_stats; a slab
 * written into is treated as paris_hip_volume_mark_dirty treats a range. PARIS_HIP_ERROR_INVALID_ARGUMENT without a setting, for a
 * NULL d_v or a zero dim_x or dim_y. */
int paris_hip_metal_reinsert(paris_hip_ctx* ctx, float* d_v, uint32_t dim_x, uint32_t dim_y, uint32_t v_dim_z, uint32_t v_offset);
/* Extension (no reference counterpart): row extension for laterally truncated projections -- the object is wider than the detector,
 * "interior" or region-of-interest tomography. The row filter zero-pads every row, as the reference does;
 * a truncated row then steps from its edge value to 0 and the ramp answers with a bright rim and cupping. With a setting the filter
 * acts as if each row q (n = dim_x pixels, as the transform sees it) continued to the left as a * t(k) and to the right as b * t(k),
 * k = 1 .. W pixels beyond the edge. No extended signal is built: the filter is linear, so the filtered extended row, restricted to
 * the detector, is the zero-padded result plus a rank-2 update,
 *   out[s] = F(q)[s] + a * c[s] + b * c[n - 1 - s],
 * with ONE vector c per (n, tau, W), computed on the host. It has no circular wrap, whatever the taper length.
 *   setting  edge_pixels m in {1, 2, 4, 8}, taper_pixels W in [1, 16384];
 *   kernel   g[d] = -1 / (2 pi^2 d^2 tau) for odd d >= 1, 0 for even d >= 2 (g[0] is not used): the spatial kernel of the
 *            reference's ramp (make_filter_real, src/openmp/filtering.cpp:52-73) times tau;
 *   taper    t(k) = cos^2(pi k / (2 (W + 1))), k = 1 .. W;
 *   response c[s] = sum_{k = 1 .. W} t(k) * g[s + k], s = 0 .. n - 1, summed in double in ascending k and rounded once to fp32;
 *            it depends on n, tau and W only. c <= 0 everywhere. g vanishes at even distances, so c is two interleaved
 *            sequences, even s and odd s: each increases towards 0, but c is not monotone from one s to the next, and with
 *            W = 1 every odd c[s] is exactly 0;
 *   means    a = ((q[0] + q[1]) + ...) * (1 / m) over the first m pixels, b the same over the last m pixels in ascending index: a
 *            sequential fp32 sum followed by an exact scaling. q is the row as the transform sees it: after the cosine weight when
 *            the weight rides in the load, the stored pixels otherwise. dim_x < m is PARIS_HIP_ERROR_INVALID_ARGUMENT;
 *   store    with y the value the plain filter stores (v * (1 / filter_size)), the stored pixel is
 *            fmaf(b, c[n - 1 - s], fmaf(a, c[s], y)); the half-precision output is that fp32 value rounded to nearest even.
 * Rows whose a and b are both 0 are therefore bit-identical to the plain filter's -- an untruncated scan with m = 1 is unchanged.
 * c is always the plain ramp's response, also for a Shepp-Logan K. That is a limit, not an equivalence: the window changes the
 * kernel's nearest taps most, so the windowed response differs from c by 0.19 of max|c| at s = 0, 0.08 and 0.03 at s = 1 and 2, and
 * by less than 0.003 from s = 8 (n = 2048, W = 512) -- with a Shepp-Logan K the outermost 2 to 3 pixels of a
 * truncated row carry that error. tau is the one the K was made with: with a setting in force a filter call with a K this ctx did not make is PARIS_HIP_ERROR_UNSUPPORTED.
 * Known limit: a low-frequency offset remains inside the field of view, and longer tapers are not better. */
typedef struct paris_hip_row_extension {
    uint32_t edge_pixels;  /* m: pixels averaged at either end of a row: 1, 2, 4 or 8 */
    uint32_t taper_pixels; /* W: length of the cos^2 taper beyond either end, 1 .. 16384 */
} paris_hip_row_extension;
/* Host only, no ctx. PARIS_HIP_ERROR_INVALID_ARGUMENT for a NULL setting, m outside {1, 2, 4, 8}, W outside [1, 16384], dim_x == 0 or
 * dim_x < m. */
int paris_hip_row_extension_check(const paris_hip_row_extension* setting, uint32_t dim_x);
/* Host only: c[0 .. dim_x) as stated above -- the single implementation of c; the device copies are made from it.
 * PARIS_HIP_ERROR_INVALID_ARGUMENT as the check, for a tau that is not finite or <= 0, or a NULL c. */
int paris_hip_row_extension_response(const paris_hip_row_extension* setting, uint32_t dim_x, float tau, float* c);
/* Both first run whatever is held back or pending -- a held-back weighting or filter, the pending backprojection group -- so no row
 * queued before the call sees the change. From then on every filter path honours the setting: paris_hip_apply_filter (with a
 * held-back weighting fused into its load or not, the radix-16 and the radix-2 kernel), paris_hip_weight_filter_rows / _batch, the
 * paris_hip_stage_* forms, the half-precision output and filter deferral. The device copies of c are made on first use and cached
 * per (dim_x, tau, W); they count towards paris_hip_projection_reserve_bytes while set, are freed once the work queued before a
 * set / clear no longer reads them, and by paris_hip_ctx_destroy. Without a setting nothing changes.
 * paris_hip_set_row_extension: PARIS_HIP_ERROR_INVALID_ARGUMENT for a NULL ctx or a setting the check refuses for dim_x = 8. */
int paris_hip_set_row_extension(paris_hip_ctx* ctx, const paris_hip_row_extension* setting);
int paris_hip_clear_row_extension(paris_hip_ctx* ctx);
/* paris::backproject (src/backprojection.cpp:37-69): p_idx / p_phi are projection::idx / projection::phi */
int paris_hip_stage_backproject(paris_hip_ctx* ctx, const float* d_p, size_t p_pitch, uint32_t p_dim_x,
                                uint32_t p_dim_y, uint32_t p_idx, float p_phi, float* d_v, uint32_t v_dim_x,
                                uint32_t v_dim_y, uint32_t v_dim_z, uint32_t v_offset,
                                const paris_detector_geometry* det_geo, const paris_volume_geometry* vol_geo,
                                int enable_angles, int enable_roi, const paris_region_of_interest* roi);

/* ---- forward projection (extension, no reference counterpart) -------------------------------------------
 * The cone-beam projections of a volume on the device, in the backprojector's geometry, by Joseph's method: every detector pixel
 * casts one ray from the source to its centre, sampled once per voxel plane along the axis (x or y) it runs more nearly parallel
 * to, bilinearly in that plane. There is no step size: the result is fully defined. For a view with s = sin_phi[f], c = cos_phi[f],
 * d_sd = |d_so| + |d_od| and delta_s, delta_t in mm as paris_hip_backproject receives them:
 *   pixel (i, j), column i in [0, n_row), row j in [0, n_col):
 *     t = (i + 1/2) l_px_row - n_row l_px_row / 2 - delta_s,   z = (j + 1/2) l_px_col - n_col l_px_col / 2 - delta_t
 *     source S = (-d_so c, -d_so s, 0),   ray direction (dx, dy, dz) = (d_sd c - t s, d_sd s + t c, z)
 *   x-marching when |dx| >= |dy|, else y-marching (the same statement with x and y exchanged):
 *     for every plane K in [0, vol_geo->dim_x):  x_K = -(dim_x l_vx_x / 2) + l_vx_x / 2 + K l_vx_x
 *       a = (x_K - S_x) / dx;  planes with a <= 0 or a > 1 (not between source and detector) add nothing
 *       y = S_y + a dy,  w = a dz
 *       fy = (y + dim_y l_vx_y / 2) / l_vx_y - 1/2,  fz = (w + dim_z l_vx_z / 2) / l_vx_z - 1/2   (dim_* of the full grid vol_geo)
 *       sample = bilinear over the taps (floor fy, floor fz), (+1, .), (., +1), (+1, +1) of plane K; a tap outside the grid, or
 *                outside the slab [v_offset, v_offset + v_dim_z), counts as 0 on its own
 *     p(i, j) = (sum_K sample_K) l_vx_x sqrt(dx^2 + dy^2 + dz^2) / |dx|
 * What is done once per ray (t, z, the direction, the choice of the marching axis with dx and dy exactly as written, the length
 * factor, the per-plane increments) is formed in double from the fp32 arguments; the per-plane work is fp32.
 * d_v is a z-slab of the grid vol_geo, as in paris_hip_backproject: v_dim_x, v_dim_y equal vol_geo's, v_dim_z slices from global
 * slice v_offset. The projections of disjoint slabs add up to the whole volume's (to fp32 rounding). No ROI form.
 * View f is written at d_p + f * p_stride_bytes (p_pitch bytes per row; only the p_dim_x floats of a row are written). With
 * accumulate != 0 the finished ray sum is added to the stored pixel in one fp32 addition instead. sin_phi / cos_phi are host
 * arrays of n_views. PARIS_HIP_ERROR_INVALID_ARGUMENT for null pointers, p_dim_x != n_row or p_dim_y != n_col, p_pitch <
 * 4 * p_dim_x or not a multiple of 4, overlapping frames (n_views > 1 with p_stride_bytes < p_pitch * p_dim_y), v_dim_x / v_dim_y
 * other than vol_geo's, v_offset + v_dim_z > vol_geo->dim_z, a pixel or voxel size <= 0, d_so <= 0, or a value that is not finite.
 * n_views == 0, or v_dim_z == 0 with accumulate, does nothing; v_dim_z == 0 without it writes zeros.
 * The call reads a volume and writes projection buffers: what is deferred (backprojections into any volume, a held-back
 * weighting) runs first, and a destination the pending by-reference group refers to has that group launched first. */
int paris_hip_forward_project(paris_hip_ctx* ctx, const float* d_v, uint32_t v_dim_x, uint32_t v_dim_y, uint32_t v_dim_z,
                              uint32_t v_offset, const paris_detector_geometry* det_geo, const paris_volume_geometry* vol_geo,
                              float* d_p, size_t p_pitch, size_t p_stride_bytes, uint32_t n_views, uint32_t p_dim_x,
                              uint32_t p_dim_y, const float* sin_phi, const float* cos_phi, float delta_s, float delta_t,
                              int accumulate);
/* One view, its angle from p_idx / p_phi exactly as paris_hip_stage_angle gives it and delta_s l_px_row, delta_t l_px_col in fp32
 * as paris_hip_stage_backproject derives them */
int paris_hip_stage_forward_project(paris_hip_ctx* ctx, const float* d_v, uint32_t v_dim_x, uint32_t v_dim_y, uint32_t v_dim_z,
                                    uint32_t v_offset, const paris_detector_geometry* det_geo, const paris_volume_geometry* vol_geo,
                                    float* d_p, size_t p_pitch, uint32_t p_dim_x, uint32_t p_dim_y, uint32_t p_idx, float p_phi,
                                    int enable_angles, int accumulate);

/* ---- volume export (extension, no reference counterpart): 8- or 16-bit voxels over a grey window ---------
 * A finished volume leaves the device as unsigned integers quantised over a chosen window [lo, hi], 1 or 2 bytes per voxel instead
 * of 4, and the statistics a window is chosen from -- extremes and a histogram -- are taken on the device.
 * Setting paris_hip_volume_window { float lo; float hi; int voxel_type; }.
 *   voxel_type is PARIS_HIP_VOXEL_U8 with L = 255, or PARIS_HIP_VOXEL_U16 with L = 65535.
 * Quantise.
 *   scale = (float)(L / ((double)hi - (double)lo)), rounded once.
 *   Per voxel v, in fp32, each operation rounded once and no contraction: x = (v - lo) * scale.
 *   q = 0 when v is NaN or x <= 0.
 *   q = L when x >= L.
 *   Otherwise q = rint(x): to nearest, ties to even.
 *   So +inf gives L, -inf gives 0, and +0 and -0 behave alike. u16 is stored as the machine stores it, little-endian.
 * Counts are 64-bit and accumulated per ctx until reset.
 *   voxels is the number of voxels examined.
 *   below is the number of finite voxels with v < lo, above the number of finite voxels with v > hi.
 *   not_finite counts NaN, +inf and -inf.
 * Check (paris_hip_volume_window_check) refuses a NULL setting, an unknown type, a lo or hi that is not finite, hi <= lo,
 *   (double)hi - lo < 2^-100, and a scale that is not finite.
 * Stats look at finite voxels only.
 *   min and max are the extremes of the finite voxels; without one, min = +inf and max = -inf. The sign of a zero extreme is
 *   unspecified.
 *   not_finite counts the others.
 *   Optionally a linear histogram of n_bins counters, 1 <= n_bins <= PARIS_HIP_VOLUME_HISTOGRAM_BINS_MAX, over [h_lo, h_hi], which
 *   the check's rules apply to with n_bins in the place of L:
 *     bscale = (float)(n_bins / ((double)h_hi - h_lo)).
 *     A finite v with h_lo <= v <= h_hi goes to bin min(n_bins - 1, (uint32_t)((v - h_lo) * bscale)): fp32 operations, and the
 *     conversion truncates (a product beyond every bin, +inf included, lands in the last bin).
 *     Finite voxels outside the range count as below or above.
 *   All counters are integers, so no result depends on the order of the device's atomics.
 * Window from a histogram (paris_hip_volume_window_from_histogram), on the host, the single implementation. It needs
 *   0 <= p_lo < p_hi <= 100. Everything is computed in double and rounded once.
 *   T is the sum of the bins, width = ((double)h_hi - h_lo) / n_bins, C(b) the inclusive cumulative count.
 *   b_lo is the smallest b with C(b) > T * p_lo / 100, and w_lo = (float)(h_lo + b_lo * width).
 *   b_hi is the smallest b with C(b) >= T * p_hi / 100, and w_hi = (float)(h_lo + (b_hi + 1) * width).
 *   (Where rounding leaves no such b, it is the last bin.) T == 0 is PARIS_HIP_ERROR_INVALID_ARGUMENT. */
#define PARIS_HIP_VOXEL_U8 1
#define PARIS_HIP_VOXEL_U16 2
#define PARIS_HIP_VOLUME_HISTOGRAM_BINS_MAX 4096
typedef struct paris_hip_volume_window {
    float lo;       /* the voxel value stored as 0 */
    float hi;       /* the voxel value stored as L; > lo */
    int voxel_type; /* PARIS_HIP_VOXEL_U8 or PARIS_HIP_VOXEL_U16 */
} paris_hip_volume_window;
/* what paris_hip_volume_quantize_counts reports */
typedef struct paris_hip_volume_counts {
    uint64_t voxels;     /* voxels examined */
    uint64_t below;      /* finite voxels below lo (stored as 0) */
    uint64_t above;      /* finite voxels above hi (stored as L) */
    uint64_t not_finite; /* NaN and +-inf */
} paris_hip_volume_counts;
/* what paris_hip_volume_stats reports */
typedef struct paris_hip_volume_statistics {
    float min;           /* of the finite voxels; +inf without one */
    float max;           /* of the finite voxels; -inf without one */
    uint64_t below;      /* finite voxels below h_lo (0 without a histogram) */
    uint64_t above;      /* finite voxels above h_hi (0 without a histogram) */
    uint64_t not_finite; /* NaN and +-inf */
    uint64_t voxels;     /* voxels examined */
} paris_hip_volume_statistics;
/* Host only, no ctx and no device. */
int paris_hip_volume_window_check(const paris_hip_volume_window* setting);
/* Host only: hist is n_bins counters over [h_lo, h_hi], p_lo and p_hi are percentiles. PARIS_HIP_ERROR_INVALID_ARGUMENT for a NULL
 * pointer, n_bins == 0, a range the check refuses, percentiles outside 0 <= p_lo < p_hi <= 100, or an empty histogram. The window
 * it returns still has to pass paris_hip_volume_window_check: both ends may round to one float. */
int paris_hip_volume_window_from_histogram(const uint64_t* hist, uint32_t n_bins, float h_lo, float h_hi, double p_lo, double p_hi,
                                           float* w_lo, float* w_hi);
/* Quantises the n_voxels floats at d_v into d_q (n_voxels bytes, or 2 n_voxels), device to device, on the ctx stream, and adds to
 * the ctx's counts. What is deferred runs first. [d_q, d_q + bytes) is treated as paris_hip_volume_mark_dirty treats it: the
 * destination may be memory of paris_hip_malloc_volume, and it now holds arbitrary bits. Aligned or not: 16-byte vectors are used
 * where source and destination reach a 16-byte boundary at the same voxel, single voxels otherwise.
 * PARIS_HIP_ERROR_INVALID_ARGUMENT for null pointers, a setting the check refuses, a d_v that is not 4-byte aligned, a u16 d_q that
 * is not 2-byte aligned, or a destination range that overlaps the source range. n_voxels == 0 does nothing. */
int paris_hip_volume_quantize(paris_hip_ctx* ctx, const float* d_v, uint64_t n_voxels, const paris_hip_volume_window* setting, void* d_q);
/* The same into a scratch the ctx owns, followed by an asynchronous copy of the bytes to h_q (pinned memory, to overlap anything)
 * on the ctx stream: the host reads h_q after paris_hip_ctx_synchronize or a fence. The scratch grows on demand and is reused --
 * stream order makes one enough; it counts towards paris_hip_projection_reserve_bytes while it exists and paris_hip_ctx_destroy
 * frees it. */
int paris_hip_volume_quantize_d2h(paris_hip_ctx* ctx, const float* d_v, uint64_t n_voxels, const paris_hip_volume_window* setting,
                                  void* h_q);
/* The counts of the ctx's quantise calls since it was created or last reset: runs what is pending, waits for the ctx stream and
 * reads them; reset != 0 zeroes them afterwards. PARIS_HIP_ERROR_INVALID_ARGUMENT for a NULL out. */
int paris_hip_volume_quantize_counts(paris_hip_ctx* ctx, paris_hip_volume_counts* out, int reset);
/* Synchronous: runs what is deferred, examines the n_voxels floats at d_v (4-byte aligned) on the device and returns the results
 * to the host. n_bins == 0: no histogram, h_lo / h_hi are ignored, hist may be NULL. Otherwise hist receives n_bins counters.
 * PARIS_HIP_ERROR_INVALID_ARGUMENT for a NULL d_v or out, n_bins beyond the maximum, a NULL hist or a refused range with
 * n_bins != 0. n_voxels == 0 gives the empty result. */
int paris_hip_volume_stats(paris_hip_ctx* ctx, const float* d_v, uint64_t n_voxels, float h_lo, float h_hi, uint32_t n_bins,
                           uint64_t* hist, paris_hip_volume_statistics* out);

/* ---- volume denoising (extension, no reference counterpart): edge-preserving 3-D bilateral filter ---------
 * The library's only neighbourhood operation on a volume (volume_bilateral.hip, bilateral_rule.cpp).
 * Setting struct paris_hip_volume_bilateral { float sigma_r; float sigma_s; uint32_t radius; } -- the entry point has the same name,
 *   so the type is always written with its `struct` keyword.
 *   sigma_r is in the volume's own units.
 *   sigma_s is in VOXELS, the same along x, y and z: the filter works on the grid, not in millimetres (a grid with unequal voxel edges
 *   is smoothed by the same number of voxels along each axis).
 *   radius is r, 1 <= r <= PARIS_HIP_BILATERAL_RADIUS_MAX: the stencil is (2r + 1)^3 taps.
 * Check (paris_hip_volume_bilateral_check) refuses a NULL setting, a sigma that is not finite or not greater than 0, a radius
 *   outside 1 .. 3, and a sigma_r for which rscale (below) is not finite or is 0.
 * Tables, made on the host in double and rounded once to fp32 (paris_hip_volume_bilateral_tables returns them):
 *   spatial s[dz][dy][dx] = exp(-(dx^2 + dy^2 + dz^2) / (2 sigma_s^2)) for offsets in [-r, r], dx fastest;
 *   range R[i] = exp(-0.5 ((i + 0.5) * 4 / 1024)^2), PARIS_HIP_BILATERAL_BINS = 1024 entries over [0, 4 sigma_r) sampled at bin centres;
 *   rscale = (float)(1024 / (4 (double)sigma_r)).
 *   R departs from the exact Gaussian by at most (2 / 1024) e^-1/2 < 0.0012 in weight inside the cutoff of 4 sigma_r and by at most
 *   e^-8 beyond it, where a tap gets no weight at all.
 * Rule for an output voxel c with the value v_c. Its taps n are walked in the order dz, then dy, then dx, each ascending from -r, the
 *   centre included, with num = den = 0 at the start. Every operation is fp32, rounded once, never contracted:
 *     a tap outside the source buffer in x, y or z is skipped;
 *     d = fabsf(v_n - v_c), t = d * rscale;
 *     the tap contributes only if t < 1024.f -- false for NaN, so neighbours that are not finite drop out;
 *     w = s[dz][dy][dx] * R[(uint32_t)t], num = num + w * v_n, den = den + w;
 *   out = num / den with the IEEE division; den > 0 because the centre always contributes.
 *   A centre that is not finite is written as stored. The device evaluates no transcendental function.
 * The device gives the bits of paris_hip_volume_bilateral_host, so a volume filtered in chunks of slices equals the volume filtered
 * whole when every chunk sees its halo of r source slices.
 * A result CAN be -0: a negative num of a few denormal steps divided by a den above 1 rounds to -0 (and a centre that is not finite
 * is copied). The destination is therefore treated as paris_hip_volume_mark_dirty treats a range. */
#define PARIS_HIP_BILATERAL_BINS 1024
#define PARIS_HIP_BILATERAL_RADIUS_MAX 3
struct paris_hip_volume_bilateral {
    float sigma_r;   /* range sigma, the volume's units; finite, > 0 */
    float sigma_s;   /* spatial sigma, voxels; finite, > 0 */
    uint32_t radius; /* r: 1 .. PARIS_HIP_BILATERAL_RADIUS_MAX */
};
/* Host only, no ctx and no device. */
int paris_hip_volume_bilateral_check(const struct paris_hip_volume_bilateral* setting);
/* Host only: spatial receives (2r + 1)^3 floats, range PARIS_HIP_BILATERAL_BINS floats, *rscale the scale. Any of the three may be
 * NULL. PARIS_HIP_ERROR_INVALID_ARGUMENT for a setting the check refuses. */
int paris_hip_volume_bilateral_tables(const struct paris_hip_volume_bilateral* setting, float* spatial, float* range, float* rscale);
/* Host only: the rule on host arrays. src is dim_x x dim_y x src_dim_z floats, x fastest; slices [z_first, z_first + z_count) are
 * filtered into the z_count slices at dst. Refuses what the device function refuses. */
int paris_hip_volume_bilateral_host(const float* src, uint32_t dim_x, uint32_t dim_y, uint32_t src_dim_z, uint32_t z_first, uint32_t z_count,
                                    const struct paris_hip_volume_bilateral* setting, float* dst);
/* Filters slices [z_first, z_first + z_count) of the source buffer d_src (dim_x x dim_y x src_dim_z floats) into z_count slices at
 * d_dst, on the ctx stream. What is deferred runs first. A z tap outside [0, src_dim_z) is skipped: where the grid continues beyond
 * the buffer the caller supplies the halo slices and leaves them out of [z_first, z_first + z_count). The tables of the setting are
 * uploaded when it differs from the one last used, owned by the ctx (the replaced ones are retired behind queued work), counted in
 * paris_hip_projection_reserve_bytes and freed by paris_hip_ctx_destroy. The destination is treated as
 * paris_hip_volume_mark_dirty treats a range (above: -0 can be produced). Aligned or not: the source is read as 16-byte vectors where
 * its base and dim_x allow, voxel by voxel otherwise.
 * PARIS_HIP_ERROR_INVALID_ARGUMENT for NULL pointers, pointers that are not 4-byte aligned, a setting the check refuses, dim_x or
 * dim_y of 0, z_count == 0, z_first + z_count > src_dim_z, or a destination range that overlaps the source BUFFER. */
int paris_hip_volume_bilateral(paris_hip_ctx* ctx, const float* d_src, uint32_t dim_x, uint32_t dim_y, uint32_t src_dim_z, uint32_t z_first,
                               uint32_t z_count, const struct paris_hip_volume_bilateral* setting, float* d_dst);

/* Extension (no reference counterpart): single-distance phase retrieval after Paganin et al. (2002) -- at magnification a micro-focus
 * scan shows propagation fringes at material edges, which the ramp filter amplifies. For one material with a known delta / beta the
 * remedy is a low-pass on the TRANSMISSION image: the library's only pass that filters a frame in two dimensions (phase.hip,
 * phase_rule.cpp).
 * Setting paris_hip_phase_retrieval { float alpha_mm2; float t_min; uint32_t margin; }: alpha_mm2 finite and > 0, 0 < t_min <= 1,
 *   1 <= margin <= PARIS_HIP_PHASE_MARGIN_MAX.
 * Input: whole frames of line integrals p, dim_x x dim_y floats (both >= 1) with the pixel pitches l_x = l_px_row, l_y = l_px_col (finite,
 *   > 0). In place.
 * Rule, per frame:
 *   1. T = expf(-p). A pixel whose p or T is not finite enters as T = 1 and is LEFT AS STORED in the output.
 *   2. N_x is the smallest power of two >= max(8, dim_x + 2 margin), N_y likewise from dim_y. Either above PARIS_HIP_PHASE_SIZE_MAX:
 *      PARIS_HIP_ERROR_UNSUPPORTED.
 *   3. Extension by edge replication with a circular wrap: padded column x >= dim_x reads column dim_x - 1 while
 *      x - dim_x < (N_x - dim_x + 1) / 2 (integer division) and column 0 beyond; rows likewise, applied to the extended rows.
 *   4. T' = IFFT2(FFT2(T_ext) H), H(k_x, k_y) = 1 / (1 + a_x[k_x] + a_y[k_y]) -- in fp32 (1 + a_x) + a_y and one IEEE division --,
 *      a_x[k] = alpha f^2 with f = k / (N_x l_x) for k <= N_x / 2 and (k - N_x) / (N_x l_x) above, a_y from N_y and l_y. Both tables
 *      are made in double on the host, rounded once to float and uploaded. H is real and even in both axes.
 *   5. p' = -logf(fmaxf(T', t_min)) on the first dim_x x dim_y samples; T' carries the division by N_x N_y, an exact scaling.
 * The answer for a frame does not depend on which other frames share the call, bit for bit: realness is exploited WITHIN the frame
 * (rows 2r and 2r + 1 packed as a + ib, split into their Hermitian half-spectra of N_x / 2 + 1 columns, merged before the inverse
 * row pass). Only the dim_y distinct rows are transformed; the column pass reads the padded rows through the row map.
 * Scratch: frames_per_launch * dim_y * (N_x / 2 + 1) complex floats, frames_per_launch = max(1, min(16, 64 MiB / the bytes of one
 * frame's spectra)); with the twiddles of both lengths (N_x / 2 + N_y / 2 complex floats) and the two tables in front of it, it is a
 * ctx-owned setting that paris_hip_projection_reserve_bytes counts.
 * Order: after the ring correction (a ring offset is a per-pixel gain in transmission, removed before a low-pass smears it), before
 * the beam-hardening polynomial, which acts on the retrieved line integral.
 * Limits: powers of two only; no band-wise form (a 2-D filter has no row band); one material, one distance. */
#define PARIS_HIP_PHASE_MARGIN_MAX 1024
#define PARIS_HIP_PHASE_SIZE_MAX 8192
typedef struct paris_hip_phase_retrieval {
    float alpha_mm2; /* pi lambda (delta / beta) z_eff at the detector plane [mm^2]; finite, > 0 */
    float t_min;     /* floor of the retrieved transmission; in (0, 1] */
    uint32_t margin; /* padding per side [px]: 1 .. PARIS_HIP_PHASE_MARGIN_MAX */
} paris_hip_phase_retrieval;
/* Host only, no ctx and no device: alpha = pi lambda (delta / beta) d_od (d_so + d_od) / d_so with lambda = 1.2398419843e-6 mm keV /
 * energy_kev, in double from |d_so| and |d_od| (as d_sd is formed), rounded once. (The effective defocus is d_od / M, and the
 * detector-plane frequencies are M times smaller than the object's: together the factor M.) PARIS_HIP_ERROR_INVALID_ARGUMENT for a
 * NULL pointer, a delta_over_beta or energy that is not finite and > 0, a d_so or d_od of 0 or not finite, or an alpha that does not
 * round to a finite float > 0. */
int paris_hip_phase_alpha(const paris_detector_geometry* det_geo, double delta_over_beta, double energy_kev, float* alpha_mm2);
/* Host only: max(8, ceil(6 sqrt(alpha) / (2 pi min(l_x, l_y)))), capped at PARIS_HIP_PHASE_MARGIN_MAX -- six decay lengths
 * sqrt(alpha) / 2 pi of the filter's kernel, in pixels. 0 for arguments that are not finite and > 0. */
uint32_t paris_hip_phase_default_margin(float alpha_mm2, float l_x, float l_y);
/* Host only: validates the setting for dim_x x dim_y frames of these pitches and returns the padded sizes and the bytes of scratch
 * the device needs (each pointer may be NULL). PARIS_HIP_ERROR_INVALID_ARGUMENT for a NULL setting, a field out of range, a zero
 * dimension or a pitch that is not finite and > 0; PARIS_HIP_ERROR_UNSUPPORTED for a padded size above PARIS_HIP_PHASE_SIZE_MAX
 * (n_x and n_y are still returned). */
int paris_hip_phase_retrieval_check(const paris_hip_phase_retrieval* setting, uint32_t dim_x, uint32_t dim_y, float l_x, float l_y,
                                    uint32_t* n_x, uint32_t* n_y, size_t* scratch_bytes);
/* Host only: the rule in DOUBLE on one dense frame, src to dst (which may be the same array), rounded to float at the store -- exp, a
 * double radix-2 transform of its own, log; the special pixels are judged as the rule says, on the fp32 expf. The C statement of the
 * model, not a mirror of the device's bits: the device agrees with it within FFT rounding. Refusals as the check, or
 * PARIS_HIP_ERROR_INVALID_ARGUMENT for a NULL src or dst. */
int paris_hip_phase_retrieval_host(const paris_hip_phase_retrieval* setting, float l_x, float l_y, const float* src, float* dst,
                                   uint32_t dim_x, uint32_t dim_y);
/* paris_hip_set_phase_retrieval runs the check and installs twiddles, tables and scratch for dim_x x dim_y frames in memory the ctx
 * owns. It replaces an earlier setting safely: work already queued keeps the old one. Without a setting nothing else changes. */
int paris_hip_set_phase_retrieval(paris_hip_ctx* ctx, const paris_hip_phase_retrieval* setting, uint32_t dim_x, uint32_t dim_y, float l_x,
                                  float l_y);
int paris_hip_clear_phase_retrieval(paris_hip_ctx* ctx);
/* In place on whole float frames, asynchronous: n_frames frames frame_stride bytes apart, d_p the first frame's row 0, rows pitch
 * bytes apart. Every row is the pass's band: a pending by-reference group and a held-back weighting run first. Calls of more than
 * frames_per_launch frames loop. PARIS_HIP_ERROR_INVALID_ARGUMENT without a setting, when dim_x / dim_y differ from the setting's, or
 * for a pitch or stride paris_hip_flat_field_rows would refuse. */
int paris_hip_phase_retrieval_frames(paris_hip_ctx* ctx, float* d_p, size_t pitch, size_t frame_stride, uint32_t n_frames, uint32_t dim_x,
                                     uint32_t dim_y);

/* Extension (no reference counterpart): correction of object scatter by kernel superposition after Ohnesorge et al. (1999) and
 * Sun & Star-Lack (2010), in its stationary form -- scatter is a smooth additive intensity on the detector, which shows as cupping and
 * as streaks between dense parts and is no function of a pixel's own line integral. A fixed-point iteration solves
 * T_m = T + (q(T) (*) g) for the primary transmission T: the second client of the library's 2-D transform (scatter.hip,
 * scatter_rule.cpp, frame_fft2.h).
 * Setting paris_hip_scatter_correction: amplitude A finite and > 0, alpha in [-2, 2], beta in [0, 4], sigma1_mm and sigma2_mm finite
 *   and > 0, weight2 finite and >= 0, limit in (0, 1), iterations in 1 .. PARIS_HIP_SCATTER_ITERATIONS_MAX, margin in
 *   1 .. PARIS_HIP_PHASE_MARGIN_MAX. The padded sizes N_x, N_y and PARIS_HIP_PHASE_SIZE_MAX are as for the phase filter.
 * Input: whole frames of line integrals p, dim_x x dim_y floats (both >= 1) with the pixel pitches l_x = l_px_row, l_y = l_px_col
 *   (finite, > 0). In place.
 * Rule, per frame:
 *   1. T_m = expf(-p). A pixel enters when p is finite and 0 < T_m < inf. Every other pixel enters as air -- T_m = 1, so a source of 0
 *      at first: it is iterated as a pixel with p = 0 is -- and is LEFT AS STORED in the output.
 *   2. T^0 = T_m. For k = 0 .. iterations - 1:
 *      source      lnT = logf(T^k), L = -lnT; q = A expf(alpha lnT + beta logf(L)) where L > 0, else q = 0 (that is A T^alpha L^beta).
 *      extension   q is extended to N_x x N_y exactly as step 3 of the phase filter: edge replication with the circular wrap.
 *      convolution S = IFFT2(FFT2(q_ext) G), G(k_x, k_y) = g1x[k_x] g1y[k_y] + g2x[k_x] g2y[k_y] in fp32 (two products, one sum);
 *                  g1y[k] = exp(-2 pi^2 sigma1^2 f^2), g1x[k] = that / (1 + w2), g2y[k] = exp(-2 pi^2 sigma2^2 f^2),
 *                  g2x[k] = w2 that / (1 + w2), f as in step 4 of the phase filter. All four tables are made in double on the host,
 *                  rounded once to float and uploaded. G(0, 0) = 1: A is the ratio of total scatter to total source. S carries the
 *                  division by N_x N_y, an exact scaling.
 *      update      T^(k+1) = fmaxf(T_m - S, (1 - limit) T_m), 1 - limit formed once in fp32. Both terms use the MEASURED T_m, never the
 *                  previous estimate: the iteration is T = T_m - S(T), and limit bounds the scatter fraction it may remove.
 *   3. p' = -logf(T^n) on the pixels that entered.
 * The answer for a frame does not depend on which other frames share the call, bit for bit. The estimate T^k never goes to memory: it
 * is a function of the unchanged frame p and of S, so one round of frames takes 2 iterations + 1 launches.
 * Scratch: as the phase filter's, with the same frames_per_launch; with the twiddles of both lengths and the four tables (2 N_x + 2 N_y
 * floats) in front of it, it is a ctx-owned setting that paris_hip_projection_reserve_bytes counts:
 * scratch_bytes + 12 (N_x + N_y) bytes.
 * Order: after the ring correction, before the phase retrieval and the beam-hardening polynomial -- scatter is additive on the measured
 * intensity and must be gone before a filter or a polynomial acts on what is taken for the primary.
 * Limits: one stationary, symmetric kernel; no down-sampled estimate; the parameters are given, not fitted. */
#define PARIS_HIP_SCATTER_ITERATIONS_MAX 16
typedef struct paris_hip_scatter_correction {
    float amplitude, alpha, beta; /* A, alpha, beta of the source q = A T^alpha (-ln T)^beta */
    float sigma1_mm, sigma2_mm;   /* widths of the two Gaussians at the detector plane [mm] */
    float weight2;                /* weight of the second Gaussian relative to the first; 0: one Gaussian */
    float limit;                  /* the largest scatter fraction S / T_m the correction removes; in (0, 1) */
    uint32_t iterations;          /* 1 .. PARIS_HIP_SCATTER_ITERATIONS_MAX */
    uint32_t margin;              /* padding per side [px]: 1 .. PARIS_HIP_PHASE_MARGIN_MAX */
} paris_hip_scatter_correction;
/* Host only: max(8, ceil(3 max(sigma1, sigma2) / min(l_x, l_y))), capped at PARIS_HIP_PHASE_MARGIN_MAX -- three widths of the wider
 * Gaussian, in pixels. 0 for arguments that are not finite and > 0. */
uint32_t paris_hip_scatter_default_margin(float sigma1_mm, float sigma2_mm, float l_x, float l_y);
/* Host only: validates the setting for dim_x x dim_y frames of these pitches and returns the padded sizes and the bytes of scratch
 * the device needs (each pointer may be NULL). Refusals as paris_hip_phase_retrieval_check: PARIS_HIP_ERROR_INVALID_ARGUMENT for a
 * NULL setting, a field out of range, a zero dimension or a pitch that is not finite and > 0; PARIS_HIP_ERROR_UNSUPPORTED for a
 * padded size above PARIS_HIP_PHASE_SIZE_MAX (n_x and n_y are still returned). */
int paris_hip_scatter_correction_check(const paris_hip_scatter_correction* setting, uint32_t dim_x, uint32_t dim_y, float l_x, float l_y,
                                       uint32_t* n_x, uint32_t* n_y, size_t* scratch_bytes);
/* Host only: the rule in DOUBLE on one dense frame, src to dst (which may be the same array), rounded to float at the store; the
 * special pixels are judged as the rule says, on the fp32 expf. The C statement of the model, not a mirror of the device's bits.
 * Refusals as the check, or PARIS_HIP_ERROR_INVALID_ARGUMENT for a NULL src or dst. */
int paris_hip_scatter_correction_host(const paris_hip_scatter_correction* setting, float l_x, float l_y, const float* src, float* dst,
                                      uint32_t dim_x, uint32_t dim_y);
/* paris_hip_set_scatter_correction runs the check and installs twiddles, tables and scratch for dim_x x dim_y frames in memory the ctx
 * owns. It replaces an earlier setting safely: work already queued keeps the old one. Without a setting nothing else changes. */
int paris_hip_set_scatter_correction(paris_hip_ctx* ctx, const paris_hip_scatter_correction* setting, uint32_t dim_x, uint32_t dim_y,
                                     float l_x, float l_y);
int paris_hip_clear_scatter_correction(paris_hip_ctx* ctx);
/* In place on whole float frames, asynchronous: the contract of paris_hip_phase_retrieval_frames -- every row is the pass's band, a
 * pending by-reference group and a held-back weighting run first, calls of more than frames_per_launch frames loop, and the
 * refusals are the same. */
int paris_hip_scatter_correction_frames(paris_hip_ctx* ctx, float* d_p, size_t pitch, size_t frame_stride, uint32_t n_frames, uint32_t dim_x,
                                        uint32_t dim_y);

/* Extension (no reference counterpart): suppression of photon-starvation streaks by adaptive filtering of the frames after Hsieh
 * (1998) and Kachelriess, Watzke & Kalender (2001). Along the longest or densest paths the detector counts a handful of photons; after
 * -ln the variance of the line integral grows like exp(p), and the ramp filter turns those pixels into streaks across the slice. The
 * pass smooths a frame only where the line integral is high, and the more the higher it is; every other pixel keeps its bits
 * (starvation.hip, starvation_rule.cpp).
 * Setting paris_hip_starvation_filter { float p0; float gain; uint32_t radius; }:
 *   p0      the line integral above which a pixel is filtered; finite.
 *   gain    finite and > 0; 1 gives full noise equalisation (below).
 *   radius  R, 1 <= R <= PARIS_HIP_STARVATION_RADIUS_MAX: the stencil is (2R + 1)^2 taps of the pixel's own frame.
 * Tables, made once on the host in double and rounded once to fp32 (paris_hip_starvation_filter_tables returns them): there are
 *   PARIS_HIP_STARVATION_LEVELS = 64 levels, each 1/16 wide in line integral; level k stands for the excess e_k = (k + 0.5) / 16 over p0.
 *   sigma_k = min(R / 2, gain sqrt(expm1(e_k) / (4 pi))) pixels -- a 2-D Gaussian of width sigma averages about 4 pi sigma^2 pixels, and
 *             exp(p - p0) pixels are what it takes to bring the variance at p down to the variance at p0.
 *   g[k][d] = exp(-d^2 / (2 sigma_k^2)) for d = 0 .. R, row k at g + k (R + 1); g[k][0] = 1.
 * Rule for pixel (x, y) of a frame with the stored value c; every operation is fp32, rounded once, never contracted:
 *   if !(c > p0) the pixel is NOT WRITTEN: its bits stay, NaN payloads and -0 included.
 *   t = (c - p0) * 16.f; k = t < 64.f ? (uint32_t)t : 63.
 *   num = den = 0. Taps are walked with dy ascending from -R and within it dx ascending from -R, the centre included. A tap outside the
 *   frame is skipped, and so is a tap whose value v is not finite. For every other tap w = g[k][|dy|] * g[k][|dx|],
 *   num = num + w * v, den = den + w.
 *   if den == 0 the pixel is not written (a +inf centre none of whose taps counts); else p = num / den, the IEEE division.
 * Every tap is the value AS STORED BEFORE THE CALL: the result is a pure function of the input frame and depends neither on the other
 * frames of the call, nor on how the launch is tiled, nor on any sweep order. The pass is not idempotent.
 * Counts (paris_hip_starvation_stats): frames examined, pixels filtered (c > p0 and den != 0: the pixels that received num / den) and
 * those of them at level 63, all exact integers equal to the host rule's. A high share at level 63 says that p0 is too low or the
 * radius too small for the scan.
 * Device: outputs go to a ctx-owned scratch of PARIS_HIP_STARVATION_FRAMES_MAX frames first and are stored into the frames by a second
 * kernel, so no window reads a filtered value; calls with more frames loop. Scratch, tables and counters are one ctx-owned setting
 *  that paris_hip_projection_reserve_bytes counts.
 * Order: on line integrals, after the ring correction and before the scatter correction.
 * Limits: 2-D only, no smoothing across views; the level comes from the noisy pixel itself; it works on the grid, not in mm. */
#define PARIS_HIP_STARVATION_RADIUS_MAX 4
#define PARIS_HIP_STARVATION_LEVELS 64
#define PARIS_HIP_STARVATION_FRAMES_MAX 8 /* frames one launch serves: 128 MiB of scratch for 2048 x 2048 frames */
typedef struct paris_hip_starvation_filter {
    float p0;        /* filter above this line integral; finite */
    float gain;      /* scales the width law; finite, > 0; 1: full noise equalisation */
    uint32_t radius; /* R: 1 .. PARIS_HIP_STARVATION_RADIUS_MAX */
} paris_hip_starvation_filter;
/* what paris_hip_starvation_stats reports */
typedef struct paris_hip_starvation_counts {
    uint64_t frames;     /* frames examined */
    uint64_t filtered;   /* pixels that received num / den */
    uint64_t last_level; /* those of them at level 63 */
} paris_hip_starvation_counts;
/* Host only: PARIS_HIP_ERROR_INVALID_ARGUMENT for a NULL setting, a p0 or gain that is not finite, gain <= 0, a radius outside
 * 1 .. PARIS_HIP_STARVATION_RADIUS_MAX or a zero dimension; PARIS_HIP_ERROR_UNSUPPORTED when dim_x * dim_y does not fit 32 bits.
 * *device_bytes (may be NULL): what the setting occupies on a device. */
int paris_hip_starvation_filter_check(const paris_hip_starvation_filter* setting, uint32_t dim_x, uint32_t dim_y, size_t* device_bytes);
/* Host only: sigma receives PARIS_HIP_STARVATION_LEVELS floats, g PARIS_HIP_STARVATION_LEVELS * (R + 1). Either may be NULL.
 * PARIS_HIP_ERROR_INVALID_ARGUMENT for a setting the check refuses. */
int paris_hip_starvation_filter_tables(const paris_hip_starvation_filter* setting, float* sigma, float* g);
/* Host only: the rule on one dense frame, src to dst (dim_x x dim_y floats each, not overlapping): dst receives src with the filtered
 * pixels replaced. counts (may be NULL) receives the frame's counts, frames = 1. The device gives these bits. Refusals as the check, or
 * PARIS_HIP_ERROR_INVALID_ARGUMENT for a NULL src or dst. */
int paris_hip_starvation_filter_host(const paris_hip_starvation_filter* setting, const float* src, float* dst, uint32_t dim_x, uint32_t dim_y,
                                     paris_hip_starvation_counts* counts);
/* paris_hip_set_starvation_filter runs the check and installs counters (zeroed), tables and scratch for dim_x x dim_y frames in memory
 * the ctx owns. It replaces an earlier setting safely: work already queued keeps the old one. */
int paris_hip_set_starvation_filter(paris_hip_ctx* ctx, const paris_hip_starvation_filter* setting, uint32_t dim_x, uint32_t dim_y);
int paris_hip_clear_starvation_filter(paris_hip_ctx* ctx);
/* In place on whole float frames, asynchronous on the ctx stream: every row is the pass's band, a pending by-reference group and a
 * held-back weighting run first, calls of more than PARIS_HIP_STARVATION_FRAMES_MAX frames loop. PARIS_HIP_ERROR_INVALID_ARGUMENT
 * without a setting, for other dimensions than the setting's, or for a pitch or stride paris_hip_flat_field_rows would refuse. */
int paris_hip_starvation_filter_frames(paris_hip_ctx* ctx, float* d_p, size_t pitch, size_t frame_stride, uint32_t n_frames, uint32_t dim_x,
                                       uint32_t dim_y);
/* The counts since the setting was made or last reset; synchronises the ctx stream. reset != 0 zeroes them behind the read. */
int paris_hip_starvation_stats(paris_hip_ctx* ctx, paris_hip_starvation_counts* out, int reset);

/* ---- diagnostics ---------------------------------------------------------------------------------- */
const char* paris_hip_strerror(int status);
/* library version "major.minor.patch" */
const char* paris_hip_version(void);
/* 1: this library is the experiments build (make -C paris_amd/csrc EXPERIMENTS=1 -> libparis_hip_experiments.so): the kernels,
 * tile orders and A/B switches that were measured and lost are compiled in. 0: the product build -- its setters answer
 * PARIS_HIP_ERROR_UNSUPPORTED for them (backprojection variants 3 and 5, unroll 3 and 4, the slice shapes, tile orders 0 / 1 / 8 /
 * 9 / 12, filter variant 2). Results never depend on any of them. */
int paris_hip_has_experiments(void);
/* Times the most recent backproject launch on this ctx (HIP events recorded on the ctx stream around the
 * kernel); synchronises the stream. Used by bench.py for roofline.achieved. */
int paris_hip_last_backproject_ms(paris_hip_ctx* ctx, float* ms);
/* Arms a ring of `capacity` HIP event pairs: every following backproject launch on this ctx is bracketed by
 * events on the ctx stream. _collect synchronises the stream and returns the durations (ms) of the launches
 * still in the ring, oldest first. Default capacity is 1 (paris_hip_last_backproject_ms). Capacity 0 switches the events
 * off (nothing but kernels and copies is enqueued: what a caller capturing the ctx stream into a hipGraph wants). */
int paris_hip_backproject_timing_arm(paris_hip_ctx* ctx, uint32_t capacity);
int paris_hip_backproject_timing_collect(paris_hip_ctx* ctx, float* ms, uint32_t max_n, uint32_t* n_out);
/* Selects the backprojection kernel: 0 = default (currently the tile kernel), 1 = one-thread-per-voxel gather kernel
 * without LDS (slow, for cross-checking), 2 = tile kernel (z-walk per workgroup), 3 = slice kernel (one slice per
 * wave; needs a 16-byte aligned volume with dim_x % 4 == 0, else falls back to 2), 4 = the fused kernel run with one
 * projection (every slice of a tile in flight before the first store; measured 5 % slower than the tile kernel). All give
 * identical bits. 3 and 5 (the two-pass variant: column constants of the whole plane precomputed per projection) were measured
 * slower and exist in the experiments build only (PARIS_HIP_ERROR_UNSUPPORTED in the product).
 * paris_hip_backproject_batch uses its fused kernel under variant 0 and runs one launch per projection otherwise. */
int paris_hip_set_backproject_variant(paris_hip_ctx* ctx, int variant);
/* Tuning knobs of the LDS-staged kernel; 0 keeps the default. vx: voxels per lane along x (1, 2, 4; capped by
 * the volume's alignment), unroll: z slices in flight per lane (1, 2, 4; 3 = one at a time with the next one prefetched), tz: slices per tile, lds_bytes: LDS
 * budget per workgroup for the staged detector box (1024..65536). Results do not depend on any of them. The launcher picks unroll 1 or 2
 * by itself; 3 and 4 are compiled into the experiments build only (PARIS_HIP_ERROR_UNSUPPORTED in the product). */
int paris_hip_set_backproject_tuning(paris_hip_ctx* ctx, int vx, int unroll, int tz, int lds_bytes);
/* Shape of the slice kernel: waves (= slices per tile) x row groups per lane; (16,4) (16,2) (8,4) (8,2) (8,1),
 * (0,0) = default. Experiments build only (the product has no slice kernel: PARIS_HIP_ERROR_UNSUPPORTED for anything but (0,0)). */
int paris_hip_set_backproject_slice_shape(paris_hip_ctx* ctx, int waves, int row_groups);
/* Workgroup -> tile order (-1 default by volume shape: 15 for planes beyond 1024^2, else 18, or 5 when the z tiles do not divide among the 8 XCDs; 0 x-fastest, 1 z-fastest, 5 one
 * contiguous run of tiles per XCD, 8 one band of y tiles per XCD swept x -> z -> y, 9 the same swept x -> y -> z, 12 order 8 in chunks
 * of 256 slices, 14 / 15 / 16 / 17 y tiles DEALT to the XCDs singly / in pairs / in fours / in eights, in shallow z chunks, 18 z tiles
 * dealt to the XCDs) and the cache
 * policy of the volume stream (2 nontemporal loads with write-through nontemporal stores, 1 nontemporal, 0 plain, -1 library
 * default: plain for slabs that largely stay in the Infinity Cache between launches, up to 384 MiB, 2 for larger ones).
 * Performance only. The product build has the orders the launcher picks from, 5 and 14 .. 18; 0 / 1 / 8 / 9 / 12 lost and are
 * compiled into the experiments build only (PARIS_HIP_ERROR_UNSUPPORTED). */
int paris_hip_set_backproject_order(paris_hip_ctx* ctx, int order, int nontemporal);
/* The per-voxel division by the detector pixel pitch may run as multiply + 2 FMA instead of the IEEE sequence,
 * but only for a divisor for which an exhaustive GPU check over all 2^32 fp32 dividends (once per ctx and divisor)
 * found the detector coordinate v = x / pitch - 0.5 identical (bit for bit, or out of any detector's range both ways).
 * enable = 0 forces the IEEE sequence. Results never depend on this. */
int paris_hip_set_backproject_fast_division(paris_hip_ctx* ctx, int enable);
/* Staging of the detector box into LDS 4 pixels per lane (default on; used when the projection base and pitch are
 * 16-byte aligned, 8-byte for half pixels). enable = 0 forces one pixel per lane. Results never depend on this. */
int paris_hip_set_backproject_vector_staging(paris_hip_ctx* ctx, int enable);
/* Runs (or looks up) the exhaustive check for one divisor: *exact = 1 when multiply + 2 FMA reproduces
 * x / divisor - 0.5 for every fp32 x (see above). */
int paris_hip_fast_division_is_exact(paris_hip_ctx* ctx, float divisor, int* exact);
/* Two more hand-expanded IEEE sequences, each used only after the device has compared it with the compiler's correctly rounded
 * operation for EVERY fp32 operand a launch can produce (once per process, device and operand range; microseconds):
 *  - the two per-column divisions d_sd / (s + d_so), d_so / (s + d_so) of the backprojection (src/openmp/backprojection.cpp:125,139)
 *    share one refined reciprocal; checked for every denominator in [0.09, 1.92] x d_so, the range the library first proves the
 *    launch stays in (otherwise, or on any mismatch, both are plain IEEE divisions). *exact = 1: both quotients have the IEEE bits.
 *  - the weighting's d_sd / sqrt(q) (src/openmp/weighting.cpp:52) inside the one-launch weight + filter; checked for every radicand
 *    q in [q_lo, q_hi] (the library asks for [d_sd^2, largest radicand of the rows], widened a little).
 * paris_hip_set_lean_validation(ctx, 0) makes the kernels trust the range tests alone (rounds 2-3 behaviour; for A/B and for testing
 * the validators). Results never depend on any of this. */
int paris_hip_lean_division_is_exact(paris_hip_ctx* ctx, float d_sd, float d_so, int* exact);
int paris_hip_lean_weighting_is_exact(paris_hip_ctx* ctx, float d_sd, float q_lo, float q_hi, int* exact);
int paris_hip_set_lean_validation(paris_hip_ctx* ctx, int enable);

#ifdef __cplusplus
}
#endif
#endif /* PARIS_HIP_H_ */
