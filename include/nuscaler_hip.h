/*
 * nuscaler_hip.h -- C ABI of the MI355X (gfx950) upscale + frame-interpolation path.
 *
 * This is the drop-in boundary for nu_scaler_core's per-pixel hot path: a Rust shim
 * (`impl Upscaler for HipUpscaler`) or the ctypes module
 * nu_scaler_amd binds exactly these entry points.  Plain pointers and sizes only.
 *
 * Reference interfaces replaced (paths relative to the reference checkout):
 *   trait Upscaler                      nu_scaler_core/src/upscale/mod.rs:67-88
 *   UpscalerFactory::create_upscaler    nu_scaler_core/src/upscale/mod.rs:95-117
 *   WgpuUpscaler::upscale / _batch      nu_scaler_core/src/upscale/mod.rs:935-1058, :609-640
 *   WgpuFrameInterpolator::interpolate_py   nu_scaler_core/src/wgpu_interpolator.rs:215-491
 *   get_last_gpu_duration_ms            nu_scaler_core/src/wgpu_interpolator.rs:494-497
 *   trait FrameInterpolator (shape)     nu_scaler_core/src/interpolation/mod.rs:29-44
 *   ErrorMetrics::calculate             Nu_scale/src/upscale/common.rs:475-543
 *   BlockMatchingInterpolator           nu_scaler_core/src/interpolation/mod.rs:513-911
 *
 * Frames are tightly packed RGBA8, row-major.  Every function returns NUS_OK (0)
 * or a negative nus_status; the message is available from nus_*_last_error(handle)
 * (per handle) and nus_last_error() (thread-local, also covers create failures).
 * Concurrent calls on one handle are serialised by a per-handle mutex (the reference
 * calls upscale(&self) from rayon threads, upscale/mod.rs:619-624).
 * There is no CPU fallback: without a usable HIP device the compute entry points
 * fail with NUS_ERR_NO_DEVICE.
 * Host entry points that take pageable buffers copy through pinned staging memory; copies of
 * 1 MiB and more are split over a few process-wide helper threads started on first use (up to 6, fewer where the process's
 * CPU mask or cgroup quota is smaller; environment: NUS_COPY_THREADS=n, 0 = copy on the calling thread only).  The same
 * threads make the pages of a pageable OUTPUT buffer present while its frame is on the GPU (a result buffer fresh from the
 * allocator -- the Vec / PyBytes of the trait's `upscale` -- otherwise takes its first-touch faults inside the copy-out);
 * buffer contents are never touched before the frame's bytes arrive.  A fresh buffer that is its own mapping also gets a transparent-huge-page
 * hint (environment NUS_NO_THP_HINT=1 turns that off).
 */
#ifndef NUSCALER_HIP_H
#define NUSCALER_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NUS_ABI_VERSION 1

typedef enum nus_status {
    NUS_OK = 0,
    NUS_ERR_INVALID_ARGUMENT = -1,
    NUS_ERR_NOT_INITIALIZED = -2, /* "Upscaler not initialized. Call initialize() first." (mod.rs:937-939) */
    NUS_ERR_SIZE_MISMATCH = -3,   /* "Input data size (..) does not match expected input buffer size (..)" (mod.rs:960-966) */
    NUS_ERR_HIP = -4,
    NUS_ERR_NO_DEVICE = -5,
    NUS_ERR_UNSUPPORTED = -6,
    NUS_ERR_OUT_OF_MEMORY = -7
} nus_status;

/* UpscaleAlgorithm (mod.rs:50-53) plus the build-defined Lanczos-3 value. */
typedef enum nus_algorithm {
    NUS_ALG_NEAREST = 0,
    NUS_ALG_BILINEAR = 1,
    NUS_ALG_LANCZOS3 = 2,
    /* "next" row: the other image-0.24.9 filters the legacy
     * BasicUpscaler delegates to (Nu_scale/src/upscale/common.rs:233-260) */
    NUS_ALG_BICUBIC = 3,  /* FilterType::CatmullRom (UpscalingAlgorithm::Bicubic) */
    NUS_ALG_TRIANGLE = 4, /* FilterType::Triangle (what Lanczos2 / Mitchell map to there) */
    /* same row: the FSR1-style shader pair the reference keeps but never dispatches
     * (nu_scaler_core/src/upscale/fsr.rs:24-169 EASU, :173-260 RCAS).  PARITY UNPINNED. */
    NUS_ALG_FSR1 = 5,     /* EASU then RCAS, fused (the EASU image stays in LDS) */
    NUS_ALG_FSR_EASU = 6, /* EASU alone */
    NUS_ALG_FSR_RCAS = 7  /* RCAS alone: output size must equal input size */
} nus_algorithm;

/* UpscalingQuality (mod.rs:37-46), same order.  Quality never changes the arithmetic
 * (mod.rs:1072-1077). */
typedef enum nus_quality {
    NUS_QUALITY_ULTRA_PERFORMANCE = 0,
    NUS_QUALITY_ULTRA = 1,
    NUS_QUALITY_QUALITY = 2,
    NUS_QUALITY_BALANCED = 3,
    NUS_QUALITY_PERFORMANCE = 4,
    NUS_QUALITY_NATIVE = 5
} nus_quality;

/* UpscalingTechnology (mod.rs:56-64), same order. */
typedef enum nus_technology {
    NUS_TECH_NONE = 0,
    NUS_TECH_FSR = 1,
    NUS_TECH_DLSS = 2,
    NUS_TECH_WGPU = 3,
    NUS_TECH_FALLBACK = 4
} nus_technology;

/* WorkgroupSizePreset (wgpu_interpolator.rs:98-127).  Accepted for API parity; the
 * HIP kernels pick their own wave64 launch shape. */
typedef enum nus_wg_preset {
    NUS_WG_SQUARE_8X8 = 0,
    NUS_WG_SQUARE_16X16 = 1,
    NUS_WG_WIDE_32X8 = 2,
    NUS_WG_TALL_8X32 = 3
} nus_wg_preset;

/* Bilinear arithmetic variant.  CPU form is the oracle; the WGSL form
 * is offered for callers that need byte-equality with the wgpu shader instead. */
typedef enum nus_bilinear_variant {
    NUS_BILINEAR_CPU = 0, /* Nu_scale/src/upscale/common.rs:199-231 */
    NUS_BILINEAR_WGSL = 1 /* nu_scaler_core/src/upscale/mod.rs:209-263 */
} nus_bilinear_variant;

/* Lanczos accumulate mode. FMA: fused multiply-add (within +-1 LSB of the oracle);
 * EXACT: separate multiply and add, same rounding sequence as the CPU restatement. */
typedef enum nus_lanczos_mode {
    NUS_LANCZOS_FMA = 0,
    NUS_LANCZOS_EXACT = 1
} nus_lanczos_mode;

typedef struct nus_upscaler nus_upscaler;
typedef struct nus_interp nus_interp;

/* ---- library ------------------------------------------------------------------ */

int nus_abi_version(void);
/* Number of usable HIP devices (0 when none; never fails). */
int nus_device_count(void);
/* HBM of one device in bytes (hipMemGetInfo): what PyAdvancedWgpuUpscaler.get_vram_stats reports
 * (nu_scaler_core/src/lib.rs:539-584, gpu/memory.rs:731-764).  NUS_ERR_NO_DEVICE without a device. */
int nus_device_memory_info(int device, uint64_t *free_bytes, uint64_t *total_bytes);
/* Host buffers the caller re-uses (a frame pool, the Vec a Rust caller keeps between calls) can be pinned once: the host entry
 * points (nus_upscaler_upscale, _upscale_batch, nus_interp_interpolate) then DMA straight from / into them and skip the copy
 * through the library's pinned staging -- upscale_batch: 0.65 instead of 0.85 ms per 1080p -> 4K frame, 0.92 of the box's D2H
 * ceiling.  hipHostRegister / hipHostUnregister underneath (page-aligned pieces of the process's address space; the buffer
 * must not be freed or re-allocated while pinned).  Buffers that are not pinned work as before.  The library never pins a
 * caller's buffer by itself: it cannot know when the memory is given back. */
int nus_host_pin(void *buffer, size_t bytes);
/* Only a pointer nus_host_pin accepted and that has not been unpinned since (anything else: NUS_ERR_INVALID_ARGUMENT, the runtime
 * is not asked).  A failing hipHostUnregister is NUS_ERR_HIP and the range stays in the library's record (nus_host_ranges): the
 * registration may still exist, and a registration that outlives its buffer is exactly what must not go unnoticed. */
int nus_host_unpin(void *buffer);
/* The road between HBM and a caller's host buffer for users of the *_device entry points -- what the reference's upscale() does at
 * its end (map the staging buffer, wait, to_vec: nu_scaler_core/src/upscale/mod.rs:1041-1057) and before its dispatch
 * (queue.write_buffer, :968-1008).  The host pointer may be pageable: it is NEVER handed to the HIP runtime (whose pageable copies
 * pin the caller's pages on the fly and cache that registration by address -- a freed and re-used heap block then meets a stale
 * one; docs/d2h_fault_analysis.md).  The bytes travel through a ring of pinned chunks the library allocates on first use
 * (4 x 8 MiB per device, kept for the life of the process) and are moved between ring and buffer by the copy threads of the host
 * path while the next chunk is on the wire.  A pinned host buffer (hipHostMalloc, nus_host_pin) is copied to / from directly.
 *   nus_download: ordered after the work already enqueued on `stream`; returns when host_dst holds the bytes.
 *   nus_upload:   returns when host_src may be re-used; the device bytes are in place for work enqueued on `stream` afterwards.
 * `stream`: a hipStream_t of the device that owns the device pointer (NULL: its null stream).  Concurrent transfers on one device
 * take turns.  NUS_ERR_INVALID_ARGUMENT for null pointers or a device pointer the runtime does not know as device memory. */
int nus_download(void *host_dst, const void *d_src, size_t bytes, void *stream);
int nus_upload(void *d_dst, const void *host_src, size_t bytes, void *stream);
/* Diagnostics (not in the reference).  The host ranges the library has registered with the runtime (nus_host_pin), allocated as
 * pinned memory itself (slots, staging, the transfer ring) or left a transparent-huge-page hint on (fresh result buffers of the
 * host path).  history = 0: the live entries; 1: the last <= 128 events, oldest first (op 1 = added, 0 = removed).
 * Returns the number of records written (<= cap). */
typedef struct nus_host_range {
    uint64_t seq;  /* order of the event, process-wide, from 1 */
    uintptr_t lo;  /* first byte */
    uintptr_t hi;  /* one past the last byte */
    uint32_t kind; /* 1 pinned by the caller (nus_host_pin), 2 hipHostMalloc by the library, 3 MADV_HUGEPAGE hint */
    uint32_t op;
} nus_host_range;
size_t nus_host_ranges(nus_host_range *out, size_t cap, int history);
/* On SIGABRT / SIGSEGV / SIGBUS / SIGILL / SIGFPE write, to a duplicate of descriptor `fd` and with async-signal-safe calls only:
 * the native backtrace of the raising thread (which library called abort()), the ranges above, and /proc/self/maps -- then hand
 * over to the handler that was installed before (or the default action).  Off unless called; idempotent.  A GPU page fault
 * reaches a process as ROCr's abort() with an address in its message: this is what lets that address be placed afterwards. */
int nus_install_fatal_trace(int fd);
/* Calibration of the box a measurement runs on (not in the reference; bench.py's denominators next to the 8 TB/s spec figure --
 * SURVEY.md section 8(d) "on-box copy ceiling" -- never on the product path).  Enqueues ONE plain kernel (or the runtime's
 * copy) on `stream`; the caller brackets it with events.  kind: 0 hipMemcpyDtoDAsync of `bytes`; 1 stream copy, 16 B per lane,
 * read one write one; 2 write-only stream of `bytes` into d_dst; 3 read-only stream of `bytes` from d_src (d_dst: >= 4 bytes of
 * device memory); 4 one read : four writes -- `bytes` read from d_src, 4 * `bytes` written to d_dst, each store instruction one
 * contiguous KiB per wave (the byte mix of a x2 upscale with no arithmetic); 5 VGPR-only f32 FMA chains, nothing touches
 * memory: 2048 blocks x 256 lanes x 16 chains x `iters` FMAs (d_dst: >= 2 MiB, never written).  Pointers 16-byte aligned,
 * `bytes` a multiple of 16 (kind 4: of 1024 -- whole waves, each of which writes four contiguous KiB; anything else is refused). */
int nus_probe_device(int kind, const void *d_src, void *d_dst, size_t bytes, uint32_t iters, void *stream);
/* Pieces (copies and page-populate requests) of the host path's helper-thread pool that are still queued or running, process-wide
 * (not in the reference; diagnostics).  0 whenever no host call is in progress: every entry point waits for what it queued
 * before it returns, on its error paths too -- the pieces point into the caller's buffers. */
size_t nus_host_pending_pieces(void);
/* Thread-local message of the last failing call on this thread ("" if none). */
const char *nus_last_error(void);
const char *nus_status_string(int status);

/* ---- Upscaler (trait Upscaler, mod.rs:67-88) ----------------------------------- */

/* WgpuUpscaler::new(quality, algorithm).  Never touches the GPU. NULL on bad enum. */
nus_upscaler *nus_upscaler_create(int algorithm, int quality);
/* UpscalerFactory::create_upscaler(technology, quality) (mod.rs:95-117):
 * Wgpu -> bilinear; FSR / DLSS / None / Fallback -> nearest. */
nus_upscaler *nus_upscaler_create_for_technology(int technology, int quality);
void nus_upscaler_destroy(nus_upscaler *h);

/* Select the HIP device (default 0).  Must precede initialize. */
int nus_upscaler_set_device(nus_upscaler *h, int device);
int nus_upscaler_set_bilinear_variant(nus_upscaler *h, int variant);
int nus_upscaler_set_lanczos_mode(nus_upscaler *h, int mode);
/* Tuning / test knobs: "force_general" (0/1, before initialize: never pick an x2
 * fast path), "force_per_pixel" (0/1, before initialize: resize without the LDS row kernel),
 * "force_rows" (0/1, before initialize: resize without the register-window variant of it),
 * "rows_per_wave" (fixed-factor resize kernels: input rows per wave, 0 = auto), "unit_order" (below),
 * "down_seg_width" (0..64, before initialize: output columns per wave of the down-scaling kernel, 0 = auto),
 * "pq_narrow" (1 default / 0: see nus_upscaler_get_option),
 * host path: "single_bands" (1 = nus_upscaler_upscale sends one frame through the pipeline in row bands where the
 * kernel allows it, default; 0 = whole), "single_out_plan" (0..3) / "batch_out_chunks" (1..8): how a pageable
 * output frame is cut into device-to-host pieces when it is alone in the pipeline / has others behind it. */
int nus_upscaler_set_option(nus_upscaler *h, const char *key, int64_t value);
/* What the library decided (diagnostics; not in the reference): "pq_p" / "pq_q" (the factor P / Q of the small-rational-factor
 * resize kernel, 0 when another kernel runs), "pq_narrow_active" (1: that kernel sums the 4 non-zero taps of a support-2 filter,
 * option "pq_narrow" 0 turns it off: same bytes either way), "rows_per_wave", "win_outputs_per_lane" (4 or 2: output columns per
 * lane of the register-window any-scale resize kernel, 0 when another kernel runs).  Unknown key: NUS_ERR_INVALID_ARGUMENT. */
int nus_upscaler_get_option(nus_upscaler *h, const char *key, int64_t *value);
/* Channel order of the input frames.  Captured frames arrive as BGRA and the reference swizzles them
 * on the CPU before upscaling (nu_scaler_core/src/lib.rs:251-270); with NUS_FORMAT_BGRA8 the kernels
 * do it inside their loads (one v_perm_b32 per loaded pixel, no extra pass).  Output is always RGBA8.
 * May be called at any time. */
typedef enum nus_pixel_format {
    NUS_FORMAT_RGBA8 = 0,
    NUS_FORMAT_BGRA8 = 1,
    /* alpha byte undefined (BGRX / XRGB capture surfaces): read as 255, so the output alpha is 255 */
    NUS_FORMAT_RGBX8 = 2,
    NUS_FORMAT_BGRX8 = 3
} nus_pixel_format;
int nus_upscaler_set_input_format(nus_upscaler *h, int format);
/* FSR1-style passes: the `sharpness` uniform of each shader (fsr.rs:35, :178), <= 1.  A negative
 * value keeps the default: EASU 0 (build-defined; the reference never assigns it), RCAS by quality
 * as the reference's CPU FSR path does -- Ultra 0.8, Quality 0.7, Balanced 0.6, else 0.5
 * (Nu_scale/src/upscale/fsr3.rs:231-236).  May be called at any time. */
int nus_upscaler_set_sharpness(nus_upscaler *h, float easu, float rcas);
int nus_upscaler_get_sharpness(const nus_upscaler *h, float *easu, float *rcas);

/* Upscaler::initialize (mod.rs:875-933).  Builds the per-axis tables on the host,
 * allocates device + pinned staging buffers.  Re-initialising with new dimensions
 * is allowed. */
int nus_upscaler_initialize(nus_upscaler *h, uint32_t in_w, uint32_t in_h,
                            uint32_t out_w, uint32_t out_h);

/* Upscaler::upscale (mod.rs:935-1058): host frame in, host frame out.
 * in_len must equal in_w*in_h*4; out_cap must be >= out_w*out_h*4. */
int nus_upscaler_upscale(nus_upscaler *h, const uint8_t *in, size_t in_len,
                         uint8_t *out, size_t out_cap);
/* WgpuUpscaler::upscale_batch (mod.rs:609-640): n host frames, pipelined over
 * H2D / kernel / D2H streams instead of a rayon map. */
int nus_upscaler_upscale_batch(nus_upscaler *h, const uint8_t *const *ins,
                               const size_t *in_lens, size_t n,
                               uint8_t *const *outs, size_t out_cap_each);

/* A persistent ring over the same three pipeline slots, for callers that get their frames one at a time (a capture loop: the
 * legacy app's FrameBuffer feeding upscale(), Nu_scale/src/capture/frame_buffer.rs:11-50, Nu_scale/src/lib.rs:107-190):
 *   stream_open    starts the ring (NUS_ERR_NOT_INITIALIZED before initialize; one stream per upscaler);
 *   stream_submit  stages and enqueues one frame and returns -- it blocks only while 3 frames are in flight -- with a
 *                  ticket (0, 1, 2 ...); `out` must stay valid until that ticket has been waited for (or the stream closed);
 *   stream_wait    returns when the frame with that ticket is in its `out` buffer (frames complete in submission order; may
 *                  be called from another thread than stream_submit);
 *   stream_close   waits for everything in flight and stops the ring (also done by initialize and destroy).
 * While a stream is open, nus_upscaler_upscale / _upscale_batch on the same handle fail (the slots are in use).  H2D of frame
 * i+1, the kernel of frame i and the D2H / copy-out of frame i-1 overlap exactly as inside nus_upscaler_upscale_batch. */
int nus_upscaler_stream_open(nus_upscaler *h);
int nus_upscaler_stream_submit(nus_upscaler *h, const uint8_t *in, size_t in_len, uint8_t *out, size_t out_cap,
                               uint64_t *ticket);
int nus_upscaler_stream_wait(nus_upscaler *h, uint64_t ticket);
int nus_upscaler_stream_close(nus_upscaler *h);

/* Device-resident path: d_in holds n_frames contiguous input frames already in HBM,
 * d_out receives n_frames contiguous output frames.  Enqueued on `stream`
 * (a hipStream_t, NULL = default stream); does not synchronise. */
int nus_upscaler_upscale_device(nus_upscaler *h, const void *d_in, void *d_out,
                                uint32_t n_frames, void *stream);

/* Fused "interpolate with zero flow, then upscale the in-between frame" -- the GUI's own sequence
 * (nu_scaler_py/nu_scaler/main.py:999-1008) -- without materialising the 1080p in-between frame:
 * unit i blends frames d_a + i*a_stride and d_b + i*b_stride at t (per channel
 * trunc((1-t) a + t b), the pixel nus_interp_interpolate would have produced) inside the resize
 * kernel's row loads.  Available for the exact-x2 resize kernels (Lanczos-3 / bicubic / triangle);
 * otherwise NUS_ERR_UNSUPPORTED and the caller runs the two stages separately.  Results equal
 * nus_interp_interpolate_device followed by nus_upscaler_upscale_device bit for bit. */
int nus_upscaler_upscale_blend_device(nus_upscaler *h, const void *d_a, size_t a_stride, const void *d_b,
                                      size_t b_stride, float t, void *d_out, uint32_t n_frames, void *stream);

/* The whole step of the GUI's frame loop for a batch of pairs in ONE launch (nu_scaler_py/nu_scaler/main.py:999-1008 interpolates
 * and then upscales; the BASELINE metric upscales the real frame too): for unit i, with A_i = d_a + i*a_stride and
 * B_i = d_b + i*b_stride (stride 0 = tightly packed frames),
 *   d_out_real[i] = upscale(A_i)                       what nus_upscaler_upscale_device writes,
 *   d_mid[i]      = blend(A_i, B_i) at t, zero flow    what nus_interp_interpolate_device writes (d_mid may be NULL),
 *   d_out_mid[i]  = upscale(blend(A_i, B_i))           what nus_upscaler_upscale_blend_device writes,
 * bit for bit.  Every (frame, row block, strip) is walked by two waves of the same kernel side by side -- one on A_i alone, one
 * blending A_i and B_i on load -- so each input row reaches HBM's bus about once per step instead of four times and the
 * in-between frame is written, never re-read.  Exact-x2 resize kernels (Lanczos-3 / bicubic / triangle) only; otherwise
 * NUS_ERR_UNSUPPORTED and the caller runs the three stages separately.  Enqueue only, no allocation.
 * Option "unit_order" (nus_upscaler_set_option): 1 = row-block-major wave order (default), 0 = frame-major. */
int nus_upscaler_upscale_unit_device(nus_upscaler *h, const void *d_a, size_t a_stride, const void *d_b, size_t b_stride,
                                     float t, void *d_mid, void *d_out_real, void *d_out_mid, uint32_t n_units,
                                     void *stream);

const char *nus_upscaler_name(const nus_upscaler *h); /* "WgpuNearestUpscaler" / "WgpuBilinearUpscaler" (mod.rs:1060-1066) / "Hip{Lanczos3,Bicubic,Triangle}Upscaler" */
int nus_upscaler_algorithm(const nus_upscaler *h);
int nus_upscaler_quality(const nus_upscaler *h);
int nus_upscaler_set_quality(nus_upscaler *h, int quality);
int nus_upscaler_is_initialized(const nus_upscaler *h);
size_t nus_upscaler_input_size(const nus_upscaler *h);  /* in_w*in_h*4, 0 before initialize */
size_t nus_upscaler_output_size(const nus_upscaler *h); /* out_w*out_h*4 */
const char *nus_upscaler_last_error(const nus_upscaler *h);
/* Kernel time (hipEvent pair) of the last host-path upscale; NUS_ERR_NOT_INITIALIZED if none. */
int nus_upscaler_last_gpu_ms(const nus_upscaler *h, double *ms_out);
/* Device-path kernel timing.  With profiling enabled every nus_upscaler_upscale_device call
 * brackets its main kernel launch with a hipEvent pair on the caller's stream (the Lanczos
 * edge-column pass is outside the bracket); profile_collect waits for the recorded pairs,
 * returns the number of launches and their summed duration, and resets the counters. */
int nus_upscaler_set_profiling(nus_upscaler *h, int enabled);
int nus_upscaler_profile_collect(nus_upscaler *h, uint64_t *launches, double *total_ms);
/* Name of the kernel variant chosen at initialize (e.g. "lanczos3_x2_regwin"). */
const char *nus_upscaler_kernel_variant(const nus_upscaler *h);

/* Shared LUT exchange for multi-GPU runs: rank 0 exports the per-axis tables built at
 * initialize, the blob is broadcast (RCCL), other ranks import it so every GPU uses
 * bit-identical weights.  export returns the blob size (or negative status);
 * with buf == NULL it only reports the size. */
int64_t nus_upscaler_export_tables(const nus_upscaler *h, void *buf, size_t cap);
int nus_upscaler_import_tables(nus_upscaler *h, const void *buf, size_t len);

/* Host-only (no GPU needed): build the same blob directly from the dimensions, and
 * check a received blob against them.  variant: nus_bilinear_variant. */
int64_t nus_tables_build_blob(uint32_t in_w, uint32_t in_h, uint32_t out_w, uint32_t out_h,
                              int variant, void *buf, size_t cap);
int64_t nus_tables_build_blob_for(int algorithm, uint32_t in_w, uint32_t in_h, uint32_t out_w,
                                  uint32_t out_h, int variant, void *buf, size_t cap);
int nus_tables_validate_blob(const void *buf, size_t len, uint32_t in_w, uint32_t in_h,
                             uint32_t out_w, uint32_t out_h);

/* ---- host-only table builders (no GPU needed; used by initialize) --------------- */

#define NUS_RESIZE_MAX_TAPS 32

/* Lanczos-3 tap windows of one axis, image-0.24.9 convention (half-pixel centres,
 * support 3*max(in/out,1), weights normalised to sum 1).  left/ntaps: out_n entries;
 * weights: out_n * NUS_RESIZE_MAX_TAPS floats, zero padded.
 * Returns the largest ntaps or a negative status. */
int nus_lanczos3_build_axis(uint32_t in_n, uint32_t out_n, int32_t *left,
                            uint32_t *ntaps, float *weights);
/* Same for filter 0 = Lanczos3, 1 = CatmullRom, 2 = Triangle. */
int nus_resize_build_axis(int filter, uint32_t in_n, uint32_t out_n, int32_t *left,
                          uint32_t *ntaps, float *weights);
/* Nearest source index per output index: min(o*in_n/out_n, in_n-1). */
int nus_nearest_build_axis(uint32_t in_n, uint32_t out_n, uint32_t *src);
/* Bilinear i0 / frac per output index. variant: nus_bilinear_variant. */
int nus_bilinear_build_axis(uint32_t in_n, uint32_t out_n, int variant,
                            uint32_t *i0, float *frac);

/* ---- Frame interpolator (WgpuFrameInterpolator) -------------------------------- */

/* WgpuFrameInterpolator::new_py(preset) (wgpu_interpolator.rs:172-212). */
nus_interp *nus_interp_create(int wg_preset);
void nus_interp_destroy(nus_interp *h);
int nus_interp_set_device(nus_interp *h, int device);
/* Channel order of BOTH input frames (see nus_upscaler_set_input_format); the new frame is RGBA8. */
int nus_interp_set_input_format(nus_interp *h, int format);
/* Element type of the flow field nus_interp_interpolate_device reads: NUS_FLOW_F32 (default, 2 x f32 per pixel,
 * the Rg32Float layout of wgpu_interpolator.rs:1211, :1418) or NUS_FLOW_F16 (2 x IEEE half per pixel, the
 * Rg16Float texture the reference's live path binds, wgpu_interpolator.rs:276: half the flow bytes).  Each
 * half is widened to f32 exactly and the arithmetic is the same.  The host entry point always takes f32. */
typedef enum nus_flow_format {
    NUS_FLOW_F32 = 0,
    NUS_FLOW_F16 = 1
} nus_flow_format;
int nus_interp_set_flow_format(nus_interp *h, int format);
/* Arithmetic of the dense-flow warp (flow != NULL), as nus_upscaler_set_lanczos_mode for the resize filters:
 *   NUS_INTERP_MODE_EXACT (default)  every product and sum rounded separately, as the CPU code of
 *                                    interpolation/mod.rs:467-510 and :386-411 -- bit-exact against the oracle;
 *   NUS_INTERP_MODE_FMA              each sample position as one fused multiply-add and each bilinear lerp as
 *                                    fma(b, f, a (1 - f)), one product and one fused multiply-add (the blend of the two
 *                                    truncated samples keeps the CPU's roundings): 0.8x the instructions.  Contract (DESIGN.md
 *                                    section 2, tests/_warp64.py): each truncated sample is the floor of the float64 bilinear
 *                                    value at the real position, or the neighbouring count where that value lies within
 *                                    255 (ex + ey) + 2^-14 of an integer, ex / ey half an f32 ulp of the coordinates; the byte
 *                                    is the CPU's blend of two such samples.  Against EXACT that is within 1 LSB, with fewer
 *                                    than 0.1 % of the samples different on frames of 328 x 200 and more.
 * The zero-flow path (the reference's live behaviour) is the same exact streaming blend in both modes. */
typedef enum nus_interp_mode_t { NUS_INTERP_MODE_EXACT = 0, NUS_INTERP_MODE_FMA = 1 } nus_interp_mode_t;
int nus_interp_set_mode(nus_interp *h, int mode);
int nus_interp_mode(const nus_interp *h);
/* Projection rounds of the dense-flow warp: the flow evaluated at the in-between time (off by default: 0).  BUILD-DEFINED -- the
 * reference has nothing like it.  A flow f lives on frame A's grid: f(q) says where A's pixel q goes.  The warp reads it at the
 * OUTPUT pixel p of the in-between frame, but the content that is at p at time t came from the A-pixel q with q + t f(q) = p, and
 * its vector is f(q); within t |f| pixels of a motion boundary the two differ by the whole motion difference.  With rounds = N > 0
 * the warp of one pair of w x h with flow f (f32, or Rg16Float widened exactly) computes for output pixel p = (x, y) and time t
 *     g = f[y][x]
 *     repeat N times:
 *         qx = clamp(x - t g.x, 0, w-1);  qy = clamp(y - t g.y, 0, h-1)      (f32; t g.x one product, then one subtraction)
 *         x0 = floor(qx); x1 = min(x0+1, w-1); fx = qx - x0                  (the same in y)
 *         top = f[y0][x0] (1-fx) + f[y0][x1] fx;  bot = f[y1][x0] (1-fx) + f[y1][x1] fx
 *         g   = top (1-fy) + bot fy          (per component; every product and sum rounded separately)
 * and then samples and blends exactly as without the setting, with g in place of f[y][x].  The projection arithmetic is the same in
 * NUS_INTERP_MODE_EXACT and NUS_INTERP_MODE_FMA (separate roundings, no contraction); only the two frame samples that follow differ
 * by mode: an EXACT frame is the oracle's warp + blend with the flow g byte for byte, an FMA frame is held by the FMA contract above
 * with g as the flow.  g stays f32 (never re-rounded to half).  At the right / bottom border the kernels may read the cell pair
 * (w-2, w-1) with fraction 1 instead of (w-1, w-1) with fraction 0: the same value (flows compare as values, -0 equals +0; NaN and
 * Inf flows are out of contract).  t = 0 gives g = f[y][x]; odd and even N oscillate at boundary cells, which is why N is a setting
 * (measured gains: DESIGN.md 8.1).  Every gather stays inside its own pair's flow plane.  The setting applies to every
 * nus_interp_interpolate* entry point given a flow (the multi-time ones project per time); flow == NULL runs the unchanged zero-flow
 * kernel, and with rounds = 0 every entry point launches the kernels and writes the bytes it did before the setting existed.  No
 * workspace.  rounds > NUS_FLOW_MAX_PROJECT: NUS_ERR_INVALID_ARGUMENT before any HIP call, the text beginning
 * "nus_interp_set_flow_project:", the setting unchanged. */
#define NUS_FLOW_MAX_PROJECT 4
int nus_interp_set_flow_project(nus_interp *h, uint32_t rounds);
int nus_interp_flow_project(const nus_interp *h);

/* trait FrameInterpolator (nu_scaler_core/src/interpolation/mod.rs:29-44) -- the shape the dead-code trait gives an
 * interpolator, next to the live pyclass's per-call form below:
 *   initialize(width, height)          :31  buffers for that frame size up front; same size again = no-op (:306-308)
 *   interpolate(frame1, frame2, t)     :34  frames of the initialize() size, zero flow; before initialize:
 *                                           NUS_ERR_NOT_INITIALIZED, "Interpolator not initialized" (:368-370)
 *   name()                             :37
 *   set_quality(q) / quality()         :40-43  nus_interp_quality_level; kept and reported, arithmetic unchanged */
typedef enum nus_interp_quality_level {
    NUS_INTERP_QUALITY_HIGH = 0, /* InterpolationQuality::High   (interpolation/mod.rs:8-14) */
    NUS_INTERP_QUALITY_MEDIUM = 1,
    NUS_INTERP_QUALITY_LOW = 2
} nus_interp_quality_level;
int nus_interp_initialize(nus_interp *h, uint32_t width, uint32_t height);
int nus_interp_interpolate_frames(nus_interp *h, const uint8_t *frame1, size_t len1, const uint8_t *frame2, size_t len2,
                                  float t, uint8_t *out, size_t out_cap);
const char *nus_interp_name(const nus_interp *h);
int nus_interp_set_quality(nus_interp *h, int quality);
int nus_interp_quality(const nus_interp *h);

/* interpolate_py (wgpu_interpolator.rs:215-491): host frames in, host frame out.
 * flow == NULL -> zero flow (the live reference behaviour); otherwise w*h*2 floats
 * (dx, dy) = pixel delta from frame A to frame B (warp_blend.wgsl:29-37).
 * a_len and b_len must equal w*h*4 (else NUS_ERR_SIZE_MISMATCH with the text of
 * wgpu_interpolator.rs:234-237); out_cap >= w*h*4. */
int nus_interp_interpolate(nus_interp *h, const uint8_t *a, size_t a_len,
                           const uint8_t *b, size_t b_len, const float *flow,
                           uint32_t w, uint32_t hgt, float t,
                           uint8_t *out, size_t out_cap);

/* Device-resident path: n_pairs independent pairs; pair i reads
 * d_a + i*a_stride, d_b + i*b_stride (byte strides; a sliding stream uses
 * d_b = d_a + frame_bytes with both strides = frame_bytes), optional
 * d_flow + i*w*h*8 (NUS_FLOW_F32; i*w*h*4 and 4-byte alignment with NUS_FLOW_F16), writes d_out + i*w*h*4.
 * Enqueued on `stream`, no sync. */
int nus_interp_interpolate_device(nus_interp *h, const void *d_a, size_t a_stride,
                                  const void *d_b, size_t b_stride,
                                  const void *d_flow, uint32_t w, uint32_t hgt,
                                  float t, void *d_out, uint32_t n_pairs, void *stream);

/* ---- Several in-between frames per pair (frame-rate multipliers 2x .. 8x) ------------
 * One launch reads each pair's A, B (and flow) once and writes the frame of every time in the set: frame k is byte for byte what
 * the single-t entry point writes at times[k], in the handle's mode, flow format and input format.  frame_times of the Python
 * package gives the times of a multiplier M: k / M for k = 1 .. M - 1.
 * Unlike nus_interp_interpolate_device, which takes any t, these entry points require 1 <= n_times <= NUS_INTERP_MAX_TIMES and
 * every time in [0, 1] (NaN is rejected).  Argument errors are NUS_ERR_INVALID_ARGUMENT, returned before any HIP call, with a
 * last_error text that names the entry point. */
/* up to 8x frame rate */
#define NUS_INTERP_MAX_TIMES 7

/* n_pairs pairs as nus_interp_interpolate_device (same pointer, stride and flow alignment); n_times in-between frames per pair, at
 * times[0..n_times).  Frame (i, k) at d_out + i * out_pair_stride + k * w*h*4; out_pair_stride 0 = n_times * w*h*4 (tightly
 * packed), else a multiple of 4 of at least n_times * w*h*4.  A stride of (n_times + 1) * w*h*4 leaves a gap per pair, so the
 * caller can put the real frame there (display order); the gap is not written.  `times` is read during the call and copied into
 * the launch.  n_pairs == 0: NUS_OK, nothing launched.  Enqueue only: no allocation, no synchronisation. */
int nus_interp_interpolate_multi_device(nus_interp *h, const void *d_a, size_t a_stride, const void *d_b, size_t b_stride,
                                        const void *d_flow, uint32_t w, uint32_t hgt, const float *times, uint32_t n_times,
                                        void *d_out, size_t out_pair_stride, uint32_t n_pairs, void *stream);
/* Host frames in (as nus_interp_interpolate, whose NUS_ERR_SIZE_MISMATCH and text it shares); n_times frames out, back to back
 * (out_cap >= n_times * w*h*4).  nus_interp_last_gpu_ms then reports the one multi-time launch. */
int nus_interp_interpolate_multi(nus_interp *h, const uint8_t *a, size_t a_len, const uint8_t *b, size_t b_len,
                                 const float *flow, uint32_t w, uint32_t hgt, const float *times, uint32_t n_times,
                                 uint8_t *out, size_t out_cap);

/* ---- The select warp: two flows per pair, each pixel takes the vector whose samples agree better ------------
 * BUILD-DEFINED -- the reference has nothing like it.  A flow A -> B is worst where A's content has no counterpart in B (background
 * about to be covered, content leaving the frame); the flow B -> A is worst somewhere else.  One pair of w x h frames A and B at
 * time t: F is the flow A -> B on A's grid, R the flow B -> A on B's grid (both f32, or Rg16Float widened exactly), N the handle's
 * projection rounds (nus_interp_set_flow_project, 0 .. NUS_FLOW_MAX_PROJECT), nt = 1.0f - t in f32.  Per output pixel p:
 *     gF = F projected N rounds at time t, exactly as the rule above nus_interp_set_flow_project states it
 *     gR = -(R projected N rounds at time nt) by the same rule: the content at p came from the B-pixel q with q + nt R(q) = p
 *          (N = 0: gR = -R[y][x]; the negation is exact)
 *     per candidate g: sa = A sampled at p - t g, sb = B sampled at p + nt g, exactly as the dense-flow warp samples them in the
 *          handle's mode (clamp, bilinear weights, truncation to an integer count held in f32)
 *     e(g) = |sa0 - sb0| + |sa1 - sb1| + |sa2 - sb2| over the three colour bytes of the pixel as stored; alpha does not vote.  An
 *          integer 0 .. 765, exact in f32, symmetric in R and B: RGBA and BGRA input order give the same choice
 *     the backward candidate wins if and only if e(gR) < e(gF); a tie goes forward
 *     the pixel is the dense-flow warp's three-rounding blend trunc(nt sa + t sb) of the WINNER's samples, then the input channel
 *          selector as there
 * So with R = -F and N = 0 every pixel is a tie and the frame is byte for byte nus_interp_interpolate_multi_device's with F; an EXACT
 * frame is, pixel by pixel, the oracle's warp + blend with flow gF or with flow gR, whichever the rule names; an FMA pixel meets the
 * FMA contract with gF or gR as its flow, and it is the rule's choice wherever |e(gF) - e(gR)| > 12 on the EXACT samples (an FMA
 * sample is within one count of the EXACT one).  Measured gains over the forward flow alone: DESIGN.md 8.1.
 *
 * nus_interp_interpolate_select_device: pointers, strides, alignment, time-set rules, output layout and error behaviour are those of
 * nus_interp_interpolate_multi_device (n_times = 1 is the single-time call); pair i's flows at d_flow_fwd / d_flow_bwd + i * w*h*8
 * (w*h*4 with NUS_FLOW_F16).  Both flows are required: a NULL flow is NUS_ERR_INVALID_ARGUMENT before any HIP call, the text
 * beginning "nus_interp_interpolate_select_device:".  It honours the handle's mode, flow format, input format and flow_project.
 * Enqueue only: no allocation, no workspace, no synchronisation. */
int nus_interp_interpolate_select_device(nus_interp *h, const void *d_a, size_t a_stride, const void *d_b, size_t b_stride,
                                         const void *d_flow_fwd, const void *d_flow_bwd, uint32_t w, uint32_t hgt,
                                         const float *times, uint32_t n_times, void *d_out, size_t out_pair_stride, uint32_t n_pairs,
                                         void *stream);
/* The host form: host frames and two f32 flows of w*h*2 floats in, n_times frames out back to back.  Checks and texts as
 * nus_interp_interpolate_multi (with this entry point's name), and a NULL flow is refused as above. */
int nus_interp_interpolate_select(nus_interp *h, const uint8_t *a, size_t a_len, const uint8_t *b, size_t b_len,
                                  const float *flow_fwd, const float *flow_bwd, uint32_t w, uint32_t hgt, const float *times,
                                  uint32_t n_times, uint8_t *out, size_t out_cap);

/* get_last_gpu_duration_ms: NUS_OK and *ms_out set, or NUS_ERR_NOT_INITIALIZED when
 * no interpolation has run yet (the reference returns None). */
int nus_interp_last_gpu_ms(const nus_interp *h, double *ms_out);
const char *nus_interp_last_error(const nus_interp *h);

/* ---- Frame queue + capture swizzle ("next" row: SURVEY.md section 8f rank 3) -----------
 * nus_frame_queue mirrors the legacy FrameBuffer (Nu_scale/src/capture/frame_buffer.rs:11-100):
 * bounded, drop-oldest on overflow, consumers read the latest frame.  Host memory only. */
typedef struct nus_frame_queue nus_frame_queue;

nus_frame_queue *nus_frame_queue_create(size_t capacity); /* reference default: 5 */
void nus_frame_queue_destroy(nus_frame_queue *q);
/* Copies the frame in; returns the total number of frames dropped so far (>= 0) or a status. */
int64_t nus_frame_queue_add(nus_frame_queue *q, const uint8_t *rgba, uint32_t w, uint32_t hgt);
/* Latest frame (stays queued) / oldest frame (removed).  Waits up to timeout_ms when empty.
 * Returns 1 and fills out (cap >= w*h*4), 0 when no frame arrived, negative status on error. */
int nus_frame_queue_latest(nus_frame_queue *q, int64_t timeout_ms, uint8_t *out, size_t out_cap,
                           uint32_t *w, uint32_t *hgt, uint64_t *sequence);
int nus_frame_queue_pop(nus_frame_queue *q, int64_t timeout_ms, uint8_t *out, size_t out_cap,
                        uint32_t *w, uint32_t *hgt, uint64_t *sequence);
size_t nus_frame_queue_size(const nus_frame_queue *q);
size_t nus_frame_queue_capacity(const nus_frame_queue *q);
uint64_t nus_frame_queue_dropped(const nus_frame_queue *q);

/* BGRA -> RGBA of a captured frame on the GPU (the CPU loop of nu_scaler_core/src/lib.rs:251-270).
 * Device pointers, n_pixels pixels, in place allowed; enqueues on `stream`. */
int nus_swizzle_bgra_to_rgba_device(const void *d_in, void *d_out, size_t n_pixels, void *stream);

/* ---- Optical-flow front end ("next" row: SURVEY.md section 8f rank 1) --------------
 * Mirrors WgpuFrameInterpolator::build_pyramid / compute_coarse_flow
 * (nu_scaler_core/src/wgpu_interpolator.rs:969-1203) and the shaders
 * gaussian_blur_{h,v}.wgsl, downsample.wgsl, horn_schunck.wgsl, flow_upsample.wgsl.
 * Images: f32 RGBA (4 floats / pixel, u8/255); flows: 2 floats / pixel (dx, dy), the
 * pixel delta from frame A to frame B that nus_interp_interpolate consumes. */
typedef struct nus_flow nus_flow;

nus_flow *nus_flow_create(void);
void nus_flow_destroy(nus_flow *h);
int nus_flow_set_device(nus_flow *h, int device);
/* 1 (default): derivatives once per level and several Jacobi steps per launch, the kernel chosen by
 * the size of the batch (2: always the LDS-tile kernel, 3: always the register-pipelined one);
 * 0: one plain kernel per step, the shader's structure.  Results are bit-identical. */
int nus_flow_set_tiled(nus_flow *h, int enabled);
/* Arithmetic of the estimators' Horn-Schunck steps, as nus_upscaler_set_lanczos_mode / nus_interp_set_mode have it for their
 * kernels.  NUS_FLOW_EXACT (default): every stage bit-identical to the oracle's restatement of the shaders.  NUS_FLOW_FAST: the
 * Jacobi steps with separable 3x3 sums, a multiply by 1/9, a precomputed reciprocal of lambda + Ix^2 + Iy^2 and FMAs
 * (shaders/horn_schunck.wgsl:24-92 in its cheapest f32 form; every level in the register-pipelined kernel) -- the flow within
 * 1e-3 px of the exact one, the frame interpolated with it within 1 LSB on < 0.1 % of its samples; 2.2x fewer instructions per
 * step.  The 1e-3 px bound holds for lambda >= 4e-4 (the default) and is checked against a float64 restatement of the shaders
 * (tests/_flow64.py).  For a smaller lambda it is NOT promised: the problem becomes ill-conditioned (lambda = 1e-6 on noise: flows
 * beyond 50 px, and the exact f32 arithmetic itself is more than 1e-3 px from the float64 result -- both asserted in
 * tests/test_flow.py), and FAST then stays within 3.1x the distance of the exact mode's own result from the float64 one
 * (measured at lambda = 1e-6: 0.56x on noise, 0.78x on a static scene; the test allows four times the larger).
 * With nus_flow_set_warps(W >= 1) the bound is the larger of 1e-3 px and four times that same distance (the exact f32 result's
 * from the float64 one, on the same pair): the finer levels re-linearise about a flow that carries the coarsest level's FAST
 * difference, doubled per level, and every further round samples frame B where the round before left it, so the estimate
 * amplifies a difference of a few ulps as it amplifies the exact arithmetic's own roundings.  Measured against the CPU float32
 * restatement (tests/test_gpu_flow_warp_lattice.py asserts the bound): W = 1 at most 3.5e-4 px on every case; W = 4 below
 * 1e-3 px except 1.01e-3 px on a 4-level estimate (exact f32 4.7e-4 px from float64: 2.1x) and 2.7e-3 / 1.6e-3 px on two
 * pairs with 45 - 59 px flows where exact f32 is itself 1.8e-3 / 1.3e-3 px from float64 (1.5x, 1.2x); the same cases with
 * W = 0 stay within 1e-3 px.
 * EXACT is bit-identical for every operand, subnormal flows around a local change on a static background included.
 * The reference never runs this front end (wgpu_interpolator.rs:1156-1203 is unwired), so neither mode has a fixture.
 * The primitives below are always exact. */
#define NUS_FLOW_EXACT 0
#define NUS_FLOW_FAST 1
int nus_flow_set_mode(nus_flow *h, int mode);
int nus_flow_mode(const nus_flow *h);
/* Re-linearisation of the finer pyramid levels about the flow they start from (off by default: 0).  Without it every level's data
 * term is linearised about zero flow, It = L2(x) - L1(x), and the upsampled coarser flow is only the Jacobi start value: motion of
 * more than about a pixel is not followed.  With warps = W (0 .. NUS_FLOW_MAX_WARPS) every level but the coarsest runs W rounds
 * after its x2 upsample; a round takes the level's current flow f0 = (u0, v0) (round 1: the upsampled one), samples frame B's
 * luminance plane bilinearly at (x + u0, y + v0) -- coordinates clamped into the plane, pixel centres at integers, the dense warp's
 * sampler -- forms It' = ((L2w - L1) - Ix*u0) - Iy*v0 and runs `refine_iters` Jacobi steps from f0 on (Ix, Iy, It'), i.e. on
 * Ix (u - u0) + Iy (v - v0) + (L2w - L1) = 0 (the intent of the reference's flow_refine.wgsl:94-106, which is not valid WGSL and
 * never runs).  The setting applies to every estimator entry point of the handle (nus_flow_estimate, _estimate_device,
 * _estimate_device_stream, _interpolate_device_stream, _interpolate_multi_device_stream); it may be changed at any time; with 0
 * every entry point writes the bytes and reserves the workspace it did before the setting existed.  A warped level costs one gather
 * launch per round plus the round's Jacobi steps, and 12 B of coefficient planes per cell and pair of workspace; in NUS_FLOW_FAST
 * its Jacobi steps run in the exact kernels; the pyramid and the coarsest level stay FAST (nus_flow_set_mode: FAST's bound
 * with warps).  A value above NUS_FLOW_MAX_WARPS: NUS_ERR_INVALID_ARGUMENT, the setting unchanged. */
#define NUS_FLOW_MAX_WARPS 4
int nus_flow_set_warps(nus_flow *h, uint32_t warps);
int nus_flow_warps(const nus_flow *h);
/* Median filter of the flow behind every Jacobi run (off by default: 0; Sun, Roth and Black, "Secrets of optical flow estimation",
 * CVPR 2010).  The quadratic smoothness term turns a motion boundary into a ramp several cells wide, and every re-linearisation
 * round then samples frame B through that ramp and keeps it; a median removes the ramp and the outliers and keeps the edge.  With
 * size = 3 or 5, after every Jacobi run of an estimate -- the coarsest level's `coarse_iters` steps, a finer level's
 * `refine_iters` steps, with nus_flow_set_warps each of a finer level's rounds -- the level's flow is replaced by its component-wise
 * size x size median: u and v separately, the window centred on the cell, coordinates clamped into the level (replicated border).
 * A run of zero steps is followed by no median.  What the next stage reads -- the x2 upsample, the next round's gather, the caller
 * or the warp -- is the filtered flow.  The median is a selection (the 5th of 9, the 13th of 25 values): it rounds nothing and is the
 * same kernel in NUS_FLOW_EXACT and NUS_FLOW_FAST (FAST's bound is the one nus_flow_set_mode states for warps); where +0 and -0
 * tie either may be returned, and NaNs are out of contract.
 * The mode is meant for warps >= 1: there, on the float64 witness of tests/_flow_median.py, it gains the t = 0.5 frame
 * +0.3 .. +1.5 dB PSNR (3 x 3) and +0.5 .. +2.1 dB (5 x 5) on frames of 192 px and more; with warps = 0 the result is mixed
 * (-0.2 .. +0.8 dB).  A 5 x 5 window on a small frame's coarsest level covers much of a small object (96 x 64, 3 levels: 3 x 3 is
 * the better choice), which is why the size is a setting.  The setting applies to every estimator entry point of the handle
 * (nus_flow_estimate, _estimate_device, _estimate_device_stream, _interpolate_device_stream, _interpolate_multi_device_stream); it
 * may be changed at any time; with 0 every entry point writes the bytes and reserves the workspace it did before the setting
 * existed.  Cost: one launch per Jacobi run that moves 16 B per cell (8 read, 8 written) through the flow ping-pong -- no new
 * workspace, except that a FAST stream with the Rg16Float hand-off and no d_flows keeps its halves beside the flows, 4 B per cell
 * and pair -- and, with the median on, the finest level's last Jacobi launch no longer writes the caller's buffer or Rg16Float
 * halves itself (the median writes the caller's f32 buffer; halves are converted afterwards).  Time per pair: DESIGN.md 8.1.
 * Any other size: NUS_ERR_INVALID_ARGUMENT, the text beginning "nus_flow_set_median:", the setting unchanged. */
#define NUS_FLOW_MEDIAN_MAX 5
int nus_flow_set_median(nus_flow *h, uint32_t size);
int nus_flow_median_size(const nus_flow *h);
/* Bytes of device workspace the handle holds now (grow-only; 0 for a null handle or before the first call that needs a device). */
size_t nus_flow_workspace_bytes(nus_flow *h);
/* TEST HOOK: every byte of the handle's device workspace -- every slot, over its whole capacity -- set to byte_value (0..255) on
 * `stream`, which is synchronised before the call returns (so the host entry points, which run on the handle's own stream, see
 * the fill as well).  What the tests use to show that no result depends on what the workspace held before the call.  Refused with
 * NUS_ERR_INVALID_ARGUMENT, the text beginning "nus_flow_fill_workspace:", unless the PROCESS has NUS_TEST_HOOKS=1 in its
 * environment (read per call), and for a value outside 0..255.  A null handle, or one that has reserved nothing: NUS_OK, no HIP call. */
int nus_flow_fill_workspace(nus_flow *h, int byte_value, void *stream);
/* Projection rounds (BUILD-DEFINED; the rule is stated at nus_interp_set_flow_project) of the warp behind the estimator:
 * nus_flow_interpolate_device_stream and nus_flow_interpolate_multi_device_stream (per time) warp with the projected vector g
 * instead of the flow at the output pixel.  0 (default) .. NUS_FLOW_MAX_PROJECT.  The flows written to d_flows are unchanged, the
 * estimate entry points are untouched, no workspace is added; the frames equal nus_flow_estimate_device_stream followed by
 * nus_interp_interpolate_multi_device in FMA mode with the same rounds.  With 0: the kernels and bytes from before the setting.
 * rounds > NUS_FLOW_MAX_PROJECT: NUS_ERR_INVALID_ARGUMENT before any HIP call, the text beginning "nus_flow_set_project:". */
int nus_flow_set_project(nus_flow *h, uint32_t rounds);
int nus_flow_project_rounds(const nus_flow *h);
/* Both flows of every pair and the select warp behind the estimator (BUILD-DEFINED; the rule is stated at
 * nus_interp_interpolate_select_device).  Off by default; off means the kernels, the bytes and the nus_flow_workspace_bytes from
 * before the setting existed (turning it off frees the slots it added).  On, nus_flow_interpolate_device_stream and
 * nus_flow_interpolate_multi_device_stream estimate every pair both ways -- the flow B -> A of a pair is the same coarse-to-fine
 * schedule on the same pyramids with the pair's two luminance planes swapped, honouring warps and median -- and warp with the select
 * kernel in FMA mode with the handle's projection rounds: the frames equal nus_interp_interpolate_select_device in FMA mode fed
 * with the forward and the backward estimate of each pair.  Both estimator families support it, the batch path and the pair-by-pair
 * shader-shaped path.  In the batch path the backward solve's Jacobi steps run the exact kernels on coefficient planes, in
 * NUS_FLOW_FAST too (inside FAST's contract, as a re-linearised level's).  So in NUS_FLOW_FAST, where the forward solve runs the
 * streamed FAST kernels, the backward flow is NOT the bytes nus_flow_estimate_device returns for (B, A) in that mode, and the frames
 * have no byte reference: each flow is within FAST's bound of the exact estimate of its direction, and every pixel is the select
 * warp's for flows within that bound.  In NUS_FLOW_EXACT the equality above holds byte for byte, the backward estimate being
 * nus_flow_estimate_device of (B, A).  d_flows, when given, receives the forward flows only, the
 * bytes it receives with the setting off for every stream whose chunk size the setting's workspace (28 B per pixel and pair more)
 * does not change; the backward flows stay in the workspace.  The stream rule below holds.  nus_flow_estimate* is not affected, and
 * scene detection applies behind the warp as before.  nus_flow_retime_device_stream with the setting on returns
 * NUS_ERR_INVALID_ARGUMENT before any HIP call ("... bidirectional flow is not supported by rate conversion yet"): rate conversion
 * with the select warp is nus_flow_retime_select_device_stream, and the backward flows leave the workspace through
 * nus_flow_estimate_both_device_stream; neither looks at this setting.
 * enabled other than 0 or 1: NUS_ERR_INVALID_ARGUMENT, the text beginning "nus_flow_set_bidirectional:", the setting unchanged. */
int nus_flow_set_bidirectional(nus_flow *h, int enabled);
int nus_flow_bidirectional(const nus_flow *h);
const char *nus_flow_last_error(const nus_flow *h);

/* primitives on host buffers */
int nus_flow_rgba8_to_f32(nus_flow *h, const uint8_t *in, uint32_t w, uint32_t hgt, float *out);
int nus_flow_blur(nus_flow *h, const float *in, uint32_t w, uint32_t hgt, float *out); /* H pass, then V pass */
int nus_flow_downsample(nus_flow *h, const float *in, uint32_t w, uint32_t hgt, float *out); /* -> (w+1)/2 x (h+1)/2 */
/* `iterations` Jacobi steps; flow_in == NULL starts from zero (compute_coarse_flow). */
int nus_flow_horn_schunck(nus_flow *h, const float *i1, const float *i2, const float *flow_in,
                          uint32_t w, uint32_t hgt, float lambda, uint32_t iterations, float *flow_out);
int nus_flow_upsample(nus_flow *h, const float *src, uint32_t sw, uint32_t sh,
                      float *dst, uint32_t dw, uint32_t dh, float scale);
/* The stage nus_flow_set_median adds, on its own: the component-wise size x size median (3 or 5) of a w*h*2 flow, border
 * replicated.  size and pointers are checked before any HIP call. */
int nus_flow_median(nus_flow *h, const float *flow_in, uint32_t w, uint32_t hgt, uint32_t size, float *flow_out);
/* The projection of nus_interp_set_flow_project on its own (BUILD-DEFINED): flow_out = the vector g of every cell of a w*h*2 f32
 * flow after `rounds` rounds (0 .. NUS_FLOW_MAX_PROJECT; 0 copies) at time t -- the device function of the projecting warp
 * kernels.  rounds above the bound, a NaN t and null pointers are refused before any HIP call, the text beginning
 * "nus_flow_project:". */
int nus_flow_project(nus_flow *h, const float *flow_in, uint32_t w, uint32_t hgt, float t, uint32_t rounds, float *flow_out);
/* The two halves of a re-linearised level (nus_flow_set_warps), always exact.  _warp_coefficients: f32 RGBA images and a w*h*2
 * flow -> w*h*3 floats (Ix, Iy, It') per cell; flow == NULL is zero flow and gives (Ix, Iy, It = L2 - L1).
 * _horn_schunck_coef: `iterations` Jacobi steps on such coefficients; flow_in == NULL starts from zero. */
int nus_flow_warp_coefficients(nus_flow *h, const float *i1, const float *i2, const float *flow, uint32_t w, uint32_t hgt,
                               float *coef_out);
int nus_flow_horn_schunck_coef(nus_flow *h, const float *coef, const float *flow_in, uint32_t w, uint32_t hgt, float lambda,
                               uint32_t iterations, float *flow_out);

/* Full estimator: pyramids of both RGBA8 frames (`levels`), `coarse_iters` steps from zero
 * flow at the coarsest level, then per finer level a x2 upsample (vectors x2) and
 * `refine_iters` steps.  flow_out: w*h*2 floats. */
int nus_flow_estimate(nus_flow *h, const uint8_t *a, const uint8_t *b, uint32_t w, uint32_t hgt,
                      uint32_t levels, uint32_t coarse_iters, uint32_t refine_iters, float lambda,
                      float *flow_out);
/* THE STREAM RULE of the device entry points below (nus_flow_estimate_device, _estimate_device_stream, _interpolate_device_stream,
 * _interpolate_multi_device_stream).  All calls of one handle share its device workspace, and no call's result depends on what the
 * workspace held before it.  Calls enqueued on ONE stream need no synchronisation between them, whatever their sizes and settings:
 * stream order keeps a call's kernels behind the previous call's, and a call that has to grow the workspace waits for the device
 * before it frees the old memory.  Before the handle is used from ANOTHER stream, or a host entry point is called (nus_flow_estimate
 * and the primitives run on the handle's own stream), the caller synchronises the stream of the calls before: nothing else orders
 * the two streams' kernels in the shared workspace. */
/* Device-resident variant; enqueues on `stream`, no synchronisation. */
int nus_flow_estimate_device(nus_flow *h, const void *d_a, const void *d_b, uint32_t w, uint32_t hgt,
                             uint32_t levels, uint32_t coarse_iters, uint32_t refine_iters, float lambda,
                             void *d_flow_out, void *stream);
/* Flows between consecutive frames of a device-resident stream (what the interpolator's batch entry
 * point consumes): d_frames = n_frames RGBA8 frames back to back, d_flows = n_frames - 1 flows,
 * flow k = frame k -> frame k+1.  Same result as n_frames - 1 calls of nus_flow_estimate_device;
 * each frame's pyramid is built once.  Enqueues on `stream`, no synchronisation. */
int nus_flow_estimate_device_stream(nus_flow *h, const void *d_frames, uint32_t n_frames, uint32_t w, uint32_t hgt,
                                    uint32_t levels, uint32_t coarse_iters, uint32_t refine_iters, float lambda,
                                    void *d_flows, void *stream);
/* Motion-compensated interpolation of a device-resident stream as ONE pipeline -- the reference's intended interpolate()
 * (wgpu_interpolator.rs:881-935: build_pyramid -> compute_coarse_flow -> warp): the n_frames - 1 flows of
 * nus_flow_estimate_device_stream AND the in-between frame of every pair (k, k + 1) at time_t in [0, 1], warped + blended with that
 * flow (warp_blend.wgsl:25-43; dense-flow warp in FMA mode: within 1 LSB of the CPU blend, as nus_interp_set_mode(.., FMA)), tightly
 * packed RGBA8 at d_mid.  d_flows may be NULL (the in-between frames only: the flows then stay in the estimator's workspace).
 * flow_format: NUS_FLOW_F32 -- same bytes as nus_flow_estimate_device_stream followed by nus_interp_interpolate_device in FMA mode;
 * NUS_FLOW_F16 -- the flows between estimator and warp (and at d_flows: w*h*4 bytes per pair) are the reference's live layout,
 * Rg16Float (wgpu_interpolator.rs:276): each the f32 flow rounded to nearest even, and the warp reads them as such (2^-11 relative
 * resolution: 5e-4 px on a 1-2 px flow; half the bytes of the hand-off).  Pointers 16-byte aligned. */
int nus_flow_interpolate_device_stream(nus_flow *h, const void *d_frames, uint32_t n_frames, uint32_t w, uint32_t hgt,
                                       uint32_t levels, uint32_t coarse_iters, uint32_t refine_iters, float lambda, float time_t,
                                       int flow_format, void *d_flows, void *d_mid, void *stream);
/* As nus_flow_interpolate_device_stream, but each pair's flow is estimated ONCE and all n_times frames are warped from it (one
 * multi-time warp launch in FMA mode behind the estimator).  Pair k's frame j goes to d_mid + k * mid_pair_stride + j * w*h*4
 * (0 = tightly packed; else a multiple of 4 of at least n_times * w*h*4).  Every frame equals the single-t call's at times[j]; the
 * flows at d_flows (when not NULL) are the same bytes.  Time-set rules and argument checks as nus_interp_interpolate_multi_device. */
int nus_flow_interpolate_multi_device_stream(nus_flow *h, const void *d_frames, uint32_t n_frames, uint32_t w, uint32_t hgt,
                                             uint32_t levels, uint32_t coarse_iters, uint32_t refine_iters, float lambda,
                                             const float *times, uint32_t n_times, int flow_format, void *d_flows,
                                             void *d_mid, size_t mid_pair_stride, void *stream);

/* ---- Image-quality metrics (ErrorMetrics::calculate, Nu_scale/src/upscale/common.rs:475-543) ------------------
 * MSE, PSNR and SSIM of RGBA8 frame pairs of one size and channel order; alpha is ignored, so every metric is symmetric in R
 * and B (BGRA and the X formats need no swizzle).
 *   MSE  = SSE / (3 W H), SSE = sum over pixels and R, G, B of (a - b)^2, summed in integers (common.rs:494-511): bit-identical
 *          to the float64 formula.
 *   PSNR = 20 log10(255 / sqrt(MSE)), +inf at MSE 0 (common.rs:513-519).
 *   SSIM (common.rs:521 keeps a 0.0 placeholder; here Wang et al. 2004) per channel on 0..255: 11 x 11 Gaussian window,
 *          sigma 1.5, weights normalised to 1, population statistics, C1 = (0.01 * 255)^2, C2 = (0.03 * 255)^2, averaged over
 *          R, G, B and the (W-10) x (H-10) centres whose window lies inside the frame; within 1e-5 of the float64 definition
 *          on any content, flat and few-valued frames included (the window statistics and their differences are f64).
 *          Needs W >= 11 and H >= 11 (below: NUS_ERR_INVALID_ARGUMENT).
 * Results are deterministic: the same inputs give the same bytes on every run, at every batch position and whatever else was
 * asked in the same call.  A metric that was not asked is NaN. */
typedef enum nus_metric { /* bit mask; PSNR comes with MSE */
    NUS_METRIC_MSE = 1,
    NUS_METRIC_SSIM = 2
} nus_metric;
/* Workspace bytes nus_metrics_compare_device needs for these frames; 0 (and nus_last_error) for an invalid shape or mask. */
size_t nus_metrics_workspace_size(uint32_t w, uint32_t h, uint32_t frames, int what);
/* Enqueue only, allocate nothing: frame i of A at d_a + i*a_stride, of B at d_b + i*b_stride (pointers and strides multiples of
 * 4 bytes, strides >= w*h*4); d_out receives 3 doubles per frame [mse, psnr, ssim] (NaN for what was not asked), ordered on
 * `stream` (a hipStream_t; NULL = the null stream).  d_workspace and d_out 8-byte aligned. */
int nus_metrics_compare_device(const void *d_a, size_t a_stride, const void *d_b, size_t b_stride, uint32_t w, uint32_t h,
                               uint32_t frames, int what, void *d_workspace, size_t workspace_bytes, double *d_out, void *stream);
/* Host buffers (pageable is fine): one pair on `device`; out receives [mse, psnr, ssim].  a_len != b_len: NUS_ERR_SIZE_MISMATCH,
 * "Images must have the same dimensions" (common.rs:486-488); a_len != w*h*4: NUS_ERR_SIZE_MISMATCH.  The bytes travel as
 * nus_upload / nus_download move them, through device buffers the library keeps per device; same results as
 * nus_metrics_compare_device. */
int nus_metrics_compare(int device, const uint8_t *a, size_t a_len, const uint8_t *b, size_t b_len, uint32_t w, uint32_t h,
                        int what, double *out);

/* ---- Block-matching motion estimator (BlockMatchingInterpolator, nu_scaler_core/src/interpolation/mod.rs:513-911) --------
 * The second motion estimator of the reference, for displacements the Horn-Schunck front end cannot follow (up to 24 pixels).
 * Integer work throughout, so vectors, SADs and flags are the same bytes on every run and at every batch position.
 *   Blocks   block_size bs in {8, 16, 32}; blocks_x = ceil(w / bs), blocks_y = ceil(h / bs); block (bx, by) of frame A starts at
 *            (bx bs, by bs).  Block (bx, by) of pair i is entry (i * blocks_y + by) * blocks_x + bx of every per-block output.
 *   Search   (find_best_match :584-622, calculate_sad :555-581) candidates (dx, dy) in [-R, R]^2, R = search_radius in 1 .. 24.  A
 *            candidate is admitted iff the block shifted by it lies wholly inside frame B.  Its SAD is the sum of
 *            |dR| + |dG| + |dB| (alpha ignored, :572-576; so every channel order gives the same result) over the block pixels
 *            that lie inside frame A: partial blocks at the right and bottom edge get vectors.  The admitted candidate with the
 *            smallest SAD wins; with none admitted the vector is (0, 0) and the SAD reads 0xFFFFFFFF.
 *   Ties     NUS_BM_TIES_SCAN is the reference's order (dy outer, dx inner, ascending, first minimum wins): every flat block
 *            gets (-R, -R).  NUS_BM_TIES_CENTER (default) takes the smallest dx^2 + dy^2 first, then scan order: a flat block
 *            stays at (0, 0).
 *   Confidence pass (handle_occlusions :795-910; nus_bm_set_refine, default on).  The pair's motion is smooth iff no block with
 *            bx >= 1 and by >= 1 differs from its left or top neighbour by more than 10 in L1.  If it is not, every interior block
 *            whose L1 differences to its 8 neighbours sum to 35 or more (the reference's 1 / (1 + 0.1 sum / 8) < 0.7, in
 *            integers) is replaced by the direct blend of the two frames -- byte for byte the warp at a zero vector, so the pass
 *            zeroes the block's vector and sets a flag.
 *   Flow     the vectors expanded to [h][w][2], every pixel its block's (dx, dy): the pixel delta from frame A to frame B, the
 *            flow nus_interp_interpolate_device defines (A is sampled at p - t v, B at p + (1 - t) v).  The reference's CPU text
 *            (:738-742) has the opposite sign, which under its own matcher moves content the wrong way: B = A shifted by +s
 *            gives v = +s, and the true mid-frame is A sampled at p - s / 2.
 *   Forward-backward check (nus_bm_set_bidirectional, default off).  BUILD-DEFINED: the reference names it as what its confidence
 *            pass lacks ("bidirectional motion estimation and consistency checks between forward and backward motion vectors",
 *            :798-799).  The search runs one way, so content that exists in one frame only -- background about to be covered or
 *            just uncovered, whatever enters or leaves at the border -- still gets a winner.  With the check on, per pair, at the
 *            handle's block size bs, radius and tie order:
 *              1. F, sadF: the search above (A's blocks in B).  G, sadG: the same search with the frames exchanged (B's blocks in
 *                 A, on the same block grid).
 *              2. A's block (bx, by) with F = (dx, dy) is consistent iff sadF != NUS_BM_NO_MATCH, sadG[cy][cx] != NUS_BM_NO_MATCH and
 *                 |dx + gx| + |dy + gy| <= tolerance, where cx = clamp(bx bs + dx + bs / 2, 0, w - 1) / bs, cy = clamp(by bs + dy +
 *                 bs / 2, 0, h - 1) / bs and (gx, gy) = G[cy][cx]: the block its centre lands in points back at it.  B's block
 *                 (bx, by) is consistent by the same rule with F and G exchanged.
 *              3. V = F where A's block is consistent; else V = -G[by][bx] where B's block at the same grid position is consistent
 *                 (flag bit 2); else the block is unresolved.
 *              4. One pass over step 3's result (so no order matters): an unresolved block takes, for dx and for dy on their own, the
 *                 lower median -- element (n - 1) / 2 of the n values in ascending order -- of that component over those of its up
 *                 to 8 neighbours that step 3 resolved (flag bit 3); with none, the zero vector (flag bit 4).
 *            d_vectors receives V (every component within +-24), d_sad stays the forward SAD, d_flags carries bits 2 - 4.  THE
 *            CONFIDENCE PASS IS NOT RUN AND BITS 0 AND 1 STAY CLEAR, WHATEVER nus_bm_set_refine SAYS: run behind V the pass zeroes
 *            true motion boundaries and takes back most of what the check gains, and on its own it loses to doing nothing as
 *            soon as the background moves, a cross-fade being the wrong fallback for a pan.  PSNR of the t = 0.5 frame against a
 *            rendered true mid-frame, on synthetic pairs of a panning background under a moving square (192 x 128 and 200 x 72,
 *            all presets; DESIGN 8.5 has the table): raw winners 22.6 .. 29.8 dB, confidence pass 19.2 .. 26.6 dB, this check
 *            28.1 .. 32.0 dB, the smallest gains 2.06 dB over the raw winners and 3.74 dB over the pass.  Everything behind the
 *            vectors (flow expansion, nus_bm_warp_device, nus_bm_interpolate, the stream entry point, scene detection) is
 *            unchanged and runs on V.  Cost: the search runs twice; both workspaces grow while the check is on and are their old
 *            sizes with it off, when every entry point writes the bytes it wrote before.  tolerance 0 .. 96 (default
 *            NUS_BM_BIDIR_DEFAULT_TOLERANCE: a SETTING, NOT A MEASUREMENT; 0, 2 and 4 moved the numbers above by under 1 dB).
 * Quality presets (:531-542): High 8 / 24, Medium 16 / 16 (default), Low 32 / 8. */
typedef struct nus_blockmatch nus_blockmatch;
typedef enum nus_bm_tie_order { NUS_BM_TIES_SCAN = 0, NUS_BM_TIES_CENTER = 1 } nus_bm_tie_order;
#define NUS_BM_MAX_RADIUS 24
#define NUS_BM_NO_MATCH 0xFFFFFFFFu
#define NUS_BM_BIDIR_DEFAULT_TOLERANCE 2

nus_blockmatch *nus_bm_create(void); /* never touches the GPU */
void nus_bm_destroy(nus_blockmatch *h);
int nus_bm_set_device(nus_blockmatch *h, int device); /* before the first estimate */
const char *nus_bm_last_error(const nus_blockmatch *h);
int nus_bm_set_params(nus_blockmatch *h, uint32_t block_size, uint32_t search_radius);
int nus_bm_set_quality(nus_blockmatch *h, int quality); /* nus_interp_quality_level */
int nus_bm_set_tie_order(nus_blockmatch *h, int order);
int nus_bm_set_refine(nus_blockmatch *h, int enabled);
/* enabled 0 or 1, tolerance 0 .. 96; anything else: NUS_ERR_INVALID_ARGUMENT before any HIP call.  Workspace sizes asked for before
 * the call no longer hold after it. */
int nus_bm_set_bidirectional(nus_blockmatch *h, int enabled, uint32_t tolerance);
/* Workspace bytes nus_bm_estimate_device needs at the handle's block size; 0 (and the reason in nus_bm_last_error) for an invalid
 * shape. */
size_t nus_bm_workspace_size(nus_blockmatch *h, uint32_t w, uint32_t hgt, uint32_t n_pairs);
/* n_pairs pairs as nus_interp_interpolate_device (same pointers and strides).  Per block: d_vectors 2 x int16 (dx, dy), after the
 * confidence pass (the raw winners with refine off); d_sad (may be NULL) the raw winner's SAD, u32; d_flags (may be NULL) u8, bit 0
 * = the pass zeroed this block, bit 1 = the pair's motion was not smooth (set on every block of the pair alike); with the
 * forward-backward check on, V and bits 2 - 4 as defined above instead.  d_flow (may be
 * NULL): the dense flow, w*h*8 bytes per pair and 8-byte aligned (NUS_FLOW_F32) or w*h*4 and 4-byte aligned (NUS_FLOW_F16; the
 * vectors are integers of magnitude <= 24, exact in f16).  d_workspace 16-byte aligned.  n_pairs == 0: NUS_OK, nothing launched.
 * Enqueue only on `stream`: no allocation, no synchronisation (a handle's first call puts its 163 KiB of rank tables on the
 * device).  Argument errors are NUS_ERR_INVALID_ARGUMENT, returned before any HIP call, with a text that names the entry point. */
int nus_bm_estimate_device(nus_blockmatch *h, const void *d_a, size_t a_stride, const void *d_b, size_t b_stride, uint32_t w,
                           uint32_t hgt, uint32_t n_pairs, void *d_workspace, size_t workspace_bytes, void *d_vectors, void *d_sad,
                           void *d_flags, void *d_flow, int flow_format, void *stream);
/* Host frames in (pageable is fine: the bytes travel as nus_upload / nus_download move them), per-block results out: vectors_out
 * blocks_x * blocks_y * 2 int16; sad_out / flags_out may be NULL.  a_len / b_len != w*h*4: nus_interp_interpolate's
 * NUS_ERR_SIZE_MISMATCH and text. */
int nus_bm_estimate(nus_blockmatch *h, const uint8_t *a, size_t a_len, const uint8_t *b, size_t b_len, uint32_t w, uint32_t hgt,
                    void *vectors_out, uint32_t *sad_out, uint8_t *flags_out);
/* Motion-compensated in-between frames of one host pair: estimate -> dense flow (NUS_FLOW_F16) -> the multi-time warp of
 * nus_interp_interpolate_multi_device in `mode` (nus_interp_mode_t).  Time-set rules as there; n_times frames back to back in out. */
int nus_bm_interpolate(nus_blockmatch *h, const uint8_t *a, size_t a_len, const uint8_t *b, size_t b_len, uint32_t w, uint32_t hgt,
                       const float *times, uint32_t n_times, int mode, uint8_t *out, size_t out_cap);
/* Warp + blend of n_pairs device pairs straight from their per-block vectors: frame (i, k), at d_out + i * out_pair_stride +
 * k * w*hgt*4, is the frame the dense route writes for pair i at times[k] -- the vectors expanded to the flow defined above, then
 * nus_interp_interpolate_multi_device -- without a flow field anywhere.  d_vectors: the layout nus_bm_estimate_device writes, 2 x
 * int16 per block at the handle's block size, blocks_x * blocks_y per pair, 4-byte aligned.  Every component must lie within
 * +-NUS_BM_MAX_RADIUS: the caller's contract, not checked on the device (a breach moves no access out of the frames: every sample
 * position is clamped).  Frames (NUS_FORMAT_RGBA8 only), strides, the time set, `mode` (nus_interp_mode_t) and out_pair_stride (0 =
 * tightly packed; the gap is never written) exactly as nus_interp_interpolate_multi_device.
 *   NUS_INTERP_MODE_EXACT  byte for byte the CPU warp + blend of the expanded vectors, and so byte for byte the dense route.
 *   NUS_INTERP_MODE_FMA    the interpolation path's FMA contract against the CPU warp + blend: no byte off by more than 1, and fewer
 *                          than 0.1 % of the bytes of a frame of at least 328 x 200 differing.  Not promised to be the dense FMA
 *                          route's bytes.
 * Enqueue only on `stream`: no allocation, no synchronisation.  n_pairs == 0: NUS_OK, nothing launched.  Argument errors are
 * NUS_ERR_INVALID_ARGUMENT, returned before any HIP call, with a text that names the entry point. */
int nus_bm_warp_device(nus_blockmatch *h, const void *d_a, size_t a_stride, const void *d_b, size_t b_stride, uint32_t w, uint32_t hgt,
                       uint32_t n_pairs, const void *d_vectors, const float *times, uint32_t n_times, int mode, void *d_out,
                       size_t out_pair_stride, void *stream);
/* Block-matched frame generation over a device-resident stream, no host in the loop: n_frames RGBA8 frames frame_stride bytes apart
 * (a multiple of 4 of at least w*hgt*4; the gaps are never read), pair k = (frame k, frame k + 1), its frames at d_mid +
 * k * mid_pair_stride + j * w*hgt*4 (mid_pair_stride as out_pair_stride above).  One search launch over all pairs, the confidence
 * pass as the handle is set, one launch of nus_bm_warp_device's kernel; with nus_bm_set_scene_detect on, the detector and the cut
 * rule behind it as in nus_bm_interpolate (off: no byte differs).  d_vectors (may be NULL) receives exactly what
 * nus_bm_estimate_device writes.  In NUS_INTERP_MODE_EXACT pair k's frames are byte for byte what nus_bm_interpolate returns for
 * (frame k, frame k + 1) under the same settings, at every batch position and for every batch size; NUS_INTERP_MODE_FMA holds the
 * contract stated at nus_bm_warp_device.  d_workspace: 16-byte aligned, at least nus_bm_stream_workspace_size(h, w, hgt, n_frames)
 * bytes at the handle's current settings -- the search's workspace, the vectors of every pair (used when d_vectors is NULL) and,
 * with detection on, the detector's workspace and flags; 0 (and the reason in nus_bm_last_error) for an invalid shape.  At most
 * 65535 pairs and block rows, as nus_bm_estimate_device.  n_frames < 2: NUS_OK, nothing launched.  Enqueue only; argument errors as
 * above. */
size_t nus_bm_stream_workspace_size(nus_blockmatch *h, uint32_t w, uint32_t hgt, uint32_t n_frames);
int nus_bm_interpolate_multi_device_stream(nus_blockmatch *h, const void *d_frames, size_t frame_stride, uint32_t n_frames, uint32_t w,
                                           uint32_t hgt, const float *times, uint32_t n_times, int mode, void *d_workspace,
                                           size_t workspace_bytes, void *d_vectors, void *d_mid, size_t mid_pair_stride, void *stream);

/* ---- Scene-cut detection and the cut-aware output rule ------------------------------------------------------------
 * BUILD-DEFINED: the reference has no such stage; its GUI interpolates every pair of a stream, the one that straddles a cut
 * included (nu_scaler_py/nu_scaler/main.py:999-1008).  Across a cut there is no motion to estimate, so for a pair flagged
 * here the multi-frame entry points write repeats of the nearer real frame instead of blends.  Everything is opt-in.
 * Per pair (A, B) of frames of one size and channel order, two integer measures:
 *   sad      u64: sum over pixels of |dR| + |dG| + |dB|; alpha ignored.
 *   hist_l1  u32: sum over 32 bins of |H_A[k] - H_B[k]|, H_F the histogram over the frame's pixels of Y >> 3,
 *            Y = (77 R + 150 G + 29 B + 128) >> 8 (the weights sum to 256, so Y <= 255).  0 .. 2 W H.  Luma is not symmetric in
 *            R and B, hence `format` (nus_pixel_format): BGRA gives the numbers of the swizzled RGBA; the X byte is ignored.
 * Decision, in 64-bit integer products (no float compare):
 *   cut  <=>  sad >= mad_threshold * 3 W H   and   hist_l1 * 1000 >= hist_permille * 2 W H
 * mad_threshold 0 .. 255 (default 20), hist_permille 0 .. 1000 (default 400).  Both must hold: the SAD term rejects slow fades
 * (a global +8 step: histogram 270 permille, mean absolute difference 8), the histogram term fast motion (a 24-pixel pan: MAD
 * 19 .. 85, histogram <= 6 permille).  The defaults are SETTINGS, NOT MEASUREMENTS: nobody has run this on real footage.  A global
 * histogram cannot tell two unrelated frames of the same luma distribution apart (two noise frames: MAD 86, 10 permille: no cut).
 * Results are deterministic: the same bytes on every run, at every batch position, whatever the batch size (per-workgroup
 * partials in a workspace, added by a finish kernel; no float, no global atomics). */
typedef struct nus_scene_measures {
    uint64_t sad;
    uint32_t hist_l1;
    uint32_t reserved; /* written as 0 */
} nus_scene_measures;
#define NUS_SCENE_DEFAULT_MAD 20
#define NUS_SCENE_DEFAULT_HIST_PERMILLE 400
/* Workspace bytes nus_scene_detect_device needs; 0 (and nus_last_error) for an invalid shape. */
size_t nus_scene_workspace_size(uint32_t w, uint32_t h, uint32_t n_pairs);
/* n_pairs pairs addressed as nus_interp_interpolate_device addresses them (a sliding stream: d_b = d_a + frame_bytes, both strides
 * frame_bytes; pointers and strides multiples of 4, strides >= w*h*4).  Per pair d_measures (may be NULL; 8-byte aligned) receives
 * a nus_scene_measures and d_cut one u8, 0 or 1.  d_workspace 8-byte aligned.  Enqueue only on `stream`: no allocation, no
 * synchronisation.  n_pairs == 0: NUS_OK, nothing launched.  Argument errors are NUS_ERR_INVALID_ARGUMENT, returned before any HIP
 * call, with a text that names the entry point. */
int nus_scene_detect_device(const void *d_a, size_t a_stride, const void *d_b, size_t b_stride, uint32_t w, uint32_t h, uint32_t n_pairs,
                            int format, uint32_t mad_threshold, uint32_t hist_permille, void *d_workspace, size_t workspace_bytes,
                            nus_scene_measures *d_measures, uint8_t *d_cut, void *stream);
/* One host pair on `device` (pageable is fine: the bytes travel as nus_upload / nus_download move them, through device buffers
 * the library keeps per device); measures_out may be NULL.  Size errors as nus_metrics_compare. */
int nus_scene_detect(int device, const uint8_t *a, size_t a_len, const uint8_t *b, size_t b_len, uint32_t w, uint32_t h, int format,
                     uint32_t mad_threshold, uint32_t hist_permille, nus_scene_measures *measures_out, uint8_t *cut_out);
/* The cut-aware output rule as a pass BEHIND an unchanged multi-time interpolation.  For every pair with d_cut[i] != 0, frame
 * (i, k) at d_out + i * out_pair_stride + k * w*h*4 is overwritten with a copy of A_i if times[k] < 0.5, else of B_i.  "Copy": the
 * bytes the zero-flow nus_interp_interpolate_device writes for that input `format` at t = 0 (A) and t = 1 (B) -- RGBA order out,
 * so a BGRA input is swizzled and the X formats get alpha 255.  Pairs with d_cut[i] == 0 are neither read nor written.  Time-set
 * rules, strides and gaps exactly as nus_interp_interpolate_multi_device; the gap of a display-order stride stays unwritten. */
int nus_scene_apply_cuts_device(const void *d_a, size_t a_stride, const void *d_b, size_t b_stride, uint32_t w, uint32_t h, int format,
                                const float *times, uint32_t n_times, const uint8_t *d_cut, void *d_out, size_t out_pair_stride,
                                uint32_t n_pairs, void *stream);
/* Detection wired into the entry points that write several frames per pair without the host in between: default off (every
 * byte as before).  On, nus_flow_interpolate_multi_device_stream / nus_bm_interpolate run the estimate + warp as before, the
 * detector, and then the apply pass, frames read as NUS_FORMAT_RGBA8.  A flagged pair's estimate and warp are still computed and
 * then overwritten. */
int nus_flow_set_scene_detect(nus_flow *h, int enabled, uint32_t mad_threshold, uint32_t hist_permille);
int nus_bm_set_scene_detect(nus_blockmatch *h, int enabled, uint32_t mad_threshold, uint32_t hist_permille);

/* ---- Frame-rate conversion by a rational ratio (24 -> 60, 25 -> 60, 30 -> 144, 60 -> 24) ------------------------------
 * BUILD-DEFINED: the reference has no rate conversion.  The multi-time entry points give every pair the same time set; in a
 * conversion by num / den = out_rate / in_rate every pair has its own in-between times and some pairs have none.  The entry points
 * below take a device-resident stream and the ratio and write the whole output stream: the kernels evaluate the schedule
 * themselves, per pair, so there is no host in the loop and no table in memory.
 * The schedule.  n_frames >= 2 input frames; 1 <= num, den <= NUS_RETIME_MAX_TERM; the ratio is reduced by its gcd inside the
 * library (60/24 and 5/2 give the same bytes) and the reduced ratio must satisfy num <= (NUS_INTERP_MAX_TIMES + 1) * den.  In 64-bit
 * integers, with the reduced terms:
 *     n_out = ((n_frames - 1) * num) / den + 1
 *     output j = 0 .. n_out - 1:   k_j = (j * den) / num,   r_j = (j * den) % num,   t_j = the float32 nearest to r_j / num
 * t_j is ONE correctly rounded f32 division of the two integers (both exact in f32), on the host and on the device alike.
 *   r_j == 0: output j is real frame k_j -- the bytes the zero-flow nus_interp_interpolate_device writes at t = 0 for the input
 *             format: RGBA order out, alpha 255 for the X formats.  Written by a copy kernel of its own, not by the warp.
 *   r_j != 0: output j is byte for byte what the single-time entry point of the same handle writes for pair (k_j, k_j + 1) at t_j,
 *             in the handle's mode, flow format, input format and projection rounds.
 * k_j never decreases; a pair has at most ceil(num / den) <= 8 outputs; the last output is the last real frame iff den divides
 * (n_frames - 1) * num; with den = 1 the in-between times of every pair are frame_times(num) of the Python package.
 * Output j goes to d_out + j * out_frame_stride: 0 = tightly packed (w*h*4), else a multiple of 4 of at least w*h*4; the gaps are
 * never written.  A pair's vectors are fetched once for all its outputs.
 * Every entry point only enqueues: no allocation beyond a handle's grow-only workspace where its sibling entry point has one, no
 * synchronisation.  Argument errors are NUS_ERR_INVALID_ARGUMENT, returned before any HIP call, with a text that names the entry
 * point: a zero term, a term above the bound, a ratio above 8, n_frames < 2, a bad stride or alignment. */
#define NUS_RETIME_MAX_TERM 4096
typedef struct nus_retime_entry {
    uint32_t pair;     /* k_j */
    uint32_t rem;      /* r_j of the reduced ratio */
    float t;           /* t_j */
    uint32_t reserved; /* written as 0 */
} nus_retime_entry;
/* Host only, no GPU needed.  n_out, or a negative nus_status (and the text in nus_last_error). */
int64_t nus_retime_count(uint32_t n_frames, uint32_t num, uint32_t den);
/* Entries first .. first + count - 1 of the table into out (first + count <= n_out; count 0 writes nothing). */
int nus_retime_schedule(uint32_t n_frames, uint32_t num, uint32_t den, uint64_t first, uint64_t count, nus_retime_entry *out);
/* DIAGNOSTIC: the same table, all n_out entries, written by the device function the kernels use (d_entries 4-byte aligned). */
int nus_retime_schedule_device(uint32_t n_frames, uint32_t num, uint32_t den, void *d_entries, void *stream);
/* n_frames frames frame_stride bytes apart (a multiple of 4 of at least w*h*4); pair k's flow at d_flows + k * w*h*8 (NUS_FLOW_F32;
 * k * w*h*4 with NUS_FLOW_F16), alignment as nus_interp_interpolate_device; d_flows == NULL: zero flow.  One warp launch over all
 * pairs and one copy launch for the real frames. */
int nus_interp_retime_device(nus_interp *h, const void *d_frames, size_t frame_stride, uint32_t n_frames, const void *d_flows,
                             uint32_t w, uint32_t hgt, uint32_t num, uint32_t den, void *d_out, size_t out_frame_stride, void *stream);
/* The estimator, then the retime warp in FMA mode: the bytes of nus_flow_estimate_device_stream followed by nus_interp_retime_device
 * in FMA mode (with the handle's projection rounds), under the handle's warps, median and scene detection, for every chunking of
 * the stream.  Frames tightly packed, pointers aligned as nus_flow_interpolate_multi_device_stream asks; the bytes at d_flows (may
 * be NULL) are the estimate's.  With detection on, a cut pair's in-between outputs are overwritten as
 * nus_scene_apply_cuts_retime_device states. */
int nus_flow_retime_device_stream(nus_flow *h, const void *d_frames, uint32_t n_frames, uint32_t w, uint32_t hgt, uint32_t levels,
                                  uint32_t coarse_iters, uint32_t refine_iters, float lambda, uint32_t num, uint32_t den,
                                  int flow_format, void *d_flows, void *d_out, size_t out_frame_stride, void *stream);
/* Rate conversion with the select warp (nus_interp_interpolate_select_device): nus_interp_retime_device with TWO flows per pair.
 * Pair k's forward plane (frame k -> frame k+1, on frame k's grid) at d_flows_fwd + k * w*h*8 and its backward plane (frame k+1 ->
 * frame k, on frame k+1's grid) at d_flows_bwd + k * w*h*8 (k * w*h*4 with NUS_FLOW_F16); layout and alignment of each as d_flows
 * there.  Output j with r_j == 0 is the real-frame copy, as there; output j with r_j != 0 is byte for byte what
 * nus_interp_interpolate_select_device of the same handle writes for pair (k_j, k_j + 1) at t_j, in the handle's mode, flow format,
 * input format and projection rounds.  Either flow pointer NULL: NUS_ERR_INVALID_ARGUMENT before any HIP call (the select warp takes
 * both flows); every other argument check is nus_interp_retime_device's.  One warp launch over all pairs and one copy launch. */
int nus_interp_retime_select_device(nus_interp *h, const void *d_frames, size_t frame_stride, uint32_t n_frames, const void *d_flows_fwd,
                                    const void *d_flows_bwd, uint32_t w, uint32_t hgt, uint32_t num, uint32_t den, void *d_out,
                                    size_t out_frame_stride, void *stream);
/* Both flows of every pair of a device-resident stream, NUS_FLOW_F32 both, as nus_flow_estimate_device_stream takes and gives its
 * arguments.  d_flows_fwd receives the bytes of nus_flow_estimate_device_stream.  d_flows_bwd receives, per pair k, the flow
 * frame k+1 -> frame k on frame k+1's grid: the backward solve nus_flow_set_bidirectional runs -- the same pyramids, the pair's two
 * planes swapped, the handle's warps and median -- written to the caller's buffer.  In NUS_FLOW_EXACT pair k's backward plane is
 * byte for byte nus_flow_estimate_device(frame k+1, frame k); in NUS_FLOW_FAST it is the plane the setting's select warp reads.
 * Both pointers are required.  It does not look at the handle's bidirectional setting. */
int nus_flow_estimate_both_device_stream(nus_flow *h, const void *d_frames, uint32_t n_frames, uint32_t w, uint32_t hgt, uint32_t levels,
                                         uint32_t coarse_iters, uint32_t refine_iters, float lambda, void *d_flows_fwd, void *d_flows_bwd,
                                         void *stream);
/* nus_flow_retime_device_stream with both flows and the select warp: for every chunking of the stream, in every mode and tiling, the
 * bytes of nus_flow_estimate_both_device_stream followed by nus_interp_retime_select_device in FMA mode (with the handle's projection
 * rounds), under the handle's warps, median and scene detection.  The flows in flow_format between estimator and warp, and at
 * d_flows_fwd / d_flows_bwd where given; either may be NULL, the handle then keeps that direction in its workspace.  Arguments and
 * alignment otherwise as nus_flow_retime_device_stream.  It does not look at the handle's bidirectional setting (which
 * nus_flow_retime_device_stream still refuses).  Workspace: at most 28 bytes per pixel and pair of a chunk more than
 * nus_flow_retime_device_stream reserves for the same call; the result does not depend on what the workspace held before. */
int nus_flow_retime_select_device_stream(nus_flow *h, const void *d_frames, uint32_t n_frames, uint32_t w, uint32_t hgt, uint32_t levels,
                                         uint32_t coarse_iters, uint32_t refine_iters, float lambda, uint32_t num, uint32_t den,
                                         int flow_format, void *d_flows_fwd, void *d_flows_bwd, void *d_out, size_t out_frame_stride,
                                         void *stream);
/* nus_bm_interpolate_multi_device_stream with the schedule in place of the time set: in NUS_INTERP_MODE_EXACT an in-between output is
 * byte for byte nus_bm_interpolate's frame for pair k_j at t_j, a real-frame output the copy.  In either mode the bytes at d_vectors
 * (may be NULL) are nus_bm_estimate_device's for the stream's pairs, and an in-between output is byte for byte what nus_bm_warp_device
 * writes from pair k_j's vectors at t_j in that mode (NUS_INTERP_MODE_FMA: the FMA warp's contract, not nus_bm_interpolate's bytes).
 * d_workspace: 16-byte aligned, at least nus_bm_stream_workspace_size(h, w, hgt, n_frames) bytes. */
int nus_bm_retime_device_stream(nus_blockmatch *h, const void *d_frames, size_t frame_stride, uint32_t n_frames, uint32_t w,
                                uint32_t hgt, uint32_t num, uint32_t den, int mode, void *d_workspace, size_t workspace_bytes,
                                void *d_vectors, void *d_out, size_t out_frame_stride, void *stream);
/* The cut rule behind an unchanged rate conversion: for every pair k with d_cut[k] != 0 (n_frames - 1 flags), each output with
 * k_j == k and r_j != 0 is overwritten with the copy -- as nus_scene_apply_cuts_device defines it for `format` -- of frame k if
 * t_j < 0.5, else of frame k + 1.  Real-frame outputs and the outputs of other pairs are neither read nor written. */
int nus_scene_apply_cuts_retime_device(const void *d_frames, size_t frame_stride, uint32_t n_frames, uint32_t w, uint32_t h, int format,
                                       uint32_t num, uint32_t den, const uint8_t *d_cut, void *d_out, size_t out_frame_stride,
                                       void *stream);

/* ---- YUV 4:2:0 frames: 8-bit planar I420 <-> RGBA8 ------------------------------------------------------------------------
 * BUILD-DEFINED: the reference has no YUV; its frames are RGBA (or BGRA capture surfaces) from end to end.  Decoded video is planar
 * YUV 4:2:0; these entry points are the road between such frames and the RGBA8 frames every other entry point takes.  Two layouts,
 * 8 bits: I420 (here) and NV12 ("NV12 frames" below).  No NV21, no 4:2:2 / 4:4:4, no P010 / 10-bit, no interlace.
 * Frame layout.  An I420 frame of w x h is a Y plane of w*h bytes, then a U plane and a V plane of cw*ch bytes each, cw = (w+1)/2,
 * ch = (h+1)/2, rows tight: w*h + 2*cw*ch bytes (nus_yuv420_frame_bytes).  Frames of a batch are yuv_frame_stride bytes apart (0 =
 * tight, else at least one frame; no alignment rule), RGBA frames rgba_frame_stride bytes apart (0 = tight, else a multiple of 4 of
 * at least w*h*4; the frames 4-byte aligned).  The gaps between frames are never written.
 * The RGBA side is any nus_pixel_format: to-RGBA writes alpha 255 (X formats too), to-YUV ignores the fourth byte.
 * Arithmetic: integers only, so that every byte can be checked for equality.  S = 14, H = 1 << 13; Q(x) = the integer nearest to
 * x * 2^14, computed in double; >> is an arithmetic shift; clamp is to 0 .. 255.
 *   (Kr, Kb) = (0.299, 0.114) for NUS_YUV_MATRIX_BT601, (0.2126, 0.0722) for NUS_YUV_MATRIX_BT709; Kg = 1 - Kr - Kb.
 *   (Ys, Cs, Yo) = (219, 224, 16) for NUS_YUV_RANGE_LIMITED, (255, 255, 0) for NUS_YUV_RANGE_FULL.
 * To YUV.  Yc = Q([Kr, Kg, Kb] Ys/255),  Uc = Q([-Kr, -Kg, 1-Kb] / (2 (1-Kb)) Cs/255),  Vc = Q([1-Kr, -Kg, -Kb] / (2 (1-Kr)) Cs/255).
 *   luma, per pixel:     Y = clamp(((Yc . (R,G,B) + H) >> S) + Yo)
 *   chroma, per chroma cell (cx, cy): (SR, SG, SB) = the integer-weighted sums over the cell's taps, tap coordinates clamped
 *   into the frame, the weights totalling W;   U = clamp(((Uc . (SR,SG,SB) + H W) >> (S + log2 W)) + 128),  V likewise: ONE rounding.
 *     NUS_YUV_SITING_CENTER (Y4M 420jpeg):  taps (2cx+i, 2cy+j), i, j in {0, 1}, weight 1 each, W = 4.
 *     NUS_YUV_SITING_LEFT (Y4M 420mpeg2):   columns 2cx-1, 2cx, 2cx+1 with weights 1, 2, 1 in rows 2cy and 2cy+1, W = 8.
 *   to-YUV always filters by the siting; chroma_filter is not looked at.
 * To RGBA.  cy = Q(255/Ys),  rv = Q(2 (1-Kr) 255/Cs),  bu = Q(2 (1-Kb) 255/Cs),  gu = Q(-2 Kb (1-Kb)/Kg 255/Cs),
 *   gv = Q(-2 Kr (1-Kr)/Kg 255/Cs).
 *   NUS_YUV_CHROMA_NEAREST:  u = U[y>>1][x>>1] - 128, v likewise;
 *     R = clamp((cy (Y-Yo) + rv v + H) >> S),  G = clamp((cy (Y-Yo) + gu u + gv v + H) >> S),  B = clamp((cy (Y-Yo) + bu u + H) >> S)
 *   NUS_YUV_CHROMA_BILINEAR: u16 = the chroma summed with integer weights totalling 16, minus 16 * 128; chroma coordinates clamped.
 *     vertical, both sitings: luma row y even: chroma rows cy-1 (weight 1) and cy (3); y odd: rows cy (3) and cy+1 (1), cy = y>>1.
 *     horizontal, CENTER: the same rule in x.  LEFT: x even: column cx (4); x odd: columns cx (2) and cx+1 (2), cx = x>>1.
 *     R = clamp((16 cy (Y-Yo) + rv v16 + 16 H) >> (S+4)), G and B likewise: ONE rounding.
 *   Every intermediate fits int32 (the largest is about 1.4e8).
 * Against the same taps evaluated with the real-valued coefficients in double and rounded once, a byte differs by at most 1, and
 * fewer than 1 % of the bytes differ (tests/test_yuv_contract.py; DESIGN.md 8.8 has the shares).
 * The *_device entry points only enqueue on `stream`: no allocation, no synchronisation.  Argument errors are
 * NUS_ERR_INVALID_ARGUMENT (sizes of the host entry points: NUS_ERR_SIZE_MISMATCH), returned before any HIP call, with a text
 * that names the entry point: a null pointer, a zero or too large dimension, an unknown enum value, n_frames == 0, a bad stride. */
typedef enum nus_yuv_matrix {
    NUS_YUV_MATRIX_BT601 = 0,
    NUS_YUV_MATRIX_BT709 = 1
} nus_yuv_matrix;
typedef enum nus_yuv_range {
    NUS_YUV_RANGE_LIMITED = 0,
    NUS_YUV_RANGE_FULL = 1
} nus_yuv_range;
typedef enum nus_yuv_siting {
    NUS_YUV_SITING_CENTER = 0,
    NUS_YUV_SITING_LEFT = 1
} nus_yuv_siting;
typedef enum nus_yuv_chroma_filter {
    NUS_YUV_CHROMA_NEAREST = 0,
    NUS_YUV_CHROMA_BILINEAR = 1
} nus_yuv_chroma_filter;
typedef struct nus_yuv_format {
    int matrix;        /* nus_yuv_matrix */
    int range;         /* nus_yuv_range */
    int siting;        /* nus_yuv_siting */
    int chroma_filter; /* nus_yuv_chroma_filter: to-RGBA only */
} nus_yuv_format;
/* Host only.  Bytes of one I420 frame; 0 (and nus_last_error) for bad dimensions: zero, more than 2^30 pixels, higher than 524280. */
size_t nus_yuv420_frame_bytes(uint32_t w, uint32_t h);
/* DIAGNOSTIC, host only: the tables the kernels use.  to_yuv[9] = Yc, Uc, Vc over (R, G, B); to_rgb[5] = cy, rv, bu, gu, gv. */
int nus_yuv_coefficients(int matrix, int range, int32_t *to_yuv, int32_t *to_rgb);
int nus_yuv420_to_rgba8_device(const void *d_yuv, size_t yuv_frame_stride, uint32_t w, uint32_t h, const nus_yuv_format *fmt,
                               int rgba_format, void *d_rgba, size_t rgba_frame_stride, uint32_t n_frames, void *stream);
int nus_rgba8_to_yuv420_device(const void *d_rgba, size_t rgba_frame_stride, uint32_t w, uint32_t h, const nus_yuv_format *fmt,
                               int rgba_format, void *d_yuv, size_t yuv_frame_stride, uint32_t n_frames, void *stream);
/* One host frame on `device` (pageable is fine: the bytes travel as nus_upload / nus_download move them, through device buffers the
 * library keeps per device).  yuv_len / rgba_len must be the frame's size exactly; the capacity at least the other frame's. */
int nus_yuv420_to_rgba8(int device, const uint8_t *yuv, size_t yuv_len, uint32_t w, uint32_t h, const nus_yuv_format *fmt,
                        int rgba_format, uint8_t *rgba, size_t rgba_cap);
int nus_rgba8_to_yuv420(int device, const uint8_t *rgba, size_t rgba_len, uint32_t w, uint32_t h, const nus_yuv_format *fmt,
                        int rgba_format, uint8_t *yuv, size_t yuv_cap);

/* ---- Up-scaling I420 frames plane by plane ----------------------------------------------------------------------------------
 * BUILD-DEFINED: the reference has no YUV.  Y, U and V of an I420 frame (layout: nus_yuv420_frame_bytes) are resampled as three
 * single-channel 8-bit images, with no colour conversion on the way: luma becomes the filter of the luma, and chroma is resampled
 * once, at the position its siting gives it.
 * Dimension rule.  iw, ih, ow, oh are all even, ow >= iw and oh >= ih: the chroma planes are then exactly half the luma planes
 * on both sides and the chroma ratio is the luma ratio.  Odd dimensions and down-scaling on an axis are NUS_ERR_UNSUPPORTED (the
 * RGBA route, nus_upscaler, takes them).  Equal sizes on both axes: the frame is copied.
 * Arithmetic.  Each plane goes through image-0.24.9 imageops::resize as the NUS_ALG_LANCZOS3 / _BICUBIC / _TRIANGLE up-scalers
 * do it per channel: a vertical pass into f32 (taps ascending), a horizontal pass (taps ascending), clamp to 0 .. 255, round to
 * nearest.  NUS_LANCZOS_EXACT: separate multiplies and adds, ties away from zero -- every plane equals the crate's resize of that
 * plane, bit for bit, under centre siting.  NUS_LANCZOS_FMA: fused, ties to even; each sample is the nearest integer to the
 * float64 resample of the same f32 weights, except within the accumulation error of a rounding tie.
 * Geometry.  A sample of index i sits at i + phi in continuous coordinates, on both sides of an axis.  phi = 0.5 for luma, for
 * chroma vertically, and for chroma horizontally under NUS_YUV_SITING_CENTER; phi = 0.25 for chroma horizontally under
 * NUS_YUV_SITING_LEFT (chroma co-sited with the even luma column).  Per output o of an axis in_n -> out_n, in f32, each operation
 * rounded on its own:  ratio = in_n / out_n;  sratio = max(ratio, 1);  centre = (o + phi) * ratio, and if phi != 0.5
 * centre = centre + (0.5 - phi);  left = clamp(floor(centre - support * sratio), 0, in_n - 1);  right = clamp(ceil(centre +
 * support * sratio), left + 1, in_n);  centre = centre - 0.5;  w_i = kernel((left + i - centre) / sratio) for i < right - left,
 * divided by their sum.  With phi = 0.5 these are nus_resize_build_axis' tables bit for bit.
 * A handle holds the four axis tables (luma x / y, chroma x / y; U and V share theirs); they are built on the host by
 * nus_yuv_resizer_initialize and uploaded by the handle's first device call, which therefore also allocates and synchronises;
 * later calls of nus_yuv420_resize_device only enqueue.  One call at a time per handle.
 * Errors: a null pointer, a zero or too large dimension, an unknown siting or mode, n_frames == 0 and a stride below the frame are
 * NUS_ERR_INVALID_ARGUMENT; a call before initialize NUS_ERR_NOT_INITIALIZED; the host entry point's sizes NUS_ERR_SIZE_MISMATCH;
 * all returned before any HIP call, with a text that begins with the entry point's name. */
typedef struct nus_yuv_resizer nus_yuv_resizer;
nus_yuv_resizer *nus_yuv_resizer_create(void);                       /* never touches the GPU */
void nus_yuv_resizer_destroy(nus_yuv_resizer *h);
const char *nus_yuv_resizer_last_error(const nus_yuv_resizer *h);
int nus_yuv_resizer_set_device(nus_yuv_resizer *h, int device);     /* before the first device call */
/* algorithm: NUS_ALG_LANCZOS3 | NUS_ALG_BICUBIC | NUS_ALG_TRIANGLE (others: NUS_ERR_UNSUPPORTED); siting: nus_yuv_siting;
 * mode: nus_lanczos_mode.  Builds the four axis tables on the host; no HIP call. */
int nus_yuv_resizer_initialize(nus_yuv_resizer *h, uint32_t iw, uint32_t ih, uint32_t ow, uint32_t oh, int algorithm, int siting, int mode);
/* DIAGNOSTIC, host only: plane 0 luma / 1 chroma, axis 0 x / 1 y; left[out_n], ntaps[out_n], weights[out_n * NUS_RESIZE_MAX_TAPS]. */
int nus_yuv_resizer_export_axis(const nus_yuv_resizer *h, int plane, int axis, int32_t *left, uint32_t *ntaps, float *weights);
/* I420 frames as nus_yuv420_frame_bytes lays them out; frame i at base + i * stride (0 = tight; gaps never read or written).
 * Enqueue only on `stream`; the handle's first device call uploads its tables. */
int nus_yuv420_resize_device(nus_yuv_resizer *h, const void *d_in, size_t in_frame_stride, void *d_out, size_t out_frame_stride,
                             uint32_t n_frames, void *stream);
int nus_yuv420_resize(nus_yuv_resizer *h, const uint8_t *in, size_t in_len, uint8_t *out, size_t out_cap);   /* one host frame */

/* ---- NV12 frames: conversions, the repack from and to I420, and the planar up-scaler ------------------------------------------
 * BUILD-DEFINED: the reference has no YUV.  NV12 is what hardware decoders and `-pix_fmt nv12` hand over: a Y plane and ONE plane
 * of interleaved U,V byte pairs, usually with a row pitch wider than the picture.  The arithmetic is the I420 contract's above:
 * an NV12 result is by definition the I420 result with the chroma bytes in another place, every byte of it.
 * Layout.  With cw = (w+1)/2 and ch = (h+1)/2:
 *   tight (layout == NULL, or pitch 0, which requires uv_offset 0): Y rows w bytes apart; the UV plane starts at w*h, its rows
 *     2*cw bytes apart; cell (cx, cy) is U at byte 2cx and V at byte 2cx+1 of row cy; frame bytes = nus_yuv420_frame_bytes(w, h).
 *   pitched (pitch != 0): pitch >= 2*cw; the rows of both planes are `pitch` apart; uv_offset is 0 (meaning pitch*h) or at least
 *     pitch*h; frame bytes = the effective uv_offset + pitch*ch.
 * Frames of a batch are nv12_frame_stride bytes apart (0 = the frame bytes, else at least that).  There is no alignment rule on
 * the NV12 side; the RGBA side is as above.  Row padding, the gap between the planes and the gaps between frames are never
 * written.  Dimension limits and error conventions are those of the I420 entry points: NUS_ERR_INVALID_ARGUMENT (sizes of the host
 * entry points: NUS_ERR_SIZE_MISMATCH) before any HIP call, with a text that begins with the entry point's name; a bad layout is
 * an invalid argument.  The *_device entry points only enqueue on `stream`.
 * Conversions.  All 16 (matrix, range, siting, chroma_filter) forms and the four RGBA formats: nus_rgba8_to_nv12* writes what
 * nus_rgba8_to_yuv420* writes with U and V interleaved; nus_nv12_to_rgba8* writes what nus_yuv420_to_rgba8* writes for the
 * de-interleaved frame.  nus_yuv420_to_nv12_device / nus_nv12_to_yuv420_device move bytes only (I420 frames tight, i420_frame_stride
 * apart, 0 = tight).  The host entry points take one tight frame, as nus_yuv420_to_rgba8 does.
 * Up-scaling.  nus_nv12_resize[_device] use the nus_yuv_resizer handle, its initialize and its four axis tables as they are (U and
 * V share theirs): the output is nus_yuv420_resize_device's output rearranged, bit for bit, in both modes.  Frames are TIGHT NV12 on
 * both sides; pitched surfaces go through the conversions or the repack.  Equal sizes copy.
 * Not here: NV21, P010 / 10-bit, 4:2:2 / 4:4:4, a pitched resize, NV12 in the `video` command (Y4M has no tag for it), the native
 * command-line tool. */
typedef struct nus_nv12_layout {
    size_t pitch;     /* bytes between rows, of the Y plane and of the UV plane alike; 0 = tight */
    size_t uv_offset; /* bytes from the frame's base to its UV plane; 0 = directly behind the Y rows */
} nus_nv12_layout;
/* Host only.  Bytes of one NV12 frame; 0 (and nus_last_error) for bad dimensions or a bad layout. */
size_t nus_nv12_frame_bytes(uint32_t w, uint32_t h, const nus_nv12_layout *layout);
int nus_nv12_to_rgba8_device(const void *d_nv12, const nus_nv12_layout *layout, size_t nv12_frame_stride, uint32_t w, uint32_t h,
                             const nus_yuv_format *fmt, int rgba_format, void *d_rgba, size_t rgba_frame_stride, uint32_t n_frames,
                             void *stream);
int nus_rgba8_to_nv12_device(const void *d_rgba, size_t rgba_frame_stride, uint32_t w, uint32_t h, const nus_yuv_format *fmt,
                             int rgba_format, void *d_nv12, const nus_nv12_layout *layout, size_t nv12_frame_stride, uint32_t n_frames,
                             void *stream);
int nus_nv12_to_rgba8(int device, const uint8_t *nv12, size_t nv12_len, uint32_t w, uint32_t h, const nus_yuv_format *fmt,
                      int rgba_format, uint8_t *rgba, size_t rgba_cap);
int nus_rgba8_to_nv12(int device, const uint8_t *rgba, size_t rgba_len, uint32_t w, uint32_t h, const nus_yuv_format *fmt,
                      int rgba_format, uint8_t *nv12, size_t nv12_cap);
int nus_yuv420_to_nv12_device(const void *d_i420, size_t i420_frame_stride, uint32_t w, uint32_t h, void *d_nv12,
                              const nus_nv12_layout *layout, size_t nv12_frame_stride, uint32_t n_frames, void *stream);
int nus_nv12_to_yuv420_device(const void *d_nv12, const nus_nv12_layout *layout, size_t nv12_frame_stride, uint32_t w, uint32_t h,
                              void *d_i420, size_t i420_frame_stride, uint32_t n_frames, void *stream);
int nus_nv12_resize_device(nus_yuv_resizer *h, const void *d_in, size_t in_frame_stride, void *d_out, size_t out_frame_stride,
                           uint32_t n_frames, void *stream);
int nus_nv12_resize(nus_yuv_resizer *h, const uint8_t *in, size_t in_len, uint8_t *out, size_t out_cap);   /* one tight host frame */

#ifdef __cplusplus
}
#endif
#endif /* NUSCALER_HIP_H */
