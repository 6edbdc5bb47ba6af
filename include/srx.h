/*
 * srx.h -- C ABI of libsrx.so, the MI355X (gfx950) multi-frame super-resolution core.
 *
 * Drop-in boundary.  The reference (benedikthoward/ENPH459-Super-Resolution) has no FFI:
 * its boundary is the set of module-level Python functions each run_sr.py driver calls
 * (mono_cal_target/run_sr.py:157-209; identical copies in rgb_cal_target :171-223,
 * mono_barcodes :188-242, rgb_barcodes :201-255).  Every entry point below replaces one
 * of those functions (or one of the two SciPy calls the drivers make directly) and says
 * which.  The Python shim `sr_mi355x` (enph459-super-resolution_amd/sr_mi355x/api.py)
 * binds these with ctypes and re-exposes the reference's names and signatures.
 *
 * Conventions
 *   - Plain C ABI: pointers + sizes, no C++/torch types.  Suffix _f32 / _f64 = element
 *     type T of every image buffer (float / double).  The reference computes in float64;
 *     _f64 reproduces it to ~1e-10 DN, _f32 (HBM-bound fast path) to ~2e-4 DN.
 *   - Image buffers are DEVICE pointers (HBM), C-contiguous, row-major [row(y), col(x)],
 *     single channel, with a leading batch count B (B independent work items: patches,
 *     sessions x reps).  B = 1 reproduces the reference's single-image call.
 *   - Small parameter arrays (PSF kernel, shift table) are HOST pointers, float64:
 *     `kernel` [kh, kw] row-major, `shifts_yx` [N, 2] = (dy, dx) in LR pixels, positive =
 *     content moves toward +index -- exactly the reference's `shift_yx`/`shifts_yx`.
 *     They are shared by all B items of a call (the *_items_* entry points take one table per item).
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream).  All work is
 *     enqueued on it; nothing synchronises the device.  No allocation happens inside a
 *     call: scratch comes from the caller's workspace (`*_workspace_bytes`, 256-B aligned
 *     device memory).  Inputs are never written; outputs never alias inputs unless stated.
 *   - Memory contract (tests/test_gpu_memory_contract.py holds every entry point to it): a call
 *     writes its outputs and bytes [0, ws_bytes) of its workspace, nothing else.  The workspace
 *     may hold anything on entry (it is never assumed zero) and nothing is kept in it between
 *     calls (plans excepted).  ws_bytes is checked on the host against the call's documented
 *     size -- its `*_workspace_bytes` at the call's own arguments, srx_ibp_workspace_bytes_for
 *     for srx_ibp -- and the pointer against the 256-byte grid: a shorter or misaligned
 *     workspace is SRX_E_WORKSPACE before anything is queued, whether or not the path the call
 *     takes would have carved less.  Image, output and errors pointers need only the alignment
 *     of their element type (a frame sliced out of a batch of odd-sized frames is fine): no
 *     kernel casts a caller pointer to a vector type at an address it has not aligned itself (srx_psf_estimate
 *     peels a scalar head and tail around its 16-byte reads of the frames, srx_register_u8's coarse kernel reads aligned words inside the
 *     stack and single bytes at its ends), and otherwise only arena planes are
 *     moved as aligned 16-byte vectors.  One kernel does reach caller memory with 128-bit BUFFER accesses at
 *     addresses that are then only 4-byte aligned (k_ibp_patch parks its state in hr_out, 16 bytes
 *     per lane): that is legal because the HIP runtime runs gfx9 devices in unaligned-access mode
 *     (SH_MEM_CONFIG.ALIGNMENT_MODE: multi-dword accesses need dword alignment), which is what
 *     this guarantee rests on for that kernel; the element-aligned cases of the memory-contract
 *     tests are its check on a given installation.
 *   - Streams and graphs: a call only queues kernels and device-to-device copies on `stream`
 *     (every fill is a kernel, the host arrays are read before the call returns and travel as
 *     kernel arguments or are expanded on the device), so it may be captured into a HIP graph
 *     (hipStreamBeginCapture on `stream`) and replayed on new frames at the same addresses;
 *     which implementation runs is decided from shapes, shifts and PSF, never from the samples
 *     (what depends on them -- 8-bit operand packing, count masks -- is decided on the device).
 *     tests/test_gpu_graph.py replays every implementation on new frames, bit for bit, with
 *     DEBUG_CLR_GRAPH_PACKET_CAPTURE=0: under ROCm 7.2's default graph path replays of short
 *     chains were intermittently wrong from the second launch on (profiles/README.md), so check
 *     before relying on it -- and replaying buys no time here (0.75x ... 1.02x of plain calls).
 *     srx_profile_enable(1) records HIP events and should stay off during a capture.
 *   - Return value: SRX_OK (0) or a negative srx_status; srx_strerror() names it.  Like the
 *     reference's core, shape mismatches that the reference handles by crop/pad
 *     (run_sr.py:172-175, :199-201) are handled the same way, not reported.
 */
#ifndef SRX_H
#define SRX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void *srx_stream_t;

typedef enum {
    SRX_OK = 0,
    SRX_E_INVALID = -1,     /* null pointer, non-positive size, bad factor */
    SRX_E_UNSUPPORTED = -2, /* kernel larger than SRX_MAX_KERNEL_TAPS, N > SRX_MAX_FRAMES, or one image plane (with its 12-sample pad) /
                               one item's N frames of 2 GiB or more: planes are indexed with 32-bit offsets; the batch count is not limited */
    SRX_E_WORKSPACE = -3,   /* workspace pointer null, not 256-byte aligned, or smaller than *_workspace_bytes() */
    SRX_E_HIP = -4          /* a HIP runtime call or kernel launch failed */
} srx_status;

#define SRX_MAX_KERNEL_TAPS 225 /* kh * kw <= 15 x 15 */
#define SRX_MAX_FRAMES 32       /* N per work item */

/* srx_ibp / srx_saa `flags` */
#define SRX_FLAG_AUTO 0u     /* fused tile kernels when eligible, composed primitives otherwise */
#define SRX_FLAG_COMPOSED 1u /* force the literal per-frame composition of the primitives */
#define SRX_FLAG_FUSED 2u    /* require a fused path; SRX_E_UNSUPPORTED if not eligible */
#define SRX_FLAG_PER_FRAME 4u /* fused, but never the "mosaic" (common-fraction, depth-to-space) formulation */
#define SRX_FLAG_TILES 8u     /* the tile kernels only: none of the register-resident kernels (the patch-resident one, the one-launch frame
                               * kernels of the mosaic formulation, the window kernels of the per-frame formulation) */
/* Diagnostic path switches: each selects between implementations that the tests hold to the same results.  They are call
 * arguments (no environment variable alters what a call computes). */
#define SRX_FLAG_DIAG_NO_ZERO_FUSE 0x100u      /* delta = 0: separate blur and index-map kernels */
#define SRX_FLAG_DIAG_NO_SEPARABLE 0x200u      /* 7x7 form of a rank-1 PSF */
#define SRX_FLAG_DIAG_NO_PREFILTER_TILE 0x400u /* line prefilter kernels for float planes */
#define SRX_FLAG_DIAG_WIDE_WINDOWS 0x1000u     /* delta != 0 frames: 256-column windows whatever the plan's cost model says */
#define SRX_FLAG_DIAG_COLUMN_TILES 0x2000u    /* delta = 0 frames in float32: the transpose-free kernel (float64's default) instead of k_ibp_ztile */
#define SRX_FLAG_DIAG_TWO_LAUNCH 0x4000u     /* common-fraction frames: the two-launch window kernels (srx_atile.hpp) also where k_ibp_dtile would run */
#define SRX_FLAG_DIAG_V1 0x800u                /* per-frame fused path with stand-alone prefilter passes: 8 queued operations / iteration -- 8 kernel
                                                * launches where the two prefilters are a row and a column kernel each (float64; float32 planes below
                                                * 64 x 64 or under SRX_FLAG_DIAG_NO_PREFILTER_TILE), 6 kernel launches and 2 device-to-device copies
                                                * where each is the tile kernel and the copy back from its scratch plane (float32 otherwise) */
#define SRX_FLAG_DIAG_SAA_ONE_PASS 0x8000u   /* shift_and_add on a common fraction: the one-kernel form (accumulation over the frames with the
                                              * fractional shift's halo) instead of accumulate + shift (k_saa_tile<ACC> + k_saa_shift); same bits */
#define SRX_FLAG_DIAG_U8_BYTE_LOADS 0x10000u /* srx_ibp_u8lr_f32, "patch" on a full phase grid: k_patch_build reads the frames one byte per lane also
                                              * where they start on a 4-byte boundary (default there: whole LR rows as 4-byte words); same bits */

int srx_version(void);
const char *srx_strerror(int status);
/* Name of the code path the last srx_ibp_* / srx_saa_* call on this thread took:
 * "patch" (mosaic formulation, a whole 256x256 HR patch per workgroup, all iterations in one launch; any 7x7 PSF), "ztile" (mosaic
 * formulation at integer HR shifts on frames of at least 128x128: one launch per iteration on register-resident tiles),
 * "ctile" (the same in float64, rank-1 PSF), "stile" (float64, a common fraction > 0, 256x256 HR patches: two launches per iteration on
 * register-resident strips that span the patch in the direction their operators run), "dtile" (a common fraction > 0 on frames of at least 256x256: one launch per iteration on
 * overlapping windows), "atile" (the same frames at other sizes: three launches per iteration -- forward windows, the near band, backward windows -- on 128x128 windows), "mosaic" (all shifts share
 * one sub-pixel fraction: dense depth-to-space formulation, tile kernels), "btile"
 * (per-frame fractional shifts at x2, float32, any 7x7 PSF: two launches per iteration on register-resident windows), "fused"
 * (per-frame tile kernels), "composed" (primitives, frame by frame). */
const char *srx_last_path(void);

/* ---- measurement hook (no reference counterpart; used by bench.py's roofline leg) ----
 * While enabled, every launch of the fused-path kernels is bracketed by HIP events recorded on the
 * launch stream.  srx_profile_get() waits for them and returns the summed duration and the launch
 * count of kernel `id` (0 <= id < srx_profile_kernel_count()).  srx_profile_enable() clears the log. */
void srx_profile_enable(int on);
int srx_profile_kernel_count(void);
const char *srx_profile_kernel_name(int id);
int srx_profile_get(int id, double *total_ms, long *launches);

/* ---- blur(img, kernel): run_sr.py:157-158, fftconvolve(img, kernel, mode='same') ----
 * zero-padded true convolution, centred crop at (k-1)//2.  img/out [B, H, W]. */
int srx_blur_f32(const float *img, int B, int H, int W, const double *kernel, int kh, int kw, float *out,
                 srx_stream_t stream);
int srx_blur_f64(const double *img, int B, int H, int W, const double *kernel, int kh, int kw, double *out,
                 srx_stream_t stream);

/* ---- scipy.ndimage.shift(in, (sy, sx), order=3, mode='nearest'): call sites run_sr.py:163-164,
 * :176-177, :186.  sy/sx in pixels of `in`; out[i] = in[i - s].  in/out [B, H, W]. */
size_t srx_shift_workspace_bytes(int elem_bytes, int B, int H, int W);
int srx_shift_cubic_f32(const float *in, int B, int H, int W, double sy, double sx, float *out, void *ws,
                        size_t ws_bytes, srx_stream_t stream);
int srx_shift_cubic_f64(const double *in, int B, int H, int W, double sy, double sx, double *out, void *ws,
                        size_t ws_bytes, srx_stream_t stream);

/* ---- scipy.ndimage.zoom(in, factor, order=3): call sites run_sr.py:185, :279 (Native-2x).
 * in [B, h, w] -> out [B, h*factor, w*factor]. */
size_t srx_zoom_workspace_bytes(int elem_bytes, int B, int h, int w, int factor);
int srx_zoom_cubic_f32(const float *in, int B, int h, int w, int factor, float *out, void *ws, size_t ws_bytes,
                       srx_stream_t stream);
int srx_zoom_cubic_f64(const double *in, int B, int h, int w, int factor, double *out, void *ws, size_t ws_bytes,
                       srx_stream_t stream);

/* ---- forward_model(hr, kernel, shift_yx, factor): run_sr.py:161-165.
 * hr [B, H, W] -> out [B, ceil(H/f), ceil(W/f)]. */
size_t srx_forward_workspace_bytes(int elem_bytes, int B, int H, int W);
int srx_forward_f32(const float *hr, int B, int H, int W, const double *kernel, int kh, int kw, double sy, double sx,
                    int factor, float *out, void *ws, size_t ws_bytes, srx_stream_t stream);
int srx_forward_f64(const double *hr, int B, int H, int W, const double *kernel, int kh, int kw, double sy, double sx,
                    int factor, double *out, void *ws, size_t ws_bytes, srx_stream_t stream);

/* ---- back_project(error_lr, kernel, shift_yx, factor, hr_shape): run_sr.py:168-178.
 * err [B, eh, ew] -> out [B, H, W] (zero-insert at [::f, ::f], pad/crop to (H, W)). */
size_t srx_backproject_workspace_bytes(int elem_bytes, int B, int H, int W);
int srx_backproject_f32(const float *err, int B, int eh, int ew, const double *kernel, int kh, int kw, double sy,
                        double sx, int factor, int H, int W, float *out, void *ws, size_t ws_bytes,
                        srx_stream_t stream);
int srx_backproject_f64(const double *err, int B, int eh, int ew, const double *kernel, int kh, int kw, double sy,
                        double sx, int factor, int H, int W, double *out, void *ws, size_t ws_bytes,
                        srx_stream_t stream);

/* ---- shift_and_add(lr_list, shifts_yx, factor, order=3): run_sr.py:181-187.
 * lr [B, N, h, w] -> out [B, h*f, w*f]. */
size_t srx_saa_workspace_bytes(int elem_bytes, int B, int N, int h, int w, int factor);
/* The name srx_last_path() reports after an srx_saa call with these arguments: "mosaic", "fused" or "composed" ("none" for arguments the
 * call refuses, SRX_FLAG_FUSED on a table that cannot fuse included).  Decided from shape, shifts and flags on the host: no device,
 * nothing queued. */
const char *srx_saa_path_for(int elem_bytes, int N, int h, int w, int factor, const double *shifts_yx, unsigned flags);
int srx_saa_f32(const float *lr, int B, int N, int h, int w, const double *shifts_yx, int factor, float *out,
                void *ws, size_t ws_bytes, srx_stream_t stream, unsigned flags);
int srx_saa_f64(const double *lr, int B, int N, int h, int w, const double *shifts_yx, int factor, double *out,
                void *ws, size_t ws_bytes, srx_stream_t stream, unsigned flags);

/* ---- ibp(lr_list, shifts_yx, kernel, hr_init, factor, n_iter, step): run_sr.py:190-209.
 * lr [B, N, h, w], hr_init/hr_out [B, H, W] (hr_out may alias hr_init), errors_out device
 * float64 [B, n_iter] = the reference's `errors` list per item (mean over frames of the mean
 * squared LR residual BEFORE that iteration's update); may be NULL to skip it. */
size_t srx_ibp_workspace_bytes(int elem_bytes, int B, int N, int h, int w, int H, int W, int factor, unsigned flags);
/* The same with the call's shift table and PSF at hand: exactly what that call will carve (<= the bound above, which must cover
 * every implementation the shape admits). */
size_t srx_ibp_workspace_bytes_for(int elem_bytes, int B, int N, int h, int w, int H, int W, int factor, const double *shifts_yx,
                                   const double *kernel, int kh, int kw, unsigned flags);
/* The name srx_last_path() reports after an srx_ibp call with these arguments ("none" for arguments the call refuses): the route
 * is decided from shapes, shifts, PSF and flags on the host, so this needs no device and queues nothing. */
const char *srx_ibp_path_for(int elem_bytes, int N, int h, int w, int H, int W, int factor, const double *shifts_yx, const double *kernel,
                             int kh, int kw, unsigned flags);
/* The form of the far-field residual step that the "patch" implementation takes on a table of shifts, decided on the host like the
 * route: 2 a full phase grid whose 0/1 count masks are all ones where the step's result is used (no mask test), 1 a phase grid with empty
 * rows or columns (masks tested), 0 a count plane (frames sharing a phase, or no product grid), -1 shifts without a common sub-pixel
 * fraction per axis or arguments out of range.  Needs no device. */
int srx_ibp_patch_gstep_for(int N, int factor, const double *shifts_yx);
int srx_ibp_f32(const float *lr, int B, int N, int h, int w, const double *shifts_yx, const double *kernel, int kh,
                int kw, const float *hr_init, int H, int W, int factor, int n_iter, double step, float *hr_out,
                double *errors_out, void *ws, size_t ws_bytes, srx_stream_t stream, unsigned flags);
int srx_ibp_f64(const double *lr, int B, int N, int h, int w, const double *shifts_yx, const double *kernel, int kh,
                int kw, const double *hr_init, int H, int W, int factor, int n_iter, double step, double *hr_out,
                double *errors_out, void *ws, size_t ws_bytes, srx_stream_t stream, unsigned flags);

/* ---- shift_and_add / ibp on the camera's own samples: load_gray's uint8 frames (run_sr.py:73-75) without the astype(float64) ----
 * The reference decodes 8-bit PNGs and converts them to float64 before anything else; these entry points take the bytes.  lr is
 * uint8 [B, N, h, w]; _f32 / _f64 is the type of the state, the output and the arithmetic, as everywhere else.  (T)uint8 is exact, so a
 * call returns the same bits as srx_saa_* / srx_ibp_* on the converted frames.  Everything else is the float call's: argument checks and
 * limits (the 2 GiB rule counts the frames as T), flags, chunking of large batches, srx_last_path(), the MSE trace, hr_out == hr_init;
 * the route is the float call's too (srx_ibp_path_for / srx_saa_path_for with elem_bytes = sizeof(T) answer for both).  lr needs byte alignment only (a
 * frame of odd h w starts on an odd byte).
 *   mosaic family ("patch", "stile", "ctile", "ztile", "dtile", "atile", "mosaic", and shift_and_add's "mosaic"): the kernels that build
 *     the tables read the bytes themselves; no converted copy exists anywhere.  shift_and_add converts frames larger than 64 x 64 into a
 *     plane the float call carves as well.
 *   "btile", "fused", "composed": the frames of a chunk are converted to T at the front of the workspace and the float driver runs on the
 *     rest.  These routes serve per-frame fractional shifts -- in the reference those belong to rep-averaged, hence non-integer, frames
 *     (rgb_cal_target), so no real uint8 workload reaches them; they are there so that the entry points accept every shift table.
 * Workspace: srx_ibp_u8lr_workspace_bytes_for = srx_ibp_workspace_bytes_for on a mosaic-family route, and that plus
 * align_up(min(B, 32768) N h w sizeof(T)) (256-byte granules) on the others; srx_ibp_u8lr_workspace_bytes (shape only) covers both.
 * srx_saa_u8lr_workspace_bytes = srx_saa_workspace_bytes + align_up(Bc N h w sizeof(T)), Bc = the items of one chunk (B, or
 * max(32768 / N, 1) when B N > 32768), on every route: the query has no shift table to tell them apart.
 * Registration reads the bytes as well (srx_register_u8_*, with srx_register_* below), srx_psf_estimate_u8 the pinhole frames and srx_mean_u8
 * (with the index maps below) the reps and frames that are averaged: every stage that touches the camera's frames has a uint8 form. */
size_t srx_saa_u8lr_workspace_bytes(int elem_bytes, int B, int N, int h, int w, int factor);
int srx_saa_u8lr_f32(const uint8_t *lr, int B, int N, int h, int w, const double *shifts_yx, int factor, float *out, void *ws,
                     size_t ws_bytes, srx_stream_t stream, unsigned flags);
int srx_saa_u8lr_f64(const uint8_t *lr, int B, int N, int h, int w, const double *shifts_yx, int factor, double *out, void *ws,
                     size_t ws_bytes, srx_stream_t stream, unsigned flags);
size_t srx_ibp_u8lr_workspace_bytes(int elem_bytes, int B, int N, int h, int w, int H, int W, int factor, unsigned flags);
size_t srx_ibp_u8lr_workspace_bytes_for(int elem_bytes, int B, int N, int h, int w, int H, int W, int factor, const double *shifts_yx,
                                        const double *kernel, int kh, int kw, unsigned flags);
int srx_ibp_u8lr_f32(const uint8_t *lr, int B, int N, int h, int w, const double *shifts_yx, const double *kernel, int kh, int kw,
                     const float *hr_init, int H, int W, int factor, int n_iter, double step, float *hr_out, double *errors_out, void *ws,
                     size_t ws_bytes, srx_stream_t stream, unsigned flags);
int srx_ibp_u8lr_f64(const uint8_t *lr, int B, int N, int h, int w, const double *shifts_yx, const double *kernel, int kh, int kw,
                     const double *hr_init, int H, int W, int factor, int n_iter, double step, double *hr_out, double *errors_out, void *ws,
                     size_t ws_bytes, srx_stream_t stream, unsigned flags);

/* ---- shift_and_add / ibp with one shift table PER ITEM: what registration measures (srx_register_* returns [B, N, 2]) ----
 * shifts_byx is HOST float64 [B, N, 2]; everything else is the shared-table call's.  Item b returns exactly the bits of srx_saa_* /
 * srx_ibp_* with B = 1 on item b's frames, hr_init and table shifts_byx[b] under the same flags: the output, the MSE trace, hr_out ==
 * hr_init.  The header's conventions hold: the tables are read before the call returns, nothing is allocated on the device, only kernels
 * and device-to-device copies are queued, the memory contract holds, and the argument checks and limits of the shared-table calls apply
 * per item -- a refusal for any item (SRX_FLAG_FUSED on an item that cannot fuse) is decided on the host before anything is queued.
 * Routing: the route is decided once per DISTINCT table (what srx_ibp_path_for / srx_saa_path_for answer on shifts_byx[b]) and the batch is walked in
 * maximal runs of consecutive items:
 *   items that all route to "btile" (float32, x2, per-frame fractional shifts; their tables may all differ): one batch, the kernels take
 *     each item's table and the range of ITS tap origins from a device array;
 *   any other run of bytewise-equal tables: the driver of its route as a batch of the run's length.  Every table equal: the call IS the
 *     shared-table call -- same route, same bits, same launches;
 *   items on "fused" / "composed" with pairwise different tables run one by one (batching those routes' tile kernels per item is not done).
 *   shift_and_add: the same with "fused" in the place of "btile".
 * srx_last_path() reports the common route name if every run took the same one, else "mixed".  Batches above 32768 items go through in
 * chunks, as everywhere.  The per-item tables travel as kernel arguments, 960 words per launch: a "btile" run of n items makes
 * ceil(n (4 + 20 N) / 960) parameter launches, a "fused" shift_and_add run ceil(n N sizeof(tap) / 3840) (tap: 40 bytes f32, 72 f64).
 * Workspace: srx_ibp_items_workspace_bytes_for = the largest run's srx_ibp_workspace_bytes_for at the run's length, plus
 * align_up(n (4 + 20 N) 4) for a per-item "btile" run of n items; srx_ibp_items_workspace_bytes (shape only) covers it for every table.
 * srx_saa_items_workspace_bytes = srx_saa_workspace_bytes + align_up(Bc N sizeof(tap)), Bc = min(B, max(32768 / N, 1)).
 * There are no uint8 forms: the per-frame routes stage the bytes to T anyway (convert with srx_u8_to_*; the result is the same bits). */
size_t srx_saa_items_workspace_bytes(int elem_bytes, int B, int N, int h, int w, int factor);
int srx_saa_items_f32(const float *lr, int B, int N, int h, int w, const double *shifts_byx, int factor, float *out, void *ws,
                      size_t ws_bytes, srx_stream_t stream, unsigned flags);
int srx_saa_items_f64(const double *lr, int B, int N, int h, int w, const double *shifts_byx, int factor, double *out, void *ws,
                      size_t ws_bytes, srx_stream_t stream, unsigned flags);
size_t srx_ibp_items_workspace_bytes(int elem_bytes, int B, int N, int h, int w, int H, int W, int factor, unsigned flags);
size_t srx_ibp_items_workspace_bytes_for(int elem_bytes, int B, int N, int h, int w, int H, int W, int factor, const double *shifts_byx,
                                         const double *kernel, int kh, int kw, unsigned flags);
int srx_ibp_items_f32(const float *lr, int B, int N, int h, int w, const double *shifts_byx, const double *kernel, int kh, int kw,
                      const float *hr_init, int H, int W, int factor, int n_iter, double step, float *hr_out, double *errors_out, void *ws,
                      size_t ws_bytes, srx_stream_t stream, unsigned flags);
int srx_ibp_items_f64(const double *lr, int B, int N, int h, int w, const double *shifts_byx, const double *kernel, int kh, int kw,
                      const double *hr_init, int H, int W, int factor, int n_iter, double step, double *hr_out, double *errors_out, void *ws,
                      size_t ws_bytes, srx_stream_t stream, unsigned flags);

/* ---- the same loop as a PLAN: tables built once, the iterations in several runs, rows of the state readable / replaceable in between ----
 * No reference counterpart (its ibp() is one call); this is what running ONE image on several GPUs needs (second row: row bands
 * with a halo exchange every few iterations, sr_mi355x/rowband.py), and what any caller that iterates in instalments saves: the ~0.5 ms of
 * per-call table building around a 39 us iteration.
 *   create : as srx_ibp_* without n_iter; [trace_row_lo, trace_row_hi) = the HR rows whose LR samples the MSE trace counts (a sample belongs to the
 *            HR row it lands on, clamped to the image): 0, H for a whole image, a rank's own rows for a row band -- the ranks' traces then add up
 *            to the whole image's.  lr, workspace (srx_ibp_plan_workspace_bytes) and the plan stay alive until destroy.
 *   run    : n more iterations; errors (device float64 [B, n], may be NULL) = this run's slice of the trace.  SRX_E_UNSUPPORTED if a trace over a
 *            row range is asked of a plan that cannot restrict it (srx_ibp_plan_supports_trace_rows() == 0: every path but the float32
 *            integer-shift frame kernel, whose tables the plan hoists; the others run a whole srx_ibp call per run)
 *   get / set_rows : HR rows [row_lo, row_hi) of the current state <-> a packed [B, rows, W] device buffer */
typedef struct srx_plan_s srx_plan_t;
size_t srx_ibp_plan_workspace_bytes(int elem_bytes, int B, int N, int h, int w, int H, int W, int factor, unsigned flags);
int srx_ibp_plan_create_f32(const float *lr, int B, int N, int h, int w, const double *shifts_yx, const double *kernel, int kh, int kw,
                            const float *hr_init, int H, int W, int factor, double step, int trace_row_lo, int trace_row_hi, void *ws,
                            size_t ws_bytes, srx_stream_t stream, unsigned flags, srx_plan_t **plan);
int srx_ibp_plan_create_f64(const double *lr, int B, int N, int h, int w, const double *shifts_yx, const double *kernel, int kh, int kw,
                            const double *hr_init, int H, int W, int factor, double step, int trace_row_lo, int trace_row_hi, void *ws,
                            size_t ws_bytes, srx_stream_t stream, unsigned flags, srx_plan_t **plan);
int srx_ibp_plan_run(srx_plan_t *plan, int n_iter, double *errors_out, srx_stream_t stream);
int srx_ibp_plan_get_rows_f32(srx_plan_t *plan, int row_lo, int row_hi, float *dst, srx_stream_t stream);
int srx_ibp_plan_set_rows_f32(srx_plan_t *plan, int row_lo, int row_hi, const float *src, srx_stream_t stream);
int srx_ibp_plan_get_rows_f64(srx_plan_t *plan, int row_lo, int row_hi, double *dst, srx_stream_t stream);
int srx_ibp_plan_set_rows_f64(srx_plan_t *plan, int row_lo, int row_hi, const double *src, srx_stream_t stream);
const char *srx_ibp_plan_path(srx_plan_t *plan);          /* "ztile" (tables hoisted) or "call per run" */
int srx_ibp_plan_supports_trace_rows(srx_plan_t *plan);
void srx_ibp_plan_destroy(srx_plan_t *plan);

/* ---- index maps and pointwise glue of the drivers (bit-exact) ----
 * decimate:    out[i, j] = in[py + i*f, px + j*f]     `shifted[::f, ::f]` run_sr.py:165;
 *              with f=2, py=px=0 it is extract_red (rgb_cal_target/run_sr.py:73-75).
 *              in [B, H, W] -> out [B, ceil((H-py)/f), ceil((W-px)/f)].
 *              _u8: the same index map on bytes -- the red plane of a raw Bayer frame stays uint8 (rgb_cal_target/run_sr.py:73-75).
 * zero_insert: out = 0; out[i*f, j*f] = in[i, j] for i*f < H, j*f < W   run_sr.py:170-175.
 *              in [B, eh, ew] -> out [B, H, W].
 * mean_frames: out = sum_r in[r] / R   (np.mean(axis=0)) run_sr.py:274, rgb_cal_target :107-108.
 *              in [B, R, n] -> out [B, n].
 * u8_to:       uint8 -> T            (load_gray: run_sr.py:73-75)
 * quantize_u8: np.clip(x, 0, 255).astype(np.uint8) -- clamp then TRUNCATE   run_sr.py:303.
 */
int srx_decimate_f32(const float *in, int B, int H, int W, int f, int py, int px, float *out, srx_stream_t stream);
int srx_decimate_f64(const double *in, int B, int H, int W, int f, int py, int px, double *out, srx_stream_t stream);
int srx_decimate_u8(const uint8_t *in, int B, int H, int W, int f, int py, int px, uint8_t *out, srx_stream_t stream);
int srx_zero_insert_f32(const float *in, int B, int eh, int ew, int f, int H, int W, float *out, srx_stream_t stream);
int srx_zero_insert_f64(const double *in, int B, int eh, int ew, int f, int H, int W, double *out,
                        srx_stream_t stream);
int srx_mean_frames_f32(const float *in, int B, int R, size_t n, float *out, srx_stream_t stream);
int srx_mean_frames_f64(const double *in, int B, int R, size_t n, double *out, srx_stream_t stream);
int srx_u8_to_f32(const uint8_t *in, size_t n, float *out, srx_stream_t stream);
int srx_u8_to_f64(const uint8_t *in, size_t n, double *out, srx_stream_t stream);
int srx_quantize_u8_f32(const float *in, size_t n, uint8_t *out, srx_stream_t stream);
int srx_quantize_u8_f64(const double *in, size_t n, uint8_t *out, srx_stream_t stream);

/* ---- rep / frame mean on the camera's own samples: rgb_cal_target/run_sr.py:73-75 + 107-108 (f = 2, py = px = 0: the
 * Bayer red plane of every rep, averaged), mono_cal_target/run_sr.py:274 (f = 1: np.mean(lr_frames, 0)) ----
 * in uint8 [B, R, H, W] -> out T [B, h, w], h = ceil((H - py) / f), w = ceil((W - px) / f); T is float for out_elem_bytes 4 and double
 * for 8.  out[b, i, j] = (T)sum_r in[b, r, py + i f, px + j f] / (T)R: exactly the bits of srx_mean_frames_T on srx_decimate_T on
 * srx_u8_to_T of the frames.  Every partial sum of that chain is an integer of at most 255 R, exact in T (R <= 65535: below 2^24), so the
 * order of the additions does not matter and the one division is the only rounding.
 * No workspace, no allocation: one kernel launch on `stream`, no host synchronisation, capture-safe like the index maps above.
 * `in` needs byte alignment only and `out` the alignment of T (frame r of a stack of odd H W starts on any byte, and so does a row of odd
 * W): for f = 1 and f = 2 with H W a multiple of 16 every row peels a scalar head and tail around its own aligned 16-byte reads, and a
 * lane stores 16 bytes at once only where it finds the address aligned; every other shape goes sample by sample.
 * SRX_E_INVALID: a null pointer; B, R, H, W or f <= 0; py outside [0, H) or px outside [0, W); out_elem_bytes not 4 or 8.
 * SRX_E_UNSUPPORTED: R > 65535 (the float sum would no longer be exact), B > 65535, one item's R H W of 2 GiB or more.  Both are
 * decided on the host before any HIP call. */
int srx_mean_u8(const uint8_t *in, int B, int R, int H, int W, int f, int py, int px, int out_elem_bytes /* 4, 8 */, void *out,
                srx_stream_t stream);

/* ---- a frame as a batch of overlapping patches, and the patches blended back into a frame ----
 * No reference counterpart (it reconstructs a session under ONE shift table): these two index maps lead from a frame stack to the batched
 * per-item entry points (srx_register_* with B = patches, srx_saa_items_* / srx_ibp_items_* with one table per patch) and back, so that a
 * reconstruction can follow a shift that varies over the field (sr_mi355x/patchwise.py).
 * Grid rule, per axis of n samples, patch length L, stride s: count = ceil((n - L) / s) + 1 patches, origin(i) = min(i s, n - L) -- the
 * last patch is pulled inward, never padded, so every patch holds L real samples.  Patch p = iy count_x + ix; batch item b of the frames
 * owns items [b P, (b + 1) P), P = count_y count_x.
 *   srx_patches_count(n, L, s): the count of one axis, on the host (0 for arguments no call accepts: n, L or s <= 0, L > n, s > L, 2 s < L).
 *   gather: frames T [B, N, h, w] -> patches T [B P, N, ph, pw] (the srx_ibp_items layout); T = uint8 keeps the bytes, so srx_register_u8_*
 *           and the u8lr calls take them.  A pure index map, bit-exact.
 *   blend : HR patches T [B P, PH, PW] -> out T [B, H, W].  Per axis, with R = L - s - 2 margin, patch i at origin o_i weighs the
 *           coordinate x inside it by w_i(x) = clamp(min(dl, dr), 0, R), dl = x - o_i + 1 - margin if o_i > 0 else R, dr = o_i + L - x -
 *           margin if o_i + L < n else R: nothing over the outer `margin` samples of a patch (where its reconstruction feels the patch's
 *           own border), a ramp of R steps, R inside; no ramp and no margin at an edge of the image.  out = sum (T)(wy_i wx_j) v_ij /
 *           (T)(Sy Sx), Sy = sum_i wy_i, Sx = sum_j wx_j: the integer product converted once, each term rounded once, the terms added in
 *           ascending (i, j) by plain additions (nothing fused), one division -- numpy reproduces the bits (tests/patchwise_cases.py).
 *           A term of weight 0 is not read.  With 2 s >= L at most 3 patches per axis cover a sample and the weight sum is positive.
 * One kernel launch each on `stream`; no workspace, no allocation, no host synchronisation, capture-safe.  Inputs are never written and
 * nothing is written outside the output.  Caller pointers need the alignment of their element only (a uint8 row of odd w starts on any
 * byte): a row, or a lane's 16 bytes of one, goes as 16-byte vectors only where the kernel finds source and destination aligned itself.
 * SRX_E_INVALID: a null pointer; B, N, h or w <= 0; L <= 0 or L > n; s <= 0 or s > L (either axis); blend: margin < 0 or R < 1.
 * SRX_E_UNSUPPORTED: 2 s < L; one item's frames (gather) or one plane (blend) of 2 GiB or more; B P > 2^31 - 1.  All decided on the
 * host before any HIP call, in this order. */
int srx_patches_count(int n, int L, int stride);
int srx_patches_gather_u8(const uint8_t *frames, int B, int N, int h, int w, int ph, int pw, int sy, int sx, void *patches, srx_stream_t stream);
int srx_patches_gather_f32(const float *frames, int B, int N, int h, int w, int ph, int pw, int sy, int sx, void *patches, srx_stream_t stream);
int srx_patches_gather_f64(const double *frames, int B, int N, int h, int w, int ph, int pw, int sy, int sx, void *patches, srx_stream_t stream);
int srx_patches_blend_f32(const float *patches, int B, int H, int W, int PH, int PW, int SY, int SX, int margin, void *out, srx_stream_t stream);
int srx_patches_blend_f64(const double *patches, int B, int H, int W, int PH, int PW, int SY, int SX, int margin, void *out, srx_stream_t stream);

/* ---- the output PNGs' compressed stream, built on the device: the encoder half of cv2.imwrite / session.write_png_u8
 * (mono_barcodes/run_sr.py:303-306) ----
 * img T [B, H, W] -> streams uint8 [B][srx_png_stream_bound(H, W)], lengths int64 [B] (both DEVICE arrays, any byte address).  Bytes
 * [0, lengths[b]) of slot b are a complete zlib stream (RFC 1950 / 1951) that inflates to the PNG scanlines of image b: H rows of 1 + W
 * bytes, filter byte 2 (Up: the sample minus the one above it modulo 256, row 0 against zeros).  A host wraps it with the PNG signature,
 * IHDR, one IDAT and IEND (session.png_container) and has the file; srx_png_file_* below does that on the device.  The float forms quantise as they
 * read, with srx_quantize_u8_T's arithmetic (clamp, then truncate: the same device function, so the same byte for every input); no uint8
 * plane exists in between.
 * Stream: 78 01; the H (W + 1) scanline bytes in chunks of SRX_PNG_CHUNK, each coded on its own and starting on a byte boundary --
 * literals and distance-1 matches of 3..258 bytes (run lengths only, like Z_RLE; a run is cut where the 128-byte span of a lane ends), one
 * dynamic-Huffman block with the chunk's own length-limited (15-bit, complete) literal/length code and one distance code, header in a
 * fixed 1222-bit form, end-of-block, an empty stored block as byte alignment; a chunk that would not come out smaller than its n bytes + 5
 * goes as one stored block, so a chunk never takes more than n + 5 bytes; then a final empty fixed block 03 00 and the Adler-32 of the
 * scanlines, combined on the device from per-chunk sums in integers.
 *   srx_png_stream_bound(H, W) = 2 + H (W + 1) + 5 ceil(H (W + 1) / SRX_PNG_CHUNK) + 6: bytes of one image's slot (0 for H or W <= 0).
 *   srx_png_scratch_bytes(B, H, W): the workspace of a call, a multiple of 256 (0 for arguments no call accepts).
 * Three kernel launches on `stream` whatever the samples hold; no allocation, no host synchronisation, no memset or copy node.  The bytes
 * are the same run to run, and item b of a batch gets the bytes of a B = 1 call on its image.  The workspace may hold anything on entry
 * (bits are ORed together in LDS only), inputs are never written, and nothing is written outside the slots (of which only
 * [0, lengths[b]) is written), `lengths` and [0, ws_bytes).  `img` needs the alignment of its element only.
 * SRX_E_INVALID: a null pointer; B, H or W <= 0.  SRX_E_UNSUPPORTED: H (W + 1) of 2 GiB or more, B > 65535.  SRX_E_WORKSPACE: the
 * workspace is shorter than srx_png_scratch_bytes or not 256-byte aligned.  All decided on the host before any HIP call. */
#define SRX_PNG_CHUNK 32768
size_t srx_png_stream_bound(int H, int W);
size_t srx_png_scratch_bytes(int B, int H, int W);
int srx_png_deflate_u8(const uint8_t *img, int B, int H, int W, void *streams, void *lengths, void *ws, size_t ws_bytes, srx_stream_t stream);
int srx_png_deflate_f32(const float *img, int B, int H, int W, void *streams, void *lengths, void *ws, size_t ws_bytes, srx_stream_t stream);
int srx_png_deflate_f64(const double *img, int B, int H, int W, void *streams, void *lengths, void *ws, size_t ws_bytes, srx_stream_t stream);

/* ---- CRC-32 of device buffers (zlib's and PNG's: reflected, P = 0xEDB88320, init and final xor 0xFFFFFFFF) ----
 * Item b is bytes [0, min(lengths[b], max_len)) at data + b * stride; crc[b] = zlib.crc32(item, seed) (seed 0: a fresh CRC; a length of 0
 * or less gives `seed`).  `data` may sit at any byte address and any stride >= max_len is allowed; `lengths` is a DEVICE int64 [B], 8-byte
 * aligned and read on the device, or NULL for "every item is max_len long" (max_len only sizes the grid); `crc` is a DEVICE uint32 [B],
 * 4-byte aligned.  No byte at or behind an item's length is read into its result.
 * CRC-32 is linear over GF(2): a workgroup reduces one segment of SRX_CRC_SEGMENT bytes, each of its 256 lanes one span of SRX_CRC_SPAN
 * bytes through a byte table in LDS, and combines the spans' remainders with multiplications by x^(8 bytes that follow) mod P; a second
 * kernel combines the segments the same way and adds the seed's term.  Segments and spans are counted from the item's END (the first
 * segment and its first span are the short ones), so an item of n bytes has ceil(n / SRX_CRC_SEGMENT) segments.
 *   srx_crc32_scratch_bytes(B, max_len): the workspace of a call, a multiple of 256 (0 for arguments no call accepts).
 * Two kernel launches on `stream`; no allocation, no host synchronisation, no memset or copy node; a fixed order, so the same bits run to
 * run, and item b of a batch gets the value of a B = 1 call.  The workspace may hold anything on entry; only crc[0, B) and [0, ws_bytes)
 * are written.
 * SRX_E_INVALID: a null data or crc; B <= 0; max_len == 0; stride < max_len with B > 1; lengths not 8-byte or crc not 4-byte aligned.
 * SRX_E_UNSUPPORTED: B > 65535, max_len of 2 GiB or more.  SRX_E_WORKSPACE: the workspace is shorter than srx_crc32_scratch_bytes or not
 * 256-byte aligned.  All decided on the host before any HIP call, in this order. */
#define SRX_CRC_SPAN 64
#define SRX_CRC_SEGMENT 16384
size_t srx_crc32_scratch_bytes(int B, size_t max_len);
int srx_crc32(const void *data, int B, size_t stride, size_t max_len, const void *lengths, uint32_t seed, void *crc, void *ws, size_t ws_bytes,
              srx_stream_t stream);

/* ---- the output PNGs as complete files, built on the device: srx_png_deflate_*'s stream inside its container ----
 * img T [B, H, W] -> files uint8 [B][srx_png_file_bound(H, W)], lengths int64 [B] (both DEVICE arrays, any byte address).  Bytes
 * [0, lengths[b]) of slot b are the 8-bit greyscale PNG file of image b: the signature, IHDR with its CRC, one IDAT whose data is exactly
 * the stream srx_png_deflate_* writes for the same image, the IDAT's CRC-32, IEND (what session.png_container builds around that stream on
 * the host); lengths[b] is the stream's length + SRX_PNG_FILE_EXTRA.  A host writes the bytes to disk and has the file.
 * The three launches of srx_png_deflate_* put the stream 41 bytes into the slot and its length into the workspace; srx_crc32's two kernels
 * then reduce the stream under the seed crc32("IDAT") (the chunk's CRC covers its tag) and the second one stores the 41 bytes in front
 * (IHDR and its CRC depend on W and H only: the host computes them and passes them as an argument), the 16 bytes behind and lengths[b].
 *   srx_png_file_bound(H, W) = srx_png_stream_bound(H, W) + SRX_PNG_FILE_EXTRA: bytes of one image's slot (0 for H or W <= 0).
 *   srx_png_file_scratch_bytes(B, H, W): the workspace of a call, a multiple of 256 and at least srx_png_scratch_bytes (0 for arguments
 *   no call accepts).
 * Five kernel launches on `stream`; otherwise the contract of srx_png_deflate_*: no allocation, no host synchronisation, the same bytes
 * run to run and for item b of a batch as for a B = 1 call; the workspace may hold anything on entry; nothing is written outside
 * [0, lengths[b]) of the slots, `lengths` and [0, ws_bytes); the same refusals in the same order. */
#define SRX_PNG_FILE_EXTRA 57 /* 8 + 25 + 8 in front of the stream, 4 + 12 behind it */
size_t srx_png_file_bound(int H, int W);
size_t srx_png_file_scratch_bytes(int B, int H, int W);
int srx_png_file_u8(const uint8_t *img, int B, int H, int W, void *files, void *lengths, void *ws, size_t ws_bytes, srx_stream_t stream);
int srx_png_file_f32(const float *img, int B, int H, int W, void *files, void *lengths, void *ws, size_t ws_bytes, srx_stream_t stream);
int srx_png_file_f64(const double *img, int B, int H, int W, void *files, void *lengths, void *ws, size_t ws_bytes, srx_stream_t stream);

/* ---- 4-frame pixel interleave of the vendor live view (opt_materials/software/XPR_Software.py:196-205, 388-410) ----
 * frames uint8 [B, 4, h, w] -> out uint8 [B, 2h, 2w]: frame k zero-inserted at [::2, ::2], translated by the integer
 * (tx, ty) = (0,0), (0,+1), (-1,+1), (-1,0) HR pixels with cv2.BORDER_REFLECT_101, the four planes summed as uint8. */
int srx_interleave4_u8(const uint8_t *frames, int B, int h, int w, uint8_t *out, srx_stream_t stream);

/* ---- quality metrics that consume the reconstructions, on DEVICE images ----
 * The reference computes these in its notebook / calibration scripts from the PNGs it wrote (mono_cal_target/analysis.ipynb cells 4, 7, 10;
 * data_collection/psf_mtf_utils.py:67-95; the vendor GUI's PSNR, opt_materials/software/XPR_Software.py:735-745, 1215-1256).  These entry points
 * are the parts that are work on a frame or an ROI; sr_mi355x/metrics.py keeps the few-thousand-operation host parts (percentile, line fits,
 * 72-sample FFT, the 7-parameter fit, compute_mtf's 256^2 FFT).  All results are float64 DEVICE arrays; every sum is a fixed-order reduction
 * (bit-identical run to run).  Workspace: srx_metrics_workspace_bytes(B, H, W, nbin) covers every call below at those sizes
 * (a call is held to it at its own arguments, with B = 1 / nbin = 1 where it has none).
 *   pair_moments : out[b] = {n, sum t, sum r, sum t^2, sum t r, sum r^2, sum (r - t)^2} over rows / columns [border, size - border) of
 *                  ref / test [B, H, W]: PSNR = 10 log10(peak^2 n / out[6]); the affine-fit PSNR follows from the other five.
 *   local_contrast: (max - min) / (max + min + 1e-9) of profile[i - w/2 : i + w/2], 0 within w/2 of either end.  [B, n] -> [B, n]
 *   ring_sums    : ring k = pixels whose distance to (cy, cx) truncates to k: out = {sum[nbin], count[nbin]}   (radial_average)
 *                  1 <= nbin <= 4096 (otherwise SRX_E_INVALID); the centre may lie off the image.
 *   spot_moments : out = {max, sum p, sum p y, sum p x} over the pixels with p > 0.1 max                       (subpixel_centre)
 *                  H W <= 2^24 (otherwise SRX_E_INVALID).  The comparison is strict and in float64; no pixel above the threshold
 *                  (a maximum <= 0): the three sums are 0.
 *   edge_magnitude: Sobel magnitude of the Gaussian(sigma)-smoothed ROI, scipy.ndimage 'reflect' boundaries; float64 [H, W] -> [H, W]
 *                  sigma > 0 (otherwise SRX_E_INVALID); a radius int(4 sigma + 0.5) above 8 is SRX_E_UNSUPPORTED.
 *   edge_dist_range / edge_bins: every ROI pixel projected on the normal of the line v = m u + b ((u, v) = (row, col) if rows_are_x else
 *                  (col, row)): min / max of the distances in (-8, 10); sums and counts per 1/4-px bin [lo + i bw, lo + (i + 1) bw).
 *                  edge_dist_range: out = {lo, hi}; when no pixel lies in (-8, 10) it stores {1e300, -1e300} (lo > hi: nothing to bin).
 *                  H W <= 2^24 and norm > 0 (otherwise SRX_E_INVALID).  edge_bins: out = {sum[nbin], count[nbin]}, 1 <= nbin <= 128,
 *                  norm > 0 and bw > 0 (otherwise SRX_E_INVALID); a pixel in (-8, 10) outside [lo, lo + nbin bw) is in no bin.
 *   ssim         : skimage structural_similarity (2-D) of the crop [border, size - border) of ref / test [B, H, W], in ONE pass over the two
 *                  images: window sums of x, y, x^2, y^2, x y by the separable correlation taps[2 radius + 1] (host float64; uniform or
 *                  Gaussian) with scipy's 'reflect' boundary, C1 = (k1 data_range)^2, C2 = (k2 data_range)^2, cov_norm = NP / (NP - 1) if
 *                  sample_cov else 1 (NP = (2 radius + 1)^2).  mssim[b] = mean of S over the crop minus a radius-pixel rim (float64 device);
 *                  map (or NULL) = S over the whole crop, [B, H - 2 border, W - 2 border] in T.  affine (device [B][3] or NULL) = {ar, at, bt}:
 *                  x = ar ref, y = at test + bt, applied on the fly (the vendor view's fitted SSIM).  radius 1..7 (larger: SRX_E_UNSUPPORTED);
 *                  2 radius + 1 must not exceed either side of the crop. */
size_t srx_metrics_workspace_bytes(int B, int H, int W, int nbin);
int srx_pair_moments_f32(const float *ref, const float *test, int B, int H, int W, int border, double *out, void *ws, size_t ws_bytes,
                         srx_stream_t stream);
int srx_pair_moments_f64(const double *ref, const double *test, int B, int H, int W, int border, double *out, void *ws, size_t ws_bytes,
                         srx_stream_t stream);
int srx_local_contrast_f32(const float *profile, int B, int n, int window, float *out, srx_stream_t stream);
int srx_local_contrast_f64(const double *profile, int B, int n, int window, double *out, srx_stream_t stream);
int srx_ring_sums_f32(const float *img, int H, int W, double cy, double cx, int nbin, double *out, void *ws, size_t ws_bytes, srx_stream_t stream);
int srx_ring_sums_f64(const double *img, int H, int W, double cy, double cx, int nbin, double *out, void *ws, size_t ws_bytes, srx_stream_t stream);
int srx_spot_moments_f32(const float *img, int H, int W, double *out, srx_stream_t stream);
int srx_spot_moments_f64(const double *img, int H, int W, double *out, srx_stream_t stream);
int srx_edge_magnitude_f64(const double *roi, int H, int W, double sigma, double *mag, void *ws, size_t ws_bytes, srx_stream_t stream);
int srx_edge_dist_range(int H, int W, double m, double b, double norm, int rows_are_x, double *out, srx_stream_t stream);
int srx_edge_bins_f32(const float *roi, int H, int W, double m, double b, double norm, int rows_are_x, double lo, double bw, int nbin,
                      double *out, void *ws, size_t ws_bytes, srx_stream_t stream);
int srx_edge_bins_f64(const double *roi, int H, int W, double m, double b, double norm, int rows_are_x, double lo, double bw, int nbin,
                      double *out, void *ws, size_t ws_bytes, srx_stream_t stream);
int srx_ssim_f32(const float *ref, const float *test, int B, int H, int W, int border, int radius, const double *taps, int sample_cov,
                 double data_range, double k1, double k2, const double *affine, double *mssim, float *map, void *ws, size_t ws_bytes,
                 srx_stream_t stream);
int srx_ssim_f64(const double *ref, const double *test, int B, int H, int W, int border, int radius, const double *taps, int sample_cov,
                 double data_range, double k1, double k2, const double *affine, double *mssim, double *map, void *ws, size_t ws_bytes,
                 srx_stream_t stream);

/* ---- slanted-edge SFR of device ROIs in one call: metrics.slanted_edge_esf -> esf_to_mtf -> mtf_at_fraction (analysis.ipynb cells 6 - 10) ----
 * img T [B] ROIs of H x W, read in place: `img` points at the first sample of item 0's ROI, rows are row_pitch ELEMENTS apart and items
 * item_pitch elements (a ROI inside a [B, Hf, Wf] stack: row_pitch = Wf, item_pitch = Hf Wf); `img` needs the alignment of its element only.
 * side 0 ("left": the edge pixels with a negative distance to the centre line) or 1; sigma: the Gaussian of the edge detector (1.5).
 * Outputs, all DEVICE arrays; summary and status are required, esf and mtf may be NULL; every element of every output passed is written:
 *   summary float64 [B][SRX_EDGE_SUMMARY] = {mtf50, mtf10 (cycles per ROI pixel; NaN where the curve never falls through), angle_deg, m, b,
 *           rows_are_x, threshold, n_edge, n_side, nbin, lo, hi, flipped, m_c, b_c, 0}
 *   esf     float64 [B][2][SRX_EDGE_MAX_BINS]: x, then y; 0 behind nbin
 *   mtf     float64 [B][2][SRX_EDGE_MAX_BINS / 2]: frequency in cycles/px, then the MTF, DC included; 0 behind nbin / 2
 *   status  int32 [B]: 0 ok; 1 fewer than 20 edge pixels; 2 fewer than 10 on the chosen side; 3 a degenerate fit (the u of the pixels have no
 *           spread) or no pixel with a distance in (-8, 10); 4 nbin < 4 or fewer than 3 non-empty bins.  For a nonzero status the summary holds
 *           NaN for what was not reached (slot 15 stays 0) and the item's esf / mtf are NaN throughout; nothing is left unwritten.
 * Per item: the magnitude plane has the bits of srx_edge_magnitude_f64 on the ROI converted to double (the same device functions).  threshold =
 * np.percentile(mag, 85) bit for bit: an exact radix selection on the bit patterns (8-bit digits, integer histograms in LDS, ties counted), the
 * two order statistics around (n - 1) 0.85 combined as numpy's _lerp does.  That holds for FINITE samples: a NaN or Inf sample gives NaN
 * magnitudes, whose bit patterns order above +Inf here, where np.percentile returns NaN for the whole plane; nothing faults (a NaN
 * threshold leaves no edge pixel: status 1), but the value is then not numpy's.  Edge pixels: mag > threshold; rows_are_x = (row span >= column
 * span).  The two np.polyfit lines (m_c, b_c through all edge pixels, m, b through those on the chosen side) are the closed form on EXACT integer
 * sums n, su, sv, suu, suv: m = (n suv - su sv) / (n suu - su^2) with both differences exact (128-bit) and converted once, b = (sv - m su) / n.
 * lo, hi: min / max of the distances (v - m u - b) / sqrt(1 + m^2) in (-8, 10) (srx_edge_dist_range's expression); bin edges lo + i / 4,
 * ceil(((hi + 1/4) - lo) / (1/4)) of them as np.arange counts, nbin one less.  Bin sums in a fixed order: the rows in min(H, 256) groups of
 * ceil(H / groups) consecutive rows, a group's pixels of a bin added in raster order, then the groups in index order.  ESF = sum / count, empty
 * bins filled as np.interp fills them over the non-empty ones, reversed (x negated) if it falls; LSF = np.gradient's non-uniform second-order
 * form, times np.hanning; a direct DFT for k < nbin / 2 (the twiddle index j k reduced mod nbin in integers), divided by its DC value if positive;
 * freq[k] = k / (nbin mean(diff(x))); MTF50 / MTF10: the first downward crossing among k >= 1, interpolated as metrics.mtf_at_fraction does.
 *   srx_edge_sfr_scratch_bytes(B, H, W): the workspace of a call, a multiple of 256 (0 for arguments no call accepts).
 * Six kernel launches on `stream` whatever the samples hold; no allocation, no host synchronisation, no memset or copy node.  The bits are the
 * same run to run, and item b of a batch gets the bits of a B = 1 call.  The workspace may hold anything on entry; only the outputs and
 * [0, ws_bytes) are written; inputs are never written.
 * SRX_E_INVALID: a null img / summary / status; B, H or W <= 0; row_pitch < W; item_pitch < (H - 1) row_pitch + W with B > 1; side not 0 / 1;
 * sigma not > 0.  SRX_E_UNSUPPORTED: H W > 2^20, B > 65535, a Gaussian radius above 8 (as srx_edge_magnitude_f64).  SRX_E_WORKSPACE: the
 * workspace is shorter than srx_edge_sfr_scratch_bytes or not 256-byte aligned.  All decided on the host before any HIP call, in this order. */
#define SRX_EDGE_MAX_BINS 80 /* distances in (-8, 10) at 1/4 px give at most 72 bins */
#define SRX_EDGE_SUMMARY 16
size_t srx_edge_sfr_scratch_bytes(int B, int H, int W);
int srx_edge_sfr_u8(const uint8_t *img, int B, int H, int W, size_t row_pitch, size_t item_pitch, int side, double sigma, void *summary, void *esf,
                    void *mtf, void *status, void *ws, size_t ws_bytes, srx_stream_t stream);
int srx_edge_sfr_f32(const float *img, int B, int H, int W, size_t row_pitch, size_t item_pitch, int side, double sigma, void *summary, void *esf,
                     void *mtf, void *status, void *ws, size_t ws_bytes, srx_stream_t stream);
int srx_edge_sfr_f64(const double *img, int B, int H, int W, size_t row_pitch, size_t item_pitch, int side, double sigma, void *summary, void *esf,
                     void *mtf, void *status, void *ws, size_t ws_bytes, srx_stream_t stream);

/* ---- sub-pixel frame registration (translation only), on DEVICE frames ----
 * frames [B, N, H, W] (the srx_saa layout); for every item b and frame k != ref: d = shifts[b][k] with frames[k] ~ ndi.shift(frames[ref], d),
 * LR pixels, (dy, dx): the sign convention of shifts_yx, so anchor + d (anchor = the reference frame's known shift) goes straight into
 * srx_saa / srx_ibp.  shifts[b][ref] is exactly (0, 0).  Every sum runs over the reference crop [m, H - m) x [m, W - m),
 * m = border + search + 2; frame samples outside the frame take the nearest edge value.
 *   coarse : zero-mean NCC at every integer d = c0_k + (oy, ox), |oy|, |ox| <= search, c0_k = rint(init[k] - init[ref]) (init: host [N][2]
 *            or NULL = zeros); the argmax is taken on the device, ties to the smallest |dy| + |dx|, then the smaller dy, then dx.
 *   refine : Gauss-Newton on sum (t(i + d) - r(i))^2 with t the cubic B-spline interpolant of frame k ('nearest' edges, as ndi.shift) and its
 *            analytic gradient; each step is clamped to +-0.5 px per axis; a frame stops once max |step| < tol or after n_iter steps.
 *            No host synchronisation: the call only enqueues work on the stream.  Sums are fixed-order float64 (bit-identical run to run,
 *            a batch item bit-identical to the same item alone).
 *   score  : [B, N] float64 device or NULL: zero-mean NCC of t(i + d) against the crop at the returned d (0 if either is constant; 1 at ref).
 *   status : [B, N] int device or NULL: 0 ok; 1 singular normal matrix (flat or one-directional content: the coarse shift is kept, never
 *            NaN); 2 coarse argmax on the search boundary; 3 not converged after n_iter steps.  Where several apply the smallest code is
 *            returned: 1 over 2 over 3.
 * Held by tests/test_gpu_register_edges.py: n_iter = 0 returns the coarse integer shift and never status 3; tol = 0 never converges, so
 * with n_iter > 0 it always ends in status 3 unless 1 or 2 applies; c0_k rounds half to even (std::rint: 0.5 -> 0, 1.5 -> 2, 2.5 -> 2,
 * -3.5 -> -4); |init[k] - init[ref]| <= 1e6 is accepted on both axes -- so far out every sample is the frame's clamped corner, the
 * window is constant, the score is exactly 0 at every offset and the tie rule alone decides.
 * SRX_E_INVALID: a null frames / shifts, B or size <= 0, N < 2, ref outside [0, N), search outside [0, 4], border < 0, n_iter < 0, tol < 0
 * or NaN, |init[k] - init[ref]| > 1e6.  SRX_E_UNSUPPORTED: a crop smaller than 16 x 16, N > SRX_MAX_FRAMES, B (N - 1) > 65535.
 * Workspace: srx_register_workspace_bytes(sizeof(T), B, N, H, W, search) (0 for arguments no call accepts) covers every border. */
size_t srx_register_workspace_bytes(int elem_bytes, int B, int N, int H, int W, int search);
int srx_register_f32(const float *frames, int B, int N, int H, int W, int ref, const double *init_yx, int search, int border, int n_iter, double tol,
                     double *shifts, double *score, int *status, void *ws, size_t ws_bytes, srx_stream_t stream);
int srx_register_f64(const double *frames, int B, int N, int H, int W, int ref, const double *init_yx, int search, int border, int n_iter,
                     double tol, double *shifts, double *score, int *status, void *ws, size_t ws_bytes, srx_stream_t stream);

/* ---- registration on the camera's own samples: load_gray's uint8 frames (run_sr.py:73-75) without the astype(float64) ----
 * frames is uint8 [B, N, H, W]; _f32 / _f64 is the type T of the spline coefficients and of the arithmetic, as in srx_saa_u8lr_*.  A call
 * returns exactly the bits of srx_register_T on the frames converted with srx_u8_to_T: shifts, score and status, the reference rows, frozen
 * and singular frames, a batch item against the same item alone.  (T)uint8 is exact, so the coefficients and the Gauss-Newton sums are the
 * float call's; the coarse sums are formed in integers on packed bytes (four samples per dot instruction) -- sums of 8-bit samples and
 * their products over a crop stay below 2^53, so the float call's float64 sums are those integers, in any order.  Everything else is the
 * float call's: the argument checks and their order, the limits (the 2 GiB rule counts a padded plane as T), init_yx, the launches, no
 * allocation and no host synchronisation.  frames needs byte alignment only (frame k of a stack of odd H W starts on any byte, a row of
 * odd W likewise): the kernel that reads words aligns its own reads and takes single bytes at the two ends of the stack.
 * Workspace: srx_register_workspace_bytes(sizeof(T), B, N, H, W, search), the float call's -- the coefficient and scratch planes stay T;
 * no converted copy of the frames exists anywhere. */
int srx_register_u8_f32(const uint8_t *frames, int B, int N, int H, int W, int ref, const double *init_yx, int search, int border, int n_iter,
                        double tol, double *shifts, double *score, int *status, void *ws, size_t ws_bytes, srx_stream_t stream);
int srx_register_u8_f64(const uint8_t *frames, int B, int N, int H, int W, int ref, const double *init_yx, int search, int border, int n_iter,
                        double tol, double *shifts, double *score, int *status, void *ws, size_t ws_bytes, srx_stream_t stream);

/* ---- the measured PSF from pinhole frames (load_measured_psf, mono_cal_target/run_sr.py:114-152), on DEVICE frames ----
 * frames [N, H, W] of uint8 (_u8: the camera's own samples, no conversion), float or double; reach = halfwidth + 6, side = 2 halfwidth + 1
 * (the 6 is the reference's constant).  Per frame: the peak = the row-major first sample equal to the frame's maximum (np.argmax,
 * run_sr.py:131); the frame is used if the window of +-reach around the peak lies inside it (reach <= row, row + reach < H, the same for the
 * column; :133-135), dropped otherwise.  The used windows are added in frame order in float64 and divided by their number (:140, bit for bit
 * numpy's stack.mean(axis=0)), cut to the central side x side (:141-142), the mean of the 36 samples at rows and columns
 * {0, 1, 2, side-3, side-2, side-1} (repeats included when side < 6) is taken off as background (:145-147), negatives are clipped and the
 * kernel is divided by its sum (:148-150).
 *   psf   : [side][side] float64 DEVICE: what srx_ibp takes as `kernel` once copied to the host.
 *   info  : [N][3] int32 DEVICE or NULL: {peak row, peak column, used (1 / 0)}; the peak is reported for dropped frames too.
 *   ties  : samples tie by value equality (==: -0.0 and +0.0 tie), the smaller index wins.  Frames are expected NaN-free; if they are not, a
 *           NaN never wins, and a frame with no winning sample (all NaN) reports the peak (0, 0).
 *   no frame used: psf is all zeros.  Frames used but nothing left above the background: the division is done anyway (0 / 0 = NaN), as the
 *           host form does.
 * At most three kernel launches, no host synchronisation; sums and ties are fixed-order (bit-identical run to run).  The frame pointer needs
 * only element alignment (frame k of a uint8 stack of odd H W starts at any byte: the kernels align their own 16-byte reads).
 * SRX_E_INVALID: a null frames / psf, N, H or W <= 0, halfwidth outside [1, 7] (side 15: SRX_MAX_KERNEL_TAPS).  SRX_E_UNSUPPORTED: one frame
 * of 2 GiB or more (indices inside a frame are 32-bit), N > 65535.  Workspace: srx_psf_estimate_workspace_bytes(sizeof(T), N, H, W,
 * halfwidth) (0 for arguments no call accepts). */
size_t srx_psf_estimate_workspace_bytes(int elem_bytes /* 1, 4, 8 */, int N, int H, int W, int halfwidth);
int srx_psf_estimate_u8(const uint8_t *frames, int N, int H, int W, int halfwidth, double *psf, int *info, void *ws, size_t ws_bytes,
                        srx_stream_t stream);
int srx_psf_estimate_f32(const float *frames, int N, int H, int W, int halfwidth, double *psf, int *info, void *ws, size_t ws_bytes,
                         srx_stream_t stream);
int srx_psf_estimate_f64(const double *frames, int N, int H, int W, int halfwidth, double *psf, int *info, void *ws, size_t ws_bytes,
                         srx_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SRX_H */
