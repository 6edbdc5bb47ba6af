/*
 * srx_bayer.h -- colour from raw Bayer (RGGB) frames: the part of libsrx.so's C ABI that turns a colour camera's raw frames into the four
 * Bayer planes, four reconstructed planes into an RGB image, and an RGB byte image into a finished PNG file.  srx.h has the types, the
 * status codes and everything between these two ends: the four planes of a frame set are a batch of four items for its batched calls, under
 * one shift table and one PSF (all four planes have the same pitch).
 *
 * Conventions (those of srx.h, written out)
 *   - Plain C ABI: pointers + sizes.  Suffix _u8 / _f32 / _f64 = element type T of the image buffers (uint8_t / float / double).
 *   - Image buffers are DEVICE pointers, C-contiguous, row-major, with a leading batch count B.  `gains` is a HOST pointer, float64,
 *     read before the call returns.
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream).  A call only queues kernels on it -- one launch each,
 *     srx_png_file_rgb8 five -- with no allocation, no host synchronisation, and no memset or copy node: it may be captured into a HIP graph.
 *   - Inputs are never written, and nothing is written outside the outputs (and bytes [0, ws_bytes) of srx_png_file_rgb8's workspace).
 *   - Caller pointers need only the alignment of their element type: a uint8 frame or row may start on any byte.  A kernel uses 16-byte
 *     accesses only at addresses it has found aligned itself, as srx_mean_u8 does.
 *   - Return value: SRX_OK (0) or a negative srx_status.  Every refusal is decided on the host before any HIP call, in the order listed:
 *     SRX_E_INVALID first, then SRX_E_UNSUPPORTED (then, for srx_png_file_rgb8, SRX_E_WORKSPACE).
 *
 * Plane order everywhere: p = 0..3 is R (0,0), G1 (0,1), G2 (1,0), B (1,1); plane p holds raw[py::2, px::2] with (py, px) = (p >> 1, p & 1).
 */
#ifndef SRX_BAYER_H
#define SRX_BAYER_H

#include "srx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* raw [B, H, W] -> planes [B, 4, H/2, W/2] of the same element type: a pure index map.  Plane p has the bits of
 * srx_decimate_T(raw, f = 2, py, px).
 * SRX_E_INVALID: a null pointer; B, H or W <= 0.  SRX_E_UNSUPPORTED: H or W odd (the four planes would differ in size); one item of
 * 2 GiB or more; B > 65535. */
int srx_bayer_split_u8(const uint8_t *raw, int B, int H, int W, void *planes, srx_stream_t stream);
int srx_bayer_split_f32(const float *raw, int B, int H, int W, void *planes, srx_stream_t stream);
int srx_bayer_split_f64(const double *raw, int B, int H, int W, void *planes, srx_stream_t stream);

/* raw uint8 [B, R, H, W] -> planes T [B, 4, H/2, W/2], T = float (out_elem_bytes 4) or double (8): the mean over the R frames.  Plane p has
 * the bits of srx_mean_u8(raw, B, R, H, W, 2, py, px, out_elem_bytes, ...) -- an integer sum and one division -- but every raw row is read
 * once and both column parities are kept (R = 1: the split with conversion).  Where H W is a multiple of 16 the rows go as aligned
 * 16-byte reads with a scalar head and tail per row; any other shape goes sample by sample.
 * SRX_E_INVALID: a null pointer; B, R, H or W <= 0; out_elem_bytes not 4 or 8.  SRX_E_UNSUPPORTED: H or W odd; R > 65535; B > 65535;
 * one item's R H W of 2 GiB or more. */
int srx_bayer_mean_u8(const uint8_t *raw, int B, int R, int H, int W, int out_elem_bytes, void *planes, srx_stream_t stream);

/* HR planes [B, 4, Hp, Wp] -> rgb T [B, 3, Hp, Wp] (planar): the four reconstructions laid over each other, no interpolation.  d is the
 * number of HR samples per raw pixel: factor / 2 for an even factor, 0 to stack the planes as they are.  HR sample x of the R plane sits at
 * raw column 2 x / f and sample x' of G1 at 2 x' / f + 1, so the same place is x' = x - d.  With c(i, n) = min(max(i, 0), n - 1):
 *     R [y, x] = P0[y, x]
 *     g1       = P1[y, c(x - d, Wp)]
 *     g2       = P2[c(y - d, Hp), x]
 *     G [y, x] = (g1 + g2) * (T)0.5          (one addition, then the multiplication; nothing fused)
 *     Bl[y, x] = P3[c(y - d, Hp), c(x - d, Wp)]
 * and each channel is then multiplied once by (T)gains[ch]; gains == NULL: no multiplication at all.  numpy reproduces the bits in T:
 *     yc, xc = np.clip(np.arange(Hp) - d, 0, Hp - 1), np.clip(np.arange(Wp) - d, 0, Wp - 1)
 *     G = (P1[:, xc] + P2[yc, :]) * T(0.5);  Bl = P3[yc][:, xc];  rgb = np.stack([P0, G, Bl]) * gains.astype(T)[:, None, None]
 * SRX_E_INVALID: a null planes / rgb; B, Hp or Wp <= 0; d < 0.  SRX_E_UNSUPPORTED: one plane of 2 GiB or more; B > 65535. */
int srx_bayer_merge_f32(const float *planes, int B, int Hp, int Wp, int d, const double *gains, void *rgb, srx_stream_t stream);
int srx_bayer_merge_f64(const double *planes, int B, int Hp, int Wp, int d, const double *gains, void *rgb, srx_stream_t stream);

/* The same arithmetic, then srx_quantize_u8_T's clamp and truncation; rgb8 is interleaved uint8 [B, Hp, Wp, 3]: the bytes of quantising
 * srx_bayer_merge_T's result and interleaving it.  Refusals as srx_bayer_merge_T. */
int srx_bayer_merge_rgb8_f32(const float *planes, int B, int Hp, int Wp, int d, const double *gains, void *rgb8, srx_stream_t stream);
int srx_bayer_merge_rgb8_f64(const double *planes, int B, int Hp, int Wp, int d, const double *gains, void *rgb8, srx_stream_t stream);

/* img uint8 [B, H, W, 3] -> complete 8-bit truecolour PNG files (colour type 2), as srx_png_file_u8 makes grey ones: files is
 * [B, srx_png_file_rgb8_bound(H, W)] bytes, lengths int64 [B] (any alignment).  The Up filter works byte against the byte above, so the
 * scanlines are those of a grey image of width 3 W: the IDAT data is exactly the stream srx_png_deflate_u8 writes for img viewed as
 * [B, H, 3 W], and only the IHDR differs (width W, colour type 2).  Five launches; the contract, refusals and bounds of srx_png_file_u8 at
 * width 3 W, and the two queries equal srx_png_file_bound(H, 3 W) and srx_png_file_scratch_bytes(B, H, 3 W) (0 where 3 W does not fit an int).
 * SRX_E_INVALID: a null img / files / lengths; B, H or W <= 0.  SRX_E_UNSUPPORTED: 3 W does not fit an int; B > 65535; H (3 W + 1) of
 * 2 GiB or more.  SRX_E_WORKSPACE: ws null, not 256-byte aligned, or ws_bytes below srx_png_file_rgb8_scratch_bytes(B, H, W). */
size_t srx_png_file_rgb8_bound(int H, int W);
size_t srx_png_file_rgb8_scratch_bytes(int B, int H, int W);
int srx_png_file_rgb8(const uint8_t *img, int B, int H, int W, void *files, void *lengths, void *ws, size_t ws_bytes, srx_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* SRX_BAYER_H */
