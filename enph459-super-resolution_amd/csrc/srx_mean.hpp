// srx_mean.hpp -- the mean over R uint8 frames of the samples at [py::f, px::f] (srx_mean_u8): in uint8 [B, R, H, W] -> out T [B, h, w],
// out = (T)sum_r in / (T)R.  The sum is an integer of at most 255 * 65535 < 2^24, exact in float and in an unsigned; the one division is
// the only rounding, so the result is srx_mean_frames_T on srx_decimate_T on srx_u8_to_T of the frames, bit for bit.  One launch.
//
//   k_mean_u8_vec<T, F>  F = 1, 2 and H W a multiple of 16, so that a row of frame r and the same row of frame 0 sit at the same address mod 16.
//                 grid (groups of 4 output rows, groups of 64 vectors, B), block (64, 4).  A row is cut by ITS OWN first sample p (frame 0):
//                 [p, first 16-byte boundary) scalar | whole aligned 16-byte vectors inside the row | the rest scalar.  Neither the caller's
//                 pointer nor W need any alignment: every row finds its own cut, and no vector reaches past the end of its row.  A vector
//                 lane reads its 16 bytes of BATCH = 8 frames at a time (a remainder of k < 8 frames has its own run of k loads), all issued before the first is used, and forms 16 (F = 1) or 8 (F = 2)
//                 consecutive outputs.  Bytes are summed as 16-bit fields, two per dword: x & 0x00ff00ff is bytes 0 and 2, (x >> 8) &
//                 0x00ff00ff bytes 1 and 3; with F = 2 only the one of the two whose parity the row's p has.  A 16-bit field holds
//                 PACKED_MAX_R = 257 frames (255 * 257 = 65535); the frames are taken in groups of at most that many and the fields are
//                 spilled into 32-bit sums after each group, so R <= 257 is one group and every larger R several.  The head (< 16 outputs)
//                 and the tail (< 16) are one output per lane of the row's first lanes, byte loads.  Stores: a lane's outputs are NO
//                 consecutive T; they go as 16-byte vectors where the lane finds their address aligned, one by one otherwise.
//   k_mean_u8_any<T>     every other f, and frames that disagree on their misalignment (H W not a multiple of 16): one output per lane,
//                 R byte loads.
#pragma once
#include <algorithm>
#include "srx_common.h"

namespace srx {
namespace mean {

constexpr int PACKED_MAX_R = 257;  // frames a 16-bit field can sum: 255 * 257 = 65535
constexpr int BATCH = 8;           // 16-byte reads of one lane in flight
constexpr int MAX_ROW_BLOCKS = 4096, MAX_COL_BLOCKS = 2;  // grid caps: 16384 rows x 128 lanes (2 KiB of a row) per item; the lanes loop beyond these

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef double f64x2 __attribute__((ext_vector_type(2)));

template <typename T> struct Vec16;
template <> struct Vec16<float> {
    typedef f32x4 type;
    static constexpr int N = 4;
};
template <> struct Vec16<double> {
    typedef f64x2 type;
    static constexpr int N = 2;
};

// one output the plain way: the sample at byte offset `off` of every frame, summed over the frames
template <typename T> __device__ __forceinline__ T mean_one(const uint8_t *__restrict__ item, unsigned HW, int R, unsigned off)
{
    unsigned s = 0;
    for (int r = 0; r < R; r++)
        s += item[(unsigned)r * HW + off];  // R H W < 2^31
    return (T)s / (T)R;
}

// N frames' 16 bytes of one lane added into the packed sums: N unpredicated loads back to back, then the adds.  (Under a per-load
// `if (j < n)` every load sat in a basic block of its own behind a full wait: one read in flight per lane.)
template <int F, int N> __device__ __forceinline__ void add_frames(const uint8_t *__restrict__ vp, unsigned HW, unsigned sh, unsigned (&pk)[8 / F])
{
    static_assert(N >= 1 && N <= BATCH, "one batch at most");
    u32x4 x[N];
#pragma unroll
    for (int j = 0; j < N; j++)
        x[j] = *(const u32x4 *)(vp + (unsigned)j * HW);
#pragma unroll
    for (int j = 0; j < N; j++) {
#pragma unroll
        for (int d = 0; d < 4; d++) {
            if (F == 1) {
                pk[2 * d] += x[j][d] & 0x00ff00ffu;
                pk[2 * d + 1] += (x[j][d] >> 8) & 0x00ff00ffu;
            } else {
                pk[d] += (x[j][d] >> sh) & 0x00ff00ffu;
            }
        }
    }
}

// the sums over the R frames of the 16 / F wanted bytes of one aligned vector: s[k] is byte F k (+ 1 where sh = 8) of vp, frames HW apart
template <int F> __device__ __forceinline__ void packed_sums(const uint8_t *__restrict__ vp, unsigned HW, int R, unsigned sh, unsigned (&s)[16 / F])
{
    constexpr int NO = 16 / F;
#pragma unroll
    for (int k = 0; k < NO; k++)
        s[k] = 0;
    for (int r0 = 0; r0 < R; r0 += PACKED_MAX_R) {
        const int r1 = min(r0 + PACKED_MAX_R, R);
        unsigned pk[NO / 2];  // two 16-bit sums each
#pragma unroll
        for (int q = 0; q < NO / 2; q++)
            pk[q] = 0;
        int r = r0;
        for (; r + BATCH <= r1; r += BATCH)
            add_frames<F, BATCH>(vp + (unsigned)r * HW, HW, sh, pk);
        switch (r1 - r) {  // the rest, < BATCH frames: each count its own unpredicated run of loads (wave-uniform)
        case 1: add_frames<F, 1>(vp + (unsigned)r * HW, HW, sh, pk); break;
        case 2: add_frames<F, 2>(vp + (unsigned)r * HW, HW, sh, pk); break;
        case 3: add_frames<F, 3>(vp + (unsigned)r * HW, HW, sh, pk); break;
        case 4: add_frames<F, 4>(vp + (unsigned)r * HW, HW, sh, pk); break;
        case 5: add_frames<F, 5>(vp + (unsigned)r * HW, HW, sh, pk); break;
        case 6: add_frames<F, 6>(vp + (unsigned)r * HW, HW, sh, pk); break;
        case 7: add_frames<F, 7>(vp + (unsigned)r * HW, HW, sh, pk); break;
        default: break;
        }
        // field -> output: F = 1, dword d: pk[2d] = bytes 0, 2 and pk[2d + 1] = bytes 1, 3; F = 2: pk[d] = outputs 2d, 2d + 1
#pragma unroll
        for (int d = 0; d < 4; d++) {
            if (F == 1) {
                s[4 * d] += pk[2 * d] & 0xffffu;
                s[4 * d + 1] += pk[2 * d + 1] & 0xffffu;
                s[4 * d + 2] += pk[2 * d] >> 16;
                s[4 * d + 3] += pk[2 * d + 1] >> 16;
            } else {
                s[2 * d] += pk[d] & 0xffffu;
                s[2 * d + 1] += pk[d] >> 16;
            }
        }
    }
}

template <typename T, int F>
__global__ void __launch_bounds__(256) k_mean_u8_vec(const uint8_t *__restrict__ in, int R, int H, int W, int py, int px, int h, int w,
                                                     T *__restrict__ out)
{
    typedef typename Vec16<T>::type OV;
    constexpr int NO = 16 / F, OVN = Vec16<T>::N;  // outputs of one vector lane; T per 16-byte store
    const unsigned HW = (unsigned)H * W;
    const uint8_t *item = in + (size_t)blockIdx.z * R * HW;
    T *oitem = out + (size_t)blockIdx.z * h * w;
    const unsigned lane = blockIdx.y * 64 + threadIdx.x, lanes = gridDim.y * 64;
    for (unsigned i = blockIdx.x * 4 + threadIdx.y; i < (unsigned)h; i += gridDim.x * 4) {
        const unsigned off0 = (unsigned)(py + i * F) * W + px;  // frame 0's first wanted sample of this row
        const uint8_t *p = item + off0;
        T *orow = oitem + (size_t)i * w;
        const unsigned avail = W - px;                                // bytes from p to the end of the row
        const unsigned a0 = (16u - (unsigned)((uintptr_t)p & 15u)) & 15u;  // bytes from p to the first boundary
        const unsigned head = min((a0 + F - 1) / F, (unsigned)w);
        const unsigned nvec = avail > a0 ? (avail - a0) / 16u : 0u;   // whole vectors inside the row: NO wanted samples each
        const unsigned tail0 = head + nvec * NO, ntail = w - tail0;   // nvec == 0 and head < w: all of it is tail, < 16 outputs
        const unsigned sh = F == 2 ? 8u * (a0 & 1u) : 0u;             // F = 2: the wanted bytes of a dword are 0, 2 or 1, 3
        if (lane < head)
            orow[lane] = mean_one<T>(item, HW, R, off0 + lane * F);
        if (lane < ntail)
            orow[tail0 + lane] = mean_one<T>(item, HW, R, off0 + (tail0 + lane) * F);
        for (unsigned v = lane; v < nvec; v += lanes) {
            const uint8_t *vp = p + a0 + 16u * v;  // 16-byte aligned by construction, in every frame (HW % 16 == 0)
            unsigned s[NO];
            packed_sums<F>(vp, HW, R, sh, s);
            T *dst = orow + head + (size_t)v * NO;
            const T den = (T)R;
            if (((uintptr_t)dst & 15u) == 0) {  // the lane's own check: 16-byte stores only here
#pragma unroll
                for (int k = 0; k < NO; k += OVN) {
                    OV o;
#pragma unroll
                    for (int e = 0; e < OVN; e++)
                        o[e] = (T)s[k + e] / den;
                    *(OV *)(dst + k) = o;
                }
            } else {
#pragma unroll
                for (int k = 0; k < NO; k++)
                    dst[k] = (T)s[k] / den;
            }
        }
    }
}

template <typename T>
__global__ void __launch_bounds__(256) k_mean_u8_any(const uint8_t *__restrict__ in, int R, int H, int W, int f, int py, int px, int h, int w,
                                                     T *__restrict__ out)
{
    const unsigned HW = (unsigned)H * W;
    const uint8_t *item = in + (size_t)blockIdx.z * R * HW;
    T *oitem = out + (size_t)blockIdx.z * h * w;
    for (unsigned i = blockIdx.x * 4 + threadIdx.y; i < (unsigned)h; i += gridDim.x * 4) {
        const unsigned off0 = (unsigned)(py + i * f) * W + px;
        for (unsigned j = blockIdx.y * 64 + threadIdx.x; j < (unsigned)w; j += gridDim.y * 64)
            oitem[(size_t)i * w + j] = mean_one<T>(item, HW, R, off0 + j * f);
    }
}

// the arguments are checked by the caller (srx_mean_u8)
template <typename T> static int mean_u8(const uint8_t *in, int B, int R, int H, int W, int f, int py, int px, T *out, hipStream_t st)
{
    const int h = (H - py - 1) / f + 1, w = (W - px - 1) / f + 1;  // ceil, without the overflow of H - py + f - 1 at a huge f
    const dim3 blk(64, 4);
    const unsigned gx = (unsigned)std::min((h - 1) / 4 + 1, MAX_ROW_BLOCKS);
    const bool vec = (f == 1 || f == 2) && ((size_t)H * W) % 16 == 0;
    if (vec) {
        // lanes of a row: its vectors (at most W / 16), and 16 for the head and the tail
        const dim3 grid(gx, (unsigned)std::min(cdiv(std::max(W / 16, 16), 64), MAX_COL_BLOCKS), B);
        if (f == 1)
            hipLaunchKernelGGL((k_mean_u8_vec<T, 1>), grid, blk, 0, st, in, R, H, W, py, px, h, w, out);
        else
            hipLaunchKernelGGL((k_mean_u8_vec<T, 2>), grid, blk, 0, st, in, R, H, W, py, px, h, w, out);
    } else {
        const dim3 grid(gx, (unsigned)std::min((w - 1) / 64 + 1, MAX_COL_BLOCKS), B);
        hipLaunchKernelGGL(k_mean_u8_any<T>, grid, blk, 0, st, in, R, H, W, f, py, px, h, w, out);
    }
    SRX_CHECK_LAUNCH();
    return SRX_OK;
}

}  // namespace mean
}  // namespace srx
