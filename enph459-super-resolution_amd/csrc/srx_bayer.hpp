// srx_bayer.hpp -- colour from raw RGGB frames (include/srx_bayer.h): the four Bayer planes of a frame in one pass, and four reconstructed
// planes laid over each other as an RGB image.  Plane p = 0..3 is R, G1, G2, B: raw[py::2, px::2] with (py, px) = (p >> 1, p & 1).
//
//   k_bayer_split<T>         raw [B, H, W] -> planes [B, 4, H/2, W/2], an index map: one 2 x 2 raw cell per lane, four stores.
//   k_bayer_mean_vec<T>      uint8 raw [B, R, H, W] -> T planes, the mean over R; H W a multiple of 16.  k_mean_u8_vec's cut of a row (scalar
//                            head up to the row's first 16-byte boundary, aligned vectors, scalar tail) on EVERY raw row, and both column
//                            parities kept: mean::packed_sums<1> gives the 16 sums of a vector, the even ones are 8 consecutive outputs of one
//                            of the row's two planes and the odd ones 8 of the other.  The raw stack is read once.
//   k_bayer_mean_any<T>      every other shape: one raw sample per lane, R byte loads.
//   k_bayer_merge<T, RGB8>   planes [B, 4, Hp, Wp] -> rgb T [B, 3, Hp, Wp] or uint8 [B, Hp, Wp, 3]: G1 and B read d samples to the left, G2 and B
//                            d samples up, clamped at the edge; G = (g1 + g2) * 0.5; one multiplication by the channel's gain.
// srx_png_file_rgb8 has no kernel of its own: the scanlines of [H, W, 3] bytes under the Up filter are those of a grey image of width 3 W, so
// it is crc::png_file at that width with a truecolour IHDR.
#pragma once
#include <algorithm>
#include "srx_bayer.h"
#include "srx_common.h"
#include "srx_crc.hpp"
#include "srx_mean.hpp"
#include "srx_prims.hpp"

namespace srx {
namespace bayer {

constexpr int MAX_ROW_BLOCKS = mean::MAX_ROW_BLOCKS, MAX_COL_BLOCKS = 1024;  // grid caps; the lanes loop beyond them

template <typename T>
__global__ void __launch_bounds__(256) k_bayer_split(const T *__restrict__ in, int h, int w, T *__restrict__ out)
{
    const size_t n = (size_t)h * w, W = 2 * (size_t)w;
    const T *item = in + (size_t)blockIdx.z * 4 * n;
    T *oitem = out + (size_t)blockIdx.z * 4 * n;
    for (unsigned i = blockIdx.x * 4 + threadIdx.y; i < (unsigned)h; i += gridDim.x * 4) {
        for (unsigned j = blockIdx.y * 64 + threadIdx.x; j < (unsigned)w; j += gridDim.y * 64) {
            const T *r0 = item + 2 * (size_t)i * W + 2 * (size_t)j, *r1 = r0 + W;
            T *o = oitem + (size_t)i * w + j;
            const T a = r0[0], b = r0[1], c = r1[0], d = r1[1];
            o[0] = a, o[n] = b, o[2 * n] = c, o[3 * n] = d;
        }
    }
}

// eight outputs s[K0], s[K0 + 2], ... / den to dst: 16-byte stores where the lane finds dst aligned, one by one otherwise
template <typename T, int K0> __device__ __forceinline__ void store_every_other(T *dst, const unsigned (&s)[16], T den)
{
    typedef typename mean::Vec16<T>::type OV;
    constexpr int OVN = mean::Vec16<T>::N;
    if (((uintptr_t)dst & 15u) == 0) {
#pragma unroll
        for (int k = 0; k < 8; k += OVN) {
            OV o;
#pragma unroll
            for (int e = 0; e < OVN; e++)
                o[e] = (T)s[K0 + 2 * (k + e)] / den;
            *(OV *)(dst + k) = o;
        }
    } else {
#pragma unroll
        for (int k = 0; k < 8; k++)
            dst[k] = (T)s[K0 + 2 * k] / den;
    }
}

template <typename T>
__global__ void __launch_bounds__(256) k_bayer_mean_vec(const uint8_t *__restrict__ in, int R, int H, int W, T *__restrict__ out)
{
    const unsigned HW = (unsigned)H * W, w = (unsigned)W / 2, n = HW / 4;  // n: samples of one plane
    const uint8_t *item = in + (size_t)blockIdx.z * R * HW;
    T *oitem = out + (size_t)blockIdx.z * HW;
    const unsigned lane = blockIdx.y * 64 + threadIdx.x, lanes = gridDim.y * 64;
    const T den = (T)R;
    for (unsigned y = blockIdx.x * 4 + threadIdx.y; y < (unsigned)H; y += gridDim.x * 4) {
        const unsigned off0 = y * W;
        const uint8_t *p = item + off0;  // frame 0's row; the same address mod 16 in every frame (HW % 16 == 0)
        T *o0 = oitem + (size_t)(2 * (y & 1)) * n + (size_t)(y >> 1) * w, *o1 = o0 + n;  // the row's two planes: px = 0 and px = 1
        const unsigned a0 = (16u - (unsigned)((uintptr_t)p & 15u)) & 15u;  // bytes from p to the first boundary
        const unsigned head = min(a0, (unsigned)W);
        const unsigned nvec = (unsigned)W > a0 ? ((unsigned)W - a0) / 16u : 0u;
        const unsigned tail0 = head + nvec * 16u, ntail = (unsigned)W - tail0;  // < 16 raw samples each, one per lane
        if (lane < head)
            ((lane & 1u) ? o1 : o0)[lane >> 1] = mean::mean_one<T>(item, HW, R, off0 + lane);
        if (lane < ntail) {
            const unsigned c = tail0 + lane;
            ((c & 1u) ? o1 : o0)[c >> 1] = mean::mean_one<T>(item, HW, R, off0 + c);
        }
        for (unsigned v = lane; v < nvec; v += lanes) {
            const unsigned c0 = a0 + 16u * v;  // the raw column of the vector's byte 0; its parity is a0's
            unsigned s[16];
            mean::packed_sums<1>(p + c0, HW, R, 0u, s);
            // bytes 0, 2, ... are columns c0, c0 + 2, ...: outputs c0 >> 1 ... of the plane of c0's parity; bytes 1, 3, ... the other plane's
            store_every_other<T, 0>(((c0 & 1u) ? o1 : o0) + (c0 >> 1), s, den);
            store_every_other<T, 1>(((c0 & 1u) ? o0 : o1) + ((c0 + 1u) >> 1), s, den);
        }
    }
}

template <typename T>
__global__ void __launch_bounds__(256) k_bayer_mean_any(const uint8_t *__restrict__ in, int R, int H, int W, T *__restrict__ out)
{
    const unsigned HW = (unsigned)H * W, w = (unsigned)W / 2, n = HW / 4;
    const uint8_t *item = in + (size_t)blockIdx.z * R * HW;
    T *oitem = out + (size_t)blockIdx.z * HW;
    for (unsigned y = blockIdx.x * 4 + threadIdx.y; y < (unsigned)H; y += gridDim.x * 4)
        for (unsigned x = blockIdx.y * 64 + threadIdx.x; x < (unsigned)W; x += gridDim.y * 64)
            oitem[(size_t)(2 * (y & 1) + (x & 1)) * n + (size_t)(y >> 1) * w + (x >> 1)] = mean::mean_one<T>(item, HW, R, y * W + x);
}

__device__ __forceinline__ int clampi(int i, int n) { return min(max(i, 0), n - 1); }

template <typename T, bool RGB8>
__global__ void __launch_bounds__(256) k_bayer_merge(const T *__restrict__ planes, int Hp, int Wp, int d, bool gain, T gr, T gg, T gb,
                                                     void *__restrict__ out)
{
    const size_t n = (size_t)Hp * Wp;
    const T *P = planes + (size_t)blockIdx.z * 4 * n;
    for (int y = blockIdx.x * 4 + threadIdx.y; y < Hp; y += gridDim.x * 4) {
        const size_t row = (size_t)y * Wp, rowc = (size_t)clampi(y - d, Hp) * Wp;
        for (int x = blockIdx.y * 64 + threadIdx.x; x < Wp; x += gridDim.y * 64) {
            const int xc = clampi(x - d, Wp);
            T r = P[row + x];
            const T g1 = P[n + row + xc], g2 = P[2 * n + rowc + x];
            T b = P[3 * n + rowc + xc];
            T g = (g1 + g2) * (T)0.5;
            if (gain)
                r *= gr, g *= gg, b *= gb;
            if (RGB8) {
                uint8_t *o = (uint8_t *)out + ((size_t)blockIdx.z * n + row + x) * 3;
                o[0] = quantize_one(r), o[1] = quantize_one(g), o[2] = quantize_one(b);
            } else {
                T *o = (T *)out + (size_t)blockIdx.z * 3 * n + row + x;
                o[0] = r, o[n] = g, o[2 * n] = b;
            }
        }
    }
}

static inline dim3 grid_of(int rows, int cols, int B)
{
    return dim3((unsigned)std::min((rows - 1) / 4 + 1, MAX_ROW_BLOCKS), (unsigned)std::min((cols - 1) / 64 + 1, MAX_COL_BLOCKS), (unsigned)B);
}

template <typename T> static int split(const T *raw, int B, int H, int W, void *planes, hipStream_t st)
{
    if (!raw || !planes || B <= 0 || H <= 0 || W <= 0)
        return SRX_E_INVALID;
    if ((H & 1) || (W & 1) || (size_t)H * W * sizeof(T) >= ((size_t)1 << 31) || B > 65535)
        return SRX_E_UNSUPPORTED;
    hipLaunchKernelGGL(k_bayer_split<T>, grid_of(H / 2, W / 2, B), dim3(64, 4), 0, st, raw, H / 2, W / 2, (T *)planes);
    SRX_CHECK_LAUNCH();
    return SRX_OK;
}

template <typename T> static int mean_planes(const uint8_t *raw, int B, int R, int H, int W, T *planes, hipStream_t st)
{
    if (((size_t)H * W) % 16 == 0)  // lanes of a row: its vectors (at most W / 16), and 16 for the head and the tail
        hipLaunchKernelGGL(k_bayer_mean_vec<T>, grid_of(H, std::max(W / 16, 16), B), dim3(64, 4), 0, st, raw, R, H, W, planes);
    else
        hipLaunchKernelGGL(k_bayer_mean_any<T>, grid_of(H, W, B), dim3(64, 4), 0, st, raw, R, H, W, planes);
    SRX_CHECK_LAUNCH();
    return SRX_OK;
}

static int mean_u8(const uint8_t *raw, int B, int R, int H, int W, int out_elem_bytes, void *planes, hipStream_t st)
{
    if (!raw || !planes || B <= 0 || R <= 0 || H <= 0 || W <= 0 || (out_elem_bytes != 4 && out_elem_bytes != 8))
        return SRX_E_INVALID;
    if ((H & 1) || (W & 1) || R > 65535 || B > 65535 || (size_t)R * H * W >= ((size_t)1 << 31))
        return SRX_E_UNSUPPORTED;
    return out_elem_bytes == 4 ? mean_planes<float>(raw, B, R, H, W, (float *)planes, st) : mean_planes<double>(raw, B, R, H, W, (double *)planes, st);
}

template <typename T, bool RGB8> static int merge(const T *planes, int B, int Hp, int Wp, int d, const double *gains, void *out, hipStream_t st)
{
    if (!planes || !out || B <= 0 || Hp <= 0 || Wp <= 0 || d < 0)
        return SRX_E_INVALID;
    if ((size_t)Hp * Wp * sizeof(T) >= ((size_t)1 << 31) || B > 65535)
        return SRX_E_UNSUPPORTED;
    const T gr = gains ? (T)gains[0] : (T)1, gg = gains ? (T)gains[1] : (T)1, gb = gains ? (T)gains[2] : (T)1;
    hipLaunchKernelGGL((k_bayer_merge<T, RGB8>), grid_of(Hp, Wp, B), dim3(64, 4), 0, st, planes, Hp, Wp, d, gains != nullptr, gr, gg, gb, out);
    SRX_CHECK_LAUNCH();
    return SRX_OK;
}

// the width in bytes of a scanline of W RGB pixels, or 0 where it does not fit the grey calls' int
static inline int rgb_width(int W) { return W > 0 && (size_t)W * 3 <= (size_t)INT32_MAX ? 3 * W : 0; }

static inline size_t png_bound(int H, int W) { return crc::file_bound(H, rgb_width(W)); }

static inline size_t png_scratch_bytes(int B, int H, int W) { return crc::file_scratch_bytes(B, H, rgb_width(W)); }

static int png_file(const uint8_t *img, int B, int H, int W, void *files, void *lengths, void *ws, size_t wsb, hipStream_t st)
{
    if (!img || !files || !lengths || B <= 0 || H <= 0 || W <= 0)
        return SRX_E_INVALID;
    if (!rgb_width(W))
        return SRX_E_UNSUPPORTED;
    return crc::png_file(img, B, H, rgb_width(W), files, lengths, ws, wsb, st, W, 2);
}

}  // namespace bayer
}  // namespace srx
