// srx_patches.hpp -- a frame cut into overlapping patches and patches blended back into a frame (srx_patches_gather_* / srx_patches_blend_*):
// the two index maps between ONE image and the batch of patches that the per-item entry points (srx_saa_items_* / srx_ibp_items_*)
// reconstruct, each patch under its own shift table.
//
// Grid rule, per axis of n samples, patch length L, stride s (L <= n, L / 2 <= s <= L):
//   count     = ceil((n - L) / s) + 1
//   origin(i) = min(i s, n - L)            the last patch is pulled inward, never padded: every patch is L real samples
// Patch p = iy count_x + ix; batch item b of the frames owns items [b P, (b + 1) P).
//
// Blend weight of patch i at coordinate x inside it, with R = L - s - 2 margin >= 1 (the part of an overlap that is ramp):
//   dl = x - o_i + 1 - margin  if o_i > 0      else R       (no ramp at an edge of the image)
//   dr = o_i + L - x - margin  if o_i + L < n  else R
//   w  = clamp(min(dl, dr), 0, R)
// an integer: 0 over the outer `margin` samples of a patch (where a patch's reconstruction feels its own border), a ramp of R steps, R
// inside.  Pixel weight wy wx; out = sum (T)(wy_i wx_j) v_ij / (T)(Sy Sx), Sy = sum_i wy_i, Sx = sum_j wx_j.  The integer product is
// converted once, each term rounded once, the terms added in ascending (i, j) with plain additions, one division: product and sum stand
// in separate statements, so -ffp-contract=on fuses nothing and numpy reproduces the bits.  A term of weight 0 is not read.
// With 2 s >= L at most two unclamped patches and the clamped last one cover a sample: 3 per axis, and their indices are consecutive.
//
// The grid and weight functions are __host__ __device__ and free of HIP types: tests/patchwise_host_model.cpp includes this header with
// SRX_PATCHES_HOST_ONLY and runs the blend as a host loop under the sanitizers.
//
//   k_patches_gather<T>  a row = one row of one frame of one patch (pw samples); a group of 2^k lanes works on it -- as many as it has
//                 16-byte vectors, at most 64 (a 128-byte uint8 row: 8 lanes, 32 rows per block pass) -- and takes GATHER_ROWS rows, a
//                 block the rows of one chunk of one item.  A row whose source and destination both sit on a 16-byte boundary and whose
//                 length is whole vectors goes as vectors; every other row sample by sample.  The test is the row's own: neither the
//                 caller's pointers nor w need any alignment.
//   k_patches_blend<T>   one lane = 16 bytes (4 float / 2 double) of BLEND_ROWS consecutive output rows: the patches over its columns and
//                 their weights are found once, those over a row once per row (the same for a whole wave).  Where the samples of a lane
//                 share their covering patches and the lane finds the output and every patch row 16-byte aligned, it reads and stores
//                 vectors; otherwise it goes sample by sample.  Every output sample is written exactly once; nothing else is.
//                 (blend_one below is the same sum for one sample, the form the host model runs.)
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define SRX_PATCHES_HD __host__ __device__
#else
#define SRX_PATCHES_HD
#endif

namespace srx {
namespace patches {

constexpr int MAX_COVER = 3;  // patches over one sample, per axis (2 s >= L)

// the arguments of one axis no call accepts: 0; otherwise the number of patches
SRX_PATCHES_HD inline int grid_count(int n, int L, int s)
{
    if (n <= 0 || L <= 0 || L > n || s <= 0 || s > L || 2 * (long long)s < L)
        return 0;
    return (int)(((long long)(n - L) + s - 1) / s) + 1;
}

SRX_PATCHES_HD inline int grid_origin(int i, int n, int L, int s)
{
    const long long o = (long long)i * s;
    return o < (long long)(n - L) ? (int)o : n - L;
}

// weight of the patch at origin o at the image coordinate x, o <= x < o + L
SRX_PATCHES_HD inline int weight(int x, int o, int n, int L, int s, int margin)
{
    const int R = L - s - 2 * margin;
    const int dl = o > 0 ? x - o + 1 - margin : R;
    const int dr = o + L < n ? o + L - x - margin : R;
    const int d = dl < dr ? dl : dr;
    return d < 0 ? 0 : (d > R ? R : d);
}

// the patches over x: indices [*lo, *lo + returned count), their weights in w[], the weights' sum in *S
SRX_PATCHES_HD inline int cover(int x, int n, int L, int s, int margin, int count, int *lo, int (&w)[MAX_COVER], long long *S)
{
    int i0 = x >= L ? (x - L) / s + 1 : 0;
    if (i0 > count - 1)
        i0 = count - 1;
    int i1 = x / s;
    if (i1 > count - 1 || x >= n - L)
        i1 = count - 1;
    int c = 0;
    long long sum = 0;
    for (int i = i0; i <= i1 && c < MAX_COVER; i++, c++) {
        w[c] = weight(x, grid_origin(i, n, L, s), n, L, s, margin);
        sum += w[c];
    }
    for (int k = c; k < MAX_COVER; k++)
        w[k] = 0;
    *lo = i0;
    *S = sum;
    return c;
}

// one term into the sum, and the one division: separate statements, nothing to contract
template <typename T> SRX_PATCHES_HD inline T add_term(T acc, long long wgt, T v)
{
    const T t = (T)wgt * v;
    return acc + t;
}

template <typename T> SRX_PATCHES_HD inline T finish(T acc, long long Sy, long long Sx) { return acc / (T)(Sy * Sx); }

struct BlendGeom {
    int H, W, PH, PW, SY, SX, margin, cy, cx;
};

// one output sample the plain way: item = the P patches of this image
template <typename T> SRX_PATCHES_HD inline T blend_one(const T *item, const BlendGeom &g, int y, int x)
{
    int iy0, jx0, wy[MAX_COVER], wx[MAX_COVER];
    long long Sy, Sx;
    const int ny = cover(y, g.H, g.PH, g.SY, g.margin, g.cy, &iy0, wy, &Sy);
    const int nx = cover(x, g.W, g.PW, g.SX, g.margin, g.cx, &jx0, wx, &Sx);
    T acc = (T)0;
    for (int a = 0; a < ny; a++) {
        if (wy[a] == 0)
            continue;
        const int oy = grid_origin(iy0 + a, g.H, g.PH, g.SY);
        for (int c = 0; c < nx; c++) {
            if (wx[c] == 0)
                continue;
            const int ox = grid_origin(jx0 + c, g.W, g.PW, g.SX);
            const size_t p = (size_t)(iy0 + a) * g.cx + (jx0 + c);
            acc = add_term<T>(acc, (long long)wy[a] * wx[c], item[(p * g.PH + (size_t)(y - oy)) * g.PW + (size_t)(x - ox)]);
        }
    }
    return finish<T>(acc, Sy, Sx);
}

}  // namespace patches
}  // namespace srx

#if defined(__HIPCC__) && !defined(SRX_PATCHES_HOST_ONLY)
#include <algorithm>
#include "srx_common.h"

namespace srx {
namespace patches {

constexpr unsigned MAX_BLOCKS = 1u << 20;  // grid cap: the blocks loop beyond it
constexpr int GATHER_ROWS = 4;             // rows of one lane group in k_patches_gather
constexpr int BLEND_ROWS = 8;              // output rows of one lane in k_patches_blend

template <typename T> struct Vec16;
template <> struct Vec16<uint8_t> {
    typedef unsigned type __attribute__((ext_vector_type(4)));
    static constexpr int N = 16;
};
template <> struct Vec16<float> {
    typedef float type __attribute__((ext_vector_type(4)));
    static constexpr int N = 4;
};
template <> struct Vec16<double> {
    typedef double type __attribute__((ext_vector_type(2)));
    static constexpr int N = 2;
};

// nblk = items * chunks blocks of work; a chunk is GATHER_ROWS * (256 >> lg) rows of an item's N ph rows, 1 << lg lanes on a row
template <typename T>
__global__ void __launch_bounds__(256) k_patches_gather(const T *__restrict__ frames, size_t nblk, unsigned chunks, int lg, int N, int h, int w, int ph,
                                                        int pw, int sy, int sx, int cy, int cx, T *__restrict__ out)
{
    typedef typename Vec16<T>::type V;
    constexpr int VN = Vec16<T>::N;
    const unsigned lpr = 1u << lg, rpb = 256u >> lg;
    const unsigned lane = threadIdx.x & (lpr - 1), rsub = threadIdx.x >> lg;
    const unsigned rows_item = (unsigned)N * ph;  // N h w < 2^31
    const size_t P = (size_t)cy * cx;
    for (size_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
        const size_t item = blk / chunks;
        const unsigned chunk = (unsigned)(blk % chunks);
        const size_t b = item / P;
        const unsigned p = (unsigned)(item % P);
        const int oy = grid_origin(p / cx, h, ph, sy), ox = grid_origin(p % cx, w, pw, sx);
        const T *src0 = frames + (b * N * h + (size_t)oy) * w + ox;
        T *dst0 = out + item * rows_item * pw;
#pragma unroll
        for (int u = 0; u < GATHER_ROWS; u++) {
            const unsigned rr = (chunk * GATHER_ROWS + u) * rpb + rsub;  // the row inside the item: frame k, row r
            if (rr >= rows_item)
                continue;
            const unsigned k = rr / ph, r = rr % ph;
            const T *src = src0 + ((size_t)k * h + r) * w;
            T *dst = dst0 + (size_t)rr * pw;
            if (pw % VN == 0 && (((uintptr_t)src | (uintptr_t)dst) & 15u) == 0) {  // the row's own check: vectors only here
                for (unsigned v = lane; v < (unsigned)(pw / VN); v += lpr)
                    ((V *)dst)[v] = ((const V *)src)[v];
            } else {
                for (unsigned c = lane; c < (unsigned)pw; c += lpr)
                    dst[c] = src[c];
            }
        }
    }
}

// A lane owns 16 bytes of BLEND_ROWS consecutive output rows: the patches over its columns and their weights are found once, those over a
// row once per row (the same for the whole wave).
template <typename T>
__global__ void __launch_bounds__(256) k_patches_blend(const T *__restrict__ patches, size_t row_blocks, unsigned col_blocks, BlendGeom g,
                                                       T *__restrict__ out)
{
    typedef typename Vec16<T>::type V;
    constexpr int VN = Vec16<T>::N;
    const size_t P = (size_t)g.cy * g.cx, rb_per_image = (size_t)cdiv(g.H, 4 * BLEND_ROWS);
    const size_t total = row_blocks * col_blocks;
    for (size_t blk = blockIdx.x; blk < total; blk += gridDim.x) {
        const size_t rb = blk / col_blocks;
        const unsigned cb = (unsigned)(blk % col_blocks);
        const size_t b = rb / rb_per_image;
        const int ybase = ((int)(rb % rb_per_image) * 4 + (int)threadIdx.y) * BLEND_ROWS;
        const long long x0l = ((long long)cb * 64 + threadIdx.x) * VN;
        if (ybase >= g.H || x0l >= g.W)
            continue;
        const int x0 = (int)x0l;
        const T *item = patches + b * P * g.PH * g.PW;
        const int nvalid = g.W - x0 < VN ? g.W - x0 : VN;
        // the columns: per sample its patches [jx0, jx0 + nx) and weights
        int jx0[VN], nx[VN], wx[VN][MAX_COVER];
        long long Sx[VN];
#pragma unroll
        for (int e = 0; e < VN; e++) {
            jx0[e] = nx[e] = 0;
            Sx[e] = 1;
            if (e < nvalid)
                nx[e] = cover(x0 + e, g.W, g.PW, g.SX, g.margin, g.cx, &jx0[e], wx[e], &Sx[e]);
        }
        // vectors: the lane's samples share their patches, and every patch row starts 16-byte aligned at the lane's first sample
        bool xvec = nvalid == VN && g.PW % VN == 0 && ((uintptr_t)item & 15u) == 0;
#pragma unroll
        for (int e = 1; e < VN; e++)
            xvec = xvec && jx0[e] == jx0[0] && nx[e] == nx[0];
        int ox[MAX_COVER];
#pragma unroll
        for (int c = 0; c < MAX_COVER; c++) {
            ox[c] = grid_origin(jx0[0] + c < g.cx ? jx0[0] + c : g.cx - 1, g.W, g.PW, g.SX);
            if (c < nx[0])
                xvec = xvec && (x0 - ox[c]) % VN == 0;
        }
        for (int r = 0; r < BLEND_ROWS; r++) {
            const int y = ybase + r;
            if (y >= g.H)
                break;
            int iy0, wy[MAX_COVER];
            long long Sy;
            const int ny = cover(y, g.H, g.PH, g.SY, g.margin, g.cy, &iy0, wy, &Sy);
            T *orow = out + (b * g.H + (size_t)y) * g.W;
            if (xvec && ((uintptr_t)(orow + x0) & 15u) == 0) {
                T acc[VN];
#pragma unroll
                for (int e = 0; e < VN; e++)
                    acc[e] = (T)0;
                for (int a = 0; a < ny; a++) {
                    if (wy[a] == 0)
                        continue;
                    const int oy = grid_origin(iy0 + a, g.H, g.PH, g.SY);
                    for (int c = 0; c < nx[0]; c++) {
                        bool any = false;
#pragma unroll
                        for (int e = 0; e < VN; e++)
                            any = any || wx[e][c] != 0;
                        if (!any)
                            continue;
                        const size_t p = (size_t)(iy0 + a) * g.cx + (jx0[0] + c);
                        const V v = *(const V *)(item + (p * g.PH + (size_t)(y - oy)) * g.PW + (size_t)(x0 - ox[c]));
#pragma unroll
                        for (int e = 0; e < VN; e++)
                            if (wx[e][c] != 0)
                                acc[e] = add_term<T>(acc[e], (long long)wy[a] * wx[e][c], v[e]);
                    }
                }
                V o;
#pragma unroll
                for (int e = 0; e < VN; e++)
                    o[e] = finish<T>(acc[e], Sy, Sx[e]);
                *(V *)(orow + x0) = o;
                continue;
            }
#pragma unroll
            for (int e = 0; e < VN; e++) {  // sample by sample
                if (e >= nvalid)
                    continue;
                T acc = (T)0;
                for (int a = 0; a < ny; a++) {
                    if (wy[a] == 0)
                        continue;
                    const int oy = grid_origin(iy0 + a, g.H, g.PH, g.SY);
                    for (int c = 0; c < nx[e]; c++) {
                        if (wx[e][c] == 0)
                            continue;
                        const int oxe = grid_origin(jx0[e] + c, g.W, g.PW, g.SX);
                        const size_t p = (size_t)(iy0 + a) * g.cx + (jx0[e] + c);
                        acc = add_term<T>(acc, (long long)wy[a] * wx[e][c], item[(p * g.PH + (size_t)(y - oy)) * g.PW + (size_t)(x0 + e - oxe)]);
                    }
                }
                orow[x0 + e] = finish<T>(acc, Sy, Sx[e]);
            }
        }
    }
}

// refusals shared by both calls, in srx.h's order; `eb` bytes per sample; gather: N frames of h x w, blend: N = 1 plane of H x W
static inline int check_grid(bool null_ptr, int B, int N, int h, int w, int ph, int pw, int sy, int sx, int margin, bool blend, size_t eb)
{
    if (null_ptr || B <= 0 || N <= 0 || h <= 0 || w <= 0 || ph <= 0 || ph > h || pw <= 0 || pw > w || sy <= 0 || sy > ph || sx <= 0 || sx > pw)
        return SRX_E_INVALID;
    if (blend && (margin < 0 || (long long)ph - sy - 2LL * margin < 1 || (long long)pw - sx - 2LL * margin < 1))
        return SRX_E_INVALID;
    const size_t lim = (size_t)1 << 31, hw = (size_t)h * w;  // (every product below stays under 2^64)
    if (2LL * sy < ph || 2LL * sx < pw || hw >= lim || hw * N >= lim || hw * N * eb >= lim)
        return SRX_E_UNSUPPORTED;
    const size_t P = (size_t)grid_count(h, ph, sy) * grid_count(w, pw, sx);
    if (P >= lim || (size_t)B * P >= lim)
        return SRX_E_UNSUPPORTED;
    return SRX_OK;
}

template <typename T>
static int gather(const T *frames, int B, int N, int h, int w, int ph, int pw, int sy, int sx, void *out, hipStream_t st)
{
    SRX_TRY(check_grid(!frames || !out, B, N, h, w, ph, pw, sy, sx, 0, false, sizeof(T)));
    const int cy = grid_count(h, ph, sy), cx = grid_count(w, pw, sx);
    // lanes on a row: its 16-byte vectors (its samples where it has no whole vectors), as a power of two of at most 64
    const int per_row = pw % Vec16<T>::N == 0 ? pw / Vec16<T>::N : pw;
    int lg = 0;
    while (lg < 6 && (1 << lg) < per_row)
        lg++;
    const unsigned rows_chunk = (unsigned)GATHER_ROWS * (256u >> lg);
    const unsigned chunks = (unsigned)(((size_t)N * ph + rows_chunk - 1) / rows_chunk);
    const size_t nblk = (size_t)B * cy * cx * chunks;
    const unsigned grid = (unsigned)std::min<size_t>(nblk, MAX_BLOCKS);
    hipLaunchKernelGGL(k_patches_gather<T>, dim3(grid), dim3(256), 0, st, frames, nblk, chunks, lg, N, h, w, ph, pw, sy, sx, cy, cx, (T *)out);
    SRX_CHECK_LAUNCH();
    return SRX_OK;
}

template <typename T>
static int blend(const T *patches, int B, int H, int W, int PH, int PW, int SY, int SX, int margin, void *out, hipStream_t st)
{
    SRX_TRY(check_grid(!patches || !out, B, 1, H, W, PH, PW, SY, SX, margin, true, sizeof(T)));
    const BlendGeom g{H, W, PH, PW, SY, SX, margin, grid_count(H, PH, SY), grid_count(W, PW, SX)};
    const size_t row_blocks = (size_t)B * cdiv(H, 4 * BLEND_ROWS);
    const unsigned col_blocks = (unsigned)cdiv(cdiv(W, Vec16<T>::N), 64);
    const unsigned grid = (unsigned)std::min<size_t>(row_blocks * col_blocks, MAX_BLOCKS);
    hipLaunchKernelGGL(k_patches_blend<T>, dim3(grid), dim3(64, 4), 0, st, patches, row_blocks, col_blocks, g, (T *)out);
    SRX_CHECK_LAUNCH();
    return SRX_OK;
}

}  // namespace patches
}  // namespace srx
#endif
