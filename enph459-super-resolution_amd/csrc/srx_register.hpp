// srx_register.hpp -- sub-pixel frame registration on the device (translation only): d_k with frames[k] ~ ndi.shift(frames[ref], d_k),
// the sign convention of shifts_yx.  Every sum runs over the reference crop [m, H - m) x [m, W - m), m = border + search + 2.
//
//   prefilter   each moving frame once into cubic B-spline coefficients with scipy's 'nearest' edges (12-sample edge pad + the
//               'reflect' recursion: k_reg_pad + prefilter2d), [B (N - 1)][H + 24][W + 24]
//   coarse      k_reg_coarse: one launch over every moving frame x crop strip.  A 64 x 16 chunk of the crop and the frame's
//               (64 + 2S) x (16 + 2S) window around it (S = search) are staged in LDS; thread (offset o, group g) accumulates
//               sum t, t^2, t r at offset o over the chunk pixels g, g + G, ... in float64.  k_reg_pick adds the strips in index
//               order, scores the zero-mean NCC of every offset and takes the argmax on the device (ties: smallest |dy| + |dx|,
//               then dy, then dx)
//   refine      Gauss-Newton, one k_reg_gn + one k_reg_solve per iteration and no host synchronisation.  The shift is the same for
//               every pixel of a frame, so the 4 + 4 B-spline taps and their derivative taps are formed once per block from the
//               current estimate in device memory.  Each thread walks one crop column down a strip with the horizontally filtered
//               coefficient rows (value and x-derivative) in a 4-row register ring: 4 coefficient loads and one reference load
//               per pixel, w = t(i + d) and (gy, gx) formed on the fly, no plane written.  Sums (8 per frame) are fixed-order
//               float64 (block partials, then one wave in index order): bit-identical run to run, no atomics.  k_reg_solve solves
//               the 2 x 2 normal equations, clamps the step to +-0.5 px and freezes the frame once max |step| < tol or after n_iter
//               steps; a singular matrix (det <= 1e-6 trace^2, or trace <= 1e-10 sum w^2) restores the coarse shift.
//   finish      one more k_reg_gn pass at the final shifts gives the score (zero-mean NCC, what metrics.ecc gives for the crop);
//               k_reg_finish writes shifts / score / status, the reference rows exactly (0, 0), 1, 0.
//
// uint8 frames (srx_register_u8_*: F = uint8_t, T the type of the coefficients and of the arithmetic) run the same launches on the same
// grids and return the bits of the float call on the converted frames.  (T)uint8 is exact, so k_reg_pad writes the float call's plane and
// k_reg_gn reads the float call's reference samples.  The coarse stage is k_reg_coarse_u8, in integers: samples are <= 255 and a crop has
// fewer than 2^29 pixels (a plane is below 2 GiB even as float), so sum t, t^2, t r, r, r^2 are all below 2^29 255^2 < 2^45 -- integers a
// float64 holds exactly, with every partial sum of them.  The float kernel's float64 sums are therefore those integers whatever the order,
// and the integer kernel's, converted to double per block, are the same `part` words; k_reg_pick reads them unchanged.
#pragma once
#include "srx_common.h"
#include "srx_metrics.hpp"
#include "srx_prims.hpp"

namespace srx {
namespace reg {

constexpr int MAX_SEARCH = 4;
constexpr int CW = 64, CH = 16;            // coarse chunk: 64 x 16 crop pixels
constexpr int CBLK = 256;                  // coarse blocks per frame (target)
constexpr int GW = 256;                    // refinement strip width (one column per thread)
constexpr int GBLK = 256;                  // refinement blocks per frame (target)
constexpr int NG = 8;                      // refinement sums: gy gy, gy gx, gx gx, gy e, gx e, w, w w, w r
constexpr int MIN_CROP = 16;
constexpr double VAR_EPS = 1e-10, DET_EPS = 1e-6, GRAD_EPS = 1e-10;

enum { ST_OK = 0, ST_SINGULAR = 1, ST_BOUNDARY = 2, ST_NOT_CONVERGED = 3 };

// per moving frame: d (current), dc (coarse), sum r, sum r^2, n, last |step|
constexpr int SD = 8;
enum { S_DY = 0, S_DX, S_CY, S_CX, S_SR, S_SRR, S_N, S_LAST };
// ints per moving frame: steps, frozen, singular, on boundary
constexpr int SI = 4;
enum { I_STEPS = 0, I_FROZEN, I_SINGULAR, I_EDGE };

struct Geo {
    int B, N, H, W, ref, m, h, w;  // crop h x w at (m, m)
    __host__ __device__ int nf() const { return B * (N - 1); }
    // moving frame f = b (N - 1) + j -> frame index k of item b
    __host__ __device__ int moving(int f) const
    {
        const int j = f % (N - 1);
        return j < ref ? j : j + 1;
    }
    __device__ size_t plane(int f) const { return (size_t)(f / (N - 1)) * N + moving(f); }
    __device__ size_t ref_plane(int f) const { return (size_t)(f / (N - 1)) * N + ref; }
};

// integer start of frame k: rint(init_k - init_ref) (by value: the caller's init is a host array)
struct Start {
    int c[SRX_MAX_FRAMES][2];
};

struct Plan {
    int noff, nv;       // offsets, coarse sums per block (3 noff + 2)
    int cgx, cgy, crow; // coarse grid per frame and rows per block
    int ggx, ggy, grow; // refinement grid per frame and rows per block
};

// block counts per frame never exceed these for a crop of width <= w (cgy <= gy <= cdiv(CBLK, cgx), likewise for the refinement)
static inline int coarse_blocks_max(int w) { return CBLK + cdiv(w, CW); }
static inline int gn_blocks_max(int w) { return GBLK + cdiv(w, GW); }

// the decomposition depends on the crop only (never on B or N): a batch adds up every frame exactly as a single call does
static inline Plan make_plan(int h, int w, int search)
{
    Plan p;
    const int D = 2 * search + 1;
    p.noff = D * D, p.nv = 3 * p.noff + 2;
    p.cgx = cdiv(w, CW);
    int gy = std::max(1, std::min(cdiv(CBLK, p.cgx), cdiv(h, CH)));
    p.crow = cdiv(cdiv(h, gy), CH) * CH;
    p.cgy = cdiv(h, p.crow);
    p.ggx = cdiv(w, GW);
    gy = std::max(1, std::min(cdiv(GBLK, p.ggx), cdiv(h, 16)));
    p.grow = cdiv(h, gy);
    p.ggy = cdiv(h, p.grow);
    return p;
}

// ---- 'nearest' edge pad of the moving frames: [nf][H + 24][W + 24] ------------------------------------------------------------------
template <typename T, typename F>
__global__ void __launch_bounds__(256) k_reg_pad(const F *__restrict__ frames, Geo g, T *__restrict__ out)
{
    const int Hp = g.H + 2 * SRX_NPAD, Wp = g.W + 2 * SRX_NPAD;
    const int c = blockIdx.x * 64 + threadIdx.x, r = blockIdx.y * 4 + threadIdx.y, f = blockIdx.z;
    if (r >= Hp || c >= Wp)
        return;
    const int rr = min(max(r - SRX_NPAD, 0), g.H - 1), cc = min(max(c - SRX_NPAD, 0), g.W - 1);
    out[(size_t)f * Hp * Wp + (size_t)r * Wp + c] = (T)frames[g.plane(f) * g.H * g.W + (size_t)rr * g.W + cc];
}

// ---- coarse search, stage 1: grid (cgx, cgy, nf), block 256 ---------------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(256) k_reg_coarse(const T *__restrict__ frames, Geo g, int search, int rows_per, Start c0,
                                                    double *__restrict__ part)
{
    constexpr int TW = CW + 2 * MAX_SEARCH, TH = CH + 2 * MAX_SEARCH;
    __shared__ T sr[CH][CW];
    __shared__ T stl[TH][TW];
    __shared__ double red[256 * 3];  // [group][offset][3]: G noff <= 256
    __shared__ double redr[256][2];
    const int f = blockIdx.z, tid = threadIdx.x;
    const int D = 2 * search + 1, noff = D * D, G = 256 / noff;
    const int o = tid % noff, grp = tid / noff;  // grp == G: idle
    const int oy = o / D, ox = o - oy * D;       // offset + search
    const int x0 = blockIdx.x * CW, cols = min(CW, g.w - x0);
    const int y0 = blockIdx.y * rows_per, y1 = min(y0 + rows_per, g.h);
    const T *t = frames + g.plane(f) * g.H * g.W, *r = frames + g.ref_plane(f) * g.H * g.W;
    const int k = g.moving(f), cy = c0.c[k][0] - search, cx = c0.c[k][1] - search;
    double st = 0.0, stt = 0.0, str = 0.0, s_r = 0.0, s_rr = 0.0;
    const int tw = cols + 2 * search;
    for (int ya = y0; ya < y1; ya += CH) {
        const int rows = min(CH, y1 - ya), th = rows + 2 * search;
        __syncthreads();
        for (int i = tid; i < rows * CW; i += 256) {
            const int py = i / CW, px = i - py * CW;
            if (px < cols)
                sr[py][px] = r[(size_t)(g.m + ya + py) * g.W + g.m + x0 + px];
        }
        for (int i = tid; i < th * TW; i += 256) {
            const int py = i / TW, px = i - py * TW;
            if (px < tw) {
                const int yy = min(max(g.m + ya + py + cy, 0), g.H - 1), xx = min(max(g.m + x0 + px + cx, 0), g.W - 1);
                stl[py][px] = t[(size_t)yy * g.W + xx];
            }
        }
        __syncthreads();
        if (grp < G) {
            for (int p = grp; p < rows * CW; p += G) {
                const int py = p / CW, px = p - py * CW;
                if (px >= cols)
                    continue;
                const double rv = (double)sr[py][px], tv = (double)stl[py + oy][px + ox];
                st += tv, stt += tv * tv, str += tv * rv;
                if (o == 0)
                    s_r += rv, s_rr += rv * rv;
            }
        }
    }
    // the groups' sums, added in group order by thread o < noff
    __syncthreads();
    if (grp < G) {
        red[3 * tid] = st, red[3 * tid + 1] = stt, red[3 * tid + 2] = str;
        if (o == 0)
            redr[grp][0] = s_r, redr[grp][1] = s_rr;
    }
    __syncthreads();
    double *out = part + ((size_t)f * gridDim.x * gridDim.y + blockIdx.y * gridDim.x + blockIdx.x) * (3 * noff + 2);
    if (tid < noff) {
        double a0 = 0.0, a1 = 0.0, a2 = 0.0;
        for (int q = 0; q < G; q++) {
            const double *e = red + 3 * (q * noff + tid);
            a0 += e[0], a1 += e[1], a2 += e[2];
        }
        out[3 * tid] = a0, out[3 * tid + 1] = a1, out[3 * tid + 2] = a2;
    }
    if (tid == 0) {
        double b0 = 0.0, b1 = 0.0;
        for (int q = 0; q < G; q++)
            b0 += redr[q][0], b1 += redr[q][1];
        out[3 * noff] = b0, out[3 * noff + 1] = b1;
    }
}

// ---- coarse search, stage 1 on bytes: the same grid, blocks and `part` layout; the sums in integers ------------------------------------
// four consecutive samples p[0..3] of the frame stack [lo, hi) as one word (p[0] in bits 0-7), p on any byte: two aligned word loads and
// a byte align where both words lie inside the stack, byte loads at its two ends
__device__ __forceinline__ unsigned load4_u8(const uint8_t *p, const uint8_t *lo, const uint8_t *hi)
{
    const uintptr_t a = (uintptr_t)p, a0 = a & ~(uintptr_t)3;
    if (a0 >= (uintptr_t)lo && a0 + 8 <= (uintptr_t)hi) {
        const unsigned *q = (const unsigned *)a0;
        return __builtin_amdgcn_alignbyte(q[1], q[0], (unsigned)(a & 3));
    }
    return (unsigned)p[0] | (unsigned)p[1] << 8 | (unsigned)p[2] << 16 | (unsigned)p[3] << 24;
}

// The chunk and its window are staged as packed bytes, 16 words per chunk row and TWW = 19 per window row (64 + 2 * 4 bytes and the word
// the byte align reads behind them; 19 is odd, so the rows a wave's offsets read fall on different banks).  Thread (offset o, group g)
// takes the words g, g + G, ... of the chunk: the four moving samples at offset o come from two aligned LDS words and a byte align, and
// three dot4 add t, t t and t r of the four pixels.  r and r r are added by the thread that stages the reference word.  Samples right of a
// partial chunk are zero in the reference word and masked out of the moving word.
// Overflow: the 32-bit accumulators hold the products of ONE 64 x 16 chunk, at most 1024 * 255^2 < 2^27, and are added into 64-bit ones
// after every chunk; a block's 64-bit totals stay below 2^45 (head comment) and convert to double exactly.
__global__ void __launch_bounds__(256) k_reg_coarse_u8(const uint8_t *__restrict__ frames, Geo g, int search, int rows_per, Start c0,
                                                       double *__restrict__ part)
{
    constexpr int CWW = CW / 4, TWW = (CW + 2 * MAX_SEARCH) / 4 + 1, TH = CH + 2 * MAX_SEARCH;
    __shared__ unsigned sr[CH][CWW];
    __shared__ unsigned stl[TH][TWW];
    __shared__ unsigned long long red[256 * 3];  // [group][offset][3]: G noff <= 256
    __shared__ unsigned long long redr[4][2];    // [wave]
    const int f = blockIdx.z, tid = threadIdx.x;
    const int D = 2 * search + 1, noff = D * D, G = 256 / noff;
    const int o = tid % noff, grp = tid / noff;  // grp == G: idle
    const int oy = o / D, ox = o - oy * D;       // offset + search
    const int x0 = blockIdx.x * CW, cols = min(CW, g.w - x0), nw = (cols + 3) >> 2;
    const int y0 = blockIdx.y * rows_per, y1 = min(y0 + rows_per, g.h);
    const uint8_t *lo = frames, *hi = frames + (size_t)g.B * g.N * g.H * g.W;
    const uint8_t *t = frames + g.plane(f) * g.H * g.W, *r = frames + g.ref_plane(f) * g.H * g.W;
    const int k = g.moving(f), cy = c0.c[k][0] - search, cx = c0.c[k][1] - search;
    const int wsh = ox >> 2;
    const unsigned bsh = ox & 3;
    unsigned long long st = 0, stt = 0, str = 0, s_r = 0, s_rr = 0;
    for (int ya = y0; ya < y1; ya += CH) {
        const int rows = min(CH, y1 - ya), th = rows + 2 * search;
        __syncthreads();
        for (int i = tid; i < rows * CWW; i += 256) {
            const int py = i / CWW, wx = i - py * CWW, n = min(cols - 4 * wx, 4);  // samples of this word inside the crop
            const uint8_t *p = r + (size_t)(g.m + ya + py) * g.W + g.m + x0 + 4 * wx;
            unsigned v = 0;
            if (n == 4)
                v = load4_u8(p, lo, hi);
            else
                for (int b = 0; b < n; b++)
                    v |= (unsigned)p[b] << (8 * b);
            sr[py][wx] = v;
            s_r += __builtin_amdgcn_udot4(v, 0x01010101u, 0u, false), s_rr += __builtin_amdgcn_udot4(v, v, 0u, false);
        }
        for (int i = tid; i < th * TWW; i += 256) {
            const int py = i / TWW, wx = i - py * TWW;
            const int yy = min(max(g.m + ya + py + cy, 0), g.H - 1), xs = g.m + x0 + 4 * wx + cx;
            const uint8_t *p = t + (size_t)yy * g.W;
            unsigned v = 0;
            if (xs >= 0 && xs + 3 < g.W)
                v = load4_u8(p + xs, lo, hi);
            else
                for (int b = 0; b < 4; b++)
                    v |= (unsigned)p[min(max(xs + b, 0), g.W - 1)] << (8 * b);
            stl[py][wx] = v;
        }
        __syncthreads();
        if (grp < G) {
            unsigned a_t = 0, a_tt = 0, a_tr = 0;  // one chunk: < 2^27
            for (int q = grp; q < rows * CWW; q += G) {
                const int py = q / CWW, wx = q - py * CWW;
                if (wx >= nw)
                    continue;
                const unsigned rv = sr[py][wx];
                const unsigned *mw = &stl[py + oy][wx + wsh];
                unsigned tv = __builtin_amdgcn_alignbyte(mw[1], mw[0], bsh);
                const int n = cols - 4 * wx;
                if (n < 4)
                    tv &= (1u << (8 * n)) - 1u;
                a_t = __builtin_amdgcn_udot4(tv, 0x01010101u, a_t, false);
                a_tt = __builtin_amdgcn_udot4(tv, tv, a_tt, false);
                a_tr = __builtin_amdgcn_udot4(tv, rv, a_tr, false);
            }
            st += a_t, stt += a_tt, str += a_tr;
        }
    }
    // the groups' sums, added by thread o < noff; the reference's, by wave and then by thread 0
    s_r = wave_sum(s_r), s_rr = wave_sum(s_rr);
    __syncthreads();
    if (grp < G)
        red[3 * tid] = st, red[3 * tid + 1] = stt, red[3 * tid + 2] = str;
    if ((tid & 63) == 0)
        redr[tid >> 6][0] = s_r, redr[tid >> 6][1] = s_rr;
    __syncthreads();
    double *out = part + ((size_t)f * gridDim.x * gridDim.y + blockIdx.y * gridDim.x + blockIdx.x) * (3 * noff + 2);
    if (tid < noff) {
        unsigned long long a0 = 0, a1 = 0, a2 = 0;
        for (int q = 0; q < G; q++) {
            const unsigned long long *e = red + 3 * (q * noff + tid);
            a0 += e[0], a1 += e[1], a2 += e[2];
        }
        out[3 * tid] = (double)a0, out[3 * tid + 1] = (double)a1, out[3 * tid + 2] = (double)a2;
    }
    if (tid == 0) {
        unsigned long long b0 = 0, b1 = 0;
        for (int q = 0; q < 4; q++)
            b0 += redr[q][0], b1 += redr[q][1];
        out[3 * noff] = (double)b0, out[3 * noff + 1] = (double)b1;
    }
}

// the coarse kernel of frames of type F.  uint8 frames through the float kernel's structure with F = uint8_t in its loads and LDS planes
// instead is what k_reg_coarse_u8 was measured against (profiles/README.md).
template <typename F>
static inline void launch_coarse(const F *frames, const Geo &g, int search, const Plan &p, const Start &c0, double *part, hipStream_t st)
{
    hipLaunchKernelGGL(k_reg_coarse<F>, dim3(p.cgx, p.cgy, g.nf()), dim3(256), 0, st, frames, g, search, p.crow, c0, part);
}
template <>
inline void launch_coarse<uint8_t>(const uint8_t *frames, const Geo &g, int search, const Plan &p, const Start &c0, double *part, hipStream_t st)
{
    hipLaunchKernelGGL(k_reg_coarse_u8, dim3(p.cgx, p.cgy, g.nf()), dim3(256), 0, st, frames, g, search, p.crow, c0, part);
}

__device__ __forceinline__ double zm_ncc(double n, double st, double stt, double sr, double srr, double str)
{
    const double vt = stt - st * st / n, vr = srr - sr * sr / n;
    if (!(vt > VAR_EPS * stt) || !(vr > VAR_EPS * srr))
        return 0.0;
    return (str - st * sr / n) / sqrt(vt * vr);
}

// ---- coarse search, stage 2: grid nf, block 256: sums in block order, NCC per offset, argmax; initialises the refinement state -------
__global__ void __launch_bounds__(256) k_reg_pick(const double *__restrict__ part, int nblk, Geo g, int search, Start c0, double *__restrict__ sd,
                                                  int *__restrict__ si)
{
    constexpr int MAXV = 3 * (2 * MAX_SEARCH + 1) * (2 * MAX_SEARCH + 1) + 2;
    __shared__ double sum[MAXV];
    __shared__ double score[(2 * MAX_SEARCH + 1) * (2 * MAX_SEARCH + 1)];
    const int f = blockIdx.x, D = 2 * search + 1, noff = D * D, nv = 3 * noff + 2, k = g.moving(f);
    const double n = (double)g.h * g.w;
    for (int v = threadIdx.x; v < nv; v += 256) {
        double s = 0.0;
        for (int k = 0; k < nblk; k++)
            s += part[((size_t)f * nblk + k) * nv + v];
        sum[v] = s;
    }
    __syncthreads();
    if (threadIdx.x < noff) {
        const int o = threadIdx.x;
        score[o] = zm_ncc(n, sum[3 * o], sum[3 * o + 1], sum[3 * noff], sum[3 * noff + 1], sum[3 * o + 2]);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int best = 0, bdy = 0, bdx = 0;
        double bs = 0.0;
        for (int o = 0; o < noff; o++) {
            const int oy = o / D - search, ox = o % D - search;
            const int dy = c0.c[k][0] + oy, dx = c0.c[k][1] + ox;
            const double s = score[o];
            bool take = o == 0 || s > bs;
            if (!take && s == bs) {
                const int l = abs(dy) + abs(dx), bl = abs(bdy) + abs(bdx);
                take = l < bl || (l == bl && (dy < bdy || (dy == bdy && dx < bdx)));
            }
            if (take)
                best = o, bs = s, bdy = dy, bdx = dx;
        }
        const int oy = best / D - search, ox = best % D - search;
        double *s = sd + (size_t)f * SD;
        int *q = si + (size_t)f * SI;
        s[S_DY] = s[S_CY] = (double)bdy;
        s[S_DX] = s[S_CX] = (double)bdx;
        s[S_SR] = sum[3 * noff], s[S_SRR] = sum[3 * noff + 1], s[S_N] = n, s[S_LAST] = 0.0;
        q[I_STEPS] = 0, q[I_FROZEN] = 0, q[I_SINGULAR] = 0;
        q[I_EDGE] = search > 0 && (abs(oy) == search || abs(ox) == search);
    }
}

// cubic B-spline taps and derivative taps at fraction u, in double
__device__ __forceinline__ void taps_d(double u, double w[4], double dw[4])
{
    const double z = 1.0 - u;
    w[0] = z * z * z / 6.0;
    w[1] = (3.0 * u * u * u - 6.0 * u * u + 4.0) / 6.0;
    w[2] = (-3.0 * u * u * u + 3.0 * u * u + 3.0 * u + 1.0) / 6.0;
    w[3] = u * u * u / 6.0;
    dw[0] = -0.5 * z * z;
    dw[1] = 1.5 * u * u - 2.0 * u;
    dw[2] = -1.5 * u * u + u + 0.5;
    dw[3] = 0.5 * u * u;
}

// ---- refinement / score pass: grid (ggx, ggy, nf), block 256 (one crop column per thread, rows_per rows) -----------------------------
// all = 0: frozen frames are skipped (their partials are never read); all = 1: every frame (the score pass)
template <typename T, typename F>
__global__ void __launch_bounds__(256) k_reg_gn(const T *__restrict__ coef, const F *__restrict__ frames, Geo g, int rows_per,
                                                const double *__restrict__ sd, const int *__restrict__ si, int all, double *__restrict__ part)
{
    __shared__ double sh[4 * NG];
    const int f = blockIdx.z;
    if (!all && si[(size_t)f * SI + I_FROZEN])
        return;
    const int Hp = g.H + 2 * SRX_NPAD, Wp = g.W + 2 * SRX_NPAD;
    const double dy = sd[(size_t)f * SD + S_DY], dx = sd[(size_t)f * SD + S_DX];
    const double fy = floor(dy), fx = floor(dx);
    double wyd[4], dwyd[4], wxd[4], dwxd[4];
    taps_d(dy - fy, wyd, dwyd);
    taps_d(dx - fx, wxd, dwxd);
    T wy[4], dwy[4], wx[4], dwx[4];
#pragma unroll
    for (int a = 0; a < 4; a++)
        wy[a] = (T)wyd[a], dwy[a] = (T)dwyd[a], wx[a] = (T)wxd[a], dwx[a] = (T)dwxd[a];
    const int x = blockIdx.x * GW + threadIdx.x;
    const int y0 = blockIdx.y * rows_per, y1 = min(y0 + rows_per, g.h);
    double v[NG];
#pragma unroll
    for (int i = 0; i < NG; i++)
        v[i] = 0.0;
    if (x < g.w) {
        const T *c = coef + (size_t)f * Hp * Wp;
        const F *r = frames + g.ref_plane(f) * g.H * g.W + g.m + x;
        // clamped tap columns ('nearest' on the padded coefficients; never taken for shifts inside the margin)
        int cx[4];
        const int bx = g.m + x + (int)fx - 1 + SRX_NPAD;
#pragma unroll
        for (int b = 0; b < 4; b++)
            cx[b] = min(max(bx + b, 0), Wp - 1);
        const int by = g.m + (int)fy - 1 + SRX_NPAD;  // tap row 0 of crop row y: by + y
        T h[4], dh[4];
        auto row = [&](int R, T &hv, T &dv) {
            const T *p = c + (size_t)min(max(R, 0), Hp - 1) * Wp;
            const T c0 = p[cx[0]], c1 = p[cx[1]], c2 = p[cx[2]], c3 = p[cx[3]];
            hv = wx[0] * c0 + wx[1] * c1 + wx[2] * c2 + wx[3] * c3;
            dv = dwx[0] * c0 + dwx[1] * c1 + dwx[2] * c2 + dwx[3] * c3;
        };
        row(by + y0, h[0], dh[0]);
        row(by + y0 + 1, h[1], dh[1]);
        row(by + y0 + 2, h[2], dh[2]);
        for (int y = y0; y < y1; y++) {
            row(by + y + 3, h[3], dh[3]);
            const double w = (double)(wy[0] * h[0] + wy[1] * h[1] + wy[2] * h[2] + wy[3] * h[3]);
            const double gy = (double)(dwy[0] * h[0] + dwy[1] * h[1] + dwy[2] * h[2] + dwy[3] * h[3]);
            const double gx = (double)(wy[0] * dh[0] + wy[1] * dh[1] + wy[2] * dh[2] + wy[3] * dh[3]);
            const double rv = (double)r[(size_t)(g.m + y) * g.W], e = w - rv;
            v[0] += gy * gy, v[1] += gy * gx, v[2] += gx * gx, v[3] += gy * e, v[4] += gx * e;
            v[5] += w, v[6] += w * w, v[7] += w * rv;
            h[0] = h[1], h[1] = h[2], h[2] = h[3];
            dh[0] = dh[1], dh[1] = dh[2], dh[2] = dh[3];
        }
    }
    metrics::block_sum<NG>(v, sh, part + ((size_t)f * gridDim.x * gridDim.y + blockIdx.y * gridDim.x + blockIdx.x) * NG);
}

// one wave adds frame f's block partials in index order (lane l: blocks l, l + 64, ...; then the fixed shuffle tree) -> lane 0
__device__ __forceinline__ void wave_partials(const double *__restrict__ part, int f, int nblk, double (&s)[NG])
{
#pragma unroll
    for (int i = 0; i < NG; i++)
        s[i] = 0.0;
    for (int k = threadIdx.x; k < nblk; k += 64) {
        const double *p = part + ((size_t)f * nblk + k) * NG;
#pragma unroll
        for (int i = 0; i < NG; i++)
            s[i] += p[i];
    }
#pragma unroll
    for (int i = 0; i < NG; i++)
        s[i] = wave_sum(s[i]);
}

// ---- Gauss-Newton step: grid nf, block 64 ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64) k_reg_solve(const double *__restrict__ part, int nblk, int n_iter, double tol, double *__restrict__ sd,
                                                  int *__restrict__ si)
{
    const int f = blockIdx.x;
    int *q = si + (size_t)f * SI;
    if (q[I_FROZEN])
        return;
    double s[NG];
    wave_partials(part, f, nblk, s);
    if (threadIdx.x != 0)
        return;
    double *d = sd + (size_t)f * SD;
    const double a = s[0], b = s[1], c = s[2], det = a * c - b * b;
    // flat (gradient energy <= 1e-10 sum w^2) or one-directional content (det <= 1e-6 trace^2); NaN sums land here too
    if (!(det > DET_EPS * (a + c) * (a + c)) || !(a + c > GRAD_EPS * s[6])) {
        d[S_DY] = d[S_CY], d[S_DX] = d[S_CX];
        q[I_SINGULAR] = 1, q[I_FROZEN] = 1;
        return;
    }
    const double sy = fmin(fmax(-(c * s[3] - b * s[4]) / det, -0.5), 0.5);
    const double sx = fmin(fmax(-(a * s[4] - b * s[3]) / det, -0.5), 0.5);
    d[S_DY] += sy, d[S_DX] += sx;
    d[S_LAST] = fmax(fabs(sy), fabs(sx));
    const int steps = ++q[I_STEPS];
    if (d[S_LAST] < tol || steps >= n_iter)
        q[I_FROZEN] = 1;
}

// ---- outputs: grid B N, block 64 ------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64) k_reg_finish(const double *__restrict__ part, int nblk, Geo g, int n_iter, double tol,
                                                   const double *__restrict__ sd, const int *__restrict__ si, double *__restrict__ shifts,
                                                   double *__restrict__ score, int *__restrict__ status)
{
    const int bk = blockIdx.x, b = bk / g.N, k = bk - b * g.N;
    if (k == g.ref) {
        if (threadIdx.x == 0) {
            shifts[2 * bk] = 0.0, shifts[2 * bk + 1] = 0.0;
            if (score)
                score[bk] = 1.0;
            if (status)
                status[bk] = ST_OK;
        }
        return;
    }
    const int f = b * (g.N - 1) + (k < g.ref ? k : k - 1);
    double s[NG];
    wave_partials(part, f, nblk, s);
    if (threadIdx.x != 0)
        return;
    const double *d = sd + (size_t)f * SD;
    const int *q = si + (size_t)f * SI;
    shifts[2 * bk] = d[S_DY], shifts[2 * bk + 1] = d[S_DX];
    if (score)
        score[bk] = zm_ncc(d[S_N], s[5], s[6], d[S_SR], d[S_SRR], s[7]);
    if (status)
        status[bk] = q[I_SINGULAR] ? ST_SINGULAR : q[I_EDGE] ? ST_BOUNDARY : (n_iter > 0 && d[S_LAST] >= tol) ? ST_NOT_CONVERGED : ST_OK;
}

// ---- host -----------------------------------------------------------------------------------------------------------------------------
static inline bool geometry(int B, int N, int H, int W, int search, int border, int &m, int &h, int &w)
{
    m = border + search + 2, h = H - 2 * m, w = W - 2 * m;
    return h >= MIN_CROP && w >= MIN_CROP;
}

// the counts the workspace layout depends on: the moving frames, their padded plane, and the block partials per frame of the coarse
// search and of a Gauss-Newton step -- both at the widest crop, border 0, whatever the call's border
struct Dims {
    size_t nf, plane, cpart, gpart;
};
static inline Dims dims(int B, int N, int H, int W, int search)
{
    const int w0 = W - 2 * (search + 2), D = 2 * search + 1;
    return {(size_t)B * (N - 1), (size_t)(H + 2 * SRX_NPAD) * (W + 2 * SRX_NPAD), (size_t)coarse_blocks_max(w0) * (3 * D * D + 2), (size_t)gn_blocks_max(w0) * NG};
}
template <typename T> struct Tabs {
    T *coef, *scratch;
    double *cpart, *gpart, *sd;
    int *si;
};
// the layout: on the call's arena it is the carve, on a counting one the size (a braced list is evaluated left to right)
template <typename T> static Tabs<T> carve(Arena &ar, const Dims &d)
{
    return {ar.take<T>(d.nf * d.plane), ar.take<T>(d.nf * d.plane), ar.take<double>(d.nf * d.cpart), ar.take<double>(d.nf * d.gpart),
            ar.take<double>(d.nf * SD), ar.take<int>(d.nf * SI)};
}
static inline size_t workspace_bytes(int elem_bytes, int B, int N, int H, int W, int search)
{
    if ((elem_bytes != 4 && elem_bytes != 8) || B <= 0 || N < 2 || H <= 0 || W <= 0 || search < 0 || search > MAX_SEARCH)
        return 0;
    int m, h, w;
    if (!geometry(B, N, H, W, search, 0, m, h, w))  // border 0: the widest crop
        return 0;
    const Dims d = dims(B, N, H, W, search);
    return measured([&](Arena &a) { elem_bytes == 8 ? (void)carve<double>(a, d) : (void)carve<float>(a, d); });
}

// F: the frames' type (T, or uint8_t: srx_register_u8_*); T: the coefficients and the arithmetic
template <typename T, typename F>
static int register_frames(const F *frames, int B, int N, int H, int W, int ref, const double *init, int search, int border, int n_iter,
                           double tol, double *shifts, double *score, int *status, void *ws, size_t wsb, hipStream_t st)
{
    if (!frames || !shifts || B <= 0 || N < 2 || H <= 0 || W <= 0 || ref < 0 || ref >= N || search < 0 || search > MAX_SEARCH || border < 0 ||
        n_iter < 0 || !(tol >= 0.0))
        return SRX_E_INVALID;
    Geo g{B, N, H, W, ref, 0, 0, 0};
    if (N > SRX_MAX_FRAMES || !geometry(B, N, H, W, search, border, g.m, g.h, g.w))
        return SRX_E_UNSUPPORTED;
    Start c0{};
    for (int k = 0; k < N && init; k++)
        for (int a = 0; a < 2; a++) {
            const double v = init[2 * k + a] - init[2 * ref + a];
            if (!(std::fabs(v) <= 1e6))
                return SRX_E_INVALID;
            c0.c[k][a] = (int)std::rint(v);
        }
    const int nf = g.nf();
    const size_t plane = (size_t)(H + 2 * SRX_NPAD) * (W + 2 * SRX_NPAD);
    if (nf > 65535 || plane * sizeof(T) >= ((size_t)1 << 31))
        return SRX_E_UNSUPPORTED;
    const Plan p = make_plan(g.h, g.w, search);
    Arena ar(ws, wsb);
    ar.require(workspace_bytes((int)sizeof(T), B, N, H, W, search));
    const auto [coef, scratch, cpart, gpart, sd, si] = carve<T>(ar, dims(B, N, H, W, search));
    if (!ar.ok)
        return SRX_E_WORKSPACE;
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_reg_pad<T, F>), dim3(cdiv(W + 2 * SRX_NPAD, 64), cdiv(H + 2 * SRX_NPAD, 4), nf), dim3(64, 4), 0, st, frames, g, coef);
    SRX_CHECK_LAUNCH();
    SRX_TRY(prefilter2d(coef, scratch, nf, H + 2 * SRX_NPAD, W + 2 * SRX_NPAD, MODE_REFLECT, st));
    launch_coarse<F>(frames, g, search, p, c0, cpart, st);
    SRX_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_reg_pick, dim3(nf), dim3(256), 0, st, cpart, p.cgx * p.cgy, g, search, c0, sd, si);
    SRX_CHECK_LAUNCH();
    const dim3 gg(p.ggx, p.ggy, nf);
    for (int it = 0; it < n_iter; it++) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_reg_gn<T, F>), gg, dim3(GW), 0, st, coef, frames, g, p.grow, sd, si, 0, gpart);
        SRX_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_reg_solve, dim3(nf), dim3(64), 0, st, gpart, p.ggx * p.ggy, n_iter, tol, sd, si);
        SRX_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_reg_gn<T, F>), gg, dim3(GW), 0, st, coef, frames, g, p.grow, sd, si, 1, gpart);
    SRX_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_reg_finish, dim3(B * N), dim3(64), 0, st, gpart, p.ggx * p.ggy, g, n_iter, tol, sd, si, shifts, score, status);
    SRX_CHECK_LAUNCH();
    return SRX_OK;
}

}  // namespace reg
}  // namespace srx
