// srx_metrics.hpp -- device forms of the quality metrics that consume the reconstructions: the parts of the
// reference's analysis that are real work on a frame or an ROI.  Every sum is a FIXED-ORDER two-stage float64 reduction (per-block
// partials, then one block adds them up in index order): no atomics, bit-identical run to run.
//
//   pair moments     n, sum t, sum r, sum t^2, sum t r, sum r^2, sum (r - t)^2 over the frame minus a border: PSNR and the vendor
//                    GUI's PSNR after an affine intensity fit (opt_materials/software/XPR_Software.py:735-745, 1215-1256) from ONE pass over
//                    two device images (12.6 MP each for the cal-target frames) instead of a device-to-host copy and numpy
//   local contrast   Michelson (max - min) / (max + min + 1e-9) over a sliding window (mono_cal_target/analysis.ipynb cell 4)
//   ring means       radial_average (data_collection/psf_mtf_utils.py:74-95): ring k = pixels whose distance to the centre truncates to k
//   spot moments     subpixel_centre (psf_mtf_utils.py:67-71): first moments where the PSF exceeds a tenth of its peak
//   edge ROI         slanted_edge_esf's image part (analysis.ipynb cell 7): Gaussian sigma 1.5 (scipy 'reflect'), Sobel magnitude; then every
//                    ROI pixel projected on the fitted edge's normal and binned at 1/4 px (sums and counts per bin)
//   SSIM             skimage structural_similarity (2-D; the vendor GUI's SSIM score, XPR_Software.py:1220-1256): the five windowed moments
//                    held on chip in ONE pass over the two images (k_ssim), the mean of S as a float64 fixed-order reduction, the map optional;
//                    its affine-fit form applies the fitted line inside the kernel.  The ECC score follows from the pair moments.
// For these entry points the percentile, the two line fits, the ESF interpolation, np.gradient / Hann / FFT of 72 samples, the 7-parameter
// Gaussian fit and the 256^2 FFT of compute_mtf stay on the host (sr_mi355x/metrics.py): a few thousand operations each.  srx_edge_sfr_*
// (srx_sfr.hpp) is the slanted-edge chain whole, without a host step; the per-pixel filter arithmetic of k_correlate1d / k_sobel_mag lives
// there, shared with it.
#pragma once
#include "srx_common.h"
#include "srx_sfr.hpp"  // the per-pixel filter arithmetic (shared with srx_edge_sfr_* and its host model)

namespace srx {
namespace metrics {

constexpr int NMOM = 7;       // n, st, sr, stt, str, srr, sdd
constexpr int RED_BLOCKS = 1024;

// ---- fixed-order block reduction of NV doubles per thread (256 threads) into out[NV] by thread 0 ------------------------------------
template <int NV> __device__ __forceinline__ void block_sum(double (&v)[NV], double *sh /*[4][NV]*/, double *out)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < NV; i++) {
        const double s = wave_sum(v[i]);
        if (lane == 0)
            sh[wave * NV + i] = s;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 0; i < NV; i++)
            out[i] = (sh[i] + sh[NV + i]) + (sh[2 * NV + i] + sh[3 * NV + i]);
    }
}

// stage 1: grid (nblk, B), block 256: the block's share of the interior pixels (row-major order, contiguous chunks of whole rows)
template <typename T>
__global__ void __launch_bounds__(256) k_pair_moments(const T *__restrict__ ref, const T *__restrict__ test, int H, int W, int border, double *__restrict__ part)
{
    __shared__ double sh[4 * NMOM];
    const int b = blockIdx.y, nblk = gridDim.x;
    const int h = H - 2 * border, w = W - 2 * border;
    const int rows_per = (h + nblk - 1) / nblk, y0 = blockIdx.x * rows_per, y1 = min(y0 + rows_per, h);
    const T *r0 = ref + (size_t)b * H * W, *t0 = test + (size_t)b * H * W;
    double v[NMOM];
#pragma unroll
    for (int i = 0; i < NMOM; i++)
        v[i] = 0.0;
    for (int y = y0; y < y1; y++) {
        const size_t row = (size_t)(y + border) * W + border;
        for (int x = threadIdx.x; x < w; x += 256) {
            const double r = (double)r0[row + x], t = (double)t0[row + x], d = r - t;
            v[0] += 1.0, v[1] += t, v[2] += r, v[3] += t * t, v[4] += t * r, v[5] += r * r, v[6] += d * d;
        }
    }
    block_sum<NMOM>(v, sh, part + ((size_t)b * nblk + blockIdx.x) * NMOM);
}

// stage 2: grid B, block 64: out[b][i] = sum over the blocks in index order (one lane per moment)
__global__ void __launch_bounds__(64) k_sum_partials(const double *__restrict__ part, int nblk, int nv, double *__restrict__ out)
{
    const int b = blockIdx.x, i = threadIdx.x;
    if (i >= nv)
        return;
    double s = 0.0;
    for (int k = 0; k < nblk; k++)
        s += part[((size_t)b * nblk + k) * nv + i];
    out[(size_t)b * nv + i] = s;
}

// ---- local contrast: grid (ceil(n / 256), B) ----------------------------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(256) k_local_contrast(const T *__restrict__ prof, int n, int window, T *__restrict__ out)
{
    const int i = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y, hw = window / 2;
    if (i >= n)
        return;
    const T *p = prof + (size_t)b * n;
    T res = 0;
    if (hw > 0 && n >= 2 * hw + 1 && i >= hw && i < n - hw) {
        T mn = p[i - hw], mx = mn;
        for (int j = i - hw + 1; j < i + hw; j++) {
            const T v = p[j];
            mn = v < mn ? v : mn, mx = v > mx ? v : mx;
        }
        res = (mx - mn) / (mx + mn + (T)1e-9);
    }
    out[(size_t)b * n + i] = res;
}

// ---- ring means: stage 1, one block per image ROW: the row's sum and count per ring into rows[y][2 nbin] (a row meets every ring at
// most twice on either side of the centre: the partial is mostly zeros, and exact); stage 2 adds the rows up in index order ------------
template <typename T>
__global__ void __launch_bounds__(256) k_ring_rows(const T *__restrict__ img, int H, int W, double cy, double cx, int nbin, double *__restrict__ rows)
{
#pragma clang fp contract(off)  // (the host evaluates these expressions with separate multiplies and adds: same bits)
    extern __shared__ double acc[];  // [2 nbin]
    const int y = blockIdx.x;
    for (int i = threadIdx.x; i < 2 * nbin; i += 256)
        acc[i] = 0.0;
    __syncthreads();
    // one thread walks the row (<= a few thousand pixels): the order of the additions is the raster order, as np.bincount's
    if (threadIdx.x == 0) {
        const double dy = (double)y - cy;
        for (int x = 0; x < W; x++) {
            const double dx = (double)x - cx;
            const int ring = (int)sqrt(dx * dx + dy * dy);
            if (ring < nbin)
                acc[ring] += (double)img[(size_t)y * W + x], acc[nbin + ring] += 1.0;
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 2 * nbin; i += 256)
        rows[(size_t)y * 2 * nbin + i] = acc[i];
}
__global__ void __launch_bounds__(256) k_ring_sum(const double *__restrict__ rows, int H, int nbin, double *__restrict__ out /*[2 nbin]: sums, counts*/)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= 2 * nbin)
        return;
    double s = 0.0;
    for (int y = 0; y < H; y++)
        s += rows[(size_t)y * 2 * nbin + i];
    out[i] = s;
}

// ---- spot moments: max, then sums of spot, y spot, x spot where img > 0.1 max.  One block (PSF images are ~41 x 41 to 256 x 256) ----------
template <typename T>
__global__ void __launch_bounds__(256) k_spot_moments(const T *__restrict__ img, int H, int W, double *__restrict__ out /*[4]: max, mass, sum y, sum x*/)
{
    __shared__ double sh[4 * 3];
    __shared__ double smax[4];
    const int n = H * W;
    double mx = -1e300;
    for (int i = threadIdx.x; i < n; i += 256)
        mx = fmax(mx, (double)img[i]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
        mx = fmax(mx, __shfl_down(mx, o, 64));
    if ((threadIdx.x & 63) == 0)
        smax[threadIdx.x >> 6] = mx;
    __syncthreads();
    mx = fmax(fmax(smax[0], smax[1]), fmax(smax[2], smax[3]));
    double v[3] = {0.0, 0.0, 0.0};
    for (int i = threadIdx.x; i < n; i += 256) {
        const double p = (double)img[i];
        if (p > 0.1 * mx) {
            const int y = i / W, x = i - y * W;
            v[0] += p, v[1] += p * (double)y, v[2] += p * (double)x;
        }
    }
    __syncthreads();
    block_sum<3>(v, sh, out + 1);
    if (threadIdx.x == 0)
        out[0] = mx;
}

// ---- edge ROI: separable correlation with scipy.ndimage's 'reflect' boundary (d c b a | a b c d | d c b a), float64 -------------------
// axis 0: along rows (y), axis 1: along columns (x).  taps [2 r + 1] by value (r <= 8).  grid (ceil(W / 64), ceil(H / 4)), block (64, 4)
using sfr::Taps17;
using sfr::reflect_idx;
__global__ void __launch_bounds__(256) k_correlate1d(const double *__restrict__ in, int H, int W, int axis, Taps17 t, double *__restrict__ out)
{
#pragma clang fp contract(off)  // (the host evaluates these expressions with separate multiplies and adds: same bits)
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= W || y >= H)
        return;
    out[(size_t)y * W + x] = sfr::correlate_at(t, axis, y, x, H, W, [&](int yy, int xx) { return in[(size_t)yy * W + xx]; });
}
// mag = sqrt(gx^2 + gy^2), gx = sobel along axis 1 (derivative along x, smoothing along y), gy along axis 0; 'reflect' boundary
__global__ void __launch_bounds__(256) k_sobel_mag(const double *__restrict__ in, int H, int W, double *__restrict__ mag)
{
#pragma clang fp contract(off)  // (the host evaluates these expressions with separate multiplies and adds: same bits)
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= W || y >= H)
        return;
    // correlate [-1 0 1] along the derivative axis first, then [1 2 1] along the other (the order of metrics._sobel)
    mag[(size_t)y * W + x] = sfr::sobel_mag_at(y, x, H, W, [&](int yy, int xx) { return in[(size_t)yy * W + xx]; });
}

// every ROI pixel projected on the edge's normal: dist = (v - m u - b) / norm with (u, v) = (row, col) if rows_are_x else (col, row);
// pixels with -8 < dist < 10 fall into bin floor-by-comparison on edges lo + i bw.  Stage 1: one block per ROI row, a thread per bin
// walks the row in raster order (<= a few hundred pixels): sums and counts per bin, exact order.  Stage 2 = k_ring_sum.
struct EdgeLine {
    double m, b, norm, lo, bw;
    int rows_are_x, nbin;
};
template <typename T>
__global__ void __launch_bounds__(128) k_edge_bins_rows(const T *__restrict__ roi, int H, int W, EdgeLine e, double *__restrict__ rows /*[H][2 nbin]*/)
{
#pragma clang fp contract(off)  // (the host evaluates these expressions with separate multiplies and adds: same bits)
    const int y = blockIdx.x, i = threadIdx.x;
    if (i >= e.nbin)
        return;
    // bin i holds lo + i bw <= d < lo + (i + 1) bw, the edges formed exactly as np.arange(lo, hi + bw, bw) forms them: lo + i * bw
    const double e0 = e.lo + (double)i * e.bw, e1 = e.lo + (double)(i + 1) * e.bw;
    double s = 0.0, c = 0.0;
    for (int x = 0; x < W; x++) {
        const double u = e.rows_are_x ? (double)y : (double)x, v = e.rows_are_x ? (double)x : (double)y;
        const double d = (v - e.m * u - e.b) / e.norm;
        if (d > -8.0 && d < 10.0 && d >= e0 && d < e1)
            s += (double)roi[(size_t)y * W + x], c += 1.0;
    }
    rows[(size_t)y * 2 * e.nbin + i] = s;
    rows[(size_t)y * 2 * e.nbin + e.nbin + i] = c;
}
// min and max of dist over the kept pixels (the bin edges start at the minimum): one block, fixed order irrelevant for min / max
__global__ void __launch_bounds__(256) k_edge_dist_range(int H, int W, EdgeLine e, double *__restrict__ out /*[2]*/)
{
#pragma clang fp contract(off)  // (the host evaluates these expressions with separate multiplies and adds: same bits)
    __shared__ double smn[4], smx[4];
    double mn = 1e300, mx = -1e300;
    for (int i = threadIdx.x; i < H * W; i += 256) {
        const int y = i / W, x = i - y * W;
        const double u = e.rows_are_x ? (double)y : (double)x, v = e.rows_are_x ? (double)x : (double)y;
        const double d = (v - e.m * u - e.b) / e.norm;
        if (d > -8.0 && d < 10.0)
            mn = fmin(mn, d), mx = fmax(mx, d);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
        mn = fmin(mn, __shfl_down(mn, o, 64)), mx = fmax(mx, __shfl_down(mx, o, 64));
    if ((threadIdx.x & 63) == 0)
        smn[threadIdx.x >> 6] = mn, smx[threadIdx.x >> 6] = mx;
    __syncthreads();
    if (threadIdx.x == 0) {
        out[0] = fmin(fmin(smn[0], smn[1]), fmin(smn[2], smn[3]));
        out[1] = fmax(fmax(smx[0], smx[1]), fmax(smx[2], smx[3]));
    }
}

// ---- SSIM (skimage structural_similarity, 2-D): ONE pass over the two images ------------------------------------------------------
// Block = 256 columns of the crop (4 waves side by side) x rows_per output rows.  Each input row (reflected, 'reflect' = d c b a | a b c d)
// is staged once in LDS (256 + 2R values of x and of y, after the optional affine and a per-block shift), every lane forms the
// horizontal window sums of x, y, x^2, y^2, x y for its column, and keeps them in a ring of the last 2R + 1 rows in registers (the row
// loop is unrolled by 2R + 1, so every ring index is a constant).  When a row completes a window, the vertical sums give S for output
// row (row - R), which is optionally stored in T and, inside [R, h - R) x [R, w - R), added to a float64 per-thread sum.  No plane other
// than the optional map goes to memory; the extra input traffic is the 2R-row / 2R-column halos.  The shift (the block's first pixel)
// leaves the moments unchanged and keeps x^2 - mean^2 from cancelling in float32.  Per-block float64 partials, then k_mean_partials.
constexpr int SSIM_MAX_R = 7;
constexpr int SSIM_TW = 256;                         // crop columns per block
constexpr int SSIM_TARGET_BLOCKS = 1024;             // 4096 waves: 16 per CU
constexpr int SSIM_MAX_BLOCKS = RED_BLOCKS * NMOM;   // per item: what srx_metrics_workspace_bytes sizes the partials for
template <typename T> struct SsimArgs {
    T k[2 * SSIM_MAX_R + 1];  // correlation taps, 2R + 1 used
    T c1, c2, cov_norm;
};

template <typename T, int R>
__global__ void __launch_bounds__(256) k_ssim(const T *__restrict__ ref, const T *__restrict__ test, int H, int W, int border, int rows_per, SsimArgs<T> a,
                                              const double *__restrict__ affine /*[B][3] or null*/, double *__restrict__ part, T *__restrict__ map)
{
    constexpr int D = 2 * R + 1, NL = SSIM_TW + 2 * R;
    __shared__ T sx[2][NL], sy[2][NL];
    __shared__ double sh[4];
    const int b = blockIdx.z, tid = threadIdx.x, h = H - 2 * border, w = W - 2 * border;
    const int x0 = blockIdx.x * SSIM_TW, y0 = blockIdx.y * rows_per, y1 = min(y0 + rows_per, h), x = x0 + tid;
    const T *rp = ref + (size_t)b * H * W + (size_t)border * W + border, *tp = test + (size_t)b * H * W + (size_t)border * W + border;
    T ar = 1, at = 1, bt = 0;
    if (affine)
        ar = (T)affine[3 * b], at = (T)affine[3 * b + 1], bt = (T)affine[3 * b + 2];
    // crop columns x0 - R + tid and (lanes < 2R) x0 - R + 256 + tid, reflected once (R < w); past w + R they feed no output: clamped
    auto col = [&](int i) { i = i < 0 ? -1 - i : (i >= w ? 2 * w - 1 - i : i); return max(0, min(i, w - 1)); };
    const int ca = col(x0 - R + tid), cb = col(x0 - R + SSIM_TW + tid);
    const bool halo = tid < 2 * R;
    const T cr = ar * rp[(size_t)y0 * W + min(x0, w - 1)], ct = at * tp[(size_t)y0 * W + min(x0, w - 1)] + bt;
    const int ylast = y1 - 1 + R;  // input rows y0 - R .. y1 - 1 + R, reflected once (R < h); the last group's rows past them are clamped
    T ra, ta, rb = 0, tb = 0;
    auto fetch = [&](int yi) {
        const int o = max(0, yi < 0 ? -1 - yi : (yi >= h ? 2 * h - 1 - yi : yi)) * W;
        ra = rp[o + ca], ta = tp[o + ca];
        if (halo)
            rb = rp[o + cb], tb = tp[o + cb];
    };
    fetch(y0 - R);
    T ring[5][D];  // horizontal sums of x, y, xx, yy, xy; slot j of a group = row (group start + j)
    double acc = 0.0;
    int buf = 0;
    // groups of D input rows with no early exit (a loop that can break is not unrolled, and the ring would go to scratch); the host
    // sizes rows_per so that only a batch item's last block row runs past ylast
#pragma nounroll
    for (int yi = y0 - R; yi <= ylast;) {
#pragma unroll
        for (int j = 0; j < D; j++, yi++) {
            sx[buf][tid] = ar * ra - cr, sy[buf][tid] = at * ta + bt - ct;
            if (halo)
                sx[buf][SSIM_TW + tid] = ar * rb - cr, sy[buf][SSIM_TW + tid] = at * tb + bt - ct;
            fetch(yi + 1);  // the next row's loads are in flight during this row's arithmetic
            __syncthreads();  // (one barrier per row: the two buffers alternate)
            T hx = 0, hy = 0, hxx = 0, hyy = 0, hxy = 0;
#pragma unroll
            for (int k = 0; k < D; k++) {
                const T u = sx[buf][tid + k], v = sy[buf][tid + k], kk = a.k[k];
                // every product formed the same way for x and y: SSIM(a, b) and SSIM(b, a) are bit-identical
                hx += kk * u, hy += kk * v, hxx += kk * (u * u), hyy += kk * (v * v), hxy += kk * (u * v);
            }
            ring[0][j] = hx, ring[1][j] = hy, ring[2][j] = hxx, ring[3][j] = hyy, ring[4][j] = hxy;
            buf ^= 1;
            if (yi >= y0 + R && yi <= ylast) {  // rows yi - 2R .. yi (the first is y0 - R) are in the ring: output row yi - R
                T m[5];
#pragma unroll
                for (int q = 0; q < 5; q++) {
                    T s = 0;
#pragma unroll
                    for (int k = 0; k < D; k++)
                        s += a.k[k] * ring[q][(j + 1 + k) % D];
                    m[q] = s;
                }
                const int yo = yi - R;
                T s;
                {
#pragma clang fp contract(off)  // symmetric in x and y to the bit
                    const T mx = m[0] + cr, my = m[1] + ct;
                    const T vx = a.cov_norm * (m[2] - m[0] * m[0]), vy = a.cov_norm * (m[3] - m[1] * m[1]), vxy = a.cov_norm * (m[4] - m[0] * m[1]);
                    s = ((T)2 * mx * my + a.c1) * ((T)2 * vxy + a.c2) / ((mx * mx + my * my + a.c1) * (vx + vy + a.c2));
                }
                if (x < w) {
                    if (map)
                        map[(size_t)b * h * w + (size_t)yo * w + x] = s;
                    if (yo >= R && yo < h - R && x >= R && x < w - R)
                        acc += (double)s;
                }
            }
        }
    }
    double v[1] = {acc};
    block_sum<1>(v, sh, part + (size_t)b * gridDim.x * gridDim.y + blockIdx.y * gridDim.x + blockIdx.x);
}

// stage 2 of k_ssim: grid B, block 64: out[b] = (sum of the block partials) / n; lane l adds partials l, l + 64, ... in order, then the
// fixed shuffle tree (bit-identical run to run)
__global__ void __launch_bounds__(64) k_mean_partials(const double *__restrict__ part, int nblk, double n, double *__restrict__ out)
{
    const int b = blockIdx.x;
    double s = 0.0;
    for (int k = threadIdx.x; k < nblk; k += 64)
        s += part[(size_t)b * nblk + k];
    s = wave_sum(s);
    if (threadIdx.x == 0)
        out[b] = s / n;
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------
// The three layouts of this file, each the carve of the calls that use it and, measured, a term of the size below:
// block partials per item (pair_moments: nblk * NMOM, ssim: nblk; at most SSIM_MAX_BLOCKS = RED_BLOCKS * NMOM either way) ...
static double *carve_partials(Arena &ar, size_t B, size_t per_item) { return ar.take<double>(B * per_item); }
// ... per-row sums and counts of nbin bins (ring_sums, edge_bins) ...
static double *carve_rows(Arena &ar, size_t H, size_t nbin) { return ar.take<double>(H * 2 * nbin); }
// ... and two float64 planes (edge_magnitude)
struct Planes {
    double *a, *b;
};
static Planes carve_planes(Arena &ar, size_t H, size_t W) { return {ar.take<double>(H * W), ar.take<double>(H * W)}; }
// srx_metrics_workspace_bytes: one size for every metric of a [B, H, W] batch with nbin bins.  A call is held to it at its own
// arguments (B = 1 / nbin = 1 where it has none), so a caller that sized the arena for the whole set passes every call.
static inline size_t workspace_bytes(int B, int H, int W, int nbin)
{
    const size_t b1 = B > 0 ? B : 1, h1 = H > 0 ? H : 1, w1 = W > 0 ? W : 1, n1 = nbin > 0 ? nbin : 1;
    const size_t a = measured([&](Arena &m) { carve_partials(m, b1, SSIM_MAX_BLOCKS); }), b = measured([&](Arena &m) { carve_rows(m, h1, n1); }),
                 c = measured([&](Arena &m) { carve_planes(m, h1, w1); });
    return std::max(a, std::max(b, c));
}

template <typename T>
static int pair_moments(const T *ref, const T *test, int B, int H, int W, int border, double *out, void *ws, size_t wsb, hipStream_t st)
{
    if (!ref || !test || !out || B <= 0 || H <= 0 || W <= 0 || border < 0 || 2 * border >= H || 2 * border >= W)
        return SRX_E_INVALID;
    if (B > 65535)
        return SRX_E_UNSUPPORTED;
    Arena ar(ws, wsb);
    ar.require(workspace_bytes(B, H, W, 1));
    const int nblk = std::min(RED_BLOCKS, H - 2 * border);
    double *part = carve_partials(ar, B, (size_t)nblk * NMOM);
    if (!ar.ok)
        return SRX_E_WORKSPACE;
    hipLaunchKernelGGL(k_pair_moments<T>, dim3(nblk, B), dim3(256), 0, st, ref, test, H, W, border, part);
    SRX_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_sum_partials, dim3(B), dim3(64), 0, st, part, nblk, NMOM, out);
    SRX_CHECK_LAUNCH();
    return SRX_OK;
}

template <typename T, int R>
static void launch_ssim(dim3 grid, hipStream_t st, const T *ref, const T *test, int H, int W, int border, int rows_per, const SsimArgs<T> &a,
                        const double *affine, double *part, T *map)
{
    hipLaunchKernelGGL((k_ssim<T, R>), grid, dim3(256), 0, st, ref, test, H, W, border, rows_per, a, affine, part, map);
}

// mean SSIM per item into mssim[B] (device); map [B][H - 2 border][W - 2 border] in T when not null.  taps: 2 radius + 1 host doubles
template <typename T>
static int ssim(const T *ref, const T *test, int B, int H, int W, int border, int radius, const double *taps, int sample_cov, double data_range, double k1,
                double k2, const double *affine, double *mssim, T *map, void *ws, size_t wsb, hipStream_t st)
{
    if (!ref || !test || !taps || !mssim || B <= 0 || H <= 0 || W <= 0 || border < 0 || 2 * border >= H || 2 * border >= W || radius < 1 ||
        !(data_range > 0.0) || !std::isfinite(data_range) || !std::isfinite(k1) || !std::isfinite(k2))
        return SRX_E_INVALID;
    if (radius > SSIM_MAX_R)
        return SRX_E_UNSUPPORTED;
    const int h = H - 2 * border, w = W - 2 * border, D = 2 * radius + 1;
    if (D > h || D > w)
        return SRX_E_INVALID;
    const int gx = cdiv(w, SSIM_TW);
    if (B > 65535 || (size_t)H * W * sizeof(T) >= ((size_t)1 << 31) || gx > SSIM_MAX_BLOCKS)
        return SRX_E_UNSUPPORTED;
    SsimArgs<T> a;
    for (int j = 0; j < 2 * SSIM_MAX_R + 1; j++)
        a.k[j] = j < D ? (T)taps[j] : (T)0;
    const double np = (double)D * D;
    a.c1 = (T)((k1 * data_range) * (k1 * data_range)), a.c2 = (T)((k2 * data_range) * (k2 * data_range));
    a.cov_norm = (T)(sample_cov ? np / (np - 1.0) : 1.0);
    // about SSIM_TARGET_BLOCKS blocks over the batch, at least 32 output rows each (the 2R-row halo stays a small share)
    int gy = std::min(cdiv(SSIM_TARGET_BLOCKS, gx * B), std::max(1, h / 32));
    gy = std::max(1, std::min(gy, SSIM_MAX_BLOCKS / gx));
    const int rows_per = cdiv(cdiv(h, gy) + 2 * radius, D) * D - 2 * radius;  // rows_per + 2R input rows: whole groups of D
    gy = cdiv(h, rows_per);
    const int nblk = gx * gy;
    Arena ar(ws, wsb);
    ar.require(workspace_bytes(B, H, W, 1));
    double *part = carve_partials(ar, B, nblk);
    if (!ar.ok)
        return SRX_E_WORKSPACE;
    const dim3 grid(gx, gy, B);
    switch (radius) {
    case 1: launch_ssim<T, 1>(grid, st, ref, test, H, W, border, rows_per, a, affine, part, map); break;
    case 2: launch_ssim<T, 2>(grid, st, ref, test, H, W, border, rows_per, a, affine, part, map); break;
    case 3: launch_ssim<T, 3>(grid, st, ref, test, H, W, border, rows_per, a, affine, part, map); break;
    case 4: launch_ssim<T, 4>(grid, st, ref, test, H, W, border, rows_per, a, affine, part, map); break;
    case 5: launch_ssim<T, 5>(grid, st, ref, test, H, W, border, rows_per, a, affine, part, map); break;
    case 6: launch_ssim<T, 6>(grid, st, ref, test, H, W, border, rows_per, a, affine, part, map); break;
    default: launch_ssim<T, 7>(grid, st, ref, test, H, W, border, rows_per, a, affine, part, map); break;
    }
    SRX_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_mean_partials, dim3(B), dim3(64), 0, st, part, nblk, (double)(h - 2 * radius) * (double)(w - 2 * radius), mssim);
    SRX_CHECK_LAUNCH();
    return SRX_OK;
}

template <typename T> static int local_contrast(const T *prof, int B, int n, int window, T *out, hipStream_t st)
{
    if (!prof || !out || B <= 0 || n <= 0 || window < 0)
        return SRX_E_INVALID;
    if (B > 65535)
        return SRX_E_UNSUPPORTED;
    hipLaunchKernelGGL(k_local_contrast<T>, dim3(cdiv(n, 256), B), dim3(256), 0, st, prof, n, window, out);
    SRX_CHECK_LAUNCH();
    return SRX_OK;
}

template <typename T>
static int ring_sums(const T *img, int H, int W, double cy, double cx, int nbin, double *out, void *ws, size_t wsb, hipStream_t st)
{
    if (!img || !out || H <= 0 || W <= 0 || nbin <= 0 || nbin > 4096)
        return SRX_E_INVALID;
    Arena ar(ws, wsb);
    ar.require(workspace_bytes(1, H, W, nbin));
    double *rows = carve_rows(ar, H, nbin);
    if (!ar.ok)
        return SRX_E_WORKSPACE;
    hipLaunchKernelGGL(k_ring_rows<T>, dim3(H), dim3(256), (size_t)2 * nbin * sizeof(double), st, img, H, W, cy, cx, nbin, rows);
    SRX_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_ring_sum, dim3(cdiv(2 * nbin, 256)), dim3(256), 0, st, rows, H, nbin, out);
    SRX_CHECK_LAUNCH();
    return SRX_OK;
}

template <typename T> static int spot_moments(const T *img, int H, int W, double *out, hipStream_t st)
{
    if (!img || !out || H <= 0 || W <= 0 || (size_t)H * W > (1u << 24))
        return SRX_E_INVALID;
    hipLaunchKernelGGL(k_spot_moments<T>, dim3(1), dim3(256), 0, st, img, H, W, out);
    SRX_CHECK_LAUNCH();
    return SRX_OK;
}

// Gaussian(sigma, truncate 4) along both axes, then the Sobel magnitude.  roi float64 [H, W] -> mag float64 [H, W]; scratch 2 planes
static int edge_magnitude(const double *roi, int H, int W, double sigma, double *mag, void *ws, size_t wsb, hipStream_t st)
{
    if (!roi || !mag || H <= 0 || W <= 0 || !(sigma > 0.0))
        return SRX_E_INVALID;
    Taps17 t;
    if (!sfr::gaussian_taps(sigma, t))
        return SRX_E_UNSUPPORTED;
    Arena ar(ws, wsb);
    ar.require(workspace_bytes(1, H, W, 1));
    const auto [a, b] = carve_planes(ar, H, W);
    if (!ar.ok)
        return SRX_E_WORKSPACE;
    const dim3 grid(cdiv(W, 64), cdiv(H, 4)), blk(64, 4);
    hipLaunchKernelGGL(k_correlate1d, grid, blk, 0, st, roi, H, W, 0, t, a);  // metrics._gaussian_filter: axis 0 first
    SRX_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_correlate1d, grid, blk, 0, st, a, H, W, 1, t, b);
    SRX_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_sobel_mag, grid, blk, 0, st, b, H, W, mag);
    SRX_CHECK_LAUNCH();
    return SRX_OK;
}

template <typename T>
static int edge_bins(const T *roi, int H, int W, EdgeLine e, double *out /*[2 nbin]*/, void *ws, size_t wsb, hipStream_t st)
{
    if (!roi || !out || H <= 0 || W <= 0 || e.nbin <= 0 || e.nbin > 128 || !(e.norm > 0.0) || !(e.bw > 0.0))
        return SRX_E_INVALID;
    Arena ar(ws, wsb);
    ar.require(workspace_bytes(1, H, W, e.nbin));
    double *rows = carve_rows(ar, H, e.nbin);
    if (!ar.ok)
        return SRX_E_WORKSPACE;
    hipLaunchKernelGGL(k_edge_bins_rows<T>, dim3(H), dim3(128), 0, st, roi, H, W, e, rows);
    SRX_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_ring_sum, dim3(cdiv(2 * e.nbin, 256)), dim3(256), 0, st, rows, H, e.nbin, out);
    SRX_CHECK_LAUNCH();
    return SRX_OK;
}

}  // namespace metrics
}  // namespace srx
