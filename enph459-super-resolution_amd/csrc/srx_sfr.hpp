// srx_sfr.hpp -- the slanted-edge SFR of device ROIs in one call (srx_edge_sfr_*): metrics.slanted_edge_esf -> esf_to_mtf -> mtf_at_fraction
// (mono_cal_target/analysis.ipynb cells 6 - 10) for a batch of ROIs, with no host step between the image and MTF50 / MTF10.
//
// Part 1 (plain C++, no HIP type, SRX_SFR_HD = __host__ __device__ under hipcc and nothing elsewhere; tests/edge_sfr_host_model.cpp includes
// it with SRX_SFR_HOST_ONLY and runs it under -fsanitize=address,undefined): every piece of arithmetic of the call --
//   the filters       reflect_idx, correlate_at, sobel_mag_at: what k_correlate1d / k_sobel_mag (srx_metrics.hpp) evaluate per pixel
//   the order statistic   an exact radix selection on the magnitudes' bit patterns (non-negative doubles order as unsigned integers): eight
//                     8-bit digits from the top; select_digit is one step on a 256-bin histogram.  np.percentile(mag, 85): the virtual index
//                     (n - 1) 0.85, the two order statistics around it, numpy's _lerp (percentile_index, lerp)
//   the line fits     np.polyfit(u, v, 1) as the closed form on EXACT integer sums n, su, sv, suu, suv: the two differences of products are
//                     formed in 128 bits (n suu reaches 2^80 on a 1 x 2^20 ROI), converted once (round to nearest even, as a 64-bit
//                     conversion does whenever the value fits one), then m = num / den, b = (sv - m su) / n
//   the bins          line_dist (the expression of k_edge_dist_range / k_edge_bins_rows), edges lo + i / 4, edge_count as np.arange counts
//   the tail          esf_from_bins (means, np.interp over the non-empty bins, flip), lsf_windowed (np.gradient's non-uniform second-order
//                     form, np.hanning), dft_abs (direct DFT, twiddle index reduced in integers), mtf_finish, mtf_crossing
// Every expression that the host forms with separate multiplies and adds is under fp contract(off).
// Part 2 (hipcc only): the six kernels and the host driver.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define SRX_SFR_HD __host__ __device__
#else
#define SRX_SFR_HD
#endif
#if defined(__clang__)
#define SRX_SFR_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define SRX_SFR_NO_CONTRACT  // (build the host model with -ffp-contract=off)
#endif

namespace srx {
namespace sfr {

constexpr int MAX_BINS = 80;      // SRX_EDGE_MAX_BINS: distances in (-8, 10) at 1/4 px give at most 72
constexpr int SUMMARY = 16;       // SRX_EDGE_SUMMARY
constexpr int MAX_GROUPS = 256;   // row groups of the bin sums
constexpr double BIN_WIDTH = 0.25;
// summary slots ([0] and [1] carry the status and the norm while the record travels through the workspace)
enum { S_MTF50 = 0, S_MTF10, S_ANGLE, S_M, S_B, S_ROWS_ARE_X, S_THRESHOLD, S_N_EDGE, S_N_SIDE, S_NBIN, S_LO, S_HI, S_FLIPPED, S_MC, S_BC, S_ZERO };
enum { ST_OK = 0, ST_FEW_EDGE = 1, ST_FEW_SIDE = 2, ST_DEGENERATE = 3, ST_FEW_BINS = 4 };

SRX_SFR_HD inline double nan_value() { return __builtin_nan(""); }

// ---- filters --------------------------------------------------------------------------------------------------------------------------
struct Taps17 {
    double k[17];
    int r;
};
SRX_SFR_HD inline int reflect_idx(int i, int n)
{
    // numpy 'symmetric' / scipy 'reflect': ... 1 0 | 0 1 2 ... n-1 | n-1 n-2 ...
    const int p = 2 * n;
    i = ((i % p) + p) % p;
    return i < n ? i : p - 1 - i;
}
// metrics._gaussian_filter's taps (truncate 4); false: the radius is above 8 (the caller has checked sigma > 0)
static inline bool gaussian_taps(double sigma, Taps17 &t)
{
    if (!(4.0 * sigma + 0.5 < 9.0))
        return false;
    t.r = (int)(4.0 * sigma + 0.5);
    double sum = 0.0;
    for (int j = 0; j <= 2 * t.r; j++) {
        const double x = (double)(j - t.r);
        t.k[j] = exp(-0.5 / (sigma * sigma) * x * x), sum += t.k[j];
    }
    for (int j = 0; j <= 2 * t.r; j++)
        t.k[j] /= sum;
    for (int j = 2 * t.r + 1; j < 17; j++)
        t.k[j] = 0.0;
    return true;
}
// one output sample of the correlation along `axis` (0: rows, 1: columns); in(yy, xx) with both indices in range
template <typename Load> SRX_SFR_HD inline double correlate_at(const Taps17 &t, int axis, int y, int x, int H, int W, Load in)
{
    SRX_SFR_NO_CONTRACT
    double s = 0.0;
    for (int j = 0; j <= 2 * t.r; j++) {
        const int yy = axis == 0 ? reflect_idx(y + j - t.r, H) : y, xx = axis == 1 ? reflect_idx(x + j - t.r, W) : x;
        s += t.k[j] * in(yy, xx);
    }
    return s;
}
// sqrt(gx^2 + gy^2), gx = sobel along axis 1, gy along axis 0: [-1 0 1] along the derivative axis first, then [1 2 1] along the other (the
// order of metrics._sobel)
template <typename Load> SRX_SFR_HD inline double sobel_mag_at(int y, int x, int H, int W, Load in)
{
    SRX_SFR_NO_CONTRACT
    auto at = [&](int yy, int xx) { return in(reflect_idx(yy, H), reflect_idx(xx, W)); };
    auto dx = [&](int yy) { return -1.0 * at(yy, x - 1) + 0.0 * at(yy, x) + 1.0 * at(yy, x + 1); };
    auto dy = [&](int xx) { return -1.0 * at(y - 1, xx) + 0.0 * at(y, xx) + 1.0 * at(y + 1, xx); };
    const double gx = 1.0 * dx(y - 1) + 2.0 * dx(y) + 1.0 * dx(y + 1);
    const double gy = 1.0 * dy(x - 1) + 2.0 * dy(x) + 1.0 * dy(x + 1);
    return sqrt(gx * gx + gy * gy);
}

// ---- order statistic ------------------------------------------------------------------------------------------------------------------
SRX_SFR_HD inline uint64_t key_of(double v)
{
    uint64_t k;
    memcpy(&k, &v, 8);
    return k;
}
SRX_SFR_HD inline double value_of(uint64_t k)
{
    double v;
    memcpy(&v, &k, 8);
    return v;
}
// does `key` share the digits above `shift + 8` with `prefix` (pass 0, shift 56: every key does)
SRX_SFR_HD inline bool in_prefix(uint64_t key, uint64_t prefix, int shift) { return shift == 56 || (key >> (shift + 8)) == (prefix >> (shift + 8)); }
// one step: hist = the digit counts of the keys that share the prefix; rank = the wanted key's rank among them (0-based).  Returns the digit
// of the wanted key and leaves its rank among the keys that share that digit too.
SRX_SFR_HD inline int select_digit(const unsigned *hist, uint64_t &rank)
{
    uint64_t below = 0;
    for (int d = 0; d < 256; d++) {
        if (rank < below + hist[d]) {
            rank -= below;
            return d;
        }
        below += hist[d];
    }
    rank = 0;  // (rank >= the number of keys: not reached for rank < n)
    return 255;
}
// np.percentile(a, 85) of n values: the lower order statistic's rank and the weight of the upper one
SRX_SFR_HD inline uint64_t percentile_index(uint64_t n, double &t)
{
    SRX_SFR_NO_CONTRACT
    const double virt = (double)(n - 1) * 0.85, fl = floor(virt);
    if (virt >= (double)(n - 1)) {  // n = 1: the last value twice
        t = 0.0;
        return n - 1;
    }
    t = virt - fl;
    return (uint64_t)fl;
}
// numpy's _lerp
SRX_SFR_HD inline double lerp(double a, double b, double t)
{
    SRX_SFR_NO_CONTRACT
    const double d = b - a;
    return t >= 0.5 ? b - d * (1.0 - t) : a + d * t;
}

// ---- line fit from exact sums ------------------------------------------------------------------------------------------------------------
struct I128 {
    uint64_t lo;
    int64_t hi;
};
SRX_SFR_HD inline I128 mul_u64(uint64_t a, uint64_t b)  // a b < 2^127
{
    const uint64_t a0 = a & 0xffffffffu, a1 = a >> 32, b0 = b & 0xffffffffu, b1 = b >> 32;
    const uint64_t p00 = a0 * b0, p01 = a0 * b1, p10 = a1 * b0, p11 = a1 * b1;
    const uint64_t mid = (p00 >> 32) + (p01 & 0xffffffffu) + (p10 & 0xffffffffu);
    I128 r;
    r.lo = (p00 & 0xffffffffu) | (mid << 32);
    r.hi = (int64_t)(p11 + (p01 >> 32) + (p10 >> 32) + (mid >> 32));
    return r;
}
SRX_SFR_HD inline I128 sub_i128(I128 a, I128 b)
{
    I128 r;
    r.lo = a.lo - b.lo;
    r.hi = (int64_t)((uint64_t)a.hi - (uint64_t)b.hi - (a.lo < b.lo ? 1u : 0u));
    return r;
}
// round to nearest even; a value that fits 64 bits goes through the 64-bit conversion itself
SRX_SFR_HD inline double i128_to_double(I128 v)
{
    if ((v.hi == 0 && !(v.lo >> 63)) || (v.hi == -1 && (v.lo >> 63)))
        return (double)(int64_t)v.lo;
    const bool neg = v.hi < 0;
    uint64_t mh = (uint64_t)v.hi, ml = v.lo;
    if (neg) {
        ml = ~ml + 1;
        mh = ~mh + (ml == 0 ? 1u : 0u);
    }
    int s = 0;  // the magnitude's top bit sits at 63 + s
    if (mh) {
        s = 64;
        while (!(mh >> 63))
            mh = (mh << 1) | (ml >> 63), ml <<= 1, s--;
        // mh: the top 64 bits; ml: what is left of the rest (sticky)
        mh |= ml ? 1u : 0u;
    } else {
        mh = ml;
    }
    double d = (double)mh;
    for (int i = 0; i < s; i++)
        d *= 2.0;
    return neg ? -d : d;
}
struct FitSums {
    uint64_t n, su, sv, suu, suv;
};
// v = m u + b by least squares; false: the u have no spread (or n = 0)
SRX_SFR_HD inline bool line_fit(const FitSums &s, double &m, double &b)
{
    SRX_SFR_NO_CONTRACT
    const I128 den = sub_i128(mul_u64(s.n, s.suu), mul_u64(s.su, s.su));
    if (s.n == 0 || (den.hi == 0 && den.lo == 0))
        return false;
    const I128 num = sub_i128(mul_u64(s.n, s.suv), mul_u64(s.su, s.sv));
    m = i128_to_double(num) / i128_to_double(den);
    b = ((double)s.sv - m * (double)s.su) / (double)s.n;
    return true;
}

// ---- projection and bins --------------------------------------------------------------------------------------------------------------
SRX_SFR_HD inline double line_norm(double m)
{
    SRX_SFR_NO_CONTRACT
    return sqrt(1.0 + m * m);
}
SRX_SFR_HD inline double line_dist(double u, double v, double m, double b, double norm)
{
    SRX_SFR_NO_CONTRACT
    return (v - m * u - b) / norm;
}
SRX_SFR_HD inline double bin_edge(double lo, int i)
{
    SRX_SFR_NO_CONTRACT
    return lo + (double)i * BIN_WIDTH;
}
// len(np.arange(lo, hi + 1/4, 1/4)), held to [0, MAX_BINS + 1]
SRX_SFR_HD inline int edge_count(double lo, double hi)
{
    SRX_SFR_NO_CONTRACT
    const double c = ceil(((hi + BIN_WIDTH) - lo) / BIN_WIDTH);
    return !(c > 0.0) ? 0 : (c > (double)(MAX_BINS + 1) ? MAX_BINS + 1 : (int)c);
}
// rows of a H-row ROI per group, for G = min(H, MAX_GROUPS) groups
SRX_SFR_HD inline int bin_groups(int H) { return H < MAX_GROUPS ? H : MAX_GROUPS; }
SRX_SFR_HD inline int group_rows(int H) { return (H + bin_groups(H) - 1) / bin_groups(H); }

// ---- the 72-sample tail ---------------------------------------------------------------------------------------------------------------
// sums and counts of nbin bins -> esf x[nbin], y[nbin]: the means, the empty bins filled as np.interp fills them over the non-empty ones
// (end values held), both reversed (x negated) if the ESF falls.  Returns ST_OK, or ST_FEW_BINS (nbin < 4 or fewer than 3 non-empty bins).
SRX_SFR_HD inline int esf_from_bins(const double *sum, const double *cnt, int nbin, double lo, double *x, double *y, int &flipped)
{
    SRX_SFR_NO_CONTRACT
    flipped = 0;
    int nvalid = 0;
    for (int i = 0; i < nbin; i++) {
        x[i] = 0.5 * (bin_edge(lo, i) + bin_edge(lo, i + 1));
        y[i] = cnt[i] > 0.0 ? sum[i] / cnt[i] : nan_value();
        nvalid += cnt[i] > 0.0 ? 1 : 0;
    }
    if (nbin < 4 || nvalid < 3)
        return ST_FEW_BINS;
    int first = 0, last = nbin - 1;
    while (!(cnt[first] > 0.0))
        first++;
    while (!(cnt[last] > 0.0))
        last--;
    for (int i = 0; i < first; i++)
        y[i] = y[first];
    for (int i = last + 1; i < nbin; i++)
        y[i] = y[last];
    for (int j0 = first; j0 < last;) {
        int j1 = j0 + 1;
        while (!(cnt[j1] > 0.0))
            j1++;
        if (j1 > j0 + 1) {
            const double slope = (y[j1] - y[j0]) / (x[j1] - x[j0]);
            for (int i = j0 + 1; i < j1; i++)
                y[i] = slope * (x[i] - x[j0]) + y[j0];
        }
        j0 = j1;
    }
    if (y[nbin - 1] < y[0]) {
        flipped = 1;
        for (int i = 0, j = nbin - 1; i <= j; i++, j--) {
            const double xi = x[i], yi = y[i];
            x[i] = -x[j], y[i] = y[j];
            x[j] = -xi, y[j] = yi;
        }
    }
    return ST_OK;
}
// np.gradient(y, x)[i] * np.hanning(n)[i]; n >= 2
SRX_SFR_HD inline double lsf_windowed_at(const double *x, const double *y, int n, int i)
{
    SRX_SFR_NO_CONTRACT
    const double pi = 3.141592653589793;
    double g;
    if (i == 0) {
        g = (y[1] - y[0]) / (x[1] - x[0]);
    } else if (i == n - 1) {
        g = (y[n - 1] - y[n - 2]) / (x[n - 1] - x[n - 2]);
    } else {
        const double dx1 = x[i] - x[i - 1], dx2 = x[i + 1] - x[i];
        const double a = -(dx2) / (dx1 * (dx1 + dx2)), b = (dx2 - dx1) / (dx1 * dx2), c = dx1 / (dx2 * (dx1 + dx2));
        g = a * y[i - 1] + b * y[i] + c * y[i + 1];
    }
    const double w = 0.5 + 0.5 * cos(pi * (double)(1 - n + 2 * i) / (double)(n - 1));
    return g * w;
}
SRX_SFR_HD inline void lsf_windowed(const double *x, const double *y, int n, double *wl)
{
    for (int i = 0; i < n; i++)
        wl[i] = lsf_windowed_at(x, y, n, i);
}
// the twiddle of index r = (j k) mod n: cos and sin of 2 pi r / n.  Only n of them exist, so the kernel keeps them in a table
SRX_SFR_HD inline void twiddle(int r, int n, double &c, double &s)
{
    SRX_SFR_NO_CONTRACT
    const double two_pi = 6.283185307179586;
    const double a = two_pi * (double)r / (double)n;
    c = cos(a), s = sin(a);
}
// |sum_j wl[j] exp(-2 pi i j k / n)|, j ascending, from the table cs[r], sn[r] = twiddle(r, n)
SRX_SFR_HD inline double dft_abs_table(const double *wl, int n, int k, const double *cs, const double *sn)
{
    SRX_SFR_NO_CONTRACT
    double re = 0.0, im = 0.0;
    for (int j = 0; j < n; j++) {
        const int r = (j * k) % n;
        re += wl[j] * cs[r];
        im -= wl[j] * sn[r];
    }
    return sqrt(re * re + im * im);
}
// the same sum with every twiddle evaluated where it is used: the same values, so the same bits
SRX_SFR_HD inline double dft_abs(const double *wl, int n, int k)
{
    SRX_SFR_NO_CONTRACT
    double re = 0.0, im = 0.0;
    for (int j = 0; j < n; j++) {
        double c, s;
        twiddle((j * k) % n, n, c, s);
        re += wl[j] * c;
        im -= wl[j] * s;
    }
    return sqrt(re * re + im * im);
}
// mtf[nh] normalised to its DC value if that is positive; freq[k] = np.fft.fftfreq(n, mean(diff(x)))[k]
SRX_SFR_HD inline void mtf_finish(double *mtf, int nh, const double *x, int n, double *freq)
{
    SRX_SFR_NO_CONTRACT
    const double dc = mtf[0];
    if (dc > 0.0)
        for (int k = 0; k < nh; k++)
            mtf[k] = mtf[k] / dc;
    double s = 0.0;
    for (int i = 0; i + 1 < n; i++)
        s += x[i + 1] - x[i];
    const double val = 1.0 / ((double)n * (s / (double)(n - 1)));
    for (int k = 0; k < nh; k++)
        freq[k] = (double)k * val;
}
// metrics.mtf_at_fraction over the samples k >= 1 (the report drops the DC sample)
SRX_SFR_HD inline double mtf_crossing(const double *freq, const double *mtf, int nh, double fraction)
{
    SRX_SFR_NO_CONTRACT
    for (int k = 1; k + 1 < nh; k++) {
        if (!(mtf[k] < fraction) && mtf[k + 1] < fraction) {
            const double rise = mtf[k + 1] - mtf[k], run = freq[k + 1] - freq[k];
            return fabs(rise) < 1e-12 ? freq[k] : freq[k] + (fraction - mtf[k]) * run / rise;
        }
    }
    return nan_value();
}
SRX_SFR_HD inline double edge_angle_deg(double m, int rows_are_x)
{
    SRX_SFR_NO_CONTRACT
    return (rows_are_x ? atan2(1.0, m) : atan2(m, 1.0)) * (180.0 / 3.141592653589793);
}

}  // namespace sfr
}  // namespace srx

#if defined(__HIPCC__) && !defined(SRX_SFR_HOST_ONLY)
#include "srx_common.h"

namespace srx {
namespace sfr {

// The record of an item while the call runs: SUMMARY doubles in the workspace, laid out as the summary, with the status in slot S_MTF50
// and the norm sqrt(1 + m^2) in slot S_MTF10 until k_sfr_tail writes the outputs.
constexpr int R_STATUS = S_MTF50, R_NORM = S_MTF10;
constexpr int FIT_THREADS = 1024;

// ---- 1 - 3: the magnitude plane, batched; a thread per pixel, grid (ceil(H W / 256), B) ---------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(256) k_sfr_smooth0(const T *__restrict__ img, int H, int W, size_t row_pitch, size_t item_pitch, Taps17 t,
                                                     double *__restrict__ out)
{
    const int i = blockIdx.x * 256 + threadIdx.x, n = H * W;
    if (i >= n)
        return;
    const int y = i / W, x = i - y * W;
    const T *p = img + (size_t)blockIdx.y * item_pitch;
    out[(size_t)blockIdx.y * n + i] = correlate_at(t, 0, y, x, H, W, [&](int yy, int xx) { return (double)p[(size_t)yy * row_pitch + xx]; });
}
__global__ void __launch_bounds__(256) k_sfr_smooth1(const double *__restrict__ in, int H, int W, Taps17 t, double *__restrict__ out)
{
    const int i = blockIdx.x * 256 + threadIdx.x, n = H * W;
    if (i >= n)
        return;
    const int y = i / W, x = i - y * W;
    const double *p = in + (size_t)blockIdx.y * n;
    out[(size_t)blockIdx.y * n + i] = correlate_at(t, 1, y, x, H, W, [&](int yy, int xx) { return p[(size_t)yy * W + xx]; });
}
__global__ void __launch_bounds__(256) k_sfr_sobel(const double *__restrict__ in, int H, int W, double *__restrict__ mag)
{
    const int i = blockIdx.x * 256 + threadIdx.x, n = H * W;
    if (i >= n)
        return;
    const int y = i / W, x = i - y * W;
    const double *p = in + (size_t)blockIdx.y * n;
    mag[(size_t)blockIdx.y * n + i] = sobel_mag_at(y, x, H, W, [&](int yy, int xx) { return p[(size_t)yy * W + xx]; });
}

// ---- 4: one workgroup per item: threshold, edge pixels, the two fits, the distance range -------------------------------------------------
// Every thread evaluates the few scalar steps between the passes from the same LDS values, so the branches on the status are uniform.
// The histograms and the integer sums are LDS atomics on integers: whatever their order, the same value.
__global__ void __launch_bounds__(FIT_THREADS) k_sfr_fit(const double *__restrict__ mag_all, int H, int W, int side, double *__restrict__ rec_all)
{
    __shared__ unsigned hist[256];
    __shared__ unsigned long long acc[6], next_key;
    __shared__ int mm[4];
    __shared__ double dmin[FIT_THREADS / 64], dmax[FIT_THREADS / 64];
    const int tid = threadIdx.x, n = H * W;
    const double *mag = mag_all + (size_t)blockIdx.x * n;
    double *rec = rec_all + (size_t)blockIdx.x * SUMMARY;

    // threshold = np.percentile(mag, 85)
    double t;
    uint64_t rank = percentile_index((uint64_t)n, t), prefix = 0;
    unsigned equal = 0;
    for (int shift = 56; shift >= 0; shift -= 8) {
        if (tid < 256)
            hist[tid] = 0;
        __syncthreads();
        // a thread adds a run of equal digits at once: the top digits (sign and exponent) are the same for nearly every magnitude, and
        // one atomic per element on one LDS word would serialise the whole pass
        int run_digit = 0;
        unsigned run = 0;
        for (int i = tid; i < n; i += FIT_THREADS) {
            const uint64_t key = key_of(mag[i]);
            if (in_prefix(key, prefix, shift)) {
                const int d = (int)((key >> shift) & 255);
                if (run && d != run_digit)
                    atomicAdd(&hist[run_digit], run), run = 0;
                run_digit = d, run++;
            }
        }
        if (run)
            atomicAdd(&hist[run_digit], run);
        __syncthreads();
        const int d = select_digit(hist, rank);
        equal = hist[d];
        prefix |= (uint64_t)d << shift;
        __syncthreads();
    }
    // the next order statistic: the same value if more of them are left (ties), else the smallest larger one
    if (tid == 0)
        next_key = ~0ull;
    __syncthreads();
    {
        unsigned long long mn = ~0ull;
        for (int i = tid; i < n; i += FIT_THREADS) {
            const uint64_t key = key_of(mag[i]);
            if (key > prefix && key < mn)
                mn = key;
        }
        if (mn != ~0ull)
            atomicMin(&next_key, mn);
    }
    if (tid < 6)
        acc[tid] = 0;
    if (tid == 0)
        mm[0] = mm[2] = 0x7fffffff, mm[1] = mm[3] = -1;
    __syncthreads();
    const uint64_t upper = (rank + 1 < equal || next_key == ~0ull) ? prefix : (uint64_t)next_key;
    const double thr = lerp(value_of(prefix), value_of(upper), t);

    // edge pixels: mag > threshold
    {
        unsigned long long a[6] = {0, 0, 0, 0, 0, 0};
        int r0 = 0x7fffffff, r1 = -1, c0 = 0x7fffffff, c1 = -1;
        for (int i = tid; i < n; i += FIT_THREADS) {
            if (mag[i] > thr) {
                const int r = i / W, c = i - r * W;
                const unsigned long long ur = r, uc = c;
                a[0] += 1, a[1] += ur, a[2] += uc, a[3] += ur * ur, a[4] += uc * uc, a[5] += ur * uc;
                r0 = min(r0, r), r1 = max(r1, r), c0 = min(c0, c), c1 = max(c1, c);
            }
        }
        if (a[0]) {
#pragma unroll
            for (int j = 0; j < 6; j++)
                atomicAdd(&acc[j], a[j]);
            atomicMin(&mm[0], r0), atomicMax(&mm[1], r1), atomicMin(&mm[2], c0), atomicMax(&mm[3], c1);
        }
    }
    __syncthreads();
    const double nanv = nan_value();
    const unsigned long long n_edge = acc[0];
    int status = ST_OK, rax = 0;
    double m_c = nanv, b_c = nanv, m = nanv, b = nanv, norm = nanv, lo = nanv, hi = nanv, n_side = nanv, nbin = nanv;
    if (n_edge < 20) {
        status = ST_FEW_EDGE;
    } else {
        rax = (mm[1] - mm[0]) >= (mm[3] - mm[2]);
        const FitSums s = rax ? FitSums{n_edge, acc[1], acc[2], acc[3], acc[5]} : FitSums{n_edge, acc[2], acc[1], acc[4], acc[5]};
        if (!line_fit(s, m_c, b_c))
            status = ST_DEGENERATE;
    }
    __syncthreads();
    // the pixels on the chosen side of the centre line, re-fitted
    if (status == ST_OK) {
        if (tid < 6)
            acc[tid] = 0;
        __syncthreads();
        const double norm_c = line_norm(m_c);
        unsigned long long a[5] = {0, 0, 0, 0, 0};
        for (int i = tid; i < n; i += FIT_THREADS) {
            if (mag[i] > thr) {
                const int r = i / W, c = i - r * W;
                const unsigned long long u = rax ? r : c, v = rax ? c : r;
                const double d = line_dist((double)u, (double)v, m_c, b_c, norm_c);
                if (side == 0 ? d < 0.0 : d > 0.0)
                    a[0] += 1, a[1] += u, a[2] += v, a[3] += u * u, a[4] += u * v;
            }
        }
        if (a[0]) {
#pragma unroll
            for (int j = 0; j < 5; j++)
                atomicAdd(&acc[j], a[j]);
        }
        __syncthreads();
        n_side = (double)acc[0];
        if (acc[0] < 10)
            status = ST_FEW_SIDE;
        else if (!line_fit(FitSums{acc[0], acc[1], acc[2], acc[3], acc[4]}, m, b))
            status = ST_DEGENERATE;
    }
    // min and max of the distances in (-8, 10) over the whole ROI
    if (status == ST_OK) {
        norm = line_norm(m);
        double mn = 1e300, mx = -1e300;
        for (int i = tid; i < n; i += FIT_THREADS) {
            const int r = i / W, c = i - r * W;
            const double d = line_dist((double)(rax ? r : c), (double)(rax ? c : r), m, b, norm);
            if (d > -8.0 && d < 10.0)
                mn = fmin(mn, d), mx = fmax(mx, d);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1)
            mn = fmin(mn, __shfl_down(mn, o, 64)), mx = fmax(mx, __shfl_down(mx, o, 64));
        if ((tid & 63) == 0)
            dmin[tid >> 6] = mn, dmax[tid >> 6] = mx;
        __syncthreads();
        mn = dmin[0], mx = dmax[0];
        for (int w = 1; w < FIT_THREADS / 64; w++)
            mn = fmin(mn, dmin[w]), mx = fmax(mx, dmax[w]);
        if (mn > mx) {
            status = ST_DEGENERATE;  // no pixel within (-8, 10) of the line
        } else {
            lo = mn, hi = mx;
            const int nb = edge_count(lo, hi) - 1;
            nbin = (double)nb;
            if (nb < 4)
                status = ST_FEW_BINS;
        }
    }
    if (tid == 0) {
        rec[R_STATUS] = (double)status, rec[R_NORM] = norm, rec[S_ANGLE] = nanv, rec[S_M] = m, rec[S_B] = b;
        rec[S_ROWS_ARE_X] = n_edge < 20 ? nanv : (double)rax, rec[S_THRESHOLD] = thr, rec[S_N_EDGE] = (double)n_edge, rec[S_N_SIDE] = n_side;
        rec[S_NBIN] = nbin, rec[S_LO] = lo, rec[S_HI] = hi, rec[S_FLIPPED] = nanv, rec[S_MC] = m_c, rec[S_BC] = b_c, rec[S_ZERO] = 0.0;
    }
}

// ---- 5: the bin sums.  grid (G, B), block 128: group g of rows, a thread per bin walks the group's pixels in raster order ------------------
template <typename T>
__global__ void __launch_bounds__(128) k_sfr_bins(const T *__restrict__ img, int H, int W, size_t row_pitch, size_t item_pitch,
                                                  const double *__restrict__ rec_all, double *__restrict__ part_all)
{
    SRX_SFR_NO_CONTRACT
    const int g = blockIdx.x, G = gridDim.x, b = blockIdx.y, i = threadIdx.x;
    const double *rec = rec_all + (size_t)b * SUMMARY;
    if (rec[R_STATUS] != 0.0)
        return;
    const int nbin = (int)rec[S_NBIN];
    if (i >= nbin || i >= MAX_BINS)
        return;
    const double m = rec[S_M], lb = rec[S_B], norm = rec[R_NORM], lo = rec[S_LO];
    const int rax = (int)rec[S_ROWS_ARE_X];
    const int rp = (H + G - 1) / G, y0 = g * rp, y1 = min(y0 + rp, H);
    const T *p = img + (size_t)b * item_pitch;
    const double e0 = bin_edge(lo, i), e1 = bin_edge(lo, i + 1);
    double s = 0.0, c = 0.0;
    for (int y = y0; y < y1; y++) {
        for (int x = 0; x < W; x++) {
            const double d = line_dist((double)(rax ? y : x), (double)(rax ? x : y), m, lb, norm);
            if (d > -8.0 && d < 10.0 && d >= e0 && d < e1)
                s += (double)p[(size_t)y * row_pitch + x], c += 1.0;
        }
    }
    double *part = part_all + ((size_t)b * G + g) * 2 * MAX_BINS;
    part[i] = s, part[MAX_BINS + i] = c;
}

// ---- 6: one workgroup per item: the groups added in index order, ESF, LSF, DFT, crossings, and every output ---------------------------------
__global__ void __launch_bounds__(128) k_sfr_tail(const double *__restrict__ rec_all, const double *__restrict__ part_all, int G,
                                                  double *__restrict__ summary, double *__restrict__ esf, double *__restrict__ mtf,
                                                  int *__restrict__ status_out)
{
    __shared__ double sum[MAX_BINS], cnt[MAX_BINS], x[MAX_BINS], y[MAX_BINS], wl[MAX_BINS], mt[MAX_BINS / 2], fr[MAX_BINS / 2];
    __shared__ double cs[MAX_BINS], sn[MAX_BINS], sm[SUMMARY];
    __shared__ int s_status;
    const int tid = threadIdx.x, b = blockIdx.x;
    const double *rec = rec_all + (size_t)b * SUMMARY;
    int status = (int)rec[R_STATUS];
    const int nbin = status == ST_OK ? min((int)rec[S_NBIN], MAX_BINS) : 0, nh = nbin / 2;
    if (tid < SUMMARY)
        sm[tid] = rec[tid];
    if (status == ST_OK) {
        if (tid < nbin) {
            const double *part = part_all + (size_t)b * G * 2 * MAX_BINS;
            double s = 0.0, c = 0.0;
            for (int g = 0; g < G; g++)
                s += part[(size_t)g * 2 * MAX_BINS + tid], c += part[(size_t)g * 2 * MAX_BINS + MAX_BINS + tid];
            sum[tid] = s, cnt[tid] = c;
        }
        __syncthreads();
        if (tid == 0) {
            int flipped = 0;
            s_status = esf_from_bins(sum, cnt, nbin, rec[S_LO], x, y, flipped);
            if (s_status == ST_OK)
                sm[S_FLIPPED] = (double)flipped;
        }
        __syncthreads();
        status = s_status;
        if (status == ST_OK) {
            if (tid < nbin) {  // a thread per LSF sample and per twiddle: only nbin distinct angles exist
                wl[tid] = lsf_windowed_at(x, y, nbin, tid);
                twiddle(tid, nbin, cs[tid], sn[tid]);
            }
            __syncthreads();
            if (tid < nh)
                mt[tid] = dft_abs_table(wl, nbin, tid, cs, sn);
            __syncthreads();
            if (tid == 0)
                mtf_finish(mt, nh, x, nbin, fr);
        }
    }
    __syncthreads();
    if (tid == 0) {
        const double nanv = nan_value();
        const bool ok = status == ST_OK, line = ok || (status == ST_FEW_BINS);
        sm[S_MTF50] = ok ? mtf_crossing(fr, mt, nh, 0.5) : nanv;
        sm[S_MTF10] = ok ? mtf_crossing(fr, mt, nh, 0.1) : nanv;
        sm[S_ANGLE] = line ? edge_angle_deg(sm[S_M], (int)sm[S_ROWS_ARE_X]) : nanv;
        status_out[b] = status;
    }
    __syncthreads();
    if (tid < SUMMARY)
        summary[(size_t)b * SUMMARY + tid] = sm[tid];
    // a failed item: NaN throughout; else zeros behind nbin / nbin / 2
    const bool ok = status == ST_OK;
    if (esf) {
        double *e = esf + (size_t)b * 2 * MAX_BINS;
        for (int i = tid; i < MAX_BINS; i += 128) {
            e[i] = !ok ? nan_value() : (i < nbin ? x[i] : 0.0);
            e[MAX_BINS + i] = !ok ? nan_value() : (i < nbin ? y[i] : 0.0);
        }
    }
    if (mtf) {
        double *q = mtf + (size_t)b * MAX_BINS;
        for (int i = tid; i < MAX_BINS / 2; i += 128) {
            q[i] = !ok ? nan_value() : (i < nh ? fr[i] : 0.0);
            q[MAX_BINS / 2 + i] = !ok ? nan_value() : (i < nh ? mt[i] : 0.0);
        }
    }
}

// ---- host -----------------------------------------------------------------------------------------------------------------------------
struct Carve {
    double *a, *b, *rec, *part;
};
static Carve carve(Arena &ar, size_t B, size_t H, size_t W)
{
    Carve c;
    c.a = ar.take<double>(B * H * W);
    c.b = ar.take<double>(B * H * W);
    c.rec = ar.take<double>(B * SUMMARY);
    c.part = ar.take<double>(B * (size_t)bin_groups((int)H) * 2 * MAX_BINS);
    return c;
}
static inline bool supported(int B, int H, int W) { return B > 0 && H > 0 && W > 0 && (size_t)H * (size_t)W <= ((size_t)1 << 20) && B <= 65535; }
static inline size_t scratch_bytes(int B, int H, int W)
{
    if (!supported(B, H, W))
        return 0;
    return measured([&](Arena &m) { carve(m, B, H, W); });
}

template <typename T>
static int edge_sfr(const T *img, int B, int H, int W, size_t row_pitch, size_t item_pitch, int side, double sigma, void *summary, void *esf, void *mtf,
                    void *status, void *ws, size_t wsb, hipStream_t st)
{
    if (!img || !summary || !status || B <= 0 || H <= 0 || W <= 0 || row_pitch < (size_t)W ||
        (B > 1 && item_pitch < (size_t)(H - 1) * row_pitch + (size_t)W) || (side != 0 && side != 1) || !(sigma > 0.0))
        return SRX_E_INVALID;
    Taps17 t;
    if (!supported(B, H, W) || !gaussian_taps(sigma, t))
        return SRX_E_UNSUPPORTED;
    Arena ar(ws, wsb);
    ar.require(scratch_bytes(B, H, W));
    const Carve c = carve(ar, B, H, W);
    if (!ar.ok)
        return SRX_E_WORKSPACE;
    const int n = H * W, G = bin_groups(H);
    const dim3 px(cdiv(n, 256), B);
    hipLaunchKernelGGL(k_sfr_smooth0<T>, px, dim3(256), 0, st, img, H, W, row_pitch, item_pitch, t, c.a);  // metrics._gaussian_filter: axis 0 first
    SRX_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_sfr_smooth1, px, dim3(256), 0, st, c.a, H, W, t, c.b);
    SRX_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_sfr_sobel, px, dim3(256), 0, st, c.b, H, W, c.a);
    SRX_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_sfr_fit, dim3(B), dim3(FIT_THREADS), 0, st, c.a, H, W, side, c.rec);
    SRX_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_sfr_bins<T>, dim3(G, B), dim3(128), 0, st, img, H, W, row_pitch, item_pitch, c.rec, c.part);
    SRX_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_sfr_tail, dim3(B), dim3(128), 0, st, c.rec, c.part, G, (double *)summary, (double *)esf, (double *)mtf, (int *)status);
    SRX_CHECK_LAUNCH();
    return SRX_OK;
}

}  // namespace sfr
}  // namespace srx
#endif
