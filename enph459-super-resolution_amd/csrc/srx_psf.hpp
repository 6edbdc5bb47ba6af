// srx_psf.hpp -- the measured PSF from pinhole frames on the device (load_measured_psf, mono_cal_target/run_sr.py:114-152): frames
// [N, H, W] of uint8 / float / double -> the normalised (2 halfwidth + 1)^2 kernel in float64.  Three launches, no host synchronisation.
//
//   k_psf_argmax  grid (chunks of a frame, N), block 256: the bandwidth kernel.  A chunk is CHUNK_BYTES = 32 KiB of one frame (a fixed
//                 range of sample indices, so the decomposition never depends on the pointer).  The caller's frame pointer has only element
//                 alignment and H W may be odd, so frame k of a uint8 stack starts at any byte: every block peels the samples in front of
//                 its chunk's first 16-byte boundary (< 16 B: one per lane) and those behind the last whole vector, and reads what lies
//                 between as aligned 16-byte vectors, 8 per lane, all issued before the first is used (32 KiB in flight per block).  The
//                 winner is found in two sweeps over those registers: the maximum (uint8: four samples per v_pk_max_u16 pair; floats: a
//                 compare that a NaN never passes), reduced over the block by shuffles and 4 LDS words; then, in the lanes that hold it,
//                 the first sample EQUAL to it (uint8: the zero-byte test on a dword xor the broadcast maximum; `==` for floats, so that
//                 -0.0 ties +0.0), reduced as a minimum index.  One (value, first index) partial per block goes to the workspace.
//   k_psf_pick    grid N, block 256: the frame's winner over its partials (larger value, then smaller index), peak = (idx / W, idx % W),
//                 used = the window of +-reach around it lies inside the frame.  No winning sample (all NaN): peak (0, 0).
//   k_psf_window  one block, one thread per pixel of the (2 reach + 1)^2 window: the used frames' windows added in frame order in float64 and
//                 divided by their number (bit for bit numpy's stack.mean(axis=0)); the central side x side cut; the mean of the 36
//                 samples core[ix_(e, e)], e = r_[0:3, side-3:side] (repeats included when side < 6) taken off; negatives clipped; sum 1.
//                 The two sums follow numpy's order for a contiguous reduction (eight running sums over strides of 8, paired, then the
//                 rest in turn; halves first above 128 terms), so a float64 stack gives the host form's bits.
#pragma once
#include "srx_common.h"

namespace srx {
namespace psf {

constexpr int EXTRA_REACH = 6;                    // the reference's margin around the kernel: reach = halfwidth + 6
constexpr int MAX_HALFWIDTH = 7;                  // side 15: SRX_MAX_KERNEL_TAPS
constexpr int BLK = 256, VPT = 8;                 // argmax block: 8 vectors of 16 bytes per lane
constexpr int CHUNK_BYTES = BLK * VPT * 16;       // 32 KiB of one frame per block
constexpr unsigned NONE = 0xffffffffu;            // no sample of this chunk can win (all NaN)
constexpr int WBATCH = 64, WUNROLL = 16;          // window stage: peaks staged per trip (3 WBATCH <= its smallest block, 15^2 -> 256), loads in flight
constexpr int MAX_SIDE = 2 * MAX_HALFWIDTH + 1;   // 15; the window is at most 27 x 27 = 729 threads

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef double f64x2 __attribute__((ext_vector_type(2)));
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));

// per sample type: the 16-byte vector, the type the maximum is carried in, and the two sweeps over one vector
template <typename T> struct Sweep;

template <> struct Sweep<uint8_t> {
    typedef u32x4 Vec;
    typedef unsigned Max;  // two 16-bit running maxima while sweeping; one value after fold()
    static constexpr int VE = 16;
    __device__ static Max lowest() { return 0u; }
    __device__ static Max pk_max(Max a, unsigned b)
    {
        const u16x2 r = __builtin_elementwise_max(__builtin_bit_cast(u16x2, a), __builtin_bit_cast(u16x2, b));
        return __builtin_bit_cast(unsigned, r);
    }
    __device__ static Max take(Max m, uint8_t v) { return pk_max(m, (unsigned)v); }
    __device__ static Max take(Max m, const Vec &x)
    {
#pragma unroll
        for (int d = 0; d < 4; d++) {
            m = pk_max(m, x[d] & 0x00ff00ffu);
            m = pk_max(m, (x[d] >> 8) & 0x00ff00ffu);
        }
        return m;
    }
    __device__ static Max fold(Max m) { return max(m & 0xffffu, m >> 16); }
    __device__ static Max larger(Max a, Max b) { return max(a, b); }
    __device__ static bool equal(uint8_t v, Max m) { return (unsigned)v == m; }
    // first sample of x equal to m, or VE.  y = dword xor the broadcast m has a zero byte where a sample matches; in
    // (y - 0x01010101) & ~y & 0x80808080 the lowest set bit marks the lowest zero byte exactly (a borrow can only raise false flags above it)
    __device__ static int first(const Vec &x, Max m)
    {
        const unsigned mm = m * 0x01010101u;
        int r = VE;
#pragma unroll
        for (int d = 3; d >= 0; d--) {
            const unsigned y = x[d] ^ mm, fl = (y - 0x01010101u) & ~y & 0x80808080u;
            if (fl)
                r = 4 * d + (__builtin_ctz(fl) >> 3);
        }
        return r;
    }
    __device__ static double value(Max m) { return (double)m; }
};

template <typename F, typename V, int N> struct SweepFloat {
    typedef V Vec;
    typedef F Max;
    static constexpr int VE = N;
    __device__ static Max lowest() { return -__builtin_huge_val(); }
    __device__ static Max take(Max m, F v) { return v > m ? v : m; }  // false for a NaN: it never wins
    __device__ static Max take(Max m, const Vec &x)
    {
#pragma unroll
        for (int e = 0; e < N; e++)
            m = take(m, x[e]);
        return m;
    }
    __device__ static Max fold(Max m) { return m; }
    __device__ static Max larger(Max a, Max b) { return b > a ? b : a; }
    __device__ static bool equal(F v, Max m) { return v == m; }
    __device__ static int first(const Vec &x, Max m)
    {
        int r = N;
#pragma unroll
        for (int e = N - 1; e >= 0; e--)
            if (x[e] == m)
                r = e;
        return r;
    }
    __device__ static double value(Max m) { return (double)m; }
};
template <> struct Sweep<float> : SweepFloat<float, f32x4, 4> {};
template <> struct Sweep<double> : SweepFloat<double, f64x2, 2> {};

static inline int chunks_of(size_t frame_bytes) { return (int)((frame_bytes + CHUNK_BYTES - 1) / CHUNK_BYTES); }

// ---- stage 1: grid (chunks, N), block 256 -> one (maximum, first index) per block --------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(BLK) k_psf_argmax(const T *__restrict__ frames, unsigned HW, double *__restrict__ pval, unsigned *__restrict__ pidx)
{
    typedef Sweep<T> S;
    typedef typename S::Vec Vec;
    typedef typename S::Max Max;
    constexpr int VE = S::VE;
    constexpr unsigned CHUNK = CHUNK_BYTES / sizeof(T);
    __shared__ Max smax[BLK / 64];
    __shared__ unsigned sidx[BLK / 64];
    const unsigned tid = threadIdx.x;
    const T *f = frames + (size_t)blockIdx.y * HW;
    const unsigned lo = blockIdx.x * CHUNK, hi = min(lo + CHUNK, HW);  // HW sizeof(T) < 2^31: no wrap
    // [lo, lo + head) scalar | nvec aligned vectors | [tail0, hi) scalar; head, tail < VE <= 16 samples: one per lane
    const unsigned head = min((unsigned)((16u - (unsigned)((uintptr_t)(f + lo) & 15u)) & 15u) / (unsigned)sizeof(T), hi - lo);
    const unsigned nvec = (hi - lo - head) / VE, body = lo + head, tail0 = body + nvec * VE;
    const Vec *vp = (const Vec *)(f + body);  // 16-byte aligned by construction
    const bool has_head = tid < head, has_tail = tail0 + tid < hi;
    // vector j of this lane is min(j BLK + tid, nvec - 1): past the end of a short chunk a lane reads the last vector again (samples of this
    // chunk at their own index, so both sweeps may take them), and no load or sweep carries a predicate
    Vec x[VPT];
    unsigned vi[VPT];
    T eh = (T)0, et = (T)0;
    if (nvec) {
#pragma unroll
        for (int j = 0; j < VPT; j++) {
            vi[j] = min(j * BLK + tid, nvec - 1u);
            x[j] = vp[vi[j]];
        }
    }
    if (has_head)
        eh = f[lo + tid];
    if (has_tail)
        et = f[tail0 + tid];
    // sweep 1: the maximum
    Max m = S::lowest();
    if (nvec) {
#pragma unroll
        for (int j = 0; j < VPT; j++)
            m = S::take(m, x[j]);
    }
    if (has_head)
        m = S::take(m, eh);
    if (has_tail)
        m = S::take(m, et);
    m = S::fold(m);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
        m = S::larger(m, __shfl_xor(m, o, 64));
    if ((tid & 63) == 0)
        smax[tid >> 6] = m;
    __syncthreads();
    const Max M = S::larger(S::larger(smax[0], smax[1]), S::larger(smax[2], smax[3]));
    // sweep 2, in the lanes that hold it: the first sample equal to it (descending, so that the smallest index is assigned last)
    unsigned idx = NONE;
    if (m == M) {
        if (has_tail && S::equal(et, M))
            idx = tail0 + tid;
        if (nvec) {
#pragma unroll
            for (int j = VPT - 1; j >= 0; j--) {
                const int r = S::first(x[j], M);
                if (r < VE)
                    idx = body + vi[j] * VE + r;
            }
        }
        if (has_head && S::equal(eh, M))
            idx = lo + tid;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
        idx = min(idx, (unsigned)__shfl_xor(idx, o, 64));
    if ((tid & 63) == 0)
        sidx[tid >> 6] = idx;
    __syncthreads();
    if (tid == 0) {
        const size_t p = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
        pval[p] = S::value(M);
        pidx[p] = min(min(sidx[0], sidx[1]), min(sidx[2], sidx[3]));
    }
}

// ---- stage 2: grid N, block 256: the frame's winner, its peak and whether its window fits ---------------------------------------------------
__global__ void __launch_bounds__(256) k_psf_pick(const double *__restrict__ pval, const unsigned *__restrict__ pidx, int chunks, int H, int W,
                                                  int reach, int *__restrict__ peaks, int *__restrict__ info)
{
    __shared__ double sv[4];
    __shared__ unsigned si[4];
    const int k = blockIdx.x, tid = threadIdx.x;
    double bv = -__builtin_huge_val();
    unsigned bi = NONE;
    auto better = [](double v, unsigned i, double w, unsigned j) { return v > w || (v == w && i < j); };
    for (int c = tid; c < chunks; c += 256) {
        const double v = pval[(size_t)k * chunks + c];
        const unsigned i = pidx[(size_t)k * chunks + c];
        if (better(v, i, bv, bi))
            bv = v, bi = i;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double v = __shfl_xor(bv, o, 64);
        const unsigned i = __shfl_xor(bi, o, 64);
        if (better(v, i, bv, bi))
            bv = v, bi = i;
    }
    if ((tid & 63) == 0)
        sv[tid >> 6] = bv, si[tid >> 6] = bi;
    __syncthreads();
    if (tid == 0) {
        for (int q = 1; q < 4; q++)
            if (better(sv[q], si[q], bv, bi))
                bv = sv[q], bi = si[q];
        const unsigned idx = bi == NONE ? 0u : bi;
        const int row = (int)(idx / (unsigned)W), col = (int)(idx % (unsigned)W);
        const int used = row >= reach && row + reach < H && col >= reach && col + reach < W;
        peaks[3 * k] = row, peaks[3 * k + 1] = col, peaks[3 * k + 2] = used;
        if (info)
            info[3 * k] = row, info[3 * k + 1] = col, info[3 * k + 2] = used;
    }
}

// numpy's sum of n <= 256 contiguous doubles (pairwise_sum: blocks of at most 128 terms in eight running sums)
__device__ static double np_sum_block(const double *a, int n)
{
    if (n < 8) {
        double s = 0.0;
        for (int i = 0; i < n; i++)
            s += a[i];
        return s;
    }
    double r[8];
    for (int j = 0; j < 8; j++)
        r[j] = a[j];
    int i = 8;
    for (; i < n - (n % 8); i += 8)
        for (int j = 0; j < 8; j++)
            r[j] += a[i + j];
    double s = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; i++)
        s += a[i];
    return s;
}
__device__ static double np_sum(const double *a, int n)
{
    if (n <= 128)
        return np_sum_block(a, n);
    int n2 = n / 2;
    n2 -= n2 % 8;
    return np_sum_block(a, n2) + np_sum_block(a + n2, n - n2);
}

// ---- stage 3: one block of win^2 threads (rounded up to whole waves) -------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(768) k_psf_window(const T *__restrict__ frames, int N, int H, int W, int halfwidth, const int *__restrict__ peaks,
                                                    double *__restrict__ psf)
{
    __shared__ double core[MAX_SIDE * MAX_SIDE];
    __shared__ double edge[36];
    __shared__ double scal[2];  // background, clipped sum
    __shared__ int spk[3 * WBATCH];
    const int reach = halfwidth + EXTRA_REACH, side = 2 * halfwidth + 1, win = 2 * reach + 1;
    const int p = threadIdx.x, wy = p / win, wx = p - wy * win;
    const bool live = p < win * win;
    // frames in order, WBATCH peaks staged per trip and WUNROLL independent loads in flight per thread (a load per frame that waits for
    // the one before it costs a memory latency per frame: 0.6 us each, more than the arg-max of a 1536 x 2048 uint8 frame); the adds keep
    // the frame order, and a frame that is not used adds nothing (not even a +0.0)
    double acc = 0.0;
    int cnt = 0;
    for (int k0 = 0; k0 < N; k0 += WBATCH) {
        const int nb = min(WBATCH, N - k0);
        __syncthreads();
        if (p < 3 * nb)
            spk[p] = peaks[3 * (size_t)k0 + p];
        __syncthreads();
        for (int j0 = 0; j0 < nb; j0 += WUNROLL) {
            double v[WUNROLL];
            bool ok[WUNROLL];
#pragma unroll
            for (int u = 0; u < WUNROLL; u++) {
                const int j = min(j0 + u, nb - 1);
                ok[u] = j0 + u < nb && spk[3 * j + 2] != 0;
                const size_t at = ok[u] && live ? (size_t)(k0 + j) * H * W + (size_t)(spk[3 * j] - reach + wy) * W + (spk[3 * j + 1] - reach + wx) : 0;
                v[u] = (double)frames[at];
            }
#pragma unroll
            for (int u = 0; u < WUNROLL; u++) {
                acc = ok[u] ? acc + v[u] : acc;
                cnt += ok[u];
            }
        }
    }
    if (cnt == 0) {  // no frame used: all zeros (block-uniform)
        if (p < side * side)
            psf[p] = 0.0;
        return;
    }
    const int cy = wy - EXTRA_REACH, cx = wx - EXTRA_REACH;
    if (live && cy >= 0 && cy < side && cx >= 0 && cx < side)
        core[cy * side + cx] = acc / (double)cnt;
    __syncthreads();
    if (p < 36) {  // core[np.ix_(e, e)], e = np.r_[0:3, side-3:side]
        const int a = p / 6, b = p - 6 * a;
        const int ey = a < 3 ? a : side - 6 + a, ex = b < 3 ? b : side - 6 + b;
        edge[p] = core[ey * side + ex];
    }
    __syncthreads();
    if (p == 0)
        scal[0] = np_sum(edge, 36) / 36.0;
    __syncthreads();
    const double bg = scal[0];
    double v = 0.0;
    if (p < side * side) {
        v = core[p] - bg;
        v = v < 0.0 ? 0.0 : v;
    }
    __syncthreads();
    if (p < side * side)
        core[p] = v;
    __syncthreads();
    if (p == 0)
        scal[1] = np_sum(core, side * side);
    __syncthreads();
    if (p < side * side)
        psf[p] = v / scal[1];  // 0 / 0 = NaN when nothing is left above the background, as the host form
}

// ---- host -----------------------------------------------------------------------------------------------------------------------------
// 0 ok; otherwise the status the call returns (decided from the arguments alone)
static inline int check_args(int elem_bytes, int N, int H, int W, int halfwidth)
{
    if ((elem_bytes != 1 && elem_bytes != 4 && elem_bytes != 8) || N <= 0 || H <= 0 || W <= 0 || halfwidth < 1 || halfwidth > MAX_HALFWIDTH)
        return SRX_E_INVALID;
    if (N > 65535 || (size_t)H * (size_t)W * (size_t)elem_bytes >= ((size_t)1 << 31))
        return SRX_E_UNSUPPORTED;
    return SRX_OK;
}

// what a call carves: one candidate (value, index) per chunk of every frame, and the frames' peaks; np = N * chunks of a frame
struct Tabs {
    double *pval;
    unsigned *pidx;
    int *peaks;
};
static Tabs carve(Arena &ar, size_t N, size_t np) { return {ar.take<double>(np), ar.take<unsigned>(np), ar.take<int>(N * 3)}; }

static inline size_t workspace_bytes(int elem_bytes, int N, int H, int W, int halfwidth)
{
    if (check_args(elem_bytes, N, H, W, halfwidth) != SRX_OK)
        return 0;
    return measured([&](Arena &m) { carve(m, N, (size_t)N * chunks_of((size_t)H * W * elem_bytes)); });
}

template <typename T>
static int estimate(const T *frames, int N, int H, int W, int halfwidth, double *psf, int *info, void *ws, size_t wsb, hipStream_t st)
{
    if (!frames || !psf)
        return SRX_E_INVALID;
    SRX_TRY(check_args((int)sizeof(T), N, H, W, halfwidth));
    const int chunks = chunks_of((size_t)H * W * sizeof(T));
    const size_t np = (size_t)N * chunks;
    Arena ar(ws, wsb);
    ar.require(workspace_bytes((int)sizeof(T), N, H, W, halfwidth));
    const auto [pval, pidx, peaks] = carve(ar, N, np);
    if (!ar.ok)
        return SRX_E_WORKSPACE;
    const int reach = halfwidth + EXTRA_REACH, win = 2 * reach + 1;
    hipLaunchKernelGGL(k_psf_argmax<T>, dim3(chunks, N), dim3(BLK), 0, st, frames, (unsigned)((size_t)H * W), pval, pidx);
    SRX_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_psf_pick, dim3(N), dim3(256), 0, st, pval, pidx, chunks, H, W, reach, peaks, info);
    SRX_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_psf_window<T>, dim3(1), dim3(cdiv(win * win, 64) * 64), 0, st, frames, N, H, W, halfwidth, peaks, psf);
    SRX_CHECK_LAUNCH();
    return SRX_OK;
}

}  // namespace psf
}  // namespace srx
