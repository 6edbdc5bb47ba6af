// srx_patch.hpp -- patch-resident IBP iteration: ONE workgroup owns a whole 256 x 256 HR patch.
//
// The tile kernels of srx_mosaic.hpp pay for their independence with halos: a 64 x 64 output tile of k_fwd_mosaic filters an
// 89 x 89 region, k_bwd_mosaic a 95 x 95 one, and the planes b, G (and M as float) travel through HBM between the three
// launches of an iteration (2.9x the algorithmic bytes, BENCH_r01).  For patch workloads (BASELINE config 2: 64 x 64 LR ->
// 256 x 256 HR) the whole HR patch fits ONE compute unit: 256 x 256 floats = 64 values in each of 1024 threads.  This kernel
// runs an entire iteration of mono_cal_target/run_sr.py:190-209 on that register-resident plane:
//
//   * 16 waves form a 4 x 4 grid of 64 x 64 blocks.  "Column layout": lane = column of the block, 64 registers = its rows;
//     "row layout": lane = row, registers = columns.  Every operator of the mosaic formulation is separable (rank-1 PSF), so
//     the iteration is  V-fwd (column layout) -> transpose -> H-fwd, G = M - C Y, H-bwd (row layout) -> transpose -> V-bwd,
//     update (column layout).  The transposes are wave-private (through LDS, no workgroup barrier).
//   * The recursive spline prefilter runs in registers, 64 dependent fmas per pass and lane.  A block starts its recursion
//     from a zero state; the true incoming state is the neighbour block's end value (|z|^64 = 0), and because the recursion
//     is linear it is added afterwards as z^(i+1) * carry over the first FIX = 16 samples (|z|^17 = 2e-10).  One LDS word
//     per lane and pass crosses a block boundary instead of an R = 11 warm-up halo.
//   * SciPy's 12-sample edge pad is never materialised.  Its effect is closed form: inside a constant run the causal state
//     is the steady state 6 v / (1 - z); the coefficients in the pad follow c[i] = z (c[i+1] - S); the far (reflect) end
//     contributes z^24.  tools/patch_proto.py derives these forms and checks them against the oracle to 3e-14 (float64).
//   * The near band (LR row / column 0 replicated into the pad, srx_mosaic.hpp) is evaluated from the same per-pixel lists
//     (k_build_near) out of two small LDS strips of Y; the one G / Y row above the block grid (frames with n_k > 0) rides in
//     the grid's last row, which holds no sample when the integer shifts span less than f ("wrapped row").
//
// HBM traffic per iteration and HR pixel: read hr twice (the second read, for the update, hits L2 / MALL), read M and C,
// write hr = the algorithmic 12 B + the re-read; no intermediate plane exists.
//
// The block primitives the stages are made of -- transpose64, chain64, fwd_chain, bwd_chain, blur_block, the 7 x 7 Horner blur, st4 /
// ld4 -- live in srx_block.hpp (namespace blk), templated on the element type: every wave-block kernel family calls them there, and the
// float64 strips of srx_stile.hpp instantiate the same source in double.  This file is the patch kernel, its tables, its eligibility,
// its carve and its driver -- and the near band of stage B for every kernel that runs it (near_count, near_coords, near_put_y, near_px,
// near_get_g: k_ibp_patch here, the windows of srx_dtile.hpp, k_ibp_sh of srx_stile.hpp in double), with what those three set up once per
// call: the operand planes (k_block_prep<T>), the near-band lists (k_near_tab) and pairs (k_near_m<T, P>), queued by block_setup().
#pragma once
#include "srx_block.hpp"
#include "srx_mosaic.hpp"

namespace srx {
namespace dtile {
// The regions of a call along one axis: a frame is cut into overlapping windows, which srx_dtile.hpp plans and names; the set-up kernels
// below take the plan of either axis by value, as k_dtile_setup does.
struct AxisTiles {
    int n;
    int o[64], a[65];  // origins; ownership boundaries (global): window t owns [a[t], a[t + 1])
};
}  // namespace dtile
namespace patch {
using namespace blk;
using dtile::AxisTiles;

// What k_ibp_patch's memory operations cost, from timing ablations that computed wrong results (C2, 161 us per iteration): without
// the hr park store 150, without the hr re-read 152, without both 144, without the M loads as well 139, without the near band and the
// MSE sums too 138: the memory operations are 14 % of the iteration; requesting the parked state or the near-band descriptors a chain
// earlier changes nothing.  What did: not parking the quarter of the state whose reload had no cover (resident_rows() below; 137.6 -> 127.1 us
// on one box).
constexpr int PN = 256;        // patch edge (HR pixels)
constexpr int YW = 260;        // row pitch of the near-band strips
constexpr int OFF_YT = 16 * RW, OFF_YL = OFF_YT + 4 * YW, OFF_GT = OFF_YL + 4 * YW, OFF_GL = OFF_GT + 3 * YW,
              OFF_ROW = OFF_GL + 3 * YW, OFF_PART = OFF_ROW + PN, LDS_WORDS = OFF_PART + 32;
static_assert(LDS_WORDS * 4 <= 160 * 1024, "LDS budget");

// Filter weights of one axis.  They live in device memory and are fetched with scalar loads right where a stage needs them
// (sload8): as by-value kernel arguments the two sets would sit in ~50 scalar registers for the whole iteration loop.
struct AxisW {
    float kb[8];  // forward blur (correlation) weights [0..6], times kq = -6 z: the recursions run in the scaled form of srx_fused.hpp
    float kt[8];  // backward blur (flipped kernel) weights [0..6]
    float wfb[8]; // [0..3] forward FIR (after the prefilter); [4..7] backward FIR (before the prefilter), times kq
};
struct AxisC {
    int ex;       // n_max: G / Y samples above the block grid (0 or 1)
    int nb;       // -n_min: near-band samples inside the grid
    int E;        // padded Y index = rho + E
};

constexpr int NN_PAD = 2048;  // near-band pixels of a patch (<= 2 per thread)

struct PatchArgs {
    AxisC y, x;
    int nn, ntop;               // near-band pixels: all / those of the top rows (the enumeration of k_near_tab)
    int ngrp;                   // groups of 4 list entries per near-band pixel
    int c01;                    // the far-field count map is C[gy, gx] = ry[gy] rx[gx], a 0/1 product (full phase grids)
    unsigned long long ry[4], rx[4];
    float sn;                   // step / N
};

// per-call device tables of the patch path
struct PatchTabs {
    const float *Mt;            // [B][64 column quads][256 gy][4] far-field LR mosaic, transposed, four columns interleaved
    const unsigned *Mt8;        // [B][16][256 gy][4]: the same as bytes, 4 columns per word, four words interleaved (valid where m8[b] != 0)
    const int *m8;              // [B]: every far-field M of the patch is an integer in [0, 255]
    const float *Ct;            // [64 column quads][256 gy][4] count map, as Mt (unused when c01)
    const AxisW *aw;            // [2]: y, x
    const uint2 *nrec;          // [NN_PAD]  x = cnt | cu << 8 | dst << 16, y = strip offset of the pixel's own Y sample
    const uint2 *nent;          // [ngrp][NN_PAD] four 16-bit strip offsets per group
    const float2 *Mn;           // [B][NN_PAD] (M, Mu) of the near-band pixels
    const float *k2;            // [2][7][8]: a PSF that is not rank 1 -- weights of the forward blur (times kq^2) and of the adjoint blur in COLUMN layout:
                                // k2[t][c][r] = K[r][c], lane-direction tap c, register-direction tap r (rows padded to 8 words)
};

// ---- the near band, for every kernel that runs stage B (k_ibp_patch, k_ibp_dtile's windows, k_ibp_sh in T) ---------------------------
// The near band of a region of RY rows x RX columns (the patch: PN x PN; a window: its own shape) is ONE enumeration: the top rows
// -exy .. nby - 1 whole (columns -exx .. RX - 1), then the left columns -exx .. nbx - 1 of the rows below them.
__host__ __device__ constexpr int near_top(int RX, int exy, int exx, int nby) { return (exy + nby) * (RX + exx); }
__host__ __device__ constexpr int near_count(int RY, int RX, int exy, int exx, int nby, int nbx)
{
    return near_top(RX, exy, exx, nby) + (RY - nby) * (exx + nbx);
}
// pixel t of that enumeration -> natural coordinates and offset in the G strips
__device__ __forceinline__ void near_coords(int t, int RX, int exy, int exx, int nby, int nbx, int &ngy, int &ngx, int &dst)
{
    const int WN = RX + exx, LN = max(exx + nbx, 1), ntop = near_top(RX, exy, exx, nby);  // (no left strip: no t reaches the second branch)
    if (t < ntop) {
        const int rr = t / WN, cc = t - rr * WN;
        ngy = rr - exy, ngx = cc - exx, dst = rr * YW + cc;
    } else {
        const int q = t - ntop, rr = q / LN, cc = q - rr * LN;
        ngy = nby + rr, ngx = cc - exx, dst = 3 * YW + rr * 3 + cc;
    }
}
// offset of Y[ry, rx] in the strips: top strip rows ry <= nby, left strip otherwise (then rx <= nbx)
__device__ __forceinline__ int strip_off(int ry, int rx, int exy, int exx, int nby)
{
    return ry <= nby ? (ry + exy) * YW + rx + exx : 4 * YW + (ry + exy) * 4 + rx + exx;
}
// In the kernel, row layout: lane = strip row q = gy + exy, r[j] = column 64 u + j, yexx = Y[gy, -1].
// A lane's Y samples into the strips: its whole row (toprow: rows up to nby, the first left-band row included) and / or its first columns
// (leftcol: the blocks of the region's first column)
template <typename T> __device__ __forceinline__ void near_put_y(const T (&r)[64], T yexx, bool toprow, bool leftcol, int q, int u, int exx, int nbx, T *Yt, T *Yl)
{
    if (toprow) {
        T *dst = Yt + q * YW + 64 * u + exx;
#pragma unroll
        for (int j = 0; j < 64; j++)
            dst[j] = r[j];
        if (u == 0 && exx)
            dst[-1] = yexx;
    }
    if (leftcol) {
        T *dst = Yl + q * 4 + exx;
#pragma unroll
        for (int j = 0; j < 3; j++)
            if (j <= nbx)
                dst[j] = r[j];
        if (exx)
            dst[-1] = yexx;
    }
}
// the first c (at most four) of the Y samples a group of list entries names
template <typename T> __device__ __forceinline__ T near_sum4(const T *Ys, uint2 e, int c)
{
    return (c > 0 ? Ys[e.x & 0xffff] : (T)0) + (c > 1 ? Ys[e.x >> 16] : (T)0) + (c > 2 ? Ys[e.y & 0xffff] : (T)0) + (c > 3 ? Ys[e.y >> 16] : (T)0);
}
// one near-band pixel: G = M - the sum of the listed Y samples, into the G strips; the counted samples' share of the MSE trace onto sq.
// nr, ne: its records of k_near_tab (ne: the first group of four entries); next(g): group g >= 1 -- more than four frames on a
// pixel: the corner, or frames sharing a phase.  Ys / Gs: the strips (behind the barrier that follows near_put_y).
template <typename T, typename NEXT> __device__ __forceinline__ void near_px(uint2 nr, uint2 ne, T M, T Mu, const T *Ys, T *Gs, NEXT next, T &sq)
{
    const int cnt = nr.x & 255, cu = (nr.x >> 8) & 255, dst = nr.x >> 16;
    T ys = near_sum4(Ys, ne, cnt);
    for (int g = 1; 4 * g < cnt; g++)
        ys += near_sum4(Ys, next(g), cnt - 4 * g);
    Gs[dst] = M - ys;
    if (cu > 0) {
        const T gu = Mu - (T)cu * Ys[nr.y];
        sq += gu * gu / (T)cu;
    }
}
// G of a lane's near-band pixels back from the strips (behind the barrier that follows near_px): the first nbx columns of a row below the
// top band (row = gy - nby; a lane of the region's first column of blocks) ...
template <typename T> __device__ __forceinline__ void near_get_g_left(T (&r)[64], T &gexx, const T *Gl, int row, int exx, int nbx)
{
    const T *src = Gl + row * 3 + exx;
#pragma unroll
    for (int j = 0; j < 3; j++)
        if (j < nbx)
            r[j] = src[j];
    if (exx)
        gexx = src[-1];
}
// ... or, rownear, the whole row (k_ibp_dtile reads its rows eight columns at a time and says why)
template <typename T> __device__ __forceinline__ void near_get_g(T (&r)[64], T &gexx, bool rownear, int gy, int u, int exy, int exx, int nby, int nbx, const T *Gt, const T *Gl)
{
    if (rownear) {
        const T *src = Gt + (gy + exy) * YW + 64 * u + exx;
#pragma unroll
        for (int j = 0; j < 64; j++)
            r[j] = src[j];
        if (u == 0 && exx)
            gexx = src[-1];
    } else if (u == 0) {
        near_get_g_left(r, gexx, Gl, gy - nby, exx, nbx);
    }
}

// ---- eligibility ----------------------------------------------------------------------------------------------------
static inline bool axis_ok(const mosaic::AxisPlan &pl, int f)
{
    const int nmin = pl.nmin, nmax = pl.nmax;
    // a common fraction > 0; at most one sample above the grid; the near band within the strips; the last `ex` grid rows
    // empty (integer shifts span less than f), which also makes G vanish from row n - 1 on when ex = 1
    return !pl.zero && nmax >= 0 && nmax <= 1 && nmin <= 0 && nmax - nmin <= 3 && nmax - nmin <= f - 1 && -nmin < f;
}

// may a call of this shape EVER take the path: the shape-only workspace bound asks this, eligible() asks it first
static inline bool shape_admits(const IbpShape &s) { return s.eb == 4 && s.H == PN && s.W == PN; }

static inline bool eligible(const IbpSpec &s, bool rank1_only = false)
{
    const int f = s.f;
    if (!shape_admits(s) || f < 2)
        return false;
    mosaic::AxisPlan py, px;
    if (!mosaic::plan_axis(s.N, s.sh, 0, f, py) || !mosaic::plan_axis(s.N, s.sh, 1, f, px))
        return false;
    fused::Kernel7<float> kc;
    fused::make_kernel7<float>(s.k, s.kh, s.kw, false, kc, s.flags);
    // (round 4: a PSF that is not rank 1 runs the 7 x 7 form of the two blurs, blur2d_pass1 / blur2d_fix)
    if (!((kc.separable || !rank1_only) && axis_ok(py, f) && axis_ok(px, f)))
        return false;
    // the near band within the kernel's two-pixels-per-thread descriptor lists (iterate() computes the same count)
    const int exy = py.nmax, nby = -py.nmin, exx = px.nmax, nbx = -px.nmin;
    return near_count(PN, PN, exy, exx, nby, nbx) <= NN_PAD;
}

// ---- once per call: the operand planes and the near-band tables, for every kernel that runs stage B ------------------------------------
// The iteration kernels read one layout per table, so each table is built in one place: k_ibp_patch, the windows of k_ibp_dtile and the
// strips k_ibp_sh (in T) all call block_setup() below.
//
// Transposed far-field operands of an H x W plane (the patch and the strips: PN x PN; a frame of windows: its own shape):
//   Mt[b][gx / 4][gy][gx % 4] = M[b][gy + 13][gx + 13] (and Ct from C, plane index B): in row layout a lane is a row, and one 16-byte
//   load brings four of its float columns (64 consecutive gy x 16 bytes per wave-instruction);
//   Mt8[b][gx / 16][gy][(gx / 4) % 4]: the same values as bytes, four columns per word, four words interleaved the same way;
//   m8[b] (preset non-zero by the host) cleared when a value of item b is not an integer in [0, 255] (uint8 sensor frames with at most one
//   sample per HR pixel: one quarter of the bytes).
// Near-band pixels (gy < nby or gx < nbx) are zero here: the kernels take them from the near-band lists (several frames: sums beyond a byte).
// grid (ceil(W / 32), ceil(H / 32), B + 1), block (32, 8); W a multiple of 4.
template <typename T>
__global__ void __launch_bounds__(256)
    k_block_prep(const T *__restrict__ Mg, const T *__restrict__ Cg, int B, int H, int W, int nby, int nbx, T *__restrict__ Mt, T *__restrict__ Ct,
                 unsigned *__restrict__ Mt8, int *__restrict__ m8)
{
    __shared__ T t[32][33];
    const int Hg = H + 27, Wg = W + 27;
    const int b = blockIdx.z, x0 = blockIdx.x * 32, y0 = blockIdx.y * 32;
    const T *src = b < B ? Mg + (size_t)b * Hg * Wg : Cg;
    T *dst = b < B ? Mt + (size_t)b * H * W : Ct;
    bool ok = true;
    for (int r = threadIdx.y; r < 32; r += 8) {
        const int gy = y0 + r, gx = x0 + (int)threadIdx.x;
        T v = (gy < H && gx < W) ? src[(size_t)(gy + 13) * Wg + gx + 13] : (T)0;  // (the ragged last tiles of a frame)
        if (b < B && (gy < nby || gx < nbx))
            v = 0;
        ok = ok && v == rint(v) && v >= (T)0 && v <= (T)255;
        t[r][threadIdx.x] = v;
    }
    __syncthreads();
    const int g = threadIdx.y, row = y0 + (int)threadIdx.x, wr = x0 / 4 + g;  // 8 groups of 4 columns: column quad wr of row `row`
    if (row < H && 4 * wr < W) {
        const T *q = &t[threadIdx.x][4 * g];
        T *d = dst + ((size_t)wr * H + row) * 4;
        if constexpr (sizeof(T) == 4) {
            *reinterpret_cast<float4 *>(d) = make_float4(q[0], q[1], q[2], q[3]);
        } else {
#pragma unroll
            for (int c = 0; c < 4; c++)
                d[c] = q[c];
        }
        if (b < B)
            Mt8[(size_t)b * (W / 4) * H + ((size_t)(wr >> 2) * H + row) * 4 + (wr & 3)] =
                (unsigned)q[0] | (unsigned)q[1] << 8 | (unsigned)q[2] << 16 | (unsigned)q[3] << 24;
    }
    // one atomic per block, not one per pixel: a batch of float-valued patches used to spend 25 ms here (65 536 atomics per patch on
    // one address) -- twice the time of the 80 iterations that followed
    const bool bad = __syncthreads_or(b < B && !ok);
    if (bad && threadIdx.x == 0 && threadIdx.y == 0)
        atomicAnd(&m8[b], 0);
}

// the patch and the strips: the plan (AxisTiles, above) with one window per axis, which owns all of itself
static inline AxisTiles one_region(int L)
{
    AxisTiles at = {};
    at.n = 1, at.a[1] = L;
    return at;
}
// Near-band table `tab` of such a plan: the windows on the top image edge first, then those below the first on the left edge
// (ty.n + tx.n - 1 tables).  A window sees the image's axis parameters where it lies on that image edge, none elsewhere.
struct NearWin {
    int oy, ox;              // window origin (image coordinates)
    int y0, y1, x0, x1;      // owned range, window-local
    int exy, exx, nby, nbx;
};
__device__ __forceinline__ NearWin near_window(const AxisTiles &ty, const AxisTiles &tx, int tab, const AxisC &ay, const AxisC &ax)
{
    const int y = tab < tx.n ? 0 : tab - tx.n + 1, x = tab < tx.n ? tab : 0;
    NearWin w;
    w.oy = ty.o[y], w.ox = tx.o[x];
    w.y0 = ty.a[y] - w.oy, w.y1 = ty.a[y + 1] - w.oy, w.x0 = tx.a[x] - w.ox, w.x1 = tx.a[x + 1] - w.ox;
    w.exy = y == 0 ? ay.ex : 0, w.nby = y == 0 ? ay.nb : 0;
    w.exx = x == 0 ? ax.ex : 0, w.nbx = x == 0 ? ax.nb : 0;
    return w;
}

// the per-pixel lists of k_build_near, re-expressed for the kernels: strip offsets instead of padded coordinates, grouped so that the
// threads of a wave read consecutive words; the counted-sample count zeroed for pixels whose (clamped) position another window owns.
// nrec[tab][NN_PAD], nent[group][tab][NN_PAD]; nn_out[tab] (if asked for): the table's pixels.  RY x RX: the windows' shape; W: the image's
// width.  One thread per near-band pixel, grid (blocks of 256 pixels, tables)
__global__ void __launch_bounds__(256)
    k_near_tab(const int *__restrict__ ncu, const int *__restrict__ nyx, int NS, int PBy, int PBx, AxisTiles ty, AxisTiles tx, int RY, int RX, int W, AxisC ay,
               AxisC ax, int *__restrict__ nn_out, uint2 *__restrict__ nrec, uint2 *__restrict__ nent)
{
    const int t = blockIdx.x * 256 + threadIdx.x, tab = blockIdx.y, ntabs = gridDim.y;
    const NearWin w = near_window(ty, tx, tab, ay, ax);
    const int nn = near_count(RY, RX, w.exy, w.exx, w.nby, w.nbx);
    if (nn_out && t == 0)
        nn_out[tab] = nn;
    if (t >= nn)
        return;
    int ngy, ngx, dst;
    near_coords(t, RX, w.exy, w.exx, w.nby, w.nbx, ngy, ngx, dst);
    const int gy = w.oy + ngy, gx = w.ox + ngx;  // image (natural) coordinates
    const int ni = mosaic::near_index(gy + 13, gx + 13, W + 27, PBy, PBx), pk = ncu[ni], cnt = pk & 255;
    int cu = pk >> 8;
    const int cy = max(ngy, 0), cx = max(ngx, 0);  // where its counted samples sit: the window that owns that pixel counts them
    if (cy < w.y0 || cy >= w.y1 || cx < w.x0 || cx >= w.x1)
        cu = 0;
    const int own = strip_off(ngy, ngx, w.exy, w.exx, w.nby);
    nrec[(size_t)tab * NN_PAD + t] = make_uint2((unsigned)cnt | (unsigned)cu << 8 | (unsigned)dst << 16, (unsigned)own);
    for (int g = 0; g < NS / 4; g++) {
        unsigned o[4];
        for (int e = 0; e < 4; e++) {
            const int c = nyx[(size_t)ni * NS + 4 * g + e];  // slots past cnt hold an in-range coordinate (k_build_near)
            o[e] = 4 * g + e < cnt ? (unsigned)strip_off((c & 0xffff) - ay.E - w.oy, (c >> 16) - ax.E - w.ox, w.exy, w.exx, w.nby) : (unsigned)own;
        }
        nent[((size_t)g * ntabs + tab) * NN_PAD + t] = make_uint2(o[0] | o[1] << 16, o[2] | o[3] << 16);
    }
}

// (M, Mu) of the near-band pixels of every item: Mn[b][tab][NN_PAD].  P: the pair of T the iteration kernel reads Mn as (float2;
// stile::T2<T>).  grid (blocks of 256 pixels, tables, B)
template <typename T, typename P>
__global__ void __launch_bounds__(256)
    k_near_m(const T *__restrict__ Mg, const T *__restrict__ Mu, int NB, int PBy, int PBx, AxisTiles ty, AxisTiles tx, int RY, int RX, int H, int W, AxisC ay,
             AxisC ax, P *__restrict__ Mn)
{
    static_assert(sizeof(P) == 2 * sizeof(T), "a pair of samples");
    const int t = blockIdx.x * 256 + threadIdx.x, tab = blockIdx.y, ntabs = gridDim.y, b = blockIdx.z;
    const NearWin w = near_window(ty, tx, tab, ay, ax);
    if (t >= near_count(RY, RX, w.exy, w.exx, w.nby, w.nbx))
        return;
    int ngy, ngx, dst;
    near_coords(t, RX, w.exy, w.exx, w.nby, w.nbx, ngy, ngx, dst);
    const int gy = w.oy + ngy, gx = w.ox + ngx, Wg = W + 27, Hg = H + 27;
    const int ni = mosaic::near_index(gy + 13, gx + 13, Wg, PBy, PBx);
    P v;
    v.x = Mg[((size_t)b * Hg + gy + 13) * Wg + gx + 13], v.y = Mu[(size_t)b * NB + ni];
    Mn[((size_t)b * ntabs + tab) * NN_PAD + t] = v;
}

// The host side.  c: srx_mosaic.hpp's common_prep()'s tables (M, C, Mu, the near lists); ty, tx, RY, RX: the plan and the windows' shape;
// ay, ax: the image's axis parameters (fill_axis); blocks: blocks of 256 near-band pixels a table is launched with, 0 when the call has no
// near band.  near_tab() alone serves a call that builds the rest of its tables itself (patch::iterate on a full phase grid).
template <typename T>
static int near_tab(const mosaic::Common<T> &c, const AxisTiles &ty, const AxisTiles &tx, int RY, int RX, const AxisC &ay, const AxisC &ax, int blocks,
                    int *nn_out, uint2 *nrec, uint2 *nent, hipStream_t st)
{
    hipLaunchKernelGGL(k_near_tab, dim3(blocks, ty.n + tx.n - 1), dim3(256), 0, st, c.ncu, c.nyx, c.NS, c.py.PB, c.px.PB, ty, tx, RY, RX, c.W, ay, ax, nn_out, nrec,
                       nent);
    SRX_CHECK_LAUNCH();
    return SRX_OK;
}
// the m8 preset, the operand planes, the near-band descriptor lists and the near-band (M, Mu) pairs of a call
template <typename T, typename P>
static int block_setup(const mosaic::Common<T> &c, const AxisTiles &ty, const AxisTiles &tx, int RY, int RX, const AxisC &ay, const AxisC &ax, int blocks, T *Mt,
                       T *Ct, unsigned *Mt8, int *m8, int *nn_out, uint2 *nrec, uint2 *nent, P *Mn, hipStream_t st)
{
    if (fill_bytes(m8, 0xff, (size_t)c.B * sizeof(int), st) != hipSuccess)
        return SRX_E_HIP;
    hipLaunchKernelGGL(k_block_prep<T>, dim3(cdiv(c.W, 32), cdiv(c.H, 32), c.B + 1), dim3(32, 8), 0, st, c.Mg, c.Cg, c.B, c.H, c.W, ay.nb, ax.nb, Mt, Ct, Mt8, m8);
    SRX_CHECK_LAUNCH();
    if (blocks > 0) {
        SRX_TRY(near_tab(c, ty, tx, RY, RX, ay, ax, blocks, nn_out, nrec, nent, st));
        hipLaunchKernelGGL((k_near_m<T, P>), dim3(blocks, ty.n + tx.n - 1, c.B), dim3(256), 0, st, c.Mg, c.Mu, c.NB, c.py.PB, c.px.PB, ty, tx, RY, RX, c.H, c.W, ay,
                           ax, Mn);
        SRX_CHECK_LAUNCH();
    }
    return SRX_OK;
}

// ---- the same tables straight from the LR frames, for full phase grids (c01: every far-field HR pixel holds at most one sample) ------
// k_mosaic_build + k_block_prep write and re-read an M plane of the whole batch (1024 patches: 328 MB out, 328 MB in, on top of the 268 MB
// of LR frames, with a gather that fetches 64 useful bytes per load instruction): 0.57 ms of a 12.6 ms C2 step.  On a full phase grid
// row gy of M is the INTERLEAVE of one LR row of the f frames of its row class -- M[gy][gx] = lr[K[cy(gy)][cx(gx)]][iy(gy)][jx(gx)],
// depth-to-space -- so the operand planes follow from the LR frames in one pass: a lane takes a column QUAD (for x4 the four frames of
// the row class at one LR column: four coalesced 256-byte reads per wave and row), a 16-row band goes through LDS so that the
// transposed planes leave in 256-byte runs.  The byte plane is written first and the float plane only for the patches that turn out to need it
// (k_patch_build<0> / <1>: a sample that is not an integer in [0, 255]): 64 KB instead of 320 KB per patch of 8-bit frames.
struct AxisMap {       // per natural coordinate g of a patch: the class of the frames that land there and the LR index they bring
    signed char cls[PN];   // -1: no frame (C = 0)
    unsigned char idx[PN];
};
struct BuildMaps {
    AxisMap y, x;
    signed char frame[4][4];  // frame of (row class, column class)
    int nby, nbx;
};
// grid (PN / 16 bands, B), block 256: wave w takes rows w, w + 4, ... of the band, lane = column quad.
// PASS 0 writes the BYTE plane of every patch and clears m8[b] (preset non-zero) when a sample it placed is not an integer in [0, 255];
// PASS 1 writes the float plane of the patches so marked and returns at once for the others.  (Round 4's first form decided with a pass of
// its own over the frames, k_patch_flags -- 63 us of a C2 step for a question this kernel answers on the way; frames of 8-bit integers,
// the reference's data, now pay one empty launch instead, frames that are not pay the byte pass: +0.08 ms per 1024 patches.)
// S = uint8_t (the camera's frames, srx_ibp_u8lr_f32): the samples ARE bytes, so PASS 0 has nothing to test, never clears m8, and PASS 1
// is not launched at all.  Two read shapes:
//   WIDE (the default; frames on a 4-byte boundary -- a block-uniform test of `lr`: h w and w are multiples of 4): a wave fetches the LR rows
//     behind one patch row WHOLE, as PN / 4 = 64 words (lane = frame of the row class x word of its row: one 4-byte load per lane and
//     patch row, four per lane instead of sixteen), parks them in the LDS and every lane picks its four bytes there;
//   one byte per lane (frames at other addresses, or SRX_FLAG_DIAG_U8_BYTE_LOADS): the float form's sixteen loads per lane, a wave's
//     request 64 consecutive bytes of one LR row.
// 1024 patches: 75 us wide, 101 us by bytes -- the kernel is bound by the loads it issues, not by their bytes -- against 79 + 7 us for the
// two passes over float frames (tools/u8lr_time.py).
template <int PASS, typename S = float, bool WIDE = false>
__global__ void __launch_bounds__(256)
    k_patch_build(const S *__restrict__ lr, int N, int h, int w, const BuildMaps *__restrict__ maps, int *__restrict__ m8,
                  float *__restrict__ Mt, unsigned *__restrict__ Mt8)
{
    __shared__ float4 tile[64][17];  // [column quad][row of the band] (+1: the write-out walks a quad's rows)
    const int b = blockIdx.y, gy0 = blockIdx.x * 16, cq = threadIdx.x & 63, wv = threadIdx.x >> 6;
    constexpr bool bytes = PASS == 0, test = PASS == 0 && std::is_same<S, float>::value;
    static_assert(PASS == 0 || std::is_same<S, float>::value, "byte frames need no float plane");
    if (PASS == 1 && __builtin_amdgcn_readfirstlane(m8[b]) != 0)
        return;
    int bad = 0;
    const S *src = lr + (size_t)b * N * h * w;
    int cx[4], jx[4];
#pragma unroll
    for (int c = 0; c < 4; c++) {
        const int gx = 4 * cq + c;
        cx[c] = gx < maps->nbx ? -1 : maps->x.cls[gx];  // near-band columns: the kernel takes them from the near-band lists
        jx[c] = maps->x.idx[gx];
    }
    // the frame of (row class, column class): 16 bytes, four scalar words (per lane and sample this was a dependent byte load from memory)
    const int *fw = reinterpret_cast<const int *>(&maps->frame[0][0]);
    const int fr0 = fw[0], fr1 = fw[1], fr2 = fw[2], fr3 = fw[3];
    float v[4][4];
    bool done = false;
    if constexpr (WIDE) {
        __shared__ unsigned rowsw[4][4][64];  // [wave][patch row of the wave][frame of the row class x word]
        if ((((size_t)lr) & 3) == 0) {  // (block-uniform: the barrier below is met by all or none)
            const int nd = w >> 2, kx = cq / nd, dw = cq - kx * nd;  // words per LR row; this lane's column class and word
            unsigned wd[4];
#pragma unroll
            for (int m = 0; m < 4; m++) {
                const int gy = gy0 + wv + 4 * m;
                const int cy = gy < maps->nby ? -1 : (int)maps->y.cls[gy], iy = maps->y.idx[gy];  // wave-uniform
                const int fsel = cy == 0 ? fr0 : cy == 1 ? fr1 : cy == 2 ? fr2 : fr3;
                wd[m] = 0;
                if (cy >= 0)
                    wd[m] = reinterpret_cast<const unsigned *>(src + ((size_t)((fsel >> (8 * kx)) & 0xff) * h + iy) * w)[dw];
            }
#pragma unroll
            for (int m = 0; m < 4; m++)
                rowsw[wv][m][cq] = wd[m];
            __syncthreads();
            const unsigned char *rb = reinterpret_cast<const unsigned char *>(&rowsw[wv][0][0]);
#pragma unroll
            for (int m = 0; m < 4; m++) {
                const int gy = gy0 + wv + 4 * m;
                const int cy = gy < maps->nby ? -1 : (int)maps->y.cls[gy];
#pragma unroll
                for (int c = 0; c < 4; c++) {
                    v[m][c] = 0.f;
                    if (cy >= 0 && cx[c] >= 0)
                        v[m][c] = (float)rb[m * 256 + cx[c] * w + jx[c]];
                }
            }
            done = true;
        }
    }
    if (!done)
#pragma unroll
    for (int m = 0; m < 4; m++) {  // all sixteen loads of a lane leave before the first one is looked at
        const int gy = gy0 + wv + 4 * m;
        const int cy = gy < maps->nby ? -1 : (int)maps->y.cls[gy], iy = maps->y.idx[gy];  // wave-uniform
        const int fsel = cy == 0 ? fr0 : cy == 1 ? fr1 : cy == 2 ? fr2 : fr3;
#pragma unroll
        for (int c = 0; c < 4; c++) {
            v[m][c] = 0.f;
            if (cy >= 0 && cx[c] >= 0)
                v[m][c] = src[((size_t)((fsel >> (8 * cx[c])) & 0xff) * h + iy) * w + jx[c]];
        }
    }
#pragma unroll
    for (int m = 0; m < 4; m++) {
        if (test) {
#pragma unroll
            for (int c = 0; c < 4; c++)  // (the zeros of absent samples pass)
                bad |= !((int)(v[m][c] == rintf(v[m][c])) & (int)(v[m][c] >= 0.f) & (int)(v[m][c] <= 255.f));
        }
        tile[cq][wv + 4 * m] = make_float4(v[m][0], v[m][1], v[m][2], v[m][3]);
    }
    if (test) {
        if (__syncthreads_or(bad) && threadIdx.x == 0)
            atomicAnd(&m8[b], 0);
    } else {
        __syncthreads();
    }
    if (bytes) {
        // Mt8[b][cq >> 2][gy][cq & 3]: one word per (quad, row); consecutive threads = the four quads of a group, then the rows
#pragma unroll
        for (int n = 0; n < 4; n++) {
            const int u = threadIdx.x + 256 * n, sub = u & 3, r = (u >> 2) & 15, grp = u >> 6, q = 4 * grp + sub;
            const float4 t = tile[q][r];
            const unsigned wd = (unsigned)t.x | (unsigned)t.y << 8 | (unsigned)t.z << 16 | (unsigned)t.w << 24;
            Mt8[(size_t)b * (PN / 4) * PN + ((size_t)grp * PN + gy0 + r) * 4 + sub] = wd;
        }
    } else {
        // Mt[b][cq][gy][4]: 16 bytes per (quad, row); consecutive threads = the rows of a quad
#pragma unroll
        for (int n = 0; n < 4; n++) {
            const int u = threadIdx.x + 256 * n, r = u & 15, q = u >> 4;
            reinterpret_cast<float4 *>(Mt)[((size_t)b * (PN / 4) + q) * PN + gy0 + r] = tile[q][r];
        }
    }
}
// (M, Mu) of the near-band pixels of every patch from the LR frames (k_mosaic_build's sums, on the near band only), and the patch's
// share of the within-pixel scatter V (zero on a full phase grid; kept for the definition's sake).  grid (ceil(nn / 256), B)
template <typename S = float>
__global__ void __launch_bounds__(256)
    k_patch_near_build(const S *__restrict__ lr, int N, int h, int w, const mosaic::MTap *__restrict__ tabY, const mosaic::MTap *__restrict__ tabX,
                       int Hg, int Wg, int Dy, int Dx, int exy, int exx, int nby, int nbx, int nn, float2 *__restrict__ Mn, double *__restrict__ Vtot)
{
    const int t = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    double var = 0.0;
    if (t < nn) {
        int ngy, ngx, dst;
        near_coords(t, PN, exy, exx, nby, nbx, ngy, ngx, dst);
        const int p = ngy + 13, q = ngx + 13;
        const S *src = lr + (size_t)b * N * h * w;
        double M = 0.0, S1 = 0.0, S2 = 0.0;
        int cu = 0;
        for (int k = 0; k < N; k++) {
            const mosaic::MTap ty = tabY[(size_t)k * Hg + p], tx = tabX[(size_t)k * Wg + q];
            if (ty.i < 0 || tx.i < 0)
                continue;
            const double lv = (double)src[((size_t)k * h + ty.i) * w + tx.i];
            M += lv;
            if (ty.rho == p - Dy && tx.rho == q - Dx)
                S1 += lv, S2 += lv * lv, cu++;
        }
        Mn[(size_t)b * NN_PAD + t] = make_float2((float)M, (float)S1);
        if (cu > 1)
            var = S2 - S1 * S1 / (double)cu;
    }
    __shared__ double part[4];
    const double ws = wave_sum(var);
    if ((threadIdx.x & 63) == 0)
        part[threadIdx.x >> 6] = ws;
    __syncthreads();
    if (threadIdx.x == 0) {
        const double sacc = part[0] + part[1] + part[2] + part[3];
        if (sacc != 0.0)
            atomicAdd(&Vtot[b], sacc);
    }
}


// =========================================================================================================================
// All n_iter IBP iterations of one patch.  grid B, block 1024 (16 waves = 4 x 4 blocks of 64 x 64).
// Between iterations the HR state stays in registers (column layout); per iteration the kernel stores it (hr_out doubles as
// the parking place of the pre-update state, re-read for the update -- at its peak, the last blur of stage C, the register file
// holds the working plane and two landing batches and nothing else; through the other stages it also holds the first
// resident_rows() rows of the pre-update state, which are then not parked), reads the LR mosaic (bytes when the patch's
// samples are uint8) and the near-band descriptors.
// =========================================================================================================================
struct AxisWPair {  // PatchTabs::aw as the host fills it
    AxisW y, x;
};

// Rows of every wave's block whose pre-update state stays in registers through the iteration instead of being parked (0 or 16: quarter 0
// of stage C's blur).  16 where the instantiation takes them without a spilled register: the pair of kernels the
// flagship's grid launches (rank-1 PSF; the byte mosaic under all-ones masks, the float mosaic of a full phase grid).  The byte-mosaic form with
// a mask test and the count-plane forms gain 2 - 11 spilled registers with 16 rows, every rank-1 form 19 - 30 with 32, and the 7 x 7 forms spill as they are: they park everything, and are
// the code they were.
constexpr int resident_rows(bool c01, bool m8, int form) { return c01 && (m8 ? form == 1 : form == 0) ? 16 : 0; }

// With resident rows the file has no register left for a value that merely waits: the thread index and the lane index of wave_sum's
// shuffles, which the compiler carries through the whole iteration loop (and then spills, one scratch read per stage), are formed
// where they are used instead -- the lane index by v_mbcnt, two instructions the compiler may not hoist.
__device__ __forceinline__ int lane_here()
{
    int l;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
    return l;
}
// wave_sum of srx_common.h -- the same tree in the same order, bit for bit -- on the caller's lane index
__device__ __forceinline__ double wave_sum_at(double v, int lane)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int idx = (lane + o >= 64 ? lane : lane + o) << 2;
        const int lo = __builtin_amdgcn_ds_bpermute(idx, __double2loint(v)), hi = __builtin_amdgcn_ds_bpermute(idx, __double2hiint(v));
        v += __hiloint2double(hi, lo);
    }
    return v;
}

// FORM: 0 rank 1 (7 + 7 taps per blur), 3 full 7 x 7, 2 a 7 x 7 whose outer ring is zero; 1 (with C01 and M8) rank 1 on a grid whose count
// masks the host found all ones wherever the G step's result is used (gstep_form): the byte-mosaic G loop runs without the mask test.  A
// template value like M8, for M8's reason: the allocator sees one G loop.
template <bool C01, bool M8, int FORM = 0>
__global__ void __launch_bounds__(1024)
    k_ibp_patch(const float *__restrict__ hr_in, float *__restrict__ hr_out, PatchTabs tb, PatchArgs pa, const double *__restrict__ Vtot,
                double scale, double *__restrict__ errors, int n_iter)
{
    constexpr bool ALL1 = FORM == 1;
    constexpr int PSF = ALL1 ? 0 : FORM;
    static_assert(!ALL1 || (C01 && M8), "the all-ones G step is the byte mosaic's on a full phase grid");
    __shared__ __attribute__((aligned(16))) float lds[LDS_WORDS];
    const int tid0 = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid0 >> 6), s = wave >> 2, u = wave & 3;
    const int b = blockIdx.x;
    float *Rown = lds + wave * RW;
    const float *Rup = lds + (wave - 4) * RW, *Rdn = lds + (wave + 4) * RW;  // vertical neighbours (same u)
    const float *Rlf = lds + (wave - 1) * RW, *Rrt = lds + (wave + 1) * RW;  // horizontal neighbours (same s)
    float *Ystrip = lds + OFF_YT, *Gstrip = lds + OFF_GT, *rowbuf = lds + OFF_ROW;
    float *Yt = lds + OFF_YT, *Yl = lds + OFF_YL, *Gt = lds + OFF_GT, *Gl = lds + OFF_GL;
    double *part = reinterpret_cast<double *>(lds + OFF_PART);
    const int exy = pa.y.ex, exx = pa.x.ex, nby = pa.y.nb, nbx = pa.x.nb;

    const __amdgpu_buffer_rsrc_t rs_in = fused::plane_rsrc(hr_in + (size_t)b * PN * PN, (size_t)PN * PN);
    const __amdgpu_buffer_rsrc_t rs_out = fused::plane_rsrc(hr_out + (size_t)b * PN * PN, (size_t)PN * PN);
    // The byte form of the mosaic (M8) and the float form are two instantiations, launched one after the other; a block whose patch
    // belongs to the other one leaves at once.  (As a run-time branch inside one kernel the two G steps cost 40 more spilled
    // registers per iteration: the allocator sees the pressure of both.)
    if ((__builtin_amdgcn_readfirstlane(tb.m8[b]) != 0) != M8)
        return;
    constexpr int m8 = M8 ? 1 : 0;
    const float *awy = tb.aw[0].kb, *awx = tb.aw[1].kb;  // 24 floats each: kb | kt | wfb
    const int nn = pa.nn;
    const float sn = pa.sn;
    const int cb0 = (64 * s * PN + 64 * u) * 4;  // byte offset of this wave's block in column layout (row pitch PN)
    const int tb0 = (16 * u * PN + 64 * s) * 16;  // ... in the transposed planes (Mt, Ct: [column quad][row][4]): lane = row
    // 0/1 count map of a full phase grid: this wave's 64 row bits (row layout: bit = lane) and 64 column bits
    const unsigned long long rmask = C01 ? pa.ry[s] : 0ull, cmask = C01 ? pa.rx[u] : 0ull;

    // The state (this wave's 64 x 64 block of hr, column layout) stays in registers from one iteration's update to the next
    // iteration's blur.  Beside the working plane the file holds KRES of its 64 rows through the stages in between (xs, below: rows
    // 0 .. KRES - 1, the quarter of stage C's blur whose reload had no cover); every iteration parks the other rows in hr_out, where
    // the update re-reads them 16 rows at a time.
    constexpr int KRES = resident_rows(C01, M8, FORM);
    constexpr int PB0 = KRES / 16;  // the first parked batch of 16 rows
    static_assert(KRES == 0 || KRES == 16, "the reload schedule of stage C");
    float a[64];
    {
        const int l4 = (tid0 & 63) * 4;
#pragma unroll
        for (int i = 0; i < 64; i++)
            a[i] = fused::buf_load<float>(rs_in, l4 + (i & 3) * PN * 4, cb0 + (i >> 2) * PN * 16);
    }
    // The parked state has its own layout inside hr_out (wave, row quad, lane: 16 bytes per lane and instruction).  When the call is
    // in place (hr_in == hr_out) no wave may park before every wave has its initial state in registers.
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    const int park0 = wave * 16384;  // byte offset of this wave's 64 x 64 block in the parking layout
    for (int it = 0; it < n_iter; it++) {
        float r[64];
        float xs[KRES > 0 ? KRES : 1];  // the pre-update state of rows 0 .. KRES - 1, from stage A to the first quarter(s) of stage C's blur
        // Everything derived from the lane index (LDS and global addresses, predicates) and from the block offsets is re-derived
        // PER STAGE from opaque copies.  Left to itself the compiler computes all of it once -- at the top of the loop, or above it
        // -- and carries ~55 registers of addresses across stages whose working plane needs the file: they were spilled, one
        // scratch round trip per use (the spill traffic was as large as the kernel's real traffic).
#define SRX_STAGE_LOCALS()                                 \
    int tid = KRES > 0 ? wave * 64 + lane_here() : tid0;   \
    asm volatile("" : "+v"(tid));                          \
    const int lane = tid & 63, l4 = lane * 4;              \
    int cbl = cb0, tbl = tb0, m8l = (4 * u * PN + 64 * s) * 16; \
    asm volatile("" : "+s"(cbl), "+s"(tbl), "+s"(m8l));    \
    (void)tbl, (void)m8l, (void)cbl, (void)l4
        float yex = 0.f;
        {  // ---------------- stage A ----------------
        SRX_STAGE_LOCALS();
        __builtin_amdgcn_sched_barrier(0);
        SRX_PSTAMP(0);
        // ================= stage A: column layout, lane = column 64 u + lane, a[i] = row 64 s + i =================
        {
            int pk = park0;
            asm volatile("" : "+s"(pk));
#pragma unroll
            for (int i = 0; i < KRES; i++)
                xs[i] = a[i];
#pragma unroll
            for (int q = KRES / 4; q < 16; q++)  // (the resident rows' slots of the parking layout are never written or read)
                st4(rs_out, l4 * 4, pk + q * 1024, a[4 * q], a[4 * q + 1], a[4 * q + 2], a[4 * q + 3]);
        }
        if (PSF == 0) {
            blur_block(a, s == 0, s == 3, Rown, Rup, Rdn, SLOT0, lane, sload8(awy));
        } else {  // both directions of the PSF here (its weights carry kq^2: the H chain of stage B expects a scaled input too)
            halo3_put(a, Rown, SLOT0, lane);
            __syncthreads();
            const Halo3<float> h = halo3_get(s == 0, s == 3, Rup, Rdn, SLOT0, lane);
            blur2d_cols<PSF == 2 ? 2 : 3>(a, h.lo, h.hi, u == 0, u == 3, Rown, Rlf, Rrt, lane, tb.k2, [](int) {}, [](int, float v) { return v; });
        }
        __builtin_amdgcn_sched_barrier(0);
        SRX_PSTAMP(1);
        fwd_chain(a, s == 0, s == 3, Rown, Rup, Rdn, SLOT1, SLOT0, lane, sload8(awy + 16), yex);
        __builtin_amdgcn_sched_barrier(0);
        SRX_PSTAMP(2);
        if (exy && s == 0)  // the Y row above the grid rides in the grid's last row (empty: axis_ok)
            rowbuf[64 * u + lane] = yex;
        __syncthreads();  // also: every wave is done with the exchange slots before the transposes overwrite them
        if (exy && s == 3)
            a[63] = rowbuf[64 * u + lane];
        __builtin_amdgcn_sched_barrier(0);
        SRX_PSTAMP(3);
        transpose64(a, r, Rown, lane);
        __builtin_amdgcn_sched_barrier(0);
        SRX_PSTAMP(4);
        }
        float sq = 0.f;
        {  // ---------------- stage B ----------------
        SRX_STAGE_LOCALS();
        const bool wrapped = exy && s == 3 && lane == 63;  // row layout: this lane holds row -1
        const int gy = wrapped ? -1 : 64 * s + lane;       // row layout: natural row of this lane
        const bool rownear = wrapped || gy < nby;
        const float crow = C01 ? (float)((rmask >> lane) & 1ull) : 0.f;
        // ================= stage B: row layout, lane = row 64 s + lane, r[j] = column 64 u + j =================
        if (PSF == 0)
            blur_block(r, u == 0, u == 3, Rown, Rlf, Rrt, SLOT0, lane, sload8(awx));
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_sched_barrier(0);
        SRX_PSTAMP(5);
        float yexx = 0.f;  // Y[gy, -1] (u == 0)
        fwd_chain(r, u == 0, u == 3, Rown, Rlf, Rrt, SLOT1, SLOT0, lane, sload8(awx + 16), yexx);
        __builtin_amdgcn_sched_barrier(0);
        SRX_PSTAMP(6);
        // ---- near-band descriptors: consumed behind the strips' barrier (the strip stores and the barrier cover their latency)
        uint2 nr0 = make_uint2(0, 0), nr1 = make_uint2(0, 0), ne0 = make_uint2(0, 0), ne1 = make_uint2(0, 0);
        float2 nm0 = make_float2(0.f, 0.f), nm1 = make_float2(0.f, 0.f);
        const bool n0 = tid < nn, n1 = tid + 1024 < nn;
        // (through buffer descriptors: one 32-bit lane offset instead of three 64-bit lane addresses, which did not survive the
        // stage in registers; a lane past the list reads zeros)
        const __amdgpu_buffer_rsrc_t rsNr = fused::plane_rsrc(tb.nrec, (size_t)nn), rsNe = fused::plane_rsrc(tb.nent, (size_t)pa.ngrp * NN_PAD),
                                     rsMn = fused::plane_rsrc(tb.Mn + (size_t)b * NN_PAD, (size_t)nn);
        {
            const int t8 = tid * 8;
            nr0 = ld_u2(rsNr, t8), ne0 = ld_u2(rsNe, t8);
            nr1 = ld_u2(rsNr, t8 + 8192), ne1 = ld_u2(rsNe, t8 + 8192);
            const uint2 m0 = ld_u2(rsMn, t8), m1 = ld_u2(rsMn, t8 + 8192);
            nm0 = make_float2(__uint_as_float(m0.x), __uint_as_float(m0.y)), nm1 = make_float2(__uint_as_float(m1.x), __uint_as_float(m1.y));
        }
        // ---- near-band strips of Y
        near_put_y(r, yexx, wrapped || (s == 0 && lane <= nby), u == 0, gy + exy, u, exx, nbx, Yt, Yl);
        __syncthreads();
        // the LR mosaic of the G step: in flight during the near-band phase -- with resident rows (the phase then holds the plane, the
        // descriptors and xs) requested behind the near-band pixels instead, in flight across the phase's closing barrier
        const __amdgpu_buffer_rsrc_t rsM8 = fused::plane_rsrc(tb.Mt8 + (size_t)b * (PN / 4) * PN, (size_t)(PN / 4) * PN);
        unsigned m8w[16];
        if (m8 && KRES == 0) {
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rsM8, l4 * 4, m8l + q * PN * 16, 0);
                m8w[4 * q] = v.x, m8w[4 * q + 1] = v.y, m8w[4 * q + 2] = v.z, m8w[4 * q + 3] = v.w;
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        SRX_PSTAMP(7);
        // ---- near band: G = M - sum of the listed Y samples; the counted samples' share of the MSE trace
        {
            // (through one local lambda: with near_px called at both places directly the tail loop of either sat behind a branch and a wait of
            // its own, and C2 lost 0.5 % -- 126.3 .. 127.4 -> 126.5 .. 128.1 us per iteration, six interleaved runs each)
            auto px = [&](uint2 nr, uint2 ne, float2 nm, int t) {
                near_px(nr, ne, nm.x, nm.y, Ystrip, Gstrip, [&](int g) { return ld_u2(rsNe, (g * NN_PAD + t) * 8); }, sq);
            };
            if (n0)
                px(nr0, ne0, nm0, tid);
            if (n1)
                px(nr1, ne1, nm1, tid + 1024);
        }
        if (m8 && KRES > 0) {
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rsM8, l4 * 4, m8l + q * PN * 16, 0);
                m8w[4 * q] = v.x, m8w[4 * q + 1] = v.y, m8w[4 * q + 2] = v.z, m8w[4 * q + 3] = v.w;
            }
        }
        __syncthreads();
        __builtin_amdgcn_sched_barrier(0);
        SRX_PSTAMP(8);
        // ---- G = M - C Y on the grid; near-band pixels take their value from the strips
        float gexx = 0.f;  // G[gy, -1]
        {
            const __amdgpu_buffer_rsrc_t rsM = fused::plane_rsrc(tb.Mt + (size_t)b * PN * PN, (size_t)PN * PN);
            const __amdgpu_buffer_rsrc_t rsC = fused::plane_rsrc(tb.Ct, (size_t)PN * PN);
            float sqf = 0.f;
            // the per-column predicates below are wave-uniform and loop-invariant: from an opaque copy of the mask, or all 64 of
            // them are hoisted out of the iteration loop as 64-bit lane masks (256 scalar registers, spilled)
            unsigned long long cm = cmask;
            asm volatile("" : "+s"(cm));
            float gn[3] = {0.f, 0.f, 0.f};  // squares of the first three columns: near band when u == 0 (subtracted again below)
            if (m8) {
                float cq[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int j = 0; j < 64; j++) {
                    const float mv = (float)((m8w[j >> 2] >> (8 * (j & 3))) & 255u);
                    float g, w;
                    if (C01 && ALL1 && j < 63) {
                        // both masks are ones here (the flagship's 4 x 4 phases: every far-field pixel holds exactly one sample): what
                        // fmaf(-1.f, r[j], mv) rounds to, without the scalar bit test and the select -- one of about five vector
                        // instructions per element.  Same box, six interleaved runs each: 129.7 - 130.6 -> 127.9 - 128.6 us per iteration
                        // (DESIGN.md section 6).
                        g = mv - r[j];
                        w = 1.f;
                    } else if (C01) {  // (ALL1: the block's last column, which is the grid's empty last column when exx = 1)
                        const bool on = (cm >> j) & 1ull;  // wave-uniform; M = 0 where no frame contributes
                        g = on ? fmaf(-crow, r[j], mv) : 0.f;
                        w = 1.f;
                    } else {
                        if ((j & 3) == 0)
                            ld4(rsC, l4 * 4, tbl + (j >> 2) * PN * 16, cq[0], cq[1], cq[2], cq[3]);
                        const float cv = cq[j & 3];
                        g = fmaf(-cv, r[j], mv);
                        w = mosaic::rcp_count(cv);
                    }
                    const float g2 = g * g * w;
                    sqf += g2;
                    if (j < 3)
                        gn[j] = g2;
                    r[j] = g;
                }
            } else {
#pragma unroll
                for (int j0 = 0; j0 < 64; j0 += 16) {
                    float mv[16], cv[16];
#pragma unroll
                    for (int q = 0; q < 4; q++) {
                        ld4(rsM, l4 * 4, tbl + ((j0 >> 2) + q) * PN * 16, mv[4 * q], mv[4 * q + 1], mv[4 * q + 2], mv[4 * q + 3]);
                        if (C01) {
#pragma unroll
                            for (int c = 0; c < 4; c++)
                                cv[4 * q + c] = ((cm >> (j0 + 4 * q + c)) & 1ull) ? crow : 0.f;
                        } else {
                            ld4(rsC, l4 * 4, tbl + ((j0 >> 2) + q) * PN * 16, cv[4 * q], cv[4 * q + 1], cv[4 * q + 2], cv[4 * q + 3]);
                        }
                    }
#pragma unroll
                    for (int j = 0; j < 16; j++) {
                        const float g = fmaf(-cv[j], r[j0 + j], mv[j]);
                        const float g2 = g * g * (C01 ? 1.f : mosaic::rcp_count(cv[j]));
                        sqf += g2;
                        if (j0 + j < 3)
                            gn[j0 + j] = g2;
                        r[j0 + j] = g;
                    }
                }
            }
            if (u == 0)  // the first nbx columns of the grid are near band: not part of the far-field sum
                sqf -= (nbx > 0 ? gn[0] : 0.f) + (nbx > 1 ? gn[1] : 0.f) + (nbx > 2 ? gn[2] : 0.f);
            sq += rownear ? 0.f : sqf;
            near_get_g(r, gexx, rownear, gy, u, exy, exx, nby, nbx, Gt, Gl);
        }
        // ---- MSE trace of this iteration (before the update): per-wave sums now, added up in a fixed order by thread 0 behind the
        // next barrier (no barrier of its own)
        if (errors) {
            const double ws = KRES > 0 ? wave_sum_at((double)sq, lane) : wave_sum((double)sq);
            if (lane == 0)
                part[wave] = ws;
        }
        __builtin_amdgcn_sched_barrier(0);
        SRX_PSTAMP(9);
        // ---- H-bwd
        {
            gnbr_put(r, Rown, SLOT1, lane);
            __syncthreads();
            if (errors && tid == 0) {
                double t = 0.0;
#pragma unroll
                for (int i = 0; i < 16; i++)
                    t += part[i];
                errors[(size_t)b * n_iter + it] = (t + Vtot[b]) * scale;
            }
            const float gtop = exx ? gexx : r[0];
            // (written out: with gnbr_get here the count-plane float forms of the 7 x 7 PSF take 4 more bytes of scratch)
            const float gm1 = u == 0 ? gtop : Rlf[SLOT1 + 128 + lane];
            const float gp1 = u == 3 ? 0.f : Rrt[SLOT1 + lane], gp2 = u == 3 ? 0.f : Rrt[SLOT1 + 64 + lane];
            float hlo[3], hhi[3];  // (unused here: the adjoint 7 x 7 runs once, in stage C)
            bwd_chain_x<PSF == 0>(r, a, u == 0, u == 3, Rown, Rlf, Rrt, SLOT0 + 384, SLOT0, lane, sload8(awx + 16), sload8(awx + 8), gm1, gp1, gp2, gtop, [](int) {},
                                  [](int, float v) { return v; }, hlo, hhi);
        }
        __builtin_amdgcn_sched_barrier(0);
        SRX_PSTAMP(10);
        __syncthreads();  // every wave has read its neighbours' slots before the transposes overwrite them
        __builtin_amdgcn_sched_barrier(0);
        SRX_PSTAMP(11);
        transpose64(a, r, Rown, lane);
        __builtin_amdgcn_sched_barrier(0);
        SRX_PSTAMP(12);
        }
        {  // ---------------- stage C ----------------
        SRX_STAGE_LOCALS();
        // ================= stage C: column layout again, r[i] = row 64 s + i (row 63 of s == 3: the wrapped row -1) =================
        float hv[16], hw[16];  // the parked state, 16 rows at a time
        {
            if (exy && s == 3) {
                rowbuf[64 * u + lane] = r[63];
                r[63] = 0.f;
            }
            gnbr_put(r, Rown, SLOT0, lane);
            __syncthreads();
            const float gtop = exy ? rowbuf[64 * u + lane] : r[0];
            const GNbr<float> nbr = gnbr_get(s == 0, s == 3, Rup, Rdn, SLOT0, lane, gtop);
            auto mid = [&](int q) {
                          // the parked state in 16-row batches, at most two in flight: batch q is consumed by quarter q of the blur, the parked
                          // batches PB0 .. 3 land in hv and hw alternately.  With resident rows no batch is consumed in the quarter whose hook
                          // requests it (quarter 0 takes xs): every request has a quarter of the blur as cover
                          auto load16 = [&](float(&ld)[16], int bq) {
                              int pk = park0;
                              asm volatile("" : "+s"(pk));
#pragma unroll
                              for (int q = 0; q < 4; q++)
                                  ld4(rs_out, l4 * 4, pk + (4 * bq + q) * 1024, ld[4 * q], ld[4 * q + 1], ld[4 * q + 2], ld[4 * q + 3]);
                          };
                          if (q == 0)
                              SRX_PSTAMP(13);
                          if (KRES == 0) {
                              if (q == 0)
                                  load16(hv, 0), load16(hw, 1);
                              if (q == 1)
                                  load16(hv, 2);
                              else if (q == 2)
                                  load16(hw, 3);
                          } else {
                              if (q == 0)
                                  load16(hv, 1), load16(hw, 2);
                              else if (q == 2)
                                  load16(hv, 3);
                          }
                      };
            auto post = [&](int i, float corr) {
                          // the update, fused into the blur's epilogue: hr <- clip(hr + step * corr / N, 0, 255), one v_med3_f32
                          const float old = i < KRES ? xs[i < KRES ? i : 0] : (((i >> 4) - PB0) & 1) ? hw[i & 15] : hv[i & 15];
                          return __builtin_amdgcn_fmed3f(fmaf(corr, sn, old), 0.f, 255.f);
                      };
            if (PSF == 0) {
                bwd_chain(r, a, s == 0, s == 3, Rown, Rup, Rdn, SLOT1 + 384, SLOT1, lane, sload8(awy + 16), sload8(awy + 8), nbr.gm1, nbr.gp1, nbr.gp2, gtop, mid, post);
            } else {  // the coefficients, then the adjoint 7 x 7 of both directions; the update is the epilogue of its second pass
                float hl[3], hr[3];
                bwd_chain_x<false>(r, a, s == 0, s == 3, Rown, Rup, Rdn, SLOT1 + 384, SLOT1, lane, sload8(awy + 16), sload8(awy + 8), nbr.gm1, nbr.gp1, nbr.gp2, gtop,
                                   [](int) {}, [](int, float v) { return v; }, hl, hr);
                blur2d_cols<PSF == 2 ? 2 : 3>(a, hl, hr, u == 0, u == 3, Rown, Rlf, Rrt, lane, tb.k2 + 56, mid, post);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        SRX_PSTAMP(14);
        }
#undef SRX_STAGE_LOCALS
    }
    {
        // the result goes out in image layout, over the parking layout: not before every wave has re-read its last parked rows
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        const int l4 = (KRES > 0 ? lane_here() : tid0 & 63) * 4;
#pragma unroll
        for (int i = 0; i < 64; i++)
            fused::buf_store<float>(a[i], rs_out, l4 + (i & 3) * PN * 4, cb0 + (i >> 2) * PN * 16);
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------
static inline void fill_axis(const mosaic::AxisPlan &pl, const float *cfwd, const float *cbwd, AxisC &ax, AxisW &aw)
{
    const double kq = -6.0 * ZD;
    double wv[4];
    fused::host_weights(1.0 - pl.delta, wv);
    for (int i = 0; i < 4; i++)
        aw.wfb[i] = (float)wv[i];
    fused::host_weights(pl.delta, wv);
    for (int i = 0; i < 4; i++)
        aw.wfb[4 + i] = (float)(kq * wv[i]);
    aw.kb[7] = aw.kt[7] = 0.f;
    for (int i = 0; i < 7; i++)
        aw.kb[i] = (float)(kq * (double)cfwd[i]), aw.kt[i] = cbwd[i];
    ax.ex = pl.nmax, ax.nb = -pl.nmin, ax.E = pl.E;
}
static inline void fill_near(PatchArgs &pa)  // (behind fill_axis of both axes)
{
    pa.ntop = near_top(PN, pa.y.ex, pa.x.ex, pa.y.nb);
    pa.nn = near_count(PN, PN, pa.y.ex, pa.x.ex, pa.y.nb, pa.x.nb);
}

// Full phase grids (every frame its own (row class, column class), classes distinct modulo f): each far-field HR pixel
// holds at most one sample and the count map is the product of a row mask and a column mask.
static inline bool c01_masks(const mosaic::AxisPlan &py, const mosaic::AxisPlan &px, int N, int f, unsigned long long ry[4],
                             unsigned long long rx[4])
{
    int ny[SRX_MAX_FRAMES], nx[SRX_MAX_FRAMES], cy = 0, cx = 0;
    for (int k = 0; k < N; k++) {
        bool fy = false, fx = false;
        for (int j = 0; j < cy; j++)
            fy = fy || ny[j] == py.n[k];
        for (int j = 0; j < cx; j++)
            fx = fx || nx[j] == px.n[k];
        if (!fy)
            ny[cy++] = py.n[k];
        if (!fx)
            nx[cx++] = px.n[k];
        for (int j = 0; j < k; j++)
            if (py.n[j] == py.n[k] && px.n[j] == px.n[k])
                return false;  // two frames on one phase
    }
    if (cy * cx != N)
        return false;
    for (int i = 0; i < cy; i++)
        for (int j = 0; j < i; j++)
            if ((ny[i] - ny[j]) % f == 0)
                return false;
    for (int i = 0; i < cx; i++)
        for (int j = 0; j < i; j++)
            if ((nx[i] - nx[j]) % f == 0)
                return false;
    for (int w = 0; w < 4; w++)
        ry[w] = rx[w] = 0ull;
    for (int g = 0; g < PN; g++) {
        for (int i = 0; i < cy; i++) {
            const int uu = g + ny[i];
            if (uu >= 0 && uu <= PN - 1 && uu % f == 0)
                ry[g >> 6] |= 1ull << (g & 63);
        }
        for (int i = 0; i < cx; i++) {
            const int uu = g + nx[i];
            if (uu >= 0 && uu <= PN - 1 && uu % f == 0)
                rx[g >> 6] |= 1ull << (g & 63);
        }
    }
    return true;
}

// Which G step a call on these plans takes: 0 the count plane, 1 the 0/1 masks of a full phase grid, tested per row and column, 2 the masks
// known to be all ones (k_ibp_patch's FORM 1, the rank-1 kernel's byte-mosaic form).  It computes G = M - Y where the masks say
// G = ry[gy] rx[gx] ? M - Y : 0, so every bit it no longer looks at must be set wherever that G is used:
//   * columns 0 .. PN - 2, all of them (the squares of the first nbx columns are added to the far-field sum and subtracted again: they must
//     be the same numbers); column PN - 1 -- the grid's empty last column when exx = 1 -- keeps its test in the kernel;
//   * rows nby .. PN - 1 - exy: the rows before them and the wrapped row -1 take G from the near-band strips and add nothing to the sum.
static inline int gstep_form(const mosaic::AxisPlan &py, const mosaic::AxisPlan &px, int N, int f, unsigned long long ry[4], unsigned long long rx[4])
{
    if (!c01_masks(py, px, N, f, ry, rx))
        return 0;
    const int nby = -py.nmin, exy = py.nmax > 0 ? 1 : 0;
    for (int g = 0; g < PN - 1; g++)
        if (!((rx[g >> 6] >> (g & 63)) & 1ull))
            return 1;
    for (int g = nby > 0 ? nby : 0; g < PN - exy; g++)
        if (!((ry[g >> 6] >> (g & 63)) & 1ull))
            return 1;
    return 2;
}

// device memory of the patch path's tables, carved from the caller's workspace by mosaic::ibp
// class tables of a full phase grid: which frames land on natural coordinate g along one axis (their class) and the LR index they bring
static inline bool axis_map(const mosaic::AxisPlan &pl, int N, int f, AxisMap &am, int cls_of_frame[SRX_MAX_FRAMES], int &ncls)
{
    int nv[SRX_MAX_FRAMES];
    ncls = 0;
    for (int k = 0; k < N; k++) {
        int c = -1;
        for (int j = 0; j < ncls; j++)
            if (nv[j] == pl.n[k])
                c = j;
        if (c < 0) {
            if (ncls == 4)
                return false;
            c = ncls, nv[ncls++] = pl.n[k];
        }
        cls_of_frame[k] = c;
    }
    for (int g = 0; g < PN; g++) {
        am.cls[g] = -1, am.idx[g] = 0;
        for (int c = 0; c < ncls; c++) {
            const int uu = g + nv[c];  // k_build_mtaps: u = p + n - 13 with p = g + 13
            if (uu >= 0 && uu <= PN - 1 && uu % f == 0)
                am.cls[g] = (signed char)c, am.idx[g] = (unsigned char)(uu / f);
        }
    }
    return true;
}

// flags: the call's (SRX_FLAG_DIAG_NO_ZERO_FUSE)
static inline bool builds_itself(const mosaic::AxisPlan &py, const mosaic::AxisPlan &px, int N, int f, unsigned flags)
{
    unsigned long long ry[4], rx[4];
    if ((flags & SRX_FLAG_DIAG_NO_ZERO_FUSE) || !c01_masks(py, px, N, f, ry, rx) || PN / f > 255)
        return false;  // (SRX_FLAG_DIAG_NO_ZERO_FUSE: the cross-check -- the tables through the batch's M / C / Mu planes, as round 3 built them)
    BuildMaps bm;
    int cy[SRX_MAX_FRAMES], cx[SRX_MAX_FRAMES], ny, nx;
    return axis_map(py, N, f, bm.y, cy, ny) && axis_map(px, N, f, bm.x, cx, nx) && ny * nx == N;
}

// the counts the workspace layout depends on (a patch is PN x PN; its near band has at most NN_PAD pixels)
struct Dims {
    size_t B, ngrp;
};
// what a call carves, in this order; PatchTabs is its read-only view for the kernel
struct Carved {
    BuildMaps *maps;
    float *Mt;
    unsigned *Mt8;
    int *m8;
    float *Ct;
    uint2 *nrec, *nent;
    float2 *Mn;
    AxisW *aw;
    float *k2;
};
// the layout: on the call's arena it is the carve, on a counting one the size (a braced list is evaluated left to right)
static Carved carve(Arena &ar, const Dims &d)
{
    return {ar.take<BuildMaps>(1), ar.take<float>(d.B * PN * PN), ar.take<unsigned>(d.B * (PN / 4) * PN), ar.take<int>(d.B), ar.take<float>((size_t)PN * PN),
            ar.take<uint2>(NN_PAD), ar.take<uint2>(d.ngrp * NN_PAD), ar.take<float2>(d.B * NN_PAD), ar.take<AxisW>(2), ar.take<float>(112)};
}
static inline size_t tabs_bytes(const IbpShape &s, int B)
{
    return measured([&](Arena &m) { carve(m, Dims{(size_t)B, ((size_t)s.N + 3) / 4}); });
}

// a PSF that is not rank 1: the 7 x 7 weights in column layout (lane-direction tap, then register-direction tap), the forward ones times
// kq^2, to k2 (PatchTabs::k2)
static int upload_k2(const fused::Kernel7<float> &kc, const fused::Kernel7<float> &kt, float *k2, hipStream_t st)
{
    const double kq = -6.0 * ZD;
    float kv[112];
    for (int c = 0; c < 7; c++)
        for (int r = 0; r < 8; r++) {
            kv[8 * c + r] = r < 7 ? (float)(kq * kq * (double)kc.k[7 * r + c]) : 0.f;
            kv[56 + 8 * c + r] = r < 7 ? kt.k[7 * r + c] : 0.f;
        }
    return upload_record(st, k2, kv);
}

// the iteration loop; the per-call tables (M, C, Mu, near lists, Vtot) are srx_mosaic.hpp's common_prep()'s
static int iterate(const mosaic::Common<float> &c, const float *hr_init, float *hr, int n_iter, double *errors, Arena &ar, hipStream_t st)
{
    const int B = c.B, N = c.N, f = c.f, NS = c.NS;
    const mosaic::AxisPlan &py = c.py, &px = c.px;
    const int Hg = PN + 27, Wg = PN + 27, ngrp = NS / 4;
    const auto [maps, Mt, Mt8, m8, Ct, nrec, nent, Mn, aw, k2] = carve(ar, Dims{(size_t)B, (size_t)ngrp});
    if (!ar.ok)
        return SRX_E_WORKSPACE;
    PatchArgs pa;
    AxisWPair awp;
    fill_axis(py, c.kc.cy, c.kt.cy, pa.y, awp.y);
    fill_axis(px, c.kc.cx, c.kt.cx, pa.x, awp.x);
    pa.sn = (float)c.step / (float)N;
    fill_near(pa);
    pa.ngrp = ngrp;
    if (pa.nn > NN_PAD)
        return SRX_E_UNSUPPORTED;
    const int gform = gstep_form(py, px, N, f, pa.ry, pa.rx);
    pa.c01 = gform > 0 ? 1 : 0;
    const AxisTiles one = one_region(PN);
    const int nblk = cdiv(pa.nn, 256);
    if (!c.own_build) {
        SRX_TRY((block_setup<float, float2>(c, one, one, PN, PN, pa.y, pa.x, nblk, Mt, Ct, Mt8, m8, nullptr, nrec, nent, Mn, st)));
    } else {  // common_prep built no M / C / Mu: the same tables straight from the frames
        if (fill_bytes(m8, 0xff, (size_t)B * sizeof(int), st) != hipSuccess)
            return SRX_E_HIP;
        BuildMaps bm;
        int cy[SRX_MAX_FRAMES], cx[SRX_MAX_FRAMES], ny, nx;
        axis_map(py, N, f, bm.y, cy, ny);
        axis_map(px, N, f, bm.x, cx, nx);
        for (int a = 0; a < 4; a++)
            for (int b = 0; b < 4; b++)
                bm.frame[a][b] = 0;
        for (int q = 0; q < N; q++)
            bm.frame[cy[q]][cx[q]] = (signed char)q;
        bm.nby = pa.y.nb, bm.nbx = pa.x.nb;
        SRX_TRY(upload_record(st, maps, bm));
        if (c.lr_u8) {  // byte frames: the byte plane of every patch and nothing else (m8 keeps its preset: no patch asks for the float plane)
            if (!(c.flags & SRX_FLAG_DIAG_U8_BYTE_LOADS) && c.w % 4 == 0 && nx * c.w <= PN)  // (the column classes' rows fill at most 64 words)
                SRX_LAUNCH(KID_PATCH_BUILD, (k_patch_build<0, uint8_t, true>), dim3(PN / 16, B), dim3(256), 0, st, (const uint8_t *)c.lr, N, c.h, c.w, maps, m8, Mt, Mt8);
            else
                SRX_LAUNCH(KID_PATCH_BUILD, (k_patch_build<0, uint8_t>), dim3(PN / 16, B), dim3(256), 0, st, (const uint8_t *)c.lr, N, c.h, c.w, maps, m8, Mt, Mt8);
        } else {
            SRX_LAUNCH(KID_PATCH_BUILD, k_patch_build<0>, dim3(PN / 16, B), dim3(256), 0, st, (const float *)c.lr, N, c.h, c.w, maps, m8, Mt, Mt8);
            SRX_LAUNCH(KID_PATCH_FLAGS, k_patch_build<1>, dim3(PN / 16, B), dim3(256), 0, st, (const float *)c.lr, N, c.h, c.w, maps, m8, Mt, Mt8);
        }
        if (pa.nn > 0) {
            SRX_TRY(near_tab(c, one, one, PN, PN, pa.y, pa.x, nblk, nullptr, nrec, nent, st));
            if (c.lr_u8)
                hipLaunchKernelGGL(k_patch_near_build<uint8_t>, dim3(nblk, B), dim3(256), 0, st, (const uint8_t *)c.lr, N, c.h, c.w, c.tabY, c.tabX, Hg, Wg, py.D, px.D,
                                   pa.y.ex, pa.x.ex, pa.y.nb, pa.x.nb, pa.nn, Mn, c.Vtot);
            else
                hipLaunchKernelGGL(k_patch_near_build<float>, dim3(nblk, B), dim3(256), 0, st, (const float *)c.lr, N, c.h, c.w, c.tabY, c.tabX, Hg, Wg, py.D, px.D,
                                   pa.y.ex, pa.x.ex, pa.y.nb, pa.x.nb, pa.nn, Mn, c.Vtot);
            SRX_CHECK_LAUNCH();
        }
    }
    SRX_TRY(upload_record(st, aw, awp));
    const int psf = fused::psf_form(c.kc, c.kt);
    if (psf != 0)
        SRX_TRY(upload_k2(c.kc, c.kt, k2, st));
    PatchTabs tb{Mt, Mt8, m8, Ct, aw, nrec, nent, Mn, k2};
    // both mosaic forms over the whole batch: every patch is iterated by exactly one of the two launches (the m8 flag)
#define SRX_PATCH_PAIR(C01_, PSF_)                                                                                                              \
    do {                                                                                                                                        \
        SRX_LAUNCH(KID_IBP_PATCH, (k_ibp_patch<C01_, true, PSF_>), dim3(B), dim3(1024), 0, st, hr_init, hr, tb, pa, c.Vtot, c.scale, errors, n_iter);  \
        SRX_LAUNCH(KID_IBP_PATCH, (k_ibp_patch<C01_, false, PSF_>), dim3(B), dim3(1024), 0, st, hr_init, hr, tb, pa, c.Vtot, c.scale, errors, n_iter); \
    } while (0)
    if (pa.c01) {
        if (psf == 0 && gform == 2) {  // (the float-mosaic twin has no mask test to drop: the instantiation of the pair below)
            SRX_LAUNCH(KID_IBP_PATCH, (k_ibp_patch<true, true, 1>), dim3(B), dim3(1024), 0, st, hr_init, hr, tb, pa, c.Vtot, c.scale, errors, n_iter);
            SRX_LAUNCH(KID_IBP_PATCH, (k_ibp_patch<true, false, 0>), dim3(B), dim3(1024), 0, st, hr_init, hr, tb, pa, c.Vtot, c.scale, errors, n_iter);
        } else if (psf == 0)
            SRX_PATCH_PAIR(true, 0);
        else if (psf == 2)
            SRX_PATCH_PAIR(true, 2);
        else
            SRX_PATCH_PAIR(true, 3);
    } else {
        if (psf == 0)
            SRX_PATCH_PAIR(false, 0);
        else if (psf == 2)
            SRX_PATCH_PAIR(false, 2);
        else
            SRX_PATCH_PAIR(false, 3);
    }
#undef SRX_PATCH_PAIR
    return SRX_OK;
}

}  // namespace patch
}  // namespace srx
