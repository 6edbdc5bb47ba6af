// srx_dtile.hpp -- delta != 0 IBP iteration of a LARGE frame on register-resident windows, ONE launch per iteration.
//
// srx_patch.hpp runs a whole 256 x 256 patch in the registers of one compute unit; a frame does not fit, and the tile kernels of
// srx_mosaic.hpp that took frames with a common sub-pixel fraction (the x4 phase grids of SURVEY 8d C3: 768 x 1024 -> 3072 x 4096)
// move 32 B per HR pixel through HBM in three launches (0.156 of the roofline, BENCH_r02).  Here the frame is cut into overlapping
// WINDOWS of 256 rows x 64 NSX columns and a workgroup runs k_ibp_patch's chain on its window as if it were a whole image:
//
//   * A window edge that is not an image edge starts its recursions from the steady state of a constant signal -- exactly what the
//     image-edge closed forms of srx_patch.hpp give -- and the transient decays as |z|^k: 32 pixels in from the edge (3 blur + 11 + 2
//     FIR, then 2 + 11 + 3 backwards) every value agrees with the whole-image result to |z|^11 = 5e-7 of the signal's deviation, the
//     warm-up length R the tile kernels use for float32.  A window OWNS (stores, counts in the MSE trace) only the pixels at least 32
//     from its interior edges; windows at an image edge end exactly there, so the closed forms of SciPy's pad apply where they hold.
//   * The state ping-pongs between two planes (a window reads its neighbours' pixels of the previous iteration) in a layout of
//     its own: four rows interleaved ([H / 4][W][4]), one 16-byte access per lane and four rows -- a CU issues one vector memory
//     instruction per ~9 cycles whatever its width (srx_patch.hpp), and a window loads, re-reads and stores 64 rows per wave.
//   * Window shape: 4 x 4 waves (256 x 256, 192 x 192 owned) recompute the least; 4 x 3 waves (256 x 192) leave fewer idle compute
//     units when ONE frame is all there is (3072 x 4096: 336 windows of 16 waves = 1.31 rounds of 256 CUs at 55 us per round, or 512 of
//     12 waves = 2.00 rounds at 37 us).  plan() picks by modelled time of one frame.
//   * Near band, count masks, byte mosaic: k_ibp_patch's, per window (only windows on the top / left image edge hold near-band
//     pixels; the tables are built per such window, by patch::block_setup as the patch's own).  The near band's code is srx_patch.hpp's too (patch::near_count, near_put_y, near_px,
//     near_get_g_left; whole rows of G come back eight columns at a time here), the exchanges around the chains srx_block.hpp's.
#pragma once
#include "srx_patch.hpp"

namespace srx {
namespace dtile {

using patch::AxisC;
using patch::AxisW;
using blk::f8;
using blk::ld4;
using blk::ld_u2;
using patch::NN_PAD;
using blk::RW;
using blk::sload8;
using blk::SLOT0;
using blk::SLOT1;
using blk::st4;
using blk::u32x4;
using patch::YW;

constexpr int RY = 256;    // window rows (4 block rows)
constexpr int HL = 32;     // halo: 3 + 11 + 2 + 2 + 11 + 3
constexpr int ALIGN_Y = 4, ALIGN_X = 16;  // origins / ownership boundaries: whole row quads, whole 16-column byte groups

template <int NSX> struct Lds {
    static constexpr int NW = 4 * NSX;
    static constexpr int OFF_YT = NW * RW, OFF_YL = OFF_YT + 4 * YW, OFF_GT = OFF_YL + 4 * YW, OFF_GL = OFF_GT + 3 * YW,
                         OFF_ROW = OFF_GL + 3 * YW, OFF_PART = OFF_ROW + 256, WORDS = OFF_PART + 2 * NW + 2;
    static_assert(WORDS * 4 <= 160 * 1024, "LDS budget");
};

struct TileD {  // 8 ints, one scalar load
    int oy, ox;          // window origin (image coordinates)
    int y0, y1, x0, x1;  // owned range, window-local
    int ntab;            // near-band table of this window, or -1
    int flags;           // 1: on the top image edge, 2: on the left image edge; ty << 8, tx << 20
};

struct DArgs {
    int H, W, tiles_x, tiles_y;
    AxisC y, x;
    int ngrp, c01;
    float sn;
};

struct DTabs {
    const float *Mt;        // [B][W / 4][H][4] far-field LR mosaic, transposed, four columns interleaved (natural coordinates)
    const unsigned *Mt8;    // [B][W / 16][H][4]: the same as bytes (valid where m8[b])
    const int *m8;          // [B]
    const float *Ct;        // [W / 4][H][4] count map (unused when c01)
    const AxisW *aw;        // [2]
    const TileD *tiles;     // [tiles_y * tiles_x]
    const unsigned long long *rowm, *colm;  // [tiles_y][4], [tiles_x][4]: 0/1 count masks of the windows' rows / columns (c01)
    const int *nn;          // [ntabs] near-band pixels per table
    const uint2 *nrec;      // [ntabs][NN_PAD]
    const uint2 *nent;      // [ngrp][ntabs][NN_PAD]
    const float2 *Mn;       // [B][ntabs][NN_PAD]
    int ntabs;
    const float *k2;        // srx_patch.hpp's 7 x 7 weight tables (a PSF that is not rank 1)
};

// ---- host-side plan (AxisTiles is declared in srx_patch.hpp, whose set-up kernels take the plan) -----------------------------------
// windows of length RL over [0, L): the first starts at 0, the last ends at L, each owns a span whose HL-neighbourhood it contains
static inline bool plan_axis_tiles(int L, int RL, int align, AxisTiles &at)
{
    if (L < RL || L % align)
        return false;
    if (L == RL) {
        at.n = 1, at.o[0] = 0, at.a[0] = 0, at.a[1] = L;
        return true;
    }
    const int edge = RL - HL, mid = RL - 2 * HL;
    int n = L <= 2 * edge ? 2 : 2 + (L - 2 * edge + mid - 1) / mid;
    for (;; n++) {  // even split, boundaries rounded to the alignment; one more window if rounding broke a containment
        if (n > 64)
            return false;
        bool ok = true;
        at.n = n, at.a[0] = 0, at.a[n] = L;
        for (int t = 1; t < n; t++)
            at.a[t] = (int)(((long long)t * L / n + align / 2) / align * align);
        for (int t = 0; t < n && ok; t++) {
            const int lo = t == 0 ? 0 : at.a[t] - HL, hi = t == n - 1 ? L : at.a[t + 1] + HL;
            int o = t == n - 1 ? L - RL : std::max(lo, 0) / align * align;
            o = std::min(o, L - RL);
            at.o[t] = o;
            ok = o <= lo && o + RL >= hi && o % align == 0 && at.a[t + 1] > at.a[t];
        }
        if (ok)
            return true;
    }
}

// what plan() admits at most: the bounds of the shape-only workspace query
constexpr int MAX_TILES = 1024;       // windows of a frame
constexpr int MAX_TABS = 64 + 64;     // near-band tables, one per window of the first row and column: tx.n + ty.n - 1 with at most 64 windows per axis

struct Plan {
    int nsx;
    AxisTiles ty, tx;
};

// flags: the call's (SRX_FLAG_DIAG_WIDE_WINDOWS); eligible() and iterate() pass the same, the spec's and the prepared call's copy of it
static inline bool plan(int H, int W, unsigned flags, Plan &pl)
{
    // 4 x 3 waves (256 x 192 windows, 128 x 192 owned in the interior) unless the caller asks for the 16-wave shape.  Round 3 chose between
    // the two by a cost model of ONE frame (a round of 12-wave windows 37 us, of 16-wave windows 55 us on 3072 x 4096; eight frames 592
    // against 574 us per iteration: what the narrow shape loses on a batch is 3 %).  Round 4 drops the choice: the 16-wave kernel has 128
    // registers per lane and does not fit them (44 spilled registers with 0/1 count masks, 142 with a count plane -- after this round's
    // fixes; 72 / 246 before), the 12-wave one has 168 and is clean, and every width the wide shape takes the narrow one takes too.  The
    // plan depends on the shape only, so a batch gives every item the bits it gets alone.
    Plan p;
    p.nsx = (flags & SRX_FLAG_DIAG_WIDE_WINDOWS) ? 4 : 3;
    if (!plan_axis_tiles(H, RY, ALIGN_Y, p.ty) || !plan_axis_tiles(W, 64 * p.nsx, ALIGN_X, p.tx))
        return false;
    if ((long)p.ty.n * p.tx.n > MAX_TILES)
        return false;
    pl = p;
    return true;
}

// the superset of every shape plan() admits whatever the call flags say: what the shape-only workspace bound tests (256-row windows of
// 192 (4 x 3 waves) or 256 columns, origins on row quads / 16-column groups)
static inline bool shape_admits(const IbpShape &s) { return s.eb == 4 && s.H >= RY && s.W >= 64 * 3 && s.H % ALIGN_Y == 0 && s.W % ALIGN_X == 0; }

static inline bool eligible(const IbpSpec &s)
{
    const int f = s.f;
    if (!shape_admits(s) || f < 2 || (s.H == patch::PN && s.W == patch::PN && !(s.flags & SRX_FLAG_DIAG_WIDE_WINDOWS)) || (s.flags & SRX_FLAG_TILES))
        return false;
    mosaic::AxisPlan py, px;
    if (!mosaic::plan_axis(s.N, s.sh, 0, f, py) || !mosaic::plan_axis(s.N, s.sh, 1, f, px))
        return false;
    fused::Kernel7<float> kc;
    fused::make_kernel7<float>(s.k, s.kh, s.kw, false, kc, s.flags);
    // (round 4: a PSF that is not rank 1 on the 12-wave windows, srx_patch.hpp's 7 x 7 form -- when its outer ring is zero, as the reference's
    // measured PSF's is: 131 us per iteration on 3072 x 4096 at x4 against the tile kernels' 141; with full 7 x 7 support the windows take 164
    // (53 - 71 spilled registers under the 168-register cap) and the tile kernels keep the call)
    if (!kc.separable) {
        bool ring0 = !(s.flags & SRX_FLAG_DIAG_WIDE_WINDOWS);
        for (int i = 0; i < 7; i++)
            for (int e : {i, 42 + i, 7 * i, 7 * i + 6})
                ring0 = ring0 && kc.k[e] == 0.f;
        if (!ring0)
            return false;
    }
    if (!(patch::axis_ok(py, f) && patch::axis_ok(px, f)))
        return false;
    Plan pl;
    if (!plan(s.H, s.W, s.flags, pl))
        return false;
    const int exy = py.nmax, nby = -py.nmin, exx = px.nmax, nbx = -px.nmin;
    return patch::near_count(RY, 256, exy, exx, nby, nbx) <= NN_PAD;  // the corner window's near band (at its widest, 4 x 4 waves) fits its lists
}

// ---- once per call ---------------------------------------------------------------------------------------------------------
// image [H][W] <-> state plane [H / 4][W][4].  grid (ceil(W/256), H / 4, B)
__global__ void __launch_bounds__(256) k_dtile_copy_in(const float *__restrict__ src, int H, int W, float *__restrict__ dst)
{
    const int x = blockIdx.x * 256 + threadIdx.x, q = blockIdx.y, b = blockIdx.z;
    if (x >= W)
        return;
    const float *s = src + ((size_t)b * H + 4 * q) * W + x;
    reinterpret_cast<float4 *>(dst)[((size_t)b * (H / 4) + q) * W + x] = make_float4(s[0], s[W], s[2 * (size_t)W], s[3 * (size_t)W]);
}
__global__ void __launch_bounds__(256) k_dtile_copy_out(const float *__restrict__ src, int H, int W, float *__restrict__ dst)
{
    const int x = blockIdx.x * 256 + threadIdx.x, q = blockIdx.y, b = blockIdx.z;
    if (x >= W)
        return;
    const float4 v = reinterpret_cast<const float4 *>(src)[((size_t)b * (H / 4) + q) * W + x];
    float *d = dst + ((size_t)b * H + 4 * q) * W + x;
    d[0] = v.x, d[W] = v.y, d[2 * (size_t)W] = v.z, d[3 * (size_t)W] = v.w;
}

// (the operand planes Mt / Ct / Mt8 / m8 of the whole frame and the near-band tables of the windows on the top / left image edge are
// srx_patch.hpp's: patch::block_setup with this plan)

// MSE trace of the LAST iteration from the windows' partial sums, fixed order (the same order as the in-kernel sum of the earlier
// iterations: lane-strided, wave tree, waves in turn).  grid B, block NTHR of the iteration kernel
template <int NTHR>
__global__ void __launch_bounds__(NTHR)
    k_dtile_trace(const double *__restrict__ epart, int ntiles, const double *__restrict__ Vtot, double scale, double *__restrict__ errors, int stride)
{
    __shared__ double part[NTHR / 64];
    const int b = blockIdx.x, tid = threadIdx.x;
    double sacc = 0.0;
    for (int i = tid; i < ntiles; i += NTHR)
        sacc += epart[(size_t)b * ntiles + i];
    sacc = wave_sum(sacc);
    if ((tid & 63) == 0)
        part[tid >> 6] = sacc;
    __syncthreads();
    if (tid == 0) {
        double t = 0.0;
        for (int i = 0; i < NTHR / 64; i++)
            t += part[i];
        errors[(size_t)b * stride] = (t + Vtot[b]) * scale;
    }
}

// =========================================================================================================================
// One iteration of one window.  grid (tiles, B), block 256 NSX: wave (s, u) owns the 64 x 64 block at window rows 64 s, columns 64 u.
// The stages are k_ibp_patch's (srx_patch.hpp has the derivations); what differs is where the state comes from and goes to, the
// operand planes' pitch, and that the MSE sum and the store are restricted to the pixels this window owns.
// =========================================================================================================================
template <bool C01, bool M8, int NSX, int PSF>  // PSF: srx_patch.hpp's forms -- 0 rank 1, 3 full 7 x 7, 2 a 7 x 7 whose outer ring is zero
__device__ __forceinline__ void dtile_body(float *lds, const float *__restrict__ hr_src, float *__restrict__ hr_dst, const DTabs &tb, const DArgs &da,
                                           double *__restrict__ epart, const double *__restrict__ eprev, const double *__restrict__ Vtot, double scale,
                                           double *__restrict__ err_prev, int err_stride)
{
    using L = Lds<NSX>;
    constexpr int NW = L::NW, NTHR = 64 * NW, NPT = (NN_PAD + NTHR - 1) / NTHR;  // near-band pixels per thread
    const int tid0 = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid0 >> 6), s = wave / NSX, u = wave - s * NSX;
    const int b = blockIdx.y;
    const unsigned wid = xcd_index(blockIdx.x, gridDim.x);  // windows that share halos (32 of 256 / 192) on one XCD's L2
    constexpr int m8 = M8 ? 1 : 0;
    TileD td;
    {
        typedef int i8 __attribute__((ext_vector_type(8)));
        i8 v;
        const TileD *p = tb.tiles + wid;
        asm volatile("s_load_dwordx8 %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=s"(v) : "s"(p) : "memory");
        td.oy = v[0], td.ox = v[1], td.y0 = v[2], td.y1 = v[3], td.x0 = v[4], td.x1 = v[5], td.ntab = v[6], td.flags = v[7];
    }
    const int H = da.H, W = da.W;
    float *Rown = lds + wave * RW;
    const float *Rup = lds + (wave - NSX) * RW, *Rdn = lds + (wave + NSX) * RW;
    const float *Rlf = lds + (wave - 1) * RW, *Rrt = lds + (wave + 1) * RW;
    float *Ystrip = lds + L::OFF_YT, *Gstrip = lds + L::OFF_GT, *rowbuf = lds + L::OFF_ROW;
    float *Yt = lds + L::OFF_YT, *Yl = lds + L::OFF_YL, *Gt = lds + L::OFF_GT, *Gl = lds + L::OFF_GL;
    double *part = reinterpret_cast<double *>(lds + L::OFF_PART);
    const bool top = td.flags & 1, left = td.flags & 2;
    const int exy = top ? da.y.ex : 0, nby = top ? da.y.nb : 0, exx = left ? da.x.ex : 0, nbx = left ? da.x.nb : 0;
    const int nn = td.ntab >= 0 ? __builtin_amdgcn_readfirstlane(tb.nn[td.ntab]) : 0;
    const size_t plane = (size_t)H * W;
    const __amdgpu_buffer_rsrc_t rs_src = fused::plane_rsrc(hr_src + (size_t)b * plane, plane);
    const __amdgpu_buffer_rsrc_t rs_dst = fused::plane_rsrc(hr_dst + (size_t)b * plane, plane);
    const float *awy = tb.aw[0].kb, *awx = tb.aw[1].kb;
    const float sn = da.sn;
    // The MSE trace of the PREVIOUS iteration: its windows' partial sums, added up in a fixed order by one window of this launch
    // (srx_ztile.hpp does the same); the last iteration's is k_dtile_trace's.
    if (eprev && (int)wid == min(da.tiles_x + 1, (int)gridDim.x - 1)) {
        double sacc = 0.0;
        for (int i = tid0; i < (int)gridDim.x; i += NTHR)
            sacc += eprev[(size_t)b * gridDim.x + i];
        sacc = wave_sum(sacc);
        if ((tid0 & 63) == 0)
            part[wave] = sacc;
        __syncthreads();
        if (tid0 == 0) {
            double t = 0.0;
#pragma unroll
            for (int i = 0; i < NW; i++)
                t += part[i];
            err_prev[(size_t)b * err_stride] = (t + Vtot[b]) * scale;
        }
        __syncthreads();
    }
    // state plane [H / 4][W][4]: lane = column, one 16-byte access = four rows
    const int sq0 = ((td.oy + 64 * s) >> 2) * W * 16;             // byte offset of this wave's first row quad
    const int tb0 = (((td.ox + 64 * u) >> 2) * H + td.oy + 64 * s) * 16;   // transposed operand planes [W / 4][H][4]: lane = row
    const int m80 = (((td.ox + 64 * u) >> 4) * H + td.oy + 64 * s) * 16;   // byte plane [W / 16][H][4]
    auto uniform64 = [](unsigned long long v) {  // (a vector load's result, the same in every lane, into scalar registers)
        return (unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)v) |  // (the builtin returns int: no sign extension)
               (unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(v >> 32)) << 32;
    };
    const unsigned long long rmask = C01 ? uniform64(tb.rowm[(size_t)((td.flags >> 8) & 0xfff) * 4 + s]) : 0ull;
    const unsigned long long cmask = C01 ? uniform64(tb.colm[(size_t)((td.flags >> 20) & 0xfff) * 4 + u]) : 0ull;

#define SRX_DT_LOCALS()                                              \
    int tid = tid0;                                                  \
    asm volatile("" : "+v"(tid));                                    \
    const int lane = tid & 63;                                       \
    int sql = sq0, tbl = tb0, m8l = m80;                             \
    asm volatile("" : "+s"(sql), "+s"(tbl), "+s"(m8l));              \
    const int vcol = (td.ox + 64 * u + lane) * 16;                   \
    (void)tbl, (void)m8l, (void)sql, (void)vcol

    float a[64], r[64];
    float yex = 0.f;
    {  // ================= stage A: column layout, lane = column 64 u + lane, a[i] = row 64 s + i =================
        SRX_DT_LOCALS();
#pragma unroll
        for (int q = 0; q < 16; q++)
            ld4(rs_src, vcol, sql + q * W * 16, a[4 * q], a[4 * q + 1], a[4 * q + 2], a[4 * q + 3]);
        if (PSF == 0) {
            blk::blur_block(a, s == 0, s == 3, Rown, Rup, Rdn, SLOT0, lane, sload8(awy));
        } else {  // round 4: srx_block.hpp's 7 x 7 form (blur2d_pass1 / blur2d_fix), here on a window: what lies beyond a window edge is zero for
                  // the blur as it is for the separable one (inside the halo nobody owns)
            blk::halo3_put(a, Rown, SLOT0, lane);
            __syncthreads();
            const blk::Halo3<float> h = blk::halo3_get(s == 0, s == 3, Rup, Rdn, SLOT0, lane);
            blk::blur2d_cols<PSF == 2 ? 2 : 3>(a, h.lo, h.hi, u == 0, u == NSX - 1, Rown, Rlf, Rrt, lane, tb.k2, [](int) {}, [](int, float v) { return v; });
        }
        __builtin_amdgcn_sched_barrier(0);
        blk::fwd_chain(a, s == 0, s == 3, Rown, Rup, Rdn, SLOT1, SLOT0, lane, sload8(awy + 16), yex);
        __builtin_amdgcn_sched_barrier(0);
        if (exy && s == 0)  // the Y row above the image rides in the window's last row (inside the halo: nobody owns it)
            rowbuf[64 * u + lane] = yex;
        __syncthreads();  // also: every wave is done with the exchange slots before the transposes overwrite them
        if (exy && s == 3)
            a[63] = rowbuf[64 * u + lane];
        __builtin_amdgcn_sched_barrier(0);
        blk::transpose64(a, r, Rown, lane);
        __builtin_amdgcn_sched_barrier(0);
    }
    float sq = 0.f;
    {  // ================= stage B: row layout, lane = row 64 s + lane, r[j] = column 64 u + j =================
        SRX_DT_LOCALS();
        const bool wrapped = exy && s == 3 && lane == 63;  // this lane holds row -1
        const int gy = wrapped ? -1 : 64 * s + lane;       // window-local natural row
        const bool rownear = wrapped || gy < nby;
        const bool rowown = !wrapped && gy >= td.y0 && gy < td.y1;
        const float crow = C01 ? (float)((rmask >> lane) & 1ull) : 0.f;
        if (PSF == 0)
            blk::blur_block(r, u == 0, u == NSX - 1, Rown, Rlf, Rrt, SLOT0, lane, sload8(awx));
        __builtin_amdgcn_sched_barrier(0);
        float yexx = 0.f;  // Y[gy, -1] (u == 0)
        blk::fwd_chain(r, u == 0, u == NSX - 1, Rown, Rlf, Rrt, SLOT1, SLOT0, lane, sload8(awx + 16), yexx);
        __builtin_amdgcn_sched_barrier(0);
        // ---- near band (windows on the top / left image edge): descriptors, strips of Y, the listed sums, strips of G
        const __amdgpu_buffer_rsrc_t rsNe = fused::plane_rsrc(tb.nent, (size_t)da.ngrp * tb.ntabs * NN_PAD);
        const int tab0 = max(td.ntab, 0) * NN_PAD;
        if (nn > 0) {  // window-uniform
            const __amdgpu_buffer_rsrc_t rsNr = fused::plane_rsrc(tb.nrec + tab0, (size_t)nn);
            const __amdgpu_buffer_rsrc_t rsMn = fused::plane_rsrc(tb.Mn + ((size_t)b * tb.ntabs) * NN_PAD + tab0, (size_t)nn);
            uint2 nr[NPT], ne[NPT];
            float2 nm[NPT];
#pragma unroll
            for (int i = 0; i < NPT; i++) {
                const int t8 = (tid + i * NTHR) * 8;
                nr[i] = ld_u2(rsNr, t8), ne[i] = ld_u2(rsNe, tab0 * 8 + t8);
                const uint2 m = ld_u2(rsMn, t8);
                nm[i] = make_float2(__uint_as_float(m.x), __uint_as_float(m.y));
            }
            // (the top strip takes row nby too: the first left-band row, whose own Y sample lives there)
            patch::near_put_y(r, yexx, wrapped || (s == 0 && lane <= nby), left && u == 0, gy + exy, u, exx, nbx, Yt, Yl);
            __syncthreads();
#pragma unroll
            for (int i = 0; i < NPT; i++) {
                const int t = tid + i * NTHR;
                if (t < nn)  // (its counted-sample count is zero where another window owns the pixel: patch::k_near_tab)
                    patch::near_px(nr[i], ne[i], nm[i].x, nm[i].y, Ystrip, Gstrip, [&](int g) { return ld_u2(rsNe, ((g * tb.ntabs) * NN_PAD + tab0 + t) * 8); }, sq);
            }
            __syncthreads();
        }
        // ---- the LR mosaic of the G step
        const __amdgpu_buffer_rsrc_t rsM8 = fused::plane_rsrc(tb.Mt8 + (size_t)b * (W / 4) * H, (size_t)(W / 4) * H);
        const int vrow = lane * 16;
        unsigned m8w[16];
        if (m8) {
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rsM8, vrow, m8l + q * H * 16, 0);
                m8w[4 * q] = v.x, m8w[4 * q + 1] = v.y, m8w[4 * q + 2] = v.z, m8w[4 * q + 3] = v.w;
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        // ---- G = M - C Y on the window; near-band pixels take their value from the strips
        float gexx = 0.f;  // G[gy, -1]
        {
            const __amdgpu_buffer_rsrc_t rsM = fused::plane_rsrc(tb.Mt + (size_t)b * plane, plane);
            const __amdgpu_buffer_rsrc_t rsC = fused::plane_rsrc(tb.Ct, plane);
            float sqg[4] = {0.f, 0.f, 0.f, 0.f};  // by 16-column group: ownership boundaries are multiples of 16
            unsigned long long cm = cmask;
            asm volatile("" : "+s"(cm));
            float gn[3] = {0.f, 0.f, 0.f};
            // The operands arrive EIGHT columns at a time, one batch in flight behind the one being used.  Every batch's address passes through
            // an asm that also takes the last G value of the batch before (and clobbers memory): these loads are pure reads whose addresses do
            // not depend on the data, and left alone the compiler issues all 64 columns' worth above the loop (64 - 128 registers in flight beside
            // the plane: round 3's <false, 4> form spilled 246 registers, 456 bytes of scratch per lane).
            float dep = 0.f;
            constexpr int NB = (NSX == 4 || !C01) ? 4 : 8;  // (the 16-wave window has 128 registers per lane, the 12-wave one 168; a count plane is a second operand)
            auto fetch = [&](const __amdgpu_buffer_rsrc_t &rs, int j0, float(&v)[NB]) {
                int off = tbl;
                asm volatile("" : "+s"(off), "+v"(dep)::"memory");
#pragma unroll
                for (int q = 0; q < NB / 4; q++)
                    ld4(rs, vrow, off + ((j0 >> 2) + q) * H * 16, v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
            };
            if (m8) {
                float cqa[NB], cqb[NB];
                if (!C01)
                    fetch(rsC, 0, cqa);
#pragma unroll
                for (int j0 = 0; j0 < 64; j0 += NB) {
                    float(&cq)[NB] = (j0 & NB) ? cqb : cqa;
                    float(&cn)[NB] = (j0 & NB) ? cqa : cqb;
                    if (!C01 && j0 + NB < 64)
                        fetch(rsC, j0 + NB, cn);
#pragma unroll
                    for (int jj = 0; jj < NB; jj++) {
                        const int j = j0 + jj;
                        const float mv = (float)((m8w[j >> 2] >> (8 * (j & 3))) & 255u);
                        float g, w;
                        if (C01) {
                            const bool on = (cm >> j) & 1ull;
                            g = on ? fmaf(-crow, r[j], mv) : 0.f;
                            w = 1.f;
                        } else {
                            const float cv = cq[jj];
                            g = fmaf(-cv, r[j], mv);
                            w = mosaic::rcp_count(cv);
                        }
                        const float g2 = g * g * w;
                        sqg[j >> 4] += g2;
                        if (j < 3)
                            gn[j] = g2;
                        r[j] = g;
                    }
                    if (!C01) {
                        // (an opaque use of the batch's results: left alone their arithmetic is SUNK below the loop, to where G is first read,
                        // and every batch's operands stay live until then)
#pragma unroll
                        for (int jj = 0; jj < NB; jj++)
                            asm volatile("" : "+v"(r[j0 + jj]));
                        dep = r[j0 + NB - 1];
                        __builtin_amdgcn_sched_barrier(0);  // (... and in front of the next batch's loads)
                    }
                }
            } else {
                float mva[NB], mvb[NB], cva[NB], cvb[NB];
                fetch(rsM, 0, mva);
                if (!C01)
                    fetch(rsC, 0, cva);
#pragma unroll
                for (int j0 = 0; j0 < 64; j0 += NB) {
                    float(&mv)[NB] = (j0 & NB) ? mvb : mva;
                    float(&mn)[NB] = (j0 & NB) ? mva : mvb;
                    float(&cv)[NB] = (j0 & NB) ? cvb : cva;
                    float(&cn)[NB] = (j0 & NB) ? cva : cvb;
                    if (j0 + NB < 64) {
                        fetch(rsM, j0 + NB, mn);
                        if (!C01)
                            fetch(rsC, j0 + NB, cn);
                    }
#pragma unroll
                    for (int jj = 0; jj < NB; jj++) {
                        const int j = j0 + jj;
                        const float c = C01 ? (((cm >> j) & 1ull) ? crow : 0.f) : cv[jj];
                        const float g = fmaf(-c, r[j], mv[jj]);
                        const float g2 = g * g * (C01 ? 1.f : mosaic::rcp_count(c));
                        sqg[j >> 4] += g2;
                        if (j < 3)
                            gn[j] = g2;
                        r[j] = g;
                    }
#pragma unroll
                    for (int jj = 0; jj < NB; jj++)
                        asm volatile("" : "+v"(r[j0 + jj]));
                    dep = r[j0 + NB - 1];
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            if (u == 0)  // the first nbx columns of a left window are near band: not part of the far-field sum
                sqg[0] -= (nbx > 0 ? gn[0] : 0.f) + (nbx > 1 ? gn[1] : 0.f) + (nbx > 2 ? gn[2] : 0.f);
            float sqf = 0.f;
#pragma unroll
            for (int g = 0; g < 4; g++) {
                const int c = 64 * u + 16 * g;
                sqf += (c >= td.x0 && c < td.x1) ? sqg[g] : 0.f;
            }
            sq += (rownear || !rowown) ? 0.f : sqf;
            // near-band rows / columns take G from the strips.  Behind WAVE-UNIFORM guards (only waves of the window's first block row,
            // or the one holding the wrapped row, can have such rows), eight columns at a time: as one divergent branch over all 64
            // columns the compiler turned it into 64 selects with every strip value in flight (38 spilled registers)
            if ((top && s == 0) || (exy && s == 3)) {
                const float *src = Gt + (rownear ? gy + exy : 0) * YW + 64 * u + exx;
#pragma unroll
                for (int j0 = 0; j0 < 64; j0 += 8) {
                    float v[8];
                    // (an opaque offset that also takes the batch before's last value, and a memory clobber: these LDS reads depend on
                    // nothing, and left alone all 64 are issued up front -- 64 registers beside the plane's 64, in a 128-register kernel)
                    int o = j0;
                    asm volatile("" : "+v"(o), "+v"(r[j0 > 0 ? j0 - 1 : 0])::"memory");
#pragma unroll
                    for (int j = 0; j < 8; j++)
                        v[j] = src[o + j];
#pragma unroll
                    for (int j = 0; j < 8; j++) {
                        r[j0 + j] = rownear ? v[j] : r[j0 + j];
                        asm volatile("" : "+v"(r[j0 + j]));
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
                if (u == 0 && exx && rownear)
                    gexx = src[-1];
            }
            if (left && u == 0 && !rownear)
                patch::near_get_g_left(r, gexx, Gl, gy - nby, exx, nbx);
        }
        if (epart) {
            const double ws = wave_sum((double)sq);
            if (lane == 0)
                part[wave] = ws;
        }
        __builtin_amdgcn_sched_barrier(0);
        // ---- H-bwd
        {
            blk::gnbr_put(r, Rown, SLOT1, lane);
            __syncthreads();
            if (epart && tid == 0) {
                double t = 0.0;
#pragma unroll
                for (int i = 0; i < NW; i++)
                    t += part[i];
                epart[(size_t)b * gridDim.x + wid] = t;
            }
            const float gtop = exx ? gexx : r[0];
            const blk::GNbr<float> nbr = blk::gnbr_get(u == 0, u == NSX - 1, Rlf, Rrt, SLOT1, lane, gtop);
            float hlo[3], hhi[3];  // (unused here: the adjoint 7 x 7 runs once, in stage C)
            blk::bwd_chain_x<PSF == 0>(r, a, u == 0, u == NSX - 1, Rown, Rlf, Rrt, SLOT0 + 384, SLOT0, lane, sload8(awx + 16), sload8(awx + 8), nbr.gm1, nbr.gp1, nbr.gp2, gtop,
                                         [](int) {}, [](int, float v) { return v; }, hlo, hhi);
        }
        __builtin_amdgcn_sched_barrier(0);
        __syncthreads();  // every wave has read its neighbours' slots before the transposes overwrite them
        __builtin_amdgcn_sched_barrier(0);
        blk::transpose64(a, r, Rown, lane);
        __builtin_amdgcn_sched_barrier(0);
    }
    {  // ================= stage C: column layout again, r[i] = row 64 s + i (row 63 of s == 3: the wrapped row -1) =================
        SRX_DT_LOCALS();
        float hv[16], hw[16];  // the old state, 16 rows at a time
        if (exy && s == 3) {
            rowbuf[64 * u + lane] = r[63];
            r[63] = 0.f;
        }
        blk::gnbr_put(r, Rown, SLOT0, lane);
        __syncthreads();
        const float gtop = exy ? rowbuf[64 * u + lane] : r[0];
        const blk::GNbr<float> nbr = blk::gnbr_get(s == 0, s == 3, Rup, Rdn, SLOT0, lane, gtop);
        // The old state in 16-row batches, two in flight: batch q is consumed by quarter q of the blur.  Every batch's address passes
        // through an asm that also takes the last value the previous quarter produced (and clobbers memory): without that dependency
        // the loads -- pure reads -- are hoisted above the whole chain, all 64 rows at once, and the chain runs on spilled registers
        float dep = 0.f;
        auto mid = [&](int q) {
                             auto load16 = [&](float(&ld)[16], int bq) {
                                 int so = sq0;
                                 asm volatile("" : "+s"(so), "+v"(dep)::"memory");
#pragma unroll
                                 for (int k = 0; k < 4; k++)
                                     ld4(rs_src, vcol, so + (4 * bq + k) * W * 16, ld[4 * k], ld[4 * k + 1], ld[4 * k + 2], ld[4 * k + 3]);
                             };
                             if (q == 0)
                                 load16(hv, 0), load16(hw, 1);
                             if (q == 1)
                                 load16(hv, 2);
                             else if (q == 2)
                                 load16(hw, 3);
                         };
        auto post = [&](int i, float corr) {
                             const float v = __builtin_amdgcn_fmed3f(fmaf(corr, sn, ((i >> 4) & 1) ? hw[i & 15] : hv[i & 15]), 0.f, 255.f);
                             if ((i & 15) == 15)
                                 dep = v;
                             return v;
                         };
        if (PSF == 0) {
            blk::bwd_chain(r, a, s == 0, s == 3, Rown, Rup, Rdn, SLOT1 + 384, SLOT1, lane, sload8(awy + 16), sload8(awy + 8), nbr.gm1, nbr.gp1, nbr.gp2, gtop, mid, post);
        } else {
            float hl[3], hr[3];
            blk::bwd_chain_x<false>(r, a, s == 0, s == 3, Rown, Rup, Rdn, SLOT1 + 384, SLOT1, lane, sload8(awy + 16), sload8(awy + 8), nbr.gm1, nbr.gp1, nbr.gp2, gtop,
                                      [](int) {}, [](int, float v) { return v; }, hl, hr);
            blk::blur2d_cols<PSF == 2 ? 2 : 3>(a, hl, hr, u == 0, u == NSX - 1, Rown, Rlf, Rrt, lane, tb.k2 + 56, mid, post);
        }
        __builtin_amdgcn_sched_barrier(0);
        // ---- store what this window owns: whole row quads (wave-uniform), the lane's column or nothing
        const int cc = 64 * u + lane;
        const int vst = (cc >= td.x0 && cc < td.x1) ? vcol : 0x7ffffff0;  // beyond the buffer's range: dropped
#pragma unroll
        for (int q = 0; q < 16; q++) {
            const int rw = 64 * s + 4 * q;
            if (rw >= td.y0 && rw < td.y1)
                st4(rs_dst, vst, sql + q * W * 16, a[4 * q], a[4 * q + 1], a[4 * q + 2], a[4 * q + 3]);
        }
    }
#undef SRX_DT_LOCALS
}

// The byte form of the mosaic (items whose samples are 8-bit integers: the sensor's format) and the float form are two instantiations
// of the body behind one workgroup-uniform branch at the very top: ONE launch per iteration.  (k_ibp_patch launches the two forms one
// after the other and lets the blocks of the wrong one leave; per iteration that is a second launch of a full grid of workgroups --
// 4.8 us + a gap on a 74 us kernel, C3-f4.  As a branch INSIDE the iteration the two G steps cost 40 spilled registers, srx_patch.hpp;
// two whole bodies do not share a live range.)
template <bool C01, int NSX, int PSF = 0>
__global__ void __launch_bounds__(256 * NSX)
    k_ibp_dtile(const float *__restrict__ hr_src, float *__restrict__ hr_dst, DTabs tb, DArgs da, double *__restrict__ epart,
                const double *__restrict__ eprev, const double *__restrict__ Vtot, double scale, double *__restrict__ err_prev, int err_stride)
{
    __shared__ __attribute__((aligned(16))) float lds[Lds<NSX>::WORDS];
    if (__builtin_amdgcn_readfirstlane(tb.m8[blockIdx.y]) != 0)
        dtile_body<C01, true, NSX, PSF>(lds, hr_src, hr_dst, tb, da, epart, eprev, Vtot, scale, err_prev, err_stride);
    else
        dtile_body<C01, false, NSX, PSF>(lds, hr_src, hr_dst, tb, da, epart, eprev, Vtot, scale, err_prev, err_stride);
}

// ---- host ----------------------------------------------------------------------------------------------------------
// the counts the workspace layout depends on
struct Dims {
    size_t B, H, W, ntabs, ntiles, ngrp;
};
// what a call carves, in this order; DTabs is its read-only view for the kernel
struct Carved {
    float *s0, *s1, *Mt;  // s0, s1: the two state planes
    unsigned *Mt8;
    int *m8;
    float *Ct;
    AxisW *aw;
    TileD *tiles;
    unsigned long long *rowm, *colm;
    int *nnt;
    uint2 *nrec, *nent;
    float2 *Mn;
    double *ep0, *ep1;    // per-window MSE partials, alternating
    float *k2;
};
// the layout: on the call's arena it is the carve, on a counting one the size (a braced list is evaluated left to right)
static Carved carve(Arena &ar, const Dims &d)
{
    const size_t plane = d.H * d.W;
    return {ar.take<float>(d.B * plane), ar.take<float>(d.B * plane), ar.take<float>(d.B * plane), ar.take<unsigned>(d.B * (d.W / 4) * d.H),
            ar.take<int>(d.B), ar.take<float>(plane), ar.take<AxisW>(2), ar.take<TileD>(d.ntiles), ar.take<unsigned long long>(64 * 4),
            ar.take<unsigned long long>(64 * 4), ar.take<int>(d.ntabs), ar.take<uint2>(d.ntabs * NN_PAD), ar.take<uint2>(d.ngrp * d.ntabs * NN_PAD),
            ar.take<float2>(d.B * d.ntabs * NN_PAD), ar.take<double>(d.B * d.ntiles), ar.take<double>(d.B * d.ntiles), ar.take<float>(112)};
}
static inline size_t tabs_bytes(const IbpShape &s, int B)
{
    return measured([&](Arena &m) { carve(m, Dims{(size_t)B, (size_t)s.H, (size_t)s.W, MAX_TABS, MAX_TILES, ((size_t)s.N + 3) / 4}); });
}

// windows and 0/1 count masks, built on the device from the two axis plans (by-value arguments: no host buffer, no copy)
struct FrameN {
    int n[SRX_MAX_FRAMES];
};
// grid ceil(max(tiles, 64 * (ty.n + tx.n) * 4) / 256): a thread per window, and a thread per mask BIT (a ballot assembles the word)
__global__ void __launch_bounds__(256)
    k_dtile_setup(AxisTiles ty, AxisTiles tx, FrameN ny, FrameN nx, int N, int f, int H, int W, int nsx, TileD *__restrict__ tiles,
                  unsigned long long *__restrict__ rowm, unsigned long long *__restrict__ colm)
{
    const int tid = blockIdx.x * 256 + threadIdx.x;
    for (int i = tid; i < ty.n * tx.n; i += gridDim.x * 256) {
        const int y = i / tx.n, x = i - y * tx.n;
        TileD t;
        t.oy = ty.o[y], t.ox = tx.o[x];
        t.y0 = ty.a[y] - t.oy, t.y1 = ty.a[y + 1] - t.oy, t.x0 = tx.a[x] - t.ox, t.x1 = tx.a[x + 1] - t.ox;
        t.flags = (y == 0 ? 1 : 0) | (x == 0 ? 2 : 0) | y << 8 | x << 20;
        t.ntab = y == 0 ? x : (x == 0 ? tx.n + y - 1 : -1);
        tiles[i] = t;
    }
    // C[gy, gx] = ry[gy] rx[gx] of a full phase grid (srx_patch.hpp, c01_masks), on the windows' own rows / columns: wave i / 64 owns
    // mask word i / 64, lane = bit
    {
        const int q0 = tid >> 6, e = tid & 63;
        if (q0 < (ty.n + tx.n) * 4) {
            const bool isy = q0 < ty.n * 4;
            const int q = isy ? q0 : q0 - ty.n * 4, t = q >> 2, w = q & 3, L = isy ? H : W, nblk = isy ? 4 : nsx;
            const int g = (isy ? ty.o[t] : tx.o[t]) + 64 * w + e;
            bool on = false;
            for (int k = 0; k < N && w < nblk; k++) {
                const int uu = g + (isy ? ny.n[k] : nx.n[k]);
                on = on || (uu >= 0 && uu <= L - 1 && uu % f == 0);
            }
            const unsigned long long m = __ballot(on);
            if (e == 0)
                (isy ? rowm : colm)[q] = m;
        }
    }
}

static int iterate(const mosaic::Common<float> &c, const float *hr_init, float *hr, int n_iter, double *errors, Arena &ar, hipStream_t st)
{
    const int B = c.B, N = c.N, f = c.f, H = c.H, W = c.W, NS = c.NS;
    const mosaic::AxisPlan &py = c.py, &px = c.px;
    const double *Vtot = c.Vtot;
    const double scale = c.scale;
    Plan pl;
    if (!plan(H, W, c.flags, pl))
        return SRX_E_UNSUPPORTED;
    const int ntiles = pl.ty.n * pl.tx.n, RX = 64 * pl.nsx, ngrp = NS / 4, ntabs = pl.tx.n + pl.ty.n - 1;
    const auto [s0, s1, Mt, Mt8, m8, Ct, aw, tiles, rowm, colm, nnt, nrec, nent, Mn, ep0, ep1, k2] =
        carve(ar, Dims{(size_t)B, (size_t)H, (size_t)W, (size_t)ntabs, (size_t)ntiles, (size_t)ngrp});
    if (!ar.ok)
        return SRX_E_WORKSPACE;
    const int psf = fused::psf_form(c.kc, c.kt);
    if (psf != 0) {
        if (pl.nsx != 3 || psf == 3)  // (eligible() keeps full 7 x 7 support on the tile kernels)
            return SRX_E_UNSUPPORTED;
        SRX_TRY(patch::upload_k2(c.kc, c.kt, k2, st));
    }
    DArgs da;
    da.H = H, da.W = W, da.tiles_x = pl.tx.n, da.tiles_y = pl.ty.n;
    patch::AxisWPair awp;
    patch::fill_axis(py, c.kc.cy, c.kt.cy, da.y, awp.y);
    patch::fill_axis(px, c.kc.cx, c.kt.cx, da.x, awp.x);
    da.sn = (float)c.step / (float)N;
    da.ngrp = ngrp;
    unsigned long long d0[4], d1[4];
    da.c01 = patch::c01_masks(py, px, N, f, d0, d1) ? 1 : 0;  // (its masks are a 256-pixel image's: only the verdict is used here)
    FrameN fy, fx;
    for (int q = 0; q < SRX_MAX_FRAMES; q++)
        fy.n[q] = q < N ? py.n[q] : 0, fx.n[q] = q < N ? px.n[q] : 0;
    hipLaunchKernelGGL(k_dtile_setup, dim3(cdiv(std::max(ntiles, 64 * (pl.ty.n + pl.tx.n) * 4), 256)), dim3(256), 0, st, pl.ty, pl.tx, fy, fx, N, f, H, W,
                       pl.nsx, tiles, rowm, colm);
    SRX_CHECK_LAUNCH();
    SRX_TRY(upload_record(st, aw, awp));
    // ---- operand planes, near-band tables, state
    // (every table is launched at the lists' capacity: the windows differ in their pixel counts, which the table kernel writes to nnt)
    SRX_TRY((patch::block_setup<float, float2>(c, pl.ty, pl.tx, RY, RX, da.y, da.x, NN_PAD / 256, Mt, Ct, Mt8, m8, nnt, nrec, nent, Mn, st)));
    hipLaunchKernelGGL(k_dtile_copy_in, dim3(cdiv(W, 256), H / 4, B), dim3(256), 0, st, hr_init, H, W, s0);
    SRX_CHECK_LAUNCH();
    DTabs tb{Mt, Mt8, m8, Ct, aw, tiles, rowm, colm, nnt, nrec, nent, Mn, ntabs, k2};
    const dim3 grid(ntiles, B);
    const bool c01 = da.c01 != 0, want = errors != nullptr;
    const auto kern = pl.nsx == 4 ? (c01 ? k_ibp_dtile<true, 4> : k_ibp_dtile<false, 4>)
                      : psf == 2  ? (c01 ? k_ibp_dtile<true, 3, 2> : k_ibp_dtile<false, 3, 2>)
                                  : (c01 ? k_ibp_dtile<true, 3> : k_ibp_dtile<false, 3>);
    PingPong<float> pp = {s0, s1, ep0, ep1, 0};
    for (int j = 0; j < n_iter; j++, pp.advance())
        SRX_LAUNCH(KID_IBP_DTILE, kern, grid, dim3(256 * pl.nsx), 0, st, pp.src(), pp.dst(), tb, da, pp.ep(j, want), pp.eprev(j, want), Vtot, scale,
                   pp.err_prev(errors, j), n_iter);
    if (want) {
        if (pl.nsx == 4)
            hipLaunchKernelGGL(k_dtile_trace<1024>, dim3(B), dim3(1024), 0, st, pp.last_ep(n_iter), ntiles, Vtot, scale, errors + n_iter - 1, n_iter);
        else
            hipLaunchKernelGGL(k_dtile_trace<768>, dim3(B), dim3(768), 0, st, pp.last_ep(n_iter), ntiles, Vtot, scale, errors + n_iter - 1, n_iter);
        SRX_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(k_dtile_copy_out, dim3(cdiv(W, 256), H / 4, B), dim3(256), 0, st, pp.cur(), H, W, hr);
    SRX_CHECK_LAUNCH();
    return SRX_OK;
}

}  // namespace dtile
}  // namespace srx
