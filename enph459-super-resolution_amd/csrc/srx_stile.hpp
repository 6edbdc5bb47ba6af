// srx_stile.hpp -- float64 on 256 x 256 patches with a common fraction > 0: one IBP iteration as TWO launches on register-resident STRIPS.
//
// The reference computes in float64 (mono_cal_target/run_sr.py:74) and the headline workload (C2: 64 x 64 LR -> 256 x 256 HR, x4, all 16
// phases) has a common fraction 1/2 -- the spline prefilter is a recursion over whole rows and columns.  srx_patch.hpp keeps a float32
// patch in the registers of ONE compute unit; a float64 patch is 512 KB, the whole register file of a compute unit, so that kernel has no
// float64 form and the float64 call ran on the tile kernels of srx_mosaic.hpp (R = 23 warm-up halos on 89 x 89 regions: 5.8x recompute,
// three launches, 0.062 of the HBM roofline for three rounds).  What does fit: a STRIP of the patch that spans it in the direction the
// operators run --
//
//   k_ibp_sv  "vertical":   a workgroup of 4 waves owns 256 rows x 64 columns (lane = column, 64 registers = rows of the wave's block, the
//                           four blocks stacked).  Every vertical operator of srx_patch.hpp's stages C and A runs on it with NO halo (the
//                           strip is the whole column; the blocks exchange carries through LDS): V-FIR' + prefilter, V-blur', the update
//                           hr <- clip(hr + step v / N), then V-blur, V-prefilter + FIR of the NEXT iteration.
//   k_ibp_sh  "horizontal": 64 rows x 256 columns (lane = row, registers = columns, four blocks side by side): stage B -- H-blur,
//                           H-prefilter + FIR = Y, the near band, G = M - C Y, the MSE sum, H-FIR' + prefilter, H-blur'.
//
// Between the two ONE plane per patch crosses memory once each way (8 B per pixel and direction), row-major, in place: k_ibp_sv reads and
// writes its columns of it as they are (lane = column), k_ibp_sh transposes its rows in and out (srx_block.hpp's wave-private transpose64
// on the low and the high words).  Per HR pixel and iteration: sv reads G' 8 + hr 8, writes hr 8 + Yv 8; sh reads Yv 8 + M 1 (bytes) or
// 8, writes G' 8 = 49 B against the algorithmic 24 (SURVEY 8d in float64) -- where the tile kernels moved ~150.  Measured (C2, B = 1024):
// both kernels run at the memory's pace (sv 2.15 GB in ~340 us, sh 1.14 GB in ~290), VALU time is a fifth of it.
// The closed forms of SciPy's 12-sample pad and the carry fix-ups between blocks (z^(i+1) * carry over the first FIX samples; FIX = 28 in
// float64: |z|^29 = 3e-17) are srx_block.hpp's, the source k_ibp_patch instantiates in float; the near band is srx_patch.hpp's, tables and
// kernel code (patch::near_put_y, near_px, near_get_g in double; the tables and the operand planes from patch::block_setup in T).  Row -1 of Y / G (frames with n_k > 0) rides as plane row 0:
// the planes between the kernels hold row q = gy + ex (the last grid row is empty then, srx_patch.hpp's axis_ok).
#pragma once
#include "srx_patch.hpp"

namespace srx {
namespace stile {

using patch::NN_PAD;
using patch::PN;
using blk::RW;
using patch::YW;

template <typename T> __device__ __forceinline__ T clip255(T v) { return v < (T)0 ? (T)0 : (v > (T)255 ? (T)255 : v); }

// exchange slots of a wave's private LDS region, in units of T (the region is RW floats = RW / 2 doubles)
constexpr int S0 = 0, S1 = 512;
static_assert(S1 + 448 <= RW / 2, "slots inside the wave's region");

template <typename T> struct AxW {  // filter weights of one axis (kernel argument: scalar registers)
    T kb[7];  // forward blur (correlation) weights times kq = -6 z
    T kt[7];  // backward blur (flipped kernel)
    T wf[4];  // forward FIR
    T wb[4];  // backward FIR times kq
};
template <typename T> struct T2 {
    T x, y;
};

// ---- eligibility: srx_patch.hpp's, for 8-byte elements -------------------------------------------------------------------------------
static inline bool shape_admits(const IbpShape &s) { return s.eb == 8 && s.H == PN && s.W == PN; }

static inline bool eligible(const IbpSpec &s)
{
    if (!shape_admits(s) || (s.flags & SRX_FLAG_TILES))
        return false;
    IbpSpec s4 = s;  // the patch path's conditions, which are stated for its own 4-byte elements
    s4.eb = 4;
    return patch::eligible(s4, true);  // rank-1 PSFs only (rank 1 is decided on the float64 weights there too)
}

// (once per call: the patch path's operand planes and near-band tables in T -- patch::block_setup<T, T2<T>>)

template <typename T> struct STabs {
    const T *Mt;           // [B][64 column quads][256 gy][4]
    const unsigned *Mt8;   // [B][16][256 gy][4] words of four byte columns
    const int *m8;         // [B]
    const T *Ct;           // [64][256][4]
    const uint2 *nrec;     // srx_patch.hpp's near-band descriptors
    const uint2 *nent;
    const T2<T> *Mn;       // [B][NN_PAD]
};

// LDS of k_ibp_sh behind the four waves' regions, in units of T: the near-band strips in srx_patch.hpp's geometry
constexpr int OFF_YT = 0, OFF_YL = 4 * YW, OFF_GT = 8 * YW, OFF_GL = 11 * YW, STRIP_T = 14 * YW;

// =====================================================================================================================================
// k_ibp_sv: grid (4 column strips, B), block 256.  mode bit 0: first launch of a call (no correction yet: read hr_in, forward half only),
// bit 1: last launch (backward half and update only).  it_done: the iteration whose G' this launch consumes (its MSE partials are summed
// here, by one thread of strip 0, in a fixed order).
// =====================================================================================================================================
template <typename T>
__global__ void __launch_bounds__(256, 2)
    k_ibp_sv(const T *__restrict__ hr_in, T *__restrict__ hr, T *P, const AxW<T> aw, int exy, T sn, int mode,
             const double *__restrict__ epart, const double *__restrict__ Vtot, double scale, double *__restrict__ errors, int n_iter, int it_done)
{
    __shared__ __attribute__((aligned(16))) float lds[4 * RW];
    const int tid = threadIdx.x, lane = tid & 63;
    const int s = __builtin_amdgcn_readfirstlane(tid >> 6), u = blockIdx.x, b = blockIdx.y;
    T *Rown = reinterpret_cast<T *>(lds + s * RW);
    const T *Rup = reinterpret_cast<const T *>(lds + (s - 1) * RW), *Rdn = reinterpret_cast<const T *>(lds + (s + 1) * RW);
    constexpr int EB = (int)sizeof(T);
    const __amdgpu_buffer_rsrc_t rs_hr = fused::plane_rsrc(hr + (size_t)b * PN * PN, (size_t)PN * PN);
    const int colb = (64 * u + lane) * EB, rowb = 64 * s * PN * EB;  // row-major planes: lane = column
    T a[64];
    if (mode & 1) {
        const __amdgpu_buffer_rsrc_t rs_in = fused::plane_rsrc(hr_in + (size_t)b * PN * PN, (size_t)PN * PN);
#pragma unroll
        for (int i = 0; i < 64; i++)
            a[i] = fused::buf_load<T>(rs_in, colb, rowb + i * PN * EB);
        if (hr_in != hr) {
#pragma unroll
            for (int i = 0; i < 64; i++)
                fused::buf_store<T>(a[i], rs_hr, colb, rowb + i * PN * EB);
        }
    } else {
        if (errors && u == 0 && tid == 0)
            errors[(size_t)b * n_iter + it_done] = (((epart[4 * b] + epart[4 * b + 1]) + (epart[4 * b + 2] + epart[4 * b + 3])) + Vtot[b]) * scale;
        // G' arrives in the plane this launch writes Yv to, row-major, plane row q = gy + exy (row 256 of the last block: out of range, 0 --
        // grid row 255 holds no sample when a frame reaches above the grid (axis_ok), G' = 0 there)
        const __amdgpu_buffer_rsrc_t rs_g = fused::plane_rsrc(P + (size_t)b * PN * PN, (size_t)PN * PN);
#pragma unroll
        for (int i = 0; i < 64; i++)
            a[i] = fused::buf_load<T>(rs_g, colb, rowb + (i + exy) * PN * EB);
        const T gtop = exy ? (s == 0 ? fused::buf_load<T>(rs_g, colb, 0) : (T)0) : a[0];
        blk::gnbr_put(a, Rown, S0, lane);
        __syncthreads();
        const blk::GNbr<T> nbr = blk::gnbr_get(s == 0, s == 3, Rup, Rdn, S0, lane, gtop);
        // V-bwd: srx_block.hpp's backward chain -- its front half, then the blur' in place with the update as its epilogue
        T hl[3], hr[3];
        blk::bwd_front(a, s == 0, s == 3, Rown, Rup, Rdn, S1 + 384, S1, lane, aw.wb, nbr.gm1, nbr.gp1, nbr.gp2, gtop, hl, hr);
        T hv[2][8];  // the state's rows, a group ahead of the blur that consumes them
        auto load8 = [&](T(&d)[8], int j0) {
#pragma unroll
            for (int j = 0; j < 8; j++)
                d[j] = fused::buf_load<T>(rs_hr, colb, rowb + (j0 + j) * PN * EB);
        };
        blk::blur_inplace(
            a, hl, hr, aw.kt,
            [&](int j0) {
                if (j0 == 0)
                    load8(hv[0], 0);
                if (j0 + 8 < 64)
                    load8(hv[((j0 >> 3) + 1) & 1], j0 + 8);
            },
            [&](int i, T corr) { return clip255(fma(corr, sn, hv[(i >> 3) & 1][i & 7])); });
#pragma unroll
        for (int i = 0; i < 64; i++)
            fused::buf_store<T>(a[i], rs_hr, colb, rowb + i * PN * EB);
        if (mode & 2)
            return;
    }
    blk::blur_block(a, s == 0, s == 3, Rown, Rup, Rdn, S0, lane, aw.kb);
    T yex = 0;
    blk::fwd_chain(a, s == 0, s == 3, Rown, Rup, Rdn, S1, S0, lane, aw.wf, yex);
    const __amdgpu_buffer_rsrc_t rs_y = fused::plane_rsrc(P + (size_t)b * PN * PN, (size_t)PN * PN);
#pragma unroll
    for (int i = 0; i < 64; i++)
        if (!(exy && s == 3 && i == 63))
            fused::buf_store<T>(a[i], rs_y, colb, rowb + (i + exy) * PN * EB);
    if (exy && s == 0)
        fused::buf_store<T>(yex, rs_y, colb, 0);
}

// =====================================================================================================================================
// k_ibp_sh: grid (4 row strips, B), block 256.  Lane = plane row q = 64 strip + lane (natural row gy = q - exy), wave u = columns 64 u ...
// =====================================================================================================================================
// The LR mosaic as bytes when every far-field sample of the patch is an integer in [0, 255] (k_block_prep's flag), else as T: two instantiations of
// the body behind ONE workgroup-uniform branch at the very top of the kernel (k_ibp_dtile's arrangement: two whole bodies share no live range).
// As a run-time choice inside one body -- even per group of eight columns, feeding the same arithmetic -- the allocator spilled 92 registers where
// either form alone spills 1; as a pair of launches (k_ibp_patch's arrangement) the empty twin cost 4.8 us per chunk and iteration, 5 % of the loop.
template <typename T, bool C01, bool M8>
__device__ __forceinline__ void sh_body(float *lds, T *P, const STabs<T> &tb, const patch::PatchArgs &pa, const AxW<T> &aw, double *__restrict__ epart,
                                        int want_err)
{
    const int tid = threadIdx.x, lane = tid & 63;
    const int u = __builtin_amdgcn_readfirstlane(tid >> 6), s = blockIdx.x, b = blockIdx.y;
    constexpr bool m8 = M8;
    T *Rown = reinterpret_cast<T *>(lds + u * RW);
    const T *Rlf = reinterpret_cast<const T *>(lds + (u - 1) * RW), *Rrt = reinterpret_cast<const T *>(lds + (u + 1) * RW);
    T *strips = reinterpret_cast<T *>(lds + 4 * RW);
    T *Yt = strips + OFF_YT, *Yl = strips + OFF_YL, *Gt = strips + OFF_GT, *Gl = strips + OFF_GL;
    double *part = reinterpret_cast<double *>(lds + 4 * RW + STRIP_T * (sizeof(T) / 4));
    constexpr int EB = (int)sizeof(T);
    const int exy = pa.y.ex, exx = pa.x.ex, nby = pa.y.nb, nbx = pa.x.nb;
    const int q = 64 * s + lane, gy = q - exy;
    const bool rownear = gy < nby;

    T r[64];
    {
        T a[64];
        const __amdgpu_buffer_rsrc_t rs_y = fused::plane_rsrc(P + (size_t)b * PN * PN, (size_t)PN * PN);
        const int colb = (64 * u + lane) * EB;
#pragma unroll
        for (int i = 0; i < 64; i++)
            a[i] = fused::buf_load<T>(rs_y, colb, (64 * s + i) * PN * EB);
        blk::transpose64(a, r, lds + u * RW, lane);
    }
    blk::blur_block(r, u == 0, u == 3, Rown, Rlf, Rrt, S0, lane, aw.kb);
    T yexx = 0;  // Y[gy, -1] (u == 0)
    blk::fwd_chain(r, u == 0, u == 3, Rown, Rlf, Rrt, S1, S0, lane, aw.wf, yexx);
    // ---- requested here, consumed behind the strips' barrier: the byte mosaic of the G step and this thread's near-band descriptors.  This strip's
    // share of srx_patch.hpp's enumeration: the top rows (strip 0 only: at most 3 x 257 pixels, four per thread) and the left columns of its
    // own rows (at most 4 x 64, one per thread).  (As loads inside the near-band loop they were three dependent round trips per pixel and
    // strip 0 took twice as long as its neighbours.)
    unsigned m8w[16];
    if (m8) {
        const __amdgpu_buffer_rsrc_t rsM8 = fused::plane_rsrc(tb.Mt8 + (size_t)b * (PN / 4) * PN, (size_t)(PN / 4) * PN);
#pragma unroll
        for (int g = 0; g < 4; g++) {
            const blk::u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rsM8, ((4 * u + g) * PN + gy) * 16, 0, 0);
            m8w[4 * g] = v.x, m8w[4 * g + 1] = v.y, m8w[4 * g + 2] = v.z, m8w[4 * g + 3] = v.w;
        }
    }
    constexpr int NQ = 5;
    int nt[NQ];
    bool non[NQ];
    uint2 nr[NQ], ne[NQ];
    T2<T> nm[NQ];
    {
        const int LN = exx + nbx, ntop = patch::near_top(PN, exy, exx, nby);
        const int gy_lo = max(nby, 64 * s - exy), gy_hi = min(PN - exy, 64 * s + 64 - exy);
#pragma unroll
        for (int k = 0; k < NQ - 1; k++)
            nt[k] = tid + 256 * k, non[k] = s == 0 && nt[k] < ntop;
        nt[NQ - 1] = ntop + (gy_lo - nby) * LN + tid, non[NQ - 1] = gy_hi > gy_lo && nt[NQ - 1] < ntop + (gy_hi - nby) * LN;
#pragma unroll
        for (int k = 0; k < NQ; k++) {
            nr[k] = ne[k] = make_uint2(0, 0), nm[k] = T2<T>{0, 0};
            if (non[k])
                nr[k] = tb.nrec[nt[k]], ne[k] = tb.nent[nt[k]], nm[k] = tb.Mn[(size_t)b * NN_PAD + nt[k]];
        }
    }
    // ---- near-band strips of Y
    patch::near_put_y(r, yexx, s == 0 && q <= nby + exy, u == 0, q, u, exx, nbx, Yt, Yl);
    __syncthreads();
    // ---- near band: G = M - the listed Y samples; the counted samples' share of the MSE trace
    T sq = 0;
#pragma unroll
    for (int k = 0; k < NQ; k++)
        if (non[k])
            patch::near_px(nr[k], ne[k], nm[k].x, nm[k].y, strips, Gt, [&](int g) { return tb.nent[(size_t)g * NN_PAD + nt[k]]; }, sq);
    __syncthreads();
    // ---- G = M - C Y on the grid; near-band pixels take their value from the strips
    T gexx = 0;  // G[gy, -1]
    {
        T sqf = 0, gn[3] = {0, 0, 0};
        const unsigned long long cm = C01 ? pa.rx[u] : 0ull;
        T crow = 0;
        if (C01) {
            const int gyc = max(gy, 0);
            const unsigned long long rm = (gyc >> 6) == 0 ? pa.ry[0] : (gyc >> 6) == 1 ? pa.ry[1] : (gyc >> 6) == 2 ? pa.ry[2] : pa.ry[3];
            crow = (T)((rm >> (gyc & 63)) & 1ull);
        }
        const __amdgpu_buffer_rsrc_t rsC = fused::plane_rsrc(tb.Ct, (size_t)PN * PN);
        const __amdgpu_buffer_rsrc_t rsM = fused::plane_rsrc(tb.Mt + (size_t)b * PN * PN, (size_t)PN * PN);
        const int tbl = ((16 * u * PN + gy) * 4) * EB;  // (column quad 16 u, row gy) of the transposed planes, bytes
#pragma unroll
        for (int j0 = 0; j0 < 64; j0 += 8) {
            T mv[8], cv[8];
            if (m8) {
#pragma unroll
                for (int j = 0; j < 8; j++)
                    mv[j] = (T)((m8w[(j0 + j) >> 2] >> (8 * ((j0 + j) & 3))) & 255u);
            } else {
#pragma unroll
                for (int j = 0; j < 8; j++)
                    mv[j] = fused::buf_load<T>(rsM, tbl + (((j0 + j) >> 2) * PN * 4 + ((j0 + j) & 3)) * EB, 0);
            }
#pragma unroll
            for (int j = 0; j < 8; j++)
                cv[j] = C01 ? (((cm >> (j0 + j)) & 1ull) ? crow : (T)0) : fused::buf_load<T>(rsC, tbl + (((j0 + j) >> 2) * PN * 4 + ((j0 + j) & 3)) * EB, 0);
#pragma unroll
            for (int j = 0; j < 8; j++) {
                const T g = fma(-cv[j], r[j0 + j], mv[j]);
                const T g2 = g * g * (C01 ? (T)1 : mosaic::rcp_count(cv[j]));
                sqf += g2;
                if (j0 + j < 3)
                    gn[j0 + j] = g2;
                r[j0 + j] = g;
            }
        }
        if (u == 0)
            sqf -= (nbx > 0 ? gn[0] : (T)0) + (nbx > 1 ? gn[1] : (T)0) + (nbx > 2 ? gn[2] : (T)0);
        sq += rownear ? (T)0 : sqf;
        patch::near_get_g(r, gexx, rownear, gy, u, exy, exx, nby, nbx, Gt, Gl);
    }
    if (want_err) {
        const double ws = wave_sum((double)sq);
        if (lane == 0)
            part[u] = ws;
    }
    // ---- H-bwd
    blk::gnbr_put(r, Rown, S1, lane);
    __syncthreads();
    if (want_err && tid == 0)
        epart[4 * b + s] = (part[0] + part[1]) + (part[2] + part[3]);
    const T gtop = exx ? gexx : r[0];
    const blk::GNbr<T> nbr = blk::gnbr_get(u == 0, u == 3, Rlf, Rrt, S1, lane, gtop);
    T hl[3], hr[3];
    blk::bwd_front(r, u == 0, u == 3, Rown, Rlf, Rrt, S0 + 384, S0, lane, aw.wb, nbr.gm1, nbr.gp1, nbr.gp2, gtop, hl, hr);
    blk::blur_inplace(r, hl, hr, aw.kt, [](int) {}, [](int, T v) { return v; });
    // back to the plane, over this strip's own rows, row-major (k_ibp_sv reads columns of it): the second transpose
    __syncthreads();  // the neighbours have read this wave's exchange slots, which the transpose runs over
    {
        T a[64];
        blk::transpose64(r, a, lds + u * RW, lane);
        const __amdgpu_buffer_rsrc_t rs_g = fused::plane_rsrc(P + (size_t)b * PN * PN, (size_t)PN * PN);
        const int colb = (64 * u + lane) * EB;
#pragma unroll
        for (int i = 0; i < 64; i++)
            fused::buf_store<T>(a[i], rs_g, colb, (64 * s + i) * PN * EB);
    }
}

template <typename T, bool C01>
__global__ void __launch_bounds__(256, 2)
    k_ibp_sh(T *P, const STabs<T> tb, const patch::PatchArgs pa, const AxW<T> aw, double *__restrict__ epart, int want_err)
{
    __shared__ __attribute__((aligned(16))) float lds[4 * RW + STRIP_T * (sizeof(T) / 4) + 16];
    if (__builtin_amdgcn_readfirstlane(tb.m8[blockIdx.y]) != 0)
        sh_body<T, C01, true>(lds, P, tb, pa, aw, epart, want_err);
    else
        sh_body<T, C01, false>(lds, P, tb, pa, aw, epart, want_err);
}

// ---- host --------------------------------------------------------------------------------------------------------------------------
template <typename T> static inline void fill_axis(const mosaic::AxisPlan &pl, const T *cfwd, const T *cbwd, patch::AxisC &ax, AxW<T> &aw)
{
    const double kq = -6.0 * blk::ZD;
    double wv[4];
    fused::host_weights(1.0 - pl.delta, wv);
    for (int i = 0; i < 4; i++)
        aw.wf[i] = (T)wv[i];
    fused::host_weights(pl.delta, wv);
    for (int i = 0; i < 4; i++)
        aw.wb[i] = (T)(kq * wv[i]);
    for (int i = 0; i < 7; i++)
        aw.kb[i] = (T)(kq * (double)cfwd[i]), aw.kt[i] = cbwd[i];
    ax.ex = pl.nmax, ax.nb = -pl.nmin, ax.E = pl.E;
}

// what a call carves, in this order (the counts are srx_patch.hpp's: the batch and the near band's slot groups)
template <typename T> struct Carved {
    T *Mt, *P;
    unsigned *Mt8;
    int *m8;
    T *Ct;
    uint2 *nrec, *nent;
    T2<T> *Mn;
    double *epart;
};
// the layout: on the call's arena it is the carve, on a counting one the size (a braced list is evaluated left to right)
template <typename T> static Carved<T> carve(Arena &ar, const patch::Dims &d)
{
    return {ar.take<T>(d.B * PN * PN), ar.take<T>(d.B * PN * PN), ar.take<unsigned>(d.B * (PN / 4) * PN), ar.take<int>(d.B), ar.take<T>((size_t)PN * PN),
            ar.take<uint2>(NN_PAD), ar.take<uint2>(d.ngrp * NN_PAD), ar.take<T2<T>>(d.B * NN_PAD), ar.take<double>(d.B * 4)};
}
static inline size_t tabs_bytes(const IbpShape &s, int B)
{
    const patch::Dims d{(size_t)B, ((size_t)s.N + 3) / 4};
    return measured([&](Arena &m) { s.eb == 8 ? (void)carve<double>(m, d) : (void)carve<float>(m, d); });
}

template <typename T>
static int iterate(const mosaic::Common<T> &c, const T *hr_init, T *hr, int n_iter, double *errors, Arena &ar, hipStream_t st)
{
    const int B = c.B, N = c.N, f = c.f, NS = c.NS;
    const mosaic::AxisPlan &py = c.py, &px = c.px;
    const double scale = c.scale;
    const int ngrp = NS / 4;
    const auto [Mt, P, Mt8, m8, Ct, nrec, nent, Mn, epart] = carve<T>(ar, patch::Dims{(size_t)B, (size_t)ngrp});
    if (!ar.ok)
        return SRX_E_WORKSPACE;
    patch::PatchArgs pa;
    AxW<T> awy, awx;
    fill_axis<T>(py, c.kc.cy, c.kt.cy, pa.y, awy);
    fill_axis<T>(px, c.kc.cx, c.kt.cx, pa.x, awx);
    pa.sn = 0.f;
    patch::fill_near(pa);
    pa.ngrp = ngrp;
    if (pa.nn > NN_PAD)
        return SRX_E_UNSUPPORTED;
    pa.c01 = patch::c01_masks(py, px, N, f, pa.ry, pa.rx) ? 1 : 0;
    const patch::AxisTiles one = patch::one_region(PN);
    SRX_TRY((patch::block_setup<T, T2<T>>(c, one, one, PN, PN, pa.y, pa.x, cdiv(pa.nn, 256), Mt, Ct, Mt8, m8, nullptr, nrec, nent, Mn, st)));
    const T sn = (T)(c.step / (double)N);
    const int want = errors ? 1 : 0;
    // The batch in chunks of 128 patches, every launch of a chunk before the next chunk's first: 512 workgroups = one round of the 256
    // compute units at two workgroups each, and the chunk's working set (state, plane, byte mosaic: 1.06 MB per patch) stays in the 256 MB
    // Infinity Cache between a launch and the next (C2, 1024 patches: 63.8 -> 58.1 ms per step; 64: 73, launch-bound; 192 / 256: 59 / 61).
    constexpr int CB = 128;
    for (int c0 = 0; c0 < B; c0 += CB) {
        const int nb = std::min(CB, B - c0);
        const size_t po = (size_t)c0 * PN * PN;
        const STabs<T> tb{Mt + po, Mt8 + (size_t)c0 * (PN / 4) * PN, m8 + c0, Ct, nrec, nent, Mn + (size_t)c0 * NN_PAD};
        double *ep = epart + 4 * c0, *er = errors ? errors + (size_t)c0 * n_iter : nullptr;
        const double *vt = c.Vtot + c0;
        const dim3 grid(4, nb), blk(256);
        SRX_LAUNCH(KID_IBP_SV, (k_ibp_sv<T>), grid, blk, 0, st, hr_init + po, hr + po, P + po, awy, pa.y.ex, sn, 1, ep, vt, scale, er, n_iter, 0);
        for (int it = 0; it < n_iter; it++) {
            if (pa.c01)
                SRX_LAUNCH(KID_IBP_SH, (k_ibp_sh<T, true>), grid, blk, 0, st, P + po, tb, pa, awx, ep, want);
            else
                SRX_LAUNCH(KID_IBP_SH, (k_ibp_sh<T, false>), grid, blk, 0, st, P + po, tb, pa, awx, ep, want);
            SRX_LAUNCH(KID_IBP_SV, (k_ibp_sv<T>), grid, blk, 0, st, hr + po, hr + po, P + po, awy, pa.y.ex, sn, it == n_iter - 1 ? 2 : 0, ep, vt, scale, er,
                       n_iter, it);
        }
    }
    return SRX_OK;
}

}  // namespace stile
}  // namespace srx
