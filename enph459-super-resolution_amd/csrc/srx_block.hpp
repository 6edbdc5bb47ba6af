// srx_block.hpp -- the 64 x 64 register-block primitives every wave-block kernel family is built from (namespace srx::blk).
//
// A wave holds a 64 x 64 block of a plane: lane = column (or row), 64 registers = its rows (columns).  What runs on such a block, alone
// or in a line of blocks that exchange a few words through the waves' private LDS regions, lives here ONCE:
//
//   * transpose64: the wave-private transpose (float; double = two float transposes on the low and the high words);
//   * chain64: the recursion a[i] <- z a[i -+ 1] + a[i] as sub-chains joined by z^(i+1) * carry fix-ups, and add_carry, the same fix-up
//     between the blocks of a line;
//   * fwd_chain / bwd_front: the spline prefilter with its FIR behind / before it over a line of blocks, with the closed forms of SciPy's
//     12-sample edge pad (the steady-state starts, c[i] = z (c[i+1] - S) in the pad, the z^24 reflect end) -- tools/patch_proto.py derives
//     them and checks them against the oracle;
//   * blur_inplace / blur_block: the 7-tap correlation along the registers with a three-sample halo from either neighbour;
//   * bwd_chain_x / bwd_chain: bwd_front + k_ibp_patch's out-of-place blur' in quarters (the float64 strips end theirs with blur_inplace);
//   * halo3_put / halo3_get and gnbr_put / gnbr_get: what a block publishes for its neighbours in front of a 7-tap blur (three samples
//     either side) and in front of a backward chain (G just before, two samples behind), each as two halves around the caller's barrier;
//   * blur2d_pass1 / blur2d_fix, together blur2d_cols: the 7 x 7 Horner blur in column layout; the DPP lane shifts; sload8, st4 / ld4 / ld_u2.
//
// The arithmetic is templated on the element type T: k_ibp_patch, k_ibp_dtile, k_ibp_ztile and the b / a kernels instantiate it in
// float, the float64 strips of srx_stile.hpp in double -- the same source, so a fix reaches both.  What differs by T is stated here and
// nowhere else: the constants are (T) of one double expression each, the carry fix-ups reach FIX = 16 samples in float (|z|^17 = 2e-10)
// and 28 in double (|z|^29 = 3e-17), and the filter weights arrive as whatever the caller holds them in (an f8 of scalar registers, a
// T[4] / T[7] kernel argument): a template parameter indexed [0..3] / [0..6].  LDS slots are in units of T.
// srx_patch.hpp keeps the patch kernel, its tables, its eligibility, its carve and its driver.
#pragma once
#include "srx_common.h"

namespace srx {
namespace blk {

#ifndef SRX_M0_NOP
#define SRX_M0_NOP "s_nop 0\n\t"  // the ISA asks for one wait state between a scalar write of M0 and an LDS add-TID instruction, and inside
                                  // an asm block nobody inserts it.  Without it the first store of a block sometimes went out with the M0 of
                                  // before (round 3: k_ibp_ztile's 7 x 7 form, one row of one wave wrong in 7 of 40 calls, always behind the
                                  // tile that sums the previous iteration's MSE partials; tools/stress_determinism.py, tests/test_gpu_parity.py::
                                  // test_frame_kernel_is_deterministic).  "" reproduces it.
#endif
constexpr int TSD = 68;        // LDS row stride of a half-block transpose (a multiple of 4 words: 16-byte row reads; 17 quads: the 16
                               // lanes the LDS serves together read 16 different quads of banks, conflict-free)
constexpr int RW = 32 * TSD;   // LDS words of a wave's private region
constexpr int SLOT0 = 0, SLOT1 = 1024;  // exchange slots inside the private region (<= 6 x 64 words each)

constexpr double ZD = -0.26794919243112270647;
template <typename T> struct Cn {  // the constants of the recursion in the element type
    static constexpr int FIX = sizeof(T) == 4 ? 16 : 28;  // samples over which a neighbour's carry is added (|z|^17 = 2e-10, |z|^29 = 3e-17)
    static constexpr T Z = (T)ZD;
    static constexpr T K2 = (T)(1.0 / (1.0 - ZD));  // steady state of the causal recursion: q = v' K2
    static constexpr T K1 = (T)(1.0 / ((1.0 - ZD) * (1.0 - ZD)));
    static constexpr T K3 = (T)(ZD / (1.0 - ZD * ZD));
    static constexpr T K4 = (T)(1.0 / (1.0 - ZD * ZD));
};
struct ZPow {
    double v[Cn<double>::FIX];
    constexpr ZPow() : v()
    {
        double p = ZD;
        for (int i = 0; i < Cn<double>::FIX; i++) {
            v[i] = p;
            p *= ZD;
        }
    }
};
__device__ constexpr ZPow ZP{};  // one table for both types: (float)ZP.v[i] and ZP.v[i] round the same double product
template <typename T> __device__ __forceinline__ constexpr T zp(int i) { return (T)ZP.v[i]; }  // z^(i+1)

// eight filter weights in scalar registers, fetched right where a stage needs them (srx_patch.hpp's AxisW)
typedef float f8 __attribute__((ext_vector_type(8)));
__device__ __forceinline__ f8 sload8(const float *p)
{
    f8 v;
    asm volatile("s_load_dwordx8 %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=s"(v) : "s"(p) : "memory");
    return v;
}

// 16 bytes per lane through a buffer descriptor: the parked state travels as four rows per instruction (a CU issues a vector
// memory instruction every ~9 cycles whatever its width -- 12 descriptor loads took a wave 1.7 K cycles to issue -- so the 64 + 64
// one-word stores and loads that parked and re-read the state were a quarter of the iteration's critical path)
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
// The store takes its whole offset in the vector register and NO scalar offset.  A 128-bit store's data registers may not be
// overwritten by the very next vector instruction; the compiler's hazard recogniser knows that rule but exempts a buffer store
// whose soffset is a scalar register (GCNHazardRecognizer::createsVALUHazard) -- and on gfx950 the exemption does not hold when the
// memory pipeline is busy: tools/microbench/store_data_war.hip (16 waves per workgroup, 1024 workgroups) sees dwords 2, 3 of lanes
// 12..15 of a 16-lane row carry the overwriting values, with 0 wait states only.  k_ibp_dtile's first build stored rows 2, 3 of some
// row quads from the wrong register pair exactly there (a register-allocator v_mov_b64 right behind the store).
__device__ __forceinline__ void st4(__amdgpu_buffer_rsrc_t rs, int voff, int soff, float x, float y, float z, float w)
{
    u32x4 v = {__float_as_uint(x), __float_as_uint(y), __float_as_uint(z), __float_as_uint(w)};
    __builtin_amdgcn_raw_buffer_store_b128(v, rs, voff + soff, 0, 0);
}
__device__ __forceinline__ void ld4(__amdgpu_buffer_rsrc_t rs, int voff, int soff, float &x, float &y, float &z, float &w)
{
    const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rs, voff, soff, 0);
    x = __uint_as_float(v.x), y = __uint_as_float(v.y), z = __uint_as_float(v.z), w = __uint_as_float(v.w);
}

// two consecutive words through a buffer descriptor (32-bit lane offset; out of range reads 0)
__device__ __forceinline__ uint2 ld_u2(__amdgpu_buffer_rsrc_t rs, int byte_off)
{
    typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
    const u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(rs, byte_off, 0, 0);
    return make_uint2(v.x, v.y);
}

// ---- wave-private 64 x 64 transpose through a 32-row LDS image ----------------------------------------------------------
// in: a[i] = element (i, lane).  out: r[j] = element (lane, j).  (Rows / columns are abstract: the same routine goes back.)
__device__ __forceinline__ void transpose64(const float (&a)[64], float (&r)[64], float *Tw, int lane)
{
    // Each half of the wave reads its rows in its own pass, so r[] is written under a lane predicate -- and a predicated write
    // keeps the other lanes' previous contents: without a full definition the compiler must treat r[] as live from wherever it was
    // last written, across the whole preceding stage and around the iteration loop (64 registers pinned beside the 64 of the
    // working plane: ~150 spills per iteration).  An empty asm defines every element, placed where its life should start: after
    // pass 0 has parked a[0..31] in LDS, not before (an up-front definition keeps 128 registers live through the first 32 stores).
    // (Reading pass 0 unpredicated instead -- the upper half-wave re-reads the lower half's rows -- takes the same registers,
    // but a third more LDS read traffic in a phase the LDS bounds: measured C2 162 against 156 us per iteration.)
    // The rows are read 16 bytes at a time (ds_read_b128, 4 LDS cycles per wave-instruction for 1 KB): with the 66-word pitch before,
    // rows were only 8-byte aligned and hipcc fused the adjacent 8-byte reads into ds_read2_b64, which moves its 1 KB in 8 cycles.  Same-box
    // A/B on C2: 132.5-133.5 -> 128.3-130.1 us per iteration.  Reading with the WHOLE wave instead (the half-waves exchange quadrants by
    // v_permlane32_swap first, half as many reads, none predicated) shortens the transposes further and gains nothing: the swaps cost a
    // SIMD's four waves 25 cycles each, and the time reappears at the barriers around the transposes.
    const unsigned m0v = __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)Tw);  // LDS byte address of the wave's region
#pragma unroll
    for (int h = 0; h < 2; h++) {
        // Tw[i * TSD + lane] = a[32 h + i] as ds_write_addtid_b32 (address = M0 + offset + 4 * lane, no address register): two LDS
        // cycles per wave-instruction, where ds_write_b32 takes four (its address and data registers travel to the LDS at two cycles
        // per dword) -- the transposes are bound by exactly that (C2: 154 -> 152 us per iteration).  M0 and the stores in one asm block:
        // the compiler does not model M0 here.  M0 carries the full LDS byte address (the wave regions reach 139 KB; gfx950 honours more
        // than the 16 bits older ISA documents name -- with the address masked to 16 bits waves 8..15 wrote into the wrong regions and
        // tests/test_gpu_parity.py::test_patch_kernel_vs_oracle failed at once).
        static_assert(TSD * 4 == 272, "offsets below");
        asm volatile("s_mov_b32 m0, %16\n\t" SRX_M0_NOP
                     "ds_write_addtid_b32 %0 offset:0\n\t"
                     "ds_write_addtid_b32 %1 offset:272\n\t"
                     "ds_write_addtid_b32 %2 offset:544\n\t"
                     "ds_write_addtid_b32 %3 offset:816\n\t"
                     "ds_write_addtid_b32 %4 offset:1088\n\t"
                     "ds_write_addtid_b32 %5 offset:1360\n\t"
                     "ds_write_addtid_b32 %6 offset:1632\n\t"
                     "ds_write_addtid_b32 %7 offset:1904\n\t"
                     "ds_write_addtid_b32 %8 offset:2176\n\t"
                     "ds_write_addtid_b32 %9 offset:2448\n\t"
                     "ds_write_addtid_b32 %10 offset:2720\n\t"
                     "ds_write_addtid_b32 %11 offset:2992\n\t"
                     "ds_write_addtid_b32 %12 offset:3264\n\t"
                     "ds_write_addtid_b32 %13 offset:3536\n\t"
                     "ds_write_addtid_b32 %14 offset:3808\n\t"
                     "ds_write_addtid_b32 %15 offset:4080\n\t"
                     :: "v"(a[32 * h + 0]), "v"(a[32 * h + 1]), "v"(a[32 * h + 2]), "v"(a[32 * h + 3]), "v"(a[32 * h + 4]), "v"(a[32 * h + 5]), "v"(a[32 * h + 6]), "v"(a[32 * h + 7]), "v"(a[32 * h + 8]), "v"(a[32 * h + 9]), "v"(a[32 * h + 10]), "v"(a[32 * h + 11]), "v"(a[32 * h + 12]), "v"(a[32 * h + 13]), "v"(a[32 * h + 14]), "v"(a[32 * h + 15]), "s"(m0v) : "memory", "m0");
        asm volatile("s_mov_b32 m0, %16\n\t" SRX_M0_NOP
                     "ds_write_addtid_b32 %0 offset:4352\n\t"
                     "ds_write_addtid_b32 %1 offset:4624\n\t"
                     "ds_write_addtid_b32 %2 offset:4896\n\t"
                     "ds_write_addtid_b32 %3 offset:5168\n\t"
                     "ds_write_addtid_b32 %4 offset:5440\n\t"
                     "ds_write_addtid_b32 %5 offset:5712\n\t"
                     "ds_write_addtid_b32 %6 offset:5984\n\t"
                     "ds_write_addtid_b32 %7 offset:6256\n\t"
                     "ds_write_addtid_b32 %8 offset:6528\n\t"
                     "ds_write_addtid_b32 %9 offset:6800\n\t"
                     "ds_write_addtid_b32 %10 offset:7072\n\t"
                     "ds_write_addtid_b32 %11 offset:7344\n\t"
                     "ds_write_addtid_b32 %12 offset:7616\n\t"
                     "ds_write_addtid_b32 %13 offset:7888\n\t"
                     "ds_write_addtid_b32 %14 offset:8160\n\t"
                     "ds_write_addtid_b32 %15 offset:8432\n\t"
                     :: "v"(a[32 * h + 16]), "v"(a[32 * h + 17]), "v"(a[32 * h + 18]), "v"(a[32 * h + 19]), "v"(a[32 * h + 20]), "v"(a[32 * h + 21]), "v"(a[32 * h + 22]), "v"(a[32 * h + 23]), "v"(a[32 * h + 24]), "v"(a[32 * h + 25]), "v"(a[32 * h + 26]), "v"(a[32 * h + 27]), "v"(a[32 * h + 28]), "v"(a[32 * h + 29]), "v"(a[32 * h + 30]), "v"(a[32 * h + 31]), "s"(m0v) : "memory", "m0");
        __builtin_amdgcn_wave_barrier();
        if (h == 0) {
#pragma unroll
            for (int j = 0; j < 64; j++)
                asm volatile("" : "=v"(r[j]));
        }
        if ((lane >> 5) == h) {
            const float4 *row = reinterpret_cast<const float4 *>(Tw + (lane & 31) * TSD);
#pragma unroll
            for (int k = 0; k < 16; k++) {
                const float4 v = row[k];
                r[4 * k] = v.x, r[4 * k + 1] = v.y, r[4 * k + 2] = v.z, r[4 * k + 3] = v.w;
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
}

// ---- 64 x 64 transpose of a block of doubles through the same region: the low and the high words as two float transposes ---------------
__device__ __forceinline__ void transpose64(const double (&a)[64], double (&r)[64], float *Tw, int lane)
{
    float lo[64], t[64];
    int hi[64];
#pragma unroll
    for (int i = 0; i < 64; i++)
        lo[i] = __int_as_float(__double2loint(a[i])), hi[i] = __double2hiint(a[i]);
    transpose64(lo, t, Tw, lane);
    int rl[64];
#pragma unroll
    for (int i = 0; i < 64; i++)
        rl[i] = __float_as_int(t[i]), lo[i] = __int_as_float(hi[i]);
    transpose64(lo, t, Tw, lane);
#pragma unroll
    for (int i = 0; i < 64; i++)
        r[i] = __hiloint2double(__float_as_int(t[i]), rl[i]);
}

// ---- the recursion a[i] <- z a[i -+ 1] + a[i] over the 64 samples of a lane, as NSUB independent sub-chains ---------------------------
// One chain is 64 DEPENDENT fmas, and a dependent fma issues every ~11 cycles (tools/microbench/valu_issue.hip): a wave that runs its
// chain alone -- the usual case, the waves of a SIMD leave the throughput-bound phases one after the other -- idles 9 of 11 cycles.
// The recursion is linear, so the identity that joins the BLOCKS also cuts a chain inside a lane: sub-chain k > 0 starts from a zero
// state, and the true state at its start -- the end value of sub-chain k - 1 -- is added afterwards as z^(i+1) * state over its first
// FIX = 16 samples (|z|^17 = 2e-10).  Measured on one box (C2, tools/ab_bench.sh): one chain 138.3 us per iteration, two sub-chains
// 132.8, four (16 steps, then 3 x 16 fix-up fmas whose end values are themselves fixed first) 141.8 -- with four waves per SIMD the
// chains of several waves already overlap, and the fix-ups are real work.
constexpr int CHAIN_NSUB = 2;
template <bool REV, typename T> __device__ __forceinline__ void chain64(T (&a)[64], T st0)
{
    constexpr int NSUB = CHAIN_NSUB, L = 64 / NSUB, FIX = Cn<T>::FIX;
    static_assert(NSUB == 1 || L >= FIX, "a fix-up may not reach into the next sub-chain's start");
    const T z = Cn<T>::Z;
    auto at = [&](int i) -> T & { return a[REV ? 63 - i : i]; };  // position along the direction of the recursion
    T st[NSUB];
#pragma unroll
    for (int k = 0; k < NSUB; k++)
        st[k] = k == 0 ? st0 : (T)0;
#pragma unroll
    for (int i = 0; i < L; i++) {
#pragma unroll
        for (int k = 0; k < NSUB; k++) {
            st[k] = fma(z, st[k], at(k * L + i));
            at(k * L + i) = st[k];
        }
    }
    if (NSUB > 1) {
        T e[NSUB];  // true end values of the sub-chains
        e[0] = st[0];
#pragma unroll
        for (int k = 1; k < NSUB; k++)
            e[k] = L == FIX ? fma(zp<T>(FIX - 1), e[k - 1], st[k]) : st[k];  // (longer sub-chains: the end is out of the fix-up's reach)
#pragma unroll
        for (int k = 1; k < NSUB; k++) {
#pragma unroll
            for (int i = 0; i < FIX; i++)
                at(k * L + i) = fma(zp<T>(i), e[k - 1], at(k * L + i));
        }
    }
}
// the same fix-up between the BLOCKS of a line: the state the block did not see -- the previous block's end value (REV: the next block's
// first coefficient) -- over its first (REV: last) FIX samples
template <bool REV, typename T> __device__ __forceinline__ void add_carry(T (&a)[64], T carry)
{
#pragma unroll
    for (int i = 0; i < Cn<T>::FIX; i++)
        a[REV ? 63 - i : i] = fma(zp<T>(i), carry, a[REV ? 63 - i : i]);
}

// ---- what the blocks of a line tell their neighbours, each in two halves with the workgroup barrier between them left to the caller ------
// halo3: the three samples before / after a block (zero beyond the line's ends), for a 7-tap blur along the registers.  s6: a 384-word slot.
template <typename T> struct Halo3 {
    T lo[3], hi[3];
};
template <typename T> __device__ __forceinline__ void halo3_put(const T (&a)[64], T *Rown, int s6, int lane)
{
    Rown[s6 + lane] = a[0];
    Rown[s6 + 64 + lane] = a[1];
    Rown[s6 + 128 + lane] = a[2];
    Rown[s6 + 192 + lane] = a[61];
    Rown[s6 + 256 + lane] = a[62];
    Rown[s6 + 320 + lane] = a[63];
}
template <typename T> __device__ __forceinline__ Halo3<T> halo3_get(bool first, bool last, const T *Rprev, const T *Rnext, int s6, int lane)
{
    Halo3<T> h = {{0, 0, 0}, {0, 0, 0}};
    if (!first)
        h.lo[0] = Rprev[s6 + 192 + lane], h.lo[1] = Rprev[s6 + 256 + lane], h.lo[2] = Rprev[s6 + 320 + lane];
    if (!last)
        h.hi[0] = Rnext[s6 + lane], h.hi[1] = Rnext[s6 + 64 + lane], h.hi[2] = Rnext[s6 + 128 + lane];
    return h;
}
// gnbr: the G samples around a block that bwd_front's FIR reaches -- gm1 just before it (gtop, the line's G[-ex], in front of the first
// block), gp1 / gp2 behind it (zero behind the last).  s3: a 192-word slot.  (By value into a const local: as three reference
// out-parameters the same code cost k_ibp_patch 4 - 12 bytes of scratch and k_ibp_dtile a register.)
template <typename T> struct GNbr {
    T gm1, gp1, gp2;
};
template <typename T> __device__ __forceinline__ void gnbr_put(const T (&g)[64], T *Rown, int s3, int lane)
{
    Rown[s3 + lane] = g[0];
    Rown[s3 + 64 + lane] = g[1];
    Rown[s3 + 128 + lane] = g[63];
}
template <typename T> __device__ __forceinline__ GNbr<T> gnbr_get(bool first, bool last, const T *Rprev, const T *Rnext, int s3, int lane, T gtop)
{
    return {first ? gtop : Rprev[s3 + 128 + lane], last ? (T)0 : Rnext[s3 + lane], last ? (T)0 : Rnext[s3 + 64 + lane]};
}

// ---- forward chain of one block, in place ------------------------------------------------------------------------------
// a[] in: kq-scaled blurred samples b' of this block.  out: Y[rho], rho = the block's own 64 indices;
// Y[rho] = sum_a wf[a] c[rho - 2 + a], c = P(pad12(b)).  yex (first block): Y[-1].
// Rown / Rprev / Rnext: LDS regions of this wave and of the waves holding the previous / next block of the line.
// Two workgroup barriers.  sa: 64-word slot, sb: 192-word slot.  wf[0..3]: the forward FIR.
template <typename T, typename W>
__device__ __forceinline__ void fwd_chain(T (&a)[64], bool first, bool last, T *Rown, const T *Rprev, const T *Rnext, int sa, int sb, int lane,
                                          const W &wf, T &yex)
{
    constexpr T z = Cn<T>::Z, K1 = Cn<T>::K1, K2 = Cn<T>::K2, K3 = Cn<T>::K3;
    const T bfirst = a[0], blast = a[63];
    chain64<false>(a, first ? bfirst * K2 : (T)0);  // inside the constant pad the causal state is the steady state
    Rown[sa + lane] = a[63];
    __syncthreads();
    if (!first)
        add_carry<false>(a, Rprev[sa + lane]);
    // coefficient of the first sample below the line: 12 constant pad samples, then SciPy's reflect end (z^24 away)
    const T cb = last ? fma(a[63] - blast * K2, K3, blast * K1) : (T)0;
    chain64<true>(a, cb);
    T cm1 = 0, cm2 = 0;  // c[-1], c[-2] relative to the block
    if (first) {         // coefficients inside the top pad: c[i] = z c[i+1] + qs
        const T qs = bfirst * K2;
        cm1 = fma(z, a[0], qs);
        cm2 = fma(z, cm1, qs);
        const T cm3 = fma(z, cm2, qs);
        yex = wf[0] * cm3 + wf[1] * cm2 + wf[2] * cm1 + wf[3] * a[0];
    }
    Rown[sb + lane] = a[0];
    Rown[sb + 64 + lane] = a[62];
    Rown[sb + 128 + lane] = a[63];
    __syncthreads();
    T hb = cb;
    if (!last) {
        hb = Rnext[sb + lane];
        add_carry<true>(a, hb);
    }
    if (!first) {  // the previous block's last two coefficients, with the carry (this block's c[0]) they have not seen yet
        cm2 = fma(zp<T>(1), a[0], Rprev[sb + 64 + lane]);
        cm1 = fma(zp<T>(0), a[0], Rprev[sb + 128 + lane]);
    }
    T c2 = cm2, c1 = cm1;
#pragma unroll
    for (int i = 0; i < 64; i++) {
        const T c0 = a[i], cn = i < 63 ? a[i + 1] : hb;
        a[i] = wf[0] * c2 + wf[1] * c1 + wf[2] * c0 + wf[3] * cn;
        c2 = c1, c1 = c0;
    }
}

// ---- backward chain of one block: its front half, in place ---------------------------------------------------------------
// a[] in: G samples of this block; gm1 / gp1 / gp2: G just before / after the block (halo exchange done by the caller);
// gtop: G[-ex] of the line (first block); wb[0..3]: the backward FIR.  out: a[] = the block's coefficients of crop P( FIR_b G ), and
// hlo / hhi = the three coefficients before / after the block (zero outside the image: the crop) for the blur' that follows -- the
// caller's, each form tuned for its register budget (bwd_chain_x below; srx_stile.hpp's blur_inplace).  Two workgroup barriers.
template <typename T, typename W>
__device__ __forceinline__ void bwd_front(T (&a)[64], bool first, bool last, T *Rown, const T *Rprev, const T *Rnext, int s1, int s6, int lane,
                                          const W &wb, T gm1, T gp1, T gp2, T gtop, T (&hlo)[3], T (&hhi)[3])
{
    constexpr T z = Cn<T>::Z, K2 = Cn<T>::K2, K4 = Cn<T>::K4;
    const T w0 = wb[0], w1 = wb[1], w2 = wb[2], w3 = wb[3];
    const T vn = last ? w0 * a[63] : (T)0;  // v'[n]: the one pad sample below the line whose FIR window holds a real row
    SRX_PSTAMP(15);
    T st = 0;
    if (first) {  // the pad: a constant run of G[-ex] (steady state), then the two samples whose window reaches rows 0, 1
        st = (w0 + w1 + w2 + w3) * gtop * K2;
        st = fma(z, st, (w0 + w1 + w2) * gtop + w3 * a[0]);
        st = fma(z, st, (w0 + w1) * gtop + w2 * a[0] + w3 * a[1]);
    }
    // the FIR in place (independent fmas), then the recursion on its output
    T gprev = gm1;
#pragma unroll
    for (int t = 0; t < 64; t++) {
        const T g0 = a[t], g1 = t < 63 ? a[t + 1] : gp1, g2 = t < 62 ? a[t + 2] : (t == 62 ? gp1 : gp2);
        a[t] = w0 * gprev + w1 * g0 + w2 * g1 + w3 * g2;
        gprev = g0;
    }
    chain64<false>(a, st);
    SRX_PSTAMP(16);
    Rown[s1 + lane] = a[63];
    __syncthreads();
    SRX_PSTAMP(17);
    if (!first)
        add_carry<false>(a, Rprev[s1 + lane]);
    const T cb = last ? fma(z, a[63], vn) * K4 : (T)0;
    chain64<true>(a, cb);
    halo3_put(a, Rown, s6, lane);  // (fetched below with the carry fix-ups, not by halo3_get)
    SRX_PSTAMP(18);
    __syncthreads();
    SRX_PSTAMP(19);
    hlo[0] = hlo[1] = hlo[2] = hhi[0] = hhi[1] = hhi[2] = (T)0;
    if (!last) {
        const T cn = Rnext[s6 + lane];
        add_carry<true>(a, cn);
        hhi[0] = cn, hhi[1] = Rnext[s6 + 64 + lane], hhi[2] = Rnext[s6 + 128 + lane];
    }
    if (!first) {  // the previous block's last three coefficients, with the carry (this block's c[0]) they have not seen yet
        hlo[0] = fma(zp<T>(2), a[0], Rprev[s6 + 192 + lane]);
        hlo[1] = fma(zp<T>(1), a[0], Rprev[s6 + 256 + lane]);
        hlo[2] = fma(zp<T>(0), a[0], Rprev[s6 + 320 + lane]);
    }
    SRX_PSTAMP(20);
}

// ---- backward chain of one block, k_ibp_patch's form: out = post(i, blur'( crop P( FIR_b G ) )[i]), out of place, in quarters ------------
// wfb[4..7]: the backward FIR.  BLUR = false (a PSF that is not rank 1: the adjoint blur is blur2d's, once, in column layout): out = the
// coefficients themselves, and hlo / hhi = the three coefficients before / after the block for that blur.
struct Hi4 {  // elements 4..7 of a weight vector, indexed [0..3]
    f8 v;
    __device__ __forceinline__ float operator[](int i) const { return v[4 + i]; }
};
template <bool BLUR, typename F, typename P>
__device__ __forceinline__ void bwd_chain_x(float (&a)[64], float (&out)[64], bool first, bool last, float *Rown, const float *Rprev,
                                            const float *Rnext, int s1, int s6, int lane, const f8 wfb, const f8 kt, float gm1, float gp1,
                                            float gp2, float gtop, F mid, P post, float (&hlo)[3], float (&hhi)[3])
{
    bwd_front(a, first, last, Rown, Rprev, Rnext, s1, s6, lane, Hi4{wfb}, gm1, gp1, gp2, gtop, hlo, hhi);
    if (!BLUR) {
#pragma unroll
        for (int i = 0; i < 64; i++)
            out[i] = a[i];
        return;
    }
    float e[70];  // the block's coefficients with three on either side
#pragma unroll
    for (int i = 0; i < 3; i++)
        e[i] = hlo[i], e[67 + i] = hhi[i];
#pragma unroll
    for (int i = 0; i < 64; i++)
        e[3 + i] = a[i];
#pragma unroll
    for (int q = 0; q < 4; q++) {
        mid(q);  // caller's hook before every quarter of the blur (loads / stores to overlap with it)
#pragma unroll
        for (int i = 16 * q; i < 16 * q + 16; i++) {
            float acc = kt[0] * e[i];
#pragma unroll
            for (int u = 1; u < 7; u++)
                acc = fmaf(kt[u], e[i + u], acc);
            out[i] = post(i, acc);  // caller's epilogue (identity, or the IBP update)
        }
        __builtin_amdgcn_sched_barrier(0);
    }
}

template <typename F, typename P>
__device__ __forceinline__ void bwd_chain(float (&a)[64], float (&out)[64], bool first, bool last, float *Rown, const float *Rprev,
                                          const float *Rnext, int s1, int s6, int lane, const f8 wfb, const f8 kt, float gm1, float gp1,
                                          float gp2, float gtop, F mid, P post)
{
    float hlo[3], hhi[3];
    bwd_chain_x<true>(a, out, first, last, Rown, Rprev, Rnext, s1, s6, lane, wfb, kt, gm1, gp1, gp2, gtop, mid, post, hlo, hhi);
}

// ---- 7-tap correlation along the registers, in place: a[i] <- post(i, sum_q k[q] x[i - 3 + q]); hl / hr: the three samples before / after
// the block; pre(j0) runs before the group of outputs that starts at j0 (loads to overlap).
// Eight outputs at a time: besides a[] only the 14-value window and the three old values the next group still needs
// are live, and a scheduling fence after every group keeps the compiler from interleaving more outputs than the registers hold
// (left alone it trades ~30 spilled registers per blur for instruction-level parallelism).
template <typename T, typename W, typename PRE, typename POST>
__device__ __forceinline__ void blur_inplace(T (&a)[64], const T (&hl)[3], const T (&hr)[3], const W &k, PRE pre, POST post)
{
    T c0 = hl[0], c1 = hl[1], c2 = hl[2];
#pragma unroll
    for (int j0 = 0; j0 < 64; j0 += 8) {
        pre(j0);
        T w[14];
        w[0] = c0, w[1] = c1, w[2] = c2;
#pragma unroll
        for (int j = 0; j < 8; j++)
            w[3 + j] = a[j0 + j];
#pragma unroll
        for (int j = 0; j < 3; j++)
            w[11 + j] = j0 + 8 + j < 64 ? a[j0 + 8 + j] : hr[j];
        c0 = w[8], c1 = w[9], c2 = w[10];
#pragma unroll
        for (int j = 0; j < 8; j++) {
            T acc = k[0] * w[j];
#pragma unroll
            for (int q = 1; q < 7; q++)
                acc = fma(k[q], w[j + q], acc);
            a[j0 + j] = post(j0 + j, acc);
        }
        __builtin_amdgcn_sched_barrier(0);
    }
}
// blur of a block with three samples from either neighbour block: halo exchange through the waves' own LDS slots, one workgroup
// barrier.  a[] in: raw samples, out: sum_k kb[k] x[i - 3 + k] (zero outside the image).
template <typename T, typename W>
__device__ __forceinline__ void blur_block(T (&a)[64], bool first, bool last, T *Rown, const T *Rprev, const T *Rnext, int s6, int lane, const W &kb)
{
    halo3_put(a, Rown, s6, lane);
    __syncthreads();
    const Halo3<T> h = halo3_get(first, last, Rprev, Rnext, s6, lane);
    blur_inplace(a, h.lo, h.hi, kb, [](int) {}, [](int, T v) { return v; });
}

// ---- one-lane wave shifts (DPP wave_shr:1 / wave_shl:1) ------------------------------------------------------------------------
// up: lane i reads lane i - 1;  dn: lane i reads lane i + 1.  lane_up / lane_dn shift a zero in at the wave's end; shift_up / shift_dn
// pull a given value in there: lane 0 (up) / lane 63 (dn) keeps `fill` (a double moves as its two words).
__device__ __forceinline__ float lane_up(float v) { return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x138, 0xf, 0xf, true)); }
__device__ __forceinline__ float lane_dn(float v) { return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x130, 0xf, 0xf, true)); }
template <int CTRL> __device__ __forceinline__ float shift_fill(float v, float fill)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(fill), __float_as_int(v), CTRL, 0xf, 0xf, false));
}
template <int CTRL> __device__ __forceinline__ double shift_fill(double v, double fill)
{
    const long long a = __double_as_longlong(v), o = __double_as_longlong(fill);
    const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp((int)(unsigned)o, (int)(unsigned)a, CTRL, 0xf, 0xf, false);
    const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp((int)(unsigned)(o >> 32), (int)(unsigned)(a >> 32), CTRL, 0xf, 0xf, false);
    return __longlong_as_double((long long)((unsigned long long)hi << 32 | lo));
}
template <typename T> __device__ __forceinline__ T shift_up(T v, T fill) { return shift_fill<0x138>(v, fill); }
template <typename T> __device__ __forceinline__ T shift_dn(T v, T fill) { return shift_fill<0x130>(v, fill); }

// ---- 7 x 7 correlation with a PSF that is not rank 1, on one block of the 4 x 4 grid, COLUMN layout (round 4) --------------------------
// out[i][l] = sum_{r, c} K[r][c] in[i - 3 + r][l - 3 + c]: the r direction runs along the registers (three rows from the blocks above / below:
// hl / hr), the c direction along the LANES -- every lane forms the seven column sums t_c = sum_r K[r][c] in[i - 3 + r] of its own column and
// a Horner scheme of one-lane wave shifts combines them, out = t_3 + up(t_2 + up(t_1 + up(t_0))) + dn(t_4 + dn(t_5 + dn(t_6))) (k_ibp_ztile's
// blur2d_block; two adjacent rows advance as one packed pair).  What k_ibp_ztile does not have is a neighbour in the lane direction: here the
// waves left / right hold the next columns.  The shifts run with zero shifted in (pass 1), and by linearity what is missing at a wave's first /
// last three lanes are the neighbour's OWN Horner partials at its last / first lane -- U1 = t_0, U2 = t_1 + up(U1), U3 = t_2 + up(U2) at lane 63,
// D1 = t_6, D2, D3 at lane 0, none of which depends on a fill: lanes 63 and 0 publish them (one 16-byte LDS store per row with the other
// lanes masked off; exec is set and restored inside the asm so that the loop stays one basic block), and behind a barrier every lane adds
// the one it lacks (lane 0 <- U3, 1 <- U2, 2 <- U1 of the left wave; 63 <- D3, 62 <- D2, 61 <- D1 of the right one; a zero word elsewhere):
// one LDS read and one add per row (pass 2, blur2d_fix, which also carries the caller's epilogue: the IBP update must see the complete sum).
// RAD = 2: the PSF's outer ring is zero (the reference's measured PSF): 25 multiply-adds and four shifts per pixel instead of 49 and six.
typedef float f2 __attribute__((ext_vector_type(2)));
typedef float f4 __attribute__((ext_vector_type(4)));
constexpr int SLOT_E = 1536;  // a wave's published partials: [64 rows][8 words] = U1 U2 U3 . D1 D2 D3 . (inside its private region, behind the exchange slots)
constexpr int SLOT_D = 512;   // 256 words between the exchange slots: where the lanes that publish nothing store (distinct quads: no bank conflict)
constexpr int SLOT_Z = 2048;  // eight zero words (what the lanes that lack nothing add; what a wave at the patch's edge reads for its missing neighbour)
static_assert(SLOT_D >= SLOT0 + 448 && SLOT_D + 256 <= SLOT1 && SLOT_E >= SLOT1 + 448 && SLOT_E + 512 <= SLOT_Z && SLOT_Z + 8 <= RW, "slots inside the wave's region");

constexpr int B2D_NB = 4;  // rows that blur2d_pass1 advances together
template <int RAD>
__device__ __forceinline__ void blur2d_pass1(float (&a)[64], const float (&hl)[3], const float (&hr)[3], float *Rown, int lane, const float *w56)
{
    static_assert(RAD == 2 || RAD == 3, "5 x 5 core or full 7 x 7");
    constexpr int LO = 3 - RAD, HI = 3 + RAD;
    f8 kw[7];  // kw[c][r]
#pragma unroll
    for (int c = 0; c < 7; c++)
        kw[c] = sload8(w56 + 8 * c);
    if (lane < 8)
        Rown[SLOT_Z + lane] = 0.f;
    // where this lane's 16 bytes of a row go: lane 63 -> U half, lane 0 -> D half of the row's slot; every other lane into its own quad of a
    // dump area (the store is unpredicated: the loop stays one basic block)
    f4 *edst = reinterpret_cast<f4 *>(__builtin_assume_aligned(lane == 63 ? Rown + SLOT_E : lane == 0 ? Rown + SLOT_E + 4 : Rown + SLOT_D + 4 * lane, 16));
    const int estr = (lane == 63 || lane == 0) ? 2 : 0;  // in units of 16 bytes per row
    constexpr int NB = B2D_NB;
    float c0 = hl[0], c1 = hl[1], c2 = hl[2];
#pragma unroll
    for (int j0 = 0; j0 < 64; j0 += NB) {
        float w[NB + 6];
        w[0] = c0, w[1] = c1, w[2] = c2;
#pragma unroll
        for (int j = 0; j < NB; j++)
            w[3 + j] = a[j0 + j];
#pragma unroll
        for (int j = 0; j < 3; j++)
            w[NB + 3 + j] = j0 + NB + j < 64 ? a[j0 + NB + j] : hr[j];
        c0 = w[NB], c1 = w[NB + 1], c2 = w[NB + 2];
        // (scalar multiply-adds, not k_ibp_ztile's packed pairs: with four waves per SIMD a v_pk_fma_f32 costs the SIMD what two v_fma_f32 do, and the
        // pairs (w[m], w[m + 1]) of BOTH alignments tie the plane's registers into 64-bit tuples all the way back through the chains of stage C:
        // 57 / 77 spilled registers and 0.32 GB of scratch traffic per C2 iteration in the packed form -- same time, 220 us.  The packed form's
        // count-PLANE instantiations (103 spilled registers) also gave results that changed from call to call on two of four configurations of
        // tools/dev/pt_check.py -- not a race (extra barriers changed nothing), no unwritten table (NaN poisoning left no NaN), never understood;
        // this form has 1 - 2 spilled registers and passes all of them)
#pragma unroll
        for (int j = 0; j < NB; j++) {
            float t[7];
#pragma unroll
            for (int c = LO; c <= HI; c++) {
                t[c] = kw[c][LO] * w[j + LO];
#pragma unroll
                for (int r = LO + 1; r <= HI; r++)
                    t[c] = fmaf(kw[c][r], w[j + r], t[c]);
            }
            float u1, u2, u3, d1, d2, d3;
            if (RAD == 3) {
                u1 = t[0], d1 = t[6];
                u2 = t[1] + lane_up(u1), d2 = t[5] + lane_dn(d1);
            } else {  // the missing first stage: U1 = D1 = 0
                u1 = 0.f, d1 = 0.f;
                u2 = t[1], d2 = t[5];
            }
            u3 = t[2] + lane_up(u2), d3 = t[4] + lane_dn(d2);
            const float res = (t[3] + lane_up(u3)) + lane_dn(d3);
            const f4 ev = lane == 0 ? (f4){d1, d2, d3, 0.f} : (f4){u1, u2, u3, 0.f};
            edst[(j0 + j) * estr] = ev;
            a[j0 + j] = res;
            asm volatile("" : "+v"(a[j0 + j]));  // (as in k_ibp_ztile: the last adds of a pixel stay with its arithmetic)
        }
        __builtin_amdgcn_sched_barrier(0);
    }
}
// pass 2: lfirst / llast: no wave before / after this one in the lane direction; Rlo / Rhi: the regions of those waves.  pre(q) runs before
// quarter q of the rows (the parked state's loads), post(i, v) is the epilogue of row i.
template <int RAD, typename PRE, typename POST>
__device__ __forceinline__ void blur2d_fix(float (&a)[64], bool lfirst, bool llast, float *Rown, const float *Rlo, const float *Rhi, int lane, PRE pre, POST post)
{
    // word offset of the partial this lane lacks inside a row's slot of the neighbour: U3, U2, U1 for lanes 0, 1, 2; D1, D2, D3 for 61, 62, 63
    const float *src = lane < 3 ? (lfirst ? Rown + SLOT_Z : Rlo + SLOT_E + 2 - lane) : lane >= 61 ? (llast ? Rown + SLOT_Z : Rhi + SLOT_E + 4 + lane - 61) : Rown + SLOT_Z;
    const int str = (lane < 3 ? !lfirst : lane >= 61 ? !llast : false) ? 8 : 0;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        pre(q);
#pragma unroll
        for (int i = 16 * q; i < 16 * q + 16; i++)
            a[i] = post(i, a[i] + src[i * str]);
        __builtin_amdgcn_sched_barrier(0);
    }
}
// both passes on a block whose three rows above / below (hl / hr) the caller holds: one workgroup barrier
template <int RAD, typename PRE, typename POST>
__device__ __forceinline__ void blur2d_cols(float (&a)[64], const float (&hl)[3], const float (&hr)[3], bool lfirst, bool llast, float *Rown, const float *Rlo,
                                            const float *Rhi, int lane, const float *w56, PRE pre, POST post)
{
    blur2d_pass1<RAD>(a, hl, hr, Rown, lane, w56);
    __syncthreads();
    blur2d_fix<RAD>(a, lfirst, llast, Rown, Rlo, Rhi, lane, pre, post);
}

}  // namespace blk
}  // namespace srx
