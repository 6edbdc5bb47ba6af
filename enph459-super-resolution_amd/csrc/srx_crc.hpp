// srx_crc.hpp -- CRC-32 (zlib's and PNG's: reflected, P = 0xEDB88320, init and final xor 0xFFFFFFFF) of device buffers (srx_crc32), and
// the PNG file around a device-made zlib stream (srx_png_file_*: signature, IHDR, one IDAT, IEND), so that a finished file leaves the device.
//
// CRC-32 is linear over GF(2).  raw(M) is the remainder with init 0 and no final xor, mulx(v, k) = v x^k mod P:
//   raw(A | B)     = mulx(raw(A), 8 |B|) ^ raw(B)
//   raw(0...0 | M) = raw(M)                                            (leading zero bytes leave a zero register at zero)
//   crc32(M, seed) = raw(M) ^ mulx(seed ^ 0xFFFFFFFF, 8 |M|) ^ 0xFFFFFFFF     (zlib.crc32(M, seed); seed = 0: a fresh CRC)
// A message of L bytes is cut into segments of SEGMENT bytes from its END (segment s of nseg = ceil(L / SEGMENT) covers
// [L - (nseg - s) SEGMENT, L - (nseg - s - 1) SEGMENT), clipped at 0), and a segment into spans of SPAN bytes from its end: only the first
// segment and its first span are short -- as if zeros stood in front of them -- and every piece that FOLLOWS another one is full.  The
// powers of a combination tree are then the same for every lane: x^(8 SPAN 2^s) at step s, out of POW8, x^(8 2^j) for j = 0..31.
//
// Part 1 (plain integer code, host and device; tests/crc_host_model.cpp builds it with g++ and reduces a file in the kernels' order):
//   table_entry, raw_step / raw_span, gfmul, POW8 / xpow8, seg_geom, slice_of, finish, the PNG file's 33 constant bytes.
// Part 2 (device), two launches:
//   k_crc_segments   grid (segments, B), 256 lanes.  The segment -> LDS (16-byte loads aligned by the kernel, single bytes at the ends;
//                    spans 68 bytes apart: 17 banks), the byte table -> LDS (each lane its own entry); a lane reduces its span, its 16
//                    words read first and the 64 table reads the only dependent chain; eight tree steps in LDS; one uint32 per segment.
//   k_crc_finish<F>  grid B, 256 lanes.  A lane folds a contiguous slice of the item's segments (Horner in x^(8 SEGMENT)), eight tree steps
//                    in x^(8 SEGMENT per) and its squares, the seed term with x^(8 L) as a product over the bits of L (32 lanes, five
//                    shuffle steps).  F = false: crc[b].  F = true (srx_png_file_*): the 41 bytes in front of the stream, the IDAT's
//                    CRC and IEND behind it, and the file's length, all as byte stores.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define SRX_CRC_HD __host__ __device__
#else
#define SRX_CRC_HD
#endif

namespace srx {
namespace crc {

constexpr int SPAN = 64;                 // SRX_CRC_SPAN: bytes one lane reduces
constexpr int SEGMENT = 16384;           // SRX_CRC_SEGMENT: bytes of one workgroup
constexpr int LANES = SEGMENT / SPAN;    // 256
constexpr uint32_t POLY = 0xEDB88320u;
constexpr uint32_t ONE = 0x80000000u;    // x^0 (reflected: bit 31 is the coefficient of x^0)
constexpr int FILE_HEAD = 41, FILE_TAIL = 16, FILE_EXTRA = FILE_HEAD + FILE_TAIL;  // SRX_PNG_FILE_EXTRA

// entry i of the byte table: i x^32 mod P after eight steps
SRX_CRC_HD constexpr uint32_t table_entry(uint32_t i)
{
    for (int k = 0; k < 8; k++)
        i = (i >> 1) ^ (POLY & (0u - (i & 1u)));
    return i;
}

// one byte into the register; `tab` is anything tab[i] reads entry i of (an array, the kernels' LDS copy)
template <typename Tab> SRX_CRC_HD inline uint32_t raw_step(uint32_t v, uint32_t byte, const Tab &tab) { return tab[(v ^ byte) & 0xffu] ^ (v >> 8); }

// raw of bytes [s, e) of `d`
template <typename Bytes, typename Tab> SRX_CRC_HD inline uint32_t raw_span(const Bytes &d, int64_t s, int64_t e, const Tab &tab)
{
    uint32_t v = 0;
    for (int64_t i = s; i < e; i++)
        v = raw_step(v, (uint32_t)d[i], tab);
    return v;
}

// a b mod P (gfmul(a, ONE) == a)
SRX_CRC_HD constexpr uint32_t gfmul(uint32_t a, uint32_t b)
{
    uint32_t p = 0;
    for (int i = 0; i < 32; i++) {
        p ^= b & (0u - (a >> 31));
        a <<= 1;
        b = (b >> 1) ^ (POLY & (0u - (b & 1u)));
    }
    return p;
}

// x^(8 2^j) mod P, j = 0..31: every power the kernels need is one of these or a product of them
struct Pow8 {
    uint32_t t[32];
};
SRX_CRC_HD constexpr Pow8 make_pow8()
{
    Pow8 p{};
    p.t[0] = ONE >> 8;
    for (int j = 1; j < 32; j++)
        p.t[j] = gfmul(p.t[j - 1], p.t[j - 1]);
    return p;
}
constexpr Pow8 POW8 = make_pow8();

// x^(8 bytes) mod P for bytes < 2^32, one factor after the other (the host's form; the kernels multiply the factors as a tree)
SRX_CRC_HD inline uint32_t xpow8(const uint32_t *pow8, uint64_t bytes)
{
    uint32_t p = ONE;
    for (int j = 0; j < 32; j++)
        if ((bytes >> j) & 1u)
            p = gfmul(p, pow8[j]);
    return p;
}

SRX_CRC_HD inline uint64_t segments_of(uint64_t L, uint64_t segment) { return (L + segment - 1) / segment; }

// segment s of a message of L bytes: its first byte, its n bytes, and the `pad` zeros imagined in front of it (n + pad == segment)
struct SegGeom {
    int64_t lo;
    int n, pad;
};
SRX_CRC_HD inline SegGeom seg_geom(uint64_t L, uint64_t nseg, uint64_t s, int segment)
{
    const int64_t start = (int64_t)L - (int64_t)(nseg - s) * segment;
    SegGeom g;
    g.lo = start < 0 ? 0 : start;
    g.pad = (int)(g.lo - start);
    g.n = segment - g.pad;
    return g;
}

// the finish: `lanes` slices of `per` = max(1, ceil(nseg / lanes)) segments each, counted from the end; [lo, hi) is lane's
SRX_CRC_HD inline uint32_t slice_len(uint64_t nseg, int lanes) { return nseg ? (uint32_t)((nseg + (uint64_t)lanes - 1) / (uint64_t)lanes) : 1u; }
SRX_CRC_HD inline void slice_of(uint64_t nseg, uint32_t per, int lane, int lanes, uint32_t &lo, uint32_t &hi)
{
    const int64_t h = (int64_t)nseg - (int64_t)(lanes - 1 - lane) * per, l = h - per;
    hi = (uint32_t)(h < 0 ? 0 : h);
    lo = (uint32_t)(l < 0 ? 0 : l);
}

// crc32(M, seed) from raw(M) and x^(8 |M|)
SRX_CRC_HD inline uint32_t finish(uint32_t raw, uint32_t seed, uint32_t pow_len) { return raw ^ gfmul(seed ^ 0xffffffffu, pow_len) ^ 0xffffffffu; }

// the plain CRC of a few bytes, bit by bit (the file's constant parts, on the host)
SRX_CRC_HD inline uint32_t crc_bytes(const uint8_t *d, int n, uint32_t seed)
{
    uint32_t v = seed ^ 0xffffffffu;
    for (int i = 0; i < n; i++)
        v = table_entry((v ^ d[i]) & 0xffu) ^ (v >> 8);
    return v ^ 0xffffffffu;
}

// The first 33 bytes of an 8-bit PNG of W x H pixels, greyscale (colour type 0) or truecolour (2: srx_png_file_rgb8): signature, IHDR
// (length, tag, 13 bytes, CRC).  Behind them: the IDAT's length
// (big endian), "IDAT", the stream, the CRC of "IDAT" + stream, and file_iend.
struct FileHead {
    uint8_t b[36];  // 33 used
};
SRX_CRC_HD inline FileHead file_head(uint32_t W, uint32_t H, uint8_t colour_type = 0)
{
    FileHead h{};
    const uint8_t sig[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1a, '\n'};
    for (int i = 0; i < 8; i++)
        h.b[i] = sig[i];
    uint8_t *c = h.b + 8;
    c[0] = c[1] = c[2] = 0, c[3] = 13;
    c[4] = 'I', c[5] = 'H', c[6] = 'D', c[7] = 'R';
    for (int i = 0; i < 4; i++) {
        c[8 + i] = (uint8_t)(W >> (24 - 8 * i));
        c[12 + i] = (uint8_t)(H >> (24 - 8 * i));
    }
    c[16] = 8;  // bit depth; the colour type; compression 0, filter 0, interlace 0
    c[17] = colour_type;
    c[18] = c[19] = c[20] = 0;
    const uint32_t v = crc_bytes(c + 4, 17, 0);
    for (int i = 0; i < 4; i++)
        c[21 + i] = (uint8_t)(v >> (24 - 8 * i));
    return h;
}
SRX_CRC_HD inline uint32_t idat_seed()
{
    const uint8_t tag[4] = {'I', 'D', 'A', 'T'};
    return crc_bytes(tag, 4, 0);
}
// the 12 bytes of IEND: an empty chunk and the CRC of its tag
SRX_CRC_HD inline void file_iend(uint8_t *t)
{
    t[0] = t[1] = t[2] = t[3] = 0;
    t[4] = 'I', t[5] = 'E', t[6] = 'N', t[7] = 'D';
    t[8] = 0xAE, t[9] = 0x42, t[10] = 0x60, t[11] = 0x82;
}

}  // namespace crc
}  // namespace srx

#if defined(__HIPCC__) && !defined(SRX_CRC_HOST_ONLY)
#include "srx_common.h"
#include "srx_png.hpp"

namespace srx {
namespace crc {

constexpr int ilog2(int v) { return v <= 1 ? 0 : 1 + ilog2(v >> 1); }
static_assert(LANES == 256 && (1 << ilog2(SPAN)) == SPAN && SPAN % 16 == 0, "the trees take their powers from POW8; the stage moves 16 bytes");

__device__ const Pow8 pow8_dev = make_pow8();

// the segment in LDS: four bytes of padding behind every span (srx_png.hpp's Raw: 68 bytes = 17 banks from lane to lane).  With the
// spans 64 bytes apart instead: measured, no difference beyond the rounds' spread.
constexpr int PAD = 4, PITCH = SPAN + PAD;
static_assert(PAD >= 0 && PAD % 4 == 0, "the spans stay word aligned");
constexpr int STAGE_BYTES = PITCH * LANES;
__device__ __forceinline__ int padded(int v) { return v + (v / SPAN) * PAD; }

// the item's length: lengths[b] clamped to [0, max_len], or max_len
__device__ __forceinline__ uint32_t item_len(const long long *__restrict__ lengths, uint32_t b, uint32_t max_len)
{
    if (!lengths)
        return max_len;
    const long long l = lengths[b];
    return l <= 0 ? 0u : l < (long long)max_len ? (uint32_t)l : max_len;
}

// x^(8 bytes) on every lane: lane j (mod 32) holds the factor of bit j, five steps of pairwise products
__device__ __forceinline__ uint32_t xpow8_wave(uint32_t bytes)
{
    const int j = threadIdx.x & 31;
    uint32_t m = ((bytes >> j) & 1u) ? pow8_dev.t[j] : ONE;
#pragma unroll
    for (int o = 16; o > 0; o >>= 1)
        m = gfmul(m, (uint32_t)__shfl_xor((int)m, o, 64));
    return m;
}

// eight steps over val[LANES]: val[i] followed by val[i + d] whose bytes are pw = x^(8 bytes of d values), squared from step to step.
// Block-uniform call; ends with the result in val[0] and a barrier behind it.
__device__ __forceinline__ void block_tree(uint32_t *val, uint32_t pw, bool table, int j0)
{
    const int lane = threadIdx.x;
#pragma unroll
    for (int s = 0; s < 8; s++) {
        const int d = 1 << s;
        __syncthreads();
        const uint32_t m = table ? pow8_dev.t[j0 + s] : pw;
        if ((lane & (2 * d - 1)) == 0)
            val[lane] = gfmul(val[lane], m) ^ val[lane + d];
        if (!table)
            pw = gfmul(pw, pw);
    }
    __syncthreads();
}

__global__ void __launch_bounds__(LANES) k_crc_segments(const uint8_t *__restrict__ data, size_t stride, uint32_t max_len,
                                                       const long long *__restrict__ lengths, uint32_t *__restrict__ seg, uint32_t nseg_max)
{
    __shared__ __align__(16) uint8_t stage[STAGE_BYTES];
    __shared__ uint32_t tab[256], val[LANES];
    const int lane = threadIdx.x;
    const uint32_t L = item_len(lengths, blockIdx.y, max_len);
    const uint32_t nseg = (uint32_t)segments_of(L, SEGMENT), s = blockIdx.x;
    if (s >= nseg)  // (uniform over the block)
        return;
    const SegGeom g = seg_geom(L, nseg, s, SEGMENT);
    const uint8_t *__restrict__ src = data + (size_t)blockIdx.y * stride + (size_t)g.lo;  // bytes [0, g.n) of it are the segment's
    tab[lane] = table_entry((uint32_t)lane);
    // byte i of the segment goes to position g.pad + i: single bytes up to the first 16-byte boundary of the source, 16-byte loads, single
    // bytes behind the last whole one.  Nothing outside [0, g.n) is read.
    int head = (int)((16u - (uint32_t)((uintptr_t)src & 15u)) & 15u);
    head = head < g.n ? head : g.n;
    const int nvec = (g.n - head) >> 4;
    if (lane < head)
        stage[padded(g.pad + lane)] = src[lane];
    for (int i = head + 16 * nvec + lane; i < g.n; i += LANES)
        stage[padded(g.pad + i)] = src[i];
    {
        typedef uint32_t u4 __attribute__((ext_vector_type(4)));
        const u4 *__restrict__ v = (const u4 *)(src + head);
        constexpr int U = SEGMENT / 16 / LANES;  // 4: all of a lane's loads in flight together
        u4 w[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int k = lane + u * LANES;
            w[u] = k < nvec ? v[k] : u4{0, 0, 0, 0};
        }
        const int at0 = g.pad + head;
        const bool words = (at0 & 3) == 0;  // (uniform) positions that are multiples of 4 stay word aligned and inside one span
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int k = lane + u * LANES;
            if (k < nvec) {
                const int at = at0 + 16 * k;
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    if (words) {
                        *(uint32_t *)(stage + padded(at + 4 * q)) = w[u][q];
                    } else {
#pragma unroll
                        for (int r = 0; r < 4; r++)
                            stage[padded(at + 4 * q + r)] = (uint8_t)(w[u][q] >> (8 * r));
                    }
                }
            }
        }
    }
    __syncthreads();
    // the lane's span: positions [lane SPAN, (lane + 1) SPAN), of which those below g.pad do not exist
    uint32_t wv[SPAN / 4];
    const uint32_t *sp = (const uint32_t *)(stage + lane * PITCH);
#pragma unroll
    for (int q = 0; q < SPAN / 4; q++)
        wv[q] = sp[q];
    uint32_t v = 0;
    const int first = g.pad - lane * SPAN;  // positions of the span below this one are padding (<= 0: none)
    if (first <= 0) {
#pragma unroll
        for (int q = 0; q < SPAN / 4; q++)
#pragma unroll
            for (int r = 0; r < 4; r++)
                v = raw_step(v, (wv[q] >> (8 * r)) & 0xffu, tab);
    } else if (first < SPAN) {
        for (int i = first; i < SPAN; i++)
            v = raw_step(v, (uint32_t)stage[lane * PITCH + i], tab);
    }
    val[lane] = v;
    block_tree(val, 0u, true, ilog2(SPAN));
    if (lane == 0)
        seg[(size_t)blockIdx.y * nseg_max + s] = val[0];
}

template <bool PNGF>
__global__ void __launch_bounds__(LANES) k_crc_finish(const uint32_t *__restrict__ seg, uint32_t nseg_max, uint32_t max_len,
                                                     const long long *__restrict__ lengths, uint32_t seed, uint32_t *__restrict__ crc,
                                                     uint8_t *__restrict__ files, size_t slot, FileHead head, uint8_t *__restrict__ file_lengths)
{
    __shared__ uint32_t val[LANES];
    const int lane = threadIdx.x;
    const uint32_t L = item_len(lengths, blockIdx.x, max_len);
    const uint32_t nseg = (uint32_t)segments_of(L, SEGMENT), per = slice_len(nseg, LANES);
    const uint32_t *__restrict__ mine = seg + (size_t)blockIdx.x * nseg_max;
    uint32_t lo, hi;
    slice_of(nseg, per, lane, LANES, lo, hi);
    const uint32_t xseg = pow8_dev.t[ilog2(SEGMENT)];
    uint32_t acc = 0;
    for (uint32_t s = lo; s < hi; s++)
        acc = gfmul(acc, xseg) ^ mine[s];
    val[lane] = acc;
    const uint32_t pw = xpow8_wave(per * (uint32_t)SEGMENT);  // per <= 2^31 / SEGMENT / LANES
    const uint32_t pl = xpow8_wave(L);
    block_tree(val, pw, false, 0);
    if (lane != 0)
        return;
    const uint32_t c = finish(val[0], seed, pl);
    if (!PNGF) {
        crc[blockIdx.x] = c;
        return;
    }
    uint8_t *f = files + (size_t)blockIdx.x * slot;
#pragma unroll
    for (int i = 0; i < 33; i++)
        f[i] = head.b[i];
    const uint8_t tag[4] = {'I', 'D', 'A', 'T'};
#pragma unroll
    for (int i = 0; i < 4; i++) {
        f[33 + i] = (uint8_t)(L >> (24 - 8 * i));
        f[37 + i] = tag[i];
    }
    uint8_t *t = f + FILE_HEAD + L;
#pragma unroll
    for (int i = 0; i < 4; i++)
        t[i] = (uint8_t)(c >> (24 - 8 * i));
    file_iend(t + 4);
    const uint64_t n = (uint64_t)L + FILE_EXTRA;
    uint8_t *lp = file_lengths + (size_t)blockIdx.x * 8;  // int64, little endian; byte stores: any alignment
#pragma unroll
    for (int k = 0; k < 8; k++)
        lp[k] = (uint8_t)(n >> (8 * k));
}

static inline bool unsupported(int B, size_t max_len) { return B > 65535 || max_len >= ((size_t)1 << 31); }

static uint32_t *carve(Arena &ar, size_t B, size_t max_len) { return ar.take<uint32_t>(B * (size_t)segments_of(max_len, SEGMENT)); }

static inline size_t scratch_bytes(int B, size_t max_len)
{
    if (B <= 0 || max_len == 0 || unsupported(B, max_len))
        return 0;
    return measured([&](Arena &m) { carve(m, (size_t)B, max_len); });
}

// the two launches; the arguments are checked by the callers
template <bool PNGF>
static int launch(const uint8_t *data, int B, size_t stride, size_t max_len, const long long *lengths, uint32_t seed, uint32_t *crc, uint32_t *seg,
                  uint8_t *files, size_t slot, const FileHead &head, uint8_t *file_lengths, hipStream_t st)
{
    const uint32_t nseg_max = (uint32_t)segments_of(max_len, SEGMENT);  // <= 2^17
    hipLaunchKernelGGL(k_crc_segments, dim3(nseg_max, (unsigned)B), dim3(LANES), 0, st, data, stride, (uint32_t)max_len, lengths, seg, nseg_max);
    SRX_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_crc_finish<PNGF>, dim3((unsigned)B), dim3(LANES), 0, st, (const uint32_t *)seg, nseg_max, (uint32_t)max_len, lengths, seed,
                       crc, files, slot, head, file_lengths);
    SRX_CHECK_LAUNCH();
    return SRX_OK;
}

// srx_crc32: the host checks, then the two launches
static int crc32(const void *data, int B, size_t stride, size_t max_len, const void *lengths, uint32_t seed, void *crc, void *ws, size_t wsb,
                 hipStream_t st)
{
    if (!data || !crc || B <= 0 || max_len == 0 || (B > 1 && stride < max_len) || ((uintptr_t)lengths & 7) || ((uintptr_t)crc & 3))
        return SRX_E_INVALID;
    if (unsupported(B, max_len))
        return SRX_E_UNSUPPORTED;
    Arena ar(ws, wsb);
    ar.require(scratch_bytes(B, max_len));
    if (!ar.ok)
        return SRX_E_WORKSPACE;
    uint32_t *seg = carve(ar, (size_t)B, max_len);
    if (!ar.ok)
        return SRX_E_WORKSPACE;
    return launch<false>((const uint8_t *)data, B, stride, max_len, (const long long *)lengths, seed, (uint32_t *)crc, seg, nullptr, 0, FileHead{},
                         nullptr, st);
}

// ---- srx_png_file_*: png::deflate's three launches into the slots' bytes [41, ...), then the CRC of "IDAT" + stream and the container ----
struct FilePlan {
    png::Plan png;
    long long *stream_len;  // [B]: what k_png_offsets writes where srx_png_deflate has the caller's lengths
    uint32_t *seg;
};

static FilePlan carve_file(Arena &ar, size_t B, size_t raw)
{
    FilePlan p;
    p.png = png::carve(ar, B, png::chunks_of(raw));
    p.stream_len = ar.take<long long>(B);
    p.seg = carve(ar, B, png::stream_bound(raw));
    return p;
}

static inline size_t file_bound(int H, int W) { return H > 0 && W > 0 ? png::stream_bound((size_t)H * ((size_t)W + 1)) + FILE_EXTRA : 0; }

static inline size_t file_scratch_bytes(int B, int H, int W)
{
    if (B <= 0 || H <= 0 || W <= 0 || png::unsupported(B, H, W))
        return 0;
    return measured([&](Arena &m) { carve_file(m, (size_t)B, (size_t)H * ((size_t)W + 1)); });
}

// W is the scanline's width in samples; head_w / colour_type: what the IHDR says where that differs (RGB: W = 3 head_w bytes of colour type 2)
template <typename T>
static int png_file(const T *img, int B, int H, int W, void *files_, void *lengths_, void *ws, size_t wsb, hipStream_t st, int head_w = 0,
                    uint8_t colour_type = 0)
{
    uint8_t *files = (uint8_t *)files_, *lengths = (uint8_t *)lengths_;
    if (!img || !files || !lengths || B <= 0 || H <= 0 || W <= 0)
        return SRX_E_INVALID;
    if (png::unsupported(B, H, W))
        return SRX_E_UNSUPPORTED;
    const size_t raw = (size_t)H * ((size_t)W + 1), slot = file_bound(H, W), bound = png::stream_bound(raw);
    Arena ar(ws, wsb);
    ar.require(file_scratch_bytes(B, H, W));
    if (!ar.ok)
        return SRX_E_WORKSPACE;
    const FilePlan p = carve_file(ar, (size_t)B, raw);
    if (!ar.ok)
        return SRX_E_WORKSPACE;
    SRX_TRY(png::launch(img, B, H, W, p.png, files + FILE_HEAD, slot, (uint8_t *)p.stream_len, st));
    // the IDAT's CRC covers its tag and the stream: the stream under the seed crc32("IDAT") (the tag is not in the file yet)
    return launch<true>(files + FILE_HEAD, B, slot, bound, p.stream_len, idat_seed(), nullptr, p.seg, files, slot,
                        file_head((uint32_t)(head_w ? head_w : W), (uint32_t)H, colour_type), lengths, st);
}

}  // namespace crc
}  // namespace srx
#endif
