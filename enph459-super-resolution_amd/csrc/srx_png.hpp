// srx_png.hpp -- the zlib stream of an 8-bit greyscale PNG, built on the device (srx_png_deflate_{u8,f32,f64}): img [B, H, W] -> one
// stream per image that inflates to the H scanlines of 1 + W bytes session.write_png_u8 hands to zlib (filter byte 2 = Up, row 0 against
// zeros).  The float forms quantise with quantize_one<T> (srx_prims.hpp: srx_quantize_u8_T's arithmetic) as they read; no uint8 plane exists.
//
// Stream:  78 01 | chunk 0 | chunk 1 | ... | 03 00 | Adler-32 (big endian).  A chunk is CHUNK = 32768 scanline bytes (not row aligned, the
// last one short), coded on its own and starting on a byte boundary (the pigz construction):
//   tokens   literals and distance-1 matches of 3..258 bytes (run length only, like Z_RLE).  A lane owns SPAN = 128 bytes of the chunk and
//            tokenises them alone: a run is cut where a span ends, but it may START on a span's first byte (the byte before it is the last
//            one of the neighbour's span, already in the window); the first byte of a chunk is always a literal.
//   block    one dynamic-Huffman block: the literal/length code of the chunk's own token histogram, at most 15 bits (Moffat-Katajainen
//            lengths, then miniz's "enforce max code size": Kraft sum exactly 1), one distance code of length 1.  Header in the simplest
//            legal form: HLIT = 286, HDIST = 1, all of the code-length symbols 0..15 with 4 bits (16, 17, 18 unused: a complete code), then
//            287 lengths as 4-bit codes: HEADER_BITS = 17 + 57 + 1148 = 1222 for every chunk.
//   end      EOB, an empty stored block (000, pad to a byte, 00 00 FF FF): the next chunk starts byte aligned.
//   stored   a chunk whose coded form is not smaller than n + 5 bytes goes as one stored block (00, n, ~n, the n bytes): a chunk never
//            takes more than n + 5 bytes, hence stream_bound().
//
// Part 1 (plain integer code, host and device; tests/png_host_model.cpp builds it with g++ and codes a file the way the kernels do):
//   tokenize_span, length_symbol, huff_lengths (sorted frequencies -> limited lengths), canonical_codes, put_bits, header_piece,
//   Adler partial sums and their combination, stream_bound.
// Part 2 (device), three launches whatever the samples hold:
//   k_png_analyse<T>  grid (chunks, B), 256 lanes.  Scanline bytes of the chunk -> LDS (spans 132 bytes apart: Raw); Adler partial sums per span; token histogram by LDS
//                     atomics; the used symbols ordered by a rank sort (every lane ranks its own symbols); lane 0 builds the lengths;
//                     every lane counts its span's bits; exclusive scan.  Leaves per chunk: lengths [288], the lanes' bit offsets [256],
//                     {coded bytes, stored?, S1, S2, token bits}.
//   k_png_offsets     grid B, 256 lanes: chunk sizes -> chunk offsets (each lane a contiguous slice of the chunks), lengths[b], the two
//                     header bytes, the final block and the Adler-32 from the chunks' (S1, S2) in integers.
//   k_png_emit<T>     grid (chunks, B): the chunk's bytes again, codes from the stored lengths, and the bits ORed into an LDS window that
//                     is cleared by the kernel, one wave of lanes (64 spans, at most 15 bits a byte) per round, whole bytes copied out
//                     after each round and the open byte carried into the next.  All ORs are on LDS words: nothing in global memory
//                     is ever accumulated into, so the workspace and the output may hold anything on entry.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define SRX_PNG_HD __host__ __device__
#else
#define SRX_PNG_HD
#endif

namespace srx {
namespace png {

constexpr int CHUNK = 32768;       // SRX_PNG_CHUNK: scanline bytes of one chunk
constexpr int SPAN = 128;          // bytes one lane tokenises
constexpr int LANES = CHUNK / SPAN;  // 256
constexpr int NSYM = 286;          // literal/length symbols (HLIT = 286)
constexpr int NSYM_PAD = 288;
constexpr int EOB = 256;
constexpr int MAX_BITS = 15;
constexpr int HEADER_BITS = 17 + 19 * 3 + (NSYM + 1) * 4;  // 1222
constexpr uint32_t ADLER_MOD = 65521;

SRX_PNG_HD inline size_t chunks_of(size_t raw) { return (raw + CHUNK - 1) / CHUNK; }
SRX_PNG_HD inline size_t stream_bound(size_t raw) { return 2 + raw + 5 * chunks_of(raw) + 6; }

// length 3..258 -> symbol 257..285, number of extra bits and their value
SRX_PNG_HD inline void length_symbol(int len, int &sym, int &ebits, int &eval)
{
    const int l = len - 3;
    if (l < 8) {
        sym = 257 + l, ebits = 0, eval = 0;
    } else if (len == 258) {
        sym = 285, ebits = 0, eval = 0;
    } else {
        int lg = 3;
        while ((l >> (lg + 1)) != 0)
            lg++;
        ebits = lg - 2;
        sym = 257 + 4 * ebits + 4 + ((l >> ebits) & 3);
        eval = l & ((1 << ebits) - 1);
    }
}

// the tokens of bytes [s, e) of a chunk `d` (chunk-relative indices): emit(sym, ebits, eval, is_match) once per token, in stream order.
// Byte i continues a run when i > 0 and d[i] == d[i - 1]; a run of L such bytes inside the span is one or more matches of 3..258 and a
// leftover of 1 or 2 literals; L < 3 is literals.  `d` is anything d[i] reads a byte of (a pointer on the host, the kernels' padded LDS image).
template <typename Bytes, typename Emit> SRX_PNG_HD inline void tokenize_span(const Bytes &d, int s, int e, Emit &&emit)
{
    int i = s;
    while (i < e) {
        const int v = d[i];
        if (i > 0 && v == d[i - 1]) {
            int j = i + 1;
            while (j < e && d[j] == v)
                j++;
            int L = j - i;
            while (L >= 3) {
                const int m = L < 258 ? L : 258;
                int sym, eb, ev;
                length_symbol(m, sym, eb, ev);
                emit(sym, eb, ev, true);
                L -= m;
            }
            for (; L > 0; L--)
                emit(v, 0, 0, false);
            i = j;
        } else {
            emit(v, 0, 0, false);
            i++;
        }
    }
}

// Code lengths of n >= 2 symbols whose frequencies stand in `key` in ascending order (key is scratch): len_sorted[k] is the length of the
// symbol of rank k, at most MAX_BITS, Kraft sum exactly 1.  Moffat and Katajainen's in-place minimum-redundancy lengths, then the limiter
// miniz calls "enforce max code size"; the depth before the limiter is returned (tests).  n == 1 gives length 1.  `num` [MAX_BITS + 1] is
// the caller's scratch (LDS in the kernel: a dynamically indexed array of a lane's own would live in scratch memory).
SRX_PNG_HD inline int huff_lengths(uint32_t *key, int n, uint8_t *len_sorted, int *num)
{
    if (n <= 0)
        return 0;
    if (n == 1) {
        len_sorted[0] = 1;
        return 1;
    }
    key[0] += key[1];
    int root = 0, leaf = 2, next;
    for (next = 1; next < n - 1; next++) {
        if (leaf >= n || key[root] < key[leaf]) {
            key[next] = key[root];
            key[root++] = (uint32_t)next;
        } else {
            key[next] = key[leaf++];
        }
        if (leaf >= n || (root < next && key[root] < key[leaf])) {
            key[next] += key[root];
            key[root++] = (uint32_t)next;
        } else {
            key[next] += key[leaf++];
        }
    }
    key[n - 2] = 0;
    for (next = n - 3; next >= 0; next--)
        key[next] = key[key[next]] + 1;
    int avbl = 1, used = 0, dpth = 0;
    root = n - 2;
    next = n - 1;
    while (avbl > 0) {
        while (root >= 0 && (int)key[root] == dpth) {
            used++;
            root--;
        }
        while (avbl > used) {
            key[next--] = (uint32_t)dpth;
            avbl--;
        }
        avbl = 2 * used;
        dpth++;
        used = 0;
    }
    // key[k] is now the unlimited depth of rank k (descending in k); count them, fold what is deeper than MAX_BITS, repair the Kraft sum
    for (int i = 0; i <= MAX_BITS; i++)
        num[i] = 0;
    int deepest = 0;
    for (int k = 0; k < n; k++) {
        const int d = (int)key[k];
        deepest = d > deepest ? d : deepest;
        num[d > MAX_BITS ? MAX_BITS : d]++;
    }
    uint32_t total = 0;
    for (int i = MAX_BITS; i > 0; i--)
        total += (uint32_t)num[i] << (MAX_BITS - i);
    while (total != (1u << MAX_BITS)) {
        num[MAX_BITS]--;
        for (int i = MAX_BITS - 1; i > 0; i--) {
            if (num[i]) {
                num[i]--;
                num[i + 1] += 2;
                break;
            }
        }
        total--;
    }
    // the shortest codes to the most frequent symbols: ranks from the top
    int k = n;
    for (int i = 1; i <= MAX_BITS; i++)
        for (int c = num[i]; c > 0; c--)
            len_sorted[--k] = (uint8_t)i;
    return deepest;
}

// RFC 1951 3.2.2, canonical codes in two steps that the kernel spreads over its lanes.  canonical_bases: the first code of every length
// from count[l] = the number of symbols of length l (count[0] is ignored).  canonical_code: the code of symbol s = the base of its length
// plus the number of earlier symbols of that length, bit-reversed (Huffman codes enter the LSB-first stream with their first bit lowest).
SRX_PNG_HD inline void canonical_bases(const uint32_t *count, uint32_t *base)
{
    uint32_t c = 0;
    base[0] = 0;
    for (int b = 1; b <= MAX_BITS; b++) {
        c = (c + (b > 1 ? count[b - 1] : 0u)) << 1;
        base[b] = c;
    }
}
SRX_PNG_HD inline uint16_t canonical_code(const uint8_t *len, int s, const uint32_t *base)
{
    const int l = len[s];
    if (!l)
        return 0;
    uint32_t v = base[l], r = 0;
    for (int j = 0; j < s; j++)
        v += len[j] == l ? 1u : 0u;
    for (int b = 0; b < l; b++)
        r |= ((v >> b) & 1u) << (l - 1 - b);
    return (uint16_t)r;
}
// all of them, one after the other (the host's form)
SRX_PNG_HD inline void canonical_codes(const uint8_t *len, int nsym, uint16_t *code)
{
    uint32_t count[MAX_BITS + 1], base[MAX_BITS + 1];
    for (int i = 0; i <= MAX_BITS; i++)
        count[i] = 0;
    for (int s = 0; s < nsym; s++)
        count[len[s]]++;
    canonical_bases(count, base);
    for (int s = 0; s < nsym; s++)
        code[s] = canonical_code(len, s, base);
}

// n <= 25 bits of `val` at bit `pos` of an LSB-first stream held in 32-bit words that start cleared; `orw(word *, bits)` is the OR (an LDS
// atomic on the device, where lanes share words)
template <typename Or> SRX_PNG_HD inline void put_bits(uint32_t *words, uint32_t pos, uint32_t val, int n, Or &&orw)
{
    const uint32_t w = pos >> 5, sh = pos & 31u;
    orw(words + w, val << sh);
    if (sh + (uint32_t)n > 32u)
        orw(words + w + 1, val >> (32u - sh));
}

// The block header as NSYM + 2 pieces that do not depend on each other: piece 0 is the 17 bits BFINAL = 0, BTYPE = 10, HLIT = 29, HDIST =
// 0, HCLEN = 15; piece 1 the 19 code-length-code lengths in the order 16 17 18 0 8 7 ... (0 0 0, then sixteen times 4), as three parts
// (k = 1: 9 bits of zeros need no write); pieces 2 + s, s = 0..286: the length of symbol s (s = 286: the distance code, 1) as its 4-bit
// code, which is the length itself bit-reversed.
SRX_PNG_HD inline uint32_t rev4(uint32_t v) { return ((v & 1u) << 3) | ((v & 2u) << 1) | ((v & 4u) >> 1) | ((v & 8u) >> 3); }
template <typename Or> SRX_PNG_HD inline void header_piece(uint32_t *words, uint32_t pos0, int piece, const uint8_t *len, Or &&orw)
{
    if (piece == 0) {
        put_bits(words, pos0, (2u << 1) | (29u << 3) | (0u << 8) | (15u << 13), 17, orw);
    } else if (piece == 1) {
        // sixteen 3-bit fields holding 4 (binary 100, LSB first: value 4), after the three zero fields: bits 17 + 9 .. 17 + 57
        for (int k = 0; k < 16; k += 8) {
            uint32_t v = 0;
            for (int q = 0; q < 8; q++)
                v |= 4u << (3 * q);
            put_bits(words, pos0 + 17 + 9 + 3 * (uint32_t)k, v, 24, orw);
        }
    } else {
        const int s = piece - 2;
        const uint32_t l = s == NSYM ? 1u : len[s];
        put_bits(words, pos0 + 17 + 57 + 4 * (uint32_t)s, rev4(l), 4, orw);
    }
}

// Adler-32 in parts.  For a segment x[0..n): S1 = sum x[i], S2 = sum (n - i) x[i], both mod 65521.  A segment followed by `after` more bytes
// adds S1 to the stream's first sum and S2 + S1 * after to the second; the stream's Adler-32 is (N + sum2) mod p << 16 | (1 + sum1) mod p.
template <typename Bytes> SRX_PNG_HD inline void adler_span(const Bytes &d, int s, int e, uint32_t &S1, uint32_t &S2)
{
    uint32_t a = 0, b = 0;  // e - s <= SPAN... any span below 2^12 bytes: b < 2^12 * 2^12 * 2^8
    for (int i = s; i < e; i++) {
        a += d[i];
        b += a;
    }
    S1 = a;
    S2 = b;
}
SRX_PNG_HD inline uint32_t adler_weight(uint32_t S1, uint32_t S2, uint64_t after)
{
    return (uint32_t)(((uint64_t)(S2 % ADLER_MOD) + (uint64_t)(S1 % ADLER_MOD) * (after % ADLER_MOD)) % ADLER_MOD);
}
SRX_PNG_HD inline uint32_t adler_final(uint64_t N, uint32_t sum1, uint32_t sum2)
{
    const uint32_t a = (uint32_t)((1u + (uint64_t)sum1) % ADLER_MOD), b = (uint32_t)((N + sum2) % ADLER_MOD);
    return (b << 16) | a;
}

// bytes of a chunk coded as a Huffman block with `token_bits` bits of tokens and an EOB of `eob_len` bits, the empty stored block included
SRX_PNG_HD inline uint32_t coded_bytes(uint32_t token_bits, int eob_len) { return (HEADER_BITS + token_bits + (uint32_t)eob_len + 3 + 7) / 8 + 4; }

}  // namespace png
}  // namespace srx

#if defined(__HIPCC__) && !defined(SRX_PNG_HOST_ONLY)
#include "srx_common.h"
#include "srx_prims.hpp"

namespace srx {
namespace png {

constexpr int ROUNDS = LANES / 64;                                         // one wave of spans per round of the emit
constexpr int WIN_WORDS = (64 * SPAN * MAX_BITS / 8 + (HEADER_BITS + 7) / 8 + 16 + 3) / 4 + 1;  // a round's bits, header, carry, EOB + sync

struct ChunkRec {
    uint32_t bytes;       // of the chunk in the stream
    uint32_t stored;      // 1: one stored block
    uint32_t S1, S2;      // Adler partial sums of the chunk's bytes (mod 65521)
    uint32_t token_bits;  // Huffman form: bits of all tokens, without header and EOB
    uint32_t offset;      // of the chunk behind the two header bytes (k_png_offsets)
};

struct Plan {
    ChunkRec *rec;      // [B chunks]
    uint8_t *len;       // [B chunks][NSYM_PAD]
    uint32_t *laneoff;  // [B chunks][LANES]: exclusive prefix of the lanes' token bits
};

static Plan carve(Arena &ar, size_t B, size_t chunks)
{
    Plan p;
    p.rec = ar.take<ChunkRec>(B * chunks);
    p.len = ar.take<uint8_t>(B * chunks * NSYM_PAD);
    p.laneoff = ar.take<uint32_t>(B * chunks * LANES);
    return p;
}

// The chunk in LDS: four bytes of padding behind every span, so that byte j of the 64 lanes' spans lies 132 bytes apart -- 33 banks, an odd
// number: no two lanes of a wave on one bank (at 128 bytes apart all 64 read the same bank, one after the other).
constexpr int RAW_BYTES = CHUNK + 4 * LANES;
__device__ __forceinline__ int padded(int i) { return i + ((i / SPAN) << 2); }
struct Raw {
    const uint8_t *p;
    __device__ __forceinline__ int operator[](int i) const { return p[padded(i)]; }
};

struct LdsOr {
    __device__ __forceinline__ void operator()(uint32_t *w, uint32_t v) const
    {
        if (v)
            atomicOr(w, v);
    }
};

__device__ __forceinline__ uint8_t sample_u8(uint8_t v) { return v; }
__device__ __forceinline__ uint8_t sample_u8(float v) { return quantize_one(v); }
__device__ __forceinline__ uint8_t sample_u8(double v) { return quantize_one(v); }

// scanline bytes [g0, g0 + n) of one image -> the padded image raw: byte g is row g / (W + 1), column g % (W + 1); column 0 is the filter
// type 2, column c the sample [row, c - 1] minus the one above it (zero above row 0), modulo 256.  Eight bytes of a lane at a time, their
// sixteen loads unconditional (a filter byte and row 0 read a sample that exists and drop it) so that they are all in flight together.
template <typename T> __device__ __forceinline__ void load_chunk(const T *__restrict__ img, int W, uint32_t g0, int n, uint8_t *raw)
{
    constexpr int U = 8;
    const uint32_t W1 = (uint32_t)W + 1u;
    for (int i0 = threadIdx.x; i0 < n; i0 += U * LANES) {
        T cur[U], up[U];
        uint32_t row[U], col[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int i = i0 + u * LANES < n ? i0 + u * LANES : n - 1;  // past the end: the last byte again, not stored
            const uint32_t g = g0 + (uint32_t)i;
            row[u] = g / W1;
            col[u] = g - row[u] * W1;
            const size_t at = (size_t)row[u] * W + (col[u] ? col[u] - 1 : 0u);
            cur[u] = img[at];
            up[u] = img[row[u] ? at - W : at];
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int i = i0 + u * LANES;
            if (i < n) {
                const uint8_t c = sample_u8(cur[u]), a = row[u] ? sample_u8(up[u]) : (uint8_t)0;
                raw[padded(i)] = col[u] ? (uint8_t)(c - a) : (uint8_t)2;
            }
        }
    }
}

// the sum of v over the lanes before this one and over all lanes; `tmp` [LANES] is scratch (barriers inside)
__device__ __forceinline__ uint32_t block_exclusive(uint32_t v, uint32_t *tmp, uint32_t &total)
{
    tmp[threadIdx.x] = v;
    __syncthreads();
    uint32_t before = 0, all = 0;
    for (int j = 0; j < LANES; j++) {
        const uint32_t t = tmp[j];
        all += t;
        before += j < (int)threadIdx.x ? t : 0u;
    }
    total = all;
    __syncthreads();
    return before;
}

template <typename T>
__global__ void __launch_bounds__(LANES) k_png_analyse(const T *__restrict__ img, int H, int W, uint32_t chunks, Plan p)
{
    __shared__ __align__(16) uint8_t raw_lds[RAW_BYTES];
    const Raw raw{raw_lds};
    __shared__ uint32_t hist[NSYM_PAD], key[NSYM_PAD], tmp[LANES], sums[2];
    __shared__ uint16_t order[NSYM_PAD];
    __shared__ uint8_t len[NSYM_PAD], len_sorted[NSYM_PAD];
    __shared__ int nused, num[MAX_BITS + 1];
    const int lane = threadIdx.x;
    const uint32_t c = blockIdx.x, total_raw = (uint32_t)H * ((uint32_t)W + 1u), g0 = c * (uint32_t)CHUNK;
    const int n = (int)(total_raw - g0 < (uint32_t)CHUNK ? total_raw - g0 : (uint32_t)CHUNK);
    const size_t ci = (size_t)blockIdx.y * chunks + c;
    load_chunk(img + (size_t)blockIdx.y * H * W, W, g0, n, raw_lds);
    for (int s = lane; s < NSYM_PAD; s += LANES) {
        hist[s] = s == EOB ? 1u : 0u;
        len[s] = 0;
    }
    if (lane == 0)
        sums[0] = sums[1] = 0, nused = 0;
    __syncthreads();
    const int s0 = lane * SPAN < n ? lane * SPAN : n, e0 = (lane + 1) * SPAN < n ? (lane + 1) * SPAN : n;
    tokenize_span(raw, s0, e0, [&](int sym, int, int, bool) { atomicAdd(&hist[sym], 1u); });
    {
        uint32_t S1, S2;
        adler_span(raw, s0, e0, S1, S2);
        if (S1) {
            atomicAdd(&sums[0], S1);  // 256 spans of at most 128 * 255
            atomicAdd(&sums[1], adler_weight(S1, S2, (uint64_t)(n - e0)));
        }
    }
    __syncthreads();
    // rank sort of the used symbols by (frequency, symbol)
    for (int s = lane; s < NSYM; s += LANES) {
        const uint32_t f = hist[s];
        if (f) {
            int rank = 0;
            for (int j = 0; j < NSYM; j++) {
                const uint32_t fj = hist[j];
                rank += (fj && (fj < f || (fj == f && j < s))) ? 1 : 0;
            }
            key[rank] = f;
            order[rank] = (uint16_t)s;
            atomicAdd(&nused, 1);
        }
    }
    __syncthreads();
    if (lane == 0)
        huff_lengths(key, nused, len_sorted, num);
    __syncthreads();
    for (int k = lane; k < nused; k += LANES)
        len[order[k]] = len_sorted[k];
    __syncthreads();
    uint32_t bits = 0;
    tokenize_span(raw, s0, e0, [&](int sym, int eb, int, bool match) { bits += (uint32_t)len[sym] + (uint32_t)eb + (match ? 1u : 0u); });
    uint32_t token_bits;
    const uint32_t before = block_exclusive(bits, tmp, token_bits);
    p.laneoff[ci * LANES + lane] = before;
    for (int s = lane; s < NSYM_PAD; s += LANES)
        p.len[ci * NSYM_PAD + s] = len[s];
    if (lane == 0) {
        const uint32_t coded = coded_bytes(token_bits, len[EOB]);
        ChunkRec r;
        r.stored = coded >= (uint32_t)n + 5u ? 1u : 0u;
        r.bytes = r.stored ? (uint32_t)n + 5u : coded;
        r.S1 = sums[0] % ADLER_MOD;
        r.S2 = sums[1] % ADLER_MOD;
        r.token_bits = token_bits;
        r.offset = 0;
        p.rec[ci] = r;
    }
}

__global__ void __launch_bounds__(LANES) k_png_offsets(int H, int W, uint32_t chunks, Plan p, uint8_t *__restrict__ streams, size_t slot,
                                                       uint8_t *__restrict__ lengths)
{
    __shared__ uint32_t tmp[LANES], sums[2];
    const int lane = threadIdx.x;
    const uint64_t N = (uint64_t)H * ((uint64_t)W + 1u);
    ChunkRec *rec = p.rec + (size_t)blockIdx.x * chunks;
    const uint32_t per = (chunks + LANES - 1) / LANES;
    const uint32_t c0 = (uint32_t)lane * per < chunks ? (uint32_t)lane * per : chunks, c1 = c0 + per < chunks ? c0 + per : chunks;
    if (lane == 0)
        sums[0] = sums[1] = 0;
    uint32_t mine = 0, a1 = 0, a2 = 0;
    for (uint32_t c = c0; c < c1; c++) {
        mine += rec[c].bytes;  // the stream is below 2^31 + 2^19 bytes
        const uint64_t end = (uint64_t)(c + 1) * CHUNK < N ? (uint64_t)(c + 1) * CHUNK : N;
        a1 = (a1 + rec[c].S1) % ADLER_MOD;
        a2 = (a2 + adler_weight(rec[c].S1, rec[c].S2, N - end)) % ADLER_MOD;
    }
    uint32_t total;
    uint32_t off = block_exclusive(mine, tmp, total);  // (its first barrier also orders the clear of sums)
    atomicAdd(&sums[0], a1);  // 256 values below 65521
    atomicAdd(&sums[1], a2);
    for (uint32_t c = c0; c < c1; c++) {
        rec[c].offset = off;
        off += rec[c].bytes;
    }
    __syncthreads();
    if (lane == 0) {
        uint8_t *out = streams + (size_t)blockIdx.x * slot;
        out[0] = 0x78;
        out[1] = 0x01;
        uint8_t *t = out + 2 + total;
        const uint32_t ad = adler_final(N, sums[0] % ADLER_MOD, sums[1] % ADLER_MOD);
        t[0] = 0x03;
        t[1] = 0x00;
        t[2] = (uint8_t)(ad >> 24);
        t[3] = (uint8_t)(ad >> 16);
        t[4] = (uint8_t)(ad >> 8);
        t[5] = (uint8_t)ad;
        const uint64_t L = (uint64_t)total + 8u;
        uint8_t *lp = lengths + (size_t)blockIdx.x * 8;  // int64, little endian; byte stores: any alignment
        for (int k = 0; k < 8; k++)
            lp[k] = (uint8_t)(L >> (8 * k));
    }
}

template <typename T>
__global__ void __launch_bounds__(LANES) k_png_emit(const T *__restrict__ img, int H, int W, uint32_t chunks, Plan p, uint8_t *__restrict__ streams,
                                                    size_t slot)
{
    __shared__ __align__(16) uint8_t raw_lds[RAW_BYTES];
    const Raw raw{raw_lds};
    __shared__ uint32_t win[WIN_WORDS], laneoff[LANES];
    __shared__ uint32_t count[MAX_BITS + 1], base[MAX_BITS + 1];
    __shared__ uint16_t code[NSYM_PAD];
    __shared__ uint8_t len[NSYM_PAD];
    const int lane = threadIdx.x;
    const uint32_t c = blockIdx.x, total_raw = (uint32_t)H * ((uint32_t)W + 1u), g0 = c * (uint32_t)CHUNK;
    const int n = (int)(total_raw - g0 < (uint32_t)CHUNK ? total_raw - g0 : (uint32_t)CHUNK);
    const size_t ci = (size_t)blockIdx.y * chunks + c;
    const ChunkRec r = p.rec[ci];
    if (lane <= MAX_BITS)
        count[lane] = 0;
    uint8_t *dst = streams + (size_t)blockIdx.y * slot + 2 + r.offset;
    load_chunk(img + (size_t)blockIdx.y * H * W, W, g0, n, raw_lds);
    for (int s = lane; s < NSYM_PAD; s += LANES)
        len[s] = p.len[ci * NSYM_PAD + s];
    laneoff[lane] = p.laneoff[ci * LANES + lane];
    __syncthreads();
    if (r.stored) {  // (uniform over the block)
        if (lane == 0) {
            dst[0] = 0x00;
            dst[1] = (uint8_t)n;
            dst[2] = (uint8_t)(n >> 8);
            dst[3] = (uint8_t)~n;
            dst[4] = (uint8_t)(~n >> 8);
        }
        for (int i = lane; i < n; i += LANES)
            dst[5 + i] = (uint8_t)raw[i];
        return;
    }
    // the codes: symbols counted per length by all lanes, the bases by lane 0, every lane the codes of its own symbols
    for (int s = lane; s < NSYM; s += LANES)
        atomicAdd(&count[len[s]], 1u);
    __syncthreads();
    if (lane == 0)
        canonical_bases(count, base);
    __syncthreads();
    for (int s = lane; s < NSYM; s += LANES)
        code[s] = canonical_code(len, s, base);
    const int s0 = lane * SPAN < n ? lane * SPAN : n, e0 = (lane + 1) * SPAN < n ? (lane + 1) * SPAN : n;
    const uint32_t end_bits = HEADER_BITS + r.token_bits + len[EOB] + 3;  // behind the empty stored block's three header bits
    const uint32_t sync_at = (end_bits + 7) / 8;                         // 00 00 FF FF from this byte; the chunk is sync_at + 4 bytes
    uint32_t carry = 0;
    const LdsOr orw;
    for (int round = 0; round < ROUNDS; round++) {
        const uint32_t R0 = round == 0 ? 0u : HEADER_BITS + laneoff[64 * round];
        const uint32_t R1 = round == ROUNDS - 1 ? 8u * (sync_at + 4) : HEADER_BITS + laneoff[64 * (round + 1)];
        const uint32_t byte0 = R0 >> 3, base = byte0 * 8u;
        const uint32_t words = (R1 - base + 31) / 32 + 1;  // at most WIN_WORDS: a round holds 64 spans of at most 15 bits a byte
        for (uint32_t w = lane; w < words; w += LANES)
            win[w] = w == 0 ? carry : 0u;
        __syncthreads();
        if (round == 0)
            for (int piece = lane; piece < NSYM + 3; piece += LANES)
                header_piece(win, 0, piece, len, orw);
        if ((lane >> 6) == round) {
            uint32_t pos = HEADER_BITS + laneoff[lane] - base;
            tokenize_span(raw, s0, e0, [&](int sym, int eb, int ev, bool match) {
                const int l = len[sym], nb = l + eb + (match ? 1 : 0);  // the distance code is one 0 bit
                put_bits(win, pos, (uint32_t)code[sym] | ((uint32_t)ev << l), nb, orw);
                pos += (uint32_t)nb;
            });
        }
        if (round == ROUNDS - 1 && lane == LANES - 1) {
            put_bits(win, HEADER_BITS + r.token_bits - base, code[EOB], len[EOB], orw);
            put_bits(win, 8u * (sync_at + 2) - base, 0xffffu, 16, orw);
        }
        __syncthreads();
        const uint32_t nout = (R1 >> 3) - byte0;  // whole bytes
        const uint8_t *wb = (const uint8_t *)win;
        for (uint32_t k = lane; k < nout; k += LANES)
            dst[byte0 + k] = wb[k];
        carry = (R1 & 7u) ? wb[nout] : 0u;  // the open byte, first of the next round's window
        __syncthreads();
    }
}

static inline bool unsupported(int B, int H, int W) { return B > 65535 || (size_t)H * ((size_t)W + 1) >= ((size_t)1 << 31); }

static inline size_t scratch_bytes(int B, int H, int W)
{
    if (B <= 0 || H <= 0 || W <= 0 || unsupported(B, H, W))
        return 0;
    return measured([&](Arena &m) { carve(m, (size_t)B, chunks_of((size_t)H * ((size_t)W + 1))); });
}

// the three launches: the streams at `streams + b * slot`, their lengths as int64 at `lengths + 8 b` (srx_png_file_* passes the slots of
// its files, 41 bytes in, and eight bytes of its workspace)
template <typename T>
static int launch(const T *img, int B, int H, int W, const Plan &p, uint8_t *streams, size_t slot, uint8_t *lengths, hipStream_t st)
{
    const size_t chunks = chunks_of((size_t)H * ((size_t)W + 1));
    const dim3 grid((unsigned)chunks, (unsigned)B);  // chunks <= 65536
    hipLaunchKernelGGL(k_png_analyse<T>, grid, dim3(LANES), 0, st, img, H, W, (uint32_t)chunks, p);
    SRX_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_png_offsets, dim3((unsigned)B), dim3(LANES), 0, st, H, W, (uint32_t)chunks, p, streams, slot, lengths);
    SRX_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_png_emit<T>, grid, dim3(LANES), 0, st, img, H, W, (uint32_t)chunks, p, streams, slot);
    SRX_CHECK_LAUNCH();
    return SRX_OK;
}

// srx_png_deflate_*: the host checks, then the three launches
template <typename T> static int deflate(const T *img, int B, int H, int W, void *streams_, void *lengths_, void *ws, size_t wsb, hipStream_t st)
{
    uint8_t *streams = (uint8_t *)streams_, *lengths = (uint8_t *)lengths_;
    if (!img || !streams || !lengths || B <= 0 || H <= 0 || W <= 0)
        return SRX_E_INVALID;
    if (unsupported(B, H, W))
        return SRX_E_UNSUPPORTED;
    const size_t raw = (size_t)H * ((size_t)W + 1);
    Arena ar(ws, wsb);
    ar.require(scratch_bytes(B, H, W));
    if (!ar.ok)
        return SRX_E_WORKSPACE;
    const Plan p = carve(ar, (size_t)B, chunks_of(raw));
    if (!ar.ok)
        return SRX_E_WORKSPACE;
    return launch(img, B, H, W, p, streams, stream_bound(raw), lengths, st);
}

}  // namespace png
}  // namespace srx
#endif
