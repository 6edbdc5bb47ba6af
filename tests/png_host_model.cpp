// png_host_model.cpp -- the host-compilable part of csrc/srx_png.hpp run the way the kernels run it (tests/test_png_host.py builds this
// with g++ -fsanitize=address,undefined): a file of PNG scanline bytes -> the zlib stream srx_png_deflate_* would write for them.
//   png_host_model IN OUT [SPAN]     SPAN: bytes one "lane" tokenises (default: the kernels' 128)
// Every chunk goes through the same steps as k_png_analyse / k_png_offsets / k_png_emit: spans tokenised one by one into a histogram, the
// used symbols ordered by (frequency, symbol), huff_lengths, the spans' bit counts and their exclusive prefix, the stored decision, the
// header pieces and every span's tokens put at its own bit offset into cleared words, the Adler parts combined in integers.
// Prints one line: chunks, stored chunks, the deepest unlimited code, the longest limited one, stream bytes.
#include <cstdio>
#include <cstdlib>
#include <vector>

#define SRX_PNG_HOST_ONLY
#include "srx_png.hpp"

using namespace srx::png;

int main(int argc, char **argv)
{
    if (argc < 3) {
        fprintf(stderr, "usage: %s IN OUT [SPAN]\n", argv[0]);
        return 2;
    }
    const int span = argc > 3 ? atoi(argv[3]) : SPAN;
    if (span < 1 || span > 4096) {
        fprintf(stderr, "SPAN must be in 1..4096\n");
        return 2;
    }
    FILE *fi = fopen(argv[1], "rb");
    if (!fi)
        return 2;
    std::vector<uint8_t> rawv;
    {
        uint8_t buf[65536];
        size_t got;
        while ((got = fread(buf, 1, sizeof buf, fi)) > 0)
            rawv.insert(rawv.end(), buf, buf + got);
        fclose(fi);
    }
    const size_t N = rawv.size();
    if (!N)
        return 2;
    const size_t chunks = chunks_of(N);
    std::vector<uint8_t> out(stream_bound(N));  // exactly the slot: a byte past it is the sanitizer's to report
    size_t at = 0;
    out[at++] = 0x78;
    out[at++] = 0x01;
    const auto orw = [](uint32_t *w, uint32_t v) { *w |= v; };
    uint32_t sum1 = 0, sum2 = 0;
    int stored_chunks = 0, deepest = 0, longest = 0;
    for (size_t c = 0; c < chunks; c++) {
        // a copy of exactly the chunk's bytes: a read in front of or behind it is the sanitizer's to report
        const int n = (int)(N - c * CHUNK < (size_t)CHUNK ? N - c * CHUNK : (size_t)CHUNK);
        std::vector<uint8_t> chunk(rawv.begin() + c * CHUNK, rawv.begin() + c * CHUNK + n);
        const uint8_t *d = chunk.data();
        const int lanes = (n + span - 1) / span;
        std::vector<uint32_t> hist(NSYM_PAD, 0), key(NSYM_PAD, 0);
        std::vector<uint16_t> order(NSYM_PAD, 0), code(NSYM_PAD, 0);
        std::vector<uint8_t> len(NSYM_PAD, 0), len_sorted(NSYM_PAD, 0);
        hist[EOB] = 1;
        uint32_t c1 = 0, c2 = 0;
        for (int l = 0; l < lanes; l++) {
            const int s0 = l * span, e0 = (l + 1) * span < n ? (l + 1) * span : n;
            tokenize_span(d, s0, e0, [&](int sym, int, int, bool) { hist[sym]++; });
            uint32_t S1, S2;
            adler_span(d, s0, e0, S1, S2);
            c1 = (c1 + S1) % ADLER_MOD;
            c2 = (c2 + adler_weight(S1, S2, (uint64_t)(n - e0))) % ADLER_MOD;
        }
        int nused = 0;
        for (int s = 0; s < NSYM; s++) {
            if (!hist[s])
                continue;
            int rank = 0;
            for (int j = 0; j < NSYM; j++)
                rank += (hist[j] && (hist[j] < hist[s] || (hist[j] == hist[s] && j < s))) ? 1 : 0;
            key[rank] = hist[s];
            order[rank] = (uint16_t)s;
            nused++;
        }
        key.resize(nused);  // huff_lengths may touch key[0, nused) only
        int num[MAX_BITS + 1];
        const int depth = huff_lengths(key.data(), nused, len_sorted.data(), num);
        deepest = depth > deepest ? depth : deepest;
        for (int k = 0; k < nused; k++) {
            len[order[k]] = len_sorted[k];
            longest = len_sorted[k] > longest ? len_sorted[k] : longest;
        }
        std::vector<uint32_t> laneoff(lanes + 1, 0);
        for (int l = 0; l < lanes; l++) {
            const int s0 = l * span, e0 = (l + 1) * span < n ? (l + 1) * span : n;
            uint32_t bits = 0;
            tokenize_span(d, s0, e0, [&](int sym, int eb, int, bool match) { bits += (uint32_t)len[sym] + (uint32_t)eb + (match ? 1u : 0u); });
            laneoff[l + 1] = laneoff[l] + bits;
        }
        const uint32_t token_bits = laneoff[lanes], coded = coded_bytes(token_bits, len[EOB]);
        const size_t end = (c + 1) * (size_t)CHUNK < N ? (c + 1) * (size_t)CHUNK : N;
        sum1 = (sum1 + c1) % ADLER_MOD;
        sum2 = (sum2 + adler_weight(c1, c2, (uint64_t)(N - end))) % ADLER_MOD;
        if (coded >= (uint32_t)n + 5u) {
            stored_chunks++;
            out[at++] = 0;
            out[at++] = (uint8_t)n;
            out[at++] = (uint8_t)(n >> 8);
            out[at++] = (uint8_t)~n;
            out[at++] = (uint8_t)(~n >> 8);
            for (int i = 0; i < n; i++)
                out[at++] = d[i];
            continue;
        }
        canonical_codes(len.data(), NSYM, code.data());
        std::vector<uint32_t> words((coded + 3) / 4 + 1, 0);
        for (int piece = 0; piece < NSYM + 3; piece++)
            header_piece(words.data(), 0, piece, len.data(), orw);
        for (int l = lanes - 1; l >= 0; l--) {  // (any order: every span knows its own offset)
            const int s0 = l * span, e0 = (l + 1) * span < n ? (l + 1) * span : n;
            uint32_t pos = HEADER_BITS + laneoff[l];
            tokenize_span(d, s0, e0, [&](int sym, int eb, int ev, bool match) {
                const int ln = len[sym], nb = ln + eb + (match ? 1 : 0);
                put_bits(words.data(), pos, (uint32_t)code[sym] | ((uint32_t)ev << ln), nb, orw);
                pos += (uint32_t)nb;
            });
        }
        put_bits(words.data(), HEADER_BITS + token_bits, code[EOB], len[EOB], orw);
        const uint32_t sync_at = (HEADER_BITS + token_bits + len[EOB] + 3 + 7) / 8;
        put_bits(words.data(), 8u * (sync_at + 2), 0xffffu, 16, orw);
        for (uint32_t k = 0; k < coded; k++)
            out[at++] = (uint8_t)(words[k >> 2] >> (8 * (k & 3)));
    }
    const uint32_t ad = adler_final(N, sum1, sum2);
    out[at++] = 0x03;
    out[at++] = 0x00;
    out[at++] = (uint8_t)(ad >> 24);
    out[at++] = (uint8_t)(ad >> 16);
    out[at++] = (uint8_t)(ad >> 8);
    out[at++] = (uint8_t)ad;
    FILE *fo = fopen(argv[2], "wb");
    if (!fo || fwrite(out.data(), 1, at, fo) != at)
        return 2;
    fclose(fo);
    printf("chunks %zu stored %d deepest %d longest %d bytes %zu\n", chunks, stored_chunks, deepest, longest, at);
    return 0;
}
