// crc_host_model.cpp -- the host-compilable part of csrc/srx_crc.hpp run the way the kernels run it (tests/test_crc_host.py builds this with
// g++ -fsanitize=address,undefined): a file of bytes -> the CRC-32 srx_crc32 would store for them.
//   crc_host_model IN SEED [SPAN SEGMENT]     SEED: zlib's (decimal); SPAN, SEGMENT: default the kernels' 64 and 16384; SEGMENT / SPAN
//                                             must be a power of two (the lanes of a tree)
// The order is the kernels': segments counted from the message's end (k_crc_segments' seg_geom), each reduced span by span from its end
// with the spans in front of the data left out, the spans' values combined by a log-step tree in x^(8 SPAN 2^s); then k_crc_finish: 256
// slices of the segments folded by Horner in x^(8 SEGMENT), the slices by a tree in x^(8 SEGMENT per) and its squares, the seed term last.
// Prints one line: crc, segments.
#include <cstdio>
#include <cstdlib>
#include <vector>

#define SRX_CRC_HOST_ONLY
#include "srx_crc.hpp"

using namespace srx::crc;

// val[i] followed by val[i + d], whose bytes are pw = x^(8 bytes of d values) at step d, squared from step to step: the result in val[0]
static void tree(std::vector<uint32_t> &val, uint32_t pw)
{
    const size_t n = val.size();
    for (size_t d = 1; d < n; d *= 2) {
        for (size_t i = 0; i + d < n; i += 2 * d)
            val[i] = gfmul(val[i], pw) ^ val[i + d];
        pw = gfmul(pw, pw);
    }
}

int main(int argc, char **argv)
{
    if (argc != 3 && argc != 5) {
        fprintf(stderr, "usage: %s IN SEED [SPAN SEGMENT]\n", argv[0]);
        return 2;
    }
    const uint32_t seed = (uint32_t)strtoul(argv[2], nullptr, 10);
    const int span = argc > 3 ? atoi(argv[3]) : SPAN, segment = argc > 3 ? atoi(argv[4]) : SEGMENT;
    if (span < 1 || segment < span || segment % span || segment > (1 << 20)) {
        fprintf(stderr, "SPAN >= 1 must divide SEGMENT <= 2^20\n");
        return 2;
    }
    const int lanes = segment / span;
    if (lanes & (lanes - 1)) {
        fprintf(stderr, "SEGMENT / SPAN must be a power of two\n");
        return 2;
    }
    FILE *fi = fopen(argv[1], "rb");
    if (!fi)
        return 2;
    std::vector<uint8_t> msg;
    {
        uint8_t buf[65536];
        size_t got;
        while ((got = fread(buf, 1, sizeof buf, fi)) > 0)
            msg.insert(msg.end(), buf, buf + got);
        fclose(fi);
    }
    const uint64_t L = msg.size();
    std::vector<uint32_t> tab(256);
    for (uint32_t i = 0; i < 256; i++)
        tab[i] = table_entry(i);
    const uint32_t *pow8 = POW8.t;

    // k_crc_segments
    const uint64_t nseg = segments_of(L, (uint64_t)segment);
    std::vector<uint32_t> seg(nseg);
    for (uint64_t s = 0; s < nseg; s++) {
        const SegGeom g = seg_geom(L, nseg, s, segment);
        // a copy of exactly the segment's bytes: a read in front of or behind it is the sanitizer's to report
        std::vector<uint8_t> bytes(msg.begin() + g.lo, msg.begin() + g.lo + g.n);
        std::vector<uint32_t> val(lanes);
        for (int l = 0; l < lanes; l++) {
            const int64_t p0 = (int64_t)l * span < g.pad ? g.pad : (int64_t)l * span, p1 = (int64_t)(l + 1) * span;  // positions
            val[l] = p0 < p1 ? raw_span(bytes.data(), p0 - g.pad, p1 - g.pad, tab) : 0u;
        }
        tree(val, xpow8(pow8, (uint64_t)span));
        seg[s] = val[0];
    }

    // k_crc_finish
    const uint32_t per = slice_len(nseg, LANES), xseg = xpow8(pow8, (uint64_t)segment);
    std::vector<uint32_t> val(LANES);
    for (int l = 0; l < LANES; l++) {
        uint32_t lo, hi, acc = 0;
        slice_of(nseg, per, l, LANES, lo, hi);
        for (uint32_t s = lo; s < hi; s++)
            acc = gfmul(acc, xseg) ^ seg[s];
        val[l] = acc;
    }
    tree(val, xpow8(pow8, (uint64_t)per * (uint64_t)segment));
    const uint32_t crc = finish(val[0], seed, xpow8(pow8, L));
    printf("crc %u segments %llu\n", crc, (unsigned long long)nseg);
    return 0;
}
