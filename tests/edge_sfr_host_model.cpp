// edge_sfr_host_model.cpp -- the host-compilable part of csrc/srx_sfr.hpp run the way the kernels run it (tests/test_edge_sfr_host.py builds
// this with g++ -fsanitize=address,undefined -ffp-contract=off): what srx_edge_sfr_* writes for one ROI.
//   edge_sfr_host_model sfr IN SIDE SIGMA     IN: int32 H, int32 W, then H W float64 samples.  Prints "status S", "summary" + 16 values,
//                                             "esf" + 2 x 80 values, "mtf" + 2 x 40 values (%.17g: the doubles round-trip)
//   edge_sfr_host_model percentile IN         IN: int64 n, then n float64 (non-negative).  Prints the 85th percentile by the radix selection
//   edge_sfr_host_model selftest              the 128-bit helpers against the compiler's __int128
// The steps are those of k_sfr_smooth0 / smooth1 / sobel / fit / bins / tail, with the kernels' order of additions: a histogram per digit, the
// integer sums, per row group and bin the pixels in raster order, then the groups in index order.
#include <cstdio>
#include <cstdlib>
#include <vector>

#define SRX_SFR_HOST_ONLY
#include "srx_sfr.hpp"

using namespace srx::sfr;

static double select85(const std::vector<double> &a)
{
    const uint64_t n = a.size();
    double t;
    uint64_t rank = percentile_index(n, t), prefix = 0;
    unsigned equal = 0;
    for (int shift = 56; shift >= 0; shift -= 8) {
        unsigned hist[256] = {0};
        for (uint64_t i = 0; i < n; i++) {
            const uint64_t key = key_of(a[i]);
            if (in_prefix(key, prefix, shift))
                hist[(key >> shift) & 255]++;
        }
        const int d = select_digit(hist, rank);
        equal = hist[d];
        prefix |= (uint64_t)d << shift;
    }
    uint64_t next = ~0ull;
    for (uint64_t i = 0; i < n; i++) {
        const uint64_t key = key_of(a[i]);
        if (key > prefix && key < next)
            next = key;
    }
    const uint64_t upper = (rank + 1 < equal || next == ~0ull) ? prefix : next;
    return lerp(value_of(prefix), value_of(upper), t);
}

static bool read_exact(FILE *f, void *p, size_t bytes) { return fread(p, 1, bytes, f) == bytes; }

static int run_percentile(const char *path)
{
    FILE *f = fopen(path, "rb");
    int64_t n = 0;
    if (!f || !read_exact(f, &n, 8) || n <= 0 || n > (1 << 24))
        return 2;
    std::vector<double> a((size_t)n);
    if (!read_exact(f, a.data(), (size_t)n * 8))
        return 2;
    fclose(f);
    printf("%.17g\n", select85(a));
    return 0;
}

static int run_selftest()
{
    uint64_t x = 0x9e3779b97f4a7c15ull;
    auto next = [&]() {
        x ^= x << 13, x ^= x >> 7, x ^= x << 17;
        return x;
    };
    for (int it = 0; it < 200000; it++) {
        const int sa = (int)(next() % 63) + 1, sb = (int)(next() % 63) + 1, sc = (int)(next() % 63) + 1, sd = (int)(next() % 63) + 1;
        const uint64_t a = next() >> (64 - sa), b = next() >> (64 - sb), c = next() >> (64 - sc), d = next() >> (64 - sd);
        if (sa + sb > 126 || sc + sd > 126)
            continue;
        const __int128 want = (__int128)a * (__int128)b - (__int128)c * (__int128)d;
        const I128 got = sub_i128(mul_u64(a, b), mul_u64(c, d));
        if (got.lo != (uint64_t)want || got.hi != (int64_t)(want >> 64) || i128_to_double(got) != (double)want) {
            fprintf(stderr, "selftest: %llu * %llu - %llu * %llu\n", (unsigned long long)a, (unsigned long long)b, (unsigned long long)c,
                    (unsigned long long)d);
            return 1;
        }
    }
    // halfway cases of the conversion: 2^100 + 2^47 (ties to even: down), + 2^47 + 1 (up), 2^100 + 3 * 2^47 (ties to even: up)
    for (int k = 0; k < 3; k++) {
        const __int128 v = ((__int128)1 << 100) + ((__int128)(k == 2 ? 3 : 1) << 47) + (k == 1 ? 1 : 0);
        for (int sgn = 0; sgn < 2; sgn++) {
            const __int128 w = sgn ? -v : v;
            I128 g;
            g.lo = (uint64_t)w, g.hi = (int64_t)(w >> 64);
            if (i128_to_double(g) != (double)w) {
                fprintf(stderr, "selftest: halfway case %d sign %d\n", k, sgn);
                return 1;
            }
        }
    }
    printf("ok\n");
    return 0;
}

static int run_sfr(const char *path, int side, double sigma)
{
    FILE *f = fopen(path, "rb");
    int32_t hw[2] = {0, 0};
    if (!f || !read_exact(f, hw, 8) || hw[0] <= 0 || hw[1] <= 0 || (int64_t)hw[0] * hw[1] > (1 << 20) || (side != 0 && side != 1) || !(sigma > 0.0))
        return 2;
    const int H = hw[0], W = hw[1], n = H * W;
    std::vector<double> img((size_t)n), a((size_t)n), b((size_t)n), mag((size_t)n);
    if (!read_exact(f, img.data(), (size_t)n * 8))
        return 2;
    fclose(f);
    Taps17 t;
    if (!gaussian_taps(sigma, t))
        return 2;
    for (int i = 0; i < n; i++)
        a[i] = correlate_at(t, 0, i / W, i % W, H, W, [&](int yy, int xx) { return img[(size_t)yy * W + xx]; });
    for (int i = 0; i < n; i++)
        b[i] = correlate_at(t, 1, i / W, i % W, H, W, [&](int yy, int xx) { return a[(size_t)yy * W + xx]; });
    for (int i = 0; i < n; i++)
        mag[i] = sobel_mag_at(i / W, i % W, H, W, [&](int yy, int xx) { return b[(size_t)yy * W + xx]; });

    const double nanv = nan_value();
    double sm[SUMMARY];
    for (int i = 0; i < SUMMARY; i++)
        sm[i] = nanv;
    sm[S_ZERO] = 0.0;
    std::vector<double> esf(2 * MAX_BINS, nanv), mtf(MAX_BINS, nanv);
    int status = ST_OK;
    do {
        const double thr = select85(mag);
        sm[S_THRESHOLD] = thr;
        uint64_t e[6] = {0, 0, 0, 0, 0, 0};
        int r0 = 0x7fffffff, r1 = -1, c0 = 0x7fffffff, c1 = -1;
        for (int i = 0; i < n; i++) {
            if (mag[i] > thr) {
                const uint64_t r = i / W, c = i % W;
                e[0] += 1, e[1] += r, e[2] += c, e[3] += r * r, e[4] += c * c, e[5] += r * c;
                r0 = (int)r < r0 ? (int)r : r0, r1 = (int)r > r1 ? (int)r : r1, c0 = (int)c < c0 ? (int)c : c0, c1 = (int)c > c1 ? (int)c : c1;
            }
        }
        sm[S_N_EDGE] = (double)e[0];
        if (e[0] < 20) {
            status = ST_FEW_EDGE;
            break;
        }
        const int rax = (r1 - r0) >= (c1 - c0);
        sm[S_ROWS_ARE_X] = (double)rax;
        double m_c, b_c, m, lb;
        if (!line_fit(rax ? FitSums{e[0], e[1], e[2], e[3], e[5]} : FitSums{e[0], e[2], e[1], e[4], e[5]}, m_c, b_c)) {
            status = ST_DEGENERATE;
            break;
        }
        sm[S_MC] = m_c, sm[S_BC] = b_c;
        const double norm_c = line_norm(m_c);
        uint64_t s[5] = {0, 0, 0, 0, 0};
        for (int i = 0; i < n; i++) {
            if (mag[i] > thr) {
                const uint64_t r = i / W, c = i % W, u = rax ? r : c, v = rax ? c : r;
                const double d = line_dist((double)u, (double)v, m_c, b_c, norm_c);
                if (side == 0 ? d < 0.0 : d > 0.0)
                    s[0] += 1, s[1] += u, s[2] += v, s[3] += u * u, s[4] += u * v;
            }
        }
        sm[S_N_SIDE] = (double)s[0];
        if (s[0] < 10) {
            status = ST_FEW_SIDE;
            break;
        }
        if (!line_fit(FitSums{s[0], s[1], s[2], s[3], s[4]}, m, lb)) {
            status = ST_DEGENERATE;
            break;
        }
        sm[S_M] = m, sm[S_B] = lb;
        const double norm = line_norm(m);
        double lo = 1e300, hi = -1e300;
        for (int i = 0; i < n; i++) {
            const int r = i / W, c = i % W;
            const double d = line_dist((double)(rax ? r : c), (double)(rax ? c : r), m, lb, norm);
            if (d > -8.0 && d < 10.0)
                lo = d < lo ? d : lo, hi = d > hi ? d : hi;
        }
        if (lo > hi) {
            status = ST_DEGENERATE;
            break;
        }
        sm[S_LO] = lo, sm[S_HI] = hi;
        const int nbin = edge_count(lo, hi) - 1;
        sm[S_NBIN] = (double)nbin;
        sm[S_ANGLE] = edge_angle_deg(m, rax);
        if (nbin < 4) {
            status = ST_FEW_BINS;
            break;
        }
        // the bins: per row group the pixels of a bin in raster order, then the groups in index order
        const int G = bin_groups(H), rp = group_rows(H);
        std::vector<double> part((size_t)G * 2 * MAX_BINS, 0.0);
        for (int y = 0; y < H; y++) {
            double *p = &part[(size_t)(y / rp) * 2 * MAX_BINS];
            for (int x = 0; x < W; x++) {
                const double d = line_dist((double)(rax ? y : x), (double)(rax ? x : y), m, lb, norm);
                if (!(d > -8.0 && d < 10.0))
                    continue;
                for (int i = 0; i < nbin; i++) {
                    if (d >= bin_edge(lo, i) && d < bin_edge(lo, i + 1)) {
                        p[i] += img[(size_t)y * W + x], p[MAX_BINS + i] += 1.0;
                        break;
                    }
                }
            }
        }
        double sum[MAX_BINS], cnt[MAX_BINS], x[MAX_BINS], y[MAX_BINS], wl[MAX_BINS], mt[MAX_BINS / 2], fr[MAX_BINS / 2];
        for (int i = 0; i < nbin; i++) {
            double ss = 0.0, cc = 0.0;
            for (int g = 0; g < G; g++)
                ss += part[(size_t)g * 2 * MAX_BINS + i], cc += part[(size_t)g * 2 * MAX_BINS + MAX_BINS + i];
            sum[i] = ss, cnt[i] = cc;
        }
        int flipped = 0;
        status = esf_from_bins(sum, cnt, nbin, lo, x, y, flipped);
        if (status != ST_OK)
            break;
        sm[S_FLIPPED] = (double)flipped;
        lsf_windowed(x, y, nbin, wl);
        const int nh = nbin / 2;
        double cs[MAX_BINS], sn[MAX_BINS];  // the kernel's twiddle table: the same values as evaluating each where it is used
        for (int r = 0; r < nbin; r++)
            twiddle(r, nbin, cs[r], sn[r]);
        for (int k = 0; k < nh; k++) {
            mt[k] = dft_abs_table(wl, nbin, k, cs, sn);
            if (key_of(mt[k]) != key_of(dft_abs(wl, nbin, k))) {
                fprintf(stderr, "the table form of the DFT differs from the direct one at k = %d\n", k);
                return 1;
            }
        }
        mtf_finish(mt, nh, x, nbin, fr);
        sm[S_MTF50] = mtf_crossing(fr, mt, nh, 0.5), sm[S_MTF10] = mtf_crossing(fr, mt, nh, 0.1);
        for (int i = 0; i < MAX_BINS; i++)
            esf[i] = i < nbin ? x[i] : 0.0, esf[MAX_BINS + i] = i < nbin ? y[i] : 0.0;
        for (int i = 0; i < MAX_BINS / 2; i++)
            mtf[i] = i < nh ? fr[i] : 0.0, mtf[MAX_BINS / 2 + i] = i < nh ? mt[i] : 0.0;
    } while (0);
    if (status != ST_OK && status != ST_FEW_BINS)
        sm[S_ANGLE] = nanv;
    printf("status %d\nsummary", status);
    for (int i = 0; i < SUMMARY; i++)
        printf(" %.17g", sm[i]);
    printf("\nesf");
    for (double v : esf)
        printf(" %.17g", v);
    printf("\nmtf");
    for (double v : mtf)
        printf(" %.17g", v);
    printf("\n");
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 2 && !strcmp(argv[1], "selftest"))
        return run_selftest();
    if (argc == 3 && !strcmp(argv[1], "percentile"))
        return run_percentile(argv[2]);
    if (argc == 5 && !strcmp(argv[1], "sfr"))
        return run_sfr(argv[2], atoi(argv[3]), atof(argv[4]));
    fprintf(stderr, "usage: %s sfr IN SIDE SIGMA | percentile IN | selftest\n", argv[0]);
    return 2;
}
