// srx_items.hpp -- one shift table PER ITEM of a batch (srx_saa_items_*, srx_ibp_items_*).  Included from srx_api.hip behind the
// dispatchers of the shared-table calls, whose route_*, *_check, ibp_need and *_run it calls: everything here is routing on the host plus
// the two per-item forms of kernels that exist.  In a spec or a call of this file sh is [B][N][2]; a table's route is the call's spec
// with sh re-pointed at that table.
//
// Registration measures a table per item (srx_register_* returns [B, N, 2]); the shared-table calls made such a caller leave the batch.
// Here the driver walks the batch in maximal RUNS of consecutive items:
//   - items that all route to "btile" (their tables may all differ): one batch through btile::ibp_items -- the ITEMS instantiations of
//     k_ibp_bfwd / k_ibp_bbwd take the table of item b at frtab + b * stride, each with the range of ITS row tap origins in front of it;
//   - any other run of bytewise-equal tables: the existing driver of its route, as a batch of the run's length (every table equal: this is
//     the shared-table call, launch for launch);
//   - items on "fused" / "composed" with pairwise different tables therefore run one by one.
// shift_and_add does the same with "fused" in the place of "btile" (k_fir_pad_items reads the tap of (item, frame) from a device table).
// The route of a table is decided once per DISTINCT table (route_ibp / route_saa, the records the shared-table calls read), on the host,
// before anything is queued; so is every refusal.  A plan (plan_ibp / plan_saa) holds those records and the runs; the drivers read it.
//
// The table's way to the device: the host builds every item's records with the code of the shared-table call (btile::make_frames,
// fused::make_tap) and btile::ParamUpload carries them, PARAM_WORDS = 960 words by value per launch: an ibp run of n items makes
// ceil(n (4 + 20 N) / 960) such launches (N = 4: one per 11 items), a shift_and_add run ceil(n N sizeof(FrameTap<T>) / 3840).
#pragma once
#include <string>
#include <unordered_map>
#include <vector>

namespace items {

// which table every item has: id[b] indexes the distinct tables in order of first appearance; first[i] is the item that brought table i
struct Tables {
    std::vector<int> id, first;
};
static Tables distinct_tables(const double *sh, int B, int N)
{
    Tables t;
    t.id.resize(B);
    const size_t bytes = (size_t)2 * N * sizeof(double);
    std::unordered_map<std::string, int> seen;
    for (int b = 0; b < B; b++) {
        const char *p = reinterpret_cast<const char *>(sh + (size_t)b * 2 * N);
        if (b > 0 && memcmp(p, p - bytes, bytes) == 0) {
            t.id[b] = t.id[b - 1];
            continue;
        }
        const auto it = seen.emplace(std::string(p, bytes), (int)t.first.size());
        if (it.second)
            t.first.push_back(b);
        t.id[b] = it.first->second;
    }
    return t;
}

struct Run {
    int b0, n, table;
    bool per_item;  // the per-item form of the run's route; else `n` items that share table `table`
};

// maximal runs: consecutive items whose route is the one with a per-item form (`batched[table]`), at most `cap` of them; else equal tables
static std::vector<Run> make_runs(const Tables &t, const std::vector<char> &batched, int B, int cap)
{
    std::vector<Run> runs;
    for (int b = 0; b < B;) {
        int e = b + 1;
        bool equal = true;
        if (batched[t.id[b]]) {
            for (; e < B && e - b < cap && batched[t.id[e]]; e++)
                equal = equal && t.id[e] == t.id[b];
        } else {
            for (; e < B && t.id[e] == t.id[b]; e++) {
            }
        }
        runs.push_back({b, e - b, t.id[b], batched[t.id[b]] && !equal});
        b = e;
    }
    return runs;
}

static inline const char *common_name(const char *have, const char *name) { return !have || strcmp(have, name) == 0 ? name : "mixed"; }

// what a per-item call does, decided before anything is queued
struct Plan {
    int status;                // the first refusal among the tables, else SRX_OK
    std::vector<Route> route;  // per distinct table
    std::vector<Run> runs;
    size_t need;               // the workspace the call must bring
    const char *name;          // what srx_last_path() reports: the runs' common route name, else "mixed"
};

// route(table) of every distinct table, the first refusal, and the runs: `per_item` is the path that has a per-item form, `cap` its longest run
template <typename RouteFn> static Plan plan_runs(const double *sh, int B, int N, Path per_item, int cap, RouteFn route)
{
    Plan p;
    p.status = SRX_OK, p.need = 0, p.name = nullptr;
    const Tables t = distinct_tables(sh, B, N);
    std::vector<char> batched;
    for (int b : t.first) {
        p.route.push_back(route(sh + (size_t)b * 2 * N));
        batched.push_back(p.route.back().path == per_item);
        if (p.route.back().status != SRX_OK && p.status == SRX_OK)
            p.status = p.route.back().status;
    }
    if (p.status != SRX_OK)
        return p;
    p.runs = make_runs(t, batched, B, cap);
    for (const Run &r : p.runs)
        p.name = common_name(p.name, p.route[r.table].name);
    return p;
}

// ---------------------------------------------------------------------------------------
// ibp
// ---------------------------------------------------------------------------------------
static Plan plan_ibp(const IbpSpec &s, int B)
{
    Plan p = plan_runs(s.sh, B, s.N, PATH_BTILE, SRX_MAX_BATCH_PER_LAUNCH, [&](const double *table) {
        IbpSpec t = s;
        t.sh = table;
        return route_ibp(t);
    });
    for (const Run &r : p.runs) {
        size_t need = ibp_need(p.route[r.table], s, r.n);
        if (r.per_item)
            need += btile::items_tab_bytes(r.n, s.N);
        p.need = need > p.need ? need : p.need;
    }
    return p;
}

static size_t ibp_ws_bound(const IbpShape &s, int B, unsigned flags)
{
    return ibp_bound(s, B, flags) + btile::items_tab_bytes(std::max(ibp_chunk_items(B), 1), s.N > 0 ? s.N : 1);
}

template <typename T> static int ibp_dispatch_items(const IbpCall<T> &c)
{
    SRX_TRY(ibp_check(c.s, c.B, c.n_iter, c.lr && c.hr_init && c.hr));
    const Plan p = plan_ibp(c.s, c.B);
    if (p.status != SRX_OK)
        return p.status;
    if (ws_short(c.ws, c.wsb, p.need))
        return SRX_E_WORKSPACE;
    g_last_path = p.name;
    for (const Run &r : p.runs) {
        const double *shr = c.s.sh + (size_t)r.b0 * 2 * c.s.N;
        if (r.per_item) {
            if constexpr (sizeof(T) == 4)
                SRX_TRY(btile::ibp_items(c.chunk(r.b0, r.n, shr)));
            else
                return SRX_E_INVALID;  // (route_ibp gives float32 calls alone this path)
            continue;
        }
        for (int b0 = r.b0; b0 < r.b0 + r.n; b0 += SRX_MAX_BATCH_PER_LAUNCH)  // as ibp_dispatch
            SRX_TRY(ibp_run(p.route[r.table], c.chunk(b0, ibp_chunk_items(r.b0 + r.n - b0), shr)));
    }
    return SRX_OK;
}

// ---------------------------------------------------------------------------------------
// shift_and_add
// ---------------------------------------------------------------------------------------
// k_fir_pad (srx_fused.hpp) with the tap of (item blockIdx.z, frame q) read from a device table [B][N]; the arithmetic is k_fir_pad's
// statement for statement (contraction is decided per statement: the same statements round the same way)
template <typename T, bool ACC>
__global__ void __launch_bounds__(256)
    k_fir_pad_items(const T *__restrict__ up, int H, int W, const fused::FrameTap<T> *__restrict__ tab, int N, int q, T *__restrict__ vpad)
{
    const int Hp = H + 2 * SRX_NPAD, Wp = W + 2 * SRX_NPAD;
    const int qx = blockIdx.x * 64 + threadIdx.x, p = blockIdx.y * 4 + threadIdx.y, b = blockIdx.z;
    if (p >= Hp || qx >= Wp)
        return;
    const fused::FrameTap<T> ft = tab[(size_t)b * N + q];
    const T *u = up + (size_t)b * H * W;
    T acc = 0;
#pragma unroll
    for (int a = 0; a < 4; a++) {
        const int y = min(max(p + ft.oy + a - SRX_NPAD, 0), H - 1);
        T racc = 0;
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const int x = min(max(qx + ft.ox + c - SRX_NPAD, 0), W - 1);
            racc += ft.wx[c] * u[(size_t)y * W + x];
        }
        acc += ft.wy[a] * racc;
    }
    T *o = vpad + (size_t)b * Hp * Wp + (size_t)p * Wp + qx;
    *o = ACC ? *o + acc : acc;
}

// the taps of one per-item run, at the head of the workspace: the carve, and measured, what the queries add for it
template <typename T> static fused::FrameTap<T> *carve_saa_tab(Arena &ar, int B, int N) { return ar.take<fused::FrameTap<T>>((size_t)B * N); }
template <typename T> static inline size_t saa_tab_bytes(int B, int N)
{
    return measured([&](Arena &m) { carve_saa_tab<T>(m, B, N); });
}

static size_t saa_ws_bound(const SaaShape &s, int B)
{
    const int n = s.N > 0 ? s.N : 1, Bc = std::max(saa_chunk_items(B, n), 1);
    return saa_bound(s, B) + (s.eb == 4 ? saa_tab_bytes<float>(Bc, n) : saa_tab_bytes<double>(Bc, n));
}

// fused::saa with one table per item: c.s.sh [B][N][2]; tab: B * N taps of device memory.  The taps go up before the body runs; its own
// refusals cannot follow them, the dispatcher having held the workspace to the bound and the run to one chunk.
template <typename T> static int saa_fused_items(const SaaCall<T> &c, fused::FrameTap<T> *tab)
{
    using namespace fused;
    const int B = c.B, N = c.s.N, f = c.s.f;
    const double *const sh = c.s.sh;
    const hipStream_t st = c.st;
    static_assert(sizeof(FrameTap<T>) % sizeof(int) == 0, "the taps travel as words");
    constexpr int TW = (int)(sizeof(FrameTap<T>) / sizeof(int));
    btile::ParamUpload words{st, reinterpret_cast<int *>(tab)};
    for (size_t i = 0; i < (size_t)B * N; i++) {
        FrameTap<T> ft;
        memset(&ft, 0, sizeof ft);
        make_tap<T>(-sh[2 * i] * f, -sh[2 * i + 1] * f, 0, ft);  // shift(+d): out[r] = in[r - d]
        int ftw[TW];
        memcpy(ftw, &ft, sizeof ft);
        SRX_TRY(words.put(ftw, TW));
    }
    SRX_TRY(words.finish());
    const int H = c.s.h * f, W = c.s.w * f;
    auto fir = [&](int q, dim3 grd, dim3 blk, const T *up, T *pad) -> int {
        if (q == 0)
            SRX_LAUNCH(KID_FIR_PAD, (k_fir_pad_items<T, false>), grd, blk, 0, st, up, H, W, tab, N, q, pad);
        else
            SRX_LAUNCH(KID_FIR_PAD, (k_fir_pad_items<T, true>), grd, blk, 0, st, up, H, W, tab, N, q, pad);
        return SRX_OK;
    };
    return saa_with<T>(fir, c);
}

// (what the call must bring is the shape-only bound: there is no exact query for shift_and_add)
static Plan plan_saa(const SaaSpec &s, int B)
{
    Plan p = plan_runs(s.sh, B, s.N, PATH_FUSED, saa_chunk_items(B, s.N), [&](const double *table) {
        SaaSpec t = s;
        t.sh = table;
        return route_saa(t);
    });
    p.need = saa_ws_bound(s, B);
    return p;
}

template <typename T> static int saa_dispatch_items(const SaaCall<T> &c)
{
    SRX_TRY(saa_check(c.s, c.B, c.lr && c.out));
    const Plan p = plan_saa(c.s, c.B);
    if (p.status != SRX_OK)  // (before the workspace, unlike saa_dispatch: see there)
        return p.status;
    if (ws_short(c.ws, c.wsb, p.need))
        return SRX_E_WORKSPACE;
    g_last_path = p.name;
    // the head of the workspace holds the taps of one per-item run, every run's driver gets the rest
    Arena ar(c.ws, c.wsb);
    fused::FrameTap<T> *tab = carve_saa_tab<T>(ar, saa_chunk_items(c.B, c.s.N), c.s.N);
    const SaaCall<T> rest = c.on(c.lr, (char *)c.ws + ar.off, c.wsb - ar.off);
    for (const Run &r : p.runs) {
        const double *shr = c.s.sh + (size_t)r.b0 * 2 * c.s.N;
        if (r.per_item) {
            SRX_TRY(saa_fused_items<T>(rest.chunk(r.b0, r.n, shr), tab));
            continue;
        }
        for (int b0 = r.b0, bc; b0 < r.b0 + r.n; b0 += bc) {  // as saa_dispatch
            bc = saa_chunk_items(r.b0 + r.n - b0, c.s.N);
            SRX_TRY(saa_run(p.route[r.table], rest.chunk(b0, bc, shr)));
        }
    }
    return SRX_OK;
}

}  // namespace items
