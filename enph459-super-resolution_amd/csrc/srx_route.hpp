// srx_route.hpp -- the implementations of the mosaic formulation (srx_mosaic.hpp) as ONE table: which of them a call takes, what each
// carves from the workspace, and the driver that prepares the call and runs the one chosen.  Included after every implementation header;
// a new implementation is a header with shape_admits / eligible / iterate, a dims bound and a carve (its workspace layout as ONE function:
// iterate runs it on the call's arena with the call's counts, tabs_bytes measures it on a counting arena with the shape-only bound of
// those counts), a row here and a case in ibp()'s switch.  A kernel on 64 x 64 register blocks builds on srx_block.hpp (namespace blk: transpose,
// recursion, pad forms, blurs -- one source for float and double) and adds none of that arithmetic of its own.
#pragma once
#include "srx_mosaic.hpp"
#include "srx_patch.hpp"
#include "srx_ztile.hpp"
#include "srx_dtile.hpp"
#include "srx_ctile.hpp"
#include "srx_atile.hpp"
#include "srx_stile.hpp"

namespace srx {
namespace mosaic {

enum Impl { IMPL_TILES = 0, IMPL_PATCH = 1, IMPL_ZTILE = 2, IMPL_DTILE = 3, IMPL_CTILE = 4, IMPL_ATILE = 5, IMPL_STILE = 6 };

// Exactly one implementation runs per call, and it carves only what it needs (tabs_bytes) behind the tables all of them use (ws_common).
struct ImplRow {
    Impl id;
    const char *name;                                // what srx_last_path() reports
    bool (*shape_admits)(const IbpShape &);          // may a call of this shape EVER take it (the shape-only workspace bound's question);
                                                     // each header's eligible() asks its own first, so bound and dispatch cannot disagree
    bool (*eligible)(const IbpSpec &);               // does THIS call take it: its tables and its flags are in the spec
    size_t (*tabs_bytes)(const IbpShape &, int B);   // the implementation's carve, measured at its dims bound
};

// (thin wrappers, not conditions of patch::eligible itself: stile::eligible calls that and must not inherit the flag exclusions -- a
// float64 patch batch under SRX_FLAG_DIAG_WIDE_WINDOWS takes stile)
static inline bool patch_row_eligible(const IbpSpec &s) { return !(s.flags & (SRX_FLAG_TILES | SRX_FLAG_DIAG_WIDE_WINDOWS)) && patch::eligible(s); }
// a common fraction > 0: k_ibp_dtile's one launch per iteration on the frames it takes (75 us on 3072 x 4096 against the 86 of the
// two-launch window kernels, whose G plane is a round trip through HBM), those kernels on every other shape (or on request)
static inline bool dtile_row_eligible(const IbpSpec &s) { return !(s.flags & SRX_FLAG_DIAG_TWO_LAUNCH) && dtile::eligible(s); }
static inline bool tiles_shape_admits(const IbpShape &) { return true; }
static inline bool tiles_eligible(const IbpSpec &) { return true; }

// in priority order; the last row takes every call the others leave
static const ImplRow impl_table[] = {
    {IMPL_PATCH, "patch", patch::shape_admits, patch_row_eligible, patch::tabs_bytes},
    {IMPL_STILE, "stile", stile::shape_admits, stile::eligible, stile::tabs_bytes},
    {IMPL_CTILE, "ctile", ctile::shape_admits, ctile::eligible, ctile::tabs_bytes},
    {IMPL_ZTILE, "ztile", ztile::shape_admits, ztile::eligible, ztile::tabs_bytes},
    {IMPL_DTILE, "dtile", dtile::shape_admits, dtile_row_eligible, dtile::tabs_bytes},
    {IMPL_ATILE, "atile", atile::shape_admits, atile::eligible, atile::tabs_bytes},
    {IMPL_TILES, "mosaic", tiles_shape_admits, tiles_eligible, tiles_bytes},
};

static inline const ImplRow &choose_impl(const IbpSpec &s)
{
    const ImplRow *r = impl_table;
    while (!r->eligible(s))
        r++;
    return *r;
}

// without the shift table and the PSF the implementation is not known: the largest of those the shape admits
static inline size_t ibp_ws(const IbpShape &s, int B)
{
    size_t m = 0;
    for (const ImplRow &r : impl_table)
        if (r.shape_admits(s))
            m = std::max(m, r.tabs_bytes(s, B));
    return ws_common(s, B) + m;
}

// ... and with them: exactly what the call will carve
static inline size_t ibp_ws_for(const ImplRow &impl, const IbpShape &s, int B) { return ws_common(s, B) + impl.tabs_bytes(s, B); }

// S: the type of the LR samples, T or uint8_t (srx_ibp_u8lr_*).  Only the table building reads the frames (k_mosaic_build in common_prep,
// the patch path's own build), so every implementation below is the same for either.
template <typename T, typename S = T> static int ibp(const ImplRow &impl, const IbpCall<T, S> &call)
{
    const IbpSpec &s = call.s;
    const T *const hr_init = call.hr_init;
    T *const hr = call.hr;
    double *const errors = call.errors;
    const int n_iter = call.n_iter;
    const hipStream_t st = call.st;
    if (n_iter == 0 && hr != hr_init && hipMemcpyAsync(hr, hr_init, (size_t)call.B * s.H * s.W * sizeof(T), hipMemcpyDeviceToDevice, st) != hipSuccess)
        return SRX_E_HIP;
    if (n_iter == 0)
        return SRX_OK;
    // a batch of patches on a full phase grid: the patch path builds its operand planes straight from the LR frames
    bool own_build = false;
    if (impl.id == IMPL_PATCH) {
        AxisPlan py, px;
        own_build = plan_axis(s.N, s.sh, 0, s.f, py) && plan_axis(s.N, s.sh, 1, s.f, px) && patch::builds_itself(py, px, s.N, s.f, s.flags);
    }
    Arena ar(call.ws, call.wsb);
    Common<T> c;
    SRX_TRY((common_prep<T, S>(c, own_build, call, ar, 0, s.H)));
    switch (impl.id) {  // (the float32-only / float64-only drivers are not templates: eligible() admits them for their own type alone)
    case IMPL_STILE:  // float64 patches with a common fraction > 0: two launches per iteration on strips
        if constexpr (sizeof(T) == 8)
            return stile::iterate<T>(c, hr_init, hr, n_iter, errors, ar, st);
        break;
    case IMPL_CTILE:  // integer HR shifts on a large frame, rows along the registers and columns along the lanes (float64; float32 on request)
        return ctile::iterate<T>(c, hr_init, hr, n_iter, errors, ar, st);
    case IMPL_PATCH:  // a 256 x 256 patch fits one compute unit: every iteration in one launch, no intermediate planes
        if constexpr (sizeof(T) == 4)
            return patch::iterate(c, hr_init, hr, n_iter, errors, ar, st);
        break;
    case IMPL_DTILE:  // a common fraction > 0 on a large frame: one launch per iteration over overlapping register-resident windows
        if constexpr (sizeof(T) == 4)
            return dtile::iterate(c, hr_init, hr, n_iter, errors, ar, st);
        break;
    case IMPL_ZTILE:  // integer HR shifts on a large frame: one launch per iteration over CU-resident tiles
        if constexpr (sizeof(T) == 4)
            return ztile::iterate(c, hr_init, hr, n_iter, errors, ar, st);
        break;
    case IMPL_ATILE:  // the remaining float32 frames with a rank-1 PSF: two launches per iteration on 2 x 2-wave windows
        if constexpr (sizeof(T) == 4)
            return atile::iterate(c, hr_init, hr, n_iter, errors, ar, st);
        break;
    case IMPL_TILES:
        break;
    }
    return iterate<T>(c, hr_init, hr, n_iter, errors, ar, st);  // srx_mosaic.hpp's own tile kernels
}

}  // namespace mosaic
}  // namespace srx
