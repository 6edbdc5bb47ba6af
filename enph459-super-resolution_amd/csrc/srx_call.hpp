// srx_call.hpp -- what an srx_ibp / srx_saa call IS, as records.  Three levels, each a superset of the one before:
//   the shape (IbpShape, SaaShape): all a shape-only question may ask -- the *_workspace_bytes bounds, every shape_admits;
//   the spec (IbpSpec, SaaSpec): + the host tables and the call's flags -- what the route, every eligible() and the exact need
//     depend on.  The batch size plays no part; no device pointer is in it, so nothing that routes or sizes can touch one;
//   the call (IbpCall, SaaCall): + the batch and its buffers -- what a driver runs.
// The flags travel in the spec and nowhere else: whoever reads one (a path-forcing flag in an eligible(), a SRX_FLAG_DIAG_* switch
// several layers below the entry point) reads it from the record it was handed, or from an explicit parameter where there is no call
// (fused::make_kernel7, fused::prefilter2d_*: the primitive entry points pass 0).
#pragma once
#include "srx_common.h"

namespace srx {

struct IbpShape {
    int eb, N, h, w, H, W, f;  // eb: bytes of an element (4 / 8); LR frames [N, h, w], HR plane [H, W]
};
struct IbpSpec : IbpShape {
    const double *sh;  // [N][2], host
    const double *k;   // [kh][kw], host
    int kh, kw;
    unsigned flags;
};
struct SaaShape {
    int eb, N, h, w, f;
};
struct SaaSpec : SaaShape {
    const double *sh;  // [N][2], host
    unsigned flags;
};

// T: the element type of the planes; S: of the LR samples as the caller holds them (T, or uint8_t: srx_*_u8lr_*)
template <typename T, typename S = T> struct IbpCall {
    IbpSpec s;
    const S *lr;
    int B;
    const T *hr_init;
    int n_iter;
    double step;
    T *hr;
    double *errors;  // [B][n_iter], or null
    void *ws;
    size_t wsb;
    hipStream_t st;
    // items [b0, b0 + bc) of the batch, on the same workspace (chunks run in stream order); sh: their shift table
    IbpCall chunk(int b0, int bc, const double *sh) const
    {
        IbpCall c = *this;
        c.s.sh = sh, c.B = bc, c.lr = lr + (size_t)b0 * s.N * s.h * s.w, c.hr_init = hr_init + (size_t)b0 * s.H * s.W, c.hr = hr + (size_t)b0 * s.H * s.W;
        c.errors = errors ? errors + (size_t)b0 * n_iter : nullptr;
        return c;
    }
    IbpCall chunk(int b0, int bc) const { return chunk(b0, bc, s.sh); }
    // the same call on other frames (the staged copy of uint8 samples) and the workspace behind them
    template <typename S2> IbpCall<T, S2> on(const S2 *frames, void *ws2, size_t wsb2) const
    {
        return {s, frames, B, hr_init, n_iter, step, hr, errors, ws2, wsb2, st};
    }
};

template <typename T, typename S = T> struct SaaCall {
    SaaSpec s;
    const S *lr;
    int B;
    T *out;
    void *ws;
    size_t wsb;
    hipStream_t st;
    SaaCall chunk(int b0, int bc, const double *sh) const
    {
        SaaCall c = *this;
        c.s.sh = sh, c.B = bc, c.lr = lr + (size_t)b0 * s.N * s.h * s.w, c.out = out + (size_t)b0 * s.h * s.f * s.w * s.f;
        return c;
    }
    SaaCall chunk(int b0, int bc) const { return chunk(b0, bc, s.sh); }
    template <typename S2> SaaCall<T, S2> on(const S2 *frames, void *ws2, size_t wsb2) const { return {s, frames, B, out, ws2, wsb2, st}; }
};

}  // namespace srx
