// srx_api.hip -- C ABI of libsrx.so (include/srx.h): primitive entry points, the composed
// (literal, per-frame) SAA / IBP built from the primitive kernels, and the route of a call:
// route_ibp() decides once which of composed / fused / btile / mosaic (and which row of
// srx_route.hpp's table of mosaic implementations) takes an srx_ibp call, route_saa() which of
// composed / fused / mosaic takes an srx_saa call; the call, its per-item form, a plan, the exact
// workspace query and the host's route queries all read that one record.
#include <cstdio>
#include <cstring>

#include "srx_prims.hpp"
#include "srx_fused.hpp"
#include "srx_route.hpp"  // srx_mosaic.hpp and every implementation built on it
#include "srx_btile.hpp"
#include "srx_metrics.hpp"
#include "srx_psf.hpp"
#include "srx_register.hpp"
#include "srx_mean.hpp"
#include "srx_png.hpp"
#include "srx_crc.hpp"
#include "srx_bayer.hpp"
#include "srx_patches.hpp"

using namespace srx;

static thread_local const char *g_last_path = "none";

namespace srx {
Profiler &profiler()
{
    static Profiler p;
    return p;
}
}  // namespace srx

static const char *const g_kernel_names[KID_COUNT] = {
#define X(id, name) name,
    SRX_KERNEL_LIST(X)
#undef X
};

// One image plane (with SciPy's 12-sample pad on every side) and one item's N frames must stay below 2 GiB: the kernels index a plane with
// 32-bit offsets and describe it to the memory unit as a buffer resource (32-bit byte count).  The batch is not limited (items are
// re-based with 64-bit arithmetic); the reference's largest image is 3072 x 4096 (100 MB in float64).
static inline bool plane_fits(size_t eb, int N, int h, int w, int H, int W)
{
    const size_t lim = (size_t)1 << 31;
    return ((size_t)H + 2 * SRX_NPAD) * ((size_t)W + 2 * SRX_NPAD) * eb < lim && (size_t)(N > 0 ? N : 1) * h * w * eb < lim;
}

// ---------------------------------------------------------------------------------------
// composed building blocks
// ---------------------------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(256) k_copy_items(const T *__restrict__ in, size_t in_item_stride, size_t n,
                                                    T *__restrict__ out)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n)
        out[(size_t)blockIdx.y * n + i] = in[(size_t)blockIdx.y * in_item_stride + i];
}

template <typename T> static int copy_items(const T *in, size_t stride, int B, size_t n, T *out, hipStream_t st)
{
    hipLaunchKernelGGL(k_copy_items<T>, dim3((unsigned)((n + 255) / 256), B), dim3(256), 0, st, in, stride, n, out);
    SRX_CHECK_LAUNCH();
    return SRX_OK;
}

// scipy.ndimage.shift(order 3, 'nearest') sampled at rows i*istep, cols j*istep (istep=1: the full image)
template <typename T>
static int shift_sampled(const T *in, int B, int H, int W, double sy, double sx, int istep, int Ho, int Wo, T *out,
                         bool accumulate, T *pad, T *scr, AxisTap<T> *ty, AxisTap<T> *tx, bool taps_ready,
                         hipStream_t st, unsigned flags)  // flags: of the ibp / saa call this runs in, 0 in a primitive entry point
{
    const int Hp = H + 2 * SRX_NPAD, Wp = W + 2 * SRX_NPAD;
    SRX_TRY(pad_edge(in, B, H, W, pad, st));
    SRX_TRY(fused::prefilter2d_fast(pad, scr, B, Hp, Wp, MODE_REFLECT, st, flags));
    if (!taps_ready) {
        SRX_TRY(build_taps(ty, Ho, Hp, TAP_SHIFT, istep, -sy, st));  // scipy negates the shift: cc = i + (-s)
        SRX_TRY(build_taps(tx, Wo, Wp, TAP_SHIFT, istep, -sx, st));
    }
    return interp(pad, B, Hp, Wp, ty, tx, Ho, Wo, out, accumulate, st);
}

// ---- workspace layouts of the primitives.  Each is one function: on the call's arena it is the carve, on a counting one (measured())
// the size its *_workspace_bytes query returns.  The counts: the planes of a [B, H, W] batch and the entries of the two tap tables --
// H and W in a call, the longer side for both in the bound (tap_bound) ----
struct ShiftDims {
    size_t B, H, W, ty, tx;
};
static ShiftDims shift_dims(int B, int H, int W) { return {(size_t)B, (size_t)H, (size_t)W, (size_t)H, (size_t)W}; }
static ShiftDims shift_bound(int eb, int B, int H, int W)
{
    const size_t tl = tap_bound(eb, (size_t)(H > W ? H : W));
    return {(size_t)B, (size_t)H, (size_t)W, tl, tl};
}
template <typename T> struct ShiftTabs {
    T *pad, *scr;
    AxisTap<T> *ty, *tx;
};
template <typename T> static ShiftTabs<T> carve_shift(Arena &ar, const ShiftDims &d)
{
    const size_t Hp = d.H + 2 * SRX_NPAD, Wp = d.W + 2 * SRX_NPAD;
    return {ar.take<T>(d.B * Hp * Wp), ar.take<T>(d.B * Hp * Wp), ar.take<AxisTap<T>>(d.ty), ar.take<AxisTap<T>>(d.tx)};
}
// forward_model: the blurred batch in front; back_project: the zero-inserted and the shifted batch (`planes` of them)
template <typename T, int planes> struct PlanesShiftTabs {
    T *p[planes];
    ShiftTabs<T> s;
};
template <typename T, int planes> static PlanesShiftTabs<T, planes> carve_planes_shift(Arena &ar, const ShiftDims &d)
{
    PlanesShiftTabs<T, planes> t;
    for (int i = 0; i < planes; i++)
        t.p[i] = ar.take<T>(d.B * d.H * d.W);
    t.s = carve_shift<T>(ar, d);
    return t;
}
template <int planes> static size_t planes_shift_ws(int eb, int B, int H, int W)
{
    const ShiftDims d = shift_bound(eb, B, H, W);
    return measured([&](Arena &m) { eb == 8 ? (void)carve_planes_shift<double, planes>(m, d) : (void)carve_planes_shift<float, planes>(m, d); });
}
static size_t shift_ws(int eb, int B, int H, int W) { return planes_shift_ws<0>(eb, B, H, W); }

template <typename T>
static int shift_cubic(const T *in, int B, int H, int W, double sy, double sx, T *out, void *ws, size_t wsb,
                       hipStream_t st)
{
    if (!in || !out || B <= 0 || H <= 0 || W <= 0)
        return SRX_E_INVALID;
    if (!plane_fits(sizeof(T), 1, H, W, H, W))
        return SRX_E_UNSUPPORTED;
    Arena ar(ws, wsb);
    ar.require(shift_ws((int)sizeof(T), B, H, W));
    const auto [pad, scr, ty, tx] = carve_shift<T>(ar, shift_dims(B, H, W));
    if (!ar.ok)
        return SRX_E_WORKSPACE;
    return shift_sampled(in, B, H, W, sy, sx, 1, H, W, out, false, pad, scr, ty, tx, false, st, 0);
}

// scipy.ndimage.zoom(order 3): in [B items, stride in_stride, h, w] -> out [B, Ho, Wo]
template <typename T>
static int zoom_into(const T *in, size_t in_stride, int B, int h, int w, int Ho, int Wo, T *out, T *coef, T *cscr,
                     AxisTap<T> *ty, AxisTap<T> *tx, hipStream_t st, unsigned flags)  // flags: as shift_sampled's
{
    SRX_TRY(copy_items(in, in_stride, B, (size_t)h * w, coef, st));
    SRX_TRY(fused::prefilter2d_fast(coef, cscr, B, h, w, MODE_MIRROR, st, flags));
    const double zy = Ho > 1 ? (double)(h - 1) / (double)(Ho - 1) : 1.0;
    const double zx = Wo > 1 ? (double)(w - 1) / (double)(Wo - 1) : 1.0;
    SRX_TRY(build_taps(ty, Ho, h, TAP_ZOOM, 1, zy, st));
    SRX_TRY(build_taps(tx, Wo, w, TAP_ZOOM, 1, zx, st));
    return interp(coef, B, h, w, ty, tx, Ho, Wo, out, false, st);
}

// zoom: the coefficient planes of a [B, h, w] batch and the two tap tables, h f and w f entries in a call
struct ZoomDims {
    size_t B, h, w, ty, tx;
};
template <typename T> struct ZoomTabs {
    T *coef, *cscr;
    AxisTap<T> *ty, *tx;
};
template <typename T> static ZoomTabs<T> carve_zoom(Arena &ar, const ZoomDims &d)
{
    return {ar.take<T>(d.B * d.h * d.w), ar.take<T>(d.B * d.h * d.w), ar.take<AxisTap<T>>(d.ty), ar.take<AxisTap<T>>(d.tx)};
}
static size_t zoom_ws(int eb, int B, int h, int w, int f)
{
    const size_t tl = tap_bound(eb, (size_t)(h > w ? h : w) * f);
    const ZoomDims d{(size_t)B, (size_t)h, (size_t)w, tl, tl};
    return measured([&](Arena &m) { eb == 8 ? (void)carve_zoom<double>(m, d) : (void)carve_zoom<float>(m, d); });
}

template <typename T>
static int zoom_cubic(const T *in, int B, int h, int w, int f, T *out, void *ws, size_t wsb, hipStream_t st)
{
    if (!in || !out || B <= 0 || h <= 0 || w <= 0 || f <= 0)
        return SRX_E_INVALID;
    if ((size_t)h * f >= ((size_t)1 << 30) || (size_t)w * f >= ((size_t)1 << 30) || !plane_fits(sizeof(T), 1, h, w, h * f, w * f))
        return SRX_E_UNSUPPORTED;
    Arena ar(ws, wsb);
    ar.require(zoom_ws((int)sizeof(T), B, h, w, f));
    const auto [coef, cscr, ty, tx] = carve_zoom<T>(ar, ZoomDims{(size_t)B, (size_t)h, (size_t)w, (size_t)h * f, (size_t)w * f});
    if (!ar.ok)
        return SRX_E_WORKSPACE;
    return zoom_into(in, (size_t)h * w, B, h, w, h * f, w * f, out, coef, cscr, ty, tx, st, 0);
}

// forward_model = decimate(shift(blur(hr)))
static size_t forward_ws(int eb, int B, int H, int W) { return planes_shift_ws<1>(eb, B, H, W); }

template <typename T>
static int forward_model(const T *hr, int B, int H, int W, const double *k, int kh, int kw, double sy, double sx, int f,
                         T *out, void *ws, size_t wsb, hipStream_t st)
{
    if (!hr || !out || !k || B <= 0 || H <= 0 || W <= 0 || f <= 0)
        return SRX_E_INVALID;
    if (!plane_fits(sizeof(T), 1, 1, 1, H, W))
        return SRX_E_UNSUPPORTED;
    Arena ar(ws, wsb);
    ar.require(forward_ws((int)sizeof(T), B, H, W));
    const auto t = carve_planes_shift<T, 1>(ar, shift_dims(B, H, W));
    T *const b = t.p[0], *const pad = t.s.pad, *const scr = t.s.scr;
    AxisTap<T> *const ty = t.s.ty, *const tx = t.s.tx;
    const int sh = cdiv(H, f), sw = cdiv(W, f);
    if (!ar.ok)
        return SRX_E_WORKSPACE;
    SRX_TRY(blur(hr, B, H, W, k, kh, kw, false, b, st));
    return shift_sampled(b, B, H, W, sy * f, sx * f, f, sh, sw, out, false, pad, scr, ty, tx, false, st, 0);
}

// back_project = blur_flipped(shift(zero_insert(err), -s f))
static size_t backproject_ws(int eb, int B, int H, int W) { return planes_shift_ws<2>(eb, B, H, W); }

template <typename T>
static int back_project(const T *err, int B, int eh, int ew, const double *k, int kh, int kw, double sy, double sx,
                        int f, int H, int W, T *out, void *ws, size_t wsb, hipStream_t st)
{
    if (!err || !out || !k || B <= 0 || eh <= 0 || ew <= 0 || H <= 0 || W <= 0 || f <= 0)
        return SRX_E_INVALID;
    if (B > 65535 || !plane_fits(sizeof(T), 1, eh, ew, H, W))
        return SRX_E_UNSUPPORTED;
    Arena ar(ws, wsb);
    ar.require(backproject_ws((int)sizeof(T), B, H, W));
    const auto t = carve_planes_shift<T, 2>(ar, shift_dims(B, H, W));
    T *const up = t.p[0], *const s2 = t.p[1], *const pad = t.s.pad, *const scr = t.s.scr;
    AxisTap<T> *const ty = t.s.ty, *const tx = t.s.tx;
    if (!ar.ok)
        return SRX_E_WORKSPACE;
    hipLaunchKernelGGL(k_zero_insert<T>, dim3(cdiv(W, 64), cdiv(H, 4), B), dim3(64, 4), 0, st, err, eh, ew, f, H, W, up);
    SRX_CHECK_LAUNCH();
    SRX_TRY(shift_sampled(up, B, H, W, -sy * f, -sx * f, 1, H, W, s2, false, pad, scr, ty, tx, false, st, 0));
    return blur(s2, B, H, W, k, kh, kw, true, out, st);
}

// ---------------------------------------------------------------------------------------
// composed shift_and_add
// ---------------------------------------------------------------------------------------
// the counts: a [B, h, w] frame batch, its [B, H, W] zoom, and two pairs of tap tables (zoom, shift) of ty / tx entries
struct SaaComposedDims {
    size_t B, h, w, H, W, ty, tx;
};
template <typename T> struct SaaComposedTabs {
    T *coef, *cscr, *up, *pad, *scr;
    AxisTap<T> *zy, *zx, *ty, *tx;
};
template <typename T> static SaaComposedTabs<T> carve_saa_composed(Arena &ar, const SaaComposedDims &d)
{
    const size_t Pp = d.B * (d.H + 2 * SRX_NPAD) * (d.W + 2 * SRX_NPAD);
    return {ar.take<T>(d.B * d.h * d.w), ar.take<T>(d.B * d.h * d.w), ar.take<T>(d.B * d.H * d.W), ar.take<T>(Pp), ar.take<T>(Pp),
            ar.take<AxisTap<T>>(d.ty), ar.take<AxisTap<T>>(d.tx), ar.take<AxisTap<T>>(d.ty), ar.take<AxisTap<T>>(d.tx)};
}
static size_t saa_ws_composed(const SaaShape &s, int B)
{
    const size_t H = (size_t)s.h * s.f, W = (size_t)s.w * s.f, tl = tap_bound(s.eb, H > W ? H : W);
    const SaaComposedDims d{(size_t)B, (size_t)s.h, (size_t)s.w, H, W, tl, tl};
    return measured([&](Arena &m) { s.eb == 8 ? (void)carve_saa_composed<double>(m, d) : (void)carve_saa_composed<float>(m, d); });
}

template <typename T> static int saa_composed(const SaaCall<T> &c)
{
    const int B = c.B, N = c.s.N, h = c.s.h, w = c.s.w, f = c.s.f, H = h * f, W = w * f;
    const double *const sh = c.s.sh;
    const T *const lr = c.lr;
    T *const out = c.out;
    const hipStream_t st = c.st;
    Arena ar(c.ws, c.wsb);
    const auto [coef, cscr, up, pad, scr, zy, zx, ty, tx] =
        carve_saa_composed<T>(ar, SaaComposedDims{(size_t)B, (size_t)h, (size_t)w, (size_t)H, (size_t)W, (size_t)H, (size_t)W});
    if (!ar.ok)
        return SRX_E_WORKSPACE;
    const size_t n = (size_t)B * H * W;
    if (fill_bytes(out, 0, n * sizeof(T), st) != hipSuccess)
        return SRX_E_HIP;
    for (int k = 0; k < N; k++) {
        SRX_TRY(zoom_into(lr + (size_t)k * h * w, (size_t)N * h * w, B, h, w, H, W, up, coef, cscr, zy, zx, st, c.s.flags));
        SRX_TRY(shift_sampled(up, B, H, W, sh[2 * k] * f, sh[2 * k + 1] * f, 1, H, W, out, true, pad, scr, ty, tx, false, st, c.s.flags));
    }
    hipLaunchKernelGGL(k_div<T>, dim3(grid1d(n)), dim3(256), 0, st, out, (T)N, n);
    SRX_CHECK_LAUNCH();
    return SRX_OK;
}

// ---------------------------------------------------------------------------------------
// composed ibp: the reference's loop, frame by frame (run_sr.py:190-209).  blur(hr) is taken
// once per iteration (it is the same array for every frame); everything else is literal.
// ---------------------------------------------------------------------------------------
// the counts: [B, H, W] planes, the [B, sh, sw] simulated frames, 4 N tap tables of tl entries, rblk block partials of k_residual per item
struct IbpComposedDims {
    size_t B, N, H, W, sh, sw, tl, rblk;
};
template <typename T> struct IbpComposedTabs {
    T *b, *up, *s2, *bp, *corr, *pad, *scr, *sim, *err;
    AxisTap<T> *taps[4 * SRX_MAX_FRAMES];
    double *rpart;
};
template <typename T> static IbpComposedTabs<T> carve_ibp_composed(Arena &ar, const IbpComposedDims &d)
{
    const size_t P = d.B * d.H * d.W, Pp = d.B * (d.H + 2 * SRX_NPAD) * (d.W + 2 * SRX_NPAD);
    IbpComposedTabs<T> t{ar.take<T>(P), ar.take<T>(P), ar.take<T>(P), ar.take<T>(P), ar.take<T>(P), ar.take<T>(Pp), ar.take<T>(Pp),
                         ar.take<T>(d.B * d.sh * d.sw), ar.take<T>(d.B * d.sh * d.sw), {}, nullptr};
    for (size_t i = 0; i < 4 * d.N; i++) {  // (a query accepts N beyond what a call does: counted, not kept)
        AxisTap<T> *const p = ar.take<AxisTap<T>>(d.tl);
        if (i < 4 * SRX_MAX_FRAMES)
            t.taps[i] = p;
    }
    t.rpart = ar.take<double>(d.B * d.rblk);
    return t;
}
// the bound: the block partials of whole simulated frames (a call's residual covers min(sh, h) x min(sw, w) of them)
static size_t ibp_ws_composed(const IbpShape &s, int B)
{
    const int H = s.H, W = s.W, sh = cdiv(H, s.f), sw = cdiv(W, s.f);
    const IbpComposedDims d{(size_t)B, (size_t)(s.N > 0 ? s.N : 0), (size_t)H, (size_t)W, (size_t)sh, (size_t)sw, tap_bound(s.eb, (size_t)(H > W ? H : W)),
                            (size_t)cdiv(sw, 64) * cdiv(sh, 4)};
    return measured([&](Arena &m) { s.eb == 8 ? (void)carve_ibp_composed<double>(m, d) : (void)carve_ibp_composed<float>(m, d); });
}

template <typename T> static int ibp_composed(const IbpCall<T> &c)
{
    const int B = c.B, N = c.s.N, h = c.s.h, w = c.s.w, H = c.s.H, W = c.s.W, f = c.s.f, kh = c.s.kh, kw = c.s.kw, n_iter = c.n_iter;
    const double *const shf = c.s.sh, *const k = c.s.k, step = c.step;
    const T *const lr = c.lr, *const hr_init = c.hr_init;
    T *const hr = c.hr;
    double *const errors = c.errors;
    const hipStream_t st = c.st;
    const unsigned flags = c.s.flags;
    const int sh = cdiv(H, f), sw = cdiv(W, f);
    const int mh = sh < h ? sh : h, mw = sw < w ? sw : w;
    const size_t P = (size_t)B * H * W;
    Arena ar(c.ws, c.wsb);
    const int rblk = cdiv(mw, 64) * cdiv(mh, 4);
    const auto [b, up, s2, bp, corr, pad, scr, sim, err, taps, rpart] = carve_ibp_composed<T>(
        ar, IbpComposedDims{(size_t)B, (size_t)N, (size_t)H, (size_t)W, (size_t)sh, (size_t)sw, (size_t)(H > W ? H : W), (size_t)rblk});
    if (!ar.ok)
        return SRX_E_WORKSPACE;
    const int Hp = H + 2 * SRX_NPAD, Wp = W + 2 * SRX_NPAD;
    for (int q = 0; q < N; q++) {
        const double sy = shf[2 * q] * f, sx = shf[2 * q + 1] * f;
        SRX_TRY(build_taps(taps[4 * q + 0], sh, Hp, TAP_SHIFT, f, -sy, st));
        SRX_TRY(build_taps(taps[4 * q + 1], sw, Wp, TAP_SHIFT, f, -sx, st));
        SRX_TRY(build_taps(taps[4 * q + 2], H, Hp, TAP_SHIFT, 1, sy, st));  // back_project shifts by -s: cc = i + s
        SRX_TRY(build_taps(taps[4 * q + 3], W, Wp, TAP_SHIFT, 1, sx, st));
    }
    if (hr != hr_init && hipMemcpyAsync(hr, hr_init, P * sizeof(T), hipMemcpyDeviceToDevice, st) != hipSuccess)
        return SRX_E_HIP;
    if (errors && fill_bytes(errors, 0, (size_t)B * n_iter * sizeof(double), st) != hipSuccess)
        return SRX_E_HIP;
    const double scale = 1.0 / ((double)mh * (double)mw) / (double)N;
    for (int it = 0; it < n_iter; it++) {
        SRX_TRY(blur(hr, B, H, W, k, kh, kw, false, b, st));
        if (fill_bytes(corr, 0, P * sizeof(T), st) != hipSuccess)
            return SRX_E_HIP;
        for (int q = 0; q < N; q++) {
            SRX_TRY(shift_sampled(b, B, H, W, 0, 0, f, sh, sw, sim, false, pad, scr, taps[4 * q], taps[4 * q + 1], true, st, flags));
            hipLaunchKernelGGL(k_residual<T>, dim3(cdiv(mw, 64), cdiv(mh, 4), B), dim3(64, 4), 0, st,
                               lr + (size_t)q * h * w, (size_t)N * h * w, w, sim, (size_t)sh * sw, sw, mh, mw, err, errors ? rpart : nullptr);
            SRX_CHECK_LAUNCH();
            if (errors) {
                hipLaunchKernelGGL(k_residual_reduce, dim3(B), dim3(256), 0, st, rpart, rblk, errors + it, n_iter, scale);
                SRX_CHECK_LAUNCH();
            }
            hipLaunchKernelGGL(k_zero_insert<T>, dim3(cdiv(W, 64), cdiv(H, 4), B), dim3(64, 4), 0, st, err, mh, mw, f, H,
                               W, up);
            SRX_CHECK_LAUNCH();
            SRX_TRY(shift_sampled(up, B, H, W, 0, 0, 1, H, W, s2, false, pad, scr, taps[4 * q + 2], taps[4 * q + 3], true, st, flags));
            SRX_TRY(blur(s2, B, H, W, k, kh, kw, true, bp, st));
            hipLaunchKernelGGL(k_add<T>, dim3(grid1d(P)), dim3(256), 0, st, corr, bp, P);
            SRX_CHECK_LAUNCH();
        }
        hipLaunchKernelGGL(k_update<T>, dim3(grid1d(P)), dim3(256), 0, st, hr, corr, (T)step, (T)N, P);
        SRX_CHECK_LAUNCH();
    }
    return SRX_OK;
}

// ---------------------------------------------------------------------------------------
// dispatch
// ---------------------------------------------------------------------------------------
#define SRX_MAX_BATCH_PER_LAUNCH 32768  // gridDim.z <= 65535; larger batches go through in chunks of this many items
// The items of one chunk (shift_and_add's kernels take an (item, frame) pair per gridDim.z).  The workspace queries accept any B and N, so
// these do: B <= 0 passes through, and a query that sizes a table or a staged copy for at least one item says so with std::max.
static inline int ibp_chunk_items(int B) { return B > SRX_MAX_BATCH_PER_LAUNCH ? SRX_MAX_BATCH_PER_LAUNCH : B; }
static inline int saa_chunk_items(int B, int N)
{
    if ((long)B * N > SRX_MAX_BATCH_PER_LAUNCH)
        return SRX_MAX_BATCH_PER_LAUNCH / N > 0 ? SRX_MAX_BATCH_PER_LAUNCH / N : 1;
    return B;
}

// Argument and limit checks of an ibp call: of every srx_ibp entry point, the per-item form, a plan and srx_ibp_path_for.  present: the
// call's device pointers are (only that counts).  Every invalid argument is answered before any limit.
static int ibp_check(const IbpSpec &s, int B, int n_iter, bool present)
{
    if (!present || !s.sh || !s.k || B <= 0 || s.N <= 0 || s.h <= 0 || s.w <= 0 || s.H <= 0 || s.W <= 0 || s.f <= 0 || s.kh <= 0 || s.kw <= 0 || n_iter < 0)
        return SRX_E_INVALID;
    if (s.N > SRX_MAX_FRAMES || s.kh * s.kw > SRX_MAX_KERNEL_TAPS || !plane_fits((size_t)s.eb, s.N, s.h, s.w, s.H, s.W))
        return SRX_E_UNSUPPORTED;
    return SRX_OK;
}
// ... and of a shift_and_add call: every srx_saa entry point, the per-item form and srx_saa_path_for
static int saa_check(const SaaSpec &s, int B, bool present)
{
    if (!present || !s.sh || B <= 0 || s.N <= 0 || s.h <= 0 || s.w <= 0 || s.f <= 0)
        return SRX_E_INVALID;
    if (s.N > SRX_MAX_FRAMES || (size_t)s.h * s.f >= ((size_t)1 << 30) || (size_t)s.w * s.f >= ((size_t)1 << 30) ||
        !plane_fits((size_t)s.eb, s.N, s.h, s.w, s.h * s.f, s.w * s.f))
        return SRX_E_UNSUPPORTED;
    return SRX_OK;
}

// The shape-only workspace bounds (srx_ibp_workspace_bytes, srx_saa_workspace_bytes): the largest of the paths a call of this shape may
// take.  Of the flags the two that name a path count and no other: no SRX_FLAG_DIAG_* switch changes a size.
static size_t ibp_bound(const IbpShape &s, int B, unsigned flags)
{
    B = ibp_chunk_items(B);
    const size_t a = ibp_ws_composed(s, B), b = std::max(fused::ibp_ws(s, B), mosaic::ibp_ws(s, B));
    if (flags & SRX_FLAG_FUSED)
        return b;
    if (flags & SRX_FLAG_COMPOSED)
        return a;
    return a > b ? a : b;
}
static size_t saa_bound(const SaaShape &s, int B)
{
    B = saa_chunk_items(B, s.N);
    return std::max(std::max(saa_ws_composed(s, B), fused::saa_ws(s, B)), mosaic::saa_ws(s, B));
}

// The route of one srx_ibp / srx_saa call (valid arguments within the library's limits), decided here and nowhere else: the call itself, its
// per-item form, a plan, the exact workspace query and srx_*_path_for read it.  A function of the spec alone -- the shape, the two host
// tables and the flags -- so the batch size plays no part and whoever holds a spec gets the route of that call.  Pure host arithmetic.
enum Path { PATH_COMPOSED, PATH_FUSED, PATH_BTILE, PATH_MOSAIC };  // (shift_and_add has no PATH_BTILE)
struct Route {
    int status;                    // an early answer (SRX_FLAG_FUSED on a call that cannot fuse), else SRX_OK
    Path path;
    const mosaic::ImplRow *impl;   // ibp on PATH_MOSAIC: the row of srx_route.hpp's table
    const char *name;              // what srx_last_path() reports
};

static Route route_ibp(const IbpSpec &s)
{
    const bool can_fuse = fused::ibp_eligible(s);
    if ((s.flags & SRX_FLAG_FUSED) && !can_fuse)
        return {SRX_E_UNSUPPORTED, PATH_COMPOSED, nullptr, "none"};
    if (!can_fuse || (s.flags & SRX_FLAG_COMPOSED))
        return {SRX_OK, PATH_COMPOSED, nullptr, "composed"};
    if (!(s.flags & SRX_FLAG_PER_FRAME) && mosaic::eligible(s)) {
        const mosaic::ImplRow &impl = mosaic::choose_impl(s);
        return {SRX_OK, PATH_MOSAIC, &impl, impl.name};
    }
    if (btile::eligible(s))
        return {SRX_OK, PATH_BTILE, nullptr, "btile"};
    return {SRX_OK, PATH_FUSED, nullptr, "fused"};
}

static Route route_saa(const SaaSpec &s)
{
    const bool can_fuse = fused::saa_eligible(s);
    if ((s.flags & SRX_FLAG_FUSED) && !can_fuse)
        return {SRX_E_UNSUPPORTED, PATH_COMPOSED, nullptr, "none"};
    if (!can_fuse || (s.flags & SRX_FLAG_COMPOSED))
        return {SRX_OK, PATH_COMPOSED, nullptr, "composed"};
    if (!(s.flags & SRX_FLAG_PER_FRAME) && mosaic::saa_eligible(s))
        return {SRX_OK, PATH_MOSAIC, nullptr, "mosaic"};
    return {SRX_OK, PATH_FUSED, nullptr, "fused"};
}

// What a call on route `r` must bring: exactly what a mosaic implementation carves (the shape-only bound covers it by construction,
// tests/test_abi.py sweeps shapes for need <= bound), the shape-only bound on every other path.
static size_t ibp_need(const Route &r, const IbpSpec &s, int B)
{
    if (r.status != SRX_OK || r.path != PATH_MOSAIC)
        return ibp_bound(s, B, s.flags);
    return mosaic::ibp_ws_for(*r.impl, s, ibp_chunk_items(B));
}

// The uint8 entry points (srx_ibp_u8lr_*, srx_saa_u8lr_*) off the mosaic family: the chunk's frames are converted to T at the front of the
// workspace and the float driver runs on the rest.  (Those routes serve per-frame fractional shifts; the mosaic family reads the bytes itself.)
template <typename T> static T *carve_u8_stage(Arena &ar, size_t n) { return ar.take<T>(n); }
template <typename Shape> static inline size_t u8_stage_bytes(const Shape &s, int Bc)  // Shape: IbpShape or SaaShape
{
    const size_t n = (size_t)Bc * s.N * s.h * s.w;
    return measured([&](Arena &m) { s.eb == 8 ? (void)carve_u8_stage<double>(m, n) : (void)carve_u8_stage<float>(m, n); });
}

template <typename T> static int u8_stage(const uint8_t *lr, size_t n, void *&ws, size_t &wsb, const T *&staged, hipStream_t st)
{
    Arena ar(ws, wsb);
    T *const dst = carve_u8_stage<T>(ar, n);
    if (!ar.ok)
        return SRX_E_WORKSPACE;
    hipLaunchKernelGGL(k_u8_to<T>, dim3(grid1d(n)), dim3(256), 0, st, lr, n, dst);
    SRX_CHECK_LAUNCH();
    staged = dst;
    ws = (char *)ws + ar.off, wsb -= ar.off;
    return SRX_OK;
}
// the frames of a chunk in T and the workspace behind them: the caller's own, or the staged copy of its uint8 samples
template <typename T, typename S> static int frames_in_t(const S *lr_, size_t n, void *&ws, size_t &wsb, const T *&lr, hipStream_t st)
{
    if constexpr (std::is_same<S, T>::value)
        return lr = lr_, SRX_OK;
    else
        return u8_stage<T>(lr_, n, ws, wsb, lr, st);
}

// one chunk (at most SRX_MAX_BATCH_PER_LAUNCH items) of a call on the route its entry point decided
template <typename T, typename S> static int ibp_run(const Route &r, const IbpCall<T, S> &c)
{
    if (r.path == PATH_MOSAIC)
        return mosaic::ibp<T, S>(*r.impl, c);
    const T *lr = nullptr;
    void *ws = c.ws;
    size_t wsb = c.wsb;
    SRX_TRY((frames_in_t<T, S>(c.lr, (size_t)c.B * c.s.N * c.s.h * c.s.w, ws, wsb, lr, c.st)));
    const IbpCall<T> ct = c.on(lr, ws, wsb);
    switch (r.path) {
    case PATH_MOSAIC:  // (taken above)
        break;
    case PATH_BTILE:
        if constexpr (sizeof(T) == 4)
            return btile::ibp(ct);
        return SRX_E_INVALID;  // (route_ibp gives float32 calls alone this path)
    case PATH_FUSED:
        return fused::ibp<T>(ct);
    case PATH_COMPOSED:
        break;
    }
    return ibp_composed<T>(ct);
}

template <typename T, typename S> static int ibp_dispatch(const IbpCall<T, S> &c)
{
    SRX_TRY(ibp_check(c.s, c.B, c.n_iter, c.lr && c.hr_init && c.hr));
    const Route r = route_ibp(c.s);  // once per call: the batch size plays no part
    if (r.status != SRX_OK)
        return r.status;
    // a short or misaligned workspace is refused before anything is queued
    size_t need = ibp_need(r, c.s, c.B);
    if (!std::is_same<S, T>::value && r.path != PATH_MOSAIC)
        need += u8_stage_bytes(c.s, ibp_chunk_items(c.B));
    if (ws_short(c.ws, c.wsb, need))
        return SRX_E_WORKSPACE;
    g_last_path = r.name;
    // batches beyond one launch's gridDim.z go through in chunks; the workspace is sized for one chunk and reused (stream order)
    for (int b0 = 0; b0 < c.B; b0 += SRX_MAX_BATCH_PER_LAUNCH)
        SRX_TRY(ibp_run(r, c.chunk(b0, ibp_chunk_items(c.B - b0))));
    return SRX_OK;
}

// one chunk (at most saa_chunk_items items) of a call on the route its entry point decided
template <typename T, typename S> static int saa_run(const Route &r, const SaaCall<T, S> &c)
{
    if (r.path == PATH_MOSAIC)
        return mosaic::saa<T, S>(c);
    const T *lr = nullptr;
    void *ws = c.ws;
    size_t wsb = c.wsb;
    SRX_TRY((frames_in_t<T, S>(c.lr, (size_t)c.B * c.s.N * c.s.h * c.s.w, ws, wsb, lr, c.st)));
    const SaaCall<T> ct = c.on(lr, ws, wsb);
    return r.path == PATH_FUSED ? fused::saa<T>(ct) : saa_composed<T>(ct);
}

template <typename T, typename S> static int saa_dispatch(const SaaCall<T, S> &c)
{
    SRX_TRY(saa_check(c.s, c.B, c.lr && c.out));
    const Route r = route_saa(c.s);  // once per call: the batch size plays no part
    // Every refusal comes before anything is queued (the uint8 staging included).  These entry points answer a short workspace BEFORE
    // SRX_FLAG_FUSED on a table that cannot fuse, items::saa_dispatch_items the other way round: callers have met both orders, both stay.
    const size_t stage = std::is_same<S, T>::value ? 0 : u8_stage_bytes(c.s, saa_chunk_items(c.B, c.s.N));  // (whatever the route: srx_saa_u8lr_workspace_bytes)
    if (ws_short(c.ws, c.wsb, saa_bound(c.s, c.B) + stage))
        return SRX_E_WORKSPACE;
    if (r.status != SRX_OK)
        return r.status;
    g_last_path = r.name;
    // batches beyond one launch's gridDim.z go through in chunks; the workspace is sized for one chunk and reused (stream order)
    for (int b0 = 0, bc; b0 < c.B; b0 += bc) {
        bc = saa_chunk_items(c.B - b0, c.s.N);
        SRX_TRY(saa_run(r, c.chunk(b0, bc)));
    }
    return SRX_OK;
}

#include "srx_items.hpp"  // one shift table per item: routing by runs on top of the route, the checks and the chunk drivers above

// ---------------------------------------------------------------------------------------
// plans: the per-call tables built ONCE, the iterations in several runs, rows of the state readable / replaceable in between
// (what a row band of a larger image needs: sr_mi355x/rowband.py).  A plan keeps device state in the caller's workspace and a
// small host record; the frames and the workspace must stay alive until the plan is destroyed.
// ---------------------------------------------------------------------------------------
struct srx_plan_s {
    IbpSpec s;            // the call every run makes; sh and k point at the copies below (a plan lives where it was made: never copied)
    double sh[2 * SRX_MAX_FRAMES], k[SRX_MAX_KERNEL_TAPS];
    int B, tr_lo, tr_hi;
    double step;
    const void *lr;
    bool z;               // k_ibp_ztile with hoisted tables (float32, integer HR shifts, frames of at least 128 x 128)
    ztile::State zs;
    void *hr;             // otherwise: the state as a plain [B, H, W] plane at the head of the workspace; every run is a whole srx_ibp call
    void *ws_rest;
    size_t wsb_rest;
    const char *path;
};

// a plan off the hoisted-table path keeps its state as a plain [B, H, W] plane at the head of the workspace
template <typename T> static T *carve_plan_state(Arena &ar, size_t B, int H, int W) { return ar.take<T>(B * H * W); }
static size_t plan_bound(const IbpShape &s, int B, unsigned flags)
{
    const size_t b1 = B > 0 ? B : 1;
    return measured([&](Arena &m) { s.eb == 8 ? (void)carve_plan_state<double>(m, b1, s.H, s.W) : (void)carve_plan_state<float>(m, b1, s.H, s.W); }) +
           ibp_bound(s, B, flags);
}

// c: the call the plan's runs make, less what a run brings (n_iter, errors) and with no hr: the state lives in the workspace
template <typename T> static int plan_create(const IbpCall<T> &c, int tr_lo, int tr_hi, srx_plan_s **out)
{
    const IbpSpec &s = c.s;
    const int B = c.B, checked = ibp_check(s, B, 0, c.lr && c.hr_init && c.ws);
    if (!out || checked == SRX_E_INVALID || tr_lo < 0 || tr_hi > s.H || tr_lo > tr_hi)
        return SRX_E_INVALID;
    if (checked != SRX_OK || B > SRX_MAX_BATCH_PER_LAUNCH)
        return SRX_E_UNSUPPORTED;
    if (ws_short(c.ws, c.wsb, plan_bound(s, B, s.flags)))  // before anything is queued
        return SRX_E_WORKSPACE;
    srx_plan_s *p = new srx_plan_s();
    std::memcpy(p->sh, s.sh, sizeof(double) * 2 * s.N);
    std::memcpy(p->k, s.k, sizeof(double) * s.kh * s.kw);
    p->s = s, p->s.sh = p->sh, p->s.k = p->k;
    p->B = B, p->tr_lo = tr_lo, p->tr_hi = tr_hi, p->step = c.step, p->lr = c.lr;
    p->z = false, p->hr = nullptr, p->ws_rest = nullptr, p->wsb_rest = 0, p->path = "none";
    Arena ar(c.ws, c.wsb);
    int rc = SRX_OK;
    const Route r = route_ibp(s);
    const bool z = r.status == SRX_OK && r.path == PATH_MOSAIC && r.impl->id == mosaic::IMPL_ZTILE;
    if constexpr (sizeof(T) == 4) {  // (k_ibp_ztile is float32 only: ztile::eligible)
        if (z) {
            mosaic::Common<float> cm;
            rc = mosaic::common_prep<float>(cm, false, c, ar, tr_lo, tr_hi);
            if (rc == SRX_OK)
                rc = ztile::setup(p->zs, cm, c.hr_init, tr_lo, tr_hi, ar, c.st);
            p->z = true, p->path = "ztile";
        }
    }
    if (!z) {
        T *hr = carve_plan_state<T>(ar, B, s.H, s.W);
        if (!ar.ok)
            rc = SRX_E_WORKSPACE;
        else if (hipMemcpyAsync(hr, c.hr_init, (size_t)B * s.H * s.W * sizeof(T), hipMemcpyDeviceToDevice, c.st) != hipSuccess)
            rc = SRX_E_HIP;
        p->hr = hr, p->ws_rest = ar.ok ? (char *)c.ws + ar.off : nullptr, p->wsb_rest = ar.ok ? c.wsb - ar.off : 0, p->path = "call per run";
    }
    if (rc != SRX_OK) {
        delete p;
        return rc;
    }
    *out = p;
    return SRX_OK;
}

// a run off the hoisted-table path: a whole srx_ibp call from the state plane onto itself
template <typename T> static int plan_run(const srx_plan_s *p, int n_iter, double *errors, hipStream_t st)
{
    T *const hr = (T *)p->hr;
    return ibp_dispatch(IbpCall<T>{p->s, (const T *)p->lr, p->B, hr, n_iter, p->step, hr, errors, p->ws_rest, p->wsb_rest, st});
}

template <typename T> __global__ void __launch_bounds__(256) k_rows_copy(const T *__restrict__ src, T *__restrict__ dst, int H, int W, int y0, int rows, int to_plane)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y, b = blockIdx.z;
    if (x >= W)
        return;
    const size_t ip = ((size_t)b * H + y0 + y) * W + x, ib = ((size_t)b * rows + y) * W + x;
    if (to_plane)
        dst[ip] = src[ib];
    else
        dst[ib] = src[ip];
}

template <typename T> static int plan_rows(srx_plan_s *p, int y0, int y1, T *buf, bool set, hipStream_t st)
{
    if (!p || !buf || p->s.eb != (int)sizeof(T) || y0 < 0 || y1 > p->s.H || y0 >= y1)
        return SRX_E_INVALID;
    const int rows = y1 - y0;
    if (rows > 65535)
        return SRX_E_UNSUPPORTED;
    if (p->z) {
        if constexpr (sizeof(T) == 4)
            return set ? ztile::rows_in(p->zs, y0, rows, buf, st) : ztile::rows_out(p->zs, y0, rows, buf, st);
        return SRX_E_INVALID;
    }
    T *hr = (T *)p->hr;
    hipLaunchKernelGGL(k_rows_copy<T>, dim3(cdiv(p->s.W, 256), rows, p->B), dim3(256), 0, st, set ? (const T *)buf : (const T *)hr, set ? hr : buf, p->s.H, p->s.W, y0, rows,
                       set ? 1 : 0);
    SRX_CHECK_LAUNCH();
    return SRX_OK;
}

// ---------------------------------------------------------------------------------------
// extern "C"
// ---------------------------------------------------------------------------------------
extern "C" {

// The records of a call, from the arguments of its entry point under the names srx.h gives them.  An entry point builds its record and
// hands it on; nothing else happens in it.
#define SRX_IBP_SHAPE(EB) IbpShape{(EB), N, h, w, H, W, f}
#define SRX_IBP_SPEC(EB) IbpSpec{SRX_IBP_SHAPE(EB), sh, k, kh, kw, flags}
#define SRX_IBP_CALL(T, S, N_ITER, HR, ERRORS) IbpCall<T, S>{SRX_IBP_SPEC((int)sizeof(T)), lr, B, hr_init, (N_ITER), step, (HR), (ERRORS), ws, wsb, hs(s)}
#define SRX_SAA_SHAPE(EB) SaaShape{(EB), N, h, w, f}
#define SRX_SAA_CALL(T, S) SaaCall<T, S>{SaaSpec{SRX_SAA_SHAPE((int)sizeof(T)), sh, flags}, lr, B, out, ws, wsb, hs(s)}

size_t srx_ibp_plan_workspace_bytes(int eb, int B, int N, int h, int w, int H, int W, int f, unsigned flags) { return plan_bound(SRX_IBP_SHAPE(eb), B, flags); }

int srx_ibp_plan_create_f32(const float *lr, int B, int N, int h, int w, const double *sh, const double *k, int kh, int kw, const float *hr_init, int H,
                            int W, int f, double step, int tr_lo, int tr_hi, void *ws, size_t wsb, srx_stream_t s, unsigned flags, srx_plan_t **plan)
{
    return plan_create(SRX_IBP_CALL(float, float, 0, nullptr, nullptr), tr_lo, tr_hi, plan);
}
int srx_ibp_plan_create_f64(const double *lr, int B, int N, int h, int w, const double *sh, const double *k, int kh, int kw, const double *hr_init, int H,
                            int W, int f, double step, int tr_lo, int tr_hi, void *ws, size_t wsb, srx_stream_t s, unsigned flags, srx_plan_t **plan)
{
    return plan_create(SRX_IBP_CALL(double, double, 0, nullptr, nullptr), tr_lo, tr_hi, plan);
}

int srx_ibp_plan_run(srx_plan_t *p, int n_iter, double *errors, srx_stream_t s)
{
    if (!p || n_iter < 0)
        return SRX_E_INVALID;
    if (n_iter == 0)
        return SRX_OK;
    if (p->z)
        return ztile::run(p->zs, n_iter, errors, hs(s));
    if (errors && (p->tr_lo != 0 || p->tr_hi != p->s.H))
        return SRX_E_UNSUPPORTED;  // a row range for the trace exists where the tables are hoisted (the float32 integer-shift frame kernel)
    return p->s.eb == 4 ? plan_run<float>(p, n_iter, errors, hs(s)) : plan_run<double>(p, n_iter, errors, hs(s));
}

int srx_ibp_plan_get_rows_f32(srx_plan_t *p, int row_lo, int row_hi, float *dst, srx_stream_t s) { return plan_rows<float>(p, row_lo, row_hi, dst, false, hs(s)); }
int srx_ibp_plan_set_rows_f32(srx_plan_t *p, int row_lo, int row_hi, const float *src, srx_stream_t s)
{
    return plan_rows<float>(p, row_lo, row_hi, const_cast<float *>(src), true, hs(s));
}
int srx_ibp_plan_get_rows_f64(srx_plan_t *p, int row_lo, int row_hi, double *dst, srx_stream_t s) { return plan_rows<double>(p, row_lo, row_hi, dst, false, hs(s)); }
int srx_ibp_plan_set_rows_f64(srx_plan_t *p, int row_lo, int row_hi, const double *src, srx_stream_t s)
{
    return plan_rows<double>(p, row_lo, row_hi, const_cast<double *>(src), true, hs(s));
}
const char *srx_ibp_plan_path(srx_plan_t *p) { return p ? p->path : "none"; }
int srx_ibp_plan_supports_trace_rows(srx_plan_t *p) { return p && p->z ? 1 : 0; }
void srx_ibp_plan_destroy(srx_plan_t *p) { delete p; }

int srx_version(void) { return 100; }

#ifdef SRX_STAMPS
// diagnostic build only: copy the phase stamps of the mosaic kernels to the host and clear them
int srx_debug_stamps(unsigned long long *host_out)
{
    if (hipDeviceSynchronize() != hipSuccess)
        return SRX_E_HIP;
    if (hipMemcpyFromSymbol(host_out, HIP_SYMBOL(srx::srx_dbg_stamps), sizeof(unsigned long long) * 5 * 8 * 40000) != hipSuccess)
        return SRX_E_HIP;
    return SRX_OK;
}
int srx_debug_pstamps(unsigned long long *host_out)
{
    if (hipDeviceSynchronize() != hipSuccess)
        return SRX_E_HIP;
    if (hipMemcpyFromSymbol(host_out, HIP_SYMBOL(srx::srx_dbg_pstamps), sizeof(unsigned long long) * 24 * 4096) != hipSuccess)
        return SRX_E_HIP;
    return SRX_OK;
}
#endif

const char *srx_strerror(int s)
{
    switch (s) {
    case SRX_OK: return "ok";
    case SRX_E_INVALID: return "invalid argument";
    case SRX_E_UNSUPPORTED: return "unsupported configuration";
    case SRX_E_WORKSPACE: return "workspace missing, not 256-byte aligned or too small";
    case SRX_E_HIP: return "HIP runtime error";
    default: return "unknown status";
    }
}

const char *srx_last_path(void) { return g_last_path; }

void srx_profile_enable(int on)
{
    profiler().clear();
    profiler().on = on != 0;
}

int srx_profile_kernel_count(void) { return KID_COUNT; }

const char *srx_profile_kernel_name(int id) { return id >= 0 && id < KID_COUNT ? g_kernel_names[id] : ""; }

int srx_profile_get(int id, double *total_ms, long *launches)
{
    if (id < 0 || id >= KID_COUNT || !total_ms || !launches)
        return SRX_E_INVALID;
    Profiler &pf = profiler();
    std::lock_guard<std::mutex> g(pf.mu);
    double tot = 0.0;
    long cnt = 0;
    for (size_t i = 0; i < pf.rec.size(); i++) {
        if (pf.rec[i].id != id || !pf.rec[i].ended)
            continue;
        float ms = 0.f;
        if (hipEventSynchronize(pf.rec[i].b) != hipSuccess || hipEventElapsedTime(&ms, pf.rec[i].a, pf.rec[i].b) != hipSuccess)
            return SRX_E_HIP;
        tot += ms;
        cnt++;
    }
    *total_ms = tot;
    *launches = cnt;
    return SRX_OK;
}

size_t srx_shift_workspace_bytes(int eb, int B, int H, int W) { return shift_ws(eb, B, H, W); }
size_t srx_zoom_workspace_bytes(int eb, int B, int h, int w, int f) { return zoom_ws(eb, B, h, w, f); }
size_t srx_forward_workspace_bytes(int eb, int B, int H, int W) { return forward_ws(eb, B, H, W); }
size_t srx_backproject_workspace_bytes(int eb, int B, int H, int W) { return backproject_ws(eb, B, H, W); }

size_t srx_saa_workspace_bytes(int eb, int B, int N, int h, int w, int f) { return saa_bound(SRX_SAA_SHAPE(eb), B); }

/* float figure + one staged copy (T) of a chunk's frames, whatever the route: the query has no shift table to tell the routes apart */
size_t srx_saa_u8lr_workspace_bytes(int eb, int B, int N, int h, int w, int f)
{
    return saa_bound(SRX_SAA_SHAPE(eb), B) + u8_stage_bytes(SRX_SAA_SHAPE(eb), saa_chunk_items(B, N));
}

size_t srx_ibp_workspace_bytes(int eb, int B, int N, int h, int w, int H, int W, int f, unsigned flags) { return ibp_bound(SRX_IBP_SHAPE(eb), B, flags); }

/* the same with the shift table and the PSF at hand: what THIS call will carve (a batch of 256 x 256 patches at a common fraction
 * needs no tile planes, a delta = 0 frame no patch tables ...), never more than srx_ibp_workspace_bytes */
size_t srx_ibp_workspace_bytes_for(int eb, int B, int N, int h, int w, int H, int W, int f, const double *sh, const double *k, int kh,
                                   int kw, unsigned flags)
{
    if (!sh || !k || N <= 0 || N > SRX_MAX_FRAMES)
        return ibp_bound(SRX_IBP_SHAPE(eb), B, flags);
    const IbpSpec spec = SRX_IBP_SPEC(eb);
    return ibp_need(route_ibp(spec), spec, B);
}

/* uint8 frames: the float figure on a mosaic-family route (the kernels read the bytes; nothing is staged), plus the staged chunk elsewhere */
size_t srx_ibp_u8lr_workspace_bytes(int eb, int B, int N, int h, int w, int H, int W, int f, unsigned flags)
{
    return ibp_bound(SRX_IBP_SHAPE(eb), B, flags) + u8_stage_bytes(SRX_IBP_SHAPE(eb), std::max(ibp_chunk_items(B), 1));
}
size_t srx_ibp_u8lr_workspace_bytes_for(int eb, int B, int N, int h, int w, int H, int W, int f, const double *sh, const double *k, int kh,
                                        int kw, unsigned flags)
{
    if (!sh || !k || N <= 0 || N > SRX_MAX_FRAMES)
        return srx_ibp_u8lr_workspace_bytes(eb, B, N, h, w, H, W, f, flags);
    const IbpSpec spec = SRX_IBP_SPEC(eb);
    const Route r = route_ibp(spec);
    const size_t need = ibp_need(r, spec, B);
    if (r.status == SRX_OK && r.path == PATH_MOSAIC)
        return need;
    return need + u8_stage_bytes(spec, std::max(ibp_chunk_items(B), 1));
}

size_t srx_saa_items_workspace_bytes(int eb, int B, int N, int h, int w, int f) { return items::saa_ws_bound(SRX_SAA_SHAPE(eb), B); }
size_t srx_ibp_items_workspace_bytes(int eb, int B, int N, int h, int w, int H, int W, int f, unsigned flags)
{
    return items::ibp_ws_bound(SRX_IBP_SHAPE(eb), B, flags);
}
/* what THIS call carves: the largest run's need (a per-item "btile" run: its route's plus the tables of its items) */
size_t srx_ibp_items_workspace_bytes_for(int eb, int B, int N, int h, int w, int H, int W, int f, const double *sh, const double *k, int kh,
                                         int kw, unsigned flags)
{
    if (!sh || !k || N <= 0 || N > SRX_MAX_FRAMES || B <= 0)
        return items::ibp_ws_bound(SRX_IBP_SHAPE(eb), B, flags);
    const items::Plan p = items::plan_ibp(SRX_IBP_SPEC(eb), B);
    return p.status == SRX_OK ? p.need : items::ibp_ws_bound(SRX_IBP_SHAPE(eb), B, flags);
}

/* (true / 1 / 1 in the checks: the device pointers, the batch and the iterations that a query does not have) */
const char *srx_ibp_path_for(int eb, int N, int h, int w, int H, int W, int f, const double *sh, const double *k, int kh, int kw, unsigned flags)
{
    const IbpSpec spec = SRX_IBP_SPEC(eb);
    if ((eb != 4 && eb != 8) || ibp_check(spec, 1, 1, true) != SRX_OK)
        return "none";
    const Route r = route_ibp(spec);
    return r.status == SRX_OK ? r.name : "none";
}

int srx_ibp_patch_gstep_for(int N, int f, const double *sh)
{
    mosaic::AxisPlan py, px;
    if (!sh || N <= 0 || N > SRX_MAX_FRAMES || f < 2 || !mosaic::plan_axis(N, sh, 0, f, py) || !mosaic::plan_axis(N, sh, 1, f, px))
        return -1;
    unsigned long long ry[4], rx[4];
    return patch::gstep_form(py, px, N, f, ry, rx);
}

const char *srx_saa_path_for(int eb, int N, int h, int w, int f, const double *sh, unsigned flags)
{
    const SaaSpec spec{SRX_SAA_SHAPE(eb), sh, flags};
    if ((eb != 4 && eb != 8) || saa_check(spec, 1, true) != SRX_OK)
        return "none";
    const Route r = route_saa(spec);
    return r.status == SRX_OK ? r.name : "none";
}

int srx_decimate_u8(const uint8_t *in, int B, int H, int W, int f, int py, int px, uint8_t *out, srx_stream_t s)
{
    if (!in || !out || B <= 0 || f <= 0 || py < 0 || px < 0 || py >= H || px >= W)
        return SRX_E_INVALID;
    if (B > 65535)
        return SRX_E_UNSUPPORTED;
    const int h = cdiv(H - py, f), w = cdiv(W - px, f);
    hipLaunchKernelGGL(k_decimate<uint8_t>, dim3(cdiv(w, 64), cdiv(h, 4), B), dim3(64, 4), 0, hs(s), in, H, W, f, py, px, h, w, out);
    SRX_CHECK_LAUNCH();
    return SRX_OK;
}

int srx_mean_u8(const uint8_t *in, int B, int R, int H, int W, int f, int py, int px, int out_elem_bytes, void *out, srx_stream_t s)
{
    if (!in || !out || B <= 0 || R <= 0 || H <= 0 || W <= 0 || f <= 0 || py < 0 || px < 0 || py >= H || px >= W ||
        (out_elem_bytes != 4 && out_elem_bytes != 8))
        return SRX_E_INVALID;
    if (R > 65535 || B > 65535 || (size_t)R * H * W >= ((size_t)1 << 31))
        return SRX_E_UNSUPPORTED;
    return out_elem_bytes == 4 ? mean::mean_u8<float>(in, B, R, H, W, f, py, px, (float *)out, hs(s))
                               : mean::mean_u8<double>(in, B, R, H, W, f, py, px, (double *)out, hs(s));
}

int srx_patches_count(int n, int L, int stride) { return patches::grid_count(n, L, stride); }

int srx_patches_gather_u8(const uint8_t *frames, int B, int N, int h, int w, int ph, int pw, int sy, int sx, void *out, srx_stream_t s)
{
    return patches::gather<uint8_t>(frames, B, N, h, w, ph, pw, sy, sx, out, hs(s));
}
int srx_patches_gather_f32(const float *frames, int B, int N, int h, int w, int ph, int pw, int sy, int sx, void *out, srx_stream_t s)
{
    return patches::gather<float>(frames, B, N, h, w, ph, pw, sy, sx, out, hs(s));
}
int srx_patches_gather_f64(const double *frames, int B, int N, int h, int w, int ph, int pw, int sy, int sx, void *out, srx_stream_t s)
{
    return patches::gather<double>(frames, B, N, h, w, ph, pw, sy, sx, out, hs(s));
}
int srx_patches_blend_f32(const float *p, int B, int H, int W, int PH, int PW, int SY, int SX, int margin, void *out, srx_stream_t s)
{
    return patches::blend<float>(p, B, H, W, PH, PW, SY, SX, margin, out, hs(s));
}
int srx_patches_blend_f64(const double *p, int B, int H, int W, int PH, int PW, int SY, int SX, int margin, void *out, srx_stream_t s)
{
    return patches::blend<double>(p, B, H, W, PH, PW, SY, SX, margin, out, hs(s));
}

size_t srx_png_stream_bound(int H, int W) { return H > 0 && W > 0 ? png::stream_bound((size_t)H * ((size_t)W + 1)) : 0; }

size_t srx_png_scratch_bytes(int B, int H, int W) { return png::scratch_bytes(B, H, W); }

int srx_png_deflate_u8(const uint8_t *img, int B, int H, int W, void *streams, void *lengths, void *ws, size_t wsb, srx_stream_t s)
{
    return png::deflate(img, B, H, W, streams, lengths, ws, wsb, hs(s));
}
int srx_png_deflate_f32(const float *img, int B, int H, int W, void *streams, void *lengths, void *ws, size_t wsb, srx_stream_t s)
{
    return png::deflate(img, B, H, W, streams, lengths, ws, wsb, hs(s));
}
int srx_png_deflate_f64(const double *img, int B, int H, int W, void *streams, void *lengths, void *ws, size_t wsb, srx_stream_t s)
{
    return png::deflate(img, B, H, W, streams, lengths, ws, wsb, hs(s));
}

size_t srx_crc32_scratch_bytes(int B, size_t max_len) { return crc::scratch_bytes(B, max_len); }

int srx_crc32(const void *data, int B, size_t stride, size_t max_len, const void *lengths, uint32_t seed, void *crc_out, void *ws, size_t wsb,
              srx_stream_t s)
{
    return crc::crc32(data, B, stride, max_len, lengths, seed, crc_out, ws, wsb, hs(s));
}

size_t srx_png_file_bound(int H, int W) { return crc::file_bound(H, W); }

size_t srx_png_file_scratch_bytes(int B, int H, int W) { return crc::file_scratch_bytes(B, H, W); }

int srx_png_file_u8(const uint8_t *img, int B, int H, int W, void *files, void *lengths, void *ws, size_t wsb, srx_stream_t s)
{
    return crc::png_file(img, B, H, W, files, lengths, ws, wsb, hs(s));
}
int srx_png_file_f32(const float *img, int B, int H, int W, void *files, void *lengths, void *ws, size_t wsb, srx_stream_t s)
{
    return crc::png_file(img, B, H, W, files, lengths, ws, wsb, hs(s));
}
int srx_png_file_f64(const double *img, int B, int H, int W, void *files, void *lengths, void *ws, size_t wsb, srx_stream_t s)
{
    return crc::png_file(img, B, H, W, files, lengths, ws, wsb, hs(s));
}

// ---- include/srx_bayer.h ----
int srx_bayer_split_u8(const uint8_t *raw, int B, int H, int W, void *planes, srx_stream_t s) { return bayer::split(raw, B, H, W, planes, hs(s)); }
int srx_bayer_split_f32(const float *raw, int B, int H, int W, void *planes, srx_stream_t s) { return bayer::split(raw, B, H, W, planes, hs(s)); }
int srx_bayer_split_f64(const double *raw, int B, int H, int W, void *planes, srx_stream_t s) { return bayer::split(raw, B, H, W, planes, hs(s)); }

int srx_bayer_mean_u8(const uint8_t *raw, int B, int R, int H, int W, int out_elem_bytes, void *planes, srx_stream_t s)
{
    return bayer::mean_u8(raw, B, R, H, W, out_elem_bytes, planes, hs(s));
}

int srx_bayer_merge_f32(const float *planes, int B, int Hp, int Wp, int d, const double *gains, void *rgb, srx_stream_t s)
{
    return bayer::merge<float, false>(planes, B, Hp, Wp, d, gains, rgb, hs(s));
}
int srx_bayer_merge_f64(const double *planes, int B, int Hp, int Wp, int d, const double *gains, void *rgb, srx_stream_t s)
{
    return bayer::merge<double, false>(planes, B, Hp, Wp, d, gains, rgb, hs(s));
}
int srx_bayer_merge_rgb8_f32(const float *planes, int B, int Hp, int Wp, int d, const double *gains, void *rgb8, srx_stream_t s)
{
    return bayer::merge<float, true>(planes, B, Hp, Wp, d, gains, rgb8, hs(s));
}
int srx_bayer_merge_rgb8_f64(const double *planes, int B, int Hp, int Wp, int d, const double *gains, void *rgb8, srx_stream_t s)
{
    return bayer::merge<double, true>(planes, B, Hp, Wp, d, gains, rgb8, hs(s));
}

size_t srx_png_file_rgb8_bound(int H, int W) { return bayer::png_bound(H, W); }

size_t srx_png_file_rgb8_scratch_bytes(int B, int H, int W) { return bayer::png_scratch_bytes(B, H, W); }

int srx_png_file_rgb8(const uint8_t *img, int B, int H, int W, void *files, void *lengths, void *ws, size_t wsb, srx_stream_t s)
{
    return bayer::png_file(img, B, H, W, files, lengths, ws, wsb, hs(s));
}

int srx_interleave4_u8(const uint8_t *frames, int B, int h, int w, uint8_t *out, srx_stream_t s)
{
    if (!frames || !out || B <= 0 || h <= 0 || w <= 0)
        return SRX_E_INVALID;
    if (B > 65535)
        return SRX_E_UNSUPPORTED;
    hipLaunchKernelGGL(k_interleave4_u8, dim3(cdiv(2 * w, 64), cdiv(2 * h, 4), B), dim3(64, 4), 0, hs(s), frames, h, w, out);
    SRX_CHECK_LAUNCH();
    return SRX_OK;
}

size_t srx_metrics_workspace_bytes(int B, int H, int W, int nbin)
{
    return metrics::workspace_bytes(B, H, W, nbin);
}

int srx_edge_magnitude_f64(const double *roi, int H, int W, double sigma, double *mag, void *ws, size_t wsb, srx_stream_t s)
{
    return metrics::edge_magnitude(roi, H, W, sigma, mag, ws, wsb, hs(s));
}

int srx_edge_dist_range(int H, int W, double m, double b, double norm, int rows_are_x, double *out, srx_stream_t s)
{
    if (!out || H <= 0 || W <= 0 || !(norm > 0.0) || (size_t)H * W > (1u << 24))
        return SRX_E_INVALID;
    metrics::EdgeLine e{m, b, norm, 0.0, 0.25, rows_are_x, 1};
    hipLaunchKernelGGL(metrics::k_edge_dist_range, dim3(1), dim3(256), 0, hs(s), H, W, e, out);
    SRX_CHECK_LAUNCH();
    return SRX_OK;
}

#define SRX_DEFINE_METRICS(SFX, T)                                                                                                            \
    int srx_pair_moments_##SFX(const T *ref, const T *test, int B, int H, int W, int border, double *out, void *ws, size_t wsb, srx_stream_t s) \
    {                                                                                                                                         \
        return metrics::pair_moments<T>(ref, test, B, H, W, border, out, ws, wsb, hs(s));                                                      \
    }                                                                                                                                         \
    int srx_local_contrast_##SFX(const T *prof, int B, int n, int window, T *out, srx_stream_t s)                                             \
    {                                                                                                                                         \
        return metrics::local_contrast<T>(prof, B, n, window, out, hs(s));                                                                     \
    }                                                                                                                                         \
    int srx_ring_sums_##SFX(const T *img, int H, int W, double cy, double cx, int nbin, double *out, void *ws, size_t wsb, srx_stream_t s)      \
    {                                                                                                                                         \
        return metrics::ring_sums<T>(img, H, W, cy, cx, nbin, out, ws, wsb, hs(s));                                                            \
    }                                                                                                                                         \
    int srx_spot_moments_##SFX(const T *img, int H, int W, double *out, srx_stream_t s) { return metrics::spot_moments<T>(img, H, W, out, hs(s)); } \
    int srx_edge_bins_##SFX(const T *roi, int H, int W, double m, double b, double norm, int rows_are_x, double lo, double bw, int nbin,       \
                            double *out, void *ws, size_t wsb, srx_stream_t s)                                                                \
    {                                                                                                                                         \
        metrics::EdgeLine e{m, b, norm, lo, bw, rows_are_x, nbin};                                                                             \
        return metrics::edge_bins<T>(roi, H, W, e, out, ws, wsb, hs(s));                                                                       \
    }                                                                                                                                         \
    int srx_ssim_##SFX(const T *ref, const T *test, int B, int H, int W, int border, int radius, const double *taps, int sample_cov,          \
                       double data_range, double k1, double k2, const double *affine, double *mssim, T *map, void *ws, size_t wsb,           \
                       srx_stream_t s)                                                                                                        \
    {                                                                                                                                         \
        return metrics::ssim<T>(ref, test, B, H, W, border, radius, taps, sample_cov, data_range, k1, k2, affine, mssim, map, ws, wsb, hs(s)); \
    }
SRX_DEFINE_METRICS(f32, float)
SRX_DEFINE_METRICS(f64, double)

size_t srx_edge_sfr_scratch_bytes(int B, int H, int W) { return sfr::scratch_bytes(B, H, W); }

int srx_edge_sfr_u8(const uint8_t *img, int B, int H, int W, size_t row_pitch, size_t item_pitch, int side, double sigma, void *summary, void *esf,
                    void *mtf, void *status, void *ws, size_t wsb, srx_stream_t s)
{
    return sfr::edge_sfr(img, B, H, W, row_pitch, item_pitch, side, sigma, summary, esf, mtf, status, ws, wsb, hs(s));
}
int srx_edge_sfr_f32(const float *img, int B, int H, int W, size_t row_pitch, size_t item_pitch, int side, double sigma, void *summary, void *esf,
                     void *mtf, void *status, void *ws, size_t wsb, srx_stream_t s)
{
    return sfr::edge_sfr(img, B, H, W, row_pitch, item_pitch, side, sigma, summary, esf, mtf, status, ws, wsb, hs(s));
}
int srx_edge_sfr_f64(const double *img, int B, int H, int W, size_t row_pitch, size_t item_pitch, int side, double sigma, void *summary, void *esf,
                     void *mtf, void *status, void *ws, size_t wsb, srx_stream_t s)
{
    return sfr::edge_sfr(img, B, H, W, row_pitch, item_pitch, side, sigma, summary, esf, mtf, status, ws, wsb, hs(s));
}

size_t srx_register_workspace_bytes(int elem_bytes, int B, int N, int H, int W, int search)
{
    return reg::workspace_bytes(elem_bytes, B, N, H, W, search);
}
int srx_register_f32(const float *frames, int B, int N, int H, int W, int ref, const double *init_yx, int search, int border, int n_iter, double tol,
                     double *shifts, double *score, int *status, void *ws, size_t wsb, srx_stream_t s)
{
    return reg::register_frames<float, float>(frames, B, N, H, W, ref, init_yx, search, border, n_iter, tol, shifts, score, status, ws, wsb, hs(s));
}
int srx_register_f64(const double *frames, int B, int N, int H, int W, int ref, const double *init_yx, int search, int border, int n_iter,
                     double tol, double *shifts, double *score, int *status, void *ws, size_t wsb, srx_stream_t s)
{
    return reg::register_frames<double, double>(frames, B, N, H, W, ref, init_yx, search, border, n_iter, tol, shifts, score, status, ws, wsb, hs(s));
}
int srx_register_u8_f32(const uint8_t *frames, int B, int N, int H, int W, int ref, const double *init_yx, int search, int border, int n_iter,
                        double tol, double *shifts, double *score, int *status, void *ws, size_t wsb, srx_stream_t s)
{
    return reg::register_frames<float, uint8_t>(frames, B, N, H, W, ref, init_yx, search, border, n_iter, tol, shifts, score, status, ws, wsb, hs(s));
}
int srx_register_u8_f64(const uint8_t *frames, int B, int N, int H, int W, int ref, const double *init_yx, int search, int border, int n_iter,
                        double tol, double *shifts, double *score, int *status, void *ws, size_t wsb, srx_stream_t s)
{
    return reg::register_frames<double, uint8_t>(frames, B, N, H, W, ref, init_yx, search, border, n_iter, tol, shifts, score, status, ws, wsb, hs(s));
}

size_t srx_psf_estimate_workspace_bytes(int elem_bytes, int N, int H, int W, int halfwidth)
{
    return psf::workspace_bytes(elem_bytes, N, H, W, halfwidth);
}
int srx_psf_estimate_u8(const uint8_t *frames, int N, int H, int W, int halfwidth, double *out, int *info, void *ws, size_t wsb, srx_stream_t s)
{
    return psf::estimate<uint8_t>(frames, N, H, W, halfwidth, out, info, ws, wsb, hs(s));
}
int srx_psf_estimate_f32(const float *frames, int N, int H, int W, int halfwidth, double *out, int *info, void *ws, size_t wsb, srx_stream_t s)
{
    return psf::estimate<float>(frames, N, H, W, halfwidth, out, info, ws, wsb, hs(s));
}
int srx_psf_estimate_f64(const double *frames, int N, int H, int W, int halfwidth, double *out, int *info, void *ws, size_t wsb, srx_stream_t s)
{
    return psf::estimate<double>(frames, N, H, W, halfwidth, out, info, ws, wsb, hs(s));
}

#define SRX_DEFINE(SFX, T)                                                                                             \
    int srx_blur_##SFX(const T *img, int B, int H, int W, const double *k, int kh, int kw, T *out, srx_stream_t s)      \
    {                                                                                                                  \
        return blur<T>(img, B, H, W, k, kh, kw, false, out, hs(s));                                                    \
    }                                                                                                                  \
    int srx_shift_cubic_##SFX(const T *in, int B, int H, int W, double sy, double sx, T *out, void *ws, size_t wsb,     \
                              srx_stream_t s)                                                                          \
    {                                                                                                                  \
        return shift_cubic<T>(in, B, H, W, sy, sx, out, ws, wsb, hs(s));                                               \
    }                                                                                                                  \
    int srx_zoom_cubic_##SFX(const T *in, int B, int h, int w, int f, T *out, void *ws, size_t wsb, srx_stream_t s)     \
    {                                                                                                                  \
        return zoom_cubic<T>(in, B, h, w, f, out, ws, wsb, hs(s));                                                     \
    }                                                                                                                  \
    int srx_forward_##SFX(const T *hr, int B, int H, int W, const double *k, int kh, int kw, double sy, double sx,      \
                          int f, T *out, void *ws, size_t wsb, srx_stream_t s)                                         \
    {                                                                                                                  \
        return forward_model<T>(hr, B, H, W, k, kh, kw, sy, sx, f, out, ws, wsb, hs(s));                               \
    }                                                                                                                  \
    int srx_backproject_##SFX(const T *err, int B, int eh, int ew, const double *k, int kh, int kw, double sy,          \
                              double sx, int f, int H, int W, T *out, void *ws, size_t wsb, srx_stream_t s)            \
    {                                                                                                                  \
        return back_project<T>(err, B, eh, ew, k, kh, kw, sy, sx, f, H, W, out, ws, wsb, hs(s));                       \
    }                                                                                                                  \
    int srx_saa_##SFX(const T *lr, int B, int N, int h, int w, const double *sh, int f, T *out, void *ws, size_t wsb,   \
                      srx_stream_t s, unsigned flags)                                                                  \
    {                                                                                                                  \
        return saa_dispatch(SRX_SAA_CALL(T, T));                                                                       \
    }                                                                                                                  \
    int srx_ibp_##SFX(const T *lr, int B, int N, int h, int w, const double *sh, const double *k, int kh, int kw,       \
                      const T *hr_init, int H, int W, int f, int n_iter, double step, T *hr_out, double *errors,       \
                      void *ws, size_t wsb, srx_stream_t s, unsigned flags)                                            \
    {                                                                                                                  \
        return ibp_dispatch(SRX_IBP_CALL(T, T, n_iter, hr_out, errors));                                               \
    }                                                                                                                  \
    int srx_saa_items_##SFX(const T *lr, int B, int N, int h, int w, const double *sh, int f, T *out, void *ws,         \
                            size_t wsb, srx_stream_t s, unsigned flags)                                                \
    {                                                                                                                  \
        return items::saa_dispatch_items(SRX_SAA_CALL(T, T));                                                          \
    }                                                                                                                  \
    int srx_ibp_items_##SFX(const T *lr, int B, int N, int h, int w, const double *sh, const double *k, int kh, int kw, \
                            const T *hr_init, int H, int W, int f, int n_iter, double step, T *hr_out, double *errors, \
                            void *ws, size_t wsb, srx_stream_t s, unsigned flags)                                      \
    {                                                                                                                  \
        return items::ibp_dispatch_items(SRX_IBP_CALL(T, T, n_iter, hr_out, errors));                                  \
    }                                                                                                                  \
    int srx_saa_u8lr_##SFX(const uint8_t *lr, int B, int N, int h, int w, const double *sh, int f, T *out, void *ws,    \
                           size_t wsb, srx_stream_t s, unsigned flags)                                                 \
    {                                                                                                                  \
        return saa_dispatch(SRX_SAA_CALL(T, uint8_t));                                                                 \
    }                                                                                                                  \
    int srx_ibp_u8lr_##SFX(const uint8_t *lr, int B, int N, int h, int w, const double *sh, const double *k, int kh,   \
                           int kw, const T *hr_init, int H, int W, int f, int n_iter, double step, T *hr_out,          \
                           double *errors, void *ws, size_t wsb, srx_stream_t s, unsigned flags)                       \
    {                                                                                                                  \
        return ibp_dispatch(SRX_IBP_CALL(T, uint8_t, n_iter, hr_out, errors));                                         \
    }                                                                                                                  \
    int srx_decimate_##SFX(const T *in, int B, int H, int W, int f, int py, int px, T *out, srx_stream_t s)             \
    {                                                                                                                  \
        if (!in || !out || B <= 0 || f <= 0 || py < 0 || px < 0 || py >= H || px >= W)                                 \
            return SRX_E_INVALID;                                                                                      \
        if (B > 65535)                                                                                                 \
            return SRX_E_UNSUPPORTED;                                                                                  \
        const int h = cdiv(H - py, f), w = cdiv(W - px, f);                                                            \
        hipLaunchKernelGGL(k_decimate<T>, dim3(cdiv(w, 64), cdiv(h, 4), B), dim3(64, 4), 0, hs(s), in, H, W, f, py, px, \
                           h, w, out);                                                                                 \
        SRX_CHECK_LAUNCH();                                                                                            \
        return SRX_OK;                                                                                                 \
    }                                                                                                                  \
    int srx_zero_insert_##SFX(const T *in, int B, int eh, int ew, int f, int H, int W, T *out, srx_stream_t s)          \
    {                                                                                                                  \
        if (!in || !out || B <= 0 || f <= 0 || eh <= 0 || ew <= 0 || H <= 0 || W <= 0)                                 \
            return SRX_E_INVALID;                                                                                      \
        if (B > 65535)                                                                                                 \
            return SRX_E_UNSUPPORTED;                                                                                  \
        hipLaunchKernelGGL(k_zero_insert<T>, dim3(cdiv(W, 64), cdiv(H, 4), B), dim3(64, 4), 0, hs(s), in, eh, ew, f, H, \
                           W, out);                                                                                    \
        SRX_CHECK_LAUNCH();                                                                                            \
        return SRX_OK;                                                                                                 \
    }                                                                                                                  \
    int srx_mean_frames_##SFX(const T *in, int B, int R, size_t n, T *out, srx_stream_t s)                              \
    {                                                                                                                  \
        if (!in || !out || B <= 0 || R <= 0 || n == 0)                                                                 \
            return SRX_E_INVALID;                                                                                      \
        if (B > 65535)                                                                                                 \
            return SRX_E_UNSUPPORTED;                                                                                  \
        hipLaunchKernelGGL(k_mean_frames<T>, dim3((unsigned)((n + 255) / 256), B), dim3(256), 0, hs(s), in, R, n, out); \
        SRX_CHECK_LAUNCH();                                                                                            \
        return SRX_OK;                                                                                                 \
    }                                                                                                                  \
    int srx_u8_to_##SFX(const uint8_t *in, size_t n, T *out, srx_stream_t s)                                            \
    {                                                                                                                  \
        if (!in || !out || n == 0)                                                                                     \
            return SRX_E_INVALID;                                                                                      \
        hipLaunchKernelGGL(k_u8_to<T>, dim3(grid1d(n)), dim3(256), 0, hs(s), in, n, out);                              \
        SRX_CHECK_LAUNCH();                                                                                            \
        return SRX_OK;                                                                                                 \
    }                                                                                                                  \
    int srx_quantize_u8_##SFX(const T *in, size_t n, uint8_t *out, srx_stream_t s)                                      \
    {                                                                                                                  \
        if (!in || !out || n == 0)                                                                                     \
            return SRX_E_INVALID;                                                                                      \
        hipLaunchKernelGGL(k_quantize_u8<T>, dim3(grid1d(n)), dim3(256), 0, hs(s), in, n, out);                        \
        SRX_CHECK_LAUNCH();                                                                                            \
        return SRX_OK;                                                                                                 \
    }

SRX_DEFINE(f32, float)
SRX_DEFINE(f64, double)

}  // extern "C"
