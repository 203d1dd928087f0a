// RGB output through a colour table, on the device (include/ovvc_hip.h, "RGB output through a colour table"): k_rgb's conversion
// with one table-driven step between its clip and its store -- a 3D colour lookup table of 17, 33 or 65 points per axis,
// interpolated tetrahedrally in integers.  The refusals and the coefficients are the host twin's (ovvc_rgb_lut.c:
// ovhip_rgb_lut_plan_make_, on top of ovvc_rgb.c's plan).
//
// k_rgb_lut is k_rgb's item (kernels_rgb.hip): a lane owns 8 horizontally adjacent output pixels of a row pair, loads each chroma
// plane's 3 x 6 taps once, blends, applies the matrix (at 10 bits whatever the dtype) and the clip.  The chroma and matrix code is a
// COPY of k_rgb's, not shared with it: moved into a common header, with a row's 24 clipped values handed over at once (which the
// gathers below need), ten of the sixteen k_rgb instantiations took 1 to 10 more VGPRs and four lost a wave of occupancy.  Unlike
// k_rgb this is no pure stream: a pixel makes four 8-byte gathers, at addresses its own value decides, from the texel array (R, G, B,
// 0 per lattice point; 39 KB, 287 KB or 2.2 MB: resident in the XCD's L2 beside the streamed picture), with plain loads.  A row's 32
// addresses are computed first and its 32 loads issued together; the order of the three fractions is three compares, the vertex steps
// are selects of the strides 1, S and S^2 by those compares: no data-dependent branch.  Stores as k_rgb's, by the run's address alone
// (run_io.hip.h).  A table of 17 points staged in LDS was tried and is not here: slower on the pictures a decoder makes (LABBOOK 30).
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <stdint.h>
#include <stdlib.h>
#include "ovvc_hip.h"
#include "ovvc_common.hip.h"
#include "ovvc_dpb_priv.h"
#include "ovvc_rgb_lut_priv.h"
#include "run_io.hip.h"

namespace {

#define RGB_NT  256
#define RGB_RUN 8            /* pixels of a row per lane */

struct RgbArgs {
    const uint16_t *y, *cb, *cr;
    char *dst;
    int stride_y, stride_c, cw, ch;       // (cw x ch: the chroma plane of the WHOLE picture, where the taps clamp)
    int x0, y0, W, H, groups;             // the window's first luma sample, the output size, runs per row
    int b;                                // V = 2y - b   (U = 2x - A: the kernel's template argument)
    int cy16, rv, gu, gv, bu, yoff;       // cy16 = 16 cy; the clip is to 0..1023
    unsigned n_items;                     // groups * H / 2
};

struct LutArgs {
    const uint2 *texels;                  // [S^3]: x = R | G << 16, y = B
    int S, S2, n;                         // points per axis, S^2, S - 1
    float to_unit;                        // (float)(1.0 / P)
};

template <int DT> struct ElemBytes { static constexpr int v = DT == OVHIP_RGB_U8 ? 1 : (DT == OVHIP_RGB_F32 ? 4 : 2); };

// the stored bits of one interpolated value
template <int DT> __device__ __forceinline__ uint32_t lut_bits(uint32_t o, float to_unit)
{
    if constexpr (DT == OVHIP_RGB_U8 || DT == OVHIP_RGB_U16) return o;
    else {
        const float f = __fmul_rn((float)o, to_unit);                      // one multiplication, round to nearest, nothing to contract with
        if constexpr (DT == OVHIP_RGB_F32) return __float_as_uint(f);
        else return (uint32_t)__half_as_ushort(__float2half_rn(f));        // (round to nearest even, subnormal halves included)
    }
}

// one chroma row's 6 columns cbase - 1 .. cbase + 4, clamped to the plane (A == 0 never reads the first)
template <int A> __device__ __forceinline__ void chroma_row(const uint16_t *row, int cbase, int cw, bool full, int (&c)[6])
{
    if (full && (((uintptr_t)(row + cbase)) & 7) == 0) {          // (a full run: cbase + 3 <= cw - 1)
        const uint2 v = *reinterpret_cast<const uint2 *>(row + cbase);
        c[1] = (int)(v.x & 0xFFFFu); c[2] = (int)(v.x >> 16); c[3] = (int)(v.y & 0xFFFFu); c[4] = (int)(v.y >> 16);
    } else {
#pragma unroll
        for (int t = 1; t < 5; ++t) c[t] = row[min(cbase - 1 + t, cw - 1)];
    }
    c[0] = A ? (int)row[max(cbase - 1, 0)] : 0;
    c[5] = row[min(cbase + 4, cw - 1)];
}

// a channel value 0..1023 -> its cell index 0..n - 1 and its fraction 0..1023 (v = 1023: the last cell's far end)
__device__ __forceinline__ void lut_cell(int v, int n, int &i, int &f)
{
    const unsigned t = (unsigned)(v * n);
    const unsigned q = t / 1023u;
    const bool top = q == (unsigned)n;
    i = top ? n - 1 : (int)q;
    f = top ? 1023 : (int)(t - 1023u * q);
}

template <int DT, int PACKED, int A>
__global__ __launch_bounds__(RGB_NT) void k_rgb_lut(RgbArgs a, LutArgs l)
{
    constexpr int ES = ElemBytes<DT>::v;
    const unsigned item = blockIdx.x * RGB_NT + threadIdx.x;
    if (item >= a.n_items) return;
    const int rp = (int)(item / (unsigned)a.groups), g = (int)(item - (unsigned)rp * (unsigned)a.groups);
    const int ox = g * RGB_RUN, n = min(RGB_RUN, a.W - ox);
    const bool full = n == RGB_RUN;
    const int px = a.x0 + ox, py = a.y0 + 2 * rp;                  // both even
    const int cbase = px >> 1, k = py >> 1;

    // chroma rows k - 1, k, k + 1 (clamped) x columns cbase - 1 .. cbase + 4 (clamped); b == 0 reads only k and k + 1
    int cbv[3][6], crv[3][6];
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        if (t == 0 && a.b == 0) {
#pragma unroll
            for (int i = 0; i < 6; ++i) { cbv[0][i] = 0; crv[0][i] = 0; }
            continue;
        }
        const size_t ro = (size_t)min(max(k - 1 + t, 0), a.ch - 1) * (size_t)a.stride_c;
        chroma_row<A>(a.cb + ro, cbase, a.cw, full, cbv[t]);
        chroma_row<A>(a.cr + ro, cbase, a.cw, full, crv[t]);
    }

    const size_t plane = (size_t)a.W * (size_t)a.H;
    const int s_all = l.S2 + l.S + 1;                              // from a cell's vertex to the opposite corner
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        // luma
        int Y[RGB_RUN];
        const uint16_t *yrow = a.y + (size_t)(py + r) * (size_t)a.stride_y + px;
        if (full && ((uintptr_t)yrow & 15) == 0) {
            const uint4 v = *reinterpret_cast<const uint4 *>(yrow);
            Y[0] = (int)(v.x & 0xFFFFu); Y[1] = (int)(v.x >> 16); Y[2] = (int)(v.y & 0xFFFFu); Y[3] = (int)(v.y >> 16);
            Y[4] = (int)(v.z & 0xFFFFu); Y[5] = (int)(v.z >> 16); Y[6] = (int)(v.w & 0xFFFFu); Y[7] = (int)(v.w >> 16);
        } else {
#pragma unroll
            for (int i = 0; i < RGB_RUN; ++i) Y[i] = yrow[min(i, n - 1)];
        }
        // vertical blend: V = 2 (2k + r) - b = 4k + (2r - b), so j0 = k + ((2r - b) >> 2) and fy = (2r - b) & 3
        const int d = 2 * r - a.b, fy = d & 3, t0 = 1 + (d >> 2);          // t0: 0 or 1, the same in every lane
        int ub[6], vb[6];
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            const int ulo = t0 ? cbv[1][i] : cbv[0][i], uhi = t0 ? cbv[2][i] : cbv[1][i];
            const int vlo = t0 ? crv[1][i] : crv[0][i], vhi = t0 ? crv[2][i] : crv[1][i];
            ub[i] = (4 - fy) * ulo + fy * uhi;
            vb[i] = (4 - fy) * vlo + fy * vhi;
        }
        // horizontal blend, matrix, clip; then the row's cells, weights and its 32 texel addresses.  The clip to 0..1023 is what
        // keeps every index inside the table: a cell index is at most n - 1, so the opposite corner is at most S^3 - 1
        int w1[RGB_RUN], w2[RGB_RUN], w3[RGB_RUN];                          // (w0 = 1023 - w1 - w2 - w3)
        int v0[RGB_RUN], v1[RGB_RUN], v2[RGB_RUN];                          // (the opposite corner: v0 + s_all)
#pragma unroll
        for (int i = 0; i < RGB_RUN; ++i) {
            const int q = 2 * i - A + 4, idx = q >> 2, fx = q & 3;          // column idx of the 6 <-> cbase - 1 + idx
            const int u = (4 - fx) * ub[idx] + fx * ub[idx + 1] - 8192;
            const int v = (4 - fx) * vb[idx] + fx * vb[idx + 1] - 8192;
            const int L = a.cy16 * (Y[i] - a.yoff) + (1 << 17);
            const int R = ov_clip3((L + a.rv * v) >> 18, 0, 1023);
            const int G = ov_clip3((L - a.gu * u - a.gv * v) >> 18, 0, 1023);
            const int B = ov_clip3((L + a.bu * u) >> 18, 0, 1023);
            int ir, ig, ib, fr, fg, fb;
            lut_cell(R, l.n, ir, fr); lut_cell(G, l.n, ig, fg); lut_cell(B, l.n, ib, fb);
            // the order of (fraction descending, channel ascending): a total order, so the first and the last channel differ
            const bool rg = fr >= fg, rb = fr >= fb, gb = fg >= fb;
            const int s_first = (rg && rb) ? 1 : ((!rg && gb) ? l.S : l.S2);
            const int s_last = (!rg && !rb) ? 1 : ((rg && !gb) ? l.S : l.S2);
            const int f1 = max(fr, max(fg, fb)), f3 = min(fr, min(fg, fb)), f2 = fr + fg + fb - f1 - f3;
            w1[i] = f1 - f2; w2[i] = f2 - f3; w3[i] = f3;
            v0[i] = (ib * l.S + ig) * l.S + ir;
            v1[i] = v0[i] + s_first;
            v2[i] = v0[i] + s_all - s_last;
        }
        // the row's gathers, all in flight together
        uint2 t0v[RGB_RUN], t1v[RGB_RUN], t2v[RGB_RUN], t3v[RGB_RUN];
#pragma unroll
        for (int i = 0; i < RGB_RUN; ++i) {
            t0v[i] = l.texels[v0[i]]; t1v[i] = l.texels[v1[i]]; t2v[i] = l.texels[v2[i]]; t3v[i] = l.texels[v0[i] + s_all];
        }
        // interpolation, pack
        constexpr int NWP = RGB_RUN * ES / 4, NWK = PACKED ? 3 * NWP : 1;          // dwords of a plane's run / of the packed run
        uint32_t wr[NWP] = {}, wg[NWP] = {}, wb[NWP] = {}, wk[NWK] = {};
#pragma unroll
        for (int i = 0; i < RGB_RUN; ++i) {
            const uint32_t c0 = (uint32_t)(1023 - w1[i] - w2[i] - w3[i]), c1 = (uint32_t)w1[i], c2 = (uint32_t)w2[i], c3 = (uint32_t)w3[i];
            // (at most 1023 * 65535 + 511 < 2^26)
            const uint32_t oR = (c0 * (t0v[i].x & 0xFFFFu) + c1 * (t1v[i].x & 0xFFFFu) + c2 * (t2v[i].x & 0xFFFFu) + c3 * (t3v[i].x & 0xFFFFu) + 511u) / 1023u;
            const uint32_t oG = (c0 * (t0v[i].x >> 16) + c1 * (t1v[i].x >> 16) + c2 * (t2v[i].x >> 16) + c3 * (t3v[i].x >> 16) + 511u) / 1023u;
            const uint32_t oB = (c0 * (t0v[i].y & 0xFFFFu) + c1 * (t1v[i].y & 0xFFFFu) + c2 * (t2v[i].y & 0xFFFFu) + c3 * (t3v[i].y & 0xFFFFu) + 511u) / 1023u;
            const uint32_t R = lut_bits<DT>(oR, l.to_unit), G = lut_bits<DT>(oG, l.to_unit), B = lut_bits<DT>(oB, l.to_unit);
            if constexpr (PACKED) {
                run_put<ES, NWK>(wk, 3 * i, R); run_put<ES, NWK>(wk, 3 * i + 1, G); run_put<ES, NWK>(wk, 3 * i + 2, B);
            } else {
                run_put<ES, NWP>(wr, i, R); run_put<ES, NWP>(wg, i, G); run_put<ES, NWP>(wb, i, B);
            }
        }
        const size_t at = (size_t)(2 * rp + r) * (size_t)a.W + (size_t)ox;
        if constexpr (PACKED) {
            run_store<ES, 3 * RGB_RUN>(a.dst + at * 3 * ES, wk, 3 * n);
        } else {
            run_store<ES, RGB_RUN>(a.dst + at * ES, wr, n);
            run_store<ES, RGB_RUN>(a.dst + (plane + at) * ES, wg, n);
            run_store<ES, RGB_RUN>(a.dst + (2 * plane + at) * ES, wb, n);
        }
    }
}

template <int DT, int PACKED> void lut_launch_a(const RgbArgs &a, const LutArgs &l, int A, hipStream_t st)
{
    const unsigned wgs = (a.n_items + RGB_NT - 1) / RGB_NT;
    if (A) hipLaunchKernelGGL((k_rgb_lut<DT, PACKED, 1>), dim3(wgs), dim3(RGB_NT), 0, st, a, l);
    else   hipLaunchKernelGGL((k_rgb_lut<DT, PACKED, 0>), dim3(wgs), dim3(RGB_NT), 0, st, a, l);
}
template <int DT> void lut_launch_l(const RgbArgs &a, const LutArgs &l, int packed, int A, hipStream_t st)
{
    if (packed) lut_launch_a<DT, 1>(a, l, A, st); else lut_launch_a<DT, 0>(a, l, A, st);
}

} // namespace

extern "C" int ovhip_rgb_lut_on_ctx_(const ovhip_rgb_lut *lut, const ovhip_ctx *ctx) { return lut && ctx && lut->device == ctx->device; }

extern "C" int ovhip_rgb_lut_create(ovhip_ctx *ctx, int size, int peak, const uint16_t *host_table, ovhip_rgb_lut **out)
{
    if (out) *out = NULL;
    if (!ctx || !out) return OVHIP_EINVAL;
    OV_DEVICE(ctx);
    if (ovhip_rgb_lut_check(size, peak, NULL) != OVHIP_OK)
        return ov_fail(ctx, OVHIP_EINVAL, "ovhip_rgb_lut_create: table size must be 17, 33 or 65 and its peak 1..65535", hipSuccess);
    if (!host_table) return ov_fail(ctx, OVHIP_EINVAL, "ovhip_rgb_lut_create: null table", hipSuccess);
    const int64_t bad = ovhip_rgb_lut_first_above_(size, peak, host_table);
    if (bad >= 0) {
        const int64_t c = bad % 3, ri = bad / 3 % size, gi = bad / 3 / size % size, bi = bad / 3 / size / size;
        snprintf(ctx->err, sizeof(ctx->err), "ovhip_rgb_lut_create: entry [%lld][%lld][%lld][%lld] (index %lld) is %u, above the peak %d: invalid argument",
                 (long long)bi, (long long)gi, (long long)ri, (long long)c, (long long)bad, (unsigned)host_table[bad], peak);
        return OVHIP_EINVAL;
    }
    const size_t bytes = (size_t)size * size * size * 8;
    ovhip_rgb_lut *lut = (ovhip_rgb_lut *)calloc(1, sizeof(*lut));
    uint16_t *texels = (uint16_t *)malloc(bytes);
    if (!lut || !texels) { free(lut); free(texels); return ov_fail(ctx, OVHIP_ENOMEM, "ovhip_rgb_lut_create: malloc", hipSuccess); }
    ovhip_rgb_lut_repack_(size, host_table, texels);
    lut->device = ctx->device; lut->size = size; lut->peak = peak;
    hipError_t e = hipMalloc(&lut->d_texels, bytes);
    int r = e == hipSuccess ? OVHIP_OK : ov_fail(ctx, OVHIP_ENOMEM, "hipMalloc(colour table)", e);
    if (r == OVHIP_OK) {
        /* once, and waited for: the staging block is freed below, and any context of this device may read the table afterwards */
        e = hipMemcpyAsync(lut->d_texels, texels, bytes, hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = ov_sync_stream(ctx);
        if (e != hipSuccess) r = ov_fail(ctx, OVHIP_ENODEV, "hipMemcpyAsync(colour table)", e);
    }
    free(texels);
    if (r != OVHIP_OK) { if (lut->d_texels) (void)hipFree(lut->d_texels); free(lut); return r; }
    *out = lut;
    return OVHIP_OK;
}

extern "C" void ovhip_rgb_lut_destroy(ovhip_rgb_lut *lut)
{
    if (!lut) return;
    if (lut->d_texels && hipSetDevice(lut->device) == hipSuccess) (void)hipFree(lut->d_texels);
    free(lut);
}

extern "C" int ovhip_rgb_lut_launch(ovhip_ctx *ctx, const ovhip_pic *pic, const ovhip_window *win, const ovhip_rgb_format *fmt, const ovhip_rgb_lut *lut,
                                    void *d_dst, size_t dst_bytes)
{
    if (!ctx || !pic || !fmt) return OVHIP_EINVAL;
    OV_DEVICE(ctx);
    ovhip_rgb_plan_ p;
    const char *why = "";
    int r = ovhip_rgb_lut_plan_make_(pic, win, fmt, lut ? lut->size : 0, lut ? lut->peak : 0, lut != NULL, d_dst, dst_bytes, &p, &why);
    if (r == OVHIP_OK && lut->device != ctx->device) { why = "the table lives on another device"; r = OVHIP_EINVAL; }
    if (r != OVHIP_OK) {
        snprintf(ctx->err, sizeof(ctx->err), "ovhip_rgb_lut_launch: %s: %s", why, r == OVHIP_EUNSUP ? "unsupported" : "invalid argument");
        return r;
    }
    RgbArgs a;
    a.y = pic->y; a.cb = pic->cb; a.cr = pic->cr; a.dst = (char *)d_dst;
    a.stride_y = pic->stride_y; a.stride_c = pic->stride_c; a.cw = pic->w / 2; a.ch = pic->h / 2;
    a.x0 = p.x0; a.y0 = p.y0; a.W = p.W; a.H = p.H; a.groups = (p.W + RGB_RUN - 1) / RGB_RUN;
    a.b = p.b;
    a.cy16 = 16 * p.coef[0]; a.rv = p.coef[1]; a.gu = p.coef[2]; a.gv = p.coef[3]; a.bu = p.coef[4]; a.yoff = p.yoff;
    const size_t items = (size_t)a.groups * (size_t)(p.H / 2);
    if (items > 0x7FFFFFFFu) return ov_fail(ctx, OVHIP_EINVAL, "ovhip_rgb_lut_launch: picture too large", hipSuccess);
    a.n_items = (unsigned)items;
    LutArgs l;
    l.texels = (const uint2 *)lut->d_texels; l.S = lut->size; l.S2 = lut->size * lut->size; l.n = lut->size - 1;
    l.to_unit = (float)(1.0 / lut->peak);
    switch (fmt->dtype) {
    case OVHIP_RGB_U8:  lut_launch_l<OVHIP_RGB_U8>(a, l, fmt->layout, p.a, ctx->stream); break;
    case OVHIP_RGB_U16: lut_launch_l<OVHIP_RGB_U16>(a, l, fmt->layout, p.a, ctx->stream); break;
    case OVHIP_RGB_F16: lut_launch_l<OVHIP_RGB_F16>(a, l, fmt->layout, p.a, ctx->stream); break;
    default:            lut_launch_l<OVHIP_RGB_F32>(a, l, fmt->layout, p.a, ctx->stream); break;
    }
    OV_LAUNCH_CHECK(ctx, "k_rgb_lut");
    return OVHIP_OK;
}

extern "C" int ovhip_pic_output_rgb_lut(ovhip_ctx *ctx, const ovhip_pic *pic, const ovhip_window *win, const ovhip_rgb_format *fmt, const ovhip_rgb_lut *lut,
                                        void *host_dst, size_t dst_bytes)
{
    if (!ctx || !pic || !fmt || !host_dst) return OVHIP_EINVAL;
    OV_DEVICE(ctx);
    const size_t bytes = ovhip_rgb_bytes(pic->w, pic->h, win, fmt);
    if (!bytes || dst_bytes < bytes) {
        /* no size, or a host_dst that is too small: the launch refuses both before it looks at the pointer, and words the reason */
        const int q = ovhip_rgb_lut_launch(ctx, pic, win, fmt, lut, host_dst, dst_bytes);
        return q != OVHIP_OK ? q : OVHIP_EINVAL;
    }
    int r = ov_scratch(ctx, bytes, 0);
    if (r == OVHIP_OK) r = ovhip_rgb_lut_launch(ctx, pic, win, fmt, lut, ctx->scratch_d, bytes);
    if (r == OVHIP_OK) r = ovhip_d2h(ctx, host_dst, ctx->scratch_d, bytes);
    return r;
}
