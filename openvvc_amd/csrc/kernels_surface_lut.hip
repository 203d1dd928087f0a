// Surface output through a colour table, on the device (include/ovvc_hip.h, "Surface output through a colour table"): the decoded
// picture to R'G'B' at 10 bits, through the 3D colour table, back to Y'CbCr with the destination's matrix, sub-sampled to 4:2:0 at the
// destination's chroma location and stored as an NV12 / P010 / I420 / I010 surface -- one launch, no intermediate picture.  The refusals
// and the coefficients are the host twin's (ovvc_surface_lut.c: ovhip_surface_lut_plan_make_, on top of the RGB and the surface plans).
//
// k_surface_lut is k_rgb_lut's item (kernels_rgb_lut.hip): a lane owns 8 horizontally adjacent luma columns of an output row pair and
// the 4 chroma pairs under them.  It loads each chroma plane's 3 x 6 taps once and walks the luma rows one after another (not
// unrolled: one row of addresses, texels and converted values is live at a time): blend, matrix at 10 bits, clip, the row's texel
// addresses, its gathers issued together, tetrahedral interpolation, the normalising division (ovhip_reduce_div_'s estimate and one
// correction: no 64-bit division), the forward matrix.  The row's 8 luma samples leave at once; its Cb14 and Cr14 go, filtered
// horizontally and weighted by the row, into four accumulators per chroma plane, which leave after the last row.  Where the
// destination's chroma is horizontally co-sited (HC) the item has a ninth column to the left of its 8, where it is vertically top
// (a.vt) a third row above its 2; column -1 and row -1 of the WINDOW are clamped to column 0 and row 0 -- luma outside the window is
// never read, and an even W and H leave nothing to clamp on the right or below.  The halo makes up to 9/8 * 3/2 of k_rgb_lut's gathers.
// The source side (arguments, chroma and luma row loads, the pixel) and the table side (lut_point, lut_mix) are colour_stage.hip.h's,
// shared with k_rgb_lut and k_rgb; what is here is the row loop with its halo, the order -- addresses, gathers, mix --, the way back, the
// stores, and the vertical blend: as a function of the header (over the rows' arrays, or one column at a time) it saved 10 VGPRs and made
// a smooth 4K picture 3 to 7 us slower where the halo column is on (55.7 -> 62.1, 76.3 -> 83.8: LABBOOK 36).  Stores through run_io.hip.h
// with the values of surface_values.hip.h: which path a run takes depends on its address alone.  The rounding mode and the vertical
// location are launch arguments (uniform branches), the rest template arguments.
//
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage; FMT x A x HC, 16 instantiations):
//   HC = 0 (centred):   A = 0: NV12 126, I420 125, P010 128, I010 127 VGPRs; A = 1: 139, 138, 139, 132
//   HC = 1 (co-sited):  A = 0: NV12 149, I420 148, P010 149, I010 148 VGPRs; A = 1: 149, 148, 150, 147
//   106 SGPRs, no scratch, no LDS in all of them; 3 waves per SIMD (the four of HC = 0, A = 0: 4).  k_rgb_lut: 118-168 VGPRs, 3-4 waves.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include "ovvc_hip.h"
#include "ovvc_common.hip.h"
#include "ovvc_dpb_priv.h"
#include "ovvc_surface_lut_priv.h"
#include "run_io.hip.h"
#include "surface_values.hip.h"
#include "colour_stage.hip.h"

namespace {

struct SlDst {
    char *dst[3];                         // the planes of the surface (semi-planar: [1] is the interleaved plane, [2] unused)
    size_t pitch_y, pitch_c;              // bytes
    int fwd[9], yoff16;                   // forward matrix: y_r y_g y_b, b_r b_g b_b, r_r r_g r_b; 16 yoff of the destination
    int vt, dither;                       // destination vertically top; OVHIP_SURF_DITHER
    unsigned P; float rcp;                // the table's peak, 1.0f / P
};

// 4 elements of one byte each (a planar 8-bit chroma run: half of what run_store's smallest run holds)
__device__ __forceinline__ void store4_u8(char *p, uint32_t w, int n)
{
    if (n == 4 && ((uintptr_t)p & 3) == 0) *reinterpret_cast<uint32_t *>(p) = w;
    else {
#pragma unroll
        for (int e = 0; e < 4; ++e) if (e < n) *reinterpret_cast<uint8_t *>(p + e) = (uint8_t)(w >> (8 * e));
    }
}

template <int FMT, int A, int HC>
__global__ __launch_bounds__(COL_NT) void k_surface_lut(ColSrc a, SlDst d, LutArgs l)
{
    constexpr bool SEMI = FMT == OVHIP_SURF_NV12 || FMT == OVHIP_SURF_P010;
    constexpr int ES = (FMT == OVHIP_SURF_P010 || FMT == OVHIP_SURF_I010) ? 2 : 1;
    constexpr int NC = COL_RUN + HC;                                // columns converted per row; column i of the run is c = i + HC
    const unsigned item = blockIdx.x * COL_NT + threadIdx.x;
    if (item >= a.n_items) return;
    const int rp = (int)(item / (unsigned)a.groups), g = (int)(item - (unsigned)rp * (unsigned)a.groups);
    const int ox = g * COL_RUN, n = min(COL_RUN, a.W - ox);          // n: 2, 4, 6 or 8
    const bool full = n == COL_RUN;
    const int px = a.x0 + ox, py = a.y0 + 2 * rp;                  // both even
    const int cbase = px >> 1, k = py >> 1;

    // source chroma rows k - 1, k, k + 1 (clamped) x columns cbase - 1 .. cbase + 4 (clamped)
    int cbv[3][6], crv[3][6];
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        const size_t ro = (size_t)min(max(k - 1 + t, 0), a.ch - 1) * (size_t)a.stride_c;
        chroma_row<1>(a.cb + ro, cbase, a.cw, full, cbv[t]);
        chroma_row<1>(a.cr + ro, cbase, a.cw, full, crv[t]);
    }

    const int s_all = l.S2 + l.S + 1;                              // from a cell's vertex to the opposite corner
    int accb[COL_RUN / 2] = {}, accr[COL_RUN / 2] = {};              // sums of w_x w_y C14 of the 4 chroma pairs
#pragma unroll 1
    for (int rr = d.vt ? -1 : 0; rr < 2; ++rr) {
        const int r = (rr < 0 && rp == 0) ? 0 : rr;                // window row -1 is row 0
        int Y[NC], ub[6], vb[6];
        const uint16_t *yrow = a.y + (size_t)(py + r) * (size_t)a.stride_y + px;
        luma_row(yrow, full, n, Y + HC);
        if constexpr (HC) Y[0] = ox ? yrow[-1] : yrow[0];          // (window column -1 is never read: its value is column 0's, below)
        // vertical blend: V = 2 (2k + r) - b = 4k + (2r - b), so j0 = k + ((2r - b) >> 2) and fy = (2r - b) & 3
        const int dv = 2 * r - a.b, fy = dv & 3, t0 = 1 + (dv >> 2);       // t0: 0 or 1, the same in every lane
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            const int ulo = t0 ? cbv[1][i] : cbv[0][i], uhi = t0 ? cbv[2][i] : cbv[1][i];
            const int vlo = t0 ? crv[1][i] : crv[0][i], vhi = t0 ? crv[2][i] : crv[1][i];
            ub[i] = (4 - fy) * ulo + fy * uhi;
            vb[i] = (4 - fy) * vlo + fy * vhi;
        }
        // the row's cells, weights and its texel addresses
        LutPoint p[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            int R, G, B;
            col_pixel<A>(a, ub, vb, c - HC, Y[c], 1023, R, G, B);
            p[c] = lut_point(R, G, B, l);
        }
        // the row's gathers, all in flight together
        uint2 t0v[NC], t1v[NC], t2v[NC], t3v[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            t0v[c] = l.texels[p[c].v0]; t1v[c] = l.texels[p[c].v1]; t2v[c] = l.texels[p[c].v2]; t3v[c] = l.texels[p[c].v0 + s_all];
        }
        // interpolation, normalise, forward matrix
        int cb14[NC], cr14[NC];
        uint32_t yv[COL_RUN / 2] = {};                              // the row's luma samples, two to a dword
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            uint32_t oR, oG, oB;
            lut_mix(p[c].w1, p[c].w2, p[c].w3, t0v[c], t1v[c], t2v[c], t3v[c], oR, oG, oB);
            const int qr = ovhip_surface_lut_norm_(oR, d.P, d.rcp), qg = ovhip_surface_lut_norm_(oG, d.P, d.rcp), qb = ovhip_surface_lut_norm_(oB, d.P, d.rcp);
            cb14[c] = 8192 + ovhip_surface_lut_row_(d.fwd + 3, qr, qg, qb);
            cr14[c] = 8192 + ovhip_surface_lut_row_(d.fwd + 6, qr, qg, qb);
            if (c >= HC) {
                const int y14 = d.yoff16 + ovhip_surface_lut_row_(d.fwd, qr, qg, qb);
                run_put<2, COL_RUN / 2>(yv, c - HC, (uint32_t)ov_clip3((y14 + 8) >> 4, 0, 1023));
            }
        }
        if constexpr (HC) if (ox == 0) { cb14[0] = cb14[1]; cr14[0] = cr14[1]; }      // window column -1 is column 0
        // the row's share of the 4 chroma pairs: taps 2m - 1, 2m, 2m + 1 (1 2 1) or 2m, 2m + 1 (2 2); the row's weight 1 2 1 or 2 2
        const int wy = (d.vt && rr != 0) ? 1 : 2;
#pragma unroll
        for (int m = 0; m < COL_RUN / 2; ++m) {
            const int c = 2 * m + HC;
            const int hb = HC ? cb14[c - 1] + 2 * cb14[c] + cb14[c + 1] : 2 * (cb14[c] + cb14[c + 1]);
            const int hr = HC ? cr14[c - 1] + 2 * cr14[c] + cr14[c + 1] : 2 * (cr14[c] + cr14[c + 1]);
            accb[m] += wy * hb; accr[m] += wy * hr;
        }
        // the luma row (the row above the pair belongs to the item above: it is only this item's halo)
        if (rr >= 0) {
            const int row = 2 * rp + rr;
            const uint32_t thr = surf_thr(d.dither != 0, row);
            char *out = d.dst[0] + (size_t)row * d.pitch_y + (size_t)ox * ES;
#pragma unroll
            for (int j = 0; j < COL_RUN / 2; ++j) yv[j] = surf_pair<FMT>(yv[j], thr);
            if constexpr (ES == 2) run_store<2, COL_RUN>(out, yv, n);
            else {
                uint32_t o8[COL_RUN / 4];
#pragma unroll
                for (int j = 0; j < COL_RUN / 4; ++j) o8[j] = narrow4(yv[2 * j], yv[2 * j + 1]);
                run_store<1, COL_RUN>(out, o8, n);
            }
        }
    }

    // the 4 chroma pairs of output chroma row rp, columns ox / 2 .. ox / 2 + 3 (even first: the dither's column parity is the pair's)
    const uint32_t thr = surf_thr(d.dither != 0, rp);
    uint32_t pb[COL_RUN / 4], pr[COL_RUN / 4];
#pragma unroll
    for (int j = 0; j < COL_RUN / 4; ++j) {
        const uint32_t b0 = (uint32_t)ov_clip3((accb[2 * j] + 128) >> 8, 0, 1023), b1 = (uint32_t)ov_clip3((accb[2 * j + 1] + 128) >> 8, 0, 1023);
        const uint32_t r0 = (uint32_t)ov_clip3((accr[2 * j] + 128) >> 8, 0, 1023), r1 = (uint32_t)ov_clip3((accr[2 * j + 1] + 128) >> 8, 0, 1023);
        pb[j] = surf_pair<FMT>(b0 | (b1 << 16), thr);
        pr[j] = surf_pair<FMT>(r0 | (r1 << 16), thr);
    }
    if constexpr (SEMI) {
        uint32_t v[COL_RUN / 2];
#pragma unroll
        for (int j = 0; j < COL_RUN / 4; ++j) surf_interleave(pb[j], pr[j], &v[2 * j], &v[2 * j + 1]);
        char *out = d.dst[1] + (size_t)rp * d.pitch_c + (size_t)ox * ES;          // (n elements: n / 2 pairs)
        if constexpr (ES == 2) run_store<2, COL_RUN>(out, v, n);
        else {
            uint32_t o8[COL_RUN / 4];
#pragma unroll
            for (int j = 0; j < COL_RUN / 4; ++j) o8[j] = narrow4(v[2 * j], v[2 * j + 1]);
            run_store<1, COL_RUN>(out, o8, n);
        }
    } else {
        const size_t at = (size_t)rp * d.pitch_c + (size_t)(ox >> 1) * ES;
        if constexpr (ES == 2) {
            run_store<2, COL_RUN / 2>(d.dst[1] + at, pb, n >> 1);
            run_store<2, COL_RUN / 2>(d.dst[2] + at, pr, n >> 1);
        } else {
            store4_u8(d.dst[1] + at, narrow4(pb[0], pb[1]), n >> 1);
            store4_u8(d.dst[2] + at, narrow4(pr[0], pr[1]), n >> 1);
        }
    }
}

struct SlLaunch { ColSrc a; SlDst d; LutArgs l; };

template <int FMT, int A> void sl_launch_h(const SlLaunch &q, int hc, hipStream_t st)
{
    const unsigned wgs = (q.a.n_items + COL_NT - 1) / COL_NT;
    if (hc) hipLaunchKernelGGL((k_surface_lut<FMT, A, 1>), dim3(wgs), dim3(COL_NT), 0, st, q.a, q.d, q.l);
    else    hipLaunchKernelGGL((k_surface_lut<FMT, A, 0>), dim3(wgs), dim3(COL_NT), 0, st, q.a, q.d, q.l);
}
template <int FMT> void sl_launch_a(const SlLaunch &q, int A, int hc, hipStream_t st)
{
    if (A) sl_launch_h<FMT, 1>(q, hc, st); else sl_launch_h<FMT, 0>(q, hc, st);
}

} // namespace

extern "C" int ovhip_surface_lut_launch(ovhip_ctx *ctx, const ovhip_pic *pic, const ovhip_window *win, const ovhip_surface_conv *conv, const ovhip_surface_format *fmt,
                                        const ovhip_rgb_lut *lut, void *d_dst, size_t dst_bytes)
{
    if (!ctx) return OVHIP_EINVAL;
    OV_DEVICE(ctx);
    ovhip_surface_lut_plan_ p;
    const char *why = "";
    int r = ovhip_surface_lut_plan_make_(pic, win, conv, fmt, lut ? lut->size : 0, lut ? lut->peak : 0, lut != NULL, d_dst, dst_bytes, &p, &why);
    if (r == OVHIP_OK && lut->device != ctx->device) { why = "the table lives on another device"; r = OVHIP_EINVAL; p.surf.bytes = 0; }
    if (r != OVHIP_OK) {
        const char *code = r == OVHIP_EUNSUP ? "unsupported" : "invalid argument";
        if (p.surf.bytes && dst_bytes < p.surf.bytes)
            snprintf(ctx->err, sizeof(ctx->err), "ovhip_surface_lut_launch: %s: %zu bytes given, the surface needs %zu: %s", why, dst_bytes, p.surf.bytes, code);
        else snprintf(ctx->err, sizeof(ctx->err), "ovhip_surface_lut_launch: %s: %s", why, code);
        return r;
    }
    SlLaunch q;
    if (!col_src_fill(q.a, pic, p.rgb)) return ov_fail(ctx, OVHIP_EINVAL, "ovhip_surface_lut_launch: picture too large", hipSuccess);
    SlDst &d = q.d;
    for (int k = 0; k < 3; ++k) d.dst[k] = (char *)d_dst + p.surf.off[k < p.surf.n_planes ? k : 1];
    d.pitch_y = p.surf.pitch[0]; d.pitch_c = p.surf.pitch[1];
    for (int k = 0; k < 9; ++k) d.fwd[k] = p.coef[k];
    d.yoff16 = 16 * p.yoff;
    d.vt = p.vt; d.dither = p.surf.dither;
    d.P = (unsigned)lut->peak; d.rcp = 1.0f / (float)lut->peak;
    q.l = lut_args_fill(lut);
    switch (fmt->format) {
    case OVHIP_SURF_NV12: sl_launch_a<OVHIP_SURF_NV12>(q, p.rgb.a, p.hc, ctx->stream); break;
    case OVHIP_SURF_I420: sl_launch_a<OVHIP_SURF_I420>(q, p.rgb.a, p.hc, ctx->stream); break;
    case OVHIP_SURF_P010: sl_launch_a<OVHIP_SURF_P010>(q, p.rgb.a, p.hc, ctx->stream); break;
    default:              sl_launch_a<OVHIP_SURF_I010>(q, p.rgb.a, p.hc, ctx->stream); break;
    }
    OV_LAUNCH_CHECK(ctx, "k_surface_lut");
    return OVHIP_OK;
}

extern "C" int ovhip_pic_output_surface_lut(ovhip_ctx *ctx, const ovhip_pic *pic, const ovhip_window *win, const ovhip_surface_conv *conv, const ovhip_surface_format *fmt,
                                            const ovhip_rgb_lut *lut, void *host_dst, size_t dst_bytes)
{
    if (!ctx || !pic || !conv || !fmt || !host_dst) return OVHIP_EINVAL;
    OV_DEVICE(ctx);
    const size_t bytes = ovhip_surface_bytes(pic->w, pic->h, win, fmt);
    if (!bytes || dst_bytes < bytes) {
        /* no size, or a host_dst that is too small: the launch refuses both before it looks at the pointer, and words the reason */
        const int q = ovhip_surface_lut_launch(ctx, pic, win, conv, fmt, lut, host_dst, dst_bytes);
        return q != OVHIP_OK ? q : OVHIP_EINVAL;
    }
    int r = ov_scratch(ctx, bytes, 0);
    if (r != OVHIP_OK) return r;
    char *d = (char *)ctx->scratch_d;
    r = ovhip_surface_lut_launch(ctx, pic, win, conv, fmt, lut, d, bytes);
    if (r != OVHIP_OK) return r;
    ovhip_surface_plan_ p;
    (void)ovhip_surface_plan_make_(pic, win, fmt, d, bytes, &p, nullptr);      // (accepted a line above)
    /* the rows' own bytes only: what lies between them in host memory stays as it was */
    hipError_t e = hipSuccess;
    for (int k = 0; k < p.n_planes && e == hipSuccess; ++k)
        e = hipMemcpy2DAsync((char *)host_dst + p.off[k], p.pitch[k], d + p.off[k], p.pitch[k], (size_t)p.elems[k] * p.es, (size_t)p.rows[k],
                             hipMemcpyDeviceToHost, ctx->stream);
    if (e != hipSuccess) return ov_fail(ctx, OVHIP_ENODEV, "ovhip_pic_output_surface_lut: D2H", e);
    if (ov_sync_stream(ctx) != hipSuccess) return ov_fail(ctx, OVHIP_ELAUNCH, "ovhip_pic_output_surface_lut", hipGetLastError());
    return OVHIP_OK;
}
