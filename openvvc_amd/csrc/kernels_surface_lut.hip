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
// The chroma and matrix code is a COPY of k_rgb_lut's, as that one's is of k_rgb's (its header says what sharing cost); both files
// are untouched.  Stores through run_io.hip.h with the values of surface_values.hip.h: which path a run takes depends on its address
// alone.  The rounding mode and the vertical location are launch arguments (uniform branches), the rest template arguments.
//
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage; FMT x A x HC, 16 instantiations):
//   HC = 0 (centred):   A = 0: NV12 131, I420 131, P010 127, I010 127 VGPRs; A = 1: 140, 140, 139, 139
//   HC = 1 (co-sited):  A = 0: NV12 148, I420 148, P010 149, I010 149 VGPRs; A = 1: 147, 147, 149, 148
//   106 SGPRs, no scratch, no LDS in all of them; 3 waves per SIMD (the two of 127 VGPRs: 4).  k_rgb_lut: 109-163 VGPRs, 3-4 waves.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include "ovvc_hip.h"
#include "ovvc_common.hip.h"
#include "ovvc_dpb_priv.h"
#include "ovvc_surface_lut_priv.h"
#include "run_io.hip.h"
#include "surface_values.hip.h"

namespace {

#define SL_NT  256
#define SL_RUN 8             /* luma columns of a row per lane */

struct SlArgs {
    const uint16_t *y, *cb, *cr;
    char *dst[3];                         // the planes of the surface (semi-planar: [1] is the interleaved plane, [2] unused)
    size_t pitch_y, pitch_c;              // bytes
    int stride_y, stride_c, cw, ch;       // (cw x ch: the chroma plane of the WHOLE picture, where the source's taps clamp)
    int x0, y0, W, H, groups;             // the window's first luma sample, the output size, runs per row
    int b;                                // source: V = 2y - b   (U = 2x - A: the kernel's template argument)
    int cy16, rv, gu, gv, bu, yoff;       // source matrix; cy16 = 16 cy; the clip is to 0..1023
    int fwd[9], yoff16;                   // forward matrix: y_r y_g y_b, b_r b_g b_b, r_r r_g r_b; 16 yoff of the destination
    int vt, dither;                       // destination vertically top; OVHIP_SURF_DITHER
    unsigned P; float rcp;                // the table's peak, 1.0f / P
    unsigned n_items;                     // groups * H / 2
};

struct LutArgs {
    const uint2 *texels;                  // [S^3]: x = R | G << 16, y = B
    int S, S2, n;                         // points per axis, S^2, S - 1
};

// one chroma row's 6 columns cbase - 1 .. cbase + 4, clamped to the plane
__device__ __forceinline__ void chroma_row(const uint16_t *row, int cbase, int cw, bool full, int (&c)[6])
{
    if (full && (((uintptr_t)(row + cbase)) & 7) == 0) {          // (a full run: cbase + 3 <= cw - 1)
        const uint2 v = *reinterpret_cast<const uint2 *>(row + cbase);
        c[1] = (int)(v.x & 0xFFFFu); c[2] = (int)(v.x >> 16); c[3] = (int)(v.y & 0xFFFFu); c[4] = (int)(v.y >> 16);
    } else {
#pragma unroll
        for (int t = 1; t < 5; ++t) c[t] = row[min(cbase - 1 + t, cw - 1)];
    }
    c[0] = row[max(cbase - 1, 0)];
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
__global__ __launch_bounds__(SL_NT) void k_surface_lut(SlArgs a, LutArgs l)
{
    constexpr bool SEMI = FMT == OVHIP_SURF_NV12 || FMT == OVHIP_SURF_P010;
    constexpr int ES = (FMT == OVHIP_SURF_P010 || FMT == OVHIP_SURF_I010) ? 2 : 1;
    constexpr int NC = SL_RUN + HC;                                // columns converted per row; column i of the run is c = i + HC
    const unsigned item = blockIdx.x * SL_NT + threadIdx.x;
    if (item >= a.n_items) return;
    const int rp = (int)(item / (unsigned)a.groups), g = (int)(item - (unsigned)rp * (unsigned)a.groups);
    const int ox = g * SL_RUN, n = min(SL_RUN, a.W - ox);          // n: 2, 4, 6 or 8
    const bool full = n == SL_RUN;
    const int px = a.x0 + ox, py = a.y0 + 2 * rp;                  // both even
    const int cbase = px >> 1, k = py >> 1;

    // source chroma rows k - 1, k, k + 1 (clamped) x columns cbase - 1 .. cbase + 4 (clamped)
    int cbv[3][6], crv[3][6];
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        const size_t ro = (size_t)min(max(k - 1 + t, 0), a.ch - 1) * (size_t)a.stride_c;
        chroma_row(a.cb + ro, cbase, a.cw, full, cbv[t]);
        chroma_row(a.cr + ro, cbase, a.cw, full, crv[t]);
    }

    const int s_all = l.S2 + l.S + 1;                              // from a cell's vertex to the opposite corner
    int accb[SL_RUN / 2] = {}, accr[SL_RUN / 2] = {};              // sums of w_x w_y C14 of the 4 chroma pairs
#pragma unroll 1
    for (int rr = a.vt ? -1 : 0; rr < 2; ++rr) {
        const int r = (rr < 0 && rp == 0) ? 0 : rr;                // window row -1 is row 0
        // luma
        int Y[NC];
        const uint16_t *yrow = a.y + (size_t)(py + r) * (size_t)a.stride_y + px;
        if (full && ((uintptr_t)yrow & 15) == 0) {
            const uint4 v = *reinterpret_cast<const uint4 *>(yrow);
            Y[HC + 0] = (int)(v.x & 0xFFFFu); Y[HC + 1] = (int)(v.x >> 16); Y[HC + 2] = (int)(v.y & 0xFFFFu); Y[HC + 3] = (int)(v.y >> 16);
            Y[HC + 4] = (int)(v.z & 0xFFFFu); Y[HC + 5] = (int)(v.z >> 16); Y[HC + 6] = (int)(v.w & 0xFFFFu); Y[HC + 7] = (int)(v.w >> 16);
        } else {
#pragma unroll
            for (int i = 0; i < SL_RUN; ++i) Y[HC + i] = yrow[min(i, n - 1)];
        }
        if constexpr (HC) Y[0] = ox ? yrow[-1] : yrow[0];          // (window column -1 is never read: its value is column 0's, below)
        // vertical blend: V = 2 (2k + r) - b = 4k + (2r - b), so j0 = k + ((2r - b) >> 2) and fy = (2r - b) & 3
        const int d = 2 * r - a.b, fy = d & 3, t0 = 1 + (d >> 2);  // t0: 0 or 1
        int ub[6], vb[6];
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            const int ulo = t0 ? cbv[1][i] : cbv[0][i], uhi = t0 ? cbv[2][i] : cbv[1][i];
            const int vlo = t0 ? crv[1][i] : crv[0][i], vhi = t0 ? crv[2][i] : crv[1][i];
            ub[i] = (4 - fy) * ulo + fy * uhi;
            vb[i] = (4 - fy) * vlo + fy * vhi;
        }
        // horizontal blend, matrix, clip; then the row's cells, weights and its texel addresses.  The clip to 0..1023 is what keeps
        // every index inside the table: a cell index is at most n - 1, so the opposite corner is at most S^3 - 1
        int w1[NC], w2[NC], w3[NC];                                // (w0 = 1023 - w1 - w2 - w3)
        int v0[NC], v1[NC], v2[NC];                                // (the opposite corner: v0 + s_all)
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const int i = c - HC;                                  // -1 .. 7
            const int q = 2 * i - A + 4, idx = q >> 2, fx = q & 3; // column idx of the 6 <-> cbase - 1 + idx  (i = -1: q = 2 - A, idx = 0)
            const int u = (4 - fx) * ub[idx] + fx * ub[idx + 1] - 8192;
            const int v = (4 - fx) * vb[idx] + fx * vb[idx + 1] - 8192;
            const int L = a.cy16 * (Y[c] - a.yoff) + (1 << 17);
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
            w1[c] = f1 - f2; w2[c] = f2 - f3; w3[c] = f3;
            v0[c] = (ib * l.S + ig) * l.S + ir;
            v1[c] = v0[c] + s_first;
            v2[c] = v0[c] + s_all - s_last;
        }
        // the row's gathers, all in flight together
        uint2 t0v[NC], t1v[NC], t2v[NC], t3v[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            t0v[c] = l.texels[v0[c]]; t1v[c] = l.texels[v1[c]]; t2v[c] = l.texels[v2[c]]; t3v[c] = l.texels[v0[c] + s_all];
        }
        // interpolation, normalise, forward matrix
        int cb14[NC], cr14[NC];
        uint32_t yv[SL_RUN / 2] = {};                              // the row's luma samples, two to a dword
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const uint32_t c0 = (uint32_t)(1023 - w1[c] - w2[c] - w3[c]), c1 = (uint32_t)w1[c], c2 = (uint32_t)w2[c], c3 = (uint32_t)w3[c];
            // (at most 1023 * 65535 + 511 < 2^26)
            const uint32_t oR = (c0 * (t0v[c].x & 0xFFFFu) + c1 * (t1v[c].x & 0xFFFFu) + c2 * (t2v[c].x & 0xFFFFu) + c3 * (t3v[c].x & 0xFFFFu) + 511u) / 1023u;
            const uint32_t oG = (c0 * (t0v[c].x >> 16) + c1 * (t1v[c].x >> 16) + c2 * (t2v[c].x >> 16) + c3 * (t3v[c].x >> 16) + 511u) / 1023u;
            const uint32_t oB = (c0 * (t0v[c].y & 0xFFFFu) + c1 * (t1v[c].y & 0xFFFFu) + c2 * (t2v[c].y & 0xFFFFu) + c3 * (t3v[c].y & 0xFFFFu) + 511u) / 1023u;
            const int qr = ovhip_surface_lut_norm_(oR, a.P, a.rcp), qg = ovhip_surface_lut_norm_(oG, a.P, a.rcp), qb = ovhip_surface_lut_norm_(oB, a.P, a.rcp);
            cb14[c] = 8192 + ovhip_surface_lut_row_(a.fwd + 3, qr, qg, qb);
            cr14[c] = 8192 + ovhip_surface_lut_row_(a.fwd + 6, qr, qg, qb);
            if (c >= HC) {
                const int y14 = a.yoff16 + ovhip_surface_lut_row_(a.fwd, qr, qg, qb);
                run_put<2, SL_RUN / 2>(yv, c - HC, (uint32_t)ov_clip3((y14 + 8) >> 4, 0, 1023));
            }
        }
        if constexpr (HC) if (ox == 0) { cb14[0] = cb14[1]; cr14[0] = cr14[1]; }      // window column -1 is column 0
        // the row's share of the 4 chroma pairs: taps 2m - 1, 2m, 2m + 1 (1 2 1) or 2m, 2m + 1 (2 2); the row's weight 1 2 1 or 2 2
        const int wy = (a.vt && rr != 0) ? 1 : 2;
#pragma unroll
        for (int m = 0; m < SL_RUN / 2; ++m) {
            const int c = 2 * m + HC;
            const int hb = HC ? cb14[c - 1] + 2 * cb14[c] + cb14[c + 1] : 2 * (cb14[c] + cb14[c + 1]);
            const int hr = HC ? cr14[c - 1] + 2 * cr14[c] + cr14[c + 1] : 2 * (cr14[c] + cr14[c + 1]);
            accb[m] += wy * hb; accr[m] += wy * hr;
        }
        // the luma row (the row above the pair belongs to the item above: it is only this item's halo)
        if (rr >= 0) {
            const int row = 2 * rp + rr;
            const uint32_t thr = surf_thr(a.dither != 0, row);
            char *out = a.dst[0] + (size_t)row * a.pitch_y + (size_t)ox * ES;
#pragma unroll
            for (int j = 0; j < SL_RUN / 2; ++j) yv[j] = surf_pair<FMT>(yv[j], thr);
            if constexpr (ES == 2) run_store<2, SL_RUN>(out, yv, n);
            else {
                uint32_t o8[SL_RUN / 4];
#pragma unroll
                for (int j = 0; j < SL_RUN / 4; ++j) o8[j] = narrow4(yv[2 * j], yv[2 * j + 1]);
                run_store<1, SL_RUN>(out, o8, n);
            }
        }
    }

    // the 4 chroma pairs of output chroma row rp, columns ox / 2 .. ox / 2 + 3 (even first: the dither's column parity is the pair's)
    const uint32_t thr = surf_thr(a.dither != 0, rp);
    uint32_t pb[SL_RUN / 4], pr[SL_RUN / 4];
#pragma unroll
    for (int j = 0; j < SL_RUN / 4; ++j) {
        const uint32_t b0 = (uint32_t)ov_clip3((accb[2 * j] + 128) >> 8, 0, 1023), b1 = (uint32_t)ov_clip3((accb[2 * j + 1] + 128) >> 8, 0, 1023);
        const uint32_t r0 = (uint32_t)ov_clip3((accr[2 * j] + 128) >> 8, 0, 1023), r1 = (uint32_t)ov_clip3((accr[2 * j + 1] + 128) >> 8, 0, 1023);
        pb[j] = surf_pair<FMT>(b0 | (b1 << 16), thr);
        pr[j] = surf_pair<FMT>(r0 | (r1 << 16), thr);
    }
    if constexpr (SEMI) {
        uint32_t v[SL_RUN / 2];
#pragma unroll
        for (int j = 0; j < SL_RUN / 4; ++j) surf_interleave(pb[j], pr[j], &v[2 * j], &v[2 * j + 1]);
        char *out = a.dst[1] + (size_t)rp * a.pitch_c + (size_t)ox * ES;          // (n elements: n / 2 pairs)
        if constexpr (ES == 2) run_store<2, SL_RUN>(out, v, n);
        else {
            uint32_t o8[SL_RUN / 4];
#pragma unroll
            for (int j = 0; j < SL_RUN / 4; ++j) o8[j] = narrow4(v[2 * j], v[2 * j + 1]);
            run_store<1, SL_RUN>(out, o8, n);
        }
    } else {
        const size_t at = (size_t)rp * a.pitch_c + (size_t)(ox >> 1) * ES;
        if constexpr (ES == 2) {
            run_store<2, SL_RUN / 2>(a.dst[1] + at, pb, n >> 1);
            run_store<2, SL_RUN / 2>(a.dst[2] + at, pr, n >> 1);
        } else {
            store4_u8(a.dst[1] + at, narrow4(pb[0], pb[1]), n >> 1);
            store4_u8(a.dst[2] + at, narrow4(pr[0], pr[1]), n >> 1);
        }
    }
}

template <int FMT, int A> void sl_launch_h(const SlArgs &a, const LutArgs &l, int hc, hipStream_t st)
{
    const unsigned wgs = (a.n_items + SL_NT - 1) / SL_NT;
    if (hc) hipLaunchKernelGGL((k_surface_lut<FMT, A, 1>), dim3(wgs), dim3(SL_NT), 0, st, a, l);
    else    hipLaunchKernelGGL((k_surface_lut<FMT, A, 0>), dim3(wgs), dim3(SL_NT), 0, st, a, l);
}
template <int FMT> void sl_launch_a(const SlArgs &a, const LutArgs &l, int A, int hc, hipStream_t st)
{
    if (A) sl_launch_h<FMT, 1>(a, l, hc, st); else sl_launch_h<FMT, 0>(a, l, hc, st);
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
    SlArgs a;
    a.y = pic->y; a.cb = pic->cb; a.cr = pic->cr;
    for (int q = 0; q < 3; ++q) a.dst[q] = (char *)d_dst + p.surf.off[q < p.surf.n_planes ? q : 1];
    a.pitch_y = p.surf.pitch[0]; a.pitch_c = p.surf.pitch[1];
    a.stride_y = pic->stride_y; a.stride_c = pic->stride_c; a.cw = pic->w / 2; a.ch = pic->h / 2;
    a.x0 = p.rgb.x0; a.y0 = p.rgb.y0; a.W = p.rgb.W; a.H = p.rgb.H; a.groups = (p.rgb.W + SL_RUN - 1) / SL_RUN;
    a.b = p.rgb.b;
    a.cy16 = 16 * p.rgb.coef[0]; a.rv = p.rgb.coef[1]; a.gu = p.rgb.coef[2]; a.gv = p.rgb.coef[3]; a.bu = p.rgb.coef[4]; a.yoff = p.rgb.yoff;
    for (int q = 0; q < 9; ++q) a.fwd[q] = p.coef[q];
    a.yoff16 = 16 * p.yoff;
    a.vt = p.vt; a.dither = p.surf.dither;
    a.P = (unsigned)lut->peak; a.rcp = 1.0f / (float)lut->peak;
    const size_t items = (size_t)a.groups * (size_t)(p.rgb.H / 2);
    if (items > 0x7FFFFFFFu) return ov_fail(ctx, OVHIP_EINVAL, "ovhip_surface_lut_launch: picture too large", hipSuccess);
    a.n_items = (unsigned)items;
    LutArgs l;
    l.texels = (const uint2 *)lut->d_texels; l.S = lut->size; l.S2 = lut->size * lut->size; l.n = lut->size - 1;
    switch (fmt->format) {
    case OVHIP_SURF_NV12: sl_launch_a<OVHIP_SURF_NV12>(a, l, p.rgb.a, p.hc, ctx->stream); break;
    case OVHIP_SURF_I420: sl_launch_a<OVHIP_SURF_I420>(a, l, p.rgb.a, p.hc, ctx->stream); break;
    case OVHIP_SURF_P010: sl_launch_a<OVHIP_SURF_P010>(a, l, p.rgb.a, p.hc, ctx->stream); break;
    default:              sl_launch_a<OVHIP_SURF_I010>(a, l, p.rgb.a, p.hc, ctx->stream); break;
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
