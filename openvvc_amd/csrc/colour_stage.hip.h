// colour_stage.hip.h -- the stages of the colour outputs that more than one kernel runs, each written once: the SOURCE side of k_rgb
// (kernels_rgb.hip), k_rgb_lut (kernels_rgb_lut.hip) and k_surface_lut (kernels_surface_lut.hip) -- a 4:2:0 picture's chroma taps, its
// luma row, the horizontal blend at the signalled sample location, the matrix in 14-bit integer coefficients and the clip -- and the
// TABLE side of the latter two: a 10-bit R'G'B' triple through a 3D colour table, interpolated tetrahedrally in integers.  Definitions:
// include/ovvc_hip.h, "RGB output on the device" and "RGB output through a colour table"; the host twins' share: ovvc_outdst_priv.h.
//
// The grain is one chroma row, one luma row, one PIXEL: every function here is inlined into a kernel's own loops, and a kernel keeps its
// loops, the order "a row's addresses, then all its gathers, then the mix" and its stores.  (A coarser grain -- a row's 24 clipped
// values handed to a functor -- cost k_rgb registers and waves: LABBOOK 30.)  The VERTICAL blend of the 6 columns is not here: as a
// function, over the rows' arrays or one column at a time, it made k_rgb_lut 2 us and k_surface_lut up to 7 us slower per 4K picture
// and cost k_rgb a wave, so each kernel writes those eight lines out; k_rgb writes its luma load out too (LABBOOK 36).
// A function of this file is optimised BEFORE it is inlined, so the compiler meets a kernel's loops in another order than with the same
// text written in place: every change here goes through the resource table and the timing of LABBOOK 36 again.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ovvc_hip.h"
#include "ovvc_common.hip.h"
#include "ovvc_dpb_priv.h"
#include "ovvc_rgb_lut_priv.h"

namespace {

#define COL_NT  256
#define COL_RUN 8            /* pixels of a row per lane */

template <int DT> struct RgbElemBytes { static constexpr int v = DT == OVHIP_RGB_U8 ? 1 : (DT == OVHIP_RGB_F32 ? 4 : 2); };

// ---- source side ----

struct ColSrc {
    const uint16_t *y, *cb, *cr;
    int stride_y, stride_c, cw, ch;       // (cw x ch: the chroma plane of the WHOLE picture, where the taps clamp)
    int x0, y0, W, H, groups;             // the window's first luma sample, the output size, runs per row
    int b;                                // V = 2y - b   (U = 2x - A: the kernels' template argument)
    int cy16, rv, gu, gv, bu, yoff;       // cy16 = 16 cy
    unsigned n_items;                     // groups * H / 2
};

// the source of a launch from the picture and its plan; false: more items than a grid holds ("picture too large")
inline bool col_src_fill(ColSrc &a, const ovhip_pic *pic, const ovhip_rgb_plan_ &p)
{
    a.y = pic->y; a.cb = pic->cb; a.cr = pic->cr;
    a.stride_y = pic->stride_y; a.stride_c = pic->stride_c; a.cw = pic->w / 2; a.ch = pic->h / 2;
    a.x0 = p.x0; a.y0 = p.y0; a.W = p.W; a.H = p.H; a.groups = (p.W + COL_RUN - 1) / COL_RUN;
    a.b = p.b;
    a.cy16 = 16 * p.coef[0]; a.rv = p.coef[1]; a.gu = p.coef[2]; a.gv = p.coef[3]; a.bu = p.coef[4]; a.yoff = p.yoff;
    const size_t items = (size_t)a.groups * (size_t)(p.H / 2);
    a.n_items = (unsigned)items;
    return items <= 0x7FFFFFFFu;
}

// the synchronous convenience of an RGB output: launch(dst, bytes) into the context's scratch, then the tensor's copy to the host
template <class L> int rgb_output_host(ovhip_ctx *ctx, const ovhip_pic *pic, const ovhip_window *win, const ovhip_rgb_format *fmt, void *host_dst, size_t dst_bytes, L launch)
{
    const size_t bytes = ovhip_rgb_bytes(pic->w, pic->h, win, fmt);
    if (!bytes || dst_bytes < bytes) {
        /* no size, or a host_dst that is too small: the launch refuses both before it looks at the pointer, and words the reason */
        const int q = launch(host_dst, dst_bytes);
        return q != OVHIP_OK ? q : OVHIP_EINVAL;
    }
    int r = ov_scratch(ctx, bytes, 0);
    if (r == OVHIP_OK) r = launch(ctx->scratch_d, bytes);
    if (r == OVHIP_OK) r = ovhip_d2h(ctx, host_dst, ctx->scratch_d, bytes);
    return r;
}

// one chroma row's 6 columns cbase - 1 .. cbase + 4, clamped to the plane; LEFT: the first is read (else it is never used)
template <int LEFT> __device__ __forceinline__ void chroma_row(const uint16_t *row, int cbase, int cw, bool full, int (&c)[6])
{
    if (full && (((uintptr_t)(row + cbase)) & 7) == 0) {          // (a full run: cbase + 3 <= cw - 1)
        const uint2 v = *reinterpret_cast<const uint2 *>(row + cbase);
        c[1] = (int)(v.x & 0xFFFFu); c[2] = (int)(v.x >> 16); c[3] = (int)(v.y & 0xFFFFu); c[4] = (int)(v.y >> 16);
    } else {
#pragma unroll
        for (int t = 1; t < 5; ++t) c[t] = row[min(cbase - 1 + t, cw - 1)];
    }
    c[0] = LEFT ? (int)row[max(cbase - 1, 0)] : 0;
    c[5] = row[min(cbase + 4, cw - 1)];
}

// a run's 8 luma samples (sample n - 1 repeated behind a tail of n): one 16-byte load where the run is full and aligned, else elements
__device__ __forceinline__ void luma_row(const uint16_t *yrow, bool full, int n, int *Y)
{
    if (full && ((uintptr_t)yrow & 15) == 0) {
        const uint4 v = *reinterpret_cast<const uint4 *>(yrow);
        Y[0] = (int)(v.x & 0xFFFFu); Y[1] = (int)(v.x >> 16); Y[2] = (int)(v.y & 0xFFFFu); Y[3] = (int)(v.y >> 16);
        Y[4] = (int)(v.z & 0xFFFFu); Y[5] = (int)(v.z >> 16); Y[6] = (int)(v.w & 0xFFFFu); Y[7] = (int)(v.w >> 16);
    } else {
#pragma unroll
        for (int i = 0; i < COL_RUN; ++i) Y[i] = yrow[min(i, n - 1)];
    }
}

// pixel i of the run (-1: the column left of it) with luma sample y, over the row's 6 vertically blended columns ub, vb (4 times the
// sample): horizontal blend, matrix, clip to 0..peak
template <int A> __device__ __forceinline__ void col_pixel(const ColSrc &a, const int (&ub)[6], const int (&vb)[6], int i, int y, int peak, int &R, int &G, int &B)
{
    const int q = 2 * i - A + 4, idx = q >> 2, fx = q & 3;          // column idx of the 6 <-> cbase - 1 + idx  (i = -1: q = 2 - A, idx = 0)
    const int u = (4 - fx) * ub[idx] + fx * ub[idx + 1] - 8192;
    const int v = (4 - fx) * vb[idx] + fx * vb[idx + 1] - 8192;
    const int L = a.cy16 * (y - a.yoff) + (1 << 17);
    R = ov_clip3((L + a.rv * v) >> 18, 0, peak);
    G = ov_clip3((L - a.gu * u - a.gv * v) >> 18, 0, peak);
    B = ov_clip3((L + a.bu * u) >> 18, 0, peak);
}

// ---- table side ----

struct LutArgs {
    const uint2 *texels;                  // [S^3]: x = R | G << 16, y = B
    int S, S2, n;                         // points per axis, S^2, S - 1
};

inline LutArgs lut_args_fill(const ovhip_rgb_lut *lut)
{
    return LutArgs{ (const uint2 *)lut->d_texels, lut->size, lut->size * lut->size, lut->size - 1 };
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

// a pixel's tetrahedron: the weights of its second to fourth vertex (the first: 1023 - w1 - w2 - w3) and the texel indices of its first
// three (the fourth, the opposite corner: v0 + S^2 + S + 1)
struct LutPoint { int w1, w2, w3, v0, v1, v2; };

// R, G, B in 0..1023, which is what keeps every index inside the table: a cell index is at most n - 1, so the opposite corner is at
// most S^3 - 1
__device__ __forceinline__ LutPoint lut_point(int R, int G, int B, LutArgs l)
{
    int ir, ig, ib, fr, fg, fb;
    lut_cell(R, l.n, ir, fr); lut_cell(G, l.n, ig, fg); lut_cell(B, l.n, ib, fb);
    // the order of (fraction descending, channel ascending): a total order, so the first and the last channel differ
    const bool rg = fr >= fg, rb = fr >= fb, gb = fg >= fb;
    const int s_first = (rg && rb) ? 1 : ((!rg && gb) ? l.S : l.S2);
    const int s_last = (!rg && !rb) ? 1 : ((rg && !gb) ? l.S : l.S2);
    const int f1 = max(fr, max(fg, fb)), f3 = min(fr, min(fg, fb)), f2 = fr + fg + fb - f1 - f3;
    LutPoint p;
    p.w1 = f1 - f2; p.w2 = f2 - f3; p.w3 = f3;
    p.v0 = (ib * l.S + ig) * l.S + ir;
    p.v1 = p.v0 + s_first;
    p.v2 = p.v0 + (l.S2 + l.S + 1) - s_last;
    return p;
}

// the four vertices' texels under their weights: (sum + 511) / 1023 per channel  (a sum is at most 1023 * 65535 + 511 < 2^26)
__device__ __forceinline__ void lut_mix(int w1, int w2, int w3, uint2 t0, uint2 t1, uint2 t2, uint2 t3, uint32_t &oR, uint32_t &oG, uint32_t &oB)
{
    const uint32_t c0 = (uint32_t)(1023 - w1 - w2 - w3), c1 = (uint32_t)w1, c2 = (uint32_t)w2, c3 = (uint32_t)w3;
    oR = (c0 * (t0.x & 0xFFFFu) + c1 * (t1.x & 0xFFFFu) + c2 * (t2.x & 0xFFFFu) + c3 * (t3.x & 0xFFFFu) + 511u) / 1023u;
    oG = (c0 * (t0.x >> 16) + c1 * (t1.x >> 16) + c2 * (t2.x >> 16) + c3 * (t3.x >> 16) + 511u) / 1023u;
    oB = (c0 * (t0.y & 0xFFFFu) + c1 * (t1.y & 0xFFFFu) + c2 * (t2.y & 0xFFFFu) + c3 * (t3.y & 0xFFFFu) + 511u) / 1023u;
}

} // namespace
