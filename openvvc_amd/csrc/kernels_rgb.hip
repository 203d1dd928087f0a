// RGB output on the device (include/ovvc_hip.h, "RGB output on the device"): a finished 4:2:0 picture as an RGB tensor in device
// memory -- chroma up-sampled bilinearly at the signalled sample location, the matrix in 14-bit integer coefficients, the consumer's
// dtype and layout.  The refusals and the coefficients are the host twin's (ovvc_rgb.c: ovhip_rgb_plan_make_).
//
// k_rgb is a streaming kernel: 3 bytes in, 3 to 12 out per pixel.  A lane owns 8 horizontally adjacent output pixels of a row pair
// (picture rows 2k, 2k + 1: a window starts on an even row, so a pair is wholly inside it).  The 16 luma samples come as two 16-byte
// loads; both rows read chroma rows out of k - 1, k, k + 1 and columns out of the 6 around the run, so each plane's 3 x 6 taps are
// loaded once (an 8-byte load for the 4 inner columns, the two outer ones clamped) and blended vertically once per row.  The
// results are packed into registers in the destination's element type and stored as runs: a row's 8 pixels are 8 / 16 / 32 bytes per
// plane (PLANAR) or 24 / 48 / 96 bytes (PACKED); a run goes out 16 bytes at a time where its address is a multiple of 16, else 8 or 4
// at a time, else element by element -- the path of a row's tail (W & 7 pixels), and of a destination that is only element-aligned,
// such as a slice of a batch tensor at odd sizes.  Which path a run takes depends on its address alone, never on the data.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <stdint.h>
#include "ovvc_hip.h"
#include "ovvc_common.hip.h"
#include "ovvc_dpb_priv.h"
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
    int cy16, rv, gu, gv, bu, yoff, peak; // cy16 = 16 cy
    unsigned n_items;                     // groups * H / 2
};

template <int DT> struct ElemBytes { static constexpr int v = DT == OVHIP_RGB_U8 ? 1 : (DT == OVHIP_RGB_F32 ? 4 : 2); };

// the stored bits of one channel value
template <int DT> __device__ __forceinline__ uint32_t rgb_bits(int v)
{
    if constexpr (DT == OVHIP_RGB_U8 || DT == OVHIP_RGB_U16) return (uint32_t)v;
    else {
        const float f = __fmul_rn((float)v, (float)(1.0 / 1023));          // one multiplication, round to nearest, nothing to contract with
        if constexpr (DT == OVHIP_RGB_F32) return __float_as_uint(f);
        else return (uint32_t)__half_as_ushort(__float2half_rn(f));
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

template <int DT, int PACKED, int A>
__global__ __launch_bounds__(RGB_NT) void k_rgb(RgbArgs a)
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
        // horizontal blend, matrix, pack
        constexpr int NWP = RGB_RUN * ES / 4, NWK = PACKED ? 3 * NWP : 1;          // dwords of a plane's run / of the packed run
        uint32_t wr[NWP] = {}, wg[NWP] = {}, wb[NWP] = {}, wk[NWK] = {};
#pragma unroll
        for (int i = 0; i < RGB_RUN; ++i) {
            const int q = 2 * i - A + 4, idx = q >> 2, fx = q & 3;          // column idx of the 6 <-> cbase - 1 + idx
            const int u = (4 - fx) * ub[idx] + fx * ub[idx + 1] - 8192;
            const int v = (4 - fx) * vb[idx] + fx * vb[idx + 1] - 8192;
            const int L = a.cy16 * (Y[i] - a.yoff) + (1 << 17);
            const uint32_t R = rgb_bits<DT>(ov_clip3((L + a.rv * v) >> 18, 0, a.peak));
            const uint32_t G = rgb_bits<DT>(ov_clip3((L - a.gu * u - a.gv * v) >> 18, 0, a.peak));
            const uint32_t B = rgb_bits<DT>(ov_clip3((L + a.bu * u) >> 18, 0, a.peak));
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

template <int DT, int PACKED> void rgb_launch_a(const RgbArgs &a, int A, hipStream_t st)
{
    const unsigned wgs = (a.n_items + RGB_NT - 1) / RGB_NT;
    if (A) hipLaunchKernelGGL((k_rgb<DT, PACKED, 1>), dim3(wgs), dim3(RGB_NT), 0, st, a);
    else   hipLaunchKernelGGL((k_rgb<DT, PACKED, 0>), dim3(wgs), dim3(RGB_NT), 0, st, a);
}
template <int DT> void rgb_launch_l(const RgbArgs &a, int packed, int A, hipStream_t st)
{
    if (packed) rgb_launch_a<DT, 1>(a, A, st); else rgb_launch_a<DT, 0>(a, A, st);
}

} // namespace

extern "C" int ovhip_rgb_launch(ovhip_ctx *ctx, const ovhip_pic *pic, const ovhip_window *win, const ovhip_rgb_format *fmt, void *d_dst, size_t dst_bytes)
{
    if (!ctx || !pic || !fmt) return OVHIP_EINVAL;
    OV_DEVICE(ctx);
    ovhip_rgb_plan_ p;
    const char *why = "";
    const int r = ovhip_rgb_plan_make_(pic, win, fmt, d_dst, dst_bytes, &p, &why);
    if (r != OVHIP_OK) {
        snprintf(ctx->err, sizeof(ctx->err), "ovhip_rgb_launch: %s: %s", why, r == OVHIP_EUNSUP ? "unsupported" : "invalid argument");
        return r;
    }
    RgbArgs a;
    a.y = pic->y; a.cb = pic->cb; a.cr = pic->cr; a.dst = (char *)d_dst;
    a.stride_y = pic->stride_y; a.stride_c = pic->stride_c; a.cw = pic->w / 2; a.ch = pic->h / 2;
    a.x0 = p.x0; a.y0 = p.y0; a.W = p.W; a.H = p.H; a.groups = (p.W + RGB_RUN - 1) / RGB_RUN;
    a.b = p.b;
    a.cy16 = 16 * p.coef[0]; a.rv = p.coef[1]; a.gu = p.coef[2]; a.gv = p.coef[3]; a.bu = p.coef[4]; a.yoff = p.yoff; a.peak = p.peak;
    const size_t items = (size_t)a.groups * (size_t)(p.H / 2);
    if (items > 0x7FFFFFFFu) return ov_fail(ctx, OVHIP_EINVAL, "ovhip_rgb_launch: picture too large", hipSuccess);
    a.n_items = (unsigned)items;
    switch (fmt->dtype) {
    case OVHIP_RGB_U8:  rgb_launch_l<OVHIP_RGB_U8>(a, fmt->layout, p.a, ctx->stream); break;
    case OVHIP_RGB_U16: rgb_launch_l<OVHIP_RGB_U16>(a, fmt->layout, p.a, ctx->stream); break;
    case OVHIP_RGB_F16: rgb_launch_l<OVHIP_RGB_F16>(a, fmt->layout, p.a, ctx->stream); break;
    default:            rgb_launch_l<OVHIP_RGB_F32>(a, fmt->layout, p.a, ctx->stream); break;
    }
    OV_LAUNCH_CHECK(ctx, "k_rgb");
    return OVHIP_OK;
}

extern "C" int ovhip_pic_output_rgb(ovhip_ctx *ctx, const ovhip_pic *pic, const ovhip_window *win, const ovhip_rgb_format *fmt, void *host_dst, size_t dst_bytes)
{
    if (!ctx || !pic || !fmt || !host_dst) return OVHIP_EINVAL;
    OV_DEVICE(ctx);
    const size_t bytes = ovhip_rgb_bytes(pic->w, pic->h, win, fmt);
    if (!bytes || dst_bytes < bytes) {
        /* no size, or a host_dst that is too small: the launch refuses both before it looks at the pointer, and words the reason */
        const int q = ovhip_rgb_launch(ctx, pic, win, fmt, host_dst, dst_bytes);
        return q != OVHIP_OK ? q : OVHIP_EINVAL;
    }
    int r = ov_scratch(ctx, bytes, 0);
    if (r == OVHIP_OK) r = ovhip_rgb_launch(ctx, pic, win, fmt, ctx->scratch_d, bytes);
    if (r == OVHIP_OK) r = ovhip_d2h(ctx, host_dst, ctx->scratch_d, bytes);
    return r;
}
