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
//
// The source's arguments and their fill, the chroma row load and the pixel (horizontal blend, matrix, clip) are colour_stage.hip.h's,
// shared with k_rgb_lut and k_surface_lut.  The luma row load and the vertical blend are written out here: as functions of the header
// (luma_row; the blend over the rows' arrays or one column at a time) they cost 8 and 3 of the 16 instantiations a wave (5 to 10 more
// VGPRs, such as 73 -> 83, 77 -> 84: LABBOOK 36).  RgbArgs' field order is part of that: with the source in front of dst and peak the same
// 3 lose a wave.
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage): 70-86 VGPRs, 44-52 SGPRs, 5-7 waves per SIMD, no
// scratch, no LDS.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <stdint.h>
#include "ovvc_hip.h"
#include "ovvc_common.hip.h"
#include "ovvc_dpb_priv.h"
#include "run_io.hip.h"
#include "colour_stage.hip.h"

namespace {

struct RgbArgs {                          // (in this order: see above)
    char *dst;
    int peak;                             // the clip is to 0..peak
    ColSrc s;
};

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

template <int DT, int PACKED, int A>
__global__ __launch_bounds__(COL_NT) void k_rgb(RgbArgs ra)
{
    const ColSrc &a = ra.s;
    constexpr int ES = RgbElemBytes<DT>::v;
    const unsigned item = blockIdx.x * COL_NT + threadIdx.x;
    if (item >= a.n_items) return;
    const int rp = (int)(item / (unsigned)a.groups), g = (int)(item - (unsigned)rp * (unsigned)a.groups);
    const int ox = g * COL_RUN, n = min(COL_RUN, a.W - ox);
    const bool full = n == COL_RUN;
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
        // luma (the text of colour_stage.hip.h's luma_row, kept here for the registers) and the vertical blend:
        // V = 2 (2k + r) - b = 4k + (2r - b), so j0 = k + ((2r - b) >> 2) and fy = (2r - b) & 3
        int Y[COL_RUN], ub[6], vb[6];
        const uint16_t *yrow = a.y + (size_t)(py + r) * (size_t)a.stride_y + px;
        if (full && ((uintptr_t)yrow & 15) == 0) {
            const uint4 v = *reinterpret_cast<const uint4 *>(yrow);
            Y[0] = (int)(v.x & 0xFFFFu); Y[1] = (int)(v.x >> 16); Y[2] = (int)(v.y & 0xFFFFu); Y[3] = (int)(v.y >> 16);
            Y[4] = (int)(v.z & 0xFFFFu); Y[5] = (int)(v.z >> 16); Y[6] = (int)(v.w & 0xFFFFu); Y[7] = (int)(v.w >> 16);
        } else {
#pragma unroll
            for (int i = 0; i < COL_RUN; ++i) Y[i] = yrow[min(i, n - 1)];
        }
        const int d = 2 * r - a.b, fy = d & 3, t0 = 1 + (d >> 2);          // t0: 0 or 1, the same in every lane
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            const int ulo = t0 ? cbv[1][i] : cbv[0][i], uhi = t0 ? cbv[2][i] : cbv[1][i];
            const int vlo = t0 ? crv[1][i] : crv[0][i], vhi = t0 ? crv[2][i] : crv[1][i];
            ub[i] = (4 - fy) * ulo + fy * uhi;
            vb[i] = (4 - fy) * vlo + fy * vhi;
        }
        // the pixels, packed as they come
        constexpr int NWP = COL_RUN * ES / 4, NWK = PACKED ? 3 * NWP : 1;          // dwords of a plane's run / of the packed run
        uint32_t wr[NWP] = {}, wg[NWP] = {}, wb[NWP] = {}, wk[NWK] = {};
#pragma unroll
        for (int i = 0; i < COL_RUN; ++i) {
            int Ri, Gi, Bi;
            col_pixel<A>(a, ub, vb, i, Y[i], ra.peak, Ri, Gi, Bi);
            const uint32_t R = rgb_bits<DT>(Ri), G = rgb_bits<DT>(Gi), B = rgb_bits<DT>(Bi);
            if constexpr (PACKED) {
                run_put<ES, NWK>(wk, 3 * i, R); run_put<ES, NWK>(wk, 3 * i + 1, G); run_put<ES, NWK>(wk, 3 * i + 2, B);
            } else {
                run_put<ES, NWP>(wr, i, R); run_put<ES, NWP>(wg, i, G); run_put<ES, NWP>(wb, i, B);
            }
        }
        const size_t at = (size_t)(2 * rp + r) * (size_t)a.W + (size_t)ox;
        if constexpr (PACKED) {
            run_store<ES, 3 * COL_RUN>(ra.dst + at * 3 * ES, wk, 3 * n);
        } else {
            run_store<ES, COL_RUN>(ra.dst + at * ES, wr, n);
            run_store<ES, COL_RUN>(ra.dst + (plane + at) * ES, wg, n);
            run_store<ES, COL_RUN>(ra.dst + (2 * plane + at) * ES, wb, n);
        }
    }
}

template <int DT, int PACKED> void rgb_launch_a(const RgbArgs &a, int A, hipStream_t st)
{
    const unsigned wgs = (a.s.n_items + COL_NT - 1) / COL_NT;
    if (A) hipLaunchKernelGGL((k_rgb<DT, PACKED, 1>), dim3(wgs), dim3(COL_NT), 0, st, a);
    else   hipLaunchKernelGGL((k_rgb<DT, PACKED, 0>), dim3(wgs), dim3(COL_NT), 0, st, a);
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
    if (!col_src_fill(a.s, pic, p)) return ov_fail(ctx, OVHIP_EINVAL, "ovhip_rgb_launch: picture too large", hipSuccess);
    a.dst = (char *)d_dst; a.peak = p.peak;
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
    return rgb_output_host(ctx, pic, win, fmt, host_dst, dst_bytes, [&](void *d, size_t n) { return ovhip_rgb_launch(ctx, pic, win, fmt, d, n); });
}
