// RGB output through a colour table, on the device (include/ovvc_hip.h, "RGB output through a colour table"): k_rgb's conversion
// with one table-driven step between its clip and its store -- a 3D colour lookup table of 17, 33 or 65 points per axis,
// interpolated tetrahedrally in integers.  The refusals and the coefficients are the host twin's (ovvc_rgb_lut.c:
// ovhip_rgb_lut_plan_make_, on top of ovvc_rgb.c's plan).
//
// k_rgb_lut is k_rgb's item (kernels_rgb.hip): a lane owns 8 horizontally adjacent output pixels of a row pair, loads each chroma
// plane's 3 x 6 taps once, blends, applies the matrix (at 10 bits whatever the dtype) and the clip.  Unlike
// k_rgb this is no pure stream: a pixel makes four 8-byte gathers, at addresses its own value decides, from the texel array (R, G, B,
// 0 per lattice point; 39 KB, 287 KB or 2.2 MB: resident in the XCD's L2 beside the streamed picture), with plain loads.  A row's 32
// addresses are computed first and its 32 loads issued together; the order of the three fractions is three compares, the vertex steps
// are selects of the strides 1, S and S^2 by those compares: no data-dependent branch.  Stores as k_rgb's, by the run's address alone
// (run_io.hip.h).  A table of 17 points staged in LDS was tried and is not here: slower on the pictures a decoder makes (LABBOOK 30).
//
// The stages are colour_stage.hip.h's, one row or one pixel at a time: the source side (arguments, chroma and luma row loads, the
// pixel), shared with k_rgb, and the table side (lut_point, lut_mix), shared with k_surface_lut.  What is here is the item's loops, their
// order -- addresses, gathers, mix --, the stores, and the vertical blend: as a function of the header (over the rows' arrays, or one
// column at a time) it made every cell of a smooth 4K picture 1.7 to 2.1 us slower (40.1 -> 42.0), at equal registers (LABBOOK 36).
// lut_point takes the table's arguments BY VALUE: by reference, four packed instantiations took 9 to 11 more VGPRs and lost a wave.
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage): packed 118-128 VGPRs, 72-96 SGPRs, 4 waves per
// SIMD; planar 158-168 VGPRs, 60 SGPRs, 3 waves; no scratch, no LDS.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <stdint.h>
#include <stdlib.h>
#include "ovvc_hip.h"
#include "ovvc_common.hip.h"
#include "ovvc_dpb_priv.h"
#include "ovvc_rgb_lut_priv.h"
#include "run_io.hip.h"
#include "colour_stage.hip.h"

namespace {

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

// dst: the tensor; to_unit: (float)(1.0 / P)
template <int DT, int PACKED, int A>
__global__ __launch_bounds__(COL_NT) void k_rgb_lut(ColSrc a, LutArgs l, char *dst, float to_unit)
{
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
    const int s_all = l.S2 + l.S + 1;                              // from a cell's vertex to the opposite corner
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        int Y[COL_RUN], ub[6], vb[6];
        luma_row(a.y + (size_t)(py + r) * (size_t)a.stride_y + px, full, n, Y);
        // vertical blend: V = 2 (2k + r) - b = 4k + (2r - b), so j0 = k + ((2r - b) >> 2) and fy = (2r - b) & 3
        const int d = 2 * r - a.b, fy = d & 3, t0 = 1 + (d >> 2);          // t0: 0 or 1, the same in every lane
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            const int ulo = t0 ? cbv[1][i] : cbv[0][i], uhi = t0 ? cbv[2][i] : cbv[1][i];
            const int vlo = t0 ? crv[1][i] : crv[0][i], vhi = t0 ? crv[2][i] : crv[1][i];
            ub[i] = (4 - fy) * ulo + fy * uhi;
            vb[i] = (4 - fy) * vlo + fy * vhi;
        }
        // the row's cells, weights and its 32 texel addresses
        LutPoint p[COL_RUN];
#pragma unroll
        for (int i = 0; i < COL_RUN; ++i) {
            int R, G, B;
            col_pixel<A>(a, ub, vb, i, Y[i], 1023, R, G, B);
            p[i] = lut_point(R, G, B, l);
        }
        // the row's gathers, all in flight together
        uint2 t0v[COL_RUN], t1v[COL_RUN], t2v[COL_RUN], t3v[COL_RUN];
#pragma unroll
        for (int i = 0; i < COL_RUN; ++i) {
            t0v[i] = l.texels[p[i].v0]; t1v[i] = l.texels[p[i].v1]; t2v[i] = l.texels[p[i].v2]; t3v[i] = l.texels[p[i].v0 + s_all];
        }
        // interpolation, pack
        constexpr int NWP = COL_RUN * ES / 4, NWK = PACKED ? 3 * NWP : 1;          // dwords of a plane's run / of the packed run
        uint32_t wr[NWP] = {}, wg[NWP] = {}, wb[NWP] = {}, wk[NWK] = {};
#pragma unroll
        for (int i = 0; i < COL_RUN; ++i) {
            uint32_t oR, oG, oB;
            lut_mix(p[i].w1, p[i].w2, p[i].w3, t0v[i], t1v[i], t2v[i], t3v[i], oR, oG, oB);
            const uint32_t R = lut_bits<DT>(oR, to_unit), G = lut_bits<DT>(oG, to_unit), B = lut_bits<DT>(oB, to_unit);
            if constexpr (PACKED) {
                run_put<ES, NWK>(wk, 3 * i, R); run_put<ES, NWK>(wk, 3 * i + 1, G); run_put<ES, NWK>(wk, 3 * i + 2, B);
            } else {
                run_put<ES, NWP>(wr, i, R); run_put<ES, NWP>(wg, i, G); run_put<ES, NWP>(wb, i, B);
            }
        }
        const size_t at = (size_t)(2 * rp + r) * (size_t)a.W + (size_t)ox;
        if constexpr (PACKED) {
            run_store<ES, 3 * COL_RUN>(dst + at * 3 * ES, wk, 3 * n);
        } else {
            run_store<ES, COL_RUN>(dst + at * ES, wr, n);
            run_store<ES, COL_RUN>(dst + (plane + at) * ES, wg, n);
            run_store<ES, COL_RUN>(dst + (2 * plane + at) * ES, wb, n);
        }
    }
}

struct LutLaunch { ColSrc a; LutArgs l; char *dst; float to_unit; };

template <int DT, int PACKED> void lut_launch_a(const LutLaunch &q, int A, hipStream_t st)
{
    const unsigned wgs = (q.a.n_items + COL_NT - 1) / COL_NT;
    if (A) hipLaunchKernelGGL((k_rgb_lut<DT, PACKED, 1>), dim3(wgs), dim3(COL_NT), 0, st, q.a, q.l, q.dst, q.to_unit);
    else   hipLaunchKernelGGL((k_rgb_lut<DT, PACKED, 0>), dim3(wgs), dim3(COL_NT), 0, st, q.a, q.l, q.dst, q.to_unit);
}
template <int DT> void lut_launch_l(const LutLaunch &q, int packed, int A, hipStream_t st)
{
    if (packed) lut_launch_a<DT, 1>(q, A, st); else lut_launch_a<DT, 0>(q, A, st);
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
    LutLaunch q;
    if (!col_src_fill(q.a, pic, p)) return ov_fail(ctx, OVHIP_EINVAL, "ovhip_rgb_lut_launch: picture too large", hipSuccess);
    q.l = lut_args_fill(lut); q.dst = (char *)d_dst; q.to_unit = (float)(1.0 / lut->peak);
    switch (fmt->dtype) {
    case OVHIP_RGB_U8:  lut_launch_l<OVHIP_RGB_U8>(q, fmt->layout, p.a, ctx->stream); break;
    case OVHIP_RGB_U16: lut_launch_l<OVHIP_RGB_U16>(q, fmt->layout, p.a, ctx->stream); break;
    case OVHIP_RGB_F16: lut_launch_l<OVHIP_RGB_F16>(q, fmt->layout, p.a, ctx->stream); break;
    default:            lut_launch_l<OVHIP_RGB_F32>(q, fmt->layout, p.a, ctx->stream); break;
    }
    OV_LAUNCH_CHECK(ctx, "k_rgb_lut");
    return OVHIP_OK;
}

extern "C" int ovhip_pic_output_rgb_lut(ovhip_ctx *ctx, const ovhip_pic *pic, const ovhip_window *win, const ovhip_rgb_format *fmt, const ovhip_rgb_lut *lut,
                                        void *host_dst, size_t dst_bytes)
{
    if (!ctx || !pic || !fmt || !host_dst) return OVHIP_EINVAL;
    OV_DEVICE(ctx);
    return rgb_output_host(ctx, pic, win, fmt, host_dst, dst_bytes, [&](void *d, size_t n) { return ovhip_rgb_lut_launch(ctx, pic, win, fmt, lut, d, n); });
}
