// Surface output on the device (include/ovvc_hip.h, "Surface output on the device"): a finished 4:2:0 picture as an NV12 / P010 / I420 /
// I010 surface in device memory, at the caller's address and pitch.  The layout and the refusals are the host twin's (ovvc_surface.c:
// ovhip_surface_plan_make_).
//
// k_surface is a streaming kernel: 2 bytes in, 1 or 2 out per sample.  One launch covers all planes: the grid's items are the runs of
// 16 output elements of every row of every plane, luma rows first.  A lane owns one run.  Its 16 samples come as two 16-byte loads
// (luma, planar chroma) or as one 16-byte load from Cb and one from Cr (interleaved chroma: 8 pairs); they stay packed two to a dword
// while the threshold is added, shifted and clipped (8-bit formats) or shifted left (P010), are interleaved and narrowed to bytes in
// registers, and leave as one 16-byte store (8-bit elements) or two (16-bit elements).  A run is loaded and stored 16 bytes at a time
// where its address is a multiple of 16, else 8 or 4 at a time, else element by element -- the path of a row's tail (W & 15 elements),
// of a window's left edge, of an odd stride or pitch and of a destination that is only element-aligned.  Which path a run takes
// depends on its address alone, never on the data.  No LDS, no atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ovvc_hip.h"
#include "ovvc_common.hip.h"
#include "ovvc_dpb_priv.h"
#include "run_io.hip.h"
#include "surface_values.hip.h"

namespace {

#define SURF_NT  256
#define SURF_RUN 16           /* output elements of a row per lane */

struct SurfArgs {
    const uint16_t *src[3];   // y, cb, cr at the window's first sample
    char *dst[3];             // the planes of the surface (semi-planar: [1] is the interleaved plane, [2] unused)
    int stride[3];            // samples                                     ([1] == [2] in the four below: the chroma planes are alike)
    size_t pitch[3];          // bytes
    int elems[3];             // elements of an output row, per plane
    int groups[3];            // runs per row, per plane
    unsigned items_y, items_c;// runs of the luma plane / of ONE chroma plane
    unsigned n_items;
};

// (the value functions -- surf_thr, surf_pair, narrow4, surf_interleave -- are surface_values.hip.h's: k_output_ladder stores with them too)
template <int FMT, int DITHER>
__global__ __launch_bounds__(SURF_NT) void k_surface(SurfArgs a)
{
    constexpr bool SEMI = FMT == OVHIP_SURF_NV12 || FMT == OVHIP_SURF_P010;
    constexpr int ES = (FMT == OVHIP_SURF_P010 || FMT == OVHIP_SURF_I010) ? 2 : 1;
    unsigned item = blockIdx.x * SURF_NT + threadIdx.x;
    if (item >= a.n_items) return;
    int pl = 0;
    if (item >= a.items_y) {
        item -= a.items_y; pl = 1;
        if (!SEMI && item >= a.items_c) { item -= a.items_c; pl = 2; }
    }
    // (selects, not an index that differs from lane to lane: the arguments stay in scalar registers)
    const int c = pl > 0, groups = c ? a.groups[1] : a.groups[0], elems = c ? a.elems[1] : a.elems[0], stride = c ? a.stride[1] : a.stride[0];
    const size_t pitch = c ? a.pitch[1] : a.pitch[0];
    const uint16_t *src = pl == 0 ? a.src[0] : (pl == 1 ? a.src[1] : a.src[2]);
    char *dst = pl == 0 ? a.dst[0] : (pl == 1 ? a.dst[1] : a.dst[2]);
    const int row = (int)(item / (unsigned)groups), g = (int)(item - (unsigned)row * (unsigned)groups);
    const int e0 = g * SURF_RUN, n = min(SURF_RUN, elems - e0);
    const uint32_t thr = surf_thr(DITHER, row);

    uint32_t v[SURF_RUN / 2];                                                  // the run's values as 16-bit elements, in output order
    if (SEMI && pl == 1) {
        // 8 pairs: columns e0 / 2 .. e0 / 2 + 7 of Cb and of Cr; the pair's column decides the threshold, so it is applied before the interleave
        uint32_t b[SURF_RUN / 4], r[SURF_RUN / 4];
        const size_t so = (size_t)row * (size_t)stride + (size_t)(e0 >> 1);
        run_load<SURF_RUN / 2>(a.src[1] + so, b, n >> 1);
        run_load<SURF_RUN / 2>(a.src[2] + so, r, n >> 1);
#pragma unroll
        for (int k = 0; k < SURF_RUN / 4; ++k) {
            const uint32_t pb = surf_pair<FMT>(b[k], thr), pr = surf_pair<FMT>(r[k], thr);
            surf_interleave(pb, pr, &v[2 * k], &v[2 * k + 1]);
        }
    } else {
        run_load<SURF_RUN>(src + (size_t)row * (size_t)stride + (size_t)e0, v, n);
#pragma unroll
        for (int k = 0; k < SURF_RUN / 2; ++k) v[k] = surf_pair<FMT>(v[k], thr);
    }
    char *out = dst + (size_t)row * pitch + (size_t)e0 * ES;
    if constexpr (ES == 2) run_store<2, SURF_RUN>(out, v, n);
    else {
        uint32_t o[SURF_RUN / 4];
#pragma unroll
        for (int k = 0; k < SURF_RUN / 4; ++k) o[k] = narrow4(v[2 * k], v[2 * k + 1]);
        run_store<1, SURF_RUN>(out, o, n);
    }
}

template <int FMT, int DITHER> void surf_launch(const SurfArgs &a, hipStream_t st)
{
    hipLaunchKernelGGL((k_surface<FMT, DITHER>), dim3((a.n_items + SURF_NT - 1) / SURF_NT), dim3(SURF_NT), 0, st, a);
}

} // namespace

extern "C" int ovhip_surface_launch(ovhip_ctx *ctx, const ovhip_pic *pic, const ovhip_window *win, const ovhip_surface_format *fmt, void *d_dst, size_t dst_bytes)
{
    if (!ctx) return OVHIP_EINVAL;
    OV_DEVICE(ctx);
    ovhip_surface_plan_ p;
    const char *why = "";
    const int r = ovhip_surface_plan_make_(pic, win, fmt, d_dst, dst_bytes, &p, &why);
    if (r != OVHIP_OK) {
        if (pic && fmt && dst_bytes < p.bytes) snprintf(ctx->err, sizeof(ctx->err), "ovhip_surface_launch: %s: %zu bytes given, the surface needs %zu: invalid argument", why, dst_bytes, p.bytes);
        else snprintf(ctx->err, sizeof(ctx->err), "ovhip_surface_launch: %s: invalid argument", why);
        return r;
    }
    SurfArgs a;
    const uint16_t *planes[3] = { pic->y, pic->cb, pic->cr };
    uint64_t items[3] = { 0, 0, 0 };
    for (int k = 0; k < 3; ++k) {
        const int c = k > 0, q = k < p.n_planes ? k : 1;                       // (q: the surface's plane that sample plane k goes to)
        a.stride[k] = c ? pic->stride_c : pic->stride_y;
        a.src[k] = planes[k] + (size_t)(p.y0 >> c) * (size_t)a.stride[k] + (size_t)(p.x0 >> c);
        a.dst[k] = (char *)d_dst + p.off[q];
        a.pitch[k] = p.pitch[q];
        a.elems[k] = p.elems[q];
        a.groups[k] = (p.elems[q] + SURF_RUN - 1) / SURF_RUN;
        items[k] = (uint64_t)a.groups[k] * (uint64_t)p.rows[q];
    }
    const uint64_t total = items[0] + (uint64_t)(p.n_planes - 1) * items[1];
    if (total > 0x7FFFFFFFu) return ov_fail(ctx, OVHIP_EINVAL, "ovhip_surface_launch: picture too large", hipSuccess);
    a.items_y = (unsigned)items[0]; a.items_c = (unsigned)items[1]; a.n_items = (unsigned)total;
    switch (fmt->format) {
    case OVHIP_SURF_NV12: if (p.dither) surf_launch<OVHIP_SURF_NV12, 1>(a, ctx->stream); else surf_launch<OVHIP_SURF_NV12, 0>(a, ctx->stream); break;
    case OVHIP_SURF_I420: if (p.dither) surf_launch<OVHIP_SURF_I420, 1>(a, ctx->stream); else surf_launch<OVHIP_SURF_I420, 0>(a, ctx->stream); break;
    case OVHIP_SURF_P010: surf_launch<OVHIP_SURF_P010, 0>(a, ctx->stream); break;
    default:              surf_launch<OVHIP_SURF_I010, 0>(a, ctx->stream); break;
    }
    OV_LAUNCH_CHECK(ctx, "k_surface");
    return OVHIP_OK;
}

extern "C" int ovhip_pic_output_surface(ovhip_ctx *ctx, const ovhip_pic *pic, const ovhip_window *win, const ovhip_surface_format *fmt, void *host_dst, size_t dst_bytes)
{
    if (!ctx || !pic || !fmt || !host_dst) return OVHIP_EINVAL;
    OV_DEVICE(ctx);
    const size_t bytes = ovhip_surface_bytes(pic->w, pic->h, win, fmt);
    if (!bytes || dst_bytes < bytes) {
        /* no size, or a host_dst that is too small: the launch refuses both before it looks at the pointer, and words the reason */
        const int q = ovhip_surface_launch(ctx, pic, win, fmt, host_dst, dst_bytes);
        return q != OVHIP_OK ? q : OVHIP_EINVAL;
    }
    int r = ov_scratch(ctx, bytes, 0);
    if (r != OVHIP_OK) return r;
    char *d = (char *)ctx->scratch_d;
    r = ovhip_surface_launch(ctx, pic, win, fmt, d, bytes);
    if (r != OVHIP_OK) return r;
    ovhip_surface_plan_ p;
    (void)ovhip_surface_plan_make_(pic, win, fmt, d, bytes, &p, nullptr);      // (accepted a line above)
    bool tight = true;
    for (int k = 0; k < p.n_planes; ++k)
        tight = tight && p.pitch[k] == (size_t)p.elems[k] * p.es && p.off[k] == (k ? p.off[k - 1] + p.pitch[k - 1] * p.rows[k - 1] : 0);
    hipError_t e = hipSuccess;
    if (tight) e = hipMemcpyAsync(host_dst, d, bytes, hipMemcpyDeviceToHost, ctx->stream);
    else {
        /* the rows' own bytes only: what lies between them in host memory stays as it was */
        for (int k = 0; k < p.n_planes && e == hipSuccess; ++k)
            e = hipMemcpy2DAsync((char *)host_dst + p.off[k], p.pitch[k], d + p.off[k], p.pitch[k], (size_t)p.elems[k] * p.es, (size_t)p.rows[k],
                                 hipMemcpyDeviceToHost, ctx->stream);
    }
    if (e != hipSuccess) return ov_fail(ctx, OVHIP_ENODEV, "ovhip_pic_output_surface: D2H", e);
    if (ov_sync_stream(ctx) != hipSuccess) return ov_fail(ctx, OVHIP_ELAUNCH, "ovhip_pic_output_surface", hipGetLastError());
    return OVHIP_OK;
}
