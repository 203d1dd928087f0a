// kernels_reduce.hip -- reduced-size output on gfx950: a decoded picture leaves the device smaller than it was coded, by the exact
// area average of include/ovvc_hip.h, "Reduced-size output on the device" (the host half and the C twin: ovvc_reduce.c; what both share:
// ovvc_reduce_priv.h).  Nothing in the reference does this: its down-sampling branch is dead code that reads past its tables.
//
// One launch for the luma tiles and both chroma planes' tiles, as k_output_scale.  A workgroup is ONE wave that owns 64 destination
// columns by a band of RD_BAND destination rows; how it walks the source rows under the band is reduce_walk.hip.h (shared with
// k_output_ladder).  The band's LDS tile leaves through run_store: 16 bytes where the address allows, narrower otherwise.  wave64, no
// MFMA.
#include "ovvc_common.hip.h"
#include "ovvc_dpb_priv.h"
#include "ovvc_reduce_priv.h"
#include "reduce_walk.hip.h"
#include "run_io.hip.h"

namespace {

struct ReducePlane {
    const uint16_t *src; uint16_t *dst;        // src: the region's first sample
    int sstride, dstride;
    int sw, sh, dw, dh;                        // region and destination, in this plane's samples
    int sgx, sgy;
    int ntx;                                   // tiles per tile row
};
// cpr: chunks a staged row takes at most; rows: rows of a group, rows * cpr <= RD_SLOTS
struct ReduceArgs { ReducePlane p[3]; int first[3]; int px, qx, py, qy, ntap, cpr, rows; uint32_t n; float rcp; };

// the band leaves as samples of the destination plane: a lane owns 8 neighbouring samples of one destination row
struct ReduceStore {
    uint16_t *dst; int dstride;
    const uint16_t (*s_out)[RD_TW];
    __device__ __forceinline__ void operator()(int k0, int k1, int ka, int kb) const
    {
        const int lane = (int)threadIdx.x;
        const int r = lane >> 3, c = (lane & 7) * 8;
        const int nvalid = min(8, k1 + 1 - (k0 + c));
        if (ka + r < kb && nvalid > 0) {
            const uint4 o = *reinterpret_cast<const uint4 *>(&s_out[r][c]);
            const uint32_t ow[4] = { o.x, o.y, o.z, o.w };
            run_store<2, 8>(reinterpret_cast<char *>(dst + (size_t)(ka + r) * (size_t)dstride + k0 + c), ow, nvalid);
        }
    }
};

__global__ __launch_bounds__(RD_NT) void k_output_reduce(ReduceArgs a)
{
    __shared__ __attribute__((aligned(16))) uint16_t s_row[2][RD_LDS];
    __shared__ __attribute__((aligned(16))) uint16_t s_out[RD_BAND][RD_TW];
    const int b = (int)blockIdx.x;
    const int pl = ov_tile_plane(a, b);
    const ReducePlane p = pl == 0 ? a.p[0] : (pl == 1 ? a.p[1] : a.p[2]);
    const int t = ov_tile_index(a, b, pl);
    const int ty = t / p.ntx, tx = t - ty * p.ntx;
    const RdTile tile = { p.src, p.sstride, p.sw, p.sh, p.dw, p.dh, p.sgx, p.sgy, a.px, a.qx, a.py, a.qy, a.ntap, a.cpr, a.rows, a.n, a.rcp, tx, ty };
    rd_walk(tile, s_row, s_out, ReduceStore{ p.dst, p.dstride, s_out });
}

} // namespace

// library-internal (ovvc_reduce_priv.h)
extern "C" int ovhip_reduce_refusal_(ovhip_ctx *ctx, const char *who, const ovhip_pic *src, const ovhip_reduce_info *info, int32_t dst_w, int32_t dst_h)
{
    ovhip_reduce_plan_ pl;
    char why[200];
    const int r = ovhip_reduce_plan_make_(src->w, src->h, info, dst_w, dst_h, &pl, why, sizeof(why));
    if (r != OVHIP_OK) snprintf(ctx->err, sizeof(ctx->err), "%s: %s", who, why);
    return r;
}

extern "C" int ovhip_output_reduce_launch(ovhip_ctx *ctx, const ovhip_pic *src, const ovhip_reduce_info *info, const ovhip_pic *dst)
{
    if (!ctx || !src || !info || !dst) return OVHIP_EINVAL;
    OV_DEVICE(ctx);
    const char *what = ovhip_reduce_why_pics_(src, dst);
    if (what) { snprintf(ctx->err, sizeof(ctx->err), "ovhip_output_reduce_launch: %s: invalid argument", what); return OVHIP_EINVAL; }
    ovhip_reduce_plan_ pl;
    char why[200];
    const int r = ovhip_reduce_plan_make_(src->w, src->h, info, dst->w, dst->h, &pl, why, sizeof(why));
    if (r != OVHIP_OK) { snprintf(ctx->err, sizeof(ctx->err), "ovhip_output_reduce_launch: %s", why); return r; }
    const uint16_t *sp[3] = { src->y, src->cb, src->cr };
    uint16_t *dp[3] = { dst->y, dst->cb, dst->cr };
    ReduceArgs a;
    a.px = pl.px; a.qx = pl.qx; a.py = pl.py; a.qy = pl.qy;
    a.n = pl.n; a.rcp = 1.0f / (float)pl.n;
    rd_shape(pl, &a.ntap, &a.cpr, &a.rows);
    int n = 0;
    for (int i = 0; i < 3; ++i) {
        ReducePlane &p = a.p[i];
        const int c = i != 0;
        p.sstride = c ? src->stride_c : src->stride_y; p.dstride = c ? dst->stride_c : dst->stride_y;
        p.src = sp[i] + (size_t)(pl.y0 >> c) * (size_t)p.sstride + (size_t)(pl.x0 >> c);
        p.dst = dp[i];
        p.sw = pl.Ws >> c; p.sh = pl.Hs >> c; p.dw = pl.Wd >> c; p.dh = pl.Hd >> c;
        p.sgx = c ? pl.sgx : 0; p.sgy = c ? pl.sgy : 0;
        p.ntx = (p.dw + RD_TW - 1) / RD_TW;
        a.first[i] = n;
        n += p.ntx * ((p.dh + RD_BAND - 1) / RD_BAND);
    }
    hipLaunchKernelGGL(k_output_reduce, dim3((unsigned)n), dim3(RD_NT), 0, ctx->stream, a);
    OV_LAUNCH_CHECK(ctx, "k_output_reduce");
    return OVHIP_OK;
}
