// kernels_reduce.hip -- reduced-size output on gfx950: a decoded picture leaves the device smaller than it was coded, by the exact
// area average of include/ovvc_hip.h, "Reduced-size output on the device" (the host half and the C twin: ovvc_reduce.c; what both share:
// ovvc_reduce_priv.h).  Nothing in the reference does this: its down-sampling branch is dead code that reads past its tables.
//
// One launch for the luma tiles and both chroma planes' tiles, as k_output_scale.  A workgroup is ONE wave: it owns 64 destination
// columns by a band of RD_BAND destination rows and walks down the source rows under the band once, a GROUP of rows at a time: as many
// rows as fill the wave's 128 chunk slots (7 rows at 2:1, 1 row at 8:1), so that a wave has all its lanes' loads in flight at every
// ratio.  A group's row segments (at most 64 * 8 + 2 samples each) are staged into LDS, double-buffered -- the next group's loads fly
// while this group is summed --, with 16-byte loads on the chunks that the row's ADDRESS puts on 16-byte boundaries and that lie inside
// the region, element loads on the chunks at the region's edge; nothing outside the region is read.  A lane keeps the first sample and
// the (at most 9) weights of ITS column in registers -- closed form, no table, no upload --, sums each row horizontally from LDS and
// adds that into the two running vertical sums a source row can meet (a footprint is at least a sample long).  A footprint that ends is
// divided (reciprocal estimate and one correction: exact) into an LDS tile of the band, which leaves through run_store: 16 bytes where
// the address allows, narrower otherwise.  wave64, no MFMA.
#include "ovvc_common.hip.h"
#include "ovvc_dpb_priv.h"
#include "ovvc_reduce_priv.h"
#include "run_io.hip.h"

namespace {

#define RD_TW    64                 /* destination columns of a wave */
#define RD_BAND  8                  /* destination rows of a wave */
#define RD_NT    64
#define RD_TAPS  OVHIP_REDUCE_MAX_TAPS
#define RD_CHUNK 8                  /* samples of a 16-byte chunk */
#define RD_NCH   2                  /* chunk slots of a lane per group: 128 of a wave */
#define RD_SLOTS (RD_NCH * RD_NT)
#define RD_ROWS  8                  /* rows of a group at most */
#define RD_SLACK (2 * RD_CHUNK)     /* behind a staged row: the reach of a lane whose trailing weights are zero */
// chunks of a row at most: the segment (<= 64 * 8 + 2 samples) begun up to 7 samples early (the address's phase), in whole chunks
#define RD_MAXCPR ((RD_TW * OVHIP_REDUCE_MAX_RATIO + 2 + 7 + 7) / RD_CHUNK)
// samples of a staged group: rows * cpr <= max(RD_SLOTS, RD_MAXCPR) chunks, and every row's slack
#define RD_LDS   (RD_SLOTS * RD_CHUNK + RD_ROWS * RD_SLACK)

struct ReducePlane {
    const uint16_t *src; uint16_t *dst;        // src: the region's first sample
    int sstride, dstride;
    int sw, sh, dw, dh;                        // region and destination, in this plane's samples
    int sgx, sgy;
    int ntx;                                   // tiles per tile row
};
// cpr: chunks a staged row takes at most; rows: rows of a group, rows * cpr <= RD_SLOTS
struct ReduceArgs { ReducePlane p[3]; int first[3]; int px, qx, py, qy, ntap, cpr, rows; uint32_t n; float rcp; };

// the first staged sample of a row whose segment begins at sample xs: back to the 16-byte boundary at or below its address
__device__ __forceinline__ int stage_base(const uint16_t *row, int xs)
{
    return xs - (int)(((uintptr_t)(row + xs) >> 1) & (RD_CHUNK - 1));
}

// chunk `ch` of row `row` (valid: the row exists and the slot is used), whose segment is samples xs .. xe; samples outside 0 .. sw-1
// are not read (they carry no weight: 0 stands in)
__device__ __forceinline__ uint4 stage_load(const uint16_t *row, bool valid, int ch, int xs, int xe, int sw)
{
    uint4 v = make_uint4(0, 0, 0, 0);
    if (!valid) return v;
    const int x = stage_base(row, xs) + RD_CHUNK * ch;
    if (x > xe) return v;
    if (x >= 0 && x + RD_CHUNK <= sw) return *reinterpret_cast<const uint4 *>(row + x);
    uint32_t e[RD_CHUNK];
#pragma unroll
    for (int i = 0; i < RD_CHUNK; ++i) e[i] = (x + i >= 0 && x + i < sw) ? (uint32_t)row[x + i] : 0u;
    return make_uint4(e[0] | (e[1] << 16), e[2] | (e[3] << 16), e[4] | (e[5] << 16), e[6] | (e[7] << 16));
}

__global__ __launch_bounds__(RD_NT) void k_output_reduce(ReduceArgs a)
{
    __shared__ __attribute__((aligned(16))) uint16_t s_row[2][RD_LDS];
    __shared__ __attribute__((aligned(16))) uint16_t s_out[RD_BAND][RD_TW];
    const int b = (int)blockIdx.x, lane = (int)threadIdx.x;
    const int pl = ov_tile_plane(a, b);
    const ReducePlane p = pl == 0 ? a.p[0] : (pl == 1 ? a.p[1] : a.p[2]);
    const int t = ov_tile_index(a, b, pl);
    const int ty = t / p.ntx, tx = t - ty * p.ntx;
    const int px = a.px, qx = a.qx, py = a.py, qy = a.qy;
    const int rows = a.rows, cpr = a.cpr, rstride = cpr * RD_CHUNK + RD_SLACK;

    // this lane's column: its first sample and its weights (a lane past the plane's width works on the last column and stores nothing)
    const int k0 = tx * RD_TW, k1 = min(k0 + RD_TW, p.dw) - 1;
    const int kx = min(k0 + lane, k1);
    const int jb = ovhip_reduce_first_(kx, px, qx, p.sgx, p.sw);
    int w[RD_TAPS];
#pragma unroll
    for (int i = 0; i < RD_TAPS; ++i) w[i] = jb + i < p.sw ? ovhip_reduce_weight_(kx, jb + i, px, qx, p.sgx, p.sw) : 0;
    const int xs = ovhip_reduce_first_(k0, px, qx, p.sgx, p.sw), xe = ovhip_reduce_last_(k1, px, qx, p.sgx, p.sw);

    const int ka = ty * RD_BAND, kb = min(ka + RD_BAND, p.dh);
    const int ys = ovhip_reduce_first_(ka, py, qy, p.sgy, p.sh), ye = ovhip_reduce_last_(kb - 1, py, qy, p.sgy, p.sh);

    // this lane's chunk slots: row of the group and chunk of that row, the same for every group
    int sr[RD_NCH], sc[RD_NCH];
#pragma unroll
    for (int c = 0; c < RD_NCH; ++c) { const int s = lane + RD_NT * c; sr[c] = s / cpr; sc[c] = s - sr[c] * cpr; }

    uint4 v[RD_NCH];
#pragma unroll
    for (int c = 0; c < RD_NCH; ++c)
        v[c] = stage_load(p.src + (size_t)(ys + sr[c]) * (size_t)p.sstride, sr[c] < rows && ys + sr[c] <= ye, sc[c], xs, xe, p.sw);

    int cur = ka, last_cur = ovhip_reduce_last_(cur, py, qy, p.sgy, p.sh);
    int acc0 = 0, acc1 = 0, buf = 0;
    const int half = (int)(a.n >> 1);
    for (int jy = ys; jy <= ye; jy += rows) {
        uint16_t *s = s_row[buf];
#pragma unroll
        for (int c = 0; c < RD_NCH; ++c)
            if (sr[c] < rows) *reinterpret_cast<uint4 *>(s + sr[c] * rstride + RD_CHUNK * sc[c]) = v[c];
        __syncthreads();
#pragma unroll
        for (int c = 0; c < RD_NCH; ++c) {                      // the next group's loads fly while this group is summed
            const int y = jy + rows + sr[c];
            v[c] = stage_load(p.src + (size_t)y * (size_t)p.sstride, sr[c] < rows && y <= ye, sc[c], xs, xe, p.sw);
        }
        const int rend = min(rows, ye + 1 - jy);
        for (int r = 0; r < rend; ++r) {
            const int y = jy + r;
            const uint16_t *mine = s + r * rstride + (jb - stage_base(p.src + (size_t)y * (size_t)p.sstride, xs));
            int h = 0;
#pragma unroll
            for (int i = 0; i < RD_TAPS; ++i)
                if (i < a.ntap) h += __mul24(w[i], (int)mine[i]);   // (a weight of 0 may meet a sample that was not staged: it counts nothing)
            acc0 += __mul24(ovhip_reduce_weight_(cur, y, py, qy, p.sgy, p.sh), h);
            if (cur + 1 < kb) acc1 += __mul24(ovhip_reduce_weight_(cur + 1, y, py, qy, p.sgy, p.sh), h);
            while (cur < kb && y == last_cur) {
                s_out[cur - ka][lane] = (uint16_t)ovhip_reduce_div_((uint32_t)(acc0 + half), a.n, a.rcp);
                acc0 = acc1; acc1 = 0;
                ++cur;
                last_cur = cur < kb ? ovhip_reduce_last_(cur, py, qy, p.sgy, p.sh) : -1;
            }
        }
        buf ^= 1;
    }
    __syncthreads();
    {   // the band leaves: a lane owns 8 neighbouring samples of one destination row
        const int r = lane >> 3, c = (lane & 7) * 8;
        const int nvalid = min(8, k1 + 1 - (k0 + c));
        if (ka + r < kb && nvalid > 0) {
            const uint4 o = *reinterpret_cast<const uint4 *>(&s_out[r][c]);
            const uint32_t ow[4] = { o.x, o.y, o.z, o.w };
            run_store<2, 8>(reinterpret_cast<char *>(p.dst + (size_t)(ka + r) * (size_t)p.dstride + k0 + c), ow, nvalid);
        }
    }
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
    a.ntap = (pl.px + pl.qx - 1) / pl.qx + 1;
    if (a.ntap > RD_TAPS) a.ntap = RD_TAPS;
    a.n = pl.n; a.rcp = 1.0f / (float)pl.n;
    // a row's segment is at most ceil(64 p / q) + 2 samples, begun up to 7 samples early and ended in a whole chunk
    a.cpr = ((RD_TW * pl.px + pl.qx - 1) / pl.qx + 2 + 7 + 7) / RD_CHUNK;
    a.rows = RD_SLOTS / a.cpr < 1 ? 1 : (RD_SLOTS / a.cpr > RD_ROWS ? RD_ROWS : RD_SLOTS / a.cpr);
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
