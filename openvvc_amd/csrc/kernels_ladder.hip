// kernels_ladder.hip -- output ladder on gfx950: one finished picture leaves as several reduced surfaces, each at its own size, format
// and address (include/ovvc_hip.h, "Output ladder on the device"; the host half and the C twin: ovvc_ladder.c; what both share:
// ovvc_ladder_priv.h).  Rung r is surface(reduce(picture)) of the two written definitions, byte for byte.
//
// k_output_ladder is ONE launch for all rungs and all planes.  A workgroup is one wave, as k_output_reduce's; it finds its rung from a
// prefix table in the arguments (the rungs' tiles lie behind one another in the grid), its plane and tile from the rung's own
// firsts, and walks the source rows under its band with reduce_walk.hip.h -- the walk k_output_reduce instantiates too.  The band's
// tile never leaves as a 16-bit picture: the epilogue takes it from LDS through the surface's value functions
// (surface_values.hip.h: what k_surface stores with) keyed by the OUTPUT plane's coordinates, and stores the surface's elements with
// run_store: 16 bytes where the address allows, narrower at row tails, odd pitches and offsets.  The chroma workgroup of a semi-planar
// rung walks the Cb and then the Cr of its tile and stores the interleaved row: 8 pairs to a lane, never a store strided by one
// element.  Per-rung arguments travel as kernel arguments (about 1 KB for 8 rungs): nothing is uploaded, nothing allocated, and no
// intermediate picture exists anywhere.  wave64, no MFMA.
#include "ovvc_common.hip.h"
#include "ovvc_dpb_priv.h"
#include "ovvc_ladder_priv.h"
#include "ovvc_outdst_priv.h"
#include "reduce_walk.hip.h"
#include "run_io.hip.h"
#include "stage_out.hip.h"
#include "surface_values.hip.h"

namespace {

struct LadderRung {
    char *dst[3];                              // the surface's planes (semi-planar: [1] is the interleaved plane, [2] unused)
    size_t pitch[2];                           // bytes: luma, chroma
    int px, qx, py, qy, ntap, cpr, rows; uint32_t n; float rcp;
    int sgx, sgy;                              // sigma of the chroma planes (luma: 0)
    int dw, dh;                                // the rung's size in luma samples
    int fmt, dither;
    int ntx[2];                                // tiles per tile row: luma, chroma
    int first[3];                              // the rung's first workgroup of luma, of chroma (semi-planar: Cb and Cr), of Cr (planar)
};
struct LadderArgs {
    const uint16_t *src[3];                    // y, cb, cr at the region's first sample
    int sstride[2];
    int sw, sh;                                // the region in luma samples
    int n_rungs;
    int end[OVHIP_LADDER_MAX_RUNGS];           // the first workgroup behind rung r: the prefix table
    LadderRung r[OVHIP_LADDER_MAX_RUNGS];
};
static_assert(sizeof(LadderArgs) <= 2048, "the kernel arguments stay well inside 4 KB");

// a planar plane's band leaves: a lane owns 8 neighbouring elements of one row
template <int FMT> struct LadderStorePlanar {
    char *dst; size_t pitch; bool dither;
    const uint16_t (*s_out)[RD_TW];
    __device__ __forceinline__ void operator()(int k0, int k1, int ka, int kb) const
    {
        constexpr int ES = (FMT == OVHIP_SURF_P010 || FMT == OVHIP_SURF_I010) ? 2 : 1;
        const int lane = (int)threadIdx.x;
        const int r = lane >> 3, c = (lane & 7) * 8;
        const int nvalid = min(8, k1 + 1 - (k0 + c));
        if (ka + r >= kb || nvalid <= 0) return;
        const uint4 o = *reinterpret_cast<const uint4 *>(&s_out[r][c]);
        const uint32_t thr = surf_thr(dither, ka + r);                         // (k0 + c is even: a dword's low half is an even column)
        const uint32_t v[4] = { surf_pair<FMT>(o.x, thr), surf_pair<FMT>(o.y, thr), surf_pair<FMT>(o.z, thr), surf_pair<FMT>(o.w, thr) };
        char *out = dst + (size_t)(ka + r) * pitch + (size_t)(k0 + c) * ES;
        if constexpr (ES == 2) run_store<2, 8>(out, v, nvalid);
        else {
            const uint32_t n8[2] = { narrow4(v[0], v[1]), narrow4(v[2], v[3]) };
            run_store<1, 8>(out, n8, nvalid);
        }
    }
};

// an interleaved chroma band leaves: a lane owns 8 neighbouring pairs (16 elements) of one row, Cb from s_cb and Cr from s_cr; the pair's
// column decides the threshold, so it is applied before the interleave
template <int FMT> struct LadderStoreSemi {
    char *dst; size_t pitch; bool dither;
    const uint16_t (*s_cb)[RD_TW], (*s_cr)[RD_TW];
    __device__ __forceinline__ void operator()(int k0, int k1, int ka, int kb) const
    {
        constexpr int ES = FMT == OVHIP_SURF_P010 ? 2 : 1;
        const int lane = (int)threadIdx.x;
        const int r = lane >> 3, c = (lane & 7) * 8;
        const int nvalid = min(8, k1 + 1 - (k0 + c));
        if (ka + r >= kb || nvalid <= 0) return;
        const uint4 ob = *reinterpret_cast<const uint4 *>(&s_cb[r][c]), orr = *reinterpret_cast<const uint4 *>(&s_cr[r][c]);
        const uint32_t b[4] = { ob.x, ob.y, ob.z, ob.w }, q[4] = { orr.x, orr.y, orr.z, orr.w };
        const uint32_t thr = surf_thr(dither, ka + r);
        uint32_t v[8];
#pragma unroll
        for (int k = 0; k < 4; ++k) surf_interleave(surf_pair<FMT>(b[k], thr), surf_pair<FMT>(q[k], thr), &v[2 * k], &v[2 * k + 1]);
        char *out = dst + (size_t)(ka + r) * pitch + (size_t)(k0 + c) * 2 * ES;
        if constexpr (ES == 2) run_store<2, 16>(out, v, 2 * nvalid);
        else {
            const uint32_t n8[4] = { narrow4(v[0], v[1]), narrow4(v[2], v[3]), narrow4(v[4], v[5]), narrow4(v[6], v[7]) };
            run_store<1, 16>(out, n8, 2 * nvalid);
        }
    }
};

// what becomes of a walked tile: nothing yet behind the Cb pass of an interleaved plane (its tile waits in LDS for the Cr's), else the
// store of the rung's format -- a choice of the rung's alone, the same for the whole workgroup
struct LadderStore {
    char *dst; size_t pitch; int fmt; bool dither, semi, last;
    const uint16_t (*s_out)[RD_TW], (*s_out2)[RD_TW];
    __device__ __forceinline__ void operator()(int k0, int k1, int ka, int kb) const
    {
        if (!last) return;
        if (semi) {
            if (fmt == OVHIP_SURF_NV12) LadderStoreSemi<OVHIP_SURF_NV12>{ dst, pitch, dither, s_out, s_out2 }(k0, k1, ka, kb);
            else LadderStoreSemi<OVHIP_SURF_P010>{ dst, pitch, dither, s_out, s_out2 }(k0, k1, ka, kb);
        } else if (fmt == OVHIP_SURF_I010) LadderStorePlanar<OVHIP_SURF_I010>{ dst, pitch, dither, s_out }(k0, k1, ka, kb);
        else if (fmt == OVHIP_SURF_P010) LadderStorePlanar<OVHIP_SURF_P010>{ dst, pitch, dither, s_out }(k0, k1, ka, kb);
        else LadderStorePlanar<OVHIP_SURF_NV12>{ dst, pitch, dither, s_out }(k0, k1, ka, kb);      // (NV12 and I420: one value function)
    }
};

__global__ __launch_bounds__(RD_NT) void k_output_ladder(LadderArgs a)
{
    __shared__ __attribute__((aligned(16))) uint16_t s_row[2][RD_LDS];
    __shared__ __attribute__((aligned(16))) uint16_t s_out[2][RD_BAND][RD_TW];      // [1]: the Cr tile of an interleaved plane
    const int b = (int)blockIdx.x;
    int rg = 0;
    while (rg + 1 < a.n_rungs && b >= a.end[rg]) ++rg;                         // (of the workgroup's index alone: scalar)
    const LadderRung &g = a.r[rg];
    const int pl = b >= g.first[2] ? 2 : (b >= g.first[1] ? 1 : 0), c = pl > 0;
    const int ti = b - (pl == 0 ? g.first[0] : (pl == 1 ? g.first[1] : g.first[2]));
    const int ntx = c ? g.ntx[1] : g.ntx[0];
    const int ty = ti / ntx, tx = ti - ty * ntx;
    const bool semi = pl == 1 && (g.fmt == OVHIP_SURF_NV12 || g.fmt == OVHIP_SURF_P010);
    RdTile t = { pl == 0 ? a.src[0] : (pl == 1 ? a.src[1] : a.src[2]), c ? a.sstride[1] : a.sstride[0], a.sw >> c, a.sh >> c, g.dw >> c, g.dh >> c,
                 c ? g.sgx : 0, c ? g.sgy : 0, g.px, g.qx, g.py, g.qy, g.ntap, g.cpr, g.rows, g.n, g.rcp, tx, ty };
    LadderStore st = { pl == 0 ? g.dst[0] : (pl == 1 ? g.dst[1] : g.dst[2]), c ? g.pitch[1] : g.pitch[0], g.fmt, g.dither != 0, semi, false, s_out[0], s_out[1] };
    // one walk per sample plane of the output plane: the Cb and then the Cr of an interleaved plane, else the plane itself
    for (int pass = semi ? 0 : 1; pass < 2; ++pass) {
        st.last = pass == 1;
        if (semi && pass == 1) t.src = a.src[2];
        rd_walk(t, s_row, s_out[semi ? pass : 0], st);
    }
}

} // namespace

extern "C" int ovhip_ladder_launch(ovhip_ctx *ctx, const ovhip_pic *src, const ovhip_reduce_info *info, const ovhip_ladder_rung *rungs, int32_t n)
{
    if (!ctx) return OVHIP_EINVAL;
    OV_DEVICE(ctx);
    if (!src) return ov_fail(ctx, OVHIP_EINVAL, "ovhip_ladder_launch: null picture", hipSuccess);
    ovhip_ladder_plan_ pl;
    char why[240];
    const int r = ovhip_ladder_plan_make_(src, 0, 0, info, rungs, n, &pl, why, sizeof(why));
    if (r != OVHIP_OK) { snprintf(ctx->err, sizeof(ctx->err), "ovhip_ladder_launch: %s", why); return r; }
    LadderArgs a;
    memset(&a, 0, sizeof(a));
    const ovhip_reduce_plan_ &p0 = pl.red[0];                                  // (the region is the same in every rung)
    rd_src_fill(a, src, p0);
    a.n_rungs = n;
    int64_t nb = 0;
    for (int k = 0; k < n; ++k) {
        const ovhip_reduce_plan_ &rp = pl.red[k];
        const ovhip_surface_plan_ &sp2 = pl.surf[k];
        LadderRung &g = a.r[k];
        for (int q = 0; q < 3; ++q) g.dst[q] = q < sp2.n_planes ? (char *)rungs[k].dst + sp2.off[q] : nullptr;
        g.pitch[0] = sp2.pitch[0]; g.pitch[1] = sp2.pitch[1];
        rd_level_fill(g, rp);
        g.fmt = rungs[k].fmt.format; g.dither = sp2.dither;
        for (int c = 0; c < 2; ++c) g.ntx[c] = ((rp.Wd >> c) + RD_TW - 1) / RD_TW;
        const int64_t ty = (rp.Hd + RD_BAND - 1) / RD_BAND, tc = ((rp.Hd >> 1) + RD_BAND - 1) / RD_BAND;
        const int64_t ny = (int64_t)g.ntx[0] * ty, nc = (int64_t)g.ntx[1] * tc;
        g.first[0] = (int)nb;
        g.first[1] = (int)(nb + ny);
        nb += ny + (sp2.semi ? nc : 2 * nc);
        g.first[2] = (int)(sp2.semi ? nb : nb - nc);                           // (semi-planar: no workgroup reaches it)
        a.end[k] = (int)nb;
    }
    if (nb > 0x7FFFFFFF) return ov_fail(ctx, OVHIP_EINVAL, "ovhip_ladder_launch: too many tiles", hipSuccess);      // (8 rungs of 16384 x 16384: 5 M)
    hipLaunchKernelGGL(k_output_ladder, dim3((unsigned)nb), dim3(RD_NT), 0, ctx->stream, a);
    OV_LAUNCH_CHECK(ctx, "k_output_ladder");
    return OVHIP_OK;
}

extern "C" int ovhip_pic_output_ladder(ovhip_ctx *ctx, const ovhip_pic *pic, const ovhip_reduce_info *info, const ovhip_ladder_rung *rungs, int32_t n)
{
    if (!ctx) return OVHIP_EINVAL;
    OV_DEVICE(ctx);
    if (!pic || !rungs || n < 1 || n > OVHIP_LADDER_MAX_RUNGS) {
        /* the launch words the reason */
        const int q = pic ? ovhip_ladder_launch(ctx, pic, info, rungs, n) : ov_fail(ctx, OVHIP_EINVAL, "ovhip_pic_output_ladder: null picture", hipSuccess);
        return q != OVHIP_OK ? q : OVHIP_EINVAL;
    }
    OvStaged<ovhip_ladder_rung> st(rungs, n, [](const ovhip_ladder_rung &g) { return ovhip_surface_bytes(g.out_w, g.out_h, nullptr, &g.fmt); });
    return ov_stage_out(ctx, "ovhip_pic_output_ladder", "rung", st,
        [&](const ovhip_ladder_rung *d) { return ovhip_ladder_launch(ctx, pic, info, d, n); },
        [&] {
            ovhip_ladder_plan_ pl;
            char why[240];
            const int q = ovhip_ladder_plan_make_(nullptr, pic->w, pic->h, info, rungs, n, &pl, why, sizeof(why));
            if (q != OVHIP_OK) snprintf(ctx->err, sizeof(ctx->err), "ovhip_pic_output_ladder: %s", why);
            return q;
        },
        [&](const ovhip_ladder_rung &d, void *host) { return ov_stage_rung_back(ctx, pic, d, host); });
}
