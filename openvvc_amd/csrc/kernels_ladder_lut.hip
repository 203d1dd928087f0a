// kernels_ladder_lut.hip -- output ladder through a colour table on gfx950: one finished picture leaves as several reduced surfaces
// whose samples are those of the CONVERTED reduced pictures (include/ovvc_hip.h, "Output ladder through a colour table"; the host half
// and the C twin: ovvc_ladder_lut.c; what both share: ovvc_ladder_lut_priv.h).  Rung r is surface_lut(reduce(picture)) of the two written
// definitions, byte for byte.
//
// k_ladder_lut is ONE launch for all rungs and all planes.  A workgroup of LL_NW waves finds its rung from a prefix table in the
// arguments, as k_output_ladder's does, and owns a tile of LL_TW x LL_TH luma samples of the rung's output with the chroma under it:
//   1. reduce: the tile's Y, Cb and Cr with their halo into LDS, by reduce_walk.hip.h's walk at the tile's own origin (rd_walk_at) --
//      up to 2 x 2 luma walks of 64 x RD_BAND and one walk per chroma plane, each by a wave of its own, all at the same time.  The
//      halo: one chroma column and row on each side for the source's bilinear taps, one luma column to the left where the destination's
//      chroma is horizontally co-sited (HC), one luma row above where it is vertically top (a.vt).  At the reduced picture's edges the
//      halo is the clamp of the definition: the chroma taps clamp to the reduced chroma plane, the filter's taps to the reduced luma
//      rectangle;
//   2. convert: a lane owns a pair of luma columns and a wave every LL_NW-th pair of the tile's rows: the chroma taps' vertical blend from
//      LDS, then colour_stage.hip.h's pixel (horizontal blend, matrix, clip), lut_point, the four pixels' 16 gathers issued together,
//      lut_mix, the normalising division and the forward matrix.  Y (10 bits) goes back to the luma tile in place, Cb14 and Cr14 into
//      two LDS planes.  Every pixel of the tile and its halo is converted once: 121 x 13 / (120 x 12) of the tile's own at most;
//   3. store: a lane owns 8 luma samples of a row, then 8 chroma samples (semi-planar: 8 pairs) of a chroma row, filtered 1 2 1 or 2 2
//      on each axis out of the Cb14 / Cr14 planes; values by surface_values.hip.h keyed by the rung's own output coordinates, stores by
//      run_io.hip.h: 16 bytes where the address allows, narrower at row tails, odd pitches and offsets.
// Per-rung arguments, the matrices and the table's LutArgs travel as kernel arguments (about 1.2 KB for 8 rungs): nothing is uploaded,
// nothing allocated, and no intermediate picture exists in device memory.  The source's horizontal location A and HC are template
// arguments, the rest launch arguments (uniform branches).  wave64, no MFMA.
//
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage; A x HC, 4 instantiations):
//   HC = 0: 70 VGPRs; HC = 1: 73 VGPRs (A = 0 and A = 1 alike); 106 SGPRs, no scratch, 40144 bytes of LDS per workgroup of 6 waves (their
//   staging rows 27648, the luma tile 4096, the chroma tiles 2048, Cb14 / Cr14 6344): 4 workgroups per CU by the LDS, 6 waves per SIMD.
//   One wave per workgroup (17104 bytes, 3 waves per SIMD, the six walks one after another) took 229 us where this takes 127: LABBOOK 37.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include "ovvc_hip.h"
#include "ovvc_common.hip.h"
#include "ovvc_dpb_priv.h"
#include "ovvc_ladder_lut_priv.h"
#include "ovvc_outdst_priv.h"
#include "reduce_walk.hip.h"
#include "run_io.hip.h"
#include "stage_out.hip.h"
#include "surface_values.hip.h"
#include "colour_stage.hip.h"

namespace {

#define LL_TW 120                   /* luma columns of a tile: with the halo column 121 <= 2 walks; its 60 chroma columns + 2 <= 1 walk */
#define LL_TH 12                    /* luma rows of a tile: with the halo row 13 <= 2 bands; its 6 chroma rows + 2 = 1 band */
#define LL_KW (LL_TW + 2)           /* columns of a Cb14 / Cr14 row in LDS (121 used) */
static_assert(LL_TW + 1 <= 2 * RD_TW && LL_TW / 2 + 2 <= RD_TW && LL_TH + 1 <= 2 * RD_BAND && LL_TH / 2 + 2 <= RD_BAND, "a tile and its halo fit the walks");
#define LL_NWALK 6                  /* walks of a tile: 2 bands x 2 column walks of luma, Cb, Cr */
#define LL_NW 6                     /* waves of a workgroup: each walks, then converts and stores its share of the tile */
#define LL_NT (LL_NW * RD_NT)
static_assert(LL_TW % 8 == 0 && LL_TW / 8 <= 16 && LL_TH / 2 <= 8, "the store's lanes cover a tile");

struct LlRung {
    char *dst[3];                              // the surface's planes (semi-planar: [1] is the interleaved plane, [2] unused)
    size_t pitch[2];                           // bytes: luma, chroma
    int px, qx, py, qy, ntap, cpr, rows; uint32_t n; float rcp;
    int sgx, sgy;                              // sigma of the chroma planes (luma: 0)
    int dw, dh;                                // the rung's size in luma samples
    int fmt, dither;
    int ntx;                                   // tiles per tile row
    int first;                                 // the rung's first workgroup
};
struct LlArgs {
    const uint16_t *src[3];                    // y, cb, cr at the region's first sample
    int sstride[2];
    int sw, sh;                                // the region in luma samples
    int n_rungs;
    int end[OVHIP_LADDER_MAX_RUNGS];           // the first workgroup behind rung r: the prefix table
    LlRung r[OVHIP_LADDER_MAX_RUNGS];
    ColSrc c;                                  // the source stage's b and matrix (its planes and sizes are not read: the tile is in LDS)
    int fwd[9], yoff16;                        // forward matrix: y_r y_g y_b, b_r b_g b_b, r_r r_g r_b; 16 yoff of the destination
    int vt;                                    // destination vertically top
    unsigned P; float rcpP;                    // the table's peak, 1.0f / P
    LutArgs l;
};
static_assert(sizeof(LlArgs) <= 2048, "the kernel arguments stay well inside 4 KB");

struct LlNone { __device__ __forceinline__ void operator()(int, int, int, int) const {} };      // the walked tile stays in LDS

// sample (x, y) of the tile's reduced luma: x, y relative to the halo'd tile's first column and row
__device__ __forceinline__ uint16_t &ll_y(uint16_t (*s_y)[RD_BAND][RD_TW], int x, int y)
{
    return s_y[(y >> 3) * 2 + (x >> 6)][y & (RD_BAND - 1)][x & (RD_TW - 1)];
}

// 8 luma samples of output row `row`, columns x .. x + 7 (x even) of which n exist, as the rung's elements
template <int FMT> __device__ __forceinline__ void ll_store_y(const LlRung &g, const uint32_t (&w)[4], int x, int row, int n)
{
    constexpr int ES = (FMT == OVHIP_SURF_P010 || FMT == OVHIP_SURF_I010) ? 2 : 1;
    const uint32_t thr = surf_thr(g.dither != 0, row);
    const uint32_t v[4] = { surf_pair<FMT>(w[0], thr), surf_pair<FMT>(w[1], thr), surf_pair<FMT>(w[2], thr), surf_pair<FMT>(w[3], thr) };
    char *out = g.dst[0] + (size_t)row * g.pitch[0] + (size_t)x * ES;
    if constexpr (ES == 2) run_store<2, 8>(out, v, n);
    else {
        const uint32_t n8[2] = { narrow4(v[0], v[1]), narrow4(v[2], v[3]) };
        run_store<1, 8>(out, n8, n);
    }
}

// 8 chroma samples of each plane of output chroma row `row`, columns m .. m + 7 (m even) of which n exist
template <int FMT> __device__ __forceinline__ void ll_store_c(const LlRung &g, const uint32_t (&b)[4], const uint32_t (&q)[4], int m, int row, int n)
{
    constexpr bool SEMI = FMT == OVHIP_SURF_NV12 || FMT == OVHIP_SURF_P010;
    constexpr int ES = (FMT == OVHIP_SURF_P010 || FMT == OVHIP_SURF_I010) ? 2 : 1;
    const uint32_t thr = surf_thr(g.dither != 0, row);
    uint32_t pb[4], pr[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) { pb[k] = surf_pair<FMT>(b[k], thr); pr[k] = surf_pair<FMT>(q[k], thr); }
    if constexpr (SEMI) {
        uint32_t v[8];
#pragma unroll
        for (int k = 0; k < 4; ++k) surf_interleave(pb[k], pr[k], &v[2 * k], &v[2 * k + 1]);
        char *out = g.dst[1] + (size_t)row * g.pitch[1] + (size_t)m * 2 * ES;
        if constexpr (ES == 2) run_store<2, 16>(out, v, 2 * n);
        else {
            const uint32_t n8[4] = { narrow4(v[0], v[1]), narrow4(v[2], v[3]), narrow4(v[4], v[5]), narrow4(v[6], v[7]) };
            run_store<1, 16>(out, n8, 2 * n);
        }
    } else {
        const size_t at = (size_t)row * g.pitch[1] + (size_t)m * ES;
        if constexpr (ES == 2) {
            run_store<2, 8>(g.dst[1] + at, pb, n);
            run_store<2, 8>(g.dst[2] + at, pr, n);
        } else {
            const uint32_t b8[2] = { narrow4(pb[0], pb[1]), narrow4(pb[2], pb[3]) }, r8[2] = { narrow4(pr[0], pr[1]), narrow4(pr[2], pr[3]) };
            run_store<1, 8>(g.dst[1] + at, b8, n);
            run_store<1, 8>(g.dst[2] + at, r8, n);
        }
    }
}

template <int A, int HC>
__global__ __launch_bounds__(LL_NT) void k_ladder_lut(LlArgs a)
{
    __shared__ __attribute__((aligned(16))) uint16_t s_row[LL_NW][2][RD_LDS];        // a wave's own staging rows
    __shared__ __attribute__((aligned(16))) uint16_t s_y[4][RD_BAND][RD_TW];        // the luma tile: [band * 2 + column walk]
    __shared__ __attribute__((aligned(16))) uint16_t s_c[2][RD_BAND][RD_TW];        // the Cb and the Cr tile
    __shared__ uint16_t s_k[2][LL_TH + 1][LL_KW];                                  // Cb14, Cr14 of the luma tile's positions
    const int tid = (int)threadIdx.x, lane = tid & (RD_NT - 1), wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b = (int)blockIdx.x;
    int rg = 0;
    while (rg + 1 < a.n_rungs && b >= a.end[rg]) ++rg;                             // (of the workgroup's index alone: scalar)
    const LlRung &g = a.r[rg];
    const int ti = b - g.first, ty = ti / g.ntx, tx = ti - ty * g.ntx;
    const int cw = g.dw >> 1, ch = g.dh >> 1;                                      // the reduced picture's chroma plane
    // the tile's own samples X0 .. X1 - 1, Y0 .. Y1 - 1 (all four even) and the first column and row of its halo'd luma
    const int X0 = tx * LL_TW, X1 = min(X0 + LL_TW, g.dw), Y0 = ty * LL_TH, Y1 = min(Y0 + LL_TH, g.dh);
    const int lx0 = max(X0 - HC, 0), ly0 = max(Y0 - a.vt, 0);
    // the chroma the source's taps reach: columns X0 / 2 - 1 .. X1 / 2, rows Y0 / 2 - 1 .. Y1 / 2, clamped to the plane
    const int kc0 = max((X0 >> 1) - 1, 0), kc1 = min(X1 >> 1, cw - 1), kr0 = max((Y0 >> 1) - 1, 0), kr1 = min(Y1 >> 1, ch - 1);

    // 1. reduce: the tile's walks dealt to the waves; a walk's lanes wait for one another only
    for (int wk = wave; wk < LL_NWALK; wk += LL_NW) {
        if (wk < 4) {
            const int ka = ly0 + RD_BAND * (wk >> 1), k0 = lx0 + RD_TW * (wk & 1);
            if (ka >= Y1 || k0 >= X1) continue;
            const RdTile t = { a.src[0], a.sstride[0], a.sw, a.sh, g.dw, g.dh, 0, 0, g.px, g.qx, g.py, g.qy, g.ntap, g.cpr, g.rows, g.n, g.rcp, 0, 0 };
            rd_walk_at(t, RdAt{ k0, min(k0 + RD_TW, X1) - 1, ka, min(ka + RD_BAND, Y1) }, s_row[wave], s_y[wk], LlNone{});
        } else {
            const RdTile t = { a.src[wk - 3], a.sstride[1], a.sw >> 1, a.sh >> 1, cw, ch, g.sgx, g.sgy, g.px, g.qx, g.py, g.qy, g.ntap, g.cpr, g.rows, g.n, g.rcp, 0, 0 };
            rd_walk_at(t, RdAt{ kc0, kc1, kr0, kr1 + 1 }, s_row[wave], s_c[wk - 4], LlNone{});
        }
    }
    __syncthreads();

    // 2. convert: this lane's columns xe, xe + 1 (the first pair of a tile with a halo column begins one column before it), this wave's rows
    {
        const int xe = (lx0 & ~1) + 2 * lane;
        if (xe < X1) {
            const int m = xe >> 1;
            int ci[3];                                                             // the taps' columns m - 1, m, m + 1 in s_c
#pragma unroll
            for (int t = 0; t < 3; ++t) ci[t] = min(max(m - 1 + t, 0), cw - 1) - kc0;
            const int xi[2] = { max(xe, lx0) - lx0, xe + 1 - lx0 };                // in the luma tile
            const int s_all = a.l.S2 + a.l.S + 1;                                  // from a cell's vertex to the opposite corner
            for (int y0 = ly0 + 2 * wave; y0 < Y1; y0 += 2 * LL_NW) {
                LutPoint p[4];
#pragma unroll
                for (int r = 0; r < 2; ++r) {
                    const int y = min(y0 + r, Y1 - 1);                             // (a last row without a partner: converted twice)
                    // vertical blend: V = 2y - b; rows j0, j0 + 1 of the reduced chroma plane, clamped
                    const int dv = 2 * y - a.c.b, fy = dv & 3, j0 = dv >> 2;
                    const int rlo = min(max(j0, 0), ch - 1) - kr0, rhi = min(max(j0 + 1, 0), ch - 1) - kr0;
                    int ub[6] = {}, vb[6] = {};
#pragma unroll
                    for (int t = 0; t < 3; ++t) {
                        ub[t] = (4 - fy) * (int)s_c[0][rlo][ci[t]] + fy * (int)s_c[0][rhi][ci[t]];
                        vb[t] = (4 - fy) * (int)s_c[1][rlo][ci[t]] + fy * (int)s_c[1][rhi][ci[t]];
                    }
#pragma unroll
                    for (int i = 0; i < 2; ++i) {
                        int R, G, B;
                        col_pixel<A>(a.c, ub, vb, i, (int)ll_y(s_y, xi[i], y - ly0), 1023, R, G, B);
                        p[2 * r + i] = lut_point(R, G, B, a.l);
                    }
                }
                // the four pixels' gathers, all in flight together
                uint2 t0v[4], t1v[4], t2v[4], t3v[4];
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    t0v[c] = a.l.texels[p[c].v0]; t1v[c] = a.l.texels[p[c].v1]; t2v[c] = a.l.texels[p[c].v2]; t3v[c] = a.l.texels[p[c].v0 + s_all];
                }
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    uint32_t oR, oG, oB;
                    lut_mix(p[c].w1, p[c].w2, p[c].w3, t0v[c], t1v[c], t2v[c], t3v[c], oR, oG, oB);
                    const int qr = ovhip_surface_lut_norm_(oR, a.P, a.rcpP), qg = ovhip_surface_lut_norm_(oG, a.P, a.rcpP), qb = ovhip_surface_lut_norm_(oB, a.P, a.rcpP);
                    const int y14 = a.yoff16 + ovhip_surface_lut_row_(a.fwd, qr, qg, qb);
                    const int ry = min(y0 + (c >> 1), Y1 - 1) - ly0, x = xe + (c & 1);
                    if (x >= lx0) {
                        s_k[0][ry][x - lx0] = (uint16_t)(8192 + ovhip_surface_lut_row_(a.fwd + 3, qr, qg, qb));      // (1 .. 16383: 8192 -+ 8184 and the rounding)
                        s_k[1][ry][x - lx0] = (uint16_t)(8192 + ovhip_surface_lut_row_(a.fwd + 6, qr, qg, qb));
                        ll_y(s_y, x - lx0, ry) = (uint16_t)ov_clip3((y14 + 8) >> 4, 0, 1023);
                    }
                }
            }
        }
    }
    __syncthreads();

    // 3a. the luma rows: 16 lanes to a row (15 runs of 8 at most)
    for (int y = Y0 + (tid >> 4); y < Y1; y += LL_NT / 16) {
        const int x = X0 + 8 * (tid & 15), n = min(8, X1 - x);
        if (n <= 0) continue;
        uint32_t w[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int xa = min(x + 2 * k, X1 - 2) - lx0;
            w[k] = (uint32_t)ll_y(s_y, xa, y - ly0) | ((uint32_t)ll_y(s_y, xa + 1, y - ly0) << 16);
        }
        switch (g.fmt) {
        case OVHIP_SURF_I010: ll_store_y<OVHIP_SURF_I010>(g, w, x, y, n); break;
        case OVHIP_SURF_P010: ll_store_y<OVHIP_SURF_P010>(g, w, x, y, n); break;
        default:              ll_store_y<OVHIP_SURF_NV12>(g, w, x, y, n); break;      // (NV12 and I420: one value function)
        }
    }

    // 3b. the chroma rows: 8 lanes to a row (8 runs of 8 at most), the tile's 6 rows at once
    static_assert(LL_NT / 8 >= LL_TH / 2, "a lane for every chroma run of the tile");
    {
        const int k = (Y0 >> 1) + (tid >> 3), m0 = (X0 >> 1) + 8 * (tid & 7), n = min(8, (X1 >> 1) - m0);
        if (k < (Y1 >> 1) && n > 0) {
            // rows 2k - 1 (vertically top only; clamped), 2k, 2k + 1 with 1 2 1 or 0 2 2; columns 2m - 1 (co-sited only; clamped), 2m, 2m + 1
            int accb[8] = {}, accr[8] = {};
            for (int ry = a.vt ? -1 : 0; ry < 2; ++ry) {
                const int row = max(2 * k + ry, 0) - ly0, wy = (a.vt && ry != 0) ? 1 : 2;
                int cb[17], cr[17];
#pragma unroll
                for (int i = 1 - HC; i < 17; ++i) {
                    const int x = min(max(2 * m0 - 1 + i, 0), X1 - 1) - lx0;
                    cb[i] = s_k[0][row][x]; cr[i] = s_k[1][row][x];
                }
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int hb = HC ? cb[2 * j] + 2 * cb[2 * j + 1] + cb[2 * j + 2] : 2 * (cb[2 * j + 1] + cb[2 * j + 2]);
                    const int hr = HC ? cr[2 * j] + 2 * cr[2 * j + 1] + cr[2 * j + 2] : 2 * (cr[2 * j + 1] + cr[2 * j + 2]);
                    accb[j] += wy * hb; accr[j] += wy * hr;
                }
            }
            uint32_t pb[4], pr[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                pb[j] = (uint32_t)ov_clip3((accb[2 * j] + 128) >> 8, 0, 1023) | ((uint32_t)ov_clip3((accb[2 * j + 1] + 128) >> 8, 0, 1023) << 16);
                pr[j] = (uint32_t)ov_clip3((accr[2 * j] + 128) >> 8, 0, 1023) | ((uint32_t)ov_clip3((accr[2 * j + 1] + 128) >> 8, 0, 1023) << 16);
            }
            switch (g.fmt) {
            case OVHIP_SURF_NV12: ll_store_c<OVHIP_SURF_NV12>(g, pb, pr, m0, k, n); break;
            case OVHIP_SURF_I420: ll_store_c<OVHIP_SURF_I420>(g, pb, pr, m0, k, n); break;
            case OVHIP_SURF_P010: ll_store_c<OVHIP_SURF_P010>(g, pb, pr, m0, k, n); break;
            default:              ll_store_c<OVHIP_SURF_I010>(g, pb, pr, m0, k, n); break;
            }
        }
    }
}

} // namespace

extern "C" int ovhip_ladder_lut_launch(ovhip_ctx *ctx, const ovhip_pic *src, const ovhip_reduce_info *info, const ovhip_ladder_rung *rungs, int32_t n,
                                       const ovhip_surface_conv *conv, const ovhip_rgb_lut *lut)
{
    if (!ctx) return OVHIP_EINVAL;
    OV_DEVICE(ctx);
    if (!src) return ov_fail(ctx, OVHIP_EINVAL, "ovhip_ladder_lut_launch: null picture", hipSuccess);
    ovhip_ladder_lut_plan_ pl;
    char why[240];
    int r = ovhip_ladder_lut_plan_make_(src, 0, 0, info, rungs, n, conv, lut ? lut->size : 0, lut ? lut->peak : 0, lut != NULL, &pl, why, sizeof(why));
    if (r == OVHIP_OK && lut->device != ctx->device) { snprintf(why, sizeof(why), "the table lives on another device"); r = OVHIP_EINVAL; }
    if (r != OVHIP_OK) { snprintf(ctx->err, sizeof(ctx->err), "ovhip_ladder_lut_launch: %s", why); return r; }
    LlArgs a;
    memset(&a, 0, sizeof(a));
    const ovhip_reduce_plan_ &p0 = pl.lad.red[0];                              // (the region is the same in every rung)
    rd_src_fill(a, src, p0);
    a.n_rungs = n;
    int64_t nb = 0;
    for (int k = 0; k < n; ++k) {
        const ovhip_reduce_plan_ &rp = pl.lad.red[k];
        const ovhip_surface_plan_ &sp2 = pl.sl[k].surf;
        LlRung &g = a.r[k];
        for (int q = 0; q < 3; ++q) g.dst[q] = q < sp2.n_planes ? (char *)rungs[k].dst + sp2.off[q] : nullptr;
        g.pitch[0] = sp2.pitch[0]; g.pitch[1] = sp2.pitch[1];
        rd_level_fill(g, rp);
        g.fmt = rungs[k].fmt.format; g.dither = sp2.dither;
        g.ntx = (rp.Wd + LL_TW - 1) / LL_TW;
        g.first = (int)nb;
        nb += (int64_t)g.ntx * ((rp.Hd + LL_TH - 1) / LL_TH);
        a.end[k] = (int)nb;
    }
    if (nb > 0x7FFFFFFF) return ov_fail(ctx, OVHIP_EINVAL, "ovhip_ladder_lut_launch: too many tiles", hipSuccess);      // (8 rungs of 16384 x 16384: 1.5 M)
    /* the conversion is the same in every rung: rung 0's plan gives the source stage's b and matrix and the forward side */
    const ovhip_surface_lut_plan_ &s0 = pl.sl[0];
    a.c.b = s0.rgb.b;
    a.c.cy16 = 16 * s0.rgb.coef[0]; a.c.rv = s0.rgb.coef[1]; a.c.gu = s0.rgb.coef[2]; a.c.gv = s0.rgb.coef[3]; a.c.bu = s0.rgb.coef[4]; a.c.yoff = s0.rgb.yoff;
    for (int k = 0; k < 9; ++k) a.fwd[k] = s0.coef[k];
    a.yoff16 = 16 * s0.yoff;
    a.vt = s0.vt;
    a.P = (unsigned)lut->peak; a.rcpP = 1.0f / (float)lut->peak;
    a.l = lut_args_fill(lut);
    const dim3 grid((unsigned)nb), block(LL_NT);
    if (s0.rgb.a) {
        if (s0.hc) hipLaunchKernelGGL((k_ladder_lut<1, 1>), grid, block, 0, ctx->stream, a);
        else       hipLaunchKernelGGL((k_ladder_lut<1, 0>), grid, block, 0, ctx->stream, a);
    } else {
        if (s0.hc) hipLaunchKernelGGL((k_ladder_lut<0, 1>), grid, block, 0, ctx->stream, a);
        else       hipLaunchKernelGGL((k_ladder_lut<0, 0>), grid, block, 0, ctx->stream, a);
    }
    OV_LAUNCH_CHECK(ctx, "k_ladder_lut");
    return OVHIP_OK;
}

extern "C" int ovhip_pic_output_ladder_lut(ovhip_ctx *ctx, const ovhip_pic *pic, const ovhip_reduce_info *info, const ovhip_ladder_rung *rungs, int32_t n,
                                           const ovhip_surface_conv *conv, const ovhip_rgb_lut *lut)
{
    if (!ctx) return OVHIP_EINVAL;
    OV_DEVICE(ctx);
    if (!pic || !rungs || n < 1 || n > OVHIP_LADDER_MAX_RUNGS) {
        /* the launch words the reason */
        const int q = pic ? ovhip_ladder_lut_launch(ctx, pic, info, rungs, n, conv, lut) : ov_fail(ctx, OVHIP_EINVAL, "ovhip_pic_output_ladder_lut: null picture", hipSuccess);
        return q != OVHIP_OK ? q : OVHIP_EINVAL;
    }
    OvStaged<ovhip_ladder_rung> st(rungs, n, [](const ovhip_ladder_rung &g) { return ovhip_surface_bytes(g.out_w, g.out_h, nullptr, &g.fmt); });
    return ov_stage_out(ctx, "ovhip_pic_output_ladder_lut", "rung", st,
        [&](const ovhip_ladder_rung *d) { return ovhip_ladder_lut_launch(ctx, pic, info, d, n, conv, lut); },
        [&] {
            ovhip_ladder_lut_plan_ pl;
            char why[240];
            int q = ovhip_ladder_lut_plan_make_(nullptr, pic->w, pic->h, info, rungs, n, conv, lut ? lut->size : 0, lut ? lut->peak : 0, lut != NULL, &pl, why, sizeof(why));
            if (q == OVHIP_OK && lut->device != ctx->device) { snprintf(why, sizeof(why), "the table lives on another device"); q = OVHIP_EINVAL; }
            if (q != OVHIP_OK) snprintf(ctx->err, sizeof(ctx->err), "ovhip_pic_output_ladder_lut: %s", why);
            return q;
        },
        [&](const ovhip_ladder_rung &d, void *host) { return ov_stage_rung_back(ctx, pic, d, host); });
}
