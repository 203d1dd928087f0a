// kernels_rgb_pyramid.hip -- RGB pyramid on gfx950: one finished picture leaves as several reduced RGB tensors (include/ovvc_hip.h, "RGB
// pyramid on the device"; the host half and the C twin: ovvc_rgb_pyramid.c; what both share: ovvc_rgb_pyramid_priv.h).  Level r is
// rgb(reduce(picture)) -- through a table: rgb_lut(reduce(picture)) -- of the written definitions, byte for byte.
//
// k_rgb_pyramid is ONE launch for all levels.  A workgroup of PY_NW waves finds its level from a prefix table in the arguments, as
// k_ladder_lut's does, and owns a tile of PY_TW x PY_TH pixels of the level's output:
//   1. reduce: the tile's Y, Cb and Cr into LDS, by reduce_walk.hip.h's walk at the tile's own origin (rd_walk_at) -- up to 2 x 2 luma
//      walks of 64 x RD_BAND and one walk per chroma plane with one chroma column and row of halo on each side for the bilinear taps,
//      each by a wave of its own, all at the same time.  At the reduced picture's edges the halo is the clamp of the definition: the
//      chroma taps clamp to the REDUCED chroma plane;
//   2. convert: a lane owns a pair of columns and a wave every PY_NW-th pair of the tile's rows: the chroma taps' vertical blend from
//      LDS written out (colour_stage.hip.h says why), then colour_stage.hip.h's pixel (horizontal blend, matrix, clip) with the LEVEL's
//      coefficient set -- the arguments carry two, 8 and 10 bits, since a U8 and a U16 level may share a launch --, and with a table
//      lut_point, the four pixels' 16 gathers issued together, lut_mix.  R goes back to the luma tile in place, G and B into two LDS
//      planes, as integers of at most 16 bits;
//   3. store: a lane owns 8 pixels of a row, reads them back from LDS, makes the level's elements (U8, U16, F16, F32) and stores them
//      as runs by run_io.hip.h: a plane's 8 / 16 / 32 bytes or the 24 / 48 / 96 bytes of 8 packed pixels, 16 bytes at a time where
//      the address allows, narrower at row tails (4 pixels) and at bases that are only element-aligned.
// The converted values pass BACK THROUGH LDS between 2 and 3, on purpose.  The lane of step 2 holds two columns of a row: stored from
// there, a U8 planar level would leave two bytes at a time.  Giving a lane 8 pixels of a row in step 2 instead leaves 180 items of a
// tile to 384 lanes, so more than half of the workgroup would idle through the gathers, the expensive part; the pair-of-columns lane
// keeps 360 of 384 busy, and the pass through LDS costs 6 bytes per pixel of LDS traffic and one barrier.
// Per-level arguments, both coefficient sets and the table's LutArgs travel as kernel arguments (under 1 KB for 8 levels): nothing is
// uploaded, nothing allocated, and no intermediate picture exists in device memory.  The source's horizontal location A and
// table-or-not are template arguments; dtype and layout are branches that are uniform in a workgroup.  wave64, no MFMA.
//
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage; A x LUT, 4 instantiations):
//   without a table: 46 VGPRs (A = 0 and A = 1 alike); with a table: 73 VGPRs (A = 0), 75 (A = 1); 103 SGPRs, no AGPRs, no scratch, 39552
//   bytes of LDS per workgroup of 6 waves (their staging rows 27648, the luma tile 4096, the chroma tiles 2048, G and B 5760): 4
//   workgroups per CU by the LDS, 6 waves per SIMD.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <stdint.h>
#include <stdlib.h>
#include "ovvc_hip.h"
#include "ovvc_common.hip.h"
#include "ovvc_dpb_priv.h"
#include "ovvc_rgb_pyramid_priv.h"
#include "ovvc_outdst_priv.h"
#include "reduce_walk.hip.h"
#include "run_io.hip.h"
#include "stage_out.hip.h"
#include "colour_stage.hip.h"

namespace {

#define PY_TW 120                   /* columns of a tile: 2 luma walks; its 60 chroma columns + 2 of halo <= 1 walk */
#define PY_TH 12                    /* rows of a tile: 2 luma bands; its 6 chroma rows + 2 of halo = 1 band */
static_assert(PY_TW <= 2 * RD_TW && PY_TW / 2 + 2 <= RD_TW && PY_TH <= 2 * RD_BAND && PY_TH / 2 + 2 <= RD_BAND, "a tile and its halo fit the walks");
#define PY_NWALK 6                  /* walks of a tile: 2 bands x 2 column walks of luma, Cb, Cr */
#define PY_NW 6                     /* waves of a workgroup: each walks, then converts and stores its share of the tile */
#define PY_NT (PY_NW * RD_NT)
#define PY_RUNS (PY_TW / COL_RUN)   /* runs of 8 pixels in a tile's row */
static_assert(PY_TW % COL_RUN == 0 && PY_TW / 2 <= RD_NT && PY_TH % 2 == 0, "the convert's lanes cover a tile's row; a tile begins on a run and on a row pair");

struct PyLevel {
    char *dst;
    int px, qx, py, qy, ntap, cpr, rows; uint32_t n; float rcp;
    int sgx, sgy;                              // sigma of the chroma planes (luma: 0)
    int dw, dh;                                // the level's size
    int dtype, packed;
    int cs;                                    // its coefficient set: 0: 10 bits, 1: 8 bits (U8 without a table)
    int ntx;                                   // tiles per tile row
    int first;                                 // the level's first workgroup
};
struct PyArgs {
    const uint16_t *src[3];                    // y, cb, cr at the region's first sample
    int sstride[2];
    int sw, sh;                                // the region in luma samples
    int n_levels;
    int end[OVHIP_PYRAMID_MAX_LEVELS];         // the first workgroup behind level r: the prefix table
    PyLevel r[OVHIP_PYRAMID_MAX_LEVELS];
    ColSrc c[2];                               // the source stage's b and matrix per coefficient set (planes and sizes are not read: the tile is in LDS)
    int peak[2];                               // the clip of each set: 1023, 255
    float to_unit;                             // of a float element: 1 / 1023, with a table 1 / its peak
    LutArgs l;
};
static_assert(sizeof(PyArgs) <= 2048, "the kernel arguments stay well inside 4 KB");

struct PyNone { __device__ __forceinline__ void operator()(int, int, int, int) const {} };      // the walked tile stays in LDS

// sample (x, y) of the tile's reduced luma, then of its R: x, y relative to the tile's first column and row
__device__ __forceinline__ uint16_t &py_y(uint16_t (*s_y)[RD_BAND][RD_TW], int x, int y)
{
    return s_y[(y >> 3) * 2 + (x >> 6)][y & (RD_BAND - 1)][x & (RD_TW - 1)];
}

// the stored bits of one channel value v of 0 .. P: to_unit = (float)(1.0 / P), as k_rgb's and k_rgb_lut's
template <int DT> __device__ __forceinline__ uint32_t py_bits(uint32_t v, float to_unit)
{
    if constexpr (DT == OVHIP_RGB_U8 || DT == OVHIP_RGB_U16) return v;
    else {
        const float f = __fmul_rn((float)v, to_unit);                      // one multiplication, round to nearest, nothing to contract with
        if constexpr (DT == OVHIP_RGB_F32) return __float_as_uint(f);
        else return (uint32_t)__half_as_ushort(__float2half_rn(f));        // (round to nearest even, subnormal halves included)
    }
}

// 8 pixels of output row `row`, columns x .. x + 7 of which n exist, as the level's elements: (xi, yi) is the first one's place in the tile
template <int DT, int PACKED>
__device__ __forceinline__ void py_store(const PyLevel &g, uint16_t (*s_y)[RD_BAND][RD_TW], uint16_t (*s_k)[PY_TH][PY_TW], int xi, int yi, int x, int row,
                                         int n, float to_unit)
{
    constexpr int ES = RgbElemBytes<DT>::v;
    constexpr int NWP = COL_RUN * ES / 4, NWK = PACKED ? 3 * NWP : 1;      // dwords of a plane's run / of the packed run
    uint32_t wr[NWP] = {}, wg[NWP] = {}, wb[NWP] = {}, wk[NWK] = {};
#pragma unroll
    for (int i = 0; i < COL_RUN; ++i) {
        // (behind a tail of n the tile's columns hold what the walk left there: packed, never stored)
        const uint32_t R = py_bits<DT>(py_y(s_y, xi + i, yi), to_unit), G = py_bits<DT>(s_k[0][yi][xi + i], to_unit), B = py_bits<DT>(s_k[1][yi][xi + i], to_unit);
        if constexpr (PACKED) {
            run_put<ES, NWK>(wk, 3 * i, R); run_put<ES, NWK>(wk, 3 * i + 1, G); run_put<ES, NWK>(wk, 3 * i + 2, B);
        } else {
            run_put<ES, NWP>(wr, i, R); run_put<ES, NWP>(wg, i, G); run_put<ES, NWP>(wb, i, B);
        }
    }
    const size_t plane = (size_t)g.dw * (size_t)g.dh, at = (size_t)row * (size_t)g.dw + (size_t)x;
    if constexpr (PACKED) {
        run_store<ES, 3 * COL_RUN>(g.dst + at * 3 * ES, wk, 3 * n);
    } else {
        run_store<ES, COL_RUN>(g.dst + at * ES, wr, n);
        run_store<ES, COL_RUN>(g.dst + (plane + at) * ES, wg, n);
        run_store<ES, COL_RUN>(g.dst + (2 * plane + at) * ES, wb, n);
    }
}

template <int A, int LUT>
__global__ __launch_bounds__(PY_NT) void k_rgb_pyramid(PyArgs a)
{
    __shared__ __attribute__((aligned(16))) uint16_t s_row[PY_NW][2][RD_LDS];        // a wave's own staging rows
    __shared__ __attribute__((aligned(16))) uint16_t s_y[4][RD_BAND][RD_TW];        // the luma tile: [band * 2 + column walk]; after step 2: R
    __shared__ __attribute__((aligned(16))) uint16_t s_c[2][RD_BAND][RD_TW];        // the Cb and the Cr tile
    __shared__ uint16_t s_k[2][PY_TH][PY_TW];                                      // G, B
    const int tid = (int)threadIdx.x, lane = tid & (RD_NT - 1), wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b = (int)blockIdx.x;
    int lv = 0;
    while (lv + 1 < a.n_levels && b >= a.end[lv]) ++lv;                            // (of the workgroup's index alone: scalar)
    const PyLevel &g = a.r[lv];
    const int ti = b - g.first, ty = ti / g.ntx, tx = ti - ty * g.ntx;
    const int cw = g.dw >> 1, ch = g.dh >> 1;                                      // the reduced picture's chroma plane
    // the tile's own pixels X0 .. X1 - 1, Y0 .. Y1 - 1 (X0 a multiple of 8, the others of 4)
    const int X0 = tx * PY_TW, X1 = min(X0 + PY_TW, g.dw), Y0 = ty * PY_TH, Y1 = min(Y0 + PY_TH, g.dh);
    // the chroma the taps reach: columns X0 / 2 - 1 .. X1 / 2, rows Y0 / 2 - 1 .. Y1 / 2, clamped to the plane
    const int kc0 = max((X0 >> 1) - 1, 0), kc1 = min(X1 >> 1, cw - 1), kr0 = max((Y0 >> 1) - 1, 0), kr1 = min(Y1 >> 1, ch - 1);

    // 1. reduce: the tile's walks dealt to the waves; a walk's lanes wait for one another only
    for (int wk = wave; wk < PY_NWALK; wk += PY_NW) {
        if (wk < 4) {
            const int ka = Y0 + RD_BAND * (wk >> 1), k0 = X0 + RD_TW * (wk & 1);
            if (ka >= Y1 || k0 >= X1) continue;
            const RdTile t = { a.src[0], a.sstride[0], a.sw, a.sh, g.dw, g.dh, 0, 0, g.px, g.qx, g.py, g.qy, g.ntap, g.cpr, g.rows, g.n, g.rcp, 0, 0 };
            rd_walk_at(t, RdAt{ k0, min(k0 + RD_TW, X1) - 1, ka, min(ka + RD_BAND, Y1) }, s_row[wave], s_y[wk], PyNone{});
        } else {
            const RdTile t = { a.src[wk - 3], a.sstride[1], a.sw >> 1, a.sh >> 1, cw, ch, g.sgx, g.sgy, g.px, g.qx, g.py, g.qy, g.ntap, g.cpr, g.rows, g.n, g.rcp, 0, 0 };
            rd_walk_at(t, RdAt{ kc0, kc1, kr0, kr1 + 1 }, s_row[wave], s_c[wk - 4], PyNone{});
        }
    }
    __syncthreads();

    // 2. convert: this lane's columns xe, xe + 1, this wave's row pairs
    {
        const ColSrc &c = a.c[g.cs];
        const int peak = LUT ? 1023 : a.peak[g.cs];
        const int xe = X0 + 2 * lane;
        if (xe < X1) {
            const int m = xe >> 1;
            int ci[3];                                                             // the taps' columns m - 1, m, m + 1 in s_c
#pragma unroll
            for (int t = 0; t < 3; ++t) ci[t] = min(max(m - 1 + t, 0), cw - 1) - kc0;
            const int xi = xe - X0;                                                // in the tile
            const int s_all = a.l.S2 + a.l.S + 1;                                  // from a cell's vertex to the opposite corner
            for (int y0 = Y0 + 2 * wave; y0 < Y1; y0 += 2 * PY_NW) {
                int R[4], G[4], B[4];
#pragma unroll
                for (int r = 0; r < 2; ++r) {
                    const int y = y0 + r;                                          // (Y1 - Y0 is even: the pair is whole)
                    // vertical blend: V = 2y - b; rows j0, j0 + 1 of the reduced chroma plane, clamped
                    const int dv = 2 * y - c.b, fy = dv & 3, j0 = dv >> 2;
                    const int rlo = min(max(j0, 0), ch - 1) - kr0, rhi = min(max(j0 + 1, 0), ch - 1) - kr0;
                    int ub[6] = {}, vb[6] = {};
#pragma unroll
                    for (int t = 0; t < 3; ++t) {
                        ub[t] = (4 - fy) * (int)s_c[0][rlo][ci[t]] + fy * (int)s_c[0][rhi][ci[t]];
                        vb[t] = (4 - fy) * (int)s_c[1][rlo][ci[t]] + fy * (int)s_c[1][rhi][ci[t]];
                    }
#pragma unroll
                    for (int i = 0; i < 2; ++i)
                        col_pixel<A>(c, ub, vb, i, (int)py_y(s_y, xi + i, y - Y0), peak, R[2 * r + i], G[2 * r + i], B[2 * r + i]);
                }
                if constexpr (LUT) {
                    LutPoint p[4];
#pragma unroll
                    for (int q = 0; q < 4; ++q) p[q] = lut_point(R[q], G[q], B[q], a.l);
                    // the four pixels' gathers, all in flight together
                    uint2 t0v[4], t1v[4], t2v[4], t3v[4];
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        t0v[q] = a.l.texels[p[q].v0]; t1v[q] = a.l.texels[p[q].v1]; t2v[q] = a.l.texels[p[q].v2]; t3v[q] = a.l.texels[p[q].v0 + s_all];
                    }
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        uint32_t oR, oG, oB;
                        lut_mix(p[q].w1, p[q].w2, p[q].w3, t0v[q], t1v[q], t2v[q], t3v[q], oR, oG, oB);
                        R[q] = (int)oR; G[q] = (int)oG; B[q] = (int)oB;            // (at most the table's peak: 65535)
                    }
                }
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int ry = y0 + (q >> 1) - Y0, x = xi + (q & 1);
                    py_y(s_y, x, ry) = (uint16_t)R[q];
                    s_k[0][ry][x] = (uint16_t)G[q];
                    s_k[1][ry][x] = (uint16_t)B[q];
                }
            }
        }
    }
    __syncthreads();

    // 3. store: a lane owns a run of 8 pixels of a row (PY_RUNS x PY_TH = 180 runs at most)
    for (int it = tid; it < PY_RUNS * (Y1 - Y0); it += PY_NT) {
        const int yi = it / PY_RUNS, xi = COL_RUN * (it - yi * PY_RUNS);
        const int x = X0 + xi, n = min(COL_RUN, X1 - x);
        if (n <= 0) continue;
#define PY_STORE(DT) do { if (g.packed) py_store<DT, 1>(g, s_y, s_k, xi, yi, x, Y0 + yi, n, a.to_unit); else py_store<DT, 0>(g, s_y, s_k, xi, yi, x, Y0 + yi, n, a.to_unit); } while (0)
        switch (g.dtype) {
        case OVHIP_RGB_U8:  PY_STORE(OVHIP_RGB_U8); break;
        case OVHIP_RGB_U16: PY_STORE(OVHIP_RGB_U16); break;
        case OVHIP_RGB_F16: PY_STORE(OVHIP_RGB_F16); break;
        default:            PY_STORE(OVHIP_RGB_F32); break;
        }
#undef PY_STORE
    }
}

// the source stage's share of a coefficient set
void py_col_fill(ColSrc &c, const ovhip_rgb_plan_ &p)
{
    c.b = p.b;
    c.cy16 = 16 * p.coef[0]; c.rv = p.coef[1]; c.gu = p.coef[2]; c.gv = p.coef[3]; c.bu = p.coef[4]; c.yoff = p.yoff;
}

} // namespace

extern "C" int ovhip_rgb_pyramid_launch(ovhip_ctx *ctx, const ovhip_pic *src, const ovhip_reduce_info *info, const ovhip_rgb_level *levels, int32_t n,
                                        const ovhip_rgb_lut *lut)
{
    if (!ctx) return OVHIP_EINVAL;
    OV_DEVICE(ctx);
    if (!src) return ov_fail(ctx, OVHIP_EINVAL, "ovhip_rgb_pyramid_launch: null picture", hipSuccess);
    ovhip_rgb_pyramid_plan_ pl;
    char why[240];
    int r = ovhip_rgb_pyramid_plan_make_(src, 0, 0, info, levels, n, lut != NULL, lut ? lut->size : 0, lut ? lut->peak : 0, 1, &pl, why, sizeof(why));
    if (r == OVHIP_OK && lut && lut->device != ctx->device) { snprintf(why, sizeof(why), "the table lives on another device"); r = OVHIP_EINVAL; }
    if (r != OVHIP_OK) { snprintf(ctx->err, sizeof(ctx->err), "ovhip_rgb_pyramid_launch: %s", why); return r; }
    PyArgs a;
    memset(&a, 0, sizeof(a));
    const ovhip_reduce_plan_ &p0 = pl.red[0];                                  // (the region is the same in every level)
    rd_src_fill(a, src, p0);
    a.n_levels = n;
    a.peak[0] = 1023; a.peak[1] = 255;
    int64_t nb = 0;
    for (int k = 0; k < n; ++k) {
        const ovhip_reduce_plan_ &rp = pl.red[k];
        PyLevel &g = a.r[k];
        g.dst = (char *)levels[k].dst;
        rd_level_fill(g, rp);
        g.dtype = (int)levels[k].fmt.dtype; g.packed = levels[k].fmt.layout == OVHIP_RGB_PACKED;
        g.cs = pl.rgb[k].peak == 255;                                          // (the level's plan: by the table 1023 whatever the dtype)
        py_col_fill(a.c[g.cs], pl.rgb[k]);
        g.ntx = (rp.Wd + PY_TW - 1) / PY_TW;
        g.first = (int)nb;
        nb += (int64_t)g.ntx * ((rp.Hd + PY_TH - 1) / PY_TH);
        a.end[k] = (int)nb;
    }
    if (nb > 0x7FFFFFFF) return ov_fail(ctx, OVHIP_EINVAL, "ovhip_rgb_pyramid_launch: too many tiles", hipSuccess);      // (8 levels of 16384 x 16384: 1.5 M)
    a.to_unit = lut ? (float)(1.0 / lut->peak) : (float)(1.0 / 1023);
    if (lut) a.l = lut_args_fill(lut);
    const dim3 grid((unsigned)nb), block(PY_NT);
    if (pl.rgb[0].a) {
        if (lut) hipLaunchKernelGGL((k_rgb_pyramid<1, 1>), grid, block, 0, ctx->stream, a);
        else     hipLaunchKernelGGL((k_rgb_pyramid<1, 0>), grid, block, 0, ctx->stream, a);
    } else {
        if (lut) hipLaunchKernelGGL((k_rgb_pyramid<0, 1>), grid, block, 0, ctx->stream, a);
        else     hipLaunchKernelGGL((k_rgb_pyramid<0, 0>), grid, block, 0, ctx->stream, a);
    }
    OV_LAUNCH_CHECK(ctx, "k_rgb_pyramid");
    return OVHIP_OK;
}

extern "C" int ovhip_pic_output_rgb_pyramid(ovhip_ctx *ctx, const ovhip_pic *pic, const ovhip_reduce_info *info, const ovhip_rgb_level *levels, int32_t n,
                                            const ovhip_rgb_lut *lut)
{
    if (!ctx) return OVHIP_EINVAL;
    OV_DEVICE(ctx);
    if (!pic) return ov_fail(ctx, OVHIP_EINVAL, "ovhip_pic_output_rgb_pyramid: null picture", hipSuccess);
    if (!levels || n < 1 || n > OVHIP_PYRAMID_MAX_LEVELS) {
        /* the launch words the reason */
        const int q = ovhip_rgb_pyramid_launch(ctx, pic, info, levels, n, lut);
        return q != OVHIP_OK ? q : OVHIP_EINVAL;
    }
    OvStaged<ovhip_rgb_level> st(levels, n, [](const ovhip_rgb_level &g) { return ovhip_rgb_bytes(g.out_w, g.out_h, nullptr, &g.fmt); });
    return ov_stage_out(ctx, "ovhip_pic_output_rgb_pyramid", "level", st,
        [&](const ovhip_rgb_level *d) { return ovhip_rgb_pyramid_launch(ctx, pic, info, d, n, lut); },
        [&] {
            ovhip_rgb_pyramid_plan_ pl;
            char why[240];
            int q = ovhip_rgb_pyramid_plan_make_(nullptr, pic->w, pic->h, info, levels, n, lut != NULL, lut ? lut->size : 0, lut ? lut->peak : 0, 1, &pl, why, sizeof(why));
            if (q == OVHIP_OK && lut && lut->device != ctx->device) { snprintf(why, sizeof(why), "the table lives on another device"); q = OVHIP_EINVAL; }
            if (q != OVHIP_OK) snprintf(ctx->err, sizeof(ctx->err), "ovhip_pic_output_rgb_pyramid: %s", why);
            return q;
        },
        /* a level is dense: one copy */
        [&](const ovhip_rgb_level &d, void *host) { return hipMemcpyAsync(host, d.dst, d.dst_bytes, hipMemcpyDeviceToHost, ctx->stream); });
}
