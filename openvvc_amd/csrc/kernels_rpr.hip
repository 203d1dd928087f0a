// kernels_rpr.hip -- motion compensation from references of another size (reference picture resampling) on gfx950.
//
// One wavefront (= one 64-thread workgroup) per ovhip_rpr_unit (<= 16x16 luma + its 4:2:0 chroma), as k_mc2.  Per list
// and plane: the horizontal pass runs over the reference rows the tile's vertical positions need (up to 2 * 16 + 8 luma
// rows at 2:1) into an int16 LDS tile, the vertical pass runs from LDS into registers, then uni / average / BCW / GPM,
// clip, LMCS forward mapping and the CIIP blend, and the store.  Unlike k_mc2 the integer position, the phase and (per
// axis) the filter set vary per output column / row, so every lane fetches its own taps from a constant table.  Coordinates
// are clamped against EACH reference's own size: the device form of emulate_block_border (rcn_inter.c:148-225).
//
// Scaled side (rcn_mcp_rpr_l / _bi_l / _c / _bi_c, rcn_inter.c:2009-2512; leaves put_vvc_{qpel,epel}_rpr_*,
// put_vvc_pel_rpr*, rcn_mc.c:549-790): column c of the PU at (anchor + ((c * step) << shift_mv) + 8192) >> 14, integer part
// >> shift_mv, phase & (2^shift_mv - 1).  Unscaled side of a mixed bi unit (rcn_mcp_bidir0_l / _c): the regular 14-bit
// prediction with the regular filters of vvc_mc_taps.h (integer phase = identity row).  Combined as rpr_sum /
// rpr_w / gpm_weighted (rcn_mc.c:649-700, :1630-1655), then lmcs_reshape_forward.  int16 x int8 on the VALU, no MFMA.
//
// k_mca_rpr (second half of the file): the affine coding units that read a scaled reference, sub-block by sub-block.
#include "mc_common.hip.h"
#include "vvc_rpr_taps.h"

namespace {

#define RPR_LROWS 48    /* luma H tile rows: (15 * 2) + 1 + 7 at 2:1, rounded up */
#define RPR_CROWS 24    /* chroma: (7 * 2) + 1 + 3 */

struct RprTaps {
    int8_t rl[6][16][8];    // scaled luma sets
    int8_t rc[3][32][4];    // scaled chroma sets
    int8_t l[17][8];        // regular luma (row 16: half-pel smoothing)
    int8_t c[32][4];        // regular chroma
};
constexpr RprTaps build_rpr_taps()
{
    RprTaps t{};
    for (int s = 0; s < 6; ++s) for (int p = 0; p < 16; ++p) for (int k = 0; k < 8; ++k) t.rl[s][p][k] = ovt_rpr_luma[s][p][k];
    for (int s = 0; s < 3; ++s) for (int p = 0; p < 32; ++p) for (int k = 0; k < 4; ++k) t.rc[s][p][k] = ovt_rpr_chroma[s][p][k];
    for (int p = 0; p < 17; ++p) for (int k = 0; k < 8; ++k) t.l[p][k] = ovt_mc_luma[p][k];
    for (int p = 0; p < 32; ++p) for (int k = 0; k < 4; ++k) t.c[p][k] = ovt_mc_chroma[p][k];
    return t;
}
__device__ const RprTaps __attribute__((aligned(16))) g_rpr = build_rpr_taps();

// Integer position and phase of output index i (column or row) of list side s along one axis.
//   scaled: anchor a (int32 as the reference computes it, wrap included: unsigned arithmetic, arithmetic shifts)
//   unscaled: base = tile position in the picture (plane units) + (mv >> shift_mv), phase = mv & mask
struct Axis { int32_t a; uint32_t step; int sh; int base; int mvph; bool scaled; };
__device__ __forceinline__ void axis_pos(const Axis &ax, int i_pu, int i_tile, int &ip, int &ph)
{
    if (ax.scaled) {
        const int32_t pm = (int32_t)((uint32_t)ax.a + (((uint32_t)i_pu * ax.step) << ax.sh) + 8192u) >> 14;
        ip = pm >> ax.sh; ph = pm & ((1 << ax.sh) - 1);
    } else {
        ip = ax.base + i_tile; ph = ax.mvph;
    }
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// One list, one plane: H pass into tile, V pass; returns in out[] (per lane-owned sample, up to 4) either the 14-bit
// intermediate (bi) or the clipped sample (uni).  NT: 8 (luma) or 4 (chroma).
template <int NT, int ROWS>
__device__ __forceinline__ void rpr_plane(const uint16_t *__restrict__ ref, int rstride, int rw, int rh, const Axis &axx, const Axis &axy,
                                          int fh, int fv, bool hpel, bool uni, int w, int h, int ox, int oy, int16_t *tile, int lane,
                                          int out[4])
{
    constexpr int B = NT / 2 - 1;                   // taps before the position: 3 / 1
    int iy0, ph0, iyl, phl;
    axis_pos(axy, oy, 0, iy0, ph0);
    axis_pos(axy, oy + h - 1, h - 1, iyl, phl);
    const int rb = iy0 - B;
    const int nrows = min(iyl - iy0 + NT, ROWS);
    // horizontal: rows rb .. rb + nrows - 1, column c -> tile[r * 16 + c]
    for (int t = lane; t < nrows * w; t += 64) {
        const int r = t / w, c = t - r * w;
        int ix, ph;
        axis_pos(axx, ox + c, c, ix, ph);
        const int8_t *tp;
        if (NT == 8) tp = axx.scaled ? g_rpr.rl[fh][ph] : g_rpr.l[(hpel && ph == 8) ? 16 : ph];
        else         tp = axx.scaled ? g_rpr.rc[fh][ph] : g_rpr.c[ph];
        const uint16_t *row = ref + (size_t)clampi(rb + r, 0, rh - 1) * rstride;
        int acc = 0;
#pragma unroll
        for (int k = 0; k < NT; ++k) acc += (int)tp[k] * (int)row[clampi(ix - B + k, 0, rw - 1)];
        tile[r * 16 + c] = (int16_t)(acc >> (OV_BD - 8));
    }
    __syncthreads();
    int j = 0;
    for (int t = lane; t < w * h; t += 64, ++j) {
        const int r = t / w, c = t - r * w;
        int iy, ph;
        axis_pos(axy, oy + r, r, iy, ph);
        const int8_t *tp;
        if (NT == 8) tp = axy.scaled ? g_rpr.rl[fv][ph] : g_rpr.l[(hpel && ph == 8) ? 16 : ph];
        else         tp = axy.scaled ? g_rpr.rc[fv][ph] : g_rpr.c[ph];
        const int base = iy - iy0;
        int acc = 0;
#pragma unroll
        for (int k = 0; k < NT; ++k) acc += (int)tp[k] * (int)tile[min(base + k, ROWS - 1) * 16 + c];
        int v;
        if (!uni) {
            v = acc >> 6;                                                     // put_vvc_*_rpr_bi_v / put_vvc_pel_rpr_bi
        } else if (fv == 0 && ph == 0) {
            // put_vvc_pel_rpr_clip reads the horizontal intermediate as uint16: a negative one clips to the maximum
            v = ov_clip_bd(((int)(uint16_t)tile[min(base + B, ROWS - 1) * 16 + c] + 8) >> 4);
        } else {
            v = ov_clip_bd(((acc >> 6) + 8) >> 4);                            // put_vvc_*_rpr_clip_v
        }
        if (j < 4) out[j] = v;
    }
    __syncthreads();
}

// Combine, LMCS forward mapping, CIIP blend and store of one plane of a unit: P = rpr_plane's outputs per list (a uni-predicted
// unit's are finished samples already, the put_vvc_pel_rpr_clip quirk included), (x0, y0) / w x h the unit in the plane, pw x ph
// the plane; cs: the plane's subsampling shift, for the GPM weights' luma coordinates; lmcs / ip: nullptr = no mapping / no blend.
__device__ __forceinline__ void rpr_finish(const ovhip_rpr_unit &u, const int P[2][4], int x0, int y0, int w, int h, int pw, int ph, int cs,
                                           uint16_t *d, int dstride, const uint16_t *__restrict__ lmcs, const uint16_t *ip, int istride,
                                           int lane)
{
    const int dir = u.dir & 3;
    const Combine cmb = mc_combine_of(BiMode{ dir, u.w0, u.w1 });
    int j = 0;
    for (int t = lane; t < w * h; t += 64, ++j) {
        const int r = t / w, c = t - r * w;
        const int p0 = P[0][j & 3], p1 = P[1][j & 3];
        int v;
        if (dir != 3)                       v = dir == 1 ? p0 : p1;
        else if (u.flags & OVHIP_RPR_GPM)   v = mc_gpm(u.aux, c << cs, r << cs, p0, p1);
        else                                v = mc_combine(cmb, p0, p1);
        if (lmcs) v = lmcs[v];
        const int px = x0 + c, py = y0 + r;
        if (px >= pw || py >= ph) continue;
        if (ip) v = ciip_blend(v, ip[(size_t)py * istride + px], u.aux & 7);
        d[(size_t)py * dstride + px] = (uint16_t)v;
    }
}

__global__ __launch_bounds__(64) void k_mc_rpr(ovhip_pic dst, RefTable refs, const ovhip_rpr_unit *__restrict__ units, uint32_t n_units,
                                               const uint16_t *__restrict__ lmcs_fwd, ovhip_pic intra)
{
    __shared__ int16_t s_tile[RPR_LROWS * 16];
    if (blockIdx.x >= n_units) return;
    const ovhip_rpr_unit u = units[blockIdx.x];
    const int lane = threadIdx.x;
    const int dir = u.dir & 3;
    const bool uni = dir != 3, gpm = (u.flags & OVHIP_RPR_GPM) != 0, hpel = (u.flags & OVHIP_RPR_HPEL_FILT) != 0;
    const int w = u.w, h = u.h;
    if (!dir || w < 4 || h < 4 || w > 16 || h > 16) return;

    if (!(u.flags & OVHIP_RPR_NO_LUMA)) {
        int P[2][4] = { { 0, 0, 0, 0 }, { 0, 0, 0, 0 } };
        for (int l = 0; l < 2; ++l) {
            if (!(dir & (1 << l))) continue;
            const ovhip_rpr_side s = u.s[l];
            const ovhip_pic &rp = refs.p[min((int)s.ref, MC_MAX_REFS - 1)];
            const bool sc = (u.flags & (l ? OVHIP_RPR_S1 : OVHIP_RPR_S0)) != 0;
            const Axis ax = { s.pos_x, s.step_x, 4, u.x + (s.pos_x >> 4), s.pos_x & 15, sc };
            const Axis ay = { s.pos_y, s.step_y, 4, u.y + (s.pos_y >> 4), s.pos_y & 15, sc };
            rpr_plane<8, RPR_LROWS>(rp.y, rp.stride_y, rp.w, rp.h, ax, ay, min(s.filt & 15, 5), min(s.filt >> 4, 5), hpel && !sc, uni, w, h,
                                    u.ox, u.oy, s_tile, lane, P[l]);
        }
        rpr_finish(u, P, u.x, u.y, w, h, dst.w, dst.h, 0, dst.y, dst.stride_y, (u.flags & OVHIP_RPR_LMCS) ? lmcs_fwd : nullptr,
                   !gpm && u.aux ? intra.y : nullptr, intra.stride_y, lane);
    }
    if (!(u.flags & OVHIP_RPR_NO_CHROMA)) {
        const int wc = w >> 1, hc = h >> 1;
        for (int plane = 1; plane <= 2; ++plane) {
            int P[2][4] = { { 0, 0, 0, 0 }, { 0, 0, 0, 0 } };
            for (int l = 0; l < 2; ++l) {
                if (!(dir & (1 << l))) continue;
                const ovhip_rpr_side s = u.s[l];
                const ovhip_pic &rp = refs.p[min((int)s.ref, MC_MAX_REFS - 1)];
                const bool sc = (u.flags & (l ? OVHIP_RPR_S1 : OVHIP_RPR_S0)) != 0;
                const Axis ax = { s.cpos_x, s.step_x, 5, (u.x >> 1) + (s.pos_x >> 5), s.pos_x & 31, sc };
                const Axis ay = { s.cpos_y, s.step_y, 5, (u.y >> 1) + (s.pos_y >> 5), s.pos_y & 31, sc };
                rpr_plane<4, RPR_CROWS>(plane == 1 ? rp.cb : rp.cr, rp.stride_c, rp.w >> 1, rp.h >> 1, ax, ay, min(s.filt_c & 15, 2),
                                        min(s.filt_c >> 4, 2), false, uni, wc, hc, u.ox >> 1, u.oy >> 1, s_tile, lane, P[l]);
            }
            const uint16_t *ip = plane == 1 ? intra.cb : intra.cr;
            rpr_finish(u, P, u.x >> 1, u.y >> 1, wc, hc, dst.w >> 1, dst.h >> 1, 1, plane == 1 ? dst.cb : dst.cr, dst.stride_c, nullptr,
                       !gpm && u.aux && !(u.aux & 0x100) ? ip : nullptr, intra.stride_c, lane);
        }
    }
}

// =====================================================================================================
// Affine units that read a scaled reference (ovhip_aff_rpr_unit).  One wavefront per <= 16x16 luma area, lane = (sub-block,
// column) as in k_mca.  To the reference every 4x4 luma sub-block is a 4x4 PU of its own (rcn_mcp_b_l(2,2) / rcn_prof_mcp_b_l,
// rcn_inter.c:2815-2918): the recorder left its anchor after clip_rpr_position (scaled list) or its clip_mv()'d vector (unscaled
// list) in the side arena.  Per list: the lane runs the horizontal pass of its column over the sub-block's own reference rows
// (at most (3 * step >> 14) + 1 + 7 = 14 at 2:1, one more when the phase carries) into the sub-block's int16 LDS tile and the
// vertical pass from it -- the lane reads back what it wrote, so the luma passes need no barrier.  Scaled lists take the "4x4"
// filter sets 3..5 (flag_4x4), the unscaled side of a mixed bi-prediction the 6-tap filters of 4x4 blocks (put_vvc_qpel_*
// with width == height == 4, rcn_mc.c:457, as rcn_mcp_bidir0_l / rcn_prof_mcp_bi_l call them) and, with its PROF bit, the
// refinement on a 6x6 tile (extend_prof_buff / compute_prof_grad / rcn_prof, rcn_prof_bdof.c:152-290).  Chroma: the 4x4 blocks
// of each 8x8 luma area (rcn_mcp_b_c(3,3): sets 0..2, the put_vvc_pel_rpr_clip uint16 quirk included), lanes 0..31.
// =====================================================================================================
#define MCAR_ROWS 16

struct Rpr4Taps { int8_t l4[16][8]; };
constexpr Rpr4Taps build_rpr4_taps()
{
    Rpr4Taps t{};
    for (int p = 0; p < 16; ++p) for (int k = 0; k < 8; ++k) t.l4[p][k] = ovt_mc_luma4[p][k];
    return t;
}
__device__ const Rpr4Taps __attribute__((aligned(16))) g_rpr4 = build_rpr4_taps();

// One list of one 4x4 block (luma sub-block: NT 8, chroma block: NT 4), the lane's column c: 14-bit intermediates of its 4
// samples in out[]; *quirk: the vertical pass of sample j is put_vvc_pel_rpr_clip's (bit j; uni-prediction reads q[] instead).
template <int NT>
__device__ __forceinline__ void mcar_block(const uint16_t *__restrict__ ref, int rstride, int rw, int rh, const Axis &axx, const Axis &axy,
                                           int fh, int fv, int c, int16_t *tile /* [MCAR_ROWS][4] */, int out[4], int q[4])
{
    constexpr int B = NT / 2 - 1;
    int iy[4], phy[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) axis_pos(axy, j, j, iy[j], phy[j]);
    const int rb = iy[0] - B;
    const int nrows = clampi(iy[3] - iy[0] + NT, 0, MCAR_ROWS);
    int ix, phx;
    axis_pos(axx, c, c, ix, phx);
    const int8_t *tp;
    if (NT == 8) tp = axx.scaled ? g_rpr.rl[fh][phx] : g_rpr4.l4[phx];
    else         tp = axx.scaled ? g_rpr.rc[fh][phx] : g_rpr.c[phx];
    int t[NT], xo[NT];
#pragma unroll
    for (int k = 0; k < NT; ++k) { t[k] = tp[k]; xo[k] = clampi(ix - B + k, 0, rw - 1); }
    for (int r = 0; r < nrows; ++r) {
        const uint16_t *row = ref + (size_t)clampi(rb + r, 0, rh - 1) * rstride;
        int acc = 0;
#pragma unroll
        for (int k = 0; k < NT; ++k) acc += t[k] * (int)row[xo[k]];
        tile[r * 4 + c] = (int16_t)(acc >> (OV_BD - 8));
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int8_t *tv;
        if (NT == 8) tv = axy.scaled ? g_rpr.rl[fv][phy[j]] : g_rpr4.l4[phy[j]];
        else         tv = axy.scaled ? g_rpr.rc[fv][phy[j]] : g_rpr.c[phy[j]];
        const int base = iy[j] - iy[0];
        int acc = 0;
#pragma unroll
        for (int k = 0; k < NT; ++k) acc += (int)tv[k] * (int)tile[clampi(base + k, 0, MCAR_ROWS - 1) * 4 + c];
        out[j] = acc >> 6;
        q[j] = (axy.scaled && fv == 0 && phy[j] == 0) ? (int)(uint16_t)tile[clampi(base + B, 0, MCAR_ROWS - 1) * 4 + c] : -1;
    }
}

__global__ __launch_bounds__(64) void k_mca_rpr(ovhip_pic dst, RefTable refs, const ovhip_aff_rpr_unit *__restrict__ units, uint32_t n_units,
                                                const int32_t *__restrict__ side, const uint16_t *__restrict__ lmcs_fwd)
{
    __shared__ int16_t s_tile[16][MCAR_ROWS * 4];
    __shared__ int16_t s_t[16][36];
    if (blockIdx.x >= n_units) return;
    const ovhip_aff_rpr_unit u = units[blockIdx.x];
    const int lane = threadIdx.x;
    const int udir = u.dir & 3;
    if (!udir || u.w < 4 || u.h < 4 || u.w > 16 || u.h > 16 || ((u.w | u.h) & 3)) return;
    const int nsx = u.w >> 2, nsb = nsx * (u.h >> 2), ncx = u.w >> 3, ncb = ncx * (u.h >> 3);
    const bool do_c = !(u.flags & OVHIP_AFFR_NO_CHROMA) && !((u.w | u.h) & 7);        // (a lone 4x4 luma block has none)
    const int32_t *mvs = side + u.side_off;

    // ---- luma: lane = (sub-block sb, column c) ----
    {
        const int sb = lane >> 2, c = lane & 3;
        const bool act = sb < nsb;
        const int bx = u.x + 4 * (sb % nsx), by = u.y + 4 * (sb / nsx);
        const int dir = ((u.ident_l >> sb) & 1) ? 2 : udir;
        int P[2][4] = { { 0, 0, 0, 0 }, { 0, 0, 0, 0 } };
#pragma unroll
        for (int l = 0; l < 2; ++l) {
            const bool on = act && (dir & (1 << l));
            const bool sc = (u.flags & (l ? OVHIP_AFFR_S1 : OVHIP_AFFR_S0)) != 0;
            const bool prof = (u.flags & OVHIP_AFFR_PROF) && udir == 3 && !sc && ((u.prof_dir >> l) & 1);      // uniform
            const ovhip_aff_rpr_list s = u.s[l];
            const ovhip_pic &rp = refs.p[min((int)s.ref, MC_MAX_REFS - 1)];
            int a = 0, b = 0;
            if (on) { a = mvs[4 * sb + 2 * l]; b = mvs[4 * sb + 2 * l + 1]; }
            if (on) {
                const Axis ax = { a, s.step_x, 4, bx + (a >> 4), a & 15, sc };
                const Axis ay = { b, s.step_y, 4, by + (b >> 4), b & 15, sc };
                int q[4];
                mcar_block<8>(rp.y, rp.stride_y, rp.w, rp.h, ax, ay, min(s.filt & 15, 5), min(s.filt >> 4, 5), c, s_tile[sb], P[l], q);
            }
            if (prof) {
                if (on) {
                    const int rx = bx + (a >> 4) - 1 + ((a & 15) >> 3), ry = by + (b >> 4) - 1 + ((b & 15) >> 3);
                    prof_fill(s_t[sb], c, P[l], [&](int i, int j) {
                        return (int)rp.y[(size_t)clampi(ry + j, 0, rp.h - 1) * rp.stride_y + clampi(rx + i, 0, rp.w - 1)];
                    });
                }
                __syncthreads();
                if (on) {
                    const int16_t *pt = reinterpret_cast<const int16_t *>(side + u.prof_off) + 32 * l;
                    int pdx[4], pdy[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) { pdx[j] = pt[4 * j + c]; pdy[j] = pt[16 + 4 * j + c]; }
                    prof_refine(s_t[sb], c, pdx, pdy, P[l]);
                }
                __syncthreads();
            }
        }
        if (act) {
            const Combine cmb = mc_combine_of(BiMode{ dir, u.w0, u.w1 });
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                int v = mc_combine(cmb, P[0][j], P[1][j]);
                if ((u.flags & OVHIP_AFFR_LMCS) && lmcs_fwd) v = lmcs_fwd[v];
                const int px = bx + c, py = by + j;
                if (px < dst.w && py < dst.h) dst.y[(size_t)py * dst.stride_y + px] = (uint16_t)v;
            }
        }
    }
    // ---- chroma: lanes 0..31 = (plane, block, column), both lists; the tiles are the lane's own again ----
    if (do_c && lane < 32) {
        const int comp = lane >> 4, blk = (lane >> 2) & 3, c = lane & 3;
        if (blk < ncb) {
            const int cbx = (u.x >> 1) + 4 * (blk % ncx), cby = (u.y >> 1) + 4 * (blk / ncx);
            const int dir = ((u.ident_c >> blk) & 1) ? 2 : udir;
            int P[2][4] = { { 0, 0, 0, 0 }, { 0, 0, 0, 0 } }, Q[2][4] = { { -1, -1, -1, -1 }, { -1, -1, -1, -1 } };
#pragma unroll
            for (int l = 0; l < 2; ++l) {
                if (!(dir & (1 << l))) continue;
                const bool sc = (u.flags & (l ? OVHIP_AFFR_S1 : OVHIP_AFFR_S0)) != 0;
                const ovhip_aff_rpr_list s = u.s[l];
                const ovhip_pic &rp = refs.p[min((int)s.ref, MC_MAX_REFS - 1)];
                const int a = mvs[4 * (nsb + blk) + 2 * l], b = mvs[4 * (nsb + blk) + 2 * l + 1];
                const Axis ax = { a, s.step_x, 5, cbx + (a >> 5), a & 31, sc };
                const Axis ay = { b, s.step_y, 5, cby + (b >> 5), b & 31, sc };
                mcar_block<4>(comp ? rp.cr : rp.cb, rp.stride_c, rp.w >> 1, rp.h >> 1, ax, ay, min(s.filt_c & 15, 2), min(s.filt_c >> 4, 2), c,
                              s_tile[comp * 4 + blk], P[l], Q[l]);
            }
            uint16_t *d = comp ? dst.cr : dst.cb;
            const Combine cmb = mc_combine_of(BiMode{ dir, u.w0, u.w1 });
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                int v = mc_combine(cmb, P[0][j], P[1][j]);
                // put_vvc_pel_rpr_clip reads the horizontal intermediate as uint16: a negative one clips to the maximum
                const int qv = dir == 1 ? Q[0][j] : Q[1][j];
                if (dir != 3 && qv >= 0) v = ov_clip_bd((qv + 8) >> 4);
                const int px = cbx + c, py = cby + j;
                if (px < (dst.w >> 1) && py < (dst.h >> 1)) d[(size_t)py * dst.stride_c + px] = (uint16_t)v;
            }
        }
    }
}

} // namespace

extern "C" int ovhip_mca_rpr_launch(ovhip_ctx *ctx, const ovhip_pic *dst, const ovhip_pic *refs, uint32_t n_refs,
                                    const ovhip_aff_rpr_unit *d_units, uint32_t n_units, const int32_t *d_side,
                                    const uint16_t *d_lmcs_fwd_lut)
{
    if (!ctx || !dst) return OVHIP_EINVAL;
    OV_DEVICE(ctx);
    if (!n_units) return OVHIP_OK;
    if (!d_units || !d_side) return ov_fail(ctx, OVHIP_EINVAL, "ovhip_mca_rpr_launch: null units / side arena", hipSuccess);
    RefTable t;
    if (int e = ref_table(ctx, &t, refs, n_refs, nullptr, "ovhip_mca_rpr_launch")) return e;
    hipLaunchKernelGGL(k_mca_rpr, dim3(n_units), dim3(64), 0, ctx->stream, *dst, t, d_units, n_units, d_side, d_lmcs_fwd_lut);
    OV_LAUNCH_CHECK(ctx, "k_mca_rpr");
    return OVHIP_OK;
}

extern "C" int ovhip_mc_rpr_launch(ovhip_ctx *ctx, const ovhip_pic *dst, const ovhip_pic *refs, uint32_t n_refs,
                                   const ovhip_rpr_unit *d_units, uint32_t n_units, const uint16_t *d_lmcs_fwd_lut,
                                   const ovhip_pic *intra)
{
    if (!ctx || !dst) return OVHIP_EINVAL;
    OV_DEVICE(ctx);
    if (!n_units) return OVHIP_OK;
    if (!d_units) return ov_fail(ctx, OVHIP_EINVAL, "ovhip_mc_rpr_launch: null units", hipSuccess);
    RefTable t;
    if (int e = ref_table(ctx, &t, refs, n_refs, nullptr, "ovhip_mc_rpr_launch")) return e;
    hipLaunchKernelGGL(k_mc_rpr, dim3(n_units), dim3(64), 0, ctx->stream, *dst, t, d_units, n_units, d_lmcs_fwd_lut,
                       intra ? *intra : *dst);
    OV_LAUNCH_CHECK(ctx, "k_mc_rpr");
    return OVHIP_OK;
}
