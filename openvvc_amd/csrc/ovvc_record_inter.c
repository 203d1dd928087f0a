/* ovvc_record_inter.c -- host recorder, inter prediction part (plain C, no GPU needed).
 *
 * The control part of the reference's inter orchestrators: which lists a block reads, where each list's vector goes last
 * (clip_mv, or the anchor after clip_rpr_position for a list on a reference of another size), the weights, and the cut into the
 * units of at most 16x16 luma samples the motion-compensation kernels take.  Behaviour restated from (never copied):
 *   rcn_mcp_b dispatch, clip_mv, identical motion, AMVR half-pel, BCW
 *                                           libovvc/rcn_inter.c:89-109, :256-268, :520-602, :2769-2813
 *   rcn_gpm_b, rcn_mc_rpr_b_l / _c          libovvc/rcn_inter.c:3118-3143, :2009-2736
 *   rcn_affine_mcp_b_l / _prof_ / _c        libovvc/drv_affine_mvp.c:3264-3411
 */
#include <stdlib.h>
#include <string.h>
#include "ovvc_hip.h"
#include "ovvc_record_priv.h"

/* ---------------------------------------------------------------- prediction units */
static int32_t clip3(int32_t v, int32_t lo, int32_t hi) { return v < lo ? lo : v > hi ? hi : v; }

static void
clip_mv(const ovhip_recorder *r, int px, int py, int pw, int ph, int32_t *mvx, int32_t *mvy)
{
    /* clip_mv(): keeps the reference window within [-(pb+3), pic+2] of the block position */
    *mvx = clip3(*mvx, -((pw + 3 + px) << 4), (r->pic_w + 2 - px) << 4);
    *mvy = clip3(*mvy, -((ph + 3 + py) << 4), (r->pic_h + 2 - py) << 4);
}

/* the weights of a bi-prediction (BCW; 4 / 4 for everything else) */
static int
bcw_weights(int dir, int bcw_idx_plus1, int8_t *w0, int8_t *w1)
{
    static const int8_t bcw[5] = { -2, 3, 4, 5, 10 };
    *w0 = *w1 = 4;
    if (dir != 3 || bcw_idx_plus1 == 0 || bcw_idx_plus1 == 3) return OVHIP_OK;
    if (bcw_idx_plus1 > 5) return OVHIP_EINVAL;
    *w1 = bcw[bcw_idx_plus1 - 1];
    *w0 = (int8_t)(8 - *w1);
    return OVHIP_OK;
}

/* the cut of a PU / CU into units of at most 16x16 luma samples; returns their number */
static int
tile_extent(int pw, int ph, int *uw, int *uh)
{
    *uw = pw > 16 ? 16 : pw; *uh = ph > 16 ? 16 : ph;
    return (pw / *uw) * (ph / *uh);
}

/* ovhip_mc_unit.aux of the unit at (ux, uy) of a GPM CU with the weight plane K + A x + B y */
static uint32_t
gpm_aux(int K, int A, int B, int ux, int uy)
{
    const int k = K + A * ux + B * uy;
    return ((uint32_t)k & 0xffff) | ((uint32_t)(A & 0xff) << 16) | ((uint32_t)(B & 0xff) << 24);
}

/* ... of a CIIP CU: the fused blend (rcn_ciip_weighted_sum); chroma of a CU 4 luma samples wide keeps the inter prediction */
static uint32_t
ciip_aux(const ovhip_pu_desc *pu)
{
    return pu->ciip_wt ? (uint32_t)(pu->ciip_wt & 7) | (pu->log2_w <= 2 ? 0x100u : 0u) : 0;
}

/* rcn_mcp_b: bi with identical motion degenerates to uni-pred from list 1 (0: a malformed inter_dir) */
static int
pu_dir(const ovhip_pu_desc *pu)
{
    const int dir = pu->inter_dir & 3;
    if (dir == 3) return pu->poc0 == pu->poc1 && pu->mv0x == pu->mv1x && pu->mv0y == pu->mv1y ? 2 : 3;
    return (dir & 2) ? 2 : dir;
}

/* bdof_enable / dmvr_enable CUs: the reference's caller cuts the CU into <=16x16 blocks and hands each
 * to rcn_bdof_mcp_l (+ one rcn_mcp_b_c for the CU's chroma) or rcn_dmvr_mv_refine
 * (vcl_coding_unit.c:2450-2472, :2598-2668). */
static int
rec_pu_refined(ovhip_recorder *r, const ovhip_pu_desc *pu)
{
    const int pw = 1 << pu->log2_w, ph = 1 << pu->log2_h;
    const int dmvr = (pu->refine & OVHIP_PU_DMVR) != 0;
    int uw, uh, n = 0;
    if ((pu->inter_dir & 3) != 3 || pw < 8 || ph < 8 || pw * ph < 128) return OVHIP_EINVAL;   /* check_bdof() */
    tile_extent(pw, ph, &uw, &uh);

    uint8_t flags = (pu->refine & OVHIP_PU_BDOF) ? OVHIP_MC_BDOF : 0;
    if (dmvr) flags |= OVHIP_MC_DMVR;
    if (pu->prec_amvr_half) flags |= OVHIP_MC_HPEL_FILT;
    if (pu->lmcs)           flags |= OVHIP_MC_LMCS;

    /* chroma of a BDOF-only CU: rcn_mcp_b_c clips the MVs against the CU, not the 16x16 block */
    int32_t c0x = pu->mv0x, c0y = pu->mv0y, c1x = pu->mv1x, c1y = pu->mv1y;
    clip_mv(r, pu->x0, pu->y0, pw, ph, &c0x, &c0y);
    clip_mv(r, pu->x0, pu->y0, pw, ph, &c1x, &c1y);

    /* ... and still applies its identical-motion shortcut (rcn_inter.c:2935-2951; never true for a
     * conforming bdof_enable, whose references lie on opposite sides of the current picture) */
    const int ident = pu->poc0 == pu->poc1 && pu->mv0x == pu->mv1x && pu->mv0y == pu->mv1y;

    for (int uy = 0; uy < ph; uy += uh) {
        for (int ux = 0; ux < pw; ux += uw) {
            ovhip_mc_unit u;
            memset(&u, 0, sizeof(u));
            u.x = (uint16_t)(pu->x0 + ux); u.y = (uint16_t)(pu->y0 + uy);
            u.w = (uint8_t)uw; u.h = (uint8_t)uh;
            u.dir = 3; u.flags = flags;
            u.ref0 = pu->ref0; u.ref1 = pu->ref1;
            u.w0 = u.w1 = 4;
            u.mv0x = pu->mv0x; u.mv0y = pu->mv0y; u.mv1x = pu->mv1x; u.mv1y = pu->mv1y;
            int split_chroma = 0;
            if (!dmvr) {
                clip_mv(r, u.x, u.y, uw, uh, &u.mv0x, &u.mv0y);       /* rcn_bdof_mcp_l, rcn_inter.c:1166-1170 */
                clip_mv(r, u.x, u.y, uw, uh, &u.mv1x, &u.mv1y);
                split_chroma = ident || u.mv0x != c0x || u.mv0y != c0y || u.mv1x != c1x || u.mv1y != c1y;
                if (split_chroma) u.flags |= OVHIP_MC_NO_CHROMA;
                if (!(pu->planes & 2)) { u.flags |= OVHIP_MC_NO_CHROMA; split_chroma = 0; }   /* rcn_bdof_mcp_l alone */
            }
            if (grow((void **)&r->mcx, &r->cap_mcx, r->n_mcx + 1, sizeof(u))) return OVHIP_ENOMEM;
            r->mcx[r->n_mcx++] = u;
            ++n;
            if (split_chroma) {
                /* the two clips disagree (block far outside the picture): chroma as a plain unit */
                u.flags = (uint8_t)((flags & OVHIP_MC_HPEL_FILT) | OVHIP_MC_NO_LUMA);
                if (ident) u.dir = 2;
                u.mv0x = c0x; u.mv0y = c0y; u.mv1x = c1x; u.mv1y = c1y;
                if (grow((void **)&r->mc, &r->cap_mc, r->n_mc + 1, sizeof(u))) return OVHIP_ENOMEM;
                r->mc[r->n_mc++] = u;
                ++n;
            }
        }
    }
    return n;
}

/* rcn_gpm_b (rcn_inter.c:3118-3143) -> rcn_mc_rpr_b_l/_c with gpm_ctx: two uni-predictions of the whole CU
 * (rcn_mcp_bidir0_l/_c: clip_mv against the CU) blended by put_weighted_gpm_bi_pixels with the weight plane
 * of rcn_gpm_weights_and_steps.  The reference walks mirrored pre-stored masks (rcn_gpm.c:149-205); the plane
 * is affine in the sample position, so the command carries it in closed form (H.266 8.5.7.2):
 *   weightIdx = ((x + offX) * 2 + 1) * dis[angle] + ((y + offY) * 2 + 1) * dis[angle + 8]
 *   w = clip3(0, 8, ((partFlip ? 32 + weightIdx : 32 - weightIdx) + 4) >> 3) */
#include "vvc_gpm_tables.h"
static void
gpm_plane(const ovhip_pu_desc *pu, int *pK, int *pA, int *pB)
{
    const int pw = 1 << pu->log2_w, ph = 1 << pu->log2_h;
    const int angle = ovt_gpm_params[pu->gpm_split_dir][0], dist = ovt_gpm_params[pu->gpm_split_dir][1];
    const int dx = ovt_gpm_dis[angle], dy = ovt_gpm_dis[(angle + 8) & 31];
    const int flip = (angle >= 13 && angle <= 27) ? 0 : 1;
    const int shift_hor = (angle % 16 == 8 || (angle % 16 != 0 && ph >= pw)) ? 0 : 1;
    int off_x = -(pw >> 1), off_y = -(ph >> 1);
    if (dist > 0) {
        if (!shift_hor) off_y += angle < 16 ? (dist * ph) >> 3 : -((dist * ph) >> 3);
        else            off_x += angle < 16 ? (dist * pw) >> 3 : -((dist * pw) >> 3);
    }
    const int sgn = flip ? 1 : -1;
    const int A = sgn * 2 * dx, B = sgn * 2 * dy;
    *pK = 36 + sgn * ((2 * off_x + 1) * dx + (2 * off_y + 1) * dy);
    *pA = A; *pB = B;
}

static int
rec_pu_gpm(ovhip_recorder *r, const ovhip_pu_desc *pu)
{
    const int pw = 1 << pu->log2_w, ph = 1 << pu->log2_h;
    int K, A, B;
    gpm_plane(pu, &K, &A, &B);

    int32_t mv0x = pu->mv0x, mv0y = pu->mv0y, mv1x = pu->mv1x, mv1y = pu->mv1y;
    clip_mv(r, pu->x0, pu->y0, pw, ph, &mv0x, &mv0y);
    clip_mv(r, pu->x0, pu->y0, pw, ph, &mv1x, &mv1y);

    uint8_t flags = OVHIP_MC_GPM;
    if (pu->prec_amvr_half) flags |= OVHIP_MC_HPEL_FILT;
    if (pu->lmcs)           flags |= OVHIP_MC_LMCS;
    int uw, uh, n = 0;
    tile_extent(pw, ph, &uw, &uh);
    for (int uy = 0; uy < ph; uy += uh) {
        for (int ux = 0; ux < pw; ux += uw) {
            if (grow((void **)&r->mc, &r->cap_mc, r->n_mc + 1, sizeof(ovhip_mc_unit))) return OVHIP_ENOMEM;
            ovhip_mc_unit *u = &r->mc[r->n_mc++];
            memset(u, 0, sizeof(*u));
            u->x = (uint16_t)(pu->x0 + ux); u->y = (uint16_t)(pu->y0 + uy);
            u->w = (uint8_t)uw; u->h = (uint8_t)uh;
            u->dir = 3; u->flags = flags;
            u->ref0 = pu->ref0; u->ref1 = pu->ref1;
            u->w0 = u->w1 = 4;
            u->mv0x = mv0x; u->mv0y = mv0y; u->mv1x = mv1x; u->mv1y = mv1y;
            u->aux = gpm_aux(K, A, B, ux, uy);
            ++n;
        }
    }
    return n;
}

/* ---------------------------------------------------------------- reference picture resampling */
static const ovhip_ref_scale rpr_default = { OVHIP_RPR_UNSCALED, OVHIP_RPR_UNSCALED, 0, 0, 0, 0, { 0, 0 } };

void
ovhip_rec_rpr_reset_(ovhip_recorder *r)
{
    r->n_rpr = 0;
    r->n_affr = 0;
    r->refusal = "";
    if (r->n_scaled || !r->ref_scale[0].scale_hor) {
        for (int i = 0; i < 256; ++i) r->ref_scale[i] = rpr_default;
        r->n_scaled = 0;
    }
}

int
ovhip_rec_set_ref_scale(ovhip_recorder *r, int32_t slot, const ovhip_ref_scale *sc)
{
    if (!r || slot < 0 || slot > 255) return OVHIP_EINVAL;
    if (sc && (sc->scale_hor < (OVHIP_RPR_UNSCALED >> 3) || sc->scale_hor > 2 * OVHIP_RPR_UNSCALED ||
               sc->scale_ver < (OVHIP_RPR_UNSCALED >> 3) || sc->scale_ver > 2 * OVHIP_RPR_UNSCALED ||
               sc->ref_w < 0 || sc->ref_h < 0 || sc->ref_w > 16384 || sc->ref_h > 16384 ||
               sc->chroma_hor_col_flag > 1 || sc->chroma_ver_col_flag > 1))
        return OVHIP_EINVAL;     /* H.266: a reference at most 2x larger and 8x smaller than the picture */
    if (r->log) ovhip_calllog_ref_scale_(r->log, slot, sc);
    ovhip_ref_scale *d = &r->ref_scale[slot];
    const int was = memcmp(d, &rpr_default, sizeof(*d)) != 0;
    *d = sc ? *sc : rpr_default;
    memset(d->pad, 0, sizeof(d->pad));
    const int is = memcmp(d, &rpr_default, sizeof(*d)) != 0;
    r->n_scaled += (uint32_t)(is - was);
    return OVHIP_OK;
}

int
ovhip_rec_set_rpr_tools(ovhip_recorder *r, uint32_t mask)
{
    if (!r || (mask & ~(OVHIP_RPR_TOOL_AFFINE | OVHIP_RPR_TOOL_PU4x4))) return OVHIP_EINVAL;
    r->rpr_tools = mask;
    return OVHIP_OK;
}

const char *ovhip_rec_refusal(const ovhip_recorder *r) { return r ? r->refusal : ""; }

static int
refuse(ovhip_recorder *r, const char *why)
{
    r->refusal = why;
    return OVHIP_EUNSUP;
}

static int is_scaled(const ovhip_ref_scale *s) { return s->scale_hor != OVHIP_RPR_UNSCALED || s->scale_ver != OVHIP_RPR_UNSCALED; }

/* 1: the slot is scaled, 0: regular prediction, <0: refused (a scale of 1 on a reference of another size) */
static int
slot_scaled(ovhip_recorder *r, int slot)
{
    const ovhip_ref_scale *s = &r->ref_scale[slot];
    if (is_scaled(s)) return 1;
    if ((s->ref_w && s->ref_w != r->pic_w) || (s->ref_h && s->ref_h != r->pic_h))
        return refuse(r, "reference picture resampling: scale 1 on a reference of another size");
    return 0;
}

/* the same without touching the refusal: does a call with these lists take a path ovhip_rec_set_rpr_tools opened? */
static int
reads_scaled(const ovhip_recorder *r, int dir, int ref0, int ref1)
{
    if (!r->n_scaled) return 0;
    return ((dir & 1) && is_scaled(&r->ref_scale[ref0])) || ((dir & 2) && is_scaled(&r->ref_scale[ref1]));
}

/* compute_rpr_filter_idx (rcn_inter.c:1991-2006) */
static int
rpr_filter_idx(int scale, int flag_4x4)
{
    int idx = flag_4x4 ? 3 : 0;
    if (scale > OVHIP_RPR_UNSCALED * 7 / 4) idx += 2;
    else if (scale > OVHIP_RPR_UNSCALED * 5 / 4) idx += 1;
    return idx;
}

/* What the units of a scaled list carry of its slot, and what their anchors are computed from. */
struct rpr_slot {
    int32_t  scale_x, scale_y;
    uint16_t step_x, step_y;  /* ((scale + 8) >> 4) << 4                                                        */
    uint8_t  filt, filt4;     /* filter sets, horizontal | vertical << 4: 0..2, and 3..5 of 4x4 blocks (flag_4x4) */
    int32_t  add_x, add_y;    /* chroma: from the collocation flags (rcn_inter.c:2322-2323)                     */
    int32_t  ref_w, ref_h;    /* the reference's luma size (the picture's where the caller gave none)           */
};

static void
rpr_slot_fill(const ovhip_recorder *r, int slot, struct rpr_slot *s)
{
    const ovhip_ref_scale *sc = &r->ref_scale[slot];
    s->scale_x = sc->scale_hor; s->scale_y = sc->scale_ver;
    s->step_x = (uint16_t)(((sc->scale_hor + 8) >> 4) << 4);
    s->step_y = (uint16_t)(((sc->scale_ver + 8) >> 4) << 4);
    s->filt  = (uint8_t)(rpr_filter_idx(sc->scale_hor, 0) | rpr_filter_idx(sc->scale_ver, 0) << 4);
    s->filt4 = (uint8_t)(rpr_filter_idx(sc->scale_hor, 1) | rpr_filter_idx(sc->scale_ver, 1) << 4);
    s->add_x = (1 - sc->chroma_hor_col_flag) * 8 * (sc->scale_hor - OVHIP_RPR_UNSCALED);
    s->add_y = (1 - sc->chroma_ver_col_flag) * 8 * (sc->scale_ver - OVHIP_RPR_UNSCALED);
    s->ref_w = sc->ref_w ? sc->ref_w : r->pic_w;
    s->ref_h = sc->ref_h ? sc->ref_h : r->pic_h;
}

/* One axis of the anchor of rcn_mcp_rpr_l / _c: ref_pos = ((pos << shift_mv) + mv) * scale + add + (1 << (shift_mv + 3)),
 * the extent ref_pu_* of the PU in the reference, then clip_rpr_position (rcn_inter.c:2009-2026).  The reference computes in
 * int32 and wraps at 4K with large vectors; the same wrap here in explicit unsigned 32-bit arithmetic (arithmetic shifts of
 * the wrapped value, as the compiled reference does). */
static int32_t
rpr_anchor(int32_t pos, int32_t mv, int32_t scale, int32_t add, int pu_len, int pic_len, int shift_mv, int min1)
{
    const int shift_pos = 14 + shift_mv;
    const uint32_t offset = 1u << 13;
    const uint32_t step = (uint32_t)(((scale + 8) >> 4) << 4);
    const int32_t ref_pos = (int32_t)((((uint32_t)pos << shift_mv) + (uint32_t)mv) * (uint32_t)scale + (uint32_t)add + (1u << (shift_mv + 3)));
    const int32_t ref_i = (int32_t)((uint32_t)ref_pos + offset) >> shift_pos;
    int32_t ext = ((int32_t)((uint32_t)ref_pos + (((uint32_t)(pu_len - 1) * step) << shift_mv) + offset) >> shift_pos) - ref_i + 1;
    if (min1 && ext < 1) ext = 1;
    const int32_t prec = ref_pos & ((1 << shift_pos) - 1);
    const int32_t hi = (int32_t)((uint32_t)(pic_len + 3) << shift_pos);
    const int32_t lo = (int32_t)(0u - ((uint32_t)(ext + 4) << shift_pos));
    int32_t v = ref_pos;
    const int32_t a = (int32_t)((uint32_t)lo + (uint32_t)prec), b = (int32_t)((uint32_t)hi + (uint32_t)prec);
    v = v > a ? v : a;                 /* ov_clip = min(max(v, a), b) */
    v = v < b ? v : b;
    return v;
}

/* Where one list's vector of the w x h luma block at (x, y) goes last: the regular 14-bit prediction clips it against the block
 * (rcn_mcp_bidir0_l / _c); a scaled list (sl) turns it into the anchor of the block (chroma: of its 4:2:0 chroma block). */
static inline void
place_mv(const ovhip_recorder *r, const struct rpr_slot *sl, int chroma, int x, int y, int w, int h, int32_t *mvx, int32_t *mvy)
{
    if (!sl) {
        clip_mv(r, x, y, w, h, mvx, mvy);
    } else if (!chroma) {
        *mvx = rpr_anchor(x, *mvx, sl->scale_x, 0, w, sl->ref_w, 4, 0);
        *mvy = rpr_anchor(y, *mvy, sl->scale_y, 0, h, sl->ref_h, 4, 1);
    } else {
        *mvx = rpr_anchor(x >> 1, *mvx, sl->scale_x, sl->add_x, w >> 1, sl->ref_w >> 1, 5, 0);
        *mvy = rpr_anchor(y >> 1, *mvy, sl->scale_y, sl->add_y, h >> 1, sl->ref_h >> 1, 5, 1);
    }
}

static void
rpr_side(const ovhip_recorder *r, const ovhip_pu_desc *pu, int l, int scaled, int32_t mvx, int32_t mvy, ovhip_rpr_side *s)
{
    const int pw = 1 << pu->log2_w, ph = 1 << pu->log2_h;
    struct rpr_slot sl;
    memset(s, 0, sizeof(*s));
    s->ref = l ? pu->ref1 : pu->ref0;
    s->pos_x = mvx; s->pos_y = mvy;
    if (!scaled) {
        place_mv(r, NULL, 0, pu->x0, pu->y0, pw, ph, &s->pos_x, &s->pos_y);
        return;
    }
    rpr_slot_fill(r, s->ref, &sl);
    s->step_x = sl.step_x; s->step_y = sl.step_y;
    s->filt = s->filt_c = pu->log2_w == 2 && pu->log2_h == 2 ? sl.filt4 : sl.filt;      /* both from the PU's own 4x4-ness */
    s->cpos_x = mvx; s->cpos_y = mvy;
    place_mv(r, &sl, 0, pu->x0, pu->y0, pw, ph, &s->pos_x, &s->pos_y);
    place_mv(r, &sl, 1, pu->x0, pu->y0, pw, ph, &s->cpos_x, &s->cpos_y);
}

/* A lone 4x4 luma block (rcn_mcp_b_l(2,2)) whose bi-prediction mixes a scaled and an unscaled list: rcn_mcp_bidir0_l runs the 6-tap
 * filters of 4x4 blocks on the unscaled side (put_vvc_qpel_*, rcn_mc.c:457), which k_mc_rpr's regular table is not -- the block
 * becomes a one-sub-block ovhip_aff_rpr_unit without chroma, whose kernel has that path. */
static int
rec_pu4_mixed(ovhip_recorder *r, const ovhip_pu_desc *pu, int s0, int s1)
{
    if (pu->prec_amvr_half || (pu->refine & OVHIP_PU_GPM) || pu->ciip_wt)
        return refuse(r, "reference picture resampling: 4x4 prediction unit with a scaled reference");
    int8_t w0, w1;
    if (bcw_weights(3, pu->bcw_idx_plus1, &w0, &w1)) return OVHIP_EINVAL;
    if (grow((void **)&r->affr, &r->cap_affr, r->n_affr + 1, sizeof(ovhip_aff_rpr_unit))) return OVHIP_ENOMEM;
    if (grow((void **)&r->aff_side, &r->cap_side, r->n_side + 4, sizeof(int32_t))) return OVHIP_ENOMEM;
    ovhip_aff_rpr_unit *u = &r->affr[r->n_affr++];
    memset(u, 0, sizeof(*u));
    u->x = pu->x0; u->y = pu->y0; u->w = u->h = 4; u->dir = 3;
    u->flags = (uint8_t)((s0 ? OVHIP_AFFR_S0 : 0) | (s1 ? OVHIP_AFFR_S1 : 0) | OVHIP_AFFR_NO_CHROMA | (pu->lmcs ? OVHIP_AFFR_LMCS : 0));
    u->w0 = w0; u->w1 = w1;
    u->side_off = (uint32_t)r->n_side;
    int32_t *o = r->aff_side + r->n_side;
    for (int l = 0; l < 2; ++l) {
        ovhip_rpr_side sd;
        rpr_side(r, pu, l, l ? s1 : s0, l ? pu->mv1x : pu->mv0x, l ? pu->mv1y : pu->mv0y, &sd);
        u->s[l].step_x = sd.step_x; u->s[l].step_y = sd.step_y; u->s[l].filt = sd.filt; u->s[l].ref = sd.ref;
        o[2 * l] = sd.pos_x; o[2 * l + 1] = sd.pos_y;
    }
    r->n_side += 4;
    return 1;
}

/* A PU with at least one scaled list used (rcn_mcp_b / _l / _c, rcn_gpm_b and CIIP's rcn_mcp_b into RPR paths,
 * rcn_inter.c:2750-2960, :3118-3143): cut into <=16x16 tiles that share the PU's anchors. */
static int
rec_pu_rpr(ovhip_recorder *r, const ovhip_pu_desc *pu, int dir, int s0, int s1)
{
    const int pw = 1 << pu->log2_w, ph = 1 << pu->log2_h;
    /* a lone 4x4 luma block (rcn_mcp_b_l(2,2): flag_4x4, filter sets 3..5) is what k_mc_rpr takes as it is; opt-in, and never with
     * chroma (no 2x2 chroma block in the reference) */
    if (pw == 4 && ph == 4 && (!(r->rpr_tools & OVHIP_RPR_TOOL_PU4x4) || pu->planes != 1))
        return refuse(r, "reference picture resampling: 4x4 prediction unit with a scaled reference");
    if (pw == 4 && ph == 4 && dir == 3 && s0 != s1) return rec_pu4_mixed(r, pu, s0, s1);
    const int gpm = (pu->refine & OVHIP_PU_GPM) != 0;
    int K = 0, A = 0, B = 0;
    if (gpm) gpm_plane(pu, &K, &A, &B);
    int8_t w0, w1;
    if (bcw_weights(gpm ? 0 : dir, pu->bcw_idx_plus1, &w0, &w1)) return OVHIP_EINVAL;
    ovhip_rpr_side sd[2];
    memset(sd, 0, sizeof(sd));
    if (dir & 1) rpr_side(r, pu, 0, s0, pu->mv0x, pu->mv0y, &sd[0]);
    if (dir & 2) rpr_side(r, pu, 1, s1, pu->mv1x, pu->mv1y, &sd[1]);

    uint8_t flags = (uint8_t)(((dir & 1) && s0 ? OVHIP_RPR_S0 : 0) | ((dir & 2) && s1 ? OVHIP_RPR_S1 : 0));
    if (gpm)                flags |= OVHIP_RPR_GPM;
    if (pu->prec_amvr_half) flags |= OVHIP_RPR_HPEL_FILT;
    if (!(pu->planes & 1))  flags |= OVHIP_RPR_NO_LUMA;
    if (!(pu->planes & 2))  flags |= OVHIP_RPR_NO_CHROMA;
    if (pu->lmcs)           flags |= OVHIP_RPR_LMCS;

    int uw, uh;
    const int nu = tile_extent(pw, ph, &uw, &uh);
    if (grow((void **)&r->rpr, &r->cap_rpr, r->n_rpr + (size_t)nu, sizeof(ovhip_rpr_unit))) return OVHIP_ENOMEM;
    for (int uy = 0; uy < ph; uy += uh) {
        for (int ux = 0; ux < pw; ux += uw) {
            ovhip_rpr_unit *u = &r->rpr[r->n_rpr++];
            memset(u, 0, sizeof(*u));
            u->x = (uint16_t)(pu->x0 + ux); u->y = (uint16_t)(pu->y0 + uy);
            u->w = (uint8_t)uw; u->h = (uint8_t)uh;
            u->ox = (uint8_t)ux; u->oy = (uint8_t)uy;
            u->dir = (uint8_t)dir; u->flags = flags;
            u->w0 = w0; u->w1 = w1;
            u->s[0] = sd[0]; u->s[1] = sd[1];
            u->aux = gpm ? gpm_aux(K, A, B, ux, uy) : ciip_aux(pu);
        }
    }
    return nu;
}

int
ovhip_rec_cu_inter(ovhip_recorder *r, const ovhip_pu_desc *pu, const ovhip_affine_desc *aff)
{
    if (!r || !pu == !aff) return OVHIP_EINVAL;
    return pu ? ovhip_rec_pu(r, pu) : ovhip_rec_affine_cu(r, aff);
}

int
ovhip_rec_pu(ovhip_recorder *r, const ovhip_pu_desc *pu)
{
    const int pw = 1 << pu->log2_w, ph = 1 << pu->log2_h;
    const int gpm = (pu->refine & OVHIP_PU_GPM) != 0;
    const int dir = pu_dir(pu);
    if (r->log) {
        /* (a malformed inter_dir, refused below, is looked up as list 0 here) */
        if ((r->rpr_tools & OVHIP_RPR_TOOL_PU4x4) && pw == 4 && ph == 4 && pu->planes == 1 && !pu->refine &&
            reads_scaled(r, dir ? dir : 1, pu->ref0, pu->ref1))
            ovhip_calllog_rpr_tools_(r->log, r->rpr_tools);
        ovhip_calllog_pu_(r->log, pu);
    }
    if (!dir) return OVHIP_EINVAL;
    if (pu->ciip_wt > 3 || (pu->ciip_wt && pu->refine)) return OVHIP_EINVAL;
    /* rcn_gpm_b always takes rcn_mc_rpr_b_l / _c; DMVR / BDOF read no scale (H.266 disables them under RPR) */
    int g0 = 0, g1 = 0;
    if (r->n_scaled && (gpm || (pu->refine && (pu->inter_dir & 3) == 3))) {
        g0 = slot_scaled(r, pu->ref0);
        g1 = g0 < 0 ? g0 : slot_scaled(r, pu->ref1);
    }
    if (gpm && (pu->gpm_split_dir > 63 || pu->log2_w < 3 || pu->log2_h < 3 || pu->log2_w > 6 || pu->log2_h > 6)) return OVHIP_EINVAL;
    if (g0 < 0 || g1 < 0) return OVHIP_EUNSUP;
    if (g0 || g1) return gpm ? rec_pu_rpr(r, pu, 3, g0, g1) : refuse(r, "reference picture resampling: DMVR / BDOF with a scaled reference");
    if (gpm) return rec_pu_gpm(r, pu);
    if (pu->refine) return rec_pu_refined(r, pu);

    if (r->n_scaled) {
        const int s0 = (dir & 1) ? slot_scaled(r, pu->ref0) : 0, s1 = (dir & 2) && s0 >= 0 ? slot_scaled(r, pu->ref1) : 0;
        if (s0 < 0 || s1 < 0) return OVHIP_EUNSUP;
        if (s0 || s1) return rec_pu_rpr(r, pu, dir, s0, s1);
    }

    int32_t mv0x = pu->mv0x, mv0y = pu->mv0y, mv1x = pu->mv1x, mv1y = pu->mv1y;
    clip_mv(r, pu->x0, pu->y0, pw, ph, &mv0x, &mv0y);
    clip_mv(r, pu->x0, pu->y0, pw, ph, &mv1x, &mv1y);
    /* the list a uni-predicted unit does not use: the caller's fields hold whatever was there (found with AddressSanitizer's malloc
     * fill: the same parse recorded different bytes) -- nothing reads them, but what is uploaded is a function of the stream only */
    uint8_t ref0 = pu->ref0, ref1 = pu->ref1;
    if (!(dir & 1)) { mv0x = mv0y = 0; ref0 = 0; }
    if (!(dir & 2)) { mv1x = mv1y = 0; ref1 = 0; }

    int8_t w0, w1;
    if (bcw_weights(dir, pu->bcw_idx_plus1, &w0, &w1)) return OVHIP_EINVAL;

    uint8_t flags = 0;
    if (pu->prec_amvr_half) flags |= OVHIP_MC_HPEL_FILT;
    if (pw == 4 && ph == 4) flags |= OVHIP_MC_FILT_4x4;
    if (!(pu->planes & 1))  flags |= OVHIP_MC_NO_LUMA;
    if (!(pu->planes & 2))  flags |= OVHIP_MC_NO_CHROMA;
    if (pu->lmcs)           flags |= OVHIP_MC_LMCS;

    int uw, uh;
    const int nu = tile_extent(pw, ph, &uw, &uh);
    if (grow((void **)&r->mc, &r->cap_mc, r->n_mc + (size_t)nu, sizeof(ovhip_mc_unit))) return OVHIP_ENOMEM;
    for (int uy = 0; uy < ph; uy += uh) {
        for (int ux = 0; ux < pw; ux += uw) {
            ovhip_mc_unit *u = &r->mc[r->n_mc++];
            memset(u, 0, sizeof(*u));
            u->x = (uint16_t)(pu->x0 + ux); u->y = (uint16_t)(pu->y0 + uy);
            u->w = (uint8_t)uw; u->h = (uint8_t)uh;
            u->dir = (uint8_t)dir; u->flags = flags;
            u->ref0 = ref0; u->ref1 = ref1;
            u->w0 = w0; u->w1 = w1;
            u->mv0x = mv0x; u->mv0y = mv0y; u->mv1x = mv1x; u->mv1y = mv1y;
            u->aux = ciip_aux(pu);
        }
    }
    return nu;
}

/* ---------------------------------------------------------------- affine CUs
 * rcn_affine_mcp_b_l / rcn_affine_prof_mcp_b_l / rcn_affine_mcp_b_c (drv_affine_mvp.c:3264-3411):
 * every 4x4 luma sub-block is predicted with its own motion vector, every 4x4 chroma block with
 * the average of the top-left and bottom-right sub-block vectors of its 8x8 luma area. */
struct aff_lists {
    int dir;                        /* the lists the CU uses                                                              */
    int placed;                     /* ... and those whose vectors go through place_mv: the regular path clips the zeros
                                     * of an unused list too (they move where the block lies beyond the picture)          */
    const struct rpr_slot *sl[2];   /* a scaled list's slot; NULL: unscaled                                               */
};

/* PROFInfo of the CU into the side arena, for the lists in `mask` */
static int
prof_copy(ovhip_recorder *r, const ovhip_affine_desc *cu, int mask, uint32_t *prof_off)
{
    *prof_off = 0;
    if (!mask) return OVHIP_OK;
    if (grow((void **)&r->aff_side, &r->cap_side, r->n_side + 32, sizeof(int32_t))) return OVHIP_ENOMEM;
    *prof_off = (uint32_t)r->n_side;
    memcpy(r->aff_side + r->n_side, cu->dmv_scale, 128);
    /* h / v tables of a list PROF is not applied to: uninitialised in the caller (compute_prof_dmv_scale runs per refined
     * list, drv_affine_mvp.c:3325-3340); never read on the device, recorded as zeros */
    if (!(mask & 1)) memset(r->aff_side + r->n_side, 0, 64);
    if (!(mask & 2)) memset(r->aff_side + r->n_side + 16, 0, 64);
    r->n_side += 32;
    return OVHIP_OK;
}

static size_t aff_side_words(int uw, int uh) { return 4 * (size_t)((uw >> 2) * (uh >> 2) + (uw >> 3) * (uh >> 3)); }

/* The side arena of the uw x uh unit at (ux, uy) of the CU, (x, y) in the picture: 4 words per 4x4 luma sub-block, then 4 per
 * 4x4 chroma block; identical motion of the two lists per block into ident_l / ident_c.  The caller has reserved
 * aff_side_words(uw, uh).  Always inlined: the regular path's copy, with both lists unscaled, is the branch-free loop it was
 * (measured: 1.2 us per affine CU of a 4K picture inlined, 1.5 us as one shared out-of-line body). */
static inline __attribute__((always_inline)) void
affine_unit_side(ovhip_recorder *r, const ovhip_affine_desc *cu, const struct aff_lists *ls, int ux, int uy, int x, int y,
                 int uw, int uh, uint16_t *ident_l, uint8_t *ident_c)
{
    const int dir = ls->dir, placed = ls->placed, same_poc = dir == 3 && cu->poc0 == cu->poc1;
    const struct rpr_slot *const sl0 = ls->sl[0], *const sl1 = ls->sl[1];
    int32_t *o = r->aff_side + r->n_side;
    for (int sy = 0; sy < uh; sy += 4) {
        for (int sx = 0; sx < uw; sx += 4) {
            const int k = ((uy + sy) >> 2) * cu->mv_stride + ((ux + sx) >> 2);
            int32_t m[4] = { cu->mv0[2 * k], cu->mv0[2 * k + 1], cu->mv1[2 * k], cu->mv1[2 * k + 1] };
            /* the list a uni-predicted CU does not use: whatever the caller's OVMV held (found by the chained stream
             * fixture: stack words of the reference's affine drivers) -- never read on the device, never recorded */
            if (!(dir & 1)) m[0] = m[1] = 0;
            if (!(dir & 2)) m[2] = m[3] = 0;
            /* rcn_mcp_b_l's identical-motion shortcut; rcn_prof_mcp_b_l has none (rcn_inter.c:2864-2918) */
            if (!cu->prof_dir && same_poc && m[0] == m[2] && m[1] == m[3])
                *ident_l |= (uint16_t)(1u << ((sy >> 2) * (uw >> 2) + (sx >> 2)));
            if (placed & 1) place_mv(r, sl0, 0, x + sx, y + sy, 4, 4, &m[0], &m[1]);
            if (placed & 2) place_mv(r, sl1, 0, x + sx, y + sy, 4, 4, &m[2], &m[3]);
            memcpy(o, m, sizeof(m));
            o += 4;
        }
    }
    for (int sy = 0; sy < uh; sy += 8) {
        for (int sx = 0; sx < uw; sx += 8) {
            const int k = ((uy + sy) >> 2) * cu->mv_stride + ((ux + sx) >> 2), k2 = k + cu->mv_stride + 1;
            int32_t m[4] = { 0, 0, 0, 0 };
            if (dir & 1) { m[0] = cu->mv0[2 * k] + cu->mv0[2 * k2]; m[1] = cu->mv0[2 * k + 1] + cu->mv0[2 * k2 + 1]; }
            if (dir & 2) { m[2] = cu->mv1[2 * k] + cu->mv1[2 * k2]; m[3] = cu->mv1[2 * k + 1] + cu->mv1[2 * k2 + 1]; }
            for (int c = 0; c < 4; ++c) { m[c] += m[c] < 0; m[c] >>= 1; }
            if (same_poc && m[0] == m[2] && m[1] == m[3])
                *ident_c |= (uint8_t)(1u << ((sy >> 3) * (uw >> 3) + (sx >> 3)));
            if (placed & 1) place_mv(r, sl0, 1, x + sx, y + sy, 8, 8, &m[0], &m[1]);
            if (placed & 2) place_mv(r, sl1, 1, x + sx, y + sy, 8, 8, &m[2], &m[3]);
            memcpy(o, m, sizeof(m));
            o += 4;
        }
    }
    r->n_side = (size_t)(o - r->aff_side);
}

/* An affine CU with at least one scaled list used (OVHIP_RPR_TOOL_AFFINE).  To the reference every 4x4 luma sub-block is a 4x4 PU
 * (rcn_mcp_b_l(2,2) / rcn_prof_mcp_b_l, rcn_inter.c:2815-2918) and every 4x4 chroma block the chroma of an 8x8 PU (rcn_mcp_b_c(3,3),
 * :2920-2966): each with its OWN anchor after clip_rpr_position, computed from the unclipped vector; the unscaled side of a mixed
 * bi-prediction keeps its clip_mv()'d vector and is the only one PROF refines (rcn_mc_rpr_prof_b_l, :2594-2649; a uni-predicted
 * block on a scaled list goes through plain rcn_mcp_rpr_l).  The filter sets of a scaled list: flag_4x4 for luma, plain for chroma. */
static int
rec_affine_rpr(ovhip_recorder *r, const ovhip_affine_desc *cu, int dir, int s0, int s1)
{
    const int cw = 1 << cu->log2_w, ch = 1 << cu->log2_h;
    const int scaled[2] = { (dir & 1) && s0, (dir & 2) && s1 };
    int8_t w0, w1;
    if (bcw_weights(dir, cu->bcw_idx_plus1, &w0, &w1)) return OVHIP_EINVAL;
    /* apply_prof (rcn_inter.c:2880): bi-prediction only here, and only the lists that are not scaled */
    const int prof = dir == 3 ? (cu->prof_dir & 3 & ((scaled[0] ? 0 : 1) | (scaled[1] ? 0 : 2))) : 0;
    uint32_t prof_off;
    if (prof_copy(r, cu, prof, &prof_off)) return OVHIP_ENOMEM;
    struct rpr_slot slot[2];
    struct aff_lists ls = { dir, dir, { NULL, NULL } };
    ovhip_aff_rpr_list hdr[2];
    memset(hdr, 0, sizeof(hdr));
    for (int l = 0; l < 2; ++l) {
        if (!(dir & (1 << l))) continue;
        hdr[l].ref = l ? cu->ref1 : cu->ref0;
        if (!scaled[l]) continue;
        rpr_slot_fill(r, hdr[l].ref, &slot[l]);
        ls.sl[l] = &slot[l];
        hdr[l].step_x = slot[l].step_x; hdr[l].step_y = slot[l].step_y;
        hdr[l].filt = slot[l].filt4; hdr[l].filt_c = slot[l].filt;
    }

    int uw, uh, n = 0;
    tile_extent(cw, ch, &uw, &uh);
    for (int uy = 0; uy < ch; uy += uh) {
        for (int ux = 0; ux < cw; ux += uw) {
            if (grow((void **)&r->affr, &r->cap_affr, r->n_affr + 1, sizeof(ovhip_aff_rpr_unit))) return OVHIP_ENOMEM;
            if (grow((void **)&r->aff_side, &r->cap_side, r->n_side + aff_side_words(uw, uh), sizeof(int32_t))) return OVHIP_ENOMEM;
            ovhip_aff_rpr_unit *u = &r->affr[r->n_affr++];
            memset(u, 0, sizeof(*u));
            u->x = (uint16_t)(cu->x0 + ux); u->y = (uint16_t)(cu->y0 + uy);
            u->w = (uint8_t)uw; u->h = (uint8_t)uh;
            u->dir = (uint8_t)dir;
            u->flags = (uint8_t)((scaled[0] ? OVHIP_AFFR_S0 : 0) | (scaled[1] ? OVHIP_AFFR_S1 : 0) | (prof ? OVHIP_AFFR_PROF : 0) |
                                 (cu->lmcs ? OVHIP_AFFR_LMCS : 0));
            u->w0 = w0; u->w1 = w1;
            u->prof_dir = (uint8_t)prof;
            u->side_off = (uint32_t)r->n_side;
            u->prof_off = prof_off;
            u->s[0] = hdr[0]; u->s[1] = hdr[1];
            affine_unit_side(r, cu, &ls, ux, uy, u->x, u->y, uw, uh, &u->ident_l, &u->ident_c);
            ++n;
        }
    }
    return n;
}

int
ovhip_rec_affine_cu(ovhip_recorder *r, const ovhip_affine_desc *cu)
{
    const int cw = 1 << cu->log2_w, ch = 1 << cu->log2_h;
    int dir = cu->inter_dir & 3;
    if (!dir || cw < 8 || ch < 8 || !cu->mv0 || !cu->mv1 || cu->mv_stride < (cw >> 2)) return OVHIP_EINVAL;
    if (dir != 3 && (dir & 2)) dir = 2;
    if (r->log) {
        if ((r->rpr_tools & OVHIP_RPR_TOOL_AFFINE) && reads_scaled(r, dir, cu->ref0, cu->ref1)) ovhip_calllog_rpr_tools_(r->log, r->rpr_tools);
        ovhip_calllog_affine_(r->log, cu);
    }
    if (r->n_scaled) {
        const int s0 = (dir & 1) ? slot_scaled(r, cu->ref0) : 0, s1 = (dir & 2) && s0 >= 0 ? slot_scaled(r, cu->ref1) : 0;
        if (s0 < 0 || s1 < 0) return OVHIP_EUNSUP;
        if (s0 || s1) {
            if (!(r->rpr_tools & OVHIP_RPR_TOOL_AFFINE))
                return refuse(r, "reference picture resampling: affine coding unit with a scaled reference");
            return rec_affine_rpr(r, cu, dir, s0, s1);
        }
    }

    int8_t w0, w1;
    if (bcw_weights(dir, cu->bcw_idx_plus1, &w0, &w1)) return OVHIP_EINVAL;
    uint32_t prof_off;
    if (prof_copy(r, cu, cu->prof_dir, &prof_off)) return OVHIP_ENOMEM;
    const struct aff_lists ls = { dir, 3, { NULL, NULL } };

    int uw, uh, n = 0;
    tile_extent(cw, ch, &uw, &uh);
    for (int uy = 0; uy < ch; uy += uh) {
        for (int ux = 0; ux < cw; ux += uw) {
            if (grow((void **)&r->aff, &r->cap_aff, r->n_aff + 1, sizeof(ovhip_aff_unit))) return OVHIP_ENOMEM;
            if (grow((void **)&r->aff_side, &r->cap_side, r->n_side + aff_side_words(uw, uh), sizeof(int32_t))) return OVHIP_ENOMEM;
            ovhip_aff_unit *u = &r->aff[r->n_aff++];
            memset(u, 0, sizeof(*u));
            u->x = (uint16_t)(cu->x0 + ux); u->y = (uint16_t)(cu->y0 + uy);
            u->w = (uint8_t)uw; u->h = (uint8_t)uh;
            u->dir = (uint8_t)dir;
            u->flags = (uint8_t)((cu->prof_dir ? OVHIP_AFF_PROF : 0) | (cu->lmcs ? OVHIP_AFF_LMCS : 0));
            u->ref0 = cu->ref0; u->ref1 = cu->ref1;
            u->w0 = w0; u->w1 = w1;
            u->prof_dir = cu->prof_dir;
            u->side_off = (uint32_t)r->n_side;
            u->prof_off = prof_off;
            affine_unit_side(r, cu, &ls, ux, uy, u->x, u->y, uw, uh, &u->ident_l, &u->ident_c);
            ++n;
        }
    }
    return n;
}
