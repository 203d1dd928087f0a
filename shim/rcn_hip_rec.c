/* rcn_hip_rec.c -- the slots of the override block that only record (rcn_hip.h, rcn_hip_priv.h): each turns one call of the decoder
 * into one call of the recorder, snapshotting the OVCTUDec fields its scalar counterpart reads implicitly and
 * doing that counterpart's host-side bookkeeping for the rest of the decoder (deblocking edge / bS maps, progress bit-fields).  Also the
 * SAO / ALF / LMCS parameter capture, and the two row hooks, which say to rcn_hip_pic.c how far the parse has come. */
#include "rcn_hip_priv.h"

/* struct TUInfo is private to the reference's .c files (rcn_transform_tree.c:51-66 and vcl_transform_unit.c:47-75): the slot
 * prototypes only forward-declare it, a back-end has to restate the layout. */
struct TBInfo { uint16_t last_pos; uint64_t sig_sb_map; };
struct TUInfo {
    uint8_t is_sbt; uint8_t cbf_mask; uint16_t pos_offset; uint8_t tr_skip_mask;
    uint8_t cu_mts_flag; uint8_t cu_mts_idx; uint8_t lfnst_flag; uint8_t lfnst_idx;
    struct TBInfo tb_info[3];
};
struct ISPTUInfo { uint8_t cbf_mask, tr_skip_mask, cu_mts_flag, cu_mts_idx, lfnst_flag, lfnst_idx; struct TBInfo tb_info[4]; };   /* rcn_transform_tree.c:68-76 */
extern uint64_t residual_coding_dpq(OVCTUDec *const, int16_t *const, uint8_t, uint8_t, uint16_t);
extern int transform_unit_st(OVCTUDec *const, unsigned int, unsigned int, unsigned int, unsigned int, uint8_t, CUFlags, uint8_t, struct TUInfo *const);
extern int transform_unit_l(OVCTUDec *const, unsigned int, unsigned int, unsigned int, unsigned int, uint8_t, CUFlags, uint8_t, struct TUInfo *const);
extern int transform_unit_c(OVCTUDec *const, unsigned int, unsigned int, unsigned int, unsigned int, uint8_t, CUFlags, uint8_t, struct TUInfo *const);

#ifndef LOG2_MIN_CU_S
#define LOG2_MIN_CU_S 2                             /* rcn_transform_tree.c:45 */
#endif

static inline OVCTUDec *ctudec_of_lmcs(struct LMCSInfo *li) { return (OVCTUDec *)((char *)li - offsetof(OVCTUDec, lmcs_info)); }

/* ------------------------------------------------------------------------------------ descriptors */
static int
ref_slot(struct hip_entry *e, const OVPicture *p)
{
    for (int i = 0; i < e->n_refs; ++i) if (e->refs[i] == p) return i;
    if (e->n_refs >= 16) { latch(e, OVHIP_EUNSUP, "more than 16 distinct reference pictures"); return 0; }
    e->refs[e->n_refs] = p;
    /* the frame thread keeps the same table (order of first use), keyed by the OVFrame: the device DPB hands the picture over */
    if (e->fr && !e->record_only) {
        const int k = ovhip_frame_ref_tag(e->fr, p->frame, pic_tag(p));
        if (k != e->n_refs) latch(e, k < 0 ? k : OVHIP_EINVAL, "ovhip_frame_ref");
    }
    return e->n_refs++;
}

/* ref_slot, plus the slot's scale for reference picture resampling: scale_fact_rpl{list}[ref_idx] (ctudec_compute_refs_scaling,
 * ctudec.c:43-86), the reference's size and its chroma collocation flags -- read from rpl0[ref_idx] whatever the list, as
 * rcn_mcp_rpr_c does (rcn_inter.c:2322-2323; the flags are SPS-level).  Unscaled slots of the picture's size keep the recorder's
 * default; the recorder emits RPR units for the others or refuses what the device path does not take. */
static int
ref_slot_scaled(struct hip_entry *e, const OVCTUDec *c, const OVPicture *p, int list, int ref_idx)
{
    const int k = ref_slot(e, p);
    const struct InterDRVCtx *ic = &c->drv_ctx.inter_ctx;
    const uint16_t *sf = list ? ic->scale_fact_rpl1[ref_idx & 15] : ic->scale_fact_rpl0[ref_idx & 15];
    const OVFrame *f = p->frame;
    if (k < 0 || k >= 32 || ((e->scale_set >> k) & 1) || !f) return k;
    if (sf[0] != (1 << RPR_SCALE_BITS) || sf[1] != (1 << RPR_SCALE_BITS) || (int)f->width != e->pic_w || (int)f->height != e->pic_h) {
        const OVPicture *q = ic->rpl0[ref_idx & 15] ? ic->rpl0[ref_idx & 15] : p;
        ovhip_ref_scale s;
        memset(&s, 0, sizeof(s));
        s.scale_hor = sf[0]; s.scale_ver = sf[1];
        s.ref_w = (int32_t)f->width; s.ref_h = (int32_t)f->height;
        s.chroma_hor_col_flag = q->scale_info.chroma_hor_col_flag; s.chroma_ver_col_flag = q->scale_info.chroma_ver_col_flag;
        latch(e, ovhip_rec_set_ref_scale(e->rec, k, &s), "ovhip_rec_set_ref_scale");
    }
    e->scale_set |= 1u << k;
    return k;
}

static void
fill_pu_lists(struct hip_entry *e, const OVCTUDec *c, ovhip_pu_desc *d, int x0, int y0, int log2_w, int log2_h, int inter_dir,
              OVMV mv0, OVMV mv1, const OVPicture *p0, const OVPicture *p1, int list0, int list1)
{
    const struct InterDRVCtx *ic = &c->drv_ctx.inter_ctx;
    const int l2 = c->part_ctx->log2_ctu_s;
    memset(d, 0, sizeof(*d));
    d->x0 = (uint16_t)((c->ctb_x << l2) + x0); d->y0 = (uint16_t)((c->ctb_y << l2) + y0);
    d->log2_w = (uint8_t)log2_w; d->log2_h = (uint8_t)log2_h;
    d->inter_dir = (uint8_t)inter_dir;
    d->ref_idx0 = (uint8_t)mv0.ref_idx; d->ref_idx1 = (uint8_t)mv1.ref_idx;
    d->bcw_idx_plus1 = mv0.bcw_idx_plus1;
    d->prec_amvr_half = ic->prec_amvr == MV_PRECISION_HALF;
    d->planes = 3;
    d->lmcs = c->lmcs_info.lmcs_enabled_flag;
    d->mv0x = mv0.x; d->mv0y = mv0.y; d->mv1x = mv1.x; d->mv1y = mv1.y;
    /* reference picture resampling (rcn_mcp_rpr_*, rcn_inter.c:2769-2800): the slot's scale goes to the recorder with the slot */
    if (p0 && (inter_dir & 1)) { d->poc0 = p0->poc; d->ref0 = (uint8_t)ref_slot_scaled(e, c, p0, list0, mv0.ref_idx); }
    if (p1 && (inter_dir & 2)) { d->poc1 = p1->poc; d->ref1 = (uint8_t)ref_slot_scaled(e, c, p1, list1, mv1.ref_idx); }
    if (inter_dir == 1) { d->ref1 = d->ref0; d->poc1 = d->poc0 + 1; }      /* keep the identical-motion test off */
    if (inter_dir == 2) { d->ref0 = d->ref1; d->poc0 = d->poc1 + 1; }
}

void
fill_pu(struct hip_entry *e, const OVCTUDec *c, ovhip_pu_desc *d, int x0, int y0, int log2_w, int log2_h, int inter_dir,
        OVMV mv0, OVMV mv1, const OVPicture *p0, const OVPicture *p1)
{
    fill_pu_lists(e, c, d, x0, y0, log2_w, log2_h, inter_dir, mv0, mv1, p0, p1, 0, 1);
}

/* the slots that get a vector's reference index beside it: list 0's picture for mv0, list 1's for mv1 */
void
fill_pu_idx(struct hip_entry *e, const OVCTUDec *c, ovhip_pu_desc *d, int x0, int y0, int log2_w, int log2_h, int inter_dir,
            OVMV mv0, OVMV mv1, int ref_idx0, int ref_idx1)
{
    const struct InterDRVCtx *ic = &c->drv_ctx.inter_ctx;
    mv0.ref_idx = (int8_t)ref_idx0; mv1.ref_idx = (int8_t)ref_idx1;
    fill_pu(e, c, d, x0, y0, log2_w, log2_h, inter_dir, mv0, mv1, ic->rpl0[ref_idx0], ic->rpl1[ref_idx1]);
}

/* An affine CU (x0, y0 CTU-local) whose 4x4 sub-block vectors lie in e->pend.mv0 / mv1, 32 per row.  A list the CU does not use takes
 * the other's slot and a picture order count that differs (keeps the identical-motion test off).  prof: NULL = no PROF tables. */
void
fill_affine(struct hip_entry *e, const OVCTUDec *c, ovhip_affine_desc *d, int x0, int y0, int log2_w, int log2_h, int inter_dir,
            int bcw_idx_plus1, int prof_dir, int ref_idx0, int ref_idx1, const struct PROFInfo *prof)
{
    const struct InterDRVCtx *ic = &c->drv_ctx.inter_ctx;
    const int l2 = c->part_ctx->log2_ctu_s;
    memset(d, 0, sizeof(*d));
    d->x0 = (uint16_t)((c->ctb_x << l2) + x0); d->y0 = (uint16_t)((c->ctb_y << l2) + y0);
    d->log2_w = (uint8_t)log2_w; d->log2_h = (uint8_t)log2_h;
    d->inter_dir = (uint8_t)inter_dir; d->bcw_idx_plus1 = (uint8_t)bcw_idx_plus1; d->prof_dir = (uint8_t)prof_dir;
    d->lmcs = c->lmcs_info.lmcs_enabled_flag;
    const OVPicture *p0 = (inter_dir & 1) ? ic->rpl0[ref_idx0] : NULL, *p1 = (inter_dir & 2) ? ic->rpl1[ref_idx1] : NULL;
    if (p0) { d->ref0 = (uint8_t)ref_slot_scaled(e, c, p0, 0, ref_idx0); d->poc0 = p0->poc; }
    if (p1) { d->ref1 = (uint8_t)ref_slot_scaled(e, c, p1, 1, ref_idx1); d->poc1 = p1->poc; }
    if (!p0) { d->ref0 = d->ref1; d->poc0 = d->poc1 + 1; }
    if (!p1) { d->ref1 = d->ref0; d->poc1 = d->poc0 + 1; }
    d->mv_stride = 32; d->mv0 = e->pend.mv0; d->mv1 = e->pend.mv1;
    if (prof) {
        memcpy(d->dmv_scale[0], prof->dmv_scale_h_0, 32); memcpy(d->dmv_scale[1], prof->dmv_scale_v_0, 32);
        memcpy(d->dmv_scale[2], prof->dmv_scale_h_1, 32); memcpy(d->dmv_scale[3], prof->dmv_scale_v_1, 32);
    }
}
/* ------------------------------------------------------------------------------------ transform units */
static void
fill_tu_state(const struct hip_entry *e, const OVCTUDec *c, ovhip_tu_state *st)
{
    memset(st, 0, sizeof(*st));
    st->qp_y = c->dequant_luma.qp; st->qp_cb = c->dequant_cb.qp; st->qp_cr = c->dequant_cr.qp;
    st->qp_jcbcr = c->dequant_joint_cb_cr.qp;
    st->qp_y_skip = c->dequant_luma_skip.qp; st->qp_cb_skip = c->dequant_cb_skip.qp;
    st->qp_cr_skip = c->dequant_cr_skip.qp; st->qp_jcbcr_skip = c->dequant_jcbcr_skip.qp;
    st->dep_quant = c->residual_coding_l == &residual_coding_dpq;          /* rcn_transform_tree.c:399 */
    st->mts_implicit = c->mts_implicit;
    st->sh_ts_disabled = c->sh_ts_disabled;
    st->ict_type = e->ict_type;
    /* scale derived on the device from the region the last rcn_lmcs_compute_chroma_scale call recorded */
    st->lmcs_scale_c = c->lmcs_info.scale_c_flag ? (e->lmcs_region_live ? 2 : 1) : 0;
    st->lmcs_chroma_scale = (int16_t)c->lmcs_info.lmcs_chroma_scale;
    st->intra_mode = (int8_t)c->intra_mode;
}

/* derive_lfnst_mode_c (drv_lfnst.c:94-121): DM / LM chroma modes take the co-located luma mode; then the wide-angle
 * remap of the CHROMA block shape */
static int8_t
lfnst_mode_c(const OVCTUDec *c, int log2_w, int log2_h, int x0, int y0)
{
    static const uint8_t shift_lut[6] = { 0, 6, 10, 12, 14, 15 };
    const int l2 = c->part_ctx_c->log2_min_cb_s;
    const int xu = x0 >> l2, yu = y0 >> l2, nw = (1 << log2_w) >> l2, nh = (1 << log2_h) >> l2;
    int m = c->intra_mode_c;
    if (m == OVINTRA_DM_CHROMA || (m >= OVINTRA_LM_CHROMA && m <= OVINTRA_MDLM_TOP))
        m = c->drv_ctx.intra_info.luma_modes[xu + ((yu + (nh >> 1)) << 5) + (nw >> 1)];
    if (m > OVINTRA_DC) {
        const int d = log2_w - log2_h, ms = shift_lut[d < 0 ? -d : d];
        if (log2_w > log2_h && m < 2 + ms) m += OVINTRA_VDIA - 1;
        else if (log2_h > log2_w && m > OVINTRA_VDIA - ms) m -= OVINTRA_VDIA + 1;
    }
    return (int8_t)(m < 0 ? m + 14 + 67 : m >= 67 ? m + 14 : m);
}


/* ------------------------------------------------------------------------------------ ordered (intra) tasks */
/* Availability of the two reference arms as the reference's fill_ref_* read it out of the progress bit-fields
 * (rcn_fill_ref.h:41-64; rcn_fill_ref.c:71-100, :166-190, :228-260): bit 0 of the shifted map = the corner unit, the
 * highest set bit = how far the arm is read. */
static inline int top_bit(uint64_t m) { return m ? 64 - __builtin_clzll(m) : 0; }

static void
task_avl(const struct CTUBitField *pf, int x0, int y0, int log2_w, int log2_h, int log2_unit, ovhip_itask *t)
{
    const int nb_a = ((1 << (log2_w + 1)) >> log2_unit) + 1, nb_l = ((1 << (log2_h + 1)) >> log2_unit) + 1;
    const uint64_t ma = (pf->hfield[y0 >> log2_unit] >> (x0 >> log2_unit)) & ((1llu << (nb_a + 1)) - 1);
    const uint64_t ml = (pf->vfield[x0 >> log2_unit] >> (y0 >> log2_unit)) & ((1llu << (nb_l + 1)) - 1);
    t->avl_abv = (uint8_t)top_bit(ma >> 1); t->avl_lft = (uint8_t)top_bit(ml >> 1);
    if ((ma | ml) & 1) t->flags |= OVHIP_IF_CORNER;
}

static void
luma_task(const OVCTUDec *c, int x0, int y0, int log2_w, int log2_h, CUFlags cu_flags, int mode, int ciip_wt, ovhip_itask *t)
{
    const int l2 = c->part_ctx->log2_ctu_s;
    memset(t, 0, sizeof(*t));
    t->kind = OVHIP_IT_LUMA;
    t->x = (uint16_t)((c->ctb_x << l2) + x0); t->y = (uint16_t)((c->ctb_y << l2) + y0);
    t->log2_w = (uint8_t)log2_w; t->log2_h = (uint8_t)log2_h;
    t->mode = (uint8_t)mode; t->ciip_wt = (uint8_t)ciip_wt;
    if (cu_flags & flg_mip_flag) {                                   /* rcn_intra_mip.c:388-402 */
        t->flags |= OVHIP_IF_MIP | ((c->cu_opaque >> 7) & 1 ? OVHIP_IF_MIP_TR : 0);
        t->mode = c->cu_opaque & 0x3f;
    } else if (cu_flags & flg_intra_bdpcm_luma_flag) {
        t->flags |= OVHIP_IF_BDPCM | ((cu_flags & flg_intra_bdpcm_luma_dir) ? OVHIP_IF_BDPCM_VER : 0);
        t->mode = 0;
    } else if (cu_flags & flg_mrl_flag) {
        t->mrl_idx = c->cu_opaque;
    }
    task_avl(&c->rcn_ctx.progress_field, x0, y0, log2_w, log2_h, 2, t);
}

/* x0, y0, size in CHROMA samples */
static void
chroma_task(const OVCTUDec *c, int x0, int y0, int log2_w, int log2_h, CUFlags cu_flags, int mode, int ciip_wt, ovhip_itask *t)
{
    const int l2 = c->part_ctx->log2_ctu_s - 1;
    const struct CTUBitField *pf = &c->rcn_ctx.progress_field_c;
    memset(t, 0, sizeof(*t));
    t->kind = OVHIP_IT_CHROMA;
    t->x = (uint16_t)((c->ctb_x << l2) + x0); t->y = (uint16_t)((c->ctb_y << l2) + y0);
    t->log2_w = (uint8_t)log2_w; t->log2_h = (uint8_t)log2_h;
    t->mode = (uint8_t)mode; t->ciip_wt = (uint8_t)ciip_wt;
    if (cu_flags & flg_intra_bdpcm_chroma_flag) {
        t->flags |= OVHIP_IF_BDPCM | ((cu_flags & flg_intra_bdpcm_chroma_dir) ? OVHIP_IF_BDPCM_VER : 0);
        t->mode = 0;
    }
    if (!(t->flags & OVHIP_IF_BDPCM) && mode >= OVINTRA_LM_CHROMA && mode <= OVINTRA_MDLM_TOP) {
        /* the linear-model modes read their own availability (rcn_intra_cclm.c:56-68, :770-776, :843-849) */
        const int w = 1 << log2_w, h = 1 << log2_h, ext = w < h ? w : h;
        const uint64_t abv = pf->hfield[y0 >> 1] >> ((x0 >> 1) + 1), lft = pf->vfield[x0 >> 1] >> ((y0 >> 1) + 1);
        const int any_abv = !!(abv & ((1llu << (w >> 1)) - 1)), any_lft = !!(lft & ((1llu << (h >> 1)) - 1));
        t->mode = (uint8_t)(67 + (mode - OVINTRA_LM_CHROMA));
        t->avl_abv = (uint8_t)any_abv; t->avl_lft = (uint8_t)any_lft;
        if (mode == OVINTRA_MDLM_TOP && any_abv) t->avl_abv = (uint8_t)__builtin_ctzll(~(abv & ((1llu << ((w + ext) >> 1)) - 1)));
        if (mode == OVINTRA_MDLM_LEFT && any_lft) t->avl_lft = (uint8_t)__builtin_ctzll(~(lft & ((1llu << ((h + ext) >> 1)) - 1)));
        return;
    }
    task_avl(pf, x0, y0, log2_w, log2_h, 1, t);
}

static void
record_tu(struct hip_entry *e, OVCTUDec *c, int tree, int x0, int y0, int log2_w, int log2_h, CUFlags cu_flags, uint8_t cbf_mask,
          const struct TUInfo *tu, const ovhip_itask *task_l, const ovhip_itask *task_c)
{
    const int l2 = c->part_ctx->log2_ctu_s;
    ovhip_tu_state st;
    ovhip_tu_desc d;
    fill_tu_state(e, c, &st);
    memset(&d, 0, sizeof(d));
    /* tree 2 (rcn_tu_c): x0, y0 and the size are in chroma samples; the picture offset likewise */
    d.x0 = (uint16_t)(((c->ctb_x << l2) >> (tree == 2)) + x0); d.y0 = (uint16_t)(((c->ctb_y << l2) >> (tree == 2)) + y0);
    d.log2_tb_w = (uint8_t)log2_w; d.log2_tb_h = (uint8_t)log2_h; d.tree = (uint8_t)tree;
    d.cbf_mask = cbf_mask; d.cu_flags = (uint16_t)cu_flags;
    d.tr_skip_mask = tu->tr_skip_mask; d.cu_mts_flag = tu->cu_mts_flag; d.cu_mts_idx = tu->cu_mts_idx;
    d.lfnst_flag = tu->lfnst_flag; d.lfnst_idx = tu->lfnst_idx;
    for (int k = 0; k < 3; ++k) { d.last_pos[k] = tu->tb_info[k].last_pos; d.sig_sb_map[k] = tu->tb_info[k].sig_sb_map; }
    d.coef[0] = c->residual_cb + tu->pos_offset; d.coef[1] = c->residual_cr + tu->pos_offset; d.coef[2] = c->residual_y + tu->pos_offset;
    if (tree == 2 && tu->lfnst_flag) st.lfnst_mode_c = lfnst_mode_c(c, log2_w, log2_h, x0, y0);
    latch(e, ovhip_rec_tu_intra(e->rec, &st, &d, task_l, task_c), "ovhip_rec_tu_intra");
}

/* rcn_jcbcr (rcn_transform_tree.c:840-847): a joint Cb-Cr block with both cbf bits set is deblocked with the JOINT chroma QP --
 * the scalar orchestrator overwrites the two chroma QP maps the caller filled (vcl_transform_unit.c:1110-1112) for the block's area
 * (x0, y0, size in LUMA samples).  Found by the chained stream fixture (tests/golden/pipe_b.ovg: pps_cb_qp_offset != pps_cr_qp_offset). */
static void
jcbcr_qp_maps(OVCTUDec *c, int x0, int y0, int log2_w, int log2_h, uint8_t cbf_mask)
{
    if ((cbf_mask & 0x8) && (cbf_mask & 0x3) == 0x3) {
        const uint8_t qp = (uint8_t)(c->dequant_joint_cb_cr.qp - c->qp_ctx.qp_bd_offset);
        dbf_fill_qp_map(&c->dbf_info.qp_map_cb, x0, y0, log2_w, log2_h, qp);
        dbf_fill_qp_map(&c->dbf_info.qp_map_cr, x0, y0, log2_w, log2_h, qp);
    }
}

static void tu_st_books(OVCTUDec *c, int x0, int y0, int log2_tb_w, int log2_tb_h, CUFlags cu_flags, uint8_t cbf_mask);

/* rcn_tu_st (rcn_transform_tree.c:1228-1301) with the luma task rcn_intra_tu made before it (or a CIIP CU's two tasks) */
static void
tu_st_common(struct hip_entry *e, OVCTUDec *c, int x0, int y0, int log2_tb_w, int log2_tb_h, CUFlags cu_flags, uint8_t cbf_mask,
             const struct TUInfo *const tu, const ovhip_itask *task_l, const ovhip_itask *task_c)
{
    ovhip_itask tc;
    if (cu_flags & flg_pred_mode_flag) {
        /* :1270-1287: the chroma prediction of an intra CU sits between the TU's luma and chroma residuals */
        ctu_field_set_rect_bitfield(&c->rcn_ctx.progress_field_c, x0 >> LOG2_MIN_CU_S, y0 >> LOG2_MIN_CU_S,
                                    (1 << log2_tb_w) >> LOG2_MIN_CU_S, (1 << log2_tb_h) >> LOG2_MIN_CU_S);
        if (!(cu_flags & flg_intra_bdpcm_chroma_flag)) fill_bs_map(&c->dbf_info.bs2_map_c, x0, y0, log2_tb_w, log2_tb_h);
        chroma_task(c, x0 >> 1, y0 >> 1, log2_tb_w - 1, log2_tb_h - 1, cu_flags, c->intra_mode_c, 0, &tc);
        task_c = &tc;
    }
    record_tu(e, c, 0, x0, y0, log2_tb_w, log2_tb_h, cu_flags, cbf_mask, tu, task_l, task_c);
    tu_st_books(c, x0, y0, log2_tb_w, log2_tb_h, cu_flags, cbf_mask);
}

/* what the scalar orchestrator's rcn_tu_st leaves behind for deblocking (:1262-1267, :1299-1300; rcn_res_c / rcn_jcbcr
 * :757-759, :793-795, :860-866) */
static void
tu_st_books(OVCTUDec *c, int x0, int y0, int log2_tb_w, int log2_tb_h, CUFlags cu_flags, uint8_t cbf_mask)
{
    if (cbf_mask & 0x10) {
        fill_bs_map(&c->dbf_info.bs1_map, x0, y0, log2_tb_w, log2_tb_h);
        if ((cu_flags & flg_pred_mode_flag) && !(cu_flags & flg_intra_bdpcm_luma_flag)) fill_bs_map(&c->dbf_info.bs2_map, x0, y0, log2_tb_w, log2_tb_h);
    }
    if (!(cu_flags & flg_intra_bdpcm_chroma_flag)) {
        if (cbf_mask & 0x8) {
            fill_bs_map(&c->dbf_info.bs1_map_cb, x0, y0, log2_tb_w, log2_tb_h);
            fill_bs_map(&c->dbf_info.bs1_map_cr, x0, y0, log2_tb_w, log2_tb_h);
        } else {
            if (cbf_mask & 0x2) fill_bs_map(&c->dbf_info.bs1_map_cb, x0, y0, log2_tb_w, log2_tb_h);
            if (cbf_mask & 0x1) fill_bs_map(&c->dbf_info.bs1_map_cr, x0, y0, log2_tb_w, log2_tb_h);
        }
    }
    fill_ctb_bound(&c->dbf_info, x0, y0, log2_tb_w, log2_tb_h);
    fill_ctb_bound_c(&c->dbf_info, x0, y0, log2_tb_w, log2_tb_h);
    jcbcr_qp_maps(c, x0, y0, log2_tb_w, log2_tb_h, cbf_mask);
}

/* tmp.rcn_tu_st (rcn_structures.h:481-486): called through the table by the SBT paths (vcl_transform_unit.c:1113-1299) */
static void
hip_rcn_tu_st(OVCTUDec *const c, uint8_t x0, uint8_t y0, uint8_t log2_tb_w, uint8_t log2_tb_h, CUFlags cu_flags, uint8_t cbf_mask,
              const struct TUInfo *const tu)
{
    ENTER(c);
    tu_st_common(e, c, x0, y0, log2_tb_w, log2_tb_h, cu_flags, cbf_mask, tu, NULL, NULL);
}

/* tmp.rcn_tu_c (rcn_structures.h:475-479; rcn_transform_tree.c:1349-1382): dual-tree chroma and the chroma of an ISP CU,
 * always intra (x0, y0, size in chroma samples) */
static void
hip_rcn_tu_c(OVCTUDec *const c, uint8_t x0, uint8_t y0, uint8_t log2_tb_w, uint8_t log2_tb_h, CUFlags cu_flags, uint8_t cbf_mask,
             const struct TUInfo *const tu)
{
    ENTER(c);
    ovhip_itask tc;
    ctu_field_set_rect_bitfield(&c->rcn_ctx.progress_field_c, (x0 << 1) >> LOG2_MIN_CU_S, (y0 << 1) >> LOG2_MIN_CU_S,
                                (2 << log2_tb_w) >> LOG2_MIN_CU_S, (2 << log2_tb_h) >> LOG2_MIN_CU_S);
    chroma_task(c, x0, y0, log2_tb_w, log2_tb_h, cu_flags, c->intra_mode_c, 0, &tc);
    fill_ctb_bound_c(&c->dbf_info, x0 << 1, y0 << 1, log2_tb_w + 1, log2_tb_h + 1);
    if (!(cu_flags & flg_intra_bdpcm_chroma_flag)) fill_bs_map(&c->dbf_info.bs2_map_c, x0 << 1, y0 << 1, log2_tb_w + 1, log2_tb_h + 1);
    record_tu(e, c, 2, x0, y0, log2_tb_w, log2_tb_h, cu_flags, cbf_mask, tu, NULL, &tc);
    if (!(cu_flags & flg_intra_bdpcm_chroma_flag)) {
        if (cbf_mask & 0x8) {
            fill_bs_map(&c->dbf_info.bs1_map_cb, x0 << 1, y0 << 1, log2_tb_w + 1, log2_tb_h + 1);
            fill_bs_map(&c->dbf_info.bs1_map_cr, x0 << 1, y0 << 1, log2_tb_w + 1, log2_tb_h + 1);
        } else {
            if (cbf_mask & 0x2) fill_bs_map(&c->dbf_info.bs1_map_cb, x0 << 1, y0 << 1, log2_tb_w + 1, log2_tb_h + 1);
            if (cbf_mask & 0x1) fill_bs_map(&c->dbf_info.bs1_map_cr, x0 << 1, y0 << 1, log2_tb_w + 1, log2_tb_h + 1);
        }
    }
    jcbcr_qp_maps(c, x0 << 1, y0 << 1, log2_tb_w + 1, log2_tb_h + 1, cbf_mask);
}

/* rcn_ibc_l / rcn_ibc_c (rcn_structures.h; rcn_ibc.c:8-139; callers vcl_coding_unit.c:1032-1066, :1088-1133, :1155-1205, :1257-1311):
 * the slots only stash the CU.  Its blocks are recorded by the leaves of the transform tree that follows, one ordered task per block
 * with the block's residual (ovhip_rec_tu_ibc): a prediction task of the whole CU followed by residual tasks would give a 4x4 unit
 * two ordered writers.  Neither slot keeps any of the decoder's books in the reference (progress fields: the caller,
 * vcl_coding_unit.c:953-991; bS / QP maps: the transform unit, restated by tu_st_common). */
void
ibc_orphan(struct hip_entry *e)
{
    e->ibc.live = 0;
    latch(e, OVHIP_EINVAL, "an intra block copy (IBC) coding unit was not followed by its transform tree");
}

static void
hip_rcn_ibc_l(OVCTUDec *const c, int16_t x0, int16_t y0, uint8_t log2_cu_w, uint8_t log2_cu_h, uint8_t log2_ctu_s, IBCMV mv)
{
    ENTER(c);
    ovhip_ibc_desc *d = &e->ibc.cu;
    memset(d, 0, sizeof(*d));
    d->x0 = (uint16_t)((c->ctb_x << log2_ctu_s) + x0); d->y0 = (uint16_t)((c->ctb_y << log2_ctu_s) + y0);
    d->log2_w = log2_cu_w; d->log2_h = log2_cu_h; d->log2_ctu = log2_ctu_s;
    d->mv_x = (int16_t)mv.x; d->mv_y = (int16_t)mv.y; d->win_x0 = (uint16_t)e->entry_x0;
    e->ibc.x0 = x0; e->ibc.y0 = y0; e->ibc.live = 1;
    /* refused vectors fail the picture here, with the recorder's reason */
    if (ovhip_rec_ibc_check(e->rec, d)) { e->ibc.live = 0; latch(e, OVHIP_EUNSUP, ovhip_rec_refusal(e->rec)); }
}

static void
hip_rcn_ibc_c(OVCTUDec *const c, int16_t x0, int16_t y0, uint8_t log2_cu_w, uint8_t log2_cu_h, uint8_t log2_ctu_s, IBCMV mv)
{
    struct hip_entry *e = entry_of(c, 0);
    if (!e || !e->rec) return;
    PROF(e);
    (void)log2_ctu_s;
    if (e->err) return;
    if (!e->ibc.live || e->ibc.x0 != x0 || e->ibc.y0 != y0 || e->ibc.cu.log2_w != log2_cu_w || e->ibc.cu.log2_h != log2_cu_h ||
        e->ibc.cu.mv_x != mv.x || e->ibc.cu.mv_y != mv.y) {
        e->ibc.live = 0;
        latch(e, OVHIP_EINVAL, "rcn_ibc_c without the rcn_ibc_l call of the same coding unit before it");
        return;
    }
    e->ibc.cu.has_chroma = 1;
}

/* a leaf of the stashed IBC CU's transform tree: the block's copy and its residual as one call (tree 0: rcn_tu_st, 1: rcn_tu_l) */
static void
record_tu_ibc(struct hip_entry *e, OVCTUDec *c, int tree, int x0, int y0, int log2_w, int log2_h, CUFlags cu_flags, uint8_t cbf_mask, const struct TUInfo *tu)
{
    const int l2 = c->part_ctx->log2_ctu_s;
    ovhip_tu_state st;
    ovhip_tu_desc d;
    fill_tu_state(e, c, &st);
    memset(&d, 0, sizeof(d));
    d.x0 = (uint16_t)((c->ctb_x << l2) + x0); d.y0 = (uint16_t)((c->ctb_y << l2) + y0);
    d.log2_tb_w = (uint8_t)log2_w; d.log2_tb_h = (uint8_t)log2_h; d.tree = (uint8_t)tree;
    d.cbf_mask = cbf_mask; d.cu_flags = (uint16_t)cu_flags;
    d.tr_skip_mask = tu->tr_skip_mask; d.cu_mts_flag = tu->cu_mts_flag; d.cu_mts_idx = tu->cu_mts_idx;
    for (int k = 0; k < 3; ++k) { d.last_pos[k] = tu->tb_info[k].last_pos; d.sig_sb_map[k] = tu->tb_info[k].sig_sb_map; }
    d.coef[0] = c->residual_cb + tu->pos_offset; d.coef[1] = c->residual_cr + tu->pos_offset; d.coef[2] = c->residual_y + tu->pos_offset;
    const int r = ovhip_rec_tu_ibc(e->rec, &st, &d, &e->ibc.cu);
    latch(e, r, r == OVHIP_EUNSUP ? ovhip_rec_refusal(e->rec) : "ovhip_rec_tu_ibc");
}

/* tmp.rcn_transform_tree (rcn_structures.h:464-468; rcn_transform_tree.c:1454-1518): the walker calls its leaves
 * directly, not through the table, so the whole walk is restated here around the leaf hooks. */
static void
hip_rcn_transform_tree(OVCTUDec *const c, uint8_t x0, uint8_t y0, uint8_t log2_tb_w, uint8_t log2_tb_h, uint8_t log2_max_tb_s,
                       uint8_t tr_depth, CUFlags cu_flags, const struct TUInfo *const tu)
{
    const int split_v = log2_tb_w > log2_max_tb_s, split_h = log2_tb_h > log2_max_tb_s;
    const int nsub = tr_depth ? 1 : (1 << (split_v + split_h));
    if (log2_tb_w > 6 && log2_tb_h < 7) {
        hip_rcn_transform_tree(c, x0, y0, 6, log2_tb_h, log2_max_tb_s, tr_depth + 1, cu_flags, &tu[0]);
        hip_rcn_transform_tree(c, x0 + 64, y0, 6, log2_tb_h, log2_max_tb_s, tr_depth + 1, cu_flags, &tu[8]);
        return;
    }
    if (log2_tb_h > 6 && log2_tb_w < 7) {
        hip_rcn_transform_tree(c, x0, y0, log2_tb_w, 6, log2_max_tb_s, tr_depth + 1, cu_flags, &tu[0]);
        hip_rcn_transform_tree(c, x0, y0 + 64, log2_tb_w, 6, log2_max_tb_s, tr_depth + 1, cu_flags, &tu[8]);
        return;
    }
    if (split_v || split_h) {
        const int w1 = (1 << log2_tb_w) >> split_v, h1 = (1 << log2_tb_h) >> split_h;
        const int l2w1 = log2_tb_w - split_v, l2h1 = log2_tb_h - split_h;
        hip_rcn_transform_tree(c, x0, y0, l2w1, l2h1, log2_max_tb_s, tr_depth + 1, cu_flags, &tu[0]);
        if (split_v) hip_rcn_transform_tree(c, x0 + w1, y0, l2w1, l2h1, log2_max_tb_s, tr_depth + 1, cu_flags, &tu[1 * nsub]);
        if (split_h) hip_rcn_transform_tree(c, x0, y0 + h1, l2w1, l2h1, log2_max_tb_s, tr_depth + 1, cu_flags, &tu[2 * nsub]);
        if (split_h && split_v) hip_rcn_transform_tree(c, x0 + w1, y0 + h1, l2w1, l2h1, log2_max_tb_s, tr_depth + 1, cu_flags, &tu[3 * nsub]);
        return;
    }
    /* leaf: rcn_res_wrap (:1432-1451) */
    if (c->transform_unit == (void *)&transform_unit_c) {
        hip_rcn_tu_c(c, x0, y0, log2_tb_w, log2_tb_h, cu_flags, tu->cbf_mask, tu);
    } else {
        struct hip_entry *e = entry_of(c, 0);
        PROF(e);
        if (e && e->rec) {
            ovhip_itask tl;
            const ovhip_itask *task_l = NULL, *task_c = NULL;
            e->aff_c_live = 0;
            if (e->pend.kind) pend_close(e, c);
            if (e->ciip.live) {
                /* the transform unit of the CIIP CU recorded last carries the residual of its two planar tasks */
                if (c->tmp_ciip && e->ciip.x0 == x0 && e->ciip.y0 == y0 && e->ciip.log2_w == log2_tb_w && e->ciip.log2_h == log2_tb_h) {
                    task_l = &e->ciip.tl; task_c = e->ciip.has_c ? &e->ciip.tc : NULL;
                    e->ciip.live = 0;
                } else {
                    ciip_close(e, c);
                }
            }
            /* the transform tree of the IBC CU stashed by rcn_ibc_l (+ rcn_ibc_c): every leaf inside the CU records its block; the
             * stash ends with the leaf that holds the CU's last sample.  A tree of any other CU while one is stashed is an error */
            int ibc_leaf = 0;
            if (e->ibc.live) {
                const int cw = 1 << e->ibc.cu.log2_w, ch = 1 << e->ibc.cu.log2_h;
                if ((cu_flags & flg_ibc_flag) && x0 >= e->ibc.x0 && y0 >= e->ibc.y0 && x0 + (1 << log2_tb_w) <= e->ibc.x0 + cw &&
                    y0 + (1 << log2_tb_h) <= e->ibc.y0 + ch) {
                    ibc_leaf = 1;
                } else ibc_orphan(e);
            } else if ((cu_flags & flg_ibc_flag) && !e->err) {
                latch(e, OVHIP_EINVAL, "transform tree of an intra block copy (IBC) coding unit without its rcn_ibc_l call");
            }
            if (ibc_leaf) {
                /* an IBC CU takes the inter branch of the transform unit: rcn_tu_st, or rcn_tu_l for the luma-only CUs of a dual tree /
                 * `share` (a cbf of 0 still records the block: it carries the prediction) */
                if (c->transform_unit == (void *)&transform_unit_st) {
                    record_tu_ibc(e, c, 0, x0, y0, log2_tb_w, log2_tb_h, cu_flags, tu->cbf_mask, tu);
                    tu_st_books(c, x0, y0, log2_tb_w, log2_tb_h, cu_flags, tu->cbf_mask);
                } else {
                    record_tu_ibc(e, c, 1, x0, y0, log2_tb_w, log2_tb_h, cu_flags, tu->cbf_mask ? 0x10 : 0, tu);
                    if (tu->cbf_mask) fill_bs_map(&c->dbf_info.bs1_map, x0, y0, log2_tb_w, log2_tb_h);
                    fill_ctb_bound(&c->dbf_info, x0, y0, log2_tb_w, log2_tb_h);
                }
                if (x0 + (1 << log2_tb_w) == e->ibc.x0 + (1 << e->ibc.cu.log2_w) && y0 + (1 << log2_tb_h) == e->ibc.y0 + (1 << e->ibc.cu.log2_h))
                    e->ibc.live = 0;
                return;
            }
            if (cu_flags & flg_pred_mode_flag) {
                /* rcn_intra_tu (:1384-1430): the prediction reads the progress field, then extends it */
                if (!(cu_flags & flg_isp_flag)) { luma_task(c, x0, y0, log2_tb_w, log2_tb_h, cu_flags, c->intra_mode, 0, &tl); task_l = &tl; }
                if (!(cu_flags & flg_intra_bdpcm_luma_flag)) fill_bs_map(&c->dbf_info.bs2_map, x0, y0, log2_tb_w, log2_tb_h);
                ctu_field_set_rect_bitfield(&c->rcn_ctx.progress_field, x0 >> LOG2_MIN_CU_S, y0 >> LOG2_MIN_CU_S,
                                            (1 << log2_tb_w) >> LOG2_MIN_CU_S, (1 << log2_tb_h) >> LOG2_MIN_CU_S);
            }
            if (c->transform_unit == (void *)&transform_unit_st) {
                tu_st_common(e, c, x0, y0, log2_tb_w, log2_tb_h, cu_flags, tu->cbf_mask, tu, task_l, task_c);
            } else {
                /* dual-tree luma: rcn_tu_l (:1305-1346) = the luma half of rcn_tu_st */
                if (tu->cbf_mask || task_l) record_tu(e, c, 1, x0, y0, log2_tb_w, log2_tb_h, cu_flags, tu->cbf_mask ? 0x10 : 0, tu, task_l, NULL);
                if (tu->cbf_mask) {
                    fill_bs_map(&c->dbf_info.bs1_map, x0, y0, log2_tb_w, log2_tb_h);
                    if ((cu_flags & flg_pred_mode_flag) && !(cu_flags & flg_intra_bdpcm_luma_flag)) fill_bs_map(&c->dbf_info.bs2_map, x0, y0, log2_tb_w, log2_tb_h);
                }
                fill_ctb_bound(&c->dbf_info, x0, y0, log2_tb_w, log2_tb_h);
            }
        }
    }
    if (c->tmp_ciip) {
        fill_bs_map(&c->dbf_info.bs2_map, x0, y0, log2_tb_w, log2_tb_h);
        fill_bs_map(&c->dbf_info.bs2_map_c, x0, y0, log2_tb_w, log2_tb_h);
    }
}

/* tmp.recon_isp_subtree_v / _h (rcn_structures.h:480-491; rcn_transform_tree.c:1087-1205).  The caller has already marked the
 * whole CU in the progress field (vcl_transform_unit.c:1878), so the partitions see each other as available. */
static void
isp_subtree(OVCTUDec *const c, unsigned int x0, unsigned int y0, unsigned int log2_cb_w, unsigned int log2_cb_h, uint8_t intra_mode,
            const struct ISPTUInfo *const tu, int vertical)
{
    ENTER(c);
    const int l2 = c->part_ctx->log2_ctu_s;
    const struct CTUBitField *pf = &c->rcn_ctx.progress_field;
    ovhip_tu_state st;
    ovhip_isp_desc d;
    int32_t l2p, n_pb, l2pred, n_pred;
    fill_tu_state(e, c, &st);
    memset(&d, 0, sizeof(d));
    ovhip_isp_geometry((int32_t)log2_cb_w, (int32_t)log2_cb_h, vertical, &l2p, &n_pb, &l2pred, &n_pred);
    d.x0 = (uint16_t)((c->ctb_x << l2) + x0); d.y0 = (uint16_t)((c->ctb_y << l2) + y0);
    d.log2_cb_w = (uint8_t)log2_cb_w; d.log2_cb_h = (uint8_t)log2_cb_h; d.vertical = (uint8_t)vertical; d.intra_mode = intra_mode;
    d.cbf_mask = tu->cbf_mask; d.lfnst_flag = tu->lfnst_flag; d.lfnst_idx = tu->lfnst_idx; d.mts_enabled = c->mts_enabled;
    d.coef = c->residual_y;
    for (int i = 0; i < n_pb && i < 4; ++i) { d.last_pos[i] = tu->tb_info[i].last_pos; d.sig_sb_map[i] = tu->tb_info[i].sig_sb_map; }
    const int nb_a = ((2 << log2_cb_w) >> 2) + 1, nb_l = ((2 << log2_cb_h) >> 2) + 1;
    for (int k = 0; k < n_pred && k < 4; ++k) {
        /* the maps intra_pred_isp hands to fill_ref_above_0 / fill_ref_left_0 for this call (rcn_intra.c:584-594) */
        const int off = k << l2pred, px = (int)x0 + (vertical ? off : 0), py = (int)y0 + (vertical ? 0 : off), off_y = vertical ? 0 : off;
        const uint64_t ma = (pf->hfield[(py >> 2) + !!(off_y % 4)] >> (x0 >> 2)) & ((1llu << (nb_a + 1)) - 1);
        const uint64_t ml = (pf->vfield[px >> 2] >> (y0 >> 2)) & ((1llu << (nb_l + 1)) - 1);
        d.corner[k] = (uint8_t)((ma & 1) | ((ml & 1) << 1));
        d.avl_abv[k] = (uint8_t)top_bit(ma >> 1); d.avl_lft[k] = (uint8_t)top_bit(ml >> 1);
        /* deblocking bookkeeping of the scalar orchestrator (:1136-1137, :1189-1192) */
        if (vertical) {
            fill_ctb_bound(&c->dbf_info, px, py, l2pred, log2_cb_h);
            fill_bs_map(&c->dbf_info.bs2_map, px, py, l2pred, log2_cb_h);
        } else if (!(off_y & 3)) {
            fill_ctb_bound(&c->dbf_info, px, py, log2_cb_w, l2p >= 2 ? l2p : 2);
            fill_bs_map(&c->dbf_info.bs2_map, px, py, log2_cb_w, l2p >= 2 ? l2p : 2);
        }
    }
    latch(e, ovhip_rec_isp_cu(e->rec, &st, &d), "ovhip_rec_isp_cu");
}

static void
hip_recon_isp_subtree_v(OVCTUDec *const c, unsigned int x0, unsigned int y0, unsigned int log2_cb_w, unsigned int log2_cb_h, uint8_t intra_mode,
                        const struct ISPTUInfo *const tu)
{ isp_subtree(c, x0, y0, log2_cb_w, log2_cb_h, intra_mode, tu, 1); }

static void
hip_recon_isp_subtree_h(OVCTUDec *const c, unsigned int x0, unsigned int y0, unsigned int log2_cb_w, unsigned int log2_cb_h, uint8_t intra_mode,
                        const struct ISPTUInfo *const tu)
{ isp_subtree(c, x0, y0, log2_cb_w, log2_cb_h, intra_mode, tu, 0); }

/* a CIIP CU without residual (no transform unit followed): its planar tasks alone */
void
ciip_close(struct hip_entry *e, OVCTUDec *c)
{
    ovhip_tu_state st;
    ovhip_tu_desc d;
    e->ciip.live = 0;
    fill_tu_state(e, c, &st);
    memset(&d, 0, sizeof(d));
    d.x0 = e->ciip.tl.x; d.y0 = e->ciip.tl.y; d.log2_tb_w = (uint8_t)e->ciip.log2_w; d.log2_tb_h = (uint8_t)e->ciip.log2_h;
    latch(e, ovhip_rec_tu_intra(e->rec, &st, &d, &e->ciip.tl, e->ciip.has_c ? &e->ciip.tc : NULL), "ovhip_rec_tu_intra(ciip)");
}

/* ------------------------------------------------------------------------------------ prediction units */
/* rcn_mcp_b (rcn_structures.h:640-646; rcn_inter.c:2769-2813) */
static void
hip_rcn_mcp_b(OVCTUDec *const c, struct OVBuffInfo dst, struct InterDRVCtx *const ic, const OVPartInfo *const part_ctx,
              const OVMV mv0, const OVMV mv1, unsigned int x0, unsigned int y0, unsigned int log2_pb_w, unsigned int log2_pb_h,
              uint8_t inter_dir, uint8_t ref_idx0, uint8_t ref_idx1)
{
    (void)dst; (void)ic; (void)part_ctx;
    ENTER(c);
    ovhip_pu_desc d;
    fill_pu_idx(e, c, &d, x0, y0, log2_pb_w, log2_pb_h, inter_dir, mv0, mv1, ref_idx0, ref_idx1);
    latch(e, ovhip_rec_pu(e->rec, &d), "ovhip_rec_pu");
}

/* rcn_mcp (rcn_structures.h:636-638; rcn_inter.c:2750-2767): uni-prediction, type 0 = list 0 */
static void
hip_rcn_mcp(OVCTUDec *const c, struct OVBuffInfo dst, int x0, int y0, int log2_pu_w, int log2_pu_h, OVMV mv, uint8_t type, uint8_t ref_idx)
{
    (void)dst;
    ENTER(c);
    struct InterDRVCtx *ic = &c->drv_ctx.inter_ctx;
    ovhip_pu_desc d;
    mv.ref_idx = (int8_t)ref_idx;
    fill_pu(e, c, &d, x0, y0, log2_pu_w, log2_pu_h, type ? 2 : 1, mv, mv, type ? NULL : ic->rpl0[ref_idx], type ? ic->rpl1[ref_idx] : NULL);
    d.bcw_idx_plus1 = 0;
    latch(e, ovhip_rec_pu(e->rec, &d), "ovhip_rec_pu");
}
/* rcn_gpm_b (rcn_structures.h:687-688; rcn_inter.c:3118-3143) */
static void
hip_rcn_gpm_b(OVCTUDec *const c, struct VVCGPM *g, int x0, int y0, int log2_pb_w, int log2_pb_h)
{
    ENTER(c);
    struct InterDRVCtx *ic = &c->drv_ctx.inter_ctx;
    const OVPicture *p0 = g->inter_dir0 == 1 ? ic->rpl0[g->mv0.ref_idx] : ic->rpl1[g->mv0.ref_idx];
    const OVPicture *p1 = g->inter_dir1 == 1 ? ic->rpl0[g->mv1.ref_idx] : ic->rpl1[g->mv1.ref_idx];
    ovhip_pu_desc d;
    fill_pu_lists(e, c, &d, x0, y0, log2_pb_w, log2_pb_h, 3, g->mv0, g->mv1, p0, p1, g->inter_dir0 == 1 ? 0 : 1, g->inter_dir1 == 1 ? 0 : 1);
    d.bcw_idx_plus1 = 0;
    d.refine = OVHIP_PU_GPM; d.gpm_split_dir = (uint8_t)g->split_dir;
    latch(e, ovhip_rec_pu(e->rec, &d), "ovhip_rec_pu(gpm)");
}

/* rcn_ciip_b / rcn_ciip (rcn_structures.h:673-683; rcn_inter.c:3011-3067): inter part + planar intra + blend */
static void
ciip_common(struct hip_entry *e, OVCTUDec *c, ovhip_pu_desc *d, int x0, int y0, int log2_pb_w, int log2_pb_h)
{
    const int l2 = c->part_ctx->log2_min_cb_s;
    const int mode_abv = c->part_map.cu_mode_x[(x0 + (1 << log2_pb_w) - 1) >> l2];
    const int mode_lft = c->part_map.cu_mode_y[(y0 + (1 << log2_pb_h) - 1) >> l2];
    const int wt = 1 + (mode_abv == OV_INTRA || mode_abv == OV_MIP) + (mode_lft == OV_INTRA || mode_lft == OV_MIP);    /* rcn_inter.c:2975-2981 */
    latch(e, ovhip_rec_pu(e->rec, d), "ovhip_rec_pu(ciip)");
    /* the planar predictions (intra_pred / intra_pred_c with mode 0 and no CU flags, rcn_inter.c:3026-3028) and the blend
     * belong to the ordered pass: two tasks with the CU's weight, the references read out of the progress fields as they
     * are now; chroma blocks 2 samples wide keep the inter prediction (:2997-2999) */
    e->ciip.live = 1; e->ciip.x0 = x0; e->ciip.y0 = y0; e->ciip.log2_w = log2_pb_w; e->ciip.log2_h = log2_pb_h;
    luma_task(c, x0, y0, log2_pb_w, log2_pb_h, 0, OVINTRA_PLANAR, wt, &e->ciip.tl);
    e->ciip.has_c = log2_pb_w > 2;
    if (e->ciip.has_c) chroma_task(c, x0 >> 1, y0 >> 1, log2_pb_w - 1, log2_pb_h - 1, 0, OVINTRA_PLANAR, wt, &e->ciip.tc);
}

static void
hip_rcn_ciip_b(OVCTUDec *const c, const OVMV mv0, const OVMV mv1, unsigned int x0, unsigned int y0, unsigned int log2_pb_w,
               unsigned int log2_pb_h, uint8_t inter_dir, uint8_t ref_idx0, uint8_t ref_idx1)
{
    ENTER(c);
    ovhip_pu_desc d;
    fill_pu_idx(e, c, &d, x0, y0, log2_pb_w, log2_pb_h, inter_dir, mv0, mv1, ref_idx0, ref_idx1);
    ciip_common(e, c, &d, x0, y0, log2_pb_w, log2_pb_h);
}

static void
hip_rcn_ciip(OVCTUDec *const c, int x0, int y0, int log2_pb_w, int log2_pb_h, OVMV mv, uint8_t ref_idx)
{
    ENTER(c);
    struct InterDRVCtx *ic = &c->drv_ctx.inter_ctx;
    ovhip_pu_desc d;
    mv.ref_idx = (int8_t)ref_idx;
    fill_pu(e, c, &d, x0, y0, log2_pb_w, log2_pb_h, 1, mv, mv, ic->rpl0[ref_idx], NULL);
    d.bcw_idx_plus1 = 0;
    ciip_common(e, c, &d, x0, y0, log2_pb_w, log2_pb_h);
}

/* ------------------------------------------------------------------------------------ LMCS */
/* rcn_init_lmcs (rcn_structures.h:540; rcn_lmcs.c:345-361): the scalar one keeps filling lmcs_info (the parse loop
 * reads it); the device tables are built from the same APS data */
static void
hip_rcn_init_lmcs(struct LMCSInfo *li, const struct OVLMCSData *const ld)
{
    OVCTUDec *c = ctudec_of_lmcs(li);
    struct hip_entry *e = entry_of(c, 0);
    PROF(e);
    if (!e) return;
    e->scalar.rcn_init_lmcs(li, ld);
    ovhip_lmcs_data hd;
    memset(&hd, 0, sizeof(hd));
    hd.min_bin_idx = ld->lmcs_min_bin_idx; hd.delta_max_bin_idx = ld->lmcs_delta_max_bin_idx;
    hd.crs_offset = (int16_t)(ld->lmcs_delta_sign_crs_flag ? -ld->lmcs_delta_abs_crs : ld->lmcs_delta_abs_crs);
    for (int i = 0; i < 16; ++i) hd.cw_delta[i] = (int16_t)(ld->lmcs_delta_sign_cw_flag[i] ? -ld->lmcs_delta_abs_cw[i] : ld->lmcs_delta_abs_cw[i]);
    latch(e, ovhip_lmcs_build(&hd, &e->luts), "ovhip_lmcs_build");
    e->have_luts = 1;
}

/* rcn_lmcs_compute_chroma_scale (rcn_structures.h:535-538; rcn_lmcs.c:320-343): needs RECONSTRUCTED luma around the
 * 64x64 region, which only exists on the device -> record the region; the TUs that follow refer to it */
static void
hip_lmcs_chroma_scale(struct LMCSInfo *const li, int16_t stride, const struct CTUBitField *const pf, const OVSample *ctu_y,
                      uint8_t x0, uint8_t y0)
{
    (void)stride; (void)ctu_y;
    OVCTUDec *c = ctudec_of_lmcs(li);
    ENTER(c);
    const int l2 = c->part_ctx->log2_ctu_s;
    const uint32_t abv = (uint32_t)((pf->hfield[y0 >> 2] >> ((x0 >> 2) + 1)) & 0xffff);
    const uint32_t lft = (uint32_t)((pf->vfield[x0 >> 2] >> ((y0 >> 2) + 1)) & 0xffff);
    int r = ovhip_rec_lmcs_region(e->rec, (c->ctb_x << l2) + x0, (c->ctb_y << l2) + y0, abv, lft);
    latch(e, r, "ovhip_rec_lmcs_region");
    e->lmcs_region_live = r >= 0;
}

/* lmcs_reshape_backward per CTU (slicedec.c:746-750): one launch per picture in the flush instead */
static void hip_noop_reshape(OVSample *dst, ptrdiff_t stride, const struct LMCSLUTs *const luts, int w, int h)
{ (void)dst; (void)stride; (void)luts; (void)w; (void)h; }

/* ------------------------------------------------------------------------------------ deblocking */
/* The CTU's maps are read where they lie in the decoder's struct DBFInfo (ovhip_dbf_view: same element layout, include/ovvc_hip.h); r3 / r4
 * filled and copied a 9 KB descriptor per CTU. */
static void
view_dbf(ovhip_dbf_view *o, const struct DBFInfo *d)
{
    o->ctb_bound_ver = d->ctb_bound_ver; o->ctb_bound_hor = d->ctb_bound_hor; o->ctb_bound_ver_c = d->ctb_bound_ver_c; o->ctb_bound_hor_c = d->ctb_bound_hor_c;
    o->aff_edg_ver = d->aff_edg_ver; o->aff_edg_hor = d->aff_edg_hor;
    o->bs2_ver = d->bs2_map.ver; o->bs2_hor = d->bs2_map.hor; o->bs2c_ver = d->bs2_map_c.ver; o->bs2c_hor = d->bs2_map_c.hor;
    o->bs1_ver = d->bs1_map.ver; o->bs1_hor = d->bs1_map.hor; o->bs1cb_ver = d->bs1_map_cb.ver; o->bs1cb_hor = d->bs1_map_cb.hor;
    o->bs1cr_ver = d->bs1_map_cr.ver; o->bs1cr_hor = d->bs1_map_cr.hor; o->affine_ver = d->affine_map.ver; o->affine_hor = d->affine_map.hor;
    o->qp_y = d->qp_map_y.hor; o->qp_cb = d->qp_map_cb.hor; o->qp_cr = d->qp_map_cr.hor;
    o->beta_offset = d->beta_offset; o->tc_offset = d->tc_offset;
    o->disable_v = d->disable_v; o->disable_h = d->disable_h;
    o->pad = 0;
}

static void
dbf_ctu(const struct OVRCNCtx *const r, struct DBFInfo *const dbf, uint8_t log2_ctu_s, uint8_t last_x, uint8_t last_y, int ctu_w, int ctu_h)
{
    OVCTUDec *c = r->ctudec;
    ENTER(c);
    ovhip_dbf_view s;
    view_dbf(&s, dbf);
    s.log2_ctu_s = log2_ctu_s; s.last_x = last_x; s.last_y = last_y;
    s.ctu_lft = !!(c->ctu_ngh_flags & CTU_LFT_FLG); s.ctu_abv = !!(c->ctu_ngh_flags & CTU_UP_FLG);
    s.ctu_w = (uint16_t)ctu_w; s.ctu_h = (uint16_t)ctu_h;
    s.ctb_x = c->ctb_x; s.ctb_y = c->ctb_y;
    if (c->tmp_slice_type != 2) {
        /* P / B slices: the slot's own MV-based boundary-strength pre-pass (dbf_ctu_preproc_v/_h, rcn_df.c:1821-1874;
         * static there) on the CTU's motion grids, straight into dbf_info->bs1_map as the scalar slot leaves it:
         * dbf_store_info() carries it to the neighbouring CTUs (slicedec.c:872-877). */
        const struct InterDRVCtx *ic = &c->drv_ctx.inter_ctx;
        ovhip_dbf_mv_ctx mc;
        memset(&mc, 0, sizeof(mc));
        memcpy(mc.cu_edge_ver, dbf->cu_edge.ver, sizeof(mc.cu_edge_ver)); memcpy(mc.cu_edge_hor, dbf->cu_edge.hor, sizeof(mc.cu_edge_hor));
        memcpy(mc.map0_h, ic->mv_ctx0.map.hfield, sizeof(mc.map0_h)); memcpy(mc.map0_v, ic->mv_ctx0.map.vfield, sizeof(mc.map0_v));
        memcpy(mc.map1_h, ic->mv_ctx1.map.hfield, sizeof(mc.map1_h)); memcpy(mc.map1_v, ic->mv_ctx1.map.vfield, sizeof(mc.map1_v));
        if (dbf->ibc_ctx) { memcpy(mc.ibc_h, dbf->ibc_ctx->ctu_map.hfield, sizeof(mc.ibc_h)); memcpy(mc.ibc_v, dbf->ibc_ctx->ctu_map.vfield, sizeof(mc.ibc_v)); }
        memcpy(mc.dist_ref0, ic->dist_ref_0, sizeof(mc.dist_ref0)); memcpy(mc.dist_ref1, ic->dist_ref_1, sizeof(mc.dist_ref1));
        mc.mvs0 = ic->mv_ctx0.mvs; mc.mvs1 = ic->mv_ctx1.mvs; mc.mv_bytes = sizeof(OVMV);
        latch(e, ovhip_rec_dbf_mv_prepass_view(&s, dbf->bs1_map.ver, dbf->bs1_map.hor, &mc), "ovhip_rec_dbf_mv_prepass");
    }
    latch(e, ovhip_rec_dbf_row(e->rec, &s, 1), "ovhip_rec_dbf_row");
}

/* df.rcn_dbf_ctu / df.rcn_dbf_truncated_ctu (rcn_structures.h:408-413; rcn_df.c:2169-2231) */
static void hip_rcn_dbf_ctu(const struct OVRCNCtx *const r, struct DBFInfo *const dbf, uint8_t log2_ctu_s, uint8_t last_x, uint8_t last_y)
{ dbf_ctu(r, dbf, log2_ctu_s, last_x, last_y, 0, 0); }
static void hip_rcn_dbf_truncated_ctu(const struct OVRCNCtx *const r, struct DBFInfo *const dbf, uint8_t log2_ctu_s, uint8_t last_x,
                                      uint8_t last_y, uint8_t ctu_w, uint8_t ctu_h)
{ dbf_ctu(r, dbf, log2_ctu_s, last_x, last_y, ctu_w, ctu_h); }

/* ------------------------------------------------------------------------------------ SAO / ALF: parameter capture */
int
params_alloc(struct hip_entry *e, const OVCTUDec *c, const struct RectEntryInfo *einfo)
{
    /* the arrays cover the PICTURE; a rect entry (tile) fills its own CTUs (slicedec.c:484-514: ctb_x / ctb_y = its origin) */
    const int l2 = c->part_ctx->log2_ctu_s;
    const int nw = (e->pic_w + (1 << l2) - 1) >> l2, nh = (e->pic_h + (1 << l2) - 1) >> l2;
    if (einfo->ctb_x + einfo->nb_ctu_w > nw || einfo->ctb_y + einfo->nb_ctu_h > nh) {
        latch(e, OVHIP_EINVAL, "rect entry outside the picture");
        return -1;
    }
    e->log2_ctu = l2; e->nb_ctu_w = nw; e->nb_ctu_h = nh;
    e->whole_pic_entry = !einfo->ctb_x && !einfo->ctb_y && einfo->nb_ctu_w == nw && einfo->nb_ctu_h == nh;
    if (e->n_ctu != (size_t)nw * nh) {
        free(e->sao); free(e->alf);
        e->n_ctu = (size_t)nw * nh;
        e->sao = calloc(e->n_ctu, sizeof(*e->sao)); e->alf = calloc(e->n_ctu, sizeof(*e->alf));
        if (!e->sao || !e->alf) { latch(e, OVHIP_ENOMEM, "filter parameter arrays"); return -1; }
    }
    return 0;
}

/* The in-loop filters of a rect entry stop at its borders: SAO leaves the samples whose neighbour lies outside alone and ALF pads
 * (is_border from the ENTRY-local CTU index, rcn_sao.c:211-214, rcn_alf.c:1313-1318; rcn_extend_filter_region, rcn_ctu.c:361-508).
 * The device filters the whole picture at once: every CTU carries which of its sides are such borders.  A picture of one entry
 * carries none (its borders are the picture's, which the kernels know). */
static uint8_t
entry_borders(const struct hip_entry *e, const struct RectEntryInfo *einfo, int x, int y)
{
    if (e->whole_pic_entry) return 0;
    return (uint8_t)((x == 0 ? OVHIP_BORDER_LEFT : 0) | (x == einfo->nb_ctu_w - 1 ? OVHIP_BORDER_RIGHT : 0) |
                     (y == 0 ? OVHIP_BORDER_UPPER : 0) | (y == einfo->nb_ctu_h - 1 ? OVHIP_BORDER_BOTTOM : 0) |
                     (einfo->nb_ctu_h == 1 ? OVHIP_BORDER_ONE_ROW : 0));
}

void
sao_row(struct hip_entry *e, const OVCTUDec *c, const struct RectEntryInfo *einfo, int ctb_y)
{
    if (ctb_y < 0 || ctb_y >= einfo->nb_ctu_h || params_alloc(e, c, einfo)) return;
    const struct SAOInfo *si = &c->sao_info;
    for (int x = 0; x < einfo->nb_ctu_w; ++x) {
        const SAOParamsCtu *s = &si->sao_params[ctb_y * einfo->nb_ctu_w + x];
        ovhip_sao_ctu *o = &e->sao[(einfo->ctb_y + ctb_y) * e->nb_ctu_w + einfo->ctb_x + x];
        memset(o, 0, sizeof(*o));
        o->border = entry_borders(e, einfo, x, ctb_y);
        for (int k = 0; k < (si->chroma_format_idc ? 3 : 1); ++k) {
            o->type[k] = s->type_idx[k]; o->band_position[k] = s->band_position[k]; o->eo_class[k] = s->eo_class[k];
            memcpy(o->offset_val[k], s->offset_val[k], sizeof(o->offset_val[k]));
        }
    }
    e->sao_on = 1;
}

/* sao.rcn_sao_filter_line / rcn_sao_first_pix_rows (rcn_structures.h:344-350; rcn_sao.c:190-293): line ctb_y filters
 * the band [128 ctb_y + 6, 128 (ctb_y + 1) + 6) with the parameters of rows ctb_y and ctb_y + 1; on the device every
 * sample takes the parameters of the CTU that contains it (same result) */
static void
hip_sao_filter_line(OVCTUDec *const c, const struct RectEntryInfo *const einfo, uint16_t ctb_y)
{
    ENTER(c);
    if (!c->sao_info.sao_luma_flag && !c->sao_info.sao_chroma_flag) return;
    sao_row(e, c, einfo, ctb_y);
    sao_row(e, c, einfo, ctb_y + 1);
}

static void
hip_sao_first_pix_rows(OVCTUDec *const c, const struct RectEntryInfo *const einfo, uint16_t ctb_y)
{
    ENTER(c);
    if (c->sao_info.sao_luma_flag || c->sao_info.sao_chroma_flag) sao_row(e, c, einfo, ctb_y);
    /* the only hook that runs at the end of row 0 (slicedec.c:934-941); an entry of one row ends in hip_alf_filter_line alone */
    if (einfo->nb_ctu_h > 1) rows_parsed(e, c, einfo, 1, 0);
}

/* the CC-ALF coefficients of the slice's two APSs, as the device reads them */
void
alf_cc_capture(struct hip_entry *e, const struct ALFInfo *ai)
{
    if (ai->aps_cc_alf_data_cb) memcpy(e->alf_cc[0], ai->aps_cc_alf_data_cb->alf_cc_mapped_coeff[0], sizeof(e->alf_cc[0]));
    if (ai->aps_cc_alf_data_cr) memcpy(e->alf_cc[1], ai->aps_cc_alf_data_cr->alf_cc_mapped_coeff[1], sizeof(e->alf_cc[1]));
}

/* the ALF parameters of CTU row ctb_y of the entry (parsed with the row's CTUs: valid once the row has been parsed) */
void
alf_row(struct hip_entry *e, const OVCTUDec *c, const struct RectEntryInfo *einfo, int ctb_y)
{
    const struct ALFInfo *ai = &c->alf_info;
    if (ctb_y < 0 || ctb_y >= einfo->nb_ctu_h || !(ai->alf_luma_enabled_flag || ai->alf_cb_enabled_flag || ai->alf_cr_enabled_flag)) return;
    for (int x = 0; x < einfo->nb_ctu_w; ++x) {
        const int i = ctb_y * einfo->nb_ctu_w + x;
        const ALFParamsCtu *p = &ai->ctb_alf_params[i];
        ovhip_alf_ctu *o = &e->alf[(einfo->ctb_y + ctb_y) * e->nb_ctu_w + einfo->ctb_x + x];
        o->flags = p->ctb_alf_flag; o->luma_set = p->ctb_alf_idx; o->cb_alt = p->cb_alternative; o->cr_alt = p->cr_alternative;
        o->cc_cb_idx = ai->cc_alf_cb_enabled_flag ? ai->ctb_cc_alf_filter_idx[0][i] : 0;
        o->cc_cr_idx = ai->cc_alf_cr_enabled_flag ? ai->ctb_cc_alf_filter_idx[1][i] : 0;
        o->border = entry_borders(e, einfo, x, ctb_y);
    }
    alf_cc_capture(e, ai);
    e->alf_on = 1;
}

/* alf.rcn_alf_filter_line (rcn_structures.h:333; rcn_alf.c:1285-1433): the LAST slot call before a CTU row is published
 * (slicedec.c:934-956).  Captures the row's ALF parameters, refines the DMVR vectors recorded so far (so that the row's
 * TMVP field is final), and for the last row of the picture runs the flush. */
static void
hip_alf_filter_line(OVCTUDec *const c, const struct RectEntryInfo *const einfo, uint16_t ctb_y)
{
    ENTER(c);
    if (params_alloc(e, c, einfo)) return;
    alf_row(e, c, einfo, ctb_y);
    /* the entry's last row: with it the last of the picture's rect entries ends the picture (ovthreads.c:93-114: the last entry
     * job to finish calls slicedec_finish_decoding) */
    int last = 0;
    if (ctb_y == einfo->nb_ctu_h - 1) {
        e->ctus_left -= einfo->nb_ctu_w * einfo->nb_ctu_h;
        last = e->ctus_left <= 0;
        if (last) e->ctus_left = 0;
    }
    /* this hook runs at the end of CTU row ctb_y + 1 (decode_ctu_line, slicedec.c:934-956) -- except for the picture's last two lines,
     * which both run at its end */
    rows_parsed(e, c, einfo, ctb_y + 2, last);
}

/* ------------------------------------------------------------------------------------ install */
void
rec_install(struct RCNFunctions *f)
{
    f->tmp.rcn_transform_tree = &hip_rcn_transform_tree;
    f->tmp.rcn_tu_st = &hip_rcn_tu_st;
    f->tmp.rcn_tu_c  = &hip_rcn_tu_c;
    f->tmp.recon_isp_subtree_h = &hip_recon_isp_subtree_h;
    f->tmp.recon_isp_subtree_v = &hip_recon_isp_subtree_v;
    f->rcn_ibc_l = &hip_rcn_ibc_l;
    f->rcn_ibc_c = &hip_rcn_ibc_c;
    f->rcn_mcp = &hip_rcn_mcp;
    f->rcn_mcp_b = &hip_rcn_mcp_b;
    f->rcn_gpm_b = &hip_rcn_gpm_b;
    f->rcn_ciip_b = &hip_rcn_ciip_b;
    f->rcn_ciip = &hip_rcn_ciip;
    f->rcn_init_lmcs = &hip_rcn_init_lmcs;
    f->rcn_lmcs_compute_chroma_scale = &hip_lmcs_chroma_scale;
    f->lmcs_reshape_backward = &hip_noop_reshape;
    f->df.rcn_dbf_ctu = &hip_rcn_dbf_ctu;
    f->df.rcn_dbf_truncated_ctu = &hip_rcn_dbf_truncated_ctu;
    f->sao.rcn_sao_filter_line = &hip_sao_filter_line;
    f->sao.rcn_sao_first_pix_rows = &hip_sao_first_pix_rows;
    f->alf.rcn_alf_filter_line = &hip_alf_filter_line;
    /* alf.rcn_alf_reconstruct_coeff_APS stays scalar: host-side expansion of the APS into RCNALF, read by the flush */
}
