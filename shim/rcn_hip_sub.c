/* rcn_hip_sub.c -- caller mode of the override block for the UNPATCHED reference (rcn_hip.h, rcn_hip_priv.h; the other mode:
 * rcn_hip_cu.c).  Its callers cut affine, BDOF and DMVR coding units into sub-block calls, which are collected back into one descriptor
 * per CU here; and the decoder reports its CTU rows itself, so the row step waits until the vectors of the rows about to be reported
 * are refined. */
#include "rcn_hip_priv.h"

/* ---- CUs the reference's callers cut into sub-block calls: collected back into one descriptor ---- */
void
pend_close(struct hip_entry *e, OVCTUDec *c)
{
    const int kind = e->pend.kind;
    e->pend.kind = PEND_NONE;
    if (kind == PEND_AFFINE) {
        /* luma sub-blocks arrived in raster order: cols x rows of 4x4 */
        const int cols = e->pend.cols ? e->pend.cols : e->pend.cur_col, rows = e->pend.n / (cols ? cols : 1);
        int log2_w = 2, log2_h = 2;
        while ((1 << log2_w) < cols * 4) ++log2_w;
        while ((1 << log2_h) < rows * 4) ++log2_h;
        if (cols * rows != e->pend.n || (4 << (log2_w - 2)) != cols * 4 || (4 << (log2_h - 2)) != rows * 4 || cols < 2 || rows < 2) {
            /* not the affine drivers' pattern: each call is what the slot says it is, a 4x4 luma prediction (on a scaled reference:
             * an ovhip_rpr_unit with the 4x4 filter sets, OVHIP_RPR_TOOL_PU4x4) */
            if (e->pend.prof_dir) { latch(e, OVHIP_EINVAL, "PROF sub-block calls do not form a CU"); return; }
            for (int i = 0; i < e->pend.n; ++i) {
                const int row = cols ? i / cols : 0, col = cols ? i % cols : i, k = (row * 32 + col) * 2;
                OVMV m0 = { .x = e->pend.mv0[k], .y = e->pend.mv0[k + 1], .bcw_idx_plus1 = e->pend.bcw };
                OVMV m1 = { .x = e->pend.mv1[k], .y = e->pend.mv1[k + 1], .bcw_idx_plus1 = e->pend.bcw };
                ovhip_pu_desc d;
                fill_pu_idx(e, c, &d, e->pend.x0 + 4 * col, e->pend.y0 + 4 * row, 2, 2, e->pend.inter_dir, m0, m1, e->pend.ref_idx0, e->pend.ref_idx1);
                d.planes = 1;
                latch(e, ovhip_rec_pu(e->rec, &d), "ovhip_rec_pu(4x4 luma)");
            }
            return;
        }
        ovhip_affine_desc d;
        fill_affine(e, c, &d, e->pend.x0, e->pend.y0, log2_w, log2_h, e->pend.inter_dir, e->pend.bcw, e->pend.prof_dir, e->pend.ref_idx0,
                    e->pend.ref_idx1, &e->pend.prof);
        latch(e, ovhip_rec_affine_cu(e->rec, &d), "ovhip_rec_affine_cu");
    } else if (kind == PEND_BDOF) {
        /* BDOF blocks without the CU's chroma call (never issued by the reference's callers): luma only */
        for (int i = 0; i < e->pend.n; ++i) {
            ovhip_pu_desc d;
            fill_pu_idx(e, c, &d, e->pend.bx[i], e->pend.by[i], e->pend.bl2w, e->pend.bl2h, 3, e->pend.bmv0, e->pend.bmv1, e->pend.ref_idx0, e->pend.ref_idx1);
            d.refine = OVHIP_PU_BDOF; d.planes = 1;
            latch(e, ovhip_rec_pu(e->rec, &d), "ovhip_rec_pu(bdof block)");
        }
    }
}

static void
pend_affine_add(struct hip_entry *e, OVCTUDec *c, int x0, int y0, OVMV mv0, OVMV mv1, uint8_t inter_dir, uint8_t ref_idx0,
                uint8_t ref_idx1, uint8_t prof_dir, const struct PROFInfo *prof)
{
    e->aff_c_live = 0;
    if (e->pend.kind == PEND_AFFINE) {
        /* next sub-block in raster order?  (x advances by 4; a row ends when x returns to the CU's left edge) */
        const int exp_x = e->pend.x0 + 4 * e->pend.cur_col, exp_y = e->pend.y0 + 4 * e->pend.rows_done;
        const int wrap = x0 == e->pend.x0 && y0 == exp_y + 4 && e->pend.cur_col >= 2 && (!e->pend.cols || e->pend.cols == e->pend.cur_col);
        if (wrap) { e->pend.cols = e->pend.cur_col; e->pend.rows_done++; e->pend.cur_col = 0; }
        else if (!(x0 == exp_x && y0 == exp_y && (!e->pend.cols || e->pend.cur_col < e->pend.cols)) || prof_dir != e->pend.prof_dir
                 || inter_dir != e->pend.inter_dir || e->pend.n >= 1024)
            pend_close(e, c);
    } else if (e->pend.kind) {
        pend_close(e, c);
    }
    if (!e->pend.kind) {
        e->pend.kind = PEND_AFFINE; e->pend.x0 = x0; e->pend.y0 = y0; e->pend.n = 0; e->pend.cols = 0; e->pend.rows_done = 0;
        e->pend.cur_col = 0;
        e->pend.inter_dir = inter_dir; e->pend.prof_dir = prof_dir; e->pend.bcw = mv0.bcw_idx_plus1;
        e->pend.ref_idx0 = ref_idx0; e->pend.ref_idx1 = ref_idx1;
        if (prof) e->pend.prof = *prof; else memset(&e->pend.prof, 0, sizeof(e->pend.prof));
    }
    const int k = (e->pend.rows_done * 32 + e->pend.cur_col) * 2;
    e->pend.mv0[k] = mv0.x; e->pend.mv0[k + 1] = mv0.y; e->pend.mv1[k] = mv1.x; e->pend.mv1[k + 1] = mv1.y;
    e->pend.cur_col++; e->pend.n++;
}

/* rcn_mcp_b_l (rcn_structures.h:648-654; rcn_inter.c:2815-2862).  The reference's only callers are the affine drivers,
 * one 4x4 sub-block per call (drv_affine_mvp.c:3264-3300). */
static void
hip_rcn_mcp_b_l(OVCTUDec *const c, struct OVBuffInfo dst, struct InterDRVCtx *const ic, const OVPartInfo *const part_ctx,
                const OVMV mv0, const OVMV mv1, unsigned int x0, unsigned int y0, unsigned int log2_pb_w, unsigned int log2_pb_h,
                uint8_t inter_dir, uint8_t ref_idx0, uint8_t ref_idx1)
{
    (void)dst; (void)ic; (void)part_ctx;
    struct hip_entry *e = entry_of(c, 0);
    PROF(e);
    if (!e || !e->rec) return;
    if (log2_pb_w == 2 && log2_pb_h == 2) { pend_affine_add(e, c, x0, y0, mv0, mv1, inter_dir, ref_idx0, ref_idx1, 0, NULL); return; }
    if (e->pend.kind) pend_close(e, c);
    ovhip_pu_desc d;
    fill_pu_idx(e, c, &d, x0, y0, log2_pb_w, log2_pb_h, inter_dir, mv0, mv1, ref_idx0, ref_idx1);
    d.planes = 1;
    latch(e, ovhip_rec_pu(e->rec, &d), "ovhip_rec_pu(luma)");
}

/* rcn_prof_mcp_b_l (rcn_structures.h:656-663; rcn_inter.c:2864-2918): 4x4 affine sub-block with PROF */
static void
hip_rcn_prof_mcp_b_l(OVCTUDec *const c, struct OVBuffInfo dst, struct InterDRVCtx *const ic, const OVPartInfo *const part_ctx,
                     const OVMV mv0, const OVMV mv1, unsigned int x0, unsigned int y0, unsigned int log2_pb_w, unsigned int log2_pb_h,
                     uint8_t inter_dir, uint8_t ref_idx0, uint8_t ref_idx1, uint8_t prof_dir, const struct PROFInfo *const prof_info)
{
    (void)dst; (void)ic; (void)part_ctx; (void)log2_pb_w; (void)log2_pb_h;
    struct hip_entry *e = entry_of(c, 0);
    PROF(e);
    if (!e || !e->rec) return;
    pend_affine_add(e, c, x0, y0, mv0, mv1, inter_dir, ref_idx0, ref_idx1, prof_dir, prof_info);
}

/* rcn_mcp_b_c (rcn_structures.h:665-671 region; rcn_inter.c:2920-2966): the chroma of an affine CU (8x8 luma area per
 * call, drv_affine_mvp.c:3371-3411), of a BDOF CU (whole CU, vcl_coding_unit.c:2469, :2664), or stand-alone */
static void
hip_rcn_mcp_b_c(OVCTUDec *const c, struct OVBuffInfo dst, struct InterDRVCtx *const ic, const OVPartInfo *const part_ctx,
                const OVMV mv0, const OVMV mv1, unsigned int x0, unsigned int y0, unsigned int log2_pb_w, unsigned int log2_pb_h,
                uint8_t inter_dir, uint8_t ref_idx0, uint8_t ref_idx1)
{
    (void)dst; (void)part_ctx;
    struct hip_entry *e = entry_of(c, 0);
    PROF(e);
    if (!e || !e->rec) return;
    if (e->pend.kind == PEND_AFFINE && log2_pb_w == 3 && log2_pb_h == 3 && (int)x0 == e->pend.x0 && (int)y0 == e->pend.y0) {
        /* first chroma call of the affine CU being collected closes its luma; the recorder derives the chroma vectors
         * of the whole CU itself (same averaging), so the remaining (3,3) calls inside the CU carry nothing new */
        const int cols = e->pend.cols ? e->pend.cols : e->pend.cur_col, rows = e->pend.n / (cols ? cols : 1);
        e->aff_c_x0 = e->pend.x0; e->aff_c_y0 = e->pend.y0; e->aff_c_x1 = e->pend.x0 + 4 * cols; e->aff_c_y1 = e->pend.y0 + 4 * rows;
        pend_close(e, c);
        e->aff_c_live = 1;
        return;
    }
    if (e->aff_c_live && log2_pb_w == 3 && log2_pb_h == 3 && (int)x0 >= e->aff_c_x0 && (int)x0 < e->aff_c_x1
        && (int)y0 >= e->aff_c_y0 && (int)y0 < e->aff_c_y1)
        return;
    e->aff_c_live = 0;
    if (e->pend.kind == PEND_BDOF) {
        /* the CU's chroma call: now the CU size is known -> one descriptor for the whole BDOF CU */
        const int w = 1 << log2_pb_w, h = 1 << log2_pb_h, bw = w > 16 ? 16 : w, bh = h > 16 ? 16 : h;
        int ok = (int)x0 == e->pend.bx[0] && (int)y0 == e->pend.by[0] && e->pend.n == (w / bw) * (h / bh) && (1 << e->pend.bl2w) == bw
                 && (1 << e->pend.bl2h) == bh && mv0.x == e->pend.bmv0.x && mv0.y == e->pend.bmv0.y && mv1.x == e->pend.bmv1.x
                 && mv1.y == e->pend.bmv1.y;
        if (ok) {
            e->pend.kind = PEND_NONE;
            ovhip_pu_desc d;
            fill_pu(e, c, &d, x0, y0, log2_pb_w, log2_pb_h, 3, e->pend.bmv0, e->pend.bmv1, ic->rpl0[ref_idx0], ic->rpl1[ref_idx1]);
            d.refine = OVHIP_PU_BDOF;
            latch(e, ovhip_rec_pu(e->rec, &d), "ovhip_rec_pu(bdof cu)");
            return;
        }
        pend_close(e, c);
    } else if (e->pend.kind) {
        pend_close(e, c);
    }
    ovhip_pu_desc d;
    fill_pu_idx(e, c, &d, x0, y0, log2_pb_w, log2_pb_h, inter_dir, mv0, mv1, ref_idx0, ref_idx1);
    d.planes = 2;
    latch(e, ovhip_rec_pu(e->rec, &d), "ovhip_rec_pu(chroma)");
}

/* rcn_bdof_mcp_l (rcn_structures.h:634-636 region; rcn_inter.c:1136-1250): one <=16x16 luma block of a BDOF CU */
static void
hip_rcn_bdof_mcp_l(OVCTUDec *const c, struct OVBuffInfo dst, uint8_t x0, uint8_t y0, uint8_t log2_pu_w, uint8_t log2_pu_h,
                   OVMV mv0, OVMV mv1, uint8_t ref_idx0, uint8_t ref_idx1)
{
    (void)dst;
    struct hip_entry *e = entry_of(c, 0);
    PROF(e);
    if (!e || !e->rec) return;
    e->aff_c_live = 0;
    if (e->pend.kind == PEND_BDOF && (e->pend.n >= 64 || log2_pu_w != e->pend.bl2w || log2_pu_h != e->pend.bl2h || mv0.x != e->pend.bmv0.x
                                      || mv0.y != e->pend.bmv0.y || mv1.x != e->pend.bmv1.x || mv1.y != e->pend.bmv1.y))
        pend_close(e, c);
    else if (e->pend.kind && e->pend.kind != PEND_BDOF)
        pend_close(e, c);
    if (!e->pend.kind) {
        e->pend.kind = PEND_BDOF; e->pend.n = 0; e->pend.bl2w = log2_pu_w; e->pend.bl2h = log2_pu_h;
        e->pend.bmv0 = mv0; e->pend.bmv1 = mv1; e->pend.bmv0.ref_idx = (int8_t)ref_idx0; e->pend.bmv1.ref_idx = (int8_t)ref_idx1;
        e->pend.ref_idx0 = ref_idx0; e->pend.ref_idx1 = ref_idx1;
    }
    e->pend.bx[e->pend.n] = x0; e->pend.by[e->pend.n] = y0; e->pend.n++;
}

/* rcn_dmvr_mv_refine (rcn_structures.h:628-632; rcn_inter.c:872-1126).
 *
 * The `OVMV *mv0, *mv1` in/out contract: the reference refines synchronously and its caller copies the result into the
 * CTU's TMVP storage (vcl_coding_unit.c:2629-2645), which store_inter_maps moves into the picture's MV plane at the end
 * of the CTU (drv_lines.c:270-330).  Here the search runs on the device at the end of the CTU ROW (the
 * alf.rcn_alf_filter_line hook below -> ovhip_job_dmvr_rows): the slot returns the vectors unrefined and remembers
 * where the caller's stores end up in the picture's MV plane; the hook patches those entries BEFORE the row is published
 * (ovdpb_report_decoded_ctu_line, slicedec.c:940-955), so every reader of the collocated motion field (tmvp of later
 * pictures, drv_mvp.c:281-345) sees refined vectors exactly when the reference guarantees them. */
static uint8_t
hip_rcn_dmvr_mv_refine(OVCTUDec *const c, struct OVBuffInfo dst, uint8_t x0, uint8_t y0, uint8_t log2_pu_w, uint8_t log2_pu_h,
                       OVMV *mv0, OVMV *mv1, uint8_t ref_idx0, uint8_t ref_idx1, uint8_t apply_bdof)
{
    (void)dst;
    struct hip_entry *e = entry_of(c, 0);
    PROF(e);
    if (!e || !e->rec) return 0;
    e->aff_c_live = 0;
    if (e->pend.kind) pend_close(e, c);
    ovhip_pu_desc d;
    fill_pu_idx(e, c, &d, x0, y0, log2_pu_w, log2_pu_h, 3, *mv0, *mv1, ref_idx0, ref_idx1);
    d.refine = OVHIP_PU_DMVR | (apply_bdof ? OVHIP_PU_BDOF : 0);
    size_t n_before = 0, n_after = 0;
    ovhip_rec_mcx_units(e->rec, &n_before);
    int r = ovhip_rec_pu(e->rec, &d);
    latch(e, r, "ovhip_rec_pu(dmvr)");
    ovhip_rec_mcx_units(e->rec, &n_after);
    if (r < 0 || n_after != n_before + 1) return 0;
    /* where the unit's vectors live in the picture's TMVP planes (8x8 grid) is derived on the device from the unit itself
     * (ovhip_tmvp_cells_launch: the caller writes tmvp_mv[l].mvs[((x0 + 7) >> 3) + ((y0 + 7) >> 3) * 16] and its right / lower
     * neighbours for 16-wide / 16-high blocks, tmvp_store_mv copies row i of that array to plane->mvs + ctb_offset + i * pln_stride);
     * r2 kept eight host pointers per unit here */
    e->n_refined = n_after;
    return 0;      /* disable_bdof: unused by the caller (vcl_coding_unit.c:2621) */
}
/* Eager DMVR, one step per row-end hook.  decode_ctu_line reports row y - 1 after row y has been parsed (slicedec.c:934-956), and
 * every reader of the collocated motion field (TMVP of later pictures, drv_mvp.c:281-345) must find refined vectors in a reported
 * row.  So: collect the pass enqueued at the end of the row before (search + vectors + plane entries: one asynchronous D2H each, it
 * ran while this row was parsed), patch the planes, enqueue the pass over the row just parsed.  The last row, and rows no hook ran
 * after, are refined synchronously.  ovhip_frame_dmvr_rows_begin waits for the picture's references on the host the first time a
 * row holds a DMVR unit (rcn_inter_synchronization waits per block, rcn_inter.c:131-146). */
static void
rows_step(struct hip_entry *e, OVCTUDec *c, int final)
{
    if (!e->fr || e->err) return;
    const size_t now = e->n_refined;
    if (now == e->dmvr_done) { e->row_mark = now; return; }
    /* what the decoder reports after this hook: the rows parsed before the hook before it -- at the picture's end, everything */
    const int64_t done = refine_now(e, c, final ? now : e->row_mark, 0);
    if (e->err) return;
    if (!final && now > (size_t)done) {
        PROF_DEVICE_BEGIN(e);
        const int64_t r = ovhip_frame_dmvr_rows_begin(e->fr, e->log2_ctu);
        PROF_DEVICE_END(e);
        if (r < 0) latch(e, (int)r, "ovhip_frame_dmvr_rows_begin");
    }
    e->row_mark = now;
}

void mode_row(struct hip_entry *e, OVCTUDec *c) { rows_step(e, c, 0); }
void mode_end(struct hip_entry *e, OVCTUDec *c) { rows_step(e, c, 1); }
void mode_begin(struct hip_entry *e) { e->pend.kind = PEND_NONE; e->aff_c_live = 0; }          /* no CU is being stitched */

void
mode_install(struct RCNFunctions *f)
{
    f->rcn_mcp_b_l = &hip_rcn_mcp_b_l;
    f->rcn_mcp_b_c = &hip_rcn_mcp_b_c;
    f->rcn_prof_mcp_b_l = &hip_rcn_prof_mcp_b_l;
    f->rcn_bdof_mcp_l = &hip_rcn_bdof_mcp_l;
    f->rcn_dmvr_mv_refine = &hip_rcn_dmvr_mv_refine;
}
