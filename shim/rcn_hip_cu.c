/* rcn_hip_cu.c -- caller mode of the override block for a reference with shim/caller.patch applied (rcn_hip.h, rcn_hip_priv.h; the
 * other mode: rcn_hip_sub.c).  The caller hands over whole coding units -- nothing to stitch -- and lets the back-end make the CTU-row
 * reports: the row step never waits for a reference picture, reports are held back until their rows' vectors are refined, and the
 * picture's last hook works through what is left row by row. */
#include "rcn_hip_priv.h"

#define MV_POS(xu, yu) (35 + (xu) + (yu) * 34)          /* PB_POS_IN_BUF, rcn_df.c:1524 */

/* rcn_cu_inter_b (shim/caller.patch): a bi-predicted coding unit with BDOF and / or DMVR, where the unpatched caller makes one
 * rcn_bdof_mcp_l / rcn_dmvr_mv_refine call per <= 16x16 block and one rcn_mcp_b_c call (vcl_coding_unit.c:2450-2472, :2598-2668).
 * The recorder cuts it the same way (ovhip_rec_cu_inter -> rec_pu_refined).  DMVR: the caller stores nothing into its collocated
 * motion arrays here (the unrefined vectors drv_merge_mvp_b wrote stay); the refined ones are patched into the picture's planes by
 * the row-end hooks, exactly as on the unpatched path (rows_step below). */
static void
hip_rcn_cu_inter_b(OVCTUDec *const c, const OVMV mv0, const OVMV mv1, unsigned int x0, unsigned int y0, unsigned int log2_cb_w,
                   unsigned int log2_cb_h, uint8_t inter_dir, uint8_t ref_idx0, uint8_t ref_idx1, uint8_t refine)
{
    ENTER(c);
    ovhip_pu_desc d;
    fill_pu_idx(e, c, &d, x0, y0, log2_cb_w, log2_cb_h, inter_dir, mv0, mv1, ref_idx0, ref_idx1);
    d.refine = (uint8_t)(((refine & 1) ? OVHIP_PU_BDOF : 0) | ((refine & 2) ? OVHIP_PU_DMVR : 0));
    const int r = ovhip_rec_cu_inter(e->rec, &d, NULL);
    latch(e, r, "ovhip_rec_cu_inter");
    if (r >= 0 && (refine & 2)) { size_t n = 0; ovhip_rec_mcx_units(e->rec, &n); e->n_refined = n; }
}

/* rcn_affine_cu (shim/caller.patch): an affine coding unit, where the unpatched drivers make one rcn_mcp_b_l / rcn_prof_mcp_b_l call
 * per 4x4 luma block and one rcn_mcp_b_c call per 8x8 luma area (drv_affine_mvp.c:3264-3411): the sub-block motion field is read
 * where the driver left it (inter_ctx->mv_ctx0 / mv_ctx1, 34 vectors per row). */
static void
hip_rcn_affine_cu(OVCTUDec *const c, struct InterDRVCtx *const ic, uint8_t x0, uint8_t y0, uint8_t log2_cu_w, uint8_t log2_cu_h,
                  uint8_t inter_dir, uint8_t prof_dir, const struct PROFInfo *const prof)
{
    ENTER(c);
    const int cols = (1 << log2_cu_w) >> 2, rows = (1 << log2_cu_h) >> 2;
    const OVMV *b0 = &ic->mv_ctx0.mvs[MV_POS(x0 >> 2, y0 >> 2)], *b1 = &ic->mv_ctx1.mvs[MV_POS(x0 >> 2, y0 >> 2)];
    for (int i = 0; i < rows; ++i)
        for (int j = 0; j < cols; ++j) {
            const int k = (i * 32 + j) * 2;
            e->pend.mv0[k] = b0[i * 34 + j].x; e->pend.mv0[k + 1] = b0[i * 34 + j].y;
            e->pend.mv1[k] = b1[i * 34 + j].x; e->pend.mv1[k + 1] = b1[i * 34 + j].y;
        }
    ovhip_affine_desc d;
    fill_affine(e, c, &d, x0, y0, log2_cu_w, log2_cu_h, inter_dir, b0->bcw_idx_plus1, prof_dir, (uint8_t)b0->ref_idx, (uint8_t)b1->ref_idx, prof);
    latch(e, ovhip_rec_cu_inter(e->rec, NULL, &d), "ovhip_rec_cu_inter(affine)");
}

/* the five slots only the unpatched callers reach (sub-block calls of affine / BDOF / DMVR coding units), and the CU they would collect */
static void
hip_unreached(OVCTUDec *const c, const char *slot)
{
    struct hip_entry *e = entry_of(c, 0);
    if (e) latch(e, OVHIP_EINVAL, slot);
}
void pend_close(struct hip_entry *e, OVCTUDec *c) { (void)c; e->pend.kind = PEND_NONE; latch(e, OVHIP_EINVAL, "sub-block calls collected under a patched caller"); }
static void hip_rcn_mcp_b_l(OVCTUDec *const c, struct OVBuffInfo dst, struct InterDRVCtx *const ic, const OVPartInfo *const part_ctx, const OVMV mv0,
                            const OVMV mv1, unsigned int x0, unsigned int y0, unsigned int l2w, unsigned int l2h, uint8_t dir, uint8_t r0, uint8_t r1)
{ (void)dst; (void)ic; (void)part_ctx; (void)mv0; (void)mv1; (void)x0; (void)y0; (void)l2w; (void)l2h; (void)dir; (void)r0; (void)r1; hip_unreached(c, "rcn_mcp_b_l called by a patched caller"); }
static void hip_rcn_mcp_b_c(OVCTUDec *const c, struct OVBuffInfo dst, struct InterDRVCtx *const ic, const OVPartInfo *const part_ctx, const OVMV mv0,
                            const OVMV mv1, unsigned int x0, unsigned int y0, unsigned int l2w, unsigned int l2h, uint8_t dir, uint8_t r0, uint8_t r1)
{ (void)dst; (void)ic; (void)part_ctx; (void)mv0; (void)mv1; (void)x0; (void)y0; (void)l2w; (void)l2h; (void)dir; (void)r0; (void)r1; hip_unreached(c, "rcn_mcp_b_c called by a patched caller"); }
static void hip_rcn_prof_mcp_b_l(OVCTUDec *const c, struct OVBuffInfo dst, struct InterDRVCtx *const ic, const OVPartInfo *const part_ctx, const OVMV mv0,
                                 const OVMV mv1, unsigned int x0, unsigned int y0, unsigned int l2w, unsigned int l2h, uint8_t dir, uint8_t r0, uint8_t r1,
                                 uint8_t prof_dir, const struct PROFInfo *const prof)
{ (void)dst; (void)ic; (void)part_ctx; (void)mv0; (void)mv1; (void)x0; (void)y0; (void)l2w; (void)l2h; (void)dir; (void)r0; (void)r1; (void)prof_dir; (void)prof; hip_unreached(c, "rcn_prof_mcp_b_l called by a patched caller"); }
static void hip_rcn_bdof_mcp_l(OVCTUDec *const c, struct OVBuffInfo dst, uint8_t x0, uint8_t y0, uint8_t l2w, uint8_t l2h, OVMV mv0, OVMV mv1, uint8_t r0, uint8_t r1)
{ (void)dst; (void)x0; (void)y0; (void)l2w; (void)l2h; (void)mv0; (void)mv1; (void)r0; (void)r1; hip_unreached(c, "rcn_bdof_mcp_l called by a patched caller"); }
static uint8_t hip_rcn_dmvr_mv_refine(OVCTUDec *const c, struct OVBuffInfo dst, uint8_t x0, uint8_t y0, uint8_t l2w, uint8_t l2h, OVMV *mv0, OVMV *mv1,
                                      uint8_t r0, uint8_t r1, uint8_t apply_bdof)
{ (void)dst; (void)x0; (void)y0; (void)l2w; (void)l2h; (void)mv0; (void)mv1; (void)r0; (void)r1; (void)apply_bdof; hip_unreached(c, "rcn_dmvr_mv_refine called by a patched caller"); return 0; }

/* With the caller patch the back-end owns the CTU-row reports (rcn_report_ctu_line), so the parse does NOT stop at the first row that
 * holds a DMVR unit until every reference picture has been reconstructed: a row pass is started only when the references are complete
 * (ovhip_frame_refs_ready never waits for a decode), the reports of rows whose vectors are not final yet are queued, and every later
 * hook -- and the picture's last one, which does wait -- issues what has become final.  The parse of a picture then overlaps the
 * reconstruction of its reference pictures, as the reference's row-granular synchronisation lets it (rcn_inter.c:131-146): the frame
 * threads' critical path is no longer the SUM of the parses along the GOP's dependency chain. */
static void
issue_reports(struct hip_entry *e, int all)
{
    int k = 0;
    while (k < e->n_reports && (all || e->reports[k].need <= e->dmvr_done)) {
        ovdpb_report_decoded_ctu_line(e->reports[k].pic, e->reports[k].y, e->reports[k].x0, e->reports[k].x1);
        ++k;
    }
    if (k) { memmove(e->reports, e->reports + k, (size_t)(e->n_reports - k) * sizeof(e->reports[0])); e->n_reports -= k; }
}

static int g_blocking_rows;          /* OVVC_HIP_BLOCKING_ROWS: the decoder reports its rows itself, every row hook waits (the A / B of the above) */

static void
rows_step(struct hip_entry *e, OVCTUDec *c, int final)
{
    if (!e->fr) return;
    final |= g_blocking_rows;
    /* the report(s) that follow this hook publish the rows parsed before the PREVIOUS hook ran: their refined units */
    e->report_need = e->row_mark;
    const size_t now = e->n_refined;
    if (!e->err && now != e->dmvr_done) {
        if (final) {
            (void)refine_now(e, c, now, 0);          /* waits for the reference pictures */
        } else {
            PROF_DEVICE_BEGIN(e);
            /* (a pass in flight began when its references were complete: this waits for device time only) */
            int64_t done = ovhip_frame_dmvr_rows_collect(e->fr);
            if (done >= 0 && (size_t)done < now) {
                const int ready = ovhip_frame_refs_ready(e->fr);
                if (ready < 0) done = ready;
                else if (ready) {
                    done = ovhip_frame_dmvr_rows_begin(e->fr, e->log2_ctu);
                    if (done >= 0) done = (int64_t)e->dmvr_done;          /* collected by the next hook */
                }
            }
            PROF_DEVICE_END(e);
            apply_done_cells(e, c, done);
        }
    }
    e->row_mark = now;
    issue_reports(e, e->err != 0 || final);        /* (a failed picture's rows are reported: nobody may hang on it) */
}

/* rcn_report_ctu_line (shim/caller.patch; slicedec.c:934-956, :1058-1073): the decoder's ovdpb_report_decoded_ctu_line, made when the
 * row's collocated motion vectors are final -- at once in pictures without DMVR units and whenever the device has already answered */
static void
hip_rcn_report_ctu_line(OVCTUDec *const c, OVPicture *const pic, int y_ctu, int xmin_ctu, int xmax_ctu)
{
    struct hip_entry *e = entry_of(c, 0);
    if (!e || e->record_only || !e->fr || e->err || (!e->n_reports && e->report_need <= e->dmvr_done)
        || e->n_reports == (int)(sizeof(e->reports) / sizeof(e->reports[0]))) {
        if (e && e->n_reports) { rows_step(e, c, 1); issue_reports(e, 1); }       /* (queue full: wait, as the unpatched path does) */
        ovdpb_report_decoded_ctu_line(pic, y_ctu, xmin_ctu, xmax_ctu);
        return;
    }
    e->reports[e->n_reports].pic = pic; e->reports[e->n_reports].y = y_ctu; e->reports[e->n_reports].x0 = xmin_ctu; e->reports[e->n_reports].x1 = xmax_ctu;
    e->reports[e->n_reports].need = e->report_need;
    e->n_reports++; e->n_reports_deferred++;
}

/* The picture's last hook, when its parse ran AHEAD of its reference pictures (with the caller patch the parse never waits for a
 * reference: the rows' reports were queued, their bands left to later hooks).  Instead of waiting for the reference pictures to be
 * complete and then doing everything at once, the rows are worked through in order as the references' rows arrive (ovhip_dpb_rows_tag
 * blocks per row): the DMVR vectors of the row's units, the row's report (its readers' parse goes on), the row's band (its readers'
 * bands go on) -- so that a chain of pictures that each trail their references by a few rows stays a chain of a few rows per link,
 * whatever the parse speeds (rcn_inter.c:131-146 + dpb.c:1309-1323 give the reference's frame threads the same behaviour). */
static void
final_progressive(struct hip_entry *e, OVCTUDec *c)
{
    if (!e->band_on || !e->fr || e->err || !e->n_refs) return;
    ovhip_job_params pr;
    picture_params(e, c, &pr, 1);
    for (int y = e->rows_sent; y < e->n_marks && !e->err; ++y) {
        const size_t units = e->marks[y].n_refined;
        if (units > e->dmvr_done) (void)refine_now(e, c, units, 1);          /* waits for the rows these units read */
        issue_reports(e, 0);
        if ((y + 1) % g_band_rows == 0 && !e->err) {
            PROF_DEVICE_BEGIN(e);
            const int r = ovhip_frame_band_upto(e->fr, &pr, (y + 1) << e->log2_ctu, &e->marks[y].counts, 1);
            PROF_DEVICE_END(e);
            if (r < 0) latch(e, r, "ovhip_frame_band_upto");
            else { e->n_bands_sent++; e->rows_sent = y + 1; }
        }
    }
}

void mode_row(struct hip_entry *e, OVCTUDec *c) { rows_step(e, c, 0); }
void mode_end(struct hip_entry *e, OVCTUDec *c) { final_progressive(e, c); rows_step(e, c, 1); }

void
mode_begin(struct hip_entry *e)
{
    if (e->n_reports) issue_reports(e, 1);             /* (a picture that never reached its last row: its readers must not hang) */
    e->report_need = 0;
}

void
mode_install(struct RCNFunctions *f)
{
    f->rcn_mcp_b_l = &hip_rcn_mcp_b_l;
    f->rcn_mcp_b_c = &hip_rcn_mcp_b_c;
    f->rcn_prof_mcp_b_l = &hip_rcn_prof_mcp_b_l;
    f->rcn_bdof_mcp_l = &hip_rcn_bdof_mcp_l;
    f->rcn_dmvr_mv_refine = &hip_rcn_dmvr_mv_refine;
    f->rcn_cu_inter_b = &hip_rcn_cu_inter_b;
    f->rcn_affine_cu = &hip_rcn_affine_cu;
    g_blocking_rows = getenv("OVVC_HIP_BLOCKING_ROWS") != NULL;
    f->rcn_report_ctu_line = g_blocking_rows ? NULL : &hip_rcn_report_ctu_line;      /* (NULL: the decoder reports by itself, the row hooks wait) */
}
