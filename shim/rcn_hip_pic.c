/* rcn_hip_pic.c -- the picture's progress on the device (rcn_hip.h, rcn_hip_priv.h): begin, the refined vectors of the rows parsed so
 * far, bands, the end of the picture, and the output entry points.  What happens when a CTU row has been parsed is decided in
 * rows_parsed(); how long it may wait for reference pictures is the caller mode's part (rcn_hip_sub.c / rcn_hip_cu.c). */
#include "rcn_hip_priv.h"

/* Entries of the picture's collocated motion planes as the device derived them (ovhip_job_tmvp_cells: 4 per refined unit, cell =
 * index into MVPlane.mvs, OVHIP_TMVP_NONE = unused / not a DMVR unit / outside what tmvp_store_mv copies): x and y of both lists. */
int
ovhip_shim_apply_tmvp_cells(OVCTUDec *c, const ovhip_tmvp_cell *cells, size_t n_entries)
{
    if (!c || (!cells && n_entries)) return OVHIP_EINVAL;
    const struct InterDRVCtx *ic = &c->drv_ctx.inter_ctx;
    const struct MVPlane *pl0 = ic->tmvp_ctx.plane0, *pl1 = ic->tmvp_ctx.plane1;
    if (!pl0 || !pl1 || !pl0->mvs || !pl1->mvs) return OVHIP_OK;         /* the picture keeps no motion field */
#ifdef OVVC_HIP_DEBUG_TMVP          /* debug scaffolding: compiled out of the product (it used to getenv() in every row hook) */
    {
        size_t nz = 0, nn = 0;
        for (size_t i = 0; i < n_entries; ++i) { nn += cells[i].cell != OVHIP_TMVP_NONE; nz += cells[i].cell != OVHIP_TMVP_NONE && !cells[i].mv0x && !cells[i].mv0y && !cells[i].mv1x && !cells[i].mv1y; }
        fprintf(stderr, "    tmvp patch ctudec %p: %zu entries, %zu used, %zu of them all-zero; first used:", (void *)c, n_entries, nn, nz);
        for (size_t i = 0, k = 0; i < n_entries && k < 3; ++i) if (cells[i].cell != OVHIP_TMVP_NONE) { fprintf(stderr, " [%u: %d %d %d %d]", cells[i].cell, cells[i].mv0x, cells[i].mv0y, cells[i].mv1x, cells[i].mv1y); ++k; }
        fprintf(stderr, "\n");
    }
#endif
    for (size_t i = 0; i < n_entries; ++i) {
        const ovhip_tmvp_cell *q = &cells[i];
        if (q->cell == OVHIP_TMVP_NONE) continue;
        pl0->mvs[q->cell].x = q->mv0x; pl0->mvs[q->cell].y = q->mv0y;
        pl1->mvs[q->cell].x = q->mv1x; pl1->mvs[q->cell].y = q->mv1y;
    }
    return OVHIP_OK;
}

/* the eager DMVR passes have refined `done` units so far (< 0: failed): the vectors not yet in the collocated planes go there */
void
apply_done_cells(struct hip_entry *e, OVCTUDec *c, int64_t done)
{
    if (done < 0) { latch(e, (int)done, "ovhip_frame_dmvr_rows"); return; }
    if ((size_t)done <= e->dmvr_done) return;
    size_t n = 0;
    ovhip_job *job = ovhip_frame_job(e->fr);                 /* (NULL: a dry frame -- nothing computes, nothing to patch) */
    const ovhip_tmvp_cell *cells = job ? ovhip_job_tmvp_cells(job, &n) : NULL;
    if (job && (!cells || n < 4 * (size_t)done)) { latch(e, OVHIP_EINVAL, "the eager DMVR pass delivered no collocated-motion entries"); return; }
    if (cells) ovhip_shim_apply_tmvp_cells(c, cells + 4 * e->dmvr_done, 4 * ((size_t)done - e->dmvr_done));
    e->dmvr_done = (size_t)done;
}

/* Refine up to `need` units NOW: collect the pass in flight; where it did not reach them, run one over everything recorded (exact: over
 * `need` units, which waits only for the reference rows those read) and collect it too.  Both wait: ovhip_frame_dmvr_rows_begin for
 * the picture's references the first time a DMVR unit turns up (rcn_inter_synchronization waits per block, rcn_inter.c:131-146). */
int64_t
refine_now(struct hip_entry *e, OVCTUDec *c, size_t need, int exact)
{
    PROF_DEVICE_BEGIN(e);
    int64_t done = ovhip_frame_dmvr_rows_collect(e->fr);
    if (done >= 0 && (size_t)done < need) {
        done = exact ? ovhip_frame_dmvr_rows_begin_upto(e->fr, e->log2_ctu, need) : ovhip_frame_dmvr_rows_begin(e->fr, e->log2_ctu);
        if (done >= 0) done = ovhip_frame_dmvr_rows_collect(e->fr);
    }
    PROF_DEVICE_END(e);
    apply_done_cells(e, c, done);
    return done;
}

/* ------------------------------------------------------------------------------------ picture begin / flush / plumbing */
/* The device half lives in libovvc_hip.so (ovvc_dpb.c, ovvc_frame.c): a process-wide device DPB keyed by the OVFrame pointer and
 * one ovhip_frame (context + job) per OVCTUDec.  This file only maps the decoder's events onto it:
 *   rcn_attach_frame_buff            -> ovhip_frame_begin(frame)
 *   first use of a reference picture -> ovhip_frame_ref(ref->frame)          (ref_slot above)
 *   the row hooks, per row           -> ovhip_frame_dmvr_rows (the caller mode's row step), ovhip_frame_band
 *   ... of the picture's last row    -> ovhip_frame_submit: uploads, wait for the references, launches, ovhip_job_wait, publish, output
 *   latched error                    -> ovhip_frame_fail: the picture's readers are released with an error, nobody hangs
 * Devices: OVVC_HIP_DEVICES="0,1,..." (default: OVVC_HIP_DEVICE or 0).  Frame thread k decodes on device k mod N -- pictures shard
 * one per GPU as the sub-decoders take them (ovdec_select_subdec, ovdec.c:188-248); a reference picture decoded on another device
 * arrives by an event-ordered peer copy the DPB starts as soon as it is done. */
static ovhip_dpb *g_dpb;
static int g_n_dev = 1, g_next_dev, g_n_entries, g_out_mode = OVHIP_OUT_PLANES, g_dpb_external;
static ovhip_ctx *g_out_ctx[OVHIP_MAX_DEVICES];
static pthread_mutex_t g_dpb_mtx = PTHREAD_MUTEX_INITIALIZER;

static int
dpb_get(struct hip_entry *e)
{
    int r = OVHIP_OK;
    pthread_mutex_lock(&g_dpb_mtx);
    if (!g_dpb) {
        int devs[OVHIP_MAX_DEVICES], n = 0;
        const char *list = getenv("OVVC_HIP_DEVICES"), *one = getenv("OVVC_HIP_DEVICE"), *om = getenv("OVVC_HIP_OUTPUT");
        if (list) { for (const char *p = list; *p && n < OVHIP_MAX_DEVICES;) { devs[n++] = atoi(p); while (*p && *p != ',') ++p; if (*p) ++p; } }
        if (!n) devs[n++] = one ? atoi(one) : 0;
        /* OVVC_HIP_OUTPUT=none: the application takes its frames through ovhip_shim_frame_output / _digest and the 24.9 MB copy of
         * every 4K picture into the OVFrame is skipped; default: the OVFrame is filled, an unmodified dectest.c:372-409 works */
        if (om && !strcmp(om, "none")) g_out_mode = OVHIP_OUT_NONE;
        r = ovhip_dpb_create(&g_dpb, devs, n);
        if (r == OVHIP_OK) g_n_dev = n; else g_dpb = NULL;
    }
    if (r == OVHIP_OK && e->dev < 0) { e->dev = g_next_dev++ % g_n_dev; g_n_entries++; }
    pthread_mutex_unlock(&g_dpb_mtx);
    return r;
}

/* The application owns the device DPB (several decoders sharing one; a test back-end made with ovhip_dpb_create_ex): call before the
 * first picture.  NULL: back to the DPB the shim creates itself from OVVC_HIP_DEVICES. */
void
ovhip_shim_set_dpb(struct ovhip_dpb *dpb)
{
    pthread_mutex_lock(&g_dpb_mtx);
    g_dpb = dpb; g_dpb_external = dpb != NULL;
    g_n_dev = dpb ? ovhip_dpb_n_devices(dpb) : 1;
    g_next_dev = 0;
    pthread_mutex_unlock(&g_dpb_mtx);
}

void ovhip_shim_set_output(int mode) { g_out_mode = mode == OVHIP_OUT_NONE ? OVHIP_OUT_NONE : OVHIP_OUT_PLANES; }

/* The host DPB dropped its last reference to the frame (ovframe_unref reaching zero): the device picture goes back to the pool.
 * Frees device memory earlier; not needed for correctness -- a frame pointer that comes back for a new picture recycles its slot,
 * and readers name the picture they mean by its tag (pic_tag above), so a slot that still shows the previous owner of the
 * OVFrame is waited past, never read. */
void ovhip_shim_frame_released(const OVFrame *frame) { if (g_dpb && frame) (void)ovhip_dpb_release(g_dpb, frame); }

/* Output path: what examples/dectest.c:372-409 (write_decoded_frame_to_file) copies out of the OVFrame plane by plane, taken
 * from the device picture of that frame instead -- cropped to frame->output_window and packed by one launch, fetched with
 * one D2H; or only fingerprinted (MD5 over the per-row MD5 digests computed on the device), nothing but 16 bytes leaving. */
static ovhip_window
frame_window(const OVFrame *f)
{
    ovhip_window w = { f->output_window.offset_lft, f->output_window.offset_rgt, f->output_window.offset_abv, f->output_window.offset_blw };
    return w;
}

static ovhip_ctx *
out_ctx_of(const OVFrame *frame, ovhip_pic *pic)
{
    int dev = 0;
    if (!g_dpb || !frame || ovhip_dpb_lookup(g_dpb, frame, &dev, pic) != OVHIP_OK) return NULL;
    pthread_mutex_lock(&g_dpb_mtx);
    if (!g_out_ctx[dev] && ovhip_ctx_create(&g_out_ctx[dev], ovhip_dpb_device(g_dpb, dev), NULL) != OVHIP_OK) g_out_ctx[dev] = NULL;
    ovhip_ctx *ctx = g_out_ctx[dev];
    pthread_mutex_unlock(&g_dpb_mtx);
    return ctx;
}

size_t
ovhip_shim_frame_bytes(const OVFrame *frame)
{
    const ovhip_window w = frame_window(frame);
    return ovhip_output_bytes(frame->width, frame->height, &w);
}

/* (one application thread at a time per device: the output contexts are not locked) */
int
ovhip_shim_frame_output(const OVCTUDec *c, const OVFrame *frame, void *dst)
{
    (void)c;
    ovhip_pic pic;
    ovhip_ctx *ctx = dst ? out_ctx_of(frame, &pic) : NULL;
    if (!ctx) return OVHIP_EINVAL;
    const ovhip_window w = frame_window(frame);
    return ovhip_pic_output(ctx, &pic, &w, dst);
}

int
ovhip_shim_frame_digest(const OVCTUDec *c, const OVFrame *frame, uint8_t out[16])
{
    (void)c;
    ovhip_pic pic;
    ovhip_ctx *ctx = out ? out_ctx_of(frame, &pic) : NULL;
    if (!ctx) return OVHIP_EINVAL;
    const ovhip_window w = frame_window(frame);
    return ovhip_pic_digest(ctx, &pic, &w, out);
}

/* The same at ONE output size, for a stream that changes its coded size: what pp_process_frame (post_proc.c:116-126, called at
 * ovdec.c:479 / :523 when the decoder's `upscale` option is on) does on the host with pp_sample_rate_conv, on the device picture instead.
 * scale_info = the picture's own (pic->scale_info), out_w x out_h = the frame pool's size.  The whole resampled frame is delivered: the
 * frame's output_window describes the coded picture, and the reference's post-processed frame does not carry it over (post_proc.c:89-129). */
static ovhip_scale_info
scale_info_of(const struct ScalingInfo *si)
{
    ovhip_scale_info o;
    memset(&o, 0, sizeof(o));
    if (si) {
        o.win_left = si->scaling_win_left; o.win_right = si->scaling_win_right;
        o.win_top = si->scaling_win_top; o.win_bottom = si->scaling_win_bottom;
        o.chroma_hor_col = si->chroma_hor_col_flag; o.chroma_ver_col = si->chroma_ver_col_flag;
    }
    return o;
}

size_t
ovhip_shim_frame_bytes_scaled(const OVFrame *frame, int out_w, int out_h)
{
    (void)frame;
    return ovhip_output_bytes(out_w, out_h, NULL);
}

int
ovhip_shim_frame_output_scaled(const OVCTUDec *c, const OVFrame *frame, const struct ScalingInfo *scale_info, int out_w, int out_h, void *dst)
{
    (void)c;
    ovhip_pic pic;
    ovhip_ctx *ctx = dst ? out_ctx_of(frame, &pic) : NULL;
    if (!ctx) return OVHIP_EINVAL;
    const ovhip_scale_info si = scale_info_of(scale_info);
    return ovhip_pic_output_scaled(ctx, &pic, &si, out_w, out_h, NULL, dst);
}

int
ovhip_shim_frame_digest_scaled(const OVCTUDec *c, const OVFrame *frame, const struct ScalingInfo *scale_info, int out_w, int out_h, uint8_t out[16])
{
    (void)c;
    ovhip_pic pic;
    ovhip_ctx *ctx = out ? out_ctx_of(frame, &pic) : NULL;
    if (!ctx) return OVHIP_EINVAL;
    const ovhip_scale_info si = scale_info_of(scale_info);
    return ovhip_pic_digest_scaled(ctx, &pic, &si, out_w, out_h, NULL, out);
}

/* picture-level side information of the flush / of a band.  by_flags: the filters are on when the slice says so (a band is submitted
 * before every row's hooks have run; the parameter arrays hold what the hooks have delivered, which is what the band's filters reach) */
void
picture_params(struct hip_entry *e, OVCTUDec *c, ovhip_job_params *pr, int by_flags)
{
    memset(pr, 0, sizeof(*pr));
    pr->lmcs = (c->lmcs_info.lmcs_enabled_flag && e->have_luts) ? &e->luts : NULL;
    const struct ALFInfo *ai = &c->alf_info;
    const int sao_on = by_flags ? (c->sao_info.sao_luma_flag || c->sao_info.sao_chroma_flag) && e->sao : e->sao_on;
    const int alf_on = by_flags ? (ai->alf_luma_enabled_flag || ai->alf_cb_enabled_flag || ai->alf_cr_enabled_flag) && e->alf : e->alf_on;
    pr->sao = sao_on ? e->sao : NULL;
    if (alf_on) {
        const RCNALF *ra = &c->alf_info.rcn_alf;
        if (by_flags) alf_cc_capture(e, ai);
        pr->alf_ctus = e->alf;
        pr->alf_luma_coeff = &ra->filter_coeff_dec[0][0]; pr->alf_luma_clip = &ra->filter_clip_dec[0][0];
        pr->alf_chroma_coeff = &ra->chroma_coeff_final[0][0]; pr->alf_chroma_clip = &ra->chroma_clip_final[0][0];
        pr->alf_cc_coeff = &e->alf_cc[0][0][0];
    }
    pr->log2_ctu_s = e->log2_ctu;
}

/* Band-wise submission (ovhip_frame_band; OVVC_HIP_BANDS = CTU rows per band; 0 = off, the DEFAULT: measured on the live decoder at 4K
 * -- DESIGN 12 -- whole-picture submission is faster at every band size: a band is ~13 launches, a picture of 17 bands ~220 instead of
 * 11, and the host side of a launch is what a frame thread's device half consists of): at the end of every g_band_rows-th CTU row
 * what has been recorded since the last band goes to the device -- upload, prediction, residuals, ordered pass at once; the filters one
 * band late -- while the parse goes on; the rows the band's filters made final are posted to the device DPB, where the frame threads
 * that reference this picture see them (slicedec.c:815-975 + dpb.c:1309-1323 do this per CTU row on the host).  A band whose
 * reference rows are not there yet is left to the next hook; only the picture's end waits. */
int g_band_rows = 0;
static int g_band_rows_set, g_band_intra = 1, g_band_inter = 1;
/* CTU rows per band; 0: every picture is submitted at its end (ovhip_frame_submit).  Overrides OVVC_HIP_BANDS. */
void ovhip_shim_set_bands(int ctu_rows_per_band) { g_band_rows = ctu_rows_per_band < 0 ? 0 : ctu_rows_per_band; g_band_rows_set = 1; }
void
ovhip_shim_band_stats(const OVCTUDec *c, uint32_t *sent, uint32_t *deferred)
{
    struct hip_entry *e = entry_of(c, 0);
    if (sent) *sent = e ? e->n_bands_sent : 0;
    if (deferred) *deferred = e ? e->n_bands_deferred : 0;
}

void
pic_knobs(void)
{
    if (!g_band_rows_set && getenv("OVVC_HIP_BANDS")) g_band_rows = atoi(getenv("OVVC_HIP_BANDS"));
    if (getenv("OVVC_HIP_BANDS_INTRA")) g_band_intra = atoi(getenv("OVVC_HIP_BANDS_INTRA"));
    if (getenv("OVVC_HIP_BANDS_INTER")) g_band_inter = atoi(getenv("OVVC_HIP_BANDS_INTER"));
}

static void
band_step(struct hip_entry *e, OVCTUDec *c, const struct RectEntryInfo *einfo, int rows_parsed)
{
    if (!e->band_on || !e->fr || e->err || g_band_rows <= 0) return;
    if (rows_parsed >= 1 && rows_parsed <= MAX_MARKS && e->n_marks == rows_parsed - 1) {
        ovhip_rec_counts(e->rec, &e->marks[rows_parsed - 1].counts);
        e->marks[rows_parsed - 1].n_refined = e->n_refined;
        e->n_marks = rows_parsed;
    }
    if (rows_parsed % g_band_rows) return;
    /* the band's filters reach into the row just parsed: its ALF parameters (the row's own hook runs a row later, slicedec.c:934-956)
     * and, for row 0, the SAO parameters are there -- parsed with the row's CTUs */
    if (params_alloc(e, c, einfo)) return;
    for (int y = rows_parsed - g_band_rows; y < rows_parsed; ++y) alf_row(e, c, einfo, y);
    if (c->sao_info.sao_luma_flag || c->sao_info.sao_chroma_flag) sao_row(e, c, einfo, rows_parsed - 1);
    ovhip_job_params pr;
    picture_params(e, c, &pr, 1);
    PROF_DEVICE_BEGIN(e);
    const int r = ovhip_frame_band(e->fr, &pr, rows_parsed << e->log2_ctu, 0, NULL);
    PROF_DEVICE_END(e);
    if (r < 0) latch(e, r, "ovhip_frame_band");
    else if (r) { e->n_bands_sent++; e->rows_sent = rows_parsed; } else e->n_bands_deferred++;
}
static void
flush_picture(struct hip_entry *e, OVCTUDec *c)
{
    if (!e->fr) return;
    if (e->err) {
        /*  every exit path publishes: a picture that cannot be decoded releases its readers with an error */
        (void)ovhip_frame_fail(e->fr, e->err);
        return;
    }
    ovhip_job_params pr;
    picture_params(e, c, &pr, e->band_on);
    /* the decoder's own output path and any host-side reader expect the samples in the OVFrame (dectest.c:372-409): copied out
     * AFTER ovhip_job_wait (which may decode the picture a second time) and after the picture was published to its readers */
    ovhip_frame_output out;
    memset(&out, 0, sizeof(out));
    const OVFrame *f = e->frame;
    out.mode = g_out_mode;
    out.y = (uint16_t *)f->data[0]; out.cb = (uint16_t *)f->data[1]; out.cr = (uint16_t *)f->data[2];
    out.stride_y = (int32_t)(f->linesize[0] / 2); out.stride_c = (int32_t)(f->linesize[1] / 2);
    /* (every refined vector is in the TMVP planes already: mode_end ran before this) */
    PROF_DEVICE_BEGIN(e);
    if (e->band_on) { const int r = ovhip_frame_band(e->fr, &pr, e->pic_h, 1, &out); latch(e, r < 0 ? r : OVHIP_OK, "ovhip_frame_band (last)"); e->n_bands_sent++; }
    else latch(e, ovhip_frame_submit(e->fr, NULL, NULL, &pr, &out), "ovhip_frame_submit");
    PROF_DEVICE_END(e);
}

/* The row hooks' one question (hip_sao_first_pix_rows, hip_alf_filter_line in rcn_hip_rec.c, their parameters captured): `rows` CTU
 * rows of the entry are parsed.  Not the last hook: the caller mode's row step makes the vectors of the rows about to be reported final
 * and starts the pass over the row just parsed; then the band that ends with this row, except the entry's last rows', which the flush
 * takes along.  The picture's last hook: everything final, every row reported, the picture flushed. */
void
rows_parsed(struct hip_entry *e, OVCTUDec *c, const struct RectEntryInfo *einfo, int rows, int last)
{
    if (e->record_only) return;
    if (last) { mode_end(e, c); flush_picture(e, c); return; }
    mode_row(e, c);
    if (rows < einfo->nb_ctu_h) band_step(e, c, einfo, rows);
}

void
begin_picture(struct hip_entry *e, const OVFrame *f, const struct RectEntryInfo *einfo)
{
    /* One device job = one picture.  A picture cut into rect entries (tiles; slicedec.c:636-657) attaches the frame once per entry:
     * the entries that follow the first on the SAME OVCTUDec (one entry thread: slicedec.c:649-653 runs them in turn) go on recording
     * into the picture's job, and the last one to end submits it (hip_alf_filter_line).  Entries of one picture on SEVERAL OVCTUDecs
     * (`-e 2`, ovthreads.c:93-114) would need their recorders merged: refused, the picture fails loudly. */
    int nw = 0, nh = 0, first = 1;
    e->whole_pic_entry = 1; e->entry_x0 = 0;
    if (einfo && e->key->part_ctx) {
        const int l2 = e->key->part_ctx->log2_ctu_s;
        const int pw = e->record_only ? e->pic_w : (int)f->width, ph = e->record_only ? e->pic_h : (int)f->height;
        nw = (pw + (1 << l2) - 1) >> l2; nh = (ph + (1 << l2) - 1) >> l2;
        first = !einfo->ctb_x && !einfo->ctb_y;
        e->entry_x0 = einfo->ctb_x << l2;
        e->whole_pic_entry = first && einfo->nb_ctu_w == nw && einfo->nb_ctu_h == nh;
    }
    if (!first) {
        if (e->frame != f || e->ctus_left <= 0 || !e->rec) {
            latch(e, OVHIP_EUNSUP, "rect entry of a picture whose first entry this OVCTUDec did not decode (entry threads > 1)");
            if (!e->record_only && e->fr) { ovhip_frame_destroy(e->fr); e->fr = NULL; e->rec = NULL; }
            return;
        }
        e->lmcs_region_live = 0;
        e->pend.kind = PEND_NONE; e->aff_c_live = 0; e->ciip.live = 0; e->ibc.live = 0;
        return;
    }
    e->frame = f;
    /* the CTU size is needed by the first row-end hook already (the row step -> the plane entries of the row's refined units): found by
     * the live decode on several frame threads -- a frame thread whose FIRST picture had DMVR units in CTU row 0 asked for the entries
     * with log2_ctu_s == 0, got none, and left that row's collocated motion vectors unrefined (params_alloc used to be the only writer) */
    if (e->key->part_ctx) e->log2_ctu = e->key->part_ctx->log2_ctu_s;
    e->ctus_left = nw * nh;
    e->err = 0;
    e->n_refs = 0;
    e->scale_set = 0;
    e->sao_on = e->alf_on = 0;
    e->lmcs_region_live = 0;
    e->n_refined = 0; e->dmvr_done = 0; e->row_mark = 0;
    mode_begin(e);
    e->ciip.live = 0; e->ibc.live = 0;
    if (e->rec && e->key->part_ctx) (void)ovhip_rec_set_ctu_size(e->rec, e->key->part_ctx->log2_ctu_s);
    if (e->n_ctu) { memset(e->sao, 0, e->n_ctu * sizeof(*e->sao)); memset(e->alf, 0, e->n_ctu * sizeof(*e->alf)); }
    if (e->record_only) { ovhip_rec_reset(e->rec); return; }
    PROF_DEVICE_BEGIN(e);
    int r = dpb_get(e);
    if (r != OVHIP_OK) { latch(e, r, "ovhip_dpb_create (the HIP back-end has no CPU fallback)"); return; }
    if (e->fr && (e->pic_w != (int)f->width || e->pic_h != (int)f->height)) { ovhip_frame_destroy(e->fr); e->fr = NULL; e->rec = NULL; }
    e->pic_w = f->width; e->pic_h = f->height;
    if (!e->fr) {
        r = ovhip_frame_create(g_dpb, e->dev, e->pic_w, e->pic_h, &e->fr);
        if (r != OVHIP_OK) { e->fr = NULL; latch(e, r, "ovhip_frame_create"); return; }
    }
    /* the OVPicture being decoded: tmvp_entry_init (slicedec.c:1085-1099, called before rcn_attach_frame_buff) left pointers to its
     * motion planes in the CTU decoder -- the table's prototypes never hand the picture itself over */
    const struct MVPlane *pl0 = e->key->drv_ctx.inter_ctx.tmvp_ctx.plane0;
    const OVPicture *cur = pl0 ? (const OVPicture *)((const char *)pl0 - offsetof(OVPicture, mv_plane0)) : NULL;
    latch(e, ovhip_frame_begin_tag(e->fr, f, cur && cur->frame == f ? pic_tag(cur) : 0), "ovhip_frame_begin");
    e->rec = ovhip_frame_recorder(e->fr);
    /* band by band: pictures of one rect entry.  (An I picture's ordered pass is one dependency chain per band, so its bands follow each
     * other on the device; ovhip_frame_band leaves a band to the next hook while the one before is still being reconstructed, so the
     * bands of a picture that is parsed faster than the device decodes it grow until the wavefront spans the rows again.)
     * OVVC_HIP_BANDS_INTRA=0: I pictures whole. */
    e->band_on = g_band_rows > 0 && e->whole_pic_entry && (e->key->tmp_slice_type == 2 ? g_band_intra : g_band_inter);
    e->n_marks = 0; e->rows_sent = 0;
    (void)ovhip_frame_set_band_mode(e->fr, e->band_on);
    PROF_DEVICE_END(e);
    if (!e->rec) { latch(e, OVHIP_ENOMEM, "ovhip_frame_recorder"); return; }
    (void)ovhip_rec_set_ctu_size(e->rec, e->key->part_ctx ? e->key->part_ctx->log2_ctu_s : 7);
    /* this caller submits through the picture job, which launches every array the recorder fills: affine CUs and lone 4x4 luma
     * blocks on scaled references are recorded instead of refused */
    (void)ovhip_rec_set_rpr_tools(e->rec, OVHIP_RPR_TOOL_AFFINE | OVHIP_RPR_TOOL_PU4x4);
    /* the slice's reference lists are known now (slicedec.c:1250-1256): a device that did not decode them asks for them before
     * the first prediction unit is parsed */
    const struct InterDRVCtx *ic = &e->key->drv_ctx.inter_ctx;
    if (g_n_dev > 1 && e->key->tmp_slice_type != 2) {
        for (int i = 0; i < ic->nb_active_ref0 && i < 16; ++i) if (ic->rpl0[i] && ic->rpl0[i]->frame) (void)ovhip_dpb_want_tag(g_dpb, ic->rpl0[i]->frame, pic_tag(ic->rpl0[i]), e->dev);
        for (int i = 0; i < ic->nb_active_ref1 && i < 16; ++i) if (ic->rpl1[i] && ic->rpl1[i]->frame) (void)ovhip_dpb_want_tag(g_dpb, ic->rpl1[i]->frame, pic_tag(ic->rpl1[i]), e->dev);
    }
}

/* the entry's OVCTUDec goes away (ovhip_shim_release): its frame thread, and with the last one of the process the device DPB (every
 * device picture) */
void
pic_release(struct hip_entry *e)
{
    if (e->fr) ovhip_frame_destroy(e->fr);
    pthread_mutex_lock(&g_dpb_mtx);
    if (e->dev >= 0 && --g_n_entries == 0 && g_dpb && !g_dpb_external) {
        for (int k = 0; k < OVHIP_MAX_DEVICES; ++k) if (g_out_ctx[k]) { ovhip_ctx_destroy(g_out_ctx[k]); g_out_ctx[k] = NULL; }
        ovhip_dpb_destroy(g_dpb);
        g_dpb = NULL; g_next_dev = 0;
    }
    pthread_mutex_unlock(&g_dpb_mtx);
}
