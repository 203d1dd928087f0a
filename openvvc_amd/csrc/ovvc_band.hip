// ovvc_band.hip -- the picture job, band by band (include/ovvc_hip.h "ovhip_job_band"); the whole-picture flush, the launch chain and the
// flow admission policy these bands share with it are in ovvc_picture.hip, the types both use in ovvc_job.hip.h.
//
// Band-wise submission: a picture enters the device while it is still being parsed.
//
// The reference reconstructs a CTU row right after parsing it and reports it (slicedec.c:815-975, dpb.c:1309-1323); a picture that
// references it runs a few rows behind (rcn_inter.c:131-146).  ovhip_job_flush takes a picture when its parse has ENDED, so every level
// of a GOP's reference hierarchy cost a whole parse plus a whole launch chain.  Here the recorder's arrays are cut at CTU-row bands:
//
//     ovhip_job_band(k)   = upload of band k's slices (ONE copy out of a staging block) + recon(k) + tail(k)
//     recon(k)            = MC -> refined / affine MC -> luma residual -> chroma-scale regions -> chroma residual -> ordered pass,
//                           the picture-wide launches over the band's slice of every list
//     tail(k)             = inverse luma mapping of the band's rows (+ un-tag) -> deblocking of the band's edge lists (V then H)
//                           -> SAO rows [.., s1) -> ALF rows [.., a1)
//
// The horizontal edge on the boundary between bands k - 1 and k belongs to band k's lists and changes up to 7 rows above it, so after
// tail(k) the rows < end_k - 8 are final for the deblocking; SAO then runs up to the last multiple of 8 rows below that (its edge
// classes read one row further), ALF up to the last multiple of 8 that keeps its 3-row reach and the classification windows inside the
// SAO output: s1 = end_k - 16, a1 = end_k - 24 for CTU-row bands (the tiles a window cuts are staged whole, rows outside it are not
// stored).  Intra prediction of band k + 1 reads the UNFILTERED, still mapped bottom row of band k (the reference keeps saved lines for
// this, rcn_ctu.c:246-510): k_band_row below sets it aside before tail(k) and puts it back for recon(k + 1).  Every launch reads exactly
// the samples the picture-wide launch reads, so the fixtures' parity carries over (tests/test_gpu_bands.py: bands of one CTU row, of
// two, of three and one band = the whole picture give identical pictures).
//
// Indices inside the commands (coefficient / side-arena offsets, region numbers) stay what the recorder wrote: the band's slice is
// addressed through a pointer moved back by the slice's first index.  The flow launches of the bands never wait for an item of another
// launch (stream order), and the workers of all band launches in flight are accounted against the device's wave slots (flow budget,
// ovvc_picture.hip), so that every launch's workers can be resident: the bounded waits cannot expire by starvation.  If one does anyway the
// picture FAILS (the rows already published to readers cannot be taken back); ovhip_job_wait reports it.
#include "ovvc_job.hip.h"

extern "C" void ovhip_rec_tb_split_range_(const ovhip_recorder *r, size_t first, size_t n, ovhip_tb_cmd *out, size_t counts[4], size_t tiny[4][4]);
extern "C" int  ovhip_rec_itasks_sorted_range_(const ovhip_recorder *r, size_t first, size_t n, ovhip_itask *out, uint32_t *level_start, size_t cap, uint32_t *n_levels);

enum { MAX_BANDS = 96, ARENA_CHUNKS = 16, BAND_LEVELS = 4096 };
struct ArenaChunk { char *host, *dev; size_t cap, used; };
struct BandRec {
    int32_t row0, row1;
    ovhip_band_counts c0, c1;
    const ovhip_itask *d_it; uint32_t n_it; int tagged;          // the band's ordered tasks on the device; tagged: a flow launch wrote them
    const ovhip_dbf_edge *d_ev, *d_eh; uint32_t n_ev, n_eh;
    int flow_charge;                                             // workers charged to the device's flow budget until ev_recon is seen
    int32_t rows_final;                                          // picture rows final once this band's tail has run
};
struct BandState {
    int active, n, tails, closed, failed;
    ovhip_pic dst;
    ovhip_band_counts cur;
    int32_t row_prev, dbf_rows, sao_rows, alf_rows, rows_final;
    int log2_ctu, sao_on, alf_on, filters_latched;
    uint32_t stages;
    const uint16_t *d_fwd, *d_bwd; int lmcs_up;                   // LMCS tables: in the first band's block
    ovhip_alf_pic d_alf; int alf_up;                              // ALF picture-level tables: in the block of the first call that has them
    ovhip_lmcs_luts luts; int have_luts;
    ovhip_dbf_offsets offs;
    ArenaChunk chunk[ARENA_CHUNKS]; int n_chunks, cur_chunk;
    BandRec band[MAX_BANDS];
    hipEvent_t ev_recon[MAX_BANDS], ev_tail[MAX_BANDS];
    uint32_t level_start[BAND_LEVELS + 2];
    void *last_event; int32_t last_rows;                          // what ovhip_job_band_progress hands out
    uint16_t *keep; int keep_valid;                               // device: the previous band's bottom row before / after its filters (4 w samples)
};

// The bottom row of a band as the band below must see it.  Intra prediction, the cross-component model and the chroma-scale
// derivation of band k + 1 read the row above it UNFILTERED and in the mapped domain (the reference keeps saved lines for this,
// rcn_ctu.c:246-510), but band k's filters run with band k, so that its rows are final one band earlier: the row (luma row end - 1,
// chroma rows end / 2 - 1) is set aside before the filters and put back for the time band k + 1 is reconstructed.  Nobody else reads
// it meanwhile: rows within 8 of a band's end are not final -- not posted to readers, not reached by SAO / ALF -- before the
// deblocking of the band below has run.  mode 0: keep_unf <- picture; 1: keep_fil <- picture, picture <- keep_unf (& mask);
// 2: picture <- keep_fil.  keep = [unf: Y w | Cb w/2 | Cr w/2][fil: the same].
__global__ __launch_bounds__(256) void k_band_row(ovhip_pic pic, uint16_t *keep, int row_y, int mode, unsigned mask)
{
    const int i = blockIdx.x * 256 + threadIdx.x, w = pic.w, wc = w >> 1;
    if (i >= 2 * w) return;
    uint16_t *p = i < w ? pic.y + (size_t)row_y * pic.stride_y + i
                        : (i < w + wc ? pic.cb + (size_t)(row_y >> 1) * pic.stride_c + (i - w) : pic.cr + (size_t)(row_y >> 1) * pic.stride_c + (i - w - wc));
    uint16_t *unf = keep + i, *fil = keep + 2 * w + i;
    if (mode == 0) *unf = *p;
    else if (mode == 1) { *fil = *p; *p = (uint16_t)(*unf & mask); }
    else *p = *fil;
}
static int band_row(ovhip_job *j, const ovhip_pic *pic, int row_y, int mode, unsigned mask)
{
    hipLaunchKernelGGL(k_band_row, dim3((2 * pic->w + 255) / 256), dim3(256), 0, j->ctx->stream, *pic, j->bs->keep, row_y, mode, mask);
    OV_LAUNCH_CHECK(j->ctx, "k_band_row");
    j->st.n_launches++;
    return OVHIP_OK;
}

// the charges of bands whose reconstruction has completed go back (in order: a later band's launches are behind the earlier ones'); the
// record of the band after the last one holds the charge of a call for it that failed (ovhip_job_band)
static void band_reclaim(ovhip_job *j, int wait)
{
    BandState *bs = j->bs;
    for (int b = 0; bs && b <= bs->n && b < MAX_BANDS; ++b)
        if (!band_flow_reclaim(j->ctx, &bs->band[b].flow_charge, bs->ev_recon[b], wait)) break;
}

int band_active(const ovhip_job *j) { return j->bs && j->bs->active; }

void band_free(ovhip_job *j)
{
    BandState *bs = j->bs;
    if (!bs) return;
    band_reclaim(j, 1);
    for (int i = 0; i < bs->n_chunks; ++i) { pinned_free(nullptr, bs->chunk[i].host); if (bs->chunk[i].dev) (void)hipFree(bs->chunk[i].dev); }
    for (int i = 0; i < MAX_BANDS; ++i) { if (bs->ev_recon[i]) (void)hipEventDestroy(bs->ev_recon[i]); if (bs->ev_tail[i]) (void)hipEventDestroy(bs->ev_tail[i]); }
    if (bs->keep) (void)hipFree(bs->keep);
    free(bs);
    j->bs = nullptr;
}

// ovhip_job_begin: the previous picture's uploads have ended (ev_h2d); the arena starts over -- as ONE chunk if the last picture needed several
int band_reset(ovhip_job *j)
{
    BandState *bs = j->bs;
    if (!bs) return OVHIP_OK;
    band_reclaim(j, 1);
    if (bs->n_chunks > 1) {
        size_t total = 0;
        if (j->flushed) OV_HIP(j->ctx, hipEventSynchronize(j->ev_done));        // the launches read the device halves
        for (int i = 0; i < bs->n_chunks; ++i) { total += bs->chunk[i].cap; pinned_free(nullptr, bs->chunk[i].host); if (bs->chunk[i].dev) (void)hipFree(bs->chunk[i].dev); }
        memset(bs->chunk, 0, sizeof(bs->chunk));
        bs->n_chunks = 0;
        total += total / 4;
        bs->chunk[0].host = (char *)pinned_alloc(nullptr, total);
        if (!bs->chunk[0].host) return ov_fail(j->ctx, OVHIP_ENOMEM, "band arena (pinned)", hipSuccess);
        if (hipMalloc((void **)&bs->chunk[0].dev, total) != hipSuccess) { pinned_free(nullptr, bs->chunk[0].host); bs->chunk[0].host = nullptr; return ov_fail(j->ctx, OVHIP_ENOMEM, "band arena (device)", hipSuccess); }
        bs->chunk[0].cap = total; bs->n_chunks = 1;
    }
    for (int i = 0; i < bs->n_chunks; ++i) bs->chunk[i].used = 0;
    bs->cur_chunk = 0;
    bs->active = 0; bs->n = 0; bs->tails = 0; bs->closed = 0; bs->failed = 0;
    return OVHIP_OK;
}

// a block of `bytes` in the arena: the same offset in a page-locked host chunk and in its device twin (one copy moves it)
static int arena_take(ovhip_job *j, size_t bytes, char **host, char **dev)
{
    BandState *bs = j->bs;
    bytes = (bytes + 255) & ~(size_t)255;
    for (;;) {
        if (bs->cur_chunk < bs->n_chunks) {
            ArenaChunk &c = bs->chunk[bs->cur_chunk];
            if (c.cap - c.used >= bytes) { *host = c.host + c.used; *dev = c.dev + c.used; c.used += bytes; return OVHIP_OK; }
            bs->cur_chunk++;
            continue;
        }
        if (bs->n_chunks == ARENA_CHUNKS) return ov_fail(j->ctx, OVHIP_ENOMEM, "band arena: too many chunks", hipSuccess);
        // first chunk: ~ a 4K B picture's arrays (they sum to 9 MB); later ones double
        size_t cap = bs->n_chunks ? 2 * bs->chunk[bs->n_chunks - 1].cap : ((size_t)j->w * j->h * 3 / 2 < ((size_t)4 << 20) ? (size_t)4 << 20 : (size_t)j->w * j->h * 3 / 2);
        while (cap < bytes) cap *= 2;
        ArenaChunk &c = bs->chunk[bs->n_chunks];
        c.host = (char *)pinned_alloc(nullptr, cap);
        if (!c.host) return ov_fail(j->ctx, OVHIP_ENOMEM, "band arena (pinned)", hipSuccess);
        if (hipMalloc((void **)&c.dev, cap) != hipSuccess) { pinned_free(nullptr, c.host); c.host = nullptr; return ov_fail(j->ctx, OVHIP_ENOMEM, "band arena (device)", hipSuccess); }
        c.cap = cap; c.used = 0;
        bs->n_chunks++;
    }
}

int band_wait_done(ovhip_job *j)
{
    BandState *bs = j->bs;
    band_reclaim(j, 1);
    if (j->abort_host && *(volatile uint32_t *)j->abort_host) {
        *(volatile uint32_t *)j->abort_host = 0;
        if (j->d_flow) (void)hipMemset(j->d_flow, 0, sizeof(uint32_t));
        bs->failed = 1;
        return ov_fail(j->ctx, OVHIP_ELAUNCH, "band-wise picture: a bounded wait of the ordered pass expired (picture incomplete; its bands may have been read)", hipSuccess);
    }
    return bs->failed ? ov_fail(j->ctx, OVHIP_ELAUNCH, "band-wise picture failed", hipSuccess) : OVHIP_OK;
}

static inline int32_t floor8(int32_t v) { return v <= 0 ? 0 : v & ~7; }

extern "C" int ovhip_job_band_active(const ovhip_job *j) { return j && band_active(j); }

// the band arena's first chunk and the bottom-row buffer now, not in the first band of the job's first band-wise picture (what
// ovhip_frame_set_band_mode(f, 1) asks for: a frame thread's job is sized when it is created, see ovhip_job_reserve_for_picture)
extern "C" int ovhip_job_band_reserve(ovhip_job *j)
{
    if (!j) return OVHIP_EINVAL;
    OV_DEVICE(j->ctx);
    if (!j->bs) {
        j->bs = (BandState *)calloc(1, sizeof(BandState));
        if (!j->bs) return OVHIP_ENOMEM;
    }
    BandState *bs = j->bs;
    if (!bs->n_chunks) {
        char *h = nullptr, *d = nullptr;
        CHK(arena_take(j, 1, &h, &d));
        bs->chunk[0].used = 0; bs->cur_chunk = 0;
    }
    if (!bs->keep) OV_HIP(j->ctx, hipMalloc((void **)&bs->keep, (size_t)4 * j->w * sizeof(uint16_t)));
    if (!j->res.y) CHK(ovhip_pic_alloc(j->ctx, j->w, j->h, &j->res));
    return state_words(j, &j->d_flow, ovhip_intra_flow_words(j->w, j->h));
}

// 1: the reconstruction of the last band submitted is still running on the device.  A caller that is ahead of the device leaves its
// next band to a later hook (it then covers more CTU rows): the launches stay few and full when the device is the slower side -- and
// an I picture, whose ordered pass is one dependency chain per band, keeps its wavefront across as many rows as the parse has delivered
extern "C" int ovhip_job_band_busy(ovhip_job *j)
{
    if (!j || !band_active(j) || !j->bs->n) return 0;
    (void)hipSetDevice(j->ctx->device);
    if (hipEventQuery(j->bs->ev_recon[j->bs->n - 1]) == hipSuccess) return 0;
    (void)hipGetLastError();
    return 1;
}

extern "C" int ovhip_job_band_progress(ovhip_job *j, int32_t *rows_final, void **event, const volatile uint32_t **abort_word)
{
    if (!j || !rows_final) return OVHIP_EINVAL;
    *rows_final = 0;
    if (event) *event = nullptr;
    if (abort_word) *abort_word = j->abort_host;
    if (!band_active(j)) return OVHIP_OK;
    *rows_final = j->bs->last_rows;
    if (event) *event = j->bs->last_event;
    return OVHIP_OK;
}

// ---- ovhip_job_band in phases: first-band initialisation -> the band's slices, the tails and filter rows to run -> layout, fill and
// upload -> recon -> tails.  What passes between them: BandCall (what this call submits) and Placement (where staging put it).
struct BandCall {
    int b, last; int32_t row_end;
    ovhip_band_counts c0, c1, n;                   // the slices [c0, c1) and their counts as this call runs them (n_itask: 0 without OVHIP_STAGE_INTRA, n_edge_*: 0 without _DBF)
    size_t n_items;                                // flow items of the band; 0: one launch per level
    int t_first, t_end;                            // tails [t_first, t_end): this band's (see "bottom row" above)
    int sao_on, alf_on;
    int32_t dbf_new, sao_new, alf_new;             // the filter rows those tails make final
    int nb_ctu_w, sao_r0, alf_r0; size_t n_sao, n_alf;      // the CTU rows of the callers' SAO / ALF parameters they read
    int have_levels; const uint32_t *h_items;      // (band_stage) the level table holds the band; the host copy of its flow items
};

static int band_first(ovhip_job *j, const ovhip_pic *dst, const ovhip_job_params *pr, int log2_ctu)
{
    BandState *bs = j->bs;
    memset(&j->st, 0, sizeof(j->st));
    bs->active = 1; bs->n = 0; bs->tails = 0; bs->closed = 0; bs->failed = 0;
    bs->dst = *dst; bs->row_prev = 0; bs->dbf_rows = bs->sao_rows = bs->alf_rows = bs->rows_final = 0;
    memset(&bs->cur, 0, sizeof(bs->cur));
    bs->log2_ctu = log2_ctu; bs->filters_latched = 0; bs->lmcs_up = 0; bs->alf_up = 0; bs->have_luts = 0;
    bs->stages = switches_of(pr).stages;
    bs->last_event = nullptr; bs->last_rows = 0; bs->keep_valid = 0;
    j->again.valid = 0; j->n_retries = 0;       // (n_mv / n_tmvp: the eager DMVR rows' -- a pass may have run before the first band)
    CHK(ordered_arm(j, &j->d_flow, ovhip_intra_flow_words(j->w, j->h)));
    CHK(dev_reserve(j, B_SCALE, 65536));                               // 32767 regions at most (ovhip_rec_lmcs_region)
    CHK(dev_reserve(j, B_CLASS, (size_t)((j->w + 3) / 4) * ((j->h + 3) / 4)));
    return OVHIP_OK;
}

static int band_plan(ovhip_job *j, const ovhip_pic *dst, const ovhip_job_params *pr, const ovhip_band_counts *upto, int log2_ctu, BandCall &k)
{
    ovhip_ctx *ctx = j->ctx;
    BandState *bs = j->bs;
    ovhip_recorder *rec = j->rec;
    const int32_t row_end = k.row_end;
    if (!(dst->y == bs->dst.y) || log2_ctu != bs->log2_ctu) return ov_fail(ctx, OVHIP_EINVAL, "ovhip_job_band: another picture than the first band's", hipSuccess);
    if (row_end < bs->row_prev || (!k.last && (row_end & ((1 << log2_ctu) - 1)) && row_end != j->h))
        return ov_fail(ctx, OVHIP_EINVAL, "ovhip_job_band: row_end must be a CTU-row boundary not above the previous band's", hipSuccess);
    if (bs->n >= MAX_BANDS) return ov_fail(ctx, OVHIP_EUNSUP, "ovhip_job_band: too many bands", hipSuccess);
    const uint32_t stages = bs->stages;
    band_reclaim(j, 0);

    // ---- the band's slices ----
    ovhip_band_counts c1;
    ovhip_rec_counts(rec, &c1);
    if (upto) {
        const uint32_t *u = &upto->n_tb, *m = &c1.n_tb, *lo = &bs->cur.n_tb;
        for (int i = 0; i < 10; ++i) if (u[i] > m[i] || u[i] < lo[i]) return ov_fail(ctx, OVHIP_EINVAL, "ovhip_job_band: counts outside the recorded arrays", hipSuccess);
        c1 = *upto;
    }
    const ovhip_band_counts c0 = bs->cur;
    const int b = k.b = bs->n;
    BandRec &B = bs->band[b];
    const int charged = B.flow_charge;           // left by a call for this band that failed after its charge (band_reclaim)
    memset(&B, 0, sizeof(B));
    B.flow_charge = charged;
    B.row0 = bs->row_prev; B.row1 = row_end; B.c0 = k.c0 = c0; B.c1 = k.c1 = c1;
    size_t dummy = 0;
    if (ovhip_rec_ciip_units(rec, &dummy) && dummy) return ov_fail(ctx, OVHIP_EUNSUP, "ovhip_job_band: stand-alone CIIP blend units (a second picture with the caller's intra prediction)", hipSuccess);
    if (ovhip_rec_rpr_units(rec, &dummy) && dummy) return ov_fail(ctx, OVHIP_EUNSUP, "ovhip_job_band: reference picture resampling units", hipSuccess);
    if (ovhip_rec_aff_rpr_units(rec, &dummy) && dummy) return ov_fail(ctx, OVHIP_EUNSUP, "ovhip_job_band: reference picture resampling units (affine)", hipSuccess);
    if (ovhip_rec_ibc_tasks(rec)) return ov_fail(ctx, OVHIP_EUNSUP, "ovhip_job_band: intra block copy tasks (the whole-picture flush runs them)", hipSuccess);
    {
        const uint32_t *hi = &c1.n_tb, *lo = &c0.n_tb; uint32_t *n = &k.n.n_tb;
        for (int i = 0; i < 10; ++i) n[i] = hi[i] - lo[i];
    }
    if (!(stages & OVHIP_STAGE_DBF)) k.n.n_edge_v = k.n.n_edge_h = 0;
    if (!(stages & OVHIP_STAGE_INTRA)) k.n.n_itask = 0;
    // flow items of the band: counted first (the count does not depend on the order), built after the sort; 0: one launch per level
    k.n_items = k.n.n_itask && !(pr->stages && (stages & OVHIP_STAGE_INTRA_LEVELS)) ? ovhip_intra_flow_items_(ovhip_rec_itasks(rec, &dummy) + c0.n_itask, k.n.n_itask, nullptr, 0) : 0;

    // ---- which tails this call runs, and the filter rows they make final ----
    const Switches sw = switches_of(pr);
    k.t_first = bs->tails; k.t_end = b + 1;
    if (k.t_end > k.t_first && !bs->filters_latched) {
        bs->sao_on = sw.sao_on; bs->alf_on = sw.alf_on;
        bs->filters_latched = 1;
    }
    if (bs->filters_latched && (bs->sao_on != sw.sao_on || bs->alf_on != sw.alf_on))
        return ov_fail(ctx, OVHIP_EINVAL, "ovhip_job_band: SAO / ALF switched on or off inside a picture", hipSuccess);
    k.sao_on = bs->filters_latched && bs->sao_on; k.alf_on = bs->filters_latched && bs->alf_on;
    if (k.alf_on && alf_tables_missing(pr)) return ov_fail(ctx, OVHIP_EINVAL, "ovhip_job_band: ALF tables missing", hipSuccess);
    k.dbf_new = bs->dbf_rows; k.sao_new = bs->sao_rows; k.alf_new = bs->alf_rows;
    if (k.t_end > k.t_first) {
        const int32_t E = k.t_end - 1 == b ? row_end : bs->band[k.t_end - 1].row1;
        const bool fin = k.last != 0;
        k.dbf_new = fin ? j->h : ((stages & OVHIP_STAGE_DBF) ? (E - 8 > k.dbf_new ? E - 8 : k.dbf_new) : E);
        // the second stage (SAO, or the copy that stands in for it) reads one row below its window; the third (ALF, or the copy back)
        // three rows below its own -- and the second stage's next window re-reads the row above it, which the third must leave alone
        k.sao_new = fin ? j->h : (floor8(k.dbf_new - 1) > k.sao_new ? floor8(k.dbf_new - 1) : k.sao_new);
        k.alf_new = fin ? j->h : (floor8(k.sao_new - 3) > k.alf_new ? floor8(k.sao_new - 3) : k.alf_new);
    }
    k.nb_ctu_w = (j->w + (1 << log2_ctu) - 1) >> log2_ctu;
    k.sao_r0 = bs->sao_rows >> log2_ctu; k.alf_r0 = bs->alf_rows >> log2_ctu;
    const int sao_r1 = k.sao_new > bs->sao_rows ? ((k.sao_new - 1) >> log2_ctu) + 1 : k.sao_r0;
    const int alf_r1 = k.alf_new > bs->alf_rows ? ((k.alf_new - 1) >> log2_ctu) + 1 : k.alf_r0;
    k.n_sao = k.sao_on ? (size_t)(sao_r1 - k.sao_r0) * k.nb_ctu_w : 0; k.n_alf = k.alf_on ? (size_t)(alf_r1 - k.alf_r0) * k.nb_ctu_w : 0;
    return OVHIP_OK;
}

// one staging block out of the arena: layout, fill, ONE copy; then the Chain over it
static int band_stage(ovhip_job *j, const ovhip_pic *dst, const ovhip_job_params *pr, BandCall &k, Placement &p, Chain &c)
{
    ovhip_ctx *ctx = j->ctx;
    BandState *bs = j->bs;
    ovhip_recorder *rec = j->rec;
    const ovhip_band_counts &c0 = k.c0, &n = k.n;
    // ---- layout ----
    Layout L;
    const bool lmcs_now = pr->lmcs && !bs->lmcs_up, alf_now = k.alf_on && !bs->alf_up;
    p = Placement{};
    p.tabs = tables_put(L, alf_now, lmcs_now);
    const size_t o_tb = L.put(n.n_tb * sizeof(ovhip_tb_cmd)), o_coef = L.put((size_t)n.n_coef * 2), o_mc = L.put(n.n_mc * sizeof(ovhip_mc_unit)),
                 o_mcx = L.put(n.n_mcx * sizeof(ovhip_mc_unit)), o_aff = L.put(n.n_aff * sizeof(ovhip_aff_unit)), o_side = L.put((size_t)n.n_side * 4),
                 o_reg = L.put(n.n_reg * sizeof(ovhip_lmcs_region)), o_it = L.put(n.n_itask * sizeof(ovhip_itask)), o_items = L.put(k.n_items * 4),
                 o_ev = L.put(n.n_edge_v * sizeof(ovhip_dbf_edge)), o_eh = L.put(n.n_edge_h * sizeof(ovhip_dbf_edge));
    p.o_sao = L.put(k.n_sao * sizeof(ovhip_sao_ctu)); p.o_alf = L.put(k.n_alf * sizeof(ovhip_alf_ctu));
    const size_t upload_bytes = L.o;
    const size_t o_mv = L.put((size_t)n.n_mcx * 16);                   // device only: the refined vectors k_mcxa leaves (nobody reads them here)
    char *hb = nullptr, *db = nullptr;
    if (L.o) CHK(arena_take(j, L.o, &hb, &db));

    // ---- fill ----
    uint32_t n_lv = 0;
    if (n.n_tb) ovhip_rec_tb_split_range_(rec, c0.n_tb, n.n_tb, (ovhip_tb_cmd *)(hb + o_tb), c.cls, c.tiny);
    k.have_levels = n.n_itask && ovhip_rec_itasks_sorted_range_(rec, c0.n_itask, n.n_itask, (ovhip_itask *)(hb + o_it), bs->level_start, BAND_LEVELS + 2, &n_lv) == 0;
    if (n.n_itask && !k.have_levels && !k.n_items) return ov_fail(ctx, OVHIP_EUNSUP, "ovhip_job_band: a band with more levels than the table holds and blocks the flow launch cannot take", hipSuccess);
    k.h_items = (const uint32_t *)(hb + o_items);
    if (k.n_items) (void)ovhip_intra_flow_items_((const ovhip_itask *)(hb + o_it), n.n_itask, (uint32_t *)(hb + o_items), k.n_items);
    size_t all;
    if (n.n_coef) memcpy(hb + o_coef, ovhip_rec_coefs(rec, &all) + c0.n_coef, (size_t)n.n_coef * 2);
    if (n.n_mc) memcpy(hb + o_mc, ovhip_rec_mc_units(rec, &all) + c0.n_mc, n.n_mc * sizeof(ovhip_mc_unit));
    if (n.n_mcx) memcpy(hb + o_mcx, ovhip_rec_mcx_units(rec, &all) + c0.n_mcx, n.n_mcx * sizeof(ovhip_mc_unit));
    if (n.n_aff) memcpy(hb + o_aff, ovhip_rec_aff_units(rec, &all) + c0.n_aff, n.n_aff * sizeof(ovhip_aff_unit));
    if (n.n_side) memcpy(hb + o_side, ovhip_rec_aff_side(rec, &all) + c0.n_side, (size_t)n.n_side * 4);
    if (n.n_reg) memcpy(hb + o_reg, ovhip_rec_lmcs_regions(rec, &all) + c0.n_reg, n.n_reg * sizeof(ovhip_lmcs_region));
    const ovhip_dbf_edge *ev = ovhip_rec_dbf_edges(rec, 0, &all, &bs->offs), *eh = ovhip_rec_dbf_edges(rec, 1, &all, nullptr);
    if (n.n_edge_v) memcpy(hb + o_ev, ev + c0.n_edge_v, n.n_edge_v * sizeof(ovhip_dbf_edge));
    if (n.n_edge_h) memcpy(hb + o_eh, eh + c0.n_edge_h, n.n_edge_h * sizeof(ovhip_dbf_edge));
    if (k.n_sao) memcpy(hb + p.o_sao, pr->sao + (size_t)k.sao_r0 * k.nb_ctu_w, k.n_sao * sizeof(ovhip_sao_ctu));
    if (k.n_alf) memcpy(hb + p.o_alf, pr->alf_ctus + (size_t)k.alf_r0 * k.nb_ctu_w, k.n_alf * sizeof(ovhip_alf_ctu));
    tables_fill(hb, p.tabs, pr, alf_now, lmcs_now);
    // ---- upload ----
    if (upload_bytes) {
        OV_HIP(ctx, hipMemcpyAsync(db, hb, upload_bytes, hipMemcpyHostToDevice, ctx->stream));
        j->st.h2d_bytes += upload_bytes; j->st.n_h2d++;
    }
    OV_HIP(ctx, hipEventRecord(j->ev_h2d, ctx->stream));
    if (lmcs_now) { bs->d_fwd = (const uint16_t *)(db + p.tabs.at[T_FWD]); bs->d_bwd = (const uint16_t *)(db + p.tabs.at[T_BWD]); bs->lmcs_up = 1; bs->luts = *pr->lmcs; bs->have_luts = 1; }
    if (alf_now) { bs->d_alf = alf_pic_at(db, p.tabs, nullptr, (uint8_t *)j->dev[B_CLASS].p, bs->log2_ctu); bs->alf_up = 1; }
    if (pr->lmcs && !bs->lmcs_up) return ov_fail(ctx, OVHIP_EINVAL, "ovhip_job_band: LMCS tables", hipSuccess);
    // ---- the placement, and the chain over it ----
    p.block = db;
    p.at[B_TB] = db + o_tb; p.at[B_COEF] = db + o_coef; p.at[B_MC] = db + o_mc; p.at[B_MCX] = db + o_mcx; p.at[B_MV] = db + o_mv;
    p.at[B_AFF] = db + o_aff; p.at[B_SIDE] = db + o_side; p.at[B_REG] = db + o_reg; p.at[B_ITASK] = db + o_it; p.at[B_IITEM] = db + o_items;
    p.at[B_EV] = db + o_ev; p.at[B_EH] = db + o_eh;
    c.j = j; c.dst = dst; c.res = &j->res; c.log2_ctu = bs->log2_ctu;
    c.luts = pr->lmcs ? &bs->luts : nullptr; c.d_fwd = pr->lmcs ? bs->d_fwd : nullptr; c.d_scales = (int16_t *)j->dev[B_SCALE].p;
    chain_bind(c, p, c0, n, 0, 0);
    c.h_it = (const ovhip_itask *)(hb + o_it); c.lv_start = bs->level_start; c.n_lv = n_lv;
    BandRec &B = bs->band[k.b];
    B.d_it = c.d_it; B.n_it = c.n_it;
    B.d_ev = (const ovhip_dbf_edge *)p.at[B_EV]; B.n_ev = n.n_edge_v; B.d_eh = (const ovhip_dbf_edge *)p.at[B_EH]; B.n_eh = n.n_edge_h;
    j->st.n_tb += n.n_tb; j->st.n_mc += n.n_mc; j->st.n_mcx += n.n_mcx; j->st.n_aff += n.n_aff;
    j->st.n_edges_v += n.n_edge_v; j->st.n_edges_h += n.n_edge_h; j->st.n_regions += n.n_reg; j->st.n_itasks += n.n_itask; j->st.n_ilevels += n_lv;
    return OVHIP_OK;
}

// the launches of recon(b) that the flow charge covers, ev_recon behind them
static int band_recon_enqueue(ovhip_job *j, const ovhip_pic *dst, const BandCall &k, Chain &c, int flow_workers)
{
    ovhip_ctx *ctx = j->ctx;
    BandState *bs = j->bs;
    const int b = k.b;
    BandRec &B = bs->band[b];
    // the row above the band as the band's reconstruction must see it (k_band_row): unfiltered, mapped -- and without the hand-over
    // bit when the readers are the per-level kernels, which take samples as they are
    const bool swap_row = b > 0 && bs->keep_valid && (c.n_it || c.n_reg) && B.row0 > 0;
    if (swap_row) CHK(band_row(j, dst, B.row0 - 1, 1, c.n_items ? 0xffffu : 0x03ffu));
    if (bs->stages & OVHIP_STAGE_ITX) CHK(chain_residual(c, nullptr));
    if (c.n_it) {
        // one launch per level: its kernels read plain samples -- the band above must not carry the flow launches' hand-over bit any more
        if (!c.n_items && b > 0 && bs->band[b - 1].tagged && bs->tails < b) {
            CHK(ovhip_intra_flow_untag_launch(ctx, dst, bs->band[b - 1].d_it, bs->band[b - 1].n_it, 1));
            bs->band[b - 1].tagged = 2;                          // (un-tagged early: the tail leaves the bit alone)
            j->st.n_launches++;
        }
        CHK(chain_ordered(c, flow_workers));
        if (c.n_items) B.tagged = 1;
    }
    if (swap_row) CHK(band_row(j, dst, B.row0 - 1, 2, 0));
    if (!k.last && B.row1 > B.row0) { CHK(band_row(j, dst, B.row1 - 1, 0, 0)); bs->keep_valid = 1; }
    OV_HIP(ctx, hipEventRecord(bs->ev_recon[b], ctx->stream));
    return OVHIP_OK;
}

static int band_recon(ovhip_job *j, const ovhip_pic *dst, const ovhip_pic *refs, uint32_t n_refs, const ovhip_job_params *pr,
                      const BandCall &k, const Placement &p, Chain &c)
{
    ovhip_ctx *ctx = j->ctx;
    BandState *bs = j->bs;
    BandRec &B = bs->band[k.b];
    if (bs->stages & OVHIP_STAGE_MC) CHK(chain_predict(c, refs, refs, n_refs, nullptr, (int32_t *)p.at[B_MV]));
    if (!bs->ev_recon[k.b]) OV_HIP(ctx, hipEventCreateWithFlags(&bs->ev_recon[k.b], hipEventDisableTiming));
    int flow_workers = 0;
    if (k.n_items) {
        // workers: no more than the band's widest level can use, no more than the device's budget has left (else: one launch per level)
        flow_workers = band_flow_take(ctx, flow_worker_count(ctx, pr->flow_workers, c.h_it, k.h_items, k.n_items, true));
        if (!flow_workers && !k.have_levels) return ov_fail(ctx, OVHIP_EUNSUP, "ovhip_job_band: flow budget exhausted and no level table", hipSuccess);
        B.flow_charge += flow_workers;
        c.n_items = flow_workers ? (uint32_t)k.n_items : 0;
    }
    // What follows enqueues the work the charge covers.  A failure leaves the charge with the band's record, ev_recon recorded behind
    // what was enqueued: band_reclaim gives it back once that has run (a retry of the band adds its own charge to it).
    const int r = band_recon_enqueue(j, dst, k, c, flow_workers);
    if (r != OVHIP_OK) {
        if (B.flow_charge) (void)hipEventRecord(bs->ev_recon[k.b], ctx->stream);
        return r;
    }
    bs->n = k.b + 1; bs->cur = k.c1; bs->row_prev = k.row_end;
    return OVHIP_OK;
}

// tails: inverse luma mapping + un-tag, deblocking, per band; then the SAO / ALF rows they made final, once
static int band_tails(ovhip_job *j, const ovhip_pic *dst, const ovhip_job_params *pr, const BandCall &k, const Placement &p, const Chain &c)
{
    ovhip_ctx *ctx = j->ctx;
    BandState *bs = j->bs;
    const uint16_t *d_bwd = pr->lmcs && (bs->stages & OVHIP_STAGE_ITX) ? bs->d_bwd : nullptr;
    for (int t = k.t_first; t < k.t_end; ++t) {
        const BandRec &T = bs->band[t];
        if (T.row1 > T.row0) CHK(chain_unmap(j, dst, T.row0, T.row1, d_bwd, T.d_it, T.tagged == 1 ? T.n_it : 0u));
        if (bs->stages & OVHIP_STAGE_DBF) CHK(chain_deblock(c, T.d_ev, T.n_ev, T.d_eh, T.n_eh, &bs->offs));
    }
    if (k.t_end <= k.t_first) return OVHIP_OK;
    ovhip_alf_pic ap = bs->d_alf;
    ap.ctus = k.alf_on ? (const ovhip_alf_ctu *)(p.block + p.o_alf) - (size_t)k.alf_r0 * k.nb_ctu_w : nullptr;
    CHK(chain_filters(c, k.sao_on ? (const ovhip_sao_ctu *)(p.block + p.o_sao) - (size_t)k.sao_r0 * k.nb_ctu_w : nullptr, k.alf_on ? &ap : nullptr,
                      bs->sao_rows, k.sao_new, bs->alf_rows, k.alf_new));
    bs->dbf_rows = k.dbf_new; bs->sao_rows = k.sao_new; bs->alf_rows = k.alf_new;
    bs->rows_final = (k.sao_on || k.alf_on) ? k.alf_new : k.dbf_new;
    bs->tails = k.t_end;
    const int te = k.t_end - 1;
    bs->band[te].rows_final = bs->rows_final;
    if (!bs->ev_tail[te]) OV_HIP(ctx, hipEventCreateWithFlags(&bs->ev_tail[te], hipEventDisableTiming));
    OV_HIP(ctx, hipEventRecord(bs->ev_tail[te], ctx->stream));
    bs->last_event = (void *)bs->ev_tail[te]; bs->last_rows = bs->rows_final;
    return OVHIP_OK;
}

extern "C" int ovhip_job_band(ovhip_job *j, const ovhip_pic *dst, const ovhip_pic *refs, uint32_t n_refs, const ovhip_job_params *pr,
                   const ovhip_band_counts *upto, int32_t row_end, int32_t last)
{
    if (!j || !dst || !pr) return OVHIP_EINVAL;
    ovhip_ctx *ctx = j->ctx;
    OV_DEVICE(ctx);
    if (dst->w != j->w || dst->h != j->h) return ov_fail(ctx, OVHIP_EINVAL, "ovhip_job_band: picture size differs from the job's", hipSuccess);
    if (dst->stride_y != j->tmp.stride_y || dst->stride_c != j->tmp.stride_c)
        return ov_fail(ctx, OVHIP_EUNSUP, "ovhip_job_band: tight planes only (stride = width)", hipSuccess);
    if (!j->bs || !j->bs->active) CHK(ovhip_job_band_reserve(j));       // (the first band of a picture)
    const int log2_ctu = switches_of(pr).log2_ctu;
    if (log2_ctu < 5 || log2_ctu > 7) return ov_fail(ctx, OVHIP_EINVAL, "ovhip_job_band: log2_ctu_s", hipSuccess);
    if (j->bs->closed) return ov_fail(ctx, OVHIP_EINVAL, "ovhip_job_band: the picture's last band was already submitted", hipSuccess);
    BandCall k = {};
    k.last = last; k.row_end = last || row_end > j->h ? j->h : row_end;
    Placement p;
    Chain c = {};
    if (!j->bs->active) CHK(band_first(j, dst, pr, log2_ctu));
    CHK(band_plan(j, dst, pr, upto, log2_ctu, k));                 // the band's slices, the tails and filter rows this call runs
    CHK(band_stage(j, dst, pr, k, p, c));                          // layout, fill, ONE copy; the chain over the block
    CHK(band_recon(j, dst, refs, n_refs, pr, k, p, c));            // recon(b) under its flow charge
    CHK(band_tails(j, dst, pr, k, p, c));
    // (behind every band: ovhip_job_wait / _begin / _destroy wait for what has been enqueued, whether or not the picture was completed)
    OV_HIP(ctx, hipEventRecord(j->ev_done, ctx->stream));
    j->flushed = 1; j->flow_launched = 0;
    if (last) j->bs->closed = 1;
    return OVHIP_OK;
}
