/* ovvc_frame.c -- one decoder frame thread on the device path (include/ovvc_hip.h, "Frame thread").
 *
 * What shim/rcn_hip.c keeps per OVCTUDec, moved into the library so that it can be executed and tested without the reference's
 * headers: context + job + the picture's place in the device DPB + its reference table, and the ORDER of a picture's end:
 *
 *     uploads enqueued -> wait for the reference pictures (host) -> launches -> ovhip_job_wait (incl. its second pass)
 *     -> publish + unpin the references -> outputs (optional; after the wait, never before: r2 downloaded first): picture_end
 *
 * The reference's order for the same events: slicedec.c:934-956 (filters of the last rows, then ovdpb_report_decoded_ctu_line),
 * rcn_inter.c:131-146 (a reader waits for its reference's rows), dectest.c:372-409 (the application reads the frame after the
 * picture was output).  Plain C over the C ABI; no HIP calls of its own.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include "ovvc_hip.h"
#include "ovvc_dpb_priv.h"
#include "ovvc_mvfield_priv.h"
#include "ovvc_rgb_lut_priv.h"
#include "ovvc_surface_lut_priv.h"

#define MAX_REFS 16

static double mono_s(void) { struct timespec t; clock_gettime(CLOCK_MONOTONIC, &t); return (double)t.tv_sec + 1e-9 * (double)t.tv_nsec; }

/* one per-picture output, in the order picture_end runs them.  RGB and surface write dst[0] through the window `win`; the motion field
 * writes its vectors to dst[0] and its info to dst[1] (either may be NULL) from the arrays of the job that decoded the picture; the
 * ladder and the RGB pyramid carry their rungs / levels, the pyramid also the size w x h it was checked against */
enum { OUT_RGB, OUT_SURFACE, OUT_LADDER, OUT_PYRAMID, OUT_MVFIELD, N_OUTS };
#define N_LUT_OUTS OUT_MVFIELD            /* the outputs in front of the motion field show the picture: each may go through a colour table */
typedef struct frame_out {
    int on;
    union {
        struct {
            union { ovhip_rgb_format rgb; ovhip_surface_format surf; ovhip_mvfield_format mvf; } fmt;
            ovhip_window win;
            void *dst[2]; size_t bytes[2];
        };
        struct { ovhip_reduce_info info; int32_t n; ovhip_ladder_rung rungs[OVHIP_LADDER_MAX_RUNGS]; } ladder;
        struct { ovhip_reduce_info info; int32_t n, w, h; ovhip_rgb_level levels[OVHIP_PYRAMID_MAX_LEVELS]; } pyr;
    };
} frame_out;
/* the colour table of such an output (ovhip_frame_set_rgb_lut / _surface_lut / _ladder_lut / _rgb_pyramid_lut) and, where the output
 * converts through it, the conversion: sticky, the table borrowed, NULL: none */
typedef struct frame_lut { const ovhip_rgb_lut *lut; ovhip_surface_conv conv; } frame_lut;

struct ovhip_frame {
    ovhip_dpb *dpb;
    int dev;
    int32_t w, h;
    int id;                               /* creation order: the frame's name in the event trace */
    ovhip_ctx *ctx;
    ovhip_job *job;                       /* own job, created on first use */
    /* dry frame (a DPB on a test back-end, no device): the same state machine and the same DPB calls, nothing launched.  Its own
     * plain recorder takes the picture's commands; the eager-DMVR counters move as the device's would. */
    double done_at, published_at;         /* CLOCK_MONOTONIC seconds: ovhip_job_wait returned / the picture was published (stall analysis) */
    int dry;
    ovhip_recorder *dry_rec;
    int64_t dry_pending, dry_done;
    const void *key; ovhip_pic dst; int live;
    const void *ref_key[MAX_REFS]; uint64_t ref_tag[MAX_REFS]; ovhip_pic ref_pic[MAX_REFS]; void *ref_ev[MAX_REFS]; unsigned char ref_pinned[MAX_REFS];
    int n_refs;
    int status;
    char err[192];
    /* band-wise submission (ovhip_frame_band): what has been handed to the job so far, how many rows were posted to the DPB */
    int band_mode;
    ovhip_band_counts band_prev;
    int32_t band_row_prev, band_rows_posted, dry_row_prev2;
    int n_bands, n_deferred;
    /* what the outputs do to the picture first (ovvc_dpb_priv.h).  SCALE (ovhip_frame_set_output_scale): resampled to post.out_w x
     * post.out_h; GRAIN (ovhip_frame_set_film_grain): with film grain at post.poc, the model derived afresh from fg for every picture;
     * REDUCE (ovhip_frame_set_output_reduce): the window post.rinfo names reduced to post.out_w x post.out_h.  ONE kind at a time */
    ovhip_post_ post;
    ovhip_fg_params fg;
    /* decoded picture hash (ovhip_frame_set_picture_hash): what to take of every completed picture, what the caller expects of the next
     * one, what the last one gave */
    int hash_on, hash_method, hash_planes, hash_expect, hash_done;
    ovhip_pic_hash_value hash_expected, hash_computed;
    /* the per-picture outputs (ovhip_frame_set_rgb_output / _surface_output / _ladder_output / _rgb_pyramid_output / _mvfield_output) of
     * the NEXT picture completed, each independent of the others: the destinations are that picture's, so the settings end with it
     * (picture_end); their colour tables do not */
    frame_out outs[N_OUTS];
    frame_lut luts[N_LUT_OUTS];
    /* OVVC_HIP_FRAME_PROF=1: where the frame-level calls spend their wall time, printed when the frame is destroyed (seconds) */
    double pt_collect, pt_rows_begin, pt_band_refs, pt_band_job, pt_final_refs, pt_job_wait, pt_output, pt_submit; int pn_pics;
    double pt_fl_prepare, pt_fl_upload, pt_fl_refs, pt_fl_launch;      /* ovhip_job_flush by phase (ovhip_job_stats.host_us_*) */
};
static int g_frame_prof = -1;
#define PT_ON() (__atomic_load_n(&g_frame_prof, __ATOMIC_RELAXED) > 0)
#define PT0() const double pt0_ = PT_ON() ? mono_s() : 0.0
#define PT(acc) do { if (PT_ON()) (acc) += mono_s() - pt0_; } while (0)

/* ---- event trace (include/ovvc_hip.h, ovhip_frame_set_trace): WHEN a caller (shim/rcn_hip.c) makes its frame-level calls ---- */
static void (*g_trace)(void *user, const ovhip_frame_event *ev);
static void *g_trace_user;
static int g_next_id;

void
ovhip_frame_set_trace(void (*sink)(void *user, const ovhip_frame_event *ev), void *user)
{
    g_trace_user = user;
    __atomic_store_n(&g_trace, sink, __ATOMIC_RELEASE);
}

static void
trace(const ovhip_frame *f, uint32_t op, const void *key, uint64_t tag, int64_t a, int64_t b, int64_t result)
{
    void (*sink)(void *, const ovhip_frame_event *) = __atomic_load_n(&g_trace, __ATOMIC_ACQUIRE);
    if (!sink) return;
    ovhip_frame_event ev;
    memset(&ev, 0, sizeof(ev));
    ev.op = op; ev.frame = f->id; ev.key = (uint64_t)(uintptr_t)key; ev.tag = tag; ev.a = a; ev.b = b; ev.result = result;
    sink(g_trace_user, &ev);
}

static size_t
n_refined_units(ovhip_frame *f)
{
    size_t n = 0;
    ovhip_recorder *r = ovhip_frame_recorder(f);
    if (r) (void)ovhip_rec_mcx_units(r, &n);
    return n;
}

static int
fail(ovhip_frame *f, int code, const char *what)
{
    if (code < 0 && !f->status) {
        f->status = code;
        snprintf(f->err, sizeof(f->err), "%s (%d)%s%s", what, code, f->ctx ? ": " : "", f->ctx ? ovhip_last_error(f->ctx) : "");
    }
    return code;
}

int
ovhip_frame_create(ovhip_dpb *dpb, int dev, int32_t w, int32_t h, ovhip_frame **out)
{
    if (!dpb || !out || dev < 0 || dev >= ovhip_dpb_n_devices(dpb) || w <= 0 || h <= 0) return OVHIP_EINVAL;
    *out = NULL;
    const int hipdev = ovhip_dpb_device(dpb, dev);
    ovhip_frame *f = (ovhip_frame *)calloc(1, sizeof(*f));
    if (!f) return OVHIP_ENOMEM;
    f->dpb = dpb; f->dev = dev; f->w = w; f->h = h;
    f->id = __atomic_fetch_add(&g_next_id, 1, __ATOMIC_RELAXED);
    if (__atomic_load_n(&g_frame_prof, __ATOMIC_RELAXED) < 0) __atomic_store_n(&g_frame_prof, getenv("OVVC_HIP_FRAME_PROF") != NULL, __ATOMIC_RELAXED);
    if (hipdev < 0) {
        /* a DPB on a test back-end has no device to decode on: a dry frame (the caller's sequence of frame-level calls is the
         * subject, tests/test_shim_device_cpu.py); pictures "decode" to whatever the back-end's pic_alloc handed out */
        f->dry = 1;
        f->dry_rec = ovhip_rec_create(w, h);
        if (!f->dry_rec) { free(f); return OVHIP_ENOMEM; }
        *out = f;
        return OVHIP_OK;
    }
    int r = ovhip_ctx_create(&f->ctx, hipdev, NULL);
    if (r != OVHIP_OK) { free(f); return r; }
    *out = f;
    return OVHIP_OK;
}

static void
unpin_refs(ovhip_frame *f)
{
    for (int i = 0; i < f->n_refs; ++i)
        if (f->ref_pinned[i]) { (void)ovhip_dpb_unpin(f->dpb, f->ref_key[i]); f->ref_pinned[i] = 0; }
}

void
ovhip_frame_destroy(ovhip_frame *f)
{
    if (!f) return;
    if (f->live) (void)ovhip_frame_fail(f, OVHIP_EINVAL);
    if (PT_ON() && f->pn_pics)
        fprintf(stderr, "frame %d: %d pictures, ms per picture: dmvr collect %.3f, dmvr begin %.3f, band refs check %.3f, band enqueue %.3f, last band: refs wait %.3f, job wait %.3f, output %.3f; whole submit %.3f (flush: prepare %.3f, uploads %.3f, reference wait %.3f, launches %.3f)\n",
                f->id, f->pn_pics, 1e3 * f->pt_collect / f->pn_pics, 1e3 * f->pt_rows_begin / f->pn_pics, 1e3 * f->pt_band_refs / f->pn_pics, 1e3 * f->pt_band_job / f->pn_pics,
                1e3 * f->pt_final_refs / f->pn_pics, 1e3 * f->pt_job_wait / f->pn_pics, 1e3 * f->pt_output / f->pn_pics, 1e3 * f->pt_submit / f->pn_pics,
                1e3 * f->pt_fl_prepare / f->pn_pics, 1e3 * f->pt_fl_upload / f->pn_pics, 1e3 * f->pt_fl_refs / f->pn_pics, 1e3 * f->pt_fl_launch / f->pn_pics);
    if (f->job) ovhip_job_destroy(f->job);
    if (f->dry_rec) ovhip_rec_destroy(f->dry_rec);
    if (f->ctx) ovhip_ctx_destroy(f->ctx);
    free(f);
}

ovhip_ctx *ovhip_frame_ctx(ovhip_frame *f) { return f ? f->ctx : NULL; }
double ovhip_frame_published_at(const ovhip_frame *f) { return f ? f->published_at : 0.0; }
double ovhip_frame_done_at(const ovhip_frame *f) { return f ? f->done_at : 0.0; }

ovhip_job *
ovhip_frame_job(ovhip_frame *f)
{
    if (!f || f->dry) return NULL;
    if (!f->job) {
        if (fail(f, ovhip_job_create(f->ctx, f->w, f->h, &f->job), "ovhip_job_create") != OVHIP_OK) f->job = NULL;
        /* a frame thread's job: sized for its pictures now, not grown picture by picture (OVVC_HIP_NO_RESERVE=1: the A / B).  The
         * reservation is an optimisation: when it cannot be had (page-locked memory is short) the buffers grow with the pictures as they
         * did before, and a picture that then does not fit fails with the allocation's own error */
        else if (!getenv("OVVC_HIP_NO_RESERVE")) (void)ovhip_job_reserve_for_picture(f->job);
    }
    return f->job;
}

ovhip_recorder *
ovhip_frame_recorder(ovhip_frame *f)
{
    if (f && f->dry) return f->dry_rec;
    ovhip_job *j = ovhip_frame_job(f);
    return j ? ovhip_job_recorder(j) : NULL;
}
const char *ovhip_frame_last_error(const ovhip_frame *f) { return f ? f->err : "no frame"; }

int ovhip_frame_begin(ovhip_frame *f, const void *key) { return ovhip_frame_begin_tag(f, key, 0); }

int
ovhip_frame_begin_tag(ovhip_frame *f, const void *key, uint64_t tag)
{
    if (!f || !key) return OVHIP_EINVAL;
    /* a picture that was begun and never submitted must not leave its readers waiting */
    if (f->live) (void)ovhip_frame_fail(f, OVHIP_EINVAL);
    f->status = 0; f->err[0] = 0; f->n_refs = 0; f->hash_done = 0;
    int r = ovhip_dpb_begin_tag(f->dpb, key, tag, f->dev, f->w, f->h, &f->dst);
    trace(f, OVHIP_FE_BEGIN, key, tag, f->dev, 0, r);
    if (r != OVHIP_OK) return fail(f, r, "ovhip_dpb_begin");
    f->key = key; f->live = 1;
    memset(&f->band_prev, 0, sizeof(f->band_prev));
    f->band_row_prev = f->band_rows_posted = f->dry_row_prev2 = 0; f->n_bands = f->n_deferred = 0;
    if (f->dry) { ovhip_rec_reset(f->dry_rec); f->dry_pending = f->dry_done = 0; }
    if (f->job) {
        r = ovhip_job_begin(f->job);
        if (r != OVHIP_OK) { fail(f, r, "ovhip_job_begin"); (void)ovhip_frame_fail(f, r); return r; }
    }
    return OVHIP_OK;
}

int ovhip_frame_ref(ovhip_frame *f, const void *ref_key) { return ovhip_frame_ref_tag(f, ref_key, 0); }

int
ovhip_frame_ref_tag(ovhip_frame *f, const void *ref_key, uint64_t tag)
{
    if (!f || !ref_key || !f->live) return OVHIP_EINVAL;
    for (int i = 0; i < f->n_refs; ++i) if (f->ref_key[i] == ref_key) return i;
    if (f->n_refs >= MAX_REFS) return fail(f, OVHIP_EUNSUP, "more than 16 distinct reference pictures");
    const int i = f->n_refs++;
    f->ref_key[i] = ref_key; f->ref_tag[i] = tag; f->ref_pinned[i] = 0; f->ref_ev[i] = NULL;
    memset(&f->ref_pic[i], 0, sizeof(f->ref_pic[i]));
    /* as soon as the reference lists are known: a picture decoded on another device is pushed here when it is done */
    (void)ovhip_dpb_want_tag(f->dpb, ref_key, tag, f->dev);
    trace(f, OVHIP_FE_REF, ref_key, tag, i, 0, i);
    return i;
}

int
ovhip_frame_ref_at(ovhip_frame *f, int slot, const void *ref_key)
{
    if (!f || !ref_key || !f->live || slot != f->n_refs) return OVHIP_EINVAL;
    if (f->n_refs >= MAX_REFS) return fail(f, OVHIP_EUNSUP, "more than 16 reference table entries");
    f->n_refs++;
    f->ref_key[slot] = ref_key; f->ref_tag[slot] = 0; f->ref_pinned[slot] = 0; f->ref_ev[slot] = NULL;
    memset(&f->ref_pic[slot], 0, sizeof(f->ref_pic[slot]));
    (void)ovhip_dpb_want(f->dpb, ref_key, f->dev);
    return slot;
}

/* the device analogue of ovdpb_frame_synchro: every reference complete and, if it was decoded elsewhere, here */
static int
acquire_refs(ovhip_frame *f)
{
    for (int i = 0; i < f->n_refs; ++i) {
        if (f->ref_pinned[i]) continue;
        int r = ovhip_dpb_acquire_tag(f->dpb, f->ref_key[i], f->ref_tag[i], f->dev, &f->ref_pic[i], &f->ref_ev[i]);
        if (r != OVHIP_OK) return fail(f, r, r == OVHIP_EREF ? "a reference picture failed to decode" : "reference picture unknown to the device DPB");
        f->ref_pinned[i] = 1;
    }
    for (int i = 0; i < f->n_refs; ++i) {
        if (!f->ref_ev[i]) continue;
        int r = ovhip_dpb_wait_copy(f->dpb, f->dev, f->ref_ev[i]);
        if (r != OVHIP_OK) return fail(f, r, "transfer of a reference picture");
        f->ref_ev[i] = NULL;
    }
    return OVHIP_OK;
}

/* 1: every reference picture named so far is complete (acquired and pinned: ovhip_frame_dmvr_rows_begin / ovhip_frame_submit will not
 * wait for a decode), 0: not yet, < 0: one of them failed.  Never waits for a decode -- what a caller that may go on parsing asks before
 * it starts the eager DMVR rows (shim/rcn_hip.c with the caller patch: the CTU rows are then reported later instead of the parse
 * stopping here). */
static int refs_rows_ready(ovhip_frame *f, const int32_t *need, int block);
static void units_need_rows(ovhip_frame *f, const ovhip_band_counts *c0, const ovhip_band_counts *c1, int only_dmvr, int32_t *need);

int
ovhip_frame_refs_ready(ovhip_frame *f)
{
    if (!f || !f->live) return OVHIP_EINVAL;
    if (f->band_mode) {
        /* row-granular: the rows the DMVR units recorded since the last eager pass reach in each reference picture (rcn_inter.c:131-146
         * waits for exactly those, per block) */
        ovhip_band_counts c0, c1;
        int32_t need[MAX_REFS];
        memset(&c0, 0, sizeof(c0));
        ovhip_rec_counts(ovhip_frame_recorder(f), &c1);
        const int64_t done = f->dry ? f->dry_done : (f->job ? ovhip_job_dmvr_rows_collect(f->job) : 0);
        if (done < 0) return fail(f, (int)done, "ovhip_job_dmvr_rows_collect");
        c0.n_mcx = (uint32_t)done; c0.n_mc = c1.n_mc; c0.n_aff = c1.n_aff;
        units_need_rows(f, &c0, &c1, 1, need);
        return refs_rows_ready(f, need, 0);
    }
    for (int i = 0; i < f->n_refs; ++i) {
        if (f->ref_pinned[i]) continue;
        const int r = ovhip_dpb_poll_tag(f->dpb, f->ref_key[i], f->ref_tag[i]);
        if (r <= 0) return r < 0 ? fail(f, r, "a reference picture failed to decode") : 0;
    }
    const int r = acquire_refs(f);
    return r == OVHIP_OK ? 1 : r;
}

static int
before_launch_cb(void *user)
{
    ovhip_frame *f = (ovhip_frame *)user;
    return acquire_refs(f) != OVHIP_OK;
}

int64_t
ovhip_frame_dmvr_rows(ovhip_frame *f)
{
    if (!f || !f->live || (!f->job && !f->dry)) return OVHIP_EINVAL;
    int r = acquire_refs(f);
    if (r != OVHIP_OK) return r;
    int64_t n;
    if (f->dry) n = f->dry_done = f->dry_pending = (int64_t)n_refined_units(f);
    else n = ovhip_job_dmvr_rows(f->job, f->ref_pic, (uint32_t)f->n_refs);
    if (n < 0) fail(f, (int)n, "ovhip_job_dmvr_rows");
    trace(f, OVHIP_FE_DMVR_ROWS, f->key, 0, (int64_t)n_refined_units(f), 0, n);
    return n;
}

int64_t ovhip_frame_dmvr_rows_begin(ovhip_frame *f, int32_t log2_ctu_s) { return ovhip_frame_dmvr_rows_begin_upto(f, log2_ctu_s, (size_t)-1); }

int64_t
ovhip_frame_dmvr_rows_begin_upto(ovhip_frame *f, int32_t log2_ctu_s, size_t upto)
{
    if (!f || !f->live || (!f->job && !f->dry)) return OVHIP_EINVAL;
    /* the references are needed (and waited for) only if a unit the pass would cover is a DMVR unit: rows of BDOF-only units do not
     * stop the parse */
    PT0();
    int64_t c = f->dry ? (f->dry_done = f->dry_pending) : ovhip_job_dmvr_rows_collect(f->job);
    if (c < 0) { fail(f, (int)c, "ovhip_job_dmvr_rows_collect"); return c; }
    size_t nu = 0;
    const ovhip_mc_unit *u = ovhip_rec_mcx_units(ovhip_frame_recorder(f), &nu);
    if (nu > upto) nu = upto;
    int any = 0;
    for (size_t i = (size_t)c; i < nu && !any; ++i) any = (u[i].flags & OVHIP_MC_DMVR) != 0;
    if (any && f->band_mode) {
        ovhip_band_counts c0, c1;
        int32_t need[MAX_REFS];
        memset(&c0, 0, sizeof(c0));
        ovhip_rec_counts(ovhip_frame_recorder(f), &c1);
        c0.n_mcx = (uint32_t)c; c0.n_mc = c1.n_mc; c0.n_aff = c1.n_aff; c1.n_mcx = (uint32_t)nu;
        units_need_rows(f, &c0, &c1, 1, need);
        int r = refs_rows_ready(f, need, 1);
        if (r < 0) return r;
    } else if (any) {
        int r = acquire_refs(f);
        if (r != OVHIP_OK) return r;
    }
    int64_t n;
    if (f->dry) n = f->dry_pending = (int64_t)nu > f->dry_pending ? (int64_t)nu : f->dry_pending;
    else n = ovhip_job_dmvr_rows_begin_upto(f->job, f->ref_pic, (uint32_t)f->n_refs, log2_ctu_s, upto);
    PT(f->pt_rows_begin);
    if (n < 0) fail(f, (int)n, "ovhip_job_dmvr_rows_begin");
    trace(f, OVHIP_FE_DMVR_BEGIN, f->key, 0, (int64_t)nu, any, n);
    return n;
}

int64_t
ovhip_frame_dmvr_rows_collect(ovhip_frame *f)
{
    if (!f || !f->live || (!f->job && !f->dry)) return OVHIP_EINVAL;
    PT0();
    int64_t n = f->dry ? (f->dry_done = f->dry_pending) : ovhip_job_dmvr_rows_collect(f->job);
    PT(f->pt_collect);
    if (n < 0) fail(f, (int)n, "ovhip_job_dmvr_rows_collect");
    trace(f, OVHIP_FE_DMVR_COLLECT, f->key, 0, (int64_t)n_refined_units(f), 0, n);
    return n;
}

static int
publish(ovhip_frame *f, int status)
{
    if (!f->live) return OVHIP_EINVAL;
    f->live = 0;
    int r = ovhip_dpb_publish(f->dpb, f->key, status);
    f->published_at = mono_s();
    unpin_refs(f);
    return r;
}

/* a picture that ends, however it ends, takes its RGB, surface, ladder, pyramid and motion field destinations with it */
static void outs_clear(ovhip_frame *f) { for (int k = 0; k < N_OUTS; ++k) f->outs[k].on = 0; }

int
ovhip_frame_fail(ovhip_frame *f, int status)
{
    if (!f) return OVHIP_EINVAL;
    if (!f->status) f->status = status ? status : OVHIP_EINVAL;
    outs_clear(f);
    trace(f, OVHIP_FE_FAIL, f->key, 0, f->status, 0, 0);
    return publish(f, f->status);
}

int
ovhip_frame_set_output_scale(ovhip_frame *f, int32_t out_w, int32_t out_h, const ovhip_scale_info *info)
{
    if (!f) return OVHIP_EINVAL;
    if (!out_w && !out_h) { if (f->post.kind == OVHIP_POST_SCALE) f->post.kind = OVHIP_POST_NONE; return OVHIP_OK; }
    if (f->post.kind == OVHIP_POST_GRAIN) return OVHIP_EUNSUP;    /* the reference resamples the UNgrained frame over the grained one: no parity to offer */
    if (f->post.kind == OVHIP_POST_REDUCE) return OVHIP_EUNSUP;   /* one post setting */
    ovhip_scale_info si;
    memset(&si, 0, sizeof(si));
    if (info) si = *info;
    if (!f->dry) {                                                /* (a dry frame has no output: only remembered) */
        int32_t scale[4];
        const int r = ovhip_output_scale_check(f->w, f->h, &si, out_w, out_h, scale);
        if (r != OVHIP_OK) return r;
    }
    f->post.kind = OVHIP_POST_SCALE; f->post.out_w = out_w; f->post.out_h = out_h; f->post.info = si;
    return OVHIP_OK;
}

int
ovhip_frame_set_film_grain(ovhip_frame *f, const ovhip_fg_params *params, int32_t poc)
{
    if (!f) return OVHIP_EINVAL;
    if (!params) { if (f->post.kind == OVHIP_POST_GRAIN) f->post.kind = OVHIP_POST_NONE; return OVHIP_OK; }
    if (f->post.kind == OVHIP_POST_SCALE || f->post.kind == OVHIP_POST_REDUCE) return OVHIP_EUNSUP;
    ovhip_fg_model model;
    const int r = ovhip_fg_derive(params, &model, NULL);      /* the refusals come back here, not from a picture's output */
    if (r != OVHIP_OK) return r;
    f->post.kind = OVHIP_POST_GRAIN; f->post.poc = poc; f->fg = *params;      /* (a dry frame has no output: only remembered) */
    return OVHIP_OK;
}

int
ovhip_frame_set_output_reduce(ovhip_frame *f, int32_t out_w, int32_t out_h, const ovhip_reduce_info *info)
{
    if (!f) return OVHIP_EINVAL;
    if (!out_w && !out_h) { if (f->post.kind == OVHIP_POST_REDUCE) f->post.kind = OVHIP_POST_NONE; return OVHIP_OK; }
    if (f->post.kind == OVHIP_POST_GRAIN || f->post.kind == OVHIP_POST_SCALE) return OVHIP_EUNSUP;      /* one post setting */
    ovhip_reduce_info ri;
    memset(&ri, 0, sizeof(ri));
    if (info) ri = *info;
    if (!f->dry) {                                                /* (a dry frame has no output: only remembered) */
        int32_t ratio[4];
        const int r = ovhip_output_reduce_check(f->w, f->h, &ri, out_w, out_h, ratio);
        if (r != OVHIP_OK) return r;
    }
    f->post.kind = OVHIP_POST_REDUCE; f->post.out_w = out_w; f->post.out_h = out_h; f->post.rinfo = ri;
    return OVHIP_OK;
}

int
ovhip_frame_set_picture_hash(ovhip_frame *f, int method, int n_planes, const ovhip_pic_hash_value *expected)
{
    if (!f) return OVHIP_EINVAL;
    if (method < 0) { f->hash_on = 0; f->hash_expect = 0; return OVHIP_OK; }
    if (method > OVHIP_HASH_CHECKSUM || (n_planes != 1 && n_planes != 3)) return OVHIP_EINVAL;
    if (expected && (expected->method != method || expected->n_planes != n_planes)) return OVHIP_EINVAL;
    f->hash_on = 1; f->hash_method = method; f->hash_planes = n_planes;      /* (a dry frame has no picture to hash: only remembered) */
    f->hash_expect = expected != NULL;
    if (expected) f->hash_expected = *expected;
    return OVHIP_OK;
}

int
ovhip_frame_picture_hash(const ovhip_frame *f, ovhip_pic_hash_value *computed)
{
    if (!f || !f->hash_done) return OVHIP_EINVAL;
    if (computed) *computed = f->hash_computed;
    return f->hash_done > 0;
}

/* what the three setters below have in common once a format has passed its own checks: the record of output `which` */
static int
out_store(ovhip_frame *f, int which, const void *fmt, size_t fmt_bytes, const ovhip_window *win, void *d0, size_t n0, void *d1, size_t n1)
{
    frame_out *o = &f->outs[which];
    memset(o, 0, sizeof(*o));
    memcpy(&o->fmt, fmt, fmt_bytes);
    if (win) o->win = *win;
    o->dst[0] = d0; o->bytes[0] = n0; o->dst[1] = d1; o->bytes[1] = n1;
    o->on = 1;
    return OVHIP_OK;
}

int
ovhip_frame_set_rgb_output(ovhip_frame *f, const ovhip_rgb_format *fmt, const ovhip_window *win, void *d_dst, size_t dst_bytes)
{
    if (!f) return OVHIP_EINVAL;
    if (!fmt) { f->outs[OUT_RGB].on = 0; return OVHIP_OK; }
    int32_t coef[5], yoff;
    const int r = ovhip_rgb_coefs(fmt, coef, &yoff);          /* the format's refusals come back here, not from a picture's last call */
    if (r != OVHIP_OK) return r;
    if (fmt->layout > OVHIP_RGB_PACKED || fmt->chroma_loc > 5 || !d_dst) return OVHIP_EINVAL;
    if (f->dry) return OVHIP_OK;                               /* (a dry frame has no picture to convert) */
    return out_store(f, OUT_RGB, fmt, sizeof(*fmt), win, d_dst, dst_bytes, NULL, 0);
}

/* What the four table setters below have in common: the conversion's own refusals where the output has one, the table's device, the
 * output's own extra check of what is already set for the next picture, and the dry-frame rule.  conv: read for the surface and the ladder only */
static int
lut_store(ovhip_frame *f, int which, const ovhip_rgb_lut *lut, const ovhip_surface_conv *conv)
{
    if (!f) return OVHIP_EINVAL;
    if (lut) {
        const frame_out *o = &f->outs[which];
        const int has_conv = which == OUT_SURFACE || which == OUT_LADDER;
        int r;
        if (has_conv && (r = ovhip_surface_conv_check_(conv, NULL)) != OVHIP_OK) return r;
        if (!f->dry && !ovhip_rgb_lut_on_ctx_(lut, f->ctx)) return OVHIP_EINVAL;
        /* (a dry frame never has an output set: the two checks below are a live frame's) */
        /* meant: a ladder already set for the next picture is asked for its sample location only -- the reduced pictures keep ITS
         * location --, not checked again through the table */
        if (which == OUT_LADDER && o->on && conv->src_chroma_loc != o->ladder.info.chroma_loc) return OVHIP_EINVAL;
        /* meant: a pyramid already set for the next picture is checked again in full, its levels through THIS table (a U8 level and the peak) */
        if (which == OUT_PYRAMID && o->on
            && (r = ovhip_rgb_pyramid_check(o->pyr.w, o->pyr.h, &o->pyr.info, o->pyr.levels, o->pyr.n, lut->size, lut->peak, NULL)) != OVHIP_OK) return r;
        if (has_conv) f->luts[which].conv = *conv;
    }
    f->luts[which].lut = f->dry ? NULL : lut;                  /* (a dry frame has no picture to convert) */
    return OVHIP_OK;
}

int ovhip_frame_set_rgb_lut(ovhip_frame *f, const ovhip_rgb_lut *lut) { return lut_store(f, OUT_RGB, lut, NULL); }
int ovhip_frame_set_surface_lut(ovhip_frame *f, const ovhip_rgb_lut *lut, const ovhip_surface_conv *conv) { return lut_store(f, OUT_SURFACE, lut, conv); }
int ovhip_frame_set_ladder_lut(ovhip_frame *f, const ovhip_rgb_lut *lut, const ovhip_surface_conv *conv) { return lut_store(f, OUT_LADDER, lut, conv); }
int ovhip_frame_set_rgb_pyramid_lut(ovhip_frame *f, const ovhip_rgb_lut *lut) { return lut_store(f, OUT_PYRAMID, lut, NULL); }

int
ovhip_frame_set_surface_output(ovhip_frame *f, const ovhip_surface_format *fmt, const ovhip_window *win, void *d_dst, size_t dst_bytes)
{
    if (!f) return OVHIP_EINVAL;
    if (!fmt) { f->outs[OUT_SURFACE].on = 0; return OVHIP_OK; }
    const int r = ovhip_surface_format_check_(fmt, NULL);      /* the format's refusals that need no picture come back here */
    if (r != OVHIP_OK) return r;
    if (!d_dst) return OVHIP_EINVAL;
    if (f->dry) return OVHIP_OK;                               /* (a dry frame has no picture to convert) */
    return out_store(f, OUT_SURFACE, fmt, sizeof(*fmt), win, d_dst, dst_bytes, NULL, 0);
}

int
ovhip_frame_set_ladder_output(ovhip_frame *f, const ovhip_reduce_info *info, const ovhip_ladder_rung *rungs, int32_t n)
{
    if (!f) return OVHIP_EINVAL;
    if (!rungs) { f->outs[OUT_LADDER].on = 0; return OVHIP_OK; }
    if (n < 1 || n > OVHIP_LADDER_MAX_RUNGS) return OVHIP_EINVAL;
    ovhip_reduce_info ri;
    memset(&ri, 0, sizeof(ri));
    if (info) ri = *info;
    for (int32_t k = 0; k < n; ++k) {                         /* what needs no picture comes back here */
        const int r = ovhip_surface_format_check_(&rungs[k].fmt, NULL);
        if (r != OVHIP_OK) return r;
        if (!rungs[k].dst) return OVHIP_EINVAL;
    }
    /* meant: a dry frame answers BEFORE the ladder is checked against a size (the pyramid's setter checks first) */
    if (f->dry) return OVHIP_OK;                               /* (a dry frame has no picture to reduce) */
    /* the size the ladder reads: the one the post-process step set now leaves */
    int32_t sw, sh;
    ovhip_post_size_(&f->post, f->w, f->h, &sw, &sh);
    /* with a table set, the table's share too: the location the conversion reads, rung sizes in multiples of 4 */
    const frame_lut *t = &f->luts[OUT_LADDER];
    const int r = t->lut ? ovhip_ladder_lut_check(sw, sh, &ri, rungs, n, &t->conv, t->lut->size, t->lut->peak, NULL) : ovhip_ladder_check(sw, sh, &ri, rungs, n, NULL);
    if (r != OVHIP_OK) return r;
    frame_out *o = &f->outs[OUT_LADDER];
    o->ladder.info = ri; o->ladder.n = n;
    memcpy(o->ladder.rungs, rungs, (size_t)n * sizeof(*rungs));
    o->on = 1;
    return OVHIP_OK;
}

int
ovhip_frame_set_rgb_pyramid_output(ovhip_frame *f, const ovhip_reduce_info *info, const ovhip_rgb_level *levels, int32_t n)
{
    if (!f) return OVHIP_EINVAL;
    if (!levels) { f->outs[OUT_PYRAMID].on = 0; return OVHIP_OK; }
    if (n < 1 || n > OVHIP_PYRAMID_MAX_LEVELS) return OVHIP_EINVAL;
    ovhip_reduce_info ri;
    memset(&ri, 0, sizeof(ri));
    if (info) ri = *info;
    for (int32_t k = 0; k < n; ++k)                           /* what needs no picture comes back here */
        if (!levels[k].dst) return OVHIP_EINVAL;
    /* the size the pyramid reads: the one the post-process step set now leaves */
    int32_t sw, sh;
    ovhip_post_size_(&f->post, f->w, f->h, &sw, &sh);
    const ovhip_rgb_lut *lut = f->luts[OUT_PYRAMID].lut;
    const int r = ovhip_rgb_pyramid_check(sw, sh, &ri, levels, n, lut ? lut->size : 0, lut ? lut->peak : 0, NULL);
    if (r != OVHIP_OK) return r;
    /* meant: a dry frame answers only AFTER the check (the ladder's setter answers before its own) */
    if (f->dry) return OVHIP_OK;                               /* (a dry frame has no picture to reduce: it answers and remembers nothing) */
    frame_out *o = &f->outs[OUT_PYRAMID];
    o->pyr.info = ri; o->pyr.n = n; o->pyr.w = sw; o->pyr.h = sh;
    memcpy(o->pyr.levels, levels, (size_t)n * sizeof(*levels));
    o->on = 1;
    return OVHIP_OK;
}

int
ovhip_frame_set_mvfield_output(ovhip_frame *f, const ovhip_mvfield_format *fmt, void *d_vec, size_t vec_bytes, void *d_info, size_t info_bytes)
{
    if (!f) return OVHIP_EINVAL;
    if (!fmt) { f->outs[OUT_MVFIELD].on = 0; return OVHIP_OK; }
    const int r = ovhip_mvfield_dst_check_(fmt, d_vec, vec_bytes, d_info, info_bytes, NULL);   /* the refusals that need no picture come back here */
    if (r != OVHIP_OK) return r;
    if (f->dry) return OVHIP_OK;                               /* (a dry frame has no motion to export) */
    if (f->band_mode) return OVHIP_EUNSUP;                     /* (meant, and this output's alone: a band-wise picture's arrays live in band arenas: ovhip_job_mvfield) */
    return out_store(f, OUT_MVFIELD, fmt, sizeof(*fmt), NULL, d_vec, vec_bytes, d_info, info_bytes);
}

/* *shown = the picture this picture's outputs show: f->dst after the frame's post-process step (if any: into the context's scratch
 * picture -- f->dst itself is only read; a grain model is derived afresh for every picture).  The step runs ONCE per picture, for the
 * first output that asks (*have); the outputs after it read the same `shown`.  That is sound because the step and all its readers are
 * enqueued by this one thread on this frame's own context and stream, in order, and nothing else writes that context's scratch
 * picture in between: no other output of this context runs until picture_end returns */
static int
frame_shown(ovhip_frame *f, ovhip_pic *shown, int *have)
{
    if (*have) return OVHIP_OK;
    ovhip_post_ post = f->post;
    ovhip_fg_model model;                                      /* (copied by the launch: not needed after it) */
    if (post.kind == OVHIP_POST_GRAIN) {
        const int r = ovhip_fg_derive(&f->fg, &model, NULL);
        if (r != OVHIP_OK) return r;
        post.model = &model;
    }
    const int r = ovhip_post_pic_(f->ctx, &f->dst, &post, shown);
    *have = r == OVHIP_OK;
    return r;
}

/* The end of a picture, for ovhip_frame_submit and the last ovhip_frame_band alike.  r: what the decode gave, after the wait (only the
 * wait marks the picture complete).  j: the job that decoded it; borrowed: j when it is a caller's job bound to this frame's context
 * (ovhip_frame_submit), which goes back to its own context here -- this frame and its context may be destroyed before the job.
 *
 *     publish (+ unpin the references) -> hash of f->dst -> RGB -> surface -> ladder -> RGB pyramid -> motion field -> the settings end -> delivery `out` names
 *
 * The picture is published first: its readers go on while this thread copies it out (the outputs only read; whoever keeps the key
 * alive -- the decoder's DPB, the stream driver's hold -- does so until this call returns).  Each output is complete on the device
 * when its step returns.  A dry frame publishes and touches no output. */
static int
picture_end(ovhip_frame *f, int r, ovhip_job *j, ovhip_job *borrowed, ovhip_frame_output *out)
{
    if (f->dry) { if (f->status) r = f->status; (void)publish(f, r); return r; }
    static const char *const name[N_OUTS] = { "RGB output", "surface output", "ladder output", "RGB pyramid output", "motion field output" };
    frame_out *mvf = &f->outs[OUT_MVFIELD];
    /* the motion field step reads the borrowed job's arrays on this frame's stream: the job goes home behind it */
    const int keep_job = borrowed && mvf->on && r == OVHIP_OK;
    if (borrowed && !keep_job) { int q = ovhip_job_bind(borrowed, NULL); if (q != OVHIP_OK && r == OVHIP_OK) r = fail(f, q, "ovhip_job_bind(home)"); }
    if (f->status) r = f->status;         /* the first error, e.g. a failed reference rather than "callback failed" */
    (void)publish(f, r);
    ovhip_pic shown;
    int have = 0;
    /* the hash is of f->dst, the decoded picture as it was published (its readers only read it, as this does), never of the
     * post-processed copy an output makes.  A value that differs from the expectation is a verdict, not an error */
    f->hash_done = 0;
    if (r == OVHIP_OK && f->hash_on) {
        if ((r = ovhip_pic_hash(f->ctx, &f->dst, f->hash_method, f->hash_planes, &f->hash_computed)) != OVHIP_OK) fail(f, r, "picture hash");
        else f->hash_done = !f->hash_expect || ovhip_pic_hash_equal(&f->hash_computed, &f->hash_expected) ? 1 : -1;
    }
    /* the outputs that show the picture, in the enum's order: the launch (through the output's table when one is set), then the wait */
    for (int k = 0; k < N_LUT_OUTS && r == OVHIP_OK; ++k) {
        const frame_out *o = &f->outs[k];
        const ovhip_rgb_lut *lut = f->luts[k].lut;
        const ovhip_surface_conv *conv = &f->luts[k].conv;
        if (!o->on) continue;
        if ((r = frame_shown(f, &shown, &have)) == OVHIP_OK)
            switch (k) {
            case OUT_RGB:
                r = lut ? ovhip_rgb_lut_launch(f->ctx, &shown, &o->win, &o->fmt.rgb, lut, o->dst[0], o->bytes[0])
                        : ovhip_rgb_launch(f->ctx, &shown, &o->win, &o->fmt.rgb, o->dst[0], o->bytes[0]);
                break;
            case OUT_SURFACE:
                r = lut ? ovhip_surface_lut_launch(f->ctx, &shown, &o->win, conv, &o->fmt.surf, lut, o->dst[0], o->bytes[0])
                        : ovhip_surface_launch(f->ctx, &shown, &o->win, &o->fmt.surf, o->dst[0], o->bytes[0]);
                break;
            case OUT_LADDER:
                r = lut ? ovhip_ladder_lut_launch(f->ctx, &shown, &o->ladder.info, o->ladder.rungs, o->ladder.n, conv, lut)
                        : ovhip_ladder_launch(f->ctx, &shown, &o->ladder.info, o->ladder.rungs, o->ladder.n);
                break;
            default:
                r = ovhip_rgb_pyramid_launch(f->ctx, &shown, &o->pyr.info, o->pyr.levels, o->pyr.n, lut);
                break;
            }
        if (r == OVHIP_OK) r = ovhip_wait_(f->ctx, name[k]);
        if (r != OVHIP_OK) fail(f, r, name[k]);
    }
    if (r == OVHIP_OK && mvf->on && (r = ovhip_job_mvfield_done_(j, &mvf->fmt.mvf, mvf->dst[0], mvf->bytes[0], mvf->dst[1], mvf->bytes[1])) != OVHIP_OK)
        fail(f, r, name[OUT_MVFIELD]);
    outs_clear(f);                        /* whatever happened: a picture that failed takes its destinations with it */
    if (keep_job) { int q = ovhip_job_bind(borrowed, NULL); if (q != OVHIP_OK && r == OVHIP_OK) r = fail(f, q, "ovhip_job_bind(home)"); }
    if (r == OVHIP_OK && out && out->mode != OVHIP_OUT_NONE) {
        PT0();
        /* (a mode that is none of the three is refused before anything is launched for it) */
        r = out->mode < OVHIP_OUT_DIGEST || out->mode > OVHIP_OUT_PACKED ? OVHIP_EINVAL : frame_shown(f, &shown, &have);
        if (r == OVHIP_OK) r = ovhip_deliver_(f->ctx, &shown, out);
        PT(f->pt_output);
        if (r != OVHIP_OK) fail(f, r, "picture output");
    }
    return r;
}

int
ovhip_frame_submit(ovhip_frame *f, ovhip_job *job, const ovhip_pic *intra, const ovhip_job_params *params, ovhip_frame_output *out)
{
    if (!f || !params || !f->live) return OVHIP_EINVAL;
    PT0();
    int r = f->status;                    /* a latched recorder error: the picture is published as failed, never launched */
    ovhip_job *j = job ? job : f->job;
    if (f->dry) {
        /* dry: the same waits and the same publication, no launches, no output */
        if (r == OVHIP_OK) r = acquire_refs(f);
        trace(f, OVHIP_FE_SUBMIT, f->key, 0, (int64_t)n_refined_units(f), f->n_refs, r);
        return picture_end(f, r, NULL, NULL, NULL);
    }
    trace(f, OVHIP_FE_SUBMIT, f->key, 0, (int64_t)n_refined_units(f), f->n_refs, r);
    if (r == OVHIP_OK && !j) r = fail(f, OVHIP_EINVAL, "ovhip_frame_submit: nothing was recorded");
    if (r == OVHIP_OK && job) r = fail(f, ovhip_job_bind(job, f->ctx), "ovhip_job_bind");
    if (r == OVHIP_OK) {
        ovhip_job_params pr = *params;
        /* the references are waited for on the host, by this thread, after the uploads have been enqueued (no barrier in the
         * stream: a blocked stream blocks the hardware queue it shares) */
        pr.before_launch = before_launch_cb; pr.before_launch_user = f;
        r = ovhip_job_flush(j, &f->dst, f->ref_pic, (uint32_t)f->n_refs, intra, &pr);
        if (r != OVHIP_OK) fail(f, r, "ovhip_job_flush");
        if (PT_ON()) {
            ovhip_job_stats st;
            if (ovhip_job_last_stats(j, &st) == OVHIP_OK) { f->pt_fl_prepare += 1e-6 * st.host_us_prepare; f->pt_fl_upload += 1e-6 * st.host_us_upload; f->pt_fl_refs += 1e-6 * st.host_us_wait; f->pt_fl_launch += 1e-6 * st.host_us_launch; }
        }
        /* ONLY the wait marks the picture complete: it may run the ordered pass a second time */
        const double tw0 = PT_ON() ? mono_s() : 0.0;
        int q = ovhip_job_wait(j);
        if (PT_ON()) f->pt_job_wait += mono_s() - tw0;
        f->done_at = mono_s();
        if (q != OVHIP_OK && r == OVHIP_OK) r = fail(f, q, "ovhip_job_wait");
    }
    r = picture_end(f, r, j, job, out);
    PT(f->pt_submit); f->pn_pics += !f->band_mode;
    return r;
}

/* ------------------------------------------------------------------------------------------------ band-wise submission
 * ovhip_job_band under the device DPB's row progress: a band goes to the device when the rows its units read are final in every
 * reference picture (the producer's posted records, seen complete on the HOST: no barrier enters the stream); a band that is not
 * there yet is simply left to the next call, which takes everything recorded since the last band that went -- the parse never waits,
 * except in the picture's last call.  Mirrors rcn_inter_synchronization (rcn_inter.c:131-146) + ovdpb_report_decoded_ctu_line
 * (dpb.c:1309-1323) at band granularity. */
int
ovhip_frame_set_band_mode(ovhip_frame *f, int on)
{
    if (!f) return OVHIP_EINVAL;
    f->band_mode = on != 0;
    if (on && !f->dry && f->job && !getenv("OVVC_HIP_NO_RESERVE")) return fail(f, ovhip_job_band_reserve(f->job), "ovhip_job_band_reserve");
    return OVHIP_OK;
}

/* luma rows [0, need[i]) of reference i are read by the units [c0, c1) (0: not used): the unit's last row + the vertical vector +
 * 8 rows -- the 8-tap window's 4 rows below, DMVR's 2-sample search range, BDOF's extension, and the chroma windows (2 chroma rows
 * = 4 luma rows below the co-located row) all stay inside it */
static void
units_need_rows(ovhip_frame *f, const ovhip_band_counts *c0, const ovhip_band_counts *c1, int only_dmvr, int32_t *need)
{
    ovhip_recorder *rec = ovhip_frame_recorder(f);
    size_t n = 0;
    for (int i = 0; i < MAX_REFS; ++i) need[i] = 0;
    if (!rec) return;
#define NEED(ref, y_last, mvy) do { int32_t v_ = (int32_t)(y_last) + ((mvy) >> 4) + 1 + 8; if (v_ < 1) v_ = 1; if (v_ > f->h) v_ = f->h; \
                                    if ((ref) < MAX_REFS && need[ref] < v_) need[ref] = v_; } while (0)
    for (int pass = 0; pass < 2; ++pass) {
        const ovhip_mc_unit *u = pass ? ovhip_rec_mcx_units(rec, &n) : ovhip_rec_mc_units(rec, &n);
        const size_t a = pass ? c0->n_mcx : c0->n_mc, b = pass ? c1->n_mcx : c1->n_mc;
        for (size_t i = a; i < b && i < n; ++i) {
            if (only_dmvr && !(u[i].flags & OVHIP_MC_DMVR)) continue;
            const int y_last = u[i].y + u[i].h - 1;
            if (u[i].dir & 1) NEED(u[i].ref0, y_last, u[i].mv0y);
            if (u[i].dir & 2) NEED(u[i].ref1, y_last, u[i].mv1y);
        }
    }
    if (!only_dmvr) {
        const ovhip_aff_unit *au = ovhip_rec_aff_units(rec, &n);
        size_t ns = 0;
        const int32_t *side = ovhip_rec_aff_side(rec, &ns);
        for (size_t i = c0->n_aff; i < c1->n_aff && i < n; ++i) {
            const int n_sub = (au[i].w / 4) * (au[i].h / 4) + (au[i].w / 8) * (au[i].h / 8);
            const int y_last = au[i].y + au[i].h - 1;
            int32_t m0 = -(1 << 30), m1 = -(1 << 30);
            for (int k = 0; k < n_sub && (size_t)au[i].side_off + 4 * (size_t)k + 3 < ns; ++k) {
                const int32_t *q = side + au[i].side_off + 4 * k;
                if (q[1] > m0) m0 = q[1];
                if (q[3] > m1) m1 = q[3];
            }
            if (m0 == -(1 << 30)) m0 = m1 = f->h * 16;                 /* (no vectors found: the whole picture) */
            if (au[i].dir & 1) NEED(au[i].ref0, y_last, m0);
            if (au[i].dir & 2) NEED(au[i].ref1, y_last, m1);
        }
    }
#undef NEED
}

/* 1: every reference has the rows (pinned, f->ref_pic[] filled), 0: not yet (block == 0 only), < 0: error */
static int
refs_rows_ready(ovhip_frame *f, const int32_t *need, int block)
{
    for (int i = 0; i < f->n_refs; ++i) {
        /* a table entry none of these units reads stays a placeholder of the right geometry (the launchers check every entry of the
         * table; no unit of the launch indexes this one): the picture being decoded itself */
        if (!need[i]) { if (!f->ref_pinned[i]) f->ref_pic[i] = f->dst; continue; }
        void *ev = NULL;
        ovhip_pic pic;
        int r = ovhip_dpb_rows_tag(f->dpb, f->ref_key[i], f->ref_tag[i], f->dev, need[i], block, !f->ref_pinned[i], &pic, &ev);
        if (r < 0) return fail(f, r, r == OVHIP_EREF ? "a reference picture failed to decode" : "reference picture unknown to the device DPB");
        if (!r) return 0;
        f->ref_pic[i] = pic; f->ref_pinned[i] = 1;
        if (ev) {
            r = ovhip_dpb_wait_copy(f->dpb, f->dev, ev);
            if (r != OVHIP_OK) return fail(f, r, "transfer of a reference picture");
        }
    }
    return 1;
}

/* rows a band-wise job has made final once the band ending at `end` has had its filters (ovvc_band.hip: deblocking leaves
 * the 8 rows above a band's end to the next band, SAO and ALF follow in steps of 8 rows) -- what a dry frame posts */
static int32_t
dry_rows_after(int32_t end)
{
    int32_t v = end - 8 - 1;
    v = v <= 0 ? 0 : v & ~7;
    v -= 3;
    return v <= 0 ? 0 : v & ~7;
}

static int frame_band(ovhip_frame *f, const ovhip_job_params *params, int32_t row_end, int32_t last, ovhip_frame_output *out, const ovhip_band_counts *upto, int block);

int ovhip_frame_band(ovhip_frame *f, const ovhip_job_params *params, int32_t row_end, int32_t last, ovhip_frame_output *out)
{
    return frame_band(f, params, row_end, last, out, NULL, last != 0);
}

int ovhip_frame_band_upto(ovhip_frame *f, const ovhip_job_params *params, int32_t row_end, const ovhip_band_counts *upto, int32_t block)
{
    return frame_band(f, params, row_end, 0, NULL, upto, block != 0);
}

static int
frame_band(ovhip_frame *f, const ovhip_job_params *params, int32_t row_end, int32_t last, ovhip_frame_output *out, const ovhip_band_counts *upto, int block)
{
    if (!f || !params || !f->live) return OVHIP_EINVAL;
    int r = f->status;
    if (r != OVHIP_OK) {
        /* a latched error: nothing more goes to the device; the last call publishes the picture as failed */
        trace(f, OVHIP_FE_BAND, f->key, 0, row_end, last, r);
        if (last) (void)picture_end(f, r, NULL, NULL, NULL);
        return r;
    }
    if (last) row_end = f->h;
    if (row_end > f->h) row_end = f->h;
    ovhip_job *j = f->dry ? NULL : ovhip_frame_job(f);
    if (!f->dry && !j) return fail(f, OVHIP_EINVAL, "ovhip_frame_band: no job");
    /* the device is behind (the band before this one is still being reconstructed): this band is left to the next call, which takes
     * its rows too -- fewer, fuller launches when the device is the slower side; an I picture's wavefront then spans the rows */
    /* (a picture of more CTU rows than the job keeps bands -- 8K with 32-sample CTUs -- goes on in fewer, larger bands: the rest is
     * left to the last call) */
    if (!last && f->n_bands >= 90) { f->n_deferred++; trace(f, OVHIP_FE_BAND, f->key, 0, row_end, last, 0); return 0; }
    if (!block && j && f->n_bands && ovhip_job_band_busy(j)) { f->n_deferred++; trace(f, OVHIP_FE_BAND, f->key, 0, row_end, last, 0); return 0; }
    ovhip_band_counts now;
    ovhip_rec_counts(ovhip_frame_recorder(f), &now);
    if (upto) {
        const uint32_t *u = &upto->n_tb, *m = &now.n_tb, *lo = &f->band_prev.n_tb;
        for (int i = 0; i < 10; ++i) if (u[i] > m[i] || u[i] < lo[i]) return fail(f, OVHIP_EINVAL, "ovhip_frame_band_upto: counts outside what has been recorded since the last band");
        now = *upto;
    }
    int32_t need[MAX_REFS];
    { PT0();
    units_need_rows(f, &f->band_prev, &now, 0, need);
    r = refs_rows_ready(f, need, block);
    if (last) PT(f->pt_final_refs); else PT(f->pt_band_refs); }
    if (r < 0) { trace(f, OVHIP_FE_BAND, f->key, 0, row_end, last, r); if (last) (void)picture_end(f, r, NULL, NULL, NULL); return r; }
    if (!r) { f->n_deferred++; trace(f, OVHIP_FE_BAND, f->key, 0, row_end, last, 0); return 0; }
    int32_t rows = 0; void *ev = NULL; const volatile uint32_t *abw = NULL;
    if (f->dry) {
        rows = last ? f->h : dry_rows_after(row_end);
        r = OVHIP_OK;
    } else {
        PT0();
        r = ovhip_job_band(j, &f->dst, f->ref_pic, (uint32_t)f->n_refs, params, upto, row_end, last);
        PT(f->pt_band_job);
        if (r != OVHIP_OK) fail(f, r, "ovhip_job_band");
        else (void)ovhip_job_band_progress(j, &rows, &ev, &abw);
    }
    f->band_prev = now; f->band_row_prev = row_end; f->n_bands++;
    trace(f, OVHIP_FE_BAND, f->key, 0, row_end, last, r == OVHIP_OK ? 1 : r);
    if (r == OVHIP_OK && !last && rows > f->band_rows_posted) {
        (void)ovhip_dpb_post_rows(f->dpb, f->key, rows, ev, abw);
        f->band_rows_posted = rows;
    }
    if (!last) return r == OVHIP_OK ? 1 : r;
    /* the picture's end: as ovhip_frame_submit -- only the wait marks it complete */
    if (r == OVHIP_OK && !f->dry) {
        PT0();
        int q = ovhip_job_wait(j);
        PT(f->pt_job_wait);
        f->done_at = mono_s();
        if (q != OVHIP_OK) r = fail(f, q, "ovhip_job_wait");
    }
    f->pn_pics++;
    r = picture_end(f, r, j, NULL, out);
    return r == OVHIP_OK ? 1 : r;
}

int
ovhip_frame_band_stats(const ovhip_frame *f, int32_t *n_bands, int32_t *n_deferred)
{
    if (!f) return OVHIP_EINVAL;
    if (n_bands) *n_bands = f->n_bands;
    if (n_deferred) *n_deferred = f->n_deferred;
    return OVHIP_OK;
}
