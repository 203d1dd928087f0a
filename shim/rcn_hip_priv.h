/* rcn_hip_priv.h -- what the units of the override block share (rcn_hip.h): the reference's headers, the per-OVCTUDec
 * side-table entry, the way every slot finds it, and the few functions one unit calls in another.  Nothing here is exported.
 *
 *   rcn_hip.c       layout assertions, side table, installer, management / accessor entry points, profile
 *   rcn_hip_rec.c   the slots that turn one decoder call into one recorder call; SAO / ALF / LMCS capture; the two row hooks
 *   rcn_hip_sub.c   caller mode, unpatched reference: sub-block calls stitched back into coding units, row step that waits
 *   rcn_hip_cu.c    caller mode, shim/caller.patch applied: whole coding units, CTU-row reports, row step that never waits
 *   rcn_hip_pic.c   the picture on the device: begin, refined rows, bands, flush, output
 * A build compiles exactly one of rcn_hip_sub.c / rcn_hip_cu.c (shim/Makefile, CALLER_PATCH=1).
 */
#ifndef OVVC_RCN_HIP_PRIV_H
#define OVVC_RCN_HIP_PRIV_H

#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ovdefs.h"
#include "ovframe.h"
#include "ovdpb.h"
#include "dec_structures.h"
#include "ctudec.h"
#include "rcn_structures.h"
#include "rcn.h"
#include "drv.h"
#include "drv_utils.h"
#include "dbf_utils.h"
#include "slicedec.h"
#include "nvcl_structures.h"
#include "ovdec_internal.h"          /* struct MVPlane */
#include "ovlog.h"

#include "ovvc_hip.h"
#include "rcn_hip.h"

#ifndef BITDEPTH
#error "compile with -DBITDEPTH=10 (the table's sample type is a compile-time macro, bitdepth.h:36-40)"
#endif

#define HIP_PRIV __attribute__((visibility("hidden")))

/* private to the reference's .c files (drv_affine_mvp.c:3303-3308 and rcn_inter.c:1128-1134): the slot prototypes only forward-declare
 * it, a back-end has to restate the layout */
struct PROFInfo { int16_t dmv_scale_h_0[16], dmv_scale_v_0[16], dmv_scale_h_1[16], dmv_scale_v_1[16]; };

/* ------------------------------------------------------------------------------------ side table */
enum { PEND_NONE = 0, PEND_AFFINE, PEND_BDOF };

#define MAX_MARKS 136          /* CTU rows of a picture: 8192 / 64 + some */
struct hip_entry {
    const OVCTUDec *key;
    struct RCNFunctions scalar;          /* the table as the scalar fill left it */
    uint8_t ict_type, lmcs_flag;
    ovhip_recorder *rec;                 /* the frame thread's recorder, or the bound one in record-only mode */
    int record_only;
    ovhip_frame *fr; int dev;            /* this OVCTUDec's frame thread on the device path (include/ovvc_hip.h) and its logical device */
    int pic_w, pic_h, log2_ctu, nb_ctu_w, nb_ctu_h;
    const OVFrame *frame;                /* picture being decoded */
    int ctus_left;                       /* CTUs of that picture whose rect entries (tiles) have not ended yet: 0 = no picture open      */
    int whole_pic_entry;                 /* the entry being decoded covers the picture (no tile borders inside)                          */
    int err;
    const OVPicture *refs[16]; int n_refs;
    uint32_t scale_set;                 /* reference-table slots whose scale this picture already handed to the recorder */
    ovhip_lmcs_luts luts; int have_luts, lmcs_region_live;
    ovhip_sao_ctu *sao; ovhip_alf_ctu *alf; size_t n_ctu; int sao_on, alf_on;
    int16_t alf_cc[2][4][8];
    size_t n_refined;                    /* refined units recorded (BDOF and DMVR: the index space of the device's results)      */
    size_t dmvr_done;                    /* ... whose vectors are already in the picture's TMVP planes                            */
    size_t row_mark;                     /* ... recorded when the last row-end hook ran                                           */
    int band_on;                         /* this picture goes to the device band by band (ovhip_frame_band), not at its end        */
    uint32_t n_bands_sent, n_bands_deferred;
    /* what had been recorded when CTU row y had just been parsed (y = index: rows_parsed - 1): the picture's last hook works through
     * the rows its reference pictures had not reached during the parse with these (final_progressive, rcn_hip_cu.c) */
    struct { ovhip_band_counts counts; size_t n_refined; } marks[MAX_MARKS]; int n_marks, rows_sent;
    /* prediction calls being collected into one CU (rcn_hip_sub.c; with the caller patch only the affine field is used, as scratch) */
    struct {
        int kind, x0, y0, n, cols, rows_done, cur_col;
        uint8_t inter_dir, prof_dir, bcw, ref_idx0, ref_idx1;
        int32_t mv0[32 * 32 * 2], mv1[32 * 32 * 2];       /* affine: sub-block field, row stride 32 */
        struct PROFInfo prof;
        OVMV bmv0, bmv1; int bx[64], by[64], bl2w, bl2h;  /* BDOF blocks */
    } pend;
    /* the luma of an affine CU has been recorded (with its chroma): the rcn_mcp_b_c(3,3) calls of the SAME CU that follow
     * carry nothing new.  Rectangle in CTU-local luma samples; any other slot call ends it. */
    int aff_c_live, aff_c_x0, aff_c_y0, aff_c_x1, aff_c_y1;
    struct { int depth; uint64_t t0, ticks_hooks, ticks_device, n_calls; } prof;
    /* CTU-row reports held back until the row's collocated motion vectors are final (rcn_report_ctu_line, shim/caller.patch; rcn_hip_cu.c) */
    struct { OVPicture *pic; int y, x0, x1; size_t need; } reports[160];
    int n_reports; size_t report_need; uint64_t n_reports_deferred;
    /* a CIIP CU whose planar tasks wait for the CU's transform unit (which carries their residual); closed without one by
     * the next slot call that is not that transform unit */
    struct { int live, x0, y0, log2_w, log2_h, has_c; ovhip_itask tl, tc; } ciip;
    /* an intra-block-copy CU (rcn_ibc_l, then rcn_ibc_c unless luma only) whose blocks wait for the CU's transform tree, which always
     * follows (vcl_transform_unit.c:1889-1959) and records prediction and residual as ONE ordered task per block; x0, y0: CTU-local.
     * Any other slot call in between, or a tree of another CU, latches an error: no CU is left unpredicted silently */
    struct { int live, x0, y0; ovhip_ibc_desc cu; } ibc;
    int entry_x0;                        /* left edge (luma samples) of the rect entry being decoded                                     */
};

/* ---- where a frame thread's time goes inside the back-end (ovhip_shim_set_profile): every installed hook brackets itself; the
 * device half (begin_picture, the row steps, flush_picture: waits for reference pictures, launches, ovhip_job_wait, the copy into the
 * OVFrame) is counted apart from the recording.  Off: one predictable branch per hook. */
extern HIP_PRIV int g_prof_on;
#if defined(__x86_64__)
static inline uint64_t prof_tick(void) { return __builtin_ia32_rdtsc(); }
#else
#include <time.h>
static inline uint64_t prof_tick(void) { struct timespec t; clock_gettime(CLOCK_MONOTONIC, &t); return (uint64_t)t.tv_sec * 1000000000ull + (uint64_t)t.tv_nsec; }
#endif

/* Every slot call starts here (the table has no user pointer).  The common case -- the same OVCTUDec as this thread's last call,
 * no entry released since -- is two thread-local compares; only a miss takes the mutex and scans (r2: mutex + scan on every call). */
extern HIP_PRIV unsigned g_entries_gen;
/* (one object: one thread-local address computation per slot call) */
extern HIP_PRIV __thread struct hip_tls { const OVCTUDec *key; struct hip_entry *entry; unsigned gen; } tls_last;
HIP_PRIV struct hip_entry *entry_miss(const OVCTUDec *c, int create);

static inline struct hip_entry *
entry_of(const OVCTUDec *c, int create)
{
    const struct hip_tls *t = &tls_last;
    if (t->key == c && t->entry && t->gen == __atomic_load_n(&g_entries_gen, __ATOMIC_ACQUIRE)) return t->entry;
    return entry_miss(c, create);
}

/* first error of the picture (code < 0), said to the decoder's log */
HIP_PRIV void latch(struct hip_entry *e, int code, const char *what);

struct prof_scope { struct hip_entry *e; };
static inline struct prof_scope
prof_enter(struct hip_entry *e)
{
    struct prof_scope p = { NULL };
    if (g_prof_on && e) { p.e = e; if (e->prof.depth++ == 0) { e->prof.t0 = prof_tick(); e->prof.n_calls++; } }
    return p;
}
static inline void prof_leave(struct prof_scope *p) { if (p->e && --p->e->prof.depth == 0) p->e->prof.ticks_hooks += prof_tick() - p->e->prof.t0; }
#define PROF(e) struct prof_scope prof_scope_ __attribute__((cleanup(prof_leave))) = prof_enter(e)
/* the device half inside a hook */
#define PROF_DEVICE_BEGIN(e) const uint64_t prof_dev_t0_ = g_prof_on ? prof_tick() : 0
#define PROF_DEVICE_END(e)   do { if (g_prof_on) (e)->prof.ticks_device += prof_tick() - prof_dev_t0_; } while (0)

/* Identity of a picture for the device DPB, beside its OVFrame pointer (which the frame pool hands to one picture after another):
 * coded video sequence + picture order count, never 0 (include/ovvc_hip.h, ovhip_dpb_begin_tag) */
static inline uint64_t pic_tag(const OVPicture *p) { return (((uint64_t)p->cvs_id << 32) | (uint32_t)p->poc) + 1; }

HIP_PRIV void pend_close(struct hip_entry *e, OVCTUDec *c);          /* the caller mode's */
HIP_PRIV void ciip_close(struct hip_entry *e, OVCTUDec *c);          /* rcn_hip_rec.c */
HIP_PRIV void ibc_orphan(struct hip_entry *e);                       /* rcn_hip_rec.c: the stashed IBC CU got no transform tree */

/* every hook that is not part of the CU being collected closes it first */
#define ENTER(c)                                               \
    struct hip_entry *e = entry_of((c), 0);                    \
    if (!e || !e->rec) return;                                 \
    PROF(e);                                                   \
    e->aff_c_live = 0;                                         \
    if (e->ciip.live) ciip_close(e, (OVCTUDec *)(c));          \
    if (e->ibc.live) ibc_orphan(e);                            \
    if (e->pend.kind) pend_close(e, (OVCTUDec *)(c))

/* ---- rcn_hip_rec.c */
HIP_PRIV void rec_install(struct RCNFunctions *f);
/* descriptor of a prediction unit whose vectors come with their reference indices apart; of an affine CU whose sub-block field lies in
 * e->pend.mv0 / mv1 (row stride 32) */
HIP_PRIV void fill_pu(struct hip_entry *e, const OVCTUDec *c, ovhip_pu_desc *d, int x0, int y0, int log2_w, int log2_h, int inter_dir,
                      OVMV mv0, OVMV mv1, const OVPicture *p0, const OVPicture *p1);
HIP_PRIV void fill_pu_idx(struct hip_entry *e, const OVCTUDec *c, ovhip_pu_desc *d, int x0, int y0, int log2_w, int log2_h, int inter_dir,
                          OVMV mv0, OVMV mv1, int ref_idx0, int ref_idx1);
HIP_PRIV void fill_affine(struct hip_entry *e, const OVCTUDec *c, ovhip_affine_desc *d, int x0, int y0, int log2_w, int log2_h, int inter_dir,
                          int bcw_idx_plus1, int prof_dir, int ref_idx0, int ref_idx1, const struct PROFInfo *prof);
HIP_PRIV int  params_alloc(struct hip_entry *e, const OVCTUDec *c, const struct RectEntryInfo *einfo);
HIP_PRIV void sao_row(struct hip_entry *e, const OVCTUDec *c, const struct RectEntryInfo *einfo, int ctb_y);
HIP_PRIV void alf_row(struct hip_entry *e, const OVCTUDec *c, const struct RectEntryInfo *einfo, int ctb_y);
HIP_PRIV void alf_cc_capture(struct hip_entry *e, const struct ALFInfo *ai);

/* ---- the caller mode (rcn_hip_sub.c or rcn_hip_cu.c) */
HIP_PRIV void mode_install(struct RCNFunctions *f);
HIP_PRIV void mode_begin(struct hip_entry *e);                           /* a picture begins on this entry */
HIP_PRIV void mode_row(struct hip_entry *e, OVCTUDec *c);                /* a CTU row has been parsed, more follow */
HIP_PRIV void mode_end(struct hip_entry *e, OVCTUDec *c);                /* the picture's last hook: every refined vector final, every row reported */

/* ---- rcn_hip_pic.c */
extern HIP_PRIV int g_band_rows;
HIP_PRIV void pic_knobs(void);
HIP_PRIV void begin_picture(struct hip_entry *e, const OVFrame *f, const struct RectEntryInfo *einfo);
/* `rows` CTU rows of the entry being decoded are parsed; `last`: this is the picture's last hook */
HIP_PRIV void rows_parsed(struct hip_entry *e, OVCTUDec *c, const struct RectEntryInfo *einfo, int rows, int last);
/* refine up to `need` units now (exact: no further): returns the units refined so far, their vectors in the collocated planes; < 0 latched */
HIP_PRIV int64_t refine_now(struct hip_entry *e, OVCTUDec *c, size_t need, int exact);
HIP_PRIV void apply_done_cells(struct hip_entry *e, OVCTUDec *c, int64_t done);
HIP_PRIV void picture_params(struct hip_entry *e, OVCTUDec *c, ovhip_job_params *pr, int by_flags);
HIP_PRIV void pic_release(struct hip_entry *e);

#endif
