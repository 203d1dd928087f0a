// ovvc_job.hip.h -- private: what the picture job's two translation units share.  ovvc_picture.hip holds the job's life cycle, the
// flush of a whole picture, the launch chain and the flow admission policy; ovvc_band.hip the band-wise submission of a picture that is
// still being parsed.  Nothing declared here is exported from the library.
#pragma once
#include "ovvc_common.hip.h"
#include "flow_state.hip.h"
#include <stdlib.h>

struct BandState;                        // ovvc_band.hip

struct DevBuf { void *p; size_t cap; };

enum { B_TB, B_COEF, B_MC, B_MCX, B_MV, B_AFF, B_SIDE, B_REG, B_SCALE, B_EV, B_EH, B_PARAM, B_CLASS, B_CIIP, B_ITASK, B_ICTU, B_IITEM, B_TMVP, B_RPR, B_AFFR, B_COUNT };

struct ovhip_job {
    ovhip_ctx *ctx;
    ovhip_ctx *home;                     // the context the job was created on (ovhip_job_bind(job, NULL) returns to it)
    int32_t w, h;
    ovhip_recorder *rec;
    DevBuf dev[B_COUNT];
    ovhip_pic tmp;                       // SAO destination / ALF source
    ovhip_pic res;                       // residuals of the ordered tasks (allocated with the first picture that has any)
    uint32_t *d_sync; uint32_t epoch;    // CTU flags of the one-launch ordered pass (zeroed once; a new epoch per picture)
    uint32_t *d_flow;                    // unit state words of the flow launch (zeroed once)
    uint32_t *items_host; size_t items_cap;   // pinned: items of the flow launch (items_cap in bytes)
    uint32_t *abort_host;                // pinned word the ordered pass writes when a bounded wait expired
    char *param_host; size_t param_cap;  // pinned staging of the picture-level tables
    int32_t *mv_host; size_t mv_cap;     // pinned: refined vectors, 4 int32 per refined unit
    struct { int valid, has_intra; ovhip_pic dst, refs[16], intra; uint32_t n_refs; ovhip_job_params pr; } again;   // the last flush's arguments
    uint32_t n_retries;                  // second passes of the last picture (ovhip_job_wait)
    int flow_launched;                   // the last flush had a flow launch (flow_launch_clean: a clean one counts towards the decay of g_flow_shift)
    int test_abort, test_abort_seen;     // ovhip_job_test_abort_next_flow (a forced abort does not count as evidence of starvation)
    ovhip_tmvp_cell *tmvp_host; size_t tmvp_cap, n_tmvp;   // pinned: TMVP plane cells of the refined units (ovhip_job_params.tmvp_cells)
    size_t n_mv;                         // units covered by the last flush / eager pass
    size_t dmvr_first;                   // refined units [0, dmvr_first) already went through the eager search
    size_t rows_end; int rows_pending;   // an eager pass is in flight: it covers [.., rows_end), ev_rows follows its copies
    hipEvent_t ev_rows;
    hipEvent_t ev_h2d, ev_done;
    int flow_on_device;                  // the last full flush uploaded the flow launch's item list (a resident replay may use it)
    int flushed;                         // ev_* recorded at least once
    const void *packed_prev[24];         // where the last full flush placed the arrays that rode in the parameter block
    int resident;                        // this flush reuses the device copies of the previous one (OVHIP_STAGE_RESIDENT)
    // ovhip_job_mvfield: where the last whole-picture flush placed the five unit lists and the side arena, their counts, and where its
    // k_mcxa left the refined vectors (device memory, or the page-locked array the device reads as well; nullptr: the prediction stage
    // did not run).  valid from a successful flush to the next ovhip_job_begin
    struct { int valid; ovhip_mvfield_src src; } mvf;
    ovhip_job_stats st;
    struct BandState *bs;                // band-wise submission (ovhip_job_band): allocated with the first band of the job's life
    // optional: HIP-event bracket around ONE launch group of the flush (ovhip_job_time_stage)
    int t_stage;                         // OVHIP_TIME_* or -1
    hipEvent_t t_ev[32][2]; uint8_t t_pending[32]; int t_next;
    double t_sum_ms; uint64_t t_count;
};

#define CHK(x) do { int r__ = (x); if (r__ != OVHIP_OK) return r__; } while (0)

// what a flush and a band both take from the parameter block: the stages (0: all of them), the CTU size (0: 128), whether SAO / ALF run
struct Switches { uint32_t stages; int log2_ctu, sao_on, alf_on; };
static inline Switches switches_of(const ovhip_job_params *pr)
{
    const uint32_t stages = pr->stages ? pr->stages : UINT32_MAX;
    return Switches{ stages, pr->log2_ctu_s ? pr->log2_ctu_s : 7, pr->sao && (stages & OVHIP_STAGE_SAO), pr->alf_ctus && (stages & OVHIP_STAGE_ALF) };
}
static inline bool alf_tables_missing(const ovhip_job_params *pr)
{
    return !pr->alf_luma_coeff || !pr->alf_luma_clip || !pr->alf_chroma_coeff || !pr->alf_chroma_clip || !pr->alf_cc_coeff;
}

// a staging block in 256-byte slots (one pinned block, one H2D)
struct Layout {
    size_t o = 0;
    size_t put(size_t bytes) { const size_t at = o; o += (bytes + 255) & ~(size_t)255; return at; }
};

// the picture-level tables: ALF luma coefficients / clipping values, chroma coefficients / clipping values, CC-ALF coefficients, the LMCS
// forward / inverse LUTs -- their slots in a staging block, their fill, the ALF launch's view of them at the block's device address
enum { T_LCOEF, T_LCLIP, T_CCOEF, T_CCLIP, T_CC, T_FWD, T_BWD, T_COUNT };
struct Tables { size_t at[T_COUNT]; };
static const size_t TABLE_BYTES[T_COUNT] = { 24 * OVHIP_ALF_LUMA_SET_SIZE * 2, 24 * OVHIP_ALF_LUMA_SET_SIZE * 2, 8 * 7 * 2, 8 * 7 * 2, 2 * 4 * 8 * 2, 2048, 2048 };

static inline Tables tables_put(Layout &L, bool alf, bool lmcs)
{
    Tables t;
    for (int k = 0; k < T_COUNT; ++k) t.at[k] = L.put((k < T_FWD ? alf : lmcs) ? TABLE_BYTES[k] : 0);
    return t;
}

static inline void tables_fill(char *h, const Tables &t, const ovhip_job_params *pr, bool alf, bool lmcs)
{
    const void *src[T_COUNT] = { pr->alf_luma_coeff, pr->alf_luma_clip, pr->alf_chroma_coeff, pr->alf_chroma_clip, pr->alf_cc_coeff,
                                 lmcs ? pr->lmcs->fwd_lut : nullptr, lmcs ? pr->lmcs->bwd_lut : nullptr };
    for (int k = 0; k < T_COUNT; ++k) if (k < T_FWD ? alf : lmcs) memcpy(h + t.at[k], src[k], TABLE_BYTES[k]);
}

static inline ovhip_alf_pic alf_pic_at(const char *d, const Tables &t, const ovhip_alf_ctu *ctus, uint8_t *class_scratch, int log2_ctu)
{
    auto tab = [&](int k) { return (const int16_t *)(d + t.at[k]); };
    return ovhip_alf_pic{ ctus, tab(T_LCOEF), tab(T_LCLIP), tab(T_CCOEF), tab(T_CCLIP), tab(T_CC), class_scratch, log2_ctu };
}

// Where a submission's arrays are on the device -- what staging leaves for the launches.  The flush and the band arrive at it by their
// own policies (the flush packs arrays up to a limit into the parameter block and gives the larger ones a copy of their own, or reuses
// the previous placement for a resident replay; a band cuts one block out of its arena); the launches only see the result.
struct Placement {
    const void *at[B_COUNT];              // the first element of this submission's slice of each recorder array (B_MV: where k_mcxa leaves the vectors)
    const char *block;                    // the staging block: the picture-level tables and the filters' CTU parameters are inside it
    Tables tabs; size_t o_sao, o_alf;     // ... at these offsets
};

// ---- the launch chain, one implementation for ovhip_job_flush (the whole picture) and ovhip_job_band (a band of CTU rows) ----
// What one submission reads.  Device pointers are rebased to the recorder's indexing: the commands' own indices (coefficient / side-arena
// offsets, region numbers) stay what the recorder wrote, and a band's slice is addressed through a pointer moved back by its first index.
struct Chain {
    ovhip_job *j;
    ovhip_job *timer;                     // whose ovhip_job_time_stage brackets the launch groups (nullptr: none; band-wise submission)
    const ovhip_pic *dst, *res;           // res: where the residuals of the ordered tasks wait for their prediction, or nullptr
    int log2_ctu;
    const ovhip_lmcs_luts *luts; const uint16_t *d_fwd; int16_t *d_scales;
    const ovhip_mc_unit *d_mc, *d_mcx; uint32_t n_mc, n_mcx;
    const ovhip_aff_unit *d_aff; uint32_t n_aff; const int32_t *d_side;
    const ovhip_rpr_unit *d_rpr; uint32_t n_rpr;                      // units that read a reference of another size (k_mc_rpr)
    const ovhip_aff_rpr_unit *d_affr; uint32_t n_affr;                // affine units that do (k_mca_rpr; their side data in d_side)
    const ovhip_tb_cmd *d_tb; size_t cls[4], tiny[4][4]; const int16_t *d_coef;
    const ovhip_lmcs_region *d_reg; uint32_t reg0, n_reg;             // this submission's regions: [reg0, reg0 + n_reg)
    const ovhip_itask *d_it, *h_it; uint32_t n_it;                    // the level-sorted tasks (h_it: host copy, level geometry)
    const uint32_t *lv_start; uint32_t n_lv;
    const uint32_t *d_items; uint32_t n_items;                        // n_items != 0: a flow launch runs the ordered pass
    int prepared;                                                     // (chain_residual) the chroma-scale launch prepared the flow state
    int ibc;                                                          // the tasks hold intra block copies: the flow kernel built with that path
};

#pragma GCC visibility push(hidden)
// ---- ovvc_picture.hip ----
void *pinned_alloc(void *user, size_t bytes);
void pinned_free(void *user, void *p);
int pinned_reserve(ovhip_job *j, void **p, size_t *cap, size_t bytes);
int dev_reserve(ovhip_job *j, int k, size_t bytes);
int state_words(ovhip_job *j, uint32_t **words, size_t n);
int ordered_arm(ovhip_job *j, uint32_t **words, size_t n);
int flow_widest(const ovhip_itask *sorted, const uint32_t *items, size_t n_items);
// the array fields of a Chain from (placement, first indices, counts): n_itask / n_edge_* as the submission runs them
void chain_bind(Chain &c, const Placement &p, const ovhip_band_counts &first, const ovhip_band_counts &n, uint32_t n_rpr, uint32_t n_affr);
int chain_predict(const Chain &c, const ovhip_pic *refs_same, const ovhip_pic *refs, uint32_t n_refs, const ovhip_pic *intra, int32_t *d_mv);
int chain_residual(Chain &c, const uint16_t *d_bwd);
int chain_ordered(const Chain &c, int n_workers);
int chain_unmap(ovhip_job *j, const ovhip_pic *dst, int32_t row0, int32_t row1, const uint16_t *d_bwd, const ovhip_itask *d_it, uint32_t n_tagged);
int chain_deblock(const Chain &c, const ovhip_dbf_edge *d_ev, uint32_t n_ev, const ovhip_dbf_edge *d_eh, uint32_t n_eh, const ovhip_dbf_offsets *offs);
int chain_filters(const Chain &c, const ovhip_sao_ctu *d_sao, const ovhip_alf_pic *alf, int32_t s0, int32_t s1, int32_t a0, int32_t a1);
// flow admission (the section of that name)
int flow_shift_of(int device);
int flow_worker_count(const ovhip_ctx *ctx, uint32_t asked, const ovhip_itask *sorted, const uint32_t *items, size_t n_items, bool in_band);
void flow_launch_abandoned(ovhip_job *j);
void flow_launch_clean(ovhip_job *j);
int band_flow_take(ovhip_ctx *ctx, int want);
void band_flow_give(ovhip_ctx *ctx, int n);
int band_flow_reclaim(ovhip_ctx *ctx, int *charge, hipEvent_t ev_recon, int wait);
// ---- ovvc_band.hip ----
void band_free(ovhip_job *j);
int band_reset(ovhip_job *j);
int band_active(const ovhip_job *j);
int band_wait_done(ovhip_job *j);
#pragma GCC visibility pop
