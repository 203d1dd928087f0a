// ovvc_picture.hip -- the per-picture flush of the rcn back-end, in C (include/ovvc_hip.h "Picture job").
//
// The reference reconstructs block by block while it parses (coding_unit() -> rcn slots, vcl_coding_unit.c:711-840);
// the device path defers: the slots record, and the LAST alf.rcn_alf_filter_line of a picture (slicedec.c:940-955) hands
// the recorded picture over.  This file is that hand-over: asynchronous H2D of the recorder's page-locked arrays, the
// launch chain prediction -> residual -> (ordered intra pass) -> inverse luma mapping -> deblocking -> SAO -> ALF, and
// the D2H of the motion vectors DMVR refined (the `OVMV *mv0, *mv1` in/out contract of rcn_dmvr_mv_refine,
// rcn_structures.h:628-632).  Host code above the launches is plain C; nothing here falls back to a CPU path.
// The types this file shares with the band-wise submission (ovvc_band.hip) are in ovvc_job.hip.h.
#include "ovvc_job.hip.h"

extern "C" int ovhip_dmvr_search_launch(ovhip_ctx *ctx, const ovhip_pic *geom, const ovhip_pic *refs, uint32_t n_refs,
                                        const ovhip_mc_unit *d_units, uint32_t n_units, int32_t *d_mv_out);

namespace {

// Reference picture resampling: k_mc2 / k_mcxa / the DMVR search take the window geometry from the picture and refuse a reference
// of another size.  Their units never read such a slot (the recorder sends every unit that reads a scaled reference to the RPR
// array), so they get a table in which those slots hold a same-size stand-in (`geom` itself); k_mc_rpr gets the real table.
static const ovhip_pic *same_size_refs(const ovhip_pic *geom, const ovhip_pic *refs, uint32_t n_refs, ovhip_pic *out)
{
    if (!refs || n_refs > 16) return refs;
    bool any = false;
    for (uint32_t i = 0; i < n_refs; ++i) {
        const bool same = refs[i].w == geom->w && refs[i].h == geom->h && refs[i].stride_y == geom->stride_y && refs[i].stride_c == geom->stride_c;
        out[i] = same ? refs[i] : *geom;
        any |= !same;
    }
    return any ? out : refs;
}

// Small results that the host reads after the picture is complete (refined vectors, TMVP plane entries) leave the device from a
// kernel that stores into page-locked host memory: a hipMemcpyAsync between two kernels of a picture's chain is a round trip
// compute queue -> DMA engine -> compute queue with the hardware queue (shared by four pictures' streams) held at the barrier.
__global__ __launch_bounds__(256) void k_store_host(uint4 *__restrict__ dst, const uint4 *__restrict__ src, size_t n)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) dst[i] = src[i];
}

int store_host(ovhip_ctx *ctx, void *dst_host, const void *src_dev, size_t bytes)
{
    const size_t n = (bytes + 15) / 16;                 // (both buffers are allocated in multiples of 16 bytes)
    if (!n) return OVHIP_OK;
    hipLaunchKernelGGL(k_store_host, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, (uint4 *)dst_host, (const uint4 *)src_dev, n);
    OV_LAUNCH_CHECK(ctx, "k_store_host");
    return OVHIP_OK;
}

double host_now_us()
{
    timespec t;
    clock_gettime(CLOCK_MONOTONIC, &t);
    return 1e6 * (double)t.tv_sec + 1e-3 * (double)t.tv_nsec;
}

int grow_trace() { static int on = -1; if (on < 0) on = getenv("OVVC_HIP_GROW_TRACE") != nullptr; return on; }

int h2d(ovhip_job *j, hipStream_t st, int k, const void *host, size_t bytes)
{
    if (!bytes) return OVHIP_OK;
    if (j->resident) return j->dev[k].cap >= bytes ? OVHIP_OK : ov_fail(j->ctx, OVHIP_EINVAL, "resident flush before a full one", hipSuccess);
    int r = dev_reserve(j, k, bytes);
    if (r) return r;
    OV_HIP(j->ctx, hipMemcpyAsync(j->dev[k].p, host, bytes, hipMemcpyHostToDevice, st));
    j->st.h2d_bytes += bytes; j->st.n_h2d++;
    return OVHIP_OK;
}

extern "C" const ovhip_tb_cmd *ovhip_rec_tb_cmds_split_tiny_(ovhip_recorder *r, size_t counts[4], size_t tiny[4][4], size_t *n);
extern "C" int ovhip_itx_launch_ex_(ovhip_ctx *ctx, const ovhip_pic *dst, const ovhip_pic *res, const ovhip_tb_cmd *d_cmds, uint32_t n_large,
                                    uint32_t n_small, const uint32_t tiny3[4], const int16_t *d_coefs, const int16_t *d_lmcs_scales, const uint16_t *d_bwd_lut);

extern "C" int ovhip_sao_launch_rows(ovhip_ctx *ctx, const ovhip_pic *dst, const ovhip_pic *src, const ovhip_sao_ctu *d_params, int32_t log2_ctu_s, int32_t row0, int32_t row1);
extern "C" int ovhip_alf_launch_rows(ovhip_ctx *ctx, const ovhip_pic *dst, const ovhip_pic *src, const ovhip_alf_pic *alf, int32_t row0, int32_t row1);

#ifndef OVHIP_PACK_LIMIT
#define OVHIP_PACK_LIMIT (1 << 20)       /* bytes: arrays up to this size ride in the staging block (round 6, uploads on shared streams:
                                          * 128 KB 3414 +- 147 / 3491 +- 79, 1 MB 3492 +- 69 / 3566 +- 49, 2 MB 3456, everything 3440 pictures/s;
                                          * tools/debug/ab_pack_limit.sh) */
#endif

int t_collect(ovhip_job *j, int k)
{
    if (!j->t_pending[k]) return OVHIP_OK;
    float ms = 0.f;
    OV_HIP(j->ctx, hipEventSynchronize(j->t_ev[k][1]));
    OV_HIP(j->ctx, hipEventElapsedTime(&ms, j->t_ev[k][0], j->t_ev[k][1]));
    j->t_sum_ms += ms; j->t_count++;
    j->t_pending[k] = 0;
    return OVHIP_OK;
}

// bracket the launches of `stage` with an event pair on the launch stream (a pair costs a few us of stream time, which
// is why only ONE stage is bracketed at a time)
struct StageTimer {
    ovhip_job *j; int k;
    StageTimer(ovhip_job *job, int stage) : j(job), k(-1)
    {
        if (!j || j->t_stage != stage) return;
        k = j->t_next; j->t_next = (j->t_next + 1) % 32;
        if (t_collect(j, k) != OVHIP_OK || hipEventRecord(j->t_ev[k][0], j->ctx->stream) != hipSuccess) k = -1;
    }
    ~StageTimer()
    {
        if (k >= 0 && hipEventRecord(j->t_ev[k][1], j->ctx->stream) == hipSuccess) j->t_pending[k] = 1;
    }
};

// rows [r0, r1) of every plane (chroma: r0 / 2 .. r1 / 2), one 2-D copy per plane (the two pictures may come from different allocators)
int copy_rows(ovhip_ctx *ctx, const ovhip_pic *d, const ovhip_pic *s, int32_t r0, int32_t r1)
{
    uint16_t *dp[3] = { d->y, d->cb, d->cr };
    uint16_t *sp[3] = { s->y, s->cb, s->cr };
    for (int p = 0; p < 3; ++p) {
        const size_t ds = p ? d->stride_c : d->stride_y, ss = p ? s->stride_c : s->stride_y;
        const int32_t a = p ? r0 / 2 : r0, b = p ? r1 / 2 : r1;
        OV_HIP(ctx, hipMemcpy2DAsync(dp[p] + a * ds, ds * 2, sp[p] + a * ss, ss * 2, (size_t)(p ? d->w / 2 : d->w) * 2, b - a,
                                     hipMemcpyDeviceToDevice, ctx->stream));
    }
    return OVHIP_OK;
}

// the refined vectors of the units [first, n) as entries of the picture's collocated motion plane (4 per unit, recorder order), stored
// into the page-locked array the host reads; d_units / d_mv: the device copies of the units and their vectors, at index first
int tmvp_cells(ovhip_job *j, const ovhip_mc_unit *d_units, const int32_t *d_mv, size_t first, size_t n, int log2_ctu)
{
    ovhip_tmvp_cell *d_cells = (ovhip_tmvp_cell *)j->dev[B_TMVP].p + 4 * first;
    CHK(ovhip_tmvp_cells_launch(j->ctx, d_units, (uint32_t)(n - first), d_mv, log2_ctu, (j->w + (1 << log2_ctu) - 1) >> log2_ctu, d_cells));
    CHK(store_host(j->ctx, j->tmvp_host + 4 * first, d_cells, 4 * (n - first) * sizeof(ovhip_tmvp_cell)));
    j->n_tmvp = 4 * n;
    return OVHIP_OK;
}

} // namespace

// The uploads of all pictures of a device on a FEW shared streams instead of every picture's own (tools/micro/h2d_concurrent.py, round 4:
// 16 streams copying at once reach 31-38 GB/s, 1-4 streams 52-56): a picture's copies go to one of the device's upload streams, dealt
// round-robin per flush, and the picture's own stream waits for the event behind them.  Measured on the headline stream, interleaved
// runs on one box (tools/debug/ab_upload_streams.sh; LABBOOK 12): own stream 3309 +- 73 pictures/s, two upload streams 3506 +- 25; on
// a second box 3336 / 3419 (three: 3427, four: 3247, eight: 3366).  OVVC_HIP_UPLOAD_STREAMS=0: every picture uploads on its own stream.
enum { UP_DEVS = 64, UP_MAX = 8 };
static pthread_mutex_t g_up_mtx = PTHREAD_MUTEX_INITIALIZER;
static hipStream_t g_up[UP_DEVS][UP_MAX];
static unsigned g_up_next[UP_DEVS];
static int g_up_n = -1;
static int upload_stream_count();
static hipStream_t upload_stream_for(ovhip_job *j)
{
    const int n = upload_stream_count(), dev = j->ctx->device;
    if (n <= 0 || dev < 0 || dev >= UP_DEVS || j->t_stage >= 0) return nullptr;
    pthread_mutex_lock(&g_up_mtx);
    const unsigned k = g_up_next[dev]++ % (unsigned)n;
    if (!g_up[dev][k] && hipStreamCreateWithFlags(&g_up[dev][k], hipStreamNonBlocking) != hipSuccess) g_up[dev][k] = nullptr;
    hipStream_t st = g_up[dev][k];
    pthread_mutex_unlock(&g_up_mtx);
    return st;
}

static int upload_stream_count()
{
    if (__atomic_load_n(&g_up_n, __ATOMIC_RELAXED) < 0) {
        const char *e = getenv("OVVC_HIP_UPLOAD_STREAMS"); const int n = e ? atoi(e) : 2;
        __atomic_store_n(&g_up_n, n < 0 ? 0 : n > UP_MAX ? UP_MAX : n, __ATOMIC_RELAXED);
    }
    return __atomic_load_n(&g_up_n, __ATOMIC_RELAXED);
}

/* (internal, ovvc_stream.c) The device's upload streams out of the hardware queue of `keep_clear`'s stream -- the look-ahead thread's: the event
 * behind a picture's copies is a packet of the upload stream's hardware queue, and behind an I picture's ordered pass it would arrive
 * milliseconds late for every picture whose copies follow.  An upload stream that shares the queue is replaced (the old one stays
 * alive: events may refer to it).  Returns the number still sharing, or < 0. */
extern "C" int ovhip_upload_streams_clear_of_(ovhip_ctx *keep_clear)
{
    if (!keep_clear) return OVHIP_EINVAL;
    const int n = upload_stream_count(), dev = keep_clear->device;
    if (n <= 0 || dev < 0 || dev >= UP_DEVS) return 0;
    OV_DEVICE(keep_clear);
    int sharing = 0;
    for (int k = 0; k < n; ++k) {
        pthread_mutex_lock(&g_up_mtx);
        if (!g_up[dev][k] && hipStreamCreateWithFlags(&g_up[dev][k], hipStreamNonBlocking) != hipSuccess) g_up[dev][k] = nullptr;
        hipStream_t st = g_up[dev][k];
        pthread_mutex_unlock(&g_up_mtx);
        if (!st) continue;
        for (int tries = 0; tries < 12; ++tries) {
            ovhip_ctx tmp; memset(&tmp, 0, sizeof(tmp)); tmp.device = dev; tmp.stream = st;
            const int q = ovhip_ctx_shares_queue(keep_clear, &tmp);
            if (q != 1) { st = q == 0 ? st : nullptr; break; }
            hipStream_t fresh = nullptr;
            if (hipStreamCreateWithFlags(&fresh, hipStreamNonBlocking) != hipSuccess) { st = nullptr; break; }
            st = fresh;
            if (tries == 11) st = nullptr;
        }
        if (!st) { ++sharing; continue; }
        pthread_mutex_lock(&g_up_mtx);
        g_up[dev][k] = st;
        pthread_mutex_unlock(&g_up_mtx);
    }
    return sharing;
}

void *pinned_alloc(void *user, size_t bytes)
{
    (void)user;
    void *p = nullptr;
    const double t0 = grow_trace() ? host_now_us() : 0.0;
    const bool ok = hipHostMalloc(&p, bytes ? bytes : 16, hipHostMallocDefault) == hipSuccess;
    if (grow_trace()) fprintf(stderr, "grow: pinned %zu bytes at %.3f ms, took %.3f ms\n", bytes, 1e-3 * t0, 1e-3 * (host_now_us() - t0));
    return ok ? p : nullptr;
}
void pinned_free(void *user, void *p) { (void)user; if (p) (void)hipHostFree(p); }

int dev_reserve(ovhip_job *j, int k, size_t bytes)
{
    DevBuf &b = j->dev[k];
    if (bytes <= b.cap) return OVHIP_OK;
    size_t nc = b.cap ? b.cap : (size_t)1 << 16;
    while (nc < bytes) nc *= 2;
    // growth is rare (first pictures of a sequence); hipFree synchronises the device, which is what makes it safe here
    const double t0 = grow_trace() ? host_now_us() : 0.0;
    if (b.p) OV_HIP(j->ctx, hipFree(b.p));
    b.p = nullptr; b.cap = 0;
    hipError_t e = hipMalloc(&b.p, nc);
    if (grow_trace()) fprintf(stderr, "grow: device buffer %d to %zu bytes at %.3f ms, took %.3f ms\n", k, nc, 1e-3 * t0, 1e-3 * (host_now_us() - t0));
    if (e != hipSuccess) return ov_fail(j->ctx, OVHIP_ENOMEM, "hipMalloc(job buffer)", e);
    b.cap = nc;
    return OVHIP_OK;
}

int pinned_reserve(ovhip_job *j, void **p, size_t *cap, size_t bytes)
{
    if (bytes <= *cap) return OVHIP_OK;
    size_t nc = *cap ? *cap : 4096;
    while (nc < bytes) nc *= 2;
    void *q = pinned_alloc(nullptr, nc);
    if (!q) return ov_fail(j->ctx, OVHIP_ENOMEM, "hipHostMalloc", hipSuccess);
    if (*p) { memcpy(q, *p, *cap); pinned_free(nullptr, *p); }
    *p = q; *cap = nc;
    return OVHIP_OK;
}

// device state words of the ordered pass (d_flow, d_sync), zeroed once
int state_words(ovhip_job *j, uint32_t **words, size_t n)
{
    if (*words) return OVHIP_OK;
    OV_HIP(j->ctx, hipMalloc((void **)words, n * sizeof(uint32_t)));
    OV_HIP(j->ctx, hipMemsetAsync(*words, 0, n * sizeof(uint32_t), j->ctx->stream));
    return OVHIP_OK;
}

// before an ordered pass whose workgroups wait for each other (the flow launch, the one-launch pass): its state words, the pinned word
// it writes when a bounded wait expired, and this picture's epoch
int ordered_arm(ovhip_job *j, uint32_t **words, size_t n)
{
    CHK(state_words(j, words, n));
    if (!j->abort_host) {
        j->abort_host = (uint32_t *)pinned_alloc(nullptr, 64);
        if (!j->abort_host) return ov_fail(j->ctx, OVHIP_ENOMEM, "pinned abort word", hipSuccess);
        *j->abort_host = 0;
    }
    if (++j->epoch >= 0x7ffffff0u) j->epoch = 1;
    return OVHIP_OK;
}

// No more workers than a flow launch's widest level can use (round 4): a worker beyond that only ever holds an item that is levels ahead
// of the front -- and its wave slot, registers and LDS are then missing to the kernels of the pictures beside it for as long as the pass
// runs.  Twice the widest level, in multiples of 64.
int flow_widest(const ovhip_itask *sorted, const uint32_t *items, size_t n_items)
{
    size_t widest = 0, run = 0;
    for (size_t q = 0; q < n_items; ++q) {
        run = (q && sorted[flow_item_unpack(items[q]).task].level == sorted[flow_item_unpack(items[q - 1]).task].level) ? run + 1 : 1;
        if (run > widest) widest = run;
    }
    return (int)((2 * widest + 63) & ~(size_t)63);
}

// =====================================================================================================================================
// Flow admission: how many workers a flow launch gets, what an abandoned and a clean launch do to the launches that follow, and the
// budget the band launches of a device share.  The flush, ovhip_job_wait and the band-wise submission all decide here.
//
// ONE launch of W persistent workers (k_intra_flow): worker b takes the items b, b + W, ... in level order.  W bounds the
// pollers of the launch, and the launches in flight together must fit the device for the forward-progress argument (an item
// waits only for lower items; the lowest unfinished item's worker is resident or will be): the kernel runs at 4 waves per
// SIMD = 16 one-wave workgroups per compute unit (106 VGPRs as built), HIP runs the process's streams on 4 hardware queues,
// so W = 16 CUs / 4 = 1024 on MI355X.
// Measured on the stream of bench.py (pictures/s, second passes): one workgroup per item 2834-2890 / 0 (the device full of
// the pollers of levels far ahead); W = 512 3280-3320 / 0; 1024 3353-3490 / 0; 2048 1561 / 9; 4096 35 / 1168 -- above
// the bound the launches starve each other, exactly as the argument says.  Alone, a B picture's wide levels want more
// workers (its pass: 104 us with a workgroup per item, 156 with 1024 workers, 229 with 512); beside other pictures that
// does not show.  GPU_MAX_HW_QUEUES = 8 with W = 512: 3000-3060 / 0, no gain.  (ovhip_job_params.flow_workers sets W.)
//  the 4 x CUs default assumes 4 hardware queues and 16 resident waves per CU; where that does not hold (another
// GPU_MAX_HW_QUEUES, another process on the GPU) flow launches starve each other and pictures fall into second passes:
// every abandoned launch halves the default for the launches that follow (g_flow_shift, down to CUs / 4)
// Round 4: 6 x CUs (1536).  The forward-progress argument at the head of this section sized 4 x CUs for four launches of the full count side by side; since the
// widest-level rule (flow_widest, applied in flow_worker_count) an I picture's launch holds ~256 workers, and B launches of 1536 were never abandoned in 4600
// pictures (tools/sweep_bpic_workers.sh, interleaved, six runs each: 1024 workers 3220 pictures/s, 1536 3308, 2048 2-10
// second passes per run); an abandoned launch still halves the default (g_flow_shift).
// (flow_widest) An I picture has ~100 items per level and runs 5 ms: 4 x CUs = 1024 workers gave 2830-2930 pictures/s on
// bench.py's stream, 128-512 gave 3000-3150 (tools/sweep_ipic_workers.sh); a B picture's levels are 1000+ items wide and
// keep the full count.
// =====================================================================================================================================

// workers of a flow launch = (6 x CUs) >> g_flow_shift[device]: grows with every launch of that device that was abandoned (co-resident
// flow launches starving each other: another GPU_MAX_HW_QUEUES, another process on the GPU) and decays again -- one step per
// FLOW_DECAY pictures whose flow launch went through -- so that one transient event does not halve the device's pictures for the life of
// the process; ovhip_job_stats.flow_shift reports it
enum { FLOW_DEVS = 64, FLOW_DECAY = 512 };
static int g_flow_shift[FLOW_DEVS], g_flow_clean[FLOW_DEVS];
int flow_shift_of(int device)          // clamped where it is read: a shift count is never negative, never above 4
{
    const int s = __atomic_load_n(&g_flow_shift[device & (FLOW_DEVS - 1)], __ATOMIC_RELAXED);
    return s < 0 ? 0 : s > 4 ? 4 : s;
}

// The worker count of the flow launch over `items` (of the level-sorted tasks `sorted`).  asked: ovhip_job_params.flow_workers, 0 for
// the default = the device's 6 x CUs >> shift, and no more than the launch's widest level can use, but at least 64.  An explicit count
// wins as it is in a flush; a band caps it like the default, and its count is a multiple of 64, as the budget below deals them.
int flow_worker_count(const ovhip_ctx *ctx, uint32_t asked, const ovhip_itask *sorted, const uint32_t *items, size_t n_items, bool in_band)
{
    const int most = (6 * ctx->num_cus) >> flow_shift_of(ctx->device);
    int n = asked ? (int)asked : flow_widest(sorted, items, n_items);
    if (in_band || !asked) n = n >= most ? most : (n < 64 ? 64 : n);
    if (in_band) return ((n < 64 ? 64 : n) + 63) & ~63;
    return n < 1 ? 1 : n;
}

// ovhip_job_wait found the abort word set: the launch was abandoned.  Every such launch halves the default of the launches that
// follow on the device -- unless the test hook forced it (no evidence of starvation) -- and is not a clean one for the decay
void flow_launch_abandoned(ovhip_job *j)
{
    const int fd = j->ctx->device & (FLOW_DEVS - 1);
    if (!j->test_abort_seen) {
        if (__atomic_load_n(&g_flow_shift[fd], __ATOMIC_RELAXED) < 4) __atomic_fetch_add(&g_flow_shift[fd], 1, __ATOMIC_RELAXED);
        __atomic_store_n(&g_flow_clean[fd], 0, __ATOMIC_RELAXED);
    }
    j->test_abort_seen = 0;
    j->flow_launched = 0;                //  an abandoned launch is not a clean one for the decay below
}

// ovhip_job_wait found the picture complete: if it had a flow launch, that one counts towards the decay
void flow_launch_clean(ovhip_job *j)
{
    if (!j->flow_launched) return;
    const int fd = j->ctx->device & (FLOW_DEVS - 1);
    j->flow_launched = 0;
    //  exactly ONE thread takes the step -- the one whose increment lands on FLOW_DECAY -- and the shift never goes
    // below zero (two threads that both saw ">= FLOW_DECAY" used to subtract twice: 1 -> -1, a negative shift count)
    if (__atomic_load_n(&g_flow_shift[fd], __ATOMIC_RELAXED) > 0 && __atomic_add_fetch(&g_flow_clean[fd], 1, __ATOMIC_RELAXED) == FLOW_DECAY) {
        __atomic_store_n(&g_flow_clean[fd], 0, __ATOMIC_RELAXED);
        int cur = __atomic_load_n(&g_flow_shift[fd], __ATOMIC_RELAXED);
        while (cur > 0 && !__atomic_compare_exchange_n(&g_flow_shift[fd], &cur, cur - 1, true, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
    }
}

// ---- flow budget: the workers of the band flow launches in flight on a device never exceed the wave slots k_intra_flow can hold
// there (16 one-wave workgroups per compute unit, three quarters of them: the whole-picture launches of I pictures run beside).  A
// launch is charged when it is enqueued and released when its job sees the event behind it -- so every charged launch's workers can
// be resident together and no worker waits for a workgroup that cannot start.
static int g_band_flow_inflight[FLOW_DEVS];
int band_flow_take(ovhip_ctx *ctx, int want)
{
    const int fd = ctx->device & (FLOW_DEVS - 1), cap = 12 * ctx->num_cus;
    int cur = __atomic_load_n(&g_band_flow_inflight[fd], __ATOMIC_RELAXED);
    for (;;) {
        int give = cap - cur < want ? cap - cur : want;
        give &= ~63;
        if (give < 64) return 0;
        if (__atomic_compare_exchange_n(&g_band_flow_inflight[fd], &cur, cur + give, true, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) return give;
    }
}
void band_flow_give(ovhip_ctx *ctx, int n) { if (n) __atomic_fetch_sub(&g_band_flow_inflight[ctx->device & (FLOW_DEVS - 1)], n, __ATOMIC_RELAXED); }

// a band's charge goes back once the event behind its reconstruction has been seen (wait: synchronise with it); 0: it is still running
int band_flow_reclaim(ovhip_ctx *ctx, int *charge, hipEvent_t ev_recon, int wait)
{
    if (!*charge) return 1;
    if (wait) (void)hipEventSynchronize(ev_recon);
    else if (hipEventQuery(ev_recon) != hipSuccess) { (void)hipGetLastError(); return 0; }
    band_flow_give(ctx, *charge);
    *charge = 0;
    return 1;
}

// ---- the launch chain (Chain, ovvc_job.hip.h) ----
void chain_bind(Chain &c, const Placement &p, const ovhip_band_counts &first, const ovhip_band_counts &n, uint32_t n_rpr, uint32_t n_affr)
{
    c.d_mc = (const ovhip_mc_unit *)p.at[B_MC]; c.n_mc = n.n_mc; c.d_mcx = (const ovhip_mc_unit *)p.at[B_MCX]; c.n_mcx = n.n_mcx;
    c.d_aff = (const ovhip_aff_unit *)p.at[B_AFF]; c.n_aff = n.n_aff; c.d_side = (const int32_t *)p.at[B_SIDE] - first.n_side;
    c.d_rpr = (const ovhip_rpr_unit *)p.at[B_RPR]; c.n_rpr = n_rpr; c.d_affr = (const ovhip_aff_rpr_unit *)p.at[B_AFFR]; c.n_affr = n_affr;
    c.d_tb = (const ovhip_tb_cmd *)p.at[B_TB]; c.d_coef = (const int16_t *)p.at[B_COEF] - first.n_coef;
    c.d_reg = (const ovhip_lmcs_region *)p.at[B_REG] - first.n_reg; c.reg0 = first.n_reg; c.n_reg = n.n_reg;
    c.d_it = (const ovhip_itask *)p.at[B_ITASK]; c.n_it = n.n_itask; c.d_items = (const uint32_t *)p.at[B_IITEM];
}

// prediction: MC with the units that read a scaled reference beside it (disjoint blocks), then refined / affine MC.  refs: the reference
// table of k_mc_rpr; refs_same: the same with a same-size stand-in for every scaled reference (same_size_refs).  intra: the picture with
// the CIIP units' intra prediction, or nullptr.  d_mv: where k_mcxa leaves the refined vectors.
int chain_predict(const Chain &c, const ovhip_pic *refs_same, const ovhip_pic *refs, uint32_t n_refs, const ovhip_pic *intra, int32_t *d_mv)
{
    ovhip_job *j = c.j;
    {
        StageTimer t_(c.timer, OVHIP_TIME_MC);
        CHK(ovhip_mc_launch(j->ctx, c.dst, refs_same, n_refs, c.d_mc, c.n_mc, c.d_fwd, intra));
        if (c.n_rpr) CHK(ovhip_mc_rpr_launch(j->ctx, c.dst, refs, n_refs, c.d_rpr, c.n_rpr, c.d_fwd, intra));
    }
    j->st.n_launches += (c.n_mc != 0) + (c.n_rpr != 0);
    if (c.n_mcx || c.n_aff) {
        StageTimer t_(c.timer, OVHIP_TIME_MCXA);
        CHK(ovhip_mcxa_launch(j->ctx, c.dst, refs_same, n_refs, c.d_mcx, c.n_mcx, d_mv, c.d_aff, c.n_aff, c.d_side, c.d_fwd));
        j->st.n_launches++;
    }
    if (c.n_affr) {
        // like k_mc_rpr: the real reference table, blocks disjoint from every other unit's
        StageTimer t_(c.timer, OVHIP_TIME_MCXA);
        CHK(ovhip_mca_rpr_launch(j->ctx, c.dst, refs, n_refs, c.d_affr, c.n_affr, c.d_side, c.d_fwd));
        j->st.n_launches++;
    }
    return OVHIP_OK;
}

// residual: luma blocks, the chroma-scale derivation on the reconstructed luma (before a flow launch: the launch that also prepares its
// state words), chroma blocks.  d_bwd: the inverse luma mapping follows at once (no ordered pass keeps the luma mapped) -- inside the
// chroma launch where that has blocks
int chain_residual(Chain &c, const uint16_t *d_bwd)
{
    ovhip_job *j = c.j;
    ovhip_ctx *ctx = j->ctx;
    const uint32_t t_luma[4] = { (uint32_t)c.tiny[1][0], (uint32_t)c.tiny[1][1], (uint32_t)c.tiny[1][2], (uint32_t)c.tiny[1][3] };
    const uint32_t t_chroma[4] = { (uint32_t)c.tiny[3][0], (uint32_t)c.tiny[3][1], (uint32_t)c.tiny[3][2], (uint32_t)c.tiny[3][3] };
    if (c.cls[0] + c.cls[1]) {
        StageTimer t_(c.timer, OVHIP_TIME_ITX_LUMA);
        CHK(ovhip_itx_launch_ex_(ctx, c.dst, c.res, c.d_tb, (uint32_t)c.cls[0], (uint32_t)c.cls[1], t_luma, c.d_coef, nullptr, nullptr));
        j->st.n_launches++;
    }
    if (c.n_reg) {
        if (!c.luts) return ov_fail(ctx, OVHIP_EINVAL, "chroma-scale regions recorded without LMCS tables", hipSuccess);
        StageTimer t_(c.timer, OVHIP_TIME_LMCS_SCALE);
        if (c.n_items) {
            CHK(ovhip_lmcs_scale_prepare_launch(ctx, c.dst, c.d_reg + c.reg0, c.n_reg, c.luts, c.d_scales + c.reg0, c.d_it, c.n_it, j->d_flow, j->epoch));
            c.prepared = 1;
        } else CHK(ovhip_lmcs_scale_launch(ctx, c.dst, c.d_reg + c.reg0, c.n_reg, c.luts, c.d_scales + c.reg0));
        j->st.n_launches++;
    }
    const ovhip_tb_cmd *d_tbc = c.d_tb + c.cls[0] + c.cls[1];
    StageTimer t_(c.timer, OVHIP_TIME_ITX_CHROMA);
    if (d_bwd && c.cls[3]) {
        CHK(ovhip_itx_launch_ex_(ctx, c.dst, nullptr, d_tbc, (uint32_t)c.cls[2], (uint32_t)c.cls[3], t_chroma, c.d_coef, c.d_scales, d_bwd));
        j->st.n_launches++;
        return OVHIP_OK;
    }
    if (c.cls[2] + c.cls[3]) {
        CHK(ovhip_itx_launch_ex_(ctx, c.dst, c.res, d_tbc, (uint32_t)c.cls[2], (uint32_t)c.cls[3], t_chroma, c.d_coef, c.d_scales, nullptr));
        j->st.n_launches++;
    }
    if (d_bwd) { CHK(ovhip_lmcs_inverse_launch(ctx, c.dst, d_bwd)); j->st.n_launches++; }
    return OVHIP_OK;
}

// ordered pass: ONE flow launch of n_workers persistent workers, or one launch per level (the launch boundary is the inter-level
// synchronisation)
int chain_ordered(const Chain &c, int n_workers)
{
    ovhip_job *j = c.j;
    if (c.n_items) {
        CHK(ovhip_intra_flow_launch(j->ctx, c.dst, c.res, c.d_it, c.n_it, c.d_items, c.n_items, c.d_reg, c.luts, c.d_scales, c.log2_ctu,
                                    j->d_flow, j->epoch, j->abort_host, (c.prepared ? 0 : 1) | (c.ibc ? OVHIP_FLOW_IBC : 0), n_workers));
        j->st.n_launches += 1 + !c.prepared;
        return OVHIP_OK;
    }
    for (uint32_t l = 0; l < c.n_lv; ++l) {
        const uint32_t a = c.lv_start[l], b = c.lv_start[l + 1];
        if (b > a) {
            CHK(ovhip_intra_level_launch(j->ctx, c.dst, c.res, c.d_it + a, b - a, c.d_reg, c.luts, c.d_scales, c.log2_ctu,
                                         ovhip_intra_level_geom(c.h_it + a, b - a)));
            j->st.n_launches++;
        }
    }
    return OVHIP_OK;
}

// tail, first half: the inverse luma mapping of rows [row0, row1) (d_bwd), which also drops the flow launches' hand-over bit -- or,
// without it, the un-tag alone.  d_it[n_tagged]: the tasks whose samples still carry the bit.
int chain_unmap(ovhip_job *j, const ovhip_pic *dst, int32_t row0, int32_t row1, const uint16_t *d_bwd, const ovhip_itask *d_it, uint32_t n_tagged)
{
    if (d_bwd) {
        ovhip_pic view = *dst;                                // the luma rows; the chroma un-tag takes picture coordinates
        view.y = dst->y + (size_t)row0 * dst->stride_y; view.h = row1 - row0;
        CHK(ovhip_lmcs_inverse_untag_launch(j->ctx, &view, d_bwd, d_it, n_tagged));
    } else if (n_tagged) CHK(ovhip_intra_flow_untag_launch(j->ctx, dst, d_it, n_tagged, 1));
    else return OVHIP_OK;
    j->st.n_launches++;
    return OVHIP_OK;
}

// tail, second half: the deblocking of the edge lists (vertical, then horizontal)
int chain_deblock(const Chain &c, const ovhip_dbf_edge *d_ev, uint32_t n_ev, const ovhip_dbf_edge *d_eh, uint32_t n_eh, const ovhip_dbf_offsets *offs)
{
    StageTimer t_(c.timer, OVHIP_TIME_DBF);
    CHK(ovhip_dbf_launch_edges_ex(c.j->ctx, c.dst, d_ev, n_ev, d_eh, n_eh, offs));
    c.j->st.n_launches += (n_ev != 0) + (n_eh != 0);
    return OVHIP_OK;
}

// filters: SAO rows [s0, s1) into tmp, ALF rows [a0, a1) back into dst (d_sao / alf: nullptr when off; their CTU tables indexed from
// the picture's first CTU row).  With only one of the two on, a copy of the rows stands in for the other, so that dst holds the result.
int chain_filters(const Chain &c, const ovhip_sao_ctu *d_sao, const ovhip_alf_pic *alf, int32_t s0, int32_t s1, int32_t a0, int32_t a1)
{
    ovhip_job *j = c.j;
    if (s1 > s0) {
        if (d_sao) {
            StageTimer t_(c.timer, OVHIP_TIME_SAO);
            CHK(ovhip_sao_launch_rows(j->ctx, &j->tmp, c.dst, d_sao, c.log2_ctu, s0, s1));
            j->st.n_launches++;
        } else if (alf) CHK(copy_rows(j->ctx, &j->tmp, c.dst, s0, s1));
    }
    if (a1 > a0) {
        if (alf) {
            StageTimer t_(c.timer, OVHIP_TIME_ALF);
            CHK(ovhip_alf_launch_rows(j->ctx, c.dst, &j->tmp, alf, a0, a1));
            j->st.n_launches++;
        } else if (d_sao) CHK(copy_rows(j->ctx, c.dst, &j->tmp, a0, a1));
    }
    return OVHIP_OK;
}

namespace {

// ---- ovhip_job_flush in three phases: gather (host only) -> stage (layout, fill, uploads, waits) -> launch.  What passes between them:
// Gathered (what the recorder holds and what was decided from it) and Placement (where staging put it on the device).
struct Gathered {
    Switches sw; size_t n_ctu;
    double t0;                                    // host time when the gather began (ovhip_job_stats.host_us_prepare counts from here)
    const ovhip_tb_cmd *tb; size_t cls[4], tiny[4][4];               // class split (luma first; big / small), the tiny blocks at the end of each class (a lane per sample)
    const int16_t *coef; const ovhip_mc_unit *mc, *mcx; const ovhip_aff_unit *aff; const int32_t *side; const ovhip_lmcs_region *reg;
    const ovhip_ciip_unit *ciip; const ovhip_rpr_unit *rpr; const ovhip_aff_rpr_unit *affr;
    const ovhip_itask *it; const ovhip_ictu *ictu; const uint32_t *lv_start; uint32_t n_lv;
    const ovhip_dbf_edge *ev, *eh; ovhip_dbf_offsets offs;
    ovhip_band_counts n;                          // (n_itask: 0 without OVHIP_STAGE_INTRA)
    size_t n_ciip, n_rpr, n_affr, n_ictu;
    size_t n_items;                               // the flow launch's items in j->items_host; 0: the ordered pass cannot run as one
    bool ibc;                                     // the ordered tasks hold intra block copies
    int by_ctu; bool ordered, flow;               // the ordered pass: grouped by CTU for the one-launch pass, as ONE flow launch, else per level
};

int flush_gather(ovhip_job *j, const ovhip_pic *dst, const ovhip_pic *intra, const ovhip_job_params *pr, Gathered &g)
{
    ovhip_ctx *ctx = j->ctx;
    if ((dst->w != j->w || dst->h != j->h)) return ov_fail(ctx, OVHIP_EINVAL, "ovhip_job_flush: picture size differs from the job's", hipSuccess);
    // an eager pass nobody collected (ovhip_job_dmvr_rows_begin): its copies land in arrays this flush may re-allocate
    { const int64_t c_ = ovhip_job_dmvr_rows_collect(j); if (c_ < 0) return (int)c_; }
    g = Gathered{};
    g.sw = switches_of(pr);
    const uint32_t stages = g.sw.stages;
    const int log2_ctu = g.sw.log2_ctu;
    if (log2_ctu < 5 || log2_ctu > 7) return ov_fail(ctx, OVHIP_EINVAL, "ovhip_job_flush: log2_ctu_s", hipSuccess);
    g.n_ctu = (size_t)((j->w + (1 << log2_ctu) - 1) >> log2_ctu) * ((j->h + (1 << log2_ctu) - 1) >> log2_ctu);
    memset(&j->st, 0, sizeof(j->st));
    j->st.n_ordered_retries = j->n_retries;
    g.t0 = host_now_us();
    j->resident = (stages & OVHIP_STAGE_RESIDENT) && pr->stages;
    ovhip_recorder *rec = j->rec;

    // ---- class split of the transform blocks, recorder arrays ----
    size_t n_tb = 0, n_coef = 0, n_mc = 0, n_mcx = 0, n_aff = 0, n_side = 0, n_reg = 0, n_ev = 0, n_eh = 0;
    g.tb = ovhip_rec_tb_cmds_split_tiny_(rec, g.cls, g.tiny, &n_tb);
    if (!g.tb && n_tb) return ov_fail(ctx, OVHIP_ENOMEM, "ovhip_rec_tb_cmds_split", hipSuccess);
    g.coef = ovhip_rec_coefs(rec, &n_coef);
    g.mc = ovhip_rec_mc_units(rec, &n_mc);
    g.mcx = ovhip_rec_mcx_units(rec, &n_mcx);
    g.aff = ovhip_rec_aff_units(rec, &n_aff);
    g.side = ovhip_rec_aff_side(rec, &n_side);
    g.reg = ovhip_rec_lmcs_regions(rec, &n_reg);
    g.ciip = ovhip_rec_ciip_units(rec, &g.n_ciip);
    if (g.n_ciip && !intra)
        return ov_fail(ctx, OVHIP_EUNSUP, "ovhip_job_flush: CIIP blend units recorded but no picture with their intra prediction", hipSuccess);
    g.rpr = ovhip_rec_rpr_units(rec, &g.n_rpr);               // units that read a reference of another size (k_mc_rpr)
    g.affr = ovhip_rec_aff_rpr_units(rec, &g.n_affr);         // affine units that do (k_mca_rpr)
    // ---- ordered tasks: grouped by CTU for the one-launch pass, or sorted by level for one launch per level ----
    size_t n_it = 0;
    // (k_intra_ctu does not know intra block copy: a picture with such tasks asked for as the CTU pass runs one launch per level)
    const int want_ctu = pr->stages && (stages & OVHIP_STAGE_INTRA_CTU);
    g.ibc = ovhip_rec_ibc_tasks(rec) != 0;
    g.by_ctu = want_ctu && !g.ibc;
    int by_flow = !want_ctu && !(pr->stages && (stages & OVHIP_STAGE_INTRA_LEVELS));
    // a resident replay runs from what the last FULL flush left on the device: after a second pass (ovhip_job_wait: per-level launches,
    // no item list in the parameter block) that is a picture without the flow launch's items
    if (j->resident && by_flow && !j->flow_on_device) by_flow = 0;
    // (the flow launch also takes the level-sorted list)
    g.it = !g.by_ctu ? ovhip_rec_itasks_sorted(rec, &n_it, &g.lv_start, &g.n_lv)
                     : ovhip_rec_itasks_by_ctu(rec, log2_ctu, &n_it, &g.ictu, &g.n_ictu);
    if (by_flow && n_it) {
        // (the count comes back even where the list does not fit: it grows to that)
        g.n_items = ovhip_intra_flow_items_(g.it, n_it, j->items_host, j->items_cap / sizeof(uint32_t));
        if (g.n_items > j->items_cap / sizeof(uint32_t)) {
            CHK(pinned_reserve(j, (void **)&j->items_host, &j->items_cap, g.n_items * sizeof(uint32_t)));
            g.n_items = ovhip_intra_flow_items_(g.it, n_it, j->items_host, g.n_items);
        }
        // (0: more tasks / strips than an item word holds: per-level launches)
    }
    if (!g.it && ovhip_rec_itask_levels(rec)) return ov_fail(ctx, OVHIP_ENOMEM, "ovhip_job_flush: sorting the ordered tasks", hipSuccess);
    if (g.by_ctu) g.n_lv = ovhip_rec_itask_levels(rec);
    if (!(stages & OVHIP_STAGE_INTRA)) { n_it = 0; g.n_lv = 0; g.n_ictu = 0; }
    g.ordered = n_it != 0;               // a picture with an ordered pass keeps its luma in the mapped domain until the pass has run
    g.flow = (stages & OVHIP_STAGE_INTRA) && g.n_items;       // the ordered pass as ONE flow launch
    if (g.ordered && !j->res.y) CHK(ovhip_pic_alloc(ctx, j->w, j->h, &j->res));
    if (g.ordered && (dst->stride_y != j->res.stride_y || dst->stride_c != j->res.stride_c))
        return ov_fail(ctx, OVHIP_EUNSUP, "ovhip_job_flush: pictures with ordered tasks need tight planes (stride = width)", hipSuccess);
    g.ev = ovhip_rec_dbf_edges(rec, 0, &n_ev, &g.offs);
    g.eh = ovhip_rec_dbf_edges(rec, 1, &n_eh, nullptr);
    g.n = ovhip_band_counts{ (uint32_t)n_tb, (uint32_t)n_coef, (uint32_t)n_mc, (uint32_t)n_mcx, (uint32_t)n_aff, (uint32_t)n_side, (uint32_t)n_reg,
                             (uint32_t)n_it, (uint32_t)n_ev, (uint32_t)n_eh };
    j->st.n_itasks = g.n.n_itask; j->st.n_ilevels = g.n_lv;
    j->st.n_tb = g.n.n_tb; j->st.n_mc = g.n.n_mc; j->st.n_mcx = g.n.n_mcx; j->st.n_aff = g.n.n_aff;
    j->st.n_edges_v = g.n.n_edge_v; j->st.n_edges_h = g.n.n_edge_h; j->st.n_regions = g.n.n_reg;
    if (g.sw.alf_on && alf_tables_missing(pr)) return ov_fail(ctx, OVHIP_EINVAL, "ovhip_job_flush: ALF tables missing", hipSuccess);
    return OVHIP_OK;
}

// a recorder array of the flush: at != 0: it rides in the parameter block, at offset at - 1
struct Small { const void *host; size_t bytes; int buf; size_t at; };

// the copies of a flush on the stream `ust`: the parameter block, then every array that does not ride in it (packed[k]: where one that does is)
int stage_uploads(ovhip_job *j, hipStream_t ust, const Gathered &g, size_t block_bytes, const Small *small, size_t n_small, const void **packed)
{
    StageTimer t_(j, OVHIP_TIME_H2D);
    CHK(h2d(j, ust, B_PARAM, j->param_host, block_bytes));
    if (g.n.n_mcx) {
        CHK(dev_reserve(j, B_MV, (size_t)g.n.n_mcx * 16));
        CHK(pinned_reserve(j, (void **)&j->mv_host, &j->mv_cap, (size_t)g.n.n_mcx * 16));
    }
    if (g.n.n_reg) CHK(dev_reserve(j, B_SCALE, (size_t)g.n.n_reg * 2));
    // (refined units that went through the eager per-row search are uploaded again with the rest: the list is small and
    // the full kernel repeats the search with the identical result)
    for (size_t i = 0; i < n_small && !j->resident; ++i) {
        const Small &sm = small[i];
        if (sm.at) packed[sm.buf] = (const char *)j->dev[B_PARAM].p + sm.at - 1;
        else CHK(h2d(j, ust, sm.buf, sm.host, sm.bytes));
    }
    return OVHIP_OK;
}

int flush_stage(ovhip_job *j, const ovhip_job_params *pr, const Gathered &g, Placement &p)
{
    ovhip_ctx *ctx = j->ctx;
    const bool dbf = (g.sw.stages & OVHIP_STAGE_DBF) != 0, lmcs = pr->lmcs != nullptr;
    // ---- layout: the picture-level tables and the small arrays in one staging block ----
    Layout L;
    p.o_sao = L.put(g.sw.sao_on ? g.n_ctu * sizeof(ovhip_sao_ctu) : 0); p.o_alf = L.put(g.sw.alf_on ? g.n_ctu * sizeof(ovhip_alf_ctu) : 0);
    p.tabs = tables_put(L, g.sw.alf_on, lmcs);
    // Uploads are what the stream is bound by once the kernels are fast (round 4, tools/micro/h2d_concurrent.py on the GPU box: a 4K
    // picture's 8.7 MB in 10 copies on 16 streams at once = 3600 pictures/s of DMA and nothing else; one copy ~20 us of fixed cost;
    // 16 streams copying at once reach 31-38 GB/s where 1-4 reach 52-56).  So: arrays up to PACK_LIMIT ride in the staging block (one
    // host memcpy each, out of the recorder's page-locked arrays), the few larger ones get a copy of their own.
#ifdef OVHIP_TUNING
    static const size_t PACK_LIMIT = getenv("OVHIP_X_PACK_LIMIT") ? (size_t)atol(getenv("OVHIP_X_PACK_LIMIT")) : (size_t)OVHIP_PACK_LIMIT;
#else
    const size_t PACK_LIMIT = OVHIP_PACK_LIMIT;
#endif
    Small small[] = {
        { g.mc, g.n.n_mc * sizeof(*g.mc), B_MC, 0 }, { g.tb, g.n.n_tb * sizeof(*g.tb), B_TB, 0 }, { g.coef, g.n.n_coef * sizeof(*g.coef), B_COEF, 0 },
        { g.it, g.n.n_itask * sizeof(*g.it), B_ITASK, 0 }, { g.ictu, g.n_ictu * sizeof(*g.ictu), B_ICTU, 0 },
        { j->items_host, g.n_items * sizeof(uint32_t), B_IITEM, 0 },
        { g.mcx, g.n.n_mcx * sizeof(*g.mcx), B_MCX, 0 }, { g.ciip, g.n_ciip * sizeof(*g.ciip), B_CIIP, 0 }, { g.aff, g.n.n_aff * sizeof(*g.aff), B_AFF, 0 },
        { g.side, g.n.n_side * sizeof(*g.side), B_SIDE, 0 }, { g.reg, g.n.n_reg * sizeof(*g.reg), B_REG, 0 },
        { g.rpr, g.n_rpr * sizeof(*g.rpr), B_RPR, 0 }, { g.affr, g.n_affr * sizeof(*g.affr), B_AFFR, 0 },
        { g.ev, dbf ? g.n.n_edge_v * sizeof(*g.ev) : 0, B_EV, 0 }, { g.eh, dbf ? g.n.n_edge_h * sizeof(*g.eh) : 0, B_EH, 0 },
    };
    for (auto &sm : small) if (sm.bytes && sm.bytes <= PACK_LIMIT && !j->resident) sm.at = L.put(sm.bytes) + 1;
    // ---- fill ----
    if (L.o) {
        CHK(pinned_reserve(j, (void **)&j->param_host, &j->param_cap, L.o));
        char *ph = j->param_host;
        for (auto &sm : small) if (sm.at) memcpy(ph + sm.at - 1, sm.host, sm.bytes);
        if (g.sw.sao_on) memcpy(ph + p.o_sao, pr->sao, g.n_ctu * sizeof(ovhip_sao_ctu));
        if (g.sw.alf_on) memcpy(ph + p.o_alf, pr->alf_ctus, g.n_ctu * sizeof(ovhip_alf_ctu));
        tables_fill(ph, p.tabs, pr, g.sw.alf_on, lmcs);
    }

    const double t1 = host_now_us();
    // ---- H2D (asynchronous DMA out of page-locked memory, in stage order so that prediction can start early) ----
    const hipStream_t up = j->resident ? nullptr : upload_stream_for(j), ust = up ? up : ctx->stream;
    if (up) {
        // The copies overwrite buffers the previous picture's launches and this picture's eager refinement rows read: the upload stream
        // waits for THEIR events (ev_done: the end of the last flush; ev_rows: the end of an eager pass not collected yet) -- with a frame
        // thread that waits for its picture before it takes the next, both long complete.  NOT for a fresh marker on the picture's own
        // stream: a marker queues behind whatever other streams put into the same hardware queue (17 streams share 4: an I picture's
        // 7 ms ordered pass, a 0.8 ms frame download), and the shared upload stream would hold up every picture behind it (measured:
        // the in-order variant 2309 -> 1476, frames leaving the device 1247 -> 1022 pictures/s with such a marker)
        hipError_t e0 = hipSuccess;
        if (j->flushed) e0 = hipStreamWaitEvent(up, j->ev_done, 0);
        if (e0 == hipSuccess && j->rows_pending) e0 = hipStreamWaitEvent(up, j->ev_rows, 0);
        if (e0 != hipSuccess) return ov_fail(ctx, OVHIP_ENODEV, "ovhip_job_flush: upload stream", e0);
    }
    static_assert(B_COUNT <= 24, "packed_prev");
    const void *packed[24] = { nullptr };           // device address of a packed array (inside the parameter block)
    const int r_up = stage_uploads(j, ust, g, L.o, small, sizeof(small) / sizeof(small[0]), packed);
    // ev_h2d behind the copies on the stream that carries them -- also when one of them failed: ovhip_job_begin orders the reuse of the
    // page-locked arrays behind it
    OV_HIP(ctx, hipEventRecord(j->ev_h2d, ust));
    j->flushed = 1;
    if (r_up != OVHIP_OK) return r_up;
    if (up) OV_HIP(ctx, hipStreamWaitEvent(ctx->stream, j->ev_h2d, 0));
    // a resident replay re-uses the placement of the flush before it
    if (j->resident) memcpy(packed, j->packed_prev, sizeof(packed)); else { memcpy(j->packed_prev, packed, sizeof(packed)); j->flow_on_device = g.n_items != 0; }
    for (int k = 0; k < B_COUNT; ++k) p.at[k] = packed[k] ? packed[k] : j->dev[k].p;
    p.block = (const char *)j->dev[B_PARAM].p;
    const double t2 = host_now_us();
    // everything below reads or writes pictures: behind the pictures this one depends on
    for (uint32_t i = 0; i < pr->n_wait_events; ++i)
        if (pr->wait_events && pr->wait_events[i]) {
            if (pr->wait_on_host) OV_HIP(ctx, hipEventSynchronize((hipEvent_t)pr->wait_events[i]));
            else OV_HIP(ctx, hipStreamWaitEvent(ctx->stream, (hipEvent_t)pr->wait_events[i], 0));
        }
    if (pr->before_launch && pr->before_launch(pr->before_launch_user))
        return ov_fail(ctx, OVHIP_EINVAL, "ovhip_job_flush: before_launch callback failed", hipSuccess);
    j->st.host_us_prepare = (uint32_t)(t1 - g.t0); j->st.host_us_upload = (uint32_t)(t2 - t1);
    j->st.host_us_wait = (uint32_t)(host_now_us() - t2);
    return OVHIP_OK;
}

// prediction, with the refined vectors back to the host, their TMVP plane cells and the CIIP blend
int launch_predict(ovhip_job *j, const Chain &c, const ovhip_pic *refs, uint32_t n_refs, const ovhip_pic *intra, const ovhip_job_params *pr,
                   const Gathered &g, const Placement &p)
{
    const size_t n_mcx = g.n.n_mcx;
    // Nothing on the device reads the refined vectors unless the TMVP entries are asked for: k_mcxa then stores them (one 16-byte
    // store per unit) straight into the page-locked array the host reads -- not even k_store_host's launch is left
    const bool mv_direct = n_mcx && !pr->tmvp_cells && !j->resident;
    ovhip_pic same[16];
    CHK(chain_predict(c, same_size_refs(c.dst, refs, n_refs, same), refs, n_refs, intra, mv_direct ? j->mv_host : (int32_t *)p.at[B_MV]));
    j->mvf.src.refined = n_mcx ? (mv_direct ? j->mv_host : (const int32_t *)p.at[B_MV]) : nullptr;
    if (mv_direct) j->st.d2h_bytes += n_mcx * 16;
    else if (n_mcx && !j->resident) {
        // refined vectors back to the host as early as the stream allows (the decoder's TMVP field needs them), stored by a kernel
        // (round 4: as a DMA between k_mcxa and the residual kernels it cost the stream 7 % -- tools/x_mvd2h.sh: 2963 -> 3177 pictures/s)
        CHK(store_host(j->ctx, j->mv_host, p.at[B_MV], n_mcx * 16));
        j->st.d2h_bytes += n_mcx * 16;
    }
    j->n_mv = n_mcx;
    j->n_tmvp = 0;
    if (n_mcx && pr->tmvp_cells) {
        // the same vectors as a delta of the picture's collocated motion plane
        const size_t bytes = 4 * n_mcx * sizeof(ovhip_tmvp_cell);
        CHK(dev_reserve(j, B_TMVP, bytes));
        CHK(pinned_reserve(j, (void **)&j->tmvp_host, &j->tmvp_cap, bytes));
        CHK(tmvp_cells(j, c.d_mcx, (const int32_t *)p.at[B_MV], 0, n_mcx, c.log2_ctu));
        j->st.n_launches++; j->st.d2h_bytes += bytes;
    }
    if (g.n_ciip) { CHK(ovhip_ciip_launch(j->ctx, c.dst, intra, (const ovhip_ciip_unit *)p.at[B_CIIP], (uint32_t)g.n_ciip)); j->st.n_launches++; }
    return OVHIP_OK;
}

int flush_launch(ovhip_job *j, const ovhip_pic *dst, const ovhip_pic *refs, uint32_t n_refs, const ovhip_pic *intra, const ovhip_job_params *pr,
                 const Gathered &g, const Placement &p)
{
    ovhip_ctx *ctx = j->ctx;
    const uint32_t stages = g.sw.stages;
    const uint16_t *d_bwd = pr->lmcs ? (const uint16_t *)(p.block + p.tabs.at[T_BWD]) : nullptr;
    Chain c = {};
    c.j = j; c.timer = j; c.dst = dst; c.res = g.ordered ? &j->res : nullptr; c.log2_ctu = g.sw.log2_ctu;
    c.luts = pr->lmcs; c.d_fwd = pr->lmcs ? (const uint16_t *)(p.block + p.tabs.at[T_FWD]) : nullptr; c.d_scales = (int16_t *)j->dev[B_SCALE].p;
    chain_bind(c, p, ovhip_band_counts{}, g.n, (uint32_t)g.n_rpr, (uint32_t)g.n_affr);
    memcpy(c.cls, g.cls, sizeof(c.cls)); memcpy(c.tiny, g.tiny, sizeof(c.tiny));
    c.h_it = g.it; c.lv_start = g.lv_start; c.n_lv = g.n_lv; c.n_items = g.flow ? (uint32_t)g.n_items : 0; c.ibc = g.ibc;
    j->mvf.src = ovhip_mvfield_src{ c.d_mc, c.d_mcx, c.d_aff, c.d_rpr, c.d_affr, c.d_side, nullptr, c.n_mc, c.n_mcx, c.n_aff, c.n_rpr, c.n_affr };

    if (stages & OVHIP_STAGE_MC) CHK(launch_predict(j, c, refs, n_refs, intra, pr, g, p));
    // ---- the flow launch's state (before the residual stage: the chroma-scale launch prepares the state words as a rider) ----
    if (g.flow) {
        CHK(ordered_arm(j, &j->d_flow, ovhip_intra_flow_words(j->w, j->h)));
        // test hook (ovhip_job_test_abort_next_flow): the abort word is set on the device BEFORE the launch, so every item that has to
        // wait for another gives up at once -- a real abandoned first pass, picture incomplete and partly tagged
        if (j->test_abort && j->n_retries == 0) {
            j->test_abort = 0; j->test_abort_seen = 1;
            OV_HIP(ctx, hipMemsetAsync(j->d_flow, 0xff, sizeof(uint32_t), ctx->stream));
            *(volatile uint32_t *)j->abort_host = 1;
        }
    }
    // ---- residual (+ the inverse luma mapping where no ordered pass follows) ----
    if (stages & OVHIP_STAGE_ITX) CHK(chain_residual(c, g.ordered ? nullptr : d_bwd));
    // ---- ordered pass: one launch per level, the flow launch (its worker count: "Flow admission" above) or, on request, ONE launch (a
    // workgroup per CTU with tasks, CTU samples in LDS, neighbour CTUs chained by flags); then the inverse luma mapping ----
    if (g.ordered) {
        StageTimer t_(j, OVHIP_TIME_INTRA);
        if (g.by_ctu) {
            CHK(ordered_arm(j, &j->d_sync, ovhip_intra_sync_words(j->w, j->h, 5)));          // the smallest CTU: enough for every size
            CHK(ovhip_intra_ctu_launch(ctx, dst, &j->res, c.d_it, (const ovhip_ictu *)p.at[B_ICTU], (uint32_t)g.n_ictu, c.d_reg, pr->lmcs, c.d_scales,
                                       c.log2_ctu, j->d_sync, j->epoch, j->abort_host));
            j->st.n_launches++;
        } else {
            CHK(chain_ordered(c, g.flow ? flow_worker_count(ctx, pr->flow_workers, g.it, j->items_host, g.n_items, false) : 0));
            if (g.flow) { j->flow_launched = 1; j->st.flow_shift = (uint32_t)flow_shift_of(ctx->device); }
        }
        // the flow launches leave a hand-over bit in what they wrote: dropped by the inverse mapping's launch, or by one of its own
        CHK(chain_unmap(j, dst, 0, j->h, (pr->lmcs && (stages & OVHIP_STAGE_ITX)) ? d_bwd : nullptr, c.d_it, c.n_items ? c.n_it : 0u));
    }
    // ---- in-loop filters ----
    if (stages & OVHIP_STAGE_DBF)
        CHK(chain_deblock(c, (const ovhip_dbf_edge *)p.at[B_EV], g.n.n_edge_v, (const ovhip_dbf_edge *)p.at[B_EH], g.n.n_edge_h, &g.offs));
    ovhip_alf_pic ap;
    if (g.sw.alf_on) {
        CHK(dev_reserve(j, B_CLASS, (size_t)((j->w + 3) / 4) * ((j->h + 3) / 4)));
        ap = alf_pic_at(p.block, p.tabs, (const ovhip_alf_ctu *)(p.block + p.o_alf), (uint8_t *)j->dev[B_CLASS].p, c.log2_ctu);
    }
    CHK(chain_filters(c, g.sw.sao_on ? (const ovhip_sao_ctu *)(p.block + p.o_sao) : nullptr, g.sw.alf_on ? &ap : nullptr, 0, j->h, 0, j->h));
    OV_HIP(ctx, hipEventRecord(j->ev_done, ctx->stream));
    return OVHIP_OK;
}

} // namespace

extern "C" {

int ovhip_job_create(ovhip_ctx *ctx, int32_t w, int32_t h, ovhip_job **out)
{
    if (!ctx || !out || w <= 0 || h <= 0 || (w & 1) || (h & 1)) return OVHIP_EINVAL;
    OV_DEVICE(ctx);
    *out = nullptr;
    ovhip_job *j = (ovhip_job *)calloc(1, sizeof(*j));
    if (!j) return OVHIP_ENOMEM;
    j->ctx = ctx; j->home = ctx; j->w = w; j->h = h; j->t_stage = -1;
    const ovhip_allocator al = { pinned_alloc, pinned_free, nullptr };
    j->rec = ovhip_rec_create_ex(w, h, &al);
    if (!j->rec) { free(j); return OVHIP_ENOMEM; }
    ovhip_rec_set_dense_dbf_planes(j->rec, 0);
    int r = ovhip_pic_alloc(ctx, w, h, &j->tmp);
    if (r == OVHIP_OK && hipEventCreateWithFlags(&j->ev_h2d, hipEventDisableTiming) != hipSuccess) r = OVHIP_ENODEV;
    if (r == OVHIP_OK && hipEventCreateWithFlags(&j->ev_done, hipEventDisableTiming) != hipSuccess) r = OVHIP_ENODEV;
    if (r == OVHIP_OK && hipEventCreateWithFlags(&j->ev_rows, hipEventDisableTiming) != hipSuccess) r = OVHIP_ENODEV;
    if (r != OVHIP_OK) { ovhip_job_destroy(j); return r; }
    *out = j;
    return OVHIP_OK;
}

void ovhip_job_destroy(ovhip_job *j)
{
    if (!j) return;
    (void)hipSetDevice(j->ctx->device);
    if (j->flushed) (void)hipEventSynchronize(j->ev_done);
    for (int k = 0; k < B_COUNT; ++k) if (j->dev[k].p) (void)hipFree(j->dev[k].p);
    if (j->tmp.y) (void)ovhip_pic_free(j->ctx, &j->tmp);
    if (j->res.y) (void)ovhip_pic_free(j->ctx, &j->res);
    if (j->d_sync) (void)hipFree(j->d_sync);
    if (j->d_flow) (void)hipFree(j->d_flow);
    pinned_free(nullptr, j->items_host);
    pinned_free(nullptr, j->abort_host);
    pinned_free(nullptr, j->param_host); pinned_free(nullptr, j->mv_host); pinned_free(nullptr, j->tmvp_host);
    for (int k = 0; k < 32; ++k) for (int q = 0; q < 2; ++q) if (j->t_ev[k][q]) (void)hipEventDestroy(j->t_ev[k][q]);
    if (j->ev_h2d) (void)hipEventDestroy(j->ev_h2d);
    if (j->ev_done) (void)hipEventDestroy(j->ev_done);
    if (j->ev_rows) { if (j->rows_pending) (void)hipEventSynchronize(j->ev_rows); (void)hipEventDestroy(j->ev_rows); }
    band_free(j);
    ovhip_rec_destroy(j->rec);
    free(j);
}

ovhip_recorder *ovhip_job_recorder(ovhip_job *j) { return j ? j->rec : nullptr; }

/* Every buffer of the job sized for a picture of its size NOW (the recorder's page-locked arrays, ovhip_rec_reserve_for_picture; the
 * device copies; the staging blocks), so that no picture of a running decoder meets a growth: a device buffer that grows is hipFree
 * (a device-wide synchronisation) + hipMalloc, a page-locked one hipHostMalloc + copy + hipHostFree.  What a frame thread's job does
 * when it is created (ovhip_frame_job); a harness that keeps a hundred pre-recorded jobs does not call it.  ~30 MB of page-locked
 * and ~30 MB of device memory at 4K. */
int ovhip_job_reserve_for_picture(ovhip_job *j)
{
    if (!j) return OVHIP_EINVAL;
    OV_DEVICE(j->ctx);
    if (ovhip_rec_reserve_for_picture(j->rec) != OVHIP_OK) return ov_fail(j->ctx, OVHIP_ENOMEM, "ovhip_rec_reserve_for_picture", hipSuccess);
    const size_t P = (size_t)j->w * j->h;
    const struct { int k; size_t bytes; } want[] = {
        { B_TB, (P / 64 + 1024) * sizeof(ovhip_tb_cmd) }, { B_COEF, (P / 2 + 1024) * 2 }, { B_MC, (P / 128 + 1024) * sizeof(ovhip_mc_unit) },
        { B_MCX, (P / 256 + 1024) * sizeof(ovhip_mc_unit) }, { B_MV, (P / 256 + 1024) * 16 }, { B_AFF, (P / 1024 + 256) * sizeof(ovhip_aff_unit) },
        { B_SIDE, (P / 6 + 1024) * 4 }, { B_REG, (P / 4096 + 64) * sizeof(ovhip_lmcs_region) }, { B_SCALE, 65536 },
        { B_EV, (P / 32 + 2048) * sizeof(ovhip_dbf_edge) }, { B_EH, (P / 32 + 2048) * sizeof(ovhip_dbf_edge) }, { B_PARAM, P / 2 + ((size_t)2 << 20) },
        { B_CLASS, (size_t)((j->w + 3) / 4) * ((j->h + 3) / 4) }, { B_ITASK, (P / 64 + 1024) * sizeof(ovhip_itask) }, { B_IITEM, (P / 32 + 1024) * 4 },
        { B_TMVP, 4 * (P / 256 + 1024) * sizeof(ovhip_tmvp_cell) },
    };
    for (const auto &q : want) CHK(dev_reserve(j, q.k, q.bytes));
    CHK(pinned_reserve(j, (void **)&j->param_host, &j->param_cap, P / 2 + ((size_t)2 << 20)));
    CHK(pinned_reserve(j, (void **)&j->mv_host, &j->mv_cap, (P / 256 + 1024) * 16));
    CHK(pinned_reserve(j, (void **)&j->tmvp_host, &j->tmvp_cap, 4 * (P / 256 + 1024) * sizeof(ovhip_tmvp_cell)));
    CHK(pinned_reserve(j, (void **)&j->items_host, &j->items_cap, (P / 32 + 1024) * sizeof(uint32_t)));
    if (!j->res.y) CHK(ovhip_pic_alloc(j->ctx, j->w, j->h, &j->res));
    return OVHIP_OK;
}

int ovhip_job_begin(ovhip_job *j)
{
    if (!j) return OVHIP_EINVAL;
    OV_DEVICE(j->ctx);
    // the DMA engines may still be reading the recorder's arrays and the parameter staging block
    if (j->flushed) OV_HIP(j->ctx, hipEventSynchronize(j->ev_h2d));
    if (j->rows_pending) { OV_HIP(j->ctx, hipEventSynchronize(j->ev_rows)); j->rows_pending = 0; }
    { const int rb = band_reset(j); if (rb != OVHIP_OK) return rb; }
    ovhip_rec_reset(j->rec);
    j->dmvr_first = 0; j->n_mv = 0; j->n_tmvp = 0; j->rows_end = 0;
    j->mvf.valid = 0;
    return OVHIP_OK;
}

int ovhip_job_bind(ovhip_job *j, ovhip_ctx *ctx)
{
    if (!j) return OVHIP_EINVAL;
    if (!ctx) ctx = j->home;             // back to the context it was created on (which outlives it by contract)
    // (errors go to the context the caller holds)
    if (ctx->device != j->ctx->device) return ov_fail(ctx, OVHIP_EINVAL, "ovhip_job_bind: context of another device", hipSuccess);
    OV_DEVICE(ctx);
    if (j->flushed) {
        hipError_t e = hipEventSynchronize(j->ev_done);
        if (e != hipSuccess) return ov_fail(ctx, OVHIP_ELAUNCH, "ovhip_job_bind: hipEventSynchronize(previous flush)", e);
    }
    j->ctx = ctx;
    return OVHIP_OK;
}

static int job_flush_impl(ovhip_job *j, const ovhip_pic *dst, const ovhip_pic *refs, uint32_t n_refs, const ovhip_pic *intra,
                          const ovhip_job_params *pr);

int ovhip_job_wait(ovhip_job *j)
{
    if (!j) return OVHIP_EINVAL;
    OV_DEVICE(j->ctx);
    if (!j->flushed) return OVHIP_OK;
    hipError_t e = hipEventSynchronize(j->ev_done);
    if (e != hipSuccess) return ov_fail(j->ctx, OVHIP_ELAUNCH, "hipEventSynchronize(job)", e);
    if (band_active(j)) return band_wait_done(j);
    if (j->abort_host && *(volatile uint32_t *)j->abort_host) {
        // a workgroup of the ordered pass gave up waiting for its inputs (workgroups of several pictures' flow launches can
        // fill the compute units with pollers whose producers then find no slot): the picture is incomplete.  Re-arm, and decode
        // the picture again with one launch per level -- no workgroup of such a launch waits for another -- from the recorder's
        // arrays, which are untouched until the next ovhip_job_begin.  Every sample of dst is rewritten by a flush.
        *(volatile uint32_t *)j->abort_host = 0;
        flow_launch_abandoned(j);
        if (j->d_sync) (void)hipMemset(j->d_sync, 0, sizeof(uint32_t));
        if (j->d_flow) (void)hipMemset(j->d_flow, 0, sizeof(uint32_t));
        if (j->again.valid && j->n_retries == 0) {
            j->n_retries = 1;
            ovhip_job_params pr = j->again.pr;
            pr.stages = ((pr.stages ? pr.stages : (uint32_t)(OVHIP_STAGE_MC | OVHIP_STAGE_ITX | OVHIP_STAGE_DBF | OVHIP_STAGE_SAO | OVHIP_STAGE_ALF | OVHIP_STAGE_INTRA)) | OVHIP_STAGE_INTRA_LEVELS) & ~(uint32_t)OVHIP_STAGE_INTRA_CTU;
            pr.wait_events = nullptr; pr.n_wait_events = 0; pr.before_launch = nullptr;      // the references were done the first time
            int r = job_flush_impl(j, &j->again.dst, j->again.refs, j->again.n_refs, j->again.has_intra ? &j->again.intra : nullptr, &pr);
            if (r) return r;
            e = hipEventSynchronize(j->ev_done);
            if (e != hipSuccess) return ov_fail(j->ctx, OVHIP_ELAUNCH, "hipEventSynchronize(job, second pass)", e);
            return OVHIP_OK;
        }
        return ov_fail(j->ctx, OVHIP_ELAUNCH, "ordered pass: a CTU's bounded wait for its neighbours expired (picture incomplete)", hipSuccess);
    }
    flow_launch_clean(j);
    return OVHIP_OK;
}

const int32_t *ovhip_job_refined_mvs(ovhip_job *j, size_t *n_units)
{
    if (!j || !n_units) return nullptr;
    *n_units = j->n_mv;
    return j->mv_host;
}

const ovhip_tmvp_cell *ovhip_job_tmvp_cells(ovhip_job *j, size_t *n_entries)
{
    if (!j || !n_entries) return nullptr;
    *n_entries = j->n_tmvp;
    return j->tmvp_host;
}

int ovhip_job_last_stats(const ovhip_job *j, ovhip_job_stats *out)
{
    if (!j || !out) return OVHIP_EINVAL;
    *out = j->st;
    return OVHIP_OK;
}

int ovhip_job_time_stage(ovhip_job *j, int stage)
{
    if (!j || stage < -1 || stage >= OVHIP_TIME_COUNT) return OVHIP_EINVAL;
    OV_DEVICE(j->ctx);
    for (int k = 0; k < 32; ++k) {
        CHK(t_collect(j, k));
        for (int q = 0; q < 2 && stage >= 0; ++q)
            if (!j->t_ev[k][q]) OV_HIP(j->ctx, hipEventCreate(&j->t_ev[k][q]));
    }
    j->t_stage = stage; j->t_sum_ms = 0.0; j->t_count = 0;
    return OVHIP_OK;
}

int ovhip_job_stage_time(ovhip_job *j, double *sum_ms, uint64_t *count)
{
    if (!j || !sum_ms || !count) return OVHIP_EINVAL;
    OV_DEVICE(j->ctx);
    for (int k = 0; k < 32; ++k) CHK(t_collect(j, k));
    *sum_ms = j->t_sum_ms; *count = j->t_count;
    return OVHIP_OK;
}

int64_t ovhip_job_dmvr_rows_collect(ovhip_job *j)
{
    if (!j) return OVHIP_EINVAL;
    if (j->rows_pending) {
        ovhip_ctx *ctx = j->ctx;
        OV_DEVICE(ctx);
        hipError_t e = hipEventSynchronize(j->ev_rows);
        j->rows_pending = 0;
        if (e != hipSuccess) return ov_fail(ctx, OVHIP_ELAUNCH, "hipEventSynchronize(dmvr rows)", e);
        if (j->rows_end > j->n_mv) j->n_mv = j->rows_end;
    }
    return (int64_t)j->rows_end;
}

int64_t ovhip_job_dmvr_rows_begin_upto(ovhip_job *j, const ovhip_pic *refs, uint32_t n_refs, int32_t log2_ctu_s, size_t upto);
int64_t ovhip_job_dmvr_rows_begin(ovhip_job *j, const ovhip_pic *refs, uint32_t n_refs, int32_t log2_ctu_s)
{
    return ovhip_job_dmvr_rows_begin_upto(j, refs, n_refs, log2_ctu_s, (size_t)-1);
}

/* the same over the refined units [.., upto) only (a caller that works through a parsed picture row by row as its reference
 * pictures' rows arrive: shim/rcn_hip.c final_progressive) */
int64_t ovhip_job_dmvr_rows_begin_upto(ovhip_job *j, const ovhip_pic *refs, uint32_t n_refs, int32_t log2_ctu_s, size_t upto)
{
    if (!j) return OVHIP_EINVAL;
    // one pass in flight: the pinned result arrays may have to grow, and they keep the recorder's indexing
    const int64_t c = ovhip_job_dmvr_rows_collect(j);
    if (c < 0) return c;
    ovhip_ctx *ctx = j->ctx;
    OV_DEVICE(ctx);
    size_t n = 0;
    const ovhip_mc_unit *u = ovhip_rec_mcx_units(j->rec, &n);
    if (n > upto) n = upto;
    const size_t first = j->dmvr_first;
    if (n <= first) return (int64_t)first;
    int any = 0;
    for (size_t i = first; i < n && !any; ++i) any = (u[i].flags & OVHIP_MC_DMVR) != 0;
    if (any) {
        // the device copy of the unit list and the vector buffer keep the recorder's indexing: [first, n) lands at first
        CHK(pinned_reserve(j, (void **)&j->mv_host, &j->mv_cap, n * 16));
        if (log2_ctu_s) CHK(pinned_reserve(j, (void **)&j->tmvp_host, &j->tmvp_cap, 4 * n * sizeof(ovhip_tmvp_cell)));
        if (j->dev[B_MCX].cap < n * sizeof(ovhip_mc_unit) || j->dev[B_MV].cap < n * 16 ||
            (log2_ctu_s && j->dev[B_TMVP].cap < 4 * n * sizeof(ovhip_tmvp_cell))) {
            // grow to the picture's upper bound at once so that earlier rows' results are never moved: one refined unit
            // covers at least 8x8 luma samples
            const size_t ub = (size_t)((j->w + 7) / 8) * ((j->h + 7) / 8);
            CHK(dev_reserve(j, B_MCX, (ub > n ? ub : n) * sizeof(ovhip_mc_unit)));
            CHK(dev_reserve(j, B_MV, (ub > n ? ub : n) * 16));
            if (log2_ctu_s) CHK(dev_reserve(j, B_TMVP, 4 * (ub > n ? ub : n) * sizeof(ovhip_tmvp_cell)));
        }
        char *d_units = (char *)j->dev[B_MCX].p + first * sizeof(ovhip_mc_unit);
        int32_t *d_mv = (int32_t *)j->dev[B_MV].p + 4 * first;
        OV_HIP(ctx, hipMemcpyAsync(d_units, u + first, (n - first) * sizeof(ovhip_mc_unit), hipMemcpyHostToDevice, ctx->stream));
        ovhip_pic geom = j->tmp, same[16];
        CHK(ovhip_dmvr_search_launch(ctx, &geom, same_size_refs(&geom, refs, n_refs, same), n_refs, (const ovhip_mc_unit *)d_units,
                                     (uint32_t)(n - first), d_mv));
        CHK(store_host(ctx, j->mv_host + 4 * first, d_mv, (n - first) * 16));
        // the same vectors as entries of the picture's collocated motion plane: what the caller patches before it publishes the row
        if (log2_ctu_s) CHK(tmvp_cells(j, (const ovhip_mc_unit *)d_units, d_mv, first, n, log2_ctu_s));
        OV_HIP(ctx, hipEventRecord(j->ev_rows, ctx->stream));
        j->rows_pending = 1;
    }
    else if (log2_ctu_s) {
        // no DMVR unit among them: their plane entries are all "none" (the caller indexes the entries by unit)
        CHK(pinned_reserve(j, (void **)&j->tmvp_host, &j->tmvp_cap, 4 * n * sizeof(ovhip_tmvp_cell)));
        for (size_t i = 4 * first; i < 4 * n; ++i) { j->tmvp_host[i] = ovhip_tmvp_cell{}; j->tmvp_host[i].cell = OVHIP_TMVP_NONE; }
        j->n_tmvp = 4 * n;
    }
    j->dmvr_first = n;
    j->rows_end = n;
    return (int64_t)n;
}

int64_t ovhip_job_dmvr_rows(ovhip_job *j, const ovhip_pic *refs, uint32_t n_refs)
{
    const int64_t n = ovhip_job_dmvr_rows_begin(j, refs, n_refs, 0);
    return n < 0 ? n : ovhip_job_dmvr_rows_collect(j);
}

int ovhip_job_flush(ovhip_job *j, const ovhip_pic *dst, const ovhip_pic *refs, uint32_t n_refs, const ovhip_pic *intra,
                    const ovhip_job_params *pr)
{
    if (!j || !dst || !pr) return OVHIP_EINVAL;
    // what a second flush of the same picture needs (ovhip_job_wait re-runs the picture with one launch per level when the
    // flow launch gave up): the pictures by value, the parameter block as the caller passed it (its tables stay the caller's
    // until ovhip_job_wait has returned)
    j->again.valid = 0;
    j->n_retries = 0;
    j->mvf.valid = 0;
    const int r = job_flush_impl(j, dst, refs, n_refs, intra, pr);
    j->mvf.valid = r == OVHIP_OK;
    // (after the flush: a before_launch callback may be what fills refs[] -- ovhip_frame_submit resolves the reference pictures
    // there, while the uploads already run)
    j->again.valid = r == OVHIP_OK && n_refs <= 16;
    j->again.dst = *dst;
    for (uint32_t i = 0; i < n_refs && i < 16; ++i) j->again.refs[i] = refs[i];
    j->again.n_refs = n_refs;
    j->again.has_intra = intra != nullptr;
    if (intra) j->again.intra = *intra;
    j->again.pr = *pr;
    return r;
}

int ovhip_job_mvfield(ovhip_job *j, const ovhip_mvfield_format *fmt, void *d_vec, size_t vec_bytes, void *d_info, size_t info_bytes)
{
    if (!j) return OVHIP_EINVAL;
    if (band_active(j)) return ov_fail(j->ctx, OVHIP_EUNSUP, "ovhip_job_mvfield: the picture was submitted band-wise (its arrays live in band arenas)", hipSuccess);
    if (!j->mvf.valid) return ov_fail(j->ctx, OVHIP_EINVAL, "ovhip_job_mvfield: no whole-picture flush since ovhip_job_begin", hipSuccess);
    return ovhip_mvfield_launch(j->ctx, j->w, j->h, &j->mvf.src, fmt, d_vec, vec_bytes, d_info, info_bytes);
}

/* ovhip_job_mvfield and the wait for it: complete on the device at return (the frame thread) */
int ovhip_job_mvfield_done_(ovhip_job *j, const ovhip_mvfield_format *fmt, void *d_vec, size_t vec_bytes, void *d_info, size_t info_bytes)
{
    int r = ovhip_job_mvfield(j, fmt, d_vec, vec_bytes, d_info, info_bytes);
    if (r == OVHIP_OK && ov_sync_stream(j->ctx) != hipSuccess) r = ov_fail(j->ctx, OVHIP_ELAUNCH, "motion field output", hipGetLastError());
    return r;
}

int ovhip_job_test_abort_next_flow(ovhip_job *j)
{
    if (!j) return OVHIP_EINVAL;
    j->test_abort = 1;
    return OVHIP_OK;
}

static int job_flush_impl(ovhip_job *j, const ovhip_pic *dst, const ovhip_pic *refs, uint32_t n_refs, const ovhip_pic *intra,
                          const ovhip_job_params *pr)
{
    OV_DEVICE(j->ctx);
    Gathered g;
    Placement p;
    CHK(flush_gather(j, dst, intra, pr, g));                       // host only: the recorder's arrays, the ordered-pass mode, validation, counts
    CHK(flush_stage(j, pr, g, p));                                 // layout, fill, uploads, the callers' waits (host_us_prepare / _upload / _wait)
    const double t3 = host_now_us();
    CHK(flush_launch(j, dst, refs, n_refs, intra, pr, g, p));      // prediction .. filters, ev_done
    j->st.host_us_launch = (uint32_t)(host_now_us() - t3);
    return OVHIP_OK;
}

} // extern "C"
