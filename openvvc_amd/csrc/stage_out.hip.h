// stage_out.hip.h -- the synchronous convenience of an output that leaves as several HOST destinations from one launch
// (ovhip_pic_output_ladder, ovhip_pic_output_ladder_lut, ovhip_pic_output_rgb_pyramid): the destinations planned behind one another in
// the context's scratch (ovhip_stage_plan_, ovvc_outdst_priv.h: plain C, tools/host_check/check_stage.c), the launch into the scratch,
// the copies back, the wait.  Host code only.
#pragma once
#include "ovvc_common.hip.h"
#include "ovvc_dpb_priv.h"
#include "ovvc_outdst_priv.h"

namespace {

#define OV_STAGE_MAX 8
static_assert(OVHIP_LADDER_MAX_RUNGS <= OV_STAGE_MAX && OVHIP_PYRAMID_MAX_LEVELS <= OV_STAGE_MAX, "a ladder and a pyramid fit a stage");

// the n items (T: ovhip_ladder_rung or ovhip_rgb_level) as the planner takes them -- host destination, bytes given, bytes needed (need_of(item);
// 0: the size function refused) --, and `dev`: the items again with the destinations a launch is to write
template <class T> struct OvStaged {
    const T *items; int n;
    void *dst[OV_STAGE_MAX]; size_t given[OV_STAGE_MAX], need[OV_STAGE_MAX];
    T dev[OV_STAGE_MAX];
    template <class Need> OvStaged(const T *items_, int n_, Need need_of) : items(items_), n(n_)
    {
        for (int k = 0; k < n; ++k) { dst[k] = items[k].dst; given[k] = items[k].dst_bytes; need[k] = need_of(items[k]); }
    }
    const T *with(void *const *d, const size_t *bytes)
    {
        for (int k = 0; k < n; ++k) { dev[k] = items[k]; dev[k].dst = d[k]; dev[k].dst_bytes = bytes[k]; }
        return dev;
    }
};

// The caller's:
//   launch(items)     the output's launch of these items; it words its own refusals in ctx->err
//   dry()             the plan's refusals that need no destination, under the caller's name in ctx->err
//   copy(item, host)  enqueues the copy of a launched item from its place in the scratch back to the host destination
// who: the calling function, the prefix of every error text; noun: what an item is called ("rung", "level").
// A refused request allocates nothing: the scratch grows only behind every refusal that can be had without it.
template <class T, class Launch, class Dry, class Copy>
int ov_stage_out(ovhip_ctx *ctx, const char *who, const char *noun, OvStaged<T> &st, Launch launch, Dry dry, Copy copy)
{
    size_t off[OV_STAGE_MAX], total;
    int k, j;
    const int p = ovhip_stage_plan_(st.n, st.dst, st.given, st.need, off, &total, &k, &j);
    if (p == OVHIP_STAGE_UNFIT_) {
        /* no size, a null or too small host destination: the launch refuses each before it looks at the pointer's memory, and words the reason */
        const int q = launch(st.items);
        return q != OVHIP_OK ? q : OVHIP_EINVAL;
    }
    if (p == OVHIP_STAGE_OVERLAP_) {
        snprintf(ctx->err, sizeof(ctx->err), "%s: %s %d: destination overlaps %s %d's", who, noun, k, noun, j);
        return OVHIP_EINVAL;
    }
    int r = dry();
    if (r == OVHIP_OK) r = ov_scratch(ctx, total, 0);
    if (r != OVHIP_OK) return r;
    void *d[OV_STAGE_MAX];
    for (k = 0; k < st.n; ++k) d[k] = (char *)ctx->scratch_d + off[k];
    if ((r = launch(st.with(d, st.need))) != OVHIP_OK) return r;
    hipError_t e = hipSuccess;
    for (k = 0; k < st.n && e == hipSuccess; ++k) e = copy(st.dev[k], st.dst[k]);
    if (e != hipSuccess) {
        char what[96];
        snprintf(what, sizeof(what), "%s: D2H", who);
        return ov_fail(ctx, OVHIP_ENODEV, what, e);
    }
    if (ov_sync_stream(ctx) != hipSuccess) return ov_fail(ctx, OVHIP_ELAUNCH, who, hipGetLastError());
    return OVHIP_OK;
}

// a launched rung (accepted by the launch) back to the host: the rows' own bytes only, what lies between them in host memory stays as it was
static inline hipError_t ov_stage_rung_back(ovhip_ctx *ctx, const ovhip_pic *pic, const ovhip_ladder_rung &g, void *host)
{
    const ovhip_pic red = { pic->y, pic->cb, pic->cr, g.out_w, g.out_h, pic->stride_y, pic->stride_c };
    ovhip_surface_plan_ p;
    (void)ovhip_surface_plan_make_(&red, nullptr, &g.fmt, g.dst, g.dst_bytes, &p, nullptr);
    hipError_t e = hipSuccess;
    for (int q = 0; q < p.n_planes && e == hipSuccess; ++q)
        e = hipMemcpy2DAsync((char *)host + p.off[q], p.pitch[q], (char *)g.dst + p.off[q], p.pitch[q], (size_t)p.elems[q] * p.es, (size_t)p.rows[q],
                             hipMemcpyDeviceToHost, ctx->stream);
    return e;
}

} // namespace
