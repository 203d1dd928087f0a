/* Output ladder on the host: the plan and the refusals the launcher shares, the check, and the definition over a picture and
 * destinations in host memory -- the composition of the reduced-size output's twin and the surface output's twin, not a restatement of
 * either.  Definition: include/ovvc_hip.h, "Output ladder on the device"; the device half is kernels_ladder.hip.
 * Plain C, no HIP calls. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "ovvc_hip.h"
#include "ovvc_ladder_priv.h"
#include "ovvc_outdst_priv.h"

int
ovhip_ladder_plan_make_(const ovhip_pic *src, int32_t src_w, int32_t src_h, const ovhip_reduce_info *info, const ovhip_ladder_rung *rungs, int32_t n,
                        ovhip_ladder_plan_ *pl, char *why, size_t why_len)
{
    char dummy[4];
    if (!why) { why = dummy; why_len = sizeof(dummy); }
    memset(pl, 0, sizeof(*pl));
#define REFUSE(code, ...) do { snprintf(why, why_len, __VA_ARGS__); return (code); } while (0)
    if (!info) REFUSE(OVHIP_EINVAL, "null info");
    if (!rungs) REFUSE(OVHIP_EINVAL, "null rungs");
    if (n < 1 || n > OVHIP_LADDER_MAX_RUNGS) REFUSE(OVHIP_EINVAL, "%d rungs: 1..%d", n, OVHIP_LADDER_MAX_RUNGS);
    if (src) {
        const char *w;
        if ((w = ovhip_out_why_planes_(src)) || (w = ovhip_out_why_strides_(src))) REFUSE(OVHIP_EINVAL, "%s", w);
        src_w = src->w; src_h = src->h;
    }
    for (int32_t r = 0; r < n; ++r) {
        const ovhip_ladder_rung *g = &rungs[r];
        char sub[200];
        const int q = ovhip_reduce_plan_make_(src_w, src_h, info, g->out_w, g->out_h, &pl->red[r], sub, sizeof(sub));
        if (q != OVHIP_OK) REFUSE(q, "rung %d: %s", r, sub);
    }
    for (int32_t r = 0; r < n; ++r) {
        const ovhip_ladder_rung *g = &rungs[r];
        const char *w = "";
        if (!src) {
            /* no picture, no destination: the format's own refusals and the layout's */
            if (ovhip_surface_format_check_(&g->fmt, &w) != OVHIP_OK) REFUSE(OVHIP_EINVAL, "rung %d: %s", r, w);
            if (!ovhip_surface_bytes(g->out_w, g->out_h, NULL, &g->fmt)) REFUSE(OVHIP_EINVAL, "rung %d: the surface's pitches or offsets", r);
            continue;
        }
        /* the surface of the rung's reduced picture: a picture of out_w x out_h that exists nowhere, so the source's planes stand in
         * for the plan's look at them and the destination is held against the source itself below */
        const ovhip_pic red = { src->y, src->cb, src->cr, g->out_w, g->out_h, src->stride_y, src->stride_c };
        if (ovhip_surface_plan_make_(&red, NULL, &g->fmt, g->dst, g->dst_bytes, &pl->surf[r], &w) != OVHIP_OK) {
            if (pl->surf[r].bytes > g->dst_bytes) REFUSE(OVHIP_EINVAL, "rung %d: %s: %zu bytes given, the surface needs %zu", r, w, g->dst_bytes, pl->surf[r].bytes);
            REFUSE(OVHIP_EINVAL, "rung %d: %s", r, w);
        }
        if ((w = ovhip_out_why_overlap_(src, g->dst, pl->surf[r].bytes)) != NULL) REFUSE(OVHIP_EINVAL, "rung %d: %s", r, w);
        for (int32_t j = 0; j < r; ++j)
            if (ovhip_ranges_overlap_(g->dst, pl->surf[r].bytes, rungs[j].dst, pl->surf[j].bytes))
                REFUSE(OVHIP_EINVAL, "rung %d: destination overlaps rung %d's", r, j);
    }
#undef REFUSE
    pl->n = n;
    why[0] = 0;
    return OVHIP_OK;
}

int
ovhip_ladder_check(int32_t src_w, int32_t src_h, const ovhip_reduce_info *info, const ovhip_ladder_rung *rungs, int32_t n, int32_t ratio[][4])
{
    ovhip_ladder_plan_ pl;
    const int r = ovhip_ladder_plan_make_(NULL, src_w, src_h, info, rungs, n, &pl, NULL, 0);
    if (ratio && rungs && n >= 1 && n <= OVHIP_LADDER_MAX_RUNGS)
        for (int32_t k = 0; k < n; ++k) { ratio[k][0] = pl.red[k].px; ratio[k][1] = pl.red[k].qx; ratio[k][2] = pl.red[k].py; ratio[k][3] = pl.red[k].qy; }
    return r;
}

int
ovhip_ladder_host(const ovhip_pic *src, const ovhip_reduce_info *info, const ovhip_ladder_rung *rungs, int32_t n)
{
    if (!src) return OVHIP_EINVAL;
    ovhip_ladder_plan_ pl;
    int r = ovhip_ladder_plan_make_(src, 0, 0, info, rungs, n, &pl, NULL, 0);
    if (r != OVHIP_OK) return r;
    /* every rung's reduced picture before anything is written: all or nothing */
    uint16_t *mem[OVHIP_LADDER_MAX_RUNGS] = { NULL };
    ovhip_pic red[OVHIP_LADDER_MAX_RUNGS];
    for (int32_t k = 0; k < n && r == OVHIP_OK; ++k) {
        const int32_t w = rungs[k].out_w, h = rungs[k].out_h;
        const size_t ny = (size_t)w * (size_t)h, nc = ny / 4;
        if (!(mem[k] = (uint16_t *)malloc((ny + 2 * nc) * sizeof(uint16_t)))) { r = OVHIP_ENOMEM; break; }
        red[k] = (ovhip_pic){ mem[k], mem[k] + ny, mem[k] + ny + nc, w, h, w, w / 2 };
        r = ovhip_output_reduce_host(src, info, &red[k]);
    }
    for (int32_t k = 0; k < n && r == OVHIP_OK; ++k)
        r = ovhip_surface_host(red[k].y, red[k].cb, red[k].cr, red[k].w, red[k].h, red[k].stride_y, red[k].stride_c, NULL, &rungs[k].fmt,
                               rungs[k].dst, rungs[k].dst_bytes);
    for (int32_t k = 0; k < n; ++k) free(mem[k]);
    return r;
}
