/* Output ladder through a colour table, on the host: the plan and the refusals the launcher shares, the check, and the definition over
 * a picture, a table and destinations in host memory -- the composition of the reduced-size output's twin and the twin of the surface
 * output through a table, not a restatement of either.  Definition: include/ovvc_hip.h, "Output ladder through a colour table"; the
 * device half is kernels_ladder_lut.hip.  Plain C, no HIP calls. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "ovvc_hip.h"
#include "ovvc_ladder_lut_priv.h"

int
ovhip_ladder_lut_plan_make_(const ovhip_pic *src, int32_t src_w, int32_t src_h, const ovhip_reduce_info *info, const ovhip_ladder_rung *rungs, int32_t n,
                            const ovhip_surface_conv *conv, int size, int peak, int have_table, ovhip_ladder_lut_plan_ *pl, char *why, size_t why_len)
{
    memset(pl->sl, 0, sizeof(pl->sl));
#define REFUSE(code, ...) do { snprintf(why, why_len, __VA_ARGS__); return (code); } while (0)
    int r = ovhip_ladder_plan_make_(src, src_w, src_h, info, rungs, n, &pl->lad, why, why_len);
    if (r != OVHIP_OK) return r;
    const char *w = "";
    if ((r = ovhip_surface_conv_check_(conv, &w)) != OVHIP_OK) REFUSE(r, "%s", w);
    /* the reduced picture keeps the source's sample location: two values would shift the chroma silently */
    if (conv->src_chroma_loc != info->chroma_loc)
        REFUSE(OVHIP_EINVAL, "the conversion's source chroma location %d is not the ladder's %d", conv->src_chroma_loc, info->chroma_loc);
    for (int32_t k = 0; k < n; ++k) {
        const ovhip_ladder_rung *g = &rungs[k];
        if (!src) {
            /* no picture, no destination: what the surface output through a table refuses of a format and a table (its rule for the
             * sizes, multiples of 4, is the reduced-size output's already) */
            if (!have_table) REFUSE(OVHIP_EINVAL, "null table");
            if ((r = ovhip_surface_lut_check(conv, &g->fmt, size, peak)) != OVHIP_OK) REFUSE(r, "table size must be 17, 33 or 65 and its peak 1..65535");
            continue;
        }
        /* the rung's reduced picture exists nowhere: the source's planes stand in for the plan's look at them, as in the ladder's plan */
        const ovhip_pic red = { src->y, src->cb, src->cr, g->out_w, g->out_h, src->stride_y, src->stride_c };
        if ((r = ovhip_surface_lut_plan_make_(&red, NULL, conv, &g->fmt, size, peak, have_table, g->dst, g->dst_bytes, &pl->sl[k], &w)) != OVHIP_OK)
            REFUSE(r, "rung %d: %s", k, w);
    }
#undef REFUSE
    why[0] = 0;
    return OVHIP_OK;
}

int
ovhip_ladder_lut_check(int32_t src_w, int32_t src_h, const ovhip_reduce_info *info, const ovhip_ladder_rung *rungs, int32_t n, const ovhip_surface_conv *conv,
                       int size, int peak, int32_t ratio[][4])
{
    ovhip_ladder_lut_plan_ pl;
    char why[240];
    const int r = ovhip_ladder_lut_plan_make_(NULL, src_w, src_h, info, rungs, n, conv, size, peak, 1, &pl, why, sizeof(why));
    if (ratio && rungs && n >= 1 && n <= OVHIP_LADDER_MAX_RUNGS)
        for (int32_t k = 0; k < n; ++k) {
            const ovhip_reduce_plan_ *p = &pl.lad.red[k];
            ratio[k][0] = p->px; ratio[k][1] = p->qx; ratio[k][2] = p->py; ratio[k][3] = p->qy;
        }
    return r;
}

int
ovhip_ladder_lut_host(const ovhip_pic *src, const ovhip_reduce_info *info, const ovhip_ladder_rung *rungs, int32_t n, const ovhip_surface_conv *conv,
                      int size, int peak, const uint16_t *host_table)
{
    if (!src) return OVHIP_EINVAL;
    ovhip_ladder_lut_plan_ pl;
    char why[240];
    int r = ovhip_ladder_lut_plan_make_(src, 0, 0, info, rungs, n, conv, size, peak, host_table != NULL, &pl, why, sizeof(why));
    if (r != OVHIP_OK) return r;
    if (ovhip_rgb_lut_first_above_(size, peak, host_table) >= 0) return OVHIP_EINVAL;      /* (the one refusal the rungs' twin would make) */
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
        r = ovhip_surface_lut_host(red[k].y, red[k].cb, red[k].cr, red[k].w, red[k].h, red[k].stride_y, red[k].stride_c, NULL, conv, &rungs[k].fmt, size, peak,
                                   host_table, rungs[k].dst, rungs[k].dst_bytes);
    for (int32_t k = 0; k < n; ++k) free(mem[k]);
    return r;
}
