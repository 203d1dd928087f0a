/* RGB pyramid on the host: the plan and the refusals the launcher shares, the check, and the definition over a picture, an optional
 * table and destinations in host memory -- the composition of the reduced-size output's twin and the twin of the RGB output (through a
 * table: of the RGB output through a colour table), not a restatement of either.  Definition: include/ovvc_hip.h, "RGB pyramid on the
 * device"; the device half is kernels_rgb_pyramid.hip.  Plain C, no HIP calls. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "ovvc_hip.h"
#include "ovvc_rgb_pyramid_priv.h"
#include "ovvc_outdst_priv.h"

/* what the RGB output (through a table: with_table) refuses of a level's size and format alone: no picture, no destination */
static int
level_format_check(const ovhip_rgb_level *g, int with_table, int size, int peak, const char **why)
{
    const ovhip_rgb_format *fmt = &g->fmt;
    int32_t coef[5], yoff;
    if (fmt->dtype > OVHIP_RGB_F32 || fmt->layout > OVHIP_RGB_PACKED || fmt->chroma_loc > 5 || fmt->full_range > 1) { *why = "bad dtype / layout / chroma location / range"; return OVHIP_EINVAL; }
    const int r = ovhip_rgb_coefs(fmt, coef, &yoff);
    if (r != OVHIP_OK) { *why = r == OVHIP_EUNSUP ? "matrix coefficients not built" : "matrix coefficients unspecified"; return r; }
    if (!ovhip_rgb_bytes(g->out_w, g->out_h, NULL, fmt)) { *why = "sizes must be positive multiples of 4"; return OVHIP_EINVAL; }
    if (with_table) {
        if (ovhip_rgb_lut_check(size, peak, NULL) != OVHIP_OK) { *why = "table size must be 17, 33 or 65 and its peak 1..65535"; return OVHIP_EINVAL; }
        if (fmt->dtype == OVHIP_RGB_U8 && peak > 255) { *why = "a U8 destination needs a table peak <= 255"; return OVHIP_EINVAL; }
    }
    *why = "";
    return OVHIP_OK;
}

int
ovhip_rgb_pyramid_plan_make_(const ovhip_pic *src, int32_t src_w, int32_t src_h, const ovhip_reduce_info *info, const ovhip_rgb_level *levels, int32_t n,
                             int with_table, int size, int peak, int have_table, ovhip_rgb_pyramid_plan_ *pl, char *why, size_t why_len)
{
    memset(pl, 0, sizeof(*pl));
#define REFUSE(code, ...) do { snprintf(why, why_len, __VA_ARGS__); return (code); } while (0)
    if (!info) REFUSE(OVHIP_EINVAL, "null info");
    if (!levels) REFUSE(OVHIP_EINVAL, "null levels");
    if (n < 1 || n > OVHIP_PYRAMID_MAX_LEVELS) REFUSE(OVHIP_EINVAL, "%d levels: 1..%d", n, OVHIP_PYRAMID_MAX_LEVELS);
    if (src) {
        const char *w;
        if ((w = ovhip_out_why_planes_(src)) || (w = ovhip_out_why_strides_(src))) REFUSE(OVHIP_EINVAL, "%s", w);
        src_w = src->w; src_h = src->h;
    }
    for (int32_t k = 0; k < n; ++k) {
        char sub[200];
        const int q = ovhip_reduce_plan_make_(src_w, src_h, info, levels[k].out_w, levels[k].out_h, &pl->red[k], sub, sizeof(sub));
        if (q != OVHIP_OK) REFUSE(q, "level %d: %s", k, sub);
    }
    /* one source: a matrix, a range and a sample location.  The reduced pictures keep the source's location: two values would shift
     * the chroma silently */
    for (int32_t k = 1; k < n; ++k)
        if (levels[k].fmt.matrix != levels[0].fmt.matrix || levels[k].fmt.full_range != levels[0].fmt.full_range || levels[k].fmt.chroma_loc != levels[0].fmt.chroma_loc)
            REFUSE(OVHIP_EINVAL, "level %d: matrix, range or chroma location differ from level 0's", k);
    if (levels[0].fmt.chroma_loc != info->chroma_loc)
        REFUSE(OVHIP_EINVAL, "the levels' chroma location %u is not the pyramid's %u", (unsigned)levels[0].fmt.chroma_loc, (unsigned)info->chroma_loc);
    for (int32_t k = 0; k < n; ++k) {
        const ovhip_rgb_level *g = &levels[k];
        const char *w = "";
        int r;
        if (!src) {
            if ((r = level_format_check(g, with_table, size, peak, &w)) != OVHIP_OK) REFUSE(r, "level %d: %s", k, w);
            continue;
        }
        /* the level's reduced picture exists nowhere: the source's planes stand in for the plan's look at them, and the destination is
         * held against the source itself below */
        const ovhip_pic red = { src->y, src->cb, src->cr, g->out_w, g->out_h, src->stride_y, src->stride_c };
        r = with_table ? ovhip_rgb_lut_plan_make_(&red, NULL, &g->fmt, size, peak, have_table, g->dst, g->dst_bytes, &pl->rgb[k], &w)
                       : ovhip_rgb_plan_make_(&red, NULL, &g->fmt, g->dst, g->dst_bytes, &pl->rgb[k], &w);
        if (r != OVHIP_OK) REFUSE(r, "level %d: %s", k, w);
        if ((w = ovhip_out_why_overlap_(src, g->dst, pl->rgb[k].bytes)) != NULL) REFUSE(OVHIP_EINVAL, "level %d: %s", k, w);
        for (int32_t j = 0; j < k; ++j)
            if (ovhip_ranges_overlap_(g->dst, pl->rgb[k].bytes, levels[j].dst, pl->rgb[j].bytes))
                REFUSE(OVHIP_EINVAL, "level %d: destination overlaps level %d's", k, j);
    }
#undef REFUSE
    pl->n = n;
    why[0] = 0;
    return OVHIP_OK;
}

int
ovhip_rgb_pyramid_check(int32_t src_w, int32_t src_h, const ovhip_reduce_info *info, const ovhip_rgb_level *levels, int32_t n, int lut_size, int lut_peak,
                        int32_t ratio[][4])
{
    ovhip_rgb_pyramid_plan_ pl;
    char why[240];
    const int r = ovhip_rgb_pyramid_plan_make_(NULL, src_w, src_h, info, levels, n, lut_size != 0, lut_size, lut_peak, 1, &pl, why, sizeof(why));
    if (ratio && levels && n >= 1 && n <= OVHIP_PYRAMID_MAX_LEVELS)
        for (int32_t k = 0; k < n; ++k) { ratio[k][0] = pl.red[k].px; ratio[k][1] = pl.red[k].qx; ratio[k][2] = pl.red[k].py; ratio[k][3] = pl.red[k].qy; }
    return r;
}

int
ovhip_rgb_pyramid_host(const ovhip_pic *src, const ovhip_reduce_info *info, const ovhip_rgb_level *levels, int32_t n, int lut_size, int lut_peak,
                       const uint16_t *host_table)
{
    if (!src) return OVHIP_EINVAL;
    const int with_table = lut_size != 0;
    ovhip_rgb_pyramid_plan_ pl;
    char why[240];
    int r = ovhip_rgb_pyramid_plan_make_(src, 0, 0, info, levels, n, with_table, lut_size, lut_peak, host_table != NULL, &pl, why, sizeof(why));
    if (r != OVHIP_OK) return r;
    if (with_table && ovhip_rgb_lut_first_above_(lut_size, lut_peak, host_table) >= 0) return OVHIP_EINVAL;      /* (the one refusal the levels' twin would make) */
    /* every level's reduced picture before anything is written: all or nothing */
    uint16_t *mem[OVHIP_PYRAMID_MAX_LEVELS] = { NULL };
    ovhip_pic red[OVHIP_PYRAMID_MAX_LEVELS];
    for (int32_t k = 0; k < n && r == OVHIP_OK; ++k) {
        const int32_t w = levels[k].out_w, h = levels[k].out_h;
        const size_t ny = (size_t)w * (size_t)h, nc = ny / 4;
        if (!(mem[k] = (uint16_t *)malloc((ny + 2 * nc) * sizeof(uint16_t)))) { r = OVHIP_ENOMEM; break; }
        red[k] = (ovhip_pic){ mem[k], mem[k] + ny, mem[k] + ny + nc, w, h, w, w / 2 };
        r = ovhip_output_reduce_host(src, info, &red[k]);
    }
    for (int32_t k = 0; k < n && r == OVHIP_OK; ++k)
        r = with_table ? ovhip_rgb_lut_host(red[k].y, red[k].cb, red[k].cr, red[k].w, red[k].h, red[k].stride_y, red[k].stride_c, NULL, &levels[k].fmt, lut_size, lut_peak,
                                            host_table, levels[k].dst, levels[k].dst_bytes)
                       : ovhip_rgb_host(red[k].y, red[k].cb, red[k].cr, red[k].w, red[k].h, red[k].stride_y, red[k].stride_c, NULL, &levels[k].fmt, levels[k].dst,
                                        levels[k].dst_bytes);
    for (int32_t k = 0; k < n; ++k) free(mem[k]);
    return r;
}
