/* Reduced-size output on the host: the refusals and the plan the launcher shares, and the definition over planes in host memory.
 * Definition: include/ovvc_hip.h, "Reduced-size output on the device"; the device half is kernels_reduce.hip.
 * Plain C, no HIP calls. */
#include <stdio.h>
#include <string.h>
#include "ovvc_hip.h"
#include "ovvc_reduce_priv.h"
#include "ovvc_outdst_priv.h"

static int32_t gcd32(int32_t a, int32_t b) { while (b) { const int32_t t = a % b; a = b; b = t; } return a; }

static int bad_size(int32_t v) { return v <= 0 || (v & 3) || v > OVHIP_REDUCE_MAX_DIM; }

int
ovhip_reduce_plan_make_(int32_t src_w, int32_t src_h, const ovhip_reduce_info *info, int32_t dst_w, int32_t dst_h,
                        ovhip_reduce_plan_ *pl, char *why, size_t why_len)
{
    char dummy[4];
    if (!why) { why = dummy; why_len = sizeof(dummy); }
    memset(pl, 0, sizeof(*pl));
#define REFUSE(code, ...) do { snprintf(why, why_len, __VA_ARGS__); return (code); } while (0)
    if (!info) REFUSE(OVHIP_EINVAL, "null info");
    if (bad_size(src_w) || bad_size(src_h) || bad_size(dst_w) || bad_size(dst_h))
        REFUSE(OVHIP_EINVAL, "%dx%d -> %dx%d: sizes have to be positive multiples of 4, at most %d", src_w, src_h, dst_w, dst_h, OVHIP_REDUCE_MAX_DIM);
    if (info->chroma_loc > 5) REFUSE(OVHIP_EINVAL, "chroma_loc %d: 0..5", info->chroma_loc);
    if (info->rsv[0] || info->rsv[1] || info->rsv[2]) REFUSE(OVHIP_EINVAL, "rsv must be 0");
    if (!ovhip_out_window_(src_w, src_h, &info->win, &pl->x0, &pl->y0, &pl->Ws, &pl->Hs)) REFUSE(OVHIP_EINVAL, "the window leaves nothing");
    if ((pl->Ws | pl->Hs) & 3) REFUSE(OVHIP_EINVAL, "the window leaves %dx%d: not multiples of 4", pl->Ws, pl->Hs);
    pl->Wd = dst_w; pl->Hd = dst_h;
    const int32_t gx = gcd32(pl->Ws, dst_w), gy = gcd32(pl->Hs, dst_h);
    pl->px = pl->Ws / gx; pl->qx = dst_w / gx; pl->py = pl->Hs / gy; pl->qy = dst_h / gy;
    if (dst_w > pl->Ws || dst_h > pl->Hs)
        REFUSE(OVHIP_EUNSUP, "%dx%d -> %dx%d is up-sampling: that is the resampler's (ovhip_output_scale_*)", pl->Ws, pl->Hs, dst_w, dst_h);
    if (pl->Ws > OVHIP_REDUCE_MAX_RATIO * dst_w || pl->Hs > OVHIP_REDUCE_MAX_RATIO * dst_h)
        REFUSE(OVHIP_EUNSUP, "%dx%d -> %dx%d: the ratio is above %d on an axis: reduce twice", pl->Ws, pl->Hs, dst_w, dst_h, OVHIP_REDUCE_MAX_RATIO);
    if (pl->px > OVHIP_REDUCE_MAX_P || pl->py > OVHIP_REDUCE_MAX_P)
        REFUSE(OVHIP_EUNSUP, "%dx%d -> %dx%d: p/q = %d/%d, %d/%d with p above %d: pick sizes with a larger common divisor",
               pl->Ws, pl->Hs, dst_w, dst_h, pl->px, pl->qx, pl->py, pl->qy, OVHIP_REDUCE_MAX_P);
#undef REFUSE
    const int32_t a = info->chroma_loc & 1, b = info->chroma_loc < 2 ? 1 : (info->chroma_loc < 4 ? 0 : 2);
    pl->sgx = (pl->px - pl->qx) * (1 - a);
    pl->sgy = (pl->py - pl->qy) * (1 - b);
    pl->n = 16u * (uint32_t)pl->px * (uint32_t)pl->py;
    why[0] = 0;
    return OVHIP_OK;
}

const char *
ovhip_reduce_why_pics_(const ovhip_pic *src, const ovhip_pic *dst)
{
    const char *w;
    if ((w = ovhip_out_why_planes_(src)) || (w = ovhip_out_why_planes_(dst))) return w;
    if ((w = ovhip_out_why_strides_(src)) || (w = ovhip_out_why_strides_(dst))) return w;
    if (src->w <= 0 || src->h <= 0 || dst->w <= 0 || dst->h <= 0) return NULL;          /* (no samples: nothing overlaps; the plan refuses next) */
    const uint16_t *dp[3] = { dst->y, dst->cb, dst->cr };
    for (int k = 0; k < 3; ++k) {
        const size_t n = ((size_t)((k ? dst->h / 2 : dst->h) - 1) * (size_t)(k ? dst->stride_c : dst->stride_y) + (size_t)(k ? dst->w / 2 : dst->w)) * 2;
        if (ovhip_out_why_overlap_(src, dp[k], n)) return "dst aliases src";
    }
    return NULL;
}

int
ovhip_output_reduce_check(int32_t src_w, int32_t src_h, const ovhip_reduce_info *info, int32_t dst_w, int32_t dst_h, int32_t ratio[4])
{
    if (!info || !ratio) return OVHIP_EINVAL;
    ovhip_reduce_plan_ pl;
    const int r = ovhip_reduce_plan_make_(src_w, src_h, info, dst_w, dst_h, &pl, NULL, 0);
    ratio[0] = pl.px; ratio[1] = pl.qx; ratio[2] = pl.py; ratio[3] = pl.qy;
    return r;
}

uint32_t
ovhip_output_reduce_divide(uint32_t num, uint32_t n)
{
    return n ? ovhip_reduce_div_(num, n, 1.0f / (float)n) : 0;
}

/* one plane: S_w x S_h samples at src into D_w x D_h at dst */
static void
reduce_plane(const uint16_t *src, int32_t sstride, int32_t Sw, int32_t Sh, uint16_t *dst, int32_t dstride, int32_t Dw, int32_t Dh,
             const ovhip_reduce_plan_ *pl, int32_t sgx, int32_t sgy)
{
    const int32_t px = pl->px, qx = pl->qx, py = pl->py, qy = pl->qy;
    const int32_t n = (int32_t)pl->n;
    for (int32_t ky = 0; ky < Dh; ++ky) {
        const int32_t y0 = ovhip_reduce_first_(ky, py, qy, sgy, Sh), y1 = ovhip_reduce_last_(ky, py, qy, sgy, Sh);
        for (int32_t kx = 0; kx < Dw; ++kx) {
            const int32_t x0 = ovhip_reduce_first_(kx, px, qx, sgx, Sw), x1 = ovhip_reduce_last_(kx, px, qx, sgx, Sw);
            int32_t V = 0;
            for (int32_t jy = y0; jy <= y1; ++jy) {
                const uint16_t *row = src + (size_t)jy * (size_t)sstride;
                int32_t h = 0;
                for (int32_t jx = x0; jx <= x1; ++jx) h += ovhip_reduce_weight_(kx, jx, px, qx, sgx, Sw) * (int32_t)row[jx];
                V += ovhip_reduce_weight_(ky, jy, py, qy, sgy, Sh) * h;
            }
            dst[(size_t)ky * (size_t)dstride + kx] = (uint16_t)((V + n / 2) / n);
        }
    }
}

int
ovhip_output_reduce_host(const ovhip_pic *src, const ovhip_reduce_info *info, const ovhip_pic *dst)
{
    if (!src || !info || !dst) return OVHIP_EINVAL;
    if (ovhip_reduce_why_pics_(src, dst)) return OVHIP_EINVAL;
    ovhip_reduce_plan_ pl;
    const int r = ovhip_reduce_plan_make_(src->w, src->h, info, dst->w, dst->h, &pl, NULL, 0);
    if (r != OVHIP_OK) return r;
    reduce_plane(src->y + (size_t)pl.y0 * (size_t)src->stride_y + pl.x0, src->stride_y, pl.Ws, pl.Hs, dst->y, dst->stride_y, pl.Wd, pl.Hd, &pl, 0, 0);
    const size_t co = (size_t)(pl.y0 / 2) * (size_t)src->stride_c + (size_t)(pl.x0 / 2);
    reduce_plane(src->cb + co, src->stride_c, pl.Ws / 2, pl.Hs / 2, dst->cb, dst->stride_c, pl.Wd / 2, pl.Hd / 2, &pl, pl.sgx, pl.sgy);
    reduce_plane(src->cr + co, src->stride_c, pl.Ws / 2, pl.Hs / 2, dst->cr, dst->stride_c, pl.Wd / 2, pl.Hd / 2, &pl, pl.sgx, pl.sgy);
    return OVHIP_OK;
}
