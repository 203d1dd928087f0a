/* RGB output on the host: the coefficients, the refusals the launcher shares, and the definition over planes in host
 * memory.  Definition: include/ovvc_hip.h, "RGB output on the device"; the device half is kernels_rgb.hip.
 * Plain C, no HIP calls of its own. */
#include <string.h>
#include "ovvc_hip.h"
#include "ovvc_dpb_priv.h"
#include "ovvc_outdst_priv.h"

/* round(p / q) for p, q > 0 (no coefficient is a tie: tests/spec_rgb.py asserts it on the exact rationals) */
static int32_t rnd_div(uint64_t p, uint64_t q) { return (int32_t)((2 * p + q) / (2 * q)); }

int
ovhip_rgb_coefs(const ovhip_rgb_format *fmt, int32_t coef[5], int32_t *yoff)
{
    if (!fmt || !coef || !yoff || fmt->full_range > 1 || fmt->dtype > OVHIP_RGB_F32) return OVHIP_EINVAL;
    uint64_t kr, kb;                                       /* in 1 / 10000 */
    switch (fmt->matrix) {
    case 1: kr = 2126; kb = 722; break;
    case 5: case 6: kr = 2990; kb = 1140; break;
    case 9: kr = 2627; kb = 593; break;
    case 2: return OVHIP_EINVAL;                           /* unspecified: the caller must decide */
    default: return OVHIP_EUNSUP;
    }
    const uint64_t one = 10000, kg = one - kr - kb;
    const uint64_t peak = fmt->dtype == OVHIP_RGB_U8 ? 255 : 1023;
    const uint64_t dy = fmt->full_range ? 1023 : 876, dc = fmt->full_range ? 1023 : 896;
    const uint64_t s = (uint64_t)1 << 14;
    coef[0] = rnd_div(s * peak, dy);                                            /* cy = sy                  */
    coef[1] = rnd_div(s * 2 * peak * (one - kr), dc * one);                     /* rv = 2 sc (1 - Kr)       */
    coef[2] = rnd_div(s * 2 * peak * (one - kb) * kb, dc * one * kg);           /* gu = bu Kb / Kg          */
    coef[3] = rnd_div(s * 2 * peak * (one - kr) * kr, dc * one * kg);           /* gv = rv Kr / Kg          */
    coef[4] = rnd_div(s * 2 * peak * (one - kb), dc * one);                     /* bu = 2 sc (1 - Kb)       */
    *yoff = fmt->full_range ? 0 : 64;
    return OVHIP_OK;
}

static int elem_bytes(int dtype) { return dtype == OVHIP_RGB_U8 ? 1 : (dtype == OVHIP_RGB_F32 ? 4 : 2); }

/* W x H and the first luma sample of the window; 0: the sizes are no positive multiples of 4 or the window leaves nothing */
static int
window_geom(int32_t w, int32_t h, const ovhip_window *win, ovhip_rgb_plan_ *p)
{
    return w > 0 && h > 0 && !(w & 3) && !(h & 3) && ovhip_out_window_(w, h, win, &p->x0, &p->y0, &p->W, &p->H);
}

size_t
ovhip_rgb_bytes(int32_t w, int32_t h, const ovhip_window *win, const ovhip_rgb_format *fmt)
{
    ovhip_rgb_plan_ p;
    if (!fmt || fmt->dtype > OVHIP_RGB_F32 || fmt->layout > OVHIP_RGB_PACKED || !window_geom(w, h, win, &p)) return 0;
    return (size_t)3 * (size_t)p.W * (size_t)p.H * (size_t)elem_bytes(fmt->dtype);
}

int
ovhip_rgb_plan_make_(const ovhip_pic *pic, const ovhip_window *win, const ovhip_rgb_format *fmt, const void *dst, size_t dst_bytes,
                     ovhip_rgb_plan_ *plan, const char **why)
{
    const char *dummy;
    if (!why) why = &dummy;
    *why = "null argument";
    if (!pic || !fmt || !plan) return OVHIP_EINVAL;
    memset(plan, 0, sizeof(*plan));
    if (fmt->dtype > OVHIP_RGB_F32 || fmt->layout > OVHIP_RGB_PACKED || fmt->chroma_loc > 5 || fmt->full_range > 1) { *why = "bad dtype / layout / chroma location / range"; return OVHIP_EINVAL; }
    const int r = ovhip_rgb_coefs(fmt, plan->coef, &plan->yoff);
    if (r != OVHIP_OK) { *why = r == OVHIP_EUNSUP ? "matrix coefficients not built" : "matrix coefficients unspecified"; return r; }
    if (!dst) { *why = "null destination"; return OVHIP_EINVAL; }
    OVHIP_OUT_REFUSE_(ovhip_out_why_planes_(pic));
    if (pic->w <= 0 || pic->h <= 0 || (pic->w & 3) || (pic->h & 3)) { *why = "sizes must be positive multiples of 4"; return OVHIP_EINVAL; }
    OVHIP_OUT_REFUSE_(ovhip_out_why_strides_(pic));
    if (!window_geom(pic->w, pic->h, win, plan)) { *why = "the window leaves nothing"; return OVHIP_EINVAL; }
    plan->es = elem_bytes(fmt->dtype);
    plan->bytes = (size_t)3 * (size_t)plan->W * (size_t)plan->H * (size_t)plan->es;
    OVHIP_OUT_REFUSE_(ovhip_out_why_small_(dst_bytes, plan->bytes));               /* (the size before the alignment: this plan's order) */
    OVHIP_OUT_REFUSE_(ovhip_out_why_unaligned_(dst, plan->es));
    OVHIP_OUT_REFUSE_(ovhip_out_why_overlap_(pic, dst, plan->bytes));
    plan->a = fmt->chroma_loc & 1;
    plan->b = fmt->chroma_loc < 2 ? 1 : (fmt->chroma_loc < 4 ? 0 : 2);
    plan->peak = fmt->dtype == OVHIP_RGB_U8 ? 255 : 1023;
    *why = "";
    return OVHIP_OK;
}

int
ovhip_rgb_host(const uint16_t *y, const uint16_t *cb, const uint16_t *cr, int32_t w, int32_t h, int32_t stride_y, int32_t stride_c,
               const ovhip_window *win, const ovhip_rgb_format *fmt, void *dst, size_t dst_bytes)
{
    const ovhip_pic pic = { (uint16_t *)y, (uint16_t *)cb, (uint16_t *)cr, w, h, stride_y, stride_c };
    ovhip_rgb_plan_ p;
    const int r = ovhip_rgb_plan_make_(&pic, win, fmt, dst, dst_bytes, &p, NULL);
    if (r != OVHIP_OK) return r;
    const float to_unit = (float)(1.0 / 1023);
    const size_t plane = (size_t)p.W * (size_t)p.H;
    for (int32_t oy = 0; oy < p.H; ++oy) {
        for (int32_t ox = 0; ox < p.W; ++ox) {
            int32_t rgb[3];
            ovhip_rgb_pixel_(&pic, &p, p.x0 + ox, p.y0 + oy, p.peak, rgb);
            for (int c = 0; c < 3; ++c) {
                const size_t e = fmt->layout == OVHIP_RGB_PLANAR ? (size_t)c * plane + (size_t)oy * p.W + ox : ((size_t)oy * p.W + ox) * 3 + c;
                ovhip_rgb_put_(dst, e, fmt->dtype, rgb[c], to_unit);
            }
        }
    }
    return OVHIP_OK;
}
