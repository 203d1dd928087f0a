/* ovvc_outdst_priv.h -- what the host twins of the picture outputs that write a caller's destination share (ovvc_rgb.c, ovvc_surface.c):
 * the cropping window's geometry and the checks of a picture and a destination, one at a time.  A check answers with the reason of its
 * refusal (a string literal, what the plans hand out as *why) or NULL; the ORDER in which a plan asks is the plan's own, since a
 * caller with two faults at once is told the first.  Plain C, no HIP calls; `pic` is only looked at, so it may hold host pointers. */
#ifndef OVVC_OUTDST_PRIV_H
#define OVVC_OUTDST_PRIV_H
#include "ovvc_hip.h"

/* the window of a w x h picture: its first luma sample and its size W x H; 0: it leaves nothing */
static inline int
ovhip_out_window_(int32_t w, int32_t h, const ovhip_window *win, int32_t *x0, int32_t *y0, int32_t *W, int32_t *H)
{
    const int32_t l = win ? win->offset_lft : 0, r = win ? win->offset_rgt : 0, a = win ? win->offset_abv : 0, b = win ? win->offset_blw : 0;
    *x0 = 2 * l; *y0 = 2 * a; *W = w - 2 * (l + r); *H = h - 2 * (a + b);
    return *W > 0 && *H > 0;
}

static inline int
ovhip_ranges_overlap_(const void *a, size_t na, const void *b, size_t nb)
{
    return (uintptr_t)a < (uintptr_t)b + nb && (uintptr_t)b < (uintptr_t)a + na;
}

static inline const char *
ovhip_out_why_planes_(const ovhip_pic *pic)
{
    return !pic->y || !pic->cb || !pic->cr ? "missing plane" : NULL;
}

static inline const char *
ovhip_out_why_strides_(const ovhip_pic *pic)
{
    return pic->stride_y < pic->w || pic->stride_c < pic->w / 2 ? "stride below the width" : NULL;
}

static inline const char *
ovhip_out_why_small_(size_t dst_bytes, size_t bytes)
{
    return dst_bytes < bytes ? "destination too small" : NULL;
}

/* es: the bytes of an element, a power of two */
static inline const char *
ovhip_out_why_unaligned_(const void *dst, int32_t es)
{
    return (uintptr_t)dst & (uintptr_t)(es - 1) ? "destination not aligned to its element" : NULL;
}

/* the `bytes` at dst against the samples of the picture's three planes (sizes and strides checked before) */
static inline const char *
ovhip_out_why_overlap_(const ovhip_pic *pic, const void *dst, size_t bytes)
{
    const size_t ny = ((size_t)(pic->h - 1) * (size_t)pic->stride_y + (size_t)pic->w) * 2;
    const size_t nc = ((size_t)(pic->h / 2 - 1) * (size_t)pic->stride_c + (size_t)(pic->w / 2)) * 2;
    return ovhip_ranges_overlap_(dst, bytes, pic->y, ny) || ovhip_ranges_overlap_(dst, bytes, pic->cb, nc) || ovhip_ranges_overlap_(dst, bytes, pic->cr, nc)
           ? "destination overlaps the picture" : NULL;
}

/* inside a plan: leave with OVHIP_EINVAL and the reason in *why when the check `q` names one */
#define OVHIP_OUT_REFUSE_(q) do { if ((*why = (q)) != NULL) return OVHIP_EINVAL; } while (0)
#endif
