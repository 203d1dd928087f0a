/* ovvc_outdst_priv.h -- what the host twins of the picture outputs that write a caller's destination share (ovvc_rgb.c, ovvc_surface.c):
 * the cropping window's geometry and the checks of a picture and a destination, one at a time.  A check answers with the reason of its
 * refusal (a string literal, what the plans hand out as *why) or NULL; the ORDER in which a plan asks is the plan's own, since a
 * caller with two faults at once is told the first.  Plain C, no HIP calls; `pic` is only looked at, so it may hold host pointers.
 * Behind the checks: what the two RGB twins (ovvc_rgb.c, ovvc_rgb_lut.c) compute alike -- a pixel's blend, matrix and clip, and the
 * stored element of each dtype. */
#ifndef OVVC_OUTDST_PRIV_H
#define OVVC_OUTDST_PRIV_H
#include <string.h>
#include "ovvc_hip.h"
#include "ovvc_dpb_priv.h"

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

/* The staging plan of an output that leaves as n host destinations through one device scratch (the ladder's rungs, the pyramid's levels):
 * item k has the host destination dst[k] of given[k] bytes and needs need[k] of them.  The items are asked in order, each first for
 * itself, then against the items before it.  OVHIP_STAGE_OK_: off[k] is item k's place in the scratch, on a 256-byte boundary, and
 * *total the scratch's size.  OVHIP_STAGE_UNFIT_: item *k has no destination, needs nothing (its size was refused) or was given too
 * little.  OVHIP_STAGE_OVERLAP_: the need[*k] bytes of item *k overlap the need[*j] bytes of the earlier item *j.  Nothing is read
 * through the pointers */
enum { OVHIP_STAGE_OK_ = 0, OVHIP_STAGE_UNFIT_, OVHIP_STAGE_OVERLAP_ };
static inline int
ovhip_stage_plan_(int n, void *const *dst, const size_t *given, const size_t *need, size_t *off, size_t *total, int *k, int *j)
{
    *total = 0;
    for (*k = 0; *k < n; ++*k) {
        if (!dst[*k] || !need[*k] || given[*k] < need[*k]) return OVHIP_STAGE_UNFIT_;
        off[*k] = *total;
        *total += (need[*k] + 255) & ~(size_t)255;
        for (*j = 0; *j < *k; ++*j)
            if (ovhip_ranges_overlap_(dst[*k], need[*k], dst[*j], need[*j])) return OVHIP_STAGE_OVERLAP_;
    }
    return OVHIP_STAGE_OK_;
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

static inline int32_t ovhip_clampi_(int32_t v, int32_t lo, int32_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

/* the pixel (px, py) of the picture under an RGB plan (include/ovvc_hip.h, "RGB output on the device"): chroma blended bilinearly at the
 * plan's sample location, the matrix, the clip to 0..peak (the plan's own, or 1023 in front of a colour table) */
static inline void
ovhip_rgb_pixel_(const ovhip_pic *pic, const ovhip_rgb_plan_ *p, int32_t px, int32_t py, int32_t peak, int32_t rgb[3])
{
    const int32_t cw = pic->w / 2, ch = pic->h / 2;
    const int32_t V = 2 * py - p->b, fy = V & 3, U = 2 * px - p->a, fx = U & 3;
    const int32_t j0 = ovhip_clampi_(V >> 2, 0, ch - 1), j1 = ovhip_clampi_((V >> 2) + 1, 0, ch - 1);
    const int32_t i0 = ovhip_clampi_(U >> 2, 0, cw - 1), i1 = ovhip_clampi_((U >> 2) + 1, 0, cw - 1);
    const int32_t w00 = (4 - fx) * (4 - fy), w01 = fx * (4 - fy), w10 = (4 - fx) * fy, w11 = fx * fy;
    const size_t a0 = (size_t)j0 * pic->stride_c, a1 = (size_t)j1 * pic->stride_c;
    const uint16_t *cb = pic->cb, *cr = pic->cr;
    const int32_t u = w00 * cb[a0 + i0] + w01 * cb[a0 + i1] + w10 * cb[a1 + i0] + w11 * cb[a1 + i1] - 8192;
    const int32_t v = w00 * cr[a0 + i0] + w01 * cr[a0 + i1] + w10 * cr[a1 + i0] + w11 * cr[a1 + i1] - 8192;
    const int32_t L = 16 * p->coef[0] * ((int32_t)pic->y[(size_t)py * pic->stride_y + px] - p->yoff) + (1 << 17);
    rgb[0] = ovhip_clampi_((L + p->coef[1] * v) >> 18, 0, peak);
    rgb[1] = ovhip_clampi_((L - p->coef[2] * u - p->coef[3] * v) >> 18, 0, peak);
    rgb[2] = ovhip_clampi_((L + p->coef[4] * u) >> 18, 0, peak);
}

/* float32 -> float16 bits, round to nearest even, for 0 <= f <= 1: normal and subnormal halves (a table peak above 16384 puts small
 * outputs below 2^-14) */
static inline uint16_t
ovhip_half_bits_(float f)
{
    uint32_t u;
    memcpy(&u, &f, 4);
    const int32_t e = (int32_t)(u >> 23) - 127;                /* (f >= 0: no sign) */
    if (e >= -14) {                                            /* a normal half, unless the rounding carries it to the next exponent: the sum does that too */
        u += 0xFFF + ((u >> 13) & 1);
        return (uint16_t)((u >> 13) - ((127 - 15) << 10));
    }
    if (e < -25) return 0;                                     /* below half of the smallest subnormal (2^-25 itself is the tie, to even: 0; above it: see below) */
    /* subnormal: the value in units of 2^-24 is m * 2^(e - 23 + 24) with m the 24-bit significand; shift right by s = -(e + 1) in 14..24 */
    const uint32_t m = (u & 0x7FFFFF) | 0x800000;
    const int s = -(e + 1);
    const uint32_t q = m >> s, rem = m & ((1u << s) - 1), half = 1u << (s - 1);
    return (uint16_t)(q + (rem > half || (rem == half && (q & 1))));
}

/* element e of an RGB destination of `dtype`: the value o of 0..P, to_unit = (float)(1.0 / P) */
static inline void
ovhip_rgb_put_(void *dst, size_t e, uint32_t dtype, int32_t o, float to_unit)
{
    const float f = (float)o * to_unit;
    switch (dtype) {
    case OVHIP_RGB_U8:  ((uint8_t *)dst)[e] = (uint8_t)o; break;
    case OVHIP_RGB_U16: ((uint16_t *)dst)[e] = (uint16_t)o; break;
    case OVHIP_RGB_F16: ((uint16_t *)dst)[e] = ovhip_half_bits_(f); break;
    default:            ((float *)dst)[e] = f; break;
    }
}
#endif
