/* ovvc_surface_lut_priv.h -- surface output through a colour table (include/ovvc_hip.h, "Surface output through a colour table"): what
 * the host half (ovvc_surface_lut.c) and the device half (kernels_surface_lut.hip) share -- the plan with both sides' refusals, and
 * the two pieces of arithmetic they must agree on to the bit: the normalising division and the forward matrix.  Plain C that hipcc also
 * compiles for the device. */
#ifndef OVVC_SURFACE_LUT_PRIV_H
#define OVVC_SURFACE_LUT_PRIV_H
#include "ovvc_hip.h"
#include "ovvc_dpb_priv.h"
#include "ovvc_rgb_lut_priv.h"
#include "ovvc_reduce_priv.h"

typedef struct ovhip_surface_lut_plan_ {
    ovhip_surface_plan_ surf;          /* the destination: its window is the RGB side's */
    ovhip_rgb_plan_ rgb;               /* the source: matrix at N = 10, chroma location */
    int32_t coef[9], yoff;             /* the forward matrix: y_r y_g y_b, b_r b_g b_b, r_r r_g r_b; the destination's luma offset */
    int32_t hc, vt;                    /* destination chroma horizontally co-sited (taps 1 2 1, else 2 2) / vertically top (1 2 1, else 2 2) */
} ovhip_surface_lut_plan_;

#ifdef __cplusplus
extern "C" {
#endif
/* everything the launch refuses but the table's device: the conversion, then what the surface output refuses, then what the RGB output
 * through a table refuses of the picture and the table.  *why (may be NULL): a string literal.  On "destination too small"
 * plan->surf.bytes holds the size needed, else 0 after a refusal. */
OVHIP_HIDDEN_ int ovhip_surface_lut_plan_make_(const ovhip_pic *pic, const ovhip_window *win, const ovhip_surface_conv *conv, const ovhip_surface_format *fmt,
                                               int size, int peak, int have_table, const void *dst, size_t dst_bytes, ovhip_surface_lut_plan_ *plan,
                                               const char **why);
/* the refusals of a conversion alone; *why as above */
OVHIP_HIDDEN_ int ovhip_surface_conv_check_(const ovhip_surface_conv *conv, const char **why);
#ifdef __cplusplus
}
#endif

/* q = (16368 o + P / 2) / P for o <= P <= 65535, as the kernel divides: the numerator is below 2^31 and the quotient at most 16368, so
 * ovhip_reduce_div_'s estimate (relative error below 2^-22) is off by one at most and its correction step makes it exact.
 * rcp = 1.0f / (float)P */
OVHIP_HD_ int32_t ovhip_surface_lut_norm_(uint32_t o, uint32_t P, float rcp)
{
    return (int32_t)ovhip_reduce_div_(16368u * o + (P >> 1), P, rcp);
}

/* one row of the forward matrix on normalised values: (c . q + 2^13) >> 14, an arithmetic shift; |c . q| < 2^29 */
OVHIP_HD_ int32_t ovhip_surface_lut_row_(const int32_t *c, int32_t qr, int32_t qg, int32_t qb)
{
    return (c[0] * qr + c[1] * qg + c[2] * qb + (1 << 13)) >> 14;
}
#endif
