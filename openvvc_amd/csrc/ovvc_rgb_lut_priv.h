/* ovvc_rgb_lut_priv.h -- RGB output through a colour table (include/ovvc_hip.h, "RGB output through a colour table"): what the host
 * half (ovvc_rgb_lut.c), the device half (kernels_rgb_lut.hip) and the frame and stream drivers share. */
#ifndef OVVC_RGB_LUT_PRIV_H
#define OVVC_RGB_LUT_PRIV_H
#include "ovvc_hip.h"
#include "ovvc_dpb_priv.h"
#ifdef __cplusplus
extern "C" {
#endif
/* the table on a device: size^3 texels of 8 bytes (R, G, B, 0), index (b * size + g) * size + r.  Immutable once created */
struct ovhip_rgb_lut {
    int device;                        /* the HIP device the texels live on */
    int32_t size, peak;
    void *d_texels;
};
/* the RGB plan of `fmt` with the coefficients and the clip of N = 10 whatever the dtype, behind the table's own refusals (size, peak, U8
 * with peak > 255, no table).  *why as ovhip_rgb_plan_make_ */
OVHIP_HIDDEN_ int ovhip_rgb_lut_plan_make_(const ovhip_pic *pic, const ovhip_window *win, const ovhip_rgb_format *fmt, int size, int peak, int have_table,
                                           const void *dst, size_t dst_bytes, ovhip_rgb_plan_ *plan, const char **why);
/* -1 when every one of the 3 size^3 entries is <= peak, else the index of the first that is not */
OVHIP_HIDDEN_ int64_t ovhip_rgb_lut_first_above_(int size, int peak, const uint16_t *table);
/* table[size][size][size][3] -> texels[size^3][4]: (R, G, B, 0) */
OVHIP_HIDDEN_ void ovhip_rgb_lut_repack_(int size, const uint16_t *table, uint16_t *texels);
/* 1: the table lives on the context's device */
OVHIP_HIDDEN_ int ovhip_rgb_lut_on_ctx_(const ovhip_rgb_lut *lut, const ovhip_ctx *ctx);
#ifdef __cplusplus
}
#endif
#endif
