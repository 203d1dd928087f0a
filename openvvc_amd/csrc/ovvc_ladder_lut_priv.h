/* ovvc_ladder_lut_priv.h -- what the host twin (ovvc_ladder_lut.c) and the launcher (kernels_ladder_lut.hip) of the output ladder through
 * a colour table share: the plan -- the ladder's plan and, per rung, the plan of the surface output through a table of the rung's
 * reduced picture -- and the refusals.  Definition: include/ovvc_hip.h, "Output ladder through a colour table".  Plain C. */
#ifndef OVVC_LADDER_LUT_PRIV_H
#define OVVC_LADDER_LUT_PRIV_H
#include "ovvc_hip.h"
#include "ovvc_ladder_priv.h"
#include "ovvc_surface_lut_priv.h"

typedef struct ovhip_ladder_lut_plan_ {
    ovhip_ladder_plan_ lad;                              /* the rungs' reduce plans (and, with a picture, their surface plans) */
    ovhip_surface_lut_plan_ sl[OVHIP_LADDER_MAX_RUNGS];  /* with a picture: of the rung's out_w x out_h picture, no window.  The source and
                                                          * the forward side (rgb.coef, rgb.a, rgb.b, coef, yoff, hc, vt) are the same in all */
} ovhip_ladder_lut_plan_;

#ifdef __cplusplus
extern "C" {
#endif
/* Everything a ladder through a table can be refused for but the table's device, in this order: what ovhip_ladder_plan_make_ refuses
 * (src, src_w, src_h as there: src NULL asks the picture-independent part only); the conversion's own refusals; a chroma location of
 * the conversion's source that is not info's; per rung what ovhip_surface_lut_plan_make_ refuses of the rung's picture, format and
 * destination, and of the table.  why (not NULL): the reason, led by the rung's index where it is a rung's, at most why_len bytes. */
OVHIP_HIDDEN_ int ovhip_ladder_lut_plan_make_(const ovhip_pic *src, int32_t src_w, int32_t src_h, const ovhip_reduce_info *info, const ovhip_ladder_rung *rungs,
                                              int32_t n, const ovhip_surface_conv *conv, int size, int peak, int have_table, ovhip_ladder_lut_plan_ *plan,
                                              char *why, size_t why_len);
#ifdef __cplusplus
}
#endif
#endif
