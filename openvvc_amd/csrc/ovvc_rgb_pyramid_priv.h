/* ovvc_rgb_pyramid_priv.h -- what the host twin (ovvc_rgb_pyramid.c) and the launcher (kernels_rgb_pyramid.hip) of the RGB pyramid share:
 * the plan -- per level the reduce plan and the RGB plan of the two definitions it composes -- and the refusals.  Definition:
 * include/ovvc_hip.h, "RGB pyramid on the device".  Plain C. */
#ifndef OVVC_RGB_PYRAMID_PRIV_H
#define OVVC_RGB_PYRAMID_PRIV_H
#include "ovvc_hip.h"
#include "ovvc_dpb_priv.h"
#include "ovvc_reduce_priv.h"
#include "ovvc_rgb_lut_priv.h"

typedef struct ovhip_rgb_pyramid_plan_ {
    int32_t n;
    ovhip_reduce_plan_ red[OVHIP_PYRAMID_MAX_LEVELS];    /* the same region in every level */
    ovhip_rgb_plan_ rgb[OVHIP_PYRAMID_MAX_LEVELS];       /* with a picture: of the level's out_w x out_h picture, no window; a, b are the
                                                          * same in all, coef / yoff / peak go by the level's dtype (by the table: 10 bits) */
} ovhip_rgb_pyramid_plan_;

#ifdef __cplusplus
extern "C" {
#endif
/* Everything a pyramid can be refused for but the table's device, in this order: null info or levels, n out of range; with a picture
 * (src not NULL; only looked at: host or device pointers) a missing plane or a stride below the width; per level what
 * ovhip_reduce_plan_make_ refuses, against src's size or src_w x src_h (src NULL: the checks that need no picture and no destination
 * only); formats that disagree in matrix, range or location, or a location that is not info's; per level what ovhip_rgb_plan_make_ --
 * with_table: ovhip_rgb_lut_plan_make_ with size, peak and have_table -- refuses of the level's picture, format and destination; a
 * destination that overlaps the picture or an earlier level's.  why (not NULL): the reason, led by the level's index where it is a
 * level's, at most why_len bytes. */
OVHIP_HIDDEN_ int ovhip_rgb_pyramid_plan_make_(const ovhip_pic *src, int32_t src_w, int32_t src_h, const ovhip_reduce_info *info, const ovhip_rgb_level *levels,
                                               int32_t n, int with_table, int size, int peak, int have_table, ovhip_rgb_pyramid_plan_ *plan, char *why,
                                               size_t why_len);
#ifdef __cplusplus
}
#endif
#endif
