/* ovvc_ladder_priv.h -- what the host twin (ovvc_ladder.c) and the launcher (kernels_ladder.hip) of the output ladder share: the plan --
 * per rung the reduce plan and the surface plan of the two definitions it composes -- and the refusals.  Definition:
 * include/ovvc_hip.h, "Output ladder on the device".  Plain C. */
#ifndef OVVC_LADDER_PRIV_H
#define OVVC_LADDER_PRIV_H
#include "ovvc_hip.h"
#include "ovvc_dpb_priv.h"
#include "ovvc_reduce_priv.h"

typedef struct ovhip_ladder_plan_ {
    int32_t n;
    ovhip_reduce_plan_ red[OVHIP_LADDER_MAX_RUNGS];      /* the same region in every rung */
    ovhip_surface_plan_ surf[OVHIP_LADDER_MAX_RUNGS];    /* of the rung's out_w x out_h picture, no window */
} ovhip_ladder_plan_;

#ifdef __cplusplus
extern "C" {
#endif
/* Everything a ladder can be refused for.  src: only looked at (host or device pointers); NULL: the checks that need no picture and
 * no destination only (ovhip_ladder_check), against src_w x src_h.  why: the reason of a refusal, led by the rung's index where it
 * is a rung's, at most why_len bytes. */
__attribute__((visibility("hidden"))) int ovhip_ladder_plan_make_(const ovhip_pic *src, int32_t src_w, int32_t src_h, const ovhip_reduce_info *info,
                                                                   const ovhip_ladder_rung *rungs, int32_t n, ovhip_ladder_plan_ *plan, char *why, size_t why_len);
#ifdef __cplusplus
}
#endif
#endif
