/* ovvc_dpb_priv.h -- library-internal links between the DPB state machine (ovvc_dpb.c), its HIP back-end (ovvc_dpb_hip.hip)
 * and the stream driver (ovvc_stream.c). */
#ifndef OVVC_DPB_PRIV_H
#define OVVC_DPB_PRIV_H
#include "ovvc_hip.h"
#ifdef __cplusplus
extern "C" {
#endif
int  ovhip_dpb_hip_ops_(const int *devices, int n_devices, ovhip_dpb_ops *ops, void **user);
void ovhip_dpb_hip_ops_free_(void *user);
void ovhip_dpb_rearm_(ovhip_dpb *d);
/* CLOCK_MONOTONIC seconds at which the frame's last picture was complete on the device / published (the stream driver's timeline) */
double ovhip_frame_published_at(const ovhip_frame *f);
double ovhip_frame_done_at(const ovhip_frame *f);
/* kernels_scale.hip: `pic` resampled to out_w x out_h in the context's scratch picture, which is handed out in *scaled (valid until the
 * context's next scaled output); asynchronous on the context's stream */
int  ovhip_scaled_scratch_(ovhip_ctx *ctx, const ovhip_pic *pic, const ovhip_scale_info *info, int32_t out_w, int32_t out_h, ovhip_pic *scaled);
/* kernels_scale.hip: that scratch picture at w x h, no launch; kernels_grain.hip: `pic` with film grain in it (valid until the context's
 * next scaled or grained output); asynchronous on the context's stream */
int  ovhip_scratch_pic_(ovhip_ctx *ctx, int32_t w, int32_t h, ovhip_pic *pic);
int  ovhip_grain_scratch_(ovhip_ctx *ctx, const ovhip_pic *pic, const ovhip_fg_model *model, int32_t poc, ovhip_pic *grained);
#ifdef __cplusplus
}
#endif
#endif
