/* ovvc_dpb_priv.h -- library-internal links between the DPB state machine (ovvc_dpb.c), its HIP back-end (ovvc_dpb_hip.hip),
 * the frame and stream drivers (ovvc_frame.c, ovvc_stream.c) and the output path's .hip files. */
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
#define OVHIP_HIDDEN_ __attribute__((visibility("hidden")))
/* ---- the post-process step of the output path (kernels_output.hip): what happens to a finished picture on its way out.  One kind at
 * a time: the reference resamples the UNgrained frame over the grained one, so there is no parity to offer for both. */
enum { OVHIP_POST_NONE = 0, OVHIP_POST_SCALE, OVHIP_POST_GRAIN, OVHIP_POST_REDUCE };
typedef struct ovhip_post_ {
    int kind;
    int32_t out_w, out_h; ovhip_scale_info info;       /* SCALE: the output size and the scaling window / chroma collocation */
    const ovhip_fg_model *model; int32_t poc;          /* GRAIN: an already derived model (ovhip_fg_derive) and the picture's POC */
    ovhip_reduce_info rinfo;                           /* REDUCE: out_w x out_h as SCALE's; the source window / chroma location */
} ovhip_post_;
/* the size the outputs read under `post` of a w x h picture: SCALE and REDUCE leave post->out_w x out_h, grain leaves the picture's */
static inline void
ovhip_post_size_(const ovhip_post_ *post, int32_t w, int32_t h, int32_t *sw, int32_t *sh)
{
    const int resized = post->kind == OVHIP_POST_SCALE || post->kind == OVHIP_POST_REDUCE;
    *sw = resized ? post->out_w : w; *sh = resized ? post->out_h : h;
}
/* *shown = the picture the output shows.  NONE: *pic itself, nothing launched, nothing allocated.  Otherwise the refusals of the kind's
 * launcher come first (same codes, reasons in the context's error text), then `pic` is resampled / grained / reduced into the context's
 * grow-only scratch picture, asynchronously on the context's stream, and that is handed out: it stays valid until the context's next
 * post-processed output.  `pic` is only read. */
int  ovhip_post_pic_(ovhip_ctx *ctx, const ovhip_pic *pic, const ovhip_post_ *post, ovhip_pic *shown);
/* the delivery out->mode names, of a picture already shown: DIGEST -> ovhip_pic_digest (into out->digest: why `out` is not const),
 * PLANES -> ovhip_pic_download, PACKED -> ovhip_pic_output; any other mode is OVHIP_EINVAL.  out->window applies to the picture shown. */
OVHIP_HIDDEN_ int ovhip_deliver_(ovhip_ctx *ctx, const ovhip_pic *shown, ovhip_frame_output *out);
/* ovhip_post_pic_, then ovhip_deliver_ of the picture it shows; a mode that is none of the three is refused before anything is launched */
int  ovhip_post_deliver_(ovhip_ctx *ctx, const ovhip_pic *pic, const ovhip_post_ *post, ovhip_frame_output *out);
/* the wait for everything enqueued on the context's stream (the frame thread, behind an output's launch: complete on the device at
 * return); `what` names the output in the error text */
OVHIP_HIDDEN_ int ovhip_wait_(ovhip_ctx *ctx, const char *what);
/* the launchers' own refusals (kernels_scale.hip, kernels_grain.hip; kernels_reduce.hip's ovhip_reduce_refusal_ is in
 * ovvc_reduce_priv.h) under the name `who`: ovhip_post_pic_ asks before it allocates */
OVHIP_HIDDEN_ int ovhip_scale_refusal_(ovhip_ctx *ctx, const char *who, const ovhip_pic *src, const ovhip_scale_info *info, int32_t dst_w, int32_t dst_h);
OVHIP_HIDDEN_ int ovhip_grain_refusal_(ovhip_ctx *ctx, const char *who, const ovhip_pic *pic, const ovhip_fg_model *model);
/* ---- RGB output (ovvc_rgb.c, kernels_rgb.hip): what the host twin and the launcher share -- the refusals and everything a loop or a
 * kernel needs beside the planes.  `pic` is only looked at (plane pointers for null and overlap, sizes, strides), so it may hold host
 * pointers.  *why (may be NULL): the reason of a refusal, a string literal. */
typedef struct ovhip_rgb_plan_ {
    int32_t x0, y0, W, H;              /* first luma sample of the window in the picture, output size */
    int32_t a, b;                      /* chroma location: U = 2x - a, V = 2y - b */
    int32_t coef[5], yoff, peak;       /* cy, rv, gu, gv, bu */
    int32_t es;                        /* bytes per element */
    size_t bytes;
} ovhip_rgb_plan_;
OVHIP_HIDDEN_ int ovhip_rgb_plan_make_(const ovhip_pic *pic, const ovhip_window *win, const ovhip_rgb_format *fmt, const void *dst, size_t dst_bytes,
                                       ovhip_rgb_plan_ *plan, const char **why);
/* ---- Surface output (ovvc_surface.c, kernels_surface.hip): what the host twin and the launcher share, as the RGB plan above.  Plane
 * 0 is luma; a semi-planar format has ONE chroma plane (1: Cb and Cr interleaved), a planar one two (1: Cb, 2: Cr). */
typedef struct ovhip_surface_plan_ {
    int32_t x0, y0, W, H;              /* first luma sample of the window in the picture, output size */
    int32_t es, n_planes, semi, dither;/* bytes per element; 2 or 3; interleaved chroma; OVHIP_SURF_DITHER */
    int32_t shift;                     /* P010: 6, else 0 */
    int32_t elems[3], rows[3];         /* elements of a row and rows, per plane */
    size_t pitch[3], off[3];           /* bytes from row to row, byte offset from the base */
    size_t bytes;                      /* the surface's size: the largest end of a plane's last row's own bytes */
} ovhip_surface_plan_;
/* the refusals that need no picture, no size and no destination: enum values, rsv, rounding, offset_c[1], pitch and offset multiples */
OVHIP_HIDDEN_ int ovhip_surface_format_check_(const ovhip_surface_format *fmt, const char **why);
/* on a refusal for "destination too small" plan->bytes holds the size needed */
OVHIP_HIDDEN_ int ovhip_surface_plan_make_(const ovhip_pic *pic, const ovhip_window *win, const ovhip_surface_format *fmt, const void *dst, size_t dst_bytes,
                                           ovhip_surface_plan_ *plan, const char **why);
/* ---- Motion field output (ovvc_mvfield.c, kernels_mvfield.hip; what they share: ovvc_mvfield_priv.h).  ovhip_job_mvfield and the
 * wait for it: complete on the device at return (the frame thread; ovvc_picture.hip) */
int  ovhip_job_mvfield_done_(ovhip_job *job, const ovhip_mvfield_format *fmt, void *d_vec, size_t vec_bytes, void *d_info, size_t info_bytes);
#ifdef __cplusplus
}
#endif
#endif
