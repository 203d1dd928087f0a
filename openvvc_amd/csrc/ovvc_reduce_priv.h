/* ovvc_reduce_priv.h -- what the host twin (ovvc_reduce.c) and the launcher (kernels_reduce.hip) of the reduced-size output share: the
 * plan, the refusals, and the three pieces of arithmetic both sides must agree on to the bit -- a footprint's samples, a sample's weight
 * and the kernel's division.  Definition: include/ovvc_hip.h, "Reduced-size output on the device".  Plain C that hipcc also compiles
 * for the device. */
#ifndef OVVC_REDUCE_PRIV_H
#define OVVC_REDUCE_PRIV_H
#include "ovvc_hip.h"
#ifdef __HIPCC__
#define OVHIP_HD_ __host__ __device__ static __forceinline__
#else
#define OVHIP_HD_ static inline
#endif

#define OVHIP_REDUCE_MAX_DIM   16384
#define OVHIP_REDUCE_MAX_RATIO 8
#define OVHIP_REDUCE_MAX_P     256
#define OVHIP_REDUCE_MAX_TAPS  (OVHIP_REDUCE_MAX_RATIO + 1)      /* samples under one footprint: ceil(p / q) + 1 */

typedef struct ovhip_reduce_plan_ {
    int32_t x0, y0, Ws, Hs;            /* the region reduced, in luma samples of the source */
    int32_t Wd, Hd;
    int32_t px, qx, py, qy;            /* S / gcd, D / gcd per axis: the chroma planes' are the same */
    int32_t sgx, sgy;                  /* sigma of the chroma planes (luma: 0) */
    uint32_t n;                        /* 16 px py */
} ovhip_reduce_plan_;

#ifdef __cplusplus
extern "C" {
#endif
/* everything ovhip_output_reduce_check refuses; px, qx, py, qy are written (0 where they cannot be derived) whatever the answer.
 * why: the reason of a refusal, at most why_len bytes. */
__attribute__((visibility("hidden"))) int ovhip_reduce_plan_make_(int32_t src_w, int32_t src_h, const ovhip_reduce_info *info, int32_t dst_w, int32_t dst_h,
                                                                   ovhip_reduce_plan_ *plan, char *why, size_t why_len);
/* what the two pictures themselves can have wrong (only looked at: host or device pointers): NULL, or the reason */
__attribute__((visibility("hidden"))) const char *ovhip_reduce_why_pics_(const ovhip_pic *src, const ovhip_pic *dst);
/* the launcher's refusals under the name `who`, the reason in the context's error text (kernels_reduce.hip): ovhip_post_pic_ asks before
 * it allocates */
__attribute__((visibility("hidden"))) int ovhip_reduce_refusal_(ovhip_ctx *ctx, const char *who, const ovhip_pic *src, const ovhip_reduce_info *info, int32_t dst_w, int32_t dst_h);
#ifdef __cplusplus
}
#endif

OVHIP_HD_ int32_t ovhip_reduce_floordiv_(int32_t a, int32_t b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }
OVHIP_HD_ int32_t ovhip_reduce_clamp_(int32_t v, int32_t lo, int32_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

/* first and last sample (of the n of the region, clamped to it) under output k's footprint [4pk - sg, 4p(k+1) - sg) */
OVHIP_HD_ int32_t ovhip_reduce_first_(int32_t k, int32_t p, int32_t q, int32_t sg, int32_t n)
{
    return ovhip_reduce_clamp_(ovhip_reduce_floordiv_(4 * p * k - sg, 4 * q), 0, n - 1);
}
OVHIP_HD_ int32_t ovhip_reduce_last_(int32_t k, int32_t p, int32_t q, int32_t sg, int32_t n)
{
    return ovhip_reduce_clamp_(ovhip_reduce_floordiv_(4 * p * (k + 1) - sg - 1, 4 * q), 0, n - 1);
}

/* the weight of sample j (0 .. n-1) in output k.  Sample j occupies [4qj, 4q(j+1)); the region's first and last sample stand for every
 * sample beyond them, so their intervals reach to the footprint's own ends: the clamped samples' weights collapse onto them. */
OVHIP_HD_ int32_t ovhip_reduce_weight_(int32_t k, int32_t j, int32_t p, int32_t q, int32_t sg, int32_t n)
{
    const int32_t A = 4 * p * k - sg, B = A + 4 * p;
    const int32_t lo = j == 0 ? A : 4 * q * j, hi = j == n - 1 ? B : 4 * q * (j + 1);
    const int32_t a = A > lo ? A : lo, b = B < hi ? B : hi;
    return b > a ? b - a : 0;
}

/* num / n as the kernel divides: num < 2^31, n <= 2^20, a quotient below 2^11, rcp = 1.0f / (float)n.  The estimate's relative error
 * is below 2^-22, so it is off by one at most, either way: one correction step from the remainder makes it exact. */
OVHIP_HD_ uint32_t ovhip_reduce_div_(uint32_t num, uint32_t n, float rcp)
{
    uint32_t qe = (uint32_t)((float)num * rcp);
    const int32_t r = (int32_t)(num - qe * n);
    if (r < 0) --qe;
    else if ((uint32_t)r >= n) ++qe;
    return qe;
}
#endif
