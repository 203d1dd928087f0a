/* Surface output through a colour table, on the host: the plan and the refusals the launcher shares, the forward coefficients, and the
 * definition over planes and a table in host memory.  Definition: include/ovvc_hip.h, "Surface output through a colour table"; the
 * device half is kernels_surface_lut.hip.  It stands on the twins of its parts: ovhip_rgb_lut_host gives the table's output for every
 * luma position of the window, ovhip_surface_host stores the converted picture.  Plain C, no HIP calls. */
#include <stdlib.h>
#include <string.h>
#include "ovvc_hip.h"
#include "ovvc_surface_lut_priv.h"
#include "ovvc_outdst_priv.h"

/* round(p / q) for p, q > 0 (no coefficient is a tie: tests/spec_surface_lut.py asserts it on the exact rationals) */
static int32_t rnd_div(uint64_t p, uint64_t q) { return (int32_t)((2 * p + q) / (2 * q)); }

int
ovhip_surface_conv_check_(const ovhip_surface_conv *conv, const char **why)
{
    const char *dummy;
    if (!why) why = &dummy;
    *why = "null conversion";
    if (!conv) return OVHIP_EINVAL;
    if (conv->rsv[0] || conv->rsv[1]) { *why = "conv rsv must be 0"; return OVHIP_EINVAL; }
    if (conv->src_full_range > 1 || conv->dst_full_range > 1) { *why = "bad range"; return OVHIP_EINVAL; }
    if (conv->src_chroma_loc > 5 || conv->dst_chroma_loc > 5) { *why = "bad chroma location"; return OVHIP_EINVAL; }
    const uint8_t m[2] = { conv->src_matrix, conv->dst_matrix };
    for (int k = 0; k < 2; ++k) {
        if (m[k] == 2) { *why = k ? "destination matrix coefficients unspecified" : "matrix coefficients unspecified"; return OVHIP_EINVAL; }
        if (m[k] != 1 && m[k] != 5 && m[k] != 6 && m[k] != 9) { *why = k ? "destination matrix coefficients not built" : "matrix coefficients not built"; return OVHIP_EUNSUP; }
    }
    if (conv->dst_chroma_loc > 3) { *why = "destination chroma locations 4 and 5 not built"; return OVHIP_EUNSUP; }
    *why = "";
    return OVHIP_OK;
}

int
ovhip_surface_lut_coefs(const ovhip_surface_conv *conv, int32_t coef[9], int32_t *yoff)
{
    if (!conv || !coef || !yoff || conv->dst_full_range > 1) return OVHIP_EINVAL;
    uint64_t kr, kb;                                       /* in 1 / 10000 */
    switch (conv->dst_matrix) {
    case 1: kr = 2126; kb = 722; break;
    case 5: case 6: kr = 2990; kb = 1140; break;
    case 9: kr = 2627; kb = 593; break;
    case 2: return OVHIP_EINVAL;                           /* unspecified: the caller must decide */
    default: return OVHIP_EUNSUP;
    }
    const uint64_t one = 10000, kg = one - kr - kb;
    const uint64_t ny = conv->dst_full_range ? 1023 : 876, nc = conv->dst_full_range ? 1023 : 896, d = 1023;
    const uint64_t s = (uint64_t)1 << 14;
    const int32_t T = rnd_div(s * ny, d);
    coef[0] = rnd_div(s * ny * kr, d * one);                                    /* y_r = sy Kr                     */
    coef[2] = rnd_div(s * ny * kb, d * one);                                    /* y_b = sy Kb                     */
    coef[1] = T - coef[0] - coef[2];                                            /* the row sums to rnd(sy)         */
    coef[3] = -rnd_div(s * nc * kr, d * 2 * (one - kb));                        /* b_r = -sc Kr / (2 (1 - Kb))     */
    coef[4] = -rnd_div(s * nc * kg, d * 2 * (one - kb));                        /* b_g = -sc Kg / (2 (1 - Kb))     */
    coef[5] = -coef[3] - coef[4];                                               /* both chroma rows sum to 0       */
    coef[7] = -rnd_div(s * nc * kg, d * 2 * (one - kr));                        /* r_g = -sc Kg / (2 (1 - Kr))     */
    coef[8] = -rnd_div(s * nc * kb, d * 2 * (one - kr));                        /* r_b = -sc Kb / (2 (1 - Kr))     */
    coef[6] = -coef[7] - coef[8];
    *yoff = conv->dst_full_range ? 0 : 64;
    return OVHIP_OK;
}

int
ovhip_surface_lut_check(const ovhip_surface_conv *conv, const ovhip_surface_format *fmt, int size, int peak)
{
    int r = ovhip_surface_conv_check_(conv, NULL);
    if (r == OVHIP_OK) r = ovhip_surface_format_check_(fmt, NULL);
    if (r == OVHIP_OK) r = ovhip_rgb_lut_check(size, peak, NULL);
    return r;
}

int
ovhip_surface_lut_plan_make_(const ovhip_pic *pic, const ovhip_window *win, const ovhip_surface_conv *conv, const ovhip_surface_format *fmt,
                             int size, int peak, int have_table, const void *dst, size_t dst_bytes, ovhip_surface_lut_plan_ *plan, const char **why)
{
    const char *dummy;
    if (!why) why = &dummy;
    *why = "null argument";
    if (!plan) return OVHIP_EINVAL;
    memset(plan, 0, sizeof(*plan));
    if (!pic) return OVHIP_EINVAL;
    if (!fmt) { *why = "null format"; return OVHIP_EINVAL; }
    int r = ovhip_surface_conv_check_(conv, why);
    if (r != OVHIP_OK) return r;
    r = ovhip_surface_plan_make_(pic, win, fmt, dst, dst_bytes, &plan->surf, why);
    if (r != OVHIP_OK) return r;
    /* the RGB side, asked here and not through ovhip_rgb_lut_plan_make_: that plan checks a destination of 3 W H elements, and this
     * output has no RGB destination -- the only range that must not overlap the picture is the surface's, checked above.  What is left
     * of its refusals: the picture's sizes (multiples of 4: stricter than the surface's "even") and the table; the planes, the strides
     * and the window are the surface plan's, the source matrix, range and location the conversion's */
    const size_t bytes = plan->surf.bytes;
    plan->surf.bytes = 0;                                                       /* (after a refusal that is not "too small") */
    if ((pic->w & 3) || (pic->h & 3)) { *why = "sizes must be positive multiples of 4"; return OVHIP_EINVAL; }
    if (!have_table) { *why = "null table"; return OVHIP_EINVAL; }
    if (ovhip_rgb_lut_check(size, peak, NULL) != OVHIP_OK) { *why = "table size must be 17, 33 or 65 and its peak 1..65535"; return OVHIP_EINVAL; }
    const ovhip_rgb_format rf = { conv->src_matrix, conv->src_full_range, conv->src_chroma_loc, OVHIP_RGB_U16, OVHIP_RGB_PLANAR, { 0, 0, 0 } };
    (void)ovhip_rgb_coefs(&rf, plan->rgb.coef, &plan->rgb.yoff);               /* at N = 10; (conv passed its own refusals above) */
    plan->rgb.x0 = plan->surf.x0; plan->rgb.y0 = plan->surf.y0; plan->rgb.W = plan->surf.W; plan->rgb.H = plan->surf.H;
    plan->rgb.a = conv->src_chroma_loc & 1;
    plan->rgb.b = conv->src_chroma_loc < 2 ? 1 : (conv->src_chroma_loc < 4 ? 0 : 2);
    plan->rgb.peak = 1023; plan->rgb.es = 2;
    plan->surf.bytes = bytes;
    (void)ovhip_surface_lut_coefs(conv, plan->coef, &plan->yoff);              /* (conv passed its own refusals above) */
    plan->hc = !(conv->dst_chroma_loc & 1);
    plan->vt = conv->dst_chroma_loc >= 2;
    *why = "";
    return OVHIP_OK;
}

static inline int32_t clampi(int32_t v, int32_t lo, int32_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

int
ovhip_surface_lut_host(const uint16_t *y, const uint16_t *cb, const uint16_t *cr, int32_t w, int32_t h, int32_t stride_y, int32_t stride_c,
                       const ovhip_window *win, const ovhip_surface_conv *conv, const ovhip_surface_format *fmt, int size, int peak,
                       const uint16_t *host_table, void *dst, size_t dst_bytes)
{
    const ovhip_pic pic = { (uint16_t *)y, (uint16_t *)cb, (uint16_t *)cr, w, h, stride_y, stride_c };
    ovhip_surface_lut_plan_ p;
    int r = ovhip_surface_lut_plan_make_(&pic, win, conv, fmt, size, peak, host_table != NULL, dst, dst_bytes, &p, NULL);
    if (r != OVHIP_OK) return r;
    if (ovhip_rgb_lut_first_above_(size, peak, host_table) >= 0) return OVHIP_EINVAL;
    const int32_t W = p.surf.W, H = p.surf.H, CW = W / 2, CH = H / 2;
    const size_t plane = (size_t)W * (size_t)H, cplane = (size_t)CW * (size_t)CH;
    /* o: the table's output at every luma position of the window (3 planes); c14: Cb14 and Cr14 there; conv_pic: the converted picture */
    uint16_t *o = (uint16_t *)malloc(3 * plane * sizeof(*o));
    int32_t *c14 = (int32_t *)malloc(2 * plane * sizeof(*c14));
    uint16_t *conv_pic = (uint16_t *)malloc((plane + 2 * cplane) * sizeof(*conv_pic));
    if (!o || !c14 || !conv_pic) { free(o); free(c14); free(conv_pic); return OVHIP_ENOMEM; }
    const ovhip_rgb_format rf = { conv->src_matrix, conv->src_full_range, conv->src_chroma_loc, OVHIP_RGB_U16, OVHIP_RGB_PLANAR, { 0, 0, 0 } };
    r = ovhip_rgb_lut_host(y, cb, cr, w, h, stride_y, stride_c, win, &rf, size, peak, host_table, o, 3 * plane * sizeof(*o));
    if (r == OVHIP_OK) {
        uint16_t *yc = conv_pic, *cbc = conv_pic + plane, *crc = cbc + cplane;
        const float rcp = 1.0f / (float)peak;
        /* parts 3 to 5: normalise, forward matrix, the luma plane */
        for (size_t i = 0; i < plane; ++i) {
            const int32_t qr = ovhip_surface_lut_norm_(o[i], (uint32_t)peak, rcp), qg = ovhip_surface_lut_norm_(o[plane + i], (uint32_t)peak, rcp),
                          qb = ovhip_surface_lut_norm_(o[2 * plane + i], (uint32_t)peak, rcp);
            const int32_t y14 = 16 * p.yoff + ovhip_surface_lut_row_(p.coef, qr, qg, qb);
            c14[i] = 8192 + ovhip_surface_lut_row_(p.coef + 3, qr, qg, qb);
            c14[plane + i] = 8192 + ovhip_surface_lut_row_(p.coef + 6, qr, qg, qb);
            yc[i] = (uint16_t)clampi((y14 + 8) >> 4, 0, 1023);
        }
        /* part 6: the chroma planes; taps clamped to the window */
        static const int32_t w121[3] = { 1, 2, 1 }, w022[3] = { 0, 2, 2 };      /* taps at 2i - 1, 2i, 2i + 1 */
        const int32_t *wx = p.hc ? w121 : w022, *wy = p.vt ? w121 : w022;
        for (int32_t j = 0; j < CH; ++j)
            for (int32_t i = 0; i < CW; ++i) {
                int32_t sb = 128, sr = 128;
                for (int ty = 0; ty < 3; ++ty)
                    for (int tx = 0; tx < 3; ++tx) {
                        const size_t at = (size_t)clampi(2 * j - 1 + ty, 0, H - 1) * (size_t)W + (size_t)clampi(2 * i - 1 + tx, 0, W - 1);
                        sb += wx[tx] * wy[ty] * c14[at];
                        sr += wx[tx] * wy[ty] * c14[plane + at];
                    }
                cbc[(size_t)j * CW + i] = (uint16_t)clampi(sb >> 8, 0, 1023);
                crc[(size_t)j * CW + i] = (uint16_t)clampi(sr >> 8, 0, 1023);
            }
        /* part 7: the surface of the converted picture */
        r = ovhip_surface_host(yc, cbc, crc, W, H, W, CW, NULL, fmt, dst, dst_bytes);
    }
    free(o); free(c14); free(conv_pic);
    return r;
}
