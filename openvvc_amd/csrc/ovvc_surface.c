/* Surface output on the host: the layout and the refusals the launcher shares, the size of a surface, and the definition over planes in
 * host memory.  Definition: include/ovvc_hip.h, "Surface output on the device"; the device half is kernels_surface.hip.
 * Plain C, no HIP calls. */
#include <string.h>
#include "ovvc_hip.h"
#include "ovvc_dpb_priv.h"
#include "ovvc_outdst_priv.h"

#define SURF_MAX_SIZE 16384

static int is_16bit(int format) { return format == OVHIP_SURF_P010 || format == OVHIP_SURF_I010; }
static int is_semi(int format) { return format == OVHIP_SURF_NV12 || format == OVHIP_SURF_P010; }

int
ovhip_surface_format_check_(const ovhip_surface_format *fmt, const char **why)
{
    const char *dummy;
    if (!why) why = &dummy;
    *why = "null format";
    if (!fmt) return OVHIP_EINVAL;
    if (fmt->format > OVHIP_SURF_I010) { *why = "unknown format"; return OVHIP_EINVAL; }
    if (fmt->rounding > OVHIP_SURF_DITHER) { *why = "unknown rounding"; return OVHIP_EINVAL; }
    if (fmt->rounding && is_16bit(fmt->format)) { *why = "a 16-bit format takes rounding 0 only"; return OVHIP_EINVAL; }
    if (fmt->rsv[0] || fmt->rsv[1]) { *why = "rsv must be 0"; return OVHIP_EINVAL; }
    if (is_semi(fmt->format) && fmt->offset_c[1]) { *why = "offset_c[1] on a semi-planar format"; return OVHIP_EINVAL; }
    if (is_16bit(fmt->format) && ((fmt->pitch_y | fmt->pitch_c | fmt->offset_c[0] | fmt->offset_c[1]) & 1)) {
        *why = "pitch or offset not a multiple of the element size"; return OVHIP_EINVAL;
    }
    *why = "";
    return OVHIP_OK;
}

/* the window and the planes' places in the surface; everything ovhip_surface_bytes refuses is refused here */
static int
surface_layout(int32_t w, int32_t h, const ovhip_window *win, const ovhip_surface_format *fmt, ovhip_surface_plan_ *p, const char **why)
{
    memset(p, 0, sizeof(*p));
    const int r = ovhip_surface_format_check_(fmt, why);
    if (r != OVHIP_OK) return r;
    if (w <= 0 || h <= 0 || (w & 1) || (h & 1) || w > SURF_MAX_SIZE || h > SURF_MAX_SIZE) { *why = "sizes must be positive, even and at most 16384"; return OVHIP_EINVAL; }
    if (!ovhip_out_window_(w, h, win, &p->x0, &p->y0, &p->W, &p->H)) { *why = "the window leaves nothing"; return OVHIP_EINVAL; }
    p->es = is_16bit(fmt->format) ? 2 : 1;
    p->semi = is_semi(fmt->format);
    p->n_planes = p->semi ? 2 : 3;
    p->dither = fmt->rounding == OVHIP_SURF_DITHER;
    p->shift = fmt->format == OVHIP_SURF_P010 ? 6 : 0;
    p->elems[0] = p->W; p->rows[0] = p->H;
    for (int k = 1; k < p->n_planes; ++k) { p->elems[k] = p->semi ? p->W : p->W / 2; p->rows[k] = p->H / 2; }
    size_t end[3];
    for (int k = 0; k < p->n_planes; ++k) {
        const size_t row = (size_t)p->elems[k] * (size_t)p->es, pitch = k ? fmt->pitch_c : fmt->pitch_y;
        if (pitch && pitch < row) { *why = "pitch below the row's bytes"; return OVHIP_EINVAL; }
        p->pitch[k] = pitch ? pitch : row;
        const uint64_t given = k ? fmt->offset_c[k - 1] : 0;
        if (given > ((uint64_t)1 << 48)) { *why = "offset out of range"; return OVHIP_EINVAL; }
        p->off[k] = given ? (size_t)given : (k ? p->off[k - 1] + p->pitch[k - 1] * (size_t)p->rows[k - 1] : 0);
        end[k] = p->off[k] + p->pitch[k] * (size_t)(p->rows[k] - 1) + row;
        if (end[k] > p->bytes) p->bytes = end[k];
        for (int j = 0; j < k; ++j)
            if (p->off[j] < end[k] && p->off[k] < end[j]) { *why = "planes overlap one another"; return OVHIP_EINVAL; }
    }
    return OVHIP_OK;
}

size_t
ovhip_surface_bytes(int32_t w, int32_t h, const ovhip_window *win, const ovhip_surface_format *fmt)
{
    ovhip_surface_plan_ p;
    const char *why;
    return surface_layout(w, h, win, fmt, &p, &why) == OVHIP_OK ? p.bytes : 0;
}

int
ovhip_surface_plan_make_(const ovhip_pic *pic, const ovhip_window *win, const ovhip_surface_format *fmt, const void *dst, size_t dst_bytes,
                         ovhip_surface_plan_ *plan, const char **why)
{
    const char *dummy;
    if (!why) why = &dummy;
    *why = "null argument";
    if (!pic || !fmt || !plan) return OVHIP_EINVAL;
    const int r = surface_layout(pic->w, pic->h, win, fmt, plan, why);
    if (r != OVHIP_OK) { plan->bytes = 0; return r; }
    const size_t bytes = plan->bytes;
    plan->bytes = 0;
    if (!dst) { *why = "null destination"; return OVHIP_EINVAL; }
    OVHIP_OUT_REFUSE_(ovhip_out_why_planes_(pic));
    OVHIP_OUT_REFUSE_(ovhip_out_why_strides_(pic));
    OVHIP_OUT_REFUSE_(ovhip_out_why_unaligned_(dst, plan->es));                    /* (the alignment before the size: this plan's order) */
    plan->bytes = bytes;                                                           /* (from here on: the launcher's message quotes it) */
    OVHIP_OUT_REFUSE_(ovhip_out_why_small_(dst_bytes, bytes));
    OVHIP_OUT_REFUSE_(ovhip_out_why_overlap_(pic, dst, bytes));
    *why = "";
    return OVHIP_OK;
}

/* one sample's stored value: (x, y) in its own output plane, the pair's column for interleaved chroma */
static inline uint32_t
surf_value(const ovhip_surface_plan_ *p, uint32_t s, int32_t x, int32_t y)
{
    static const uint8_t D[2][2] = { { 0, 2 }, { 3, 1 } };
    if (p->es == 2) return s << p->shift;
    const uint32_t v = (s + (p->dither ? D[y & 1][x & 1] : 2u)) >> 2;
    return v > 255 ? 255 : v;
}

static inline void
surf_put(const ovhip_surface_plan_ *p, uint8_t *row, int32_t e, uint32_t v)
{
    if (p->es == 2) ((uint16_t *)row)[e] = (uint16_t)v; else row[e] = (uint8_t)v;
}

int
ovhip_surface_host(const uint16_t *y, const uint16_t *cb, const uint16_t *cr, int32_t w, int32_t h, int32_t stride_y, int32_t stride_c,
                   const ovhip_window *win, const ovhip_surface_format *fmt, void *dst, size_t dst_bytes)
{
    const ovhip_pic pic = { (uint16_t *)y, (uint16_t *)cb, (uint16_t *)cr, w, h, stride_y, stride_c };
    ovhip_surface_plan_ p;
    const int r = ovhip_surface_plan_make_(&pic, win, fmt, dst, dst_bytes, &p, NULL);
    if (r != OVHIP_OK) return r;
    uint8_t *base = (uint8_t *)dst;
    for (int32_t oy = 0; oy < p.H; ++oy) {
        const uint16_t *src = y + (size_t)(p.y0 + oy) * (size_t)stride_y + p.x0;
        uint8_t *row = base + p.off[0] + (size_t)oy * p.pitch[0];
        for (int32_t ox = 0; ox < p.W; ++ox) surf_put(&p, row, ox, surf_value(&p, src[ox], ox, oy));
    }
    const int32_t cx0 = p.x0 / 2, cy0 = p.y0 / 2, CW = p.W / 2, CH = p.H / 2;
    for (int32_t oy = 0; oy < CH; ++oy) {
        const uint16_t *sb = cb + (size_t)(cy0 + oy) * (size_t)stride_c + cx0, *sr = cr + (size_t)(cy0 + oy) * (size_t)stride_c + cx0;
        uint8_t *row1 = base + p.off[1] + (size_t)oy * p.pitch[1];
        uint8_t *row2 = p.semi ? NULL : base + p.off[2] + (size_t)oy * p.pitch[2];
        for (int32_t ox = 0; ox < CW; ++ox) {
            const uint32_t vb = surf_value(&p, sb[ox], ox, oy), vr = surf_value(&p, sr[ox], ox, oy);
            if (p.semi) { surf_put(&p, row1, 2 * ox, vb); surf_put(&p, row1, 2 * ox + 1, vr); }
            else { surf_put(&p, row1, ox, vb); surf_put(&p, row2, ox, vr); }
        }
    }
    return OVHIP_OK;
}
