/* RGB output through a colour table, on the host: the checks the launcher shares, the texel repack, and the definition over planes and
 * a table in host memory.  Definition: include/ovvc_hip.h, "RGB output through a colour table"; the device half is
 * kernels_rgb_lut.hip.  Plain C, no HIP calls of its own. */
#include <string.h>
#include "ovvc_hip.h"
#include "ovvc_rgb_lut_priv.h"
#include "ovvc_outdst_priv.h"

int
ovhip_rgb_lut_check(int size, int peak, const ovhip_rgb_format *fmt)
{
    if (size != 17 && size != 33 && size != 65) return OVHIP_EINVAL;
    if (peak < 1 || peak > 65535) return OVHIP_EINVAL;
    if (fmt && (fmt->dtype > OVHIP_RGB_F32 || (fmt->dtype == OVHIP_RGB_U8 && peak > 255))) return OVHIP_EINVAL;
    return OVHIP_OK;
}

int
ovhip_rgb_lut_plan_make_(const ovhip_pic *pic, const ovhip_window *win, const ovhip_rgb_format *fmt, int size, int peak, int have_table,
                         const void *dst, size_t dst_bytes, ovhip_rgb_plan_ *plan, const char **why)
{
    const char *dummy;
    if (!why) why = &dummy;
    const int r = ovhip_rgb_plan_make_(pic, win, fmt, dst, dst_bytes, plan, why);
    if (r != OVHIP_OK) return r;
    if (!have_table) { *why = "null table"; return OVHIP_EINVAL; }
    if (ovhip_rgb_lut_check(size, peak, NULL) != OVHIP_OK) { *why = "table size must be 17, 33 or 65 and its peak 1..65535"; return OVHIP_EINVAL; }
    if (fmt->dtype == OVHIP_RGB_U8 && peak > 255) { *why = "a U8 destination needs a table peak <= 255"; return OVHIP_EINVAL; }
    /* the matrix at N = 10 whatever the dtype: the table's input is 0..1023 */
    ovhip_rgb_format f10 = *fmt;
    f10.dtype = OVHIP_RGB_U16;
    (void)ovhip_rgb_coefs(&f10, plan->coef, &plan->yoff);      /* (fmt passed its own refusals above) */
    plan->peak = 1023;
    return OVHIP_OK;
}

int64_t
ovhip_rgb_lut_first_above_(int size, int peak, const uint16_t *table)
{
    const int64_t n = (int64_t)3 * size * size * size;
    for (int64_t i = 0; i < n; ++i) if (table[i] > peak) return i;
    return -1;
}

void
ovhip_rgb_lut_repack_(int size, const uint16_t *table, uint16_t *texels)
{
    const size_t n = (size_t)size * size * size;
    for (size_t i = 0; i < n; ++i) {
        texels[4 * i] = table[3 * i]; texels[4 * i + 1] = table[3 * i + 1]; texels[4 * i + 2] = table[3 * i + 2]; texels[4 * i + 3] = 0;
    }
}

int
ovhip_rgb_lut_host(const uint16_t *y, const uint16_t *cb, const uint16_t *cr, int32_t w, int32_t h, int32_t stride_y, int32_t stride_c,
                   const ovhip_window *win, const ovhip_rgb_format *fmt, int size, int peak, const uint16_t *host_table, void *dst, size_t dst_bytes)
{
    const ovhip_pic pic = { (uint16_t *)y, (uint16_t *)cb, (uint16_t *)cr, w, h, stride_y, stride_c };
    ovhip_rgb_plan_ p;
    const int r = ovhip_rgb_lut_plan_make_(&pic, win, fmt, size, peak, host_table != NULL, dst, dst_bytes, &p, NULL);
    if (r != OVHIP_OK) return r;
    if (ovhip_rgb_lut_first_above_(size, peak, host_table) >= 0) return OVHIP_EINVAL;
    const int32_t n = size - 1;
    const float to_unit = (float)(1.0 / peak);
    const size_t plane = (size_t)p.W * (size_t)p.H;
    for (int32_t oy = 0; oy < p.H; ++oy) {
        for (int32_t ox = 0; ox < p.W; ++ox) {
            int32_t rgb[3];
            ovhip_rgb_pixel_(&pic, &p, p.x0 + ox, p.y0 + oy, 1023, rgb);
            /* the cell and the fractions; ch_[k]: the channel with the k-th largest fraction */
            int32_t idx[3], f[3], ch_[3] = { 0, 1, 2 };
            for (int c = 0; c < 3; ++c) {
                const int32_t t = rgb[c] * n;
                idx[c] = t / 1023; f[c] = t - 1023 * idx[c];
                if (idx[c] == n) { idx[c] = n - 1; f[c] = 1023; }
            }
#define OV_SWAP_(i, j) do { if (f[ch_[i]] < f[ch_[j]]) { const int32_t t_ = ch_[i]; ch_[i] = ch_[j]; ch_[j] = t_; } } while (0)
            OV_SWAP_(0, 1); OV_SWAP_(1, 2); OV_SWAP_(0, 1);
#undef OV_SWAP_
            const int32_t wt[4] = { 1023 - f[ch_[0]], f[ch_[0]] - f[ch_[1]], f[ch_[1]] - f[ch_[2]], f[ch_[2]] };
            int32_t acc[3] = { 511, 511, 511 };
            for (int k = 0; k < 4; ++k) {
                if (k) idx[ch_[k - 1]] += 1;
                const uint16_t *e = host_table + 3 * (((size_t)idx[2] * size + idx[1]) * size + idx[0]);
                for (int c = 0; c < 3; ++c) acc[c] += wt[k] * (int32_t)e[c];
            }
            for (int c = 0; c < 3; ++c) {
                const size_t e = fmt->layout == OVHIP_RGB_PLANAR ? (size_t)c * plane + (size_t)oy * p.W + ox : ((size_t)oy * p.W + ox) * 3 + c;
                ovhip_rgb_put_(dst, e, fmt->dtype, acc[c] / 1023, to_unit);
            }
        }
    }
    return OVHIP_OK;
}
