/* Motion field output on the host: the refusals and the sizes the launcher shares, and the definition over unit lists in host memory.
 * Definition: include/ovvc_hip.h, "Motion field output on the device"; the device half is kernels_mvfield.hip.
 * Plain C, no HIP calls. */
#include <stdlib.h>
#include <string.h>
#include "ovvc_hip.h"
#include "ovvc_mvfield_priv.h"

int
ovhip_mvfield_format_check_(const ovhip_mvfield_format *fmt, const char **why)
{
    const char *dummy;
    if (!why) why = &dummy;
    *why = "null format";
    if (!fmt) return OVHIP_EINVAL;
    if (fmt->dtype > OVHIP_MVF_F16) { *why = "unknown dtype"; return OVHIP_EINVAL; }
    if (fmt->layout > OVHIP_MVF_CELLS) { *why = "unknown layout"; return OVHIP_EINVAL; }
    if (fmt->vectors > OVHIP_MVF_REFINED) { *why = "unknown vectors value"; return OVHIP_EINVAL; }
    if (fmt->rsv) { *why = "rsv must be 0"; return OVHIP_EINVAL; }
    *why = "";
    return OVHIP_OK;
}

static int elem_bytes(const ovhip_mvfield_format *fmt) { return fmt->dtype == OVHIP_MVF_F16 ? 2 : 4; }

int
ovhip_mvfield_dst_check_(const ovhip_mvfield_format *fmt, const void *vec, size_t vec_bytes, const void *info, size_t info_bytes, const char **why)
{
    const char *dummy;
    if (!why) why = &dummy;
    const int r = ovhip_mvfield_format_check_(fmt, why);
    if (r != OVHIP_OK) return r;
    if (!vec && !info) { *why = "both destinations are NULL"; return OVHIP_EINVAL; }
    if (((uintptr_t)vec & (uintptr_t)(elem_bytes(fmt) - 1)) || ((uintptr_t)info & 3)) { *why = "destination not aligned to its element"; return OVHIP_EINVAL; }
    if (vec && info && (uintptr_t)vec < (uintptr_t)info + info_bytes && (uintptr_t)info < (uintptr_t)vec + vec_bytes) {
        *why = "the destinations overlap each other"; return OVHIP_EINVAL;
    }
    *why = "";
    return OVHIP_OK;
}

static int
field_sizes(int32_t w, int32_t h, const ovhip_mvfield_format *fmt, ovhip_mvfield_plan_ *p, const char **why)
{
    memset(p, 0, sizeof(*p));
    const int r = ovhip_mvfield_format_check_(fmt, why);
    if (r != OVHIP_OK) return r;
    if (w <= 0 || h <= 0 || w > OVHIP_MVF_MAX_SIZE || h > OVHIP_MVF_MAX_SIZE) { *why = "sizes must be positive and at most 16384"; return OVHIP_EINVAL; }
    p->W4 = (w + 3) >> 2; p->H4 = (h + 3) >> 2; p->es = elem_bytes(fmt);
    p->info_bytes = (size_t)4 * (size_t)p->W4 * (size_t)p->H4;
    p->vec_bytes = p->info_bytes * (size_t)p->es;
    return OVHIP_OK;
}

size_t
ovhip_mvfield_bytes(int32_t w, int32_t h, const ovhip_mvfield_format *fmt, size_t *info_bytes)
{
    ovhip_mvfield_plan_ p;
    const char *why;
    const int ok = field_sizes(w, h, fmt, &p, &why) == OVHIP_OK;
    if (info_bytes) *info_bytes = ok ? p.info_bytes : 0;
    return ok ? p.vec_bytes : 0;
}

int
ovhip_mvfield_plan_make_(int32_t w, int32_t h, const ovhip_mvfield_src *src, const ovhip_mvfield_format *fmt, const void *vec, size_t vec_bytes,
                         const void *info, size_t info_bytes, ovhip_mvfield_plan_ *plan, const char **why)
{
    const char *dummy;
    if (!why) why = &dummy;
    int r = field_sizes(w, h, fmt, plan, why);
    if (r != OVHIP_OK) return r;
    if (!src) { *why = "null source"; return OVHIP_EINVAL; }
    if (!vec && !info) { *why = "both destinations are NULL"; return OVHIP_EINVAL; }
    if (((uintptr_t)vec & (uintptr_t)(plan->es - 1)) || ((uintptr_t)info & 3)) { *why = "destination not aligned to its element"; return OVHIP_EINVAL; }
    if (vec && vec_bytes < plan->vec_bytes) { plan->given = vec_bytes; plan->need = plan->vec_bytes; *why = "vector destination too small"; return OVHIP_EINVAL; }
    if (info && info_bytes < plan->info_bytes) { plan->given = info_bytes; plan->need = plan->info_bytes; *why = "info destination too small"; return OVHIP_EINVAL; }
    if (vec && info && (uintptr_t)vec < (uintptr_t)info + plan->info_bytes && (uintptr_t)info < (uintptr_t)vec + plan->vec_bytes) {
        *why = "the destinations overlap each other"; return OVHIP_EINVAL;
    }
    if ((src->n_mc && !src->mc) || (src->n_mcx && !src->mcx) || (src->n_aff && !src->aff) || (src->n_rpr && !src->rpr) || (src->n_affr && !src->affr) ||
        ((src->n_aff || src->n_affr) && !src->side)) { *why = "a non-zero count with a NULL array"; return OVHIP_EINVAL; }
    if (fmt->vectors == OVHIP_MVF_REFINED && src->n_mcx && !src->refined) { *why = "refined vectors asked for, mcx units and no refined array"; return OVHIP_EINVAL; }
    *why = "";
    return OVHIP_OK;
}

/* float32 -> float16 bits, round to nearest even, for the values that occur: 0 and +-[1/16, 2^20] (never subnormal; 65520 and above: infinity) */
static inline uint16_t
half_bits(float f)
{
    uint32_t u;
    memcpy(&u, &f, 4);
    const uint16_t sign = (uint16_t)((u >> 16) & 0x8000u);
    u &= 0x7FFFFFFFu;
    if (!u) return sign;
    u += 0xFFF + ((u >> 13) & 1);
    const uint32_t hv = (u >> 13) - ((127 - 15) << 10);
    return (uint16_t)(sign | (hv >= 0x7C00u ? 0x7C00u : hv));
}

/* unit k of the five lists in their order; 0: it carries no luma */
static int
unit_at(const ovhip_mvfield_src *s, int refined, int list, uint32_t k, mvf_unit_ *o)
{
    switch (list) {
    case 0:  return mvf_from_mc_(&s->mc[k], 0, NULL, o);
    case 1:  return mvf_from_mc_(&s->mcx[k], 1, refined ? s->refined + 4 * (size_t)k : NULL, o);
    case 2:  return mvf_from_aff_(&s->aff[k], o);
    case 3:  return mvf_from_rpr_(&s->rpr[k], o);
    default: return mvf_from_affr_(&s->affr[k], o);
    }
}

static inline void
put_vec(void *vec, int dtype, size_t e, int32_t v)
{
    const float f = (float)v * 0.0625f;
    if (dtype == OVHIP_MVF_I32) ((int32_t *)vec)[e] = v;
    else if (dtype == OVHIP_MVF_F32) ((float *)vec)[e] = f;
    else ((uint16_t *)vec)[e] = half_bits(f);
}

int
ovhip_mvfield_host(int32_t w, int32_t h, const ovhip_mvfield_src *src, const ovhip_mvfield_format *fmt,
                   void *vec, size_t vec_bytes, uint32_t *info, size_t info_bytes)
{
    ovhip_mvfield_plan_ p;
    int r = ovhip_mvfield_plan_make_(w, h, src, fmt, vec, vec_bytes, info, info_bytes, &p, NULL);
    if (r != OVHIP_OK) return r;
    const uint32_t n[5] = { src->n_mc, src->n_mcx, src->n_aff, src->n_rpr, src->n_affr };
    const int refined = fmt->vectors == OVHIP_MVF_REFINED;
    const size_t cells = (size_t)p.W4 * (size_t)p.H4;
    /* the twin's own refusals first, so that a refusal writes nothing: every unit 4-aligned, no cell covered twice */
    uint8_t *seen = (uint8_t *)calloc(cells, 1);
    if (!seen) return OVHIP_ENOMEM;
    mvf_unit_ u;
    for (int l = 0; l < 5 && r == OVHIP_OK; ++l)
        for (uint32_t k = 0; k < n[l] && r == OVHIP_OK; ++k) {
            if (!unit_at(src, refined, l, k, &u)) continue;
            if (((u.x | u.y | u.w | u.h) & 3) || !u.w || !u.h) { r = OVHIP_EINVAL; break; }
            for (int32_t cy = u.y / 4; cy < (u.y + u.h) / 4 && cy < p.H4 && r == OVHIP_OK; ++cy)
                for (int32_t cx = u.x / 4; cx < (u.x + u.w) / 4 && cx < p.W4; ++cx) {
                    if (seen[(size_t)cy * p.W4 + cx]) { r = OVHIP_EINVAL; break; }
                    seen[(size_t)cy * p.W4 + cx] = 1;
                }
        }
    free(seen);
    if (r != OVHIP_OK) return r;

    if (vec) memset(vec, 0, p.vec_bytes);                     /* (0 is the empty vector in every dtype) */
    for (size_t i = 0; info && i < cells; ++i) info[i] = OVHIP_MVF_EMPTY;
    const int cells_layout = fmt->layout == OVHIP_MVF_CELLS;
    for (int l = 0; l < 5; ++l)
        for (uint32_t k = 0; k < n[l]; ++k) {
            if (!unit_at(src, refined, l, k, &u)) continue;
            const int32_t cx0 = u.x / 4, cy0 = u.y / 4, uw4 = u.w / 4;
            for (int32_t cy = cy0; cy < (u.y + u.h) / 4 && cy < p.H4; ++cy)
                for (int32_t cx = cx0; cx < (u.x + u.w) / 4 && cx < p.W4; ++cx) {
                    const size_t cell = (size_t)cy * p.W4 + cx;
                    if (info) info[cell] = u.info;
                    if (!vec) continue;
                    const int32_t *sw = u.aff ? src->side + u.side_off + 4 * (size_t)((cy - cy0) * uw4 + (cx - cx0)) : NULL;
                    for (int c = 0; c < 4; ++c) {
                        const int32_t v = u.aff ? (((u.use >> (c >> 1)) & 1) ? sw[c] : 0) : u.v[c];
                        put_vec(vec, fmt->dtype, cells_layout ? 4 * cell + c : (size_t)c * cells + cell, v);
                    }
                }
        }
    return OVHIP_OK;
}
