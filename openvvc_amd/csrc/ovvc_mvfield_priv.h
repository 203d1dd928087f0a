/* ovvc_mvfield_priv.h -- private: what the host twin (ovvc_mvfield.c) and the launcher (kernels_mvfield.hip) of the motion field output
 * share: the refusals, the sizes, and what ONE unit of each list says about its cells (include/ovvc_hip.h, "Motion field output on
 * the device").  Plain C; under hipcc the per-unit functions are also device code. */
#ifndef OVVC_MVFIELD_PRIV_H
#define OVVC_MVFIELD_PRIV_H
#include "ovvc_hip.h"
#include "ovvc_dpb_priv.h"

#ifdef __HIPCC__
#define MVF_FN_ __host__ __device__ __forceinline__
#else
#define MVF_FN_ static inline
#endif

#define OVHIP_MVF_MAX_SIZE 16384

typedef struct ovhip_mvfield_plan_ {
    int32_t W4, H4, es;                /* the grid; bytes per vector element */
    size_t vec_bytes, info_bytes;      /* the sizes of the two destinations */
    size_t given, need;                /* of a refusal for "too small": the destination's byte count and its size */
} ovhip_mvfield_plan_;

#ifdef __cplusplus
extern "C" {
#endif
/* the refusals that need neither a size nor a destination: a null format, enum values, rsv */
OVHIP_HIDDEN_ int ovhip_mvfield_format_check_(const ovhip_mvfield_format *fmt, const char **why);
/* the refusals that need no picture: the format's, both destinations NULL, alignment, and -- of what the byte counts say -- overlap */
OVHIP_HIDDEN_ int ovhip_mvfield_dst_check_(const ovhip_mvfield_format *fmt, const void *vec, size_t vec_bytes, const void *info, size_t info_bytes, const char **why);
/* every refusal the host twin and the launch have in common; *why: a string literal */
OVHIP_HIDDEN_ int ovhip_mvfield_plan_make_(int32_t w, int32_t h, const ovhip_mvfield_src *src, const ovhip_mvfield_format *fmt, const void *vec, size_t vec_bytes,
                                           const void *info, size_t info_bytes, ovhip_mvfield_plan_ *plan, const char **why);
#ifdef __cplusplus
}
#endif

/* What a unit says about the cells it covers.  aff: the cells' vectors are the side words side[side_off + 4k + c] of the channels
 * whose list is in `use` (bit 0: list 0, bit 1: list 1), 0 for the others; otherwise they are v[] for every cell. */
typedef struct mvf_unit_ {
    int32_t x, y, w, h;
    uint32_t info;
    int32_t v[4];
    uint32_t side_off, use;
    int32_t aff;
} mvf_unit_;

MVF_FN_ uint32_t mvf_info_(uint32_t dir, uint32_t ref0, uint32_t ref1, uint32_t kind, int gpm, int w0, int w1, uint32_t scaled)
{
    if (gpm) kind |= OVHIP_MVF_GPM;
    else if (dir == 3 && (w0 != 4 || w1 != 4)) kind |= OVHIP_MVF_BCW;
    return ((dir & 1) ? ref0 : 0xFFu) | (((dir & 2) ? ref1 : 0xFFu) << 8) | (kind << 16) | ((scaled & dir) << 24);
}

/* a unit of mc (is_mcx 0) or of mcx; refined: the unit's four words of the refined array, or NULL.  0: the unit carries no luma */
MVF_FN_ int mvf_from_mc_(const ovhip_mc_unit *u, int is_mcx, const int32_t *refined, mvf_unit_ *o)
{
    if (!is_mcx && (u->flags & OVHIP_MC_NO_LUMA)) return 0;
    uint32_t kind = OVHIP_MVF_INTER;
    if (is_mcx && (u->flags & OVHIP_MC_DMVR)) kind |= OVHIP_MVF_DMVR;
    if (is_mcx && (u->flags & OVHIP_MC_BDOF)) kind |= OVHIP_MVF_BDOF;
    o->x = u->x; o->y = u->y; o->w = u->w; o->h = u->h; o->aff = 0; o->side_off = 0; o->use = u->dir;
    o->info = mvf_info_(u->dir, u->ref0, u->ref1, kind, (u->flags & OVHIP_MC_GPM) != 0, u->w0, u->w1, 0);
    const int take = is_mcx && refined && (u->flags & OVHIP_MC_DMVR);
    o->v[0] = take ? refined[0] : u->mv0x; o->v[1] = take ? refined[1] : u->mv0y;
    o->v[2] = take ? refined[2] : u->mv1x; o->v[3] = take ? refined[3] : u->mv1y;
    if (!(u->dir & 1)) o->v[0] = o->v[1] = 0;
    if (!(u->dir & 2)) o->v[2] = o->v[3] = 0;
    return 1;
}

MVF_FN_ int mvf_from_aff_(const ovhip_aff_unit *u, mvf_unit_ *o)
{
    o->x = u->x; o->y = u->y; o->w = u->w; o->h = u->h; o->aff = 1; o->side_off = u->side_off; o->use = u->dir;
    o->info = mvf_info_(u->dir, u->ref0, u->ref1, OVHIP_MVF_INTER | OVHIP_MVF_AFFINE | ((u->flags & OVHIP_AFF_PROF) ? OVHIP_MVF_PROF : 0), 0, u->w0, u->w1, 0);
    o->v[0] = o->v[1] = o->v[2] = o->v[3] = 0;
    return 1;
}

MVF_FN_ int mvf_from_rpr_(const ovhip_rpr_unit *u, mvf_unit_ *o)
{
    if (u->flags & OVHIP_RPR_NO_LUMA) return 0;
    const uint32_t scaled = u->flags & (OVHIP_RPR_S0 | OVHIP_RPR_S1), use = u->dir & ~scaled;
    o->x = u->x; o->y = u->y; o->w = u->w; o->h = u->h; o->aff = 0; o->side_off = 0; o->use = use;
    o->info = mvf_info_(u->dir, u->s[0].ref, u->s[1].ref, OVHIP_MVF_INTER, (u->flags & OVHIP_RPR_GPM) != 0, u->w0, u->w1, scaled);
    o->v[0] = (use & 1) ? u->s[0].pos_x : 0; o->v[1] = (use & 1) ? u->s[0].pos_y : 0;
    o->v[2] = (use & 2) ? u->s[1].pos_x : 0; o->v[3] = (use & 2) ? u->s[1].pos_y : 0;
    return 1;
}

MVF_FN_ int mvf_from_affr_(const ovhip_aff_rpr_unit *u, mvf_unit_ *o)
{
    const uint32_t scaled = u->flags & (OVHIP_AFFR_S0 | OVHIP_AFFR_S1);
    o->x = u->x; o->y = u->y; o->w = u->w; o->h = u->h; o->aff = 1; o->side_off = u->side_off; o->use = u->dir & ~scaled;
    o->info = mvf_info_(u->dir, u->s[0].ref, u->s[1].ref, OVHIP_MVF_INTER | OVHIP_MVF_AFFINE | ((u->flags & OVHIP_AFFR_PROF) ? OVHIP_MVF_PROF : 0), 0, u->w0, u->w1, scaled);
    o->v[0] = o->v[1] = o->v[2] = o->v[3] = 0;
    return 1;
}
#endif
