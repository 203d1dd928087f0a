/* gen_rpr_affine.c -- TEST INFRASTRUCTURE (run where the reference sources are present; not part of build()).
 *
 * Writes tests/golden/rpr/rpr_affine.ovg: what the reference's own slots rcn_mcp_b_l(2,2), rcn_prof_mcp_b_l and rcn_mcp_b_c(3,3)
 * (rcn_inter.c:2815-2966) predict for AFFINE coding units, driven the way rcn_affine_mcp_b_l / rcn_affine_prof_mcp_b_l /
 * rcn_affine_mcp_b_c drive them (drv_affine_mvp.c:3264-3411; gen_mca() of oracle/ref_harness/gen_golden.c), when a used list
 * reads a reference picture of another size.  Reference sizes, seed and collocation settings are gen_rpr.c's, so the reference
 * pictures ARE those of rpr.ovg (their checksums are stored; the samples are not stored twice).  CU sizes 8..64 on both axes; far /
 * normal / integer-translation motion fields, identical motion on one picture, BCW, prof_dir 0..3; at least one case in five is a
 * mixed scaled / unscaled bi-prediction with PROF on the unscaled side.  Every case runs twice over differently poisoned scratch
 * buffers; a case whose outputs differ reads memory nothing wrote and is dropped (more than 2 %, or a whole class: exit 1).
 *
 * Built with -DWITH_SHIM (gen_rpr_affine_shim, needs shim/_build/librcn_hip.so): the second mode.  The same slot calls go to
 * rcn_init_functions_hip's table bound to a recorder (ovhip_shim_bind_recorder, record-only), and what it recorded -- the
 * ovhip_aff_rpr_unit array and the side arena -- must equal, byte for byte, a direct ovhip_rec_affine_cu recording of the same
 * CUs; ovhip_shim_last_error must stay 0.  Writes nothing; exit status 0 / 1.
 */
#include "../../oracle/ref_harness/ref_common.h"
#include "ovvc_hip.h"
#ifdef WITH_SHIM
#include "rcn_hip.h"
#endif

#define PW 128
#define PH 96
#define NSLOT 6

/* struct PROFInfo is private to rcn_inter.c:1128-1134; the slot only forward-declares it. */
struct PROFInfo { int16_t dmv_scale_h_0[16], dmv_scale_v_0[16], dmv_scale_h_1[16], dmv_scale_v_1[16]; };

enum { K_FAR, K_NORMAL, K_INT, K_IDENT, K_BCW, K_PROF0, K_PROF1, K_PROF2, K_PROF3, K_MIXED_PROF, K_BOTH, K_UNI, K_COUNT };
static const char *const k_name[K_COUNT] = { "far", "normal", "integer translation", "identical motion", "BCW", "prof_dir 0", "prof_dir 1",
                                             "prof_dir 2", "prof_dir 3", "mixed bi with PROF", "both lists scaled", "uni" };

static void
dump_rect(gbuf *exp, const uint16_t *p, int stride, int x, int y, int w, int h)
{
    for (int j = 0; j < h; ++j) gbuf_push(exp, p + (y + j) * stride + x, w);
}

static void
poison(OVCTUDec *c, int v)
{
    struct OVRCNCtx *r = &c->rcn_ctx;
    memset(r->data.tmp_rpr, v, sizeof(r->data.tmp_rpr));
    memset(r->data.tmp_buff, v, sizeof(r->data.tmp_buff));
    memset(r->data.tmp_bi_mrg0, v, sizeof(r->data.tmp_bi_mrg0));
    memset(r->data.tmp_bi_mrg1, v, sizeof(r->data.tmp_bi_mrg1));
    memset(r->data.tmp_bi_mrg2, v, sizeof(r->data.tmp_bi_mrg2));
    memset(r->data.tmp_buff0, v, sizeof(r->data.tmp_buff0));
    const struct OVBuffInfo *cb = &r->ctu_buff;
    for (int j = 0; j < 128; ++j) memset(cb->y + j * cb->stride, v, 256);
    for (int j = 0; j < 64; ++j) { memset(cb->cb + j * cb->stride_c, v, 128); memset(cb->cr + j * cb->stride_c, v, 128); }
}

/* the three affine drivers' slot calls for one CU (mv0 / mv1: (x, y) per 4x4 sub-block, row stride nsx) */
static void
drive(OVCTUDec *c, const ovhip_affine_desc *d, int ri0, int ri1, int x0, int y0)
{
    struct InterDRVCtx *ic = &c->drv_ctx.inter_ctx;
    const struct OVBuffInfo *cb = &c->rcn_ctx.ctu_buff;
    const int nsx = (1 << d->log2_w) >> 2, nsy = (1 << d->log2_h) >> 2;
    const int32_t *m0 = d->mv0, *m1 = d->mv1;
    struct PROFInfo pi;
    memcpy(&pi, d->dmv_scale, sizeof(pi));
    for (int j = 0; j < nsy; ++j)
        for (int i = 0; i < nsx; ++i) {
            const int k = j * nsx + i;
            OVMV mv0 = { .x = m0[2 * k], .y = m0[2 * k + 1], .ref_idx = ri0, .bcw_idx_plus1 = d->bcw_idx_plus1 };
            OVMV mv1 = { .x = m1[2 * k], .y = m1[2 * k + 1], .ref_idx = ri1, .bcw_idx_plus1 = d->bcw_idx_plus1 };
            if (!d->prof_dir)
                c->rcn_funcs.rcn_mcp_b_l(c, *cb, ic, c->part_ctx, mv0, mv1, x0 + 4 * i, y0 + 4 * j, 2, 2, d->inter_dir, ri0, ri1);
            else
                c->rcn_funcs.rcn_prof_mcp_b_l(c, *cb, ic, c->part_ctx, mv0, mv1, x0 + 4 * i, y0 + 4 * j, 2, 2, d->inter_dir, ri0, ri1,
                                              d->prof_dir, (const void *)&pi);
        }
    for (int j = 0; j < nsy; j += 2)
        for (int i = 0; i < nsx; i += 2) {
            const int k = j * nsx + i, k2 = k + nsx + 1;
            OVMV mv0 = { .x = m0[2 * k] + m0[2 * k2], .y = m0[2 * k + 1] + m0[2 * k2 + 1], .ref_idx = ri0, .bcw_idx_plus1 = d->bcw_idx_plus1 };
            OVMV mv1 = { .x = m1[2 * k] + m1[2 * k2], .y = m1[2 * k + 1] + m1[2 * k2 + 1], .ref_idx = ri1, .bcw_idx_plus1 = d->bcw_idx_plus1 };
            mv0.x += mv0.x < 0; mv0.y += mv0.y < 0; mv0.x >>= 1; mv0.y >>= 1;
            mv1.x += mv1.x < 0; mv1.y += mv1.y < 0; mv1.x >>= 1; mv1.y >>= 1;
            c->rcn_funcs.rcn_mcp_b_c(c, *cb, ic, c->part_ctx, mv0, mv1, x0 + 4 * i, y0 + 4 * j, 3, 3, d->inter_dir, ri0, ri1);
        }
}

static void
run_case(OVCTUDec *c, const ovhip_affine_desc *d, int ri0, int ri1, int x0, int y0, gbuf *out)
{
    const struct OVBuffInfo *cb = &c->rcn_ctx.ctu_buff;
    const int w = 1 << d->log2_w, h = 1 << d->log2_h;
    drive(c, d, ri0, ri1, x0, y0);
    dump_rect(out, cb->y, cb->stride, x0, y0, w, h);
    dump_rect(out, cb->cb, cb->stride_c, x0 >> 1, y0 >> 1, w >> 1, h >> 1);
    dump_rect(out, cb->cr, cb->stride_c, x0 >> 1, y0 >> 1, w >> 1, h >> 1);
}

static const int sizes[NSLOT + 1][2] = { { 256, 192 }, { 226, 170 }, { 192, 144 }, { 162, 122 }, { 86, 64 }, { 16, 12 }, { PW, PH } };
static OVPicture *ref[NSLOT + 1];
static int slot0[NSLOT + 1], slot1[NSLOT + 1];

/* reference pictures and lists exactly as gen_rpr.c builds them (same seed, same order of random draws) */
static void
setup_refs(OVCTUDec *c)
{
    struct InterDRVCtx *ic = &c->drv_ctx.inter_ctx;
    for (int i = 0; i <= NSLOT; ++i) {
        slot0[i] = i; slot1[i] = i == NSLOT ? NSLOT : NSLOT - 1 - i;
        ic->rpl0[i] = ref[slot0[i]]; ic->rpl1[i] = ref[slot1[i]];
        for (int l = 0; l < 2; ++l) {
            const int s = l ? slot1[i] : slot0[i];
            uint16_t *f = l ? ic->scale_fact_rpl1[i] : ic->scale_fact_rpl0[i];
            f[0] = (uint16_t)(((sizes[s][0] << 14) + PW / 2) / PW);
            f[1] = (uint16_t)(((sizes[s][1] << 14) + PH / 2) / PH);
        }
    }
    ic->prec_amvr = 0;                                        /* drv_affine_mvp.c:3508 */
}

#ifdef WITH_SHIM
/* one decoder + bound recorder + directly driven recorder per collocation setting: the shim hands a slot's scale (and the
 * collocation flags with it) to its recorder once, when it first assigns the slot */
struct shim_side { OVCTUDec *c; ovhip_recorder *shim, *direct; int slot_of[NSLOT + 1], n_slots; };

static int
direct_slot(struct shim_side *s, int pic, int list_ri, int list, const uint8_t col[2])
{
    (void)list_ri; (void)list;
    if (s->slot_of[pic] >= 0) return s->slot_of[pic];
    const int k = s->n_slots++;
    s->slot_of[pic] = k;
    const int sh = ((sizes[pic][0] << 14) + PW / 2) / PW, sv = ((sizes[pic][1] << 14) + PH / 2) / PH;
    if (sh != 1 << 14 || sv != 1 << 14 || sizes[pic][0] != PW || sizes[pic][1] != PH) {
        ovhip_ref_scale sc;
        memset(&sc, 0, sizeof(sc));
        sc.scale_hor = sh; sc.scale_ver = sv; sc.ref_w = sizes[pic][0]; sc.ref_h = sizes[pic][1];
        sc.chroma_hor_col_flag = col[0]; sc.chroma_ver_col_flag = col[1];
        if (ovhip_rec_set_ref_scale(s->direct, k, &sc)) { fprintf(stderr, "shim mode: ovhip_rec_set_ref_scale\n"); exit(1); }
    }
    return k;
}
#endif

int
main(int argc, char **argv)
{
    const char *dir = argc > 1 ? argv[1] : "tests/golden/rpr";
    g_seed = 0x5250;
    OVCTUDec *c = ref_new_ctudec(0, 0);
    struct InterDRVCtx *ic = &c->drv_ctx.inter_ctx;
    for (int i = 0; i <= NSLOT; ++i) {
        ref[i] = ref_new_picture(sizes[i][0], sizes[i][1], 4 * (i + 1));
        fill_plane(ref[i]->frame->data[0], sizes[i][0], sizes[i][1], sizes[i][0]);
        fill_plane(ref[i]->frame->data[1], sizes[i][0] / 2, sizes[i][1] / 2, sizes[i][0] / 2);
        fill_plane(ref[i]->frame->data[2], sizes[i][0] / 2, sizes[i][1] / 2, sizes[i][0] / 2);
    }
    setup_refs(c);
#ifdef WITH_SHIM
    struct shim_side S[4];
    for (int k = 0; k < 4; ++k) {
        S[k].c = ref_new_ctudec(0, 0);
        setup_refs(S[k].c);
        rcn_init_functions_hip(&S[k].c->rcn_funcs, 0, 1, 0, 0, 10);
        S[k].shim = ovhip_rec_create(PW, PH); S[k].direct = ovhip_rec_create(PW, PH);
        if (!S[k].shim || !S[k].direct || ovhip_shim_bind_recorder(S[k].c, S[k].shim, PW, PH) ||
            ovhip_rec_set_rpr_tools(S[k].direct, OVHIP_RPR_TOOL_AFFINE | OVHIP_RPR_TOOL_PU4x4)) { fprintf(stderr, "shim mode: bind failed\n"); return 1; }
        for (int i = 0; i <= NSLOT; ++i) S[k].slot_of[i] = -1;
        S[k].n_slots = 0;
    }
    uint32_t n_compared = 0;
#endif
    g_seed = 0x5250 + 0xAFF;

    gbuf b_desc = { .type = T_U8 }, b_off = { .type = T_U32 }, b_exp = { .type = T_U16 }, b_col = { .type = T_U8 }, b_mv = { .type = T_I32 };
    uint32_t n_cases = 0, n_dropped = 0, kept[K_COUNT] = { 0 }, lost[K_COUNT] = { 0 };
    for (int l2w = 3; l2w <= 6; ++l2w) {
        for (int l2h = 3; l2h <= 6; ++l2h) {
            const int w = 1 << l2w, h = 1 << l2h;
            const int reps = w * h <= 256 ? 30 : (w * h <= 1024 ? 15 : 5);
            for (int rep = 0; rep < reps; ++rep) {
                ovhip_affine_desc d;
                memset(&d, 0, sizeof(d));
                int px, py;
                do {
                    px = rnd_range(0, (PW - w) / 4) * 4;
                    py = rnd_range(0, (PH - h) / 4) * 4;
                } while ((px >> 7) != ((px + w - 1) >> 7) || (py >> 7) != ((py + h - 1) >> 7));
                if (rep % 10 == 6) px = 0;
                if (rep % 10 == 8) py = PH - h;
                d.x0 = px; d.y0 = py; d.log2_w = l2w; d.log2_h = l2h;
                d.inter_dir = rnd_range(1, 3);
                int ri0 = rnd_range(0, NSLOT), ri1 = rnd_range(0, NSLOT);
                d.bcw_idx_plus1 = (rep % 4 == 1) ? rnd_range(1, 5) : 0;
                d.prof_dir = rep % 3 == 0 ? 0 : (d.inter_dir == 3 ? rnd_range(1, 3) : d.inter_dir);
                const int ident = rep % 9 == 4, mixed = rep % 5 == 1;
                if (ident) { d.inter_dir = 3; ri0 = rnd_range(0, NSLOT - 1); ri1 = NSLOT - 1 - ri0; d.prof_dir = 0; }     /* same picture in both lists */
                if (mixed) {
                    /* one list on the unscaled picture, PROF (at least) on that list */
                    d.inter_dir = 3;
                    if (rep & 2) { ri0 = NSLOT; ri1 = rnd_range(0, NSLOT - 1); d.prof_dir = (rep & 4) ? 3 : 1; }
                    else         { ri1 = NSLOT; ri0 = rnd_range(0, NSLOT - 1); d.prof_dir = (rep & 4) ? 3 : 2; }
                }
                d.ref0 = (uint8_t)slot0[ri0]; d.ref1 = (uint8_t)slot1[ri1];
                d.poc0 = ic->rpl0[ri0]->poc; d.poc1 = ic->rpl1[ri1]->poc;
                d.mv_stride = w >> 2;
                for (int t = 0; t < 4; ++t)
                    for (int k = 0; k < 16; ++k) d.dmv_scale[t][k] = (int16_t)(rep % 5 == 3 ? (rnd_range(0, 1) ? 31 : -31) : rnd_range(-31, 31));

                /* a 6-parameter motion field per list, 1/16 pel; every fourth far outside (clip_rpr_position) */
                const int nsx = w >> 2, nsy = h >> 2;
                int32_t *mvs = calloc((size_t)nsx * nsy * 4, sizeof(int32_t));
                int32_t *m0 = mvs, *m1 = mvs + 2 * nsx * nsy;
                const int far = rep % 4 == 0, integer = rep % 7 == 2;
                const int range = far ? 40000 : 300;
                for (int l = 0; l < 2; ++l) {
                    int bx = rnd_range(-range, range), by = rnd_range(-range, range);
                    int ax = rnd_range(-24, 24), ay = rnd_range(-24, 24), cx = rnd_range(-24, 24), cy = rnd_range(-24, 24);
                    if (integer) { ax = ay = cx = cy = 0; bx &= ~15; by &= ~15; }
                    int32_t *m = l ? m1 : m0;
                    for (int j = 0; j < nsy; ++j)
                        for (int i = 0; i < nsx; ++i) {
                            m[2 * (j * nsx + i)] = bx + ((ax * i + cx * j) >> 1);
                            m[2 * (j * nsx + i) + 1] = by + ((ay * i + cy * j) >> 1);
                        }
                }
                if (ident) memcpy(m1, m0, (size_t)nsx * nsy * 8);
                d.mv0 = m0; d.mv1 = m1;

                const int dir = d.inter_dir == 3 ? 3 : (d.inter_dir & 2) ? 2 : 1;
                const int s0 = (dir & 1) && (ic->scale_fact_rpl0[ri0][0] != 1 << 14 || ic->scale_fact_rpl0[ri0][1] != 1 << 14);
                const int s1 = (dir & 2) && (ic->scale_fact_rpl1[ri1][0] != 1 << 14 || ic->scale_fact_rpl1[ri1][1] != 1 << 14);
                if (!s0 && !s1) { free(mvs); continue; }
                int cls[K_COUNT] = { 0 };
                cls[far ? K_FAR : K_NORMAL] = 1; cls[K_INT] = integer; cls[K_IDENT] = ident; cls[K_BCW] = dir == 3 && d.bcw_idx_plus1 && d.bcw_idx_plus1 != 3;
                cls[K_PROF0 + d.prof_dir] = 1; cls[K_UNI] = dir != 3; cls[K_BOTH] = s0 && s1;
                cls[K_MIXED_PROF] = dir == 3 && s0 != s1 && (d.prof_dir & (s0 ? 2 : 1));

                /* chroma collocation flags (SPS-level: every picture the same) */
                uint8_t col[2] = { (uint8_t)(rep & 1), (uint8_t)((rep >> 1) & 1) };
                for (int i = 0; i <= NSLOT; ++i) { ref[i]->scale_info.chroma_hor_col_flag = col[0]; ref[i]->scale_info.chroma_ver_col_flag = col[1]; }
#ifdef WITH_SHIM
                {
                    struct shim_side *s = &S[col[0] | col[1] << 1];
                    s->c->ctb_x = px >> 7; s->c->ctb_y = py >> 7;
                    drive(s->c, &d, ri0, ri1, px & 127, py & 127);
                    ovhip_shim_flush_pending(s->c);
                    if (ovhip_shim_last_error(s->c)) { fprintf(stderr, "shim mode: slot latched error %d (case %u)\n", ovhip_shim_last_error(s->c), n_cases); return 1; }
                    ovhip_affine_desc dd = d;
                    dd.lmcs = s->c->lmcs_info.lmcs_enabled_flag;
                    /* the shim's reference table: order of first use, list 0 before list 1 */
                    if (dir & 1) dd.ref0 = (uint8_t)direct_slot(s, slot0[ri0], ri0, 0, col);
                    if (dir & 2) dd.ref1 = (uint8_t)direct_slot(s, slot1[ri1], ri1, 1, col);
                    if (!(dir & 1)) { dd.ref0 = dd.ref1; dd.poc0 = dd.poc1 + 1; }
                    if (!(dir & 2)) { dd.ref1 = dd.ref0; dd.poc1 = dd.poc0 + 1; }
                    if (ovhip_rec_affine_cu(s->direct, &dd) <= 0) { fprintf(stderr, "shim mode: direct recording failed: %s\n", ovhip_rec_refusal(s->direct)); return 1; }
                    size_t na, nb, sa, sb;
                    const ovhip_aff_rpr_unit *ua = ovhip_rec_aff_rpr_units(s->shim, &na), *ub = ovhip_rec_aff_rpr_units(s->direct, &nb);
                    const int32_t *da = ovhip_rec_aff_side(s->shim, &sa), *db = ovhip_rec_aff_side(s->direct, &sb);
                    if (na != nb || sa != sb || !na || memcmp(ua, ub, na * sizeof(*ua)) || memcmp(da, db, sa * 4)) {
                        fprintf(stderr, "shim mode: case %u: the slots recorded %zu units / %zu side words, the direct call %zu / %zu%s\n", n_cases, na, sa,
                                nb, sb, na == nb && sa == sb ? " (bytes differ)" : "");
                        return 1;
                    }
                    n_compared++; n_cases++;
                    free(mvs);
                    continue;
                }
#endif
                c->ctb_x = px >> 7; c->ctb_y = py >> 7;
                gbuf a = { .type = T_U16 }, b = { .type = T_U16 };
                poison(c, 0xAB); run_case(c, &d, ri0, ri1, px & 127, py & 127, &a);
                poison(c, 0x5C); run_case(c, &d, ri0, ri1, px & 127, py & 127, &b);
                const int stable = a.n == b.n && !memcmp(a.data, b.data, a.n * 2);
                for (int k = 0; k < K_COUNT; ++k) if (cls[k]) (stable ? kept : lost)[k]++;
                if (stable) {
                    uint32_t off[4] = { (uint32_t)b_exp.n, (uint32_t)b_exp.n + w * h, (uint32_t)b_exp.n + w * h + w * h / 4, (uint32_t)b_mv.n };
                    gbuf_push(&b_exp, a.data, a.n);
                    gbuf_push(&b_mv, mvs, (size_t)nsx * nsy * 4);
                    d.mv0 = d.mv1 = NULL;
                    gbuf_push(&b_desc, &d, sizeof(d));
                    gbuf_push(&b_off, off, 4);
                    gbuf_push(&b_col, col, 2);
                    n_cases++;
                } else n_dropped++;
                free(a.data); free(b.data); free(mvs);
            }
        }
    }
#ifdef WITH_SHIM
    fprintf(stderr, "rpr_affine shim mode: %u cases, the slots' recording equals the direct one\n", n_compared);
    return n_compared ? 0 : 1;
#else
    int bad = n_dropped * 50 > n_cases + n_dropped;
    for (int k = 0; k < K_COUNT; ++k) if (!kept[k]) { fprintf(stderr, "rpr_affine.ovg: no case of class '%s' kept (%u dropped)\n", k_name[k], lost[k]); bad = 1; }
    if (n_cases && kept[K_MIXED_PROF] * 5 < n_cases) { fprintf(stderr, "rpr_affine.ovg: fewer than one case in five is mixed bi with PROF\n"); bad = 1; }
    if (bad) { fprintf(stderr, "rpr_affine.ovg: %u of %u cases dropped -- not written\n", n_dropped, n_cases + n_dropped); return 1; }
    gfile g = gfile_open(dir, "rpr_affine.ovg");
    uint32_t sz[NSLOT + 1][2], sums[NSLOT + 1][3];
    for (int i = 0; i <= NSLOT; ++i) {
        sz[i][0] = (uint32_t)sizes[i][0]; sz[i][1] = (uint32_t)sizes[i][1];
        for (int p = 0; p < 3; ++p) {
            const uint16_t *q = (const uint16_t *)ref[i]->frame->data[p];
            const size_t n = (size_t)(sizes[i][0] >> !!p) * (sizes[i][1] >> !!p);
            uint32_t s = 0;
            for (size_t k = 0; k < n; ++k) s = s * 31u + q[k];
            sums[i][p] = s;
        }
    }
    uint32_t dpic[1] = { 2 }, pic[2] = { PW, PH };
    gfile_array(&g, "pic", T_U32, pic, 1, dpic);
    uint32_t ds[2] = { NSLOT + 1, 2 };
    gfile_array(&g, "ref_size", T_U32, sz, 2, ds);
    ds[1] = 3; gfile_array(&g, "ref_sum", T_U32, sums, 2, ds);        /* s = s * 31 + sample over each plane of rpr.ovg's ref<i>_y / _cb / _cr */
    uint32_t d2[2] = { n_cases, sizeof(ovhip_affine_desc) };
    gfile_array(&g, "desc", T_U8, b_desc.data, 2, d2);
    d2[1] = 2; gfile_array(&g, "col", T_U8, b_col.data, 2, d2);
    d2[1] = 4; gfile_array(&g, "off", T_U32, b_off.data, 2, d2);      /* luma, cb, cr in exp; the sub-block vectors in mv */
    gfile_buf(&g, "exp", &b_exp);
    gfile_buf(&g, "mv", &b_mv);
    uint32_t d1[1] = { 1 };
    gfile_array(&g, "n_dropped", T_U32, &n_dropped, 1, d1);
    gfile_close(&g);
    fprintf(stderr, "rpr_affine.ovg: %u cases (%u dropped: output depends on unwritten scratch), %zu expected samples;", n_cases, n_dropped, b_exp.n);
    for (int k = 0; k < K_COUNT; ++k) fprintf(stderr, " %s %u", k_name[k], kept[k]);
    fprintf(stderr, "\n");
    return 0;
#endif
}
