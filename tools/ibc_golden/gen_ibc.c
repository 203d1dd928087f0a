/* gen_ibc.c -- TEST INFRASTRUCTURE (run where the reference sources are present; not part of build()).
 *
 * Writes tests/golden/ibc/ibc.ovg (scenarios a and c) and tests/golden/ibc/ibc_rows.ovg (scenario b; one file would pass the size a
 * committed file may have): what the reference's own slots rcn_ibc_l / rcn_ibc_c (rcn_ibc.c:8-139) followed by tmp.rcn_transform_tree
 * with cu_flags = flg_ibc_flag (vcl_coding_unit.c:1032-1066, vcl_transform_unit.c:1889-1959) leave in a picture.  A scenario is one or
 * two CTU rows; for every CTU the generator attaches the ring (rcn_attach_ctu_buff, rcn_ctu.c:554-568), copies that CTU's seeded
 * "already reconstructed" background into it, runs the CTU's coding units in list order and copies the CTU out into the frame:
 *   a  CTU 128, 512x128: CU sizes 4x4 (luma only), 4x64, 64x4, 8x8, 16x32, 64x64 with log2_max_tb_s = 5; odd and even vectors; sources in
 *      the left CTU, in the current one and across the boundary; mv = (-w, 0) and (0, -h); a chain of 32 CUs each copying the one before
 *      it across two CTU boundaries; sources covering several producers; CUs with and without residual (DC only, transform skip)
 *   b  the same over two CTU rows (512x256): nothing crosses rows
 *   c  CTU 64, 640x64: ten CTUs, so the ring of eight wraps; sources up to seven CTUs left and across the ring's end
 * The lists are built here and checked here: no two CUs overlap, every vector lies in the window in which the ring holds the picture's
 * own sample (ovhip_rec_ibc_check states the same rule), and no CU's source touches the block of a LATER CU (a decoder never meets
 * that: such samples are not decoded yet).  Every scenario runs twice over differently poisoned ring memory and must come out the same.
 * Stored per scenario <s>: <s>_dims (w, h, log2_ctu, log2_max_tb), <s>_bg_y/cb/cr, <s>_exp_y/cb/cr, <s>_cu [n][8] (x0, y0, log2_w,
 * log2_h, mv_x, mv_y, has_chroma, first TU), <s>_tu [m][14] (CU, x0, y0, log2_w, log2_h, tree, cbf_mask, tr_skip_mask, last_pos x 3,
 * coefficient offsets x 3 or -1), <s>_map [m][3] (sig_sb_map), <s>_coef, <s>_state (ovhip_tu_state).
 *
 * Built with -DWITH_SHIM (gen_ibc_shim, needs shim/_build/librcn_hip.so): the second mode.  The same slot calls go to
 * rcn_init_functions_hip's table bound to a recorder, and the ordered tasks, transform-block commands and coefficients it recorded must
 * equal, byte for byte, those of direct ovhip_rec_tu_ibc calls; ovhip_shim_last_error must stay 0.  Writes nothing; exit status 0 / 1.
 */
#include "../../oracle/ref_harness/ref_common.h"
#include "ovvc_hip.h"
#ifdef WITH_SHIM
#include "rcn_hip.h"
#endif

/* struct TUInfo is private to rcn_transform_tree.c:51-66; the slot signature only forward-declares it */
struct TBInfo { uint16_t last_pos; uint64_t sig_sb_map; };
struct TUInfo {
    uint8_t is_sbt; uint8_t cbf_mask; uint16_t pos_offset; uint8_t tr_skip_mask;
    uint8_t cu_mts_flag; uint8_t cu_mts_idx; uint8_t lfnst_flag; uint8_t lfnst_idx;
    struct TBInfo tb_info[3];
};
extern int transform_unit_st(OVCTUDec *const, unsigned int, unsigned int, unsigned int, unsigned int, uint8_t, CUFlags, uint8_t, struct TUInfo *const);
extern int transform_unit_l(OVCTUDec *const, unsigned int, unsigned int, unsigned int, unsigned int, uint8_t, CUFlags, uint8_t, struct TUInfo *const);

enum { RES_NONE, RES_DC, RES_TS, RES_MIXED };
struct cu { int x0, y0, l2w, l2h, mvx, mvy, chroma, res, seq; };
struct scen { const char *name; int w, h, l2c, max_tb; struct cu cu[1024]; int n; };

static int
n_ring_ctb(int l2c) { return ((256 * 128) >> l2c) >> l2c; }

/* the window in which the ring holds the picture's own sample (include/ovvc_hip.h, ovhip_ibc_desc) */
static int
window_ok(const struct scen *s, const struct cu *c)
{
    const int w = 1 << c->l2w, h = 1 << c->l2h, sx = c->x0 + c->mvx, sy = c->y0 + c->mvy, l2c = s->l2c, cx = c->x0 >> l2c;
    if (sy < 0 || (sy >> l2c) != (c->y0 >> l2c) || ((sy + h - 1) >> l2c) != (c->y0 >> l2c)) return 0;
    if (sx < 0 || sx < ((cx - (n_ring_ctb(l2c) - 1)) << l2c)) return 0;
    if (sx + w > ((cx + 1) << l2c) || sx + w > s->w || sy + h > s->h) return 0;
    if (sx < c->x0 + w && sx + w > c->x0 && sy < c->y0 + h && sy + h > c->y0) return 0;
    return 1;
}

static int
rects_meet(int ax, int ay, int aw, int ah, int bx, int by, int bw, int bh) { return ax < bx + bw && ax + aw > bx && ay < by + bh && ay + ah > by; }

static int
ctu_of(const struct scen *s, const struct cu *c) { return (c->y0 >> s->l2c) * ((s->w + (1 << s->l2c) - 1) >> s->l2c) + (c->x0 >> s->l2c); }

/* may this CU be appended: in the picture, aligned, window, no overlap with a CU already there nor with the source of one that is
 * decoded before it (a CU of an earlier CTU, or one listed earlier in the same CTU) */
static int
can_add(const struct scen *s, const struct cu *c)
{
    const int w = 1 << c->l2w, h = 1 << c->l2h;
    if (c->x0 < 0 || c->y0 < 0 || c->x0 + w > s->w || c->y0 + h > s->h || (c->x0 & 3) || (c->y0 & 3)) return 0;
    if ((c->x0 >> s->l2c) != ((c->x0 + w - 1) >> s->l2c) || (c->y0 >> s->l2c) != ((c->y0 + h - 1) >> s->l2c)) return 0;
    if (!window_ok(s, c)) return 0;
    for (int i = 0; i < s->n; ++i) {
        const struct cu *o = &s->cu[i];
        const int ow = 1 << o->l2w, oh = 1 << o->l2h;
        if (rects_meet(c->x0, c->y0, w, h, o->x0, o->y0, ow, oh)) return 0;
        if (ctu_of(s, c) >= ctu_of(s, o) && rects_meet(c->x0, c->y0, w, h, o->x0 + o->mvx, o->y0 + o->mvy, ow, oh)) return 0;
    }
    return 1;
}

static void
add(struct scen *s, int x0, int y0, int l2w, int l2h, int mvx, int mvy, int chroma, int res)
{
    struct cu c = { x0, y0, l2w, l2h, mvx, mvy, chroma, res, s->n };
    if (s->n >= 1024 || !can_add(s, &c)) { fprintf(stderr, "%s: CU %d (%d, %d) %dx%d mv (%d, %d) breaks a rule of the list\n", s->name, s->n, x0, y0, 1 << l2w, 1 << l2h, mvx, mvy); exit(1); }
    s->cu[s->n++] = c;
}

static const int shapes[6][2] = { { 2, 2 }, { 2, 6 }, { 6, 2 }, { 3, 3 }, { 4, 5 }, { 6, 6 } };

/* seeded CUs in CTU (cx, cy): any shape, any vector the window allows */
static void
add_random(struct scen *s, int cx, int cy, int count, int max_shape)
{
    const int S = 1 << s->l2c, X0 = cx << s->l2c, Y0 = cy << s->l2c;
    for (int k = 0, tries = 0; k < count && tries < 20000; ++tries) {
        const int *sh = shapes[rnd_range(0, max_shape)];
        const int w = 1 << sh[0], h = 1 << sh[1];
        if (w > S || h > S) continue;
        struct cu c = { X0 + rnd_range(0, (S - w) / w) * w, Y0 + rnd_range(0, (S - h) / h) * h, sh[0], sh[1], 0, 0, !(sh[0] == 2 && sh[1] == 2), rnd_range(0, 3), s->n };
        int lo = (cx - (n_ring_ctb(s->l2c) - 1)) << s->l2c;
        if (rnd_range(0, 3) && lo < X0 - S) lo = X0 - S;          /* three in four from the CTU itself or its left neighbour: producers are met */
        if (lo < 0) lo = 0;
        c.mvx = rnd_range(lo, X0 + S - w) - c.x0; c.mvy = rnd_range(Y0, Y0 + S - h) - c.y0;
        if (!can_add(s, &c)) continue;
        s->cu[s->n++] = c; ++k;
    }
}

/* scenario a's list, in the CTU row that starts at picture row Y */
static void
build_row(struct scen *s, int Y)
{
    /* CTU 0: no CTU to the left; columns 0..63 stay background */
    add(s, 64, Y + 0, 6, 6, -64, 0, 1, RES_MIXED);            /* 64x64: four transform units, mv = (-w, 0) */
    add(s, 64, Y + 64, 4, 5, -33, -17, 1, RES_TS);            /* odd vector on both axes */
    add(s, 80, Y + 64, 3, 3, -8, 0, 1, RES_DC);               /* the block written just before, to the left */
    add(s, 80, Y + 72, 3, 3, 0, -8, 1, RES_NONE);             /* ... and above */
    add(s, 88, Y + 64, 2, 2, -5, -3, 0, RES_TS);              /* 4x4, luma only: its source covers two producers */
    add(s, 100, Y + 64, 2, 6, -61, -64, 1, RES_DC);           /* 4x64 */
    add(s, 0, Y + 124, 6, 2, 3, -4, 1, RES_TS);               /* 64x4, vector to the right */
    add(s, 92, Y + 64, 2, 2, -4, 0, 0, RES_NONE);
    /* CTU 1 */
    add(s, 128, Y + 0, 3, 3, -128, 0, 1, RES_DC);             /* source wholly in the left CTU, even vector */
    add(s, 144, Y + 0, 4, 5, -75, 13, 1, RES_TS);             /* ... inside the left CTU's 64x64 CU, odd vector */
    add(s, 128, Y + 64, 6, 2, -40, -8, 1, RES_NONE);          /* source across the CTU boundary */
    add(s, 160, Y + 72, 3, 3, -9, -1, 1, RES_TS);             /* source in the current CTU */
    add(s, 192, Y + 0, 6, 6, -64, 0, 1, RES_MIXED);           /* source covers two CUs of this CTU and background */
    /* the chain: 32 CUs of 8x8, each a copy of the one before it (+ residual), through CTU 1, 2 and 3 */
    for (int k = 0; k < 32; ++k) add(s, 160 + 8 * k, Y + 104, 3, 3, -8, 0, 1, (k & 1) ? RES_TS : RES_DC);
    add_random(s, 2, Y >> 7, 24, 5);
    add_random(s, 3, Y >> 7, 24, 5);
    add_random(s, 1, Y >> 7, 8, 4);
}

static int
cmp_cu(const void *a, const void *b)
{
    const struct cu *p = a, *q = b;
    return p->seq - q->seq;
}

/* decoding order: CTU by CTU (raster), inside a CTU as listed */
static void
sort_by_ctu(struct scen *s)
{
    const int ncx = (s->w + (1 << s->l2c) - 1) >> s->l2c;
    for (int i = 0; i < s->n; ++i) s->cu[i].seq += 4096 * ((s->cu[i].y0 >> s->l2c) * ncx + (s->cu[i].x0 >> s->l2c));
    qsort(s->cu, s->n, sizeof(s->cu[0]), cmp_cu);
    /* no source may touch the block of a later CU */
    for (int i = 0; i < s->n; ++i)
        for (int j = i + 1; j < s->n; ++j) {
            const struct cu *a = &s->cu[i], *b = &s->cu[j];
            if (rects_meet(a->x0 + a->mvx, a->y0 + a->mvy, 1 << a->l2w, 1 << a->l2h, b->x0, b->y0, 1 << b->l2w, 1 << b->l2h)) {
                fprintf(stderr, "%s: CU %d reads what CU %d writes later\n", s->name, i, j); exit(1);
            }
        }
}

/* TUInfo slots tmp.rcn_transform_tree visits for a CU no larger than 64x64, with the leaf's position (rcn_transform_tree.c:1454-1506) */
struct leaf { int slot, x, y; };
static int
leaves_of(int l2w, int l2h, int max_tb, struct leaf *out)
{
    const int sv = l2w > max_tb, sh = l2h > max_tb, nsub = 1 << (sv + sh), w1 = (1 << l2w) >> sv, h1 = (1 << l2h) >> sh;
    int n = 0;
    out[n++] = (struct leaf){ 0, 0, 0 };
    if (sv) out[n++] = (struct leaf){ nsub, w1, 0 };
    if (sh) out[n++] = (struct leaf){ 2 * nsub, 0, h1 };
    if (sv && sh) out[n++] = (struct leaf){ 3 * nsub, w1, h1 };
    return n;
}

static int16_t
small_coef(void)
{
    const int k = rnd_range(0, 15);
    return (int16_t)(k < 12 ? rnd_range(-40, 40) : (k < 15 ? rnd_range(-300, 300) : rnd_range(-1100, 1100)));
}

struct tu_rec { int32_t v[14]; uint64_t map[3]; };
struct cu_tus { struct TUInfo tu[16]; int n_leaf; struct leaf leaf[4]; int lw, lh; uint32_t used; };

/* the CU's TUInfo array and coefficients (into c->residual_*), seeded; records go to recs / coefs when given */
static void
make_tus(OVCTUDec *c, const struct scen *s, const struct cu *cu, int cu_idx, struct cu_tus *o, gbuf *recs, gbuf *maps, gbuf *coefs)
{
    memset(o, 0, sizeof(*o));
    memset(c->residual_y, 0, sizeof(c->residual_y)); memset(c->residual_cb, 0, sizeof(c->residual_cb)); memset(c->residual_cr, 0, sizeof(c->residual_cr));
    o->lw = cu->l2w > s->max_tb ? s->max_tb : cu->l2w; o->lh = cu->l2h > s->max_tb ? s->max_tb : cu->l2h;
    o->n_leaf = leaves_of(cu->l2w, cu->l2h, s->max_tb, o->leaf);
    const uint32_t leaf_sz = 1u << (o->lw + o->lh);
    for (int q = 0; q < o->n_leaf; ++q) {
        struct TUInfo *t = &o->tu[o->leaf[q].slot];
        int res = cu->res == RES_MIXED ? rnd_range(0, 2) : cu->res;
        t->pos_offset = (uint16_t)o->used;
        int32_t r[14] = { cu_idx, cu->x0 + o->leaf[q].x, cu->y0 + o->leaf[q].y, o->lw, o->lh, cu->chroma ? 0 : 1, 0, 0, 0, 0, 0, -1, -1, -1 };
        uint64_t map[3] = { 0, 0, 0 };
        int16_t *dst[3] = { c->residual_cb, c->residual_cr, c->residual_y };
        for (int comp = 0; comp < 3 && res != RES_NONE; ++comp) {
            const int is_l = comp == 2, l2w = is_l ? o->lw : o->lw - 1, l2h = is_l ? o->lh : o->lh - 1;
            if (!is_l && !cu->chroma) continue;
            if (rnd_range(0, 4) == 0 && !(is_l && !cu->chroma)) continue;              /* this block's cbf is 0 */
            const int bit = is_l ? 0x10 : (comp ? 0x1 : 0x2), n = 1 << (l2w + l2h);
            int16_t *d = dst[comp] + t->pos_offset;
            t->cbf_mask |= bit;
            if (res == RES_TS) {
                t->tr_skip_mask |= bit;
                for (int i = 0; i < n; ++i) d[i] = rnd_range(0, 2) ? small_coef() : 0;
                t->tb_info[comp].last_pos = 0x0101; t->tb_info[comp].sig_sb_map = 1;
            } else {
                d[0] = (int16_t)rnd_range(-700, 700);
                if (!d[0]) d[0] = 9;
                t->tb_info[comp].last_pos = 0; t->tb_info[comp].sig_sb_map = 1;
            }
            r[8 + comp] = t->tb_info[comp].last_pos; map[comp] = t->tb_info[comp].sig_sb_map;
            if (coefs) { r[11 + comp] = (int32_t)coefs->n; gbuf_push(coefs, d, n); }
        }
        /* (the transform unit of a luma-only CU gets the luma cbf alone: rcn_tu_l) */
        r[6] = t->cbf_mask; r[7] = t->tr_skip_mask;
        if (recs) { gbuf_push(recs, r, 14); gbuf_push(maps, map, 3); }
        o->used += leaf_sz;
    }
}

static void
set_state(OVCTUDec *c, ovhip_tu_state *st)
{
    memset(st, 0, sizeof(*st));
    st->qp_y = 34; st->qp_cb = 31; st->qp_cr = 37; st->qp_jcbcr = 33;
    st->qp_y_skip = st->qp_y; st->qp_cb_skip = st->qp_cb; st->qp_cr_skip = st->qp_cr; st->qp_jcbcr_skip = st->qp_jcbcr;
    c->dequant_luma.qp = st->qp_y; c->dequant_cb.qp = st->qp_cb; c->dequant_cr.qp = st->qp_cr; c->dequant_joint_cb_cr.qp = st->qp_jcbcr;
    c->dequant_luma_skip.qp = st->qp_y_skip; c->dequant_cb_skip.qp = st->qp_cb_skip; c->dequant_cr_skip.qp = st->qp_cr_skip; c->dequant_jcbcr_skip.qp = st->qp_jcbcr_skip;
    c->residual_coding_l = NULL; c->mts_implicit = 0; c->sh_ts_disabled = 0; c->tmp_ciip = 0;
    c->lmcs_info.scale_c_flag = 0; c->lmcs_info.lmcs_chroma_scale = 0;
    c->qp_ctx.qp_bd_offset = 12;
}

/* one pass over the scenario: frame = what the reference leaves; the records of the TUs go to recs / maps / coefs when given */
static void
run_scenario(OVCTUDec *c, const struct scen *s, uint16_t *const bg[3], uint16_t *const frame[3], int poison, gbuf *recs, gbuf *maps, gbuf *coefs,
             gbuf *cu_first)
{
    const int l2c = s->l2c, S = 1 << l2c, ncx = (s->w + S - 1) >> l2c, ncy = (s->h + S - 1) >> l2c, wc = s->w >> 1;
    struct OVRCNCtx *r = &c->rcn_ctx;
    memset(r->data.y_buff, poison, sizeof(r->data.y_buff)); memset(r->data.cb_buff, poison, sizeof(r->data.cb_buff)); memset(r->data.cr_buff, poison, sizeof(r->data.cr_buff));
    g_seed = 0x1bc0 + (uint32_t)s->w;                          /* the coefficients: the same in both passes */
    int i = 0;
    uint32_t n_tu = 0;
    for (int cy = 0; cy < ncy; ++cy)
        for (int cx = 0; cx < ncx; ++cx) {
            const int X0 = cx << l2c, Y0 = cy << l2c, cw = s->w - X0 < S ? s->w - X0 : S, ch = s->h - Y0 < S ? s->h - Y0 : S;
            c->ctb_x = cx; c->ctb_y = cy;
            const struct OVBuffInfo *b = &r->ctu_buff;
            if (bg) c->rcn_funcs.rcn_attach_ctu_buff(r, l2c, cx);
            for (int y = 0; bg && y < ch; ++y) memcpy(b->y + y * b->stride, bg[0] + (size_t)(Y0 + y) * s->w + X0, 2 * cw);
            for (int y = 0; bg && y < ch / 2; ++y) {
                memcpy(b->cb + y * b->stride_c, bg[1] + (size_t)(Y0 / 2 + y) * wc + X0 / 2, cw);
                memcpy(b->cr + y * b->stride_c, bg[2] + (size_t)(Y0 / 2 + y) * wc + X0 / 2, cw);
            }
            for (; i < s->n && (s->cu[i].x0 >> l2c) == cx && (s->cu[i].y0 >> l2c) == cy; ++i) {
                const struct cu *cu = &s->cu[i];
                const IBCMV mv = { cu->mvx, cu->mvy };
                struct cu_tus t;
                if (cu_first) gbuf_push(cu_first, &n_tu, 1);
                make_tus(c, s, cu, i, &t, recs, maps, coefs);
                n_tu += t.n_leaf;
                c->rcn_funcs.rcn_ibc_l(c, cu->x0 - X0, cu->y0 - Y0, cu->l2w, cu->l2h, l2c, mv);
                if (cu->chroma) c->rcn_funcs.rcn_ibc_c(c, cu->x0 - X0, cu->y0 - Y0, cu->l2w, cu->l2h, l2c, mv);
                c->transform_unit = cu->chroma ? (void *)&transform_unit_st : (void *)&transform_unit_l;
                c->rcn_funcs.tmp.rcn_transform_tree(c, cu->x0 - X0, cu->y0 - Y0, cu->l2w, cu->l2h, s->max_tb, 0, flg_ibc_flag, t.tu);
            }
            if (!frame) continue;
            for (int y = 0; y < ch; ++y) memcpy(frame[0] + (size_t)(Y0 + y) * s->w + X0, b->y + y * b->stride, 2 * cw);
            for (int y = 0; y < ch / 2; ++y) {
                memcpy(frame[1] + (size_t)(Y0 / 2 + y) * wc + X0 / 2, b->cb + y * b->stride_c, cw);
                memcpy(frame[2] + (size_t)(Y0 / 2 + y) * wc + X0 / 2, b->cr + y * b->stride_c, cw);
            }
        }
    if (i != s->n) { fprintf(stderr, "%s: %d of %d CUs run\n", s->name, i, s->n); exit(1); }
}

static void
named(gfile *g, const struct scen *s, const char *what, int type, const void *data, int ndim, uint32_t d0, uint32_t d1)
{
    char nm[32];
    uint32_t dims[2] = { d0, d1 };
    snprintf(nm, sizeof(nm), "%s_%s", s->name, what);
    gfile_array(g, nm, type, data, ndim, dims);
}

#ifdef WITH_SHIM
/* the same CUs through the installed slots and through direct recorder calls: the recordings must be the same bytes */
static int
shim_compare(const struct scen *s)
{
    g_part.log2_ctu_s = (uint8_t)s->l2c;
    OVCTUDec *c = ref_new_ctudec(0, 0), *cd = ref_new_ctudec(0, 0);
    ovhip_tu_state st;
    set_state(c, &st); set_state(cd, &st);
    rcn_init_functions_hip(&c->rcn_funcs, 0, 1, 0, 0, 10);
    ovhip_recorder *shim = ovhip_rec_create(s->w, s->h), *direct = ovhip_rec_create(s->w, s->h);
    if (!shim || !direct || ovhip_shim_bind_recorder(c, shim, s->w, s->h) || ovhip_rec_set_ctu_size(direct, s->l2c)) { fprintf(stderr, "shim mode: bind failed\n"); return 1; }
    run_scenario(c, s, NULL, NULL, 0, NULL, NULL, NULL, NULL);       /* (the slots record; nothing is reconstructed on the host) */
    ovhip_shim_flush_pending(c);
    if (ovhip_shim_last_error(c)) { fprintf(stderr, "shim mode: %s: the slots latched error %d\n", s->name, ovhip_shim_last_error(c)); return 1; }
    g_seed = 0x1bc0 + (uint32_t)s->w;
    for (int i = 0; i < s->n; ++i) {
        const struct cu *cu = &s->cu[i];
        struct cu_tus t;
        make_tus(cd, s, cu, i, &t, NULL, NULL, NULL);
        ovhip_ibc_desc d;
        memset(&d, 0, sizeof(d));
        d.x0 = cu->x0; d.y0 = cu->y0; d.log2_w = cu->l2w; d.log2_h = cu->l2h; d.log2_ctu = s->l2c; d.has_chroma = cu->chroma;
        d.mv_x = cu->mvx; d.mv_y = cu->mvy;
        for (int q = 0; q < t.n_leaf; ++q) {
            const struct TUInfo *ti = &t.tu[t.leaf[q].slot];
            ovhip_tu_desc tu;
            memset(&tu, 0, sizeof(tu));
            tu.x0 = cu->x0 + t.leaf[q].x; tu.y0 = cu->y0 + t.leaf[q].y; tu.log2_tb_w = t.lw; tu.log2_tb_h = t.lh; tu.tree = cu->chroma ? 0 : 1;
            tu.cbf_mask = cu->chroma ? ti->cbf_mask : (ti->cbf_mask ? 0x10 : 0); tu.cu_flags = flg_ibc_flag; tu.tr_skip_mask = ti->tr_skip_mask;
            for (int k = 0; k < 3; ++k) { tu.last_pos[k] = ti->tb_info[k].last_pos; tu.sig_sb_map[k] = ti->tb_info[k].sig_sb_map; }
            tu.coef[0] = cd->residual_cb + ti->pos_offset; tu.coef[1] = cd->residual_cr + ti->pos_offset; tu.coef[2] = cd->residual_y + ti->pos_offset;
            if (ovhip_rec_tu_ibc(direct, &st, &tu, &d) < 0) { fprintf(stderr, "shim mode: %s: direct recording of CU %d failed: %s\n", s->name, i, ovhip_rec_refusal(direct)); return 1; }
        }
    }
    size_t na, nb, ta, tb, ca, cb_;
    const ovhip_itask *ia = ovhip_rec_itasks(shim, &na), *ib = ovhip_rec_itasks(direct, &nb);
    const ovhip_tb_cmd *xa = ovhip_rec_tb_cmds(shim, &ta), *xb = ovhip_rec_tb_cmds(direct, &tb);
    const int16_t *ka = ovhip_rec_coefs(shim, &ca), *kb = ovhip_rec_coefs(direct, &cb_);
    if (!na || na != nb || ta != tb || ca != cb_ || memcmp(ia, ib, na * sizeof(*ia)) || memcmp(xa, xb, ta * sizeof(*xa)) || memcmp(ka, kb, ca * 2)) {
        fprintf(stderr, "shim mode: %s: the slots recorded %zu tasks / %zu commands / %zu coefficients, the direct calls %zu / %zu / %zu%s\n", s->name, na, ta, ca,
                nb, tb, cb_, na == nb && ta == tb && ca == cb_ ? " (bytes differ)" : "");
        return 1;
    }
    fprintf(stderr, "ibc shim mode: %s: %zu tasks, %zu commands: the slots' recording equals the direct one\n", s->name, na, ta);
    return 0;
}
#endif

int
main(int argc, char **argv)
{
    const char *dir = argc > 1 ? argv[1] : "tests/golden/ibc";
    static struct scen A = { "a", 512, 128, 7, 5 }, B = { "b", 512, 256, 7, 5 }, C = { "c", 640, 64, 6, 5 };
    g_seed = 0x1bc;
    build_row(&A, 0);
    build_row(&B, 0); build_row(&B, 128);
    /* c: CTU 64, ring of eight.  The far vectors first (they need background that nothing else takes) */
    add(&C, 576, 0, 4, 5, -88, 0, 1, RES_TS);                 /* CTU 9: source across the ring's end (picture column 512) */
    add(&C, 592, 32, 3, 3, -83, -5, 1, RES_DC);               /* ... with an odd vector */
    add(&C, 512, 0, 6, 6, -448, 0, 1, RES_MIXED);             /* CTU 8: a whole CTU from seven CTUs left */
    add(&C, 448, 0, 4, 5, -441, 7, 1, RES_TS);                /* CTU 7: from CTU 0, odd */
    add(&C, 608, 0, 4, 5, -416, 3, 1, RES_NONE);              /* CTU 9: from CTU 3, six left */
    for (int cx = 1; cx < 10; ++cx) if (cx != 8) add_random(&C, cx, 0, 10, 4);
    sort_by_ctu(&A); sort_by_ctu(&B); sort_by_ctu(&C);
    struct scen *all[3] = { &A, &B, &C };
#ifdef WITH_SHIM
    (void)dir;
    for (int k = 0; k < 3; ++k) if (shim_compare(all[k])) return 1;
    return 0;
#else
    gfile g = gfile_open(dir, "ibc.ovg"), g_rows = gfile_open(dir, "ibc_rows.ovg");
    for (int k = 0; k < 3; ++k) {
        struct scen *s = all[k];
        gfile *out = k == 1 ? &g_rows : &g;
        g_part.log2_ctu_s = (uint8_t)s->l2c;
        OVCTUDec *c = ref_new_ctudec(0, 0);
        ovhip_tu_state st;
        set_state(c, &st);
        const size_t ny = (size_t)s->w * s->h, nc = ny / 4;
        uint16_t *bg[3] = { malloc(ny * 2), malloc(nc * 2), malloc(nc * 2) }, *f0[3], *f1[3];
        for (int p = 0; p < 3; ++p) { f0[p] = calloc(p ? nc : ny, 2); f1[p] = calloc(p ? nc : ny, 2); }
        g_seed = 0x1bc + 77 * (uint32_t)k;
        fill_plane(bg[0], s->w, s->h, s->w); fill_plane(bg[1], s->w / 2, s->h / 2, s->w / 2); fill_plane(bg[2], s->w / 2, s->h / 2, s->w / 2);
        gbuf recs = { .type = T_I32 }, maps = { .type = T_U64 }, coefs = { .type = T_I16 }, first = { .type = T_U32 };
        run_scenario(c, s, bg, f0, 0xAB, &recs, &maps, &coefs, &first);
        run_scenario(c, s, bg, f1, 0x5C, NULL, NULL, NULL, NULL);
        for (int p = 0; p < 3; ++p)
            if (memcmp(f0[p], f1[p], (p ? nc : ny) * 2)) { fprintf(stderr, "%s: plane %d depends on memory nothing wrote -- not written\n", s->name, p); return 1; }
        /* outside the CUs the frame is the background */
        int32_t *cus = calloc((size_t)s->n * 8, 4);
        for (int i = 0; i < s->n; ++i) {
            const struct cu *cu = &s->cu[i];
            const int32_t r[8] = { cu->x0, cu->y0, cu->l2w, cu->l2h, cu->mvx, cu->mvy, cu->chroma, (int32_t)((uint32_t *)first.data)[i] };
            memcpy(cus + 8 * i, r, sizeof(r));
        }
        const uint32_t dims[4] = { (uint32_t)s->w, (uint32_t)s->h, (uint32_t)s->l2c, (uint32_t)s->max_tb };
        named(out, s, "dims", T_U32, dims, 1, 4, 1);
        static const char *const pn[3] = { "y", "cb", "cr" };
        for (int p = 0; p < 3; ++p) {
            char nm[16];
            snprintf(nm, sizeof(nm), "bg_%s", pn[p]); named(out, s, nm, T_U16, bg[p], 2, s->h >> !!p, s->w >> !!p);
            snprintf(nm, sizeof(nm), "exp_%s", pn[p]); named(out, s, nm, T_U16, f0[p], 2, s->h >> !!p, s->w >> !!p);
        }
        named(out, s, "cu", T_I32, cus, 2, s->n, 8);
        named(out, s, "tu", T_I32, recs.data, 2, (uint32_t)(recs.n / 14), 14);
        named(out, s, "map", T_U64, maps.data, 2, (uint32_t)(maps.n / 3), 3);
        named(out, s, "coef", T_I16, coefs.data ? coefs.data : (void *)"", 1, (uint32_t)coefs.n, 1);
        named(out, s, "state", T_U8, &st, 1, sizeof(st), 1);
        fprintf(stderr, "ibc scenario %s: %dx%d, CTU %d, %d CUs, %zu TUs, %zu coefficients\n", s->name, s->w, s->h, 1 << s->l2c, s->n, recs.n / 14, coefs.n);
    }
    gfile_close(&g); gfile_close(&g_rows);
    return 0;
#endif
}
