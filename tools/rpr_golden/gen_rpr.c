/* gen_rpr.c -- TEST INFRASTRUCTURE (run where the reference sources are present; not part of build()).
 *
 * Writes tests/golden/rpr/rpr.ovg: what the reference's own slots rcn_mcp_b (rcn_inter.c:2769-2813) and rcn_gpm_b (:3118-3143)
 * predict when the reference pictures have another size than the picture (scale_fact_rpl0 / rpl1 != 1 << 14): the RPR paths
 * rcn_mcp_rpr_* / rcn_mc_rpr_b_* with their mixed scaled / unscaled bi-prediction, BCW, identical motion, GPM.  Links the
 * compiled reference (oracle/_ref/libovvcref.so, built by `make -C oracle`) and the fake decoder state of
 * oracle/ref_harness/ref_common.h.  Every case runs twice, with the reference's scratch buffers (tmp_rpr, tmp_buff, the
 * bi-prediction intermediates) poisoned with two different values; a case whose outputs differ reads memory nothing wrote and
 * is not pinned.  PUs whose 2:1 footprint would not fit the reference's tmp_rpr are not generated.
 */
#include "../../oracle/ref_harness/ref_common.h"
#include "ovvc_hip.h"

extern void rcn_init_gpm_params(void);

#define PW 128
#define PH 96
#define NSLOT 6

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

/* one slot call; returns the outputs (luma, cb, cr of the PU) appended to out */
static void
run_case(OVCTUDec *c, const ovhip_pu_desc *d, int x0, int y0, gbuf *out)
{
    struct InterDRVCtx *ic = &c->drv_ctx.inter_ctx;
    const struct OVBuffInfo *cb = &c->rcn_ctx.ctu_buff;
    OVMV mv0 = { .x = d->mv0x, .y = d->mv0y, .ref_idx = d->ref_idx0, .bcw_idx_plus1 = d->bcw_idx_plus1 };
    OVMV mv1 = { .x = d->mv1x, .y = d->mv1y, .ref_idx = d->ref_idx1, .bcw_idx_plus1 = d->bcw_idx_plus1 };
    if (d->refine & OVHIP_PU_GPM) {
        struct VVCGPM *g = &ic->gpm_ctx;
        g->mv0 = mv0; g->mv1 = mv1; g->inter_dir0 = 1; g->inter_dir1 = 2; g->split_dir = d->gpm_split_dir;
        c->rcn_funcs.rcn_gpm_b(c, g, x0, y0, d->log2_w, d->log2_h);
    } else {
        c->rcn_funcs.rcn_mcp_b(c, *cb, ic, c->part_ctx, mv0, mv1, x0, y0, d->log2_w, d->log2_h, d->inter_dir, d->ref_idx0, d->ref_idx1);
    }
    const int w = 1 << d->log2_w, h = 1 << d->log2_h;
    dump_rect(out, cb->y, cb->stride, x0, y0, w, h);
    dump_rect(out, cb->cb, cb->stride_c, x0 >> 1, y0 >> 1, w >> 1, h >> 1);
    dump_rect(out, cb->cr, cb->stride_c, x0 >> 1, y0 >> 1, w >> 1, h >> 1);
}

int
main(int argc, char **argv)
{
    const char *dir = argc > 1 ? argv[1] : "tests/golden";
    g_seed = 0x5250;
    rcn_init_gpm_params();
    OVCTUDec *c = ref_new_ctudec(0, 0);
    struct InterDRVCtx *ic = &c->drv_ctx.inter_ctx;
    /* slots: 2, just above 7/4, 3/2, 5/4 + one step, 2/3, 1/8 ... (each slot one reference size); rpl0[i] = slot i,
     * rpl1[i] = slot (NSLOT - 1 - i); a seventh, unscaled picture sits at rpl0[6] / rpl1[6] for mixed bi-prediction */
    static const int sizes[NSLOT + 1][2] = { { 256, 192 }, { 226, 170 }, { 192, 144 }, { 162, 122 }, { 86, 64 }, { 16, 12 }, { PW, PH } };
    OVPicture *ref[NSLOT + 1];
    for (int i = 0; i <= NSLOT; ++i) {
        ref[i] = ref_new_picture(sizes[i][0], sizes[i][1], 4 * (i + 1));
        fill_plane(ref[i]->frame->data[0], sizes[i][0], sizes[i][1], sizes[i][0]);
        fill_plane(ref[i]->frame->data[1], sizes[i][0] / 2, sizes[i][1] / 2, sizes[i][0] / 2);
        fill_plane(ref[i]->frame->data[2], sizes[i][0] / 2, sizes[i][1] / 2, sizes[i][0] / 2);
    }
    int slot0[NSLOT + 1], slot1[NSLOT + 1];
    for (int i = 0; i <= NSLOT; ++i) {
        slot0[i] = i; slot1[i] = i == NSLOT ? NSLOT : NSLOT - 1 - i;
        ic->rpl0[i] = ref[slot0[i]]; ic->rpl1[i] = ref[slot1[i]];
        /* ctudec_compute_refs_scaling (ctudec.c:43-86) with the scaling windows equal to the pictures */
        for (int l = 0; l < 2; ++l) {
            const int s = l ? slot1[i] : slot0[i];
            uint16_t *f = l ? ic->scale_fact_rpl1[i] : ic->scale_fact_rpl0[i];
            f[0] = (uint16_t)(((sizes[s][0] << 14) + PW / 2) / PW);
            f[1] = (uint16_t)(((sizes[s][1] << 14) + PH / 2) / PH);
        }
    }
    /* a PU of the largest size at 2:1 must fit tmp_rpr: (2 h + 8 + 3) rows of 2 * RCN_CTB_STRIDE */
    const size_t rpr_elems = sizeof(c->rcn_ctx.data.tmp_rpr) / 2;
    const size_t rpr_stride = 2 * RCN_CTB_STRIDE;

    gbuf b_desc = { .type = T_U8 }, b_eoff = { .type = T_U32 }, b_exp = { .type = T_U16 }, b_col = { .type = T_U8 };
    uint32_t n_cases = 0, n_dropped = 0;
    for (int l2w = 3; l2w <= 6; ++l2w) {
        for (int l2h = 3; l2h <= 6; ++l2h) {
            const int w = 1 << l2w, h = 1 << l2h;
            if ((size_t)(2 * h + 11) * rpr_stride > rpr_elems || (size_t)(2 * w + 11) > rpr_stride) continue;
            const int reps = w * h <= 256 ? 14 : (w * h <= 1024 ? 6 : 2);
            for (int rep = 0; rep < reps; ++rep) {
                ovhip_pu_desc d;
                memset(&d, 0, sizeof(d));
                int px, py;
                do {
                    px = rnd_range(0, (PW - w) / 8) * 8;
                    py = rnd_range(0, (PH - h) / 8) * 8;
                } while ((px >> 7) != ((px + w - 1) >> 7) || (py >> 7) != ((py + h - 1) >> 7));
                d.x0 = px; d.y0 = py; d.log2_w = l2w; d.log2_h = l2h;
                d.inter_dir = rnd_range(1, 3);
                d.ref_idx0 = rnd_range(0, NSLOT); d.ref_idx1 = rnd_range(0, NSLOT);
                const int range = rep % 4 == 0 ? 40000 : (rep % 4 == 1 ? 64 : 900);   /* far outside (clip_rpr_position) / tiny / normal */
                d.mv0x = rnd_range(-range, range); d.mv0y = rnd_range(-range, range);
                d.mv1x = rnd_range(-range, range); d.mv1y = rnd_range(-range, range);
                if (rep % 7 == 3) { d.mv0x &= ~15; d.mv1y &= ~15; }
                if (rep % 9 == 4) { d.inter_dir = 3; d.ref_idx1 = (uint8_t)(NSLOT - 1 - d.ref_idx0 < 0 ? 0 : d.ref_idx0); d.mv1x = d.mv0x; d.mv1y = d.mv0y; }
                d.bcw_idx_plus1 = (rep % 3 == 1) ? rnd_range(1, 5) : 0;
                d.prec_amvr_half = rep % 5 == 2;
                if (d.prec_amvr_half) { d.mv0x = (d.mv0x & ~15) | 8; d.mv1y = (d.mv1y & ~15) | 8; }
                d.planes = 3;
                if (rep % 6 == 5 && l2w <= 6 && l2h <= 6) {          /* GPM: list 0 side from rpl0, list 1 side from rpl1 */
                    d.refine = OVHIP_PU_GPM; d.inter_dir = 3; d.bcw_idx_plus1 = 0; d.gpm_split_dir = (uint8_t)rnd_range(0, 63);
                }
                d.poc0 = ic->rpl0[d.ref_idx0]->poc; d.poc1 = ic->rpl1[d.ref_idx1]->poc;
                d.ref0 = (uint8_t)slot0[d.ref_idx0]; d.ref1 = (uint8_t)slot1[d.ref_idx1];
                const int s0 = ic->scale_fact_rpl0[d.ref_idx0][0] != 1 << 14 || ic->scale_fact_rpl0[d.ref_idx0][1] != 1 << 14;
                const int s1 = ic->scale_fact_rpl1[d.ref_idx1][0] != 1 << 14 || ic->scale_fact_rpl1[d.ref_idx1][1] != 1 << 14;
                if (!s0 && !s1) continue;
                /* chroma collocation flags (SPS-level: every picture the same) */
                uint8_t col[2] = { (uint8_t)(rep & 1), (uint8_t)((rep >> 1) & 1) };
                for (int i = 0; i <= NSLOT; ++i) { ref[i]->scale_info.chroma_hor_col_flag = col[0]; ref[i]->scale_info.chroma_ver_col_flag = col[1]; }
                c->ctb_x = px >> 7; c->ctb_y = py >> 7;
                ic->prec_amvr = d.prec_amvr_half ? MV_PRECISION_HALF : 0;
                gbuf a = { .type = T_U16 }, b = { .type = T_U16 };
                poison(c, 0xAB); run_case(c, &d, px & 127, py & 127, &a);
                poison(c, 0x5C); run_case(c, &d, px & 127, py & 127, &b);
                const int stable = a.n == b.n && !memcmp(a.data, b.data, a.n * 2);
                if (stable) {
                    uint32_t off = (uint32_t)b_exp.n;
                    gbuf_push(&b_exp, a.data, a.n);
                    gbuf_push(&b_desc, &d, sizeof(d));
                    gbuf_push(&b_eoff, &off, 1);
                    gbuf_push(&b_col, col, 2);
                    n_cases++;
                } else n_dropped++;
                free(a.data); free(b.data);
            }
        }
    }
    gfile g = gfile_open(dir, "rpr.ovg");
    uint32_t sz[NSLOT + 1][2];
    for (int i = 0; i <= NSLOT; ++i) {
        char name[32];
        uint32_t d2[2] = { (uint32_t)sizes[i][1], (uint32_t)sizes[i][0] };
        sz[i][0] = (uint32_t)sizes[i][0]; sz[i][1] = (uint32_t)sizes[i][1];
        snprintf(name, sizeof(name), "ref%d_y", i); gfile_array(&g, name, T_U16, ref[i]->frame->data[0], 2, d2);
        d2[0] /= 2; d2[1] /= 2;
        snprintf(name, sizeof(name), "ref%d_cb", i); gfile_array(&g, name, T_U16, ref[i]->frame->data[1], 2, d2);
        snprintf(name, sizeof(name), "ref%d_cr", i); gfile_array(&g, name, T_U16, ref[i]->frame->data[2], 2, d2);
    }
    uint32_t dpic[1] = { 2 }, pic[2] = { PW, PH };
    gfile_array(&g, "pic", T_U32, pic, 1, dpic);
    uint32_t ds[2] = { NSLOT + 1, 2 };
    gfile_array(&g, "ref_size", T_U32, sz, 2, ds);
    uint32_t d2[2] = { n_cases, sizeof(ovhip_pu_desc) };
    gfile_array(&g, "desc", T_U8, b_desc.data, 2, d2);
    d2[1] = 2; gfile_array(&g, "col", T_U8, b_col.data, 2, d2);
    uint32_t d1[1] = { n_cases };
    gfile_array(&g, "exp_off", T_U32, b_eoff.data, 1, d1);
    gfile_buf(&g, "exp", &b_exp);
    gfile_close(&g);
    fprintf(stderr, "rpr.ovg: %u cases (%u dropped: output depends on unwritten scratch), %zu expected samples\n", n_cases, n_dropped, b_exp.n);
    return 0;
}
