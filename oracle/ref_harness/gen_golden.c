/* gen_golden.c -- TEST INFRASTRUCTURE (this container only).
 *
 * Drives the COMPILED REFERENCE (oracle/_ref/libovvcref.so, built from /root/reference where it
 * lies) through its own orchestrator slots on seeded inputs and writes small golden fixtures
 * to tests/golden/*.ovg.  The inputs are stored in the vocabulary of include/ovvc_hip.h
 * (ovhip_tu_state / ovhip_tu_desc / ovhip_pu_desc = what the slots receive), the expected
 * outputs are the bytes the reference produced.  Nothing from the reference is copied; the
 * reference does not travel to the GPU box, the fixtures do.
 *
 *   itx.ovg : tmp.rcn_tu_st / tmp.rcn_tu_c  (rcn_transform_tree.c:1228-1382)  -> K1..K4
 *   mc.ovg  : rcn_mcp_b / rcn_mcp_b_l / rcn_mcp_b_c (rcn_inter.c:2769-2966)   -> K5, K6, K11
 */
#include "ref_common.h"
#include "ovvc_hip.h"
#include "shim_stream.h"
#include <time.h>

/* "time" mode: seconds spent inside the reference's slots per stage (profiles/cpu_calibration.json: the oracle port is timed on
 * the same cases from Python, tools/cpu_calibration.py) */
enum { TS_ITX, TS_MC, TS_MCX, TS_MCA, TS_DBF, TS_SAO, TS_ALF, TS_INTRA, TS_N };
static const char *g_ts_name[TS_N] = { "itx", "mc", "mcx", "mca", "dbf", "sao", "alf", "intra" };
static double g_ts[TS_N];
static int g_time;
static inline double now_s(void) { struct timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return ts.tv_sec + ts.tv_nsec * 1e-9; }
#define TIMED(k, stmt) do { if (g_time) { const double t0_ = now_s(); stmt; g_ts[k] += now_s() - t0_; } else { stmt; } } while (0)

/* struct TUInfo is private to rcn_transform_tree.c:51-66 (and duplicated in
 * vcl_transform_unit.c:47-75); the slot signature only forward-declares it. */
struct TBInfo { uint16_t last_pos; uint64_t sig_sb_map; };
struct TUInfo {
    uint8_t is_sbt; uint8_t cbf_mask; uint16_t pos_offset; uint8_t tr_skip_mask;
    uint8_t cu_mts_flag; uint8_t cu_mts_idx; uint8_t lfnst_flag; uint8_t lfnst_idx;
    struct TBInfo tb_info[3];
};

extern uint64_t residual_coding_dpq(OVCTUDec *const, int16_t *const, uint8_t, uint8_t, uint16_t);

static void stub_intra_pred_c(const struct OVRCNCtx *const r, uint8_t m, int x0, int y0, int lw, int lh, CUFlags f)
{ (void)r; (void)m; (void)x0; (void)y0; (void)lw; (void)lh; (void)f; }

static int16_t rnd_coef(void)
{
    int k = rnd_range(0, 15);
    if (k < 9)  return (int16_t)rnd_range(-24, 24);
    if (k < 13) return (int16_t)rnd_range(-900, 900);
    if (k < 15) return (int16_t)rnd_range(-32768, 32767);
    return (int16_t)(rnd_range(0, 1) ? 32767 : -32768);
}

/* fill one TB worth of coefficients in the reference layout; returns number of int16 used */
static int
make_coefs(int16_t *dst, int log2_w, int log2_h, int pattern, int raster, uint64_t *map, uint16_t *last_pos)
{
    int w = 1 << log2_w, h = 1 << log2_h;
    if (raster) {
        int n = w * h;
        memset(dst, 0, n * 2);
        if (pattern == 0) { dst[0] = rnd_coef(); *last_pos = 0; }
        else { for (int i = 0; i < n; ++i) if (pattern == 2 || rnd_range(0, 2) == 0) dst[i] = rnd_coef(); *last_pos = 0x0101; }
        *map = 1;
        return n;
    }
    int cw = w > 32 ? 32 : w, ch = h > 32 ? 32 : h;
    int nx = cw / 4, ny = ch / 4;
    memset(dst, 0, cw * ch * 2);
    *map = 0;
    if (pattern == 0) {
        dst[0] = rnd_coef();
        if (!dst[0]) dst[0] = 7;
        *last_pos = 0;
        *map = rnd_range(0, 1);
        return cw * ch;
    }
    int lim_x = pattern == 2 ? nx : rnd_range(1, nx), lim_y = pattern == 2 ? ny : rnd_range(1, ny);
    for (int sy = 0; sy < lim_y; ++sy) {
        for (int sx = 0; sx < lim_x; ++sx) {
            if (pattern != 2 && (sx || sy) && rnd_range(0, 2) == 0) continue;
            *map |= 1ull << (sy * 8 + sx);
            int16_t *sb = dst + sy * 4 * cw + sx * 16;
            for (int i = 0; i < 16; ++i) sb[i] = (pattern == 2 || rnd_range(0, 1)) ? rnd_coef() : 0;
        }
    }
    *last_pos = 0x0302;
    return cw * ch;
}

static void
dump_rect(gbuf *exp, const uint16_t *p, int stride, int x, int y, int w, int h)
{
    for (int j = 0; j < h; ++j) gbuf_push(exp, p + (y + j) * stride + x, w);
}

/* derive_lfnst_mode_c (drv_lfnst.c:94-121) reads CTU-local luma mode maps; the shim performs
 * this lookup at record time.  For the fixtures the chroma mode is an explicit angular mode. */
static int shim_lfnst_mode_c(int log2_w, int log2_h, int mode)
{
    static const uint8_t ms_lut[6] = { 0, 6, 10, 12, 14, 15 };
    if (mode > 1) {
        int d = log2_w - log2_h; int ms = ms_lut[d < 0 ? -d : d];
        if (log2_w > log2_h && mode < 2 + ms) mode += 65;
        else if (log2_h > log2_w && mode > 66 - ms) mode -= 67;
    }
    return mode < 0 ? mode + 14 + 67 : mode >= 67 ? mode + 14 : mode;
}

/* TUInfo slots tmp.rcn_transform_tree visits for a CU (index arithmetic of rcn_transform_tree.c:1454-1506) */
static void
tt_slots(int l2w, int l2h, int max_tb, int depth, int base, int *out, int *n)
{
    int sv = l2w > max_tb, sh = l2h > max_tb, nsub = depth ? 1 : (1 << (sv + sh));
    if (l2w > 6 && l2h < 7) { tt_slots(6, l2h, max_tb, depth + 1, base, out, n); tt_slots(6, l2h, max_tb, depth + 1, base + 8, out, n); return; }
    if (l2h > 6 && l2w < 7) { tt_slots(l2w, 6, max_tb, depth + 1, base, out, n); tt_slots(l2w, 6, max_tb, depth + 1, base + 8, out, n); return; }
    if (sv || sh) {
        tt_slots(l2w - sv, l2h - sh, max_tb, depth + 1, base, out, n);
        if (sv) tt_slots(l2w - sv, l2h - sh, max_tb, depth + 1, base + nsub, out, n);
        if (sh) tt_slots(l2w - sv, l2h - sh, max_tb, depth + 1, base + 2 * nsub, out, n);
        if (sv && sh) tt_slots(l2w - sv, l2h - sh, max_tb, depth + 1, base + 3 * nsub, out, n);
        return;
    }
    out[(*n)++] = base;
}

/* what gen_itx and gen_itx_cells share: the prediction picture, the decoder state of one case, the CTU buffer before a case */
static void
itx_fill_pred(uint16_t *pred_y, uint16_t *pred_cb, uint16_t *pred_cr)
{
    fill_plane(pred_y, 128, 128, 128);
    fill_plane(pred_cb, 64, 64, 64);
    fill_plane(pred_cr, 64, 64, 64);
    /* make clipping at both ends reachable */
    for (int i = 0; i < 128 * 128; i += 37) pred_y[i] = (i & 1) ? 1023 : 0;
    for (int i = 0; i < 64 * 64; i += 29) { pred_cb[i] = (i & 1) ? 1023 : 0; pred_cr[i] = (i & 1) ? 0 : 1023; }
}

static void
itx_set_state(OVCTUDec *c, const ovhip_tu_state *st, int c_mode)
{
    c->dequant_luma.qp = st->qp_y; c->dequant_cb.qp = st->qp_cb; c->dequant_cr.qp = st->qp_cr;
    c->dequant_joint_cb_cr.qp = st->qp_jcbcr;
    c->dequant_luma_skip.qp = st->qp_y_skip; c->dequant_cb_skip.qp = st->qp_cb_skip;
    c->dequant_cr_skip.qp = st->qp_cr_skip; c->dequant_jcbcr_skip.qp = st->qp_jcbcr_skip;
    c->residual_coding_l = st->dep_quant ? &residual_coding_dpq : NULL;
    c->mts_implicit = st->mts_implicit;
    c->sh_ts_disabled = st->sh_ts_disabled;
    c->lmcs_info.scale_c_flag = st->lmcs_scale_c;
    c->lmcs_info.lmcs_chroma_scale = (uint16_t)st->lmcs_chroma_scale;
    c->intra_mode = (uint8_t)st->intra_mode;
    c->intra_mode_c = (uint8_t)c_mode;
    c->qp_ctx.qp_bd_offset = 12;
}

static void
itx_load_pred(OVCTUDec *c, const uint16_t *pred_y, const uint16_t *pred_cb, const uint16_t *pred_cr)
{
    const struct OVBuffInfo *cb = &c->rcn_ctx.ctu_buff;
    for (int j = 0; j < 128; ++j) memcpy(cb->y + j * cb->stride, pred_y + j * 128, 256);
    for (int j = 0; j < 64; ++j) {
        memcpy(cb->cb + j * cb->stride_c, pred_cb + j * 64, 128);
        memcpy(cb->cr + j * cb->stride_c, pred_cr + j * 64, 128);
    }
    memset(&c->dbf_info, 0, sizeof(c->dbf_info));
}

static void
gen_itx(const char *dir)
{
    static uint16_t pred_y[128 * 128], pred_cb[64 * 64], pred_cr[64 * 64];
    gbuf b_state = { .type = T_U8 }, b_desc = { .type = T_U8 }, b_coff = { .type = T_U32 }, b_clen = { .type = T_U32 };
    gbuf b_coefs = { .type = T_I16 }, b_eoff = { .type = T_U32 }, b_exp = { .type = T_U16 };
    uint32_t n_cases = 0;
    g_seed = 0x266;

    itx_fill_pred(pred_y, pred_cb, pred_cr);

    OVCTUDec *c = ref_new_ctudec(0, 0);
    c->rcn_funcs.intra_pred_c = stub_intra_pred_c;
    const struct OVBuffInfo *cb = &c->rcn_ctx.ctu_buff;
    struct shim_stream S, ST;
    shim_stream_init(&S); shim_stream_init(&ST);
    if (g_shim) shim_bind(c, 128, 128, 0, 0);

    for (int tree = 0; tree <= 2; tree += 2) {
        int lmin = tree ? 1 : 2, lmax = tree ? 5 : 6;
        for (int l2w = lmin; l2w <= lmax; ++l2w) {
            for (int l2h = lmin; l2h <= lmax; ++l2h) {
                int reps = tree ? 5 : 12;
                for (int rep = 0; rep < reps; ++rep) {
                    ovhip_tu_state st; ovhip_tu_desc d; struct TUInfo tu;
                    memset(&st, 0, sizeof(st)); memset(&d, 0, sizeof(d)); memset(&tu, 0, sizeof(tu));
                    int w = 1 << l2w, h = 1 << l2h;
                    int unit = tree ? 2 : 4;
                    int x0 = rnd_range(0, ((tree ? 64 : 128) - w) / unit) * unit;
                    int y0 = rnd_range(0, ((tree ? 64 : 128) - h) / unit) * unit;
                    /* chroma TB size seen by the chroma path */
                    int cl2w = tree ? l2w : l2w - 1, cl2h = tree ? l2h : l2h - 1;

                    st.qp_y = rnd_range(0, 75); st.qp_cb = rnd_range(0, 75); st.qp_cr = rnd_range(0, 75); st.qp_jcbcr = rnd_range(0, 75);
                    st.qp_y_skip = st.qp_y < 16 ? 16 : st.qp_y; st.qp_cb_skip = st.qp_cb < 16 ? 16 : st.qp_cb;
                    st.qp_cr_skip = st.qp_cr < 16 ? 16 : st.qp_cr; st.qp_jcbcr_skip = st.qp_jcbcr < 16 ? 16 : st.qp_jcbcr;
                    st.dep_quant = rnd_range(0, 1);
                    st.mts_implicit = rnd_range(0, 1);
                    st.sh_ts_disabled = rnd_range(0, 1);
                    st.ict_type = rnd_range(0, 3);
                    st.lmcs_scale_c = rnd_range(0, 1);
                    st.lmcs_chroma_scale = (int16_t)rnd_range(1200, 3400);
                    st.intra_mode = (int8_t)rnd_range(0, 66);

                    d.x0 = x0; d.y0 = y0; d.log2_tb_w = l2w; d.log2_tb_h = l2h; d.tree = tree;

                    int variant = rep % 6;   /* 0 inter dct2, 1 implicit MTS intra, 2 explicit MTS, 3 LFNST, 4 TS, 5 inter */
                    int max_l2 = l2w > l2h ? l2w : l2h;
                    if (variant == 2 && (max_l2 > 5 || tree)) variant = 0;
                    if (variant == 4 && max_l2 > 5) variant = 5;
                    if (variant == 3 && tree && (l2w < 2 || l2h < 2)) variant = 0;
                    if (variant == 1 || variant == 3) d.cu_flags |= 1u << 1;                  /* pred_mode_flag (intra) */
                    if (variant == 2) { d.cu_mts_flag = 1; d.cu_mts_idx = rnd_range(0, 3); d.cu_flags |= (rnd_range(0, 1) << 1); }
                    if (variant == 3) { d.lfnst_flag = 1; d.lfnst_idx = rnd_range(0, 1); }

                    static const uint8_t cbf_st[8] = { 0x10, 0x12, 0x11, 0x13, 0x1b, 0x1a, 0x19, 0x0b };
                    static const uint8_t cbf_c[6] = { 0x2, 0x1, 0x3, 0xb, 0xa, 0x9 };
                    d.cbf_mask = tree ? cbf_c[rnd_range(0, 5)] : cbf_st[rnd_range(0, 7)];
                    if (!tree && l2w + l2h < 6) d.cbf_mask &= 0x10;          /* no 2x2 / 2x4 chroma TBs in single tree */
                    if (!d.cbf_mask) d.cbf_mask = 0x10;
                    if (variant == 4) {
                        d.tr_skip_mask = 0;
                        if (d.cbf_mask & 0x10) d.tr_skip_mask |= 0x10;
                        if (rnd_range(0, 1)) d.tr_skip_mask |= 0x3;
                        if (rep >= 6 || (tree && rnd_range(0, 1))) {
                            /* block DPCM (intra CUs): transform skip is implied, direction random */
                            d.cu_flags |= 1u << 1;
                            if (d.tr_skip_mask & 0x10) d.cu_flags |= (1u << 8) | ((uint32_t)rnd_range(0, 1) << 10);
                            if (d.tr_skip_mask & 0x3)  d.cu_flags |= (1u << 9) | ((uint32_t)rnd_range(0, 1) << 11);
                        }
                    }

                    /* chroma LFNST only exists in the dual-tree chroma path */
                    int c_mode = rnd_range(0, 66);
                    st.lfnst_mode_c = (int8_t)shim_lfnst_mode_c(cl2w, cl2h, c_mode);

                    /* ---- coefficients ---- */
                    int16_t *res[3] = { c->residual_cb, c->residual_cr, c->residual_y };
                    uint32_t off3[3] = { 0, 0, 0 }, len3[3] = { 0, 0, 0 };
                    int pos_offset = rnd_range(0, 3) * 16;
                    for (int comp = 0; comp < 3; ++comp) {
                        int is_l = comp == 2;
                        int used = is_l ? (d.cbf_mask & 0x10) && tree != 2
                                        : (tree != 1) && ((d.cbf_mask & 0x8) ? comp == 0 : (d.cbf_mask & (comp ? 0x1 : 0x2)));
                        if (!used) continue;
                        int tl2w = is_l ? l2w : cl2w, tl2h = is_l ? l2h : cl2h;
                        int ts = is_l ? !!(d.tr_skip_mask & 0x10)
                                      : (d.cbf_mask & 0x8) ? !!(d.tr_skip_mask & 0x1) : !!(d.tr_skip_mask & (comp ? 0x1 : 0x2));
                        int raster = (ts && !st.sh_ts_disabled) || tl2w < 2 || tl2h < 2;
                        int pattern = variant == 3 ? 1 : rnd_range(0, 2);
                        uint64_t map; uint16_t lp;
                        int n = make_coefs(res[comp] + pos_offset, tl2w, tl2h, pattern, raster, &map, &lp);
                        if (variant == 3) { map = 1; lp = 0x0101; }   /* LFNST: first sub-block only */
                        if (variant == 3 && !raster) {
                            int cw = (1 << tl2w) > 32 ? 32 : (1 << tl2w), ch = (1 << tl2h) > 32 ? 32 : (1 << tl2h);
                            memset(res[comp] + pos_offset + 16, 0, (cw * ch - 16) * 2);
                        }
                        d.sig_sb_map[comp] = map; d.last_pos[comp] = lp;
                        tu.tb_info[comp].sig_sb_map = map; tu.tb_info[comp].last_pos = lp;
                        off3[comp] = (uint32_t)b_coefs.n; len3[comp] = (uint32_t)n;
                        gbuf_push(&b_coefs, res[comp] + pos_offset, n);
                    }

                    /* ---- reference state ---- */
                    rcn_init_ict_functions_10(&c->rcn_funcs, st.ict_type, 10);
                    if (g_shim) rcn_init_functions_hip(&c->rcn_funcs, st.ict_type, 1, 0, 0, 10);   /* per slice in the decoder (slicedec.c:1462) */
                    itx_set_state(c, &st, c_mode);
                    tu.cbf_mask = d.cbf_mask; tu.pos_offset = (uint16_t)pos_offset; tu.tr_skip_mask = d.tr_skip_mask;
                    tu.cu_mts_flag = d.cu_mts_flag; tu.cu_mts_idx = d.cu_mts_idx;
                    tu.lfnst_flag = d.lfnst_flag; tu.lfnst_idx = d.lfnst_idx;

                    itx_load_pred(c, pred_y, pred_cb, pred_cr);

                    if (g_shim && tree == 2 && d.lfnst_flag) {
                        /* derive_lfnst_mode_c's inputs as the decoder holds them: an explicit angular chroma mode */
                        c->part_ctx_c = &g_part;
                    }
                    if (tree == 0) TIMED(TS_ITX, c->rcn_funcs.tmp.rcn_tu_st(c, x0, y0, l2w, l2h, d.cu_flags, d.cbf_mask, &tu));
                    else           TIMED(TS_ITX, c->rcn_funcs.tmp.rcn_tu_c(c, x0, y0, l2w, l2h, d.cu_flags, d.cbf_mask, &tu));
                    if (g_shim) shim_case_end(c, &S, "itx");

                    uint32_t eoff[3] = { 0, 0, 0 };
                    if (tree == 0) {
                        eoff[0] = (uint32_t)b_exp.n; dump_rect(&b_exp, cb->y, cb->stride, x0, y0, w, h);
                        eoff[1] = (uint32_t)b_exp.n; dump_rect(&b_exp, cb->cb, cb->stride_c, x0 >> 1, y0 >> 1, w >> 1, h >> 1);
                        eoff[2] = (uint32_t)b_exp.n; dump_rect(&b_exp, cb->cr, cb->stride_c, x0 >> 1, y0 >> 1, w >> 1, h >> 1);
                    } else {
                        eoff[1] = (uint32_t)b_exp.n; dump_rect(&b_exp, cb->cb, cb->stride_c, x0, y0, w, h);
                        eoff[2] = (uint32_t)b_exp.n; dump_rect(&b_exp, cb->cr, cb->stride_c, x0, y0, w, h);
                    }
                    gbuf_push(&b_state, &st, sizeof(st));
                    gbuf_push(&b_desc, &d, sizeof(d));
                    gbuf_push(&b_coff, off3, 3); gbuf_push(&b_clen, len3, 3); gbuf_push(&b_eoff, eoff, 3);
                    n_cases++;
                }
            }
        }
    }

    /* ---- whole transform trees through tmp.rcn_transform_tree (rcn_transform_tree.c:1454-1506): inter CUs up to
     * 128x128, maximum transform size 64 or 32, one struct TUInfo per leaf as the caller lays them out ---- */
    gbuf t_state = { .type = T_U8 }, t_desc = { .type = T_U8 }, t_info = { .type = T_U8 }, t_coef = { .type = T_I16 };
    gbuf t_coff = { .type = T_U32 }, t_eoff = { .type = T_U32 };
    uint32_t n_tt = 0;
    {
        extern int transform_unit_st(OVCTUDec *const, unsigned int, unsigned int, unsigned int, unsigned int, uint8_t, CUFlags, uint8_t, struct TUInfo *const);
        c->transform_unit = (void *)&transform_unit_st;
        static const uint8_t shapes[][3] = { {6,6,6}, {7,6,6}, {6,7,6}, {7,7,6}, {7,5,6}, {5,7,6}, {6,6,5}, {6,5,5}, {7,7,5}, {5,5,6}, {7,4,6}, {6,6,6} };
        for (unsigned sc = 0; sc < sizeof(shapes) / 3; ++sc) {
            const int l2w = shapes[sc][0], l2h = shapes[sc][1], max_tb = shapes[sc][2];
            ovhip_tu_state st; ovhip_tt_desc td; ovhip_tu_info ti[16]; struct TUInfo tu[16];
            memset(&st, 0, sizeof(st)); memset(&td, 0, sizeof(td)); memset(ti, 0, sizeof(ti)); memset(tu, 0, sizeof(tu));
            st.qp_y = rnd_range(20, 60); st.qp_cb = rnd_range(20, 60); st.qp_cr = rnd_range(20, 60); st.qp_jcbcr = rnd_range(20, 60);
            st.qp_y_skip = st.qp_y; st.qp_cb_skip = st.qp_cb; st.qp_cr_skip = st.qp_cr; st.qp_jcbcr_skip = st.qp_jcbcr;
            st.dep_quant = rnd_range(0, 1); st.ict_type = rnd_range(0, 3); st.lmcs_scale_c = rnd_range(0, 1);
            st.lmcs_chroma_scale = (int16_t)rnd_range(1200, 3400);
            td.x0 = 0; td.y0 = 0; td.log2_w = l2w; td.log2_h = l2h; td.log2_max_tb_s = max_tb; td.tree = 0; td.cu_flags = 0;
            memset(c->residual_y, 0, sizeof(c->residual_y)); memset(c->residual_cb, 0, sizeof(c->residual_cb)); memset(c->residual_cr, 0, sizeof(c->residual_cr));
            /* leaf geometry: what the walker will hand out, in its own visiting order per TUInfo slot */
            const int lw = l2w > max_tb ? max_tb : l2w, lh = l2h > max_tb ? max_tb : l2h;
            uint32_t used = 0;
            int slots[64], n_slots = 0;
            tt_slots(l2w, l2h, max_tb, 0, 0, slots, &n_slots);
            const uint32_t leaf_sz = (uint32_t)(1 << ((lw > 5 ? 5 : lw) + (lh > 5 ? 5 : lh)));
            for (int q = 0; q < n_slots; ++q) {
                const int k = slots[q];
                if (k > 15 || ti[k].pos_offset || tu[k].cbf_mask) continue;      /* a slot may be visited twice (depth > 1): keep the first fill */
                static const uint8_t cbfs[6] = { 0x10, 0x13, 0x1b, 0x12, 0x00, 0x11 };
                ti[k].cbf_mask = cbfs[rnd_range(0, 5)];
                ti[k].pos_offset = (uint16_t)used;
                int16_t *res[3] = { c->residual_cb, c->residual_cr, c->residual_y };
                for (int comp = 0; comp < 3; ++comp) {
                    int is_l = comp == 2;
                    int use = is_l ? (ti[k].cbf_mask & 0x10) : ((ti[k].cbf_mask & 0x8) ? comp == 0 : (ti[k].cbf_mask & (comp ? 0x1 : 0x2)));
                    if (!use) continue;
                    uint64_t map; uint16_t lp;
                    make_coefs(res[comp] + ti[k].pos_offset, is_l ? lw : lw - 1, is_l ? lh : lh - 1, rnd_range(0, 2), 0, &map, &lp);
                    ti[k].sig_sb_map[comp] = map; ti[k].last_pos[comp] = lp;
                    tu[k].tb_info[comp].sig_sb_map = map; tu[k].tb_info[comp].last_pos = lp;
                }
                tu[k].cbf_mask = ti[k].cbf_mask; tu[k].pos_offset = ti[k].pos_offset;
                used += leaf_sz;
            }
            rcn_init_ict_functions_10(&c->rcn_funcs, st.ict_type, 10);
            if (g_shim) rcn_init_functions_hip(&c->rcn_funcs, st.ict_type, 1, 0, 0, 10);
            c->dequant_luma.qp = st.qp_y; c->dequant_cb.qp = st.qp_cb; c->dequant_cr.qp = st.qp_cr; c->dequant_joint_cb_cr.qp = st.qp_jcbcr;
            c->dequant_luma_skip.qp = st.qp_y_skip; c->dequant_cb_skip.qp = st.qp_cb_skip; c->dequant_cr_skip.qp = st.qp_cr_skip; c->dequant_jcbcr_skip.qp = st.qp_jcbcr_skip;
            c->residual_coding_l = st.dep_quant ? &residual_coding_dpq : NULL;
            c->mts_implicit = 0; c->sh_ts_disabled = 0; c->tmp_ciip = 0;
            c->lmcs_info.scale_c_flag = st.lmcs_scale_c; c->lmcs_info.lmcs_chroma_scale = (uint16_t)st.lmcs_chroma_scale;
            for (int j = 0; j < 128; ++j) memcpy(cb->y + j * cb->stride, pred_y + j * 128, 256);
            for (int j = 0; j < 64; ++j) { memcpy(cb->cb + j * cb->stride_c, pred_cb + j * 64, 128); memcpy(cb->cr + j * cb->stride_c, pred_cr + j * 64, 128); }
            memset(&c->dbf_info, 0, sizeof(c->dbf_info));
            c->rcn_funcs.tmp.rcn_transform_tree(c, 0, 0, l2w, l2h, max_tb, 0, 0, tu);
            if (g_shim) shim_case_end(c, &ST, "itx tree");

            uint32_t coff = (uint32_t)t_coef.n, eoff[3];
            gbuf_push(&t_coef, c->residual_cb, used); gbuf_push(&t_coef, c->residual_cr, used); gbuf_push(&t_coef, c->residual_y, used);
            uint32_t co[2] = { coff, used };
            eoff[0] = (uint32_t)b_exp.n; dump_rect(&b_exp, cb->y, cb->stride, 0, 0, 1 << l2w, 1 << l2h);
            eoff[1] = (uint32_t)b_exp.n; dump_rect(&b_exp, cb->cb, cb->stride_c, 0, 0, 1 << (l2w - 1), 1 << (l2h - 1));
            eoff[2] = (uint32_t)b_exp.n; dump_rect(&b_exp, cb->cr, cb->stride_c, 0, 0, 1 << (l2w - 1), 1 << (l2h - 1));
            gbuf_push(&t_state, &st, sizeof(st)); gbuf_push(&t_desc, &td, sizeof(td)); gbuf_push(&t_info, ti, sizeof(ti));
            gbuf_push(&t_coff, co, 2); gbuf_push(&t_eoff, eoff, 3);
            n_tt++;
        }
    }

    if (g_shim) {
        shim_stream_write(dir, "shim_itx.ovg", &S, c, NULL, 0);
        shim_stream_write(dir, "shim_itx_tree.ovg", &ST, c, NULL, 0);
        return;
    }
    gfile g = gfile_open(dir, "itx.ovg");
    uint32_t d2[2];
    d2[0] = n_tt; d2[1] = sizeof(ovhip_tu_state); gfile_array(&g, "tt_state", T_U8, t_state.data, 2, d2);
    d2[1] = sizeof(ovhip_tt_desc);  gfile_array(&g, "tt_desc", T_U8, t_desc.data, 2, d2);
    d2[1] = 16 * sizeof(ovhip_tu_info); gfile_array(&g, "tt_info", T_U8, t_info.data, 2, d2);
    d2[1] = 2; gfile_array(&g, "tt_coef_off", T_U32, t_coff.data, 2, d2);
    d2[1] = 3; gfile_array(&g, "tt_exp_off", T_U32, t_eoff.data, 2, d2);
    gfile_buf(&g, "tt_coefs", &t_coef);
    d2[0] = 128; d2[1] = 128; gfile_array(&g, "pred_y", T_U16, pred_y, 2, d2);
    d2[0] = 64; d2[1] = 64;   gfile_array(&g, "pred_cb", T_U16, pred_cb, 2, d2);
    gfile_array(&g, "pred_cr", T_U16, pred_cr, 2, d2);
    d2[0] = n_cases; d2[1] = sizeof(ovhip_tu_state); gfile_array(&g, "state", T_U8, b_state.data, 2, d2);
    d2[1] = sizeof(ovhip_tu_desc); gfile_array(&g, "desc", T_U8, b_desc.data, 2, d2);
    d2[1] = 3; gfile_array(&g, "coef_off", T_U32, b_coff.data, 2, d2);
    gfile_array(&g, "coef_len", T_U32, b_clen.data, 2, d2);
    gfile_array(&g, "exp_off", T_U32, b_eoff.data, 2, d2);
    gfile_buf(&g, "coefs", &b_coefs);
    gfile_buf(&g, "exp", &b_exp);
    gfile_close(&g);
    fprintf(stderr, "itx.ovg: %u cases, %zu coef int16, %zu expected samples\n", n_cases, b_coefs.n, b_exp.n);
}

/* ---------------------------------------------------------------------------------------------------------------------
 * itx_cells_<family>_NN.ovg: tmp.rcn_tu_st / tmp.rcn_tu_c on ENUMERATED inputs (itx.ovg draws 12 / 5 cases per shape), on itx.ovg's
 * prediction picture and in its layout (state, desc, coef_off, coef_len, exp_off, coefs, exp), cut into files below 1 MiB.
 * A family sets up state and descriptor, writes the levels into the decoder's residual buffers at offset 0 in the reference's
 * layout, and hands the case to icells_case. */
struct icells {
    const char *dir, *family;
    int file_no;
    uint32_t n, n_total;
    gbuf state, desc, coff, clen, coefs, eoff, exp;
    OVCTUDec *c;
    uint16_t pred_y[128 * 128], pred_cb[64 * 64], pred_cr[64 * 64];
};

static void
icells_flush(struct icells *o)
{
    if (!o->n) return;
    char name[64];
    snprintf(name, sizeof(name), "itx_cells_%s_%02d.ovg", o->family, o->file_no++);
    gfile g = gfile_open(o->dir, name);
    uint32_t d2[2];
    d2[0] = 128; d2[1] = 128; gfile_array(&g, "pred_y", T_U16, o->pred_y, 2, d2);
    d2[0] = 64; d2[1] = 64;   gfile_array(&g, "pred_cb", T_U16, o->pred_cb, 2, d2);
    gfile_array(&g, "pred_cr", T_U16, o->pred_cr, 2, d2);
    d2[0] = o->n; d2[1] = sizeof(ovhip_tu_state); gfile_array(&g, "state", T_U8, o->state.data, 2, d2);
    d2[1] = sizeof(ovhip_tu_desc); gfile_array(&g, "desc", T_U8, o->desc.data, 2, d2);
    d2[1] = 3; gfile_array(&g, "coef_off", T_U32, o->coff.data, 2, d2);
    gfile_array(&g, "coef_len", T_U32, o->clen.data, 2, d2);
    gfile_array(&g, "exp_off", T_U32, o->eoff.data, 2, d2);
    gfile_buf(&g, "coefs", &o->coefs);
    gfile_buf(&g, "exp", &o->exp);
    gfile_close(&g);
    fprintf(stderr, "%s: %u cases, %zu coef int16, %zu expected samples\n", name, o->n, o->coefs.n, o->exp.n);
    o->n = 0;
    o->state.n = o->desc.n = o->coff.n = o->clen.n = o->coefs.n = o->eoff.n = o->exp.n = 0;
}

static void
icells_begin(struct icells *o, const char *family)
{
    icells_flush(o);
    o->family = family; o->file_no = 0; o->n_total = 0;
}

/* a fresh state / descriptor: mid QPs, no tool on; the block's position walks over the CTU so that the picture's samples at 0 and
 * 1023 fall into blocks of every family */
static void
icells_init(const struct icells *o, ovhip_tu_state *st, ovhip_tu_desc *d, int tree, int l2w, int l2h)
{
    memset(st, 0, sizeof(*st)); memset(d, 0, sizeof(*d));
    st->qp_y = 30; st->qp_cb = 31; st->qp_cr = 33; st->qp_jcbcr = 32;
    st->qp_y_skip = 30; st->qp_cb_skip = 31; st->qp_cr_skip = 33; st->qp_jcbcr_skip = 32;
    st->lmcs_chroma_scale = 1 << 11;
    const int unit = tree ? 2 : 4, size = tree ? 64 : 128, w = 1 << l2w, h = 1 << l2h, k = (int)o->n_total;
    d->x0 = (uint16_t)(((k * 5) % ((size - w) / unit + 1)) * unit);
    d->y0 = (uint16_t)(((k * 3) % ((size - h) / unit + 1)) * unit);
    d->log2_tb_w = (uint8_t)l2w; d->log2_tb_h = (uint8_t)l2h; d->tree = (uint8_t)tree;
    d->cbf_mask = tree ? 0x3 : 0x10;
    memset(o->c->residual_y, 0, sizeof(o->c->residual_y)); memset(o->c->residual_cb, 0, sizeof(o->c->residual_cb));
    memset(o->c->residual_cr, 0, sizeof(o->c->residual_cr));
}

static void
icells_case(struct icells *o, const ovhip_tu_state *st, ovhip_tu_desc *d, int c_mode)
{
    OVCTUDec *c = o->c;
    const struct OVBuffInfo *cb = &c->rcn_ctx.ctu_buff;
    const int tree = d->tree, l2w = d->log2_tb_w, l2h = d->log2_tb_h, w = 1 << l2w, h = 1 << l2h, x0 = d->x0, y0 = d->y0;
    const int cl2w = tree ? l2w : l2w - 1, cl2h = tree ? l2h : l2h - 1;
    struct TUInfo tu;
    memset(&tu, 0, sizeof(tu));
    /* a file stays below 1 MiB (worst case of one case: three blocks of levels and three expected rectangles) and holds 512 cases at
     * most: the tests lay a file's cases out on 128-row bands of ONE picture, and a command addresses its row with 16 bits */
    if (o->n == 512 || 49152 + (o->coefs.n + o->exp.n + 6 * (size_t)w * h) * 2 + (o->n + 1) * (sizeof(*st) + sizeof(*d) + 36) > 1000000) icells_flush(o);

    int16_t *res[3] = { c->residual_cb, c->residual_cr, c->residual_y };
    uint32_t off3[3] = { 0, 0, 0 }, len3[3] = { 0, 0, 0 };
    for (int comp = 0; comp < 3; ++comp) {
        const int is_l = comp == 2;
        const int used = is_l ? (d->cbf_mask & 0x10) && tree != 2
                              : (d->cbf_mask & 0x8) ? comp == 0 : (d->cbf_mask & (comp ? 0x1 : 0x2));
        if (!used) continue;
        const int tl2w = is_l ? l2w : cl2w, tl2h = is_l ? l2h : cl2h;
        const int ts = is_l ? !!(d->tr_skip_mask & 0x10)
                            : (d->cbf_mask & 0x8) ? !!(d->tr_skip_mask & 0x1) : !!(d->tr_skip_mask & (comp ? 0x1 : 0x2));
        const int raster = (ts && !st->sh_ts_disabled) || tl2w < 2 || tl2h < 2;
        const int cw = (1 << tl2w) > 32 ? 32 : (1 << tl2w), ch = (1 << tl2h) > 32 ? 32 : (1 << tl2h);
        const int n = raster ? (1 << (tl2w + tl2h)) : cw * ch;
        tu.tb_info[comp].sig_sb_map = d->sig_sb_map[comp]; tu.tb_info[comp].last_pos = d->last_pos[comp];
        off3[comp] = (uint32_t)o->coefs.n; len3[comp] = (uint32_t)n;
        gbuf_push(&o->coefs, res[comp], n);
    }
    rcn_init_ict_functions_10(&c->rcn_funcs, st->ict_type, 10);
    itx_set_state(c, st, c_mode);
    tu.cbf_mask = d->cbf_mask; tu.pos_offset = 0; tu.tr_skip_mask = d->tr_skip_mask;
    tu.cu_mts_flag = d->cu_mts_flag; tu.cu_mts_idx = d->cu_mts_idx;
    tu.lfnst_flag = d->lfnst_flag; tu.lfnst_idx = d->lfnst_idx;
    itx_load_pred(c, o->pred_y, o->pred_cb, o->pred_cr);
    if (tree == 0) c->rcn_funcs.tmp.rcn_tu_st(c, x0, y0, l2w, l2h, d->cu_flags, d->cbf_mask, &tu);
    else           c->rcn_funcs.tmp.rcn_tu_c(c, x0, y0, l2w, l2h, d->cu_flags, d->cbf_mask, &tu);

    uint32_t eoff[3] = { 0, 0, 0 };
    if (tree == 0) {
        eoff[0] = (uint32_t)o->exp.n; dump_rect(&o->exp, cb->y, cb->stride, x0, y0, w, h);
        eoff[1] = (uint32_t)o->exp.n; dump_rect(&o->exp, cb->cb, cb->stride_c, x0 >> 1, y0 >> 1, w >> 1, h >> 1);
        eoff[2] = (uint32_t)o->exp.n; dump_rect(&o->exp, cb->cr, cb->stride_c, x0 >> 1, y0 >> 1, w >> 1, h >> 1);
    } else {
        eoff[1] = (uint32_t)o->exp.n; dump_rect(&o->exp, cb->cb, cb->stride_c, x0, y0, w, h);
        eoff[2] = (uint32_t)o->exp.n; dump_rect(&o->exp, cb->cr, cb->stride_c, x0, y0, w, h);
    }
    gbuf_push(&o->state, st, sizeof(*st));
    gbuf_push(&o->desc, d, sizeof(*d));
    gbuf_push(&o->coff, off3, 3); gbuf_push(&o->clen, len3, 3); gbuf_push(&o->eoff, eoff, 3);
    o->n++; o->n_total++;
}

/* levels that stay levels: small ones with a few of three digits, never zero (a cleared sub-block must change the block) */
static int16_t rnd_level(void)
{
    int v = rnd_range(0, 7) ? rnd_range(1, 24) : rnd_range(100, 900);
    return (int16_t)(rnd_range(0, 1) ? v : -v);
}

/* the sub-block (sx, sy) of a block of levels in the reference's layout (cw = min(32, width)) */
static void
icells_sb(int16_t *dst, int cw, int sx, int sy, int16_t (*draw)(void))
{
    int16_t *sb = dst + sy * 4 * cw + sx * 16;
    for (int i = 0; i < 16; ++i) sb[i] = draw();
}

/* one level at (x, y): raster, or inside its 4x4 sub-block */
static void
icells_put(int16_t *dst, int raster, int w, int x, int y, int v)
{
    if (raster) dst[y * w + x] = (int16_t)v;
    else dst[(y >> 2) * 4 * (w > 32 ? 32 : w) + (x >> 2) * 16 + (y & 3) * 4 + (x & 3)] = (int16_t)v;
}

static uint64_t
icells_full_map(int l2w, int l2h)
{
    const int nx = 1 << ((l2w > 5 ? 5 : l2w) - 2), ny = 1 << ((l2h > 5 ? 5 : l2h) - 2);
    uint64_t m = 0;
    for (int sy = 0; sy < ny; ++sy) m |= ((1ull << nx) - 1) << (8 * sy);
    return m;
}

/* a luma transform block whose significant sub-blocks are `map`, levels from `draw` */
static void
icells_luma_map(struct icells *o, ovhip_tu_state *st, ovhip_tu_desc *d, uint64_t map, int16_t (*draw)(void))
{
    const int cw = (1 << d->log2_tb_w) > 32 ? 32 : (1 << d->log2_tb_w);
    for (int b = 0; b < 64; ++b) if ((map >> b) & 1) icells_sb(o->c->residual_y, cw, b & 7, b >> 3, draw);
    d->sig_sb_map[2] = map; d->last_pos[2] = 0x0302;
    icells_case(o, st, d, 0);
}

/* the 16 levels of the de-quantisation family: both ends of int16, +-1 and values between (mostly small ones: where every sample
 * ends at a picture clip, no QP shows); transform skip adds the de-quantised level itself to the sample: more of the smallest */
static const int16_t icells_dq_levels[2][16] = { { 1, -1, 32767, -32768, 2, -3, 517, -32767, 90, -90, 7, -33, 4000, -15, 11, -6 },
                                                 { 1, -1, 32767, -32768, 2, -2, 1, -1, 3, -3, 1, -1, 517, -32767, 5, -7 } };

/* BDPCM levels of a w x h block: the first two lines along the direction run into the two int16 ends of the running sum */
static void
icells_bdpcm_levels(int16_t *dst, int raster, int w, int h, int vertical)
{
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
            const int line = vertical ? x : y, pos = vertical ? y : x;
            int v = line == 0 ? 20000 : line == 1 ? -20000 : line == 2 ? (pos & 1 ? -30000 : 31000) : ((x * 7 + y * 13) % 19) - 9;
            icells_put(dst, raster, w, x, y, v);
        }
}

static void
gen_itx_cells(const char *dir)
{
    static struct icells O;
    struct icells *o = &O;
    ovhip_tu_state st; ovhip_tu_desc d;
    memset(o, 0, sizeof(*o));
    o->dir = dir;
    o->state.type = T_U8; o->desc.type = T_U8; o->coff.type = T_U32; o->clen.type = T_U32; o->coefs.type = T_I16; o->eoff.type = T_U32; o->exp.type = T_U16;
    g_seed = 0x266;
    itx_fill_pred(o->pred_y, o->pred_cb, o->pred_cr);       /* itx.ovg's picture */
    g_seed = 0x266 + 901;
    OVCTUDec *c = o->c = ref_new_ctudec(0, 0);
    c->rcn_funcs.intra_pred_c = stub_intra_pred_c;

    /* ---- transform pairs: every luma shape 4..32, fully populated from rnd_coef's mixture: DCT-II / DCT-II and the four explicit
     *      cu_mts_idx on an inter CU, implicit MTS on an intra CU; the shapes with a side of 64: DCT-II, zero-out to 32 ---- */
    icells_begin(o, "tr");
    for (int l2w = 2; l2w <= 6; ++l2w)
        for (int l2h = 2; l2h <= 6; ++l2h)
            for (int v = 0; v < 6; ++v) {
                if ((l2w == 6 || l2h == 6) && v && !(v == 5 && (l2w <= 4 || l2h <= 4))) continue;   /* (implicit MTS: DST-VII along a side of at most 16) */
                icells_init(o, &st, &d, 0, l2w, l2h);
                st.qp_y = (uint8_t)(8 + v + l2w); st.dep_quant = v & 1;
                if (v >= 1 && v <= 4) { d.cu_mts_flag = 1; d.cu_mts_idx = (uint8_t)(v - 1); }
                if (v == 5) { d.cu_flags |= 1u << 1; st.mts_implicit = 1; }
                icells_luma_map(o, &st, &d, icells_full_map(l2w, l2h), rnd_coef);
            }

    /* ---- extents: every (last significant sub-block column, row) of the one-wave shapes (at most 256 samples, no side above 32), a
     *      map with a hole; the four corners and a hole for the four-wave shapes 32x32, 64x32, 32x64, 64x64 ---- */
    icells_begin(o, "ext");
    for (int l2w = 2; l2w <= 6; ++l2w)
        for (int l2h = 2; l2h <= 6; ++l2h) {
            const int one_wave = l2w + l2h <= 8 && l2w <= 5 && l2h <= 5;
            if (!one_wave && (l2w < 5 || l2h < 5)) continue;
            const int nx = 1 << ((l2w > 5 ? 5 : l2w) - 2), ny = 1 << ((l2h > 5 ? 5 : l2h) - 2);
            for (int ly = 0; ly < ny; ++ly)
                for (int lx = 0; lx < nx; ++lx) {
                    if (!one_wave && !((lx == 0 || lx == nx - 1) && (ly == 0 || ly == ny - 1))) continue;
                    icells_init(o, &st, &d, 0, l2w, l2h);
                    st.qp_y = (uint8_t)(26 + lx + ly);
                    icells_luma_map(o, &st, &d, 1ull | 1ull << lx | 1ull << (8 * ly) | 1ull << (8 * ly + lx), rnd_level);
                }
            if (nx * ny >= 4) {
                icells_init(o, &st, &d, 0, l2w, l2h);
                const int hx = nx >> 1, hy = (ny - 1) >> 1;
                icells_luma_map(o, &st, &d, icells_full_map(l2w, l2h) & ~(1ull << (8 * hy + hx)), rnd_level);
            }
        }

    /* ---- LFNST: the sets through the intra mode (0, 1: set 0; 12, 56: set 1; 18, 50: set 2; 30, 40: set 3; the modes above 34
     *      transposed; 2 and 66 are remapped to wide angles on the non-square shapes), both indices, the size classes; levels in the
     *      first sub-block only (4x4 and 8x8: its first 8 in scan order), the ends of int16 among them.  Luma, then dual-tree chroma
     *      with the mode in lfnst_mode_c: the same modes and LM (67), which takes the mode of the luma block behind it ---- */
    icells_begin(o, "lfnst");
    {
        static const uint8_t shapes[8][2] = { {2,2}, {2,4}, {4,2}, {3,3}, {4,4}, {3,5}, {5,3}, {5,5} };
        static const uint8_t modes[11] = { 0, 1, 12, 56, 18, 50, 30, 40, 2, 66, 67 };
        static const uint8_t scan8[8] = { 0, 4, 1, 8, 5, 2, 12, 9 };
        for (int tree = 0; tree <= 2; tree += 2)
            for (int s = 0; s < 8; ++s)
                for (int m = 0; m < (tree ? 11 : 10); ++m)
                    for (int idx = 0; idx < 2; ++idx) {
                        const int l2w = shapes[s][0], l2h = shapes[s][1], n8 = l2w == l2h && l2w <= 3;
                        icells_init(o, &st, &d, tree, l2w, l2h);
                        d.cu_flags |= 1u << 1; d.lfnst_flag = 1; d.lfnst_idx = (uint8_t)idx;
                        st.qp_y = st.qp_cb = st.qp_cr = (uint8_t)(4 + (m + idx) % 6 + ((m & 1) ? 20 : 0));
                        int c_mode = 0, eff = modes[m];
                        if (tree) {
                            c_mode = modes[m];
                            if (c_mode == 67) { eff = 40; memset(c->drv_ctx.intra_info.luma_modes, eff, sizeof(c->drv_ctx.intra_info.luma_modes)); }
                            st.lfnst_mode_c = (int8_t)shim_lfnst_mode_c(l2w, l2h, eff);
                        } else st.intra_mode = (int8_t)modes[m];
                        for (int comp = tree ? 0 : 2; comp < (tree ? 2 : 3); ++comp) {
                            int16_t *sb = comp == 2 ? c->residual_y : comp ? c->residual_cr : c->residual_cb;
                            for (int i = 0; i < (n8 ? 8 : 16); ++i) {
                                const int k = (i + m + idx + comp) % 7;
                                sb[n8 ? scan8[i] : i] = k == 0 ? 32767 : k == 1 ? -32768 : k == 2 ? -32767 : rnd_level();
                            }
                            d.sig_sb_map[comp] = 1; d.last_pos[comp] = 0x0101;
                        }
                        icells_case(o, &st, &d, c_mode);
                    }
    }

    /* ---- de-quantisation: every QP x dep_quant on 4x4, 8x4 (odd log2 sum), 16x16, 32x16, the first sub-block holding both ends of
     *      int16, +-1 and values between; transform skip with the _skip QP (16 at least, as gen_itx sets it) and regular residual
     *      coding (sh_ts_disabled: the levels are de-quantised); with TS residual coding the levels are final, whatever the QP:
     *      the two small shapes at every QP, 16x16 and 32x16 (raster blocks of the one-wave generic and the four-wave body) at four,
     *      with levels in the block's far corners too ---- */
    icells_begin(o, "dq");
    {
        static const uint8_t shapes[4][2] = { {2,2}, {3,2}, {4,4}, {5,4} };
        for (int qp = 0; qp <= 75; ++qp)
            for (int dq = 0; dq < 2; ++dq)
                for (int s = 0; s < 4; ++s) {
                    icells_init(o, &st, &d, 0, shapes[s][0], shapes[s][1]);
                    st.qp_y = (uint8_t)qp; st.qp_y_skip = (uint8_t)(qp < 16 ? 16 : qp); st.dep_quant = (uint8_t)dq;
                    for (int i = 0; i < 16; ++i) c->residual_y[i] = icells_dq_levels[0][(i + qp) & 15];
                    d.sig_sb_map[2] = 1; d.last_pos[2] = 0x0302;
                    icells_case(o, &st, &d, 0);
                }
        for (int qp = 16; qp <= 75; ++qp)
            for (int tsd = 0; tsd < 2; ++tsd)
                for (int s = 0; s < 4; ++s) {
                    const int l2w = shapes[s][0], l2h = shapes[s][1];
                    if (!tsd && s >= 2 && (qp - 16) % 20 && qp != 75) continue;
                    icells_init(o, &st, &d, 0, l2w, l2h);
                    st.qp_y = st.qp_y_skip = (uint8_t)qp; st.sh_ts_disabled = (uint8_t)tsd; d.tr_skip_mask = 0x10;
                    /* at the picture's corner, +1 on its sample (0, 0) = 0 and -1 on (3, 2) = 1023: from QP 57 on, the level 1 takes every
                     * other sample of the picture to a clip */
                    d.x0 = d.y0 = 0;
                    for (int i = 0; i < 16; ++i) icells_put(c->residual_y, !tsd, 1 << l2w, i & 3, i >> 2, icells_dq_levels[1][i]);
                    if (!tsd && s >= 2) {
                        icells_put(c->residual_y, 1, 1 << l2w, (1 << l2w) - 1, 0, -2); icells_put(c->residual_y, 1, 1 << l2w, 0, (1 << l2h) - 1, 5);
                        icells_put(c->residual_y, 1, 1 << l2w, (1 << l2w) - 1, (1 << l2h) - 1, 3);
                    }
                    d.sig_sb_map[2] = 1; d.last_pos[2] = 0x0302;
                    icells_case(o, &st, &d, 0);
                }
    }

    /* ---- transform skip with BDPCM: every shape up to 32x32, both directions, luma (TS and regular residual coding) and dual-tree
     *      chroma; the running sum saturates at both ends ---- */
    icells_begin(o, "bdpcm");
    for (int tree = 0; tree <= 2; tree += 2)
        for (int l2w = tree ? 1 : 2; l2w <= 5; ++l2w)
            for (int l2h = tree ? 1 : 2; l2h <= 5; ++l2h)
                for (int dir = 0; dir < 2; ++dir)
                    for (int tsd = 0; tsd < 2; ++tsd) {
                        icells_init(o, &st, &d, tree, l2w, l2h);
                        st.sh_ts_disabled = (uint8_t)tsd;
                        st.qp_y_skip = st.qp_cb_skip = st.qp_cr_skip = (uint8_t)(16 + 3 * l2w + l2h + dir);
                        d.cu_flags |= 1u << 1;
                        const int raster = !tsd || l2w < 2 || l2h < 2;
                        if (tree) {
                            d.tr_skip_mask = 0x3; d.cu_flags |= (1u << 9) | ((uint32_t)dir << 11);
                            icells_bdpcm_levels(c->residual_cb, raster, 1 << l2w, 1 << l2h, dir);
                            icells_bdpcm_levels(c->residual_cr, raster, 1 << l2w, 1 << l2h, dir);
                            d.sig_sb_map[0] = d.sig_sb_map[1] = raster ? 1 : icells_full_map(l2w, l2h);
                            d.last_pos[0] = d.last_pos[1] = 0x0101;
                        } else {
                            d.tr_skip_mask = 0x10; d.cu_flags |= (1u << 8) | ((uint32_t)dir << 10);
                            icells_bdpcm_levels(c->residual_y, raster, 1 << l2w, 1 << l2h, dir);
                            d.sig_sb_map[2] = raster ? 1 : icells_full_map(l2w, l2h); d.last_pos[2] = 0x0101;
                        }
                        icells_case(o, &st, &d, 0);
                    }

    /* ---- DC: every luma and dual-tree chroma shape with the first coefficient only: a moderate level, the level that the
     *      de-quantisation clips at either end (|flat value| then is 1024, the most an int16 coefficient allows: the int16 clip of the
     *      flat value itself cannot be reached), and a map whose bit 0 is clear ---- */
    icells_begin(o, "dc");
    for (int tree = 0; tree <= 2; tree += 2)
        for (int l2w = tree ? 1 : 2; l2w <= (tree ? 5 : 6); ++l2w)
            for (int l2h = tree ? 1 : 2; l2h <= (tree ? 5 : 6); ++l2h)
                for (int v = 0; v < 4; ++v) {
                    icells_init(o, &st, &d, tree, l2w, l2h);
                    const int lvl = v == 0 ? 37 + 5 * l2w - 11 * l2h : v == 1 ? 32767 : v == 2 ? -32768 : -21;
                    if (v == 1 || v == 2) st.qp_y = st.qp_cb = st.qp_cr = 51;
                    for (int comp = tree ? 0 : 2; comp < (tree ? 2 : 3); ++comp) {
                        (comp == 2 ? c->residual_y : comp ? c->residual_cr : c->residual_cb)[0] = (int16_t)(comp == 1 ? -lvl - (lvl == -32768) : lvl);
                        d.sig_sb_map[comp] = v != 3; d.last_pos[comp] = 0;
                    }
                    icells_case(o, &st, &d, 0);
                }

    /* ---- sinks: dual-tree chroma 2x2 .. 32x32 (the raster 2xN / Nx2 shapes among them) x ict_type x cbf_mask (Cr, Cb, both, and
     *      the three joint forms) x LMCS chroma scale off / on at both ends of its range (where ict_type applies a scale): the
     *      reference derives (1 << 17) / (window size + offset) with a divisor of 8..511 (rcn_lmcs.c:341-342): 16384 .. 256 ---- */
    icells_begin(o, "sink");
    {
        static const uint8_t cbfs[6] = { 0x1, 0x2, 0x3, 0x9, 0xa, 0xb };
        for (int l2w = 1; l2w <= 5; ++l2w)
            for (int l2h = 1; l2h <= 5; ++l2h)
                for (int ict = 0; ict < 4; ++ict)
                    for (int k = 0; k < 6; ++k)
                        for (int lm = 0; lm < ((ict & 1) ? 3 : 1); ++lm) {
                            icells_init(o, &st, &d, 2, l2w, l2h);
                            st.ict_type = (uint8_t)ict; d.cbf_mask = cbfs[k];
                            st.lmcs_scale_c = lm != 0; st.lmcs_chroma_scale = (int16_t)(lm == 1 ? 256 : lm == 2 ? 16384 : 2048);
                            const int raster = l2w < 2 || l2h < 2;
                            for (int comp = 0; comp < 2; ++comp) {
                                const int used = (cbfs[k] & 0x8) ? comp == 0 : (cbfs[k] & (comp ? 0x1 : 0x2));
                                if (!used) continue;
                                int16_t *dst = comp ? c->residual_cr : c->residual_cb;
                                if (raster) {
                                    for (int i = 0; i < (1 << (l2w + l2h)); ++i) dst[i] = rnd_level();
                                    d.sig_sb_map[comp] = 1;
                                } else {
                                    d.sig_sb_map[comp] = icells_full_map(l2w, l2h) & 0x0303;          /* the first 8x8 at most: the sinks are the subject */
                                    for (int b = 0; b < 16; ++b) if ((d.sig_sb_map[comp] >> b) & 1) icells_sb(dst, 1 << l2w, b & 7, b >> 3, rnd_level);
                                }
                                d.last_pos[comp] = 0x0101;
                            }
                            icells_case(o, &st, &d, 0);
                        }
    }

    /* ---- quads: luma blocks of the one-wave class that are not tiny, in fours, so that the recorder's stable split hands one
     *      workgroup four DIFFERENT paths: LFNST, BDPCM, DC and plain specialised.  The shapes rotate through 16x16, 32x8, 8x32, 32x4
     *      (the most LDS the class uses), then through the remaining shapes ---- */
    icells_begin(o, "quad");
    {
        static const uint8_t big[4][2] = { {4,4}, {5,3}, {3,5}, {5,2} };
        static const uint8_t rest[4][2] = { {2,5}, {4,3}, {3,4}, {4,2} };
        for (int q = 0; q < 8; ++q)
            for (int path = 0; path < 4; ++path) {
                const uint8_t *sh = (q < 4 ? big : rest)[(path + q) & 3];
                const int l2w = sh[0], l2h = sh[1], slot = (path + (q >> 1)) & 3;       /* the paths change waves too */
                icells_init(o, &st, &d, 0, l2w, l2h);
                st.qp_y = st.qp_y_skip = (uint8_t)(22 + q + slot);
                if (slot == 0) {                 /* LFNST */
                    d.cu_flags |= 1u << 1; d.lfnst_flag = 1; d.lfnst_idx = (uint8_t)(q & 1); st.intra_mode = (int8_t)(q & 2 ? 50 : 18);
                    for (int i = 0; i < 16; ++i) c->residual_y[i] = rnd_level();
                    d.sig_sb_map[2] = 1; d.last_pos[2] = 0x0101;
                    icells_case(o, &st, &d, 0);
                } else if (slot == 1) {          /* BDPCM, TS residual coding on even quads, regular on odd ones */
                    st.sh_ts_disabled = q & 1; d.cu_flags |= (1u << 1) | (1u << 8) | ((uint32_t)((q >> 1) & 1) << 10); d.tr_skip_mask = 0x10;
                    icells_bdpcm_levels(c->residual_y, !(q & 1), 1 << l2w, 1 << l2h, (q >> 1) & 1);
                    d.sig_sb_map[2] = (q & 1) ? icells_full_map(l2w, l2h) : 1; d.last_pos[2] = 0x0101;
                    icells_case(o, &st, &d, 0);
                } else if (slot == 2) {          /* DC */
                    c->residual_y[0] = (int16_t)(q & 1 ? -411 : 293); d.sig_sb_map[2] = 1; d.last_pos[2] = 0;
                    icells_case(o, &st, &d, 0);
                } else {                         /* plain, fully populated */
                    if (q & 1) { d.cu_mts_flag = 1; d.cu_mts_idx = (uint8_t)((q >> 1) & 3); }
                    icells_luma_map(o, &st, &d, icells_full_map(l2w, l2h), rnd_level);
                }
            }
    }
    icells_flush(o);
}

/* ====================================================================================== MC */
#define MC_W 208
#define MC_H 120

static void
gen_mc(const char *dir)
{
    gbuf b_desc = { .type = T_U8 }, b_eoff = { .type = T_U32 }, b_exp = { .type = T_U16 };
    uint32_t n_cases = 0;
    g_seed = 0x266 + 1;

    OVCTUDec *c = ref_new_ctudec(0, 0);
    struct InterDRVCtx *ic = &c->drv_ctx.inter_ctx;
    OVPicture *ref[3];
    for (int i = 0; i < 3; ++i) {
        ref[i] = ref_new_picture(MC_W, MC_H, 8 * (i + 1));
        fill_plane(ref[i]->frame->data[0], MC_W, MC_H, MC_W);
        fill_plane(ref[i]->frame->data[1], MC_W / 2, MC_H / 2, MC_W / 2);
        fill_plane(ref[i]->frame->data[2], MC_W / 2, MC_H / 2, MC_W / 2);
    }
    /* rpl0 = {ref0, ref1}, rpl1 = {ref2, ref0}: rpl0[0] and rpl1[1] are the SAME picture (identical-motion path) */
    ic->rpl0[0] = ref[0]; ic->rpl0[1] = ref[1]; ic->rpl1[0] = ref[2]; ic->rpl1[1] = ref[0];
    static const uint8_t slot0[2] = { 0, 1 }, slot1[2] = { 2, 0 };
    for (int i = 0; i < 16; ++i) {
        ic->scale_fact_rpl0[i][0] = ic->scale_fact_rpl0[i][1] = 1 << RPR_SCALE_BITS;
        ic->scale_fact_rpl1[i][0] = ic->scale_fact_rpl1[i][1] = 1 << RPR_SCALE_BITS;
    }
    const struct OVBuffInfo *cb = &c->rcn_ctx.ctu_buff;
    struct shim_stream S;
    shim_stream_init(&S);
    if (g_shim) shim_bind(c, MC_W, MC_H, 0, 0);

    for (int l2w = 2; l2w <= 7; ++l2w) {
        for (int l2h = 2; l2h <= 7; ++l2h) {
            int w = 1 << l2w, h = 1 << l2h;
            if (w > MC_W || h > MC_H) continue;
            int reps = (w * h <= 256) ? 40 : (w * h <= 1024 ? 14 : 4);
            for (int rep = 0; rep < reps; ++rep) {
                ovhip_pu_desc d;
                memset(&d, 0, sizeof(d));
                /* position: anywhere on the 4-grid such that the PU is inside the picture and one CTU */
                int px, py;
                do {
                    px = rnd_range(0, (MC_W - w) / 4) * 4;
                    py = rnd_range(0, (MC_H - h) / 4) * 4;
                } while ((px >> 7) != ((px + w - 1) >> 7) || (py >> 7) != ((py + h - 1) >> 7));
                d.x0 = px; d.y0 = py; d.log2_w = l2w; d.log2_h = l2h;
                d.inter_dir = rnd_range(1, 3);
                d.ref_idx0 = rnd_range(0, 1); d.ref_idx1 = rnd_range(0, 1);
                int range = rep % 4 == 0 ? 4000 : (rep % 4 == 1 ? 64 : 600);   /* far outside / tiny / normal, 1/16 pel */
                d.mv0x = rnd_range(-range, range); d.mv0y = rnd_range(-range, range);
                d.mv1x = rnd_range(-range, range); d.mv1y = rnd_range(-range, range);
                if (rep % 7 == 3) { d.mv0x &= ~15; d.mv1y &= ~15; }            /* H-only / V-only / copy paths */
                if (rep % 7 == 5) { d.mv0x &= ~15; d.mv0y &= ~15; d.mv1x &= ~15; }
                if (rep % 9 == 4) { d.inter_dir = 3; d.ref_idx0 = 0; d.ref_idx1 = 1; d.mv1x = d.mv0x; d.mv1y = d.mv0y; } /* identical motion */
                d.prec_amvr_half = rep % 5 == 2;
                if (d.prec_amvr_half) { d.mv0x = (d.mv0x & ~15) | 8; d.mv1y = (d.mv1y & ~15) | 8; }
                if (w == 4 && h == 4) d.prec_amvr_half = 0;
                d.bcw_idx_plus1 = (rep % 3 == 1) ? rnd_range(1, 5) : 0;
                d.planes = rep % 11 == 7 ? 1 : (rep % 11 == 9 ? 2 : 3);
                d.poc0 = ic->rpl0[d.ref_idx0]->poc; d.poc1 = ic->rpl1[d.ref_idx1]->poc;
                d.ref0 = slot0[d.ref_idx0]; d.ref1 = slot1[d.ref_idx1];

                c->ctb_x = px >> 7; c->ctb_y = py >> 7;
                int x0 = px & 127, y0 = py & 127;
                ic->prec_amvr = d.prec_amvr_half ? MV_PRECISION_HALF : 0;
                OVMV mv0 = { .x = d.mv0x, .y = d.mv0y, .ref_idx = d.ref_idx0, .bcw_idx_plus1 = d.bcw_idx_plus1 };
                OVMV mv1 = { .x = d.mv1x, .y = d.mv1y, .ref_idx = d.ref_idx1, .bcw_idx_plus1 = d.bcw_idx_plus1 };
                for (int j = 0; j < 128; ++j) memset(cb->y + j * cb->stride, 0xAB, 256);
                for (int j = 0; j < 64; ++j) { memset(cb->cb + j * cb->stride_c, 0xAB, 128); memset(cb->cr + j * cb->stride_c, 0xAB, 128); }

                if (d.planes == 3)
                    TIMED(TS_MC, c->rcn_funcs.rcn_mcp_b(c, *cb, ic, c->part_ctx, mv0, mv1, x0, y0, l2w, l2h, d.inter_dir, d.ref_idx0, d.ref_idx1));
                else if (d.planes == 1)
                    TIMED(TS_MC, c->rcn_funcs.rcn_mcp_b_l(c, *cb, ic, c->part_ctx, mv0, mv1, x0, y0, l2w, l2h, d.inter_dir, d.ref_idx0, d.ref_idx1));
                else
                    TIMED(TS_MC, c->rcn_funcs.rcn_mcp_b_c(c, *cb, ic, c->part_ctx, mv0, mv1, x0, y0, l2w, l2h, d.inter_dir, d.ref_idx0, d.ref_idx1));
                if (g_shim) shim_case_end(c, &S, "mc");

                uint32_t eoff[3];
                eoff[0] = (uint32_t)b_exp.n; dump_rect(&b_exp, cb->y, cb->stride, x0, y0, w, h);
                eoff[1] = (uint32_t)b_exp.n; dump_rect(&b_exp, cb->cb, cb->stride_c, x0 >> 1, y0 >> 1, w >> 1, h >> 1);
                eoff[2] = (uint32_t)b_exp.n; dump_rect(&b_exp, cb->cr, cb->stride_c, x0 >> 1, y0 >> 1, w >> 1, h >> 1);
                gbuf_push(&b_desc, &d, sizeof(d));
                gbuf_push(&b_eoff, eoff, 3);
                n_cases++;
            }
        }
    }

    if (g_shim) { shim_stream_write(dir, "shim_mc.ovg", &S, c, ref, 3); return; }
    gfile g = gfile_open(dir, "mc.ovg");
    uint32_t d3[3] = { 3, MC_H, MC_W };
    uint16_t *all = malloc(3 * MC_W * MC_H * 2);
    for (int i = 0; i < 3; ++i) memcpy(all + i * MC_W * MC_H, ref[i]->frame->data[0], MC_W * MC_H * 2);
    gfile_array(&g, "ref_y", T_U16, all, 3, d3);
    d3[1] = MC_H / 2; d3[2] = MC_W / 2;
    for (int i = 0; i < 3; ++i) memcpy(all + i * (MC_W / 2) * (MC_H / 2), ref[i]->frame->data[1], (MC_W / 2) * (MC_H / 2) * 2);
    gfile_array(&g, "ref_cb", T_U16, all, 3, d3);
    for (int i = 0; i < 3; ++i) memcpy(all + i * (MC_W / 2) * (MC_H / 2), ref[i]->frame->data[2], (MC_W / 2) * (MC_H / 2) * 2);
    gfile_array(&g, "ref_cr", T_U16, all, 3, d3);
    uint32_t d2[2] = { n_cases, sizeof(ovhip_pu_desc) };
    gfile_array(&g, "desc", T_U8, b_desc.data, 2, d2);
    d2[1] = 3; gfile_array(&g, "exp_off", T_U32, b_eoff.data, 2, d2);
    gfile_buf(&g, "exp", &b_exp);
    gfile_close(&g);
    fprintf(stderr, "mc.ovg: %u cases, %zu expected samples\n", n_cases, b_exp.n);
}


/* ====================================================================================== MCX
 * mcx.ovg : rcn_bdof_mcp_l (+ rcn_mcp_b_c) and rcn_dmvr_mv_refine driven the way their caller does
 *           (vcl_coding_unit.c:2450-2472, :2598-2668)                          -> K7, K8
 * Reference pictures: R0 smooth random; R1 = R0 displaced by a per-64x64-region integer shift plus a
 * per-region noise level (0 = exact copy: exercises DMVR's early exit and the BDOF disable);
 * R2 independent.  rpl0 = {R0, R2}, rpl1 = {R1, R0}.
 * mcx_make_refs: those pictures (mcx_cells_*.ovg use them too and do not store them); draws from g_seed. */
static void
mcx_make_refs(OVPicture *ref[3])
{
    for (int i = 0; i < 3; ++i) {
        ref[i] = ref_new_picture(MC_W, MC_H, i == 0 ? 8 : (i == 1 ? 24 : 4));
        for (int p = 0; p < 3; ++p) fill_plane(ref[i]->frame->data[p], MC_W >> !!p, MC_H >> !!p, MC_W >> !!p);
    }
    for (int p = 0; p < 3; ++p) {
        int w = MC_W >> !!p, h = MC_H >> !!p, rs = p ? 32 : 64;
        uint16_t *a = (uint16_t *)ref[0]->frame->data[p], *b = (uint16_t *)ref[1]->frame->data[p];
        static int shx[16], shy[16], nz[16];
        if (!p) for (int k = 0; k < 16; ++k) { shx[k] = rnd_range(-2, 2); shy[k] = rnd_range(-2, 2); nz[k] = k % 3 == 0 ? 0 : (k % 3 == 1 ? 2 : 12); }
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < w; ++x) {
                int k = ((y / rs) * 4 + x / rs) & 15;
                int sx = x + (p ? shx[k] / 2 : shx[k]), sy = y + (p ? shy[k] / 2 : shy[k]);
                sx = sx < 0 ? 0 : sx >= w ? w - 1 : sx; sy = sy < 0 ? 0 : sy >= h ? h - 1 : sy;
                int v = a[sy * w + sx] + (nz[k] ? rnd_range(-nz[k], nz[k]) : 0);
                b[y * w + x] = (uint16_t)(v < 0 ? 0 : v > 1023 ? 1023 : v);
            }
    }
}

static void
gen_mcx(const char *dir)
{
    gbuf b_desc = { .type = T_U8 }, b_eoff = { .type = T_U32 }, b_exp = { .type = T_U16 }, b_mv = { .type = T_I32 };
    uint32_t n_cases = 0;
    g_seed = 0x266 + 77;

    OVCTUDec *c = ref_new_ctudec(0, 0);
    struct InterDRVCtx *ic = &c->drv_ctx.inter_ctx;
    OVPicture *ref[3];
    mcx_make_refs(ref);
    ic->rpl0[0] = ref[0]; ic->rpl0[1] = ref[2]; ic->rpl1[0] = ref[1]; ic->rpl1[1] = ref[0];
    static const uint8_t slot0[2] = { 0, 2 }, slot1[2] = { 1, 0 };
    for (int i = 0; i < 16; ++i) {
        ic->scale_fact_rpl0[i][0] = ic->scale_fact_rpl0[i][1] = 1 << RPR_SCALE_BITS;
        ic->scale_fact_rpl1[i][0] = ic->scale_fact_rpl1[i][1] = 1 << RPR_SCALE_BITS;
    }
    const struct OVBuffInfo *cb = &c->rcn_ctx.ctu_buff;
    struct shim_stream S;
    shim_stream_init(&S);
    /* shim mode: a picture-level TMVP motion plane per list, as ovdpb_init_picture allocates them (mvpool.c), so that the
     * write-back of the refined vectors can be checked against where the reference's caller + tmvp_store_mv put them */
    struct MVPlane pl0, pl1;
    const int nb_ctb_w = (MC_W + 127) / 128, nb_ctb_h = (MC_H + 127) / 128, pln_stride = 16 * nb_ctb_w;
    if (g_shim) {
        shim_bind(c, MC_W, MC_H, 0, 0);
        memset(&pl0, 0, sizeof(pl0)); memset(&pl1, 0, sizeof(pl1));
        pl0.mvs = calloc((size_t)pln_stride * 16 * nb_ctb_h, sizeof(OVMV)); pl1.mvs = calloc((size_t)pln_stride * 16 * nb_ctb_h, sizeof(OVMV));
        ic->tmvp_ctx.plane0 = &pl0; ic->tmvp_ctx.plane1 = &pl1;
        c->nb_ctb_pic_w = nb_ctb_w;
    }

    for (int l2w = 3; l2w <= 6; ++l2w) {
        for (int l2h = 3; l2h <= 6; ++l2h) {
            int w = 1 << l2w, h = 1 << l2h;
            if (l2w + l2h < 7 || w > MC_W || h > MC_H) continue;
            int reps = (w * h <= 256) ? 60 : (w * h <= 1024 ? 18 : 8);
            for (int rep = 0; rep < reps; ++rep) {
                ovhip_pu_desc d;
                memset(&d, 0, sizeof(d));
                int px, py;
                do {
                    px = rnd_range(0, (MC_W - w) / 4) * 4;
                    py = rnd_range(0, (MC_H - h) / 4) * 4;
                } while ((px >> 7) != ((px + w - 1) >> 7) || (py >> 7) != ((py + h - 1) >> 7));
                if (rep % 10 == 6) px = 0;
                if (rep % 10 == 8) py = 0;
                d.x0 = px; d.y0 = py; d.log2_w = l2w; d.log2_h = l2h;
                d.inter_dir = 3;
                d.ref_idx0 = rep % 6 == 5; d.ref_idx1 = rep % 8 == 7;
                int range = rep % 9 == 0 ? 4000 : (rep % 3 == 1 ? 40 : 300);
                d.mv0x = rnd_range(-range, range); d.mv0y = rnd_range(-range, range);
                if (rep % 4 != 3) { d.mv1x = -d.mv0x + rnd_range(-20, 20); d.mv1y = -d.mv0y + rnd_range(-20, 20); }   /* mirrored + jitter */
                else              { d.mv1x = rnd_range(-range, range); d.mv1y = rnd_range(-range, range); }
                if (rep % 7 == 3) { d.mv0x &= ~15; d.mv1y &= ~15; }
                if (rep % 7 == 5) { d.mv0x &= ~15; d.mv0y &= ~15; d.mv1x &= ~15; d.mv1y &= ~15; }
                d.prec_amvr_half = rep % 5 == 2;
                if (d.prec_amvr_half) { d.mv0x = (d.mv0x & ~15) | 8; d.mv1y = (d.mv1y & ~15) | 8; }
                d.planes = 3;
                d.refine = (uint8_t)(1 + rep % 3);                  /* BDOF, DMVR, DMVR + BDOF */
                d.poc0 = ic->rpl0[d.ref_idx0]->poc; d.poc1 = ic->rpl1[d.ref_idx1]->poc;
                d.ref0 = slot0[d.ref_idx0]; d.ref1 = slot1[d.ref_idx1];

                c->ctb_x = px >> 7; c->ctb_y = py >> 7;
                int x0 = px & 127, y0 = py & 127;
                ic->prec_amvr = d.prec_amvr_half ? MV_PRECISION_HALF : 0;
                OVMV mv0 = { .x = d.mv0x, .y = d.mv0y, .ref_idx = d.ref_idx0 };
                OVMV mv1 = { .x = d.mv1x, .y = d.mv1y, .ref_idx = d.ref_idx1 };
                for (int j = 0; j < 128; ++j) memset(cb->y + j * cb->stride, 0xAB, 256);
                for (int j = 0; j < 64; ++j) { memset(cb->cb + j * cb->stride_c, 0xAB, 128); memset(cb->cr + j * cb->stride_c, 0xAB, 128); }

                int l2sw = l2w < 4 ? l2w : 4, l2sh = l2h < 4 ? l2h : 4;
                uint32_t mv_off = (uint32_t)b_mv.n;
                for (int i = 0; i < (h >> l2sh); ++i)
                    for (int j = 0; j < (w >> l2sw); ++j) {
                        OVMV m0 = mv0, m1 = mv1;
                        if (d.refine & OVHIP_PU_DMVR)
                            c->rcn_funcs.rcn_dmvr_mv_refine(c, *cb, x0 + j * 16, y0 + i * 16, l2sw, l2sh, &m0, &m1,
                                                            d.ref_idx0, d.ref_idx1, d.refine & OVHIP_PU_BDOF);
                        else
                            c->rcn_funcs.rcn_bdof_mcp_l(c, *cb, x0 + j * 16, y0 + i * 16, l2sw, l2sh, m0, m1, d.ref_idx0, d.ref_idx1);
                        int32_t o[4] = { m0.x, m0.y, m1.x, m1.y };
                        gbuf_push(&b_mv, o, 4);
                    }
                if (!(d.refine & OVHIP_PU_DMVR))
                    c->rcn_funcs.rcn_mcp_b_c(c, *cb, ic, c->part_ctx, mv0, mv1, x0, y0, l2w, l2h, 3, d.ref_idx0, d.ref_idx1);
                if (g_shim) {
                    if (d.refine & OVHIP_PU_DMVR) {
                        /* vectors "from the device" for this case's units: a recognisable value per unit and component;
                         * then every entry the reference's flow would have written must hold it, and no other entry */
                        const int nu = (h >> l2sh) * (w >> l2sw);
                        int32_t fake[64 * 4];
                        for (int u = 0; u < nu; ++u) for (int k = 0; k < 4; ++k) fake[4 * u + k] = 100000 + (int32_t)n_cases * 1000 + u * 8 + k;
                        memset(pl0.mvs, 0, (size_t)pln_stride * 16 * nb_ctb_h * sizeof(OVMV)); memset(pl1.mvs, 0, (size_t)pln_stride * 16 * nb_ctb_h * sizeof(OVMV));
                        {
                            /* the plane entries as the device derives them (k_tmvp_cells; its CPU restatement here: the harness runs
                             * without a GPU, tests/test_gpu_shim_replay.py holds the kernel to the same entries) */
                            extern void oracle_tmvp_cells(const ovhip_mc_unit *, uint32_t, const int32_t *, int, int, ovhip_tmvp_cell *);
                            size_t n_rec = 0;
                            const ovhip_mc_unit *ru = ovhip_rec_mcx_units(ovhip_shim_recorder(c), &n_rec);
                            if ((int)n_rec != nu) { fprintf(stderr, "shim: %zu refined units recorded, %d expected (case %u)\n", n_rec, nu, n_cases); exit(1); }
                            static ovhip_tmvp_cell cells[64 * 4];
                            oracle_tmvp_cells(ru, (uint32_t)nu, fake, 7, pln_stride / 16, cells);
                            ovhip_shim_apply_tmvp_cells(c, cells, 4 * (size_t)nu);
                        }
                        int32_t checked = 0, bad = 0;
                        static OVMV exp0[16 * 16], exp1[16 * 16];      /* the CTU-local tmvp_mv[] arrays of the caller */
                        memset(exp0, 0, sizeof(exp0)); memset(exp1, 0, sizeof(exp1));
                        for (int i = 0, u = 0; i < (h >> l2sh); ++i)
                            for (int j = 0; j < (w >> l2sw); ++j, ++u) {
                                /* vcl_coding_unit.c:2629-2645 */
                                const int b = ((x0 + 7 + j * 16) >> 3) + ((y0 + 7 + i * 16) >> 3) * 16;
                                for (int dy = 0; dy <= (l2sh > 3); ++dy) for (int dx = 0; dx <= (l2sw > 3); ++dx) {
                                    if (((x0 + 7 + j * 16) >> 3) + dx > 15 || ((y0 + 7 + i * 16) >> 3) + dy > 15) continue;
                                    exp0[b + dx + 16 * dy].x = fake[4 * u]; exp0[b + dx + 16 * dy].y = fake[4 * u + 1];
                                    exp1[b + dx + 16 * dy].x = fake[4 * u + 2]; exp1[b + dx + 16 * dy].y = fake[4 * u + 3];
                                }
                            }
                        /* tmvp_store_mv (drv_lines.c:270-330): row i of the CTU array -> plane->mvs + ctb_offset + i * pln_stride */
                        const int ctb_off = (c->ctb_x + c->ctb_y * pln_stride) * 16;
                        for (int py2 = 0; py2 < 16 * nb_ctb_h; ++py2)
                            for (int px2 = 0; px2 < pln_stride; ++px2) {
                                const int lx = px2 - c->ctb_x * 16, ly = py2 - c->ctb_y * 16;
                                OVMV e0 = { 0 }, e1 = { 0 };
                                if (lx >= 0 && lx < 16 && ly >= 0 && ly < 16) { e0 = exp0[lx + 16 * ly]; e1 = exp1[lx + 16 * ly]; }
                                const OVMV *g0 = &pl0.mvs[py2 * pln_stride + px2], *g1 = &pl1.mvs[py2 * pln_stride + px2];
                                (void)ctb_off;
                                if (g0->x != e0.x || g0->y != e0.y || g1->x != e1.x || g1->y != e1.y) bad++;
                                checked += e0.x != 0;
                                if (e0.x != 0) {
                                    /* which unit of the case the entry belongs to is encoded in the recognisable value */
                                    int32_t rec[3] = { (int32_t)S.n_cases, py2 * pln_stride + px2, (e0.x - 100000 - (int32_t)n_cases * 1000) / 8 };
                                    gbuf_push(&S.tmvp_exp, rec, 3);
                                }
                            }
                        if (bad) { fprintf(stderr, "shim: refined-MV write-back differs from the reference's flow in %d entries (case %u)\n", bad, n_cases); exit(1); }
                        gbuf_push(&S.mv_chk, &checked, 1);
                    }
                    shim_case_end(c, &S, "mcx");
                    /* next case: fresh patch list, as a new picture would */
                    ovhip_shim_new_picture_for_test(c);
                }

                uint32_t eoff[4];
                eoff[0] = (uint32_t)b_exp.n; dump_rect(&b_exp, cb->y, cb->stride, x0, y0, w, h);
                eoff[1] = (uint32_t)b_exp.n; dump_rect(&b_exp, cb->cb, cb->stride_c, x0 >> 1, y0 >> 1, w >> 1, h >> 1);
                eoff[2] = (uint32_t)b_exp.n; dump_rect(&b_exp, cb->cr, cb->stride_c, x0 >> 1, y0 >> 1, w >> 1, h >> 1);
                eoff[3] = mv_off;
                gbuf_push(&b_desc, &d, sizeof(d));
                gbuf_push(&b_eoff, eoff, 4);
                n_cases++;
            }
        }
    }

    if (g_shim) { shim_stream_write(dir, "shim_mcx.ovg", &S, c, ref, 3); return; }
    gfile g = gfile_open(dir, "mcx.ovg");
    uint32_t d3[3] = { 3, MC_H, MC_W };
    uint16_t *all = malloc(3 * MC_W * MC_H * 2);
    for (int i = 0; i < 3; ++i) memcpy(all + i * MC_W * MC_H, ref[i]->frame->data[0], MC_W * MC_H * 2);
    gfile_array(&g, "ref_y", T_U16, all, 3, d3);
    d3[1] = MC_H / 2; d3[2] = MC_W / 2;
    for (int i = 0; i < 3; ++i) memcpy(all + i * (MC_W / 2) * (MC_H / 2), ref[i]->frame->data[1], (MC_W / 2) * (MC_H / 2) * 2);
    gfile_array(&g, "ref_cb", T_U16, all, 3, d3);
    for (int i = 0; i < 3; ++i) memcpy(all + i * (MC_W / 2) * (MC_H / 2), ref[i]->frame->data[2], (MC_W / 2) * (MC_H / 2) * 2);
    gfile_array(&g, "ref_cr", T_U16, all, 3, d3);
    uint32_t d2[2] = { n_cases, sizeof(ovhip_pu_desc) };
    gfile_array(&g, "desc", T_U8, b_desc.data, 2, d2);
    d2[1] = 4; gfile_array(&g, "exp_off", T_U32, b_eoff.data, 2, d2);
    gfile_buf(&g, "exp", &b_exp);
    gfile_buf(&g, "exp_mv", &b_mv);
    gfile_close(&g);
    fprintf(stderr, "mcx.ovg: %u cases, %zu expected samples, %zu refined MVs\n", n_cases, b_exp.n, b_mv.n / 4);
}

/* ====================================================================================== MCA
 * mca.ovg : affine CUs the way rcn_affine_mcp_b_l / rcn_affine_prof_mcp_b_l / rcn_affine_mcp_b_c
 *           (drv_affine_mvp.c:3264-3411) drive rcn_mcp_b_l(2,2) / rcn_prof_mcp_b_l / rcn_mcp_b_c(3,3)  -> K9
 * struct PROFInfo is private to rcn_inter.c:1128-1134; the slot only forward-declares it. */
struct PROFInfo { int16_t dmv_scale_h_0[16], dmv_scale_v_0[16], dmv_scale_h_1[16], dmv_scale_v_1[16]; };

static void
gen_mca(const char *dir)
{
    gbuf b_desc = { .type = T_U8 }, b_eoff = { .type = T_U32 }, b_exp = { .type = T_U16 }, b_mv = { .type = T_I32 };
    uint32_t n_cases = 0;
    g_seed = 0x266 + 99;

    OVCTUDec *c = ref_new_ctudec(0, 0);
    struct InterDRVCtx *ic = &c->drv_ctx.inter_ctx;
    OVPicture *ref[3];
    for (int i = 0; i < 3; ++i) {
        ref[i] = ref_new_picture(MC_W, MC_H, 8 * (i + 1));
        for (int p = 0; p < 3; ++p) fill_plane(ref[i]->frame->data[p], MC_W >> !!p, MC_H >> !!p, MC_W >> !!p);
    }
    ic->rpl0[0] = ref[0]; ic->rpl0[1] = ref[1]; ic->rpl1[0] = ref[2]; ic->rpl1[1] = ref[0];
    static const uint8_t slot0[2] = { 0, 1 }, slot1[2] = { 2, 0 };
    for (int i = 0; i < 16; ++i) {
        ic->scale_fact_rpl0[i][0] = ic->scale_fact_rpl0[i][1] = 1 << RPR_SCALE_BITS;
        ic->scale_fact_rpl1[i][0] = ic->scale_fact_rpl1[i][1] = 1 << RPR_SCALE_BITS;
    }
    ic->prec_amvr = 0;                                        /* drv_affine_mvp.c:3508 */
    const struct OVBuffInfo *cb = &c->rcn_ctx.ctu_buff;
    struct shim_stream S;
    shim_stream_init(&S);
    if (g_shim) shim_bind(c, MC_W, MC_H, 0, 0);

    for (int l2w = 3; l2w <= 6; ++l2w) {
        for (int l2h = 3; l2h <= 6; ++l2h) {
            int w = 1 << l2w, h = 1 << l2h;
            if (w > MC_W || h > MC_H) continue;
            int reps = (w * h <= 256) ? 36 : (w * h <= 1024 ? 14 : 6);
            for (int rep = 0; rep < reps; ++rep) {
                ovhip_affine_desc d;
                memset(&d, 0, sizeof(d));
                int px, py;
                do {
                    px = rnd_range(0, (MC_W - w) / 4) * 4;
                    py = rnd_range(0, (MC_H - h) / 4) * 4;
                } while ((px >> 7) != ((px + w - 1) >> 7) || (py >> 7) != ((py + h - 1) >> 7));
                if (rep % 10 == 6) px = 0;
                if (rep % 10 == 8) py = MC_H - h;
                d.x0 = px; d.y0 = py; d.log2_w = l2w; d.log2_h = l2h;
                d.inter_dir = rnd_range(1, 3);
                int ri0 = rnd_range(0, 1), ri1 = rnd_range(0, 1);
                if (rep % 9 == 4) { d.inter_dir = 3; ri0 = 0; ri1 = 1; }          /* same picture in both lists */
                d.bcw_idx_plus1 = (rep % 4 == 1) ? rnd_range(1, 5) : 0;
                d.prof_dir = rep % 3 == 0 ? 0 : (d.inter_dir == 3 ? rnd_range(1, 3) : d.inter_dir);
                d.ref0 = slot0[ri0]; d.ref1 = slot1[ri1];
                d.poc0 = ic->rpl0[ri0]->poc; d.poc1 = ic->rpl1[ri1]->poc;
                d.mv_stride = w >> 2;
                for (int t = 0; t < 4; ++t)
                    for (int k = 0; k < 16; ++k) d.dmv_scale[t][k] = (int16_t)(rep % 5 == 3 ? (rnd_range(0, 1) ? 31 : -31) : rnd_range(-31, 31));

                /* a 6-parameter motion field per list, 1/16 pel; occasionally far outside the picture */
                int nsx = w >> 2, nsy = h >> 2;
                int32_t *mvs = calloc((size_t)nsx * nsy * 4, sizeof(int32_t));
                int32_t *m0 = mvs, *m1 = mvs + 2 * nsx * nsy;
                int range = rep % 8 == 0 ? 3000 : 300;
                for (int l = 0; l < 2; ++l) {
                    int bx = rnd_range(-range, range), by = rnd_range(-range, range);
                    int ax = rnd_range(-24, 24), ay = rnd_range(-24, 24), cx = rnd_range(-24, 24), cy = rnd_range(-24, 24);
                    if (rep % 7 == 2) { ax = ay = cx = cy = 0; bx &= ~15; by &= ~15; }          /* integer translation */
                    int32_t *m = l ? m1 : m0;
                    for (int j = 0; j < nsy; ++j)
                        for (int i = 0; i < nsx; ++i) {
                            m[2 * (j * nsx + i)] = bx + ((ax * i + cx * j) >> 1);
                            m[2 * (j * nsx + i) + 1] = by + ((ay * i + cy * j) >> 1);
                        }
                }
                if (rep % 9 == 4) memcpy(m1, m0, (size_t)nsx * nsy * 8);                       /* identical motion */
                d.mv0 = m0; d.mv1 = m1;

                c->ctb_x = px >> 7; c->ctb_y = py >> 7;
                int x0 = px & 127, y0 = py & 127;
                for (int j = 0; j < 128; ++j) memset(cb->y + j * cb->stride, 0xAB, 256);
                for (int j = 0; j < 64; ++j) { memset(cb->cb + j * cb->stride_c, 0xAB, 128); memset(cb->cr + j * cb->stride_c, 0xAB, 128); }

                struct PROFInfo pi;
                memcpy(&pi, d.dmv_scale, sizeof(pi));
                for (int j = 0; j < nsy; ++j)
                    for (int i = 0; i < nsx; ++i) {
                        int k = j * nsx + i;
                        OVMV mv0 = { .x = m0[2 * k], .y = m0[2 * k + 1], .ref_idx = ri0, .bcw_idx_plus1 = d.bcw_idx_plus1 };
                        OVMV mv1 = { .x = m1[2 * k], .y = m1[2 * k + 1], .ref_idx = ri1, .bcw_idx_plus1 = d.bcw_idx_plus1 };
                        if (!d.prof_dir)
                            c->rcn_funcs.rcn_mcp_b_l(c, *cb, ic, c->part_ctx, mv0, mv1, x0 + 4 * i, y0 + 4 * j, 2, 2, d.inter_dir, ri0, ri1);
                        else
                            c->rcn_funcs.rcn_prof_mcp_b_l(c, *cb, ic, c->part_ctx, mv0, mv1, x0 + 4 * i, y0 + 4 * j, 2, 2, d.inter_dir, ri0, ri1,
                                                          d.prof_dir, (const void *)&pi);
                    }
                for (int j = 0; j < nsy; j += 2)
                    for (int i = 0; i < nsx; i += 2) {
                        int k = j * nsx + i, k2 = k + nsx + 1;
                        OVMV mv0 = { .x = m0[2 * k] + m0[2 * k2], .y = m0[2 * k + 1] + m0[2 * k2 + 1], .ref_idx = ri0, .bcw_idx_plus1 = d.bcw_idx_plus1 };
                        OVMV mv1 = { .x = m1[2 * k] + m1[2 * k2], .y = m1[2 * k + 1] + m1[2 * k2 + 1], .ref_idx = ri1, .bcw_idx_plus1 = d.bcw_idx_plus1 };
                        mv0.x += mv0.x < 0; mv0.y += mv0.y < 0; mv0.x >>= 1; mv0.y >>= 1;
                        mv1.x += mv1.x < 0; mv1.y += mv1.y < 0; mv1.x >>= 1; mv1.y >>= 1;
                        c->rcn_funcs.rcn_mcp_b_c(c, *cb, ic, c->part_ctx, mv0, mv1, x0 + 4 * i, y0 + 4 * j, 3, 3, d.inter_dir, ri0, ri1);
                    }
                if (g_shim) shim_case_end(c, &S, "mca");

                uint32_t eoff[4];
                eoff[0] = (uint32_t)b_exp.n; dump_rect(&b_exp, cb->y, cb->stride, x0, y0, w, h);
                eoff[1] = (uint32_t)b_exp.n; dump_rect(&b_exp, cb->cb, cb->stride_c, x0 >> 1, y0 >> 1, w >> 1, h >> 1);
                eoff[2] = (uint32_t)b_exp.n; dump_rect(&b_exp, cb->cr, cb->stride_c, x0 >> 1, y0 >> 1, w >> 1, h >> 1);
                eoff[3] = (uint32_t)b_mv.n;
                gbuf_push(&b_mv, mvs, (size_t)nsx * nsy * 4);
                d.mv0 = d.mv1 = NULL;
                gbuf_push(&b_desc, &d, sizeof(d));
                gbuf_push(&b_eoff, eoff, 4);
                free(mvs);
                n_cases++;
            }
        }
    }

    if (g_shim) { shim_stream_write(dir, "shim_mca.ovg", &S, c, ref, 3); return; }
    gfile g = gfile_open(dir, "mca.ovg");
    uint32_t d3[3] = { 3, MC_H, MC_W };
    uint16_t *all = malloc(3 * MC_W * MC_H * 2);
    for (int i = 0; i < 3; ++i) memcpy(all + i * MC_W * MC_H, ref[i]->frame->data[0], MC_W * MC_H * 2);
    gfile_array(&g, "ref_y", T_U16, all, 3, d3);
    d3[1] = MC_H / 2; d3[2] = MC_W / 2;
    for (int i = 0; i < 3; ++i) memcpy(all + i * (MC_W / 2) * (MC_H / 2), ref[i]->frame->data[1], (MC_W / 2) * (MC_H / 2) * 2);
    gfile_array(&g, "ref_cb", T_U16, all, 3, d3);
    for (int i = 0; i < 3; ++i) memcpy(all + i * (MC_W / 2) * (MC_H / 2), ref[i]->frame->data[2], (MC_W / 2) * (MC_H / 2) * 2);
    gfile_array(&g, "ref_cr", T_U16, all, 3, d3);
    uint32_t d2[2] = { n_cases, sizeof(ovhip_affine_desc) };
    gfile_array(&g, "desc", T_U8, b_desc.data, 2, d2);
    d2[1] = 4; gfile_array(&g, "exp_off", T_U32, b_eoff.data, 2, d2);
    gfile_buf(&g, "exp", &b_exp);
    gfile_buf(&g, "mvs", &b_mv);
    gfile_close(&g);
    fprintf(stderr, "mca.ovg: %u cases, %zu expected samples\n", n_cases, b_exp.n);
}

/* ====================================================================================== LMCS
 * lmcs.ovg : rcn_init_lmcs (table construction), rcn_lmcs_compute_chroma_scale, lmcs_reshape_backward  -> K11
 * struct LMCSLUTs is private to rcn_lmcs.c:75-81. */
#include "rcn_lmcs.h"
struct LMCSLUTs { OVSample fwd_lut[1024]; OVSample bwd_lut[1024]; OVSample wnd_bnd[17]; };
#define LM_W 256
#define LM_H 128

static void
gen_lmcs(const char *dir)
{
    gbuf b_data = { .type = T_U8 }, b_luts = { .type = T_U8 }, b_reg = { .type = T_I32 }, b_inv = { .type = T_U16 };
    g_seed = 0x266 + 111;
    OVCTUDec *c = ref_new_ctudec(0, 1);
    const struct OVBuffInfo *cb = &c->rcn_ctx.ctu_buff;
    struct shim_stream S;
    shim_stream_init(&S);
    gbuf s_luts = { .type = T_U8 };
    if (g_shim) shim_bind(c, LM_W, LM_H, 0, 1);
    uint16_t *pic = malloc(LM_W * LM_H * 2);
    fill_plane(pic, LM_W, LM_H, LM_W);
    int n_sets = 0;

    for (int set = 0; set < 24; ++set) {
        struct OVLMCSData ld;
        memset(&ld, 0, sizeof(ld));
        ld.lmcs_min_bin_idx = rnd_range(0, 4);
        ld.lmcs_delta_max_bin_idx = rnd_range(0, 4);
        int amp = set % 4 == 0 ? 0 : (set % 4 == 1 ? 8 : (set % 4 == 2 ? 30 : 60));
        for (int i = 0; i < 16; ++i) {
            ld.lmcs_delta_abs_cw[i] = rnd_range(0, amp);
            ld.lmcs_delta_sign_cw_flag[i] = rnd_range(0, 1);
        }
        if (set % 6 == 5) { ld.lmcs_delta_abs_cw[7] = 64; ld.lmcs_delta_sign_cw_flag[7] = 1; }   /* an empty window */
        ld.lmcs_delta_abs_crs = rnd_range(0, 7);
        ld.lmcs_delta_sign_crs_flag = rnd_range(0, 1);

        struct LMCSInfo *li = &c->lmcs_info;
        if (!li->luts) li->luts = calloc(1, sizeof(struct LMCSLUTs));   /* keeps rcn_init_lmcs off ov_malloc (ovmem.c is not built) */
        c->rcn_funcs.rcn_init_lmcs(li, &ld);
        if (g_shim) gbuf_push(&s_luts, ovhip_shim_lmcs(c), sizeof(ovhip_lmcs_luts));

        ovhip_lmcs_data hd;
        memset(&hd, 0, sizeof(hd));
        hd.min_bin_idx = ld.lmcs_min_bin_idx; hd.delta_max_bin_idx = ld.lmcs_delta_max_bin_idx;
        hd.crs_offset = ld.lmcs_delta_sign_crs_flag ? -ld.lmcs_delta_abs_crs : ld.lmcs_delta_abs_crs;
        for (int i = 0; i < 16; ++i) hd.cw_delta[i] = ld.lmcs_delta_sign_cw_flag[i] ? -ld.lmcs_delta_abs_cw[i] : ld.lmcs_delta_abs_cw[i];
        gbuf_push(&b_data, &hd, sizeof(hd));

        ovhip_lmcs_luts hl;
        memset(&hl, 0, sizeof(hl));
        memcpy(hl.fwd_lut, li->luts->fwd_lut, 2048); memcpy(hl.bwd_lut, li->luts->bwd_lut, 2048);
        memcpy(hl.wnd_bnd, li->luts->wnd_bnd, 34);
        hl.min_idx = li->min_idx; hl.max_idx = li->max_idx; hl.crs_offset = li->lmcs_chroma_scaling_offset;
        gbuf_push(&b_luts, &hl, sizeof(hl));

        /* chroma scale of every 64x64 region of the 2-CTU picture under several availability patterns */
        for (int ctb = 0; ctb < 2; ++ctb) {
            /* CTU scratch = picture samples incl. the row above / column left of the CTU (zero outside the picture) */
            for (int j = -1; j < 128; ++j)
                for (int i = -1; i < 128; ++i) {
                    int px = ctb * 128 + i, py = j;
                    cb->y[j * cb->stride + i] = (px < 0 || py < 0) ? 0 : pic[py * LM_W + px];
                }
            for (int k = 0; k < 12; ++k) {
                int x0 = (k & 1) * 64, y0 = ((k >> 1) & 1) * 64;
                int n_abv = k < 4 ? 16 : rnd_range(0, 16), n_lft = k < 4 ? 16 : rnd_range(0, 16);
                if (y0 == 0) n_abv = 0;
                if (ctb == 0 && x0 == 0) n_lft = 0;
                struct CTUBitField pf;
                memset(&pf, 0, sizeof(pf));
                uint64_t am = n_abv ? ((1ull << n_abv) - 1) : 0, lm = n_lft ? ((1ull << n_lft) - 1) : 0;
                pf.hfield[y0 >> 2] = am << ((x0 >> 2) + 1);
                pf.vfield[x0 >> 2] = lm << ((y0 >> 2) + 1);
                li->lmcs_chroma_scale = 0;
                c->ctb_x = ctb; c->ctb_y = 0;
                c->rcn_funcs.rcn_lmcs_compute_chroma_scale(li, cb->stride, &pf, cb->y, x0, y0);
                if (g_shim) shim_case_end(c, &S, "lmcs region");
                int32_t rec[6] = { set, ctb * 128 + x0, y0, (int32_t)am, (int32_t)lm, li->lmcs_chroma_scale };
                gbuf_push(&b_reg, rec, 6);
            }
        }
        /* inverse mapping of the whole picture, CTU by CTU (every 6th table set keeps the fixture small) */
        for (int ctb = 0; ctb < 2 && set % 6 == 1; ++ctb) {
            uint16_t *blk = malloc(128 * 128 * 2);
            for (int j = 0; j < 128; ++j) memcpy(blk + j * 128, pic + j * LM_W + ctb * 128, 256);
            c->rcn_funcs.lmcs_reshape_backward(blk, 128, li->luts, 128, 128);
            gbuf_push(&b_inv, blk, 128 * 128);
            free(blk);
        }
        n_sets++;
    }

    if (g_shim) {
        gfile gs = gfile_open(dir, "shim_lmcs.ovg");
        uint32_t ds[2] = { (uint32_t)n_sets, sizeof(ovhip_lmcs_luts) };
        gfile_array(&gs, "luts", T_U8, s_luts.data, 2, ds);
        ds[0] = (uint32_t)(S.arr[OVHIP_REC_REGION].n / sizeof(ovhip_lmcs_region)); ds[1] = sizeof(ovhip_lmcs_region);
        gfile_array(&gs, "region", T_U8, S.arr[OVHIP_REC_REGION].data, 2, ds);
        gfile_close(&gs);
        fprintf(stderr, "shim_lmcs.ovg: %d table sets, %u regions\n", n_sets, ds[0]);
        return;
    }
    gfile g = gfile_open(dir, "lmcs.ovg");
    uint32_t d2[2] = { LM_H, LM_W };
    gfile_array(&g, "pic_y", T_U16, pic, 2, d2);
    d2[0] = n_sets; d2[1] = sizeof(ovhip_lmcs_data);  gfile_array(&g, "data", T_U8, b_data.data, 2, d2);
    d2[1] = sizeof(ovhip_lmcs_luts);                   gfile_array(&g, "luts", T_U8, b_luts.data, 2, d2);
    d2[0] = (uint32_t)(b_reg.n / 6); d2[1] = 6;        gfile_array(&g, "regions", T_I32, b_reg.data, 2, d2);
    uint32_t d4[4] = { (uint32_t)(b_inv.n / (2 * 128 * 128)), 2, 128, 128 };          gfile_array(&g, "inverse", T_U16, b_inv.data, 4, d4);
    gfile_close(&g);
    fprintf(stderr, "lmcs.ovg: %d table sets, %zu chroma-scale regions\n", n_sets, b_reg.n / 6);
}

/* ====================================================================================== GPM / CIIP
 * gpm.ovg : rcn_gpm_b (rcn_inter.c:3118-3143) for every merge_gpm_partition_idx, and rcn_ciip_b
 *           (rcn_inter.c:3011-3037) with the intra slots replaced by a stub that delivers a known
 *           "planar" prediction (intra prediction itself is outside the path)          -> K10 */
extern void rcn_init_gpm_params(void);
static uint16_t *g_ciip_intra[3];
static OVCTUDec *g_ciip_c;
static void stub_ciip_intra_l(const struct OVRCNCtx *const r, const struct OVBuffInfo *b, uint8_t m, int x0, int y0, int lw, int lh, CUFlags f)
{
    (void)r; (void)m; (void)f;
    int px = (g_ciip_c->ctb_x << 7) + x0, py = (g_ciip_c->ctb_y << 7) + y0;
    for (int j = 0; j < (1 << lh); ++j)
        for (int i = 0; i < (1 << lw); ++i) b->y[(y0 + j) * b->stride + x0 + i] = g_ciip_intra[0][(py + j) * MC_W + px + i];
}
static void stub_ciip_intra_c(const struct OVRCNCtx *const r, uint8_t m, int x0, int y0, int lw, int lh, CUFlags f)
{
    (void)m; (void)f;
    const struct OVBuffInfo *b = &r->ctu_buff;
    int px = (g_ciip_c->ctb_x << 6) + x0, py = (g_ciip_c->ctb_y << 6) + y0;
    for (int j = 0; j < (1 << lh); ++j)
        for (int i = 0; i < (1 << lw); ++i) {
            b->cb[(y0 + j) * b->stride_c + x0 + i] = g_ciip_intra[1][(py + j) * (MC_W / 2) + px + i];
            b->cr[(y0 + j) * b->stride_c + x0 + i] = g_ciip_intra[2][(py + j) * (MC_W / 2) + px + i];
        }
}

static void
gen_gpm(const char *dir)
{
    gbuf b_desc = { .type = T_U8 }, b_eoff = { .type = T_U32 }, b_exp = { .type = T_U16 }, b_ciip = { .type = T_I32 };
    uint32_t n_cases = 0, n_gpm = 0;
    g_seed = 0x266 + 131;
    rcn_init_gpm_params();

    OVCTUDec *c = ref_new_ctudec(0, 0);
    g_ciip_c = c;
    struct InterDRVCtx *ic = &c->drv_ctx.inter_ctx;
    OVPicture *ref[3];
    for (int i = 0; i < 3; ++i) {
        ref[i] = ref_new_picture(MC_W, MC_H, 8 * (i + 1));
        for (int p = 0; p < 3; ++p) fill_plane(ref[i]->frame->data[p], MC_W >> !!p, MC_H >> !!p, MC_W >> !!p);
    }
    for (int p = 0; p < 3; ++p) {
        g_ciip_intra[p] = malloc((MC_W >> !!p) * (MC_H >> !!p) * 2);
        fill_plane(g_ciip_intra[p], MC_W >> !!p, MC_H >> !!p, MC_W >> !!p);
    }
    ic->rpl0[0] = ref[0]; ic->rpl0[1] = ref[1]; ic->rpl1[0] = ref[2]; ic->rpl1[1] = ref[0];
    static const uint8_t slot[2][2] = { { 0, 1 }, { 2, 0 } };            /* [list][ref_idx] -> picture slot */
    for (int i = 0; i < 16; ++i) {
        ic->scale_fact_rpl0[i][0] = ic->scale_fact_rpl0[i][1] = 1 << RPR_SCALE_BITS;
        ic->scale_fact_rpl1[i][0] = ic->scale_fact_rpl1[i][1] = 1 << RPR_SCALE_BITS;
    }
    void *real_intra_l = (void *)c->rcn_funcs.intra_pred, *real_intra_c = (void *)c->rcn_funcs.intra_pred_c;
    c->rcn_funcs.intra_pred = stub_ciip_intra_l;
    c->rcn_funcs.intra_pred_c = stub_ciip_intra_c;
    uint16_t *cur[3];                                                     /* pass 2: the picture being decoded */
    for (int p = 0; p < 3; ++p) { cur[p] = malloc((MC_W >> !!p) * (MC_H >> !!p) * 2); }
    c->part_map.cu_mode_x = calloc(64, 1);
    const struct OVBuffInfo *cb = &c->rcn_ctx.ctu_buff;
    struct shim_stream S;
    shim_stream_init(&S);
    if (g_shim) shim_bind(c, MC_W, MC_H, 0, 0);

    uint32_t n_ciip2 = 0;
    for (int pass = 0; pass < 3; ++pass) {                                /* 0: GPM, 1: CIIP (planar stubbed), 2: CIIP, real planar */
        int n_iter = pass == 0 ? 64 * 3 : pass == 1 ? 150 : 120;
        if (pass == 2) {
            /* the real slots: intra_pred / intra_pred_c read the CTU scratch around the block, as in a decoder */
            c->rcn_funcs.intra_pred = real_intra_l; c->rcn_funcs.intra_pred_c = real_intra_c;
            c->rcn_funcs.rcn_attach_ctu_buff(&c->rcn_ctx, 7, 1);
            cb = &c->rcn_ctx.ctu_buff;
            for (int p = 0; p < 3; ++p) fill_plane(cur[p], MC_W >> !!p, MC_H >> !!p, MC_W >> !!p);
        }
        for (int it = 0; it < n_iter; ++it) {
            ovhip_pu_desc d;
            memset(&d, 0, sizeof(d));
            int l2w, l2h;
            if (pass == 0) { l2w = rnd_range(3, 6); l2h = rnd_range(3, 6); }
            else { do { l2w = rnd_range(2, 6); l2h = rnd_range(2, 6); } while (l2w + l2h < 6); }
            int w = 1 << l2w, h = 1 << l2h, px, py;
            do {
                px = rnd_range(0, (MC_W - w) / 4) * 4;
                py = rnd_range(0, (MC_H - h) / 4) * 4;
            } while ((px >> 7) != ((px + w - 1) >> 7) || (py >> 7) != ((py + h - 1) >> 7));
            d.x0 = px; d.y0 = py; d.log2_w = l2w; d.log2_h = l2h;
            int range = it % 9 == 0 ? 4000 : 400;
            d.mv0x = rnd_range(-range, range); d.mv0y = rnd_range(-range, range);
            d.mv1x = rnd_range(-range, range); d.mv1y = rnd_range(-range, range);
            if (it % 7 == 3) { d.mv0x &= ~15; d.mv1y &= ~15; }
            d.planes = 3;
            d.ref_idx0 = rnd_range(0, 1); d.ref_idx1 = rnd_range(0, 1);
            c->ctb_x = px >> 7; c->ctb_y = py >> 7;
            int x0 = px & 127, y0 = py & 127;
            if (pass < 2) {
                for (int j = 0; j < 128; ++j) memset(cb->y + j * cb->stride, 0xAB, 256);
                for (int j = 0; j < 64; ++j) { memset(cb->cb + j * cb->stride_c, 0xAB, 128); memset(cb->cr + j * cb->stride_c, 0xAB, 128); }
            } else {
                /* CTU scratch <- current picture (clamped at the picture border: what lies outside is never available);
                 * progress: the decoder's CTU start, every row of the CTU above the block, and the part of the block's rows
                 * (and some below) left of it */
                const int ox = c->ctb_x << 7, oy = c->ctb_y << 7;
                #define CLAMP(v, lo, hi) ((v) < (lo) ? (lo) : (v) > (hi) ? (hi) : (v))
                for (int j = -1; j < 132; ++j) for (int i = -128; i < 196; ++i)
                    cb->y[j * cb->stride + i] = cur[0][CLAMP(oy + j, 0, MC_H - 1) * MC_W + CLAMP(ox + i, 0, MC_W - 1)];
                for (int j = -1; j < 66; ++j) for (int i = -64; i < 98; ++i) {
                    const int yy = CLAMP(oy / 2 + j, 0, MC_H / 2 - 1), xx = CLAMP(ox / 2 + i, 0, MC_W / 2 - 1);
                    cb->cb[j * cb->stride_c + i] = cur[1][yy * (MC_W / 2) + xx]; cb->cr[j * cb->stride_c + i] = cur[2][yy * (MC_W / 2) + xx];
                }
                struct OVRCNCtx *r = &c->rcn_ctx;
                memset(&r->progress_field, 0, sizeof(r->progress_field)); memset(&r->progress_field_c, 0, sizeof(r->progress_field_c));
                init_ctu_bitfield(r, (c->ctb_x ? CTU_LFT_FLG : 0) | (c->ctb_y ? CTU_UP_FLG : 0), 7);
                const int xu = x0 >> 2, yu = y0 >> 2, hu = h >> 2;
                const int wu = (MC_W - ox) >> 2 < 32 ? (MC_W - ox) >> 2 : 32;          /* the CTU's columns inside the picture */
                if (yu) { ctu_field_set_rect_bitfield(&r->progress_field, 0, 0, wu, yu); ctu_field_set_rect_bitfield(&r->progress_field_c, 0, 0, wu, yu); }
                if (xu) {
                    int nl = rnd_range(hu, 2 * hu);
                    if (yu + nl > (MC_H >> 2)) nl = (MC_H >> 2) - yu;
                    if (yu + nl > 32) nl = 32 - yu;
                    ctu_field_set_rect_bitfield(&r->progress_field, 0, yu, xu, nl); ctu_field_set_rect_bitfield(&r->progress_field_c, 0, yu, xu, nl);
                }
            }
            int32_t cargs[2] = { 0, 0 };

            if (pass == 0) {
                struct VVCGPM *g = &ic->gpm_ctx;
                memset(g, 0, sizeof(*g));
                g->split_dir = it % 64;
                g->inter_dir0 = rnd_range(1, 2); g->inter_dir1 = rnd_range(1, 2);
                g->mv0 = (OVMV){ .x = d.mv0x, .y = d.mv0y, .ref_idx = d.ref_idx0 };
                g->mv1 = (OVMV){ .x = d.mv1x, .y = d.mv1y, .ref_idx = d.ref_idx1 };
                d.inter_dir = 3; d.refine = OVHIP_PU_GPM; d.gpm_split_dir = (uint8_t)g->split_dir;
                d.ref0 = slot[g->inter_dir0 - 1][d.ref_idx0]; d.ref1 = slot[g->inter_dir1 - 1][d.ref_idx1];
                d.prec_amvr_half = it % 5 == 2;
                ic->prec_amvr = d.prec_amvr_half ? MV_PRECISION_HALF : 0;
                c->rcn_funcs.rcn_gpm_b(c, g, x0, y0, l2w, l2h);
                n_gpm++;
            } else {
                d.inter_dir = rnd_range(1, 3);
                d.bcw_idx_plus1 = 0;
                d.poc0 = ic->rpl0[d.ref_idx0]->poc; d.poc1 = ic->rpl1[d.ref_idx1]->poc;
                d.ref0 = slot[0][d.ref_idx0]; d.ref1 = slot[1][d.ref_idx1];
                ic->prec_amvr = 0;
                cargs[0] = (int32_t[]){ OV_INTER, OV_INTRA, OV_MIP, OV_INTER_SKIP }[rnd_range(0, 3)];
                cargs[1] = (int32_t[]){ OV_INTER, OV_INTRA, OV_MIP, OV_INTER_SKIP }[rnd_range(0, 3)];
                c->part_map.cu_mode_x[(x0 + w - 1) >> 2] = (uint8_t)cargs[0];
                c->part_map.cu_mode_y[(y0 + h - 1) >> 2] = (uint8_t)cargs[1];
                OVMV mv0 = { .x = d.mv0x, .y = d.mv0y, .ref_idx = d.ref_idx0 };
                OVMV mv1 = { .x = d.mv1x, .y = d.mv1y, .ref_idx = d.ref_idx1 };
                if (d.inter_dir == 1 && it % 2)
                    c->rcn_funcs.rcn_ciip(c, x0, y0, l2w, l2h, mv0, d.ref_idx0);              /* P-slice entry point */
                else
                    c->rcn_funcs.rcn_ciip_b(c, mv0, mv1, x0, y0, l2w, l2h, d.inter_dir, d.ref_idx0, d.ref_idx1);
            }
            if (g_shim) shim_case_end(c, &S, "gpm / ciip");
            if (pass == 2) n_ciip2++;
            uint32_t eoff[3];
            eoff[0] = (uint32_t)b_exp.n; dump_rect(&b_exp, cb->y, cb->stride, x0, y0, w, h);
            eoff[1] = (uint32_t)b_exp.n; dump_rect(&b_exp, cb->cb, cb->stride_c, x0 >> 1, y0 >> 1, w >> 1, h >> 1);
            eoff[2] = (uint32_t)b_exp.n; dump_rect(&b_exp, cb->cr, cb->stride_c, x0 >> 1, y0 >> 1, w >> 1, h >> 1);
            gbuf_push(&b_desc, &d, sizeof(d));
            gbuf_push(&b_eoff, eoff, 3);
            gbuf_push(&b_ciip, cargs, 2);
            n_cases++;
        }
    }

    if (g_shim) { shim_stream_write(dir, "shim_gpm.ovg", &S, c, ref, 3); return; }
    gfile g = gfile_open(dir, "gpm.ovg");
    uint32_t d3[3] = { 3, MC_H, MC_W };
    uint16_t *all = malloc(3 * MC_W * MC_H * 2);
    for (int i = 0; i < 3; ++i) memcpy(all + i * MC_W * MC_H, ref[i]->frame->data[0], MC_W * MC_H * 2);
    gfile_array(&g, "ref_y", T_U16, all, 3, d3);
    d3[1] = MC_H / 2; d3[2] = MC_W / 2;
    for (int i = 0; i < 3; ++i) memcpy(all + i * (MC_W / 2) * (MC_H / 2), ref[i]->frame->data[1], (MC_W / 2) * (MC_H / 2) * 2);
    gfile_array(&g, "ref_cb", T_U16, all, 3, d3);
    for (int i = 0; i < 3; ++i) memcpy(all + i * (MC_W / 2) * (MC_H / 2), ref[i]->frame->data[2], (MC_W / 2) * (MC_H / 2) * 2);
    gfile_array(&g, "ref_cr", T_U16, all, 3, d3);
    uint32_t di[2] = { MC_H, MC_W };
    gfile_array(&g, "intra_y", T_U16, g_ciip_intra[0], 2, di);
    di[0] = MC_H / 2; di[1] = MC_W / 2;
    gfile_array(&g, "intra_cb", T_U16, g_ciip_intra[1], 2, di);
    gfile_array(&g, "intra_cr", T_U16, g_ciip_intra[2], 2, di);
    uint32_t d2[2] = { n_cases, sizeof(ovhip_pu_desc) };
    gfile_array(&g, "desc", T_U8, b_desc.data, 2, d2);
    d2[1] = 3; gfile_array(&g, "exp_off", T_U32, b_eoff.data, 2, d2);
    d2[1] = 2; gfile_array(&g, "ciip_modes", T_I32, b_ciip.data, 2, d2);
    uint32_t one = n_gpm; gfile_array(&g, "n_gpm", T_U32, &one, 1, (uint32_t[]){ 1 });
    one = n_ciip2; gfile_array(&g, "n_ciip_planar", T_U32, &one, 1, (uint32_t[]){ 1 });
    di[0] = MC_H; di[1] = MC_W; gfile_array(&g, "cur_y", T_U16, cur[0], 2, di);
    di[0] = MC_H / 2; di[1] = MC_W / 2; gfile_array(&g, "cur_cb", T_U16, cur[1], 2, di); gfile_array(&g, "cur_cr", T_U16, cur[2], 2, di);
    gfile_buf(&g, "exp", &b_exp);
    gfile_close(&g);
    fprintf(stderr, "gpm.ovg: %u GPM + %u CIIP (planar stubbed) + %u CIIP cases, %zu expected samples\n", n_gpm, n_cases - n_gpm - n_ciip2, n_ciip2, b_exp.n);
}

/* ====================================================================================== MC / MCX cells
 * mc_cells_<family>_<nn>.ovg : the cells of the plain units (k_mc2) that mc.ovg's random draws leave out, enumerated -- what the
 * cells are and what reaches them is counted by tests/mc_census.py.  Same slots as mc.ovg (rcn_mcp_b / _l / _c; the combine family
 * also rcn_gpm_b and rcn_ciip / rcn_ciip_b with the intra slots stubbed as in gpm.ovg), same 208x120 pictures (not stored again)
 * except for the combine family, which paints its own.  A PU is one unit (<= 16x16) unless the cell needs a unit that lies wholly
 * outside the picture, which only a unit of a larger PU can.  Families:
 *   phase    every (shape, lists, chroma phase of 32) horizontally and vertically (the luma phase is its low four bits), the half-pel
 *            rows; every window inside the picture
 *   combine  uni L0 / L1, average, the five BCW indices, GPM and the three CIIP weights per shape, on pictures of full-swing steps:
 *            the interpolation overshoots, so that the final clip binds at 0 and at 1023
 *   planes   both, luma only, chroma only
 *   border   per shape, for the luma and for the chroma window: the window crosses the left / right / top / bottom border or a
 *            corner, or lies wholly outside on one side, at each offset 0..3 of its first column within an aligned group of 4
 * Every case: the reference must leave the CTU buffer outside the PU untouched (checked here).  The cases sit on a grid of slots so
 * that a test can launch many of them into one picture.
 * mcx_cells_<family>_<nn>.ovg : refined units (rcn_dmvr_mv_refine) on mcx.ovg's pictures (not stored again):
 *   far      DMVR with one or both initial vectors beyond clip_mv's range, on each side
 *   limit    DMVR with initial vectors next to the +-2^17 limits of the refined vector */
#define MCC_MAX_EXP 400000          /* expected samples per file */
struct mcc_out {
    const char *dir, *prefix, *fam;
    int part, with_mv;
    gbuf desc, eoff, exp, modes, mv;
    uint32_t n;
    OVPicture **ref;                /* pictures of the family's own: stored in each of its files */
    uint16_t **intra;
};

static void
mcc_flush(struct mcc_out *o)
{
    char name[96];
    if (!o->n) return;
    snprintf(name, sizeof(name), "%s_%s_%02d.ovg", o->prefix, o->fam, o->part++);
    gfile g = gfile_open(o->dir, name);
    if (o->ref) {
        uint32_t d3[3] = { 3, MC_H, MC_W };
        uint16_t *all = malloc(3 * MC_W * MC_H * 2);
        for (int i = 0; i < 3; ++i) memcpy(all + i * MC_W * MC_H, o->ref[i]->frame->data[0], MC_W * MC_H * 2);
        gfile_array(&g, "ref_y", T_U16, all, 3, d3);
        d3[1] = MC_H / 2; d3[2] = MC_W / 2;
        for (int p = 1; p < 3; ++p) {
            for (int i = 0; i < 3; ++i) memcpy(all + i * (MC_W / 2) * (MC_H / 2), o->ref[i]->frame->data[p], (MC_W / 2) * (MC_H / 2) * 2);
            gfile_array(&g, p == 1 ? "ref_cb" : "ref_cr", T_U16, all, 3, d3);
        }
        free(all);
    }
    if (o->intra) {
        uint32_t di[2] = { MC_H, MC_W };
        gfile_array(&g, "intra_y", T_U16, o->intra[0], 2, di);
        di[0] = MC_H / 2; di[1] = MC_W / 2;
        gfile_array(&g, "intra_cb", T_U16, o->intra[1], 2, di);
        gfile_array(&g, "intra_cr", T_U16, o->intra[2], 2, di);
    }
    uint32_t d2[2] = { o->n, sizeof(ovhip_pu_desc) };
    gfile_array(&g, "desc", T_U8, o->desc.data, 2, d2);
    d2[1] = o->with_mv ? 4 : 3; gfile_array(&g, "exp_off", T_U32, o->eoff.data, 2, d2);
    if (!o->with_mv) { d2[1] = 2; gfile_array(&g, "ciip_modes", T_I32, o->modes.data, 2, d2); }
    gfile_buf(&g, "exp", &o->exp);
    if (o->with_mv) gfile_buf(&g, "exp_mv", &o->mv);
    gfile_close(&g);
    fprintf(stderr, "%s: %u cases, %zu expected samples\n", name, o->n, o->exp.n);
    o->desc.n = o->eoff.n = o->exp.n = o->modes.n = o->mv.n = 0; o->n = 0;
}

/* before a case: the CTU buffer filled; after it: the PU's three rectangles dumped, everything else must still hold the fill */
static void
mcc_fill(const struct OVBuffInfo *cb)
{
    for (int j = 0; j < 128; ++j) memset(cb->y + j * cb->stride, 0xAB, 256);
    for (int j = 0; j < 64; ++j) { memset(cb->cb + j * cb->stride_c, 0xAB, 128); memset(cb->cr + j * cb->stride_c, 0xAB, 128); }
}

static void
mcc_dump(struct mcc_out *o, const struct OVBuffInfo *cb, const ovhip_pu_desc *d, uint32_t eoff[3])
{
    const int x0 = d->x0 & 127, y0 = d->y0 & 127, w = 1 << d->log2_w, h = 1 << d->log2_h;
    for (int p = 0; p < 3; ++p) {
        const int c = p != 0, n = 128 >> c, stride = c ? cb->stride_c : cb->stride;
        const uint16_t *q = p == 0 ? cb->y : p == 1 ? cb->cb : cb->cr;
        const int written = p ? (d->planes & 2) : (d->planes & 1);
        for (int j = 0; j < n; ++j)
            for (int i = 0; i < n; ++i) {
                const int in = written && i >= (x0 >> c) && i < ((x0 + w) >> c) && j >= (y0 >> c) && j < ((y0 + h) >> c);
                if (!in && q[j * stride + i] != 0xABAB) {
                    fprintf(stderr, "%s %s case %u: the reference wrote plane %d at (%d, %d), outside the PU\n", o->prefix, o->fam, o->n, p, i, j);
                    exit(1);
                }
            }
        eoff[p] = (uint32_t)o->exp.n;
        dump_rect(&o->exp, q, stride, x0 >> c, y0 >> c, w >> c, h >> c);
    }
}

enum { MCC_PLAIN, MCC_GPM, MCC_CIIP };
struct mcc_ctx { OVCTUDec *c; struct InterDRVCtx *ic; };
static const uint8_t mcc_slot[2][2] = { { 0, 1 }, { 2, 0 } };            /* [list][ref_idx] -> picture slot, as mc.ovg and gpm.ovg */

/* one case through the reference.  kind MCC_GPM: d->inter_dir holds the two partitions' lists (dir0 | dir1 << 2) on entry;
 * MCC_CIIP: modes = the neighbours' CU modes (above, left), p_entry: the P-slice entry point rcn_ciip */
static void
mcc_case(struct mcc_out *o, struct mcc_ctx *m, ovhip_pu_desc *d, int kind, const int32_t modes[2], int p_entry)
{
    OVCTUDec *c = m->c;
    struct InterDRVCtx *ic = m->ic;
    const struct OVBuffInfo *cb = &c->rcn_ctx.ctu_buff;
    const int w = 1 << d->log2_w, h = 1 << d->log2_h, l2w = d->log2_w, l2h = d->log2_h;
    int32_t cargs[2] = { modes ? modes[0] : 0, modes ? modes[1] : 0 };
    if ((d->x0 >> 7) != ((d->x0 + w - 1) >> 7) || d->y0 + h > MC_H || d->x0 + w > MC_W) { fprintf(stderr, "%s: PU outside its CTU or the picture\n", o->fam); exit(1); }
    if (o->exp.n + (size_t)w * h * 3 / 2 > MCC_MAX_EXP) mcc_flush(o);
    c->ctb_x = d->x0 >> 7; c->ctb_y = d->y0 >> 7;
    const int x0 = d->x0 & 127, y0 = d->y0 & 127;
    ic->prec_amvr = d->prec_amvr_half ? MV_PRECISION_HALF : 0;
    mcc_fill(cb);
    if (kind == MCC_GPM) {
        struct VVCGPM *g = &ic->gpm_ctx;
        memset(g, 0, sizeof(*g));
        g->split_dir = d->gpm_split_dir;
        g->inter_dir0 = d->inter_dir & 3; g->inter_dir1 = d->inter_dir >> 2;
        g->mv0 = (OVMV){ .x = d->mv0x, .y = d->mv0y, .ref_idx = d->ref_idx0 };
        g->mv1 = (OVMV){ .x = d->mv1x, .y = d->mv1y, .ref_idx = d->ref_idx1 };
        d->ref0 = mcc_slot[g->inter_dir0 - 1][d->ref_idx0]; d->ref1 = mcc_slot[g->inter_dir1 - 1][d->ref_idx1];
        d->inter_dir = 3; d->refine = OVHIP_PU_GPM; d->planes = 3;
        c->rcn_funcs.rcn_gpm_b(c, g, x0, y0, l2w, l2h);
    } else {
        d->poc0 = ic->rpl0[d->ref_idx0]->poc; d->poc1 = ic->rpl1[d->ref_idx1]->poc;
        d->ref0 = mcc_slot[0][d->ref_idx0]; d->ref1 = mcc_slot[1][d->ref_idx1];
        OVMV mv0 = { .x = d->mv0x, .y = d->mv0y, .ref_idx = d->ref_idx0, .bcw_idx_plus1 = d->bcw_idx_plus1 };
        OVMV mv1 = { .x = d->mv1x, .y = d->mv1y, .ref_idx = d->ref_idx1, .bcw_idx_plus1 = d->bcw_idx_plus1 };
        if (kind == MCC_CIIP) {
            d->planes = 3;
            c->part_map.cu_mode_x[(x0 + w - 1) >> 2] = (uint8_t)cargs[0];
            c->part_map.cu_mode_y[(y0 + h - 1) >> 2] = (uint8_t)cargs[1];
            if (p_entry) c->rcn_funcs.rcn_ciip(c, x0, y0, l2w, l2h, mv0, d->ref_idx0);
            else         c->rcn_funcs.rcn_ciip_b(c, mv0, mv1, x0, y0, l2w, l2h, d->inter_dir, d->ref_idx0, d->ref_idx1);
        } else if (d->planes == 3) c->rcn_funcs.rcn_mcp_b(c, *cb, ic, c->part_ctx, mv0, mv1, x0, y0, l2w, l2h, d->inter_dir, d->ref_idx0, d->ref_idx1);
        else if (d->planes == 1)   c->rcn_funcs.rcn_mcp_b_l(c, *cb, ic, c->part_ctx, mv0, mv1, x0, y0, l2w, l2h, d->inter_dir, d->ref_idx0, d->ref_idx1);
        else                       c->rcn_funcs.rcn_mcp_b_c(c, *cb, ic, c->part_ctx, mv0, mv1, x0, y0, l2w, l2h, d->inter_dir, d->ref_idx0, d->ref_idx1);
    }
    uint32_t eoff[3];
    mcc_dump(o, cb, d, eoff);
    gbuf_push(&o->desc, d, sizeof(*d));
    gbuf_push(&o->eoff, eoff, 3);
    gbuf_push(&o->modes, cargs, 2);
    o->n++;
}

/* the n-th slot of the grid for a pw x ph PU: 16-sample slots (32 for a side of 32), PUs narrower than their slot at every multiple
 * of 4 inside it in turn; margin: the slots keep that far from the picture's borders */
static void
mcc_place(ovhip_pu_desc *d, int n, int margin)
{
    const int pw = 1 << d->log2_w, ph = 1 << d->log2_h, sw = pw > 16 ? 32 : 16, sh = ph > 16 ? 32 : 16;
    const int x_lo = (margin + sw - 1) / sw * sw, y_lo = (margin + sh - 1) / sh * sh;
    const int nx = (MC_W - margin - x_lo) / sw, ny = (MC_H - margin - y_lo) / sh;
    d->x0 = (uint16_t)(x_lo + sw * (n % nx) + 4 * ((n / 7) % ((sw - pw) / 4 + 1)));
    d->y0 = (uint16_t)(y_lo + sh * ((n / nx) % ny) + 4 * ((n / 5) % ((sh - ph) / 4 + 1)));
}

/* one axis of a reference window [s0, s0 + len) against [0, pic): 0 inside, 1 crosses the low border, 2 the high one, 3 / 4 wholly
 * outside on the low / high side */
static int
mcc_axis_class(int s0, int len, int pic)
{
    return s0 + len <= 0 ? 3 : s0 >= pic ? 4 : s0 < 0 ? 1 : s0 + len > pic ? 2 : 0;
}

/* border family, one axis: a vector component (1/16) for the PU at pos (length pu_len, units of unit_len) so that SOME unit's window
 * (luma: chroma == 0) has class `cls` and, if off >= 0, starts at offset `off` within its aligned group of 4; `pick` chooses among the
 * vectors that do; frac: the fraction asked for (lost where clip_mv moves the vector).  Returns 0 if there is none. */
static int
mcc_find_mv(int pos, int pu_len, int unit_len, int pic, int chroma, int cls, int off, int frac, int pick, int32_t *mv)
{
    int found[1024], n = 0;
    const int lo = -((pu_len + 3 + pos) << 4), hi = (pic + 2 - pos) << 4;
    for (int dx = -(pu_len + 8 + pos); dx <= pic + 8 - pos && n < 1024; ++dx) {
        int v = 16 * dx + frac;
        v = v < lo ? lo : v > hi ? hi : v;                                   /* clip_mv */
        if (n && found[n - 1] == v) continue;
        for (int u = 0; u < pu_len; u += unit_len) {
            const int s0 = chroma ? ((pos + u) >> 1) + (v >> 5) - 1 : pos + u + (v >> 4) - 3;
            const int len = chroma ? (unit_len >> 1) + 3 : unit_len + 7;
            if (mcc_axis_class(s0, len, chroma ? pic >> 1 : pic) == cls && (off < 0 || (s0 & 3) == off)) { found[n++] = v; break; }
        }
    }
    if (!n) return 0;
    *mv = found[pick % n];
    return 1;
}

static void
gen_mc_cells(const char *dir)
{
    g_seed = 0x266 + 1;                                       /* mc.ovg's seed: the first draws are its three pictures */
    rcn_init_gpm_params();
    OVCTUDec *c = ref_new_ctudec(0, 0);
    g_ciip_c = c;
    struct InterDRVCtx *ic = &c->drv_ctx.inter_ctx;
    OVPicture *ref[3], *paint[3];
    for (int i = 0; i < 3; ++i) {
        ref[i] = ref_new_picture(MC_W, MC_H, 8 * (i + 1));
        fill_plane(ref[i]->frame->data[0], MC_W, MC_H, MC_W);
        fill_plane(ref[i]->frame->data[1], MC_W / 2, MC_H / 2, MC_W / 2);
        fill_plane(ref[i]->frame->data[2], MC_W / 2, MC_H / 2, MC_W / 2);
    }
    g_seed = 0x266 + 811;                                     /* this generator's own */
    /* the combine family's pictures: runs of 0 and 1023 (a few mid-range samples between), rows repeating with flips; the third
     * picture is the first with a tenth of its samples drawn again, so that both lists of a bi-prediction overshoot together */
    for (int i = 0; i < 3; ++i) {
        paint[i] = ref_new_picture(MC_W, MC_H, 8 * (i + 1));
        for (int p = 0; p < 3; ++p) {
            const int w = MC_W >> !!p, h = MC_H >> !!p;
            uint16_t *a = (uint16_t *)paint[i]->frame->data[p];
            for (int y = 0; y < h; ++y) {
                int v = rnd_range(0, 1) ? 1023 : 0, run = rnd_range(1, 7);
                for (int x = 0; x < w; ++x) {
                    if (!run--) { v = rnd_range(0, 7) == 0 ? rnd_range(0, 1023) : v > 511 ? 0 : 1023; run = rnd_range(1, 7); }
                    a[y * w + x] = (uint16_t)((y % 3) && rnd_range(0, 7) ? a[(y - 1) * w + x] : v);
                }
            }
            if (i == 2) {
                const uint16_t *src = (const uint16_t *)paint[0]->frame->data[p];
                for (int k = 0; k < w * h; ++k) if (rnd_range(0, 9)) a[k] = src[k];
            }
        }
    }
    for (int p = 0; p < 3; ++p) {
        g_ciip_intra[p] = malloc((MC_W >> !!p) * (MC_H >> !!p) * 2);
        for (int k = 0; k < (MC_W >> !!p) * (MC_H >> !!p); ++k) {
            const int r = rnd_range(0, 3);
            g_ciip_intra[p][k] = (uint16_t)(r == 0 ? 0 : r == 1 ? 1023 : rnd_range(0, 1023));
        }
    }
    for (int i = 0; i < 16; ++i) {
        ic->scale_fact_rpl0[i][0] = ic->scale_fact_rpl0[i][1] = 1 << RPR_SCALE_BITS;
        ic->scale_fact_rpl1[i][0] = ic->scale_fact_rpl1[i][1] = 1 << RPR_SCALE_BITS;
    }
    c->rcn_funcs.intra_pred = stub_ciip_intra_l;
    c->rcn_funcs.intra_pred_c = stub_ciip_intra_c;
    c->part_map.cu_mode_x = calloc(64, 1);
    struct mcc_ctx M = { c, ic };
    #define MCC_REFS(r) do { ic->rpl0[0] = (r)[0]; ic->rpl0[1] = (r)[1]; ic->rpl1[0] = (r)[2]; ic->rpl1[1] = (r)[0]; } while (0)

    /* ---- phase ---- */
    {
        struct mcc_out o = { .dir = dir, .prefix = "mc_cells", .fam = "phase", .desc = { .type = T_U8 }, .eoff = { .type = T_U32 }, .exp = { .type = T_U16 }, .modes = { .type = T_I32 } };
        MCC_REFS(ref);
        int n = 0;
        for (int l2w = 2; l2w <= 4; ++l2w)
            for (int l2h = 2; l2h <= 4; ++l2h)
                for (int dirn = 1; dirn <= 3; ++dirn) {
                    for (int k = 0; k < 32 + (l2w + l2h > 4 ? 4 : 0); ++k, ++n) {
                        ovhip_pu_desc d;
                        memset(&d, 0, sizeof(d));
                        d.log2_w = l2w; d.log2_h = l2h; d.inter_dir = dirn; d.planes = 3;
                        d.ref_idx0 = n & 1; d.ref_idx1 = 0;
                        int fa[2], fb[2];                                     /* (fx, fy) of the list the case is about, of the other one */
                        if (k < 32) { fa[0] = k; fa[1] = (13 * k + 5) & 31; fb[0] = 31 - k; fb[1] = (7 * k + 2) & 31; }
                        else {
                            static const int hp[4][2] = { { 8, 8 }, { 8, 24 }, { 24, 3 }, { 5, 8 } };
                            fa[0] = hp[k - 32][0]; fa[1] = hp[k - 32][1]; fb[0] = fa[1]; fb[1] = fa[0];
                            d.prec_amvr_half = 1;
                        }
                        const int ix = 32 * (k % 5 - 2), iy = 32 * (k % 3 - 1);
                        const int a = dirn == 2;                              /* the list the case is about */
                        int32_t mv[2][2] = { { ix + fa[0], iy + fa[1] }, { -ix + fb[0], -iy + fb[1] } };
                        d.mv0x = mv[a][0]; d.mv0y = mv[a][1]; d.mv1x = mv[!a][0]; d.mv1y = mv[!a][1];
                        mcc_place(&d, n, 12);
                        mcc_case(&o, &M, &d, MCC_PLAIN, NULL, 0);
                    }
                }
        mcc_flush(&o);
    }
    /* ---- combine ---- */
    {
        struct mcc_out o = { .dir = dir, .prefix = "mc_cells", .fam = "combine", .desc = { .type = T_U8 }, .eoff = { .type = T_U32 }, .exp = { .type = T_U16 }, .modes = { .type = T_I32 },
                             .ref = paint, .intra = g_ciip_intra };
        MCC_REFS(paint);
        int n = 0;
        for (int l2w = 2; l2w <= 4; ++l2w)
            for (int l2h = 2; l2h <= 4; ++l2h) {
                for (int cell = 0; cell < 8; ++cell)                          /* uni L0, uni L1, average, BCW index 1..5 */
                    for (int rep = 0; rep < 3; ++rep, ++n) {
                        ovhip_pu_desc d;
                        memset(&d, 0, sizeof(d));
                        d.log2_w = l2w; d.log2_h = l2h; d.planes = 3;
                        d.inter_dir = cell < 2 ? cell + 1 : 3;
                        d.bcw_idx_plus1 = cell < 3 ? 0 : cell - 2;
                        d.ref_idx0 = 0; d.ref_idx1 = 0;                       /* the first picture and its near copy */
                        d.mv0x = rnd_range(-40, 40) | 1; d.mv0y = rnd_range(-40, 40) | 2;
                        d.mv1x = d.mv0x + 2 * rnd_range(-1, 1); d.mv1y = d.mv0y + 4 * rnd_range(-1, 1);
                        mcc_place(&d, n, 12);
                        mcc_case(&o, &M, &d, MCC_PLAIN, NULL, 0);
                    }
                if (l2w >= 3 && l2h >= 3)                                     /* GPM: coding units of 8x8 and more (rcn_gpm_b) */
                    for (int k = 0; k < 16; ++k, ++n) {
                        ovhip_pu_desc d;
                        memset(&d, 0, sizeof(d));
                        d.log2_w = l2w; d.log2_h = l2h;
                        d.gpm_split_dir = (uint8_t)((4 * k + 2 * (l2w - 3) + (l2h - 3)) & 63);
                        d.inter_dir = (uint8_t)(rnd_range(1, 2) | rnd_range(1, 2) << 2);
                        d.ref_idx0 = 0; d.ref_idx1 = rnd_range(0, 1);
                        d.mv0x = rnd_range(-40, 40) | 1; d.mv0y = rnd_range(-40, 40) | 2;
                        d.mv1x = rnd_range(-40, 40) | 4; d.mv1y = rnd_range(-40, 40) | 1;
                        d.prec_amvr_half = k % 5 == 2;
                        mcc_place(&d, n, 12);
                        mcc_case(&o, &M, &d, MCC_GPM, NULL, 0);
                    }
                if (l2w + l2h >= 6)                                           /* CIIP: coding units of 64 samples and more */
                    for (int wt = 1; wt <= 3; ++wt)
                        for (int dirn = 0; dirn <= 3; ++dirn, ++n) {          /* 0: list 0 through the P-slice entry point */
                            ovhip_pu_desc d;
                            memset(&d, 0, sizeof(d));
                            d.log2_w = l2w; d.log2_h = l2h; d.inter_dir = dirn ? dirn : 1;
                            d.ref_idx0 = 0; d.ref_idx1 = 0;
                            d.mv0x = rnd_range(-40, 40) | 1; d.mv0y = rnd_range(-40, 40) | 2;
                            d.mv1x = d.mv0x + 2 * rnd_range(-1, 1); d.mv1y = d.mv0y + 4 * rnd_range(-1, 1);
                            const int32_t modes[2] = { wt >= 2 ? OV_INTRA : n & 1 ? OV_INTER : OV_INTER_SKIP, wt == 3 ? OV_MIP : OV_INTER };
                            mcc_place(&d, n, 12);
                            mcc_case(&o, &M, &d, MCC_CIIP, modes, dirn == 0);
                        }
            }
        mcc_flush(&o);
    }
    /* ---- planes ---- */
    {
        struct mcc_out o = { .dir = dir, .prefix = "mc_cells", .fam = "planes", .desc = { .type = T_U8 }, .eoff = { .type = T_U32 }, .exp = { .type = T_U16 }, .modes = { .type = T_I32 } };
        MCC_REFS(ref);
        int n = 0;
        for (int l2w = 2; l2w <= 4; ++l2w)
            for (int l2h = 2; l2h <= 4; ++l2h)
                for (int planes = 1; planes <= 3; ++planes)
                    for (int dirn = 1; dirn <= 3; ++dirn, ++n) {
                        ovhip_pu_desc d;
                        memset(&d, 0, sizeof(d));
                        d.log2_w = l2w; d.log2_h = l2h; d.inter_dir = dirn; d.planes = planes;
                        d.ref_idx0 = n & 1; d.ref_idx1 = 0;
                        d.bcw_idx_plus1 = n % 4 == 1 ? 1 + n % 5 : 0;
                        d.mv0x = rnd_range(-60, 60); d.mv0y = rnd_range(-60, 60); d.mv1x = rnd_range(-60, 60); d.mv1y = rnd_range(-60, 60);
                        mcc_place(&d, n, 12);
                        mcc_case(&o, &M, &d, MCC_PLAIN, NULL, 0);
                    }
        mcc_flush(&o);
    }
    /* ---- border ---- */
    {
        struct mcc_out o = { .dir = dir, .prefix = "mc_cells", .fam = "border", .desc = { .type = T_U8 }, .eoff = { .type = T_U32 }, .exp = { .type = T_U16 }, .modes = { .type = T_I32 } };
        MCC_REFS(ref);
        /* (class along x, class along y) of the twelve side sets: L R T B, the corners LT RT LB RB, wholly outside L R T B */
        static const int sets[12][2] = { { 1, 0 }, { 2, 0 }, { 0, 1 }, { 0, 2 }, { 1, 1 }, { 2, 1 }, { 1, 2 }, { 2, 2 }, { 3, 0 }, { 4, 0 }, { 0, 3 }, { 0, 4 } };
        int n = 0;
        for (int chroma = 0; chroma <= 1; ++chroma)
            for (int l2w = 2; l2w <= 4; ++l2w)
                for (int l2h = 2; l2h <= 4; ++l2h)
                    for (int s = 0; s < 12; ++s)
                        for (int off = 0; off < 4; ++off) {
                            ovhip_pu_desc d;
                            memset(&d, 0, sizeof(d));
                            /* a unit wholly outside: of a PU of 32 where the unit's side is 16 (clip_mv keeps a PU's window
                             * within reach of the picture; only a unit further out in a larger PU leaves it for good) */
                            d.log2_w = (uint8_t)(sets[s][0] >= 3 && l2w == 4 ? 5 : l2w);
                            d.log2_h = (uint8_t)(sets[s][1] >= 3 && l2h == 4 ? 5 : l2h);
                            d.inter_dir = (uint8_t)(1 + n % 3); d.planes = 3;
                            d.ref_idx0 = n & 1; d.ref_idx1 = 0;
                            mcc_place(&d, n, 0);
                            int32_t mvx, mvy;
                            if (!mcc_find_mv(d.x0, 1 << d.log2_w, 1 << l2w, MC_W, chroma, sets[s][0], off, (5 * n + 3) & 15, 7 * n + 1, &mvx)) continue;
                            if (!mcc_find_mv(d.y0, 1 << d.log2_h, 1 << l2h, MC_H, chroma, sets[s][1], -1, (3 * n + 6) & 15, 5 * n + 2, &mvy)) continue;
                            const int a = d.inter_dir == 2 || (d.inter_dir == 3 && (n & 2));        /* the list the case is about */
                            int32_t ox = rnd_range(-70, 70), oy = rnd_range(-70, 70);
                            if (a) { d.mv1x = mvx; d.mv1y = mvy; d.mv0x = ox; d.mv0y = oy; }
                            else   { d.mv0x = mvx; d.mv0y = mvy; d.mv1x = ox; d.mv1y = oy; }
                            mcc_case(&o, &M, &d, MCC_PLAIN, NULL, 0);
                            ++n;
                        }
        mcc_flush(&o);
    }
    #undef MCC_REFS
}

/* one DMVR PU (= one unit) through rcn_dmvr_mv_refine on the pictures of mcx.ovg's lists: rpl0 = { 0, 2 }, rpl1 = { 1, 0 } */
static void
mcxc_run(struct mcc_out *o, OVCTUDec *c, ovhip_pu_desc *d)
{
    struct InterDRVCtx *ic = &c->drv_ctx.inter_ctx;
    const struct OVBuffInfo *cb = &c->rcn_ctx.ctu_buff;
    static const uint8_t slot0[2] = { 0, 2 }, slot1[2] = { 1, 0 };
    d->poc0 = ic->rpl0[d->ref_idx0]->poc; d->poc1 = ic->rpl1[d->ref_idx1]->poc;
    d->ref0 = slot0[d->ref_idx0]; d->ref1 = slot1[d->ref_idx1];
    c->ctb_x = d->x0 >> 7; c->ctb_y = d->y0 >> 7;
    ic->prec_amvr = d->prec_amvr_half ? MV_PRECISION_HALF : 0;
    mcc_fill(cb);
    OVMV m0 = { .x = d->mv0x, .y = d->mv0y, .ref_idx = d->ref_idx0 }, m1 = { .x = d->mv1x, .y = d->mv1y, .ref_idx = d->ref_idx1 };
    c->rcn_funcs.rcn_dmvr_mv_refine(c, *cb, d->x0 & 127, d->y0 & 127, d->log2_w, d->log2_h, &m0, &m1, d->ref_idx0, d->ref_idx1, d->refine & OVHIP_PU_BDOF);
    uint32_t eoff[4];
    eoff[3] = (uint32_t)o->mv.n;
    int32_t out[4] = { m0.x, m0.y, m1.x, m1.y };
    gbuf_push(&o->mv, out, 4);
    mcc_dump(o, cb, d, eoff);
    gbuf_push(&o->desc, d, sizeof(*d));
    gbuf_push(&o->eoff, eoff, 4);
    o->n++;
}

static void
gen_mcx_cells(const char *dir)
{
    g_seed = 0x266 + 77;                                      /* mcx.ovg's seed: the first draws are its three pictures */
    OVCTUDec *c = ref_new_ctudec(0, 0);
    struct InterDRVCtx *ic = &c->drv_ctx.inter_ctx;
    OVPicture *ref[3];
    mcx_make_refs(ref);
    g_seed = 0x266 + 877;                                     /* this generator's own */
    ic->rpl0[0] = ref[0]; ic->rpl0[1] = ref[2]; ic->rpl1[0] = ref[1]; ic->rpl1[1] = ref[0];
    for (int i = 0; i < 16; ++i) {
        ic->scale_fact_rpl0[i][0] = ic->scale_fact_rpl0[i][1] = 1 << RPR_SCALE_BITS;
        ic->scale_fact_rpl1[i][0] = ic->scale_fact_rpl1[i][1] = 1 << RPR_SCALE_BITS;
    }
    static const int shapes[3][2] = { { 3, 4 }, { 4, 3 }, { 4, 4 } };
    for (int fam = 0; fam < 2; ++fam) {
        struct mcc_out o = { .dir = dir, .prefix = "mcx_cells", .fam = fam ? "limit" : "far", .with_mv = 1, .desc = { .type = T_U8 }, .eoff = { .type = T_U32 },
                             .exp = { .type = T_U16 }, .modes = { .type = T_I32 }, .mv = { .type = T_I32 } };
        int n = 0;
        for (int sh = 0; sh < 3; ++sh)
            for (int refine = 2; refine <= 3; ++refine)
                for (int s0 = 0; s0 < 4 + 4 * fam; ++s0)                      /* list 0: left, right, top, bottom (limit: the corner of signs, twice) */
                    for (int s1 = 0; s1 < 5; ++s1, ++n) {                     /* list 1: within range, or one of the four (limit: its corner of signs) */
                        ovhip_pu_desc d;
                        memset(&d, 0, sizeof(d));
                        d.log2_w = shapes[sh][0]; d.log2_h = shapes[sh][1]; d.inter_dir = 3; d.planes = 3; d.refine = (uint8_t)refine;
                        d.ref_idx0 = n % 6 == 5; d.ref_idx1 = n % 8 == 7;
                        d.prec_amvr_half = n % 5 == 2;
                        mcc_place(&d, n, 0);
                        const int w = 1 << d.log2_w, h = 1 << d.log2_h;
                        int32_t mv[2][2];
                        for (int l = 0; l < 2; ++l) {
                            const int side = l ? s1 - 1 : s0;
                            mv[l][0] = rnd_range(-40, 40); mv[l][1] = rnd_range(-40, 40);
                            if (fam == 0) {
                                /* beyond clip_mv's range by a fraction of a sample, or by whole samples */
                                const int past = n % 3 == 0 ? 1 + n % 15 : 16 * (1 + n % 40) + rnd_range(0, 15);
                                if (side == 0) mv[l][0] = -((w + 3 + d.x0) << 4) - past;
                                if (side == 1) mv[l][0] = ((MC_W + 2 - d.x0) << 4) + past;
                                if (side == 2) mv[l][1] = -((h + 3 + d.y0) << 4) - past;
                                if (side == 3) mv[l][1] = ((MC_H + 2 - d.y0) << 4) + past;
                                if (l && side < 0) { mv[1][0] = -(mv[0][0] % 64) + rnd_range(-20, 20); mv[1][1] = -(mv[0][1] % 64) + rnd_range(-20, 20); }
                            } else {
                                /* within a few sixteenths of +-2^17 in one or both components */
                                const int sx = (l ? s1 : s0) & 1 ? 1 : -1, sy = (l ? s1 : s0) & 2 ? 1 : -1, e = rnd_range(0, 24);
                                if ((n + l) % 3 != 1) mv[l][0] = sx > 0 ? (1 << 17) - 1 - e : -(1 << 17) + e;
                                if ((n + l) % 3 != 2) mv[l][1] = sy > 0 ? (1 << 17) - 1 - e / 2 : -(1 << 17) + e / 2;
                            }
                        }
                        d.mv0x = mv[0][0]; d.mv0y = mv[0][1]; d.mv1x = mv[1][0]; d.mv1y = mv[1][1];
                        mcxc_run(&o, c, &d);
                    }
        mcc_flush(&o);
    }

    /* ---- paint: a pair of pictures made for the search's branches, in regions of 26 x 24 -- smooth content, rows that are flat, columns
     * that are flat, a constant, a step edge; the second picture is the first displaced by a whole (dx, dy) of -2..2 per region plus
     * noise of a per-region amplitude around the two cost thresholds (0: an exact copy; a constant region: offset by 0..6 instead).
     * The cases are a table: 400000 random candidates (position, shape, vectors mirrored with a little jitter, some on whole samples)
     * were once traced through the oracle and the 41 kept that reached an outcome of the search no earlier one had (early exit,
     * arg-min index, tie kind, sub-pel branch per axis, +-7, BDOF kept or switched off by the cost); tests/mc_census.py says what
     * each reaches now.  Two constant regions near the ends of the sample range, noisy enough for BDOF to stay on, clip its output. ---- */
    {
        OVPicture *paint[3];
        for (int i = 0; i < 3; ++i) {
            paint[i] = ref_new_picture(MC_W, MC_H, i == 0 ? 8 : (i == 1 ? 24 : 4));
            for (int p = 0; p < 3; ++p) fill_plane(paint[i]->frame->data[p], MC_W >> !!p, MC_H >> !!p, MC_W >> !!p);
        }
        uint16_t *a = (uint16_t *)paint[0]->frame->data[0], *b = (uint16_t *)paint[1]->frame->data[0];
        static int typ[40], shx[40], shy[40], amp[40], va[40], vb[40];
        static const int amps[8] = { 0, 0, 1, 2, 3, 5, 8, 12 };
        for (int k = 0; k < 40; ++k) {
            typ[k] = k % 5; shx[k] = rnd_range(-2, 2); shy[k] = rnd_range(-2, 2); amp[k] = amps[rnd_range(0, 7)];
            va[k] = rnd_range(100, 900); vb[k] = va[k] + rnd_range(-200, 200);
        }
        #define REGION(x, y) (((y) / 24) * 8 + (x) / 26)
        for (int y = 0; y < MC_H; ++y)
            for (int x = 0; x < MC_W; ++x) {
                const int k = REGION(x, y);
                if (typ[k] == 1) a[y * MC_W + x] = a[y * MC_W + (x / 26) * 26];                   /* flat rows */
                if (typ[k] == 2) a[y * MC_W + x] = a[(y / 24) * 24 * MC_W + x];                   /* flat columns */
                if (typ[k] == 3) a[y * MC_W + x] = (uint16_t)va[k];
                if (typ[k] == 4) a[y * MC_W + x] = (uint16_t)(x % 26 < 13 ? va[k] : vb[k]);
            }
        for (int y = 0; y < MC_H; ++y)
            for (int x = 0; x < MC_W; ++x) {
                const int k = REGION(x, y);
                int sx = x + shx[k], sy = y + shy[k];
                sx = sx < 0 ? 0 : sx >= MC_W ? MC_W - 1 : sx; sy = sy < 0 ? 0 : sy >= MC_H ? MC_H - 1 : sy;
                int v = typ[k] == 3 ? va[k] + k % 7 : a[sy * MC_W + sx] + (amp[k] ? rnd_range(-amp[k], amp[k]) : 0);
                b[y * MC_W + x] = (uint16_t)(v < 0 ? 0 : v > 1023 ? 1023 : v);
            }
        #undef REGION
        /* a zero denominator of the sub-pel step takes three equal costs around the minimum, and beside a minimum anywhere but at the
         * centre the lower index would have won: the centre's cost (three quarters of its SAD) has to equal both neighbours'.  Two
         * constant regions carry an offset profile made for that, for an 8x16 unit at (88, 4) along x and a 16x16 unit at (4, 28)
         * along y (every second row counts): a shift by one sample either way lowers the SAD by exactly a quarter, by two raises it. */
        for (int y = 0; y < 24; ++y)
            for (int x = 78; x < 104; ++x) {
                const int j = x - 88, g = j == 0 || j == 7 ? 6 : j > 0 && j < 7 ? 2 : j == -1 || j == 8 ? 0 : 20;
                b[y * MC_W + x] = (uint16_t)(va[3] + g);
            }
        for (int y = 24; y < 48; ++y)
            for (int x = 0; x < 26; ++x) {
                const int j = y - 28, g = j == -1 || j == 15 ? 4 : j < -1 || j > 15 ? 20 : j & 1 ? 2 : 3;
                b[y * MC_W + x] = (uint16_t)(va[8] + g);
            }
        /* BDOF's output clips: both pictures within 40 of an end of the range, independently drawn, in two regions no case of the
         * table reads (high at (52, 0), low at (182, 96)) */
        for (int hi = 0; hi <= 1; ++hi)
            for (int y = hi ? 0 : 96; y < (hi ? 24 : 120); ++y)
                for (int x = hi ? 52 : 182; x < (hi ? 78 : 208); ++x) {
                    a[y * MC_W + x] = (uint16_t)(hi ? 1023 - rnd_range(0, 39) : rnd_range(0, 39));
                    b[y * MC_W + x] = (uint16_t)(hi ? 1023 - rnd_range(0, 39) : rnd_range(0, 39));
                }
        ic->rpl0[0] = paint[0]; ic->rpl0[1] = paint[2]; ic->rpl1[0] = paint[1]; ic->rpl1[1] = paint[0];
        struct mcc_out o = { .dir = dir, .prefix = "mcx_cells", .fam = "paint", .with_mv = 1, .desc = { .type = T_U8 }, .eoff = { .type = T_U32 },
                             .exp = { .type = T_U16 }, .modes = { .type = T_I32 }, .mv = { .type = T_I32 }, .ref = paint };
        static const int16_t found[41][9] = {      /* log2_w, log2_h, refine, x0, y0, mv0x, mv0y, mv1x, mv1y */
            { 3, 4, 2, 20, 0, 0, 32, 0, -32 }, { 4, 3, 2, 176, 44, 0, -16, 0, 16 }, { 3, 4, 2, 128, 36, -33, -9, 33, 9 },
            { 4, 3, 3, 56, 84, -48, 0, 48, 0 }, { 3, 4, 3, 200, 56, 16, 0, -16, 0 }, { 4, 4, 2, 20, 12, -5, -13, 5, 13 },
            { 4, 4, 3, 16, 52, -23, -34, 39, 21 }, { 4, 4, 2, 60, 76, 21, 7, -21, -7 }, { 4, 3, 3, 64, 56, 16, 0, -16, 0 },
            { 3, 4, 2, 160, 8, -16, 21, 6, -14 }, { 4, 3, 3, 180, 40, 15, -38, -28, 38 }, { 3, 4, 2, 136, 60, 16, -29, -7, 43 },
            { 4, 3, 3, 144, 32, -22, -17, 22, 17 }, { 3, 4, 2, 84, 88, -16, 0, 16, 0 }, { 3, 4, 3, 156, 0, -32, -16, 32, 16 },
            { 4, 3, 2, 100, 112, 11, 18, -2, -37 }, { 3, 4, 2, 8, 88, -16, 0, 16, 0 }, { 4, 4, 2, 112, 8, 9, 37, -9, -37 },
            { 3, 4, 3, 48, 60, 14, 30, -14, -30 }, { 3, 4, 2, 96, 104, 16, 16, -16, -16 }, { 3, 4, 2, 32, 32, 18, 25, -28, -22 },
            { 4, 4, 2, 52, 28, 22, -40, -13, 29 }, { 3, 4, 3, 152, 72, -16, 32, 16, -32 }, { 4, 3, 2, 84, 108, 17, -14, -17, 14 },
            { 4, 3, 3, 24, 36, 17, -21, -17, 21 }, { 4, 4, 2, 104, 28, -16, 0, 16, 0 }, { 4, 3, 3, 128, 72, -48, 0, 48, 0 },
            { 4, 3, 3, 4, 32, 16, -16, -16, 16 }, { 3, 4, 2, 104, 4, 23, -13, -10, 31 }, { 4, 4, 2, 140, 88, 1, -13, -4, 23 },
            { 3, 4, 2, 168, 8, -48, -16, 48, 16 }, { 4, 3, 2, 156, 96, 0, 16, 0, -16 }, { 3, 4, 2, 92, 100, -16, 0, 16, 0 },
            { 4, 4, 3, 156, 52, 0, -32, 0, 32 }, { 4, 4, 3, 176, 32, 11, -2, -15, 14 }, { 3, 4, 3, 56, 84, -32, 0, 32, 0 },
            { 4, 4, 3, 4, 28, -24, -15, 36, 19 }, { 3, 4, 3, 0, 28, 21, 3, -21, -3 }, { 4, 4, 3, 4, 28, 0, 0, 0, 0 },
            { 4, 3, 3, 140, 24, 23, 1, -26, 0 }, { 3, 4, 2, 88, 4, 0, 32, 0, -32 },
        };
        for (int k = 0; k < 41; ++k) {
            ovhip_pu_desc d;
            memset(&d, 0, sizeof(d));
            d.log2_w = (uint8_t)found[k][0]; d.log2_h = (uint8_t)found[k][1]; d.inter_dir = 3; d.planes = 3; d.refine = (uint8_t)found[k][2];
            d.x0 = (uint16_t)found[k][3]; d.y0 = (uint16_t)found[k][4];
            d.mv0x = found[k][5]; d.mv0y = found[k][6]; d.mv1x = found[k][7]; d.mv1y = found[k][8];
            mcxc_run(&o, c, &d);
        }
        for (int k = 0; k < 2; ++k) {                                        /* the two zero-denominator cases */
            ovhip_pu_desc d;
            memset(&d, 0, sizeof(d));
            d.log2_w = k ? 4 : 3; d.log2_h = 4; d.inter_dir = 3; d.planes = 3; d.refine = OVHIP_PU_DMVR;
            d.x0 = k ? 4 : 88; d.y0 = k ? 28 : 4;
            mcxc_run(&o, c, &d);
        }
        for (int sh = 0; sh < 3; ++sh)                                      /* BDOF's output clips, at 1023 and at 0 */
            for (int k = 0; k < 8; ++k) {
                ovhip_pu_desc d;
                memset(&d, 0, sizeof(d));
                d.log2_w = shapes[sh][0]; d.log2_h = shapes[sh][1]; d.inter_dir = 3; d.planes = 3; d.refine = OVHIP_PU_DMVR | OVHIP_PU_BDOF;
                d.x0 = (uint16_t)((k & 1 ? 184 : 56) + 4 * ((k >> 1) & 1)); d.y0 = (uint16_t)((k & 1 ? 100 : 4) + 4 * (k >> 2) * (shapes[sh][1] == 3));
                d.mv0x = 3 + 2 * k; d.mv0y = 5 - k; d.mv1x = -d.mv0x + (k >> 2); d.mv1y = -d.mv0y;
                mcxc_run(&o, c, &d);
            }
        mcc_flush(&o);
    }
}

/* ====================================================================================== DBF */
#include "dbf_utils.h"
#include "drv_lines.h"
#include "slicedec.h"

static void
snapshot_dbf(ovhip_dbf_ctu *o, const struct DBFInfo *d)
{
    memset(o, 0, sizeof(*o));
    memcpy(o->ctb_bound_ver, d->ctb_bound_ver, sizeof(o->ctb_bound_ver));
    memcpy(o->ctb_bound_hor, d->ctb_bound_hor, sizeof(o->ctb_bound_hor));
    memcpy(o->ctb_bound_ver_c, d->ctb_bound_ver_c, sizeof(o->ctb_bound_ver_c));
    memcpy(o->ctb_bound_hor_c, d->ctb_bound_hor_c, sizeof(o->ctb_bound_hor_c));
    memcpy(o->aff_edg_ver, d->aff_edg_ver, sizeof(o->aff_edg_ver));
    memcpy(o->aff_edg_hor, d->aff_edg_hor, sizeof(o->aff_edg_hor));
    memcpy(o->bs2_ver, d->bs2_map.ver, sizeof(o->bs2_ver));       memcpy(o->bs2_hor, d->bs2_map.hor, sizeof(o->bs2_hor));
    memcpy(o->bs2c_ver, d->bs2_map_c.ver, sizeof(o->bs2c_ver));   memcpy(o->bs2c_hor, d->bs2_map_c.hor, sizeof(o->bs2c_hor));
    memcpy(o->bs1_ver, d->bs1_map.ver, sizeof(o->bs1_ver));       memcpy(o->bs1_hor, d->bs1_map.hor, sizeof(o->bs1_hor));
    memcpy(o->bs1cb_ver, d->bs1_map_cb.ver, sizeof(o->bs1cb_ver)); memcpy(o->bs1cb_hor, d->bs1_map_cb.hor, sizeof(o->bs1cb_hor));
    memcpy(o->bs1cr_ver, d->bs1_map_cr.ver, sizeof(o->bs1cr_ver)); memcpy(o->bs1cr_hor, d->bs1_map_cr.hor, sizeof(o->bs1cr_hor));
    memcpy(o->affine_ver, d->affine_map.ver, sizeof(o->affine_ver)); memcpy(o->affine_hor, d->affine_map.hor, sizeof(o->affine_hor));
    memcpy(o->qp_y, d->qp_map_y.hor, sizeof(o->qp_y));
    memcpy(o->qp_cb, d->qp_map_cb.hor, sizeof(o->qp_cb));
    memcpy(o->qp_cr, d->qp_map_cr.hor, sizeof(o->qp_cr));
    o->beta_offset = d->beta_offset; o->tc_offset = d->tc_offset;
    o->disable_v = d->disable_v; o->disable_h = d->disable_h;
}

/* random partition of a w x h region of one CTU into CUs; fills the deblocking maps the way the
 * decoder's parse loop does (vcl_coding_unit.c:742, vcl_transform_unit.c:1093-1146, :1934-1957,
 * rcn_transform_tree.c fill_bs_map calls, drv_affine_mvp.c:3052-3082) and paints a DC offset per CU
 * into the unfiltered picture so that block edges are visible to the filter decisions */
struct dbf_gen { struct DBFInfo *d; uint16_t *y, *cb, *cr; int stride, stride_c; int px, py; OVCTUDec *c; int bmode; struct IBCMVCtx *ibc; int pic_w, pic_h; };

/* second profile ("dbf_ends" -> dbf_ends.ovg): content, QPs, offsets and partition chosen so that the reference takes the long luma
 * filters, both ends of the threshold tables, the bit-depth clips and the CTU-boundary strong chroma filter.  The first profile
 * draws exactly the random numbers it always drew: every draw the second one adds sits behind this flag. */
static int g_dbf_ends;

static inline int clip_pix(int v) { return v < 0 ? 0 : v > 1023 ? 1023 : v; }

/* "ends" content of one CU: absolute sample values, not an offset on a textured picture.  Most CUs are flat or a gentle ramp
 * around a level that drifts slowly over the picture, so neighbouring CUs differ by a few codes (the long / strong decisions
 * pass); some are noisy (off / weak); inside two vertical bands of the picture most CUs are pinned at 0..8 or 1015..1023. */
static int
paint_cu_ends(struct dbf_gen *g, int x, int y, int w, int h)
{
    const int ax = g->px + x, ay = g->py + y;
    int mode = rnd_range(0, 99);                       /* < 75 flat, < 85 ramp, else noise */
    if ((w >= 32 || h >= 32) && rnd_range(0, 9) < 7) mode = 0;     /* the blocks the long filters apply to: flat more often */
    int pin = 0;
    if (ax >= g->pic_w * 5 / 8 && ax < g->pic_w * 7 / 8 && rnd_range(0, 9) < 8) pin = ax < g->pic_w * 3 / 4 ? 1 : 2;
    const int big = rnd_range(0, 7) == 0;              /* a step large enough for the tc gates of high QPs */
    const int level = 420 + (ax >> 5) - (ay >> 5) + (big ? rnd_range(-70, 70) : rnd_range(-3, 3));
    const int level_c = 500 - (ax >> 5) + (ay >> 4) + (big ? rnd_range(-40, 40) : rnd_range(-4, 4));
    const int sx = rnd_range(-2, 2), sy = rnd_range(-2, 2), amp = rnd_range(4, 70);
    const int pin_flat = rnd_range(0, 1), pin_v = rnd_range(0, 3);
    for (int j = 0; j < h; ++j) for (int i = 0; i < w; ++i) {
        int v;
        if (pin)            v = pin_flat ? pin_v : rnd_range(0, 8);
        else if (mode < 75) v = level;
        else if (mode < 85) v = level + ((i * sx + j * sy) >> 2);
        else                v = level + rnd_range(-amp, amp);
        if (pin == 2) v = 1023 - v;
        g->y[(ay + j) * g->stride + ax + i] = clip_pix(v);
    }
    for (int j = 0; j < h / 2; ++j) for (int i = 0; i < w / 2; ++i) {
        int o = (ay / 2 + j) * g->stride_c + ax / 2 + i, v, u;
        if (pin)            { v = pin_flat ? pin_v : rnd_range(0, 8); u = pin_flat ? 3 - pin_v : rnd_range(0, 8); }
        else if (mode < 75) { v = level_c; u = 1023 - level_c; }
        else if (mode < 85) { v = level_c + ((i * sx + j * sy) >> 1); u = 1023 - v; }
        else                { v = level_c + rnd_range(-amp / 2, amp / 2); u = 1023 - level_c + rnd_range(-amp / 2, amp / 2); }
        if (pin == 2) { v = 1023 - v; u = 1023 - u; }
        g->cb[o] = clip_pix(v); g->cr[o] = clip_pix(u);
    }
    return pin;
}

/* B-slice mode: the CU's motion goes into inter_ctx->mv_ctx0/1 (maps + 34x34 vectors, PB_POS_IN_BUF layout) the way
 * update_mv_ctx_b does; the MV-based bS pre-pass inside rcn_dbf_ctu then derives bS 1 itself */
static void
gen_cu_motion(struct dbf_gen *g, int x, int y, int w, int h, int intra)
{
    struct InterDRVCtx *ic = &g->c->drv_ctx.inter_ctx;
    int x0 = x >> 2, y0 = y >> 2, nw = w >> 2, nh = h >> 2;
    uint64_t mh = (((uint64_t)1 << nw) - 1) << (x0 + 1), mv_ = (((uint64_t)1 << nh) - 1) << (y0 + 1);
    if (intra) return;
    if (rnd_range(0, 15) == 0) {                       /* IBC CU: no inter motion, IBC map set */
        for (int j = 0; j < nh; ++j) g->ibc->ctu_map.hfield[y0 + 1 + j] |= mh;
        for (int i = 0; i < nw; ++i) g->ibc->ctu_map.vfield[x0 + 1 + i] |= mv_;
        return;
    }
    static const int pal[3][2] = { { 40, -24 }, { 44, -20 }, { -96, 130 } };
    int lists = rnd_range(1, 3);
    for (int l = 0; l < 2; ++l) {
        if (!(lists & (1 << l))) continue;
        struct OVMVCtx *m = l ? &ic->mv_ctx1 : &ic->mv_ctx0;
        int k = rnd_range(0, 2);
        OVMV mv = { .x = pal[k][0] + rnd_range(-6, 6), .y = pal[k][1] + rnd_range(-6, 6), .ref_idx = rnd_range(0, 2) };
        for (int j = 0; j < nh; ++j) { m->map.hfield[y0 + 1 + j] |= mh; for (int i = 0; i < nw; ++i) m->mvs[35 + x0 + i + (y0 + j) * 34] = mv; }
        for (int i = 0; i < nw; ++i) m->map.vfield[x0 + 1 + i] |= mv_;
    }
}

static void
gen_cu(struct dbf_gen *g, int x, int y, int w, int h)
{
    struct DBFInfo *d = g->d;
    int l2w = 31 - __builtin_clz(w), l2h = 31 - __builtin_clz(h);
    const int ends = g_dbf_ends;
    int qp = ends ? (rnd_range(0, 2) ? rnd_range(28, 63) : rnd_range(0, 63)) : rnd_range(18, 50);   /* ends: all of 0..63, the upper part more often */
    int intra = ends ? rnd_range(0, 4) == 0 : rnd_range(0, 9) == 0;
    int affine = !intra && w >= 16 && h >= 16 && rnd_range(0, 5) <= (ends && g->px + x < g->pic_w / 2 ? 4 : 0);   /* ends: affine CUs side by side in the left part: (5, 5) */
    int off_y = rnd_range(-40, 40), off_c = rnd_range(-24, 24);
    if (ends && (w >= 32 || h >= 32) && rnd_range(0, 9) < 6) qp = rnd_range(30, 63);   /* large blocks: more often a QP with tc > 0 */
    if (ends && paint_cu_ends(g, x, y, w, h)) qp = rnd_range(40, 63);      /* pinned CUs: a QP at which the weak filter is on */
    else for (int j = 0; j < h; ++j) for (int i = 0; i < w; ++i) {
        int v = g->y[(g->py + y + j) * g->stride + g->px + x + i] + off_y;
        g->y[(g->py + y + j) * g->stride + g->px + x + i] = v < 0 ? 0 : v > 1023 ? 1023 : v;
    }
    if (!ends) for (int j = 0; j < h / 2; ++j) for (int i = 0; i < w / 2; ++i) {
        int o = ((g->py + y) / 2 + j) * g->stride_c + (g->px + x) / 2 + i;
        int v = g->cb[o] + off_c; g->cb[o] = v < 0 ? 0 : v > 1023 ? 1023 : v;
        v = g->cr[o] - off_c;     g->cr[o] = v < 0 ? 0 : v > 1023 ? 1023 : v;
    }
    dbf_fill_cu_edge(&d->cu_edge, x >> 2, y >> 2, w >> 2, h >> 2);
    if (intra) { fill_bs_map(&d->bs2_map, x, y, l2w, l2h); fill_bs_map(&d->bs2_map_c, x, y, l2w, l2h); }
    if (g->bmode) gen_cu_motion(g, x, y, w, h, intra);
    else if (rnd_range(0, 2) == 0) {      /* "motion differs from the neighbours" (what dbf_ctu_preproc_* derives) */
        fill_bs_map(&d->bs1_map, x, y, l2w, l2h);
        if (rnd_range(0, 1)) fill_bs_map(&d->bs1_map_cb, x, y, l2w, l2h);
        if (rnd_range(0, 1)) fill_bs_map(&d->bs1_map_cr, x, y, l2w, l2h);
    }
    if (affine) {
        int x0_u = x >> 2, y0_u = y >> 2, nw = w >> 2, nh = h >> 2;
        uint64_t msk_v = (((uint64_t)1 << nh) - 1) << y0_u, msk_h = (((uint64_t)1 << nw) - 1) << (2 + x0_u);
        for (int i = 2; i < nw; i += 2) { d->aff_edg_ver[8 + x0_u + i] |= msk_v; if (rnd_range(0, 1)) d->bs1_map.ver[x0_u + i] |= msk_v & ((uint64_t)rnd32() << 32 | rnd32() << 8 | rnd32()); }
        for (int i = 2; i < nh; i += 2) { d->aff_edg_hor[8 + y0_u + i] |= msk_h; if (rnd_range(0, 1)) d->bs1_map.hor[y0_u + i] |= msk_h & ((uint64_t)rnd32() << 32 | rnd32() << 8 | rnd32()); }
        dbf_fill_aff_map(&d->affine_map, x0_u, y0_u, nw, nh);
    }
    /* transform units: split at 64 */
    for (int ty = 0; ty < h; ty += 64) for (int tx = 0; tx < w; tx += 64) {
        int tl2w = l2w > 6 ? 6 : l2w, tl2h = l2h > 6 ? 6 : l2h;
        fill_ctb_bound(d, x + tx, y + ty, tl2w, tl2h);
        fill_ctb_bound_c(d, x + tx, y + ty, tl2w, tl2h);
        dbf_fill_qp_map(&d->qp_map_y, x + tx, y + ty, tl2w, tl2h, qp);
        /* "ends": the chroma QPs cover 0..63 as well, up to 9 away from the luma QP on either side */
        int qp_cb = ends ? qp + rnd_range(-9, 9) : qp - rnd_range(0, 3), qp_cr = ends ? qp + rnd_range(-9, 9) : qp - rnd_range(0, 3);
        if (ends) { qp_cb = qp_cb < 0 ? 0 : qp_cb > 63 ? 63 : qp_cb; qp_cr = qp_cr < 0 ? 0 : qp_cr > 63 ? 63 : qp_cr; }
        dbf_fill_qp_map(&d->qp_map_cb, x + tx, y + ty, tl2w, tl2h, qp_cb);
        dbf_fill_qp_map(&d->qp_map_cr, x + tx, y + ty, tl2w, tl2h, qp_cr);
        if (rnd_range(0, 1)) fill_bs_map(&d->bs1_map, x + tx, y + ty, tl2w, tl2h);          /* cbf luma */
        if (rnd_range(0, 2) == 0) fill_bs_map(&d->bs1_map_cb, x + tx, y + ty, tl2w, tl2h);  /* cbf cb   */
        if (rnd_range(0, 2) == 0) fill_bs_map(&d->bs1_map_cr, x + tx, y + ty, tl2w, tl2h);  /* cbf cr   */
    }
}

static void
gen_part(struct dbf_gen *g, int x, int y, int w, int h, int lim_w, int lim_h)
{
    if (x >= lim_w || y >= lim_h) return;
    if (x + w > lim_w || y + h > lim_h) {
        if (w > 4 && x + w > lim_w && !(h > 4 && y + h > lim_h)) { gen_part(g, x, y, w / 2, h, lim_w, lim_h); gen_part(g, x + w / 2, y, w / 2, h, lim_w, lim_h); }
        else if (h > 4 && y + h > lim_h && !(w > 4 && x + w > lim_w)) { gen_part(g, x, y, w, h / 2, lim_w, lim_h); gen_part(g, x, y + h / 2, w, h / 2, lim_w, lim_h); }
        else { gen_part(g, x, y, w / 2, h / 2, lim_w, lim_h); gen_part(g, x + w / 2, y, w / 2, h / 2, lim_w, lim_h);
               gen_part(g, x, y + h / 2, w / 2, h / 2, lim_w, lim_h); gen_part(g, x + w / 2, y + h / 2, w / 2, h / 2, lim_w, lim_h); }
        return;
    }
    int m = w > h ? w : h;
    static const int p_split[8] = { 0, 0, 0, 15, 45, 65, 85, 95 };   /* % by log2(max dim): 8->15 .. 128->95 */
    static const int p_split_ends[8] = { 0, 0, 0, 10, 25, 40, 80, 97 };   /* blocks of 32 and more on both sides of many edges */
    if (m > 4 && rnd_range(0, 99) < (g_dbf_ends ? p_split_ends : p_split)[31 - __builtin_clz(m)]) {
        int k = rnd_range(0, 3);
        if (k < 2 && w == h && w > 4) { gen_part(g, x, y, w / 2, h / 2, lim_w, lim_h); gen_part(g, x + w / 2, y, w / 2, h / 2, lim_w, lim_h);
                                        gen_part(g, x, y + h / 2, w / 2, h / 2, lim_w, lim_h); gen_part(g, x + w / 2, y + h / 2, w / 2, h / 2, lim_w, lim_h); }
        else if ((k == 2 && w > 4) || h <= 4) { gen_part(g, x, y, w / 2, h, lim_w, lim_h); gen_part(g, x + w / 2, y, w / 2, h, lim_w, lim_h); }
        else { gen_part(g, x, y, w, h / 2, lim_w, lim_h); gen_part(g, x, y + h / 2, w, h / 2, lim_w, lim_h); }
        return;
    }
    gen_cu(g, x, y, w, h);
}

/* ends = 1: the second profile (g_dbf_ends above), reference mode only.  Its pictures are smaller (a fixture file stays below
 * 1 MiB) and their CTUs carry (beta, tc) offset pairs from a per-picture table, as if every CTU began a new slice: picture 0 has
 * 3 x 3 CTUs with 8 distinct pairs (the 9th CTU has the first one's again), picture 1 2 x 2 CTUs with 3, picture 2 (B slice) a single pair so that the dense planes exist. */
static void
gen_dbf(const char *dir, int ends)
{
    enum { NPIC = 3 };
    static const int PW0[NPIC] = { 304, 264, 256 }, PH0[NPIC] = { 200, 136, 192 };     /* picture 2: B slice, motion-derived bS */
    static const int PW1[NPIC] = { 264, 136, 136 }, PH1[NPIC] = { 264, 200, 136 };
    /* (beta_offset, tc_offset) = sh_luma_{beta,tc}_offset_div2 * 2: both ends of -24..24, mixed signs.  Every pair leaves a window of
     * QPs in which both limits are above 0 (with the reference's tables (24, -24) has none, (-24, 24) only QP 40 and 41: beta is 0 from
     * index 64 on), so that every pair index can be seen to change samples */
    static const int8_t pairs[NPIC][8][2] = {
        { { -24, 12 }, { 20, -20 }, { 0, 0 }, { 24, 24 }, { -24, -24 }, { 6, -2 }, { -10, 14 }, { 12, -24 } },
        { { 24, 24 }, { -12, 8 }, { 4, -20 } },
        { { 2, 4 } } };
    static const int n_pairs[NPIC] = { 8, 3, 1 };
    const int *PW = ends ? PW1 : PW0, *PH = ends ? PH1 : PH0;
    if (ends && g_shim) return;
    g_dbf_ends = ends;
    gfile g = gfile_open(dir, ends ? "dbf_ends.ovg" : g_shim ? "shim_dbf.ovg" : "dbf.ovg");
    g_seed = 0x266 + 2 + 47 * ends;     /* ends: a seed at which the reference's pictures meet the census tests/test_dbf_spec_cpu.py asserts */
    for (int pi = 0; pi < NPIC; ++pi) {
        const int W = PW[pi], H = PH[pi], nx = (W + 127) / 128, ny = (H + 127) / 128;
        uint16_t *y = malloc(W * H * 2), *cb = malloc(W * H / 2), *cr = malloc(W * H / 2);
        fill_plane(y, W, H, W); fill_plane(cb, W / 2, H / 2, W / 2); fill_plane(cr, W / 2, H / 2, W / 2);
        /* very smooth content so that beta decisions pass often: low-pass once more */
        for (int j = 0; j < H; ++j) for (int i = 1; i < W; ++i) y[j * W + i] = (y[j * W + i] + 3 * y[j * W + i - 1] + 2) >> 2;
        for (int j = 1; j < H; ++j) for (int i = 0; i < W; ++i) y[j * W + i] = (y[j * W + i] + 3 * y[(j - 1) * W + i] + 2) >> 2;
        for (int j = 0; j < H / 2; ++j) for (int i = 1; i < W / 2; ++i) { cb[j * (W / 2) + i] = (cb[j * (W / 2) + i] + 3 * cb[j * (W / 2) + i - 1] + 2) >> 2; cr[j * (W / 2) + i] = (cr[j * (W / 2) + i] + 3 * cr[j * (W / 2) + i - 1] + 2) >> 2; }
        for (int j = 1; j < H / 2; ++j) for (int i = 0; i < W / 2; ++i) { cb[j * (W / 2) + i] = (cb[j * (W / 2) + i] + 3 * cb[(j - 1) * (W / 2) + i] + 2) >> 2; cr[j * (W / 2) + i] = (cr[j * (W / 2) + i] + 3 * cr[(j - 1) * (W / 2) + i] + 2) >> 2; }

        OVCTUDec *c = ref_new_ctudec(0, 0);
        if (g_shim) shim_bind(c, W, H, 0, 0);
        struct DBFInfo *d = &c->dbf_info;
        const int bmode = pi == 2;
        c->tmp_slice_type = bmode ? 0 : 2;     /* I: the MV-based bS pre-pass is emulated by gen_cu(); B: rcn_dbf_ctu derives it */
        static struct IBCMVCtx ibc;
        d->ibc_ctx = &ibc;
        struct InterDRVCtx *ic = &c->drv_ctx.inter_ctx;
        static const int16_t dr0[16] = { -8, -16, 8, -24 }, dr1[16] = { 8, -8, 16, -16 };   /* POC distances: lists share pictures */
        memcpy(ic->dist_ref_0, dr0, sizeof(dr0)); memcpy(ic->dist_ref_1, dr1, sizeof(dr1));
        gbuf b_mv = { .type = T_U8 };
        struct DBFLines L;
        int npu = W / 4 + 40;
        L.qp_x_map = calloc(npu, 1); L.qp_x_map_cb = calloc(npu, 1); L.qp_x_map_cr = calloc(npu, 1);
        L.small_map = calloc(nx + 1, 8); L.dbf_bs2_hor = calloc(nx + 1, 8); L.dbf_bs2_hor_c = calloc(nx + 1, 8);
        L.dbf_bs1_hor = calloc(nx + 1, 8); L.dbf_bs1_hor_cb = calloc(nx + 1, 8); L.dbf_bs1_hor_cr = calloc(nx + 1, 8);
        L.dbf_affine = calloc(nx + 1, 8); L.large_map_c = calloc(nx + 1, 8);

        /* the partition pass paints block offsets into the picture, so do it first for all CTUs
         * into per-CTU map snapshots?  No: maps are CTU-local and rotated by load/store, so generate,
         * filter and snapshot CTU by CTU exactly in decoding order; the unfiltered picture is captured
         * from a second identical generation pass (same seed) that does not filter. */
        uint16_t *y0 = malloc(W * H * 2), *cb0 = malloc(W * H / 2), *cr0 = malloc(W * H / 2);
        gbuf b_ctu = { .type = T_U8 };
        uint32_t n_ctu = 0;
        for (int pass = 0; pass < 2; ++pass) {
            uint32_t seed_save = g_seed;
            uint16_t *ty = pass ? y : y0, *tcb = pass ? cb : cb0, *tcr = pass ? cr : cr0;
            if (!pass) { memcpy(y0, y, W * H * 2); memcpy(cb0, cb, W * H / 2); memcpy(cr0, cr, W * H / 2); }
            memset(d, 0, sizeof(*d));
            d->ibc_ctx = &ibc;
            d->beta_offset = (pi ? 2 : -2) * 2; d->tc_offset = (pi ? -1 : 3) * 2;
            memset(L.qp_x_map, 0, npu); memset(L.qp_x_map_cb, 0, npu); memset(L.qp_x_map_cr, 0, npu);
            memset(L.small_map, 0, (nx + 1) * 8); memset(L.dbf_bs2_hor, 0, (nx + 1) * 8); memset(L.dbf_bs2_hor_c, 0, (nx + 1) * 8);
            memset(L.dbf_bs1_hor, 0, (nx + 1) * 8); memset(L.dbf_bs1_hor_cb, 0, (nx + 1) * 8); memset(L.dbf_bs1_hor_cr, 0, (nx + 1) * 8);
            memset(L.dbf_affine, 0, (nx + 1) * 8); memset(L.large_map_c, 0, (nx + 1) * 8);
            for (int cy = 0; cy < ny; ++cy) {
                dbf_load_info(d, &L, 7, 0);
                for (int cx = 0; cx < nx; ++cx) {
                    int ctu_w = W - cx * 128 < 128 ? W - cx * 128 : 128, ctu_h = H - cy * 128 < 128 ? H - cy * 128 : 128;
                    struct dbf_gen gg = { d, ty, tcb, tcr, W, W / 2, cx * 128, cy * 128, c, bmode, &ibc, W, H };
                    if (ends) { const int8_t *pr = pairs[pi][(cy * nx + cx) % n_pairs[pi]]; d->beta_offset = pr[0]; d->tc_offset = pr[1]; }
                    if (bmode) {
                        /* fresh CTU motion context; the 1-unit border (row above / column left) stands in for what
                         * the line buffers would bring in from the neighbouring CTUs */
                        memset(&ic->mv_ctx0, 0, sizeof(ic->mv_ctx0)); memset(&ic->mv_ctx1, 0, sizeof(ic->mv_ctx1)); memset(&ibc, 0, sizeof(ibc));
                        for (int l = 0; l < 2; ++l) {
                            struct OVMVCtx *m = l ? &ic->mv_ctx1 : &ic->mv_ctx0;
                            for (int k = 0; k < 33; ++k) {
                                if (cy && rnd_range(0, 2)) { m->map.hfield[0] |= (uint64_t)1 << (k + 1); m->map.vfield[k + 1] |= 1;
                                                             m->mvs[1 + k] = (OVMV){ .x = 40 + rnd_range(-8, 8), .y = -24 + rnd_range(-8, 8), .ref_idx = rnd_range(0, 2) }; }
                                if (cx && rnd_range(0, 2)) { m->map.vfield[0] |= (uint64_t)1 << (k + 1); m->map.hfield[k + 1] |= 1;
                                                             m->mvs[34 + 34 * k] = (OVMV){ .x = 44 + rnd_range(-8, 8), .y = -20 + rnd_range(-8, 8), .ref_idx = rnd_range(0, 2) }; }
                            }
                        }
                    }
                    gen_part(&gg, 0, 0, 128, 128, ctu_w, ctu_h);
                    if (pass) {
                        c->ctu_ngh_flags = (cx ? CTU_LFT_FLG : 0) | (cy ? CTU_UP_FLG : 0);
                        c->ctb_x = cx; c->ctb_y = cy;
                        c->rcn_ctx.frame_buff.y = y + cy * 128 * W + cx * 128;
                        c->rcn_ctx.frame_buff.cb = cb + cy * 64 * (W / 2) + cx * 64;
                        c->rcn_ctx.frame_buff.cr = cr + cy * 64 * (W / 2) + cx * 64;
                        c->rcn_ctx.frame_buff.stride = W; c->rcn_ctx.frame_buff.stride_c = W / 2;
                        int last_x = cx == nx - 1, last_y = cy == ny - 1;
                        int truncated = ctu_w < 128 || ctu_h < 128;
                        ovhip_dbf_ctu o;
                        snapshot_dbf(&o, d);            /* BEFORE the slot: in a B slice it adds the motion-derived bS 1 to d */
                        if (bmode) {
                            ovhip_dbf_mv_ctx mc;
                            memset(&mc, 0, sizeof(mc));
                            memcpy(mc.cu_edge_ver, d->cu_edge.ver, sizeof(mc.cu_edge_ver)); memcpy(mc.cu_edge_hor, d->cu_edge.hor, sizeof(mc.cu_edge_hor));
                            memcpy(mc.map0_h, ic->mv_ctx0.map.hfield, sizeof(mc.map0_h)); memcpy(mc.map0_v, ic->mv_ctx0.map.vfield, sizeof(mc.map0_v));
                            memcpy(mc.map1_h, ic->mv_ctx1.map.hfield, sizeof(mc.map1_h)); memcpy(mc.map1_v, ic->mv_ctx1.map.vfield, sizeof(mc.map1_v));
                            memcpy(mc.ibc_h, ibc.ctu_map.hfield, sizeof(mc.ibc_h)); memcpy(mc.ibc_v, ibc.ctu_map.vfield, sizeof(mc.ibc_v));
                            memcpy(mc.dist_ref0, ic->dist_ref_0, sizeof(mc.dist_ref0)); memcpy(mc.dist_ref1, ic->dist_ref_1, sizeof(mc.dist_ref1));
                            mc.mv_bytes = sizeof(OVMV);
                            gbuf_push(&b_mv, &mc, sizeof(mc));
                            gbuf_push(&b_mv, ic->mv_ctx0.mvs, sizeof(ic->mv_ctx0.mvs));
                            gbuf_push(&b_mv, ic->mv_ctx1.mvs, sizeof(ic->mv_ctx1.mvs));
                        }
                        if (!truncated) TIMED(TS_DBF, c->rcn_funcs.df.rcn_dbf_ctu(&c->rcn_ctx, d, 7, last_x, last_y));
                        else            TIMED(TS_DBF, c->rcn_funcs.df.rcn_dbf_truncated_ctu(&c->rcn_ctx, d, 7, last_x, last_y, ctu_w, ctu_h));
                        o.log2_ctu_s = 7; o.last_x = last_x; o.last_y = last_y;
                        o.ctu_lft = !!cx; o.ctu_abv = !!cy;
                        o.ctu_w = truncated ? ctu_w : 0; o.ctu_h = truncated ? ctu_h : 0;
                        o.ctb_x = cx; o.ctb_y = cy;
                        gbuf_push(&b_ctu, &o, sizeof(o));
                        n_ctu++;
                    }
                    dbf_store_info(d, &L, 7, cx);
                    if (cx < nx - 1) dbf_load_info(d, &L, 7, cx + 1);
                }
            }
            if (!pass) g_seed = seed_save;      /* replay the same partition in the filtering pass */
        }
        /* pass 0 painted y0; pass 1 painted y identically then filtered it */
        char nm[32];
        if (g_shim) {
            /* what the installed df.rcn_dbf_ctu / rcn_dbf_truncated_ctu slots recorded for the whole picture */
            if (ovhip_shim_last_error(c)) { fprintf(stderr, "shim: dbf picture %d latched %d\n", pi, ovhip_shim_last_error(c)); exit(1); }
            ovhip_recorder *r = ovhip_shim_recorder(c);
            ovhip_dbf_offsets offs;
            for (int dir2 = 0; dir2 < 2; ++dir2) {
                size_t ne = 0;
                const ovhip_dbf_edge *ed = ovhip_rec_dbf_edges(r, dir2, &ne, &offs);
                uint32_t de[2] = { (uint32_t)ne, sizeof(ovhip_dbf_edge) };
                snprintf(nm, 32, "p%d_edges_%c", pi, dir2 ? 'h' : 'v'); gfile_array(&g, nm, T_U8, ne ? (const void *)ed : (const void *)"", 2, de);
            }
            uint32_t dof = sizeof(offs);
            snprintf(nm, 32, "p%d_offsets", pi); gfile_array(&g, nm, T_I8, &offs, 1, &dof);
            continue;
        }
        uint32_t d2[2] = { H, W };
        snprintf(nm, 32, "p%d_in_y", pi); gfile_array(&g, nm, T_U16, y0, 2, d2);
        snprintf(nm, 32, "p%d_exp_y", pi); gfile_array(&g, nm, T_U16, y, 2, d2);
        d2[0] = H / 2; d2[1] = W / 2;
        snprintf(nm, 32, "p%d_in_cb", pi); gfile_array(&g, nm, T_U16, cb0, 2, d2);
        snprintf(nm, 32, "p%d_in_cr", pi); gfile_array(&g, nm, T_U16, cr0, 2, d2);
        snprintf(nm, 32, "p%d_exp_cb", pi); gfile_array(&g, nm, T_U16, cb, 2, d2);
        snprintf(nm, 32, "p%d_exp_cr", pi); gfile_array(&g, nm, T_U16, cr, 2, d2);
        d2[0] = n_ctu; d2[1] = sizeof(ovhip_dbf_ctu);
        snprintf(nm, 32, "p%d_ctus", pi); gfile_array(&g, nm, T_U8, b_ctu.data, 2, d2);
        if (bmode) { d2[1] = (uint32_t)(b_mv.n / n_ctu); snprintf(nm, 32, "p%d_mvctx", pi); gfile_array(&g, nm, T_U8, b_mv.data, 2, d2); }
        size_t diff = 0;
        for (int i = 0; i < W * H; ++i) diff += y[i] != y0[i];
        fprintf(stderr, "%s: picture %d %dx%d, %u CTUs, %zu luma samples changed by the reference\n", ends ? "dbf_ends.ovg" : "dbf.ovg", pi, W, H, n_ctu, diff);
    }
    gfile_close(&g);
    g_dbf_ends = 0;
}


/* ====================================================================================== SAO */
/* rcn_alloc_filter_buffers() (rcn_ctu.c:512-551) calls ov_malloc (ovmem.c is not built, see
 * oracle/Makefile); the harness performs the same sizing with plain calloc. */
static void
harness_alloc_filter_buffers(struct OVRCNCtx *rcn_ctx, int nb_ctu_w, int margin, int log2_ctb_s)
{
    struct OVFilterBuffers *fb = &rcn_ctx->filter_buffers;
    int ctu_s = 1 << log2_ctb_s;
    fb->margin = margin;
    for (int comp = 0; comp < 3; ++comp) {
        int ratio = comp ? 2 : 1;
        fb->filter_region_w[comp] = ctu_s / ratio;
        fb->filter_region_h[comp] = ctu_s / ratio;
        fb->filter_region_stride[comp] = ctu_s / ratio + 2 * margin;
        fb->filter_region_offset[comp] = margin * fb->filter_region_stride[comp] + margin;
        int ext = fb->filter_region_stride[comp] * (fb->filter_region_h[comp] + 2 * margin + 1);
        fb->filter_region[comp] = calloc(ext, sizeof(OVSample));
        fb->saved_cols[comp] = calloc(fb->filter_region_h[comp] * margin, sizeof(OVSample));
        fb->saved_rows_stride[comp] = nb_ctu_w * ctu_s / ratio;
        fb->saved_rows_sao[comp] = calloc(margin * fb->saved_rows_stride[comp], sizeof(OVSample));
        fb->saved_rows_alf[comp] = calloc(margin * fb->saved_rows_stride[comp], sizeof(OVSample));
    }
}

static OVFrame *
harness_frame(int w, int h)
{
    OVPicture *p = ref_new_picture(w, h, 0);
    fill_plane(p->frame->data[0], w, h, w);
    fill_plane(p->frame->data[1], w / 2, h / 2, w / 2);
    fill_plane(p->frame->data[2], w / 2, h / 2, w / 2);
    return p->frame;
}

/* the pictures of sao*.ovg / alf*.ovg per CTU size: at 128 the three of the first fixtures; at 64 and 32 (reference mode only) three
 * full CTU rows and a truncated one with a ragged width, a second ragged picture, a single truncated CTU row and a single row of
 * exactly one CTU (the single-row quirk of rcn_sao_first_pix_rows).  No width is a multiple of the CTU or of a device tile. */
enum { FLT_NPIC_MAX = 4 };
struct flt_pics { int n; int w[FLT_NPIC_MAX], h[FLT_NPIC_MAX]; const char *name; };

static const struct flt_pics *
flt_pics_for(int alf, int log2_ctu)
{
    static const struct flt_pics sao[3] = {
        { 4, { 152, 104, 72, 72 },  { 104, 64, 24, 32 },  "sao_ctu32.ovg" },
        { 4, { 304, 200, 136, 136 }, { 200, 136, 56, 64 }, "sao_ctu64.ovg" },
        { 3, { 304, 264, 136 },      { 200, 264, 72 },     "sao.ovg" } };
    static const struct flt_pics al[3] = {
        { 4, { 152, 104, 72, 72 },  { 104, 64, 24, 32 },  "alf_ctu32.ovg" },
        { 4, { 304, 200, 136, 136 }, { 200, 128, 56, 64 }, "alf_ctu64.ovg" },
        { 3, { 304, 264, 136 },      { 200, 256, 72 },     "alf.ovg" } };
    if (log2_ctu < 5 || log2_ctu > 7 || (g_shim && log2_ctu != 7)) { fprintf(stderr, "sao / alf: CTU size 2^%d is not generated%s\n", log2_ctu, g_shim ? " in shim mode" : ""); exit(1); }
    return alf ? &al[log2_ctu - 5] : &sao[log2_ctu - 5];
}

/* SAO of a whole picture (one rect entry): call order of decode_ctu_line / decode_ctu_last_line (slicedec.c:934-956, :1058-1073) */
static void
sao_filter_picture(OVCTUDec *c, struct RectEntryInfo *einfo, int ny)
{
    for (int cy = 0; cy < ny; ++cy) {
        c->ctb_y = cy;
        if (cy == 0) {
            TIMED(TS_SAO, c->rcn_funcs.sao.rcn_sao_first_pix_rows(c, einfo, 0));
            if (ny == 1) TIMED(TS_SAO, c->rcn_funcs.sao.rcn_sao_filter_line(c, einfo, 0));
        } else if (cy == ny - 1) {
            TIMED(TS_SAO, c->rcn_funcs.sao.rcn_sao_filter_line(c, einfo, cy - 1));
            TIMED(TS_SAO, c->rcn_funcs.sao.rcn_sao_filter_line(c, einfo, cy));
        } else {
            TIMED(TS_SAO, c->rcn_funcs.sao.rcn_sao_filter_line(c, einfo, cy - 1));
        }
    }
}

static void
gen_sao(const char *dir, int log2_ctu)
{
    const struct flt_pics *P = flt_pics_for(0, log2_ctu);
    const int NPIC = P->n, *PW = P->w, *PH = P->h, ctu = 1 << log2_ctu;
    gfile g = gfile_open(dir, g_shim ? "shim_sao.ovg" : P->name);
    g_seed = 0x266 + 3;
    g_part.log2_ctu_s = log2_ctu;
    for (int pi = 0; pi < NPIC; ++pi) {
        const int W = PW[pi], H = PH[pi], nx = (W + ctu - 1) / ctu, ny = (H + ctu - 1) / ctu;
        OVFrame *f = harness_frame(W, H);
        /* sprinkle extremes so clipping and every band are hit */
        uint16_t *py = f->data[0];
        for (int i = 0; i < W * H; i += 11) py[i] = (uint16_t)rnd_range(0, 1023);
        char nm[32];
        uint32_t d2[2] = { H, W };
        if (!g_shim) {
        snprintf(nm, 32, "p%d_in_y", pi); gfile_array(&g, nm, T_U16, f->data[0], 2, d2);
        d2[0] = H / 2; d2[1] = W / 2;
        snprintf(nm, 32, "p%d_in_cb", pi); gfile_array(&g, nm, T_U16, f->data[1], 2, d2);
        snprintf(nm, 32, "p%d_in_cr", pi); gfile_array(&g, nm, T_U16, f->data[2], 2, d2);
        }

        OVCTUDec *c = ref_new_ctudec(0, 0);
        if (g_shim) shim_bind(c, W, H, 0, 0);
        c->pic_w = W; c->pic_h = H;
        c->rcn_ctx.frame_start = f;
        harness_alloc_filter_buffers(&c->rcn_ctx, nx, 3, log2_ctu);
        c->sao_info.sao_luma_flag = 1; c->sao_info.sao_chroma_flag = 1; c->sao_info.chroma_format_idc = 1;
        SAOParamsCtu *prm = calloc(nx * ny, sizeof(*prm));
        ovhip_sao_ctu *mine = calloc(nx * ny, sizeof(*mine));
        c->sao_info.sao_params = prm;
        for (int i = 0; i < nx * ny; ++i) {
            for (int comp = 0; comp < 3; ++comp) {
                int t = rnd_range(0, 3); if (t == 3) t = 2;
                prm[i].type_idx[comp] = t;
                prm[i].band_position[comp] = rnd_range(0, 31);
                prm[i].eo_class[comp] = rnd_range(0, 3);
                for (int k = 0; k < 5; ++k) prm[i].offset_val[comp][k] = (int16_t)rnd_range(-31, 31);
                if (t == 2) { prm[i].offset_val[comp][2] = 0; }
                mine[i].type[comp] = t; mine[i].band_position[comp] = prm[i].band_position[comp];
                mine[i].eo_class[comp] = prm[i].eo_class[comp];
                memcpy(mine[i].offset_val[comp], prm[i].offset_val[comp], 10);
            }
        }
        struct RectEntryInfo einfo;
        memset(&einfo, 0, sizeof(einfo));
        einfo.nb_ctu_w = nx; einfo.nb_ctu_h = ny;
        sao_filter_picture(c, &einfo, ny);
        if (g_shim) {
            size_t nc = 0;
            const ovhip_sao_ctu *sp = ovhip_shim_sao_params(c, &nc);
            if (!sp || nc != (size_t)(nx * ny) || ovhip_shim_last_error(c)) { fprintf(stderr, "shim: sao picture %d: no parameters captured\n", pi); exit(1); }
            d2[0] = nx * ny; d2[1] = sizeof(ovhip_sao_ctu);
            snprintf(nm, 32, "p%d_params", pi); gfile_array(&g, nm, T_U8, sp, 2, d2);
            continue;
        }
        d2[0] = H; d2[1] = W;
        snprintf(nm, 32, "p%d_exp_y", pi); gfile_array(&g, nm, T_U16, f->data[0], 2, d2);
        d2[0] = H / 2; d2[1] = W / 2;
        snprintf(nm, 32, "p%d_exp_cb", pi); gfile_array(&g, nm, T_U16, f->data[1], 2, d2);
        snprintf(nm, 32, "p%d_exp_cr", pi); gfile_array(&g, nm, T_U16, f->data[2], 2, d2);
        d2[0] = nx * ny; d2[1] = sizeof(ovhip_sao_ctu);
        snprintf(nm, 32, "p%d_params", pi); gfile_array(&g, nm, T_U8, mine, 2, d2);
        fprintf(stderr, "%s: picture %d %dx%d (%d CTUs of %d)\n", P->name, pi, W, H, nx * ny, ctu);
    }
    g_part.log2_ctu_s = 7;
    if (g_shim) {
        /* a picture cut into TWO rect entries (tile columns) with each entry on its OWN OVCTUDec (entry threads: ovthreads.c:112-114),
         * record-only: the shim keeps one recorder per OVCTUDec.  The entry that starts the picture is taken; the one whose
         * OVCTUDec never saw the picture's first entry has nobody to record into and must latch OVHIP_EUNSUP at its attach (the
         * entries of a picture in turn on ONE OVCTUDec are the supported form: gen_pipe's tiles streams). */
        const int W = 384, H = 136, nx = 3, ny = 2;
        int32_t codes[2];
        for (int en = 0; en < 2; ++en) {
            OVFrame *f = harness_frame(W, H);
            OVCTUDec *c = ref_new_ctudec(0, 0);
            shim_bind(c, W, H, 0, 0);
            c->pic_w = W; c->pic_h = H;
            c->rcn_ctx.frame_start = f;
            harness_alloc_filter_buffers(&c->rcn_ctx, nx, 3, 7);
            c->sao_info.sao_luma_flag = 1; c->sao_info.chroma_format_idc = 1;
            c->sao_info.sao_params = calloc(nx * ny, sizeof(SAOParamsCtu));
            struct RectEntryInfo einfo;
            memset(&einfo, 0, sizeof(einfo));
            einfo.ctb_x = en ? 2 : 0; einfo.nb_ctu_w = en ? 1 : 2; einfo.nb_ctu_h = ny;
            c->ctb_y = 0;
            c->rcn_funcs.rcn_attach_frame_buff(&c->rcn_ctx, f, &einfo, 7);
            c->rcn_funcs.sao.rcn_sao_first_pix_rows(c, &einfo, 0);
            codes[en] = ovhip_shim_last_error(c);
            if (codes[en] != (en ? OVHIP_EUNSUP : 0)) { fprintf(stderr, "shim: entry %d of a two-OVCTUDec picture: code %d\n", en, codes[en]); exit(1); }
        }
        uint32_t d1 = 2;
        gfile_array(&g, "two_entries_latched", T_I32, codes, 1, &d1);
        fprintf(stderr, "shim_sao.ovg: two rect entries on two OVCTUDecs: first taken, second refused (%d, %d)\n", codes[0], codes[1]);
    }
    gfile_close(&g);
}


/* ====================================================================================== ALF */
static void
rand_alf_aps(OVALFData *a)
{
    memset(a, 0, sizeof(*a));
    int nf = rnd_range(1, 25);
    a->alf_luma_num_filters_signalled_minus1 = nf - 1;
    a->alf_luma_clip_flag = rnd_range(0, 1);
    for (int c = 0; c < 25; ++c) a->alf_luma_coeff_delta_idx[c] = rnd_range(0, nf - 1);
    for (int f = 0; f < 25; ++f) for (int k = 0; k < 12; ++k) {
        a->alf_luma_coeff[f][k] = (int16_t)(rnd_range(0, 7) == 0 ? rnd_range(-127, 127) : rnd_range(-24, 24));
        a->alf_luma_clip_idx[f][k] = rnd_range(0, 3);
    }
    a->alf_chroma_clip_flag = rnd_range(0, 1);
    a->alf_chroma_num_alt_filters_minus1 = rnd_range(0, 7);
    for (int f = 0; f < 8; ++f) for (int k = 0; k < 6; ++k) {
        a->alf_chroma_coeff[f][k] = (int16_t)(rnd_range(0, 7) == 0 ? rnd_range(-127, 127) : rnd_range(-24, 24));
        a->alf_chroma_clip_idx[f][k] = rnd_range(0, 3);
    }
    a->alf_cc_cb_filters_signalled_minus1 = 3; a->alf_cc_cr_filters_signalled_minus1 = 3;
    for (int c = 0; c < 2; ++c) for (int f = 0; f < 4; ++f) for (int k = 0; k < 7; ++k) {
        int m = rnd_range(0, 7);
        int v = m == 0 ? 0 : 1 << (m - 1);
        a->alf_cc_mapped_coeff[c][f][k] = (int16_t)(rnd_range(0, 1) ? -v : v);
    }
}

static void
gen_alf(const char *dir, int log2_ctu)
{
    const struct flt_pics *P = flt_pics_for(1, log2_ctu);
    const int NPIC = P->n, *PW = P->w, *PH = P->h, ctu = 1 << log2_ctu;
    gfile g = gfile_open(dir, g_shim ? "shim_alf.ovg" : P->name);
    g_seed = 0x266 + 4;
    g_part.log2_ctu_s = log2_ctu;
    for (int pi = 0; pi < NPIC; ++pi) {
        const int W = PW[pi], H = PH[pi], nx = (W + ctu - 1) / ctu, ny = (H + ctu - 1) / ctu;
        OVFrame *f = harness_frame(W, H);
        uint16_t *py = f->data[0];
        for (int i = 0; i < W * H; i += 13) py[i] = (uint16_t)rnd_range(0, 1023);
        char nm[32];
        uint32_t d2[2] = { H, W };
        if (!g_shim) {
        snprintf(nm, 32, "p%d_in_y", pi); gfile_array(&g, nm, T_U16, f->data[0], 2, d2);
        d2[0] = H / 2; d2[1] = W / 2;
        snprintf(nm, 32, "p%d_in_cb", pi); gfile_array(&g, nm, T_U16, f->data[1], 2, d2);
        snprintf(nm, 32, "p%d_in_cr", pi); gfile_array(&g, nm, T_U16, f->data[2], 2, d2);
        }

        OVCTUDec *c = ref_new_ctudec(0, 0);
        if (g_shim) shim_bind(c, W, H, 0, 0);
        c->pic_w = W; c->pic_h = H;
        c->rcn_ctx.frame_start = f;
        harness_alloc_filter_buffers(&c->rcn_ctx, nx, 3, log2_ctu);
        struct ALFInfo *ai = &c->alf_info;
        static OVALFData aps[5];
        /* the first fixture draws five APSs per picture; the smaller-CTU ones draw them once and store the tables once (p0_*): the
         * two luma tables are 125 KB a picture, and a committed file stays below 1 MiB */
        const int own_aps = log2_ctu == 7 || pi == 0;
        if (own_aps) for (int i = 0; i < 5; ++i) rand_alf_aps(&aps[i]);
        /* one draw has to cover what three cover in the first fixture: a luma APS with and one without non-linear clipping, clipped chroma */
        if (log2_ctu != 7) { aps[0].alf_luma_clip_flag = 1; aps[1].alf_luma_clip_flag = 0; aps[2].alf_chroma_clip_flag = 1; }
        ai->alf_luma_enabled_flag = ai->alf_cb_enabled_flag = ai->alf_cr_enabled_flag = 1;
        ai->cc_alf_cb_enabled_flag = ai->cc_alf_cr_enabled_flag = 1;
        ai->num_alf_aps_ids_luma = 2;
        ai->aps_alf_data[0] = &aps[0]; ai->aps_alf_data[1] = &aps[1];
        ai->aps_alf_data_c = &aps[2]; ai->aps_cc_alf_data_cb = &aps[3]; ai->aps_cc_alf_data_cr = &aps[4];
        ai->ctb_alf_params = calloc(nx * ny, sizeof(ALFParamsCtu));
        ai->ctb_cc_alf_filter_idx[0] = calloc(nx * ny, 1); ai->ctb_cc_alf_filter_idx[1] = calloc(nx * ny, 1);
        c->rcn_funcs.alf.rcn_alf_reconstruct_coeff_APS(&ai->rcn_alf, c, 1, 1);
        ovhip_alf_ctu *mine = calloc(nx * ny, sizeof(*mine));
        for (int i = 0; i < nx * ny; ++i) {
            ALFParamsCtu *p = &ai->ctb_alf_params[i];
            p->ctb_alf_flag = rnd_range(0, 9) < 8 ? (rnd_range(0, 7) | (rnd_range(0, 2) ? 4 : 0)) : 0;
            p->ctb_alf_idx = rnd_range(0, 17);
            if (log2_ctu != 7 && i % 3 == 0) p->ctb_alf_idx = 16 + ((i / 3) & 1);      /* every third CTU filters with an APS set, not a fixed one */
            p->cb_alternative = rnd_range(0, aps[2].alf_chroma_num_alt_filters_minus1);
            p->cr_alternative = rnd_range(0, aps[2].alf_chroma_num_alt_filters_minus1);
            ai->ctb_cc_alf_filter_idx[0][i] = rnd_range(0, 4);
            ai->ctb_cc_alf_filter_idx[1][i] = rnd_range(0, 4);
            mine[i].flags = p->ctb_alf_flag; mine[i].luma_set = p->ctb_alf_idx;
            mine[i].cb_alt = p->cb_alternative; mine[i].cr_alt = p->cr_alternative;
            mine[i].cc_cb_idx = ai->ctb_cc_alf_filter_idx[0][i]; mine[i].cc_cr_idx = ai->ctb_cc_alf_filter_idx[1][i];
        }
        struct RectEntryInfo einfo;
        memset(&einfo, 0, sizeof(einfo));
        einfo.nb_ctu_w = nx; einfo.nb_ctu_h = ny;
        for (int cy = 0; cy < ny; ++cy) { c->ctb_y = cy; TIMED(TS_ALF, c->rcn_funcs.alf.rcn_alf_filter_line(c, &einfo, cy)); }

        if (g_shim) {
            size_t nc = 0, nt = 0;
            const ovhip_alf_ctu *ap = ovhip_shim_alf_params(c, &nc);
            if (!ap || nc != (size_t)(nx * ny) || ovhip_shim_last_error(c)) { fprintf(stderr, "shim: alf picture %d: no parameters captured\n", pi); exit(1); }
            d2[0] = nx * ny; d2[1] = sizeof(ovhip_alf_ctu);
            snprintf(nm, 32, "p%d_ctus", pi); gfile_array(&g, nm, T_U8, ap, 2, d2);
            static const char *tn[5] = { "luma_coeff", "luma_clip", "chroma_coeff", "chroma_clip", "cc_coeff" };
            for (int t = 0; t < 5; ++t) {
                const int16_t *tp = ovhip_shim_alf_table(c, t, &nt);
                uint32_t dt = (uint32_t)nt;
                snprintf(nm, 32, "p%d_%s", pi, tn[t]); gfile_array(&g, nm, T_I16, tp, 1, &dt);
            }
            continue;
        }
        d2[0] = H; d2[1] = W;
        snprintf(nm, 32, "p%d_exp_y", pi); gfile_array(&g, nm, T_U16, f->data[0], 2, d2);
        d2[0] = H / 2; d2[1] = W / 2;
        snprintf(nm, 32, "p%d_exp_cb", pi); gfile_array(&g, nm, T_U16, f->data[1], 2, d2);
        snprintf(nm, 32, "p%d_exp_cr", pi); gfile_array(&g, nm, T_U16, f->data[2], 2, d2);
        d2[0] = nx * ny; d2[1] = sizeof(ovhip_alf_ctu);
        snprintf(nm, 32, "p%d_ctus", pi); gfile_array(&g, nm, T_U8, mine, 2, d2);
        if (own_aps) {
        d2[0] = 24; d2[1] = OVHIP_ALF_LUMA_SET_SIZE;
        snprintf(nm, 32, "p%d_luma_coeff", pi); gfile_array(&g, nm, T_I16, ai->rcn_alf.filter_coeff_dec, 2, d2);
        snprintf(nm, 32, "p%d_luma_clip", pi); gfile_array(&g, nm, T_I16, ai->rcn_alf.filter_clip_dec, 2, d2);
        d2[0] = 8; d2[1] = 7;
        snprintf(nm, 32, "p%d_chroma_coeff", pi); gfile_array(&g, nm, T_I16, ai->rcn_alf.chroma_coeff_final, 2, d2);
        snprintf(nm, 32, "p%d_chroma_clip", pi); gfile_array(&g, nm, T_I16, ai->rcn_alf.chroma_clip_final, 2, d2);
        int16_t cc[2][4][8];
        memcpy(cc[0], aps[3].alf_cc_mapped_coeff[0], sizeof(cc[0]));
        memcpy(cc[1], aps[4].alf_cc_mapped_coeff[1], sizeof(cc[1]));
        uint32_t d3[3] = { 2, 4, 8 };
        snprintf(nm, 32, "p%d_cc_coeff", pi); gfile_array(&g, nm, T_I16, cc, 3, d3);
        }
        fprintf(stderr, "%s: picture %d %dx%d (%d CTUs of %d)\n", P->name, pi, W, H, nx * ny, ctu);
    }
    g_part.log2_ctu_s = 7;
    gfile_close(&g);
}

/* ====================================================================================== SAO and ALF: enumerated cells
 * sao_cells_<family>_NN.ovg / alf_cells_<family>_NN.ovg: one picture a file, in the layout of sao.ovg / alf.ovg (p0_*) plus
 * "log2_ctu"; the expected planes are the reference's, through the slots and the call order of gen_sao / gen_alf.  What the
 * families have to reach is asserted from tests/filter_census.py (tests/test_oracle_golden.py); the generator only draws content
 * and parameters so that they do.
 *   sao    equal runs, plateaus, two-level steps and both ends of the sample range beside noise; distinct offsets up to +-31;
 *          every band position; pictures with a ragged last group of 8 in luma and chroma, a truncated last CTU row, one of a
 *          single CTU row; CTU 128, 64 and 32
 *   class  16x16 patches of curved surfaces, drawn, classified (the generator's own fc_block_sums / fc_class) and kept while a
 *          (class, transpose) pair still lacks blocks -- on a fixed filter set and on an APS set apart, and among the blocks at a
 *          virtual boundary every activity class, direction class and transpose; every luma_set value
 *   edge   patches moved sample by sample (a local search from such a surface) until the 4x4 block at their centre has a given
 *          act, a sum_h + sum_v on either side of an activity threshold, or one of the five ties of alf_derive_filter_idx -- on
 *          plain blocks and on blocks at a virtual boundary; the all-zero block; the largest sums (0 / 1023 checkerboard, stripes)
 *   taps   APS sets built for the purpose (see alf_cells_taps) on the content of the sao family */
static void
fcell_put_planes(gfile *g, const char *what, const OVFrame *f, int W, int H)
{
    char nm[32];
    uint32_t d2[2] = { H, W };
    snprintf(nm, 32, "p0_%s_y", what); gfile_array(g, nm, T_U16, f->data[0], 2, d2);
    d2[0] = H / 2; d2[1] = W / 2;
    snprintf(nm, 32, "p0_%s_cb", what); gfile_array(g, nm, T_U16, f->data[1], 2, d2);
    snprintf(nm, 32, "p0_%s_cr", what); gfile_array(g, nm, T_U16, f->data[2], 2, d2);
}

/* cells of cs x cs samples, each of one kind of content */
static void
fcell_fill_plane(uint16_t *p, int w, int h, int cs)
{
    for (int cy = 0; cy < h; cy += cs)
        for (int cx = 0; cx < w; cx += cs) {
            const int mode = rnd_range(0, 7), base = rnd_range(3, 1019), step = rnd_range(1, 3);
            for (int y = cy; y < cy + cs && y < h; ++y)
                for (int x = cx; x < cx + cs && x < w; ++x) {
                    int v;
                    switch (mode) {
                    case 2: v = base + rnd_range(0, 1); break;                                          /* two levels */
                    case 3: v = ((x | y) & 1) ? p[(y & ~1) * w + (x & ~1)] : rnd_range(0, 1023); break; /* 2x2 plateaus */
                    case 4: v = (x & 3) ? p[y * w + x - 1] : rnd_range(0, 1023); break;                 /* runs of four */
                    case 5: v = rnd_range(0, 24); break;                                                /* the ends of the range */
                    case 6: v = 1023 - rnd_range(0, 24); break;
                    case 7: v = base + rnd_range(-step, step); break;
                    default: v = rnd_range(0, 1023); break;
                    }
                    p[y * w + x] = (uint16_t)v;
                }
        }
}

static OVFrame *
fcell_frame(int w, int h)
{
    OVFrame *f = ref_new_picture(w, h, 0)->frame;
    fcell_fill_plane((uint16_t *)f->data[0], w, h, 8);
    fcell_fill_plane((uint16_t *)f->data[1], w / 2, h / 2, 4);
    fcell_fill_plane((uint16_t *)f->data[2], w / 2, h / 2, 4);
    return f;
}

/* a picture cut into rect entries (tiles): the CTU columns col[k] .. col[k + 1] and rows row[k] .. row[k + 1]; NULL: one entry.  The
 * reference's line drivers run once per entry with that entry's RectEntryInfo and entry-local parameter arrays, one entry after
 * the other on one OVCTUDec, as the slice decoder calls them (slicedec.c:636-657); is_border comes from the entry-local CTU index. */
struct fcell_cut { int nc, nr, col[4], row[4]; };
static int
fcell_border(const struct fcell_cut *cut, int cx, int cy)
{
    int b = 0;
    if (!cut) return 0;
    for (int k = 0; k < cut->nc; ++k) { if (cx == cut->col[k]) b |= OVHIP_BORDER_LEFT; if (cx == cut->col[k + 1] - 1) b |= OVHIP_BORDER_RIGHT; }
    for (int k = 0; k < cut->nr; ++k) {
        if (cy == cut->row[k]) b |= OVHIP_BORDER_UPPER;
        if (cy == cut->row[k + 1] - 1) b |= OVHIP_BORDER_BOTTOM;
        if (cy == cut->row[k] && cut->row[k + 1] - cut->row[k] == 1) b |= OVHIP_BORDER_ONE_ROW;
    }
    return b;
}

static void
sao_cells_picture(const char *dir, const char *name, int W, int H, int log2_ctu, const struct fcell_cut *cut)
{
    const int ctu = 1 << log2_ctu, nx = (W + ctu - 1) / ctu, ny = (H + ctu - 1) / ctu, n = nx * ny;
    gfile g = gfile_open(dir, name);
    g_part.log2_ctu_s = log2_ctu;
    OVFrame *f = fcell_frame(W, H);
    OVCTUDec *c = ref_new_ctudec(0, 0);
    c->pic_w = W; c->pic_h = H;
    c->rcn_ctx.frame_start = f;
    harness_alloc_filter_buffers(&c->rcn_ctx, nx, 3, log2_ctu);
    c->sao_info.sao_luma_flag = 1; c->sao_info.sao_chroma_flag = 1; c->sao_info.chroma_format_idc = 1;
    SAOParamsCtu *prm = calloc(n, sizeof(*prm));
    ovhip_sao_ctu *mine = calloc(n, sizeof(*mine));
    c->sao_info.sao_params = prm;
    /* few CTUs: every second one edge, one off, the rest band; many: every third one edge.  The edge classes and the band positions
     * run on from CTU to CTU, shifted per plane; the offsets are all different, with +-31 at the ends, in both sign patterns */
    int n_band[3] = { 0, 0, 0 }, n_edge[3] = { 0, 0, 0 };
    for (int i = 0; i < n; ++i)
        for (int comp = 0; comp < 3; ++comp) {
            const int t = n < 12 ? (i % 2 == 0 ? 2 : i == 3 ? 0 : 1) : (i % 3 == 0 ? 2 : 1), s = ((i + comp) & 1) ? 1 : -1;
            static const int16_t band[4] = { 31, -31, 17, -9 }, edge[5] = { 31, -23, 0, 13, -31 };
            prm[i].type_idx[comp] = t;
            prm[i].band_position[comp] = (29 + 11 * comp + n_band[comp]) & 31;
            prm[i].eo_class[comp] = (n_edge[comp] + comp + (ny == 1)) & 3;          /* (a single CTU row: luma not horizontal, for the 6-row quirk) */
            n_band[comp] += t == 1; n_edge[comp] += t == 2;
            for (int k = 0; k < 5; ++k) prm[i].offset_val[comp][k] = (int16_t)(s * (t == 2 ? edge[k] : k < 4 ? band[k] : 0));
            mine[i].type[comp] = t; mine[i].band_position[comp] = prm[i].band_position[comp];
            mine[i].eo_class[comp] = prm[i].eo_class[comp];
            memcpy(mine[i].offset_val[comp], prm[i].offset_val[comp], 10);
            if (t == 1) {
                /* a band CTU holds a sample of each of its four bands, wherever else its content lies */
                const int sh = comp ? 1 : 0, cs = ctu >> sh, pw = W >> sh, ph = H >> sh, x0 = (i % nx) * cs, y0 = (i / nx) * cs;
                for (int k = 0; k < 4; ++k) {
                    const int x = x0 + rnd_range(0, (x0 + cs < pw ? cs : pw - x0) - 1), y = y0 + rnd_range(0, (y0 + cs < ph ? cs : ph - y0) - 1);
                    ((uint16_t *)f->data[comp])[y * pw + x] = (uint16_t)((((prm[i].band_position[comp] + k) & 31) << 5) + rnd_range(0, 31));
                }
            }
        }
    fcell_put_planes(&g, "in", f, W, H);
    struct RectEntryInfo einfo;
    memset(&einfo, 0, sizeof(einfo));
    einfo.nb_ctu_w = nx; einfo.nb_ctu_h = ny;
    if (!cut) sao_filter_picture(c, &einfo, ny);
    else
        for (int er = 0; er < cut->nr; ++er)
            for (int ec = 0; ec < cut->nc; ++ec) {
                einfo.ctb_x = cut->col[ec]; einfo.ctb_y = cut->row[er];
                einfo.nb_ctu_w = cut->col[ec + 1] - cut->col[ec]; einfo.nb_ctu_h = cut->row[er + 1] - cut->row[er];
                SAOParamsCtu *loc = calloc(einfo.nb_ctu_w * einfo.nb_ctu_h, sizeof(*loc));
                for (int y = 0; y < einfo.nb_ctu_h; ++y)
                    for (int x = 0; x < einfo.nb_ctu_w; ++x) {
                        loc[y * einfo.nb_ctu_w + x] = prm[(einfo.ctb_y + y) * nx + einfo.ctb_x + x];
                        mine[(einfo.ctb_y + y) * nx + einfo.ctb_x + x].border = fcell_border(cut, einfo.ctb_x + x, einfo.ctb_y + y);
                    }
                c->sao_info.sao_params = loc;
                sao_filter_picture(c, &einfo, einfo.nb_ctu_h);
            }
    fcell_put_planes(&g, "exp", f, W, H);
    uint32_t d2[2] = { n, sizeof(ovhip_sao_ctu) }, d1 = 1;
    int32_t l2 = log2_ctu;
    gfile_array(&g, "p0_params", T_U8, mine, 2, d2);
    gfile_array(&g, "log2_ctu", T_I32, &l2, 1, &d1);
    fprintf(stderr, "%s: %dx%d (%d CTUs of %d)\n", name, W, H, n, ctu);
    g_part.log2_ctu_s = 7;
    gfile_close(&g);
}

static void
gen_sao_cells(const char *dir)
{
    g_seed = 0x266 + 13;
    sao_cells_picture(dir, "sao_cells_sao_00.ovg", 300, 264, 7, NULL);       /* 3 x 3 CTUs, the last row 8 rows high; 300 and 150: ragged groups */
    sao_cells_picture(dir, "sao_cells_sao_01.ovg", 140, 72, 7, NULL);        /* a single CTU row (the 6-row quirk) */
    sao_cells_picture(dir, "sao_cells_sao64_00.ovg", 300, 200, 6, NULL);
    sao_cells_picture(dir, "sao_cells_sao32_00.ovg", 252, 172, 5, NULL);     /* 8 x 6 CTUs: 32 band CTUs a plane, one per band position */
    /* 2 x 2 rect entries: 5 x 4 CTUs of 64 cut into columns of 3 and 2 and rows of 1 (an entry a single CTU row high) and 3 */
    static const struct fcell_cut cut = { 2, 2, { 0, 3, 5 }, { 0, 1, 4 } };
    sao_cells_picture(dir, "sao_cells_entry64_00.ovg", 300, 200, 6, &cut);
}

/* ---- ALF: the generator's own classification, to choose content by (the expected planes come from the reference alone) */
/* Laplacian sums v, h, d, b of the 4x4 block at (bx, by); vb: picture row of the virtual boundary of the block's CTU */
static int
fc_block_sums(const uint16_t *p, int stride, int bx, int by, int vb, uint32_t s[4])
{
    int first = 0, last = 3, is_vb = 0;
    if (by == vb - 4) { last = 2; is_vb = 1; }
    if (by == vb)     { first = 1; is_vb = 1; }
    s[0] = s[1] = s[2] = s[3] = 0;
#define FP(x, y) ((int)p[(y) * stride + (x)])
    for (int k = first; k <= last; ++k) {
        const int r = by - 2 + 2 * k;
        const int above = r == vb ? r : r - 1, below = r + 2 == vb ? r + 1 : r + 2;
        for (int q = 0; q < 4; ++q) {
            const int c0 = bx - 2 + 2 * q, c1 = c0 + 1, y1 = FP(c0, r) << 1, y2 = FP(c1, r + 1) << 1;
            s[0] += abs(y1 - FP(c0, above) - FP(c0, r + 1)) + abs(y2 - FP(c1, r) - FP(c1, below));
            s[1] += abs(y1 - FP(c0 + 1, r) - FP(c0 - 1, r)) + abs(y2 - FP(c1 + 1, r + 1) - FP(c1 - 1, r + 1));
            s[2] += abs(y1 - FP(c0 - 1, above) - FP(c0 + 1, r + 1)) + abs(y2 - FP(c1 - 1, r) - FP(c1 + 1, below));
            s[3] += abs(y1 - FP(c0 - 1, r + 1) - FP(c0 + 1, above)) + abs(y2 - FP(c1 - 1, below) - FP(c1 + 1, r));
        }
    }
#undef FP
    return is_vb;
}

struct fc_cls { int act, cls, tr; uint64_t max_dir, min_dir, cross_a, cross_b; };
static struct fc_cls
fc_class(const uint32_t s[4], int is_vb)
{
    static const int th[16] = { 0, 1, 2, 2, 2, 2, 2, 3, 3, 3, 3, 3, 3, 3, 3, 4 }, tr_lut[8] = { 0, 1, 0, 2, 2, 3, 1, 3 };
    const uint64_t sv = s[0], sh = s[1], sd = s[2], sb = s[3];
    struct fc_cls o;
    const uint64_t a = ((sh + sv) * (is_vb ? 96 : 64)) >> 14;
    o.act = a > 15 ? 15 : (int)a;
    const uint64_t max_hv = sv > sh ? sv : sh, min_hv = sv > sh ? sh : sv, max_db = sd > sb ? sd : sb, min_db = sd > sb ? sb : sd;
    const int dir_hv = sv > sh ? 1 : 3, dir_db = sd > sb ? 0 : 2;
    o.cross_a = max_db * min_hv; o.cross_b = max_hv * min_db;
    const int db = o.cross_a > o.cross_b, main_dir = db ? dir_db : dir_hv, sec_dir = db ? dir_hv : dir_db;
    o.max_dir = db ? max_db : max_hv; o.min_dir = db ? min_db : min_hv;
    o.cls = th[o.act];
    if (o.max_dir * 2 > 9 * o.min_dir) o.cls += (((main_dir & 1) << 1) + 2) * 5;
    else if (o.max_dir > 2 * o.min_dir) o.cls += (((main_dir & 1) << 1) + 1) * 5;
    o.tr = tr_lut[(main_dir << 1) + (sec_dir >> 1)];
    return o;
}

/* a 16x16 patch of base + (2 a x^2 + 2 b y^2 + c (x + y)^2 + e (x - y)^2) / 64 + noise (+ a wave), x and y from the patch's centre */
static void
fc_surface(uint16_t *p, int stride, int amp, int noise)
{
    int k[4];
    for (int i = 0; i < 4; ++i) k[i] = rnd_range(0, 1) ? rnd_range(-amp, amp) : 0;
    const int base = rnd_range(300, 700);
    /* every other patch: one or two triangle waves of period 4 across one of the four directions on top (high activity that keeps a direction) */
    static const int tri[4] = { 0, 1, 2, 1 }, dirs[4][2] = { { 1, 0 }, { 0, 1 }, { 1, 1 }, { 1, 3 } };
    const int wmax = amp < 8 ? 8 : amp > 160 ? 160 : amp;
    const int wave = rnd_range(0, 1) ? rnd_range(1, wmax) : 0, wd = rnd_range(0, 3), wave2 = wave && rnd_range(0, 1) ? rnd_range(1, wmax) : 0, wd2 = rnd_range(0, 3);
    for (int y = 0; y < 16; ++y)
        for (int x = 0; x < 16; ++x) {
            const int X = x - 8, Y = y - 8;
            int v = base + (2 * k[0] * X * X + 2 * k[1] * Y * Y + k[2] * (X + Y) * (X + Y) + k[3] * (X - Y) * (X - Y)) / 64 + rnd_range(-noise, noise)
                    + wave * tri[(dirs[wd][0] * x + dirs[wd][1] * y) & 3] + wave2 * tri[(dirs[wd2][0] * x + dirs[wd2][1] * y + 1) & 3];
            p[y * stride + x] = (uint16_t)(v < 0 ? 0 : v > 1023 ? 1023 : v);
        }
}
static void
fc_draw_surface(uint16_t *p, int stride)
{
    static const int amps[10] = { 1, 2, 4, 8, 16, 32, 64, 128, 256, 512 }, noises[12] = { 0, 0, 0, 1, 1, 2, 3, 5, 8, 13, 21, 34 };
    fc_surface(p, stride, amps[rnd_range(0, 9)], noises[rnd_range(0, 11)]);
}

/* the slots of the 16x16 patches: columns 4 + 16 i; in every CTU row of full height rows 4 + 16 k up to the one that ends at ctu - 12,
 * then one at ctu - 12 whose inner blocks are the two at the virtual boundary (rows ctu - 8 and ctu - 4) */
struct fc_slot { int x, y, vb; };                    /* vb: the slot at a virtual boundary */
static int
fc_slots(struct fc_slot *out, int W, int H, int ctu)
{
    int n = 0;
    for (int b = 0; b + ctu <= H; b += ctu)
        for (int k = 0; k <= (ctu - 16) / 16; ++k) {
            const int y = b + (k < (ctu - 16) / 16 ? 4 + 16 * k : ctu - 12), vb = k == (ctu - 16) / 16;
            if (y + 16 > H) continue;
            for (int x = 4; x + 16 <= W; x += 16) { out[n].x = x; out[n].y = y; out[n].vb = vb; ++n; }
        }
    return n;
}

/* ALF of a whole picture with the tables of aps[5] (two luma sets, chroma, CC Cb, CC Cr) and the CTU parameters of `mine`; writes the file */
static void
alf_cells_write(const char *dir, const char *name, OVFrame *f, int W, int H, int log2_ctu, OVALFData *aps, ovhip_alf_ctu *mine, const struct fcell_cut *cut)
{
    const int ctu = 1 << log2_ctu, nx = (W + ctu - 1) / ctu, ny = (H + ctu - 1) / ctu, n = nx * ny;
    gfile g = gfile_open(dir, name);
    g_part.log2_ctu_s = log2_ctu;
    fcell_put_planes(&g, "in", f, W, H);
    OVCTUDec *c = ref_new_ctudec(0, 0);
    c->pic_w = W; c->pic_h = H;
    c->rcn_ctx.frame_start = f;
    harness_alloc_filter_buffers(&c->rcn_ctx, nx, 3, log2_ctu);
    struct ALFInfo *ai = &c->alf_info;
    ai->alf_luma_enabled_flag = ai->alf_cb_enabled_flag = ai->alf_cr_enabled_flag = 1;
    ai->cc_alf_cb_enabled_flag = ai->cc_alf_cr_enabled_flag = 1;
    ai->num_alf_aps_ids_luma = 2;
    ai->aps_alf_data[0] = &aps[0]; ai->aps_alf_data[1] = &aps[1];
    ai->aps_alf_data_c = &aps[2]; ai->aps_cc_alf_data_cb = &aps[3]; ai->aps_cc_alf_data_cr = &aps[4];
    ai->ctb_alf_params = calloc(n, sizeof(ALFParamsCtu));
    ai->ctb_cc_alf_filter_idx[0] = calloc(n, 1); ai->ctb_cc_alf_filter_idx[1] = calloc(n, 1);
    c->rcn_funcs.alf.rcn_alf_reconstruct_coeff_APS(&ai->rcn_alf, c, 1, 1);
    static const struct fcell_cut whole = { 1, 1 };
    struct fcell_cut one = whole;
    one.col[1] = nx; one.row[1] = ny;
    const struct fcell_cut *ct = cut ? cut : &one;
    for (int er = 0; er < ct->nr; ++er)
        for (int ec = 0; ec < ct->nc; ++ec) {
            struct RectEntryInfo einfo;
            memset(&einfo, 0, sizeof(einfo));
            einfo.ctb_x = ct->col[ec]; einfo.ctb_y = ct->row[er];
            einfo.nb_ctu_w = ct->col[ec + 1] - ct->col[ec]; einfo.nb_ctu_h = ct->row[er + 1] - ct->row[er];
            /* the parameter arrays are entry-local */
            for (int y = 0; y < einfo.nb_ctu_h; ++y)
                for (int x = 0; x < einfo.nb_ctu_w; ++x) {
                    ovhip_alf_ctu *m = &mine[(einfo.ctb_y + y) * nx + einfo.ctb_x + x];
                    const int i = y * einfo.nb_ctu_w + x;
                    ALFParamsCtu *p = &ai->ctb_alf_params[i];
                    p->ctb_alf_flag = m->flags; p->ctb_alf_idx = m->luma_set;
                    p->cb_alternative = m->cb_alt; p->cr_alternative = m->cr_alt;
                    ai->ctb_cc_alf_filter_idx[0][i] = m->cc_cb_idx; ai->ctb_cc_alf_filter_idx[1][i] = m->cc_cr_idx;
                    m->border = fcell_border(cut, einfo.ctb_x + x, einfo.ctb_y + y);
                }
            for (int cy = 0; cy < einfo.nb_ctu_h; ++cy) { c->ctb_y = cy; c->rcn_funcs.alf.rcn_alf_filter_line(c, &einfo, cy); }
        }
    fcell_put_planes(&g, "exp", f, W, H);
    uint32_t d2[2] = { n, sizeof(ovhip_alf_ctu) }, d1 = 1;
    gfile_array(&g, "p0_ctus", T_U8, mine, 2, d2);
    d2[0] = 24; d2[1] = OVHIP_ALF_LUMA_SET_SIZE;
    gfile_array(&g, "p0_luma_coeff", T_I16, ai->rcn_alf.filter_coeff_dec, 2, d2);
    gfile_array(&g, "p0_luma_clip", T_I16, ai->rcn_alf.filter_clip_dec, 2, d2);
    d2[0] = 8; d2[1] = 7;
    gfile_array(&g, "p0_chroma_coeff", T_I16, ai->rcn_alf.chroma_coeff_final, 2, d2);
    gfile_array(&g, "p0_chroma_clip", T_I16, ai->rcn_alf.chroma_clip_final, 2, d2);
    int16_t cc[2][4][8];
    memcpy(cc[0], aps[3].alf_cc_mapped_coeff[0], sizeof(cc[0]));
    memcpy(cc[1], aps[4].alf_cc_mapped_coeff[1], sizeof(cc[1]));
    uint32_t d3[3] = { 2, 4, 8 };
    gfile_array(&g, "p0_cc_coeff", T_I16, cc, 3, d3);
    int32_t l2 = log2_ctu;
    gfile_array(&g, "log2_ctu", T_I32, &l2, 1, &d1);
    fprintf(stderr, "%s: %dx%d (%d CTUs of %d)\n", name, W, H, n, ctu);
    g_part.log2_ctu_s = 7;
    gfile_close(&g);
}

/* the tables rcn_alf_reconstruct_coeff_APS builds from aps[0..1], to compare coefficient rows with */
static const int16_t *
fc_luma_rows(OVALFData *aps)
{
    static OVCTUDec *c;
    if (!c) c = ref_new_ctudec(0, 0);
    struct ALFInfo *ai = &c->alf_info;
    ai->num_alf_aps_ids_luma = 2;
    ai->aps_alf_data[0] = &aps[0]; ai->aps_alf_data[1] = &aps[1]; ai->aps_alf_data_c = &aps[2];
    c->rcn_funcs.alf.rcn_alf_reconstruct_coeff_APS(&ai->rcn_alf, c, 1, 1);
    return (const int16_t *)ai->rcn_alf.filter_coeff_dec;
}
/* the row of (set, cls, tr) differs from the rows of the other transposes, of the classes cls +- 1 in its group of five and cls +- 5 */
static int
fc_row_stands_out(const int16_t *t, int set, int cls, int tr)
{
#define ROW(c_, t_) (t + set * OVHIP_ALF_LUMA_SET_SIZE + (t_) * 25 * 13 + (c_) * 13)
    const int16_t *own = ROW(cls, tr);
    for (int k = 1; k < 4; ++k) if (!memcmp(own, ROW(cls, (tr + k) & 3), 24)) return 0;
    if (cls % 5 > 0 && !memcmp(own, ROW(cls - 1, tr), 24)) return 0;
    if (cls % 5 < 4 && !memcmp(own, ROW(cls + 1, tr), 24)) return 0;
    if (cls >= 5 && !memcmp(own, ROW(cls - 5, tr), 24)) return 0;
    if (cls < 20 && !memcmp(own, ROW(cls + 5, tr), 24)) return 0;
#undef ROW
    return 1;
}

/* APS sets whose 25 classes all have a filter of their own, the first linear, the second with clipping */
static void
alf_cells_class_aps(OVALFData *aps)
{
    for (int i = 0; i < 5; ++i) rand_alf_aps(&aps[i]);
    for (int i = 0; i < 2; ++i) {
        aps[i].alf_luma_num_filters_signalled_minus1 = 24;
        aps[i].alf_luma_clip_flag = i;
        for (int cl = 0; cl < 25; ++cl) aps[i].alf_luma_coeff_delta_idx[cl] = cl;
    }
}

static void
alf_cells_random_ctus(ovhip_alf_ctu *mine, int n, const OVALFData *aps)
{
    for (int i = 0; i < n; ++i) {
        mine[i].flags = 4 | rnd_range(0, 3);
        mine[i].cb_alt = rnd_range(0, aps[2].alf_chroma_num_alt_filters_minus1);
        mine[i].cr_alt = rnd_range(0, aps[2].alf_chroma_num_alt_filters_minus1);
        mine[i].cc_cb_idx = rnd_range(0, 4); mine[i].cc_cr_idx = rnd_range(0, 4);
    }
}

enum { FC_MAX_SLOTS = 512 };
/* blocks wanted per (kind of set, class, transpose): more where the activity is low, since a nearly flat block often filters alike under
 * neighbouring classes and then does not count */
#define FC_TARGET(cls) ((cls) % 5 == 0 ? 20 : (cls) % 5 == 1 ? 10 : 6)
struct fc_need { int pair[2][25][4], vb_act[5], vb_dir[5], vb_tr[4]; };
static int
fc_need_open(const struct fc_need *nd)
{
    int open = 0;
    for (int k = 0; k < 2; ++k) for (int cl = 0; cl < 25; ++cl) for (int t = 0; t < 4; ++t) open += nd->pair[k][cl][t] < FC_TARGET(cl);
    for (int i = 0; i < 5; ++i) open += (nd->vb_act[i] < 2) + (nd->vb_dir[i] < 2);
    for (int i = 0; i < 4; ++i) open += nd->vb_tr[i] < 2;
    return open;
}

/* one picture of the class family: patches are drawn and kept while they add to what `nd` still lacks */
static void
alf_cells_class_picture(const char *dir, const char *name, int W, int H, int log2_ctu, int pic, struct fc_need *nd, int max_draws)
{
    const int ctu = 1 << log2_ctu, nx = (W + ctu - 1) / ctu, ny = (H + ctu - 1) / ctu, n = nx * ny;
    static OVALFData aps[5];
    alf_cells_class_aps(aps);
    const int16_t *rows = fc_luma_rows(aps);
    OVFrame *f = harness_frame(W, H);
    uint16_t *py = (uint16_t *)f->data[0];
    ovhip_alf_ctu *mine = calloc(n, sizeof(*mine));
    alf_cells_random_ctus(mine, n, aps);
    /* CTU 128: fixed and APS sets alternate, the fixed ones running on from picture to picture; CTU 64: every set in turn */
    for (int i = 0; i < n; ++i) mine[i].luma_set = log2_ctu == 7 ? ((i + pic) & 1 ? 16 + ((i >> 1) & 1) : (pic * 5 + (i >> 1)) & 15) : i % 18;
    static struct fc_slot slots[FC_MAX_SLOTS];
    const int ns = fc_slots(slots, W, H, ctu);
    if (ns > FC_MAX_SLOTS) { fprintf(stderr, "alf_cells: too many slots\n"); exit(1); }
    uint8_t *taken = calloc(ns, 1);
    int placed = 0;
    uint16_t patch[256];
    for (int draw = 0; draw < max_draws && placed < ns && fc_need_open(nd); ++draw) {
        fc_draw_surface(patch, 16);
        /* the four inner blocks' windows lie inside the patch: classified once as plain blocks, once as the blocks of a slot at a virtual
         * boundary (rows 4 and 8 of the patch are the rows vb - 4 and vb) */
        struct { int ok, cls, tr, is_vb; } blk[2][4];
        for (int v = 0; v < 2; ++v)
            for (int b = 0; b < 4; ++b) {
                uint32_t s[4];
                blk[v][b].is_vb = fc_block_sums(patch, 16, 4 + 4 * (b & 1), 4 + 4 * (b >> 1), v ? 8 : -1000, s);
                const struct fc_cls k = fc_class(s, blk[v][b].is_vb);
                /* a block whose diagonal sums (or the other two) are equal is mirror-symmetric as far as the classifier sees, and such
                 * content often filters alike under two transposes: it is not counted */
                blk[v][b].ok = s[0] != s[1] && s[2] != s[3]; blk[v][b].cls = k.cls; blk[v][b].tr = k.tr;
            }
        /* the first free slot that the patch adds something to; slots of one CTU and kind see it alike, so the first of each is asked */
        for (int si = 0; si < ns; ++si) {
            if (taken[si]) continue;
            const struct fc_slot *sl = &slots[si];
            int gain = 0, upd[4][4], nu = 0;
            for (int b = 0; b < 4; ++b) {
                const int bx = sl->x + 4 + 4 * (b & 1), by = sl->y + 4 + 4 * (b >> 1), set = mine[(by / ctu) * nx + bx / ctu].luma_set;
                const int cls = blk[sl->vb][b].cls, tr = blk[sl->vb][b].tr, is_vb = blk[sl->vb][b].is_vb, kind = set >= 16;
                if (!blk[sl->vb][b].ok || !fc_row_stands_out(rows, set, cls, tr)) continue;
                if (!sl->vb && nd->pair[kind][cls][tr] < FC_TARGET(cls)) ++gain;             /* (the slots at a boundary are kept for what only they can add) */
                if (is_vb && (nd->vb_act[cls % 5] < 2 || nd->vb_dir[cls / 5] < 2 || nd->vb_tr[tr] < 2)) ++gain;
                upd[nu][0] = kind; upd[nu][1] = cls; upd[nu][2] = tr; upd[nu][3] = is_vb; ++nu;
            }
            /* early draws have to add several blocks, so that the slots last for the rare pairs */
            if (gain >= (sl->vb ? 1 : draw < 30000 ? 3 : draw < 120000 ? 2 : 1)) {
                for (int u = 0; u < nu; ++u) {
                    ++nd->pair[upd[u][0]][upd[u][1]][upd[u][2]];
                    if (upd[u][3]) { ++nd->vb_act[upd[u][1] % 5]; ++nd->vb_dir[upd[u][1] / 5]; ++nd->vb_tr[upd[u][2]]; }
                }
                for (int y = 0; y < 16; ++y) memcpy(py + (sl->y + y) * W + sl->x, patch + 16 * y, 32);
                taken[si] = 1; ++placed;
                break;
            }
            int sj = si + 1;
            while (sj < ns && (taken[sj] || (slots[sj].vb == sl->vb && (slots[sj].y & ~(ctu - 1)) == (sl->y & ~(ctu - 1)) && (slots[sj].x + 4) / ctu == (sl->x + 4) / ctu))) ++sj;
            si = sj - 1;
        }
    }
    fprintf(stderr, "%s: %d of %d slots hold a kept patch, %d needs open\n", name, placed, ns, fc_need_open(nd));
    alf_cells_write(dir, name, f, W, H, log2_ctu, aps, mine, NULL);
}

/* ---- edge family: a patch moved sample by sample until cost() of the block at its centre is 0 */
enum { FE_HV, FE_TIE_VH, FE_TIE_DB, FE_TIE_CROSS, FE_TIE_9, FE_TIE_2 };
static uint64_t
fe_cost(const uint32_t s[4], int is_vb, int kind, int64_t target)
{
    const struct fc_cls k = fc_class(s, is_vb);
    const uint64_t zero = (!s[0] || !s[1] || !s[2] || !s[3]) ? 1000 : 0;
#define AD(a, b) ((a) > (b) ? (a) - (b) : (b) - (a))
    switch (kind) {
    case FE_HV: return AD((int64_t)s[0] + s[1], target);
    case FE_TIE_VH: return AD(s[0], s[1]) + zero;
    case FE_TIE_DB: return AD(s[2], s[3]) + zero;
    case FE_TIE_CROSS: return AD(k.cross_a, k.cross_b) + zero + (s[0] == s[1]) + (s[2] == s[3]);
    case FE_TIE_9: return AD(2 * k.max_dir, 9 * k.min_dir) + zero;
    default: return AD(k.max_dir, 2 * k.min_dir) + zero;
    }
#undef AD
}
static void
fe_search(uint16_t *py, int W, int ctu, const struct fc_slot *sl, int lower, int kind, int64_t target, const char *what)
{
    const int bx = sl->x + 4, by = sl->y + (lower ? 8 : 4), vb = (by & ~(ctu - 1)) + ctu - 4;
    uint32_t s[4];
    for (int attempt = 0; attempt < 64; ++attempt) {
        static const int amps[4] = { 4, 16, 64, 256 };
        fc_surface(py + sl->y * W + sl->x, W, kind == FE_HV ? (target < 600 ? 8 : target < 2000 ? 64 : 256) : amps[attempt & 3], kind == FE_HV ? (target < 300 ? 1 : 6) : 1 + (attempt & 3));
        int is_vb = fc_block_sums(py, W, bx, by, vb, s);
        uint64_t best = fe_cost(s, is_vb, kind, target);
        for (int step = 0; step < 20000 && best; ++step) {
            const int x = sl->x + rnd_range(0, 15), y = sl->y + rnd_range(0, 15), d = rnd_range(1, 3) * (rnd_range(0, 1) ? 1 : -1);
            const int old = py[y * W + x], v = old + d;
            if (v < 0 || v > 1023) continue;
            py[y * W + x] = (uint16_t)v;
            is_vb = fc_block_sums(py, W, bx, by, vb, s);
            const uint64_t cost = fe_cost(s, is_vb, kind, target);
            if (cost <= best) best = cost; else py[y * W + x] = (uint16_t)old;
        }
        if (!best) return;
    }
    fprintf(stderr, "alf_cells edge: no patch for %s\n", what);
    exit(1);
}

static void
alf_cells_edge_picture(const char *dir, const char *name, int W, int H)
{
    const int log2_ctu = 7, ctu = 128, nx = (W + ctu - 1) / ctu, ny = (H + ctu - 1) / ctu, n = nx * ny;
    static OVALFData aps[5];
    alf_cells_class_aps(aps);
    OVFrame *f = harness_frame(W, H);
    uint16_t *py = (uint16_t *)f->data[0];
    ovhip_alf_ctu *mine = calloc(n, sizeof(*mine));
    alf_cells_random_ctus(mine, n, aps);
    for (int i = 0; i < n; ++i) mine[i].luma_set = (7 * i + 3) % 18;
    static struct fc_slot slots[FC_MAX_SLOTS];
    const int ns = fc_slots(slots, W, H, ctu);
    int next[2] = { 0, 0 };
    char what[64];
    for (int vbk = 0; vbk < 2; ++vbk) {
        static const int edges[2][8] = { { 255, 256, 511, 512, 1791, 1792, 3839, 3840 }, { 170, 171, 341, 342, 1194, 1195, 2559, 2560 } };
#define FE_SLOT() ({ while (next[vbk] < ns && slots[next[vbk]].vb != vbk) ++next[vbk]; if (next[vbk] >= ns) { fprintf(stderr, "alf_cells edge: out of slots\n"); exit(1); } &slots[next[vbk]++]; })
        int lower = 0;
        for (int act = 0; act < 16; ++act, lower ^= vbk) {
            /* the middle of the range of sum_h + sum_v that gives this act */
            const int64_t lo = vbk ? (act * 16384 + 95) / 96 : act * 256, hi = act == 15 ? lo + 400 : vbk ? ((act + 1) * 16384 + 95) / 96 : (act + 1) * 256;
            snprintf(what, 64, "act %d vb %d", act, vbk);
            fe_search(py, W, ctu, FE_SLOT(), lower, FE_HV, (lo + hi) / 2, what);
        }
        for (int e = 0; e < 8; ++e, lower ^= vbk) {
            snprintf(what, 64, "sum %d vb %d", edges[vbk][e], vbk);
            fe_search(py, W, ctu, FE_SLOT(), lower, FE_HV, edges[vbk][e], what);
        }
        if (vbk) break;
        for (int t = FE_TIE_VH; t <= FE_TIE_2; ++t) {
            snprintf(what, 64, "tie %d", t);
            fe_search(py, W, ctu, FE_SLOT(), 0, t, 0, what);
        }
        /* the all-zero block; the largest sums: a 0 / 1023 checkerboard, stripes along the four directions */
        for (int pat = 0; pat < 6; ++pat) {
            const struct fc_slot *sl = FE_SLOT();
            for (int y = 0; y < 16; ++y)
                for (int x = 0; x < 16; ++x) {
                    const int on = pat == 0 ? 0 : pat == 1 ? (x + y) & 1 : pat == 2 ? x & 1 : pat == 3 ? y & 1 : pat == 4 ? ((x + y) >> 1) & 1 : ((x - y + 16) >> 1) & 1;
                    py[(sl->y + y) * W + sl->x + x] = pat == 0 ? 600 : on ? 1023 : 0;
                }
        }
#undef FE_SLOT
    }
    alf_cells_write(dir, name, f, W, H, log2_ctu, aps, mine, NULL);
}

/* ---- taps family.  aps[0]: alf_luma_clip_flag = 0.  aps[1]: the flag on, the classes alternately on filter 0 (every clip index 0: its
 * clip values cannot clip) and on filters 1..4, whose 12 taps carry every clip index between them; the coefficients include -128 and
 * 127.  aps[2]: 8 chroma alternatives whose 6 taps carry every clip index, the flag off or on.  CC-ALF: coefficients up to +-64. */
static void
alf_cells_taps_picture(const char *dir, const char *name, int W, int H, int log2_ctu, int chroma_clip, const struct fcell_cut *cut)
{
    const int ctu = 1 << log2_ctu, nx = (W + ctu - 1) / ctu, ny = (H + ctu - 1) / ctu, n = nx * ny;
    static OVALFData aps[5];
    for (int i = 0; i < 5; ++i) rand_alf_aps(&aps[i]);
    for (int i = 0; i < 2; ++i) {
        aps[i].alf_luma_num_filters_signalled_minus1 = 4;
        aps[i].alf_luma_clip_flag = i;
        for (int cl = 0; cl < 25; ++cl) aps[i].alf_luma_coeff_delta_idx[cl] = (cl & 1) ? 1 + ((cl >> 1) & 3) : 0;
        for (int fl = 0; fl < 5; ++fl)
            for (int k = 0; k < 12; ++k) {
                aps[i].alf_luma_clip_idx[fl][k] = fl ? (k + fl) & 3 : 0;
                if ((k + 5 * fl) % 7 == 0) aps[i].alf_luma_coeff[fl][k] = (k + fl) & 1 ? -128 : 127;
            }
    }
    if (chroma_clip)                     /* the second picture: no class of aps[0] is linear either, for waves that clip in every lane */
        for (int cl = 0; cl < 25; ++cl) { aps[0].alf_luma_clip_flag = 1; aps[0].alf_luma_coeff_delta_idx[cl] = 1 + (cl & 3); }
    aps[2].alf_chroma_clip_flag = chroma_clip;
    aps[2].alf_chroma_num_alt_filters_minus1 = 7;
    for (int a = 0; a < 8; ++a)
        for (int k = 0; k < 6; ++k) {
            aps[2].alf_chroma_clip_idx[a][k] = (k + a) & 3;
            if ((k + a) % 5 == 0) aps[2].alf_chroma_coeff[a][k] = (k + a) & 1 ? -128 : 127;
        }
    for (int cc = 0; cc < 2; ++cc) for (int k = 0; k < 7; ++k) { aps[3 + cc].alf_cc_mapped_coeff[cc][0][k] = (k + cc) & 1 ? -64 : 64; aps[3 + cc].alf_cc_mapped_coeff[cc][1][k] = k < 3 + cc ? 64 : -64; }
    OVFrame *f = fcell_frame(W, H);
    /* luma: every other 16x16 region is a surface of the class family, for classes beside the highest activity */
    for (int y = 0; y + 16 <= H; y += 16)
        for (int x = (y & 16); x + 16 <= W; x += 32) fc_draw_surface((uint16_t *)f->data[0] + y * W + x, W);
    ovhip_alf_ctu *mine = calloc(n, sizeof(*mine));
    for (int i = 0; i < n; ++i) {
        /* the three pictures between them: every flags value, every alternative on either plane under either chroma APS */
        static const uint8_t sets[6] = { 17, 16, 17, 3, 17, 12 }, flags[2][9] = { { 7, 7, 6, 5, 7, 4, 3, 7, 7 }, { 7, 2, 7, 1, 7, 0, 7, 7, 7 } };
        mine[i].flags = n == 9 ? flags[chroma_clip][i] : 7;
        mine[i].luma_set = sets[(i + chroma_clip) % 6];
        mine[i].cb_alt = n == 9 ? i & 7 : 3 + 2 * i; mine[i].cr_alt = n == 9 ? (i + 3) & 7 : 4 * i;
        mine[i].cc_cb_idx = i % 5; mine[i].cc_cr_idx = (i + 2) % 5;
        if (cut) { mine[i].flags = 7; mine[i].cb_alt = i & 7; mine[i].cr_alt = (i + 3) & 7; mine[i].cc_cb_idx = 1 + i % 4; mine[i].cc_cr_idx = 1 + (i + 2) % 4; }
    }
    alf_cells_write(dir, name, f, W, H, log2_ctu, aps, mine, cut);
}

static void
gen_alf_cells(const char *dir)
{
    g_seed = 0x266 + 14;
    struct fc_need nd;
    memset(&nd, 0, sizeof(nd));
    char name[64];
    int pic = 0;
    for (; pic < 4 && fc_need_open(&nd); ++pic) {
        snprintf(name, 64, "alf_cells_class_%02d.ovg", pic);
        alf_cells_class_picture(dir, name, 296, 264, 7, pic, &nd, 1500000);
    }
    if (fc_need_open(&nd)) {
        for (int k = 0; k < 2; ++k) for (int cl = 0; cl < 25; ++cl) for (int t = 0; t < 4; ++t) if (nd.pair[k][cl][t] < FC_TARGET(cl)) fprintf(stderr, " open: kind %d class %d transpose %d: %d\n", k, cl, t, nd.pair[k][cl][t]);
        fprintf(stderr, "alf_cells class: %d needs still open after %d pictures\n", fc_need_open(&nd), pic); exit(1);
    }
    memset(&nd, 0, sizeof(nd));
    alf_cells_class_picture(dir, "alf_cells_class64_00.ovg", 296, 264, 6, 0, &nd, 150000);     /* what so many draws reach: the pairs are all required at CTU 128 */
    alf_cells_edge_picture(dir, "alf_cells_edge_00.ovg", 296, 264);
    alf_cells_taps_picture(dir, "alf_cells_taps_00.ovg", 296, 264, 7, 0, NULL);
    alf_cells_taps_picture(dir, "alf_cells_taps_01.ovg", 296, 264, 7, 1, NULL);
    alf_cells_taps_picture(dir, "alf_cells_taps_02.ovg", 136, 72, 7, 1, NULL);      /* a single, truncated CTU row: the boundary is the picture's height */
    /* 2 x 2 rect entries, as sao_cells_entry64_00.ovg; every CTU with luma, chroma and CC-ALF on */
    static const struct fcell_cut cut = { 2, 2, { 0, 3, 5 }, { 0, 1, 4 } };
    alf_cells_taps_picture(dir, "alf_cells_entry64_00.ovg", 296, 200, 6, 1, &cut);
}

/* ====================================================================================== INTRA
 * intra.ovg : the reference's intra prediction slots on one CTU of a 2x2-CTU neighbourhood:
 *   intra_pred (planar / DC / 65 angular incl. wide angles, reference smoothing, fC / fG, PDPC, luma BDPCM),
 *   intra_pred_mrl, mip.rcn_intra_mip (+ transposed), intra_pred_c (planar / DC / angular / BDPCM) and cclm.{cclm,
 *   mdlm_left, mdlm_top} behind it                                  (rcn_structures.h:507-524, :558-593)
 * with every neighbour-availability pattern the progress bit-fields can express.  Inputs in the vocabulary of
 * include/ovvc_hip.h (ovhip_itask on a picture), outputs = the predicted block(s).
 * Picture = what the slots see of the CTU scratch (rcn_ctu.c:553-568, ctb_x = 1): the current CTU at luma (128, 128),
 * the previous CTU's columns to its left, one reconstructed row above, 64 columns of the CTU to the right. */
#define IN_W 328
#define IN_H 264
#define IN_OX 128
#define IN_OY 128

/* what gen_intra and gen_intra_cells share: the decoder context, the picture and one case through a slot */
struct intra_gen {
    OVCTUDec *c;
    struct OVRCNCtx *r;
    const struct OVBuffInfo *cb;
    gbuf b_task, b_eoff, b_exp;
    uint32_t n_cases;
};
static uint16_t g_in_py[IN_W * IN_H], g_in_pcb[(IN_W / 2) * (IN_H / 2)], g_in_pcr[(IN_W / 2) * (IN_H / 2)];

/* the picture of intra.ovg (its seed): both generators predict on the same samples */
static void
intra_gen_init(struct intra_gen *G)
{
    memset(G, 0, sizeof(*G));
    G->b_task.type = T_U8; G->b_eoff.type = T_U32; G->b_exp.type = T_U16;
    g_seed = 0x266 + 555;
    G->c = ref_new_ctudec(0, 0);
    G->c->rcn_funcs.rcn_attach_ctu_buff(&G->c->rcn_ctx, 7, 1);
    G->cb = &G->c->rcn_ctx.ctu_buff;
    G->r = &G->c->rcn_ctx;
    fill_plane(g_in_py, IN_W, IN_H, IN_W); fill_plane(g_in_pcb, IN_W / 2, IN_H / 2, IN_W / 2); fill_plane(g_in_pcr, IN_W / 2, IN_H / 2, IN_W / 2);
    for (int i = 0; i < IN_W * IN_H; i += 41) g_in_py[i] = (i & 1) ? 1023 : 0;
}

/* kind: 0 luma regular, 1 luma MRL, 2 MIP, 3 chroma regular, 4 chroma LM, 5 luma BDPCM, 6 chroma BDPCM (dir: vertical).
 * (x0, y0): inside the CTU, in samples of the plane; corner / avl_abv / avl_lft: what the progress bit-fields say (units from the corner) */
static void
intra_case(struct intra_gen *G, int kind, int l2w, int l2h, int mode, int dir, int mrl, int mip_tr, int x0, int y0, int corner, int avl_abv, int avl_lft)
{
    OVCTUDec *c = G->c;
    struct OVRCNCtx *r = G->r;
    const struct OVBuffInfo *cb = G->cb;
    const uint16_t *py = g_in_py, *pcb = g_in_pcb, *pcr = g_in_pcr;
    const int chroma = kind == 3 || kind == 4 || kind == 6;
    const int w = 1 << l2w, h = 1 << l2h, unit = chroma ? 2 : 4;
    ovhip_itask t;
    memset(&t, 0, sizeof(t));
    /* progress bit-fields: bit (unit + 1) of hfield[row above] / vfield[column left]; bit `unit` = the corner */
    struct CTUBitField *pf = chroma ? &r->progress_field_c : &r->progress_field;
    memset(pf, 0, sizeof(*pf));
    const int xu = x0 / unit, yu = y0 / unit;
    pf->hfield[yu] = (((uint64_t)corner) | ((((uint64_t)1 << avl_abv) - 1) << 1)) << xu;
    pf->vfield[xu] = (((uint64_t)corner) | ((((uint64_t)1 << avl_lft) - 1) << 1)) << yu;
    /* CTU scratch <- picture: rows -1 .. 131, columns -128 .. 195 (what the buffer holds around the CTU) */
    for (int j = -1; j < 132; ++j) for (int i = -128; i < 196; ++i) cb->y[j * cb->stride + i] = py[(IN_OY + j) * IN_W + IN_OX + i];
    for (int j = -1; j < 66; ++j) for (int i = -64; i < 98; ++i) {
        cb->cb[j * cb->stride_c + i] = pcb[(IN_OY / 2 + j) * (IN_W / 2) + IN_OX / 2 + i];
        cb->cr[j * cb->stride_c + i] = pcr[(IN_OY / 2 + j) * (IN_W / 2) + IN_OX / 2 + i]; }
    CUFlags fl = flg_pred_mode_flag;
    t.x = (uint16_t)((chroma ? IN_OX / 2 : IN_OX) + x0); t.y = (uint16_t)((chroma ? IN_OY / 2 : IN_OY) + y0);
    t.log2_w = l2w; t.log2_h = l2h; t.kind = chroma ? OVHIP_IT_CHROMA : OVHIP_IT_LUMA;
    t.mode = (uint8_t)mode; t.flags = corner ? OVHIP_IF_CORNER : 0;
    t.avl_lft = avl_lft; t.avl_abv = avl_abv; t.mrl_idx = mrl; t.level = 1;
    const double t_in = g_time ? now_s() : 0.0;
    switch (kind) {
    case 0: c->rcn_funcs.intra_pred(r, cb, mode, x0, y0, l2w, l2h, fl); break;
    case 1: c->rcn_funcs.intra_pred_mrl(c, cb->y, cb->stride, mode, x0, y0, l2w, l2h, mrl); break;
    case 2: t.flags |= OVHIP_IF_MIP | (mip_tr ? OVHIP_IF_MIP_TR : 0);
            c->rcn_funcs.mip.rcn_intra_mip(r, x0, y0, l2w, l2h, (uint8_t)(mode | (mip_tr << 7))); break;
    case 5: fl |= flg_intra_bdpcm_luma_flag | (dir ? flg_intra_bdpcm_luma_dir : 0);
            t.flags |= OVHIP_IF_BDPCM | (dir ? OVHIP_IF_BDPCM_VER : 0); t.mode = 0;
            c->rcn_funcs.intra_pred(r, cb, 0, x0, y0, l2w, l2h, fl); break;
    case 6: fl |= flg_intra_bdpcm_chroma_flag | (dir ? flg_intra_bdpcm_chroma_dir : 0);
            t.flags |= OVHIP_IF_BDPCM | (dir ? OVHIP_IF_BDPCM_VER : 0); t.mode = 0;
            c->rcn_funcs.intra_pred_c(r, 0, x0, y0, l2w, l2h, fl); break;
    case 4: {
        /* the LM modes read their own availability: abv / lft "any unit" flags, MDLM: contiguous units
         * over w + min(w, h) (h + min(w, h)) samples (rcn_intra_cclm.c:56-68, :770-776, :843-849) */
        const int any_abv = avl_abv > 0, any_lft = avl_lft > 0;
        int need_a = (w + (w < h ? w : h)) / 2, need_l = (h + (w < h ? w : h)) / 2;
        t.avl_abv = mode == 69 ? (avl_abv < need_a ? avl_abv : need_a) : any_abv;
        t.avl_lft = mode == 68 ? (avl_lft < need_l ? avl_lft : need_l) : any_lft;
        c->rcn_funcs.intra_pred_c(r, mode, x0, y0, l2w, l2h, fl); break; }
    default: c->rcn_funcs.intra_pred_c(r, mode, x0, y0, l2w, l2h, fl); break;
    }
    if (g_time) g_ts[TS_INTRA] += now_s() - t_in;
    uint32_t eoff[2] = { 0, 0 };
    if (!chroma) { eoff[0] = (uint32_t)G->b_exp.n; dump_rect(&G->b_exp, cb->y, cb->stride, x0, y0, w, h); }
    else { eoff[0] = (uint32_t)G->b_exp.n; dump_rect(&G->b_exp, cb->cb, cb->stride_c, x0, y0, w, h);
           eoff[1] = (uint32_t)G->b_exp.n; dump_rect(&G->b_exp, cb->cr, cb->stride_c, x0, y0, w, h); }
    gbuf_push(&G->b_task, &t, sizeof(t)); gbuf_push(&G->b_eoff, eoff, 2);
    G->n_cases++;
}

/* intra.ovg is kept small: big blocks take every third (fifth) mode plus the structurally special ones, big MIP blocks every other
 * matrix.  != 0: gen_intra leaves the cell (kind, shape, mi) out -- gen_intra_cells then writes it. */
static int
intra_thinned(int kind, int l2w, int l2h, int mi)
{
    const int w = 1 << l2w, h = 1 << l2h;
    const int key_mode = mi <= 2 || mi == 18 || mi == 34 || mi == 50 || mi == 66;
    const int thin = w * h >= 2048 ? 5 : w * h >= 512 ? 3 : (kind == 1 && w * h >= 128 ? 2 : 1);
    if ((kind == 0 || kind == 1 || kind == 3) && !key_mode && (mi % thin) != ((l2w * 3 + l2h) % thin)) return 1;
    if (kind == 2 && w * h >= 1024 && (mi & 1) != ((l2w + l2h) & 1)) return 1;
    return 0;
}

/* matrices of a MIP block (the standard's three size classes) */
static int mip_matrices(int l2w, int l2h) { return (l2w == 2 && l2h == 2) ? 16 : (l2h == 2 || l2w == 2 || (l2h <= 3 && l2w <= 3)) ? 8 : 6; }

static void
intra_write(struct intra_gen *G, const char *dir, const char *name, int with_pic)
{
    gfile g = gfile_open(dir, name);
    uint32_t d2[2] = { IN_H, IN_W };
    if (with_pic) {
        gfile_array(&g, "pic_y", T_U16, g_in_py, 2, d2);
        d2[0] = IN_H / 2; d2[1] = IN_W / 2;
        gfile_array(&g, "pic_cb", T_U16, g_in_pcb, 2, d2); gfile_array(&g, "pic_cr", T_U16, g_in_pcr, 2, d2);
    }
    d2[0] = G->n_cases; d2[1] = sizeof(ovhip_itask); gfile_array(&g, "task", T_U8, G->b_task.data, 2, d2);
    d2[1] = 2; gfile_array(&g, "exp_off", T_U32, G->b_eoff.data, 2, d2);
    gfile_buf(&g, "exp", &G->b_exp);
    gfile_close(&g);
    fprintf(stderr, "%s: %u cases, %zu expected samples\n", name, G->n_cases, G->b_exp.n);
}

static void
gen_intra(const char *dir)
{
    struct intra_gen G;
    intra_gen_init(&G);

    /* kind: 0 luma regular, 1 luma MRL, 2 MIP, 3 chroma regular, 4 chroma LM, 5 luma BDPCM, 6 chroma BDPCM */
    for (int kind = 0; kind < 7; ++kind) {
        const int chroma = kind == 3 || kind == 4 || kind == 6;
        const int lmin = chroma ? 1 : 2, lmax = chroma ? 5 : 6;
        for (int l2w = lmin; l2w <= lmax; ++l2w) {
            for (int l2h = lmin; l2h <= lmax; ++l2h) {
                if (chroma && l2w + l2h < 3) continue;                   /* no 2x2 chroma blocks */
                if (kind == 2 && (l2w > 6 || l2h > 6)) continue;
                if ((kind == 5 || kind == 6) && (l2w > 5 || l2h > 5)) continue;
                const int w = 1 << l2w, h = 1 << l2h, unit = chroma ? 2 : 4, ctu = chroma ? 64 : 128;
                int n_modes = kind == 0 || kind == 3 ? 67 : kind == 1 ? 67 : kind == 2 ? 32 : kind == 4 ? 3 : 2;
                int reps = kind == 0 ? (w * h <= 256 ? 3 : 2) : kind == 4 ? (w * h >= 256 ? 3 : 6) : 1;
                for (int mi = 0; mi < n_modes; ++mi) {
                    if (intra_thinned(kind, l2w, l2h, mi)) continue;
                    for (int rep = 0; rep < (w * h >= 512 && kind != 4 ? 1 : reps); ++rep) {
                        int mode = mi, mrl = 0, mip_tr = 0;
                        if (kind == 1) { if (mode == 0 || mode == 1) { if (rep) continue; } mrl = 1 + ((mi + rep) & 1); }
                        if (kind == 2) {
                            const int n_mip = mip_matrices(l2w, l2h);
                            mode = mi % n_mip; mip_tr = (mi / n_mip) & 1;
                            if (mi >= 2 * n_mip) continue;
                        }
                        if (kind == 4) mode = 67 + mi;
                        /* position inside the CTU, availability pattern */
                        int x0, y0;
                        x0 = rnd_range(0, (ctu - w) / unit) * unit; y0 = rnd_range(0, (ctu - h) / unit) * unit;
                        if (rep % 3 == 1 || (kind != 0 && rnd_range(0, 3) == 0)) { if (rnd_range(0, 1)) x0 = 0; else y0 = 0; }
                        if (kind == 1 && y0 < 4) y0 = 4 * rnd_range(1, (ctu - h) / 4 > 1 ? (ctu - h) / 4 : 1);
                        if (kind == 1 && y0 + h > ctu) continue;
                        int max_abv = 2 * w / unit, max_lft = 2 * h / unit;
                        int cap_abv = ((chroma ? 96 : 192) - x0) / unit, cap_lft = ((chroma ? 64 : 128) - y0) / unit;
                        if (max_abv > cap_abv) max_abv = cap_abv;
                        if (max_lft > cap_lft) max_lft = cap_lft;
                        int corner = 1, avl_abv = max_abv, avl_lft = max_lft;
                        /* the availability states a decoder can be in (decoding order + slice / picture borders) */
                        int pat = rnd_range(0, 9);
                        if (kind == 1 && pat < 3) pat += 3;                                       /* MRL is not signalled on the first CTU row */
                        if (pat == 0) { corner = 0; avl_abv = 0; avl_lft = 0; }                  /* nothing (picture / slice corner) */
                        else if (pat == 1) { corner = 0; avl_abv = 0; }                           /* top row */
                        else if (pat == 2) { corner = 0; avl_lft = 0; }                           /* left column */
                        else if (pat <= 5) { avl_abv = rnd_range(w / unit < max_abv ? w / unit : max_abv, max_abv);
                                             avl_lft = rnd_range(h / unit < max_lft ? h / unit : max_lft, max_lft); }
                        else if (pat == 6) { avl_abv = w / unit < max_abv ? w / unit : max_abv; avl_lft = h / unit < max_lft ? h / unit : max_lft; }
                        else if (pat == 7 && kind != 1) { corner = 0; }                          /* a slice starts at the CTU above */
                        intra_case(&G, kind, l2w, l2h, mode, mi, mrl, mip_tr, x0, y0, corner, avl_abv, avl_lft);
                    }
                }
            }
        }
    }
    intra_write(&G, dir, "intra.ovg", 1);
}

/* ---------------------------------------------------------------------------------------------------------------------
 * intra_cells_*.ovg : the cells intra.ovg does not reach, from the same slots on the same picture (the files hold tasks and
 * expected blocks only; the picture is intra.ovg's).  Everything is enumerated, positions included -- nothing is drawn:
 *   - every (shape, mode) of luma regular, MRL (modes 1..66) and chroma regular, every (shape, matrix, transposed) of MIP that
 *     gen_intra thinned out (intra_thinned), at full availability;
 *   - every (kind, shape, class) of luma regular, chroma regular, MIP and LM / MDLM over the five availability classes
 *     0 none, 1 above only, 2 left only, 3 both without the corner, 4 both with the corner -- with modes that READ the arm in
 *     question (planar: both arms; 34: the corner sample on the block's diagonal), so that the expected block differs from what
 *     full availability predicts;
 *   - every (mode, class) of luma regular (8x8) and chroma regular (4x4);
 *   - MRL at the left edge of a picture, tile or slice: avl_lft = 0, no corner, rows above available (not the CTU's first row),
 *     every shape with mrl_idx 1 and 2, modes 18 (reads only the left arm) and 34.  fill_ref_left_0_mref pads that arm with the
 *     first sample of the row above (rcn_fill_ref.c:290-310), all of it written.
 * Left out: MRL WITHOUT the rows above (classes 0 and 2).  fill_ref_above_0_mref writes 2w + 1 samples there (its "FIXME",
 * rcn_fill_ref.c:558-582) and the prediction reads up to mrl_idx + 1 past them: stack memory nothing wrote.  A decoder never
 * gets there (MRL is not signalled on a CTU's first row; rows above inside the CTU are decoded).
 * Files are cut below 1 MiB: <kind>_<nn>. */
#define CELLS_MAX_EXP 480000          /* expected samples per file */
struct cells_out { struct intra_gen *G; const char *dir, *kind; int part; };

static void
cells_flush(struct cells_out *o)
{
    char name[64];
    if (!o->G->n_cases) return;
    snprintf(name, sizeof(name), "intra_cells_%s_%02d.ovg", o->kind, o->part++);
    intra_write(o->G, o->dir, name, 0);
    o->G->b_task.n = o->G->b_eoff.n = o->G->b_exp.n = 0; o->G->n_cases = 0;
}

/* one enumerated case: class cls, arms as long as they get (ext 0) or as long as the block (ext 1), position k of the shape */
static void
cells_case(struct cells_out *o, int kind, int l2w, int l2h, int mode, int mrl, int mip_tr, int cls, int ext, int k)
{
    const int chroma = kind == 3 || kind == 4;
    const int w = 1 << l2w, h = 1 << l2h, unit = chroma ? 2 : 4, ctu = chroma ? 64 : 128;
    const int nx = (ctu - w) / unit + 1, ny = (ctu - h) / unit + 1;
    int x0 = unit * ((7 * k + 3 * l2w + 5 * l2h + 11 * cls) % nx), y0 = unit * ((5 * k + 7 * l2w + 3 * l2h + 13 * cls + 1) % ny);
    if (kind == 1) y0 = 4 * (1 + (5 * k + l2w + cls) % ((ctu - h) / 4));         /* MRL: not the CTU's first row, rows above inside the picture */
    if (kind == 4) {
        /* LM: half of the cases on the CTU's first line (one luma row above instead of two); the others on no row that starts a
         * CTU of 32 or 64 either (tests place the cases at those CTU sizes) */
        if ((k + cls + l2w + l2h) & 1) y0 = 0;
        else if ((2 * y0) % 32 == 0) y0 += y0 + 2 + h <= ctu ? 2 : -2;
    }
    int max_abv = 2 * w / unit, max_lft = 2 * h / unit;
    const int cap_abv = ((chroma ? 96 : 192) - x0) / unit, cap_lft = ((chroma ? 64 : 128) - y0) / unit;
    if (max_abv > cap_abv) max_abv = cap_abv;
    if (max_lft > cap_lft) max_lft = cap_lft;
    if (ext) { if (max_abv > w / unit) max_abv = w / unit; if (max_lft > h / unit) max_lft = h / unit; }
    const int corner = cls == 4, avl_abv = (cls == 1 || cls >= 3) ? max_abv : 0, avl_lft = cls >= 2 ? max_lft : 0;
    if (o->G->b_exp.n + (size_t)(chroma ? 2 : 1) * w * h > CELLS_MAX_EXP) cells_flush(o);
    intra_case(o->G, kind, l2w, l2h, mode, 0, mrl, mip_tr, x0, y0, corner, avl_abv, avl_lft);
}

static void
gen_intra_cells(const char *dir)
{
    struct intra_gen G;
    intra_gen_init(&G);                       /* intra.ovg's picture */
    g_seed = 0x266 + 556;                     /* (this generator's own; it draws nothing) */
    static const char *names[5] = { "luma", "mrl", "mip", "chroma", "lm" };
    for (int kind = 0; kind < 5; ++kind) {
        struct cells_out o = { &G, dir, names[kind], 0 };
        const int chroma = kind >= 3, lmin = chroma ? 1 : 2, lmax = chroma ? 5 : 6;
        for (int l2w = lmin; l2w <= lmax; ++l2w) {
            for (int l2h = lmin; l2h <= lmax; ++l2h) {
                if (chroma && l2w + l2h < 3) continue;                   /* no 2x2 chroma blocks */
                /* (a) the cells gen_intra thinned out */
                if (kind == 0 || kind == 3) for (int m = 0; m < 67; ++m) { if (intra_thinned(kind, l2w, l2h, m)) cells_case(&o, kind, l2w, l2h, m, 0, 0, 4, m & 1, m); }
                if (kind == 1) for (int m = 1; m < 67; ++m) { if (intra_thinned(kind, l2w, l2h, m)) cells_case(&o, kind, l2w, l2h, m, 1 + (m & 1), 0, 4, (m >> 1) & 1, m); }
                if (kind == 2) {
                    const int n_mip = mip_matrices(l2w, l2h);
                    for (int mi = 0; mi < 2 * n_mip; ++mi) if (intra_thinned(kind, l2w, l2h, mi)) cells_case(&o, kind, l2w, l2h, mi % n_mip, 0, mi / n_mip, 4, mi & 1, mi);
                }
                /* (b), (d) every availability class, with modes that read the arm in question */
                for (int cls = 0; cls < 5; ++cls) {
                    if (kind == 0 || kind == 3) { cells_case(&o, kind, l2w, l2h, 0, 0, 0, cls, 0, cls); cells_case(&o, kind, l2w, l2h, 34, 0, 0, cls, 1, cls + 5); }
                    if (kind == 2) cells_case(&o, kind, l2w, l2h, (l2w + 2 * l2h + cls) % mip_matrices(l2w, l2h), 0, cls & 1, cls, cls & 1, cls);
                    if (kind == 4) for (int m = 67; m < 70; ++m) cells_case(&o, kind, l2w, l2h, m, 0, 0, cls, 0, m - 67 + 3 * cls);
                }
                /* (c) MRL at a left edge */
                if (kind == 1) for (int mrl = 1; mrl <= 2; ++mrl) { cells_case(&o, kind, l2w, l2h, 18, mrl, 0, 1, 0, mrl); cells_case(&o, kind, l2w, l2h, 34, mrl, 0, 1, 1, mrl + 2); }
            }
        }
        /* (b) every (mode, class) */
        if (kind == 0) for (int m = 0; m < 67; ++m) for (int cls = 0; cls < 5; ++cls) cells_case(&o, kind, 3, 3, m, 0, 0, cls, (m + cls) & 1, m + cls);
        if (kind == 3) for (int m = 0; m < 67; ++m) for (int cls = 0; cls < 5; ++cls) cells_case(&o, kind, 2, 2, m, 0, 0, cls, (m + cls) & 1, m + cls);
        cells_flush(&o);
    }
}
/* ---------------------------------------------------------------------------------------------------------------------
 * K12  whole intra CTUs through tmp.rcn_transform_tree (rcn_transform_tree.c:1454-1518 -> rcn_res_wrap -> rcn_intra_tu /
 *      rcn_tu_st / rcn_tu_l / rcn_tu_c): a random partition of the CTU at (128, 128), CUs in decoding order, every CU intra
 *      (regular / MRL / MIP / BDPCM luma, DC / planar / angular / DM / LM / MDLM chroma, with residuals: DCT-2, implicit MTS,
 *      LFNST, transform skip) or left as it is ("decoded before", as an inter CU would be).  Single tree and dual tree.
 *      Reference mode: intra_ctu.ovg = the start picture + the CTU each case ends with.
 *      Shim mode: shim_intra_ctu.ovg = what the installed slots recorded for the same CTUs (commands, coefficients, ordered
 *      tasks).  Executing the stream on the start picture must give the reference's CTU. */
struct ictu_cu { int x, y, l2w, l2h; };
static void
ictu_part(struct ictu_cu *out, int *n, int x, int y, int l2w, int l2h)
{
    const int w = 1 << l2w, h = 1 << l2h;
    int choice = 0;                                  /* 0 leaf, 1 quad, 2 vertical, 3 horizontal */
    if (w > 64 || h > 64) choice = 1;
    else {
        const int r = rnd_range(0, 99);
        const int p_leaf = w * h >= 2048 ? 25 : w * h >= 512 ? 45 : w * h >= 128 ? 60 : 85;
        if (r >= p_leaf) {
            int opts[3], no = 0;
            if (l2w == l2h && l2w >= 4) opts[no++] = 1;
            if (l2w >= 4) opts[no++] = 2;
            if (l2h >= 3) opts[no++] = 3;
            if (no) choice = opts[rnd_range(0, no - 1)];
        }
    }
    if (choice == 0) { out[*n] = (struct ictu_cu){ x, y, l2w, l2h }; ++*n; return; }
    if (choice == 1) {
        ictu_part(out, n, x, y, l2w - 1, l2h - 1); ictu_part(out, n, x + w / 2, y, l2w - 1, l2h - 1);
        ictu_part(out, n, x, y + h / 2, l2w - 1, l2h - 1); ictu_part(out, n, x + w / 2, y + h / 2, l2w - 1, l2h - 1);
    } else if (choice == 2) { ictu_part(out, n, x, y, l2w - 1, l2h); ictu_part(out, n, x + w / 2, y, l2w - 1, l2h); }
    else { ictu_part(out, n, x, y, l2w, l2h - 1); ictu_part(out, n, x, y + h / 2, l2w, l2h - 1); }
}

static void
gen_intra_ctu(const char *dir)
{
    extern int transform_unit_st(OVCTUDec *const, unsigned int, unsigned int, unsigned int, unsigned int, uint8_t, CUFlags, uint8_t, struct TUInfo *const);
    extern int transform_unit_l(OVCTUDec *const, unsigned int, unsigned int, unsigned int, unsigned int, uint8_t, CUFlags, uint8_t, struct TUInfo *const);
    extern int transform_unit_c(OVCTUDec *const, unsigned int, unsigned int, unsigned int, unsigned int, uint8_t, CUFlags, uint8_t, struct TUInfo *const);
    gbuf b_exp = { .type = T_U16 }, b_info = { .type = T_I32 };
    uint32_t n_cases = 0;
    g_seed = 0x266 + 777;
    OVCTUDec *c = ref_new_ctudec(0, 0);
    c->rcn_funcs.rcn_attach_ctu_buff(&c->rcn_ctx, 7, 1);
    const struct OVBuffInfo *cb = &c->rcn_ctx.ctu_buff;
    struct OVRCNCtx *r = &c->rcn_ctx;
    static uint16_t py[IN_W * IN_H], pcb[(IN_W / 2) * (IN_H / 2)], pcr[(IN_W / 2) * (IN_H / 2)];
    fill_plane(py, IN_W, IN_H, IN_W); fill_plane(pcb, IN_W / 2, IN_H / 2, IN_W / 2); fill_plane(pcr, IN_W / 2, IN_H / 2, IN_W / 2);
    struct shim_stream S;
    shim_stream_init(&S);
    c->ctb_x = IN_OX >> 7; c->ctb_y = IN_OY >> 7;
    if (g_shim) shim_bind(c, IN_W, IN_H, 0, 0);

    for (int ci = 0; ci < 36; ++ci) {
        const int dual = ci % 3 == 2;
        struct ictu_cu cus[1024]; int n_cu = 0;
        ictu_part(cus, &n_cu, 0, 0, 7, 7);
        const int ict_type = rnd_range(0, 3);
        rcn_init_ict_functions_10(&c->rcn_funcs, ict_type, 10);
        if (g_shim) rcn_init_functions_hip(&c->rcn_funcs, ict_type, 1, 0, 0, 10);
        c->dequant_luma.qp = rnd_range(18, 50); c->dequant_cb.qp = rnd_range(18, 50); c->dequant_cr.qp = rnd_range(18, 50);
        c->dequant_joint_cb_cr.qp = rnd_range(18, 50);
        c->dequant_luma_skip.qp = c->dequant_luma.qp; c->dequant_cb_skip.qp = c->dequant_cb.qp; c->dequant_cr_skip.qp = c->dequant_cr.qp;
        c->dequant_jcbcr_skip.qp = c->dequant_joint_cb_cr.qp;
        c->residual_coding_l = rnd_range(0, 1) ? &residual_coding_dpq : NULL;
        c->mts_implicit = rnd_range(0, 1); c->sh_ts_disabled = 0; c->tmp_ciip = 0;
        c->lmcs_info.scale_c_flag = rnd_range(0, 1); c->lmcs_info.lmcs_chroma_scale = (uint16_t)rnd_range(1200, 3400);
        memset(&c->dbf_info, 0, sizeof(c->dbf_info));
        /* the CTU scratch holds the picture around the CTU; the neighbours that exist: left and above CTUs, and the part of the
         * above-right one inside the picture */
        for (int j = -1; j < 132; ++j) for (int i = -128; i < 196; ++i) cb->y[j * cb->stride + i] = py[(IN_OY + j) * IN_W + IN_OX + i];
        for (int j = -1; j < 66; ++j) for (int i = -64; i < 98; ++i) {
            cb->cb[j * cb->stride_c + i] = pcb[(IN_OY / 2 + j) * (IN_W / 2) + IN_OX / 2 + i];
            cb->cr[j * cb->stride_c + i] = pcr[(IN_OY / 2 + j) * (IN_W / 2) + IN_OX / 2 + i];
        }
        /* the decoder's own CTU start (decode_ctu, slicedec.c:731-737): left, above and above-right CTUs exist, the last one
         * only as far as the picture goes */
        memset(&r->progress_field, 0, sizeof(r->progress_field)); memset(&r->progress_field_c, 0, sizeof(r->progress_field_c));
        init_ctu_bitfield(r, CTU_LFT_FLG | CTU_UP_FLG | CTU_UPRGT_FLG, 7);
        {
            const uint64_t mask = ((uint64_t)1 << ((((IN_W - IN_OX - 128) + 128) >> 2) + 1)) - 1;
            r->progress_field_c.hfield[0] &= mask; r->progress_field.hfield[0] &= mask;
        }
        int n_intra = 0;
        uint8_t luma_mode_of[1024];
        for (int pass = 0; pass < (dual ? 2 : 1); ++pass) {
            c->transform_unit = dual ? (pass ? (void *)&transform_unit_c : (void *)&transform_unit_l) : (void *)&transform_unit_st;
            for (int k = 0; k < n_cu; ++k) {
                const int x0 = cus[k].x, y0 = cus[k].y, l2w = cus[k].l2w, l2h = cus[k].l2h, w = 1 << l2w, h = 1 << l2h;
                struct TUInfo tu;
                memset(&tu, 0, sizeof(tu));
                /* "decoded before": the same CUs in both passes of a dual tree */

                const int skip = ((cus[k].x * 31 + cus[k].y * 17 + ci * 7) % 100) < 22;
                if (skip) {
                    struct CTUBitField *pf = (dual && pass) ? &r->progress_field_c : &r->progress_field;
                    ctu_field_set_rect_bitfield(pf, x0 >> 2, y0 >> 2, w >> 2, h >> 2);
                    if (!dual) ctu_field_set_rect_bitfield(&r->progress_field_c, x0 >> 2, y0 >> 2, w >> 2, h >> 2);
                    continue;
                }
                CUFlags fl = flg_pred_mode_flag;
                int kind = rnd_range(0, 99);                      /* luma: regular / MRL / MIP / BDPCM */
                kind = kind < 50 ? 0 : kind < 65 ? 1 : kind < 82 ? 2 : 3;
                if (kind == 1 && y0 == 0) kind = 0;               /* MRL is not signalled on the first line of a CTU */
                if (kind == 3 && (l2w > 5 || l2h > 5)) kind = 0;
                int mode = rnd_range(0, 66), mode_c;
                int bdpcm_c = 0;
                if (!(dual && pass)) {
                    c->cu_opaque = 0;
                    if (kind == 1) { fl |= flg_mrl_flag; c->cu_opaque = (uint8_t)rnd_range(1, 2); }
                    if (kind == 2) {
                        const int n_mip = (l2w == 2 && l2h == 2) ? 16 : (l2h == 2 || l2w == 2 || (l2h <= 3 && l2w <= 3)) ? 8 : 6;
                        fl |= flg_mip_flag; c->cu_opaque = (uint8_t)(rnd_range(0, n_mip - 1) | (rnd_range(0, 1) << 7));
                        mode = 0;
                    }
                    if (kind == 3) { fl |= flg_intra_bdpcm_luma_flag | (rnd_range(0, 1) ? flg_intra_bdpcm_luma_dir : 0); mode = (fl & flg_intra_bdpcm_luma_dir) ? 50 : 18; }
                    luma_mode_of[k] = (uint8_t)mode;
                } else {
                    mode = luma_mode_of[k];
                }
                c->intra_mode = (uint8_t)mode;
                {
                    static const uint8_t cm[8] = { 0, 1, 18, 50, 255, 67, 68, 69 };
                    mode_c = cm[rnd_range(0, 7)];
                    if (mode_c == 255) mode_c = mode;             /* DM */
                    if (kind == 3 && l2w <= 5 && l2h <= 5 && rnd_range(0, 1)) { bdpcm_c = 1; fl |= flg_intra_bdpcm_chroma_flag | (rnd_range(0, 1) ? flg_intra_bdpcm_chroma_dir : 0); }
                }
                c->intra_mode_c = (uint8_t)mode_c;
                /* residual */
                const int has_l = !(dual && pass) && rnd_range(0, 99) < 70;
                static const uint8_t cbf_c[7] = { 0, 0x2, 0x1, 0x3, 0xb, 0xa, 0x9 };
                int cbfc = (dual && !pass) ? 0 : cbf_c[rnd_range(0, 6)];
                if (bdpcm_c) cbfc &= 0x3;
                tu.cbf_mask = (uint8_t)((has_l ? 0x10 : 0) | cbfc);
                int lfnst = !(fl & (flg_intra_bdpcm_luma_flag)) && has_l && rnd_range(0, 3) == 0;
                if (lfnst) { tu.lfnst_flag = 1; tu.lfnst_idx = (uint8_t)rnd_range(0, 1); }
                if (fl & flg_intra_bdpcm_luma_flag) tu.tr_skip_mask |= 0x10;
                if (bdpcm_c) tu.tr_skip_mask |= 0x3;
                int16_t *res[3] = { c->residual_cb, c->residual_cr, c->residual_y };
                const int cl2w = (dual && pass) ? l2w - 1 : l2w - 1, cl2h = l2h - 1;
                for (int comp = 0; comp < 3; ++comp) {
                    const int is_l = comp == 2;
                    const int used = is_l ? has_l : ((cbfc & 0x8) ? comp == 0 : !!(cbfc & (comp ? 0x1 : 0x2)));
                    if (!used) continue;
                    const int tl2w = is_l ? l2w : cl2w, tl2h = is_l ? l2h : cl2h;
                    const int ts = is_l ? !!(tu.tr_skip_mask & 0x10) : (cbfc & 0x8) ? !!(tu.tr_skip_mask & 0x1) : !!(tu.tr_skip_mask & (comp ? 0x1 : 0x2));
                    const int raster = ts || tl2w < 2 || tl2h < 2;
                    uint64_t map; uint16_t lp;
                    make_coefs(res[comp], tl2w, tl2h, (is_l && lfnst) ? 1 : rnd_range(0, 2), raster, &map, &lp);
                    if (is_l && lfnst) {
                        map = 1; lp = 0x0101;
                        if (!raster) { int cw = (1 << tl2w) > 32 ? 32 : (1 << tl2w), ch = (1 << tl2h) > 32 ? 32 : (1 << tl2h); memset(res[comp] + 16, 0, (cw * ch - 16) * 2); }
                    }
                    tu.tb_info[comp].sig_sb_map = map; tu.tb_info[comp].last_pos = lp;
                }
                if (dual && pass) c->rcn_funcs.tmp.rcn_transform_tree(c, x0 >> 1, y0 >> 1, l2w - 1, l2h - 1, 5, 0, fl, &tu);
                else c->rcn_funcs.tmp.rcn_transform_tree(c, x0, y0, l2w, l2h, 6, 0, fl, &tu);
                ++n_intra;
            }
        }
        if (g_shim) shim_case_end(c, &S, "intra ctu");
        int32_t info[4] = { dual, n_cu, n_intra, (int32_t)b_exp.n };
        gbuf_push(&b_info, info, 4);
        dump_rect(&b_exp, cb->y, cb->stride, 0, 0, 128, 128);
        dump_rect(&b_exp, cb->cb, cb->stride_c, 0, 0, 64, 64);
        dump_rect(&b_exp, cb->cr, cb->stride_c, 0, 0, 64, 64);
        n_cases++;
    }
    if (g_shim) { shim_stream_write(dir, "shim_intra_ctu.ovg", &S, c, NULL, 0); return; }
    gfile g = gfile_open(dir, "intra_ctu.ovg");
    uint32_t d2[2] = { IN_H, IN_W };
    gfile_array(&g, "pic_y", T_U16, py, 2, d2);
    d2[0] = IN_H / 2; d2[1] = IN_W / 2;
    gfile_array(&g, "pic_cb", T_U16, pcb, 2, d2); gfile_array(&g, "pic_cr", T_U16, pcr, 2, d2);
    d2[0] = n_cases; d2[1] = 4; gfile_array(&g, "info", T_I32, b_info.data, 2, d2);
    gfile_buf(&g, "exp", &b_exp);
    gfile_close(&g);
    fprintf(stderr, "intra_ctu.ovg: %u CTUs, %zu expected samples\n", n_cases, b_exp.n);
}

/* ---------------------------------------------------------------------------------------------------------------------
 * K13  intra sub-partitions: tmp.recon_isp_subtree_v / _h (rcn_transform_tree.c:1087-1205 -> intra_pred_isp, rcn_isp_tu,
 *      rcn_2xX_tb / rcn_1xX_tb / rcn_Xx2_tb / rcn_Xx1_tb): every CU shape ISP exists for (4x8 ... 64x64), both split
 *      directions, planar / DC / angular modes incl. wide angles, DST-VII on and off, LFNST, random cbf patterns; the CU sits in
 *      a CTU whose surroundings are partly decoded.  isp.ovg = start picture + the CU each case ends with; shim mode:
 *      shim_isp.ovg = what the installed slots recorded. */
struct ISPTUInfo_h { uint8_t cbf_mask, tr_skip_mask, cu_mts_flag, cu_mts_idx, lfnst_flag, lfnst_idx; struct TBInfo tb_info[4]; };
static void
gen_isp(const char *dir)
{
    gbuf b_exp = { .type = T_U16 }, b_info = { .type = T_I32 };
    uint32_t n_cases = 0;
    g_seed = 0x266 + 999;
    OVCTUDec *c = ref_new_ctudec(0, 0);
    c->rcn_funcs.rcn_attach_ctu_buff(&c->rcn_ctx, 7, 1);
    const struct OVBuffInfo *cb = &c->rcn_ctx.ctu_buff;
    struct OVRCNCtx *r = &c->rcn_ctx;
    static uint16_t py[IN_W * IN_H], pcb[(IN_W / 2) * (IN_H / 2)], pcr[(IN_W / 2) * (IN_H / 2)];
    fill_plane(py, IN_W, IN_H, IN_W); fill_plane(pcb, IN_W / 2, IN_H / 2, IN_W / 2); fill_plane(pcr, IN_W / 2, IN_H / 2, IN_W / 2);
    struct shim_stream S;
    shim_stream_init(&S);
    c->ctb_x = IN_OX >> 7; c->ctb_y = IN_OY >> 7;
    if (g_shim) shim_bind(c, IN_W, IN_H, 0, 0);
    for (int l2w = 2; l2w <= 6; ++l2w)
        for (int l2h = 2; l2h <= 6; ++l2h) {
            if (l2w + l2h < 5) continue;                                 /* no ISP for 4x4 */
            for (int vertical = 0; vertical < 2; ++vertical) {
                /* the standard forbids a split that would leave partitions wider / higher than the maximum transform size only;
                 * both directions exist for every shape here */
                const int reps = (l2w + l2h <= 8) ? 10 : 6;
                /* 64x8 split horizontally = 64x2 partitions: rcn_Xx2_tb de-quantises with a row stride of 32 (dequant_tb, min(5,
                 * log2_tb_w)) but transforms with a stride of 64, reading stack memory nothing initialised (:985-1009): the
                 * reference's output for these is not a function of its inputs, there is nothing to pin (the recorder refuses them) */
                if (!vertical && l2w == 6 && l2h == 3) continue;
                for (int rep = 0; rep < reps; ++rep) {
                    const int w = 1 << l2w, h = 1 << l2h;
                    int32_t l2p, n_pb, l2pred, n_pred;
                    ovhip_isp_geometry(l2w, l2h, vertical, &l2p, &n_pb, &l2pred, &n_pred);
                    const int l2tw = vertical ? l2p : l2w, l2th = vertical ? l2h : l2p;
                    int x0 = rnd_range(0, (128 - w) / 4) * 4, y0 = rnd_range(0, (128 - h) / 4) * 4;
                    if (rep % 4 == 1) { if (rnd_range(0, 1)) x0 = 0; else y0 = 0; }
                    static const uint8_t key[8] = { 0, 1, 2, 18, 34, 50, 66, 0 };
                    const int mode = rep < 7 ? key[rep] : rnd_range(2, 66);
                    const int mode2 = (rep & 1) ? rnd_range(2, 66) : mode;
                    const uint8_t intra_mode = (uint8_t)(rep >= 3 && rep < 7 ? mode2 : mode);
                    c->dequant_luma.qp = rnd_range(18, 50); c->dequant_luma_skip.qp = c->dequant_luma.qp;
                    c->residual_coding_l = rnd_range(0, 1) ? &residual_coding_dpq : NULL;
                    c->mts_enabled = (uint8_t)rnd_range(0, 1); c->mts_implicit = 0; c->sh_ts_disabled = 0; c->tmp_ciip = 0;
                    c->intra_mode = intra_mode;
                    memset(&c->dbf_info, 0, sizeof(c->dbf_info));
                    for (int j = -1; j < 132; ++j) for (int i = -128; i < 196; ++i) cb->y[j * cb->stride + i] = py[(IN_OY + j) * IN_W + IN_OX + i];
                    /* progress: the decoder's CTU start, the rows above the CU and the columns left of it inside the CTU decoded
                     * (with some of the left part further down), then the CU itself (vcl_transform_unit.c:1878) */
                    memset(&r->progress_field, 0, sizeof(r->progress_field)); memset(&r->progress_field_c, 0, sizeof(r->progress_field_c));
                    int flags = CTU_LFT_FLG | CTU_UP_FLG | CTU_UPRGT_FLG;
                    if (rep % 5 == 2) flags &= ~CTU_UP_FLG & ~CTU_UPRGT_FLG;
                    if (rep % 5 == 3) flags &= ~CTU_LFT_FLG;
                    init_ctu_bitfield(r, (uint8_t)flags, 7);
                    { const uint64_t mask = ((uint64_t)1 << ((((IN_W - IN_OX - 128) + 128) >> 2) + 1)) - 1; r->progress_field.hfield[0] &= mask; }
                    const int xu = x0 >> 2, yu = y0 >> 2, wu = w >> 2, hu = h >> 2;
                    if (yu) ctu_field_set_rect_bitfield(&r->progress_field, 0, 0, rnd_range(0, 2) ? 32 : (xu + wu < 32 ? xu + wu : 32), yu);
                    if (xu) { int nl = rnd_range(hu, 2 * hu); if (yu + nl > 32) nl = 32 - yu; ctu_field_set_rect_bitfield(&r->progress_field, 0, yu, xu, nl); }
                    ctu_field_set_rect_bitfield(&r->progress_field, xu, yu, wu, hu);
                    /* residual */
                    struct ISPTUInfo_h tu;
                    memset(&tu, 0, sizeof(tu));
                    memset(c->residual_y, 0, sizeof(c->residual_y));
                    tu.cbf_mask = (uint8_t)rnd_range(1, (1 << n_pb) - 1);
                    const int can_lfnst = l2tw >= 2 && l2th >= 2;
                    if (can_lfnst && rnd_range(0, 3) == 0) { tu.lfnst_flag = 1; tu.lfnst_idx = (uint8_t)rnd_range(0, 1); }
                    for (int i = 0; i < n_pb; ++i) {
                        if (!((tu.cbf_mask >> (n_pb - i - 1)) & 1)) continue;
                        int16_t *dst = c->residual_y + (i << (l2tw + l2th));
                        uint64_t map; uint16_t lp;
                        if (l2tw >= 2 && l2th >= 2) {
                            make_coefs(dst, l2tw, l2th, tu.lfnst_flag ? 1 : rnd_range(0, 2), 0, &map, &lp);
                            if (tu.lfnst_flag) { map = 1; lp = 0x0101; int cw = (1 << l2tw) > 32 ? 32 : (1 << l2tw), ch = (1 << l2th) > 32 ? 32 : (1 << l2th); memset(dst + 16, 0, (cw * ch - 16) * 2); }
                        } else {
                            /* thin blocks: raster; the sub-block map of 2x8 / 8x2 (1x16 / 16x1) coefficient groups along the long side */
                            const int n = 1 << (l2tw + l2th);
                            const int pattern = rnd_range(0, 2);
                            for (int k = 0; k < n; ++k) dst[k] = (pattern == 2 || (pattern == 1 && rnd_range(0, 2) == 0) || k == 0) ? rnd_coef() : 0;
                            const int n_sb = n >> 4;                     /* 16 coefficients per group */
                            map = 0;
                            for (int sb = 0; sb < (n_sb ? n_sb : 1); ++sb) map |= (uint64_t)1 << (vertical ? sb * 8 : sb);
                            if (pattern == 0) { map = 1; for (int k = 1; k < n; ++k) dst[k] = 0; }
                            lp = (uint16_t)(pattern == 0 ? 0 : (vertical ? ((((1 << l2th) - 1) & 0x1f) << 8) | (((1 << l2th) - 1) & 0x1f) : ((1 << l2tw) - 1) & 0x1f));
                        }
                        tu.tb_info[i].sig_sb_map = map; tu.tb_info[i].last_pos = lp;
                    }
                    rcn_init_ict_functions_10(&c->rcn_funcs, 0, 10);
                    if (g_shim) rcn_init_functions_hip(&c->rcn_funcs, 0, 1, 0, 0, 10);
                    if (vertical) c->rcn_funcs.tmp.recon_isp_subtree_v(c, x0, y0, l2w, l2h, intra_mode, (const void *)&tu);
                    else          c->rcn_funcs.tmp.recon_isp_subtree_h(c, x0, y0, l2w, l2h, intra_mode, (const void *)&tu);
                    if (g_shim) shim_case_end(c, &S, "isp");
                    int32_t info[8] = { IN_OX + x0, IN_OY + y0, l2w, l2h, vertical, intra_mode, tu.cbf_mask | (tu.lfnst_flag << 8) | (c->mts_enabled << 9), (int32_t)b_exp.n };
                    gbuf_push(&b_info, info, 8);
                    dump_rect(&b_exp, cb->y, cb->stride, x0, y0, w, h);
                    n_cases++;
                }
            }
        }
    if (g_shim) { shim_stream_write(dir, "shim_isp.ovg", &S, c, NULL, 0); return; }
    gfile g = gfile_open(dir, "isp.ovg");
    uint32_t d2[2] = { IN_H, IN_W };
    gfile_array(&g, "pic_y", T_U16, py, 2, d2);
    d2[0] = n_cases; d2[1] = 8; gfile_array(&g, "info", T_I32, b_info.data, 2, d2);
    gfile_buf(&g, "exp", &b_exp);
    gfile_close(&g);
    fprintf(stderr, "isp.ovg: %u CUs, %zu expected samples\n", n_cases, b_exp.n);
}

int
main(int argc, char **argv)
{
    const char *dir = argc > 1 ? argv[1] : "../tests/golden";
    const char *only = argc > 2 ? argv[2] : NULL;
    if (only && !strcmp(only, "shim")) { g_shim = 1; only = argc > 3 ? argv[3] : NULL; }
    /* "simd": the same generators through the reference's SSE4.1 / AVX2 slots (`gen_golden <scratch dir> simd` rewrites the
     * fixtures from them -- byte-identical to the scalar ones if the reference's back-ends agree; `... simd time` times them) */
    if (only && !strcmp(only, "simd")) { g_simd = 1; only = argc > 3 ? argv[3] : NULL; }
    if (only && !strcmp(only, "time")) {
        /* five passes over the generators, the best time per stage; fixtures go to `dir` (use a scratch directory) */
        double best[TS_N];
        for (int k = 0; k < TS_N; ++k) best[k] = 1e30;
        g_time = 1;
        for (int pass = 0; pass < 5; ++pass) {
            memset(g_ts, 0, sizeof(g_ts));
            gen_itx(dir); gen_mc(dir); gen_dbf(dir, 0); gen_sao(dir, 7); gen_alf(dir, 7); gen_intra(dir);
            for (int k = 0; k < TS_N; ++k) if (g_ts[k] > 0 && g_ts[k] < best[k]) best[k] = g_ts[k];
        }
        printf("{");
        int first = 1;
        for (int k = 0; k < TS_N; ++k) if (best[k] < 1e29) { printf("%s\"%s\": %.6f", first ? "" : ", ", g_ts_name[k], best[k]); first = 0; }
        printf("}\n");
        return 0;
    }
    if (!only || !strcmp(only, "itx")) gen_itx(dir);
    if (!only || !strcmp(only, "mc"))  gen_mc(dir);
    if (!only || !strcmp(only, "mcx")) gen_mcx(dir);
    if (!only || !strcmp(only, "mca")) gen_mca(dir);
    if (!only || !strcmp(only, "lmcs")) gen_lmcs(dir);
    if (!only || !strcmp(only, "gpm")) gen_gpm(dir);
    if (!only || !strcmp(only, "dbf")) gen_dbf(dir, 0);
    /* deblocking's second profile (table ends, long filters, several offset pairs): by name only, like the CTU sizes below */
    if (only && !strcmp(only, "dbf_ends")) gen_dbf(dir, 1);
    if (!only || !strcmp(only, "sao")) gen_sao(dir, 7);
    if (!only || !strcmp(only, "alf")) gen_alf(dir, 7);
    /* SAO and ALF at the smaller CTU sizes: asked for by name only, each a run of its own (a generator seeds itself) */
    if (only && !strcmp(only, "sao_ctu64")) gen_sao(dir, 6);
    if (only && !strcmp(only, "sao_ctu32")) gen_sao(dir, 5);
    if (only && !strcmp(only, "alf_ctu64")) gen_alf(dir, 6);
    if (only && !strcmp(only, "alf_ctu32")) gen_alf(dir, 5);
    if ((!only || !strcmp(only, "intra")) && !g_shim) gen_intra(dir);
    /* the cells intra.ovg does not reach: by name only, a run of its own */
    if (only && !strcmp(only, "intra_cells") && !g_shim) gen_intra_cells(dir);
    if (only && !strcmp(only, "itx_cells") && !g_shim) gen_itx_cells(dir);
    /* the enumerated inter prediction cells: by name only, each a run of its own */
    if (only && !strcmp(only, "mc_cells") && !g_shim) gen_mc_cells(dir);
    if (only && !strcmp(only, "mcx_cells") && !g_shim) gen_mcx_cells(dir);
    /* the enumerated SAO and ALF cells: by name only, each a run of its own */
    if (only && !strcmp(only, "sao_cells") && !g_shim) gen_sao_cells(dir);
    if (only && !strcmp(only, "alf_cells") && !g_shim) gen_alf_cells(dir);
    if (!only || !strcmp(only, "intra_ctu")) gen_intra_ctu(dir);
    if (!only || !strcmp(only, "isp")) gen_isp(dir);
    return 0;
}
