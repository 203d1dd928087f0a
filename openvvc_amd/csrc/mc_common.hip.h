// mc_common.hip.h -- device building blocks shared by the inter-prediction kernels: plain units (kernels_mc.hip), refined BDOF /
// DMVR and affine units (kernels_mcx.hip), units that read a reference of another size (kernels_rpr.hip).  Every decision that more
// than one of them takes is written here once:
//   ref_table                        the launchers' reference table and its argument checks
//   WinStage, stage_unit_windows     reference windows of a <= 16x16 unit -> LDS (k_mc2, k_mcx)
//   AffStage                         reference window of one 4x4 affine block -> LDS (k_mca: luma 9x9, chroma 7x7)
//   fir4 / firn, h_task, h_pass, v_pass, v_outputs    packed v_dot2 FIR; separable H (LDS->LDS, transposed) and V (LDS->registers) passes
//   Combine, mc_gpm, ciip_blend      uni / average / BCW, geometric-partition and CIIP blends of the lists' 14-bit intermediates
//   chroma_finish                    chroma V pass + combine + store of a unit (k_mc2, k_mcx)
//   prof_ring, prof_fill, prof_refine    PROF on a 6x6 tile (k_mca, k_mca_rpr)
#pragma once
#include "ovvc_common.hip.h"
#define OVT_ATTR __device__
#include "vvc_mc_taps.h"

namespace {

#define MC_MAX_REFS 16
struct RefTable { ovhip_pic p[MC_MAX_REFS]; };

// Host: the reference table of a launch from the caller's (refs, n_refs), 1 <= n_refs <= MC_MAX_REFS (anything else, or no table,
// is refused: OVHIP_EINVAL); unused entries repeat refs[0].  geom: the picture whose window geometry the kernel applies to every
// reference -- one of another size is RPR, outside such a kernel (OVHIP_EUNSUP); nullptr: every reference is read with its own
// geometry, and only a plane that is not there is refused (OVHIP_EINVAL).  `who`: the entry point's name, which leads the messages.
static inline int ref_table(ovhip_ctx *ctx, RefTable *t, const ovhip_pic *refs, uint32_t n_refs, const ovhip_pic *geom, const char *who)
{
    char what[96];
    if (!refs || !n_refs || n_refs > MC_MAX_REFS) {
        snprintf(what, sizeof(what), "%s: bad reference table", who);
        return ov_fail(ctx, OVHIP_EINVAL, what, hipSuccess);
    }
    memset(t, 0, sizeof(*t));
    for (uint32_t i = 0; i < n_refs; ++i) {
        const ovhip_pic &p = refs[i];
        if (geom ? p.w != geom->w || p.h != geom->h || p.stride_y != geom->stride_y || p.stride_c != geom->stride_c
                 : !p.y || !p.cb || !p.cr || p.w < 8 || p.h < 8 || p.stride_y < p.w || p.stride_c < (p.w >> 1)) {
            snprintf(what, sizeof(what), geom ? "%s: reference picture geometry differs (RPR)" : "%s: bad reference picture", who);
            return ov_fail(ctx, geom ? OVHIP_EUNSUP : OVHIP_EINVAL, what, hipSuccess);
        }
        t->p[i] = p;
    }
    for (uint32_t i = n_refs; i < MC_MAX_REFS; ++i) t->p[i] = refs[0];
    return OVHIP_OK;
}

typedef short short2v __attribute__((ext_vector_type(2)));

#define WIN_STRIDE 28   /* luma window row in LDS: 7 aligned qwords (<= 3 + 23 samples) = 56 B            */
#define CWIN_STRIDE 16  /* chroma window row: 4 aligned qwords (<= 3 + 11 samples) = 32 B                 */
#define LUMA_WIN (23 * WIN_STRIDE)
#define CHR_WIN  (11 * CWIN_STRIDE)
#define HT_STRIDE 28    /* transposed H-pass tile: one COLUMN per row of HT_STRIDE int16 (h + 7 <= 23), 8-B aligned rows */
#define CHT_STRIDE 12

// ---- stage 1: reference window -> LDS.  Every lane loads one ALIGNED 8-byte group of 4 samples -- QW lanes per
// window row, 64/QW rows per instruction: 3 instructions for a 23x23 luma window, 1 for an 11x11 chroma window --
// and parks it with one ds_write_b64; the sub-group offset `off` (0..3 samples) is resolved by the horizontal pass.
// Three ways to fill the registers, all equal to emulate_block_border() (rcn_inter.c:148-225) where it applies:
//   interior  window inside the picture: plain loads;
//   clamped   window crosses a border of a picture whose width and stride are multiples of 4 samples (every VVC
//             4:2:0 picture in buffers of this library): rows clamp per lane, and an aligned group lies either
//             wholly inside or wholly outside the picture, so an outside group is the nearest inside group's edge
//             sample replicated -- same loads as the interior path, no extra latency;
//   slow      any other geometry: per-sample loads with clamped coordinates, parked at off = 0. ----
template <int QW, int NIT, int COLS, int NITS>
struct WinStage {
    uint2 q[NIT];
    bool fast;
    int off, side;          // side: -1 / +1 = this lane's groups lie left / right of the picture

    // (bitwise on purpose: short-circuit && on wave-uniform values turns into scalar branches, and scalar issue is what
    // bounds k_mc2)
    static __device__ __forceinline__ int interior(int sx0, int sy0, int ww, int wh, int rw, int rh)
    {
        const int ax = sx0 & ~3, nq = (sx0 - ax + ww + 3) >> 2;
        return (int)(ax >= 0) & (int)(ax + 4 * nq <= rw) & (int)(sy0 >= 0) & (int)(sy0 + wh <= rh);
    }
    __device__ __forceinline__ void issue_fast(const uint16_t *__restrict__ ref, int rstride, int sx0, int sy0, int ww, int wh, int lane)
    {
        const int ax = sx0 & ~3;
        off = sx0 - ax; fast = true; side = 0;
        const int nq = (off + ww + 3) >> 2;
        const int c = lane & (QW - 1), r0 = lane / QW;
        const uint16_t *base = ref + ov_rowoff(sy0 + r0, rstride) + ax + 4 * c;
#pragma unroll
        for (int k = 0; k < NIT; ++k)
            if (c < nq && (64 / QW) * k + r0 < wh) q[k] = *reinterpret_cast<const uint2 *>(base + (64 / QW) * k * rstride);
    }
    __device__ __forceinline__ void issue_clamped(const uint16_t *__restrict__ ref, int rstride, int rw, int rh, int sx0, int sy0,
                                                  int ww, int wh, int lane)
    {
        const int ax = sx0 & ~3;
        off = sx0 - ax; fast = true;
        const int nq = (off + ww + 3) >> 2;
        const int c = lane & (QW - 1), r0 = lane / QW;
        const int qx = ax + 4 * c;
        side = qx < 0 ? -1 : qx >= rw ? 1 : 0;
        const uint16_t *base = ref + ov_clip3(qx, 0, rw - 4);
#pragma unroll
        for (int k = 0; k < NIT; ++k) {
            const int r = (64 / QW) * k + r0;
            if (c < nq && r < wh) q[k] = *reinterpret_cast<const uint2 *>(base + ov_rowoff(ov_clip3(sy0 + r, 0, rh - 1), rstride));
        }
    }
    __device__ __forceinline__ void issue_slow(const uint16_t *__restrict__ ref, int rstride, int rw, int rh, int sx0, int sy0,
                                               int ww, int wh, int lane, uint16_t *s_win, int winstride)
    {
        off = 0; fast = false; side = 0;
        const int c = lane & (COLS - 1), r0 = lane / COLS;
        const int sx = ov_clip3(sx0 + c, 0, rw - 1);
#pragma unroll 1
        for (int k = 0; k < NITS; ++k) {
            const int r = (64 / COLS) * k + r0;
            if (c < ww && r < wh) s_win[r * winstride + c] = ref[ov_clip3(sy0 + r, 0, rh - 1) * rstride + sx];
        }
    }
    template <bool FIX = true>
    __device__ __forceinline__ void park(uint16_t *s_win, int winstride, int ww, int wh, int lane) const
    {
        if (fast) {
            const int nq = (off + ww + 3) >> 2;
            const int c = lane & (QW - 1), r0 = lane / QW;
#pragma unroll
            for (int k = 0; k < NIT; ++k) {
                const int r = (64 / QW) * k + r0;
                if (c < nq && r < wh) {
                    uint2 v = q[k];
                    if (FIX && side) { const uint32_t e = (side < 0 ? v.x & 0xffffu : v.y >> 16) * 0x10001u; v.x = e; v.y = e; }
                    *reinterpret_cast<uint2 *>(s_win + r * winstride + 4 * c) = v;
                }
            }
        }
    }
};
typedef WinStage<8, 3, 32, 12> LumaStage;
typedef WinStage<4, 1, 16, 3> ChromaStage;

// All reference windows of one unit (<= 16x16 luma, both lists, Cb and Cr) -> LDS.  The path is chosen once per unit:
// every window interior -> all loads issued, then all parked; a border unit goes list by list (rolled, so that the
// rare path does not raise the kernel's register budget).  `geom` is the geometry shared by dst and every reference.
// lwin[l] / cwin[plane * 2 + l] are the LDS windows; offl / offc receive the sub-group offsets.
__device__ __forceinline__ void stage_unit_windows(const ovhip_pic &geom, const uint16_t *const ry[2], const uint16_t *const rcb[2],
                                                   const uint16_t *const rcr[2], const int lx[2], const int ly[2],
                                                   const int cx[2], const int cy[2], int w, int h, int dir, bool do_l, bool do_c,
                                                   int lane, uint16_t *const lwin[2], int lstride, uint16_t *const cwin[4], int cstride,
                                                   int offl[2], int offc[2])
{
    const int wc = w >> 1, hc = h >> 1, pw = geom.w, ph = geom.h, pwc = geom.w >> 1, phc = geom.h >> 1;
    const bool aligned = !((geom.stride_y | geom.stride_c | pw | pwc) & 3);
    int all_in = aligned;
#pragma unroll
    for (int l = 0; l < 2; ++l) {
        const int need_l = ((dir >> l) & 1) & (int)do_l, need_c = ((dir >> l) & 1) & (int)do_c;
        all_in &= (need_l ^ 1) | LumaStage::interior(lx[l], ly[l], w + 7, h + 7, pw, ph);
        all_in &= (need_c ^ 1) | ChromaStage::interior(cx[l], cy[l], wc + 3, hc + 3, pwc, phc);
    }
    const bool fast = all_in;
    offl[0] = offl[1] = offc[0] = offc[1] = 0;
    if (fast) {
        LumaStage sl[2];
        ChromaStage sc[2][2];
#pragma unroll
        for (int l = 0; l < 2; ++l) {
            if (!(dir & (1 << l))) continue;
            if (do_l) sl[l].issue_fast(ry[l], geom.stride_y, lx[l], ly[l], w + 7, h + 7, lane);
            if (do_c) {
                sc[0][l].issue_fast(rcb[l], geom.stride_c, cx[l], cy[l], wc + 3, hc + 3, lane);
                sc[1][l].issue_fast(rcr[l], geom.stride_c, cx[l], cy[l], wc + 3, hc + 3, lane);
            }
        }
#pragma unroll
        for (int l = 0; l < 2; ++l) {
            if (!(dir & (1 << l))) continue;
            if (do_l) { sl[l].park<false>(lwin[l], lstride, w + 7, h + 7, lane); offl[l] = sl[l].off; }
            if (do_c) {
                sc[0][l].park<false>(cwin[l], cstride, wc + 3, hc + 3, lane);
                sc[1][l].park<false>(cwin[2 + l], cstride, wc + 3, hc + 3, lane);
                offc[l] = sc[0][l].off;
            }
        }
        return;
    }
#pragma unroll 1
    for (int l = 0; l < 2; ++l) {
        if (!(dir & (1 << l))) continue;
        const uint16_t *y = l ? ry[1] : ry[0], *cb = l ? rcb[1] : rcb[0], *cr = l ? rcr[1] : rcr[0];
        const int x0 = l ? lx[1] : lx[0], y0 = l ? ly[1] : ly[0], xc = l ? cx[1] : cx[0], yc = l ? cy[1] : cy[0];
        uint16_t *wl = l ? lwin[1] : lwin[0], *wb = l ? cwin[1] : cwin[0], *wr = l ? cwin[3] : cwin[2];
        LumaStage a;
        ChromaStage b0, b1;
        a.off = b0.off = 0;
        if (aligned) {
            if (do_l) a.issue_clamped(y, geom.stride_y, pw, ph, x0, y0, w + 7, h + 7, lane);
            if (do_c) {
                b0.issue_clamped(cb, geom.stride_c, pwc, phc, xc, yc, wc + 3, hc + 3, lane);
                b1.issue_clamped(cr, geom.stride_c, pwc, phc, xc, yc, wc + 3, hc + 3, lane);
            }
            if (do_l) a.park<true>(wl, lstride, w + 7, h + 7, lane);
            if (do_c) { b0.park<true>(wb, cstride, wc + 3, hc + 3, lane); b1.park<true>(wr, cstride, wc + 3, hc + 3, lane); }
        } else {
            if (do_l) a.issue_slow(y, geom.stride_y, pw, ph, x0, y0, w + 7, h + 7, lane, wl, lstride);
            if (do_c) {
                b0.issue_slow(cb, geom.stride_c, pwc, phc, xc, yc, wc + 3, hc + 3, lane, wb, cstride);
                b1.issue_slow(cr, geom.stride_c, pwc, phc, xc, yc, wc + 3, hc + 3, lane, wr, cstride);
            }
        }
        if (l) { offl[1] = do_l ? a.off : 0; offc[1] = do_c ? b0.off : 0; }
        else   { offl[0] = do_l ? a.off : 0; offc[0] = do_c ? b0.off : 0; }
    }
}

// ---- 4 outputs of an NT-tap FIR over a packed int16 row: out[o] = sum_k taps[k] * s[o + k].
// d[j] = (s[2j], s[2j+1]); even outputs use the dwords as they are, odd outputs the dwords shifted by
// one sample (v_alignbit); every dword pair is one v_dot2c_i32_i16 (2 MACs). ----
template <int NT>
__device__ __forceinline__ void fir4(const int d[NT / 2 + 2], const int tp[NT / 2], int out[4])
{
    int e[NT / 2 + 1];
#pragma unroll
    for (int j = 0; j < NT / 2 + 1; ++j) e[j] = (int)__builtin_amdgcn_alignbit((uint32_t)d[j + 1], (uint32_t)d[j], 16);
#pragma unroll
    for (int o = 0; o < 4; ++o) {
        int acc = 0;
#pragma unroll
        for (int m = 0; m < NT / 2; ++m) {
            const int v = (o & 1) ? e[(o >> 1) + m] : d[(o >> 1) + m];
            acc = __builtin_amdgcn_sdot2(__builtin_bit_cast(short2v, v), __builtin_bit_cast(short2v, tp[m]), acc, false);
        }
        out[o] = acc;
    }
}

// Filter taps as pairs ((f[2m], f[2m+1]) = int16 halves of one dword, what v_dot2_i32_i16 multiplies), packed at COMPILE time:
// a wave-uniform filter is then one scalar load instead of 8 byte loads, 8 sign extensions and 12 shift / or (the tap
// set-up was a fifth of k_mc2's scalar instructions).  luma6 = the 6 taps 1..6 of the 4x4-block luma filter.
struct PackedTaps { uint32_t luma[17][4], luma4[16][4], luma6[16][4], chroma[32][2]; };
constexpr uint32_t pack_pair(int a, int b) { return ((uint32_t)a & 0xffffu) | ((uint32_t)b << 16); }
constexpr PackedTaps build_packed_taps()
{
    PackedTaps t{};
    for (int f = 0; f < 17; ++f)
        for (int m = 0; m < 4; ++m) t.luma[f][m] = pack_pair(ovt_mc_luma[f][2 * m], ovt_mc_luma[f][2 * m + 1]);
    for (int f = 0; f < 16; ++f)
        for (int m = 0; m < 4; ++m) {
            t.luma4[f][m] = pack_pair(ovt_mc_luma4[f][2 * m], ovt_mc_luma4[f][2 * m + 1]);
            t.luma6[f][m] = m < 3 ? pack_pair(ovt_mc_luma4[f][2 * m + 1], ovt_mc_luma4[f][2 * m + 2]) : 0u;
        }
    for (int f = 0; f < 32; ++f)
        for (int m = 0; m < 2; ++m) t.chroma[f][m] = pack_pair(ovt_mc_chroma[f][2 * m], ovt_mc_chroma[f][2 * m + 1]);
    return t;
}
__device__ const PackedTaps __attribute__((aligned(16))) g_taps = build_packed_taps();

template <int ND>
__device__ __forceinline__ void load_taps(const uint32_t *row, int tp[ND])
{
#pragma unroll
    for (int m = 0; m < ND; ++m) tp[m] = (int)row[m];
}

template <int NT>
__device__ __forceinline__ void load_row(const void *p, int d[NT / 2 + 2])
{
    // segment starts are 8-byte aligned in LDS (strides are multiples of 4 samples)
    const int2 *q = reinterpret_cast<const int2 *>(p);
#pragma unroll
    for (int j = 0; j < (NT / 2 + 2) / 2; ++j) { const int2 v = q[j]; d[2 * j] = v.x; d[2 * j + 1] = v.y; }
}

// same, starting at an arbitrary SAMPLE index s0 of a dword-aligned row (window rows keep their
// aligned-group offset): dword loads + one v_alignbit per dword when s0 is odd
template <int NT>
__device__ __forceinline__ void load_row_at(const uint16_t *row, int s0, int d[NT / 2 + 2])
{
    const int *q = reinterpret_cast<const int *>(row) + (s0 >> 1);
    int D[NT / 2 + 2];
#pragma unroll
    for (int j = 0; j < NT / 2 + 2; ++j) D[j] = q[j];
    if (s0 & 1) {
#pragma unroll
        for (int j = 0; j < NT / 2 + 1; ++j) d[j] = (int)__builtin_amdgcn_alignbit((uint32_t)D[j + 1], (uint32_t)D[j], 16);
        d[NT / 2 + 1] = (int)((uint32_t)D[NT / 2 + 1] >> 16);
    } else {
#pragma unroll
        for (int j = 0; j < NT / 2 + 2; ++j) d[j] = D[j];
    }
}

// ---- stage 3: vertical pass LDS -> registers.  Lane = one column x 4 consecutive rows (group g):
// P[j] = F_v(t)[x][4g + j] >> 6, the 14-bit intermediate of put_vvc_{qpel,epel}_*. ----
template <int NT>
__device__ __forceinline__ void v_pass(const int16_t *s_ht, int htstride, int log2w, int h, const uint32_t *fv_packed, int lane, int P[4])
{
    int tp[NT / 2];
    load_taps<NT / 2>(fv_packed, tp);
    const int w = 1 << log2w;
    const int ngrp = (h + 3) >> 2;
    if (lane < (ngrp << log2w)) {
        const int x = lane & (w - 1), g = lane >> log2w;
        int d[NT / 2 + 2];
        load_row<NT>(s_ht + x * htstride + 4 * g, d);
        fir4<NT>(d, tp, P);
#pragma unroll
        for (int o = 0; o < 4; ++o) P[o] >>= 6;
    }
}



// ---- NOUT (1, 2 or 4) outputs of an NT-tap FIR over packed int16 dwords d[0 .. (NT + NOUT) / 2] (see fir4) ----
template <int NT, int NOUT>
__device__ __forceinline__ void firn(const int *d, const int tp[NT / 2], int out[NOUT])
{
#pragma unroll
    for (int o = 0; o < NOUT; ++o) {
        int acc = 0;
#pragma unroll
        for (int m = 0; m < NT / 2; ++m) {
            const int j = (o >> 1) + m;
            const int v = (o & 1) ? (int)__builtin_amdgcn_alignbit((uint32_t)d[j + 1], (uint32_t)d[j], 16) : d[j];
            acc = __builtin_amdgcn_sdot2(__builtin_bit_cast(short2v, v), __builtin_bit_cast(short2v, tp[m]), acc, false);
        }
        out[o] = acc;
    }
}

// NT + NOUT - 1 samples starting at SAMPLE index s0 of a dword-aligned row, as packed dwords (last one may be half used)
template <int NT, int NOUT>
__device__ __forceinline__ void load_span(const int16_t *row, int s0, int d[(NT + NOUT) / 2])
{
    constexpr int ND = (NT + NOUT) / 2;                // dwords covering NT + NOUT - 1 samples from an even start
    const int *q = reinterpret_cast<const int *>(row) + (s0 >> 1);
    int D[ND + 1];
#pragma unroll
    for (int j = 0; j < ND + 1; ++j) D[j] = q[j];
    if (s0 & 1) {
#pragma unroll
        for (int j = 0; j < ND; ++j) d[j] = (int)__builtin_amdgcn_alignbit((uint32_t)D[j + 1], (uint32_t)D[j], 16);
    } else {
#pragma unroll
        for (int j = 0; j < ND; ++j) d[j] = D[j];
    }
}


// ---- merged-pass building blocks (k_mc2, k_mcx): one horizontal task = one window row x 4 outputs; one
// vertical call = NOUT consecutive outputs of one transposed-tile column ----
template <int NT>
__device__ __forceinline__ void h_task(const uint16_t *wrow, int off, int x0, const int tp[NT / 2], bool ident, int16_t *ht,
                                       int htstride, int r)
{
    int d[NT / 2 + 2], out[4];
    if (ident) {
        const uint16_t *sp = wrow + off + x0 + NT / 2 - 1;
#pragma unroll
        for (int o = 0; o < 4; ++o) out[o] = (int)sp[o] << 6;
    } else {
        load_row_at<NT>(wrow, off + x0, d);
        fir4<NT>(d, tp, out);
    }
#pragma unroll
    for (int o = 0; o < 4; ++o)
        ht[(x0 + o) * htstride + r] = (int16_t)(out[o] >> (OV_BD - 8));      // a 2-wide chroma block also fills columns 2, 3: never read
}

template <int NT, int NOUT>
__device__ __forceinline__ void v_outputs(const int16_t *col, int s0, const int tp[NT / 2], int P[NOUT])
{
    int d[(NT + NOUT) / 2];
    load_span<NT, NOUT>(col, s0, d);
    firn<NT, NOUT>(d, tp, P);
#pragma unroll
    for (int o = 0; o < NOUT; ++o) P[o] >>= 6;
}

// The horizontal pass of ONE window by the 2^l2per lanes dealt to it (tl = the lane's index among them): one task = one window
// row x 4 outputs, so that everything a task needs except its row -- taps, alignment, tile -- is fixed per lane and leaves the
// loop.  win / winstride / off: the window, its row stride and sub-group offset; rows: its height; log2seg: log2 of the plane
// width in 4-sample segments, the caller's to clamp at 0 (k_mcx's luma is >= 8 wide and passes log2w - 2 as it is).
// (k_mc2 spells the same two loops out: through this function the compiler orders the set-up in front of its loops differently --
// same instructions, other schedule and registers -- and that kernel's instruction text is kept fixed.)
template <int NT>
__device__ __forceinline__ void h_pass(const uint16_t *win, int winstride, int off, int rows, int log2seg, int l2per, int tl,
                                       const int tp[NT / 2], bool ident, int16_t *ht, int htstride)
{
    const int x0 = (tl & ((1 << log2seg) - 1)) << 2, rstep = (1 << l2per) >> log2seg;
    for (int r = tl >> log2seg; r < rows; r += rstep) h_task<NT>(win + r * winstride, off, x0, tp, ident, ht, htstride, r);
}

// ---- the lists' 14-bit intermediates -> one sample.  24-bit multiplies throughout (v_mad_i32_i24 is full rate where
// v_mul_lo_u32 is not); every operand fits: the intermediates are int16 (PROF's refinement included; the scaled filters' stay
// below 2^19), the BCW weights lie in {-2, 3, 4, 5, 10}, the GPM slopes are int8 and its coordinates unit-relative (<= 30), the
// intra samples and CIIP weights are 10 and 2 bits. ----
// uni (p + 8) >> 4, bi average (p0 + p1 + 16) >> 5, BCW (p1 w1 + p0 w0 + 64) >> 7 (put_vvc_uni/bi(_w)_*): one weighted form whose
// constants are chosen ONCE per unit (k_mca: per block) -- per-sample three-way branches on wave-uniform unit fields cost scalar
// issue slots, which is what bounds k_mc2.  M: anything with dir, w0 and w1 -- a unit, or a BiMode where the direction is the
// block's and not the unit's (k_mca, k_mca_rpr: a block whose lists are identical is predicted from list 1 alone)
struct Combine { int a0, a1, rnd, sh; };
struct BiMode { int dir, w0, w1; };
template <class M>
__device__ __forceinline__ Combine mc_combine_of(const M &u)
{
    Combine c;
    if (u.dir != 3)                 { c.a0 = u.dir == 1; c.a1 = u.dir != 1; c.rnd = 8; c.sh = 4; }
    else if (u.w0 == 4 && u.w1 == 4) { c.a0 = 1; c.a1 = 1; c.rnd = 16; c.sh = 5; }
    else                            { c.a0 = u.w0; c.a1 = u.w1; c.rnd = 64; c.sh = 7; }
    return c;
}
__device__ __forceinline__ int mc_combine(const Combine &c, int p0, int p1) { return ov_clip_bd((__mul24(p1, c.a1) + __mul24(p0, c.a0) + c.rnd) >> c.sh); }

// geometric partitioning: w = clip3(0, 8, (K + A*x + B*y) >> 3), put_weighted_gpm_bi_pixels (rcn_mc.c:1630-1655)
__device__ __forceinline__ int mc_gpm(uint32_t aux, int x, int y, int p0, int p1)
{
    const int k = (int16_t)(aux & 0xffff), a = (int8_t)((aux >> 16) & 0xff), b = (int8_t)(aux >> 24);
    const int wgt = ov_clip3((k + __mul24(a, x) + __mul24(b, y)) >> 3, 0, 8);
    return ov_clip_bd((__mul24(p1, 8 - wgt) + __mul24(p0, wgt) + 64) >> 7);
}

// fused CIIP blend: (intra * wt + inter * (4 - wt) + 2) >> 2, put_weighted_ciip_pixels (rcn_mc.c:1611-1628)
__device__ __forceinline__ int ciip_blend(int inter, int intra, int wt) { return ov_clip_bd((__mul24(intra, wt) + __mul24(inter, 4 - wt) + 2) >> 2); }

// ---- chroma vertical pass + combine + store of one unit: both planes in one pass, NOUT rows per lane so that the lanes cover
// both.  s_hc: the transposed H tiles [plane * 2 + list][8 * CHT_STRIDE].  AVG (k_mcx: refined units are plain bi-predicted):
// both lists, the average, and no GPM or CIIP code in the instantiation -- `intra` is then never read. ----
template <int NOUT, bool AVG = false>
__device__ __forceinline__ void chroma_finish(const ovhip_mc_unit &u, const ovhip_pic &dst, const int16_t *s_hc, const int tv[2][2],
                                              int lane, int log2wc, int hc, const ovhip_pic &intra)
{
    const int wc = 1 << log2wc;
    const int per_plane = (wc * hc) / NOUT;                   // lanes per plane (power of two, <= 32)
    const int plane = lane >= per_plane, ll = lane - plane * per_plane;
    if (lane >= 2 * per_plane) return;
    const int x = ll & (wc - 1), y0 = (ll >> log2wc) * NOUT;
    int P[2][NOUT];
#pragma unroll
    for (int l = 0; l < 2; ++l) {
#pragma unroll
        for (int o = 0; o < NOUT; ++o) P[l][o] = 0;
        if (AVG || (u.dir & (1 << l))) v_outputs<4, NOUT>(s_hc + (plane * 2 + l) * 8 * CHT_STRIDE + x * CHT_STRIDE, y0, tv[l], P[l]);
    }
    uint16_t *d = (plane ? dst.cr : dst.cb) + ov_rowoff((u.y >> 1) + y0, dst.stride_c) + (u.x >> 1) + x;
    const bool ciip = !AVG && !(u.flags & OVHIP_MC_GPM) && u.aux && !(u.aux & 0x100);
    const uint16_t *ip = ciip ? (plane ? intra.cr : intra.cb) + ov_rowoff((u.y >> 1) + y0, intra.stride_c) + (u.x >> 1) + x : nullptr;
    int v[NOUT];
    if (!AVG && (u.flags & OVHIP_MC_GPM)) {
#pragma unroll
        for (int j = 0; j < NOUT; ++j) v[j] = mc_gpm(u.aux, 2 * x, 2 * (y0 + j), P[0][j], P[1][j]);
    } else {
        const Combine cmb = AVG ? Combine{ 1, 1, 16, 5 } : mc_combine_of(u);
#pragma unroll
        for (int j = 0; j < NOUT; ++j) v[j] = mc_combine(cmb, P[0][j], P[1][j]);
    }
    if (ciip) {
#pragma unroll
        for (int j = 0; j < NOUT; ++j) v[j] = ciip_blend(v[j], ip[j * intra.stride_c], u.aux & 7);
    }
#pragma unroll
    for (int j = 0; j < NOUT; ++j) d[j * dst.stride_c] = (uint16_t)v[j];
}

// ---- PROF of one 4x4 block and list on a 6x6 int16 tile (extend_prof_buff / compute_prof_grad / rcn_prof,
// rcn_prof_bdof.c:152-290): interior = the prediction, ring = integer reference samples << 4.  Lane c of the block's 4 owns
// column c of the interior and the ring samples 5c .. 5c + 4. ----
// ring sample e (0 .. 19) -> column i, row j of the tile: top row, bottom row, left column, right column
__device__ __forceinline__ void prof_ring(int e, int &i, int &j)
{
    if (e < 6)       { i = e; j = 0; }
    else if (e < 12) { i = e - 6; j = 5; }
    else if (e < 16) { i = 0; j = e - 11; }
    else             { i = 5; j = e - 15; }
}
// fill: the lane's share of the tile; ring(i, j) = the reference sample under tile position (i, j)
template <class Ring>
__device__ __forceinline__ void prof_fill(int16_t *t, int c, const int P[4], Ring ring)
{
#pragma unroll
    for (int j = 0; j < 4; ++j) t[(j + 1) * 6 + c + 1] = (int16_t)P[j];
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        int i, j;
        prof_ring(5 * c + k, i, j);
        t[j * 6 + i] = (int16_t)(ring(i, j) << 4);
    }
}
// refine (after a barrier): gradients of the lane's 4 samples, P += clip(dx gx + dy gy); dx / dy: the lane's offsets (int16)
__device__ __forceinline__ void prof_refine(const int16_t *t, int c, const int dx[4], const int dy[4], int P[4])
{
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int o = (j + 1) * 6 + c + 1;
        const int gx = (t[o + 1] >> 6) - (t[o - 1] >> 6), gy = (t[o + 6] >> 6) - (t[o - 6] >> 6);
        const int add = ov_clip3(__mul24(dx[j], gx) + __mul24(dy[j], gy), -(1 << 13), (1 << 13) - 1);
        P[j] = (int)(int16_t)(P[j] + add);
    }
}

// ---- reference window of one 4x4 affine block and list (ROWS x ROWS samples: luma 9, chroma 7) -> LDS rows of AFF_WS samples,
// by the block's 4 lanes (c = 0 .. 3, one aligned group of 4 samples each).  Split into issue (loads into registers) and park
// (registers -> LDS, returns the sub-group offset) so that a window can fly while another is being filtered.  Aligned geometry
// takes WinStage's clamped loads, inside the picture and at its borders alike; any other geometry is fetched sample by sample
// with clamped coordinates at park time, at offset 0. ----
#define AFF_WS 12
template <int ROWS>
struct AffStage {
    uint2 q[ROWS];
    const uint16_t *ref;
    int sx0, sy0, off, side;
    bool fast;

    __device__ __forceinline__ void issue(const uint16_t *__restrict__ r, int rstride, int rw, int rh, int x0, int y0, int c)
    {
        ref = r; sx0 = x0; sy0 = y0;
        const int ax = sx0 & ~3;
        off = sx0 - ax;
        const int nq = (off + ROWS + 3) >> 2;
        fast = !((rstride | rw) & 3);
        if (fast && c < nq) {
            // rows clamp per lane; an aligned group outside the picture = the edge sample replicated (see WinStage)
            const int qx = ax + 4 * c;
            side = qx < 0 ? -1 : qx >= rw ? 1 : 0;
            const uint16_t *base = ref + ov_clip3(qx, 0, rw - 4);
#pragma unroll
            for (int k = 0; k < ROWS; ++k) q[k] = *reinterpret_cast<const uint2 *>(base + ov_rowoff(ov_clip3(sy0 + k, 0, rh - 1), rstride));
        }
    }
    __device__ __forceinline__ int park(int rstride, int rw, int rh, int c, uint16_t *win)
    {
        if (fast) {
            if (c < ((off + ROWS + 3) >> 2)) {
#pragma unroll
                for (int k = 0; k < ROWS; ++k) {
                    uint2 v = q[k];
                    if (side) { const uint32_t e = (side < 0 ? v.x & 0xffffu : v.y >> 16) * 0x10001u; v.x = e; v.y = e; }
                    *reinterpret_cast<uint2 *>(win + k * AFF_WS + 4 * c) = v;
                }
            }
            return off;
        }
        for (int i = c; i < ROWS; i += 4) {
            const int sx = ov_clip3(sx0 + i, 0, rw - 1);
#pragma unroll 1
            for (int k = 0; k < ROWS; ++k) win[k * AFF_WS + i] = ref[ov_clip3(sy0 + k, 0, rh - 1) * rstride + sx];
        }
        return 0;
    }
};

} // namespace
