"""Test infrastructure: a numpy restatement of how the reference predicts an AFFINE coding unit of which at least one
used list reads a scaled reference (reference picture resampling), built on spec_rpr's anchor and filter functions.

The affine drivers (drv_affine_mvp.c:3264-3411) hand every 4x4 luma sub-block to rcn_mcp_b_l(2,2) or rcn_prof_mcp_b_l and
every 8x8 luma area's chroma to rcn_mcp_b_c(3,3) (libovvc/rcn_inter.c:2815-2966):
  * each sub-block is a 4x4 PU of its own: its own ref_pos / ref_pu_w/h / clip_rpr_position, flag_4x4 set, so the luma
    filter sets are 3..5; the chroma of an 8x8 area is a 4x4 chroma block with sets 0..2 (log2 = 3: flag_4x4 false);
  * rcn_mcp_b_l / rcn_mcp_b_c turn a bi block with identical motion into a uni block from list 1, rcn_prof_mcp_b_l does not;
  * the unscaled side of a mixed bi block is rcn_mcp_bidir0_l, which for a 4x4 block runs the 6-tap filters
    (put_vvc_qpel_* pick ov_mc_filters_4 when width == height == 4, rcn_mc.c:457); with PROF (apply_prof, :2880) it is
    rcn_prof_mcp_bi_l: the same prediction refined by extend_prof_buff / compute_prof_grad / rcn_prof
    (rcn_prof_bdof.c:152-290); a scaled side is never refined, a uni block on a scaled list is plain rcn_mcp_rpr_l;
  * put_vvc_pel_rpr_clip's uint16 quirk needs filter set 0, so it only reaches the chroma.
Reference pictures are read with coordinates clamped to their own size (= emulate_block_border)."""
import numpy as np

import spec_rpr
from spec_rpr import BCW, MC_CHROMA, RPR_CHROMA, RPR_LUMA, UNSCALED, anchor, clip_mv, filter_idx, regular_bi_plane, scaled_plane

MC_LUMA4 = spec_rpr._table("vvc_mc_taps.h", "ovt_mc_luma4", (16, 8))


def _scale_of(scales, slot, pic_w, pic_h):
    return scales.get(slot, dict(scale_hor=UNSCALED, scale_ver=UNSCALED, ref_w=pic_w, ref_h=pic_h, col_hor=0, col_ver=0))


def _is_scaled(s):
    return s["scale_hor"] != UNSCALED or s["scale_ver"] != UNSCALED


def luma_words(s, x, y, mvx, mvy, pic_w, pic_h):
    """What the recorder keeps per sub-block and list: the clipped anchor pair (scaled) or the clip_mv()'d vector."""
    if not _is_scaled(s):
        return clip_mv(x, y, 4, 4, pic_w, pic_h, mvx, mvy)
    ax, _ = anchor(x, mvx, s["scale_hor"], 0, 4, s["ref_w"], 4, False)
    ay, _ = anchor(y, mvy, s["scale_ver"], 0, 4, s["ref_h"], 4, True)
    return ax, ay


def chroma_words(s, x, y, mvx, mvy, pic_w, pic_h):
    """The same for the chroma block of the 8x8 luma area at (x, y) with the averaged vector."""
    if not _is_scaled(s):
        return clip_mv(x, y, 8, 8, pic_w, pic_h, mvx, mvy)
    add_x = (1 - s["col_hor"]) * 8 * (s["scale_hor"] - UNSCALED)
    add_y = (1 - s["col_ver"]) * 8 * (s["scale_ver"] - UNSCALED)
    cx, _ = anchor(x >> 1, mvx, s["scale_hor"], add_x, 4, s["ref_w"] >> 1, 5, False)
    cy, _ = anchor(y >> 1, mvy, s["scale_ver"], add_y, 4, s["ref_h"] >> 1, 5, True)
    return cx, cy


def steps_and_sets(s):
    """(step_x, step_y, luma sets h | v << 4, chroma sets h | v << 4) of a scaled list."""
    return (((s["scale_hor"] + 8) >> 4) << 4, ((s["scale_ver"] + 8) >> 4) << 4,
            filter_idx(s["scale_hor"], True) | filter_idx(s["scale_ver"], True) << 4,
            filter_idx(s["scale_hor"], False) | filter_idx(s["scale_ver"], False) << 4)


def avg_mv(a, b):
    """Rounded average of the top-left and bottom-right sub-block vectors of an 8x8 area (drv_affine_mvp.c:3371-3411)."""
    out = []
    for p, q in zip(a, b):
        m = int(p) + int(q)
        m += m < 0
        out.append(m >> 1)
    return out


def prof_refine(pred, plane, rx, ry, ex, ey, dmv_h, dmv_v):
    """extend_prof_buff / compute_prof_grad / rcn_prof (bi form): pred = the 4x4 14-bit prediction, (rx, ry) the integer
    reference position of its top-left sample, ex / ey = (phase >> 3).  Returns the refined 14-bit block (int16 wrap)."""
    t = np.zeros((6, 6), dtype=np.int64)
    t[1:5, 1:5] = pred
    h, w = plane.shape
    for j in range(6):
        for i in range(6):
            if 1 <= i <= 4 and 1 <= j <= 4:
                continue
            yy = min(max(ry - 1 + ey + j, 0), h - 1)
            xx = min(max(rx - 1 + ex + i, 0), w - 1)
            t[j, i] = int(plane[yy, xx]) << 4
    out = np.zeros((4, 4), dtype=np.int64)
    for y in range(4):
        for x in range(4):
            gy = ((t[y + 2, x + 1] - 8192) >> 6) - ((t[y, x + 1] - 8192) >> 6)
            gx = ((t[y + 1, x + 2] - 8192) >> 6) - ((t[y + 1, x] - 8192) >> 6)
            add = int(dmv_h[4 * y + x]) * int(gx) + int(dmv_v[4 * y + x]) * int(gy)
            add = min(max(add, -8192), 8191)
            out[y, x] = ((int(pred[y, x]) + add + 32768) % 65536) - 32768          # int16_t val = src[x] + add
    return out


def _combine(bcw_idx_plus1):
    if bcw_idx_plus1 in (0, 3):
        return lambda a, c: np.clip((a + c + 16) >> 5, 0, 1023)
    w1 = BCW[bcw_idx_plus1 - 1]
    return lambda a, c: np.clip((a * (8 - w1) + c * w1 + 64) >> 7, 0, 1023)


def predict_affine_cu(refs, scales, pic_w, pic_h, cu, lmcs_lut=None):
    """refs: slot -> (Y, Cb, Cr) planes of the reference's own size; scales as in spec_rpr.predict_pu.  cu: dict with x0, y0,
    log2_w, log2_h, inter_dir, ref0, ref1, poc0, poc1, bcw_idx_plus1, prof_dir, lmcs, mv0 / mv1 ([ny][nx][2] per 4x4
    sub-block), dmv_scale ([4][16]: h0, v0, h1, v1).  Returns (Y, Cb, Cr) of the CU as the three affine drivers leave them."""
    x0, y0, cw, ch = cu["x0"], cu["y0"], 1 << cu["log2_w"], 1 << cu["log2_h"]
    dir_cu = cu["inter_dir"] & 3
    if dir_cu != 3 and dir_cu & 2:
        dir_cu = 2
    slots = (cu["ref0"], cu["ref1"])
    sc = [_scale_of(scales, slots[l], pic_w, pic_h) for l in (0, 1)]
    scaled = [_is_scaled(sc[l]) for l in (0, 1)]
    if not any(scaled[l] for l in (0, 1) if dir_cu & (1 << l)):
        raise ValueError("no scaled list: not a reference-picture-resampling CU")
    mv = (np.asarray(cu["mv0"], dtype=np.int64), np.asarray(cu["mv1"], dtype=np.int64))
    prof_dir = cu.get("prof_dir", 0)
    dmv = np.asarray(cu.get("dmv_scale", np.zeros((4, 16))), dtype=np.int64)
    comb = _combine(cu.get("bcw_idx_plus1", 0))
    same_poc = cu["poc0"] == cu["poc1"]
    Y = np.zeros((ch, cw), dtype=np.int64)
    C = [np.zeros((ch >> 1, cw >> 1), dtype=np.int64) for _ in range(2)]

    def luma_side(l, x, y, m, bi, prof):
        s = sc[l]
        plane = refs[slots[l]][0]
        if scaled[l]:
            ax, ay = luma_words(s, x, y, int(m[0]), int(m[1]), pic_w, pic_h)
            stx, sty, filt, _ = steps_and_sets(s)
            return scaled_plane(plane, ax, ay, stx, sty, filt & 15, filt >> 4, 4, 4, 4, RPR_LUMA, bi)
        mx, my = clip_mv(x, y, 4, 4, pic_w, pic_h, int(m[0]), int(m[1]))
        p = regular_bi_plane(plane, x, y, 4, 4, mx, my, 4, MC_LUMA4)
        if prof:
            p = prof_refine(p, plane, x + (mx >> 4), y + (my >> 4), (mx & 15) >> 3, (my & 15) >> 3, dmv[2 * l], dmv[2 * l + 1])
        return p if bi else np.clip((p + 8) >> 4, 0, 1023)          # rcn_mcp_l

    for sy in range(ch >> 2):
        for sx in range(cw >> 2):
            x, y = x0 + 4 * sx, y0 + 4 * sy
            m = (mv[0][sy, sx], mv[1][sy, sx])
            d = dir_cu
            if not prof_dir and d == 3 and same_poc and m[0][0] == m[1][0] and m[0][1] == m[1][1]:
                d = 2
            if d == 3:
                p0 = luma_side(0, x, y, m[0], True, bool(prof_dir & 1))
                p1 = luma_side(1, x, y, m[1], True, bool(prof_dir & 2))
                blk = comb(p0, p1)
            else:
                blk = luma_side(d - 1, x, y, m[d - 1], False, False)
            Y[4 * sy:4 * sy + 4, 4 * sx:4 * sx + 4] = blk

    def chroma_side(l, comp, x, y, m, bi):
        s = sc[l]
        plane = refs[slots[l]][1 + comp]
        if scaled[l]:
            cx, cy = chroma_words(s, x, y, m[0], m[1], pic_w, pic_h)
            stx, sty, _, filt_c = steps_and_sets(s)
            return scaled_plane(plane, cx, cy, stx, sty, filt_c & 15, filt_c >> 4, 4, 4, 5, RPR_CHROMA, bi)
        mx, my = clip_mv(x, y, 8, 8, pic_w, pic_h, m[0], m[1])
        p = regular_bi_plane(plane, x >> 1, y >> 1, 4, 4, mx, my, 5, MC_CHROMA)
        return p if bi else np.clip((p + 8) >> 4, 0, 1023)          # rcn_mcp_c

    for by in range(ch >> 3):
        for bx in range(cw >> 3):
            x, y = x0 + 8 * bx, y0 + 8 * by
            m = [avg_mv(mv[l][2 * by, 2 * bx], mv[l][2 * by + 1, 2 * bx + 1]) if dir_cu & (1 << l) else [0, 0] for l in (0, 1)]
            d = dir_cu
            if d == 3 and same_poc and m[0] == m[1]:
                d = 2
            for comp in range(2):
                if d == 3:
                    blk = comb(chroma_side(0, comp, x, y, m[0], True), chroma_side(1, comp, x, y, m[1], True))
                else:
                    blk = chroma_side(d - 1, comp, x, y, m[d - 1], False)
                C[comp][4 * by:4 * by + 4, 4 * bx:4 * bx + 4] = blk

    if cu.get("lmcs") and lmcs_lut is not None:
        Y = np.asarray(lmcs_lut, dtype=np.int64)[Y]
    return Y.astype(np.uint16), C[0].astype(np.uint16), C[1].astype(np.uint16)
