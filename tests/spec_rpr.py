"""Test infrastructure: a numpy restatement of the reference's prediction from scaled references (reference picture
resampling), written PU by PU as the reference runs it -- rcn_mcp_rpr_l / _bi_l / _c / _bi_c, rcn_mc_rpr_b_l / _c and
rcn_mcp_bidir0_l / _c for the unscaled side of a mixed bi-prediction (libovvc/rcn_inter.c:1557-1660, :1991-2736) -- with
the reference's quirks:
  * put_vvc_pel_rpr_clip reads the horizontal intermediate as uint16 (uni-prediction, vertical phase 0, filter set 0);
  * ref_pos is int32 arithmetic and wraps (restated with explicit 32-bit wrapping);
  * the chroma collocation flags come from the reference picture's scale info.
Reference pictures are read with coordinates clamped to their own size (= emulate_block_border)."""
import re
from pathlib import Path

import numpy as np

CSRC = Path(__file__).resolve().parent.parent / "openvvc_amd" / "csrc"
UNSCALED = 1 << 14


def _table(header: str, name: str, shape):
    txt = (CSRC / header).read_text()
    m = re.search(name + r"\[[^=]*=\s*\{(.*?)\};", txt, re.S)
    vals = [int(v) for v in re.findall(r"-?\d+", re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S))]
    return np.array(vals, dtype=np.int64).reshape(shape)


RPR_LUMA = _table("vvc_rpr_taps.h", "ovt_rpr_luma", (6, 16, 8))
RPR_CHROMA = _table("vvc_rpr_taps.h", "ovt_rpr_chroma", (3, 32, 4))
MC_LUMA = _table("vvc_mc_taps.h", "ovt_mc_luma", (17, 8))
MC_CHROMA = _table("vvc_mc_taps.h", "ovt_mc_chroma", (32, 4))
BCW = [-2, 3, 4, 5, 10]


def i32(v: int) -> int:
    v &= 0xFFFFFFFF
    return v - (1 << 32) if v >= (1 << 31) else v


def filter_idx(scale: int, flag_4x4: bool) -> int:
    idx = 3 if flag_4x4 else 0
    if scale > UNSCALED * 7 // 4:
        idx += 2
    elif scale > UNSCALED * 5 // 4:
        idx += 1
    return idx


def anchor(pos, mv, scale, add, pu_len, pic_len, shift_mv, min1):
    """ref_pos of one axis after clip_rpr_position, and the rounded step."""
    sp = 14 + shift_mv
    step = ((scale + 8) >> 4) << 4
    ref_pos = i32(((pos << shift_mv) + mv) * scale + add + (1 << (shift_mv + 3)))
    ref_i = i32(ref_pos + 8192) >> sp
    ext = (i32(ref_pos + (((pu_len - 1) * step) << shift_mv) + 8192) >> sp) - ref_i + 1
    if min1:
        ext = max(1, ext)
    prec = ref_pos & ((1 << sp) - 1)
    lo = i32(i32(-((ext + 4) << sp)) + prec)
    hi = i32(i32((pic_len + 3) << sp) + prec)
    return min(max(ref_pos, lo), hi), step


def clip_mv(x0, y0, pw, ph, pic_w, pic_h, mvx, mvy):
    mvx = min(max(mvx, -((pw + 3 + x0) << 4)), (pic_w + 2 - x0) << 4)
    mvy = min(max(mvy, -((ph + 3 + y0) << 4)), (pic_h + 2 - y0) << 4)
    return mvx, mvy


def _rows(plane, ys):
    return plane[np.clip(ys, 0, plane.shape[0] - 1)]


def _cols(rows, xs):
    return rows[:, np.clip(xs, 0, rows.shape[1] - 1)]


def scaled_plane(plane, ax, ay, step_x, step_y, fh, fv, w, h, shift_mv, table, bi):
    """rcn_mcp_rpr_{l,c} (uni: clipped samples) / rcn_mcp_rpr_bi_{l,c} (bi: 14-bit) over a whole PU."""
    nt = table.shape[2]
    b = nt // 2 - 1
    mask = (1 << shift_mv) - 1
    px = [i32(ax + ((c * step_x) << shift_mv) + 8192) >> 14 for c in range(w)]
    py = [i32(ay + ((r * step_y) << shift_mv) + 8192) >> 14 for r in range(h)]
    ix = [p >> shift_mv for p in px]
    iy = [p >> shift_mv for p in py]
    y0 = iy[0]
    nrows = iy[-1] - y0 + nt
    src = _rows(plane.astype(np.int64), np.arange(y0 - b, y0 - b + nrows))
    hor = np.zeros((nrows, w), dtype=np.int64)
    for c in range(w):
        taps = table[fh][px[c] & mask]
        win = _cols(src, np.arange(ix[c] - b, ix[c] - b + nt))
        hor[:, c] = (win @ taps) >> 2
    hor = hor.astype(np.int16).astype(np.int64)
    out = np.zeros((h, w), dtype=np.int64)
    for r in range(h):
        ph = py[r] & mask
        base = iy[r] - y0
        acc = table[fv][ph] @ hor[base:base + nt]
        if bi:
            out[r] = acc >> 6
        elif fv == 0 and ph == 0:
            out[r] = np.clip(((hor[base + b] & 0xFFFF) + 8) >> 4, 0, 1023)
        else:
            out[r] = np.clip(((acc >> 6) + 8) >> 4, 0, 1023)
    return out


def regular_bi_plane(plane, x, y, w, h, mvx, mvy, shift_mv, table, hpel=False):
    """rcn_mcp_bidir0_{l,c}: the regular 14-bit prediction (mv already clipped), the reference's four variants."""
    nt = table.shape[1]
    b = nt // 2 - 1
    mask = (1 << shift_mv) - 1
    fx, fy = mvx & mask, mvy & mask
    if hpel and shift_mv == 4:
        fx = 16 if fx == 8 else fx
        fy = 16 if fy == 8 else fy
    bx, by = x + (mvx >> shift_mv), y + (mvy >> shift_mv)
    p = plane.astype(np.int64)
    if not fx and not fy:
        return _cols(_rows(p, np.arange(by, by + h)), np.arange(bx, bx + w)) << 4
    if fx and not fy:
        src = _rows(p, np.arange(by, by + h))
        return sum(table[fx][k] * _cols(src, np.arange(bx - b + k, bx - b + k + w)) for k in range(nt)) >> 2
    if fy and not fx:
        src = _cols(_rows(p, np.arange(by - b, by - b + h + nt - 1)), np.arange(bx, bx + w))
        return sum(table[fy][k] * src[k:k + h] for k in range(nt)) >> 2
    src = _rows(p, np.arange(by - b, by - b + h + nt - 1))
    hor = sum(table[fx][k] * _cols(src, np.arange(bx - b + k, bx - b + k + w)) for k in range(nt)) >> 2
    return sum(table[fy][k] * hor[k:k + h] for k in range(nt)) >> 6


def predict_pu(refs, scales, pic_w, pic_h, pu, lmcs_lut=None):
    """refs: slot -> (Y, Cb, Cr) numpy planes of the reference's own size; scales: slot -> dict(scale_hor, scale_ver,
    ref_w, ref_h, col_hor, col_ver) (missing = unscaled).  pu: dict with x0, y0, log2_w, log2_h, inter_dir, ref0, ref1,
    mv0x, mv0y, mv1x, mv1y, bcw_idx_plus1, poc0, poc1, lmcs, prec_amvr_half.  Returns (Y, Cb, Cr) of the PU, as
    rcn_mcp_b writes them when at least one used list is scaled."""
    x0, y0, pw, ph = pu["x0"], pu["y0"], 1 << pu["log2_w"], 1 << pu["log2_h"]
    dir_ = pu["inter_dir"] & 3
    if dir_ == 3 and pu["poc0"] == pu["poc1"] and pu["mv0x"] == pu["mv1x"] and pu["mv0y"] == pu["mv1y"]:
        dir_ = 2
    elif dir_ != 3 and dir_ & 2:
        dir_ = 2
    bi = dir_ == 3

    def sc(slot):
        return scales.get(slot, dict(scale_hor=UNSCALED, scale_ver=UNSCALED, ref_w=pic_w, ref_h=pic_h, col_hor=0, col_ver=0))

    def side(l):
        slot = pu["ref1"] if l else pu["ref0"]
        mvx, mvy = (pu["mv1x"], pu["mv1y"]) if l else (pu["mv0x"], pu["mv0y"])
        s = sc(slot)
        Y, Cb, Cr = refs[slot]
        if s["scale_hor"] == UNSCALED and s["scale_ver"] == UNSCALED:
            mx, my = clip_mv(x0, y0, pw, ph, pic_w, pic_h, mvx, mvy)
            yl = regular_bi_plane(Y, x0, y0, pw, ph, mx, my, 4, MC_LUMA, bool(pu.get("prec_amvr_half")))
            cs = [regular_bi_plane(P, x0 >> 1, y0 >> 1, pw >> 1, ph >> 1, mx, my, 5, MC_CHROMA) for P in (Cb, Cr)]
            return yl, cs
        f4 = pw == 4 and ph == 4
        fh, fv = filter_idx(s["scale_hor"], f4), filter_idx(s["scale_ver"], f4)
        ax, stx = anchor(x0, mvx, s["scale_hor"], 0, pw, s["ref_w"], 4, False)
        ay, sty = anchor(y0, mvy, s["scale_ver"], 0, ph, s["ref_h"], 4, True)
        yl = scaled_plane(Y, ax, ay, stx, sty, fh, fv, pw, ph, 4, RPR_LUMA, bi)
        add_x = (1 - s["col_hor"]) * 8 * (s["scale_hor"] - UNSCALED)
        add_y = (1 - s["col_ver"]) * 8 * (s["scale_ver"] - UNSCALED)
        cx, _ = anchor(x0 >> 1, mvx, s["scale_hor"], add_x, pw >> 1, s["ref_w"] >> 1, 5, False)
        cy, _ = anchor(y0 >> 1, mvy, s["scale_ver"], add_y, ph >> 1, s["ref_h"] >> 1, 5, True)
        cs = [scaled_plane(P, cx, cy, stx, sty, fh, fv, pw >> 1, ph >> 1, 5, RPR_CHROMA, bi) for P in (Cb, Cr)]
        return yl, cs

    used = [pu["ref1"] if l else pu["ref0"] for l in (0, 1) if dir_ & (1 << l)]
    if all(sc(slot)["scale_hor"] == UNSCALED and sc(slot)["scale_ver"] == UNSCALED for slot in used):
        raise ValueError("no scaled list: not a reference-picture-resampling PU")
    if not bi:
        yl, (cb, cr) = side(0 if dir_ == 1 else 1)
    else:
        (y_0, c_0), (y_1, c_1) = side(0), side(1)
        b = pu.get("bcw_idx_plus1", 0)
        if b in (0, 3):
            comb = lambda a, c: np.clip((a + c + 16) >> 5, 0, 1023)
        else:
            w1 = BCW[b - 1]
            comb = lambda a, c: np.clip((a * (8 - w1) + c * w1 + 64) >> 7, 0, 1023)
        yl, cb, cr = comb(y_0, y_1), comb(c_0[0], c_1[0]), comb(c_0[1], c_1[1])
    if pu.get("lmcs") and lmcs_lut is not None:
        yl = np.asarray(lmcs_lut, dtype=np.int64)[yl]
    return yl.astype(np.uint16), cb.astype(np.uint16), cr.astype(np.uint16)


def scale_factor(ref_len: int, cur_len: int) -> int:
    """ctudec_compute_refs_scaling for windows equal to the pictures."""
    return ((ref_len << 14) + (cur_len >> 1)) // cur_len
