"""Intra block copy restated in numpy: the reference's per-CTU-row ring (rcn_attach_ctu_buff, rcn_ctu.c:554-568; rcn_ibc_l / rcn_ibc_c,
rcn_ibc.c:8-139) with its wrap split and the chroma floor, the residual of a DC-only or transform-skip transform unit, residual add and clip.
Beside it the same picture decoded by reading the PICTURE at (x0 + mv_x, y0 + mv_y), which is what the device does; the two agree inside the
window ovhip_rec_ibc_check accepts (include/ovvc_hip.h, ovhip_ibc_desc).

Fixtures (tests/golden/ibc/*.ovg, written by tools/ibc_golden/gen_ibc.c from the reference's own slots): per scenario <s> the arrays
<s>_dims, <s>_bg_*, <s>_exp_*, <s>_cu [n][8] = (x0, y0, log2_w, log2_h, mv_x, mv_y, has_chroma, first TU), <s>_tu [m][14] = (CU, x0, y0,
log2_w, log2_h, tree, cbf_mask, tr_skip_mask, last_pos x 3 (Cb, Cr, Y), coefficient offsets x 3 or -1), <s>_map, <s>_coef, <s>_state."""
import numpy as np

import golden_io

BD = 10
PIX_MAX = (1 << BD) - 1
IQ_SCALE = ((40, 45, 51, 57, 64, 72), (57, 64, 72, 80, 90, 102))
CU_X0, CU_Y0, CU_L2W, CU_L2H, CU_MVX, CU_MVY, CU_CHROMA, CU_FIRST_TU = range(8)
TU_CU, TU_X0, TU_Y0, TU_L2W, TU_L2H, TU_TREE, TU_CBF, TU_TS = range(8)
TU_LAST, TU_COEF = 8, 11            # + component: 0 Cb, 1 Cr, 2 Y
FLG_IBC = 1 << 12                   # flg_ibc_flag (cu_utils.h)


class Scenario:
    def __init__(self, g: dict, s: str):
        self.name = s
        self.w, self.h, self.log2_ctu, self.log2_max_tb = (int(v) for v in g[f"{s}_dims"])
        self.bg = [g[f"{s}_bg_{p}"] for p in ("y", "cb", "cr")]
        self.exp = [g[f"{s}_exp_{p}"] for p in ("y", "cb", "cr")]
        self.cu, self.tu, self.map, self.coef = g[f"{s}_cu"], g[f"{s}_tu"], g[f"{s}_map"], np.ascontiguousarray(g[f"{s}_coef"])
        self.state = g[f"{s}_state"].tobytes()

    def tus_of(self, i: int):
        a = int(self.cu[i][CU_FIRST_TU])
        b = int(self.cu[i + 1][CU_FIRST_TU]) if i + 1 < len(self.cu) else len(self.tu)
        return range(a, b)


_cache = {}


def scenario(s: str) -> Scenario:
    """a, c: tests/golden/ibc/ibc.ovg; b: ibc_rows.ovg"""
    f = "ibc/ibc_rows.ovg" if s == "b" else "ibc/ibc.ovg"
    if f not in _cache:
        _cache[f] = golden_io.load(f)
    return Scenario(_cache[f], s)


def n_ring_ctb(log2_ctu: int) -> int:
    return ((256 * 128) >> log2_ctu) >> log2_ctu


def in_window(cu, log2_ctu: int, pic_w: int, pic_h: int, win_x0: int = 0) -> bool:
    """The rule of ovhip_rec_ibc_check, restated."""
    x0, y0, w, h = int(cu[CU_X0]), int(cu[CU_Y0]), 1 << int(cu[CU_L2W]), 1 << int(cu[CU_L2H])
    sx, sy, cx = x0 + int(cu[CU_MVX]), y0 + int(cu[CU_MVY]), x0 >> log2_ctu
    if sy < 0 or (sy >> log2_ctu) != (y0 >> log2_ctu) or ((sy + h - 1) >> log2_ctu) != (y0 >> log2_ctu):
        return False
    if sx < max(win_x0, (cx - (n_ring_ctb(log2_ctu) - 1)) << log2_ctu, 0):
        return False
    if sx + w > min((cx + 1) << log2_ctu, pic_w) or sy + h > pic_h:
        return False
    return not (sx < x0 + w and sx + w > x0 and sy < y0 + h and sy + h > y0)


def dc_residual(c0: int, qp: int, log2_w: int, log2_h: int) -> int:
    """A DC-only block (inverse_dct_ii_dc, rcn_transform.c:576-598) after the regular (non dependent) de-quantisation."""
    l2s = log2_w + log2_h
    shift = 6 - 5 - qp // 6 + (l2s >> 1) + (l2s & 1)
    scale = IQ_SCALE[l2s & 1][qp % 6]
    v = c0 * (scale << -shift) if shift < 0 else (c0 * scale + ((1 << shift) >> 1)) >> shift
    v = int(np.clip(v, -32768, 32767))
    return int(np.clip((((v + 1) >> 1) + (1 << (14 - BD - 1))) >> (14 - BD), -32768, 32767))


def tu_residual(sc: Scenario, t: int, comp: int):
    """Residual block (int32) of component comp (0 Cb, 1 Cr, 2 Y) of transform unit t, or None when its cbf is 0."""
    tu = sc.tu[t]
    bit = 0x10 if comp == 2 else (0x1 if comp else 0x2)
    if not int(tu[TU_CBF]) & bit:
        return None
    l2w, l2h = int(tu[TU_L2W]) - (comp != 2), int(tu[TU_L2H]) - (comp != 2)
    off = int(tu[TU_COEF + comp])
    if int(tu[TU_TS]) & bit:                                      # transform skip with TS residual coding: the levels are the residual
        return sc.coef[off:off + (1 << (l2w + l2h))].astype(np.int32).reshape(1 << l2h, 1 << l2w)
    qp = sc.state[0 if comp == 2 else 1 + comp]
    return np.full((1 << l2h, 1 << l2w), dc_residual(int(sc.coef[off]), qp, l2w, l2h), np.int32)


def scaled(res: np.ndarray, scale: int) -> np.ndarray:
    """LMCS chroma residual scaling of a block larger than 2x2 (rcn_residuals.c: ict with scale)"""
    a = (np.minimum(np.abs(res), PIX_MAX) * scale + (1 << 10)) >> 11
    return np.clip(np.where(res < 0, -a, a), -(1 << 15), 1 << 15)


def _add_residuals(sc: Scenario, i: int, planes, origin, chroma_scale):
    """planes: views whose (0, 0) is picture position `origin` (luma samples)"""
    ox, oy = origin
    for t in sc.tus_of(i):
        tu = sc.tu[t]
        for comp in (2, 0, 1):
            r = tu_residual(sc, t, comp)
            if r is None:
                continue
            sh = comp != 2
            if sh and chroma_scale is not None and r.size > 4:
                r = scaled(r, chroma_scale)
            x, y = (int(tu[TU_X0]) - ox) >> sh, (int(tu[TU_Y0]) - oy) >> sh
            p = planes[0 if comp == 2 else 1 + comp]
            blk = p[y:y + r.shape[0], x:x + r.shape[1]]
            blk[...] = np.clip(blk.astype(np.int32) + r, 0, PIX_MAX).astype(np.uint16)


def decode_ring(sc: Scenario, bg=None, chroma_scale=None, poison: int = 0xABAB):
    """The scenario through the reference's ring: returns ([Y, Cb, Cr], per CU the luma and chroma source blocks the ring delivered)."""
    bg = sc.bg if bg is None else bg
    l2c, S = sc.log2_ctu, 1 << sc.log2_ctu
    ring_w = (256 * 128) >> l2c
    msk_h, msk_v, ctb_msk = ring_w - 1, S - 1, n_ring_ctb(l2c) - 1
    out = [np.array(p, dtype=np.uint16) for p in bg]
    reads = [None] * len(sc.cu)
    i = 0
    for cy in range((sc.h + S - 1) >> l2c):
        ring = [np.full((S, ring_w), poison, np.uint16), np.full((S // 2, ring_w // 2), poison, np.uint16), np.full((S // 2, ring_w // 2), poison, np.uint16)]
        for cx in range((sc.w + S - 1) >> l2c):
            X0, Y0 = cx << l2c, cy << l2c
            cw, ch = min(S, sc.w - X0), min(S, sc.h - Y0)
            ctb_pos = (cx & ctb_msk) << l2c                       # rcn_attach_ctu_buff: the CTU's columns of the ring
            ring[0][:ch, ctb_pos:ctb_pos + cw] = bg[0][Y0:Y0 + ch, X0:X0 + cw]
            for p in (1, 2):
                ring[p][:ch // 2, ctb_pos // 2:(ctb_pos + cw) // 2] = bg[p][Y0 // 2:(Y0 + ch) // 2, X0 // 2:(X0 + cw) // 2]
            while i < len(sc.cu) and int(sc.cu[i][CU_X0]) >> l2c == cx and int(sc.cu[i][CU_Y0]) >> l2c == cy:
                cu = sc.cu[i]
                x0, y0, w, h = int(cu[CU_X0]) - X0, int(cu[CU_Y0]) - Y0, 1 << int(cu[CU_L2W]), 1 << int(cu[CU_L2H])
                ref_x, ref_y = (ctb_pos + x0 + int(cu[CU_MVX])) & msk_h, (y0 + int(cu[CU_MVY])) & msk_v
                wrap = ref_x + w > ring_w
                size1 = ref_x + w - ring_w if wrap else 0         # columns taken from the ring's start
                src = np.concatenate([ring[0][ref_y:ref_y + h, ref_x:ref_x + w - size1], ring[0][ref_y:ref_y + h, :size1]], axis=1)
                ring[0][y0:y0 + h, ctb_pos + x0:ctb_pos + x0 + w] = src
                rd = [src.copy(), None, None]
                if int(cu[CU_CHROMA]):
                    wc, hc = w >> 1, h >> 1
                    rxc, ryc = ref_x >> 1, ref_y >> 1             # (ref_x - ctb_pos) >> 1 from the CTU's chroma origin ctb_pos / 2: the floor
                    s1 = rxc + wc - ring_w // 2 if wrap else 0
                    for p in (1, 2):
                        srcc = np.concatenate([ring[p][ryc:ryc + hc, rxc:rxc + wc - s1], ring[p][ryc:ryc + hc, :s1]], axis=1)
                        ring[p][y0 >> 1:(y0 >> 1) + hc, (ctb_pos + x0) >> 1:((ctb_pos + x0) >> 1) + wc] = srcc
                        rd[p] = srcc.copy()
                reads[i] = rd
                views = [ring[0][:, ctb_pos:], ring[1][:, ctb_pos // 2:], ring[2][:, ctb_pos // 2:]]
                _add_residuals(sc, i, views, (X0, Y0), chroma_scale)
                i += 1
            out[0][Y0:Y0 + ch, X0:X0 + cw] = ring[0][:ch, ctb_pos:ctb_pos + cw]
            for p in (1, 2):
                out[p][Y0 // 2:(Y0 + ch) // 2, X0 // 2:(X0 + cw) // 2] = ring[p][:ch // 2, ctb_pos // 2:(ctb_pos + cw) // 2]
    assert i == len(sc.cu)
    return out, reads


def decode_picture(sc: Scenario, bg=None, chroma_scale=None, cus=None):
    """The same by reading the picture itself at the vector's distance (chroma: the vector halved, arithmetic): what the device does.
    cus: the CUs to run (indices, in order); default all."""
    bg = sc.bg if bg is None else bg
    out = [np.array(p, dtype=np.uint16) for p in bg]
    reads = {}
    for i in (range(len(sc.cu)) if cus is None else cus):
        cu = sc.cu[i]
        x0, y0, w, h, mx, my = int(cu[CU_X0]), int(cu[CU_Y0]), 1 << int(cu[CU_L2W]), 1 << int(cu[CU_L2H]), int(cu[CU_MVX]), int(cu[CU_MVY])
        src = out[0][y0 + my:y0 + my + h, x0 + mx:x0 + mx + w].copy()
        out[0][y0:y0 + h, x0:x0 + w] = src
        rd = [src, None, None]
        if int(cu[CU_CHROMA]):
            xc, yc, dx, dy = x0 >> 1, y0 >> 1, mx >> 1, my >> 1
            for p in (1, 2):
                srcc = out[p][yc + dy:yc + dy + (h >> 1), xc + dx:xc + dx + (w >> 1)].copy()
                out[p][yc:yc + (h >> 1), xc:xc + (w >> 1)] = srcc
                rd[p] = srcc
        reads[i] = rd
        _add_residuals(sc, i, out, (0, 0), chroma_scale)
    return out, reads
