"""TEST INFRASTRUCTURE: what the SAO and ALF slot fixtures reach of what k_sao and k_alf decide.

Pure numpy.  The module restates both filters from the reference's rcn_sao.c (sao_band_filter / sao_edge_filter / rcn_sao_ctu with
the callers rcn_sao_first_pix_rows and rcn_sao_filter_line) and rcn_alf.c (alf_derive_filter_idx, rcn_alf_classif_{vbnd,novbnd},
the luma and chroma filters with their virtual-boundary variants, cc_alf_filterBlk, rcn_alf_filter_line) -- not from the kernels --
and labels everything they decide on the way.  tests/test_oracle_golden.py asserts the restated planes EQUAL to the reference's
expected planes on every SAO and ALF fixture; a label comes only out of the functions that computed those planes, which is what
makes it trustworthy.

    sao(pic, prm, log2_ctu)      -> (HostPic, [labels of plane 0, 1, 2])         labels: one array entry per sample
    alf(pic, tables, log2_ctu)   -> (HostPic, labels)                            labels: per 4x4 block, per sample, per CTU
    sao_reach / alf_reach        -> {family of cells: set}                       what a list of labels reaches
    sao_cells_that_exist / alf_cells_that_exist                                 derived from the arithmetic
    sao_paths / alf_paths        -> the load / store / staging paths a launch on a picture of given strides enters

Bit depth 10 throughout, 4:2:0."""
import numpy as np

from oracle_lib import HostPic
from openvvc_amd import capi

BD, PIX_MAX = 10, 1023
SAO_BAND, SAO_EDGE = 1, 2
B_LEFT, B_RIGHT, B_UPPER, B_BOTTOM, B_ONE_ROW = capi.BORDER_LEFT, capi.BORDER_RIGHT, capi.BORDER_UPPER, capi.BORDER_BOTTOM, capi.BORDER_ONE_ROW
SAO_TW, SAO_TH, ALF_TL = 64, 32, 32                    # the device tiles
# neighbour a of the edge classes (dx, dy); neighbour b is the mirrored one (rcn_sao.c: horizontal, vertical, 135 and 45 degrees)
EO_A = ((-1, 0), (0, -1), (-1, -1), (1, -1))
SKIP_REASONS = ("picture column", "picture row", "entry column", "entry row", "6-row quirk", "BORDER_ONE_ROW")
CLIP_LUT = (1 << BD, 1 << (BD - 8 + 7 - 2), 1 << (BD - 8 + 7 - 4), 1 << (BD - 8 + 7 - 6))        # alf_clip_lut
TH = np.array([0, 1, 2, 2, 2, 2, 2, 3, 3, 3, 3, 3, 3, 3, 3, 4])
TR_LUT = np.array([0, 1, 0, 2, 2, 3, 1, 3])
# the 12 luma / 6 chroma tap pairs: (dx, which row offset: 3, 2, 1 = min(d, 3 / 2 / 1), 0 = the sample's own row)
LUMA_TAPS = ((0, 3), (1, 2), (0, 2), (-1, 2), (2, 1), (1, 1), (0, 1), (-1, 1), (-2, 1), (3, 0), (2, 0), (1, 0))
CHROMA_TAPS = ((0, 2), (1, 1), (0, 1), (-1, 1), (2, 0), (1, 0))
TIES = ("v=h", "d=b", "cross", "2max=9min", "max=2min")


def planes_of(pic):
    return (pic.y, pic.cb, pic.cr)


# ===================================================================================================================== SAO
def sao(pic, prm, log2_ctu=7):
    """The restated SAO of a whole picture and its per-sample labels.  prm: capi.SAO_CTU_DTYPE, raster order."""
    out = HostPic(pic.w, pic.h)
    labels = []
    nbw = (pic.w + (1 << log2_ctu) - 1) >> log2_ctu
    one_row = pic.h <= (1 << log2_ctu)             # rcn_sao_first_pix_rows passes the BOTTOM flag for its 6-row band then
    for c, (s, d) in enumerate(zip(planes_of(pic), planes_of(out))):
        sh = 1 if c else 0
        h, w = s.shape
        l2, cs = log2_ctu - sh, 1 << (log2_ctu - sh)
        yy, xx = np.mgrid[0:h, 0:w]
        ci = (yy >> l2) * nbw + (xx >> l2)
        typ, bp, eo, bd = prm["type"][ci, c], prm["band_position"][ci, c].astype(int), prm["eo_class"][ci, c].astype(int), prm["border"][ci].astype(int)
        off = prm["offset_val"][ci, c].astype(int)                                   # (h, w, 5)
        v = s.astype(int)
        res = v.copy()
        # ---- band
        k = ((v >> (BD - 5)) - bp) & 31
        band = typ == SAO_BAND
        hit = band & (k < 4)
        bsum = v + np.take_along_axis(off, np.minimum(k, 3)[..., None], 2)[..., 0]
        res[hit] = np.clip(bsum, 0, PIX_MAX)[hit]
        # ---- edge
        edge = typ == SAO_EDGE
        cx0, cy0 = xx & ~(cs - 1), yy & ~(cs - 1)
        cx1, cy1 = np.minimum(cx0 + cs, w) - 1, np.minimum(cy0 + cs, h) - 1
        q = (6 >> sh) - 1
        reasons = np.stack([(eo != 1) & ((xx == 0) | (xx == w - 1)),
                            (eo != 0) & ((yy == 0) | (yy == h - 1)),
                            (eo != 1) & ((((bd & B_LEFT) != 0) & (xx == cx0)) | (((bd & B_RIGHT) != 0) & (xx == cx1))),
                            (eo != 0) & ((((bd & B_UPPER) != 0) & (yy == cy0)) | (((bd & B_BOTTOM) != 0) & (yy == cy1))),
                            (eo != 0) & one_row & (yy == q),
                            (eo != 0) & ((bd & B_ONE_ROW) != 0) & (yy == cy0 + q)]) & edge
        skip = reasons.any(0)
        pad = np.pad(v, 1)
        dxa, dya = np.array([p[0] for p in EO_A])[eo], np.array([p[1] for p in EO_A])[eo]
        a, b = pad[yy + dya + 1, xx + dxa + 1], pad[yy - dya + 1, xx - dxa + 1]
        sa, sb = np.sign(v - a), np.sign(v - b)
        idx = 2 + sa + sb
        esum = v + np.take_along_axis(off, idx[..., None], 2)[..., 0]
        run = edge & ~skip
        res[run] = np.clip(esum, 0, PIX_MAX)[run]
        d[:] = res
        total = np.where(hit, bsum, np.where(run, esum, v))
        ax, ay, bx, by = xx + dxa, yy + dya, xx - dxa, yy - dya
        across = lambda f: run & ((f(ax, ay) != f(xx, yy)) | (f(bx, by) != f(xx, yy)))
        labels.append({
            "plane": c, "w": w, "h": h, "type": typ.astype(int), "band_k": np.where(hit, k, -1), "band_pos": bp,
            "band_wrap": hit & ((v >> (BD - 5)) < bp),                               # the four bands run past 31: `& 31` acts
            "eo": eo, "idx": np.where(run, idx, -1), "sa": sa, "sb": sb, "run": run, "skip": reasons,
            "clip": np.where(total < 0, -1, np.where(total > PIX_MAX, 1, 0)), "group": xx & 7,
            "across_ctu": across(lambda x, y: (x >> l2) + 4096 * (y >> l2)), "across_tile": across(lambda x, y: x // SAO_TW + 4096 * (y // SAO_TH)),
            "across_lane": run & ((ax >> 3 != xx >> 3) | (bx >> 3 != xx >> 3)) & (dya == 0) | run & (dya != 0)})
    return out, labels


def sao_cells_that_exist():
    """Per plane.  A sign pair of an edge class: each comparison `<`, `=`, `>` on its own; a sample next to the picture's first or last
    column (row) is skipped, so group position 0 takes its left neighbour from ra[0] / rb[0] only from the second group on."""
    cells = {"type": set(), "band_k": set(), "band_pos": set(), "edge": set(), "clip": set(), "skip": set(), "group": set(), "across": set()}
    for p in range(3):
        cells["type"] |= {(p, t) for t in (0, SAO_BAND, SAO_EDGE)}
        cells["band_k"] |= {(p, k) for k in (-1, 0, 1, 2, 3)}
        cells["band_pos"] |= {(p, bp, wrap) for bp in range(32) for wrap in (False, True) if wrap <= (bp > 28)}
        cells["edge"] |= {(p, eo, sa, sb) for eo in range(4) for sa in (-1, 0, 1) for sb in (-1, 0, 1)}
        cells["clip"] |= {(p, t, e) for t in ("band", "edge") for e in (0, PIX_MAX)}
        cells["skip"] |= {(p, r) for r in SKIP_REASONS}
        cells["group"] |= {(p, eo, g) for eo in (0, 2, 3) for g in (0, 7)}
        cells["across"] |= {(p, k) for k in ("ctu", "tile", "lane")}
    return cells


def sao_reach(labels):
    """labels: the per-plane label dicts of any number of pictures"""
    r = {k: set() for k in sao_cells_that_exist()}
    for lb in labels:
        p = lb["plane"]
        r["type"] |= {(p, int(t)) for t in np.unique(lb["type"])}
        band = lb["type"] == SAO_BAND
        r["band_k"] |= {(p, int(k)) for k in np.unique(lb["band_k"][band])}
        hit = lb["band_k"] >= 0
        r["band_pos"] |= {(p, int(b), bool(wr)) for b, wr in set(zip(lb["band_pos"][hit].tolist(), lb["band_wrap"][hit].tolist()))}
        run = lb["run"]
        r["edge"] |= {(p,) + t for t in set(zip(lb["eo"][run].tolist(), lb["sa"][run].tolist(), lb["sb"][run].tolist()))}
        for t, m in (("band", hit), ("edge", run)):
            r["clip"] |= {(p, t, 0 if e < 0 else PIX_MAX) for e in np.unique(lb["clip"][m]) if e}
        r["skip"] |= {(p, SKIP_REASONS[i]) for i in range(len(SKIP_REASONS)) if lb["skip"][i].any()}
        g = run & np.isin(lb["eo"], (0, 2, 3)) & np.isin(lb["group"], (0, 7))
        r["group"] |= {(p,) + t for t in set(zip(lb["eo"][g].tolist(), lb["group"][g].tolist()))}
        r["across"] |= {(p, k) for k in ("ctu", "tile", "lane") if lb["across_" + k].any()}
    return r


def sao_paths(w, h, stride_y, stride_c):
    """(plane, path) of the lanes of a k_sao launch: "16-byte" (a full group of 8, strides multiples of 8 samples; the planes of a
    picture start 16-byte aligned), "scalar" (a full group loaded sample by sample) and "ragged" (the last group of a row, n < 8)."""
    out = set()
    for p in range(3):
        wp, st = (w >> 1, stride_c) if p else (w, stride_y)
        vec = not st & 7
        if wp >= 8:
            out.add((p, "16-byte" if vec else "scalar"))
        if wp & 7:
            out.add((p, "ragged"))
    return out


# ===================================================================================================================== ALF
def _rect(border, cx0, cy0, ctu, w, h):
    """the rectangle a CTU's windows are clamped to (rcn_extend_filter_region pads at the picture's and at the rect entry's borders)"""
    x0, y0, x1, y1 = 0, 0, w - 1, h - 1
    if border & B_LEFT:
        x0 = cx0
    if border & B_UPPER:
        y0 = cy0
    if border & B_RIGHT:
        x1 = min(x1, cx0 + ctu - 1)
    if border & B_BOTTOM:
        y1 = min(y1, cy0 + ctu - 1)
    return x0, y0, x1, y1


def _window(plane, rect, x0, y0, w, h, halo):
    """samples [y0 - halo, y0 + h + halo) x [x0 - halo, x0 + w + halo) with the coordinates clamped to rect, as int"""
    ys = np.clip(np.arange(y0 - halo, y0 + h + halo), rect[1], rect[3])
    xs = np.clip(np.arange(x0 - halo, x0 + w + halo), rect[0], rect[2])
    return plane[np.ix_(ys, xs)].astype(np.int64)


def filter_idx(sum_h, sum_v, sum_d, sum_b, is_vb):
    """alf_derive_filter_idx on arrays (uint32 arithmetic: the products stay below 2^32, asserted)"""
    sum_h, sum_v, sum_d, sum_b = (np.asarray(a, np.int64) for a in (sum_h, sum_v, sum_d, sum_b))
    scale = np.where(is_vb, 96, 64)
    act = np.minimum(((sum_h + sum_v) * scale) >> (BD + 4), 15)
    v_gt = sum_v > sum_h
    max_hv, min_hv, dir_hv = np.where(v_gt, sum_v, sum_h), np.where(v_gt, sum_h, sum_v), np.where(v_gt, 1, 3)
    d_gt = sum_d > sum_b
    max_db, min_db, dir_db = np.where(d_gt, sum_d, sum_b), np.where(d_gt, sum_b, sum_d), np.where(d_gt, 0, 2)
    assert (max_db * min_hv < 1 << 32).all() and (max_hv * min_db < 1 << 32).all()
    db = max_db * min_hv > max_hv * min_db
    max_dir, min_dir = np.where(db, max_db, max_hv), np.where(db, min_db, min_hv)
    main, sec = np.where(db, dir_db, dir_hv), np.where(db, dir_hv, dir_db)
    strong, weak = max_dir * 2 > 9 * min_dir, max_dir > 2 * min_dir
    dirc = np.where(strong, ((main & 1) << 1) + 2, np.where(weak, ((main & 1) << 1) + 1, 0))
    nz = (sum_h > 0) & (sum_v > 0) & (sum_d > 0) & (sum_b > 0)
    ties = np.stack([sum_v == sum_h, sum_d == sum_b, max_db * min_hv == max_hv * min_db, max_dir * 2 == 9 * min_dir, max_dir == 2 * min_dir]) & nz
    return {"act": act, "actc": TH[act], "dirc": dirc, "cls": TH[act] + 5 * dirc, "tr": TR_LUT[(main << 1) + (sec >> 1)], "ties": ties,
            "cross": np.maximum(max_db * min_hv, max_hv * min_db)}


def _classify_ctu(y, rect, cx0, cy0, cw, ch, vb):
    """sums (4, ch / 4, cw / 4) in the order v, h, d, b and is_vb (ch / 4) of a CTU's 4x4 blocks; vb: CTU-local row"""
    P = _window(y, rect, cx0, cy0, cw, ch, 4)
    o = 4
    npair, nq = ch // 2 + 2, cw // 2 + 2                       # row pairs r = -2 + 2 p, positions c0 = -2 + 2 q
    r = -2 + 2 * np.arange(npair)
    above, below = r - 1, r + 2
    below = np.where(r + 2 == vb, r + 1, below)                # pair (vb - 2, vb - 1): row vb is not available
    above = np.where(r == vb, r, above)                        # pair (vb, vb + 1): row vb - 1 is not available
    c0 = -2 + 2 * np.arange(nq)
    R = lambda rows, cols: P[np.ix_(rows + o, cols + o)]
    y1, y2 = 2 * R(r, c0), 2 * R(r + 1, c0 + 1)
    lap = np.stack([
        np.abs(y1 - R(above, c0) - R(r + 1, c0)) + np.abs(y2 - R(r, c0 + 1) - R(below, c0 + 1)),
        np.abs(y1 - R(r, c0 + 1) - R(r, c0 - 1)) + np.abs(y2 - R(r + 1, c0 + 2) - R(r + 1, c0)),
        np.abs(y1 - R(above, c0 - 1) - R(r + 1, c0 + 1)) + np.abs(y2 - R(r, c0) - R(below, c0 + 2)),
        np.abs(y1 - R(r + 1, c0 - 1) - R(above, c0 + 1)) + np.abs(y2 - R(below, c0) - R(r, c0 + 2))])
    nby, nbx = ch // 4, cw // 4
    colsum = sum(lap[:, :, k:k + 2 * nbx:2] for k in range(4))                     # (4, npair, nbx)
    lby = 4 * np.arange(nby)
    first, last = np.where(lby == vb, 1, 0), np.where(lby == vb - 4, 2, 3)
    sums = np.zeros((4, nby, nbx), np.int64)
    for k in range(4):
        use = (k >= first) & (k <= last)
        sums += colsum[:, k:k + 2 * nby:2] * use[None, :, None]
    return sums, (lby == vb) | (lby == vb - 4)


def _luma_rows(ctu, cy0, ch, H):
    """per CTU-local row: (d, near) of the luma filter; vb as the reference derives it (ctu - 4, or pic_h in a truncated CTU, where it
    is compared with CTU-local rows and so only ever matches in pictures of a single CTU row); check_virtual_bound picks the variant"""
    truncated = cy0 + ctu > H
    vb = H if truncated else ctu - 4
    last_local = (cy0 + ch - 1) & (ctu - 1)
    req_vb = (vb - 4 <= last_local < vb) or (vb <= last_local <= vb + 3)
    ly = np.arange(ch)
    d = np.full(ch, 3)
    near, side = np.zeros(ch, bool), np.zeros(ch, int)             # side: 1 = the four rows above the boundary, 2 = the four below
    if req_vb:
        side = np.where((ly < vb) & (ly >= vb - 4), 1, np.where((ly >= vb) & (ly <= vb + 3), 2, 0))
        d = np.where(side == 1, vb - 1 - ly, np.where(side == 2, ly - vb, 3))
        near = (ly == vb - 1) | (ly == vb)
    return vb, d, near, side


def _filter_block_rows(P, halo, w, h, d, near, taps, coef, clip):
    """The symmetric-tap filter of a window: P (h + 2 halo, w + 2 halo); d, near per row; coef / clip (ntaps, h, w).
    -> (output before the clip to the sample range, states (ntaps, 3, h, w): a difference of the tap not clipped / clipped low / high)"""
    yy, xx = np.mgrid[0:h, 0:w]
    cur = P[halo:halo + h, halo:halo + w]
    total = np.zeros((h, w), np.int64)
    states = np.zeros((len(taps), 3, h, w), bool)
    for k, (dx, which) in enumerate(taps):
        dy = np.minimum(d, which)[:, None] if which else 0
        a, b = P[yy + dy + halo, xx + dx + halo] - cur, P[yy - dy + halo, xx - dx + halo] - cur
        c = clip[k]
        total += coef[k] * (np.clip(a, -c, c) + np.clip(b, -c, c))
        states[k, 0] = (np.abs(a) <= c) | (np.abs(b) <= c)
        states[k, 1] = (a < -c) | (b < -c)
        states[k, 2] = (a > c) | (b > c)
    n = near[:, None]
    return cur + np.where(n, (total + 512) >> 10, (total + 64) >> 7), states


def _ctus(W, H, log2_ctu):
    ctu = 1 << log2_ctu
    nbw = (W + ctu - 1) // ctu
    for cy0 in range(0, H, ctu):
        for cx0 in range(0, W, ctu):
            yield (cy0 // ctu) * nbw + cx0 // ctu, cx0, cy0, min(ctu, W - cx0), min(ctu, H - cy0)


def classify(pic, tables, log2_ctu=7):
    """Luma classification of the CTUs with ALF luma on: {"sums" (4, H/4, W/4) v h d b, "is_vb", "on", "set", + filter_idx's arrays}"""
    W, H, ctu = pic.w, pic.h, 1 << log2_ctu
    sums, is_vb, on, lset = np.zeros((4, H // 4, W // 4), np.int64), np.zeros((H // 4, W // 4), bool), np.zeros((H // 4, W // 4), bool), np.zeros((H // 4, W // 4), int)
    for i, cx0, cy0, cw, ch in _ctus(W, H, log2_ctu):
        c = tables["ctus"][i]
        if not c["flags"] & 4:
            continue
        vb = _luma_rows(ctu, cy0, ch, H)[0]
        s, v = _classify_ctu(pic.y, _rect(int(c["border"]), cx0, cy0, ctu, W, H), cx0, cy0, cw, ch, vb)
        sl = (slice(cy0 // 4, (cy0 + ch) // 4), slice(cx0 // 4, (cx0 + cw) // 4))
        sums[(slice(None),) + sl] = s
        is_vb[sl] = v[:, None]
        on[sl], lset[sl] = True, int(c["luma_set"])
    out = filter_idx(sums[1], sums[0], sums[2], sums[3], is_vb)
    out.update(sums=sums, is_vb=is_vb, on=on, set=lset)
    return out


def luma_filter(pic, tables, cl, log2_ctu=7, cls=None, tr=None, want_states=True):
    """The luma plane filtered with the classes cl["cls"] / cl["tr"] (or the edited maps cls / tr): (plane before the output clip,
    per-sample labels).  CTUs with ALF luma off keep their samples."""
    W, H, ctu = pic.w, pic.h, 1 << log2_ctu
    cls, tr = cl["cls"] if cls is None else cls, cl["tr"] if tr is None else tr
    coef_t = np.asarray(tables["luma_coeff"], np.int64).reshape(-1, 4, 25, 13)
    clip_t = np.asarray(tables["luma_clip"], np.int64).reshape(-1, 4, 25, 13)
    out = pic.y.astype(np.int64)
    lb = {"d": np.full((H, W), 3), "near": np.zeros((H, W), bool), "on": np.zeros((H, W), bool), "side": np.zeros((H, W), int),
          "states": np.zeros((12, 3, H, W), bool), "clipidx": np.zeros((12, H, W), int)}
    for i, cx0, cy0, cw, ch in _ctus(W, H, log2_ctu):
        c = tables["ctus"][i]
        if not c["flags"] & 4:
            continue
        _, d, near, side = _luma_rows(ctu, cy0, ch, H)
        P = _window(pic.y, _rect(int(c["border"]), cx0, cy0, ctu, W, H), cx0, cy0, cw, ch, 3)
        bs = (slice(cy0 // 4, (cy0 + ch) // 4), slice(cx0 // 4, (cx0 + cw) // 4))
        up = lambda a: np.repeat(np.repeat(a, 4, 0), 4, 1)
        f = coef_t[int(c["luma_set"]), up(tr[bs]), up(cls[bs])]                       # (ch, cw, 13)
        k = clip_t[int(c["luma_set"]), up(tr[bs]), up(cls[bs])]
        res, st = _filter_block_rows(P, 3, cw, ch, d, near, LUMA_TAPS, np.moveaxis(f, 2, 0), np.moveaxis(k, 2, 0))
        sl = (slice(cy0, cy0 + ch), slice(cx0, cx0 + cw))
        out[sl] = res
        lb["on"][sl] = True
        if want_states:
            lb["d"][sl], lb["near"][sl], lb["side"][sl] = d[:, None], near[:, None], side[:, None]
            lb["states"][(slice(None), slice(None)) + sl] = st
            lb["clipidx"][(slice(None),) + sl] = np.searchsorted(-np.array(CLIP_LUT), -np.moveaxis(k, 2, 0)[:12])
    return out, lb


def _discriminates(pic, tables, cl, log2_ctu, base):
    """per 4x4 block: the filter of each other transpose of its class, of the class one step away in activity (within its group of five)
    and of the class one step away in direction gives ANOTHER 4x4 block, all from the picture's own tables"""
    cls, tr = cl["cls"], cl["tr"]
    ok = cl["on"].copy()
    edits = [(cls, (tr + k) & 3, None) for k in (1, 2, 3)]
    edits += [(cls - 1, tr, cls % 5 > 0), (cls + 1, tr, cls % 5 < 4), (cls - 5, tr, cls >= 5), (cls + 5, tr, cls < 20)]
    for c2, t2, valid in edits:
        c2 = np.clip(c2, 0, 24)
        other = np.clip(luma_filter(pic, tables, cl, log2_ctu, c2, t2, want_states=False)[0], 0, PIX_MAX)
        diff = (other != base).reshape(pic.h // 4, 4, pic.w // 4, 4).any((1, 3))
        ok &= diff if valid is None else (diff | ~valid)
    return ok


def _chroma(pic, tables, log2_ctu, comp, out, lb):
    W, H, ctu = pic.w, pic.h, 1 << log2_ctu
    Wc, Hc, ctuc = W // 2, H // 2, ctu // 2
    src = planes_of(pic)[comp]
    coef_t, clip_t = np.asarray(tables["chroma_coeff"], np.int64).reshape(8, 7), np.asarray(tables["chroma_clip"], np.int64).reshape(8, 7)
    cc_t = np.asarray(tables["cc_coeff"], np.int64).reshape(2, 4, 8)
    for i, cx0, cy0, cw, ch in _ctus(W, H, log2_ctu):
        c = tables["ctus"][i]
        x0, y0, w, h = cx0 // 2, cy0 // 2, cw // 2, ch // 2
        sl = (slice(y0, y0 + h), slice(x0, x0 + w))
        truncated = cy0 + ctu > H
        border = int(c["border"])
        res = src[sl].astype(np.int64)
        lb["flags"][sl] = int(c["flags"])
        if c["flags"] & (2 if comp == 1 else 1):
            alt = int(c["cb_alt"] if comp == 1 else c["cr_alt"])
            vb = H // 2 if truncated else (ctu - 4) // 2                       # alf_filter_cVB: always the virtual-boundary variant
            ly = np.arange(h)
            side = np.where((ly < vb) & (ly >= vb - 2), 1, np.where((ly >= vb) & (ly <= vb + 1), 2, 0))
            d = np.where(side == 1, vb - 1 - ly, np.where(side == 2, ly - vb, 2))
            near = (ly == vb - 1) | (ly == vb)
            lb["side"][sl] = side[:, None]
            P = _window(src, _rect(border, x0, y0, ctuc, Wc, Hc), x0, y0, w, h, 2)
            ones = np.ones((6, h, w), np.int64)
            res, st = _filter_block_rows(P, 2, w, h, d, near, CHROMA_TAPS, coef_t[alt, :6, None, None] * ones, clip_t[alt, :6, None, None] * ones)
            lb["on"][sl], lb["alt"][sl], lb["d"][sl], lb["near"][sl] = True, alt, d[:, None], near[:, None]
            lb["states"][(slice(None), slice(None)) + sl] = st
            lb["clipidx"][(slice(None),) + sl] = np.searchsorted(-np.array(CLIP_LUT), -clip_t[alt, :6])[:, None, None]
            lb["linear"][sl] = bool((clip_t[alt, :6] > PIX_MAX).all())
            lb["clip"][sl] = np.where(res < 0, -1, np.where(res > PIX_MAX, 1, 0))
            res = np.clip(res, 0, PIX_MAX)
        cc = int(c["cc_cb_idx"] if comp == 1 else c["cc_cr_idx"])
        if cc:
            # cc_alf_filterBlk: vbPos is NOT halved in a full-height CTU and is compared with the CTU-local LUMA row
            f = cc_t[comp - 1, cc - 1]
            vbpos = H // 2 if truncated else ctu - 4
            pos = (2 * (y0 + np.arange(h))) & (ctu - 1)
            r1, r2, r3 = np.ones(h, int), -np.ones(h, int), np.full(h, 2)
            same = (pos == vbpos - 2) | (pos == vbpos + 1)
            zero = (pos == vbpos - 1) | (pos == vbpos)
            r3 = np.where(same, r1, r3)
            r1, r2, r3 = (np.where(zero, 0, a) for a in (r1, r2, r3))
            L = _window(pic.y, _rect(border, cx0, cy0, ctu, W, H), cx0, cy0, cw, ch, 2)
            yy, xx = np.mgrid[0:h, 0:w]
            g = lambda dx, dy: L[2 * yy + (dy[:, None] if isinstance(dy, np.ndarray) else dy) + 2, 2 * xx + dx + 2]
            cy = g(0, 0)
            s = (f[0] * (g(0, r2) - cy) + f[1] * (g(-1, 0) - cy) + f[2] * (g(1, 0) - cy) + f[3] * (g(-1, r1) - cy)
                 + f[4] * (g(0, r1) - cy) + f[5] * (g(1, r1) - cy) + f[6] * (g(0, r3) - cy))
            s = ((s + 64) >> 7) + 512
            lb["cc_clip1"][sl] = np.where(s < 0, -1, np.where(s > PIX_MAX, 1, 0))
            s = np.clip(s, 0, PIX_MAX) + res - 512
            lb["cc_clip2"][sl] = np.where(s < 0, -1, np.where(s > PIX_MAX, 1, 0))
            res = np.clip(s, 0, PIX_MAX)
            lb["cc"][sl] = cc
            lb["cc_row"][sl] = np.where(zero, 2, np.where(same, 1, 0))[:, None]
        lb["full"][sl] = not truncated
        out[sl] = res


def alf(pic, tables, log2_ctu=7, discriminate=True):
    """The restated ALF of a whole picture and its labels: {"blocks": per 4x4 luma block, "luma": per luma sample, "waves": per wave of
    k_alf's luma tiles, "cb" / "cr": per chroma sample}"""
    out = HostPic(pic.w, pic.h)
    cl = classify(pic, tables, log2_ctu)
    raw, lb = luma_filter(pic, tables, cl, log2_ctu)
    lb["clip"] = np.where(raw < 0, -1, np.where(raw > PIX_MAX, 1, 0)) * lb["on"]
    out.y[:] = np.clip(raw, 0, PIX_MAX)
    cl["flat"] = (cl["sums"].sum(0) == 0) & cl["on"]
    cl["discriminates"] = _discriminates(pic, tables, cl, log2_ctu, out.y.astype(np.int64)) if discriminate else np.zeros_like(cl["on"])
    # the filter of a block is linear where none of its 12 clip values can clip a 10-bit difference
    clip_t = np.asarray(tables["luma_clip"], np.int64).reshape(-1, 4, 25, 13)
    cl["linear"] = (clip_t[cl["set"], cl["tr"], cl["cls"], :12] > PIX_MAX).all(-1)
    labels = {"blocks": cl, "luma": lb, "waves": _waves(cl, pic.w, pic.h), "w": pic.w, "h": pic.h, "log2_ctu": log2_ctu,
              "ctus": tables["ctus"]}
    for comp, name in ((1, "cb"), (2, "cr")):
        shape = (pic.h // 2, pic.w // 2)
        z = lambda dt=int: np.zeros(shape, dt)
        c = {"on": z(bool), "alt": z(), "d": np.full(shape, 2), "near": z(bool), "states": np.zeros((6, 3) + shape, bool),
             "clipidx": np.zeros((6,) + shape, int), "side": z(), "linear": z(bool), "clip": z(), "cc": z(), "cc_row": z(), "cc_clip1": z(), "cc_clip2": z(),
             "flags": z(), "full": z(bool)}
        _chroma(pic, tables, log2_ctu, comp, planes_of(out)[comp], c)
        labels[name] = c
    return out, labels


def _waves(cl, W, H):
    """a wave of a luma tile filters 16 blocks, two block rows of the 32x32 tile; it takes the linear form only if every block of it
    does (the vote over the lanes that are inside the picture's rows): "linear", "clipping" or "mixed" (blocks inside the picture)"""
    out = []
    for ty in range(0, H // 4, 2):
        for tx in range(0, W // 4, 8):
            on = cl["on"][ty:ty + 2, tx:tx + 8]
            if on.any():
                lin = cl["linear"][ty:ty + 2, tx:tx + 8][on]
                out.append("linear" if lin.all() else "mixed" if lin.any() else "clipping")
    return out


def alf_cells_that_exist():
    """Clip index 0 is 1 << 10: no difference of two 10-bit samples reaches it, so a tap with it is never clipped; with the other three
    a difference stays, is clipped low or is clipped high.  d and near: near holds on the rows d = 0 alone."""
    tap = lambda n: {(t, 0, 0) for t in range(n)} | {(t, ci, s) for t in range(n) for ci in (1, 2, 3) for s in (0, 1, 2)}
    return {"pair": {(c, t) for c in range(25) for t in range(4)}, "set": set(range(18)), "act": {(a, v) for a in range(16) for v in (False, True)},
            "ties": set(TIES), "luma_tap": tap(12), "chroma_tap": {(p,) + c for p in (1, 2) for c in tap(6)}, "wave": {"linear", "clipping", "mixed"},
            "clip": {(p, e) for p in range(3) for e in (0, PIX_MAX)}, "alt": {(p, a) for p in (1, 2) for a in range(8)},
            "cc": {(p, i) for p in (1, 2) for i in range(5)}, "cc_row": {(p, r) for p in (1, 2) for r in ("plain", "r3=r1", "zero")},
            "cc_clip": {(p, k, e) for p in (1, 2) for k in (1, 2) for e in (0, PIX_MAX)}, "flags": set(range(8)),
            # rows next to the virtual boundary: (plane, d, above / below, CTU of full height); in a truncated CTU the boundary is the
            # picture's height and matches CTU-local rows in pictures of a single CTU row alone, where no row lies below it
            "d": {(p, d, sd, full) for p, n in ((0, 4), (1, 2), (2, 2)) for d in range(n) for sd, full in (("above", True), ("below", True), ("above", False))},
            "thresholds": {(v, s) for v in (False, True) for s in ACT_EDGES[v]}}


# both sides of the four steps of th[]: sum_h + sum_v at which act becomes 1, 2, 7 and 15 (scale 64: >> 8; scale 96: * 96 >> 14)
ACT_EDGES = {False: (255, 256, 511, 512, 1791, 1792, 3839, 3840), True: (170, 171, 341, 342, 1194, 1195, 2559, 2560)}


def alf_reach(labels, kind=None):
    """labels: alf()'s label dicts of any number of pictures.  kind "fixed" / "aps": count the luma blocks of those sets only."""
    r = {k: set() for k in alf_cells_that_exist()}
    r.update(pair_n={}, vb_actc=set(), vb_dirc=set(), vb_tr=set(), all_zero=False, max_cross=0)
    for L in labels:
        b = L["blocks"]
        on = b["on"] & (True if kind is None else (b["set"] < 16) == (kind == "fixed"))
        good = on & b["discriminates"]
        for c, t in zip(b["cls"][good].tolist(), b["tr"][good].tolist()):
            r["pair_n"][(c, t)] = r["pair_n"].get((c, t), 0) + 1
        r["pair"] |= set(zip(b["cls"][good].tolist(), b["tr"][good].tolist()))
        r["set"] |= {int(c["luma_set"]) for c in L["ctus"] if c["flags"] & 4}
        r["act"] |= set(zip(b["act"][on].tolist(), b["is_vb"][on].tolist()))
        vb = on & b["is_vb"]
        r["vb_actc"] |= set(b["actc"][vb].tolist()); r["vb_dirc"] |= set(b["dirc"][vb].tolist()); r["vb_tr"] |= set(b["tr"][vb].tolist())
        r["ties"] |= {TIES[i] for i in range(5) if (b["ties"][i] & on).any()}
        hv = b["sums"][0] + b["sums"][1]
        r["thresholds"] |= {(bool(v), int(s)) for v in (False, True) for s in ACT_EDGES[v] if (on & (b["is_vb"] == v) & (hv == s)).any()}
        r["all_zero"] |= bool((on & b["flat"]).any())
        r["max_cross"] = max(r["max_cross"], int(b["cross"][on].max()) if on.any() else 0)
        r["wave"] |= set(L["waves"])
        lu = L["luma"]
        for t in range(12):
            for s in range(3):
                m = lu["states"][t, s] & lu["on"]
                r["luma_tap"] |= {(t, int(ci), s) for ci in np.unique(lu["clipidx"][t][m])}
        r["clip"] |= {(0, 0 if e < 0 else PIX_MAX) for e in np.unique(lu["clip"]) if e}
        full_rows = np.zeros((L["h"], L["w"]), bool)
        ctu = 1 << L["log2_ctu"]
        full_rows[:L["h"] // ctu * ctu] = True
        m = lu["on"] & (lu["side"] > 0)
        r["d"] |= {(0, d, ("above", "below")[sd - 1], f) for d, sd, f in set(zip(lu["d"][m].tolist(), lu["side"][m].tolist(), full_rows[m].tolist()))}
        for p, name in ((1, "cb"), (2, "cr")):
            c = L[name]
            for t in range(6):
                for s in range(3):
                    m = c["states"][t, s] & c["on"]
                    r["chroma_tap"] |= {(p, t, int(ci), s) for ci in np.unique(c["clipidx"][t][m])}
            r["clip"] |= {(p, 0 if e < 0 else PIX_MAX) for e in np.unique(c["clip"]) if e}
            r["alt"] |= {(p, int(a)) for a in np.unique(c["alt"][c["on"]])}
            r["cc"] |= {(p, int(i)) for i in np.unique(c["cc"])}
            r["cc_row"] |= {(p, ("plain", "r3=r1", "zero")[int(k)]) for k in np.unique(c["cc_row"][c["cc"] > 0])}
            for k in (1, 2):
                r["cc_clip"] |= {(p, k, 0 if e < 0 else PIX_MAX) for e in np.unique(c[f"cc_clip{k}"][c["cc"] > 0]) if e}
            r["flags"] |= {int(f) for f in np.unique(c["flags"])}
            m = c["on"] & (c["side"] > 0)
            r["d"] |= {(p, d, ("above", "below")[sd - 1], f) for d, sd, f in set(zip(c["d"][m].tolist(), c["side"][m].tolist(), c["full"][m].tolist()))}
    return r


def alf_paths(w, h, stride_y, stride_c, tables, log2_ctu=7):
    """What the tiles of a k_alf launch enter, from the kernel's selectors restated on the picture's geometry:
    ("luma" / "chroma", staging "16-byte" / "clamped" / "copy" (luma, ALF off) / "none" (chroma off), store "8-byte" / "scalar")
    and ("cc", "inside" / "clamped"); plus per luma tile the sides its window is clamped at."""
    ctu = 1 << log2_ctu
    nbw = (w + ctu - 1) // ctu
    out, sides = set(), set()
    for plane, (pw, ph, st, s, halo) in (("luma", (w, h, stride_y, ctu, 3)), ("chroma", (w // 2, h // 2, stride_c, ctu // 2, 2))):
        for ty0 in range(0, ph, ALF_TL):
            for tx0 in range(0, pw, ALF_TL):
                c = tables["ctus"][(ty0 // s) * nbw + tx0 // s]
                x0, y0, x1, y1 = _rect(int(c["border"]), tx0 & ~(s - 1), ty0 & ~(s - 1), s, pw, ph)
                inside = tx0 >= x0 + 4 and tx0 + ALF_TL + 4 <= x1 + 1 and ty0 >= y0 + halo and ty0 + ALF_TL + halo <= y1 + 1
                stores = {"8-byte" if tx0 + k + 3 < pw and not st & 3 else "scalar" for k in range(0, min(ALF_TL, pw - tx0), 4)}
                if plane == "luma":
                    on = bool(c["flags"] & 4)
                    out |= {(plane, "16-byte" if inside and not st & 7 else "clamped", sto) for sto in stores} if on else {(plane, "copy", "scalar")}
                    if on:
                        sides.add((tx0 - halo < x0, tx0 + ALF_TL + halo > x1 + 1, ty0 - halo < y0, ty0 + ALF_TL + halo > y1 + 1))
                else:
                    for comp in (1, 2):
                        on = bool(c["flags"] & (2 if comp == 1 else 1))
                        out |= {(plane, ("16-byte" if inside and not st & 7 else "clamped") if on else "none", sto) for sto in stores}
                        if c["cc_cb_idx" if comp == 1 else "cc_cr_idx"]:
                            out.add(("cc", "inside" if tx0 > x0 and ty0 > y0 and tx0 + ALF_TL <= x1 and ty0 + ALF_TL <= y1 else "clamped"))
    return out, sides
