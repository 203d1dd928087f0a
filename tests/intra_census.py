"""What the intra slot fixtures (tests/golden/intra.ovg, intra_cells_*.ovg) reach: every case labelled with kind, shape, mode,
neighbour-availability class and MRL index, and the counting test_oracle_golden.py asserts.

Availability classes: 0 none; 1 above only; 2 left only; 3 both without the corner; 4 both with the corner."""
import numpy as np

import oracle_lib
from oracle_lib import HostPic
from openvvc_amd import capi

LUMA, MRL, MIP, CHROMA, LM, BDPCM = range(6)
KIND_NAMES = ("luma regular", "MRL", "MIP", "chroma regular", "LM / MDLM", "BDPCM")
CLASS_NAMES = ("none", "above only", "left only", "both without corner", "both with corner")
LUMA_SHAPES = [(a, b) for a in range(2, 7) for b in range(2, 7)]                              # (log2_w, log2_h): 25
CHROMA_SHAPES = [(a, b) for a in range(1, 6) for b in range(1, 6) if a + b >= 3]              # 24: no 2x2
CTU_X, CTU_Y = 128, 128         # the fixtures' CTU in the picture (luma)


def mip_matrices(l2w, l2h):
    """matrices of a MIP block: the standard's size classes (4x4: 16; 4xN, Nx4 and 8x8: 8; the others: 6), each also transposed"""
    return 16 if (l2w, l2h) == (2, 2) else 8 if (l2w == 2 or l2h == 2 or (l2w, l2h) == (3, 3)) else 6


def mip_cells():
    return {(s, m, tr) for s in LUMA_SHAPES for m in range(mip_matrices(*s)) for tr in (0, 1)}


def label(tasks):
    """-> dict of int arrays: kind, l2w, l2h, mode (MIP: matrix), tr (MIP transposed), cls, mrl, samples (of the block)"""
    fl = tasks["flags"].astype(np.int64)
    luma = tasks["kind"] == capi.IT_LUMA
    mip = (fl & capi.IF_MIP) != 0
    kind = np.where(mip, MIP, np.where((fl & capi.IF_BDPCM) != 0, BDPCM, np.where(luma & (tasks["mrl_idx"] > 0), MRL,
                    np.where(luma, LUMA, np.where(tasks["mode"] >= 67, LM, CHROMA)))))
    abv, lft, corner = tasks["avl_abv"] > 0, tasks["avl_lft"] > 0, (fl & capi.IF_CORNER) != 0
    cls = np.where(abv & lft, np.where(corner, 4, 3), np.where(abv, 1, np.where(lft, 2, 0)))
    return dict(kind=kind, l2w=tasks["log2_w"].astype(int), l2h=tasks["log2_h"].astype(int), mode=tasks["mode"].astype(int),
                tr=((fl & capi.IF_MIP_TR) != 0).astype(int), cls=cls, mrl=np.where(kind == MRL, tasks["mrl_idx"], 0).astype(int),
                samples=1 << (tasks["log2_w"].astype(int) + tasks["log2_h"].astype(int)))


def cells(lb, kind, *keys):
    """the set of tuples over `keys` (names of label()'s arrays; "shape" = (l2w, l2h)) among the cases of `kind`"""
    sel = np.nonzero(lb["kind"] == kind)[0]
    cols = [list(zip(lb["l2w"][sel].tolist(), lb["l2h"][sel].tolist())) if k == "shape" else lb[k][sel].tolist() for k in keys]
    return set(zip(*cols))


def modes_per_shape(lb, kind):
    out = {}
    for s, m in cells(lb, kind, "shape", "mode"):
        out[s] = out.get(s, 0) + 1
    return out


def with_full_availability(tasks):
    """The same tasks with both arms as long as the fixtures' geometry lets them be and the corner: what gen_intra's max_abv / max_lft
    are for the block's position (the picture holds 192 luma columns from the CTU's left edge and its 128 rows)."""
    t = tasks.copy()
    chroma = t["kind"] != capi.IT_LUMA
    unit, sx, sy = np.where(chroma, 2, 4), np.where(chroma, 96, 192), np.where(chroma, 64, 128)
    w, h = 1 << t["log2_w"].astype(int), 1 << t["log2_h"].astype(int)
    x0 = t["x"].astype(int) - np.where(chroma, CTU_X // 2, CTU_X)
    y0 = t["y"].astype(int) - np.where(chroma, CTU_Y // 2, CTU_Y)
    abv, lft = np.minimum(2 * w // unit, (sx - x0) // unit), np.minimum(2 * h // unit, (sy - y0) // unit)
    # LM / MDLM carry their own availability: "any unit" flags, MDLM the contiguous units over w + min(w, h) (h + min(w, h)) samples
    lm = chroma & (t["mode"] >= 67)
    m = np.minimum(w, h)
    abv = np.where(lm, np.where(t["mode"] == 69, np.minimum(abv, (w + m) // 2), 1), abv)
    lft = np.where(lm, np.where(t["mode"] == 68, np.minimum(lft, (h + m) // 2), 1), lft)
    t["avl_abv"], t["avl_lft"] = abv, lft
    t["flags"] |= capi.IF_CORNER
    return t


def expected_block(tt, eo, exp):
    w, h = 1 << int(tt["log2_w"]), 1 << int(tt["log2_h"])
    if tt["kind"] == capi.IT_LUMA:
        return (exp[eo[0]:eo[0] + w * h].reshape(h, w),)
    return exp[eo[0]:eo[0] + w * h].reshape(h, w), exp[eo[1]:eo[1] + w * h].reshape(h, w)


def oracle_block(pic, tt):
    """the oracle's prediction of ONE task on a copy of the picture pic = (y, cb, cr) -> the block(s) it wrote"""
    H, W = pic[0].shape
    hp = HostPic(W, H, pic[0].copy(), pic[1].copy(), pic[2].copy())
    oracle_lib.intra_tasks(hp, np.array([tt], dtype=capi.ITASK_DTYPE))
    w, h, x, y = 1 << int(tt["log2_w"]), 1 << int(tt["log2_h"]), int(tt["x"]), int(tt["y"])
    if tt["kind"] == capi.IT_LUMA:
        return (hp.y[y:y + h, x:x + w],)
    return hp.cb[y:y + h, x:x + w], hp.cr[y:y + h, x:x + w]


def blocks_equal(a, b):
    return all(np.array_equal(p, q) for p, q in zip(a, b))


def sensitive(tasks, exp_off, exp, pic, sel):
    """For the cases sel (indices): does the reference's block differ from the oracle's prediction of the same task with full
    availability?  -> bool array over sel.  A case that does not differ pins nothing about the availability logic."""
    full = with_full_availability(tasks[sel])
    return np.array([not blocks_equal(expected_block(tasks[i], exp_off[i], exp), oracle_block(pic, full[k])) for k, i in enumerate(sel)], bool)
