"""Test infrastructure: prediction units and scaled references for the reference-picture-resampling tests."""
import random

import numpy as np

from spec_rpr import UNSCALED, scale_factor


def ref_planes(w, h, seed):
    rng = np.random.default_rng(seed)
    # smooth content plus noise: filtered values exercise both signs of the 14-bit intermediates
    yy, xx = np.mgrid[0:h, 0:w]
    base = 512 + 300 * np.sin(xx / 7.0 + seed) * np.cos(yy / 5.0)
    y = np.clip(base + rng.integers(-200, 200, (h, w)), 0, 1023).astype(np.uint16)
    y[rng.random((h, w)) < 0.02] = 0            # isolated dark samples: negative intermediates after sharp filters
    cb = rng.integers(0, 1024, (h // 2, w // 2)).astype(np.uint16)
    cr = np.clip(cb.astype(np.int32) // 2 + 200, 0, 1023).astype(np.uint16)
    return y, cb, cr


def scales_for(pic_w, pic_h, sizes, col_flags=(0, 0)):
    """slot -> scale dict for references of the given sizes (slot i = sizes[i]); a size equal to the picture = unscaled."""
    out = {}
    for i, (rw, rh) in enumerate(sizes):
        sh, sv = scale_factor(rw, pic_w), scale_factor(rh, pic_h)
        if (rw, rh) == (pic_w, pic_h):
            continue
        out[i] = dict(scale_hor=sh, scale_ver=sv, ref_w=rw, ref_h=rh, col_hor=col_flags[0], col_ver=col_flags[1])
    return out


SHAPES = [(3, 3), (4, 3), (3, 4), (4, 4), (5, 3), (3, 5), (5, 5), (6, 6), (6, 4), (4, 6)]


def random_pus(pic_w, pic_h, n_slots, n, seed, far=False):
    """Non-overlapping PUs on a grid of 64x64 cells; bi / uni, BCW, identical motion, LMCS, mixed lists."""
    rnd = random.Random(seed)
    pus = []
    cells = [(x, y) for y in range(0, pic_h - 63, 64) for x in range(0, pic_w - 63, 64)]
    rnd.shuffle(cells)
    for (cx, cy) in cells[:n]:
        lw, lh = rnd.choice(SHAPES)
        x0 = cx + rnd.randrange(0, 64 - (1 << lw) + 1, 8)
        y0 = cy + rnd.randrange(0, 64 - (1 << lh) + 1, 8)
        span = 1 << 15 if far else 1 << 10
        d = rnd.choice([1, 2, 3, 3, 3])
        mv = [rnd.randrange(-span, span) for _ in range(4)]
        r0, r1 = rnd.randrange(n_slots), rnd.randrange(n_slots)
        ident = d == 3 and rnd.random() < 0.1
        if ident:
            mv[2:] = mv[:2]
        pus.append(dict(x0=x0, y0=y0, log2_w=lw, log2_h=lh, inter_dir=d, ref0=r0, ref1=r1, mv0x=mv[0], mv0y=mv[1], mv1x=mv[2],
                        mv1y=mv[3], bcw_idx_plus1=rnd.choice([0, 0, 1, 2, 4, 5]), poc0=r0 if ident else 10 + r0,
                        poc1=r1 if ident else 20 + r1, lmcs=int(rnd.random() < 0.3), prec_amvr_half=int(rnd.random() < 0.2)))
    return pus


def pu_desc(capi, pu):
    d = capi.PuDesc()
    d.x0, d.y0, d.log2_w, d.log2_h = pu["x0"], pu["y0"], pu["log2_w"], pu["log2_h"]
    d.inter_dir, d.bcw_idx_plus1, d.planes, d.lmcs = pu["inter_dir"], pu.get("bcw_idx_plus1", 0), 3, pu.get("lmcs", 0)
    d.prec_amvr_half = pu.get("prec_amvr_half", 0)
    d.refine, d.gpm_split_dir, d.ciip_wt = pu.get("refine", 0), pu.get("gpm_split_dir", 0), pu.get("ciip_wt", 0)
    d.mv0x, d.mv0y, d.mv1x, d.mv1y = pu["mv0x"], pu["mv0y"], pu["mv1x"], pu["mv1y"]
    d.poc0, d.poc1, d.ref0, d.ref1 = pu["poc0"], pu["poc1"], pu["ref0"], pu["ref1"]
    d.ref_idx0, d.ref_idx1 = pu["ref0"], pu["ref1"]
    return d


def lmcs_lut():
    return np.clip((np.arange(1024) * 9) // 8 - 40, 0, 1023).astype(np.uint16)
