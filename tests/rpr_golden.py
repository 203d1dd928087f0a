"""Test infrastructure: tests/golden/rpr/rpr.ovg (the reference's rcn_mcp_b / rcn_gpm_b on scaled references, written by
tools/rpr_golden/gen_rpr.c) as Python objects."""
import ctypes as C

import numpy as np

import golden_io
from spec_rpr import UNSCALED, scale_factor


def load():
    # (a directory of its own: tests/golden/*.ovg are the fixtures oracle/ref_harness/gen_golden regenerates)
    g = golden_io.load("rpr.ovg", golden_io.GOLDEN / "rpr")
    from openvvc_amd import capi
    pic_w, pic_h = (int(v) for v in g["pic"])
    sizes = [tuple(int(v) for v in s) for s in g["ref_size"]]
    refs = [(g[f"ref{i}_y"], g[f"ref{i}_cb"], g[f"ref{i}_cr"]) for i in range(len(sizes))]
    cases = []
    for k, raw in enumerate(g["desc"]):
        d = capi.PuDesc.from_buffer_copy(raw.tobytes())
        pu = {f: getattr(d, f) for f, _ in capi.PuDesc._fields_}
        w, h = 1 << d.log2_w, 1 << d.log2_h
        o = int(g["exp_off"][k])
        ey = g["exp"][o:o + w * h].reshape(h, w)
        o += w * h
        ecb = g["exp"][o:o + w * h // 4].reshape(h // 2, w // 2)
        o += w * h // 4
        ecr = g["exp"][o:o + w * h // 4].reshape(h // 2, w // 2)
        cases.append(dict(pu=pu, col=tuple(int(v) for v in g["col"][k]), exp=(ey, ecb, ecr)))
    return pic_w, pic_h, sizes, refs, cases


def scales(pic_w, pic_h, sizes, col):
    out = {}
    for i, (rw, rh) in enumerate(sizes):
        sh, sv = scale_factor(rw, pic_w), scale_factor(rh, pic_h)
        if sh == UNSCALED and sv == UNSCALED and (rw, rh) == (pic_w, pic_h):
            continue
        out[i] = dict(scale_hor=sh, scale_ver=sv, ref_w=rw, ref_h=rh, col_hor=col[0], col_ver=col[1])
    return out


def batches(cases):
    """Greedy groups of cases whose PUs do not overlap (one picture each); every group has one collocation setting."""
    left = list(range(len(cases)))
    while left:
        taken, occ, col, rest = [], [], None, []
        for i in left:
            p = cases[i]["pu"]
            r = (p["x0"], p["y0"], p["x0"] + (1 << p["log2_w"]), p["y0"] + (1 << p["log2_h"]))
            if (col is None or cases[i]["col"] == col) and all(r[2] <= o[0] or o[2] <= r[0] or r[3] <= o[1] or o[3] <= r[1] for o in occ):
                taken.append(i); occ.append(r); col = cases[i]["col"]
            else:
                rest.append(i)
        yield taken
        left = rest


def is_rpr(case, pic_w, pic_h, sizes) -> bool:
    """Does the reference take an RPR path for this case (a used list scaled)?  (GPM: always both sides.)"""
    pu = case["pu"]
    sc = scales(pic_w, pic_h, sizes, case["col"])
    d = pu["inter_dir"] & 3
    if pu["refine"]:
        d = 3
    elif d == 3 and pu["poc0"] == pu["poc1"] and pu["mv0x"] == pu["mv1x"] and pu["mv0y"] == pu["mv1y"]:
        d = 2
    used = [pu["ref1"] if l else pu["ref0"] for l in (0, 1) if d & (1 << l)]
    return any(u in sc for u in used)
