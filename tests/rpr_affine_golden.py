"""Test infrastructure: tests/golden/rpr/rpr_affine.ovg (the reference's rcn_mcp_b_l(2,2) / rcn_prof_mcp_b_l / rcn_mcp_b_c(3,3)
driven as the affine drivers drive them, on scaled references; written by tools/rpr_golden/gen_rpr_affine.c) as Python objects.
The reference pictures are those of rpr.ovg (same sizes, same seed): stored there once, checked here by checksum."""
import ctypes as C

import numpy as np

import golden_io
import rpr_golden


def _sum31(plane) -> int:
    s = 0
    for v in plane.reshape(-1).tolist():
        s = (s * 31 + v) & 0xFFFFFFFF
    return s


def load():
    g = golden_io.load("rpr_affine.ovg", golden_io.GOLDEN / "rpr")
    from openvvc_amd import capi
    pic_w, pic_h, sizes, refs, _ = rpr_golden.load()
    assert (pic_w, pic_h) == tuple(int(v) for v in g["pic"]) and sizes == [tuple(int(v) for v in s) for s in g["ref_size"]]
    for i, planes in enumerate(refs):
        assert [_sum31(p) for p in planes] == [int(v) for v in g["ref_sum"][i]], "rpr.ovg's reference pictures are not the generator's"
    cases = []
    for k, raw in enumerate(g["desc"]):
        d = capi.AffineDesc.from_buffer_copy(raw.tobytes())
        w, h = 1 << d.log2_w, 1 << d.log2_h
        nsx, nsy = w >> 2, h >> 2
        oy, ocb, ocr, omv = (int(v) for v in g["off"][k])
        mv = g["mv"][omv:omv + 4 * nsx * nsy]
        cu = dict(x0=d.x0, y0=d.y0, log2_w=d.log2_w, log2_h=d.log2_h, inter_dir=d.inter_dir, bcw_idx_plus1=d.bcw_idx_plus1,
                  prof_dir=d.prof_dir, lmcs=d.lmcs, ref0=d.ref0, ref1=d.ref1, poc0=d.poc0, poc1=d.poc1,
                  mv0=mv[:2 * nsx * nsy].reshape(nsy, nsx, 2).copy(), mv1=mv[2 * nsx * nsy:].reshape(nsy, nsx, 2).copy(),
                  dmv_scale=np.array([[d.dmv_scale[t][i] for i in range(16)] for t in range(4)], dtype=np.int16))
        exp = (g["exp"][oy:oy + w * h].reshape(h, w), g["exp"][ocb:ocb + w * h // 4].reshape(h // 2, w // 2),
               g["exp"][ocr:ocr + w * h // 4].reshape(h // 2, w // 2))
        cases.append(dict(cu=cu, col=tuple(int(v) for v in g["col"][k]), exp=exp))
    return pic_w, pic_h, sizes, refs, cases, int(g["n_dropped"][0])


def affine_desc(capi, cu, keep):
    """ovhip_affine_desc of a case; `keep` collects the ctypes arrays the descriptor points to."""
    nsy, nsx = cu["mv0"].shape[:2]
    m0 = (C.c_int32 * (2 * nsx * nsy))(*np.asarray(cu["mv0"], dtype=np.int64).reshape(-1).tolist())
    m1 = (C.c_int32 * (2 * nsx * nsy))(*np.asarray(cu["mv1"], dtype=np.int64).reshape(-1).tolist())
    keep += [m0, m1]
    d = capi.AffineDesc(x0=cu["x0"], y0=cu["y0"], log2_w=cu["log2_w"], log2_h=cu["log2_h"], inter_dir=cu["inter_dir"],
                        bcw_idx_plus1=cu.get("bcw_idx_plus1", 0), prof_dir=cu.get("prof_dir", 0), lmcs=cu.get("lmcs", 0),
                        ref0=cu["ref0"], ref1=cu["ref1"], poc0=cu["poc0"], poc1=cu["poc1"], mv_stride=nsx,
                        mv0=C.cast(m0, C.c_void_p), mv1=C.cast(m1, C.c_void_p))
    dmv = np.asarray(cu.get("dmv_scale", np.zeros((4, 16))), dtype=np.int64)
    for t in range(4):
        for i in range(16):
            d.dmv_scale[t][i] = int(dmv[t][i])
    return d


def effective_dir(cu) -> int:
    d = cu["inter_dir"] & 3
    return 2 if d != 3 and d & 2 else d


def batches(cases):
    """Greedy groups of cases whose CUs do not overlap (one picture each); every group has one collocation setting."""
    pus = [dict(pu=dict(x0=c["cu"]["x0"], y0=c["cu"]["y0"], log2_w=c["cu"]["log2_w"], log2_h=c["cu"]["log2_h"]), col=c["col"]) for c in cases]
    return rpr_golden.batches(pus)
