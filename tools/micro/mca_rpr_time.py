"""Affine coding units on scaled references (k_mca_rpr) beside the same CUs on references of the picture's size (k_mca, the affine
body of k_mcxa): the numbers LABBOOK quotes.

    python tools/micro/mca_rpr_time.py [N]
        a 3840x2160 picture of affine CUs (every 64x64 cell one CU of 8x8 ... 64x64, uni / bi, BCW, PROF) recorded twice: list 0 on
        a 7680x4320 reference (2:1) and list 1 on a 2560x1440 one (2/3) -> ovhip_aff_rpr_unit; both lists on 3840x2160 references
        -> ovhip_aff_unit.  Warm-up, then N (default 100) launches of ovhip_mca_rpr_launch and of ovhip_mca_launch, alternating.
        Run it under `rocprofv3 --kernel-trace --stats -d <dir> -- python ...` and read the two kernels' averages there; the unit
        counts are printed.  The host clock is not reported: it times the enqueue.
"""
import ctypes as C
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))


def main(n):
    from openvvc_amd import capi, engine
    import rpr_affine_golden as G
    from rpr_affine_cases import random_affine_cus
    from rpr_cases import scales_for
    lib = capi.load()
    pic_w, pic_h = 3840, 2160
    sizes = [(7680, 4320), (2560, 1440), (3840, 2160), (3840, 2160)]
    cus = random_affine_cus(pic_w, pic_h, 1, 10 ** 6, seed=17)
    ctx = engine.Context(0)
    rs = np.random.RandomState(5)
    refs = [ctx.upload_pic(rs.randint(0, 1024, (h, w)).astype(np.uint16), rs.randint(0, 1024, (h // 2, w // 2)).astype(np.uint16),
                           rs.randint(0, 1024, (h // 2, w // 2)).astype(np.uint16)) for w, h in sizes]
    dst = ctx.new_pic(pic_w, pic_h)
    keep, dev = [], {}
    for name, slots in (("scaled", (0, 1)), ("unscaled", (0, 1))):      # (k_mca gets refs[2:], all of the picture size)
        rec = lib.ovhip_rec_create(pic_w, pic_h)
        assert lib.ovhip_rec_set_rpr_tools(rec, capi.RPR_TOOL_AFFINE) == 0
        if name == "scaled":
            for slot, s in scales_for(pic_w, pic_h, sizes).items():
                assert capi.set_ref_scale(lib, rec, slot, s["scale_hor"], s["scale_ver"], s["ref_w"], s["ref_h"], 0, 0) == 0
        for cu in cus:
            assert lib.ovhip_rec_affine_cu(rec, C.byref(G.affine_desc(capi, dict(cu, ref0=slots[0], ref1=slots[1], lmcs=0), keep))) > 0
        arrs = []
        for fn, elem in (("ovhip_rec_aff_rpr_units" if name == "scaled" else "ovhip_rec_aff_units", 48 if name == "scaled" else 32),
                         ("ovhip_rec_aff_side", 4)):
            cnt = C.c_size_t(0)
            p = getattr(lib, fn)(rec, C.byref(cnt))
            d = ctx.upload(np.frombuffer(C.string_at(p, cnt.value * elem), dtype=np.uint8))
            d.count = cnt.value
            arrs.append(d)
        dev[name] = arrs
        lib.ovhip_rec_destroy(rec)
    print(f"{len(cus)} affine CUs of a {pic_w}x{pic_h} picture: {dev['scaled'][0].count} ovhip_aff_rpr_unit (k_mca_rpr; list 0 from "
          f"{sizes[0][0]}x{sizes[0][1]}, list 1 from {sizes[1][0]}x{sizes[1][1]}), {dev['unscaled'][0].count} ovhip_aff_unit (k_mca); {n} launches each")
    for i in range(5 + n):
        ctx.mca_rpr(dst, refs, dev["scaled"][0], dev["scaled"][1])
        ctx.mca(dst, refs[2:], dev["unscaled"][0], dev["unscaled"][1])
    ctx.sync()
    ctx.close()


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 100)
