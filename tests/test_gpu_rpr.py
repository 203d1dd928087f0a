"""GPU: prediction from references of another size (reference picture resampling) through the recorder and
ovhip_mc_rpr_launch is bit-exact with the numpy restatement of the reference (tests/spec_rpr.py), PU by PU, for a
1920x1080 B picture predicting from references of 3840x2160, 2880x1620, 1280x720 and 960x540 plus one unscaled
reference, and for a size-changing sequence (1920x1080 -> 960x540 from it -> 1920x1080 from both)."""
import ctypes as C

import numpy as np
import pytest

from openvvc_amd import capi, engine
import spec_rpr as S
from rpr_cases import lmcs_lut, pu_desc, random_pus, ref_planes, scales_for

pytestmark = pytest.mark.gpu


def _run(ctx, pic_w, pic_h, refs_np, scales, pus, lut):
    lib = capi.load()
    rec = lib.ovhip_rec_create(pic_w, pic_h)
    try:
        for slot, s in scales.items():
            assert capi.set_ref_scale(lib, rec, slot, s["scale_hor"], s["scale_ver"], s["ref_w"], s["ref_h"],
                                      s["col_hor"], s["col_ver"]) == 0
        kept = []
        for pu in pus:
            before = len(capi.rpr_units(lib, rec))
            assert lib.ovhip_rec_pu(rec, C.byref(pu_desc(capi, pu))) > 0
            if len(capi.rpr_units(lib, rec)) > before:
                kept.append(pu)
        units = capi.rpr_units(lib, rec)
    finally:
        lib.ovhip_rec_destroy(rec)
    assert len(kept) > 20
    arr = np.frombuffer(bytes((capi.RprUnit * len(units))(*units)), dtype=np.uint8)
    d_units = ctx.upload(arr)
    d_units.count = len(units)
    d_lut = ctx.upload(lut)
    refs = [ctx.upload_pic(*refs_np[i]) for i in range(len(refs_np))]
    dst = ctx.new_pic(pic_w, pic_h)
    ctx.mc_rpr(dst, refs, d_units, d_lut)
    ctx.sync()
    y, cb, cr = dst.download()
    for pu in kept:
        ey, ecb, ecr = S.predict_pu(refs_np, scales, pic_w, pic_h, pu, lut)
        x0, y0, pw, ph = pu["x0"], pu["y0"], 1 << pu["log2_w"], 1 << pu["log2_h"]
        assert np.array_equal(y[y0:y0 + ph, x0:x0 + pw], ey), pu
        assert np.array_equal(cb[y0 // 2:(y0 + ph) // 2, x0 // 2:(x0 + pw) // 2], ecb), pu
        assert np.array_equal(cr[y0 // 2:(y0 + ph) // 2, x0 // 2:(x0 + pw) // 2], ecr), pu
    for p in refs + [dst]:
        ctx.lib.ovhip_pic_free(ctx.h, C.byref(p.s))
    d_units.free()
    d_lut.free()
    return len(units)


@pytest.fixture(scope="module")
def ctx():
    c = engine.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("far,cols", [(False, (0, 0)), (True, (1, 1))])
def test_b_picture_from_four_sizes(ctx, far, cols):
    pic_w, pic_h = 1920, 1080
    sizes = [(3840, 2160), (2880, 1620), (1280, 720), (960, 540), (1920, 1080)]
    refs_np = [ref_planes(w, h, 11 + i) for i, (w, h) in enumerate(sizes)]
    scales = scales_for(pic_w, pic_h, sizes, cols)
    n = _run(ctx, pic_w, pic_h, refs_np, scales, random_pus(pic_w, pic_h, len(sizes), 160, seed=21 + far, far=far), lmcs_lut())
    assert n > 100


def test_ratios_at_the_limits(ctx):
    # 2 (upper limit), just above 7/4, 3/2, exactly 5/4 and one step above, 2/3, 1/8 (lower limit)
    pic_w, pic_h = 640, 384
    sizes = [(1280, 768), (1128, 676), (960, 576), (800, 480), (802, 482), (428, 256), (80, 48), (640, 384)]
    refs_np = [ref_planes(w, h, 40 + i) for i, (w, h) in enumerate(sizes)]
    scales = scales_for(pic_w, pic_h, sizes)
    _run(ctx, pic_w, pic_h, refs_np, scales, random_pus(pic_w, pic_h, len(sizes), 60, seed=5, far=True), lmcs_lut())


def test_size_changing_sequence(ctx):
    # 1920x1080 -> 960x540 predicting from it -> 1920x1080 predicting from both
    big = ref_planes(1920, 1080, 3)
    scales = scales_for(960, 540, [(1920, 1080)])
    pus = random_pus(960, 540, 1, 60, seed=8)
    lib = capi.load()
    small = [np.zeros((540, 960), np.uint16), np.zeros((270, 480), np.uint16), np.zeros((270, 480), np.uint16)]
    # picture 2 is the restatement's prediction of picture 1 where the units land (the rest stays as allocated: zeros)
    for pu in pus:
        ey, ecb, ecr = S.predict_pu([big], scales, 960, 540, pu, None)
        x0, y0, pw, ph = pu["x0"], pu["y0"], 1 << pu["log2_w"], 1 << pu["log2_h"]
        small[0][y0:y0 + ph, x0:x0 + pw] = ey
        small[1][y0 // 2:(y0 + ph) // 2, x0 // 2:(x0 + pw) // 2] = ecb
        small[2][y0 // 2:(y0 + ph) // 2, x0 // 2:(x0 + pw) // 2] = ecr
    _run(ctx, 960, 540, [big], scales, pus, lmcs_lut())
    scales3 = scales_for(1920, 1080, [(1920, 1080), (960, 540)])
    _run(ctx, 1920, 1080, [big, tuple(small)], scales3, random_pus(1920, 1080, 2, 120, seed=9), lmcs_lut())
