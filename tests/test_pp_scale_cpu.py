"""CPU: output resampling (include/ovvc_hip.h, "Output resampling").  The numpy restatement (tests/spec_pp_scale.py) against what the
reference's pp_sample_rate_conv wrote (tests/golden/pp_scale/*.ovg, tools/pp_scale_golden/gen_pp_scale.c), the host half of the
argument check (ovhip_output_scale_check) against the restatement, and the frame-level setter on a dry frame.
tests/test_gpu_pp_scale.py runs the kernel."""
import ctypes as C

import numpy as np
import pytest

import spec_pp_scale as sp
from openvvc_amd import capi

CASES = sp.load_cases()


def lib_check(lib, src_w, src_h, win, col, dst_w, dst_h):
    info = capi.ScaleInfo(*win, *col)
    scale = (C.c_int32 * 4)()
    r = lib.ovhip_output_scale_check(src_w, src_h, C.byref(info), dst_w, dst_h, C.byref(scale))
    return r, [int(v) for v in scale]


def test_fixture_is_the_eleven_shapes():
    shapes = [(c["src_w"], c["src_h"], c["dst_w"], c["dst_h"], c["win"]) for c in CASES]
    assert shapes == [(64, 48, 128, 96, (0, 0, 0, 0)), (96, 64, 144, 96, (0, 0, 0, 0)), (80, 48, 104, 72, (0, 0, 0, 0)),
                      (176, 144, 352, 288, (0, 0, 0, 0)), (72, 40, 72, 40, (0, 0, 0, 0)), (64, 64, 128, 64, (0, 0, 0, 0)),
                      (64, 64, 64, 96, (0, 0, 0, 0)), (96, 80, 160, 136, (1, 2, 1, 0)), (120, 72, 128, 80, (2, 0, 0, 1)),
                      (8, 8, 16, 16, (0, 0, 0, 0)), (208, 120, 416, 240, (0, 0, 0, 0))]
    # both values of each collocation flag; both clip bounds bind somewhere
    assert {c["col"][0] for c in CASES} == {0, 1} and {c["col"][1] for c in CASES} == {0, 1}
    assert any(int(e.max()) == 1023 for c in CASES for e in c["exp"]) and any(int(e.min()) == 0 for c in CASES for e in c["exp"])
    for c in CASES:
        for p in range(3):
            d = 2 if p else 1
            assert c["src"][p].shape == (c["src_h"] // d, c["src_w"] // d) and c["exp"][p].shape == (c["dst_h"] // d, c["dst_w"] // d)


@pytest.mark.parametrize("k", range(len(CASES)))
def test_restatement_equals_the_reference(k):
    c = CASES[k]
    assert sp.is_upsampling(c["src_w"], c["src_h"], c["win"], c["col"], c["dst_w"], c["dst_h"])
    got = sp.scale_picture(*c["src"], c["dst_w"], c["dst_h"], c["win"], c["col"])
    for p, name in enumerate(("Y", "Cb", "Cr")):
        assert got[p].tobytes() == c["exp"][p].tobytes(), (k, name)


def test_the_phase_is_the_low_bits_of_the_position():
    """the quirk, stated: at 2:1 every luma phase is 0; at 3:2, 60 of the first 64 luma columns have a non-zero phase"""
    for ow, sw, want in ((64, 128, 0), (96, 144, 60)):
        scale = (ow << 13) // sw
        ph = (np.arange(64) * scale) & 15
        assert int(np.count_nonzero(ph)) == want


def test_check_returns_the_scale_factors(built_lib):
    for c in CASES:
        r, scale = lib_check(built_lib, c["src_w"], c["src_h"], c["win"], c["col"], c["dst_w"], c["dst_h"])
        want = sp.check(c["src_w"], c["src_h"], c["win"], c["col"], c["dst_w"], c["dst_h"])
        assert (r, scale) == (sp.OK, want[1]), c["idx"]
    # sizes people use
    for (sw, sh), (dw, dh) in (((1920, 1080), (3840, 2160)), ((2560, 1440), (3840, 2160)), ((1280, 720), (1920, 1080)), ((3840, 2160), (3840, 2160))):
        r, scale = lib_check(built_lib, sw, sh, (0, 0, 0, 0), (0, 0), dw, dh)
        assert (r, scale) == sp.check(sw, sh, (0, 0, 0, 0), (0, 0), dw, dh) and r == sp.OK


def test_check_refuses(built_lib):
    none = (0, 0, 0, 0)
    # down-sampling, and one axis up with the other down
    assert lib_check(built_lib, 128, 96, none, (0, 0), 64, 48)[0] == capi.OVHIP_EUNSUP == sp.check(128, 96, none, (0, 0), 64, 48)[0]
    assert lib_check(built_lib, 64, 96, none, (0, 0), 128, 48)[0] == capi.OVHIP_EUNSUP
    assert lib_check(built_lib, 128, 48, none, (1, 1), 64, 96)[0] == capi.OVHIP_EUNSUP
    # a scaling window that leaves nothing: luma extra = (16 + 16) << 2 = 128 >= 128
    assert lib_check(built_lib, 128, 96, (16, 16, 0, 0), (0, 0), 256, 192)[0] == capi.OVHIP_EINVAL == sp.check(128, 96, (16, 16, 0, 0), (0, 0), 256, 192)[0]
    assert lib_check(built_lib, 128, 96, (0, 0, 12, 12), (0, 0), 256, 192)[0] == capi.OVHIP_EINVAL
    # sizes that are not multiples of 4, empty sizes, missing arguments
    for bad in ((66, 48, 128, 96), (64, 50, 128, 96), (64, 48, 130, 96), (64, 48, 128, 98), (0, 48, 128, 96), (64, 48, 0, 0), (64, 48, -128, 96)):
        assert lib_check(built_lib, bad[0], bad[1], none, (0, 0), bad[2], bad[3])[0] == capi.OVHIP_EINVAL, bad
    scale = (C.c_int32 * 4)()
    assert built_lib.ovhip_output_scale_check(64, 48, None, 128, 96, C.byref(scale)) == capi.OVHIP_EINVAL
    # a window that turns a larger source into up-sampling is accepted (the factor is taken over the window)
    assert lib_check(built_lib, 144, 96, (4, 4, 0, 0), (0, 0), 128, 96)[0] == sp.OK


def test_launch_refuses_without_a_context(built_lib):
    info = capi.ScaleInfo()
    a, b = capi.Pic(), capi.Pic()
    assert built_lib.ovhip_output_scale_launch(None, C.byref(a), C.byref(info), C.byref(b)) == capi.OVHIP_EINVAL
    out = (C.c_uint8 * 16)()
    assert built_lib.ovhip_pic_digest_scaled(None, C.byref(a), C.byref(info), 64, 64, None, out) == capi.OVHIP_EINVAL
    assert built_lib.ovhip_pic_output_scaled(None, C.byref(a), C.byref(info), 64, 64, None, out) == capi.OVHIP_EINVAL
    assert built_lib.ovhip_frame_set_output_scale(None, 64, 64, None) == capi.OVHIP_EINVAL
    assert built_lib.ovhip_stream_set_output_scale(None, 64, 64, None) == capi.OVHIP_EINVAL


def test_dry_frame_accepts_the_output_scale(built_lib):
    """a DPB on a counting memory back-end (no device): the setter is accepted, the picture is submitted and published as before"""
    from test_dpb_cpu import FakeMem
    lib = built_lib
    mem, h = FakeMem(), C.c_void_p()
    assert lib.ovhip_dpb_create_ex(C.byref(h), 1, C.byref(mem.ops)) == 0
    f = C.c_void_p()
    assert lib.ovhip_frame_create(h, 0, 64, 64, C.byref(f)) == 0
    info = capi.ScaleInfo(0, 0, 0, 0, 1, 0)
    assert lib.ovhip_frame_set_output_scale(f, 128, 128, C.byref(info)) == 0
    assert lib.ovhip_frame_set_output_scale(f, 128, 128, None) == 0
    assert lib.ovhip_frame_begin_tag(f, C.c_void_p(0x10), 1) == 0
    p = capi.JobParams()
    out = capi.FrameOutput()
    out.mode = capi.OUT_DIGEST
    assert lib.ovhip_frame_submit(f, None, None, C.byref(p), C.byref(out)) == 0
    assert bytes(out.digest) == bytes(16)                                       # dry: no output
    dev, pic = C.c_int(-1), capi.Pic()
    assert lib.ovhip_dpb_lookup(h, C.c_void_p(0x10), C.byref(dev), C.byref(pic)) == 0 and (pic.w, pic.h) == (64, 64)
    assert lib.ovhip_frame_set_output_scale(f, 0, 0, None) == 0
    lib.ovhip_frame_destroy(f)
    lib.ovhip_dpb_destroy(h)
