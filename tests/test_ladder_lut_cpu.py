"""CPU: the output ladder through a colour table on the host (openvvc_amd/csrc/ovvc_ladder_lut.c): ovhip_ladder_lut_host against the
numpy restatement tests/spec_ladder_lut.py byte for byte on the whole census, every surface inside a sentinel buffer, at source strides w
and w + 6; the refusals with their codes, all or nothing; ovhip_ladder_lut_check against the picture-independent part of them; the
exports.  The definition is integer only: every comparison is of bytes."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import spec_ladder_lut as sx
import spec_surface as ss
from openvvc_amd import capi, engine
from test_ladder_cpu import GUARD, assert_equals_want, host_buffers, host_pic
from test_reduce_cpu import info_of

ROOT = Path(__file__).resolve().parent.parent
EINVAL, EUNSUP = capi.OVHIP_EINVAL, capi.OVHIP_EUNSUP
NEW = ["ovhip_ladder_lut_check", "ovhip_ladder_lut_host", "ovhip_ladder_lut_launch", "ovhip_pic_output_ladder_lut", "ovhip_frame_set_ladder_lut",
       "ovhip_stream_set_ladder_lut"]


def host_ladder(lib, planes, rungs, conv, table, peak, window=(0, 0, 0, 0), spad=0):
    bufs, c_rungs = host_buffers(lib, rungs)
    _src, pic = host_pic(planes, spad)
    arr, n = engine._rung_array(c_rungs)
    table = np.ascontiguousarray(table)
    r = lib.ovhip_ladder_lut_host(C.byref(pic), C.byref(info_of(window, conv[2])), arr, n, C.byref(engine.surface_conv(*conv)), table.shape[0], peak, table.ctypes.data)
    assert r == 0, (r, rungs, window, conv)
    return bufs


@pytest.mark.parametrize("case", list(sx.CENSUS))
def test_host_twin_equals_the_restatement_on_the_census(built_lib, case):
    _size, win, rungs, (_s, peak), combos = sx.CENSUS[case]
    planes, table = sx.census_planes(case), sx.census_table(case)
    for k, combo in enumerate(combos):
        assert_equals_want(host_ladder(built_lib, planes, rungs, sx.conv_of(*combo), table, peak, win), sx.census_want(case, k, GUARD), (case, combo))
    if case != "D":                                           # (the large case runs once)
        assert_equals_want(host_ladder(built_lib, planes, rungs, sx.conv_of(*combos[0]), table, peak, win, spad=6), sx.census_want(case, 0, GUARD),
                           (case, "source strides w + 6"))


def test_a_refused_ladder_writes_nothing_and_check_agrees(built_lib):
    lib = built_lib
    planes = sx.ramp_planes(72, 40, 9)
    _src, pic = host_pic(planes)
    table = sx.st.random_table(17, 1023, 5)
    good = [sx.rung(48, 24, sx.P010), sx.rung(36, 20, sx.NV12, sx.DITHER), sx.rung(72, 40, sx.I420)]
    conv = sx.conv_of(0, 0)
    bufs, c_rungs = host_buffers(lib, good)

    def run(rungs=c_rungs, n=None, info=None, p=pic, cv=conv, size=17, peak=1023, tab=table, check=None):
        """ovhip_ladder_lut_host's code; check: what ovhip_ladder_lut_check must say of the same arguments (None: the same)"""
        arr, cnt = engine._rung_array(rungs)
        cnt = cnt if n is None else n
        inf = info if info is not None else info_of(loc=cv[2] if cv is not None else 0)
        cc = C.byref(engine.surface_conv(*cv)) if cv is not None else None
        r = lib.ovhip_ladder_lut_host(C.byref(p) if p is not None else None, C.byref(inf), arr, cnt, cc, size, peak, tab.ctypes.data if tab is not None else None)
        if p is not None:
            q = lib.ovhip_ladder_lut_check(p.w, p.h, C.byref(inf), arr, cnt, cc, size, peak, None)
            assert q == (r if check is None else check), (q, r, check)
        return r

    def untouched(b=bufs):
        return all((x == ss.FILL).all() for x in b)

    # everything the ladder refuses: a ratio above 8 and an up-sampling rung in the last position, n out of range, null arguments
    far = engine.ladder_rung(8, 40, engine.surface_format(), bufs[0].ctypes.data, 1 << 20)
    up = engine.ladder_rung(144, 80, engine.surface_format(), bufs[0].ctypes.data, 1 << 20)
    assert run(c_rungs + [far]) == EUNSUP and run(c_rungs + [up]) == EUNSUP and untouched()
    assert run(n=0) == EINVAL and run(c_rungs * 3) == EINVAL and untouched()
    arr3 = engine._rung_array(c_rungs)[0]
    cc = engine.surface_conv(*conv)
    assert lib.ovhip_ladder_lut_host(None, C.byref(info_of()), arr3, 3, C.byref(cc), 17, 1023, table.ctypes.data) == EINVAL
    assert lib.ovhip_ladder_lut_host(C.byref(pic), None, arr3, 3, C.byref(cc), 17, 1023, table.ctypes.data) == EINVAL
    assert lib.ovhip_ladder_lut_host(C.byref(pic), C.byref(info_of()), None, 3, C.byref(cc), 17, 1023, table.ctypes.data) == EINVAL
    assert lib.ovhip_ladder_lut_check(72, 40, None, arr3, 3, C.byref(cc), 17, 1023, None) == EINVAL
    assert untouched()
    # what only a picture or a destination shows: the check accepts, the twin refuses
    small = list(c_rungs)
    small[2] = engine.ladder_rung(72, 40, c_rungs[2].fmt, bufs[2].ctypes.data, c_rungs[2].dst_bytes - 1)
    null = list(c_rungs)
    null[1] = engine.ladder_rung(36, 20, c_rungs[1].fmt, None, c_rungs[1].dst_bytes)
    both = np.full(c_rungs[0].dst_bytes + c_rungs[1].dst_bytes, ss.FILL, np.uint8)
    over = [engine.ladder_rung(48, 24, c_rungs[0].fmt, both.ctypes.data, c_rungs[0].dst_bytes),
            engine.ladder_rung(36, 20, c_rungs[1].fmt, both.ctypes.data + c_rungs[0].dst_bytes - 2, c_rungs[1].dst_bytes)]
    assert run(small, check=0) == EINVAL and run(null, check=0) == EINVAL and run(over, check=0) == EINVAL and untouched() and untouched([both])
    assert run(p=capi.Pic(pic.y, None, pic.cr, 72, 40, 72, 36), check=0) == EINVAL and run(p=capi.Pic(pic.y, pic.cb, pic.cr, 72, 40, 70, 36), check=0) == EINVAL
    src, p2 = host_pic(planes)
    inside = list(c_rungs)
    inside[2] = engine.ladder_rung(72, 40, c_rungs[2].fmt, src[2].ctypes.data + 2 * src[2].size - 8, c_rungs[2].dst_bytes)
    assert run(inside, p=p2, check=0) == EINVAL and untouched() and np.array_equal(src[2], planes[2])
    # what the surface output through a table refuses of a rung: a size that is a multiple of 2 only, a format
    two = engine.ladder_rung(36, 18, engine.surface_format(), bufs[1].ctypes.data, 1 << 20)
    assert run(c_rungs[:1] + [two]) == EINVAL and untouched()
    f = engine.surface_format(capi.SURF_P010)
    f.rounding = 1
    assert run([engine.ladder_rung(48, 24, f, bufs[0].ctypes.data, c_rungs[0].dst_bytes)] + c_rungs[1:]) == EINVAL and untouched()
    # the conversion's own refusals, with their codes
    assert run(cv=None) == EINVAL
    for cv, code in (((2, 0, 0, 1, 0, 0), EINVAL), ((3, 0, 0, 1, 0, 0), EUNSUP), ((9, 0, 0, 2, 0, 0), EINVAL), ((9, 0, 0, 4, 0, 0), EUNSUP), ((9, 2, 0, 1, 0, 0), EINVAL),
                     ((9, 0, 0, 1, 2, 0), EINVAL), ((9, 0, 0, 1, 0, 4), EUNSUP), ((9, 0, 0, 1, 0, 6), EINVAL)):
        assert run(cv=cv) == code, cv
    rsv = engine.surface_conv(*conv)
    rsv.rsv[1] = 1
    assert lib.ovhip_ladder_lut_host(C.byref(pic), C.byref(info_of()), arr3, 3, C.byref(rsv), 17, 1023, table.ctypes.data) == EINVAL
    assert untouched()
    # the table: null, a size or a peak that is none, an entry above the peak (the twin's alone)
    assert run(tab=None, check=0) == EINVAL and run(size=16) == EINVAL and run(peak=0) == EINVAL and run(peak=65536) == EINVAL
    assert run(peak=1022, check=0) == EINVAL and untouched()
    # two sample locations: the conversion reads another one than the ladder's reduced pictures keep
    assert run(info=info_of(loc=1)) == EINVAL and run(cv=sx.conv_of(2, 0), info=info_of(loc=0)) == EINVAL and untouched()
    assert run(cv=sx.conv_of(2, 0), info=info_of(loc=2)) == 0 and not any(untouched([b]) for b in bufs)


def test_engine_check_gives_the_ratios_and_the_conversions_location(built_lib):
    (w, h), win, rungs, (size, peak), _combos = sx.CENSUS[sx.WINDOW_CASE]
    plain = [engine.ladder_rung(g[0], g[1]) for g in rungs]
    r, ratios = engine.ladder_lut_check(w, h, plain, engine.surface_conv(*sx.conv_of(2, 1)), size, peak, win)
    assert r == 0 and ratios == [(1, 1, 1, 1), (3, 2, 5, 3), (2, 1, 2, 1)]
    assert engine.ladder_lut_check(w, h, plain, engine.surface_conv(*sx.conv_of(2, 1)), size, peak, win, chroma_loc=0)[0] == EINVAL
    assert engine.ladder_lut_check(w, h, plain, None, size, peak, win)[0] == EINVAL


def test_a_dry_frame_accepts_the_call_and_does_nothing(built_lib):
    from test_dpb_cpu import FakeMem
    lib = built_lib
    mem, h = FakeMem(), C.c_void_p()
    assert lib.ovhip_dpb_create_ex(C.byref(h), 1, C.byref(mem.ops)) == 0
    f = C.c_void_p()
    assert lib.ovhip_frame_create(h, 0, 64, 64, C.byref(f)) == 0
    conv = engine.surface_conv(*sx.conv_of(0, 0))
    fake = C.c_void_p(0x1000)                                  # (a dry frame never looks at the table)
    assert lib.ovhip_frame_set_ladder_lut(f, fake, C.byref(conv)) == 0
    assert lib.ovhip_frame_set_ladder_lut(f, fake, None) == EINVAL
    bad = engine.surface_conv(*sx.conv_of(0, 4))
    assert lib.ovhip_frame_set_ladder_lut(f, fake, C.byref(bad)) == EUNSUP
    assert lib.ovhip_frame_set_ladder_lut(None, None, None) == EINVAL and lib.ovhip_stream_set_ladder_lut(None, None, 0, 0, None) == EINVAL
    buf = np.full(4096, ss.FILL, np.uint8)
    arr, n = engine._rung_array([engine.ladder_rung(32, 32, engine.surface_format(), buf.ctypes.data, buf.nbytes)])
    assert lib.ovhip_frame_set_ladder_output(f, None, arr, n) == 0
    assert lib.ovhip_frame_begin_tag(f, C.c_void_p(0x10), 1) == 0
    p = capi.JobParams()
    assert lib.ovhip_frame_submit(f, None, None, C.byref(p), None) == 0
    assert (buf == ss.FILL).all()
    assert lib.ovhip_frame_set_ladder_lut(f, None, None) == 0
    lib.ovhip_frame_destroy(f)
    lib.ovhip_dpb_destroy(h)


def test_exports_and_abi(built_lib):
    header = (ROOT / "include" / "ovvc_hip.h").read_text()
    for name in NEW:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in capi.EXPORTED_SYMBOLS and hasattr(built_lib, name), name
    assert "Output ladder through a colour table" in header
    assert capi.OVHIP_ABI_VERSION == 9 and built_lib.ovhip_abi_version() == 9
    assert "ovhip_ladder_lut_plan_make_" not in header
