"""CPU: the output ladder on the host (openvvc_amd/csrc/ovvc_ladder.c): ovhip_ladder_host against the numpy restatement
tests/spec_ladder.py byte for byte on the whole census, every surface inside a sentinel buffer; each rung against
ovhip_surface_host(ovhip_output_reduce_host(...)); the ratios of ovhip_ladder_check; the refusals, all or nothing; the exports.  The
definition is integer only: every comparison is of bytes."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import spec_ladder as sl
import spec_reduce as sd
import spec_surface as ss
from openvvc_amd import capi, engine
from test_reduce_cpu import info_of, strided

ROOT = Path(__file__).resolve().parent.parent
EINVAL, EUNSUP = capi.OVHIP_EINVAL, capi.OVHIP_EUNSUP
GUARD = 16                                                    # bytes behind a surface that must stay as they were
NEW = ["ovhip_ladder_check", "ovhip_ladder_host", "ovhip_ladder_launch", "ovhip_pic_output_ladder", "ovhip_frame_set_ladder_output",
       "ovhip_stream_set_ladder_output"]


def c_format(fmt, rounding, lay):
    return engine.surface_format(fmt, rounding, **lay)


def sizes_of(lib, rungs):
    """the bytes of every rung's surface by ovhip_surface_bytes"""
    return [lib.ovhip_surface_bytes(w, h, None, C.byref(c_format(fmt, rounding, lay))) for (w, h, fmt, rounding, lay) in rungs]


def host_buffers(lib, rungs, guard=GUARD):
    """per rung a buffer of its surface's size + guard that holds the sentinel, and the C rungs that point at them"""
    bufs = [np.full(n + guard, ss.FILL, np.uint8) for n in sizes_of(lib, rungs)]
    c_rungs = [engine.ladder_rung(w, h, c_format(fmt, rounding, lay), b.ctypes.data, b.nbytes - guard) for (w, h, fmt, rounding, lay), b in zip(rungs, bufs)]
    return bufs, c_rungs


def host_pic(planes, spad=0):
    """(the strided copies, which must stay alive, and the capi.Pic over them)"""
    h, w = planes[0].shape
    src = strided(planes, w + spad, w // 2 + spad)
    return src, capi.Pic(src[0].ctypes.data, src[1].ctypes.data, src[2].ctypes.data, w, h, w + spad, w // 2 + spad)


def host_ladder(lib, planes, rungs, window=(0, 0, 0, 0), loc=0, spad=0):
    bufs, c_rungs = host_buffers(lib, rungs)
    _src, pic = host_pic(planes, spad)
    arr, n = engine._rung_array(c_rungs)
    r = lib.ovhip_ladder_host(C.byref(pic), C.byref(info_of(window, loc)), arr, n)
    assert r == 0, (r, rungs, window, loc)
    return bufs


def assert_equals_want(got, want, what):
    """got: the buffers, surface and guard; want: spec_ladder.ladder(..., guard=GUARD): gaps, the bytes behind the last row and the
    guard all hold the sentinel there"""
    assert len(got) == len(want)
    for k, (g, (x, size)) in enumerate(zip(got, want)):
        assert g.nbytes == size + GUARD, (what, k, "ovhip_surface_bytes against the restatement's size")
        assert g.tobytes() == x.tobytes(), (what, k)


@pytest.mark.parametrize("case", range(len(sl.CENSUS)))
def test_host_twin_equals_the_restatement_on_the_census(built_lib, case):
    _size, win, rungs, locs = sl.CENSUS[case]
    planes = sl.census_planes(case)
    for loc in locs:
        assert_equals_want(host_ladder(built_lib, planes, rungs, win, loc), sl.census_want(case, loc, GUARD), (case, loc))
    assert_equals_want(host_ladder(built_lib, planes, rungs, win, locs[0], spad=6), sl.census_want(case, locs[0], GUARD), (case, "source strides w + 6"))
    if case == sl.WINDOW_CASE:
        inner = sl.window_planes()[1]
        assert_equals_want(host_ladder(built_lib, planes, rungs, win), sl.ladder(inner, rungs, guard=GUARD), "nothing outside the window is read")


@pytest.mark.parametrize("case", [0, 1, 5, 7])
def test_each_rung_equals_the_surface_twin_of_the_reduce_twin(built_lib, case):
    lib = built_lib
    (w, h), win, rungs, locs = sl.CENSUS[case]
    planes = sl.census_planes(case)
    loc = locs[-1]
    got = host_ladder(lib, planes, rungs, win, loc)
    _src, pic = host_pic(planes)
    for k, (Wd, Hd, fmt, rounding, lay) in enumerate(rungs):
        red = [np.zeros((Hd, Wd), np.uint16), np.zeros((Hd // 2, Wd // 2), np.uint16), np.zeros((Hd // 2, Wd // 2), np.uint16)]
        rp = capi.Pic(red[0].ctypes.data, red[1].ctypes.data, red[2].ctypes.data, Wd, Hd, Wd, Wd // 2)
        assert lib.ovhip_output_reduce_host(C.byref(pic), C.byref(info_of(win, loc)), C.byref(rp)) == 0
        one = np.full(got[k].nbytes, ss.FILL, np.uint8)
        f = c_format(fmt, rounding, lay)
        assert lib.ovhip_surface_host(red[0].ctypes.data, red[1].ctypes.data, red[2].ctypes.data, Wd, Hd, Wd, Wd // 2, None, C.byref(f),
                                      one.ctypes.data, one.nbytes - GUARD) == 0
        assert one.tobytes() == got[k].tobytes(), (case, k)


def test_check_returns_the_ratios_of_every_rung(built_lib):
    pairs = list(sd.RATIOS.items())
    for at in range(0, len(pairs), sl.MAX_RUNGS):
        by_src = {}
        for (src, dst), want in pairs[at:at + sl.MAX_RUNGS]:
            by_src.setdefault(src, []).append((dst, want))
        for src, rows in by_src.items():
            r, ratios = engine.ladder_check(*src, [engine.ladder_rung(*dst) for dst, _ in rows])
            assert r == 0 and ratios == [want for _, want in rows], (src, rows)
    (w, h), win, rungs, _locs = sl.CENSUS[sl.WINDOW_CASE]
    r, ratios = engine.ladder_check(w, h, [engine.ladder_rung(g[0], g[1]) for g in rungs], win)
    assert r == 0 and ratios == [(1, 1, 1, 1), (3, 2, 5, 3), (2, 1, 2, 1)]
    # a refused rung: its own ratios where they can be derived, zeros behind it
    r, ratios = engine.ladder_check(72, 40, [engine.ladder_rung(36, 20), engine.ladder_rung(8, 40), engine.ladder_rung(48, 24)])
    assert r == EUNSUP and ratios == [(2, 1, 2, 1), (9, 1, 1, 1), (0, 0, 0, 0)]
    assert built_lib.ovhip_ladder_check(72, 40, C.byref(info_of()), engine._rung_array([engine.ladder_rung(36, 20)])[0], 1, None) == 0


def test_a_refused_ladder_writes_nothing(built_lib):
    lib = built_lib
    planes = sd.random_planes(72, 40, 9)
    _src, pic = host_pic(planes)
    good = [sl.rung(48, 24, sl.P010), sl.rung(36, 20, sl.NV12, sl.DITHER), sl.rung(72, 40, sl.I420)]

    def run(c_rungs, n=None, info=None, p=pic):
        arr, cnt = engine._rung_array(c_rungs)
        return lib.ovhip_ladder_host(C.byref(p) if p is not None else None, C.byref(info if info is not None else info_of()), arr, cnt if n is None else n)

    def untouched(bufs):
        return all((b == ss.FILL).all() for b in bufs)

    # a rung the reduced-size output refuses, in the last position: every earlier rung's destination stays as it was
    for (src, dst), code in zip(sd.REFUSED, (EUNSUP, EUNSUP)):
        big = sd.random_planes(*src, 1)
        _keep, bp = host_pic(big)
        first = [sl.rung(src[0], src[1], sl.NV12), sl.rung(src[0], src[1] // 2, sl.I010)]
        bufs, c_rungs = host_buffers(lib, first)
        bad = engine.ladder_rung(dst[0], dst[1], engine.surface_format(), bufs[0].ctypes.data, 1 << 20)       # (never looked at: the ratio refuses first)
        assert run(c_rungs + [bad], p=bp) == code and untouched(bufs), (src, dst)
        assert engine.ladder_check(*src, c_rungs + [bad])[0] == code
    bufs, c_rungs = host_buffers(lib, good)
    up = engine.ladder_rung(144, 80, engine.surface_format(), bufs[0].ctypes.data, 1 << 20)
    assert run(c_rungs + [up]) == EUNSUP and untouched(bufs)
    odd = engine.ladder_rung(34, 20, engine.surface_format(), bufs[0].ctypes.data, 1 << 20)
    assert run(c_rungs + [odd]) == EINVAL and untouched(bufs)
    # n = 0 and n = max + 1; null arguments
    assert run(c_rungs, n=0) == EINVAL and untouched(bufs)
    nine_bufs, nine = host_buffers(lib, [sl.rung(36, 20)] * (sl.MAX_RUNGS + 1))
    assert run(nine) == EINVAL and untouched(nine_bufs)
    assert run(nine[:sl.MAX_RUNGS]) == 0 and not untouched(nine_bufs[:sl.MAX_RUNGS]) and untouched(nine_bufs[sl.MAX_RUNGS:])
    assert engine.ladder_check(72, 40, [])[0] == EINVAL and engine.ladder_check(72, 40, [engine.ladder_rung(36, 20)] * (sl.MAX_RUNGS + 1))[0] == EINVAL
    assert lib.ovhip_ladder_host(None, C.byref(info_of()), engine._rung_array(c_rungs)[0], 3) == EINVAL
    assert lib.ovhip_ladder_host(C.byref(pic), None, engine._rung_array(c_rungs)[0], 3) == EINVAL
    assert lib.ovhip_ladder_host(C.byref(pic), C.byref(info_of()), None, 3) == EINVAL
    assert lib.ovhip_ladder_check(72, 40, None, engine._rung_array(c_rungs)[0], 3, None) == EINVAL
    assert lib.ovhip_ladder_check(72, 40, C.byref(info_of()), None, 3, None) == EINVAL
    # a destination too small by one byte, in the last rung; a null destination
    for k in (2, 0):
        small = list(c_rungs)
        small[k] = engine.ladder_rung(good[k][0], good[k][1], c_rungs[k].fmt, bufs[k].ctypes.data, c_rungs[k].dst_bytes - 1)
        assert run(small) == EINVAL and untouched(bufs), k
    null = list(c_rungs)
    null[1] = engine.ladder_rung(36, 20, c_rungs[1].fmt, None, c_rungs[1].dst_bytes)
    assert run(null) == EINVAL and untouched(bufs)
    # two rungs' destinations overlapping one another: the same address, and a last byte shared with the next rung's first
    both = np.full(c_rungs[0].dst_bytes + c_rungs[1].dst_bytes, ss.FILL, np.uint8)
    for at in (0, c_rungs[0].dst_bytes - 2):
        over = [engine.ladder_rung(48, 24, c_rungs[0].fmt, both.ctypes.data, c_rungs[0].dst_bytes),
                engine.ladder_rung(36, 20, c_rungs[1].fmt, both.ctypes.data + at, c_rungs[1].dst_bytes)]
        assert run(over) == EINVAL and untouched([both]), at
    over[1] = engine.ladder_rung(36, 20, c_rungs[1].fmt, both.ctypes.data + c_rungs[0].dst_bytes, c_rungs[1].dst_bytes)
    assert run(over) == 0 and not untouched([both])                                            # (behind one another: accepted)
    # a destination that overlaps the picture
    src, p2 = host_pic(planes)
    inside = list(c_rungs)
    inside[2] = engine.ladder_rung(72, 40, c_rungs[2].fmt, src[2].ctypes.data + 2 * src[2].size - 8, c_rungs[2].dst_bytes)
    assert run(inside, p=p2) == EINVAL and untouched(bufs) and np.array_equal(src[2], planes[2])
    # a format's own refusals, non-zero reserved bytes in the format and in the info, a window that leaves nothing, chroma_loc 6
    for spoil in ("format", "rounding16", "fmt_rsv", "pitch"):
        bad = list(c_rungs)
        f = engine.surface_format(capi.SURF_P010)
        if spoil == "format":
            f.format = 4
        elif spoil == "rounding16":
            f.rounding = 1
        elif spoil == "fmt_rsv":
            f.rsv[1] = 1
        else:
            f.pitch_y = 48 * 2 - 2
        bad[0] = engine.ladder_rung(48, 24, f, bufs[0].ctypes.data, c_rungs[0].dst_bytes)
        assert run(bad) == EINVAL and untouched(bufs), spoil
        assert engine.ladder_check(72, 40, bad)[0] == EINVAL, spoil
    rsv = info_of()
    rsv.rsv[0] = 1
    assert run(c_rungs, info=rsv) == EINVAL and run(c_rungs, info=info_of((18, 18, 0, 0))) == EINVAL and run(c_rungs, info=info_of(loc=6)) == EINVAL
    # a missing plane, a stride below the width
    assert run(c_rungs, p=capi.Pic(pic.y, None, pic.cr, 72, 40, 72, 36)) == EINVAL and run(c_rungs, p=capi.Pic(pic.y, pic.cb, pic.cr, 72, 40, 70, 36)) == EINVAL
    assert untouched(bufs)
    assert run(c_rungs) == 0 and not any(untouched([b]) for b in bufs)


def test_a_dry_frame_accepts_the_call_and_does_nothing(built_lib):
    """a DPB on a counting memory back-end (no device): the setter is accepted, the picture is submitted and published as before"""
    from test_dpb_cpu import FakeMem
    lib = built_lib
    mem, h = FakeMem(), C.c_void_p()
    assert lib.ovhip_dpb_create_ex(C.byref(h), 1, C.byref(mem.ops)) == 0
    f = C.c_void_p()
    assert lib.ovhip_frame_create(h, 0, 64, 64, C.byref(f)) == 0
    buf = np.full(4096, ss.FILL, np.uint8)
    arr, n = engine._rung_array([engine.ladder_rung(32, 32, engine.surface_format(), buf.ctypes.data, buf.nbytes)])
    assert lib.ovhip_frame_set_ladder_output(f, C.byref(info_of()), arr, n) == 0
    assert lib.ovhip_frame_set_ladder_output(f, None, arr, n) == 0
    assert lib.ovhip_frame_set_ladder_output(f, None, arr, sl.MAX_RUNGS + 1) == EINVAL and lib.ovhip_frame_set_ladder_output(None, None, arr, n) == EINVAL
    assert lib.ovhip_stream_set_ladder_output(None, None, arr, n, 1) == EINVAL
    assert lib.ovhip_frame_begin_tag(f, C.c_void_p(0x10), 1) == 0
    p = capi.JobParams()
    assert lib.ovhip_frame_submit(f, None, None, C.byref(p), None) == 0
    dev, pic = C.c_int(-1), capi.Pic()
    assert lib.ovhip_dpb_lookup(h, C.c_void_p(0x10), C.byref(dev), C.byref(pic)) == 0 and (pic.w, pic.h) == (64, 64)
    assert (buf == ss.FILL).all()
    assert lib.ovhip_frame_set_ladder_output(f, None, None, 0) == 0
    lib.ovhip_frame_destroy(f)
    lib.ovhip_dpb_destroy(h)


def test_exports_and_abi(built_lib):
    header = (ROOT / "include" / "ovvc_hip.h").read_text()
    for name in NEW:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in capi.EXPORTED_SYMBOLS and hasattr(built_lib, name), name
    assert "Output ladder on the device" in header
    m = re.search(r"#define OVHIP_LADDER_MAX_RUNGS (\d+)", header)
    assert m and int(m.group(1)) == capi.LADDER_MAX_RUNGS == sl.MAX_RUNGS
    assert C.sizeof(capi.LadderRung) == 56 and capi.LadderRung.fmt.offset == 8 and capi.LadderRung.dst.offset == 40
    assert capi.OVHIP_ABI_VERSION == 9 and built_lib.ovhip_abi_version() == 9
    assert "ovhip_ladder_plan_make_" not in header
