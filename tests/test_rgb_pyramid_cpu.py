"""CPU: the RGB pyramid on the host (openvvc_amd/csrc/ovvc_rgb_pyramid.c): ovhip_rgb_pyramid_host against the numpy restatement
tests/spec_rgb_pyramid.py byte for byte on the whole census, every tensor between sentinels, at 16-byte aligned destinations and at
destinations one element behind such a boundary, at source strides w and w + 6; the ratios of ovhip_rgb_pyramid_check; the refusals
with their codes, all or nothing; the exports; the frame's setters on a dry frame.  (The setters' combined check with a table needs a
table, and a table a device: tests/test_gpu_rgb_pyramid.py.)"""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import spec_rgb_pyramid as sp
from openvvc_amd import capi, engine
from test_ladder_cpu import host_pic
from test_reduce_cpu import info_of

ROOT = Path(__file__).resolve().parent.parent
EINVAL, EUNSUP = capi.OVHIP_EINVAL, capi.OVHIP_EUNSUP
FILL, GUARD = 0xA5, 32                                        # the sentinel; bytes in front of and behind a tensor that must stay as they were
NEW = ["ovhip_rgb_pyramid_check", "ovhip_rgb_pyramid_host", "ovhip_rgb_pyramid_launch", "ovhip_pic_output_rgb_pyramid", "ovhip_frame_set_rgb_pyramid_output",
       "ovhip_frame_set_rgb_pyramid_lut", "ovhip_stream_set_rgb_pyramid_output", "ovhip_stream_set_rgb_pyramid_lut"]


def c_format(lv, matrix, full_range, loc):
    return engine.rgb_format(matrix, full_range, loc, lv[2], lv[3])


def layout_of(levels, off_by_one=False):
    """[(offset of the tensor in its buffer, its bytes, the buffer's bytes)]: GUARD bytes on each side; the buffer's base is a multiple
    of 16, so the tensor begins on a 16-byte boundary or, with off_by_one, one element behind one"""
    return [(GUARD + (sp.ES[lv[2]] if off_by_one else 0), sp.level_bytes(lv), sp.level_bytes(lv) + 2 * GUARD + 16) for lv in levels]


def aligned_fill(nbytes):
    """a sentinel-filled uint8 array of nbytes whose address is a multiple of 16"""
    raw = np.full(nbytes + 16, FILL, np.uint8)
    a = raw[(-raw.ctypes.data) % 16:][:nbytes]
    assert a.ctypes.data % 16 == 0
    return a


def c_levels(levels, fmt3, bases, off_by_one=False):
    """the C levels over buffers at the addresses `bases` laid out by layout_of"""
    return [engine.rgb_level(lv[0], lv[1], c_format(lv, *fmt3), base + off, nbytes=n) for lv, base, (off, n, _t) in zip(levels, bases, layout_of(levels, off_by_one))]


def assert_equals_want(got, levels, want, what, off_by_one=False):
    """got: the whole buffers; want: spec_rgb_pyramid.pyramid(...): the tensor's bytes, the sentinel everywhere else"""
    assert len(got) == len(want)
    for k, (g, (off, n, total)) in enumerate(zip(got, layout_of(levels, off_by_one))):
        assert g.nbytes == total and want[k].nbytes == n, (what, k)
        assert g[off:off + n].tobytes() == want[k].tobytes(), (what, k, "the tensor")
        assert (g[:off] == FILL).all() and (g[off + n:] == FILL).all(), (what, k, "the guards")


def host_pyramid(lib, case, loc, off_by_one=False, spad=0, planes=None, window=None):
    _size, win, levels, (matrix, full_range), _t, _locs = sp.CENSUS[case]
    table, peak = sp.census_table(case)
    bufs = [aligned_fill(t) for _o, _n, t in layout_of(levels, off_by_one)]
    lv = c_levels(levels, (matrix, full_range, loc), [b.ctypes.data for b in bufs], off_by_one)
    _src, pic = host_pic(planes if planes is not None else sp.census_planes(case), spad)
    arr, n = engine._level_array(lv)
    tab = np.ascontiguousarray(table) if table is not None else None
    r = lib.ovhip_rgb_pyramid_host(C.byref(pic), C.byref(info_of(win if window is None else window, loc)), arr, n, tab.shape[0] if tab is not None else 0, peak,
                                   tab.ctypes.data if tab is not None else None)
    assert r == 0, (r, case, loc)
    return bufs


@pytest.mark.parametrize("case", list(sp.CENSUS))
def test_host_twin_equals_the_restatement_on_the_census(built_lib, case):
    levels, locs = sp.CENSUS[case][2], sp.CENSUS[case][5]
    for loc in locs:
        assert_equals_want(host_pyramid(built_lib, case, loc), levels, sp.census_want(case, loc), (case, loc))
    if case != "B":                                           # (the large case runs once)
        loc = locs[-1]
        assert_equals_want(host_pyramid(built_lib, case, loc, off_by_one=True), levels, sp.census_want(case, loc), (case, "one element behind a boundary"), True)
        assert_equals_want(host_pyramid(built_lib, case, loc, spad=6), levels, sp.census_want(case, loc), (case, "source strides w + 6"))
    if case in sp.WINDOW_CASES:
        inner = sp.window_planes(case)[1]
        assert_equals_want(host_pyramid(built_lib, case, locs[0], planes=inner, window=(0, 0, 0, 0)), levels, sp.census_want(case, locs[0]), "nothing outside the window is read")


def test_check_gives_the_ratios(built_lib):
    (w, h), win, levels, (matrix, full_range), _t, _locs = sp.CENSUS["A"]
    plain = [engine.rgb_level(lv[0], lv[1], c_format(lv, matrix, full_range, 3)) for lv in levels]
    r, ratios = engine.rgb_pyramid_check(w, h, plain)
    assert r == 0 and ratios == [(1, 1, 1, 1), (4, 3, 4, 3), (2, 1, 2, 1), (2, 1, 2, 1), (4, 1, 4, 1), (8, 3, 8, 3), (8, 1, 8, 1), (68, 9, 6, 1)]
    assert engine.rgb_pyramid_check(w, h, plain, lut_size=17, lut_peak=255)[0] == 0
    assert engine.rgb_pyramid_check(w, h, plain, lut_size=17, lut_peak=256)[0] == EINVAL            # (a U8 level)
    assert engine.rgb_pyramid_check(w, h, plain, chroma_loc=0)[0] == EINVAL                         # (the levels say 3)
    (w, h), win, levels, (matrix, full_range), _t, _locs = sp.CENSUS["W"]
    plain = [engine.rgb_level(lv[0], lv[1], c_format(lv, matrix, full_range, 0)) for lv in levels]
    assert engine.rgb_pyramid_check(w, h, plain, win, lut_size=65, lut_peak=65535) == (0, [(1, 1, 1, 1), (2, 1, 2, 1), (4, 1, 2, 1)])


def test_a_refused_pyramid_writes_nothing_and_check_agrees(built_lib):
    lib = built_lib
    planes = sp.ramp_planes(72, 40, 9)
    _src, pic = host_pic(planes)
    table = sp.st.random_table(17, 255, 5)
    good = [sp.level(48, 24, sp.F16, sp.CHW), sp.level(36, 20, sp.U8, sp.HWC), sp.level(72, 40, sp.U16, sp.CHW)]
    fmt3 = (1, 0, 0)
    bufs = [aligned_fill(t) for _o, _n, t in layout_of(good)]
    lv = c_levels(good, fmt3, [b.ctypes.data for b in bufs])

    def run(levels=lv, n=None, info=None, p=pic, size=0, peak=0, tab=None, check=None):
        """ovhip_rgb_pyramid_host's code; check: what ovhip_rgb_pyramid_check must say of the same arguments (None: the same)"""
        arr, cnt = engine._level_array(levels)
        cnt = cnt if n is None else n
        inf = info if info is not None else info_of()
        r = lib.ovhip_rgb_pyramid_host(C.byref(p) if p is not None else None, C.byref(inf), arr, cnt, size, peak, tab.ctypes.data if tab is not None else None)
        if p is not None:
            q = lib.ovhip_rgb_pyramid_check(p.w, p.h, C.byref(inf), arr, cnt, size, peak, None)
            assert q == (r if check is None else check), (q, r, check)
        return r

    def untouched(b=bufs):
        return all((x == FILL).all() for x in b)

    def at(k, ptr, nbytes=None, size=None, fmt=None):
        w, h = size or good[k][:2]
        return engine.rgb_level(w, h, fmt if fmt is not None else lv[k].fmt, ptr, nbytes=lv[k].dst_bytes if nbytes is None else nbytes)

    spare = aligned_fill(1 << 16)
    # everything the reduced-size output refuses for a level, in the last position: a ratio above 8, an up-sampling level, an odd size
    assert run(lv + [at(0, spare.ctypes.data, 1 << 16, (8, 40))]) == EUNSUP and run(lv + [at(0, spare.ctypes.data, 1 << 16, (144, 80))]) == EUNSUP
    assert run(lv + [at(0, spare.ctypes.data, 1 << 16, (34, 20))]) == EINVAL and untouched()
    # n out of range, null arguments
    assert run(n=0) == EINVAL and run(lv * 3) == EINVAL and untouched()
    arr3 = engine._level_array(lv)[0]
    assert lib.ovhip_rgb_pyramid_host(None, C.byref(info_of()), arr3, 3, 0, 0, None) == EINVAL
    assert lib.ovhip_rgb_pyramid_host(C.byref(pic), None, arr3, 3, 0, 0, None) == EINVAL
    assert lib.ovhip_rgb_pyramid_host(C.byref(pic), C.byref(info_of()), None, 3, 0, 0, None) == EINVAL
    assert lib.ovhip_rgb_pyramid_check(72, 40, None, arr3, 3, 0, 0, None) == EINVAL and lib.ovhip_rgb_pyramid_check(72, 40, C.byref(info_of()), None, 3, 0, 0, None) == EINVAL
    assert untouched()
    # what the RGB output refuses of a level's size and format: a size that is a multiple of 2 only, a dtype, a layout, a range, matrices
    assert run(lv[:1] + [at(1, bufs[1].ctypes.data + GUARD, size=(36, 18))]) == EINVAL
    for bad, code in ((engine.rgb_format(1, 0, 0, 4, 0), EINVAL), (engine.rgb_format(1, 0, 0, 0, 2), EINVAL), (engine.rgb_format(2, 0, 0, 0, 0), EINVAL),
                      (engine.rgb_format(3, 0, 0, 0, 0), EUNSUP), (engine.rgb_format(1, 2, 0, 0, 0), EINVAL), (engine.rgb_format(1, 0, 6, 0, 0), EINVAL)):
        assert run([at(1, lv[1].dst, fmt=bad)]) == code, (bad.matrix, bad.full_range, bad.chroma_loc, bad.dtype, bad.layout)
    assert untouched()
    # formats that disagree in matrix, range or location; a location that is not the pyramid's
    for other in (engine.rgb_format(9, 0, 0, sp.U8, sp.HWC), engine.rgb_format(1, 1, 0, sp.U8, sp.HWC), engine.rgb_format(1, 0, 2, sp.U8, sp.HWC)):
        assert run([lv[0], at(1, lv[1].dst, fmt=other), lv[2]]) == EINVAL
    assert run(info=info_of(loc=1)) == EINVAL and untouched()
    # what only a picture or a destination shows: the check accepts, the twin refuses
    small = [lv[0], lv[1], at(2, lv[2].dst, lv[2].dst_bytes - 1)]
    null = [lv[0], at(1, None), lv[2]]
    odd = [at(0, lv[0].dst + 1), lv[1], lv[2]]
    both = aligned_fill(lv[0].dst_bytes + lv[1].dst_bytes)
    over = [at(0, both.ctypes.data), at(1, both.ctypes.data + lv[0].dst_bytes - 2)]
    assert run(small, check=0) == EINVAL and run(null, check=0) == EINVAL and run(odd, check=0) == EINVAL and run(over, check=0) == EINVAL
    assert untouched() and untouched([both])
    assert run(p=capi.Pic(pic.y, None, pic.cr, 72, 40, 72, 36), check=0) == EINVAL and run(p=capi.Pic(pic.y, pic.cb, pic.cr, 72, 40, 70, 36), check=0) == EINVAL
    src, p2 = host_pic(planes)
    inside = [lv[0], lv[1], at(2, src[2].ctypes.data + 2 * src[2].size - 8)]
    assert run(inside, p=p2, check=0) == EINVAL and untouched() and np.array_equal(src[2], planes[2])
    # the table: null, a size or a peak that is none, a peak a U8 level cannot take, an entry above the peak (the twin's alone)
    assert run(size=17, peak=255, tab=None, check=0) == EINVAL and run(size=16, peak=255, tab=table) == EINVAL and run(size=17, peak=0, tab=table) == EINVAL
    assert run(size=17, peak=65536, tab=table) == EINVAL and run(size=17, peak=256, tab=table) == EINVAL
    assert run(size=17, peak=254, tab=table, check=0) == EINVAL and untouched()
    # accepted: with the table, and without
    assert run(size=17, peak=255, tab=table) == 0 and not any(untouched([b]) for b in bufs)
    assert run() == 0


def test_a_dry_frame_answers_and_does_nothing(built_lib):
    from test_dpb_cpu import FakeMem
    lib = built_lib
    mem, h = FakeMem(), C.c_void_p()
    assert lib.ovhip_dpb_create_ex(C.byref(h), 1, C.byref(mem.ops)) == 0
    f = C.c_void_p()
    assert lib.ovhip_frame_create(h, 0, 64, 64, C.byref(f)) == 0
    fake = C.c_void_p(0x1000)                                  # (a dry frame never looks at the table)
    assert lib.ovhip_frame_set_rgb_pyramid_lut(f, fake) == 0 and lib.ovhip_frame_set_rgb_pyramid_lut(f, None) == 0
    assert lib.ovhip_frame_set_rgb_pyramid_lut(None, None) == EINVAL and lib.ovhip_frame_set_rgb_pyramid_output(None, None, None, 0) == EINVAL
    assert lib.ovhip_stream_set_rgb_pyramid_lut(None, 0, 0, None) == EINVAL and lib.ovhip_stream_set_rgb_pyramid_output(None, None, None, 0, 0) == EINVAL
    buf = np.full(2 * 3 * 32 * 32, FILL, np.uint8)
    ok = [engine.rgb_level(32, 32, engine.rgb_format(), buf.ctypes.data, nbytes=3 * 32 * 32),
          engine.rgb_level(16, 16, engine.rgb_format(dtype=capi.RGB_F16), buf.ctypes.data + 3 * 32 * 32, nbytes=3 * 32 * 32)]

    def setter(levels, n=None, info=None):
        arr, cnt = engine._level_array(levels)
        return lib.ovhip_frame_set_rgb_pyramid_output(f, C.byref(info) if info is not None else None, arr, cnt if n is None else n)

    # the refusals that need no picture come back from the setter: n, a null destination, the levels' own, the formats' agreement
    assert setter(ok, n=0) == EINVAL and setter(ok * 5) == EINVAL
    assert setter([engine.rgb_level(32, 32, engine.rgb_format(), None, nbytes=4096)]) == EINVAL
    assert setter([engine.rgb_level(4, 32, engine.rgb_format(), buf.ctypes.data, nbytes=4096)]) == EUNSUP      # (16:1)
    assert setter([engine.rgb_level(30, 32, engine.rgb_format(), buf.ctypes.data, nbytes=4096)]) == EINVAL
    assert setter([ok[0], engine.rgb_level(16, 16, engine.rgb_format(matrix=9), ok[1].dst, nbytes=4096)]) == EINVAL
    assert setter(ok, info=info_of(loc=2)) == EINVAL
    # against the size the post setting of the moment leaves: behind a first reduce to 32 x 32 a 64 x 64 level would be up-sampling
    big = [engine.rgb_level(64, 64, engine.rgb_format(), buf.ctypes.data, nbytes=1 << 20)]
    assert setter(big) == 0
    assert lib.ovhip_frame_set_output_reduce(f, 32, 32, None) == 0 and setter(big) == EUNSUP and setter(ok) == 0
    assert lib.ovhip_frame_set_output_reduce(f, 0, 0, None) == 0
    # accepted, cleared, accepted: the picture is published and nothing is written
    assert setter(ok) == 0 and lib.ovhip_frame_set_rgb_pyramid_output(f, None, None, 0) == 0 and setter(ok) == 0
    assert lib.ovhip_frame_begin_tag(f, C.c_void_p(0x10), 1) == 0
    p = capi.JobParams()
    assert lib.ovhip_frame_submit(f, None, None, C.byref(p), None) == 0
    assert (buf == FILL).all()
    lib.ovhip_frame_destroy(f)
    lib.ovhip_dpb_destroy(h)


def test_exports_and_abi(built_lib):
    header = (ROOT / "include" / "ovvc_hip.h").read_text()
    for name in NEW:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in capi.EXPORTED_SYMBOLS and hasattr(built_lib, name), name
    assert "RGB pyramid on the device" in header and "OVHIP_PYRAMID_MAX_LEVELS 8" in header
    assert capi.OVHIP_ABI_VERSION == 9 and built_lib.ovhip_abi_version() == 9
    assert capi.PYRAMID_MAX_LEVELS == sp.MAX_LEVELS == 8
    assert "ovhip_rgb_pyramid_plan_make_" not in header
    assert C.sizeof(capi.RgbLevel) == 32
