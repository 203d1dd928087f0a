"""GPU: the RGB pyramid on the device (k_rgb_pyramid, openvvc_amd/csrc/kernels_rgb_pyramid.hip) and the layers above it:
ovhip_rgb_pyramid_launch against the numpy restatement tests/spec_rgb_pyramid.py on the whole census -- all levels of a pyramid in ONE
device buffer with sentinels around and between them, at 16-byte boundaries and one element behind them, strided sources, torch
tensors --, the refusals, the synchronous convenience and the scratch, the frame thread (whole and band-wise; behind film grain and
behind a first reduce; against the frame's own reduced RGB output; the table until it is cleared) and the stream driver's slots beside
an NV12 ladder of grained pictures.  Every comparison is of bytes."""
import ctypes as C

import numpy as np
import pytest

import spec_film_grain as sf
import spec_ladder as sl
import spec_reduce as sd
import spec_rgb_lut as st
import spec_rgb_pyramid as sp
from openvvc_amd import capi, engine, gop
from test_film_grain_cpu import c_params
from test_gpu_ladder import device_pic
from test_gpu_reduce import _frame
from test_gpu_stream import _contents, _jobs_for, _make_contents, _stream_pics
from test_rgb_pyramid_cpu import FILL, GUARD, c_format

pytestmark = pytest.mark.gpu
EINVAL, EUNSUP = capi.OVHIP_EINVAL, capi.OVHIP_EUNSUP


@pytest.fixture(scope="module")
def ctx(built_lib):
    c = engine.Context(0)
    yield c
    c.close()


def arena_of(levels, off_by_one=False):
    """([offset of level r in one buffer], the buffer's bytes): GUARD bytes in front of, between and behind the tensors; a tensor begins
    on a 16-byte boundary of the buffer (whose base is one) or, with off_by_one, one element behind one"""
    offs, cur = [], 0
    for lv in levels:
        cur = (cur + GUARD + 15) // 16 * 16 + (sp.ES[lv[2]] if off_by_one else 0)
        offs.append(cur)
        cur += sp.level_bytes(lv)
    return offs, cur + GUARD


def arena_levels(levels, fmt3, base, off_by_one=False):
    return [engine.rgb_level(lv[0], lv[1], c_format(lv, *fmt3), base + off, nbytes=sp.level_bytes(lv)) for lv, off in zip(levels, arena_of(levels, off_by_one)[0])]


def assert_arena(got, levels, want, what, off_by_one=False):
    """got: the whole buffer; want: spec_rgb_pyramid.pyramid(...) or None for an untouched buffer: the tensors' bytes, the sentinel
    everywhere else"""
    offs, total = arena_of(levels, off_by_one)
    assert got.nbytes == total
    mask = np.ones(total, bool)
    for k, (lv, off) in enumerate(zip(levels, offs)):
        n = sp.level_bytes(lv)
        mask[off:off + n] = False
        assert want[k].nbytes == n and got[off:off + n].tobytes() == want[k].tobytes(), (what, k, "the tensor")
    assert (got[mask] == FILL).all(), (what, "the guards around and between the tensors")


def device_pyramid(ctx, planes, levels, fmt3, window=(0, 0, 0, 0), lut=None, off_by_one=False, spad=0):
    """ovhip_rgb_pyramid_launch of the planes (rows of w + spad samples) -> the whole buffer, tensors and guards"""
    sb, held, pic = device_pic(ctx, planes, spad)
    buf = ctx.upload(np.full(arena_of(levels, off_by_one)[1], FILL, np.uint8))
    assert buf.ptr.value % 16 == 0
    pic.rgb_pyramid_into(arena_levels(levels, fmt3, buf.ptr.value, off_by_one), window, lut=lut)
    ctx.sync()
    got = buf.download()
    assert all(np.array_equal(a.ravel(), b.download(np.uint16)) for a, b in zip(held, sb)), "the source is only read"
    [b.free() for b in sb + [buf]]
    return got


@pytest.mark.parametrize("case", list(sp.CENSUS))
def test_launch_equals_the_restatement_on_the_census(ctx, case):
    _size, win, levels, (matrix, full_range), _t, locs = sp.CENSUS[case]
    planes = sp.census_planes(case)
    table, peak = sp.census_table(case)
    lut = engine.RgbLut(ctx, table, peak) if table is not None else None
    for loc in locs:
        assert_arena(device_pyramid(ctx, planes, levels, (matrix, full_range, loc), win, lut), levels, sp.census_want(case, loc), (case, loc))
    if case != "B":                                           # (the large case runs once)
        loc = locs[-1]
        fmt3, want = (matrix, full_range, loc), sp.census_want(case, loc)
        assert_arena(device_pyramid(ctx, planes, levels, fmt3, win, lut, off_by_one=True), levels, want, (case, "one element behind a boundary"), True)
        assert_arena(device_pyramid(ctx, planes, levels, fmt3, win, lut, spad=6), levels, want, (case, "source strides w + 6"))
        assert_arena(device_pyramid(ctx, planes, levels, fmt3, win, lut, off_by_one=True, spad=6), levels, want, (case, "both"), True)
    if lut is not None:
        lut.close()


def test_torch_tensors_are_the_destinations(ctx):
    """a level per picture of a batch tensor; a batch tensor that begins one element behind a 16-byte boundary"""
    import torch
    case, loc = "F", 4
    _size, win, levels, (matrix, full_range), _t, _locs = sp.CENSUS[case]
    want = sp.census_want(case, loc)
    pic = ctx.upload_pic(*sp.census_planes(case))
    tdt = {sp.U8: torch.uint8, sp.U16: torch.uint16, sp.F16: torch.float16, sp.F32: torch.float32}
    keep, c_lv = [], []
    for lv, x in zip(levels, want):
        n = int(np.prod(x.shape))
        flat = torch.zeros(2 * n + 1, dtype=tdt[lv[2]], device="cuda:0")
        batch = flat[1:].view(2, *x.shape)                    # (element-aligned only)
        assert batch.data_ptr() % 16 == sp.ES[lv[2]] and batch.is_contiguous()
        keep.append((flat, batch))
        c_lv.append(engine.rgb_level(lv[0], lv[1], c_format(lv, matrix, full_range, loc), batch[1]))
    with pytest.raises(engine.EngineError):
        engine.rgb_level(levels[0][0], levels[0][1], c_format(levels[0], matrix, full_range, loc), keep[1][1][1])      # (another level's shape and dtype)
    torch.cuda.synchronize()
    pic.rgb_pyramid_into(c_lv, win)
    ctx.sync()
    as_bytes = lambda t: t.contiguous().view(torch.uint8).cpu().numpy()
    for (flat, batch), x in zip(keep, want):
        assert as_bytes(batch[1]).tobytes() == x.tobytes()
        assert not as_bytes(flat[:1 + x.size]).any(), "the element in front and the picture before stay as they were"
    pic.free()


def test_refusals_write_nothing_on_the_device(ctx):
    """return values, the error text and the sentinels only: nothing is provoked on the device"""
    lib = ctx.lib
    planes = sp.ramp_planes(72, 40, 9)
    sb, _held, pic = device_pic(ctx, planes)
    good = [sp.level(48, 24, sp.F16, sp.CHW), sp.level(36, 20, sp.U8, sp.HWC), sp.level(72, 40, sp.U16, sp.CHW)]
    offs, total = arena_of(good)
    buf = ctx.upload(np.full(total, FILL, np.uint8))
    lv = arena_levels(good, (1, 0, 0), buf.ptr.value)
    lut = engine.RgbLut(ctx, st.random_table(17, 255, 5), 255)
    big = engine.RgbLut(ctx, st.random_table(17, 1023, 6), 1023)
    err = lambda: lib.ovhip_last_error(ctx.h).decode()

    def into(levels=lv, window=(0, 0, 0, 0), chroma_loc=None, table=None):
        return pic.rgb_pyramid_into(levels, window, chroma_loc, check=False, lut=table)

    def untouched():
        ctx.sync()
        return (buf.download() == FILL).all()

    def at(k, ptr, nbytes=None, size=None, fmt=None):
        w, h = size or good[k][:2]
        return engine.rgb_level(w, h, fmt if fmt is not None else lv[k].fmt, ptr, nbytes=lv[k].dst_bytes if nbytes is None else nbytes)

    spare = ctx.upload(np.full(1 << 16, FILL, np.uint8))
    # the reduced-size output's refusals, in the last position, with the level's index
    assert into(lv + [at(0, spare.ptr.value, 1 << 16, (8, 40))]) == EUNSUP and "level 3" in err() and "ratio" in err()
    assert into(lv + [at(0, spare.ptr.value, 1 << 16, (144, 80))]) == EUNSUP and "up-sampling" in err()
    assert into(lv + [at(0, spare.ptr.value, 1 << 16, (34, 20))]) == EINVAL and "level 3" in err()
    # n out of range, null arguments
    arr, _n = engine._level_array(lv)
    info = capi.ReduceInfo()
    assert lib.ovhip_rgb_pyramid_launch(ctx.h, C.byref(pic.s), C.byref(info), arr, 0, None) == EINVAL and "levels" in err()
    assert into([at(1, spare.ptr.value + 4096 * k) for k in range(sp.MAX_LEVELS + 1)]) == EINVAL
    assert lib.ovhip_rgb_pyramid_launch(ctx.h, None, C.byref(info), arr, 3, None) == EINVAL
    assert lib.ovhip_rgb_pyramid_launch(ctx.h, C.byref(pic.s), None, arr, 3, None) == EINVAL and lib.ovhip_rgb_pyramid_launch(ctx.h, C.byref(pic.s), C.byref(info), None, 3, None) == EINVAL
    assert lib.ovhip_rgb_pyramid_launch(None, C.byref(pic.s), C.byref(info), arr, 3, None) == EINVAL
    # what the RGB output refuses of a level: too small by one byte (last level), a null destination, an unaligned one, a size, a format
    assert into(lv[:2] + [at(2, lv[2].dst, lv[2].dst_bytes - 1)]) == EINVAL and "level 2" in err() and "too small" in err()
    assert into([lv[0], at(1, None), lv[2]]) == EINVAL and "level 1" in err()
    assert into([at(0, lv[0].dst + 1)] + lv[1:]) == EINVAL and "aligned" in err()
    assert into([lv[0], at(1, lv[1].dst, size=(36, 18))]) == EINVAL and "level 1" in err() and "multiples of 4" in err()
    assert into([at(1, lv[1].dst, fmt=engine.rgb_format(3, 0, 0, sp.U8, sp.HWC))]) == EUNSUP and into([at(1, lv[1].dst, fmt=engine.rgb_format(1, 0, 0, 4, 0))]) == EINVAL
    # destinations that overlap one another, or the picture
    assert into([lv[0], at(1, lv[0].dst + lv[0].dst_bytes - 2)]) == EINVAL and "overlaps level 0" in err()
    assert into(lv[:2] + [at(2, sb[0].ptr.value)]) == EINVAL and "overlaps the picture" in err()
    # formats that disagree; the pyramid's location; the window; a missing plane
    for other in (engine.rgb_format(9, 0, 0, sp.U8, sp.HWC), engine.rgb_format(1, 1, 0, sp.U8, sp.HWC), engine.rgb_format(1, 0, 2, sp.U8, sp.HWC)):
        assert into([lv[0], at(1, lv[1].dst, fmt=other), lv[2]]) == EINVAL and "level 1" in err() and "differ" in err()
    assert into(chroma_loc=1) == EINVAL and "location" in err()
    assert into(window=(18, 18, 0, 0)) == EINVAL
    s = capi.Pic(pic.s.y, None, pic.s.cr, 72, 40, 72, 36)
    assert engine.DevPic(ctx, s, owns=False).rgb_pyramid_into(lv, check=False) == EINVAL and "missing plane" in err()
    # the table: a peak a U8 level cannot take
    assert into(table=big) == EINVAL and "level 1" in err() and "peak" in err()
    assert untouched()
    with pytest.raises(engine.EngineError):
        pic.rgb_pyramid([engine.rgb_level(36, 20), engine.rgb_level(8, 40)])
    assert "level 1" in err()
    assert into(table=lut) == 0 and not untouched()
    lut.close(); big.close()
    [b.free() for b in sb + [buf, spare]]


def test_the_convenience_equals_the_launch_and_the_scratch_stays_flat(built_lib):
    ctx = engine.Context(0)
    for case in ("WN", "T"):
        _size, win, levels, (matrix, full_range), _t, locs = sp.CENSUS[case]
        loc = locs[0]
        planes = sp.census_planes(case)
        table, peak = sp.census_table(case)
        pic = ctx.upload_pic(*planes)
        plain = [engine.rgb_level(lv[0], lv[1], c_format(lv, matrix, full_range, loc)) for lv in levels]
        lut = engine.RgbLut(ctx, table, peak) if table is not None else None
        before = ctx.scratch_bytes()
        buf = ctx.upload(np.full(arena_of(levels)[1], FILL, np.uint8))
        for rep in range(3):
            pic.rgb_pyramid_into(arena_levels(levels, (matrix, full_range, loc), buf.ptr.value), win, lut=lut)
        ctx.sync()
        assert ctx.scratch_bytes() == before, "the launch allocates nothing"
        assert_arena(buf.download(), levels, sp.census_want(case, loc), case)
        buf.free()
        with pytest.raises(engine.EngineError):
            pic.rgb_pyramid(plain + [engine.rgb_level(4, 4, plain[0].fmt)], win, lut=lut)
        assert ctx.scratch_bytes() == before, "a refused request allocates nothing"
        got = pic.rgb_pyramid(plain, win, lut=lut)
        assert [g.tobytes() for g in got] == [x.tobytes() for x in sp.census_want(case, loc)], case
        assert [g.shape for g in got] == [x.shape for x in sp.census_want(case, loc)]
        held = ctx.scratch_bytes()
        assert [g.tobytes() for g in pic.rgb_pyramid(plain, win, lut=lut)] == [g.tobytes() for g in got]
        assert ctx.scratch_bytes() == held, "no allocation once the sizes have been seen"
        if lut is not None:
            lut.close()
        pic.free()
    ctx.close()


def _pyramid_case(post):
    """(frame size, the size the pyramid reads, its levels, the film grain SEI)"""
    if post == "grain":
        sei = sf.make_sei(log2_scale=2, comps=((8, 3, 200, 8, 8), (3, 2, 100, 4, 6), (1, 1, 90, 8, 8)))
        return (88, 56), (88, 56), [sp.level(88, 56, sp.U8, sp.HWC), sp.level(44, 28, sp.F16, sp.CHW), sp.level(24, 8, sp.U16, sp.CHW)], sei
    if post == "reduce":
        return (72, 40), (48, 24), [sp.level(48, 24, sp.U16, sp.HWC), sp.level(24, 12, sp.U8, sp.CHW), sp.level(12, 8, sp.F32, sp.CHW)], None
    return (72, 40), (72, 40), [sp.level(72, 40, sp.F32, sp.HWC), sp.level(48, 24, sp.F16, sp.CHW), sp.level(36, 20, sp.U8, sp.HWC)], None


@pytest.mark.parametrize("via", ["submit", "band"])
@pytest.mark.parametrize("post", ["none", "grain", "reduce"])
def test_frame_pyramid_reads_the_shown_picture_and_the_table_stays_until_cleared(built_lib, via, post):
    """the pyramid of the picture the frame shows -- the decoded one, the grained one (the reason for the feature: a stream with an FGC
    SEI feeds reduced tensors) or a first reduce's; the destinations end with the picture; the table is sticky; a refused pyramid fails
    the call, not the publication; the second setter makes the combined check"""
    lib = built_lib
    (w, h), (ow, oh), levels, sei = _pyramid_case(post)
    wl, dpb, ctx, f, params = _frame(w, h)
    loc, poc, matrix, full_range = 2, 7, 9, 0
    fmt3 = (matrix, full_range, loc)
    table, peak = st.random_table(17, 255, 21), 255
    lut = engine.RgbLut(ctx, table, peak)
    if post == "grain":
        f.set_film_grain(c_params(sei), poc)
    elif post == "reduce":
        f.set_output_reduce(ow, oh, chroma_loc=loc)

    def picture(key, c_lv, check=True):
        if c_lv is not None:
            f.set_rgb_pyramid_output(c_lv)
        f.begin(key)
        f.recorder().replay(wl.calllog)
        if via == "submit":
            return f.submit(params, check=check)
        assert lib.ovhip_frame_set_band_mode(f.f, 1) == 0
        r = lib.ovhip_frame_band(f.f, C.byref(params), h, 1, None)
        assert lib.ovhip_frame_set_band_mode(f.f, 0) == 0
        return 0 if r == 1 else r

    def pyramid_of(key, with_levels=True):
        buf = ctx.upload(np.full(arena_of(levels)[1], FILL, np.uint8))
        assert picture(key, arena_levels(levels, fmt3, buf.ptr.value) if with_levels else None) == 0
        got = buf.download()
        buf.free()
        return got

    got = pyramid_of(0x100)
    _dev, held_pic = dpb.lookup(0x100)
    assert (held_pic.w, held_pic.h) == (w, h)
    dec = engine.DevPic(ctx, held_pic, owns=False).download()
    shown = sf.apply(dec, sei, poc)[0] if post == "grain" else (sd.reduce_picture(*dec, ow, oh, loc=loc) if post == "reduce" else dec)
    if post == "grain":
        assert not all(np.array_equal(a, b) for a, b in zip(shown, dec)), "the grain acts"
    plain = sp.pyramid(shown, levels, matrix, full_range, loc)
    assert_arena(got, levels, plain, (post, via, "the pyramid of the shown picture"))
    # the destinations ended with the picture: the next one, with nothing set, writes nothing
    assert (pyramid_of(0x101, with_levels=False) == FILL).all()
    # the table: sticky until cleared
    through = sp.pyramid(shown, levels, matrix, full_range, loc, table, peak)
    f.set_rgb_pyramid_lut(lut)
    assert_arena(pyramid_of(0x102), levels, through, (post, via, "through the table"))
    assert_arena(pyramid_of(0x103), levels, through, "sticky: the next picture too")
    # a pyramid the picture's last call refuses fails that call, not the publication, and writes nothing
    buf = ctx.upload(np.full(arena_of(levels)[1], FILL, np.uint8))
    c_lv = arena_levels(levels, fmt3, buf.ptr.value)
    c_lv[-1].dst_bytes -= 1
    assert picture(0x104, c_lv, check=False) == EINVAL
    assert dpb.lookup(0x104)[1].w == w
    ctx.sync()
    assert (buf.download() == FILL).all()
    # the second setter makes the combined check: a table of peak 1023 behind levels with a U8 one, and those levels behind that table
    c_lv = arena_levels(levels, fmt3, buf.ptr.value)
    big = engine.RgbLut(ctx, st.random_table(17, 1023, 22), 1023)
    assert f.set_rgb_pyramid_output(c_lv) == 0 and f.set_rgb_pyramid_lut(big, check=False) == EINVAL
    assert f.set_rgb_pyramid_output(None) == 0 and f.set_rgb_pyramid_lut(big) == 0 and f.set_rgb_pyramid_output(c_lv, check=False) == EINVAL
    assert f.set_rgb_pyramid_lut(lut) == 0
    # the setter's own refusals; off
    assert f.set_rgb_pyramid_output([], check=False) == EINVAL
    assert f.set_rgb_pyramid_output([engine.rgb_level(ow * 2, oh * 2, c_lv[0].fmt, 4096, nbytes=1 << 20)], check=False) == EUNSUP
    assert f.set_rgb_pyramid_output([engine.rgb_level(ow, oh, c_lv[0].fmt, None, nbytes=1 << 20)], check=False) == EINVAL
    assert f.set_rgb_pyramid_output(c_lv, chroma_loc=0, check=False) == EINVAL
    buf.free()
    assert_arena(pyramid_of(0x105), levels, through, "the setters' refusals leave the table as it was")
    f.set_rgb_pyramid_lut(None)
    assert_arena(pyramid_of(0x106), levels, plain, "cleared")
    lut.close(); big.close()
    f.close(); ctx.close(); dpb.close()


@pytest.mark.parametrize("with_table", [False, True])
def test_frame_level_equals_the_frames_own_reduced_rgb_output(built_lib, with_table):
    """a level is what the same frame writes as its RGB output with set_output_reduce to that size in front of it (set_rgb_lut when a
    table is set); the RGB output's table and the pyramid's are independent"""
    (w, h), _o, levels, _sei = _pyramid_case("none")
    wl, dpb, ctx, f, params = _frame(w, h)
    loc, matrix, full_range = 0, 1, 0
    fmt3 = (matrix, full_range, loc)
    table, peak = st.random_table(33, 255, 31), 255
    lut = engine.RgbLut(ctx, table, peak) if with_table else None
    other = engine.RgbLut(ctx, st.random_table(17, 255, 32), 255)
    key = [0x200]

    def picture(reduce_to, c_lv, rgb):
        f.set_output_reduce(*((reduce_to[0], reduce_to[1], (0, 0, 0, 0), loc) if reduce_to else (0, 0)))
        if c_lv:
            f.set_rgb_pyramid_output(c_lv)
        if rgb:
            f.set_rgb_output(rgb[0], rgb[1], nbytes=rgb[2])
        f.begin(key[0])
        f.recorder().replay(wl.calllog)
        assert f.submit(params) == 0
        key[0] += 1

    buf = ctx.upload(np.full(arena_of(levels)[1], FILL, np.uint8))
    f.set_rgb_pyramid_lut(lut)
    f.set_rgb_lut(other)                                      # (the RGB output's table is not the pyramid's)
    picture(None, arena_levels(levels, fmt3, buf.ptr.value), None)
    got = buf.download()
    dec = engine.DevPic(ctx, dpb.lookup(0x200)[1], owns=False).download()
    assert_arena(got, levels, sp.pyramid(dec, levels, matrix, full_range, loc, table if with_table else None, peak), "the pyramid")
    f.set_rgb_lut(lut)
    for lv, off in zip(levels, arena_of(levels)[0]):
        n = sp.level_bytes(lv)
        d = ctx.upload(np.full(n + GUARD, FILL, np.uint8))
        picture(lv[:2], None, (d.ptr.value, c_format(lv, *fmt3), n))
        own = d.download()
        assert own[:n].tobytes() == got[off:off + n].tobytes() and (own[n:] == FILL).all(), lv
        d.free()
    buf.free()
    [x.close() for x in (lut, other) if x is not None]
    f.close(); ctx.close(); dpb.close()


def _stream(w, h):
    wls = _contents(w, h, (41, 42), 43)
    spics = _stream_pics(gop.build_stream(1, 4, 4, 1), 2)                               # I and one GOP of 4
    ctx = engine.Context(0)
    dpb = engine.Dpb((0,))
    jobs = _jobs_for(ctx, wls, spics, w, h)
    strm = engine.Stream(dpb, w, h, _make_contents(wls), jobs, threads_per_device=4)
    return spics, ctx, dpb, jobs, strm


def _slot_tensors(levels, n):
    import torch
    tdt = {sp.U8: torch.uint8, sp.U16: torch.uint16, sp.F16: torch.float16, sp.F32: torch.float32}
    ts = []
    for (w, h, dtype, layout) in levels:
        shape = (3, h, w) if layout == sp.CHW else (h, w, 3)
        ts.append(torch.zeros((n,) + shape, dtype=tdt[dtype], device="cuda:0"))
    torch.cuda.synchronize()
    return ts


def test_stream_with_film_grain_delivers_a_ladder_and_a_pyramid(built_lib):
    """what a frame could not express before: a stream with a film grain SEI feeds an NV12 ladder AND reduced tensors, both of the
    grained pictures"""
    import torch
    w, h = 416, 240
    spics, ctx, dpb, jobs, strm = _stream(w, h)
    n = len(spics)
    arr = strm.pics_array(spics)
    sei = sf.make_sei(log2_scale=2, comps=((8, 3, 200, 8, 8), (3, 2, 100, 4, 6), (1, 1, 90, 8, 8)))
    strm.set_film_grain(c_params(sei))
    loc, matrix = 1, 1
    levels = [sp.level(208, 120, sp.F16, sp.CHW), sp.level(104, 60, sp.U8, sp.HWC)]
    ts = _slot_tensors(levels, n)
    c_lv = [engine.rgb_level(lv[0], lv[1], c_format(lv, matrix, 0, loc), t, slots=True) for lv, t in zip(levels, ts)]
    sizes = [(416, 240), (208, 120)]
    need = [sw * sh * 3 // 2 for sw, sh in sizes]
    ls = [torch.zeros((n, nb), dtype=torch.uint8, device="cuda:0") for nb in need]
    torch.cuda.synchronize()
    rungs = [engine.ladder_rung(sw, sh, engine.surface_format(capi.SURF_NV12), t, slots=True) for (sw, sh), t in zip(sizes, ls)]
    assert strm.set_ladder_output(rungs, chroma_loc=loc) == 0
    assert strm.set_rgb_pyramid_output(c_lv) == 0
    res, _dg = strm.run(arr, n, 0, n, flags=capi.STREAM_KEEP | capi.STREAM_HOLD_ALL)
    assert res.status == 0 and res.n_decoded == n
    got_p, got_l = [t.cpu().numpy() for t in ts], [t.cpu().numpy() for t in ls]
    for i in range(n):
        dec = strm.picture(i, ctx).download()
        shown = sf.apply(dec, sei, spics[i]["poc"])[0]
        want_p = sp.pyramid(shown, levels, matrix, 0, loc)
        want_l = sl.ladder(shown, [sl.rung(*sizes[0], sl.NV12), sl.rung(*sizes[1], sl.NV12)], loc=loc)
        for k in range(2):
            assert got_p[k][i].tobytes() == want_p[k].tobytes(), (i, k, "pyramid")
            assert got_l[k][i].tobytes() == want_l[k][0].tobytes(), (i, k, "ladder")
    strm.close(); [j.close() for j in jobs]; dpb.close(); ctx.close()


def test_stream_writes_a_two_level_pyramid_into_slots(built_lib):
    w, h = 416, 240
    spics, ctx, dpb, jobs, strm = _stream(w, h)
    n = len(spics)
    arr = strm.pics_array(spics)
    loc, matrix = 0, 9
    levels = [sp.level(208, 120, sp.F16, sp.CHW), sp.level(104, 60, sp.U8, sp.HWC)]
    ts = _slot_tensors(levels, n)
    c_lv = [engine.rgb_level(lv[0], lv[1], c_format(lv, matrix, 0, loc), t, slots=True) for lv, t in zip(levels, ts)]
    assert [g.dst_bytes for g in c_lv] == [sp.level_bytes(lv) for lv in levels]
    fmt0 = c_lv[0].fmt
    # the setter's refusals: a slot below the tensor's size, no slots, an up-sampling level; the previous setting (none) stands
    assert strm.set_rgb_pyramid_output([engine.rgb_level(208, 120, fmt0, ts[0].data_ptr(), nbytes=c_lv[0].dst_bytes - 2)], n_slots=n, check=False) == EINVAL
    assert strm.set_rgb_pyramid_output([engine.rgb_level(208, 120, fmt0, ts[0].data_ptr(), nbytes=c_lv[0].dst_bytes)], n_slots=0, check=False) == EINVAL
    assert strm.set_rgb_pyramid_output([engine.rgb_level(832, 480, fmt0, ts[0].data_ptr(), nbytes=1 << 24)], n_slots=n, check=False) == EUNSUP
    assert strm.set_rgb_pyramid_output(c_lv) == 0
    # the second setter makes the combined check: a peak the U8 level cannot take; on a refusal the previous setting (no table) stands
    assert strm.set_rgb_pyramid_lut(st.random_table(17, 1023, 50), 1023, check=False) == EINVAL
    res, _dg = strm.run(arr, n, 0, n, flags=capi.STREAM_KEEP | capi.STREAM_HOLD_ALL)
    assert res.status == 0 and res.n_decoded == n
    decoded = [strm.picture(i, ctx).download() for i in range(n)]
    got = [t.cpu().numpy() for t in ts]
    for i in range(n):                                                                  # every picture of the run, each in its own slot
        want = sp.pyramid(decoded[i], levels, matrix, 0, loc)
        for k in range(2):
            assert got[k][i].tobytes() == want[k].tobytes(), (i, k)
    # through a table; a table with an entry above its peak is refused and the one set stands; levels the table cannot serve are refused
    table, peak = st.random_table(17, 255, 51), 255
    assert strm.set_rgb_pyramid_lut(table, peak) == 0
    bad = table.copy()
    bad[0, 0, 0, 0] = 256
    assert strm.set_rgb_pyramid_lut(bad, peak, check=False) == EINVAL
    res, _dg = strm.run(arr, n, 0, n)
    assert res.status == 0
    got = [t.cpu().numpy() for t in ts]
    want = sp.pyramid(decoded[n - 1], levels, matrix, 0, loc, table, peak)
    assert all(got[k][n - 1].tobytes() == want[k].tobytes() for k in range(2))
    # cleared: the plain pyramid again; off
    assert strm.set_rgb_pyramid_lut(None) == 0
    res, _dg = strm.run(arr, n, 0, n)
    assert res.status == 0
    got = [t.cpu().numpy() for t in ts]
    want = sp.pyramid(decoded[n - 1], levels, matrix, 0, loc)
    assert all(got[k][n - 1].tobytes() == want[k].tobytes() for k in range(2))
    assert strm.set_rgb_pyramid_output(None) == 0
    strm.close(); [j.close() for j in jobs]; dpb.close(); ctx.close()
