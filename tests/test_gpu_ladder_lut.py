"""GPU: the output ladder through a colour table on the device (k_ladder_lut, openvvc_amd/csrc/kernels_ladder_lut.hip) and the layers
above it: ovhip_ladder_lut_launch against the numpy restatement tests/spec_ladder_lut.py on the whole census -- every surface inside a
sentinel buffer, tight and loose layouts, strided sources --, the refusals, the synchronous convenience, the scratch, the frame thread
(whole and band-wise; behind film grain and behind a first reduce; against the frame's own surface output through a table; the three
tables' independence) and the stream driver's slots.  The definition is integer only: every comparison is of bytes."""
import ctypes as C

import numpy as np
import pytest

import spec_film_grain as sf
import spec_ladder as sl
import spec_ladder_lut as sx
import spec_reduce as sd
import spec_rgb as sr
import spec_rgb_lut as st
import spec_surface as ss
import spec_surface_lut as ssl
from openvvc_amd import capi, engine, gop
from test_film_grain_cpu import c_params
from test_gpu_ladder import _ladder_case, device_buffers, device_pic
from test_gpu_reduce import _frame
from test_gpu_stream import _contents, _jobs_for, _make_contents, _stream_pics
from test_ladder_cpu import GUARD, assert_equals_want, c_format

pytestmark = pytest.mark.gpu
EINVAL, EUNSUP = capi.OVHIP_EINVAL, capi.OVHIP_EUNSUP


@pytest.fixture(scope="module")
def ctx(built_lib):
    c = engine.Context(0)
    yield c
    c.close()


def device_ladder(ctx, lut, planes, rungs, conv, window=(0, 0, 0, 0), spad=0):
    """ovhip_ladder_lut_launch of the planes (rows of w + spad samples) -> the rungs' whole buffers, surface and guard"""
    sb, held, pic = device_pic(ctx, planes, spad)
    bufs, c_rungs = device_buffers(ctx, rungs)
    pic.ladder_into(c_rungs, window, lut=lut, conv=engine.surface_conv(*conv))
    ctx.sync()
    got = [b.download() for b in bufs]
    assert all(np.array_equal(a.ravel(), b.download(np.uint16)) for a, b in zip(held, sb)), "the source is only read"
    [b.free() for b in sb + bufs]
    return got


@pytest.mark.parametrize("case", list(sx.CENSUS))
def test_launch_equals_the_restatement_on_the_census(ctx, case):
    _size, win, rungs, (_s, peak), combos = sx.CENSUS[case]
    planes, table = sx.census_planes(case), sx.census_table(case)
    with engine.RgbLut(ctx, table, peak) as lut:
        for k, combo in enumerate(combos):
            assert_equals_want(device_ladder(ctx, lut, planes, rungs, sx.conv_of(*combo), win), sx.census_want(case, k, GUARD), (case, combo))
        if case != "D":                                       # (the large case runs once)
            k = len(combos) - 1
            conv = sx.conv_of(*combos[k])
            assert_equals_want(device_ladder(ctx, lut, planes, sx.loosened(rungs), conv, win), sx.census_want(case, k, GUARD, True), (case, "loose layouts"))
            assert_equals_want(device_ladder(ctx, lut, planes, rungs, conv, win, spad=6), sx.census_want(case, k, GUARD), (case, "source strides w + 6"))
            assert_equals_want(device_ladder(ctx, lut, planes, sx.loosened(rungs), conv, win, spad=6), sx.census_want(case, k, GUARD, True), (case, "loose, strides"))


def test_refusals_write_nothing_on_the_device(ctx):
    """return values, the error text and the sentinels only: nothing is provoked on the device"""
    lib = ctx.lib
    planes = sx.ramp_planes(72, 40, 9)
    sb, _held, pic = device_pic(ctx, planes)
    good = [sx.rung(48, 24, sx.P010), sx.rung(36, 20, sx.NV12, sx.DITHER), sx.rung(72, 40, sx.I420)]
    bufs, c_rungs = device_buffers(ctx, good)
    lut = engine.RgbLut(ctx, st.random_table(17, 1023, 5), 1023)
    conv = engine.surface_conv(*sx.conv_of(0, 0))
    err = lambda: lib.ovhip_last_error(ctx.h).decode()

    def into(rungs=c_rungs, window=(0, 0, 0, 0), chroma_loc=None, cv=conv, table=lut):
        return pic.ladder_into(rungs, window, chroma_loc, check=False, lut=table, conv=cv)

    def untouched():
        ctx.sync()
        return all((b.download() == ss.FILL).all() for b in bufs)

    def rung_at(k, ptr, nbytes=None, size=None, fmt=None):
        w, h = size or good[k][:2]
        return engine.ladder_rung(w, h, fmt if fmt is not None else c_rungs[k].fmt, ptr, c_rungs[k].dst_bytes if nbytes is None else nbytes)

    spare = ctx.upload(np.full(1 << 16, ss.FILL, np.uint8))
    # everything the plain ladder refuses, with the rung's index
    assert into(c_rungs + [rung_at(0, spare.ptr.value, 1 << 16, (8, 40))]) == EUNSUP and "rung 3" in err() and "ratio" in err()
    assert into(c_rungs + [rung_at(0, spare.ptr.value, 1 << 16, (144, 80))]) == EUNSUP and "up-sampling" in err()
    assert into(c_rungs + [rung_at(0, spare.ptr.value, 1 << 16, (34, 20))]) == EINVAL and "rung 3" in err()
    arr, _n = engine._rung_array(c_rungs)
    assert lib.ovhip_ladder_lut_launch(ctx.h, C.byref(pic.s), C.byref(capi.ReduceInfo()), arr, 0, C.byref(conv), lut.h) == EINVAL and "rungs" in err()
    assert into([rung_at(1, spare.ptr.value + 4096 * k) for k in range(sx.MAX_RUNGS + 1)]) == EINVAL
    assert lib.ovhip_ladder_lut_launch(ctx.h, None, C.byref(capi.ReduceInfo()), arr, 3, C.byref(conv), lut.h) == EINVAL
    assert lib.ovhip_ladder_lut_launch(ctx.h, C.byref(pic.s), None, arr, 3, C.byref(conv), lut.h) == EINVAL
    assert lib.ovhip_ladder_lut_launch(ctx.h, C.byref(pic.s), C.byref(capi.ReduceInfo()), None, 3, C.byref(conv), lut.h) == EINVAL
    assert lib.ovhip_ladder_lut_launch(None, C.byref(pic.s), C.byref(capi.ReduceInfo()), arr, 3, C.byref(conv), lut.h) == EINVAL
    assert into(c_rungs[:2] + [rung_at(2, bufs[2].ptr.value, c_rungs[2].dst_bytes - 1)]) == EINVAL and "rung 2" in err() and "too small" in err()
    assert into([c_rungs[0], rung_at(1, None)] + c_rungs[2:]) == EINVAL and "rung 1" in err()
    assert into([rung_at(0, bufs[0].ptr.value + 1, c_rungs[0].dst_bytes)] + c_rungs[1:]) == EINVAL and "aligned" in err()
    assert into([c_rungs[0], rung_at(1, bufs[0].ptr.value + c_rungs[0].dst_bytes - 2)]) == EINVAL and "overlaps rung 0" in err()
    assert into(c_rungs[:2] + [rung_at(2, sb[0].ptr.value)]) == EINVAL and "overlaps the picture" in err()
    f = engine.surface_format(capi.SURF_P010, capi.SURF_DITHER)
    assert into([rung_at(0, bufs[0].ptr.value, fmt=f)] + c_rungs[1:]) == EINVAL and "rung 0" in err()
    assert into(window=(18, 18, 0, 0)) == EINVAL and into(chroma_loc=6) == EINVAL
    s = capi.Pic(pic.s.y, None, pic.s.cr, 72, 40, 72, 36)
    assert engine.DevPic(ctx, s, owns=False).ladder_into(c_rungs, check=False, lut=lut, conv=conv) == EINVAL and "missing plane" in err()
    assert untouched()
    # the conversion's own refusals with their codes; the table; the two sample locations
    assert into(cv=None) == EINVAL and "conversion" in err()
    assert into(cv=engine.surface_conv(dst_chroma_loc=4)) == EUNSUP and into(cv=engine.surface_conv(dst_matrix=2)) == EINVAL
    assert into(cv=engine.surface_conv(src_matrix=3)) == EUNSUP
    assert into(table=None) == EINVAL and "null table" in err()
    assert into(chroma_loc=1) == EINVAL and "location" in err()
    assert into(cv=engine.surface_conv(*sx.conv_of(2, 0)), chroma_loc=0) == EINVAL and "location" in err()
    assert untouched()
    with pytest.raises(engine.EngineError):
        pic.ladder([engine.ladder_rung(36, 20), engine.ladder_rung(8, 40)], lut=lut, conv=conv)
    assert "rung 1" in err()
    assert into(cv=engine.surface_conv(*sx.conv_of(2, 0))) == 0 and not untouched()      # (chroma_loc left alone: the conversion's)
    lut.close()
    [b.free() for b in sb + bufs + [spare]]


def test_the_convenience_equals_the_launch_and_the_scratch_stays_flat(built_lib):
    ctx = engine.Context(0)
    for case in ("C1", "C7"):
        _size, win, rungs, (_s, peak), combos = sx.CENSUS[case]
        planes, table, conv = sx.census_planes(case), sx.census_table(case), sx.conv_of(*combos[0])
        pic = ctx.upload_pic(*planes)
        plain = [engine.ladder_rung(g[0], g[1], c_format(*g[2:])) for g in rungs]
        with engine.RgbLut(ctx, table, peak) as lut:
            before = ctx.scratch_bytes()
            bufs, c_rungs = device_buffers(ctx, rungs)
            for rep in range(3):
                pic.ladder_into(c_rungs, win, lut=lut, conv=engine.surface_conv(*conv))
            ctx.sync()
            assert ctx.scratch_bytes() == before, "the launch allocates nothing"
            launched = [b.download() for b in bufs]
            [b.free() for b in bufs]
            assert_equals_want(launched, sx.census_want(case, 0, GUARD), case)
            got = pic.ladder(plain, win, lut=lut, conv=engine.surface_conv(*conv))
            red = sx.census_reduced(case, conv[2])
            for k, (g, (Wd, Hd, fmt, rounding, lay)) in enumerate(zip(got, rungs)):
                # (bytes a layout leaves out are 0 in the fetched array)
                want, size = ss.surface(ssl.converted(red[k], conv, table, peak), fmt, rounding, fill=0, **lay)
                assert g.nbytes == size and g.tobytes() == want.tobytes(), (case, k)
            held = ctx.scratch_bytes()
            for rep in range(2):
                assert [a.tobytes() for a in pic.ladder(plain, win, lut=lut, conv=engine.surface_conv(*conv))] == [a.tobytes() for a in got]
            assert ctx.scratch_bytes() == held, "no allocation once the sizes have been seen"
        pic.free()
    ctx.close()


@pytest.mark.parametrize("via", ["submit", "band"])
@pytest.mark.parametrize("post", ["none", "grain", "reduce"])
def test_frame_ladder_goes_through_the_table_until_it_is_cleared(built_lib, via, post):
    """with the table set the rungs are those of the converted reduced pictures of the picture the frame shows -- the decoded one, the
    grained one or a first reduce's; cleared, they are ovhip_ladder_launch's bytes again; a refused ladder fails the call, not the
    publication"""
    lib = built_lib
    (w, h), rungs, sei = _ladder_case(post)
    wl, dpb, ctx, f, params = _frame(w, h)
    loc, poc = 2, 7
    conv = sx.conv_of(loc, 1)
    table, peak = st.random_table(17, 4000, 21), 4000
    lut = engine.RgbLut(ctx, table, peak)
    ow, oh = (48, 24) if post == "reduce" else (w, h)
    if post == "grain":
        f.set_film_grain(c_params(sei), poc)
    elif post == "reduce":
        f.set_output_reduce(ow, oh, chroma_loc=loc)

    def picture(key, c_rungs, check=True):
        f.set_ladder_output(c_rungs, chroma_loc=loc)
        f.begin(key)
        f.recorder().replay(wl.calllog)
        if via == "submit":
            return f.submit(params, check=check)
        assert lib.ovhip_frame_set_band_mode(f.f, 1) == 0
        r = lib.ovhip_frame_band(f.f, C.byref(params), h, 1, None)
        assert lib.ovhip_frame_set_band_mode(f.f, 0) == 0
        return 0 if r == 1 else r

    def ladder_of(key):
        bufs, c_rungs = device_buffers(ctx, rungs)
        assert picture(key, c_rungs) == 0
        got = [b.download() for b in bufs]
        [b.free() for b in bufs]
        return got

    f.set_ladder_lut(lut, engine.surface_conv(*conv))
    got = ladder_of(0x100)
    _dev, held_pic = dpb.lookup(0x100)
    dec = engine.DevPic(ctx, held_pic, owns=False).download()
    shown = sf.apply(dec, sei, poc)[0] if post == "grain" else (sd.reduce_picture(*dec, ow, oh, loc=loc) if post == "reduce" else dec)
    want = sx.ladder(shown, rungs, conv, table, peak, guard=GUARD)
    assert_equals_want(got, want, (post, via, "the converted ladder of the shown picture"))
    assert_equals_want(ladder_of(0x101), want, "sticky: the next picture too")
    # a ladder the picture's last call refuses fails that call, not the publication, and writes nothing
    bufs, c_rungs = device_buffers(ctx, rungs)
    c_rungs[-1].dst_bytes -= 1
    assert picture(0x102, c_rungs, check=False) == EINVAL
    assert dpb.lookup(0x102)[1].w == w
    ctx.sync()
    assert all((b.download() == ss.FILL).all() for b in bufs)
    [b.free() for b in bufs]
    # the location: from whichever setter comes second
    bufs, c_rungs = device_buffers(ctx, rungs)
    assert f.set_ladder_output(c_rungs, chroma_loc=0, check=False) == EINVAL
    assert f.set_ladder_output(c_rungs, chroma_loc=loc) == 0 and f.set_ladder_lut(lut, engine.surface_conv(*sx.conv_of(0, 1)), check=False) == EINVAL
    assert f.set_ladder_output(None) == 0
    [b.free() for b in bufs]
    assert f.set_ladder_lut(lut, None, check=False) == EINVAL and f.set_ladder_lut(lut, engine.surface_conv(dst_chroma_loc=4), check=False) == EUNSUP
    assert_equals_want(ladder_of(0x103), want, "the setter's refusals leave the setting as it was")
    # cleared: the plain ladder's bytes
    f.set_ladder_lut(None)
    assert_equals_want(ladder_of(0x104), sl.ladder(shown, rungs, loc=loc, guard=GUARD), "cleared")
    lut.close()
    f.close(); ctx.close(); dpb.close()


def test_frame_rung_equals_the_frames_own_reduced_surface_through_the_table(built_lib):
    """a rung is what the same frame writes as its surface with set_output_reduce to that size in front of set_surface_lut; the RGB
    table, the surface table and the ladder table are independent"""
    (w, h), _rungs, _sei = _ladder_case("none")
    wl, dpb, ctx, f, params = _frame(w, h)
    loc = 0
    conv = sx.conv_of(loc, 2)
    t_lad, t_surf, t_rgb = st.random_table(17, 1023, 31), st.random_table(33, 255, 32), st.random_table(17, 255, 33)
    lut_lad, lut_surf, lut_rgb = engine.RgbLut(ctx, t_lad, 1023), engine.RgbLut(ctx, t_surf, 255), engine.RgbLut(ctx, t_rgb, 255)
    rung = sx.rung(48, 24, sx.NV12, sx.DITHER)
    rgb_fmt = engine.rgb_format(9, 0, 0, capi.RGB_U8, capi.RGB_PLANAR)
    surf_fmt = engine.surface_format(capi.SURF_NV12, capi.SURF_DITHER)
    need = 48 * 24 * 3 // 2
    key = [0x200]

    def picture(reduce_first, ladder, surface, rgb_bytes=0):
        bufs, c_rungs = device_buffers(ctx, [rung] if ladder else [])
        d_surf = ctx.upload(np.full(w * h * 3, ss.FILL, np.uint8))
        d_rgb = ctx.upload(np.full(3 * w * h, ss.FILL, np.uint8))
        f.set_output_reduce(*((48, 24, (0, 0, 0, 0), loc) if reduce_first else (0, 0)))
        if ladder:
            f.set_ladder_output(c_rungs, chroma_loc=loc)
        if surface:
            f.set_surface_output(d_surf.ptr.value, surf_fmt, nbytes=surface)
        if rgb_bytes:
            f.set_rgb_output(d_rgb.ptr.value, rgb_fmt, nbytes=rgb_bytes)
        f.begin(key[0])
        f.recorder().replay(wl.calllog)
        assert f.submit(params) == 0
        key[0] += 1
        got = [b.download() for b in bufs], d_surf.download(), d_rgb.download()
        [b.free() for b in bufs + [d_surf, d_rgb]]
        return got

    f.set_ladder_lut(lut_lad, engine.surface_conv(*conv))
    f.set_surface_lut(lut_lad, engine.surface_conv(*conv))
    rungs_got, _s, _r = picture(False, True, 0)
    _l, surf_got, _r = picture(True, False, need)
    assert rungs_got[0][:need].tobytes() == surf_got[:need].tobytes() and (rungs_got[0][need:] == ss.FILL).all()
    dec = engine.DevPic(ctx, dpb.lookup(0x200)[1], owns=False).download()
    assert rungs_got[0].tobytes() == sx.ladder(dec, [rung], conv, t_lad, 1023, guard=GUARD)[0][0].tobytes()
    # three tables at once, each output its own; then each cleared alone
    full = w * h * 3 // 2
    want_lad = {True: sx.ladder(dec, [rung], conv, t_lad, 1023, guard=GUARD)[0][0], False: sl.ladder(dec, [rung], loc=loc, guard=GUARD)[0][0]}
    want_surf = {True: ssl.surface(dec, conv, t_surf, 255, ss.NV12, ss.DITHER)[0], False: ss.surface(dec, ss.NV12, ss.DITHER)[0]}
    want_rgb = {True: st.convert(*dec, 9, 0, 0, sr.U8, sr.PLANAR, t_rgb, 255), False: sr.convert(*dec, 9, 0, 0, sr.U8, sr.PLANAR)}
    for a, b, c in ((True, True, True), (False, True, True), (True, False, True), (True, True, False), (False, False, False)):
        f.set_ladder_lut(lut_lad if a else None, engine.surface_conv(*conv) if a else None)
        f.set_surface_lut(lut_surf if b else None, engine.surface_conv(*conv) if b else None)
        f.set_rgb_lut(lut_rgb if c else None)
        lad, surf, rgb = picture(False, True, full, 3 * w * h)
        assert lad[0].tobytes() == want_lad[a].tobytes(), (a, b, c)
        assert surf[:full].tobytes() == want_surf[b].tobytes(), (a, b, c)
        assert rgb.tobytes() == np.ascontiguousarray(want_rgb[c]).tobytes(), (a, b, c)
    [x.close() for x in (lut_lad, lut_surf, lut_rgb)]
    f.close(); ctx.close(); dpb.close()


def test_stream_writes_a_two_rung_converted_ladder_into_slots(built_lib):
    import torch
    w, h = 416, 240
    sizes = [(208, 120), (104, 60)]
    wls = _contents(w, h, (41, 42), 43)
    spics = _stream_pics(gop.build_stream(1, 4, 4, 1), 2)                               # I and one GOP of 4
    n = len(spics)
    ctx = engine.Context(0)
    dpb = engine.Dpb((0,))
    jobs = _jobs_for(ctx, wls, spics, w, h)
    strm = engine.Stream(dpb, w, h, _make_contents(wls), jobs, threads_per_device=4)
    arr = strm.pics_array(spics)
    fmts = [engine.surface_format(capi.SURF_NV12), engine.surface_format(capi.SURF_P010)]
    need = [built_lib.ovhip_surface_bytes(ow, oh, None, C.byref(f)) for (ow, oh), f in zip(sizes, fmts)]
    pad = 32                                                                            # (a slot larger than the surface)
    ts = [torch.full((n, nb + pad), ss.FILL, dtype=torch.uint8, device="cuda:0") for nb in need]
    torch.cuda.synchronize()
    rungs = [engine.ladder_rung(ow, oh, f, t, slots=True) for (ow, oh), f, t in zip(sizes, fmts, ts)]
    table, peak, conv = st.random_table(17, 1023, 51), 1023, sx.conv_of(1, 0)
    assert strm.set_ladder_lut(table, peak, engine.surface_conv(*conv)) == 0
    assert strm.set_ladder_output(rungs, chroma_loc=0, check=False) == EINVAL             # (the second setter: another location than the conversion's)
    assert strm.set_ladder_output(rungs, chroma_loc=1) == 0
    assert strm.set_ladder_lut(table, peak, engine.surface_conv(*sx.conv_of(0, 0)), check=False) == EINVAL
    bad = table.copy()
    bad[0, 0, 0, 0] = 1024
    assert strm.set_ladder_lut(bad, peak, engine.surface_conv(*conv), check=False) == EINVAL
    assert strm.set_ladder_lut(table, peak, None, check=False) == EINVAL                  # (on a refusal the previous setting stands)
    res, _dg = strm.run(arr, n, 0, n, flags=capi.STREAM_KEEP | capi.STREAM_HOLD_ALL)
    assert res.status == 0 and res.n_decoded == n
    got = [t.cpu().numpy() for t in ts]
    decoded = [strm.picture(i, ctx).download() for i in range(n)]
    spec = [sx.rung(*sizes[0], sx.NV12), sx.rung(*sizes[1], sx.P010)]
    for i in range(n):                                                                  # every picture of the run, each in its own slot
        want = sx.ladder(decoded[i], spec, conv, table, peak, guard=pad)
        for k in range(2):
            assert got[k][i].tobytes() == want[k][0].tobytes(), (i, k)
    # cleared: the plain ladder
    assert strm.set_ladder_lut(None) == 0
    res, _dg = strm.run(arr, n, 0, n)
    assert res.status == 0
    got = [t.cpu().numpy() for t in ts]
    want = sl.ladder(decoded[n - 1], spec, loc=1, guard=pad)
    assert all(got[k][n - 1].tobytes() == want[k][0].tobytes() for k in range(2))
    assert strm.set_ladder_output(None) == 0
    strm.close(); [j.close() for j in jobs]; dpb.close(); ctx.close()
