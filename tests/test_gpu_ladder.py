"""GPU: the output ladder on the device (k_output_ladder, openvvc_amd/csrc/kernels_ladder.hip) and the layers above it:
ovhip_ladder_launch against the numpy restatement tests/spec_ladder.py on the whole census -- every surface inside a sentinel buffer,
tight and loose layouts, strided sources --, the refusals, the synchronous convenience, the frame thread (whole and band-wise; with an
RGB output and a PACKED delivery of the one shown picture; behind film grain and behind a first reduce), and the stream driver's
slots.  The definition is integer only: every comparison is of bytes."""
import ctypes as C

import numpy as np
import pytest

import spec_film_grain as sf
import spec_ladder as sl
import spec_reduce as sd
import spec_rgb as sr
import spec_surface as ss
from openvvc_amd import capi, engine, gop
from test_film_grain_cpu import c_params
from test_gpu_reduce import _frame
from test_gpu_stream import _contents, _jobs_for, _make_contents, _stream_pics
from test_ladder_cpu import GUARD, assert_equals_want, c_format, sizes_of
from test_reduce_cpu import strided

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(built_lib):
    c = engine.Context(0)
    yield c
    c.close()


def device_buffers(ctx, rungs):
    """per rung a device buffer of its surface's size + GUARD that holds the sentinel, and the C rungs that point at them"""
    bufs = [ctx.upload(np.full(n + GUARD, ss.FILL, np.uint8)) for n in sizes_of(ctx.lib, rungs)]
    c_rungs = [engine.ladder_rung(w, h, c_format(fmt, rounding, lay), b.ptr.value, n)
               for (w, h, fmt, rounding, lay), b, n in zip(rungs, bufs, sizes_of(ctx.lib, rungs))]
    return bufs, c_rungs


def device_pic(ctx, planes, spad=0):
    h, w = planes[0].shape
    held = strided(planes, w + spad, w // 2 + spad)
    sb = [ctx.upload(a) for a in held]
    return sb, held, engine.DevPic(ctx, capi.Pic(sb[0].ptr.value, sb[1].ptr.value, sb[2].ptr.value, w, h, w + spad, w // 2 + spad), owns=False)


def device_ladder(ctx, planes, rungs, window=(0, 0, 0, 0), loc=0, spad=0):
    """ovhip_ladder_launch of the planes (rows of w + spad samples) -> the rungs' whole buffers, surface and guard"""
    sb, held, pic = device_pic(ctx, planes, spad)
    bufs, c_rungs = device_buffers(ctx, rungs)
    pic.ladder_into(c_rungs, window, loc)
    ctx.sync()
    got = [b.download() for b in bufs]
    assert all(np.array_equal(a.ravel(), b.download(np.uint16)) for a, b in zip(held, sb)), "the source is only read"
    [b.free() for b in sb + bufs]
    return got


@pytest.mark.parametrize("case", range(len(sl.CENSUS)))
def test_launch_equals_the_restatement_on_the_census(ctx, case):
    _size, win, rungs, locs = sl.CENSUS[case]
    planes = sl.census_planes(case)
    for loc in locs:
        assert_equals_want(device_ladder(ctx, planes, rungs, win, loc), sl.census_want(case, loc, GUARD), (case, loc))
    loc = locs[-1]
    assert_equals_want(device_ladder(ctx, planes, sl.loosened(rungs), win, loc), sl.census_want(case, loc, GUARD, True), (case, "loose layouts"))
    assert_equals_want(device_ladder(ctx, planes, rungs, win, loc, spad=6), sl.census_want(case, loc, GUARD), (case, "source strides w + 6"))
    assert_equals_want(device_ladder(ctx, planes, sl.loosened(rungs), win, loc, spad=6), sl.census_want(case, loc, GUARD, True), (case, "loose, strides"))
    if planes[0].shape[1] == 1024:
        full = [np.full_like(p, 1023) for p in planes]
        assert_equals_want(device_ladder(ctx, full, rungs), sl.ladder(full, rungs, guard=GUARD), "the int32 ceiling")


def test_refusals_write_nothing_on_the_device(ctx):
    """return values, the error text and the sentinels only: nothing is provoked on the device"""
    lib = ctx.lib
    planes = sd.random_planes(72, 40, 9)
    sb, _held, pic = device_pic(ctx, planes)
    good = [sl.rung(48, 24, sl.P010), sl.rung(36, 20, sl.NV12, sl.DITHER), sl.rung(72, 40, sl.I420)]
    bufs, c_rungs = device_buffers(ctx, good)
    err = lambda: lib.ovhip_last_error(ctx.h).decode()

    def untouched():
        ctx.sync()
        return all((b.download() == ss.FILL).all() for b in bufs)

    def rung_at(k, ptr, nbytes=None, size=None, fmt=None):
        w, h = size or good[k][:2]
        return engine.ladder_rung(w, h, fmt if fmt is not None else c_rungs[k].fmt, ptr, c_rungs[k].dst_bytes if nbytes is None else nbytes)

    EINVAL, EUNSUP = capi.OVHIP_EINVAL, capi.OVHIP_EUNSUP
    spare = ctx.upload(np.full(1 << 16, ss.FILL, np.uint8))
    # the reduced-size output's refusals, in the last position, with the rung's index
    assert pic.ladder_into(c_rungs + [rung_at(0, spare.ptr.value, 1 << 16, (8, 40))], check=False) == EUNSUP and "rung 3" in err() and "ratio" in err()
    assert pic.ladder_into(c_rungs + [rung_at(0, spare.ptr.value, 1 << 16, (144, 80))], check=False) == EUNSUP and "up-sampling" in err()
    assert pic.ladder_into(c_rungs + [rung_at(0, spare.ptr.value, 1 << 16, (34, 20))], check=False) == EINVAL and "rung 3" in err()
    assert untouched()
    # n out of range, null arguments
    arr, _n = engine._rung_array(c_rungs)
    assert lib.ovhip_ladder_launch(ctx.h, C.byref(pic.s), C.byref(capi.ReduceInfo()), arr, 0) == EINVAL and "rungs" in err()
    assert pic.ladder_into([rung_at(1, spare.ptr.value + 4096 * k) for k in range(sl.MAX_RUNGS + 1)], check=False) == EINVAL
    assert lib.ovhip_ladder_launch(ctx.h, None, C.byref(capi.ReduceInfo()), arr, 3) == EINVAL
    assert lib.ovhip_ladder_launch(ctx.h, C.byref(pic.s), None, arr, 3) == EINVAL and lib.ovhip_ladder_launch(ctx.h, C.byref(pic.s), C.byref(capi.ReduceInfo()), None, 3) == EINVAL
    assert lib.ovhip_ladder_launch(None, C.byref(pic.s), C.byref(capi.ReduceInfo()), arr, 3) == EINVAL
    # too small by one byte (last rung), a null destination, an unaligned 16-bit destination
    assert pic.ladder_into(c_rungs[:2] + [rung_at(2, bufs[2].ptr.value, c_rungs[2].dst_bytes - 1)], check=False) == EINVAL and "rung 2" in err() and "too small" in err()
    assert pic.ladder_into([c_rungs[0], rung_at(1, None)] + c_rungs[2:], check=False) == EINVAL and "rung 1" in err()
    assert pic.ladder_into([rung_at(0, bufs[0].ptr.value + 1, c_rungs[0].dst_bytes)] + c_rungs[1:], check=False) == EINVAL and "aligned" in err()
    # destinations that overlap one another, or the picture
    assert pic.ladder_into([c_rungs[0], rung_at(1, bufs[0].ptr.value + c_rungs[0].dst_bytes - 2)], check=False) == EINVAL and "overlaps rung 0" in err()
    assert pic.ladder_into(c_rungs[:2] + [rung_at(2, sb[0].ptr.value)], check=False) == EINVAL and "overlaps the picture" in err()
    # a format's refusal, reserved bytes, the window, a missing plane
    f = engine.surface_format(capi.SURF_P010, capi.SURF_DITHER)
    assert pic.ladder_into([rung_at(0, bufs[0].ptr.value, fmt=f)] + c_rungs[1:], check=False) == EINVAL and "rung 0" in err()
    rsv = capi.ReduceInfo()
    rsv.rsv[1] = 1
    assert lib.ovhip_ladder_launch(ctx.h, C.byref(pic.s), C.byref(rsv), arr, 3) == EINVAL
    assert pic.ladder_into(c_rungs, (18, 18, 0, 0), check=False) == EINVAL and pic.ladder_into(c_rungs, chroma_loc=6, check=False) == EINVAL
    s = capi.Pic(pic.s.y, None, pic.s.cr, 72, 40, 72, 36)
    assert engine.DevPic(ctx, s, owns=False).ladder_into(c_rungs, check=False) == EINVAL and "missing plane" in err()
    assert untouched()
    with pytest.raises(engine.EngineError):
        pic.ladder([engine.ladder_rung(36, 20), engine.ladder_rung(8, 40)])
    assert "rung 1" in err()
    assert pic.ladder_into(c_rungs) == 0 and not untouched()
    [b.free() for b in sb + bufs + [spare]]


def test_the_convenience_equals_the_launch(built_lib):
    ctx = engine.Context(0)
    for case in (1, 7):
        (w, h), win, rungs, locs = sl.CENSUS[case]
        planes = sl.census_planes(case)
        pic = ctx.upload_pic(*planes)
        got = pic.ladder([engine.ladder_rung(g[0], g[1], c_format(*g[2:])) for g in rungs], win, locs[-1])
        launched = device_ladder(ctx, planes, rungs, win, locs[-1])
        assert_equals_want(launched, sl.census_want(case, locs[-1], GUARD), case)
        for k, (g, (Wd, Hd, fmt, rounding, lay)) in enumerate(zip(got, rungs)):
            # (bytes a layout leaves out are 0 in the fetched array)
            want, size = ss.surface(sd.reduce_picture(*planes, Wd, Hd, win, locs[-1]), fmt, rounding, fill=0, **lay)
            assert g.nbytes == size and g.tobytes() == want.tobytes(), (case, k)
        held = ctx.scratch_bytes()
        assert [a.tobytes() for a in pic.ladder([engine.ladder_rung(g[0], g[1], c_format(*g[2:])) for g in rungs], win, locs[-1])] == [a.tobytes() for a in got]
        assert ctx.scratch_bytes() == held, "no allocation once the sizes have been seen"
        pic.free()
    ctx.close()


def _ladder_case(post):
    """(frame size, the ladder's rungs as descriptions, the picture the ladder reads from the decoded one)"""
    if post == "grain":
        sei = sf.make_sei(log2_scale=2, comps=((8, 3, 200, 8, 8), (3, 2, 100, 4, 6), (1, 1, 90, 8, 8)))
        return (88, 56), [sl.rung(88, 56, sl.P010), sl.rung(44, 28, sl.NV12, sl.DITHER), sl.rung(24, 8, sl.I420, loose=True)], sei
    if post == "reduce":
        return (72, 40), [sl.rung(48, 24, sl.I010), sl.rung(24, 12, sl.NV12, sl.DITHER, True), sl.rung(16, 8, sl.I420)], None
    return (72, 40), [sl.rung(72, 40, sl.NV12), sl.rung(48, 24, sl.P010, loose=True), sl.rung(24, 8, sl.I420, sl.DITHER)], None


@pytest.mark.parametrize("via", ["submit", "band"])
@pytest.mark.parametrize("post", ["none", "grain", "reduce"])
def test_frame_ladder_rgb_and_packed_read_the_one_shown_picture(built_lib, via, post):
    """a ladder of three rungs, an RGB output and a PACKED delivery of ONE picture: each equals that output of the picture the frame
    shows -- the decoded one, the grained one (the reason for the feature: a stream with an FGC SEI feeds a ladder), or a first
    reduce's; a following picture without a ladder leaves the sentinels alone; the scratch is constant from the second picture on"""
    lib = built_lib
    (w, h), rungs, sei = _ladder_case(post)
    wl, dpb, ctx, f, params = _frame(w, h)
    loc, poc = 2, 7
    ow, oh = (48, 24) if post == "reduce" else (w, h)
    if post == "grain":
        f.set_film_grain(c_params(sei), poc)
    elif post == "reduce":
        f.set_output_reduce(ow, oh, chroma_loc=loc)
    rgb_fmt = engine.rgb_format(1, 0, 0, capi.RGB_U8, capi.RGB_PLANAR)
    win = (1, 0, 0, 1)
    cwin = capi.Window(*win)
    n_rgb, n_packed = 3 * (ow - 2) * (oh - 2), lib.ovhip_output_bytes(ow, oh, C.byref(cwin))
    fctx = lib.ovhip_frame_ctx(f.f)

    def picture(key, outputs, ladder=True):
        d_rgb = ctx.upload(np.full(n_rgb + GUARD, ss.FILL, np.uint8))
        bufs, c_rungs = device_buffers(ctx, rungs)
        host = np.full(n_packed + GUARD, ss.FILL, np.uint8)
        out = capi.FrameOutput()
        out.mode, out.window, out.packed = (capi.OUT_PACKED if outputs else capi.OUT_NONE), cwin, host.ctypes.data
        if outputs:
            f.set_rgb_output(d_rgb.ptr.value, rgb_fmt, win, nbytes=n_rgb)
            if ladder:
                f.set_ladder_output(c_rungs, chroma_loc=loc)
        f.begin(key)
        f.recorder().replay(wl.calllog)
        if via == "submit":
            assert f.submit(params, out=out) == 0
        else:
            assert lib.ovhip_frame_set_band_mode(f.f, 1) == 0
            assert lib.ovhip_frame_band(f.f, C.byref(params), h, 1, C.byref(out)) == 1, lib.ovhip_frame_last_error(f.f)
            assert lib.ovhip_frame_set_band_mode(f.f, 0) == 0
        got = [b.download() for b in bufs], d_rgb.download(), host
        [b.free() for b in bufs + [d_rgb]]
        return got

    got = picture(0x100, True)
    held = lib.ovhip_ctx_scratch_bytes(fctx)
    _dev, held_pic = dpb.lookup(0x100)
    assert (held_pic.w, held_pic.h) == (w, h)
    dec = engine.DevPic(ctx, held_pic, owns=False).download()
    shown = sf.apply(dec, sei, poc)[0] if post == "grain" else (sd.reduce_picture(*dec, ow, oh, loc=loc) if post == "reduce" else dec)
    if post == "grain":
        assert not all(np.array_equal(a, b) for a, b in zip(shown, dec)), "the grain acts"
    assert_equals_want(got[0], sl.ladder(shown, rungs, loc=loc, guard=GUARD), (post, via, "the ladder of the shown picture"))
    assert got[2][:n_packed].tobytes() == sd.packed(shown, win).tobytes() and (got[2][n_packed:] == ss.FILL).all(), "PACKED"
    want_rgb = sr.convert(*shown, 1, 0, 0, sr.U8, sr.PLANAR, win)
    assert got[1][:n_rgb].tobytes() == np.ascontiguousarray(want_rgb).tobytes() and (got[1][n_rgb:] == ss.FILL).all(), "RGB"
    # the setting ended with the picture: nothing set, then RGB alone -- the rungs' buffers keep the sentinel
    idle = picture(0x101, False)
    assert all((b == ss.FILL).all() for b in idle[0]) and (idle[1] == ss.FILL).all() and (idle[2] == ss.FILL).all()
    alone = picture(0x102, True, ladder=False)
    assert all((b == ss.FILL).all() for b in alone[0]) and alone[1].tobytes() == got[1].tobytes()
    again = picture(0x103, True)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got[0], again[0])) and again[1].tobytes() == got[1].tobytes()
    assert lib.ovhip_ctx_scratch_bytes(fctx) == held, "constant from the second picture on"
    # a ladder the picture's last call refuses fails that call, not the publication, and writes nothing
    bufs, c_rungs = device_buffers(ctx, rungs)
    c_rungs[-1].dst_bytes -= 1
    assert f.set_ladder_output(c_rungs, chroma_loc=loc) == 0
    f.begin(0x104)
    f.recorder().replay(wl.calllog)
    assert f.submit(params, check=False) == capi.OVHIP_EINVAL
    assert dpb.lookup(0x104)[1].w == w
    ctx.sync()
    assert all((b.download() == ss.FILL).all() for b in bufs)
    [b.free() for b in bufs]
    # the setter's own refusals; off
    assert f.set_ladder_output([], check=False) == capi.OVHIP_EINVAL
    assert f.set_ladder_output([engine.ladder_rung(ow * 2, oh * 2, None, 4096, 1 << 20)], check=False) == capi.OVHIP_EUNSUP
    assert f.set_ladder_output([engine.ladder_rung(ow, oh, None, None, 1 << 20)], check=False) == capi.OVHIP_EINVAL
    assert f.set_ladder_output(None) == 0 and lib.ovhip_frame_set_ladder_output(None, None, None, 0) == capi.OVHIP_EINVAL
    f.close(); ctx.close(); dpb.close()


def test_stream_writes_a_two_rung_ladder_into_slots(built_lib):
    import torch
    w, h = 416, 240
    sizes = [(208, 120), (104, 60)]
    wls = _contents(w, h, (41, 42), 43)
    spics = _stream_pics(gop.build_stream(1, 4, 4, 1), 2)                               # I and one GOP of 4
    n = len(spics)
    ctx = engine.Context(0)
    dpb = engine.Dpb((0,))
    jobs = _jobs_for(ctx, wls, spics, w, h)
    st = engine.Stream(dpb, w, h, _make_contents(wls), jobs, threads_per_device=4)
    arr = st.pics_array(spics)
    fmts = [engine.surface_format(capi.SURF_NV12), engine.surface_format(capi.SURF_P010)]
    need = [built_lib.ovhip_surface_bytes(ow, oh, None, C.byref(f)) for (ow, oh), f in zip(sizes, fmts)]
    assert need == [208 * 120 * 3 // 2, 104 * 60 * 3]
    pad = 32                                                                            # (a slot larger than the surface)
    ts = [torch.full((n, nb + pad), ss.FILL, dtype=torch.uint8, device="cuda:0") for nb in need]
    torch.cuda.synchronize()
    rungs = [engine.ladder_rung(ow, oh, f, t, slots=True) for (ow, oh), f, t in zip(sizes, fmts, ts)]
    assert [g.dst_bytes for g in rungs] == [nb + pad for nb in need]
    with pytest.raises(engine.EngineError):
        engine.ladder_rung(208, 120, fmts[0], torch.zeros((n, need[0] - 1), dtype=torch.uint8, device="cuda:0"), slots=True)
    assert st.set_ladder_output([engine.ladder_rung(208, 120, fmts[0], ts[0].data_ptr(), need[0] - 1)], n_slots=n, check=False) == capi.OVHIP_EINVAL
    assert st.set_ladder_output([engine.ladder_rung(208, 120, fmts[0], ts[0].data_ptr(), need[0])], n_slots=0, check=False) == capi.OVHIP_EINVAL
    assert st.set_ladder_output([engine.ladder_rung(832, 480, fmts[0], ts[0].data_ptr(), 1 << 20)], n_slots=n, check=False) == capi.OVHIP_EUNSUP
    assert st.set_ladder_output(rungs, chroma_loc=1) == 0
    res, _dg = st.run(arr, n, 0, n, flags=capi.STREAM_KEEP | capi.STREAM_HOLD_ALL)
    assert res.status == 0 and res.n_decoded == n
    got = [t.cpu().numpy() for t in ts]
    for i in range(n):                                                                  # every picture of the run, each in its own slot
        want = sl.ladder(st.picture(i, ctx).download(), [sl.rung(*sizes[0], sl.NV12), sl.rung(*sizes[1], sl.P010)], loc=1, guard=pad)
        for k in range(2):
            assert got[k][i].tobytes() == want[k][0].tobytes(), (i, k)
    assert st.set_ladder_output(None) == 0
    st.close(); [j.close() for j in jobs]; dpb.close(); ctx.close()
