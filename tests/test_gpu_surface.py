"""GPU: surface output on the device (openvvc_amd/csrc/kernels_surface.hip): ovhip_surface_launch and ovhip_pic_output_surface against
the host twin and the numpy restatement tests/spec_surface.py -- layouts with gaps, destinations that are only element-aligned, odd
pitches, strided pictures --, the frame thread (alone, with film grain, with an output scale, band-wise, beside the RGB output), the
stream driver into a torch tensor.  The definition is integer only: every comparison is of bytes."""
import ctypes as C

import numpy as np
import pytest

import spec_film_grain as sf
import spec_pp_scale as spp
import spec_rgb as sr
import spec_surface as ss
from openvvc_amd import capi, engine, gop, synth
from test_film_grain_cpu import c_params
from test_gpu_pic_hash import _frame_case
from test_gpu_stream import _Keep, _contents, _jobs_for, _make_contents, _stream_pics
from test_surface_cpu import c_format, host_surface

pytestmark = pytest.mark.gpu
GUARD = 16                                                    # bytes behind the surface that must stay as they were


@pytest.fixture(scope="module")
def ctx(built_lib):
    c = engine.Context(0)
    yield c
    c.close()


def _a5(ctx, nbytes):
    return ctx.upload(np.full(nbytes, ss.FILL, np.uint8))


def _launched(ctx, pic, fmt, rounding, wd, lead=0, **lay):
    """ovhip_surface_launch into a buffer of `lead` + surface + GUARD bytes that held 0xA5 -> the whole buffer"""
    cf, win = c_format(fmt, rounding, **lay), capi.Window(*wd)
    need = ctx.lib.ovhip_surface_bytes(pic.w, pic.h, C.byref(win), C.byref(cf))
    assert need
    d = _a5(ctx, lead + need + GUARD)
    pic.surface_into(d.ptr.value + lead, need, cf, wd)
    ctx.sync()
    raw = d.download()
    d.free()
    return raw


def _check(ctx, pic, planes, fmt, rounding, wd, lead=0, convenience=True, **lay):
    what = (pic.w, pic.h, fmt, rounding, wd, lead, lay)
    raw = _launched(ctx, pic, fmt, rounding, wd, lead, **lay)
    body, size = ss.surface(planes, fmt, rounding, wd, total=len(raw) - lead, **lay)
    assert size == len(raw) - lead - GUARD, what
    assert (raw[:lead] == ss.FILL).all(), what
    assert raw[lead:].tobytes() == body.tobytes(), what
    twin, need = host_surface(ctx.lib, planes, fmt, rounding, wd, **lay)
    assert need == size and twin[:need + GUARD].tobytes() == body.tobytes(), what
    if convenience:
        host = np.full(size + GUARD, ss.FILL, np.uint8)
        cf, win = c_format(fmt, rounding, **lay), capi.Window(*wd)
        assert ctx.lib.ovhip_pic_output_surface(ctx.h, C.byref(pic.s), C.byref(win), C.byref(cf), host.ctypes.data, size) == 0, what
        assert host.tobytes() == body.tobytes(), what


@pytest.mark.parametrize("w,h", ss.SIZES)
def test_launch_and_convenience_equal_host_and_restatement(ctx, w, h):
    planes = ss.random_planes(w, h, 31 * w + h)
    pic = ctx.upload_pic(*planes)
    for fmt, rounding in ss.MODES:
        for wd in (ss.windows_for(w, h) if (w, h) == (72, 40) else ss.WINDOWS[:1]):
            _check(ctx, pic, planes, fmt, rounding, wd)
        assert pic.surface(c_format(fmt, rounding)).tobytes() == ss.surface(planes, fmt, rounding)[0].tobytes()
    assert all(np.array_equal(a, b) for a, b in zip(pic.download(), planes)), "the picture is only read"
    pic.free()


@pytest.mark.parametrize("w,h", ss.SIZES)
def test_layouts_with_gaps_leave_the_gaps_unwritten(ctx, w, h):
    planes = ss.random_planes(w, h, 7 * w + h)
    pic = ctx.upload_pic(*planes)
    for fmt, rounding in ss.MODES:
        for wd in ss.windows_for(w, h):
            W, H = w - 2 * (wd[0] + wd[1]), h - 2 * (wd[2] + wd[3])
            _check(ctx, pic, planes, fmt, rounding, wd, **ss.loose_layout(fmt, W, H))
    pic.free()


@pytest.mark.parametrize("w,h,wd", [(20, 12, (0, 0, 0, 0)), (72, 40, (1, 0, 0, 1)), (136, 72, (0, 0, 0, 0)), (264, 136, (0, 1, 1, 0))])
def test_a_destination_offset_by_one_element_and_an_odd_pitch(ctx, w, h, wd):
    """a base that is aligned to its element and to nothing more, bases at 4 and 8 bytes, and a luma pitch of one element more than the
    row: runs start at every alignment, so the element path and the 4- and 8-byte paths are all taken; the bytes around stay"""
    planes = ss.random_planes(w, h, 9)
    pic = ctx.upload_pic(*planes)
    W = w - 2 * (wd[0] + wd[1])
    for fmt, rounding in ss.MODES:
        es = ss.ELEM[fmt]
        for lead in (es, 3 * es, 4, 8, 16 + es):
            _check(ctx, pic, planes, fmt, rounding, wd, lead=lead, convenience=False)
        for lead in (0, es):
            _check(ctx, pic, planes, fmt, rounding, wd, lead=lead, convenience=False, pitch_y=(W + 1) * es)
            _check(ctx, pic, planes, fmt, rounding, wd, lead=lead, convenience=False, pitch_y=(W + 2) * es, pitch_c=(W + 4) * es)
    pic.free()


def test_views_with_a_stride_above_their_width_and_a_band(ctx):
    """the left 72 columns of a 136x72 picture as a picture of its own (chroma rows of stride 68: not 16-byte aligned from row to
    row), the same view moved 4 and 6 columns to the right (luma rows 8 and 12 bytes off, chroma rows 4 and 6), and a band of rows"""
    planes = ss.random_planes(136, 72, 3)
    pic = ctx.upload_pic(*planes)
    for x in (0, 4, 6):
        s = capi.Pic(pic.s.y + 2 * x, pic.s.cb + x, pic.s.cr + x, 72, 72, pic.s.stride_y, pic.s.stride_c)
        view = engine.DevPic(ctx, s, owns=False)
        part = (planes[0][:, x:x + 72], planes[1][:, x // 2:x // 2 + 36], planes[2][:, x // 2:x // 2 + 36])
        for fmt, rounding in ss.MODES:
            for wd in ss.WINDOWS:
                _check(ctx, view, part, fmt, rounding, wd, convenience=(x == 0))
    band = pic.band(16, 24)
    part = (planes[0][16:40], planes[1][8:20], planes[2][8:20])
    for fmt, rounding in ss.MODES:
        _check(ctx, band, part, fmt, rounding, (0, 1, 1, 0))
    pic.free()


def test_i010_tight_is_the_packed_output(ctx):
    for w, h in ss.SIZES:
        pic = ctx.upload_pic(*ss.random_planes(w, h, 40 + w))
        for wd in ss.windows_for(w, h):
            assert pic.surface(c_format(ss.I010), wd).tobytes() == pic.output(wd).tobytes(), (w, h, wd)
        pic.free()


def test_scratch_stays_flat_over_repeated_calls(built_lib):
    ctx = engine.Context(0)
    pic = ctx.upload_pic(*ss.random_planes(264, 136, 1))
    d = ctx.alloc(264 * 136 * 3 + 4096)
    before = ctx.scratch_bytes()
    for rep in range(3):
        for fmt, rounding in ss.MODES:
            pic.surface_into(d.ptr.value, d.nbytes, c_format(fmt, rounding))
    ctx.sync()
    assert ctx.scratch_bytes() == before, "the launch allocates nothing"
    first = pic.surface(c_format(ss.P010, 0, **ss.loose_layout(ss.P010, 264, 136)))       # the convenience: its scratch at the largest size first
    held = ctx.scratch_bytes()
    assert held - before >= first.nbytes
    for rep in range(2):
        for fmt, rounding in ss.MODES:
            pic.surface(c_format(fmt, rounding), (1, 0, 0, 1))
            assert ctx.scratch_bytes() == held
    d.free(); pic.free(); ctx.close()


def test_refusals_come_back_before_anything_is_launched(ctx):
    """return values and the error text only: nothing is provoked on the device, and the destination stays as it was"""
    w, h = 72, 40
    pic = ctx.upload_pic(*ss.random_planes(w, h, 2))
    ok = c_format(ss.NV12)
    need = ctx.lib.ovhip_surface_bytes(w, h, None, C.byref(ok))
    assert need == w * h * 3 // 2
    d = _a5(ctx, 4 * need)
    held = ctx.scratch_bytes()
    P = pic.s

    def view(**kw):
        f = dict(y=P.y, cb=P.cb, cr=P.cr, w=P.w, h=P.h, stride_y=P.stride_y, stride_c=P.stride_c)
        f.update(kw)
        return engine.DevPic(ctx, capi.Pic(f["y"], f["cb"], f["cr"], f["w"], f["h"], f["stride_y"], f["stride_c"]), owns=False)

    rsv = c_format(ss.NV12)
    rsv.rsv[1] = 1
    F = c_format
    cases = [
        ("null destination", pic, ok, None, 0, need),
        ("too small", pic, ok, None, d.ptr.value, need - 1),
        ("too small", pic, F(ss.NV12, 0, w + 8), None, d.ptr.value, need),
        ("overlaps the picture", pic, ok, None, P.cb, 1 << 20),
        ("overlaps the picture", pic, ok, None, P.y - need + 1, 1 << 20),
        ("window leaves nothing", pic, ok, (18, 18, 0, 0), d.ptr.value, need),
        ("missing plane", view(cr=None), ok, None, d.ptr.value, need),
        ("stride below the width", view(stride_c=w // 2 - 2), ok, None, d.ptr.value, need),
        ("stride below the width", view(stride_y=w - 2), ok, None, d.ptr.value, need),
        ("sizes must be", view(w=w - 1), ok, None, d.ptr.value, need),
        ("sizes must be", view(h=h - 1), ok, None, d.ptr.value, need),
        ("sizes must be", view(w=16386), ok, None, d.ptr.value, 1 << 30),
        ("unknown format", pic, F(4), None, d.ptr.value, 4 * need),
        ("unknown rounding", pic, F(ss.I420, 2), None, d.ptr.value, 4 * need),
        ("rounding 0 only", pic, F(ss.P010, 1), None, d.ptr.value, 4 * need),
        ("rsv", pic, rsv, None, d.ptr.value, 4 * need),
        ("offset_c[1]", pic, F(ss.NV12, 0, 0, 0, (0, 2 * need)), None, d.ptr.value, 4 * need),
        ("pitch below", pic, F(ss.NV12, 0, w - 1), None, d.ptr.value, 4 * need),
        ("pitch below", pic, F(ss.I010, 0, 0, w - 2), None, d.ptr.value, 4 * need),
        ("multiple of the element", pic, F(ss.P010, 0, 2 * w + 1), None, d.ptr.value, 4 * need),
        ("multiple of the element", pic, F(ss.I010, 0, 0, 0, (2 * w * h + 1, 0)), None, d.ptr.value, 4 * need),
        ("not aligned", pic, F(ss.P010), None, d.ptr.value + 1, 4 * need - 1),
        ("planes overlap", pic, F(ss.NV12, 0, 0, 0, (w * h - 1, 0)), None, d.ptr.value, 4 * need),
        ("planes overlap", pic, F(ss.I420, 0, 0, 0, (w * h, w * h + 1)), None, d.ptr.value, 4 * need),
    ]
    for text, p, fmt, wd, ptr, nbytes in cases:
        assert p.surface_into(ptr, nbytes, fmt, wd or (0, 0, 0, 0), check=False) == capi.OVHIP_EINVAL, text
        assert text in ctx.lib.ovhip_last_error(ctx.h).decode(), (text, ctx.lib.ovhip_last_error(ctx.h))
    assert pic.surface_into(d.ptr.value, need - 1, ok, check=False) == capi.OVHIP_EINVAL
    msg = ctx.lib.ovhip_last_error(ctx.h).decode()
    assert "too small" in msg and str(need - 1) in msg and str(need) in msg, msg
    assert pic.surface_into(d.ptr.value, need, None, check=False) == capi.OVHIP_EINVAL
    # the convenience refuses the same way, into host memory that stays as it was
    host = np.full(need, ss.FILL, np.uint8)
    assert ctx.lib.ovhip_pic_output_surface(ctx.h, C.byref(P), None, C.byref(ok), host.ctypes.data, need - 1) == capi.OVHIP_EINVAL
    assert "too small" in ctx.lib.ovhip_last_error(ctx.h).decode()
    assert ctx.lib.ovhip_pic_output_surface(ctx.h, C.byref(P), C.byref(capi.Window(18, 18, 0, 0)), C.byref(ok), host.ctypes.data, need) == capi.OVHIP_EINVAL
    assert ctx.lib.ovhip_pic_output_surface(ctx.h, C.byref(P), None, C.byref(F(ss.P010, 1)), host.ctypes.data, 4 * need) == capi.OVHIP_EINVAL
    ctx.sync()
    assert (host == ss.FILL).all() and (d.download() == ss.FILL).all()
    assert ctx.scratch_bytes() == held
    d.free(); pic.free()


def test_python_layer_checks_the_tensor(built_lib):
    import torch
    nv12, p010 = c_format(ss.NV12), c_format(ss.P010)
    good = torch.zeros(96, dtype=torch.uint8, device="cuda:0")
    assert engine._surface_tensor(good, nv12, 96) == (good.data_ptr(), 96, 1)
    assert engine._surface_tensor(torch.zeros((2, 100), dtype=torch.uint8, device="cuda:0"), nv12, 96, slots=True)[1:] == (100, 2)
    wide = torch.zeros((3, 64), dtype=torch.int16, device="cuda:0")
    assert engine._surface_tensor(wide, p010, 128, slots=True)[1:] == (128, 3)
    for bad, fmt, need, slots in ((torch.zeros(95, dtype=torch.uint8, device="cuda:0"), nv12, 96, False),
                                  (torch.zeros(96, dtype=torch.uint8), nv12, 96, False),
                                  (torch.zeros(96, dtype=torch.int16, device="cuda:0"), nv12, 96, False),
                                  (torch.zeros(96, dtype=torch.float16, device="cuda:0"), p010, 96, False),
                                  (torch.zeros((2, 192), dtype=torch.uint8, device="cuda:0")[:, ::2], nv12, 96, True),
                                  (torch.zeros((2, 95), dtype=torch.uint8, device="cuda:0"), nv12, 96, True),
                                  (torch.zeros(192, dtype=torch.uint8, device="cuda:0"), nv12, 96, True),
                                  (np.zeros(96, np.uint8), nv12, 96, False)):
        with pytest.raises(engine.EngineError):
            engine._surface_tensor(bad, fmt, need, slots)


def _frame_fixture():
    w, h, wl, dec = _frame_case()
    dpb = engine.Dpb((0,))
    ctx = engine.Context(0)
    f = engine.Frame(dpb, 0, w, h)
    params = engine.Job.make_params(_Keep(), wl)

    def submit(key, out=None, check=True):
        f.begin(key)
        f.recorder().replay(wl.calllog)
        return f.submit(params, out=out, check=check)

    def published(key):
        return engine.DevPic(ctx, dpb.lookup(key)[1], owns=False).download()

    return w, h, wl, dec, dpb, ctx, f, params, submit, published


def test_frame_writes_the_picture_the_output_shows(built_lib):
    import torch
    w, h, wl, dec, dpb, ctx, f, params, submit, published = _frame_fixture()
    # no output description at all, a torch tensor as the destination
    fmt = engine.surface_format(capi.SURF_NV12)
    want, need = ss.surface(dec, ss.NV12)
    t = torch.full((need + GUARD,), 7, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    f.set_surface_output(t, fmt)
    assert submit(0x100) == 0
    got = t.cpu().numpy()
    assert got[:need].tobytes() == want.tobytes() and (got[need:] == 7).all()
    assert all(np.array_equal(a, b) for a, b in zip(published(0x100), dec))
    # per picture: a second submit without a new call writes nothing
    t.fill_(7)
    torch.cuda.synchronize()
    out = capi.FrameOutput()
    out.mode = capi.OUT_NONE
    assert submit(0x101, out) == 0
    assert (t.cpu().numpy() == 7).all()
    # a window, P010 with a pitch, a raw device address
    wd = (1, 0, 0, 1)
    lay = ss.loose_layout(ss.P010, w - 2, h - 2)
    fmt16 = engine.surface_format(capi.SURF_P010, **lay)
    want16, need16 = ss.surface(dec, ss.P010, 0, wd, total=None, **lay)
    body16, _ = ss.surface(dec, ss.P010, 0, wd, total=need16 + GUARD, **lay)
    d = _a5(ctx, need16 + GUARD)
    f.set_surface_output(d.ptr.value, fmt16, wd, nbytes=need16)
    assert submit(0x102, out) == 0
    assert d.download().tobytes() == body16.tobytes()
    # switched off again before the picture: the destination stays as it was
    d2 = _a5(ctx, need16)
    f.set_surface_output(d2.ptr.value, fmt16, wd, nbytes=need16)
    f.set_surface_output(None, None)
    assert submit(0x103) == 0
    assert (d2.download() == ss.FILL).all()
    # the format's refusals that need no picture come from the setter
    bad_rsv = engine.surface_format(capi.SURF_NV12)
    bad_rsv.rsv[0] = 1
    for bad in (engine.surface_format(4), engine.surface_format(capi.SURF_NV12, 2), engine.surface_format(capi.SURF_I010, 1), bad_rsv,
                engine.surface_format(capi.SURF_P010, 0, 0, 0, (0, 1 << 20)), engine.surface_format(capi.SURF_P010, 0, 2 * w + 1),
                engine.surface_format(capi.SURF_I010, 0, 0, 0, (2 * w * h + 1, 0))):
        assert f.set_surface_output(d2.ptr.value, bad, nbytes=1 << 20, check=False) == capi.OVHIP_EINVAL
    assert f.set_surface_output(0, fmt16, nbytes=1 << 20, check=False) == capi.OVHIP_EINVAL
    assert submit(0x104) == 0 and (d2.download() == ss.FILL).all(), "a refused setting is no setting"
    # a destination that is too small fails the call, not the publication
    f.set_surface_output(d2.ptr.value, fmt16, wd, nbytes=need16 - 1)
    assert submit(0x105, check=False) == capi.OVHIP_EINVAL
    assert b"too small" in built_lib.ovhip_frame_last_error(f.f)
    assert (d2.download() == ss.FILL).all()
    assert all(np.array_equal(a, b) for a, b in zip(published(0x105), dec))
    # the last band of a band-wise picture writes the surface
    d3 = _a5(ctx, need16)
    f.set_surface_output(d3.ptr.value, fmt16, wd, nbytes=need16)
    f.begin(0x106)
    f.recorder().replay(wl.calllog)
    assert built_lib.ovhip_frame_set_band_mode(f.f, 1) == 0
    assert built_lib.ovhip_frame_band(f.f, C.byref(params), h, 1, None) == 1, built_lib.ovhip_frame_last_error(f.f)
    assert d3.download().tobytes() == want16.tobytes()
    assert built_lib.ovhip_frame_set_band_mode(f.f, 0) == 0
    [b.free() for b in (d, d2, d3)]
    f.close(); ctx.close(); dpb.close()


def test_frame_composes_with_film_grain_and_with_the_output_scale(built_lib):
    w, h, wl, dec, dpb, ctx, f, params, submit, published = _frame_fixture()
    fmt = engine.surface_format(capi.SURF_NV12)
    plain, need = ss.surface(dec, ss.NV12)
    d = _a5(ctx, 128 * 96 * 3 // 2)
    # film grain: the surface is the grained picture's, the DPB holds the decoded one
    sei, poc = sf.make_sei(), 9
    f.set_film_grain(c_params(sei), poc)
    f.set_surface_output(d.ptr.value, fmt, nbytes=need)
    assert submit(0x100) == 0
    grained, _ = ss.surface(sf.apply(dec, sei, poc)[0], ss.NV12)
    got = d.download()[:need]
    assert got.tobytes() == grained.tobytes() != plain.tobytes()
    assert all(np.array_equal(a, b) for a, b in zip(published(0x100), dec))
    f.set_film_grain(None)
    # output scale to 128 x 96: the surface has the output's size
    f.set_output_scale(128, 96)
    want, need2 = ss.surface(spp.scale_picture(*dec, 128, 96, (0, 0, 0, 0), (0, 0)), ss.NV12, ss.DITHER)
    assert need2 == 128 * 96 * 3 // 2
    f.set_surface_output(d.ptr.value, engine.surface_format(capi.SURF_NV12, capi.SURF_DITHER), nbytes=need2)
    assert submit(0x200) == 0
    assert d.download().tobytes() == want.tobytes()
    _dev, held = dpb.lookup(0x200)
    assert (held.w, held.h) == (w, h)
    d.free()
    f.close(); ctx.close(); dpb.close()


def test_frame_writes_rgb_and_surface_of_one_submit(built_lib):
    w, h, wl, dec, dpb, ctx, f, params, submit, published = _frame_fixture()
    rgb_fmt = engine.rgb_format(1, 0, 0, capi.RGB_U8, capi.RGB_PLANAR)
    want_rgb = sr.convert(*dec, 1, 0, 0, sr.U8, sr.PLANAR)
    want_surf, need = ss.surface(dec, ss.I420, ss.DITHER)
    d_rgb, d_surf = _a5(ctx, want_rgb.nbytes + GUARD), _a5(ctx, need + GUARD)
    f.set_rgb_output(d_rgb.ptr.value, rgb_fmt, nbytes=want_rgb.nbytes)
    f.set_surface_output(d_surf.ptr.value, engine.surface_format(capi.SURF_I420, capi.SURF_DITHER), nbytes=need)
    assert submit(0x100) == 0
    raw_rgb, raw_surf = d_rgb.download(), d_surf.download()
    assert raw_rgb[:want_rgb.nbytes].tobytes() == want_rgb.tobytes() and (raw_rgb[want_rgb.nbytes:] == ss.FILL).all()
    assert raw_surf[:need].tobytes() == want_surf.tobytes() and (raw_surf[need:] == ss.FILL).all()
    assert all(np.array_equal(a, b) for a, b in zip(published(0x100), dec))
    d_rgb.free(); d_surf.free()
    f.close(); ctx.close(); dpb.close()


@pytest.mark.parametrize("via", ["submit", "band"])
@pytest.mark.parametrize("post", ["grain", "scale"])
def test_frame_outputs_of_one_picture_share_the_post_processed_picture(built_lib, post, via):
    """RGB, a surface and a PACKED delivery of ONE picture, behind film grain or an output scale: each equals, byte for byte, what the
    picture gives when that output is the only one set (the post-process step runs once, all three read its picture), and a picture
    with nothing set leaves all three destinations as they were"""
    w, h = 72, 40
    wl = synth.make_workload(w, h, 77, tools=synth.INTRA_TOOLS, intra_frac=1.0, calllog=True)
    lib = built_lib
    dpb = engine.Dpb((0,))
    ctx = engine.Context(0)
    f = engine.Frame(dpb, 0, w, h)
    params = engine.Job.make_params(_Keep(), wl)
    if post == "grain":
        f.set_film_grain(c_params(sf.make_sei()), 9)
        ow, oh = w, h
    else:
        ow, oh = 144, 80
        f.set_output_scale(ow, oh)
    rgb_fmt = engine.rgb_format(1, 0, 0, capi.RGB_U8, capi.RGB_PLANAR)
    surf_fmt = engine.surface_format(capi.SURF_NV12, pitch_y=ow + 24, pitch_c=ow + 8)      # (pitches above the row's bytes)
    win = capi.Window(0, 0, 0, 0)
    n_rgb, n_surf = 3 * ow * oh, lib.ovhip_surface_bytes(ow, oh, C.byref(win), C.byref(surf_fmt))
    n_packed = lib.ovhip_output_bytes(ow, oh, C.byref(win))
    assert n_surf == (ow + 24) * oh + (ow + 8) * (oh // 2 - 1) + ow and n_packed == ow * oh * 3

    def picture(key, rgb, surf, packed):
        """one picture with the outputs named; what the three destinations hold after it (sentinel bytes where nothing was written)"""
        d_rgb, d_surf = _a5(ctx, n_rgb + GUARD), _a5(ctx, n_surf + GUARD)
        host = np.full(n_packed + GUARD, ss.FILL, np.uint8)
        out = capi.FrameOutput()
        out.mode, out.window, out.packed = (capi.OUT_PACKED if packed else capi.OUT_NONE), win, host.ctypes.data
        if rgb:
            f.set_rgb_output(d_rgb.ptr.value, rgb_fmt, nbytes=n_rgb)
        if surf:
            f.set_surface_output(d_surf.ptr.value, surf_fmt, nbytes=n_surf)
        f.begin(key)
        f.recorder().replay(wl.calllog)
        if via == "submit":
            assert f.submit(params, out=out) == 0
        else:
            assert lib.ovhip_frame_set_band_mode(f.f, 1) == 0
            assert lib.ovhip_frame_band(f.f, C.byref(params), h, 1, C.byref(out)) == 1, lib.ovhip_frame_last_error(f.f)
            assert lib.ovhip_frame_set_band_mode(f.f, 0) == 0
        got = d_rgb.download().tobytes(), d_surf.download().tobytes(), host.tobytes()
        d_rgb.free(); d_surf.free()
        return got

    untouched = tuple(bytes([ss.FILL]) * (n + GUARD) for n in (n_rgb, n_surf, n_packed))
    all_three = picture(0x100, True, True, True)
    assert picture(0x101, False, False, False) == untouched, "the settings were the first picture's"
    alone = picture(0x102, True, False, False), picture(0x103, False, True, False), picture(0x104, False, False, True)
    for k, name in enumerate(("RGB", "surface", "PACKED")):
        assert all_three[k] != untouched[k] and all_three[k][-GUARD:] == untouched[k][-GUARD:], name
        assert all_three[k] == alone[k][k], name
        assert all(alone[k][j] == untouched[j] for j in range(3) if j != k), name
    f.close(); ctx.close(); dpb.close()


def test_stream_writes_every_picture_into_a_torch_tensor(built_lib):
    import torch
    w, h = 416, 240
    wls = _contents(w, h, (41, 42), 43)
    spics = _stream_pics(gop.build_stream(1, 4, 4, 1), 2)                               # I and one GOP of 4
    n = len(spics)
    ctx = engine.Context(0)
    dpb = engine.Dpb((0,))
    jobs = _jobs_for(ctx, wls, spics, w, h)
    st = engine.Stream(dpb, w, h, _make_contents(wls), jobs, threads_per_device=4)
    arr = st.pics_array(spics)
    fmt = engine.surface_format(capi.SURF_NV12)
    need = built_lib.ovhip_surface_bytes(w, h, None, C.byref(fmt))
    assert need == w * h * 3 // 2
    t = torch.zeros((n, need), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    st.set_surface_output(t, fmt)
    res, _ = st.run(arr, n, 0, n, flags=capi.STREAM_KEEP | capi.STREAM_HOLD_ALL)
    assert res.status == 0 and res.n_decoded == n
    got = t.cpu().numpy()
    want = [ss.surface(st.picture(i, ctx).download(), ss.NV12)[0] for i in range(n)]
    for i in range(n):
        assert got[i].tobytes() == want[i].tobytes(), i
    assert len({x.tobytes() for x in want}) == n - 1          # (pictures 0 and 1 are the stream's one recorded I picture twice)
    # n_slots = 2: picture idx lands in slot idx % 2.  One run per pair of pictures, so that no two pictures in flight share a slot
    t2 = torch.zeros((2, need + 64), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    st.set_surface_output(t2, fmt)
    for first, cnt in ((0, 2), (2, 2), (4, 1)):
        res, _ = st.run(arr, n, first, cnt, flags=capi.STREAM_KEEP)
        assert res.status == 0 and res.n_decoded == cnt
        got = t2.cpu().numpy()
        last = first + cnt - 1
        for slot in range(2):
            idx = last if last % 2 == slot else last - 1
            assert got[slot, :need].tobytes() == want[idx].tobytes() and not got[slot, need:].any(), (first, slot)
    # a bytes_per_picture that is too small, a bad slot count, a null base, a format the setter refuses, a tensor that is too small
    assert st.set_surface_output(t2.data_ptr(), fmt, bytes_per_picture=need - 1, n_slots=2, check=False) == capi.OVHIP_EINVAL
    assert st.set_surface_output(t2.data_ptr(), fmt, bytes_per_picture=need, n_slots=0, check=False) == capi.OVHIP_EINVAL
    assert st.set_surface_output(0, fmt, bytes_per_picture=need, n_slots=2, check=False) == capi.OVHIP_EINVAL
    assert st.set_surface_output(t2.data_ptr(), engine.surface_format(capi.SURF_P010, 1), bytes_per_picture=4 * need, n_slots=2, check=False) == capi.OVHIP_EINVAL
    assert st.set_surface_output(t2.data_ptr(), engine.surface_format(capi.SURF_NV12, 0, w - 1), bytes_per_picture=4 * need, n_slots=2, check=False) == capi.OVHIP_EINVAL
    assert st.set_surface_output(t2.data_ptr(), fmt, (1, 0, 0, 1), bytes_per_picture=need - 1, n_slots=2, check=False) == 0       # (the window needs less)
    with pytest.raises(engine.EngineError):
        st.set_surface_output(t2[:, :need - 1].contiguous(), fmt)
    with pytest.raises(engine.EngineError):
        st.set_surface_output(t2[:, ::2], fmt)
    # off again: the tensor stays as it is
    st.set_surface_output(None, None)
    t2.zero_()
    torch.cuda.synchronize()
    res, _ = st.run(arr, n, 0, n)
    assert res.status == 0 and not t2.any().item()
    assert dpb.stats().n_live == 0
    st.close(); [j.close() for j in jobs]; dpb.close(); ctx.close()
