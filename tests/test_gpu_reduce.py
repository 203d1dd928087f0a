"""GPU: reduced-size output on the device (k_output_reduce, openvvc_amd/csrc/kernels_reduce.hip) and the layers above it:
ovhip_output_reduce_launch against the numpy restatement tests/spec_reduce.py on the whole census -- every chroma location where the
census says so, strided pictures, a window whose rows are 4- and 2-byte aligned, sentinels around the destination --, the synchronous
conveniences, the frame thread (whole and band-wise, with RGB, a surface and a PACKED delivery of one picture), the stream driver, and
the refusals.  The definition is integer only: every comparison is of bytes."""
import ctypes as C

import numpy as np
import pytest

import spec_film_grain as sf
import spec_reduce as sd
import spec_rgb as sr
import spec_surface as ss
from openvvc_amd import capi, engine, gop, synth
from test_film_grain_cpu import c_params
from test_gpu_stream import _Keep, _contents, _jobs_for, _make_contents, _stream_pics
from test_reduce_cpu import SENT, info_of, strided

pytestmark = pytest.mark.gpu
GUARD_ROWS = 3                                                # sentinel rows above and below every destination plane
GUARD = 16                                                    # bytes behind a destination that must stay as they were


@pytest.fixture(scope="module")
def ctx(built_lib):
    c = engine.Context(0)
    yield c
    c.close()


def device_reduce(ctx, planes, Wd, Hd, window=(0, 0, 0, 0), loc=0, spad=0, dpad=0):
    """ovhip_output_reduce_launch of the planes (rows of w + spad samples) into planes of rows Wd + dpad inside buffers that held the
    sentinel, GUARD_ROWS rows above and below -> the three whole buffers as arrays"""
    h, w = planes[0].shape
    sb = [ctx.upload(a) for a in strided(planes, w + spad, w // 2 + spad)]
    shapes = [(Hd + 2 * GUARD_ROWS, Wd + dpad), (Hd // 2 + 2 * GUARD_ROWS, Wd // 2 + dpad), (Hd // 2 + 2 * GUARD_ROWS, Wd // 2 + dpad)]
    db = [ctx.upload(np.full(s, SENT, np.uint16)) for s in shapes]
    sp = capi.Pic(sb[0].ptr.value, sb[1].ptr.value, sb[2].ptr.value, w, h, w + spad, w // 2 + spad)
    dp = capi.Pic(*[b.ptr.value + GUARD_ROWS * s[1] * 2 for b, s in zip(db, shapes)], Wd, Hd, Wd + dpad, Wd // 2 + dpad)
    src = engine.DevPic(ctx, sp, owns=False)
    src.reduce_into(engine.DevPic(ctx, dp, owns=False), window, loc)
    ctx.sync()
    got = [b.download(np.uint16).reshape(s) for b, s in zip(db, shapes)]
    back = [b.download(np.uint16) for b in sb]
    assert all(np.array_equal(a.ravel(), b) for a, b in zip(strided(planes, w + spad, w // 2 + spad), back)), "the source is only read"
    [b.free() for b in sb + db]
    return got


def assert_device_equals(got, want, what):
    for g, x in zip(got, want):
        body = g[GUARD_ROWS:-GUARD_ROWS]
        bad = int((body[:, :x.shape[1]] != x).sum())
        assert bad == 0, f"{what}: {bad} samples differ from the restatement"
        assert (g[:GUARD_ROWS] == SENT).all() and (g[-GUARD_ROWS:] == SENT).all(), f"{what}: rows around the destination"
        assert (body[:, x.shape[1]:] == SENT).all(), f"{what}: the stride gap"


@pytest.mark.parametrize("case", range(len(sd.CENSUS)))
def test_launch_equals_the_restatement_on_the_census(ctx, case):
    (w, h), (Wd, Hd), locs = sd.CENSUS[case]
    planes = sd.random_planes(w, h, 200 + case)
    for loc in locs:
        assert_device_equals(device_reduce(ctx, planes, Wd, Hd, loc=loc), sd.reduce_picture(*planes, Wd, Hd, loc=loc), (w, h, Wd, Hd, loc))
    if (w, h, Wd, Hd) == (72, 40, 72, 40):
        assert_device_equals(device_reduce(ctx, planes, Wd, Hd), planes, "the identity")
    if (w, h, Wd, Hd) == (72, 40, 48, 24):
        assert_device_equals(device_reduce(ctx, planes, Wd, Hd, spad=6, dpad=2), sd.reduce_picture(*planes, Wd, Hd), "source stride w + 6, destination stride Wd + 2")
    if w == 1024:
        full = [np.full_like(p, 1023) for p in planes]
        assert_device_equals(device_reduce(ctx, full, Wd, Hd), [np.full((Hd, Wd), 1023, np.uint16)] + [np.full((Hd // 2, Wd // 2), 1023, np.uint16)] * 2, "the int32 ceiling")


def test_a_window_whose_rows_are_only_4_and_2_byte_aligned(ctx):
    """everything outside the window holds 1023 over content of at most 511 inside: the result is the reduction of the cropped picture"""
    (w, h), wd, (Wd, Hd) = sd.WINDOW_CASE
    l, r, a, b = wd
    inner = sd.random_planes(w - 2 * (l + r), h - 2 * (a + b), 3, top=512)
    planes = [np.full((h, w), 1023, np.uint16), np.full((h // 2, w // 2), 1023, np.uint16), np.full((h // 2, w // 2), 1023, np.uint16)]
    planes[0][2 * a:h - 2 * b, 2 * l:w - 2 * r] = inner[0]
    planes[1][a:h // 2 - b, l:w // 2 - r] = inner[1]
    planes[2][a:h // 2 - b, l:w // 2 - r] = inner[2]
    for loc in (0, 5):
        assert_device_equals(device_reduce(ctx, planes, Wd, Hd, wd, loc), sd.reduce_picture(*inner, Wd, Hd, loc=loc), ("window", loc))
        assert_device_equals(device_reduce(ctx, planes, Wd, Hd, wd, loc, spad=6, dpad=2), sd.reduce_picture(*inner, Wd, Hd, loc=loc), ("window, strides", loc))


def test_conveniences_equal_output_and_digest_of_the_restated_picture(built_lib):
    ctx = engine.Context(0)
    (w, h), wd, (Wd, Hd) = sd.WINDOW_CASE
    planes = sd.random_planes(w, h, 17)
    pic = ctx.upload_pic(*planes)
    held0 = ctx.scratch_bytes()
    # a refused request allocates nothing
    with pytest.raises(engine.EngineError):
        pic.output_reduced(8, 24)
    assert "ratio" in ctx.lib.ovhip_last_error(ctx.h).decode()
    with pytest.raises(engine.EngineError):
        pic.output_reduced(160, 96)
    msg = ctx.lib.ovhip_last_error(ctx.h).decode()
    assert "up-sampling" in msg and "ovhip_output_scale" in msg
    big = ctx.new_pic(1028, 64)
    with pytest.raises(engine.EngineError):
        big.digest_reduced(132, 64)
    msg = ctx.lib.ovhip_last_error(ctx.h).decode()
    assert "257/33" in msg and "common divisor" in msg
    big.free()
    assert ctx.scratch_bytes() == held0
    held = None
    for src_win, loc, ow, oh in (((0, 0, 0, 0), 0, 64, 32), (wd, 3, Wd, Hd)):      # 80x48 -> 64x32 (5/4; 3/2), then the window's 72x40 -> 48x24
        want = sd.reduce_picture(*planes, ow, oh, src_win, loc)
        ref = ctx.upload_pic(*want)
        for win in ((0, 0, 0, 0), (1, 2, 0, 1)):
            assert pic.output_reduced(ow, oh, src_win, loc, win).tobytes() == ref.output(win).tobytes() == sd.packed(want, win).tobytes(), (src_win, win)
            assert pic.digest_reduced(ow, oh, src_win, loc, win) == ref.digest(win), (src_win, win)
        ref.free()
        held = held or ctx.scratch_bytes()                   # (the larger size came first: grow-only, constant from here on)
        assert ctx.scratch_bytes() == held
    assert all(np.array_equal(a, b) for a, b in zip(pic.download(), planes)), "the picture is only read"
    pic.free(); ctx.close()


def test_launch_refusals_come_back_before_anything_is_launched(ctx):
    """return values and the error text only: nothing is provoked on the device"""
    big, small = ctx.new_pic(128, 96), ctx.new_pic(64, 48)
    err = lambda: ctx.lib.ovhip_last_error(ctx.h).decode()
    assert small.reduce_into(big, check=False) == capi.OVHIP_EUNSUP and "up-sampling" in err()
    tiny = ctx.new_pic(8, 48)
    assert big.reduce_into(tiny, check=False) == capi.OVHIP_EUNSUP and "ratio" in err()
    assert big.reduce_into(big, check=False) == capi.OVHIP_EINVAL and "aliases" in err()
    assert big.reduce_into(big.band(0, 48), check=False) == capi.OVHIP_EINVAL
    s = capi.Pic(small.s.y, small.s.cb, None, small.s.w, small.s.h, small.s.stride_y, small.s.stride_c)
    assert big.reduce_into(engine.DevPic(ctx, s, owns=False), check=False) == capi.OVHIP_EINVAL and "missing plane" in err()
    s = capi.Pic(small.s.y, small.s.cb, small.s.cr, small.s.w, small.s.h, 60, small.s.stride_c)
    assert big.reduce_into(engine.DevPic(ctx, s, owns=False), check=False) == capi.OVHIP_EINVAL and "stride" in err()
    assert big.reduce_into(small, (32, 32, 0, 0), check=False) == capi.OVHIP_EINVAL and "leaves nothing" in err()
    assert big.reduce_into(small, (1, 0, 0, 0), check=False) == capi.OVHIP_EINVAL
    assert big.reduce_into(small, chroma_loc=6, check=False) == capi.OVHIP_EINVAL
    rsv = info_of()
    rsv.rsv[0] = 1
    assert ctx.lib.ovhip_output_reduce_launch(ctx.h, C.byref(big.s), C.byref(rsv), C.byref(small.s)) == capi.OVHIP_EINVAL
    assert ctx.lib.ovhip_output_reduce_launch(ctx.h, C.byref(big.s), None, C.byref(small.s)) == capi.OVHIP_EINVAL
    odd = ctx.new_pic(66, 50)
    assert big.reduce_into(odd, check=False) == capi.OVHIP_EINVAL
    # the resampler keeps refusing down-sampling, with its own text
    assert big.scale_into(small, check=False) == capi.OVHIP_EUNSUP and "down-sampling" in err()
    for p in (big, small, tiny, odd):
        p.free()


def _frame(w=72, h=40, seed=77):
    wl = synth.make_workload(w, h, seed, tools=synth.INTRA_TOOLS, intra_frac=1.0, calllog=True)
    dpb = engine.Dpb((0,))
    ctx = engine.Context(0)
    f = engine.Frame(dpb, 0, w, h)
    return wl, dpb, ctx, f, engine.Job.make_params(_Keep(), wl)


@pytest.mark.parametrize("via", ["submit", "band"])
def test_frame_outputs_of_one_picture_read_the_one_reduced_picture(built_lib, via):
    """RGB, a surface and a PACKED delivery of ONE picture with reduce set: each equals that output of the restated reduced picture;
    the DPB holds the decoded picture; a following picture with nothing set leaves all three destinations as they were; the scratch
    is constant from the second picture on"""
    w, h, ow, oh = 72, 40, 48, 24
    lib = built_lib
    wl, dpb, ctx, f, params = _frame(w, h)
    src_win, loc = (0, 0, 0, 0), 2
    f.set_output_reduce(ow, oh, src_win, loc)
    rgb_fmt = engine.rgb_format(1, 0, 0, capi.RGB_U8, capi.RGB_PLANAR)
    surf_fmt = engine.surface_format(capi.SURF_NV12, pitch_y=ow + 24, pitch_c=ow + 8)
    win = (1, 0, 0, 1)
    cwin = capi.Window(*win)
    n_rgb, n_surf = 3 * (ow - 2) * (oh - 2), lib.ovhip_surface_bytes(ow, oh, C.byref(cwin), C.byref(surf_fmt))
    n_packed = lib.ovhip_output_bytes(ow, oh, C.byref(cwin))
    assert n_surf and n_packed == (ow - 2) * (oh - 2) * 3
    fctx = lib.ovhip_frame_ctx(f.f)

    def picture(key, outputs):
        d_rgb, d_surf = ctx.upload(np.full(n_rgb + GUARD, ss.FILL, np.uint8)), ctx.upload(np.full(n_surf + GUARD, ss.FILL, np.uint8))
        host = np.full(n_packed + GUARD, ss.FILL, np.uint8)
        out = capi.FrameOutput()
        out.mode, out.window, out.packed = (capi.OUT_PACKED if outputs else capi.OUT_NONE), cwin, host.ctypes.data
        if outputs:
            f.set_rgb_output(d_rgb.ptr.value, rgb_fmt, win, nbytes=n_rgb)
            f.set_surface_output(d_surf.ptr.value, surf_fmt, win, nbytes=n_surf)
        f.begin(key)
        f.recorder().replay(wl.calllog)
        if via == "submit":
            assert f.submit(params, out=out) == 0
        else:
            assert lib.ovhip_frame_set_band_mode(f.f, 1) == 0
            assert lib.ovhip_frame_band(f.f, C.byref(params), h, 1, C.byref(out)) == 1, lib.ovhip_frame_last_error(f.f)
            assert lib.ovhip_frame_set_band_mode(f.f, 0) == 0
        got = d_rgb.download(), d_surf.download(), host
        d_rgb.free(); d_surf.free()
        return got

    got = picture(0x100, True)
    held = lib.ovhip_ctx_scratch_bytes(fctx)
    _dev, held_pic = dpb.lookup(0x100)
    assert (held_pic.w, held_pic.h) == (w, h)
    dec = engine.DevPic(ctx, held_pic, owns=False).download()
    red = sd.reduce_picture(*dec, ow, oh, src_win, loc)
    want_rgb = sr.convert(*red, 1, 0, 0, sr.U8, sr.PLANAR, win)
    want_surf, size = ss.surface(red, ss.NV12, ss.ROUND, win, total=n_surf + GUARD, pitch_y=ow + 24, pitch_c=ow + 8)
    assert size == n_surf
    assert got[1].tobytes() == want_surf.tobytes(), "surface"
    assert got[2][:n_packed].tobytes() == sd.packed(red, win).tobytes() and (got[2][n_packed:] == ss.FILL).all(), "PACKED"
    # RGB: against the launch on the restated reduced picture alone
    ref = ctx.upload_pic(*red)
    d = ctx.upload(np.full(n_rgb + GUARD, ss.FILL, np.uint8))
    assert lib.ovhip_rgb_launch(ctx.h, C.byref(ref.s), C.byref(cwin), C.byref(rgb_fmt), d.ptr, n_rgb) == 0
    ctx.sync()
    assert got[0].tobytes() == d.download().tobytes() and got[0][:n_rgb].any(), "RGB"
    assert got[0][:n_rgb].tobytes() == np.ascontiguousarray(want_rgb).tobytes(), "RGB against its restatement"
    d.free(); ref.free()
    # nothing set: the destinations stay, the scratch stays
    idle = picture(0x101, False)
    assert all((x == ss.FILL).all() for x in idle)
    again = picture(0x102, True)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again))
    assert lib.ovhip_ctx_scratch_bytes(fctx) == held, "constant from the second picture on"
    # switched off: the packed frame is the decoded picture's again
    f.set_output_reduce(0, 0)
    host = np.zeros(lib.ovhip_output_bytes(w, h, None) // 2, np.uint16)
    out = capi.FrameOutput()
    out.mode, out.packed = capi.OUT_PACKED, host.ctypes.data
    f.begin(0x103)
    f.recorder().replay(wl.calllog)
    assert f.submit(params, out=out) == 0
    assert host.tobytes() == sd.packed(dec).tobytes()
    f.close(); ctx.close(); dpb.close()


def test_setters_hold_one_post_setting_and_refuse_before_they_allocate(built_lib):
    lib = built_lib
    w, h = 72, 40
    wl, dpb, ctx, f, params = _frame(w, h)
    fctx = lib.ovhip_frame_ctx(f.f)
    held = lib.ovhip_ctx_scratch_bytes(fctx)
    fg = c_params(sf.make_sei())
    UNSUP, INVAL = capi.OVHIP_EUNSUP, capi.OVHIP_EINVAL
    # reduce first: grain and scale are refused, switching either off is not
    assert f.set_output_reduce(48, 24) == 0
    assert f.set_film_grain(fg, 5, check=False) == UNSUP and f.set_output_scale(144, 80, check=False) == UNSUP
    assert f.set_film_grain(None) == 0 and f.set_output_scale(0, 0) == 0
    assert f.set_output_reduce(0, 0) == 0
    # grain first, then scale first
    assert f.set_film_grain(fg, 5) == 0
    assert f.set_output_reduce(48, 24, check=False) == UNSUP and f.set_output_reduce(0, 0) == 0
    assert f.set_film_grain(None) == 0
    assert f.set_output_scale(144, 80) == 0
    assert f.set_output_reduce(48, 24, check=False) == UNSUP and f.set_output_reduce(0, 0) == 0
    assert f.set_output_scale(0, 0) == 0
    # the definition's refusals come from the setter
    assert f.set_output_reduce(144, 80, check=False) == UNSUP and f.set_output_reduce(8, 40, check=False) == UNSUP
    assert f.set_output_reduce(46, 24, check=False) == INVAL and f.set_output_reduce(48, 24, (18, 18, 0, 0), check=False) == INVAL
    assert f.set_output_reduce(48, 24, chroma_loc=6, check=False) == INVAL
    assert lib.ovhip_frame_set_output_reduce(None, 48, 24, None) == INVAL and lib.ovhip_stream_set_output_reduce(None, 48, 24, None) == INVAL
    assert lib.ovhip_frame_set_output_reduce(f.f, 48, 24, None) == 0 and f.set_output_reduce(0, 0) == 0
    # the resampler still refuses to halve
    assert f.set_output_scale(w // 2, h // 2, check=False) == UNSUP
    assert lib.ovhip_ctx_scratch_bytes(fctx) == held, "a refused request allocates nothing"
    # a refused setting is no setting: the picture leaves at its coded size
    host = np.zeros(lib.ovhip_output_bytes(w, h, None) // 2, np.uint16)
    out = capi.FrameOutput()
    out.mode, out.packed = capi.OUT_PACKED, host.ctypes.data
    f.begin(0x100)
    f.recorder().replay(wl.calllog)
    assert f.submit(params, out=out) == 0
    dec = engine.DevPic(ctx, dpb.lookup(0x100)[1], owns=False).download()
    assert host.tobytes() == sd.packed(dec).tobytes()
    f.close(); ctx.close(); dpb.close()


def test_stream_with_slots_sized_for_the_reduced_size(built_lib):
    import torch
    w, h, ow, oh = 416, 240, 208, 120
    wls = _contents(w, h, (41, 42), 43)
    spics = _stream_pics(gop.build_stream(1, 4, 4, 1), 2)                               # I and one GOP of 4
    n = len(spics)
    ctx = engine.Context(0)
    dpb = engine.Dpb((0,))
    jobs = _jobs_for(ctx, wls, spics, w, h)
    st = engine.Stream(dpb, w, h, _make_contents(wls), jobs, threads_per_device=4)
    arr = st.pics_array(spics)
    fmt = engine.surface_format(capi.SURF_NV12)
    fg = c_params(sf.make_sei())
    # one post setting, in both orders
    assert st.set_output_reduce(ow, oh, chroma_loc=1) == 0
    assert st.set_film_grain(fg, check=False) == capi.OVHIP_EUNSUP and st.set_output_scale(832, 480, check=False) == capi.OVHIP_EUNSUP
    assert st.set_output_reduce(0, 0) == 0 and st.set_film_grain(fg) == 0
    assert st.set_output_reduce(ow, oh, check=False) == capi.OVHIP_EUNSUP
    assert st.set_film_grain(None) == 0 and st.set_output_scale(832, 480) == 0
    assert st.set_output_reduce(ow, oh, check=False) == capi.OVHIP_EUNSUP
    assert st.set_output_scale(0, 0) == 0
    assert st.set_output_reduce(48, 240, check=False) == capi.OVHIP_EUNSUP              # 26/3 on x: the ratio
    assert st.set_output_scale(w // 2, h // 2, check=False) == capi.OVHIP_EUNSUP
    assert st.set_output_reduce(ow, oh, chroma_loc=1) == 0
    need = built_lib.ovhip_surface_bytes(ow, oh, None, C.byref(fmt))
    assert need == ow * oh * 3 // 2
    t = torch.zeros((n, need), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    st.set_surface_output(t, fmt)                                                       # (checked against the reduced size)
    with pytest.raises(engine.EngineError):
        st.set_surface_output(torch.zeros((n, need - 1), dtype=torch.uint8, device="cuda:0"), fmt)
    st.set_surface_output(t, fmt)
    res, dg = st.run(arr, n, 0, n, flags=capi.STREAM_KEEP | capi.STREAM_HOLD_ALL, digests=True)
    assert res.status == 0 and res.n_decoded == n
    got = t.cpu().numpy()
    for i in range(n):
        red = sd.reduce_picture(*st.picture(i, ctx).download(), ow, oh, loc=1)
        assert got[i].tobytes() == ss.surface(red, ss.NV12)[0].tobytes(), i
        ref = ctx.upload_pic(*red)
        assert bytes(dg[i]) == ref.digest(), i
        ref.free()
    st.close(); [j.close() for j in jobs]; dpb.close(); ctx.close()
