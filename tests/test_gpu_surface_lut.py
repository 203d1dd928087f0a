"""GPU: surface output through a colour table on the device (openvvc_amd/csrc/kernels_surface_lut.hip): ovhip_surface_lut_launch and
ovhip_pic_output_surface_lut against the host twin and the numpy restatement tests/spec_surface_lut.py; destinations that are only
element-aligned, with a pitch with gaps, over a sentinel; a strided view as the source; the refusals; one table under two contexts; the
frame thread (sticky, cleared, with film grain, with an output scale, with the reduced size, beside the RGB table); the stream driver
into a torch tensor.  The definition is integer only: every comparison is of bytes."""
import ctypes as C
import itertools

import numpy as np
import pytest

import spec_film_grain as sf
import spec_pp_scale as spp
import spec_reduce as sd
import spec_rgb as sr
import spec_rgb_lut as sl
import spec_surface as ss
import spec_surface_lut as sx
import surface_lut_cases as cs
from openvvc_amd import capi, engine, gop, lut3d
from test_film_grain_cpu import c_params
from test_gpu_stream import _contents, _jobs_for, _make_contents, _stream_pics
from test_gpu_surface import _frame_fixture

pytestmark = pytest.mark.gpu

GUARD = 96


@pytest.fixture(scope="module")
def ctx(built_lib):
    c = engine.Context(0)
    yield c
    c.close()


def _a5(ctx, nbytes):
    return ctx.upload(np.full(nbytes, ss.FILL, np.uint8))


def _check(ctx, w, h, conv, size, peak, windows, modes=ss.MODES, gaps=(False, True), leads=(0,)):
    """launch (into a sentinel-filled buffer, `lead` elements behind its start), convenience and host twin against the restatement"""
    planes = cs.census_planes(w, h)
    table = cs.census_table(size, peak)
    pic = ctx.upload_pic(*planes)
    cc = cs.c_conv(conv)
    with engine.RgbLut(ctx, table, peak) as lut:
        for wd, (fmt, rounding), loose, lead in itertools.product(windows, modes, gaps, leads):
            W, H = cs.window_size(w, h, wd)
            lay = cs.loose(fmt, W, H) if loose else {}
            cf = engine.surface_format(fmt, rounding, **lay)
            what = (w, h, conv, size, peak, wd, fmt, rounding, loose, lead)
            need = ctx.lib.ovhip_surface_bytes(w, h, C.byref(capi.Window(*wd)), C.byref(cf))
            off = lead * ss.ELEM[fmt]
            want, size_want = cs.reference(w, h, conv, size, peak, wd, fmt, rounding, total=need + GUARD, **lay)
            assert need == size_want, what
            twin, _ = cs.host_twin(ctx.lib, planes, conv, fmt, rounding, table, peak, wd, **lay)
            assert twin[:need].tobytes() == want[:need].tobytes(), what
            d = _a5(ctx, off + need + GUARD)
            pic.surface_into(d.ptr.value + off, need, cf, wd, lut=lut, conv=cc)
            ctx.sync()
            raw = d.download()
            assert (raw[:off] == ss.FILL).all() and raw[off:].tobytes() == want.tobytes(), what       # (gaps and tail: the sentinel)
            d.free()
            if lead == 0:
                got = pic.surface(cf, wd, lut=lut, conv=cc)
                zero_gaps, _ = cs.reference(w, h, conv, size, peak, wd, fmt, rounding, fill=0, **lay)
                assert got.tobytes() == zero_gaps.tobytes(), what
    assert all(np.array_equal(a, b) for a, b in zip(pic.download(), planes)), "the picture is only read"
    pic.free()


@pytest.mark.parametrize("dloc", sx.DST_LOCS)
def test_every_format_and_rounding_at_72x40(ctx, dloc):
    _check(ctx, 72, 40, cs.conv_of(dloc % 3, (0, 1, 2, 1)[dloc], dloc), cs.TABLE_SIZES[dloc % 3], cs.PEAKS[dloc], cs.WINDOWS)


@pytest.mark.parametrize("w,h", [(20, 12), (16, 8), (136, 24), (2052, 8)])
@pytest.mark.parametrize("dloc", sx.DST_LOCS)
def test_launch_and_convenience_equal_host_and_restatement(ctx, w, h, dloc):
    """20 x 12: a run tail of 4; 16 x 8 under (1, 1, 1, 1): 12 x 4, two row pairs, both halo directions at every edge; 136 x 24: 17
    runs per row, a row ends inside a workgroup's items; 2052 x 8: more items than one workgroup, and a tail of 4"""
    n = (w // 4 + dloc) % 3
    modes = [(ss.NV12, ss.DITHER), (ss.I010, ss.ROUND)] if dloc & 1 else [(ss.P010, ss.ROUND), (ss.I420, ss.DITHER)]
    _check(ctx, w, h, cs.conv_of(n, (dloc + w // 4) % 3, dloc), cs.TABLE_SIZES[(n + 1) % 3], cs.PEAKS[(dloc + w // 8) % 4], cs.WINDOWS, modes, gaps=(bool(dloc & 2),))


@pytest.mark.parametrize("w,h", cs.PICTURES)
@pytest.mark.parametrize("sloc", range(6))
def test_every_instantiation_and_vertical_case(ctx, w, h, sloc):
    """every k_surface_lut<format, a, hc> under every row selection of the source (a = sloc & 1 with b = 1, 1, 0, 0, 2, 2) and both
    vertical cases of the destination (hc = 1 at dloc 0 and 2, the halo row at dloc 2 and 3), the full window, tight rows; the 8-bit formats
    round and dither in turn, the 16-bit ones take rounding only.  72 x 40: nine full runs per row, twenty row pairs; 20 x 12: a run
    tail of 4.  A case's converted picture is restated once and stored in the four formats"""
    for dloc in sx.DST_LOCS:
        r8 = (ss.ROUND, ss.DITHER)[(sloc + dloc) & 1]
        modes = [(ss.NV12, r8), (ss.I420, ss.ROUND + ss.DITHER - r8), (ss.P010, ss.ROUND), (ss.I010, ss.ROUND)]
        _check(ctx, w, h, cs.conv_of((sloc + dloc) % 3, sloc, dloc), cs.TABLE_SIZES[(sloc + dloc) % 3], cs.PEAKS[dloc], [(0, 0, 0, 0)], modes, gaps=(False,))


def test_a_destination_offset_by_one_element(ctx):
    """aligned to its element and to nothing more, with a pitch with gaps, over a sentinel: no byte outside the rows' own bytes is written"""
    _check(ctx, 72, 40, cs.conv_of(1, 2, 2), 17, 1023, [(0, 0, 0, 0), (1, 0, 0, 1)], gaps=(True,), leads=(1, 3))
    _check(ctx, 20, 12, cs.conv_of(0, 0, 0), 33, 255, [(1, 1, 1, 1)], gaps=(False, True), leads=(1,))


def test_a_view_with_a_stride_above_its_width(ctx):
    """the left 72 columns of a 136 x 24 picture as a picture of its own (chroma rows of stride 68: not 8-byte aligned), and the same
    view moved 4 columns to the right (luma rows not 16-byte aligned): the source's chroma taps clamp at the VIEW's edge"""
    planes = cs.census_planes(136, 24)
    pic = ctx.upload_pic(*planes)
    table = cs.census_table(33, 4000)
    with engine.RgbLut(ctx, table, 4000) as lut:
        for x in (0, 4):
            s = capi.Pic(pic.s.y + 2 * x, pic.s.cb + x, pic.s.cr + x, 72, 24, pic.s.stride_y, pic.s.stride_c)
            view = engine.DevPic(ctx, s, owns=False)
            part = (planes[0][:, x:x + 72], planes[1][:, x // 2:x // 2 + 36], planes[2][:, x // 2:x // 2 + 36])
            for (fmt, rounding), dloc, wd in itertools.product([(ss.NV12, 0), (ss.I010, 0)], (0, 3), ((0, 0, 0, 0), (1, 0, 0, 1))):
                conv = cs.conv_of(0, 1, dloc)
                want, _ = sx.surface(part, conv, table, 4000, fmt, rounding, wd)
                got = view.surface(engine.surface_format(fmt, rounding), wd, lut=lut, conv=cs.c_conv(conv))
                assert got.tobytes() == want.tobytes(), (x, fmt, dloc, wd)
    assert all(np.array_equal(a, b) for a, b in zip(pic.download(), planes))
    pic.free()


def test_refusals_come_back_before_anything_is_launched(ctx):
    """return values and the error text only: nothing is provoked on the device, and the destination stays as it was"""
    w, h = 72, 40
    lib = ctx.lib
    pic = ctx.upload_pic(*sr.random_planes(w, h, 2))
    ok = engine.surface_format(capi.SURF_P010)
    okc = engine.surface_conv()
    need = lib.ovhip_surface_bytes(w, h, None, C.byref(ok))
    d = _a5(ctx, need)
    P = pic.s
    lut = engine.RgbLut(ctx, sl.random_table(17, 1023, 4), 1023)
    pic.surface(ok, lut=lut, conv=okc)                                             # (the convenience's scratch has this size from here on)
    held = ctx.scratch_bytes()

    def view(**kw):
        f = dict(y=P.y, cb=P.cb, cr=P.cr, w=P.w, h=P.h, stride_y=P.stride_y, stride_c=P.stride_c)
        f.update(kw)
        return engine.DevPic(ctx, capi.Pic(f["y"], f["cb"], f["cr"], f["w"], f["h"], f["stride_y"], f["stride_c"]), owns=False)

    def conv(**kw):
        c = engine.surface_conv()
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    rsv = engine.surface_conv()
    rsv.rsv[0] = 1
    EIN, EUN = capi.OVHIP_EINVAL, capi.OVHIP_EUNSUP
    cases = [
        # the conversion's
        ("null conversion", pic, None, ok, None, d.ptr.value, need, lut, EIN),
        ("conv rsv", pic, rsv, ok, None, d.ptr.value, need, lut, EIN),
        ("matrix coefficients unspecified", pic, conv(src_matrix=2), ok, None, d.ptr.value, need, lut, EIN),
        ("matrix coefficients not built", pic, conv(src_matrix=14), ok, None, d.ptr.value, need, lut, EUN),
        ("destination matrix coefficients unspecified", pic, conv(dst_matrix=2), ok, None, d.ptr.value, need, lut, EIN),
        ("destination matrix coefficients not built", pic, conv(dst_matrix=0), ok, None, d.ptr.value, need, lut, EUN),
        ("bad range", pic, conv(dst_full_range=2), ok, None, d.ptr.value, need, lut, EIN),
        ("bad chroma location", pic, conv(src_chroma_loc=6), ok, None, d.ptr.value, need, lut, EIN),
        ("destination chroma locations 4 and 5 not built", pic, conv(dst_chroma_loc=4), ok, None, d.ptr.value, need, lut, EUN),
        ("destination chroma locations 4 and 5 not built", pic, conv(dst_chroma_loc=5), ok, None, d.ptr.value, need, lut, EUN),
        # the table's and the RGB side's
        ("null table", pic, okc, ok, None, d.ptr.value, need, None, EIN),
        ("multiples of 4", view(w=w - 2), okc, ok, None, d.ptr.value, need, lut, EIN),
        ("multiples of 4", view(h=h - 2), okc, ok, None, d.ptr.value, need, lut, EIN),
        # the surface output's
        ("null format", pic, okc, None, None, d.ptr.value, need, lut, EIN),
        ("unknown format", pic, okc, engine.surface_format(4), None, d.ptr.value, need, lut, EIN),
        ("a 16-bit format takes rounding 0 only", pic, okc, engine.surface_format(capi.SURF_P010, 1), None, d.ptr.value, need, lut, EIN),
        ("pitch below the row's bytes", pic, okc, engine.surface_format(capi.SURF_P010, 0, 2 * w - 2), None, d.ptr.value, need, lut, EIN),
        ("planes overlap one another", pic, okc, engine.surface_format(capi.SURF_P010, 0, 0, 0, (2 * w, 0)), None, d.ptr.value, need, lut, EIN),
        ("null destination", pic, okc, ok, None, 0, need, lut, EIN),
        ("too small", pic, okc, ok, None, d.ptr.value, need - 1, lut, EIN),
        (f"{need - 1} bytes given, the surface needs {need}", pic, okc, ok, None, d.ptr.value, need - 1, lut, EIN),
        ("overlaps", pic, okc, ok, None, P.cb, 1 << 20, lut, EIN),
        ("window leaves nothing", pic, okc, ok, (18, 18, 0, 0), d.ptr.value, need, lut, EIN),
        ("missing plane", view(cr=None), okc, ok, None, d.ptr.value, need, lut, EIN),
        ("stride below the width", view(stride_c=w // 2 - 2), okc, ok, None, d.ptr.value, need, lut, EIN),
        ("not aligned", pic, okc, ok, None, d.ptr.value + 1, need - 1, lut, EIN),
    ]
    for text, p, cv, fmt, wd, ptr, nbytes, table, code in cases:
        assert p.surface_into(ptr, nbytes, fmt, wd or (0, 0, 0, 0), check=False, lut=table, conv=cv) == code, text
        err = lib.ovhip_last_error(ctx.h).decode()
        assert err.startswith("ovhip_surface_lut_launch: ") and text in err, (text, err)
    # the convenience refuses the same way, into host memory that stays as it was
    host = np.full(need, ss.FILL, np.uint8)
    assert lib.ovhip_pic_output_surface_lut(ctx.h, C.byref(P), None, C.byref(okc), C.byref(ok), lut.h, host.ctypes.data, need - 1) == EIN
    assert lib.ovhip_pic_output_surface_lut(ctx.h, C.byref(P), None, C.byref(okc), C.byref(ok), None, host.ctypes.data, need) == EIN
    assert "ovhip_surface_lut_launch: null table" in lib.ovhip_last_error(ctx.h).decode()
    assert lib.ovhip_pic_output_surface_lut(ctx.h, C.byref(P), None, C.byref(conv(dst_chroma_loc=4)), C.byref(ok), lut.h, host.ctypes.data, need) == EUN
    with pytest.raises(engine.EngineError):
        pic.surface(ok, lut=lut)                                                   # (a table without a conversion)
    ctx.sync()
    assert (host == ss.FILL).all() and (d.download() == ss.FILL).all()
    # a table created on another context of the same device is accepted; no restriction on the peak for an 8-bit surface
    other = engine.Context(0)
    with engine.RgbLut(other, sl.random_table(17, 65535, 6), 65535) as foreign:
        nv12 = engine.surface_format(capi.SURF_NV12)
        assert pic.surface_into(d.ptr.value, need, nv12, lut=foreign, conv=okc) == 0
        ctx.sync()
    other.close()
    assert (d.download() != ss.FILL).any()
    assert ctx.scratch_bytes() == held
    lut.close(); d.free(); pic.free()


def test_scratch_stays_flat_over_repeated_launches(built_lib):
    ctx = engine.Context(0)
    w, h = 136, 24
    pic = ctx.upload_pic(*cs.census_planes(w, h))
    d = ctx.alloc(w * h * 3)
    with engine.RgbLut(ctx, cs.census_table(33, 255), 255) as lut:
        before = ctx.scratch_bytes()
        for rep in range(3):
            for (fmt, rounding), dloc in itertools.product(ss.MODES, sx.DST_LOCS):
                pic.surface_into(d.ptr.value, d.nbytes, engine.surface_format(fmt, rounding), lut=lut, conv=cs.c_conv(cs.conv_of(0, 0, dloc)))
        ctx.sync()
        assert ctx.scratch_bytes() == before, "the launch allocates nothing"
        first = pic.surface(engine.surface_format(capi.SURF_P010), lut=lut, conv=engine.surface_conv())       # the convenience: its scratch at the largest size first
        held = ctx.scratch_bytes()
        assert held - before >= first.nbytes
        for fmt, rounding in ss.MODES:
            pic.surface(engine.surface_format(fmt, rounding), (1, 0, 0, 1), lut=lut, conv=engine.surface_conv())
            assert ctx.scratch_bytes() == held
    d.free(); pic.free(); ctx.close()


def test_one_table_under_two_contexts_on_different_streams(built_lib):
    a, b = engine.Context(0), engine.Context(0)
    assert a.stream != b.stream
    w, h, size, peak = 136, 24, 65, 65535
    conv = cs.conv_of(1, 2, 0)
    fmt = engine.surface_format(capi.SURF_NV12, capi.SURF_DITHER)
    want, need = cs.reference(w, h, conv, size, peak, (0, 0, 0, 0), ss.NV12, ss.DITHER)
    planes = cs.census_planes(w, h)
    pa, pb = a.upload_pic(*planes), b.upload_pic(*planes)
    da, db = a.alloc(need), b.alloc(need)
    with engine.RgbLut(a, cs.census_table(size, peak), peak) as lut:
        for rep in range(4):                                                    # both streams busy with the same table at once
            pa.surface_into(da.ptr.value, need, fmt, lut=lut, conv=cs.c_conv(conv))
            pb.surface_into(db.ptr.value, need, fmt, lut=lut, conv=cs.c_conv(conv))
        a.sync(); b.sync()
        ga, gb = da.download(), db.download()
    assert ga.tobytes() == gb.tobytes() == want.tobytes()
    [x.free() for x in (da, db, pa, pb)]
    a.close(); b.close()


def test_frame_goes_through_the_table_until_it_is_cleared(built_lib):
    import torch
    w, h, wl, dec, dpb, ctx, f, params, submit, published = _frame_fixture()
    table = lut3d.pq_bt2020_to_bt709(33, 1023)
    lut = engine.RgbLut(ctx, table, 1023)                                         # (another context of the frame's device)
    wd = (1, 0, 0, 1)
    conv = (9, 0, 2, 1, 0, 0)
    fmt = engine.surface_format(capi.SURF_NV12)
    want, need = sx.surface(dec, conv, table, 1023, ss.NV12, window=wd)
    plain, _ = ss.surface(dec, ss.NV12, 0, wd)
    assert len(want) == len(plain) and want.tobytes() != plain.tobytes()
    f.set_surface_lut(lut, cs.c_conv(conv))
    # sticky: two pictures, each with its own destination, one setting of the table
    for key in (0x100, 0x101):
        t = torch.full((need + GUARD,), 7, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        f.set_surface_output(t, fmt, wd)
        assert submit(key) == 0
        got = t.cpu().numpy()
        assert got[:need].tobytes() == want.tobytes() and (got[need:] == 7).all(), key
        assert all(np.array_equal(a, b) for a, b in zip(published(key), dec))
    # the setter's refusals leave the setting as it was
    assert f.set_surface_lut(lut, None, check=False) == capi.OVHIP_EINVAL
    assert f.set_surface_lut(lut, engine.surface_conv(dst_chroma_loc=4), check=False) == capi.OVHIP_EUNSUP
    assert f.set_surface_lut(lut, engine.surface_conv(dst_matrix=2), check=False) == capi.OVHIP_EINVAL
    assert built_lib.ovhip_frame_set_surface_lut(None, lut.h, C.byref(cs.c_conv(conv))) == capi.OVHIP_EINVAL
    d = _a5(ctx, need + GUARD)
    f.set_surface_output(d.ptr.value, fmt, wd, nbytes=need)
    assert submit(0x102) == 0
    assert d.download()[:need].tobytes() == want.tobytes()
    # cleared: today's bytes
    f.set_surface_lut(None)
    f.set_surface_output(d.ptr.value, fmt, wd, nbytes=need)
    assert submit(0x103) == 0
    raw = d.download()
    assert raw[:need].tobytes() == plain.tobytes() and (raw[need:] == ss.FILL).all()
    d.free(); lut.close()
    f.close(); ctx.close(); dpb.close()


def test_frame_composes_with_film_grain_output_scale_and_reduce(built_lib):
    w, h, wl, dec, dpb, ctx, f, params, submit, published = _frame_fixture()
    assert (w, h) == (64, 48)
    table, peak = sl.random_table(17, 65535, 12), 65535
    lut = engine.RgbLut(ctx, table, peak)
    conv = (9, 0, 0, 1, 1, 2)
    f.set_surface_lut(lut, cs.c_conv(conv))
    fmt = engine.surface_format(capi.SURF_P010)
    d = _a5(ctx, 128 * 96 * 3)

    def through(planes):
        return sx.surface(planes, conv, table, peak, ss.P010)[0]

    def picture(key, want):
        f.set_surface_output(d.ptr.value, fmt, nbytes=len(want))
        assert submit(key) == 0
        return d.download()[:len(want)]

    plain = through(dec)
    # film grain: the table's picture is the grained one, the DPB holds the decoded one
    sei, poc = sf.make_sei(), 9
    f.set_film_grain(c_params(sei), poc)
    grained = through(sf.apply(dec, sei, poc)[0])
    got = picture(0x100, grained)
    assert got.tobytes() == grained.tobytes() != plain.tobytes()
    assert all(np.array_equal(a, b) for a, b in zip(published(0x100), dec))
    f.set_film_grain(None)
    # output scale to 128 x 96
    f.set_output_scale(128, 96)
    want = through(spp.scale_picture(*dec, 128, 96, (0, 0, 0, 0), (0, 0)))
    assert len(want) == 128 * 96 * 3
    assert picture(0x200, want).tobytes() == want.tobytes()
    f.set_output_scale(0, 0)
    # reduced 2:1 to 32 x 24: the restatement applied to the reduced picture
    f.set_output_reduce(32, 24, (0, 0, 0, 0), 2)
    want = through(sd.reduce_picture(*dec, 32, 24, (0, 0, 0, 0), 2))
    assert len(want) == 32 * 24 * 3
    assert picture(0x300, want).tobytes() == want.tobytes()
    f.set_output_reduce(0, 0)
    # nothing but the table
    assert picture(0x400, plain).tobytes() == plain.tobytes()
    d.free(); lut.close()
    f.close(); ctx.close(); dpb.close()


def test_frame_rgb_table_and_surface_table_are_independent(built_lib):
    w, h, wl, dec, dpb, ctx, f, params, submit, published = _frame_fixture()
    t_rgb, t_surf = sl.random_table(17, 255, 1), sl.random_table(33, 4000, 2)
    lut_rgb, lut_surf = engine.RgbLut(ctx, t_rgb, 255), engine.RgbLut(ctx, t_surf, 4000)
    conv = (9, 0, 2, 1, 0, 1)
    rgb_fmt = engine.rgb_format(9, 0, 0, capi.RGB_U8, capi.RGB_PLANAR)
    surf_fmt = engine.surface_format(capi.SURF_I420, capi.SURF_DITHER)
    rgb_plain, rgb_lut = sr.convert(*dec, 9, 0, 0, sr.U8, sr.PLANAR), sl.convert(*dec, 9, 0, 0, sr.U8, sr.PLANAR, t_rgb, 255)
    surf_plain, need = ss.surface(dec, ss.I420, ss.DITHER)
    surf_lut, _ = sx.surface(dec, conv, t_surf, 4000, ss.I420, ss.DITHER)
    surf_one, _ = sx.surface(dec, conv, t_rgb, 255, ss.I420, ss.DITHER)
    d_rgb, d_surf = _a5(ctx, rgb_plain.nbytes), _a5(ctx, need)
    key = 0x100
    # (RGB table, surface table) -> what the two destinations hold; the last row: ONE table serving both outputs
    for a, b, want_rgb, want_surf in ((lut_rgb, lut_surf, rgb_lut, surf_lut), (None, lut_surf, rgb_plain, surf_lut), (lut_rgb, None, rgb_lut, surf_plain),
                                      (None, None, rgb_plain, surf_plain), (lut_rgb, lut_rgb, rgb_lut, surf_one)):
        f.set_rgb_lut(a)
        f.set_surface_lut(b, cs.c_conv(conv) if b is not None else None)
        f.set_rgb_output(d_rgb.ptr.value, rgb_fmt, nbytes=rgb_plain.nbytes)
        f.set_surface_output(d_surf.ptr.value, surf_fmt, nbytes=need)
        assert submit(key) == 0
        key += 1
        assert d_rgb.download().tobytes() == want_rgb.tobytes(), (a is not None, b is not None)
        assert d_surf.download().tobytes() == want_surf.tobytes(), (a is not None, b is not None)
    d_rgb.free(); d_surf.free(); lut_rgb.close(); lut_surf.close()
    f.close(); ctx.close(); dpb.close()


def test_stream_writes_every_picture_through_the_table_into_a_torch_tensor(built_lib):
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
    table = lut3d.pq_bt2020_to_bt709(17, 1023)
    conv = (9, 0, 2, 1, 0, 0)
    t = torch.zeros((n, need), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    st.set_surface_output(t, fmt)
    st.set_surface_lut(table, 1023, cs.c_conv(conv))
    res, _ = st.run(arr, n, 0, n, flags=capi.STREAM_KEEP | capi.STREAM_HOLD_ALL)
    assert res.status == 0 and res.n_decoded == n
    got = t.cpu().numpy()
    decoded = [st.picture(i, ctx).download() for i in range(n)]
    want = [sx.surface(decoded[i], conv, table, 1023, ss.NV12)[0] for i in range(n)]
    for i in range(n):
        assert got[i].tobytes() == want[i].tobytes(), i
    # a table or a conversion the library refuses leaves the setting as it was; then cleared: the surface output as before
    bad = table.copy()
    bad[0, 0, 0, 0] = 1024
    assert st.set_surface_lut(bad, 1023, cs.c_conv(conv), check=False) == capi.OVHIP_EINVAL
    assert st.set_surface_lut(table, 1023, engine.surface_conv(dst_chroma_loc=5), check=False) == capi.OVHIP_EUNSUP
    assert st.set_surface_lut(table, 1023, None, check=False) == capi.OVHIP_EINVAL
    t.zero_()
    torch.cuda.synchronize()
    res, _ = st.run(arr, n, 0, n, flags=capi.STREAM_KEEP)
    assert res.status == 0
    assert t.cpu().numpy()[n - 1].tobytes() == want[n - 1].tobytes()
    st.set_surface_lut(None)
    res, _ = st.run(arr, n, 0, n)
    assert res.status == 0
    got = t.cpu().numpy()
    for i in range(n):
        assert got[i].tobytes() == ss.surface(decoded[i], ss.NV12)[0].tobytes(), i
    st.close(); [j.close() for j in jobs]; dpb.close(); ctx.close()
