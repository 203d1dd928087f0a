"""GPU: RGB output through a colour table on the device (openvvc_amd/csrc/kernels_rgb_lut.hip): ovhip_rgb_lut_launch and
ovhip_pic_output_rgb_lut against the host twin and the numpy restatement tests/spec_rgb_lut.py, destinations that are only
element-aligned, the refusals, one table under two contexts, the frame thread (alone, with film grain, with an output scale, with the
reduced size; sticky; cleared), the stream driver into a torch tensor.  The definition is integer only: every comparison is of bytes."""
import ctypes as C
import itertools

import numpy as np
import pytest

import spec_film_grain as sf
import spec_pp_scale as spp
import spec_reduce as sd
import spec_rgb as sr
import spec_rgb_lut as sl
from openvvc_amd import capi, engine, gop, lut3d
from test_film_grain_cpu import c_params
from test_gpu_pic_hash import _frame_case
from test_gpu_stream import _Keep, _contents, _jobs_for, _make_contents, _stream_pics
from test_rgb_cpu import same_bits
from test_rgb_lut_cpu import CASES, DTYPES, LAYOUTS, census_planes, host_lut

pytestmark = pytest.mark.gpu

ES = {sr.U8: 1, sr.U16: 2, sr.F16: 2, sr.F32: 4}


@pytest.fixture(scope="module")
def ctx(built_lib):
    c = engine.Context(0)
    yield c
    c.close()


def _a5(ctx, nbytes):
    return ctx.upload(np.full(nbytes, 0xA5, np.uint8))


def _as_picture(raw: np.ndarray, fmt, w, h, window) -> np.ndarray:
    shape = engine.rgb_shape(fmt, w, h, window)
    n = shape[0] * shape[1] * shape[2] * ES[fmt.dtype]
    return raw[:n].view(sr.NP_DTYPE[fmt.dtype]).reshape(shape)


def _check(ctx, planes, table, peak, combos, windows, matrix=9, full=0, loc=0):
    """launch, convenience and host twin against the restatement for every (dtype, layout) of `combos` x window"""
    h, w = planes[0].shape
    pic = ctx.upload_pic(*planes)
    d = ctx.alloc(3 * w * h * 4)
    with engine.RgbLut(ctx, table, peak) as lut:
        for wd in windows:
            o = sl.interpolate(sl.rgb10(*planes, matrix, full, loc, wd), table)            # the reference, once per window
            for dtype, layout in combos:
                fmt = capi.RgbFormat(matrix, full, loc, dtype, layout)
                want = sl.store(o, peak, dtype, layout)
                what = (w, h, table.shape[0], peak, dtype, layout, wd)
                assert same_bits(host_lut(ctx.lib, planes, fmt, table, peak, wd), want), what
                pic.rgb_into(d.ptr.value, want.nbytes, fmt, wd, lut=lut)
                ctx.sync()
                assert same_bits(_as_picture(d.download(), fmt, w, h, wd), want), what
                assert same_bits(pic.rgb(fmt, wd, lut=lut), want), what
    assert all(np.array_equal(a, b) for a, b in zip(pic.download(), planes)), "the picture is only read"
    d.free(); pic.free()


@pytest.mark.parametrize("size", sl.SIZES)
@pytest.mark.parametrize("w,h,wd", CASES)
def test_launch_and_convenience_equal_host_and_restatement(ctx, size, w, h, wd):
    planes = census_planes(w, h, 7 * w + size)
    _check(ctx, planes, sl.random_table(size, 65535, size + w), 65535, [(sr.U16, sr.PLANAR), (sr.F16, sr.PACKED), (sr.F32, sr.PLANAR)], [wd])
    _check(ctx, planes, sl.random_table(size, 255, size + w + 1), 255, [(sr.U8, sr.PACKED)], [wd], matrix=1, full=1, loc=3)


@pytest.mark.parametrize("peak", (255, 65535))
def test_every_dtype_and_layout_at_72x40(ctx, peak):
    combos = [(dt, lay) for dt, lay in itertools.product(DTYPES, LAYOUTS) if dt != sr.U8 or peak <= 255]
    _check(ctx, census_planes(72, 40, 500 + peak % 7), sl.random_table(33, peak, peak), peak, combos, [(0, 0, 0, 0), (1, 0, 0, 1), (0, 3, 2, 0)], loc=2)


@pytest.mark.parametrize("w,h", [(72, 40), (20, 12)])
@pytest.mark.parametrize("loc", range(6))
def test_every_instantiation_and_vertical_case(ctx, w, h, loc):
    """every k_rgb_lut<dtype, layout, a> under every row selection b: the six chroma locations are a = loc & 1 with b = 1, 1, 0, 0, 2, 2.
    72 x 40: nine full runs per row, twenty row pairs; 20 x 12: a run tail of 4.  The table's output is restated once per location and
    peak and stored in every dtype and layout"""
    planes = census_planes(w, h, 40 + loc)
    _check(ctx, planes, sl.random_table(17, 255, loc), 255, [(sr.U8, lay) for lay in LAYOUTS], [(0, 0, 0, 0)], loc=loc)
    _check(ctx, planes, sl.random_table(17, 65535, 6 + loc), 65535, [(dt, lay) for dt in DTYPES if dt != sr.U8 for lay in LAYOUTS], [(0, 0, 0, 0)], loc=loc)


def test_the_lattice_table_gives_exactly_n_times_the_rgb_output(ctx):
    planes = census_planes(136, 72, 6)
    pic = ctx.upload_pic(*planes)
    fmt = capi.RgbFormat(1, 0, 0, sr.U16, sr.PLANAR)
    plain = pic.rgb(fmt)
    for size in sl.SIZES:
        with engine.RgbLut(ctx, lut3d.lattice(size), 65535) as lut:
            assert np.array_equal(pic.rgb(fmt, lut=lut), (size - 1) * plain), size
    pic.free()


@pytest.mark.parametrize("w,h,wd", CASES)
def test_a_destination_offset_by_one_element(ctx, w, h, wd):
    """a slice of a batch tensor at odd sizes is aligned to its element and to nothing more: the bytes around it stay as they were"""
    planes = census_planes(w, h, 9)
    pic = ctx.upload_pic(*planes)
    table = sl.random_table(17, 255, 9)
    o = sl.interpolate(sl.rgb10(*planes, 5, 0, 1, wd), table)
    with engine.RgbLut(ctx, table, 255) as lut:
        for dtype, layout in itertools.product(DTYPES, LAYOUTS):
            fmt = capi.RgbFormat(5, 0, 1, dtype, layout)
            want = sl.store(o, 255, dtype, layout)
            es = ES[dtype]
            for lead in (es, 3 * es, 16 + es):
                d = _a5(ctx, lead + want.nbytes + 37)
                pic.rgb_into(d.ptr.value + lead, want.nbytes, fmt, wd, lut=lut)
                ctx.sync()
                raw = d.download()
                assert (raw[:lead] == 0xA5).all() and (raw[lead + want.nbytes:] == 0xA5).all(), (dtype, layout, lead)
                assert raw[lead:lead + want.nbytes].tobytes() == want.tobytes(), (dtype, layout, lead)
                d.free()
    pic.free()


def test_a_view_with_a_stride_above_its_width(ctx):
    """the left 72 columns of a 136x72 picture as a picture of its own (chroma rows of stride 68: not 8-byte aligned), and the same
    view moved 4 columns to the right (luma rows not 16-byte aligned): the chroma taps clamp at the VIEW's edge"""
    planes = census_planes(136, 72, 3)
    pic = ctx.upload_pic(*planes)
    table = sl.random_table(33, 1023, 3)
    with engine.RgbLut(ctx, table, 1023) as lut:
        for x in (0, 4):
            s = capi.Pic(pic.s.y + 2 * x, pic.s.cb + x, pic.s.cr + x, 72, 72, pic.s.stride_y, pic.s.stride_c)
            view = engine.DevPic(ctx, s, owns=False)
            part = (planes[0][:, x:x + 72], planes[1][:, x // 2:x // 2 + 36], planes[2][:, x // 2:x // 2 + 36])
            for dtype, layout, loc in itertools.product((sr.U16, sr.F16), LAYOUTS, (1, 4)):
                fmt = capi.RgbFormat(1, 0, loc, dtype, layout)
                for wd in ((0, 0, 0, 0), (1, 0, 0, 1)):
                    assert same_bits(view.rgb(fmt, wd, lut=lut), sl.convert(*part, 1, 0, loc, dtype, layout, table, 1023, wd)), (x, dtype, layout, loc, wd)
    pic.free()


def test_refusals_come_back_before_anything_is_launched(ctx):
    """return values and the error text only: nothing is provoked on the device, and the destination stays as it was"""
    w, h = 72, 40
    lib = ctx.lib
    pic = ctx.upload_pic(*sr.random_planes(w, h, 2))
    ok = capi.RgbFormat(1, 0, 0, sr.U16, sr.PLANAR)
    u8 = capi.RgbFormat(1, 0, 0, sr.U8, sr.PLANAR)
    need = lib.ovhip_rgb_bytes(w, h, None, C.byref(ok))
    d = _a5(ctx, need)
    held = ctx.scratch_bytes()
    P = pic.s
    lut = engine.RgbLut(ctx, sl.random_table(17, 1023, 4), 1023)
    closed = engine.RgbLut(ctx, sl.random_table(17, 255, 4), 255)
    closed.close()

    def view(**kw):
        f = dict(y=P.y, cb=P.cb, cr=P.cr, w=P.w, h=P.h, stride_y=P.stride_y, stride_c=P.stride_c)
        f.update(kw)
        return engine.DevPic(ctx, capi.Pic(f["y"], f["cb"], f["cr"], f["w"], f["h"], f["stride_y"], f["stride_c"]), owns=False)

    cases = [
        ("null table", pic, ok, None, d.ptr.value, need, closed, capi.OVHIP_EINVAL),
        ("peak <= 255", pic, u8, None, d.ptr.value, need, lut, capi.OVHIP_EINVAL),
        ("null destination", pic, ok, None, 0, need, lut, capi.OVHIP_EINVAL),
        ("too small", pic, ok, None, d.ptr.value, need - 1, lut, capi.OVHIP_EINVAL),
        ("overlaps", pic, ok, None, P.cb, 1 << 20, lut, capi.OVHIP_EINVAL),
        ("window leaves nothing", pic, ok, (18, 18, 0, 0), d.ptr.value, need, lut, capi.OVHIP_EINVAL),
        ("missing plane", view(cr=None), ok, None, d.ptr.value, need, lut, capi.OVHIP_EINVAL),
        ("stride below the width", view(stride_c=w // 2 - 2), ok, None, d.ptr.value, need, lut, capi.OVHIP_EINVAL),
        ("multiples of 4", view(w=w - 2), ok, None, d.ptr.value, need, lut, capi.OVHIP_EINVAL),
        ("bad dtype", pic, capi.RgbFormat(1, 0, 0, 4, 0), None, d.ptr.value, 1 << 20, lut, capi.OVHIP_EINVAL),
        ("unspecified", pic, capi.RgbFormat(2, 0, 0, 1, 0), None, d.ptr.value, need, lut, capi.OVHIP_EINVAL),
        ("not built", pic, capi.RgbFormat(14, 0, 0, 1, 0), None, d.ptr.value, need, lut, capi.OVHIP_EUNSUP),
        ("not aligned", pic, ok, (1, 0, 0, 0), d.ptr.value + 1, need - 1, lut, capi.OVHIP_EINVAL),
    ]
    for text, p, fmt, wd, ptr, nbytes, table, code in cases:
        assert p.rgb_into(ptr, nbytes, fmt, wd or (0, 0, 0, 0), check=False, lut=table) == code, text
        assert text in lib.ovhip_last_error(ctx.h).decode(), (text, lib.ovhip_last_error(ctx.h))
    # the convenience refuses the same way, into host memory that stays as it was
    host = np.full(need, 0xA5, np.uint8)
    assert lib.ovhip_pic_output_rgb_lut(ctx.h, C.byref(P), None, C.byref(ok), lut.h, host.ctypes.data, need - 1) == capi.OVHIP_EINVAL
    assert lib.ovhip_pic_output_rgb_lut(ctx.h, C.byref(P), None, C.byref(ok), None, host.ctypes.data, need) == capi.OVHIP_EINVAL
    assert lib.ovhip_pic_output_rgb_lut(ctx.h, C.byref(P), None, C.byref(u8), lut.h, host.ctypes.data, need) == capi.OVHIP_EINVAL
    ctx.sync()
    assert (host == 0xA5).all() and (d.download() == 0xA5).all()
    # the table's creation: sizes, peaks, a null table, an entry above the peak with its index in the error text
    h_ = C.c_void_p()
    t17 = sl.random_table(17, 1023, 5)
    for size, peak in ((16, 1023), (34, 1023), (17, 0), (17, 65536)):
        assert lib.ovhip_rgb_lut_create(ctx.h, size, peak, t17.ctypes.data, C.byref(h_)) == capi.OVHIP_EINVAL and not h_.value
    assert lib.ovhip_rgb_lut_create(ctx.h, 17, 1023, None, C.byref(h_)) == capi.OVHIP_EINVAL and not h_.value
    t17[16, 3, 5, 1] = 1024
    assert lib.ovhip_rgb_lut_create(ctx.h, 17, 1023, t17.ctypes.data, C.byref(h_)) == capi.OVHIP_EINVAL and not h_.value
    err = lib.ovhip_last_error(ctx.h).decode()
    assert "[16][3][5][1]" in err and f"index {3 * ((16 * 17 + 3) * 17 + 5) + 1}" in err and "1024" in err, err
    with pytest.raises(engine.EngineError):
        engine.RgbLut(ctx, t17, 1023)
    with pytest.raises(engine.EngineError):
        engine.RgbLut(ctx, t17.astype(np.int32), 1023)
    with pytest.raises(engine.EngineError):
        engine.RgbLut(ctx, t17[:, :, :16], 1023)
    # a table created on another context of the same device is accepted
    other = engine.Context(0)
    with engine.RgbLut(other, sl.random_table(17, 1023, 6), 1023) as foreign:
        assert pic.rgb_into(d.ptr.value, need, ok, lut=foreign) == 0
        ctx.sync()
    other.close()
    assert (d.download() != 0xA5).any()
    assert ctx.scratch_bytes() == held
    lut.close(); d.free(); pic.free()


def test_scratch_stays_flat_over_repeated_launches(built_lib):
    ctx = engine.Context(0)
    pic = ctx.upload_pic(*sr.random_planes(264, 136, 1))
    d = ctx.alloc(3 * 264 * 136 * 4)
    with engine.RgbLut(ctx, sl.random_table(33, 255, 1), 255) as lut:
        before = ctx.scratch_bytes()
        for rep in range(3):
            for dtype, layout in itertools.product(DTYPES, LAYOUTS):
                pic.rgb_into(d.ptr.value, d.nbytes, capi.RgbFormat(1, 0, 0, dtype, layout), lut=lut)
        ctx.sync()
        assert ctx.scratch_bytes() == before, "the launch allocates nothing"
        first = pic.rgb(capi.RgbFormat(1, 0, 0, sr.F32, sr.PLANAR), lut=lut)               # the convenience: its scratch at the largest size first
        held = ctx.scratch_bytes()
        assert held - before >= first.nbytes
        for dtype, layout in itertools.product(DTYPES, LAYOUTS):
            pic.rgb(capi.RgbFormat(1, 0, 0, dtype, layout), (1, 0, 0, 1), lut=lut)
            assert ctx.scratch_bytes() == held
    d.free(); pic.free(); ctx.close()


def test_one_table_under_two_contexts_on_different_streams(built_lib):
    a, b = engine.Context(0), engine.Context(0)
    assert a.stream != b.stream
    planes = census_planes(264, 136, 8)
    table = sl.random_table(65, 65535, 8)
    fmt = capi.RgbFormat(9, 0, 0, sr.F16, sr.PACKED)
    want = sl.convert(*planes, 9, 0, 0, sr.F16, sr.PACKED, table, 65535)
    pa, pb = a.upload_pic(*planes), b.upload_pic(*planes)
    da, db = a.alloc(want.nbytes), b.alloc(want.nbytes)
    with engine.RgbLut(a, table, 65535) as lut:
        for rep in range(4):                                                    # both streams busy with the same table at once
            pa.rgb_into(da.ptr.value, want.nbytes, fmt, lut=lut)
            pb.rgb_into(db.ptr.value, want.nbytes, fmt, lut=lut)
        a.sync(); b.sync()
        ga, gb = da.download(), db.download()
    assert ga.tobytes() == gb.tobytes() == want.tobytes()
    [x.free() for x in (da, db, pa, pb)]
    a.close(); b.close()


def test_frame_goes_through_the_table_until_it_is_cleared(built_lib):
    import torch
    w, h, wl, dec = _frame_case()
    dpb = engine.Dpb((0,))
    ctx = engine.Context(0)
    f = engine.Frame(dpb, 0, w, h)
    params = engine.Job.make_params(_Keep(), wl)

    def submit(key, check=True):
        f.begin(key)
        f.recorder().replay(wl.calllog)
        return f.submit(params, check=check)

    table = lut3d.pq_bt2020_to_bt709(33, 255)
    lut = engine.RgbLut(ctx, table, 255)                                          # (another context of the frame's device)
    wd = (1, 0, 0, 1)
    fmt = engine.rgb_format(9, 0, 0, capi.RGB_U8, capi.RGB_PACKED)
    want = sl.convert(*dec, 9, 0, 0, sr.U8, sr.PACKED, table, 255, wd)
    plain = sr.convert(*dec, 9, 0, 0, sr.U8, sr.PACKED, wd)
    assert want.shape == plain.shape and not np.array_equal(want, plain)
    f.set_rgb_lut(lut)
    # sticky: two pictures, each with its own destination, one setting of the table
    for key in (0x100, 0x101):
        t = torch.full(want.shape, 7, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        f.set_rgb_output(t, fmt, wd)
        assert submit(key) == 0
        assert same_bits(t.cpu().numpy(), want), key
        assert all(np.array_equal(a, b) for a, b in zip(engine.DevPic(ctx, dpb.lookup(key)[1], owns=False).download(), dec))
    # the launch's refusals fail the call, not the publication: U16 is fine with this table, a U8 table of peak 1023 is not
    big = engine.RgbLut(ctx, sl.random_table(17, 1023, 1), 1023)
    f.set_rgb_lut(big)
    d = _a5(ctx, want.nbytes)
    f.set_rgb_output(d.ptr.value, fmt, wd, nbytes=want.nbytes)
    assert submit(0x102, check=False) == capi.OVHIP_EINVAL
    assert b"peak <= 255" in built_lib.ovhip_frame_last_error(f.f)
    assert (d.download() == 0xA5).all()
    # cleared: today's bytes
    f.set_rgb_lut(None)
    f.set_rgb_output(d.ptr.value, fmt, wd, nbytes=want.nbytes)
    assert submit(0x103) == 0
    assert d.download().tobytes() == plain.tobytes()
    assert built_lib.ovhip_frame_set_rgb_lut(None, lut.h) == capi.OVHIP_EINVAL
    d.free(); big.close(); lut.close()
    f.close(); ctx.close(); dpb.close()


def test_frame_composes_with_film_grain_output_scale_and_reduce(built_lib):
    w, h, wl, dec = _frame_case()
    dpb = engine.Dpb((0,))
    ctx = engine.Context(0)
    f = engine.Frame(dpb, 0, w, h)
    params = engine.Job.make_params(_Keep(), wl)

    def submit(key):
        f.begin(key)
        f.recorder().replay(wl.calllog)
        assert f.submit(params) == 0

    table = sl.random_table(17, 65535, 12)
    lut = engine.RgbLut(ctx, table, 65535)
    f.set_rgb_lut(lut)
    fmt = engine.rgb_format(1, 0, 0, capi.RGB_U16, capi.RGB_PLANAR)

    def through(planes):
        return sl.convert(*planes, 1, 0, 0, sr.U16, sr.PLANAR, table, 65535)

    d = _a5(ctx, 3 * 128 * 96 * 2)

    def picture(key, want):
        f.set_rgb_output(d.ptr.value, fmt, nbytes=want.nbytes)
        submit(key)
        return d.download()[:want.nbytes].view(np.uint16).reshape(want.shape)

    plain = through(dec)
    # film grain: the table's picture is the grained one, the DPB holds the decoded one
    sei, poc = sf.make_sei(), 9
    f.set_film_grain(c_params(sei), poc)
    grained = through(sf.apply(dec, sei, poc)[0])
    got = picture(0x100, grained)
    assert np.array_equal(got, grained) and not np.array_equal(got, plain)
    assert all(np.array_equal(a, b) for a, b in zip(engine.DevPic(ctx, dpb.lookup(0x100)[1], owns=False).download(), dec))
    f.set_film_grain(None)
    # output scale to 128 x 96
    f.set_output_scale(128, 96)
    want = through(spp.scale_picture(*dec, 128, 96, (0, 0, 0, 0), (0, 0)))
    assert want.shape == (3, 96, 128)
    assert np.array_equal(picture(0x200, want), want)
    f.set_output_scale(0, 0)
    # reduced to 32 x 24
    f.set_output_reduce(32, 24, (0, 0, 0, 0), 2)
    want = through(sd.reduce_picture(*dec, 32, 24, (0, 0, 0, 0), 2))
    assert want.shape == (3, 24, 32)
    assert np.array_equal(picture(0x300, want), want)
    f.set_output_reduce(0, 0)
    # nothing but the table
    assert np.array_equal(picture(0x400, plain), plain)
    d.free(); lut.close()
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
    fmt = engine.rgb_format(9, 0, 0, capi.RGB_F16, capi.RGB_PLANAR)
    table = lut3d.pq_bt2020_to_bt709(17, 1023)
    t = torch.zeros((n, 3, h, w), dtype=torch.float16, device="cuda:0")
    torch.cuda.synchronize()
    st.set_rgb_output(t, fmt)
    st.set_rgb_lut(table, 1023)
    res, _ = st.run(arr, n, 0, n, flags=capi.STREAM_KEEP | capi.STREAM_HOLD_ALL)
    assert res.status == 0 and res.n_decoded == n
    got = t.cpu().numpy()
    decoded = [st.picture(i, ctx).download() for i in range(n)]
    for i in range(n):
        assert same_bits(got[i], sl.convert(*decoded[i], 9, 0, 0, sr.F16, sr.PLANAR, table, 1023)), i
    # a table the library refuses leaves the setting as it was; replaced by another table; then cleared: the RGB output as before
    bad = table.copy()
    bad[0, 0, 0, 0] = 1024
    assert st.set_rgb_lut(bad, 1023, check=False) == capi.OVHIP_EINVAL
    with pytest.raises(engine.EngineError):
        st.set_rgb_lut(table[:16], 1023)
    t.zero_()
    torch.cuda.synchronize()
    res, _ = st.run(arr, n, 0, n, flags=capi.STREAM_KEEP)
    assert res.status == 0
    assert same_bits(t.cpu().numpy()[n - 1], sl.convert(*decoded[n - 1], 9, 0, 0, sr.F16, sr.PLANAR, table, 1023))
    other = sl.random_table(33, 65535, 2)
    st.set_rgb_lut(other, 65535)
    res, _ = st.run(arr, n, 0, n, flags=capi.STREAM_KEEP)
    assert res.status == 0
    got = t.cpu().numpy()
    for i in range(n):
        assert same_bits(got[i], sl.convert(*decoded[i], 9, 0, 0, sr.F16, sr.PLANAR, other, 65535)), i
    st.set_rgb_lut(None)
    res, _ = st.run(arr, n, 0, n)
    assert res.status == 0
    got = t.cpu().numpy()
    for i in range(n):
        assert same_bits(got[i], sr.convert(*decoded[i], 9, 0, 0, sr.F16, sr.PLANAR)), i
    st.close(); [j.close() for j in jobs]; dpb.close(); ctx.close()
