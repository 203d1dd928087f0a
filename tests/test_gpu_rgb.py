"""GPU: RGB output on the device (openvvc_amd/csrc/kernels_rgb.hip): ovhip_rgb_launch and ovhip_pic_output_rgb against the host twin
and the numpy restatement tests/spec_rgb.py, destinations that are only element-aligned, the frame thread (alone, with film grain,
with an output scale, band-wise), the stream driver into a torch tensor.  The definition is integer only: every comparison is of
bytes."""
import ctypes as C
import itertools

import numpy as np
import pytest

import spec_film_grain as sf
import spec_pp_scale as spp
import spec_rgb as sr
from openvvc_amd import capi, engine, gop
from test_film_grain_cpu import c_params
from test_gpu_pic_hash import _frame_case
from test_gpu_stream import _Keep, _contents, _jobs_for, _make_contents, _stream_pics
from test_rgb_cpu import DTYPES, LAYOUTS, WINDOWS, host_rgb, same_bits

pytestmark = pytest.mark.gpu

# a plane narrower than one lane's run of 8 pixels (and a window that leaves 2 columns of it); rows that are no multiple of 16 bytes in
# any dtype (20, and 70 / 18 under the windows); a row tail; more than one wave per row pair (136: 17 runs); more than one workgroup
SIZES = [(8, 8), (20, 12), (24, 8), (72, 40), (136, 72), (264, 136)]
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


def _check_formats(ctx, planes, formats, windows=WINDOWS):
    """launch, convenience and host twin against the restatement for every (matrix, range, location) of `formats` x dtype x layout x window"""
    h, w = planes[0].shape
    pic = ctx.upload_pic(*planes)
    d = ctx.alloc(3 * w * h * 4)
    for matrix, full, loc in formats:
        ints = {nb: sr.rgb_int(*planes, matrix, full, loc, nb) for nb in (8, 10)}          # the reference, once per coefficient set
        for dtype, layout, wd in itertools.product(DTYPES, LAYOUTS, windows):
            fmt = capi.RgbFormat(matrix, full, loc, dtype, layout)
            want = sr.store(ints[sr.n_bits(dtype)], dtype, layout, wd)
            what = (w, h, matrix, full, loc, dtype, layout, wd)
            assert same_bits(host_rgb(ctx.lib, planes, fmt, wd), want), what
            pic.rgb_into(d.ptr.value, want.nbytes, fmt, wd)
            ctx.sync()
            assert same_bits(_as_picture(d.download(), fmt, w, h, wd), want), what
            assert same_bits(pic.rgb(fmt, wd), want), what
    assert all(np.array_equal(a, b) for a, b in zip(pic.download(), planes)), "the picture is only read"
    d.free(); pic.free()


@pytest.mark.parametrize("w,h", SIZES)
def test_launch_and_convenience_equal_host_and_restatement(ctx, w, h):
    _check_formats(ctx, sr.random_planes(w, h, 31 * w + h), [(1, 0, 0), (1, 0, 2), (9, 1, 0), (9, 1, 2)])


@pytest.mark.parametrize("matrix", sr.MATRICES)
def test_every_format_at_72x40(ctx, matrix):
    _check_formats(ctx, sr.random_planes(72, 40, 500 + matrix), [(matrix, full, loc) for full in (0, 1) for loc in range(6)])


@pytest.mark.parametrize("w,h", [(72, 40), (20, 12)])
def test_every_instantiation_and_vertical_case(ctx, w, h):
    """every k_rgb<dtype, layout, a> under every row selection b: the six chroma locations are a = loc & 1 with b = 1, 1, 0, 0, 2, 2, each
    in every dtype and layout over the full window.  72 x 40: nine full runs per row, twenty row pairs; 20 x 12: a run tail of 4"""
    _check_formats(ctx, sr.random_planes(w, h, 77 + w), [(9, 0, loc) for loc in range(6)], [(0, 0, 0, 0)])


@pytest.mark.parametrize("w,h,wd", [(20, 12, (0, 0, 0, 0)), (72, 40, (1, 0, 0, 1)), (136, 72, (0, 0, 0, 0))])
def test_a_destination_offset_by_one_element(ctx, w, h, wd):
    """a slice of a batch tensor at odd sizes is aligned to its element and to nothing more: the bytes around it stay as they were"""
    planes = sr.random_planes(w, h, 9)
    pic = ctx.upload_pic(*planes)
    for dtype, layout in itertools.product(DTYPES, LAYOUTS):
        fmt = capi.RgbFormat(5, 0, 1, dtype, layout)
        want = sr.convert(*planes, 5, 0, 1, dtype, layout, wd)
        es = ES[dtype]
        for lead in (es, 3 * es, 16 + es):
            d = _a5(ctx, lead + want.nbytes + 37)
            pic.rgb_into(d.ptr.value + lead, want.nbytes, fmt, wd)
            ctx.sync()
            raw = d.download()
            assert (raw[:lead] == 0xA5).all() and (raw[lead + want.nbytes:] == 0xA5).all(), (dtype, layout, lead)
            assert raw[lead:lead + want.nbytes].tobytes() == want.tobytes(), (dtype, layout, lead)
            d.free()
    pic.free()


def test_a_view_with_a_stride_above_its_width(ctx):
    """the left 72 columns of a 136x72 picture as a picture of its own (chroma rows of stride 68: not 8-byte aligned), and the same
    view moved 4 columns to the right (luma rows not 16-byte aligned): the chroma taps clamp at the VIEW's edge"""
    planes = sr.random_planes(136, 72, 3)
    pic = ctx.upload_pic(*planes)
    for x in (0, 4):
        s = capi.Pic(pic.s.y + 2 * x, pic.s.cb + x, pic.s.cr + x, 72, 72, pic.s.stride_y, pic.s.stride_c)
        view = engine.DevPic(ctx, s, owns=False)
        part = (planes[0][:, x:x + 72], planes[1][:, x // 2:x // 2 + 36], planes[2][:, x // 2:x // 2 + 36])
        for dtype, layout, loc in itertools.product((sr.U8, sr.F16), LAYOUTS, (1, 4)):
            fmt = capi.RgbFormat(1, 0, loc, dtype, layout)
            for wd in WINDOWS:
                assert same_bits(view.rgb(fmt, wd), sr.convert(*part, 1, 0, loc, dtype, layout, wd)), (x, dtype, layout, loc, wd)
    whole = sr.convert(*planes, 1, 0, 1, sr.U16, sr.PLANAR)
    assert not np.array_equal(whole[:, :, :72], sr.convert(planes[0][:, :72], planes[1][:, :36], planes[2][:, :36], 1, 0, 1, sr.U16, sr.PLANAR))
    pic.free()


def test_scratch_stays_flat_over_repeated_launches(built_lib):
    ctx = engine.Context(0)
    planes = sr.random_planes(264, 136, 1)
    pic = ctx.upload_pic(*planes)
    d = ctx.alloc(3 * 264 * 136 * 4)
    before = ctx.scratch_bytes()
    for rep in range(3):
        for dtype, layout in itertools.product(DTYPES, LAYOUTS):
            pic.rgb_into(d.ptr.value, d.nbytes, capi.RgbFormat(1, 0, 0, dtype, layout))
    ctx.sync()
    assert ctx.scratch_bytes() == before, "the launch allocates nothing"
    fmt = capi.RgbFormat(1, 0, 0, sr.F32, sr.PLANAR)
    first = pic.rgb(fmt)                                                   # the convenience: its scratch at the largest size first
    held = ctx.scratch_bytes()
    assert held - before >= first.nbytes
    for rep in range(2):
        for dtype, layout in itertools.product(DTYPES, LAYOUTS):
            pic.rgb(capi.RgbFormat(1, 0, 0, dtype, layout), (1, 0, 0, 1))
            assert ctx.scratch_bytes() == held
    d.free(); pic.free(); ctx.close()


def test_refusals_come_back_before_anything_is_launched(ctx):
    """return values and the error text only: nothing is provoked on the device, and the destination stays as it was"""
    w, h = 72, 40
    pic = ctx.upload_pic(*sr.random_planes(w, h, 2))
    ok = capi.RgbFormat(1, 0, 0, sr.U16, sr.PLANAR)
    need = ctx.lib.ovhip_rgb_bytes(w, h, None, C.byref(ok))
    d = _a5(ctx, need)
    held = ctx.scratch_bytes()
    P = pic.s

    def view(**kw):
        f = dict(y=P.y, cb=P.cb, cr=P.cr, w=P.w, h=P.h, stride_y=P.stride_y, stride_c=P.stride_c)
        f.update(kw)
        return engine.DevPic(ctx, capi.Pic(f["y"], f["cb"], f["cr"], f["w"], f["h"], f["stride_y"], f["stride_c"]), owns=False)

    cases = [
        ("null destination", pic, ok, None, 0, need, capi.OVHIP_EINVAL),
        ("too small", pic, ok, None, d.ptr.value, need - 1, capi.OVHIP_EINVAL),
        ("overlaps", pic, ok, None, P.cb, 1 << 20, capi.OVHIP_EINVAL),
        ("window leaves nothing", pic, ok, (18, 18, 0, 0), d.ptr.value, need, capi.OVHIP_EINVAL),
        ("missing plane", view(cr=None), ok, None, d.ptr.value, need, capi.OVHIP_EINVAL),
        ("stride below the width", view(stride_c=w // 2 - 2), ok, None, d.ptr.value, need, capi.OVHIP_EINVAL),
        ("multiples of 4", view(w=w - 2), ok, None, d.ptr.value, need, capi.OVHIP_EINVAL),
        ("multiples of 4", view(h=h - 2), ok, None, d.ptr.value, need, capi.OVHIP_EINVAL),
        ("bad dtype", pic, capi.RgbFormat(1, 0, 0, 4, 0), None, d.ptr.value, 1 << 20, capi.OVHIP_EINVAL),
        ("bad dtype", pic, capi.RgbFormat(1, 0, 0, 1, 2), None, d.ptr.value, need, capi.OVHIP_EINVAL),
        ("bad dtype", pic, capi.RgbFormat(1, 0, 6, 1, 0), None, d.ptr.value, need, capi.OVHIP_EINVAL),
        ("unspecified", pic, capi.RgbFormat(2, 0, 0, 1, 0), None, d.ptr.value, need, capi.OVHIP_EINVAL),
        ("not built", pic, capi.RgbFormat(14, 0, 0, 1, 0), None, d.ptr.value, need, capi.OVHIP_EUNSUP),
        ("not aligned", pic, ok, (1, 0, 0, 0), d.ptr.value + 1, need - 1, capi.OVHIP_EINVAL),
    ]
    for text, p, fmt, wd, ptr, nbytes, code in cases:
        assert p.rgb_into(ptr, nbytes, fmt, wd or (0, 0, 0, 0), check=False) == code, text
        assert text in ctx.lib.ovhip_last_error(ctx.h).decode(), (text, ctx.lib.ovhip_last_error(ctx.h))
    # the convenience refuses the same way, into host memory that stays as it was
    host = np.full(need, 0xA5, np.uint8)
    assert ctx.lib.ovhip_pic_output_rgb(ctx.h, C.byref(P), None, C.byref(ok), host.ctypes.data, need - 1) == capi.OVHIP_EINVAL
    assert ctx.lib.ovhip_pic_output_rgb(ctx.h, C.byref(P), C.byref(capi.Window(18, 18, 0, 0)), C.byref(ok), host.ctypes.data, need) == capi.OVHIP_EINVAL
    assert ctx.lib.ovhip_pic_output_rgb(ctx.h, C.byref(P), None, C.byref(capi.RgbFormat(0, 0, 0, 1, 0)), host.ctypes.data, need) == capi.OVHIP_EUNSUP
    ctx.sync()
    assert (host == 0xA5).all() and (d.download() == 0xA5).all()
    assert ctx.scratch_bytes() == held
    d.free(); pic.free()


def test_python_layer_checks_the_tensor(built_lib):
    import torch
    fmt = engine.rgb_format(dtype=capi.RGB_F16, layout=capi.RGB_PLANAR)
    shape = engine.rgb_shape(fmt, 64, 48)
    assert shape == (3, 48, 64) and engine.rgb_shape(engine.rgb_format(layout=capi.RGB_PACKED), 64, 48, (1, 0, 0, 1)) == (46, 62, 3)
    good = torch.zeros(shape, dtype=torch.float16, device="cuda:0")
    assert engine._rgb_tensor(good, fmt, shape) == (good.data_ptr(), 3 * 48 * 64 * 2)
    batch = torch.zeros((5, *shape), dtype=torch.float16, device="cuda:0")
    assert engine._rgb_tensor(batch, fmt, shape, 5) == (batch.data_ptr(), 3 * 48 * 64 * 2)
    for bad in (torch.zeros(shape, dtype=torch.float32, device="cuda:0"), torch.zeros(shape, dtype=torch.float16),
                torch.zeros((48, 64, 3), dtype=torch.float16, device="cuda:0"), batch[:, :, :, ::2], np.zeros(shape, np.float16)):
        with pytest.raises(engine.EngineError):
            engine._rgb_tensor(bad, fmt, shape)
    with pytest.raises(engine.EngineError):
        engine._rgb_tensor(batch, fmt, shape, 4)


def test_frame_writes_the_picture_the_output_shows(built_lib):
    import torch
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

    # OVHIP_OUT_NONE (no output description at all, then one that says NONE), a torch tensor as the destination
    fmt = engine.rgb_format(1, 0, 0, capi.RGB_F16, capi.RGB_PLANAR)
    t = torch.full((3, h, w), 7.0, dtype=torch.float16, device="cuda:0")
    torch.cuda.synchronize()
    f.set_rgb_output(t, fmt)
    assert submit(0x100) == 0
    want = sr.convert(*dec, 1, 0, 0, sr.F16, sr.PLANAR)
    assert same_bits(t.cpu().numpy(), want)
    assert all(np.array_equal(a, b) for a, b in zip(published(0x100), dec))
    # per picture: a second submit without a new call converts nothing
    t.fill_(7.0)
    torch.cuda.synchronize()
    out = capi.FrameOutput()
    out.mode = capi.OUT_NONE
    assert submit(0x101, out) == 0
    assert (t.cpu().numpy() == 7.0).all()
    # a window, packed uint8, a raw device address
    wd = (1, 0, 0, 1)
    fmt8 = engine.rgb_format(9, 1, 3, capi.RGB_U8, capi.RGB_PACKED)
    want8 = sr.convert(*dec, 9, 1, 3, sr.U8, sr.PACKED, wd)
    d = _a5(ctx, want8.nbytes + 16)
    f.set_rgb_output(d.ptr.value, fmt8, wd, nbytes=want8.nbytes)
    assert submit(0x102, out) == 0
    raw = d.download()
    assert raw[:want8.nbytes].tobytes() == want8.tobytes() and (raw[want8.nbytes:] == 0xA5).all()
    # switched off again before the picture: the destination stays as it was
    d2 = _a5(ctx, want8.nbytes)
    f.set_rgb_output(d2.ptr.value, fmt8, wd, nbytes=want8.nbytes)
    f.set_rgb_output(None, None)
    assert submit(0x103) == 0
    assert (d2.download() == 0xA5).all()
    # the format's refusals come from the setter; a destination that is too small fails the call, not the publication
    assert f.set_rgb_output(d2.ptr.value, engine.rgb_format(2), nbytes=1 << 20, check=False) == capi.OVHIP_EINVAL
    assert f.set_rgb_output(d2.ptr.value, engine.rgb_format(4), nbytes=1 << 20, check=False) == capi.OVHIP_EUNSUP
    assert f.set_rgb_output(0, fmt8, nbytes=1 << 20, check=False) == capi.OVHIP_EINVAL
    f.set_rgb_output(d2.ptr.value, fmt8, wd, nbytes=want8.nbytes - 1)
    assert submit(0x104, check=False) == capi.OVHIP_EINVAL
    assert b"too small" in built_lib.ovhip_frame_last_error(f.f)
    assert (d2.download() == 0xA5).all()
    assert all(np.array_equal(a, b) for a, b in zip(published(0x104), dec))
    # the last band of a band-wise picture converts too
    d3 = _a5(ctx, want8.nbytes)
    f.set_rgb_output(d3.ptr.value, fmt8, wd, nbytes=want8.nbytes)
    f.begin(0x105)
    f.recorder().replay(wl.calllog)
    assert built_lib.ovhip_frame_set_band_mode(f.f, 1) == 0
    assert built_lib.ovhip_frame_band(f.f, C.byref(params), h, 1, None) == 1, built_lib.ovhip_frame_last_error(f.f)
    assert d3.download().tobytes() == want8.tobytes()
    assert built_lib.ovhip_frame_set_band_mode(f.f, 0) == 0
    [b.free() for b in (d, d2, d3)]
    f.close(); ctx.close(); dpb.close()


def test_frame_composes_with_film_grain_and_with_the_output_scale(built_lib):
    w, h, wl, dec = _frame_case()
    dpb = engine.Dpb((0,))
    ctx = engine.Context(0)
    f = engine.Frame(dpb, 0, w, h)
    params = engine.Job.make_params(_Keep(), wl)

    def submit(key):
        f.begin(key)
        f.recorder().replay(wl.calllog)
        assert f.submit(params) == 0

    fmt = engine.rgb_format(1, 0, 0, capi.RGB_U16, capi.RGB_PLANAR)
    plain = sr.convert(*dec, 1, 0, 0, sr.U16, sr.PLANAR)
    d = _a5(ctx, 3 * 128 * 96 * 2)
    # film grain: the RGB picture is the grained one, the DPB holds the decoded one
    sei, poc = sf.make_sei(), 9
    f.set_film_grain(c_params(sei), poc)
    f.set_rgb_output(d.ptr.value, fmt, nbytes=plain.nbytes)
    submit(0x100)
    grained = sr.convert(*sf.apply(dec, sei, poc)[0], 1, 0, 0, sr.U16, sr.PLANAR)
    got = d.download()[:plain.nbytes].view(np.uint16).reshape(plain.shape)
    assert np.array_equal(got, grained) and not np.array_equal(got, plain)
    assert all(np.array_equal(a, b) for a, b in zip(engine.DevPic(ctx, dpb.lookup(0x100)[1], owns=False).download(), dec))
    f.set_film_grain(None)
    # output scale to 128 x 96: the RGB picture has the output's size
    f.set_output_scale(128, 96)
    want = sr.convert(*spp.scale_picture(*dec, 128, 96, (0, 0, 0, 0), (0, 0)), 1, 0, 0, sr.U16, sr.PLANAR)
    assert want.shape == (3, 96, 128)
    f.set_rgb_output(d.ptr.value, fmt, nbytes=want.nbytes)
    submit(0x200)
    assert d.download().tobytes() == want.tobytes()
    _dev, held = dpb.lookup(0x200)
    assert (held.w, held.h) == (w, h)
    d.free()
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
    fmt = engine.rgb_format(1, 0, 0, capi.RGB_F16, capi.RGB_PLANAR)
    t = torch.zeros((n, 3, h, w), dtype=torch.float16, device="cuda:0")
    torch.cuda.synchronize()
    st.set_rgb_output(t, fmt)
    res, _ = st.run(arr, n, 0, n, flags=capi.STREAM_KEEP | capi.STREAM_HOLD_ALL)
    assert res.status == 0 and res.n_decoded == n
    got = t.cpu().numpy()
    want = [sr.convert(*st.picture(i, ctx).download(), 1, 0, 0, sr.F16, sr.PLANAR) for i in range(n)]
    for i in range(n):
        assert same_bits(got[i], want[i]), i
    # the pictures differ from one another -- but for 0 and 1, which are the stream's one recorded I picture twice (POC 0 and POC 4)
    assert (spics[0]["content"], spics[0]["refs"]) == (spics[1]["content"], spics[1]["refs"])
    for i, j in itertools.combinations(range(n), 2):
        assert (want[i].tobytes() != want[j].tobytes()) == ((i, j) != (0, 1)), (i, j)
    # n_slots = 2: picture idx lands in slot idx % 2.  One run per pair of pictures, so that no two pictures in flight share a slot
    t2 = torch.zeros((2, 3, h, w), dtype=torch.float16, device="cuda:0")
    torch.cuda.synchronize()
    st.set_rgb_output(t2, fmt)
    for first, cnt in ((0, 2), (2, 2), (4, 1)):
        res, _ = st.run(arr, n, first, cnt, flags=capi.STREAM_KEEP)
        assert res.status == 0 and res.n_decoded == cnt
        got = t2.cpu().numpy()
        last = first + cnt - 1
        for slot in range(2):
            idx = last if last % 2 == slot else last - 1
            assert same_bits(got[slot], want[idx]), (first, slot)
    # a bytes_per_picture that is too small, a bad slot count, a tensor of the wrong shape
    need = built_lib.ovhip_rgb_bytes(w, h, None, C.byref(fmt))
    assert st.set_rgb_output(t2.data_ptr(), fmt, bytes_per_picture=need - 1, n_slots=2, check=False) == capi.OVHIP_EINVAL
    assert st.set_rgb_output(t2.data_ptr(), fmt, bytes_per_picture=need, n_slots=0, check=False) == capi.OVHIP_EINVAL
    assert st.set_rgb_output(t2.data_ptr(), fmt, (1, 0, 0, 1), bytes_per_picture=need - 1, n_slots=2, check=False) == 0       # (the window needs less)
    with pytest.raises(engine.EngineError):
        st.set_rgb_output(t2[:, :, :-2], fmt)
    # off again: the tensor stays as it is
    st.set_rgb_output(None, None)
    t2.zero_()
    torch.cuda.synchronize()
    res, _ = st.run(arr, n, 0, n)
    assert res.status == 0 and not t2.any().item()
    assert dpb.stats().n_live == 0
    st.close(); [j.close() for j in jobs]; dpb.close(); ctx.close()
