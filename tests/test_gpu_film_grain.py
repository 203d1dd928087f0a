"""GPU: film grain synthesis on the device (k_film_grain, openvvc_amd/csrc/kernels_grain.hip) and the layers above it.

The kernel against what the reference's fg_grain_apply_pic wrote (tests/golden/film_grain/fg.ovg) and, at sizes people use, against the
numpy restatement tests/spec_film_grain.py (which tests/test_film_grain_cpu.py pins to the same fixture); the synchronous conveniences,
the frame layer and the stream driver against the restatement applied to the ORACLE's decode.  Every comparison is exact: integers."""
import ctypes as C
import hashlib
import sys
from pathlib import Path

import numpy as np
import pytest

import oracle_pipeline
import spec_film_grain as sf
from openvvc_amd import capi, engine, gop, synth

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "oracle"))
import ovvc_oracle_output as oo                                                        # noqa: E402
from test_output_path import WINDOWS                                                   # noqa: E402
from test_gpu_stream import _Keep, _contents, _jobs_for, _make_contents, _oracle_stream, _stream_pics      # noqa: E402
from test_film_grain_cpu import N_CASES, c_params, case                                # noqa: E402

pytestmark = pytest.mark.gpu

NONE = (0, 0, 0, 0)
# luma: 8 intervals, three model values; Cb: 3 intervals, two; Cr: one interval, one
SEI = sf.make_sei(log2_scale=2, comps=((8, 3, 200, 8, 8), (3, 2, 100, 4, 6), (1, 1, 90, 8, 8)))


@pytest.fixture(scope="module")
def ctx(built_lib):
    c = engine.Context(0)
    yield c
    c.close()


def _device_grain(ctx, planes, sei, poc):
    h, w = planes[0].shape
    src = ctx.upload_pic(*planes)
    dst = ctx.new_pic(w, h)
    # the destination starts out as something the result never holds: a sample the kernel leaves out shows
    dst.upload(np.full((h, w), 0xFFFF, np.uint16), np.full((h // 2, w // 2), 0xFFFF, np.uint16), np.full((h // 2, w // 2), 0xFFFF, np.uint16))
    src.grain_into(dst, c_params(sei), poc)
    ctx.sync()
    got, back = dst.download(), src.download()
    src.free(); dst.free()
    assert all(np.array_equal(a, b) for a, b in zip(back, planes)), "the source is only read"
    return got


@pytest.mark.parametrize("k", range(N_CASES))
def test_kernel_equals_the_reference(ctx, k):
    c = case(k)
    got = _device_grain(ctx, c["src"], c["sei"], c["poc"])
    for p, name in enumerate(("Y", "Cb", "Cr")):
        assert got[p].shape == c["exp"][p].shape
        assert np.array_equal(got[p], c["exp"][p]), f"case {k} plane {name}: {int((got[p] != c['exp'][p]).sum())} samples differ from the reference"


# sizes people use (1920x1080: a last stripe of 8 luma / 12 chroma rows, several workgroups per stripe), and the sizes at which the
# reference is undefined and the back-end's own rule holds (blocks inside the plane only): chroma 50 and 4 wide, stripes 4 rows high
SIZES = [(416, 240, 7), (1920, 1080, 255), (3840, 2160, -3), (100, 52, 5), (16, 8, 0), (8, 8, 256), (200, 20, 100000)]


@pytest.mark.parametrize("w,h,poc", SIZES)
def test_kernel_equals_the_restatement(ctx, w, h, poc):
    rs = np.random.RandomState(w * 7 + h)
    # a smooth diagonal ramp plus noise: the blocks of one picture fall into all intervals, samples clip at both ends
    ramp = lambda hh, ww: np.clip((np.add.outer(np.arange(hh) * 400 // hh, np.arange(ww) * 800 // ww) - 80) + rs.randint(-30, 31, (hh, ww)), 0, 1023).astype(np.uint16)
    planes = (ramp(h, w), ramp(h // 2, w // 2), ramp(h // 2, w // 2))
    want, _ = sf.apply(planes, SEI, poc)
    got = _device_grain(ctx, planes, SEI, poc)
    for p, name in enumerate(("Y", "Cb", "Cr")):
        assert np.array_equal(got[p], want[p]), f"{w}x{h} plane {name}: {int((got[p] != want[p]).sum())} samples differ from the restatement"
    assert not np.array_equal(got[0], planes[0])


def test_a_cancelled_sei_and_a_view_with_a_stride(ctx):
    w, h = 416, 240
    rs = np.random.RandomState(5)
    planes = (rs.randint(0, 1024, (h, w)).astype(np.uint16), rs.randint(0, 1024, (h // 2, w // 2)).astype(np.uint16),
              rs.randint(0, 1024, (h // 2, w // 2)).astype(np.uint16))
    cancelled = dict(SEI, cancel=1)
    got = _device_grain(ctx, planes, cancelled, 3)
    assert all(np.array_equal(a, b) for a, b in zip(got, planes))                       # the decoded picture is delivered
    # the upper 64 rows of the picture as a picture of its own: the same planes, the rows below are not touched
    src, dst = ctx.upload_pic(*planes), ctx.upload_pic(*planes)
    src.band(0, 64).grain_into(dst.band(0, 64), c_params(SEI), 9)
    ctx.sync()
    top = tuple(p[:64 // (2 if i else 1)] for i, p in enumerate(planes))
    want, _ = sf.apply(top, SEI, 9)
    got = dst.download()
    for i in range(3):
        n = 64 // (2 if i else 1)
        assert np.array_equal(got[i][:n], want[i]) and np.array_equal(got[i][n:], planes[i][n:])
    src.free(); dst.free()


def test_conveniences_pack_and_fingerprint_the_grained_picture(built_lib):
    w, h, poc = 416, 240, 11
    rs = np.random.RandomState(31)
    planes = (rs.randint(0, 1024, (h, w)).astype(np.uint16), rs.randint(0, 1024, (h // 2, w // 2)).astype(np.uint16),
              rs.randint(0, 1024, (h // 2, w // 2)).astype(np.uint16))
    want, _ = sf.apply(planes, SEI, poc)
    fg = c_params(SEI)
    ctx = engine.Context(0)
    pic = ctx.upload_pic(*planes)
    for win in WINDOWS:
        assert pic.output_grain(fg, poc, win).tobytes() == oo.packed_frame(*want, win), win
        assert pic.digest_grain(fg, poc, win) == oo.picture_digest(*want, win), win
    # the size has been seen: nothing more is allocated
    held = ctx.scratch_bytes()
    assert held >= w * h * 3 + capi.FG_DB_BYTES
    assert pic.output_grain(fg, poc + 1).tobytes() == oo.packed_frame(*sf.apply(planes, SEI, poc + 1)[0], NONE)
    assert ctx.scratch_bytes() == held
    # the source is only read
    assert all(np.array_equal(a, b) for a, b in zip(pic.download(), planes))
    pic.free(); ctx.close()


def test_scale_and_grain_alternate_on_one_scratch_picture_through_every_delivery(built_lib):
    """Both post-process kinds on ONE context (a frame's, so that the frame's PLANES outputs share it), one after the other, through
    the packed frame, the fingerprint, the plain output and the frame's planes: each result is what the same launch into a picture
    of its own gives, and the scratch picture is allocated once, at the larger size.

    ovhip_ctx_scratch_bytes sums every grow-only buffer of the context, so the explicit-destination results are taken FIRST: they
    bring the packing buffer, the digest buffers and the grain database to their final sizes without touching the scratch picture,
    and what step 1 adds afterwards is exactly that picture."""
    w, h, ow, oh, poc = 64, 48, 128, 96, 9
    win = (1, 0, 0, 1)
    sei = sf.make_sei()
    fg = c_params(sei)
    rs = np.random.RandomState(64 * 48)
    planes = (rs.randint(0, 1024, (h, w)).astype(np.uint16), rs.randint(0, 1024, (h // 2, w // 2)).astype(np.uint16),
              rs.randint(0, 1024, (h // 2, w // 2)).astype(np.uint16))
    wl = synth.make_workload(w, h, 77, tools=synth.INTRA_TOOLS, intra_frac=1.0, calllog=True)
    o = oracle_pipeline.decode(wl)
    dec = (o.y, o.cb, o.cr)
    dpb = engine.Dpb((0,))
    f = engine.Frame(dpb, 0, w, h)
    ctx = f.job().ctx                                                                   # the frame's context: not owned
    keep = _Keep()
    params = engine.Job.make_params(keep, wl)
    pic, dpic = ctx.upload_pic(*planes), ctx.upload_pic(*dec)

    # with explicit destination pictures
    scaled, grained, dscaled, dgrained = ctx.new_pic(ow, oh), ctx.new_pic(w, h), ctx.new_pic(ow, oh), ctx.new_pic(w, h)
    pic.scale_into(scaled); pic.grain_into(grained, fg, poc)
    dpic.scale_into(dscaled); dpic.grain_into(dgrained, fg, poc)
    ctx.sync()
    want = [scaled.output(win), grained.output(win), scaled.digest(win), grained.digest(win)]
    want_planes = [dscaled.download(), dgrained.download()]
    assert not np.array_equal(want_planes[1][0], dec[0])                                # (grain was added)
    held0 = ctx.scratch_bytes()

    # 1 .. 5 on the shared scratch picture
    assert np.array_equal(pic.output_scaled(ow, oh, window=win), want[0])
    held = ctx.scratch_bytes()
    assert held - held0 == ow * oh * 3                                                  # the scratch picture at 128 x 96, nothing else
    assert np.array_equal(pic.output_grain(fg, poc, win), want[1]) and ctx.scratch_bytes() == held      # the smaller picture in the larger scratch
    assert pic.digest_scaled(ow, oh, window=win) == want[2] and ctx.scratch_bytes() == held
    assert pic.digest_grain(fg, poc, win) == want[3] and ctx.scratch_bytes() == held
    assert pic.output(win).tobytes() == oo.packed_frame(*planes, win) and ctx.scratch_bytes() == held

    # 6, 7: a frame delivers PLANES into host planes with a stride above the width
    def planes_of(fw, fh, key):
        sy, sc = fw + 24, fw // 2 + 8
        y, cb, cr = (np.full((fh, sy), 0xFFFF, np.uint16), np.full((fh // 2, sc), 0xFFFF, np.uint16), np.full((fh // 2, sc), 0xFFFF, np.uint16))
        out = capi.FrameOutput()
        out.mode, out.y, out.cb, out.cr, out.stride_y, out.stride_c = capi.OUT_PLANES, y.ctypes.data, cb.ctypes.data, cr.ctypes.data, sy, sc
        f.begin(key)
        f.recorder().replay(wl.calllog)
        f.submit(params, out=out)
        assert (y[:, fw:] == 0xFFFF).all() and (cb[:, fw // 2:] == 0xFFFF).all() and (cr[:, fw // 2:] == 0xFFFF).all()
        return y[:, :fw], cb[:, :fw // 2], cr[:, :fw // 2]

    f.set_output_scale(ow, oh)
    assert all(np.array_equal(a, b) for a, b in zip(planes_of(ow, oh, 0x100), want_planes[0]))
    f.set_output_scale(0, 0)
    f.set_film_grain(fg, poc)
    assert all(np.array_equal(a, b) for a, b in zip(planes_of(w, h, 0x200), want_planes[1]))
    assert ctx.scratch_bytes() == held

    # the sources are only read
    assert all(np.array_equal(a, b) for a, b in zip(pic.download(), planes))
    for key in (0x100, 0x200):
        assert all(np.array_equal(a, b) for a, b in zip(engine.DevPic(ctx, dpb.lookup(key)[1], owns=False).download(), dec))
    for p in (pic, dpic, scaled, grained, dscaled, dgrained):
        p.free()
    f.close(); dpb.close()


def _packed_out(win, w, h):
    out = capi.FrameOutput()
    cwin = capi.Window(*win)
    buf = np.zeros(capi.load().ovhip_output_bytes(w, h, C.byref(cwin)) // 2, np.uint16)
    out.mode, out.window, out.packed = capi.OUT_PACKED, cwin, buf.ctypes.data
    return out, buf


def test_frame_outputs_the_grained_picture_and_publishes_the_decoded_one(built_lib):
    w, h = 416, 240
    win = (1, 0, 2, 1)
    wl = synth.make_workload(w, h, 61, tools=synth.INTRA_TOOLS, intra_frac=1.0, calllog=True)
    o = oracle_pipeline.decode(wl)
    dec = (o.y, o.cb, o.cr)
    fg = c_params(SEI)
    dpb = engine.Dpb((0,))
    ctx = engine.Context(0)
    f = engine.Frame(dpb, 0, w, h)
    keep = _Keep()
    params = engine.Job.make_params(keep, wl)

    def submit(key, out):
        f.begin(key)
        f.recorder().replay(wl.calllog)
        f.submit(params, out=out)

    # before: the decoded picture
    out, buf = _packed_out(win, w, h)
    submit(0x100, out)
    before = buf.tobytes()
    assert before == oo.packed_frame(*dec, win)
    # PACKED
    f.set_film_grain(fg, 5)
    out, buf = _packed_out(win, w, h)
    submit(0x200, out)
    assert buf.tobytes() == oo.packed_frame(*sf.apply(dec, SEI, 5)[0], win) != before
    # PLANES, another POC
    f.set_film_grain(fg, 256)
    want = sf.apply(dec, SEI, 256)[0]
    y, cb, cr = np.zeros((h, w), np.uint16), np.zeros((h // 2, w // 2), np.uint16), np.zeros((h // 2, w // 2), np.uint16)
    out = capi.FrameOutput()
    out.mode, out.y, out.cb, out.cr, out.stride_y, out.stride_c = capi.OUT_PLANES, y.ctypes.data, cb.ctypes.data, cr.ctypes.data, w, w // 2
    submit(0x300, out)
    assert np.array_equal(y, want[0]) and np.array_equal(cb, want[1]) and np.array_equal(cr, want[2])
    # DIGEST: the same params for the next picture are derived afresh (no drift)
    out = capi.FrameOutput()
    out.mode, out.window = capi.OUT_DIGEST, capi.Window(*win)
    submit(0x400, out)
    assert bytes(out.digest) == oo.picture_digest(*want, win)
    # what the DPB holds is the decoded picture
    for key in (0x200, 0x300, 0x400):
        _dev, pic = dpb.lookup(key)
        dp = engine.DevPic(ctx, pic, owns=False)
        assert dp.digest() == oo.picture_digest(*dec)
        assert all(np.array_equal(a, b) for a, b in zip(dp.download(), dec))
    # grain and an output scale exclude each other; a refused model leaves the setting as it was; switched off, the output is what it was
    assert f.set_output_scale(2 * w, 2 * h, check=False) == capi.OVHIP_EUNSUP
    assert f.set_film_grain(c_params(dict(SEI, blending_mode=1)), 0, check=False) == capi.OVHIP_EUNSUP
    out = capi.FrameOutput()
    out.mode, out.window = capi.OUT_DIGEST, capi.Window(*win)
    submit(0x500, out)
    assert bytes(out.digest) == oo.picture_digest(*want, win)
    f.set_film_grain(None)
    out, buf = _packed_out(win, w, h)
    submit(0x600, out)
    assert buf.tobytes() == before
    f.set_output_scale(2 * w, 2 * h)
    assert f.set_film_grain(fg, 0, check=False) == capi.OVHIP_EUNSUP
    f.close(); ctx.close(); dpb.close()


def test_the_last_band_outputs_the_grained_picture_too(built_lib):
    """ovhip_frame_band's last call shares the output helper of ovhip_frame_submit: the same picture as ONE band"""
    w, h = 416, 240
    win = (0, 2, 1, 0)
    wl = synth.make_workload(w, h, 61, tools=synth.INTRA_TOOLS, intra_frac=1.0, calllog=True)
    o = oracle_pipeline.decode(wl)
    want = sf.apply((o.y, o.cb, o.cr), SEI, 100000)[0]
    lib = capi.load()
    dpb = engine.Dpb((0,))
    ctx = engine.Context(0)
    f = engine.Frame(dpb, 0, w, h)
    keep = _Keep()
    params = engine.Job.make_params(keep, wl)
    f.begin(0x100)
    f.recorder().replay(wl.calllog)
    assert lib.ovhip_frame_set_band_mode(f.f, 1) == 0
    f.set_film_grain(c_params(SEI), 100000)
    out, buf = _packed_out(win, w, h)
    assert lib.ovhip_frame_band(f.f, C.byref(params), h, 1, C.byref(out)) == 1, lib.ovhip_frame_last_error(f.f)
    assert buf.tobytes() == oo.packed_frame(*want, win)
    _dev, pic = dpb.lookup(0x100)
    assert engine.DevPic(ctx, pic, owns=False).digest() == oo.picture_digest(o.y, o.cb, o.cr)
    f.close(); ctx.close(); dpb.close()


def test_stream_driver_writes_the_grained_file(built_lib):
    """OVHIP_OUT_PACKED + OVHIP_STREAM_FILE_MD5 with film grain: the frames of the file are the grained pictures in output order, each
    at its own POC"""
    w, h = 416, 240
    win = (1, 2, 0, 3)
    wls = _contents(w, h, (41, 42), 43)
    pics = gop.build_stream(2, 8, 16, 1)
    spics = _stream_pics(pics, 2)
    planes = _oracle_stream(wls, spics)
    order = sorted(range(len(spics)), key=lambda i: spics[i]["poc"])
    grained = {i: sf.apply(planes[i], SEI, spics[i]["poc"])[0] for i in order}
    today = hashlib.md5(b"".join(oo.packed_frame(*planes[i], win) for i in order)).digest()
    want = hashlib.md5(b"".join(oo.packed_frame(*grained[i], win) for i in order)).digest()
    fg = c_params(SEI)
    ctx = engine.Context(0)
    dpb = engine.Dpb((0,))
    jobs = _jobs_for(ctx, wls, spics, w, h)
    st = engine.Stream(dpb, w, h, _make_contents(wls), jobs, threads_per_device=4, output=capi.OUT_PACKED, window=win)
    arr = st.pics_array(spics)
    n = len(spics)
    res, _ = st.run(arr, n, 0, n, flags=capi.STREAM_FILE_MD5)
    assert bytes(res.out_md5) == today
    assert st.set_film_grain(c_params(dict(SEI, model_id=1)), check=False) == capi.OVHIP_EUNSUP      # refused before anything runs
    st.set_film_grain(fg)
    assert st.set_output_scale(2 * w, 2 * h, check=False) == capi.OVHIP_EUNSUP
    res, _ = st.run(arr, n, 0, n, flags=capi.STREAM_FILE_MD5)
    assert res.out_frames == n and bytes(res.out_md5) == want != today
    assert dpb.stats().n_live == 0
    st.set_film_grain(None)
    res, _ = st.run(arr, n, 0, n, flags=capi.STREAM_FILE_MD5)
    assert bytes(res.out_md5) == today
    st.close()
    # the frame threads' DIGEST path
    st = engine.Stream(dpb, w, h, _make_contents(wls), jobs, threads_per_device=4, output=capi.OUT_DIGEST, window=win)
    st.set_film_grain(fg)
    res, dg = st.run(arr, n, 0, n, digests=True)
    assert bytes(res.out_md5) == hashlib.md5(b"".join(oo.picture_digest(*grained[i], win) for i in order)).digest()
    for i in range(n):
        assert bytes(dg[i]) == oo.picture_digest(*grained[i], win), i
    st.close(); [j.close() for j in jobs]; dpb.close(); ctx.close()


def test_refusals_come_back_before_anything_is_launched(ctx):
    """return values only: nothing is provoked on the device"""
    fg = c_params(SEI)
    a, b = ctx.new_pic(128, 96), ctx.new_pic(64, 48)
    assert a.grain_into(b, fg, 0, check=False) == capi.OVHIP_EINVAL                     # sizes differ
    assert a.grain_into(a, fg, 0, check=False) == capi.OVHIP_EINVAL                     # aliasing: the picture itself, and a view into it
    assert "aliases" in ctx.lib.ovhip_last_error(ctx.h).decode()
    c = ctx.new_pic(128, 48)
    assert a.band(0, 48).grain_into(a.band(16, 48), fg, 0, check=False) == capi.OVHIP_EINVAL
    s = capi.Pic(b.s.y, b.s.cb, None, b.s.w, b.s.h, b.s.stride_y, b.s.stride_c)          # a missing plane
    assert engine.DevPic(ctx, s, owns=False).grain_into(b, fg, 0, check=False) == capi.OVHIP_EINVAL
    odd1, odd2 = ctx.new_pic(130, 98), ctx.new_pic(130, 98)                             # sizes that are not multiples of 4
    assert odd1.grain_into(odd2, fg, 0, check=False) == capi.OVHIP_EINVAL
    # a model that points outside the database (built by hand: ovhip_fg_derive never makes one)
    r, model, _ = capi.fg_derive(ctx.lib, fg)
    assert r == 0
    model.entry[0][40] = capi.FG_VALID | 100 | (13 << 16)
    b2 = ctx.new_pic(64, 48)
    assert ctx.lib.ovhip_film_grain_launch(ctx.h, C.byref(b.s), C.byref(model), 0, 0, C.byref(b2.s)) == capi.OVHIP_EINVAL
    # the conveniences refuse likewise, and allocate nothing for it
    held = ctx.scratch_bytes()
    out = np.zeros(130 * 98 * 3 // 2, np.uint16)
    assert ctx.lib.ovhip_pic_output_grain(ctx.h, C.byref(odd1.s), C.byref(model), 0, None, out.ctypes.data) == capi.OVHIP_EINVAL
    assert ctx.scratch_bytes() == held
    for p in (a, b, c, b2, odd1, odd2):
        p.free()
