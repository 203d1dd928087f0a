"""GPU: output resampling on the device (k_output_scale, openvvc_amd/csrc/kernels_scale.hip) and the layers above it.

The kernel against what the reference's pp_sample_rate_conv wrote (tests/golden/pp_scale/*.ovg) and, at sizes people use, against the
numpy restatement tests/spec_pp_scale.py (which tests/test_pp_scale_cpu.py pins to the same fixture); the synchronous conveniences,
the frame layer and the stream driver against the restatement applied to the ORACLE's decode.  Every comparison is exact: integers."""
import ctypes as C
import hashlib
import sys
from pathlib import Path

import numpy as np
import pytest

import oracle_pipeline
import spec_pp_scale as sp
from openvvc_amd import capi, engine, gop, synth

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "oracle"))
import ovvc_oracle_output as oo                                                        # noqa: E402
from test_output_path import WINDOWS                                                   # noqa: E402
from test_gpu_stream import _Keep, _contents, _jobs_for, _make_contents, _oracle_stream, _stream_pics      # noqa: E402

pytestmark = pytest.mark.gpu

CASES = sp.load_cases()
NONE = (0, 0, 0, 0)


def _device_scale(ctx, planes, dst_w, dst_h, win, col):
    src = ctx.upload_pic(*planes)
    dst = ctx.new_pic(dst_w, dst_h)
    # the destination starts out as something the result never holds: a sample the kernel leaves out shows
    dst.upload(np.full((dst_h, dst_w), 0xFFFF, np.uint16), np.full((dst_h // 2, dst_w // 2), 0xFFFF, np.uint16),
               np.full((dst_h // 2, dst_w // 2), 0xFFFF, np.uint16))
    src.scale_into(dst, win, col)
    ctx.sync()
    got = dst.download()
    src.free(); dst.free()
    return got


@pytest.mark.parametrize("k", range(len(CASES)))
def test_kernel_equals_the_reference(built_lib, k):
    c = CASES[k]
    ctx = engine.Context(0)
    got = _device_scale(ctx, c["src"], c["dst_w"], c["dst_h"], c["win"], c["col"])
    for p, name in enumerate(("Y", "Cb", "Cr")):
        assert got[p].shape == c["exp"][p].shape
        assert np.array_equal(got[p], c["exp"][p]), f"case {k} plane {name}: {int((got[p] != c['exp'][p]).sum())} samples differ from the reference"
    ctx.close()


# (source, destination, scaling window, collocation flags): the sizes people use -- window offsets in two of them, the four
# collocation combinations -- and two shapes whose chroma planes are not 8- / 16-byte alignable (the kernel's narrow paths)
SIZES = [((1920, 1080), (3840, 2160), NONE, (0, 0)),
         ((2560, 1440), (3840, 2160), (2, 2, 1, 1), (1, 0)),
         ((1280, 720), (1920, 1080), (0, 4, 2, 0), (0, 1)),
         ((416, 240), (832, 480), NONE, (1, 1)),
         ((3840, 2160), (3840, 2160), NONE, (0, 0)),
         ((100, 52), (200, 100), NONE, (0, 1)),
         ((100, 52), (108, 60), (1, 0, 0, 1), (1, 0))]


@pytest.mark.parametrize("src,dst,win,col", SIZES)
def test_kernel_equals_the_restatement(built_lib, src, dst, win, col):
    assert sp.is_upsampling(src[0], src[1], win, col, dst[0], dst[1])        # (before the GPU is touched)
    rs = np.random.RandomState(src[0] * 7 + dst[1])
    planes = (rs.randint(0, 1024, (src[1], src[0])).astype(np.uint16), rs.randint(0, 1024, (src[1] // 2, src[0] // 2)).astype(np.uint16),
              rs.randint(0, 1024, (src[1] // 2, src[0] // 2)).astype(np.uint16))
    want = sp.scale_picture(*planes, dst[0], dst[1], win, col)
    ctx = engine.Context(0)
    got = _device_scale(ctx, planes, dst[0], dst[1], win, col)
    for p, name in enumerate(("Y", "Cb", "Cr")):
        assert np.array_equal(got[p], want[p]), f"{src} -> {dst} plane {name}: {int((got[p] != want[p]).sum())} samples differ from the restatement"
    ctx.close()


def test_conveniences_pack_and_fingerprint_the_resampled_picture(built_lib):
    w, h, ow, oh = 416, 240, 832, 480
    col = (1, 0)
    rs = np.random.RandomState(31)
    planes = (rs.randint(0, 1024, (h, w)).astype(np.uint16), rs.randint(0, 1024, (h // 2, w // 2)).astype(np.uint16),
              rs.randint(0, 1024, (h // 2, w // 2)).astype(np.uint16))
    want = sp.scale_picture(*planes, ow, oh, NONE, col)
    ctx = engine.Context(0)
    pic = ctx.upload_pic(*planes)
    for win in WINDOWS:
        assert pic.output_scaled(ow, oh, NONE, col, win).tobytes() == oo.packed_frame(*want, win), win
        assert pic.digest_scaled(ow, oh, NONE, col, win) == oo.picture_digest(*want, win), win
    # the sizes have been seen: nothing more is allocated, also not for a smaller output (grow-only)
    held = ctx.scratch_bytes()
    assert held >= ow * oh * 3
    assert pic.output_scaled(ow, oh, NONE, col).tobytes() == oo.packed_frame(*want, NONE)
    assert ctx.scratch_bytes() == held
    ident = pic.output_scaled(w, h)                                                    # equal size, empty scaling window: an identity copy
    assert ident.tobytes() == oo.packed_frame(*planes, NONE) and ctx.scratch_bytes() == held
    # the source is only read
    assert all(np.array_equal(a, b) for a, b in zip(pic.download(), planes))
    pic.free(); ctx.close()


def test_frame_outputs_the_resampled_picture_and_publishes_the_decoded_one(built_lib):
    w, h, ow, oh = 416, 240, 832, 480
    col, win = (0, 1), (1, 0, 2, 1)
    wl = synth.make_workload(w, h, 61, tools=synth.INTRA_TOOLS, intra_frac=1.0, calllog=True)
    o = oracle_pipeline.decode(wl)
    dec = (o.y, o.cb, o.cr)
    want = sp.scale_picture(*dec, ow, oh, NONE, col)
    dpb = engine.Dpb((0,))
    ctx = engine.Context(0)
    f = engine.Frame(dpb, 0, w, h)

    keep = _Keep()
    params = engine.Job.make_params(keep, wl)

    def submit(key, out):
        f.begin(key)
        f.recorder().replay(wl.calllog)
        f.submit(params, out=out)

    def packed_out(win, ow, oh):
        out = capi.FrameOutput()
        cwin = capi.Window(*win)
        buf = np.zeros(capi.load().ovhip_output_bytes(ow, oh, C.byref(cwin)) // 2, np.uint16)
        out.mode, out.window, out.packed = capi.OUT_PACKED, cwin, buf.ctypes.data
        return out, buf

    # before: the decoded picture
    out, buf = packed_out(win, w, h)
    submit(0x100, out)
    before = buf.tobytes()
    assert before == oo.packed_frame(*dec, win)
    f.set_output_scale(ow, oh, NONE, col)
    # PACKED
    out, buf = packed_out(win, ow, oh)
    submit(0x200, out)
    assert buf.tobytes() == oo.packed_frame(*want, win)
    # PLANES: the caller's pointers describe planes of the output size
    y, cb, cr = np.zeros((oh, ow), np.uint16), np.zeros((oh // 2, ow // 2), np.uint16), np.zeros((oh // 2, ow // 2), np.uint16)
    out = capi.FrameOutput()
    out.mode, out.y, out.cb, out.cr, out.stride_y, out.stride_c = capi.OUT_PLANES, y.ctypes.data, cb.ctypes.data, cr.ctypes.data, ow, ow // 2
    submit(0x300, out)
    assert np.array_equal(y, want[0]) and np.array_equal(cb, want[1]) and np.array_equal(cr, want[2])
    # DIGEST
    out = capi.FrameOutput()
    out.mode, out.window = capi.OUT_DIGEST, capi.Window(*win)
    submit(0x400, out)
    assert bytes(out.digest) == oo.picture_digest(*want, win)
    # what the DPB holds is the decoded picture at its coded size
    for key in (0x200, 0x300, 0x400):
        _dev, pic = dpb.lookup(key)
        assert (pic.w, pic.h) == (w, h)
        dp = engine.DevPic(ctx, pic, owns=False)
        assert dp.digest() == oo.picture_digest(*dec)
        assert all(np.array_equal(a, b) for a, b in zip(dp.download(), dec))
    # refused factors leave the setting as it was; switched off, the output is what it was before
    assert f.set_output_scale(w // 2, h // 2, check=False) == capi.OVHIP_EUNSUP
    out, buf = packed_out(win, ow, oh)
    submit(0x500, out)
    assert buf.tobytes() == oo.packed_frame(*want, win)
    f.set_output_scale(0, 0)
    out, buf = packed_out(win, w, h)
    submit(0x600, out)
    assert buf.tobytes() == before
    f.close(); ctx.close(); dpb.close()


def test_the_last_band_outputs_the_resampled_picture_too(built_lib):
    """ovhip_frame_band's last call shares the output helper of ovhip_frame_submit: the same picture as ONE band"""
    w, h, ow, oh = 416, 240, 832, 480
    col, win = (1, 1), (0, 2, 1, 0)
    wl = synth.make_workload(w, h, 61, tools=synth.INTRA_TOOLS, intra_frac=1.0, calllog=True)
    o = oracle_pipeline.decode(wl)
    want = sp.scale_picture(o.y, o.cb, o.cr, ow, oh, NONE, col)
    lib = capi.load()
    dpb = engine.Dpb((0,))
    ctx = engine.Context(0)
    f = engine.Frame(dpb, 0, w, h)
    keep = _Keep()
    params = engine.Job.make_params(keep, wl)
    f.begin(0x100)
    f.recorder().replay(wl.calllog)
    assert lib.ovhip_frame_set_band_mode(f.f, 1) == 0
    f.set_output_scale(ow, oh, NONE, col)
    cwin = capi.Window(*win)
    buf = np.zeros(lib.ovhip_output_bytes(ow, oh, C.byref(cwin)) // 2, np.uint16)
    out = capi.FrameOutput()
    out.mode, out.window, out.packed = capi.OUT_PACKED, cwin, buf.ctypes.data
    assert lib.ovhip_frame_band(f.f, C.byref(params), h, 1, C.byref(out)) == 1, lib.ovhip_frame_last_error(f.f)
    assert buf.tobytes() == oo.packed_frame(*want, win)
    _dev, pic = dpb.lookup(0x100)
    assert (pic.w, pic.h) == (w, h) and engine.DevPic(ctx, pic, owns=False).digest() == oo.picture_digest(o.y, o.cb, o.cr)
    f.close(); ctx.close(); dpb.close()


def test_stream_driver_writes_the_file_at_the_output_size(built_lib):
    """OVHIP_OUT_PACKED + OVHIP_STREAM_FILE_MD5 with a 2:1 output scale: the frames of the file are the resampled pictures in output order"""
    w, h, ow, oh = 416, 240, 832, 480
    win, col = (1, 2, 0, 3), (0, 0)
    wls = _contents(w, h, (41, 42), 43)
    pics = gop.build_stream(2, 8, 16, 1)
    spics = _stream_pics(pics, 2)
    planes = _oracle_stream(wls, spics)
    order = sorted(range(len(spics)), key=lambda i: spics[i]["poc"])
    scaled = {i: sp.scale_picture(*planes[i], ow, oh, NONE, col) for i in order}
    today = hashlib.md5(b"".join(oo.packed_frame(*planes[i], win) for i in order)).digest()
    want = hashlib.md5(b"".join(oo.packed_frame(*scaled[i], win) for i in order)).digest()
    lib = capi.load()
    cwin = capi.Window(*win)
    ctx = engine.Context(0)
    dpb = engine.Dpb((0,))
    jobs = _jobs_for(ctx, wls, spics, w, h)
    st = engine.Stream(dpb, w, h, _make_contents(wls), jobs, threads_per_device=4, output=capi.OUT_PACKED, window=win)
    arr = st.pics_array(spics)
    n = len(spics)
    # without the setter: the digest it gives today
    res, _ = st.run(arr, n, 0, n, flags=capi.STREAM_FILE_MD5)
    assert bytes(res.out_md5) == today and res.out_bytes == n * lib.ovhip_output_bytes(w, h, C.byref(cwin))
    assert st.set_output_scale(w // 2, h // 2, check=False) == capi.OVHIP_EUNSUP            # refused before anything runs
    st.set_output_scale(ow, oh, NONE, col)
    res, _ = st.run(arr, n, 0, n, flags=capi.STREAM_FILE_MD5)
    assert res.out_frames == n and res.out_bytes == n * lib.ovhip_output_bytes(ow, oh, C.byref(cwin))
    assert bytes(res.out_md5) == want
    assert dpb.stats().n_live == 0
    st.set_output_scale(0, 0)
    res, _ = st.run(arr, n, 0, n, flags=capi.STREAM_FILE_MD5)
    assert bytes(res.out_md5) == today and res.out_bytes == n * lib.ovhip_output_bytes(w, h, C.byref(cwin))
    st.close()
    # the frame threads' DIGEST path
    st = engine.Stream(dpb, w, h, _make_contents(wls), jobs, threads_per_device=4, output=capi.OUT_DIGEST, window=win)
    st.set_output_scale(ow, oh, NONE, col)
    res, dg = st.run(arr, n, 0, n, digests=True)
    assert bytes(res.out_md5) == hashlib.md5(b"".join(oo.picture_digest(*scaled[i], win) for i in order)).digest()
    for i in range(n):
        assert bytes(dg[i]) == oo.picture_digest(*scaled[i], win), i
    st.close(); [j.close() for j in jobs]; dpb.close(); ctx.close()


def test_refusals_come_back_before_anything_is_launched(built_lib):
    """return values only: nothing is provoked on the device"""
    ctx = engine.Context(0)
    big, small = ctx.new_pic(128, 96), ctx.new_pic(64, 48)
    assert big.scale_into(small, check=False) == capi.OVHIP_EUNSUP
    assert "down-sampling" in ctx.lib.ovhip_last_error(ctx.h).decode()
    mixed = ctx.new_pic(256, 48)                                                       # one axis up, the other down
    assert big.scale_into(mixed, check=False) == capi.OVHIP_EUNSUP
    assert small.scale_into(big, (8, 8, 0, 0), check=False) == capi.OVHIP_EINVAL      # the window leaves nothing: (8 + 8) << 2 = 64
    # aliasing: the picture itself, and a view into it
    assert big.scale_into(big, check=False) == capi.OVHIP_EINVAL
    assert "aliases" in ctx.lib.ovhip_last_error(ctx.h).decode()
    assert big.band(0, 48).scale_into(big, check=False) == capi.OVHIP_EINVAL
    # a missing plane
    s = capi.Pic(small.s.y, small.s.cb, None, small.s.w, small.s.h, small.s.stride_y, small.s.stride_c)
    assert engine.DevPic(ctx, s, owns=False).scale_into(big, check=False) == capi.OVHIP_EINVAL
    # sizes that are not multiples of 4
    odd = ctx.new_pic(130, 98)
    assert small.scale_into(odd, check=False) == capi.OVHIP_EINVAL
    # the conveniences refuse likewise, and allocate nothing for it
    info, out = capi.ScaleInfo(), np.zeros(64 * 48 * 3 // 2, np.uint16)
    held = ctx.scratch_bytes()
    assert ctx.lib.ovhip_pic_output_scaled(ctx.h, C.byref(big.s), C.byref(info), 64, 48, None, out.ctypes.data) == capi.OVHIP_EUNSUP
    dg = (C.c_uint8 * 16)()
    assert ctx.lib.ovhip_pic_digest_scaled(ctx.h, C.byref(big.s), C.byref(info), 64, 48, None, dg) == capi.OVHIP_EUNSUP
    assert ctx.lib.ovhip_pic_output_scaled(ctx.h, C.byref(big.s), C.byref(info), 258, 192, None, out.ctypes.data) == capi.OVHIP_EINVAL
    assert ctx.scratch_bytes() == held
    for p in (big, small, mixed, odd):
        p.free()
    ctx.close()
