"""GPU: the decoded picture hash SEI on the device (k_pic_hash / k_pic_hash_rows, openvvc_amd/csrc/kernels_pichash.hip) and the
layers above it: the launch and the synchronous convenience against ovhip_pic_hash_host and the restatement tests/spec_pic_hash.py
(which tests/test_pic_hash_cpu.py holds to the vector table), the frame thread and the stream driver against the host hash of the
pictures they publish.  Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import oracle_pipeline
import spec_film_grain as sf
import spec_pic_hash as sp
from openvvc_amd import capi, engine, gop, synth
from test_film_grain_cpu import c_params
from test_gpu_film_grain import _packed_out, oo
from test_gpu_stream import _Keep, _contents, _jobs_for, _make_contents, _stream_pics
from test_pic_hash_cpu import METHODS, host_hash, random_picture

pytestmark = pytest.mark.gpu

# the five sizes of the CPU tests, 136x72 (rows that end inside a wave's span; chroma rows that are not 16-byte aligned) and 264x136:
# a plane narrower than one load, a row tail, more than one wave per row, more than one workgroup, coordinates of 256 and above
SIZES = [(8, 8), (24, 8), (72, 40), (520, 264), (8, 520), (136, 72), (264, 136)]


@pytest.fixture(scope="module")
def ctx(built_lib):
    c = engine.Context(0)
    yield c
    c.close()


def _launch_values(ctx, pic, method, n_planes):
    """ovhip_pic_hash_launch into device words -> the values' bytes as the SEI holds them"""
    d = ctx.alloc(12)
    pic.hash_launch(method, n_planes, d)
    ctx.sync()
    words = d.download(np.uint32)
    d.free()
    return [int(words[c]).to_bytes(4, "big")[4 - sp.VALUE_BYTES[method]:] for c in range(n_planes)]


@pytest.mark.parametrize("w,h", SIZES)
def test_device_equals_host_and_restatement(ctx, w, h):
    lib = ctx.lib
    for planes in (sp.formula_picture(w, h), random_picture(w, h, 7 * w + h)):
        pic = ctx.upload_pic(*planes)
        for method in METHODS:
            for n_planes in (3, 1):
                want = sp.picture_hash(method, planes, n_planes)
                host = host_hash(lib, method, planes, n_planes)
                assert host.planes() == want
                got = pic.hash(method, n_planes)
                assert got.planes() == want, (w, h, method, n_planes, [v.hex() for v in got.planes()], [v.hex() for v in want])
                assert lib.ovhip_pic_hash_equal(C.byref(got), C.byref(host)) == 1
                assert bytes(got) == bytes(host)                       # the zero bytes and the zero rows of absent planes too
                if method != sp.MD5:
                    assert _launch_values(ctx, pic, method, n_planes) == want, (w, h, method, n_planes)
        assert all(np.array_equal(a, b) for a, b in zip(pic.download(), planes)), "the picture is only read"
        pic.free()


def test_a_view_with_a_stride_above_its_width(ctx):
    """the left 72 columns of a 136x72 picture as a picture of its own: luma rows 16-byte aligned with a stride above the width,
    chroma rows (stride 68) not aligned"""
    planes = random_picture(136, 72, 3)
    pic = ctx.upload_pic(*planes)
    s = capi.Pic(pic.s.y, pic.s.cb, pic.s.cr, 72, 72, pic.s.stride_y, pic.s.stride_c)
    view = engine.DevPic(ctx, s, owns=False)
    part = (planes[0][:, :72], planes[1][:, :36], planes[2][:, :36])
    for method in METHODS:
        assert view.hash(method).planes() == sp.picture_hash(method, part), method
    pic.free()


def test_crc_is_deterministic_over_20_launches(ctx):
    planes = random_picture(264, 136, 20)
    pic = ctx.upload_pic(*planes)
    d = ctx.alloc(20 * 12)
    for i in range(20):
        pic.hash_launch(sp.CRC, 3, d, offset=12 * i)
    ctx.sync()
    words = d.download(np.uint32).reshape(20, 3)
    want = [int.from_bytes(v, "big") for v in sp.picture_hash(sp.CRC, planes)]
    for i in range(20):
        assert words[i].tolist() == want, i
    d.free(); pic.free()


def test_one_sample_is_told_apart_in_the_right_plane(ctx):
    w, h = 264, 136
    planes = random_picture(w, h, 99)
    base = ctx.upload_pic(*planes)
    base_v = {m: base.hash(m).planes() for m in METHODS}
    # the last sample of a row, the first of the next row, the last of a plane
    cases = [(0, 5, w - 1), (0, 6, 0), (0, h - 1, w - 1), (1, 9, w // 2 - 1), (1, 10, 0), (2, h // 2 - 1, w // 2 - 1)]
    for c, y, x in cases:
        changed = [p.copy() for p in planes]
        changed[c][y, x] ^= 0x0100                                      # ONE bit: the checksum is a sum, two bits can cancel
        pic = ctx.upload_pic(*changed)
        for m in METHODS:
            got = pic.hash(m).planes()
            assert got == sp.picture_hash(m, changed), (c, y, x, m)
            for k in range(3):
                assert (got[k] != base_v[m][k]) == (k == c), (c, y, x, m, k)
        pic.free()
    base.free()


def test_scratch_is_grow_only(built_lib):
    ctx = engine.Context(0)
    pics = [ctx.upload_pic(*random_picture(w, h, 1)) for w, h in ((264, 136), (72, 40))]
    first = [[p.hash(m).planes() for m in METHODS] for p in pics]             # the larger size first: every buffer at its final size
    held = ctx.scratch_bytes()
    assert held >= 264 * 136 * 3 + 2 * 136 * 4                                 # the MD5 route's planes and the CRC's row remainders
    for rep in range(2):
        for p, want in zip(pics, first):
            assert [p.hash(m).planes() for m in METHODS] == want
            assert ctx.scratch_bytes() == held
    [p.free() for p in pics]
    ctx.close()


def test_refusals_come_back_before_anything_is_launched(ctx):
    """return values only: nothing is provoked on the device"""
    pic = ctx.new_pic(72, 40)
    d = ctx.alloc(12)
    held = ctx.scratch_bytes()
    assert pic.hash_launch(sp.MD5, 3, d, check=False) == capi.OVHIP_EINVAL              # not a device method
    assert pic.hash_launch(sp.CRC, 2, d, check=False) == capi.OVHIP_EINVAL
    assert pic.hash_launch(3, 3, d, check=False) == capi.OVHIP_EINVAL
    assert pic.hash_launch(sp.CRC, 3, None, check=False) == capi.OVHIP_EINVAL
    s = capi.Pic(pic.s.y, None, pic.s.cr, pic.s.w, pic.s.h, pic.s.stride_y, pic.s.stride_c)      # a missing chroma plane
    lame = engine.DevPic(ctx, s, owns=False)
    for m in (sp.CRC, sp.CHECKSUM):
        assert lame.hash_launch(m, 3, d, check=False) == capi.OVHIP_EINVAL
        assert lame.hash(m, 3, check=False) == capi.OVHIP_EINVAL
    assert lame.hash(sp.MD5, 3, check=False) == capi.OVHIP_EINVAL
    assert lame.hash(sp.CRC, 1).planes() == pic.hash(sp.CRC, 1).planes()                # one plane: chroma is not looked at
    s = capi.Pic(pic.s.y, pic.s.cb, pic.s.cr, 72, 40, 70, 36)                           # a stride below the width
    assert engine.DevPic(ctx, s, owns=False).hash(sp.CHECKSUM, 3, check=False) == capi.OVHIP_EINVAL
    assert pic.hash(sp.CRC, 2, check=False) == capi.OVHIP_EINVAL
    assert ctx.scratch_bytes() - held <= 32 + 40 * 4                                     # (the one valid call's words and rows)
    d.free(); pic.free()


def _frame_case():
    """the smallest recorded picture the frame tests use"""
    w, h = 64, 48
    wl = synth.make_workload(w, h, 77, tools=synth.INTRA_TOOLS, intra_frac=1.0, calllog=True)
    o = oracle_pipeline.decode(wl)
    return w, h, wl, (o.y, o.cb, o.cr)


def test_frame_verdict_and_the_picture_is_published_either_way(built_lib):
    w, h, wl, dec = _frame_case()
    dpb = engine.Dpb((0,))
    ctx = engine.Context(0)
    f = engine.Frame(dpb, 0, w, h)
    params = engine.Job.make_params(_Keep(), wl)

    def submit(key, out=None):
        f.begin(key)
        f.recorder().replay(wl.calllog)
        return f.submit(params, out=out)

    def published(key):
        return engine.DevPic(ctx, dpb.lookup(key)[1], owns=False).download()

    assert f.picture_hash()[0] == capi.OVHIP_EINVAL                                      # nothing computed yet
    submit(0x100)
    assert f.picture_hash()[0] == capi.OVHIP_EINVAL                                      # off is the default
    key = 0x200
    for method in METHODS:
        for n_planes in (3, 1):
            want = host_hash(built_lib, method, dec, n_planes)
            # compute only
            f.set_picture_hash(method, n_planes)
            assert submit(key) == 0
            verdict, got = f.picture_hash()
            assert verdict == 1 and bytes(got) == bytes(want)
            # the right expectation
            f.set_picture_hash(method, n_planes, want)
            assert submit(key + 1) == 0
            verdict, got = f.picture_hash()
            assert verdict == 1 and bytes(got) == bytes(want)
            # one byte changed: the verdict is 0, the picture is still published as decoded
            wrong = capi.PicHashValue.from_buffer_copy(bytes(want))
            wrong.value[n_planes - 1][sp.VALUE_BYTES[method] - 1] ^= 0x40
            f.set_picture_hash(method, n_planes, wrong)
            assert submit(key + 2) == 0
            verdict, got = f.picture_hash()
            assert verdict == 0 and bytes(got) == bytes(want)
            for k in range(3):
                assert all(np.array_equal(a, b) for a, b in zip(published(key + k), dec))
            key += 0x10
    # the last band of a band-wise picture takes the hash too
    f.set_picture_hash(sp.CRC, 3, host_hash(built_lib, sp.CRC, dec))
    f.begin(0x900)
    f.recorder().replay(wl.calllog)
    assert built_lib.ovhip_frame_set_band_mode(f.f, 1) == 0
    assert built_lib.ovhip_frame_band(f.f, C.byref(params), h, 1, None) == 1, built_lib.ovhip_frame_last_error(f.f)
    verdict, got = f.picture_hash()
    assert verdict == 1 and got.planes() == sp.picture_hash(sp.CRC, dec)
    assert built_lib.ovhip_frame_set_band_mode(f.f, 0) == 0
    # switched off: nothing is computed for the next picture
    f.set_picture_hash(-1)
    submit(0xa00)
    assert f.picture_hash()[0] == capi.OVHIP_EINVAL
    f.close(); ctx.close(); dpb.close()


def test_frame_hashes_the_decoded_picture_whatever_leaves(built_lib):
    """film grain and a PACKED output: the packed frame is the grained one, the hash is of the picture the DPB holds"""
    w, h, wl, dec = _frame_case()
    win, poc = (1, 0, 0, 1), 9
    sei = sf.make_sei()
    dpb = engine.Dpb((0,))
    ctx = engine.Context(0)
    f = engine.Frame(dpb, 0, w, h)
    params = engine.Job.make_params(_Keep(), wl)
    f.set_film_grain(c_params(sei), poc)
    for method in METHODS:
        f.set_picture_hash(method, 3)
        out, buf = _packed_out(win, w, h)
        f.begin(0x100 + method)
        f.recorder().replay(wl.calllog)
        f.submit(params, out=out)
        grained = sf.apply(dec, sei, poc)[0]
        assert buf.tobytes() == oo.packed_frame(*grained, win) != oo.packed_frame(*dec, win)
        held = engine.DevPic(ctx, dpb.lookup(0x100 + method)[1], owns=False).download()
        verdict, got = f.picture_hash()
        assert verdict == 1 and bytes(got) == bytes(host_hash(built_lib, method, held))
        assert got.planes() == sp.picture_hash(method, dec) != sp.picture_hash(method, grained)
    f.close(); ctx.close(); dpb.close()


def test_stream_hashes_every_picture_on_its_own_frame_thread(built_lib):
    w, h = 416, 240
    wls = _contents(w, h, (41, 42), 43)
    spics = _stream_pics(gop.build_stream(1, 4, 4, 1), 2)                               # I and one GOP of 4
    n = len(spics)
    ctx = engine.Context(0)
    dpb = engine.Dpb((0,))
    jobs = _jobs_for(ctx, wls, spics, w, h)
    st = engine.Stream(dpb, w, h, _make_contents(wls), jobs, threads_per_device=4)
    arr = st.pics_array(spics)
    flags = capi.STREAM_KEEP | capi.STREAM_HOLD_ALL
    assert st.picture_hashes(n)[0] == capi.OVHIP_EINVAL                                 # no run has computed any
    assert st.set_picture_hashes(3, 3, check=False) == capi.OVHIP_EINVAL
    want = {}
    for method in (sp.CRC, sp.CHECKSUM, sp.MD5):
        # compute only
        st.set_picture_hashes(method, 3)
        res, _ = st.run(arr, n, 0, n, flags=flags)
        assert res.status == 0 and res.n_decoded == n
        r, got, n_mis, first_mis = st.picture_hashes(n)
        assert (r, n_mis, first_mis) == (0, 0, -1)
        held = [st.picture(i, ctx).download() for i in range(n)]
        want[method] = [host_hash(built_lib, method, held[i]) for i in range(n)]
        for i in range(n):
            assert bytes(got[i]) == bytes(want[method][i]), (method, i)
        assert len({bytes(v) for v in got}) > 1                                         # (the pictures differ)
        # the right expectations, then one of them corrupted
        exp = (capi.PicHashValue * n)(*[capi.PicHashValue.from_buffer_copy(bytes(v)) for v in want[method]])
        st.set_picture_hashes(method, 3, exp)
        res, _ = st.run(arr, n, 0, n, flags=flags)
        assert res.status == 0 and st.picture_hashes(n)[2:] == (0, -1)
        exp[3].value[1][0] ^= 1
        res, _ = st.run(arr, n, 0, n, flags=flags)
        r, got, n_mis, first_mis = st.picture_hashes(n)
        assert res.status == 0 and res.n_decoded == n and (r, n_mis, first_mis) == (0, 1, 3)
        for i in range(n):
            assert bytes(got[i]) == bytes(want[method][i])
    # off again
    st.set_picture_hashes(-1)
    res, _ = st.run(arr, n, 0, n)
    assert res.status == 0 and st.picture_hashes(n)[0] == capi.OVHIP_EINVAL
    assert dpb.stats().n_live == 0
    st.close(); [j.close() for j in jobs]; dpb.close(); ctx.close()
