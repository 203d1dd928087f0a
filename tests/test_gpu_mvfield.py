"""GPU: motion field output on the device (openvvc_amd/csrc/kernels_mvfield.hip): ovhip_mvfield_launch against the host twin on the
directed lists and on a recorded picture -- destinations inside sentinel buffers, at offsets 0 and one element, a second launch that
must leave no stale cell --, ovhip_job_mvfield after a flush, a resident replay, a band-wise submission and ovhip_job_begin, the frame
thread (its own job, a borrowed job, a failed picture, beside the RGB and surface outputs) and the stream driver into torch tensors.
The definition is exact: every comparison is of bytes."""
import copy

import numpy as np
import pytest

import spec_mvfield as sm
import spec_rgb as sr
import spec_surface as ss
from openvvc_amd import capi, engine, gop, synth
from test_gpu_stream import _Keep, _contents, _jobs_for, _make_contents, _stream_pics
from test_mvfield_cpu import host_field, test_dry_frame_accepts_the_setter_and_writes_nothing as _dry_frame, workload_lists

pytestmark = pytest.mark.gpu
GUARD = 32                                                    # bytes before and behind a destination that must stay as they were
W, H = 416, 240
COMBOS = [(d, l, v) for d in sm.DTYPES for l in sm.LAYOUTS for v in sm.VECTORS]


@pytest.fixture(scope="module")
def ctx(built_lib):
    c = engine.Context(0)
    yield c
    c.close()


def _upload_lists(ctx, L):
    """the lists of a spec_mvfield.lists() dict as DevBufs (count: units), for Context.mvfield"""
    dev = {k: ctx.upload(L[k]) if len(L[k]) else None for k in ("mc", "mcx", "aff", "rpr", "affr", "side")}
    dev["refined"] = ctx.upload(L["refined"]) if L["refined"] is not None else None
    return dev


def _free(dev):
    [b.free() for b in dev.values() if b is not None]


class _Dst:
    """a pair of device buffers that hold 0xA5: GUARD + lead bytes, the destination, GUARD bytes"""

    def __init__(self, ctx, w, h, dtype, lead=(0, 0), want=(True, True)):
        self.vb, self.ib = sm.sizes(w, h, dtype)
        self.lead, self.want = (GUARD + lead[0], GUARD + lead[1]), want
        self.vec = ctx.upload(np.full(self.lead[0] + self.vb + GUARD, sm.FILL, np.uint8)) if want[0] else None
        self.info = ctx.upload(np.full(self.lead[1] + self.ib + GUARD, sm.FILL, np.uint8)) if want[1] else None

    @property
    def args(self):
        return dict(vec=self.vec.ptr.value + self.lead[0] if self.vec else None, vec_bytes=self.vb,
                    info=self.info.ptr.value + self.lead[1] if self.info else None, info_bytes=self.ib)

    def check(self, want_vec, want_info, what):
        for buf, lead, n, want in ((self.vec, self.lead[0], self.vb, want_vec), (self.info, self.lead[1], self.ib, want_info)):
            if buf is None:
                continue
            raw = buf.download()
            assert (raw[:lead] == sm.FILL).all() and (raw[lead + n:] == sm.FILL).all(), ("guard bytes", what)
            assert raw[lead:lead + n].tobytes() == want.tobytes(), what

    def free(self):
        [b.free() for b in (self.vec, self.info) if b is not None]


def _twin(lib, w, h, L, dtype, layout, vectors):
    vec, info, (vb, ib) = host_field(lib, w, h, L, dtype, layout, vectors)
    return vec[:vb], info[:ib]


def _picture_lists(w, h, seed):
    """the recorder's arrays of a synthetic picture, with refined vectors that differ from the units' own in every DMVR unit"""
    wl = synth.make_workload(w, h, seed)
    ux = wl.mcx_units
    own = np.stack([ux["mv0x"], ux["mv0y"], ux["mv1x"], ux["mv1y"]], axis=1).astype(np.int32)
    return workload_lists(wl, own + np.array([3, -2, -3, 2], np.int32) * (1 + np.arange(len(ux), dtype=np.int32)[:, None] % 7))


@pytest.mark.parametrize("case", ["directed", "136x72"])
def test_launch_equals_the_twin_inside_sentinel_buffers(ctx, case):
    (w, h), L = (sm.DIRECTED_SIZE, sm.directed_lists()) if case == "directed" else ((136, 72), _picture_lists(136, 72, 11))
    assert len(L["mcx"]) and len(L["aff"]) and ((L["mcx"]["flags"] & sm.MC_DMVR) != 0).any()
    dev = _upload_lists(ctx, L)
    for dtype, layout, vectors in COMBOS:
        fmt = engine.mvfield_format(dtype, layout, vectors)
        tv, ti = _twin(ctx.lib, w, h, L, dtype, layout, vectors)
        sv, si = sm.field(w, h, L, dtype, layout, vectors)
        assert tv.tobytes() == sv.tobytes() and ti.tobytes() == si.tobytes()
        for lead, want in (((0, 0), (True, True)), ((sm.ELEM[dtype], 4), (True, True)), ((0, 0), (True, False)), ((sm.ELEM[dtype], 4), (False, True))):
            d = _Dst(ctx, w, h, dtype, lead, want)
            ctx.mvfield(w, h, fmt, **d.args, **dev)
            ctx.sync()
            d.check(tv, ti, (case, dtype, layout, vectors, lead, want))
            d.free()
    _free(dev)


def test_a_second_launch_leaves_no_stale_cell(ctx):
    w, h = sm.DIRECTED_SIZE
    first, second = sm.directed_lists(), sm.other_lists()
    d1, d2 = _upload_lists(ctx, first), _upload_lists(ctx, second)
    for dtype, layout, vectors in COMBOS[::2]:
        fmt = engine.mvfield_format(dtype, layout, sm.UNIT)
        for lead in ((0, 0), (sm.ELEM[dtype], 4)):
            d = _Dst(ctx, w, h, dtype, lead)
            ctx.mvfield(w, h, fmt, **d.args, **d1)
            ctx.mvfield(w, h, fmt, **d.args, **d2)
            ctx.sync()
            tv, ti = _twin(ctx.lib, w, h, second, dtype, layout, sm.UNIT)
            assert int((ti.view(np.uint32) != sm.EMPTY).sum()) == 8
            d.check(tv, ti, (dtype, layout, lead))
            # empty lists: the clear step alone
            ctx.mvfield(w, h, fmt, **d.args)
            ctx.sync()
            d.check(np.zeros(d.vb, np.uint8), np.full(d.ib // 4, sm.EMPTY, np.uint32), ("empty", dtype, layout, lead))
            d.free()
    _free(d1); _free(d2)


def test_launch_refusals_come_back_before_anything_is_launched(ctx):
    """return values and the error text only: nothing is provoked on the device, and the destinations stay as they were"""
    w, h = sm.DIRECTED_SIZE
    L = sm.directed_lists()
    dev = _upload_lists(ctx, L)
    d = _Dst(ctx, w, h, sm.I32)
    a = d.args
    ok = engine.mvfield_format(sm.I32, sm.CELLS, sm.REFINED)
    rsv = engine.mvfield_format()
    rsv.rsv = 1
    no_refined = dict(dev, refined=None)
    cases = [
        ("both destinations", ok, dict(a, vec=None, info=None), dev),
        ("unknown dtype", engine.mvfield_format(3), a, dev), ("unknown layout", engine.mvfield_format(0, 2), a, dev),
        ("unknown vectors", engine.mvfield_format(0, 0, 2), a, dev), ("rsv", rsv, a, dev),
        ("not aligned", ok, dict(a, vec=a["vec"] + 2), dev), ("not aligned", ok, dict(a, info=a["info"] + 1), dev),
        ("too small", ok, dict(a, vec_bytes=d.vb - 4), dev), ("too small", ok, dict(a, info_bytes=d.ib - 1), dev),
        ("overlap", ok, dict(a, info=a["vec"] + d.vb - 4), dev),
        ("refined", ok, a, no_refined),
    ]
    for text, fmt, args, lists in cases:
        assert ctx.mvfield(w, h, fmt, check=False, **args, **lists) == capi.OVHIP_EINVAL, text
        assert text in ctx.lib.ovhip_last_error(ctx.h).decode(), (text, ctx.lib.ovhip_last_error(ctx.h))
    assert ctx.mvfield(w, h, ok, check=False, **dict(a, vec_bytes=d.vb - 4), **dev) == capi.OVHIP_EINVAL
    msg = ctx.lib.ovhip_last_error(ctx.h).decode()
    assert "too small" in msg and str(d.vb - 4) in msg and str(d.vb) in msg, msg
    for ww, hh in ((0, h), (w, -4), (16388, h)):
        assert ctx.mvfield(ww, hh, ok, check=False, **dict(a, vec_bytes=1 << 40, info_bytes=1 << 40), **dev) == capi.OVHIP_EINVAL
        assert "sizes must be" in ctx.lib.ovhip_last_error(ctx.h).decode()
    assert ctx.mvfield(w, h, None, check=False, **a, **dev) == capi.OVHIP_EINVAL
    assert ctx.lib.ovhip_mvfield_launch(None, w, h, None, None, None, 0, None, 0) == capi.OVHIP_EINVAL
    ctx.sync()
    d.check(np.full(d.vb, sm.FILL, np.uint8), np.full(d.ib, sm.FILL, np.uint8), "refusals write nothing")
    d.free(); _free(dev)


def test_python_layer_checks_the_tensors(built_lib):
    import torch
    fmt = engine.mvfield_format(capi.MVF_F16, capi.MVF_CELLS)
    vec = torch.zeros((10, 18, 4), dtype=torch.float16, device="cuda:0")
    info = torch.zeros((10, 18), dtype=torch.int32, device="cuda:0")
    assert engine._mvfield_dsts(vec, info, fmt, 72, 40, None, None) == (vec.data_ptr(), 1440, info.data_ptr(), 720, 1)
    assert engine._mvfield_dsts(None, info, fmt, 72, 40, None, None) == (0, 0, info.data_ptr(), 720, 1)
    slots = torch.zeros((3, 10, 18, 4), dtype=torch.float16, device="cuda:0")
    assert engine._mvfield_dsts(slots, None, fmt, 72, 40, None, None, slots=True) == (slots.data_ptr(), 1440, 0, 0, 3)
    for bad_vec, bad_info, sl in ((torch.zeros((10, 18, 4), dtype=torch.float32, device="cuda:0"), None, False),
                                  (torch.zeros((4, 10, 18), dtype=torch.float16, device="cuda:0"), None, False),
                                  (torch.zeros((10, 18, 4), dtype=torch.float16), None, False),
                                  (None, torch.zeros((10, 18), dtype=torch.float32, device="cuda:0"), False),
                                  (None, torch.zeros((10, 36), dtype=torch.int32, device="cuda:0")[:, ::2], False),
                                  (slots, torch.zeros((2, 10, 18), dtype=torch.int32, device="cuda:0"), True),
                                  (vec, None, True), (np.zeros((10, 18, 4), np.float16), None, False)):
        with pytest.raises(engine.EngineError):
            engine._mvfield_dsts(bad_vec, bad_info, fmt, 72, 40, None, None, slots=sl)


# ---- the picture job ----
@pytest.fixture(scope="module")
def workloads():
    """the two 416x240 pictures of tests/test_mvfield_cpu.py and an I picture (made once, shared, left unchanged)"""
    return (synth.make_workload(W, H, 3, tools=synth.ALL_TOOLS), synth.make_workload(W, H, 9, tools=synth.INTRA_TOOLS, intra_frac=0.3, calllog=True),
            synth.make_workload(W, H, 11, tools=synth.INTRA_TOOLS, intra_frac=1.0, calllog=True))


def _job_with(ctx, wl):
    job = engine.Job(ctx, wl.w, wl.h)
    refs = [ctx.upload_pic(*r) for r in wl.refs]
    intra = ctx.upload_pic(*wl.intra) if wl.intra is not None else None
    dst = ctx.new_pic(wl.w, wl.h)
    job.load_workload(wl)
    return job, refs, intra, dst


def _check_job_field(ctx, job, L, combos, what):
    for dtype, layout, vectors in combos:
        d = _Dst(ctx, job.w, job.h, dtype)
        job.mvfield(engine.mvfield_format(dtype, layout, vectors), **d.args)
        ctx.sync()
        sv, si = sm.field(job.w, job.h, L, dtype, layout, vectors)
        d.check(sv, si, (what, dtype, layout, vectors))
        d.free()


@pytest.mark.parametrize("which", [0, 1])
def test_job_mvfield_after_a_flush_and_after_a_resident_replay(ctx, workloads, which):
    wl = workloads[which]
    job, refs, intra, dst = _job_with(ctx, wl)
    # before any flush: refused
    d = _Dst(ctx, W, H, sm.I32)
    assert job.mvfield(engine.mvfield_format(), check=False, **d.args) == capi.OVHIP_EINVAL
    job.flush(dst, refs, intra); job.wait()
    L = workload_lists(wl, job.refined_mvs())
    is_dmvr = (L["mcx"]["flags"] & sm.MC_DMVR) != 0
    own = np.stack([L["mcx"][k] for k in ("mv0x", "mv0y", "mv1x", "mv1y")], axis=1)
    assert int((L["refined"][is_dmvr] != own[is_dmvr]).any(axis=1).sum()) >= 10
    before = dst.digest()
    _check_job_field(ctx, job, L, COMBOS, "flush")
    assert dst.digest() == before, "the decoded picture is only read"
    # a second, resident flush of the same job: the device copies of the first
    job.flush(dst, refs, intra, params=job.make_params(wl, stages=capi.STAGE_ALL | capi.STAGE_RESIDENT)); job.wait()
    assert dst.digest() == before
    _check_job_field(ctx, job, L, [(sm.I32, sm.CELLS, sm.REFINED), (sm.F16, sm.PLANAR, sm.UNIT), (sm.F32, sm.CELLS, sm.REFINED)], "resident replay")
    assert dst.digest() == before
    # the refusals of the launch come through, and write nothing
    assert job.mvfield(engine.mvfield_format(), check=False, **dict(d.args, vec_bytes=d.vb - 1)) == capi.OVHIP_EINVAL
    assert "too small" in ctx.lib.ovhip_last_error(ctx.h).decode()
    # after ovhip_job_begin the arrays are the next picture's: refused
    job.begin()
    assert job.mvfield(engine.mvfield_format(), check=False, **d.args) == capi.OVHIP_EINVAL
    ctx.sync()
    d.check(np.full(d.vb, sm.FILL, np.uint8), np.full(d.ib, sm.FILL, np.uint8), "refused calls write nothing")
    d.free(); job.close()
    [p.free() for p in refs + [dst] + ([intra] if intra else [])]


def test_job_mvfield_is_unsupported_after_a_band_wise_submission(ctx, workloads):
    # (a band is a slice of the lists in decoding order: the transform blocks sorted back into it, as tests/test_gpu_bands.py does)
    wl = copy.copy(workloads[1])
    tb = np.asarray(wl.tb_cmds).view(capi.TB_CMD_DTYPE).reshape(-1)
    wl.tb_cmds = np.ascontiguousarray(tb[np.argsort(tb["coef_off"], kind="stable")])
    job, refs, intra, dst = _job_with(ctx, wl)
    job.flush_in_bands(wl, dst, refs); job.wait()
    d = _Dst(ctx, W, H, sm.I32)
    assert job.mvfield(engine.mvfield_format(), check=False, **d.args) == capi.OVHIP_EUNSUP
    assert "band" in ctx.lib.ovhip_last_error(ctx.h).decode()
    ctx.sync()
    d.check(np.full(d.vb, sm.FILL, np.uint8), np.full(d.ib, sm.FILL, np.uint8), "refused calls write nothing")
    # the next whole-picture flush of the same job gives the field again
    job.load_workload(wl)
    job.flush(dst, refs, intra); job.wait()
    _check_job_field(ctx, job, workload_lists(wl, job.refined_mvs()), [(sm.I32, sm.PLANAR, sm.REFINED)], "flush after bands")
    d.free(); job.close()
    [p.free() for p in refs + [dst]]


def test_an_i_picture_gives_an_all_empty_field(ctx, workloads):
    wl = workloads[2]
    job, refs, intra, dst = _job_with(ctx, wl)
    job.flush(dst, refs, intra); job.wait()
    d = _Dst(ctx, W, H, sm.F32)
    job.mvfield(engine.mvfield_format(sm.F32, sm.CELLS, sm.REFINED), **d.args)
    ctx.sync()
    d.check(np.zeros(d.vb, np.uint8), np.full(d.ib // 4, sm.EMPTY, np.uint32), "I picture")
    d.free(); job.close()
    [p.free() for p in refs + [dst]]


# ---- the frame thread ----
def _frame_fixture(workloads):
    """an I picture under KEY_I and the means to decode the B picture of workloads[1] from it, with the frame's own job or a borrowed one"""
    wl_i, wl_b = workloads[2], workloads[1]
    dpb = engine.Dpb((0,))
    ctx = engine.Context(0)
    fi, f = engine.Frame(dpb, 0, W, H), engine.Frame(dpb, 0, W, H)
    keep = _Keep()
    KEY_I = 0xA000
    fi.begin(KEY_I)
    fi.recorder().replay(wl_i.calllog)
    fi.submit(engine.Job.make_params(keep, wl_i))
    params = engine.Job.make_params(keep, wl_b)
    borrowed = engine.Job(ctx, W, H)

    def submit(key, borrow=False, out=None, check=True):
        f.begin(key)
        assert f.ref(KEY_I) == 0 and f.ref_at(1, KEY_I) == 1
        if borrow:
            borrowed.load_workload(wl_b)
        else:
            f.recorder().replay(wl_b.calllog)
        return f.submit(params, job=borrowed if borrow else None, out=out, check=check)

    def close():
        borrowed.close(); fi.close(); f.close(); ctx.close(); dpb.close()

    return wl_b, dpb, ctx, f, borrowed, submit, close


def _a5(ctx, nbytes):
    return ctx.upload(np.full(nbytes, sm.FILL, np.uint8))


def test_frame_writes_the_field_of_the_picture_it_completes(built_lib, workloads):
    import torch
    wl, dpb, ctx, f, borrowed, submit, close = _frame_fixture(workloads)
    fmt = engine.mvfield_format(capi.MVF_F16, capi.MVF_CELLS, capi.MVF_REFINED)
    vshape, ishape = engine.mvfield_shape(fmt, W, H)
    for borrow in (False, True):
        vec = torch.full(vshape, 7, dtype=torch.float16, device="cuda:0")
        info = torch.full(ishape, 7, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        f.set_mvfield_output(fmt, vec, info)
        assert submit(0x100 + borrow, borrow) == 0
        job = borrowed if borrow else f.job()
        sv, si = sm.field(W, H, workload_lists(wl, job.refined_mvs()), sm.F16, sm.CELLS, sm.REFINED)
        assert vec.cpu().numpy().tobytes() == sv.tobytes() and info.cpu().numpy().tobytes() == si.tobytes(), borrow
        assert (si != sm.EMPTY).sum() > 2000 and ((si >> 16) & sm.DMVR).any()
        # the setting is gone for the next picture: its submit leaves the sentinel in place
        vec.fill_(7); info.fill_(7)
        torch.cuda.synchronize()
        assert submit(0x110 + borrow, borrow) == 0
        assert (vec.cpu().numpy() == 7).all() and (info.cpu().numpy() == 7).all()
    # raw addresses, the info alone; switched off again before the picture: untouched
    d = _Dst(ctx, W, H, sm.I32, want=(False, True))
    f.set_mvfield_output(engine.mvfield_format(), **d.args)
    assert submit(0x120) == 0
    d.check(None, sm.field(W, H, workload_lists(wl), sm.I32)[1], "info alone")
    d2 = _Dst(ctx, W, H, sm.I32)
    f.set_mvfield_output(engine.mvfield_format(), **d2.args)
    f.set_mvfield_output(None)
    assert submit(0x121) == 0
    # a picture failed with Frame.fail leaves the destinations untouched, and takes the setting with it
    f.set_mvfield_output(engine.mvfield_format(), **d2.args)
    f.begin(0x122)
    f.fail(capi.OVHIP_EUNSUP)
    assert submit(0x123) == 0
    # the setter's own refusals; a refused setting is no setting
    a = d2.args
    rsv = engine.mvfield_format()
    rsv.rsv = 1
    for bad, args in ((engine.mvfield_format(3), a), (engine.mvfield_format(0, 2), a), (engine.mvfield_format(0, 0, 2), a), (rsv, a),
                      (engine.mvfield_format(), dict(a, vec=None, info=None)), (engine.mvfield_format(), dict(a, vec=a["vec"] + 2)),
                      (engine.mvfield_format(), dict(a, info=a["vec"] + 16))):
        assert f.set_mvfield_output(bad, check=False, **args) == capi.OVHIP_EINVAL
    assert submit(0x124) == 0
    # a destination that is too small fails the call, not the publication
    f.set_mvfield_output(engine.mvfield_format(), **dict(a, vec_bytes=d2.vb - 4))
    assert submit(0x125, check=False) == capi.OVHIP_EINVAL
    assert b"too small" in built_lib.ovhip_frame_last_error(f.f)
    assert dpb.lookup(0x125)[1].w == W
    # a frame in band mode refuses the setter
    assert built_lib.ovhip_frame_set_band_mode(f.f, 1) == 0
    assert f.set_mvfield_output(engine.mvfield_format(), check=False, **a) == capi.OVHIP_EUNSUP
    assert built_lib.ovhip_frame_set_band_mode(f.f, 0) == 0
    ctx.sync()
    d2.check(np.full(d2.vb, sm.FILL, np.uint8), np.full(d2.ib, sm.FILL, np.uint8), "none of these wrote")
    _dry_frame(built_lib)
    d.free(); d2.free(); close()


def test_frame_rgb_and_surface_outputs_are_what_they_are_without_the_field(built_lib, workloads):
    wl, dpb, ctx, f, borrowed, submit, close = _frame_fixture(workloads)
    rgb_fmt = engine.rgb_format(1, 0, 0, capi.RGB_U8, capi.RGB_PLANAR)
    surf_fmt = engine.surface_format(capi.SURF_NV12)
    n_rgb, n_surf = 3 * W * H, W * H * 3 // 2
    got = []
    for with_field in (False, True):
        d_rgb, d_surf, d = _a5(ctx, n_rgb + GUARD), _a5(ctx, n_surf + GUARD), _Dst(ctx, W, H, sm.I32)
        f.set_rgb_output(d_rgb.ptr.value, rgb_fmt, nbytes=n_rgb)
        f.set_surface_output(d_surf.ptr.value, surf_fmt, nbytes=n_surf)
        if with_field:
            f.set_mvfield_output(engine.mvfield_format(sm.I32, sm.PLANAR, sm.REFINED), **d.args)
        assert submit(0x200 + with_field, borrow=with_field) == 0
        got.append((d_rgb.download().tobytes(), d_surf.download().tobytes()))
        if with_field:
            d.check(*sm.field(W, H, workload_lists(wl, borrowed.refined_mvs()), sm.I32, sm.PLANAR, sm.REFINED), "beside RGB and surface")
        else:
            d.check(np.full(d.vb, sm.FILL, np.uint8), np.full(d.ib, sm.FILL, np.uint8), "off")
        dec = engine.DevPic(ctx, dpb.lookup(0x200 + with_field)[1], owns=False).download()
        assert got[-1][0][:n_rgb] == sr.convert(*dec, 1, 0, 0, sr.U8, sr.PLANAR).tobytes()
        assert got[-1][1][:n_surf] == ss.surface(dec, ss.NV12)[0].tobytes()
        d_rgb.free(); d_surf.free(); d.free()
    assert got[0] == got[1]
    close()


# ---- the stream driver ----
def test_stream_writes_every_pictures_field_into_its_slot(built_lib):
    import torch
    wls = _contents(W, H, (41, 42), 43)
    spics = _stream_pics(gop.build_stream(1, 4, 4, 1), 2)                               # I and one GOP of 4
    n = len(spics)
    ctx = engine.Context(0)
    dpb = engine.Dpb((0,))
    jobs = _jobs_for(ctx, wls, spics, W, H)
    st = engine.Stream(dpb, W, H, _make_contents(wls), jobs, threads_per_device=4)
    arr = st.pics_array(spics)

    def own(wl):
        ux = wl.mcx_units
        return np.stack([ux["mv0x"], ux["mv0y"], ux["mv1x"], ux["mv1y"]], axis=1).astype(np.int32) if len(ux) else None

    assert n > 2 and len({p["content"] for p in spics}) == 3
    for vectors in sm.VECTORS:
        fmt = engine.mvfield_format(capi.MVF_I32, capi.MVF_CELLS, vectors)
        vshape, ishape = engine.mvfield_shape(fmt, W, H)
        vec = torch.full((2,) + vshape, 7, dtype=torch.int32, device="cuda:0")
        info = torch.full((2,) + ishape, 7, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        st.set_mvfield_output(fmt, vec, info)
        # n_slots = 2 < n: picture idx lands in slot idx % 2.  One run per pair of pictures, so that no two pictures in flight share a slot
        for first, cnt in ((0, 2), (2, 2), (4, 1)):
            res, _ = st.run(arr, n, first, cnt, flags=capi.STREAM_KEEP)
            assert res.status == 0 and res.n_decoded == cnt
            gv, gi = vec.cpu().numpy(), info.cpu().numpy().view(np.uint32)
            last = first + cnt - 1
            for slot in range(2):
                idx = last if last % 2 == slot else last - 1
                wl = wls[spics[idx]["content"]]
                sv, si = sm.field(W, H, workload_lists(wl, own(wl)), sm.I32, sm.CELLS, vectors)
                assert np.array_equal(gi[slot], si), (vectors, first, slot)
                keep = np.ones(si.shape, bool) if vectors == sm.UNIT else ((si >> 16) & sm.DMVR) == 0
                assert np.array_equal(gv[slot][keep], sv[keep]), (vectors, first, slot)
    # refused at the setter: buffers too small, no slots, both bases NULL, a bad format, tensors of another shape
    vb, ib = sm.sizes(W, H, sm.I32)
    ok = engine.mvfield_format()
    p, q = vec.data_ptr(), info.data_ptr()
    assert st.set_mvfield_output(ok, p, q, vb - 4, ib, 2, check=False) == capi.OVHIP_EINVAL
    assert st.set_mvfield_output(ok, p, q, vb, ib - 4, 2, check=False) == capi.OVHIP_EINVAL
    assert st.set_mvfield_output(ok, p, q, vb, ib, 0, check=False) == capi.OVHIP_EINVAL
    assert st.set_mvfield_output(ok, None, None, vb, ib, 2, check=False) == capi.OVHIP_EINVAL
    assert st.set_mvfield_output(engine.mvfield_format(3), p, q, vb, ib, 2, check=False) == capi.OVHIP_EINVAL
    assert st.set_mvfield_output(ok, p, None, vb, 0, 2, check=False) == 0                                  # (the vectors alone)
    with pytest.raises(engine.EngineError):
        st.set_mvfield_output(ok, vec[:, :-1].contiguous(), info)
    # off again: the tensors stay as they are
    st.set_mvfield_output(None)
    vec.fill_(7); info.fill_(7)
    torch.cuda.synchronize()
    res, _ = st.run(arr, n, 0, n)
    assert res.status == 0 and (vec == 7).all().item() and (info == 7).all().item()
    assert dpb.stats().n_live == 0
    st.close(); [j.close() for j in jobs]; dpb.close(); ctx.close()
