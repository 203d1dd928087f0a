"""GPU: all five per-picture outputs of ONE frame for the SAME picture -- RGB, surface, ladder, RGB pyramid, motion field --, a different
colour table on each of the four that take one.  Every destination equals what its output gives alone through its own table, by the
numpy restatements tests/spec_*.py; the next picture of the frame, with no destination set, writes nothing; the tables stay.  This
pins the end of a picture (the order and the envelope of the outputs in ovvc_frame.c's picture_end) and the rule "destinations end with
the picture, tables do not" across all outputs at once.  The definitions are integer only: every comparison is of bytes."""
import numpy as np
import pytest

import spec_ladder_lut as sx
import spec_mvfield as sm
import spec_rgb as sr
import spec_rgb_lut as st
import spec_rgb_pyramid as sp
import spec_surface as ss
import spec_surface_lut as ssl
from openvvc_amd import capi, engine, synth
from test_gpu_ladder import device_buffers
from test_gpu_mvfield import H, W, _Dst, _frame_fixture
from test_gpu_rgb_pyramid import arena_levels, arena_of, assert_arena
from test_ladder_cpu import GUARD, assert_equals_want
from test_mvfield_cpu import workload_lists
from test_rgb_pyramid_cpu import FILL

pytestmark = pytest.mark.gpu
assert FILL == ss.FILL == sm.FILL


def test_five_outputs_of_one_picture_each_through_its_own_table(built_lib):
    # (the fixture takes a B picture [1] and the I picture it refers to [2])
    workloads = (None, synth.make_workload(W, H, 9, tools=synth.INTRA_TOOLS, intra_frac=0.3, calllog=True),
                 synth.make_workload(W, H, 11, tools=synth.INTRA_TOOLS, intra_frac=1.0, calllog=True))
    wl, dpb, ctx, f, _borrowed, submit, close = _frame_fixture(workloads)
    loc, matrix, full_range = 0, 9, 0
    conv = sx.conv_of(loc, 2)
    tables = {"rgb": (st.random_table(17, 255, 61), 255), "surface": (st.random_table(33, 255, 62), 255), "ladder": (st.random_table(17, 1023, 63), 1023),
              "pyramid": (st.random_table(33, 255, 64), 255)}
    luts = {k: engine.RgbLut(ctx, t, p) for k, (t, p) in tables.items()}
    f.set_rgb_lut(luts["rgb"])
    f.set_surface_lut(luts["surface"], engine.surface_conv(*conv))
    f.set_ladder_lut(luts["ladder"], engine.surface_conv(*conv))
    f.set_rgb_pyramid_lut(luts["pyramid"])

    rgb_fmt = engine.rgb_format(matrix, full_range, loc, capi.RGB_U8, capi.RGB_PLANAR)
    surf_fmt = engine.surface_format(capi.SURF_NV12, capi.SURF_DITHER)
    n_rgb, n_surf = 3 * W * H, W * H * 3 // 2
    rungs = [sx.rung(208, 120, sx.NV12, sx.DITHER), sx.rung(104, 60, sx.P010)]
    levels = [sp.level(208, 120, sp.U8, sp.HWC), sp.level(104, 60, sp.F16, sp.CHW)]
    mvf_fmt = engine.mvfield_format(sm.I32, sm.PLANAR, sm.REFINED)

    # the destinations: each holds the sentinel, with guard bytes behind (the ladder's, the pyramid's and the field's helpers put theirs)
    d_rgb, d_surf = ctx.upload(np.full(n_rgb + GUARD, FILL, np.uint8)), ctx.upload(np.full(n_surf + GUARD, FILL, np.uint8))
    lad_bufs, c_rungs = device_buffers(ctx, rungs)
    d_pyr = ctx.upload(np.full(arena_of(levels)[1], FILL, np.uint8))
    d_mvf = _Dst(ctx, W, H, sm.I32)
    everything = [d_rgb, d_surf, d_pyr, d_mvf.vec, d_mvf.info] + lad_bufs

    def set_all():
        f.set_rgb_output(d_rgb.ptr.value, rgb_fmt, nbytes=n_rgb)
        f.set_surface_output(d_surf.ptr.value, surf_fmt, nbytes=n_surf)
        f.set_ladder_output(c_rungs, chroma_loc=loc)
        f.set_rgb_pyramid_output(arena_levels(levels, (matrix, full_range, loc), d_pyr.ptr.value))
        f.set_mvfield_output(mvf_fmt, **d_mvf.args)

    def wipe():
        for b in everything:
            fill = np.full(b.nbytes, FILL, np.uint8)
            assert ctx.lib.ovhip_h2d(ctx.h, b.ptr, fill.ctypes.data, fill.nbytes) == 0
            ctx.sync()

    want = {}

    def check_all(key, what):
        dec = engine.DevPic(ctx, dpb.lookup(key)[1], owns=False).download()
        if not want:                                           # (the restatements once: the same picture is decoded every time)
            want["dec"] = dec
            want["rgb"] = st.convert(*dec, matrix, full_range, loc, sr.U8, sr.PLANAR, *tables["rgb"])
            want["surface"] = ssl.surface(dec, conv, *tables["surface"], ss.NV12, ss.DITHER)[0]
            want["ladder"] = sx.ladder(dec, rungs, conv, *tables["ladder"], guard=GUARD)
            want["pyramid"] = sp.pyramid(dec, levels, matrix, full_range, loc, *tables["pyramid"])
        assert all(np.array_equal(a, b) for a, b in zip(dec, want["dec"])), (what, "the same picture")
        rgb, surf = d_rgb.download(), d_surf.download()
        assert rgb[:n_rgb].tobytes() == np.ascontiguousarray(want["rgb"]).tobytes() and (rgb[n_rgb:] == FILL).all(), (what, "RGB")
        assert surf[:n_surf].tobytes() == want["surface"].tobytes() and (surf[n_surf:] == FILL).all(), (what, "surface")
        assert_equals_want([b.download() for b in lad_bufs], want["ladder"], (what, "ladder"))
        assert_arena(d_pyr.download(), levels, want["pyramid"], (what, "RGB pyramid"))
        d_mvf.check(*sm.field(W, H, workload_lists(wl, f.job().refined_mvs()), sm.I32, sm.PLANAR, sm.REFINED), (what, "motion field"))

    set_all()
    assert submit(0x300) == 0
    check_all(0x300, "five outputs of one picture")
    # each differs from what it is without its table: the tables were used, each its own
    assert want["rgb"].tobytes() != sr.convert(*want["dec"], matrix, full_range, loc, sr.U8, sr.PLANAR).tobytes()
    assert len({t.tobytes()[:4096] for t, _p in tables.values()}) == 4
    # the destinations ended with the picture: the next one, with nothing set, writes nothing anywhere
    wipe()
    assert submit(0x301) == 0
    ctx.sync()
    for b in everything:
        assert (b.download() == FILL).all(), "a picture with no destination set wrote"
    # the tables did not: the same destinations set again give the same bytes
    set_all()
    assert submit(0x302) == 0
    check_all(0x302, "the tables stayed")
    [b.free() for b in [d_rgb, d_surf, d_pyr] + lad_bufs]
    d_mvf.free()
    [x.close() for x in luts.values()]
    close()
