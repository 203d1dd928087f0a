"""GPU: the four places where a kernel's result depends on the CTU size, at CTU 64 and 32 (every other GPU test runs 128):
k_sao (a 64x32 tile covers several CTUs: per-lane parameters, CTU-local border rows), k_alf (virtual boundary at CTU row ctu - 4
inside the tiles), CCLM's first-line rule and k_intra_ctu's tile in the ordered pass, k_tmvp_cells' cell index.  SAO and ALF against
the reference's own slots run at those sizes (tests/golden/{sao,alf}_ctu{64,32}.ovg; test_oracle_golden.py pins the oracle on them)."""
import ctypes as C
import types

import numpy as np
import pytest

import golden_cases
import golden_io
import intra_cases
import oracle_lib
from oracle_lib import HostPic
from openvvc_amd import capi, engine

pytestmark = pytest.mark.gpu
SENTINEL = 777          # what a destination picture holds before a launch that must not (or only partly) write it


@pytest.fixture(scope="module")
def ctx(built_lib):
    c = engine.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def sao_small():
    return {6: golden_cases.sao_cases("sao_ctu64.ovg"), 5: golden_cases.sao_cases("sao_ctu32.ovg")}


@pytest.fixture(scope="module")
def alf_small():
    return {6: golden_cases.alf_cases("alf_ctu64.ovg"), 5: golden_cases.alf_cases("alf_ctu32.ovg")}


def _sentinel_pic(ctx, w, h):
    return ctx.upload_pic(np.full((h, w), SENTINEL, np.uint16), np.full((h // 2, w // 2), SENTINEL, np.uint16),
                          np.full((h // 2, w // 2), SENTINEL, np.uint16))


def _assert_planes(got, exp: HostPic, what):
    for name, a, b in (("Y", got[0], exp.y), ("Cb", got[1], exp.cb), ("Cr", got[2], exp.cr)):
        bad = np.argwhere(a != b)
        assert len(bad) == 0, f"{what} plane {name}: {len(bad)} samples differ, first at (y,x) {bad[:6].tolist()}"


def _partitions(h, log2_ctu):
    """Row windows that together cover a picture of h rows: cut at the CTU rows, and at 8-row steps that are not CTU rows."""
    out = []
    for cuts in (range(1 << log2_ctu, h, 1 << log2_ctu), (40, 104)):
        edges = [0] + [c for c in cuts if c < h] + [h]
        out.append(list(zip(edges[:-1], edges[1:])))
    return out


# ---------------------------------------------------------------------------------------------------------------- SAO
@pytest.mark.parametrize("log2_ctu", [6, 5])
def test_sao_kernel_equals_the_reference(ctx, sao_small, log2_ctu):
    for i, (pic, prm, exp) in enumerate(sao_small[log2_ctu]):
        src = ctx.upload_pic(pic.y, pic.cb, pic.cr)
        dst = _sentinel_pic(ctx, pic.w, pic.h)
        ctx.sao(dst, src, ctx.upload(prm), log2_ctu)
        ctx.sync()
        _assert_planes(dst.download(), exp, f"k_sao at CTU {1 << log2_ctu}, picture {i} ({pic.w}x{pic.h})")
        src.free(); dst.free()


@pytest.mark.parametrize("log2_ctu", [6, 5])
def test_sao_row_windows_equal_the_reference(ctx, sao_small, log2_ctu):
    """ovhip_sao_launch_rows, what band-wise submission calls: every partition of the rows gives the whole-picture result."""
    for i, (pic, prm, exp) in enumerate(sao_small[log2_ctu]):
        src = ctx.upload_pic(pic.y, pic.cb, pic.cr)
        d_prm = ctx.upload(prm)
        for part in _partitions(pic.h, log2_ctu):
            dst = _sentinel_pic(ctx, pic.w, pic.h)
            for r0, r1 in part:
                ctx._chk(ctx.lib.ovhip_sao_launch_rows(ctx.h, C.byref(dst.s), C.byref(src.s), d_prm.ptr, log2_ctu, r0, r1), "sao_launch_rows")
            ctx.sync()
            _assert_planes(dst.download(), exp, f"k_sao at CTU {1 << log2_ctu}, picture {i} ({pic.w}x{pic.h}), windows {part}")
            dst.free()
        src.free()


# ---------------------------------------------------------------------------------------------------------------- ALF
def test_alf_kernel_equals_the_reference_ctu64(ctx, alf_small):
    for i, (pic, alf, exp) in enumerate(alf_small[6]):
        src = ctx.upload_pic(pic.y, pic.cb, pic.cr)
        dst = _sentinel_pic(ctx, pic.w, pic.h)
        ctx.alf(dst, src, engine.DevAlf(ctx, alf, pic.w, pic.h, log2_ctu=6))
        ctx.sync()
        _assert_planes(dst.download(), exp, f"k_alf at CTU 64, picture {i} ({pic.w}x{pic.h})")
        src.free(); dst.free()


def test_alf_row_windows_equal_the_reference_ctu64(ctx, alf_small):
    for i, (pic, alf, exp) in enumerate(alf_small[6]):
        src = ctx.upload_pic(pic.y, pic.cb, pic.cr)
        dalf = engine.DevAlf(ctx, alf, pic.w, pic.h, log2_ctu=6)
        for part in _partitions(pic.h, 6):
            dst = _sentinel_pic(ctx, pic.w, pic.h)
            for r0, r1 in part:
                ctx._chk(ctx.lib.ovhip_alf_launch_rows(ctx.h, C.byref(dst.s), C.byref(src.s), C.byref(dalf.s), r0, r1), "alf_launch_rows")
            ctx.sync()
            _assert_planes(dst.download(), exp, f"k_alf at CTU 64, picture {i} ({pic.w}x{pic.h}), windows {part}")
            dst.free()
        src.free()


def _filter_job(ctx, pic: HostPic, prm, alf, log2_ctu):
    """A job that runs SAO and ALF only on `pic`: (job, destination picture holding the input, parameters)"""
    job = engine.Job(ctx, pic.w, pic.h)
    job.begin()
    params = job.make_params(types.SimpleNamespace(sao_params=prm, alf=alf, lmcs=None), log2_ctu, capi.STAGE_SAO | capi.STAGE_ALF)
    return job, ctx.upload_pic(pic.y, pic.cb, pic.cr), params


def test_job_passes_the_ctu_size_to_both_filters(ctx, sao_small, alf_small):
    """ovhip_job_params.log2_ctu_s = 6 through ovvc_picture.hip into both launches: the 304x200 SAO input with the 304x200 ALF tables,
    expected = the oracle's ALF of the oracle's SAO at CTU 64."""
    pic, prm, _ = sao_small[6][0]
    _, alf, _ = alf_small[6][0]
    assert (pic.w, pic.h) == (304, 200) and len(prm) == len(alf["ctus"]) == 20
    mid, want = HostPic(pic.w, pic.h), HostPic(pic.w, pic.h)
    oracle_lib.sao(mid, pic, prm, 6)
    oracle_lib.alf(want, mid, alf, 6)
    at128 = HostPic(pic.w, pic.h)
    oracle_lib.alf(at128, mid, alf, 7)
    assert (at128.y != want.y).sum() > 100, "the picture does not tell CTU 64 from CTU 128"
    job, dst, params = _filter_job(ctx, pic, prm, alf, 6)
    job.flush(dst, [], None, params)
    job.wait()
    _assert_planes(dst.download(), want, "job with SAO and ALF at CTU 64")
    job.close()
    dst.free()


def test_alf_refuses_ctu32(ctx, sao_small, alf_small):
    """k_alf reads one parameter set per 32x32 tile, and a chroma tile would cover four chroma CTUs of 16: ALF at CTU 32 is not on the
    device, and the launch says so instead of filtering with the wrong CTU's parameters."""
    pic, alf, _ = alf_small[5][0]
    src = ctx.upload_pic(pic.y, pic.cb, pic.cr)
    dst = _sentinel_pic(ctx, pic.w, pic.h)
    dalf = engine.DevAlf(ctx, alf, pic.w, pic.h, log2_ctu=5)
    assert ctx.lib.ovhip_alf_launch(ctx.h, C.byref(dst.s), C.byref(src.s), C.byref(dalf.s)) == capi.OVHIP_EINVAL
    assert b"ovhip_alf_launch" in ctx.lib.ovhip_last_error(ctx.h)
    ctx.sync()
    assert all((p == SENTINEL).all() for p in dst.download()), "a refused launch wrote the destination"
    src.free(); dst.free()
    # the same through the job: the flush fails
    job, dst, params = _filter_job(ctx, pic, sao_small[5][0][1], alf, 5)
    with pytest.raises(engine.EngineError, match="ovhip_alf_launch"):
        job.flush(dst, [], None, params)
    ctx.sync()
    y, cb, cr = dst.download()
    assert np.array_equal(y, pic.y) and np.array_equal(cb, pic.cb) and np.array_equal(cr, pic.cr), "a failed flush wrote the destination"
    job.close()
    dst.free()


# ---------------------------------------------------------------------------------------------------------------- ordered intra pass
# (the placement of intra.ovg at a smaller CTU size: intra_cases.small_ctu, shared with test_gpu_intra_flow.py)
BAND, NB = intra_cases.BAND, intra_cases.NB
_intra_small_ctu, _in_bands, _case_ok, _describe = intra_cases.small_ctu, intra_cases.in_bands, intra_cases.case_ok, intra_cases.describe


@pytest.mark.parametrize("log2_ctu", [6, 5])
def test_intra_level_kernel_small_ctu(ctx, log2_ctu):
    S = 1 << log2_ctu
    tasks, exp_off, exp, base, n_out, n_first = _intra_small_ctu(S)
    assert n_out <= 25 and n_first >= 100, (n_out, n_first)
    assert len(tasks) + n_out == 6506
    W = base[0].shape[1]
    tall_planes = [np.tile(p, (NB, 1)) for p in base]
    res = ctx.new_pic(W, BAND * NB)
    bad = []
    for b0 in range(0, len(tasks), NB):
        t = _in_bands(tasks[b0:b0 + NB])
        pic = ctx.upload_pic(*tall_planes)
        ctx.intra_level(pic, res, ctx.upload(t), 0, len(t), log2_ctu=log2_ctu)
        ctx.sync()
        planes = pic.download()
        pic.free()
        bad += [_describe(b0 + i, t[i]) for i in range(len(t)) if not _case_ok(t[i], planes, exp_off[b0 + i], exp)]
    res.free()
    assert not bad, f"{len(bad)} / {len(tasks)} intra cases differ from the reference through k_intra_level at CTU {S}, first: {bad[:8]}"


def _inside_ctu_geometry(t, S):
    """The block lies in one CTU of size S, and so do the samples it reads, as in a decoder: the fixture draws positions and
    availability at random; a decoder never marks samples available that lie right of the CTU below its first row, or below the
    CTU (not decoded yet) -- the only samples the CTU tile does not hold.  (t: the task where it is run, y moved by S)"""
    chroma = t["kind"] != capi.IT_LUMA
    s, unit = (S // 2, 2) if chroma else (S, 4)
    x0, y0 = int(t["x"]), int(t["y"]) % (BAND // 2 if chroma else BAND)
    X0, Y0 = x0 & ~(s - 1), y0 & ~(s - 1)
    if x0 + (1 << int(t["log2_w"])) > X0 + s or y0 + (1 << int(t["log2_h"])) > Y0 + s:
        return False
    mrl = 0 if (chroma or t["flags"] & capi.IF_MIP) else int(t["mrl_idx"])
    if y0 == Y0 and mrl:
        return False
    if y0 > Y0 and x0 + unit * int(t["avl_abv"]) > X0 + s:
        return False
    return y0 + unit * int(t["avl_lft"]) <= Y0 + s


@pytest.mark.parametrize("log2_ctu,n_min", [(6, 3600), (5, 2000)])
def test_intra_ctu_kernel_small_ctu(ctx, log2_ctu, n_min):
    """k_intra_ctu builds its LDS tile from S = 1 << log2_ctu: every case is the only task of its CTU of that size."""
    S = 1 << log2_ctu
    tasks, exp_off, exp, base, n_out, n_first = _intra_small_ctu(S)
    assert n_out <= 25 and n_first >= 100, (n_out, n_first)
    W = base[0].shape[1]
    tall_planes = [np.tile(p, (NB, 1)) for p in base]
    res = ctx.new_pic(W, BAND * NB)
    sync = ctx.upload(np.zeros(int(ctx.lib.ovhip_intra_sync_words(W, BAND * NB, log2_ctu)), np.uint32))
    bad, n_checked = [], 0
    for epoch, b0 in enumerate(range(0, len(tasks), NB), 1):
        t = _in_bands(tasks[b0:b0 + NB])
        rec = capi.Recorder(W, BAND * NB)
        rec.append_raw(capi.REC_ITASK, t)
        ts, cs = rec.itasks_by_ctu(log2_ctu)
        rec.close()
        assert len(cs) == len(t) and not cs["deps"].any()
        pic = ctx.upload_pic(*tall_planes)
        ctx.intra_ctu(pic, res, ctx.upload(ts), ctx.upload(cs), len(cs), sync, epoch, log2_ctu=log2_ctu)
        ctx.sync()
        planes = pic.download()
        pic.free()
        inside = [_inside_ctu_geometry(t[i], S) for i in range(len(t))]
        n_checked += sum(inside)
        bad += [_describe(b0 + i, t[i]) for i in range(len(t)) if inside[i] and not _case_ok(t[i], planes, exp_off[b0 + i], exp)]
        # nothing but the task's block may change
        if not bad:
            for a, b, name in ((planes[0], tall_planes[0], "Y"), (planes[1], tall_planes[1], "Cb"), (planes[2], tall_planes[2], "Cr")):
                d = a != b
                for tt in t:
                    if (tt["kind"] == capi.IT_LUMA) == (name == "Y"):
                        d[int(tt["y"]):int(tt["y"]) + (1 << int(tt["log2_h"])), int(tt["x"]):int(tt["x"]) + (1 << int(tt["log2_w"]))] = False
                assert not d.any(), f"plane {name}: samples outside the tasks' blocks changed"
    res.free()
    assert n_checked >= n_min, n_checked
    assert not bad, f"{len(bad)} / {n_checked} intra cases differ from the reference through k_intra_ctu at CTU {S}, first: {bad[:8]}"


# ---------------------------------------------------------------------------------------------------------------- TMVP cells
@pytest.mark.parametrize("log2_ctu", [5, 6, 7])
def test_tmvp_cells_at_every_position_of_a_3x2_ctu_picture(ctx, log2_ctu):
    """DMVR units at every 8-aligned position, in the four shapes 8 / 16 x 8 / 16 that fit their CTU: the kernel's cells == the oracle's
    == the plane layout of tmvp_store_mv: a raster of 8x8 cells with stride (ctu >> 3) * nb_ctb_w."""
    ctu, nb_ctb_w = 1 << log2_ctu, 3
    pos = [(x, y, w, h) for y in range(0, 2 * ctu, 8) for x in range(0, 3 * ctu, 8) for w in (8, 16) for h in (8, 16)
           if (x & (ctu - 1)) + w <= ctu and (y & (ctu - 1)) + h <= ctu]
    units = np.zeros(len(pos) + 8, capi.MC_UNIT_DTYPE)
    p = np.array(pos)
    n = len(pos)
    units["x"][:n], units["y"][:n], units["w"][:n], units["h"][:n] = p[:, 0], p[:, 1], p[:, 2], p[:, 3]
    units["flags"][:n] = capi.MC_DMVR
    units["x"][n:], units["y"][n:], units["w"][n:], units["h"][n:] = 8 * np.arange(8), 8, 16, 16        # not refined: no cells
    units["flags"][n:] = capi.MC_BDOF
    mv = (1000 + 8 * np.arange(len(units))[:, None] + np.arange(4)[None, :]).astype(np.int32)
    got = ctx.tmvp_cells(ctx.upload(units), len(units), ctx.upload(mv), log2_ctu, nb_ctb_w)
    assert np.array_equal(got, oracle_lib.tmvp_cells(units, mv, log2_ctu, nb_ctb_w)), "kernel != oracle"
    stride = (ctu >> 3) * nb_ctb_w
    want = np.zeros(4 * len(units), capi.TMVP_CELL_DTYPE)
    want["cell"] = capi.TMVP_NONE
    w4 = want.reshape(-1, 4)
    base = (p[:, 1] >> 3) * stride + (p[:, 0] >> 3)
    for k, (on, off) in enumerate(((np.ones(n, bool), 0), (p[:, 2] > 8, 1), (p[:, 3] > 8, stride), ((p[:, 2] > 8) & (p[:, 3] > 8), stride + 1))):
        idx = np.nonzero(on)[0]
        w4["cell"][idx, k] = base[idx] + off
        for c, name in enumerate(("mv0x", "mv0y", "mv1x", "mv1y")):
            w4[name][idx, k] = mv[idx, c]
    assert np.array_equal(got, want), "kernel != the plane layout of tmvp_store_mv"
    used = got["cell"][got["cell"] != capi.TMVP_NONE]
    assert len(np.unique(used)) == stride * 2 * (ctu >> 3), "not every cell of the plane is written"
