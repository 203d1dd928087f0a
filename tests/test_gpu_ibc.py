"""GPU: intra block copy through the picture job's ordered pass.  Picture = a scenario's background uploaded, then ovhip_job_flush: the
fixtures of tests/golden/ibc (expected frames written by the reference, tools/ibc_golden/gen_ibc.c) under the flow launch, one launch per
level and the route a picture asked for as the CTU pass takes; with LMCS; and compositions with intra tasks from pieces pinned elsewhere.
Everything bit-exact; after every flush no second pass was needed and no sample carries the flow launch's hand-over bit."""
import ctypes as C

import numpy as np
import pytest

import ibc_cases
import spec_ibc as S
from openvvc_amd import capi, engine, synth

pytestmark = pytest.mark.gpu
STAGES = capi.STAGE_MC | capi.STAGE_ITX | capi.STAGE_INTRA          # no loop filter: IBC reads and the fixtures hold the picture before them


@pytest.fixture(scope="module")
def ctx(built_lib):
    c = engine.Context(0)
    yield c
    c.close()


def _params(extra=0, lmcs=None):
    p = capi.JobParams()
    p.log2_ctu_s, p.stages = 7, STAGES | extra
    p.lmcs = C.addressof(lmcs) if lmcs is not None else None
    return p


def _flush(ctx, w, h, start, record, extra=0, lmcs=None):
    """One picture: `start` uploaded, record(job.rec) recorded, flushed; returns the planes."""
    job = engine.Job(ctx, w, h)
    job.begin()
    record(job.rec)
    dst = ctx.upload_pic(*[np.ascontiguousarray(p, dtype=np.uint16) for p in start])
    job.flush(dst, [], None, params=_params(extra, lmcs))
    job.wait()
    st = job.stats()
    got = dst.download()
    dst.free()
    job.close()
    assert st.n_ordered_retries == 0
    for name, p in zip(("Y", "Cb", "Cr"), got):
        assert not (p & 0x8000).any(), f"plane {name}: samples left with the hand-over bit"
    return got, st


def _same(got, exp, what):
    for name, a, b in zip(("Y", "Cb", "Cr"), got, exp):
        assert np.array_equal(a, b), f"{what}: plane {name}: {int((a != b).sum())} samples differ, first at {np.argwhere(a != b)[0]}"


@pytest.mark.parametrize("name,route", [("a", 0), ("a", capi.STAGE_INTRA_LEVELS), ("a", capi.STAGE_INTRA_CTU), ("b", 0), ("b", capi.STAGE_INTRA_LEVELS)])
def test_fixture_pictures_equal_the_reference(ctx, name, route):
    """Scenarios a (512x128) and b (two CTU rows) == the frame the reference's rcn_ibc_l / rcn_ibc_c + transform tree left, under the flow
    launch (default), one launch per level, and -- a only -- asked for as the CTU pass, which IBC pictures run level by level."""
    sc = S.scenario(name)
    got, st = _flush(ctx, sc.w, sc.h, sc.bg, lambda rec: ibc_cases.record(rec, sc), extra=route)
    _same(got, sc.exp, f"scenario {name}, route {route:#x}")
    assert st.n_itasks > 200 and st.n_ilevels >= 32
    if route:
        assert st.n_launches >= st.n_ilevels                # one launch per level, not one for the pass


def test_fixture_picture_with_lmcs(ctx):
    """Scenario a with the job's LMCS on: the copies happen in the mapped domain, the inverse mapping follows the pass (result = the inverse
    LUT applied to the expected luma); chroma residuals are scaled with a constant scale, restated in numpy (spec_ibc.scaled)."""
    sc = S.scenario("a")
    luts = synth._lmcs_tables(np.random.RandomState(5))
    bwd = np.frombuffer(bytes(luts), np.uint16)[1024:2048]
    scale = 2600
    exp, _ = S.decode_ring(sc, chroma_scale=scale)
    plain, _ = S.decode_ring(sc)
    assert not np.array_equal(exp[1], plain[1]), "the scale changes chroma"
    got, _ = _flush(ctx, sc.w, sc.h, sc.bg, lambda rec: ibc_cases.record(rec, sc, chroma_scale=scale), lmcs=luts)
    _same(got, [bwd[exp[0]], exp[1], exp[2]], "scenario a with LMCS")


def test_band_submission_refuses_ibc_pictures(ctx):
    sc = S.scenario("a")
    job = engine.Job(ctx, sc.w, sc.h)
    job.begin()
    ibc_cases.record(job.rec, sc)
    dst = ctx.upload_pic(*sc.bg)
    job.params = _params()
    with pytest.raises(engine.EngineError, match="intra block copy"):
        job.band(dst, [], sc.h, last=True)
    dst.free()
    job.close()


# ---- compositions with intra tasks, 256x128, blocks 4x4 .. 32x32 ----
W, H = 256, 128


def _planes(seed):
    rs = np.random.RandomState(seed)
    return [rs.randint(0, 1024, (H, W)).astype(np.uint16), rs.randint(0, 1024, (H // 2, W // 2)).astype(np.uint16), rs.randint(0, 1024, (H // 2, W // 2)).astype(np.uint16)]


class _Intra:
    """Intra CUs (luma + chroma tasks, transform-skip luma residual) as ovhip_rec_tu_intra calls"""

    def __init__(self, blocks, seed):
        rs = np.random.RandomState(seed)
        self.blocks = blocks                                   # (x0, y0, log2 size, luma mode, chroma mode)
        self.coef = [np.ascontiguousarray(rs.randint(-60, 61, (1 << l2, 1 << l2)).astype(np.int16)) for _, _, l2, _, _ in blocks]

    def record(self, rec):
        st = capi.TuState()
        for (x0, y0, l2, mode, mode_c), coef in zip(self.blocks, self.coef):
            n = (1 << l2) >> 2
            d = capi.TuDesc()
            d.x0, d.y0, d.log2_tb_w, d.log2_tb_h, d.tree, d.cu_flags = x0, y0, l2, l2, 0 if l2 > 2 else 1, 2          # (4x4: luma only)
            d.cbf_mask, d.tr_skip_mask, d.coef[2] = 0x10, 0x10, coef.ctypes.data
            tl, tc = capi.ITask(), capi.ITask()
            tl.kind, tl.x, tl.y, tl.log2_w, tl.log2_h, tl.mode = capi.IT_LUMA, x0, y0, l2, l2, mode
            tc.kind, tc.x, tc.y, tc.log2_w, tc.log2_h, tc.mode = capi.IT_CHROMA, x0 >> 1, y0 >> 1, l2 - 1, l2 - 1, mode_c
            for t in (tl, tc):
                t.avl_abv, t.avl_lft = (n if y0 else 0), (n if x0 else 0)
                t.flags = capi.IF_CORNER if x0 and y0 else 0
            assert rec.tu_intra(st, d, tl, tc if l2 > 2 else None) >= 0


def _ibc_scenario(cus, seed):
    """A spec_ibc.Scenario of IBC CUs (x0, y0, log2 size, mv_x, mv_y, has_chroma) with seeded transform-skip residuals on every plane"""
    rs = np.random.RandomState(seed)
    cu, tu, maps, coef = [], [], [], []
    for k, (x0, y0, l2, mx, my, chroma) in enumerate(cus):
        cu.append((x0, y0, l2, l2, mx, my, chroma, k))
        row = [k, x0, y0, l2, l2, 0 if chroma else 1, 0x13 if chroma else 0x10, 0x13 if chroma else 0x10, 0x0101, 0x0101, 0x0101, -1, -1, -1]
        for comp in ((0, 1, 2) if chroma else (2,)):
            n = 1 << (2 * (l2 - (comp != 2)))
            row[S.TU_COEF + comp] = sum(len(c) for c in coef)
            coef.append(rs.randint(-90, 91, n).astype(np.int16))
        tu.append(row); maps.append((1, 1, 1))
    g = {"x_dims": np.array([W, H, 7, 5], np.uint32), "x_cu": np.array(cu, np.int32), "x_tu": np.array(tu, np.int32), "x_map": np.array(maps, np.uint64),
         "x_coef": np.concatenate(coef), "x_state": np.frombuffer(bytes(capi.TuState()), np.uint8)}
    for p in ("y", "cb", "cr"):
        g[f"x_bg_{p}"] = g[f"x_exp_{p}"] = np.zeros((1, 1), np.uint16)
    return S.Scenario(g, "x")


INTRA_LEFT = [(32, 0, 5, 0, 1), (64, 0, 4, 1, 0), (80, 0, 3, 34, 1), (88, 0, 2, 50, 0), (64, 16, 4, 18, 0), (32, 32, 5, 66, 1), (64, 32, 3, 2, 0), (72, 32, 2, 1, 1)]


def test_ibc_cus_copying_intra_blocks(ctx):
    """One job with intra tasks plus IBC CUs that copy those blocks (whole, and across several of them at odd offsets) == [the job with
    the intra tasks only -> download -> the copies + residuals in numpy]."""
    bg = _planes(11)
    intra = _Intra(INTRA_LEFT, 12)
    sc = _ibc_scenario([(160, 0, 5, -128, 0, 1), (192, 0, 4, -128, 0, 1), (208, 0, 3, -129, 3, 1), (216, 0, 2, -131, 1, 0), (160, 32, 5, -113, -31, 1),
                        (192, 32, 4, -27, -29, 1), (224, 32, 3, -8, 0, 1), (232, 32, 2, -12, 2, 0), (160, 64, 5, -117, -30, 1)], 13)
    first, _ = _flush(ctx, W, H, bg, intra.record)
    exp, _ = S.decode_picture(sc, bg=first)
    got, st = _flush(ctx, W, H, bg, lambda rec: (intra.record(rec), ibc_cases.record(rec, sc)))
    _same(got, exp, "intra tasks + IBC CUs copying them")
    assert st.n_ilevels >= 4
    got, _ = _flush(ctx, W, H, bg, lambda rec: (intra.record(rec), ibc_cases.record(rec, sc)), extra=capi.STAGE_INTRA_LEVELS)
    _same(got, exp, "intra tasks + IBC CUs copying them, one launch per level")


def test_intra_tasks_predicting_from_ibc_cus(ctx):
    """One job with IBC CUs plus intra tasks whose reference arms are those CUs == [the job with the IBC CUs only -> its result uploaded as
    the next picture's start -> the job with the intra tasks only]."""
    bg = _planes(21)
    sc = _ibc_scenario([(128, 0, 5, -100, 5, 1), (160, 0, 4, -16, 0, 1), (128, 32, 4, 3, -32, 1), (144, 32, 3, -77, 9, 1), (152, 32, 2, -4, 0, 0),
                        (144, 40, 3, 0, -8, 1)], 22)
    # blocks right of / below the IBC CUs: their above and left arms, and the corner, are IBC samples
    intra = _Intra([(176, 0, 4, 18, 1), (160, 16, 4, 50, 0), (176, 16, 3, 0, 1), (184, 16, 2, 1, 0), (128, 48, 4, 34, 1), (144, 48, 3, 66, 0), (152, 40, 2, 2, 1),
                    (192, 0, 5, 0, 0)], 23)
    first, _ = _flush(ctx, W, H, bg, lambda rec: ibc_cases.record(rec, sc))
    _same(first, S.decode_picture(sc, bg=bg)[0], "the IBC CUs alone")
    exp, _ = _flush(ctx, W, H, first, intra.record)
    got, st = _flush(ctx, W, H, bg, lambda rec: (ibc_cases.record(rec, sc), intra.record(rec)))
    _same(got, exp, "IBC CUs + intra tasks predicting from them")
    assert st.n_ilevels >= 4
    got, _ = _flush(ctx, W, H, bg, lambda rec: (ibc_cases.record(rec, sc), intra.record(rec)), extra=capi.STAGE_INTRA_LEVELS)
    _same(got, exp, "IBC CUs + intra tasks predicting from them, one launch per level")
