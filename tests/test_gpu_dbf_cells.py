"""GPU: directed deblocking cells (tests/dbf_cells.py) through every route into the deblocking kernels, compared sample by sample
on all three planes with the plain restatement tests/spec_dbf.py (pinned to the reference by tests/test_dbf_spec_cpu.py).

Whole planes are compared, not the cells' rectangles: everything between the cells is noise and must come back untouched.
The cells of one direction share no sample, so the result does not depend on the order of the list -- the shuffled run checks
exactly that.  k_dbf (dense planes) runs its long filters here for the first time; k_dbf_list sees all 8 offset-pair indices,
negative offsets, both ends of both threshold tables and vertical chroma edges at both alignments."""
from functools import lru_cache

import numpy as np
import pytest

import dbf_cells
import pipe_cases
import spec_dbf
from openvvc_amd import capi, engine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(built_lib):
    c = engine.Context(0)
    yield c
    c.close()


@lru_cache(maxsize=None)
def cells():
    return dbf_cells.build()


@lru_cache(maxsize=None)
def expected(n=None):
    """spec_dbf on the first n edges of each list (all of them by default), computed once per length"""
    y, cb, cr, ev, eh, offs, _, _ = cells()
    return spec_dbf.filter(y, cb, cr, ev[:n], eh[:n], offs)


def run_lists(ctx, ev, eh, offs):
    y, cb, cr = cells()[:3]
    d = ctx.upload_pic(y, cb, cr)
    ctx.dbf_edges_ex(d, ctx.upload(ev), ctx.upload(eh), offs)
    ctx.sync()
    return d.download()


def compare(got, want, what):
    for name, a, b in zip(("Y", "Cb", "Cr"), got, want[:3]):
        bad = np.argwhere(a != b)
        assert len(bad) == 0, f"{what}, plane {name}: {len(bad)} samples differ from the restatement, first at (y, x) {bad[:6].tolist()}"


def test_every_cell_takes_its_branch():
    """(needs no device; here as well so that a device run never compares cells that drifted into another branch)"""
    _, _, _, _, _, _, cv, ch = cells()
    want = expected()
    assert not dbf_cells.check_labels(cv, want[3]) and not dbf_cells.check_labels(ch, want[4])


@pytest.mark.parametrize("order", ["raster", "shuffled"])
def test_edge_lists_with_offset_table(ctx, order):
    _, _, _, ev, eh, offs, _, _ = cells()
    if order == "shuffled":
        rng = np.random.default_rng(7)
        ev, eh = ev[rng.permutation(len(ev))], eh[rng.permutation(len(eh))]
    compare(run_lists(ctx, ev, eh, offs), expected(), f"ovhip_dbf_launch_edges_ex ({order})")


@pytest.mark.parametrize("n", [1, 63, 64, 65, 64 * 9 + 3])
def test_edge_lists_cut_short(ctx, n):
    """one quad; a tail inside a block of 64 edges; exactly one block; one edge into the second; 10 blocks: a grid that is no
    multiple of the 8 XCDs the blocks are dealt over"""
    _, _, _, ev, eh, offs, _, _ = cells()
    assert len(ev) >= n and len(eh) >= n
    want = expected(n)
    assert want[3]["changed"].any() or n == 1
    compare(run_lists(ctx, ev[:n], eh[:n], offs), want, f"lists cut to {n} edges")


def _subset(idx, dense):
    _, _, _, ev, eh, _, cv, ch = cells()
    keep = []
    for e in (ev, eh):
        k = e["pad"] == idx
        if dense:                                   # the dense chroma planes hold every second unit column only
            k &= ~((e["comp"] > 0) & (e["ux"] % 2 == 1))
        keep.append(k)
    return ev[keep[0]], eh[keep[1]], [c for c, k in zip(cv, keep[0]) if k], [c for c, k in zip(ch, keep[1]) if k]


@pytest.mark.parametrize("layout", ["tight", "view"])
def test_dense_planes(ctx, layout):
    """ovhip_dbf_launch (k_dbf) on the planes the cells of ONE pair stand for: the whole luma matrix, long filters included.
    view: the picture is the left 320 columns of a 322-wide noise picture -- strides above the width, luma rows whose 8-byte
    alignment alternates (stride 644 bytes) and chroma rows at every 2-byte alignment (322 bytes), so the vertical-edge line load
    takes its vector and its scalar path; the columns outside the view must come back untouched"""
    y, cb, cr, _, _, offs, _, _ = cells()
    ev, eh, cv, ch = _subset(dbf_cells.DENSE_IDX, dense=True)
    want = spec_dbf.filter(y, cb, cr, ev, eh, offs)
    for cs, br in ((cv, want[3]), (ch, want[4])):
        assert not dbf_cells.check_labels(cs, br)
        lng = br[(br["comp"] == 0) & (br["kind"] == "long")]
        assert set(zip(lng["lp"].tolist(), lng["lq"].tolist())) == set(dbf_cells.LONG_PAIRS)
        assert {"off", "strong", "weak"} <= set(br["kind"][br["comp"] == 0].tolist()) and {"strong", "weak"} <= set(br["kind"][br["comp"] > 0].tolist())
    planes = pipe_cases.edges_to_planes(ev, eh, dbf_cells.W // 4, dbf_cells.H // 4)
    planes["beta_offset"], planes["tc_offset"] = dbf_cells.OFF_BETA[dbf_cells.DENSE_IDX], dbf_cells.OFF_TC[dbf_cells.DENSE_IDX]
    for d in (0, 1):                                # the planes hold exactly these segments
        assert len(capi.dbf_compact(planes, d)) == len((ev, eh)[d])
    if layout == "tight":
        d = ctx.upload_pic(y, cb, cr)
        ctx.dbf(d, engine.DevDbfPlanes(ctx, planes))
        ctx.sync()
        compare(d.download(), want, "ovhip_dbf_launch (dense planes)")
        return
    W, H, WIDE = dbf_cells.W, dbf_cells.H, dbf_cells.W + 2
    assert WIDE % 4 == 2
    rng = np.random.default_rng(11)
    wide = [rng.integers(0, 1024, (H // s, WIDE // s)).astype(np.uint16) for s in (1, 2, 2)]
    for big, part in zip(wide, (y, cb, cr)):
        big[:, :part.shape[1]] = part
    pic = ctx.upload_pic(*wide)
    assert (pic.s.stride_y, pic.s.stride_c) == (WIDE, WIDE // 2)
    view = engine.DevPic(ctx, capi.Pic(pic.s.y, pic.s.cb, pic.s.cr, W, H, pic.s.stride_y, pic.s.stride_c), owns=False)
    ctx.dbf(view, engine.DevDbfPlanes(ctx, planes))
    ctx.sync()
    got = pic.download()
    compare([g[:, :p.shape[1]] for g, p in zip(got, (y, cb, cr))], want, "ovhip_dbf_launch (dense planes, 320x320 view of 322x320)")
    for name, g, big, part in zip(("Y", "Cb", "Cr"), got, wide, (y, cb, cr)):
        assert np.array_equal(g[:, part.shape[1]:], big[:, part.shape[1]:]), f"plane {name}: columns outside the view changed"
    pic.free()


def test_single_pair_wrapper_with_a_negative_pair(ctx):
    """ovhip_dbf_launch_edges fills all 8 slots with its one pair; here (-24, -24): a lost sign would push both indices past
    the tables' ends, where both limits are 0 and nothing is filtered"""
    y, cb, cr, _, _, offs, _, _ = cells()
    ev, eh, _, _ = _subset(dbf_cells.NEG_IDX, dense=False)
    beta, tc = dbf_cells.OFF_BETA[dbf_cells.NEG_IDX], dbf_cells.OFF_TC[dbf_cells.NEG_IDX]
    assert beta < 0 and tc < 0
    want = spec_dbf.filter(y, cb, cr, ev, eh, offs)
    assert want[3]["changed"].sum() >= 8 and want[4]["changed"].sum() >= 8
    ev, eh = ev.copy(), eh.copy()
    ev["pad"] = 0; eh["pad"] = 0
    d = ctx.upload_pic(y, cb, cr)
    ctx.dbf_edges(d, ctx.upload(ev), ctx.upload(eh), beta, tc)
    ctx.sync()
    compare(d.download(), want, "ovhip_dbf_launch_edges (-24, -24)")
