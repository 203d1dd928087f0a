"""GPU: the flow launch of the ordered pass (k_intra_flow, the route every picture takes by default) on the reference's own intra
slot cases -- intra.ovg and the enumerated cells of intra_cells_*.ovg (tests/intra_census.py says what they reach) -- at CTU 128, 64
and 32.  Its reference arms (fetch_refs_tagged), packed epilogue (flow_load / flow_store), 256-sample strips and k_flow_untag are code
of its own; the picture tests see them only on random CTUs and against the oracle.

Every case sits alone on its band of a tall picture, so no item has anything to wait for: an abort word != 0 is a finding about
which state words the kernel reads, and the test stops there -- nothing more is launched."""
import numpy as np
import pytest

import intra_cases
from intra_cases import BAND, NB
from openvvc_amd import engine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(built_lib):
    c = engine.Context(0)
    yield c
    c.close()


def _run_flow(ctx, tasks, exp_off, exp, S, log2_ctu, n_workers, what):
    """tasks (all level 1: level-sorted as they stand) NB per launch through k_intra_flow + k_flow_untag on the fixture's picture placed
    S rows down each band.  After every launch: the abort word is 0; every case's block equals the reference's; with those blocks set
    back to the start picture, all three planes EQUAL the start picture -- no sample outside the cases' blocks changed, and since
    neither the start picture nor an expected block holds a sample above 1023, no sample of the picture has bit 15 set."""
    assert (tasks["level"] == 1).all()
    start = intra_cases.tall_planes(S)
    assert int(exp.max()) < 0x8000 and all(int(p.max()) < 0x8000 for p in start)
    W = start[0].shape[1]
    res = ctx.new_pic(W, BAND * NB)
    state = ctx.upload(np.zeros(ctx.intra_flow_words(W, BAND * NB), np.uint32))
    try:
        for epoch, b0 in enumerate(range(0, len(tasks), NB), 1):
            t = intra_cases.in_bands(tasks[b0:b0 + NB])
            items = ctx.intra_flow_items(t)
            assert len(items) >= len(t)
            pic = ctx.upload_pic(*start)
            d_t, d_items = ctx.upload(t), ctx.upload(items)
            ctx.intra_flow(pic, res, d_t, len(t), d_items, len(items), state, epoch, log2_ctu=log2_ctu, prepare=1, n_workers=n_workers)
            abort = ctx.intra_flow_abort(state)
            assert abort == 0, f"{what}: a wait of the flow launch expired (abort word {abort}) on cases {b0}..{b0 + len(t) - 1}, each alone on its band"
            ctx.intra_flow_untag(pic, d_t, len(t), 1)
            ctx.sync()
            planes = pic.download()
            pic.free(); d_t.free(); d_items.free()
            bad = [intra_cases.describe(b0 + i, t[i]) for i in range(len(t)) if not intra_cases.case_ok(t[i], planes, exp_off[b0 + i], exp)]
            assert not bad, f"{what}: {len(bad)} of the cases {b0}..{b0 + len(t) - 1} differ from the reference, first: {bad[:8]}"
            intra_cases.restore_blocks(planes, start, t)
            for name, a, b in zip(("Y", "Cb", "Cr"), planes, start):
                if not np.array_equal(a, b):
                    yx = np.argwhere(a != b)
                    tagged = int((a[a != b] & 0x8000 != 0).sum())
                    assert False, (f"{what}: plane {name}: {len(yx)} samples outside the tasks' blocks changed ({tagged} of them carry the hand-over "
                                   f"bit), first (y, x): {yx[:6].tolist()}")
    finally:
        res.free(); state.free()


@pytest.mark.parametrize("n_workers", [0, 5])
@pytest.mark.parametrize("fixture", intra_cases.FIXTURES)
def test_flow_launch_matches_reference(ctx, fixture, n_workers):
    """one workgroup per item (0) and five persistent workers that take the items in turn"""
    tasks, exp_off, exp, pic = intra_cases.load(fixture)
    _run_flow(ctx, tasks, exp_off, exp, 0, 7, n_workers, f"{fixture}, {n_workers} workers")


@pytest.mark.parametrize("log2_ctu", [6, 5])
@pytest.mark.parametrize("fixture", intra_cases.FIXTURES)
def test_flow_launch_small_ctu(ctx, fixture, log2_ctu):
    """the placement of test_gpu_ctu_sizes.py: LM cases at y0 = 0 are on a first line only for a CTU of this size"""
    S = 1 << log2_ctu
    tasks, exp_off, exp, base, n_out, n_first = intra_cases.small_ctu(S, fixture)
    assert n_out <= 25 and n_first >= 100, (n_out, n_first)
    _run_flow(ctx, tasks, exp_off, exp, S, log2_ctu, 0, f"{fixture} at CTU {S}")
