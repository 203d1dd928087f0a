"""GPU: the enumerated inverse transform cells (tests/golden/itx_cells_*.ovg, gen_itx_cells) through every body of k_itx_all.

Each file goes three ways against the reference's blocks, every case on its own 128-row band of one tall picture (golden_cases.itx_cases_rec):
  "itx"      ovhip_itx_launch: every block in the four-wave body;
  "classes"  ovhip_itx_launch_classes on the recorder's split: one-wave generic, specialised and DC bodies;
  "job"      a picture job (engine.Job, STAGE_ITX | STAGE_INTRA): the tiny bodies, and the STORE sink for the blocks of ordered tasks.
After each, the cases' rectangles equal the reference and every other sample equals the start picture.  tests/itx_census.py says which
body a command takes on which route; test_routes_run_every_cell_the_census_claims ties the launches below to it."""
import functools

import numpy as np
import pytest

import golden_cases
import golden_io
import itx_census as ic
from oracle_lib import HostPic
from openvvc_amd import capi, engine

pytestmark = pytest.mark.gpu
BAND = golden_cases.BAND
FILES = golden_cases.itx_cell_files()


@pytest.fixture(scope="module")
def ctx(built_lib):
    c = engine.Context(0)
    yield c
    c.close()


def start(g, n):
    """the fixtures' 128x128 prediction picture on n bands"""
    return HostPic(128, BAND * n, np.tile(g["pred_y"], (n, 1)), np.tile(g["pred_cb"], (n, 1)), np.tile(g["pred_cr"], (n, 1)))


@functools.lru_cache(maxsize=None)
def plan(name, route):
    """What `route` launches for the fixture `name`: the number of cases (= bands of the start picture), the commands in launch order,
    the class counts of the split (luma large, luma small, chroma large, chroma small), the coefficient arena, the ordered tasks
    (route "job"), rects, expected."""
    pic, rec, _, rects, exp = golden_cases.itx_cases_rec(name, ordered=route == "job")
    cmds, counts = rec.tb_cmds().copy(), None
    if route != "itx":
        order, counts = ic.split_order(cmds)
        split, rec_counts = rec.tb_cmds_split()
        assert counts == rec_counts and split.tobytes() == cmds[order].tobytes(), "the census restates another split than the recorder's"
        if route == "classes":
            cmds = split
    tasks = rec.itasks().copy()
    tasks["kind"] = capi.IT_RES_C            # the reference ran with intra_pred_c stubbed out: the residual half of the task only
    return pic.h // BAND, cmds, counts, rec.coefs().copy(), tasks, rects, exp


def check(start, got, rects, exp, what):
    """the cases' rectangles equal the reference's blocks; every sample outside them is the start picture's"""
    golden_cases.check_rects(got, rects, exp, what)
    for p, (a, b) in enumerate(zip(start.planes(), got.planes())):
        outside = np.ones(a.shape, bool)
        for q, x, y, w, h, _ in rects:
            if q == p:
                outside[y:y + h, x:x + w] = False
        bad = np.argwhere(outside & (a != b))
        assert len(bad) == 0, f"{what}: {len(bad)} samples of plane {p} outside the cases' rectangles changed, first at (y, x) {bad[:6].tolist()}"


def run_job(ctx, pic, cmds, coefs, tasks):
    d = ctx.upload_pic(pic.y, pic.cb, pic.cr)
    job = engine.Job(ctx, pic.w, pic.h)
    job.begin()
    job.rec.append_raw(capi.REC_COEF, coefs)
    job.rec.append_raw(capi.REC_TB, cmds)
    if len(tasks):
        job.rec.append_raw(capi.REC_ITASK, tasks)
    # what the flush launches is the job's own recorder's split: the same order and counts as the census restates
    order, counts = ic.split_order(cmds)
    split, rec_counts = job.rec.tb_cmds_split()
    assert counts == rec_counts and split.tobytes() == cmds[order].tobytes()
    p = capi.JobParams()
    p.log2_ctu_s = 7
    p.stages = capi.STAGE_ITX | (capi.STAGE_INTRA if len(tasks) else 0)
    job.flush(d, [], None, params=p)
    job.wait()
    job.close()
    return HostPic(pic.w, pic.h, *d.download())


@pytest.mark.parametrize("name", FILES)
def test_itx_cells_four_wave(ctx, name):
    n, cmds, _, coefs, _, rects, exp = plan(name, "itx")
    pic = start(golden_io.load(name), n)
    d = ctx.upload_pic(pic.y, pic.cb, pic.cr)
    ctx.itx(d, ctx.upload(cmds), ctx.upload(coefs))
    ctx.sync()
    check(pic, HostPic(pic.w, pic.h, *d.download()), rects, exp, f"{name}, every block four-wave")


@pytest.mark.parametrize("name", FILES)
def test_itx_cells_one_wave(ctx, name):
    n, cmds, counts, coefs, _, rects, exp = plan(name, "classes")
    pic = start(golden_io.load(name), n)
    d = ctx.upload_pic(pic.y, pic.cb, pic.cr)
    dc, da = ctx.upload(cmds), ctx.upload(coefs)
    ctx.itx_classes(d, dc, da, 0, counts[0], counts[1])
    ctx.itx_classes(d, dc, da, counts[0] + counts[1], counts[2], counts[3])
    ctx.sync()
    check(pic, HostPic(pic.w, pic.h, *d.download()), rects, exp, f"{name}, the recorder's classes")


@pytest.mark.parametrize("name", FILES)
def test_itx_cells_picture_job(ctx, name):
    n, cmds, _, coefs, tasks, rects, exp = plan(name, "job")
    pic = start(golden_io.load(name), n)
    check(pic, run_job(ctx, pic, cmds, coefs, tasks), rects, exp, f"{name}, picture job")


def test_routes_run_every_cell_the_census_claims():
    """Over the three routes above, every body was handed every cell tests/itx_census.py claims for it (test_itx_fixture_census asserts
    what those are), the STORE sinks among them, and four different one-wave paths met in one workgroup, four times with all four at
    the most LDS the class uses.  This test launches nothing; it labels the commands plan() gives the launches above.  What ties the
    labels to the device is: the split (order and class counts) is asserted against the recorder's own in plan() and in run_job(), and
    the tests above launch exactly those commands with exactly those counts.  The restated `switch` of k_itx_all (specialised or
    generic body) and the hand-over of the tiny counts inside the picture job are read off the source, not observed on the device: if
    they change, the restatement in itx_census.body() has to follow."""
    ran, store = set(), set()
    for name in FILES:
        for route in ic.ROUTES:
            _, cmds, _, _, _, _, _ = plan(name, route)
            ran |= ic.reach(cmds, (route,))["body_cells"]
            if route == "job":
                store |= set(ic.label(cmds)["sink"])
    claimed = ic.reach(ic.load(FILES)[0])["body_cells"]
    assert ran == claimed and {b for b, *_ in ran} == set(range(5))
    # blocks of ordered tasks: the dual-tree chroma blocks of the intra CUs in the lfnst and bdpcm files, Cb and Cr, plain add into STORE
    assert {s for s in store if s[3]} == {(1, capi.RES_ADD, None, True, False), (2, capi.RES_ADD, None, True, False)}
    # the quads of itx_cells_quad_00.ovg as the classes route launches them: four commands to a workgroup
    _, cmds, counts, _, _, _, _ = plan("itx_cells_quad_00.ovg", "classes")
    assert counts == (0, len(cmds), 0, 0) and len(cmds) % 4 == 0
    lb, body = ic.label(cmds), ic.body(cmds, "classes")
    path = ["lfnst" if lb["lfnst"][i] else "bdpcm" if lb["kind"][i] in (ic.K_BDPCM_H, ic.K_BDPCM_V) else "dc" if body[i] == ic.DC1 else
            "plain" if body[i] == ic.SPEC else "?" for i in range(len(cmds))]
    quads = [(set(path[q:q + 4]), set(lb["shape"][q:q + 4])) for q in range(0, len(cmds), 4)]
    assert all(p == {"lfnst", "bdpcm", "dc", "plain"} for p, _ in quads)
    assert sum(s == {(4, 4), (5, 3), (3, 5), (5, 2)} for _, s in quads) >= 4


@functools.lru_cache(maxsize=None)
def tiny_pool():
    """the plain tiny blocks of every fixture, by shape: (command, its coefficients, expected block)"""
    pool = {s: [] for s in ic.TINY_SHAPES}
    for name in ["itx.ovg"] + FILES:
        _, cmds, _, coefs, _, rects, exp = plan(name, "itx")
        where = {(p, x, y): off for p, x, y, _, _, off in rects}
        shape = ic.tiny_shape(cmds)
        for i in np.nonzero((shape > 0) & (cmds["plane2"] == 0xff))[0]:
            c = cmds[i]
            w, h, n = 1 << int(c["log2_w"]), 1 << int(c["log2_h"]), 16 * bin(int(c["sig_sb_map"])).count("1")
            off = where[(int(c["plane"]), int(c["x"]), int(c["y"]))]
            pool[ic.TINY_SHAPES[shape[i] - 1]].append((c.copy(), coefs[int(c["coef_off"]):int(c["coef_off"]) + n].copy(), exp[off:off + w * h].reshape(h, w)))
    return pool


@pytest.mark.parametrize("shape", ic.TINY_SHAPES, ids=["8x8", "4x8", "8x4", "4x4"])
def test_tiny_group_tails(ctx, shape):
    """1, G - 1, G and G + 1 blocks of one tiny shape in a flush (G blocks share a workgroup): the last group's lanes without a block
    leave the picture alone, the blocks beside them are the reference's."""
    g = golden_io.load("itx.ovg")
    group, pool = ic.TINY_GROUP[shape], tiny_pool()[shape]
    assert len(pool) > group
    for n in (1, group - 1, group, group + 1):
        pic = start(g, n)
        cmds, arena, rects, exp = np.zeros(n, capi.TB_CMD_DTYPE), [], [], []
        for k, (c, co, want) in enumerate(pool[-n:]):                 # each block on a band of its own
            cmds[k] = c
            band = BAND if c["plane"] == 0 else BAND // 2
            cmds[k]["y"] = int(c["y"]) % band + k * band
            cmds[k]["coef_off"] = sum(len(a) for a in arena)
            rects.append((int(c["plane"]), int(c["x"]), int(cmds[k]["y"]), want.shape[1], want.shape[0], sum(e.size for e in exp)))
            arena.append(co); exp.append(want.ravel())
        assert (ic.body(cmds, "job") == ic.TINY).all()
        got = run_job(ctx, pic, cmds, np.concatenate(arena), np.zeros(0, capi.ITASK_DTYPE))
        check(pic, got, rects, np.concatenate(exp), f"{n} tiny blocks of shape {shape}")
