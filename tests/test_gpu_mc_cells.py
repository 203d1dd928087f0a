"""GPU: the enumerated inter prediction cells (tests/golden/mc_cells_*.ovg, mcx_cells_*.ovg; gen_mc_cells / gen_mcx_cells) through every route
that runs their units, bit-exact against the reference, every sample outside the PUs keeping the fill.

The cases of a file are dealt to sheets (mc_census.sheets: PUs that do not overlap), a sheet is one picture and one launch:
  plain units    "mc"     ovhip_mc_launch;
                 "job"    a picture job (engine.Job, STAGE_MC) recording the same PUs; sheets whose unit count is no multiple of 8 run
                          k_mc2's XCD slot order with a ragged tail;
                 "view"   the border family once more through a 208-wide view of 210-wide pictures (stride no multiple of 4 samples):
                          stage_unit_windows' slow path against the same expected samples;
  refined units  "mcx"    ovhip_mcx_launch, samples and refined vectors;
                 "mcxa"   ovhip_mcxa_launch with affine units of mca.ovg alongside (their pictures in further slots of the table);
                 "search" ovhip_dmvr_search_launch: the vectors equal k_mcx's and the reference's, the picture stays untouched -- also
                          on mcx.ovg;
                 "job"    a picture job recording the same PUs: its eager search (ovhip_job_dmvr_rows -> k_dmvr_search), then the flush
                          (k_mcxa), vectors after each;
  LMCS           the planes family once more with OVHIP_MC_LMCS set and a forward table of lmcs.ovg, against the oracle (the reference's
                 plain slots take no reshaper: no fixture of it).
  affine units   "view"   mca.ovg's CUs (not cells: the fixture of test_gpu_parity_golden) through ovhip_mca_launch on the same kind of
                          208-wide view: AffStage's per-sample path.
tests/mc_census.py labels the units; test_routes_run_every_cell_the_census_claims ties what the routes launched to its cells."""
import functools

import numpy as np
import pytest

import golden_cases
import mc_census as mc
from oracle_lib import HostPic
from openvvc_amd import capi, engine

pytestmark = pytest.mark.gpu
FILL = 0xABAB
MC_FILES = golden_cases.mc_cell_files()
MCX_FILES = golden_cases.mcx_cell_files()
BORDER_FILES = [f for f in MC_FILES if "_border_" in f]


@pytest.fixture(scope="module")
def ctx(built_lib):
    c = engine.Context(0)
    yield c
    c.close()


class Pool:
    """device buffers and pictures of one test, freed when it ends"""
    def __init__(self, ctx):
        self.ctx, self.items = ctx, []

    def buf(self, arr):
        self.items.append(self.ctx.upload(arr))
        return self.items[-1]

    def pic(self, pic):
        self.items.append(self.ctx.upload_pic(pic.y, pic.cb, pic.cr))
        return self.items[-1]

    def planes(self, y, cb, cr):
        self.items.append(self.ctx.upload_pic(y, cb, cr))
        return self.items[-1]


@pytest.fixture
def pool(ctx):
    p = Pool(ctx)
    yield p
    ctx.sync()
    for it in p.items:
        it.free()


def filled(w, h):
    pic = HostPic(w, h)
    pic.y[:] = FILL; pic.cb[:] = FILL; pic.cr[:] = FILL
    return pic


def same_picture(got, want, what):
    for name, a, b in zip("Y Cb Cr".split(), got, want.planes()):
        bad = np.argwhere(a != b)
        assert len(bad) == 0, f"{what}, plane {name}: {len(bad)} samples differ from the reference's picture, first at (y, x) {bad[:6].tolist()}"


@functools.lru_cache(maxsize=None)
def plain_plan(name):
    """-> (refs, intra, descs, [(cases, units, expected picture)] per sheet)"""
    refs, intra, descs, exp_off, exp, units = mc.plain_fixture(name)
    out = []
    for cases in mc.sheets(descs):
        want = set(cases)
        out.append((cases, np.array([u for i, u, _ in units if i in want], capi.MC_UNIT_DTYPE),
                    mc.expected_picture(descs, exp_off, exp, refs[0].w, refs[0].h, cases, FILL)))
    return refs, intra, descs, out


@functools.lru_cache(maxsize=None)
def refined_plan(name):
    """-> (refs, descs, [(cases, plain units, refined units, expected vectors, expected picture)] per sheet)"""
    refs, descs, exp_off, exp, exp_mv = golden_cases.mcx_cases(name)
    rec = mc.recorded(descs, refs[0].w, refs[0].h)
    out = []
    for cases in mc.sheets(descs):
        plain = np.concatenate([rec[i][1] for i in cases])
        refined = np.concatenate([rec[i][2] for i in cases])
        mv = np.concatenate([exp_mv[int(exp_off[i, 3]) // 4:int(exp_off[i, 3]) // 4 + len(rec[i][2])] for i in cases])
        out.append((cases, plain, refined, mv, mc.expected_picture(descs, exp_off, exp, refs[0].w, refs[0].h, cases, FILL)))
    return refs, descs, out


@pytest.mark.parametrize("name", MC_FILES)
def test_mc_cells_launch(ctx, pool, name):
    refs, intra, _, plan = plain_plan(name)
    drefs, dintra = [pool.pic(r) for r in refs], pool.pic(intra) if intra is not None else None
    for k, (_, units, want) in enumerate(plan):
        d = pool.pic(filled(want.w, want.h))
        ctx.mc(d, drefs, pool.buf(units), intra=dintra)
        ctx.sync()
        same_picture(d.download(), want, f"{name} sheet {k}, ovhip_mc_launch")


@pytest.mark.parametrize("name", MC_FILES)
def test_mc_cells_picture_job(ctx, pool, name):
    refs, intra, descs, plan = plain_plan(name)
    drefs, dintra = [pool.pic(r) for r in refs], pool.pic(intra) if intra is not None else None
    job = engine.Job(ctx, refs[0].w, refs[0].h)
    p = capi.JobParams()
    p.log2_ctu_s, p.stages = 7, capi.STAGE_MC
    assert any(len(units) % 8 and len(units) > 8 for _, units, _ in plan), "no sheet with a ragged XCD tail"
    for k, (cases, units, want) in enumerate(plan):
        job.begin()
        for i in cases:
            job.rec.pu(descs[i])
        assert job.rec.mc_units().tobytes() == units.tobytes()          # what the flush launches is what the census labelled
        d = pool.pic(filled(want.w, want.h))
        job.flush(d, drefs, dintra, params=p)
        job.wait()
        same_picture(d.download(), want, f"{name} sheet {k}, picture job")
    job.close()


@pytest.mark.parametrize("name", BORDER_FILES)
def test_mc_border_cells_slow_staging(ctx, pool, name):
    """the pictures are the left 208 columns of 210-wide ones (luma stride 210, chroma 105 samples): no aligned 8-byte groups, every
    window goes through issue_slow; the columns outside the view must come back untouched"""
    refs, _, _, plan = plain_plan(name)
    W, H = refs[0].w, refs[0].h
    rng = np.random.default_rng(5)

    def wide(pic):
        planes = []
        for k, p in enumerate(pic.planes()):
            big = rng.integers(0, 1024, (p.shape[0], p.shape[1] + (1 if k else 2)), dtype=np.uint16)
            big[:, :p.shape[1]] = p
            planes.append(big)
        d = pool.planes(*planes)
        assert (d.s.stride_y, d.s.stride_c) == (W + 2, W // 2 + 1)
        return d, planes, engine.DevPic(ctx, capi.Pic(d.s.y, d.s.cb, d.s.cr, W, H, d.s.stride_y, d.s.stride_c), owns=False)

    vrefs = [wide(r)[2] for r in refs]
    for k, (_, units, want) in enumerate(plan):
        assert all(w[2] == "slow" for u in units for w in mc.windows(u, W, H, W + 2, W // 2 + 1))
        d, start, view = wide(filled(W, H))
        ctx.mc(view, vrefs, pool.buf(units))
        ctx.sync()
        got = d.download()
        same_picture([g[:, :p.shape[1]] for g, p in zip(got, want.planes())], want, f"{name} sheet {k}, 208-wide view of 210")
        for g, s, p in zip(got, start, want.planes()):
            assert np.array_equal(g[:, p.shape[1]:], s[:, p.shape[1]:]), f"{name} sheet {k}: columns outside the view changed"


def test_mca_slow_staging(ctx, pool):
    """mca.ovg's affine CUs through ovhip_mca_launch with its 208x120 pictures as the left 208 columns of 210-wide ones (luma stride 210,
    chroma 105 samples): neither plane has aligned 8-byte groups, so every window of every unit, luma 9x9 and chroma 7x7, is fetched
    sample by sample.  The fixture's expected samples do not depend on the stride; the columns outside the view must come back untouched."""
    refs, cases, exp_off, exp = golden_cases.mca_cases()
    W, H, n = refs[0].w, refs[0].h, len(cases)
    rng = np.random.default_rng(6)

    def wide(planes):
        big = []
        for k, p in enumerate(planes):
            b = rng.integers(0, 1024, (p.shape[0], p.shape[1] + (1 if k else 2)), dtype=np.uint16)
            b[:, :p.shape[1]] = p
            big.append(b)
        d = pool.planes(*big)
        return d, big, engine.DevPic(ctx, capi.Pic(d.s.y, d.s.cb, d.s.cr, W, planes[0].shape[0], d.s.stride_y, d.s.stride_c), owns=False)

    vrefs = [wide(r.planes())[2] for r in refs]
    fill = np.full((H * n, W), FILL, np.uint16)
    d, start, tall = wide((fill, fill[:H * n // 2, :W // 2], fill[:H * n // 2, :W // 2]))
    for v in vrefs + [tall]:
        assert (v.s.stride_y | v.s.w) & 3 and (v.s.stride_c | (v.s.w >> 1)) & 3, "a plane is back on the aligned staging path"
    rec = capi.Recorder(W, H)
    rects, n_units = [], 0
    for i, (c, mv0, mv1) in enumerate(cases):
        rec.reset()
        rec.affine_cu(c, mv0, mv1)
        ctx.mca(tall.band(i * H, H), vrefs, pool.buf(rec.aff_units()), pool.buf(rec.aff_side()))
        n_units += len(rec.aff_units())
        w, h = 1 << c.log2_w, 1 << c.log2_h
        rects += [(0, c.x0, c.y0 + i * H, w, h, int(exp_off[i, 0])),
                  (1, c.x0 >> 1, (c.y0 >> 1) + i * (H // 2), w >> 1, h >> 1, int(exp_off[i, 1])),
                  (2, c.x0 >> 1, (c.y0 >> 1) + i * (H // 2), w >> 1, h >> 1, int(exp_off[i, 2]))]
    ctx.sync()
    assert n_units >= len(cases) > 0
    got = d.download()
    golden_cases.check_rects(HostPic(W, H * n, *[g[:, :W >> (k != 0)] for k, g in enumerate(got)]), rects, exp, "mca HIP, 208-wide view of 210")
    for k, (g, s) in enumerate(zip(got, start)):
        assert np.array_equal(g[:, W >> (k != 0):], s[:, W >> (k != 0):]), f"plane {k}: columns outside the view changed"


def run_refined(ctx, pool, drefs, plain, refined, w, h, route, extra=None):
    """-> (planes, vectors) of one sheet through ovhip_mcx_launch or ovhip_mcxa_launch (extra = (affine units, side arena))"""
    d = pool.pic(filled(w, h))
    if len(plain):
        ctx.mc(d, drefs, pool.buf(plain))
    mv = pool.buf(np.full((len(refined), 4), 0x5a5a5a5a, np.int32))
    if route == "mcx":
        ctx.mcx(d, drefs, pool.buf(refined), mv_out=mv)
    else:
        ctx.mcxa(d, drefs, pool.buf(refined), pool.buf(extra[0]), pool.buf(extra[1]), mv_out=mv)
    ctx.sync()
    return d.download(), mv.download(np.int32).reshape(-1, 4)


@pytest.mark.parametrize("name", MCX_FILES)
def test_mcx_cells_launch(ctx, pool, name):
    refs, _, plan = refined_plan(name)
    drefs = [pool.pic(r) for r in refs]
    for k, (_, plain, refined, want_mv, want) in enumerate(plan):
        got, mv = run_refined(ctx, pool, drefs, plain, refined, want.w, want.h, "mcx")
        assert np.array_equal(mv, want_mv), f"{name} sheet {k}: refined vectors differ from the reference's"
        same_picture(got, want, f"{name} sheet {k}, ovhip_mcx_launch")


@functools.lru_cache(maxsize=None)
def affine_beside(rects):
    """affine CUs of mca.ovg that do not touch the rectangles `rects` (nor each other), their reference slots moved past the refined
    units' three -> (units, side arena, [(x, y, w, h, expected planes)], mca.ovg's reference pictures)"""
    refs, cases, exp_off, exp = golden_cases.mca_cases()
    rec = capi.Recorder(refs[0].w, refs[0].h)
    taken, out = list(rects), []
    for i, (d, mv0, mv1) in enumerate(cases):
        w, h = 1 << d.log2_w, 1 << d.log2_h
        r = (d.x0, d.y0, d.x0 + w, d.y0 + h)
        if len(out) < 11 and all(r[2] <= q[0] or q[2] <= r[0] or r[3] <= q[1] or q[3] <= r[1] for q in taken):
            d.ref0 += 3; d.ref1 += 3
            rec.affine_cu(d, mv0, mv1)
            taken.append(r)
            e = [exp[int(exp_off[i, p]):int(exp_off[i, p]) + (w >> (p != 0)) * (h >> (p != 0))].reshape(h >> (p != 0), w >> (p != 0)) for p in range(3)]
            out.append((d.x0, d.y0, w, h, e))
    return rec.aff_units().copy(), rec.aff_side().copy(), out, refs


@pytest.mark.parametrize("name", MCX_FILES)
def test_mcx_cells_fused_with_affine(ctx, pool, name):
    """k_mcxa's split: the first workgroups take the affine units, the others the refined ones"""
    refs, descs, plan = refined_plan(name)
    n_aff, drefs = 0, None
    for k, (cases, plain, refined, want_mv, want) in enumerate(plan):
        rects = tuple((descs[i].x0, descs[i].y0, descs[i].x0 + (1 << descs[i].log2_w), descs[i].y0 + (1 << descs[i].log2_h)) for i in cases)
        aunits, side, blocks, arefs = affine_beside(rects)
        assert len(aunits) >= 4, f"{name} sheet {k}: no room for affine CUs beside it, the sheet would not run the fused launch's split"
        drefs = drefs or [pool.pic(r) for r in refs + arefs]
        got, mv = run_refined(ctx, pool, drefs, plain, refined, want.w, want.h, "mcxa", (aunits, side))
        both = HostPic(want.w, want.h, want.y.copy(), want.cb.copy(), want.cr.copy())
        for x, y, w, h, e in blocks:
            for p, plane in enumerate(both.planes()):
                c = p != 0
                plane[y >> c:(y + h) >> c, x >> c:(x + w) >> c] = e[p]
        assert np.array_equal(mv, want_mv), f"{name} sheet {k}: refined vectors differ from the reference's"
        same_picture(got, both, f"{name} sheet {k}, ovhip_mcxa_launch with {len(aunits)} affine units")
        n_aff += len(aunits)
    assert n_aff > 8


@pytest.mark.parametrize("name", ["mcx.ovg"] + MCX_FILES)
def test_dmvr_search_equals_the_fused_refinement(ctx, pool, name):
    """k_dmvr_search (the SEARCH_ONLY instantiation) on the same units as k_mcx: the same vectors for every DMVR unit (= the reference's),
    the entries of the BDOF-only units left alone, nothing written to the picture"""
    refs, _, plan = refined_plan(name)
    drefs = [pool.pic(r) for r in refs]
    n_dmvr = 0
    for k, (_, plain, refined, want_mv, want) in enumerate(plan):
        _, mv_mcx = run_refined(ctx, pool, drefs, plain[:0], refined, want.w, want.h, "mcx")
        d = pool.pic(filled(want.w, want.h))
        mv = pool.buf(np.full((len(refined), 4), 0x5a5a5a5a, np.int32))
        ctx.dmvr_search(d, drefs, pool.buf(refined), mv)
        ctx.sync()
        got = mv.download(np.int32).reshape(-1, 4)
        dm = (refined["flags"] & capi.MC_DMVR) != 0
        assert np.array_equal(got[dm], mv_mcx[dm]) and np.array_equal(got[dm], want_mv[dm]), f"{name} sheet {k}: the search's vectors differ"
        assert (got[~dm] == 0x5a5a5a5a).all(), f"{name} sheet {k}: the search wrote the entry of a unit without DMVR"
        same_picture(d.download(), filled(want.w, want.h), f"{name} sheet {k}: the search wrote to the picture")
        n_dmvr += int(dm.sum())
    assert n_dmvr == (728 if name == "mcx.ovg" else len(refined_plan(name)[1]))        # every unit of the cell files is a DMVR unit


@pytest.mark.parametrize("name", MCX_FILES)
def test_mcx_cells_picture_job(ctx, pool, name):
    """the refined units as a picture job runs them: the eager search over the recorded units (ovhip_job_dmvr_rows: k_dmvr_search)
    leaves the reference's vectors before anything is predicted, the flush (k_mcxa) the same vectors and the reference's samples"""
    refs, descs, plan = refined_plan(name)
    drefs = [pool.pic(r) for r in refs]
    job = engine.Job(ctx, refs[0].w, refs[0].h)
    p = capi.JobParams()
    p.log2_ctu_s, p.stages = 7, capi.STAGE_MC
    for k, (cases, plain, refined, want_mv, want) in enumerate(plan):
        job.begin()
        for i in cases:
            job.rec.pu(descs[i])
        assert job.rec.mcx_units().tobytes() == refined.tobytes() and job.rec.mc_units().tobytes() == plain.tobytes()
        assert job.dmvr_rows(drefs) == len(refined)
        assert np.array_equal(job.refined_mvs()[:len(refined)], want_mv), f"{name} sheet {k}: the job's eager search differs from the reference's vectors"
        d = pool.pic(filled(want.w, want.h))
        job.flush(d, drefs, None, params=p)
        job.wait()
        assert np.array_equal(job.refined_mvs(), want_mv), f"{name} sheet {k}: the flush's vectors differ from the reference's"
        same_picture(d.download(), want, f"{name} sheet {k}, picture job")
    job.close()


def test_mc_planes_cells_with_lmcs(ctx, pool):
    """OVHIP_MC_LMCS on the units of the planes family (every shape, lists and plane set): k_mc2's three luma finish bodies map the
    combined sample through the forward table, chroma stays.  Expected samples from the oracle (equal to the reference on these units
    without the flag; its table step is one lookup), the table one lmcs.ovg's reference built."""
    import oracle_lib
    name = [f for f in MC_FILES if "_planes_" in f][0]
    refs, _, _, plan = plain_plan(name)
    _, sets, _, _ = golden_cases.lmcs_cases()
    fwd = np.frombuffer(bytes(capi.lmcs_build(sets[1][0])), np.uint16)[:1024].copy()
    assert len(np.unique(fwd)) > 100 and (fwd != np.arange(1024)).any()
    drefs = [pool.pic(r) for r in refs]
    for k, (_, units, plain_want) in enumerate(plan):
        units = units.copy()
        units["flags"] |= capi.MC_LMCS
        want = filled(plain_want.w, plain_want.h)
        oracle_lib.mc(want, refs, units, lmcs_fwd=fwd)
        assert (want.y != plain_want.y).any() and np.array_equal(want.cb, plain_want.cb) and np.array_equal(want.cr, plain_want.cr)
        d = pool.pic(filled(want.w, want.h))
        ctx.mc(d, drefs, pool.buf(units), lmcs_fwd=pool.buf(fwd))
        ctx.sync()
        same_picture(d.download(), want, f"{name} sheet {k} with LMCS, ovhip_mc_launch against the oracle")
    luma = [lb for _, us, _ in plan for lb in (mc.label_plain(u, want.w, want.h) for u in us) if lb["planes"] != "no luma"]
    assert {(lb["nout_l"], lb["lists"]) for lb in luma} == {(n, ls) for n in (1, 2, 4) for ls in ("L0", "L1", "BI")}


def test_routes_run_every_cell_the_census_claims():
    """Over the routes above every cell tests/mc_census.py claims was launched (test_mc_fixture_census asserts what those are).  This test
    launches nothing; it labels the units the plans above hand to the launches.  What ties the labels to the device: the "mc" and
    "view" routes upload exactly the plan's units, the "job" route asserts its recorder's units equal them byte for byte, the refined
    routes upload the units mc_census.recorded() took from Recorder.pu().  Which path a window takes inside stage_unit_windows, and which
    finish body a shape takes, is read off the source, not observed on the device: if they change, mc_census has to follow."""
    W, H = 208, 120
    per_route = {"mc": [], "view": []}
    for name in MC_FILES:
        units = [u for _, us, _ in plain_plan(name)[3] for u in us]
        per_route["mc"] += [mc.label_plain(u, W, H) for u in units]
        if name in BORDER_FILES:
            per_route["view"] += [mc.label_plain(u, W, H, W + 2, W // 2 + 1) for u in units]
    r = mc.reach_plain(per_route["mc"])                                   # "mc" and "job" launch the same units
    assert r["phase"] == mc.phase_cells_that_exist() and r["combine"] == mc.combine_cells_that_exist()
    assert r["planes"] == mc.plane_cells_that_exist() and r["border"] == mc.border_cells_that_exist(W, H)
    assert r["path"] == {"interior", "clamped"} and len(r["nout"]) == 9
    # issue_slow parks every window at offset 0: the offset within the aligned group means nothing on that route
    v = mc.reach_plain(per_route["view"])
    assert {c[:3] for c in v["border"]} == {c[:3] for c in mc.border_cells_that_exist(W, H)} and v["path"] == {"slow"}
    refined = [lb for f in MCX_FILES for _, _, lb in mc.refined_fixture(f)[5]]        # "mcx", "mcxa" and "search" launch all of them
    assert sum(len(p[2]) for f in MCX_FILES for p in refined_plan(f)[2]) == len(refined)
    assert {(lb["shape"], lb["bdof"], l, s) for lb in refined for l, s in lb["clip"]} == {(sh, b, l, s) for sh in ((8, 16), (16, 8), (16, 16))
                                                                                        for b in (False, True) for l in (0, 1) for s in "LRTB"}
    assert {e for lb in refined for e in lb["at_limit"] - lb["ini_at_limit"]} == {(k, hi) for k in range(4) for hi in (False, True)}
    rd, cells = mc.reach_dmvr(refined), mc.dmvr_cells_that_exist()         # DMVR's outcome: every cell, from the cell files alone
    assert all(rd[k] == cells[k] for k in cells)
    rr, rc = mc.reach_refined(refined), mc.refined_cells_that_exist()      # steps 3 and 4: displacements, apron reads, BDOF
    assert rr["disp_l"] == rc["disp_l"] and rr["disp_c"] == rc["disp_c"] and rr["apron"] == rc["apron"] and rr["bdof"] == rc["bdof"]
    with_bdof = mc.reach_refined([lb for _, _, lb in mc.refined_fixture("mcx.ovg")[5]] + refined)       # BDOF-only units: mcx.ovg ("search" route, and the parity test)
    assert with_bdof["flags"] == rc["flags"]
