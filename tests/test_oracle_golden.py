"""CPU: the oracle restatement + the host recorder reproduce the compiled reference bit-exactly
on the committed golden fixtures (tests/golden/*.ovg, made by oracle/ref_harness/gen_golden.c from
the reference's own rcn_tu_st / rcn_tu_c / rcn_mcp_b* slots)."""
import numpy as np
import pytest

import golden_cases
import oracle_lib
from oracle_lib import HostPic
from openvvc_amd import capi


def test_itx_oracle_matches_reference(built_lib):
    pic, cmds, coefs, rects, exp = golden_cases.itx_cases()
    assert len(cmds) > 400
    oracle_lib.itx(pic, cmds, coefs)
    golden_cases.check_rects(pic, rects, exp, "itx oracle vs reference")


def test_transform_tree_oracle_matches_reference(built_lib):
    """tmp.rcn_transform_tree: CUs up to 128x128 cut at the maximum transform size, one TUInfo per leaf."""
    pic, cmds, coefs, rects, exp = golden_cases.tt_cases()
    assert len(rects) == 36 and len(cmds) > 60
    oracle_lib.itx(pic, cmds, coefs)
    golden_cases.check_rects(pic, rects, exp, "transform tree oracle vs reference")


def test_mc_oracle_matches_reference(built_lib):
    refs, descs, exp_off, exp = golden_cases.mc_cases()
    rw, rh = refs[0].w, refs[0].h
    rec = capi.Recorder(rw, rh)
    for i, d in enumerate(descs):
        rec.reset()
        rec.pu(d)
        dst = HostPic(rw, rh)
        dst.y[:] = 0xABAB; dst.cb[:] = 0xABAB; dst.cr[:] = 0xABAB
        oracle_lib.mc(dst, refs, rec.mc_units())
        w, h = 1 << d.log2_w, 1 << d.log2_h
        rects = [(0, d.x0, d.y0, w, h, int(exp_off[i, 0])),
                 (1, d.x0 >> 1, d.y0 >> 1, w >> 1, h >> 1, int(exp_off[i, 1])),
                 (2, d.x0 >> 1, d.y0 >> 1, w >> 1, h >> 1, int(exp_off[i, 2]))]
        golden_cases.check_rects(dst, rects, exp, f"mc case {i} dir={d.inter_dir} planes={d.planes}")


def test_mcx_oracle_matches_reference(built_lib):
    """BDOF (rcn_bdof_mcp_l + rcn_mcp_b_c) and DMVR (rcn_dmvr_mv_refine, incl. the MV write-back)."""
    refs, descs, exp_off, exp, exp_mv = golden_cases.mcx_cases()
    rw, rh = refs[0].w, refs[0].h
    rec = capi.Recorder(rw, rh)
    n_moved = n_bdof = 0
    for i, d in enumerate(descs):
        rec.reset()
        rec.pu(d)
        dst = HostPic(rw, rh)
        dst.y[:] = 0xABAB; dst.cb[:] = 0xABAB; dst.cr[:] = 0xABAB
        ux = rec.mcx_units()
        oracle_lib.mc(dst, refs, rec.mc_units())
        mv = oracle_lib.mc_ex(dst, refs, ux)
        w, h = 1 << d.log2_w, 1 << d.log2_h
        rects = [(0, d.x0, d.y0, w, h, int(exp_off[i, 0])),
                 (1, d.x0 >> 1, d.y0 >> 1, w >> 1, h >> 1, int(exp_off[i, 1])),
                 (2, d.x0 >> 1, d.y0 >> 1, w >> 1, h >> 1, int(exp_off[i, 2]))]
        golden_cases.check_rects(dst, rects, exp, f"mcx case {i} refine={d.refine} {w}x{h} @({d.x0},{d.y0})")
        if d.refine & capi.PU_DMVR:
            want = exp_mv[int(exp_off[i, 3]) // 4:int(exp_off[i, 3]) // 4 + len(ux)]
            assert np.array_equal(mv, want), f"mcx case {i}: refined MVs differ {mv.tolist()} vs {want.tolist()}"
            n_moved += int((mv != np.array([d.mv0x, d.mv0y, d.mv1x, d.mv1y])).any(axis=1).sum())
        else:
            n_bdof += len(ux)
    assert n_moved > 100 and n_bdof > 100, "fixture does not exercise DMVR / BDOF"


def test_mca_oracle_matches_reference(built_lib):
    """Affine sub-block MC + PROF (rcn_mcp_b_l(2,2) / rcn_prof_mcp_b_l / rcn_mcp_b_c(3,3))."""
    refs, cases, exp_off, exp = golden_cases.mca_cases()
    rw, rh = refs[0].w, refs[0].h
    rec = capi.Recorder(rw, rh)
    n_prof = 0
    for i, (d, mv0, mv1) in enumerate(cases):
        rec.reset()
        rec.affine_cu(d, mv0, mv1)
        dst = HostPic(rw, rh)
        dst.y[:] = 0xABAB; dst.cb[:] = 0xABAB; dst.cr[:] = 0xABAB
        oracle_lib.mca(dst, refs, rec.aff_units(), rec.aff_side())
        w, h = 1 << d.log2_w, 1 << d.log2_h
        rects = [(0, d.x0, d.y0, w, h, int(exp_off[i, 0])),
                 (1, d.x0 >> 1, d.y0 >> 1, w >> 1, h >> 1, int(exp_off[i, 1])),
                 (2, d.x0 >> 1, d.y0 >> 1, w >> 1, h >> 1, int(exp_off[i, 2]))]
        golden_cases.check_rects(dst, rects, exp, f"mca case {i} dir={d.inter_dir} prof={d.prof_dir} {w}x{h} @({d.x0},{d.y0})")
        n_prof += d.prof_dir != 0
    assert n_prof > 100


def test_lmcs_host_tables_and_oracle_match_reference(built_lib):
    """K11: ovhip_lmcs_build (host) == rcn_init_lmcs; oracle chroma scale == rcn_lmcs_compute_chroma_scale;
    oracle inverse map == lmcs_reshape_backward."""
    pic_y, sets, regions, inverse = golden_cases.lmcs_cases()
    h, w = pic_y.shape
    rec = capi.Recorder(w, h)
    n_inv = 0
    for si, (data, want) in enumerate(sets):
        got = capi.lmcs_build(data)
        assert bytes(got) == bytes(want), f"LMCS tables of set {si} differ"
        rows = regions[regions[:, 0] == si]
        rec.reset()
        for r in rows:
            rec.lmcs_region(int(r[1]), int(r[2]), int(r[3]), int(r[4]))
        pic = HostPic(w, h, pic_y.copy())
        scales = oracle_lib.lmcs_scale(pic, rec.lmcs_regions(), got)
        assert np.array_equal(scales, rows[:, 5].astype(np.int16)), f"chroma scales of set {si}: {scales.tolist()} vs {rows[:, 5].tolist()}"
        if si % 6 == 1:
            oracle_lib.lmcs_inverse(pic, np.frombuffer(bytes(got), np.uint16)[1024:2048])
            exp = np.concatenate([inverse[n_inv, 0], inverse[n_inv, 1]], axis=1)
            assert np.array_equal(pic.y, exp), f"inverse map of set {si} differs"
            n_inv += 1
    assert n_inv == len(inverse) and len(np.unique(regions[:, 5])) > 10


def test_gpm_ciip_oracle_matches_reference(built_lib):
    """K10: geometric partitioning (rcn_gpm_b, all 64 partition indices) and the CIIP blend (rcn_ciip / rcn_ciip_b)."""
    refs, intra, descs, modes, n_gpm, exp_off, exp = golden_cases.gpm_cases()
    _, first_planar = golden_cases.ciip_planar_cases()        # from there on: CIIP through ordered planar tasks (test_shim_cpu)
    descs = descs[:first_planar]
    rw, rh = refs[0].w, refs[0].h
    rec = capi.Recorder(rw, rh)
    for i, d in enumerate(descs):
        rec.reset()
        rec.pu(d)
        dst = HostPic(rw, rh)
        dst.y[:] = 0xABAB; dst.cb[:] = 0xABAB; dst.cr[:] = 0xABAB
        oracle_lib.mc(dst, refs, rec.mc_units())
        if i >= n_gpm:
            rec.ciip(d.x0, d.y0, d.log2_w, d.log2_h, int(modes[i, 0]), int(modes[i, 1]))
            oracle_lib.ciip(dst, intra, rec.ciip_units())
        w, h = 1 << d.log2_w, 1 << d.log2_h
        rects = [(0, d.x0, d.y0, w, h, int(exp_off[i, 0])),
                 (1, d.x0 >> 1, d.y0 >> 1, w >> 1, h >> 1, int(exp_off[i, 1])),
                 (2, d.x0 >> 1, d.y0 >> 1, w >> 1, h >> 1, int(exp_off[i, 2]))]
        what = f"GPM split {d.gpm_split_dir}" if i < n_gpm else f"CIIP modes {modes[i].tolist()} dir {d.inter_dir}"
        golden_cases.check_rects(dst, rects, exp, f"case {i} {what} {w}x{h} @({d.x0},{d.y0})")
        if i >= n_gpm:
            # second route: the blend fused into the prediction units (ovhip_pu_desc.ciip_wt)
            d.ciip_wt = capi.load().ovhip_ciip_weight(int(modes[i, 0]), int(modes[i, 1]))
            rec.reset()
            rec.pu(d)
            assert len(rec.ciip_units()) == 0 and (rec.mc_units()["aux"] != 0).all()
            dst = HostPic(rw, rh)
            oracle_lib.mc(dst, refs, rec.mc_units(), intra=intra)
            golden_cases.check_rects(dst, rects, exp, f"case {i} fused {what} {w}x{h}")
            d.ciip_wt = 0
    assert n_gpm >= 192 and len(descs) - n_gpm >= 100


def test_dbf_oracle_matches_reference(built_lib):
    cases = golden_cases.dbf_cases()
    assert len(cases) == 3
    for i, (pic, planes, exp) in enumerate(cases):
        work = pic.copy()
        oracle_lib.dbf(work, planes)
        for name, a, b, c in (("Y", work.y, exp.y, pic.y), ("Cb", work.cb, exp.cb, pic.cb), ("Cr", work.cr, exp.cr, pic.cr)):
            assert (b != c).sum() > 500, "fixture does not exercise the filter"
            bad = np.argwhere(a != b)
            assert len(bad) == 0, f"dbf picture {i} plane {name}: {len(bad)} samples differ, first at (y,x) {bad[:6].tolist()}"


def test_dbf_edge_lists_equal_compacted_planes(built_lib):
    """The edge lists ovhip_rec_dbf_ctu emits CTU by CTU (what ovhip_job_flush uploads) hold exactly the segments
    ovhip_dbf_compact extracts from the dense planes the reference-pinned oracle test consumes."""
    for i, (_, planes, _) in enumerate(golden_cases.dbf_cases()):
        for d in (0, 1):
            direct, offs = planes["edges"][d]
            compact = capi.dbf_compact(planes, d)
            key = lambda a: sorted(zip(a["comp"].tolist(), a["uy"].tolist(), a["ux"].tolist(), a["word"].tolist()))
            assert key(direct) == key(compact), f"picture {i} dir {d}"
            assert len(direct) > 100 and (direct["pad"] == 0).all()
            assert offs.beta[0] == planes["beta_offset"] and offs.tc[0] == planes["tc_offset"]


def test_sao_oracle_matches_reference(built_lib):
    cases = golden_cases.sao_cases()
    assert len(cases) == 3
    for i, (pic, prm, exp) in enumerate(cases):
        out = HostPic(pic.w, pic.h)
        oracle_lib.sao(out, pic, prm)
        for name, a, b, c in (("Y", out.y, exp.y, pic.y), ("Cb", out.cb, exp.cb, pic.cb), ("Cr", out.cr, exp.cr, pic.cr)):
            assert (b != c).sum() > 20, "fixture does not exercise SAO"
            bad = np.argwhere(a != b)
            assert len(bad) == 0, f"sao picture {i} plane {name}: {len(bad)} samples differ, first at (y,x) {bad[:6].tolist()}"


def test_alf_oracle_matches_reference(built_lib):
    cases = golden_cases.alf_cases()
    assert len(cases) == 3
    for i, (pic, alf, exp) in enumerate(cases):
        out = HostPic(pic.w, pic.h)
        oracle_lib.alf(out, pic, alf)
        for name, a, b, c in (("Y", out.y, exp.y, pic.y), ("Cb", out.cb, exp.cb, pic.cb), ("Cr", out.cr, exp.cr, pic.cr)):
            assert (b != c).sum() > 100, "fixture does not exercise ALF"
            bad = np.argwhere(a != b)
            assert len(bad) == 0, f"alf picture {i} plane {name}: {len(bad)} samples differ, first at (y,x) {bad[:6].tolist()}"


# (file, log2_ctu, picture sizes): three full CTU rows and a truncated one, a second ragged picture, a single truncated CTU row, a single
# row of exactly one CTU; no width (luma or chroma) is a multiple of the CTU, the SAO tile (64) or the ALF tile (32)
SAO_SMALL_CTU = (("sao_ctu64.ovg", 6, [(304, 200), (200, 136), (136, 56), (136, 64)]),
                 ("sao_ctu32.ovg", 5, [(152, 104), (104, 64), (72, 24), (72, 32)]))
ALF_SMALL_CTU = (("alf_ctu64.ovg", 6, [(304, 200), (200, 128), (136, 56), (136, 64)]),
                 ("alf_ctu32.ovg", 5, [(152, 104), (104, 64), (72, 24), (72, 32)]))


@pytest.mark.parametrize("name,log2_ctu,sizes", SAO_SMALL_CTU, ids=["ctu64", "ctu32"])
def test_sao_oracle_matches_reference_small_ctu(built_lib, name, log2_ctu, sizes):
    """The reference's SAO slots run with 64- and 32-sample CTUs (rcn_sao_first_pix_rows / rcn_sao_filter_line)."""
    cases = golden_cases.sao_cases(name)
    assert [(p.w, p.h) for p, _, _ in cases] == sizes
    for i, (pic, prm, exp) in enumerate(cases):
        ctu = 1 << log2_ctu
        assert len(prm) == -(-pic.w // ctu) * -(-pic.h // ctu)
        out = HostPic(pic.w, pic.h)
        oracle_lib.sao(out, pic, prm, log2_ctu)
        for name_, a, b, c in (("Y", out.y, exp.y, pic.y), ("Cb", out.cb, exp.cb, pic.cb), ("Cr", out.cr, exp.cr, pic.cr)):
            assert (b != c).sum() > 20, "fixture does not exercise SAO"
            bad = np.argwhere(a != b)
            assert len(bad) == 0, f"{name} picture {i} plane {name_}: {len(bad)} samples differ, first at (y,x) {bad[:6].tolist()}"


@pytest.mark.parametrize("name,log2_ctu,sizes", ALF_SMALL_CTU, ids=["ctu64", "ctu32"])
def test_alf_oracle_matches_reference_small_ctu(built_lib, name, log2_ctu, sizes):
    """The reference's rcn_alf_filter_line with 64- and 32-sample CTUs (virtual boundary at CTU row ctu - 4, chroma ctu / 2 - 2)."""
    cases = golden_cases.alf_cases(name)
    assert [(p.w, p.h) for p, _, _ in cases] == sizes
    for i, (pic, alf, exp) in enumerate(cases):
        ctu = 1 << log2_ctu
        assert len(alf["ctus"]) == -(-pic.w // ctu) * -(-pic.h // ctu)
        out = HostPic(pic.w, pic.h)
        oracle_lib.alf(out, pic, alf, log2_ctu)
        for name_, a, b, c in (("Y", out.y, exp.y, pic.y), ("Cb", out.cb, exp.cb, pic.cb), ("Cr", out.cr, exp.cr, pic.cr)):
            assert (b != c).sum() > 100, "fixture does not exercise ALF"
            bad = np.argwhere(a != b)
            assert len(bad) == 0, f"{name} picture {i} plane {name_}: {len(bad)} samples differ, first at (y,x) {bad[:6].tolist()}"


# ---------------------------------------------------------------------------------------------- SAO and ALF: census and enumerated cells
_OLD_SAO = {"sao.ovg": 7, "sao_ctu64.ovg": 6, "sao_ctu32.ovg": 5}
_OLD_ALF = {"alf.ovg": 7, "alf_ctu64.ovg": 6, "alf_ctu32.ovg": 5}
_filter_labels = {}


def _filter_census(name):
    """[(input, parameters, the reference's picture, the census's restated picture, its labels)] per picture of a SAO or ALF fixture,
    computed once for all the tests below"""
    import filter_census as fc
    if name not in _filter_labels:
        is_sao = name.startswith("sao")
        l2 = (_OLD_SAO | _OLD_ALF)[name] if name in _OLD_SAO | _OLD_ALF else golden_cases.filter_cell_ctu(name)
        cases = golden_cases.sao_cases(name) if is_sao else golden_cases.alf_cases(name)
        _filter_labels[name] = [(pic, prm, exp) + (fc.sao if is_sao else fc.alf)(pic, prm, l2) for pic, prm, exp in cases], l2
    return _filter_labels[name]


def _family(files, fam):
    return [f for f in files if f.split("_")[2] == fam]


def test_sao_and_alf_oracle_match_reference_on_the_enumerated_cells(built_lib):
    """sao_cells_*.ovg / alf_cells_*.ovg (gen_sao_cells / gen_alf_cells: the reference's rcn_sao_first_pix_rows / rcn_sao_filter_line and
    rcn_alf_filter_line, in the entry family once per rect entry with that entry's RectEntryInfo): the oracle equals the reference on
    every picture, at the CTU size the file was generated at."""
    import golden_io
    sf, af = golden_cases.sao_cell_files(), golden_cases.alf_cell_files()
    assert {f.split("_")[2] for f in sf} == {"sao", "sao64", "sao32", "entry64"} and {f.split("_")[2] for f in af} == {"class", "class64", "edge", "taps", "entry64"}
    assert all((golden_io.GOLDEN / f).stat().st_size < (1 << 20) for f in sf + af)
    for f in sf + af:
        l2 = golden_cases.filter_cell_ctu(f)
        (pic, prm, exp), = golden_cases.sao_cases(f) if f in sf else golden_cases.alf_cases(f)
        out = HostPic(pic.w, pic.h)
        (oracle_lib.sao if f in sf else oracle_lib.alf)(out, pic, prm, l2)
        _same_picture(out, exp, f"{f} (CTU {1 << l2}): oracle")
        assert all((a != b).sum() > 100 for a, b in zip(exp.planes(), pic.planes())), f


def test_filter_census_restates_the_reference(built_lib):
    """tests/filter_census.py's numpy restatements of SAO and ALF -- written from rcn_sao.c and rcn_alf.c, with the virtual boundary, the
    single-CTU-row quirks and the rect-entry borders -- equal the reference's expected planes on EVERY SAO and ALF fixture, old and new:
    what makes the labels below trustworthy, since a label only comes out of the functions that computed these planes."""
    n = 0
    for f in list(_OLD_SAO) + list(_OLD_ALF) + golden_cases.sao_cell_files() + golden_cases.alf_cell_files():
        cases, l2 = _filter_census(f)
        for i, (_, _, exp, got, _) in enumerate(cases):
            _same_picture(got, exp, f"{f} picture {i} (CTU {1 << l2}): census restatement")
            n += 1
    assert n == 11 + 11 + len(golden_cases.sao_cell_files()) + len(golden_cases.alf_cell_files())


def test_sao_fixture_census(built_lib):
    """What the SAO slot fixtures reach of what k_sao decides, per plane (tests/filter_census.py; cells reached of cells that exist).

    sao.ovg alone: band positions with a sample in one of the four bands 17 of 105 (32 positions a plane, 29..31 also with the `& 31` wrap
    acting); (edge class, sign of either comparison) 86 of 108; (band / edge, clip at 0 / at 1023) 7 of 12; group positions 0 and 7 under
    the horizontal and the diagonal classes 14 of 18; skip reasons 8 of 18.  A comparison with an equal neighbour is 1.4 to 3.7 % of the
    filtered edge samples of a plane, both equal at most 0.08 %.
    With sao_ctu64.ovg and sao_ctu32.ovg: band positions 50 of 105, sign pairs 106 of 108, clips 8 of 12, skip reasons 9 of 18 -- the
    three reasons that take a rect entry's border on every plane are out of their reach, every ovhip_sao_ctu.border being 0.
    The enumerated cells reach every cell, the families at CTU 128 / 64 / 32 between them; on its own each CTU size reaches what depends
    on the CTU size: a neighbour in another CTU, the picture's border columns and rows, all nine sign pairs of every class."""
    import filter_census as fc
    ex = fc.sao_cells_that_exist()
    count = lambda r: {k: len(r[k] & ex[k]) for k in ex}
    assert {k: len(v) for k, v in ex.items()} == {"type": 9, "band_k": 15, "band_pos": 105, "edge": 108, "clip": 12, "skip": 18, "group": 18, "across": 9}
    labels = lambda files: [lb for f in files for case in _filter_census(f)[0] for lb in case[4]]
    r = fc.sao_reach(labels(["sao.ovg"]))
    assert count(r) == {"type": 9, "band_k": 15, "band_pos": 17, "edge": 86, "clip": 7, "skip": 8, "group": 14, "across": 9}
    eq = [(((lb["sa"] == 0) | (lb["sb"] == 0))[lb["run"]].mean(), ((lb["sa"] == 0) & (lb["sb"] == 0))[lb["run"]].mean()) for lb in labels(["sao.ovg"]) if lb["run"].any()]
    assert 0.013 < min(e for e, _ in eq) and max(e for e, _ in eq) < 0.038 and max(b for _, b in eq) < 0.0009
    r = fc.sao_reach(labels(_OLD_SAO))
    assert count(r) == {"type": 9, "band_k": 15, "band_pos": 50, "edge": 106, "clip": 8, "skip": 9, "group": 18, "across": 9}
    assert ex["skip"] - r["skip"] == {(p, why) for p in range(3) for why in ("entry column", "entry row", "BORDER_ONE_ROW")}
    assert not any(prm["border"].any() for f in _OLD_SAO for _, prm, _, _, _ in _filter_census(f)[0])

    # ---- the enumerated cells
    files = golden_cases.sao_cell_files()
    r = fc.sao_reach(labels(files))
    for k in ex:
        assert r[k] == ex[k], f"SAO {k} cells without a case: {sorted(ex[k] - r[k], key=str)[:8]}"
    for fam in ("sao", "sao64", "sao32"):
        r = fc.sao_reach(labels(_family(files, fam)))
        assert r["edge"] == ex["edge"] and r["across"] == ex["across"] and r["group"] == ex["group"] and r["band_k"] == ex["band_k"], fam
        assert {(p, why) for p in range(3) for why in ("picture column", "picture row")} <= r["skip"], fam
    assert fc.sao_reach(labels(_family(files, "sao32")))["band_pos"] == ex["band_pos"]
    # the rect entries: every border bit on a CTU whose three planes have an edge class on; the three reasons on every plane
    (_, prm, _, _, lbs), = _filter_census("sao_cells_entry64_00.ovg")[0]
    edge_on = (prm["type"] == fc.SAO_EDGE).all(axis=1)
    for bit in (capi.BORDER_LEFT, capi.BORDER_RIGHT, capi.BORDER_UPPER, capi.BORDER_BOTTOM, capi.BORDER_ONE_ROW):
        assert ((prm["border"] & bit) != 0)[edge_on].any(), bit
    assert {(p, why) for p in range(3) for why in ("entry column", "entry row", "BORDER_ONE_ROW")} <= fc.sao_reach(lbs)["skip"]
    # pictures with a ragged last group of 8 on every plane, a truncated last CTU row, a single CTU row
    sizes = [(c[0].w, c[0].h, _filter_census(f)[1]) for f in files for c in _filter_census(f)[0]]
    assert any(w % 8 and (w // 2) % 8 and h % (1 << l2) for w, h, l2 in sizes) and any(h <= 1 << l2 for w, h, l2 in sizes)
    # the load and store paths: in an allocation whose strides are multiples of 8 samples the full groups go 16 bytes at a time, in
    # one as wide as the picture (no width here is a multiple of 8) or two samples wider (tests/test_gpu_filter_cells.py) sample by sample
    for w, h, l2 in sizes:
        ragged = {(p, "ragged") for p in range(3) if (w >> (p > 0)) % 8}
        assert len(ragged) >= 2 and fc.sao_paths(w, h, (w + 15) & ~15, ((w + 15) & ~15) // 2) == {(p, "16-byte") for p in range(3)} | ragged
        assert fc.sao_paths(w, h, w, w // 2) == fc.sao_paths(w, h, w + 2, w // 2 + 1) == {(p, "scalar") for p in range(3)} | ragged


def test_alf_fixture_census(built_lib):
    """What the ALF slot fixtures reach of what k_alf decides (tests/filter_census.py; cells reached of cells that exist).  A 4x4 luma
    block counts for its (class, transpose) pair only if it discriminates: the filter of each other transpose of its class, of the
    class one step away in activity and of the class one step away in direction gives another 4x4 block, from the picture's own tables.

    alf.ovg alone: 5924 luma blocks, 5737 of them in class 4; 8 of the 25 classes and 19 of the 100 (class, transpose) pairs occur, 18
    with a block that discriminates, 13 with four; act 6 and 8..15 only; luma sets 7 of 18; no luma tap is ever clipped (every luma set
    in use is linear: (tap, clip index, state) 12 of 120, waves linear alone); chroma taps 12 of 120; chroma alternatives 6 of 16; none
    of the 16 sums next to an activity threshold; ties 2 of 5; no all-zero block; max_db * min_hv at most 1.1e8 of 2^32.
    With alf_ctu64.ovg and alf_ctu32.ovg: 11136 blocks, 10596 in class 4, 27 pairs, 25 that discriminate, 18 with four; act 3..15; sets
    15 of 18; luma taps 120 of 120, chroma taps 84 of 120, waves linear and clipping but never mixed; thresholds 0 of 16; ties 3 of 5.
    The enumerated cells: see the assertions per family below."""
    import filter_census as fc
    ex = fc.alf_cells_that_exist()
    count = lambda r: {k: len(r[k] & ex[k]) for k in ex}
    labels = lambda files: [case[4] for f in files for case in _filter_census(f)[0]]
    blocks = lambda lbs, key: np.concatenate([L["blocks"][key][L["blocks"]["on"]] for L in lbs])
    assert {k: len(v) for k, v in ex.items()} == {"pair": 100, "set": 18, "act": 32, "ties": 5, "luma_tap": 120, "chroma_tap": 120, "wave": 3, "clip": 6, "alt": 16,
                                                  "cc": 10, "cc_row": 6, "cc_clip": 8, "flags": 8, "d": 24, "thresholds": 16}
    lbs = labels(["alf.ovg"])
    r = fc.alf_reach(lbs)
    assert count(r) == {"pair": 18, "set": 7, "act": 15, "ties": 2, "luma_tap": 12, "chroma_tap": 12, "wave": 1, "clip": 6, "alt": 6, "cc": 8, "cc_row": 6,
                        "cc_clip": 6, "flags": 7, "d": 24, "thresholds": 0}
    cls, tr = blocks(lbs, "cls"), blocks(lbs, "tr")
    assert (len(cls), int((cls == 4).sum()), sorted(set(cls.tolist())), len(set(zip(cls.tolist(), tr.tolist())))) == (5924, 5737, [2, 3, 4, 8, 9, 18, 19, 24], 19)
    assert sum(v >= 4 for v in r["pair_n"].values()) == 13 and sorted({a for a, _ in r["act"]}) == [6, 8, 9, 10, 11, 12, 13, 14, 15]
    assert not r["all_zero"] and r["max_cross"] < 1.2e8 and r["wave"] == {"linear"}
    lbs = labels(_OLD_ALF)
    r = fc.alf_reach(lbs)
    assert count(r) == {"pair": 25, "set": 15, "act": 25, "ties": 3, "luma_tap": 120, "chroma_tap": 84, "wave": 2, "clip": 6, "alt": 8, "cc": 10, "cc_row": 6,
                        "cc_clip": 7, "flags": 8, "d": 24, "thresholds": 0}
    cls, tr = blocks(lbs, "cls"), blocks(lbs, "tr")
    assert (len(cls), int((cls == 4).sum()), len(set(zip(cls.tolist(), tr.tolist())))) == (11136, 10596, 27)
    assert sum(v >= 4 for v in r["pair_n"].values()) == 18 and r["wave"] == {"linear", "clipping"} and not r["all_zero"]
    assert not any(t["ctus"]["border"].any() for f in _OLD_ALF for _, t, _, _, _ in _filter_census(f)[0])

    files = golden_cases.alf_cell_files()
    # ---- class: all 100 pairs by at least 4 discriminating blocks on a fixed set and again on an APS set; every luma_set on a CTU that
    # is on; among the blocks at a virtual boundary every activity class, direction class and transpose
    lbs = labels(_family(files, "class"))
    for kind in ("fixed", "aps"):
        n = fc.alf_reach(lbs, kind)["pair_n"]
        thin = sorted(p for p in ex["pair"] if n.get(p, 0) < 4)
        assert not thin, f"(class, transpose) with fewer than 4 discriminating blocks on a {kind} set: {[(p, n.get(p, 0)) for p in thin[:8]]}"
    r = fc.alf_reach(lbs + labels(_family(files, "class64")))
    assert r["set"] == ex["set"] and (r["vb_actc"], r["vb_dirc"], r["vb_tr"]) == (set(range(5)), set(range(5)), set(range(4)))
    r = fc.alf_reach(lbs)
    assert (r["vb_actc"], r["vb_dirc"], r["vb_tr"]) == (set(range(5)), set(range(5)), set(range(4))) and len(r["set"]) == 16
    # (the picture regenerated at CTU 64, 150000 draws: as measured)
    assert len(fc.alf_reach(labels(_family(files, "class64")))["pair"]) == 93
    # ---- edge: every act on plain blocks and on blocks at a virtual boundary, both sides of each activity threshold exactly, each of
    # the five ties with non-zero sums, the all-zero block, the largest sums: 65472^2 = 2^32 - 8384512
    r = fc.alf_reach(labels(_family(files, "edge")))
    assert r["act"] == ex["act"] and r["thresholds"] == ex["thresholds"] and r["ties"] == ex["ties"] and r["all_zero"]
    assert r["max_cross"] == 65472 ** 2 == (1 << 32) - 8384512
    # ---- taps
    r = fc.alf_reach(labels(_family(files, "taps")))
    for k in ("luma_tap", "chroma_tap", "wave", "clip", "alt", "cc", "cc_row", "cc_clip", "flags", "d"):
        assert r[k] == ex[k], f"ALF {k} cells without a case in the taps family: {sorted(ex[k] - r[k], key=str)[:8]}"
    for f in _family(files, "taps"):
        (_, t, _, _, _), = _filter_census(f)[0]
        assert {-128, 127} <= set(np.asarray(t["luma_coeff"])[16:18].ravel().tolist()) and {-128, 127} <= set(np.asarray(t["chroma_coeff"]).ravel().tolist())
    # ---- entry: every border bit on a CTU with luma, both chroma planes and both CC-ALF filters on
    (_, t, _, _, L), = _filter_census("alf_cells_entry64_00.ovg")[0]
    c = t["ctus"]
    full = (c["flags"] == 7) & (c["cc_cb_idx"] > 0) & (c["cc_cr_idx"] > 0)
    for bit in (capi.BORDER_LEFT, capi.BORDER_RIGHT, capi.BORDER_UPPER, capi.BORDER_BOTTOM, capi.BORDER_ONE_ROW):
        assert ((c["border"] & bit) != 0)[full].any(), bit
    paths, sides = fc.alf_paths(L["w"], L["h"], L["w"], L["w"] // 2, t, 6)
    assert {s for s in sides if any(s)} >= {(True, False, False, False), (False, True, False, False), (False, False, True, False), (False, False, False, True)}
    # at least one picture per family has a width that is no multiple of 64 in luma or chroma and a truncated last CTU row
    for fam in ("class", "edge", "taps"):
        assert any(c[0].w % 64 and c[0].h % 128 for f in _family(files, fam) for c in _filter_census(f)[0]), fam


def test_fixtures_regenerate_from_the_compiled_reference(tmp_path):
    """Where the compiled reference is available (this container: oracle/_ref built from /root/reference),
    re-running the harness reproduces every committed fixture byte for byte."""
    import subprocess
    from pathlib import Path
    import pytest
    root = Path(__file__).resolve().parent.parent
    gen = root / "oracle" / "_ref" / "gen_golden"
    if not gen.exists() or not (root / "oracle" / "_ref" / "libovvcref.so").exists():
        pytest.skip("compiled reference not present")
    subprocess.check_call([str(gen), str(tmp_path)], stderr=subprocess.DEVNULL)
    for only in ("dbf_ends", "sao_ctu64", "sao_ctu32", "alf_ctu64", "alf_ctu32", "intra_cells", "itx_cells", "mc_cells", "mcx_cells", "sao_cells", "alf_cells"):        # deblocking's second profile, the smaller CTU sizes and the enumerated intra / inverse transform / inter prediction / SAO / ALF cells are runs of their own
        subprocess.check_call([str(gen), str(tmp_path), only], stderr=subprocess.DEVNULL)
    # shim_*: test_shim_cpu.py; pipe* / tiles*: the chained streams of gen_pipe, test_pipe_cpu.py
    names = sorted(p.name for p in (root / "tests" / "golden").glob("*.ovg") if not p.name.startswith(("shim_", "pipe", "tiles")))
    assert len(names) >= 14
    for n in names:
        assert (tmp_path / n).read_bytes() == (root / "tests" / "golden" / n).read_bytes(), f"{n} differs from a fresh run of the reference"
    assert sorted(p.name for p in tmp_path.glob("intra_cells_*.ovg")) == [n for n in names if n.startswith("intra_cells_")], "the generator cuts the intra cells into other files than the committed ones"
    assert sorted(p.name for p in tmp_path.glob("itx_cells_*.ovg")) == [n for n in names if n.startswith("itx_cells_")], "the generator cuts the inverse transform cells into other files than the committed ones"
    assert sorted(p.name for p in tmp_path.glob("mc_cells_*.ovg")) == [n for n in names if n.startswith("mc_cells_")], "the generator cuts the plain prediction cells into other files than the committed ones"
    assert sorted(p.name for p in tmp_path.glob("mcx_cells_*.ovg")) == [n for n in names if n.startswith("mcx_cells_")], "the generator cuts the refined prediction cells into other files than the committed ones"
    assert sorted(p.name for p in tmp_path.glob("sao_cells_*.ovg")) == [n for n in names if n.startswith("sao_cells_")], "the generator cuts the SAO cells into other files than the committed ones"
    assert sorted(p.name for p in tmp_path.glob("alf_cells_*.ovg")) == [n for n in names if n.startswith("alf_cells_")], "the generator cuts the ALF cells into other files than the committed ones"


def test_intra_oracle_matches_reference(built_lib):
    """Intra prediction: the reference's intra_pred / intra_pred_mrl / mip.rcn_intra_mip / intra_pred_c (+ cclm.*) slots vs the oracle's
    ordered-task executor on intra.ovg: every block shape, but for blocks of 512 samples or more every third or fifth mode only (every
    other MIP matrix from 1024), and ONE availability pattern per case, drawn at random; every MRL case has both arms and the corner.
    test_intra_fixture_census pins what that reaches; the cells it does not reach are intra_cells_*.ovg
    (test_intra_oracle_matches_reference_on_the_enumerated_cells)."""
    import golden_io
    g = golden_io.load("intra.ovg")
    tasks = np.frombuffer(g["task"].tobytes(), dtype=capi.ITASK_DTYPE)
    H, W = g["pic_y"].shape
    kinds = {"luma": 0, "mrl": 0, "mip": 0, "chroma": 0, "lm": 0, "bdpcm": 0}
    bad = []
    for i, t in enumerate(tasks):
        pic = HostPic(W, H, g["pic_y"].copy(), g["pic_cb"].copy(), g["pic_cr"].copy())
        oracle_lib.intra_tasks(pic, tasks[i:i + 1])
        w, h, x, y = 1 << int(t["log2_w"]), 1 << int(t["log2_h"]), int(t["x"]), int(t["y"])
        eo = g["exp_off"][i]
        if t["kind"] == capi.IT_LUMA:
            ok = np.array_equal(pic.y[y:y + h, x:x + w], g["exp"][eo[0]:eo[0] + w * h].reshape(h, w))
        else:
            ok = (np.array_equal(pic.cb[y:y + h, x:x + w], g["exp"][eo[0]:eo[0] + w * h].reshape(h, w))
                  and np.array_equal(pic.cr[y:y + h, x:x + w], g["exp"][eo[1]:eo[1] + w * h].reshape(h, w)))
        fl = int(t["flags"])
        k = ("mip" if fl & capi.IF_MIP else "bdpcm" if fl & capi.IF_BDPCM else "mrl" if t["mrl_idx"] else
             "lm" if t["mode"] >= 67 else "luma" if t["kind"] == capi.IT_LUMA else "chroma")
        kinds[k] += 1
        if not ok:
            bad.append((i, k, int(t["mode"]), w, h, x, y, fl, int(t["avl_lft"]), int(t["avl_abv"])))
    assert not bad, f"{len(bad)} / {len(tasks)} intra cases differ from the reference, first: {bad[:6]}"
    assert kinds["luma"] > 2500 and kinds["mrl"] > 500 and kinds["mip"] > 200 and kinds["chroma"] > 1000 and kinds["lm"] > 200 and kinds["bdpcm"] > 50


def test_intra_oracle_matches_reference_on_the_enumerated_cells(built_lib):
    """intra_cells_*.ovg (gen_intra_cells: the (shape, mode) cells intra.ovg thins out, every availability class per kind and shape,
    MRL at a left edge), same slots and picture as intra.ovg: the oracle equals the reference on every case."""
    import golden_io
    import intra_cases
    import intra_census as ic
    tasks, exp_off, exp, pic = intra_cases.load("cells")
    assert len(tasks) > 2500 and all((golden_io.GOLDEN / n).stat().st_size < (1 << 20) for n in intra_cases.cell_files())
    bad = [intra_cases.describe(i, t) for i, t in enumerate(tasks)
           if not ic.blocks_equal(ic.expected_block(t, exp_off[i], exp), ic.oracle_block(pic, t))]
    assert not bad, f"{len(bad)} / {len(tasks)} enumerated intra cases differ from the reference, first: {bad[:6]}"


def test_intra_fixture_census(built_lib):
    """What the intra slot fixtures reach, written down so that it cannot shrink unnoticed (tests/intra_census.py does the counting).

    intra.ovg alone -- thinned modes for big blocks, one random availability pattern per case:
      (shape, mode) cells: luma regular 1251 of 1675 (the 10 shapes of >= 512 samples have 19 or 27 of 67 modes), MRL 979 of 1675 (19 of
      25 shapes have 19 to 39 modes), chroma regular 1488 of 1608 (16x32, 32x16, 32x32: 27 modes), MIP 320 of the 356 (shape, matrix,
      transposed) cells; luma regular (shape, mode, class): 2297 of 8375; all 979 MRL cases have both arms and the corner; 696 cases
      span several 256-sample strips of the flow launch, 132 several 1024-sample strips of the level launch; 90 of the 1335 luma
      regular cases without full availability predict exactly what full availability predicts (the missing arm is not read).
    With intra_cells_*.ovg, conditions (a) to (d) below hold.  Not reachable, by what the operations read: MIP and LM / MDLM never read
    the corner sample, so their "both without the corner" cases equal full availability -- asserted as such; MRL without the rows
    above is left out (the reference reads memory nothing wrote there)."""
    import collections
    import intra_cases
    import intra_census as ic
    tasks, exp_off, exp, pic = intra_cases.load("intra.ovg")
    lb = ic.label(tasks)
    big = {s for s in ic.LUMA_SHAPES if s[0] + s[1] >= 9}
    n_modes = ic.modes_per_shape(lb, ic.LUMA)
    assert len(ic.cells(lb, ic.LUMA, "shape", "mode")) == 1251 and len(big) == 10
    assert all(n_modes[s] in (19, 27) for s in big) and all(n_modes[s] == 67 for s in set(ic.LUMA_SHAPES) - big)
    n_modes = ic.modes_per_shape(lb, ic.MRL)
    assert len(ic.cells(lb, ic.MRL, "shape", "mode")) == 979
    assert sorted(n for n in n_modes.values() if n < 67)[::18] == [19, 39] and sum(n < 67 for n in n_modes.values()) == 19
    n_modes = ic.modes_per_shape(lb, ic.CHROMA)
    assert len(ic.cells(lb, ic.CHROMA, "shape", "mode")) == 1488 and {s: n for s, n in n_modes.items() if n < 67} == {(4, 5): 27, (5, 4): 27, (5, 5): 27}
    assert len(ic.mip_cells()) == 356 and len(ic.cells(lb, ic.MIP, "shape", "mode", "tr")) == 320
    assert len(ic.cells(lb, ic.LUMA, "shape", "mode", "cls")) == 2297
    assert ic.cells(lb, ic.MRL, "cls") == {(4,)} and int((lb["kind"] == ic.MRL).sum()) == 979
    assert int((lb["samples"] > 256).sum()) == 696 and int((lb["samples"] > 1024).sum()) == 132
    sel = np.nonzero((lb["kind"] == ic.LUMA) & (lb["cls"] != 4))[0]
    assert len(sel) == 1335 and int((~ic.sensitive(tasks, exp_off, exp, pic, sel)).sum()) == 90

    # ---- both fixtures together
    tc, eoc, expc, _ = intra_cases.load("cells")
    n0 = len(tasks)
    tasks, exp_off, exp = np.concatenate([tasks, tc]), np.concatenate([exp_off, eoc + len(exp)]), np.concatenate([exp, expc])
    lb = ic.label(tasks)
    # (a) every (shape, mode): luma regular 25 x 0..66, chroma regular 24 x 0..66, MRL 25 x 1..66, MIP every (shape, matrix, transposed)
    assert ic.cells(lb, ic.LUMA, "shape", "mode") == {(s, m) for s in ic.LUMA_SHAPES for m in range(67)}
    assert ic.cells(lb, ic.CHROMA, "shape", "mode") == {(s, m) for s in ic.CHROMA_SHAPES for m in range(67)}
    assert ic.cells(lb, ic.MRL, "shape", "mode") >= {(s, m) for s in ic.LUMA_SHAPES for m in range(1, 67)}
    assert ic.cells(lb, ic.MIP, "shape", "mode", "tr") == ic.mip_cells()
    # (b) every (kind, shape, class); every (mode, class) of luma regular and chroma regular
    for kind, shapes in ((ic.LUMA, ic.LUMA_SHAPES), (ic.CHROMA, ic.CHROMA_SHAPES), (ic.MIP, ic.LUMA_SHAPES), (ic.LM, ic.CHROMA_SHAPES)):
        assert ic.cells(lb, kind, "shape", "cls") == {(s, c) for s in shapes for c in range(5)}, ic.KIND_NAMES[kind]
    for kind in (ic.LUMA, ic.CHROMA):
        assert ic.cells(lb, kind, "mode", "cls") == {(m, c) for m in range(67) for c in range(5)}, ic.KIND_NAMES[kind]
    assert ic.cells(lb, ic.LM, "mode") == {(67,), (68,), (69,)}
    # (c) MRL: every shape at a left edge (no left arm, no corner, rows above), every shape with both indices
    assert {s for s, c in ic.cells(lb, ic.MRL, "shape", "cls") if c == 1} == set(ic.LUMA_SHAPES)
    assert ic.cells(lb, ic.MRL, "shape", "mrl") == {(s, m) for s in ic.LUMA_SHAPES for m in (1, 2)}
    assert {c for (c,) in ic.cells(lb, ic.MRL, "cls")} == {1, 4}, "MRL without the rows above has no defined result in the reference"
    # (d) every (kind, shape, class != both with corner) has a case that full availability would predict differently
    sel = np.nonzero((lb["cls"] != 4) & (lb["kind"] != ic.BDPCM))[0]
    sens = ic.sensitive(tasks, exp_off, exp, pic, sel)
    triples = collections.defaultdict(list)
    for k, i in enumerate(sel):
        triples[(int(lb["kind"][i]), (int(lb["l2w"][i]), int(lb["l2h"][i])), int(lb["cls"][i]))].append(bool(sens[k]))
    no_corner_read = {t for t in triples if t[0] in (ic.MIP, ic.LM) and t[2] == 3}            # neither reads the corner sample
    assert len(triples) == 4 * (25 + 24 + 25 + 24) + 25 and len(no_corner_read) == 25 + 24
    dull = sorted(t for t, v in triples.items() if not any(v) and t not in no_corner_read)
    assert not dull, f"(kind, shape, class) without a case that pins the availability logic: {dull[:8]}"
    assert not any(any(triples[t]) for t in no_corner_read), "a MIP or LM case reads the corner sample?"
    # (a figure, not a condition: the (mode, class) pairs hold modes that do not read the missing arm, and planar never reads the corner)
    new = sel >= n0
    print(f"enumerated cases without full availability that predict what full availability predicts: {int((new & ~sens).sum())} of {int(new.sum())}")


def test_itx_oracle_matches_reference_on_the_enumerated_cells(built_lib):
    """itx_cells_*.ovg (gen_itx_cells: transform pairs, extents, LFNST, de-quantisation, BDPCM, DC, sinks and the mixed quads, on itx.ovg's
    picture and through the same slots): the oracle equals the reference on every block of every file."""
    import golden_io
    files = golden_cases.itx_cell_files()
    assert {f.split("_")[2] for f in files} == {"tr", "ext", "lfnst", "dq", "bdpcm", "dc", "sink", "quad"}
    assert all((golden_io.GOLDEN / f).stat().st_size < (1 << 20) for f in files)
    n = 0
    for f in files:
        pic, cmds, coefs, rects, exp = golden_cases.itx_cases(f)
        oracle_lib.itx(pic, cmds, coefs)
        golden_cases.check_rects(pic, rects, exp, f"{f}: oracle vs reference")
        n += len(cmds)
    assert n > 3500


def test_itx_fixture_census(built_lib):
    """What the inverse transform slot fixtures reach, written down so that it cannot shrink unnoticed (tests/itx_census.py does the
    counting, and asserts its restatement of the recorder's split against the recorder on every file).

    itx.ovg alone, on the routes it had (every block four-wave; the picture job) -- cells reached of cells that exist:
      plain luma transform blocks (body, shape, transform pair): four-wave 64 of 101, specialised 27 of 69, tiny 14 of 20;
      LFNST (set, index, transposed, size class): 28 of 56 (no 4x4 block with set 0, 2 or 3 at index 0, ...);
      (shape, nb_row, nb_col) of the one-wave shapes: specialised 29 of 97, tiny 8 of 9;
      de-quantisation classes (scale, table, dq_neg, dq_shift) of the enumerated QP range: 169 of 186;
      sink modes without STORE (first plane, mode, second plane's mode, scale on): 25 of 25, but the scale within 1200..3400 of the
      256..16384 the reference can derive.
    With itx_cells_*.ovg on the three routes every one of these cells has a case."""
    import itx_census as ic
    cmds, _ = ic.load(["itx.ovg"])
    r = ic.reach(cmds, ("itx", "job"))
    tr, ext = ic.tr_cells_that_exist(), ic.extent_cells_that_exist()
    per_body = lambda cells, b: {c for c in cells if c[0] == b}
    assert [len(per_body(tr, b)) for b in (ic.FOUR, ic.SPEC, ic.TINY)] == [101, 69, 20]
    assert [len(per_body(r["tr"] & tr, b)) for b in (ic.FOUR, ic.SPEC, ic.TINY)] == [64, 27, 14] and r["tr"] <= tr
    assert len(ic.lfnst_cells_that_exist()) == 56 and len(r["lfnst"]) == 28 and r["lfnst"] <= ic.lfnst_cells_that_exist()
    assert len(ext) == 97 and len({c[1:] for c in per_body(r["extent"], ic.SPEC)} & ext) == 29
    assert len({c[1:] for c in per_body(r["extent"], ic.TINY)} & ext) == 8
    assert len(ic.dq_cells_that_exist()) == 186 and len(r["dq"] & ic.dq_cells_that_exist()) == 169
    assert len(ic.sink_cells_that_exist()) == 25 and r["sink"] == ic.sink_cells_that_exist()
    scales = cmds["c_scale"][(cmds["res_mode"] & capi.RES_SCALE) != 0]
    assert 1200 <= scales.min() and scales.max() <= 3400

    # ---- with the enumerated cells, on the three routes
    cmds, _ = ic.load(["itx.ovg"] + golden_cases.itx_cell_files())
    r = ic.reach(cmds)
    assert r["tr"] == tr, f"(body, shape, transform pair) without a case: {sorted(tr - r['tr'])[:8]}"
    lf = ic.lfnst_cells_that_exist()
    assert r["lfnst"] == lf and r["lfnst_body"] == {(b, c) for c in lf for b in ((ic.FOUR,) if c[3] != "larger" else ()) + (ic.FOUR, ic.GENERIC)}
    for b in (ic.FOUR, ic.SPEC):
        assert {c[1:] for c in per_body(r["extent"], b)} >= ext, ic.BODY_NAMES[b]
    assert {c[1:] for c in per_body(r["extent"], ic.TINY)} == {c for c in ext if c[0] in ic.TINY_SHAPES}
    assert r["dq"] >= ic.dq_cells_that_exist() and r["sink"] >= ic.sink_cells_that_exist()
    # the chroma scale at both ends of what the reference derives, (1 << 17) / (8 .. 511), on every scaled sink mode
    for end in (256, 16384):
        at_end = ic.label(cmds[((cmds["res_mode"] & capi.RES_SCALE) != 0) & (cmds["c_scale"] == end)])["sink"]
        assert set(at_end) == {c for c in ic.sink_cells_that_exist() if c[4]}, end
    # transform-skip blocks whose levels are final (TS residual coding), raster: 16x16 in the one-wave generic body, 32x16 four-wave
    raw = {c[:2] for c in r["body_cells"] if c[3] == ic.K_TS_RAW}
    assert {(ic.GENERIC, (2, 2)), (ic.GENERIC, (3, 2)), (ic.GENERIC, (4, 4)), (ic.FOUR, (4, 4)), (ic.FOUR, (5, 4))} <= raw
    # every kind in every body that can take it: DC and raster DC in the one-wave shortcut, transform skip / BDPCM / raster blocks in the generic body
    kinds = {(ic.BODY_NAMES[b], k, l) for b, k, l in r["kind_body"]}
    assert {("one-wave DC", "DC", True), ("one-wave DC", "DC", False), ("one-wave DC", "raster DC", False), ("tiny", "DC", True), ("tiny", "DC", False),
            ("one-wave generic", "raster TR", False)} <= kinds
    assert {(ic.BODY_NAMES[b], k, l) for b in (ic.FOUR, ic.GENERIC) for k in ("TS", "TS_RAW", "BDPCM horizontal", "BDPCM vertical") for l in (True, False)} <= kinds


def test_itx_cells_discriminate(built_lib):
    """The enumerated cells pin what they are named after: the oracle (equal to the reference on every block, above) reconstructs ANOTHER
    block when the command is edited -- transform pair: tr_h and tr_v swapped (where they differ), DST-VII replaced by DCT-VIII, DCT-II /
    DCT-II by DST-VII / DST-VII (no side above 32); LFNST: every other (set, index, transposed); extent: the outermost significant sub-block
    cleared (maps of more than one sub-block); de-quantisation: the class of QP - 1 and of QP + 1.  No cell may fail to."""
    import golden_io
    import itx_census as ic
    g = golden_io.load("itx.ovg")
    pred = (g["pred_y"], g["pred_cb"], g["pred_cr"])
    dull, n = [], 0

    def cases(prefix):
        for f in golden_cases.itx_cell_files():
            if f.startswith(prefix):
                _, rec, n_cmds, _, _ = golden_cases.itx_cases_rec(f)
                gg = golden_io.load(f)
                cmds, coefs, k = rec.tb_cmds().copy(), rec.coefs().copy(), 0
                for i, m in enumerate(n_cmds):
                    for c in cmds[k:k + m]:
                        yield f, i, c, coefs, capi.TuState.from_buffer_copy(gg["state"][i].tobytes()), capi.TuDesc.from_buffer_copy(gg["desc"][i].tobytes())
                    k += m

    for f, i, c, coefs, _, _ in cases("itx_cells_tr_"):
        v, h = int(c["tr_v"]), int(c["tr_h"])
        edits = [(h, v)] if v != h and max(c["log2_w"], c["log2_h"]) <= 5 else []      # (a side of 64 has DCT-II alone)
        if capi.DST_VII in (v, h):
            edits.append(tuple(capi.DCT_VIII if t == capi.DST_VII else t for t in (v, h)))
        if (v, h) == (capi.DCT_II, capi.DCT_II) and max(c["log2_w"], c["log2_h"]) <= 5:
            edits.append((capi.DST_VII, capi.DST_VII))
        for ev, eh in edits:
            n += 1
            if not ic.changes(pred, c, coefs, tr_v=ev, tr_h=eh):
                dull.append((f, i, "pair", (v, h), (ev, eh)))
    n_tr = n
    for f, i, c, coefs, _, _ in cases("itx_cells_lfnst_"):
        for field in range(16):
            other = 1 | (field << 1)
            if other != int(c["lfnst"]):
                n += 1
                if not ic.changes(pred, c, coefs, lfnst=other):
                    dull.append((f, i, "lfnst", int(c["lfnst"]), other))
    n_lf = n - n_tr
    for f, i, c, coefs, _, _ in cases("itx_cells_ext_"):
        m = int(c["sig_sb_map"])
        if m & (m - 1):
            n += 1
            if not ic.changes(pred, c, coefs, sig_sb_map=m & ~(1 << (m.bit_length() - 1))):
                dull.append((f, i, "extent", hex(m)))
    n_ext = n - n_tr - n_lf
    for f, i, c, coefs, st, d in cases("itx_cells_dq_"):
        if (int(c["kind"]) & 0x3f) == capi.TB_TS_RAW:
            continue                                      # TS residual coding: the levels are final, there is no QP in the command
        ts = bool(d.tr_skip_mask & 0x10)
        kind, qp, l2s = (2, st.qp_y_skip, 4) if ts else (int(st.dep_quant), st.qp_y, int(c["log2_w"]) + int(c["log2_h"]))
        assert ic.derive_dq(kind, qp, l2s) == (int(c["dq_scale"]), 0 if ts else l2s & 1, int(c["dq_neg"]), int(c["dq_shift"]))
        for q in (qp - 1, qp + 1):
            if 0 <= q <= 75:
                scale, _, neg, shift = ic.derive_dq(kind, q, l2s)
                # a transform-skip block adds the de-quantised level itself to the sample: where both classes take the level 1 to 1023 or
                # more, every sample with a level ends at a picture clip under both -- no block can tell them apart
                if ts and min(scale << shift if neg else 0, int(c["dq_scale"]) << int(c["dq_shift"]) if c["dq_neg"] else 0) >= 1023:
                    continue
                n += 1
                if not ic.changes(pred, c, coefs, dq_scale=scale, dq_neg=neg, dq_shift=shift):
                    dull.append((f, i, "dq", kind, qp, q))
    print(f"edits: {n_tr} transform pairs, {n_lf} LFNST, {n_ext} extents, {n - n_tr - n_lf - n_ext} de-quantisation classes; without effect: {len(dull)}")
    assert n_tr > 100 and n_lf == 512 * 15 and n_ext > 100 and n - n_tr - n_lf - n_ext > 1500
    assert not dull, f"{len(dull)} of {n} edits leave the block as it is, first: {dull[:8]}"


def _filled(w, h, fill=0xABAB):
    pic = HostPic(w, h)
    pic.y[:] = fill; pic.cb[:] = fill; pic.cr[:] = fill
    return pic


def _same_picture(got, want, what):
    for name, a, b in zip("Y Cb Cr".split(), got.planes(), want.planes()):
        bad = np.argwhere(a != b)
        assert len(bad) == 0, f"{what}, plane {name}: {len(bad)} samples differ from the reference's picture, first at (y, x) {bad[:6].tolist()}"


def test_mc_oracle_matches_reference_on_the_enumerated_cells(built_lib):
    """mc_cells_*.ovg (gen_mc_cells: phases, combines, planes, windows across and beyond every border; the reference's rcn_mcp_b / _l / _c,
    rcn_gpm_b, rcn_ciip / rcn_ciip_b): the oracle equals the reference on every case -- over the WHOLE picture: the cases run sheet by
    sheet (PUs that do not overlap) into a filled picture, and every sample outside the PUs keeps the fill, as the generator checked the
    reference's CTU buffer does."""
    import golden_io
    import mc_census as mc
    files = golden_cases.mc_cell_files()
    assert {f.split("_")[2] for f in files} == {"phase", "combine", "planes", "border"}
    assert all((golden_io.GOLDEN / f).stat().st_size < (1 << 20) for f in files)
    n = 0
    for f in files:
        refs, intra, descs, exp_off, exp, units = mc.plain_fixture(f)
        for k, cases in enumerate(mc.sheets(descs)):
            dst = _filled(refs[0].w, refs[0].h)
            want = set(cases)
            oracle_lib.mc(dst, refs, np.array([u for i, u, _ in units if i in want], capi.MC_UNIT_DTYPE), intra=intra)
            _same_picture(dst, mc.expected_picture(descs, exp_off, exp, refs[0].w, refs[0].h, cases), f"{f} sheet {k}")
        n += len(descs)
    assert n > 2000


def test_mcx_oracle_matches_reference_on_the_enumerated_cells(built_lib):
    """mcx_cells_*.ovg (gen_mcx_cells: rcn_dmvr_mv_refine with initial vectors beyond clip_mv's range on every side, and next to the
    +-2^17 limits): samples over the whole picture and the refined vectors."""
    import golden_io
    import mc_census as mc
    files = golden_cases.mcx_cell_files()
    assert {f.split("_")[2] for f in files} == {"far", "limit", "paint"}
    assert all((golden_io.GOLDEN / f).stat().st_size < (1 << 20) for f in files)
    for f in files:
        refs, descs, exp_off, exp, exp_mv, units = mc.refined_fixture(f)
        assert len(units) == len(descs) == len(exp_mv)           # a PU is one unit
        for k, cases in enumerate(mc.sheets(descs)):
            dst = _filled(refs[0].w, refs[0].h)
            mv = oracle_lib.mc_ex(dst, refs, np.array([units[i][1] for i in cases], capi.MC_UNIT_DTYPE))
            assert np.array_equal(mv, exp_mv[cases]), f"{f} sheet {k}: refined vectors differ from the reference's"
            _same_picture(dst, mc.expected_picture(descs, exp_off, exp, refs[0].w, refs[0].h, cases), f"{f} sheet {k}")


def test_mc_fixture_census(built_lib):
    """What the inter prediction slot fixtures reach, written down so that it cannot shrink unnoticed (tests/mc_census.py does the
    counting from the units Recorder.pu() cuts, and asserts its restatement of that cut against the recorder on every plain PU).

    mc.ovg alone (750 random draws -> 1912 plain units, 4814 reference windows, 2415 of them luma) -- cells reached of cells that exist:
      phase cells (pass, plane, shape, lists, list, phase; the luma phase is the tap row, 16 = half-pel): 1637 of 3520.  Keyed as the
        issue counted them: luma H (shape, list, fx) 234 of 288, luma V (shape, fy) 142 of 144 + 8 half-pel, chroma H (shape, list, fx
        of 32) 345 of 576, chroma V (shape, fy) 231 of 288;
      combine cells (shape, uni L0 / L1 / weight pair / GPM / CIIP weight): 54 of 85 -- 36 of the 45 (shape, pair), no GPM, no CIIP;
      plane cells (shape, lists, both / luma only / chroma only): 74 of 81;
      luma windows: 1495 inside the picture, 260 wholly outside, 660 across a border; border cells (plane, shape, side set, offset 0..3)
        365 of 732; staging paths interior and clamped, never slow; LMCS never on.
    With mc_cells_*.ovg every cell that exists is reached, and every (shape, combine) of the combine family has a case whose combine
    leaves the sample range below 0 and one above 1023 (from mc_census.final_before_clip, which is asserted to reproduce the reference's
    samples on that family).  Not covered at this level: LMCS (the plain slots of the reference take no reshaper, so no fixture sets
    the flag and the label only says so; tests/test_gpu_mc_cells.py runs the planes family with it against the oracle, the picture
    streams pipe*.ovg run it against the reference), the slow staging path (no recorder emits it: it takes a picture whose stride or width is no multiple of 4,
    tests/test_gpu_mc_cells.py runs the border family through such a view).

    mcx.ovg alone (450 draws -> 1108 units, 728 of them DMVR): clip_mv moves the initial vector of 7 DMVR units (narrow units next to
    the border; the far range is drawn for BDOF-only cases alone), never of both lists; 46 DMVR units keep their vectors; no refined
    vector ends at a +-2^17 limit.  With mcx_cells_*.ovg: clip_mv moves the vector of each list on each of the four sides, for every
    refined shape, with and without BDOF, and of both lists at once; the final clip stops every component of the refined vectors at
    either limit where the initial vector was not there, which breaks the mirrored update.
    DMVR's outcome, labelled from the oracle's trace of the 25 costs (the labels predict the reference's refined vector on every DMVR
    unit of every file: mc_census.refined_fixture asserts it).  mcx.ovg alone: never an early exit (the 46 units that stay are centre
    wins), all 25 arg-min indices, index ties but no centre tie, 8 of the 14 (axis, sub-pel branch) -- no zero denominator, no -8, no
    +8 --, +-7 on both axes, BDOF never switched off by the cost (3 of 9 cells).  With the paint family every cell of
    mc_census.dmvr_cells_that_exist() is reached.
    Steps 3 and 4 of k_mcx (mc_census.refined_reads / label_bdof / refined_cells_that_exist).  mcx.ovg alone reaches all 18 (shape,
    BDOF / DMVR / both, half-pel), all 25 (ldx, ldy) and 9 (cdx, cdy), and reads the apron on all four sides of the luma and of the
    chroma windows in a way that shows (the reference picture's samples there would give another block: its pictures are rough
    enough, computed from the pictures); of the 30 (shape, BDOF label) it reaches 24 -- never an output clipped at 0 or at 1023.  The paint family's two
    regions near the ends of the sample range add those."""
    import mc_census as mc
    refs, _, descs, _, _, units = mc.plain_fixture("mc.ovg")
    W, H = refs[0].w, refs[0].h
    labels = [lb for _, _, lb in units]
    r = mc.reach_plain(labels)
    ph, cb, pl, bd = mc.phase_cells_that_exist(), mc.combine_cells_that_exist(), mc.plane_cells_that_exist(), mc.border_cells_that_exist(W, H)
    assert (len(ph), len(cb), len(pl), len(bd)) == (3520, 85, 81, 732)
    assert len(descs) == 750 and len(units) == 1912 and sum(len(lb["windows"]) for lb in labels) == 4814
    assert r["phase"] <= ph and r["combine"] <= cb and r["planes"] <= pl and r["border"] <= bd
    assert (len(r["phase"]), len(r["combine"]), len(r["planes"]), len(r["border"])) == (1637, 54, 74, 365)
    coarse = lambda axis, plane, key: len({key(c) for c in r["phase"] if c[:2] == (axis, plane)})
    assert coarse("H", "luma", lambda c: (c[2], c[4], c[5])) == 234 and coarse("V", "luma", lambda c: (c[2], c[5])) == 142
    assert coarse("H", "chroma", lambda c: (c[2], c[4], c[5])) == 345 and coarse("V", "chroma", lambda c: (c[2], c[5])) == 231
    assert len({c for c in r["combine"] if c[1][0] == "bi"}) == 36 and not {c for c in r["combine"] if c[1][0] in ("gpm", "ciip")}
    lw = [w for lb in labels for w in lb["windows"] if not w[1]]
    assert len(lw) == 2415 and sum(w[3] is None for w in lw) == 1495 and sum(w[3] is not None and w[3].startswith("out") for w in lw) == 260
    assert r["path"] == {"interior", "clamped"} and r["lmcs"] == {False}

    # ---- with the enumerated cells
    fams = {}
    for f in golden_cases.mc_cell_files():
        refs_f, intra, descs_f, exp_off, exp, units_f = mc.plain_fixture(f)
        assert (refs_f[0].w, refs_f[0].h) == (W, H)
        fr = mc.reach_plain([lb for _, _, lb in units_f])
        fam = fams.setdefault(f.split("_")[2], {k: set() for k in fr if isinstance(fr[k], set)})
        for k in fam:
            fam[k] |= fr[k]
        r = {k: (r[k] | fr[k] if isinstance(fr[k], set) else r[k]) for k in r}
    assert r["phase"] == ph, f"phase cells without a case: {sorted(ph - r['phase'])[:8]}"
    assert r["combine"] == cb, f"combine cells without a case: {sorted(cb - r['combine'], key=str)[:8]}"
    assert r["planes"] == pl and r["border"] == bd, f"border cells without a case: {sorted(bd - r['border'])[:8]}"
    # each family reaches its cells on its own, the phase family with every window inside the picture
    assert fams["phase"]["phase"] == ph and fams["phase"]["path"] == {"interior"}
    assert fams["combine"]["combine"] == cb and fams["planes"]["planes"] == pl and fams["border"]["border"] == bd
    assert r["nout"] == {(nl, nc, ls) for nl, nc in ((1, 1), (2, 1), (4, 2)) for ls in ("L0", "L1", "BI")}
    # the combine family: the restated combine reproduces the reference, and the clip binds at both ends in every cell
    clips = {}
    for f in golden_cases.mc_cell_files():
        if "_combine_" not in f:
            continue
        refs_f, intra, descs_f, exp_off, exp, units_f = mc.plain_fixture(f)
        for i, u, lb in units_f:
            d = descs_f[i]
            assert (d.x0, d.y0, 1 << d.log2_w, 1 << d.log2_h) == (u["x"], u["y"], u["w"], u["h"])       # a PU is one unit
            want = mc.expected_picture(descs_f, exp_off, exp, W, H, [i]).planes()
            for p, (v, s) in enumerate(zip(mc.final_before_clip(u, refs_f), mc.final_samples(u, refs_f, intra))):
                c = p != 0
                x, y = d.x0 >> c, d.y0 >> c
                assert np.array_equal(s, want[p][y:y + s.shape[0], x:x + s.shape[1]]), f"{f} case {i} plane {p}: the census restates another combine than the reference's"
                ends = clips.setdefault((lb["shape"], lb["combine"][:3] if lb["combine"][0] == "ciip" else lb["combine"]), set())
                ends |= ({"below 0"} if (v < 0).any() else set()) | ({"above 1023"} if (v > 1023).any() else set())
    assert set(clips) == cb
    dull = sorted((k for k, v in clips.items() if v != {"below 0", "above 1023"}), key=str)
    assert not dull, f"(shape, combine) whose cases never leave the sample range at both ends: {dull[:8]}"

    # ---- refined units
    _, descs_x, _, _, _, ux = mc.refined_fixture("mcx.ovg")
    dm = [lb for _, _, lb in ux if lb["dmvr"]]
    assert len(descs_x) == 450 and len(ux) == 1108 and len(dm) == 728
    assert sum(bool(lb["clip"]) for lb in dm) == 7 and not any(len({l for l, _ in lb["clip"]}) == 2 for lb in dm)
    assert sum(not lb["moved"] for lb in dm) == 46 and not any(lb["at_limit"] for lb in dm) and all(lb["symmetric"] for lb in dm)
    far = [lb for f in golden_cases.mcx_cell_files() if "_far_" in f for _, _, lb in mc.refined_fixture(f)[5]]
    lim = [lb for f in golden_cases.mcx_cell_files() if "_limit_" in f for _, _, lb in mc.refined_fixture(f)[5]]
    assert all(lb["dmvr"] for lb in far + lim)
    want = {(s, b, l, side) for s in ((8, 16), (16, 8), (16, 16)) for b in (False, True) for l in (0, 1) for side in "LRTB"}
    assert {(lb["shape"], lb["bdof"], l, side) for lb in far for l, side in lb["clip"]} == want
    assert any(len({l for l, _ in lb["clip"]}) == 2 for lb in far) and any(lb["moved"] for lb in far if lb["clip"])
    assert {e for lb in lim for e in lb["at_limit"] - lb["ini_at_limit"]} == {(k, hi) for k in range(4) for hi in (False, True)}, "a component the final clip never stops"
    assert any(not lb["symmetric"] for lb in lim), "the +-2^17 clip never breaks the mirrored update"
    # DMVR's outcome
    cells = mc.dmvr_cells_that_exist()
    rd = mc.reach_dmvr(dm)
    assert all(rd[k] <= cells[k] for k in cells)
    assert rd["exit"] == {(s, False) for s in mc.REFINED_SHAPES} and rd["idx"] == cells["idx"] and rd["tie"] == {"none", "index"}
    assert rd["branch"] == {(a, b) for a in "xy" for b in ("ring", "q<0", "q=0", "q>0")} and rd["q7"] == cells["q7"]
    assert not rd["clip"] and rd["bdof_off"] == {(s, True, False) for s in mc.REFINED_SHAPES}
    assert all(lb["outcome"]["idx"] == 12 and lb["outcome"]["searched"] for lb in dm if not lb["moved"])
    everything = dm + [lb for f in golden_cases.mcx_cell_files() for _, _, lb in mc.refined_fixture(f)[5]]
    ra = mc.reach_dmvr(everything)
    for k in cells:
        assert ra[k] == cells[k], f"DMVR {k} cells without a case: {sorted(cells[k] - ra[k], key=str)}"
    assert {e for lb in lim for e in lb["outcome"]["clip_binds"]} == cells["clip"]
    # steps 3 and 4: flags, displacements, apron reads, BDOF
    rc, all_x = mc.refined_cells_that_exist(), [lb for _, _, lb in ux]
    r0 = mc.reach_refined(all_x)
    assert all(r0[k] <= rc[k] for k in rc) and r0["disp_all"] <= rc["disp_l"]
    assert (len(rc["flags"]), len(rc["disp_l"]), len(rc["disp_c"]), len(rc["apron"]), len(rc["bdof"])) == (18, 25, 9, 8, 30)
    assert all(r0[k] == rc[k] for k in ("flags", "disp_l", "disp_c", "apron"))
    assert rc["bdof"] - r0["bdof"] == {(s, c) for s in mc.REFINED_SHAPES for c in ("clip at 0", "clip at 1023")}
    ra = mc.reach_refined(all_x + [lb for lb in everything if lb not in dm])
    for k in rc:
        assert ra[k] == rc[k], f"refined {k} cells without a case: {sorted(rc[k] - ra[k], key=str)}"
    cells_alone = mc.reach_refined([lb for f in golden_cases.mcx_cell_files() for _, _, lb in mc.refined_fixture(f)[5]])
    assert cells_alone["apron"] == rc["apron"] and cells_alone["bdof"] == rc["bdof"] and cells_alone["disp_l"] == rc["disp_l"]


def test_mc_cells_discriminate(built_lib):
    """The enumerated cells pin what they are named after: the oracle (equal to the reference on every case, above) predicts ANOTHER
    block when a unit is edited -- every vector component of a list the unit reads moved by one sixteenth either way (the next phase;
    phase family), the weights of a BCW pair swapped (combine family), and for the DMVR units whose initial vector lies beyond clip_mv's
    range that component mirrored to the same distance inside it (far family: samples or refined vectors must change).  No edit may
    fail to.  The apron edit (the oracle's true_apron switch: the final interpolation and BDOF's ring read the reference picture where
    rcn_dmvr_mv_refine reads the 2-sample replicated apron) runs on every DMVR unit of mcx.ovg and of the cell files that
    mc_census.refined_reads labels as reading the apron in a way that shows (the averaged sample or a ring sample differs): every one
    must come out another block, on every (plane, side)."""
    import mc_census as mc
    dull, n = [], {"phase": 0, "bcw": 0, "clip": 0}

    def run(refs, u, intra=None, refined=False):
        dst = _filled(refs[0].w, refs[0].h, 0)
        a = np.array([u], capi.MC_UNIT_DTYPE)
        mv = oracle_lib.mc_ex(dst, refs, a) if refined else oracle_lib.mc(dst, refs, a, intra=intra)
        return [p.copy() for p in dst.planes()], None if mv is None else mv.tolist()

    def differs(a, b):
        return a[1] != b[1] or any(not np.array_equal(p, q) for p, q in zip(a[0], b[0]))

    for f in golden_cases.mc_cell_files():
        fam = f.split("_")[2]
        if fam not in ("phase", "combine"):
            continue
        refs, intra, _, _, _, units = mc.plain_fixture(f)
        for i, u, lb in units:
            base = run(refs, u, intra)
            if fam == "phase":
                for l in lb["phases"]:
                    for field in ("mv1x", "mv1y") if l else ("mv0x", "mv0y"):
                        for step in (-1, 1):
                            e = u.copy()
                            e[field] += step
                            n["phase"] += 1
                            if not differs(base, run(refs, e, intra)):
                                dull.append((f, i, field, step))
            elif lb["combine"][0] == "bi" and lb["combine"][1] != lb["combine"][2]:
                e = u.copy()
                e["w0"], e["w1"] = u["w1"], u["w0"]
                n["bcw"] += 1
                if not differs(base, run(refs, e)):
                    dull.append((f, i, "bcw pair"))
    for f in golden_cases.mcx_cell_files():
        if "_far_" not in f:
            continue
        refs, _, _, _, _, units = mc.refined_fixture(f)
        for i, u, lb in units:
            base = run(refs, u, refined=True)
            for l, side in sorted(lb["clip"]):
                field = ("mv1" if l else "mv0") + ("x" if side in "LR" else "y")
                cx, cy = mc.clip_mv(refs[0].w, refs[0].h, int(u["x"]), int(u["y"]), int(u["w"]), int(u["h"]), int(u["mv1x" if l else "mv0x"]), int(u["mv1y" if l else "mv0y"]))
                limit = cx if side in "LR" else cy
                e = u.copy()
                e[field] = 2 * limit - int(u[field])
                n["clip"] += 1
                if not differs(base, run(refs, e, refined=True)):
                    dull.append((f, i, field, "across the clip limit"))
    apron_changed, apron_n = set(), 0
    for f in ["mcx.ovg"] + golden_cases.mcx_cell_files():
        refs, _, _, _, _, units = mc.refined_fixture(f)
        for i, u, lb in units:
            if lb["reads"]["apron"]:
                a, b = _filled(refs[0].w, refs[0].h, 0), _filled(refs[0].w, refs[0].h, 0)
                _, mv_a = oracle_lib.dmvr_trace(a, refs, u)
                _, mv_b = oracle_lib.dmvr_trace(b, refs, u, true_apron=True)
                assert np.array_equal(mv_a, mv_b)                         # the search reads no apron: the vectors stay
                apron_n += 1
                apron_changed |= lb["reads"]["apron"]
                if all(np.array_equal(p, q) for p, q in zip(a.planes(), b.planes())):
                    dull.append((f, i, "apron", sorted(lb["reads"]["apron"])))
    n["apron"] = apron_n
    assert apron_n > 500 and apron_changed == {(p, sd) for p in ("luma", "chroma") for sd in "LRTB"}
    print(f"edits: {n}; without effect: {len(dull)}")
    assert n["phase"] > 5000 and n["bcw"] >= 9 * 4 * 3 and n["clip"] > 150
    assert not dull, f"{len(dull)} edits leave the prediction as it is, first: {dull[:8]}"
