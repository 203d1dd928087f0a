"""CPU: the reference-side override block (shim/rcn_hip.c -> rcn_init_functions_hip) is pinned on the reference.

The command streams the INSTALLED slots recorded (tests/golden/shim_*.ovg, see shim_cases.py) are executed by the oracle
and compared with the bytes the reference's scalar slots produced for the same seeded decoder states (tests/golden/*.ovg).
Also: the shim compiles against the reference's headers with its layout assertions (only where /root/reference exists)."""
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import golden_cases
import golden_io
import oracle_lib
from oracle_lib import HostPic
from openvvc_amd import capi
from shim_cases import ShimStream

ROOT = Path(__file__).resolve().parent.parent
REF = Path("/root/reference/libovvc/rcn_structures.h")


def _dynamic_symbols(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", str(lib)], capture_output=True, text=True, check=True).stdout
    return {line.split()[2] for line in out.splitlines() if len(line.split()) == 3 and line.split()[1] in "TDB"}


@pytest.mark.skipif(not REF.exists(), reason="the reference tree is only present in the build container")
def test_shim_builds_against_reference_headers(built_lib):
    """sizeof(struct RCNFunctions) == 5952 and the slot offsets are _Static_asserts in shim/rcn_hip.c; the library must
    export the installer with the signature of rcn_init_functions() -- and exactly what shim/rcn_hip.h declares: whatever else the
    units of the override block share stays hidden.  The same for the build against the patched reference, where it exists."""
    subprocess.check_call(["make", "-C", str(ROOT / "shim")], stdout=subprocess.DEVNULL)
    header = (ROOT / "shim" / "rcn_hip.h").read_text()
    declared = set(re.findall(r"\b(rcn_init_functions_hip|ovhip_shim_\w+)\s*\(", header))
    assert len(declared) == 26 and {"rcn_init_functions_hip", "ovhip_shim_bind_recorder", "ovhip_shim_apply_tmvp_cells"} <= declared
    assert _dynamic_symbols(ROOT / "shim" / "_build" / "librcn_hip.so") == declared
    patched = ROOT / "oracle" / "_ref" / "patched" / "librcn_hip.so"
    if patched.exists():
        assert _dynamic_symbols(patched) == declared


@pytest.mark.skipif(not REF.exists(), reason="the reference tree is only present in the build container")
def test_shim_fixtures_regenerate_identically(built_lib, tmp_path):
    """The committed shim_*.ovg are what the harness produces from the current shim + recorder sources."""
    subprocess.check_call(["make", "-C", str(ROOT / "oracle")], stdout=subprocess.DEVNULL)
    subprocess.check_call([str(ROOT / "oracle" / "_ref" / "gen_golden"), str(tmp_path), "shim"], stderr=subprocess.DEVNULL)
    for f in sorted(f for f in (ROOT / "tests" / "golden").glob("shim_*.ovg") if not f.name.startswith(("shim_pipe", "shim_tiles"))):      # shim_pipe* / shim_tiles*: test_pipe_cpu.py
        assert (tmp_path / f.name).read_bytes() == f.read_bytes(), f.name


def _pred_pic(g):
    return HostPic(128, 128, g["pred_y"].copy(), g["pred_cb"].copy(), g["pred_cr"].copy())


def run_tu_stream(pic, c):
    """A recorded TU on `pic`.  TUs of intra CUs carry the chroma prediction as an ordered task; the reference run behind
    itx.ovg had intra_pred_c stubbed out (the fixture isolates the residual paths), so the task keeps only its residual half
    (OVHIP_IT_RES_C: prediction = what is there).  The prediction half is pinned by intra.ovg / intra_ctu.ovg."""
    t = c["itask"].copy()
    assert (t["kind"] == capi.IT_CHROMA).all()
    t["kind"] = capi.IT_RES_C
    res = HostPic(pic.w, pic.h)
    oracle_lib.itx_res(pic, c["tb"], c["coef"], None, res)
    if len(t):
        oracle_lib.intra_tasks(pic, t, (res.y.view(np.int16), res.cb.view(np.int16), res.cr.view(np.int16)))
    return len(t)


def test_shim_tu_slots_match_reference(built_lib):
    """tmp.rcn_tu_st / tmp.rcn_tu_c through the installed table: 425 TUs."""
    g = golden_io.load("itx.ovg")
    s = ShimStream("shim_itx.ovg")
    assert s.n == g["desc"].shape[0] == 425
    n_cmds = n_tasks = 0
    for i in range(s.n):
        d = capi.TuDesc.from_buffer_copy(g["desc"][i].tobytes())
        c = s.case(i)
        pic = _pred_pic(g)
        n_tasks += run_tu_stream(pic, c)
        n_cmds += len(c["tb"])
        x0, y0, w, h = d.x0, d.y0, 1 << d.log2_tb_w, 1 << d.log2_tb_h
        eo = g["exp_off"][i]
        if d.tree == 0:
            rects = [(0, x0, y0, w, h, int(eo[0])), (1, x0 >> 1, y0 >> 1, w >> 1, h >> 1, int(eo[1])), (2, x0 >> 1, y0 >> 1, w >> 1, h >> 1, int(eo[2]))]
        else:
            rects = [(1, x0, y0, w, h, int(eo[1])), (2, x0, y0, w, h, int(eo[2]))]
        golden_cases.check_rects(pic, rects, g["exp"], f"shim tu case {i} tree={d.tree}")
    assert n_cmds > 600 and n_tasks > 200


def test_shim_transform_tree_slot_matches_reference(built_lib):
    g = golden_io.load("itx.ovg")
    s = ShimStream("shim_itx_tree.ovg")
    assert s.n == g["tt_desc"].shape[0] == 12
    for i in range(s.n):
        d = capi.TtDesc.from_buffer_copy(g["tt_desc"][i].tobytes())
        c = s.case(i)
        pic = _pred_pic(g)
        oracle_lib.itx(pic, c["tb"], c["coef"])
        w, h = 1 << d.log2_w, 1 << d.log2_h
        eo = g["tt_exp_off"][i]
        golden_cases.check_rects(pic, [(0, 0, 0, w, h, int(eo[0])), (1, 0, 0, w >> 1, h >> 1, int(eo[1])), (2, 0, 0, w >> 1, h >> 1, int(eo[2]))],
                                 g["exp"], f"shim transform tree {i}")


def _pu_rects(d, exp_off, i):
    w, h = 1 << d.log2_w, 1 << d.log2_h
    return [(0, d.x0, d.y0, w, h, int(exp_off[i, 0])), (1, d.x0 >> 1, d.y0 >> 1, w >> 1, h >> 1, int(exp_off[i, 1])),
            (2, d.x0 >> 1, d.y0 >> 1, w >> 1, h >> 1, int(exp_off[i, 2]))]


def _blank(rw, rh):
    dst = HostPic(rw, rh)
    dst.y[:] = 0xABAB; dst.cb[:] = 0xABAB; dst.cr[:] = 0xABAB
    return dst


def test_shim_mcp_slots_match_reference(built_lib):
    """rcn_mcp_b / rcn_mcp_b_l / rcn_mcp_b_c through the installed table: 750 PUs."""
    refs, descs, exp_off, exp = golden_cases.mc_cases()
    s = ShimStream("shim_mc.ovg")
    assert s.n == len(descs) == 750
    srefs = s.refs(refs)
    for i, d in enumerate(descs):
        dst = _blank(refs[0].w, refs[0].h)
        oracle_lib.mc(dst, srefs, s.case(i)["mc"])
        golden_cases.check_rects(dst, _pu_rects(d, exp_off, i), exp, f"shim mc case {i} dir={d.inter_dir} planes={d.planes}")


def test_shim_refined_slots_match_reference(built_lib):
    """rcn_bdof_mcp_l (+ rcn_mcp_b_c) and rcn_dmvr_mv_refine through the installed table, incl. the refined vectors; the
    harness has already checked that ovhip_shim_apply_tmvp_cells writes exactly the TMVP plane entries the reference's
    caller + tmvp_store_mv write (mv_patch_checked = entries compared per DMVR case)."""
    refs, descs, exp_off, exp, exp_mv = golden_cases.mcx_cases()
    s = ShimStream("shim_mcx.ovg")
    assert s.n == len(descs) == 450
    srefs = s.refs(refs)
    n_dmvr = 0
    for i, d in enumerate(descs):
        c = s.case(i)
        dst = _blank(refs[0].w, refs[0].h)
        oracle_lib.mc(dst, srefs, c["mc"])
        mv = oracle_lib.mc_ex(dst, srefs, c["mcx"])
        golden_cases.check_rects(dst, _pu_rects(d, exp_off, i), exp, f"shim mcx case {i} refine={d.refine}")
        if d.refine & capi.PU_DMVR:
            want = exp_mv[int(exp_off[i, 3]) // 4:int(exp_off[i, 3]) // 4 + len(c["mcx"])]
            assert np.array_equal(mv, want), f"shim mcx case {i}: refined MVs differ"
            n_dmvr += 1
    chk = s.g["mv_patch_checked"]
    assert len(chk) == n_dmvr and chk.min() >= 1 and chk.sum() > 600


def _tmvp_expected(s, i):
    e = np.asarray(s.g["tmvp_expected"]).reshape(-1, 3)
    return {(int(c), int(u)) for k, c, u in e if k == i}


def test_tmvp_plane_cells_match_reference_flow(built_lib):
    """Where the refined vectors go in the picture's collocated motion plane: the oracle's sequential restatement
    of the caller's stores + tmvp_store_mv against the entries the harness saw the reference's flow write (tmvp_expected:
    case, plane cell, unit), for every DMVR case of the shim-recorded stream."""
    refs, descs, exp_off, exp, exp_mv = golden_cases.mcx_cases()
    s = ShimStream("shim_mcx.ovg")
    nb_ctb_w = (refs[0].w + 127) // 128
    n = 0
    for i, d in enumerate(descs):
        if not d.refine & capi.PU_DMVR:
            assert not _tmvp_expected(s, i)
            continue
        units = s.case(i)["mcx"]
        fake = (1000 + 8 * np.arange(len(units))[:, None] + np.arange(4)[None, :]).astype(np.int32)
        got = oracle_lib.tmvp_cells(units, fake, 7, nb_ctb_w)
        have = {(int(c["cell"]), int((c["mv0x"] - 1000) // 8)) for c in got if c["cell"] != capi.TMVP_NONE}
        assert have == _tmvp_expected(s, i), f"case {i}"
        for c in got:
            if c["cell"] != capi.TMVP_NONE:
                u = (int(c["mv0x"]) - 1000) // 8
                assert [c["mv0x"], c["mv0y"], c["mv1x"], c["mv1y"]] == fake[u].tolist()
        n += len(have)
    assert n > 600


def test_shim_affine_slots_match_reference(built_lib):
    """The affine drivers' per-4x4 rcn_mcp_b_l / rcn_prof_mcp_b_l and per-8x8 rcn_mcp_b_c calls, collected back into CUs."""
    refs, cases, exp_off, exp = golden_cases.mca_cases()
    s = ShimStream("shim_mca.ovg")
    assert s.n == len(cases) == 332
    srefs = s.refs(refs)
    for i, (d, _, _) in enumerate(cases):
        c = s.case(i)
        assert len(c["mc"]) == 0 and len(c["aff"]) >= 1
        dst = _blank(refs[0].w, refs[0].h)
        oracle_lib.mca(dst, srefs, c["aff"], c["side"])
        golden_cases.check_rects(dst, _pu_rects(d, exp_off, i), exp, f"shim mca case {i} dir={d.inter_dir} prof={d.prof_dir}")


def test_shim_gpm_ciip_slots_match_reference(built_lib):
    """rcn_gpm_b, rcn_ciip_b / rcn_ciip through the installed table.  A CIIP CU is recorded as its inter unit + two planar
    ordered tasks carrying the blend weight.  Cases [n_gpm, first_planar) come from a reference run whose intra slots were
    stubbed (a known "planar" picture): there the tasks are checked through their geometry and weight only (fed to the fused
    blend with that picture); cases from first_planar on ran the real intra_pred / intra_pred_c and are executed as recorded."""
    refs, intra, descs, modes, n_gpm, exp_off, exp = golden_cases.gpm_cases()
    cur, first_planar = golden_cases.ciip_planar_cases()
    s = ShimStream("shim_gpm.ovg")
    assert s.n == len(descs) and n_gpm < first_planar < s.n
    srefs = s.refs(refs)
    for i, d in enumerate(descs):
        c = s.case(i)
        t = c["itask"]
        dst = _blank(refs[0].w, refs[0].h) if i < first_planar else HostPic(cur.w, cur.h, cur.y.copy(), cur.cb.copy(), cur.cr.copy())
        oracle_lib.mc(dst, srefs, c["mc"])
        if i < n_gpm:
            assert len(t) == 0
        else:
            lw = int(d.log2_w)
            assert len(t) == (2 if lw > 2 else 1) and t[0]["kind"] == capi.IT_LUMA and t[0]["mode"] == 0 and 1 <= t[0]["ciip_wt"] <= 3
            assert (t[0]["x"], t[0]["y"], t[0]["log2_w"], t[0]["log2_h"]) == (d.x0, d.y0, d.log2_w, d.log2_h)
            if i < first_planar:
                u = np.zeros(1, capi.CIIP_UNIT_DTYPE)
                u["x"], u["y"], u["log2_w"], u["log2_h"], u["wt"], u["chroma_inter"] = d.x0, d.y0, d.log2_w, d.log2_h, t[0]["ciip_wt"], lw <= 2
                oracle_lib.ciip(dst, intra, u)
            else:
                oracle_lib.intra_tasks(dst, t)
        golden_cases.check_rects(dst, _pu_rects(d, exp_off, i), exp, f"shim {'gpm' if i < n_gpm else 'ciip'} case {i}")


def test_shim_lmcs_slots_match_reference(built_lib):
    """rcn_init_lmcs -> device tables; rcn_lmcs_compute_chroma_scale -> regions whose device-derived scale equals the
    reference's."""
    pic_y, sets, regions, _ = golden_cases.lmcs_cases()
    g = golden_io.load("shim_lmcs.ovg")
    assert g["luts"].shape[0] == len(sets)
    reg = np.frombuffer(g["region"].tobytes(), dtype=capi.LMCS_REGION_DTYPE)
    assert len(reg) == len(regions)
    h, w = pic_y.shape
    for si, (_, want) in enumerate(sets):
        assert g["luts"][si].tobytes() == bytes(want), f"LMCS tables of set {si} differ"
        sel = np.nonzero(regions[:, 0] == si)[0]
        scales = oracle_lib.lmcs_scale(HostPic(w, h, pic_y.copy()), reg[sel], want)
        assert np.array_equal(scales, regions[sel, 5].astype(np.int16)), f"set {si}"


def test_shim_filter_slots_match_reference(built_lib):
    """df.rcn_dbf_ctu(_truncated): the edge lists equal the ones the reference-pinned recorder test derives; sao / alf
    lines: the captured parameters equal the reference's SAOParamsCtu / ALFParamsCtu / RCNALF contents."""
    gd = golden_io.load("shim_dbf.ovg")
    for i, (_, planes, _) in enumerate(golden_cases.dbf_cases()):
        for d, name in ((0, "v"), (1, "h")):
            want, offs = planes["edges"][d]
            got = np.frombuffer(gd[f"p{i}_edges_{name}"].tobytes(), dtype=capi.DBF_EDGE_DTYPE)
            assert np.array_equal(got, want), f"dbf picture {i} dir {name}"
        o = gd[f"p{i}_offsets"]
        assert o[0] == planes["beta_offset"] and o[8] == planes["tc_offset"]
    gs, gr = golden_io.load("shim_sao.ovg"), golden_io.load("sao.ovg")
    for i in range(3):
        assert gs[f"p{i}_params"].tobytes() == gr[f"p{i}_params"].tobytes(), f"sao picture {i}"
    ga, gr = golden_io.load("shim_alf.ovg"), golden_io.load("alf.ovg")
    for i in range(3):
        for k in ("ctus", "luma_coeff", "luma_clip", "chroma_coeff", "chroma_clip", "cc_coeff"):
            assert ga[f"p{i}_{k}"].tobytes() == gr[f"p{i}_{k}"].tobytes(), f"alf picture {i} {k}"


def test_shim_refuses_rect_entries_spread_over_two_ctu_decoders(built_lib):
    """A picture cut into two rect entries (tile columns) with each entry on its OWN OVCTUDec (entry threads, ovthreads.c:112-114):
    the harness attached the frame and drove `sao.rcn_sao_first_pix_rows` with each entry's einfo (record-only) and stored what
    `ovhip_shim_last_error` latched.  The entry that starts the picture is taken; the OVCTUDec that never saw the picture's first
    entry latches OVHIP_EUNSUP -- not a half-picture flush.  (Entries in turn on one OVCTUDec: tests/test_pipe_cpu.py, tiles.)"""
    g = golden_io.load("shim_sao.ovg")
    assert [int(v) for v in g["two_entries_latched"]] == [0, capi.OVHIP_EUNSUP]


def intra_ctu_cases():
    """(start picture planes, [(dual, expected Y / Cb / Cr of the CTU at (128, 128))]) from intra_ctu.ovg."""
    g = golden_io.load("intra_ctu.ovg")
    out = []
    for dual, n_cu, n_intra, off in g["info"]:
        e = g["exp"][int(off):int(off) + 128 * 128 + 2 * 64 * 64]
        out.append((int(dual), int(n_intra), e[:16384].reshape(128, 128), e[16384:20480].reshape(64, 64), e[20480:].reshape(64, 64)))
    return (g["pic_y"], g["pic_cb"], g["pic_cr"]), out


def test_shim_intra_ctus_match_reference(built_lib):
    """tmp.rcn_transform_tree on intra CUs (-> rcn_intra_tu + rcn_tu_st, rcn_tu_l, rcn_tu_c): the installed slots turn every
    CU into ordered tasks (availability out of the progress bit-fields, MIP / MRL / BDPCM / LM parameters out of the ctudec) +
    STORE-mode transform blocks; the recorder levels them.  Executing each recorded CTU on the start picture gives the CTU
    the reference's own slots left, 36 CTUs (single and dual tree), ~2000 tasks."""
    base, cases = intra_ctu_cases()
    s = ShimStream("shim_intra_ctu.ovg")
    assert s.n == len(cases) == 36
    h, w = base[0].shape
    n_tasks = 0
    for i, (dual, n_intra, ey, ecb, ecr) in enumerate(cases):
        c = s.case(i)
        t = c["itask"]
        assert len(t) >= n_intra and len(c["mc"]) == 0
        n_tasks += len(t)
        dst = HostPic(w, h, base[0].copy(), base[1].copy(), base[2].copy())
        res = HostPic(w, h)
        oracle_lib.itx_res(dst, c["tb"], c["coef"], None, res)
        oracle_lib.intra_tasks(dst, t, (res.y.view(np.int16), res.cb.view(np.int16), res.cr.view(np.int16)))
        for name, got, exp in (("Y", dst.y[128:256, 128:256], ey), ("Cb", dst.cb[64:128, 64:128], ecb), ("Cr", dst.cr[64:128, 64:128], ecr)):
            assert np.array_equal(got, exp), f"intra CTU {i} (dual={dual}) plane {name}: {int((got != exp).sum())} samples differ"
        # level order == decoding order for what the shim recorded
        order = np.argsort(t["level"], kind="stable")
        dst2 = HostPic(w, h, base[0].copy(), base[1].copy(), base[2].copy())
        oracle_lib.itx_res(dst2, c["tb"], c["coef"], None, res)
        oracle_lib.intra_tasks(dst2, t[order], (res.y.view(np.int16), res.cb.view(np.int16), res.cr.view(np.int16)))
        assert np.array_equal(dst2.y, dst.y) and np.array_equal(dst2.cb, dst.cb) and np.array_equal(dst2.cr, dst.cr)
    assert n_tasks > 1500


def isp_cases():
    g = golden_io.load("isp.ovg")
    return g["pic_y"], g["info"], g["exp"]


def test_shim_isp_slots_match_reference(built_lib):
    """tmp.recon_isp_subtree_v / _h through the installed table: 394 intra-sub-partition CUs (4x8 ... 64x64, both directions,
    1xN / 2xN / Nx1 / Nx2 and regular transform blocks, DST-VII, LFNST).  Each prediction call is an ordered task with the CU's
    arms, chained partition after partition; executing the recorded stream gives the CU the reference's slot left."""
    base, info, exp = isp_cases()
    s = ShimStream("shim_isp.ovg")
    assert s.n == len(info) == 394
    h, w = base.shape
    bad = []
    for i, (x, y, l2w, l2h, vertical, mode, bits, off) in enumerate(info):
        c = s.case(i)
        t = c["itask"]
        assert len(t) >= 1 and (t["flags"] & capi.IF_ISP).all() and np.all(np.diff(t["level"].astype(int)) > 0)
        dst = HostPic(w, h, base.copy())
        res = HostPic(w, h)
        res.y[:] = 0x1234                  # the residual picture is only defined where a transform block stored into it
        oracle_lib.itx_res(dst, c["tb"], c["coef"], None, res)
        oracle_lib.intra_tasks(dst, t, (res.y.view(np.int16), res.cb.view(np.int16), res.cr.view(np.int16)))
        bw, bh = 1 << int(l2w), 1 << int(l2h)
        got = dst.y[y:y + bh, x:x + bw]
        want = exp[int(off):int(off) + bw * bh].reshape(bh, bw)
        if not np.array_equal(got, want):
            bad.append((i, bw, bh, int(vertical), int(mode), hex(int(bits)), int((got != want).sum())))
    assert not bad, f"{len(bad)} / {len(info)} ISP CUs differ from the reference, first: {bad[:10]}"
