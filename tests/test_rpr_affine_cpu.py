"""CPU: affine coding units and lone 4x4 luma blocks on scaled references (reference picture resampling) in the recorder --
the opt-in (ovhip_rec_set_rpr_tools), the ovhip_aff_rpr_unit array and its side arena (anchors, steps and filter sets equal to
the numpy restatement tests/spec_rpr_affine.py, which equals the reference's samples of tests/golden/rpr/rpr_affine.ovg), the
unchanged recordings without such units, and the call log."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from openvvc_amd import capi
import rpr_affine_golden as G
import rpr_golden
import spec_rpr as S
import spec_rpr_affine as A
from rpr_affine_cases import random_affine_cus, reads_scaled
from rpr_cases import pu_desc, random_pus, scales_for

ROOT = Path(__file__).resolve().parent.parent
PIC_W, PIC_H = 1920, 1080
SIZES = [(3840, 2160), (1280, 720), (960, 540), (1920, 1080)]
BOTH = capi.RPR_TOOL_AFFINE | capi.RPR_TOOL_PU4x4


@pytest.fixture
def lib():
    return capi.load()


def _rec(lib, w=PIC_W, h=PIC_H, tools=None):
    r = lib.ovhip_rec_create(w, h)
    assert r
    if tools is not None:
        assert lib.ovhip_rec_set_rpr_tools(r, tools) == 0
    return r


def _set_scales(lib, rec, scales):
    for slot, s in scales.items():
        assert capi.set_ref_scale(lib, rec, slot, s["scale_hor"], s["scale_ver"], s["ref_w"], s["ref_h"], s["col_hor"], s["col_ver"]) == 0


def _bytes(lib, rec, fn, elem):
    n = C.c_size_t(0)
    p = getattr(lib, fn)(rec, C.byref(n))
    return C.string_at(p, n.value * elem) if n.value else b""


def _all_bytes(lib, rec):
    return (_bytes(lib, rec, "ovhip_rec_mc_units", C.sizeof(capi.McUnit)), _bytes(lib, rec, "ovhip_rec_rpr_units", C.sizeof(capi.RprUnit)),
            _bytes(lib, rec, "ovhip_rec_aff_units", 32), _bytes(lib, rec, "ovhip_rec_aff_side", 4),
            _bytes(lib, rec, "ovhip_rec_aff_rpr_units", C.sizeof(capi.AffRprUnit)))


def _side(lib, rec):
    return np.frombuffer(_bytes(lib, rec, "ovhip_rec_aff_side", 4), dtype=np.int32)


def _log_bytes(lib, log):
    n = C.c_size_t(0)
    p = lib.ovhip_calllog_data(log, C.byref(n))
    return C.string_at(p, n.value) if n.value else b""


def test_struct_sizes_and_abi():
    # fixed in include/ovvc_hip.h: ovhip_aff_rpr_unit 48 bytes (its per-list part 8); the v9 structs keep their sizes
    assert C.sizeof(capi.AffRprUnit) == 48 and C.sizeof(capi.AffRprList) == 8
    assert C.sizeof(capi.RprUnit) == 64 and C.sizeof(capi.RprSide) == 24 and C.sizeof(capi.RefScale) == 20
    assert C.sizeof(capi.McUnit) == 32
    assert capi.OVHIP_ABI_VERSION == 9 and capi.load().ovhip_abi_version() == 9
    hdr = (ROOT / "include" / "ovvc_hip.h").read_text()
    assert re.search(r"as ovhip_aff_unit\.\s+48 bytes\.", hdr)


def test_restatement_equals_reference():
    """Every case of the fixture, luma and both chroma planes; the classes the generator must cover are all there."""
    pic_w, pic_h, sizes, refs, cases, n_dropped = G.load()
    assert n_dropped * 50 <= len(cases) + n_dropped
    seen = dict(far=0, integer=0, ident=0, bcw=0, mixed_prof=0, both=0, uni=0)
    prof_dirs, shapes = set(), set()
    for c in cases:
        cu = c["cu"]
        sc = rpr_golden.scales(pic_w, pic_h, sizes, c["col"])
        got = A.predict_affine_cu(refs, sc, pic_w, pic_h, cu)
        for a, b in zip(got, c["exp"]):
            assert np.array_equal(a, b), {k: v for k, v in cu.items() if k not in ("mv0", "mv1", "dmv_scale")}
        d = G.effective_dir(cu)
        s0, s1 = d & 1 and cu["ref0"] in sc, d & 2 and cu["ref1"] in sc
        assert s0 or s1
        seen["far"] += int(np.abs(cu["mv0"]).max() > 8000 or np.abs(cu["mv1"]).max() > 8000)
        seen["integer"] += int(not (cu["mv0"] & 15).any() and not (cu["mv1"] & 15).any())
        seen["ident"] += int(d == 3 and cu["poc0"] == cu["poc1"] and np.array_equal(cu["mv0"], cu["mv1"]))
        seen["bcw"] += int(d == 3 and cu["bcw_idx_plus1"] not in (0, 3))
        seen["mixed_prof"] += int(d == 3 and bool(s0) != bool(s1) and bool(cu["prof_dir"] & (2 if s0 else 1)))
        seen["both"] += int(bool(s0) and bool(s1))
        seen["uni"] += int(d != 3)
        prof_dirs.add(cu["prof_dir"])
        shapes.add((cu["log2_w"], cu["log2_h"]))
    assert all(v > 0 for v in seen.values()), seen
    assert seen["mixed_prof"] * 5 >= len(cases), seen
    assert prof_dirs == {0, 1, 2, 3} and shapes == {(a, b) for a in (3, 4, 5, 6) for b in (3, 4, 5, 6)}


def test_opt_in(lib):
    scales = scales_for(PIC_W, PIC_H, SIZES)
    cu = random_affine_cus(PIC_W, PIC_H, 1, 1, seed=2)[0]
    cu.update(inter_dir=3, ref0=0, ref1=3)
    keep = []
    d = G.affine_desc(capi, cu, keep)
    rec = _rec(lib)
    try:
        _set_scales(lib, rec, scales)
        # a fresh recorder refuses, as every caller of the plain v9 interface expects
        assert lib.ovhip_rec_affine_cu(rec, C.byref(d)) == -5 and b"affine" in lib.ovhip_rec_refusal(rec)
        assert lib.ovhip_rec_cu_inter(rec, None, C.byref(d)) == -5
        assert lib.ovhip_rec_set_rpr_tools(rec, 4) == -3 and lib.ovhip_rec_set_rpr_tools(rec, 0xffffffff) == -3
        assert lib.ovhip_rec_set_rpr_tools(rec, capi.RPR_TOOL_PU4x4) == 0          # the other tool alone: still refused
        assert lib.ovhip_rec_affine_cu(rec, C.byref(d)) == -5
        assert lib.ovhip_rec_set_rpr_tools(rec, capi.RPR_TOOL_AFFINE) == 0
        n = lib.ovhip_rec_affine_cu(rec, C.byref(d))
        assert n == ((1 << cu["log2_w"]) // min(1 << cu["log2_w"], 16)) * ((1 << cu["log2_h"]) // min(1 << cu["log2_h"], 16))
        assert len(capi.aff_rpr_units(lib, rec)) == n and not _bytes(lib, rec, "ovhip_rec_aff_units", 32)
        # the setting belongs to the caller: it survives the reset, the units and the scale table do not
        lib.ovhip_rec_reset(rec)
        assert not capi.aff_rpr_units(lib, rec)
        _set_scales(lib, rec, scales)
        assert lib.ovhip_rec_cu_inter(rec, None, C.byref(d)) == n and len(capi.aff_rpr_units(lib, rec)) == n
        assert lib.ovhip_rec_set_rpr_tools(rec, 0) == 0
        assert lib.ovhip_rec_affine_cu(rec, C.byref(d)) == -5 and b"affine" in lib.ovhip_rec_refusal(rec)
    finally:
        lib.ovhip_rec_destroy(rec)


def _check_units(lib, rec, cu, units, side, scales, pic_w, pic_h):
    w, h = 1 << cu["log2_w"], 1 << cu["log2_h"]
    d = G.effective_dir(cu)
    sc = [A._scale_of(scales, cu["ref1"] if l else cu["ref0"], pic_w, pic_h) for l in (0, 1)]
    scaled = [bool(d & (1 << l)) and A._is_scaled(sc[l]) for l in (0, 1)]
    assert len(units) == (w // min(w, 16)) * (h // min(h, 16))
    prof = cu["prof_dir"] & ((0 if scaled[0] else 1) | (0 if scaled[1] else 2)) if d == 3 else 0
    mv = (cu["mv0"], cu["mv1"])
    k = 0
    for uy in range(0, h, min(h, 16)):
        for ux in range(0, w, min(w, 16)):
            u = units[k]
            k += 1
            assert (u.x, u.y, u.w, u.h, u.dir) == (cu["x0"] + ux, cu["y0"] + uy, min(w, 16), min(h, 16), d)
            assert bool(u.flags & capi.AFFR_S0) == scaled[0] and bool(u.flags & capi.AFFR_S1) == scaled[1]
            assert bool(u.flags & capi.AFFR_PROF) == bool(prof) and u.prof_dir == prof
            assert bool(u.flags & capi.AFFR_LMCS) == bool(cu.get("lmcs", 0))
            for l in (0, 1):
                s = u.s[l]
                if not d & (1 << l):      # nothing of a list a uni CU does not use
                    assert (s.step_x, s.step_y, s.filt, s.filt_c, s.ref) == (0, 0, 0, 0, 0)
                elif scaled[l]:
                    assert (s.step_x, s.step_y, s.filt, s.filt_c) == A.steps_and_sets(sc[l]) and s.ref == (cu["ref1"] if l else cu["ref0"])
                    assert 3 <= (s.filt & 15) <= 5 and 3 <= (s.filt >> 4) <= 5 and (s.filt_c & 15) <= 2 and (s.filt_c >> 4) <= 2
                else:
                    assert (s.step_x, s.step_y, s.filt, s.filt_c) == (0, 0, 0, 0)
            o = u.side_off
            ident_l = ident_c = 0
            for sy in range(0, u.h, 4):
                for sx in range(0, u.w, 4):
                    m = [mv[l][(uy + sy) >> 2, (ux + sx) >> 2] for l in (0, 1)]
                    for l in (0, 1):
                        e = A.luma_words(sc[l], u.x + sx, u.y + sy, int(m[l][0]), int(m[l][1]), pic_w, pic_h) if d & (1 << l) else (0, 0)
                        assert tuple(side[o + 2 * l:o + 2 * l + 2]) == tuple(e), (cu["x0"], cu["y0"], sx, sy, l)
                    if not cu["prof_dir"] and d == 3 and cu["poc0"] == cu["poc1"] and tuple(m[0]) == tuple(m[1]):
                        ident_l |= 1 << ((sy >> 2) * (u.w >> 2) + (sx >> 2))
                    o += 4
            for sy in range(0, u.h, 8):
                for sx in range(0, u.w, 8):
                    jj, ii = (uy + sy) >> 2, (ux + sx) >> 2
                    m = [A.avg_mv(mv[l][jj, ii], mv[l][jj + 1, ii + 1]) if d & (1 << l) else [0, 0] for l in (0, 1)]
                    for l in (0, 1):
                        e = A.chroma_words(sc[l], u.x + sx, u.y + sy, m[l][0], m[l][1], pic_w, pic_h) if d & (1 << l) else (0, 0)
                        assert tuple(side[o + 2 * l:o + 2 * l + 2]) == tuple(e)
                    if d == 3 and cu["poc0"] == cu["poc1"] and m[0] == m[1]:
                        ident_c |= 1 << ((sy >> 3) * (u.w >> 3) + (sx >> 3))
                    o += 4
            assert (u.ident_l, u.ident_c) == (ident_l, ident_c)
            if prof:
                t = side[u.prof_off:u.prof_off + 32].view(np.int16).reshape(4, 16)
                for l in (0, 1):
                    want = cu["dmv_scale"][2 * l:2 * l + 2] if prof & (1 << l) else np.zeros((2, 16), np.int16)
                    assert np.array_equal(t[2 * l:2 * l + 2], want)


@pytest.mark.parametrize("far,cols", [(False, (0, 0)), (True, (1, 0))])
def test_units_match_restatement(lib, far, cols):
    """1920x1080 with 4K / 720p / 540p references and one of the picture's size."""
    scales = scales_for(PIC_W, PIC_H, SIZES, cols)
    cus = random_affine_cus(PIC_W, PIC_H, len(SIZES), 220, seed=31 + far, far=far)
    if far:
        # ((1856 << 4) + 2^17) * 32768 + 128 = 5268045952 does not fit int32: the anchor wraps as the reference's does
        wrap = random_affine_cus(PIC_W, PIC_H, 1, 1, seed=5, cells=[(1856, 1016)])[0]
        wrap.update(inter_dir=1, ref0=0, prof_dir=0)
        wrap["mv0"] = wrap["mv0"] * 0 + (1 << 17)
        assert ((wrap["x0"] << 4) + (1 << 17)) * 32768 + 128 >= 1 << 31
        cus.append(wrap)
    rec = _rec(lib, tools=capi.RPR_TOOL_AFFINE)
    keep = []
    try:
        _set_scales(lib, rec, scales)
        n_rpr = 0
        for cu in cus:
            before = len(capi.aff_rpr_units(lib, rec))
            assert lib.ovhip_rec_affine_cu(rec, C.byref(G.affine_desc(capi, cu, keep))) > 0, lib.ovhip_rec_refusal(rec)
            units = capi.aff_rpr_units(lib, rec)[before:]
            if not reads_scaled(cu, scales):
                assert not units
                continue
            _check_units(lib, rec, cu, units, _side(lib, rec), scales, PIC_W, PIC_H)
            n_rpr += len(units)
        assert n_rpr > 200
        if far:
            u = capi.aff_rpr_units(lib, rec)[-1]
            x = int(_side(lib, rec)[u.side_off])
            assert x == S.anchor(u.x, 1 << 17, 32768, 0, 4, 3840, 4, False)[0] == S.i32(((u.x << 4) + (1 << 17)) * 32768 + 128)
    finally:
        lib.ovhip_rec_destroy(rec)


def test_recorder_on_reference_cases(lib):
    pic_w, pic_h, sizes, refs, cases, _ = G.load()
    keep = []
    for c in cases:
        sc = rpr_golden.scales(pic_w, pic_h, sizes, c["col"])
        rec = _rec(lib, pic_w, pic_h, tools=BOTH)
        try:
            _set_scales(lib, rec, sc)
            assert lib.ovhip_rec_affine_cu(rec, C.byref(G.affine_desc(capi, c["cu"], keep))) > 0, lib.ovhip_rec_refusal(rec)
            _check_units(lib, rec, c["cu"], capi.aff_rpr_units(lib, rec), _side(lib, rec), sc, pic_w, pic_h)
        finally:
            lib.ovhip_rec_destroy(rec)


def test_recordings_without_such_units_are_unchanged(lib):
    """Affine CUs on unscaled slots, and every recording of test_no_scale_table_records_as_before, with and without the opt-in."""
    scales = scales_for(PIC_W, PIC_H, SIZES)
    cus = random_affine_cus(PIC_W, PIC_H, 1, 60, seed=4)
    for cu in cus:
        cu.update(ref0=3, ref1=3)            # the slot of the picture's own size
    pus = random_pus(PIC_W, PIC_H, 7, 120, seed=1)
    keep = []
    out = []
    for tools in (None, BOTH):
        a, b = _rec(lib, tools=tools), _rec(lib, tools=tools)
        try:
            for pu in pus:
                assert lib.ovhip_rec_pu(a, C.byref(pu_desc(capi, pu))) > 0
            for cu in cus:
                assert lib.ovhip_rec_affine_cu(a, C.byref(G.affine_desc(capi, cu, keep))) > 0
            _set_scales(lib, b, scales)            # b: scaled slots exist, none is read
            for cu in cus:
                assert lib.ovhip_rec_affine_cu(b, C.byref(G.affine_desc(capi, cu, keep))) > 0
            out.append((_all_bytes(lib, a), _all_bytes(lib, b)))
            assert out[-1][0][4] == b"" and out[-1][1][4] == b"" and out[-1][0][2] and out[-1][0][2:] == out[-1][1][2:]
        finally:
            lib.ovhip_rec_destroy(a)
            lib.ovhip_rec_destroy(b)
    assert out[0] == out[1]


def test_pu4x4(lib):
    scales = scales_for(PIC_W, PIC_H, SIZES)
    pu = dict(x0=60, y0=100, log2_w=2, log2_h=2, inter_dir=3, ref0=0, ref1=1, mv0x=-37, mv0y=90, mv1x=5, mv1y=-3, poc0=1, poc1=2)
    rec = _rec(lib)
    try:
        _set_scales(lib, rec, scales)
        d = pu_desc(capi, pu)
        d.planes = 1
        assert lib.ovhip_rec_pu(rec, C.byref(d)) == -5 and b"4x4" in lib.ovhip_rec_refusal(rec)
        assert lib.ovhip_rec_set_rpr_tools(rec, capi.RPR_TOOL_PU4x4) == 0
        assert lib.ovhip_rec_pu(rec, C.byref(d)) == 1
        u = capi.rpr_units(lib, rec)[0]
        assert (u.x, u.y, u.w, u.h, u.ox, u.oy, u.dir) == (60, 100, 4, 4, 0, 0, 3)
        assert u.flags & capi.RPR_S0 and u.flags & capi.RPR_S1 and u.flags & capi.RPR_NO_CHROMA
        assert u.s[0].filt == 5 | 5 << 4 and u.s[1].filt == 3 | 3 << 4           # 2:1 and 2:3 with flag_4x4
        assert (u.s[0].pos_x, u.s[0].pos_y) == A.luma_words(scales[0], 60, 100, -37, 90, PIC_W, PIC_H)
        assert (u.s[1].pos_x, u.s[1].pos_y) == A.luma_words(scales[1], 60, 100, 5, -3, PIC_W, PIC_H)
        # a bi-prediction that mixes a scaled and an unscaled list: the unscaled side takes the 6-tap filters of 4x4 blocks, which
        # only the affine kernel holds -- a one-sub-block ovhip_aff_rpr_unit without chroma
        d = pu_desc(capi, dict(pu, ref1=3, bcw_idx_plus1=5, lmcs=1))
        d.planes = 1
        assert lib.ovhip_rec_pu(rec, C.byref(d)) == 1 and len(capi.rpr_units(lib, rec)) == 1
        a = capi.aff_rpr_units(lib, rec)[0]
        assert (a.x, a.y, a.w, a.h, a.dir, a.w0, a.w1) == (60, 100, 4, 4, 3, -2, 10)
        assert a.flags == capi.AFFR_S0 | capi.AFFR_NO_CHROMA | capi.AFFR_LMCS
        assert (a.s[0].step_x, a.s[0].step_y, a.s[0].filt, a.s[0].ref) == (32768, 32768, 5 | 5 << 4, 0) and a.s[1].ref == 3
        words = _side(lib, rec)[a.side_off:a.side_off + 4]
        assert tuple(words[:2]) == A.luma_words(scales[0], 60, 100, -37, 90, PIC_W, PIC_H)
        assert tuple(words[2:]) == S.clip_mv(60, 100, 4, 4, PIC_W, PIC_H, 5, -3)
        # with chroma it stays refused (the reference has no such call)
        for planes in (3, 2):
            d.planes = planes
            assert lib.ovhip_rec_pu(rec, C.byref(d)) == -5 and b"4x4" in lib.ovhip_rec_refusal(rec)
    finally:
        lib.ovhip_rec_destroy(rec)


def test_calllog(lib):
    scales = scales_for(PIC_W, PIC_H, SIZES, (1, 0))
    cus = random_affine_cus(PIC_W, PIC_H, len(SIZES), 80, seed=6, far=True)
    pus = random_pus(PIC_W, PIC_H, len(SIZES), 40, seed=3)
    pu4 = dict(x0=8, y0=1000, log2_w=2, log2_h=2, inter_dir=1, ref0=1, ref1=0, mv0x=11, mv0y=-7, mv1x=0, mv1y=0, poc0=1, poc1=2)
    keep = []

    def record(rec, cu_list, with_pu4):
        _set_scales(lib, rec, scales)
        for pu in pus:
            assert lib.ovhip_rec_pu(rec, C.byref(pu_desc(capi, pu))) > 0
        for cu in cu_list:
            assert lib.ovhip_rec_affine_cu(rec, C.byref(G.affine_desc(capi, cu, keep))) > 0
        if with_pu4:
            d = pu_desc(capi, pu4)
            d.planes = 1
            assert lib.ovhip_rec_pu(rec, C.byref(d)) == 1

    # a new log replays into the same bytes on a recorder that was never opted in by hand
    rec, rep = _rec(lib, tools=BOTH), _rec(lib)
    log = lib.ovhip_calllog_create()
    try:
        lib.ovhip_rec_set_calllog(rec, log)
        record(rec, cus, True)
        raw = _log_bytes(lib, log)
        assert lib.ovhip_calllog_replay(raw, len(raw), rep) > 0
        assert _all_bytes(lib, rec) == _all_bytes(lib, rep) and _all_bytes(lib, rec)[4] and _all_bytes(lib, rec)[1]
    finally:
        lib.ovhip_rec_set_calllog(rec, None)
        lib.ovhip_calllog_destroy(log)
        lib.ovhip_rec_destroy(rec)
        lib.ovhip_rec_destroy(rep)

    # a stream without such units: the log of an opted-in recorder is the log of a plain one, byte for byte
    plain = [cu for cu in cus if not reads_scaled(cu, scales)]
    assert len(plain) > 3
    logs = []
    for tools in (None, BOTH):
        rec = _rec(lib, tools=tools)
        log = lib.ovhip_calllog_create()
        try:
            lib.ovhip_rec_set_calllog(rec, log)
            record(rec, plain, False)
            logs.append(_log_bytes(lib, log))
        finally:
            lib.ovhip_rec_set_calllog(rec, None)
            lib.ovhip_calllog_destroy(log)
            lib.ovhip_rec_destroy(rec)
    assert logs[0] == logs[1] and logs[0]


def _need_reference():
    if not (ROOT / "oracle" / "_ref" / "libovvcref.so").exists():
        pytest.skip("compiled reference not present")


def test_fixture_regenerates_from_the_reference(tmp_path):
    """tests/golden/rpr/rpr_affine.ovg is what tools/rpr_golden/gen_rpr_affine.c writes; re-run it where the compiled reference exists."""
    _need_reference()
    subprocess.check_call(["make", "-s", "-C", str(ROOT / "tools" / "rpr_golden"), "_build/gen_rpr_affine"])
    subprocess.check_call([str(ROOT / "tools" / "rpr_golden" / "_build" / "gen_rpr_affine"), str(tmp_path)], stderr=subprocess.DEVNULL)
    assert (tmp_path / "rpr_affine.ovg").read_bytes() == (ROOT / "tests" / "golden" / "rpr" / "rpr_affine.ovg").read_bytes()
    assert (ROOT / "tests" / "golden" / "rpr" / "rpr_affine.ovg").stat().st_size <= 1 << 20


def test_shim_slots_record_what_the_direct_call_records():
    """The generator's second mode: the fixture's slot calls through the shim's table bound to a recorder."""
    _need_reference()
    if not (ROOT / "shim" / "_build" / "librcn_hip.so").exists():
        pytest.skip("shim not built")
    subprocess.check_call(["make", "-s", "-C", str(ROOT / "tools" / "rpr_golden"), "_build/gen_rpr_affine_shim"])
    subprocess.check_call([str(ROOT / "tools" / "rpr_golden" / "_build" / "gen_rpr_affine_shim")], stderr=subprocess.DEVNULL)
